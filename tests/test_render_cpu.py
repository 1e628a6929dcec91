"""CPU (-m "not gpu"): the restatement tests/render_ref.py that the device rendering (db_text_minimal_amd.render,
csrc/render.hip) is compared with: strokes with known answers and against Python-integer arithmetic, the colour layer
against matplotlib itself, minmax_scale_u8 against the numpy expression of the reference, the float resize against values
worked out by hand, and the argument checks of the public functions."""
import numpy as np
import pytest
import torch

from db_text_minimal_amd import render as Rn
import render_ref as R


# ---- strokes -----------------------------------------------------------------------------------------------------------
def _rect(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.int64)


def test_axis_aligned_rectangle_known_answer():
    H, W, (x0, y0, x1, y1) = 40, 50, (10, 8, 30, 25)
    m3 = R.stroke_mask(H, W, [_rect(x0, y0, x1, y1)], 3)
    want = np.zeros((H, W), bool)
    want[y0 - 1:y1 + 2, x0 - 1:x1 + 2] = True
    want[y0 + 2:y1 - 1, x0 + 2:x1 - 1] = False
    assert np.array_equal(m3, want)
    m1 = R.stroke_mask(H, W, [_rect(x0, y0, x1, y1)], 1)
    want = np.zeros((H, W), bool)
    want[y0:y1 + 1, x0:x1 + 1] = True
    want[y0 + 1:y1, x0 + 1:x1] = False
    assert np.array_equal(m1, want)


@pytest.mark.parametrize('t', [1, 2, 3, 4, 7, 8, 25])
def test_single_point_is_a_disc(t):
    H = W = 61
    m = R.stroke_mask(H, W, [np.array([[30, 29]])], t)
    y, x = np.mgrid[0:H, 0:W]
    want = 4 * ((x - 30) ** 2 + (y - 29) ** 2) <= t * t if t > 1 else (x == 30) & (y == 29)
    assert np.array_equal(m, want)


def _random_polygon(rng, n, lo, hi):
    return rng.integers(lo, hi, (n, 2)).astype(np.int64)


def test_thin_line_lies_inside_the_thick_stroke_and_symmetries():
    """thickness >= 2: the stroke is a union of per-edge sets that do not depend on an edge's direction, so it is
    invariant under reversing the vertex order and rotating the start vertex.  thickness 1: dbn_on_line orders each
    edge left to right (top to bottom for a vertical one) before stepping, so the same holds."""
    rng = np.random.default_rng(1)
    H, W = 90, 120
    painted = 0
    for trial in range(12):
        p = _random_polygon(rng, int(rng.integers(2, 9)), -20, 140)
        thin = R.stroke_mask(H, W, [p], 1)
        painted += int(thin.sum())
        assert not (thin & ~R.stroke_mask(H, W, [p], 2)).any()
        for t in (1, 2, 3, 8):
            m = R.stroke_mask(H, W, [p], t)
            assert np.array_equal(m, R.stroke_mask(H, W, [p[::-1]], t)), (trial, t)
            assert np.array_equal(m, R.stroke_mask(H, W, [np.roll(p, 3, 0)], t)), (trial, t)
    assert painted > 1000


def test_stroke_predicate_against_python_integers():
    """random segments, with coordinates at the ends of the int16 range and of the polygon range, image sides of 65 535:
    the int64 predicate equals the Python-integer one on pixels sampled near the segment and anywhere in the image"""
    rng = np.random.default_rng(2)
    S = 65535
    ends = [-32768, 32767, 0, S - 1, -2 ** 20, 2 ** 20]
    checked = hits = 0
    for trial in range(300):
        pts = [int(rng.choice(ends)) if rng.random() < 0.4 else int(rng.integers(-40000, 70000)) for _ in range(4)]
        xa, ya, xb, yb = pts
        if trial % 10 == 0:
            xb, yb = xa, ya  # a point
        t = int(rng.choice([2, 3, 8, 254, 255]))
        # pixels near the segment: a point of it plus a small offset, clipped to the image; and uniform ones
        s = rng.random(40)
        off = rng.integers(-t, t + 1, (40, 2))
        px = np.clip(np.round(xa + s * (xb - xa)).astype(np.int64) + off[:, 0], 0, S - 1)
        py = np.clip(np.round(ya + s * (yb - ya)).astype(np.int64) + off[:, 1], 0, S - 1)
        px = np.r_[px, rng.integers(0, S, 10), 0, S - 1]
        py = np.r_[py, rng.integers(0, S, 10), S - 1, 0]
        got = R.stroke_hit(px, py, xa, ya, xb, yb, t)
        want = np.array([R.stroke_hit_exact(x, y, xa, ya, xb, yb, t) for x, y in zip(px, py)])
        assert np.array_equal(got, want), (xa, ya, xb, yb, t)
        checked += len(px)
        hits += int(want.sum())
    assert hits > checked // 20  # the sample does reach the strokes


def test_on_line_matches_stepping_the_line():
    """the closed form equals a walk of the 8-connected line (one pixel per major step, minor = round half down), also for an
    edge longer than 32 767 pixels, where 32-bit products would overflow"""
    for xa, ya, xb, yb in [(3, 4, 40, 17), (40, 17, 3, 4), (5, 50, 9, 2), (7, 7, 7, 30), (2, 9, 30, 9), (4, 4, 4, 4), (-32768, -5, 32767, 40000)]:
        dx, dy = xb - xa, yb - ya
        n = max(abs(dx), abs(dy))
        x1, y1, x2, y2 = (xa, ya, xb, yb) if dx > 0 or (dx == 0) else (xb, yb, xa, ya)
        px, py = [], []
        for i in range(0, n + 1, 1 if n < 1000 else 997):
            if abs(dy) > abs(dx):
                sy = 1 if y2 >= y1 else -1
                px.append(x1 + (2 * (x2 - x1) * i + n - 1) // (2 * n))
                py.append(y1 + sy * i)
            else:
                sy = 1 if y2 >= y1 else -1
                px.append(x1 + i)
                py.append(y1 + sy * ((2 * abs(y2 - y1) * i + n - 1) // (2 * n) if n else 0))
        px, py = np.array(px), np.array(py)
        assert R.on_line(px, py, xa, ya, xb, yb).all(), (xa, ya, xb, yb)
        assert not R.on_line(px + 1, py + 1, xa, ya, xb, yb).all() or n == 0 or abs(dx) == abs(dy)


def test_dropped_shapes_and_edges():
    boxes = np.array([_rect(2, 2, 9, 9), np.zeros((4, 2)), _rect(-5, -5, 1, 2)], np.int16)  # the last sums to -14
    e = Rn.stroke_edges([boxes, []], 2)
    assert e.dtype == np.int32 and e.shape == (4, 5) and (e[:, 0] == 0).all()
    assert e[0].tolist() == [0, 2, 9, 2, 2] and e[1].tolist() == [0, 2, 2, 9, 2]  # edge 0 comes from the last vertex
    assert len(R.select_shapes(boxes)) == 1
    polys = ([np.array([[1, 1], [5, 1], [5, 6]]), np.array([[0, 0]])], [0.9, 0.8])  # a detect_polygons pair
    e = Rn.stroke_edges([(boxes, np.ones(3, np.float32)), polys], 2)
    assert e.shape == (7, 5) and e[4:, 0].tolist() == [1, 1, 1]
    assert Rn.stroke_edges(boxes, 1).shape == (4, 5) and Rn.stroke_edges([np.array([[3, 3]])], 1).tolist() == [[0, 3, 3, 3, 3]]


# ---- colour layer, against matplotlib itself -------------------------------------------------------------------------------
def _mpl_bytes(name, x, vmin, vmax):
    from matplotlib import colormaps
    from matplotlib.colors import Normalize
    return colormaps[name](Normalize(vmin, vmax)(x), bytes=True)[..., :3]


def _separating_values(vmin, vmax, rng, want=200):
    """float32 inputs on which an all-float32 or an all-float64 evaluation of t picks another table entry than numpy's
    mixed evaluation (double arithmetic, float32 stores): values next to the points where t * 256 crosses an integer"""
    k = rng.integers(1, 256, 4000)
    x = (vmin + (vmax - vmin) * k / 256.0).astype(np.float32)
    x = np.nextafter(x, np.float32(np.inf) * rng.choice([-1, 1], x.shape).astype(np.float32)) if rng.random() < 0.5 else x
    x = np.concatenate([x, np.nextafter(x, np.float32(-np.inf)), np.nextafter(x, np.float32(np.inf))])
    mixed = R.color_index(R.normalize(x, vmin, vmax))
    f32 = R.color_index((x - np.float32(vmin)) / (np.float32(vmax) - np.float32(vmin)))
    f64 = R.color_index(((x.astype(np.float64) - vmin) / (vmax - vmin)).astype(np.float32))
    sep32, sep64 = x[mixed != f32], x[mixed != f64]
    return sep32[:want], sep64[:want]


@pytest.mark.parametrize('name', ['inferno', 'jet'])
def test_colour_layer_equals_matplotlib(name):
    pytest.importorskip('matplotlib')
    rng = np.random.default_rng(3)
    cases = [(rng.random((37, 41)).astype(np.float32), None, None),
             ((rng.random((29, 31)) * 3 - 1).astype(np.float32), None, None),          # values outside 0 .. 1, autoscaled
             ((rng.random((29, 31)) * 3 - 1).astype(np.float32), 0.0, 1.0),            # ... and clipped by explicit limits
             (np.full((5, 7), 0.37, np.float32), None, None),                          # constant
             (np.full((5, 7), 0.37, np.float32), 0.37, 0.37),
             (np.array([[0.1, 0.7, 0.4, 0.7000001, 0.69999995]], np.float32), 0.1, 0.7),  # holds vmax (0.7 in float32 is not 0.7)
             (np.array([[0.25, 0.5, 1.0, 0.0, -0.0]], np.float32), 0.0, 1.0),             # t = 1 exactly -> entry 255
             (rng.random((64, 64)).astype(np.float32), 0.123, 0.877),
             (rng.random((64, 64)).astype(np.float32) * 1e-3, None, None)]
    n_sep32 = n_sep64 = 0
    for vmin, vmax in [(0.1, 0.7), (0.123, 0.877), (-0.3, 2.2), (1e-3, 0.999)]:
        s32, s64 = _separating_values(vmin, vmax, rng)
        n_sep32 += len(s32)
        n_sep64 += len(s64)
        cases.append((np.concatenate([s32, s64, np.float32([vmin, vmax])])[None, :], vmin, vmax))
    # the search found inputs that tell numpy's mixed evaluation from a pure float32 and from a pure float64 one
    assert n_sep32 > 0 and n_sep64 > 0, (n_sep32, n_sep64)
    for x, vmin, vmax in cases:
        col, idx, _ = R.colorize(x, name, vmin, vmax)
        want = _mpl_bytes(name, x.copy(), vmin, vmax)
        assert col.dtype == np.uint8 and np.array_equal(col, want), (name, vmin, vmax, int((col != want).any(-1).sum()))
        assert idx.min() >= 0 and idx.max() <= 255


def test_committed_tables_equal_matplotlib():
    pytest.importorskip('matplotlib')
    from matplotlib import colormaps
    for name in Rn.CMAPS:
        want = colormaps[name](np.arange(256), bytes=True)[:, :3]
        assert np.array_equal(Rn.colormap_table(name), want) and np.array_equal(R.table(name), want)
        cm = colormaps[name]
        if not cm._isinit:
            cm._init()
        lut = cm._lut
        assert np.array_equal(want, (lut[:256, :3] * 255).astype(np.uint8))


def test_blend_rounds_half_to_even_in_float32():
    img = np.array([[[0, 1, 2]], [[3, 255, 10]]], np.uint8)
    col = np.array([[[1, 2, 3]], [[0, 255, 11]]], np.uint8)
    # alpha = 0.5: (a + b) / 2 exactly; halves go to the even neighbour
    assert R.blend(img, col, 0.5).reshape(-1).tolist() == [0, 2, 2, 2, 255, 10]
    assert np.array_equal(R.blend(img, col, 0.0), img) and np.array_equal(R.blend(img, col, 1.0), col)
    a = np.float32(0.6)
    want = np.rint(np.float32(200) * (np.float32(1) - a) + np.float32(17) * a)
    assert R.blend(np.full((1, 1, 3), 200, np.uint8), np.full((1, 1, 3), 17, np.uint8), 0.6)[0, 0, 0] == int(want)


# ---- minmax_scale_u8 -------------------------------------------------------------------------------------------------------
def test_minmax_scale_equals_the_numpy_expression():
    rng = np.random.default_rng(4)
    cases = [rng.normal(0, 60, (3, 17, 23)).astype(np.float32), rng.random((3, 8, 9)).astype(np.float32),
             (rng.random((3, 8, 9)) * 3).astype(np.float32)]
    x = rng.random((3, 6, 5)).astype(np.float32)
    x[0, 0, 0], x[1, 2, 3] = 0.0, 3.0  # max - min = 3: 1 / 3 and 255 / 3 are inexact in float32
    cases.append(x)
    for x in cases:
        img = x.transpose(1, 2, 0)  # utils.py:126, then :110-113 typed out:
        want = ((img - img.min()) * (1 / (img.max() - img.min()) * 255)).astype('uint8')
        got = R.minmax_scale_u8(x)
        assert got.dtype == np.uint8 and np.array_equal(got, want)
        assert got.max() >= 254 and got.min() == 0
    assert not R.minmax_scale_u8(np.full((3, 4, 4), 2.5, np.float32)).any()


# ---- resize ----------------------------------------------------------------------------------------------------------------
def test_resize_known_answers():
    rng = np.random.default_rng(5)
    src = rng.random((13, 17)).astype(np.float32)
    assert np.array_equal(R.resize_linear_f32(src, 13, 17), src)  # identity
    assert np.array_equal(R.resize_linear_f32(np.full((7, 5), 0.3, np.float32), 40, 33), np.full((40, 33), 0.3, np.float32))
    # 2x upscaling of the ramp 0, 4, 8, 12: source position (d + 0.5) / 2 - 0.5 = -0.25, 0.25, 0.75, ... -> the left edge is
    # clamped, interior samples sit a quarter or three quarters of the way, the right edge is clamped
    ramp = np.array([[0, 4, 8, 12]], np.float32)
    assert R.resize_linear_f32(ramp, 1, 8)[0].tolist() == [0, 1, 3, 5, 7, 9, 11, 12]
    assert R.resize_linear_f32(ramp.T.copy(), 8, 1)[:, 0].tolist() == [0, 1, 3, 5, 7, 9, 11, 12]
    for hw in [(5, 9), (64, 64), (200, 31), (1, 1)]:
        out = R.resize_linear_f32(src, *hw)
        assert out.shape == hw and out.dtype == np.float32
        # a convex combination in float32: at most a few ulp outside the source's range
        assert out.min() >= src.min() - 1e-6 and out.max() <= src.max() + 1e-6


# ---- argument checks (before any launch: none of these reaches the device) ---------------------------------------------------
def test_argument_errors():
    img = torch.zeros((8, 9, 3), dtype=torch.uint8)
    box = np.array([_rect(1, 1, 5, 5)], np.int16)
    with pytest.raises(ValueError):
        Rn.draw_outlines(img, [box], thickness=0)
    with pytest.raises(ValueError):
        Rn.draw_outlines(img, [box], thickness=256)
    with pytest.raises(ValueError):
        Rn.draw_outlines(img, [box], color=(256, 0, 0))
    with pytest.raises(ValueError):
        Rn.draw_outlines(img, [box, box])
    with pytest.raises(ValueError):
        Rn.draw_outlines(img, [np.array([[[1.5, 2.0]]])])
    with pytest.raises(ValueError):
        Rn.draw_outlines(img, [[np.array([[2 ** 20 + 1, 0]])]])
    with pytest.raises(ValueError):
        Rn.draw_outlines(torch.zeros((8, 9), dtype=torch.uint8), [box])
    with pytest.raises(ValueError):
        Rn.overlay_heatmap(img, torch.zeros((1, 4, 4)))  # not a device tensor
    with pytest.raises(ValueError):
        Rn.overlay_plan([(8, 9)], (4, 4), vmin=0.0)
    with pytest.raises(ValueError):
        Rn.overlay_plan([(8, 9)], (4, 4), vmin=1.0, vmax=0.0)
    with pytest.raises(ValueError):
        Rn.overlay_plan([(8, 9)], (4, 4), valid_hw=[(5, 4)])
    with pytest.raises(ValueError):
        Rn.colormap_table('viridis')
    with pytest.raises(ValueError):
        Rn.minmax_scale_u8(torch.zeros((2, 3, 4, 4)))
    desc, coef, auto = Rn.overlay_plan([(8, 9), (2, 3)], (4, 6), valid_hw=[(4, 6), (3, 2)], vmin=0.0, vmax=[1.0, 2.0])
    assert not auto and desc.tolist() == [[0, 8, 9, 4, 6], [72, 2, 3, 3, 2]]
    assert coef[:, 2:].tolist() == [[0.0, 1.0], [0.0, 2.0]] and coef[0, 0] == 1. / (9. / 6.) and coef[1, 1] == 1. / (2. / 3.)
    assert Rn.overlay_plan([(8, 9)], (4, 4))[2]
