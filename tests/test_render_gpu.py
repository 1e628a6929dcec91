"""GPU (-m gpu): rendering of detection results (csrc/render.hip through db_text_minimal_amd.render), bit for bit against the
restatement tests/render_ref.py: every operation is integer or uncontracted fp32 / fp64 in a fixed order, so nothing here is
a tolerance.  Mixed batches of outlines and heat maps, the autoscale reduction, untouched inputs, fully written outputs
with guards, render_detections against its two calls, and end to end from a probability map through detect_boxes."""
import numpy as np
import pytest
import torch

from db_text_minimal_amd import (detect_boxes, draw_outlines, image_collate, image_views, minmax_scale_u8, overlay_heatmap,
                                 render_detections)
from db_text_minimal_amd import render as Rn
from db_text_minimal_amd import packed as Pk
from db_text_minimal_amd._lib import check, lib
import render_ref as R
from gpu_util import DEV

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (5, 3), (37, 53), (64, 1), (720, 1280), (2160, 3840)]


def _image(rng, H, W):
    y, x = np.mgrid[0:H, 0:W]
    base = (np.stack([x * 7 + y * 3, x * 2 - y * 5, (x ^ y) * 11], -1) % 256).astype(np.uint8)
    noise = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return np.where(rng.random((H, W, 1)) < 0.3, noise, base).astype(np.uint8)


def _packed(imgs):
    return torch.from_numpy(np.concatenate([i.reshape(-1) for i in imgs])).to(DEV), [i.shape[:2] for i in imgs]


def _split(packed, shapes):
    return [v.cpu().numpy() for v in image_views(packed, shapes)]


def _shapes_for(rng, H, W, n, pts=4):
    """n shapes of `pts` vertices: inside, straddling the border, fully outside, degenerate (repeated points, zero area,
    a single repeated point) and, once, at the ends of the int16 range"""
    out = []
    for k in range(n):
        kind = k % 6
        c = rng.uniform(-0.2, 1.2, 2) * (W, H)
        s = rng.uniform(2, 0.4 * max(H, W) + 3)
        if kind == 0:
            p = c + rng.uniform(-s, s, (pts, 2))
        elif kind == 1:   # straddles a corner
            p = np.array([0, 0]) + rng.uniform(-s, s, (pts, 2))
        elif kind == 2:   # outside
            p = np.array([W, H]) * rng.uniform(1.5, 3, 2) * rng.choice([-1, 1], 2) + rng.uniform(-20, 20, (pts, 2)) + 3 * max(W, H)
        elif kind == 3:   # repeated points
            p = np.repeat(c[None] + rng.uniform(-s, s, (1, 2)), pts, 0)
            p[pts // 2:] = c
        elif kind == 4:   # zero area
            p = c + np.outer(np.linspace(-1, 1, pts), rng.uniform(-s, s, 2))
        else:
            p = c + rng.uniform(-s, s, (pts, 2)) * (1, 0.05)
        out.append(np.round(p))
    out = np.clip(np.array(out), -32768, 32767)
    if n > 6:
        out[6] = [[-32768, -32768], [32767, -30000], [32767, 32767], [-32768, 20000]][:pts] if pts == 4 else out[6]
    return out.astype(np.int16)


def _batch_shapes(rng, t):
    per = []
    for n, (H, W) in enumerate(SHAPES):
        k = 14 if H * W < 10 ** 6 else (8 if t < 100 else 3)
        b = _shapes_for(rng, H, W, k, 4)
        if n % 2 == 0:
            per.append(b)                                                          # int16 [K, 4, 2] boxes
        else:
            pl = [p.astype(np.int64) for p in _shapes_for(rng, H, W, k, 7)]
            pl += [np.array([[W // 2, H // 2]], np.int64), np.array([[0, 0], [W + 5, H + 2]], np.int64)]  # a point, a two-gon
            per.append(pl)                                                         # a list of int64 [P, 2] polygons
    return per


@pytest.mark.parametrize('t', [1, 2, 3, 8, 255])
def test_outlines_bit_exact_on_mixed_batch(t):
    rng = np.random.default_rng(100 + t)
    imgs = [_image(rng, H, W) for H, W in SHAPES]
    per = _batch_shapes(rng, t)
    packed, shapes = _packed(imgs)
    before = packed.clone()
    color = (255, 0, 0) if t != 8 else (7, 250, 33)
    out = draw_outlines((packed, shapes), per, color, t)
    out2 = draw_outlines((packed, shapes), per, color, t)
    torch.cuda.synchronize()
    assert out.is_cuda and out.dtype == torch.uint8 and out.shape == packed.shape
    assert torch.equal(packed, before) and torch.equal(out, out2)  # the input is not written; two runs agree
    painted = 0
    for n, got in enumerate(_split(out, shapes)):
        ref = R.draw_outlines(imgs[n], per[n], color, t)
        assert np.array_equal(got, ref), (t, n, np.argwhere((got != ref).any(-1))[:4])
        painted += int((ref != imgs[n]).any(-1).sum())
    assert painted > 1000


def test_more_than_65535_boxes_in_one_call():
    rng = np.random.default_rng(7)
    imgs = [_image(rng, 37, 53), _image(rng, 200, 311)]
    boxes = []
    for (H, W), k in zip([(37, 53), (200, 311)], [30000, 36001]):
        c = rng.integers(-3, [W + 3, H + 3], (k, 1, 2))
        boxes.append((c + rng.integers(-4, 5, (k, 4, 2))).astype(np.int16))
    packed, shapes = _packed(imgs)
    # few pixels stay unpainted under so many boxes unless they are sparse: only every 40th box of image 1 is its own
    boxes[1][0] = [[20, 30], [90, 35], [88, 60], [18, 50]]
    boxes[1][np.arange(len(boxes[1])) % 40 != 0, :, :] = boxes[1][0]
    assert sum(int((b.reshape(len(b), -1).astype(np.int64).sum(1) > 0).sum()) for b in boxes) > 65535
    out = draw_outlines((packed, shapes), boxes, (1, 2, 3), 2)
    torch.cuda.synchronize()
    for n, got in enumerate(_split(out, shapes)):
        ref = R.draw_outlines(imgs[n], boxes[n], (1, 2, 3), 2)
        assert np.array_equal(got, ref), n
    ref1 = R.stroke_mask(200, 311, boxes[1], 2)
    assert 0.02 < ref1.mean() < 0.98


def test_polygon_with_the_maximum_vertex_count():
    """a polygon with as many vertices as detect_polygons' vertex buffer holds for one 640 x 640 map"""
    cap = int(lib().dbn_detect_poly_verts_cap(1, 640, 640))
    assert cap == 2 * 640 * 640 + 1280
    rng = np.random.default_rng(8)
    loop = np.round(np.stack([150 + 120 * np.cos(np.linspace(0, 2 * np.pi, 97)[:-1] * 5), 100 + 90 * np.sin(np.linspace(0, 2 * np.pi, 97)[:-1] * 3)], 1))
    poly = np.tile(loop, (cap // len(loop) + 1, 1))[:cap].astype(np.int64)
    img = _image(rng, 200, 300)
    t = torch.from_numpy(img).to(DEV)
    for th in (1, 3):
        out = draw_outlines(t, [[poly]], (0, 255, 0), th)
        torch.cuda.synchronize()
        ref = R.draw_outlines(img, [poly], (0, 255, 0), th)
        assert np.array_equal(_split(out, [(200, 300)])[0], ref) and (ref != img).any()
    assert Rn.stroke_edges([[poly]], 1).shape == (cap, 5)


def test_single_image_empty_lists_and_host_batch():
    rng = np.random.default_rng(9)
    img = _image(rng, 30, 40)
    box = np.array([[[3, 4], [30, 4], [30, 20], [3, 20]]], np.int16)
    t = torch.from_numpy(img).to(DEV)
    ref = R.draw_outlines(img, box)
    for arg in (box, [box], (box, np.ones(1, np.float32)), [[box[0].astype(np.int64)]]):
        out = draw_outlines(t, arg)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().reshape(30, 40, 3), ref)
    for arg in ([[]], [np.zeros((0, 4, 2), np.int16)], [np.zeros((3, 4, 2), np.int16)], [([], [])]):
        out = draw_outlines(t, arg)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().reshape(30, 40, 3), img)
    imgs = [img, _image(rng, 50, 20)]
    batch = image_collate([(i, [], None) for i in imgs])
    assert not batch[0].is_cuda
    out = draw_outlines(batch, [box, []], thickness=1)
    torch.cuda.synchronize()
    got = _split(out, batch[1])
    assert np.array_equal(got[0], R.draw_outlines(img, box, thickness=1)) and np.array_equal(got[1], imgs[1])


# ---- heat map ----------------------------------------------------------------------------------------------------------------
def _maps(rng, N, C=2, S=640):
    y, x = np.mgrid[0:S, 0:S].astype(np.float32)
    out = np.empty((N, C, S, S), np.float32)
    for n in range(N):
        blob = np.exp(-(((x - rng.uniform(0, S)) / 90) ** 2 + ((y - rng.uniform(0, S)) / 60) ** 2))
        out[n, 0] = (0.7 * blob + 0.3 * rng.random((S, S))).astype(np.float32)
        out[n, 1:] = 7.0  # the other channels must not be read
    return out


VALID = [(640, 640), (640, 384), (443, 640), (640, 10), (360, 640), (1, 640)]


@pytest.mark.parametrize('cmap, alpha, binary', [('inferno', 0.6, None), ('jet', 0.35, None), ('jet', 0.6, 0.45)])
def test_heatmap_bit_exact_on_mixed_batch(cmap, alpha, binary):
    rng = np.random.default_rng(11)
    imgs = [_image(rng, H, W) for H, W in SHAPES]
    prob = _maps(rng, len(SHAPES))
    prob[2, 0, :VALID[2][0], :VALID[2][1]] *= 0.5
    prob[2, 0, VALID[2][0] - 1, VALID[2][1] - 1] = 0.93   # the maximum in the last valid row and column ...
    prob[4, 0, VALID[4][0] - 1, 0] = -0.25                # ... a minimum in the last row
    prob[3, 0] = 0.5                                      # a constant map
    packed, shapes = _packed(imgs)
    before = packed.clone()
    pd = torch.from_numpy(prob).to(DEV)
    Rn.LAUNCH_LOG.clear()
    out = overlay_heatmap((packed, shapes), pd, VALID, cmap, alpha, binary=binary)
    assert Rn.LAUNCH_LOG == ['dbn_render_minmax', 'dbn_render_paint']
    out2 = overlay_heatmap((packed, shapes), pd, VALID, cmap, alpha, binary=binary)
    torch.cuda.synchronize()
    assert torch.equal(packed, before) and torch.equal(out, out2)
    for n, got in enumerate(_split(out, shapes)):
        ref = R.overlay_heatmap(imgs[n], prob[n, 0], VALID[n], cmap, alpha, binary=binary)
        assert np.array_equal(got, ref), (n, int((got != ref).sum()))
    # explicit limits: no reduction launch; one number, or one per image; a 3-D map
    lo, hi = [0.0, 0.1, 0.2, 0.5, -1.0, 0.3], [1.0, 0.7, 0.9, 0.5, 2.0, 0.31]
    Rn.LAUNCH_LOG.clear()
    out = overlay_heatmap((packed, shapes), pd[:, 0].contiguous(), VALID, cmap, alpha, vmin=lo, vmax=hi, binary=binary)
    assert Rn.LAUNCH_LOG == ['dbn_render_paint']
    torch.cuda.synchronize()
    for n, got in enumerate(_split(out, shapes)):
        ref = R.overlay_heatmap(imgs[n], prob[n, 0], VALID[n], cmap, alpha, lo[n], hi[n], binary)
        assert np.array_equal(got, ref), (n, int((got != ref).sum()))


def _decode(keys):
    k = keys.astype(np.uint32)
    bits = np.where(k & 0x80000000, k & 0x7FFFFFFF, ~k).astype(np.uint32)
    return bits.view(np.float32)


def test_autoscale_limits_equal_the_restatement():
    rng = np.random.default_rng(12)
    shapes = [(3, 1500), (641, 1283), (1, 1), (1280, 1280)]
    prob = _maps(rng, 4, 1)
    prob[1, 0, -1, -1], prob[1, 0, -1, 0] = 5.0, -3.0
    prob[2, 0] = -0.0
    prob[3, 0] -= 0.5
    valid = [(640, 640), (640, 640), (640, 640), (333, 640)]
    desc, coef, auto = Rn.overlay_plan(shapes, (640, 640), valid)
    assert auto
    pd = torch.from_numpy(prob).to(DEV)
    mm = torch.full((2 * 4 + 16, ), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    d, c = torch.from_numpy(desc).to(DEV), torch.from_numpy(coef).to(DEV)
    for _ in range(2):
        check(lib().dbn_render_minmax(d.data_ptr(), c.data_ptr(), 4, sum(h * w for h, w in shapes), pd.data_ptr(), pd.numel(), 640 * 640, 640, 0, 0.0,
                                      mm.data_ptr(), torch.cuda.current_stream().cuda_stream), 'render_minmax')
        torch.cuda.synchronize()
        host = mm.cpu().numpy()
        assert (host[8:] == 0x5A5A5A5A).all()
        keys = host[:8].view(np.uint32).reshape(4, 2)
        lo, hi = _decode(keys[:, 0]), _decode(~keys[:, 1])
        for n in range(4):
            v = R.resized_map(prob[n, 0], shapes[n], valid[n])
            assert lo[n] == v.min() and hi[n] == v.max(), (n, lo[n], v.min(), hi[n], v.max())
    assert hi[1] == 5.0 and lo[1] == -3.0  # the clamped corner pixels of an upscaled map are its corner values


@pytest.mark.parametrize('shapes, shift', [([(1, 1)], 0), ([(37, 53), (5, 3)], 0), ([(37, 53), (64, 1)], 1), ([(32, 32), (64, 48)], 0), ([(100, 41)], 3)])
def test_every_output_byte_written_and_nothing_past_it(shapes, shift):
    """the paint launch and the stroke launch into a poisoned buffer with a guard behind it (`shift`: an output that is not
    dword aligned); src stays as it was"""
    rng = np.random.default_rng(13)
    imgs = [_image(rng, H, W) for H, W in shapes]
    N = len(shapes)
    prob = rng.random((N, 1, 24, 40)).astype(np.float32)
    packed, _ = _packed(imgs)
    before = packed.clone()
    n = packed.numel()
    buf = torch.full((n + 4096 + shift, ), 0xA5, dtype=torch.uint8, device=DEV)
    dst = buf[shift:]
    desc, coef, _ = Rn.overlay_plan(shapes, (24, 40), None, 0.0, 1.0)
    d, c, pd = torch.from_numpy(desc).to(DEV), torch.from_numpy(coef).to(DEV), torch.from_numpy(prob).to(DEV)
    tab = Rn.colormap_table('inferno').astype(np.int64)
    lut = torch.from_numpy((tab[:, 0] | tab[:, 1] << 8 | tab[:, 2] << 16).astype(np.int32)).to(DEV)
    st = torch.cuda.current_stream().cuda_stream
    check(lib().dbn_render_paint(packed.data_ptr(), dst.data_ptr(), d.data_ptr(), c.data_ptr(), N, n // 3, pd.data_ptr(), pd.numel(), 24 * 40, 40, 0, 0.0,
                                 None, lut.data_ptr(), 0.6, st), 'render_paint')
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:shift] == 0xA5).all() and (host[shift + n:] == 0xA5).all() and torch.equal(packed, before)
    o = 0
    for i, (H, W) in enumerate(shapes):
        ref = R.overlay_heatmap(imgs[i], prob[i, 0], None, 'inferno', 0.6, 0.0, 1.0)
        assert np.array_equal(host[shift + o:shift + o + H * W * 3].reshape(H, W, 3), ref), i
        o += H * W * 3
    # strokes: dst = a copy of src plus the edges, nothing else
    buf.fill_(0xA5)
    boxes = [_shapes_for(rng, H, W, 9) for H, W in shapes]
    edges = torch.from_numpy(Rn.stroke_edges(boxes, N)).to(DEV)
    off = Pk.offsets([h * w * 3 for h, w in shapes])
    idesc = torch.from_numpy(np.stack([off[:-1], [h for h, _ in shapes], [w for _, w in shapes]], 1).astype(np.int64)).to(DEV)
    check(lib().dbn_draw_strokes(packed.data_ptr(), dst.data_ptr(), n, idesc.data_ptr(), N, edges.data_ptr(), len(edges), 3, 9, 8, 7, st), 'draw_strokes')
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:shift] == 0xA5).all() and (host[shift + n:] == 0xA5).all() and torch.equal(packed, before)
    o = 0
    for i, (H, W) in enumerate(shapes):
        assert np.array_equal(host[shift + o:shift + o + H * W * 3].reshape(H, W, 3), R.draw_outlines(imgs[i], boxes[i], (9, 8, 7), 3)), i
        o += H * W * 3


def test_render_detections_equals_its_two_calls():
    rng = np.random.default_rng(14)
    shapes = [(300, 500), (97, 61), (720, 1280)]
    imgs = [_image(rng, H, W) for H, W in shapes]
    per = [_shapes_for(rng, H, W, 12) for H, W in shapes]
    prob = torch.from_numpy(_maps(rng, 3)).to(DEV)
    packed, _ = _packed(imgs)
    before = packed.clone()
    both = render_detections((packed, shapes), prob, per, thickness=3, alpha=0.6)
    lines = draw_outlines((packed, shapes), per, thickness=3)
    kept = lines.clone()
    two = overlay_heatmap((packed, shapes), prob, out=lines)
    torch.cuda.synchronize()
    assert two.data_ptr() == lines.data_ptr() and torch.equal(both, two) and torch.equal(packed, before)
    assert torch.equal(render_detections((packed, shapes), prob, per, heatmap=False), kept)
    for n, got in enumerate(_split(both, shapes)):
        ref = R.overlay_heatmap(R.draw_outlines(imgs[n], per[n]), prob[n, 0].cpu().numpy())
        assert np.array_equal(got, ref), n


def test_end_to_end_from_probability_map():
    """rectangles in a probability map -> detect_boxes(dest_sizes) -> render_detections: with alpha = 0 the painted pixels
    are exactly the strokes of the returned boxes and every other pixel is the source's; with alpha = 1 and no shapes the
    output is the colour table applied to the resized map"""
    Hm, Wm = 128, 128
    sizes = [(256, 256), (200, 380)]
    rects = [[((10, 40, 10, 20), 0.9), ((60, 110, 30, 45), 0.99), ((20, 70, 70, 80), 0.75), ((100, 102, 100, 102), 0.9)],
             [((5, 120, 5, 25), 0.95), ((30, 60, 60, 100), 0.72)]]
    pred = torch.zeros((2, 1, Hm, Wm), dtype=torch.float32)
    for n, rs in enumerate(rects):
        for (x0, x1, y0, y1), p in rs:
            pred[n, 0, y0:y1, x0:x1] = p
    pred = pred.to(DEV)
    res = detect_boxes(pred, dest_sizes=sizes)
    rng = np.random.default_rng(15)
    imgs = [_image(rng, H, W) for H, W in sizes]
    imgs = [np.where(i == 255, 254, i).astype(np.uint8) for i in imgs]  # no source pixel has the stroke's red byte
    batch = image_collate([(i, [], None) for i in imgs])
    out = render_detections(batch, pred, res, alpha=0.0)
    torch.cuda.synchronize()
    kept = 0
    for n, got in enumerate(_split(out, sizes)):
        mask = R.stroke_mask(sizes[n][0], sizes[n][1], res[n][0], 3)
        kept += len(R.select_shapes(res[n][0]))
        assert mask.any() and (got[mask] == (255, 0, 0)).all() and np.array_equal(got[~mask], imgs[n][~mask])
    assert kept == 5
    out = render_detections(batch, pred, [[], []], alpha=1.0)
    torch.cuda.synchronize()
    p = pred.cpu().numpy()
    for n, got in enumerate(_split(out, sizes)):
        col, idx, lim = R.colorize(R.resize_linear_f32(p[n, 0], *sizes[n]), 'inferno')
        assert np.array_equal(got, col) and lim[0] == 0.0 and idx.max() == 255 and idx.min() == 0


def test_minmax_scale_u8():
    rng = np.random.default_rng(16)
    for shape in [(3, 3, 17, 23), (1, 3, 1, 1), (2, 3, 64, 64), (2, 3, 5, 1)]:
        x = rng.normal(0, 60, shape).astype(np.float32)
        x[0, 0, 0, 0], x[0, 1, -1, -1] = -200.0, 100.0  # max - min = 300: an inexact factor
        if shape[0] > 1:
            x[1] = 2.5  # a constant image
        out = minmax_scale_u8(torch.from_numpy(x).to(DEV))
        torch.cuda.synchronize()
        assert out.shape == (shape[0], shape[2], shape[3], 3) and out.dtype == torch.uint8
        for n in range(shape[0]):
            assert np.array_equal(out[n].cpu().numpy(), R.minmax_scale_u8(x[n])), (shape, n)
    one = minmax_scale_u8(torch.from_numpy(x[0]).to(DEV))
    assert np.array_equal(one.cpu().numpy(), R.minmax_scale_u8(x[0]))
