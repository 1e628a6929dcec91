"""CPU (-m "not gpu"): the synthetic scene text without a device.  The numpy restatement tests/synth_ref.py (what
the device is compared with byte for byte) against matplotlib's containment test on the CURVED outlines under affine maps, against its
Python-integer twin, under rotations and a mirror, and on known answers; the planner, the records and bins of
db_text_minimal_amd.synth against plain loops; the refusals of the entry point before any launch."""
import math
import os

import numpy as np
import pytest

from db_text_minimal_amd import _lib, gt_maps
from db_text_minimal_amd import synth as S
from db_text_minimal_amd.render import glyph_table
import synth_ref as R

VISIBLE = ''.join(chr(c) for c in range(33, 127))
L = R.L


def matrix(cap, degrees, shear=0.0, mirror=False):
    """the quantised matrix of an upright glyph of cap height `cap` px, sheared, then rotated by `degrees` in image coordinates"""
    k = cap / R.font()['head']['cap_height']
    c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    A = np.array([[c, -s], [s, c]]) @ np.array([[1.0, -shear], [0.0, 1.0]]) @ np.diag([-k if mirror else k, -k])
    return [int(v) for v in np.rint(A.reshape(-1) * L)]


# ---- the predicate -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cap,degrees,shear,n', [(8, 17, 0.2, 4), (16, -33, 0, 4), (40, 90, -0.3, 4), (40, 180, 0, 1), (6, 11, 0, 4)])
def test_predicate_under_an_affine_map_against_matplotlib(cap, degrees, shear, n):
    """The restatement fills chords of the table under the quantised matrix, matplotlib its own flattening of the curves, so samples on
    the outline may differ: at most 0.5 % of the inside ones, the bound of the labels.  Using the table's edge array
    without the edges that are horizontal in font units made 22 - 58 % wrong.  Measured: printed below, recorded in DESIGN section 41."""
    pytest.importorskip('matplotlib')
    import matplotlib
    from matplotlib.ft2font import FT2Font, LoadFlags
    from matplotlib.path import Path
    ft = FT2Font(os.path.join(matplotlib.get_data_path(), 'fonts', 'ttf', 'DejaVuSans.ttf'), hinting_factor=1)
    a = matrix(cap, degrees, shear)
    inv = np.linalg.inv(np.array(a, np.float64).reshape(2, 2))
    inside = differ = 0
    for ch in VISIBLE:
        contours = R.font()['contours'][R.glyph_of(ch)]
        box = R.instance_box(a, (0, 0), R.box_of(contours))
        t = (2 * L + 13 * 4099 - box[0], 2 * L + 37 * 4099 - box[1])  # two pixels of room, at a generic sub-pixel position
        H, W = (box[3] - box[1]) // L + 5, (box[2] - box[0]) // L + 5
        ref = R.samples_inside(H, W, contours, a, t, n)
        assert not ref[0].any() and not ref[-1].any() and not ref[:, 0].any() and not ref[:, -1].any()  # nothing is clipped
        ky, kx = np.mgrid[0:H * n, 0:W * n]
        lat = np.stack([kx.reshape(-1) * (L // n) + L // (2 * n) - t[0], ky.reshape(-1) * (L // n) + L // (2 * n) - t[1]], 1).astype(np.float64)
        pts = lat @ inv.T  # the samples in font units
        ft.load_char(ord(ch), flags=LoadFlags.NO_SCALE)
        verts, codes = ft.get_path()
        v = np.asarray(verts, np.float64) * 64
        starts = [i for i, c in enumerate(codes) if c == Path.MOVETO] + [len(codes)]
        mpl = np.zeros(len(pts), bool)
        for s0, s1 in zip(starts[:-1], starts[1:]):
            mpl ^= Path(v[s0:s1], codes[s0:s1]).contains_points(pts)
        inside += int(ref.sum())
        differ += int((ref.reshape(-1) != mpl).sum())
    print('cap %g, %g degrees, shear %g, %d per axis: %d of %d inside samples differ (%.2f %%)' % (cap, degrees, shear, n, differ, inside, 100.0 * differ / inside))
    assert inside > 1000 and differ <= 0.005 * inside


def test_vectorised_predicate_equals_python_integers():
    rng = np.random.default_rng(1)
    for ch, a in [('g', matrix(7.5, 17, 0.2)), ('@', matrix(256, 45, 0.3)), ('8', matrix(16, 90)), ('%', matrix(4, -120, -0.2, True))]:
        contours = R.font()['contours'][R.glyph_of(ch)]
        edges = R.edges_of(contours)
        te = R.transform(edges, a)
        lo, hi = te[:, [0, 2]].min(), te[:, [0, 2]].max()
        X = rng.integers(lo - 1000, hi + 1000, 300)
        Y = rng.integers(te[:, [1, 3]].min() - 1000, te[:, [1, 3]].max() + 1000, 300)
        Y[:40] = te[np.arange(40) % len(te), 1]  # at the height of a vertex
        X[:10] = te[np.arange(10) % len(te), 0]  # ... ten of them on the vertex itself
        got = R.winding(te, X, Y)
        assert got.tolist() == [R.winding_exact(edges, a, int(x), int(y)) for x, y in zip(X, Y)]
        assert set(got.tolist()) <= {0, 1, -1} and (got != 0).any()
    assert [R.blend_exact(c, k, f) for c, k, f in [(0, 8, 255), (0, 8, 1), (200, 0, 3), (7, 16, 90)]] == [128, 1, 200, 90]


@pytest.mark.parametrize('ch', ['R', 'g', '5', '&'])
def test_quarter_turns_and_mirror_give_the_turned_mask(ch):
    """About a pixel corner the sample grid maps onto itself under a quarter turn and under a mirror, so the mask turns exactly."""
    contours = R.font()['contours'][R.glyph_of(ch)]
    side, s = 64, 2 * 7001  # pixels; an even scale and an odd t: no sample shares a coordinate with a vertex
    c = side // 2 * L
    t0 = (c - 300 * s + 1, c + 500 * s + 3)
    up = R.samples_inside(side, side, contours, (s, 0, 0, -s), t0)
    assert up.sum() > 1000 and not up[0].any() and not up[-1].any() and not up[:, 0].any() and not up[:, -1].any()
    ky, kx = np.nonzero(up)
    u, v = 2 * kx + 1 - 4 * side, 2 * ky + 1 - 4 * side  # odd coordinates about the centre, in half sample steps
    rot = np.array([[0, -1], [1, 0]])
    M = np.eye(2, dtype=np.int64)
    for quarter in range(1, 4):
        M = rot @ M
        a = (M @ np.array([[s, 0], [0, -s]])).reshape(-1).tolist()
        t = (M @ (np.array(t0) - c) + c).tolist()
        got = R.samples_inside(side, side, contours, a, t)
        want = np.zeros_like(up)
        uu, vv = M[0, 0] * u + M[0, 1] * v, M[1, 0] * u + M[1, 1] * v
        want[(vv + 4 * side - 1) // 2, (uu + 4 * side - 1) // 2] = True
        assert np.array_equal(got, want), quarter
        assert np.array_equal(want, np.rot90(up, -quarter))
    mirrored = R.samples_inside(side, side, contours, (-s, 0, 0, -s), (2 * c - t0[0], t0[1]))  # det < 0
    assert np.array_equal(mirrored, up[:, ::-1]) and not np.array_equal(mirrored, up)


def test_known_answers_for_coverage_and_blend():
    rect = [np.array([[0, 0], [10, 0], [10, 5], [0, 5]], np.int64)]  # 2.5 x 1.25 pixels at a quarter pixel per unit
    cov = R.coverage(5, 6, rect, (L // 4, 0, 0, -(L // 4)), (L, 3 * L))  # x 1.0 .. 3.5, y 1.75 .. 3.0
    want = np.zeros((5, 6), np.int64)
    want[1, 1:4], want[2, 1:4] = (4, 4, 2), (16, 16, 8)
    assert np.array_equal(cov, want)
    cur = np.zeros((5, 6, 3), np.uint8)
    cur[..., 1], cur[..., 2] = 200, 7
    out = R.blend(cur, cov, (255, 1, 90))
    assert out[2, 3].tolist() == [128, (8 * 1 + 8 * 200 + 8) >> 4, (8 * 90 + 8 * 7 + 8) >> 4] and out[2, 3, 0] == 128  # 127.5 rounds up
    assert out[2, 1].tolist() == [255, 1, 90] and out[0, 0].tolist() == [0, 200, 7] and out[1, 3].tolist() == [(2 * 255 + 8) >> 4, (2 + 14 * 200 + 8) >> 4, (180 + 98 + 8) >> 4]
    assert R.blend(np.zeros((1, 1, 3), np.uint8), np.full((1, 1), 8), (1, 1, 1)).tolist() == [[[1, 1, 1]]]  # 0.5 rounds up


# ---- the background ------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    for counter, key, want in [((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
                               ((0xffffffff, ) * 4, (0xffffffff, ) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
                               ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1')]:
        assert ' '.join('%08x' % int(w) for w in R.philox(counter, key)) == want


def test_background_known_answers():
    flat = R.background(70, 90, (10, 200, 255), (0, 0, 0), 12345)
    assert (flat == np.array([10, 200, 255], np.uint8)).all()
    seed, base, amps = 0x0123456789ABCDEF, (100, 120, 90), (64, 24, 7)
    img = R.background(130, 70, base, amps, seed)
    # pixel (x 64, y 128) is a corner of every octave: T_o = C^2 n_o, so D = sum A_o (n_o - 128) 2^12
    n = [int(R.philox((64 // C, 128 // C, o, 0), (seed & 0xFFFFFFFF, seed >> 32))[0]) >> 24 for o, C in enumerate((64, 16, 4))]
    D = sum(a * (v - 128) * 4096 for a, v in zip(amps, n))
    move = (D + (1 << 18)) // (1 << 19)
    assert img[128, 64].tolist() == [min(255, max(0, b + move)) for b in base] and move != 0
    assert len(np.unique(img[..., 0])) > 20
    assert (np.diff(img.astype(np.int64), axis=2) == np.diff(base)).all()  # the channels move together (nothing clamps here)
    edge = R.background(130, 70, (3, 250, 128), amps, seed)
    assert edge.min() == 0 and edge.max() == 255 and np.array_equal(edge[..., 2], img[..., 0] + 28)  # ... and clamp each on its own
    other = R.background(130, 70, base, amps, seed ^ 1 << 40)  # the high word alone
    assert (other != img).mean() > 0.5


# ---- the planner ---------------------------------------------------------------------------------------------------
def _inside_polygon(poly, pts, slack):
    """pts inside the closed polygon, or within `slack` of its border"""
    a, b = poly, np.roll(poly, -1, 0)
    x, y = pts[:, 0][:, None], pts[:, 1][:, None]
    cross = ((a[:, 1] <= y) != (b[:, 1] <= y)) & (x < a[:, 0] + (y - a[:, 1]) * (b[:, 0] - a[:, 0]) / np.where(b[:, 1] == a[:, 1], 1.0, b[:, 1] - a[:, 1]))
    inside = cross.sum(1) % 2 == 1
    d = b - a
    t = np.clip(((x - a[:, 0]) * d[:, 0] + (y - a[:, 1]) * d[:, 1]) / np.maximum((d * d).sum(1), 1e-300), 0.0, 1.0)
    near = np.hypot(a[:, 0] + t * d[:, 0] - x, a[:, 1] + t * d[:, 1] - y).min(1) <= slack
    return inside | near


def test_planner_words_polygons_and_boxes():
    source = [S.SynthTextBatches(10, 10, (96, 128), seed=3, height=(8, 28), curve_p=0.5), S.SynthTextBatches(10, 10, (64, 64), seed=4, height=(8, 20), curve_p=0.5)]
    words = curved = 0
    for src in source:
        for b in range(len(src)):
            shapes, plans = src.plan(b)
            for (H, W), plan in zip(shapes, plans):
                boxes = []
                for w in plan['words']:
                    poly = w['polygon']
                    assert poly.dtype == np.float64 and poly.shape[1] == 2 and 4 <= len(poly) <= 28 and (len(poly) == 4) != w['curved']
                    assert poly.min() >= 0 and poly[:, 0].max() <= W and poly[:, 1].max() <= H
                    boxes.append((poly[:, 0].min() - 2, poly[:, 1].min() - 2, poly[:, 0].max() + 2, poly[:, 1].max() + 2))
                    assert w['tag'] == w['text'] and len(w['instances']) == len(w['text']) and 8 <= w['height'] <= 28
                    for inst in w['instances'].tolist():
                        contours = R.font()['contours'][inst[0]]
                        assert chr(32 + inst[0]) in w['text']
                        ky, kx = np.nonzero(R.samples_inside(H, W, contours, inst[1:5], inst[5:7]))
                        assert len(ky) > 0
                        pts = np.stack([(2 * kx + 1) / 8.0, (2 * ky + 1) / 8.0], 1)
                        assert _inside_polygon(poly, pts, 1e-6).all(), (w['text'], w['curved'])
                    words += 1
                    curved += w['curved']
                for i, p in enumerate(boxes):
                    for q in boxes[:i]:
                        assert p[2] < q[0] or q[2] < p[0] or p[3] < q[1] or q[3] < p[1]
                gt_maps.plan_polygons([[w['polygon'] for w in plan['words']]], [[w['tag'] for w in plan['words']]], max(H, W))  # accepts them
    print('%d words, %d curved' % (words, curved))
    assert words > 300 and curved > 40


def _same(p, q):
    return (p['base'], p['amps'], p['seed'], len(p['words'])) == (q['base'], q['amps'], q['seed'], len(q['words'])) and all(
        a['text'] == b['text'] and a['colour'] == b['colour'] and np.array_equal(a['polygon'], b['polygon']) and np.array_equal(a['instances'], b['instances'])
        for a, b in zip(p['words'], q['words']))


def test_planner_is_reproducible_per_image_and_independent_of_the_batch_size():
    a, b, c = S.SynthTextBatches(3, 4, (96, 128), seed=5), S.SynthTextBatches(3, 4, (96, 128), seed=5), S.SynthTextBatches(3, 2, (96, 128), seed=5)
    assert len(a) == 3 and all(_same(p, q) for p, q in zip(a.plan(1)[1], b.plan(1)[1]))
    assert all(_same(p, q) for p, q in zip(a.plan(2)[1][:2], c.plan(2)[1]))
    assert not _same(a.plan(1)[1][0], a.plan(2)[1][0]) and not _same(a.plan(1)[1][0], a.plan(1)[1][1])
    assert not _same(a.plan(1)[1][0], S.SynthTextBatches(3, 4, (96, 128), seed=6).plan(1)[1][0])
    rng = np.random.RandomState([5, 0x7374, 1, 2])
    assert _same(S.plan_synth_text([(96, 128)], rng)[0], a.plan(1)[1][2])
    many = S.SynthTextBatches(2, 8, [(64, 64), (96, 128), (50, 200)], seed=1).plan(0)[0]
    assert len(set(many)) > 1 and set(many) <= {(64, 64), (96, 128), (50, 200)}


def test_planner_options_and_small_images():
    rng = np.random.RandomState(0)
    assert all(p['words'] == [] for p in S.plan_synth_text([(4, 4), (1, 1), (7, 300)], rng))  # too small for any word: legal
    plans = S.plan_synth_text([(200, 300)] * 6, rng, vocabulary=['Hello', 'a b', '   '], words=(3, 3), ignore_below=20, height=(10, 40), min_contrast=100)
    words = [w for p in plans for w in p['words']]
    assert words and {w['text'] for w in words} <= {'Hello', 'a b'}  # a word without an outlined glyph is not placed
    assert all(len(w['instances']) == len(w['text'].replace(' ', '')) for w in words)
    assert all((w['tag'] == '###') == (w['height'] < 20) for w in words) and any(w['tag'] == '###' for w in words)
    luma = lambda c: (299 * c[0] + 587 * c[1] + 114 * c[2]) / 1000.0
    assert all(abs(luma(w['colour']) - luma(p['base'])) >= 100 or w['colour'] in ((0, 0, 0), (255, 255, 255)) for p in plans for w in p['words'])
    assert all(0 <= a <= 24 for p in plans for a in p['amps']) and all(0 <= p['seed'] < 1 << 64 for p in plans)
    assert ',' not in S.CHARSET


@pytest.mark.parametrize('kw', [{'height': (2, 10)}, {'height': (8, 300)}, {'height': (20, 10)}, {'words': (3, 1)}, {'length': (0, 4)}, {'angle': (10, -10)},
                                {'shear': (-2, 0)}, {'aspect': (0.1, 1)}, {'texture': (0, 65)}, {'curve_p': 1.5}, {'max_arc': 0}, {'pad': -1}, {'tries': 0},
                                {'vocabulary': []}, {'charset': ''}, {'height': 5}])
def test_planner_refuses(kw):
    with pytest.raises(ValueError):
        S.plan_synth_text([(64, 64)], np.random.RandomState(0), **kw)


def test_span_limit_and_list_lengths_raise():
    # cap 256 at aspect 4 spans more than 2^30 lattice units: the device would skip the glyph, so the planner raises
    with pytest.raises(ValueError, match='2\\^30'):
        for seed in range(20):
            S.plan_synth_text([(8000, 16000)], np.random.RandomState(seed), height=(256, 256), aspect=(4, 4), vocabulary=['W'], angle=(0, 0), curve_p=0)
    plans = S.plan_synth_text([(64, 64)] * 2, np.random.RandomState(0))
    with pytest.raises(ValueError, match='one plan per image'):
        S.synth_records([(64, 64)] * 3, plans)
    with pytest.raises(ValueError, match='a batch holds'):
        S.synth_records([], [])
    with pytest.raises(ValueError, match='outside 1'):
        S.synth_records([(64, 20000), (64, 64)], plans)
    for key, value in (('base', (1, 2, 256)), ('amps', (0, 65, 0)), ('seed', 1 << 64)):
        with pytest.raises(ValueError, match='plan 0'):
            S.synth_records([(64, 64)] * 2, [dict(plans[0], **{key: value}), plans[1]])
    assert S.instance_box([0, 0, 1 << 19, 0, 0, 1, 0, 0, 0], (0, 0, 1, 1)) is None and S.instance_box([0, 0, 5, 0, 0, -5, (1 << 35) + 1, 0, 0], (0, 0, 1, 1)) is None
    assert S.instance_box([0, 0, 3, 1, -2, -5, 7, 7, 0], (-10, -20, 30, 40)) == R.instance_box((3, 1, -2, -5), (7, 7), (-10, -20, 30, 40)) == (-50, -260, 130, 120)


# ---- records and bins ----------------------------------------------------------------------------------------------
def _batch():
    shapes = [(96, 128), (33, 65), (64, 64), (5, 7)]
    plans = S.plan_synth_text(shapes, np.random.RandomState(7), height=(8, 16), words=(4, 8))
    big = [0, 0, 1 << 19, 0, 0, -(1 << 19), 0, 0]  # not evaluated
    plans[2]['words'].append({'text': 'W', 'tag': 'W', 'height': 0.0, 'curved': False, 'colour': (1, 2, 3), 'polygon': np.zeros((4, 2)),
                              'instances': np.array([[ord('W') - 32] + big[2:], [0, 5000, 0, 0, -5000, 40 * L, 40 * L]], np.int64)})  # ... and a space
    return shapes, plans


def test_records_and_bins_equal_a_plain_loop():
    shapes, plans = _batch()
    recs, bins, desc = S.synth_records(shapes, plans)
    f = glyph_table()
    want = [[n, *inst, w['colour'][0] | w['colour'][1] << 8 | w['colour'][2] << 16] for n, p in enumerate(plans) for w in p['words'] for inst in w['instances'].tolist()]
    assert recs.dtype == np.int64 and recs.tolist() == want and len(recs) > 20
    assert bins.dtype == np.int32 and desc.dtype == np.int64 and desc.shape == (4, 8)
    off = tile = 0
    rows, lists = [], []
    for n, ((H, W), p) in enumerate(zip(shapes, plans)):
        assert desc[n].tolist() == [off, H, W, tile, p['base'][0] | p['base'][1] << 8 | p['base'][2] << 16, p['amps'][0] | p['amps'][1] << 8 | p['amps'][2] << 16,
                                    p['seed'] - (1 << 64 if p['seed'] >= 1 << 63 else 0), 0]
        for y0 in range(0, H, S.TILE):
            for x0 in range(0, W, S.TILE):
                mine = []
                for r, rec in enumerate(want):
                    contours = R.font()['contours'][rec[1]]
                    box = R.instance_box(rec[2:6], rec[6:8], R.box_of(contours)) if contours and rec[0] == n else None
                    if box is None:
                        continue
                    # a sample of the tile inside the box, per axis
                    hit = [any(box[i] <= L * p_ + (2 * k + 1) * L // 8 - rec[6 + i] <= box[i + 2] for p_ in range(o, min(o + S.TILE, lim)) for k in range(4))
                           for i, (o, lim) in enumerate(((x0, W), (y0, H)))]
                    if all(hit):
                        mine.append(r)
                rows.append([n, y0, x0])
                lists.append(mine)
                tile += 1
        off += 3 * H * W
    T = len(rows)
    assert T == 12 + 6 + 4 + 1 and len(bins) == 4 * T + sum(map(len, lists))
    ends = 4 * T + np.cumsum([len(m) for m in lists])
    assert bins[:4 * T].reshape(T, 4).tolist() == [r + [int(e)] for r, e in zip(rows, ends)]
    assert bins[4 * T:].tolist() == [r for m in lists for r in m]
    assert max(map(len, lists)) >= 3 and not any(len(want) - 2 in m or len(want) - 1 in m for m in lists)  # the two that are not evaluated
    assert f['index_all'][:, 1].sum() == len(f['edges_all']) == R.font()['head']['points'] and len(f['edges']) < len(f['edges_all'])
    assert np.array_equal(f['edges_all'], np.concatenate([R.edges_of(c) for c in R.font()['contours'] if c]).astype(np.int32))
    empty = S.synth_records([(5, 7)], [{'base': (1, 2, 3), 'amps': (0, 0, 0), 'seed': 0, 'words': []}])
    assert empty[0].shape == (0, 9) and empty[1].tolist() == [0, 0, 0, 4]


# ---- the entry point -----------------------------------------------------------------------------------------------
def test_entry_point_refuses_before_any_launch():
    """dbn_synth_text_u8 checks the host copies first and answers DBN_ERR_ARG (1) without touching a device"""
    shapes, plans = _batch()
    recs, bins, desc = S.synth_records(shapes, plans)
    f = glyph_table()
    need = sum(3 * h * w for h, w in shapes)
    T = int(sum(-(-h // S.TILE) * -(-w // S.TILE) for h, w in shapes))
    buf = np.zeros(2 * need, np.uint8)
    index, edges = np.ascontiguousarray(f['index_all']), np.ascontiguousarray(f['edges_all'])

    def call(desc=desc, recs=recs, bins=bins, need=need, T=T, bg=None, out=buf.ctypes.data, index=index, E=len(edges), R_=None):
        desc, recs, bins, index = (np.ascontiguousarray(a) for a in (desc, recs, bins, index))
        return _lib.lib().dbn_synth_text_u8(bg, out, need, desc.ctypes.data, desc.ctypes.data, len(shapes), recs.ctypes.data, recs.ctypes.data,
                                            len(recs) if R_ is None else R_, bins.ctypes.data, bins.ctypes.data, T, len(bins), edges.ctypes.data, E,
                                            index.ctypes.data, index.ctypes.data, len(index), None)

    def changed(a, at, value):
        a = a.copy()
        a[at] = value
        return a

    first = int(np.flatnonzero(np.diff(np.concatenate([[4 * T], bins[3:4 * T:4]])) >= 2)[0])  # a tile that lists two records or more
    at = int(bins[4 * first - 1]) if first else 4 * T
    assert bins[at] < bins[at + 1]
    # damaged records: an image or a glyph out of range, a colour of more than 24 bits, a record of another image in a bin
    for where, value in (((0, 0), -1), ((0, 0), 4), ((3, 1), 95), ((3, 1), -1), ((0, 8), 1 << 24), ((int(bins[at]), 0), 3)):
        assert call(recs=changed(recs, where, value)) == 1, where
    # bins: descending, repeated, out of range
    swapped = changed(changed(bins, at, bins[at + 1]), at + 1, bins[at])
    assert call(bins=swapped) == 1 and call(bins=changed(bins, at, bins[at + 1])) == 1
    assert call(bins=changed(bins, at, len(recs))) == 1 and call(bins=changed(bins, at, -1)) == 1 and call(R_=int(bins[4 * T:].max())) == 1
    # tiles: one missing, one twice, out of order, a wrong origin, ends that run backwards or past the lists
    missing = np.concatenate([bins[:4], bins[8:4 * T], bins[4 * T:]]).astype(np.int32)
    missing[3:4 * (T - 1):4] -= 4
    assert call(bins=missing, T=T - 1) == 1
    assert call(bins=changed(bins, slice(4, 8), bins[0:4])) == 1 and call(bins=changed(bins, 5, 32)) == 1 and call(bins=changed(bins, 4 * 12, 0)) == 1
    assert call(bins=changed(bins, 4 * T - 1, len(bins) + 1)) == 1 and call(bins=changed(bins, 4 * first + 3, 4 * T - 1)) == 1 and call(bins=bins[:-1]) == 1
    # descriptors: past `bytes`, overlapping, sizes, amplitudes, the first tile
    assert call(need=need - 1) == 1
    for where, value in (((1, 0), desc[1, 0] - 1), ((3, 0), need), ((0, 1), 0), ((0, 2), 16385), ((2, 2), 65), ((0, 5), 65), ((1, 5), 65 << 16), ((0, 4), 1 << 24),
                         ((1, 3), 11)):
        assert call(desc=changed(desc, where, value)) == 1, where
    # the glyph table: edges past E, too many edges, a box out of order or out of range
    assert call(E=len(edges) - 1) == 1
    for where, value in (((5, 1), 513), ((5, 0), -1), ((5, 2), 5000), ((5, 3), 1 << 15)):
        assert call(index=changed(index, where, value)) == 1, where
    # an `out` that overlaps the backgrounds; no out
    assert call(bg=buf.ctypes.data, out=buf.ctypes.data + need - 1) == 1 and call(bg=buf.ctypes.data + 1, out=buf.ctypes.data) == 1 and call(out=None) == 1
