"""CPU (-m "not gpu"): the labels of db_text_minimal_amd.render.  The committed glyph table against what
fonts/make_glyphs.py regenerates; table and winding predicate of the restatement tests/labels_ref.py (what the device is
compared with bit for bit) against matplotlib's own containment test on the CURVED outlines; the host side of render.py
(glyph_table, label_records, label_backgrounds, text_size, score_labels) against the restatement; every argument check."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from db_text_minimal_amd import render as Rn
import labels_ref as LR

VISIBLE = ''.join(chr(c) for c in range(33, 127))
FONTS = os.path.join(LR.ROOT, 'db_text_minimal_amd', 'fonts')


def _make_glyphs():
    spec = importlib.util.spec_from_file_location('make_glyphs', os.path.join(FONTS, 'make_glyphs.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_committed_table_equals_regeneration():
    pytest.importorskip('matplotlib', reason='the glyph table is regenerated from the font matplotlib bundles')
    assert _make_glyphs().generate() == open(LR.TABLE).read()


def test_table_header_and_known_metrics():
    f = LR.font()
    assert f['head']['units_per_EM'] == 2048 and f['head']['ascender'] == 1901 and f['head']['descender'] == -483 and f['head']['cap_height'] == 1493
    assert sorted(f['adv']) == list(range(32, 127))
    assert f['adv'][ord('A')] == 1401 and f['adv'][32] == 651 and f['contours'][32] == []
    assert max(int(c[:, 1].max()) for c in f['contours'][ord('H')]) == 1493
    points = [sum(len(c) for c in cs) for cs in f['contours'].values()]
    assert sum(points) == f['head']['points'] and max(points) <= 512  # a glyph's edges fit the kernel's LDS stage
    assert os.path.getsize(LR.TABLE) < 100 * 1024
    for cs in f['contours'].values():
        for c in cs:
            assert len(c) >= 3 and (c != np.roll(c, 1, 0)).any(1).all()  # closed, no repeated point


def _lines(cap):
    """the 94 visible glyphs, 16 to a line"""
    pitch = int(np.ceil(2.0 * cap))
    return [(VISIBLE[i:i + 16], (5, int(np.floor(1.6 * cap)) + k * pitch)) for k, i in enumerate(range(0, len(VISIBLE), 16))]


def _mpl_mask(H, W, labels, cap, sub):
    """even-odd containment of the pixel centres, per contour of the curved outline, by matplotlib"""
    import matplotlib
    from matplotlib.ft2font import FT2Font, LoadFlags
    from matplotlib.path import Path
    font = FT2Font(os.path.join(matplotlib.get_data_path(), 'fonts', 'ttf', 'DejaVuSans.ttf'), hinting_factor=1)
    scale = LR.size64(cap) / LR.L  # pixels per font unit
    py, px = np.mgrid[0:H, 0:W]
    centres = np.stack([px.reshape(-1) + 0.5, py.reshape(-1) + 0.5], 1)
    mask = np.zeros(H * W, bool)
    for text, (x, y) in labels:
        pen = 0
        for ch in text:
            g = font.load_char(ord(ch), flags=LoadFlags.NO_SCALE)
            verts, codes = font.get_path()
            v = np.asarray(verts, np.float64) * 64
            # the centres in the glyph's font units, not the outline in pixels: matplotlib flattens a curve to a tolerance in
            # the units of its vertices, which is fine at 2048 per em and coarse at 8 pixels per cap height
            pts = np.stack([(centres[:, 0] - x - sub[0] / 64) / scale - pen, (y + sub[1] / 64 - centres[:, 1]) / scale], 1)
            starts = [i for i, c in enumerate(codes) if c == Path.MOVETO] + [len(codes)]
            lo, hi = v.min(0), v.max(0)
            box = (pts[:, 0] >= lo[0] - 1) & (pts[:, 0] <= hi[0] + 1) & (pts[:, 1] >= lo[1] - 1) & (pts[:, 1] <= hi[1] + 1)
            inside = np.zeros(int(box.sum()), bool)
            for a, b in zip(starts[:-1], starts[1:]):
                inside ^= Path(v[a:b], codes[a:b]).contains_points(pts[box])
            mask[box] |= inside
            pen += g.horiAdvance
    return mask.reshape(H, W)


@pytest.mark.parametrize('cap', [8, 16, 40])
def test_table_and_predicate_against_matplotlib_containment(cap):
    """The restatement fills chords of the table, matplotlib its own flattening of the curves, so pixels whose centre
    lies on the outline may differ: at most 0.5 % of the filled ones (a wrong winding rule, a dropped contour or a
    mis-scaled axis is tens of percent).  Measured: 2 of 1 350, 8 of 5 540 and 43 of 34 582 (0.15, 0.14, 0.12 %; printed below)."""
    pytest.importorskip('matplotlib')
    labels, sub = _lines(cap), (13, 37)
    W = 5 + int(np.ceil(max(LR.advance(t) for t, _ in labels) * LR.size64(cap) / LR.L)) + 5
    H = labels[-1][1][1] + cap
    ref = LR.label_mask(H, W, labels, cap, sub)
    mpl = _mpl_mask(H, W, labels, cap, sub)
    filled, differ = int(ref.sum()), int((ref != mpl).sum())
    print('cap %d: %d of %d filled pixels differ (%.2f %%)' % (cap, differ, filled, 100.0 * differ / filled))
    assert not ref[0].any() and not ref[-1].any() and not ref[:, 0].any() and not ref[:, -1].any()  # nothing is clipped
    assert filled > 1000 and differ <= 0.005 * filled


def test_vectorised_predicate_equals_python_integers():
    rng = np.random.default_rng(1)
    f = LR.font()
    for ch, height in [('g', 7.5), ('@', 512), ('8', 16), ('%', 4)]:
        s, cs = LR.size64(height), f['contours'][ord(ch)]
        Px = rng.integers(-200 * s, 2200 * s, 300)
        Py = rng.integers(-600 * s, 2000 * s, 300)
        Py[:40] = [int(cs[0][k % len(cs[0]), 1]) * s for k in range(40)]  # at the height of a vertex
        got = LR.winding(cs, s, Px, Py)
        assert got.tolist() == [LR.winding_exact(cs, s, int(a), int(b)) for a, b in zip(Px, Py)]
        assert set(got.tolist()) <= {0, 1, -1} and (got != 0).any()


def test_known_answers():
    # 'H' at cap height 14.93 px is 1 px per 100 units: stems 2.01 .. 4.03 and 11.37 .. 13.39, bar 7.11 .. 8.81 below the top
    s = LR.size64(14.93)
    assert s == 64 * 2048 // 100 + 1  # rint(1310.72)
    m = LR.label_mask(20, 20, [('H', (0, 16))], 14.93)
    assert np.flatnonzero(m[1]).tolist() == [2, 3, 11, 12] and np.flatnonzero(m.any(1)).tolist() == list(range(1, 16))
    assert np.flatnonzero(m[:, 5]).tolist() == [7, 8] and m[1:16, 2].all() and np.flatnonzero(m[7]).tolist() == list(range(2, 13))
    # '|' and space: a space paints nothing and moves the pen
    assert not LR.label_mask(30, 30, [('   ', (3, 20))]).any()
    a, b = LR.label_mask(30, 60, [('|', (3, 20))]), LR.label_mask(30, 60, [('  |', (3, 20))])
    assert a.any() and b.any() and not np.array_equal(a, b)
    # 'O' has a hole: the ring's centre is empty
    o = LR.label_mask(60, 60, [('O', (5, 50))], 40)
    ys, xs = np.nonzero(o)
    assert not o[(ys.min() + ys.max()) // 2, (xs.min() + xs.max()) // 2] and o.sum() > 300


def test_host_tables_equal_the_restatement():
    f, g = LR.font(), Rn.glyph_table()
    assert g['first'] == 32 and g['advance'].tolist() == [f['adv'][c] for c in range(32, 127)]
    assert (g['units_per_EM'], g['ascender'], g['descender'], g['cap_height']) == (2048, 1901, -483, 1493)
    for k, cp in enumerate(range(32, 127)):
        e0, ne, x0, y0, x1, y1 = g['index'][k].tolist()
        want = [np.concatenate([c, np.roll(c, -1, 0)], 1) for c in f['contours'][cp]]
        want = np.concatenate(want) if want else np.zeros((0, 4), np.int64)
        want = want[want[:, 1] != want[:, 3]]
        assert np.array_equal(g['edges'][e0:e0 + ne], want) and ne <= 512
        if ne:
            p = np.concatenate(f['contours'][cp])
            assert (x0, y0, x1, y1) == (p[:, 0].min(), p[:, 1].min(), p[:, 0].max(), p[:, 1].max())
    assert int(g['index'][:, 1].sum()) == len(g['edges'])


def test_records_question_mark_and_pens():
    recs = Rn.label_records([[('A b', (3, -4)), ('', (0, 0))], [], [('é~\x7f\n', (2 ** 20, -2 ** 20))]], 3)
    q, t = ord('?') - 32, ord('~') - 32
    adv = LR.font()['adv']
    assert recs.dtype == np.int32 and recs.tolist() == [
        [0, ord('A') - 32, 0, 3, -4], [0, ord('b') - 32, adv[ord('A')] + adv[32], 3, -4],
        [2, q, 0, 2 ** 20, -2 ** 20], [2, t, adv[63], 2 ** 20, -2 ** 20], [2, q, adv[63] + adv[126], 2 ** 20, -2 ** 20],
        [2, q, 2 * adv[63] + adv[126], 2 ** 20, -2 ** 20]]
    assert Rn.label_records([[], []], 2).shape == (0, 5)
    # an empty label between two others, one of them at x = 0: the pens restart with every label
    mixed = Rn.label_records([[('ab', (0, 7)), ('', (5, 6)), ('c d', (9, 0))], [('', (1, 1))], [('e', (-3, 2))]], 3)
    assert mixed.tolist() == [[0, ord('a') - 32, 0, 0, 7], [0, ord('b') - 32, adv[ord('a')], 0, 7], [0, ord('c') - 32, 0, 9, 0],
                              [0, ord('d') - 32, adv[ord('c')] + adv[32], 9, 0], [2, ord('e') - 32, 0, -3, 2]]
    assert Rn.label_records([[('', (3, 4)), ('  ', (0, 0))]], 1).shape == (0, 5)
    one = Rn.label_records([('x', (1, 2))], 1)  # a single image: the list of labels itself
    assert one.tolist() == [[0, ord('x') - 32, 0, 1, 2]]
    m = LR.label_mask(40, 80, [('aéb', (2, 30))])
    assert np.array_equal(m, LR.label_mask(40, 80, [('a?b', (2, 30))]))


def test_backgrounds_are_rectangles_with_a_two_pixel_margin():
    for height in (4, 16, 333.3):
        s = LR.size64(height)
        e, g, r = Rn.label_backgrounds([[('Word', (7, 9))], [('', (1, 2)), ('xy', (-5, 6))]], 2, s)
        m = -((-2 * LR.L) // s)
        assert (m - 1) * s < 2 * LR.L <= m * s
        assert r.tolist() == [[0, 0, 0, 7, 9], [1, 1, 0, 1, 2], [1, 2, 0, -5, 6]]
        for k, text in enumerate(['Word', '', 'xy']):
            x0, x1, y0, y1 = -m, LR.advance(text) + m, -483 - m, 1901 + m
            assert g[k].tolist() == [2 * k, 2, x0, y0, x1, y1]
            assert e[2 * k:2 * k + 2].tolist() == [[x1, y0, x1, y1], [x0, y1, x0, y0]]
    bm = LR.background_mask(60, 120, [('Word', (10, 40))], 16)
    ys, xs = np.nonzero(bm)
    s, m = LR.size64(16), -((-2 * LR.L) // LR.size64(16))
    k = s / LR.L  # pixels per font unit; a pixel is inside iff its centre is (none of these bounds is near a centre)
    assert bm[ys.min():ys.max() + 1, xs.min():xs.max() + 1].all()
    assert xs.min() == np.ceil(10 - m * k - 0.5) == 8 and xs.max() == np.floor(10 + (LR.advance('Word') + m) * k - 0.5)
    assert ys.min() == np.ceil(40 - (1901 + m) * k - 0.5) and ys.max() == np.floor(40 + (483 + m) * k - 0.5) == 46
    assert LR.label_mask(60, 120, [('Word', (10, 40))], 16)[bm].sum() == LR.label_mask(60, 120, [('Word', (10, 40))], 16).sum()


def test_text_size_against_the_advances():
    adv = LR.font()['adv']
    for text, height in [('Hello, world', 16), ('', 16), (' ', 4), ('W' * 256, 512), ('café', 7.5)]:
        s = LR.size64(height)
        total = sum(adv[LR.code(c)] for c in text)
        w, a, d = Rn.text_size(text, height)
        assert all(isinstance(v, int) for v in (w, a, d))
        assert (w - 1) * LR.L < total * s <= w * LR.L or (total == 0 and w == 0)
        assert (a - 1) * LR.L < 1901 * s <= a * LR.L and (d - 1) * LR.L < 483 * s <= d * LR.L
    assert Rn.text_size('A')[0] == -(-1401 * LR.size64(16) // LR.L) and Rn.text_size('H', 100)[1] == -(-1901 * LR.size64(100) // LR.L)
    assert LR.size64(16) == int(np.rint(16 * 64 * 2048 / 1493)) == 1405 and Rn._size64(16) == 1405 and Rn._size64(7.5) == LR.size64(7.5)


def test_score_labels():
    boxes = np.array([[[3, 4], [9, 4], [9, 8], [3, 8]], [[0, 0], [0, 0], [0, 0], [0, 0]], [[-5, 2], [9, 2], [9, 8], [3, 8]]], np.int16)
    polys = [np.array([[7, 1], [9, 2], [8, 5]], np.int64)]
    got = Rn.score_labels([(boxes, np.array([0.5, 0.9, 0.987], np.float32)), (polys, [0.25]), ([], [])], 3)
    assert got == [[('0.50', (3, 4)), ('0.99', (-5, 2))], [('0.25', (7, 1))], []]
    assert Rn.score_labels((boxes[:1], [1.0]), 1, '%.1f') == [[('1.0', (3, 4))]]
    with pytest.raises(ValueError):
        Rn.score_labels([boxes], 1)  # no scores
    with pytest.raises(ValueError):
        Rn.score_labels([(boxes, [0.5])], 1)


# ---- argument checks (before any launch: none of these reaches the device) ---------------------------------------------------
def test_argument_errors():
    img = torch.zeros((8, 9, 3), dtype=torch.uint8)
    ok = [('ab', (1, 5))]
    for height in (3.99, 512.5, -1, float('nan'), 'tall', None, True):
        with pytest.raises(ValueError):
            Rn.draw_labels(img, [ok], height=height)
        with pytest.raises(ValueError):
            Rn.text_size('ab', height)
    for org in ((2 ** 20 + 1, 0), (0, -2 ** 20 - 1), (1.5, 2), ('a', 2), (1, ), None):
        with pytest.raises(ValueError):
            Rn.draw_labels(img, [[('ab', org)]])
    with pytest.raises(ValueError):
        Rn.draw_labels(img, [[('a' * 257, (0, 0))]])
    with pytest.raises(ValueError):
        Rn.text_size('a' * 257)
    with pytest.raises(ValueError):
        Rn.draw_labels(img, [[(b'ab', (0, 0))]])
    for color in ((256, 0, 0), (0, 0), (1, 2, -3), (0.5, 1, 2), 'red'):
        with pytest.raises(ValueError):
            Rn.draw_labels(img, [ok], color=color)
        with pytest.raises(ValueError):
            Rn.draw_labels(img, [ok], background=color)
        with pytest.raises(ValueError):
            Rn.draw_words(img, [[]], dot_color=color)
    for labels in ([ok, ok], [], 'ab', None):
        with pytest.raises(ValueError):
            Rn.draw_labels(img, labels)
    with pytest.raises(ValueError):
        Rn.draw_labels(img, [['ab']])
    with pytest.raises(ValueError):
        Rn.draw_words(img, [[{'box': None, 'pred': 'x', 'score': 1.0}]])
    with pytest.raises(ValueError):
        Rn.draw_words(img, [[], []])
    with pytest.raises(ValueError):
        Rn.draw_scores(img, [[], []])
    with pytest.raises(ValueError):
        Rn.draw_dots(img, [[(2 ** 21, 0)]])
    with pytest.raises(ValueError):
        Rn.draw_labels(img, [ok], out=torch.zeros(8 * 9 * 3, dtype=torch.uint8))  # a host buffer
    # the accepted ends of every range raise nothing on the host
    assert Rn.label_records([[('a' * 256, (2 ** 20, -2 ** 20))]], 1).shape == (256, 5)
    assert Rn._size64(4) == LR.size64(4) and Rn._size64(512) == LR.size64(512) == 44949


def test_records_equal_a_plain_loop_over_the_table():
    """label_records is vectorised over all labels of a batch; a loop over characters with the restatement's table must
    give the same rows: long and short labels, empty ones in every position, x = 0, non-ASCII, all 95 characters"""
    rng = np.random.default_rng(2)
    f = LR.font()
    alphabet = [chr(c) for c in range(32, 127)] + ['é', '\n', '\x7f', '€', '\U0001f600']
    batch = []
    for n in range(7):
        labs = []
        for k in range(int(rng.integers(0, 9))):
            length = int(rng.choice([0, 0, 1, 2, 6, 95, 256]))
            text = ''.join(alphabet[i] for i in rng.integers(0, len(alphabet), length))
            labs.append((text, (int(rng.choice([0, 0, 5, -2 ** 20, 2 ** 20])), int(rng.integers(-50, 50)))))
        batch.append(labs)
    batch[3] = []
    batch[5] = [('', (0, 0))] + batch[5] + [('', (1, 1)), (''.join(chr(c) for c in range(32, 127)), (0, 0))]
    want = []
    for n, labs in enumerate(batch):
        for text, (x, y) in labs:
            pen = 0
            for ch in text:
                cp = LR.code(ch)
                if any(len(c) for c in f['contours'][cp]):
                    want.append([n, cp - 32, pen, x, y])
                pen += f['adv'][cp]
    got = Rn.label_records(batch, 7)
    assert len(want) > 500 and got.dtype == np.int32 and got.tolist() == want
