"""CPU: the host half of the polygon word crops (db_text_minimal_amd.word_crops.polygon_ribbons, dbn_polygon_ribbons)
against the numpy restatement tests/rectify_ref.py: the chosen ends exactly and the knots within one unit of 1 / 1024 px
(both round the same float64 values, so only a rounding tie can differ), shapes with a known answer, invalid and refused
inputs, and the pixel restatement itself on the crop with a known answer (the axis-aligned rectangle is the slice)."""
import numpy as np
import pytest
import torch

from db_text_minimal_amd import offset_polygon, polygon_ribbons, recognize_words, rectify_from_ribbons, rectify_words
from db_text_minimal_amd.word_crops import select_polygons
import rectify_ref as R

GAP = 1e-9  # inputs are built so that the best and the second-best E differ by more than this, relatively


def rot(p, deg, about=(0.0, 0.0)):
    a = np.radians(deg)
    m = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    return (np.asarray(p, np.float64) - about) @ m.T + about


def rectangle(x0, y0, w, h):
    return np.array([[x0, y0], [x0 + w, y0], [x0 + w, y0 + h], [x0, y0 + h]], np.float64)


def sector(deg, r0=80.0, r1=110.0, side=12, centre=(200.0, 200.0)):
    """an annular sector: `side` points along the outer arc, then `side` back along the inner arc"""
    a = np.radians(np.linspace(0.0, deg, side))
    outer = np.stack([centre[0] + r1 * np.cos(a), centre[1] + r1 * np.sin(a)], 1)
    inner = np.stack([centre[0] + r0 * np.cos(a[::-1]), centre[1] + r0 * np.sin(a[::-1])], 1)
    return np.concatenate([outer, inner])


def curve_ribbon(rng, side=8, length=None, width=None):
    """a random smooth curve (two sine waves on a line, turned by a random angle) offset by +-width / 2 along its normals:
    `side` points on one side, then `side` back on the other"""
    length = rng.uniform(120, 400) if length is None else length
    width = rng.uniform(15, 40) if width is None else width
    t = np.linspace(0.0, 1.0, side)
    a1, a2, p1, p2 = rng.uniform(5, 30), rng.uniform(2, 10), rng.uniform(0, 6.28), rng.uniform(0, 6.28)
    y = a1 * np.sin(3.0 * t + p1) + a2 * np.sin(7.0 * t + p2)
    dy = (a1 * 3.0 * np.cos(3.0 * t + p1) + a2 * 7.0 * np.cos(7.0 * t + p2)) / length
    c = np.stack([t * length, y], 1)
    nrm = np.stack([-dy, np.ones_like(dy)], 1) / np.sqrt(1.0 + dy * dy)[:, None]
    top, bottom = c - nrm * width / 2, c + nrm * width / 2
    return rot(np.concatenate([top, bottom[::-1]]), rng.uniform(-180, 180)) + rng.uniform(300, 600, 2)


def general_inputs():
    """(name, polygon) of every kind the issue lists; built once"""
    rng = np.random.default_rng(20)
    out = [('rect', rectangle(10, 20, 100, 32)), ('rect 25 deg', rot(rectangle(10, 20, 100, 32), 25) + 50), ('tall rect', rectangle(5, 7, 20, 90)),
           ('rect -70 deg', rot(rectangle(0, 0, 240, 50), -70) + 300), ('thin rect', rectangle(100.25, 30.5, 333.5, 11.25))]
    out += [('sector %d' % d, sector(d)) for d in (90, 180, 270, 330)]
    out += [('curve %d' % i, curve_ribbon(rng, side=int(rng.integers(4, 12)))) for i in range(8)]
    for i, (quad, delta) in enumerate([(rectangle(100, 100, 150, 20), 6.0), (rot(rectangle(0, 0, 90, 14), 33) + 200, 5.0),
                                       (np.array([[50, 60], [220, 40], [230, 75], [45, 90]], np.float64), 8.0)]):
        p = offset_polygon(quad, delta).astype(np.float64)  # rounded corners, as the detector's unclip gives them
        assert 8 <= len(p) <= 80, len(p)
        out.append(('unclipped %d' % i, p))
    out += [('triangle %d' % i, rng.uniform(0, 200, (3, 2)) * (3.0, 1.0) + 50) for i in range(5)]
    return out


_cache = {}


def restated(name, poly, S=32, ends='auto'):
    """the restatement's ribbon and energy table, computed once per input"""
    key = (name, S, ends)
    if key not in _cache:
        E = R.energies(poly, S) if ends == 'auto' else None
        _cache[key] = (R.ribbon(poly, S, ends, E=E), E)
    return _cache[key]


def assert_ribbon_equal(poly, S, ends, ref, tag):
    knots, valid, info = polygon_ribbons([poly], S, ends, return_info=True)
    assert knots.shape == (1, S + 1, 4) and knots.dtype == np.int32 and valid.shape == (1, ) and valid.dtype == np.uint8
    assert tuple(info['ends'][0]) == ref['ends'], (tag, info['ends'][0], ref['ends'])
    assert valid[0] == ref['valid'], tag
    worst = np.abs(knots[0].astype(np.int64) - ref['knots'].astype(np.int64)).max()
    assert worst <= 1, (tag, worst)
    return knots[0]


@pytest.mark.parametrize('S', [32, 4, 64])
def test_ribbons_against_the_restatement(S):
    inputs = general_inputs() if S == 32 else general_inputs()[::3]
    for name, poly in inputs:
        ref, E = restated(name, poly, S)
        gap = R.energy_gap(E)
        assert gap > GAP, (name, S, gap)  # none has to be left out
        assert ref['valid'] == 1, name
        assert_ribbon_equal(poly, S, 'auto', ref, (name, S))


def test_one_call_for_a_batch_equals_one_call_each():
    polys = [p for _, p in general_inputs()]
    knots, valid = polygon_ribbons(polys)
    for k, p in enumerate(polys):
        k1, v1 = polygon_ribbons([p])
        assert np.array_equal(knots[k], k1[0]) and valid[k] == v1[0]
    k0, v0 = polygon_ribbons([])
    assert k0.shape == (0, 33, 4) and v0.shape == (0, )


def test_both_orientations_and_every_starting_vertex():
    rng = np.random.default_rng(3)
    for name, poly in (('sector', sector(120, side=5)), ('curve', curve_ribbon(rng, side=5)), ('rect', rot(rectangle(0, 0, 90, 31), 12) + 40),
                       ('triangle', np.array([[10, 10], [200, 40], [30, 70]], np.float64))):
        base, _ = restated(name + ' as given', poly)
        want = {tuple(base['start']), tuple(base['stop'])}
        first = polygon_ribbons([poly])[0][0]
        for flip in (False, True):
            for s in range(len(poly)):
                q = np.roll(poly[::-1] if flip else poly, s, axis=0)
                tag = '%s flip %d roll %d' % (name, flip, s)
                ref, E = restated(tag, q)
                assert R.energy_gap(E) > GAP, tag
                assert {tuple(ref['start']), tuple(ref['stop'])} == want, tag  # the same two boundary points
                knots = assert_ribbon_equal(q, 32, 'auto', ref, tag)
                assert np.abs(knots.astype(np.int64) - first).max() <= 1, tag  # the same crop geometry


def _centre_length(knots):
    c = knots[:, :2].astype(np.float64) / 1024
    return np.sqrt(((c[1:] - c[:-1]) ** 2).sum(1)).sum()


def test_rectangle_known_answer():
    for deg in (0, 25, 90, -140):
        poly = rot(rectangle(10, 20, 100, 32), deg) + 300
        knots, valid, info = polygon_ribbons([poly], return_info=True)
        assert valid[0] == 1 and tuple(info['ends'][0]) == (3, 7)  # the two short-edge midpoints
        assert abs(info['width'][0] - 32) < 1e-9 and abs(info['length'][0] - 100) < 1e-9
        assert abs(info['E'][0] - 833.5075757575758) < 1e-6  # 25 samples across the full width, 8 on the two caps
        c, n = knots[0, :, :2] / 1024.0, knots[0, :, 2:] / 1024.0
        mids = [(poly[1] + poly[2]) / 2, (poly[3] + poly[0]) / 2]
        assert min(np.abs(c[0] - mids[0]).max() + np.abs(c[-1] - mids[1]).max(), np.abs(c[0] - mids[1]).max() + np.abs(c[-1] - mids[0]).max()) < 2e-3
        step = c[1:] - c[:-1]
        assert np.abs(step - step[0]).max() < 4e-3 and abs(_centre_length(knots[0]) - 100) < 0.01  # straight, evenly spaced
        assert np.abs(np.sqrt((n ** 2).sum(1)) - 32).max() < 2e-3
        d = c[-1] - c[0]
        assert (d[0] > 0) if abs(d[0]) >= abs(d[1]) else (d[1] > 0)  # starts at the smaller x, or y for a tall line
        assert np.abs(n @ d).max() < 0.3 and (d[0] * n[0, 1] - d[1] * n[0, 0]) > 0  # the normal: the direction turned by +90 degrees


@pytest.mark.parametrize('deg, width, length', [(90, 30.2, 152.8), (180, 30.5, 300.5), (270, 30.3, 443.2), (330, 30.4, 536.5)])
def test_sector_known_answer(deg, width, length):
    """the ends are the caps; the width within 2 % of 30 and the centre line within 2.5 % of the mid-radius arc (the values
    in the parametrisation are the issue's own measurements of the rule, to 0.05)"""
    poly = sector(deg)
    knots, valid, info = polygon_ribbons([poly], return_info=True)
    assert valid[0] == 1 and tuple(info['ends'][0]) == (23, 47)  # mid(v11, v12) and mid(v23, v0)
    arc = np.radians(deg) * 95.0
    assert abs(info['width'][0] - 30) <= 0.02 * 30 and abs(info['length'][0] - arc) <= 0.025 * arc
    assert abs(info['width'][0] - width) <= 0.05 and abs(info['length'][0] - length) <= 0.05
    c = knots[0, :, :2] / 1024.0
    caps = [(poly[11] + poly[12]) / 2, (poly[23] + poly[0]) / 2]
    assert min(np.abs(c[0] - caps[0]).max() + np.abs(c[-1] - caps[1]).max(), np.abs(c[0] - caps[1]).max() + np.abs(c[-1] - caps[0]).max()) < 2e-3
    sagitta = 95 * (1 - np.cos(np.radians(deg / 11) / 2))  # the 12 points a side are joined by chords
    assert np.abs(np.sqrt(((c - 200) ** 2).sum(1)) - 95).max() < sagitta + 1  # the centre line runs along the mid radius


def test_square_tie_goes_to_the_smallest_pair():
    sq = rectangle(0, 0, 64, 64)  # every operation exact, so the symmetric pairs tie exactly
    E = R.energies(sq)
    best = min(E.values())
    tied = sorted(ij for ij, v in E.items() if v == best)
    assert len(tied) >= 2 and R.energy_gap(E) == 0  # the rule is live
    _, valid, info = polygon_ribbons([sq], return_info=True)
    assert tuple(info['ends'][0]) == tied[0] == R.ribbon(sq, E=E)['ends'] and info['E'][0] == best and valid[0] == 1
    for s in (1, 2, 3):  # from another starting vertex the indices are the same, so the points are others
        _, _, info = polygon_ribbons([np.roll(sq, s, axis=0)], return_info=True)
        assert tuple(info['ends'][0]) == tied[0]


def ctw_polygon(curved):
    """14 points in CTW1500 order: v0 .. v6 along the top from the left, v7 .. v13 back along the bottom"""
    x = np.linspace(40.0, 400.0, 7)
    bend = 40.0 * np.sin(np.linspace(0, np.pi, 7)) if curved else np.zeros(7)
    top, bottom = np.stack([x, 100.0 - bend], 1), np.stack([x, 148.0 - bend], 1)
    return np.concatenate([top, bottom[::-1]])


def test_half_mode_follows_the_annotation_order():
    for curved in (False, True):
        poly = ctw_polygon(curved)
        ref = R.ribbon(poly, 32, 'half')
        knots = assert_ribbon_equal(poly, 32, 'half', ref, curved)
        _, _, info = polygon_ribbons([poly], ends='half', return_info=True)
        assert tuple(info['ends'][0]) == (27, 13)
        c, n = knots[:, :2] / 1024.0, knots[:, 2:] / 1024.0
        assert np.abs(c[0] - (poly[13] + poly[0]) / 2).max() < 1e-3 and np.abs(c[-1] - (poly[6] + poly[7]) / 2).max() < 1e-3
        assert (n @ (poly[13] - poly[0]) > 0).all()  # y = 0 is at C - n / 2: the side of v0 .. v6
        if not curved:
            assert np.abs(c[0] - n[0] / 2 - poly[0]).max() < 2e-3 and np.abs(c[-1] + n[-1] / 2 - poly[7]).max() < 2e-3
        # no re-orientation: the same word upside down keeps its start, where 'auto' starts at the smaller x
        turned = rot(poly, 180, about=(220.0, 120.0))
        k_half, k_auto = polygon_ribbons([turned], ends='half')[0][0], polygon_ribbons([turned])[0][0]
        assert np.abs(k_half[0, :2] / 1024.0 - (turned[13] + turned[0]) / 2).max() < 1e-3 and k_half[0, 0] > k_half[-1, 0]
        assert k_auto[0, 0] < k_auto[-1, 0]


def test_invalid_polygons_give_no_ribbon():
    bad = [
        [[0, 0], [10, 10], [20, 20], [30, 30]],           # collinear
        [[0, 0], [5, 0], [10, 0]],                        # collinear triangle
        [[5, 5], [5, 5], [5, 5], [5, 5]],                 # one point
        [[0, 0], [10, 0], [10, 0], [0, 0]],               # a segment twice
        [[0, 0], [10, 4], [0, 0], [10, 4], [0, 0], [10, 4]],
        [[0, 0], [10, 0], [0, 10], [10, 10]],             # a bow tie: the two halves cancel
    ]
    for ends in ('auto', 'half'):
        for p in bad:
            if ends == 'half' and len(p) % 2:
                continue
            knots, valid = polygon_ribbons([np.array(p, np.float64)], ends=ends)
            assert valid[0] == 0 and not knots.any(), (ends, p)
            assert R.ribbon(p, 32, ends)['valid'] == 0
    # a repeated vertex alone does not spoil a polygon
    p = np.array([[0, 0], [100, 0], [100, 0], [100, 30], [0, 30]], np.float64)
    assert polygon_ribbons([p])[1][0] == 1
    # a cross-section beyond int32 units: no crop
    huge = rectangle(-2.0 ** 20, -2.0 ** 20, 2.0 ** 21, 2.0 ** 21)
    knots, valid = polygon_ribbons([huge])
    assert valid[0] == 0 and not knots.any() and R.ribbon(huge)['valid'] == 0
    knots, valid = polygon_ribbons([rectangle(-2.0 ** 20, -2.0 ** 20, 2.0 ** 21, 1000.0)])  # the largest coordinates fit
    assert valid[0] == 1 and knots[:, :, 0].min() == -2 ** 30 and knots[:, :, 0].max() == 2 ** 30


def test_refused_inputs():
    ok = rectangle(0, 0, 50, 10)
    for bad, kw in [(ok[:2], {}), (np.zeros((257, 2)) + ok[0], {}), (sector(90, side=4)[:7], dict(ends='half')), (ok * np.nan, {}),
                    (np.where(np.eye(4, 2) > 0, np.inf, ok), {}), (ok + 2.0 ** 20, {}), (-ok - 2.0 ** 20 - 1, {}), (ok, dict(segments=3)),
                    (ok, dict(segments=65)), (ok, dict(segments=8.5)), (ok, dict(ends='both')), (ok.reshape(-1), {}), (np.zeros((4, 3)), {})]:
        with pytest.raises(ValueError):
            polygon_ribbons([ok, bad], **kw)
    assert polygon_ribbons([np.zeros((256, 2)) + ok[0]])[1][0] == 0  # 256 vertices are taken (one point: no ribbon)
    assert polygon_ribbons([ok, ok], segments=4)[0].shape == (2, 5, 4) and polygon_ribbons([ok], segments=64)[0].shape == (1, 65, 4)


def test_select_polygons_applies_the_rule_of_select_boxes():
    a, b, z = rectangle(1, 1, 5, 3), rectangle(2, 2, 9, 4).astype(np.int64), np.zeros((4, 2), np.int64)
    kept, index = select_polygons([[a, z, b], [], [z]])
    assert index.tolist() == [[0, 0], [0, 2]] and kept[1] is b
    kept, index = select_polygons([([a, z, b], [0.9, 0.9, 0.5]), ([b], [0.8])], min_score=0.8)
    assert index.tolist() == [[0, 0], [1, 0]]
    assert select_polygons([[-a]])[1].shape == (0, 2)
    with pytest.raises(ValueError, match='needs the scores'):
        select_polygons([[a]], min_score=0.5)
    with pytest.raises(ValueError, match='mixes'):
        select_polygons([([a], [1.0]), [a]])
    with pytest.raises(ValueError, match='scores'):
        select_polygons([[a, b]], scores=[[1.0]], min_score=0.5)


def test_argument_errors_come_before_any_launch():
    img = torch.zeros((10, 12, 3), dtype=torch.uint8)
    poly = rectangle(1, 1, 8, 4)
    knots, valid = polygon_ribbons([poly])
    for kw, match in [(dict(size=(0, 5)), 'crop size'), (dict(size=32), 'size must be'), (dict(segments=2), 'segments'), (dict(ends='x'), 'ends'),
                      (dict(min_score=0.5), 'needs the scores'), (dict(device='cpu'), 'GPU device'), (dict(size=(40000, 40000)), 'too large')]:
        with pytest.raises(ValueError, match=match):
            rectify_words(img, [[poly]], **kw)
    with pytest.raises(ValueError, match='2 images'):
        rectify_words(img, [[poly], [poly]], device='cpu')
    with pytest.raises(ValueError, match='uint8'):
        rectify_words(img.float(), [[poly]])
    with pytest.raises(ValueError, match='vertices'):
        rectify_words(img, [[poly[:2] + 1]])
    for args, match in [((knots[0], valid, [0]), 'knots must be'), ((knots, valid, [0, 0]), 'image indices'), ((knots, valid, [1]), 'outside'),
                        ((knots[:, :3], valid, [0]), 'segments'), ((knots, valid, [0], (40000, 40000)), 'too large')]:
        with pytest.raises(ValueError, match=match):
            rectify_from_ribbons(img, *args)
    with pytest.raises(ValueError, match='not both'):
        recognize_words(img, [np.zeros((1, 4, 2), np.int16)], None, None, polygons=[[poly]])


# ---- the pixel restatement on the crop with a known answer ----------------------------------------------------------------
@pytest.mark.parametrize('S', [4, 32, 64])
def test_axis_aligned_rectangle_is_the_slice(S):
    rng = np.random.default_rng(S)
    img = rng.integers(0, 256, (90, 150, 3), dtype=np.uint8)
    for (h, w), (x0, y0) in (((32, 100), (17, 40)), ((32, 100), (0, 0)), ((32, 100), (50, 58)), ((16, 64), (3, 5)), ((8, 128), (22, 82))):
        r = R.ribbon(rectangle(x0, y0, w, h), S)
        knots, valid = polygon_ribbons([rectangle(x0, y0, w, h)], S)
        assert np.array_equal(knots[0], r['knots']) and valid[0] == 1
        assert np.array_equal(R.rectify(img, r['knots'], 1, h, w), img[y0:y0 + h, x0:x0 + w]), (S, h, w, x0, y0)
    # past the border the slice continues with zeros
    r = R.ribbon(rectangle(-10, 70, 100, 32), S)
    want = np.zeros((32, 100, 3), np.uint8)
    want[:20, 10:] = img[70:, :90]
    assert np.array_equal(R.rectify(img, r['knots'], 1, 32, 100), want)
    assert not R.rectify(img, r['knots'], 0, 32, 100).any()
