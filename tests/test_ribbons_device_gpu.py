"""GPU (-m gpu): polygon_ribbons_device (csrc/rectify.hip polygon_ribbons_kernel) against polygon_ribbons of the same
library, the host half it repeats.  The reference is exact, so equality is np.array_equal on knots, valid and ends and
bit equality on E, width and length; no input is left out and there is no tolerance.  Broad inputs at 4 / 32 / 64 segments
and both `ends`, exact ties and perfect-square lengths (the tie rule and the square root), the size limits (3 and 256
vertices), batches (0, 1, 1 000 mixed; one call each; two runs; every output byte written and none beyond; inputs
unchanged), untrusted offsets and coordinates through the raw C entry (a defined result: that polygon alone gets no
ribbon), and end to end through rectify_words, rectify_from_ribbons and recognize_words."""
import numpy as np
import pytest
import torch

from db_text_minimal_amd import (CTCLabelConverter, image_collate, polygon_ribbons, polygon_ribbons_device, recognize_words, rectify_from_ribbons,
                                 rectify_words)
from db_text_minimal_amd._lib import check, lib
from gpu_util import DEV, stream
from test_recognise_gpu import CHARS
from test_rectify_cpu import ctw_polygon, curve_ribbon, general_inputs, rectangle
from test_rectify_gpu import _Stub, _images, _polygons

pytestmark = pytest.mark.gpu

POISON, GUARD = 0xA5, 64
INVALID = [  # the list of test_invalid_polygons_give_no_ribbon
    [[0, 0], [10, 10], [20, 20], [30, 30]], [[0, 0], [5, 0], [10, 0]], [[5, 5], [5, 5], [5, 5], [5, 5]], [[0, 0], [10, 0], [10, 0], [0, 0]],
    [[0, 0], [10, 4], [0, 0], [10, 4], [0, 0], [10, 4]], [[0, 0], [10, 0], [0, 10], [10, 10]],
    [[0, 0], [100, 0], [100, 0], [100, 30], [0, 30]],  # valid: a repeated vertex alone does not spoil a polygon
]


def _host(polys, S, ends):
    knots, valid, info = polygon_ribbons(polys, S, ends, return_info=True)
    return dict(knots=knots, valid=valid, ends=info['ends'], E=info['E'], width=info['width'], length=info['length'])


def _same(got, want, tag):
    """got == want: the integer outputs as numbers, the three doubles as bits; names the first polygon that differs"""
    for key in ('ends', 'valid', 'knots', 'E', 'width', 'length'):
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.shape == w.shape and g.dtype == w.dtype, (tag, key, g.shape, w.shape, g.dtype, w.dtype)
        if g.dtype == np.float64:
            g, w = g.view(np.int64), w.view(np.int64)
        if not np.array_equal(g, w):
            k = int(np.flatnonzero((g != w).reshape(len(g), -1).any(1))[0])
            raise AssertionError('%s: %s of polygon %d differs: device %s, host %s' % (tag, key, k, got[key][k].tolist(), want[key][k].tolist()))


def _device(polys, S, ends):
    knots, valid, info = polygon_ribbons_device(polys, S, ends, return_info=True)
    K = len(polys)
    assert knots.shape == (K, S + 1, 4) and knots.dtype == torch.int32 and valid.shape == (K, ) and valid.dtype == torch.uint8
    assert all(a.is_cuda and a.is_contiguous() for a in (knots, valid, *info.values())) and sorted(info) == ['E', 'ends', 'length', 'width']
    return dict(knots=knots.cpu().numpy(), valid=valid.cpu().numpy(), **{k: v.cpu().numpy() for k, v in info.items()})


def _check(polys, S, ends, tag):
    want = _host(polys, S, ends)
    _same(_device(polys, S, ends), want, (tag, S, ends))
    return want


def _broad():
    polys = [p for _, p in general_inputs()] + [ctw_polygon(False), ctw_polygon(True)] + [np.array(p, np.float64) for p in INVALID]
    polys.append(rectangle(-2.0 ** 20, -2.0 ** 20, 2.0 ** 21, 2.0 ** 21))  # a cross-section beyond int32: no ribbon
    polys.append(rectangle(-2.0 ** 20, -2.0 ** 20, 2.0 ** 21, 1000.0))     # the largest coordinates fit: knots at +-2^30
    return polys


@pytest.mark.parametrize('ends', ['auto', 'half'])
@pytest.mark.parametrize('S', [32, 4, 64])
def test_equal_to_the_host(S, ends):
    polys = [p for p in _broad() if ends == 'auto' or len(p) % 2 == 0]
    want = _check(polys, S, ends, 'broad')
    assert 0 < want['valid'].sum() < len(polys)  # ribbons and refusals both
    assert want['valid'][-2] == 0 and want['valid'][-1] == 1 and np.abs(want['knots'][-1, :, 0].astype(np.int64)).max() == 2 ** 30


def test_the_square_ties_go_to_the_smallest_pair():
    sq = rectangle(0, 0, 64, 64)
    polys = [np.roll(sq, s, axis=0) for s in range(4)] + [np.roll(sq[::-1], s, axis=0) for s in range(4)]
    want = _check(polys, 32, 'auto', 'square')
    assert (want['ends'] == want['ends'][0]).all() and want['valid'].all()  # the same indices from every start: the tie rule, not the geometry


def _small_integer_polygons():
    rng = np.random.default_rng(11)
    polys = [rng.integers(0, 16, (int(rng.integers(3, 13)), 2)).astype(np.float64) for _ in range(300)]
    polys += [rng.integers(0, 64, (int(rng.integers(3, 13)), 2)).astype(np.float64) / 4 for _ in range(100)]
    return polys


@pytest.mark.parametrize('S', [32, 4, 64])
def test_exact_ties_and_perfect_squares(S):
    """integer and quarter-pixel vertices on a small grid: exact ties between pairs, repeated points, segments of no length
    and of perfect-square length, all decided as the host decides them"""
    polys = _small_integer_polygons()
    want = _check(polys, S, 'auto', 'grid')
    assert 0 < want['valid'].sum() < len(polys)
    assert any((np.abs(p - np.roll(p, 1, axis=0)).sum(1) == 0).any() for p in polys)  # repeated points are among them
    even = [p for p in polys if len(p) % 2 == 0]
    _check(even, S, 'half', 'grid')


def test_three_vertices():
    rng = np.random.default_rng(5)
    tris = [rng.uniform(0, 200, (3, 2)) for _ in range(20)] + [np.array([[0, 0], [7, 0], [0, 5.0]]), np.array([[1, 1], [1, 1], [4, 9.0]])]
    for S in (4, 32, 64):
        _check(tris, S, 'auto', 'triangles')


def test_256_vertices_at_64_segments():
    """the largest polygon: every LDS table at its full size, loops longer than the workgroup; one polygon, not a batch"""
    rng = np.random.default_rng(9)
    p = curve_ribbon(rng, side=128)
    assert p.shape == (256, 2)
    for ends in ('auto', 'half'):
        want = _check([p], 64, ends, '256')
        assert want['valid'][0] == 1
    point = np.zeros((256, 2)) + [3.0, 4.0]
    want = _check([point], 64, 'auto', '256 x one point')
    assert want['valid'][0] == 0 and not want['knots'].any()


def _mixed(n=1000):
    rng = np.random.default_rng(3)
    polys = []
    for q in range(n):
        kind = q % 4
        if kind == 0:
            side = int(rng.integers(2, 21))
            p = curve_ribbon(rng, side=side)
        elif kind == 1:
            p = rng.integers(0, 300, (int(rng.integers(3, 41)), 2)).astype(np.float64)
        elif kind == 2:
            p = np.round(curve_ribbon(rng, side=int(rng.integers(2, 21))))
        else:
            p = np.array(INVALID[q // 4 % len(INVALID)], np.float64)
        polys.append(p)
    for q in (17, 500, n - 1):
        polys[q] = np.round(curve_ribbon(rng, side=128) * 4) / 4
    return polys


@pytest.fixture(scope='module')
def mixed():
    polys = _mixed()
    return polys, _host(polys, 32, 'auto')


def test_batches_of_none_and_one():
    knots, valid, info = polygon_ribbons_device([], 8, return_info=True)
    assert knots.shape == (0, 9, 4) and valid.shape == (0, ) and info['ends'].shape == (0, 2) and info['E'].shape == (0, ) and knots.is_cuda
    assert lib().dbn_polygon_ribbons_device(None, None, 0, 0, 32, 0, None, None, None, None, stream()) == 0
    _check([general_inputs()[9][1]], 32, 'auto', 'one')


def test_a_mixed_batch_equals_the_host_and_one_call_each(mixed):
    polys, want = mixed
    assert sorted({len(p) for p in polys})[0] == 3 and sum(len(p) == 256 for p in polys) == 3 and 0 < want['valid'].sum() < len(polys)
    got = _device(polys, 32, 'auto')
    _same(got, want, 'mixed')
    _same(_device(polys, 32, 'auto'), got, 'mixed, again')  # two runs agree
    ones = [polygon_ribbons_device([p], 32, 'auto', return_info=True) for p in polys]  # one call each, compared after the last
    for key, pick in (('knots', lambda o: o[0]), ('valid', lambda o: o[1]), ('ends', lambda o: o[2]['ends']), ('E', lambda o: o[2]['E']),
                      ('width', lambda o: o[2]['width']), ('length', lambda o: o[2]['length'])):
        each = torch.cat([pick(o) for o in ones]).cpu().numpy()
        assert np.array_equal(each.view(np.int64) if each.dtype == np.float64 else each,
                              got[key].view(np.int64) if each.dtype == np.float64 else got[key]), key


def _guarded(nbytes):
    buf = torch.full((GUARD + nbytes + GUARD, ), POISON, dtype=torch.uint8, device=DEV)
    return buf, buf[GUARD:GUARD + nbytes]


def _raw(xy, offs, total, S, half):
    """dbn_polygon_ribbons_device on the caller's arrays, into poisoned buffers with guard bytes on both sides ->
    (the outputs as polygon_ribbons gives them, the buffers, the inputs on the device)"""
    K = len(offs) - 1
    x, o = torch.from_numpy(np.ascontiguousarray(xy, np.float64)).to(DEV), torch.from_numpy(np.ascontiguousarray(offs, np.int64)).to(DEV)
    bufs = [_guarded(n) for n in (K * (S + 1) * 4 * 4, K, K * 2 * 4, K * 3 * 8)]
    (kn, va, en, inf) = [v for _, v in bufs]
    check(lib().dbn_polygon_ribbons_device(x.data_ptr(), o.data_ptr(), K, total, S, half, kn.data_ptr(), va.data_ptr(), en.data_ptr(), inf.data_ptr(),
                                           stream()), 'polygon_ribbons_device')
    torch.cuda.synchronize()
    info = inf.cpu().numpy().view(np.float64).reshape(K, 3)
    out = dict(knots=kn.cpu().numpy().view(np.int32).reshape(K, S + 1, 4), valid=va.cpu().numpy(), ends=en.cpu().numpy().view(np.int32).reshape(K, 2),
               E=info[:, 0].copy(), width=info[:, 1].copy(), length=info[:, 2].copy())
    return out, [b for b, _ in bufs], (x, o)


def test_every_output_byte_is_written_and_none_beyond(mixed):
    polys, want = mixed
    polys = polys[:120]
    xy, offs = np.concatenate(polys), np.concatenate([[0], np.cumsum([len(p) for p in polys])]).astype(np.int64)
    out, bufs, (x, o) = _raw(xy, offs, len(xy), 32, 0)
    _same(out, {k: v[:120] for k, v in want.items()}, 'raw')  # equal to the host, so no poison byte is left
    for b in bufs:
        assert bool((b[:GUARD] == POISON).all()) and bool((b[-GUARD:] == POISON).all())
    assert np.array_equal(x.cpu().numpy(), xy) and np.array_equal(o.cpu().numpy(), offs)  # the inputs are unchanged


def _good():
    rng = np.random.default_rng(21)
    return [np.round(curve_ribbon(rng, side=s) * 4) / 4 for s in (4, 7, 3, 10, 5)]  # even counts, for half = 1 too


BAD = ['nan', 'coordinate', 'two vertices', '257 vertices', 'odd with half', 'offsets run back', 'offsets past the end']


@pytest.mark.parametrize('case', BAD)
def test_untrusted_input_spoils_its_own_polygon_only(case):
    """five good polygons with a bad one in the middle.  The result is defined: valid 0, zero knots, ends (-1, -1), info 0
    for the bad one, the host's ribbons for the others.  An offset is shared by the two polygons it separates, so the two
    offset cases are laid out for that: where the offsets run back the later polygons reuse the first two's vertices, and
    an offset past the end spoils both its neighbours (five good ones around them)."""
    good = _good()
    S, half = 16, int(case == 'odd with half')
    bad_poly = rectangle(5, 5, 40, 12)
    if case == 'nan':
        bad_poly = bad_poly.copy()
        bad_poly[2, 1] = np.nan
    elif case == 'coordinate':
        bad_poly = bad_poly + [2.0 ** 20 + 1 - 45, 0]  # the largest x is 2^20 + 1
    elif case == 'two vertices':
        bad_poly = bad_poly[:2]
    elif case == '257 vertices':
        bad_poly = np.zeros((257, 2)) + curve_ribbon(np.random.default_rng(1), side=128)[np.arange(257) % 256]
    elif case == 'odd with half':
        bad_poly = np.concatenate([bad_poly, [[3.0, 9.0]]])
    polys = good[:3] + [bad_poly] + good[3:]
    xy = np.concatenate(polys)
    offs = np.concatenate([[0], np.cumsum([len(p) for p in polys])]).astype(np.int64)
    total, bad, kept = len(xy), [3], {0: good[0], 1: good[1], 2: good[2], 4: good[3], 5: good[4]}
    if case == 'offsets run back':
        # polygons 0 1 2 as laid out, polygon 3 = [offs[3], 0): a negative count, polygons 4 and 5 = the vertices of 0 and 1 again
        offs = np.array([offs[0], offs[1], offs[2], offs[3], offs[0], offs[1], offs[2]], np.int64)
        kept = {0: good[0], 1: good[1], 2: good[2], 4: good[0], 5: good[1]}
    elif case == 'offsets past the end':
        # K = 7: polygon 3 ends past total_vertices, so polygon 4 starts there; 5 and 6 are the vertices of 0 and 1 again
        offs = np.array([offs[0], offs[1], offs[2], offs[3], total + 3, offs[0], offs[1], offs[2]], np.int64)
        bad, kept = [3, 4], {0: good[0], 1: good[1], 2: good[2], 5: good[0], 6: good[1]}
    out, bufs, _ = _raw(xy, offs, total, S, half)
    for k in bad:
        assert out['valid'][k] == 0 and not out['knots'][k].any() and out['ends'][k].tolist() == [-1, -1], (case, k)
        assert out['E'][k].view(np.int64) == 0 and out['width'][k].view(np.int64) == 0 and out['length'][k].view(np.int64) == 0, (case, k)
    rows = sorted(kept)
    want = _host([kept[k] for k in rows], S, 'half' if half else 'auto')
    assert want['valid'].all()
    _same({key: v[rows] for key, v in out.items()}, want, case)
    for b in bufs:
        assert bool((b[:GUARD] == POISON).all()) and bool((b[-GUARD:] == POISON).all())


@pytest.mark.parametrize('ends, S, size', [('auto', 32, (32, 100)), ('half', 32, (32, 100)), ('auto', 8, (48, 160)), ('half', 64, (5, 7))])
def test_rectify_words_gives_the_same_bytes(ends, S, size):
    """the inputs of test_rectify_words_equals_the_restatement, ribbons='device' against ribbons='host'"""
    rng = np.random.default_rng(S + size[0])
    imgs = _images(rng)[2:]
    batch = image_collate([(i, [], None) for i in imgs])
    polys = [_polygons(rng, *i.shape[:2], 5) for i in imgs]
    polys[0].insert(2, np.zeros((4, 2)))                                 # dropped: coordinate sum 0
    polys[1].insert(0, np.array([[0, 0], [9, 9], [18, 18], [27, 27.]]))  # kept, no area: a zero crop
    scores = [list(rng.uniform(0.5, 1.0, len(p))) for p in polys]
    host, index = rectify_words(batch, polys, size, segments=S, ends=ends)
    dev, index_d = rectify_words(batch, polys, size, segments=S, ends=ends, ribbons='device')
    assert dev.shape == (11, ) + size + (3, ) and np.array_equal(index, index_d) and torch.equal(dev, host)
    assert not dev[5].any() and sum(bool(c.any()) for c in dev) == 10
    few_h, idx_h = rectify_words(batch, list(zip(polys, scores)), size, min_score=0.75, segments=S, ends=ends)
    few_d, idx_d = rectify_words(batch, list(zip(polys, scores)), size, min_score=0.75, segments=S, ends=ends, ribbons='device')
    assert 0 < len(few_d) < 11 and np.array_equal(idx_h, idx_d) and torch.equal(few_d, few_h)
    one, _ = rectify_words(torch.from_numpy(imgs[0]), [polys[0]], size, segments=S, ends=ends, ribbons='device')  # an image on the host
    assert torch.equal(one, host[:len(one)])
    # the device half alone: the device tensors in place, and their host copies
    kept = [p for ps in polys for p in ps if p.sum() > 0]
    knots, valid = polygon_ribbons_device(kept, S, ends)
    a = rectify_from_ribbons(batch, knots, valid, index[:, 0], size)
    b = rectify_from_ribbons(batch, knots.cpu().numpy(), valid.cpu().numpy(), index[:, 0], size)
    assert torch.equal(a, host) and torch.equal(b, host)
    for kn, va in ((knots.cpu(), valid), (knots, valid.cpu().numpy()), (knots.long(), valid), (knots[:, :, :2], valid), (knots, valid.int())):
        with pytest.raises(ValueError):
            rectify_from_ribbons(batch, kn, va, index[:, 0], size)


def test_recognize_words_reads_the_same_strings():
    rng = np.random.default_rng(8)
    imgs = [rng.integers(0, 256, (200, 300, 3), dtype=np.uint8) for _ in range(2)]
    batch = image_collate([(i, [], None) for i in imgs])
    polys = [_polygons(rng, 200, 300, 4) for _ in imgs]
    conv = CTCLabelConverter(CHARS)
    host_model, dev_model = _Stub(37, 1).to(DEV), _Stub(37, 1).to(DEV)
    host = recognize_words(batch, None, host_model, conv, polygons=polys)
    dev = recognize_words(batch, None, dev_model, conv, polygons=polys, ribbons='device')
    assert torch.equal(torch.cat(dev_model.images), torch.cat(host_model.images))  # the recogniser saw the same crops
    assert [len(o) for o in dev] == [4, 4] and [w['pred'] for o in dev for w in o] == [w['pred'] for o in host for w in o]
    assert [w['score'] for o in dev for w in o] == [w['score'] for o in host for w in o]
