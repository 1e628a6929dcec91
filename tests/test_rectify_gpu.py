"""GPU (-m gpu): the polygon word crops of csrc/rectify.hip rectify_u8 through db_text_minimal_amd.word_crops, bit for bit
against the restatement tests/rectify_ref.py: mixed batches (image sizes at odd byte offsets, crop sizes, segment counts,
ribbons across and outside the border, knots over the whole int32 range, invalid ribbons), every output byte written and
none beyond, the crop with a known answer (a rectangle is the slice, and crop_words' crop of that box), and end to end
from a probability map through detect_polygons and recognize_words."""
import numpy as np
import pytest
import torch

from db_text_minimal_amd import (CTCLabelConverter, crop_words, detect_polygons, draw_words, image_collate, polygon_ribbons, recognize_words,
                                 rectify_from_ribbons, rectify_words, words_to_input)
from db_text_minimal_amd._lib import check, lib
import recognise_ref as Rr
import rectify_ref as R
from gpu_util import DEV, stream
from test_recognise_gpu import CHARS, _StubCTC
from test_rectify_cpu import curve_ribbon, rectangle, sector

pytestmark = pytest.mark.gpu

SHAPES = [(5, 7), (1, 1), (200, 300), (48, 64)]  # (H, W); packed in this order behind one byte: offsets 1, 106, 109, 180109
SIZES = [(32, 100), (1, 1), (5, 7), (48, 160)]
POISON = 0xA5


def _images(rng):
    out = []
    for H, W in SHAPES:
        y, x = np.mgrid[0:H, 0:W]
        base = (np.stack([x * 7 + y * 3, x * 2 - y * 5, (x ^ y) * 11], -1) % 256).astype(np.uint8)
        out.append(np.where(rng.random((H, W, 1)) < 0.3, rng.integers(0, 256, (H, W, 3), dtype=np.uint8), base).astype(np.uint8))
    return out


def _packed(imgs, shift=1):
    """the images behind `shift` bytes of one buffer: (the flat device view from the first image on, shapes)"""
    flat = np.concatenate([np.zeros(shift, np.uint8)] + [i.reshape(-1) for i in imgs])
    return torch.from_numpy(flat).to(DEV)[shift:], [i.shape[:2] for i in imgs]


def _ribbons(rng, imgs, S, n, size):
    """n ribbons over the images, for crops of `size` ->(image index [n], knots int32 [n, S + 1, 4], valid uint8 [n]), of six kinds"""
    img_of = rng.integers(0, len(imgs), n)
    knots, valid = np.zeros((n, S + 1, 4), np.int32), np.ones(n, np.uint8)
    for q in range(n):
        H, W = imgs[img_of[q]].shape[:2]
        kind = q % 6
        if kind == 0:    # the ribbon of a curved polygon scaled onto the image, often across its border
            p = curve_ribbon(rng, side=6)
            p = (p - p.min(0)) / (p.max(0) - p.min(0)).max() * max(H, W) * rng.uniform(0.5, 1.3) + rng.uniform(-0.3, 0.3, 2) * (W, H)
            k, v = polygon_ribbons([p], S)
            knots[q], valid[q] = k[0], v[0]
        elif kind in (1, 2):  # free knots around the image, at any fraction of a pixel
            c = rng.uniform(-0.3, 1.3, (S + 1, 2)) * (W, H) if kind == 1 else np.cumsum(rng.uniform(-0.2, 0.4, (S + 1, 2)) * (W, H) / S * 4, 0)
            nrm = rng.uniform(-0.5, 0.5, (S + 1, 2)) * max(H, W, 8)
            knots[q] = np.rint(np.concatenate([c, nrm], 1) * 1024)
        elif kind == 3:  # wholly outside
            c = rng.uniform(2, 3, (S + 1, 2)) * (W + 40, H + 40) * rng.choice([-1, 1], 2)
            knots[q] = np.rint(np.concatenate([c, rng.uniform(-20, 20, (S + 1, 2))], 1) * 1024)
        elif kind == 4:  # anything an int32 holds: the 64-bit evaluation at its limits ...
            knots[q] = rng.integers(-2 ** 31, 2 ** 31, (S + 1, 4))
            knots[q, rng.integers(0, S + 1), :] = [2 ** 31 - 1, -2 ** 31, -2 ** 31, 2 ** 31 - 1]
            # ... with one column x brought back onto the image: c_k+1 is solved from w c_k + r (c_k+1 - c_k) = w target
            x = int(rng.integers(0, size[1]))
            k, r = x * S // size[1], x * S % size[1]
            target = np.rint(rng.uniform(0, 1, 2) * (W, H) * 1024).astype(np.int64)
            ck = knots[q, k, :2].astype(np.int64)
            nxt = ck + (size[1] * (target - ck)) // max(r, 1)
            if r == 0 or np.abs(nxt).max() >= 2 ** 31:
                knots[q, k, :2], knots[q, k + 1, :2] = target, target
            else:
                knots[q, k + 1, :2] = nxt
            if q % 12 == 4:  # and half of them with a cross-section of ordinary size
                knots[q, :, 2:] = np.rint(rng.uniform(-0.5, 0.5, (S + 1, 2)) * max(H, W, 8) * 1024)
        else:            # an invalid ribbon, whatever its knots say
            knots[q] = np.rint(np.concatenate([rng.uniform(0, 1, (S + 1, 2)) * (W, H), rng.uniform(-9, 9, (S + 1, 2))], 1) * 1024)
            valid[q] = 0
    return img_of, knots, valid


def _expected(imgs, img_of, knots, valid, size):
    return np.stack([R.rectify(imgs[i], k, v, *size) for i, k, v in zip(img_of, knots, valid)]) if len(knots) else np.zeros((0, ) + size + (3, ), np.uint8)


def _launch(packed, shapes, img_of, knots, valid, size, dst_shift, guard=64):
    """dbn_rectify_u8 into a caller's poisoned buffer with guard bytes on both sides, with the descriptors
    rectify_from_ribbons builds -> (crops, buffer, the inputs on the device)"""
    K, S, (h, w) = len(knots), knots.shape[1] - 1, size
    off = np.concatenate([[0], np.cumsum([H * W * 3 for H, W in shapes])])
    desc = np.array([[off[i], shapes[i][0], shapes[i][1]] for i in img_of], np.int64).reshape(-1, 3)
    d, kn, va = torch.from_numpy(desc).to(DEV), torch.from_numpy(knots).to(DEV), torch.from_numpy(valid).to(DEV)
    n = K * h * w * 3
    buf = torch.full((guard + dst_shift + n + guard, ), POISON, dtype=torch.uint8, device=DEV)
    out = buf[guard + dst_shift:guard + dst_shift + n]
    check(lib().dbn_rectify_u8(packed.data_ptr(), packed.numel(), d.data_ptr(), kn.data_ptr(), va.data_ptr(), K, S, h, w, out.data_ptr(), n,
                               stream()), 'rectify_u8')
    torch.cuda.synchronize()
    return out.view(K, h, w, 3), buf, (d, desc, kn, va)


def _check_batch(rng, size, S, n, dst_shift):
    imgs = _images(rng)
    packed, shapes = _packed(imgs)
    assert packed.data_ptr() % 2 == 1
    keep = packed.clone()
    img_of, knots, valid = _ribbons(rng, imgs, S, n, size)
    want = _expected(imgs, img_of, knots, valid, size)
    got, buf, (d, desc, kn, va) = _launch(packed, shapes, img_of, knots, valid, size, dst_shift)
    g = got.cpu().numpy()
    bad = [q for q in range(n) if not np.array_equal(g[q], want[q])]
    assert not bad, (size, S, bad[:10], [q % 6 for q in bad[:10]])
    lo, hi = 64 + dst_shift, 64 + dst_shift + got.numel()
    assert bool((buf[:lo] == POISON).all()) and bool((buf[hi:] == POISON).all())  # the guards on both sides
    assert torch.equal(packed, keep) and np.array_equal(d.cpu().numpy(), desc) and np.array_equal(kn.cpu().numpy(), knots)
    assert np.array_equal(va.cpu().numpy(), valid)  # the inputs are unchanged
    again, _, _ = _launch(packed, shapes, img_of, knots, valid, size, dst_shift)
    assert torch.equal(again, got)  # two runs, bit for bit
    api = rectify_from_ribbons((packed, shapes), knots, valid, img_of, size)
    assert api.shape == (n, ) + size + (3, ) and api.dtype == torch.uint8 and api.is_cuda and np.array_equal(api.cpu().numpy(), want)
    if n:  # what the batch holds: pixels from inside, zero crops, and the poison value overwritten everywhere
        inside = [q for q in range(n) if valid[q] and want[q].any()]
        assert len(inside) >= n // 12 and all(not want[q].any() for q in range(n) if not valid[q])
        assert n < 36 or any(q % 6 == 4 for q in inside)  # some at the limits of int32 among them
    return want


@pytest.mark.parametrize('S', [4, 32, 64])
@pytest.mark.parametrize('size', SIZES)
def test_bit_equal_to_the_restatement(size, S):
    rng = np.random.default_rng(size[0] * 1000 + size[1] * 10 + S)
    for dst_shift in (0, 1):  # dword stores where the crops allow them, byte stores where not
        _check_batch(rng, size, S, 36, dst_shift)


@pytest.mark.parametrize('size, S', [((32, 100), 32), ((5, 7), 4)])
@pytest.mark.parametrize('n', [0, 1, 1000])
def test_crop_counts(n, size, S):
    _check_batch(np.random.default_rng(n + S), size, S, n, 0)


def test_no_crops_no_launch_and_an_empty_result():
    img = torch.zeros((4, 4, 3), dtype=torch.uint8, device=DEV)
    assert lib().dbn_rectify_u8(None, 0, None, None, None, 0, 32, 32, 100, None, 0, stream()) == 0
    crops, index = rectify_words(img, [[]])
    assert crops.shape == (0, 32, 100, 3) and index.shape == (0, 2)


def _polygons(rng, H, W, n):
    out = []
    for i in range(n):
        p = curve_ribbon(rng, side=int(rng.integers(4, 9))) if i % 3 else sector(rng.uniform(60, 300), side=6)
        p = (p - p.min(0)) / (p.max(0) - p.min(0)).max() * min(H, W) * rng.uniform(0.4, 1.1) + rng.uniform(-0.1, 0.3, 2) * (W, H)
        out.append(np.round(p * 4) / 4)  # quarter pixels: detector output is integer, annotations often are not
    return out


@pytest.mark.parametrize('ends, S, size', [('auto', 32, (32, 100)), ('half', 32, (32, 100)), ('auto', 8, (48, 160)), ('half', 64, (5, 7))])
def test_rectify_words_equals_the_restatement(ends, S, size):
    rng = np.random.default_rng(S + size[0])
    imgs = _images(rng)[2:]
    batch = image_collate([(i, [], None) for i in imgs])
    polys = [_polygons(rng, *i.shape[:2], 5) for i in imgs]
    polys[0].insert(2, np.zeros((4, 2)))                       # dropped: coordinate sum 0
    polys[1].insert(0, np.array([[0, 0], [9, 9], [18, 18], [27, 27.]]))  # kept, no area: a zero crop
    scores = [list(rng.uniform(0.5, 1.0, len(p))) for p in polys]
    crops, index = rectify_words(batch, polys, size, segments=S, ends=ends)
    torch.cuda.synchronize()
    kept = [(n, k) for n in range(2) for k in range(len(polys[n])) if polys[n][k].sum() > 0]
    assert index.tolist() == [list(nk) for nk in kept] and len(kept) == 11 and crops.shape == (11, ) + size + (3, )
    got = crops.cpu().numpy()
    for j, (n, k) in enumerate(kept):
        r = R.ribbon(polys[n][k], S, ends)
        assert np.array_equal(polygon_ribbons([polys[n][k]], S, ends)[0][0], r['knots']), (n, k)  # no rounding tie in these inputs
        assert np.array_equal(got[j], R.rectify(imgs[n], r['knots'], r['valid'], *size)), (n, k)
    assert not got[5].any() and sum(bool(g.any()) for g in got) == 10
    # the (polygons, scores) pairs of detect_polygons, with a threshold
    few, idx = rectify_words(batch, list(zip(polys, scores)), size, min_score=0.75, segments=S, ends=ends)
    sel = [j for j, (n, k) in enumerate(kept) if scores[n][k] >= 0.75]
    assert 0 < len(sel) < 11 and idx.tolist() == [list(kept[j]) for j in sel] and np.array_equal(few.cpu().numpy(), got[sel])
    # one image as a tensor, on the host: the same crops
    one, _ = rectify_words(torch.from_numpy(imgs[0]), [polys[0]], size, segments=S, ends=ends)
    assert np.array_equal(one.cpu().numpy(), got[:len(one)])


def test_a_rectangle_is_the_slice_and_the_crop_of_its_box():
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (90, 150, 3), dtype=np.uint8)
    t = torch.from_numpy(img).to(DEV)
    for (h, w), corners in (((32, 100), [(17, 40), (0, 0), (50, 58)]), ((16, 64), [(3, 5), (86, 74)]), ((8, 128), [(22, 82)])):
        rects = [rectangle(x0, y0, w, h) for x0, y0 in corners]
        for S in (4, 32, 64):
            crops, _ = rectify_words(t, [rects], (h, w), segments=S)
            boxes, _ = crop_words(t, [np.array(rects).astype(np.int16)], (h, w))
            for k, (x0, y0) in enumerate(corners):
                assert np.array_equal(crops[k].cpu().numpy(), img[y0:y0 + h, x0:x0 + w]), (h, w, S, x0, y0)
            assert torch.equal(crops, boxes)
        for start in range(4):  # from any corner, in either orientation
            for flip in (False, True):
                turned = [np.roll(r[::-1] if flip else r, start, axis=0) for r in rects]
                assert torch.equal(rectify_words(t, [turned], (h, w))[0], boxes)


class _Stub(_StubCTC):
    def forward(self, image, text):
        self.images = getattr(self, 'images', []) + [image.clone()]
        return super().forward(image, text)


def test_recognize_words_from_polygons_end_to_end():
    """an arc-shaped blob in a probability map -> detect_polygons -> recognize_words(polygons=...) with a CTC stub: the crops
    the recogniser sees and the strings are the restatement's on the same polygons"""
    Hm, S = 128, 2
    y, x = np.mgrid[0:Hm, 0:Hm]
    rad, ang = np.hypot(x - 64.0, y - 90.0), np.degrees(np.arctan2(90.0 - y, x - 64.0))
    pred = torch.zeros((2, 1, Hm, Hm), dtype=torch.float32)
    pred[0, 0][torch.from_numpy((rad > 44) & (rad < 56) & (ang > 20) & (ang < 160))] = 0.95  # an arch
    pred[1, 0, 20:30, 10:90] = 0.9                                                            # a straight word
    pred[1, 0][torch.from_numpy((np.hypot(x - 60.0, y - 40.0) > 50) & (np.hypot(x - 60.0, y - 40.0) < 60) & (y > 70))] = 0.8  # a bowl
    res = detect_polygons(pred.to(DEV), dest_sizes=[(Hm * S, Hm * S)] * 2)
    assert [len(p) for p, _ in res] == [1, 2] and all(3 <= len(q) <= 256 for p, _ in res for q in p)
    rng = np.random.default_rng(8)
    imgs = [rng.integers(0, 256, (Hm * S, Hm * S, 3), dtype=np.uint8) for _ in range(2)]
    batch = image_collate([(i, [], None) for i in imgs])
    conv, model = CTCLabelConverter(CHARS), _Stub(37, 1).to(DEV)
    out = recognize_words(batch, None, model, conv, polygons=res, batch_size=2)
    ribbons = [R.ribbon(q, 32) for p, _ in res for q in p]
    assert all(r['valid'] for r in ribbons)
    assert 1.2 * np.hypot(*(ribbons[0]['stop'] - ribbons[0]['start'])) < ribbons[0]['length']  # the arch is followed, not cut across
    want = np.stack([R.rectify(imgs[n], r['knots'], 1, 32, 100) for n, r in zip([0, 1, 1], ribbons)])
    crops, index = rectify_words(batch, res)
    assert index.tolist() == [[0, 0], [1, 0], [1, 1]] and np.array_equal(crops.cpu().numpy(), want)
    assert torch.equal(torch.cat(model.images), words_to_input(torch.from_numpy(want).to(DEV)))
    codes, count, _ = Rr.greedy_decode(torch.cat(model.logits).double().cpu().numpy(), 'ctc')
    strings = Rr.strings(codes, count, conv.character)
    assert [len(o) for o in out] == [1, 2] and [w['pred'] for o in out for w in o] == strings and all(len(s) > 0 for s in strings)
    for (n, k), w in zip(index.tolist(), [w for o in out for w in o]):
        assert np.array_equal(w['box'], res[n][0][k]) and isinstance(w['score'], float)
    few = recognize_words(batch, None, model, conv, polygons=res, min_score=2.0)
    assert few == [[], []]
    drawn = draw_words(batch, out)  # the text is anchored at the polygon's first vertex
    assert drawn.numel() == batch[0].numel() and not torch.equal(drawn.cpu().reshape(-1), batch[0].reshape(-1))
    with pytest.raises(ValueError, match='not both'):
        recognize_words(batch, [np.zeros((0, 4, 2), np.int16)] * 2, model, conv, polygons=res)
