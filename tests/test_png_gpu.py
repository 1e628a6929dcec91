"""GPU (-m gpu): the device half of the PNG decode (csrc/png.hip png_unfilter_kernel / png_pixels_kernel through
db_text_minimal_amd.png): pixels exactly equal to the golden ones (Pillow's decode, tests/golden/png_cases.npz) as one mixed batch
and one by one, at every alignment of the packed layout, into poisoned workspaces, with a corrupt member, through
augment_images / preprocess_image, DeviceBatches over png_collate against image_collate, on a non-default stream, and
decode_image_batch on an interleaved JPEG / PNG list.  Reads tests/golden only."""
import json
import os

import numpy as np
import pytest
import torch

from db_text_minimal_amd import (CorruptPng, DeviceBatches, UnsupportedPng, augment_images, decode_image_batch, decode_jpeg_batch, decode_png,
                                 decode_png_batch, image_collate, inflate_png, plan_augment, png_collate, preprocess_image, unfilter_png)
from gpu_util import DEV

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BIG = ('pillow_RGB_640x480_strokes', 'pillow_RGB_637x479_strokes', 'chunk_2100x9', 'band_5x2100_cycle', 'adam7_rgba16_100x75')


@pytest.fixture(scope='module')
def golden():
    g = np.load(os.path.join(HERE, 'golden', 'png_cases.npz'))
    names = json.loads(str(g['names']))
    return names, [g['png_%d' % i].tobytes() for i in range(len(names))], [g['rgb_%d' % i] for i in range(len(names))], g


def _split(packed, shapes):
    out, o = [], 0
    flat = packed.cpu().numpy()
    for h, w in shapes:
        out.append(flat[o:o + h * w * 3].reshape(h, w, 3))
        o += h * w * 3
    assert o == flat.size
    return out


def test_mixed_batch_equals_golden_exactly(golden):
    names, datas, rgbs, _ = golden
    packed, shapes = decode_png_batch(datas, DEV)
    torch.cuda.synchronize()
    assert packed.is_cuda and packed.dtype == torch.uint8 and packed.dim() == 1
    assert shapes == [r.shape[:2] for r in rgbs]
    for n, got, want in zip(names, _split(packed, shapes), rgbs):
        assert np.array_equal(got, want), '%s: %d values differ' % (n, int((got != want).sum()))


def test_one_by_one_equals_golden_exactly(golden):
    names, datas, rgbs, _ = golden
    for n, d, want in zip(names, datas, rgbs):
        got = decode_png(d, DEV)
        assert got.shape == want.shape and got.dtype == torch.uint8 and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), want), n


def test_every_order_of_alignment(golden):
    """the packed layout gives an image's first byte any alignment: batches that start the large cases at offsets 1, 2, 3 mod 4"""
    names, datas, rgbs, _ = golden
    lead = names.index('size_b8_1x1')  # three bytes
    big = [names.index(n) for n in BIG]
    for k in (1, 2, 3):
        order = [lead] * k + big
        packed, shapes = decode_png_batch([datas[i] for i in order], DEV)
        assert (3 * k) % 4 == (0, 3, 2, 1)[k]
        for i, got in zip(order, _split(packed, shapes)):
            assert np.array_equal(got, rgbs[i]), names[i]


def test_poisoned_workspaces_give_the_same_bits(golden):
    """nothing read is left from an earlier use of the memory: two runs into workspaces filled with different bytes agree"""
    names, datas, rgbs, _ = golden
    obj = inflate_png(datas)
    outs = []
    for poison in (0x00, 0xA5, 0xFF):
        raw = torch.full((obj.raw_bytes, ), poison, dtype=torch.uint8, device=DEV)
        packed, shapes = unfilter_png(obj, DEV, _raw=raw)
        outs.append(packed.clone())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert torch.equal(outs[0].cpu(), torch.from_numpy(np.concatenate([r.reshape(-1) for r in rgbs])))


def test_batch_with_one_corrupt_member(golden):
    names, datas, rgbs, g = golden
    i, j, k = names.index('size_b8_100x75'), names.index('adam7_pal4_13x10'), names.index('pair_ct4_d16_17x33')
    batch = [datas[i], g['corrupt_crc'].tobytes(), datas[j], g['refused_cgbi'].tobytes(), datas[k]]
    with pytest.raises(CorruptPng, match='image 1'):
        decode_png_batch(batch, DEV)
    packed, shapes, errs = decode_png_batch(batch, DEV, errors='report')
    assert [e is None for e in errs] == [True, False, True, False, True]
    assert isinstance(errs[1], CorruptPng) and errs[1].index == 1 and isinstance(errs[3], UnsupportedPng) and 'CgBI' in str(errs[3])
    assert shapes[1] == (0, 0) and shapes[3] == (0, 0)
    got = _split(packed, shapes)
    for pos, src in ((0, i), (2, j), (4, k)):
        assert np.array_equal(got[pos], rgbs[src])
    for kind in ('corrupt_truncated_idat', 'corrupt_filter5', 'corrupt_zero_width', 'corrupt_depth3', 'corrupt_no_iend'):
        with pytest.raises(CorruptPng):
            decode_png(g[kind].tobytes(), DEV)
    with pytest.raises(UnsupportedPng, match='CgBI'):
        decode_png(g['refused_cgbi'].tobytes(), DEV)
    packed, shapes, errs = decode_png_batch([g['corrupt_crc'].tobytes()], DEV, errors='report')  # nothing decodable: nothing launched
    assert packed.numel() == 0 and shapes == [(0, 0)] and isinstance(errs[0], CorruptPng)


def test_fallback_splices_refused_images(golden, monkeypatch):
    """fallback=True: a refused kind goes through the fallback decoder (a stand-in here: the GPU suite reads no PIL)"""
    from db_text_minimal_amd import png as P
    names, datas, rgbs, g = golden
    cgbi = g['refused_cgbi'].tobytes()
    stand_in = rgbs[names.index('size_b8_100x75')][:9, :31].copy()
    monkeypatch.setattr(P, '_pil_rgb', lambda data: np.ascontiguousarray(stand_in))
    i = names.index('size_b16_17x33')
    packed, shapes = decode_png_batch([cgbi, datas[i]], DEV, fallback=True)
    assert shapes == [(9, 31), rgbs[i].shape[:2]]
    for got, want in zip(_split(packed, shapes), [stand_in, rgbs[i]]):
        assert np.array_equal(got, want)
    with pytest.raises(CorruptPng):
        decode_png_batch([cgbi, g['corrupt_crc'].tobytes()], DEV, fallback=True)


def test_packed_output_through_augment_and_preprocess(golden):
    names, datas, rgbs, _ = golden
    pick = [i for i, r in enumerate(rgbs) if min(r.shape[:2]) >= 17 and max(r.shape[:2]) <= 100][:12]
    packed, shapes = decode_png_batch([datas[i] for i in pick], DEV)
    want_packed = image_collate([(rgbs[i], [], []) for i in pick])[0].to(DEV)
    assert torch.equal(packed, want_packed)
    polys = [[np.array([[1, 1], [w // 2, 1], [w // 2, h // 2], [1, h // 2]], np.float64)] for h, w in shapes]
    plans = plan_augment(shapes, polys, np.random.RandomState(9), 96)
    assert torch.equal(augment_images(packed, shapes, plans, 96), augment_images(want_packed, shapes, plans, 96))
    assert torch.equal(augment_images(packed, shapes, None, 64), augment_images(want_packed, shapes, None, 64))
    i = names.index('pillow_RGB_640x480_strokes')
    one = decode_png(datas[i], DEV)
    for pad in (False, True):
        assert torch.equal(preprocess_image(one, 320, pad=pad), preprocess_image(torch.from_numpy(rgbs[i]).to(DEV), 320, pad=pad))


class _Items(torch.utils.data.Dataset):
    def __init__(self, firsts, polys):
        self.firsts, self.polys = firsts, polys

    def __len__(self):
        return len(self.firsts)

    def __getitem__(self, i):
        return self.firsts[i], self.polys[i], ['w', '###']


@pytest.mark.parametrize('training', [True, False])
def test_device_batches_over_png_collate_equals_image_collate(golden, training):
    names, datas, rgbs, _ = golden
    pick = [names.index(n) for n in ('size_b8_100x75', 'adam7_rgba16_100x75', 'pillow_P_100x75', 'size_sub_100x75')]
    polys = []
    for i in pick:
        h, w = rgbs[i].shape[:2]
        polys.append([np.array([[5, 5], [w // 2, 6], [w // 2, h // 2], [5, h // 2]], np.float64),
                      np.array([[w // 2 + 4, h // 2 + 4], [w - 6, h // 2 + 4], [w - 6, h - 5], [w // 2 + 4, h - 5]], np.float64)])
    S = 96
    a = DeviceBatches(torch.utils.data.DataLoader(_Items([datas[i] for i in pick], polys), batch_size=2, collate_fn=png_collate), DEV, training,
                      size=S, seed=11)
    b = DeviceBatches(torch.utils.data.DataLoader(_Items([rgbs[i] for i in pick], polys), batch_size=2, collate_fn=image_collate), DEV, training,
                      size=S, seed=11)
    n = 0
    for x, y in zip(a, b):
        assert x.keys() == y.keys()
        for k in x:
            if torch.is_tensor(x[k]):
                assert torch.equal(x[k], y[k]), k
            elif k == 'anns':
                assert all(np.array_equal(p, q) for u, v in zip(x[k], y[k]) for p, q in zip(u, v))
            else:
                assert x[k] == y[k], k
        n += 1
    assert n == 2


def test_non_default_stream(golden):
    names, datas, rgbs, _ = golden
    s = torch.cuda.Stream()
    obj = inflate_png(datas)
    with torch.cuda.stream(s):
        packed, shapes = unfilter_png(obj, DEV)
        total = packed.to(torch.int64).sum()
    s.synchronize()
    assert int(total) == int(sum(int(r.sum(dtype=np.int64)) for r in rgbs))
    for n, got, want in zip(names, _split(packed, shapes), rgbs):
        assert np.array_equal(got, want), n


def test_decode_image_batch_on_an_interleaved_list(golden):
    names, datas, rgbs, g = golden
    j = np.load(os.path.join(HERE, 'golden', 'jpeg_cases.npz'))
    jpegs = [j['jpeg_%d' % i].tobytes() for i in (0, 5, 9)]
    pngs = [datas[names.index(n)] for n in ('size_b8_17x33', 'adam7_grey2_13x10', 'pillow_LA_100x75', 'band_5x2100_f3')]
    mixed = [pngs[0], jpegs[0], jpegs[1], pngs[1], pngs[2], jpegs[2], pngs[3]]
    kinds = 'pjjppjp'
    packed, shapes = decode_image_batch(mixed, DEV)
    jp, js = decode_jpeg_batch(jpegs, DEV)
    pp, ps = decode_png_batch(pngs, DEV)
    want = {'j': iter(zip(_split(jp, js), js)), 'p': iter(zip(_split(pp, ps), ps))}
    for k, got, shape in zip(kinds, _split(packed, shapes), shapes):
        img, s = next(want[k])
        assert shape == s and np.array_equal(got, img)
    assert torch.equal(decode_image_batch(pngs, DEV)[0], pp) and torch.equal(decode_image_batch(jpegs, DEV)[0], jp)
    bad = mixed[:3] + [g['corrupt_crc'].tobytes()] + mixed[3:]
    with pytest.raises(CorruptPng, match='image 3'):
        decode_image_batch(bad, DEV)
    packed, shapes, errs = decode_image_batch(bad, DEV, errors='report')
    assert [e is None for e in errs] == [True, True, True, False, True, True, True, True] and errs[3].index == 3 and shapes[3] == (0, 0)
    assert torch.equal(packed, decode_image_batch(mixed, DEV)[0])
