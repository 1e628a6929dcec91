"""GPU (-m gpu): the device half of the JPEG decode (csrc/jpeg.hip jpeg_idct_kernel / jpeg_rgb_kernel through
db_text_minimal_amd.jpeg): pixels exactly equal to the golden ones (Pillow's decode, tests/golden/jpeg_cases.npz) as one mixed
batch and one by one, the packed output through augment_images / preprocess_image, DeviceBatches over jpeg_collate against
image_collate, a non-default stream, and a batch with one corrupt member.  Reads tests/golden only."""
import json
import os

import numpy as np
import pytest
import torch

from db_text_minimal_amd import (CorruptJpeg, DeviceBatches, UnsupportedJpeg, augment_images, decode_coefficients, decode_jpeg,
                                 decode_jpeg_batch, entropy_decode, image_collate, jpeg_collate, plan_augment, preprocess_image)
from gpu_util import DEV

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jpeg_cases.npz')


def golden():
    g = np.load(GOLDEN)
    names = json.loads(str(g['names']))
    return names, [g['jpeg_%d' % i].tobytes() for i in range(len(names))], [g['rgb_%d' % i] for i in range(len(names))], g


def _split(packed, shapes):
    out, o = [], 0
    flat = packed.cpu().numpy()
    for h, w in shapes:
        out.append(flat[o:o + h * w * 3].reshape(h, w, 3))
        o += h * w * 3
    assert o == flat.size
    return out


def test_mixed_batch_equals_golden_exactly():
    names, datas, rgbs, _ = golden()
    packed, shapes = decode_jpeg_batch(datas, DEV)
    torch.cuda.synchronize()
    assert packed.is_cuda and packed.dtype == torch.uint8 and packed.dim() == 1
    assert shapes == [r.shape[:2] for r in rgbs]
    for n, got, want in zip(names, _split(packed, shapes), rgbs):
        assert np.array_equal(got, want), '%s: %d values differ' % (n, int((got != want).sum()))


def test_one_by_one_equals_golden_exactly():
    names, datas, rgbs, _ = golden()
    for n, d, want in zip(names, datas, rgbs):
        got = decode_jpeg(d, DEV)
        assert got.shape == want.shape and got.dtype == torch.uint8 and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), want), n


def test_every_order_of_alignment():
    """the packed layout gives an image's first byte any alignment: batches that start the large cases at offsets 1, 2, 3 mod 4"""
    names, datas, rgbs, _ = golden()
    odd = [i for i, r in enumerate(rgbs) if (r.size % 4) != 0][:3]
    big = [names.index('640x480_420_strokes_q75'), names.index('250x131_420_ramp_q75'), names.index('637x479_422_strokes_q30')]
    for lead in (odd[:1], odd[:2], odd[:3]):
        order = list(lead) + big
        packed, shapes = decode_jpeg_batch([datas[i] for i in order], DEV)
        for i, got in zip(order, _split(packed, shapes)):
            assert np.array_equal(got, rgbs[i]), names[i]


def test_packed_output_through_augment_and_preprocess():
    names, datas, rgbs, _ = golden()
    pick = [i for i, r in enumerate(rgbs) if min(r.shape[:2]) >= 17][:12]
    packed, shapes = decode_jpeg_batch([datas[i] for i in pick], DEV)
    want_packed = torch.from_numpy(np.concatenate([rgbs[i].reshape(-1) for i in pick])).to(DEV)
    assert torch.equal(packed, want_packed)
    polys = [[np.array([[1, 1], [w // 2, 1], [w // 2, h // 2], [1, h // 2]], np.float64)] for h, w in shapes]
    plans = plan_augment(shapes, polys, np.random.RandomState(9), 96)
    a = augment_images(packed, shapes, plans, 96)
    b = augment_images(want_packed, shapes, plans, 96)
    assert torch.equal(a, b)
    assert torch.equal(augment_images(packed, shapes, None, 64), augment_images(want_packed, shapes, None, 64))
    i = names.index('640x480_420_strokes_q75')
    one = decode_jpeg(datas[i], DEV)
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
def test_device_batches_over_jpeg_collate_equals_image_collate(training):
    names, datas, rgbs, _ = golden()
    pick = [names.index(n) for n in ('100x75_420_ramp_q75_opt', '250x131_420_ramp_q75', '100x75_444_noise_q95_opt', '250x131_grey_strokes_q95')]
    polys = []
    for i in pick:
        h, w = rgbs[i].shape[:2]
        polys.append([np.array([[5, 5], [w // 2, 6], [w // 2, h // 2], [5, h // 2]], np.float64),
                      np.array([[w // 2 + 4, h // 2 + 4], [w - 6, h // 2 + 4], [w - 6, h - 5], [w // 2 + 4, h - 5]], np.float64)])
    S = 96
    a = DeviceBatches(torch.utils.data.DataLoader(_Items([datas[i] for i in pick], polys), batch_size=2, collate_fn=jpeg_collate), DEV, training,
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


def test_non_default_stream():
    names, datas, rgbs, _ = golden()
    s = torch.cuda.Stream()
    obj = entropy_decode(datas)
    with torch.cuda.stream(s):
        packed, shapes = decode_coefficients(obj, DEV)
        total = packed.to(torch.int64).sum()
    s.synchronize()
    assert int(total) == int(sum(int(r.sum(dtype=np.int64)) for r in rgbs))
    for n, got, want in zip(names, _split(packed, shapes), rgbs):
        assert np.array_equal(got, want), n


def test_batch_with_one_corrupt_member():
    names, datas, rgbs, g = golden()
    i, j = names.index('100x75_422_noise_q75_rst_rows'), names.index('250x131_420_ramp_q75')
    k = [n.startswith('17x33_444_') for n in names].index(True)
    cut = datas[j][:len(datas[j]) // 2]
    batch = [datas[i], cut, datas[k], g['refused_progressive'].tobytes(), datas[j]]
    with pytest.raises(CorruptJpeg, match='image 1'):
        decode_jpeg_batch(batch, DEV)
    packed, shapes, errs = decode_jpeg_batch(batch, DEV, errors='report')
    assert [e is None for e in errs] == [True, False, True, False, True]
    assert isinstance(errs[1], CorruptJpeg) and errs[1].index == 1 and isinstance(errs[3], UnsupportedJpeg) and 'progressive' in str(errs[3])
    assert shapes[1] == (0, 0) and shapes[3] == (0, 0)
    got = _split(packed, shapes)
    for pos, src in ((0, i), (2, k), (4, j)):
        assert np.array_equal(got[pos], rgbs[src])
    with pytest.raises(UnsupportedJpeg, match='progressive'):
        decode_jpeg(g['refused_progressive'].tobytes(), DEV)


def test_fallback_splices_refused_images(monkeypatch):
    """fallback=True: a refused kind goes through the fallback decoder (a stand-in here: the GPU suite reads no PIL) and is
    spliced into the packed batch at its place; a corrupt stream still raises"""
    from db_text_minimal_amd import jpeg as J
    names, datas, rgbs, g = golden()
    prog, cmyk = g['refused_progressive'].tobytes(), g['refused_cmyk'].tobytes()
    stand_in = {prog: rgbs[20][:16, :24].copy(), cmyk: rgbs[22][:9, :31].copy()}
    monkeypatch.setattr(J, '_pil_rgb', lambda data: np.ascontiguousarray(stand_in[bytes(data)]))
    batch = [prog, datas[16], cmyk, datas[21]]
    packed, shapes = decode_jpeg_batch(batch, DEV, fallback=True)
    assert packed.is_cuda and shapes == [(16, 24), rgbs[16].shape[:2], (9, 31), rgbs[21].shape[:2]]
    for got, want in zip(_split(packed, shapes), [stand_in[prog], rgbs[16], stand_in[cmyk], rgbs[21]]):
        assert np.array_equal(got, want)
    assert torch.equal(decode_jpeg(prog, DEV, fallback=True).cpu(), torch.from_numpy(stand_in[prog]))
    with pytest.raises(UnsupportedJpeg):
        decode_jpeg_batch(batch, DEV)
    with pytest.raises(CorruptJpeg):
        decode_jpeg_batch(batch + [datas[21][:200]], DEV, fallback=True)
