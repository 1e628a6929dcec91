"""GPU (-m gpu): JPEG streams of more than one scan through the whole decode (entropy_decode(..., multiscan=True) on the host,
csrc/jpeg.hip's pixel kernels on the device): pixels exactly equal to the golden ones (Pillow's decode,
tests/golden/jpeg_scans_cases.npz) in one mixed batch with a damaged member, the refusals without the keyword and with
entropy='device', and DeviceBatches over the multiscan collate against image_collate.  Reads tests/golden only."""
import json
import os

import numpy as np
import pytest
import torch

from db_text_minimal_amd import CorruptJpeg, DeviceBatches, UnsupportedJpeg, decode_jpeg, decode_jpeg_batch, image_collate, jpeg_multiscan_collate
from gpu_util import DEV

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    g = np.load(os.path.join(HERE, 'golden', name))
    names = json.loads(str(g['names']))
    return names, [g['jpeg_%d' % i].tobytes() for i in range(len(names))], [g['rgb_%d' % i] for i in range(len(names))]


def _split(packed, shapes):
    out, o = [], 0
    flat = packed.cpu().numpy()
    for h, w in shapes:
        out.append(flat[o:o + h * w * 3].reshape(h, w, 3))
        o += h * w * 3
    assert o == flat.size
    return out


def _mixed():
    names, datas, rgbs = _load('jpeg_scans_cases.npz')
    bn, bd, br = _load('jpeg_cases.npz')
    pick = [bn.index('100x75_420_ramp_q75_opt'), bn.index('100x75_422_noise_q75_rst_rows'), [n.startswith('17x33_444_') for n in bn].index(True)]
    big = names.index([n for n in names if n.startswith('640x480_')][0])
    batch = datas[:6] + [bd[pick[0]]] + datas[6:20] + [datas[big][:len(datas[big]) // 2], bd[pick[1]]] + datas[20:] + [bd[pick[2]]]
    want = rgbs[:6] + [br[pick[0]]] + rgbs[6:20] + [None, br[pick[1]]] + rgbs[20:] + [br[pick[2]]]
    kinds = ['scans'] * 6 + ['baseline'] + ['scans'] * 14 + ['cut', 'baseline'] + ['scans'] * (len(datas) - 20) + ['baseline']
    return batch, want, kinds


def test_mixed_batch_equals_golden_exactly():
    batch, want, kinds = _mixed()
    packed, shapes, errs = decode_jpeg_batch(batch, DEV, multiscan=True, errors='report')
    torch.cuda.synchronize()
    assert packed.is_cuda and packed.dtype == torch.uint8 and packed.dim() == 1
    assert packed.numel() == sum(w.size for w in want if w is not None)  # the failed member takes no bytes
    for i, (got, w, k) in enumerate(zip(_split(packed, shapes), want, kinds)):
        if k == 'cut':
            assert isinstance(errs[i], CorruptJpeg) and errs[i].index == i and shapes[i] == (0, 0)
        else:
            assert errs[i] is None and got.shape == w.shape and np.array_equal(got, w), '%d: %d values differ' % (i, int((got != w).sum()))
    with pytest.raises(CorruptJpeg, match='image %d' % kinds.index('cut')):
        decode_jpeg_batch(batch, DEV, multiscan=True)
    i = kinds.index('scans')
    assert np.array_equal(decode_jpeg(batch[i], DEV, multiscan=True).cpu().numpy(), want[i])


def test_without_the_keyword_the_batch_is_refused():
    batch, want, kinds = _mixed()
    packed, shapes, errs = decode_jpeg_batch(batch, DEV, errors='report')
    for i, k in enumerate(kinds):
        if k == 'scans':
            assert isinstance(errs[i], UnsupportedJpeg) and errs[i].code in (3, 9) and shapes[i] == (0, 0)
        elif k == 'baseline':
            assert errs[i] is None
    got = [g for g, k in zip(_split(packed, shapes), kinds) if k == 'baseline']
    assert all(np.array_equal(a, b) for a, b in zip(got, [w for w, k in zip(want, kinds) if k == 'baseline']))
    with pytest.raises(UnsupportedJpeg):
        decode_jpeg_batch(batch, DEV)
    with pytest.raises(UnsupportedJpeg, match='progressive'):
        decode_jpeg(batch[0], DEV)


def test_device_entropy_does_not_take_the_keyword():
    batch, _, _ = _mixed()
    with pytest.raises(ValueError, match='multiscan'):
        decode_jpeg_batch(batch[:3], DEV, entropy='device', multiscan=True)
    with pytest.raises(ValueError, match='multiscan'):
        decode_jpeg(batch[0], DEV, entropy='device', multiscan=True)


class _Items(torch.utils.data.Dataset):
    def __init__(self, firsts, polys):
        self.firsts, self.polys = firsts, polys

    def __len__(self):
        return len(self.firsts)

    def __getitem__(self, i):
        return self.firsts[i], self.polys[i], ['w', '###']


@pytest.mark.parametrize('training', [True, False])
def test_device_batches_over_the_multiscan_collate_equals_image_collate(training):
    names, datas, rgbs = _load('jpeg_scans_cases.npz')
    pick = [i for i, n in enumerate(names) if n.startswith(('96x80_420', '53x37_422', '96x80_grey')) or '_multi_y_then_cbcr_dri' in n][:4]
    assert len(pick) == 4
    polys = []
    for i in pick:
        h, w = rgbs[i].shape[:2]
        polys.append([np.array([[5, 5], [w // 2, 6], [w // 2, h // 2], [5, h // 2]], np.float64),
                      np.array([[w // 2 + 4, h // 2 + 4], [w - 6, h // 2 + 4], [w - 6, h - 5], [w // 2 + 4, h - 5]], np.float64)])
    S = 96
    a = DeviceBatches(torch.utils.data.DataLoader(_Items([datas[i] for i in pick], polys), batch_size=2, collate_fn=jpeg_multiscan_collate), DEV,
                      training, size=S, seed=11)
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
