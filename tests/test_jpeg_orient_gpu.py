"""GPU (-m gpu): the Exif orientation applied on the device (csrc/jpeg.hip jpeg_rgb_oriented_kernel through orient=True): every tag
on every partial-tile case of the 32-pixel tile equal to the numpy permutation of the unoriented decode (and to Pillow's
ImageOps.exif_transpose where Pillow imports), one packed batch whose members start at every offset mod 4, both entropy
paths, and DeviceBatches(orient=True) against image_collate of the array turned beforehand."""
import io
import json
import os

import numpy as np
import pytest
import torch

from db_text_minimal_amd import DeviceBatches, decode_jpeg, decode_jpeg_batch, image_collate, jpeg_collate, jpeg_stream_collate
from db_text_minimal_amd.jpeg import orient_array
from gpu_util import DEV
import jpeg_enc_ref as E
from test_jpeg_cpu import with_exif

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [(1, 1), (1, 9), (9, 1), (7, 5), (31, 33), (32, 32), (33, 65), (37, 53), (64, 96)]  # (H, W): every partial-tile case of 32 x 32
_made = {}


def _load(name):
    g = np.load(os.path.join(HERE, 'golden', name))
    names = json.loads(str(g['names']))
    return names, [g['jpeg_%d' % i].tobytes() for i in range(len(names))], [g['rgb_%d' % i] for i in range(len(names))]


def turned(a, tag):
    """output pixel (y', x') of tag t is source pixel: 2 (y', W-1-x'), 3 (H-1-y', W-1-x'), 4 (H-1-y', x'), 5 (x', y'), 6 (H-1-x', y'),
    7 (H-1-x', W-1-y'), 8 (x', W-1-y'): written out index by index, on purpose not with the package's orient_array"""
    H, W = a.shape[:2]
    oh, ow = (W, H) if tag >= 5 else (H, W)
    y, x = np.mgrid[0:oh, 0:ow]
    sy, sx = {1: (y, x), 2: (y, W - 1 - x), 3: (H - 1 - y, W - 1 - x), 4: (H - 1 - y, x), 5: (x, y), 6: (H - 1 - x, y), 7: (H - 1 - x, W - 1 - y),
              8: (x, W - 1 - y)}[tag]
    return np.ascontiguousarray(a[sy, sx])


def stream(h, w, mode):
    """a baseline stream of a seeded noise image, coded by tests/jpeg_enc_ref.py (made once)"""
    if (h, w, mode) not in _made:
        rng = np.random.default_rng(h * 1000 + w)
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        img[:, :, 0] = (np.add.outer(np.arange(h) * 7, np.arange(w) * 3) % 256).astype(np.uint8)  # a gradient: a turn cannot hide in noise
        _made[h, w, mode] = E.encode(img[:, :, 0] if mode == 'grey' else img, 90, '444' if mode == 'grey' else mode)
    return _made[h, w, mode]


def _split(packed, shapes):
    out, o = [], 0
    flat = packed.cpu().numpy()
    for h, w in shapes:
        out.append(flat[o:o + h * w * 3].reshape(h, w, 3))
        o += h * w * 3
    assert o == flat.size
    return out


@pytest.mark.parametrize('mode', ['grey', '444', '420'])
def test_every_tag_and_partial_tile_is_the_permutation_of_the_unoriented_decode(mode):
    try:
        from PIL import Image, ImageOps
    except ImportError:
        Image = None
    for h, w in SIZES:
        d = stream(h, w, mode)
        plain = decode_jpeg(d, DEV).cpu().numpy()
        assert plain.shape == (h, w, 3)
        assert np.array_equal(decode_jpeg(d, DEV, orient=True).cpu().numpy(), plain)  # no Exif: nothing to apply
        for tag in range(1, 9):
            t = with_exif(d, tag, 'II' if tag % 2 else 'MM')
            got = decode_jpeg(t, DEV, orient=True)
            assert got.is_cuda and got.dtype == torch.uint8
            assert tuple(got.shape) == ((w, h, 3) if tag >= 5 else (h, w, 3)), (h, w, tag)
            got = got.cpu().numpy()
            assert np.array_equal(got, turned(plain, tag)), (h, w, tag, int((got != turned(plain, tag)).sum()))
            assert np.array_equal(decode_jpeg(t, DEV).cpu().numpy(), plain)  # the default leaves the image as stored
            if Image is not None:
                pil = np.asarray(ImageOps.exif_transpose(Image.open(io.BytesIO(t))).convert('RGB'))
                assert np.array_equal(got, pil), (h, w, tag)
    a = np.arange(3 * 4 * 3).reshape(3, 4, 3)
    assert all(np.array_equal(orient_array(a, tag), turned(a, tag)) for tag in range(1, 9))


def _packed_batch():
    names, datas, rgbs = _load('jpeg_scans_cases.npz')
    p = names.index([n for n in names if n.startswith('53x37_420') and '_prog' in n][0])
    base = stream(37, 53, '420')
    batch = [stream(1, 1, '444')] + [with_exif(base, t) for t in range(1, 9)] + [stream(7, 5, 'grey'), base[:len(base) // 2],
                                                                                with_exif(datas[p], 6), with_exif(stream(33, 65, '444'), 7), base]
    tags = [0] + list(range(1, 9)) + [0, 0, 6, 7, 0]
    return batch, tags, rgbs[p]


def test_one_packed_batch_holds_every_tag_at_every_alignment():
    batch, tags, prog_rgb = _packed_batch()
    plain, pshapes, perrs = decode_jpeg_batch(batch, DEV, multiscan=True, errors='report')
    packed, shapes, errs = decode_jpeg_batch(batch, DEV, multiscan=True, orient=True, errors='report')
    torch.cuda.synchronize()
    assert [e is None for e in errs] == [e is None for e in perrs] == [i != 10 for i in range(len(batch))]
    assert shapes[10] == (0, 0) and packed.numel() == plain.numel() == sum(h * w * 3 for h, w in shapes)
    starts = np.cumsum([0] + [h * w * 3 for h, w in shapes])[:-1]
    assert {int(s) % 4 for s, t in zip(starts, tags) if t >= 2} == {0, 1, 2, 3}
    for i, (got, src, tag) in enumerate(zip(_split(packed, shapes), _split(plain, pshapes), tags)):
        if i == 10:
            continue
        want = turned(src, tag) if tag else src
        assert got.shape == want.shape and np.array_equal(got, want), (i, tag)
    assert np.array_equal(_split(packed, shapes)[11], turned(prog_rgb, 6))  # the progressive member against the golden pixels


def test_orient_on_files_without_exif_changes_nothing():
    names, datas, rgbs = _load('jpeg_cases.npz')
    a, sa = decode_jpeg_batch(datas, DEV)
    b, sb = decode_jpeg_batch(datas, DEV, orient=True)
    assert sa == sb and torch.equal(a, b)


def test_both_entropy_paths_give_the_same_oriented_bytes():
    batch, tags, _ = _packed_batch()
    keep = [i for i in range(len(batch)) if i not in (10, 11)]  # the device Huffman stage takes neither multi-scan nor (without errors='report') damage
    batch = [batch[i] for i in keep]
    a, sa = decode_jpeg_batch(batch, DEV, orient=True)
    b, sb = decode_jpeg_batch(batch, DEV, orient=True, entropy='device')
    assert sa == sb and torch.equal(a, b)
    assert sa[5] == (53, 37) and sa[1] == (37, 53)


class _Items(torch.utils.data.Dataset):
    def __init__(self, firsts, polys):
        self.firsts, self.polys = firsts, polys

    def __len__(self):
        return len(self.firsts)

    def __getitem__(self, i):
        return self.firsts[i], self.polys[i], ['w']


@pytest.mark.parametrize('collate', [jpeg_collate, jpeg_stream_collate])
def test_device_batches_orient_equals_image_collate_of_the_turned_array(collate):
    d = stream(64, 96, '420')
    plain = decode_jpeg(d, DEV).cpu().numpy()
    rot = turned(plain, 6)  # 96 x 64: what cv2.imread shows, and what the polygons are drawn on
    polys = [[np.array([[5, 5], [40, 6], [40, 60], [5, 60]], np.float64)]] * 2
    S = 96
    a = DeviceBatches(torch.utils.data.DataLoader(_Items([with_exif(d, 6), d], polys), batch_size=2, collate_fn=collate), DEV, False, size=S,
                      orient=True)
    b = DeviceBatches(torch.utils.data.DataLoader(_Items([rot, plain], polys), batch_size=2, collate_fn=image_collate), DEV, False, size=S)
    (x, ), (y, ) = list(a), list(b)
    assert x.keys() == y.keys()
    for k in x:
        if torch.is_tensor(x[k]):
            assert torch.equal(x[k], y[k]), k
    c = DeviceBatches(torch.utils.data.DataLoader(_Items([with_exif(d, 6), d], polys), batch_size=2, collate_fn=collate), DEV, False, size=S)
    (z, ) = list(c)
    assert not torch.equal(z['img'][0], x['img'][0]) and torch.equal(z['img'][1], x['img'][1])  # the default still decodes as stored


def test_fallback_images_are_turned_too(monkeypatch):
    """fallback=True with orient=True: the image the fallback decoder returns (a stand-in here: the GPU suite reads no PIL) is
    turned by the tag this package's own parser reads, and spliced in at its place"""
    from db_text_minimal_amd import jpeg as J
    g = np.load(os.path.join(HERE, 'golden', 'jpeg_cases.npz'))
    cmyk = with_exif(g['refused_cmyk'].tobytes(), 6)
    stand_in = np.arange(16 * 24 * 3, dtype=np.uint8).reshape(16, 24, 3)
    monkeypatch.setattr(J, '_pil_rgb', lambda data: stand_in.copy())
    d = stream(37, 53, '420')
    plain = decode_jpeg(d, DEV).cpu().numpy()
    packed, shapes = decode_jpeg_batch([with_exif(d, 8), cmyk, d], DEV, fallback=True, orient=True)
    assert shapes == [(53, 37), (24, 16), (37, 53)]
    for got, want in zip(_split(packed, shapes), [turned(plain, 8), turned(stand_in, 6), plain]):
        assert np.array_equal(got, want)
    packed, shapes = decode_jpeg_batch([with_exif(d, 8), cmyk, d], DEV, fallback=True)
    assert shapes == [(37, 53), (16, 24), (37, 53)] and np.array_equal(_split(packed, shapes)[1], stand_in)
