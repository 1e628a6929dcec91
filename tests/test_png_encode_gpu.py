"""GPU (-m gpu): the PNG encoder (csrc/png.hip png_filter_kernel through db_text_minimal_amd.png): filter_png_rows equals the
numpy restatement's filtered bytes exactly (tests/png_ref.py: the same type for every row, 'adaptive' and each fixed type),
encode_png gives the restatement's file byte for byte, every input layout round-trips through decode_png_batch, save_pngs
writes files decode_png reads back, and the renderer's reader and writer take a .png suffix without PIL."""
import numpy as np
import pytest
import torch

import png_ref
from db_text_minimal_amd import decode_png, decode_png_batch, encode_png, encode_png_batch, filter_png_rows, save_pngs
from gpu_util import DEV

pytestmark = pytest.mark.gpu

SIZES = ((1, 1), (1, 7), (7, 1), (33, 17), (100, 75), (257, 6), (5, 600))  # W x H
FILTERS = ('adaptive', 0, 1, 2, 3, 4)


def _image(w, h, grey, seed=0):
    """a ramp with +-6 noise (photo-like: the adaptive choice varies over the rows); small ones are plain noise"""
    rng = np.random.RandomState(w * 1009 + h * 7 + grey + seed)
    if w * h <= 49:
        img = rng.randint(0, 256, size=(h, w, 3))
    else:
        y, x = np.mgrid[:h, :w]
        img = (3 * x + 2 * y)[..., None] + np.array([0, 60, 130]) + rng.randint(-6, 7, size=(h, w, 3))
        img[h // 3:h // 3 + 2] = rng.randint(0, 256, size=img[h // 3:h // 3 + 2].shape)  # rows where None or Sub wins
        img[:, w // 2:] = img[:1, w // 2:]  # columns that repeat down the image: Up wins
    img = (img & 255).astype(np.uint8)
    return np.ascontiguousarray(img[..., 0]) if grey else img


@pytest.fixture(scope='module')
def images():
    out = [_image(w, h, grey) for w, h in SIZES for grey in (False, True)]
    return out + [np.zeros((9, 17, 3), np.uint8), np.zeros((9, 17), np.uint8)]  # all zero: every score ties, type 0 wins


@pytest.mark.parametrize('filter', FILTERS)
def test_filter_png_rows_equals_the_reference_exactly(images, filter):
    got = filter_png_rows(images, filter=filter, device=DEV)
    assert len(got) == len(images)
    for img, rows in zip(images, got):
        want = png_ref.filter_rows(img, filter)
        assert rows.dtype == np.uint8 and rows.shape == want.shape
        assert np.array_equal(rows[:, 0], want[:, 0]), 'filter types of %s: %s, not %s' % (img.shape, rows[:, 0], want[:, 0])
        assert np.array_equal(rows, want), img.shape
    if filter == 'adaptive':
        used = set(np.concatenate([r[:, 0] for r in got]).tolist())
        assert used == {0, 1, 2, 3, 4}, used  # the images make every type win somewhere
        assert not got[-1][:, 0].any() and not got[-2][:, 0].any()


def test_encode_png_equals_the_reference_file(images):
    for img in images:
        for f, level in (('adaptive', 6), (4, 9), (0, 0), (3, 1)):
            assert encode_png(torch.from_numpy(img).to(DEV), level, f) == png_ref.encode(img, level, f), (img.shape, f, level)
    datas = encode_png_batch(images, device=DEV)
    assert datas == [png_ref.encode(img) for img in images]
    p = png_ref.parse(datas[0])
    assert (p['depth'], p['ctype'], p['interlace']) == (8, 2, 0) and datas[0].count(b'IDAT') == 1 and datas[0][12:16] == b'IHDR'
    with pytest.raises(ValueError, match='compress_level'):
        encode_png_batch(images, compress_level=10, device=DEV)
    with pytest.raises(ValueError, match='adaptive'):
        encode_png_batch(images, filter='sub', device=DEV)
    with pytest.raises(ValueError, match=r'\[H, W\]'):
        encode_png_batch(np.zeros((2, 3, 4, 5), np.uint8), device=DEV)
    with pytest.raises(ValueError, match='uint8'):
        encode_png_batch(np.zeros((4, 5, 3), np.float32), device=DEV)


def _decoded(datas):
    packed, shapes = decode_png_batch(datas, DEV)
    flat, out, o = packed.cpu().numpy(), [], 0
    for h, w in shapes:
        out.append(flat[o:o + h * w * 3].reshape(h, w, 3))
        o += h * w * 3
    return out


def test_every_input_layout_round_trips(images):
    rgb = [im for im in images if im.ndim == 3]
    packed = torch.from_numpy(np.concatenate([im.reshape(-1) for im in rgb])).to(DEV)
    shapes = [im.shape[:2] for im in rgb]
    for got, want in zip(_decoded(encode_png_batch(packed, shapes)), rgb):  # packed + shapes, on the device
        assert np.array_equal(got, want)
    one = _image(33, 17, False, 1)
    assert np.array_equal(_decoded(encode_png_batch(one, device=DEV))[0], one)  # [H, W, 3], a host array
    stack = np.stack([_image(100, 32, False, s) for s in range(5)])  # crop_words' [N, 32, 100, 3]
    for got, want in zip(_decoded(encode_png_batch(torch.from_numpy(stack).to(DEV), filter=4)), stack):
        assert np.array_equal(got, want)
    grey = _image(33, 17, True, 2)
    assert np.array_equal(_decoded(encode_png_batch(grey, device=DEV))[0], grey[..., None].repeat(3, 2))  # [H, W]
    gstack = np.stack([_image(21, 12, True, s) for s in range(3)])  # [N, H, W]
    for got, want in zip(_decoded(encode_png_batch(torch.from_numpy(gstack).to(DEV), compress_level=1)), gstack):
        assert np.array_equal(got, want[..., None].repeat(3, 2))
    mixed = [torch.from_numpy(images[0]).to(DEV), images[1], images[4]]  # a list of both kinds, on both sides
    for got, want in zip(_decoded(encode_png_batch(mixed, device=DEV)), mixed):
        want = want.cpu().numpy() if torch.is_tensor(want) else want
        assert np.array_equal(got, want if want.ndim == 3 else want[..., None].repeat(3, 2))


def test_save_pngs_writes_files_decode_png_reads_back(tmp_path):
    stack = torch.from_numpy(np.stack([_image(100, 32, False, s) for s in range(3)])).to(DEV)
    paths = save_pngs([tmp_path / ('word_%d.png' % i) for i in range(3)], stack)
    assert paths == [str(tmp_path / ('word_%d.png' % i)) for i in range(3)]
    for p, want in zip(paths, stack):
        with open(p, 'rb') as f:
            assert torch.equal(decode_png(f.read(), DEV), want)
    with pytest.raises(ValueError, match='paths'):
        save_pngs([tmp_path / 'a.png'], stack)


def test_renderer_reads_and_writes_png_without_pil(tmp_path, monkeypatch):
    """python -m db_text_minimal_amd.render's reader and writer take a .png suffix through this module: with PIL made
    unimportable the file is written, holds the image, and reads back as the device tensor"""
    import sys

    from db_text_minimal_amd import render as R
    monkeypatch.setitem(sys.modules, 'PIL', None)
    monkeypatch.setitem(sys.modules, 'PIL.Image', None)
    img = torch.from_numpy(_image(100, 75, False, 3)).to(DEV)
    path = str(tmp_path / 'result.PNG')
    R._write_image(path, img)
    with open(path, 'rb') as f:
        assert f.read() == png_ref.encode(img.cpu().numpy())
    back = R._read_image(path)
    assert torch.is_tensor(back) and back.is_cuda and torch.equal(back, img)
