"""CPU: the host half of the PNG path (db_text_minimal_amd.png: png_info, inflate_png) and the numpy restatement the GPU tests
compare with (tests/png_ref.py), against the golden cases (Pillow's decode, tests/golden/png_cases.npz): the reference
reproduces the golden pixels; descriptors and blob bytes of inflate_png equal the reference's; every corrupt or refused fixture
raises its class with its index; the reference's writer decodes under Pillow; the inflate bound; the entry points refuse
inconsistent descriptors before anything is launched."""
import io
import json
import os
import struct
import zlib

import numpy as np
import pytest

import png_ref
from db_text_minimal_amd import CorruptPng, PngError, UnsupportedPng, inflate_png, png_info
from db_text_minimal_amd import png as P
from db_text_minimal_amd._lib import lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'png_cases.npz')
BAD = {'refused_cgbi': UnsupportedPng, 'corrupt_crc': CorruptPng, 'corrupt_truncated_idat': CorruptPng, 'corrupt_filter5': CorruptPng,
       'corrupt_zero_width': CorruptPng, 'corrupt_depth3': CorruptPng, 'corrupt_no_iend': CorruptPng}


@pytest.fixture(scope='module')
def golden():
    g = np.load(GOLDEN)
    names = json.loads(str(g['names']))
    return names, [g['png_%d' % i].tobytes() for i in range(len(names))], [g['rgb_%d' % i] for i in range(len(names))], g


def test_golden_holds_the_cases_the_kernels_can_go_wrong_at(golden):
    names = golden[0]
    assert len(names) == len(set(names)) == 90
    for ct, d in ((0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16), (6, 8), (6, 16)):
        assert 'pair_ct%d_d%d_17x33' % (ct, d) in names
    for n in ['band_5x2100_f%d' % t for t in range(5)] + ['band_5x2100_cycle', 'chunk_2100x9', 'short_plte', 'idat_byte_chunks', 'pal2_trns']:
        assert n in names
    assert set(BAD) <= set(golden[3].files)


def test_reference_reproduces_the_golden_pixels(golden):
    for n, d, want in zip(*golden[:3]):
        got = png_ref.decode(d)
        assert got.shape == want.shape and np.array_equal(got, want), n


def test_png_info_against_the_reference(golden):
    for n, d, want in zip(*golden[:3]):
        p, info = png_ref.parse(d), png_info(d)
        assert (info['width'], info['height'], info['bit_depth'], info['colour_type'], info['interlace']) == (
            p['width'], p['height'], p['depth'], p['ctype'], bool(p['interlace'])), n
        assert info['channels'] == png_ref.CHANNELS[p['ctype']] and info['supported'] and info['status'] == 0 and info['reason'] is None
        assert (info['height'], info['width']) == want.shape[:2]
    bad = png_info(golden[3]['refused_cgbi'].tobytes())
    assert not bad['supported'] and 'CgBI' in bad['reason']
    assert not png_info(b'\xff\xd8\xff\xe0 not a png')['supported']
    assert not png_info(golden[3]['corrupt_depth3'].tobytes())['supported']


def test_inflate_png_descriptors_and_blob_against_the_reference(golden):
    names, datas, rgbs, _ = golden
    obj = inflate_png(datas, pin=False)
    assert len(obj) == len(datas) and not obj.status.any() and obj.errors() == [None] * len(datas)
    assert obj.shapes == [r.shape[:2] for r in rgbs]
    assert obj.blob.numel() >= obj.blob_len + 32 and not obj.blob.is_pinned()
    blob = obj.blob.numpy()
    o = out = nsub = 0
    for i, (n, d) in enumerate(zip(names, datas)):
        p, raw = png_ref.scanlines(d)
        row = obj.desc[i]
        assert tuple(row[:5]) == (p['width'], p['height'], p['depth'], p['ctype'], p['interlace']), n
        assert row[5] == out and row[6] == len(p['palette']) and row[7] == 0
        assert np.array_equal(obj.palettes[i, :len(p['palette'])], p['palette']) and not obj.palettes[i, len(p['palette']):].any()
        assert np.array_equal(blob[o:o + raw.size], raw), n
        slots = [s for k, s in obj.subs if k == i]
        assert len(slots) == len(png_ref.passes(p)) and (slots == [0] if not p['interlace'] else min(slots) >= 1 and slots == sorted(slots))
        q = o
        for s, (_, _, _, _, pw, ph) in zip(slots, png_ref.passes(p)):
            assert row[8 + s] == q and row[16 + s] % 16 == 0
            q += ph * (1 + png_ref.row_bytes(p, pw))
        o, out, nsub = o + raw.size, out + p['width'] * p['height'] * 3, nsub + len(slots)
    assert o == obj.blob_len and nsub == len(obj.subs)
    one = inflate_png(datas[:3], threads=1, pin=False)
    assert np.array_equal(one.blob.numpy()[:one.blob_len], blob[:one.blob_len]) and np.array_equal(one.desc, obj.desc[:3])


@pytest.mark.parametrize('kind', sorted(BAD))
def test_bad_files_raise_their_class_with_their_index(golden, kind):
    names, datas, _, g = golden
    bad = g[kind].tobytes()
    obj = inflate_png([datas[0], datas[20], bad, datas[3]], pin=False)
    errs = obj.errors()
    assert [e is None for e in errs] == [True, True, False, True]
    assert type(errs[2]) is BAD[kind] and isinstance(errs[2], PngError) and isinstance(errs[2], ValueError)
    assert errs[2].index == 2 and 'image 2' in str(errs[2]) and errs[2].code == int(obj.status[2]) != 0
    assert obj.shapes[2] == (0, 0) and obj.shapes[3] == (int(obj.desc[3][1]), int(obj.desc[3][0]))
    alone = inflate_png([datas[0], datas[20], datas[3]], pin=False)  # the failed member takes no bytes anywhere
    assert obj.blob_len == alone.blob_len and np.array_equal(obj.blob.numpy()[:obj.blob_len], alone.blob.numpy()[:alone.blob_len])
    assert obj.raw_bytes == alone.raw_bytes and obj.desc[3][5] == alone.desc[2][5]
    with pytest.raises(BAD[kind], match='image 0'):  # png_collate raises what the batch reports
        P.png_collate([(bad, [], [])])


def test_surplus_scanline_bytes_are_ignored_and_missing_ones_are_not(golden):
    x = np.arange(5 * 4 * 3, dtype=np.uint8).reshape(5, 4, 3)
    rows = png_ref.filter_rows(x, 1).tobytes()
    ihdr = png_ref.chunk(b'IHDR', struct.pack('>IIBBBBB', 4, 5, 8, 2, 0, 0, 0))
    good = inflate_png([png_ref.SIGNATURE + ihdr + png_ref.chunk(b'IDAT', zlib.compress(rows + b'\x07' * 40)) + png_ref.chunk(b'IEND', b'')], pin=False)
    assert good.status[0] == 0 and good.blob_len == len(rows) and bytes(good.blob.numpy()[:len(rows)]) == rows
    short = inflate_png([png_ref.SIGNATURE + ihdr + png_ref.chunk(b'IDAT', zlib.compress(rows[:-1])) + png_ref.chunk(b'IEND', b'')], pin=False)
    assert isinstance(short.errors()[0], CorruptPng) and 'fewer' in str(short.errors()[0])


def test_inflate_is_bounded_by_what_ihdr_implies(monkeypatch):
    """a 2 x 2 grey image whose stream inflates to 64 MiB: no call asks zlib for more than the 6 bytes IHDR implies"""
    bomb = zlib.compress(b'\x00' * (64 << 20), 9)
    cut = [bomb[:len(bomb) // 2], bomb[len(bomb) // 2:]]
    data = (png_ref.SIGNATURE + png_ref.chunk(b'IHDR', struct.pack('>IIBBBBB', 2, 2, 8, 0, 0, 0, 0)) + png_ref.chunk(b'IDAT', cut[0])
            + png_ref.chunk(b'IDAT', cut[1]) + png_ref.chunk(b'IEND', b''))
    asked, produced = [], []
    real = zlib.decompressobj

    class Watched:
        def __init__(self):
            self.z = real()

        def decompress(self, data, max_length=0):
            asked.append(max_length)
            out = self.z.decompress(data, max_length)
            produced.append(len(out))
            return out

        def __getattr__(self, name):
            return getattr(self.z, name)

    monkeypatch.setattr(P.zlib, 'decompressobj', Watched)
    obj = inflate_png([data], pin=False)
    assert obj.status[0] == 0 and obj.blob_len == 6 and obj.blob.numel() == 6 + 32
    assert asked and all(0 < a <= 6 for a in asked) and sum(produced) == 6


@pytest.mark.parametrize('shape', [(1, 1), (7, 1), (1, 7), (17, 33), (75, 100)])  # (H, W): 1x1, 1x7, 7x1, 33x17 and 100x75 as W x H
@pytest.mark.parametrize('grey', [False, True])
def test_reference_writer_decodes_under_pillow(shape, grey):
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.RandomState(shape[0] * 131 + shape[1] + grey)
    y, x = np.mgrid[:shape[0], :shape[1]]
    base = (3 * x + 2 * y)[..., None] + np.array([0, 60, 130])
    img = ((base + rng.randint(-6, 7, size=base.shape)) & 255).astype(np.uint8)
    img = np.ascontiguousarray(img[..., 0]) if grey else img
    for f in ('adaptive', 0, 1, 2, 3, 4):
        data = png_ref.encode(img, 6, f)
        im = Image.open(io.BytesIO(data))
        assert im.mode == ('L' if grey else 'RGB') and np.array_equal(np.asarray(im), img), f
        assert np.array_equal(png_ref.decode(data), img[..., None].repeat(3, 2) if grey else img)
        if f != 'adaptive':
            assert (png_ref.filter_rows(img, f)[:, 0] == f).all()
    p = png_ref.parse(png_ref.encode(img))
    assert (p['depth'], p['ctype'], p['interlace']) == (8, 0 if grey else 2, 0)


def test_adaptive_choice_takes_the_lowest_type_of_equal_scores():
    assert (png_ref.filter_rows(np.zeros((4, 9, 3), np.uint8))[:, 0] == 0).all()
    flat = np.full((3, 8), 200, np.uint8)  # None scores 8 x 56; Sub leaves one byte (score 56), Up the first row: row 0 takes Sub, the others Up
    assert list(png_ref.filter_rows(flat)[:, 0]) == [1, 2, 2]


def _arrays(obj):
    hdesc, hsubs = np.ascontiguousarray(obj.desc, np.int64).copy(), np.ascontiguousarray(obj.subs, np.int32).copy()
    out = sum(h * w * 3 for h, w in obj.shapes)
    return hdesc, hsubs, out


def test_entry_points_refuse_inconsistent_descriptors(golden):
    """every value a kernel bounds a loop with is checked on the host first: a descriptor that disagrees with the buffer
    lengths is refused (1: invalid argument) by dbn_png_check and, before any launch, by the device entry points"""
    names, datas, _, _ = golden
    pick = [names.index(n) for n in ('pair_ct2_d8_17x33', 'adam7_rgba16_13x10', 'pair_ct3_d4_17x33')]
    obj = inflate_png([datas[i] for i in pick], pin=False)
    L = lib()
    hdesc, hsubs, out = _arrays(obj)

    def rc(d=hdesc, s=hsubs, blob_len=obj.blob_len, raw_bytes=obj.raw_bytes, out_bytes=out):
        return L.dbn_png_check(d.ctypes.data, len(obj), s.ctypes.data, len(s), blob_len, raw_bytes, out_bytes)

    assert rc() == 0
    assert rc(blob_len=obj.blob_len - 1) == 1 and rc(raw_bytes=obj.raw_bytes - 1) == 1 and rc(out_bytes=out - 3) == 1 and rc(out_bytes=out + 3) == 1
    for field, value in ((0, 18), (0, 0), (0, 65536), (1, 34), (2, 16), (2, 3), (3, 5), (4, 2), (5, 3), (6, 257), (8, obj.blob_len), (8, -1),
                         (16, 8), (16, obj.raw_bytes)):
        d = hdesc.copy()
        d[0, field] = value
        assert rc(d=d) == 1, (field, value)
    d = hdesc.copy()
    d[1, 0] = 4000  # the interlaced member claims rows the blob does not hold
    assert rc(d=d) == 1
    for bad in ((3, 0), (-1, 0), (0, 1), (1, 0), (1, 8)):
        s = hsubs.copy()
        s[0] = bad
        assert rc(s=s) == 1, bad
    small = inflate_png([png_ref.encode(np.zeros((1, 1), np.uint8))], pin=False)  # an empty Adam7 pass has no workgroup
    d, s, o = _arrays(small)
    d[0, 4], s[0, 1] = 1, 2
    assert L.dbn_png_check(d.ctypes.data, 1, s.ctypes.data, 1, small.blob_len, small.raw_bytes, o) == 1
    # the device entry points make the same checks before they launch anything: no GPU is touched here
    d = hdesc.copy()
    d[0, 1] = 34
    fake = hdesc.ctypes.data  # stands for device memory that is never read
    assert L.dbn_png_unfilter(fake, obj.blob_len, obj.blob_len + 32, d.ctypes.data, fake, len(obj), hsubs.ctypes.data, fake, len(hsubs), fake,
                              obj.raw_bytes, out, None) == 1
    assert L.dbn_png_unfilter(fake, obj.blob_len, obj.blob_len + 31, hdesc.ctypes.data, fake, len(obj), hsubs.ctypes.data, fake, len(hsubs), fake,
                              obj.raw_bytes, out, None) == 1
    assert L.dbn_png_pixels(fake, obj.raw_bytes, d.ctypes.data, fake, fake, len(obj), obj.blob_len, fake, out, None) == 1
    e = np.array([[0, 5, 4, 3, 0, 0, 0, 0]], np.int64)
    for in_bytes, out_bytes, filt, row in ((59, 65, -1, e[0]), (60, 64, -1, e[0]), (60, 65, 5, e[0]), (60, 65, -2, e[0]), (60, 65, 0, [0, 5, 4, 2, 0, 0, 0, 0]),
                                           (60, 65, 0, [0, 5, 4, 3, 0, 1, 0, 0]), (60, 65, 0, [0, 0, 4, 3, 0, 0, 0, 0]), (60, 65, 0, [1, 5, 4, 3, 0, 0, 0, 0])):
        h = np.array([row], np.int64)
        assert L.dbn_png_filter_rows(fake, in_bytes, h.ctypes.data, fake, 1, filt, fake, out_bytes, None) == 1, (in_bytes, out_bytes, filt, row)


def test_package_arguments_are_checked():
    with pytest.raises(ValueError):
        inflate_png([])
    with pytest.raises(ValueError, match='adaptive'):
        P._filter_arg('paeth')
    with pytest.raises(ValueError, match='adaptive'):
        P._filter_arg(5)
    assert [P._filter_arg(f) for f in ('adaptive', 0, 4)] == [-1, 0, 4]
    with pytest.raises(ValueError, match="errors is"):
        P.decode_png_batch([b''], errors='ignore')
