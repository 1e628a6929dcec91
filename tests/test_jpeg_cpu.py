"""CPU (-m "not gpu"): the host half of the JPEG decode (csrc/jpeg.hip dbn_jpeg_info / dbn_jpeg_entropy_batch through
db_text_minimal_amd.jpeg) and the numpy restatement tests/jpeg_ref.py: the restatement against the golden pixels (Pillow's) and
against fresh Pillow decodes, the library's coefficients and tables against the restatement, jpeg_info, every refused kind,
and a fuzz of truncations and corruptions with a guard around the coefficient buffer."""
import ctypes
import io
import json
import mmap
import os

import numpy as np
import pytest
import torch

from db_text_minimal_amd import CorruptJpeg, JpegError, UnsupportedJpeg, entropy_decode, jpeg_info
from db_text_minimal_amd import jpeg as J
from db_text_minimal_amd._lib import lib
import jpeg_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jpeg_cases.npz')


def golden():
    g = np.load(GOLDEN)
    names = json.loads(str(g['names']))
    return names, [g['jpeg_%d' % i].tobytes() for i in range(len(names))], [g['rgb_%d' % i] for i in range(len(names))], g


def _pil():
    try:
        from PIL import Image, features
        if not features.check('jpg'):
            return None
        return Image
    except ImportError:
        return None


def _ref_coefs(data):
    h, co = R.entropy_decode(data)
    return h, np.concatenate([c.reshape(-1) for c in co])


# ---- stream surgery --------------------------------------------------------------------------------------------------
def segments(data):
    """[(marker, start of the FF, end)] of the header segments up to and including SOS"""
    out, p = [], 2
    while True:
        assert data[p] == 0xFF
        m = data[p + 1]
        L = data[p + 2] << 8 | data[p + 3]
        out.append((m, p, p + 2 + L))
        p += 2 + L
        if m == 0xDA:
            return out


def patch_sof(data, marker=None, precision=None, sampling=None):
    data = bytearray(data)
    for m, a, _ in segments(bytes(data)):
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            if marker is not None:
                data[a + 1] = marker
            if precision is not None:
                data[a + 4] = precision
            if sampling is not None:
                data[a + 11] = sampling
    return bytes(data)


def drop_segment(data, marker):
    for m, a, b in segments(data):
        if m == marker:
            return data[:a] + data[b:]
    raise AssertionError('no such segment')


def widen_dqt(data):
    """rewrite every 8-bit DQT table as a 16-bit one"""
    out, last = b'', 0
    for m, a, b in segments(data):
        if m == 0xDB:
            seg, q, body = data[a + 4:b], 0, b''
            while q < len(seg):
                assert seg[q] >> 4 == 0
                body += bytes([0x10 | seg[q]]) + b''.join(bytes([0, v]) for v in seg[q + 1:q + 65])
                q += 65
            out += data[last:a] + b'\xff\xdb' + (len(body) + 2).to_bytes(2, 'big') + body
            last = b
    return out + data[last:]


def one_component_scan(data):
    """the SOS of a 3-component file rewritten to name its first component only (a non-interleaved scan)"""
    for m, a, b in segments(data):
        if m == 0xDA:
            seg = data[a + 4:b]
            body = bytes([1]) + seg[1:3] + seg[-3:]
            return data[:a] + b'\xff\xda' + (len(body) + 2).to_bytes(2, 'big') + body + data[b:]


def with_exif(data, orientation, order='II'):
    e = 'little' if order == 'II' else 'big'
    tiff = order.encode() + (42).to_bytes(2, e) + (8).to_bytes(4, e) + (1).to_bytes(2, e) + (0x0112).to_bytes(2, e) + (3).to_bytes(2, e) + \
        (1).to_bytes(4, e) + orientation.to_bytes(2, e) + b'\0\0' + (0).to_bytes(4, e)
    body = b'Exif\0\0' + tiff
    return data[:2] + b'\xff\xe1' + (len(body) + 2).to_bytes(2, 'big') + body + data[2:]


# ---- the restatement ---------------------------------------------------------------------------------------------------
def test_golden_covers_what_it_should():
    names, datas, rgbs, g = golden()
    others = [os.path.getsize(os.path.join(os.path.dirname(GOLDEN), f)) for f in os.listdir(os.path.dirname(GOLDEN))
              if f.endswith('.npz') and f != 'jpeg_cases.npz']
    assert os.path.getsize(GOLDEN) <= max(others)  # no larger than the largest golden beside it
    for w, h in [(1, 1), (7, 5), (8, 8), (17, 33), (100, 75), (250, 131), (640, 480)]:
        assert any(n.startswith('%dx%d_' % (w, h)) for n in names), (w, h)
    for key in ['_444_', '_422_', '_420_', '_grey_', '_q30', '_q75', '_q95', '_q100', '_opt', '_qtables', '_rst_blocks', '_rst_rows', '_noise_',
                '_ramp_', '_strokes_']:
        assert any(key in n for n in names), key
    assert 'refused_progressive' in g and 'refused_cmyk' in g


def test_ref_equals_golden_pixels():
    names, datas, rgbs, _ = golden()
    for n, d, want in zip(names, datas, rgbs):
        got = R.decode(d)
        assert got.shape == want.shape and np.array_equal(got, want), n


def _random_cases(count, seed):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN)))
    from make_jpeg_golden import content, encode
    rng = np.random.default_rng(seed)
    for k in range(count):
        w, h = int(rng.integers(1, 70)), int(rng.integers(1, 70))
        sub = ['444', '422', '420', 'grey'][int(rng.integers(0, 4))]
        kind = ['noise', 'ramp', 'strokes'][int(rng.integers(0, 3))]
        kw = dict(quality=int(rng.choice([5, 30, 50, 75, 90, 95, 100])))
        if rng.random() < 0.3:
            kw['optimize'] = True
        if rng.random() < 0.3:
            kw['restart_marker_blocks'] = int(rng.integers(1, 9))
        elif rng.random() < 0.2:
            kw['restart_marker_rows'] = int(rng.integers(1, 3))
        yield '%d: %dx%d %s %s %s' % (k, w, h, sub, kind, kw), encode(content(kind, rng, w, h), sub, **kw)


def test_ref_and_library_equal_fresh_pil_decodes():
    Image = _pil()
    if Image is None:
        return  # the golden pins the same arithmetic; this adds breadth where Pillow is installed
    cases = list(_random_cases(240, 77))
    assert len(cases) >= 200
    datas = [d for _, d in cases]
    obj = entropy_decode(datas, pin=False)
    assert not obj.status.any()
    coef = obj.coef.numpy()
    for i, (name, d) in enumerate(cases):
        want = np.asarray(Image.open(io.BytesIO(d)).convert('RGB'))
        h, co = R.entropy_decode(d)
        got = R.to_rgb(h, R.planes(h, co))
        assert got.shape == want.shape and np.array_equal(got, want), name
        ref = np.concatenate([c.reshape(-1) for c in co])
        o = int(obj.desc[i, 0])
        assert np.array_equal(coef[o:o + ref.size], ref), name


# ---- the library's host half --------------------------------------------------------------------------------------------
def test_library_coefficients_tables_and_descriptors_equal_ref():
    names, datas, rgbs, _ = golden()
    extra = [patch_sof(datas[6], marker=0xC1), widen_dqt(datas[10]), drop_segment(datas[12], 0xE0), with_exif(datas[14], 6)]
    datas = datas + extra
    obj = entropy_decode(datas, pin=False)
    assert obj.status.tolist() == [0] * len(datas)
    coef, off, out = obj.coef.numpy(), 0, 0
    for i, d in enumerate(datas):
        h, ref = _ref_coefs(d)
        dsc = obj.desc[i]
        assert dsc[0] == off and dsc[0] % 64 == 0 and (dsc[1], dsc[2], dsc[3]) == (h.width, h.height, h.ncomp)
        assert dsc[4] == out and dsc[5] == 192 * i
        for c in range(h.ncomp):
            assert tuple(dsc[6 + 4 * c:10 + 4 * c]) == (h.grid[c][1], h.grid[c][0]) + tuple(h.samp[c])
            assert np.array_equal(obj.qtabs[i, c], h.qtabs[c].astype(np.uint16))
        assert tuple(dsc[18:24]) == (h.hmax, h.vmax, h.mcux, h.mcuy, 0, h.ri)
        assert np.array_equal(coef[off:off + ref.size], ref), i
        off += ref.size
        out += h.width * h.height * 3
    assert off == coef.size
    assert obj.shapes[:len(rgbs)] == [r.shape[:2] for r in rgbs]
    # the rewritten streams decode to the pixels of their originals
    for e, k in zip(extra, (6, 10, 12, 14)):
        assert np.array_equal(R.decode(e), rgbs[k])


def test_jpeg_info_fields():
    names, datas, rgbs, _ = golden()
    for n, d, rgb in zip(names, datas, rgbs):
        info = jpeg_info(d)
        h = R.parse(d)
        assert info['supported'] and info['status'] == 0 and info['reason'] is None
        assert (info['height'], info['width']) == rgb.shape[:2] and info['components'] == h.ncomp
        assert info['sampling'] == [(c[1], c[2]) for c in h.comps] and info['restart_interval'] == h.ri
        assert info['process'] == 'baseline' and info['precision'] == 8 and info['jfif'] and info['adobe_transform'] is None
        assert info['orientation'] == 0 and info['coefficients'] == sum(a * b * 64 for a, b in h.grid)
        sub = n.split('_')[1]
        assert info['sampling'][0] == {'444': (1, 1), '422': (2, 1), '420': (2, 2), 'grey': (1, 1)}[sub]
        assert (info['restart_interval'] > 0) == ('_rst_' in n)
    for o in range(1, 9):
        assert jpeg_info(with_exif(datas[4], o, 'II'))['orientation'] == o
        assert jpeg_info(with_exif(datas[4], o, 'MM'))['orientation'] == o
    assert jpeg_info(patch_sof(datas[4], marker=0xC1))['process'] == 'extended'
    assert not jpeg_info(drop_segment(datas[4], 0xE0))['jfif']
    assert jpeg_info(np.frombuffer(datas[4], np.uint8))['width'] == rgbs[4].shape[1]


def refused_streams():
    names, datas, rgbs, g = golden()
    base = datas[names.index('100x75_420_ramp_q75_opt')]
    return [
        ('progressive', g['refused_progressive'].tobytes(), 3, 'progressive'),
        ('cmyk', g['refused_cmyk'].tobytes(), 7, '4-component'),
        ('arithmetic', patch_sof(base, marker=0xC9), 4, 'arithmetic'),
        ('lossless', patch_sof(base, marker=0xC3), 5, 'lossless'),
        ('12-bit', patch_sof(base, marker=0xC1, precision=12), 6, '12-bit'),
        ('sampling 1x2', patch_sof(base, sampling=0x12), 8, 'sampling'),
        ('sampling 4x1', patch_sof(base, sampling=0x41), 8, 'sampling'),
        ('multi-scan', one_component_scan(base), 9, 'multi-scan'),
    ]


def test_every_refused_kind_raises_with_its_reason():
    for name, data, code, word in refused_streams():
        info = jpeg_info(data)
        assert not info['supported'] and info['status'] == code and word in info['reason'], name
        obj = entropy_decode([data], pin=False)
        assert obj.status.tolist() == [code] and obj.shapes == [(0, 0)] and obj.coef.numel() == 0, name
        err = obj.errors()[0]
        assert isinstance(err, UnsupportedJpeg) and isinstance(err, JpegError) and err.code == code and word in str(err), name
        with pytest.raises(R.JpegError) as ei:
            R.parse(data)
        assert ei.value.code == code, name
        with pytest.raises(UnsupportedJpeg, match=word):
            J.jpeg_collate([(data, [], [])])
    # an Adobe marker that declares RGB (transform 0) on three components
    names, datas, _, _ = golden()
    adobe = b'Adobe' + bytes([0, 100, 0, 0, 0, 0, 0])
    rgb3 = datas[8][:2] + b'\xff\xee' + (len(adobe) + 2).to_bytes(2, 'big') + adobe + datas[8][2:]
    assert jpeg_info(rgb3)['status'] == 7 and jpeg_info(rgb3)['adobe_transform'] == 0
    for junk, code in ((b'', 1), (b'\x89PNG\r\n\x1a\n' + bytes(40), 1), (datas[8][:30], 2)):
        e = entropy_decode([junk], pin=False).errors()[0]
        assert isinstance(e, CorruptJpeg) and e.code == code


def test_refused_kinds_have_the_codes_of_the_restatement():
    assert J.REASONS == R.REASONS


def test_one_bad_stream_fails_alone():
    names, datas, rgbs, _ = golden()
    bad = bytearray(datas[20])
    cut = bytes(bad[:len(bad) // 2])
    batch = [datas[3], cut, datas[20], refused_streams()[0][1], datas[7]]
    obj = entropy_decode(batch, pin=False)
    assert obj.status.tolist()[0] == 0 and obj.status[1] != 0 and obj.status.tolist()[2:] == [0, 3, 0]
    assert obj.shapes[1] == (0, 0) and obj.shapes[3] == (0, 0)
    coef = obj.coef.numpy()
    for i in (0, 2, 4):
        _, ref = _ref_coefs(batch[i])
        o = int(obj.desc[i, 0])
        assert np.array_equal(coef[o:o + ref.size], ref)
    # the failed image's slice is zeroed, not half written
    o, n = int(obj.desc[1, 0]), int(obj.desc[2, 0]) - int(obj.desc[1, 0])
    assert n > 0 and not coef[o:o + n].any()


def test_thread_counts_give_identical_buffers():
    names, datas, _, _ = golden()
    a = entropy_decode(datas, threads=1, pin=False)
    for t in (16, 64, 3):  # 64 is capped at 16 inside
        b = entropy_decode(datas, threads=t, pin=False)
        assert torch.equal(a.coef, b.coef) and np.array_equal(a.desc, b.desc) and np.array_equal(a.qtabs, b.qtabs)
        assert np.array_equal(a.status, b.status)


# ---- fuzz ----------------------------------------------------------------------------------------------------------------
GUARD = 4096
_LIBC = ctypes.CDLL(None, use_errno=True)


class Fenced:
    """bytes placed so that their last byte is the last byte of a page, with an unreadable page behind it: a read past the end
    of the stream ends the process instead of going unseen"""

    def __init__(self, data):
        page = mmap.PAGESIZE
        size = -(-max(len(data), 1) // page) * page + page
        self.map = mmap.mmap(-1, size)
        self.anchor = ctypes.c_char.from_buffer(self.map)
        base = ctypes.addressof(self.anchor)
        assert _LIBC.mprotect(ctypes.c_void_p(base + size - page), ctypes.c_size_t(page), 0) == 0, ctypes.get_errno()
        start = size - page - len(data)
        self.map[start:start + len(data)] = data
        self.ptr, self.len = base + start, len(data)


def _fenced_status(data):
    """dbn_jpeg_info, dbn_jpeg_coef_elems and dbn_jpeg_entropy_batch of ONE stream that ends at an unreadable page -> status"""
    L = lib()
    f = Fenced(data)
    info = np.zeros(24, np.int64)
    assert L.dbn_jpeg_info(f.ptr, f.len, info.ctypes.data) == 0
    offs = np.array([0, f.len], np.int64)
    per = np.zeros(1, np.int64)
    total = int(L.dbn_jpeg_coef_elems(f.ptr, offs.ctypes.data, 1, per.ctypes.data))
    assert total == per[0] == info[15]
    buf = np.full(total + 2 * GUARD, 0x5A5A, np.int16)
    desc, qt, st = np.zeros((1, 24), np.int64), np.zeros((1, 3, 64), np.uint16), np.full(1, -1, np.int32)
    assert L.dbn_jpeg_entropy_batch(f.ptr, offs.ctypes.data, 1, buf[GUARD:].ctypes.data, total, desc.ctypes.data, qt.ctypes.data,
                                    st.ctypes.data, 1) == 0
    assert (buf[:GUARD] == 0x5A5A).all() and (buf[GUARD + total:] == 0x5A5A).all(), 'a decode wrote outside the coefficient buffer'
    assert (info[0] == 0) == (total > 0) and (st[0] == 0) <= (info[0] == 0)
    return int(st[0])


def _guarded_decode(streams, threads=4):
    """dbn_jpeg_entropy_batch straight through ctypes on a coefficient buffer with guard regions, the batch ending at an
    unreadable page; then every stream once more on its own, each ending at an unreadable page, with the same status.
    -> (status list, coefficients, descriptors)"""
    L = lib()
    N = len(streams)
    offs = np.zeros(N + 1, np.int64)
    offs[1:] = np.cumsum([len(s) for s in streams])
    f = Fenced(b''.join(streams))
    per = np.zeros(N, np.int64)
    total = int(L.dbn_jpeg_coef_elems(f.ptr, offs.ctypes.data, N, per.ctypes.data))
    assert total == per.sum() and total >= 0
    buf = np.full(total + 2 * GUARD, 0x5A5A, np.int16)
    desc, qt, st = np.zeros((N, 24), np.int64), np.zeros((N, 3, 64), np.uint16), np.full(N, -1, np.int32)
    rc = L.dbn_jpeg_entropy_batch(f.ptr, offs.ctypes.data, N, buf[GUARD:].ctypes.data, total, desc.ctypes.data, qt.ctypes.data,
                                  st.ctypes.data, threads)
    assert rc == 0
    assert (buf[:GUARD] == 0x5A5A).all() and (buf[GUARD + total:] == 0x5A5A).all(), 'a decode wrote outside the coefficient buffer'
    assert ((st >= 0) & (st <= 13)).all()
    for n in range(N):  # each image owns [desc[n, 0], desc[n, 0] + per[n]); a failed one left zeros there
        if st[n] != 0 and per[n]:
            o = GUARD + int(desc[n, 0])
            assert not buf[o:o + per[n]].any()
        assert _fenced_status(streams[n]) == st[n]
    return st.tolist(), buf[GUARD:GUARD + total], desc


def test_fuzz_truncations_and_corruptions_never_crash_or_write_outside():
    names, datas, _, _ = golden()
    n_trunc = n_corrupt = n_ref = 0
    rng = np.random.default_rng(4242)
    for d in datas:
        stride = max(1, len(d) // 97)
        cuts = [d[:k] for k in range(0, len(d), stride)]
        st, _, _ = _guarded_decode(cuts)
        assert st[0] == 1  # the empty stream
        n_trunc += len(cuts)
        # a stream cut inside its entropy data is never reported as decoded
        scan = R.parse(d).scan_start
        for c, s in zip(cuts, st):
            if scan < len(c) < len(d) - 2:
                assert s != 0, len(c)
    assert n_trunc >= 2000
    # single-byte corruptions of EVERY golden stream; each result is compared with the restatement's for the short streams,
    # and for the first few corruptions of the long ones (the restatement is a Python loop per symbol)
    for d in datas:
        batch = []
        for _ in range(52):
            c = bytearray(d)
            c[int(rng.integers(0, len(c)))] = int(rng.integers(0, 256))
            batch.append(bytes(c))
        st, coef, desc = _guarded_decode(batch)
        for i, s in enumerate(st):
            info = jpeg_info(batch[i])
            assert (s == 0) <= info['supported']  # decoded implies a supported header
            if len(d) >= 1500 and i >= 3:
                continue
            n_ref += 1
            if s == 0:  # and what was decoded is what the restatement decodes
                try:
                    _, ref = _ref_coefs(batch[i])
                except R.JpegError:
                    raise AssertionError('the library decoded a stream the restatement refuses')
                o = int(desc[i, 0])
                assert np.array_equal(coef[o:o + ref.size], ref)
            else:
                with pytest.raises(R.JpegError) as ei:
                    R.entropy_decode(batch[i])
                assert ei.value.code == s
        n_corrupt += len(batch)
    assert n_corrupt >= 2000 and n_ref >= 1000


def test_fallback_splice_bookkeeping():
    """decode_jpeg_batch(fallback=True) on the host side: PIL decodes the refused fixtures, splice_images puts them in place"""
    names, datas, rgbs, g = golden()
    a, b = rgbs[4], rgbs[9]
    packed = torch.from_numpy(np.concatenate([a.reshape(-1), b.reshape(-1)]))
    extra = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    out, shapes = J.splice_images(packed, [a.shape[:2], (0, 0), b.shape[:2], (0, 0)], {1: extra, 3: extra[:2]})
    assert shapes == [a.shape[:2], (5, 7), b.shape[:2], (2, 7)]
    assert np.array_equal(out.numpy(), np.concatenate([a.reshape(-1), extra.reshape(-1), b.reshape(-1), extra[:2].reshape(-1)]))
    with pytest.raises(ValueError):
        J.splice_images(packed, [a.shape[:2], b.shape[:2]], {0: extra})
    with pytest.raises(ValueError):
        J.splice_images(packed, [a.shape[:2], (0, 0)], {1: extra})
    Image = _pil()
    if Image is None:
        return
    for key in ('refused_progressive', 'refused_cmyk'):
        data = g[key].tobytes()
        got = J._pil_rgb(data)
        assert got.dtype == np.uint8 and got.shape == (16, 24, 3) and got.flags['C_CONTIGUOUS']
        assert np.array_equal(got, np.asarray(Image.open(io.BytesIO(data)).convert('RGB')))


def test_collate_and_pickle_round_trip():
    import pickle
    names, datas, rgbs, _ = golden()
    items = [(datas[i], [np.array([[1, 1], [5, 1], [5, 4], [1, 4]])], ['a']) for i in (16, 17, 21)]
    obj, shapes, polys, tags = J.jpeg_collate(items)
    assert shapes == [rgbs[i].shape[:2] for i in (16, 17, 21)] and len(obj) == 3
    assert polys[0][0].dtype == np.float64 and tags == [['a']] * 3
    back = pickle.loads(pickle.dumps(obj))
    assert torch.equal(back.coef, obj.coef) and np.array_equal(back.desc, obj.desc) and back.shapes == shapes
    ta, tb = J.work_tables(obj.desc, obj.status)
    assert ta.dtype == np.int32 and ta.shape[1] == 4 and len(tb) == sum(-(-h * w // J.RGB_PIXELS) for h, w in shapes)
    for n, c, first, _ in ta:
        assert 0 <= first < obj.desc[n, 6 + 4 * c] * obj.desc[n, 7 + 4 * c] and first % J.IDCT_BLOCKS == 0


class _Items(torch.utils.data.Dataset):
    def __init__(self, datas):
        self.datas = datas

    def __len__(self):
        return len(self.datas)

    def __getitem__(self, i):
        return self.datas[i], [np.array([[0, 0], [3, 0], [3, 3]])], None


def test_host_half_runs_in_a_loader_worker():
    names, datas, rgbs, _ = golden()
    pick = [4, 9, 18, 21, 30, 31]
    loader = torch.utils.data.DataLoader(_Items([datas[i] for i in pick]), batch_size=3, collate_fn=J.jpeg_collate, num_workers=1)
    batches = list(loader)
    assert len(batches) == 2
    for b, (obj, shapes, polys, tags) in enumerate(batches):
        here = entropy_decode([datas[i] for i in pick[3 * b:3 * b + 3]], pin=False)
        assert torch.equal(obj.coef, here.coef) and np.array_equal(obj.desc, here.desc) and np.array_equal(obj.qtabs, here.qtabs)
        assert shapes == [rgbs[i].shape[:2] for i in pick[3 * b:3 * b + 3]] and tags == [[None]] * 3
