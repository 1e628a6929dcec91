"""CPU (-m "not gpu"): the host half of the JPEG encode (csrc/jpeg_enc.hip dbn_jpeg_encode_bound / dbn_jpeg_encode_batch through
db_text_minimal_amd.jpeg) and the numpy restatement tests/jpeg_enc_ref.py: quant_tables and the restatement's coefficients
against the golden streams (Pillow's, tests/golden/jpeg_encode_cases.npz), lossless transcoding of every Annex K stream of both
archives, whole files against the restatement, thread counts, refusals that fail alone, a guard around a tight output
buffer, and, where Pillow imports, fresh random cases decoded by Pillow."""
import ctypes
import io
import json
import mmap
import os

import numpy as np
import pytest
import torch

from db_text_minimal_amd import JpegCoefficients, JpegEncodeError, entropy_decode, entropy_encode, jpeg_info, quant_tables
from db_text_minimal_amd import jpeg as J
from db_text_minimal_amd._lib import lib
import jpeg_enc_ref as E
import jpeg_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
_cache = {}


def golden():
    """[(case dict, image, Pillow's stream)] with the stack split into its images; loaded once"""
    if 'enc' not in _cache:
        g = np.load(os.path.join(HERE, 'golden', 'jpeg_encode_cases.npz'))
        out = []
        for i, c in enumerate(json.loads(str(g['cases']))):
            img = g['img_%d' % i]
            if img.ndim == 4:
                out += [(dict(c, name='%s[%d]' % (c['name'], m)), img[m], g['jpeg_%d_%d' % (i, m)].tobytes()) for m in range(len(img))]
            else:
                out.append((c, img, g['jpeg_%d' % i].tobytes()))
        _cache['enc'] = out
    return _cache['enc']


def decode_golden():
    """the non-optimised streams of the decoder's archive: [(name, stream)]"""
    if 'dec' not in _cache:
        g = np.load(os.path.join(HERE, 'golden', 'jpeg_cases.npz'))
        names = json.loads(str(g['names']))
        _cache['dec'] = [(n, g['jpeg_%d' % i].tobytes()) for i, n in enumerate(names) if not n.endswith('_opt')]
    return _cache['dec']


def parsed():
    """entropy_decode of every golden stream, once: a JpegCoefficients over all of them"""
    if 'obj' not in _cache:
        _cache['obj'] = entropy_decode([d for _, _, d in golden()], pin=False)
        assert not _cache['obj'].status.any()
    return _cache['obj']


def one(obj, n):
    """image n of a JpegCoefficients as a batch of its own"""
    d = obj.desc[n:n + 1].copy()
    per = int(sum(d[0, 6 + 4 * c] * d[0, 7 + 4 * c] for c in range(3))) * 64
    coef = obj.coef[int(d[0, 0]):int(d[0, 0]) + per].clone()
    d[0, 0], d[0, 5] = 0, 0
    return JpegCoefficients(coef, d, obj.qtabs[n:n + 1].copy(), obj.status[n:n + 1].copy())


def _pil():
    try:
        from PIL import Image, features
        return Image if features.check('jpg') else None
    except ImportError:
        return None


def _tables_of(case, nc):
    return E.component_tables(nc, case['quality'] if case['quality'] is not None else 75, case['qtables'])


def test_quant_tables_equal_the_golden_streams_tables():
    obj = parsed()
    for n, (c, img, _) in enumerate(golden()):
        if c['quality'] is None:
            continue
        t = quant_tables(c['quality'])
        assert t.dtype == np.uint16 and t.shape == (2, 64)
        assert np.array_equal(obj.qtabs[n, 0], t[0]), c['name']
        if img.ndim == 3:
            assert np.array_equal(obj.qtabs[n, 1], t[1]) and np.array_equal(obj.qtabs[n, 2], t[1]), c['name']
        assert np.array_equal(t, E.quant_tables(c['quality']))
    for bad in (0, 101, 7.5, True):
        with pytest.raises(ValueError):
            quant_tables(bad)


def test_restatement_coefficients_equal_the_golden_streams():
    obj = parsed()
    for n, (c, img, _) in enumerate(golden()):
        nc = 1 if img.ndim == 2 else 3
        samp, grids, coefs = E.forward(img, _tables_of(c, nc), c['sub'] if nc == 3 else '444')
        got = np.concatenate([k.reshape(-1) for k in coefs])
        d = obj.desc[n]
        assert [(int(d[7 + 4 * k]), int(d[6 + 4 * k])) for k in range(nc)] == grids, c['name']
        want = obj.coef[int(d[0]):int(d[0]) + got.size].numpy()
        assert np.array_equal(got, want), '%s: %d coefficients differ' % (c['name'], int((got != want).sum()))


def test_lossless_transcoding_of_every_annex_k_stream():
    streams = [(c['name'], d) for c, _, d in golden()] + decode_golden()
    assert len(streams) > 80
    by_ri = {}
    for name, d in streams:
        by_ri.setdefault(jpeg_info(d)['restart_interval'], []).append((name, d))
    assert len([r for r in by_ri if r]) >= 3
    for ri, group in by_ri.items():
        obj = entropy_decode([d for _, d in group], pin=False)
        assert not obj.status.any()
        again = entropy_encode(obj, restart_interval=ri)
        back = entropy_decode(again, pin=False)
        assert not back.status.any()
        assert np.array_equal(back.coef.numpy(), obj.coef.numpy()) and np.array_equal(back.qtabs, obj.qtabs) and np.array_equal(back.desc, obj.desc)
        for (name, d), mine in zip(group, again):
            assert E.scan_bytes(mine) == E.scan_bytes(d), name
            a, b = jpeg_info(mine), jpeg_info(d)
            assert a['supported'] and a['process'] == 'baseline' and a['jfif']
            for k in ('width', 'height', 'components', 'sampling', 'restart_interval'):
                assert a[k] == b[k], (name, k)


def test_whole_files_equal_the_restatement():
    obj = parsed()
    cases = golden()
    got = entropy_encode(obj)
    ri3 = entropy_encode(obj, restart_interval=3)
    for n, (c, img, _) in enumerate(cases):
        if img.size > 64 * 84 * 3:
            continue  # the restatement writes bit by bit in Python
        nc = 1 if img.ndim == 2 else 3
        tabs = _tables_of(c, nc)
        samp, _, coefs = E.forward(img, tabs, c['sub'] if nc == 3 else '444')
        assert got[n] == E.write_stream(img.shape[1], img.shape[0], samp, tabs, coefs, 0), c['name']
        assert ri3[n] == E.write_stream(img.shape[1], img.shape[0], samp, tabs, coefs, 3), c['name']
    # Cr with a table of its own: a third DQT, and SOF0 names it
    o = one(obj, [c['name'] for c, _, _ in cases].index('17x33_420_ramp_q30'))
    o.qtabs[0, 2] = o.qtabs[0, 2] + 1
    img = cases[[c['name'] for c, _, _ in cases].index('17x33_420_ramp_q30')][1]
    h, co = R.entropy_decode(entropy_encode(o)[0])
    assert [c[3] for c in h.comps] == [0, 1, 2] and np.array_equal(h.qtabs[2], o.qtabs[0, 2])
    assert entropy_encode(o)[0] == E.write_stream(17, 33, h.samp, [o.qtabs[0, k] for k in range(3)], co, 0)


def test_thread_counts_give_identical_output():
    obj = parsed()
    want = entropy_encode(obj, threads=1)
    for t in (3, 16, 64):
        assert entropy_encode(obj, threads=t) == want
    assert entropy_encode(obj, restart_interval=2, threads=64) == entropy_encode(obj, restart_interval=2, threads=1)


def test_an_image_that_cannot_be_coded_fails_alone():
    obj = parsed()
    names = [c['name'] for c, _, _ in golden()]
    want = entropy_encode(obj)
    bad_ac, bad_dc, bad_q = names.index('16x16_444_ramp_q75'), names.index('8x8_grey_strokes_q100'), names.index('7x5_422_noise_q95')
    o = JpegCoefficients(obj.coef.clone(), obj.desc.copy(), obj.qtabs.copy(), obj.status.copy())
    o.coef[int(o.desc[bad_ac, 0]) + 5] = 1024      # 11 bits of AC
    o.coef[int(o.desc[bad_dc, 0])] = 2048          # a first DC difference of 12 bits
    o.qtabs[bad_q, 1, 3] = 256
    o.status[names.index('1x1_420_noise_q10')] = 2
    with pytest.raises(JpegEncodeError, match='image 0') as ei:
        entropy_encode(o)
    assert ei.value.index == 0 and isinstance(ei.value, ValueError)
    got, errs = entropy_encode(o, errors='report')
    failed = {bad_ac: 'AC', bad_dc: 'DC', bad_q: 'quantisation', names.index('1x1_420_noise_q10'): 'not decoded'}
    for n in range(len(obj)):
        if n in failed:
            assert got[n] is None and errs[n].index == n and failed[n] in errs[n].reason, (n, errs[n])
        else:
            assert errs[n] is None and got[n] == want[n], names[n]
    # the largest magnitudes a baseline stream holds are coded, and come back
    o = one(obj, bad_ac)
    o.coef[5], o.coef[0], o.coef[64] = -1023, 1000, -1047
    back = entropy_decode(entropy_encode(o), pin=False)
    assert np.array_equal(back.coef.numpy(), o.coef.numpy())
    for bad in (-1, 65536, 1.5):
        with pytest.raises(ValueError):
            entropy_encode(obj, restart_interval=bad)


def test_guard_regions_stay_intact_when_the_bound_is_tight():
    """the C entry point with slots of exactly the streams' sizes (all fit), of one byte less (none fits, nothing outside
    the slots is written) and in a mapping whose last byte is the buffer's last"""
    obj = parsed()
    N = len(obj)
    want = entropy_encode(obj, restart_interval=5)
    L = lib()
    desc, qt = np.ascontiguousarray(obj.desc), np.ascontiguousarray(obj.qtabs)
    per = np.zeros(N, np.int64)
    total = L.dbn_jpeg_encode_bound(desc.ctypes.data, N, 5, per.ctypes.data)
    assert total == per.sum() and (per >= [len(w) for w in want]).all()
    assert L.dbn_jpeg_encode_bound(desc.ctypes.data, N, 70000, None) == -1
    G = 64
    for shrink in (0, 1):
        sizes = np.array([len(w) - shrink for w in want], np.int64)
        offs = np.zeros(N + 1, np.int64)
        offs[1:] = np.cumsum(sizes + G)  # a guard after every slot
        buf = np.full(G + int(offs[-1]), 0xA5, np.uint8)
        ends = offs[:-1] + sizes
        lens, status = np.zeros(N, np.int64), np.full(N, -1, np.int32)
        # slots are [offs[n], offs[n + 1]): give each image its own call so that the slot ends at its size
        for n in range(N):
            o2 = np.array([offs[n], ends[n]], np.int64)
            sub = one(obj, n)
            rc = L.dbn_jpeg_encode_batch(sub.coef.data_ptr(), sub.coef.numel(), sub.desc.ctypes.data, sub.qtabs.ctypes.data, 1, 5,
                                         buf[G:].ctypes.data, int(offs[-1]), o2.ctypes.data, lens[n:].ctypes.data, status[n:].ctypes.data, 4)
            assert rc == 0
        assert (buf[:G] == 0xA5).all()
        for n in range(N):
            assert (buf[G + ends[n]:G + offs[n + 1]] == 0xA5).all(), n
            if shrink == 0:
                assert status[n] == 0 and lens[n] == len(want[n]) and buf[G + offs[n]:G + ends[n]].tobytes() == want[n]
            else:
                assert status[n] == 6 and lens[n] == 0
    # the whole batch against the end of a mapping: one byte past it would fault
    exact = np.array([len(w) for w in want], np.int64)
    offs = np.zeros(N + 1, np.int64)
    offs[1:] = np.cumsum(exact)
    size = int(offs[-1])
    page = mmap.PAGESIZE
    m = mmap.mmap(-1, (-(-size // page) + 1) * page)
    base = ctypes.addressof(ctypes.c_char.from_buffer(m))
    libc = ctypes.CDLL(None, use_errno=True)
    libc.mprotect.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert libc.mprotect(base + -(-size // page) * page, page, 0) == 0
    start = base + -(-size // page) * page - size
    lens, status = np.zeros(N, np.int64), np.zeros(N, np.int32)
    assert L.dbn_jpeg_encode_batch(obj.coef.data_ptr(), obj.coef.numel(), desc.ctypes.data, qt.ctypes.data, N, 5, start, size, offs.ctypes.data,
                                   lens.ctypes.data, status.ctypes.data, 16) == 0
    assert not status.any() and np.array_equal(lens, exact)
    assert ctypes.string_at(start, size) == b''.join(want)
    # arguments that do not describe a buffer are refused
    bad = offs.copy()
    bad[-1] = size + 1
    assert L.dbn_jpeg_encode_batch(obj.coef.data_ptr(), obj.coef.numel(), desc.ctypes.data, qt.ctypes.data, N, 5, start, size, bad.ctypes.data,
                                   lens.ctypes.data, status.ctypes.data, 16) == 1
    # a descriptor whose coefficients would lie outside the buffer is refused for that image
    short = L.dbn_jpeg_encode_batch(obj.coef.data_ptr(), obj.coef.numel() - 64, desc.ctypes.data, qt.ctypes.data, N, 5, start, size,
                                    offs.ctypes.data, lens.ctypes.data, status.ctypes.data, 16)
    assert short == 0 and status[-1] == 2 and not status[:-1].any()
    assert libc.mprotect(base + -(-size // page) * page, page, 3) == 0


def test_forward_plan_is_the_decoders_layout():
    """host side of the device half: descriptors, offsets and work tables for a mixed batch equal what entropy_decode
    writes for Pillow's streams of the same images"""
    obj = parsed()
    cases = golden()
    for sub in ('444', '422', '420'):
        pick = [n for n, (c, img, _) in enumerate(cases) if img.ndim == 2 or c['sub'] == sub]
        items, o = [], 0
        for n in pick:
            img = cases[n][1]
            items.append((o + 1, img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3))
            o += img.size
        desc, qtabs, total, tp, tf = J.forward_plan(items, sub, quant_tables(75))
        ref = obj.desc[pick]
        assert np.array_equal(desc[:, 1:4], ref[:, 1:4]) and np.array_equal(desc[:, 6:22], ref[:, 6:22])
        assert np.array_equal(desc[:, 0], np.cumsum(np.r_[0, [int(jpeg_info(cases[n][2])['coefficients']) for n in pick]])[:-1])
        assert [int(v) for v in desc[:, 4]] == [it[0] for it in items]
        assert total == sum(int(jpeg_info(cases[n][2])['coefficients']) for n in pick)
        assert tp.dtype == np.int32 and tf.dtype == np.int32
        for k in range(len(pick)):
            cells = int(desc[k, 20]) * 8 * int(desc[k, 21]) * 8
            assert sorted(tp[tp[:, 0] == k, 1]) == list(range(-(-cells // 256)))
            for c in range(3):
                blocks = int(desc[k, 6 + 4 * c] * desc[k, 7 + 4 * c])
                assert sorted(tf[(tf[:, 0] == k) & (tf[:, 1] == c), 2]) == list(range(0, blocks, 32))
    for bad in ('411', None):
        with pytest.raises(ValueError):
            J.forward_plan([(0, 8, 8, 3)], bad, quant_tables(75))
    for bad in ([[0] * 64], [[256] * 64], [[1] * 63], [[1.5] * 64], [[1] * 64] * 4):
        with pytest.raises(ValueError):
            J._tables(75, bad)


@pytest.mark.skipif(_pil() is None, reason='Pillow with JPEG support is not installed')
def test_fresh_cases_decode_in_pillow_to_the_pixels_of_its_own_file():
    Image = _pil()
    import sys
    sys.path.insert(0, os.path.join(HERE, 'golden'))
    from make_jpeg_golden import SUBSAMPLING, content
    for q in range(1, 101):
        buf = io.BytesIO()
        Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(buf, 'JPEG', quality=q)
        o = entropy_decode([buf.getvalue()], pin=False)
        assert np.array_equal(o.qtabs[0, :2], quant_tables(q)), q
    rng = np.random.default_rng(77)
    imgs, tabs, subs, theirs = [], [], [], []
    for k in range(200):
        w, h = int(rng.integers(1, 90)), int(rng.integers(1, 90))
        sub = ('444', '422', '420', 'grey')[k % 4]
        q = int(rng.integers(10, 101))
        img = content(('noise', 'ramp', 'strokes')[k % 3], rng, w, h)
        buf = io.BytesIO()
        if sub == 'grey':
            img = np.ascontiguousarray(img[:, :, 0])
            Image.fromarray(img).save(buf, 'JPEG', quality=q)
        else:
            Image.fromarray(img).save(buf, 'JPEG', quality=q, subsampling=SUBSAMPLING[sub])
        imgs.append(img), tabs.append(q), subs.append(sub), theirs.append(buf.getvalue())
    # the coefficients of the restatement through the library's writer: our file
    streams = []
    for img, q, sub in zip(imgs, tabs, subs):
        nc = 1 if img.ndim == 2 else 3
        t = [quant_tables(q)[min(c, 1)] for c in range(nc)]
        samp, grids, coefs = E.forward(img, t, sub if nc == 3 else '444')
        desc = np.zeros((1, 24), np.int64)
        desc[0, 1:4] = img.shape[1], img.shape[0], nc
        for c in range(nc):
            desc[0, 6 + 4 * c:10 + 4 * c] = grids[c][1], grids[c][0], samp[c][0], samp[c][1]
        qt = np.zeros((1, 3, 64), np.uint16)
        qt[0, :nc] = t
        coef = torch.from_numpy(np.concatenate([c.reshape(-1) for c in coefs]))
        streams.append(entropy_encode(JpegCoefficients(coef, desc, qt, np.zeros(1, np.int32)))[0])
    for k, (mine, their) in enumerate(zip(streams, theirs)):
        a, b = (np.asarray(Image.open(io.BytesIO(d))) for d in (mine, their))
        assert a.shape == b.shape and np.array_equal(a, b), (k, subs[k], tabs[k], imgs[k].shape)
        assert E.scan_bytes(mine) == E.scan_bytes(their), k
