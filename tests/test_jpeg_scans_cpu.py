"""CPU (-m "not gpu"): the host entropy stage for JPEG streams of more than one scan (csrc/jpeg.hip decode_scans through
entropy_decode(..., multiscan=True)) and its restatement tests/jpeg_scans_ref.py: the restatement against the golden pixels
(Pillow's, tests/golden/jpeg_scans_cases.npz) and fresh Pillow decodes, the library against the restatement bit for bit, the
progressive / baseline cross-check, every validation rule, status 14, the unchanged defaults, a fuzz of truncations and
corruptions with guard regions, and the Exif orientation the host half hands on."""
import io
import json
import os
import pickle

import numpy as np
import pytest
import torch

from db_text_minimal_amd import CorruptJpeg, UnsupportedJpeg, entropy_decode, jpeg_info
from db_text_minimal_amd import jpeg as J
from db_text_minimal_amd._lib import lib
import jpeg_ref as R
import jpeg_scans_ref as S
from test_jpeg_cpu import GUARD, Fenced, with_exif

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'jpeg_scans_cases.npz')
BASELINE = os.path.join(HERE, 'golden', 'jpeg_cases.npz')
_cache = {}


def golden():
    if 'g' not in _cache:
        g = np.load(GOLDEN)
        names = json.loads(str(g['names']))
        _cache['g'] = (names, [g['jpeg_%d' % i].tobytes() for i in range(len(names))], [g['rgb_%d' % i] for i in range(len(names))],
                       {int(k[5:]): g[k].tobytes() for k in g.files if k.startswith('twin_')})
    return _cache['g']


def ref(i):
    """the restatement's (header, coefficients end to end) of fixture i, computed once and never written to"""
    if ('ref', i) not in _cache:
        h, co = S.entropy_decode(golden()[1][i])
        flat = np.concatenate([c.reshape(-1) for c in co])
        flat.setflags(write=False)
        _cache['ref', i] = (h, flat, co)
    return _cache['ref', i]


def _pil():
    try:
        from PIL import Image, features
        return Image if features.check('jpg') else None
    except ImportError:
        return None


def pick(*words):
    names = golden()[0]
    return [i for i, n in enumerate(names) if all(w in n for w in words)][0]


# ---- stream surgery --------------------------------------------------------------------------------------------------
def pieces(data):
    """[(marker, start of its FF, end of its segment, end of the entropy data behind it)] of every segment up to EOI"""
    out, p = [], 2
    while data[p + 1] != 0xD9:
        assert data[p] == 0xFF
        m, e = data[p + 1], p + 2 + (data[p + 2] << 8 | data[p + 3])
        q = e
        if m == 0xDA:
            while not (data[q] == 0xFF and data[q + 1] != 0 and not 0xD0 <= data[q + 1] <= 0xD7):
                q += 1
        out.append((m, p, e, q))
        p = q
    return out


def scans(data):
    return [x for x in pieces(data) if x[0] == 0xDA]


def set_scan(data, k, Ss=None, Se=None, Ah=None, Al=None, comp=None):
    """scan k's SOS header with fields replaced (comp: the id of its first component)"""
    _, a, e, _ = scans(data)[k]
    d = bytearray(data)
    if Ss is not None:
        d[e - 3] = Ss
    if Se is not None:
        d[e - 2] = Se
    if Ah is not None:
        d[e - 1] = Ah << 4 | (d[e - 1] & 15)
    if Al is not None:
        d[e - 1] = (d[e - 1] & 0xF0) | Al
    if comp is not None:
        d[a + 5] = comp
    return bytes(d)


def drop_scan(data, k):
    _, a, _, q = scans(data)[k]
    return data[:a] + data[q:]


def add_component(data, k, cid):
    """scan k's SOS header naming one more component"""
    _, a, e, _ = scans(data)[k]
    body = bytes([data[a + 4] + 1]) + data[a + 5:e - 3] + bytes([cid, 0x11]) + data[e - 3:e]
    return data[:a] + b'\xff\xda' + (len(body) + 2).to_bytes(2, 'big') + body + data[e:]


def zero_progressive(band):
    """a 1 x 1 grey progressive stream of all-zero coefficients, made by hand: DC first (Al = 1), then per band of `band`
    coefficients an AC first scan (Al = 1), then the DC refinement and per band an AC refinement.  Every scan is one code of
    one bit ('0': DC size 0, or EOB) or one correction bit 0, padded with ones: the byte 7F."""
    seg = lambda m, body: bytes([0xFF, m]) + (len(body) + 2).to_bytes(2, 'big') + bytes(body)  # noqa: E731
    one = bytes([1] + [0] * 15 + [0])  # one code of length 1 for symbol 0
    s = b'\xff\xd8' + seg(0xDB, bytes([0]) + bytes([1] * 64)) + seg(0xC2, bytes([8, 0, 1, 0, 1, 1, 1, 0x11, 0]))
    s += seg(0xC4, bytes([0x00]) + one) + seg(0xC4, bytes([0x10]) + one)
    bands = [(k, min(k + band - 1, 63)) for k in range(1, 64, band)]
    sos = lambda Ss, Se, Ah, Al: seg(0xDA, bytes([1, 1, 0x00, Ss, Se, Ah << 4 | Al])) + b'\x7f'  # noqa: E731
    s += sos(0, 0, 0, 1) + b''.join(sos(a, b, 0, 1) for a, b in bands) + sos(0, 0, 1, 0) + b''.join(sos(a, b, 1, 0) for a, b in bands)
    return s + b'\xff\xd9', 2 + 2 * len(bands)


# ---- the restatement ---------------------------------------------------------------------------------------------------
def test_golden_covers_what_it_should():
    names, datas, rgbs, twins = golden()
    assert os.path.getsize(GOLDEN) <= os.path.getsize(BASELINE)
    for w, h in [(1, 1), (7, 5), (8, 8), (17, 16), (33, 31), (53, 37), (96, 80), (640, 480)]:
        for sub in ('grey', '444', '422', '420') if (w, h) != (640, 480) else ('420', ):
            assert any(n.startswith('%dx%d_%s_' % (w, h, sub)) and '_prog' in n for n in names), (w, h, sub)
    for key in ['_q30', '_q75', '_q95', '_q100', '_opt', '_rst_blocks', '_rst_rows', '_noise_', '_ramp_', '_strokes_', '_multi_per_component',
                '_multi_y_then_cbcr']:
        assert any(key in n for n in names), key
    assert twins and all(rgbs[i].shape[0] % 16 == 0 and rgbs[i].shape[1] % 16 == 0 for i in twins)
    # Pillow's script has every kind of scan: (components, Ss, Se, Ah, Al)
    d = datas[pick('53x37_420', '_prog')]
    script = [(d[a + 4], d[e - 3], d[e - 2], d[e - 1] >> 4, d[e - 1] & 15) for _, a, e, _ in scans(d)]
    assert script == [(3, 0, 0, 0, 1), (1, 1, 5, 0, 2), (1, 1, 63, 0, 1), (1, 1, 63, 0, 1), (1, 6, 63, 0, 2), (1, 1, 63, 2, 1), (3, 0, 0, 1, 0),
                      (1, 1, 63, 1, 0), (1, 1, 63, 1, 0), (1, 1, 63, 1, 0)]
    assert any(m == 0xDD for m, _, _, _ in pieces(datas[pick('_multi_per_component_dri')])[6:])  # a DRI between scans


def test_ref_equals_golden_pixels():
    names, datas, rgbs, _ = golden()
    for i, (n, want) in enumerate(zip(names, rgbs)):
        h, _, co = ref(i)
        got = R.to_rgb(h, R.planes(h, co))
        assert got.shape == want.shape and np.array_equal(got, want), n


def _random_progressive(count, seed):
    import sys
    sys.path.insert(0, os.path.join(HERE, 'golden'))
    from make_jpeg_golden import content, encode
    rng = np.random.default_rng(seed)
    for k in range(count):
        w, h = int(rng.integers(1, 70)), int(rng.integers(1, 70))
        sub = ['444', '422', '420', 'grey'][int(rng.integers(0, 4))]
        kind = ['noise', 'ramp', 'strokes'][int(rng.integers(0, 3))]
        kw = dict(quality=int(rng.choice([30, 50, 75, 90, 95, 100])), progressive=True)
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
    cases = list(_random_progressive(100, 99))
    obj = entropy_decode([d for _, d in cases], pin=False, multiscan=True)
    assert not obj.status.any()
    coef = obj.coef.numpy()
    for i, (name, d) in enumerate(cases):
        want = np.asarray(Image.open(io.BytesIO(d)).convert('RGB'))
        h, co = S.entropy_decode(d)
        got = R.to_rgb(h, R.planes(h, co))
        assert got.shape == want.shape and np.array_equal(got, want), name
        flat = np.concatenate([c.reshape(-1) for c in co])
        o = int(obj.desc[i, 0])
        assert np.array_equal(coef[o:o + flat.size], flat), name


# ---- the library against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize('threads', [1, 3, 16])
def test_library_coefficients_tables_and_descriptors_equal_ref(threads):
    names, datas, rgbs, _ = golden()
    obj = entropy_decode(datas, threads=threads, pin=False, multiscan=True)
    assert obj.status.tolist() == [0] * len(datas)
    coef, off, out = obj.coef.numpy(), 0, 0
    for i, n in enumerate(names):
        h, flat, _ = ref(i)
        dsc = obj.desc[i]
        assert dsc[0] == off and dsc[0] % 64 == 0 and (dsc[1], dsc[2], dsc[3]) == (h.width, h.height, h.ncomp), n
        assert dsc[4] == out and dsc[5] == 192 * i
        for c in range(h.ncomp):
            assert tuple(dsc[6 + 4 * c:10 + 4 * c]) == (h.grid[c][1], h.grid[c][0]) + tuple(h.samp[c]), n
            assert np.array_equal(obj.qtabs[i, c], h.qtabs[c].astype(np.uint16)), n
        assert not obj.qtabs[i, h.ncomp:].any()
        assert tuple(dsc[18:24]) == (h.hmax, h.vmax, h.mcux, h.mcuy, 0, h.ri), n
        assert np.array_equal(coef[off:off + flat.size], flat), n  # padding blocks included: what no scan sends stays zero
        off += flat.size
        out += h.width * h.height * 3
    assert off == coef.size and obj.shapes == [r.shape[:2] for r in rgbs]
    assert not obj.orientation.any()


def test_jpeg_info_with_the_keyword():
    names, datas, rgbs, _ = golden()
    for i, (n, d) in enumerate(zip(names, datas)):
        plain, info = jpeg_info(d), jpeg_info(d, multiscan=True)
        assert not plain['supported'] and plain['status'] == (3 if '_prog' in n else 9) and 'scans' not in plain, n
        assert info['supported'] and info['status'] == 0 and info['reason'] is None, n
        assert info['process'] == ('progressive' if '_prog' in n else 'baseline') and info['scans'] == ref(i)[0].scans, n
        assert (info['height'], info['width']) == rgbs[i].shape[:2] and info['coefficients'] == ref(i)[1].size
    assert jpeg_info(datas[pick('53x37_420', '_prog')], multiscan=True)['scans'] == 10
    assert jpeg_info(datas[pick('53x37_grey', '_prog')], multiscan=True)['scans'] == 6


def test_progressive_and_baseline_twins_have_the_same_coefficients():
    names, datas, _, twins = golden()
    assert len(twins) >= 4
    for i, twin in twins.items():
        a = entropy_decode([datas[i]], pin=False, multiscan=True)
        b = entropy_decode([twin], pin=False)
        assert a.status[0] == 0 and b.status[0] == 0 and jpeg_info(twin)['process'] == 'baseline'
        assert torch.equal(a.coef, b.coef) and np.array_equal(a.qtabs, b.qtabs), names[i]


# ---- validation, status 14, defaults ------------------------------------------------------------------------------------------
def _status(data):
    s = int(entropy_decode([data], pin=False, multiscan=True).status[0])
    assert s == S.status(data)
    return s


def test_every_validation_rule_gives_status_10():
    names, datas, _, _ = golden()
    p = datas[pick('53x37_420', '_prog')]   # scans: see test_golden_covers_what_it_should
    per = datas[pick('_multi_per_component')]
    ycc = datas[pick('_multi_y_then_cbcr')]
    assert _status(p) == 0 and _status(per) == 0 and _status(ycc) == 0
    cases = {
        'Ss = 0 with Se != 0': set_scan(p, 0, Se=5),
        'an AC scan of two components': add_component(p, 1, 2),
        'Se < Ss': set_scan(p, 1, Ss=5, Se=1),
        'Se > 63': set_scan(p, 4, Se=64),
        'Al > 13': set_scan(p, 0, Al=14),
        'Ah neither 0 nor Al + 1': set_scan(p, 5, Ah=3),
        'a refinement that is not the one due (Ah = 1 after Al = 2)': set_scan(p, 5, Ah=1, Al=0),
        'a refinement of a band never sent': drop_scan(p, 1),
        'a DC refinement with the wrong Ah': set_scan(p, 6, Ah=2, Al=1),
        'a band sent first twice': set_scan(p, 4, Ss=5),
        'an AC scan before the DC scan': drop_scan(p, 0),
        'a sequential scan with Se = 62': set_scan(per, 1, Se=62),
        'a sequential first scan with Ss = 1': set_scan(per, 0, Ss=1),
        'a sequential scan with Al = 1': set_scan(ycc, 1, Al=1),
        'a sequential scan with Ah = 1': set_scan(ycc, 1, Ah=1),
        'a component in two sequential scans': set_scan(per, 2, comp=2),
        'a scan of a component the frame does not have': set_scan(per, 2, comp=9),
    }
    for what, data in cases.items():
        assert _status(data) == 10, what
        obj = entropy_decode([data], pin=False, multiscan=True)
        assert isinstance(obj.errors()[0], CorruptJpeg) and obj.shapes == [(0, 0)] and not obj.coef.numpy().any(), what


def test_incomplete_and_overlong_scripts_give_status_14():
    names, datas, _, _ = golden()
    for i in (pick('53x37_420', '_prog'), pick('33x31_grey', '_prog'), pick('_multi_per_component'), pick('_multi_y_then_cbcr')):
        d = datas[i]
        cut = drop_scan(d, len(scans(d)) - 1)
        assert _status(cut) == 14, names[i]
        obj = entropy_decode([cut, d], pin=False, multiscan=True)
        e = obj.errors()[0]
        assert isinstance(e, UnsupportedJpeg) and e.code == 14 and 'scan script' in str(e) and obj.errors()[1] is None
        assert obj.shapes[0] == (0, 0) and not obj.coef.numpy()[:int(obj.desc[1, 0])].any()
        assert np.array_equal(obj.coef.numpy()[int(obj.desc[1, 0]):], ref(i)[1])
    d = datas[pick('53x37_420', '_prog')]
    assert _status(drop_scan(d, 6)) == 14  # the DC refinement alone is missing: never refined to Al = 0
    ok, n_ok = zero_progressive(2)
    assert n_ok == 66 and _status(ok) == 0 and jpeg_info(ok, multiscan=True)['scans'] == 66
    assert not entropy_decode([ok], pin=False, multiscan=True).coef.numpy().any()
    long, n_long = zero_progressive(1)
    assert n_long == 128 and _status(long) == 14 and jpeg_info(long, multiscan=True)['scans'] == 128
    assert 14 in J._REFUSED and 14 not in J.REASONS and J.MULTISCAN_REASONS[14] == S.REASON_SCRIPT


def test_without_the_keyword_nothing_changes():
    names, datas, _, _ = golden()
    obj = entropy_decode(datas, pin=False)
    assert obj.status.tolist() == [3 if '_prog' in n else 9 for n in names] and obj.coef.numel() == 0
    assert all(isinstance(e, UnsupportedJpeg) for e in obj.errors())
    with pytest.raises(UnsupportedJpeg):
        J.jpeg_collate([(datas[0], [], [])])
    # the baseline fixtures: the keyword changes nothing about them
    g = np.load(BASELINE)
    base = [g['jpeg_%d' % i].tobytes() for i in range(len(json.loads(str(g['names']))))]
    extra = [g['refused_progressive'].tobytes(), g['refused_cmyk'].tobytes(), base[3][:len(base[3]) // 2], b'']
    a, b = entropy_decode(base + extra, pin=False), entropy_decode(base + extra, pin=False, multiscan=True)
    n = len(base)
    assert a.status.tolist()[n:] == [3, 7, a.status[n + 2], 1] and b.status.tolist()[n:] == [0, 7, a.status[n + 2], 1]
    a2, b2 = entropy_decode(base, pin=False), entropy_decode(base, pin=False, multiscan=True)
    assert a2.coef.numpy().tobytes() == b2.coef.numpy().tobytes() and a2.desc.tobytes() == b2.desc.tobytes()
    assert a2.qtabs.tobytes() == b2.qtabs.tobytes() and a2.status.tobytes() == b2.status.tobytes()
    for d in base[:8]:
        plain = jpeg_info(d)
        assert 'scans' not in plain and jpeg_info(d, multiscan=True) == dict(plain, scans=1)


def test_collate_with_the_keyword():
    import functools
    names, datas, rgbs, _ = golden()
    idx = [pick('53x37_420', '_prog'), pick('_multi_y_then_cbcr'), pick('33x31_grey', '_prog')]
    items = [(datas[i], [np.array([[1, 1], [5, 1], [5, 4], [1, 4]])], ['a']) for i in idx]
    for fn in (J.jpeg_multiscan_collate, functools.partial(J.jpeg_multiscan_collate, multiscan=True)):
        obj, shapes, polys, tags = fn(items)
        assert shapes == [rgbs[i].shape[:2] for i in idx] and polys[0][0].dtype == np.float64 and tags == [['a']] * 3
        assert np.array_equal(obj.coef.numpy(), np.concatenate([ref(i)[1] for i in idx]))
    with pytest.raises(UnsupportedJpeg):
        functools.partial(J.jpeg_multiscan_collate, multiscan=False)(items)
    loader = torch.utils.data.DataLoader(items, batch_size=3, collate_fn=J.jpeg_multiscan_collate, num_workers=1)
    (obj2, shapes2, _, _), = list(loader)
    assert torch.equal(obj2.coef, obj.coef) and shapes2 == shapes and np.array_equal(obj2.orientation, obj.orientation)


# ---- damage ------------------------------------------------------------------------------------------------------------------
def _fenced_status(data):
    """the three _ex entry points on ONE stream that ends at an unreadable page, guards around the coefficients -> status"""
    L = lib()
    f = Fenced(data)
    info = np.zeros(24, np.int64)
    assert L.dbn_jpeg_info_ex(f.ptr, f.len, 1, info.ctypes.data) == 0
    offs = np.array([0, f.len], np.int64)
    per = np.zeros(1, np.int64)
    total = int(L.dbn_jpeg_coef_elems_ex(f.ptr, offs.ctypes.data, 1, 1, per.ctypes.data))
    assert total == per[0] == info[15]
    buf = np.full(total + 2 * GUARD, 0x5A5A, np.int16)
    desc, qt, st, ori = np.zeros((1, 24), np.int64), np.zeros((1, 3, 64), np.uint16), np.full(1, -1, np.int32), np.full(3, -7, np.int32)
    assert L.dbn_jpeg_entropy_batch_ex(f.ptr, offs.ctypes.data, 1, buf[GUARD:].ctypes.data, total, desc.ctypes.data, qt.ctypes.data,
                                       st.ctypes.data, ori[1:].ctypes.data, 1, 1) == 0
    assert (buf[:GUARD] == 0x5A5A).all() and (buf[GUARD + total:] == 0x5A5A).all(), 'a decode wrote outside the coefficient buffer'
    assert ori[0] == -7 and ori[2] == -7 and 0 <= ori[1] <= 8
    assert (info[0] == 0) == (total > 0) and (st[0] == 0) <= (info[0] == 0)
    if st[0] != 0:
        assert not buf[GUARD:GUARD + total].any()
    return int(st[0])


def _guarded_batch(streams, good, good_ref, threads=4):
    """`good` in front of and behind `streams`, as one batch that ends at an unreadable page, the coefficient buffer between guard
    regions: the good members decode to good_ref whatever happens between them -> the status of each of `streams`"""
    L = lib()
    batch = [good] + list(streams) + [good]
    N = len(batch)
    offs = np.zeros(N + 1, np.int64)
    offs[1:] = np.cumsum([len(s) for s in batch])
    f = Fenced(b''.join(batch))
    per = np.zeros(N, np.int64)
    total = int(L.dbn_jpeg_coef_elems_ex(f.ptr, offs.ctypes.data, N, 1, per.ctypes.data))
    assert total == per.sum()
    buf = np.full(total + 2 * GUARD, 0x5A5A, np.int16)
    desc, qt, st = np.zeros((N, 24), np.int64), np.zeros((N, 3, 64), np.uint16), np.full(N, -1, np.int32)
    assert L.dbn_jpeg_entropy_batch_ex(f.ptr, offs.ctypes.data, N, buf[GUARD:].ctypes.data, total, desc.ctypes.data, qt.ctypes.data,
                                       st.ctypes.data, None, threads, 1) == 0
    assert (buf[:GUARD] == 0x5A5A).all() and (buf[GUARD + total:] == 0x5A5A).all(), 'a decode wrote outside the coefficient buffer'
    assert ((st >= 0) & (st <= 14)).all() and st[0] == 0 and st[-1] == 0
    for n in (0, N - 1):
        o = GUARD + int(desc[n, 0])
        assert np.array_equal(buf[o:o + per[n]], good_ref)
    for n in range(1, N - 1):
        if st[n] != 0 and per[n]:
            o = GUARD + int(desc[n, 0])
            assert not buf[o:o + per[n]].any()
    return st[1:-1].tolist()


def _corruptions(d, count, rng):
    out = []
    for _ in range(count):
        c = bytearray(d)
        c[int(rng.integers(0, len(c)))] = int(rng.integers(0, 256))
        out.append(bytes(c))
    return out


def test_damage_of_the_two_shortest_streams_has_the_status_of_the_restatement():
    names, datas, _, _ = golden()
    order = sorted(range(len(datas)), key=lambda i: len(datas[i]))
    rng = np.random.default_rng(1414)
    n = 0
    for i in order[:2]:
        d = datas[i]
        damaged = [d[:k] for k in range(len(d))] + _corruptions(d, 200, rng)
        obj = entropy_decode(damaged, pin=False, multiscan=True)
        assert all(s != 0 for s in obj.status[:len(d)])
        coef = obj.coef.numpy()
        for k, c in enumerate(damaged):
            s = int(obj.status[k])
            assert s == S.status(c), (names[i], k)
            if s == 0:
                flat = np.concatenate([x.reshape(-1) for x in S.entropy_decode(c)[1]])
                o = int(obj.desc[k, 0])
                assert np.array_equal(coef[o:o + flat.size], flat), (names[i], k)
            n += 1
    assert n >= 2 * 400


def test_damage_never_leaves_the_buffers_and_fails_alone():
    names, datas, _, _ = golden()
    order = sorted(range(len(datas)), key=lambda i: len(datas[i]))
    g = pick('17x16_420', '_prog')
    good, good_ref = datas[g], ref(g)[1]
    rng = np.random.default_rng(4343)
    n_trunc = n_corrupt = 0
    for i in order[2:]:
        d = datas[i]
        cuts = [d[:k] for k in range(0, len(d), 7)]
        st = _guarded_batch(cuts, good, good_ref)
        assert all(s != 0 for s in st), names[i]
        alone = cuts[::max(1, len(cuts) // 12)]  # and a dozen of them alone, each ending at an unreadable page
        assert [_fenced_status(c) for c in alone] == st[::max(1, len(cuts) // 12)]
        n_trunc += len(cuts)
        bad = _corruptions(d, 50, rng)
        st = _guarded_batch(bad, good, good_ref)
        assert [_fenced_status(c) for c in bad[:6]] == st[:6]
        n_corrupt += len(bad)
    assert n_trunc >= 3000 and n_corrupt >= 1900


# ---- orientation, as the host half hands it on -----------------------------------------------------------------------------------
def test_orientation_attribute_shapes_and_pickle():
    names, datas, rgbs, _ = golden()
    i, j = pick('53x37_420', '_prog'), pick('33x31_grey', '_prog')
    g = np.load(BASELINE)
    base = g['jpeg_4'].tobytes()
    for order in ('II', 'MM'):
        batch = [with_exif(datas[i], t, order) if t else datas[i] for t in range(9)] + [with_exif(base, 6, order), datas[j][:40]]
        for t in range(9):
            assert jpeg_info(batch[t], multiscan=True)['orientation'] == t and jpeg_info(batch[t])['orientation'] == t
        obj = entropy_decode(batch, pin=False, multiscan=True)
        assert obj.orientation.dtype == np.int32 and obj.orientation.tolist() == list(range(9)) + [6, 0]
        h, w = rgbs[i].shape[:2]
        bh, bw = obj.shapes[9]
        assert obj.shapes == [(h, w)] * 9 + [(bh, bw), (0, 0)]
        assert obj.oriented_shapes == [(h, w)] * 5 + [(w, h)] * 4 + [(bw, bh), (0, 0)]
        back = pickle.loads(pickle.dumps(obj))
        assert np.array_equal(back.orientation, obj.orientation) and back.oriented_shapes == obj.oriented_shapes
        assert torch.equal(back.coef, obj.coef) and back.shapes == obj.shapes
    plain = entropy_decode([with_exif(base, 8)], pin=False)
    assert plain.orientation.tolist() == [8] and plain.oriented_shapes == [plain.shapes[0][::-1]]
    old = J.JpegCoefficients(plain.coef, plain.desc, plain.qtabs, plain.status)  # as one made before there was the attribute
    assert old.orientation is None and old.oriented_shapes == old.shapes
    a = np.arange(2 * 3 * 3).reshape(2, 3, 3)
    assert np.array_equal(J.orient_array(a, 6), np.rot90(a, -1)) and np.array_equal(J.orient_array(a, 8), np.rot90(a, 1))
    assert np.array_equal(J.orient_array(a, 3), a[::-1, ::-1]) and np.array_equal(J.orient_array(a, 5), a.transpose(1, 0, 2))
    assert np.array_equal(J.orient_array(a, 1), a) and np.array_equal(J.orient_array(a, 0), a)


def test_tile_table_lists_every_tile_of_the_oriented_images_once():
    desc = np.zeros((4, 24), np.int64)
    desc[:, 1], desc[:, 2] = [65, 40, 33, 7], [33, 50, 65, 5]  # W, H
    tt = J.tile_table(desc, np.array([0, 0, 3, 0]), np.array([6, 1, 5, 2]))
    assert tt.dtype == np.int32 and tt.shape[1] == 4
    assert sorted(map(tuple, tt[tt[:, 0] == 0][:, 1:3])) == [(y, x) for y in range(3) for x in range(2)]  # oriented: 65 rows, 33 columns
    assert tt[tt[:, 0] == 3][:, 1:3].tolist() == [[0, 0]] and not (tt[:, 0] == 1).any() and not (tt[:, 0] == 2).any()
    assert len(J.tile_table(desc, np.zeros(4), np.zeros(4))) == 0
