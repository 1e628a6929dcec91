"""CPU: the host half of the device Huffman decoder (parse_streams: dbn_jpeg_stream_plan of csrc/jpeg.hip) and the plain
restatement of its device half (tests/jpeg_dhuff_ref.py).  The oracle is the host decoder entropy_decode (pinned against
Pillow by tests/test_jpeg_cpu.py) and tests/jpeg_ref.py: descriptors, tables and status of every golden stream; the segment
table against one derived from jpeg_ref's parse (byte ranges, MCU ranges, the RSTn sequence through RST7 -> RST0); refused
kinds and truncations with guard regions around every output; pickling and a DataLoader worker; the restatement against
jpeg_ref.entropy_decode on the golden and the hand-built streams, its round counts within the default, and max_rounds=0
leaving every segment that crosses workgroups unconverged.  Reads tests/golden only."""
import pickle

import numpy as np
import torch

import jpeg_dhuff_cases as C
import jpeg_dhuff_ref as D
import jpeg_ref as R
from db_text_minimal_amd import JpegStreams, entropy_decode, jpeg_stream_collate, parse_streams
from db_text_minimal_amd import jpeg as J
from db_text_minimal_amd._lib import lib
from test_jpeg_cpu import Fenced, golden, refused_streams

GUARD = 64


def test_constants_agree():
    assert (J.DHUFF_BITS, J.DHUFF_LANES, J.DHUFF_ROUNDS) == (D.S, D.W, D.ROUNDS) and D.ROUNDS >= 2


def test_plan_equals_the_host_decoder_and_the_restatement_on_every_golden_stream():
    datas = [d for _, d in C.golden_streams()] + [d for _, d in C.hand_built()]
    st, host = parse_streams(datas, pin=False), entropy_decode(datas, pin=False)
    assert isinstance(st, JpegStreams) and len(st) == len(datas) and st.shapes == host.shapes and st.errors() == [None] * len(datas)
    assert (st.desc == host.desc).all() and (st.qtabs == host.qtabs).all() and (st.status == host.status).all() and not st.host_only.any()
    assert st.coef_elems == host.coef.numel()
    rows, seen_wrap = [], False
    for n, d in enumerate(datas):
        h, segs = D.segments(d)
        # independently of segments(): the markers of the scan as jpeg_ref's reader meets them
        assert len(segs) == (-(-h.mcux * h.mcuy // h.ri) if h.ri else 1)
        for k, (a, b, m0, mc, rst) in enumerate(segs):
            assert d[b] == 0xFF and (d[b + 1] == 0xD0 + k % 8 if k + 1 < len(segs) else d[b + 1] == 0xD9)
            assert a == (h.scan_start if k == 0 else segs[k - 1][1] + 2) and m0 == k * h.ri and rst == ((k - 1) % 8 if k else -1)
            seen_wrap = seen_wrap or (k >= 9 and rst == 0)
            rows.append((n, a + int(st.offs[n]), b + int(st.offs[n]), m0, mc, rst))
        assert sum(s[3] for s in segs) == h.mcux * h.mcuy
        sel = int(st.info[n, 0])
        assert [(sel >> 8 * c & 15, sel >> (8 * c + 4) & 15) for c in range(h.ncomp)] == list(h.scan)
        for t in range(8):
            tab = (h.dc if t < 4 else h.ac).get(t & 3)
            assert bool(st.tables[n, t, 0]) == (tab is not None)
            if tab is not None:
                counts = [hi - lo + 1 if hi >= 0 else 0 for lo, hi, _ in tab[0]]
                assert st.tables[n, t, 1:17].tolist() == counts and st.tables[n, t, 17:17 + len(tab[1])].tolist() == list(tab[1])
    assert seen_wrap
    assert st.segments.tolist() == [list(r) for r in rows]
    bits = (st.segments[:, 2] - st.segments[:, 1]) * 8
    assert (np.diff(st.sub_base) == np.maximum(1, -(-bits // D.S))).all() and st.sub_base[0] == 0
    assert st.wgtab[:, 2].sum() == st.sub_base[-1] and (st.wgtab[:, 2] <= D.W).all()


def _guarded_plan(datas):
    """dbn_jpeg_stream_plan straight through ctypes, the batch ending at an unreadable page and every output between guard words"""
    L, N = lib(), len(datas)
    offs = np.zeros(N + 1, np.int64)
    offs[1:] = np.cumsum([len(d) for d in datas])
    f = Fenced(b''.join(datas))

    def arr(n, dt):
        a = np.full(n + 2 * GUARD, 0x5A, dt)
        return a, a[GUARD:GUARD + n]
    outs = [arr(N * 24, np.int64), arr(N * 192, np.uint16), arr(N, np.int32), arr(N * 8 * 273, np.uint8), arr(N * 8, np.int64)]
    counts = np.zeros(4, np.int64)
    head = [f.ptr, offs.ctypes.data, N] + [v.ctypes.data for _, v in outs]
    assert L.dbn_jpeg_stream_plan(*head, None, 0, None, None, 0, counts.ctypes.data) == 0
    nseg, nwg = int(counts[0]), int(counts[2])
    more = [arr(max(nseg, 1) * 6, np.int64), arr(nseg + 1, np.int64), arr(max(nwg, 1) * 4, np.int32)]
    c2 = np.zeros(4, np.int64)
    assert L.dbn_jpeg_stream_plan(*head, more[0][1].ctypes.data, nseg, more[1][1].ctypes.data, more[2][1].ctypes.data, nwg, c2.ctypes.data) == 0
    assert (c2 == counts).all()
    for (full, v), n in zip(outs + more, [N * 24, N * 192, N, N * 8 * 273, N * 8, max(nseg, 1) * 6, nseg + 1, max(nwg, 1) * 4]):
        assert (full[:GUARD] == 0x5A).all() and (full[GUARD + n:] == 0x5A).all(), 'the plan wrote outside a buffer'
    return outs[2][1].copy(), outs[4][1].reshape(N, 8)[:, 1].copy()


def test_refused_kinds_and_truncations_have_the_host_status():
    _, datas, _, _ = golden()
    cases = [d for _, d, _, _ in refused_streams()]
    short = sorted(datas, key=len)[:3]
    for d in short:
        cases += [d[:k] for k in range(0, len(d))]
    host = entropy_decode(cases, pin=False).status
    status, host_only = _guarded_plan(cases)
    hdr = np.array([R.OK, R.TRUNCATED, R.BAD_CODE, R.COEF_RUN, R.MARKER])
    for n in range(len(cases)):
        # what the header gives is the same status; what is wrong inside the scan is left to the decoder: marked, status 0
        assert status[n] == host[n] or (status[n] == 0 and host_only[n] and host[n] in hdr[1:]), (n, status[n], host[n], host_only[n])
        assert not (host[n] == 0 and host_only[n])
    assert (status[:len(refused_streams())] == host[:len(refused_streams())]).all() and (host[:len(refused_streams())] != 0).all()
    assert host_only.any()


class _Bytes(torch.utils.data.Dataset):
    def __init__(self, datas):
        self.datas = datas

    def __len__(self):
        return len(self.datas)

    def __getitem__(self, i):
        return self.datas[i], [np.zeros((4, 2))], ['x']


def test_streams_pickle_and_collate_in_a_loader_worker():
    datas = [d for _, d in C.golden_streams()[:6]]
    want = parse_streams(datas, pin=False)
    got = pickle.loads(pickle.dumps(want))
    loader = torch.utils.data.DataLoader(_Bytes(datas), batch_size=6, collate_fn=jpeg_stream_collate, num_workers=1)
    (obj, shapes, polys, tags), = list(loader)
    for o in (got, obj):
        assert isinstance(o, JpegStreams) and torch.equal(o.blob, want.blob) and shapes == want.shapes
        for k in ('offs', 'desc', 'qtabs', 'status', 'tables', 'info', 'segments', 'sub_base', 'wgtab'):
            assert (getattr(o, k) == getattr(want, k)).all(), k
    assert hasattr(obj, 'pin_memory') and len(polys) == 6 and tags[0] == ['x']


def test_restatement_equals_the_reference_decode_and_stays_within_the_default_rounds():
    multi = 0
    for name, d in C.golden_streams() + C.hand_built():
        _, want = R.entropy_decode(d)
        r = D.decode(d)
        assert not r.flagged and r.converged and not r.host, name
        assert r.rounds is not None and 2 * r.rounds <= D.ROUNDS, (name, r.rounds)
        for a, b in zip(want, r.coefs):
            assert (a == b).all(), name
        multi += r.rounds > 0
    assert multi  # some streams do cross workgroups


def test_without_rounds_every_segment_that_crosses_workgroups_is_unconverged():
    crossing = 0
    for name, d in C.golden_streams() + C.hand_built():
        h, segs = D.segments(d)
        first, crosses = 0, False
        for a, b, _, _, _ in segs:
            ns = max(1, -(-(b - a) * 8 // D.S))
            crosses = crosses or first // D.W != (first + ns - 1) // D.W
            first += ns
        r = D.decode(d, 0)
        assert r.converged == (not crosses) and r.host == crosses, name
        crossing += crosses
    assert crossing >= 3
