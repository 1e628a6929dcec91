"""A plain Python / numpy restatement, written from ITU-T T.81, of the entropy stage for JPEG streams of more than one scan:
progressive Huffman streams (SOF2, Annex G: spectral selection and successive approximation) and sequential streams (SOF0 /
SOF1) whose components arrive in several scans.  It is what csrc/jpeg.hip's multiscan path (entropy_decode(...,
multiscan=True)) is tested against bit for bit, status codes included; the pixels come from jpeg_ref.planes / to_rgb and are
pinned against Pillow by tests/golden/make_jpeg_scans_golden.py and tests/test_jpeg_scans_cpu.py.

  entropy_decode(data)  -> (Header, [per component int16 [bh * bw, 64] natural-order blocks over the padded grid]); raises
                           jpeg_ref.JpegError with the status code of include/dbnet_hip.h (14: SCRIPT)
  decode(data)          -> uint8 [H, W, 3]
  status(data)          -> the code, 0 when it decodes

A stream whose first scan is sequential and names every component is jpeg_ref's, and is handed to it.  The rules (all status
10 unless noted): Ss = 0 needs Se = 0; an AC scan has one component and Ss <= Se <= 63; Al <= 13; Ah is 0 or Al + 1; a first
scan (Ah = 0) of a coefficient that was sent before, or a refinement whose Ah is not the Al the coefficient was last sent with;
an AC scan before the component's DC; a sequential scan with Ss, Se, Ah, Al other than 0, 63, 0, 0; a component in two
sequential scans; scan components out of the frame's order.  More than 100 scans, or a coefficient not sent down to Al = 0 at
EOI: 14."""
import numpy as np

import jpeg_ref as R
from jpeg_ref import ARITHMETIC, BAD_CODE, BAD_HEADER, COEF_RUN, COMPONENTS, LOSSLESS, MARKER, NOT_JPEG, PRECISION, SAMPLING, TRUNCATED, ZIGZAG, \
    JpegError

SCRIPT = 14
MAX_SCANS = 100
REASON_SCRIPT = 'scan script incomplete at the end of the image, or longer than 100 scans'


class ScriptError(JpegError):
    def __init__(self):
        ValueError.__init__(self, REASON_SCRIPT)
        self.code = SCRIPT


def _marker(data, p):
    n = len(data)
    if p >= n:
        raise JpegError(TRUNCATED)
    if data[p] != 0xFF:
        raise JpegError(BAD_HEADER)
    while p < n and data[p] == 0xFF:
        p += 1
    if p >= n:
        raise JpegError(TRUNCATED)
    return data[p], p + 1


def _segment(data, p):
    n = len(data)
    if p + 2 > n:
        raise JpegError(TRUNCATED)
    L = data[p] << 8 | data[p + 1]
    if L < 2:
        raise JpegError(BAD_HEADER)
    if p + L > n:
        raise JpegError(TRUNCATED)
    return data[p + 2:p + L], p + L


def _tables(h, m, seg):
    """DHT, DQT, DRI: they hold for the scans that follow"""
    if m == 0xC4:
        q = 0
        while q < len(seg):
            if q + 17 > len(seg):
                raise JpegError(BAD_HEADER)
            tc, th = seg[q] >> 4, seg[q] & 15
            counts = list(seg[q + 1:q + 17])
            tot = sum(counts)
            if tc > 1 or th > 3 or tot > 256 or q + 17 + tot > len(seg):
                raise JpegError(BAD_HEADER)
            (h.dc if tc == 0 else h.ac)[th] = R._huff_table(counts, seg[q + 17:q + 17 + tot])
            q += 17 + tot
    elif m == 0xDB:
        q = 0
        while q < len(seg):
            pq, tq = seg[q] >> 4, seg[q] & 15
            need = 128 if pq else 64
            if pq > 1 or tq > 3 or q + 1 + need > len(seg):
                raise JpegError(BAD_HEADER)
            raw = seg[q + 1:q + 1 + need]
            t = np.zeros(64, np.int32)
            t[ZIGZAG] = [raw[2 * k] << 8 | raw[2 * k + 1] for k in range(64)] if pq else list(raw)
            h.qt[tq] = t
            q += 1 + need
    elif m == 0xDD:
        if len(seg) != 2:
            raise JpegError(BAD_HEADER)
        h.ri = seg[0] << 8 | seg[1]


def _frame(h, m, seg):
    if h.sof is not None:
        raise JpegError(BAD_HEADER)
    if m in (0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
        raise JpegError(ARITHMETIC)
    if m in (0xC3, 0xC5, 0xC6, 0xC7):
        raise JpegError(LOSSLESS)
    if len(seg) < 6:
        raise JpegError(BAD_HEADER)
    if seg[0] != 8:
        raise JpegError(PRECISION)
    h.sof = m - 0xC0
    h.height, h.width, h.ncomp = seg[1] << 8 | seg[2], seg[3] << 8 | seg[4], seg[5]
    if h.height == 0 or h.width == 0 or h.ncomp == 0 or len(seg) != 6 + 3 * h.ncomp:
        raise JpegError(BAD_HEADER)
    h.comps = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(h.ncomp)]


def _geometry(h):
    if h.ncomp == 1:
        h.hmax = h.vmax = 1
        h.samp = [(1, 1)]
    else:
        h.hmax, h.vmax = h.comps[0][1], h.comps[0][2]
        h.samp = [(c[1], c[2]) for c in h.comps]
    h.mcux, h.mcuy = -(-h.width // (8 * h.hmax)), -(-h.height // (8 * h.vmax))
    h.grid = [(h.mcuy * v, h.mcux * hh) for hh, v in h.samp]


def _sequential_block(b, dc, ac, pred, blk):
    s = R._symbol(b, dc)
    if s > 11:
        raise JpegError(BAD_CODE)
    pred = R._wrap16(pred + R._extend(b.get(s), s))
    blk[0] = pred
    k = 1
    while k < 64:
        rs = R._symbol(b, ac)
        r, s = rs >> 4, rs & 15
        if s == 0:
            if r != 15:
                break
            k += 16
            if k > 64:
                raise JpegError(COEF_RUN)
            continue
        k += r
        if k > 63:
            raise JpegError(COEF_RUN)
        blk[ZIGZAG[k]] = R._wrap16(R._extend(b.get(s), s))
        k += 1
    return pred


def _refine(b, blk, z, p1):
    """G.1.2.3: the correction bit of a coefficient whose history is non-zero"""
    if b.get(1) and (int(blk[z]) & p1) == 0:
        v = int(blk[z])
        blk[z] = R._wrap16(v + p1 if v >= 0 else v - p1)


def _progressive_block(b, sc, dc, ac, pred, eob, blk):
    """one block of a progressive scan -> (predictor, end-of-band run)"""
    Ss, Se, Ah, Al = sc
    p1 = 1 << Al
    if Ss == 0:
        if Ah:  # G.1.2.1, refinement: one bit
            if b.get(1):
                blk[0] = R._wrap16(int(blk[0]) | p1)
            return pred, eob
        s = R._symbol(b, dc)
        if s > 11:
            raise JpegError(BAD_CODE)
        pred = R._wrap16(pred + R._extend(b.get(s), s))
        blk[0] = R._wrap16(pred << Al)
        return pred, eob
    k = Ss
    if Ah == 0:  # G.1.2.2
        if eob > 0:
            return pred, eob - 1
        while k <= Se:
            rs = R._symbol(b, ac)
            r, s = rs >> 4, rs & 15
            if s == 0:
                if r != 15:
                    eob = (1 << r) - 1 + (b.get(r) if r else 0)
                    break
                k += 16
                if k > Se + 1:
                    raise JpegError(COEF_RUN)
                continue
            k += r
            if k > Se:
                raise JpegError(COEF_RUN)
            blk[ZIGZAG[k]] = R._wrap16(R._extend(b.get(s), s) << Al)
            k += 1
        return pred, eob
    if eob == 0:  # G.1.2.3
        while k <= Se:
            rs = R._symbol(b, ac)
            r, s = rs >> 4, rs & 15
            val = 0
            if s:
                if s != 1:
                    raise JpegError(BAD_CODE)
                val = p1 if b.get(1) else -p1
            elif r != 15:
                eob = (1 << r) + (b.get(r) if r else 0)
                break
            while k <= Se:
                z = ZIGZAG[k]
                if blk[z] != 0:
                    _refine(b, blk, z, p1)
                else:
                    r -= 1
                    if r < 0:
                        break
                k += 1
            if k > Se:
                raise JpegError(COEF_RUN)
            if s:
                blk[ZIGZAG[k]] = val
            k += 1
    if eob > 0:
        while k <= Se:
            z = ZIGZAG[k]
            if blk[z] != 0:
                _refine(b, blk, z, p1)
            k += 1
        eob -= 1
    return pred, eob


def _scan(data, p, h, comps, tabs, sc, coefs):
    """the entropy data of one scan from byte p -> (the marker that ends it, the byte behind it)"""
    b = R._Bits(data, p)
    prog = h.sof == 2
    if len(comps) == 1:
        c = comps[0]
        cw, ch = -(-h.width * h.samp[c][0] // h.hmax), -(-h.height * h.samp[c][1] // h.vmax)
        ux = -(-cw // 8)
        units = ux * -(-ch // 8)
    else:
        ux, units = h.mcux, h.mcux * h.mcuy
    pred, eob = [0] * 3, 0
    for u in range(units):
        if h.ri and u and u % h.ri == 0:
            if b.end_interval() != 0xD0 + (u // h.ri - 1) % 8:
                raise JpegError(MARKER)
            pred, eob = [0] * 3, 0
        uy, uxx = divmod(u, ux)
        for c, (td, ta) in zip(comps, tabs):
            hh, vv = (1, 1) if len(comps) == 1 else h.samp[c]
            for v in range(vv):
                for x in range(hh):
                    blk = coefs[c][(uy * vv + v) * h.grid[c][1] + uxx * hh + x]
                    if prog:
                        pred[c], eob = _progressive_block(b, sc, h.dc.get(td), h.ac.get(ta), pred[c], eob, blk)
                    else:
                        pred[c] = _sequential_block(b, h.dc[td], h.ac[ta], pred[c], blk)
        if b.overrun():
            raise JpegError(MARKER if b.marker != -1 else TRUNCATED)
    m = b.end_interval()
    if 0xD0 <= m <= 0xD7:
        raise JpegError(MARKER)
    return m, b.p


def entropy_decode(data):
    data = bytes(data)
    if len(data) < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise JpegError(NOT_JPEG)
    h = R.Header()
    h.qt, h.dc, h.ac = {}, {}, {}
    h.ri, h.orientation, h.jfif, h.adobe, h.sof, h.scans = 0, 0, False, -1, None, 0
    p, m, started = 2, None, False
    coefs, sent, cqt = None, None, {}
    while True:
        if m is None:
            m, p = _marker(data, p)
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            m = None
            continue
        if m == 0xD9:
            if not started:
                raise JpegError(BAD_HEADER)
            break
        seg, p = _segment(data, p)
        mk, m = m, None
        if started and mk == 0xCC:
            raise JpegError(ARITHMETIC)
        if 0xC0 <= mk <= 0xCF and mk not in (0xC4, 0xC8, 0xCC):
            _frame(h, mk, seg)
        elif mk == 0xC8:
            raise JpegError(BAD_HEADER)
        elif mk == 0xCC:
            raise JpegError(ARITHMETIC)
        elif mk in (0xC4, 0xDB, 0xDD):
            _tables(h, mk, seg)
        elif mk == 0xE0 and not started:
            if seg[:5] == b'JFIF\0':
                h.jfif = True
        elif mk == 0xE1 and not started:
            if h.orientation == 0:
                h.orientation = R._orientation(seg)
        elif mk == 0xEE and not started:
            if len(seg) >= 12 and seg[:5] == b'Adobe':
                h.adobe = seg[11]
        elif mk == 0xDA:
            if not started:
                if h.sof is None or len(seg) < 1:
                    raise JpegError(BAD_HEADER)
                if h.ncomp not in (1, 3) or (h.ncomp == 3 and h.adobe == 0):
                    raise JpegError(COMPONENTS)
                if h.ncomp == 3:
                    (_, h0, v0, _), (_, h1, v1, _), (_, h2, v2, _) = h.comps
                    if (h0, v0) not in ((1, 1), (2, 1), (2, 2)) or (h1, v1, h2, v2) != (1, 1, 1, 1):
                        raise JpegError(SAMPLING)
                if seg[0] == h.ncomp and h.sof != 2:
                    return R.entropy_decode(data)  # one interleaved sequential scan: the plain decoder's stream
                if any(c[3] > 3 for c in h.comps):
                    raise JpegError(BAD_HEADER)
                _geometry(h)
                h.first_ri = h.ri
                coefs = [np.zeros((bh * bw, 64), np.int16) for bh, bw in h.grid]
                sent = np.full((h.ncomp, 64), -1, np.int64)
                started = True
            h.scans += 1
            if h.scans > MAX_SCANS:
                raise ScriptError()
            ns = seg[0] if len(seg) else 0
            if ns < 1 or ns > h.ncomp or len(seg) != 4 + 2 * ns:
                raise JpegError(BAD_HEADER)
            comps, tabs = [], []
            for i in range(ns):
                ids = [c[0] for c in h.comps]
                if seg[1 + 2 * i] not in ids:
                    raise JpegError(BAD_HEADER)
                c = ids.index(seg[1 + 2 * i])
                if comps and c <= comps[-1]:
                    raise JpegError(BAD_HEADER)
                td, ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
                if td > 3 or ta > 3:
                    raise JpegError(BAD_HEADER)
                comps.append(c)
                tabs.append((td, ta))
            Ss, Se, Ah, Al = seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns] >> 4, seg[3 + 2 * ns] & 15
            prog = h.sof == 2
            if prog:
                if (Se != 0) if Ss == 0 else (ns > 1 or Se < Ss or Se > 63):
                    raise JpegError(BAD_HEADER)
                if Al > 13 or (Ah != 0 and Ah != Al + 1):
                    raise JpegError(BAD_HEADER)
            elif (Ss, Se, Ah, Al) != (0, 63, 0, 0):
                raise JpegError(BAD_HEADER)
            for c, (td, ta) in zip(comps, tabs):
                if prog and Ss > 0 and sent[c, 0] < 0:
                    raise JpegError(BAD_HEADER)
                if (sent[c, Ss:Se + 1] != (Ah if Ah else -1)).any():
                    raise JpegError(BAD_HEADER)
                sent[c, Ss:Se + 1] = Al
                need_dc, need_ac = not prog or (Ss == 0 and Ah == 0), not prog or Ss > 0
                if (need_dc and td not in h.dc) or (need_ac and ta not in h.ac):
                    raise JpegError(BAD_HEADER)
                if c not in cqt:
                    if h.comps[c][3] not in h.qt:
                        raise JpegError(BAD_HEADER)
                    cqt[c] = h.qt[h.comps[c][3]].copy()
            m, p = _scan(data, p, h, comps, tabs, (Ss, Se, Ah, Al), coefs)
    if (sent != 0).any():
        raise ScriptError()
    h.qtabs = [cqt[c] for c in range(h.ncomp)]
    h.ri = h.first_ri  # the descriptor's: the interval in force at the first scan
    return h, coefs


def decode(data):
    h, coefs = entropy_decode(data)
    return R.to_rgb(h, R.planes(h, coefs))


def status(data):
    try:
        entropy_decode(data)
        return 0
    except JpegError as e:
        return e.code
