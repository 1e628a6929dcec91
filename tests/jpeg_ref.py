"""A plain numpy restatement of a baseline JPEG decode as libjpeg does it (jdmarker.c, jdhuff.c, jidctint.c, jdsample.c,
jdcolor.c): markers, Huffman decoding into natural-order coefficients, dequantisation, the slow-integer 8 x 8 inverse DCT,
"fancy" triangle chroma upsampling and YCbCr -> RGB.  It is what csrc/jpeg.hip (host entropy stage, device pixel stage)
is tested against bit for bit, and is itself pinned against Pillow / libjpeg-turbo by tests/golden/make_jpeg_golden.py
and tests/test_jpeg_cpu.py.

  parse(data)            -> Header (raises JpegError with the status code of include/dbnet_hip.h)
  entropy_decode(data)   -> (Header, [per component int16 [bh * bw, 64] natural-order blocks, raster over the padded grid])
  planes(header, coefs)  -> per component uint8 [bh * 8, bw * 8] sample planes (dequantise + IDCT + 128 + clamp)
  decode(data)           -> uint8 [H, W, 3]
"""
import numpy as np

OK, NOT_JPEG, TRUNCATED, PROGRESSIVE, ARITHMETIC, LOSSLESS, PRECISION, COMPONENTS, SAMPLING, MULTISCAN, BAD_HEADER, BAD_CODE, \
    COEF_RUN, MARKER = range(14)
REASONS = {
    NOT_JPEG: 'not a JPEG stream', TRUNCATED: 'truncated stream', PROGRESSIVE: 'progressive (SOF2) is not supported',
    ARITHMETIC: 'arithmetic coding is not supported', LOSSLESS: 'lossless / hierarchical processes are not supported',
    PRECISION: 'sample precision is not 8 bits (12-bit is not supported)',
    COMPONENTS: '4-component / Adobe-transform files are not supported',
    SAMPLING: 'sampling factors other than 4:4:4, 4:2:2 (2x1) and 4:2:0 (2x2) are not supported',
    MULTISCAN: 'non-interleaved multi-scan files are not supported', BAD_HEADER: 'malformed header or missing table',
    BAD_CODE: 'invalid Huffman code', COEF_RUN: 'coefficient run past index 63',
    MARKER: 'entropy data and markers disagree (too few or too many MCUs before a marker)',
}

# natural (row-major) index of the k-th coefficient in zigzag order
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])


class JpegError(ValueError):
    def __init__(self, code):
        ValueError.__init__(self, REASONS[code])
        self.code = code


class Header:
    pass


def _orientation(seg):
    """Exif orientation of an APP1 payload, 0 when absent or malformed"""
    if len(seg) < 14 or seg[:6] != b'Exif\0\0':
        return 0
    t = seg[6:]
    if t[:2] == b'II':
        order = 'little'
    elif t[:2] == b'MM':
        order = 'big'
    else:
        return 0
    u = lambda o, n: int.from_bytes(t[o:o + n], order) if o + n <= len(t) else None  # noqa: E731
    if u(2, 2) != 42:
        return 0
    ifd = u(4, 4)
    n = u(ifd, 2) if ifd is not None else None
    if n is None:
        return 0
    for k in range(n):
        e = ifd + 2 + 12 * k
        if u(e, 2) is None or u(e + 8, 2) is None:
            return 0
        if u(e, 2) == 0x0112:
            v = u(e + 8, 2)
            return v if u(e + 2, 2) == 3 and u(e + 4, 4) == 1 and 1 <= v <= 8 else 0
    return 0


def _huff_table(counts, vals):
    """canonical codes: per length 1..16 (mincode, maxcode, first value index)"""
    code, k, tab = 0, 0, []
    for l in range(1, 17):
        n = counts[l - 1]
        if code + n > (1 << l):
            raise JpegError(BAD_HEADER)
        tab.append((code, code + n - 1 if n else -1, k))
        code = (code + n) << 1
        k += n
    return tab, list(vals)


def parse(data):
    data = bytes(data)
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise JpegError(NOT_JPEG)
    h = Header()
    h.qt, h.dc, h.ac = {}, {}, {}
    h.ri, h.orientation, h.jfif, h.adobe, h.sof = 0, 0, False, -1, None
    p = 2
    while True:
        if p >= n:
            raise JpegError(TRUNCATED)
        if data[p] != 0xFF:
            raise JpegError(BAD_HEADER)
        while p < n and data[p] == 0xFF:
            p += 1
        if p >= n:
            raise JpegError(TRUNCATED)
        m = data[p]
        p += 1
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9:
            raise JpegError(BAD_HEADER)
        if p + 2 > n:
            raise JpegError(TRUNCATED)
        L = data[p] << 8 | data[p + 1]
        if L < 2:
            raise JpegError(BAD_HEADER)
        if p + L > n:
            raise JpegError(TRUNCATED)
        seg = data[p + 2:p + L]
        p += L
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            if h.sof is not None:
                raise JpegError(BAD_HEADER)
            if m == 0xC2:
                raise JpegError(PROGRESSIVE)
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
        elif m == 0xC8:
            raise JpegError(BAD_HEADER)
        elif m == 0xCC:
            raise JpegError(ARITHMETIC)
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                if q + 17 > len(seg):
                    raise JpegError(BAD_HEADER)
                tc, th = seg[q] >> 4, seg[q] & 15
                counts = list(seg[q + 1:q + 17])
                tot = sum(counts)
                if tc > 1 or th > 3 or tot > 256 or q + 17 + tot > len(seg):
                    raise JpegError(BAD_HEADER)
                (h.dc if tc == 0 else h.ac)[th] = _huff_table(counts, seg[q + 17:q + 17 + tot])
                q += 17 + tot
        elif m == 0xDB:
            q = 0
            while q < len(seg):
                pq, tq = seg[q] >> 4, seg[q] & 15
                need = 64 * (2 if pq else 1)
                if pq > 1 or tq > 3 or q + 1 + need > len(seg):
                    raise JpegError(BAD_HEADER)
                raw = seg[q + 1:q + 1 + need]
                zz = [raw[2 * k] << 8 | raw[2 * k + 1] for k in range(64)] if pq else list(raw)
                t = np.zeros(64, np.int32)
                t[ZIGZAG] = zz
                h.qt[tq] = t
                q += 1 + need
        elif m == 0xDD:
            if len(seg) != 2:
                raise JpegError(BAD_HEADER)
            h.ri = seg[0] << 8 | seg[1]
        elif m == 0xE0:
            if seg[:5] == b'JFIF\0':
                h.jfif = True
        elif m == 0xE1:
            if h.orientation == 0:
                h.orientation = _orientation(seg)
        elif m == 0xEE:
            if len(seg) >= 12 and seg[:5] == b'Adobe':
                h.adobe = seg[11]
        elif m == 0xDA:
            if h.sof is None or len(seg) < 1:
                raise JpegError(BAD_HEADER)
            if h.ncomp not in (1, 3) or (h.ncomp == 3 and h.adobe == 0):
                raise JpegError(COMPONENTS)
            if h.ncomp == 3:
                (_, h0, v0, _), (_, h1, v1, _), (_, h2, v2, _) = h.comps
                if (h0, v0) not in ((1, 1), (2, 1), (2, 2)) or (h1, v1, h2, v2) != (1, 1, 1, 1):
                    raise JpegError(SAMPLING)
            ns = seg[0]
            if ns != h.ncomp:
                raise JpegError(MULTISCAN)
            if len(seg) != 4 + 2 * ns:
                raise JpegError(BAD_HEADER)
            h.scan = []
            for c in range(ns):
                cid, t = seg[1 + 2 * c], seg[2 + 2 * c]
                if cid != h.comps[c][0]:
                    raise JpegError(BAD_HEADER)
                td, ta = t >> 4, t & 15
                if td not in h.dc or ta not in h.ac or h.comps[c][3] not in h.qt:
                    raise JpegError(BAD_HEADER)
                h.scan.append((td, ta))
            h.scan_start = p
            break
    if h.ncomp == 1:
        h.hmax = h.vmax = 1
        h.samp = [(1, 1)]
    else:
        h.hmax, h.vmax = h.comps[0][1], h.comps[0][2]
        h.samp = [(c[1], c[2]) for c in h.comps]
    h.mcux = -(-h.width // (8 * h.hmax))
    h.mcuy = -(-h.height // (8 * h.vmax))
    h.grid = [(h.mcuy * v, h.mcux * hh) for hh, v in h.samp]  # (block rows, block columns), padded to whole MCUs
    h.qtabs = [h.qt[c[3]] for c in h.comps]
    return h


class _Bits:
    """the entropy-coded segment as a bit stream: FF00 unstuffed, stops at a marker (zeros are supplied past it)"""

    def __init__(self, data, p):
        self.d, self.p, self.acc, self.n, self.marker, self.fake = data, p, 0, 0, None, 0

    def _byte(self):
        d = self.d
        if self.marker is not None:
            self.fake += 8
            return 0
        if self.p >= len(d):
            self.marker = -1
            self.fake += 8
            return 0
        b = d[self.p]
        self.p += 1
        if b != 0xFF:
            return b
        while True:
            if self.p >= len(d):
                self.marker = -1
                break
            m = d[self.p]
            self.p += 1
            if m == 0:
                return 0xFF
            if m != 0xFF:
                self.marker = m
                break
        self.fake += 8
        return 0

    def fill(self):
        while self.n <= 24:
            self.acc = (self.acc << 8 | self._byte()) & 0xFFFFFFFFFFFF
            self.n += 8

    def get(self, k):
        if k == 0:
            return 0
        self.fill()
        self.n -= k
        return (self.acc >> self.n) & ((1 << k) - 1)

    def overrun(self):
        return self.marker is not None and self.n < self.fake

    def end_interval(self):
        """drop the padding bits; the next thing in the stream must be a marker: -> its code (-1: end of data)"""
        if self.overrun():
            raise JpegError(MARKER if self.marker != -1 else TRUNCATED)
        real = self.n - self.fake if self.marker is not None else self.n
        if real >= 8:
            raise JpegError(MARKER)
        if self.marker is None:
            d = self.d
            if self.p >= len(d):
                raise JpegError(TRUNCATED)
            if d[self.p] != 0xFF:
                raise JpegError(MARKER)
            while self.p < len(d) and d[self.p] == 0xFF:
                self.p += 1
            if self.p >= len(d):
                raise JpegError(TRUNCATED)
            m = d[self.p]
            self.p += 1
            if m == 0:
                raise JpegError(MARKER)
            self.marker = m
        m = self.marker
        if m == -1:
            raise JpegError(TRUNCATED)
        self.acc = self.n = self.fake = 0
        self.marker = None
        return m


def _symbol(b, table):
    tab, vals = table
    b.fill()
    code = 0
    for l in range(1, 17):
        code = (b.acc >> (b.n - l)) & ((1 << l) - 1)
        lo, hi, first = tab[l - 1]
        if hi >= 0 and lo <= code <= hi:
            b.n -= l
            return vals[first + code - lo]
    raise JpegError(BAD_CODE)


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def _wrap16(v):
    return ((v + 32768) & 0xFFFF) - 32768


def entropy_decode(data):
    data = bytes(data)
    h = parse(data)
    coefs = [np.zeros((bh * bw, 64), np.int16) for bh, bw in h.grid]
    b = _Bits(data, h.scan_start)
    pred = [0] * h.ncomp
    total = h.mcux * h.mcuy
    for mcu in range(total):
        if h.ri and mcu and mcu % h.ri == 0:
            if b.end_interval() != 0xD0 + (mcu // h.ri - 1) % 8:
                raise JpegError(MARKER)
            pred = [0] * h.ncomp
        my, mx = divmod(mcu, h.mcux)
        for c in range(h.ncomp):
            hh, vv = h.samp[c]
            td, ta = h.scan[c]
            for v in range(vv):
                for u in range(hh):
                    blk = coefs[c][(my * vv + v) * h.grid[c][1] + mx * hh + u]
                    s = _symbol(b, h.dc[td])
                    if s > 11:
                        raise JpegError(BAD_CODE)
                    pred[c] = _wrap16(pred[c] + _extend(b.get(s), s))
                    blk[0] = pred[c]
                    k = 1
                    while k < 64:
                        rs = _symbol(b, h.ac[ta])
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
                        blk[ZIGZAG[k]] = _wrap16(_extend(b.get(s), s))
                        k += 1
        if b.overrun():
            raise JpegError(MARKER if b.marker != -1 else TRUNCATED)
    m = b.end_interval()
    if 0xD0 <= m <= 0xD7:
        raise JpegError(MARKER)
    return h, coefs


# ---- pixels ---------------------------------------------------------------------------------------------------------
def _idct_1d(i, shift, first):
    z2, z3 = i[2], i[6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 + z3 * (-15137)
    tmp3 = z1 + z2 * 6270
    tmp0 = (i[0] + i[4]) << 13
    tmp1 = (i[0] - i[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * (-7373), z2 * (-20995), z3 * (-16069) + z5, z4 * (-3196) + z5
    tmp0 += z1 + z3
    tmp1 += z2 + z4
    tmp2 += z2 + z3
    tmp3 += z1 + z4
    r = 1 << (shift - 1)
    return [(tmp10 + tmp3 + r) >> shift, (tmp11 + tmp2 + r) >> shift, (tmp12 + tmp1 + r) >> shift, (tmp13 + tmp0 + r) >> shift,
            (tmp13 - tmp0 + r) >> shift, (tmp12 - tmp1 + r) >> shift, (tmp11 - tmp2 + r) >> shift, (tmp10 - tmp3 + r) >> shift]


def idct_blocks(blocks, q):
    """int16 [n, 64] natural-order coefficients, q int [64] -> uint8 [n, 8, 8] (jpeg_idct_islow + range limit)"""
    d = (blocks.astype(np.int64) * np.asarray(q, np.int64)).reshape(-1, 8, 8)
    ws = np.stack(_idct_1d([d[:, k, :] for k in range(8)], 11, True), 1)   # column pass: [n, row, col]
    out = np.stack(_idct_1d([ws[:, :, k] for k in range(8)], 18, False), 2)  # row pass
    return np.clip(out + 128, 0, 255).astype(np.uint8)


def planes(h, coefs):
    out = []
    for c in range(h.ncomp):
        bh, bw = h.grid[c]
        px = idct_blocks(coefs[c], h.qtabs[c]).reshape(bh, bw, 8, 8)
        out.append(px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8))
    return out


def _h2v1(s):
    """rows of the true downsampled width -> twice as wide (h2v1_fancy_upsample)"""
    s = s.astype(np.int32)
    left = np.concatenate([s[:, :1], s[:, :-1]], 1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], 1)
    even = (3 * s + left + 1) >> 2
    odd = (3 * s + right + 2) >> 2
    even[:, 0] = s[:, 0]
    odd[:, -1] = s[:, -1]
    return np.stack([even, odd], 2).reshape(s.shape[0], -1)


def _h2v2(s):
    s = s.astype(np.int32)
    up = np.concatenate([s[:1], s[:-1]], 0)
    down = np.concatenate([s[1:], s[-1:]], 0)
    rows = np.stack([3 * s + up, 3 * s + down], 1).reshape(-1, s.shape[1])
    t = rows
    left = np.concatenate([t[:, :1], t[:, :-1]], 1)
    right = np.concatenate([t[:, 1:], t[:, -1:]], 1)
    even = (3 * t + left + 8) >> 4
    odd = (3 * t + right + 7) >> 4
    even[:, 0] = (4 * t[:, 0] + 8) >> 4
    odd[:, -1] = (4 * t[:, -1] + 7) >> 4
    return np.stack([even, odd], 2).reshape(t.shape[0], -1)


def upsample(plane, H, W, hs, vs):
    """one chroma plane (padded) -> int32 [H, W] at full resolution, for luma sampling hs x vs"""
    ch, cw = -(-H // vs), -(-W // hs)
    s = plane[:ch, :cw]
    if (hs, vs) == (1, 1):
        return s.astype(np.int32)
    if cw <= 2:  # jinit_upsampler: fancy only when downsampled_width > 2
        return np.repeat(np.repeat(s, vs, 0), hs, 1)[:H, :W].astype(np.int32)
    return (_h2v1(s) if vs == 1 else _h2v2(s))[:H, :W]


def to_rgb(h, pl):
    H, W = h.height, h.width
    y = pl[0][:H, :W].astype(np.int32)
    if h.ncomp == 1:
        return np.repeat(y[:, :, None], 3, 2).astype(np.uint8)
    cb = upsample(pl[1], H, W, h.hmax, h.vmax) - 128
    cr = upsample(pl[2], H, W, h.hmax, h.vmax) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], 2), 0, 255).astype(np.uint8)


def decode(data):
    h, coefs = entropy_decode(data)
    return to_rgb(h, planes(h, coefs))
