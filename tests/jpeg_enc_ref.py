"""A plain numpy restatement of a baseline JPEG encode as libjpeg does it (jccolor.c, jcsample.c without smoothing,
jfdctint.c, jcdctmgr.c's quantiser, jccoefct.c's dummy blocks, jcparam.c's quality scaling, jcmarker.c, jchuff.c with the
Annex K tables).  It is what csrc/jpeg_enc.hip (device forward stage, host Huffman stage) is tested against bit for bit, and
is itself pinned against Pillow / libjpeg-turbo by tests/golden/make_jpeg_encode_golden.py and tests/test_jpeg_encode_cpu.py.

  quant_tables(quality)                          -> int [2, 64] natural order (luma, chroma)
  forward(img, qtabs, subsampling)               -> (samp [(h, v)], grids [(block rows, block columns)], [int16 [bh * bw, 64]])
  write_stream(W, H, samp, qtabs, coefs, ri)     -> bytes (coefficients as given, dummy blocks included)
  encode(img, quality, subsampling, qtables, ri) -> bytes
  scan_bytes(data)                               -> the bytes after the SOS header, EOI included
"""
import numpy as np

from jpeg_ref import ZIGZAG

SAMPLING = {'444': (1, 1), '422': (2, 1), '420': (2, 2)}

# Annex K.1 / K.2 base tables, natural (row-major) order
BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                      80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
                      95, 98, 112, 100, 103, 99])
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99,
                        99, 99] + [99] * 32)

# Annex K.3 Huffman tables: (counts per code length 1 .. 16, values)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
            0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
            0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
            0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
            0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
            0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
            0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
            0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
              0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
              0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
              0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
              0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
              0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
              0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
              0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])


class EncodeError(ValueError):
    """a coefficient that a baseline stream cannot hold"""


def quant_tables(quality):
    """jpeg_set_quality: the Annex K tables scaled by jpeg_quality_scaling(quality), baseline-clamped"""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError('quality is 1 .. 100')
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((b * scale + 50) // 100, 1, 255) for b in (BASE_LUMA, BASE_CHROMA)]).astype(np.int64)


# ---- forward path ----------------------------------------------------------------------------------------------------
def ycc(img):
    """uint8 [H, W, 3] -> int32 Y, Cb, Cr planes (jccolor.c rgb_ycc_convert)"""
    r, g, b = (img[:, :, k].astype(np.int64) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad_cols(p, n):
    return p if p.shape[1] >= n else np.concatenate([p, np.repeat(p[:, -1:], n - p.shape[1], 1)], 1)


def _pad_rows(p, n):
    return p if p.shape[0] >= n else np.concatenate([p, np.repeat(p[-1:], n - p.shape[0], 0)], 0)


def component_plane(p, hs, vs, bh, bw):
    """full-resolution int plane [H, W] of a component downsampled by hs x vs -> int [bh * 8, bw * 8] samples: the last
    column replicated out to 8 * bw * hs, the last row only to a multiple of vs, the downsampling, then the last
    downsampled row replicated to 8 * bh"""
    H = p.shape[0]
    p = _pad_rows(_pad_cols(p, 8 * bw * hs), -(-H // vs) * vs)
    if hs == 2 and vs == 1:
        bias = np.tile([0, 1], p.shape[1] // 2)[:p.shape[1] // 2]
        p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
    elif hs == 2 and vs == 2:
        bias = np.tile([1, 2], p.shape[1] // 2)[:p.shape[1] // 2]
        p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
    elif (hs, vs) != (1, 1):
        raise ValueError('sampling %d x %d' % (hs, vs))
    return _pad_rows(p, 8 * bh)


def _fdct_1d(d, first):
    """jpeg_fdct_islow's one-dimensional pass over eight arrays"""
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    r = 1 << (n - 1)
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[0], o[4] = (t10 + t11 + 2) >> 2, (t10 - t11 + 2) >> 2
    z1 = (t12 + t13) * 4433
    o[2] = (z1 + t13 * 6270 + r) >> n
    o[6] = (z1 - t12 * 15137 + r) >> n
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7] = (t4 + z1 + z3 + r) >> n
    o[5] = (t5 + z2 + z4 + r) >> n
    o[3] = (t6 + z2 + z3 + r) >> n
    o[1] = (t7 + z1 + z4 + r) >> n
    return o


def fdct_quantise(blocks, q):
    """int [n, 8, 8] samples (0 .. 255), q int [64] natural -> int [n, 64] quantised coefficients"""
    d = blocks.astype(np.int64) - 128
    rows = np.stack(_fdct_1d([d[:, :, k] for k in range(8)], True), 2)      # along each row: [n, row, frequency]
    out = np.stack(_fdct_1d([rows[:, k, :] for k in range(8)], False), 1)   # along each column
    x = out.reshape(-1, 64)
    div = 8 * np.asarray(q, np.int64)
    return np.sign(x) * ((np.abs(x) + div // 2) // div)


def geometry(W, H, samp):
    """-> (mcux, mcuy, padded grids [(bh, bw)], real grids [(block rows, block columns)])"""
    hmax, vmax = max(h for h, _ in samp), max(v for _, v in samp)
    mcux, mcuy = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    grids = [(mcuy * v, mcux * h) for h, v in samp]
    real = [(-(-(-(-H * v // vmax)) // 8), -(-(-(-W * h // hmax)) // 8)) for h, v in samp]
    return mcux, mcuy, grids, real


def forward(img, qtabs, subsampling='420'):
    """uint8 [H, W, 3] (or [H, W] grey), per-component tables -> (samp, grids, coefs): libjpeg's quantised coefficients
    over the MCU-padded grid, dummy blocks as jccoefct.c compress_data leaves them"""
    img = np.asarray(img)
    if img.ndim == 2:
        comps, samp = [img.astype(np.int64)], [(1, 1)]
    else:
        comps, samp = list(ycc(img)), [SAMPLING[subsampling], (1, 1), (1, 1)]
    H, W = img.shape[:2]
    hmax, vmax = samp[0]
    mcux, mcuy, grids, real = geometry(W, H, samp)
    coefs = []
    for c, p in enumerate(comps):
        (h, v), (bh, bw), (rh, rw) = samp[c], grids[c], real[c]
        plane = component_plane(p, hmax // h, vmax // v, rh, rw)
        blocks = plane.reshape(rh, 8, rw, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)
        k = fdct_quantise(blocks, qtabs[c]).reshape(rh, rw, 64)
        out = np.zeros((bh, bw, 64), np.int64)
        out[:rh, :rw] = k
        for by in range(bh):
            for bx in range(bw):
                if by < rh and bx >= rw:
                    out[by, bx, 0] = out[by, bx - 1, 0]
                elif by >= rh:  # the last block of the row above within the same MCU, or the left neighbour
                    out[by, bx, 0] = out[by - 1, bx // h * h + h - 1, 0] if bx % h == 0 else out[by, bx - 1, 0]
        coefs.append(out.reshape(bh * bw, 64).astype(np.int16))
    return samp, grids, coefs


# ---- the stream ------------------------------------------------------------------------------------------------------
def _codes(table):
    counts, vals = table
    out, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            out[vals[k]] = (code, l)
            code += 1
            k += 1
        code <<= 1
    return out


class _Writer:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, size):
        self.acc = self.acc << size | code
        self.n += size
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 255
            self.out.append(b)
            if b == 255:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, 'big') + bytes(payload)


def _dht(tc, th, table):
    return _seg(0xC4, bytes([tc << 4 | th]) + bytes(table[0]) + bytes(table[1]))


def write_stream(W, H, samp, qtabs, coefs, ri=0):
    nc = len(samp)
    qtabs = [np.asarray(q, np.int64).reshape(64) for q in qtabs]
    if any(q.min() < 1 or q.max() > 255 for q in qtabs):
        raise EncodeError('quantisation values are 1 .. 255 in a baseline stream')
    tq = [0] if nc == 1 else [0, 1, 1 if np.array_equal(qtabs[1], qtabs[2]) else 2]
    s = bytes([0xFF, 0xD8]) + _seg(0xE0, b'JFIF\0' + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for t in sorted(set(tq)):
        s += _seg(0xDB, bytes([t]) + bytes(int(v) for v in qtabs[tq.index(t)][ZIGZAG]))
    s += _seg(0xC0, bytes([8]) + H.to_bytes(2, 'big') + W.to_bytes(2, 'big') + bytes([nc])
              + b''.join(bytes([c + 1, samp[c][0] << 4 | samp[c][1], tq[c]]) for c in range(nc)))
    s += _dht(0, 0, DC_LUMA) + _dht(1, 0, AC_LUMA)
    if nc == 3:
        s += _dht(0, 1, DC_CHROMA) + _dht(1, 1, AC_CHROMA)
    if ri:
        s += _seg(0xDD, ri.to_bytes(2, 'big'))
    s += _seg(0xDA, bytes([nc]) + b''.join(bytes([c + 1, 0x00 if c == 0 else 0x11]) for c in range(nc)) + bytes([0, 63, 0]))
    dc = [_codes(DC_LUMA)] + [_codes(DC_CHROMA)] * 2
    ac = [_codes(AC_LUMA)] + [_codes(AC_CHROMA)] * 2
    mcux, mcuy, grids, _ = geometry(W, H, samp)
    w = _Writer()
    pred = [0] * nc
    for mcu in range(mcux * mcuy):
        if ri and mcu and mcu % ri == 0:
            w.flush()
            w.out += bytes([0xFF, 0xD0 + (mcu // ri - 1) % 8])
            pred = [0] * nc
        my, mx = divmod(mcu, mcux)
        for c in range(nc):
            hh, vv = samp[c]
            for v in range(vv):
                for u in range(hh):
                    blk = coefs[c][(my * vv + v) * grids[c][1] + mx * hh + u]
                    zz = [int(x) for x in blk[ZIGZAG]]
                    d = zz[0] - pred[c]
                    pred[c] = zz[0]
                    n = abs(d).bit_length()
                    if n > 11:
                        raise EncodeError('a DC difference needs more than 11 bits')
                    w.put(*dc[c][n])
                    if n:
                        w.put((d if d >= 0 else d - 1) & ((1 << n) - 1), n)
                    run = 0
                    for k in range(1, 64):
                        x = zz[k]
                        if x == 0:
                            run += 1
                            continue
                        while run > 15:
                            w.put(*ac[c][0xF0])
                            run -= 16
                        n = abs(x).bit_length()
                        if n > 10:
                            raise EncodeError('an AC coefficient needs more than 10 bits')
                        w.put(*ac[c][run << 4 | n])
                        w.put((x if x >= 0 else x - 1) & ((1 << n) - 1), n)
                        run = 0
                    if run:
                        w.put(*ac[c][0])
    w.flush()
    return s + bytes(w.out) + bytes([0xFF, 0xD9])


def component_tables(nc, quality=75, qtables=None):
    """the per-component tables: quant_tables(quality), or `qtables` (1, 2 or 3 tables of 64 in natural order)"""
    t = quant_tables(quality) if qtables is None else np.asarray(qtables, np.int64).reshape(-1, 64)
    return [t[min(c, len(t) - 1)] for c in range(nc)]


def encode(img, quality=75, subsampling='420', qtables=None, ri=0):
    img = np.asarray(img)
    qt = component_tables(1 if img.ndim == 2 else 3, quality, qtables)
    samp, _, coefs = forward(img, qt, subsampling)
    return write_stream(img.shape[1], img.shape[0], samp, qt, coefs, ri)


def scan_bytes(data):
    """the entropy-coded segment and EOI: everything after the SOS header"""
    data = bytes(data)
    p = 2
    while True:
        assert data[p] == 0xFF, 'not at a marker'
        m, L = data[p + 1], data[p + 2] << 8 | data[p + 3]
        p += 2 + L
        if m == 0xDA:
            return data[p:]
