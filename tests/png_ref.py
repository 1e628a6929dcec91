"""numpy restatement of what db_text_minimal_amd.png computes (shares no code with it): chunk parsing with CRCs, inflate, the
five scanline filters, Adam7, the conversion to cv2.imread's IMREAD_COLOR pixels (as RGB), and the writer: the encoder's filter
choice and the file.  Slow and plain; tests/test_png_cpu.py pins it against Pillow (tests/golden/png_cases.npz).

  parse(data)            -> dict(width, height, depth, ctype, interlace, palette uint8 [n, 3], idat bytes)
  scanlines(data)        -> (dict, the inflated, still filtered bytes, cut to what IHDR implies)
  decode(data)           -> uint8 [H, W, 3]
  filter_rows(x, filter) -> uint8 [H, 1 + W * C]: the filtered rows, type bytes included ('adaptive' or 0 .. 4)
  encode(x, level, filter) -> bytes (IHDR, one IDAT, IEND)
"""
import struct
import zlib

import numpy as np

SIGNATURE = b'\x89PNG\r\n\x1a\n'
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}
# Adam7: (x0, y0, dx, dy) of passes 1 .. 7
ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))


class RefCorrupt(Exception):
    pass


class RefRefused(Exception):
    pass


def parse(data):
    data = bytes(data)
    if data[:8] != SIGNATURE:
        raise RefCorrupt('signature')
    pos, hdr, pal, idat, end = 8, None, np.zeros((0, 3), np.uint8), [], False
    while pos < len(data):
        if pos + 12 > len(data):
            raise RefCorrupt('chunk header past the end')
        n, kind = struct.unpack('>I4s', data[pos:pos + 8])
        if pos + 12 + n > len(data):
            raise RefCorrupt('chunk past the end')
        body = data[pos + 8:pos + 8 + n]
        if struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])[0] != (zlib.crc32(kind + body) & 0xFFFFFFFF):
            raise RefCorrupt('crc of ' + repr(kind))
        pos += 12 + n
        if kind == b'CgBI':
            raise RefRefused('CgBI')
        if hdr is None and kind != b'IHDR':
            raise RefCorrupt('IHDR is not first')
        if kind == b'IHDR':
            if n != 13 or hdr is not None:
                raise RefCorrupt('IHDR')
            hdr = struct.unpack('>IIBBBBB', body)
        elif kind == b'PLTE':
            if n % 3 or not 3 <= n <= 768:
                raise RefCorrupt('PLTE')
            pal = np.frombuffer(body, np.uint8).reshape(-1, 3).copy()
        elif kind == b'IDAT':
            idat.append(body)
        elif kind == b'IEND':
            end = True
            break
    if hdr is None or not end:
        raise RefCorrupt('IHDR or IEND missing')
    w, h, depth, ctype, comp, flt, lace = hdr
    if w == 0 or h == 0 or ctype not in DEPTHS or depth not in DEPTHS[ctype] or comp or flt or lace > 1:
        raise RefCorrupt('IHDR values')
    if not idat or (ctype == 3 and not len(pal)):
        raise RefCorrupt('IDAT or PLTE missing')
    return dict(width=w, height=h, depth=depth, ctype=ctype, interlace=lace, palette=pal, idat=b''.join(idat))


def passes(p):
    """[(x0, y0, dx, dy, pass width, pass height)] of the sub-images that hold bytes"""
    w, h = p['width'], p['height']
    if not p['interlace']:
        return [(0, 0, 1, 1, w, h)]
    out = []
    for x0, y0, dx, dy in ADAM7:
        pw, ph = (w - x0 + dx - 1) // dx, (h - y0 + dy - 1) // dy
        if pw > 0 and ph > 0:
            out.append((x0, y0, dx, dy, pw, ph))
    return out


def row_bytes(p, pw):
    return (pw * p['depth'] * CHANNELS[p['ctype']] + 7) // 8


def raw_size(p):
    return sum(ph * (1 + row_bytes(p, pw)) for _, _, _, _, pw, ph in passes(p))


def scanlines(data):
    p = parse(data)
    need = raw_size(p)
    try:
        raw = zlib.decompressobj().decompress(p['idat'], need)
    except zlib.error:
        raise RefCorrupt('zlib')
    if len(raw) < need:
        raise RefCorrupt('short data')
    raw = np.frombuffer(raw, np.uint8)
    o = 0
    for _, _, _, _, pw, ph in passes(p):
        rb = row_bytes(p, pw)
        if raw[o:o + ph * (rb + 1)].reshape(ph, rb + 1)[:, 0].max() > 4:
            raise RefCorrupt('filter type')
        o += ph * (rb + 1)
    return p, raw


def paeth(a, b, c):
    pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def unfilter(rows, bpp):
    """uint8 [H, 1 + rb] filtered rows -> uint8 [H, rb]; along anti-diagonals of (row, pixel), every row's own type"""
    H, rb = rows.shape[0], rows.shape[1] - 1
    ft = rows[:, 0].astype(np.int64)
    F = rows[:, 1:].astype(np.int64)
    npx = (rb + bpp - 1) // bpp
    P = np.zeros((H + 1, (npx + 1) * bpp), np.int64)  # P[r + 1, x + bpp] is byte x of row r; zeros above and to the left
    Fp = np.zeros((H, npx * bpp), np.int64)
    Fp[:, :rb] = F
    j = np.arange(bpp)[None, :]
    for t in range(npx + H - 1):
        r = np.arange(max(0, t - npx + 1), min(H - 1, t) + 1)
        x = (t - r)[:, None] * bpp + j
        R = r[:, None]
        a, b, c = P[R + 1, x], P[R, x + bpp], P[R, x]
        f = ft[r][:, None]
        pred = np.select([f == 0, f == 1, f == 2, f == 3], [0 * a, a, b, (a + b) // 2], paeth(a, b, c))
        P[R + 1, x + bpp] = (Fp[R, x] + pred) & 255
    return P[1:, bpp:bpp + rb].astype(np.uint8)


def samples(p, raw_rows, pw):
    """uint8 [ph, rb] unfiltered bytes -> int [ph, pw, channels] samples (16-bit: the high byte)"""
    depth, ch = p['depth'], CHANNELS[p['ctype']]
    if depth == 8:
        return raw_rows.reshape(raw_rows.shape[0], pw, ch).astype(np.int64)
    if depth == 16:
        return raw_rows.reshape(raw_rows.shape[0], pw, ch, 2)[..., 0].astype(np.int64)
    bits = np.unpackbits(raw_rows, axis=1)[:, :pw * depth].reshape(raw_rows.shape[0], pw, depth).astype(np.int64)
    return (bits * (1 << np.arange(depth - 1, -1, -1))).sum(2)[..., None]


def to_rgb(p, s):
    """samples [h, w, channels] -> uint8 [h, w, 3] by cv2.imread's rule"""
    ct = p['ctype']
    if ct == 3:
        pal = np.zeros((256, 3), np.uint8)
        pal[:len(p['palette'])] = p['palette']
        return pal[s[..., 0]]
    if ct in (0, 4):
        g = s[..., 0] * (255 // ((1 << p['depth']) - 1)) if p['depth'] < 8 else s[..., 0]
        return np.repeat(g[..., None], 3, 2).astype(np.uint8)
    return s[..., :3].astype(np.uint8)


def decode(data):
    p, raw = scanlines(data)
    bpp = max(1, p['depth'] * CHANNELS[p['ctype']] // 8)
    out = np.zeros((p['height'], p['width'], 3), np.uint8)
    o = 0
    for x0, y0, dx, dy, pw, ph in passes(p):
        rb = row_bytes(p, pw)
        rows = raw[o:o + ph * (rb + 1)].reshape(ph, rb + 1)
        o += ph * (rb + 1)
        out[y0::dy, x0::dx] = to_rgb(p, samples(p, unfilter(rows, bpp), pw))
    return out


# ---- writer ------------------------------------------------------------------------------------------------------------
def _rows(x):
    x = np.asarray(x)
    assert x.dtype == np.uint8 and (x.ndim == 2 or (x.ndim == 3 and x.shape[2] == 3))
    return x.reshape(x.shape[0], -1).astype(np.int64), (1 if x.ndim == 2 else 3)


def filter_rows(x, filter='adaptive'):
    raw, bpp = _rows(x)
    H, rb = raw.shape
    cur = np.zeros((H + 1, rb + bpp), np.int64)
    cur[1:, bpp:] = raw
    x_, a, b, c = cur[1:, bpp:], cur[1:, :-bpp], cur[:-1, bpp:], cur[:-1, :-bpp]
    five = np.stack([x_, x_ - a, x_ - b, x_ - (a + b) // 2, x_ - paeth(a, b, c)]) & 255  # [5, H, rb]
    if filter == 'adaptive':
        score = np.minimum(five, 256 - five).sum(2)  # [5, H]
        pick = np.argmin(score, axis=0)  # the first of equal scores: the lowest type
    else:
        assert filter in (0, 1, 2, 3, 4)
        pick = np.full(H, filter)
    out = np.zeros((H, rb + 1), np.uint8)
    out[:, 0] = pick
    out[:, 1:] = five[pick, np.arange(H)]
    return out


def chunk(kind, body):
    return struct.pack('>I', len(body)) + kind + body + struct.pack('>I', zlib.crc32(kind + body) & 0xFFFFFFFF)


def encode(x, level=6, filter='adaptive'):
    x = np.asarray(x)
    rows = filter_rows(x, filter)
    ihdr = struct.pack('>IIBBBBB', x.shape[1], x.shape[0], 8, 0 if x.ndim == 2 else 2, 0, 0, 0)
    return SIGNATURE + chunk(b'IHDR', ihdr) + chunk(b'IDAT', zlib.compress(rows.tobytes(), level)) + chunk(b'IEND', b'')
