#!/usr/bin/env python3
"""Writes tests/golden/png_cases.npz: PNG byte strings and the pixels Pillow decodes from each (Image.open(...).convert('RGB');
for 16-bit grey without alpha, where Pillow clips instead of taking the high byte, np.asarray(im) >> 8 of its raw I;16 image),
plus byte-only fixtures of refused and corrupt files.  Most files come from the small writer below, which forces every row's
filter type (Pillow never picks Average and cannot write Adam7); the rest from Pillow's own save.  Before writing,
tests/png_ref.py must reproduce every case exactly.  The archive is written with fixed time stamps: a rerun gives the same bytes.

Keys: names (json list), png_<i> (uint8 bytes), rgb_<i> (uint8 [H, W, 3]), refused_<kind>, corrupt_<kind> (uint8 bytes).
Usage: python tests/golden/make_png_golden.py
"""
import io
import json
import os
import struct
import sys
import zipfile
import zlib

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import png_ref  # noqa: E402

SIG = b'\x89PNG\r\n\x1a\n'
CH = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
PAIRS = [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16), (6, 8), (6, 16)]
CYCLE = [4, 3, 1, 2, 0, 4, 4, 3, 3]
ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))


def chunk(kind, body=b''):
    return struct.pack('>I', len(body)) + kind + body + struct.pack('>I', zlib.crc32(kind + body) & 0xFFFFFFFF)


def content(kind, rng, w, h, ch, depth):
    """int [h, w, ch] samples in 0 .. 2^depth - 1"""
    top = (1 << depth) - 1
    if kind == 'noise':
        return rng.randint(0, top + 1, size=(h, w, ch)).astype(np.int64)
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(ch), indexing='ij')
    v = (x * 3 + y * 2 + c * 61 + (x * y) // 37) & 255  # a ramp with a slow ripple
    if kind == 'strokes':  # a plain ramp under the strokes: the large cases stay small in the archive
        v = (x + y // 2 + c * 61) & 255
        v = np.where(((x // 9 + y // 5) % 7 == 0) | ((x - y) % 53 < 3), 255 - v, v)
    if depth == 16:
        return (v << 8) | ((x * 7 + y * 13 + c) & 255)
    return v >> (8 - depth)


def pack_rows(s, depth):
    """samples [h, w, ch] -> uint8 [h, rb]"""
    h = s.shape[0]
    if depth == 8:
        return s.reshape(h, -1).astype(np.uint8)
    if depth == 16:
        return np.stack([s >> 8, s & 255], -1).reshape(h, -1).astype(np.uint8)
    bits = (s.reshape(h, -1, 1) >> np.arange(depth - 1, -1, -1)) & 1
    return np.packbits(bits.reshape(h, -1).astype(np.uint8), axis=1)


def forward(raw, bpp, types):
    """uint8 [h, rb] -> filtered bytes with the type byte of types[row] in front of each row"""
    h, rb = raw.shape
    cur = np.zeros((h + 1, rb + bpp), np.int64)
    cur[1:, bpp:] = raw
    x, a, b, c = cur[1:, bpp:], cur[1:, :-bpp], cur[:-1, bpp:], cur[:-1, :-bpp]
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    pth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    five = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - pth]) & 255
    out = np.zeros((h, rb + 1), np.uint8)
    out[:, 0] = types
    out[:, 1:] = five[np.asarray(types), np.arange(h)]
    return out.tobytes()


def write_png(s, ctype, depth, types=CYCLE, interlace=0, palette=None, before=(), split=None, between=None, level=6):
    """samples [h, w, ch] -> a PNG file.  types: the filter cycle over the rows of every (sub-)image.  before: chunks between
    IHDR and the first IDAT.  split: the IDAT payload cut into that many chunks ('bytes': one per byte); between: a chunk put
    after the first IDAT."""
    h, w = s.shape[:2]
    bpp = max(1, depth * CH[ctype] // 8)
    subs = [s] if not interlace else [s[y0::dy, x0::dx] for x0, y0, dx, dy in ADAM7]
    raw = b''
    for sub in subs:
        if sub.shape[0] and sub.shape[1]:
            raw += forward(pack_rows(sub, depth), bpp, [types[r % len(types)] for r in range(sub.shape[0])])
    z = zlib.compress(raw, level)
    n = 1 if split is None else len(z) if split == 'bytes' else split
    cuts = [len(z) * i // n for i in range(n + 1)]
    idats = [chunk(b'IDAT', z[cuts[i]:cuts[i + 1]]) for i in range(n)]
    if between is not None:
        idats.insert(1, between)
    out = SIG + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, depth, ctype, 0, 0, interlace))
    if palette is not None:
        out += chunk(b'PLTE', np.asarray(palette, np.uint8).tobytes())
    return out + b''.join(before) + b''.join(idats) + chunk(b'IEND')


def pillow_rgb(data):
    im = Image.open(io.BytesIO(data))
    if im.mode.startswith('I;16') or im.mode == 'I':
        g = (np.asarray(im).astype(np.int64) >> 8).astype(np.uint8)
        return np.ascontiguousarray(np.repeat(g[..., None], 3, 2))
    return np.ascontiguousarray(np.asarray(im.convert('RGB')))


def pal_for(rng, n):
    return rng.randint(0, 256, size=(n, 3)).astype(np.uint8)


def cases():
    rng = np.random.RandomState(20260)
    out = []

    def add(name, ctype, depth, w, h, kind=None, **kw):
        kind = kind or ('noise' if w * h <= 17 * 33 else 'ramp')
        s = content(kind, rng, w, h, CH[ctype], depth)
        if ctype == 3 and 'palette' not in kw:
            kw['palette'] = pal_for(rng, 1 << depth)
        out.append((name, write_png(s, ctype, depth, **kw)))

    for ct, d in PAIRS:  # every valid pair
        add('pair_ct%d_d%d_17x33' % (ct, d), ct, d, 17, 33)
    for fam, (ct, d) in (('sub', (0, 4)), ('b8', (2, 8)), ('b16', (6, 16))):  # sizes, per pixel family
        for w, h in ((1, 1), (1, 7), (7, 1), (5, 3), (17, 33), (100, 75)):
            add('size_%s_%dx%d' % (fam, w, h), ct, d, w, h)
    for t in range(5):  # band and chunk edges
        add('band_5x2100_f%d' % t, 2, 8, 5, 2100, 'ramp', types=[t])
    add('band_5x2100_cycle', 2, 8, 5, 2100, 'ramp')
    for w in (1, 2, 15, 16, 17, 63, 64, 65, 257, 1030):
        add('chunk_%dx6' % w, 2, 8, w, 6, 'noise' if w <= 65 else 'strokes')
    add('chunk_2100x9', 2, 8, 2100, 9, 'strokes')
    for w, h in ((1, 1), (2, 2), (3, 5), (8, 8), (13, 10), (100, 75)):  # Adam7
        for tag, (ct, d) in (('grey2', (0, 2)), ('pal4', (3, 4)), ('rgb8', (2, 8)), ('rgba16', (6, 16))):
            add('adam7_%s_%dx%d' % (tag, w, h), ct, d, w, h, interlace=1)
    # container
    add('idat_1_chunk', 2, 8, 17, 9, split=1)
    add('idat_3_chunks', 2, 8, 17, 9, split=3)
    add('idat_byte_chunks', 2, 8, 17, 9, split='bytes')
    add('pal2_trns', 3, 2, 17, 9, before=[chunk(b'tRNS', bytes([0, 128, 255]))])
    add('rgb8_trns', 2, 8, 17, 9, before=[chunk(b'tRNS', bytes([0, 7, 0, 9, 0, 200]))])
    text = [chunk(b'gAMA', struct.pack('>I', 45455)), chunk(b'tEXt', b'Comment\x00made for a test'), chunk(b'pHYs', struct.pack('>IIB', 2835, 2835, 1))]
    add('ancillary_before', 2, 8, 17, 9, before=text)
    add('ancillary_between', 2, 8, 17, 9, before=text[:1], split=3, between=chunk(b'teSt', b'between the data'))
    s = content('noise', rng, 17, 9, 1, 4)
    out.append(('short_plte', write_png(s, 3, 4, palette=pal_for(rng, 5))))
    # Pillow's own files
    rgb = content('ramp', rng, 100, 75, 3, 8).astype(np.uint8)
    modes = {'RGB': Image.fromarray(rgb), 'L': Image.fromarray(rgb[..., 0]), 'P': Image.fromarray(rgb).quantize(64),
             '1': Image.fromarray(((rgb[..., 0] >> 4) & 1).astype(np.uint8) * 255).convert('1'),
             'LA': Image.fromarray(np.ascontiguousarray(rgb[..., :2]), 'LA'),
             'RGBA': Image.fromarray(np.concatenate([rgb, rgb[..., :1] ^ 255], 2))}
    for m, im in modes.items():
        buf = io.BytesIO()
        im.save(buf, 'PNG')
        out.append(('pillow_%s_100x75' % m, buf.getvalue()))
    for w, h in ((640, 480), (637, 479)):
        buf = io.BytesIO()
        Image.fromarray(content('strokes', rng, w, h, 3, 8).astype(np.uint8)).save(buf, 'PNG')
        out.append(('pillow_RGB_%dx%d_strokes' % (w, h), buf.getvalue()))
    return out


def bad_files():
    rng = np.random.RandomState(7)
    s = content('noise', rng, 17, 9, 3, 8)
    good = write_png(s, 2, 8)
    ihdr_end = 8 + 25
    out = {'refused_cgbi': good[:8] + chunk(b'CgBI', b'\x50\x00\x20\x02') + good[8:]}
    flipped = bytearray(good)
    flipped[-13] ^= 1  # the last byte of the IDAT's CRC
    out['corrupt_crc'] = bytes(flipped)
    out['corrupt_truncated_idat'] = good[:ihdr_end + 8 + 20]
    raw = bytearray(forward(pack_rows(s, 8), 3, [1] * 9))
    raw[4 * (17 * 3 + 1)] = 5
    out['corrupt_filter5'] = SIG + chunk(b'IHDR', struct.pack('>IIBBBBB', 17, 9, 8, 2, 0, 0, 0)) + chunk(b'IDAT', zlib.compress(bytes(raw))) + chunk(b'IEND')
    out['corrupt_zero_width'] = SIG + chunk(b'IHDR', struct.pack('>IIBBBBB', 0, 9, 8, 2, 0, 0, 0)) + good[ihdr_end:]
    out['corrupt_depth3'] = SIG + chunk(b'IHDR', struct.pack('>IIBBBBB', 17, 9, 3, 2, 0, 0, 0)) + good[ihdr_end:]
    out['corrupt_no_iend'] = good[:-12]
    return out


def write_npz(path, arrays):
    """np.savez_compressed with fixed time stamps (a rerun gives the same bytes)"""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    cs = cases()
    arrays = {'names': np.array(json.dumps([n for n, _ in cs]))}
    for i, (name, data) in enumerate(cs):
        if name == 'ancillary_between':  # Pillow stops reading at a chunk between IDATs: the pixels are those of the file without it
            want = png_ref.decode(data)
            i0 = data.index(b'teSt') - 4
            assert np.array_equal(pillow_rgb(data[:i0] + data[i0 + 12 + 16:]), want)
        else:
            want = pillow_rgb(data)
        got = png_ref.decode(data)
        assert got.shape == want.shape and np.array_equal(got, want), '%s: png_ref differs from Pillow in %d values' % (name, int((got != want).sum()))
        arrays['png_%d' % i] = np.frombuffer(data, np.uint8)
        arrays['rgb_%d' % i] = want
    for k, v in bad_files().items():
        try:
            png_ref.decode(v)
        except (png_ref.RefRefused if k.startswith('refused') else png_ref.RefCorrupt):
            pass
        else:
            raise AssertionError('%s decodes' % k)
        arrays[k] = np.frombuffer(v, np.uint8)
    path = os.path.join(HERE, 'png_cases.npz')
    write_npz(path, arrays)
    print('%s: %d cases, %d bytes' % (path, len(cs), os.path.getsize(path)))


if __name__ == '__main__':
    main()
