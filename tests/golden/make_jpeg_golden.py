#!/usr/bin/env python3
"""Writes tests/golden/jpeg_cases.npz: JPEG byte strings encoded by Pillow (libjpeg-turbo) from seeded synthetic images, and
Pillow's own decode of each (RGB; grey through convert('RGB')), plus one byte-only fixture per refused kind.  Before
writing, tests/jpeg_ref.py must reproduce Pillow's pixels exactly on every case.  The archive is written with fixed
time stamps, so a rerun is byte-identical.

Keys: names (json list), jpeg_<i> (uint8 bytes), rgb_<i> (uint8 [H, W, 3]), refused_progressive, refused_cmyk (uint8 bytes).
Usage: python tests/golden/make_jpeg_golden.py
"""
import io
import json
import os
import sys
import zipfile

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_ref as R  # noqa: E402

SUBSAMPLING = {'444': 0, '422': 1, '420': 2}


def content(kind, rng, w, h):
    """uint8 [h, w, 3]: noise (drives the clamps), smooth ramps, or hard black-on-white strokes"""
    y, x = np.mgrid[0:h, 0:w]
    if kind == 'noise':
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == 'ramp':
        a = rng.uniform(0.2, 2.0, 6)
        return np.stack([(x * a[0] + y * a[1]) % 256, 255 - (x * a[2] + y * a[3]) % 256, (x * a[4] * 0.5 + y * a[5] * 2) % 256],
                        -1).astype(np.uint8)
    img = np.full((h, w, 3), 255, np.uint8)
    for _ in range(max(2, (w * h) // 900)):
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        if rng.random() < 0.5:
            img[y0:y0 + int(rng.integers(1, 4)), x0:x0 + int(rng.integers(3, 40))] = 0
        else:
            img[y0:y0 + int(rng.integers(3, 24)), x0:x0 + int(rng.integers(1, 4))] = 0
    d = (x - y + int(rng.integers(0, 50))) % 61
    img[d < 2] = 0
    return img


def encode(img, sub, **kw):
    buf = io.BytesIO()
    if sub == 'grey':
        Image.fromarray(img[:, :, 1]).save(buf, 'JPEG', **kw)
    else:
        Image.fromarray(img).save(buf, 'JPEG', subsampling=SUBSAMPLING[sub], **kw)
    return buf.getvalue()


def pil_decode(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))


def cases():
    rng = np.random.default_rng(20240607)
    sizes = [(1, 1), (7, 5), (8, 8), (17, 33), (100, 75), (250, 131)]
    subs = ['444', '422', '420', 'grey']
    kinds = ['noise', 'ramp', 'strokes']
    quals = [30, 75, 95, 100]
    out, k = [], 0
    for w, h in sizes:
        for sub in subs:
            kind, q = kinds[k % 3], quals[(k // 3 + k) % 4]
            if (w, h) == (250, 131) and kind == 'noise' and sub != '420':
                kind = 'strokes'  # noise does not compress: one large noise case is enough
            out.append(('%dx%d_%s_%s_q%d' % (w, h, sub, kind, q), encode(content(kind, rng, w, h), sub, quality=q)))
            k += 1
    # every quality on noise (clamps) and on strokes, 4:2:0 and 4:4:4
    for q in quals:
        out.append(('40x24_420_noise_q%d' % q, encode(content('noise', rng, 40, 24), '420', quality=q)))
        out.append(('33x17_444_noise_q%d' % q, encode(content('noise', rng, 33, 17), '444', quality=q)))
        out.append(('61x40_422_strokes_q%d' % q, encode(content('strokes', rng, 61, 40), '422', quality=q)))
    # around 640 x 480
    out.append(('640x480_420_strokes_q75', encode(content('strokes', rng, 640, 480), '420', quality=75)))
    out.append(('637x479_422_strokes_q30', encode(content('strokes', rng, 637, 479), '422', quality=30)))
    # optimised Huffman tables, custom quantisation tables, restart markers
    out.append(('100x75_420_ramp_q75_opt', encode(content('ramp', rng, 100, 75), '420', quality=75, optimize=True)))
    out.append(('100x75_444_noise_q95_opt', encode(content('noise', rng, 100, 75), '444', quality=95, optimize=True)))
    out.append(('50x70_grey_strokes_q30_opt', encode(content('strokes', rng, 50, 70), 'grey', quality=30, optimize=True)))
    qt = [[int(v) for v in rng.integers(1, 64, 64)], [int(v) for v in rng.integers(1, 120, 64)]]
    out.append(('90x60_420_noise_qtables', encode(content('noise', rng, 90, 60), '420', qtables=qt)))
    out.append(('90x60_444_ramp_qtables', encode(content('ramp', rng, 90, 60), '444', qtables=qt)))
    out.append(('100x75_420_strokes_q75_rst_blocks', encode(content('strokes', rng, 100, 75), '420', quality=75, restart_marker_blocks=3)))
    out.append(('100x75_422_noise_q75_rst_rows', encode(content('noise', rng, 100, 75), '422', quality=75, restart_marker_rows=1)))
    out.append(('70x90_grey_ramp_q95_rst_blocks', encode(content('ramp', rng, 70, 90), 'grey', quality=95, restart_marker_blocks=11)))
    out.append(('120x40_444_strokes_q100_rst_rows', encode(content('strokes', rng, 120, 40), '444', quality=100, restart_marker_rows=2)))
    refused = {}
    buf = io.BytesIO()
    Image.fromarray(content('ramp', rng, 24, 16)).save(buf, 'JPEG', quality=75, progressive=True)
    refused['refused_progressive'] = buf.getvalue()
    buf = io.BytesIO()
    Image.fromarray(content('ramp', rng, 24, 16)).convert('CMYK').save(buf, 'JPEG', quality=75)
    refused['refused_cmyk'] = buf.getvalue()
    return out, refused


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
    cs, refused = cases()
    arrays = {'names': np.array(json.dumps([n for n, _ in cs]))}
    for i, (name, data) in enumerate(cs):
        want = pil_decode(data)
        got = R.decode(data)
        assert got.shape == want.shape and np.array_equal(got, want), \
            '%s: jpeg_ref differs from Pillow in %d values' % (name, int((got != want).sum()))
        arrays['jpeg_%d' % i] = np.frombuffer(data, np.uint8)
        arrays['rgb_%d' % i] = want
    for k, v in refused.items():
        arrays[k] = np.frombuffer(v, np.uint8)
    path = os.path.join(HERE, 'jpeg_cases.npz')
    write_npz(path, arrays)
    print('%d cases, %d bytes' % (len(cs), os.path.getsize(path)))


if __name__ == '__main__':
    main()
