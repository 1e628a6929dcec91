#!/usr/bin/env python3
"""Writes tests/golden/jpeg_encode_cases.npz: seeded synthetic images, Pillow's (libjpeg-turbo's) baseline encoding of each
with optimize=False, and Pillow's decode of its own file.  Before writing, tests/jpeg_enc_ref.py must reproduce Pillow's
quantised coefficients (read back with jpeg_ref.entropy_decode), its quantisation tables and its scan bytes on every case.
The archive is written with fixed time stamps, so a rerun is byte-identical.

Keys: cases (json list of {name, sub, quality, qtables, ri}), img_<i> (uint8 [H, W, 3], [H, W] for grey, [M, H, W, 3] for the
stack), jpeg_<i> (uint8 bytes; jpeg_<i>_<m> for the stack), dec_<i> (Pillow's decode: the shape of img_<i>).
`quality` is null for the custom-table case, whose tables are `qtables` ([2][64], natural order); `ri` is the restart
interval in MCUs that Pillow chose for the case's restart_marker_blocks / restart_marker_rows setting.
Usage: python tests/golden/make_jpeg_encode_golden.py
"""
import io
import json
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import jpeg_enc_ref as E  # noqa: E402
import jpeg_ref as R  # noqa: E402
from make_jpeg_golden import SUBSAMPLING, content, write_npz  # noqa: E402


def pil_encode(img, sub, **kw):
    buf = io.BytesIO()
    if sub == 'grey':
        Image.fromarray(img).save(buf, 'JPEG', optimize=False, **kw)
    else:
        Image.fromarray(img).save(buf, 'JPEG', subsampling=SUBSAMPLING[sub], optimize=False, **kw)
    return buf.getvalue()


def pil_decode(data, sub):
    return np.asarray(Image.open(io.BytesIO(data)).convert('L' if sub == 'grey' else 'RGB'))


def image(kind, rng, w, h, sub):
    """content() of make_jpeg_golden.py, and 'tiles': its strokes over flat random colours in 13 x 11 tiles (hard chroma
    edges off the block grid, and an image that still compresses in the archive)"""
    if kind == 'tiles':
        y, x = np.mgrid[0:h, 0:w]
        colours = rng.integers(0, 256, (h // 11 + 1, w // 13 + 1, 3), dtype=np.uint8)
        img = np.where(content('strokes', rng, w, h) == 0, np.uint8(0), colours[y // 11, x // 13])
    else:
        img = content(kind, rng, w, h)
    return np.ascontiguousarray(img[:, :, 1]) if sub == 'grey' else img


def cases():
    """[(name, sub, quality or None, qtables or None, Pillow's restart setting, image or stack)]"""
    rng = np.random.default_rng(20240911)
    sizes = [(1, 1), (7, 5), (8, 8), (16, 16), (17, 33), (34, 18), (64, 84), (1, 20), (100, 75), (250, 131)]
    subs = ['420', '444', '422', 'grey']
    kinds = ['noise', 'ramp', 'strokes']
    quals = [10, 30, 75, 95, 100]
    out, k = [], 0
    for w, h in sizes:
        for sub in subs:
            kind, q = kinds[k % 3], quals[(k // 3 + k) % 5]
            if sub not in {(64, 84): ('420', '422'), (100, 75): ('444', 'grey'), (250, 131): ('420', )}.get((w, h), subs):
                continue  # the large sizes are not crossed with every sampling: the archive stays small
            if (w, h) == (250, 131):
                kind, q = 'tiles', 75  # noise, ramps and high qualities do not compress
            if (w, h) == (100, 75) and kind == 'noise':
                kind = 'tiles'
            out.append(('%dx%d_%s_%s_q%d' % (w, h, sub, kind, q), sub, q, None, {}, image(kind, rng, w, h, sub)))
            k += 1
    # even height under 4:2:0 at every quality: the bottom chroma block row
    for q in quals:
        out.append(('34x18_420_noise_q%d' % q, '420', q, None, {}, image('noise', rng, 34, 18, '420')))
    qt = [[int(v) for v in rng.integers(1, 64, 64)], [int(v) for v in rng.integers(1, 120, 64)]]
    out.append(('90x60_420_noise_qtables', '420', None, qt, {}, image('noise', rng, 90, 60, '420')))
    out.append(('100x75_420_strokes_q75_rst_blocks', '420', 75, None, {'restart_marker_blocks': 3}, image('strokes', rng, 100, 75, '420')))
    out.append(('100x75_422_noise_q75_rst_rows', '422', 75, None, {'restart_marker_rows': 1}, image('noise', rng, 100, 75, '422')))
    out.append(('words_5x32x100_420_strokes_q75', '420', 75, None, {}, np.stack([image('strokes', rng, 100, 32, '420') for _ in range(5)])))
    return out


def check(name, img, sub, q, qt, kw):
    """Pillow's stream for one image, after jpeg_enc_ref has reproduced its tables, coefficients and scan bytes"""
    # Pillow takes qtables in natural order and writes them in zigzag order (checked below through the parsed stream)
    data = pil_encode(img, sub, **(dict(qtables=qt) if qt is not None else dict(quality=q)), **kw)
    h, want = R.entropy_decode(data)
    tabs = E.component_tables(h.ncomp, q if q is not None else 75, qt)
    for c in range(h.ncomp):
        assert np.array_equal(h.qtabs[c], tabs[c]), '%s: table of component %d differs from Pillow\'s' % (name, c)
    samp, grids, got = E.forward(img, tabs, sub if sub != 'grey' else '444')
    assert samp == h.samp and grids == h.grid, name
    for c in range(h.ncomp):
        assert np.array_equal(got[c], want[c]), '%s: component %d differs from Pillow in %d coefficients' % (name, c, int((got[c] != want[c]).sum()))
    mine = E.write_stream(h.width, h.height, samp, tabs, got, h.ri)
    assert E.scan_bytes(mine) == E.scan_bytes(data), '%s: scan bytes differ from Pillow\'s' % name
    assert bool(kw) == bool(h.ri), name
    return data, h.ri


def main():
    arrays, meta = {}, []
    for i, (name, sub, q, qt, kw, img) in enumerate(cases()):
        arrays['img_%d' % i] = img
        if img.ndim == 4:
            datas = [check('%s[%d]' % (name, m), img[m], sub, q, qt, kw) for m in range(len(img))]
            for m, (d, _) in enumerate(datas):
                arrays['jpeg_%d_%d' % (i, m)] = np.frombuffer(d, np.uint8)
            arrays['dec_%d' % i] = np.stack([pil_decode(d, sub) for d, _ in datas])
            ri = datas[0][1]
        else:
            data, ri = check(name, img, sub, q, qt, kw)
            arrays['jpeg_%d' % i] = np.frombuffer(data, np.uint8)
            arrays['dec_%d' % i] = pil_decode(data, sub)
        meta.append(dict(name=name, sub=sub, quality=q, qtables=qt, ri=ri))
    arrays['cases'] = np.array(json.dumps(meta))
    path = os.path.join(HERE, 'jpeg_encode_cases.npz')
    write_npz(path, arrays)
    print('%d cases, %d bytes' % (len(meta), os.path.getsize(path)))


if __name__ == '__main__':
    main()
