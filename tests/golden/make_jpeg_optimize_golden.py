#!/usr/bin/env python3
"""Writes tests/golden/jpeg_optimize_cases.npz: seeded synthetic images and Pillow's (libjpeg-turbo's) baseline encoding of
each with optimize=True.  Before writing, tests/jpeg_opt_ref.py must reproduce every DHT segment and the whole stream's scan
bytes from tests/jpeg_enc_ref.py's coefficients.  The archive is written with fixed time stamps: a rerun is byte-identical.

Keys: cases (json list of {name, sub, quality, ri}), img_<i> (uint8 [H, W, 3], [H, W] for grey), jpeg_<i> (uint8 bytes).
Usage: python tests/golden/make_jpeg_optimize_golden.py
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
import jpeg_opt_ref as O  # noqa: E402
import jpeg_ref as R  # noqa: E402
from make_jpeg_encode_golden import image  # noqa: E402
from make_jpeg_golden import SUBSAMPLING, write_npz  # noqa: E402


def cases():
    rng = np.random.default_rng(20241017)
    out = []
    sizes = [(1, 1), (7, 5), (8, 8), (17, 9), (16, 16), (33, 17), (61, 40), (100, 32), (100, 75)]
    subs, kinds, quals = ['420', '444', '422', 'grey'], ['strokes', 'ramp', 'noise', 'tiles'], [30, 50, 75, 90, 95]
    for k, (w, h) in enumerate(sizes):
        for sub in (subs[k % 4], subs[(k + 1) % 4]):
            kind, q = kinds[len(out) % 4], quals[len(out) % 5]
            out.append(('%dx%d_%s_%s_q%d' % (w, h, sub, kind, q), sub, q, {}, image(kind, rng, w, h, sub)))
    out.append(('24x24_420_constant_q75', '420', 75, {}, np.full((24, 24, 3), 117, np.uint8)))
    out.append(('40x24_444_noise_q100', '444', 100, {}, image('noise', rng, 40, 24, '444')))
    out.append(('100x75_420_strokes_q75_rst_blocks', '420', 75, {'restart_marker_blocks': 3}, image('strokes', rng, 100, 75, '420')))
    out.append(('100x75_422_tiles_q75_rst_rows', '422', 75, {'restart_marker_rows': 1}, image('tiles', rng, 100, 75, '422')))
    out.append(('70x90_grey_ramp_q95_rst_blocks', 'grey', 95, {'restart_marker_blocks': 11}, image('ramp', rng, 70, 90, 'grey')))
    return out


def check(name, img, sub, q, kw):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, 'JPEG', quality=q, optimize=True, **({} if sub == 'grey' else dict(subsampling=SUBSAMPLING[sub])), **kw)
    data = buf.getvalue()
    h, _ = R.entropy_decode(data)
    tabs = E.component_tables(h.ncomp, q, None)
    samp, _, coefs = E.forward(img, tabs, sub if sub != 'grey' else '444')
    hist = O.histograms(h.width, h.height, samp, coefs, h.ri)
    theirs = O.dht_tables(data)
    assert len(theirs) == (2 if sub == 'grey' else 4), name
    for (tc, th), t in theirs.items():
        counts, syms = O.optimal_table(hist[2 * th + tc])
        assert (counts, syms) == t, '%s: table %d/%d differs from Pillow\'s' % (name, tc, th)
    mine = O.write_stream(h.width, h.height, samp, tabs, coefs, h.ri)
    assert E.scan_bytes(mine) == E.scan_bytes(data), '%s: scan bytes differ from Pillow\'s' % name
    assert bool(kw) == bool(h.ri), name
    return data, h.ri


def main():
    arrays, meta = {}, []
    for i, (name, sub, q, kw, img) in enumerate(cases()):
        data, ri = check(name, img, sub, q, kw)
        arrays['img_%d' % i], arrays['jpeg_%d' % i] = img, np.frombuffer(data, np.uint8)
        meta.append(dict(name=name, sub=sub, quality=q, ri=ri))
    arrays['cases'] = np.array(json.dumps(meta))
    path = os.path.join(HERE, 'jpeg_optimize_cases.npz')
    write_npz(path, arrays)
    print('%d cases, %d bytes' % (len(meta), os.path.getsize(path)))


if __name__ == '__main__':
    main()
