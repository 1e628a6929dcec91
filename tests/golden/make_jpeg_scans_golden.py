#!/usr/bin/env python3
"""Writes tests/golden/jpeg_scans_cases.npz: JPEG streams of more than one scan and Pillow's (libjpeg-turbo's) decode of each.

  progressive   seeded images (noise, ramps, strokes) saved by Pillow with progressive=True.  Its scan script has every kind
                of scan: DC first with Al = 1 (interleaved), AC first over bands 1-5 and 6-63 with Al = 2, two AC refinements
                (to Al 1 and 0), a DC refinement.  Grey, 4:4:4, 4:2:2, 4:2:0; 1x1 .. 96x80 and one 640x480; qualities 30 .. 100;
                optimize=True; restart intervals by blocks and by rows.
  multi-scan    sequential streams made here: the coefficients of a baseline stream Pillow wrote, coded again with the
                stream's own Huffman tables as one scan per component, or as Y and then Cb + Cr interleaved; one with DRI
                segments between its scans.  Pillow must decode each to the RGB of the stream it was made from.
  twin_<i>      for the progressive cases whose sides are multiples of 16: the baseline stream Pillow writes from the same
                image with the same settings (the coefficients are the same; Pillow's pixels are checked equal here).

Before writing, tests/jpeg_scans_ref.py must reproduce Pillow's pixels exactly on every case.  Fixed time stamps: a rerun is
byte-identical.  Keys: names (json list), jpeg_<i> (uint8 bytes), rgb_<i> (uint8 [H, W, 3]), twin_<i> (uint8 bytes, some i).
Usage: python tests/golden/make_jpeg_scans_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import jpeg_enc_ref as E  # noqa: E402
import jpeg_ref as R  # noqa: E402
import jpeg_scans_ref as S  # noqa: E402
from make_jpeg_golden import content, encode, pil_decode, write_npz  # noqa: E402


def _codes(table):
    """jpeg_ref's Huffman table -> {symbol: (code, length)}"""
    tab, vals = table
    return {vals[first + code - lo]: (code, l + 1) for l, (lo, hi, first) in enumerate(tab) if hi >= 0 for code in range(lo, hi + 1)}


def _put_block(w, blk, pred, dc, ac):
    zz = [int(x) for x in blk[R.ZIGZAG]]
    d = zz[0] - pred
    n = abs(d).bit_length()
    w.put(*dc[n])
    if n:
        w.put((d if d >= 0 else d - 1) & ((1 << n) - 1), n)
    run = 0
    for k in range(1, 64):
        x = zz[k]
        if x == 0:
            run += 1
            continue
        while run > 15:
            w.put(*ac[0xF0])
            run -= 16
        n = abs(x).bit_length()
        w.put(*ac[run << 4 | n])
        w.put((x if x >= 0 else x - 1) & ((1 << n) - 1), n)
        run = 0
    if run:
        w.put(*ac[0])
    return zz[0]


def multiscan(data, groups, dri=None):
    """the baseline stream `data` coded again as one sequential scan per group of component indices (T.81 A.2: a scan of one
    component walks its real block grid, a scan of several walks MCUs); dri: per scan a restart interval to declare in front
    of it (None: leave it as it is)"""
    h, coefs = R.entropy_decode(data)
    assert h.ri == 0
    p = 2
    while data[p + 1] != 0xDA:  # everything in front of the SOS is kept
        p += 2 + (data[p + 2] << 8 | data[p + 3])
    out, ri = bytearray(data[:p]), 0
    for g, comps in enumerate(groups):
        if dri is not None and dri[g] is not None:
            ri = dri[g]
            out += E._seg(0xDD, ri.to_bytes(2, 'big'))
        out += E._seg(0xDA, bytes([len(comps)]) + b''.join(bytes([h.comps[c][0], h.scan[c][0] << 4 | h.scan[c][1]]) for c in comps) + bytes([0, 63, 0]))
        w, pred = E._Writer(), [0] * 3
        if len(comps) == 1:
            c = comps[0]
            ux = -(-(-(-h.width * h.samp[c][0] // h.hmax)) // 8)
            units = [[(c, y * h.grid[c][1] + x)] for y in range(-(-(-(-h.height * h.samp[c][1] // h.vmax)) // 8)) for x in range(ux)]
        else:
            units = [[(c, (my * h.samp[c][1] + v) * h.grid[c][1] + mx * h.samp[c][0] + u) for c in comps for v in range(h.samp[c][1])
                      for u in range(h.samp[c][0])] for my in range(h.mcuy) for mx in range(h.mcux)]
        for i, unit in enumerate(units):
            if ri and i and i % ri == 0:
                w.flush()
                w.out += bytes([0xFF, 0xD0 + (i // ri - 1) % 8])
                pred = [0] * 3
            for c, blk in unit:
                pred[c] = _put_block(w, coefs[c][blk], pred[c], _codes(h.dc[h.scan[c][0]]), _codes(h.ac[h.scan[c][1]]))
        w.flush()
        out += w.out
    return bytes(out) + b'\xff\xd9'


def cases():
    rng = np.random.default_rng(20250311)
    out, twins = [], {}

    def prog(w, h, sub, kind, q, **kw):
        img = content(kind, rng, w, h)
        name = '%dx%d_%s_%s_q%d_prog' % (w, h, sub, kind, q) + ('_opt' if kw.get('optimize') else '') + \
            ('_rst_blocks' if 'restart_marker_blocks' in kw else '') + ('_rst_rows' if 'restart_marker_rows' in kw else '')
        out.append((name, encode(img, sub, quality=q, progressive=True, **kw)))
        if w % 16 == 0 and h % 16 == 0 and (w, h) != (640, 480):
            twins[len(out) - 1] = encode(img, sub, quality=q, **kw)

    sizes = [(1, 1), (7, 5), (8, 8), (17, 16), (33, 31), (53, 37), (96, 80)]
    subs, kinds, quals = ['grey', '444', '422', '420'], ['noise', 'ramp', 'strokes'], [30, 75, 95, 100]
    k = 0
    for w, h in sizes:
        for sub in subs:
            prog(w, h, sub, kinds[k % 3], quals[k % 4])
            k += 1
    prog(640, 480, '420', 'strokes', 50)
    prog(53, 37, '420', 'noise', 75, optimize=True)
    prog(33, 31, 'grey', 'strokes', 90, optimize=True)
    prog(96, 80, '422', 'ramp', 85, optimize=True)
    prog(53, 37, '420', 'strokes', 75, restart_marker_blocks=3)
    prog(33, 31, '444', 'noise', 60, restart_marker_blocks=1)
    prog(96, 80, '420', 'ramp', 40, restart_marker_rows=1)
    prog(53, 37, 'grey', 'noise', 95, restart_marker_rows=2)
    multi = []
    for w, h, sub, kind, q, groups, dri, tag in [
            (17, 16, '420', 'noise', 75, [[0], [1], [2]], None, 'per_component'),
            (53, 37, '422', 'strokes', 90, [[0], [1], [2]], [None, 3, 0], 'per_component_dri'),
            (33, 31, '444', 'ramp', 60, [[0], [1, 2]], None, 'y_then_cbcr'),
            (96, 80, '420', 'noise', 50, [[0], [1, 2]], [5, None], 'y_then_cbcr_dri'),
            (7, 5, '420', 'ramp', 95, [[0, 1], [2]], None, 'ycb_then_cr')]:
        base = encode(content(kind, rng, w, h), sub, quality=q)
        multi.append(('%dx%d_%s_%s_q%d_multi_%s' % (w, h, sub, kind, q, tag), multiscan(base, groups, dri), pil_decode(base)))
    return out, twins, multi


def main():
    cs, twins, multi = cases()
    names = [n for n, _ in cs] + [n for n, _, _ in multi]
    arrays = {'names': np.array(json.dumps(names))}
    for i, (name, data) in enumerate(cs + [(n, d) for n, d, _ in multi]):
        want = pil_decode(data)
        if i >= len(cs):
            assert np.array_equal(want, multi[i - len(cs)][2]), '%s: Pillow decodes the re-coded stream to other pixels' % name
        got = S.decode(data)
        assert got.shape == want.shape and np.array_equal(got, want), \
            '%s: jpeg_scans_ref differs from Pillow in %d values' % (name, int((got != want).sum()))
        arrays['jpeg_%d' % i] = np.frombuffer(data, np.uint8)
        arrays['rgb_%d' % i] = want
        if i in twins:
            assert np.array_equal(pil_decode(twins[i]), want), '%s: Pillow decodes the baseline twin to other pixels' % name
            arrays['twin_%d' % i] = np.frombuffer(twins[i], np.uint8)
    path = os.path.join(HERE, 'jpeg_scans_cases.npz')
    write_npz(path, arrays)
    print('%d cases (%d progressive, %d multi-scan, %d twins), %d bytes' % (len(names), len(cs), len(multi), len(twins), os.path.getsize(path)))
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, 'jpeg_cases.npz'))


if __name__ == '__main__':
    main()
