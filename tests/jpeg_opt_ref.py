"""A plain restatement of libjpeg's optimised Huffman tables (jchuff.c: the gather pass of optimize_coding and
jpeg_gen_optimal_table), beside tests/jpeg_enc_ref.py, which writes the streams.  It is what the host table builder and
both Huffman coders are tested against, and is itself pinned against Pillow's optimize=True by
tests/golden/make_jpeg_optimize_golden.py and tests/test_jpeg_optimize_cpu.py.

  optimal_table(freq)                              -> (counts per code length 1 .. 16, symbols by length then value)
  histograms(W, H, samp, coefs, ri)                -> int [4, 256]: DC 0, AC 0, DC 1, AC 1 (zeros for a grey image's 2 and 3)
  write_stream(W, H, samp, qtabs, coefs, ri)       -> bytes, with the image's own tables
  dht_tables(data)                                 -> {(class, id): (counts, symbols)} of a stream's DHT segments
"""
import numpy as np

import jpeg_enc_ref as E
from jpeg_ref import ZIGZAG


def optimal_table(freq):
    freq = [int(v) for v in freq] + [1]  # the pseudo-symbol 256 keeps the all-ones code unused
    assert len(freq) == 257
    codesize, others = [0] * 257, [-1] * 257
    while True:
        c1, v = -1, None
        for i in range(257):
            if freq[i] and (v is None or freq[i] <= v):
                v, c1 = freq[i], i
        c2, v = -1, None
        for i in range(257):
            if freq[i] and i != c1 and (v is None or freq[i] <= v):
                v, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    bits = [0] * 33
    for i in range(257):
        if codesize[i]:
            assert codesize[i] <= 32, 'libjpeg gives up'
            bits[codesize[i]] += 1
    for i in range(32, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    syms = [j for l in range(1, 33) for j in range(256) if codesize[j] == l]
    return bits[1:17], syms


def histograms(W, H, samp, coefs, ri=0):
    nc = len(samp)
    mcux, mcuy, grids, _ = E.geometry(W, H, samp)
    hist = np.zeros((4, 256), np.int64)
    pred = [0] * nc
    for mcu in range(mcux * mcuy):
        if ri and mcu and mcu % ri == 0:
            pred = [0] * nc
        my, mx = divmod(mcu, mcux)
        for c in range(nc):
            hh, vv = samp[c]
            t = 2 if c else 0
            for v in range(vv):
                for u in range(hh):
                    zz = [int(x) for x in coefs[c][(my * vv + v) * grids[c][1] + mx * hh + u][ZIGZAG]]
                    d = zz[0] - pred[c]
                    pred[c] = zz[0]
                    hist[t, abs(d).bit_length()] += 1
                    run = 0
                    for k in range(1, 64):
                        if zz[k] == 0:
                            run += 1
                            continue
                        while run > 15:
                            hist[t + 1, 0xF0] += 1
                            run -= 16
                        hist[t + 1, run << 4 | abs(zz[k]).bit_length()] += 1
                        run = 0
                    if run:
                        hist[t + 1, 0] += 1
    return hist


def write_stream(W, H, samp, qtabs, coefs, ri=0):
    """jpeg_enc_ref.write_stream with the image's own tables in the place of the Annex K ones"""
    hist = histograms(W, H, samp, coefs, ri)
    own = [optimal_table(hist[t]) for t in range(4 if len(samp) == 3 else 2)]
    own += own[:2] if len(own) == 2 else []
    names = ('DC_LUMA', 'AC_LUMA', 'DC_CHROMA', 'AC_CHROMA')
    saved = [getattr(E, n) for n in names]
    try:
        for n, t in zip(names, own):
            setattr(E, n, t)
        return E.write_stream(W, H, samp, qtabs, coefs, ri)
    finally:
        for n, t in zip(names, saved):
            setattr(E, n, t)


def dht_tables(data):
    data, p, out = bytes(data), 2, {}
    while True:
        assert data[p] == 0xFF
        m, L = data[p + 1], data[p + 2] << 8 | data[p + 3]
        seg = data[p + 4:p + 2 + L]
        p += 2 + L
        if m == 0xC4:
            q = 0
            while q < len(seg):
                counts = list(seg[q + 1:q + 17])
                n = sum(counts)
                out[(seg[q] >> 4, seg[q] & 15)] = (counts, list(seg[q + 17:q + 17 + n]))
                q += 17 + n
        if m == 0xDA:
            return out
