"""Streams for the tests of the device Huffman decoder (tests/test_jpeg_dhuff_cpu.py, tests/test_jpeg_dhuff_gpu.py): the golden
archives, and hand-built coefficient sets coded by the host coder entropy_encode (pinned against Pillow by
tests/test_jpeg_encode_cpu.py), so that the bytes are known-good and the lengths are known by construction."""
import json
import os

import numpy as np
import torch

from db_text_minimal_amd import JpegCoefficients, entropy_decode, entropy_encode, jpeg_info, quant_tables
from db_text_minimal_amd import jpeg as J
from jpeg_dhuff_ref import S, W

HERE = os.path.dirname(os.path.abspath(__file__))
ARCHIVES = ('jpeg_cases.npz', 'jpeg_encode_cases.npz', 'jpeg_optimize_cases.npz')
_cache = {}


def golden_streams():
    """[(name, stream)] of the three archives"""
    if 'golden' not in _cache:
        out = []
        for a in ARCHIVES:
            g = np.load(os.path.join(HERE, 'golden', a))
            out += [('%s:%s' % (a, k), g[k].tobytes()) for k in g.files if k.startswith('jpeg_')]
        _cache['golden'] = out
    return _cache['golden']


def golden_pixels():
    """[(stream, rgb)] of jpeg_cases.npz"""
    g = np.load(os.path.join(HERE, 'golden', ARCHIVES[0]))
    return [(g['jpeg_%d' % i].tobytes(), g['rgb_%d' % i]) for i in range(len(json.loads(str(g['names']))))]


def coefficients(shape, sub, blocks):
    """a JpegCoefficients of one image (W, H, components) whose blocks (padded grid, component after component) are `blocks` [n, 64]"""
    w, h, nc = shape
    desc, qtabs, total, _, _ = J.forward_plan([(0, h, w, nc)], sub, quant_tables(75))
    k = np.ascontiguousarray(blocks, np.int16).reshape(-1)
    assert k.size == total, (k.size, total)
    desc[:, 4] = 0
    return JpegCoefficients(torch.from_numpy(k.copy()), desc, qtabs, np.zeros(1, np.int32))


def grey(bw, bh, blocks, **kw):
    """the stream of a grey image of bw x bh blocks"""
    return entropy_encode(coefficients((8 * bw, 8 * bh, 1), '444', blocks), **kw)[0]


def dc_only(diffs):
    """blocks [n, 64] that are only a DC value, with the given differences: 0 codes in 6 bits with the Annex K tables (00 +
    EOB 1010), +-1 in 8 (010 x 1010), +-2 / +-3 in 9 (011 xx 1010)"""
    b = np.zeros((len(diffs), 64), np.int16)
    b[:, 0] = np.cumsum(diffs)
    return b


def exact_bits(n_bits):
    """170 blocks (17 x 10) of a grey image whose scan is exactly n_bits bits before padding: S - 1, S or S + 1"""
    nine, eight = n_bits & 1, 0
    while (n_bits - 9 * nine - 8 * eight) % 6 or (n_bits - 9 * nine - 8 * eight) // 6 + nine + eight != 170:
        eight += 1
        assert eight < 170
    six = 170 - nine - eight
    diffs = [2] * nine + [1, -1] * (eight // 2) + [1] * (eight % 2) + [0] * six
    assert 9 * nine + 8 * eight + 6 * six == n_bits
    return grey(17, 10, dc_only(diffs))


def dense_blocks(n, rng):
    """n blocks of 63 coefficients of 10 bits each (codes of 16 bits + 10): 1658 bits a block, more than a subsequence"""
    b = rng.integers(512, 1024, (n, 64)) * rng.choice([-1, 1], (n, 64))
    b[:, 0] = np.cumsum(rng.integers(-1000, 1000, n)) % 900
    return b.astype(np.int16)


def scan_of(data):
    """(first byte of the entropy data, the stream's bytes)"""
    d = bytes(data)
    p = 2
    while d[p + 1] != 0xDA:
        p += 2 + (d[p + 2] << 8 | d[p + 3])
    return p + 2 + (d[p + 2] << 8 | d[p + 3]), d


def ff_positions(data):
    """offsets within the scan of every FF that is followed by 00"""
    p, d = scan_of(data)
    a = np.frombuffer(d, np.uint8)[p:]
    return np.nonzero((a[:-1] == 0xFF) & (a[1:] == 0))[0]


def stuffing_streams(limit=4000):
    """dense grey streams, searched over seeds with the host coder, that between them carry an FF as the last byte of a
    dword, of a subsequence and of a workgroup's span (with its 00 behind the boundary), and two FF 00 in a row"""
    if 'stuff' in _cache:
        return _cache['stuff']
    need = {'dword': lambda p: (p % 4 == 3).any(), 'subsequence': lambda p: (p % (S // 8) == S // 8 - 1).any(),
            'span': lambda p: (p == W * S // 8 - 1).any(), 'run': lambda p: (np.diff(p) == 2).any()}
    found = {}
    for seed in list(STUFF_SEEDS) + list(range(limit)):
        rng = np.random.default_rng(seed)
        blocks = np.concatenate([dense_blocks(170, rng), np.zeros((30, 64), np.int16)])
        d = grey(20, 10, blocks)
        p = ff_positions(d)
        for k, f in need.items():
            if k not in found and f(p):
                found[k] = (seed, d)
        if len(found) == len(need):
            break
    assert len(found) == len(need), sorted(found)
    _cache['stuff'] = found
    return found


STUFF_SEEDS = (0, 11)  # where the search ends today; it goes on from 0 if the coder or the sets change


def hand_built():
    """[(name, stream)]: subsequence edges, block counts 0 and > 128 per subsequence, restart intervals, samplings, tables"""
    if 'hand' in _cache:
        return _cache['hand']
    rng = np.random.default_rng(26)
    out = [('short', grey(5, 2, dc_only([0] * 10))), ('S bits', exact_bits(S)), ('S - 1 bits', exact_bits(S - 1)), ('S + 1 bits', exact_bits(S + 1)),
           ('4000 EOB blocks', grey(80, 50, dc_only([0] * 4000))), ('dense blocks', grey(6, 4, dense_blocks(24, rng))),
           ('dense then EOB', grey(80, 50, np.concatenate([dense_blocks(40, rng), dc_only([0] * 3960)])))]
    out += [('FF at %s end (seed %d)' % (k, s), d) for k, (s, d) in sorted(stuffing_streams().items())]
    # restart intervals over golden images of every sampling, Annex K and optimised tables
    picked = {}
    for name, d in golden_streams():
        i = jpeg_info(d)
        key = tuple(i['sampling'])
        if i['width'] * i['height'] >= 32 * 32 and (key not in picked or i['width'] * i['height'] > picked[key][1]):
            picked[key] = (d, i['width'] * i['height'], i)
    assert len(picked) == 4, sorted(picked)
    for key, (d, _, i) in sorted(picked.items()):
        obj = entropy_decode([d], pin=False)
        mcux = int(obj.desc[0, 20])
        for ri, opt in ((1, False), (mcux, True), (3, False)):
            out.append(('%s ri %d%s' % (key, ri, ' optimised' if opt else ''), entropy_encode(obj, restart_interval=ri, optimize=opt)[0]))
    out.append(('SOF1, four tables', four_tables(picked[((2, 2), (1, 1), (1, 1))][0])))
    _cache['hand'] = out
    return out


def four_tables(data):
    """a YCbCr stream rewritten as SOF1 with Huffman tables 0 .. 3 of both classes: Cb uses 2, Cr uses 3 (copies of table 1)"""
    from test_jpeg_cpu import patch_sof, segments
    d = bytes(patch_sof(data, marker=0xC1))
    extra = b''
    for m, a, e in segments(d):
        if m == 0xC4:
            q = a + 4
            while q < e:
                n = 17 + sum(d[q + 1:q + 17])
                if d[q] & 15 == 1:
                    for i in (2, 3):
                        t = bytes([d[q] & 0xF0 | i]) + d[q + 1:q + n]
                        extra += b'\xff\xc4' + (len(t) + 2).to_bytes(2, 'big') + t
                q += n
    m, a, e = segments(d)[-1]
    sos = bytearray(d[a:e])
    assert sos[4] == 3
    sos[8], sos[10] = 0x22, 0x33
    return d[:a] + extra + bytes(sos) + d[e:]


def host_coefs(datas):
    return entropy_decode(list(datas), pin=False)
