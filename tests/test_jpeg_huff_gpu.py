"""GPU (-m gpu): Huffman coding on the device (csrc/jpeg_huff.hip through db_text_minimal_amd.jpeg entropy_encode_device and
encode_jpeg_batch(entropy='device')).  The oracle is the host coder (pinned by tests/test_jpeg_encode_cpu.py and
tests/test_jpeg_optimize_cpu.py) and Pillow's streams in tests/golden, never the device path itself: transcoding every
golden stream, with and without optimised tables, in one batch and one by one; the whole encode against entropy='host';
hand-built coefficient sets (blocks of 6 bits, ZRL runs, the longest codes, FF bytes at every kind of boundary, one-MCU
images, dummy blocks, restart intervals with RST7 -> RST0); batches that cross images, workgroups and scan chunks; errors
that fail alone; determinism.  Reads tests/golden only."""
import json
import os

import numpy as np
import pytest
import torch

from db_text_minimal_amd import (JpegCoefficients, JpegEncodeError, encode_jpeg_batch, entropy_decode, entropy_encode, entropy_encode_device,
                                 forward_coefficients, jpeg_info, quant_tables)
from db_text_minimal_amd import jpeg as J
from gpu_util import DEV
from jpeg_enc_ref import scan_bytes
from jpeg_opt_ref import dht_tables
from jpeg_ref import ZIGZAG

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_cache = {}


def streams(which):
    """[(name, restart interval, Pillow's stream)] of an archive"""
    if which not in _cache:
        g = np.load(os.path.join(HERE, 'golden', which))
        out = []
        for i, c in enumerate(json.loads(str(g['cases']))):
            if 'jpeg_%d' % i in g.files:
                out.append((c['name'], c['ri'], g['jpeg_%d' % i].tobytes()))
            else:
                out += [('%s[%d]' % (c['name'], m), c['ri'], g['jpeg_%d_%d' % (i, m)].tobytes()) for m in range(len(g['img_%d' % i]))]
        _cache[which] = out
    return _cache[which]


def by_ri(cases):
    out = {}
    for name, ri, d in cases:
        out.setdefault(ri, []).append((name, d))
    return out


def coefficients(shape, sub, blocks, quality=75):
    """a JpegCoefficients of one image (W, H, components) whose blocks (padded grid, component after component) are `blocks` [n, 64]"""
    w, h, nc = shape
    desc, qtabs, total, _, _ = J.forward_plan([(0, h, w, nc)], sub, quant_tables(quality))
    k = np.ascontiguousarray(blocks, np.int16).reshape(-1)
    assert k.size == total, (k.size, total)
    desc[:, 4] = 0
    return JpegCoefficients(torch.from_numpy(k.copy()), desc, qtabs, np.zeros(1, np.int32))


def n_blocks(shape, sub):
    return J.forward_plan([(0, shape[1], shape[0], shape[2])], sub, quant_tables(75))[2] // 64


def batch(objs):
    """several JpegCoefficients as one"""
    coef = torch.cat([o.coef for o in objs])
    desc = np.concatenate([o.desc for o in objs]).copy()
    sizes = np.array([o.coef.numel() for o in objs])
    desc[:, 0] = np.concatenate([o.desc[:, 0] + s for o, s in zip(objs, np.cumsum(sizes) - sizes)])
    desc[:, 5] = np.arange(len(desc)) * 192
    return JpegCoefficients(coef, desc, np.concatenate([o.qtabs for o in objs]), np.concatenate([o.status for o in objs]))


def same_as_host(obj, tag, ris=(0, ), optimize=(False, True)):
    for ri in ris:
        for opt in optimize:
            want = entropy_encode(obj, restart_interval=ri, optimize=opt)
            got = entropy_encode_device(obj, restart_interval=ri, optimize=opt, device=DEV)
            assert len(got) == len(want)
            for n, (a, b) in enumerate(zip(got, want)):
                assert a == b, '%s: image %d, restart interval %d, optimize %s: %d bytes against %d, first difference at %d' % (
                    tag, n, ri, opt, len(a), len(b), next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b))))
    return got


def test_transcoding_the_annex_k_golden_streams():
    for ri, group in by_ri(streams('jpeg_encode_cases.npz')).items():
        obj = entropy_decode([d for _, d in group], pin=False)
        got = same_as_host(obj, 'batch', (ri, ), (False, ))
        for (name, d), mine in zip(group, got):
            assert scan_bytes(mine) == scan_bytes(d), name
        for n, (name, d) in enumerate(group):
            one = entropy_decode([d], pin=False)
            assert entropy_encode_device(one, restart_interval=ri, device=DEV) == [got[n]], name


def test_transcoding_with_optimised_tables():
    for ri, group in by_ri(streams('jpeg_optimize_cases.npz')).items():
        obj = entropy_decode([d for _, d in group], pin=False)
        got = same_as_host(obj, 'batch', (ri, ), (True, ))
        for n, ((name, d), mine) in enumerate(zip(group, got)):
            assert scan_bytes(mine) == scan_bytes(d) and dht_tables(mine) == dht_tables(d), name
            assert entropy_encode_device(entropy_decode([d], pin=False), restart_interval=ri, optimize=True, device=DEV) == [mine], name
    # the Annex K archive's coefficients with their own tables: against the host
    for ri, group in by_ri(streams('jpeg_encode_cases.npz')).items():
        same_as_host(entropy_decode([d for _, d in group], pin=False), 'annex k archive', (ri, ), (True, ))


def test_end_to_end_equals_the_host_path_for_every_input_layout():
    g = np.load(os.path.join(HERE, 'golden', 'jpeg_encode_cases.npz'))
    cases = json.loads(str(g['cases']))
    imgs = [g['img_%d' % i] for i in range(len(cases))]
    words = next(a for a in imgs if a.ndim == 4)
    rgb = [a for a in imgs if a.ndim == 3][:8]
    grey = [a for a in imgs if a.ndim == 2][:4]
    packed = torch.from_numpy(np.concatenate([a.reshape(-1) for a in rgb])).to(DEV)
    layouts = [((rgb + grey, ), {}), (([torch.from_numpy(a).to(DEV) for a in rgb + grey], ), {}), ((packed, [a.shape[:2] for a in rgb]), {}),
               ((torch.from_numpy(words).to(DEV), ), {}), ((words[:, :, :, 1].copy(), ), {}), ((rgb[3], ), {}), ((grey[1], ), {})]
    for args, _ in layouts:
        for kw in (dict(), dict(quality=90, subsampling='444', restart_interval=2), dict(subsampling='422', optimize=True)):
            want = encode_jpeg_batch(*args, device=DEV, **kw)
            assert encode_jpeg_batch(*args, device=DEV, entropy='device', **kw) == want
    obj = forward_coefficients(torch.from_numpy(words).to(DEV), host_copy=False)
    assert obj.coef.is_cuda and obj.coef.dtype == torch.int16
    with pytest.raises(ValueError, match='entropy_encode_device'):
        entropy_encode(obj)
    assert entropy_encode_device(obj) == encode_jpeg_batch(words, device=DEV)
    with pytest.raises(ValueError):
        encode_jpeg_batch(words, device=DEV, entropy='gpu')


def test_hand_built_coefficients():
    rng = np.random.default_rng(11)
    sets = {}
    # 6 bits per block (DC 0, EOB): five blocks and more in every word
    sets['zeros'] = ((250, 131, 3), '420', np.zeros((n_blocks((250, 131, 3), '420'), 64)))
    k = np.zeros((n_blocks((64, 40, 3), '444'), 64))
    k[:, 63] = rng.integers(1, 4, len(k)) * rng.choice([-1, 1], len(k))
    sets['index 63 only'] = ((64, 40, 3), '444', k)  # three ZRL and no EOB
    k = np.full((n_blocks((48, 32, 3), '422'), 64), 1023) * rng.choice([-1, 1], (n_blocks((48, 32, 3), '422'), 64))
    k[:, 0] = 1023
    k[::2, 0] = -1024  # differences of +-2047 inside a component
    sets['longest codes'] = ((48, 32, 3), '422', k)
    for name, (shape, sub, k) in sets.items():
        same_as_host(coefficients(shape, sub, k), name, (0, 3))
    # FF bytes: Annex K luma codes 0xFFFx are runs with size 1 .. 10 from (run 1, size 10) up; a grey image of such ACs is mostly FF
    for w in (8, 16, 64, 96, 200, 520):
        nb = n_blocks((w, 64, 1), '444')
        k = np.zeros((nb, 64))
        for b in range(nb):
            at = 1
            while at < 64:
                run = 15 if b % 3 == 0 else int(rng.integers(9, 16))  # (run 15, size 10) is FFFE: fifteen ones, then ten more for +1023
                at += run
                if at < 64:
                    k[b, ZIGZAG[at]] = 1023 if b % 3 == 0 else int(rng.choice([-1, 1])) * int(rng.integers(512, 1024))
                at += 1
        obj = coefficients((w, 64, 1), '444', k)
        got = same_as_host(obj, 'FF runs %d' % w, (0, 1, 5), (False, ))
        assert scan_bytes(got[0]).count(b'\xff\x00') >= nb and (w < 64 or b'\xff\x00' * 2 in got[0])  # FF bytes in every block, and in runs
    # one-MCU images and dummy blocks; and the interval's last padded byte FF: +1023 at index 63 ends a block in ten ones, no EOB
    for shape, sub in (((8, 8, 1), '444'), ((16, 16, 3), '420'), ((16, 8, 3), '422'), ((8, 8, 3), '444'), ((7, 5, 3), '420'), ((17, 9, 3), '420')):
        nb = n_blocks(shape, sub)
        k = np.zeros((nb, 64))
        k[:, 0] = rng.integers(-1000, 1000, nb)
        k[:, 1:8] = rng.integers(-40, 40, (nb, 7))
        same_as_host(coefficients(shape, sub, k), '%s %s' % (shape, sub), (0, 1, 2, 3, 1000))
        k[:] = 0
        k[:, 0], k[:, 63] = rng.integers(-60, 60, nb), 1023
        got = same_as_host(coefficients(shape, sub, k), '%s %s pad' % (shape, sub), (0, 1), (False, ))
        assert got[0].endswith(b'\xff\x00\xff\xd9')
    # more than eight intervals: RST7 -> RST0
    nb = n_blocks((100, 75, 3), '420')
    k = rng.integers(-30, 30, (nb, 64)) * (rng.random((nb, 64)) < 0.2)
    got = same_as_host(coefficients((100, 75, 3), '420', k), 'wrap', (1, 2, 3, 7))
    assert jpeg_info(got[0])['restart_interval'] == 7


def test_batches_that_cross_images_workgroups_and_chunks():
    rng = np.random.default_rng(12)
    crops = rng.integers(0, 256, (300, 32, 100, 3), dtype=np.uint8)
    crops[:, 8:20, 10:90] = 0
    for kw in (dict(), dict(optimize=True), dict(restart_interval=4)):
        assert encode_jpeg_batch(crops, device=DEV, entropy='device', **kw) == encode_jpeg_batch(crops, device=DEV, **kw), kw
    noise = rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)
    for kw in (dict(quality=100, subsampling='444'), dict(quality=100, optimize=True), dict(quality=100, restart_interval=40)):
        assert encode_jpeg_batch(noise, device=DEV, entropy='device', **kw) == encode_jpeg_batch(noise, device=DEV, **kw), kw


def test_an_image_that_cannot_be_coded_fails_alone():
    group = by_ri(streams('jpeg_encode_cases.npz'))[0][:12]
    obj = entropy_decode([d for _, d in group], pin=False)
    o = JpegCoefficients(obj.coef.clone(), obj.desc.copy(), obj.qtabs.copy(), obj.status.copy())
    o.coef[int(o.desc[3, 0]) + 5] = 1024
    o.coef[int(o.desc[7, 0])] = 2048
    o.coef[int(o.desc[9, 0]) + 64 + 9] = -1024   # an AC error in the second block ...
    o.coef[int(o.desc[9, 0]) + 128] = 30000      # ... in front of a DC error in the third: the first in scan order decides
    o.qtabs[5, 0, 3] = 256
    o.status[0] = 2
    for opt in (False, True):
        want, werrs = entropy_encode(o, errors='report', optimize=opt)
        got, gerrs = entropy_encode_device(o, errors='report', optimize=opt, device=DEV)
        assert got == want
        assert [(e.index, e.code, e.reason, str(e)) if e else None for e in gerrs] == [(e.index, e.code, e.reason, str(e)) if e else None for e in werrs]
        assert [e.code if e else 0 for e in gerrs] == [1, 0, 0, 5, 0, 3, 0, 4, 0, 5, 0, 0]
        with pytest.raises(JpegEncodeError, match='image 0'):
            entropy_encode_device(o, optimize=opt, device=DEV)
    for bad in (-1, 65536, 1.5):
        with pytest.raises(ValueError):
            entropy_encode_device(obj, restart_interval=bad, device=DEV)


def test_determinism_and_a_non_default_stream():
    group = by_ri(streams('jpeg_encode_cases.npz'))[0]
    obj = entropy_decode([d for _, d in group], pin=False)
    want = entropy_encode(obj, restart_interval=2, optimize=True)
    for _ in range(3):
        assert entropy_encode_device(obj, restart_interval=2, optimize=True, device=DEV) == want
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        assert entropy_encode_device(obj, restart_interval=2, optimize=True, device=DEV) == want
        assert entropy_encode_device(obj, device=DEV) == entropy_encode(obj)
    s.synchronize()
