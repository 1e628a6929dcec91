"""GPU (-m gpu): the device half of the JPEG encode (csrc/jpeg_enc.hip jpeg_planes_kernel / jpeg_fdct_kernel through
db_text_minimal_amd.jpeg): coefficients exactly equal to the ones inside Pillow's streams (tests/golden/jpeg_encode_cases.npz),
dummy blocks included, in mixed batches, one by one and at every byte alignment; scan bytes equal to Pillow's; the round
trip through the device decoder against Pillow's decode of its own file; the input layouts, a non-default stream,
save_jpegs and the render command line.  Reads tests/golden only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from db_text_minimal_amd import (decode_coefficients, decode_jpeg, encode_jpeg, encode_jpeg_batch, entropy_decode, entropy_encode,
                                 forward_coefficients, jpeg_info, save_jpegs)
from gpu_util import DEV
from jpeg_enc_ref import scan_bytes

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_cache = {}


def golden():
    """[(case, image, Pillow's stream, Pillow's decode, its coefficients int16 [..], its tables uint16 [3, 64])], the stack split"""
    if 'g' not in _cache:
        g = np.load(os.path.join(HERE, 'golden', 'jpeg_encode_cases.npz'))
        out = []
        for i, c in enumerate(json.loads(str(g['cases']))):
            img, dec = g['img_%d' % i], g['dec_%d' % i]
            if img.ndim == 4:
                out += [[dict(c, name='%s[%d]' % (c['name'], m)), img[m], g['jpeg_%d_%d' % (i, m)].tobytes(), dec[m]] for m in range(len(img))]
            else:
                out.append([c, img, g['jpeg_%d' % i].tobytes(), dec])
        obj = entropy_decode([e[2] for e in out], pin=False)  # pinned against tests/jpeg_ref.py by tests/test_jpeg_cpu.py
        assert not obj.status.any()
        ends = list(obj.desc[1:, 0]) + [obj.coef.numel()]
        for n, e in enumerate(out):
            e += [obj.coef[int(obj.desc[n, 0]):int(ends[n])].numpy(), obj.qtabs[n]]
        _cache['g'] = [tuple(e) for e in out]
    return _cache['g']


def settings(c):
    return dict(subsampling=c['sub'] if c['sub'] != 'grey' else '420', **(dict(qtables=c['qtables']) if c['quality'] is None else dict(quality=c['quality'])))


def group_settings(ns):
    """the settings of a group's colour images (its grey ones only share the tables)"""
    cases = golden()
    return settings(cases[([n for n in ns if cases[n][1].ndim == 3] or ns)[0]][0])


def check_coefficients(obj, picks, tag):
    cases = golden()
    obj.wait()
    assert len(obj) == len(picks) and not obj.status.any() and obj.coef.dtype == torch.int16
    ends = list(obj.desc[1:, 0]) + [obj.coef.numel()]
    for k, n in enumerate(picks):
        c, img, data, _, want, qt = cases[n]
        got = obj.coef[int(obj.desc[k, 0]):int(ends[k])].numpy()
        assert got.shape == want.shape, (tag, c['name'])
        assert np.array_equal(got, want), '%s %s: %d of %d coefficients differ' % (tag, c['name'], int((got != want).sum()), want.size)
        assert np.array_equal(obj.qtabs[k], qt), (tag, c['name'])
        assert obj.shapes[k] == img.shape[:2]


def groups():
    """golden cases that one call can take together: the same tables, and one sampling among the colour images"""
    out = {}
    for n, (c, img, *_rest) in enumerate(golden()):
        out.setdefault((c['quality'], json.dumps(c['qtables'])), []).append(n)
    res = []
    for key, ns in out.items():
        greys = [n for n in ns if golden()[n][1].ndim == 2]
        subs = sorted(set(golden()[n][0]['sub'] for n in ns if golden()[n][1].ndim == 3))
        for i, sub in enumerate(subs):
            res.append([n for n in ns if golden()[n][0]['sub'] == sub] + (greys if i == 0 else []))
    assert sum(len(r) for r in res) == len(golden())
    return res


def test_mixed_batches_equal_golden_exactly():
    cases = golden()
    for ns in groups():
        obj = forward_coefficients([torch.from_numpy(cases[n][1]).to(DEV) for n in ns], **group_settings(ns))
        assert obj.coef.is_pinned()
        check_coefficients(obj, ns, 'list')
        rgb = [n for n in ns if cases[n][1].ndim == 3]
        packed = torch.from_numpy(np.concatenate([cases[n][1].reshape(-1) for n in rgb])).to(DEV)
        check_coefficients(forward_coefficients(packed, [cases[n][1].shape[:2] for n in rgb], **group_settings(rgb)), rgb, 'packed')


def test_one_by_one_equals_golden_exactly():
    for n, (c, img, *_rest) in enumerate(golden()):
        check_coefficients(forward_coefficients(torch.from_numpy(img).to(DEV), **settings(c)), [n], 'single')
        check_coefficients(forward_coefficients(img, **settings(c), device=DEV), [n], 'host array')


def test_every_alignment_of_the_first_pixel():
    cases = golden()
    for ns in groups():
        rgb = [n for n in ns if cases[n][1].ndim == 3]
        body = np.concatenate([cases[n][1].reshape(-1) for n in rgb])
        for lead in (1, 2, 3):
            buf = torch.from_numpy(np.concatenate([np.full(lead, 255, np.uint8), body])).to(DEV)
            view = buf[lead:]
            assert view.data_ptr() % 4 == lead
            check_coefficients(forward_coefficients(view, [cases[n][1].shape[:2] for n in rgb], **group_settings(rgb)), rgb, 'lead %d' % lead)


def test_scan_bytes_equal_pillows():
    cases = golden()
    seen_ri = set()
    for ns in groups():
        by_ri = {}
        for n in ns:
            by_ri.setdefault(cases[n][0]['ri'], []).append(n)
        for ri, ms in by_ri.items():
            assert ri == jpeg_info(cases[ms[0]][2])['restart_interval']
            seen_ri.add(ri)
            got = encode_jpeg_batch([cases[n][1] for n in ms], restart_interval=ri, device=DEV,
                                    **group_settings(ms))
            for n, mine in zip(ms, got):
                assert scan_bytes(mine) == scan_bytes(cases[n][2]), cases[n][0]['name']
                info = jpeg_info(mine)
                assert info['supported'] and info['restart_interval'] == ri and (info['height'], info['width']) == cases[n][1].shape[:2]
    assert len(seen_ri) == 3  # none, by blocks, by rows


def test_round_trip_equals_pillows_decode_of_its_own_file():
    for c, img, _, dec, _, _ in golden():
        back = decode_jpeg(encode_jpeg(torch.from_numpy(img).to(DEV), **settings(c)), DEV).cpu().numpy()
        want = dec if dec.ndim == 3 else np.repeat(dec[:, :, None], 3, 2)
        assert back.shape == want.shape and np.array_equal(back, want), c['name']
    # the same on the device alone: no stream in between
    n = [c['name'] for c, *_ in golden()].index('250x131_420_tiles_q75')
    c, img, _, dec, _, _ = golden()[n]
    packed, shapes = decode_coefficients(forward_coefficients(torch.from_numpy(img).to(DEV), **settings(c)), DEV)
    assert shapes == [img.shape[:2]] and np.array_equal(packed.cpu().numpy().reshape(dec.shape), dec)


def test_stacks_are_accepted():
    cases = golden()
    words = [n for n, (c, *_) in enumerate(cases) if c['name'].startswith('words_')]
    stack = torch.from_numpy(np.stack([cases[n][1] for n in words])).to(DEV)  # crop_words' [M, 32, 100, 3]
    assert stack.shape == (5, 32, 100, 3)
    check_coefficients(forward_coefficients(stack), words, 'word stack')
    for n, mine in zip(words, encode_jpeg_batch(stack)):
        assert scan_bytes(mine) == scan_bytes(cases[n][2])
    # [N, H, W] grey (probability masks after minmax_scale_u8) and [N, H, W, 3] (a render output): equal to one by one
    grey = stack[:, :, :, 1].contiguous()
    assert encode_jpeg_batch(grey, quality=90) == [encode_jpeg(g, quality=90) for g in grey]
    assert all(jpeg_info(d)['components'] == 1 for d in encode_jpeg_batch(grey))
    n = [c['name'] for c, *_ in cases].index('64x84_420_noise_q75')
    render = torch.from_numpy(np.stack([cases[n][1], cases[n][1][::-1].copy()])).to(DEV)
    got = forward_coefficients(render)
    check_coefficients(forward_coefficients(render[:1]), [n], 'render stack')
    got.wait()
    assert np.array_equal(got.coef[:got.coef.numel() // 2].numpy(), cases[n][4])
    flipped = forward_coefficients(render[1]).wait()
    assert np.array_equal(got.coef[got.coef.numel() // 2:].numpy(), flipped.coef.numpy())
    for bad in (torch.zeros(2, 3, 4, 5, dtype=torch.uint8), torch.zeros(8, 8, 3), torch.zeros(0, 8, 8, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            forward_coefficients(bad, device=DEV)
    with pytest.raises(ValueError):
        forward_coefficients(stack, subsampling='411')
    with pytest.raises(ValueError):
        forward_coefficients(stack.view(-1), [(32, 100)] * 4)


def test_non_default_stream():
    cases = golden()
    ns = max(groups(), key=len)
    imgs = [torch.from_numpy(cases[n][1]).to(DEV) for n in ns]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        obj = forward_coefficients(imgs, **group_settings(ns))
        packed, shapes = decode_coefficients(obj, DEV)
    check_coefficients(obj, ns, 'stream')
    s.synchronize()
    assert shapes == [cases[n][1].shape[:2] for n in ns]
    assert entropy_encode(obj) == encode_jpeg_batch(imgs, **group_settings(ns))


def test_save_jpegs_writes_the_bytes_of_encode_jpeg_batch(tmp_path):
    cases = golden()
    words = [n for n, (c, *_) in enumerate(cases) if c['name'].startswith('words_')]
    stack = torch.from_numpy(np.stack([cases[n][1] for n in words])).to(DEV)
    paths = [tmp_path / ('word_%d.jpg' % i) for i in range(len(words))]
    assert save_jpegs(paths, stack, quality=30, subsampling='444') == [str(p) for p in paths]
    want = encode_jpeg_batch(stack, quality=30, subsampling='444')
    assert [p.read_bytes() for p in paths] == want
    with pytest.raises(ValueError):
        save_jpegs(paths[:2], stack)


def test_render_cli_reads_and_writes_jpeg_without_pil(tmp_path):
    """python -m db_text_minimal_amd.render with a .jpg --image and a .jpg --out: the project's own decoder and encoder,
    PIL never imported (a fresh process: this one may hold PIL already)"""
    from db_text_minimal_amd import DBTextModel
    n = [c['name'] for c, *_ in golden()].index('250x131_420_tiles_q75')
    src, ckpt, out = tmp_path / 'in.jpg', tmp_path / 'model.pth', tmp_path / 'out.jpeg'
    src.write_bytes(golden()[n][2])
    torch.manual_seed(0)
    torch.save(DBTextModel().state_dict(), ckpt)
    code = ('import sys\nfrom db_text_minimal_amd import render\nrender.main(%r)\n'
            'assert not [m for m in sys.modules if m == "PIL" or m.startswith("PIL.")], "PIL was imported"\n'
            % (['--image', str(src), '--model_path', str(ckpt), '--out', str(out)], ))
    r = subprocess.run([sys.executable, '-c', code], cwd=os.path.dirname(HERE), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    data = out.read_bytes()
    info = jpeg_info(data)
    assert info['supported'] and (info['width'], info['height']) == (250, 131) and info['sampling'][0] == (2, 2)
    assert decode_jpeg(data, DEV).shape == (131, 250, 3)
