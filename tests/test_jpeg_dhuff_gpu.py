"""GPU (-m gpu): Huffman decoding on the device (csrc/jpeg_dhuff.hip through db_text_minimal_amd.jpeg entropy_decode_device and
decode_jpeg_batch(entropy='device')).  The oracle is the host decoder entropy_decode (pinned by tests/test_jpeg_cpu.py), the
golden pixels and the restatement's account of which images need the host (tests/jpeg_dhuff_ref.py), never the device
path itself.  Every comparison is exact.  Golden streams in one mixed batch and one by one; subsequence edges (fewer than
S bits, S - 1, S, S + 1, more than 128 blocks in a subsequence, blocks that span three, both in one image); FF at the end
of a dword, a subsequence and a workgroup's span, FF 00 runs; restart intervals of one MCU, one MCU row and more than
eight, every sampling, optimised tables, SOF1 with four tables; 1 x 1 beside 640 x 480; determinism; the fallback with
too few rounds and with damaged members; 200 corruptions and 200 truncations of three short streams between guard words;
the loader pipeline.  Reads tests/golden only."""
import numpy as np
import pytest
import torch

import jpeg_dhuff_cases as C
import jpeg_dhuff_ref as D
from db_text_minimal_amd import (DeviceBatches, decode_jpeg, decode_jpeg_batch, entropy_decode, entropy_decode_device, jpeg_collate, jpeg_stream_collate,
                                 parse_streams)
from db_text_minimal_amd import jpeg as J
from gpu_util import DEV

pytestmark = pytest.mark.gpu


def same_as_host(datas, tag, max_rounds=None, host=None):
    want = entropy_decode(datas, pin=False) if host is None else host
    got = entropy_decode_device(datas, DEV, max_rounds)
    assert got.coef.is_cuda and got.coef.dtype == torch.int16 and got.coef.numel() == want.coef.numel(), tag
    assert (got.status == want.status).all() and (got.desc == want.desc).all() and (got.qtabs == want.qtabs).all(), tag
    diff = (got.coef.cpu() != want.coef).nonzero()
    assert diff.numel() == 0, '%s: %d coefficients differ, the first at %d' % (tag, len(diff), int(diff[0]))
    return got


def mixed():
    return [d for _, d in C.golden_streams()]


def test_golden_streams_as_one_batch():
    got = same_as_host(mixed(), 'mixed batch')
    assert got.host_decoded.dtype == bool and not got.host_decoded.any()


def test_golden_streams_one_by_one_and_their_pixels():
    for name, d in C.golden_streams():
        assert not same_as_host([d], name).host_decoded.any(), name
    pairs = C.golden_pixels()
    packed, shapes = decode_jpeg_batch([d for d, _ in pairs], DEV, entropy='device')
    flat = packed.cpu().numpy()
    o = 0
    for (h, w), (_, rgb) in zip(shapes, pairs):
        assert (flat[o:o + h * w * 3].reshape(h, w, 3) == rgb).all()
        o += h * w * 3
    d, rgb = max(pairs, key=lambda p: p[1].size)
    assert (decode_jpeg(d, DEV, entropy='device').cpu().numpy() == rgb).all()


def test_hand_built_streams():
    cases = C.hand_built()
    st = parse_streams([d for _, d in cases], pin=False)
    bits = dict(zip([n for n, _ in cases], [int((st.segments[st.segments[:, 0] == i, 2] - st.segments[st.segments[:, 0] == i, 1]).sum()) * 8
                                            for i in range(len(cases))]))
    assert bits['short'] < D.S and bits['S bits'] == D.S == bits['S - 1 bits'] and bits['S + 1 bits'] == D.S + 8  # padded to bytes
    assert max(J.jpeg_info(d)['restart_interval'] and st.info[i, 5] for i, (_, d) in enumerate(cases)) > 8
    for name, d in cases:
        assert not same_as_host([d], name).host_decoded.any(), name
    got = same_as_host([d for _, d in cases], 'hand-built batch')
    assert not got.host_decoded.any()


def test_sizes_side_by_side_and_determinism():
    g = sorted(C.golden_streams(), key=lambda nd: len(nd[1]))
    datas = [g[0][1], g[-1][1], g[1][1], C.hand_built()[4][1], g[-2][1], g[0][1], g[2][1]]
    shapes = entropy_decode(datas, pin=False).shapes
    assert (1, 1) in shapes and (480, 640) in shapes
    a = same_as_host(datas, 'seven images')
    b = entropy_decode_device(parse_streams(datas), DEV)
    assert torch.equal(a.coef, b.coef) and not a.host_decoded.any() and not b.host_decoded.any()


@pytest.mark.parametrize('rounds', [0, 1])
def test_too_few_rounds_fall_back_exactly_where_the_restatement_says(rounds):
    datas = mixed() + [d for _, d in C.hand_built()[:8]]
    got = same_as_host(datas, 'max_rounds=%d' % rounds, rounds)
    want = np.array([D.decode(d, rounds).host for d in datas])
    assert want.any() and not want.all()
    assert (got.host_decoded == want).all(), (np.nonzero(got.host_decoded)[0], np.nonzero(want)[0])


def damaged(d, at=None):
    p, _ = C.scan_of(d)
    b = bytearray(d)
    b[p + (len(d) - p) // 2 if at is None else at] ^= 0x5A
    return bytes(b)


def test_damaged_members_fail_alone():
    g = [d for _, d in C.golden_streams()]
    progressive = bytes(__import__('test_jpeg_cpu').patch_sof(g[5], marker=0xC2))
    datas = [g[10], g[20][:len(g[20]) * 2 // 3], g[11], progressive, damaged(g[30]), g[12]]
    host = entropy_decode(datas, pin=False)
    assert host.status[1] != 0 and host.status[3] == 3 and (host.status[[0, 2, 5]] == 0).all()
    got = same_as_host(datas, 'damaged members', host=host)
    assert got.host_decoded[1] and not got.host_decoded[[0, 2, 3, 5]].any()
    assert got.host_decoded[4] or host.status[4] == 0
    for n in np.nonzero(host.status != 0)[0]:
        o, e = int(host.desc[n, 0]), int(host.desc[n + 1, 0]) if n + 1 < len(datas) else host.coef.numel()
        assert not got.coef[o:e].any()
    packed, shapes, errs = decode_jpeg_batch(datas, DEV, errors='report', entropy='device')
    want = decode_jpeg_batch(datas, DEV, errors='report')
    assert torch.equal(packed, want[0]) and shapes == want[1] and [type(e) for e in errs] == [type(e) for e in want[2]]


def test_corruptions_and_truncations_between_guard_words():
    short = sorted((d for _, d in C.golden_streams()), key=len)
    short = [d for d in short if J.jpeg_info(d)['width'] > 8][:3]
    for d in short:
        p, _ = C.scan_of(d)
        n = len(d) - p
        cases = [damaged(d, p + (k * 7919) % n) for k in range(200)] + [d[:p + (k * n) // 200] for k in range(200)]
        host = entropy_decode(cases, pin=False)
        st = parse_streams(cases)
        guard, words = 1024, J.dhuff_workspace_bytes(st)
        coef = torch.full((st.coef_elems + 2 * guard, ), 0x5A5A, dtype=torch.int16, device=DEV)
        ws = torch.full((words + 2 * guard * 8, ), 0x5A, dtype=torch.uint8, device=DEV)
        res = J._dhuff_launch(st, torch.device(DEV), J.DHUFF_ROUNDS, coef[guard:guard + st.coef_elems], ws[guard * 8:guard * 8 + words]).cpu().numpy()
        assert (coef[:guard] == 0x5A5A).all() and (coef[guard + st.coef_elems:] == 0x5A5A).all(), 'a kernel wrote outside the coefficient buffer'
        assert (ws[:guard * 8] == 0x5A).all() and (ws[guard * 8 + words:] == 0x5A).all(), 'a kernel wrote outside the workspace'
        clean = (res[0] == -1) & (res[-1] == 0) & ~st.host_only
        # what the device took for good is good, bit for bit; everything else is the host decoder's
        got = coef[guard:guard + st.coef_elems].cpu()
        for i in np.nonzero(clean)[0]:
            o, e = int(host.desc[i, 0]), int(host.desc[i + 1, 0]) if i + 1 < len(cases) else host.coef.numel()
            assert host.status[i] == 0 and torch.equal(got[o:e], host.coef[o:e]), i
        assert clean.any() and not clean.all()
        same_as_host(cases, 'damaged streams', host=host)


class _Items(torch.utils.data.Dataset):
    def __init__(self, datas):
        self.datas = datas

    def __len__(self):
        return len(self.datas)

    def __getitem__(self, i):
        return self.datas[i], [np.array([[2., 2.], [30., 2.], [30., 20.], [2., 20.]])], ['word']


def test_device_batches_over_both_collates():
    datas = [d for d, rgb in C.golden_pixels() if rgb.shape[0] >= 32 and rgb.shape[1] >= 32][:4]
    outs = []
    for collate in (jpeg_collate, jpeg_stream_collate):
        loader = torch.utils.data.DataLoader(_Items(datas), batch_size=4, collate_fn=collate, num_workers=0)
        outs.append(list(DeviceBatches(loader, DEV, training=False, size=64)))
    assert len(outs[0]) == len(outs[1]) == 1
    for k, v in outs[0][0].items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, outs[1][0][k]), k
