"""CPU (-m "not gpu"): the cases of tests/test_wgrad_fp64_gpu.py (conv_ref.WGRAD_SPLIT_CASES, WGRAD_PATCH_CASES) reach the kernels, split
counts and reduction forms their comments name — asked of the library's own host-only plan functions (dbn_wgrad_kernel_config_hw,
dbn_wgrad_tile_config, dbn_wgrad_splitk_hw, dbn_wgrad_reduce_describe: no device call, nothing is launched), so that a change of the
plan which moves a case off its path fails HERE and the list is repaired, instead of the GPU pins quietly testing less.

The only arithmetic restated from csrc/wgrad.hip (wgrad_run) is what no entry point reports: the pixels per split,
pchunk = ceil(P / splits) rounded up to 16, and for the pixel-patch kernel the patches per split, ceil(patches / splits)."""
import ctypes

import pytest

import conv_ref as R
from db_text_minimal_amd import _lib

DBN_OK, DBN_ERR_ARG = 0, 1
# mode -> (at, ns) of dbn_wgrad_t: the activation type of dY and X, the matrix math
MODES = {'f32': (0, 0), 'bf16x3': (0, 3), 'bf16': (0, 1), 'bf16 storage': (1, 1)}
TILE = {'64x192': 1, '128x128': 2, '64x128': 3, '64x64': 4}  # dbn_wgrad_tile_config
BN = {1: 192, 2: 128, 3: 128, 4: 64}
TR, PATCH = 16, 32  # bits of dbn_wgrad_kernel_config_hw: wgrad_tr_kernel, wgrad_patch_kernel
FAKE = 64  # a non-null pointer: dbn_wgrad_reduce_describe records it and dereferences nothing

# case -> (P, splits, pchunk, tile, G); G None: no 64-channel reduction form (wgrad_reduce_kernel)
SPLIT_PLAN = {
    (3, 64, 64, 3, 1, 1, 40, 36): (4320, 9, 480, '64x192', 2),
    (2, 64, 64, 3, 1, 1, 37, 59): (4366, 9, 496, '64x192', 2),
    (2, 32, 64, 3, 1, 1, 37, 41): (3034, 6, 512, '64x128', None),
    (2, 96, 64, 3, 1, 1, 37, 41): (3034, 6, 512, '64x128', None),
    (1, 64, 128, 3, 2, 1, 97, 83): (2058, 5, 416, '128x128', 1),
    (2, 64, 128, 1, 2, 0, 90, 94): (4230, 9, 480, '64x64', 2),
    (4, 128, 64, 1, 1, 0, 45, 47): (8460, 17, 512, '64x128', 4),
    (2, 64, 64, 2, 2, 0, 100, 96): (4800, 10, 480, '64x128', 2),
    (2, 64, 64, 4, 2, 1, 90, 94): (4230, 9, 480, '64x128', 2),
    (2, 3, 64, 7, 2, 3, 97, 99): (4900, 10, 496, '64x128', None),
}
# case -> (patches, splits, patches per split, splits that hold patches, G)
PATCH_PLAN = {
    (2, 64, 64, 3, 1, 1, 48, 48): (72, 9, 8, 9, 2),
    (3, 64, 64, 3, 1, 1, 44, 48): (99, 13, 8, 13, 3),
    (2, 64, 192, 3, 1, 1, 36, 32): (36, 5, 8, 5, 1),
    (2, 128, 64, 3, 1, 1, 36, 32): (36, 5, 8, 5, 1),
    (1, 256, 256, 3, 1, 1, 60, 240): (225, 28, 9, 25, 7),
}
ALL_CASES = R.WGRAD_SPLIT_CASES + R.WGRAD_PATCH_CASES


def L():
    return _lib.lib()


def cb_of(ci, at):
    """Stored channels of X: fp32 tensors pad to 4, bf16 storage to 16 (the stem)."""
    return (ci + 3) // 4 * 4 if at == 0 else (ci + 15) // 16 * 16


def plan(case, mode):
    """What the library says one dbn_wgrad_t call of this case does."""
    N, Ci, Co, k, s, p, H, W = case
    at, ns = MODES[mode]
    Cb = cb_of(Ci, at)
    Ho, Wo = R.out_size(H, k, s, p), R.out_size(W, k, s, p)
    P, J = N * Ho * Wo, k * k * Cb
    cfg = L().dbn_wgrad_kernel_config_hw(at, ns, Co, Cb, k, k, s, p, Ho, Wo, H, W)
    tile = L().dbn_wgrad_tile_config(Co, J)
    splits = L().dbn_wgrad_splitk_hw(N, Ho, Wo, Co, H, W, Cb, k, k)
    job = _lib.WgradReduceJob()
    rc = L().dbn_wgrad_reduce_describe(at, ns, FAKE, FAKE, FAKE, FAKE, N, Ho, Wo, Co, H, W, Cb, Ci, k, k, s, p, 1.0, ctypes.byref(job))
    d = dict(case=case, mode=mode, Cb=Cb, P=P, J=J, cfg=cfg, tile=tile, splits=splits, rc=rc, job=job, patch=bool(cfg & PATCH), tr=bool(cfg & TR),
             pchunk=(-(-P // splits) + 15) // 16 * 16, Jp=J if cfg & PATCH else -(-J // BN[tile]) * BN[tile])
    if cfg & PATCH:
        d['patches'] = N * (H // 4) * (W // 16)
        d['per_split'] = -(-d['patches'] // splits)
        d['used'] = -(-d['patches'] // d['per_split'])
    return d


def test_the_tables_cover_the_lists():
    assert list(SPLIT_PLAN) == R.WGRAD_SPLIT_CASES, 'SPLIT_PLAN does not list conv_ref.WGRAD_SPLIT_CASES case by case'
    assert list(PATCH_PLAN) == R.WGRAD_PATCH_CASES, 'PATCH_PLAN does not list conv_ref.WGRAD_PATCH_CASES case by case'


def expected(case):
    table = SPLIT_PLAN if case in R.WGRAD_SPLIT_CASES else PATCH_PLAN
    assert case in table, 'the plan tables of this module do not list %s' % (case, )
    return table[case]


@pytest.mark.parametrize('case', R.WGRAD_PATCH_CASES)
def test_patch_cases_reach_the_pixel_patch_kernel(case):
    """wgrad_patch_kernel<1,1>, <1,0> and <3,0>; exact fp32 math has no patch form."""
    for mode in ('bf16 storage', 'bf16', 'bf16x3'):
        d = plan(case, mode)
        assert d['patch'], 'wgrad_patch_kernel lost: %s in mode %s runs kernel config %d' % (case, mode, d['cfg'])
    assert not plan(case, 'f32')['patch'], case
    patches, splits, per_split, used, G = expected(case)
    for mode in MODES:
        d = plan(case, mode)
        assert d['splits'] == splits, 'split count of %s in mode %s: %d, not %d' % (case, mode, d['splits'], splits)
        if d['patch']:
            got = (d['patches'], d['per_split'], d['used'])
            assert got == (patches, per_split, used), 'patch ranges of %s in mode %s: %s, not %s' % (case, mode, got, (patches, per_split, used))


@pytest.mark.parametrize('case', R.WGRAD_SPLIT_CASES)
def test_split_cases_reach_their_matrix_kernel_and_split_count(case):
    N, Ci, Co, k, s, p, H, W = case
    P, splits, pchunk, tile, _ = expected(case)
    for mode in MODES:
        d = plan(case, mode)
        assert not d['patch'], 'a split case took the pixel-patch kernel: %s in mode %s' % (case, mode)
        got = (d['P'], d['splits'], d['pchunk'], d['tile'])
        assert got == (P, splits, pchunk, TILE[tile]), 'pixel splits / tile of %s in mode %s: %s, not %s' % (case, mode, got, (P, splits, pchunk, TILE[tile]))
        assert d['splits'] >= 2 and (d['splits'] - 1) * d['pchunk'] < P, 'every split of %s holds pixels' % (case, )
    d = plan(case, 'bf16 storage')
    if d['Cb'] % 32 == 0:
        assert d['tr'], 'wgrad_tr_kernel lost: %s on bf16 storage runs kernel config %d' % (case, d['cfg'])
    else:  # the stem on 16-channel bf16 input: the register-transposing kernel with AT = 1
        assert Ci == 3 and d['Cb'] == 16 and not d['tr'], 'the bf16-storage stem left the register-transposing kernel: config %d' % d['cfg']
    assert not any(plan(case, mode)['tr'] for mode in ('f32', 'bf16x3', 'bf16')), case


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('case', ALL_CASES)
def test_reduction_form(case, mode):
    """dbn_wgrad_reduce_describe: wgrad_reduce64_kernel's job (splits, thread groups, slab order, row length) where X has a multiple
    of 64 channels, DBN_ERR_ARG where it has not (Cb = 32, Cb = 96, the stem: wgrad_reduce_kernel)."""
    d = plan(case, mode)
    job = d['job']
    G = expected(case)[4]
    if d['Cb'] % 64:
        assert G is None and d['rc'] == DBN_ERR_ARG, 'describe of %s (Cb = %d) returned %d' % (case, d['Cb'], d['rc'])
        return
    assert d['rc'] == DBN_OK, (case, mode, d['rc'])
    assert (job.splitk, job.G) == (d['splits'], G), 'reduction of %s in mode %s: %d splits in G = %d groups, not %d in %d' % (
        case, mode, job.splitk, job.G, d['splits'], G)
    # natural (o, j) slabs from wgrad_tr_kernel and wgrad_patch_kernel, position space from the register-transposing kernel
    assert job.natural == int(d['patch'] or d['tr']), (case, mode, job.natural)
    assert (job.J, job.Jp) == (d['J'], d['Jp']), (case, mode, job.J, job.Jp, d['J'], d['Jp'])
    assert (job.O, job.Cb, job.I, job.RS, job.blocks) == (case[2], d['Cb'], case[1], case[3]**2, case[2] * (d['Cb'] // 64)), (case, mode)
    assert job.smem_bytes <= 64 * 1024 and job.scale == 1.0


def test_every_path_occurs():
    """Conditions on the lists, not measurements: each path the GPU pins are there for is taken by at least one case."""
    plans = [plan(c, m) for c in ALL_CASES for m in MODES]
    ok = [d for d in plans if d['rc'] == DBN_OK]
    assert any(d['job'].G >= 2 for d in ok), 'no case folds thread groups in the reduction (G >= 2)'
    assert {d['job'].G for d in ok} >= {1, 2, 3, 4, 7} and {d['job'].RS for d in ok} == {1, 4, 9, 16}, 'the grouped reduction mixes fewer forms'
    assert {d['job'].natural for d in ok} == {0, 1}
    assert any(d['tr'] and d['pchunk'] % 32 == 16 for d in plans), 'no wgrad_tr_kernel case ends a split inside a 32-pixel LDS stage'
    assert any(d['P'] % 16 for d in plans), 'no case ends its last split inside a k-step (P % 16 != 0)'
    assert any(d['job'].Jp > d['job'].J for d in ok), 'no case with padded slab columns in the 64-channel reduction (Jp > J)'
    assert any(d['Jp'] > d['J'] and d['Cb'] % 64 for d in plans), 'no case with padded slab columns in wgrad_reduce_kernel'
    assert any(d['patch'] and d['used'] < d['splits'] for d in plans), 'no pixel-patch case with a split past the last patch (zero slab)'
    assert any(d['patch'] and d['patches'] % d['per_split'] for d in plans), 'no pixel-patch case whose last used split is partial'
    assert {d['tile'] for d in plans if d['tr']} == {1, 2, 3, 4}, 'wgrad_tr_kernel is not reached in all four tiles'
    assert any(d['cfg'] & 64 for d in plans) and any(not d['cfg'] & 64 and d['mode'] == 'f32' for d in plans), 'block-wise and general gather of the fp32 kernel'


@pytest.mark.parametrize('case', ALL_CASES)
def test_the_exact_data_is_representable_and_sums_exactly(case):
    """Dense operands on {-4..4} / 4 and impulses 1, -2, 1 / 2 are bf16 values; every product is a multiple of 2^-4 of magnitude <= 2,
    so every partial sum over at most P pixels is a multiple of 2^-4 of magnitude <= 2 P < 2^20: 24 bits hold it, it is exact in fp32
    in any order, and so is the result scaled by 1 or 1 / 2."""
    import torch
    N, Ci, Co, k, s, p, H, W = case
    Ho, Wo = R.out_size(H, k, s, p), R.out_size(W, k, s, p)
    assert N * Ho * Wo * 16 < 2**24 and 2 * N * Ho * Wo * 16 < 2**24
    x, dy = R.dense_x((N, Ci, H, W), 11), R.dense_x((N, Co, Ho, Wo), 14)
    (sdy, ) = R.impulse_maps(N, Co, Ho, Wo, R.seam_pixels(N, Ho, Wo, Ho, Wo, 1, tile_rows=16), 0)
    (sx, ) = R.impulse_maps(N, Ci, H, W, R.wgrad_x_seams(case), 0)
    for t in (x, dy, sdy, sx):
        assert R.representable(t, torch.bfloat16) and float(t.abs().max()) <= 2
    pts = set(R.wgrad_x_seams(case))
    assert {(n, h, w) for n in range(N) for h in (0, H - 1) for w in (0, W - 1)} <= pts
    if case in R.WGRAD_PATCH_CASES:
        assert {(N - 1, h, w) for h in (3, 4) for w in (15, 16)} <= pts and (0, H - 5, W - 17) in pts
