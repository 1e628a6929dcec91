"""CPU (-m "not gpu"): the cases of tests/test_winograd_fp64_gpu.py (conv_ref.WINO_WGRAD_PLAN, WINO_FWD_PLAN, IGEMM_FINAL_PLAN) reach the
forms, group counts, split counts and reduction kernels their tables name — asked of the library's own host-only plan functions
(dbn_winograd_describe, dbn_winograd_rows, dbn_winograd_wgrad_linear, dbn_winograd_wgrad_slab_floats, the two eligibility tests,
dbn_igemm_bn_rows: no device call, nothing is launched), so that a change of a threshold which moves a case off its path fails HERE and the
list is repaired, instead of the GPU pins quietly testing less.  The only arithmetic restated from csrc/winograd_wgrad_f32.hip is what no
entry point reports: the groups of a workgroup, g0 = split * groups / nsplit (conv_ref.wino_ranges), and — for the seams and the fp32
emulation — which tiles a group holds (conv_ref.wino_group_tiles).

The second half shows WHY the exact data of the GPU module is exact: every stage of the weight gradient (A dY A^T, B^T d B, the per-workgroup
fp32 sums over its groups in two orders, the float64 slab sum, G^T . G) and of the forward transform evaluated in float32 equals float64,
every partial sum stays below 2^24 units of its grid, and the small data set of the BatchNorm-backward sums keeps sum |g| and
sum |g xhat| below 2^24 grid units per channel."""
import ctypes

import pytest
import torch

import conv_ref as R
from db_text_minimal_amd import _lib

DBN_OK = 0
WIDE_FROM = 128  # splits from which the table says 'wide' (asserted against the library case by case, never used to predict it)


def L():
    return _lib.lib()


def describe(N, H, W, O, Cb):
    plan = _lib.WinogradPlan()
    assert L().dbn_winograd_describe(N, H, W, O, Cb, ctypes.byref(plan)) == DBN_OK
    return plan


def test_the_tables_cover_the_lists():
    assert list(R.WINO_WGRAD_PLAN) == R.WINO_WGRAD_CASES and list(R.WINO_FWD_PLAN) == R.WINO_FWD_CASES
    assert list(R.IGEMM_FINAL_PLAN) == R.IGEMM_FINAL_CASES
    assert len(set(R.WINO_WGRAD_CASES)) == 10 and len(set(R.WINO_FWD_CASES)) == 8


def test_describe_rejects_what_it_cannot_describe():
    plan = _lib.WinogradPlan()
    assert L().dbn_winograd_describe(2, 16, 16, 64, 64, None) != DBN_OK
    assert L().dbn_winograd_describe(2, 16, 16, 60, 64, ctypes.byref(plan)) != DBN_OK
    assert L().dbn_winograd_describe(0, 16, 16, 64, 64, ctypes.byref(plan)) != DBN_OK


@pytest.mark.parametrize('case', R.WINO_WGRAD_CASES)
def test_weight_gradient_cases_reach_their_plan(case):
    N, Ci, Cs, Co, H, W = case
    form, groups, nsub, nsplit, red = R.WINO_WGRAD_PLAN[case]
    assert L().dbn_winograd_wgrad_eligible(N, H, W, Co, Cs, Ci) == 1, 'not a Winograd weight gradient any more: %s' % (case, )
    p = describe(N, H, W, Co, Cs)
    got = ('lin' if p.wgrad_lin else 'patch', p.wgrad_groups, p.wgrad_nsub, p.wgrad_nsplit, 'wide' if p.wgrad_wide else 'serial')
    assert got == (form, groups, nsub, nsplit, red), 'plan of %s: %s, not %s' % (case, got, (form, groups, nsub, nsplit, red))
    # the entry points the engine sizes its buffers with agree with the description
    assert L().dbn_winograd_wgrad_linear(H, W) == p.wgrad_lin
    assert L().dbn_winograd_wgrad_slab_floats(N, H, W, Co, Cs) == nsplit * nsub * 16 * 4096
    assert nsub == (Co // 64) * (Cs // 64) and (red == 'wide') == (nsplit >= WIDE_FROM)
    ranges = R.wino_ranges(groups, nsplit)
    assert ranges[0][0] == 0 and ranges[-1][1] == groups and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    assert all(g1 > g0 for g0, g1 in ranges), 'a workgroup of %s has no group: its slab would be all zero' % (case, )


@pytest.mark.parametrize('case', R.WINO_FWD_CASES)
def test_forward_cases_reach_their_plan(case):
    N, Ci, Cs, Cd, H, W = case
    form, rows = R.WINO_FWD_PLAN[case]
    assert L().dbn_winograd_eligible(N, H, W, Cs, Cd) == 1, 'not a Winograd conv any more: %s' % (case, )
    p = describe(N, H, W, 64, 64)
    got = ('lin' if p.fwd_lin else 'patch', p.fwd_rows)
    assert got == (form, rows), 'plan of %s: %s, not %s' % (case, got, (form, rows))
    assert L().dbn_winograd_rows(N, H, W) == rows
    row, piv = R.wino_rows(N, H, W, form == 'lin')
    assert int(row.max()) + 1 == rows == piv.shape[0] and int(row.min()) == 0
    assert all(int(row[n, h, w]) == r for r, (n, h, w) in enumerate(piv.tolist())), 'a pivot pixel outside its own row'


@pytest.mark.parametrize('case', R.IGEMM_FINAL_CASES)
def test_implicit_gemm_finalize_cases_have_their_rows(case):
    N, Ci, Co, k, s, p, H, W = case
    Ho, Wo = R.out_size(H, k, s, p), R.out_size(W, k, s, p)
    # the data gradient: source dy [N, Ho, Wo, Co], destination dx [N, H, W, Ci], mode 1, fp32, tile hint 0
    assert L().dbn_igemm_bn_rows(0, 0, N, Ho, Wo, Co, H, W, Ci, k, k, s, p, 1, 0) == R.IGEMM_FINAL_PLAN[case]


def per_workgroup(case):
    _, groups, _, nsplit, _ = R.WINO_WGRAD_PLAN[case]
    return [g1 - g0 for g0, g1 in R.wino_ranges(groups, nsplit)]


def crosses_images(case):
    N, _, _, _, H, W = case
    form, groups, _, nsplit, _ = R.WINO_WGRAD_PLAN[case]
    gpi = groups // N
    return any(g0 // gpi != (g1 - 1) // gpi for g0, g1 in R.wino_ranges(groups, nsplit))


def test_every_path_occurs():
    """Conditions on the tables (which the tests above tie to the library), not measurements: each path the GPU pins are there for."""
    P, C = R.WINO_WGRAD_PLAN, R.WINO_WGRAD_CASES
    patch, lin = [c for c in C if P[c][0] == 'patch'], [c for c in C if P[c][0] == 'lin']
    ragged = lambda c: c[4] % 8 != 0 and c[5] % 16 != 0
    assert any(set(per_workgroup(c)) == {1, 2} for c in patch), 'no patch-form case with uneven 1 - 2 groups per workgroup'
    assert any(min(per_workgroup(c)) >= 3 and ragged(c) and c[5] % 2 and crosses_images(c) for c in patch), \
        'no ragged odd-width patch-form case with >= 3 groups per workgroup and a range across two images'
    assert any(min(per_workgroup(c)) >= 3 and crosses_images(c) and P[c][4] == 'serial' for c in lin), 'no LIN case with 3 groups per workgroup across images'
    wide = [c for c in C if P[c][4] == 'wide']
    assert any(P[c][3] == 128 for c in wide), 'the wide reduction is not pinned at its threshold'
    assert any(P[c][3] % 32 for c in wide), 'no wide reduction with uneven split shares (nsplit % 32 != 0)'
    assert any(P[c][3] > 128 and ragged(c) for c in wide), 'no wide reduction on a ragged map'
    assert any(c[2] // 64 == 2 for c in wide), 'no wide reduction with two input-channel blocks'
    assert any(32 < c[1] < 64 == c[2] for c in wide) and any(c[1] <= 32 and c[2] == 64 for c in wide), 'the padding-channel tails (I = 40, I = 20) are gone'
    assert any(c in lin and max(per_workgroup(c)) > 1 for c in wide), 'no LIN case with the wide reduction and more than one group per workgroup'
    F, FC = R.WINO_FWD_PLAN, R.WINO_PATCH_CASES
    assert any(c[4] % 8 and c[5] % 16 and c[4] % 2 and c[5] % 2 for c in FC), 'no patch-form forward case ragged in both directions with odd sides'
    assert any(c[3] == 128 and c[4] % 8 and c[5] % 16 for c in FC) and any(c[2] > c[1] for c in FC)
    rows = {F[c] for c in R.WINO_FINAL_CASES}
    assert {('patch', 64), ('patch', 72), ('patch', 144), ('lin', 65), ('lin', 68)} <= rows
    assert {r % 64 for _, r in rows} >= {0, 8, 16, 1, 4} and max(-(-r // 64) for _, r in rows) == 3
    ir = sorted(R.IGEMM_FINAL_PLAN.values())
    assert ir[0] == 64 and ir[1] == 65 and ir[2] >= 129
    assert {c[4] for c in R.IGEMM_FINAL_CASES} == {1, 2}


def test_the_seams_name_what_they_claim():
    case = (3, 256, 256, 256, 29, 77)
    N, _, _, _, H, W = case
    form, groups, _, nsplit, _ = R.WINO_WGRAD_PLAN[case]
    pts = set(R.winograd_wgrad_seams(N, H, W, form, groups, nsplit))
    assert {(n, h, w) for n in range(N) for h in (0, H - 1) for w in (0, W - 1)} <= pts
    assert {(1, h, w) for h in (7, 8, 23, 24) for w in (15, 16, 63, 64)} <= pts and {(0, H - 1, w) for w in range(W)} <= pts
    # patch 3 of image 0 is the first of workgroup 1's range: all four pixels of its first tile and of its last in-map tile
    assert R.wino_ranges(groups, nsplit)[1] == (3, 7) and R.wino_group_tiles(N, H, W, False, 3)[1][0] == (0, 24)
    assert {(0, h, w) for h in (0, 1) for w in (48, 49)} <= pts and {(0, h, w) for h in (6, 7) for w in (62, 63)} <= pts
    # the range 18 .. 21 holds the last two patches of image 0 and the first two of image 1
    assert (18, 22) in R.wino_ranges(groups, nsplit) and {(0, H - 1, W - 1), (1, 0, 0)} <= pts
    lin_case = (3, 512, 512, 512, 20, 20)
    pts = set(R.winograd_wgrad_seams(3, 20, 20, 'lin', 12, 4))
    assert {(0, 2 * (31 // 10), 2 * (31 % 10) + 1), (0, 2 * (32 // 10), 2 * (32 % 10)), (1, 0, 0), (0, 19, 19)} <= pts and lin_case in R.WINO_WGRAD_PLAN
    fpts = set(R.winograd_patch_seams(2, 15, 77))
    assert {(1, h, w) for h in (7, 8) for w in (15, 16, 63, 64)} <= fpts and {(0, 14, w) for w in range(77)} <= fpts and {(1, h, 76) for h in range(15)} <= fpts


# ---- why the exact data is exact --------------------------------------------------------------------------------------------------------
CO_SUB, CI_SUB = 3, 4  # channels of the emulation: every (o, i) pair of the weight gradient is independent of the others


def emulate(case, x, dy, grid):
    """The emulated weight gradient of the first channels in float32 against float64, stage by stage, and against the direct reference."""
    form, groups, _, nsplit, _ = R.WINO_WGRAD_PLAN[case]
    xs, dys = x[:, -CI_SUB:], dy[:, -CO_SUB:]  # the last channels: those of the impulses
    e32 = R.winograd_wgrad_emulated(xs, dys, form, groups, nsplit, torch.float32)
    e64 = R.winograd_wgrad_emulated(xs, dys, form, groups, nsplit, torch.float64)
    for k in ('D', 'V', 'slabs', 'slabs_rev'):
        assert torch.equal(e32[k].double(), e64[k]), '%s of %s is not exact in float32' % (k, case)
    assert torch.equal(e64['slabs'], e64['slabs_rev'])
    ref = R.conv2d_wgrad(xs, dys, 3, 3, 1, 1)
    assert torch.equal(e32['dg'].double(), ref), 'the emulated weight gradient of %s differs from the direct reference' % (case, )
    # all channels, any order: |D| <= 4 max |dy| and |V| <= 4 max |x| (two signed pairs each), 32 tiles per group
    most = max(g1 - g0 for g0, g1 in R.wino_ranges(groups, nsplit))
    assert 16 * float(dy.abs().max()) * float(x.abs().max()) * 32 * most / grid < 2**24
    # the float64 slab sum and G^T . G (entries 1, 1 / 2: two more bits) hold sum |x| |dy| over ALL pixels with room to spare; the fp32 result
    # is a multiple of `grid` below 2^24 of it
    N, _, _, _, H, W = case
    total = 16 * float(dy.abs().max()) * float(x.abs().max()) * N * ((H + 7) // 8 * 4) * ((W + 15) // 16 * 8)
    assert total / (grid / 4) < 2**50
    assert float(x.abs().max()) * float(dy.abs().max()) * N * H * W / grid < 2**24


@pytest.mark.parametrize('case', R.WINO_WGRAD_CASES)
def test_weight_gradient_data_is_exact_in_every_stage(case):
    N, Ci, Cs, Co, H, W = case
    x, dy = R.wino_wgrad_data(case, 'dense')
    emulate(case, x, dy, 2.0**-4)  # D and V on 2^-2: products on 2^-4
    sc, sh = R.act_coeffs(Cs, 35)
    xa = R.apply_act(x, sc[:Ci], sh[:Ci])
    assert torch.equal(xa * 8, (xa * 8).round()) and float(xa.max()) <= 2 and float(xa.min()) == 0
    assert torch.equal(R.apply_act(x.float(), sc[:Ci].float(), sh[:Ci].float()).double(), xa), 'apply-on-load is not exact in float32'
    emulate(case, xa, dy, 2.0**-5)  # V on 2^-3
    for kind in ('sparse dy', 'sparse x'):
        xs, dys = R.wino_wgrad_data(case, kind)
        assert float(xs.abs().max()) <= 2 and float(dys.abs().max()) <= 2
        emulate(case, xs, dys, 2.0**-3)  # impulses on 2^-1, the dense operand on 2^-2
    xs, dys = R.wino_wgrad_data(case, 'sparse dy')
    emulate(case, R.apply_act(xs, sc[:Ci], sh[:Ci]), dys, 2.0**-4)


@pytest.mark.parametrize('case', R.WINO_FWD_CASES)
@pytest.mark.parametrize('data', ['dense', 'dense act', 'impulses'])
def test_forward_data_is_exact_in_every_stage(case, data):
    """As test_winograd_transforms_are_exact_in_fp32_on_the_exact_data of tests/test_conv_ref_cpu.py, on the patch-form and finalize cases
    (eight output channels: they are independent of each other) and with the activation applied on load; the data gradient is the same
    kernel on the rotated filter, with dy in place of x."""
    N, Ci, Cs, Cd, H, W = case
    co = min(Cd, 8)
    b = R.dense_bias(co, 23)
    if data == 'impulses':
        (x, ) = R.impulse_maps(N, Ci, H, W, R.winograd_patch_seams(N, H, W), 0)
        w = R.distinct_w(Cd, Ci, 3, 3)[:co]
        grid = 2.0**-10  # V on 2^-1, U on 2^-9
    else:
        x, w = R.dense_x((N, Ci, H, W), 21), R.dense_w((Cd, Ci, 3, 3), 22, winograd=True)[:co]
        grid = 2.0**-5  # V on 2^-2, U on 2^-3
        if data == 'dense act':
            sc, sh = R.act_coeffs(Cs, 25)
            x = R.apply_act(x, sc[:Ci], sh[:Ci])
            grid = 2.0**-6  # V on 2^-3
    got = R.winograd_fp32(x, w, b)
    ref = R.winograd_fp64(x, w, b)
    for name, g, r in zip(('y', 'V', 'U', 'M'), got, ref):
        assert torch.equal(g.double(), r), name
    assert torch.equal(ref[0], R.conv2d(x, w, b, 1, 1))
    _, V, U, _ = ref
    bound = 16 * float(torch.einsum('ocij,nchwij->nohwij', U.abs(), V.abs()).max()) + 2
    assert bound / grid < 2**22
    # residual + ReLU of dbn_winograd_conv_act_f32: y + res with res on 2^-5 in [-1, 1] keeps the grid; relu is exact


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('case', R.WINO_FINAL_CASES + R.WINO_PATCH_CASES[:1])
def test_small_sums_data_adds_exactly_in_fp32(case, accumulate):
    """The two BatchNorm-backward sums of conv_ref.wino_sums_data: every term g is a multiple of 2^-3 and g xhat of 2^-4, and sum |g|,
    sum |g xhat| over ALL pixels of a channel stay below 2^24 units of those grids — so every partial sum of every order (16 pixels per
    lane, lane pairs, four waves, 64-row groups, groups) is exact in fp32, the fused multiply-adds included."""
    d = R.wino_sums_data(case, accumulate)
    dx = d['dx']
    assert torch.equal(dx * 8, (dx * 8).round()) and R.representable(dx, torch.float32)
    for m, y, mean, rstd in ((d['y'] * d['msc'].view(1, -1, 1, 1) + d['msh'].view(1, -1, 1, 1), d['y'], d['mean'], d['rstd']),
                             (d['z'], d['y'], d['mean'], d['rstd']), (d['z'], d['y2'], d['mean2'], d['rstd2'])):
        xhat = (y - mean.view(1, -1, 1, 1)) * rstd.view(1, -1, 1, 1)
        assert torch.equal(xhat * 2, (xhat * 2).round()) and float(xhat.abs().max()) <= 3
        assert bool((m != 0).all())
        s1, s2, a1, a2 = R.bn_backward_sums(dx, y, mean, rstd, m)
        assert float(a1.max()) * 8 < 2**24 and float(a2.max()) * 16 < 2**24, (float(a1.max()) * 8, float(a2.max()) * 16)
    assert int((d['msh'] > 0).sum()) >= 8 and int((d['msh'] < 0).sum()) >= 8
