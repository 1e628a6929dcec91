"""-m gpu: the three Winograd kernels (csrc/winograd_f32.hip forward / data gradient, csrc/winograd_wgrad_f32.hip weight gradient and its slab
reductions) on the paths the training step takes, against the float64 reference of tests/conv_ref.py.  It continues the Winograd rows of
tests/test_conv_fp64_gpu.py, whose shapes all give a weight-gradient workgroup ONE patch or tile group, launch only the serial slab
reduction, run the forward kernel in its consecutive-tile form and fold the BatchNorm-backward sums in one row group.  The cases and the
plan each must reach stand in conv_ref.WINO_WGRAD_PLAN / WINO_FWD_PLAN / IGEMM_FINAL_PLAN; tests/test_winograd_cases_cpu.py asks the library
(dbn_winograd_describe and friends, nothing launched) that every case still reaches its plan, and shows by fp32 emulation why the exact
data below is exact in any order of summation.

Every output, slab, partial-row, group and statistics buffer starts as NaN; operands and float64 references are built once per case.

Weight gradient (dbn_winograd_wgrad_f32), every case plain and with the BatchNorm + ReLU applied on load (x_scale / x_shift; the reference
is the gradient of the conv of relu(fma(x, scale, shift))), the scale alternating between 1 and 1 / 2:
  * dense dyadic data: equal to float64 BIT FOR BIT; padding channels (Cs > Ci) hold zeros in one run and a finite constant in another —
    the reduction drops their columns;
  * impulses in dY (x dense), and in x (dY dense), on conv_ref.winograd_wgrad_seams: first / last pixel of every patch or 32-tile group,
    every pixel of the first and last tile of each workgroup's range g0 .. g1, both sides of the image boundaries inside a range, the four
    pixels around every 8 x 16 patch corner, the whole border of every image (the halo outside must read as zero): bit for bit;
  * random data: distance to float64 against that of fp32 autograd on the CPU (gpu_util.distance_ratio);
  * phases 1 then 2, and a second run, equal phase 3 bit for bit; and phase 2 ALONE on a slab the test fills with dyadic values equals a
    float64 host fold (sum over the splits, G^T . G, scale, cast) to the last bit — both reduction kernels, every split share z0 .. z1, the
    hand-over between the split lanes and the padding-channel tail, with no matrix kernel in the way.

Forward (dbn_winograd_conv_bn_f32, dbn_winograd_conv_bn_act_f32 with the activation applied on load, dbn_winograd_conv_act_f32 with residual
and ReLU) and data gradient (dbn_winograd_dgrad_bnsums_f32, accumulate 0 and 1) in the patch form on ragged maps, Cd = 128 and padded source
channels, and on the finalize cases: dense dyadic data and impulses on conv_ref.winograd_patch_seams bit for bit, random data by distance.
  * BatchNorm statistics (gamma given), with the finalize kernel and folded in the kernel (dbn_conv_bn_set_final): on a constant map under a
    centre-tap filter the output is one constant per channel inside the map and the bare bias on the pixels a ragged patch computes outside
    it — save_mean must equal the constant bit for bit and the variance 0 (rstd = 1 / sqrt(eps) to 2 ulp), which fails as soon as one
    out-of-map pixel is counted; on random data against float64 statistics of the kernel's own stored output within the bound of
    stats_bounds (the derivation of tests/test_fpn_fp64_gpu.py with the conv's own error taken out).
  * BatchNorm-backward sums and their in-kernel finalize on 64 / 72 / 144 (patch form) and 65 / 68 rows (consecutive-tile form), masks
    'self', 'tensor' + a second BatchNorm, none: the folded partial rows, c1c2, dgamma, dbeta against float64 sums over the kernel's own dx
    as stored (tolerances of test_winograd_dgrad_with_bn_sums); each launch twice on the same counters, which must read zero after
    each, with bit-identical finalized outputs; against dbn_bn_backward_t folding the same rows (sums_parts = rows).  That route adds all
    rows in float64, the kernel rounds each 64-row group's float64 sum to fp32 first: bit-identical with one group, otherwise within
    2^-23 of sum |rows| per channel.  y, zmask and y2 carry values four times the usual size: a ragged patch's out-of-map lane that
    loaded the pixel behind the row's end instead of nothing would move the sums far beyond the tolerance; with the mask recomputed
    from y ('self') the channels with mask_shift > 0 count an out-of-map pixel that reads as zero unless the lane is masked.
  * one small dyadic data set (conv_ref.wino_sums_data) on which dx, the partial rows, both group levels and the finalized outputs are
    exact in fp32: all compared bit for bit with float64.
  * the same finalize checks on the implicit-GEMM data gradient (dbn_igemm_bnsums_t, fp32) at 64, 65 and 132 rows, stride 1 and 2.

What a deliberately broken kernel trips.  Each of these was built once (memory-safe changes of arithmetic only; the broken variants are not
committed) and this module run against it on the MI355X; the counts are the failing test cases:
  * skipping the matrix phase of the second patch of a range (patch form): 14 — the dense, sparse-dY, sparse-x and random tests of the two
    patch-form cases with more than one patch per workgroup, (5, 128, ..) and (3, 256, ..), plain and with apply-on-load.  The impulses on
    the first tile of EVERY group leave gradient entries that only this patch contributes to.  (The consecutive-tile cases (3, 512, ..) and
    (40, 128, ..) guard the same loop of the LIN form.)
  * multiplying from the other LDS image (cbuf ^ 1): 63 — every exact and random weight-gradient test of all eight patch-form cases, and
    the run-to-run test of seven of them (the image read has not been written yet);
  * one split lane of the wide reduction not adding its own share: 56 — test_reduction_alone_equals_a_float64_fold on all seven wide cases
    (every slab element is non-zero, so a missing z0 .. z1 share moves every output) and every exact and random test of those cases;
  * counting the out-of-map pixels of a ragged patch in the statistics: 24 — test_statistics_of_a_constant_map_over_ragged_patches on the five
    ragged patch-form cases, with the finalize kernel and folded in the kernel (mean and variance move by the filter's centre sum), and the
    random-data statistics of the same cases;
  * folding only the first row group in the finalize of the BatchNorm-backward sums: 24 — every masked case of the 72 / 144 / 65 / 68-row
    shapes, on random and on exact data; the 64-row case, one group, rightly passes.  The 65 / 132-row implicit-GEMM cases guard the
    same fold in igemm_kernel.h.

The margins m follow the rule of tests/test_conv_fp64_gpu.py: per kernel, twice the largest ratio measured on the MI355X over these cases,
rounded up to a power of two, capped at 16.  Each random-data test prints
    RATIO winograd <kernel> <case> [act | res | + base]: rms <ratio> max <ratio> (fp32 itself: rms <abs> max <abs>)
and the table holds "rms ratio / max ratio".

    weight gradient                              plain           act
    wgrad (5, 128, 128, 128, 40, 40)         0.25 / 0.18   0.23 / 0.21
    wgrad (3, 256, 256, 256, 29, 77)         0.23 / 0.12   0.21 / 0.07
    wgrad (3, 512, 512, 512, 20, 20)         0.46 / 0.26   0.43 / 0.22
    wgrad (2, 64, 64, 64, 64, 128)           0.23 / 0.24   0.21 / 0.20
    wgrad (9, 64, 64, 64, 40, 36)            0.26 / 0.21   0.23 / 0.15
    wgrad (3, 64, 64, 64, 61, 125)           0.19 / 0.19   0.18 / 0.14
    wgrad (2, 128, 128, 64, 61, 125)         0.12 / 0.08   0.11 / 0.08
    wgrad (2, 40, 64, 64, 64, 128)           0.23 / 0.23   0.21 / 0.16
    wgrad (2, 20, 64, 64, 61, 125)           0.24 / 0.22   0.22 / 0.15
    wgrad (40, 128, 128, 64, 20, 20)         0.27 / 0.23   0.25 / 0.22
    forward                                      plain           act     res + ReLU     data gradient      plain        + base
    fwd (2, 64, 64, 64, 15, 77)              1.20 / 0.90   1.23 / 1.07   1.19 / 0.93     dgrad            1.20 / 1.08   1.20 / 1.03
    fwd (2, 32, 32, 128, 13, 78)             0.94 / 0.58   1.02 / 0.89   0.94 / 0.62     dgrad            0.93 / 0.68   0.94 / 0.66
    fwd (2, 20, 32, 64, 15, 77)              0.85 / 0.42   0.93 / 0.75   0.86 / 0.50     dgrad            0.85 / 0.42   0.86 / 0.40
    fwd (1, 64, 64, 64, 64, 128)             1.19 / 1.07   1.23 / 1.26   1.19 / 1.13     dgrad            1.20 / 0.87   1.19 / 0.85
    fwd (1, 64, 64, 64, 65, 113)             1.18 / 0.94   1.23 / 1.06   1.18 / 1.18     dgrad            1.19 / 1.11   1.19 / 1.03
    fwd (1, 64, 64, 64, 71, 241)             1.19 / 1.08   1.23 / 0.98   1.18 / 1.03     dgrad            1.19 / 1.12   1.19 / 1.02
    fwd (5, 64, 64, 64, 40, 40)              1.20 / 1.15   1.24 / 1.10   1.19 / 1.07     dgrad            1.20 / 0.88   1.20 / 0.91
    fwd (17, 64, 64, 64, 20, 20)             1.23 / 0.88   1.27 / 1.37   1.22 / 0.86     dgrad            1.22 / 0.97   1.22 / 0.93
    wgrad 0.46 -> m = 1      fwd 1.37 -> m = 4      dgrad 1.22 -> m = 4

Every weight-gradient ratio is below 1 / 2: a workgroup's fp32 chain is at most four groups (128 tiles) long and the slabs are added in float64,
where the one-group-per-workgroup cases of tests/test_conv_fp64_gpu.py sit at 0.36 - 0.39; the consecutive-tile form at layer4's shape
(three groups per workgroup, four slabs) is the farthest at 0.46.  The forward kernel and the data gradient sit where the two small cases of
that module do (1.2), in both forms, ragged or not.  No case exposed a defect: the kernels needed no change.  The only change to the library
is dbn_winograd_describe, a host-side report of the plans that launches nothing.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import conv_ref as R
from gpu_util import DEV, L, NAN, U, distance_ratio, exact, igemm_t, nchw, nhwc, pack, reduce_ws, report, rnd, stream, within
from db_text_minimal_amd import _lib

pytestmark = pytest.mark.gpu

# margins m of the random-data tests: per kernel, twice the largest ratio of the table in the module docstring, rounded up to a power of two
MARGIN = {'wgrad': 1, 'fwd': 4, 'dgrad': 4}
assert max(MARGIN.values()) <= 16
EPS, MOM = 1e-5, 0.1
SCALE = {c: (1.0, 0.5)[i % 2] for i, c in enumerate(R.WINO_WGRAD_CASES)}
JUNK = 3.0  # what the padding channels of x hold in the second run of a padded case


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def pad_c(x, c, fill=0.0):
    return x if x.shape[1] == c else torch.cat([x, torch.full((x.shape[0], c - x.shape[1], *x.shape[2:]), fill, dtype=x.dtype)], 1)


def dev(t):
    return t.float().contiguous().to(DEV)


def ptr(t):
    return None if t is None else t.data_ptr()


def same_bits(tag, a, b):
    assert a.shape == b.shape and bool(torch.isfinite(a).all()), tag + ': non-finite values'
    ne = a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)
    assert not bool(ne.any()), '%s: %d of %d elements differ in their bits' % (tag, int(ne.sum()), a.numel())


# ---- the weight gradient ----------------------------------------------------------------------------------------------------------------
def wgrad_buffers(case):
    N, Ci, Cs, Co, H, W = case
    assert L().dbn_winograd_wgrad_eligible(N, H, W, Co, Cs, Ci)
    return nan(L().dbn_winograd_wgrad_slab_floats(N, H, W, Co, Cs)), nan(Co, Ci, 3, 3)


def run_wgrad(case, x, dy, act=None, fill=0.0, phases=(3, )):
    """dbn_winograd_wgrad_f32 on CPU NCHW operands (NaN-filled slab and gradient) -> the gradient [Co, Ci, 3, 3] on the CPU.  act: the
    (scale, shift) [Cs] applied on load."""
    N, Ci, Cs, Co, H, W = case
    xs, dys = nhwc(pad_c(x.float(), Cs, fill)), nhwc(dy.float())
    slab, g = wgrad_buffers(case)
    sc, sh = (None, None) if act is None else (dev(act[0]), dev(act[1]))
    for ph in phases:
        _lib.check(L().dbn_winograd_wgrad_f32(ph, dys.data_ptr(), xs.data_ptr(), ptr(sc), ptr(sh), slab.data_ptr(), g.data_ptr(), N, H, W, Co, Cs, Ci,
                                              SCALE[case], stream()), 'winograd wgrad phase %d' % ph)
    torch.cuda.synchronize()
    return g.cpu()


def fills(case):
    return (0.0, JUNK) if case[2] > case[1] else (0.0, )


@functools.lru_cache(maxsize=None)
def act_of(case):
    return R.act_coeffs(case[2], 35)


def activated(case, x):
    sc, sh = act_of(case)
    return R.apply_act(x, sc[:case[1]], sh[:case[1]])


@functools.lru_cache(maxsize=None)
def wgrad_exact_case(case, kind, act):
    x, dy = R.wino_wgrad_data(case, kind)
    return x, dy, SCALE[case] * R.conv2d_wgrad(activated(case, x) if act else x, dy, 3, 3, 1, 1)


@pytest.mark.parametrize('act', [False, True])
@pytest.mark.parametrize('case', R.WINO_WGRAD_CASES)
def test_weight_gradient_is_exact_on_dense_dyadic_data(case, act):
    x, dy, ref = wgrad_exact_case(case, 'dense', act)
    for fill in fills(case):
        exact('winograd wgrad dense %s act %d padding %g' % (case, act, fill), run_wgrad(case, x, dy, act_of(case) if act else None, fill), ref)


@pytest.mark.parametrize('act', [False, True])
@pytest.mark.parametrize('case', R.WINO_WGRAD_CASES)
def test_weight_gradient_is_exact_on_sparse_dy(case, act):
    x, dy, ref = wgrad_exact_case(case, 'sparse dy', act)
    exact('winograd wgrad sparse dy %s act %d' % (case, act), run_wgrad(case, x, dy, act_of(case) if act else None), ref)


@pytest.mark.parametrize('case', R.WINO_WGRAD_CASES)
def test_weight_gradient_is_exact_on_sparse_x(case):
    x, dy, ref = wgrad_exact_case(case, 'sparse x', False)
    for fill in fills(case):
        exact('winograd wgrad sparse x %s padding %g' % (case, fill), run_wgrad(case, x, dy, None, fill), ref)


@functools.lru_cache(maxsize=None)
def wgrad_random_case(case):
    N, Ci, Cs, Co, H, W = case
    return rnd(N, Ci, H, W, seed=1), rnd(N, Co, H, W, seed=4), (rnd(Cs, seed=6) * 0.5 + 1, rnd(Cs, seed=7))


def act32(x, sc, sh):
    """relu(fma(x, scale, shift)) as the kernel's loads form it: the product is exact in float64, one rounding to fp32."""
    return R.apply_act(x.double(), sc[:x.shape[1]].double(), sh[:x.shape[1]].double()).float()


def wgrad_refs(case, x, dy):
    w = torch.zeros((case[3], case[1], 3, 3), requires_grad=True)  # (the gradient with respect to w does not depend on w)
    (g32, ) = torch.autograd.grad(F.conv2d(x, w, None, 1, 1), w, dy)
    return SCALE[case] * R.conv2d_wgrad(x.double(), dy.double(), 3, 3, 1, 1), SCALE[case] * g32


@pytest.mark.parametrize('act', [False, True])
@pytest.mark.parametrize('case', R.WINO_WGRAD_CASES)
def test_weight_gradient_distance_to_fp64(case, act):
    x, dy, coeffs = wgrad_random_case(case)
    r64, r32 = wgrad_refs(case, act32(x, *coeffs) if act else x, dy)
    distance_ratio('winograd wgrad %s%s' % (case, ' act' if act else ''), run_wgrad(case, x, dy, coeffs if act else None), r64, r32, MARGIN['wgrad'])


@pytest.mark.parametrize('case', R.WINO_WGRAD_CASES)
def test_weight_gradient_phases_and_a_second_run_are_bit_identical(case):
    x, dy, coeffs = wgrad_random_case(case)
    g = run_wgrad(case, x, dy, coeffs)
    same_bits('second run %s' % (case, ), run_wgrad(case, x, dy, coeffs), g)
    same_bits('phase 1 + phase 2 %s' % (case, ), run_wgrad(case, x, dy, coeffs, phases=(1, 2)), g)


@pytest.mark.parametrize('case', R.WINO_WGRAD_CASES)
def test_reduction_alone_equals_a_float64_fold(case):
    """Phase 2 on slab contents of the test's own: multiples of 1 / 4 in [-16, 16], none zero — every sum over <= 192 splits and G^T . G on
    top (entries 1 and 1 / 2) is a multiple of 2^-6 below 2^16: exact in any order and representable in fp32."""
    N, Ci, Cs, Co, H, W = case
    _, _, nsub, nsplit, _ = R.WINO_WGRAD_PLAN[case]
    slab, g = wgrad_buffers(case)
    assert slab.numel() == nsplit * nsub * 16 * 4096
    v = torch.randint(1, 65, (slab.numel(), ), generator=torch.Generator().manual_seed(9)).float() / 4
    v = v * (torch.randint(0, 2, (slab.numel(), ), generator=torch.Generator().manual_seed(10)).float() * 2 - 1)
    slab.copy_(v.to(DEV))
    xs, dys = nan(N, H, W, Cs), nan(N, H, W, Co)  # phase 2 reads neither
    _lib.check(L().dbn_winograd_wgrad_f32(2, dys.data_ptr(), xs.data_ptr(), None, None, slab.data_ptr(), g.data_ptr(), N, H, W, Co, Cs, Ci, SCALE[case],
                                          stream()), 'winograd wgrad phase 2')
    torch.cuda.synchronize()
    ref = R.fold_slabs(v.view(nsplit, Co // 64, Cs // 64, 4, 4, 64, 64), SCALE[case])[:, :Ci]
    assert R.representable(ref.double(), torch.float32)
    exact('winograd wgrad reduction %s' % (case, ), g.cpu(), ref)
    same_bits('the slab is left as it was', slab.cpu(), v)


# ---- forward and data gradient: launches ------------------------------------------------------------------------------------------------
def pack_wino(w, O, I, Cs, dgrad):
    up = nan(L().dbn_winograd_panel_floats(O, Cs))
    wd = dev(w)
    _lib.check(L().dbn_winograd_pack(wd.data_ptr(), O, I, Cs, dgrad, up.data_ptr(), stream()), 'winograd pack')
    return up


def bn_params(C):
    return rnd(C, seed=4) * 0.3 + 1, rnd(C, seed=5), rnd(C, seed=6) * 0.1, rnd(C, seed=7).abs() + 0.5


def run_conv(case, x, up, b, act=None, bn=None, final=False):
    """dbn_winograd_conv_bn_f32 / _act_f32 (act: (scale, shift) [Cs]) -> y [N, Cd, H, W] on the CPU and, with bn = (gamma, beta, run_mean,
    run_var), the statistics; final: folded by the kernel's own last workgroups (dbn_conv_bn_set_final)."""
    N, Ci, Cs, Cd, H, W = case
    assert L().dbn_winograd_eligible(N, H, W, Cs, Cd)
    xs, y = nhwc(pad_c(x.float(), Cs)), nan(N, H, W, Cd)
    bd = None if b is None else dev(b)
    sc, sh = (None, None) if act is None else (dev(act[0]), dev(act[1]))
    st, cnt = {}, None
    if bn is not None:
        st = dict(gamma=dev(bn[0]), beta=dev(bn[1]), run_mean=dev(bn[2]), run_var=dev(bn[3]), scale=nan(Cd), shift=nan(Cd), mean=nan(Cd), rstd=nan(Cd),
                  ws=nan(L().dbn_winograd_ws_floats(N, H, W, Cd)))
        if final:
            rows = L().dbn_winograd_rows(N, H, W)
            cnt = torch.zeros(L().dbn_igemm_bn_final_counters(rows, Cd), device=DEV, dtype=torch.int32)
            grp = nan(L().dbn_conv_bn_final_group_doubles(rows, Cd), dtype=torch.float64)
            _lib.check(L().dbn_conv_bn_set_final(cnt.data_ptr(), grp.data_ptr()), 'set_final')
    g = lambda k: ptr(st.get(k))
    _lib.check(L().dbn_winograd_conv_bn_act_f32(xs.data_ptr(), ptr(sc), ptr(sh), up.data_ptr(), ptr(bd), y.data_ptr(), N, H, W, Cs, Cd, g('gamma'), g('beta'),
                                                EPS if bn else 0.0, MOM if bn else 0.0, g('run_mean'), g('run_var'), g('scale'), g('shift'), g('mean'),
                                                g('rstd'), g('ws'), stream()), 'winograd conv')
    torch.cuda.synchronize()
    if cnt is not None:
        assert int(cnt.abs().sum()) == 0, 'the finalize left a counter behind'
    return nchw(y), {k: v.cpu() for k, v in st.items() if k not in ('gamma', 'beta', 'ws')}


def run_conv_res(case, x, up, b, res):
    """dbn_winograd_conv_act_f32: relu(conv(x) + bias + res)."""
    N, Ci, Cs, Cd, H, W = case
    xs, y, bd, rs = nhwc(pad_c(x.float(), Cs)), nan(N, H, W, Cd), dev(b), nhwc(res.float())
    _lib.check(L().dbn_winograd_conv_act_f32(xs.data_ptr(), up.data_ptr(), bd.data_ptr(), rs.data_ptr(), 1, y.data_ptr(), N, H, W, Cs, Cd, stream()),
               'winograd conv act')
    torch.cuda.synchronize()
    return nchw(y)


class Sums:
    """The arguments of the BatchNorm-backward sums of a data gradient (CPU NCHW / [C] tensors) and their device copies."""

    def __init__(self, mask, y, z, msc, msh, mean, rstd, y2, mean2, rstd2):
        self.mask, self.two = mask, mask == 'tensor'
        self.y, self.z, self.msc, self.msh, self.mean, self.rstd, self.y2, self.mean2, self.rstd2 = y, z, msc, msh, mean, rstd, y2, mean2, rstd2
        self.d = dict(y=nhwc(y.float()), z=nhwc(z.float()), y2=nhwc(y2.float()), msc=dev(msc), msh=dev(msh), mean=dev(mean), rstd=dev(rstd),
                      mean2=dev(mean2), rstd2=dev(rstd2))

    def m(self):
        """The mask values: fma(y, msc, msh) as the kernel forms it in fp32, or the mask tensor."""
        if self.two:
            return self.z.double()
        return (self.y.double() * self.msc.double().view(1, -1, 1, 1) + self.msh.double().view(1, -1, 1, 1)).float().double()


class Finalized:
    """NaN-filled partial rows, counters, group scratch and outputs of a dbn_bnb_final for `rows` rows of C channels."""

    def __init__(self, rows, C, two, grad_scale=0.5):
        self.rows, self.C, self.two, self.grad_scale = rows, C, two, grad_scale
        self.part, self.part2 = nan(2, C, rows), nan(2, C, rows)
        self.cnt = torch.zeros(L().dbn_igemm_bn_final_counters(rows, C), device=DEV, dtype=torch.int32)
        self.grp = nan(L().dbn_igemm_bn_final_group_floats(rows, C))
        self.out = [nan(n) for n in (2 * C, C, C, 2 * C, C, C)]
        o = [t.data_ptr() for t in self.out]
        self.rec = _lib.BnbFinal(self.cnt.data_ptr(), self.grp.data_ptr(), o[0], o[1], o[2], o[3] if two else None, o[4] if two else None,
                                 o[5] if two else None, grad_scale)

    def check_counters(self):
        torch.cuda.synchronize()
        assert int(self.cnt.abs().sum()) == 0, 'the finalize left a counter behind'

    def outputs(self):
        return [t.cpu().clone() for t in self.out[:6 if self.two else 3]]

    def refill(self):
        for t in [self.part, self.part2, self.grp] + self.out:
            t.fill_(NAN)


def run_dgrad(case, dy, up, base=None, sums=None, fin=None):
    """dbn_winograd_dgrad_bnsums_f32: dx [N, Cd, H, W] = [base +] the data gradient of the conv Cd -> Ci with dy [N, Ci, H, W]."""
    N, Ci, Cs, Cd, H, W = case
    dys = nhwc(pad_c(dy.float(), Cs))
    dx = nan(N, H, W, Cd) if base is None else nhwc(base.float())
    a = [None] * 12
    if sums is not None:
        d, two = sums.d, sums.two
        a = [d['y'].data_ptr(), d['z'].data_ptr() if two else None, None if two else d['msc'].data_ptr(), None if two else d['msh'].data_ptr(),
             d['mean'].data_ptr(), d['rstd'].data_ptr(), fin.part.data_ptr(), d['y2'].data_ptr() if two else None, d['mean2'].data_ptr() if two else None,
             d['rstd2'].data_ptr() if two else None, fin.part2.data_ptr() if two else None, ctypes.byref(fin.rec)]
    _lib.check(L().dbn_winograd_dgrad_bnsums_f32(dys.data_ptr(), up.data_ptr(), dx.data_ptr(), N, H, W, Cs, Cd, 0 if base is None else 1, *a, stream()),
               'winograd dgrad')
    torch.cuda.synchronize()
    return nchw(dx)


# ---- forward and data gradient: exact data ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fwd_dense_case(case):
    N, Ci, Cs, Cd, H, W = case
    x, w, b = R.dense_x((N, Ci, H, W), 21), R.dense_w((Cd, Ci, 3, 3), 22, winograd=True), R.dense_bias(Cd, 23)
    res = R.dense_bias(N * Cd * H * W, 26).reshape(N, Cd, H, W)
    return x, w, b, res, R.act_coeffs(Cs, 25)


@pytest.mark.parametrize('case', R.WINO_FWD_CASES)
def test_forward_is_exact_on_dense_dyadic_data(case):
    N, Ci, Cs, Cd, H, W = case
    x, w, b, res, act = fwd_dense_case(case)
    up = pack_wino(w, Cd, Ci, Cs, 0)
    ref = R.conv2d(x, w, b, 1, 1)
    exact('winograd fwd dense %s' % (case, ), run_conv(case, x, up, b)[0], ref)
    exact('winograd fwd dense act %s' % (case, ), run_conv(case, x, up, b, act)[0], R.conv2d(R.apply_act(x, act[0][:Ci], act[1][:Ci]), w, b, 1, 1))
    exact('winograd fwd dense res %s' % (case, ), run_conv_res(case, x, up, b, res), (ref + res).clamp_min(0))


@pytest.mark.parametrize('case', R.WINO_FWD_CASES)
def test_forward_is_exact_on_seam_impulses(case):
    N, Ci, Cs, Cd, H, W = case
    (x, ) = R.impulse_maps(N, Ci, H, W, R.winograd_patch_seams(N, H, W), 0)
    w, b = R.distinct_w(Cd, Ci, 3, 3), R.dense_bias(Cd, 23)
    up = pack_wino(w, Cd, Ci, Cs, 0)
    ref = R.conv2d(x, w, b, 1, 1)
    exact('winograd fwd impulses %s' % (case, ), run_conv(case, x, up, b)[0], ref)
    exact('winograd fwd impulses res %s' % (case, ), run_conv_res(case, x, up, b, fwd_dense_case(case)[3]), (ref + fwd_dense_case(case)[3]).clamp_min(0))


@pytest.mark.parametrize('case', R.WINO_FWD_CASES)
def test_data_gradient_is_exact_on_dense_dyadic_data_and_seam_impulses(case):
    N, Ci, Cs, Cd, H, W = case
    dy, w = R.dense_x((N, Ci, H, W), 24), R.dense_w((Ci, Cd, 3, 3), 22, winograd=True)
    base = R.dense_bias(N * Cd * H * W, 16).reshape(N, Cd, H, W)
    up = pack_wino(w, Cd, Ci, Cs, 1)
    ref = R.conv2d_dgrad(dy, w, 1, 1, H, W)
    exact('winograd dgrad dense %s' % (case, ), run_dgrad(case, dy, up), ref)
    exact('winograd dgrad dense + base %s' % (case, ), run_dgrad(case, dy, up, base), R.accumulate(base, ref))
    (dys, ) = R.impulse_maps(N, Ci, H, W, R.winograd_patch_seams(N, H, W), 0)
    wd = R.distinct_w(Ci, Cd, 3, 3)
    exact('winograd dgrad impulses %s' % (case, ), run_dgrad(case, dys, pack_wino(wd, Cd, Ci, Cs, 1)), R.conv2d_dgrad(dys, wd, 1, 1, H, W))


# ---- forward and data gradient: random data -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fwd_random_case(case):
    N, Ci, Cs, Cd, H, W = case
    x, w, b = rnd(N, Ci, H, W, seed=1), rnd(Cd, Ci, 3, 3, seed=2, scale=(2.0 / (Ci * 9))**0.5), rnd(Cd, seed=3)
    return x, w, b, rnd(N, Cd, H, W, seed=8), (rnd(Cs, seed=6) * 0.5 + 1, rnd(Cs, seed=7))


@pytest.mark.parametrize('case', R.WINO_FWD_CASES)
def test_forward_distance_to_fp64(case):
    N, Ci, Cs, Cd, H, W = case
    x, w, b, res, act = fwd_random_case(case)
    up = pack_wino(w, Cd, Ci, Cs, 0)
    r64, r32 = R.conv2d(x.double(), w.double(), b.double(), 1, 1), F.conv2d(x, w, b, 1, 1)
    distance_ratio('winograd fwd %s' % (case, ), run_conv(case, x, up, b)[0], r64, r32, MARGIN['fwd'])
    xa = act32(x, *act)
    distance_ratio('winograd fwd %s act' % (case, ), run_conv(case, x, up, b, act)[0], R.conv2d(xa.double(), w.double(), b.double(), 1, 1),
                   F.conv2d(xa, w, b, 1, 1), MARGIN['fwd'])
    distance_ratio('winograd fwd %s res' % (case, ), run_conv_res(case, x, up, b, res), (r64 + res.double()).clamp_min(0), (r32 + res).clamp_min(0),
                   MARGIN['fwd'])


@pytest.mark.parametrize('case', R.WINO_FWD_CASES)
def test_data_gradient_distance_to_fp64(case):
    N, Ci, Cs, Cd, H, W = case
    dy, w = rnd(N, Ci, H, W, seed=4), rnd(Ci, Cd, 3, 3, seed=2, scale=(2.0 / (Cd * 9))**0.5)
    base = rnd(N, Cd, H, W, seed=13)
    xg = torch.zeros((N, Cd, H, W), requires_grad=True)
    (d32, ) = torch.autograd.grad(F.conv2d(xg, w, None, 1, 1), xg, dy)
    r64 = R.conv2d_dgrad(dy.double(), w.double(), 1, 1, H, W)
    up = pack_wino(w, Cd, Ci, Cs, 1)
    distance_ratio('winograd dgrad %s' % (case, ), run_dgrad(case, dy, up), r64, d32, MARGIN['dgrad'])
    distance_ratio('winograd dgrad %s + base' % (case, ), run_dgrad(case, dy, up, base), r64 + base.double(), d32 + base, MARGIN['dgrad'])


# ---- the BatchNorm statistics of the forward kernel -----------------------------------------------------------------------------------------
def ulps(a, b):
    return float(((a.double() - b.double()).abs() / (b.abs().double() * 2.0**-23)).max())


@pytest.mark.parametrize('final', [False, True])
@pytest.mark.parametrize('case', R.WINO_FWD_CASES)
def test_statistics_of_a_constant_map_over_ragged_patches(case, final):
    """x = 1 on every pixel and channel, a filter with the centre tap only (1 / 2 or 1 per (co, ci)): y = bias + the row sum of the centre
    taps inside the map, on every pixel; a pixel that a ragged patch computes OUTSIDE the map sees zero padding only and holds the bare
    bias.  Every row's pivot is the in-map constant and its sums are 0: save_mean is the constant bit for bit, the variance 0 (save_rstd = 1 /
    sqrt(eps) to 2 ulp), run_var' = (1 - momentum) run_var bit for bit — unless an out-of-map pixel was counted, or a row's count is off.
    With the activation on load the map is relu(scale + shift) per channel, still zero outside."""
    N, Ci, Cs, Cd, H, W = case
    x = torch.ones((N, Ci, H, W), dtype=torch.float64)
    w = torch.zeros((Cd, Ci, 3, 3), dtype=torch.float64)
    w[:, :, 1, 1] = R._ints((Cd, Ci), 1, 2, 27) / 2
    b = R.dense_bias(Cd, 23)
    gamma, beta, rm, rv = bn = bn_params(Cd)
    up = pack_wino(w, Cd, Ci, Cs, 0)
    one_m = torch.tensor(1.0) - torch.tensor(MOM, dtype=torch.float32)
    act = R.act_coeffs(Cs, 25)
    for tag, a, xin in (('plain', None, x), ('act', act, R.apply_act(x, act[0][:Ci], act[1][:Ci]))):
        const = b + (w[:, :, 1, 1] * xin[0, :, 0, 0].view(1, Ci)).sum(1)
        assert bool(((const - b).abs() >= 0.5).all()), 'an out-of-map pixel would not show'
        y, st = run_conv(case, x, up, b, a, bn, final)
        tag = 'constant map %s %s final %d' % (case, tag, final)
        exact(tag + ' y', y, const.view(1, Cd, 1, 1).expand(N, Cd, H, W))
        exact(tag + ' save_mean', st['mean'], const)
        rstd = torch.full((Cd, ), 1.0 / float(torch.tensor(EPS, dtype=torch.float32))**0.5, dtype=torch.float64).float()
        assert ulps(st['rstd'], rstd) <= 2, tag + ': save_rstd %r' % st['rstd'][:4]
        exact(tag + ' run_var', st['run_var'], one_m * rv)
        exact(tag + ' scale', st['scale'], gamma * st['rstd'])
        ms = st['mean'].double() * st['scale'].double()
        within(tag + ' shift', st['shift'], beta.double() - ms, U * (beta.double().abs() + ms.abs()))
        rmean = (1 - MOM) * rm.double() + MOM * const
        within(tag + ' run_mean', st['run_mean'], rmean, 3 * U * ((1 - MOM) * rm.double()).abs() + 2 * U * MOM * const.abs() + U * rmean.abs())


def stats_bounds(y, row, piv, gamma, beta, rm, rv):
    """float64 statistics of the kernel's own output y [N, C, H, W] (fp32 values) and the bounds of its epilogue's chain (csrc/winograd_f32.hip
    "optional BatchNorm statistics", bn_finalize_tiles_kernel / dbn_bn_stats_finish) — stats_bounds of tests/test_fpn_fp64_gpu.py with the
    conv's own error e = 0, since the reference is taken from the very values the kernel summed.  A row — the in-map pixels of one patch or of
    32 consecutive tiles, n_t <= 128 — takes its first pixel as the pivot p_t and sums v = y - p_t (one fp32 rounding) and v v (three) in
    fp32 in some order: any order of n additions errs by at most (n - 1) u sum |terms|, so E1_t = 128 u sum |v|, E2_t = 130 u sum v^2.
    The merge is float64 (exact to 2^-53, dropped): d var / d s1_t = 2 (p_t - mean) / M.  With E1 = sum_t E1_t / M:
      mean (cast to fp32):  bm = E1 + u |mean|
      var:   Ev = sum_t E2_t / M + 2 sum_t (|p_t - mean| + bm) E1_t / M + E1^2
      rstd, scale, shift, running statistics: from bm and Ev as there."""
    N, C, H, W = y.shape
    M = N * H * W
    yc = y.double().permute(1, 0, 2, 3).reshape(C, M)
    r = row.reshape(M)
    rows = piv.shape[0]
    pv = y.double()[piv[:, 0], :, piv[:, 1], piv[:, 2]].t()  # [C, rows]
    v = (yc - pv[:, r]).abs()
    e1 = 128 * U * torch.zeros(C, rows, dtype=torch.float64).index_add_(1, r, v)
    e2 = 130 * U * torch.zeros(C, rows, dtype=torch.float64).index_add_(1, r, v * v)
    mean = yc.mean(1)
    var = ((yc - mean.view(C, 1))**2).mean(1)
    E1, E2 = e1.sum(1) / M, e2.sum(1) / M
    bm = E1 + U * mean.abs()
    Ev = E2 + 2 * (((pv - mean.view(C, 1)).abs() + bm.view(C, 1)) * e1).sum(1) / M + E1**2
    rstd = 1.0 / torch.sqrt(var + EPS)
    gam, bet = gamma.double(), beta.double()
    ref = dict(mean=mean, rstd=rstd, scale=gam * rstd, shift=bet - mean * gam * rstd)
    b = dict(mean=bm)
    er = 0.5 * Ev * ((var - Ev).clamp_min(0) + EPS)**-1.5
    br = b['rstd'] = er + U * (rstd + er)
    bs = b['scale'] = gam.abs() * br + U * gam.abs() * (rstd + br)
    A = bm * ref['scale'].abs() + (mean.abs() + bm) * bs
    b['shift'] = A + U * ((mean * ref['scale']).abs() + bet.abs() + A)
    fM = M / (M - 1.0)
    unb = var * fM
    bu = Ev * fM + U * (unb + Ev * fM)
    ref['run_mean'] = (1 - MOM) * rm.double() + MOM * mean
    ref['run_var'] = (1 - MOM) * rv.double() + MOM * unb
    b['run_mean'] = MOM * bm + 3 * U * ((1 - MOM) * rm.double()).abs() + 2 * U * MOM * (mean.abs() + bm)
    b['run_var'] = MOM * bu + 3 * U * ((1 - MOM) * rv.double()).abs() + 2 * U * MOM * (unb + bu)
    return ref, b


@pytest.mark.parametrize('final', [False, True])
@pytest.mark.parametrize('case', R.WINO_FWD_CASES)
def test_statistics_on_random_data_against_fp64_of_the_stored_output(case, final):
    N, Ci, Cs, Cd, H, W = case
    x, w, b, _, act = fwd_random_case(case)
    bn = bn_params(Cd)
    up = pack_wino(w, Cd, Ci, Cs, 0)
    row, piv = R.wino_rows(N, H, W, R.WINO_FWD_PLAN[case][0] == 'lin')
    plain = run_conv(case, x, up, b)[0]
    for tag, a in (('plain', None), ('act', act)):
        y, st = run_conv(case, x, up, b, a, bn, final)
        if a is None:
            same_bits('the statistics epilogue changed the convolution result', y, plain)
        ref, bound = stats_bounds(y, row, piv, *bn)
        for k in ('mean', 'rstd', 'scale', 'shift', 'run_mean', 'run_var'):
            within('statistics %s %s final %d %s' % (case, tag, final, k), st[k], ref[k], bound[k])


# ---- the BatchNorm-backward sums and their in-kernel finalize ---------------------------------------------------------------------------------
BIG = 4.0  # y, zmask, y2 of the random-data sums: four times the usual size


@functools.lru_cache(maxsize=None)
def sums_args(N, C, H, W):
    """y, zmask, y2 and the per-channel coefficients of the two BatchNorms over a gradient of shape [N, C, H, W]."""
    # y and msc on the 2^-6 grid, msh an odd multiple of 2^-13: fma(y, msc, msh) is an odd multiple of 2^-13 below 2^10 — exact in fp32, so
    # the recomputed mask cannot differ from the float64 one by round-off, and never zero
    grid = lambda t: torch.round(t * 64) / 64
    arg = dict(y=grid(rnd(N, C, H, W, seed=7) * BIG), z=rnd(N, C, H, W, seed=12) * BIG, msc=grid(rnd(C, seed=10)),
               msh=grid(rnd(C, seed=11, scale=0.3)) + 2.0**-13, mean=rnd(C, seed=8, scale=0.2), rstd=rnd(C, seed=9).abs() + 0.5,
               y2=rnd(N, C, H, W, seed=21) * BIG, mean2=rnd(C, seed=22, scale=0.3), rstd2=rnd(C, seed=23).abs() + 0.4)
    assert int((arg['msh'] > 0).sum()) >= 8 and int((arg['msh'] < 0).sum()) >= 8
    return arg


@functools.lru_cache(maxsize=None)
def sums_random_case(case):
    N, Ci, Cs, Cd, H, W = case
    dy, w = rnd(N, Ci, H, W, seed=4), rnd(Ci, Cd, 3, 3, seed=2, scale=(2.0 / (Cd * 9))**0.5)
    return dy, w, rnd(N, Cd, H, W, seed=13), sums_args(N, Cd, H, W), R.conv2d_dgrad(dy.double(), w.double(), 1, 1, H, W)


def backward_fold(fin, sums, dx, M):
    """dbn_bn_backward_t on the partial rows of `fin` (sums_parts = rows): its dgamma, dbeta for the first BatchNorm."""
    C = fin.C
    d = sums.d
    dxd = nhwc(dx.float())
    out, dg, db, ones = nan(*dxd.shape), nan(C), nan(C), torch.ones(C, device=DEV)
    ws = reduce_ws()
    two = sums.two
    _lib.check(L().dbn_bn_backward_t(0, fin.part.data_ptr(), fin.rows, d['y'].data_ptr(), d['z'].data_ptr() if two else None,
                                     None if two else d['msc'].data_ptr(), None if two else d['msh'].data_ptr(), dxd.data_ptr(), d['mean'].data_ptr(),
                                     d['rstd'].data_ptr(), ones.data_ptr(), out.data_ptr(), None, 0, dg.data_ptr(), db.data_ptr(), None, M, C,
                                     fin.grad_scale, ws.data_ptr(), stream()), 'bn backward from the partial rows')
    torch.cuda.synchronize()
    return dg.cpu(), db.cpu()


def check_sums(tag, fin, sums, dx, M, runs, exactly=False):
    """The folded partial rows and the finalized outputs of `fin` against float64 sums over dx as stored; runs: the finalized outputs of the
    launches on the same counters.  exactly: bit for bit (data on which every sum is exact in fp32)."""
    C = fin.C
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            same_bits(tag + ': finalized outputs of two launches', a, b)
    s1, s2, a1, a2 = R.bn_backward_sums(dx, sums.y, sums.mean, sums.rstd, sums.m())
    sc = float(a1.max()) + 1e-9
    gs = fin.grad_scale
    c1c2, dgamma, dbeta = runs[0][:3]
    cmp = (lambda t, got, ref, atol: exact(tag + ' ' + t, got, ref)) if exactly else (lambda t, got, ref, atol: report(tag + ' ' + t, got, ref, atol, 1e-5))
    part = fin.part.cpu()
    if exactly:  # (a1 / M, a2 / M in fp32: the kernel multiplies by fl(1 / M))
        invM = float(torch.tensor(1.0) / torch.tensor(float(M)))
        c12 = torch.stack([s1, s2]) * invM
        cmp('partial rows folded', part.double().sum(2), torch.stack([s1, s2]), 0)
    else:
        c12 = torch.stack([s1, s2]) / M
        cmp('partial rows folded', part.double().sum(2), torch.stack([s1, s2]), 2e-6 * sc)
    cmp('c1, c2', c1c2.view(2, C), c12.float() if exactly else c12, 2e-6 * sc / M)
    cmp('dgamma', dgamma, gs * s2, 2e-6 * sc)
    cmp('dbeta', dbeta, gs * s1, 2e-6 * sc)
    if sums.two:
        t1, t2, _, _ = R.bn_backward_sums(dx, sums.y2, sums.mean2, sums.rstd2, sums.m())
        d12 = torch.stack([t1, t2]) * invM if exactly else torch.stack([t1, t2]) / M
        cmp('second BatchNorm: partial rows folded', fin.part2.cpu().double().sum(2), torch.stack([t1, t2]), 2e-6 * sc)
        cmp('second BatchNorm: c1, c2', runs[0][3].view(2, C), d12.float() if exactly else d12, 2e-6 * sc / M)
        cmp('second BatchNorm: dgamma', runs[0][4], gs * t2, 2e-6 * sc)
        cmp('second BatchNorm: dbeta', runs[0][5], gs * t1, 2e-6 * sc)
    # the other route to dgamma / dbeta: dbn_bn_backward_t folds all rows in float64; the kernel rounds every 64-row group's float64 sum to
    # fp32 before it adds the groups — one group: the same bits; several: within 2^-23 of sum |rows| per channel (+ the final rounding)
    dg, db = backward_fold(fin, sums, dx, M)
    if fin.rows <= 64 or exactly:
        same_bits(tag + ' dgamma against dbn_bn_backward_t', dgamma, dg)
        same_bits(tag + ' dbeta against dbn_bn_backward_t', dbeta, db)
    else:
        ab = part.double().abs().sum(2) * gs
        within(tag + ' dgamma against dbn_bn_backward_t', dgamma, dg, 2 * U * ab[1] + 2 * U * dg.double().abs())
        within(tag + ' dbeta against dbn_bn_backward_t', dbeta, db, 2 * U * ab[0] + 2 * U * db.double().abs())


@pytest.mark.parametrize('mask,accumulate', [('self', 0), ('self', 1), ('tensor', 0), ('tensor', 1), ('none', 0), ('none', 1)])
@pytest.mark.parametrize('case', R.WINO_FINAL_CASES + R.WINO_PATCH_CASES[:2])
def test_data_gradient_sums_and_their_finalize(case, mask, accumulate):
    N, Ci, Cs, Cd, H, W = case
    dy, w, old, arg, dx64 = sums_random_case(case)
    base = old if accumulate else None
    up = pack_wino(w, Cd, Ci, Cs, 1)
    plain = run_dgrad(case, dy, up, base)
    if mask == 'none':
        xg = torch.zeros((N, Cd, H, W), requires_grad=True)
        (d32, ) = torch.autograd.grad(F.conv2d(xg, w, None, 1, 1), xg, dy)
        distance_ratio('winograd dgrad %s acc %d' % (case, accumulate), plain, dx64 + (old.double() if accumulate else 0),
                       d32 + (old if accumulate else 0), MARGIN['dgrad'])
        return
    sums = Sums(mask, **arg)
    if mask == 'self':  # the kernel evaluates fma(y, sc, sh) in fp32: exact on this grid, and no value at round-off level
        m64 = sums.y.double() * sums.msc.double().view(1, -1, 1, 1) + sums.msh.double().view(1, -1, 1, 1)
        assert torch.equal(sums.m(), m64) and bool((m64.abs() >= 2.0**-13).all())
    fin = Finalized(L().dbn_winograd_rows(N, H, W), Cd, sums.two)
    runs = []
    for rep in range(2):  # twice: the second launch relies on the counters the first one left behind
        fin.refill()
        dx = run_dgrad(case, dy, up, base, sums, fin)
        fin.check_counters()
        runs.append(fin.outputs())
        same_bits('the sums epilogue changed the data gradient', dx, plain)
    check_sums('winograd sums %s %s acc %d' % (case, mask, accumulate), fin, sums, dx, N * H * W, runs)


@pytest.mark.parametrize('mask,accumulate', [('self', 0), ('tensor', 1)])
@pytest.mark.parametrize('case', R.WINO_FINAL_CASES + R.WINO_PATCH_CASES[:1])
def test_data_gradient_sums_are_exact_on_small_dyadic_data(case, mask, accumulate):
    """conv_ref.wino_sums_data: dx, every partial row, both levels of the finalize and its outputs are exact in fp32 (tests/test_winograd_cases_cpu.py),
    so they equal float64 bit for bit — and the float64 fold of dbn_bn_backward_t as well."""
    N, Ci, Cs, Cd, H, W = case
    d = R.wino_sums_data(case, accumulate)
    sums = Sums(mask, d['y'], d['z'], d['msc'], d['msh'], d['mean'], d['rstd'], d['y2'], d['mean2'], d['rstd2'])
    fin = Finalized(L().dbn_winograd_rows(N, H, W), Cd, sums.two)
    up = pack_wino(d['w'], Cd, Ci, Cs, 1)
    runs = []
    for rep in range(2):
        fin.refill()
        dx = run_dgrad(case, d['dy'], up, d['base'], sums, fin)
        fin.check_counters()
        runs.append(fin.outputs())
    exact('winograd dgrad small data %s' % (case, ), dx, d['dx'])
    check_sums('winograd exact sums %s %s acc %d' % (case, mask, accumulate), fin, sums, dx, N * H * W, runs, exactly=True)


@pytest.mark.parametrize('mask,accumulate', [('self', 0), ('tensor', 1)])
@pytest.mark.parametrize('case', R.IGEMM_FINAL_CASES)
def test_implicit_gemm_data_gradient_sums_and_their_finalize(case, mask, accumulate):
    """dbn_igemm_bnsums_t (fp32 MFMA, tile hint 0, mode 1) with 64, 65 and 132 partial rows: one full group, a last group of one row, three
    groups over the four parity classes of a stride-2 gradient."""
    N, Ci, Co, k, s, p, H, W = case
    Ho, Wo = R.out_size(H, k, s, p), R.out_size(W, k, s, p)
    w = rnd(Co, Ci, k, k, seed=2, scale=(2.0 / (Ci * k * k))**0.5)
    dy, old = rnd(N, Co, Ho, Wo, seed=4), rnd(N, Ci, H, W, seed=13)
    sums = Sums(mask, **sums_args(N, Ci, H, W))
    rows = L().dbn_igemm_bn_rows(0, 0, N, Ho, Wo, Co, H, W, Ci, k, k, s, p, 1, 0)
    assert rows == R.IGEMM_FINAL_PLAN[case]
    fin = Finalized(rows, Ci, sums.two)
    wpk = pack(w, 1, s)
    dys = nhwc(dy)
    fresh = lambda: nhwc(old) if accumulate else nan(N, H, W, Ci)
    plain = fresh()
    igemm_t(dys, wpk, None, plain, k, s, p, 1, accumulate, 0, ns=0)
    d, two = sums.d, sums.two
    runs = []
    for rep in range(2):
        fin.refill()
        dx = fresh()
        _lib.check(L().dbn_igemm_bnsums_t(0, 0, dys.data_ptr(), wpk.data_ptr(), None, dx.data_ptr(), N, Ho, Wo, Co, H, W, Ci, k, k, s, p, 1, accumulate, 0,
                                          d['y'].data_ptr(), d['z'].data_ptr() if two else None, None if two else d['msc'].data_ptr(),
                                          None if two else d['msh'].data_ptr(), d['mean'].data_ptr(), d['rstd'].data_ptr(), fin.part.data_ptr(),
                                          d['y2'].data_ptr() if two else None, d['mean2'].data_ptr() if two else None,
                                          d['rstd2'].data_ptr() if two else None, fin.part2.data_ptr() if two else None, ctypes.byref(fin.rec),
                                          stream()), 'igemm_bnsums')
        fin.check_counters()
        runs.append(fin.outputs())
        same_bits('the sums epilogue changed the data gradient', dx.cpu(), plain.cpu())
    check_sums('igemm sums %s %s acc %d' % (case, mask, accumulate), fin, sums, nchw(dx), N * H * W, runs)
