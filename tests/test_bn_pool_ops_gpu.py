"""-m gpu: operation-level pins of the BatchNorm, stem-pool, nearest-upsample and Adam kernels of csrc/pointwise.hip against float64, in
every storage type they accept (at = 0 fp32, 1 bf16, 2 fp16), to the standard of tests/test_train16_ops_gpu.py:

  (a) dbn_bn_train_stats_t            (b) dbn_bn_apply_t            (c) dbn_bn_backward_t (reduce + finalize + apply, dbias_conv, sums)
  (d) dbn_bnrelu_maxpool_fwd_t / _bwd_t (+ bn_part), dbn_bnrelu_maxpool_fwd_arg_t / dbn_maxpool_bn_backward_t
  (e) dbn_nearest_up_fwd_t / _bwd_t   (f) dbn_adam_step             and the refusals of (a) and (c)

The reference is tests/bn_pool_ref.py in float64 on the operands AS STORED (rounded to the storage type first), evaluated on the GPU from
elementwise operations and reductions; tests/test_bn_pool_ref_cpu.py checks it against torch.  Every output starts as NaN and every
workspace is NaN-poisoned.  Bounds are elementwise: u = 2^-24 (U), s = SR[at] the storage type's unit roundoff, eta = ETA[at]; an fp32
serial chain of `depth` adds errs by at most (depth + c) u sum|terms|, c counting the roundings inside a term, sum|terms| taken in float64;
the chain of channel_reduce is col_sum_depth(M, C) (rows per thread + row lanes), the partials are folded in float64.  Exact cases use
dyadic operands with few significant bits, so that every fp32 and storage operation is exact and the kernel must equal float64 bit for bit;
their gradients sit on the seams of the row split (first / last row of every block, of every 1024-channel chunk)."""
import math

import pytest
import torch
import torch.nn.functional as F

import bn_pool_ref as R
from gpu_util import DEV, DT, ETA, NAN, SR, U, L, col_sum_depth, exact, gen, stream, within
from db_text_minimal_amd import _lib

pytestmark = pytest.mark.gpu

CAP_M = 768 * 64 + 1  # the 768-block cap of part_blocks: 65 rows per block, the trailing blocks own no rows
RED_CASES = [(1, 4), (2, 8), (63, 20), (65, 48), (130, 1024), (193, 2048), (40, 4096), (CAP_M, 64), (CAP_M, 2048)]
EPS = float(torch.tensor(1e-5, dtype=torch.float32))  # the float the entry point receives
MOM = float(torch.tensor(0.1, dtype=torch.float32))
GS = float(torch.tensor(0.7, dtype=torch.float32))  # a grad_scale that is no power of two, as the float the entry points receive
ATS = [0, 1, 2]


def ws_for(C):
    return torch.full((L().dbn_reduce_ws_floats(C), ), NAN, device=DEV)


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def ptr(t):
    return None if t is None else t.data_ptr()


def pick(vals, n, g):
    return torch.tensor(vals, device=DEV)[torch.randint(0, len(vals), (n, ), generator=g, device=DEV)]


# ------------------------------------------------------------------------------------------------------------------------------------
# (a) dbn_bn_train_stats_t
# ------------------------------------------------------------------------------------------------------------------------------------
HARD = ('const', 'ratio', 'row0', 'corner')


def padded_corner(M, seed):
    """M pixels (row-major, from pixel (0, 0)) of a real 3 x 3 zero-padded convolution of all-positive data with positive weights: row 0
    is the corner pixel, which sees 4 of the 9 taps."""
    g = torch.Generator().manual_seed(seed)
    W = min(M, 61)
    H = -(-M // W)
    img = torch.rand(1, 1, H, W, generator=g) + 0.5
    w = torch.rand(1, 1, 3, 3, generator=g) + 0.5
    return F.conv2d(img, w, padding=1).flatten()[:M].to(DEV)


def stats_data(M, C, at, seed):
    """Random channels (mean in +-8, spread 2^-6 .. 2^3) and, in the first and the last channel quad, the hard ones: a constant channel;
    |mean| / spread = 2^10; row 0 sixty-four spreads from the rest; the padded-corner channel."""
    g = gen(seed)
    mean = torch.rand(C, generator=g, device=DEV) * 16 - 8
    spread = torch.exp2(torch.rand(C, generator=g, device=DEV) * 9 - 6)
    x = torch.randn(M, C, generator=g, device=DEV) * spread + mean
    hard = {k: [] for k in HARD}
    for i, base in enumerate([0] if C < 8 else [0, C - 4]):
        x[:, base] = 3.25 - 5 * i
        x[:, base + 1] = 64 + torch.randn(M, generator=g, device=DEV) * 2.0**-4
        x[:, base + 2] = torch.randn(M, generator=g, device=DEV) * 0.5 + 1
        x[0, base + 2] += 32
        x[:, base + 3] = padded_corner(M, seed + i)
        for j, k in enumerate(HARD):
            hard[k].append(base + j)
    return x.to(DT[at]), hard


def stats_run(at, x, gamma, beta, rm, rv, eps=EPS, momentum=MOM):
    M, C = x.shape
    out = {k: nan(C) for k in ('scale', 'shift', 'mean', 'rstd')}
    out['run_mean'], out['run_var'] = (None, None) if rm is None else (rm.clone(), rv.clone())
    ws = ws_for(C)
    _lib.check(L().dbn_bn_train_stats_t(at, x.data_ptr(), M, C, gamma.data_ptr(), beta.data_ptr(), eps, momentum, ptr(out['run_mean']),
                                        ptr(out['run_var']), out['scale'].data_ptr(), out['shift'].data_ptr(), out['mean'].data_ptr(),
                                        out['rstd'].data_ptr(), ws.data_ptr(), stream()), 'bn_train_stats_t')
    torch.cuda.synchronize()
    return out


def stats_bounds(x, gamma, beta, rm, rv, momentum=MOM):
    """float64 reference and the bounds of bn_stats_kernel + bn_finalize_kernel.  With p = row 0 (the pivot) and v = x - p (one fp32
    rounding), a thread chains S1 = sum v and S2 = sum v v (v v: 3 roundings) over depth = col_sum_depth(M, C) adds; the fold, dm = S1 / M,
    mean = p + dm, var = S2 / M - dm^2 and 1 / sqrt(var + eps) are float64:
      E1 = (depth + 2) u sum|v|, E2 = (depth + 4) u sum v^2
      mean (cast to fp32):  bm = E1 / M + u |mean|
      var:   Ev = E2 / M + 2 |dm| E1 / M + (E1 / M)^2   (it grows with sum (x - pivot)^2: loose by construction when row 0 is an outlier)
      rstd:  e = Ev / 2 (max(var - Ev, 0) + eps)^-3/2 (the derivative's largest value on the interval), br = e + u (rstd + e)
      scale = gamma rstd (1 rounding):  bs = |gamma| br + u |gamma| (rstd + br)
      shift = fma(-mean, scale, beta):  A = bm |scale| + (|mean| + bm) bs, bsh = A + u (|mean scale| + |beta| + A)
      running = (1 - m) old + m new in fp32, (1 - m) itself rounded: 3 roundings on the first product, 2 on the second:
             brm = m bm + 3 u |(1 - m) rm| + 2 u m (|mean| + bm);  with unb = var M / (M - 1) cast to fp32, bu = Ev f + u (unb + Ev f):
             brv = m bu + 3 u |(1 - m) rv| + 2 u m (unb + bu)."""
    M, C = x.shape
    xd, gam, bet = x.double(), gamma.double(), beta.double()
    ref = R.bn_stats(xd, gam, bet, EPS, momentum, None if rm is None else rm.double(), None if rv is None else rv.double())
    d = col_sum_depth(M, C)
    v = xd - xd[0]
    dm = v.sum(0) / M
    E1, E2 = (d + 2) * U * v.abs().sum(0), (d + 4) * U * (v * v).sum(0)
    del v
    b = {}
    bm = b['mean'] = E1 / M + U * ref['mean'].abs()
    Ev = b['var'] = E2 / M + 2 * dm.abs() * E1 / M + (E1 / M)**2
    e = 0.5 * Ev * ((ref['var'] - Ev).clamp_min(0) + EPS)**-1.5
    br = b['rstd'] = e + U * (ref['rstd'] + e)
    bs = b['scale'] = gam.abs() * br + U * gam.abs() * (ref['rstd'] + br)
    A = bm * ref['scale'].abs() + (ref['mean'].abs() + bm) * bs
    b['shift'] = A + U * ((ref['mean'] * ref['scale']).abs() + bet.abs() + A)
    if rm is not None:
        f = M / (M - 1.0) if M > 1 else 1.0
        bu = Ev * f + U * (ref['unbiased'] + Ev * f)
        b['run_mean'] = momentum * bm + 3 * U * ((1 - momentum) * rm.double()).abs() + 2 * U * momentum * (ref['mean'].abs() + bm)
        b['run_var'] = momentum * bu + 3 * U * ((1 - momentum) * rv.double()).abs() + 2 * U * momentum * (ref['unbiased'] + bu)
    return ref, b


def stats_params(C, seed):
    g = gen(seed)
    r = lambda s=1.0: torch.randn(C, generator=g, device=DEV) * s
    return r(0.3) + 1, r(), r(), r().abs() + 0.5  # gamma, beta, running mean, running var


@pytest.mark.parametrize('at', ATS)
@pytest.mark.parametrize('M,C', RED_CASES)
def test_bn_stats_random_and_hard_channels_vs_fp64(M, C, at):
    """save_mean, save_rstd, scale, shift and the running statistics on stats_data against float64 within stats_bounds; without running
    statistics (NULL) the other four outputs are the same bits."""
    x, _ = stats_data(M, C, at, seed=M + C)
    gamma, beta, rm, rv = stats_params(C, seed=C)
    out = stats_run(at, x, gamma, beta, rm, rv)
    ref, b = stats_bounds(x, gamma, beta, rm, rv)
    for k in ('mean', 'rstd', 'scale', 'shift', 'run_mean', 'run_var'):
        within('bn stats %s M=%d C=%d at=%d' % (k, M, C, at), out[k], ref[k], b[k])
    out2 = stats_run(at, x, gamma, beta, None, None)
    for k in ('mean', 'rstd', 'scale', 'shift'):
        assert torch.equal(out[k], out2[k]), k + ': differs without running statistics'


STATS_EXACT = [(1, 4), (2, 8), (64, 20), (128, 48), (256, 1024), (128, 2048), (64, 4096), (65536, 64), (65536, 2048)]


@pytest.mark.parametrize('at', ATS)
@pytest.mark.parametrize('M,C', STATS_EXACT)
def test_bn_stats_exact(M, C, at):
    """x = {-4 .. 4} 2^k (k per channel in [-2, 2]; channel 0 constant), M a power of two (65536 rows: the 768-block cap with empty
    trailing blocks), gamma a power of two, running mean a multiple of 1/4, momentum 1/4: S1, S2, the mean and the new running mean are
    exactly representable -> save_mean and running_mean bit-exact, scale = gamma save_rstd bit-exact, rstd within two roundings (2 u) of
    float64, the rest within stats_bounds."""
    g = gen(M * 3 + C)
    k = torch.randint(-2, 3, (C, ), generator=g, device=DEV).float()
    x = torch.randint(-4, 5, (M, C), generator=g, device=DEV).float() * torch.exp2(k)
    x[:, 0] = 3.0
    x = x.to(DT[at])
    gamma, beta = pick([0.5, 1.0, 2.0, -1.0], C, g), pick([-1.0, -0.5, 0.0, 0.5, 1.0], C, g)
    rm, rv = torch.randint(-8, 9, (C, ), generator=g, device=DEV).float() / 4, pick([0.5, 1.0, 1.5], C, g)
    out = stats_run(at, x, gamma, beta, rm, rv, momentum=0.25)
    ref, b = stats_bounds(x, gamma, beta, rm, rv, momentum=0.25)
    tag = 'bn stats exact M=%d C=%d at=%d ' % (M, C, at)
    exact(tag + 'mean', out['mean'], ref['mean'])
    exact(tag + 'running mean', out['run_mean'], ref['run_mean'])
    exact(tag + 'scale / gamma', out['scale'], gamma.double() * out['rstd'].double())
    within(tag + 'rstd', out['rstd'], ref['rstd'], 2 * U * ref['rstd'])
    for kk in ('shift', 'run_var'):
        within(tag + kk, out[kk], ref[kk], b[kk])


@pytest.mark.parametrize('at', ATS)
def test_bn_stats_pivot_on_outlier_rows_measured(at):
    """The pivot (row 0) on channels where row 0 is NOT typical, at M = 768 x 64 + 1, C = 64: prints the kernel's relative error in var
    and rstd against float64 and, beside it, the error of fp32 torch.native_batch_norm on the CPU (what F.batch_norm runs) against the
    same float64 values.  Asserted on the padded-corner channels: 16-bit storage: rstd error <= SR[at], the roundoff of the activations
    it normalises; fp32: <= 8 x the fp32 reference's own error (the margin: serial chains where torch reduces pairwise).
    Measured on an MI355X (relative errors, worst of the two channels of a kind; kernel | torch fp32):
      fp32  row 0 at 64 spreads  var 2.9e-05 rstd 1.5e-05 | var 3.5e-08 rstd 5.6e-08     padded corner  var 1.5e-07 rstd 7.6e-08 | var 1.8e-08 rstd 3.7e-08
      bf16  row 0 at 64 spreads  var 7.6e-05 rstd 3.8e-05 | var 3.9e-08 rstd 2.3e-08     padded corner  var 6.6e-08 rstd 3.3e-08 | var 7.6e-08 rstd 3.8e-08
      fp16  row 0 at 64 spreads  var 7.5e-06 rstd 3.7e-06 | var 1.7e-08 rstd 3.8e-08     padded corner  var 3.1e-07 rstd 1.5e-07 | var 2.7e-08 rstd 2.8e-08
    The padded corner (about 6 spreads from the mean) costs a factor 2 to 5 against a two-pass fp32 reduction and meets the criterion; a
    row 0 at 64 spreads costs 2 to 3 decimal digits of rstd (still below the roundoff of 16-bit activations, 260 u in fp32)."""
    M, C = CAP_M, 64
    x, hard = stats_data(M, C, at, seed=M + C)
    gamma, beta, _, _ = stats_params(C, seed=C)
    out = stats_run(at, x, gamma, beta, None, None)
    xd = x.double()
    ref = R.bn_stats(xd, gamma.double(), beta.double(), EPS)
    var_k = (1.0 / out['rstd'].double()**2 - EPS)  # (var is not an output: recovered from rstd in float64)
    xc = x.float().cpu().t().reshape(1, C, M, 1).contiguous()
    rm_t, rv_t = torch.zeros(C), torch.ones(C)
    _, _, invstd_t = torch.native_batch_norm(xc, gamma.cpu(), beta.cpu(), rm_t, rv_t, True, 1.0, EPS)
    var_t = rv_t.double() * (M - 1.0) / M  # momentum 1: running_var = the unbiased variance
    rel = lambda got, want: ((got.double().cpu() - want.cpu()).abs() / want.cpu().abs())
    res = {}
    for kind in ('row0', 'corner'):
        ch = hard[kind]
        res[kind] = (float(rel(var_k, ref['var'])[ch].max()), float(rel(out['rstd'], ref['rstd'])[ch].max()),
                     float(rel(var_t, ref['var'])[ch].max()), float(rel(invstd_t, ref['rstd'])[ch].max()))
        print('bn stats pivot at=%d %-6s: kernel var %.3e rstd %.3e | torch fp32 var %.3e rstd %.3e' % ((at, kind) + res[kind]))
    k_rstd, t_rstd = res['corner'][1], res['corner'][3]
    if at == 0:
        assert k_rstd <= 8 * t_rstd, 'padded corner: kernel rstd error %.3e > 8 x the fp32 reference\'s %.3e' % (k_rstd, t_rstd)
    else:
        assert k_rstd <= SR[at], 'padded corner: kernel rstd error %.3e > storage roundoff %.3e' % (k_rstd, SR[at])


# ------------------------------------------------------------------------------------------------------------------------------------
# (b) dbn_bn_apply_t
# ------------------------------------------------------------------------------------------------------------------------------------
# M x C; items = M C / 4 (fp32, and 16-bit with C % 8 != 0: the narrow form) or M C / 8 (16-bit wide), never a multiple of 256 x UNROLL;
# (3073, 2048) and (CAP_M, 64) exceed the 768 x 256 x UNROLL items of one pass of the grid (16-bit wide: 3073 x 256; fp32: both)
APPLY_CASES = [(3, 8), (37, 64), (63, 20), (5, 1024), (3073, 2048), (CAP_M, 64)]
APPLY_FORMS = {'plain': (False, False, 0), 'relu': (False, False, 1), 'res_relu': (True, False, 1), 'res_affine': (True, True, 0)}


def apply_run(at, y, sc, sh, res, rsc, rsh, relu):
    M, C = y.shape
    out = nan(M, C, dtype=DT[at])
    _lib.check(L().dbn_bn_apply_t(at, y.data_ptr(), sc.data_ptr(), sh.data_ptr(), ptr(res), ptr(rsc), ptr(rsh), out.data_ptr(), M, C, relu,
                                  stream()), 'bn_apply_t')
    torch.cuda.synchronize()
    return out


def apply_ref(y, sc, sh, res, rsc, rsh, relu):
    """float64 reference and the fp32 evaluation error: a = fma(y, sc, sh) (1 rounding), b = res or fma(res, rsc, rsh), out = a + b
    (1 rounding of the computed sum), ReLU (1-Lipschitz): e32 = u (|a| + |b|) + u (|a + b| + u (|a| + |b|)), without a residual u |a|."""
    d = lambda t: None if t is None else t.double()
    a = y.double() * sc.double() + sh.double()
    ref = R.bn_apply(y.double(), sc.double(), sh.double(), d(res), d(rsc), d(rsh), bool(relu))
    if res is None:
        return ref, U * a.abs()
    b = d(res) * d(rsc) + d(rsh) if rsc is not None else d(res)
    ab = a.abs() + b.abs()
    return ref, U * ab + U * ((a + b).abs() + U * ab)


@pytest.mark.parametrize('at', ATS)
@pytest.mark.parametrize('M,C', APPLY_CASES)
def test_bn_apply_forms_vs_fp64(M, C, at):
    """The four forms on random operands: |out - ref| <= e32 + s (|ref| + e32) + eta (apply_ref; one storage rounding of the fp32
    value); then on dyadic operands (y, res integers in [-4, 4], scales in {+-1/2, 1, 2}, shifts multiples of 1/2: every value a multiple
    of 1/2 below 32) bit-exact."""
    s, eta = SR[at], ETA[at]
    g = gen(M + C + at)
    r = lambda *shape, sc=1.0: torch.randn(*shape, generator=g, device=DEV) * sc
    y, res = r(M, C).to(DT[at]), r(M, C).to(DT[at])
    sc, sh, rsc, rsh = r(C, sc=0.3) + 1, r(C), r(C, sc=0.3) - 1, r(C)
    yi = torch.randint(-4, 5, (M, C), generator=g, device=DEV).to(DT[at])
    ri = torch.randint(-4, 5, (M, C), generator=g, device=DEV).to(DT[at])
    sci, rsci = pick([-0.5, 0.5, 1.0, 2.0], C, g), pick([-0.5, 0.5, 1.0, 2.0], C, g)
    shi, rshi = pick([-1.0, -0.5, 0.0, 0.5, 1.0], C, g), pick([-1.0, -0.5, 0.0, 0.5, 1.0], C, g)
    for form, (with_res, with_aff, relu) in APPLY_FORMS.items():
        args = (y, sc, sh, res if with_res else None, rsc if with_aff else None, rsh if with_aff else None, relu)
        ref, e32 = apply_ref(*args)
        within('bn apply %s M=%d C=%d at=%d' % (form, M, C, at), apply_run(at, *args), ref, e32 + s * (ref.abs() + e32) + eta)
        args = (yi, sci, shi, ri if with_res else None, rsci if with_aff else None, rshi if with_aff else None, relu)
        exact('bn apply exact %s M=%d C=%d at=%d' % (form, M, C, at), apply_run(at, *args), apply_ref(*args)[0])


@pytest.mark.parametrize('at', ATS)
@pytest.mark.parametrize('C', [8, 20])
def test_bn_apply_relu_seam(C, at):
    """Pre-activations exactly +0, -0, +-the smallest subnormal and +-the smallest normal value of the storage type (scale 1, shift 0,
    and through the residual form with a zero residual), and y sc + sh = 0 with sc = 1/2, sh = -1, y = 2: ReLU gives +0 for everything
    that is not positive and passes the smallest positive values unchanged (bit-exact)."""
    dt, it = DT[at], torch.int16 if at else torch.int32
    tiny_sub = {0: 2.0**-149, 1: 2.0**-133, 2: 2.0**-24}[at]
    tiny = float(torch.finfo(dt).tiny)
    seam = torch.tensor([0.0, -0.0, tiny_sub, -tiny_sub, tiny, -tiny, 1.0, -1.0], dtype=torch.float64)
    M = 2 * 8 + 3
    yc = seam.repeat(-(-M * C // 8))[:M * C].view(M, C).to(dt)  # (converted on the CPU; compared as bit patterns throughout)
    assert torch.equal(yc.double().view(-1)[:8], seam)  # (the storage type holds them)
    want = torch.where(yc.double() > 0, yc.double(), torch.zeros(M, C, dtype=torch.float64)).to(dt).view(it)  # +0 for all that is not positive
    y = yc.to(DEV)
    one, zero = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    for tag, res in (('relu', None), ('res_relu', torch.zeros(M, C, device=DEV, dtype=dt))):
        out = apply_run(at, y, one, zero, res, None, None, 1)
        ne = out.cpu().view(it) != want
        assert not bool(ne.any()), 'bn apply seam %s C=%d at=%d: %d elements differ, the first at %d' % (tag, C, at, int(ne.sum()),
                                                                                                        int(ne.view(-1).nonzero()[0]))
    y2 = torch.full((M, C), 2.0, device=DEV, dtype=dt)
    out = apply_run(at, y2, one * 0.5, -one, None, None, None, 1)
    assert not bool((out.cpu().view(it) != 0).any()), 'relu(fma(2, 1/2, -1)) is not +0'


# ------------------------------------------------------------------------------------------------------------------------------------
# (c) dbn_bn_backward_t
# ------------------------------------------------------------------------------------------------------------------------------------
BWD_CASES = RED_CASES + [(67, 4)]  # (67, 4): dbias_conv on 16-bit storage with C % 8 != 0, where `wide` falls back to the narrow form
MASKS = ['zmask', 'recomputed', 'none']


def stream_grid(total, Cq):
    """bn_stream_grid of csrc/pointwise.hip: min(ceil(total / 256), 768) blocks, rounded up to a multiple of (Cq / 4) / gcd(Cq / 4, 256)."""
    g = min(max(-(-total // 256), 1), 768)
    m = (Cq // 4) // math.gcd(Cq // 4, 256)
    return -(-g // m) * m


def bias_depth(at, M, C):
    """Chain of the in-apply bias gradient: a thread adds its ceil(items / threads) items, then 256 / cin threads are added in LDS."""
    wide = at != 0 and C % 8 == 0
    cin = C // (8 if wide else 4)
    total = M * cin
    return -(-total // (stream_grid(total, C // 2 if wide else C) * 256)) + 256 // cin


def bwd_run(at, y, dout, mean, rstd, gamma, zmask=None, msc=None, msh=None, gout=None, gout_acc=0, gs=1.0, dbias=False, sums=None,
            parts=0):
    M, C = y.shape
    out = {'dy': nan(M, C, dtype=DT[at]), 'dgamma': nan(C), 'dbeta': nan(C), 'gout': gout, 'dbias': nan(C) if dbias else None}
    ws = ws_for(C)
    _lib.check(L().dbn_bn_backward_t(at, ptr(sums), parts, y.data_ptr(), ptr(zmask), ptr(msc), ptr(msh), dout.data_ptr(), mean.data_ptr(),
                                     rstd.data_ptr(), gamma.data_ptr(), out['dy'].data_ptr(), ptr(gout), gout_acc, out['dgamma'].data_ptr(),
                                     out['dbeta'].data_ptr(), ptr(out['dbias']), M, C, gs, ws.data_ptr(), stream()), 'bn_backward_t')
    torch.cuda.synchronize()
    return out


def bwd_dy_bound(at, ref, gamma, rstd, M, e1, e2):
    """bn_bwd_apply_kernel in fp32: xh = (y - mean) rstd (2 roundings), gr = gamma rstd (1), dy = gr ((g - c1) - xh c2): with
    A = |g| + |c1| + |xh c2| the roundings of g - c1 (1), xh c2 (3) and their difference (1) stay below 4 u A, the product with gr adds
    2 u: 7 u A with the second-order terms; the errors e1, e2 of c1, c2 enter as e1 + |xh| e2.
    e32 = |gamma rstd| (e1 + |xh| e2 + 7 u A);  stored: e32 + s (|dy| + e32) + eta."""
    A = ref['g'].abs() + ref['c1'].abs() + (ref['xhat'] * ref['c2']).abs()
    e32 = (gamma.double() * rstd.double()).abs() * (e1 + ref['xhat'].abs() * e2 + 7 * U * A)
    return e32 + SR[at] * (ref['dy'].abs() + e32) + ETA[at]


def bwd_check(tag, at, y, dout, mean, rstd, gamma, mask, gs, out, d1, d2, is_exact=False, gout_old=None, abs_terms=None):
    """dgamma / dbeta: the chains of d1 / d2 adds (channel_reduce: d1 = depth + 2: exact terms, d2 = depth + 5: g ((y - mean) rstd) has 3
    roundings), folded in float64, times grad_scale, cast once: |gs| d u sum|terms| + u |ref|; c1, c2 = the sums / M, cast once:
    e1 = d1 u sum|g| / M + u |c1|, e2 likewise; dy: bwd_dy_bound.  is_exact: dgamma and dbeta must equal float64 bit for bit.
    abs_terms: the float64 sums of |terms| of the two chains where the kernel's terms are not the per-row g and g xhat.
    gout (the masked dout): the stored operand itself, or fp32 g + old stored once: s |ref| + (1 + s) u |ref| + eta."""
    M, C = y.shape
    ref = R.bn_backward(y.double(), dout.double(), mean.double(), rstd.double(), gamma.double(), mask, gs)
    if abs_terms is not None:
        ref['abs1'], ref['abs2'] = abs_terms
    if is_exact:
        exact(tag + ' dbeta', out['dbeta'], ref['dbeta'])
        exact(tag + ' dgamma', out['dgamma'], ref['dgamma'])
    else:
        within(tag + ' dbeta', out['dbeta'], ref['dbeta'], abs(gs) * d1 * U * ref['abs1'] + U * ref['dbeta'].abs())
        within(tag + ' dgamma', out['dgamma'], ref['dgamma'], abs(gs) * d2 * U * ref['abs2'] + U * ref['dgamma'].abs())
    e1 = d1 * U * ref['abs1'] / M + U * ref['c1'].abs()
    e2 = d2 * U * ref['abs2'] / M + U * ref['c2'].abs()
    within(tag + ' dy', out['dy'], ref['dy'], bwd_dy_bound(at, ref, gamma, rstd, M, e1, e2))
    if out['gout'] is not None:
        if gout_old is None:
            exact(tag + ' gout', out['gout'], ref['g'])
        else:
            gref = ref['g'] + gout_old.double()
            within(tag + ' gout (acc)', out['gout'], gref, (SR[at] + (1 + SR[at]) * U) * gref.abs() + ETA[at])
    if out['dbias'] is not None:  # the float64 column sum of the dy the kernel returned, as stored
        dyk = out['dy'].double()
        bref = dyk.sum(0) * gs
        within(tag + ' dbias_conv', out['dbias'], bref, abs(gs) * (bias_depth(at, M, C) + 2) * U * dyk.abs().sum(0) + U * bref.abs())
    return ref


def bwd_inputs(M, C, at, seed):
    g = gen(seed)
    r = lambda *shape, sc=1.0: torch.randn(*shape, generator=g, device=DEV) * sc
    return {'y': (r(M, C) * 2 + 1).to(DT[at]), 'dout': r(M, C).to(DT[at]), 'z': r(M, C).to(DT[at]), 'mean': r(C, sc=0.3) + 1,
            'rstd': torch.rand(C, generator=g, device=DEV) + 0.3, 'gamma': r(C, sc=0.3) + 1, 'msc': r(C, sc=0.3) + 0.5, 'msh': r(C) - 0.5}


def mask_args(form, t):
    if form == 'zmask':
        return {'zmask': t['z']}, R.bn_mask(t['y'].double(), zmask=t['z'].double())
    if form == 'recomputed':  # the sign of the kernel's fma is the sign of the float64 y msc + msh (the product is exact in float64)
        return {'msc': t['msc'], 'msh': t['msh']}, R.bn_mask(t['y'].double(), mask_scale=t['msc'].double(), mask_shift=t['msh'].double())
    return {}, None


@pytest.mark.parametrize('at', ATS)
@pytest.mark.parametrize('form', MASKS)
@pytest.mark.parametrize('M,C', BWD_CASES)
def test_bn_backward_random_vs_fp64(M, C, form, at):
    """Reduce + finalize + apply on random operands with grad_scale fp32(0.7) (bounds: bwd_check), gout absent / written / accumulated onto
    a non-zero tensor (one each, by mask form), and dbias_conv wherever the entry point accepts it (256 % (C / 4) == 0)."""
    t = bwd_inputs(M, C, at, seed=M + 2 * C)
    kw, mask = mask_args(form, t)
    gs = GS
    gout_mode = MASKS.index(form)  # zmask: written, recomputed: accumulated, none: absent
    old = torch.randn(M, C, generator=gen(5), device=DEV).to(DT[at]) if gout_mode == 1 else None
    gout = nan(M, C, dtype=DT[at]) if gout_mode == 0 else old.clone() if gout_mode == 1 else None
    dbias = 256 % (C // 4) == 0
    out = bwd_run(at, t['y'], t['dout'], t['mean'], t['rstd'], t['gamma'], gout=gout, gout_acc=int(gout_mode == 1), gs=gs, dbias=dbias, **kw)
    d = col_sum_depth(M, C)
    bwd_check('bn bwd %s M=%d C=%d at=%d' % (form, M, C, at), at, t['y'], t['dout'], t['mean'], t['rstd'], t['gamma'], mask, gs, out, d + 2,
              d + 5, gout_old=old)


def seam_rows(M):
    """Row 0, row M - 1, and the last row of every block's range with the first of the next (part_blocks: nb = min(ceil(M / 64), 768)
    blocks of ceil(M / nb) rows)."""
    nb = min(max(-(-M // 64), 1), 768)
    rows_per = -(-M // nb)
    rows = {0, M - 1}
    for k in range(rows_per, M, rows_per):
        rows |= {k - 1, k}
    return torch.tensor(sorted(rows), device=DEV)


@pytest.mark.parametrize('at', ATS)
@pytest.mark.parametrize('form', MASKS)
@pytest.mark.parametrize('M,C', BWD_CASES)
def test_bn_backward_exact_on_the_seams(M, C, form, at):
    """y, the saved activation: integers in [-4, 4]; mean in {-1/2, 0, 1/2}, rstd in {1/2, 1, 2}, mask scale / shift dyadic, grad_scale
    1/4; dout = {+-1, +-2} / 16 on the seam rows (seam_rows) in EVERY channel (so in the first quad of every 1024-channel chunk), zero
    elsewhere: g xhat is a multiple of 2^-6 below 2 and at most 2 x 768 rows are non-zero, so every partial sum is exact and dgamma, dbeta
    must equal float64 bit for bit: a dropped, doubled or misplaced row at a block or chunk boundary, or a stale partial of an empty
    trailing block (the workspace is NaN), cannot hide.  dy and dbias_conv stay within the bounds of bwd_check."""
    g = gen(M * 5 + C)
    dt = DT[at]
    rows = seam_rows(M)
    dout = torch.zeros(M, C, device=DEV)
    dout[rows] = pick([-2.0, -1.0, 1.0, 2.0], len(rows) * C, g).view(len(rows), C) / 16
    t = {'y': torch.randint(-4, 5, (M, C), generator=g, device=DEV).to(dt), 'dout': dout.to(dt),
         'z': torch.randint(-4, 5, (M, C), generator=g, device=DEV).to(dt), 'mean': pick([-0.5, 0.0, 0.5], C, g),
         'rstd': pick([0.5, 1.0, 2.0], C, g), 'gamma': pick([-1.0, 0.5, 1.0, 2.0], C, g), 'msc': pick([-1.0, 0.5, 1.0], C, g),
         'msh': pick([-1.0, -0.5, 0.0, 0.5], C, g)}
    kw, mask = mask_args(form, t)
    out = bwd_run(at, t['y'], t['dout'], t['mean'], t['rstd'], t['gamma'], gs=0.25, dbias=256 % (C // 4) == 0, **kw)
    d = col_sum_depth(M, C)
    bwd_check('bn bwd exact %s M=%d C=%d at=%d' % (form, M, C, at), at, t['y'], t['dout'], t['mean'], t['rstd'], t['gamma'], mask, 0.25, out,
              d + 2, d + 5, is_exact=True)


@pytest.mark.parametrize('at', [1, 2])
@pytest.mark.parametrize('parts', [37, 513])
def test_bn_backward_from_given_partial_sums_on_16bit_storage(parts, at):
    """`sums` = [2][C][parts] fp32 partials produced elsewhere (37: the 32-lane team fold, 513: the 256-thread fold), 16-bit tensors:
    the folds are float64, so dgamma / dbeta = the float64 sum of the given partials times grad_scale, cast once (u |ref|), c1 / c2
    likewise (e = u |c|), dy within bwd_dy_bound."""
    M, C, gs = 240, 64, GS
    t = bwd_inputs(M, C, at, seed=parts)
    kw, mask = mask_args('zmask', t)
    ref = R.bn_backward(t['y'].double(), t['dout'].double(), t['mean'].double(), t['rstd'].double(), t['gamma'].double(), mask, gs)
    s12 = torch.stack([ref['dbeta'], ref['dgamma']]) / gs
    wts = torch.rand(2, C, parts, generator=gen(3), device=DEV, dtype=torch.float64) + 0.1
    part = (s12.unsqueeze(2) * wts / wts.sum(2, keepdim=True)).float().contiguous()
    out = bwd_run(at, t['y'], t['dout'], t['mean'], t['rstd'], t['gamma'], gs=gs, sums=part, parts=parts, **kw)
    tot = part.double().sum(2)
    tag = 'bn bwd given sums parts=%d at=%d' % (parts, at)
    within(tag + ' dbeta', out['dbeta'], tot[0] * gs, U * (tot[0] * gs).abs())
    within(tag + ' dgamma', out['dgamma'], tot[1] * gs, U * (tot[1] * gs).abs())
    ref['c1'], ref['c2'] = tot[0] / M, tot[1] / M
    ref['dy'] = t['gamma'].double() * t['rstd'].double() * (ref['g'] - ref['c1'] - ref['xhat'] * ref['c2'])
    within(tag + ' dy', out['dy'], ref['dy'], bwd_dy_bound(at, ref, t['gamma'], t['rstd'], M, U * ref['c1'].abs(), U * ref['c2'].abs()))


@pytest.mark.parametrize('C', [6, 1536, 8192])
def test_bn_stats_and_backward_refuse_unsupported_channel_counts(C):
    """C % 4 != 0, a C above 1024 that is no multiple of 1024, and C > 4096: a non-zero status, nothing launched, outputs untouched."""
    M = 4
    x = torch.zeros(M, C, device=DEV)
    vec = torch.ones(C, device=DEV)
    outs = [nan(C) for _ in range(4)]
    ws = torch.full((1024 * 2 * C, ), NAN, device=DEV)
    rc = L().dbn_bn_train_stats_t(0, x.data_ptr(), M, C, vec.data_ptr(), vec.data_ptr(), EPS, MOM, None, None, *(o.data_ptr() for o in outs),
                                  ws.data_ptr(), stream())
    torch.cuda.synchronize()
    assert rc != 0 and all(bool(torch.isnan(o).all()) for o in outs)
    dy, dg, db = nan(M, C), nan(C), nan(C)
    rc = L().dbn_bn_backward_t(0, None, 0, x.data_ptr(), None, None, None, x.data_ptr(), vec.data_ptr(), vec.data_ptr(), vec.data_ptr(),
                               dy.data_ptr(), None, 0, dg.data_ptr(), db.data_ptr(), None, M, C, 1.0, ws.data_ptr(), stream())
    torch.cuda.synchronize()
    assert rc != 0 and all(bool(torch.isnan(o).all()) for o in (dy, dg, db))
    assert bool(torch.isnan(ws).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# (d) the stem's pool family
# ------------------------------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(1, 1, 1), (2, 2, 1), (1, 1, 9), (1, 7, 9), (3, 16, 12), (2, 33, 47)]
POOL_C = [8, 64, 256]  # 256 % (C / 4) == 0: every form; 20 in addition for the plain forward / backward (the narrow 16-bit form)


def pool_inputs(kind, at, N, H, W, C, seed):
    """'dyadic': y integers in [-4, 4], scale in {-1, +-1/2, 1, 2}, shift a multiple of 1/2: z = relu(y sc + sh) is a multiple of 1/2
    below 16, exact in every type, and most windows hold TIES; dpool in {-2 .. 2} / 16.  'random': y, dpool random; scale and shift
    bf16-VALUED, so that y sc + sh is exact in float64 and its rounding to fp32 is the kernel's fma bit for bit."""
    g = gen(seed)
    dt = DT[at]
    Ho, Wo = R.pool_out(H), R.pool_out(W)
    if kind == 'dyadic':
        y = torch.randint(-4, 5, (N, H, W, C), generator=g, device=DEV).to(dt)
        sc, sh = pick([-1.0, -0.5, 0.5, 1.0, 2.0], C, g), pick([-1.0, -0.5, 0.0, 0.5, 1.0], C, g)
        dp = (torch.randint(-2, 3, (N, Ho, Wo, C), generator=g, device=DEV).float() / 16).to(dt)
    else:
        y = torch.randn(N, H, W, C, generator=g, device=DEV).to(dt)
        sc = (torch.randn(C, generator=g, device=DEV) * 0.5 + 1).bfloat16().float()
        sh = (torch.randn(C, generator=g, device=DEV) * 0.3).bfloat16().float()
        dp = torch.randn(N, Ho, Wo, C, generator=g, device=DEV).to(dt)
    return y, sc, sh, dp


def pool_z(y, sc, sh, at):
    """relu(fma(y, sc, sh)) as the kernels see it: rounded to fp32 (bit-exact: see pool_inputs), then to the storage type (the backward
    compares the ROUNDED activation with the stored maximum)."""
    return (y.double() * sc.double() + sh.double()).float().clamp_min(0).to(DT[at]).double()


def pool_fwd_run(at, y, sc, sh):
    N, H, W, C = y.shape
    out = nan(N, R.pool_out(H), R.pool_out(W), C, dtype=DT[at])
    _lib.check(L().dbn_bnrelu_maxpool_fwd_t(at, y.data_ptr(), sc.data_ptr(), sh.data_ptr(), out.data_ptr(), N, H, W, C, stream()), 'pool fwd')
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('at', ATS)
@pytest.mark.parametrize('kind', ['dyadic', 'random'])
@pytest.mark.parametrize('N,H,W', POOL_SHAPES)
def test_pool_forward_exact(N, H, W, kind, at):
    """dbn_bnrelu_maxpool_fwd_t = max over the 3 x 3 / 2 / 1 window of relu(fma(y, sc, sh)), rounded to the storage type (rounding is
    monotone: the maximum of the rounded values): bit-exact on both kinds of pool_inputs, C = 8, 64, 256 and 20."""
    for C in POOL_C + [20]:
        y, sc, sh, _ = pool_inputs(kind, at, N, H, W, C, seed=H * W + C)
        exact('pool fwd %s %s C=%d at=%d' % ((N, H, W), kind, C, at), pool_fwd_run(at, y, sc, sh), R.pool_fwd(pool_z(y, sc, sh, at)))


def pool_parts_depth(N, H, W, C, parts):
    """bnrelu_maxpool_bwd_kernel: an item is a 2 x 2 pixel block of a channel quad (4 adds per item), threads stride the items by
    parts x 256, then 256 / (C / 4) threads are added in LDS."""
    cin = C // 4
    total = N * ((H + 1) // 2) * ((W + 1) // 2) * cin
    return 4 * -(-total // (parts * 256)) + 256 // cin


@pytest.mark.parametrize('at', ATS)
@pytest.mark.parametrize('kind', ['dyadic', 'random'])
@pytest.mark.parametrize('N,H,W', POOL_SHAPES)
def test_pool_backward_and_its_batchnorm_sums(N, H, W, kind, at):
    """dbn_bnrelu_maxpool_bwd_t: dz = [z > 0] sum of dpool over the windows whose stored maximum EQUALS the rounded z (every tying
    position receives the gradient: the kernel's documented rule, R.pool_bwd_all_ties; on tie-free data autograd's).
    'dyadic' (ties in most windows): bit-exact.  'random': at most 4 terms in an fp32 chain, stored once: 3 u sum|terms| + s |ref| + eta.
    With bn_part (C = 8, 64, 256) dz is the same bits, and the partial sums fed to dbn_bn_backward_t as `sums` give the dgamma / dbeta
    (and dy) of float64 on the dz the kernel stored, within the chain of pool_parts_depth (+ 2; + 5 for dz ((y - mean) rstd))."""
    M, gs = N * H * W, 0.5
    for C in POOL_C + [20]:
        y, sc, sh, dp = pool_inputs(kind, at, N, H, W, C, seed=H * W + C + 1)
        z = pool_z(y, sc, sh, at)
        pooled = pool_fwd_run(at, y, sc, sh)
        dz = nan(N, H, W, C, dtype=DT[at])
        _lib.check(L().dbn_bnrelu_maxpool_bwd_t(at, y.data_ptr(), sc.data_ptr(), sh.data_ptr(), pooled.data_ptr(), dp.data_ptr(), dz.data_ptr(),
                                                N, H, W, C, None, None, None, stream()), 'pool bwd')
        torch.cuda.synchronize()
        ref = R.pool_bwd_all_ties(z, pooled.double(), dp.double())
        tag = 'pool bwd %s %s C=%d at=%d' % ((N, H, W), kind, C, at)
        if kind == 'dyadic':
            exact(tag, dz, ref)
        else:
            within(tag, dz, ref, 3 * U * R.pool_bwd_all_ties(z, pooled.double(), dp.double().abs()) + SR[at] * ref.abs() + ETA[at])
        if C == 20:
            continue
        g = gen(C)
        mean, rstd = torch.randn(C, generator=g, device=DEV) * 0.3, torch.rand(C, generator=g, device=DEV) + 0.5
        gamma = torch.randn(C, generator=g, device=DEV) * 0.3 + 1
        if kind == 'dyadic':
            mean, rstd = pick([-0.5, 0.0, 0.5], C, g), pick([0.5, 1.0, 2.0], C, g)
        nparts = L().dbn_maxpool_bwd_parts(N, H, W, C)
        parts = nan(2 * C * nparts)
        dz2 = nan(N, H, W, C, dtype=DT[at])
        _lib.check(L().dbn_bnrelu_maxpool_bwd_t(at, y.data_ptr(), sc.data_ptr(), sh.data_ptr(), pooled.data_ptr(), dp.data_ptr(), dz2.data_ptr(),
                                                N, H, W, C, mean.data_ptr(), rstd.data_ptr(), parts.data_ptr(), stream()), 'pool bwd + bn_part')
        torch.cuda.synchronize()
        assert torch.equal(dz.view(torch.int16 if at else torch.int32), dz2.view(torch.int16 if at else torch.int32)), tag + ': bn_part changed dz'
        out = bwd_run(at, y.view(M, C), dz.view(M, C), mean, rstd, gamma, gs=gs, sums=parts, parts=nparts)
        d = pool_parts_depth(N, H, W, C, nparts)
        bwd_check(tag + ' bn_part', at, y.view(M, C), dz.view(M, C), mean, rstd, gamma, None, gs, out, d + 2, d + 5, is_exact=kind == 'dyadic')


@pytest.mark.parametrize('at', ATS)
@pytest.mark.parametrize('kind', ['dyadic', 'random'])
@pytest.mark.parametrize('N,H,W', POOL_SHAPES)
def test_pool_with_recorded_argmax_and_backward_through_batchnorm(N, H, W, kind, at):
    """dbn_bnrelu_maxpool_fwd_arg_t: the pooled value bit-exact; the code of every window is 15 exactly where the pooled value is 0 and
    otherwise names a position inside the image whose rounded z EQUALS the maximum (WHICH of several tying positions is not asserted), and
    ypool is y at that position.  dbn_maxpool_bn_backward_t: with g = every window's dpool on the one position its code names,
    dbeta = gs sum g = gs sum of dpool over the windows with a positive maximum (each pooled gradient lands on exactly one input), dgamma and
    dy as the BatchNorm backward of float64 on g: maxpool_bn_stats_kernel chains ceil(items / (parts x 256)) adds per thread and
    256 / (C / 4) in LDS (+ 2; + 5 for g ((ypool - mean) rstd)) over its per-WINDOW terms, folded in float64; dy: bwd_dy_bound.  'dyadic':
    dgamma, dbeta bit-exact."""
    M, gs = N * H * W, 0.5
    Ho, Wo = R.pool_out(H), R.pool_out(W)
    for C in POOL_C:
        y, sc, sh, dp = pool_inputs(kind, at, N, H, W, C, seed=H * W + C + 2)
        z = pool_z(y, sc, sh, at)
        pooled, ypool = nan(N, Ho, Wo, C, dtype=DT[at]), nan(N, Ho, Wo, C, dtype=DT[at])
        idx = torch.full((N, Ho, Wo, C), 77, device=DEV, dtype=torch.uint8)
        _lib.check(L().dbn_bnrelu_maxpool_fwd_arg_t(at, y.data_ptr(), sc.data_ptr(), sh.data_ptr(), pooled.data_ptr(), idx.data_ptr(),
                                                    ypool.data_ptr(), N, H, W, C, stream()), 'pool fwd arg')
        torch.cuda.synchronize()
        tag = 'pool arg %s %s C=%d at=%d' % ((N, H, W), kind, C, at)
        pref = R.pool_fwd(z)
        exact(tag + ' pooled', pooled, pref)
        live = idx != 15
        assert not bool(((idx > 8) & live).any()), tag + ': a code outside 0..8 / 15'
        assert torch.equal(live, pref > 0), tag + ': code 15 does not mark exactly the zero maxima'
        oh, ow = torch.arange(Ho, device=DEV).view(1, Ho, 1, 1), torch.arange(Wo, device=DEV).view(1, 1, Wo, 1)
        ih, iw = (2 * oh - 1 + idx // 3)[live], (2 * ow - 1 + idx % 3)[live]
        assert bool(((ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)).all()), tag + ': a code names a padding position'
        exact(tag + ' z at the code', R.pool_gather_codes(z, idx), pref)
        exact(tag + ' ypool', ypool.double() * live, R.pool_gather_codes(y.double(), idx))
        assert bool(torch.isfinite(ypool.float()).all())
        g_ = gen(C + 1)
        mean, rstd = torch.randn(C, generator=g_, device=DEV) * 0.3, torch.rand(C, generator=g_, device=DEV) + 0.5
        gamma = torch.randn(C, generator=g_, device=DEV) * 0.3 + 1
        if kind == 'dyadic':
            mean, rstd = pick([-0.5, 0.0, 0.5], C, g_), pick([0.5, 1.0, 2.0], C, g_)
        out = {'dy': nan(N, H, W, C, dtype=DT[at]), 'dgamma': nan(C), 'dbeta': nan(C), 'gout': None, 'dbias': None}
        ws = torch.full((L().dbn_maxpool_bn_backward_ws_floats(N, H, W, C), ), NAN, device=DEV)
        _lib.check(L().dbn_maxpool_bn_backward_t(at, y.data_ptr(), dp.data_ptr(), idx.data_ptr(), ypool.data_ptr(), mean.data_ptr(),
                                                 rstd.data_ptr(), gamma.data_ptr(), out['dy'].data_ptr(), out['dgamma'].data_ptr(),
                                                 out['dbeta'].data_ptr(), N, H, W, C, gs, ws.data_ptr(), stream()), 'pool + bn bwd')
        torch.cuda.synchronize()
        gref = R.pool_bwd_from_codes(idx, dp.double(), H, W)
        pooled4 = N * Ho * Wo * (C // 4)
        nparts = min(max(-(-pooled4 // 256), 1), 2048)
        d = -(-pooled4 // (nparts * 256)) + 256 // (C // 4)
        out['dy'] = out['dy'].view(M, C)
        # the kernel's terms are per WINDOW (dpool and dpool xhat(ypool)); two windows may land on one input with gradients that cancel
        gw = dp.double() * live
        xh = (y.double() - mean.double()) * rstd.double()
        abs_terms = gw.abs().sum((0, 1, 2)), (gw * R.pool_gather_codes(xh, idx)).abs().sum((0, 1, 2))
        ref = bwd_check(tag + ' bn bwd', at, y.view(M, C), gref.view(M, C), mean, rstd, gamma, None, gs, out, d + 2, d + 5,
                        is_exact=kind == 'dyadic', abs_terms=abs_terms)
        once = (dp.double() * live).sum((0, 1, 2)) * gs  # every pooled gradient on exactly one input, whichever tie took it
        assert float((ref['dbeta'] - once).abs().max()) <= 1e-12 * max(float(once.abs().max()), 1.0)


# ------------------------------------------------------------------------------------------------------------------------------------
# (e) dbn_nearest_up_fwd_t / dbn_nearest_up_bwd_t
# ------------------------------------------------------------------------------------------------------------------------------------
UP_SHAPES = [(4, 4, 8, 8), (2, 3, 8, 12), (1, 1, 8, 8), (3, 5, 7, 9), (8, 8, 8, 8)]  # (hs, ws, h, w) of test_ops_gpu.test_nearest_upsample


@pytest.mark.parametrize('at', ATS)
@pytest.mark.parametrize('hs,ws,h,w', UP_SHAPES)
def test_nearest_upsample_forward_add_and_concat(hs, ws, h, w, at):
    """A copy plus at most one fp32 addition, stored once: bit-exact against float64 rounded to fp32 and then to the storage type (the
    kernel's own two roundings; the float64 sum of two stored values is exact).  Concat at coff = 0, 64, 68 of 256 destination channels
    (68: coff % 8 != 0, the narrow 16-bit form): the channels outside [coff, coff + C) keep their NaN poison."""
    N, C, dt = 2, 64, DT[at]
    g = gen(hs * 7 + w)
    a = torch.randn(N, hs, ws, C, generator=g, device=DEV).to(dt)
    b = torch.randn(N, h, w, C, generator=g, device=DEV).to(dt)
    up = R.nearest_up(a.double(), h, w)
    out = nan(N, h, w, C, dtype=dt)
    _lib.check(L().dbn_nearest_up_fwd_t(at, a.data_ptr(), b.data_ptr(), out.data_ptr(), N, hs, ws, C, h, w, C, 0, stream()), 'up add')
    torch.cuda.synchronize()
    exact('upsample + add %s at=%d' % ((hs, ws, h, w), at), out, (up + b.double()).float().to(dt).double())
    for coff in (0, 64, 68):
        cat = nan(N, h, w, 256, dtype=dt)
        _lib.check(L().dbn_nearest_up_fwd_t(at, a.data_ptr(), None, cat.data_ptr(), N, hs, ws, C, h, w, 256, coff, stream()), 'up cat')
        torch.cuda.synchronize()
        exact('upsample concat coff=%d %s at=%d' % (coff, (hs, ws, h, w), at), cat[..., coff:coff + C], up)
        outside = torch.cat([cat[..., :coff], cat[..., coff + C:]], -1)
        assert bool(torch.isnan(outside.float()).all()), 'concat at coff=%d touched channels outside its range' % coff


@pytest.mark.parametrize('at', ATS)
@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('hs,ws,h,w', UP_SHAPES)
def test_nearest_upsample_adjoint(hs, ws, h, w, accumulate, at):
    """dsrc (+)= the sum of dbig[..., coff : coff + C] over the k destination pixels that read the source pixel: an fp32 chain of k terms
    (+ the old value), stored once: (k + 1) u (sum|terms| + |old|) + s |ref| + eta; the other channels of dbig hold NaN (not read).
    coff = 64 and 68 of 256 channels."""
    N, C, dt = 2, 64, DT[at]
    g = gen(hs * 11 + w + accumulate)
    for coff in (64, 68):
        dbig = nan(N, h, w, 256, dtype=dt)
        dbig[..., coff:coff + C] = torch.randn(N, h, w, C, generator=g, device=DEV).to(dt)
        old = torch.randn(N, hs, ws, C, generator=g, device=DEV).to(dt)
        da = old.clone() if accumulate else nan(N, hs, ws, C, dtype=dt)
        _lib.check(L().dbn_nearest_up_bwd_t(at, dbig.data_ptr(), da.data_ptr(), N, hs, ws, C, h, w, 256, coff, accumulate, stream()), 'up bwd')
        torch.cuda.synchronize()
        d64 = dbig[..., coff:coff + C].double()
        o64 = old.double() * accumulate
        ref = R.nearest_up_adjoint(d64, hs, ws) + o64
        k = R.nearest_up_adjoint(torch.ones_like(d64), hs, ws)
        bound = (k + 1) * U * (R.nearest_up_adjoint(d64.abs(), hs, ws) + o64.abs()) + SR[at] * ref.abs() + ETA[at]
        within('upsample adjoint coff=%d acc=%d %s at=%d' % (coff, accumulate, (hs, ws, h, w), at), da, ref, bound)


# ------------------------------------------------------------------------------------------------------------------------------------
# (f) dbn_adam_step
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, 4 * 1003 + 3])
def test_adam_two_steps_vs_fp64(n):
    """Two steps (the second on non-zero moments), each against R.adam_step in float64 on the state the kernel held BEFORE the step, with
    the hyper-parameters as the floats the entry point receives and grad_scale 1/4 (the 1 / world path).  adam_kernel in fp32:
      gg = g gs (1 rounding);  m' = b1 m + (1 - b1) gg ((1 - b) is exact: Sterbenz): |dm| <= 3 u (|b1 m| + |(1 - b1) gg|)
      v' = b2 v + ((1 - b2) gg) gg: positive terms, at most 5 roundings on a term: |dv| <= 5 u v'
      denom = sqrt(v') c2 + eps, c2 = fp32(1 / sqrt(bc2)): 2.5 u (v') + 1 (sqrt) + 2 (c2, product) + 1 (sum) = 6.5 u relative
      p' = p - lrc (m' / denom), lrc = fp32(lr / bc1): |dp| <= lrc (|dm| + 8 u |m'|) / denom + 2 u |lrc m' / denom| + u |p'|
    (a few u relative per element).  n = 1, 3, 5, 1023, 4 x 1003 + 3 run the scalar tail; the buffers are 8 elements longer than n and the
    NaN beyond n must survive."""
    lr, b1, b2, eps = (float(torch.tensor(v, dtype=torch.float32)) for v in (0.005, 0.9, 0.999, 1e-8))
    g = gen(n)
    mk = lambda t: torch.cat([t, nan(8)])
    p, m, v = mk(torch.randn(n, generator=g, device=DEV)), mk(torch.zeros(n, device=DEV)), mk(torch.zeros(n, device=DEV))
    for step, gscale in ((1, 1e-3), (2, 1e-2)):
        grad = mk(torch.randn(n, generator=g, device=DEV) * gscale * 4)
        p0, m0, v0 = p[:n].double(), m[:n].double(), v[:n].double()
        _lib.check(L().dbn_adam_step(p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, b1, b2, eps, step, 0.25, stream()), 'adam')
        torch.cuda.synchronize()
        pr, mr, vr, parts = R.adam_step(p0, grad[:n].double(), m0, v0, lr, b1, b2, eps, step, grad_scale=0.25)
        bm = 3 * U * parts['m_terms']
        tag = 'adam n=%d step %d ' % (n, step)
        within(tag + 'exp_avg', m[:n], mr, bm)
        within(tag + 'exp_avg_sq', v[:n], vr, 5 * U * vr)
        within(tag + 'param', p[:n], pr, parts['lrc'] * (bm + 8 * U * mr.abs()) / parts['denom'] + 2 * U * parts['upd'].abs() + U * pr.abs())
        for name, t in (('param', p), ('exp_avg', m), ('exp_avg_sq', v)):
            assert bool(torch.isnan(t[n:]).all()), tag + name + ': the guard beyond n was written'
