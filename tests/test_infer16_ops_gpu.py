"""-m gpu: operation-level float64 pins of the dedicated 16-bit kernels of csrc/stem16.hip and csrc/convt16.hip and of the forward
head tail of csrc/head_loss.hip, to the standard of tests/test_train16_ops_gpu.py, in every storage type they accept (at = 1 bf16,
2 fp16; dbn_head_tail_fwd_t also 0 fp32):

  dbn_stem16_conv_bn_t            (with dbn_nchw3_to_padded4_t and dbn_stem16_pack on the way in), without / with BatchNorm statistics
  dbn_stem16_conv_bn_relu_pool_t  conv + eval BatchNorm + ReLU + MaxPool2d(3, 2, 1) in one launch
  dbn_convt16_bn_t                ConvTranspose2d(64, 64, 2, 2), without / with statistics, without / with bias
  dbn_pw16_act_t                  Conv2d(64, 64 | 256, 1), relu 0 / 1, bias NULL / given
  dbn_head16_tail_eval_t          ConvT -> BatchNorm -> ReLU -> ConvT(64, 1) -> sigmoid of both branches in one launch
  dbn_head_tail_fwd_t             channels 2 / 3, without / with the fused BatchNorm, both lane forms on 16-bit storage

The reference is tests/infer16_ref.py in float64 on the operands AS STORED (rounded to the storage type first), evaluated on the GPU image
by image.  Every output and workspace starts as NaN.  Three kinds of case per entry point:

  random   elementwise bounds built from u = 2^-24 (U), s = SR[at], eta = ETA[at] and float64 magnitude sums.  Products of two 16-bit
           operands are exact in fp32; an MFMA accumulation of n terms in any order errs by at most n u sum|terms| (n = 224 for the stem:
           14 k-steps of 16, the padding taps included; 64 + 1 for the ConvT / pointwise conv / second ConvT, the bias being the initial
           value); the affine is one fmaf (one rounding), a bias add one rounding, each store to a 16-bit tensor s |v| + eta; ReLU and max
           are 1-Lipschitz (a pooled bound is the maximum of its window's bounds); a logit error d moves a sigmoid by at most d / 4.
  exact    dyadic operands with few significant bits (images and activations small integers, integer weights scaled by a power of two per
           output channel, BatchNorm scale a power of two): every fp32 and storage operation is exact and the kernel must equal float64
           bit for bit; the head maps must lie within SIGMA of the sigmoid of the exactly known logit.  Dense data, and sparse impulses
           on the seams of the walk (first / last pixel of every image, both sides of every 32-pixel block boundary — blocks span images
           at these shapes — the ragged last block, the borders of the stem's 7x7 window), weights differing per (co, ci, tap).
  multi-block  the smallest sizes at which a wave of the persistent walks takes a second and a third block (the prefetch across blocks,
           the statistics carried across blocks, a ragged block as a wave's third; in the pool kernel a wave's second .. fifth task and
           rpc = 5): random, exact and "late" data (non-zero only in the waves' second and third blocks); each test asserts the
           blocks-per-wave count (the pool test the host plan) it relies on.  rpc = 10 and 20 of the pool kernel differ from 5 only in
           the trip count and need the benchmark's own 32 x 1280^2 workload: left out.  dbn_head_tail_fwd_t is no wave walk: a block
           streams one run of `per` pixels, per = 64 up to 2^20 pixels; one case just above (per = 128) runs the eight-lane form's
           unrolled four-pixel trip, which 64-pixel runs never reach.

The sigmoids are __expf + v_rcp_f32, whose error is not derivable.  Measured here against float64 sigmoid on logits that are exact by
construction (test_sigmoid_error_on_exact_logits: k / 8, |k| <= 160, and k / 8 - 1 / 16; every exact case checks it again):
max |error| = SIGMA_MEASURED = 8.753e-8; SIGMA, the allowance, is twice that rounded up to a power of two, 2^-22, well below the 2^-19 (2e-6)
that tests/test_ops_gpu.py grants these maps.  The binary map is checked as a function of the P and T the kernel itself wrote:
B = sigmoid(k (P - T)) with two fp32 roundings in the logit: |B - B64(P, T)| <= k 2 u |P - T| / 4 + SIGMA."""
import pytest
import torch

import infer16_ref as R
from gpu_util import DEV, DT, ETA, NAN, SR, U, L, exact, gen, stream, within
from db_text_minimal_amd import _lib

pytestmark = pytest.mark.gpu

SIGMA_MEASURED = 8.753e-8  # (the largest error printed by test_sigmoid_error_on_exact_logits and by the exact cases: any storage type, both kernels)
SIGMA = 2.0**-22  # 2.38e-7
assert 2 * SIGMA_MEASURED <= SIGMA <= 2.0**-19

ATS = [1, 2]
BLK = 32  # pixels per block of the wave walks
EPS = float(torch.tensor(1e-5, dtype=torch.float32))  # the floats the entry points receive
MOM = float(torch.tensor(0.1, dtype=torch.float32))
KSTEP = 50.0


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def ptr(t):
    return None if t is None else t.data_ptr()


def pick(vals, shape, g):
    n = 1
    for s in shape:
        n *= s
    return torch.tensor(vals, device=DEV, dtype=torch.float32)[torch.randint(0, len(vals), (n, ), generator=g, device=DEV)].reshape(shape)


def ints(lo, hi, shape, g):
    return torch.randint(lo, hi + 1, shape, generator=g, device=DEV).float()


def stored(t, at):
    """The float64 value of t after rounding to the storage type."""
    return t.to(DT[at]).double()


def assert_storable(tag, ref, at):
    """(the construction of an exact case: the float64 result is representable in the storage type)"""
    assert torch.equal(stored(ref, at), ref), tag + ': the exact case is not representable in the storage type'


def store_bound(at, ref, e):
    """A value with fp32-level error bound e, rounded once to the storage type."""
    return e + SR[at] * (ref.abs() + e) + ETA[at]


def walk(M, waves):
    """(blocks, blocks of the busiest wave) of a grid-stride walk of 32-pixel blocks."""
    nblk = -(-M // BLK)
    return nblk, -(-nblk // waves)


def seam_pixels(N, HW, block=BLK):
    """First / last pixel of every image, both sides of every block boundary, the last (ragged) block's first and last pixel."""
    M = N * HW
    px = {0, M - 1}
    for n in range(N):
        px |= {n * HW, n * HW + HW - 1}
    for b in range(block, M, block):
        px |= {b - 1, b}
    return torch.tensor(sorted(px), device=DEV)


def bn_params(seed, dyadic):
    """gamma, beta, running mean, running var (the running statistics away from 0 / 1)."""
    g = gen(seed)
    if dyadic:
        return pick([0.5, 1.0, 2.0, -1.0], (64, ), g), pick([-1.0, -0.5, 0.0, 0.5, 1.0], (64, ), g), ints(-8, 8, (64, ), g) / 4, pick([0.5, 1.5, 2.0], (64, ), g)
    r = lambda s=1.0: torch.randn(64, generator=g, device=DEV) * s
    return r(0.3) + 1, r(), r(), r().abs() + 0.5


def wave_stats_bounds(c, e, waves, gamma, beta, rm, rv):
    """float64 reference and bounds of the train-mode BatchNorm statistics that stem7x7_b16_kernel / convt2x2_b16_kernel +
    bn_finalize_tiles_kernel produce.  c [M, K, 64]: the float64 accumulators (before the output rounding) of pixel m, class k
    (K = 1 stem, 4 ConvT); e: the elementwise bound of the kernel's fp32 accumulator against c (MFMA error; 0 in exact cases).

    The kernel: wave w = (m / 32) mod waves takes the pivot p_w = its first block's row 0, class 0; every lane chains S1 = sum d and
    S2 = sum d d over d = acc - p_w (one rounding; d d one more; no contraction) through Lc = 16 registers x K classes x blocks adds,
    + 1 for the exchange of the two half waves.  With D = |c - p_w| + e + e_pivot >= |d|:
      E1_w = (Lc + 1) u sum_w D,   E2_w = (Lc + 3) u sum_w D^2
    bn_finalize_tiles_kernel shifts every wave's sums to p_0 in float64 (exact algebra): a1 = sum_w S1_w + n_w d_w, a2 = sum_w S2_w +
    d_w (2 S1_w + n_w d_w), d_w = p_w - p_0, mean = p_0 + a1 / n, var = a2 / n - (a1 / n)^2:
      mean:  bm = (E1 + sum e) / n, cast to fp32: + u (|mean| + bm)
      var:   Ev = (E2 + 2 sum_w |d_w| E1_w) / n + 2 |dm| E1 / n + (E1 / n)^2 + 2 sqrt(var mean(e^2)) + mean(e^2),  |dm| <= |mean - p_0| +
             mean(e) + e_0 (the last two terms: the variance of acc = c + delta against that of c, Cauchy-Schwarz)
    rstd, scale, shift and the running statistics follow as in tests/test_bn_pool_ops_gpu.py stats_bounds:
      rstd:  er = Ev / 2 (max(var - Ev, 0) + eps)^-3/2, br = er + u (rstd + er);   scale = gamma rstd: bs = |gamma| br + u |gamma| (rstd + br)
      shift = fma(-mean, scale, beta): A = bm |scale| + (|mean| + bm) bs, bsh = A + u (|mean scale| + |beta| + A)
      running = (1 - m) old + m new in fp32 ((1 - m) itself rounded): m b_new + 3 u |(1 - m) old| + 2 u m (|new| + b_new), the new
             variance being var n / (n - 1) cast to fp32."""
    M, K, C = c.shape
    n = M * K
    _, bpw = walk(M, waves)
    Lc = 16 * K * bpw + 1
    first = ((torch.arange(M, device=c.device) // BLK) % waves) * BLK  # the pivot pixel of every pixel's wave
    piv, epiv = c[first, 0], e[first, 0]
    D = (c - piv[:, None]).abs() + e + epiv[:, None]
    dw = (piv - c[0, 0]).abs() + epiv + e[0, 0]
    E1 = (Lc + 1) * U * D.sum((0, 1))
    E1w = (Lc + 1) * U * (dw[:, None] * D).sum((0, 1))
    E2 = (Lc + 3) * U * (D * D).sum((0, 1))
    del D
    gam, bet = gamma.double(), beta.double()
    ref = R.bn_stats(c.reshape(n, C), gam, bet, EPS, MOM, rm.double(), rv.double())
    se, se2 = e.sum((0, 1)) / n, (e * e).sum((0, 1)) / n
    dm = (ref['mean'] - c[0, 0]).abs() + se + e[0, 0]
    b = {}
    bm = (E1 + e.sum((0, 1))) / n
    bm = b['mean'] = bm + U * (ref['mean'].abs() + bm)
    Ev = (E2 + 2 * E1w) / n + 2 * dm * E1 / n + (E1 / n)**2 + 2 * torch.sqrt(ref['var'] * se2) + se2
    er = 0.5 * Ev * ((ref['var'] - Ev).clamp_min(0) + EPS)**-1.5
    br = b['rstd'] = er + U * (ref['rstd'] + er)
    bs = b['scale'] = gam.abs() * br + U * gam.abs() * (ref['rstd'] + br)
    A = bm * ref['scale'].abs() + (ref['mean'].abs() + bm) * bs
    b['shift'] = A + U * ((ref['mean'] * ref['scale']).abs() + bet.abs() + A)
    f = n / (n - 1.0)
    bu = Ev * f + U * (ref['unbiased'] + Ev * f)
    b['run_mean'] = MOM * bm + 3 * U * ((1 - MOM) * rm.double()).abs() + 2 * U * MOM * (ref['mean'].abs() + bm)
    b['run_var'] = MOM * bu + 3 * U * ((1 - MOM) * rv.double()).abs() + 2 * U * MOM * (ref['unbiased'] + bu)
    return ref, b


STAT_KEYS = ('mean', 'rstd', 'scale', 'shift', 'run_mean', 'run_var')


def check_stats(tag, out, c, e, waves, bn):
    ref, b = wave_stats_bounds(c, e, waves, *bn)
    for k in STAT_KEYS:
        within('%s BN %s' % (tag, k), out[k], ref[k], b[k])


def stats_outputs(bn, rows):
    out = {k: nan(64) for k in ('scale', 'shift', 'mean', 'rstd')}
    out['run_mean'], out['run_var'] = bn[2].clone(), bn[3].clone()
    out['ws'] = nan((3 * 64 + 1) * rows)
    return out


def stats_args(bn, out):
    if bn is None:
        return (None, None, 0.0, 0.0) + (None, ) * 7
    return (bn[0].data_ptr(), bn[1].data_ptr(), EPS, MOM) + tuple(out[k].data_ptr() for k in ('run_mean', 'run_var', 'scale', 'shift', 'mean', 'rstd', 'ws'))


# ------------------------------------------------------------------------------------------------------------------------------------
# (1, 2) the stem: dbn_nchw3_to_padded4_t + dbn_stem16_pack + dbn_stem16_conv_bn_t / dbn_stem16_conv_bn_relu_pool_t
# ------------------------------------------------------------------------------------------------------------------------------------
def stem_dims(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def stem_prepare(at, x, w):
    """The way in: the fp32 image -> the zero-bordered packed 16-bit form (checked bit for bit: the interior is the image as stored, the
    fourth channel and the border are zero; the packed copy x4 likewise), the fp32 weight -> the 16-bit panel."""
    N, _, H, W = x.shape
    Hp, Wp = L().dbn_stem16_padded_h(H), L().dbn_stem16_padded_w(W)
    assert L().dbn_stem16_eligible(at, N, H, W) == 1
    xp = torch.zeros(N, Hp, Wp, 4, device=DEV, dtype=DT[at])
    x4 = nan(N, H, W, 4, dtype=DT[at])
    _lib.check(L().dbn_nchw3_to_padded4_t(at, x.data_ptr(), xp.data_ptr(), x4.data_ptr(), N, H, W, stream()), 'padded4')
    want = torch.zeros(N, Hp, Wp, 4, device=DEV, dtype=DT[at])
    want[:, 3:H + 3, 3:W + 3, :3] = x.permute(0, 2, 3, 1).to(DT[at])
    exact('stem way in: padded image', xp, want)
    exact('stem way in: packed image', x4, want[:, 3:H + 3, 3:W + 3])
    panel = torch.full((L().dbn_stem16_panel_bytes(), ), 0xFF, device=DEV, dtype=torch.uint8)  # (0xFFFF: a NaN in both 16-bit types)
    _lib.check(L().dbn_stem16_pack(at, w.data_ptr(), panel.data_ptr(), stream()), 'stem16 pack')
    return xp, panel


def stem_ref(x, w, at):
    """float64 conv of the operands as stored, image by image: c [N, Ho, Wo, 64] and conv(|x|, |w|)."""
    w64 = stored(w, at)
    parts = [R.stem_conv(stored(x[n:n + 1], at), w64) for n in range(x.shape[0])]
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])


def stem_data(kind, N, H, W, seed):
    """random: the image ~ N(0, 1), He-scaled weights.  dense / late / seams: exact cases — image in {-1, 0, 1} (late: zero wherever the
    output pixel under it lies in a wave's first block or within two rows behind it; seams: zero but for +-1 under the seam pixels of
    the output walk, at the four corners and on the four borders), weights integer {-1, 0, 1} 2^k(co) (seams: {-7 .. 7} / 4, where an
    output sums the few impulses in its window: at most 8 of them in 3 channels, 168 steps of 1 / 4).  Also returns the grid of the
    conv's values per output channel (2^k(co); seams: 1 / 4; random: None)."""
    g = gen(seed)
    Ho, Wo = stem_dims(H, W)
    if kind == 'random':
        return torch.randn(N, 3, H, W, generator=g, device=DEV), torch.randn(64, 3, 7, 7, generator=g, device=DEV) * (2.0 / 147)**0.5, None
    k = ints(-2, 2, (64, 1, 1, 1), g)
    unit = torch.exp2(k).view(64)
    x = ints(-1, 1, (N, 3, H, W), g)
    w = ints(-1, 1, (64, 3, 7, 7), g) * torch.exp2(k)
    if kind == 'late':
        cut = L().dbn_stem16_rows() * BLK + 2 * Wo + 4
        m = (torch.arange(N, device=DEV).view(N, 1, 1) * Ho + torch.arange(H, device=DEV).view(1, H, 1) // 2) * Wo + torch.arange(W, device=DEV).view(1, 1, W) // 2
        x = x * (m >= cut).view(N, 1, H, W)
    if kind == 'seams':
        w, unit = ints(-7, 7, (64, 3, 7, 7), g) / 4, torch.full((64, ), 0.25, device=DEV)
        px = seam_pixels(N, Ho * Wo)
        n, ho, wo = px // (Ho * Wo), px % (Ho * Wo) // Wo, px % Wo
        imp = torch.zeros(N, 3, H, W, device=DEV)
        imp[n, :, 2 * ho, 2 * wo] = 1
        for hh in (0, H // 2, H - 1):
            for ww in (0, W // 2, W - 1):
                imp[:, :, hh, ww] = 1
        x = torch.where(imp > 0, torch.where(x == 0, torch.ones_like(x), x), imp)
    return x, w, unit


def stem_case(at, N, H, W, kind, seed, stats=True):
    """dbn_stem16_conv_bn_t on stem_data: y against the float64 conv within 224 u conv(|x|, |w|), stored once (exact kinds: bit for bit);
    with the statistics: the same bits of y, and save_mean / save_rstd / scale / shift / running statistics within wave_stats_bounds
    (e = 224 u conv(|x|, |w|); exact kinds: e = 0)."""
    tag = 'stem %s %s at=%d' % ((N, H, W), kind, at)
    x, w, _ = stem_data(kind, N, H, W, seed)
    xp, panel = stem_prepare(at, x, w)
    Ho, Wo = stem_dims(H, W)
    c, mag = stem_ref(x, w, at)
    e = 224 * U * mag if kind == 'random' else torch.zeros_like(mag)
    del mag
    y = nan(N, Ho, Wo, 64, dtype=DT[at])
    _lib.check(L().dbn_stem16_conv_bn_t(at, xp.data_ptr(), panel.data_ptr(), y.data_ptr(), N, H, W, *stats_args(None, None), stream()), 'stem16')
    if kind == 'random':
        within(tag, y, c, store_bound(at, c, e))
    else:
        assert_storable(tag, c, at)
        exact(tag, y, c)
    if not stats:
        return
    rows = L().dbn_stem16_rows()
    bn = bn_params(seed + 1, kind != 'random')
    out = stats_outputs(bn, rows)
    y2 = nan(N, Ho, Wo, 64, dtype=DT[at])
    _lib.check(L().dbn_stem16_conv_bn_t(at, xp.data_ptr(), panel.data_ptr(), y2.data_ptr(), N, H, W, *stats_args(bn, out), stream()), 'stem16+bn')
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16)), tag + ': y differs with the statistics'
    check_stats(tag, out, c.reshape(-1, 1, 64), e.reshape(-1, 1, 64), rows, bn)


STEM_SHAPES = [(2, 64, 64), (1, 96, 70), (3, 33, 47), (1, 7, 9)]  # M = 2048 (whole blocks); 1680 and 1224 (ragged, blocks span images); 20


@pytest.mark.parametrize('at', ATS)
@pytest.mark.parametrize('kind', ['random', 'dense', 'seams'])
@pytest.mark.parametrize('N,H,W', STEM_SHAPES)
def test_stem_conv(N, H, W, kind, at):
    """dbn_stem16_conv_bn_t without and with the BatchNorm statistics at small shapes (stem_case)."""
    stem_case(at, N, H, W, kind, seed=N * 100 + H)


STEM_BIG = (3, 422, 418)  # 3 x 211 x 209 = 132 297 = 4134 x 32 + 9 output pixels


@pytest.mark.parametrize('at', ATS)
@pytest.mark.parametrize('kind', ['random', 'dense', 'late'])
def test_stem_conv_multi_block(kind, at):
    """4135 blocks on 2048 waves: waves 0 .. 38 take three blocks, the last of them ragged — the prefetch of block mb + nw under block
    mb's second half, the pivot from a wave's first block only, S1 / S2 / the count carried across blocks (stem_case)."""
    N, H, W = STEM_BIG
    Ho, Wo = stem_dims(H, W)
    M = N * Ho * Wo
    nblk, bpw = walk(M, L().dbn_stem16_rows())
    assert (M, nblk, bpw, nblk - 2 * L().dbn_stem16_rows(), M % BLK) == (132297, 4135, 3, 39, 9)
    stem_case(at, N, H, W, kind, seed=7)


def pool_plan(N, H, W):
    """The host plan of dbn_stem16_conv_bn_relu_pool_t (csrc/stem16.hip): strips of 15 pooled columns, chunks of rpc pooled rows."""
    Ho, Wo = stem_dims(H, W)
    Hq, Wq = stem_dims(Ho, Wo)
    nseg = -(-Wq // 15)
    waves = 4 * 512  # (`const int grid = 512, waves = 4 * grid` in dbn_stem16_conv_bn_relu_pool_t, csrc/stem16.hip)
    rpc = 20
    while rpc > 4 and N * nseg * -(-Hq // rpc) < 5 * waves:
        rpc >>= 1
    return {'Hq': Hq, 'Wq': Wq, 'nseg': nseg, 'rpc': rpc, 'ntask': N * nseg * -(-Hq // rpc), 'waves': waves}


def pool_data(kind, N, H, W, seed):
    """stem_data + the eval BatchNorm: random scale ~ 1 +- 0.4 / shift ~ 0.5 N(0, 1).  Exact kinds: the image made non-negative, scale
    +-2^j, shift = |scale| grid(co) i with integer |i| <= 60, so that conv scale + shift = |scale| grid (integer of at most 147 + 60 <
    256; seams: 168 + 60): storable.  Channel 0 (weights >= 0, shift -200 grid) is negative everywhere: the pooled map must be +0 there;
    channel 1 (weights >= 0, shift +60 grid) positive everywhere; the others mixed: negative values beside positive ones.  late: the dense
    image, zero wherever the pooled pixel above it (h / 4, w / 4) belongs to one of the first 2048 tasks, every wave's first task."""
    x, w, unit = stem_data('dense' if kind == 'late' else kind, N, H, W, seed)
    g = gen(seed + 3)
    if kind == 'random':
        return x, w, torch.randn(64, generator=g, device=DEV) * 0.4 + 1, torch.randn(64, generator=g, device=DEV) * 0.5
    if kind == 'late':
        plan = pool_plan(N, H, W)
        nchunk = -(-plan['Hq'] // plan['rpc'])
        py = (torch.arange(H, device=DEV) // 4).clamp_max(plan['Hq'] - 1).view(1, H, 1)
        px = (torch.arange(W, device=DEV) // 4).clamp_max(plan['Wq'] - 1).view(1, 1, W)
        task = ((torch.arange(N, device=DEV).view(N, 1, 1) * nchunk + py // plan['rpc']) * plan['nseg'] + px // 15)  # (the kernel's task order)
        x = x * (task >= plan['waves']).view(N, 1, H, W)
    sc = pick([0.5, 1.0, 2.0, -1.0, -0.5], (64, ), g)
    sh = sc.abs() * unit * ints(-60, 60, (64, ), g)
    w[0], w[1] = w[0].abs(), w[1].abs()
    sc[0], sc[1] = 1.0, 1.0
    sh[0], sh[1] = -unit[0] * 200, unit[1] * 60  # (a negative value is never stored: any size will do)
    return x.abs(), w, sc, sh


def pool_case(at, N, H, W, kind, seed):
    """dbn_stem16_conv_bn_relu_pool_t against maxpool(relu(c scale + shift)) in float64: per conv pixel the fp32 value errs by
    ez = |scale| e + u (|c scale| + |shift| + |scale| e), e = 224 u conv(|x|, |w|) (one fmaf on the accumulator), and is stored once:
    b = store_bound(z, ez); the pooled bound is the maximum of b over the window.  Exact kinds: bit for bit, and no -0 anywhere."""
    tag = 'stem pool %s %s at=%d' % ((N, H, W), kind, at)
    x, w, sc, sh = pool_data(kind, N, H, W, seed)
    xp, panel = stem_prepare(at, x, w)
    assert L().dbn_stem16_pool_eligible(at, N, H, W) == 1
    plan = pool_plan(N, H, W)
    out = nan(N, plan['Hq'], plan['Wq'], 64, dtype=DT[at])
    _lib.check(L().dbn_stem16_conv_bn_relu_pool_t(at, xp.data_ptr(), panel.data_ptr(), sc.data_ptr(), sh.data_ptr(), out.data_ptr(), N, H, W,
                                                  stream()), 'stem16 pool')
    w64, sc64, sh64 = stored(w, at), sc.double(), sh.double()
    ref, bound = [], []
    for n in range(N):
        c, mag = R.stem_conv(stored(x[n:n + 1], at), w64)
        z, zmag = R.affine_relu(c, sc64, sh64)
        if kind == 'random':
            e = sc64.abs() * (224 * U * mag)
            bound.append(R.maxpool3x3s2p1(store_bound(at, z, e + U * (zmag + e)), 0.0))
        else:
            assert_storable(tag, z, at)
        ref.append(R.maxpool3x3s2p1(z))
        del c, mag, z, zmag
    ref = torch.cat(ref)
    if kind == 'random':
        within(tag, out, ref, torch.cat(bound))
    else:
        exact(tag, out, ref)
        assert not bool((out.view(torch.int16) == -32768).any()), tag + ': a -0 in the pooled map'
        assert float(ref[..., 0].abs().max()) == 0 and float(ref[..., 1].min()) > 0  # (the construction: all-negative / all-positive windows)
    return plan


# Wq = 16 = 15 + 1 and Hq = 5 (chunks of 2, 2 and 1 pooled rows); Wq = 30 = 15 + 15; one ragged strip, Hq = 9; the smallest map
POOL_SHAPES = [(2, 20, 63), (1, 19, 118), (3, 36, 47), (1, 8, 7)]


@pytest.mark.parametrize('at', ATS)
@pytest.mark.parametrize('kind', ['random', 'dense', 'seams'])
@pytest.mark.parametrize('N,H,W', POOL_SHAPES)
def test_stem_pool(N, H, W, kind, at):
    """The fused stem at small shapes: strip columns 0, 14 and 15, last strips of 1 and of 15 columns, pooled row 0, first and last
    row of a chunk, a one-row last chunk (pool_case)."""
    plan = pool_case(at, N, H, W, kind, seed=N * 10 + W)
    assert plan['rpc'] == 2


@pytest.mark.parametrize('at', ATS)
@pytest.mark.parametrize('kind', ['random', 'dense', 'late'])
@pytest.mark.parametrize('shape,nseg,rpc,ntask', [((3, 516, 697), 12, 2, 2340), ((40, 2568, 64), 2, 5, 10320)])
def test_stem_pool_multi_task(shape, nseg, rpc, ntask, kind, at):
    """More tasks than the 2048 waves: (3, 516, 697): 129 x 175 pooled, 12 strips, rpc = 2, 2340 tasks: a second task for waves 0 .. 291
    (PREV / HA re-used) and a one-row last chunk; (40, 2568, 64): 642 x 16 pooled, rpc = 5 for the first time, 10 320 tasks = five per wave
    and more, the last strip one column wide.  The host plan is recomputed here and asserted.  late: an image that is non-zero only under
    the waves' second and later tasks."""
    plan = pool_plan(*shape)
    assert (plan['nseg'], plan['rpc'], plan['ntask']) == (nseg, rpc, ntask) and ntask > plan['waves']
    pool_case(at, *shape, kind, seed=11)


# ------------------------------------------------------------------------------------------------------------------------------------
# (3, 4) dbn_convt16_bn_t and dbn_pw16_act_t
# ------------------------------------------------------------------------------------------------------------------------------------
def act_data(kind, N, H, W, seed, waves):
    """The 64-channel input [N, H, W, 64] (fp32 values; the caller stores them): random N(0, 1); dense {-1, 0, 1}; late: dense, zero in
    every wave's first block; seams: zero but for +-1 in two channels of every seam pixel."""
    g = gen(seed)
    if kind == 'random':
        return torch.randn(N, H, W, 64, generator=g, device=DEV)
    x = ints(-1, 1, (N * H * W, 64), g)
    if kind == 'late':
        x[:waves * BLK] = 0
    if kind == 'seams':
        px = seam_pixels(N, H * W)
        imp = torch.zeros_like(x)
        for j in range(2):
            imp[px, torch.randint(0, 64, (len(px), ), generator=g, device=DEV)] = 1
        x = torch.where(imp > 0, torch.where(x == 0, torch.ones_like(x), x), imp)
    return x.view(N, H, W, 64)


def weight_data(kind, shape, co_dim, seed, with_bias):
    """random: He-scaled weights, bias 0.1 N(0, 1).  exact: integers {-2 .. 2} 2^k(co), bias {-8 .. 8} 2^k(co): 64 terms of magnitude <= 2
    and the bias: 2^k (integer <= 136 < 256); seams (one or two impulses per pixel): {-15 .. 15} / 8, bias {-8 .. 8} / 8.  Also returns the
    grid of the results per output channel (2^k(co); seams: 1 / 8; random: None)."""
    g = gen(seed)
    Co = shape[co_dim]
    if kind == 'random':
        return torch.randn(shape, generator=g, device=DEV) * (2.0 / 64)**0.5, (torch.randn(Co, generator=g, device=DEV) * 0.1 if with_bias else None), None
    if kind == 'seams':
        return ints(-15, 15, shape, g) / 8, (ints(-8, 8, (Co, ), g) / 8 if with_bias else None), torch.full((Co, ), 0.125, device=DEV)
    k = torch.exp2(ints(-2, 2, (Co, ), g))
    kshape = [1] * len(shape)
    kshape[co_dim] = Co
    return ints(-2, 2, shape, g) * k.view(kshape), (ints(-8, 8, (Co, ), g) * k if with_bias else None), k


def convt_case(at, N, H, W, kind, with_bias, seed, stats=True):
    """dbn_convt16_bn_t: y against the float64 ConvT within e = 65 u (|bias| + sum |x| |w|), stored once (exact kinds: bit for bit); with
    the statistics: the same bits, and the six statistics within wave_stats_bounds (K = 4 classes per input pixel)."""
    tag = 'convt %s %s bias=%d at=%d' % ((N, H, W), kind, with_bias, at)
    rows = L().dbn_convt16_rows()
    xs = act_data(kind, N, H, W, seed, rows).to(DT[at])
    w, bias, _ = weight_data(kind, (64, 64, 2, 2), 1, seed + 1, with_bias)
    assert L().dbn_convt16_eligible(at, N, H, W, 64, 64) == 1
    panel = torch.full((L().dbn_convt16_panel_bytes(), ), 0xFF, device=DEV, dtype=torch.uint8)
    _lib.check(L().dbn_convt16_pack(at, w.data_ptr(), panel.data_ptr(), stream()), 'convt16 pack')
    c, mag = R.conv_transpose2x2(xs.double(), stored(w, at), None if bias is None else bias.double())
    e = 65 * U * mag if kind == 'random' else torch.zeros_like(mag)
    del mag
    y = nan(N, 2 * H, 2 * W, 64, dtype=DT[at])
    _lib.check(L().dbn_convt16_bn_t(at, xs.data_ptr(), panel.data_ptr(), ptr(bias), y.data_ptr(), N, H, W, *stats_args(None, None), stream()), 'convt16')
    if kind == 'random':
        within(tag, y, c, store_bound(at, c, e))
    else:
        assert_storable(tag, c, at)
        exact(tag, y, c)
    if not stats:
        return
    bn = bn_params(seed + 2, kind != 'random')
    out = stats_outputs(bn, rows)
    y2 = nan(N, 2 * H, 2 * W, 64, dtype=DT[at])
    _lib.check(L().dbn_convt16_bn_t(at, xs.data_ptr(), panel.data_ptr(), ptr(bias), y2.data_ptr(), N, H, W, *stats_args(bn, out), stream()), 'convt16+bn')
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16)), tag + ': y differs with the statistics'
    cls = lambda t: t.view(N, H, 2, W, 2, 64).permute(0, 1, 3, 2, 4, 5).reshape(N * H * W, 4, 64)  # [input pixel, class 2 a + b, co]
    check_stats(tag, out, cls(c), cls(e), rows, bn)


ACT_SHAPES = [(2, 16, 16), (1, 24, 17), (3, 5, 7), (1, 1, 1)]  # M = 512 (whole blocks); 408 and 105 (ragged; blocks span images); 1
ACT_BIG = (3, 211, 209)  # 132 297 pixels, as STEM_BIG's output


def assert_three_blocks(waves):
    N, H, W = ACT_BIG
    M = N * H * W
    nblk, bpw = walk(M, waves)
    assert (M, nblk, bpw, nblk - 2 * waves, M % BLK) == (132297, 4135, 3, 39, 9) and waves == 2048


@pytest.mark.parametrize('at', ATS)
@pytest.mark.parametrize('with_bias', [False, True])
@pytest.mark.parametrize('kind', ['random', 'dense', 'seams'])
@pytest.mark.parametrize('N,H,W', ACT_SHAPES)
def test_convt(N, H, W, kind, with_bias, at):
    """dbn_convt16_bn_t without and with the BatchNorm statistics, without and with bias, at small shapes (convt_case)."""
    convt_case(at, N, H, W, kind, with_bias, seed=N * 50 + W)


@pytest.mark.parametrize('at', ATS)
@pytest.mark.parametrize('kind,with_bias', [('random', True), ('dense', False), ('late', True)])
def test_convt_multi_block(kind, with_bias, at):
    """4135 blocks on 2048 waves: three blocks for waves 0 .. 38, the last ragged; the pivot from the first block's class 0 only, S1 / S2
    carried over 3 blocks x 4 classes, the count 4 x rows of every block (convt_case)."""
    assert_three_blocks(L().dbn_convt16_rows())
    convt_case(at, *ACT_BIG, kind, with_bias, seed=9)


def pw_case(at, N, H, W, Co, kind, relu, with_bias, seed):
    """dbn_pw16_act_t: y = [relu](x W^T + bias) against float64 within e = 65 u (|bias| + sum |x| |w|) (the ReLU is 1-Lipschitz), stored
    once; exact kinds bit for bit."""
    tag = 'pw16 %s Co=%d %s relu=%d bias=%d at=%d' % ((N, H, W), Co, kind, relu, with_bias, at)
    waves = 4 * (1024 if Co == 64 else 512)  # (`const int grid = Cout == 64 ? 1024 : 512` x 4 waves in dbn_pw16_act_t, csrc/convt16.hip)
    xs = act_data(kind, N, H, W, seed, waves).to(DT[at])
    w, bias, _ = weight_data(kind, (Co, 64), 0, seed + 1, with_bias)
    assert L().dbn_pw16_eligible(at, N, H, W, 64, Co) == 1
    panel = torch.full((L().dbn_pw16_panel_bytes(), ), 0xFF, device=DEV, dtype=torch.uint8)
    _lib.check(L().dbn_pw16_pack(at, w.data_ptr(), Co, panel.data_ptr(), stream()), 'pw16 pack')
    y = nan(N, H, W, Co, dtype=DT[at])
    _lib.check(L().dbn_pw16_act_t(at, xs.data_ptr(), panel.data_ptr(), ptr(bias), relu, y.data_ptr(), N, H, W, Co, stream()), 'pw16')
    w64, b64 = stored(w, at), None if bias is None else bias.double()
    for n in range(N):  # (image by image: 256 float64 channels)
        ref, mag = R.pointwise(xs[n].double(), w64, b64, bool(relu))
        if kind == 'random':
            within('%s image %d' % (tag, n), y[n], ref, store_bound(at, ref, 65 * U * mag))
        else:
            assert_storable(tag, ref, at)
            exact('%s image %d' % (tag, n), y[n], ref)


PW_VARIANTS = [(0, False), (1, True), (1, False), (0, True)]  # (relu, bias)


@pytest.mark.parametrize('at', ATS)
@pytest.mark.parametrize('relu,with_bias', PW_VARIANTS)
@pytest.mark.parametrize('kind', ['random', 'dense', 'seams'])
@pytest.mark.parametrize('Co', [64, 256])
@pytest.mark.parametrize('N,H,W', ACT_SHAPES[1:3])
def test_pw16(N, H, W, Co, kind, relu, with_bias, at):
    """dbn_pw16_act_t, Cout 64 and 256, relu 0 / 1, bias NULL / given, at small shapes (pw_case)."""
    pw_case(at, N, H, W, Co, kind, relu, with_bias, seed=N * 70 + H + Co)


@pytest.mark.parametrize('at', ATS)
@pytest.mark.parametrize('kind,relu,with_bias', [('random', 1, True), ('dense', 0, False), ('late', 1, True)])
@pytest.mark.parametrize('Co', [64, 256])
def test_pw16_multi_block(Co, kind, relu, with_bias, at):
    """Cout 256: 4135 blocks on 2048 waves (three blocks for waves 0 .. 38, the last ragged); Cout 64 runs 4096 waves: 3 x 300 x 291 =
    261 900 pixels = 8185 blocks, a second block for every wave but seven, the last one ragged (pw_case)."""
    if Co == 256:
        assert_three_blocks(4 * 512)  # (the grid of dbn_pw16_act_t, see pw_case)
        shape = ACT_BIG
    else:
        shape = (3, 300, 291)
        M = 3 * 300 * 291
        assert (M, walk(M, 4 * 1024), M % BLK) == (261900, (8185, 2), 12)
    pw_case(at, *shape, Co, kind, relu, with_bias, seed=13)


# ------------------------------------------------------------------------------------------------------------------------------------
# (5) dbn_head16_tail_eval_t
# ------------------------------------------------------------------------------------------------------------------------------------
def head16_data(kind, N, Hq, Wq, seed, with_bias1):
    """Per branch: x, the first ConvT (weight_data), the eval BatchNorm behind it, the second ConvT [64, 1, 2, 2] and its bias.
    random: scale ~ 1 +- 0.3, shift ~ 0.3 N(0, 1), w2 ~ 0.2 N(0, 1) rounded to the storage type by the caller (the kernel multiplies in
    that type).  exact: the first ConvT gives grid(co) (integer <= 136, weight_data); scale = +-2^j / grid(co), j in {-4, -3}, shift =
    2^j (integer in +-8): z = 2^j (integer < 256) is storable; w2 in {-1, -1/2, 0, 1/2, 1}, bias2 a multiple of 1/4: the logit, 64 terms
    on a grid of 2^-5 below 2^11, is exact in fp32 in any order.  The small shift keeps most logits within +-10, where a sigmoid is
    further than SIGMA from 0 and 1 and a wrong logit shows."""
    br = []
    for i in range(2):
        g = gen(seed + 10 * i)
        x = act_data(kind, N, Hq, Wq, seed + 10 * i + 1, 2048)
        w1, b1, unit = weight_data(kind, (64, 64, 2, 2), 1, seed + 10 * i + 2, with_bias1)
        if kind == 'random':
            sc, sh = torch.randn(64, generator=g, device=DEV) * 0.3 + 1, torch.randn(64, generator=g, device=DEV) * 0.3
            w2, b2 = torch.randn(64, 1, 2, 2, generator=g, device=DEV) * 0.2, torch.randn(1, generator=g, device=DEV)
        else:
            tj = torch.exp2(ints(-4, -3, (64, ), g))
            sc, sh = pick([1.0, 1.0, -1.0], (64, ), g) * tj / unit, tj * ints(-8, 8, (64, ), g)
            w2, b2 = pick([-1.0, -0.5, 0.0, 0.5, 1.0], (64, 1, 2, 2), g), ints(-4, 4, (1, ), g) / 4
        br.append({'x': x, 'w1': w1, 'b1': b1, 'sc': sc, 'sh': sh, 'w2': w2, 'b2': b2})
    return br


def head16_run(at, br, N, Hq, Wq):
    assert L().dbn_head16_eligible(at, N, Hq, Wq) == 1
    xs, panels = [], []
    for d in br:
        xs.append(d['x'].to(DT[at]))
        panels.append(torch.full((L().dbn_convt16_panel_bytes(), ), 0xFF, device=DEV, dtype=torch.uint8))
        _lib.check(L().dbn_convt16_pack(at, d['w1'].data_ptr(), panels[-1].data_ptr(), stream()), 'convt16 pack')
    out = nan(N, 2, 4 * Hq, 4 * Wq)
    p = lambda k: [ptr(d[k]) for d in br]
    _lib.check(L().dbn_head16_tail_eval_t(at, xs[0].data_ptr(), xs[1].data_ptr(), panels[0].data_ptr(), panels[1].data_ptr(), *p('b1'),
                                          br[0]['sc'].data_ptr(), br[0]['sh'].data_ptr(), br[1]['sc'].data_ptr(), br[1]['sh'].data_ptr(),
                                          *p('w2'), *p('b2'), out.data_ptr(), N, Hq, Wq, stream()), 'head16')
    torch.cuda.synchronize()
    return xs, out


def head16_case(at, N, Hq, Wq, kind, with_bias1, seed):
    """dbn_head16_tail_eval_t against sigmoid(head_chain) in float64, per branch.  The kernel's chain and its bound:
      c1 = bias1 + sum x w1 (MFMA):                        e1 = 65 u (|bias1| + sum |x| |w1|)
      z  = relu(fmaf(c1, scale, shift)), stored 16-bit:    ez = |scale| e1 + u (|c1 scale| + |shift| + |scale| e1), ezs = store_bound(z, ez)
      l  = sum_co z w2 (MFMA, w2 in the storage type) + bias2:  el = sum |w2| ezs + 65 u (sum (z + ezs) |w2| + |bias2|)
      P  = sigmoid(l):                                     el / 4 + SIGMA
    Exact kinds: every step is exact, so |P - sigmoid64(l64)| <= SIGMA."""
    tag = 'head16 %s %s bias1=%d at=%d' % ((N, Hq, Wq), kind, with_bias1, at)
    br = head16_data(kind, N, Hq, Wq, seed, with_bias1)
    for d in br:
        d['w2'] = d['w2'].to(DT[at]).float()  # (the operand as the kernel stores it)
    xs, out = head16_run(at, br, N, Hq, Wq)
    worst = 0.0
    for i, d in enumerate(br):
        w2, b2 = d['w2'].double(), d['b2'].double()
        for n in range(N):
            r = R.head_chain(xs[i][n:n + 1].double(), stored(d['w1'], at), None if d['b1'] is None else d['b1'].double(), d['sc'].double(),
                             d['sh'].double(), w2, b2)
            P = torch.sigmoid(r['logit'])
            name = '%s branch %d image %d' % (tag, i, n)
            if kind == 'random':
                e1 = d['sc'].double().abs() * (65 * U * r['mag1'])
                ezs = store_bound(at, r['z'], e1 + U * (r['zmag'] + e1))
                el = R.propagate_convt1(ezs, w2) + 65 * U * (R.propagate_convt1(r['z'] + ezs, w2) + b2.abs())
                within(name, out[n:n + 1, i], P, el / 4 + SIGMA)
            else:
                assert_storable(name, r['z'], at)
                assert torch.equal(r['logit'].float().double(), r['logit'])
                within(name, out[n:n + 1, i], P, SIGMA)
                worst = max(worst, float((out[n:n + 1, i].double() - P).abs().max()))
    if kind != 'random':
        print('%s: sigmoid error on exact logits %.3e (SIGMA %.3e)' % (tag, worst, SIGMA))


@pytest.mark.parametrize('at', ATS)
@pytest.mark.parametrize('with_bias1', [False, True])
@pytest.mark.parametrize('kind', ['random', 'dense', 'seams'])
@pytest.mark.parametrize('N,Hq,Wq', ACT_SHAPES)
def test_head16_tail(N, Hq, Wq, kind, with_bias1, at):
    """dbn_head16_tail_eval_t at small shapes, both branches with parameters of their own (head16_case)."""
    head16_case(at, N, Hq, Wq, kind, with_bias1, seed=N * 20 + Wq)


@pytest.mark.parametrize('at', ATS)
@pytest.mark.parametrize('kind', ['random', 'dense', 'late'])
def test_head16_tail_multi_block(kind, at):
    """4135 blocks on the 256 x 8 = 2048 waves of a branch: waves 0 .. 38 take three blocks, the last ragged — load_a(an, mb + nw) under
    block mb and the rotate a[t] = an[t] (head16_case)."""
    assert_three_blocks(256 * 8)  # (`const dim3 grid(256, 2)` x H16_WAVES = 8 waves per branch in dbn_head16_tail_eval_t, csrc/convt16.hip)
    head16_case(at, *ACT_BIG, kind, True, seed=17)


# ------------------------------------------------------------------------------------------------------------------------------------
# (6) dbn_head_tail_fwd_t
# ------------------------------------------------------------------------------------------------------------------------------------
def ht_data(kind, at, N, Hq, Wq, seed):
    """random: x ~ N(0, 1) stored, w ~ 0.2 N(0, 1) fp32, BatchNorm scale ~ 1 +- 0.3 / shift ~ 0.5 N(0, 1).  exact: x integers in +-4
    (seams: zero but at the seam pixels of the 64-pixel runs), scale in {+-1/4, 1/2}, shift multiples of 1/4, w multiples of 1/8 up to 1/2,
    bias of 1/4: a logit is 64 terms on a grid of 2^-5 below 2^7: exact in fp32 in any order."""
    g = gen(seed)
    d = {}
    for br in ('b', 't'):
        if kind == 'random':
            d['x' + br] = torch.randn(N, Hq, Wq, 64, generator=g, device=DEV).to(DT[at])
            d['w' + br], d['bias' + br] = torch.randn(64, 1, 2, 2, generator=g, device=DEV) * 0.2, torch.randn(1, generator=g, device=DEV)
            d['sc' + br], d['sh' + br] = torch.randn(64, generator=g, device=DEV) * 0.3 + 1, torch.randn(64, generator=g, device=DEV) * 0.5
        else:
            x = ints(-4, 4, (N * Hq * Wq, 64), g)
            if kind == 'seams':
                keep = torch.zeros(N * Hq * Wq, 1, device=DEV)
                keep[seam_pixels(N, Hq * Wq, 64)] = 1
                x = torch.where(keep > 0, x, keep)
            d['x' + br] = x.view(N, Hq, Wq, 64).to(DT[at])
            d['w' + br], d['bias' + br] = ints(-4, 4, (64, 1, 2, 2), g) / 8, ints(-4, 4, (1, ), g) / 4
            d['sc' + br], d['sh' + br] = pick([0.25, -0.25, 0.5], (64, ), g), ints(-4, 4, (64, ), g) / 4
    return d


def ht_run(at, d, N, Hq, Wq, ch, bn):
    out = nan(N, ch, 2 * Hq, 2 * Wq)
    p = lambda k: d[k].data_ptr() if bn else None
    _lib.check(L().dbn_head_tail_fwd_t(at, d['xb'].data_ptr(), d['xt'].data_ptr(), d['wb'].data_ptr(), d['wt'].data_ptr(), d['biasb'].data_ptr(),
                                       d['biast'].data_ptr(), p('scb'), p('shb'), p('sct'), p('sht'), out.data_ptr(), N, Hq, Wq, ch, KSTEP,
                                       stream()), 'head_tail_fwd')
    torch.cuda.synchronize()
    return out


def ht_check(tag, at, d, out, N, Hq, Wq, ch, bn, is_exact):
    """head_tail_fwd_kernel in fp32 (no contraction), per branch: v = relu(fmaf(x, scale, shift)) (ev = u (|x scale| + |shift|); without
    the BatchNorm v = x, ev = 0); l = bias + sum v w: one rounding per product, 63 adds (a lane's chain, then the DPP tree) and the
    bias add, at most 65 roundings on any term: el = sum |w| ev + 65 u (|bias| + sum (|v| + ev) |w|); P = sigmoid(l): el / 4 + SIGMA.
    B against the float64 step function of the P, T the kernel wrote: k 2 u |P - T| / 4 + SIGMA.  is_exact: el = 0."""
    kw = {k: d[a].double() for k, a in (('scale_b', 'scb'), ('shift_b', 'shb'), ('scale_t', 'sct'), ('shift_t', 'sht'))} if bn else {}
    r = R.head_tail(d['xb'].double(), d['xt'].double(), d['wb'].double(), d['wt'].double(), d['biasb'].double(), d['biast'].double(), ch,
                    KSTEP, **kw)
    for i, br in enumerate(('b', 't')):
        if is_exact:
            assert torch.equal(r['logit_' + br].float().double(), r['logit_' + br])  # (the construction)
            bound = SIGMA
        else:
            w = d['w' + br].double()
            ev = U * r['vmag_' + br] if bn else torch.zeros_like(r['vmag_' + br])
            pe = R.propagate_convt1(ev, w)
            bound = (pe + 65 * U * (r['mag_' + br] + pe)) / 4 + SIGMA
        within('%s %s' % (tag, 'PT'[i]), out[:, i], r['out'][:, i], bound)
    if ch == 3:
        P, T = out[:, 0].double(), out[:, 1].double()
        within(tag + ' B of the stored P, T', out[:, 2], R.step_map(P, T, KSTEP), KSTEP * 2 * U * (P - T).abs() / 4 + SIGMA)
    return float((out[:, :2].double() - r['out'][:, :2]).abs().max())


def ht_case(at, N, Hq, Wq, ch, bn, kind, seed):
    """One data set through every lane form the storage type has (16-bit: sixteen and eight lanes per pixel, dbn_set_head_tail_wide)."""
    d = ht_data(kind, at, N, Hq, Wq, seed)
    worst = 0.0
    old = L().dbn_set_head_tail_wide(0)
    try:
        for mode in ((0, ) if at == 0 else (-1, 1)):
            L().dbn_set_head_tail_wide(mode)
            out = ht_run(at, d, N, Hq, Wq, ch, bn)
            tag = 'head_tail_fwd %s ch=%d bn=%d %s at=%d wide=%d' % ((N, Hq, Wq), ch, bn, kind, at, mode)
            worst = max(worst, ht_check(tag, at, d, out, N, Hq, Wq, ch, bn, kind != 'random'))
    finally:
        L().dbn_set_head_tail_wide(old)
    return worst


# A lane group steps by gstride = 16 pixels (sixteen lanes per pixel) or 32 (eight).  (40, 1, 3) and (30, 2, 3): images of 3 and 6 pixels,
# 120 and 180 pixels in all: the stride spans g_n = 5 / 2 (10 / 5) whole images plus a rest with carries from wq into hq into n, over
# several trips, the four-pixel trip included.  (5, 1, 3) and (1, 2, 3): maps smaller than one stride (one pixel per lane group);
# (2, 9, 7): Wq < 16; (3, 16, 16), (2, 33, 20): g_n = 0, whole and ragged runs of 64, several blocks
HT_SHAPES = [(40, 1, 3), (30, 2, 3), (5, 1, 3), (2, 9, 7), (1, 2, 3), (3, 16, 16), (2, 33, 20)]


@pytest.mark.parametrize('at', [0, 1, 2])
@pytest.mark.parametrize('ch,bn', [(3, True), (3, False), (2, True), (2, False)])
@pytest.mark.parametrize('kind', ['random', 'dense', 'seams'])
@pytest.mark.parametrize('N,Hq,Wq', HT_SHAPES)
def test_head_tail_fwd(N, Hq, Wq, kind, ch, bn, at):
    """dbn_head_tail_fwd_t, channels 2 / 3, without / with the fused BatchNorm, every lane form (ht_case, bounds in ht_check).  A block
    streams one run of `per` pixels and per = 64 up to 2^20 pixels: the sixteen-lane form takes its four-pixel trip here (4 x 16 = 64),
    the eight-lane form only its one-pixel tail trips (test_head_tail_fwd_long_runs runs the other)."""
    npx = N * Hq * Wq
    assert ((npx + 16383) // 16384 + 63) // 64 * 64 == 64
    worst = ht_case(at, N, Hq, Wq, ch, bn, kind, seed=N * 30 + Wq)
    if kind != 'random':
        print('head_tail_fwd %s at=%d: sigmoid error on exact logits %.3e (SIGMA %.3e)' % ((N, Hq, Wq), at, worst, SIGMA))


@pytest.mark.parametrize('at', [0, 1, 2])
@pytest.mark.parametrize('kind', ['random', 'dense'])
def test_head_tail_fwd_long_runs(kind, at):
    """Just above 2^20 pixels (2 x 1025 x 512) the run length per doubles to 128: the eight-lane form (gstride 32) takes its unrolled
    four-pixel trip with its four advance() calls — the only loop it runs at the sizes that select it (>= 2^22 pixels, per >= 256) —
    and the sixteen-lane form two such trips per block.  Channels 3, fused BatchNorm; reference and bounds as in ht_check."""
    N, Hq, Wq = 2, 1025, 512
    npx = N * Hq * Wq
    assert npx > 1 << 20 and ((npx + 16383) // 16384 + 63) // 64 * 64 == 128
    ht_case(at, N, Hq, Wq, 3, True, kind, seed=41)


# ------------------------------------------------------------------------------------------------------------------------------------
# the sigmoid's measured error
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('at', [0, 1, 2])
def test_sigmoid_error_on_exact_logits(at):
    """Logits k / 8, |k| <= 160 (channel 0 = k / 8 with unit weights, every other channel zero; the thresh branch with bias -1 / 16), through
    both lane forms of head_tail_fwd_kernel and (16-bit storage: j / 8 through a unit first ConvT, second ConvT +-1) through
    head16_tail_eval_kernel: the measured max |P - sigmoid64| is printed; SIGMA must be at least twice it."""
    ks = torch.arange(-160, 161, device=DEV).float() / 8
    N, Hq, Wq = 1, 3, 107
    x = torch.zeros(N * Hq * Wq, 64, device=DEV)
    x[:, 0] = ks
    w = torch.zeros(64, 1, 2, 2, device=DEV)
    w[0] = 1
    d = {'xb': x.view(N, Hq, Wq, 64).to(DT[at]), 'wb': w, 'biasb': torch.zeros(1, device=DEV)}
    d.update({'xt': d['xb'], 'wt': w, 'biast': torch.full((1, ), -0.0625, device=DEV)})
    assert torch.equal(d['xb'].double().view(-1, 64)[:, 0], ks.double())
    want = torch.stack([torch.sigmoid(ks.double()), torch.sigmoid(ks.double() - 0.0625)], 0).view(2, Hq, 1, Wq, 1).expand(2, Hq, 2, Wq, 2)
    want = want.reshape(1, 2, 2 * Hq, 2 * Wq)
    measured = 0.0
    old = L().dbn_set_head_tail_wide(0)
    try:
        for mode in ((0, ) if at == 0 else (-1, 1)):
            L().dbn_set_head_tail_wide(mode)
            out = ht_run(at, d, N, Hq, Wq, 2, False)
            within('sigmoid sweep head_tail_fwd at=%d wide=%d' % (at, mode), out, want, SIGMA)
            measured = max(measured, float((out.double() - want).abs().max()))
    finally:
        L().dbn_set_head_tail_wide(old)
    if at != 0:
        js = torch.arange(0, 161, device=DEV).float() / 8
        Hq, Wq = 7, 23
        x = torch.zeros(Hq * Wq, 64, device=DEV)
        x[:, 0] = js
        w1 = torch.zeros(64, 64, 2, 2, device=DEV)
        w1[0, 0] = 1
        w2 = torch.zeros(64, 1, 2, 2, device=DEV)
        w2[0, 0] = torch.tensor([[1.0, -1.0], [-1.0, 1.0]], device=DEV)
        one, zero = torch.ones(64, device=DEV), torch.zeros(64, device=DEV)
        br = [{'x': x.view(1, Hq, Wq, 64), 'w1': w1, 'b1': None, 'sc': one, 'sh': zero, 'w2': w2, 'b2': torch.zeros(1, device=DEV)},
              {'x': x.view(1, Hq, Wq, 64), 'w1': w1, 'b1': zero, 'sc': one, 'sh': zero, 'w2': -w2, 'b2': torch.full((1, ), -0.0625, device=DEV)}]
        _, out = head16_run(at, br, 1, Hq, Wq)
        for i, d2 in enumerate(br):
            r = R.head_chain(br[i]['x'].double(), w1.double(), None, one.double(), zero.double(), d2['w2'].double(), d2['b2'].double())
            assert torch.equal(r['logit'][0, ::4, ::4].reshape(-1), (1 - 2 * i) * js.double() + d2['b2'].double())  # (the construction)
            P = torch.sigmoid(r['logit'])
            within('sigmoid sweep head16 at=%d branch %d' % (at, i), out[:, i], P, SIGMA)
            measured = max(measured, float((out[:, i].double() - P).abs().max()))
    print('measured sigmoid error at=%d: %.4e (SIGMA_MEASURED %.4e, SIGMA %.4e)' % (at, measured, SIGMA_MEASURED, SIGMA))
    assert 2 * measured <= SIGMA, 'the measured sigmoid error %.3e is more than half of SIGMA' % measured
