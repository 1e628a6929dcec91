"""-m gpu: operation-level pins of the kernels the 16-bit training step launches (BASELINE configs[2] / [3]: bf16 activations and
gradients) that no other operation test calls, in all the storage types they accept (at = 0 fp32, 1 bf16, 2 fp16):

  dbn_head_tail_bwd_t               last ConvT + both sigmoids + step function, backward, with the fused BatchNorm-backward sums
  dbn_col_sum_t                     bias gradients (per-channel column sums)
  dbn_deform_im2col_t               the deformable convolution's bilinear sampling (configs[3])
  dbn_deform_offset_absmax_t        max |offset| that picks the deformable adjoint's form
  dbn_nchw3_to_nhwc16_and_4_t       the first launch of every 16-bit step (the stem's input forms)

Each kernel meets three kinds of case:
  random data  against a float64 reference computed on the operands AS STORED (inputs rounded to the storage type first), with an
               elementwise bound derived in the test's docstring from the kernel's own arithmetic: u = 2^-24 (fp32 evaluation),
               s = the storage type's unit roundoff (bf16 2^-8, fp16 2^-11, fp32 2^-24); an fp32 sum of n terms computed by a serial
               chain of length `depth` errs by at most about (depth + c) u sum|terms|, sum|terms| taken in float64 beside the reference;
  exact data   dyadic values with few significant bits, so that every fp32 and storage-type operation of the kernel is exact: the
               kernel must equal the float64 reference bit for bit.  Gradients are sparse and sit on the seams of the kernels'
               pixel walks (first / last pixel of every image, px = 0 and gstride - 1 mod the grid stride, last pixel of the batch),
               where one dropped, duplicated or misplaced term would hide inside a random-data bound;
  step sizes   the shapes the bf16 step launches, so that grid-stride loops and partial-sum folds run many iterations; there the
               reference runs on the GPU in float64 from elementwise ops, reductions and matmul (no convolution), elsewhere on the CPU.
Every output starts as NaN (an element the kernel never writes fails), and padding channels the kernel must not read hold NaN."""
import pytest
import torch

from deform_ref import edge_offsets
from gpu_util import DEV, DT, ETA, NAN, SR, U, L, col_sum_depth, exact, gen, stream, within
from db_text_minimal_amd import _lib
from oracle import dbnet_oracle as O

pytestmark = pytest.mark.gpu

STEP_N, STEP_HQ = 16, 320  # configs[2]: 16 x 640^2 images, the head tail works on 320^2 quarter-resolution maps of the 640^2 output


# ------------------------------------------------------------------------------------------------------------------------------------
# (a) dbn_head_tail_bwd_t
# ------------------------------------------------------------------------------------------------------------------------------------
def ht_walk(N, Hq, Wq):
    """The kernel's pixel walk (csrc/head_loss.hip): nb = min(ceil(16 npx / 256), 2047) blocks of 16 pixels; a lane visits pixels
    px0, px0 + gstride, ... with gstride = 16 nb, at most `depth` = ceil(npx / gstride) of them."""
    npx = N * Hq * Wq
    nb = min(max(-(-npx * 16 // 256), 1), 2047)
    gstride = 16 * nb
    return npx, gstride, -(-npx // gstride)


def to_quads(t, N, Hq, Wq):
    """[N, 2Hq, 2Wq] full-resolution map -> [N Hq Wq, 4]: the 2 x 2 block (a, b) of each quarter pixel, ab = 2 a + b (the ConvT tap)."""
    return t.reshape(N, Hq, 2, Wq, 2).permute(0, 1, 3, 2, 4).reshape(N * Hq * Wq, 4)


def from_quads(q, N, Hq, Wq):
    return q.reshape(N, Hq, Wq, 2, 2).permute(0, 1, 3, 2, 4).reshape(N, 2 * Hq, 2 * Wq)


def ht_run(at, inp, N, Hq, Wq, CH, kstep, gs, bn, sums):
    """One dbn_head_tail_bwd_t call with NaN-filled outputs and workspace; returns the outputs."""
    dt = DT[at]
    out = {
        'dxb': torch.full((N, Hq, Wq, 64), NAN, device=DEV, dtype=dt),
        'dxt': torch.full((N, Hq, Wq, 64), NAN, device=DEV, dtype=dt),
        'dwb': torch.full((256, ), NAN, device=DEV), 'dbb': torch.full((1, ), NAN, device=DEV),
        'dwt': torch.full((256, ), NAN, device=DEV), 'dbt': torch.full((1, ), NAN, device=DEV),
    }
    if sums:
        out['sums'] = torch.full((4, 64), NAN, device=DEV)
    ws = torch.full((L().dbn_head_tail_bwd_ws_floats(), ), NAN, device=DEV)
    p = lambda k: inp[k].data_ptr() if bn else None
    _lib.check(L().dbn_head_tail_bwd_t(at, inp['yb'].data_ptr(), inp['yt'].data_ptr(), inp['wb'].data_ptr(), inp['wt'].data_ptr(),
                                       inp['preds'].data_ptr(), inp['dpreds'].data_ptr(), p('scb'), p('shb'), p('sct'), p('sht'),
                                       inp['mub'].data_ptr() if sums else None, inp['rsb'].data_ptr() if sums else None,
                                       inp['mut'].data_ptr() if sums else None, inp['rst'].data_ptr() if sums else None,
                                       out['sums'].data_ptr() if sums else None, out['dxb'].data_ptr(), out['dxt'].data_ptr(),
                                       out['dwb'].data_ptr(), out['dbb'].data_ptr(), out['dwt'].data_ptr(), out['dbt'].data_ptr(), N, Hq, Wq,
                                       CH, kstep, gs, ws.data_ptr(), stream()), 'head_tail_bwd_t')
    torch.cuda.synchronize()
    return out


def ht_logit_grads(inp, N, Hq, Wq, CH, kstep, rdev):
    """float64 dl_b, dl_t [npx, 4] (gradients w.r.t. the two logits) from the given preds / dpreds, and A_b, A_t: the magnitudes
    (|dP| + |gB|) P (1 - P) that bound the fp32 evaluation error of dl."""
    q = lambda t, c: to_quads(t[:, c].to(rdev, torch.float64), N, Hq, Wq)
    P, T, dP, dT = q(inp['preds'], 0), q(inp['preds'], 1), q(inp['dpreds'], 0), q(inp['dpreds'], 1)
    aP, aT = dP.abs(), dT.abs()
    if CH == 3:
        B = q(inp['preds'], 2)
        gB = q(inp['dpreds'], 2) * kstep * B * (1 - B)
        dP, dT = dP + gB, dT - gB
        aP, aT = aP + gB.abs(), aT + gB.abs()
    return {'b': dP * P * (1 - P), 't': dT * T * (1 - T)}, {'b': aP * (P * (1 - P)).abs(), 't': aT * (T * (1 - T)).abs()}


def ht_check(tag, at, inp, out, N, Hq, Wq, CH, kstep, gs, bn, sums, is_exact):
    """Compares every output of ht_run with float64 (on the CPU for small maps, on the GPU at step sizes).

    Kernel arithmetic (fp32, no contraction; csrc/head_loss.hip head_tail_bwd_kernel) and the bounds it implies, per branch:
      dl   = ((dP + gB) P)(1 - P), gB = ((dB k) B)(1 - B): at most 8 roundings -> |dl - dl64| <= 8 u A, A = (|dP| + |gB|) P (1 - P)
      dx   = w0 dl0 + w1 dl1 + w2 dl2 + w3 dl3 (left to right), stored: |dx - dx64| <= s |dx64| + (1 + s) 12 u sum_ab |w_ab| A_ab + eta
      dw   = gs * sum_px x dl: a lane's serial chain of `depth` fp32 adds, then 16 lane groups added in LDS, then the blocks folded in
             float64 and rounded once; each term carries 1 (x = fmaf(y, sc, sh)) + 8 (dl) + 1 (product) roundings:
             |dw - dw64| <= |gs| (depth + 16 + 12) u sum_px |x| A + u |dw64|
      dbias = gs * sum_px (dl0 + dl1 + dl2 + dl3): four terms per step of the chain: (depth + 16 + 3 + 8 + 2) u |gs| sum A + u |db64|
      bn sums: sums over the kernel's OWN STORED dx (it sums the rounded gradient, which the BatchNorm backward reads), masked by the
             float64 y sc + sh > 0 (its sign is the sign of the kernel's fmaf: y sc is exact in float64): s1 = sum m dx exact terms,
             (depth + 16 + 1) u sum |m dx| + u |s1|;  s2 = sum m dx ((y - mean) rstd): 3 roundings per term, (depth + 16 + 4) u ...
    is_exact: every quantity above is exact (the inputs are built so): all outputs must equal float64 exactly."""
    npx, gstride, depth = ht_walk(N, Hq, Wq)
    rdev = 'cpu' if npx * 64 < (1 << 22) else DEV
    s, eta = SR[at], ETA[at]
    dl, A = ht_logit_grads(inp, N, Hq, Wq, CH, kstep, rdev)
    d = lambda t: t.to(rdev, torch.float64)
    for br in ('b', 't'):
        w = d(inp['w' + br]).reshape(64, 4)
        y = d(inp['y' + br]).reshape(npx, 64)
        if bn:
            x = y * d(inp['sc' + br]) + d(inp['sh' + br])
            mask = x > 0
            x = x.clamp_min_(0)
        else:
            x, mask = y, None
        dx_ref = dl[br] @ w.t()
        dx_got = d(out['dx' + br]).reshape(npx, 64)
        if is_exact:
            exact('%s dx%s' % (tag, br), dx_got, dx_ref)
        else:
            within('%s dx%s' % (tag, br), dx_got, dx_ref, s * dx_ref.abs() + (1 + s) * 12 * U * (A[br] @ w.abs().t()) + eta)
        del dx_ref
        dw_ref = gs * (x.t() @ dl[br])  # [64, 4]: ConvTranspose2d weight [64, 1, 2, 2] flattened
        db_ref = gs * dl[br].sum()
        if is_exact:
            exact('%s dw%s' % (tag, br), out['dw' + br], dw_ref)
            exact('%s dbias%s' % (tag, br), out['db' + br], db_ref.view(1))
        else:
            within('%s dw%s' % (tag, br), out['dw' + br], dw_ref, abs(gs) * (depth + 28) * U * (x.abs().t() @ A[br]) + U * dw_ref.abs())
            within('%s dbias%s' % (tag, br), out['db' + br], db_ref.view(1), abs(gs) * (depth + 29) * U * A[br].sum() + U * db_ref.abs())
        del x
        if sums:
            i = 0 if br == 'b' else 2
            m = dx_got * mask
            xhat = (y - d(inp['mu' + br])) * d(inp['rs' + br])
            s1, s2 = m.sum(0), (m * xhat).sum(0)
            if is_exact:
                exact('%s bn sum%s' % (tag, br), out['sums'][i], s1)
                exact('%s bn sum_xhat%s' % (tag, br), out['sums'][i + 1], s2)
            else:
                within('%s bn sum%s' % (tag, br), out['sums'][i], s1, (depth + 17) * U * m.abs().sum(0) + U * s1.abs())
                within('%s bn sum_xhat%s' % (tag, br), out['sums'][i + 1], s2, (depth + 20) * U * (m * xhat).abs().sum(0) + U * s2.abs())
            del m, xhat
        del y, dx_got


def ht_inputs_random(at, N, Hq, Wq, CH, seed):
    g = gen(seed)
    dt = DT[at]
    r = lambda *shape, scale=1.0: torch.randn(*shape, generator=g, device=DEV) * scale
    u = lambda *shape: torch.rand(*shape, generator=g, device=DEV) * 0.96 + 0.02  # maps in (0.02, 0.98)
    return {
        'yb': r(N, Hq, Wq, 64).to(dt), 'yt': r(N, Hq, Wq, 64).to(dt),
        'wb': r(64, 4, scale=0.2), 'wt': r(64, 4, scale=0.2),
        'preds': u(N, CH, 2 * Hq, 2 * Wq), 'dpreds': r(N, CH, 2 * Hq, 2 * Wq, scale=0.1),
        'scb': r(64, scale=0.3) + 1, 'shb': r(64, scale=0.5), 'sct': r(64, scale=0.3) + 1, 'sht': r(64, scale=0.5),
        'mub': r(64, scale=0.2), 'rsb': torch.rand(64, generator=g, device=DEV) + 0.5,
        'mut': r(64, scale=0.2), 'rst': torch.rand(64, generator=g, device=DEV) + 0.5,
    }


def seam_pixels(N, Hq, Wq, gstride, extra, g):
    """Pixels on the seams of the walk: first / last of every image, px = 0 and gstride - 1 (mod gstride), the batch's last, + `extra`."""
    HWq = Hq * Wq
    npx = N * HWq
    px = set()
    for n in range(N):
        px |= {n * HWq, n * HWq + HWq - 1}
    px |= set(range(0, npx, gstride)) | set(range(gstride - 1, npx, gstride)) | {npx - 1}
    px |= set(torch.randint(0, npx, (extra, ), generator=g).tolist())
    return torch.tensor(sorted(px))


def ht_inputs_exact(at, N, Hq, Wq, CH, seed):
    """Dyadic operands: y in [-4, 4] integers, sc / sh / mean / rstd / w multiples of 1/4 .. 1/2, P = T = B = 1/2 and logit gradients
    dl in {-2..2} / 16 at the seam pixels only (zero elsewhere): dP = 4 dl_b - 12.5 dB, dT = 4 dl_t + 12.5 dB, so that the kernel's
    ((dP + dB k B (1 - B)) P)(1 - P) with k = 50 is exactly dl.  dx = sum w dl is then a multiple of 2^-6 below 2^-2 (exact in every
    storage type) and every sum of the kernel is a short dyadic number: exact in fp32."""
    npx, gstride, _ = ht_walk(N, Hq, Wq)
    g = torch.Generator().manual_seed(seed)
    dt = DT[at]
    pick = lambda vals, n: torch.tensor(vals)[torch.randint(0, len(vals), (n, ), generator=g)]
    gd = gen(seed + 1)
    px = seam_pixels(N, Hq, Wq, gstride, 64, g)
    k = len(px)
    dq = {}
    for br in ('b', 't'):
        t = torch.zeros(npx, 4)
        t[px] = torch.randint(-2, 3, (k, 4), generator=g).float() / 16
        dq[br] = t
    dB = torch.zeros(npx, 4)
    if CH == 3:
        dB[px] = torch.randint(-2, 3, (k, 4), generator=g).float() / 16
    dP, dT = 4 * dq['b'] - 12.5 * dB, 4 * dq['t'] + 12.5 * dB
    planes = [dP, dT] + ([dB] if CH == 3 else [])
    dpreds = torch.stack([from_quads(p, N, Hq, Wq) for p in planes], 1).to(DEV)
    return {
        'yb': torch.randint(-4, 5, (N, Hq, Wq, 64), generator=gd, device=DEV).to(dt),
        'yt': torch.randint(-4, 5, (N, Hq, Wq, 64), generator=gd, device=DEV).to(dt),
        'wb': (pick([-2, -1, 0, 1, 2], 256) / 4).view(64, 4).to(DEV), 'wt': (pick([-2, -1, 1, 2], 256) / 4).view(64, 4).to(DEV),
        'preds': torch.full((N, CH, 2 * Hq, 2 * Wq), 0.5, device=DEV), 'dpreds': dpreds,
        'scb': pick([-0.5, 0.5, 1, 1.5, 2], 64).to(DEV), 'shb': pick([-1, -0.5, 0, 0.5, 1], 64).to(DEV),
        'sct': pick([0.5, 1, 2], 64).to(DEV), 'sht': pick([-1, 0, 0.5], 64).to(DEV),
        'mub': pick([-0.5, 0, 0.5], 64).to(DEV), 'rsb': pick([0.5, 1, 2], 64).to(DEV),
        'mut': pick([-0.5, 0.5], 64).to(DEV), 'rst': pick([0.5, 2], 64).to(DEV),
        '_dl': dq,
    }


HT_SHAPES = [(1, 5, 7), (2, 9, 13), (3, 157, 203), (40, 50, 50)]  # ragged; both carries of the walk; gstride > one image (g_n >= 1)
# (the call as engine.py makes it: BatchNorm + ReLU on load, the fused sums, channels 3, k = 50, grad_scale 0.5), then without the
# BatchNorm, then the two-channel maps
HT_VARIANTS = {'engine': (3, True, True), 'no_bn': (3, False, False), 'ch2': (2, True, True)}


@pytest.mark.parametrize('at', [0, 1, 2])
@pytest.mark.parametrize('variant', list(HT_VARIANTS))
@pytest.mark.parametrize('shape', HT_SHAPES)
def test_head_tail_bwd_random_vs_fp64(shape, variant, at):
    """dbn_head_tail_bwd_t on random operands vs float64 on the operands as stored; bounds in ht_check."""
    N, Hq, Wq = shape
    CH, bn, sums = HT_VARIANTS[variant]
    inp = ht_inputs_random(at, N, Hq, Wq, CH, seed=11 + N)
    out = ht_run(at, inp, N, Hq, Wq, CH, 50.0, 0.5, bn, sums)
    ht_check('head bwd %s %s at=%d' % (shape, variant, at), at, inp, out, N, Hq, Wq, CH, 50.0, 0.5, bn, sums, False)


@pytest.mark.parametrize('at', [0, 1, 2])
@pytest.mark.parametrize('variant', list(HT_VARIANTS))
@pytest.mark.parametrize('shape', HT_SHAPES)
def test_head_tail_bwd_exact_on_the_seams(shape, variant, at):
    """Exact operands (ht_inputs_exact) with gradients on the seams of the pixel walk: every output equals float64 bit for bit."""
    N, Hq, Wq = shape
    CH, bn, sums = HT_VARIANTS[variant]
    inp = ht_inputs_exact(at, N, Hq, Wq, CH, seed=5 + Hq)
    out = ht_run(at, inp, N, Hq, Wq, CH, 50.0, 0.5, bn, sums)
    dl, _ = ht_logit_grads(inp, N, Hq, Wq, CH, 50.0, 'cpu')
    assert torch.equal(dl['b'], inp['_dl']['b'].double()) and torch.equal(dl['t'], inp['_dl']['t'].double())  # (the construction)
    ht_check('head bwd exact %s %s at=%d' % (shape, variant, at), at, inp, out, N, Hq, Wq, CH, 50.0, 0.5, bn, sums, True)


@pytest.mark.parametrize('at', [1, 0, 2])
def test_head_tail_bwd_at_step_size(at):
    """The configs[2] launch: 16 x 320 x 320 quarter pixels (2047 partial rows, about 50 pixels per lane), the call as the engine makes
    it, random operands (bounds of ht_check) and then exact operands on the seams; the reference in float64 on the GPU."""
    N, Hq, Wq = STEP_N, STEP_HQ, STEP_HQ
    npx, gstride, depth = ht_walk(N, Hq, Wq)
    assert gstride == 2047 * 16 and depth == 51
    inp = ht_inputs_random(at, N, Hq, Wq, 3, seed=21)
    out = ht_run(at, inp, N, Hq, Wq, 3, 50.0, 0.5, True, True)
    ht_check('head bwd step at=%d' % at, at, inp, out, N, Hq, Wq, 3, 50.0, 0.5, True, True, False)
    del inp, out
    inp = ht_inputs_exact(at, N, Hq, Wq, 3, seed=22)
    out = ht_run(at, inp, N, Hq, Wq, 3, 50.0, 0.5, True, True)
    ht_check('head bwd step exact at=%d' % at, at, inp, out, N, Hq, Wq, 3, 50.0, 0.5, True, True, True)


# ------------------------------------------------------------------------------------------------------------------------------------
# (b) dbn_col_sum_t
# ------------------------------------------------------------------------------------------------------------------------------------
# M x C: one row; one block; 64 rows per block exactly; a second block; 767 x 64 + 1 rows (768 blocks, the last with one row);
# 768 x 64 + 1 rows (the 768-block cap: 65 rows per block, the last blocks EMPTY); C = 2048 / 4096: the 1024-channel chunks of the
# grid's second dimension; the step's M = 16 x 320 x 320
COLSUM_CASES = [(1, 4), (63, 20), (64, 64), (65, 256), (767 * 64 + 1, 1024), (768 * 64 + 1, 64), (768 * 64 + 1, 2048), (130, 4096),
                (STEP_N * STEP_HQ * STEP_HQ, 64)]


def col_sum_run(at, x, scale):
    M, C = x.shape
    out = torch.full((C, ), NAN, device=DEV)
    ws = torch.full((L().dbn_reduce_ws_floats(C), ), NAN, device=DEV)
    _lib.check(L().dbn_col_sum_t(at, x.data_ptr(), M, C, out.data_ptr(), scale, ws.data_ptr(), stream()), 'col_sum_t')
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('at', [0, 1, 2])
@pytest.mark.parametrize('M,C', COLSUM_CASES)
def test_col_sum_random_vs_fp64(M, C, at):
    """dbn_col_sum_t = scale * sum over rows, on random data.  A thread sums its rows in an fp32 chain, the block's row lanes are added
    in LDS, the blocks are folded in float64 and multiplied by `scale` once: with depth = rows per thread + row lanes (col_sum_depth),
    |out - ref| <= |scale| (depth + 2) u sum |x| + u |ref| (the inputs are exact in the reference: it reads them as stored)."""
    x = torch.randn(M, C, generator=gen(M + C), device=DEV).to(DT[at])
    scale = -0.7
    out = col_sum_run(at, x, scale)
    xd = x.double()
    ref = xd.sum(0) * scale
    within('col_sum M=%d C=%d at=%d' % (M, C, at), out, ref, abs(scale) * (col_sum_depth(M, C) + 2) * U * xd.abs().sum(0) + U * ref.abs())


@pytest.mark.parametrize('at', [0, 1, 2])
@pytest.mark.parametrize('M,C', COLSUM_CASES)
def test_col_sum_exact(M, C, at):
    """Entries in {-1, 0, +1} 2^k (k per column in [-6, 6]), scale 2^-3: every partial sum is an integer multiple of 2^k below 2^24 of
    them, so the result is exact: a dropped, doubled or misplaced row, block or channel chunk shows as a wrong number."""
    g = gen(M * 7 + C)
    k = torch.randint(-6, 7, (C, ), generator=g, device=DEV).float()
    x = (torch.randint(-1, 2, (M, C), generator=g, device=DEV).float() * torch.exp2(k)).to(DT[at])
    if M > 1:  # the first and the last row are never zero (the seams of the row split)
        x[0] = torch.exp2(k).to(DT[at])
        x[-1] = -torch.exp2(k).to(DT[at]) * 2
    out = col_sum_run(at, x, 0.125)
    exact('col_sum exact M=%d C=%d at=%d' % (M, C, at), out, x.double().sum(0) * 0.125)


# ------------------------------------------------------------------------------------------------------------------------------------
# (c) dbn_deform_im2col_t
# ------------------------------------------------------------------------------------------------------------------------------------
DEFORM_CASES = [(2, 64, 9, 11, 1), (1, 128, 12, 10, 2), (1, 256, 13, 9, 2), (1, 512, 7, 8, 1), (2, 64, 10, 10, 1)]
DEFORM_BIG = (8, 128, 100, 100, 1)  # 8 x 100^2 x 9 = 720 000 sample teams: more than the 2^16 x 8 = 524 288 of one grid pass


def deform_run(at, xs, offs, N, H, W, C, stride, os_):
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    cols = torch.full((N, Ho, Wo, 9, C), NAN, device=DEV, dtype=DT[at])
    _lib.check(L().dbn_deform_im2col_t(at, xs.data_ptr(), offs.data_ptr(), cols.data_ptr(), N, H, W, C, Ho, Wo, 3, 3, stride, 1, os_,
                                       stream()), 'deform_im2col_t')
    torch.cuda.synchronize()
    return cols


def deform_ref(x_nhwc, off_nhwc, stride, rdev):
    """oracle.deform_sample in float64 on the stored operands -> [N, Ho, Wo, 9, C] (the kernel's column layout)."""
    x = x_nhwc.to(rdev, torch.float64).permute(0, 3, 1, 2)
    off = off_nhwc[..., :18].to(rdev, torch.float64).permute(0, 3, 1, 2)
    return O.deform_sample(x, off, 3, 3, stride, 1).permute(0, 3, 4, 2, 1)


def deform_offsets(kind, at, N, H, W, stride, os_, g):
    """The stored offset map [N, Ho, Wo, os_], channels 18.. NaN (the kernel must not read them)."""
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if kind == 'random':  # (bf16-valued offsets: the sample positions are exact in fp32 for every storage type)
        off = (torch.randn(N, Ho, Wo, 18, generator=g) * 1.5).to(torch.bfloat16).float()
    elif kind == 'half':  # multiples of 1/2: weights in {0, 1/4, 1/2, 1}
        off = torch.randint(-6, 7, (N, Ho, Wo, 18), generator=g).float() / 2
    elif kind == 'integer':
        off = torch.randint(-3, 4, (N, Ho, Wo, 18), generator=g).float()
    else:
        off = edge_offsets(N, H, W, stride, g)
    full = torch.full((N, Ho, Wo, os_), NAN)
    full[..., :18] = off
    return full.to(DEV).to(DT[at])


@pytest.mark.parametrize('at', [0, 1, 2])
@pytest.mark.parametrize('kind', ['random', 'half', 'integer', 'edges'])
@pytest.mark.parametrize('case', DEFORM_CASES)
def test_deform_im2col_vs_oracle(case, kind, at):
    """dbn_deform_im2col_t vs oracle.deform_sample in float64 on the stored operands, off_stride 64 with NaN in channels 18..63
    (os 18 for the last case).  'half' / 'integer' / 'edges' (x integers in [-4, 4], offsets multiples of 1/4 or 1/2 landing on the
    boundary classes of edge_offsets): all weights are multiples of 1/16 and every sample a multiple of 1/16 below 4 in magnitude,
    exact in fp32 and in every storage type -> bit-exact.  'random': each weight (1 - ly)(1 - lx) ... is formed with 3 roundings, each
    of the 4 products and 3 adds with one: |got - ref| <= s |ref| + (1 + s) 7 u sum_corners w |x| + eta (the position is exact:
    bf16-valued offsets plus an integer)."""
    N, C, H, W, stride = case
    os_ = 18 if case == DEFORM_CASES[-1] else 64
    g = torch.Generator().manual_seed(sum(case) * 10 + ['random', 'half', 'integer', 'edges'].index(kind))
    if kind == 'random':
        x = torch.randn(N, H, W, C, generator=g).to(DT[at]).to(DEV)
    else:
        x = torch.randint(-4, 5, (N, H, W, C), generator=g).float().to(DT[at]).to(DEV)
    offs = deform_offsets(kind, at, N, H, W, stride, os_, g)
    cols = deform_run(at, x, offs, N, H, W, C, stride, os_)
    ref = deform_ref(x, offs, stride, 'cpu')
    tag = 'deform im2col %s %s at=%d' % (case, kind, at)
    if kind == 'random':
        rabs = deform_ref(x.abs(), offs, stride, 'cpu')
        within(tag, cols, ref, SR[at] * ref.abs() + (1 + SR[at]) * 7 * U * rabs + ETA[at])
    else:
        exact(tag, cols, ref)


@pytest.mark.parametrize('at', [1, 0, 2])
def test_deform_im2col_grid_stride_loop(at):
    """More sample teams than one pass of the grid (DEFORM_BIG): half-integer offsets and the edge classes, bit-exact against the oracle
    run in float64 on the GPU."""
    N, C, H, W, stride = DEFORM_BIG
    g = torch.Generator().manual_seed(31)
    x = torch.randint(-4, 5, (N, H, W, C), generator=g).float().to(DT[at]).to(DEV)
    for kind in ('half', 'edges'):
        offs = deform_offsets(kind, at, N, H, W, stride, 64, g)
        cols = deform_run(at, x, offs, N, H, W, C, stride, 64)
        exact('deform im2col big %s at=%d' % (kind, at), cols, deform_ref(x, offs, stride, DEV))
        del cols


@pytest.mark.parametrize('at', [0, 1, 2])
def test_deform_im2col_non_finite_offset_stays_in_its_sample(at):
    """A NaN / +inf / -inf offset may only change its own sample's C columns: those are what the oracle gives (NaN: the sample's weights
    are NaN), every other column is bit-identical to the clean run."""
    N, C, H, W, stride = 2, 64, 9, 11, 1
    g = torch.Generator().manual_seed(41)
    x = torch.randn(N, H, W, C, generator=g).to(DT[at]).to(DEV)
    offs = deform_offsets('random', at, N, H, W, stride, 64, g)
    clean = deform_run(at, x, offs, N, H, W, C, stride, 64)
    hits = [(0, 2, 3, 4, NAN), (0, 0, 0, 1, float('inf')), (1, 8, 10, 16, -float('inf')), (1, 4, 5, 9, NAN)]  # (n, ho, wo, channel, v)
    bad = offs.clone()
    poisoned = torch.zeros(N, H, W, 9, 1, dtype=torch.bool, device=DEV)
    for n, ho, wo, ch, v in hits:
        bad[n, ho, wo, ch] = v
        poisoned[n, ho, wo, ch // 2] = True
    got = deform_run(at, x, bad, N, H, W, C, stride, 64)
    ref = deform_ref(x, bad, stride, 'cpu').to(DEV)
    poisoned = poisoned.expand_as(got)
    assert bool(torch.isnan(ref[poisoned]).all())  # (what the oracle gives: the pin)
    assert bool(torch.isnan(got[poisoned].float()).all()), 'a non-finite offset: its sample is not the oracle\'s NaN'
    keep = ~poisoned
    assert torch.equal(got[keep].view(torch.int16 if at else torch.int32), clean[keep].view(torch.int16 if at else torch.int32)), \
        'a non-finite offset changed another sample'


# ------------------------------------------------------------------------------------------------------------------------------------
# (d) dbn_deform_offset_absmax_t
# ------------------------------------------------------------------------------------------------------------------------------------
NONFINITE_BITS = 0x7FC00000
ABSMAX_STEP_N = 16 * 80 * 80 * 64  # the step's first deformable layer: N x Ho x Wo x 64 offset channels (80^2 maps of a 640^2 image)
LARGEST = {0: 3.4028234663852886e38, 1: 3.3895313892515355e38, 2: 65504.0}  # the largest finite value of the storage type


def absmax_run(at, x):
    bits = torch.full((1, ), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    _lib.check(L().dbn_deform_offset_absmax_t(at, x.data_ptr(), x.numel(), bits.data_ptr(), stream()), 'offset_absmax_t')
    torch.cuda.synchronize()
    return int(bits.cpu()[0]) & 0xFFFFFFFF


def absmax_want(x):
    x = x.float()
    if not bool(torch.isfinite(x).all()):
        return NONFINITE_BITS
    return int(x.abs().max().view(1).view(torch.int32).cpu()[0]) & 0xFFFFFFFF


@pytest.mark.parametrize('at', [0, 1, 2])
@pytest.mark.parametrize('n', [4, ABSMAX_STEP_N])
def test_deform_offset_absmax_bits(n, at):
    """out_bits = the bit pattern of max |offset| (torch's abs().max()), 0x7FC00000 as soon as one element is not finite.  The largest
    finite value of the storage type (FLT_MAX, bf16's 0x7F7F...) is finite: it is reported as itself."""
    dt = DT[at]
    base = (torch.randn(n, generator=gen(n + at), device=DEV) * 3).to(dt)
    cases = {'random': base}
    for where, i in (('first', 0), ('last', n - 1), ('middle', n // 2 + 1)):
        for sign in (1.0, -1.0):
            t = base.clone()
            t[i] = sign * 1000.0
            cases['max %s %+g' % (where, sign)] = t
    cases['zeros'] = torch.zeros(n, device=DEV, dtype=dt)
    cases['-0'] = torch.full((n, ), -0.0, device=DEV, dtype=dt)
    for where, i in (('first', 0), ('last', n - 1), ('middle', n // 3)):
        for v in (NAN, float('inf'), -float('inf')):
            t = base.clone()
            t[i] = v
            cases['%r %s' % (v, where)] = t
    for sign in (1.0, -1.0):
        t = base.clone()
        t[n - 1] = sign * LARGEST[at]
        assert bool(torch.isfinite(t.float()).all())
        cases['largest finite %+g' % sign] = t
    for name, t in cases.items():
        got, want = absmax_run(at, t), absmax_want(t)
        assert got == want, '%s (n=%d at=%d): 0x%08X, want 0x%08X' % (name, n, at, got, want)
    if at == 0:
        assert absmax_run(0, torch.tensor([1.0, 3.1e38, -2.0, 0.5], device=DEV)) == absmax_want(torch.tensor([3.1e38]))


# ------------------------------------------------------------------------------------------------------------------------------------
# (e) dbn_nchw3_to_nhwc16_and_4_t
# ------------------------------------------------------------------------------------------------------------------------------------
def halfway_values(at, n, g):
    """fp32 values exactly halfway between two neighbouring values of the storage type (and one fp32 ulp either side of that), where
    truncation, round-half-up and round-half-even all differ, plus ordinary random values."""
    dt = DT[at]
    a = (torch.randn(n, generator=g) * 4).to(dt)
    ia = a.view(torch.int16).int()
    b = (ia + 1).short().view(dt)  # the next representable value away from zero
    mid = (a.double() + b.double()) / 2  # exact in fp32: one more bit than the 16-bit type
    kind = torch.randint(0, 4, (n, ), generator=g)
    ulp = mid.abs().float().view(torch.int32)
    up = (ulp + 1).view(torch.float32).double() * mid.sign()
    dn = (ulp - 1).view(torch.float32).double() * mid.sign()
    v = torch.where(kind == 0, mid, torch.where(kind == 1, up, torch.where(kind == 2, dn, torch.randn(n, generator=g).double())))
    fin = torch.isfinite(b.float())
    return torch.where(fin, v, torch.zeros_like(v)).float()


@pytest.mark.parametrize('at', [1, 2])
@pytest.mark.parametrize('shape', [(1, 5, 7), (3, 17, 9), (STEP_N, 640, 640)])
def test_input_pack_rounds_to_nearest_even(shape, at):
    """out16 [N, H, W, 16]: channels 0..2 = x.to(bf16 | fp16) bit for bit (halfway values included), 3..15 = +0; out4 [N, H, W, 4]:
    channels 0..2 the same, 3 = +0.  With out4 = NULL only out16 is written (a sentinel guard behind it stays).  16 x 640^2 runs the
    grid-stride loop (more than 4096 x 256 pixels)."""
    N, H, W = shape
    dt = DT[at]
    g = torch.Generator().manual_seed(N * H + W)
    n = N * 3 * H * W
    x = halfway_values(at, n, g).view(N, 3, H, W).to(DEV)
    want = x.permute(0, 2, 3, 1).to(dt).view(torch.int16)
    bits = lambda t: t.view(torch.int16)
    for with4 in (True, False):
        guard = 4096
        buf16 = torch.full((N * H * W * 16 + guard, ), -7.0, device=DEV, dtype=dt)  # (sentinel: -7)
        buf4 = torch.full((N * H * W * 4 + guard, ), -7.0, device=DEV, dtype=dt)
        out16, out4 = buf16[:N * H * W * 16].view(N, H, W, 16), buf4[:N * H * W * 4].view(N, H, W, 4)
        out16.fill_(NAN)
        if with4:
            out4.fill_(NAN)
        _lib.check(L().dbn_nchw3_to_nhwc16_and_4_t(at, x.data_ptr(), out16.data_ptr(), out4.data_ptr() if with4 else None, N, H, W,
                                                   stream()), 'nchw3_to_nhwc16_and_4_t')
        torch.cuda.synchronize()
        tag = '%s at=%d out4=%s' % (shape, at, with4)
        assert torch.equal(bits(out16[..., :3]), want), tag + ': out16 is not round-to-nearest-even'
        assert not bool((bits(out16[..., 3:]) != 0).any()), tag + ': out16 channels 3..15 are not +0'
        sentinel = int(torch.tensor([-7.0], dtype=dt).view(torch.int16)[0])
        assert bool((bits(buf16[N * H * W * 16:]) == sentinel).all()), tag + ': out16 written out of range'
        if with4:
            assert torch.equal(bits(out4[..., :3]), want), tag + ': out4 is not round-to-nearest-even'
            assert not bool((bits(out4[..., 3:]) != 0).any()), tag + ': out4 channel 3 is not +0'
            assert bool((bits(buf4[N * H * W * 4:]) == sentinel).all()), tag + ': out4 written out of range'
        else:
            assert bool((bits(buf4) == sentinel).all()), tag + ': out4 = NULL, but the buffer changed'
