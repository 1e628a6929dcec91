"""-m gpu: the optimizer extensions of csrc/optim.hip against float64 (tests/optim_ref.py, itself pinned against torch by
tests/test_optim_ext_cpu.py), to the standard of test_adam_two_steps_vs_fp64 (tests/test_bn_pool_ops_gpu.py):

  (a) dbn_grad_accumulate    (b) dbn_grad_sqnorm    (c) dbn_adam_step_ex, options off: the bits of dbn_adam_step
  (d) dbn_adam_step_ex, every option on             (e) DBTrainer + FusedAdam(amsgrad, max_grad_norm, accumulation_steps) on ResNet-18
  (f) the refusals, the checkpoint round trip, the hipGraph step, fit()'s per-update scheduler

Sizes: the scalar-tail cases of the plain step's test and one n that spans two reduction chunks plus 3 (three partial sums).  Every buffer
is 8 elements longer than n and holds NaN there, which must survive every kernel; workspaces are poisoned.

The fp32 error model of (d) and (e), first order in U = 2^-24 as in the plain step's test (ex_bounds below).  With ga = coef s acc,
gd = wd p, g = ga + gd of the float64 restatement and E = (n + 8) 2^-53 for the float64 chain behind the coefficient (the n-term sum under
a square root, |s| x, + 1e-6, the quotient, x s):
  gs = fp32(coef s): 1 rounding; gs acc: 1;  wd p: 1;  the sum: 1         |dg| <= (2 U + E) |ga| + U |gd| + U |g|   (wd = 0: the first term only)
  m' = b1 m + (1 - b1) gg ((1 - b1) is exact: Sterbenz)                   |dm| <= (1 - b1) |dg| + 2 U (|b1 m| + |(1 - b1) g|)
  v' = b2 v + ((1 - b2) gg) gg                                            |dv| <= U b2 v + (1 - b2) (2 |g| |dg| + 2 U g^2) + U v'
  vmax' = max(vmax, v'): max is 1-Lipschitz                               |dvmax| <= |dv|
  denom = sqrt(root) c2 + eps, c2 = fp32(1 / sqrt(bc2)); |sqrt(a) - sqrt(b)| <= |a - b| / sqrt(b); sqrt, c2, product, sum: 4 roundings
                                                                          |dd| <= c2 |dv| / sqrt(root) + 4 U denom
  p' = p - lrc (m' / denom), lrc = fp32(lr / bc1): lrc, quotient, product: 3 roundings, the difference: 1
                                                                          |dp| <= lrc |dm| / denom + |upd| (|dd| / denom + 3 U) + U |p'|
"""
import math

import pytest
import torch

import optim_ref as R
from gpu_util import DEV, NAN, U, L, gen, stream, within
from db_text_minimal_amd import DBLoss, DBTextModel, DBTrainer, FusedAdam, _lib
from oracle import dbnet_oracle as O

pytestmark = pytest.mark.gpu

SQ_CHUNK = 16384  # elements per workgroup of the norm's first stage (csrc/optim.hip; test_sqnorm_partition checks the value)
NS = [1, 3, 4, 5, 1023, 4 * 1003 + 3, 2 * SQ_CHUNK + 3]
LR, B1, B2, EPS, WD = (float(torch.tensor(x, dtype=torch.float32)) for x in (0.005, 0.9, 0.999, 1e-8, 0.01))  # the floats the ABI receives
GS = 0.25


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def mk(t):
    return torch.cat([t, nan(8, dtype=t.dtype)])


def bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int64)


def same_bits(tag, got, ref):
    ne = bits(got) != bits(ref)
    assert not bool(ne.any()), '%s: %d of %d elements differ in their bits; the first at %d' % (tag, int(ne.sum()), ne.numel(), int(ne.nonzero()[0]))


def guard_kept(tag, t, n):
    assert bool(torch.isnan(t[n:]).all()) and t.numel() == n + 8, tag + ': the guard beyond n was written'


def ex_bounds(parts, pr, vr, b1, b2, n, decay, g_round=2, m_round=2, v_round=(1, 2), coef_err=None):
    """(|dm|, |dv|, |dp|) of the module docstring from the magnitudes R.adam_step_ex returns.  g_round / m_round / v_round: the fp32 roundings
    on ga, on the terms of m' and on the two terms of v' — the kernel's by default; coef_err: the relative error of the clip coefficient
    (default: E of the float64 chain)."""
    E = (n + 8) * 2.0**-53 if coef_err is None else coef_err
    g, ga = parts['g'], parts['ga'].abs()
    dg = (g_round * U + E) * ga
    if decay:
        dg = dg + U * (parts['g_terms'] - ga) + U * g.abs()
    bm = (1 - b1) * dg + m_round * U * parts['m_terms']
    bv = v_round[0] * U * parts['b2v'] + (1 - b2) * (2 * g.abs() * dg + v_round[1] * U * g * g) + U * vr
    root = parts['root']
    dsqrt = torch.where(root > 0, bv / root.sqrt().clamp_min(1e-300), torch.zeros_like(bv))  # (root = 0: g = v = 0 and sqrt(0) is exact)
    bd = parts['c2'] * dsqrt + 4 * U * parts['denom']
    bp = parts['lrc'] * bm / parts['denom'] + parts['upd'].abs() * (bd / parts['denom'] + 3 * U) + U * pr.abs()
    return bm, bv, bp


# ------------------------------------------------------------------------------------------------------------------------------------
# (a) dbn_grad_accumulate
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', NS)
def test_grad_accumulate_bits(n):
    """first = 1 copies bit for bit (the accumulator starts as NaN: nothing of it may be read); first = 0 is torch's fp32 acc + g bit for
    bit: one rounding, the same operation.  The gradient's 8 elements beyond n are FINITE here, so a copy that runs past n would replace
    the accumulator's NaN guard."""
    g = gen(n)
    g1 = torch.cat([torch.randn(n, generator=g, device=DEV), torch.ones(8, device=DEV)])
    g2 = torch.cat([torch.randn(n, generator=g, device=DEV) * 3, torch.ones(8, device=DEV)])
    acc = nan(n + 8)
    _lib.check(L().dbn_grad_accumulate(acc.data_ptr(), g1.data_ptr(), n, 1, stream()), 'fold first')
    torch.cuda.synchronize()
    same_bits('first fold n=%d' % n, acc[:n], g1[:n])
    guard_kept('first fold n=%d' % n, acc, n)
    _lib.check(L().dbn_grad_accumulate(acc.data_ptr(), g2.data_ptr(), n, 0, stream()), 'fold')
    torch.cuda.synchronize()
    same_bits('second fold n=%d' % n, acc[:n], g1[:n] + g2[:n])
    guard_kept('second fold n=%d' % n, acc, n)


# ------------------------------------------------------------------------------------------------------------------------------------
# (b) dbn_grad_sqnorm
# ------------------------------------------------------------------------------------------------------------------------------------
def test_sqnorm_partition():
    ws = L().dbn_grad_sqnorm_ws_doubles
    assert (ws(SQ_CHUNK), ws(SQ_CHUNK + 1), ws(NS[-1])) == (1, 2, 3)


@pytest.mark.parametrize('n', NS)
def test_grad_sqnorm_bits_and_value(n):
    """Two runs with the workspace prefilled with different bytes (NaN, then 0x5A) give the same bits: no partial sum is read before it is
    written and nothing depends on what ran before.  Against the exactly rounded sum of the float64 squares (math.fsum; a product of two
    fp32 values is exact in float64): n - 1 float64 adds of positive terms err by at most (n - 1) 2^-53 relative in any order, the
    reference by 2^-53: n 2^-53.  The gradient's NaN beyond n must not be read, the workspace's 8 doubles beyond its size and out[1] must
    not be written."""
    g = mk(torch.randn(n, generator=gen(n + 1), device=DEV) * 3)
    nws = L().dbn_grad_sqnorm_ws_doubles(n)
    outs = []
    for fill in (0xFF, 0x5A):
        ws = torch.empty(nws + 8, device=DEV, dtype=torch.float64)
        ws.view(torch.uint8).fill_(fill)
        before = ws[nws:].clone()
        out = nan(2, dtype=torch.float64)
        _lib.check(L().dbn_grad_sqnorm(g.data_ptr(), n, ws.data_ptr(), out.data_ptr(), stream()), 'sqnorm')
        torch.cuda.synchronize()
        same_bits('sqnorm n=%d: the workspace beyond its size' % n, ws[nws:], before)
        assert bool(torch.isnan(out[1])), 'sqnorm n=%d: out[1] was written' % n
        outs.append(out[:1].clone())
    same_bits('sqnorm n=%d: two runs' % n, outs[0], outs[1])
    ref = math.fsum(g[:n].double().square().cpu().tolist())
    within('sqnorm n=%d' % n, outs[0], torch.tensor([ref], dtype=torch.float64), n * 2.0**-53 * ref)


# ------------------------------------------------------------------------------------------------------------------------------------
# (c) dbn_adam_step_ex with the options off
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', NS)
def test_adam_ex_options_off_is_adam_step_bit_for_bit(n):
    """vmax = NULL, sqnorm = NULL, weight_decay = 0: p, m, v (and their NaN guards) equal dbn_adam_step's on copies, for two steps"""
    g = gen(n + 2)
    a = [mk(torch.randn(n, generator=g, device=DEV)), mk(torch.zeros(n, device=DEV)), mk(torch.zeros(n, device=DEV))]
    b = [t.clone() for t in a]
    for step, gscale in ((1, 1e-3), (2, 1e-2)):
        grad = mk(torch.randn(n, generator=g, device=DEV) * gscale * 4)
        _lib.check(L().dbn_adam_step(a[0].data_ptr(), grad.data_ptr(), a[1].data_ptr(), a[2].data_ptr(), n, LR, B1, B2, EPS, step, GS, stream()),
                   'adam')
        _lib.check(L().dbn_adam_step_ex(b[0].data_ptr(), grad.data_ptr(), b[1].data_ptr(), b[2].data_ptr(), None, n, LR, B1, B2, EPS, 0.0, step,
                                        GS, None, 0.0, stream()), 'adam_ex')
        torch.cuda.synchronize()
        for name, x, y in zip(('param', 'exp_avg', 'exp_avg_sq'), a, b):
            assert bool(torch.isfinite(y[:n]).all())
            same_bits('adam_ex plain n=%d step %d %s' % (n, step, name), y, x)


# ------------------------------------------------------------------------------------------------------------------------------------
# (d) dbn_adam_step_ex with every option on
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['clipped', 'unclipped'])
@pytest.mark.parametrize('n', NS)
def test_adam_ex_all_options_vs_fp64(n, mode):
    """AMSGrad, weight_decay 0.01, grad_scale 1/4 and a max-norm of half (coefficient 1/2) or twice (coefficient 1) the step's own norm, the
    squared norm taken from dbn_grad_sqnorm's device value: two steps, the second on non-zero moments, each against R.adam_step_ex in
    float64 on the state the kernel held BEFORE the step; bounds: ex_bounds (module docstring).  The second gradient has one hundredth of
    the first's scale, so exp_avg_sq falls below its running maximum on most elements — asserted in the reference (n >= 1023), so that
    the test cannot pass with AMSGrad inert.  (v' < v needs g2^2 < v = (1 - b2) g1^2, |g2| < 0.032 |g1|: the scaled gradients are 10 z and
    0.1 z for standard normal z, and the decay term 0.01 p is a tenth of the second: |g2| / |g1| ~ 0.01.)"""
    g = gen(n + 3)
    p = mk(torch.randn(n, generator=g, device=DEV))
    m, v, x = (mk(torch.zeros(n, device=DEV)) for _ in range(3))
    nws = L().dbn_grad_sqnorm_ws_doubles(n)
    for step, gscale in ((1, 10.0), (2, 0.1)):
        grad = mk(torch.randn(n, generator=g, device=DEV) * gscale * 4)
        p0, m0, v0, x0 = (t[:n].double() for t in (p, m, v, x))
        norm = float(R.grad_norm(grad[:n], GS))
        c = float(torch.tensor(norm * (0.5 if mode == 'clipped' else 2.0), dtype=torch.float32))
        ws, sq = nan(nws + 8, dtype=torch.float64), nan(2, dtype=torch.float64)
        _lib.check(L().dbn_grad_sqnorm(grad.data_ptr(), n, ws.data_ptr(), sq.data_ptr(), stream()), 'sqnorm')
        _lib.check(L().dbn_adam_step_ex(p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), x.data_ptr(), n, LR, B1, B2, EPS, WD, step, GS,
                                        sq.data_ptr(), c, stream()), 'adam_ex')
        torch.cuda.synchronize()
        pr, mr, vr, xr, parts = R.adam_step_ex(p0, grad[:n], m0, v0, x0, LR, B1, B2, EPS, WD, step, grad_scale=GS, max_norm=c)
        assert bool(parts['coef'] < 1) == (mode == 'clipped'), float(parts['coef'])
        if step == 2 and n >= 1023:
            below = float((vr < xr).double().mean())
            assert below > 0.5, 'exp_avg_sq is below its maximum on %.3f of the elements only: AMSGrad would be inert' % below
        bm, bv, bp = ex_bounds(parts, pr, vr, B1, B2, n, decay=True)
        tag = 'adam_ex %s n=%d step %d ' % (mode, n, step)
        within(tag + 'exp_avg', m[:n], mr, bm)
        within(tag + 'exp_avg_sq', v[:n], vr, bv)
        within(tag + 'max_exp_avg_sq', x[:n], xr, bv)
        within(tag + 'param', p[:n], pr, bp)
        for name, t in (('param', p), ('exp_avg', m), ('exp_avg_sq', v), ('max_exp_avg_sq', x)):
            guard_kept(tag + name, t, n)
        assert bool(torch.isnan(sq[1])) and bool(torch.isnan(ws[nws:]).all()), tag + 'the norm wrote beyond its outputs'


# ------------------------------------------------------------------------------------------------------------------------------------
# (e) end to end on the real model
# ------------------------------------------------------------------------------------------------------------------------------------
def make_model(seed):
    m = DBTextModel()
    m.load_state_dict(O.new_state(seed))
    return m.to(DEV).train()


def micro_batches(seed, count, n=1, size=64):
    return [tuple(t.to(DEV) for t in O.synthetic_batch(n, size, seed=seed + i)) for i in range(count)]


def flat_like(eng, tensors):
    """the tensors of the live parameters (None: zeros) laid out as the engine's flat buffer"""
    out = torch.zeros_like(eng.flat)
    for (_, p), off, t in zip(eng.live_params, eng.offsets, tensors):
        if t is not None:
            out[off:off + p.numel()] = t.detach().reshape(-1)
    return out


def test_trainer_accumulates_clips_and_amsgrad_against_torch():
    """ResNet-18 at 1 x 3 x 64 x 64, two models from one seed, 2 cycles of k = 2 micro-batches.  Model A: DBTrainer with
    FusedAdam(amsgrad, max_grad_norm = c, accumulation_steps = 2).  Model B: the autograd surface, .grad summing the two passes, then
    p.grad.mul_(0.5), clip_grad_norm_(c), torch.optim.Adam(amsgrad=True).step().  c is half of model B's own first-cycle norm (rounded to
    fp32), so the first cycle clips (asserted); the second clips or not as its own norm decides (after one update the loss and its gradient
    are smaller).

    Per cycle, with R = R.adam_step_ex in float64 on each model's own state and accumulated gradient BEFORE the update:
      |A' - R(A)| <= ex_bounds with the kernel's roundings (the kernel test's bound, at the full buffer);
      |A' - B'|   <= that + |R(A) - R(B)| + ex_bounds with torch's roundings on R(B).
    |R(A) - R(B)| is how far the two models' inputs had drifted apart, carried through the update in float64: 0 in the first cycle (the
    accumulated gradients are bit-equal, asserted: the fold is autograd's sum), afterwards what the first update's rounding differences
    and the network made of them.  torch's roundings (foreach Adam, fp32): the coefficient c / (norm + 1e-6) carries the error of torch's
    fp32 norm — taken as it is, |returned norm - float64 norm of B's gradient| / norm — and 2 roundings (coef_err), g coef 1 more (g_round 1);
    lerp_(g, 1 - b1) = m + w (g - m) with w cast to fp32: 4 on the terms of m'; mul_(b2) and addcmul_(value = 1 - b2) with the scalars
    cast: 2 and 3 on the terms of v'; sqrt, / sqrt(bc2), + eps: 4 on the denominator; addcdiv_(value = -lr / bc1): 3 on the update, 1 on
    the difference — the last two as in the kernel.

    last_grad_norm (float64, |s| sqrt(sum)): within (n + 4) 2^-53 relative of the float64 norm of A's accumulator (either sum errs by
    n 2^-53, halved by the root; the root, the product), and of clip_grad_norm_'s return value within that plus the drift |norm(A) - norm(B)| plus the a priori
    bound of a fp32 two-level norm over T tensors of at most n_max elements, (n_max / 2 + T / 2 + 3) U relative (squares, sums of
    positive terms in any order, two roots)."""
    seed, k, lr = 9, 2, 0.005
    mbs = micro_batches(seed, 4)
    A, B = make_model(seed), make_model(seed)
    crit = DBLoss()
    liveB = [p for _, p in B.engine.live_params]
    optB = torch.optim.Adam(liveB, lr=lr, amsgrad=True)
    nmax, T = max(p.numel() for p in liveB), len(liveB)
    optA = trainer = c = None
    for cyc in range(2):
        # ---- model B: the two backward passes
        optB.zero_grad()
        for img, gts in mbs[k * cyc:k * cyc + k]:
            crit(B(img), gts)[4].backward()
        engB = B.engine
        accB = flat_like(engB, [p.grad for p in liveB])
        if c is None:
            c = float(torch.tensor(0.5 * float(R.grad_norm(accB, 0.5)), dtype=torch.float32))
            optA = FusedAdam(A, lr=lr, amsgrad=True, max_grad_norm=c, accumulation_steps=k)
            trainer = DBTrainer(A, DBLoss(), optA, distributed=False)
        stB = [optB.state.get(p, {}) for p in liveB]
        pB0, mB0, vB0, xB0 = [engB.flat.clone()] + [flat_like(engB, [s.get(key) for s in stB]) for key in ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq')]
        for p in liveB:
            p.grad.mul_(0.5)
        tnorm = float(torch.nn.utils.clip_grad_norm_(liveB, c))
        optB.step()
        # ---- model A: the trainer
        engA = A.engine
        trainer.step(*mbs[k * cyc])
        assert not trainer.updated and optA.folded == 1 and optA.step_count == cyc
        pA0, mA0, vA0, xA0 = (t.clone() for t in (engA.flat, optA.exp_avg, optA.exp_avg_sq, optA.max_exp_avg_sq))
        trainer.step(*mbs[k * cyc + 1])
        assert trainer.updated and optA.folded == 0 and optA.step_count == cyc + 1
        torch.cuda.synchronize()
        accA, n = optA.grad_acc, engA.flat.numel()
        if cyc == 0:
            same_bits('cycle 0: the accumulator against autograd\'s summed .grad', accA, accB)
        lrf = float(torch.tensor(lr, dtype=torch.float32))
        pa, ma, va, xa, partsA = R.adam_step_ex(pA0, accA, mA0, vA0, xA0, lrf, B1, B2, EPS, 0.0, cyc + 1, grad_scale=0.5, max_norm=c)
        pb, mb, vb, xb, partsB = R.adam_step_ex(pB0, accB, mB0, vB0, xB0, lr, 0.9, 0.999, 1e-8, 0.0, cyc + 1, grad_scale=0.5, max_norm=c)
        print('cycle %d coefficients: A %.6f B %.6f' % (cyc, float(partsA['coef']), float(partsB['coef'])))
        assert cyc > 0 or (bool(partsA['coef'] < 1) and bool(partsB['coef'] < 1)), 'the first cycle does not clip'
        tag = 'cycle %d ' % cyc
        bmA, bvA, bpA = ex_bounds(partsA, pa, va, B1, B2, n, decay=False)
        within(tag + 'A exp_avg vs fp64', optA.exp_avg, ma, bmA)
        within(tag + 'A exp_avg_sq vs fp64', optA.exp_avg_sq, va, bvA)
        within(tag + 'A max_exp_avg_sq vs fp64', optA.max_exp_avg_sq, xa, bvA)
        within(tag + 'A param vs fp64', engA.flat, pa, bpA)
        normB = float(partsB['norm'])
        _, _, bpB = ex_bounds(partsB, pb, vb, 0.9, 0.999, n, decay=False, g_round=1, m_round=4, v_round=(2, 3),
                              coef_err=abs(tnorm - normB) / normB + 2 * U)
        drift = (pa - pb).abs()
        print(tag + 'drift of the float64 updates: max %.3e' % float(drift.max()))
        within(tag + 'A param vs B param', engA.flat, engB.flat, bpA + drift + bpB)
        # ---- the norm
        normA = float(partsA['norm'])
        last = optA.last_grad_norm
        assert last.dim() == 0 and last.is_cuda and last.dtype == torch.float64
        print(tag + 'last_grad_norm %.9e, float64 %.9e, clip_grad_norm_ %.9e' % (float(last), normA, tnorm))
        assert abs(float(last) - normA) <= (n + 4) * 2.0**-53 * normA
        assert abs(float(last) - tnorm) <= (n + 4) * 2.0**-53 * normA + abs(normA - normB) + (nmax / 2 + T / 2 + 3) * U * normB


# ------------------------------------------------------------------------------------------------------------------------------------
# (f) refusals, checkpoints, hipGraph
# ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    seed = 3
    (img, gts), = micro_batches(seed, 1)
    crit = DBLoss()
    model = make_model(seed)
    opt = FusedAdam(model, lr=0.005, accumulation_steps=2)
    crit(model(img), gts)[4].backward()
    opt.accumulate()
    torch.cuda.synchronize()
    before = model.engine.flat.clone()
    with pytest.raises(RuntimeError, match='1 of accumulation_steps=2'):  # one fold of two: both counts are named
        opt.step()
    torch.cuda.synchronize()
    assert torch.equal(model.engine.flat, before) and opt.step_count == 0 and opt.folded == 1
    crit(model(img), gts)[4].backward()
    with pytest.raises(RuntimeError, match='1 of accumulation_steps=2.*1 ran without'):  # a pass that was not folded is not dropped either
        opt.step()
    assert torch.equal(model.engine.flat, before)
    opt.accumulate()
    opt.step(grad_scale=0.5)
    torch.cuda.synchronize()
    assert not torch.equal(model.engine.flat, before) and opt.step_count == 1 and opt.folded == 0
    with pytest.raises(RuntimeError, match='0 backward passes'):  # nothing new to fold
        opt.accumulate()
    # the bucketed exchange reduces one pass's gradient: refused with k = 2 at construction
    monkeypatch.setenv('DBN_OVERLAP_ALLREDUCE', '1')
    with pytest.raises(RuntimeError, match='accumulation_steps=2'):
        DBTrainer(model, DBLoss(), opt, distributed=False)
    monkeypatch.delenv('DBN_OVERLAP_ALLREDUCE')
    # k = 1 and a second backward pass: the message of before
    model1 = make_model(seed)
    opt1 = FusedAdam(model1, lr=0.005, amsgrad=True)
    for _ in range(2):
        crit(model1(img), gts)[4].backward()
    with pytest.raises(RuntimeError, match=r'2 backward passes ran since the last zero_grad\(\)/step\(\); the flat gradient buffer holds only '
                       r'the last one \(no gradient accumulation on the fused path'):
        opt1.step()


def test_state_dict_round_trip_and_old_checkpoints():
    seed = 4
    (img, gts), = micro_batches(seed, 1)
    model = make_model(seed)
    opt = FusedAdam(model, lr=0.005, amsgrad=True, max_grad_norm=1.0, accumulation_steps=2)
    tr = DBTrainer(model, DBLoss(), opt, distributed=False)
    for _ in range(4):  # two updates: max_exp_avg_sq differs from exp_avg_sq after the second
        tr.step(img, gts)
    sd = opt.state_dict()
    assert set(sd) == {'step', 'exp_avg', 'exp_avg_sq', 'max_exp_avg_sq', 'param_groups'} and 'grad_acc' not in sd
    g = sd['param_groups'][0]
    assert (g['amsgrad'], g['max_grad_norm'], g['accumulation_steps']) == (True, 1.0, 2) and 'params' not in g
    assert not torch.equal(sd['max_exp_avg_sq'], sd['exp_avg_sq']) and bool((sd['max_exp_avg_sq'] >= sd['exp_avg_sq']).all())
    model2 = make_model(seed)
    opt2 = FusedAdam(model2, lr=0.1)
    opt2.load_state_dict(sd)
    assert (opt2.step_count, opt2.amsgrad, opt2.max_grad_norm, opt2.accumulation_steps) == (2, True, 1.0, 2)
    assert opt2.param_groups[0]['lr'] == 0.005
    for name in ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq'):
        assert torch.equal(getattr(opt2, name), sd[name]) and getattr(opt2, name) is not sd[name], name
    # a checkpoint from before the options existed: its hyper-parameters lack them, and there is no max_exp_avg_sq
    old = {'step': 7, 'exp_avg': sd['exp_avg'], 'exp_avg_sq': sd['exp_avg_sq'],
           'param_groups': [{'lr': 0.002, 'betas': (0.9, 0.999), 'eps': 1e-8, 'weight_decay': 0}]}
    opt3 = FusedAdam(make_model(seed), amsgrad=True, max_grad_norm=2.0, accumulation_steps=3)
    opt3.load_state_dict(old)
    assert (opt3.step_count, opt3.amsgrad, opt3.max_grad_norm, opt3.accumulation_steps) == (7, False, None, 1)
    assert opt3.param_groups[0]['lr'] == 0.002 and torch.equal(opt3.exp_avg_sq, sd['exp_avg_sq'])
    assert opt3.state_dict()['max_exp_avg_sq'] is None
    # ... and one that asks for amsgrad without carrying the third moment: zeros
    old['param_groups'][0]['amsgrad'] = True
    opt4 = FusedAdam(make_model(seed))
    opt4.load_state_dict(old)
    assert opt4.amsgrad and opt4.max_exp_avg_sq.shape == opt4.exp_avg.shape and float(opt4.max_exp_avg_sq.abs().max()) == 0.0


def test_graph_step_under_accumulation_is_bit_identical_to_eager():
    """use_graph with k = 2, AMSGrad and clipping: forward + loss + backward replay from the captured graph, the fold, the norm and the
    update stay outside it.  Six calls over changing micro-batches — two eager warm-up calls (cycle 1), the capturing call and a replay
    (cycle 2), two replays (cycle 3) — leave parameters and all three moments bit-equal to six eager calls."""
    seed = 9
    mbs = micro_batches(seed, 3)

    def run(use_graph):
        model = make_model(seed)
        opt = FusedAdam(model, lr=0.005, amsgrad=True, max_grad_norm=0.5, accumulation_steps=2)
        trainer = DBTrainer(model, DBLoss(), opt, distributed=False)
        trainer.use_graph = use_graph
        updates = []
        for it in range(6):
            trainer.step(*mbs[it % 3])
            updates.append(trainer.updated)
        torch.cuda.synchronize()
        assert updates == [False, True] * 3 and opt.step_count == 3
        assert (trainer._graph is not None and trainer._graph['graph'] is not None) == use_graph
        return [t.clone() for t in (model.engine.flat, opt.exp_avg, opt.exp_avg_sq, opt.max_exp_avg_sq, opt.last_grad_norm)]

    eager, graph = run(False), run(True)
    for name, a, b in zip(('param', 'exp_avg', 'exp_avg_sq', 'max_exp_avg_sq', 'last_grad_norm'), eager, graph):
        same_bits('graph vs eager: ' + name, b.reshape(-1), a.reshape(-1))


def test_fit_steps_a_poly_scheduler_on_update_calls_only():
    """fit() with accumulation_steps = 2 over 4 batches and 2 epochs: 8 calls, 4 updates — a per-iteration ('poly') scheduler is stepped 4
    times, `global_steps` counts the 8 calls"""
    from db_text_minimal_amd.train import fit
    seed = 3
    loader = []
    for i in range(4):
        img, gts = O.synthetic_batch(1, 64, seed=seed + i)
        loader.append({'img': img, 'prob_map': gts[0], 'supervision_mask': gts[1], 'thresh_map': gts[2], 'text_area_map': gts[3]})
    model = make_model(seed)
    opt = FusedAdam(model, lr=0.005, amsgrad=True, max_grad_norm=1.0, accumulation_steps=2)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda it: 0.5**it)
    hist = fit(model, DBLoss(), opt, loader, None, epochs=2, scheduler=sched, lrs_mode='poly', device=DEV, pixel_metric=False)
    assert [h['global_steps'] for h in hist] == [4, 8] and opt.step_count == 4 and opt.folded == 0
    assert sched.last_epoch == 4 and abs(opt.param_groups[0]['lr'] - 0.005 * 0.5**4) < 1e-12
