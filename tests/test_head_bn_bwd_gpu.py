"""-m gpu: dbn_head_tail_bn_bwd_t — the DB head's tail backward through the BatchNorm in front of each branch's last ConvT in one call,
the two [npx, 64] gradients between them formed again inside the BatchNorm apply pass instead of stored (csrc/head_loss.hip,
csrc/bn_bwd_apply.h).

  (a) bit identity with the sequence it replaces (dbn_head_tail_bwd_t with the fused sums, then dbn_bn_backward_t per branch with the
      sums given, the recomputed ReLU mask and dbias_conv) on the same operands: every output torch.equal, in every storage type
      Engine.head_bwd_fused_ats enables;
  (b) accuracy against the float64 reference tests/head_bn_bwd_ref.py at (2, 7, 9), with the bounds of tests/test_train16_ops_gpu.py
      (ht_check) and tests/test_bn_pool_ops_gpu.py (bwd_check, bwd_dy_bound) for the same quantities, composed — see hb_bounds;
  (c) one DBTrainer step with Engine.head_bwd_fused on and off from the same seed: the flat gradient buffers are torch.equal.
Every output and workspace starts as NaN."""
import math

import pytest
import torch

import head_bn_bwd_ref as R
from gpu_util import DEV, DT, ETA, NAN, SR, U, L, exact, gen, stream, within
from db_text_minimal_amd import _lib
from db_text_minimal_amd.engine import Engine

pytestmark = pytest.mark.gpu

KSTEP = 50.0
GS = float(torch.tensor(0.7, dtype=torch.float32))  # a grad_scale that is no power of two, as the float the entry points receive
STREAM_ITEMS = 768 * 256  # STREAM_BLOCKS (csrc/bn_bwd_apply.h) workgroups of 256 threads: the apply pass's grid stride at its cap
ATS = list(Engine.head_bwd_fused_ats)
assert 0 in ATS, 'fp32 storage must take the fused path'


def big_shape(at):
    """Just above 4 x STREAM_BLOCKS x 256 items (16 per quarter pixel on fp32 storage, 8 on 16-bit) with a ragged remainder: every thread
    runs the four-fold unrolled loop of the apply pass and some the tail behind it; the sums pass runs at its cap of 2047 workgroups."""
    shape = (3, 127, 131) if at == 0 else (3, 181, 183)
    items = shape[0] * shape[1] * shape[2] * (16 if at == 0 else 8)
    assert 4 * STREAM_ITEMS < items < 5 * STREAM_ITEMS and items % 256 != 0
    return shape


SHAPES = {'idle': lambda at: (1, 4, 4),      # fewer items than one row of workgroups: most of them idle
          'odd': lambda at: (2, 7, 9),       # odd sizes, a pixel count that is no multiple of 16, row and image carries
          'unrolled': big_shape}


def inputs(at, N, Hq, Wq, CH, seed):
    g = gen(seed)
    dt = DT[at]
    r = lambda *shape, scale=1.0: torch.randn(*shape, generator=g, device=DEV) * scale
    u = lambda *shape: torch.rand(*shape, generator=g, device=DEV) * 0.96 + 0.02  # maps in (0.02, 0.98)
    t = {'preds': u(N, CH, 2 * Hq, 2 * Wq), 'dpreds': r(N, CH, 2 * Hq, 2 * Wq, scale=0.1)}
    for br in 'bt':
        t['y' + br] = r(N, Hq, Wq, 64).to(dt)
        t['w' + br] = r(64, 4, scale=0.2)
        t['bn' + br] = {'scale': r(64, scale=0.3) + 1, 'shift': r(64, scale=0.5), 'mean': r(64, scale=0.2),
                        'rstd': torch.rand(64, generator=g, device=DEV) + 0.5, 'gamma': r(64, scale=0.3) + 1}
    return t


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def outputs(at, N, Hq, Wq):
    o = {}
    for br in 'bt':
        o['dy' + br] = nan(N, Hq, Wq, 64, dtype=DT[at])
        o.update({k + br: nan(64) for k in ('dgamma', 'dbeta', 'dbias3')})
        o['dw' + br], o['db' + br] = nan(256), nan(1)
    return o


def run_fused(at, t, N, Hq, Wq, CH, phases=(3, )):
    o = outputs(at, N, Hq, Wq)
    ws = nan(L().dbn_head_tail_bn_bwd_ws_floats())
    p = lambda x: x.data_ptr()
    bn = [t['bnb'], t['bnt']]
    for ph in phases:
        _lib.check(L().dbn_head_tail_bn_bwd_t(
            at, ph, p(t['yb']), p(t['yt']), p(t['wb']), p(t['wt']), p(t['preds']), p(t['dpreds']), p(bn[0]['scale']), p(bn[0]['shift']),
            p(bn[1]['scale']), p(bn[1]['shift']), p(bn[0]['mean']), p(bn[0]['rstd']), p(bn[1]['mean']), p(bn[1]['rstd']), p(bn[0]['gamma']),
            p(bn[1]['gamma']), p(o['dyb']), p(o['dyt']), p(o['dgammab']), p(o['dbetab']), p(o['dgammat']), p(o['dbetat']), p(o['dbias3b']),
            p(o['dbias3t']), p(o['dwb']), p(o['dbb']), p(o['dwt']), p(o['dbt']), N, Hq, Wq, CH, KSTEP, GS, p(ws), stream()), 'head_tail_bn_bwd_t')
    torch.cuda.synchronize()
    return o


def run_sequence(at, t, N, Hq, Wq, CH):
    """What Engine.backward launched before: the head tail with the BatchNorm sums, then each branch's BatchNorm backward."""
    o = outputs(at, N, Hq, Wq)
    p = lambda x: x.data_ptr()
    bn = {'b': t['bnb'], 't': t['bnt']}
    dz = {br: nan(N, Hq, Wq, 64, dtype=DT[at]) for br in 'bt'}
    sums = nan(4, 64)
    ws = nan(L().dbn_head_tail_bwd_ws_floats())
    _lib.check(L().dbn_head_tail_bwd_t(
        at, p(t['yb']), p(t['yt']), p(t['wb']), p(t['wt']), p(t['preds']), p(t['dpreds']), p(bn['b']['scale']), p(bn['b']['shift']),
        p(bn['t']['scale']), p(bn['t']['shift']), p(bn['b']['mean']), p(bn['b']['rstd']), p(bn['t']['mean']), p(bn['t']['rstd']), p(sums),
        p(dz['b']), p(dz['t']), p(o['dwb']), p(o['dbb']), p(o['dwt']), p(o['dbt']), N, Hq, Wq, CH, KSTEP, GS, p(ws), stream()), 'head_tail_bwd_t')
    M = N * Hq * Wq
    for i, br in enumerate('bt'):
        rws = nan(L().dbn_reduce_ws_floats(64))
        b = bn[br]
        _lib.check(L().dbn_bn_backward_t(at, p(sums[2 * i:2 * i + 2]), 1, p(t['y' + br]), None, p(b['scale']), p(b['shift']), p(dz[br]),
                                         p(b['mean']), p(b['rstd']), p(b['gamma']), p(o['dy' + br]), None, 0, p(o['dgamma' + br]),
                                         p(o['dbeta' + br]), p(o['dbias3' + br]), M, 64, GS, p(rws), stream()), 'bn_backward_t')
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize('at', ATS)
@pytest.mark.parametrize('CH', [3, 2])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_fused_head_bn_backward_equals_the_sequence_bit_for_bit(shape, CH, at):
    N, Hq, Wq = SHAPES[shape](at)
    t = inputs(at, N, Hq, Wq, CH, seed=7 + 3 * N + CH)
    want = run_sequence(at, t, N, Hq, Wq, CH)
    got = run_fused(at, t, N, Hq, Wq, CH)
    for k in want:
        assert bool(torch.isfinite(want[k].float()).all()), 'the sequence left %s non-finite' % k
        assert torch.equal(got[k], want[k]), '%s differs at %s CH=%d at=%d: %d of %d elements, max |diff| %.3e' % (
            k, (N, Hq, Wq), CH, at, int((got[k] != want[k]).sum()), want[k].numel(), float((got[k].float() - want[k].float()).abs().max()))


@pytest.mark.parametrize('at', ATS)
def test_fused_head_bn_backward_in_two_phases_equals_one_call(at):
    """phases 1 then 2 (how the engine calls it, to bracket the two passes for its profiler) = phases 3."""
    N, Hq, Wq = SHAPES['odd'](at)
    t = inputs(at, N, Hq, Wq, 3, seed=5)
    one, two = run_fused(at, t, N, Hq, Wq, 3), run_fused(at, t, N, Hq, Wq, 3, phases=(1, 2))
    for k in one:
        assert torch.equal(one[k], two[k]), k


def stream_grid(total, Cq):
    """bn_stream_grid of csrc/bn_bwd_apply.h (as tests/test_bn_pool_ops_gpu.py)."""
    g = min(max(-(-total // 256), 1), 768)
    m = (Cq // 4) // math.gcd(Cq // 4, 256)
    return -(-g // m) * m


def hb_bounds(at, r, A, w, bn, M, depth):
    """Bounds of one branch's outputs against the float64 result r of head_bn_bwd_ref.branch_backward, composed from the existing ones.
    u = 2^-24, s = SR[at], eta = ETA[at]; depth = the sums pass's pixels per lane (ht_walk).
      dw6, dbias6   ht_check:  |gs| (depth + 28) u sum_px |x| A + u |ref|   and   |gs| (depth + 29) u sum A + u |ref|
      g             the gradient the apply pass forms is ht_check's dx: eg = s |g64| + (1 + s) 12 u (A |w|^T) + eta (0 where masked)
      sums          ht_check bounds the kernel's sums against the float64 sums of ITS OWN g: (depth + 17) u sum |g| + u |s1| and
                    (depth + 20) u sum |g xhat| + u |s2|; against the float64 g the terms' own errors add: E1 = ... + sum eg,
                    E2 = ... + sum eg |xhat| (and |g| <= |g64| + eg inside the chains)
      dbeta, dgamma bwd_check with the sums given: the fold is float64, times grad_scale, cast once: |gs| E + u |ref|
      dy            bwd_dy_bound with e1 = E1 / M + u |c1|, e2 = E2 / M + u |c2| and the error of g itself beside them:
                    e32 = |gamma rstd| (eg + e1 + |xhat| e2 + 7 u A'), A' = |g64| + eg + |c1| + |xhat c2|;  stored: e32 + s (|dy| + e32) + eta."""
    s, eta = SR[at], ETA[at]
    d = lambda x: x.double()
    wabs = d(w).reshape(64, 4).abs()
    eg = (s * r['g'].abs() + (1 + s) * 12 * U * (A @ wabs.t()) + eta) * r['mask']
    xa = r['xhat'].abs()
    E1 = (depth + 17) * U * (r['abs1'] + eg.sum(0)) + U * (r['dbeta'] / GS).abs() + eg.sum(0)
    E2 = (depth + 20) * U * (r['abs2'] + (eg * xa).sum(0)) + U * (r['dgamma'] / GS).abs() + (eg * xa).sum(0)
    e1, e2 = E1 / M + U * r['c1'].abs(), E2 / M + U * r['c2'].abs()
    Ap = r['g'].abs() + eg + r['c1'].abs() + (r['xhat'] * r['c2']).abs()
    e32 = (d(bn['gamma']) * d(bn['rstd'])).abs() * (eg + e1 + xa * e2 + 7 * U * Ap)
    return {'dw': abs(GS) * (depth + 28) * U * (r['x'].abs().t() @ A) + U * r['dw6'].abs(),
            'db': abs(GS) * (depth + 29) * U * A.sum() + U * r['dbias6'].abs(),
            'dbeta': abs(GS) * E1 + U * r['dbeta'].abs(), 'dgamma': abs(GS) * E2 + U * r['dgamma'].abs(),
            'dy': e32 + s * (r['dy1'].abs() + e32) + eta}


@pytest.mark.parametrize('at', ATS)
def test_fused_head_bn_backward_vs_fp64(at):
    """Random operands at (2, 7, 9), three maps, k = 50, grad_scale fp32(0.7), against float64 on the operands as stored; bounds: hb_bounds.
    The ConvT bias gradient (dbias3) is the column sum of dy AS THE KERNEL STORED IT (bwd_check): a chain of the thread's items plus
    the 256 / cin threads added in LDS, folded in float64: |gs| (chain + 2) u sum |dy| + u |ref|."""
    N, Hq, Wq = 2, 7, 9
    M = N * Hq * Wq
    t = inputs(at, N, Hq, Wq, 3, seed=13)
    got = run_fused(at, t, N, Hq, Wq, 3)
    cpu = lambda x: {k: v.cpu() for k, v in x.items()} if isinstance(x, dict) else x.cpu()
    rb, rt, A = R.head_bn_bwd(cpu(t['yb']), cpu(t['yt']), cpu(t['wb']), cpu(t['wt']), cpu(t['preds']), cpu(t['dpreds']), cpu(t['bnb']),
                              cpu(t['bnt']), N, Hq, Wq, 3, KSTEP, GS)
    nb = min(max(-(-M * 16 // 256), 1), 2047)
    depth = -(-M // (16 * nb))
    cin = 16 if at == 0 else 8
    chain = -(-M * cin // (stream_grid(M * cin, 64 if at == 0 else 32) * 256)) + 256 // cin
    for i, (br, r) in enumerate((('b', rb), ('t', rt))):
        b = hb_bounds(at, r, A[i], cpu(t['w' + br]), cpu(t['bn' + br]), M, depth)
        tag = 'head bn bwd %s at=%d ' % (br, at)
        within(tag + 'dw6', got['dw' + br].cpu(), r['dw6'], b['dw'])
        within(tag + 'dbias6', got['db' + br].cpu(), r['dbias6'].view(1), b['db'])
        within(tag + 'dbeta', got['dbeta' + br].cpu(), r['dbeta'], b['dbeta'])
        within(tag + 'dgamma', got['dgamma' + br].cpu(), r['dgamma'], b['dgamma'])
        within(tag + 'dy1', got['dy' + br].cpu(), r['dy1'], b['dy'])
        dyk = got['dy' + br].cpu().double().reshape(M, 64)
        bref = dyk.sum(0) * GS
        within(tag + 'dbias3', got['dbias3' + br].cpu(), bref, abs(GS) * (chain + 2) * U * dyk.abs().sum(0) + U * bref.abs())


def test_trainer_step_gradients_equal_with_and_without_the_fused_head_backward():
    """One DBTrainer step at 2 x 3 x 64 x 64 from the same seed with Engine.head_bwd_fused on and off: the same flat gradient, bit for bit,
    and the fused path never allocates the two 64-channel gradients."""
    from db_text_minimal_amd import DBLoss, DBTextModel, DBTrainer, FusedAdam
    from oracle import dbnet_oracle as O
    img, gts = O.synthetic_batch(2, 64, seed=5)
    sd = O.new_state(5)
    grads = {}
    for fused in (True, False):
        model = DBTextModel()
        model.load_state_dict(sd)
        model = model.to(DEV).train()
        model.engine.head_bwd_fused = fused
        trainer = DBTrainer(model, DBLoss(), FusedAdam(model, lr=0.005))
        trainer.step(img.to(DEV), gts.to(DEV))
        torch.cuda.synchronize()
        grads[fused] = model.engine.flat_grad.clone()
        assert ('binarize/dz1' in model.engine.bufs) == (not fused) and ('thresh/dz1' in model.engine.bufs) == (not fused)
        assert 'binarize/dy1' in model.engine.bufs and 'thresh/dy1' in model.engine.bufs
    assert bool(torch.isfinite(grads[True]).all())
    assert torch.equal(grads[True], grads[False]), '%d of %d gradient elements differ' % (int((grads[True] != grads[False]).sum()), grads[True].numel())
