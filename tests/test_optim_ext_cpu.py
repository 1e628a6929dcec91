"""CPU (-m "not gpu"): the host side of the optimizer extensions (optim.py, csrc/optim.hip) — what FusedAdam accepts and
still refuses, the four C entry points as the header declares them, the workspace size query, and tests/optim_ref.py (the float64
restatement the GPU tests compare the kernels with) against torch.optim.Adam and clip_grad_norm_ themselves."""
import ctypes
import re

import pytest
import torch

import optim_ref as R
from db_text_minimal_amd import DBTextModel, FusedAdam, _lib


def test_fused_adam_accepts_the_new_options():
    m = DBTextModel()
    opt = FusedAdam(m, amsgrad=True, max_grad_norm=1.0, accumulation_steps=2)
    assert opt.amsgrad is True and opt.max_grad_norm == 1.0 and opt.accumulation_steps == 2
    g = opt.param_groups[0]
    assert (g['amsgrad'], g['max_grad_norm'], g['accumulation_steps'], g['weight_decay']) == (True, 1.0, 2, 0)
    assert opt.last_grad_norm is None and opt.folded == 0
    for one in (dict(amsgrad=True), dict(max_grad_norm=1.0), dict(accumulation_steps=2)):
        FusedAdam(m, **one)
    plain = FusedAdam(m)
    assert (plain.amsgrad, plain.max_grad_norm, plain.accumulation_steps) == (False, None, 1)


def test_fused_adam_still_refuses():
    m = DBTextModel()
    with pytest.raises(NotImplementedError, match='dbn_adam_step_ex'):  # the message names the entry point that does take it
        FusedAdam(m, weight_decay=0.1)
    with pytest.raises(NotImplementedError):
        FusedAdam(m, weight_decay=0.1, amsgrad=True, max_grad_norm=1.0, accumulation_steps=2)
    for bad in (dict(max_grad_norm=0.0), dict(max_grad_norm=-1.0), dict(accumulation_steps=0), dict(accumulation_steps=1.5)):
        with pytest.raises(ValueError):
            FusedAdam(m, **bad)
    with pytest.raises(RuntimeError, match='accumulation_steps > 1'):
        FusedAdam(m).accumulate()


def test_trainer_refuses_the_bucketed_exchange_under_accumulation(monkeypatch):
    from db_text_minimal_amd import DBLoss, DBTrainer
    m = DBTextModel()
    monkeypatch.setenv('DBN_OVERLAP_ALLREDUCE', '1')
    with pytest.raises(RuntimeError, match='accumulation_steps=2'):
        DBTrainer(m, DBLoss(), FusedAdam(m, accumulation_steps=2), distributed=False)
    assert DBTrainer(m, DBLoss(), FusedAdam(m), distributed=False).accumulation_steps == 1


ENTRIES = {'dbn_grad_accumulate': 'pp' + 'l' + 'i' + 'p',
           'dbn_grad_sqnorm_ws_doubles': 'l',
           'dbn_grad_sqnorm': 'p' + 'l' + 'pp' + 'p',
           'dbn_adam_step_ex': 'ppppp' + 'l' + 'fffff' + 'i' + 'f' + 'p' + 'f' + 'p'}


def test_header_declares_the_entry_points():
    text = open(_lib.HEADER).read()
    for name, kinds in ENTRIES.items():
        assert len(re.findall(r'\b(?:int|long)\s+%s\s*\(' % name, text)) == 1, name
        assert _lib.SIGNATURES[name] == kinds, name
    assert {n for n in ENTRIES if n in _lib.LONG_RETURN} == {'dbn_grad_sqnorm_ws_doubles'}
    assert _lib.SIGNATURES['dbn_adam_step'] == 'pppp' + 'l' + 'ffff' + 'i' + 'f' + 'p'  # the plain step's entry point is as it was
    L = _lib.lib()
    assert L.dbn_grad_sqnorm_ws_doubles.restype is ctypes.c_long and L.dbn_adam_step_ex.restype is ctypes.c_int
    assert L.dbn_adam_step_ex.argtypes[10] is ctypes.c_float and L.dbn_adam_step_ex.argtypes[5] is ctypes.c_long


def test_sqnorm_workspace_size():
    ws = _lib.lib().dbn_grad_sqnorm_ws_doubles
    sizes = [ws(n) for n in (1, 2, 1000, 16384, 16385, 12269378, 2**31, 2**31 + 5, 2**40)]
    assert sizes[0] >= 1 and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert ws(0) == 0


@pytest.mark.parametrize('amsgrad', [False, True])
def test_reference_against_torch_in_float64(amsgrad):
    """tests/optim_ref.py against torch.optim.Adam(amsgrad, weight_decay) + clip_grad_norm_ in float64 on the CPU: 5 updates, each from
    k = 3 accumulated gradients with the mean factor s = 1 / (2 k), weight decay 0.01, max-norm 0.5; the gradient scale alternates so that
    the updates alternately clip and do not (asserted).  Both sides are float64 evaluations of the same real function with a few dozen
    roundings per element and update, each 2^-53 relative, on well-conditioned operations (sums of same-sign or dominated terms, products,
    one quotient, one root): 1e-13 relative is ~1000 roundings of headroom-free float64 and twelve orders below any modelling error."""
    lr, b1, b2, eps, wd, c, k = 0.005, 0.9, 0.999, 1e-8, 0.01, 0.5, 3
    s = 1.0 / (2 * k)
    g = torch.Generator().manual_seed(11)
    shapes = [(7, 5), (33, ), (2, 3, 4)]
    params = [torch.randn(sh, generator=g, dtype=torch.float64).requires_grad_() for sh in shapes]
    opt = torch.optim.Adam(params, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, amsgrad=amsgrad)
    flat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts])
    p = flat(params).clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    vmax = torch.zeros_like(p) if amsgrad else None
    clipped = []
    for step in range(1, 6):
        scale = 30.0 if step % 2 else 0.03  # norm ~ s sqrt(3 x 92) scale = 2.8 scale: 83 and 0.083 around c = 0.5
        micro = [[torch.randn(sh, generator=g, dtype=torch.float64) * scale for sh in shapes] for _ in range(k)]
        for q in params:
            q.grad = None
        for mb in micro:  # .grad sums the passes in order, as autograd does
            for q, gq in zip(params, mb):
                q.grad = gq.clone() if q.grad is None else q.grad + gq
        acc = flat([q.grad for q in params]).clone()
        for q in params:
            q.grad.mul_(s)
        tnorm = torch.nn.utils.clip_grad_norm_(params, c)
        opt.step()
        p, m, v, vmax, parts = R.adam_step_ex(p, acc, m, v, vmax, lr, b1, b2, eps, wd, step, grad_scale=s, max_norm=c)
        clipped.append(bool(parts['coef'] < 1))
        assert abs(float(parts['norm']) - float(tnorm)) <= 1e-13 * float(tnorm)
        st = [opt.state[q] for q in params]
        pairs = [('param', p, flat(params)), ('exp_avg', m, flat([t['exp_avg'] for t in st])),
                 ('exp_avg_sq', v, flat([t['exp_avg_sq'] for t in st]))]
        if amsgrad:
            pairs.append(('max_exp_avg_sq', vmax, flat([t['max_exp_avg_sq'] for t in st])))
        for name, mine, theirs in pairs:
            err = float(((mine - theirs).abs() / theirs.abs().clamp_min(1e-300)).max())
            assert err <= 1e-13, (name, step, err)
    assert clipped == [True, False, True, False, True]


def test_reference_options_off_is_the_plain_step():
    """With no clipping, no decay and no AMSGrad the restatement is tests/bn_pool_ref.py's adam_step (the plain step's reference)"""
    import bn_pool_ref as B
    g = torch.Generator().manual_seed(3)
    p, grad, m, v = (torch.randn(50, generator=g, dtype=torch.float64) for _ in range(4))
    v = v.abs()
    mine = R.adam_step_ex(p, grad, m, v, None, 0.005, 0.9, 0.999, 1e-8, 0.0, 2, grad_scale=0.25)
    theirs = B.adam_step(p, grad, m, v, 0.005, 0.9, 0.999, 1e-8, 2, grad_scale=0.25)
    for a, b in zip(mine[:3], theirs[:3]):
        assert torch.equal(a, b)
    assert mine[3] is None and float(mine[4]['coef']) == 1.0


def test_nan_norm_propagates():
    """error_if_nonfinite=False: a NaN in the gradient makes the coefficient NaN and every parameter NaN"""
    acc = torch.tensor([1.0, float('nan'), 2.0], dtype=torch.float64)
    out = R.adam_step_ex(torch.ones(3), acc, torch.zeros(3), torch.zeros(3), None, 0.005, 0.9, 0.999, 1e-8, 0.0, 1, max_norm=1.0)
    assert bool(torch.isnan(out[0]).all()) and bool(torch.isnan(out[4]['coef']))
