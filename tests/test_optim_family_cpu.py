"""CPU (-m "not gpu"): the host side of the optimizer family (optim.py, lr_schedulers.py, csrc/optim_groups.hip) —
tests/optim_family_ref.py against torch's own optimizers in float64, the proof that the GPU tests' bounds tell wrong rules apart, the run
builder, the refusals, WarmupPolyLR against its closed form, and the C entry points as the header declares them."""
import ctypes
import re
import warnings

import pytest
import torch

import optim_family_ref as F
import optim_ref as R
from db_text_minimal_amd import DBTextModel, FusedAdam, FusedAdamW, FusedSGD, WarmupPolyLR, _lib, split_decay
from db_text_minimal_amd.engine import flat_layout
from db_text_minimal_amd.optim import MAX_GROUPS, MAX_RUNS, build_runs

SHAPES = [(7, 5), (33, ), (2, 3, 4)]  # the first and the last form group 0, the middle one group 1


def flat(ts):
    return torch.cat([t.detach().reshape(-1) for t in ts])


def spread(values, groups):
    """the per-element vector of a per-group value over SHAPES laid end to end"""
    return torch.cat([torch.full((torch.Size(sh).numel(), ), float(values[g]), dtype=torch.float64) for sh, g in zip(SHAPES, groups)])


def rel_err(mine, theirs):
    return float(((mine - theirs).abs() / theirs.abs().clamp_min(1e-300)).max())


def updates(params, k, s, c, seed):
    """5 updates' worth of gradients: k micro-batches each, summed into .grad in pass order, scaled by s and clipped to c as the torch
    side does it; yields (step, acc) after leaving the clipped gradient in .grad.  The scale alternates so that the updates alternately
    clip and do not."""
    g = torch.Generator().manual_seed(seed)
    for step in range(1, 6):
        scale = 30.0 if step % 2 else 0.03
        for q in params:
            q.grad = None
        for _ in range(k):
            for q in params:
                gq = torch.randn(q.shape, generator=g, dtype=torch.float64) * scale
                q.grad = gq if q.grad is None else q.grad + gq
        acc = flat([q.grad for q in params]).clone()
        for q in params:
            q.grad.mul_(s)
        tnorm = torch.nn.utils.clip_grad_norm_(params, c)
        yield step, acc, float(tnorm)


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. the restatements against torch in float64
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grouped', [False, True])
@pytest.mark.parametrize('decay', [False, True])
@pytest.mark.parametrize('mode', list(F.SGD_MODES))
def test_sgd_reference_against_torch_in_float64(mode, decay, grouped):
    """F.sgd_step against torch.optim.SGD with clip_grad_norm_ in front, float64 on the CPU, 5 updates from k = 3 accumulated gradients
    with the mean factor 1 / (2 k); to 1e-13 relative for the reason test_optim_ext_cpu.py gives (a few dozen float64 roundings on
    well-conditioned operations)."""
    mu, damp, nesterov = F.SGD_MODES[mode]
    lrs, wds = (0.1, 0.03), ((0.05, 0.2) if decay else (0.0, 0.0))
    groups = [0, 1, 0] if grouped else [0, 0, 0]
    k, c = 3, 0.5
    s = 1.0 / (2 * k)
    g = torch.Generator().manual_seed(5)
    params = [torch.randn(sh, generator=g, dtype=torch.float64).requires_grad_() for sh in SHAPES]
    tgroups = [{'params': [q for q, gi in zip(params, groups) if gi == i], 'lr': lrs[i], 'weight_decay': wds[i]} for i in sorted(set(groups))]
    opt = torch.optim.SGD(tgroups, lr=lrs[0], momentum=mu, dampening=damp, nesterov=nesterov)
    lr, wd = spread(lrs, groups), spread(wds, groups)
    p, buf = flat(params).clone(), None
    clipped = []
    for step, acc, tnorm in updates(params, k, s, c, seed=21):
        opt.step()
        p, buf, parts = F.sgd_step(p, acc, buf, lr, wd, mu, damp, nesterov, step == 1, grad_scale=s, max_norm=c)
        clipped.append(bool(parts['coef'] < 1))
        assert abs(float(parts['norm']) - tnorm) <= 1e-13 * tnorm
        assert rel_err(p, flat(params)) <= 1e-13, (step, rel_err(p, flat(params)))
        if mu:
            assert rel_err(buf, flat([opt.state[q]['momentum_buffer'] for q in params])) <= 1e-13, step
        else:
            assert buf is None
    assert clipped == [True, False, True, False, True]


@pytest.mark.parametrize('amsgrad', [False, True])
@pytest.mark.parametrize('decoupled', [True, False])
def test_adamw_reference_against_torch_in_float64(decoupled, amsgrad):
    """F.adamw_step against torch.optim.AdamW (decoupled) and torch.optim.Adam(weight_decay) (coupled), two groups, as above"""
    lrs, wds, groups = (0.005, 0.02), (0.1, 0.3), [0, 1, 0]
    b1, b2, eps, k, c = 0.9, 0.999, 1e-8, 3, 0.5
    s = 1.0 / (2 * k)
    g = torch.Generator().manual_seed(6)
    params = [torch.randn(sh, generator=g, dtype=torch.float64).requires_grad_() for sh in SHAPES]
    tgroups = [{'params': [q for q, gi in zip(params, groups) if gi == i], 'lr': lrs[i], 'weight_decay': wds[i]} for i in (0, 1)]
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(tgroups, lr=lrs[0], betas=(b1, b2), eps=eps, amsgrad=amsgrad)
    lr, wd = spread(lrs, groups), spread(wds, groups)
    p = flat(params).clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    vmax = torch.zeros_like(p) if amsgrad else None
    for step, acc, tnorm in updates(params, k, s, c, seed=22):
        opt.step()
        p, m, v, vmax, parts = F.adamw_step(p, acc, m, v, vmax, lr, b1, b2, eps, wd, step, decoupled, grad_scale=s, max_norm=c)
        st = [opt.state[q] for q in params]
        pairs = [('param', p, flat(params)), ('exp_avg', m, flat([t['exp_avg'] for t in st])), ('exp_avg_sq', v, flat([t['exp_avg_sq'] for t in st]))]
        if amsgrad:
            pairs.append(('max_exp_avg_sq', vmax, flat([t['max_exp_avg_sq'] for t in st])))
        for name, mine, theirs in pairs:
            assert rel_err(mine, theirs) <= 1e-13, (name, step, rel_err(mine, theirs))


def test_ema_reference_against_torch_in_float64():
    """F.ema_step is torch's lerp form of the average, shadow + (1 - d) (p - shadow), to float64 rounding"""
    g = torch.Generator().manual_seed(7)
    shadow, p = (torch.randn(50, generator=g, dtype=torch.float64) for _ in range(2))
    mine, terms = F.ema_step(shadow, p, 0.9, 1 - 0.9)
    assert rel_err(mine, torch.lerp(shadow, p, 1 - 0.9)) <= 1e-13 and bool((terms >= mine.abs()).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. the GPU tests' bounds tell wrong rules apart
# ------------------------------------------------------------------------------------------------------------------------------------
def differs(tag, right, wrong, bound):
    frac = float(((right - wrong).abs() > 100 * bound).double().mean())
    print('%s: the wrong rule is more than 100 bounds away on %.3f of the elements' % (tag, frac))
    assert frac > 0.5, (tag, frac)


def test_wrong_rules_are_told_apart():
    """On the data of tests/test_optim_family_gpu.py (F.family_data, n = 1023, two groups, the clipped case: coefficient 1/2) each wrong
    variant of a rule lands more than 100 times the GPU test's bound away from the right one on more than half of the elements.  The
    learning rates (0.1, 0.05) and decays (0.5, 0.25) are as large as they are for this: the decoupled decay applied after the update
    differs by lr wd |update| ~ lr^2 wd from the right order, which at lr = 0.005, wd = 0.01 would be within a few roundings of p."""
    n = 1023
    p, grads = F.family_data(n, n)
    ends, groups = F.two_runs(n)
    lr, wd = F.per_element(F.LRS, ends, groups, n), F.per_element(F.WDS, ends, groups, n)
    c = float(torch.tensor(0.5 * float(R.grad_norm(grads[0], F.GS)), dtype=torch.float32))
    kw = dict(grad_scale=F.GS, max_norm=c)

    def sgd(mode, wrong=None, lr=lr):
        mu, damp, nesterov = F.SGD_MODES[mode]
        return F.sgd_step(p, grads[0], None, lr, wd, mu, damp, nesterov, True, wrong=wrong, **kw)

    for mode, wrong in (('dampening', 'dampen_first'), ('momentum', 'decay_before_clip'), ('nesterov', 'no_nesterov')):
        p1, _, parts = sgd(mode)
        assert bool(parts['coef'] < 1)
        differs('sgd %s' % wrong, p1, sgd(mode, wrong)[0], F.sgd_bounds(parts, p1, n, decay=True)[1])
    swapped = F.per_element(F.LRS[::-1], ends, groups, n)
    p1, _, parts = sgd('momentum')
    differs('sgd lr of the neighbour group', p1, sgd('momentum', lr=swapped)[0], F.sgd_bounds(parts, p1, n, decay=True)[1])

    z = torch.zeros(n, dtype=torch.float64)
    adam = lambda wrong=None, lr=lr: F.adamw_step(p, grads[0], z, z, None, lr, F.B1, F.B2, F.EPS, wd, 1, True, wrong=wrong, **kw)
    p1, _, v1, _, parts = adam()
    bp = F.adam_bounds(parts, p1, v1, F.B1, F.B2, n, decay=False, decoupled=True)[2]
    differs('adamw decay after the update', p1, adam('decay_after')[0], bp)
    differs('adamw lr of the neighbour group', p1, adam(lr=swapped)[0], bp)


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. the run builder
# ------------------------------------------------------------------------------------------------------------------------------------
def test_build_runs_by_hand():
    sizes = [1, 3, 4, 5, 1023]  # quads: 1, 1, 1, 2, 256 -> ends 1, 2, 3, 5, 261
    offs, total = flat_layout(sizes)
    assert offs == [0, 4, 8, 12, 20] and total == 1044
    assert build_runs(offs, sizes, [0, 0, 0, 0, 0]) == ([261], [0])
    assert build_runs(offs, sizes, [0, 1, 0, 1, 0]) == ([1, 2, 3, 5, 261], [0, 1, 0, 1, 0])
    assert build_runs(offs, sizes, [2, 2, 1, 1, 2]) == ([2, 5, 261], [2, 1, 2])  # adjacent parameters of one group merge
    assert build_runs(offs, sizes, [0, 0, 0, 1, 1]) == ([3, 261], [0, 1])
    # padding stays with its parameter: the size-5 tensor owns both of its quads (elements 12 .. 19), the size-1 tensor all of quad 0
    assert build_runs(offs, sizes, [1, 0, 0, 3, 0]) == ([1, 3, 5, 261], [1, 0, 3, 0])
    with pytest.raises(ValueError):
        build_runs([0, 2], [1, 1], [0, 1])  # not flat_layout's packing
    with pytest.raises(ValueError):
        build_runs(offs, sizes, [0, 0])


def test_build_runs_on_the_model_with_split_decay():
    """every quad's group equals the group of the parameter whose range contains it, by brute force; well under the cap of runs"""
    m = DBTextModel()
    opt = FusedSGD(m, lr=0.1, param_groups=split_decay(m, 1e-4))
    live = m.engine.live_params
    sizes = [p.numel() for _, p in live]
    offs, total = flat_layout(sizes)
    gop = opt.group_of_params()
    assert [g for g, (_, p) in zip(gop, live)] == [0 if p.ndim >= 2 else 1 for _, p in live]
    ends, groups = build_runs(offs, sizes, gop)
    assert ends == sorted(set(ends)) and ends[-1] == total // 4 and len(ends) == len(groups) < 100 <= MAX_RUNS
    assert all(a != b for a, b in zip(groups, groups[1:]))  # maximal runs
    by_param = torch.full((total // 4, ), -1, dtype=torch.int64)
    for off, n, g in zip(offs, sizes, gop):
        by_param[off // 4:(off + n + 3) // 4] = g
    assert int(by_param.min()) >= 0
    by_run = F.per_element(groups, ends, list(range(len(ends))), total, dtype=torch.int64)[::4]
    assert torch.equal(by_run, by_param)
    print('ResNet-18 with split_decay: %d parameters in %d runs' % (len(sizes), len(ends)))


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. what the classes accept and refuse
# ------------------------------------------------------------------------------------------------------------------------------------
def test_groups_become_param_groups():
    m = DBTextModel()
    live = [p for _, p in m.engine.live_params]
    opt = FusedAdamW(m, lr=0.01, weight_decay=0.1, param_groups=[{'params': live[:3], 'lr': 0.001}, {'params': [live[5]], 'weight_decay': 0.0}])
    assert [(g['lr'], g['weight_decay'], len(g['params'])) for g in opt.param_groups] == [(0.001, 0.1, 3), (0.01, 0.0, 1), (0.01, 0.1, len(live) - 4)]
    assert all(g['decoupled'] is True and g['betas'] == (0.9, 0.999) for g in opt.param_groups)
    a, b = split_decay(m, 1e-4)
    assert a['weight_decay'] == 1e-4 and b['weight_decay'] == 0.0 and len(a['params']) + len(b['params']) == len(live)
    assert all(p.ndim >= 2 for p in a['params']) and all(p.ndim < 2 for p in b['params'])
    sgd = FusedSGD(m, lr=0.1, momentum=0.9, param_groups=[a, b], ema_decay=0.99, max_grad_norm=1.0, accumulation_steps=2)
    assert len(sgd.param_groups) == 2 and (sgd.ema_decay, sgd.max_grad_norm, sgd.accumulation_steps, sgd.folded) == (0.99, 1.0, 2, 0)
    assert sgd.last_grad_norm is None and sgd.grad_acc is None
    sched = WarmupPolyLR(sgd, warmup_iters=10)  # a torch scheduler accepts it and drives every group
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')  # (no update ran before the scheduler: there is no device here)
        sched.step()
    assert sgd.param_groups[0]['lr'] == sgd.param_groups[1]['lr'] == pytest.approx(0.1 * (1 / 3 * 0.9 + 0.1))


def test_refusals():
    m = DBTextModel()
    live = [p for _, p in m.engine.live_params]
    for cls, kw in ((FusedSGD, dict(lr=0.1)), (FusedAdamW, {})):
        with pytest.raises(ValueError, match='second time'):
            cls(m, param_groups=[{'params': live[:2]}, {'params': live[1:3]}], **kw)
        with pytest.raises(ValueError, match='not a live parameter'):
            cls(m, param_groups=[{'params': [torch.nn.Parameter(torch.zeros(3))]}], **kw)
        with pytest.raises(ValueError, match='at most %d' % MAX_GROUPS):
            cls(m, param_groups=[{'params': [live[i]], 'lr': 0.1 * (i + 1)} for i in range(MAX_GROUPS)], **kw)
        cls(m, param_groups=[{'params': [live[i]], 'lr': 0.1 * (i + 1)} for i in range(MAX_GROUPS - 1)], **kw)  # 7 and the rest: 8
        for bad in (dict(max_grad_norm=0.0), dict(accumulation_steps=0), dict(accumulation_steps=1.5), dict(ema_decay=1.0)):
            with pytest.raises(ValueError):
                cls(m, **kw, **bad)
        with pytest.raises(RuntimeError, match=cls.__name__ + r'\.accumulate\(\) needs accumulation_steps > 1'):
            cls(m, **kw).accumulate()
        with pytest.raises(RuntimeError, match='needs ema_decay'):
            cls(m, **kw).ema_state_dict()
    with pytest.raises(ValueError, match="sets 'momentum'"):
        FusedSGD(m, lr=0.1, momentum=0.9, param_groups=[{'params': live[:2], 'momentum': 0.5}])
    FusedSGD(m, lr=0.1, momentum=0.9, param_groups=[{'params': live[:2], 'momentum': 0.9}])  # the default's own value is no difference
    with pytest.raises(ValueError, match="sets 'betas'"):
        FusedAdamW(m, param_groups=[{'params': live[:2], 'betas': (0.8, 0.999)}])
    with pytest.raises(ValueError, match="sets 'colour'"):
        FusedAdamW(m, param_groups=[{'params': live[:2], 'colour': 1}])
    # nesterov, as torch.optim.SGD
    for bad in (dict(momentum=0), dict(momentum=0.9, dampening=0.1)):
        with pytest.raises(ValueError, match='Nesterov momentum requires a momentum and zero dampening'):
            FusedSGD(m, lr=0.1, nesterov=True, **bad)
        with pytest.raises(ValueError, match='Nesterov momentum requires a momentum and zero dampening'):
            torch.optim.SGD(live, lr=0.1, nesterov=True, **bad)
    # the split stays deliberate: weight decay is FusedAdamW's, FusedAdam still refuses it
    with pytest.raises(NotImplementedError, match='dbn_adam_step_ex'):
        FusedAdam(m, weight_decay=0.1)
    assert FusedAdamW(m, weight_decay=0.1, decoupled=False).param_groups[0]['weight_decay'] == 0.1


def test_ema_factors():
    m = DBTextModel()
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
    opt = FusedSGD(m, lr=0.1, ema_decay=0.999)
    assert opt.ema_factors(1) == opt.ema_factors(10**6) == (f32(0.999), f32(1 - 0.999))
    warm = FusedSGD(m, lr=0.1, ema_decay=0.999, ema_warmup=True)
    assert warm.ema_factors(1) == (f32(2 / 11), f32(1 - 2 / 11)) and warm.ema_factors(90) == (f32(0.91), f32(1 - 0.91))
    assert warm.ema_factors(10**6) == opt.ema_factors(1)


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. WarmupPolyLR
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('max_iters', [0, 1000])
@pytest.mark.parametrize('method', ['linear', 'constant'])
def test_warmup_poly_lr_closed_form(method, max_iters):
    """1200 steps, two groups with different base rates, against the formula written out here.  max_iters = 0 is what the reference
    driver gets: past the warm-up the factor (1 + T / warmup_iters)^0.9 rises.  With max_iters = 1000 the rate reaches target_lr at
    t = 1000 and stays there (beyond it 1 - T / N is negative and has no real 0.9-th power)."""
    target, power, wf, wi = 1e-4, 0.9, 1.0 / 3, 200
    a, b = (torch.nn.Parameter(torch.zeros(2)) for _ in range(2))
    base = (0.007, 0.0007)
    opt = torch.optim.SGD([{'params': [a], 'lr': base[0]}, {'params': [b], 'lr': base[1]}], lr=1.0)
    sched = WarmupPolyLR(opt, target_lr=target, max_iters=max_iters, power=power, warmup_factor=wf, warmup_iters=wi, warmup_method=method)
    for t in range(1201):
        if t < wi:
            f = wf if method == 'constant' else wf * (1 - t / wi) + t / wi
        else:
            x = 1 - (t - wi) / (max_iters - wi)
            f = x**power if x > 0 else 0.0
        for g, b0 in zip(opt.param_groups, base):
            assert g['lr'] == pytest.approx(target + (b0 - target) * f, rel=1e-12, abs=0), (t, g['lr'])
        assert sched.get_last_lr() == [g['lr'] for g in opt.param_groups]
        opt.step()
        sched.step()
    last = opt.param_groups[0]['lr']
    if max_iters == 0:
        assert last == pytest.approx(target + (base[0] - target) * (1 + 1001 / wi)**0.9, rel=1e-12) and last > 4 * base[0]  # (t = 1201)
    else:
        assert last == target
    with pytest.raises(ValueError):
        WarmupPolyLR(opt, warmup_method='cosine')


def test_warmup_poly_lr_defaults_are_the_reference_drivers():
    a = torch.nn.Parameter(torch.zeros(2))
    opt = torch.optim.SGD([a], lr=0.005)
    s = WarmupPolyLR(opt, warmup_iters=100)
    assert (s.target_lr, s.max_iters, s.power, s.warmup_factor, s.warmup_method) == (0, 0, 0.9, 1.0 / 3, 'linear')
    assert opt.param_groups[0]['lr'] == pytest.approx(0.005 / 3, rel=1e-12)
    assert 'max_iters' in WarmupPolyLR.__doc__ and 'RISES' in WarmupPolyLR.__doc__


# ------------------------------------------------------------------------------------------------------------------------------------
# 6. the C entry points
# ------------------------------------------------------------------------------------------------------------------------------------
GROUP_ARGS = 'pp' + 'i' + 'pp' + 'i'      # lr, weight_decay, ngroups, run_end, run_group, nruns
TAIL_ARGS = 'f' + 'p' + 'f' + 'pff' + 'p'  # grad_scale, sqnorm, max_norm, shadow, ema_decay, ema_one_minus, stream
ENTRIES = {'dbn_optim_max_groups': '',
           'dbn_optim_max_runs': '',
           'dbn_sgd_step': 'ppp' + 'l' + GROUP_ARGS + 'ff' + 'ii' + TAIL_ARGS,
           'dbn_adamw_step': 'ppppp' + 'l' + GROUP_ARGS + 'fff' + 'ii' + TAIL_ARGS}


def test_header_declares_the_entry_points():
    text = open(_lib.HEADER).read()
    for name, kinds in ENTRIES.items():
        assert len(re.findall(r'\b(?:int|long)\s+%s\s*\(' % name, text)) == 1, name
        assert _lib.SIGNATURES[name] == kinds, name
        assert name not in _lib.LONG_RETURN
    L = _lib.lib()
    assert L.dbn_sgd_step.restype is ctypes.c_int and L.dbn_adamw_step.restype is ctypes.c_int
    assert L.dbn_sgd_step.argtypes[3] is ctypes.c_long and L.dbn_adamw_step.argtypes[5] is ctypes.c_long
    assert (L.dbn_optim_max_groups(), L.dbn_optim_max_runs()) == (MAX_GROUPS, MAX_RUNS) == (8, 1024)
    # the four existing entry points are as they were
    assert _lib.SIGNATURES['dbn_adam_step'] == 'pppp' + 'l' + 'ffff' + 'i' + 'f' + 'p'
    assert _lib.SIGNATURES['dbn_adam_step_ex'] == 'ppppp' + 'l' + 'fffff' + 'i' + 'f' + 'p' + 'f' + 'p'


def test_entry_points_refuse_bad_group_arguments():
    """argument checks run before anything touches the device: more runs than the cap, no groups, more than 8, a missing table"""
    L = _lib.lib()
    one = (ctypes.c_float * 8)(*([0.1] * 8))
    fake = 4096  # (never dereferenced: every call below is refused first)
    sgd = lambda ng, ends, grps, nr: L.dbn_sgd_step(fake, fake, fake, 8, one, one, ng, ends, grps, nr, 0.9, 0.0, 0, 1, 1.0, None, 0.0, None, 0.0, 0.0, None)
    adamw = lambda ng, ends, grps, nr: L.dbn_adamw_step(fake, fake, fake, fake, None, 8, one, one, ng, ends, grps, nr, 0.9, 0.999, 1e-8, 1, 1, 1.0,
                                                       None, 0.0, None, 0.0, 0.0, None)
    for fn in (sgd, adamw):
        assert fn(2, fake, fake, MAX_RUNS + 1) == 1
        assert fn(0, None, None, 0) == 1 and fn(MAX_GROUPS + 1, fake, fake, 2) == 1
        assert fn(2, None, None, 0) == 1 and fn(2, None, fake, 2) == 1 and fn(2, fake, fake, -1) == 1
    assert L.dbn_sgd_step(fake, fake, None, 8, one, one, 1, None, None, 0, 0.9, 0.0, 0, 1, 1.0, None, 0.0, None, 0.0, 0.0, None) == 1  # momentum, no buffer
    assert L.dbn_sgd_step(fake, fake, fake, 8, one, one, 1, None, None, 0, 0.9, 0.5, 1, 1, 1.0, None, 0.0, None, 0.0, 0.0, None) == 1  # nesterov + dampening
    assert L.dbn_adamw_step(fake, fake, fake, fake, None, 8, one, one, 1, None, None, 0, 0.9, 0.999, 1e-8, 1, 0, 1.0, None, 0.0, None, 0.0, 0.0, None) == 1
