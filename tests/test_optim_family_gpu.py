"""-m gpu: the optimizer family of csrc/optim_groups.hip (dbn_sgd_step, dbn_adamw_step) and the classes over it.

  (a) exact, no tolerance: one-group coupled AdamW is dbn_adam_step_ex bit for bit; equal groups are one group; different groups equal, run
      by run, a one-group launch over that slice alone; the shadow changes nothing else; refused arguments write nothing
  (b) against float64 (tests/optim_family_ref.py, pinned against torch by tests/test_optim_family_cpu.py): SGD in every mode, decoupled
      AdamW, the EMA, two updates each
  (c) FusedSGD / FusedAdamW under DBTrainer on ResNet-18: the update against float64 on the engine's own gradient, checkpoints, fit()
      with WarmupPolyLR and ema_eval, the hipGraph step

Sizes: the scalar-tail cases and the three-chunk n of test_optim_ext_gpu.py, plus BIG = 4 (4096 x 256) + 4 x 1003 + 3, at which the
grid-stride loop runs twice (dbn_grid caps the grid at 4096 workgroups of 256 threads, one quad each).  Every buffer is 8 elements
longer than n and holds NaN there, which must survive; the norm's workspace and the run table's slack are poisoned.  The data
(F.family_data) comes from CPU generators, so that the CPU tests hold wrong rules against the very numbers used here.

The fp32 error model of (b) and (c), first order in U = 2^-24 as ex_bounds of test_optim_ext_gpu.py (F.sgd_bounds, F.adam_bounds,
F.ema_bound).  With ga = coef s acc, gd = wd p, g = ga + gd of the float64 restatement and E = (n + 8) 2^-53 for the float64 chain behind
the coefficient; the state the kernel held before the update is the restatement's input, so it carries no error:
  gs = fp32(coef s): 1 rounding; gs acc: 1; wd p: 1; the sum: 1           |dg| <= (2 U + E) |ga| + U |gd| + U |g|   (wd = 0: the first term only)
  buf' = g on the first update                                             |db| <= |dg|
  buf' = mu buf + (1 - damp) g afterwards: two products and a sum; 1 - damp is formed in float64 and rounded once, exactly for the
         values used here (0 and 1/4)                                      |db| <= (1 - damp) |dg| + 2 U (|mu buf| + |(1 - damp) g|)
  d = g + mu buf' (nesterov): a product and a sum, bounded as two products and a sum   |dd| <= |dg| + mu |db| + 2 U (|g| + |mu buf'|)
  d = buf' (momentum), g (none)                                            |dd| = |db|, |dg|
  p' = p - lr d: a product and a difference                                |dp| <= lr |dd| + U |lr d| + U |p'|
  AdamW, decoupled: pd = p pf with pf = fp32(1 - lr wd) formed in float64: the difference's rounding and the product's, 2 U |pd|, added
         to the bound of Adam's update on pd without decay (ex_bounds: m' 2, v' 1 and 2, the denominator 4, the update 3, the difference 1)
  shadow' = d shadow + (1 - d) p' with the two fp32 factors the restatement also uses: two products and a sum
                                                                           |ds| <= (1 - d) |dp| + 2 U (|d shadow| + |(1 - d) p'|)
"""
import ctypes

import pytest
import torch

import optim_family_ref as F
import optim_ref as R
from gpu_util import DEV, NAN, L, stream, within
from db_text_minimal_amd import DBLoss, DBTextModel, DBTrainer, FusedAdamW, FusedSGD, WarmupPolyLR, _lib, split_decay
from db_text_minimal_amd.optim import MAX_RUNS
from oracle import dbnet_oracle as O

pytestmark = pytest.mark.gpu

SQ_CHUNK = 16384
WRAP = 4096 * 256  # the quad at which the grid-stride loop starts its second round
BIG = 4 * WRAP + 4 * 1003 + 3
NS = [1, 3, 4, 5, 1023, 4 * 1003 + 3, 2 * SQ_CHUNK + 3, BIG]
f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
# eight groups' coefficients, all different (the floats the ABI receives); the first two are F.LRS / F.WDS
LR8 = F.LRS + [f32(0.1 / (i + 3)) for i in range(6)]
WD8 = F.WDS + [f32(0.05 * (i + 1)) for i in range(5)] + [0.0]
KINDS = {'sgd-plain': ('sgd', 'plain'), 'sgd-dampening': ('sgd', 'dampening'), 'sgd-nesterov': ('sgd', 'nesterov'),
         'adamw-decoupled-ams': ('adamw', True, True), 'adamw-coupled': ('adamw', False, False)}


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def mk(t):
    return torch.cat([t.to(DEV), nan(8, dtype=t.dtype)])


def bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int64)


def same_bits(tag, got, ref):
    ne = bits(got) != bits(ref)
    assert not bool(ne.any()), '%s: %d of %d elements differ in their bits; the first at %d' % (tag, int(ne.sum()), ne.numel(), int(ne.nonzero()[0]))


def guard_kept(tag, t, n):
    assert bool(torch.isnan(t[n:]).all()) and t.numel() == n + 8, tag + ': the guard beyond n was written'


def floats(xs):
    return (ctypes.c_float * len(xs))(*xs)


def device_runs(ends, groups):
    """the run table on the device, 8 poisoned entries of slack behind each array"""
    poison = [0x7f7f7f7f] * 8
    return (torch.tensor(list(ends) + poison, dtype=torch.int32, device=DEV), torch.tensor(list(groups) + poison, dtype=torch.int32, device=DEV),
            len(ends))


def norm_of(grad, n):
    """dbn_grad_sqnorm's device value (poisoned workspace) and the float64 norm with grad_scale applied"""
    nws = L().dbn_grad_sqnorm_ws_doubles(n)
    ws, sq = nan(nws + 8, dtype=torch.float64), nan(2, dtype=torch.float64)
    _lib.check(L().dbn_grad_sqnorm(grad.data_ptr(), n, ws.data_ptr(), sq.data_ptr(), stream()), 'sqnorm')
    return sq, float(R.grad_norm(grad[:n], F.GS))


def new_state(kind, n, seed):
    """the buffers of one optimizer: parameters (and the shadow, a copy of them) from F.family_data; the SGD buffer starts as NaN (the
    first update must not read it), Adam's moments as zeros.  Returns (state dict, the two gradients)."""
    p, grads = F.family_data(n, seed)
    st = {'p': mk(p), 'shadow': mk(p)}
    if KINDS[kind][0] == 'sgd':
        if KINDS[kind][1] != 'plain':
            st['buf'] = nan(n + 8)
    else:
        st['m'], st['v'] = mk(torch.zeros(n)), mk(torch.zeros(n))
        if KINDS[kind][2]:
            st['x'] = mk(torch.zeros(n))
    return st, [mk(g) for g in grads]


def launch(kind, st, grad, n, lrs, wds, runs, step, sq=None, c=0.0, ema=True, off=0, expect=0):
    """one update of `kind` on the n elements at offset `off` (floats) of the state's buffers; runs None: one group"""
    ptr = lambda t: None if t is None else t.data_ptr() + 4 * off
    table = (None, None, 0) if runs is None else (runs[0].data_ptr(), runs[1].data_ptr(), runs[2])
    groups = (floats(lrs), floats(wds), len(lrs)) + table
    tail = (F.GS, None if sq is None else sq.data_ptr(), c, ptr(st['shadow']) if ema else None, F.EMA_D, F.EMA_OMD, stream())
    if KINDS[kind][0] == 'sgd':
        mu, damp, nesterov = F.SGD_MODES[KINDS[kind][1]]
        rc = L().dbn_sgd_step(ptr(st['p']), ptr(grad), ptr(st.get('buf')), n, *groups, mu, damp, int(nesterov), int(step == 1), *tail)
    else:
        rc = L().dbn_adamw_step(ptr(st['p']), ptr(grad), ptr(st['m']), ptr(st['v']), ptr(st.get('x')), n, *groups, F.B1, F.B2, F.EPS,
                                int(KINDS[kind][1]), step, *tail)
    assert rc == expect, (kind, rc)


def clone_state(st):
    return {k: t.clone() for k, t in st.items()}


def same_state(tag, got, ref, n):
    for name in ref:
        same_bits('%s %s' % (tag, name), got[name], ref[name])
        if not bool(torch.isnan(ref[name][:n]).any()):
            assert bool(torch.isfinite(got[name][:n]).all()), '%s %s: non-finite values' % (tag, name)


# ------------------------------------------------------------------------------------------------------------------------------------
# (a) exact
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ams', [False, True])
@pytest.mark.parametrize('n', NS)
def test_adamw_one_group_is_adam_step_ex_bit_for_bit(n, ams):
    """dbn_adamw_step with one group, coupled decay and a NULL shadow against dbn_adam_step_ex with the same weight_decay, with and
    without clipping (coefficient 1/2), two updates; decoupled with weight_decay 0 against dbn_adam_step_ex with 0 as well"""
    kind = 'adamw-decoupled-ams' if ams else 'adamw-coupled'  # (the state's shape only: the decay mode is set per launch below)
    for clip in (False, True):
        for decoupled, wd in ((False, F.WDS[0]), (True, 0.0)):
            mine, grads = new_state(kind, n, n)
            theirs = clone_state(mine)
            for step, grad in enumerate(grads, 1):
                sq, c = None, 0.0
                if clip:
                    sq, norm = norm_of(grad, n)
                    c = f32(0.5 * norm)
                ptr = lambda t: None if t is None else t.data_ptr()
                rc = L().dbn_adamw_step(ptr(mine['p']), ptr(grad), ptr(mine['m']), ptr(mine['v']), ptr(mine.get('x')), n, floats([F.LRS[0]]),
                                        floats([wd]), 1, None, None, 0, F.B1, F.B2, F.EPS, int(decoupled), step, F.GS, ptr(sq), c, None, 0.0, 0.0,
                                        stream())
                assert rc == 0
                _lib.check(L().dbn_adam_step_ex(ptr(theirs['p']), ptr(grad), ptr(theirs['m']), ptr(theirs['v']), ptr(theirs.get('x')), n, F.LRS[0],
                                                F.B1, F.B2, F.EPS, wd, step, F.GS, ptr(sq), c, stream()), 'adam_ex')
                torch.cuda.synchronize()
                same_state('adamw n=%d ams=%d clip=%d decoupled=%d step %d' % (n, ams, clip, decoupled, step), mine, theirs, n)
            assert not torch.equal(mine['p'][:n], mine['shadow'][:n])  # the parameters moved, the unused shadow did not


@pytest.mark.parametrize('kind', list(KINDS))
@pytest.mark.parametrize('n', NS)
def test_equal_groups_are_one_group(n, kind):
    """two groups (F.two_runs) with the same (lr, wd): the bits of the launch without a table, shadow included, two clipped updates"""
    mine, grads = new_state(kind, n, n + 1)
    theirs = clone_state(mine)
    runs = device_runs(*F.two_runs(n))
    for step, grad in enumerate(grads, 1):
        sq, norm = norm_of(grad, n)
        c = f32(0.5 * norm)
        launch(kind, mine, grad, n, [F.LRS[0]] * 2, [F.WDS[0]] * 2, runs, step, sq, c)
        launch(kind, theirs, grad, n, [F.LRS[0]], [F.WDS[0]], None, step, sq, c)
        torch.cuda.synchronize()
        same_state('%s n=%d step %d' % (kind, n, step), mine, theirs, n)
        for name, t in mine.items():
            guard_kept('%s n=%d %s' % (kind, n, name), t, n)


def even_cuts(n4, count):
    return [n4 * (i + 1) // count for i in range(count)]


def run_tables(n):
    """name -> run_end for n elements: one run; single-quad runs at the start, at the end and on either side of a workgroup's first quad
    (256 k); a boundary where the grid-stride loop wraps, with single-quad runs around it; 2, 3, 65 and the maximum number of runs"""
    n4 = n // 4
    assert n4 > 600
    tables = {'one run': [n4], 'single quads': [1, 255, 256, 257, 511, 512, n4 - 1, n4], '2 runs': even_cuts(n4, 2), '3 runs': even_cuts(n4, 3),
              '65 runs': even_cuts(n4, 65)}
    if n4 >= 4 * MAX_RUNS:
        tables['%d runs' % MAX_RUNS] = even_cuts(n4, MAX_RUNS)
    if n4 > WRAP + 1:
        tables['wrap'] = [WRAP, n4]
        tables['single quads at the wrap'] = [WRAP - 1, WRAP, WRAP + 1, n4]
    return tables


# (a size has the tables it can hold: the maximum number of runs from 4096 quads on, the wrap at BIG only)
GROUPED_CASES = [(n, name) for n in (4 * 1003 + 3, 2 * SQ_CHUNK + 3, BIG) for name in run_tables(n)]
assert {name for _, name in GROUPED_CASES} >= {'%d runs' % MAX_RUNS, 'wrap', 'single quads at the wrap'}


@pytest.mark.parametrize('kind', list(KINDS))
@pytest.mark.parametrize('n,name', GROUPED_CASES)
def test_groups_equal_one_group_launches_over_their_slices(n, name, kind):
    """Eight groups with different (lr, wd), run r in group (3 r + 1) mod 8 (neighbours always differ).  The kernel is elementwise, so every
    run's elements must equal, bit for bit, a one-group launch over that slice alone with that group's coefficients and the same device
    value of the squared norm (coefficient 1/2); the last run's slice extends over the elements past the last whole quad.  Two updates,
    the EMA on."""
    ends = run_tables(n)[name]
    groups = [(3 * r + 1) % 8 for r in range(len(ends))]
    runs = device_runs(ends, groups)
    mine, grads = new_state(kind, n, n + 2)
    theirs = clone_state(mine)
    for step, grad in enumerate(grads, 1):
        sq, norm = norm_of(grad, n)
        c = f32(0.5 * norm)
        launch(kind, mine, grad, n, LR8, WD8, runs, step, sq, c)
        lo = 0
        for r, (end, g) in enumerate(zip(ends, groups)):
            hi = n if r == len(ends) - 1 else 4 * end
            launch(kind, theirs, grad, hi - 4 * lo, [LR8[g]], [WD8[g]], None, step, sq, c, off=4 * lo)
            lo = end
        torch.cuda.synchronize()
        same_state('%s n=%d %s step %d' % (kind, n, name, step), mine, theirs, n)
    for t in mine.values():
        guard_kept('%s n=%d %s' % (kind, n, name), t, n)
    assert bool((bits(runs[0][-8:]) == 0x7f7f7f7f).all()) and bool((bits(runs[1][-8:]) == 0x7f7f7f7f).all())


@pytest.mark.parametrize('kind', ['sgd-dampening', 'adamw-decoupled-ams'])
def test_one_run_more_than_the_maximum_is_refused_and_writes_nothing(kind):
    n = 2 * SQ_CHUNK + 3
    ends = even_cuts(n // 4, MAX_RUNS + 1)
    runs = device_runs(ends, [r % 8 for r in range(len(ends))])
    st, grads = new_state(kind, n, 5)
    before = clone_state(st)
    launch(kind, st, grads[0], n, LR8, WD8, runs, 1, expect=1)  # DBN_ERR_ARG
    torch.cuda.synchronize()
    same_state(kind, st, before, n)


@pytest.mark.parametrize('kind', list(KINDS))
@pytest.mark.parametrize('n', [5, 4 * 1003 + 3])
def test_shadow_changes_nothing_else(n, kind):
    """With a NULL shadow the shadow's buffer keeps its bits; with it, the parameters and the state equal the launch without it"""
    runs = device_runs(*F.two_runs(n))
    with_ema, grads = new_state(kind, n, n + 3)
    without = clone_state(with_ema)
    for step, grad in enumerate(grads, 1):
        untouched = without['shadow'].clone()
        launch(kind, with_ema, grad, n, F.LRS, F.WDS, runs, step)
        launch(kind, without, grad, n, F.LRS, F.WDS, runs, step, ema=False)
        torch.cuda.synchronize()
        same_bits('%s n=%d: the shadow of a launch that was given none' % (kind, n), without['shadow'], untouched)
        for name in with_ema:
            if name != 'shadow':
                same_bits('%s n=%d step %d %s' % (kind, n, step, name), with_ema[name], without[name])
    assert not torch.equal(with_ema['shadow'][:n], without['shadow'][:n])


# ------------------------------------------------------------------------------------------------------------------------------------
# (b) against float64
# ------------------------------------------------------------------------------------------------------------------------------------
def group_vectors(n, ends, groups, lrs=F.LRS, wds=F.WDS):
    return F.per_element(lrs, ends, groups, n, device=DEV), F.per_element(wds, ends, groups, n, device=DEV)


@pytest.mark.parametrize('clip', ['clipped', 'unclipped'])
@pytest.mark.parametrize('decay', [False, True])
@pytest.mark.parametrize('mode', list(F.SGD_MODES))
@pytest.mark.parametrize('n', NS)
def test_sgd_vs_fp64(n, mode, decay, clip):
    """dbn_sgd_step with two groups, grad_scale 1/4, a max-norm of half (coefficient 1/2) or twice (1) the update's own norm taken from
    dbn_grad_sqnorm's device value, and the EMA: two updates (the first sets the buffer, the second uses it), each against F.sgd_step and
    F.ema_step in float64 on the state the kernel held before; bounds: the module docstring"""
    kind = 'sgd-' + ('dampening' if mode in ('momentum', 'dampening') else mode)
    mu, damp, nesterov = F.SGD_MODES[mode]
    ends, groups = F.two_runs(n)
    runs = device_runs(ends, groups)
    wds = F.WDS if decay else [0.0, 0.0]
    lr, wd = group_vectors(n, ends, groups, wds=wds)
    st, grads = new_state(kind, n, n)
    for step, grad in enumerate(grads, 1):
        before = {k: t[:n].double() for k, t in st.items()}
        sq, norm = norm_of(grad, n)
        c = f32(norm * (0.5 if clip == 'clipped' else 2.0))
        ptr = lambda t: None if t is None else t.data_ptr()
        rc = L().dbn_sgd_step(ptr(st['p']), ptr(grad), ptr(st.get('buf')), n, floats(F.LRS), floats(wds), 2, runs[0].data_ptr(), runs[1].data_ptr(),
                              runs[2], mu, damp, int(nesterov), int(step == 1), F.GS, ptr(sq), c, ptr(st['shadow']), F.EMA_D, F.EMA_OMD, stream())
        assert rc == 0
        torch.cuda.synchronize()
        p1, buf1, parts = F.sgd_step(before['p'], grad[:n], before.get('buf'), lr, wd, mu, damp, nesterov, step == 1, grad_scale=F.GS, max_norm=c)
        assert bool(parts['coef'] < 1) == (clip == 'clipped'), float(parts['coef'])
        bbuf, bp = F.sgd_bounds(parts, p1, n, decay)
        tag = 'sgd %s decay=%d %s n=%d step %d ' % (mode, decay, clip, n, step)
        within(tag + 'param', st['p'][:n], p1, bp)
        if mu:
            within(tag + 'momentum_buffer', st['buf'][:n], buf1, bbuf)
        s1, terms = F.ema_step(before['shadow'], p1, F.EMA_D, F.EMA_OMD)
        within(tag + 'shadow', st['shadow'][:n], s1, F.ema_bound(terms, bp, F.EMA_OMD))
        for name, t in st.items():
            guard_kept(tag + name, t, n)


@pytest.mark.parametrize('clip', ['clipped', 'unclipped'])
@pytest.mark.parametrize('ams', [False, True])
@pytest.mark.parametrize('n', NS)
def test_adamw_decoupled_vs_fp64(n, ams, clip):
    """dbn_adamw_step, decoupled, two groups, the EMA, as test_sgd_vs_fp64: two updates against F.adamw_step in float64"""
    kind = 'adamw-decoupled-ams' if ams else 'adamw-coupled'  # (the state's shape; decoupled is passed below)
    ends, groups = F.two_runs(n)
    runs = device_runs(ends, groups)
    lr, wd = group_vectors(n, ends, groups)
    st, grads = new_state(kind, n, n)
    for step, grad in enumerate(grads, 1):
        before = {k: t[:n].double() for k, t in st.items()}
        sq, norm = norm_of(grad, n)
        c = f32(norm * (0.5 if clip == 'clipped' else 2.0))
        ptr = lambda t: None if t is None else t.data_ptr()
        rc = L().dbn_adamw_step(ptr(st['p']), ptr(grad), ptr(st['m']), ptr(st['v']), ptr(st.get('x')), n, floats(F.LRS), floats(F.WDS), 2,
                                runs[0].data_ptr(), runs[1].data_ptr(), runs[2], F.B1, F.B2, F.EPS, 1, step, F.GS, ptr(sq), c, ptr(st['shadow']),
                                F.EMA_D, F.EMA_OMD, stream())
        assert rc == 0
        torch.cuda.synchronize()
        p1, m1, v1, x1, parts = F.adamw_step(before['p'], grad[:n], before['m'], before['v'], before.get('x'), lr, F.B1, F.B2, F.EPS, wd, step, True,
                                             grad_scale=F.GS, max_norm=c)
        assert bool(parts['coef'] < 1) == (clip == 'clipped'), float(parts['coef'])
        bm, bv, bp = F.adam_bounds(parts, p1, v1, F.B1, F.B2, n, decay=False, decoupled=True)
        tag = 'adamw ams=%d %s n=%d step %d ' % (ams, clip, n, step)
        within(tag + 'exp_avg', st['m'][:n], m1, bm)
        within(tag + 'exp_avg_sq', st['v'][:n], v1, bv)
        if ams:
            within(tag + 'max_exp_avg_sq', st['x'][:n], x1, bv)
        within(tag + 'param', st['p'][:n], p1, bp)
        s1, terms = F.ema_step(before['shadow'], p1, F.EMA_D, F.EMA_OMD)
        within(tag + 'shadow', st['shadow'][:n], s1, F.ema_bound(terms, bp, F.EMA_OMD))
        for name, t in st.items():
            guard_kept(tag + name, t, n)


# ------------------------------------------------------------------------------------------------------------------------------------
# (c) the classes
# ------------------------------------------------------------------------------------------------------------------------------------
def make_model(seed):
    m = DBTextModel()
    m.load_state_dict(O.new_state(seed))
    return m.to(DEV).train()


def batches(seed, count, n=2, size=64):
    return [tuple(t.to(DEV) for t in O.synthetic_batch(n, size, seed=seed + i)) for i in range(count)]


def halves(model, **second):
    """two groups over the live parameters: the first half with the constructor's values, the second with `second`"""
    live = [p for _, p in model.engine.live_params]
    return [{'params': live[:len(live) // 2]}, dict(second, params=live[len(live) // 2:])]


CONFIGS = {
    'sgd-split-decay-clip': lambda m: FusedSGD(m, lr=0.02, momentum=0.9, weight_decay=1e-4, param_groups=split_decay(m, 1e-4), max_grad_norm=1.0),
    'adamw-two-groups-ema': lambda m: FusedAdamW(m, lr=0.005, weight_decay=0.01, param_groups=halves(m, lr=0.001, weight_decay=0.1),
                                                 ema_decay=0.9),
    'sgd-nesterov-accumulate-ema': lambda m: FusedSGD(m, lr=0.02, momentum=0.9, nesterov=True, weight_decay=1e-4,
                                                      param_groups=halves(m, lr=0.01, weight_decay=0.0), max_grad_norm=0.5,
                                                      accumulation_steps=2, ema_decay=0.9, ema_warmup=True)}


def opt_state(opt):
    names = list(opt._state_names()) + (['ema'] if opt.ema_decay is not None else [])
    return {name: getattr(opt, name) for name in names}


@pytest.mark.parametrize('config', list(CONFIGS))
def test_trainer_updates_against_fp64(config):
    """ResNet-18 at 2 x 3 x 64 x 64: DBTrainer.step three times (four with accumulation_steps = 2: two updates).  Around every update the
    parameters, the state and the shadow are held before it; the gradient the update consumed is the engine's flat gradient (or the
    accumulator) as it stands afterwards — the update does not write it.  The float64 restatement, fed that gradient and the group
    vectors built from the optimizer's own run table, bounds parameters, state and shadow as in (b): the optimizer is isolated from the
    model's tolerances."""
    seed = 9
    model = make_model(seed)
    opt = CONFIGS[config](model)
    trainer = DBTrainer(model, DBLoss(), opt, distributed=False)
    k = opt.accumulation_steps
    mbs = batches(seed, 4)
    eng = model.engine
    updates = 0
    for call in range(3 if k == 1 else 4):
        opt._ensure_state()
        torch.cuda.synchronize()
        before = {name: t.double() for name, t in opt_state(opt).items()}
        before['p'] = eng.flat.double()
        trainer.step(*mbs[call])
        torch.cuda.synchronize()
        if not trainer.updated:
            assert k == 2 and call % 2 == 0 and torch.equal(eng.flat.double(), before['p'])
            continue
        updates += 1
        assert opt.step_count == updates
        n = eng.flat.numel()
        grad = opt.grad_acc if k > 1 else eng.flat_grad
        table, nruns = opt._runs
        ends, groups = table[0].tolist(), table[1].tolist()
        assert nruns == len(ends) > 1 and ends[-1] == n // 4
        lrs, wds = ([f32(g[key]) for g in opt.param_groups] for key in ('lr', 'weight_decay'))
        lr, wd = F.per_element(lrs, ends, groups, n, device=DEV), F.per_element(wds, ends, groups, n, device=DEV)
        c = opt.max_grad_norm
        scale = 1.0 / k
        g0 = opt.param_groups[0]
        tag = '%s update %d ' % (config, updates)
        if isinstance(opt, FusedSGD):
            mu, damp = f32(g0['momentum']), f32(g0['dampening'])
            p1, buf1, parts = F.sgd_step(before['p'], grad, before.get('momentum_buffer'), lr, wd, mu, damp, g0['nesterov'], updates == 1,
                                         grad_scale=scale, max_norm=c)
            bbuf, bp = F.sgd_bounds(parts, p1, n, decay=True)
            within(tag + 'momentum_buffer', opt.momentum_buffer, buf1, bbuf)
        else:
            b1, b2, eps = f32(g0['betas'][0]), f32(g0['betas'][1]), f32(g0['eps'])
            p1, m1, v1, _, parts = F.adamw_step(before['p'], grad, before['exp_avg'], before['exp_avg_sq'], None, lr, b1, b2, eps, wd, updates, True,
                                                grad_scale=scale, max_norm=c)
            bm, bv, bp = F.adam_bounds(parts, p1, v1, b1, b2, n, decay=False, decoupled=True)
            within(tag + 'exp_avg', opt.exp_avg, m1, bm)
            within(tag + 'exp_avg_sq', opt.exp_avg_sq, v1, bv)
        within(tag + 'param', eng.flat, p1, bp)
        print(tag + 'clip coefficient %.4f' % float(parts['coef']))
        if c is not None:
            norm = float(parts['norm'])
            assert abs(float(opt.last_grad_norm) - norm) <= (n + 4) * 2.0**-53 * norm
        if opt.ema_decay is not None:
            d, omd = opt.ema_factors(updates)
            if opt.ema_warmup:
                assert d == f32((1 + updates) / (10 + updates)) < f32(opt.ema_decay)
            s1, terms = F.ema_step(before['ema'], p1, d, omd)
            within(tag + 'shadow', opt.ema, s1, F.ema_bound(terms, bp, omd))
            if updates == 1:
                same_bits(tag + 'the shadow started as the parameters', before['ema'].float(), before['p'].float())
    assert updates == (3 if k == 1 else 2)


def test_refusals_are_fused_adams():
    """a wrong fold count and a second backward pass are refused with FusedAdam's messages under the class's own name, and change nothing"""
    seed = 3
    (img, gts), = batches(seed, 1, n=1)
    crit = DBLoss()
    model = make_model(seed)
    opt = FusedSGD(model, lr=0.02, momentum=0.9, param_groups=split_decay(model, 1e-4), accumulation_steps=2, ema_decay=0.9)
    crit(model(img), gts)[4].backward()
    opt.accumulate()
    torch.cuda.synchronize()
    before = model.engine.flat.clone()
    with pytest.raises(RuntimeError, match=r'FusedSGD\.step\(\): 1 of accumulation_steps=2'):
        opt.step()
    crit(model(img), gts)[4].backward()
    with pytest.raises(RuntimeError, match='1 of accumulation_steps=2.*1 ran without'):
        opt.step()
    torch.cuda.synchronize()
    assert torch.equal(model.engine.flat, before) and torch.equal(opt.ema, before) and opt.step_count == 0 and opt.folded == 1
    opt.accumulate()
    opt.step(grad_scale=0.5)
    torch.cuda.synchronize()
    assert not torch.equal(model.engine.flat, before) and opt.step_count == 1 and opt.folded == 0
    with pytest.raises(RuntimeError, match=r'FusedSGD\.accumulate\(\): 0 backward passes'):
        opt.accumulate()
    with pytest.raises(NotImplementedError, match='closures'):
        opt.step(closure=lambda: None)
    model1 = make_model(seed)
    opt1 = FusedAdamW(model1)
    for _ in range(2):
        crit(model1(img), gts)[4].backward()
    with pytest.raises(RuntimeError, match=r'FusedAdamW\.step\(\): 2 backward passes ran since the last zero_grad\(\)/step\(\); the flat gradient '
                       r'buffer holds only the last one \(no gradient accumulation on the fused path — use torch.optim.AdamW over'):
        opt1.step()
    opt2 = FusedSGD(model1, lr=0.1)
    with pytest.raises(RuntimeError, match='use torch.optim.SGD over'):
        opt2.step()


def test_ema_weights_twice_restores_both_buffers():
    """inside the block the model holds the shadow's bits and evaluates with them; afterwards both buffers are back, bit for bit"""
    seed = 4
    model = make_model(seed)
    opt = CONFIGS['adamw-two-groups-ema'](model)
    trainer = DBTrainer(model, DBLoss(), opt, distributed=False)
    (img, gts), = batches(seed, 1)
    for _ in range(2):
        trainer.step(img, gts)
    torch.cuda.synchronize()
    eng = model.engine
    flat0, ema0 = eng.flat.clone(), opt.ema.clone()
    assert not torch.equal(flat0, ema0)
    model.eval()
    with torch.no_grad():
        own = model(img).clone()
        with opt.ema_weights():
            same_bits('inside: parameters', eng.flat, ema0)
            same_bits('inside: shadow', opt.ema, flat0)
            name, p = eng.live_params[0]
            same_bits('inside: the model\'s tensors are views of the flat buffer', p.detach().reshape(-1), ema0[:p.numel()])
            averaged = model(img).clone()
        again = model(img).clone()
    torch.cuda.synchronize()
    same_bits('after: parameters', eng.flat, flat0)
    same_bits('after: shadow', opt.ema, ema0)
    same_bits('after: the model evaluates with its own weights again', again.reshape(-1), own.reshape(-1))
    assert not torch.equal(averaged, own), 'the forward pass inside the block did not see the averaged weights'
    sd = opt.ema_state_dict()
    msd = model.state_dict()
    assert set(sd) == set(msd)
    live = dict(eng.live_params)
    for (pname, p), off in zip(eng.live_params, eng.offsets):
        same_bits('ema_state_dict ' + pname, sd[pname].reshape(-1), ema0[off:off + p.numel()])
    for key in msd:
        if key not in live:
            assert torch.equal(sd[key], msd[key]), key  # BatchNorm buffers: the model's


@pytest.mark.parametrize('config', ['adamw-two-groups-ema', 'sgd-nesterov-accumulate-ema'])
def test_state_dict_round_trip_continues_bit_for_bit(config):
    seed = 5
    mbs = batches(seed, 3)
    A = make_model(seed)
    optA = CONFIGS[config](A)
    trA = DBTrainer(A, DBLoss(), optA, distributed=False)
    k = optA.accumulation_steps
    for i in range(2 * k):
        trA.step(*mbs[i % 3])
    sd = optA.state_dict()
    assert sd['step'] == 2 and len(sd['param_groups']) == 2 and all('params' not in g for g in sd['param_groups']) and 'grad_acc' not in sd
    assert sd['ema'] is optA.ema and sd['param_groups'][1]['lr'] == optA.param_groups[1]['lr']
    B = make_model(seed + 1)  # other weights, overwritten by the checkpoint
    B.load_state_dict(A.state_dict())
    same_bits('the model checkpoint', *(torch.cat([p.detach().reshape(-1) for _, p in m.engine.live_params]) for m in (B, A)))
    optB = CONFIGS[config](B)
    optB.param_groups[0]['lr'] = 123.0  # overwritten by the checkpoint too
    optB.load_state_dict(sd)
    assert optB.step_count == 2 and optB.param_groups[0]['lr'] == optA.param_groups[0]['lr']
    trB = DBTrainer(B, DBLoss(), optB, distributed=False)
    for i in range(k):
        trA.step(*mbs[i])
        trB.step(*mbs[i])
    torch.cuda.synchronize()
    assert optA.step_count == optB.step_count == 3
    same_bits('param', B.engine.flat, A.engine.flat)
    for name, t in opt_state(optA).items():
        assert getattr(optB, name) is not t
        same_bits(name, getattr(optB, name), t)


def test_fit_with_warmup_poly_and_ema_eval_writes_the_averaged_weights(tmp_path):
    """fit() over a two-batch loader, two epochs, WarmupPolyLR stepped per update, ema_eval: the test pass runs inside ema_weights() and
    both checkpoints hold the shadow's bits for the parameters and the model's BatchNorm buffers; training went on with the model's own
    weights (they differ from the shadow), and the rate followed the schedule in both groups"""
    from db_text_minimal_amd.train import fit
    seed = 3
    loader = []
    for i in range(2):
        img, gts = O.synthetic_batch(2, 64, seed=seed + i)
        loader.append({'img': img, 'prob_map': gts[0], 'supervision_mask': gts[1], 'thresh_map': gts[2], 'text_area_map': gts[3]})
    model = make_model(seed)
    opt = FusedSGD(model, lr=0.02, momentum=0.9, param_groups=split_decay(model, 1e-4), ema_decay=0.9)
    sched = WarmupPolyLR(opt, warmup_iters=2, max_iters=10)
    best, last = str(tmp_path / 'best.pt'), str(tmp_path / 'last.pt')
    hist = fit(model, DBLoss(), opt, loader, loader, epochs=2, scheduler=sched, lrs_mode='poly', device=DEV, pixel_metric=False,
               best_cp_path=best, last_cp_path=last, ema_eval=True)
    torch.cuda.synchronize()
    assert [h['global_steps'] for h in hist] == [2, 4] and opt.step_count == 4 and sched.last_epoch == 4 and hist[0].get('saved_best')
    for g in opt.param_groups:
        assert g['lr'] == pytest.approx(0.02 * (1 - 2 / 8)**0.9, rel=1e-12)
    eng = model.engine
    assert not torch.equal(eng.flat, opt.ema)
    ck = torch.load(last)
    msd = model.state_dict()
    assert set(ck) == set(msd)
    live = dict(eng.live_params)
    for (name, p), off in zip(eng.live_params, eng.offsets):
        same_bits('checkpoint ' + name, ck[name].to(DEV).reshape(-1), opt.ema[off:off + p.numel()])
        same_bits('model ' + name, msd[name].reshape(-1), eng.flat[off:off + p.numel()])
    for key in msd:
        if key not in live:
            assert torch.equal(ck[key].to(DEV), msd[key]), key
    assert set(torch.load(best)) == set(msd)
    # without ema_eval nothing changes: the checkpoint holds the model's own weights
    fit(model, DBLoss(), opt, loader[:1], None, epochs=1, device=DEV, pixel_metric=False, last_cp_path=last)
    torch.cuda.synchronize()
    ck = torch.load(last)
    name, p = eng.live_params[0]
    same_bits('default checkpoint ' + name, ck[name].to(DEV).reshape(-1), eng.flat[:p.numel()])


def test_graph_step_with_fused_sgd_is_bit_identical_to_eager():
    """use_graph (DBN_STEP_GRAPH=1) with FusedSGD: forward + loss + backward replay from the captured graph, the norm and the update stay
    outside it.  Five calls over changing batches — two eager warm-up calls, the capturing call, two replays — leave parameters, momentum
    buffer, shadow and norm bit-equal to five eager calls."""
    seed = 9
    mbs = batches(seed, 3, n=1)

    def run(use_graph):
        model = make_model(seed)
        opt = FusedSGD(model, lr=0.02, momentum=0.9, nesterov=True, param_groups=split_decay(model, 1e-4), max_grad_norm=0.5, ema_decay=0.9)
        trainer = DBTrainer(model, DBLoss(), opt, distributed=False)
        trainer.use_graph = use_graph
        for it in range(5):
            trainer.step(*mbs[it % 3])
            assert trainer.updated
        torch.cuda.synchronize()
        assert opt.step_count == 5 and (trainer._graph is not None and trainer._graph['graph'] is not None) == use_graph
        return [t.clone() for t in (model.engine.flat, opt.momentum_buffer, opt.ema, opt.last_grad_norm)]

    eager, graph = run(False), run(True)
    for name, a, b in zip(('param', 'momentum_buffer', 'shadow', 'last_grad_norm'), eager, graph):
        same_bits('graph vs eager: ' + name, b.reshape(-1), a.reshape(-1))
