"""-m gpu: the DB loss kernels of csrc/head_loss.hip (db_loss_fwd_kernel<1|4>, db_loss_bwd_kernel<1|4>, the ohem_* radix select and its
finalize) pinned against the float64 reference of tests/loss_ref.py — through the C ABI on NaN-filled outputs and NaN-poisoned
workspaces, and through DBLoss with autograd.

Bounds (loss_ref.loss_bounds carries the derivation line by line): a thread of db_loss_fwd_kernel adds depth = min(trips, 64) V terms
in fp32 before its sums become doubles, and a term carries c roundings of its own (loss_ref.C_TERM, counted from the kernel; the native
logarithm and reciprocal at the 1 ulp AMD's ISA documentation states, so the BCE term at C_LOG = 10 u), so every sum S_k sits within
(gamma(depth + c_k) + 2^-40) S_k of float64 — all terms are >= 0.  db_loss_finish and ohem_finalize_kernel then cost one u per fp32
operation, propagated to first order into absolute bounds of the five losses and of coef[0..3]; the backward's coefficient carries that
error plus its own operations, and dpreds is held elementwise to (that + c' u) |ref| — which is exactly 0 wherever the reference is
exactly 0: masked L1, T == thresh_gt, M = 0 for the dice term, unselected negatives, P equal to its target.
The counts (n_pos, n_neg, non-binary pixels) are integers and must be exact.  reduction='none': the kernel orders fp32 values, the
reference float64 ones; negatives whose float64 value lies within 2 gamma(C_PX) of the k-th value (loss_ref.select_band: exact ties and
near neighbours) may be taken or left, so inside that band the test asks for weights in [0, 1] that add up to the number of places left
in the top k, equal weights on exact ties, and the reference's sum of dP over a tie class; outside the band everything is elementwise.

Outcome of the cases the code had never met: see the docstrings of test_subnormal_predictions and test_flush_of_the_running_sums.
"""
import numpy as np
import pytest
import torch

import loss_ref as R
from gpu_util import DEV, L, NAN, exact, stream, within
from db_text_minimal_amd import DBLoss, _lib

pytestmark = pytest.mark.gpu

MODES = ['mean', 'sum', 'none', 'literal_mean', 'literal_sum']
PARAMS = {3: (0.75, 3.5), 2: (1.0, 10.0)}  # alpha, beta (exact in fp32): other than the defaults for 3 channels, the defaults for 2


def t64(x):
    return torch.tensor(x, dtype=torch.float64)


def reduction_of(mode):
    return mode.split('_')[-1]


def gout_of(seed):
    return torch.randn(5, generator=torch.Generator().manual_seed(seed)).float()


def run_abi(preds, gts, mode, gout, alpha, beta, ratio, eps=1e-6):
    """Forward and backward through the C ABI.  Returns losses[5], coef[8], dpreds, the eight folded sums of the partial rows
    ([workgroups][8] doubles at the start of the workspace) and, for the select paths, k from the select state (head_loss.hip: the state
    words follow the 1024 + 2048 partial doubles behind dbn_db_loss_ws_bytes())."""
    N, CH, H, W = preds.shape
    select = mode == 'none' or mode.startswith('literal')
    nbytes = L().dbn_db_loss_ohem_ws_bytes(N, H, W) if select else L().dbn_db_loss_ws_bytes()
    ws = torch.empty(nbytes // 4 + 2, dtype=torch.int32, device=DEV).fill_(-1)  # every word a NaN
    losses = torch.full((5, ), NAN, device=DEV)
    coef = torch.full((8, ), NAN, device=DEV)
    dpreds = torch.full_like(preds, NAN)
    head = (preds.data_ptr(), gts.data_ptr(), N, H, W, CH, alpha, beta, float(ratio), eps)
    tail = (losses.data_ptr(), coef.data_ptr(), ws.data_ptr(), stream())
    if mode.startswith('literal'):
        _lib.check(L().dbn_db_loss_frac_fwd(*head, 1 if mode.endswith('sum') else 0, *tail), mode)
    else:
        fwd = {'mean': L().dbn_db_loss_fwd, 'sum': L().dbn_db_loss_sum_fwd, 'none': L().dbn_db_loss_ohem_fwd}[mode]
        _lib.check(fwd(*head, *tail), mode)
    g = gout.to(DEV)
    if mode == 'none':
        _lib.check(L().dbn_db_loss_ohem_bwd(preds.data_ptr(), gts.data_ptr(), coef.data_ptr(), g.data_ptr(), ws.data_ptr(), alpha, beta, N, H, W,
                                            CH, dpreds.data_ptr(), stream()), 'ohem_bwd')
    else:
        _lib.check(L().dbn_db_loss_bwd(preds.data_ptr(), gts.data_ptr(), coef.data_ptr(), g.data_ptr(), alpha, beta, N, H, W, CH,
                                       dpreds.data_ptr(), stream()), 'bwd')
    torch.cuda.synchronize()
    nb = R.fwd_geometry(N, H, W)['nb']
    sums = ws[:nb * 16].view(torch.float64).view(nb, 8).sum(0)
    k = None
    if select:
        off = L().dbn_db_loss_ws_bytes() + 1024 * 8 + 2048 * 8
        k = int(ws[off // 4:off // 4 + 2].view(torch.int64)[0])
    return losses, coef, dpreds, sums, k


def run_module(preds, gts, mode, gout, alpha, beta, ratio, eps=1e-6):
    """The same through DBLoss and autograd; 2-channel preds return the one value losses[4]."""
    crit = DBLoss(alpha=alpha, beta=beta, reduction=reduction_of(mode), negative_ratio=ratio, eps=eps, fractional_maps=mode.startswith('literal'))
    p = preds.clone().requires_grad_(True)
    res = crit(p, gts)
    if preds.shape[1] == 3:
        sum(float(g) * r for g, r in zip(gout, res)).backward()
        losses = torch.stack([r.detach() for r in res])
    else:
        (float(gout[4]) * res).backward()
        losses = res.detach().reshape(1)
    return losses, p.grad


def check_select_gradient(tag, dP, dref, ref, gts, preds, gout, bnd, sel, tie):
    """dP of reduction='none' (see the module docstring)."""
    G, M = gts[0].double(), gts[1].double()
    neg = (1.0 - G) * M > 0
    band = R.select_band(ref, gts)
    ref_P = dref[:, 0]
    outside = ~band
    within(tag + ' dP outside the band', dP[outside], ref_P[outside], bnd['r_dP'] * ref_P[outside].abs())
    P = preds[:, 0].double()
    w_prob = R.weights(gout, ref['CH'], ref['alpha'], ref['beta'])[0]
    dbce = (w_prob / ref['denom']) * (P - G) / ((1.0 - P) * P).clamp_min(R.EPS12)
    full, base = (1.0 - G) * M * dbce, G * M * dbce  # a pixel's gradient as a negative at weight 1, and as a positive (fractional prob_gt)
    n_band = int(band.sum())
    if n_band == 1:  # no ties at the k-th value: exactly n_neg negatives carry a gradient (those whose gradient is not 0 by itself)
        pure = neg & (base == 0)
        assert int(((dP != 0) & pure).sum()) == int(((sel > 0) & pure & (full != 0)).sum()), tag
    if n_band == 0:
        return
    fb, gb = full[band], dP[band].double() - base[band]
    flat = fb == 0
    assert bool((gb[flat] == 0).all()), tag
    wgt = gb[~flat] / fb[~flat]
    tol = (16 * R.U + 2 * bnd['r_dP']) * (1.0 + (base[band][~flat] / fb[~flat]).abs())  # (a weight is the quotient of two gradients)
    print('%s: %d negatives in the band of the k-th value, weights %.6f .. %.6f' % (tag, n_band, float(wgt.min()) if wgt.numel() else 0,
                                                                                 float(wgt.max()) if wgt.numel() else 0))
    assert bool(((wgt >= -tol) & (wgt <= 1 + tol)).all()), tag
    tol = float(tol.max()) if tol.numel() else 0.0
    if not bool(flat.any()):
        left = ref['n_neg'] - int(((sel > 0) & outside).sum())
        within(tag + ' weights inside the band add up to the places left', wgt.sum().reshape(1), t64([float(left)]), n_band * tol)
    if bool((band == tie).all()) and n_band > 1:  # an exact tie class: equal weights, and the reference's sum of dP over the class
        if wgt.numel():
            assert float(wgt.max() - wgt.min()) <= tol, tag
        within(tag + ' sum of dP over the tie class', dP[tie].double().sum().reshape(1), ref_P[tie].sum().reshape(1),
               bnd['r_dP'] * ref_P[tie].abs().sum() + n_band * tol * float(fb.abs().max()))


def check(tag, preds, gts, mode, seed=0, ratio=3, dyadic=False, c_log=R.C_LOG, module=True, underflow=False):
    """One case in one mode, through the C ABI and (module) through DBLoss."""
    N, CH, H, W = preds.shape
    alpha, beta = PARAMS[CH]
    gout = gout_of(seed)
    pd, gd = preds.to(DEV), gts.to(DEV)
    ref = R.db_loss_ref(pd, gd, alpha, beta, reduction_of(mode), ratio, 1e-6)
    literal = mode.startswith('literal')
    if not literal and mode != 'none' and ref['nonbin']:
        raise AssertionError('the closed form is exact for binary maps only: use the literal form')
    bnd = R.loss_bounds(ref, N, H, W, gout, literal=literal, c_log=c_log)
    dref, sel, tie = R.db_loss_grad_ref(pd, gd, gout, ref)
    dbound = R.dpreds_bound(dref, gd, bnd, preds=pd if underflow else None)
    tag = '%s %s %dch %s' % (tag, (N, H, W), CH, mode)
    losses, coef, dpreds, sums, k = run_abi(pd, gd, mode, gout, alpha, beta, ratio)
    # integers
    assert int(np.float32(float(sums[0]))) == ref['n_pos'] and int(np.float32(float(sums[1]))) == int(ref['sums']['neg']), (tag, sums.tolist())
    assert float(sums[7]) == ref['nonbin'], tag
    if k is not None:
        assert k == ref['n_neg'], (tag, k, ref['n_neg'])
    if mode == 'none':
        assert round(1.0 / float(coef[0]) - ref['n_pos']) == ref['n_neg'], tag
    exact(tag + ' coef[7]', coef[7:8], t64([0.0 if literal else float(ref['nonbin'])]))
    # sums
    for i, name in enumerate(R.SUMS):
        if CH == 2 and name in ('bgm', 'bm'):
            assert float(sums[i]) == 0.0
        elif dyadic and name != 'bce':
            exact('%s S_%s' % (tag, name), sums[i:i + 1], t64([ref['sums'][name]]))
        else:
            within('%s S_%s' % (tag, name), sums[i:i + 1], t64([ref['sums'][name]]), bnd['E'][name])
    # losses and the backward's coefficients
    within(tag + ' losses', losses, t64(ref['losses']), t64(bnd['losses']))
    within(tag + ' coef[0..3]', coef[:4], t64(bnd['coef']), t64(bnd['b_coef']))
    runs = [('abi', losses, dpreds)]
    if module:
        ml, mg = run_module(pd, gd, mode, gout, alpha, beta, ratio)
        want = t64(ref['losses']) if CH == 3 else t64(ref['losses'][4:])
        within(tag + ' DBLoss losses', ml, want, t64(bnd['losses'] if CH == 3 else bnd['losses'][4:]))
        runs.append(('DBLoss', ml, mg))
    for name, _, d in runs:
        t = '%s %s' % (tag, name)
        if mode == 'none':
            check_select_gradient(t, d[:, 0], dref, ref, gd, pd, gout, bnd, sel, tie)
            within(t + ' dT, dB', d[:, 1:], dref[:, 1:], dbound[:, 1:])
        else:
            within(t + ' dpreds', d, dref, dbound)
    if dyadic:
        check_dyadic_bits(tag, preds, gts, ref, gout, alpha, beta, losses, coef, dpreds)
    return ref, bnd


def check_dyadic_bits(tag, preds, gts, ref, gout, alpha, beta, losses, coef, dpreds):
    """Family (d): the sums other than the BCE are exact, so what db_loss_finish and db_loss_bwd_kernel derive from them alone is
    determined bit for bit — restated here operation by operation in IEEE fp32 (numpy / CPU torch)."""
    f = np.float32
    s, CH = ref['sums'], preds.shape[1]
    eps = f(1e-6)
    sa = f(s['area']) + eps
    thr, c1 = f(s['l1']) / sa, f(1) / sa
    g = [f(float(v)) for v in gout]
    G, M, Tg, A = gts
    if CH == 3:
        Un = f(s['bm']) + f(s['pos']) + eps
        I = f(s['bgm'])
        binl = f(1) - f(2) * I / Un
        w_thr = g[1] + f(beta) * (g[3] + g[4])
        w_bin = g[2] + f(alpha) * g[4]
        exact(tag + ' losses[1..2] bit for bit', losses[1:3], t64([float(thr), float(binl)]))
        exact(tag + ' coef[1..3] bit for bit', coef[1:4], t64([float(c1), float(Un), float(I)]))
        cd = f(-2) * w_bin / (Un * Un)
        dB = (float(cd) * M) * (G * float(Un) - float(I))
        assert dB.dtype == torch.float32
        exact(tag + ' dB bit for bit', dpreds[:, 2], dB)
    else:
        w_thr = f(beta) * g[4]
        exact(tag + ' losses[1] bit for bit', losses[1:2], t64([float(thr)]))
        exact(tag + ' coef[1..3] bit for bit', coef[1:4], t64([float(c1), 1.0, 0.0]))
    ca = c1 * w_thr
    dT = (float(ca) * A) * torch.sign(preds[:, 1] - Tg)
    assert dT.dtype == torch.float32 and isinstance(ca, np.float32)
    exact(tag + ' dT bit for bit', dpreds[:, 1], dT)
    exact(tag + ' coef[7]', coef[7:8], t64([0.0]))


# ---- (a) random data: every shape, mode and channel count -----------------------------------------------------------------------------


@pytest.mark.parametrize('CH', [2, 3])
@pytest.mark.parametrize('shape', R.SHAPES_SMALL + R.SHAPES_GRID)
def test_random_data(shape, CH):
    """(a) V = 1 (H W % 4 != 0) and V = 4, one workgroup to the 1024-workgroup cap with a second trip, all five modes, a random weight on
    all five outputs at once."""
    preds, gts = R.case_random(*shape, CH, seed=shape[1])
    small = shape[1] * shape[2] < 10000
    for i, mode in enumerate(MODES):
        check('(a)', preds, gts, mode, seed=10 * CH + i, ratio=3 if i % 2 == 0 else 0.5, module=small or mode in ('mean', 'none'))


def test_flush_of_the_running_sums():
    """(9, 2047, 2049): V = 1 at the cap with 72 trips per thread — `if (++cnt == 64)` of db_loss_fwd_kernel flushes the fp32 sums into
    the doubles once and eight more trips accumulate after it; 'mean', the reference image by image.
    Outcome on the MI355X (2026-10-19), the first time the flush ran: every sum within its bound (S_bce err / bound 0.004, the others
    below 0.001, the counts exact), losses 0.033, coef 0.022, dpreds 0.083."""
    N, H, W = R.SHAPE_FLUSH
    g = torch.Generator(device=DEV).manual_seed(9)
    P = torch.rand(N, H, W, device=DEV, generator=g) * 0.98 + 0.01
    T = torch.rand(N, H, W, device=DEV, generator=g) * 0.98 + 0.01
    preds = torch.stack([P, T, torch.sigmoid(50 * (P - T))], 1)
    del P, T
    u = torch.rand(4, N, H, W, device=DEV, generator=g)
    gts = torch.stack([(u[0] < 0.05).float(), (u[1] < 0.9).float(), 0.3 + 0.4 * u[2], (u[3] < 0.3).float()])
    del u
    alpha, beta = PARAMS[3]
    gout = gout_of(72)
    ref = R.db_loss_ref(preds, gts, alpha, beta, 'mean', 3, 1e-6)
    bnd = R.loss_bounds(ref, N, H, W, gout)
    assert bnd['geo']['trips'] >= 72 and bnd['geo']['depth'] == 64
    losses, coef, dpreds, sums, _ = run_abi(preds, gts, 'mean', gout, alpha, beta, 3)
    tag = '(flush) %s' % ((N, H, W), )
    # (binary maps: the folded doubles are the counts themselves — 32 million negatives, past what a float holds exactly)
    assert float(sums[0]) == ref['sums']['pos'] == ref['n_pos'] and float(sums[1]) == ref['sums']['neg'] and float(sums[7]) == 0
    assert ref['n_neg'] == 3 * ref['n_pos'] < ref['sums']['neg']
    for i, name in enumerate(R.SUMS):
        within('%s S_%s' % (tag, name), sums[i:i + 1], t64([ref['sums'][name]]), bnd['E'][name])
    within(tag + ' losses', losses, t64(ref['losses']), t64(bnd['losses']))
    within(tag + ' coef[0..3]', coef[:4], t64(bnd['coef']), t64(bnd['b_coef']))
    for n in (0, N // 2, N - 1):  # (the backward has no chain: three images, the first, one in the middle and the last)
        dref, _, _ = R.db_loss_grad_ref(preds, gts, gout, ref, image=n)
        within('%s dpreds of image %d' % (tag, n), dpreds[n:n + 1], dref, R.dpreds_bound(dref, gts, bnd, image=n))


# ---- (b) confident predictions ---------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize('sure', [False, True])
@pytest.mark.parametrize('shape', [(3, 7, 9), (1, 33, 31), (2, 64, 64), (5, 182, 181)])
def test_confident_predictions(shape, sure):
    """(b) P at distance 2^-30 .. 2^-1 from its target, wrong sides, P = 0, 1, 1 - 2^-24 and 2^-40 on both kinds of pixel, T == thresh_gt;
    sure: tiny terms alone (distance 2^-30 .. 2^-20, right side), where S_bce feels every bit of log1p.  'mean', 'sum', the literal
    form (bce_term) and 'none' (the libm form of the per-pixel path)."""
    for CH in (3, 2):
        preds, gts, sp = R.case_confident(*shape, CH, seed=shape[2], sure=sure)
        for i, mode in enumerate(['mean', 'sum', 'literal_mean', 'none']):
            ref, _ = check('(b%s)' % ('-sure' if sure else ''), preds, gts, mode, seed=20 + i, module=False)
    same = sp['same_T']
    d = run_abi(preds.to(DEV), gts.to(DEV), 'mean', gout_of(1), 1.0, 10.0, 3)[2]
    assert float(d[:, 1][same.to(DEV)].abs().max()) == 0.0  # dT exactly 0 where T == thresh_gt


# ---- (c) subnormal predictions -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize('shape', [(2, 33, 31), (2, 8, 8)])
def test_subnormal_predictions(shape):
    """(c) eight P in (2^-149, 2^-126), four on positive pixels (true terms 87.3 .. 100) and four on negative ones.  A logarithm that
    took a subnormal argument for 0 would return the clamp 100 and move S_bce by a hundred times its bound (test_loss_ref_cpu.py).
    Outcome on the MI355X (2026-10-19): bce_term passes as it is — S_bce err / bound 0.03 at (2, 33, 31), 0.05 at (2, 8, 8): the
    compiler expands __logf with a 2^32 scaling of subnormal arguments in front of the hardware instruction.  dP carries the absolute
    floor of gradual underflow here (loss_ref.dpreds_bound)."""
    preds, gts, idx = R.case_subnormal(*shape, 3)
    for mode in ('mean', 'sum', 'literal_mean', 'none'):
        check('(c)', preds, gts, mode, seed=30, module=mode == 'mean', underflow=True)


# ---- (d) dyadic data, (e) fractional maps ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize('CH', [2, 3])
@pytest.mark.parametrize('shape', [(3, 7, 9), (2, 5, 4), (2, 64, 64), (5, 182, 181), (2, 1030, 1028)])
def test_dyadic_data_bit_for_bit(shape, CH):
    """(d) every sum but the BCE exact in fp32: losses[1], losses[2], coef[1..3], coef[7], dT and dB bit for bit."""
    preds, gts = R.case_dyadic(*shape, CH, seed=shape[1])
    for i, mode in enumerate(['mean', 'sum']):
        check('(d)', preds, gts, mode, seed=40 + i, dyadic=True, module=False)


@pytest.mark.parametrize('CH', [2, 3])
@pytest.mark.parametrize('shape', [(3, 7, 9), (2, 64, 64), (5, 182, 181)])
def test_fractional_maps(shape, CH):
    """(e) prob_gt and mask multiples of 1/8, the literal form (two-logarithm BCE, top-k over `negative`) and 'none'; under the default
    form coef[7] is the exact number of non-binary pixels."""
    preds, gts = R.case_fractional(*shape, CH, seed=shape[1])
    for i, (mode, ratio) in enumerate([('literal_mean', 3), ('literal_sum', 2.3), ('none', 0.7)]):
        ref, _ = check('(e)', preds, gts, mode, seed=50 + i, ratio=ratio, module=shape[1] < 100)
    pd, gd = preds.to(DEV), gts.to(DEV)
    for mode in ('mean', 'sum'):
        coef = run_abi(pd, gd, mode, gout_of(0), 1.0, 10.0, 3)[1]
        exact('(e) %s coef[7] of the default form' % mode, coef[7:8], t64([float(ref['nonbin'])]))
    assert ref['nonbin'] > 0


# ---- (f) ratios, (g) select ------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize('ratio', R.RATIOS)
def test_negative_ratio_truncates_as_the_reference(ratio):
    """(f) int(n_pos * ratio) in doubles (losses.py:26) with exactly 10 m positives: a ratio rounded to float truncates one lower for 0.7,
    2.3 and 3.3 (asserted by the generator).  'none' (the count is exact) and the literal form on fractional masks (the loss moves)."""
    shape = (2, 33, 31)
    for CH in (3, 2):
        preds, gts = R.case_ratio(*shape, CH, ratio)
        ref, _ = check('(f) ratio %g' % ratio, preds, gts, 'none', seed=60, ratio=ratio)
        print('(f) ratio %g: n_pos %d, n_neg %d' % (ratio, ref['n_pos'], ref['n_neg']))
        preds, gts = R.case_ratio(*shape, CH, ratio, fractional=True)
        check('(f) ratio %g' % ratio, preds, gts, 'literal_mean', seed=61, ratio=ratio)
        check('(f) ratio %g' % ratio, preds, gts, 'literal_sum', seed=62, ratio=ratio, module=False)


@pytest.mark.parametrize('kind', ['group', 'low_bits', 'k_zero', 'all', 'tau_zero'])
def test_radix_select(kind):
    """(g) 'none': k inside a group of 50 equal values; k inside ~1000 values that share their top 22 bits (the third radix pass); k = 0;
    k = every negative; tau = 0 with masked pixels tying with it."""
    for shape, CH in [((2, 33, 31), 3), ((2, 64, 64), 2)]:
        preds, gts = R.case_select(kind, *shape, CH)
        ref, _ = check('(g) ' + kind, preds, gts, 'none', seed=70)
        if kind == 'k_zero':
            d = run_abi(preds.to(DEV), gts.to(DEV), 'none', gout_of(70), *PARAMS[CH], 3)[2]
            assert float(d[:, 0].abs().max()) == 0.0 and ref['losses'][0] == 0.0
