"""The float64 DBLoss reference of tests/loss_ref.py against the oracle (autograd in float64) and the golden known answers, the
preconditions every case generator of tests/test_loss_fp64_gpu.py claims, and two fp32 restatements showing that the cases would
catch a naive log(1 - x) and a float-rounded negative_ratio.  No GPU."""
import os

import numpy as np
import pytest
import torch

import loss_ref as R
from loss_ref import U
from oracle import dbnet_oracle as O

GOUT = [0.7, -1.3, 0.4, 1.1, 0.9]


def _oracle(preds, gts, gout, **kw):
    p = preds.double().requires_grad_(True)
    out = O.db_loss(p, gts.double(), **kw)
    if preds.shape[1] == 3:
        vals = [float(v.detach()) for v in out]
        sum(g * v for g, v in zip(gout, out)).backward()
    else:
        vals = [float(out.detach())]
        (gout[4] * out).backward()
    return vals, p.grad


@pytest.mark.parametrize('CH', [2, 3])
@pytest.mark.parametrize('reduction', ['mean', 'sum', 'none'])
@pytest.mark.parametrize('family', ['random', 'fractional'])
def test_reference_equals_the_oracle_with_autograd(family, reduction, CH):
    """db_loss_ref / db_loss_grad_ref against oracle.db_loss (F.binary_cross_entropy, torch.topk, autograd) in float64: same statements,
    so they agree to float64 rounding.  Both map families: on fractional maps the literal top-k form is the only one."""
    N, H, W = 2, 13, 11
    preds, gts = (R.case_random if family == 'random' else R.case_fractional)(N, H, W, CH, seed=3)
    kw = dict(alpha=0.75, beta=3.5, reduction=reduction, negative_ratio=2.3, eps=1e-6)
    ref = R.db_loss_ref(preds, gts, **kw)
    vals, grad = _oracle(preds, gts, GOUT, **kw)
    got = ref['losses'] if CH == 3 else [ref['losses'][4]]
    assert np.allclose(got, vals, rtol=1e-12, atol=1e-14), (got, vals)
    dref, sel, tie = R.db_loss_grad_ref(preds, gts, GOUT, ref)
    assert torch.allclose(dref, grad, rtol=1e-11, atol=1e-16), float((dref - grad).abs().max())
    if reduction == 'none':
        assert int(sel.sum()) == ref['n_neg'] and int(tie.sum()) >= 1
    if family == 'random':
        assert ref['nonbin'] == 0
        if reduction != 'none':
            cf = O.db_loss_closed_form(preds, gts, **kw)
            assert np.allclose(got, cf if CH == 3 else cf[-1:], rtol=1e-12, atol=1e-14), (got, cf)
    else:
        assert ref['nonbin'] == int(((gts[0] * (1 - gts[0]) != 0) | (gts[1] * (1 - gts[1]) != 0)).sum()) > 0


KATS = {'default': {}, 'eval2ch': {}, 'no_positive': {}, 'all_masked': {}, 'neg_limited': {}, 'saturated': {},
        'alpha_beta': dict(alpha=5.0, beta=2.0, negative_ratio=1), 'reduction_none': dict(reduction='none'), 'reduction_sum': dict(reduction='sum'),
        'fractional_mask': {}, 'fractional_gt_and_mask': {}, 'fractional_mask_topk_selects': dict(negative_ratio=2),
        'fractional_mask_sum': dict(negative_ratio=2, reduction='sum')}


@pytest.mark.parametrize('tag', sorted(KATS))
def test_reference_equals_the_golden_known_answers(golden_dir, tag):
    """... at the tolerances tests/test_loss_gpu.py holds the kernels to (the goldens are the reference's own fp32 outputs)."""
    z = np.load(os.path.join(golden_dir, 'loss_kats.npz'))
    preds, gts = torch.from_numpy(z[tag + '/preds']), torch.from_numpy(z[tag + '/gts'])
    ref = R.db_loss_ref(preds, gts, **KATS[tag])
    want = z[tag + '/losses'].astype(np.float64).reshape(-1)
    got = np.array(ref['losses'] if preds.shape[1] == 3 else [ref['losses'][4]])
    assert want.shape == got.shape and np.all(np.abs(got - want) <= 1e-5 + 1e-5 * np.abs(want)), (got, want)
    dref, _, _ = R.db_loss_grad_ref(preds, gts, [0, 0, 0, 0, 1.0], ref)
    wd = torch.from_numpy(z[tag + '/dpreds']).double()
    atol = 1e-6 * max(float(wd.abs().max()), 1e-3)
    assert bool(((dref - wd).abs() <= atol + 1e-4 * wd.abs()).all()), float((dref - wd).abs().max())


# ---- preconditions of the case generators -----------------------------------------------------------------------------------------


def test_geometry_of_the_issue_shapes():
    geo = {s: R.fwd_geometry(*s) for s in R.SHAPES_SMALL + R.SHAPES_GRID + [R.SHAPE_FLUSH]}
    for s in [(1, 1, 1), (1, 1, 3), (2, 3, 5), (3, 7, 9), (1, 33, 31)]:
        assert geo[s]['V'] == 1 and geo[s]['nb'] <= 4, s  # (a handful of workgroups at the most)
    assert geo[(2, 5, 4)] == dict(V=4, nb=1, trips=1, depth=4)
    assert geo[(2, 64, 64)]['V'] == 4
    assert geo[(5, 182, 181)]['V'] == 1 and 100 < geo[(5, 182, 181)]['nb'] < 1024 and geo[(5, 182, 181)]['trips'] == 1
    assert geo[(3, 419, 421)]['V'] == 1 and geo[(3, 419, 421)]['nb'] == 1024 and geo[(3, 419, 421)]['trips'] == 2
    assert geo[(2, 1030, 1028)]['V'] == 4 and geo[(2, 1030, 1028)]['nb'] == 1024 and geo[(2, 1030, 1028)]['trips'] == 2
    f = geo[R.SHAPE_FLUSH]
    assert f['V'] == 1 and f['nb'] == 1024 and f['trips'] >= 72 and f['depth'] == 64  # the flush at 64, and at least 8 trips after it


@pytest.mark.parametrize('shape', [(3, 7, 9), (1, 33, 31), (2, 64, 64)])
def test_confident_family_holds_what_it_claims(shape):
    preds, gts, sp = R.case_confident(*shape, 3, seed=1)
    P, G = preds[:, 0], gts[0]
    d = torch.where(G == 1, 1 - P.double(), P.double())
    assert float(d.min()) == 0.0 and bool(((d > 0) & (d < 2.0**-24)).any() or shape[1] < 30)
    assert bool((d > 0.5).any())  # wrong side
    want = dict(zero=0.0, one=1.0, one_minus=float(np.float32(1 - 2.0**-24)), tiny=float(np.float32(2.0**-40)))
    for name in R.SPECIALS:
        assert bool((P[sp[name]] == want[name]).all())
        if shape[1] >= 30:  # on both kinds of pixel
            assert bool((G[sp[name]] == 1).any()) and bool((G[sp[name]] == 0).any()), name
    assert float(np.float32(1) - np.float32(2.0**-40)) == 1.0 and float(np.float32(1 - 2.0**-24)) < 1.0
    assert bool((preds[:, 1][sp['same_T']] == gts[2][sp['same_T']]).all()) and int(sp['same_T'].sum()) > 0
    dref, _, _ = R.db_loss_grad_ref(preds, gts, [0, 1.0, 0, 0, 0], R.db_loss_ref(preds, gts))
    assert float(dref[:, 1][sp['same_T']].abs().max()) == 0.0  # dT exactly 0 there


def test_subnormal_family_holds_what_it_claims():
    preds, gts, idx = R.case_subnormal(2, 33, 31, 3, seed=0)
    P = preds[:, 0].reshape(-1)[idx].double()
    assert bool(((P > 2.0**-149) & (P < 2.0**-126)).all())
    G, M = gts[0].reshape(-1)[idx], gts[1].reshape(-1)[idx]
    assert G.tolist() == [1.0] * 4 + [0.0] * 4 and bool((M == 1).all())
    term = R.bce64(P, G.double())
    assert bool(((term[:4] > 87.3) & (term[:4] <= 100)).all()) and bool((term[4:] == P[4:]).all())
    # a flushed logarithm returns the clamp 100: that moves S_bce by far more than its bound
    ref = R.db_loss_ref(preds, gts)
    bnd = R.loss_bounds(ref, 2, 33, 31)
    assert float((100.0 - term[:4]).sum()) > 100 * bnd['E']['bce']


@pytest.mark.parametrize('shape', [(3, 7, 9), (2, 64, 64)])
def test_dyadic_and_fractional_families_hold_what_they_claim(shape):
    preds, gts = R.case_dyadic(*shape, 3, seed=0)
    for t in (gts[0], gts[1], gts[3]):
        assert bool(((t == 0) | (t == 1)).all())
    for t in (preds[:, 1], preds[:, 2], gts[2]):
        assert bool((t * 64 == (t * 64).round()).all()) and 0 <= float(t.min()) and float(t.max()) <= 1
    ref = R.db_loss_ref(preds, gts)
    for k in ('pos', 'neg', 'l1', 'area', 'bgm', 'bm'):  # exact in fp32 in any order: multiples of 2^-6 below 2^18
        assert ref['sums'][k] * 64 == round(ref['sums'][k] * 64) and ref['sums'][k] < 2.0**18
    preds, gts = R.case_fractional(*shape, 3, seed=0)
    for t in (gts[0], gts[1]):
        assert bool((t * 8 == (t * 8).round()).all())
    ref = R.db_loss_ref(preds, gts, negative_ratio=2.3)
    assert ref['nonbin'] > 0 and 0 < ref['n_neg']
    for k in ('pos', 'neg'):
        fr = ref['sums'][k] - int(ref['sums'][k])
        assert 1 / 64 <= fr <= 63 / 64 and ref['sums'][k] * 64 == round(ref['sums'][k] * 64)
    assert ref['top_term'] * 64 == round(ref['top_term'] * 64)  # the top-k sum of `negative` is exact


@pytest.mark.parametrize('ratio', R.RATIOS)
def test_ratio_family_fails_for_a_float_rounded_ratio(ratio):
    """The fp32 restatement of the truncation: for 0.7, 2.3 and 3.3 a ratio that crossed the C ABI as float selects one negative fewer,
    and both forms of family (f) see it: the count under 'none', the loss of the literal form by far more than its bound."""
    N, H, W = 2, 33, 31
    preds, gts = R.case_ratio(N, H, W, 3, ratio)
    ref = R.db_loss_ref(preds, gts, reduction='none', negative_ratio=ratio)
    n_pos = R.ratio_positives(ratio)
    assert ref['n_pos'] == n_pos and n_pos % 10 == 0 and ref['n_neg'] == int(n_pos * ratio) < int(ref['sums']['neg'])
    slipped = R.n_neg_float_ratio(ref['n_pos'], ref['sums']['neg'], ratio)
    if ratio in (0.7, 2.3, 3.3):
        assert slipped == ref['n_neg'] - 1
    else:
        assert slipped == ref['n_neg']
        return
    assert R.select_band(ref, gts).sum() == 1  # no ties: the number of negatives with a gradient is n_neg exactly
    preds, gts = R.case_ratio(N, H, W, 3, ratio, fractional=True)
    lit = R.db_loss_ref(preds, gts, reduction='mean', negative_ratio=ratio)
    assert lit['n_neg'] == ref['n_neg']
    neg = ((1 - gts[0]) * gts[1]).double().reshape(-1)
    top = float(torch.topk(neg, slipped)[0].sum())
    wrong = lit['scalar'] * (lit['pos_term'] + top) / (lit['n_pos'] + slipped + 1e-6)
    bound = R.loss_bounds(lit, N, H, W, literal=True)['losses'][0]
    print('ratio %g: n_neg %d, float-rounded %d; literal prob %.9g vs %.9g, bound %.3e' % (ratio, lit['n_neg'], slipped, lit['losses'][0], wrong, bound))
    assert abs(wrong - lit['losses'][0]) > 100 * bound


@pytest.mark.parametrize('kind', ['group', 'low_bits', 'k_zero', 'all', 'tau_zero'])
def test_select_family_holds_what_it_claims(kind):
    N, H, W = 2, 33, 31
    preds, gts = R.case_select(kind, N, H, W, 3)
    ref = R.db_loss_ref(preds, gts, reduction='none')
    v = ref['negative_loss']
    neg = (((1 - gts[0]) * gts[1]) > 0).reshape(-1)
    _, _, tie = R.db_loss_grad_ref(preds, gts, GOUT, ref)
    if kind == 'group':
        assert ref['n_neg'] == 60 and ref['kth'] == float(R.bce64(torch.tensor(0.5, dtype=torch.float64), torch.tensor(0.0, dtype=torch.float64)))
        assert int(tie.sum()) == 50 >= 40 and int((v > ref['kth']).sum()) == 40 < ref['n_neg'] < 90  # k falls inside the group
        assert bool((R.select_band(ref, gts) == tie).all())
    elif kind == 'low_bits':
        bits = v.float().numpy().view(np.int32)  # the float32 reference values
        kb = int(np.float32(ref['kth']).view(np.int32))
        cls = (bits >> 10) == (kb >> 10)
        above, below = int(((bits >> 10) > (kb >> 10)).sum()), int((neg.numpy() & ((bits >> 10) < (kb >> 10))).sum())
        assert ref['n_neg'] == 600 and int(cls.sum()) >= 900 and 0 < above < 600 < above + int(cls.sum()) and below > 0, (int(cls.sum()), above, below)
        assert len(np.unique(bits[cls])) >= 900  # ... and they are different values: the third pass has to separate them
        assert int(tie.sum()) == 1
    elif kind == 'k_zero':
        assert ref['n_pos'] == 0 and ref['n_neg'] == 0 and ref['losses'][0] == 0.0
    elif kind == 'all':
        assert ref['n_neg'] == int(ref['sums']['neg']) == int(neg.sum()) < 3 * ref['n_pos']
    else:
        assert ref['n_neg'] == 60 and ref['kth'] == 0.0 and int((v > 0).sum()) == 30 and int((neg & (v == 0)).sum()) == 100
        assert int((~neg & (v == 0)).sum()) > 0  # masked pixels tie with tau = 0


# ---- fp32 restatements of bce_term ---------------------------------------------------------------------------------------------------


def test_bce_term_form_against_float64_and_a_naive_log_fails_family_b():
    """log(w) u / (w - 1) in torch fp32 (CPU logarithm) against float64 on negative pixels whose prediction is log-uniform in distance
    2^-30 .. 2^-1 from the target: the form's own distance, printed in units of u — it has to sit inside the C_LOG u that loss_bounds
    grants the kernel's term.  log(1 - x) as it stands loses every bit below 2^-24: on family (b) its BCE sum misses the bound."""
    g = torch.Generator().manual_seed(11)
    d = torch.exp2(-(1.0 + 29.0 * torch.rand(1 << 18, generator=g).double())).float()
    zero = torch.zeros_like(d)
    ref = R.bce64(d.double(), zero.double())
    rel = ((R.bce_term_f32(d, zero).double() - ref).abs() / ref).max() / U
    rel_naive = ((R.bce_term_f32(d, zero, naive=True).double() - ref).abs() / ref).max() / U
    print('bce_term form in fp32: worst relative error %.2f u (naive log(1 - x): %.3g u)' % (float(rel), float(rel_naive)))
    assert float(rel) <= R.C_LOG and float(rel_naive) > 1e6
    # positive pixels near 1: log(x) itself
    one = torch.ones_like(d)
    refp = R.bce64((1 - d).float().double(), one.double())
    ok = refp > 0
    relp = ((R.bce_term_f32((1 - d).float(), one).double() - refp).abs()[ok] / refp[ok]).max() / U
    print('log(x) near 1 in fp32: worst relative error %.2f u' % float(relp))
    assert float(relp) <= R.C_LOG
    for shape, sure in [((1, 33, 31), True), ((2, 64, 64), True), ((2, 64, 64), False)]:
        preds, gts, _ = R.case_confident(*shape, 3, seed=0, sure=sure)
        r = R.db_loss_ref(preds, gts)
        E = R.loss_bounds(r, *shape)['E']['bce']
        P, G = preds[:, 0], gts[0]
        good = float(R.bce_term_f32(P, G).double().sum())
        naive = float(R.bce_term_f32(P, G, naive=True).double().sum())
        print('family (b) %s sure=%s: S_bce %.9g, form err / bound %.3f, naive err / bound %.3f' % (shape, sure, r['sums']['bce'], abs(good - r['sums']['bce']) / E,
                                                                                             abs(naive - r['sums']['bce']) / E))
        assert abs(good - r['sums']['bce']) <= E
        if sure:  # (with wrong-side pixels and clamped terms in the sum, the tiny terms a naive logarithm loses hide below its bound)
            assert abs(naive - r['sums']['bce']) > 100 * E
