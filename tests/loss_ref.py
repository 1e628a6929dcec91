"""float64 reference of DBLoss (the reference's losses.py:18-139, statement by statement), its analytic gradient, the error bounds of
the HIP loss kernels (csrc/head_loss.hip) against it, and the case generators of tests/test_loss_fp64_gpu.py.

Plain torch elementwise operations and reductions in float64 on whatever device the inputs live on; the case generators draw on the
CPU from seeded generators, so tests/test_loss_ref_cpu.py checks the preconditions of exactly the data the GPU tests run.
"""
import math

import numpy as np
import torch

U = 2.0**-24  # unit roundoff of fp32
EPS12 = float(np.float32(1e-12))  # ATen's binary_cross_entropy_backward: max((1 - x) x, EPSILON) with EPSILON = 1e-12 in the input's type
SUMS = ('pos', 'neg', 'bce', 'l1', 'area', 'bgm', 'bm')


def bce64(P, G):
    """F.binary_cross_entropy(..., reduction='none') as ATen evaluates it: both logarithms clamped at -100."""
    return -(G * torch.log(P).clamp_min(-100.0) + (1.0 - G) * torch.log1p(-P).clamp_min(-100.0))


def db_loss_ref(preds, gts, alpha=1.0, beta=10.0, reduction='mean', negative_ratio=3, eps=1e-6):
    """losses.py:18-139 in float64, image by image (the float64 temporaries stay one image large; only the vector handed to
    torch.topk is whole).  Returns a dict: losses[5] (for 2-channel preds [2] = 0 and [3] = [4] = prob + beta thresh, what the kernels
    write), sums (pos, neg, bce, l1, area and the dice sums bgm, bm), n_pos, n_neg, nonbin (pixels whose prob_gt or mask is neither 0
    nor 1), and what the gradient needs: pos_term + top_term = the numerator of the balance loss (in units of the scalar loss for
    'mean' / 'sum'), idx (topk's indices), kth (the k-th value of topk's input)."""
    N, CH, H, W = preds.shape
    s = dict.fromkeys(SUMS, 0.0)
    nonbin = 0
    neg_parts, loss_parts, pos_term = [], [], 0.0
    for n in range(N):
        P, T = preds[n, 0].double(), preds[n, 1].double()
        G, M, Tg, A = (gts[k, n].double() for k in range(4))
        positive = G * M  # losses.py:22-23
        negative = (1.0 - G) * M
        l = bce64(P, G)
        s['pos'] += float(positive.sum())
        s['neg'] += float(negative.sum())
        s['bce'] += float(l.sum())
        s['l1'] += float(((T - Tg).abs() * A).sum())  # losses.py:77
        s['area'] += float(A.sum())
        if CH == 3:
            B = preds[n, 2].double()
            s['bgm'] += float((B * G * M).sum())  # losses.py:62-63
            s['bm'] += float((B * M).sum())
        nonbin += int(((G * (1.0 - G) != 0) | (M * (1.0 - M) != 0)).sum())
        if reduction == 'none':
            pos_term += float((l * positive).sum())
            loss_parts.append((l * negative).reshape(-1))
        else:
            pos_term += float(positive.sum())
        neg_parts.append(negative.reshape(-1))
    px = N * H * W
    n_pos = int(s['pos'])  # losses.py:25-28
    n_neg = min(int(n_pos * negative_ratio), int(s['neg']))
    negative = torch.cat(neg_parts)
    if reduction == 'none':
        scalar = 1.0
        negative_loss = torch.cat(loss_parts)
    else:
        scalar = s['bce'] if reduction == 'sum' else s['bce'] / px  # losses.py:30: ONE scalar
        negative_loss = scalar * negative  # losses.py:34
    vals, idx = torch.topk(negative_loss, n_neg)  # losses.py:36
    kth = float(vals[-1]) if n_neg > 0 else None
    # (in units of the scalar: scalar * negative[idx] is what topk returned, and the scalar is >= 0)
    top_term = float(vals.sum()) if reduction == 'none' else float(negative[idx].sum())
    denom = n_pos + n_neg + eps
    prob = scalar * (pos_term + top_term) / denom  # losses.py:38-39
    thr = s['l1'] / (s['area'] + eps)  # losses.py:77-78
    pt = prob + beta * thr
    if CH == 3:
        union = s['bm'] + s['pos'] + eps
        binl = 1.0 - 2.0 * s['bgm'] / union  # losses.py:64
        losses = [prob, thr, binl, pt, alpha * binl + pt]
    else:
        losses = [prob, thr, 0.0, pt, pt]
    return dict(losses=losses, sums=s, n_pos=n_pos, n_neg=n_neg, nonbin=nonbin, px=px, scalar=scalar, pos_term=pos_term, top_term=top_term,
                denom=denom, idx=idx, kth=kth, negative_loss=negative_loss, reduction=reduction, CH=CH, alpha=alpha, beta=beta, eps=eps)


def weights(gout, CH, alpha, beta):
    """Weights of the three base losses under upstream gradients gout[5] of (prob, thresh, binary, prob + beta thresh, total)."""
    g = [float(v) for v in gout]
    if CH == 3:
        return g[0] + g[3] + g[4], g[1] + beta * (g[3] + g[4]), g[2] + alpha * g[4]
    return g[4], beta * g[4], 0.0


def db_loss_grad_ref(preds, gts, gout, ref, image=None):
    """d(sum_i gout[i] losses[i]) / d preds in float64 for the evaluation `ref` = db_loss_ref(preds, gts, ...); image: that image only
    (not with 'none').  BCE: ATen's (x - t) / max((1 - x) x, float32(1e-12)) — the clamp of the forward is not differentiated, as in
    ATen.  For 'none' also returns topk's selection mask and the tie class (negatives whose value equals the k-th value), else None."""
    N, CH, H, W = preds.shape
    w_prob, w_thr, w_bin = weights(gout, CH, ref['alpha'], ref['beta'])
    s = ref['sums']
    sl = slice(None) if image is None else slice(image, image + 1)
    P, T = preds[sl, 0].double(), preds[sl, 1].double()
    G, M, Tg, A = (gts[k, sl].double() for k in range(4))
    dbce = (P - G) / ((1.0 - P) * P).clamp_min(EPS12)
    sel = tie = None
    if ref['reduction'] == 'none':
        assert image is None
        sel = torch.zeros(N * H * W, dtype=torch.float64, device=preds.device)
        sel[ref['idx']] = 1.0
        sel = sel.view(N, H, W)
        neg = (1.0 - G) * M
        dP = (w_prob / ref['denom']) * (G * M + neg * sel) * dbce
        tie = torch.zeros_like(sel, dtype=torch.bool) if ref['kth'] is None else (ref['negative_loss'].view(N, H, W) == ref['kth']) & (neg > 0)
    else:
        div = 1.0 if ref['reduction'] == 'sum' else ref['px']
        dP = (w_prob * (ref['pos_term'] + ref['top_term']) / ref['denom'] / div) * dbce
    d = T - Tg
    dT = (w_thr / (s['area'] + ref['eps'])) * A * torch.sign(d)
    out = [dP, dT]
    if CH == 3:
        union = s['bm'] + s['pos'] + ref['eps']
        out.append((-2.0 * w_bin / (union * union)) * M * (G * union - s['bgm']))
    return torch.stack(out, 1), sel, tie


# ---- the kernels' launch geometry and error bounds -------------------------------------------------------------------------------


def fwd_geometry(N, H, W):
    """db_loss_fwd_run: V floats per item (4 when H W % 4 == 0), workgroups of 512 threads capped at 1024, grid-stride trips per thread,
    and the depth of a thread's fp32 chain: min(trips, 64) V adds (the running sums are flushed into doubles every 64 trips)."""
    V = 4 if (H * W) % 4 == 0 else 1
    items = N * H * W // V
    nb = min(max(-(-items // 512), 1), 1024)
    trips = -(-items // (nb * 512))
    return dict(V=V, nb=nb, trips=trips, depth=min(trips, 64) * V)


# Roundings inside one term, counted from db_loss_fwd_kernel (-ffp-contract=off: no fused multiply-add):
#   pos  G M: 1.   neg  (1 - G) M: 2.   l1  |T - Tg| A: 2.   area: 0.   bgm  B G M: 2.   bm  B M: 1.
#   bce  binary target, positive pixel: log(x) = v_log_f32 (1 ulp = 2 u) times the rounded constant ln 2 (u) and the product (u): 4 u.
#        negative pixel: log(w) u / (w - 1) with w = fl(1 + u) and w - 1 exact: log 4 u, v_rcp_f32 1 ulp = 2 u, two products 2 u, and the
#        form's own distance to log1p from the rounding of w, below 1 u (|d/dw ln(log(w) / (w - 1))| <= 0.89 on [1/2, 1] where the
#        rounding of w is at most u / 2; w is exact below 1/2): 9 u, taken as 10.
#        fractional target: two libm logarithms at 2 ulp = 4 u each on terms of one sign, (t - 1) 1, two products and a difference: below 10.
C_TERM = dict(pos=1, neg=2, bce=10, l1=2, area=0, bgm=2, bm=1)
C_LOG = 10  # the bce entry: the one constant the issue allows to be replaced by a measured one
# bce_px of the per-pixel path (ohem_values_kernel): the two-logarithm form (7 u, see above) times (1 - G) M (2) or G M (1) and the product: 10
C_PX = 10
SECOND_ORDER = 1.001  # every relative error below is < 1e-3 (asserted): products of two of them stay below 1e-3 of their sum


def gamma(n):
    return n * U / (1.0 - n * U)


def _r(b, x):
    return b / abs(x) if x != 0 else 0.0


def loss_bounds(ref, N, H, W, gout=None, literal=False, c_log=C_LOG):
    """Absolute bounds of losses[5] and of coef[0..3], and the relative errors of the backward's coefficients, first order with the
    factor SECOND_ORDER on top.

    Forward sums: a thread adds depth = min(trips, 64) V terms in fp32 (fwd_geometry), each with c roundings of its own (C_TERM);
    everything after the chain is float64 (2^-40 covers it).  All terms are >= 0, so sum |term| is the sum:
        E_k = (gamma(depth + c_k) + 2^-40) S_k.
    db_loss_finish, one u per fp32 operation or cast (eps itself is the float 1e-6: u eps):
        bce  = (float)(S_bce / div):                        E_bce / div + u bce
        num  = (float)S_pos + (float)n_neg:                 E_pos + u S_pos + u n_neg + u num
               literal form (ohem_finalize_kernel, the top-k sum of `negative` exact in float64 by the cases' construction): u num
               'none': pos_loss + top-k sum of per-pixel values at C_PX u each (a top-k sum moves by at most the k largest
               perturbations, and those are proportional to the values): gamma(C_PX) num + u num
        den  = (float)(n_pos + n_neg + eps):                u den
        prob = bce num / den: relative errors add, + 2 u    ('none': num / den, + u)
        thr  = (float)S_l1 / ((float)S_area + eps):         sa = S_area + eps with E_area + u S_area + u eps + u sa; + u for the division
        pt   = prob + beta thr:                             b_prob + beta b_thr + u |beta thr| + u |pt|
        Un   = (float)S_bm + (float)S_pos + eps:            E_bm + E_pos + u (S_bm + S_pos) + u eps + 2 u Un;   I = (float)S_bgm: E_bgm + u I
        binl = 1 - 2 I / Un:                                q = 2 I / Un with relative r_I + r_U + u; b_q + u |binl|
        total = alpha binl + pt:                            alpha b_binl + u |alpha binl| + b_pt + u |total|
        coef[0] = num / den / (float)div: r_num + r_den + 3 u   ('none': 1 / den: r_den + u);  coef[1] = 1 / sa: r_sa + u
    db_loss_bwd_kernel: w_prob = g0 + g3 + g4 (2 u (|g0| + |g3| + |g4|)), w_thr = g1 + beta (g3 + g4), w_bin = g2 + alpha g4 likewise;
        dP = cb wsel (P - G) / max((1 - P) P, 1e-12): cb = coef[0] w_prob (+ u), then P - G, 1 - P, two products and a division, the tie
             weight and its product under 'none': r_cb + 8 u relative
        dT = ca A sign: r_ca + u with ca = coef[1] w_thr (+ u)
        dB = cd M (G Un - I), cd = -2 w_bin / (Un Un): r_cd = r_wbin + 2 r_U + 2 u; the bracket has the ABSOLUTE error
             b_in = G b_U + u G Un + b_I + u |G Un - I| (it cancels), so |dB - ref| <= |cd| M b_in + (r_cd + 2 u) |ref|."""
    geo = fwd_geometry(N, H, W)
    s, CH, red, alpha, beta, eps = ref['sums'], ref['CH'], ref['reduction'], ref['alpha'], ref['beta'], ref['eps']
    c = dict(C_TERM, bce=c_log)
    E = {k: (gamma(geo['depth'] + c[k]) + 2.0**-40) * s[k] for k in SUMS}
    n_pos, n_neg, den = ref['n_pos'], ref['n_neg'], ref['denom']
    div = 1.0 if red == 'sum' else float(ref['px'])
    num = ref['pos_term'] + ref['top_term']
    if red == 'none':
        b_num = gamma(C_PX) * num + U * num
        r_prob = _r(b_num, num) + U + U
        r_c0 = U + U
    else:
        bce = s['bce'] / div
        b_bce = E['bce'] / div + U * bce
        b_num = (U * num + 2.0**-40 * num) if literal else (E['pos'] + U * s['pos'] + U * n_neg + U * num)
        r_prob = _r(b_bce, bce) + _r(b_num, num) + U + 2 * U
        r_c0 = _r(b_num, num) + U + 3 * U
    prob, thr, binl, pt, total = ref['losses']
    b_prob = abs(prob) * r_prob
    sa = s['area'] + eps
    b_sa = E['area'] + U * s['area'] + U * eps + U * sa
    r_thr = _r(E['l1'] + U * s['l1'], s['l1']) + b_sa / sa + U
    b_thr = thr * r_thr
    r_c1 = b_sa / sa + U
    b_pt = b_prob + beta * b_thr + U * abs(beta * thr) + U * abs(pt)
    out = dict(geo=geo, E=E)
    if CH == 3:
        Un = s['bm'] + s['pos'] + eps
        b_U = E['bm'] + E['pos'] + U * (s['bm'] + s['pos']) + U * eps + 2 * U * Un
        I = s['bgm']
        b_I = E['bgm'] + U * I
        q = 2.0 * I / Un
        b_binl = q * (_r(b_I, I) + b_U / Un + U) + U * abs(binl)
        b_total = alpha * b_binl + U * abs(alpha * binl) + b_pt + U * abs(total)
        b_losses = [b_prob, b_thr, b_binl, b_pt, b_total]
        coef = [num / den / div if red != 'none' else 1.0 / den, 1.0 / sa, Un, I]
        b_coef = [coef[0] * r_c0, coef[1] * r_c1, b_U, b_I]
    else:
        Un, b_U, I, b_I = 1.0, 0.0, 0.0, 0.0
        b_losses = [b_prob, b_thr, 0.0, b_pt, b_pt]
        coef = [num / den / div if red != 'none' else 1.0 / den, 1.0 / sa, 1.0, 0.0]
        b_coef = [coef[0] * r_c0, coef[1] * r_c1, 0.0, 0.0]
    rels = [r_prob, r_thr, r_c0, r_c1, b_U / Un]
    out.update(losses=[SECOND_ORDER * b for b in b_losses], coef=coef, b_coef=[SECOND_ORDER * b for b in b_coef])
    if gout is not None:
        g = [abs(float(v)) for v in gout]
        gs = [float(v) for v in gout]
        w_prob, w_thr, w_bin = weights(gout, CH, alpha, beta)
        if CH == 3:
            b_wp = 2 * U * (g[0] + g[3] + g[4])
            s34 = abs(beta * (gs[3] + gs[4]))
            b_wt = beta * U * (g[3] + g[4]) + U * s34 + U * (g[1] + s34)
            b_wb = U * abs(alpha * gs[4]) + U * (g[2] + abs(alpha * gs[4]))
        else:
            b_wp, b_wt, b_wb = 0.0, U * abs(beta * gs[4]), 0.0
        r_cb = r_c0 + _r(b_wp, w_prob) + U
        r_ca = r_c1 + _r(b_wt, w_thr) + U
        r_cd = _r(b_wb, w_bin) + 2 * b_U / Un + 2 * U
        rels += [r_cb, r_ca, r_cd]
        out.update(r_dP=SECOND_ORDER * (r_cb + 8 * U), r_dT=SECOND_ORDER * (r_ca + U), r_dB=SECOND_ORDER * (r_cd + 2 * U),
                   cd=-2.0 * w_bin / (Un * Un), Un=Un, I=I, b_in=(b_U, b_I))
    assert max(rels) < 1e-3, rels  # (what SECOND_ORDER relies on)
    return out


def dpreds_bound(dref, gts, bnd, image=None, preds=None):
    """Elementwise bound of dpreds against db_loss_grad_ref's `dref` (see loss_bounds).  It is exactly 0 wherever the reference is
    exactly 0 and the bracket of dB carries no weight: masked L1, T == Tg, M = 0, unselected negatives, P == G.
    preds (the subnormal family): the two products in front of dP's division may round in the subnormal range, 2^-150 each in absolute
    terms whatever the value (gradual underflow), which the division by max((1 - P) P, 1e-12) magnifies: + 2^-149 / max(...) + 2^-149."""
    sl = slice(None) if image is None else slice(image, image + 1)
    out = [bnd['r_dP'] * dref[:, 0].abs(), bnd['r_dT'] * dref[:, 1].abs()]
    if preds is not None:
        P = preds[sl, 0].double()
        out[0] = out[0] + 2.0**-149 / ((1.0 - P) * P).clamp_min(EPS12) + 2.0**-149
    if dref.shape[1] == 3:
        G, M = gts[0, sl].double(), gts[1, sl].double()
        b_U, b_I = bnd['b_in']
        b_in = G * b_U + U * G * bnd['Un'] + b_I + U * (G * bnd['Un'] - bnd['I']).abs()
        out.append(SECOND_ORDER * abs(bnd['cd']) * M * b_in + bnd['r_dB'] * dref[:, 2].abs())
    return torch.stack(out, 1)


# ---- fp32 restatements (tests/test_loss_ref_cpu.py) ------------------------------------------------------------------------------


def bce_term_f32(P, G, naive=False):
    """bce_term of head_loss.hip for binary targets in torch fp32: log(x) on positive pixels; on negative ones log1p(u), u = -x, as
    log(w) u / (w - 1) with w = fl(1 + u) (w == 1: u).  naive: log(1 - x) as it stands."""
    P, G = P.float(), G.float()
    u = -P
    w = torch.where(G == 1, P, 1.0 + u)
    l = torch.log(w)
    if not naive:
        safe = torch.where(w == 1, torch.full_like(w, 0.5), w)
        l = torch.where(G == 1, l, torch.where(w == 1, u, l * (u / (safe - 1.0))))
    return -l.clamp_min(-100.0)


def n_neg_float_ratio(n_pos, s_neg, ratio):
    """The truncation with the ratio rounded to float first: what a `float negative_ratio` argument computes."""
    return min(int(float(n_pos) * float(np.float32(ratio))), int(s_neg))


# ---- cases -------------------------------------------------------------------------------------------------------------------------

SHAPES_SMALL = [(1, 1, 1), (1, 1, 3), (2, 3, 5), (3, 7, 9), (1, 33, 31), (2, 5, 4), (2, 64, 64)]
SHAPES_GRID = [(5, 182, 181), (3, 419, 421), (2, 1030, 1028)]
SHAPE_FLUSH = (9, 2047, 2049)
RATIOS = [3, 1, 0.5, 0.7, 2.3, 3.3]


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _binary_gts(N, H, W, g, p_pos=0.2, p_mask=0.9, p_area=0.3):
    u = torch.rand(4, N, H, W, generator=g)
    return torch.stack([(u[0] < p_pos).float(), (u[1] < p_mask).float(), 0.3 + 0.4 * u[2], (u[3] < p_area).float()])


def _preds(P, T, CH):
    planes = [P, T] + ([torch.sigmoid(50 * (P - T))] if CH == 3 else [])
    return torch.stack(planes, 1).contiguous()


def case_random(N, H, W, CH, seed=0):
    """(a) P, T in (0.01, 0.99), binary prob_gt / mask / text area, thresh_gt in (0.3, 0.7)."""
    g = _g(1000 + seed)
    P = torch.rand(N, H, W, generator=g) * 0.98 + 0.01
    T = torch.rand(N, H, W, generator=g) * 0.98 + 0.01
    return _preds(P, T, CH), _binary_gts(N, H, W, g)


SPECIALS = ('zero', 'one', 'one_minus', 'tiny')


def case_confident(N, H, W, CH, seed=0, sure=False):
    """(b) P at distance 2^-30 .. 2^-1 (log-uniform) from its target, a tenth of the pixels on the wrong side; on a quarter of the pixels
    (at most 64 of each kind) P = 0, P = 1, P = 1 - 2^-24 and P = 2^-40 (1 - P == 1), cycling, so that on maps of a few hundred pixels each
    value meets positive and negative pixels; T == thresh_gt on every fifth pixel.  Returns (preds, gts, special), special[name] = mask.
    sure: every pixel on the right side at distance 2^-30 .. 2^-20 and no special values — the BCE sum is then made of tiny terms alone,
    and an evaluation that loses them (log(1 - x) as it stands) moves it by far more than its bound."""
    g = _g(2000 + seed)
    gts = _binary_gts(N, H, W, g, p_pos=0.4)
    G = gts[0]
    d = torch.exp2(-((20.0 if sure else 1.0) + (10.0 if sure else 29.0) * torch.rand(N, H, W, generator=g).double()))
    wrong = torch.rand(N, H, W, generator=g) < (0.0 if sure else 0.1)
    tgt = torch.where(wrong, 1.0 - G, G).double()
    P = torch.where(tgt == 1, 1.0 - d, d).float().reshape(-1)
    n = P.numel()
    perm = torch.randperm(n, generator=g)
    vals = dict(zero=0.0, one=1.0, one_minus=1.0 - 2.0**-24, tiny=2.0**-40)
    special = {}
    m = 0 if sure else min(n // 4, 256)
    for j, name in enumerate(SPECIALS):
        idx = perm[j:m:4]
        P[idx] = vals[name]
        mask = torch.zeros(n, dtype=torch.bool)
        mask[idx] = True
        special[name] = mask.view(N, H, W)
    P = P.view(N, H, W)
    T = torch.rand(N, H, W, generator=g) * 0.98 + 0.01
    same = (torch.arange(n) % 5 == 0).view(N, H, W)
    T = torch.where(same, gts[2], T)
    special['same_T'] = same
    return _preds(P, T, CH), gts, special


def case_subnormal(N, H, W, CH, seed=0):
    """(c) the random family with eight subnormal P, multiples of 2^-149 inside (2^-149, 2^-126), four on positive and four on negative
    pixels inside the mask.  Returns (preds, gts, index of the eight pixels)."""
    preds, gts = case_random(N, H, W, CH, seed)
    mult = [3, 1000, 2**20 + 1, 2**23 - 1]
    G = gts[0].reshape(-1)
    M = gts[1].reshape(-1)
    P = preds[:, 0].reshape(-1).clone()
    pos = ((G == 1) & (M == 1)).nonzero().reshape(-1)[:4]
    neg = ((G == 0) & (M == 1)).nonzero().reshape(-1)[:4]
    assert pos.numel() == 4 and neg.numel() == 4
    sub = torch.tensor(mult, dtype=torch.float64) * 2.0**-149
    P[pos] = sub.float()
    P[neg] = sub.float()
    preds[:, 0] = P.view(N, H, W)
    return preds, gts, torch.cat([pos, neg])


def case_dyadic(N, H, W, CH, seed=0):
    """(d) binary G, M, A; T, thresh_gt, B multiples of 2^-6 in [0, 1]: a thread's fp32 sums other than the BCE are exact (at most 256 terms, all
    multiples of 2^-6 in [0, 1]), so the folded doubles are the exact sums, in any order."""
    g = _g(4000 + seed)
    gts = _binary_gts(N, H, W, g)
    gts[2] = torch.randint(0, 65, (N, H, W), generator=g).float() / 64
    P = torch.rand(N, H, W, generator=g) * 0.98 + 0.01
    T = torch.randint(0, 65, (N, H, W), generator=g).float() / 64
    planes = [P, T] + ([torch.randint(0, 65, (N, H, W), generator=g).float() / 64] if CH == 3 else [])
    return torch.stack(planes, 1).contiguous(), gts


def case_fractional(N, H, W, CH, seed=0):
    """(e) prob_gt and mask multiples of 1/8: G M and (1 - G) M are multiples of 1/64, their sums exact in fp32 and float64.  Asserts that
    both sums lie at least 1/64 above an integer, so that no truncation sits on a boundary."""
    g = _g(5000 + seed)
    preds, gts = case_random(N, H, W, CH, seed)
    gts[0] = torch.randint(0, 9, (N, H, W), generator=g).float() / 8
    gts[1] = torch.randint(0, 9, (N, H, W), generator=g).float() / 8
    for s in ((gts[0] * gts[1]).double().sum(), ((1 - gts[0]) * gts[1]).double().sum()):
        assert 1 / 64 <= float(s) - math.floor(float(s)) <= 63 / 64, float(s)
    return preds, gts


def ratio_positives(ratio):
    """n_pos = 10 m, the smallest m at which the float-rounded ratio truncates differently (3 where it never does: 3, 1, 0.5)."""
    for m in range(1, 40):
        if int(10 * m * ratio) != int(10 * m * float(np.float32(ratio))):
            return 10 * m
    return 30


def case_ratio(N, H, W, CH, ratio, seed=0, fractional=False):
    """(f) exactly 10 m positives inside the mask and more negatives than ratio n_pos.  fractional (the literal form): the negatives' mask
    values are multiples of 1/8 in [1/8, 7/8], so that one negative more or less changes the top-k sum."""
    g = _g(6000 + seed)
    preds, gts = case_random(N, H, W, CH, seed)
    n = N * H * W
    n_pos = ratio_positives(ratio)
    if ratio in (0.7, 2.3, 3.3):
        assert int(n_pos * ratio) != int(n_pos * float(np.float32(ratio))), ratio  # the double and the float truncation differ
    perm = torch.randperm(n, generator=g)
    G = torch.zeros(n)
    G[perm[:n_pos]] = 1.0
    M = torch.ones(n)
    if fractional:
        M = torch.randint(1, 8, (n, ), generator=g).float() / 8
        M[perm[:n_pos]] = 1.0
    M[perm[n_pos:n_pos + n // 8]] = 0.0  # some masked negatives
    gts[0], gts[1] = G.view(N, H, W), M.view(N, H, W)
    assert float((G * M).sum()) == n_pos and int(((1 - G) * M).double().sum()) > int(n_pos * ratio) + 1
    return preds, gts


def case_select(kind, N, H, W, CH, seed=0):
    """(g) the radix select of reduction='none' (negative_ratio 3):  'group' 50 negatives with P = 1/2, 40 harder ones, 20 positives:
    k = 60 takes 20 of the group.  'low_bits' 200 positives, 100 hard negatives, 1000 negatives at consecutive floats from 2^-10 up
    (their loss values share the top 22 bits: only the third radix pass separates them), the rest easier: k = 600 falls inside.
    'k_zero' no positives.  'all' more positives than a third of the negatives: every negative is selected.  'tau_zero' 20 positives,
    30 negatives with a loss, 100 with P = 0 (loss exactly 0), everything else masked: k = 60, the k-th value is 0."""
    g = _g(7000 + seed)
    preds, gts = case_random(N, H, W, CH, seed)
    n = N * H * W
    perm = torch.randperm(n, generator=g)
    P = preds[:, 0].reshape(-1).clone()
    G, M = torch.zeros(n), torch.ones(n)

    def take(count, at=[0]):
        idx = perm[at[0]:at[0] + count]
        at[0] += count
        assert idx.numel() == count
        return idx

    if kind == 'group':
        G[take(20)] = 1.0
        P[take(40)] = torch.rand(40, generator=g) * 0.09 + 0.9
        P[take(50)] = 0.5
        rest = perm[110:]
        P[rest] = torch.rand(rest.numel(), generator=g) * 0.29 + 0.01
    elif kind == 'low_bits':
        G[take(200)] = 1.0
        P[take(100)] = torch.rand(100, generator=g) * 0.4 + 0.5
        base = int(np.float32(2.0**-10).view(np.int32))
        P[take(1000)] = torch.from_numpy((base + np.arange(1000, dtype=np.int32)).view(np.float32).copy())
        rest = perm[1300:]
        P[rest] = torch.rand(rest.numel(), generator=g) * 2.0**-12 + 2.0**-13
    elif kind == 'k_zero':
        pass
    elif kind == 'all':
        G[take(n // 2)] = 1.0
        M[take(n // 8)] = 0.0
    elif kind == 'tau_zero':
        G[take(20)] = 1.0
        take(30)
        P[take(100)] = 0.0
        M[perm[150:]] = 0.0
    else:
        raise ValueError(kind)
    preds[:, 0] = P.view(N, H, W)
    gts[0], gts[1] = G.view(N, H, W), M.view(N, H, W)
    return preds, gts


def select_band(ref, gts):
    """Negatives whose float64 value lies within 2 gamma(C_PX) (relative) of the k-th value: where an fp32 evaluation of the values (C_PX
    roundings each, on the value and on the threshold) may order differently from float64.  Exact ties are inside."""
    N, H, W = gts.shape[1:]
    if ref['kth'] is None:
        return torch.zeros(N, H, W, dtype=torch.bool, device=gts.device)
    v = ref['negative_loss'].view(N, H, W)
    neg = ((1.0 - gts[0].double()) * gts[1].double()) > 0
    return neg & ((v - ref['kth']).abs() <= 2 * gamma(C_PX) * abs(ref['kth']))
