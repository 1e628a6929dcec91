"""float64 reference of the DB head's tail backward THROUGH the BatchNorm in front of each branch's last transposed convolution
(db_text_minimal_amd/csrc/head_loss.hip dbn_head_tail_bn_bwd_t), written from the formulas (no autograd):

    y [npx, 64] --BatchNorm (train)--> y sc + sh --ReLU--> x --ConvT(64 -> 1, k 2, s 2), weight w [64, 4]--> logits [npx, 4]
    P = sigmoid(logit_b), T = sigmoid(logit_t), B = sigmoid(k (P - T));  given d(preds) on the maps.

The entry point takes the maps `preds` as given (it never recomputes them), so does the reference.  tests/test_head_bn_bwd_ref_cpu.py
checks it against torch.autograd."""
import torch


def to_quads(t, N, Hq, Wq):
    """[N, 2Hq, 2Wq] full-resolution map -> [N Hq Wq, 4]: the 2 x 2 block (a, b) of each quarter pixel, ab = 2 a + b (the ConvT tap)."""
    return t.reshape(N, Hq, 2, Wq, 2).permute(0, 1, 3, 2, 4).reshape(N * Hq * Wq, 4)


def logit_grads(preds, dpreds, N, Hq, Wq, CH, kstep):
    """dl_b, dl_t [npx, 4] (gradients w.r.t. the two logits) and A_b, A_t = (|dP| + |gB|) P (1 - P): the magnitudes that bound the fp32
    evaluation error of dl (as tests/test_train16_ops_gpu.py ht_logit_grads)."""
    q = lambda t, c: to_quads(t[:, c].double(), N, Hq, Wq)
    P, T, dP, dT = q(preds, 0), q(preds, 1), q(dpreds, 0), q(dpreds, 1)
    aP, aT = dP.abs(), dT.abs()
    if CH == 3:
        B = q(preds, 2)
        gB = q(dpreds, 2) * kstep * B * (1 - B)
        dP, dT = dP + gB, dT - gB
        aP, aT = aP + gB.abs(), aT + gB.abs()
    return (dP * P * (1 - P), dT * T * (1 - T)), (aP * (P * (1 - P)).abs(), aT * (T * (1 - T)).abs())


def branch_backward(y, w, dl, scale, shift, mean, rstd, gamma, grad_scale=1.0):
    """One branch, all float64: y [npx, 64] BatchNorm input, w [64, 4], dl [npx, 4] logit gradients; scale / shift the BatchNorm's
    affine (gamma rstd, beta - mean gamma rstd), mean / rstd its saved statistics.
    Returns dy1 [npx, 64] (gradient of y), dgamma, dbeta [64], dbias3 [64] (bias gradient of the conv that produced y: column sums of
    dy1), dw6 [64, 4] and dbias6 (the last ConvT's gradients) — the parameter gradients times grad_scale — and the intermediates
    g (ReLU-masked gradient of the BatchNorm output), xhat, c1, c2, x, abs1 = sum |g|, abs2 = sum |g xhat|."""
    M = y.shape[0]
    a = y * scale + shift
    mask = a > 0
    x = a.clamp_min(0)
    g = (dl @ w.t()) * mask
    xhat = (y - mean) * rstd
    gx = g * xhat
    s1, s2 = g.sum(0), gx.sum(0)
    c1, c2 = s1 / M, s2 / M
    dy = gamma * rstd * (g - c1 - xhat * c2)
    return {'dy1': dy, 'dgamma': s2 * grad_scale, 'dbeta': s1 * grad_scale, 'dbias3': dy.sum(0) * grad_scale,
            'dw6': (x.t() @ dl) * grad_scale, 'dbias6': dl.sum() * grad_scale,
            'g': g, 'xhat': xhat, 'c1': c1, 'c2': c2, 'x': x, 'mask': mask, 'abs1': g.abs().sum(0), 'abs2': gx.abs().sum(0)}


def head_bn_bwd(yb, yt, wb, wt, preds, dpreds, bn_b, bn_t, N, Hq, Wq, CH, kstep, grad_scale=1.0):
    """Both branches.  yb / yt [N, Hq, Wq, 64]; wb / wt [64, 4]; preds / dpreds [N, CH, 2Hq, 2Wq]; bn_b / bn_t: dicts with scale, shift,
    mean, rstd, gamma [64].  Returns (result of branch_backward for b, for t, (A_b, A_t))."""
    d = lambda t: t.double()
    (dlb, dlt), A = logit_grads(preds, dpreds, N, Hq, Wq, CH, kstep)
    out = []
    for y, w, dl, bn in ((yb, wb, dlb, bn_b), (yt, wt, dlt, bn_t)):
        r = branch_backward(d(y).reshape(-1, 64), d(w).reshape(64, 4), dl, d(bn['scale']), d(bn['shift']), d(bn['mean']), d(bn['rstd']),
                            d(bn['gamma']), grad_scale)
        r['dl'] = dl
        out.append(r)
    return out[0], out[1], A
