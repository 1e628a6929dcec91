"""float64 restatement of the optimizer extensions of csrc/optim.hip (gradient accumulation, global norm clipping, L2 weight decay, AMSGrad),
written from the definitions of torch.optim.Adam and torch.nn.utils.clip_grad_norm_ with elementwise operations only; runs on whatever
device its operands live on.  tests/test_optim_ext_cpu.py pins it against torch itself in float64.

    acc  = g_1 + ... + g_k
    norm = |s| sqrt(sum acc^2)                       s = grad_scale
    coef = min(1, max_norm / (norm + 1e-6))          (1 when max_norm is None; a NaN norm gives NaN)
    g    = coef s acc + weight_decay p
    m'   = b1 m + (1 - b1) g;   v' = b2 v + (1 - b2) g^2;   vmax' = max(vmax, v')   (amsgrad)
    p'   = p - (lr / bc1) m' / (sqrt(vmax' or v') / sqrt(bc2) + eps)
"""
import torch


def grad_norm(acc, grad_scale=1.0):
    """|s| sqrt(sum acc^2): the norm clip_grad_norm_ sees when the gradients are s acc."""
    return abs(grad_scale) * acc.double().square().sum().sqrt()


def clip_coef(norm, max_norm):
    """clip_grad_norm_'s coefficient: max_norm / (norm + 1e-6) clamped to at most 1 (torch.clamp: a NaN stays NaN)"""
    if max_norm is None:
        return torch.ones((), dtype=torch.float64, device=norm.device)
    return torch.clamp(max_norm / (norm + 1e-6), max=1.0)


def adam_step_ex(p, acc, m, v, vmax, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, max_norm=None):
    """One update in float64.  vmax None: no AMSGrad.  Returns (p', m', v', vmax' or None, parts): parts holds the magnitudes the tests'
    bounds are made of (the norm, the coefficient, the two terms of g and of m', the root, the denominator, the update)."""
    p, acc, m, v = p.double(), acc.double(), m.double(), v.double()
    norm = grad_norm(acc, grad_scale)
    coef = clip_coef(norm, max_norm)
    ga, gd = coef * grad_scale * acc, weight_decay * p
    g = ga + gd
    a, b = beta1 * m, (1 - beta1) * g
    m1 = a + b
    v1 = beta2 * v + (1 - beta2) * g * g
    vmax1 = None if vmax is None else torch.maximum(vmax.double(), v1)
    root = v1 if vmax is None else vmax1
    bc1, bc2 = 1 - beta1**step, 1 - beta2**step
    denom = root.sqrt() / (bc2**0.5) + eps
    upd = (lr / bc1) * (m1 / denom)
    parts = {'norm': norm, 'coef': coef, 'g': g, 'g_terms': ga.abs() + gd.abs(), 'ga': ga, 'm_terms': a.abs() + b.abs(), 'b2v': beta2 * v,
             'root': root, 'denom': denom, 'upd': upd, 'lrc': lr / bc1, 'c2': 1 / bc2**0.5}
    return p - upd, m1, v1, vmax1, parts
