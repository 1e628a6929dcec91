"""float64 restatements of the optimizer family of csrc/optim_groups.hip (dbn_sgd_step, dbn_adamw_step: parameter groups, norm clipping,
the weight EMA), written from the definitions of torch.optim.SGD, torch.optim.AdamW, torch.optim.Adam(weight_decay) and
torch.nn.utils.clip_grad_norm_ with elementwise operations only, in the manner of tests/optim_ref.py (whose norm, coefficient and Adam
update are reused); they run on whatever device their operands live on.  tests/test_optim_family_cpu.py pins them against torch itself
in float64.  `lr` and `weight_decay` are floats or per-element tensors (per_element() spreads a run table).

    coef = min(1, max_norm / (|s| sqrt(sum acc^2) + 1e-6))       (1 without clipping)        s = grad_scale
    SGD    g = coef s acc + wd p;   buf' = g (first update) | mu buf + (1 - damp) g;   d = g + mu buf' | buf' | g;   p' = p - lr d
    AdamW  decoupled: pd = p (1 - lr wd), then Adam's update on pd with the undecayed gradient;  coupled: Adam's on g = coef s acc + wd p
    EMA    shadow' = d shadow + (1 - d) p'       with d and 1 - d the two fp32 values the kernel receives

The same file holds the data of the GPU tests (family_data: CPU generators, so that the CPU tests see the very same numbers) and the
first-order fp32 error bounds derived in tests/test_optim_family_gpu.py's docstring, so that the CPU tests can hold wrong variants of the
rules against them.  `wrong` selects such a variant: 'dampen_first', 'decay_before_clip', 'no_nesterov' (SGD), 'decay_after' (AdamW).
"""
import torch

import optim_ref as R

U = 2.0**-24
# the floats the ABI receives: two groups, their learning rates and decays (large on purpose: see test_wrong_rules_are_told_apart)
LRS, WDS = ([float(torch.tensor(x, dtype=torch.float32)) for x in xs] for xs in ((0.1, 0.05), (0.5, 0.25)))
MU, DAMP = float(torch.tensor(0.9, dtype=torch.float32)), 0.25  # (1 - DAMP is exact in fp32)
B1, B2, EPS = (float(torch.tensor(x, dtype=torch.float32)) for x in (0.9, 0.999, 1e-8))
GS = 0.25
EMA_D = float(torch.tensor(0.9, dtype=torch.float32))
EMA_OMD = float(torch.tensor(1.0 - 0.9, dtype=torch.float32))
SGD_MODES = {'plain': (0.0, 0.0, False), 'momentum': (MU, 0.0, False), 'dampening': (MU, DAMP, False), 'nesterov': (MU, 0.0, True)}


def per_element(values, run_end, run_group, n, dtype=torch.float64, device='cpu'):
    """values[run_group[r]] on the elements of run r (quads [run_end[r - 1], run_end[r])); the elements past the last whole quad and
    past the last end take the last run's"""
    out = torch.full((n, ), float(values[run_group[-1]]), dtype=dtype, device=device)
    lo = 0
    for end, g in zip(run_end, run_group):
        out[4 * lo:min(4 * end, n)] = values[g]
        lo = end
    return out


def family_data(n, seed, steps=2):
    """(p, [gradient of each update]) in fp32 on the CPU.  With grad_scale 1/4 the scaled gradients are z and z / 2 for standard normal z,
    the parameters standard normal."""
    g = torch.Generator().manual_seed(1000 + seed)
    p = torch.randn(n, generator=g)
    return p, [torch.randn(n, generator=g) * (4.0 / (i + 1)) for i in range(steps)]


def two_runs(n):
    """a two-group run table over n elements that splits at about a third (quads)"""
    n4 = max((n + 3) // 4, 1)
    cut = max(n4 // 3, 1)
    return ([cut, n4], [0, 1]) if n4 > 1 else ([n4], [1])


def sgd_step(p, acc, buf, lr, wd, momentum, dampening, nesterov, first, grad_scale=1.0, max_norm=None, wrong=None):
    """One update in float64.  buf None with momentum 0.  Returns (p', buf' or None, parts): parts holds the magnitudes the bounds are
    made of."""
    p, acc = p.double(), acc.double()
    norm = R.grad_norm(acc, grad_scale)
    coef = R.clip_coef(norm, max_norm)
    ga, gd = coef * grad_scale * acc, wd * p
    if wrong == 'decay_before_clip':
        gd = coef * gd
    g = ga + gd
    parts = {'norm': norm, 'coef': coef, 'ga': ga, 'gd': gd + torch.zeros_like(ga), 'g': g, 'lr': lr, 'first': first}
    buf1 = None
    if momentum == 0:
        d = g
    else:
        if first and wrong != 'dampen_first':
            a, b = torch.zeros_like(g), g
        else:
            a, b = momentum * (torch.zeros_like(g) if first else buf.double()), (1 - dampening) * g
        buf1 = a + b
        parts.update(b_terms=a.abs() + b.abs(), omd=1 - dampening, mu=momentum)
        if nesterov and wrong != 'no_nesterov':
            d = g + momentum * buf1
            parts['d_terms'] = g.abs() + (momentum * buf1).abs()
        else:
            d = buf1
    upd = lr * d
    parts.update(d=d, upd=upd)
    return p - upd, buf1, parts


def adamw_step(p, acc, m, v, vmax, lr, b1, b2, eps, wd, step, decoupled, grad_scale=1.0, max_norm=None, wrong=None):
    """One update in float64 through optim_ref.adam_step_ex.  Returns (p', m', v', vmax' or None, parts); parts['pd'] is the decayed
    parameter of the decoupled form."""
    p = p.double()
    if not decoupled:
        return R.adam_step_ex(p, acc, m, v, vmax, lr, b1, b2, eps, wd, step, grad_scale=grad_scale, max_norm=max_norm)
    pd = p if wrong == 'decay_after' else p * (1 - lr * wd)
    p1, m1, v1, x1, parts = R.adam_step_ex(pd, acc, m, v, vmax, lr, b1, b2, eps, 0.0, step, grad_scale=grad_scale, max_norm=max_norm)
    if wrong == 'decay_after':
        p1 = p1 * (1 - lr * wd)
    parts['pd'] = pd
    return p1, m1, v1, x1, parts


def ema_step(shadow, p1, d, omd):
    """shadow' and the magnitudes of its two terms"""
    a, b = d * shadow.double(), omd * p1.double()
    return a + b, a.abs() + b.abs()


# ------------------------------------------------------------------------------------------------------------------------------------
# the fp32 error bounds (first order in U; derivation: tests/test_optim_family_gpu.py)
# ------------------------------------------------------------------------------------------------------------------------------------
def grad_bound(parts, n, decay):
    E = (n + 8) * 2.0**-53
    dg = (2 * U + E) * parts['ga'].abs()
    if decay:
        dg = dg + U * parts['gd'].abs() + U * parts['g'].abs()
    return dg


def sgd_bounds(parts, p1, n, decay):
    """(|dbuf| or None, |dp|) from the magnitudes sgd_step returns"""
    dg = grad_bound(parts, n, decay)
    dbuf = None
    if 'b_terms' in parts:
        dbuf = dg if parts['first'] else parts['omd'] * dg + 2 * U * parts['b_terms']
        dd = dg + parts['mu'] * dbuf + 2 * U * parts['d_terms'] if 'd_terms' in parts else dbuf
    else:
        dd = dg
    return dbuf, parts['lr'] * dd + U * parts['upd'].abs() + U * p1.abs()


def adam_bounds(parts, p1, v1, b1, b2, n, decay, decoupled=False):
    """(|dm|, |dv|, |dp|): ex_bounds of tests/test_optim_ext_gpu.py with the kernel's roundings, plus 2 U |pd| for the decoupled decay"""
    dg = grad_bound(parts, n, decay)
    g = parts['g']
    bm = (1 - b1) * dg + 2 * U * parts['m_terms']
    bv = U * parts['b2v'] + (1 - b2) * (2 * g.abs() * dg + 2 * U * g * g) + U * v1
    root = parts['root']
    dsqrt = torch.where(root > 0, bv / root.sqrt().clamp_min(1e-300), torch.zeros_like(bv))
    bd = parts['c2'] * dsqrt + 4 * U * parts['denom']
    bp = parts['lrc'] * bm / parts['denom'] + parts['upd'].abs() * (bd / parts['denom'] + 3 * U) + U * p1.abs()
    if decoupled:
        bp = bp + 2 * U * parts['pd'].abs()
    return bm, bv, bp


def ema_bound(terms, dp, omd):
    return omd * dp + 2 * U * terms
