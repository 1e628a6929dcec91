"""float64 references of the kernels of csrc/pointwise.hip that tests/test_bn_pool_ops_gpu.py pins: train-mode BatchNorm (statistics and
running statistics, the four apply forms, the backward with its three mask forms), MaxPool2d(3, 2, 1) over relu(affine) and its two
backward forms, the FPN's nearest upsample (add, concat, adjoint) and one Adam step.

Plain torch, elementwise operations and reductions only, on whatever device the operands live on (the step-sized cases keep them on
the GPU); every operand is expected in float64 already (the caller rounds to the storage type first, then .double()).  Activations are
[M, C] or NHWC.  tests/test_bn_pool_ref_cpu.py checks every function here against torch.autograd / F.batch_norm / F.max_pool2d /
F.interpolate / oracle.AdamState, so that a wrong reference cannot make a GPU test pass."""
import torch


# ---- BatchNorm ----------------------------------------------------------------------------------------------------------------------
def bn_stats(x, gamma, beta, eps, momentum=None, run_mean=None, run_var=None):
    """x [M, C] -> dict: mean, var (biased), rstd = 1 / sqrt(var + eps), scale = gamma rstd, shift = beta - mean scale and, with running
    statistics given, their update run' = (1 - momentum) run + momentum new (new variance unbiased: var M / (M - 1), var itself at M = 1)."""
    M = x.shape[0]
    mean = x.mean(0)
    var = ((x - mean)**2).mean(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * rstd
    out = {'mean': mean, 'var': var, 'rstd': rstd, 'scale': scale, 'shift': beta - mean * scale}
    if run_mean is not None:
        out['unbiased'] = var * (M / (M - 1.0)) if M > 1 else var
        out['run_mean'] = (1 - momentum) * run_mean + momentum * mean
        out['run_var'] = (1 - momentum) * run_var + momentum * out['unbiased']
    return out


def bn_apply(y, scale, shift, res=None, res_scale=None, res_shift=None, relu=False):
    """The four forms: y sc + sh; relu(.); relu(. + res); . + (res rsc + rsh) (any of them with or without the ReLU)."""
    o = y * scale + shift
    if res is not None:
        o = o + (res * res_scale + res_shift if res_scale is not None else res)
    return o.clamp_min(0) if relu else o


def bn_mask(y, zmask=None, mask_scale=None, mask_shift=None):
    """The ReLU mask of the backward: saved activation > 0, or y msc + msh > 0 recomputed, or None (no ReLU behind the BatchNorm)."""
    if zmask is not None:
        return zmask > 0
    if mask_scale is not None:
        return y * mask_scale + mask_shift > 0
    return None


def bn_backward(y, dout, mean, rstd, gamma, mask=None, grad_scale=1.0):
    """Backward of train-mode BatchNorm at y [M, C] for saved mean / rstd: g = dout [mask]; xhat = (y - mean) rstd;
    dbeta = gs sum g; dgamma = gs sum g xhat; dy = gamma rstd (g - mean(g) - xhat mean(g xhat)).  Returns a dict that also holds g, xhat,
    c1 = mean(g), c2 = mean(g xhat) and the float64 sums of |g| and |g xhat| (the test's bounds need them)."""
    M = y.shape[0]
    g = dout if mask is None else dout * mask
    xhat = (y - mean) * rstd
    gx = g * xhat
    s1, s2 = g.sum(0), gx.sum(0)
    c1, c2 = s1 / M, s2 / M
    return {'g': g, 'xhat': xhat, 'c1': c1, 'c2': c2, 'dbeta': s1 * grad_scale, 'dgamma': s2 * grad_scale, 'abs1': g.abs().sum(0),
            'abs2': gx.abs().sum(0), 'dy': gamma * rstd * (g - c1 - xhat * c2)}


# ---- MaxPool2d(3, 2, 1) over z = relu(y sc + sh) ------------------------------------------------------------------------------------
def pool_out(n):
    return (n - 1) // 2 + 1


def _windows(z, pad_value):
    """z [N, H, W, C] -> [9, N, Ho, Wo, C]: tap 3 r + q of every window (rows 2 oh - 1 + r, columns 2 ow - 1 + q), padding = pad_value."""
    N, H, W, C = z.shape
    Ho, Wo = pool_out(H), pool_out(W)
    p = torch.full((N, 2 * Ho + 1, 2 * Wo + 1, C), pad_value, dtype=z.dtype, device=z.device)
    p[:, 1:H + 1, 1:W + 1] = z
    return torch.stack([p[:, r:r + 2 * Ho:2, q:q + 2 * Wo:2] for r in range(3) for q in range(3)])


def pool_fwd(z):
    """z [N, H, W, C] (>= 0) -> pooled [N, Ho, Wo, C]."""
    return _windows(z, -1.0).amax(0)


def _scatter(t9, H, W):
    """Adjoint of _windows: t9 [9, N, Ho, Wo, C] -> [N, H, W, C]."""
    _, N, Ho, Wo, C = t9.shape
    p = torch.zeros((N, 2 * Ho + 1, 2 * Wo + 1, C), dtype=t9.dtype, device=t9.device)
    for r in range(3):
        for q in range(3):
            p[:, r:r + 2 * Ho:2, q:q + 2 * Wo:2] += t9[3 * r + q]
    return p[:, 1:H + 1, 1:W + 1].contiguous()


def pool_bwd_all_ties(z, pooled, dpool):
    """dz [N, H, W, C] = [z > 0] * sum of dpool over the windows that contain the pixel and whose maximum EQUALS z: every position that
    ties with the maximum receives the window's gradient (the rule of dbn_bnrelu_maxpool_bwd_t; without ties it is autograd's)."""
    N, H, W, C = z.shape
    zw = _windows(z, -1.0)
    hit = (zw == pooled.unsqueeze(0)) & (zw > 0)
    return _scatter(hit * dpool.unsqueeze(0), H, W)


def pool_first_argmax(z):
    """Code 3 r + q of the FIRST maximum of every window in scan order (nn.MaxPool2d's rule), 15 where the pooled value is 0."""
    zw = _windows(z, -1.0)
    m = zw.amax(0)
    first = (zw == m.unsqueeze(0)).to(torch.uint8).argmax(0)  # argmax of a 0 / 1 tensor: the first 1
    return torch.where(m > 0, first, torch.full_like(first, 15))


def pool_bwd_from_codes(codes, dpool, H, W):
    """g [N, H, W, C]: every window's dpool lands on the one position its code names (none for code 15)."""
    taps = torch.arange(9, device=codes.device).view(9, 1, 1, 1, 1)
    return _scatter((codes.unsqueeze(0) == taps) * dpool.unsqueeze(0), H, W)


def pool_gather_codes(t, codes):
    """t [N, H, W, C] -> its value at the position every window's code names ([N, Ho, Wo, C]; 0 for code 15)."""
    tw = _windows(t, 0.0)
    return torch.gather(tw, 0, codes.clamp_max(8).long().unsqueeze(0)).squeeze(0) * (codes != 15)


# ---- nearest upsample (F.interpolate(size=...)) -------------------------------------------------------------------------------------
def nearest_index(out_size, in_size, device='cpu'):
    """src = min(floor(dst in / out), in - 1) in exact integer arithmetic (equal to PyTorch's float evaluation at the tested sizes:
    tests/test_bn_pool_ref_cpu.py)."""
    return ((torch.arange(out_size, device=device) * in_size) // out_size).clamp_max(in_size - 1)


def nearest_up(src, H, W):
    """src [N, Hs, Ws, C] -> [N, H, W, C]."""
    ih, iw = nearest_index(H, src.shape[1], src.device), nearest_index(W, src.shape[2], src.device)
    return src[:, ih][:, :, iw]


def nearest_up_adjoint(dbig, Hs, Ws):
    """dbig [N, H, W, C] -> [N, Hs, Ws, C]: sum over the destination pixels that read each source pixel."""
    N, H, W, C = dbig.shape
    ih, iw = nearest_index(H, Hs, dbig.device), nearest_index(W, Ws, dbig.device)
    rows = torch.zeros((N, Hs, W, C), dtype=dbig.dtype, device=dbig.device).index_add_(1, ih, dbig)
    return torch.zeros((N, Hs, Ws, C), dtype=dbig.dtype, device=dbig.device).index_add_(2, iw, rows)


# ---- Adam (torch.optim.Adam, amsgrad=False, weight_decay=0), gradient scaled by grad_scale (the 1 / world of data parallelism) ---------
def adam_step(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0):
    """Returns (p', m', v', parts): parts holds the magnitudes the test's bound is made of."""
    gg = g * grad_scale
    a, b = beta1 * m, (1 - beta1) * gg
    m1 = a + b
    v1 = beta2 * v + (1 - beta2) * gg * gg
    bc1, bc2 = 1 - beta1**step, 1 - beta2**step
    denom = v1.sqrt() / (bc2**0.5) + eps
    upd = (lr / bc1) * (m1 / denom)
    return p - upd, m1, v1, {'m_terms': a.abs() + b.abs(), 'denom': denom, 'upd': upd, 'lrc': lr / bc1}
