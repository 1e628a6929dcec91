"""float64 references of the 16-bit inference kernels (csrc/stem16.hip, csrc/convt16.hip) and of the forward head tail
(csrc/head_loss.hip head_tail_fwd_kernel), written from the formulas — strided slices, elementwise operations and matmul, no F.conv* —
so that tests/test_infer16_ops_gpu.py can evaluate them on the GPU at the multi-block sizes.  Every tensor is float64 and activations are
NHWC, as the kernels store them.  Beside its value each reference returns the magnitude sum its error bound needs (the same formula on
absolute values).  tests/test_infer16_ref_cpu.py checks this module against torch.nn.functional."""
import torch


def stem_cols(x):
    """x [N, 3, H, W] -> the 7x7 / stride 2 / pad 3 patches [N, Ho, Wo, 147] (column = (ci, r, s)), Ho = (H - 1) // 2 + 1."""
    N, C, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = x.new_zeros(N, C, 2 * Ho + 5, 2 * Wo + 5)
    xp[:, :, 3:H + 3, 3:W + 3] = x
    taps = [xp[:, :, r:r + 2 * Ho:2, s:s + 2 * Wo:2] for r in range(7) for s in range(7)]  # each [N, 3, Ho, Wo]
    return torch.stack(taps, -1).permute(0, 2, 3, 1, 4).reshape(N, Ho, Wo, C * 49)


def stem_conv(x, w):
    """Conv2d(3 -> Co, 7x7, stride 2, pad 3, no bias): x [N, 3, H, W], w [Co, 3, 7, 7] -> y [N, Ho, Wo, Co] and conv(|x|, |w|)."""
    cols = stem_cols(x)
    wm = w.reshape(w.shape[0], -1).t()
    return cols @ wm, cols.abs() @ wm.abs()


def conv_transpose2x2(x, w, bias=None):
    """ConvTranspose2d(Ci -> Co, 2x2, stride 2): x [N, H, W, Ci], w [Ci, Co, 2, 2], out[n, 2h + a, 2w + b, co] = bias[co] +
    sum_ci x[n, h, w, ci] w[ci, co, a, b] -> y [N, 2H, 2W, Co] and |bias| + sum |x| |w|."""
    N, H, W, Ci = x.shape
    Co = w.shape[1]
    wm = w.permute(0, 2, 3, 1).reshape(Ci, 4 * Co)  # column = (a, b, co)

    def run(xx, ww, bb):
        y = xx.reshape(-1, Ci) @ ww
        if bb is not None:
            y = y + bb.repeat(4)
        return y.reshape(N, H, W, 2, 2, Co).permute(0, 1, 3, 2, 4, 5).reshape(N, 2 * H, 2 * W, Co)

    return run(x, wm, bias), run(x.abs(), wm.abs(), None if bias is None else bias.abs())


def pointwise(x, w, bias=None, relu=False):
    """Conv2d(Ci -> Co, 1x1) + bias [+ ReLU]: x [..., Ci], w [Co, Ci] -> y [..., Co] and |bias| + sum |x| |w| (of the value before the ReLU)."""
    y, mag = x @ w.t(), x.abs() @ w.abs().t()
    if bias is not None:
        y, mag = y + bias, mag + bias.abs()
    return (y.clamp_min(0) if relu else y), mag


def affine_relu(y, scale, shift):
    """relu(y scale + shift) over the last (channel) dimension, and |y scale| + |shift|."""
    return (y * scale + shift).clamp_min(0), (y * scale).abs() + shift.abs()


def maxpool3x3s2p1(z, pad=float('-inf')):
    """MaxPool2d(3, 2, 1) of z [N, H, W, C] -> [N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C]; positions outside the map hold `pad`."""
    N, H, W, C = z.shape
    Hq, Wq = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    zp = z.new_full((N, 2 * Hq + 1, 2 * Wq + 1, C), pad)
    zp[:, 1:H + 1, 1:W + 1] = z
    out = None
    for r in range(3):
        for s in range(3):
            t = zp[:, r:r + 2 * Hq:2, s:s + 2 * Wq:2]
            out = t if out is None else torch.maximum(out, t)
    return out.contiguous()


def bn_stats(y, gamma, beta, eps, momentum, run_mean=None, run_var=None):
    """Train-mode BatchNorm statistics of y [M, C] (every leading dimension flattened): mean, biased variance `var`, `unbiased`
    = var M / (M - 1), rstd = 1 / sqrt(var + eps), scale = gamma rstd, shift = beta - mean scale, and the running update
    (1 - momentum) old + momentum new (new variance: the unbiased one)."""
    y = y.reshape(-1, y.shape[-1])
    M = y.shape[0]
    mean = y.mean(0)
    var = ((y - mean)**2).mean(0)
    r = {'mean': mean, 'var': var, 'unbiased': var * (M / (M - 1.0)) if M > 1 else var, 'rstd': 1.0 / torch.sqrt(var + eps)}
    r['scale'] = gamma * r['rstd']
    r['shift'] = beta - mean * r['scale']
    if run_mean is not None:
        r['run_mean'] = (1 - momentum) * run_mean + momentum * mean
        r['run_var'] = (1 - momentum) * run_var + momentum * r['unbiased']
    return r


def head_chain(x, w1, bias1, scale, shift, w2, bias2):
    """One branch of the DB head's tail up to the logits: ConvTranspose2d(64, 64, 2, 2) + bias1 -> eval-mode BatchNorm (scale, shift) ->
    ReLU -> ConvTranspose2d(64, 1, 2, 2) + bias2.  x [N, Hq, Wq, 64], w1 [64, 64, 2, 2], w2 [64, 1, 2, 2], bias2 [1].
    Returns a dict: logit [N, 4Hq, 4Wq]; c1 the first ConvT [N, 2Hq, 2Wq, 64] and its magnitude sum mag1; z the activation between the
    two ConvTs and zmag = |c1 scale| + |shift|."""
    c1, mag1 = conv_transpose2x2(x, w1, bias1)
    z, zmag = affine_relu(c1, scale, shift)
    logit, _ = conv_transpose2x2(z, w2, bias2)
    return {'logit': logit[..., 0], 'c1': c1, 'mag1': mag1, 'z': z, 'zmag': zmag}


def propagate_convt1(e, w2):
    """sum_co e[n, h, w, co] |w2[co, 0, a, b]| on the 2x-upsampled grid: how an elementwise error bound e [N, H, W, 64] of the input of
    ConvTranspose2d(64, 1, 2, 2) reaches its output [N, 2H, 2W]."""
    return conv_transpose2x2(e, w2.abs())[0][..., 0]


def step_map(P, T, kstep):
    """The approximate binary map 1 / (1 + exp(-k (P - T)))."""
    return torch.sigmoid(kstep * (P - T))


def head_tail(xb, xt, wb, wt, bias_b, bias_t, channels, kstep, scale_b=None, shift_b=None, scale_t=None, shift_t=None):
    """The forward head tail: per branch [relu(x scale + shift) ->] ConvTranspose2d(64, 1, 2, 2) + bias -> sigmoid, and (channels = 3)
    B = step_map(P, T).  x* [N, Hq, Wq, 64], w* [64, 1, 2, 2] -> dict: out [N, channels, 2Hq, 2Wq]; per branch br in 'b', 't':
    'logit_' br, 'v_' br (the ConvT's input), 'vmag_' br (|x scale| + |shift|, or |x|) and 'mag_' br = |bias| + sum |v| |w|."""
    r = {}
    for br, x, w, bias, sc, sh in (('b', xb, wb, bias_b, scale_b, shift_b), ('t', xt, wt, bias_t, scale_t, shift_t)):
        v, vmag = (x, x.abs()) if sc is None else affine_relu(x, sc, sh)
        logit, mag = conv_transpose2x2(v, w, bias)
        r['logit_' + br], r['mag_' + br], r['v_' + br], r['vmag_' + br] = logit[..., 0], mag[..., 0], v, vmag
    P, T = torch.sigmoid(r['logit_b']), torch.sigmoid(r['logit_t'])
    r['out'] = torch.stack([P, T] + ([step_map(P, T, kstep)] if channels == 3 else []), 1)
    return r
