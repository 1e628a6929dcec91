"""tests/head_bn_bwd_ref.py (the float64 yardstick of tests/test_head_bn_bwd_gpu.py) against torch.autograd in float64 on the CPU:
BatchNorm2d (train) -> ReLU -> ConvTranspose2d(64 -> 1, k 2, s 2) -> sigmoid for both branches, the step function on top, and a loss
that is linear in the three maps with the given d(preds) as its coefficients."""
import pytest
import torch
import torch.nn.functional as F

import head_bn_bwd_ref as R

N, HQ, WQ = 2, 5, 7
EPS = 1e-5


def make(seed, CH):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, sc=1.0: torch.randn(*s, generator=g, dtype=torch.float64) * sc
    t = {}
    for br in 'bt':
        t['y' + br] = (r(N, 64, HQ, WQ) * 1.5 + 0.3).requires_grad_()       # NCHW for torch; the reference takes NHWC
        t['gamma' + br] = (r(64, sc=0.3) + 1).requires_grad_()
        t['beta' + br] = r(64, sc=0.5).requires_grad_()
        t['w' + br] = r(64, 1, 2, 2, sc=0.2).requires_grad_()
        t['b6' + br] = r(1, sc=0.1).requires_grad_()
    t['dpreds'] = r(N, CH, 2 * HQ, 2 * WQ, sc=0.1)
    return t


@pytest.mark.parametrize('CH', [3, 2])
def test_head_bn_bwd_reference_matches_autograd(CH):
    kstep, gs = 50.0, 0.7
    t = make(3 + CH, CH)
    logits = {}
    for br in 'bt':
        a = F.batch_norm(t['y' + br], None, None, t['gamma' + br], t['beta' + br], True, 0.1, EPS)
        logits[br] = F.conv_transpose2d(F.relu(a), t['w' + br], t['b6' + br], stride=2)
    P, T = torch.sigmoid(logits['b']), torch.sigmoid(logits['t'])
    maps = [P, T] + ([torch.sigmoid(kstep * (P - T))] if CH == 3 else [])
    preds = torch.cat(maps, 1)
    (preds * t['dpreds']).sum().backward()

    bn = {}
    for br in 'bt':
        y = t['y' + br].detach()
        mean = y.mean((0, 2, 3))
        rstd = 1 / torch.sqrt(y.var((0, 2, 3), unbiased=False) + EPS)
        scale = t['gamma' + br].detach() * rstd
        bn[br] = {'mean': mean, 'rstd': rstd, 'scale': scale, 'shift': t['beta' + br].detach() - mean * scale, 'gamma': t['gamma' + br].detach()}
    nhwc = lambda x: x.detach().permute(0, 2, 3, 1).contiguous()
    rb, rt, _ = R.head_bn_bwd(nhwc(t['yb']), nhwc(t['yt']), t['wb'].detach().reshape(64, 4), t['wt'].detach().reshape(64, 4), preds.detach(),
                              t['dpreds'], bn['b'], bn['t'], N, HQ, WQ, CH, kstep, gs)
    for br, r in (('b', rb), ('t', rt)):
        want = {'dy1': nhwc(t['y' + br].grad).reshape(-1, 64), 'dgamma': t['gamma' + br].grad * gs, 'dbeta': t['beta' + br].grad * gs,
                'dbias3': t['y' + br].grad.sum((0, 2, 3)) * gs, 'dw6': t['w' + br].grad.reshape(64, 4) * gs, 'dbias6': t['b6' + br].grad[0] * gs}
        for k, w in want.items():
            err = float((r[k] - w).abs().max())
            tol = 1e-12 * max(1.0, float(w.abs().max()))
            print('%s %s: max err %.3e (max |ref| %.3e)' % (br, k, err, float(w.abs().max())))
            assert err <= tol, (br, k, err, tol)
