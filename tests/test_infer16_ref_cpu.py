"""tests/infer16_ref.py (the float64 references of tests/test_infer16_ops_gpu.py) against torch.nn.functional in float64, at small odd
shapes.  Both sides are float64 sums of the same terms in different orders: they agree to a few float64 roundings of the magnitude sum."""
import pytest
import torch
import torch.nn.functional as F

import infer16_ref as R

EPS64 = 2.0**-52


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def close(got, ref, mag, terms):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert bool(((got - ref).abs() <= 2 * terms * EPS64 * mag + 1e-300).all()), float((got - ref).abs().max())


def to_nchw(t):
    return t.permute(0, 3, 1, 2)


@pytest.mark.parametrize('N,H,W', [(1, 7, 7), (2, 13, 10), (1, 16, 9), (3, 8, 21)])
def test_stem_conv(N, H, W):
    x, w = rnd(N, 3, H, W, seed=1), rnd(5, 3, 7, 7, seed=2)
    y, mag = R.stem_conv(x, w)
    close(to_nchw(y), F.conv2d(x, w, None, 2, 3), to_nchw(mag), 147)
    close(to_nchw(mag), F.conv2d(x.abs(), w.abs(), None, 2, 3), to_nchw(mag), 147)


@pytest.mark.parametrize('Co,with_bias', [(64, True), (6, False), (1, True)])
def test_conv_transpose2x2(Co, with_bias):
    x, w = rnd(2, 3, 5, 64, seed=3), rnd(64, Co, 2, 2, seed=4)
    b = rnd(Co, seed=5) if with_bias else None
    y, mag = R.conv_transpose2x2(x, w, b)
    close(to_nchw(y), F.conv_transpose2d(to_nchw(x), w, b, 2), to_nchw(mag), 65)
    close(to_nchw(mag), F.conv_transpose2d(to_nchw(x).abs(), w.abs(), None if b is None else b.abs(), 2), to_nchw(mag), 65)


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('with_bias', [False, True])
def test_pointwise(relu, with_bias):
    x, w = rnd(2, 3, 5, 64, seed=6), rnd(7, 64, seed=7)
    b = rnd(7, seed=8) if with_bias else None
    y, mag = R.pointwise(x, w, b, relu)
    ref = F.conv2d(to_nchw(x), w.view(7, 64, 1, 1), b)
    close(to_nchw(y), F.relu(ref) if relu else ref, to_nchw(mag), 65)
    close(to_nchw(mag), F.conv2d(to_nchw(x).abs(), w.abs().view(7, 64, 1, 1), None if b is None else b.abs()), to_nchw(mag), 65)


def test_affine_relu():
    y, sc, sh = rnd(2, 3, 4, 8, seed=9), rnd(8, seed=10), rnd(8, seed=11)
    z, mag = R.affine_relu(y, sc, sh)
    assert torch.equal(z, F.relu(y * sc + sh)) and torch.equal(mag, (y * sc).abs() + sh.abs())
    assert bool((z >= 0).all()) and bool((z == 0).any()) and bool((z > 0).any())


@pytest.mark.parametrize('H,W', [(1, 1), (2, 2), (5, 7), (8, 6), (9, 16)])
def test_maxpool(H, W):
    z = rnd(2, H, W, 4, seed=H * 31 + W)
    assert torch.equal(R.maxpool3x3s2p1(z), F.max_pool2d(to_nchw(z), 3, 2, 1).permute(0, 2, 3, 1))
    zz = z.clamp_min(0)  # after a ReLU a zero outside the map is as good as -inf: what the fused stem kernel relies on
    assert torch.equal(R.maxpool3x3s2p1(zz, 0.0), R.maxpool3x3s2p1(zz))


@pytest.mark.parametrize('M', [2, 37])
def test_bn_stats(M):
    C = 6
    y = rnd(M, C, seed=12) * 3 + 5
    gamma, beta, rm, rv = rnd(C, seed=13), rnd(C, seed=14), rnd(C, seed=15), rnd(C, seed=16).abs() + 0.5
    r = R.bn_stats(y.view(1, M, C), gamma, beta, 1e-5, 0.1, rm, rv)
    rm_t, rv_t = rm.clone(), rv.clone()
    out = F.batch_norm(y, rm_t, rv_t, gamma, beta, True, 0.1, 1e-5)
    tol = lambda t: 64 * EPS64 * (t.abs() + 1)
    assert bool(((r['mean'] - y.mean(0)).abs() <= tol(r['mean'])).all())
    assert bool(((r['var'] - y.var(0, unbiased=False)).abs() <= tol(r['var'])).all())
    assert bool(((r['unbiased'] - y.var(0, unbiased=True)).abs() <= tol(r['unbiased'])).all())
    assert bool(((r['run_mean'] - rm_t).abs() <= tol(rm_t)).all()) and bool(((r['run_var'] - rv_t).abs() <= tol(rv_t)).all())
    assert bool(((y * r['scale'] + r['shift'] - out).abs() <= 1e-12 * (out.abs() + 1)).all())
    assert bool(((r['rstd'] - (y.var(0, unbiased=False) + 1e-5).rsqrt()).abs() <= tol(r['rstd'])).all())
    assert 'run_mean' not in R.bn_stats(y, gamma, beta, 1e-5, 0.1)


def head_params(seed):
    w1, b1 = rnd(64, 64, 2, 2, seed=seed) * 0.2, rnd(64, seed=seed + 1) * 0.1
    sc, sh = rnd(64, seed=seed + 2) * 0.3 + 1, rnd(64, seed=seed + 3) * 0.3
    w2, b2 = rnd(64, 1, 2, 2, seed=seed + 4) * 0.2, rnd(1, seed=seed + 5)
    return w1, b1, sc, sh, w2, b2


def test_head_chain():
    x = rnd(2, 3, 5, 64, seed=20)
    w1, b1, sc, sh, w2, b2 = head_params(21)
    r = R.head_chain(x, w1, b1, sc, sh, w2, b2)
    c1 = F.conv_transpose2d(to_nchw(x), w1, b1, 2)
    z = F.relu(c1 * sc.view(1, 64, 1, 1) + sh.view(1, 64, 1, 1))
    logit = F.conv_transpose2d(z, w2, b2, 2)[:, 0]
    assert r['logit'].shape == (2, 12, 20)
    assert bool(((r['logit'] - logit).abs() <= 1e-12).all()) and bool(((to_nchw(r['z']) - z).abs() <= 1e-12).all())
    e = rnd(2, 6, 10, 64, seed=22).abs()
    close(R.propagate_convt1(e, w2), F.conv_transpose2d(to_nchw(e), w2.abs(), None, 2)[:, 0], R.propagate_convt1(e, w2), 65)


@pytest.mark.parametrize('channels', [2, 3])
@pytest.mark.parametrize('bn', [False, True])
def test_head_tail(channels, bn):
    N, Hq, Wq = 2, 3, 5
    xb, xt = rnd(N, Hq, Wq, 64, seed=30), rnd(N, Hq, Wq, 64, seed=31)
    _, _, scb, shb, wb, bb = head_params(32)
    _, _, sct, sht, wt, bt = head_params(40)
    kw = dict(scale_b=scb, shift_b=shb, scale_t=sct, shift_t=sht) if bn else {}
    r = R.head_tail(xb, xt, wb, wt, bb, bt, channels, 50.0, **kw)
    act = (lambda x, sc, sh: F.relu(x * sc.view(1, 64, 1, 1) + sh.view(1, 64, 1, 1))) if bn else (lambda x, sc, sh: x)
    P = torch.sigmoid(F.conv_transpose2d(act(to_nchw(xb), scb, shb), wb, bb, 2))
    T = torch.sigmoid(F.conv_transpose2d(act(to_nchw(xt), sct, sht), wt, bt, 2))
    ref = torch.cat([P, T] + ([1 / (1 + torch.exp(-50.0 * (P - T)))] if channels == 3 else []), 1)
    assert r['out'].shape == (N, channels, 2 * Hq, 2 * Wq)
    # (the step function multiplies the float64 roundoff of P - T by k / 4)
    assert bool(((r['out'] - ref).abs() <= 1e-11).all()), float((r['out'] - ref).abs().max())
    mag = F.conv_transpose2d(act(to_nchw(xb), scb, shb).abs(), wb.abs(), bb.abs(), 2)[:, 0]
    close(r['mag_b'], mag, mag, 65)
