"""The float64 references of tests/bn_pool_ref.py against torch itself in float64 (F.batch_norm, torch.autograd, F.max_pool2d,
F.interpolate) and oracle.AdamState, at small shapes, without a GPU: a wrong reference cannot make a GPU test pass.
Agreement is asked to 1e-12 relative to the largest magnitude (two float64 evaluations in different orders), index results exactly."""
import pytest
import torch
import torch.nn.functional as F

import bn_pool_ref as R
from oracle import dbnet_oracle as O


def close(tag, got, ref, rel=1e-12):
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    err = float((got - ref).abs().max()) if got.numel() else 0.0
    lim = rel * max(float(ref.abs().max()) if ref.numel() else 0.0, 1.0)
    assert err <= lim, '%s: max err %.3e > %.3e' % (tag, err, lim)


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def to_nchw(t, N, H, W):
    return t.reshape(N, H, W, -1).permute(0, 3, 1, 2).contiguous()


def to_rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


@pytest.mark.parametrize('N,H,W,C', [(1, 1, 1, 4), (1, 2, 1, 8), (2, 3, 5, 20), (3, 4, 4, 48)])
def test_batchnorm_statistics_and_running_statistics(N, H, W, C):
    M = N * H * W
    x = rnd(M, C, seed=1) * 3 + rnd(C, seed=2) * 8
    gamma, beta = rnd(C, seed=3), rnd(C, seed=4)
    rm, rv = rnd(C, seed=5), rnd(C, seed=6).abs() + 0.5
    got = R.bn_stats(x, gamma, beta, 1e-5, 0.1, rm, rv)
    rm_t, rv_t = rm.clone(), rv.clone()
    if M > 1:  # (F.batch_norm refuses a single value per channel in training mode)
        out = F.batch_norm(to_nchw(x, N, H, W), rm_t, rv_t, gamma, beta, True, 0.1, 1e-5)
        close('normalised', to_nchw(R.bn_apply(x, got['scale'], got['shift']), N, H, W), out, 1e-10)
        close('running_mean', got['run_mean'], rm_t)
        close('running_var', got['run_var'], rv_t)
        close('var', got['var'], x.var(0, unbiased=False))
    else:
        assert float(got['var'].abs().max()) == 0.0 and torch.equal(got['unbiased'], got['var'])
        close('running_var at M = 1', got['run_var'], 0.9 * rv)
        close('rstd at var = 0', got['rstd'], torch.full((C, ), 1e-5, dtype=torch.float64).rsqrt())
    close('mean', got['mean'], x.mean(0))
    close('rstd', got['rstd'], 1 / torch.sqrt(got['var'] + 1e-5))
    close('shift', got['shift'], beta - got['mean'] * gamma * got['rstd'])


def test_batchnorm_apply_forms():
    M, C = 17, 12
    y, res = rnd(M, C, seed=1), rnd(M, C, seed=2)
    sc, sh, rsc, rsh = (rnd(C, seed=s) for s in (3, 4, 5, 6))
    close('plain', R.bn_apply(y, sc, sh), y * sc + sh)
    close('relu', R.bn_apply(y, sc, sh, relu=True), F.relu(y * sc + sh))
    close('res relu', R.bn_apply(y, sc, sh, res, relu=True), F.relu(y * sc + sh + res))
    close('res affine', R.bn_apply(y, sc, sh, res, rsc, rsh), y * sc + sh + res * rsc + rsh)


@pytest.mark.parametrize('mask_form', ['zmask', 'recomputed', 'none'])
@pytest.mark.parametrize('N,H,W,C', [(1, 2, 1, 8), (2, 3, 5, 20), (3, 4, 4, 48)])
def test_batchnorm_backward_against_autograd(N, H, W, C, mask_form):
    M = N * H * W
    x = (rnd(M, C, seed=1) * 2 + 3).requires_grad_(True)
    gamma, beta = (rnd(C, seed=2) * 0.3 + 1).requires_grad_(True), rnd(C, seed=3).requires_grad_(True)
    ybn = F.batch_norm(to_nchw(x, N, H, W), None, None, gamma, beta, True, 0.1, 1e-5)
    z = ybn if mask_form == 'none' else F.relu(ybn)
    dout = rnd(M, C, seed=4)
    dx, dg, db = torch.autograd.grad(z, (x, gamma, beta), to_nchw(dout, N, H, W))
    xd = x.detach()
    st = R.bn_stats(xd, gamma.detach(), beta.detach(), 1e-5)
    if mask_form == 'zmask':
        mask = R.bn_mask(xd, zmask=to_rows(z.detach()))
    elif mask_form == 'recomputed':
        mask = R.bn_mask(xd, mask_scale=st['scale'], mask_shift=st['shift'])
    else:
        mask = R.bn_mask(xd)
    got = R.bn_backward(xd, dout, st['mean'], st['rstd'], gamma.detach(), mask, grad_scale=0.5)
    close('dy', got['dy'], dx, 1e-10)
    close('dgamma', got['dgamma'], 0.5 * dg, 1e-10)
    close('dbeta', got['dbeta'], 0.5 * db, 1e-10)
    close('c1', got['c1'], got['g'].mean(0))
    close('abs2', got['abs2'], (got['g'] * got['xhat']).abs().sum(0))


@pytest.mark.parametrize('N,H,W', [(1, 1, 1), (2, 2, 1), (1, 1, 9), (1, 7, 9), (3, 16, 12), (2, 9, 14)])
@pytest.mark.parametrize('ties', [False, True])
def test_maxpool_over_relu_affine(N, H, W, ties):
    C = 8
    y = rnd(N, H, W, C, seed=H * 31 + W)
    if ties:
        y = torch.round(y * 2) / 2
    sc, sh = rnd(C, seed=2) * 0.5 + 1, rnd(C, seed=3) * 0.3
    if ties:
        sc, sh = torch.round(sc * 2) / 2 + 0.5, torch.round(sh * 2) / 2
        sc[::3] = -sc[::3]
    z = R.bn_apply(y, sc, sh, relu=True)
    zt = to_nchw(z, N, H, W).requires_grad_(True)
    pool_t, idx_t = F.max_pool2d(zt, 3, 2, 1, return_indices=True)
    pooled = R.pool_fwd(z)
    assert pooled.shape == (N, R.pool_out(H), R.pool_out(W), C)
    assert torch.equal(to_nchw(pooled, N, pooled.shape[1], pooled.shape[2]), pool_t.detach())
    dp = rnd(*pooled.shape, seed=5)
    dz_t, = torch.autograd.grad(pool_t, zt, to_nchw(dp, N, pooled.shape[1], pooled.shape[2]))
    dz_t = dz_t * (zt.detach() > 0)
    # first-maximum routing (nn.MaxPool2d): the codes name torch's own argmax wherever the maximum is positive
    codes = R.pool_first_argmax(z)
    Ho, Wo = pooled.shape[1:3]
    oh, ow = torch.arange(Ho).view(1, Ho, 1, 1), torch.arange(Wo).view(1, 1, Wo, 1)
    flat = (2 * oh - 1 + codes // 3) * W + (2 * ow - 1 + codes % 3)
    live = codes != 15
    assert torch.equal(live, pooled > 0)
    assert torch.equal(flat[live], to_rows(idx_t).reshape(N, Ho, Wo, C)[live])
    close('first-argmax backward', to_nchw(R.pool_bwd_from_codes(codes, dp, H, W), N, H, W), dz_t)
    close('gather by codes', R.pool_gather_codes(z, codes), pooled * live)
    if not ties:
        close('all-ties backward (no ties)', to_nchw(R.pool_bwd_all_ties(z, pooled, dp), N, H, W), dz_t)
    else:  # every tying position receives the gradient: the column sums count each window once per tie
        zw = R._windows(z, -1.0)
        nt = ((zw == pooled.unsqueeze(0)) & (zw > 0)).sum(0)
        close('all-ties column sums', R.pool_bwd_all_ties(z, pooled, dp).sum((0, 1, 2)), (dp * nt).sum((0, 1, 2)))
        assert H * W < 9 or int(nt.max()) > 1  # (the data does hold ties)


@pytest.mark.parametrize('hs,ws,h,w', [(4, 4, 8, 8), (2, 3, 8, 12), (1, 1, 8, 8), (3, 5, 7, 9), (8, 8, 8, 8)])
def test_nearest_upsample_add_concat_adjoint(hs, ws, h, w):
    N, C = 2, 6
    a = rnd(N, hs, ws, C, seed=1)
    at = to_nchw(a, N, hs, ws).requires_grad_(True)
    up_t = F.interpolate(at, size=(h, w))
    assert torch.equal(to_nchw(R.nearest_up(a, h, w), N, h, w), up_t.detach())
    for dt in (torch.float32, torch.float64):  # the index rule in exact integers == torch's float evaluation
        probe = torch.arange(hs * ws, dtype=dt).view(1, 1, hs, ws)
        want = F.interpolate(probe, size=(h, w)).view(h, w).long()
        got = R.nearest_index(h, hs).view(h, 1) * ws + R.nearest_index(w, ws).view(1, w)
        assert torch.equal(got, want)
    dbig = rnd(N, h, w, C, seed=2)
    da_t, = torch.autograd.grad(up_t, at, to_nchw(dbig, N, h, w))
    close('adjoint', to_nchw(R.nearest_up_adjoint(dbig, hs, ws), N, hs, ws), da_t)


@pytest.mark.parametrize('n', [1, 5, 1023])
def test_adam_two_steps_against_the_oracle(n):
    p0, g1, g2 = rnd(n, seed=1), rnd(n, seed=2) * 1e-3, rnd(n, seed=3) * 1e-2
    sd = {'w': p0.clone()}
    opt = O.AdamState(lr=0.005)
    opt.step(sd, {'w': g1.clone()})
    opt.step(sd, {'w': g2.clone()})
    p, m, v = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for i, g in enumerate((g1, g2)):
        p, m, v, _ = R.adam_step(p, g * 4, m, v, 0.005, 0.9, 0.999, 1e-8, i + 1, grad_scale=0.25)  # (the 1 / world path)
    close('params', p, sd['w'])
    close('exp_avg', m, opt.m['w'])
    close('exp_avg_sq', v, opt.v['w'])
    t = torch.nn.Parameter(p0.clone())
    topt = torch.optim.Adam([t], lr=0.005)
    for g in (g1, g2):
        t.grad = g.clone()
        topt.step()
    close('params vs torch.optim.Adam', p, t.detach())
