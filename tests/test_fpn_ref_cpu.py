"""CPU: tests/fpn_ref.py is right (against F.interpolate, F.conv2d, F.conv_transpose2d and autograd in float64), its forms agree exactly on
dyadic data, the data sets of tests/test_fpn_fp64_gpu.py are exact in fp32 in any summation order, and those data sets tell a reference
with one fault in it — a dropped tap, a class whose vertical origin is off by one, a block stored across the row-tile boundary — from the
right one."""
import functools

import pytest
import torch
import torch.nn.functional as F

import conv_ref as R
import fpn_ref as P

SMALL = (2, 16, 24, 4, 8)  # N, H, W, Cg, Co: the reference's own checks
RAGGED = (3, 56, 64, 16, 128)  # the first shape of the GPU module: 168 blocks, a row-tile boundary inside image 2


def rand64(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def random_operands(shape, seed=0):
    N, H, W, Cg, Co = shape
    ps = [rand64(N, Cg, H >> g, W >> g, seed=seed + g) for g in range(4)]
    return ps, rand64(Co, 4 * Cg, 3, 3, seed=seed + 4), rand64(Co, seed=seed + 5), rand64(N, Co, H, W, seed=seed + 6)


def close(a, b):
    return float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


# ---- the reference against torch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f', [1, 2, 4, 8])
def test_upsample_and_its_adjoint_against_torch(f):
    x = rand64(2, 3, 5, 7, seed=f).requires_grad_(True)
    up = F.interpolate(x, scale_factor=f, mode='nearest')
    assert torch.equal(P.upsample(x.detach(), f), up.detach())
    d = rand64(*up.shape, seed=f + 10)
    assert close(P.upsample_adjoint(d, f), torch.autograd.grad(up, x, d)[0])


def test_concat_conv_and_gradients_against_torch():
    N, H, W, Cg, Co = SMALL
    ps, w, b, dy = random_operands(SMALL)
    pg = [p.clone().requires_grad_(True) for p in ps]
    wg = w.clone().requires_grad_(True)
    cat = torch.cat([pg[0]] + [F.interpolate(pg[g], size=(H, W)) for g in range(1, 4)], 1)
    y = F.conv2d(cat, wg, b, 1, 1)
    grads = torch.autograd.grad(y, pg + [wg], dy)
    assert torch.equal(P.concat(ps), cat.detach())
    assert close(P.concat_conv(ps, w, b), y.detach())
    assert close(P.classwise_conv(ps, w, b, Cg), y.detach())
    for g, d in enumerate(P.concat_dgrad(dy, w, Cg)):
        assert close(d, grads[g]), g
    assert close(P.concat_wgrad(ps, dy), grads[4])


def test_combine_and_scatter_against_torch():
    """combine: the concat conv equals the sum of F.conv_transpose2d with the combined filters; scatter: autograd of <combine(w), T>."""
    N, H, W, Cg, Co = SMALL
    ps, w, b, _ = random_operands(SMALL, seed=20)
    wcs = [P.combine(w, g, Cg) for g in range(4)]
    y = b.view(1, Co, 1, 1) + sum(F.conv_transpose2d(ps[g], wcs[g], None, 1 << g, 1) for g in range(4))
    assert close(y, F.conv2d(P.concat(ps), w, b, 1, 1))
    assert close(P.transposed_sum(ps, wcs, b), y)
    ts = [rand64(Cg, Co, (1 << g) + 2, (1 << g) + 2, seed=30 + g) for g in range(4)]
    wg = w.clone().requires_grad_(True)
    s = sum((P.combine(wg, g, Cg) * ts[g]).sum() for g in range(4))
    assert close(P.scatter(ts, Co, Cg), torch.autograd.grad(s, wg)[0])


# ---- identities, exactly on dyadic data ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense(shape):
    ps, w, b = P.dense_operands(shape)
    N, H, W, Cg, Co = shape
    return ps, w, b, [P.combine(w, g, Cg) for g in range(4)], P.concat_conv(ps, w, b)


def test_forms_agree_exactly_on_dyadic_data():
    N, H, W, Cg, Co = shape = (2, 16, 24, 16, 128)
    ps, w, b, wcs, y = dense(shape)
    assert torch.equal(P.transposed_sum(ps, wcs, b), y)
    assert torch.equal(P.classwise_conv(ps, w, b, Cg), y)
    ts = [R.dense_x((Cg, Co, (1 << g) + 2, (1 << g) + 2), 40 + g) for g in range(4)]
    assert float(sum((wcs[g] * ts[g]).sum() for g in range(4))) == float((w * P.scatter(ts, Co, Cg)).sum())
    dy = R.dense_x((N, Co, H, W), 50)
    dps = P.concat_dgrad(dy, w, Cg)
    dw = P.concat_wgrad(ps, dy)
    for g in range(4):  # the per-level gradients are those of a (f + 2) x (f + 2) / stride-f / pad-1 conv with the combined weights
        assert torch.equal(R.conv2d(dy, wcs[g], None, 1 << g, 1), dps[g]), g
    assert torch.equal(P.scatter([R.conv2d_wgrad(dy, ps[g], (1 << g) + 2, (1 << g) + 2, 1 << g, 1) for g in range(4)], Co, Cg), dw)


# ---- exactness of the data ----------------------------------------------------------------------------------------------------------
def test_dense_set_is_exact_in_fp32_in_any_order():
    """fp32 F.conv2d, an fp32 emulation that adds the 9 x 4 Cg terms in reverse order and float64 give the same numbers; the combined weights
    are bf16-representable; every output is fp16-representable (bf16: most of them — the 16-bit storage tests round the reference once)."""
    N, H, W, Cg, Co = RAGGED
    ps, w, b, wcs, y = dense(RAGGED)
    cat = P.concat(ps)
    assert torch.equal(F.conv2d(cat.float(), w.float(), b.float(), 1, 1).double(), y)
    cols, wk = R.conv_terms(cat, w, 1, 1)
    rev = torch.zeros((cols.shape[0], Co), dtype=torch.float32)
    for k in reversed(range(cols.shape[1])):
        rev += cols[:, k, None] * wk[None, k]
    rev = (rev + b.float()).reshape(N, H, W, Co).permute(0, 3, 1, 2)
    assert torch.equal(rev.double(), y)
    assert R.abs_sum_bound(cat, w, 1, 1) + 1 < 2.0**24 / 32  # every partial sum is a multiple of 2^-5 below 2^19
    for g in range(4):
        assert R.representable(wcs[g], torch.bfloat16), g
    assert R.representable(y, torch.float16)
    print('dense outputs exact in bf16: %.1f %%' % (100 * float((y.bfloat16().double() == y).double().mean())))


def test_combined_distinct_weights_need_the_rounded_reference():
    """distinct_w combined is exact in fp32 and fp16 but, from level 2 on (sums of up to 9 odd multiples of 1 / 128: 11 bits; levels 0 and 1
    add 1, 2 or 4 of them: 8 bits), not in bf16: in the bf16 modes the reference takes bf16_rne(combine(w)) per level."""
    w = R.distinct_w(128, 64, 3, 3)
    for g in range(4):
        wc = P.combine(w, g, 16)
        assert R.representable(wc, torch.float32) and R.representable(wc, torch.float16)
        assert R.representable(wc, torch.bfloat16) == (g < 2)
        assert torch.equal(R.bf16_rne(wc.float()).double(), wc.bfloat16().double())


def test_grid_weights_combine_exactly_in_fp32():
    w = P.grid_w((128, 64, 3, 3), 7)
    assert float(w.abs().max()) <= 2.0**-3 and torch.equal((w * 1024).round(), w * 1024)
    for g in range(4):
        wc = P.combine(w, g, 16)
        assert torch.equal((wc * 1024).round(), wc * 1024) and float(wc.abs().max()) < 2.0  # multiples of 2^-10 below 2: 11 bits
        assert torch.equal(P.combine(w.float(), g, 16).double(), wc)
        assert torch.equal(P.combine(w.float().flip(2, 3), g, 16).double(), P.combine(w.flip(2, 3), g, 16))  # (another order of the taps)


# ---- teeth --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seam(g):
    return P.seam_levels(RAGGED, g)


def test_seam_sources_hold_every_seam():
    N, H, W, Cg, Co = RAGGED
    for g in range(4):
        pts = set(P.seam_sources(N, H, W, g))
        Hg, Wg = H >> g, W >> g
        for n in range(N):
            assert {(n, 0, 0), (n, 0, Wg - 1), (n, Hg - 1, 0), (n, Hg - 1, Wg - 1)} <= pts
        for m in (127, 128, 167):
            n, hb, wb = P.block_of(N, H, W, m)
            assert (n, (8 * hb) >> g, (8 * wb) >> g) in pts and (n, (8 * hb + 7) >> g, (8 * wb + 7) >> g) in pts
        assert all(0 <= h < Hg and 0 <= w < Wg and 0 <= n < N for (n, h, w) in pts)
    assert P.block_of(N, H, W, 127)[0] == P.block_of(N, H, W, 128)[0] == 2  # the tile boundary falls inside image 2
    assert N * (H // 8) * (W // 8) - 128 == 40  # the ragged tile


@pytest.mark.parametrize('g', range(4))
def test_a_dropped_tap_shows(g):
    """Every (u, v) of every level: the combination without one of its taps changes the result on the seam set and on the dense set."""
    N, H, W, Cg, Co = RAGGED
    w = R.distinct_w(Co, 4 * Cg, 3, 3)
    wd = dense(RAGGED)[1]
    f, k = 1 << g, (1 << g) + 2
    for ps, ww in ((seam(g), w), (dense(RAGGED)[0], wd)):
        full = P.combine(ww, g, Cg)
        for u in range(k):
            for v in range(k):
                delta = full - P.combine(ww, g, Cg, drop=(u, v))
                only = torch.zeros_like(delta)
                only[:, :, u, v] = delta[:, :, u, v]
                assert torch.equal(only, delta)
                # its effect on the output: this tap alone, every source pixel to output (hs f - 1 + u, ws f - 1 + v)
                hs = torch.arange(H >> g) * f - 1 + u
                ws = torch.arange(W >> g) * f - 1 + v
                src = ps[g][:, :, (hs >= 0) & (hs < H)][:, :, :, (ws >= 0) & (ws < W)]
                assert bool((torch.einsum('co,nchw->nohw', delta[:, :, u, v], src) != 0).any()), (g, u, v)


@pytest.mark.parametrize('g', range(4))
def test_a_vertical_origin_off_by_one_shows(g):
    """Each of the 64 classes of every level: the walk whose padh is off by one for that class differs on the seam set and on the dense set."""
    N, H, W, Cg, Co = RAGGED
    w = R.distinct_w(Co, 4 * Cg, 3, 3)
    for ps, ww in ((seam(g), w), (dense(RAGGED)[0], dense(RAGGED)[1])):
        for oh0 in range(8):
            for ow0 in range(8):
                good = P.classwise_conv(ps, ww, None, Cg, only=(g, oh0, ow0))
                bad = P.classwise_conv(ps, ww, None, Cg, padh_fault=(g, oh0, ow0), only=(g, oh0, ow0))
                assert not torch.equal(good, bad), (g, oh0, ow0)


@pytest.mark.parametrize('g', range(4))
def test_a_block_stored_across_the_tile_boundary_shows(g):
    N, H, W, Cg, Co = RAGGED
    y = P.concat_conv(seam(g), R.distinct_w(Co, 4 * Cg, 3, 3))
    yd = dense(RAGGED)[4]
    for c in range(64):
        assert not torch.equal(P.displace_block(y, 127, 128, c // 8, c % 8), y), (g, c)
        assert not torch.equal(P.displace_block(yd, 127, 128, c // 8, c % 8), yd), c
