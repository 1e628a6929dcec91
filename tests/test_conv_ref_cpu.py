"""CPU checks of tests/conv_ref.py, the float64 reference and the exact data sets that tests/test_conv_fp64_gpu.py pins the convolution
kernels against: every reference function equals F.conv2d / F.conv_transpose2d / torch.autograd in float64 to 1e-12 relative on the
shapes used there; the dense and the impulse data are exact in fp32 in ANY summation order (shown by evaluating them forward, reversed
and pairwise in fp32, and by the bound sum |term| 2^5 < 2^24 that covers every other order); operands and, where claimed, results are
representable in bf16 / fp16; the Winograd transforms B^T d B, G g G^T, A^T M A are exact on this data in fp32 emulation."""
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R

REL = 1e-12


def rnd64(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def close(got, ref):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert float((got - ref).abs().max()) <= REL * float(ref.abs().max()), float((got - ref).abs().max())


ALL_CONV = R.FWD_CASES + R.SPLITK_CASES


@pytest.mark.parametrize('case', ALL_CONV)
def test_conv2d_and_its_gradients_equal_autograd(case):
    N, Ci, Co, k, s, p, H, W = case
    x = rnd64(N, Ci, H, W, seed=1).requires_grad_(True)
    w = rnd64(Co, Ci, k, k, seed=2).requires_grad_(True)
    b = rnd64(Co, seed=3)
    y = F.conv2d(x, w, b, s, p)
    close(R.conv2d(x.detach(), w.detach(), b, s, p), y.detach())
    close(R.conv2d(x.detach(), w.detach(), None, s, p), F.conv2d(x, w, None, s, p).detach())
    dy = rnd64(*y.shape, seed=4)
    dx, dw = torch.autograd.grad(y, (x, w), dy)
    close(R.conv2d_dgrad(dy, w.detach(), s, p, H, W), dx)
    close(R.conv2d_wgrad(x.detach(), dy, k, k, s, p), dw)
    base = rnd64(*y.shape, seed=5)
    close(R.accumulate(base, R.conv2d(x.detach(), w.detach(), None, s, p)), base + F.conv2d(x, w, None, s, p).detach())


CONVT = [R.CONVT2 + (2, 2, 0)] + [R.CONVT_GENERAL_SHAPE + c for c in R.CONVT_GENERAL]


@pytest.mark.parametrize('case', CONVT)
def test_conv_transpose_and_its_gradients_equal_autograd(case):
    N, Ci, Co, H, W, f, k, pad = case
    x = rnd64(N, Ci, H, W, seed=1).requires_grad_(True)
    w = rnd64(Ci, Co, k, k, seed=2).requires_grad_(True)
    b = rnd64(Co, seed=3)
    y = F.conv_transpose2d(x, w, b, f, pad)
    close(R.conv_transpose2d(x.detach(), w.detach(), b, f, pad), y.detach())
    dy = rnd64(*y.shape, seed=4)
    dx, dw = torch.autograd.grad(y, (x, w), dy)
    # the gradients of a transposed conv are a forward conv of dy and the weight gradient with the roles of x and dy swapped
    close(R.conv2d(dy, w.detach(), None, f, pad), dx)
    close(R.conv2d_wgrad(dy, x.detach(), k, k, f, pad), dw)
    base = rnd64(*y.shape, seed=5)
    close(R.accumulate(base, R.conv_transpose2d(x.detach(), w.detach(), None, f, pad)), base + F.conv_transpose2d(x, w, None, f, pad).detach())


def test_bf16_rounding_is_to_nearest_even():
    t = torch.randn(1 << 16, generator=torch.Generator().manual_seed(0))
    assert torch.equal(R.bf16_rne(t), t.to(torch.bfloat16).float())
    ties = torch.tensor([1 + 2.0**-8, 1 + 3 * 2.0**-8, -(1 + 2.0**-8), 2.0**-8 + 2.0**-16])  # halfway cases go to the even neighbour
    assert R.bf16_rne(ties).tolist() == [1.0, 1 + 2.0**-6, -1.0, 2.0**-8]


def exact_in_fp32(x, w, s, p):
    """The convolution of this data is exact in fp32 whatever the order of its K products: three orders evaluated, all orders bounded."""
    ref = R.conv2d(x, w, None, s, p)
    cols, wk = R.conv_terms(x, w, s, p)
    sums = R.fp32_sums(cols, wk).double()
    flat = ref.permute(0, 2, 3, 1).reshape(-1, ref.shape[1])
    for name, got in zip(('forward', 'reversed', 'pairwise'), sums):
        assert torch.equal(got, flat), name
    return ref


@pytest.mark.parametrize('case', ALL_CONV)
def test_dense_data_is_exact_in_every_summation_order(case):
    N, Ci, Co, k, s, p, H, W = case
    x, w, b = R.dense_x((N, Ci, H, W), 11), R.dense_w((Co, Ci, k, k), 12), R.dense_bias(Co, 13)
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        assert R.representable(x, dt) and R.representable(w, dt) and R.representable(b, dt)
    assert torch.equal(x * 4, (x * 4).round()) and torch.equal(w * 8, (w * 8).round()) and torch.equal(b * 32, (b * 32).round())
    # every term is a multiple of 2^-5; with sum |term| 2^5 (+ the bias and a base of the accumulate form, <= 1 each) far below 2^24 every
    # partial sum of every order is an integer multiple of 2^-5 below 2^19: a float32
    assert (R.abs_sum_bound(x, w, s, p) + 2) * 2**5 < 2**20
    assert Ci * k * k * 2**5 < 2**20  # ... and so it is for ANY data of these ranges at these K
    if Ci * k * k <= 4608:
        exact_in_fp32(x, w, s, p)
    # the gradients: dy from the same set as x; their terms are multiples of 2^-5 (data) and 2^-4 (weights) under the same bounds
    Ho, Wo = R.out_size(H, k, s, p), R.out_size(W, k, s, p)
    dy = R.dense_x((N, Co, Ho, Wo), 14)
    assert (float(R.conv2d_dgrad(dy.abs(), w.abs(), s, p, H, W).max()) + 2) * 2**5 < 2**20
    assert float(R.conv2d_wgrad(x.abs(), dy.abs(), k, k, s, p).max()) * 2**4 < 2**20


@pytest.mark.parametrize('case', CONVT)
def test_dense_transposed_data_is_exact(case):
    N, Ci, Co, H, W, f, k, pad = case
    x, w = R.dense_x((N, Ci, H, W), 11), R.dense_w((Ci, Co, k, k), 12)
    assert (float(R.conv_transpose2d(x.abs(), w.abs(), None, f, pad).max()) + 2) * 2**5 < 2**20


def impulse_cases():
    for case in R.FWD_CASES:
        yield case
    for case in R.SPLITK_CASES:
        yield case


@pytest.mark.parametrize('case', list(impulse_cases()))
@pytest.mark.parametrize('two', [True, False])
def test_impulse_data_is_exact_and_where_claimed_representable_in_16_bits(case, two):
    N, Ci, Co, k, s, p, H, W = case
    Ho, Wo = R.out_size(H, k, s, p), R.out_size(W, k, s, p)
    w = R.distinct_w(Co, Ci, k, k)
    assert float(w.abs().max()) <= 127 / 128 and torch.equal(w * 128 % 2, torch.ones_like(w))
    for dt in (torch.bfloat16, torch.float16):
        assert R.representable(w, dt)
    # distinct within every window of 128 consecutive (co, ci, tap) indices
    flat = w.reshape(-1)
    for i0 in (0, 77, flat.numel() - 128):
        assert flat[i0:i0 + 128].unique().numel() == 128
    pts = R.seam_pixels(N, H, W, Ho, Wo, s)
    assert {(0, 0, 0), (0, H - 1, W - 1), (N - 1, 0, 0), (N - 1, H - 1, W - 1)} <= set(pts)
    if s == 2:
        assert {(h % 2, w_ % 2) for (_, h, w_) in pts} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    maps = R.impulse_maps(N, Ci, H, W, pts, k, two_channels=two)
    assert sum(int((m_.abs().sum(1) > 0).sum()) for m_ in maps) == len(pts)  # every seam pixel in exactly one map
    last = 0
    for x in maps:
        assert set(x.unique().tolist()) <= {0.0, 1.0, -2.0, 0.5}
        last += int((x[:, Ci - 1] != 0).sum())
        assert int((x != 0).sum(1).max()) <= (2 if two else 1)
        ref = R.conv2d(x, w, None, s, p)
        # at most one impulse pixel under any window: each output is one term, or two with two channels
        assert float(R.conv2d((x != 0).double().amax(1, keepdim=True), torch.ones(1, 1, k, k, dtype=torch.float64), None, s, p).max()) <= 1
        assert R.representable(ref, torch.float32)
        if not two:
            assert R.representable(ref, torch.bfloat16) and R.representable(ref, torch.float16)
        if Ci * k * k <= 2304 and x is maps[0]:
            exact_in_fp32(x, w, s, p)
    assert last > 0  # the last real channel carries impulses


@pytest.mark.parametrize('case', R.WINOGRAD_CASES + R.WINOGRAD_SEAM_CASES)
@pytest.mark.parametrize('data', ['dense', 'impulses'])
def test_winograd_transforms_are_exact_in_fp32_on_the_exact_data(case, data):
    """Every stage of F(2x2, 3x3) evaluated in float32 — V = B^T d B, U = G g G^T, M = sum_ci U V, y = A^T M A — equals the same stage in
    float64, and y equals the direct reference: no fp32 Winograd kernel, whatever its summation order over the channels (all partial
    sums lie on the grid of the terms and below 2^24 of it), is entitled to differ from the direct float64 result on this data."""
    N, Ci, Co, H, W = case
    if data == 'dense':
        x, w = R.dense_x((N, Ci, H, W), 21), R.dense_w((Co, Ci, 3, 3), 22, winograd=True)
        assert torch.equal(w * 2, (w * 2).round())
        grid = 2.0**-5  # V on 2^-2, U on 2^-3
    else:
        pts = R.winograd_seams(N, H, W)
        (x, ) = R.impulse_maps(N, Ci, H, W, pts, 0)
        w = R.distinct_w(Co, Ci, 3, 3)
        grid = 2.0**-10  # V on 2^-1, U on 2^-9
        if H > 8 and W > 16:
            assert {(0, 7, 15), (0, 7, 16), (0, 8, 15), (0, 8, 16)} <= set(pts)
        assert (0, H - 1, W - 1) in pts and (N - 1, H - 1, 0) in pts
    b = R.dense_bias(Co, 23)
    got = R.winograd_fp32(x, w, b)
    ref = R.winograd_fp64(x, w, b)
    for name, g, r in zip(('y', 'V', 'U', 'M'), got, ref):
        assert torch.equal(g.double(), r), name
    assert torch.equal(ref[0], R.conv2d(x, w, b, 1, 1))
    # any order of the channel sum: sum |U| |V| over the channels, on the grid, stays far below 2^24 grid steps (A^T . A adds 16 of them)
    _, V, U, _ = ref
    bound = 16 * float(torch.einsum('ocij,nchwij->nohwij', U.abs(), V.abs()).max()) + 2
    assert bound / grid < 2**22
    # the weight gradient's transforms (A dy A^T on 2^-2 data, G^T . G with entries 1 and 1/2) obey the same argument with grid 2^-6
    dy = R.dense_x((N, Co, H, W), 24)
    assert float(R.conv2d_wgrad(x.abs(), dy.abs(), 3, 3, 1, 1).max()) * 16 * 2**12 < 2**40  # (the slab reduction runs in float64)


def test_winograd_seams_name_the_32_tile_groups():
    pts = R.winograd_seams(3, 20, 20)  # 100 tiles per image, 300 in the batch: groups end at tiles 31, 63, ...
    assert (0, 2 * (31 // 10), 2 * (31 % 10)) in pts and (0, 2 * (32 // 10), 2 * (32 % 10)) in pts
    assert (2, 2 * (88 // 10), 2 * (88 % 10)) in pts  # tile 288 = 9 * 32 is tile 88 of the last image
    assert (0, 8, 8) in R.winograd_seams(1, 10, 9)  # 25 tiles: one partial group, its last tile
