"""-m gpu: the convolution kernels (direct implicit GEMM in its three matrix modes and on 16-bit storage, split-K, ConvTranspose2d, the
weight gradient, Winograd forward / data gradient / weight gradient) against the float64 reference of tests/conv_ref.py.  The weight-gradient
cases here fit one or two pixel splits; tests/test_wgrad_fp64_gpu.py pins the same entry point with many splits, in the pixel-patch kernel, on
stored-bf16 operands (the "-" of the wgrad rows below) and through the grouped slab reduction.

Three kinds of case per kernel:
  * random data: the kernel's distance to float64 is measured against the distance of plain fp32 (F.conv2d / autograd in fp32 on the CPU,
    same operands) to float64 — rms(got - ref64) <= m rms(ref32 - ref64) and max |got - ref64| <= m max |ref32 - ref64| — on the operands
    as the kernel sees them (ns = 1: rounded to bf16, ties to even; 16-bit storage: rounded to the storage type, with one output rounding
    SR |ref64| + ETA allowed on top).  A kernel whose products carry 16 instead of 24 mantissa bits sits 2^8 / sqrt(K)-fold above fp32
    and fails whatever the flat tolerances of tests/test_ops_gpu.py say;
  * exact dyadic data, dense ({-4..4}/4 times {-8..8}/8, bias on 2^-5) and impulses on the seams of the kernel's walk (first / last pixel of
    every image, both sides of every M-tile boundary, the stride-2 parity classes, the Winograd patch corners and 32-tile groups) under
    weights that differ per (co, ci, tap): equal to float64 BIT FOR BIT in every mode — a property of the data, not of the summation
    order (tests/test_conv_ref_cpu.py shows it), so a dropped, duplicated or misplaced term cannot hide;
  * every output buffer starts as NaN.  Padding channels (Cs > Ci, the stem) hold zeros for the forward kernels: include/dbnet_hip.h
    promises for none of them that padding is not read (the panels carry zero weights for it, and 0 * NaN is NaN).  The weight gradient
    runs with zeros and with NaN there: its reduction drops the columns of the padding channels, so nothing in them may reach the result.

The margins m.  Per mode, m is twice the largest ratio measured on the MI355X over all cases, rounded up to a power of two; the rule caps
it at 16, and every m below is within that cap.  Each random-data test prints one line per launch,
    RATIO <operation> <case> <mode> [tile t | ksplit n | padding v]: rms <ratio> max <ratio> (fp32 itself: rms <abs> max <abs>)
(pytest -rA shows them).  The table holds "rms ratio / max ratio", the worst over the tiles, split counts and padding forms of a row.  On
16-bit storage the ratio is taken after the one output rounding SR |ref64| + ETA is taken off, so most of it is 0.

    operation and case                                         f32        bf16x3          bf16  bf16 storage  fp16 storage      winograd
    fwd (2, 64, 64, 3, 1, 1, 16, 12)                   1.93 / 1.85   1.62 / 1.81   1.39 / 1.83   0.00 / 0.00   0.01 / 0.25             -
    fwd (3, 128, 64, 1, 1, 0, 9, 7)                    0.71 / 0.77   0.58 / 0.53   0.65 / 0.67   0.00 / 0.00   0.00 / 0.02             -
    fwd (1, 64, 128, 3, 2, 1, 18, 14)                  1.75 / 1.98   1.49 / 1.99   1.36 / 1.95   0.00 / 0.00   0.01 / 0.13             -
    fwd (1, 64, 64, 3, 2, 1, 17, 13)                   1.67 / 1.73   1.42 / 2.02   1.35 / 1.07   0.00 / 0.00   0.00 / 0.00             -
    fwd (2, 3, 64, 7, 2, 3, 32, 40)                    0.99 / 1.00   0.95 / 0.71   0.88 / 0.77             -             -             -
    fwd (1, 256, 256, 3, 1, 1, 12, 12)                 3.56 / 6.07   3.10 / 4.43   2.07 / 2.36   0.01 / 0.28   0.04 / 1.16             -
    fwd (1, 512, 512, 3, 1, 1, 2, 2)                   0.58 / 0.73   0.47 / 0.44   0.32 / 0.38   0.00 / 0.00   0.00 / 0.00             -
    fwd (1, 64, 192, 3, 1, 1, 10, 9)                   1.71 / 3.37   1.41 / 1.93   1.26 / 1.46   0.00 / 0.02   0.00 / 0.03             -
    fwd (1, 64, 64, 3, 1, 1, 16, 32)                   1.95 / 2.73   1.65 / 2.43   1.42 / 2.23   0.01 / 0.29   0.00 / 0.09             -
    dgrad (2, 64, 64, 3, 1, 1, 16, 12)                 1.96 / 2.84   1.66 / 2.24   1.49 / 1.66   0.00 / 0.00   0.00 / 0.07             -
    dgrad (3, 128, 64, 1, 1, 0, 9, 7)                  1.00 / 1.17   0.75 / 0.74   0.82 / 0.86   0.00 / 0.00   0.00 / 0.00             -
    dgrad (1, 64, 128, 3, 2, 1, 18, 14)                1.57 / 2.30   1.30 / 1.73   1.23 / 1.77   0.00 / 0.00   0.00 / 0.03             -
    dgrad (1, 64, 64, 3, 2, 1, 17, 13)                 1.59 / 2.33   1.26 / 1.98   1.12 / 1.84   0.00 / 0.00   0.00 / 0.00             -
    dgrad (1, 256, 256, 3, 1, 1, 12, 12)               3.72 / 6.82   3.25 / 4.42   2.57 / 3.93   0.01 / 0.13   0.01 / 0.35             -
    dgrad (1, 512, 512, 3, 1, 1, 2, 2)                 1.97 / 2.66   1.59 / 1.51   1.72 / 2.60   0.00 / 0.00   0.00 / 0.00             -
    dgrad (1, 64, 192, 3, 1, 1, 10, 9)                 2.74 / 4.53   2.40 / 3.80   2.16 / 2.00   0.00 / 0.00   0.02 / 0.25             -
    dgrad (1, 64, 64, 3, 1, 1, 16, 32)                 1.96 / 2.50   1.65 / 2.20   1.50 / 3.58   0.00 / 0.08   0.00 / 0.05             -
    wgrad (2, 64, 64, 3, 1, 1, 16, 12)                 1.00 / 0.89   0.88 / 1.10   0.80 / 0.66             -             -             -
    wgrad (1, 64, 128, 3, 2, 1, 18, 14)                1.00 / 1.00   0.78 / 0.47   0.83 / 0.71             -             -             -
    wgrad (1, 64, 64, 3, 2, 1, 17, 13)                 1.00 / 1.12   0.80 / 0.93   0.85 / 0.70             -             -             -
    wgrad (2, 3, 64, 7, 2, 3, 32, 40)                  1.00 / 0.91   0.87 / 0.94   0.81 / 0.83             -             -             -
    wgrad (1, 256, 256, 3, 1, 1, 12, 12)               1.00 / 0.92   0.85 / 0.88   0.83 / 0.62             -             -             -
    wgrad (1, 512, 512, 3, 1, 1, 2, 2)                 1.00 / 1.00   1.04 / 0.85   1.00 / 1.00             -             -             -
    splitk (1, 512, 512, 3, 1, 1, 10, 12)              3.21 / 3.41   2.83 / 3.70   1.65 / 2.12   0.01 / 0.26   0.01 / 0.28             -
    splitk (2, 256, 64, 10, 8, 1, 40, 40)              2.74 / 3.79   2.59 / 3.80   2.09 / 2.92   0.01 / 0.09   0.02 / 0.17             -
    convT 2x2 fwd                                      1.00 / 0.81   0.77 / 0.72   0.89 / 0.83             -             -             -
    convT 2x2 dgrad                                    1.97 / 4.34   1.64 / 3.10   1.35 / 1.76             -             -             -
    convT 2x2 wgrad                                    1.00 / 1.10   0.78 / 0.90   0.82 / 0.78             -             -             -
    convT s4 k6 p1                                     1.00 / 1.11   0.82 / 0.81   0.85 / 1.04             -             -             -
    convT s8 k2 p0                                     1.01 / 1.28   0.76 / 1.16   0.82 / 0.74             -             -             -
    winograd fwd (2, 64, 64, 13, 30)                             -             -             -             -             -   1.21 / 1.12
    winograd dgrad (2, 64, 64, 13, 30)                           -             -             -             -             -   1.22 / 1.03
    winograd wgrad (2, 64, 64, 13, 30)                           -             -             -             -             -   0.36 / 0.18
    winograd fwd (2, 64, 64, 20, 20)                             -             -             -             -             -   1.24 / 0.87
    winograd dgrad (2, 64, 64, 20, 20)                           -             -             -             -             -   1.23 / 0.96
    winograd wgrad (2, 64, 64, 20, 20)                           -             -             -             -             -   0.39 / 0.26
    f32 6.82 -> m = 16      bf16x3 4.43 -> m = 16      bf16 3.93 -> m = 8
    bf16 storage 0.29 -> m = 1      fp16 storage 1.16 -> m = 4      winograd 1.24 -> m = 4

The direct kernels are about as far from float64 as plain fp32 where K is short (1 x 1, the stem, ConvTranspose2d), and so is the weight
gradient throughout (its slabs are added in float64); on the 3 x 3 layers the ratio grows with K, to 3.7 rms / 6.8 max at K = 2304.  That is
consistent with the order of summation: an MFMA accumulator takes its K products along one chain, while fp32 on the CPU adds in vector
lanes and blocks, whose error grows more slowly.  bf16x3 follows the fp32 MFMA row by row, which is the claim these tests guard.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import conv_ref as R
from gpu_util import (DEV, ETA, L, NAN, SR, distance_ratio, exact, igemm, igemm_splitk, igemm_t, nchw, nhwc, pack, pack_t, rnd, stream,
                      wgrad)
from db_text_minimal_amd import _lib

pytestmark = pytest.mark.gpu

NS = {'f32': 0, 'bf16x3': 3, 'bf16': 1}
MODES = list(NS)
# margins m of the random-data tests: per mode, twice the largest ratio of the table in the module docstring, rounded up to a power of two
MARGIN = {'f32': 16, 'bf16x3': 16, 'bf16': 8, 'bf16 storage': 1, 'fp16 storage': 4, 'winograd': 4}
assert max(MARGIN.values()) <= 16
FWD_TILES = (0, 1, 2, 3, 4)
DGRAD_TILES = (0, 4)


def pad_c(x, c, fill=0.0):
    return x if x.shape[1] == c else torch.cat([x, torch.full((x.shape[0], c - x.shape[1], *x.shape[2:]), fill, dtype=x.dtype)], 1)


# what the padding channels (Cs > Ci) hold.  The forward kernels gather whole 4-channel vectors against zero panel rows, and
# include/dbnet_hip.h promises for none of them that padding is not read: zeros only.  The weight gradient drops the slab columns of the
# padding channels in its reduction (csrc/wgrad.hip: i >= I), so nothing they hold may reach the gradient: zeros and NaN.
WGRAD_FILLS = (0.0, NAN)


def cs_of(ci):
    return (ci + 3) // 4 * 4


def seen(t, mode):
    """The operand as the kernel's products see it (float32 values)."""
    if mode == 'bf16':
        return R.bf16_rne(t.float())
    if mode in ('bf16 storage', 'fp16 storage'):
        return t.float().to(STORAGE[mode]).float()
    return t.float()


STORAGE = {'bf16 storage': torch.bfloat16, 'fp16 storage': torch.float16}
KIND = {torch.bfloat16: 1, torch.float16: 2}


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


# ---- launches: CPU NCHW operands and device weight panels in, CPU NCHW result out ---------------------------------------------------
# (a test packs its weights once per mode and launches every tile, split count and impulse map on the same panels)
def pack_fwd(w, s, ns):
    return pack(w.float(), 0, s, ns)


def pack_bwd(w, s, ns):
    """The panels of the data gradient / of ConvTranspose2d (gather mode 1)."""
    return pack(w.float(), 1, s, ns)


def pack16(w, mode, s, dtype, cs=0):
    return pack_t(w.float(), mode, s, KIND[dtype], cs)


def run_fwd(x, wpk, Co, b, k, s, p, ns, tile, base=None):
    N, Ci, H, W = x.shape
    xs = nhwc(pad_c(x.float(), cs_of(Ci)))
    y = nan(N, R.out_size(H, k, s, p), R.out_size(W, k, s, p), Co) if base is None else nhwc(base.float())
    igemm(xs, wpk, None if b is None else b.float().to(DEV), y, k, s, p, 0, 0 if base is None else 1, tile, ns)
    return nchw(y)


def run_dgrad(dy, wpk, Ci, k, s, p, H, W, ns, tile, base=None):
    N = dy.shape[0]
    dx = nan(N, H, W, Ci) if base is None else nhwc(base.float())
    igemm(nhwc(dy.float()), wpk, None, dx, k, s, p, 1, 0 if base is None else 1, tile, ns)
    return nchw(dx)


def run_wgrad(x, dy, k, s, p, ns, fill=0.0):
    Ci, Co = x.shape[1], dy.shape[1]
    return wgrad(nhwc(dy.float()), nhwc(pad_c(x.float(), cs_of(Ci), fill)), Co, Ci, k, s, p, 1.0, ns).cpu()


def fills(Ci):
    return WGRAD_FILLS if cs_of(Ci) > Ci else (0.0, )


def run_splitk(x, wpk, Co, b, k, s, p, ns, ksplit, base=None):
    N, Ci, H, W = x.shape
    y = nan(N, R.out_size(H, k, s, p), R.out_size(W, k, s, p), Co) if base is None else nhwc(base.float())
    igemm_splitk(nhwc(x.float()), wpk, None if b is None else b.float().to(DEV), y, k, s, p, 0, ksplit,
                 0 if base is None else 1, 0, ns)
    return nchw(y)


def run_convt(x, wpk, Co, b, f, k, pad, ns, base=None):
    """ConvTranspose2d forward: mode 1 with the parity-class panels."""
    N, Ci, H, W = x.shape
    Ho, Wo = (H - 1) * f - 2 * pad + k, (W - 1) * f - 2 * pad + k
    y = nan(N, Ho, Wo, Co) if base is None else nhwc(base.float())
    igemm(nhwc(x.float()), wpk, None if b is None else b.float().to(DEV), y, k, f, pad, 1, 0 if base is None else 1, 0, ns)
    return nchw(y)


def run_t(x, wpk, Cd, b, k, s, p, dtype, tile, mode=0, out_hw=None, ksplit=1, base=None):
    """dbn_igemm_t on 16-bit storage.  mode 0: forward; mode 1: data gradient (x is dy, out_hw the size of dx)."""
    N, C, H, W = x.shape
    Hd, Wd = (R.out_size(H, k, s, p), R.out_size(W, k, s, p)) if mode == 0 else out_hw
    y = nan(N, Hd, Wd, Cd, dtype=dtype) if base is None else nhwc(base.float()).to(dtype)
    slab = None
    if ksplit > 1:
        slab = nan(L().dbn_igemm_splitk_slab_floats(ksplit, N, Hd, Wd, Cd))
    igemm_t(nhwc(x.float()).to(dtype), wpk, None if b is None else b.float().to(DEV), y, k, s, p, mode, 0 if base is None else 1, tile, 1, ksplit,
            slab)
    return nchw(y.float())


def winograd_fwd(x, w, b):
    N, Ci, H, W = x.shape
    Co = w.shape[0]
    xs = nhwc(x.float())
    up = nan(L().dbn_winograd_panel_floats(Co, Ci))
    _lib.check(L().dbn_winograd_pack(w.float().contiguous().to(DEV).data_ptr(), Co, Ci, Ci, 0, up.data_ptr(), stream()), 'winograd pack')
    assert L().dbn_winograd_eligible(N, H, W, Ci, Co)
    y = nan(N, H, W, Co)
    bd = b.float().to(DEV)
    _lib.check(L().dbn_winograd_conv_bn_f32(xs.data_ptr(), up.data_ptr(), bd.data_ptr(), y.data_ptr(), N, H, W, Ci, Co, None, None, 0.0, 0.0, None,
                                            None, None, None, None, None, None, stream()), 'winograd')
    return nchw(y)


def winograd_dgrad(dy, w, base=None):
    """dbn_winograd_dgrad_bnsums_f32 without a mask."""
    N, Co, H, W = dy.shape
    Ci = w.shape[1]
    dys = nhwc(dy.float())
    up = nan(L().dbn_winograd_panel_floats(Ci, Co))
    _lib.check(L().dbn_winograd_pack(w.float().contiguous().to(DEV).data_ptr(), Ci, Co, Co, 1, up.data_ptr(), stream()), 'winograd pack (dgrad)')
    dx = nan(N, H, W, Ci) if base is None else nhwc(base.float())
    _lib.check(L().dbn_winograd_dgrad_bnsums_f32(dys.data_ptr(), up.data_ptr(), dx.data_ptr(), N, H, W, Co, Ci, 0 if base is None else 1, None, None,
                                                 None, None, None, None, None, None, None, None, None, None, stream()), 'winograd dgrad')
    return nchw(dx)


def winograd_wgrad(x, dy):
    N, Ci, H, W = x.shape
    Co = dy.shape[1]
    xs, dys = nhwc(x.float()), nhwc(dy.float())
    assert L().dbn_winograd_wgrad_eligible(N, H, W, Co, Ci, Ci)
    slab = nan(L().dbn_winograd_wgrad_slab_floats(N, H, W, Co, Ci))
    g = nan(Co, Ci, 3, 3)
    _lib.check(L().dbn_winograd_wgrad_f32(3, dys.data_ptr(), xs.data_ptr(), None, None, slab.data_ptr(), g.data_ptr(), N, H, W, Co, Ci, Ci, 1.0,
                                          stream()), 'winograd wgrad')
    return g.cpu()


# ---- random data --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_case(case, mode):
    """Operands (float32, as handed to the kernel), the operands the products see, and the forward references — shared by the tests."""
    N, Ci, Co, k, s, p, H, W = case
    x = rnd(N, Ci, H, W, seed=1)
    w = rnd(Co, Ci, k, k, seed=2, scale=(2.0 / (Ci * k * k))**0.5)
    b = rnd(Co, seed=3)
    dy = rnd(N, Co, R.out_size(H, k, s, p), R.out_size(W, k, s, p), seed=4)
    return x, w, b, dy, seen(x, mode), seen(w, mode), seen(dy, mode)


def fwd_refs(xo, wo, b, s, p):
    return R.conv2d(xo.double(), wo.double(), b.double(), s, p), F.conv2d(xo, wo, b, s, p)


def grad_refs32(xo, wo, dyo, s, p):
    xg, wg = xo.clone().requires_grad_(True), wo.clone().requires_grad_(True)
    return torch.autograd.grad(F.conv2d(xg, wg, None, s, p), (xg, wg), dyo)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', R.FWD_CASES)
def test_forward_distance_to_fp64(case, mode):
    N, Ci, Co, k, s, p, H, W = case
    x, w, b, _, xo, wo, _ = random_case(case, mode)
    ref64, ref32 = fwd_refs(xo, wo, b, s, p)
    wpk = pack_fwd(w, s, NS[mode])
    for tile in FWD_TILES:
        distance_ratio('fwd %s %s tile %d' % (case, mode, tile), run_fwd(x, wpk, Co, b, k, s, p, NS[mode], tile), ref64, ref32, MARGIN[mode])


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', R.DGRAD_CASES)
def test_data_gradient_distance_to_fp64(case, mode):
    N, Ci, Co, k, s, p, H, W = case
    x, w, _, dy, xo, wo, dyo = random_case(case, mode)
    ref64 = R.conv2d_dgrad(dyo.double(), wo.double(), s, p, H, W)
    ref32 = grad_refs32(xo, wo, dyo, s, p)[0]
    wpk = pack_bwd(w, s, NS[mode])
    for tile in DGRAD_TILES:
        distance_ratio('dgrad %s %s tile %d' % (case, mode, tile), run_dgrad(dy, wpk, Ci, k, s, p, H, W, NS[mode], tile), ref64, ref32, MARGIN[mode])


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', R.WGRAD_CASES)
def test_weight_gradient_distance_to_fp64(case, mode):
    N, Ci, Co, k, s, p, H, W = case
    x, w, _, dy, xo, wo, dyo = random_case(case, mode)
    ref64 = R.conv2d_wgrad(xo.double(), dyo.double(), k, k, s, p)
    ref32 = grad_refs32(xo, wo, dyo, s, p)[1]
    for fill in fills(Ci):
        distance_ratio('wgrad %s %s padding %g' % (case, mode, fill), run_wgrad(x, dy, k, s, p, NS[mode], fill), ref64, ref32, MARGIN[mode])


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', R.SPLITK_CASES)
def test_splitk_distance_to_fp64(case, mode):
    N, Ci, Co, k, s, p, H, W = case
    x, w, b, _, xo, wo, _ = random_case(case, mode)
    ref64, ref32 = fwd_refs(xo, wo, b, s, p)
    wpk = pack_fwd(w, s, NS[mode])
    for ksplit in R.KSPLITS:
        distance_ratio('splitk %s %s ksplit %d' % (case, mode, ksplit), run_splitk(x, wpk, Co, b, k, s, p, NS[mode], ksplit), ref64, ref32, MARGIN[mode])


def convt_operands(shape, k, mode):
    N, Ci, Co, H, W = shape
    x, w, b = rnd(N, Ci, H, W, seed=1), rnd(Ci, Co, k, k, seed=2, scale=0.1), rnd(Co, seed=3)
    return x, w, b, seen(x, mode), seen(w, mode)


@pytest.mark.parametrize('mode', MODES)
def test_conv_transpose_2x2_distance_to_fp64(mode):
    """Forward (fp32: the dedicated 2 x 2 kernel and, with it switched off, the general parity-class launch), data and weight gradient."""
    N, Ci, Co, H, W = R.CONVT2
    ns = NS[mode]
    x, w, b, xo, wo = convt_operands(R.CONVT2, 2, mode)
    dy = rnd(N, Co, 2 * H, 2 * W, seed=5)
    dyo = seen(dy, mode)
    ref64 = R.conv_transpose2d(xo.double(), wo.double(), b.double(), 2, 0)
    xg, wg = xo.clone().requires_grad_(True), wo.clone().requires_grad_(True)
    y32 = F.conv_transpose2d(xg, wg, b, 2, 0)
    dx32, dw32 = torch.autograd.grad(y32, (xg, wg), dyo)
    wpk = pack_bwd(w, 2, ns)
    distance_ratio('convT 2x2 fwd %s' % mode, run_convt(x, wpk, Co, b, 2, 2, 0, ns), ref64, y32.detach(), MARGIN[mode])
    if ns == 0:
        old = L().dbn_set_convt_kernel(0)
        try:
            distance_ratio('convT 2x2 fwd (parity classes) %s' % mode, run_convt(x, wpk, Co, b, 2, 2, 0, ns), ref64, y32.detach(), MARGIN[mode])
        finally:
            L().dbn_set_convt_kernel(old)
    # its data gradient is a stride-2 forward conv of dy, its weight gradient the conv weight gradient with x and dy swapped
    distance_ratio('convT 2x2 dgrad %s' % mode, run_fwd(dy, pack_fwd(w, 2, ns), Ci, None, 2, 2, 0, ns, 0),
                   R.conv2d(dyo.double(), wo.double(), None, 2, 0), dx32, MARGIN[mode])
    distance_ratio('convT 2x2 wgrad %s' % mode, run_wgrad(dy, x, 2, 2, 0, ns), R.conv2d_wgrad(dyo.double(), xo.double(), 2, 2, 2, 0), dw32,
                   MARGIN[mode])


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('f,k,pad', R.CONVT_GENERAL)
def test_conv_transpose_general_stride_distance_to_fp64(f, k, pad, mode):
    x, w, b, xo, wo = convt_operands(R.CONVT_GENERAL_SHAPE, k, mode)
    if k < f:
        b = None  # pixels without taps: the kernel takes no bias there
    ref64 = R.conv_transpose2d(xo.double(), wo.double(), None if b is None else b.double(), f, pad)
    ref32 = F.conv_transpose2d(xo, wo, b, f, pad)
    got = run_convt(x, pack_bwd(w, f, NS[mode]), w.shape[1], b, f, k, pad, NS[mode])
    distance_ratio('convT s%d k%d p%d %s' % (f, k, pad, mode), got, ref64, ref32, MARGIN[mode])


def allowance(ref64, dtype):
    at = KIND[dtype]
    return SR[at] * ref64.abs() + ETA[at]


@pytest.mark.parametrize('mode', list(STORAGE))
@pytest.mark.parametrize('case', [c for c in R.FWD_CASES if c[1] % 16 == 0])
def test_16bit_storage_forward_distance_to_fp64(case, mode):
    N, Ci, Co, k, s, p, H, W = case
    dtype = STORAGE[mode]
    x, w, b, _, xo, wo, _ = random_case(case, mode)
    ref64, ref32 = fwd_refs(xo, wo, b, s, p)
    wpk = pack16(w, 0, s, dtype, Ci)
    for tile in FWD_TILES:
        distance_ratio('fwd %s %s tile %d' % (case, mode, tile), run_t(x, wpk, Co, b, k, s, p, dtype, tile), ref64, ref32, MARGIN[mode],
                       allowance(ref64, dtype))


@pytest.mark.parametrize('mode', list(STORAGE))
@pytest.mark.parametrize('case', R.DGRAD_CASES)
def test_16bit_storage_data_gradient_distance_to_fp64(case, mode):
    N, Ci, Co, k, s, p, H, W = case
    dtype = STORAGE[mode]
    x, w, _, dy, xo, wo, dyo = random_case(case, mode)
    ref64 = R.conv2d_dgrad(dyo.double(), wo.double(), s, p, H, W)
    ref32 = grad_refs32(xo, wo, dyo, s, p)[0]
    wpk = pack16(w, 1, s, dtype)
    for tile in DGRAD_TILES:
        distance_ratio('dgrad %s %s tile %d' % (case, mode, tile), run_t(dy, wpk, Ci, None, k, s, p, dtype, tile, 1, (H, W)), ref64, ref32, MARGIN[mode],
                       allowance(ref64, dtype))


@pytest.mark.parametrize('mode', list(STORAGE))
@pytest.mark.parametrize('case', R.SPLITK_CASES)
def test_16bit_storage_splitk_distance_to_fp64(case, mode):
    N, Ci, Co, k, s, p, H, W = case
    dtype = STORAGE[mode]
    x, w, b, _, xo, wo, _ = random_case(case, mode)
    ref64, ref32 = fwd_refs(xo, wo, b, s, p)
    wpk = pack16(w, 0, s, dtype, Ci)
    for ksplit in R.KSPLITS:
        distance_ratio('splitk %s %s ksplit %d' % (case, mode, ksplit), run_t(x, wpk, Co, b, k, s, p, dtype, 0, ksplit=ksplit), ref64, ref32, MARGIN[mode],
                       allowance(ref64, dtype))


@pytest.mark.parametrize('shape', R.WINOGRAD_CASES)
def test_winograd_distance_to_fp64(shape):
    """Forward, data gradient and weight gradient once each, so that every convolution kernel stands in the table."""
    N, Ci, Co, H, W = shape
    case = (N, Ci, Co, 3, 1, 1, H, W)
    x, w, b, dy, xo, wo, dyo = random_case(case, 'f32')
    ref64, ref32 = fwd_refs(xo, wo, b, 1, 1)
    m = MARGIN['winograd']
    distance_ratio('winograd fwd %s' % (shape, ), winograd_fwd(x, w, b), ref64, ref32, m)
    dx32, dw32 = grad_refs32(xo, wo, dyo, 1, 1)
    distance_ratio('winograd dgrad %s' % (shape, ), winograd_dgrad(dy, w), R.conv2d_dgrad(dy.double(), w.double(), 1, 1, H, W), dx32, m)
    distance_ratio('winograd wgrad %s' % (shape, ), winograd_wgrad(x, dy), R.conv2d_wgrad(x.double(), dy.double(), 3, 3, 1, 1), dw32, m)


# ---- exact data: dense --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense_case(case):
    N, Ci, Co, k, s, p, H, W = case
    Ho, Wo = R.out_size(H, k, s, p), R.out_size(W, k, s, p)
    x, w, b = R.dense_x((N, Ci, H, W), 11), R.dense_w((Co, Ci, k, k), 12), R.dense_bias(Co, 13)
    dy = R.dense_x((N, Co, Ho, Wo), 14)
    base_y = R.dense_bias(N * Co * Ho * Wo, 15).reshape(N, Co, Ho, Wo)  # the dyadic base of the accumulate form
    base_x = R.dense_bias(N * Ci * H * W, 16).reshape(N, Ci, H, W)
    return x, w, b, dy, base_y, base_x


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', R.FWD_CASES)
def test_forward_is_exact_on_dense_dyadic_data(case, mode):
    N, Ci, Co, k, s, p, H, W = case
    x, w, b, _, base, _ = dense_case(case)
    ref, ref_acc = R.conv2d(x, w, b, s, p), R.accumulate(base, R.conv2d(x, w, None, s, p))
    wpk = pack_fwd(w, s, NS[mode])
    for tile in FWD_TILES:
        exact('fwd %s %s tile %d' % (case, mode, tile), run_fwd(x, wpk, Co, b, k, s, p, NS[mode], tile), ref)
        exact('fwd + base %s %s tile %d' % (case, mode, tile), run_fwd(x, wpk, Co, None, k, s, p, NS[mode], tile, base), ref_acc)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', R.DGRAD_CASES)
def test_data_gradient_is_exact_on_dense_dyadic_data(case, mode):
    N, Ci, Co, k, s, p, H, W = case
    _, w, _, dy, _, base = dense_case(case)
    ref = R.conv2d_dgrad(dy, w, s, p, H, W)
    wpk = pack_bwd(w, s, NS[mode])
    for tile in DGRAD_TILES:
        exact('dgrad %s %s tile %d' % (case, mode, tile), run_dgrad(dy, wpk, Ci, k, s, p, H, W, NS[mode], tile), ref)
        exact('dgrad + base %s %s tile %d' % (case, mode, tile), run_dgrad(dy, wpk, Ci, k, s, p, H, W, NS[mode], tile, base), R.accumulate(base, ref))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', R.WGRAD_CASES)
def test_weight_gradient_is_exact_on_dense_dyadic_data(case, mode):
    N, Ci, Co, k, s, p, H, W = case
    x, _, _, dy, _, _ = dense_case(case)
    ref = R.conv2d_wgrad(x, dy, k, k, s, p)
    for fill in fills(Ci):
        exact('wgrad %s %s padding %g' % (case, mode, fill), run_wgrad(x, dy, k, s, p, NS[mode], fill), ref)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', R.SPLITK_CASES)
def test_splitk_is_exact_on_dense_dyadic_data(case, mode):
    N, Ci, Co, k, s, p, H, W = case
    x, w, b, _, base, _ = dense_case(case)
    ref = R.conv2d(x, w, b, s, p)
    wpk = pack_fwd(w, s, NS[mode])
    for ksplit in R.KSPLITS:
        exact('splitk %s %s ksplit %d' % (case, mode, ksplit), run_splitk(x, wpk, Co, b, k, s, p, NS[mode], ksplit), ref)
        exact('splitk + base %s %s ksplit %d' % (case, mode, ksplit), run_splitk(x, wpk, Co, b, k, s, p, NS[mode], ksplit, base), R.accumulate(base, ref))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('f,k,pad', [(2, 2, 0)] + R.CONVT_GENERAL)
def test_conv_transpose_is_exact_on_dense_dyadic_data(f, k, pad, mode):
    N, Ci, Co, H, W = R.CONVT2 if k == 2 and f == 2 else R.CONVT_GENERAL_SHAPE
    ns = NS[mode]
    x, w = R.dense_x((N, Ci, H, W), 11), R.dense_w((Ci, Co, k, k), 12)
    b = R.dense_bias(Co, 13) if k >= f else None
    ref = R.conv_transpose2d(x, w, b, f, pad)
    base = R.dense_bias(ref.numel(), 15).reshape(ref.shape)
    wpk = pack_bwd(w, f, ns)
    for convt_kernel in ((1, 0) if (ns == 0 and f == 2 and k == 2) else (1, )):
        old = L().dbn_set_convt_kernel(convt_kernel)
        try:
            exact('convT s%d k%d p%d %s' % (f, k, pad, mode), run_convt(x, wpk, Co, b, f, k, pad, ns), ref)
            exact('convT + base s%d k%d p%d %s' % (f, k, pad, mode), run_convt(x, wpk, Co, None, f, k, pad, ns, base),
                  R.accumulate(base, R.conv_transpose2d(x, w, None, f, pad)))
        finally:
            L().dbn_set_convt_kernel(old)
    if f == 2 and k == 2:
        dy = R.dense_x(tuple(ref.shape), 14)
        exact('convT dgrad %s' % mode, run_fwd(dy, pack_fwd(w, 2, ns), Ci, None, 2, 2, 0, ns, 0), R.conv2d(dy, w, None, 2, 0))
        exact('convT wgrad %s' % mode, run_wgrad(dy, x, 2, 2, 0, ns), R.conv2d_wgrad(dy, x, 2, 2, 2, 0))


@pytest.mark.parametrize('shape', R.WINOGRAD_CASES + R.WINOGRAD_SEAM_CASES[:2])
def test_winograd_is_exact_on_dense_dyadic_data(shape):
    """Weights on multiples of 1 / 2: G g G^T stays dyadic and every transform is exact in fp32 (tests/test_conv_ref_cpu.py)."""
    N, Ci, Co, H, W = shape
    x, w, b = R.dense_x((N, Ci, H, W), 21), R.dense_w((Co, Ci, 3, 3), 22, winograd=True), R.dense_bias(Co, 23)
    dy = R.dense_x((N, Co, H, W), 24)
    base = R.dense_bias(N * Ci * H * W, 16).reshape(N, Ci, H, W)
    exact('winograd fwd %s' % (shape, ), winograd_fwd(x, w, b), R.conv2d(x, w, b, 1, 1))
    dx = R.conv2d_dgrad(dy, w, 1, 1, H, W)
    exact('winograd dgrad %s' % (shape, ), winograd_dgrad(dy, w), dx)
    exact('winograd dgrad + base %s' % (shape, ), winograd_dgrad(dy, w, base), R.accumulate(base, dx))
    exact('winograd wgrad %s' % (shape, ), winograd_wgrad(x, dy), R.conv2d_wgrad(x, dy, 3, 3, 1, 1))


# ---- exact data: impulses on the seams ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def impulse_case(case, two_channels=True):
    """The impulse maps of a forward conv (in x) and of its gradients (in dy), the distinct weights and the references."""
    N, Ci, Co, k, s, p, H, W = case
    Ho, Wo = R.out_size(H, k, s, p), R.out_size(W, k, s, p)
    w = R.distinct_w(Co, Ci, k, k)
    xs = R.impulse_maps(N, Ci, H, W, R.seam_pixels(N, H, W, Ho, Wo, s), k, two_channels)
    dys = R.impulse_maps(N, Co, Ho, Wo, R.seam_pixels(N, Ho, Wo, H, W, s), k, two_channels)
    return w, xs, dys


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', R.FWD_CASES)
def test_forward_is_exact_on_seam_impulses(case, mode):
    N, Ci, Co, k, s, p, H, W = case
    w, xs, _ = impulse_case(case)
    b = R.dense_bias(Co, 13)
    wpk = pack_fwd(w, s, NS[mode])
    for i, x in enumerate(xs):
        ref = R.conv2d(x, w, b, s, p)
        for tile in FWD_TILES:
            exact('fwd impulses %d %s %s tile %d' % (i, case, mode, tile), run_fwd(x, wpk, Co, b, k, s, p, NS[mode], tile), ref)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', R.DGRAD_CASES)
def test_data_gradient_is_exact_on_seam_impulses(case, mode):
    N, Ci, Co, k, s, p, H, W = case
    w, _, dys = impulse_case(case)
    wpk = pack_bwd(w, s, NS[mode])
    for i, dy in enumerate(dys):
        ref = R.conv2d_dgrad(dy, w, s, p, H, W)
        for tile in DGRAD_TILES:
            exact('dgrad impulses %d %s %s tile %d' % (i, case, mode, tile), run_dgrad(dy, wpk, Ci, k, s, p, H, W, NS[mode], tile), ref)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', R.WGRAD_CASES)
def test_weight_gradient_is_exact_on_sparse_dy(case, mode):
    """dy zero except on the seams of the output map, x dense and exact."""
    N, Ci, Co, k, s, p, H, W = case
    Ho, Wo = R.out_size(H, k, s, p), R.out_size(W, k, s, p)
    x = dense_case(case)[0]
    (dy, ) = R.impulse_maps(N, Co, Ho, Wo, R.seam_pixels(N, Ho, Wo, Ho, Wo, 1), 0)
    ref = R.conv2d_wgrad(x, dy, k, k, s, p)
    for fill in fills(Ci):
        exact('wgrad sparse dy %s %s padding %g' % (case, mode, fill), run_wgrad(x, dy, k, s, p, NS[mode], fill), ref)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', R.SPLITK_CASES)
def test_splitk_is_exact_on_seam_impulses(case, mode):
    """The impulse channels (the last one, and one per pixel elsewhere) fall into different split-K chunks."""
    N, Ci, Co, k, s, p, H, W = case
    w, xs, _ = impulse_case(case)
    b = R.dense_bias(Co, 13)
    wpk = pack_fwd(w, s, NS[mode])
    for i, x in enumerate(xs):
        ref = R.conv2d(x, w, b, s, p)
        for ksplit in R.KSPLITS:
            exact('splitk impulses %d %s %s ksplit %d' % (i, case, mode, ksplit), run_splitk(x, wpk, Co, b, k, s, p, NS[mode], ksplit), ref)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('f,k,pad', [(2, 2, 0)] + R.CONVT_GENERAL)
def test_conv_transpose_is_exact_on_seam_impulses(f, k, pad, mode):
    N, Ci, Co, H, W = R.CONVT2 if k == 2 and f == 2 else R.CONVT_GENERAL_SHAPE
    w = R.distinct_w(Ci, Co, k, k)
    Ho, Wo = (H - 1) * f - 2 * pad + k, (W - 1) * f - 2 * pad + k
    # the seams of a walk over the output map and of one over the input map (the 2 x 2 kernel and the parity-class launches tile the
    # pixels of one class, which are the input pixels)
    pts = R.seam_pixels(N, H, W, Ho, Wo, f) + R.seam_pixels(N, H, W, H, W, 1) + [(0, H // 2, W // 2), (N - 1, H // 2, W // 2 + 1)]
    wpk = pack_bwd(w, f, NS[mode])
    for i, x in enumerate(R.impulse_maps(N, Ci, H, W, sorted(set(pts)), 2)):
        exact('convT impulses %d s%d k%d p%d %s' % (i, f, k, pad, mode), run_convt(x, wpk, Co, None, f, k, pad, NS[mode]),
              R.conv_transpose2d(x, w, None, f, pad))


@pytest.mark.parametrize('mode', list(STORAGE))
@pytest.mark.parametrize('case', [c for c in R.FWD_CASES if c[1] % 16 == 0])
def test_16bit_storage_is_exact_on_seam_impulses(case, mode):
    """One channel per impulse and no bias: every output is a single product m / 128 times 1, -2 or 1 / 2 — representable in bf16 and
    fp16 (tests/test_conv_ref_cpu.py), so the stored result equals float64 as well.  All tiles, the data gradient where the kernel has
    one (Ci % 64 == 0)."""
    N, Ci, Co, k, s, p, H, W = case
    dtype = STORAGE[mode]
    w, xs, dys = impulse_case(case, False)
    wpk = pack16(w, 0, s, dtype, Ci)
    for i, x in enumerate(xs):
        ref = R.conv2d(x, w, None, s, p)
        for tile in FWD_TILES:
            exact('fwd impulses %d %s %s tile %d' % (i, case, mode, tile), run_t(x, wpk, Co, None, k, s, p, dtype, tile), ref)
    if case in R.DGRAD_CASES:
        wpk = pack16(w, 1, s, dtype)
        for i, dy in enumerate(dys):
            ref = R.conv2d_dgrad(dy, w, s, p, H, W)
            for tile in DGRAD_TILES:
                exact('dgrad impulses %d %s %s tile %d' % (i, case, mode, tile), run_t(dy, wpk, Ci, None, k, s, p, dtype, tile, 1, (H, W)), ref)


@pytest.mark.parametrize('mode', list(STORAGE))
@pytest.mark.parametrize('case', R.SPLITK_CASES)
def test_16bit_storage_splitk_is_exact_on_seam_impulses(case, mode):
    N, Ci, Co, k, s, p, H, W = case
    dtype = STORAGE[mode]
    w, xs, _ = impulse_case(case, False)
    wpk = pack16(w, 0, s, dtype, Ci)
    for i, x in enumerate(xs):
        ref = R.conv2d(x, w, None, s, p)
        for ksplit in R.KSPLITS:
            exact('splitk impulses %d %s %s ksplit %d' % (i, case, mode, ksplit), run_t(x, wpk, Co, None, k, s, p, dtype, 0, ksplit=ksplit), ref)


@pytest.mark.parametrize('shape', R.WINOGRAD_SEAM_CASES)
def test_winograd_is_exact_on_seam_impulses(shape):
    """Impulses around an 8 x 16 patch corner, on the last row and column of odd maps and in the first and last tile of every 32-tile group of
    the consecutive-tile form; the weight gradient with sparse dy on the same seams and dense exact x."""
    N, Ci, Co, H, W = shape
    pts = R.winograd_seams(N, H, W)
    w = R.distinct_w(Co, Ci, 3, 3)
    b = R.dense_bias(Co, 23)
    (x, ) = R.impulse_maps(N, Ci, H, W, pts, 0)
    (dy, ) = R.impulse_maps(N, Co, H, W, pts, 0)
    exact('winograd fwd impulses %s' % (shape, ), winograd_fwd(x, w, b), R.conv2d(x, w, b, 1, 1))
    exact('winograd dgrad impulses %s' % (shape, ), winograd_dgrad(dy, w), R.conv2d_dgrad(dy, w, 1, 1, H, W))
    xd = R.dense_x((N, Ci, H, W), 21)
    exact('winograd wgrad sparse dy %s' % (shape, ), winograd_wgrad(xd, dy), R.conv2d_wgrad(xd, dy, 3, 3, 1, 1))
