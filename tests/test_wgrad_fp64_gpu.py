"""-m gpu: the weight gradient (dbn_wgrad_t, csrc/wgrad.hip and wgrad_kernels.h) at the sizes where it runs as the training step runs it —
several pixel splits, a split that ends inside a k-step or inside a 32-pixel LDS stage, the pixel-patch kernel, stored-bf16 operands,
the slab reduction with more than one thread group — against the float64 reference of tests/conv_ref.py.  It continues
tests/test_conv_fp64_gpu.py, whose weight-gradient cases all fit one or two splits; tests/test_wgrad_cases_cpu.py asks the library's plan
functions that every case below reaches the path it is listed for.

Modes (at, ns of dbn_wgrad_t): f32 (0, 0), bf16x3 (0, 3), bf16 (0, 1) on fp32 tensors, bf16 storage (1, 1) on stored-bf16 dY and X.  The
gradient is fp32 in all of them.  Every launch gets a NaN-filled slab and a NaN-filled gradient: a slab element that no workgroup wrote and
the reduction reads, or a gradient element nobody wrote, fails the test.  The scale alternates between 1 and 1 / 2 from case to case (both
exact).  The stem's padding channels (Ci = 3 stored as 4 fp32 or 16 bf16 channels) hold zeros in one run and NaN in another: the
reduction drops their columns, so nothing they hold may reach the gradient.

  * dense dyadic data ({-4..4} / 4 in x and dy): equal to float64 BIT FOR BIT in every mode, whatever the order of summation (every
    partial sum is exact in fp32: test_wgrad_cases_cpu.py).  On bf16 storage also under dbn_set_wgrad_variant(2), the register-transposing
    kernel with AT = 1: a third implementation on the same tensors;
  * sparse dy, dense x: impulses on both sides of every multiple of 16 flattened output pixels — every split boundary (pchunk % 16 == 0),
    every k-step, every 32-pixel stage of wgrad_tr_kernel, every patch row — and on the first and last pixel of every image;
  * sparse x, dense dy: impulses in the image corners, all along the last row and column, at the input pixel of both sides of every
    16-pixel boundary and, on the pixel-patch cases, on the four pixels around every 4 x 16 patch corner: the halo pixels that
    wgrad_patch_kernel's 18-wide rows and the per-tap gathers of the other kernels must fetch, or replace by zero;
  * random data: the distance to float64 against that of fp32 autograd on the CPU on the operands as the mode sees them (bf16 and bf16
    storage: rounded to bf16, ties to even), rms and max, as in test_conv_fp64_gpu.py; no output rounding is allowed for;
  * dbn_wgrad_phase_t(1) then (2), a second run of the same launch, and ONE dbn_wgrad_reduce_many over the records of all cases whose X
    has a multiple of 64 channels (natural and position-space slabs, R S in {1, 4, 9, 16}, G in {1, 2, 3, 4, 7} thread groups): bit-identical
    to the single call, on random data (on exact data every order gives the same bits).

The margins m follow the rule of test_conv_fp64_gpu.py: per mode twice the largest ratio measured on the MI355X over these cases, rounded
up to a power of two, capped at 16.  Each random-data test prints
    RATIO wgrad <case> <mode> padding <v>: rms <ratio> max <ratio> (fp32 itself: rms <abs> max <abs>)
and the table holds "rms ratio / max ratio", the worse of the two padding forms of the stem.

    case                                                   f32        bf16x3          bf16  bf16 storage
    wgrad (3, 64, 64, 3, 1, 1, 40, 36)             0.67 / 0.56   0.58 / 0.46   0.48 / 0.43   0.48 / 0.42
    wgrad (2, 64, 64, 3, 1, 1, 37, 59)             0.47 / 0.40   0.41 / 0.41   0.31 / 0.24   0.31 / 0.24
    wgrad (2, 32, 64, 3, 1, 1, 37, 41)             0.58 / 0.49   0.50 / 0.42   0.39 / 0.29   0.39 / 0.29
    wgrad (2, 96, 64, 3, 1, 1, 37, 41)             0.58 / 0.56   0.50 / 0.46   0.39 / 0.28   0.39 / 0.28
    wgrad (1, 64, 128, 3, 2, 1, 97, 83)            0.45 / 0.39   0.38 / 0.28   0.29 / 0.14   0.29 / 0.14
    wgrad (2, 64, 128, 1, 2, 0, 90, 94)            0.93 / 0.89   0.80 / 0.64   0.71 / 0.74   0.71 / 0.74
    wgrad (4, 128, 64, 1, 1, 0, 45, 47)            0.85 / 0.83   0.76 / 0.76   0.63 / 0.62   0.63 / 0.62
    wgrad (2, 64, 64, 2, 2, 0, 100, 96)            0.63 / 0.56   0.55 / 0.54   0.43 / 0.41   0.43 / 0.41
    wgrad (2, 64, 64, 4, 2, 1, 90, 94)             0.47 / 0.37   0.41 / 0.27   0.31 / 0.20   0.31 / 0.20
    wgrad (2, 3, 64, 7, 2, 3, 97, 99)              0.64 / 0.51   0.56 / 0.40   0.44 / 0.34   0.44 / 0.34
    wgrad (2, 64, 64, 3, 1, 1, 48, 48)             0.67 / 0.52   0.58 / 0.48   0.47 / 0.46   0.47 / 0.46
    wgrad (3, 64, 64, 3, 1, 1, 44, 48)             0.56 / 0.59   0.50 / 0.53   0.38 / 0.30   0.38 / 0.30
    wgrad (2, 64, 192, 3, 1, 1, 36, 32)            0.63 / 0.70   0.56 / 0.49   0.46 / 0.34   0.46 / 0.34
    wgrad (2, 128, 64, 3, 1, 1, 36, 32)            0.63 / 0.51   0.56 / 0.40   0.46 / 0.28   0.46 / 0.28
    wgrad (1, 256, 256, 3, 1, 1, 60, 240)          0.38 / 0.24   0.37 / 0.26   0.24 / 0.13   0.24 / 0.13
    f32 0.93 -> m = 2      bf16x3 0.80 -> m = 2      bf16 0.74 -> m = 2      bf16 storage 0.74 -> m = 2

With several splits the kernel is CLOSER to float64 than fp32 autograd: a split's fp32 chain is P / splits pixels long and the slabs are added
in float64: every ratio is below 1, where the one-split rows of test_conv_fp64_gpu.py sit at 0.8 - 1.1.  bf16 on fp32 tensors and bf16 storage form
the same products from the same rounded operands; their rows agree to the digits shown.  No case exposed a defect: the kernels needed no change.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import conv_ref as R
from gpu_util import DEV, L, NAN, distance_ratio, exact, nhwc, rnd, stream, wgrad_t, wgrad_t_call
from db_text_minimal_amd import _lib

pytestmark = pytest.mark.gpu

MODES = {'f32': (0, 0), 'bf16x3': (0, 3), 'bf16': (0, 1), 'bf16 storage': (1, 1)}  # mode -> (at, ns)
# margins m of the random-data test: per mode, twice the largest ratio of the table in the module docstring, rounded up to a power of two
MARGIN = {'f32': 2, 'bf16x3': 2, 'bf16': 2, 'bf16 storage': 2}
assert max(MARGIN.values()) <= 16
CASES = R.WGRAD_SPLIT_CASES + R.WGRAD_PATCH_CASES
CASES64 = [c for c in CASES if c[1] % 64 == 0]  # the 64-channel reduction form (wgrad_reduce64_kernel, dbn_wgrad_reduce_many)
SCALE = {c: (1.0, 0.5)[i % 2] for i, c in enumerate(CASES)}


def cb_of(ci, at):
    """Stored channels of X: fp32 tensors pad to 4, bf16 storage to 16 (the stem)."""
    return (ci + 3) // 4 * 4 if at == 0 else (ci + 15) // 16 * 16


def fills(case, mode):
    """What the padding channels of X hold, run by run."""
    return (0.0, NAN) if cb_of(case[1], MODES[mode][0]) > case[1] else (0.0, )


def device_operands(case, mode, x, dy, fill=0.0):
    """CPU NCHW operands -> device NHWC (dY, X) in the mode's storage type, X padded to its stored channel count with `fill`."""
    at = MODES[mode][0]
    Cb = cb_of(case[1], at)
    x = x.float()
    if Cb > x.shape[1]:
        x = torch.cat([x, torch.full((x.shape[0], Cb - x.shape[1], *x.shape[2:]), fill)], 1)
    dt = torch.bfloat16 if at == 1 else torch.float32
    return nhwc(dy.float()).to(dt), nhwc(x).to(dt)


def run(case, mode, x, dy, fill=0.0, variant=0, phases=False):
    """One dbn_wgrad_t call (NaN-filled slab and gradient) -> the gradient [Co, Ci, k, k] on the CPU."""
    N, Ci, Co, k, s, p, H, W = case
    sm, big = device_operands(case, mode, x, dy, fill)
    try:
        _lib.check(L().dbn_set_wgrad_variant(variant), 'variant')
        g = wgrad_t(sm, big, Co, Ci, k, s, p, MODES[mode][1], SCALE[case], phases)
        torch.cuda.synchronize()
    finally:
        L().dbn_set_wgrad_variant(0)
    return g.cpu()


def seen(t, mode):
    """The operand as the kernel's products see it (float32 values)."""
    return R.bf16_rne(t.float()) if mode in ('bf16', 'bf16 storage') else t.float()


def out_hw(case):
    N, Ci, Co, k, s, p, H, W = case
    return R.out_size(H, k, s, p), R.out_size(W, k, s, p)


# ---- operands and references, computed once per case ------------------------------------------------------------------------------------
def ref64(case, x, dy):
    k, s, p = case[3:6]
    return SCALE[case] * R.conv2d_wgrad(x.double(), dy.double(), k, k, s, p)


@functools.lru_cache(maxsize=None)
def dense_case(case):
    N, Ci, Co, k, s, p, H, W = case
    x, dy = R.dense_x((N, Ci, H, W), 11), R.dense_x((N, Co, *out_hw(case)), 14)
    return x, dy, ref64(case, x, dy)


@functools.lru_cache(maxsize=None)
def sparse_dy_case(case):
    N, Ci, Co, k, s, p, H, W = case
    Ho, Wo = out_hw(case)
    x = dense_case(case)[0]
    (dy, ) = R.impulse_maps(N, Co, Ho, Wo, R.seam_pixels(N, Ho, Wo, Ho, Wo, 1, tile_rows=16), 0)
    return x, dy, ref64(case, x, dy)


@functools.lru_cache(maxsize=None)
def sparse_x_case(case):
    N, Ci, Co, k, s, p, H, W = case
    dy = dense_case(case)[1]
    (x, ) = R.impulse_maps(N, Ci, H, W, R.wgrad_x_seams(case), 0)
    return x, dy, ref64(case, x, dy)


@functools.lru_cache(maxsize=None)
def random_operands(case):
    N, Ci, Co, k, s, p, H, W = case
    return rnd(N, Ci, H, W, seed=1), rnd(N, Co, *out_hw(case), seed=4)


@functools.lru_cache(maxsize=None)
def random_refs(case, rounded):
    """(float64 reference, fp32 autograd on the CPU) on the operands as seen: as they are, or rounded to bf16."""
    N, Ci, Co, k, s, p, H, W = case
    x, dy = (seen(t, 'bf16' if rounded else 'f32') for t in random_operands(case))
    w = torch.zeros((Co, Ci, k, k), requires_grad=True)  # (the gradient with respect to w does not depend on w)
    (g32, ) = torch.autograd.grad(F.conv2d(x, w, None, s, p), w, dy)
    return ref64(case, x, dy), SCALE[case] * g32


# ---- exact data -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('case', CASES)
def test_weight_gradient_is_exact_on_dense_dyadic_data(case, mode):
    x, dy, ref = dense_case(case)
    for fill in fills(case, mode):
        exact('wgrad dense %s %s padding %g' % (case, mode, fill), run(case, mode, x, dy, fill), ref)
        if mode == 'bf16 storage':
            exact('wgrad dense %s %s padding %g variant 2' % (case, mode, fill), run(case, mode, x, dy, fill, variant=2), ref)


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('case', CASES)
def test_weight_gradient_is_exact_on_sparse_dy(case, mode):
    x, dy, ref = sparse_dy_case(case)
    for fill in fills(case, mode):
        exact('wgrad sparse dy %s %s padding %g' % (case, mode, fill), run(case, mode, x, dy, fill), ref)


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('case', CASES)
def test_weight_gradient_is_exact_on_sparse_x(case, mode):
    x, dy, ref = sparse_x_case(case)
    for fill in fills(case, mode):
        exact('wgrad sparse x %s %s padding %g' % (case, mode, fill), run(case, mode, x, dy, fill), ref)


# ---- random data ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('case', CASES)
def test_weight_gradient_distance_to_fp64(case, mode):
    x, dy = random_operands(case)
    r64, r32 = random_refs(case, mode in ('bf16', 'bf16 storage'))
    for fill in fills(case, mode):
        distance_ratio('wgrad %s %s padding %g' % (case, mode, fill), run(case, mode, x, dy, fill), r64, r32, MARGIN[mode])


# ---- phases, repetition, grouped reduction: bit for bit ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def first_run(case, mode):
    return run(case, mode, *random_operands(case))


def same_bits(tag, a, b):
    assert bool(torch.isfinite(a).all()), tag + ': non-finite values'
    ne = a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)
    assert not bool(ne.any()), '%s: %d of %d elements differ in their bits' % (tag, int(ne.sum()), a.numel())


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('case', CASES64)
def test_phases_and_a_second_run_are_bit_identical(case, mode):
    x, dy = random_operands(case)
    g = first_run(case, mode)
    same_bits('second run %s %s' % (case, mode), run(case, mode, x, dy), g)
    same_bits('phase 1 + phase 2 %s %s' % (case, mode), run(case, mode, x, dy, phases=True), g)


@pytest.mark.parametrize('mode', list(MODES))
def test_grouped_reduction_is_bit_identical_to_the_single_calls(mode):
    """Phase 1 of every case, then ONE dbn_wgrad_reduce_many over their records."""
    keep, jobs = [], []
    for case in CASES64:
        N, Ci, Co, k, s, p, H, W = case
        sm, big = device_operands(case, mode, *random_operands(case))
        slab, g, args = wgrad_t_call(sm, big, Co, Ci, k, s, p, MODES[mode][1], SCALE[case])
        _lib.check(L().dbn_wgrad_phase_t(1, *args, stream()), 'wgrad_phase_t(1)')
        job = _lib.WgradReduceJob()
        _lib.check(L().dbn_wgrad_reduce_describe(*args, ctypes.byref(job)), 'wgrad_reduce_describe')
        keep.append((sm, big, slab, g))
        jobs.append(job)
    # position-space slabs from the register-transposing kernel, natural ones from wgrad_patch_kernel and wgrad_tr_kernel
    assert {j.natural for j in jobs} == {'f32': {0}, 'bf16x3': {0, 1}, 'bf16': {0, 1}, 'bf16 storage': {1}}[mode]
    assert {j.RS for j in jobs} == {1, 4, 9, 16} and {j.G for j in jobs} == {1, 2, 3, 4, 7}
    first = [0]
    for j in jobs:
        first.append(first[-1] + j.blocks)
    table = torch.frombuffer(bytearray(bytes((_lib.WgradReduceJob * len(jobs))(*jobs))), dtype=torch.uint8).to(DEV)
    first_d = torch.tensor(first, dtype=torch.int32, device=DEV)
    _lib.check(L().dbn_wgrad_reduce_many(table.data_ptr(), first_d.data_ptr(), len(jobs), first[-1], max(j.smem_bytes for j in jobs), stream()),
               'wgrad_reduce_many')
    torch.cuda.synchronize()
    for case, (_, _, _, g) in zip(CASES64, keep):
        same_bits('grouped reduction %s %s' % (case, mode), g.cpu(), first_run(case, mode))
