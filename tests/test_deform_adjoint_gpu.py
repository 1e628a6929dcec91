"""-m gpu: the two adjoints of the deformable sampling (csrc/deform.hip) against the float64 reference of tests/deform_ref.py:
dbn_deform_col2im_gather_t (the per-pixel gather in plain fp32) and dbn_deform_col2im_t (the fixed-point scatter), on fp32, bf16 and fp16
storage, plus dbn_permute_weight.

Every output starts as NaN and every workspace as 0xff bytes (both entry points promise that it needs no initialisation); the offset map
has off_stride 64 with NaN in channels 18..63 (20 on the last shape), which the kernels must not read.

  * exact cases (deform_ref.EXACT_CASES): x and dcols integers in [-4, 4], offsets multiples of 1/4, so that every partial sum in every
    order is a float32 number (tests/test_deform_ref_cpu.py checks that premise case by case).  dx and doffset[..., :18] equal adjoint64 BIT
    FOR BIT, on 16-bit storage after its one rounding to the storage type; doffset[..., 18:] is exactly zero; the accumulate form gives
    round(base + adjoint64) on a dyadic base.  The generators aim at the kernels' index code: the position classes of edge_offsets with and
    without the far ones (whole-map search | finite window), integer offsets (taps exactly on the window's rim), a 15 x 15 window over
    three 96-pixel rounds, single far-travelling samples, every tap piled onto one point (27 hits per tap group: four hit batches), rows
    with wildly different trip counts side by side in one wave, and one offset just below / at / above the switch to the whole-map search;
  * all-zero dcols (the scatter's fixed_scale(0)) and dcols scaled by 2^40 and 2^-40 (its per-call scale): exact;
  * more work than one pass of each grid-stride loop (deform_ref.GRID_CASES), exact, against adjoint64 run on the GPU through torch;
  * random data: the distance to float64 against plain fp32's own (gpu_util.distance_ratio), on operands rounded to the storage type and
    bf16-valued offsets (every sample position is exact in fp32), one output rounding SR |ref64| + ETA allowed on 16-bit storage;
  * each form twice on one case: the same bits.

What the exact cases catch (scratch builds of deliberately wrong kernels, nothing of them kept): the gather's window lower bound tightened
by one tap fails 'integer' on every shape and 'quarter6'; its 96-pixel loop stopped after one round fails every generator but 'integer' on
the maps with more than 96 output pixels; hits beyond the first batch dropped fail every 'pile' and 'pile_rows' (and 'edges_near' on three
shapes); the scatter's out-of-patch path skipped fails 'edges', 'integer', 'quarter6', 'traveller' and the piles that leave a tile's patch.

The margins m of the random cases.  Per (form, quantity), m is twice the largest ratio measured on the MI355X over all random cases, rounded
up to a power of two, and never more than 16.  Each random test prints
    RATIO <form> <quantity> <shape> at=<at>: rms <ratio> max <ratio> (fp32 itself: rms <abs> max <abs>)
(pytest -rA shows them); the table holds "rms ratio / max ratio", one line per shape and storage type.

    shape (N, C, H, W, stride) and storage     gather dx  gather doffset    scatter dx  scatter doffset
    (2, 64, 9, 11, 1)            fp32       1.16 / 1.41     0.97 / 1.07     0.41 / 0.30     0.94 / 0.88
    (2, 64, 9, 11, 1)            bf16       0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    (2, 64, 9, 11, 1)            fp16       0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    (1, 128, 12, 10, 2)          fp32       1.04 / 1.06     0.86 / 0.90     0.60 / 0.36     0.77 / 0.73
    (1, 128, 12, 10, 2)          bf16       0.00 / 0.01     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    (1, 128, 12, 10, 2)          fp16       0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    (1, 192, 13, 9, 2)           fp32       1.02 / 0.89     0.89 / 0.71     0.57 / 0.32     0.81 / 0.62
    (1, 192, 13, 9, 2)           bf16       0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    (1, 192, 13, 9, 2)           fp16       0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    (1, 320, 7, 8, 1)            fp32       1.12 / 1.28     0.95 / 0.92     0.41 / 0.26     0.74 / 0.73
    (1, 320, 7, 8, 1)            bf16       0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    (1, 320, 7, 8, 1)            fp16       0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    (1, 512, 7, 8, 1)            fp32       1.09 / 1.37     0.93 / 1.06     0.41 / 0.29     0.72 / 0.74
    (1, 512, 7, 8, 1)            bf16       0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    (1, 512, 7, 8, 1)            fp16       0.00 / 0.00     0.02 / 0.14     0.00 / 0.00     0.00 / 0.00
    (1, 64, 21, 19, 1)           fp32       1.10 / 1.13     0.93 / 0.76     0.43 / 0.34     0.91 / 0.89
    (1, 64, 21, 19, 1)           bf16       0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    (1, 64, 21, 19, 1)           fp16       0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    (1, 64, 5, 4, 1)             fp32       1.06 / 1.15     0.95 / 1.05     0.48 / 0.50     0.96 / 0.85
    (1, 64, 5, 4, 1)             bf16       0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    (1, 64, 5, 4, 1)             fp16       0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    (1, 20, 6, 7, 1)             fp32       1.16 / 1.08     0.90 / 0.96     0.43 / 0.30     0.94 / 1.19
    (1, 20, 6, 7, 1)             bf16       0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    (1, 20, 6, 7, 1)             fp16       0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    gather dx 1.41 -> m = 4      gather doffset 1.07 -> m = 4      scatter dx 0.60 -> m = 2      scatter doffset 1.19 -> m = 4

On 16-bit storage nearly everything is 0: what is left after the one output rounding is taken off.  The gather sits at 1.0 - 1.4 times
plain fp32's own distance, as a sum of fp32 products in one fixed order should.  The scatter's dx sits at 0.3 - 0.6: its sum is exact
(fixed point) and rounded once, so only the rounding of the weights and products remains, as expected; its doffset is a fp32 shuffle tree
over the channels before it goes to fixed point, and sits with the gather's at about 1.
"""
import functools

import pytest
import torch

import deform_ref as D
from gpu_util import DEV, DT, ETA, NAN, SR, L, distance_ratio, exact, stream
from db_text_minimal_amd import _lib

pytestmark = pytest.mark.gpu

FORMS = ('gather', 'scatter')
# twice the largest ratio of the table in the module docstring, rounded up to a power of two
MARGIN = {('gather', 'dx'): 4, ('gather', 'doffset'): 4, ('scatter', 'dx'): 2, ('scatter', 'doffset'): 4}
assert max(MARGIN.values()) <= 16


def run(form, at, x, offs, dcols, stride, base=None):
    """One launch of an adjoint on device tensors in the storage type DT[at]: x [N, H, W, C], offs [N, Ho, Wo, off_stride],
    dcols [N, Ho, Wo, 9, C] -> (dx, doffset).  base: the accumulate form, dx starts as base."""
    N, H, W, C = x.shape
    _, Ho, Wo, os_ = offs.shape
    assert (Ho, Wo) == D.out_size(H, W, stride) and dcols.shape == (N, Ho, Wo, 9, C)
    assert x.dtype == offs.dtype == dcols.dtype == DT[at] and x.is_contiguous() and offs.is_contiguous() and dcols.is_contiguous()
    dx = torch.full((N, H, W, C), NAN, device=DEV, dtype=DT[at]) if base is None else base.clone()
    doff = torch.full((N, Ho, Wo, os_), NAN, device=DEV, dtype=DT[at])
    if form == 'gather':
        nbytes, fn = L().dbn_deform_col2im_gather_ws_bytes(N, Ho, Wo), L().dbn_deform_col2im_gather_t
    else:
        nbytes, fn = L().dbn_deform_col2im_ws_bytes(N, H, W, C, Ho, Wo, 3, 3), L().dbn_deform_col2im_t
    ws = torch.empty(nbytes, device=DEV, dtype=torch.uint8).fill_(0xff)
    _lib.check(fn(at, dcols.data_ptr(), x.data_ptr(), offs.data_ptr(), dx.data_ptr(), doff.data_ptr(), 0 if base is None else 1, ws.data_ptr(),
                  N, H, W, C, Ho, Wo, 3, 3, stride, 1, os_, stream()), 'deform adjoint ' + form)
    torch.cuda.synchronize()
    return dx, doff


@functools.lru_cache(maxsize=None)
def exact_data(si, name, at):
    """The case in the storage type and its float64 adjoint, on the CPU; shared by the forms and never modified."""
    shape = D.SHAPES[si]
    x, off, dcols = D.exact_case(shape, name, at)
    x, dcols, offs = x.to(DT[at]), dcols.to(DT[at]), D.stored_offsets(off, D.off_stride_of(shape), DT[at])
    dx64, do64 = D.adjoint64(x, offs, dcols, shape[4])
    return x, offs, dcols, dx64, do64


def check_exact(tag, at, dx, doff, dx64, do64):
    exact(tag + ' dx', dx, dx64.to(DT[at]))
    exact(tag + ' doffset', doff[..., :18], do64.to(DT[at]))
    pad = doff[..., 18:].float()
    assert not bool((pad != 0).any()), tag + ': a padding channel of doffset is not zero'


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('at', [0, 1, 2])
@pytest.mark.parametrize('si,name', D.EXACT_CASES)
def test_exact_cases(si, name, at, form):
    """dx and doffset equal adjoint64 (rounded once to the storage type), plain and accumulated onto a dyadic base."""
    shape = D.SHAPES[si]
    x, offs, dcols, dx64, do64 = exact_data(si, name, at)
    x, offs, dcols = x.to(DEV), offs.to(DEV), dcols.to(DEV)
    tag = '%s %s %s at=%d' % (form, shape, name, at)
    dx, doff = run(form, at, x, offs, dcols, shape[4])
    check_exact(tag, at, dx, doff, dx64, do64)
    g = torch.Generator().manual_seed(si)
    base = (torch.randint(-63, 64, dx64.shape, generator=g).float() / 16).to(DT[at])  # multiples of 1/16 below 4: base + dx is a float32 number
    dx, doff = run(form, at, x, offs, dcols, shape[4], base=base.to(DEV))
    check_exact(tag + ' accumulate', at, dx, doff, base.double() + dx64, do64)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('at', [0, 1, 2])
@pytest.mark.parametrize('si', [0, 1])
def test_zero_dcols_give_zero(si, at, form):
    """All-zero dcols: all-zero, finite outputs (the scatter's scale of a zero maximum)."""
    shape = D.SHAPES[si]
    x, offs, dcols, dx64, do64 = exact_data(si, 'edges_near', at)
    dx, doff = run(form, at, x.to(DEV), offs.to(DEV), torch.zeros_like(dcols).to(DEV), shape[4])
    check_exact('%s %s zero dcols at=%d' % (form, shape, at), at, dx, doff, torch.zeros_like(dx64), torch.zeros_like(do64))


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('e', [40, -40])
@pytest.mark.parametrize('si', [0, 1, 5])
def test_scaled_dcols_scale_the_result(si, e, form):
    """fp32: dcols times 2^40 or 2^-40 gives the exactly scaled result (the scatter takes its fixed-point scale per call from max |dcols|)."""
    shape = D.SHAPES[si]
    x, offs, dcols, dx64, do64 = exact_data(si, 'edges_near', 0)
    dx, doff = run(form, 0, x.to(DEV), offs.to(DEV), (dcols * 2.0**e).to(DEV), shape[4])
    check_exact('%s %s dcols * 2^%d' % (form, shape, e), 0, dx, doff, dx64 * 2.0**e, do64 * 2.0**e)


@functools.lru_cache(maxsize=None)
def random_data(si, at):
    shape = D.SHAPES[si]
    N, C, H, W, stride = shape
    Ho, Wo = D.out_size(H, W, stride)
    g = torch.Generator().manual_seed(77 + si)
    x = torch.randn(N, H, W, C, generator=g).to(DT[at])
    dcols = torch.randn(N, Ho, Wo, 9, C, generator=g).to(DT[at])
    sd = 6.0 if (H, W) == (21, 19) else 1.5
    off = (torch.randn(N, Ho, Wo, 18, generator=g) * sd).to(torch.bfloat16).float()  # (bf16-valued: the positions are exact in fp32)
    offs = D.stored_offsets(off, D.off_stride_of(shape), DT[at])
    return x, offs, dcols, D.adjoint64(x, offs, dcols, stride), D.adjoint32(x, offs, dcols, stride)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('at', [0, 1, 2])
@pytest.mark.parametrize('si', range(len(D.SHAPES)))
def test_random_vs_fp64(si, at, form):
    """Gaussian data: no further from float64 than MARGIN times plain fp32 (after the one output rounding on 16-bit storage)."""
    shape = D.SHAPES[si]
    x, offs, dcols, (dx64, do64), (dx32, do32) = random_data(si, at)
    dx, doff = run(form, at, x.to(DEV), offs.to(DEV), dcols.to(DEV), shape[4])
    allow = (lambda r: SR[at] * r.abs() + ETA[at]) if at else (lambda r: None)
    distance_ratio('%s dx %s at=%d' % (form, shape, at), dx, dx64, dx32, MARGIN[form, 'dx'], allow(dx64))
    distance_ratio('%s doffset %s at=%d' % (form, shape, at), doff[..., :18], do64, do32, MARGIN[form, 'doffset'], allow(do64))
    assert not bool((doff[..., 18:].float() != 0).any())


@functools.lru_cache(maxsize=1)
def grid_data(shape, at):
    """The grid case on the device and its float64 adjoint, run there through torch (one entry: the two forms of a case follow each other)."""
    x, off, dcols = D.grid_case(shape)
    x, dcols, offs = x.to(DT[at]).to(DEV), dcols.to(DT[at]).to(DEV), D.stored_offsets(off, 64, DT[at]).to(DEV)
    dx64, do64 = D.adjoint64(x, offs, dcols, shape[4], dev=DEV)
    return x, offs, dcols, dx64, do64


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('at', [0, 1])
@pytest.mark.parametrize('shape', D.GRID_CASES)
def test_beyond_one_grid_pass(shape, at, form):
    """Exact data, edges_near offsets.  (8, 64, 100, 100): 720 000 sample teams, more than the 2^16 x 8 of one pass of deform_doffset_kernel,
    and 46 M / 4 column quads, more than the 2048 x 256 of one pass of the scatter's absmax.  (53, 4, 100, 100): 530 000 output pixels, more
    than the 2048 x 256 threads of one pass of deform_bbox_kernel."""
    x, offs, dcols, dx64, do64 = grid_data(shape, at)
    dx, doff = run(form, at, x, offs, dcols, shape[4])
    check_exact('%s %s at=%d' % (form, shape, at), at, dx, doff, dx64, do64)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('at', [0, 1, 2])
def test_run_to_run_identity(at, form):
    """Gaussian data under quarter6 offsets on the 21 x 19 map, twice: the same bits."""
    shape = D.SHAPES[5]
    N, C, H, W, stride = shape
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, H, W, C, generator=g).to(DT[at]).to(DEV)
    dcols = torch.randn(N, H, W, 9, C, generator=g).to(DT[at]).to(DEV)
    offs = D.stored_offsets(D.offsets('quarter6', shape, g), 64, DT[at]).to(DEV)
    bits = torch.int32 if at == 0 else torch.int16
    a, b = run(form, at, x, offs, dcols, stride), run(form, at, x, offs, dcols, stride)
    assert bool(torch.isfinite(a[0].float()).all()) and bool(torch.isfinite(a[1].float()).all())
    assert torch.equal(a[0].view(bits), b[0].view(bits)) and torch.equal(a[1].view(bits), b[1].view(bits)), form + ': two runs differ'


@pytest.mark.parametrize('scale', [1.0, 0.25])
@pytest.mark.parametrize('O_,C,T', [(64, 64, 9), (3, 20, 9), (256, 4, 1)])
def test_permute_weight_bits(O_, C, T, scale):
    """dbn_permute_weight, both directions, against a torch permute bit for bit (a power-of-two scale is exact), and the round trip."""
    g = torch.Generator().manual_seed(O_ + C + T)
    w = torch.randn(O_, C, T, generator=g).to(DEV)  # OIHW, the taps flattened
    bits = lambda t: t.contiguous().view(torch.int32)

    def permute(src, to_ohwi, s):
        dst = torch.full((O_, T, C) if to_ohwi else (O_, C, T), NAN, device=DEV)
        _lib.check(L().dbn_permute_weight(src.data_ptr(), dst.data_ptr(), O_, C, T, to_ohwi, s, stream()), 'permute_weight')
        torch.cuda.synchronize()
        return dst

    ohwi = permute(w, 1, scale)
    assert torch.equal(bits(ohwi), bits(w.permute(0, 2, 1) * scale))
    back = permute(ohwi, 0, scale)
    assert torch.equal(bits(back), bits(ohwi.permute(0, 2, 1) * scale))
    assert torch.equal(bits(permute(permute(w, 1, scale), 0, 1 / scale)), bits(w)), 'the round trip is not the identity'
