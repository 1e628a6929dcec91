"""-m gpu: the FPN output conv — the pyramid form (MODE 3 of csrc/igemm_kernel.h: dbn_pyramid_conv_f32 / _from_t / _act_t), its combined
filters (dbn_fpn_combine_weights, dbn_fpn_scatter_wgrad) and its per-level gradients (mode 0 at k = f + 2, stride f; dbn_wgrad_t) — against
the float64 reference of tests/fpn_ref.py, the way tests/test_conv_fp64_gpu.py pins the plain modes.

Shapes (N, H, W, Cg, Co), the smallest at which each seam of the kernel's walk exists (M = N H/8 W/8 blocks of 8 x 8 pixels, row tiles of 128
blocks times 64 pixel classes):
  (3, 56, 64, 16, 128)  168 blocks: the tile boundary falls inside image 2, the last tile is ragged (40 blocks), image boundaries inside tile 0,
                        level 3 is 7 x 8
  (3, 56, 64, 16, 256)  the same on the 128 x 256 tile of the 16-bit storage types (dbn_set_pyramid_wide(3) against (0))
  (2, 16, 24, 64, 256)  K = 2304
  (1, 8, 40, 32, 128)   level 3 is one pixel high: every vertical halo is padding
  (2, 24, 40, 64, 128)  gradients only (with (2, 16, 24, 64, 256)): the data gradient's Cd is Cg, a multiple of 64
Every output buffer starts as NaN.

Kinds of case:
  * random data (weights on a 2^-10 grid, so that the combined filters are exact in fp32 and the 16-bit modes see the rounding of a known
    number): gpu_util.distance_ratio against plain fp32 on the operands as the kernel sees them — F.conv2d of the concatenation for f32 and
    bf16x3, the fp32 sum of F.conv_transpose2d over the rounded combined filters where the kernel rounds those (bf16, 16-bit storage; that sum
    has no concat form).  16-bit storage: one output rounding SR |ref64| + ETA is taken off first, and for first_level = 1 also the rounding
    SR |level 0 + bias| + ETA of the part the level-0 launch stored;
  * exact dyadic data, dense and impulses on fpn_ref.seam_sources per level: equal to float64 BIT FOR BIT in every mode and form (16-bit
    storage: to float64 rounded once to the storage type; first_level = 1: with the level-0 part rounded first; the bf16 modes: on
    bf16_rne(combine(w)) per level, which tests/test_fpn_ref_cpu.py shows is what they must see);
  * the fused BatchNorm statistics: on a constant map (x = 0: y = bias on every pixel, so a padding row of the ragged tile that was counted
    moves the mean, the variance or the count) and on random data within stats_bounds below;
  * combine / scatter bit for bit on dyadic weights and within the bound of a serial fp32 chain on random ones.

Forms: without statistics, with statistics, the ReLU form dbn_pyramid_conv_act_t; first_level 0 and 1 (fp32: level 0 written by
dbn_winograd_conv_bn_f32 as the engine does; 16-bit storage: by the mode-1 3 x 3 launch on the level-0 panel); both tiles on 16-bit storage.
DBN_PYR_GROUP (the tile order of the wide tile, read once from the environment, no setter) is not exercised here.

The margins m, by the rule of tests/test_conv_fp64_gpu.py: per mode twice the largest ratio measured on the MI355X over all cases, rounded up
to a power of two, capped at 16.  Each random-data launch prints a line "RATIO <operation> <shape> <mode> ...: rms <ratio> max <ratio>"
(pytest -rA).  "rms ratio / max ratio", the worst over forms, tiles and first_level of a row:

    operation and case                                         f32        bf16x3          bf16  bf16 storage  fp16 storage
    pyramid (3, 56, 64, 16, 128)                       1.06 / 1.58   0.60 / 0.81   1.05 / 1.37   0.00 / 0.05   0.00 / 0.23
    pyramid (3, 56, 64, 16, 256)                       1.06 / 1.58   0.60 / 0.81   1.05 / 1.12   0.00 / 0.09   0.00 / 0.23
    pyramid (2, 16, 24, 64, 256)                       1.97 / 3.65   1.11 / 2.83   1.38 / 2.40   0.00 / 0.09   0.01 / 0.14
    pyramid (1, 8, 40, 32, 128)                        1.42 / 2.22   0.80 / 1.19   1.15 / 2.22   0.00 / 0.00   0.02 / 0.45
    fpn dgrad (2, 24, 40, 64, 128) level 0             2.72 / 4.79   1.46 / 2.47   1.59 / 2.06             -             -
    fpn dgrad (2, 24, 40, 64, 128) level 0 split-K     1.92 / 2.75   1.04 / 1.92   1.13 / 1.59             -             -
    fpn dgrad (2, 24, 40, 64, 128) level 1             3.56 / 6.70   2.00 / 4.01   2.19 / 3.56             -             -
    fpn dgrad (2, 24, 40, 64, 128) level 1 split-K     1.77 / 1.98   0.99 / 1.25   1.07 / 1.12             -             -
    fpn dgrad (2, 24, 40, 64, 128) level 2             5.08 / 9.10   3.06 / 5.76   2.79 / 4.40             -             -
    fpn dgrad (2, 24, 40, 64, 128) level 2 split-K     1.73 / 1.94   1.03 / 1.52   0.90 / 0.96             -             -
    fpn dgrad (2, 24, 40, 64, 128) level 3            8.42 / 15.17   5.17 / 8.15   3.10 / 6.23             -             -
    fpn dgrad (2, 24, 40, 64, 128) level 3 split-K     1.67 / 2.00   1.10 / 1.31   0.66 / 0.61             -             -
    fpn dgrad (2, 16, 24, 64, 256) level 0             3.74 / 6.03   2.02 / 3.77   1.90 / 3.40             -             -
    fpn dgrad (2, 16, 24, 64, 256) level 0 split-K     1.87 / 2.26   1.01 / 1.12   0.96 / 0.97             -             -
    fpn dgrad (2, 16, 24, 64, 256) level 1             4.79 / 6.51   2.73 / 4.22   2.71 / 4.33             -             -
    fpn dgrad (2, 16, 24, 64, 256) level 1 split-K     1.71 / 1.64   0.98 / 1.16   0.97 / 0.88             -             -
    fpn dgrad (2, 16, 24, 64, 256) level 2            7.15 / 10.70   4.32 / 4.78   3.89 / 6.50             -             -
    fpn dgrad (2, 16, 24, 64, 256) level 2 split-K     1.69 / 1.57   1.03 / 0.82   0.93 / 0.95             -             -
    fpn dgrad (2, 16, 24, 64, 256) level 3           10.45 / 15.41  7.28 / 14.58   4.55 / 6.24             -             -
    fpn dgrad (2, 16, 24, 64, 256) level 3 split-K     1.78 / 2.22   1.19 / 1.54   0.81 / 0.71             -             -
    fpn wgrad (2, 24, 40, 64, 128)                     0.40 / 0.33   0.34 / 0.23   0.35 / 0.30             -             -
    fpn wgrad (2, 16, 24, 64, 256)                     0.49 / 0.48   0.43 / 0.49   0.54 / 0.50             -             -
    f32 15.41 -> m = 16      bf16x3 14.58 -> m = 16      bf16 6.50 -> m = 16      bf16 storage 0.09 -> m = 0.25      fp16 storage 0.45 -> m = 1

The pyramid launches keep fp32's own distance (at most 2.0 rms / 3.7 max, at K = 2304), first_level = 1 included (Winograd level 0: 0.8 / 2.6),
and on 16-bit storage nothing but the output rounding is left.  The weight gradient is closer to float64 than fp32 (its slabs are added in
float64).  A finding: the UNSPLIT data gradient (ksplit 1) grows with K along its one MFMA accumulator chain, from 2.7 / 4.8 at level 0 to
10.5 / 15.4 at level 3 (k = 10, stride 8: K = 100 Co = 25 600 products per output) — twice that is beyond the cap, so f32 and bf16x3 stand AT
the cap of 16 without the factor of two of the rule.  It is the order of summation, not lost bits: the split-K launch the library itself
plans for these geometries (25 and 50 splits at level 3, slabs added in a fixed order; the engine runs that one) sits at 1.8 / 2.2, the
bf16 mode, whose products are exact, follows the same growth (3.1-4.6 / 6.5), and both launches are bit-exact on the dyadic sets below.
(Kernels, seeds and the CPU reference are deterministic — fp32 autograd's own error does not move with the thread count — and the figures
repeated to the last digit between runs.)
The data gradients take their panels from fpn_ref.combine (equal to dbn_fpn_combine_weights bit for bit on these weights, which
test_combine_* shows), so a failure there names the conv; the forward launches take the library's own combined filters, as the engine does."""
import functools

import pytest
import torch
import torch.nn.functional as F

import conv_ref as R
import fpn_ref as P
from gpu_util import (DEV, ETA, L, NAN, SR, U, distance_ratio, exact, igemm, igemm_t, nchw, nhwc, pack, pack_t, rnd, stream, wgrad_t, within)
from db_text_minimal_amd import _lib

pytestmark = pytest.mark.gpu

FWD_SHAPES = [(3, 56, 64, 16, 128), (3, 56, 64, 16, 256), (2, 16, 24, 64, 256), (1, 8, 40, 32, 128)]
RAGGED_SHAPES = FWD_SHAPES[:2]
GRAD_SHAPES = [(2, 24, 40, 64, 128), (2, 16, 24, 64, 256)]
NS = {'f32': 0, 'bf16x3': 3, 'bf16': 1, 'bf16 storage': 1, 'fp16 storage': 1}
AT = {'f32': 0, 'bf16x3': 0, 'bf16': 0, 'bf16 storage': 1, 'fp16 storage': 2}
DTYPE = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
MODES = list(NS)
GRAD_MODES = MODES[:3]
FORMS = ('plain', 'stats', 'relu')
# margins m of the random-data tests: per mode, twice the largest ratio of the table in the module docstring, rounded up to a power of two, capped
# at 16 (f32 and bf16x3 are capped: see the finding there)
MARGIN = {'f32': 16, 'bf16x3': 16, 'bf16': 16, 'bf16 storage': 0.25, 'fp16 storage': 1}
assert max(MARGIN.values()) <= 16
EPS, MOM = 1e-5, 0.1


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def seen(t, mode):
    """An activation as the kernel's products see it (float32 values)."""
    if mode == 'bf16':
        return R.bf16_rne(t.float())
    return t.float().to(DTYPE[AT[mode]]).float()


def seen_w(wc, mode):
    """A combined filter as the products see it: the panels of the 16-bit modes hold it rounded once."""
    if mode in ('bf16', 'bf16 storage'):
        return R.bf16_rne(wc.float())
    return wc.float().half().float() if mode == 'fp16 storage' else wc.float()


def firsts(mode):
    """first_level = 1 exists in exact fp32 and on 16-bit storage (include/dbnet_hip.h)."""
    return (0, ) if mode in ('bf16x3', 'bf16') else (0, 1)


def wides(mode, Co):
    """dbn_set_pyramid_wide settings to run: both tiles where the 128 x 256 tile exists (16-bit storage, Cd % 256 == 0)."""
    return (0, 3) if AT[mode] and Co % 256 == 0 else (0, )


# ---- launches -----------------------------------------------------------------------------------------------------------------------
def combine_gpu(w, Cin, g, Cg):
    """dbn_fpn_combine_weights of a CPU weight [Co, Cin, 3, 3] -> device [Cg, Co, k, k]."""
    Co, k = w.shape[0], (1 << g) + 2
    wd = nan(Cg, Co, k, k)
    _lib.check(L().dbn_fpn_combine_weights(w.float().contiguous().to(DEV).data_ptr(), Co, Cin, g, Cg, wd.data_ptr(), stream()), 'combine')
    return wd


def scatter_gpu(ts, Co, Cg):
    dw = nan(Co, 4 * Cg, 3, 3)
    _lib.check(L().dbn_fpn_scatter_wgrad(*[t.data_ptr() for t in ts], Co, Cg, dw.data_ptr(), stream()), 'scatter')
    return dw.cpu()


class Launch:
    """The device side of one (levels, weights, bias, mode): typed NHWC levels, the combined filters (dbn_fpn_combine_weights, as the engine
    makes them) and their mode-1 panels.  run() launches one form into a NaN-filled output."""

    def __init__(self, shape, ps, w, b, mode):
        self.shape, self.mode, self.at, self.ns = shape, mode, AT[mode], NS[mode]
        N, H, W, Cg, Co = shape
        self.dtype = DTYPE[self.at]
        self.set_levels(ps)
        self.wds = [combine_gpu(w, 4 * Cg, g, Cg) for g in range(4)]
        if self.at:
            self.wpk = [pack_t(wd.cpu(), 1, 1 << g, self.at) for g, wd in enumerate(self.wds)]
        else:
            self.wpk = [pack(wd.cpu(), 1, 1 << g, self.ns) for g, wd in enumerate(self.wds)]
        self.bias = None if b is None else b.float().to(DEV)
        self.level0 = ''

    def set_levels(self, ps):
        self.xs = [nhwc(p.float()).to(self.dtype) for p in ps]

    def write_level0(self, y):
        N, H, W, Cg, Co = self.shape
        bp = None if self.bias is None else self.bias.data_ptr()
        if self.at:
            igemm_t(self.xs[0], self.wpk[0], self.bias, y, 3, 1, 1, 1)
            self.level0 = 'mode-1 3x3'
        elif L().dbn_winograd_eligible(N, H, W, Cg, Co):
            # (wds[0][ci][co][u][v] = W[co][ci][2 - u][2 - v]: its data-gradient panel is the forward conv of W's first Cg input channels)
            up = nan(L().dbn_winograd_panel_floats(Co, Cg))
            _lib.check(L().dbn_winograd_pack(self.wds[0].data_ptr(), Co, Cg, Cg, 1, up.data_ptr(), stream()), 'winograd pack')
            _lib.check(L().dbn_winograd_conv_bn_f32(self.xs[0].data_ptr(), up.data_ptr(), bp, y.data_ptr(), N, H, W, Cg, Co, None, None, 0.0, 0.0,
                                                    None, None, None, None, None, None, None, stream()), 'winograd level 0')
            self.level0 = 'winograd'
        else:  # a map the Winograd kernel does not take: the engine then runs first_level = 0; here the direct 3 x 3 launch writes level 0
            igemm(self.xs[0], self.wpk[0], self.bias, y, 3, 1, 1, 1)
            self.level0 = 'direct 3x3'

    def run(self, form='plain', first=0, wide=0, bn=None):
        """-> (y as CPU NCHW float32, statistics dict or None).  bn = (gamma, beta, run_mean, run_var) on the CPU for form 'stats'."""
        N, H, W, Cg, Co = self.shape
        old = L().dbn_set_pyramid_wide(wide)
        try:
            y = nan(N, H, W, Co, dtype=self.dtype)
            if first:
                self.write_level0(y)
            ptrs = [t.data_ptr() for t in self.xs] + [t.data_ptr() for t in self.wpk] + [None if self.bias is None else self.bias.data_ptr()]
            st = None
            if form == 'relu':
                _lib.check(L().dbn_pyramid_conv_act_t(first, self.at, *ptrs, 1, y.data_ptr(), N, H, W, Cg, Co, self.ns, stream()), 'pyramid_act')
            else:
                bnargs = (None, None, 0.0, 0.0) + (None, ) * 7
                if form == 'stats':
                    g_, b_, rm_, rv_ = (t.float().clone().to(DEV) for t in bn)
                    sc, sh, mu, rs = nan(Co), nan(Co), nan(Co), nan(Co)
                    ws = nan(L().dbn_pyramid_conv_ws_floats(N, H, W, Co))
                    bnargs = (g_.data_ptr(), b_.data_ptr(), EPS, MOM, rm_.data_ptr(), rv_.data_ptr(), sc.data_ptr(), sh.data_ptr(), mu.data_ptr(),
                              rs.data_ptr(), ws.data_ptr())
                if self.at == 0 and first == 0:
                    _lib.check(L().dbn_pyramid_conv_f32(*ptrs, y.data_ptr(), N, H, W, Cg, Co, 0, self.ns, *bnargs, stream()), 'pyramid')
                else:
                    _lib.check(L().dbn_pyramid_conv_from_t(first, self.at, *ptrs, y.data_ptr(), N, H, W, Cg, Co, 0, self.ns, *bnargs, stream()),
                               'pyramid_from')
                if form == 'stats':
                    torch.cuda.synchronize()
                    st = dict(mean=mu.cpu(), rstd=rs.cpu(), scale=sc.cpu(), shift=sh.cpu(), run_mean=rm_.cpu(), run_var=rv_.cpu())
            return nchw(y.float()), st
        finally:
            L().dbn_set_pyramid_wide(old)


def bn_params(Co, seed=60):
    return rnd(Co, seed=seed) * 0.3 + 1, rnd(Co, seed=seed + 1), rnd(Co, seed=seed + 2), rnd(Co, seed=seed + 3).abs() + 0.5


def variants(mode, Co):
    return [(form, first, wide) for wide in wides(mode, Co) for first in firsts(mode) for form in FORMS]


def rounded(ref, y0, mode, first):
    """The float64 result as the storage type holds it: rounded once — and with first_level = 1 the level-0 part (y0, bias included) first."""
    dt = DTYPE[AT[mode]]
    if first:
        ref = y0.to(dt).double() + (ref - y0)
    return ref.to(dt).double()


def tag_of(what, shape, mode, form, first, wide, level0=''):
    return '%s %s %s %s first %d%s wide %d' % (what, shape, mode, form, first, ' (%s)' % level0 if first else '', wide)


# ---- combine and scatter ------------------------------------------------------------------------------------------------------------
COMBINE_CASES = [(128, 64, 16), (256, 256, 64), (128, 96, 32)]  # Co, Cin, Cg; the last has three groups only


@pytest.mark.parametrize('case', COMBINE_CASES)
def test_combine_is_exact_on_dyadic_weights_and_within_a_serial_chain_on_random_ones(case):
    """acc = 0, then up to 9 additions in fp32: |got - ref64| <= 9 u sum |taps| (the sum in float64); dyadic weights: no rounding at all."""
    Co, Cin, Cg = case
    wr = rnd(Co, Cin, 3, 3, seed=3, scale=0.03)
    for g in range(min(4, Cin // Cg)):
        for name, w in (('dense', R.dense_w((Co, Cin, 3, 3), 71)), ('distinct', R.distinct_w(Co, Cin, 3, 3)), ('grid', P.grid_w((Co, Cin, 3, 3), 72))):
            exact('combine %s %s level %d' % (name, case, g), combine_gpu(w, Cin, g, Cg), P.combine(w, g, Cg))
        within('combine random %s level %d' % (case, g), combine_gpu(wr, Cin, g, Cg), P.combine(wr.double(), g, Cg), 9 * U * P.combine(wr.double().abs(), g, Cg))


@pytest.mark.parametrize('case', [(128, 16), (256, 64), (128, 32)])
def test_scatter_is_exact_on_dyadic_data_and_within_a_serial_chain_on_random_data(case):
    """Per (r, s) of level g the kernel adds f x f entries in fp32: |got - ref64| <= (f^2 + 1) u sum |t|."""
    Co, Cg = case
    td = [R.dense_x((Cg, Co, (1 << g) + 2, (1 << g) + 2), 80 + g) for g in range(4)]
    exact('scatter dense %s' % (case, ), scatter_gpu([t.float().to(DEV) for t in td], Co, Cg), P.scatter(td, Co, Cg))
    tr = [rnd(Cg, Co, (1 << g) + 2, (1 << g) + 2, seed=90 + g) for g in range(4)]
    zero = [torch.zeros_like(t, dtype=torch.float64) for t in tr]
    bound = sum(((1 << g)**2 + 1) * U * P.scatter([tr[l].double().abs() if l == g else zero[l] for l in range(4)], Co, Cg) for g in range(4))
    within('scatter random %s' % (case, ), scatter_gpu([t.to(DEV) for t in tr], Co, Cg), P.scatter([t.double() for t in tr], Co, Cg), bound)


# ---- pyramid forward: random data -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_case(shape, mode):
    """Operands as handed to the kernel, the float64 reference on the operands the products see (its level-0 part apart) and plain fp32."""
    N, H, W, Cg, Co = shape
    ps = [rnd(N, Cg, H >> g, W >> g, seed=10 + g) for g in range(4)]
    w, b = P.grid_w((Co, 4 * Cg, 3, 3), 3), rnd(Co, seed=5)
    pso = [seen(p, mode) for p in ps]
    wco = [seen_w(P.combine(w, g, Cg), mode) for g in range(4)]
    ref64 = P.transposed_sum([p.double() for p in pso], [t.double() for t in wco], b.double())
    y0 = P.transposed_sum([pso[0].double()], [wco[0].double()], b.double())
    if mode in ('f32', 'bf16x3'):
        ref32 = F.conv2d(P.concat(pso), w.float(), b, 1, 1)
    else:
        ref32 = b.view(1, Co, 1, 1) + sum(F.conv_transpose2d(pso[g], wco[g], None, 1 << g, 1) for g in range(4))
    return ps, w, b, ref64, y0, ref32


def allowance(ref64, y0, mode, first):
    at = AT[mode]
    if at == 0:
        return None
    a = SR[at] * ref64.abs() + ETA[at]
    return a + SR[at] * y0.abs() + ETA[at] if first else a


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', FWD_SHAPES)
def test_pyramid_distance_to_fp64(shape, mode):
    N, H, W, Cg, Co = shape
    ps, w, b, ref64, y0, ref32 = random_case(shape, mode)
    run = Launch(shape, ps, w, b, mode)
    bn = bn_params(Co)
    for form, first, wide in variants(mode, Co):
        y, _ = run.run(form, first, wide, bn)
        r64, r32 = (ref64.clamp_min(0), ref32.clamp_min(0)) if form == 'relu' else (ref64, ref32)
        distance_ratio(tag_of('pyramid', shape, mode, form, first, wide, run.level0), y, r64, r32, MARGIN[mode], allowance(ref64, y0, mode, first))


# ---- pyramid forward: exact data ------------------------------------------------------------------------------------------------------
def check_exact(what, run, shape, mode, ref, y0):
    Co = shape[4]
    bn = bn_params(Co)
    for form, first, wide in variants(mode, Co):
        y, _ = run.run(form, first, wide, bn)
        want = rounded(ref, y0, mode, first) if AT[mode] else ref
        exact(tag_of(what, shape, mode, form, first, wide, run.level0), y, want.clamp_min(0) if form == 'relu' else want)


@functools.lru_cache(maxsize=None)
def dense_case(shape):
    N, H, W, Cg, Co = shape
    ps, w, b = P.dense_operands(shape)
    return ps, w, b, P.concat_conv(ps, w, b), R.conv2d(ps[0], w[:, :Cg], b, 1, 1)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', FWD_SHAPES)
def test_pyramid_is_exact_on_dense_dyadic_data(shape, mode):
    ps, w, b, ref, y0 = dense_case(shape)
    check_exact('pyramid dense', Launch(shape, ps, w, b, mode), shape, mode, ref, y0)


@functools.lru_cache(maxsize=None)
def distinct_combined(Co, Cg):
    w = R.distinct_w(Co, 4 * Cg, 3, 3)
    return w, [P.combine(w, g, Cg) for g in range(4)]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', FWD_SHAPES)
def test_pyramid_is_exact_on_seam_impulses(shape, mode):
    """Impulses under every seam of the walk, in one level at a time (fpn_ref.seam_sources), weights that differ per (co, ci, tap)."""
    N, H, W, Cg, Co = shape
    w, wcs = distinct_combined(Co, Cg)
    b = R.dense_bias(Co, 13)
    wco = [seen_w(t, mode).double() for t in wcs]
    run = Launch(shape, P.seam_levels(shape, 0), w, b, mode)
    for g in range(4):
        ps = P.seam_levels(shape, g)
        run.set_levels(ps)
        check_exact('pyramid seams level %d' % g, run, shape, mode, P.transposed_sum(ps, wco, b), P.transposed_sum(ps[:1], wco[:1], b))


# ---- the fused statistics -------------------------------------------------------------------------------------------------------------
def ulps(a, b):
    """Distance of two fp32 tensors in units of the last place of b."""
    return float(((a.double() - b.double()).abs() / (b.abs().double() * 2.0**-23)).max())


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', RAGGED_SHAPES)
def test_statistics_of_a_constant_map_on_a_ragged_tile(shape, mode):
    """x = 0: y = bias on every pixel.  Every tile's pivot is the bias and its sums are 0, so save_mean is the bias bit for bit, the variance
    0 (save_rstd = 1 / sqrt(eps) to 2 ulp), run_var' = (1 - momentum) run_var bit for bit — unless a padding row of the ragged tile (acc = 0,
    not the bias) was counted, or the count row is off.  first_level = 1 on 16-bit storage: the stored level-0 part is the rounded bias."""
    N, H, W, Cg, Co = shape
    ps = [torch.zeros(N, Cg, H >> g, W >> g) for g in range(4)]
    w, b = P.grid_w((Co, 4 * Cg, 3, 3), 3), rnd(Co, seed=5)
    gamma, beta, rm, rv = bn = bn_params(Co)
    run = Launch(shape, ps, w, b, mode)
    one_m = torch.tensor(1.0) - torch.tensor(MOM, dtype=torch.float32)
    for first in firsts(mode):
        for wide in wides(mode, Co):
            y, st = run.run('stats', first, wide, bn)
            tag = tag_of('constant map', shape, mode, 'stats', first, wide, run.level0)
            bias = b.to(DTYPE[AT[mode]]).float() if first and AT[mode] else b
            exact(tag + ' y', y, bias.to(DTYPE[AT[mode]]).double().view(1, Co, 1, 1).expand(N, Co, H, W))
            exact(tag + ' save_mean', st['mean'], bias)
            rstd = torch.full((Co, ), 1.0 / (0.0 + float(torch.tensor(EPS, dtype=torch.float32)))**0.5, dtype=torch.float64).float()
            assert ulps(st['rstd'], rstd) <= 2, tag + ': save_rstd %r' % st['rstd'][:4]
            exact(tag + ' run_var', st['run_var'], one_m * rv)
            exact(tag + ' scale', st['scale'], gamma * st['rstd'])
            within(tag + ' shift', st['shift'], beta.double() - st['mean'].double() * st['scale'].double(),
                   U * (beta.double().abs() + (st['mean'].double() * st['scale'].double()).abs()))
            rmean = (1 - MOM) * rm.double() + MOM * bias.double()
            within(tag + ' run_mean', st['run_mean'], rmean, 3 * U * ((1 - MOM) * rm.double()).abs() + 2 * U * MOM * bias.double().abs() + U * rmean.abs())


def stats_bounds(y64, e, gamma, beta, rm, rv):
    """float64 statistics of the float64 y and the bounds of the epilogue's chain (csrc/igemm_kernel.h "optional BatchNorm statistics",
    csrc/conv.hip bn_finalize_tiles_kernel).  e >= |kernel's fp32 y - y64| elementwise (the caller's bound of the conv itself).
    A tile — one pixel class, up to 128 consecutive blocks — takes its first row as the pivot p and sums v = y - p (one fp32 rounding) and
    v v (three) over its <= 128 rows in fp32, in some order: any order of n additions errs by at most (n - 1) u sum |terms|, so
      E1_t = 128 u sum |v|,  E2_t = 130 u sum v^2   with |v| <= |y64 - p64| + e + e_p (the kernel's own values)
    The merge is float64 (exact to 2^-53, dropped): mean = p_0 + sum_t (s1_t + n_t (p_t - p_0)) / M, var = sum_t (s2_t + 2 d_t s1_t +
    n_t d_t^2) / M - m1^2 — d var / d s1_t = 2 (p_t - mean) / M.  With E1 = sum_t E1_t / M, ebar = mean(e), c = y64 - mean:
      mean (cast to fp32):  bm = E1 + ebar + u |mean|
      var:   Ev = [2 mean(|c| (e + ebar)) + mean((e + ebar)^2)]  (the conv's error)  + sum_t E2_t / M + 2 sum_t (|p_t - mean| + e_p + bm) E1_t / M + E1^2
      rstd, scale, shift, running statistics: as stats_bounds of tests/test_bn_pool_ops_gpu.py from bm and Ev."""
    N, C, H, W = y64.shape
    yc, ec = P.class_rows(y64), P.class_rows(e)
    M = yc.shape[0] * yc.shape[1]
    mean = yc.mean((0, 1))
    c = (yc - mean).abs()
    var = (c * c).mean((0, 1))
    ebar = ec.mean((0, 1))
    E1, E2, T = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    for m0 in range(0, yc.shape[1], P.TILE_BLOCKS):
        seg, es = yc[:, m0:m0 + P.TILE_BLOCKS], ec[:, m0:m0 + P.TILE_BLOCKS]
        v = (seg - seg[:, :1]).abs() + es + es[:, :1]
        e1 = 128 * U * v.sum(1)  # [64 classes, C]
        E1 += e1.sum(0)
        E2 += 130 * U * (v * v).sum((0, 1))
        T += (((seg[:, 0] - mean).abs() + es[:, 0]) * e1).sum(0)
    E1, E2, T = E1 / M, E2 / M, T / M
    rstd = 1.0 / torch.sqrt(var + EPS)
    gam, bet = gamma.double(), beta.double()
    ref = dict(mean=mean, rstd=rstd, scale=gam * rstd, shift=bet - mean * gam * rstd)
    b = {}
    bm = b['mean'] = E1 + ebar + U * mean.abs()
    ee = ec + ebar
    Ev = 2 * (c * ee).mean((0, 1)) + (ee * ee).mean((0, 1)) + E2 + 2 * (T + bm * E1) + E1**2
    er = 0.5 * Ev * ((var - Ev).clamp_min(0) + EPS)**-1.5
    br = b['rstd'] = er + U * (rstd + er)
    bs = b['scale'] = gam.abs() * br + U * gam.abs() * (rstd + br)
    A = bm * ref['scale'].abs() + (mean.abs() + bm) * bs
    b['shift'] = A + U * ((mean * ref['scale']).abs() + bet.abs() + A)
    fM = M / (M - 1.0)
    unb = var * fM
    bu = Ev * fM + U * (unb + Ev * fM)
    ref['run_mean'] = (1 - MOM) * rm.double() + MOM * mean
    ref['run_var'] = (1 - MOM) * rv.double() + MOM * unb
    b['run_mean'] = MOM * bm + 3 * U * ((1 - MOM) * rm.double()).abs() + 2 * U * MOM * (mean.abs() + bm)
    b['run_var'] = MOM * bu + 3 * U * ((1 - MOM) * rv.double()).abs() + 2 * U * MOM * (unb + bu)
    return ref, b


STATS_MODES = ('f32', 'bf16', 'bf16 storage', 'fp16 storage')


@pytest.mark.parametrize('mode', STATS_MODES)
@pytest.mark.parametrize('shape', FWD_SHAPES)
def test_statistics_on_random_data_against_fp64(shape, mode):
    """save_mean, save_rstd, scale, shift and the running statistics against float64 statistics of the float64 y, within stats_bounds.  The
    conv's own error: in these modes every product is exact in fp32 or rounded once, and an accumulator adds its <= 36 Cg products and the
    bias in fp32 in some order: e = (36 Cg + 2) u (sum |x| |w| + |bias|), the sum in float64.  first_level = 1 (16-bit storage) adds the
    rounding of the stored level-0 part, SR |level 0 + bias| + ETA.  (bf16x3 splits every product into several: its statistics are pinned
    on the constant map and through y in the other tests.)"""
    N, H, W, Cg, Co = shape
    ps, w, b, ref64, y0, _ = random_case(shape, mode)
    pso = [seen(p, mode).double().abs() for p in ps]
    # sum |x| |w| over the 3 x 3 taps is the combined form with |w| combined BEFORE any cancellation; where the kernel rounds the combined
    # filter, the products are |x| |rounded sum| <= |x| (sum |w|) (1 + 2^-8)
    wabs = [P.combine(w.abs(), g, Cg) * (1 + 2.0**-8) for g in range(4)]
    e = (36 * Cg + 2) * U * P.transposed_sum(pso, wabs, b.double().abs())
    bn = bn_params(Co)
    run = Launch(shape, ps, w, b, mode)
    for first in ((0, 1) if AT[mode] else (0, )):
        ef = e + (SR[AT[mode]] * y0.abs() + ETA[AT[mode]] if first else 0)
        ref, bound = stats_bounds(ref64, ef, *bn)
        for wide in wides(mode, Co):
            _, st = run.run('stats', first, wide, bn)
            for k in ('mean', 'rstd', 'scale', 'shift', 'run_mean', 'run_var'):
                within('%s %s' % (tag_of('statistics', shape, mode, 'stats', first, wide, run.level0), k), st[k], ref[k], bound[k])


# ---- the structured gradients ---------------------------------------------------------------------------------------------------------
def ksplits(shape, g, ns):
    """Split counts of level g's data gradient: none (the plain launch) and the library's own plan, which the engine follows."""
    N, H, W, Cg, Co = shape
    k = (1 << g) + 2
    return sorted({1, L().dbn_igemm_splitk_plan_ns(N * (H >> g) * (W >> g), Cg, k * k * Co, Co, ns)})


def run_level_dgrad(dy_d, wc, shape, g, ns, ksplit=1):
    """Level g's data gradient: mode 0 with k = f + 2, stride f, pad 1 on the combined panel (dy_d: device NHWC fp32)."""
    N, H, W, Cg, Co = shape
    f, k = 1 << g, (1 << g) + 2
    d = nan(N, H >> g, W >> g, Cg)
    slab = nan(L().dbn_igemm_splitk_slab_floats(ksplit, N, H >> g, W >> g, Cg)) if ksplit > 1 else None
    igemm_t(dy_d, pack(wc.float(), 0, f, ns), None, d, k, f, 1, 0, ns=ns, ksplit=ksplit, slab=slab)
    return nchw(d)


def run_wgrad(ps, dy, shape, ns):
    """dbn_wgrad_t per level, then dbn_fpn_scatter_wgrad."""
    N, H, W, Cg, Co = shape
    dy_d = nhwc(dy.float())
    ts = [wgrad_t(nhwc(ps[g].float()), dy_d, Cg, Co, (1 << g) + 2, 1 << g, 1, ns) for g in range(4)]
    return scatter_gpu(ts, Co, Cg)


@functools.lru_cache(maxsize=None)
def random_grad_case(shape, mode):
    N, H, W, Cg, Co = shape
    ps = [rnd(N, Cg, H >> g, W >> g, seed=10 + g) for g in range(4)]
    w = P.grid_w((Co, 4 * Cg, 3, 3), 3)
    dy = rnd(N, Co, H, W, seed=4)
    pso, dyo = [seen(p, mode) for p in ps], seen(dy, mode)
    pg = [p.clone().requires_grad_(True) for p in pso]
    wg = w.float().requires_grad_(True)
    grads32 = torch.autograd.grad(F.conv2d(P.concat(pg), wg, None, 1, 1), pg + [wg], dyo)
    return ps, w, dy, pso, dyo, grads32


@pytest.mark.parametrize('mode', GRAD_MODES)
@pytest.mark.parametrize('shape', GRAD_SHAPES)
def test_level_data_gradients_distance_to_fp64(shape, mode):
    """f32 and bf16x3 against fp32 autograd of the concat conv; bf16, whose panel holds the rounded combined filter, against the fp32 strided
    conv with that filter."""
    N, H, W, Cg, Co = shape
    ps, w, dy, pso, dyo, grads32 = random_grad_case(shape, mode)
    dy_d = nhwc(dy)
    for g in range(4):
        wc = P.combine(w, g, Cg)
        wco = seen_w(wc, mode)
        ref64 = R.conv2d(dyo.double(), wco.double(), None, 1 << g, 1)
        ref32 = F.conv2d(dyo, wco, None, 1 << g, 1) if mode == 'bf16' else grads32[g]
        for ks in ksplits(shape, g, NS[mode]):
            distance_ratio('fpn dgrad %s %s level %d ksplit %d' % (shape, mode, g, ks), run_level_dgrad(dy_d, wc, shape, g, NS[mode], ks), ref64, ref32,
                           MARGIN[mode])


@pytest.mark.parametrize('mode', GRAD_MODES)
@pytest.mark.parametrize('shape', GRAD_SHAPES)
def test_weight_gradient_distance_to_fp64(shape, mode):
    N, H, W, Cg, Co = shape
    ps, w, dy, pso, dyo, grads32 = random_grad_case(shape, mode)
    ref64 = P.concat_wgrad([p.double() for p in pso], dyo.double())
    distance_ratio('fpn wgrad %s %s' % (shape, mode), run_wgrad(ps, dy, shape, NS[mode]), ref64, grads32[4], MARGIN[mode])


@pytest.mark.parametrize('mode', GRAD_MODES)
@pytest.mark.parametrize('shape', GRAD_SHAPES)
def test_gradients_are_exact_on_dyadic_data(shape, mode):
    """Dense dyadic data (both gradients), impulses in dy on the seams (data gradient: the pyramid's seams and the strided conv's own M-tile
    seams; weights that differ per (co, ci, tap), rounded per level where the panel rounds them) and the same sparse dy against dense levels
    (weight gradient).  dy has exactly Co = I channels here: the weight gradient has no padding columns to fill."""
    N, H, W, Cg, Co = shape
    ps, w, _ = P.dense_operands(shape)
    dy = R.dense_x((N, Co, H, W), 50)
    dy_d = nhwc(dy.float())
    wd = R.distinct_w(Co, 4 * Cg, 3, 3)
    exact('fpn wgrad dense %s %s' % (shape, mode), run_wgrad(ps, dy, shape, NS[mode]), P.concat_wgrad(ps, dy))
    for g in range(4):
        f = 1 << g
        wc = P.combine(w, g, Cg)
        for ks in ksplits(shape, g, NS[mode]):
            exact('fpn dgrad dense %s %s level %d ksplit %d' % (shape, mode, g, ks), run_level_dgrad(dy_d, wc, shape, g, NS[mode], ks),
                  R.conv2d(dy, wc, None, f, 1))
        pts = sorted(set(P.seam_outputs(N, H, W)) | set(R.seam_pixels(N, H, W, H >> g, W >> g, f)))
        wcd = P.combine(wd, g, Cg)
        for i, dys in enumerate(R.impulse_maps(N, Co, H, W, pts, 1)):
            for ks in ksplits(shape, g, NS[mode]):
                exact('fpn dgrad seams %s %s level %d map %d ksplit %d' % (shape, mode, g, i, ks),
                      run_level_dgrad(nhwc(dys.float()), wcd, shape, g, NS[mode], ks), R.conv2d(dys, seen_w(wcd, mode).double(), None, f, 1))
    for i, dys in enumerate(R.impulse_maps(N, Co, H, W, P.seam_outputs(N, H, W), 1)):
        exact('fpn wgrad sparse dy %s %s map %d' % (shape, mode, i), run_wgrad(ps, dys, shape, NS[mode]), P.concat_wgrad(ps, dys))
