"""Helpers shared by the -m gpu parity tests (call the C ABI through ctypes)."""
import numpy as np
import torch

from db_text_minimal_amd import _lib

DEV = 'cuda'


def L():
    return _lib.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def nhwc(x_nchw):
    return x_nchw.permute(0, 2, 3, 1).contiguous().to(DEV)


def nchw(x_nhwc):
    return x_nhwc.permute(0, 3, 1, 2).contiguous().cpu()


def report(tag, got, ref, atol, rtol):
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    assert torch.isfinite(got).all(), tag + ': non-finite values'
    err = (got - ref).abs()
    tol = atol + rtol * ref.abs()
    worst = float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0
    if float(err.max() if err.numel() else 0) == 0.0:
        worst = 0.0
    msg = '%s: max abs err %.3e (ref max %.3e), worst err/tol %.3f' % (tag, float(err.max()) if err.numel() else 0,
                                                                      float(ref.abs().max()) if ref.numel() else 0, worst)
    print(msg)
    assert worst <= 1.0, msg


def pack(w, mode, stride=1, ns=0):
    """w: CPU OIHW tensor -> device panels (ns = 0 fp32 MFMA, 3 = bf16x3 split, 1 = bf16)."""
    O, I, R, S = w.shape
    wd = w.contiguous().to(DEV)
    if ns == 0:
        out = torch.empty(L().dbn_igemm_panel_floats(O, I, R, S, mode, stride), device=DEV)
        _lib.check(L().dbn_pack_weights(wd.data_ptr(), O, I, R, S, mode, stride, out.data_ptr(), stream()), 'pack')
    else:
        out = torch.empty(L().dbn_igemm_bf16s_panel_floats(O, I, R, S, mode, stride, ns), device=DEV)
        _lib.check(L().dbn_pack_weights_bf16s(wd.data_ptr(), O, I, R, S, mode, stride, ns, out.data_ptr(), stream()), 'pack')
    return out


def igemm(src, wpk, bias, dst, R, stride, pad, mode, accumulate=0, tile=0, ns=0):
    N, Hs, Ws, Cs = src.shape
    _, Hd, Wd, Cd = dst.shape
    args = (src.data_ptr(), wpk.data_ptr(), None if bias is None else bias.data_ptr(), dst.data_ptr(), N, Hs, Ws, Cs, Hd, Wd, Cd, R,
            R, stride, pad, mode, accumulate, tile)
    if ns == 0:
        _lib.check(L().dbn_igemm_f32(*args, stream()), 'igemm')
    else:
        _lib.check(L().dbn_igemm_bf16s(*args, ns, stream()), 'igemm_bf16s')


AT_OF = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def igemm_t(src, wpk, bias, dst, R, stride, pad, mode, accumulate=0, tile=0, ns=1, ksplit=1, slab=None):
    N, Hs, Ws, Cs = src.shape
    _, Hd, Wd, Cd = dst.shape
    _lib.check(L().dbn_igemm_t(AT_OF[src.dtype], ns, src.data_ptr(), wpk.data_ptr(), None if bias is None else bias.data_ptr(), dst.data_ptr(),
                               N, Hs, Ws, Cs, Hd, Wd, Cd, R, R, stride, pad, mode, accumulate, tile, ksplit,
                               None if slab is None else slab.data_ptr(), stream()), 'igemm_t')


def pack_t(w, mode, stride, kind, cs=0):
    O, I, R, S = w.shape
    wd = w.contiguous().to(DEV)
    out = torch.empty(L().dbn_igemm_panel_floats_t(kind, O, I, R, S, mode, stride, cs), device=DEV)
    _lib.check(L().dbn_pack_weights_t(kind, wd.data_ptr(), O, I, R, S, mode, stride, cs, out.data_ptr(), stream()), 'pack_t')
    return out


def igemm_splitk(src, wpk, bias, dst, R, stride, pad, mode, ksplit, accumulate=0, tile=0, ns=0):
    """dbn_igemm_splitk_f32 with a NaN-filled slab."""
    N, Hs, Ws, Cs = src.shape
    _, Hd, Wd, Cd = dst.shape
    slab = torch.full((L().dbn_igemm_splitk_slab_floats(ksplit, N, Hd, Wd, Cd), ), float('nan'), device=DEV)
    _lib.check(L().dbn_igemm_splitk_f32(src.data_ptr(), wpk.data_ptr(), None if bias is None else bias.data_ptr(), dst.data_ptr(), N, Hs, Ws,
                                        Cs, Hd, Wd, Cd, R, R, stride, pad, mode, accumulate, tile, ns, ksplit, slab.data_ptr(), stream()),
               'splitk')


def wgrad(sm, big, O, I, k, stride, pad, scale=1.0, ns=0):
    N, Ho, Wo, _ = sm.shape
    _, H, W, Cb = big.shape
    slab = torch.empty(L().dbn_wgrad_slab_floats_hw(N, Ho, Wo, O, H, W, Cb, k, k, 4), device=DEV)
    g = torch.full((O, I, k, k), float('nan'), device=DEV)
    args = (sm.data_ptr(), big.data_ptr(), slab.data_ptr(), g.data_ptr(), N, Ho, Wo, O, H, W, Cb, I, k, k, stride, pad, scale)
    if ns == 0:
        _lib.check(L().dbn_wgrad_f32(*args, stream()), 'wgrad')
    else:
        _lib.check(L().dbn_wgrad_bf16s(*args, ns, stream()), 'wgrad_bf16s')
    return g


def wgrad_t_call(sm, big, O, I, k, stride, pad, ns=0, scale=1.0):
    """A NaN-filled slab, a NaN-filled gradient and the arguments of a dbn_wgrad_t / dbn_wgrad_phase_t / dbn_wgrad_reduce_describe call
    on them (all but the last one: the stream, or the job record)."""
    assert sm.dtype == big.dtype and sm.is_contiguous() and big.is_contiguous()
    N, Ho, Wo, _ = sm.shape
    _, H, W, Cb = big.shape
    slab = torch.full((L().dbn_wgrad_slab_floats_hw(N, Ho, Wo, O, H, W, Cb, k, k, big.element_size()), ), float('nan'), device=DEV)
    g = torch.full((O, I, k, k), float('nan'), device=DEV)
    return slab, g, (AT_OF[big.dtype], ns, sm.data_ptr(), big.data_ptr(), slab.data_ptr(), g.data_ptr(), N, Ho, Wo, O, H, W, Cb, I, k, k, stride,
                     pad, scale)


def wgrad_t(sm, big, O, I, k, stride, pad, ns=0, scale=1.0, phases=False):
    """dbn_wgrad_t on fp32 / bf16 tensors (sm: the output-side tensor [N, Ho, Wo, O], big: the input side [N, H, W, Cb]) with a NaN-filled
    slab and gradient; phases: as dbn_wgrad_phase_t(1) followed by (2)."""
    slab, g, args = wgrad_t_call(sm, big, O, I, k, stride, pad, ns, scale)
    if phases:
        _lib.check(L().dbn_wgrad_phase_t(1, *args, stream()), 'wgrad_phase_t(1)')
        _lib.check(L().dbn_wgrad_phase_t(2, *args, stream()), 'wgrad_phase_t(2)')
    else:
        _lib.check(L().dbn_wgrad_t(*args, stream()), 'wgrad_t')
    return g


def reduce_ws():
    return torch.empty(L().dbn_reduce_ws_floats(512), device=DEV)


def col_sum_depth(M, C):
    """Longest serial fp32 chain of dbn_col_sum_t (csrc/pointwise.hip channel_reduce): nb = min(ceil(M / 64), 768) blocks of
    ceil(M / nb) rows; in a chunk of Cc = min(C, 1024) channels, 256 / (Cc / 4) row lanes share a block's rows and are then added in LDS."""
    nb = min(max(-(-M // 64), 1), 768)
    rows = -(-M // nb)
    nrl = max(256 // (min(C, 1024) // 4), 1)
    return -(-rows // nrl) + nrl


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def report_robust(tag, got, ref, atol, rtol, frac=0.999):
    """Like report(), but tolerates a tiny fraction of outliers (Adam turns a sign flip of a
    ~zero gradient into a +-lr step, so a handful of elements legitimately differ)."""
    got = got.detach().cpu().double().reshape(-1)
    ref = ref.detach().cpu().double().reshape(-1)
    assert got.shape == ref.shape and torch.isfinite(got).all(), tag
    ok = (got - ref).abs() <= atol + rtol * ref.abs()
    f = float(ok.double().mean())
    print('%s: %.5f of elements within tol, mean abs err %.3e' % (tag, f, float((got - ref).abs().mean())))
    assert f >= frac, tag


# ---- float64 pins of the storage-typed kernels (test_train16_ops_gpu.py, test_bn_pool_ops_gpu.py, test_infer16_ops_gpu.py) ----
U = 2.0**-24
DT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
SR = {0: 2.0**-24, 1: 2.0**-8, 2: 2.0**-11}  # unit roundoff of the storage type (round to nearest even)
ETA = {0: 0.0, 1: 0.0, 2: 2.0**-25}  # absolute floor of one rounding: half the fp16 subnormal spacing
NAN = float('nan')


def gen(seed, dev=DEV):
    return torch.Generator(device=dev).manual_seed(seed)


CHUNK = 1 << 24  # elements per comparison slice (keeps the float64 temporaries of the step-sized checks small)


def within(tag, got, ref, bound):
    """|got - ref| <= bound elementwise; got must be finite everywhere (NaN-filled outputs that were never written fail here)."""
    got, ref = got.detach().reshape(-1), ref.detach().reshape(-1)
    bound = torch.as_tensor(bound, dtype=torch.float64).detach().reshape(-1)
    assert got.numel() == ref.numel() and bound.numel() in (1, ref.numel()), (tag, got.shape, ref.shape, bound.shape)
    worst, emax, nover, first = 0.0, 0.0, 0, None
    for i in range(0, got.numel(), CHUNK):
        g = got[i:i + CHUNK].double()
        r = ref[i:i + CHUNK].to(g.device, torch.float64)
        b = (bound if bound.numel() == 1 else bound[i:i + CHUNK]).to(g.device, torch.float64)
        nf = ~torch.isfinite(g)
        assert not bool(nf.any()), '%s: %d non-finite elements, the first at %d' % (tag, int(nf.sum()), i + int(nf.nonzero()[0]))
        err = (g - r).abs()
        over = err > b
        emax = max(emax, float(err.max()))
        worst = max(worst, float(torch.where(err > 0, err / b.clamp_min(1e-300), torch.zeros_like(err)).max()))
        if bool(over.any()):
            nover += int(over.sum())
            if first is None:
                j = int(over.nonzero()[0])
                first = (i + j, float(g[j]), float(r[j]), float(b[j] if b.numel() > 1 else b[0]))
    msg = '%s: max err %.3e, worst err / bound %.3f' % (tag, emax, worst)
    print(msg)
    assert nover == 0, msg + ' (%d elements over; the first at %d: got %r ref %r bound %.3e)' % ((nover, ) + first)


def exact(tag, got, ref):
    """got == ref exactly (as numbers: -0 == +0), got finite everywhere."""
    got, ref = got.detach().reshape(-1), ref.detach().reshape(-1)
    assert got.numel() == ref.numel(), (tag, got.shape, ref.shape)
    nne, first = 0, None
    for i in range(0, got.numel(), CHUNK):
        g = got[i:i + CHUNK].double()
        r = ref[i:i + CHUNK].to(g.device, torch.float64)
        nf = ~torch.isfinite(g)
        assert not bool(nf.any()), '%s: %d non-finite elements, the first at %d' % (tag, int(nf.sum()), i + int(nf.nonzero()[0]))
        ne = g != r
        if bool(ne.any()):
            nne += int(ne.sum())
            if first is None:
                j = int(ne.nonzero()[0])
                first = (i + j, float(g[j]), float(r[j]))
    assert nne == 0, '%s: %d of %d elements differ; the first at %d: got %r ref %r' % ((tag, nne, got.numel()) + first)
    print('%s: %d elements bit-exact' % (tag, got.numel()))


def distance_ratio(tag, got, ref64, ref32, margin, allow=None):
    """The kernel's distance to float64 against plain fp32's own: rms(got - ref64) <= margin rms(ref32 - ref64) and
    max |got - ref64| <= margin max |ref32 - ref64|; got finite everywhere.  allow (16-bit storage): an elementwise allowance for the one
    output rounding, taken off |got - ref64| first.  Prints and returns the two ratios."""
    got, ref64, ref32 = got.detach().cpu().double(), ref64.detach().cpu().double(), ref32.detach().cpu().double()
    assert got.shape == ref64.shape == ref32.shape, (tag, got.shape, ref64.shape, ref32.shape)
    nf = ~torch.isfinite(got)
    assert not bool(nf.any()), '%s: %d non-finite elements, the first at %d' % (tag, int(nf.sum()), int(nf.reshape(-1).nonzero()[0]))
    err = (got - ref64).abs()
    if allow is not None:
        err = (err - allow).clamp_min(0)
    e32 = (ref32 - ref64).abs()
    r_rms = float(err.pow(2).mean().sqrt() / e32.pow(2).mean().sqrt())
    r_max = float(err.max() / e32.max())
    msg = 'RATIO %s: rms %.3f max %.3f (fp32 itself: rms %.3e max %.3e)' % (tag, r_rms, r_max, float(e32.pow(2).mean().sqrt()), float(e32.max()))
    print(msg)
    assert r_rms <= margin and r_max <= margin, msg + ' over the margin %g' % margin
    return r_rms, r_max
