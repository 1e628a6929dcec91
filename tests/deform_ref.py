"""Float64 references and case generators for the two adjoints of the deformable sampling (csrc/deform.hip:
dbn_deform_col2im_gather_t, the gather, and dbn_deform_col2im_t, the fixed-point scatter).  Needs no GPU.

Layouts are the kernels': x / dx [N, H, W, C], offsets / doffset [N, Ho, Wo, >= 18] (channel 2k = dy, 2k + 1 = dx of tap k = 3 r + s),
dcols [N, Ho, Wo, 9, C]; 3 x 3 taps, pad 1.

The exact cases.  x and dcols are integers in [-4, 4] and every offset a multiple of 1/4, so every bilinear weight is a multiple of 1/16:
every dx addend w * g is a multiple of 1/16 and every d(offset) addend g * v * (1 - l | l) a multiple of 1/4.  While
16 sum |dx addends| < 2^24 and 4 sum |doffset addends| < 2^24 per element, every partial sum in every order is a float32 number: the result
does not depend on the summation order, and both kernels have to equal the float64 reference BIT FOR BIT whatever their schedule
(tests/test_deform_ref_cpu.py checks that premise for every case listed in EXACT_CASES and GRID_CASES)."""
import math

import numpy as np
import torch

from oracle import dbnet_oracle as O

# (N, C, H, W, stride): the smallest shapes that still reach each mechanism of the two kernels
SHAPES = [
    (2, 64, 9, 11, 1),  # 24 gather workgroups; N > 1
    (1, 128, 12, 10, 2),  # stride 2: the scatter's 16-channel workgroups
    (1, 192, 13, 9, 2),  # NQ = 2, half filled; odd map
    (1, 320, 7, 8, 1),  # NQ = 4, partly filled
    (1, 512, 7, 8, 1),  # the channel limit
    (1, 64, 21, 19, 1),  # 30 workgroups = 8 * 3 + 6; odd rows in the last tile; W odd
    (1, 64, 5, 4, 1),  # 2 workgroups, fewer than one per XCD
    (1, 20, 6, 7, 1),  # C / 4 = 5 < 32 lanes; C not a multiple of the scatter's 32
]
ALL_GENERATORS_ON = (0, 1, 5)  # the shapes that run every generator; the others run SHORT_LIST
PILE_POINTS = 5
GENERATORS = (['edges', 'edges_near', 'integer', 'quarter6', 'traveller'] + ['pile%d' % i for i in range(PILE_POINTS)] +
              ['pile_rows', 'rim_below', 'rim_at', 'rim_above', 'rim_far'])
SHORT_LIST = ['edges_near', 'integer', 'pile2']
EXACT_CASES = [(si, gn) for si in range(len(SHAPES)) for gn in (GENERATORS if si in ALL_GENERATORS_ON else SHORT_LIST)]
# exact data beyond one pass of a grid-stride loop, edges_near offsets (tests/test_deform_adjoint_gpu.py says which loop)
GRID_CASES = [(8, 64, 100, 100, 1), (53, 4, 100, 100, 1)]


def out_size(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def off_stride_of(shape):
    """The offset map's channel count: 64 (the layer's offset conv runs on 64 channels), 20 on the last shape."""
    return 20 if shape == SHAPES[-1] else 64


# ------------------------------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------------------------------
def _adjoint(x, off, dcols, stride, dtype, dev):
    xx = x.detach().to(dev, dtype).permute(0, 3, 1, 2).requires_grad_(True)
    oo = off.detach()[..., :18].to(dev, dtype).permute(0, 3, 1, 2).requires_grad_(True)
    g = dcols.detach().to(dev, dtype).permute(0, 4, 3, 1, 2)
    cols = O.deform_sample(xx, oo, 3, 3, stride, 1)  # [N, C, 9, Ho, Wo]
    dx, do = torch.autograd.grad(cols, (xx, oo), g)
    return dx.permute(0, 2, 3, 1).contiguous(), do.permute(0, 2, 3, 1).contiguous()


def adjoint64(x, off, dcols, stride, dev='cpu'):
    """(dx [N, H, W, C], doffset [N, Ho, Wo, 18]) in float64: torch.autograd.grad of oracle.dbnet_oracle.deform_sample on the operands as
    stored (any dtype; offset channels beyond 18 are not looked at).  At an integer position the derivative with respect to the offset is
    the one-sided one that floor gives (y0 = y, ly = 0: the slope towards y + 1); the kernels use the same expression,
    hx * (v2 - v0) + lx * (v3 - v1), so nothing is special-cased on either side."""
    return _adjoint(x, off, dcols, stride, torch.float64, dev)


def adjoint32(x, off, dcols, stride, dev='cpu'):
    """The float32 twin of adjoint64: what plain fp32 gives on the same operands (the baseline of gpu_util.distance_ratio)."""
    return _adjoint(x, off, dcols, stride, torch.float32, dev)


def adjoint_loops(x, off, dcols, stride):
    """The same adjoint restated in plain numpy float64, sharing nothing with the oracle: a loop over (sample, corner) that scatters
    w * g into dx and forms d(offset) from the four masked corner values.  Returns (dx, doffset, sum |dx addends|, sum |doffset addends|);
    the last two are the adjoint of |dcols|, |x|: per element, the sum of |w g| and of |g| |v_corner| |dw_corner / d(y, x)|."""
    x = np.asarray(x.detach().cpu().double().numpy())
    off = np.asarray(off.detach().cpu().double().numpy())
    g_all = np.asarray(dcols.detach().cpu().double().numpy())
    N, H, W, C = x.shape
    Ho, Wo = out_size(H, W, stride)
    dx, sdx = np.zeros_like(x), np.zeros_like(x)
    do, sdo = np.zeros((N, Ho, Wo, 18)), np.zeros((N, Ho, Wo, 18))
    zero = np.zeros(C)
    for n in range(N):
        for ho in range(Ho):
            for wo in range(Wo):
                for k in range(9):
                    py = ho * stride - 1 + k // 3 + off[n, ho, wo, 2 * k]
                    px = wo * stride - 1 + k % 3 + off[n, ho, wo, 2 * k + 1]
                    if not (py > -1 and py < H and px > -1 and px < W):
                        continue  # the sample is the constant zero
                    y0, x0 = math.floor(py), math.floor(px)
                    ly, lx = py - y0, px - x0
                    g = g_all[n, ho, wo, k]
                    v = []
                    for yy, xx, w in ((y0, x0, (1 - ly) * (1 - lx)), (y0, x0 + 1, (1 - ly) * lx), (y0 + 1, x0, ly * (1 - lx)),
                                      (y0 + 1, x0 + 1, ly * lx)):
                        if 0 <= yy <= H - 1 and 0 <= xx <= W - 1:
                            dx[n, yy, xx] += w * g
                            sdx[n, yy, xx] += np.abs(w * g)
                            v.append(x[n, yy, xx])
                        else:
                            v.append(zero)
                    a = [np.abs(t) for t in v]
                    do[n, ho, wo, 2 * k] = np.sum(g * ((1 - lx) * (v[2] - v[0]) + lx * (v[3] - v[1])))
                    do[n, ho, wo, 2 * k + 1] = np.sum(g * ((1 - ly) * (v[1] - v[0]) + ly * (v[3] - v[2])))
                    sdo[n, ho, wo, 2 * k] = np.sum(np.abs(g) * ((1 - lx) * (a[2] + a[0]) + lx * (a[3] + a[1])))
                    sdo[n, ho, wo, 2 * k + 1] = np.sum(np.abs(g) * ((1 - ly) * (a[1] + a[0]) + ly * (a[3] + a[2])))
    return dx, do, sdx, sdo


# ------------------------------------------------------------------------------------------------------------------------------------
# offsets: [N, Ho, Wo, 18] float32, multiples of 1/4
# ------------------------------------------------------------------------------------------------------------------------------------
def tap_base(Ho, Wo, stride):
    """The undeformed tap positions (by, bx), each broadcastable to [1, Ho, Wo, 9]."""
    ho = torch.arange(Ho).view(1, Ho, 1, 1) * stride - 1
    wo = torch.arange(Wo).view(1, 1, Wo, 1) * stride - 1
    r = torch.arange(9).view(1, 1, 1, 9) // 3
    s_ = torch.arange(9).view(1, 1, 1, 9) % 3
    return ho + r, wo + s_


def edge_offsets(N, H, W, stride, g, quarter=True, far=True):
    """Offsets [N, Ho, Wo, 18] that move each tap onto a chosen position class: exactly -1 and exactly H / W (outside), (-1, 0),
    exactly 0, exactly H - 1 / W - 1, (H - 1, H) / (W - 1, W), interior integers and quarters, far outside (+-(H + 7), +-1000, +-6e4).
    far = False leaves the far classes out: max |offset| <= max(H, W) + 1."""
    Ho, Wo = out_size(H, W, stride)

    def targets(E, n):
        cls = torch.tensor([-1.0, -0.75, -0.5, -0.25, 0.0, E - 1.0, E - 0.75, E - 0.5, E - 0.25, float(E), -(E + 7.0), E + 7.0, -1000.0,
                            1000.0, 6e4, -6e4])
        if not far:
            cls = cls[:10]
        t = cls[torch.randint(0, len(cls), (n, ), generator=g)]
        inner = torch.randint(0, 4 * (E - 1) + 1, (n, ), generator=g).float() / (4 if quarter else 1)
        return torch.where(torch.rand(n, generator=g) < 0.3, inner, t)

    by, bx = tap_base(Ho, Wo, stride)
    n = N * Ho * Wo * 9
    off = torch.empty(N, Ho, Wo, 18)
    off[..., 0::2] = targets(H, n).view(N, Ho, Wo, 9) - by
    off[..., 1::2] = targets(W, n).view(N, Ho, Wo, 9) - bx
    return off


def emax_of(H, W):
    """The offset magnitude from which on the gather searches the whole map (csrc/deform.hip: max(H, W) + R)."""
    return max(H, W) + 3


def pile_point(i, H, W):
    return [(0.0, 0.0), (-0.5, -0.5), (1.25, 2.5), (H - 1.0, W - 1.0), (H - 0.25, W - 0.5)][i]


def traveller_offsets(N, H, W, stride, g):
    """All zero except about eight samples per image, each moved from within two output pixels of one corner of the map to a quarter point
    within 2.25 pixels of the opposite corner: one large offset widens every pixel's window, and only the landing pixels change."""
    Ho, Wo = out_size(H, W, stride)
    off = torch.zeros(N, Ho, Wo, 18)
    ri = lambda lo, hi: int(torch.randint(lo, hi, (1, ), generator=g))
    for n in range(N):
        for j in range(8):
            low_y, low_x = not (j & 1), not (j & 2)  # the corner the sample starts in
            ho, wo, k = ri(0, min(2, Ho)), ri(0, min(2, Wo)), ri(0, 9)
            ty, tx = ri(0, 10) / 4, ri(0, 10) / 4
            if low_y:
                ty = H - 1 - ty
            else:
                ho = Ho - 1 - ho
            if low_x:
                tx = W - 1 - tx
            else:
                wo = Wo - 1 - wo
            off[n, ho, wo, 2 * k] = ty - (ho * stride - 1 + k // 3)
            off[n, ho, wo, 2 * k + 1] = tx - (wo * stride - 1 + k % 3)
    return off


def offsets(name, shape, g, at=0):
    """The generator `name` on SHAPES-style `shape`; at (0 fp32, 1 bf16, 2 fp16) only matters to rim_far."""
    N, C, H, W, stride = shape
    Ho, Wo = out_size(H, W, stride)
    by, bx = tap_base(Ho, Wo, stride)
    if name == 'edges':  # with the far classes: max |offset| >= H + W + 3, the gather searches the whole map
        return edge_offsets(N, H, W, stride, g)
    if name == 'edges_near':  # max |offset| < max(H, W) + 3: the finite window
        return edge_offsets(N, H, W, stride, g, far=False)
    if name == 'integer':  # E an exact integer, taps exactly on the window's rim, half of all corner weights exactly 0
        return torch.randint(-3, 4, (N, Ho, Wo, 18), generator=g).float()
    if name == 'quarter6':  # a 15 x 15 window: three 96-pixel rounds on the 21 x 19 map
        return torch.randint(-24, 25, (N, Ho, Wo, 18), generator=g).float() / 4
    if name == 'traveller':
        return traveller_offsets(N, H, W, stride, g)
    if name.startswith('pile') and name != 'pile_rows':  # every tap of every output pixel onto one position
        py, px = pile_point(int(name[4:]), H, W)
        off = torch.empty(N, Ho, Wo, 18)
        off[..., 0::2] = py - by
        off[..., 1::2] = px - bx
        return off
    if name == 'pile_rows':  # even output rows onto input row 0, odd ones far outside: wildly different trip counts side by side
        off = torch.zeros(N, Ho, Wo, 18)
        even = (torch.arange(Ho).view(1, Ho, 1, 1) % 2 == 0).expand(N, Ho, Wo, 9)
        off[..., 0::2] = torch.where(even, (0 - by).float().expand(N, Ho, Wo, 9), torch.tensor(1000.0))
        return off
    if name.startswith('rim_'):  # edges_near, and one corner sample (far outside) that alone sets max |offset| = v
        off = edge_offsets(N, H, W, stride, g, far=False)
        off[0, 0, 0, 0] = -rim_value(name, shape, at)
        return off
    raise KeyError(name)


def rim_value(name, shape, at):
    """v of rim(v): just below, at and just above the switch to the whole-map search, and far above (all exact in bf16 and fp16)."""
    e = emax_of(shape[2], shape[3])
    return {'rim_below': e - 0.25, 'rim_at': float(e), 'rim_above': e + 0.25, 'rim_far': 6e4 if at == 2 else 1000.0}[name]


def exact_case(shape, name, at=0):
    """(x [N, H, W, C], offsets [N, Ho, Wo, 18], dcols [N, Ho, Wo, 9, C]) in float32: integers in [-4, 4] and multiples of 1/4.  The same
    generator state for every `at`, so the storage types see the same case (rim_far apart)."""
    N, C, H, W, stride = shape
    Ho, Wo = out_size(H, W, stride)
    g = torch.Generator().manual_seed(1000 * sum(shape) + GENERATORS.index(name))
    x = torch.randint(-4, 5, (N, H, W, C), generator=g).float()
    dcols = torch.randint(-4, 5, (N, Ho, Wo, 9, C), generator=g).float()
    return x, offsets(name, shape, g, at), dcols


def grid_case(shape):
    N, C, H, W, stride = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randint(-4, 5, (N, H, W, C), generator=g).float()
    dcols = torch.randint(-4, 5, (N, H, W, 9, C), generator=g).float()
    return x, edge_offsets(N, H, W, stride, g, far=False), dcols


def stored_offsets(off, os_, dtype):
    """The offset map as the kernels get it: [N, Ho, Wo, os_] in the storage type, channels 18.. NaN (they must not be read)."""
    full = torch.full(off.shape[:3] + (os_, ), float('nan'))
    full[..., :18] = off
    return full.to(dtype)


def positions(off, H, W, stride):
    """Sample positions (y, x), each [N, Ho, Wo, 9] float64, of an offset map [N, Ho, Wo, >= 18]."""
    Ho, Wo = out_size(H, W, stride)
    by, bx = tap_base(Ho, Wo, stride)
    return off[..., 0:18:2].double() + by, off[..., 1:18:2].double() + bx
