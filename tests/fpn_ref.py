"""float64 reference of the FPN output conv — the 3 x 3 conv over [p2 | up2(p3) | up4(p4) | up8(p5)] (segmentation_body.py:75-76,82-87) — in the
forms the library computes it in: the concatenation itself, the combined (f + 2) x (f + 2) / stride-f filters of csrc/pointwise.hip
(fpn_combine_weights_kernel / fpn_scatter_wgrad_kernel) and the pyramid kernel's walk over 8 x 8 pixel classes (csrc/igemm_kernel.h, MODE 3).

Plain torch on the CPU, built on conv_ref.conv2d / conv2d_dgrad / conv2d_wgrad / conv_transpose2d; combine and scatter are explicit loops over
the definition R(u) = {r in 0..2 : 2 - u <= r <= f + 1 - u}.  tests/test_fpn_ref_cpu.py checks every function against F.interpolate, F.conv2d
and autograd in float64, shows the identities between the forms exactly on dyadic data, and shows that the data sets of
tests/test_fpn_fp64_gpu.py tell a reference with one fault in it from the right one.  Level g has the upsample factor f = 2^g; tensors are
NCHW float64, the combined weights [Cg, Co, k, k] (ConvTranspose2d's layout)."""
import torch

import conv_ref as R

LEVELS = 4
BLOCK = 8  # the pyramid kernel walks 8 x 8 pixel blocks: 64 classes (oh0, ow0), one row of its GEMM per block
TILE_BLOCKS = 128  # blocks per row tile


def upsample(x, f):
    """Nearest upsample by index: out[h, w] = x[h // f, w // f]."""
    N, C, H, W = x.shape
    return x[:, :, torch.arange(H * f) // f][:, :, :, torch.arange(W * f) // f]


def upsample_adjoint(d, f):
    """Its adjoint: the f x f block sum."""
    N, C, H, W = d.shape
    return d.reshape(N, C, H // f, f, W // f, f).sum((3, 5))


def concat(ps):
    return torch.cat([upsample(p, 1 << g) for g, p in enumerate(ps)], 1)


def concat_conv(ps, w, b=None):
    return R.conv2d(concat(ps), w, b, 1, 1)


def concat_dgrad(dy, w, Cg):
    """Gradients of concat_conv with respect to the four levels: the block sum of the matching channel slice."""
    N, _, H, W = dy.shape
    d = R.conv2d_dgrad(dy, w, 1, 1, H, W)
    return [upsample_adjoint(d[:, g * Cg:(g + 1) * Cg], 1 << g) for g in range(w.shape[1] // Cg)]


def concat_wgrad(ps, dy):
    return R.conv2d_wgrad(concat(ps), dy, 3, 3, 1, 1)


def taps(u, f):
    """R(u): the rows r of the 3 x 3 filter that read source pixel hs at output h = hs f - 1 + u ((h + r - 1) // f == hs)."""
    return [r for r in range(3) if 2 - u <= r <= f + 1 - u]


def combine(w, g, Cg, drop=None):
    """Wd[ci, co, u, v] = sum_{r in R(u)} sum_{s in R(v)} w[co, g Cg + ci, r, s].  drop = (u, v): a faulty combination that loses the last
    tap of that one (u, v) (test_fpn_ref_cpu.py: the teeth of the data sets)."""
    f, k = 1 << g, (1 << g) + 2
    Co = w.shape[0]
    wd = torch.zeros((Cg, Co, k, k), dtype=w.dtype)
    for u in range(k):
        for v in range(k):
            pairs = [(r, s) for r in taps(u, f) for s in taps(v, f)]
            if drop == (u, v):
                pairs = pairs[:-1]
            for (r, s) in pairs:
                wd[:, :, u, v] += w[:, g * Cg:(g + 1) * Cg, r, s].t()
    return wd


def scatter(ts, Co, Cg):
    """The adjoint of combine: dw[co, g Cg + ci, r, s] = sum_{u : r in R(u)} sum_{v : s in R(v)} ts[g][ci, co, u, v]."""
    dw = torch.zeros((Co, len(ts) * Cg, 3, 3), dtype=ts[0].dtype)
    for g, t in enumerate(ts):
        f, k = 1 << g, (1 << g) + 2
        for r in range(3):
            for s in range(3):
                for u in range(k):
                    for v in range(k):
                        if r in taps(u, f) and s in taps(v, f):
                            dw[:, g * Cg:(g + 1) * Cg, r, s] += t[:, :, u, v].t()
    return dw


def transposed_sum(ps, wcs, b=None, first=0):
    """bias + sum_{g >= first} ConvTranspose2d(k = f + 2, stride f, padding 1)(p_g, wcs[g]): the pyramid kernel's definition
    (include/dbnet_hip.h), on whatever combined weights the caller hands in (rounded to the kernel's operand type where it rounds them)."""
    y = None
    for g in range(first, len(ps)):
        t = R.conv_transpose2d(ps[g], wcs[g], None, 1 << g, 1)
        y = t if y is None else y + t
    return y if b is None else y + b.view(1, -1, 1, 1)


def classwise_conv(ps, w, b, Cg, padh_fault=None, only=None):
    """The same conv the way the pyramid kernel walks it: per class (oh0, ow0) of the 8 x 8 blocks and per level, output pixel
    (8 hb + oh0, 8 wb + ow0) takes tap (r, s) from source pixel ((h + r - 1) >> g, (w + s - 1) >> g) of a zero-padded level.
    padh_fault = (g, oh0, ow0): a faulty walk whose vertical origin is one source row too low for that one class of that level.
    only = (g, oh0, ow0): that level's part of that class's pixels alone (the rest of the result stays 0)."""
    N, _, H, W = ps[0].shape
    Co = w.shape[0]
    y = torch.zeros((N, Co, H, W), dtype=w.dtype)
    for g, p in enumerate(ps):
        if only is not None and only[0] != g:
            continue
        Hg, Wg = p.shape[2:]
        pp = torch.zeros((N, Cg, Hg + 2, Wg + 2), dtype=w.dtype)
        pp[:, :, 1:Hg + 1, 1:Wg + 1] = p
        for oh0 in range(BLOCK):
            for ow0 in range(BLOCK):
                if only is not None and only[1:] != (oh0, ow0):
                    continue
                hs, ws = torch.arange(oh0, H, BLOCK), torch.arange(ow0, W, BLOCK)
                off = 1 if padh_fault == (g, oh0, ow0) else 0
                for r in range(3):
                    rows = (((hs + r - 1) >> g) + 1 + off).clamp(0, Hg + 1)
                    for s in range(3):
                        cols = ((ws + s - 1) >> g) + 1
                        src = pp[:, :, rows][:, :, :, cols]
                        y[:, :, oh0::BLOCK, ow0::BLOCK] += torch.einsum('oc,nchw->nohw', w[:, g * Cg:(g + 1) * Cg, r, s], src)
    return y if b is None else y + b.view(1, Co, 1, 1)


def block_of(N, H, W, m):
    """GEMM row m of the pyramid kernel -> (n, hb, wb): blocks are numbered through the batch, row-major inside an image."""
    Hb, Wb = H // BLOCK, W // BLOCK
    return m // (Hb * Wb), m // Wb % Hb, m % Wb


def displace_block(y, m_a, m_b, oh0, ow0):
    """A faulty store: the pixel of class (oh0, ow0) of block m_a lands in block m_b and the other way round."""
    N, _, H, W = y.shape
    (na, ha, wa), (nb, hb, wb) = block_of(N, H, W, m_a), block_of(N, H, W, m_b)
    out = y.clone()
    out[na, :, BLOCK * ha + oh0, BLOCK * wa + ow0] = y[nb, :, BLOCK * hb + oh0, BLOCK * wb + ow0]
    out[nb, :, BLOCK * hb + oh0, BLOCK * wb + ow0] = y[na, :, BLOCK * ha + oh0, BLOCK * wa + ow0]
    return out


def class_rows(y):
    """y [N, C, H, W] -> [64, M, C]: class (oh0, ow0) major, then the kernel's GEMM rows (blocks), then channels — the order in which the
    pyramid kernel's tiles (one class, 128 consecutive blocks) see the output."""
    N, C, H, W = y.shape
    t = y.reshape(N, C, H // BLOCK, BLOCK, W // BLOCK, BLOCK).permute(3, 5, 0, 2, 4, 1)
    return t.reshape(BLOCK * BLOCK, N * (H // BLOCK) * (W // BLOCK), C)


# ---- the data sets ------------------------------------------------------------------------------------------------------------------
def dense_operands(shape, seed=30):
    """Dense dyadic levels ({-4..4} / 4), weights ({-8..8} / 8; level 0's on multiples of 1 / 2, so that a Winograd level 0 is exact too) and
    bias (2^-5 grid).  The combined sums are multiples of 1 / 8 of magnitude <= 9: 7 significant bits, bf16-representable."""
    N, H, W, Cg, Co = shape
    ps = [R.dense_x((N, Cg, H >> g, W >> g), seed + g) for g in range(LEVELS)]
    w = R.dense_w((Co, LEVELS * Cg, 3, 3), seed + 4)
    w[:, :Cg] = R.dense_w((Co, Cg, 3, 3), seed + 5, winograd=True)
    return ps, w, R.dense_bias(Co, seed + 6)


def grid_w(shape, seed):
    """Random weights on a 2^-10 grid with |w| <= 2^-3: a combined sum of up to 9 of them is a multiple of 2^-10 below 2^1 (at most 12
    significant bits), exact in fp32 in any order — so the operand the 16-bit modes see is the rounding of a KNOWN number, combine()'s."""
    return torch.randint(-128, 129, shape, generator=torch.Generator().manual_seed(seed)).double() / 1024


def seam_sources(N, H, W, g):
    """Source pixels (n, h, w) of level g (an [N, H >> g, W >> g] map) that feed the seams of the pyramid kernel's walk over the [N, H, W]
    output: the four map corners of every image (the last block of image n and the first of image n + 1 among them); both sides of every
    8 x 8 block edge along h and along w (one position per edge, moving from edge to edge); blocks 127 | 128 of every row-tile boundary and
    the last block of the ragged tile (their first and last pixel); for each of the 64 pixel classes (oh0, ow0) the source under that
    class's pixel of a block on a row-tile boundary (even classes: the last block of tile 0, odd classes: the first block of tile 1; one
    row tile only: the first and the last block), so that every class — hence each of the 2^g x 2^g phase classes of every level — has
    an impulse under its centre tap; and two interior pixels of different parity."""
    Hg, Wg = H >> g, W >> g
    M = N * (H // BLOCK) * (W // BLOCK)
    probe = (TILE_BLOCKS - 1, TILE_BLOCKS) if M > TILE_BLOCKS else (0, M - 1)
    out = []  # output-map pixels first
    for c in range(BLOCK * BLOCK):
        n, hb, wb = block_of(N, H, W, probe[c % 2])
        out.append((n, BLOCK * hb + c // BLOCK, BLOCK * wb + c % BLOCK))
    for n in range(N):
        out += [(n, 0, 0), (n, 0, W - 1), (n, H - 1, 0), (n, H - 1, W - 1)]
        for j in range(1, H // BLOCK):
            out += [(n, BLOCK * j - 1, (13 * j + 3 + n) % W), (n, BLOCK * j, (13 * j + 3 + n) % W)]
        for j in range(1, W // BLOCK):
            out += [(n, (11 * j + 5 + n) % H, BLOCK * j - 1), (n, (11 * j + 5 + n) % H, BLOCK * j)]
    for m in sorted(set([t for t in range(TILE_BLOCKS - 1, M, TILE_BLOCKS)] + [t for t in range(TILE_BLOCKS, M, TILE_BLOCKS)] + [M - 1])):
        n, hb, wb = block_of(N, H, W, m)
        out += [(n, BLOCK * hb, BLOCK * wb), (n, BLOCK * hb + BLOCK - 1, BLOCK * wb + BLOCK - 1)]
    pts = [(n, h >> g, w >> g) for (n, h, w) in out]
    pts += [(0, Hg // 2, Wg // 2), (N - 1, (Hg // 2 + 1) % Hg, (Wg // 2 + 1) % Wg)]
    return sorted(set(pts))


def seam_levels(shape, g):
    """The four levels with R.IMPULSE_VALUES on seam_sources of level g (one map, in two channels) and zeros in the other levels."""
    N, H, W, Cg, Co = shape
    ps = [torch.zeros((N, Cg, H >> l, W >> l), dtype=torch.float64) for l in range(LEVELS)]
    maps = R.impulse_maps(N, Cg, H >> g, W >> g, seam_sources(N, H, W, g), 1)
    assert len(maps) == 1
    ps[g] = maps[0]
    return ps


def seam_outputs(N, H, W):
    """Output pixels on the same seams (seam_sources of level 0): where the data gradient's dy carries its impulses."""
    return seam_sources(N, H, W, 0)
