"""float64 references of the convolution kernels that tests/test_conv_fp64_gpu.py pins (csrc/conv*.hip, wgrad*.hip, winograd*.hip), the
two exact data sets of that module and the fp32 emulations that show WHY those data sets are exact.

Plain torch on the CPU: explicit loops over the taps, one matmul over the channels per tap, strided slices of a zero-padded copy.  No
F.conv2d, no autograd: tests/test_conv_ref_cpu.py checks every function here against those in float64, so that a wrong reference cannot
make a GPU test pass.  Tensors are NCHW, weights OIHW (ConvTranspose2d: [Cin, Cout, k, k] as in PyTorch); every operand is expected in
float64 already (the caller rounds to the kernel's operand type first, then .double())."""
import torch


def out_size(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def _padded(x, p):
    N, C, H, W = x.shape
    xp = torch.zeros((N, C, H + 2 * p, W + 2 * p), dtype=x.dtype)
    xp[:, :, p:p + H, p:p + W] = x
    return xp


def _tap(t, r, q, s, Ho, Wo):
    """The pixels of a padded tensor that tap (r, q) pairs with the Ho x Wo output pixels (a view)."""
    return t[:, :, r:r + s * (Ho - 1) + 1:s, q:q + s * (Wo - 1) + 1:s]


def conv2d(x, w, b=None, stride=1, pad=0):
    N, Ci, H, W = x.shape
    Co, _, R, S = w.shape
    Ho, Wo = out_size(H, R, stride, pad), out_size(W, S, stride, pad)
    xp = _padded(x, pad)
    y = torch.zeros((N, Co, Ho * Wo), dtype=x.dtype)
    for r in range(R):
        for q in range(S):
            y += torch.matmul(w[:, :, r, q], _tap(xp, r, q, stride, Ho, Wo).reshape(N, Ci, Ho * Wo))
    y = y.reshape(N, Co, Ho, Wo)
    return y if b is None else y + b.view(1, Co, 1, 1)


def conv2d_dgrad(dy, w, stride, pad, H, W):
    """Gradient of conv2d(x [N, Ci, H, W], w) with respect to x."""
    N, Co, Ho, Wo = dy.shape
    _, Ci, R, S = w.shape
    dxp = torch.zeros((N, Ci, H + 2 * pad, W + 2 * pad), dtype=dy.dtype)
    d = dy.reshape(N, Co, Ho * Wo)
    for r in range(R):
        for q in range(S):
            _tap(dxp, r, q, stride, Ho, Wo).add_(torch.matmul(w[:, :, r, q].t(), d).reshape(N, Ci, Ho, Wo))
    return dxp[:, :, pad:pad + H, pad:pad + W].contiguous()


def conv2d_wgrad(x, dy, R, S, stride, pad):
    """Gradient of conv2d(x, w [Co, Ci, R, S]) with respect to w."""
    N, Ci, H, W = x.shape
    _, Co, Ho, Wo = dy.shape
    xp = _padded(x, pad)
    d = dy.reshape(N, Co, Ho * Wo)
    dw = torch.zeros((Co, Ci, R, S), dtype=x.dtype)
    for r in range(R):
        for q in range(S):
            dw[:, :, r, q] = torch.matmul(d, _tap(xp, r, q, stride, Ho, Wo).reshape(N, Ci, Ho * Wo).transpose(1, 2)).sum(0)
    return dw


def conv_transpose2d(x, w, b=None, stride=1, pad=0):
    """nn.ConvTranspose2d (output_padding 0): x [N, Ci, H, W], w [Ci, Co, k, k] -> [N, Co, (H - 1) stride - 2 pad + k, ...]; every
    input pixel adds x w[:, :, r, q] at output (h stride - pad + r, w stride - pad + q).  Pixels no tap reaches are 0 (+ bias)."""
    N, Ci, H, W = x.shape
    _, Co, R, S = w.shape
    full = torch.zeros((N, Co, (H - 1) * stride + R, (W - 1) * stride + S), dtype=x.dtype)
    xf = x.reshape(N, Ci, H * W)
    for r in range(R):
        for q in range(S):
            _tap(full, r, q, stride, H, W).add_(torch.matmul(w[:, :, r, q].t(), xf).reshape(N, Co, H, W))
    y = full[:, :, pad:full.shape[2] - pad, pad:full.shape[3] - pad].contiguous()
    return y if b is None else y + b.view(1, Co, 1, 1)


def accumulate(base, y):
    """The accumulate form of every kernel: dst = dst + result."""
    return base + y


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def bf16_rne(t):
    """fp32 -> nearest bf16 (ties to even) in integer arithmetic, as float32 (the rounding csrc/igemm_common.h bf16_bits_rne documents)."""
    u = t.float().contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return (u - ((u >> 31) << 32)).to(torch.int32).view(torch.float32)


# ---- the exact data sets ------------------------------------------------------------------------------------------------------------
def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).double()


def dense_x(shape, seed):
    """{-4 .. 4} / 4."""
    return _ints(shape, -4, 4, seed) / 4


def dense_w(shape, seed, winograd=False):
    """{-8 .. 8} / 8; for Winograd multiples of 1 / 2 in [-1, 1], so that G g G^T (entries of G: 1, 1/2) stays on a 2^-3 grid."""
    return _ints(shape, -2, 2, seed) / 2 if winograd else _ints(shape, -8, 8, seed) / 8


def dense_bias(n, seed):
    """Multiples of 1 / 32 in [-1, 1]."""
    return _ints((n, ), -32, 32, seed) / 32


def distinct_w(Co, Ci, R, S, seed=0):
    """m / 128 with odd |m| <= 127 and, within any window of 128 consecutive (co, ci, tap) indices, 128 distinct values: a term that
    lands at the wrong output channel, input channel or tap changes the result instead of cancelling.  8 significant bits at the most:
    exact in bf16 and fp16."""
    n = Co * Ci * R * S
    i = (torch.arange(n) * 37 + seed) % 128  # 37 is odd: a bijection of every run of 128 indices
    m = torch.where(i < 64, 2 * i + 1, -(2 * (i - 64) + 1))
    return (m.double() / 128).reshape(Co, Ci, R, S)


IMPULSE_VALUES = (1.0, -2.0, 0.5)
M_TILES = (64, 128, 256)  # rows of the library's M tiles (csrc/igemm_kernel.h launch_igemm_ns: BM)


def seam_pixels(N, H, W, Hd, Wd, stride, tile_rows=64, extra=()):
    """Pixels (n, h, w) of an [N, H, W] map on the seams of a kernel that walks the [N, Hd, Wd] map on the other side of a stride-`stride`
    convolution in tiles of `tile_rows` flattened pixels (a divisor of every M tile, so that every tile's boundaries are among them): the
    first and last pixel of every image, the pixel on each side of every tile boundary and, for stride 2, one pixel of each parity class; `extra` adds (h, w)
    pairs to every image."""
    assert all(t % tile_rows == 0 for t in M_TILES), tile_rows
    big = H >= Hd  # this map is the finer one: a pixel of the other map lies at (h stride, w stride) here
    pts = []
    for n in range(N):
        pts += [(n, 0, 0), (n, H - 1, W - 1)]
        pts += [(n, h, w) for (h, w) in extra if h < H and w < W]
    if stride == 2 and H > 4 and W > 4:
        pts += [(0, H // 2 | 1, W // 2 | 1), (0, H // 2 | 1, (W // 2 | 1) - 1), (N - 1, (H // 2 | 1) - 1, W // 2 | 1), (N - 1, (H // 2 | 1) - 1, (W // 2 | 1) - 1)]
    for m in range(tile_rows, N * Hd * Wd, tile_rows):
        for mm in (m - 1, m):
            n, hd, wd = mm // (Hd * Wd), mm // Wd % Hd, mm % Wd
            h, w = (hd * stride, wd * stride) if big else (hd // stride, wd // stride)
            pts.append((n, min(h, H - 1), min(w, W - 1)))
    return sorted(set(pts))


def separate(pts, dist):
    """Greedy split of the pixels into sets in which two pixels of one image differ by >= dist in h or in w: no output of a kernel
    with a support below dist sees two of them."""
    sets = []
    for p in pts:
        for s in sets:
            if all(q[0] != p[0] or max(abs(q[1] - p[1]), abs(q[2] - p[2])) >= dist for q in s):
                s.append(p)
                break
        else:
            sets.append([p])
    return sets


def impulse_maps(N, C, H, W, pts, dist, two_channels=True):
    """One [N, C, H, W] map per set of separate(pts, dist): zero except at the set's pixels, which carry a value of IMPULSE_VALUES in
    channel C - 1 (the last real channel) or, in turn, in another channel — and, with two_channels, every third pixel in both."""
    maps = []
    j = 0
    for s in separate(pts, dist):
        x = torch.zeros((N, C, H, W), dtype=torch.float64)
        for (n, h, w) in s:
            v = IMPULSE_VALUES[j % 3]
            other = (5 * j + 1) % C
            both = two_channels and j % 3 == 0
            if both or j % 2 == 0:
                x[n, C - 1, h, w] = v
            if both or j % 2 == 1:
                x[n, other, h, w] = IMPULSE_VALUES[(j + 1) % 3] if both else v
            j += 1
        maps.append(x)
    return maps


def representable(t, dtype):
    return bool((t.to(dtype).double() == t.double()).all())


# ---- why the data sets are exact: fp32 evaluation in three summation orders ----------------------------------------------------------
def conv_terms(x, w, stride, pad):
    """The products of conv2d in float32: cols [M, K], wk [K, Co] with K = (tap, channel) — term k of output (m, co) is cols[m, k] wk[k, co]."""
    N, Ci, H, W = x.shape
    Co, _, R, S = w.shape
    Ho, Wo = out_size(H, R, stride, pad), out_size(W, S, stride, pad)
    xp = _padded(x, pad)
    cols = torch.stack([_tap(xp, r, q, stride, Ho, Wo) for r in range(R) for q in range(S)], 0)  # [RS, N, Ci, Ho, Wo]
    cols = cols.permute(1, 3, 4, 0, 2).reshape(N * Ho * Wo, R * S * Ci)
    wk = w.permute(2, 3, 1, 0).reshape(R * S * Ci, Co)
    return cols.float(), wk.float()


def fp32_sums(cols, wk, block=64):
    """sum_k cols[m, k] wk[k, co] evaluated in float32 three ways — forward, reversed and pairwise (a binary tree) — every product and every
    addition rounded to float32 (elementwise float32 ops; no matmul, whose order is the library's own business).  [3, M, Co]."""
    M, K = cols.shape
    Co = wk.shape[1]
    fwd = torch.zeros((M, Co), dtype=torch.float32)
    rev = torch.zeros((M, Co), dtype=torch.float32)
    for k in range(K):
        fwd += cols[:, k, None] * wk[None, k]
        rev += cols[:, K - 1 - k, None] * wk[None, K - 1 - k]
    pair = torch.zeros((M, Co), dtype=torch.float32)
    for m0 in range(0, M, block):
        t = cols[m0:m0 + block, :, None] * wk[None]  # [block, K, Co]
        while t.shape[1] > 1:
            if t.shape[1] % 2:
                t = torch.cat([t, torch.zeros_like(t[:, :1])], 1)
            t = t[:, 0::2] + t[:, 1::2]
        pair[m0:m0 + block] = t[:, 0]
    return torch.stack([fwd, rev, pair])


def abs_sum_bound(x, w, stride, pad):
    """max over the outputs of sum |term|: bounds every partial sum of every summation order."""
    return float(conv2d(x.abs(), w.abs(), None, stride, pad).max())


# ---- Winograd F(2x2, 3x3) in float32 -------------------------------------------------------------------------------------------------
BT = torch.tensor([[1., 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]])
G = torch.tensor([[1., 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]])
AT = torch.tensor([[1., 1, 1, 0], [0, 1, -1, -1]])


def _mm32(a, b):
    """a @ b with every product and every addition rounded to float32, summed in index order (broadcast elementwise ops)."""
    out = torch.zeros(a.shape[:-1] + b.shape[-1:], dtype=torch.float32)
    for k in range(a.shape[-1]):
        out = out + a[..., :, k, None] * b[..., k, None, :]
    return out


def winograd_fp32(x, w, b=None):
    """3x3 / stride 1 / pad 1 convolution through Winograd F(2x2, 3x3), every step in float32: V = B^T d B per 4 x 4 input tile,
    U = G g G^T per filter, M = sum_ci U V (forward channel order), y = A^T M A.  Returns (y, V, U, M) as float32; the caller compares
    each with the same quantity in float64 (winograd_fp64)."""
    return _winograd(x.float(), w.float(), None if b is None else b.float(), torch.float32)


def winograd_fp64(x, w, b=None):
    return _winograd(x.double(), w.double(), None if b is None else b.double(), torch.float64)


def _winograd(x, w, b, dt):
    N, Ci, H, W = x.shape
    Co = w.shape[0]
    th, tw = (H + 1) // 2, (W + 1) // 2
    xp = torch.zeros((N, Ci, 2 * th + 2, 2 * tw + 2), dtype=dt)
    xp[:, :, 1:H + 1, 1:W + 1] = x
    d = torch.stack([torch.stack([xp[:, :, i:i + 2 * th:2, j:j + 2 * tw:2] for j in range(4)], -1) for i in range(4)], -2)  # [N, Ci, th, tw, 4, 4]
    bt, g, at = BT.to(dt), G.to(dt), AT.to(dt)
    mm = _mm32 if dt == torch.float32 else torch.matmul
    V = mm(mm(bt.expand(N, Ci, th, tw, 4, 4), d), bt.t().expand(N, Ci, th, tw, 4, 4))
    U = mm(mm(g.expand(Co, Ci, 4, 3), w), g.t().expand(Co, Ci, 3, 4))  # [Co, Ci, 4, 4]
    M = torch.zeros((N, Co, th, tw, 4, 4), dtype=dt)
    for ci in range(Ci):
        M = M + U[None, :, ci, None, None] * V[:, None, ci]
    y4 = mm(mm(at.expand(N, Co, th, tw, 2, 4), M), at.t().expand(N, Co, th, tw, 4, 2))  # [N, Co, th, tw, 2, 2]
    y = y4.permute(0, 1, 2, 4, 3, 5).reshape(N, Co, 2 * th, 2 * tw)[:, :, :H, :W]
    if b is not None:
        y = y + b.view(1, Co, 1, 1)
    return y.contiguous(), V, U, M


# ---- the cases of tests/test_conv_fp64_gpu.py (checked on the CPU in tests/test_conv_ref_cpu.py) ---------------------------------------
# N, Ci, Co, k, stride, pad, H, W
FWD_CASES = [
    (2, 64, 64, 3, 1, 1, 16, 12),  # the baseline
    (3, 128, 64, 1, 1, 0, 9, 7),  # M = 189 straddles every M tile
    (1, 64, 128, 3, 2, 1, 18, 14),  # stride 2, even map
    (1, 64, 64, 3, 2, 1, 17, 13),  # stride 2, odd map
    (2, 3, 64, 7, 2, 3, 32, 40),  # the stem: Ci padded to 4
    (1, 256, 256, 3, 1, 1, 12, 12),  # K = 2304
    (1, 512, 512, 3, 1, 1, 2, 2),  # K = 4608 on a map smaller than the halo
    (1, 64, 192, 3, 1, 1, 10, 9),  # Co = 192 crosses a 128 tile and is no multiple of 256
    (1, 64, 64, 3, 1, 1, 16, 32),  # Hd % 8 == 0, Wd % 16 == 0, Cs % 32 == 0: the 8 x 16 pixel-patch kernels (csrc/conv.hip patch_eligible)
]
DGRAD_CASES = [c for c in FWD_CASES if c[1] % 64 == 0]  # the gradient's channel count Ci is the kernel's Cd: a multiple of 64
WGRAD_CASES = [FWD_CASES[i] for i in (0, 2, 3, 4, 5, 6)]  # those of tests/test_ops_gpu.py WGRAD_CASES
# The weight gradient with several pixel splits (tests/test_wgrad_fp64_gpu.py); tests/test_wgrad_cases_cpu.py asks the library's own plan
# functions whether each case still reaches what its comment names.  P = N Ho Wo pixels, `splits` slabs of pchunk pixels each, G thread
# groups in the slab reduction.  None of these has the pixel-patch form (W % 16 != 0, or not 3 x 3 / stride 1).
WGRAD_SPLIT_CASES = [
    (3, 64, 64, 3, 1, 1, 40, 36),  # P 4320, 9 splits of 480, 64 x 192, G 2: the baseline; image boundaries inside splits
    (2, 64, 64, 3, 1, 1, 37, 59),  # P 4366 (% 16 = 14), 9 splits of 496 (% 32 = 16): a split ends inside a 32-pixel stage and inside a k-step
    (2, 32, 64, 3, 1, 1, 37, 41),  # P 3034, 6 splits of 512, 64 x 128, G 1; Cb = 32: J = 288 padded to Jp = 384
    (2, 96, 64, 3, 1, 1, 37, 41),  # Cb = 96, no multiple of 64: wgrad_reduce_kernel
    (1, 64, 128, 3, 2, 1, 97, 83),  # P 2058, 5 splits of 416, 128 x 128: stride 2, odd map
    (2, 64, 128, 1, 2, 0, 90, 94),  # P 4230, 9 splits of 480, 64 x 64, G 2: 1 x 1 / stride 2 (the downsample convs)
    (4, 128, 64, 1, 1, 0, 45, 47),  # P 8460, 17 splits of 512, 64 x 128, G 4: 1 x 1
    (2, 64, 64, 2, 2, 0, 100, 96),  # P 4800, 10 splits of 480, G 2: the geometry of the ConvTranspose2d weight gradient
    (2, 64, 64, 4, 2, 1, 90, 94),  # P 4230, 9 splits of 480, G 2: FPN level 1 (k = f + 2, stride f)
    (2, 3, 64, 7, 2, 3, 97, 99),  # P 4900, 10 splits of 496: the stem, Cb = 4 (fp32 tensors) or 16 (bf16 storage), I = 3
]
# 3 x 3 / stride 1 / pad 1 with H % 4 == 0 and W % 16 == 0: wgrad_patch_kernel in the 16-bit matrix modes, splits over 4 x 16 patches
WGRAD_PATCH_CASES = [
    (2, 64, 64, 3, 1, 1, 48, 48),  # 72 patches, 9 splits of 8, G 2: the baseline
    (3, 64, 64, 3, 1, 1, 44, 48),  # 99 patches, 13 splits of 8, G 3: the last split partial; three images
    (2, 64, 192, 3, 1, 1, 36, 32),  # 36 patches, 5 splits: three output-channel blocks
    (2, 128, 64, 3, 1, 1, 36, 32),  # 36 patches, 5 splits: two input-channel blocks
    (1, 256, 256, 3, 1, 1, 60, 240),  # 225 patches, 28 splits of 9, G 7: 25 splits hold patches, 3 write zero slabs
]


def wgrad_x_seams(case):
    """Pixels (n, h, w) of x at which a weight-gradient kernel's gather goes wrong first: the four corners, the whole last row and
    column, the input pixel of the output pixel on each side of every multiple of 16 flattened output pixels (split boundaries, k-steps,
    32-pixel LDS stages) and, on the pixel-patch cases, the four pixels around every 4 x 16 patch corner (the halo of the 18-wide rows)."""
    N, Ci, Co, k, s, p, H, W = case
    Ho, Wo = out_size(H, k, s, p), out_size(W, k, s, p)
    extra = [(0, W - 1), (H - 1, 0)] + [(H - 1, w) for w in range(W)] + [(h, W - 1) for h in range(H)]
    if case in WGRAD_PATCH_CASES:
        extra += [(h, w) for i in range(4, H, 4) for j in range(16, W, 16) for h in (i - 1, i) for w in (j - 1, j)]
    return seam_pixels(N, H, W, Ho, Wo, s, tile_rows=16, extra=extra)


SPLITK_CASES = [(1, 512, 512, 3, 1, 1, 10, 12), (2, 256, 64, 10, 8, 1, 40, 40)]
KSPLITS = (2, 5, 7)
CONVT2 = (2, 64, 64, 8, 6)  # N, Ci, Co, H, W: ConvTranspose2d(k = 2, stride 2)
CONVT_GENERAL = [(4, 6, 1), (8, 2, 0)]  # (stride, k, pad) on CONVT_GENERAL_SHAPE
CONVT_GENERAL_SHAPE = (2, 64, 128, 5, 7)
# N, Ci, Co, H, W.  The forward / data-gradient kernel runs every one of these maps in its consecutive-tile (LIN) form (all are below 74
# pixels wide); the weight gradient, whose rule differs, runs 13 x 30 in ragged 8 x 16 patches and the others in its LIN form — always with
# as many workgroups as groups (one patch or 32-tile group each) and the serial slab reduction.  The patch form of the forward kernel,
# several groups per workgroup and the wide reduction: WINO_FWD_PLAN / WINO_WGRAD_PLAN below.
WINOGRAD_CASES = [(2, 64, 64, 13, 30), (2, 64, 64, 20, 20)]
WINOGRAD_SEAM_CASES = [(3, 64, 64, 20, 20), (1, 64, 64, 10, 9), (2, 64, 64, 13, 30)]  # LIN in both kernels (two); forward LIN, weight gradient in ragged patches


def winograd_seams(N, H, W):
    """Pixels on the seams of the Winograd kernels' walk: image corners, the four pixels around the first 8 x 16 patch corner, the last
    row and column, and the first and last 2 x 2 tile of every group of 32 consecutive tiles (the small-map form numbers the tiles
    through the whole batch)."""
    th, tw = (H + 1) // 2, (W + 1) // 2
    pts = []
    for n in range(N):
        pts += [(n, 0, 0), (n, H - 1, W - 1), (n, H - 1, 0), (n, 0, W - 1), (n, H - 1, W // 2), (n, H // 2, W - 1)]
        pts += [(n, h, w) for h in (7, 8) for w in (15, 16) if h < H and w < W]
    total = N * th * tw
    for g in sorted(set(list(range(31, total, 32)) + list(range(32, total, 32)) + [total - 1])):
        n, t = g // (th * tw), g % (th * tw)
        pts.append((n, min(2 * (t // tw), H - 1), min(2 * (t % tw), W - 1)))
    return sorted(set(pts))


# ---- the Winograd kernels on the paths the training step takes (tests/test_winograd_fp64_gpu.py) ----------------------------------------
# Every table below is checked against the library's own host-side plan (dbn_winograd_describe, dbn_winograd_rows, dbn_igemm_bn_rows: nothing
# is launched) in tests/test_winograd_cases_cpu.py: a threshold that moves a case off its path fails there.
# Weight gradient (csrc/winograd_wgrad_f32.hip).  (N, Ci, Cs, Co, H, W): x has Cs stored channels, Ci of them real.
# -> (form, groups, nsub, nsplit, reduction): `groups` 8 x 16 patches ('patch') or groups of 32 consecutive tiles ('lin') in the batch, shared
# among nsplit workgroups per 64 x 64 channel block (nsub blocks); workgroup `split` takes groups split * groups / nsplit up to the next one's first.
WINO_WGRAD_PLAN = {
    (5, 128, 128, 128, 40, 40): ('patch', 75, 4, 64, 'serial'),  # uneven 1 - 2 patches per workgroup; 15 patches per image: ranges cross images
    (3, 256, 256, 256, 29, 77): ('patch', 60, 16, 16, 'serial'),  # 3 - 4 patches per workgroup, ragged in both directions, odd W; 20 patches per image: two ranges cross images
    (3, 512, 512, 512, 20, 20): ('lin', 12, 64, 4, 'serial'),  # layer4's shape: 3 groups per workgroup, 4 per image: every range but the first crosses images
    (2, 64, 64, 64, 64, 128): ('patch', 128, 1, 128, 'wide'),  # the wide reduction at its threshold: 4 splits per lane
    (9, 64, 64, 64, 40, 36): ('patch', 135, 1, 135, 'wide'),  # nsplit % 32 != 0: lanes of 4 and 5 splits
    (3, 64, 64, 64, 61, 125): ('patch', 192, 1, 192, 'wide'),  # ragged map, 6 splits per lane
    (2, 128, 128, 64, 61, 125): ('patch', 128, 2, 128, 'wide'),  # two input-channel blocks (nib = 2)
    (2, 40, 64, 64, 64, 128): ('patch', 128, 1, 128, 'wide'),  # padding channels: the second 32-channel half holds 8 real channels
    (2, 20, 64, 64, 61, 125): ('patch', 128, 1, 128, 'wide'),  # padding channels: the second half is empty
    (40, 128, 128, 64, 20, 20): ('lin', 160, 2, 128, 'wide'),  # consecutive-tile form + wide reduction, 1 - 2 groups per workgroup
}
WINO_WGRAD_CASES = list(WINO_WGRAD_PLAN)
# Forward / data gradient (csrc/winograd_f32.hip).  (N, Ci, Cs, Cd, H, W): the kernel's source has Cs stored channels (Ci real), its
# destination Cd.  The forward conv is Ci -> Cd; the data-gradient launch of the same shape is that of a conv Cd -> Ci (dy: Ci of Cs channels).
# -> (form, rows): rows = 8 x 16 patches or 32-tile groups in the batch = rows of BatchNorm partials = workgroups per 64 output channels
WINO_FWD_PLAN = {
    (2, 64, 64, 64, 15, 77): ('patch', 20),  # ragged in both directions, odd H and W
    (2, 32, 32, 128, 13, 78): ('patch', 20),  # the same with a second column tile (Cd = 128)
    (2, 20, 32, 64, 15, 77): ('patch', 20),  # padded source channels
    (1, 64, 64, 64, 64, 128): ('patch', 64),  # finalize: one full group of 64 rows
    (1, 64, 64, 64, 65, 113): ('patch', 72),  # finalize: a last group of 8 rows, ragged
    (1, 64, 64, 64, 71, 241): ('patch', 144),  # finalize: three groups (64, 64, 16), ragged
    (5, 64, 64, 64, 40, 40): ('lin', 65),  # consecutive-tile form: a last group of one row
    (17, 64, 64, 64, 20, 20): ('lin', 68),  # consecutive-tile form: a last group of four rows
}
WINO_FWD_CASES = list(WINO_FWD_PLAN)
WINO_PATCH_CASES = [c for c in WINO_FWD_CASES if WINO_FWD_PLAN[c][0] == 'patch']
WINO_FINAL_CASES = [c for c in WINO_FWD_CASES if WINO_FWD_PLAN[c][1] >= 64]  # the in-kernel finalize with a full first group of 64 rows
# The implicit-GEMM data gradient with BatchNorm-backward sums and the in-kernel finalize (dbn_igemm_bnsums_t, fp32, tile hint 0):
# (N, Ci, Co, k, stride, pad, H, W) of the forward conv -> rows of partials (dbn_igemm_bn_rows)
IGEMM_FINAL_PLAN = {
    (1, 64, 64, 3, 1, 1, 64, 64): 64,  # one full group
    (1, 64, 64, 3, 1, 1, 33, 125): 65,  # a last group of one row; the last tile partial
    (1, 64, 128, 3, 2, 1, 91, 91): 132,  # stride 2, odd map: four parity classes of 34 + 33 + 33 + 32 rows, three groups
}
IGEMM_FINAL_CASES = list(IGEMM_FINAL_PLAN)


def wino_group_tiles(N, H, W, lin, g):
    """Group g of a Winograd launch over an [N, H, W] map: (image, [(ty, tx), ...]) — its 2 x 2 tiles in the order of the kernel's k-steps.
    lin: 32 consecutive tiles of the image's ceil(H / 2) x ceil(W / 2) grid (the last group of an image may hold fewer); patch form: the 4 x 8
    tiles of an 8 x 16-pixel patch, row by row, INCLUDING those past the map's edge (the kernels multiply zeros there)."""
    TH, TW = (H + 1) // 2, (W + 1) // 2
    if lin:
        n, t = divmod(g, (TH * TW + 31) // 32)
        return n, [(q // TW, q % TW) for q in range(32 * t, min(32 * t + 32, TH * TW))]
    pw = (W + 15) // 16
    n, t = divmod(g, ((H + 7) // 8) * pw)
    return n, [(4 * (t // pw) + i, 8 * (t % pw) + j) for i in range(4) for j in range(8)]


def wino_ranges(groups, nsplit):
    """The groups g0 .. g1 - 1 of every workgroup of the weight gradient (csrc/winograd_wgrad_f32.hip: g0 = split * groups / nsplit)."""
    return [(s * groups // nsplit, (s + 1) * groups // nsplit) for s in range(nsplit)]


def wino_rows(N, H, W, lin):
    """(row [N, H, W], pivot [rows, 3]): the row of BatchNorm partials (= workgroup) that holds each pixel in the forward kernel, and the
    pixel (n, h, w) whose value that workgroup takes as the pivot of its statistics (the first pixel of its first tile)."""
    TH, TW = (H + 1) // 2, (W + 1) // 2
    h, w = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    if lin:
        gpi = (TH * TW + 31) // 32
        row = ((h // 2) * TW + w // 2) // 32
        piv = [(n, 2 * (32 * t // TW), 2 * (32 * t % TW)) for n in range(N) for t in range(gpi)]
    else:
        pw, gpi = (W + 15) // 16, ((H + 7) // 8) * ((W + 15) // 16)
        row = (h // 8) * pw + w // 16
        piv = [(n, 8 * (t // pw), 16 * (t % pw)) for n in range(N) for t in range(gpi)]
    row = row.expand(H, W).unsqueeze(0) + gpi * torch.arange(N).view(N, 1, 1)
    return row, torch.tensor(piv)


def _border(N, H, W):
    pts = []
    for n in range(N):
        pts += [(n, h, w) for h in (0, H - 1) for w in range(W)] + [(n, h, w) for h in range(H) for w in (0, W - 1)]
    return pts


def _patch_corners(N, H, W):
    return [(n, h, w) for n in range(N) for i in range(8, H, 8) for j in range(16, W, 16) for h in (i - 1, i) for w in (j - 1, j)]


def winograd_wgrad_seams(N, H, W, form, groups, nsplit):
    """Pixels (n, h, w) on the seams of the Winograd weight gradient's walk, for impulses in dY or in x: the first and the last in-map
    pixel of every group (patch or 32 consecutive tiles); all four pixels of the first and of the last tile of the first and last group
    of every workgroup's range g0 .. g1 — and with them the pixel on each side of every image boundary inside a range —; the four pixels
    around every 8 x 16 patch corner; the whole first and last row and column (x: their halo lies outside the map and must read as zero;
    ragged maps: the last row and column end inside a patch) — which include the image corners."""
    lin = form == 'lin'
    pts = set(_border(N, H, W))
    if not lin:
        pts |= set(_patch_corners(N, H, W))

    def ends(g):
        n, tiles = wino_group_tiles(N, H, W, lin, g)
        tiles = [t for t in tiles if 2 * t[0] < H and 2 * t[1] < W]
        return n, tiles[0], tiles[-1]

    for g in range(groups):
        n, (ty0, tx0), (ty1, tx1) = ends(g)
        pts |= {(n, 2 * ty0, 2 * tx0), (n, min(2 * ty1 + 1, H - 1), min(2 * tx1 + 1, W - 1))}
    for g0, g1 in wino_ranges(groups, nsplit):
        for g in {g0, g1 - 1}:
            n, first, last = ends(g)
            pts |= {(n, min(2 * ty + i, H - 1), min(2 * tx + j, W - 1)) for (ty, tx) in (first, last) for i in (0, 1) for j in (0, 1)}
    return sorted(pts)


def winograd_patch_seams(N, H, W):
    """Pixels on the seams of the forward kernel's patch form: the four pixels around every 8 x 16 patch corner, the whole first and last row and column
    of every image (the ragged last patch row and column, the image corners) and the first row and column of the ragged patches."""
    pts = set(_border(N, H, W)) | set(_patch_corners(N, H, W))
    for n in range(N):
        pts |= {(n, H // 8 * 8 if H % 8 else H - 8, w) for w in range(0, W, 5)} | {(n, h, W // 16 * 16 if W % 16 else W - 16) for h in range(0, H, 3)}
    return sorted(pts)


def act_coeffs(C, seed):
    """Dyadic coefficients of the BatchNorm + ReLU applied on load: scale in {1/2, 1, 3/2}, shift a multiple of 1/8 in [-1/2, 1/2]: on x in
    {-4..4} / 4, fma(x, scale, shift) is a multiple of 1/8 in [-2, 2] — exact in fp32, with or without the fused rounding."""
    return _ints((C, ), 1, 3, seed) / 2, _ints((C, ), -4, 4, seed + 1) / 8


def apply_act(x, scale, shift):
    """relu(x scale[c] + shift[c]) on an NCHW tensor, in x's precision (float64: exact on the dyadic data)."""
    return (x * scale.to(x.dtype).view(1, -1, 1, 1) + shift.to(x.dtype).view(1, -1, 1, 1)).clamp_min(0)


def winograd_wgrad_emulated(x, dy, form, groups, nsplit, dt):
    """The Winograd weight gradient as csrc/winograd_wgrad_f32.hip evaluates it, every step before the slab sum in `dt` (float32: every
    product and addition rounded, elementwise ops only): D = A dY A^T and V = B^T d B per 2 x 2 tile (zero past the map), per workgroup
    the sum of D (.) V over the tiles of its groups g0 .. g1 — once in the kernel's order and once reversed —, then the sum of the
    workgroups' slabs in float64 and dg = G^T dU G, cast to float32.  x [N, Ci, H, W], dy [N, Co, H, W] (few channels: the channel pairs
    are independent of each other).  Returns dict(D, V, slabs, slabs_rev [nsplit, Co, Ci, 4, 4], dg [Co, Ci, 3, 3])."""
    N, Ci, H, W = x.shape
    Co = dy.shape[1]
    lin = form == 'lin'
    th, tw = ((H + 1) // 2, (W + 1) // 2) if lin else ((H + 7) // 8 * 4, (W + 15) // 16 * 8)
    xp = torch.zeros((N, Ci, 2 * th + 2, 2 * tw + 2), dtype=dt)
    xp[:, :, 1:H + 1, 1:W + 1] = x.to(dt)
    yp = torch.zeros((N, Co, 2 * th, 2 * tw), dtype=dt)
    yp[:, :, :H, :W] = dy.to(dt)
    d = torch.stack([torch.stack([xp[:, :, i:i + 2 * th:2, j:j + 2 * tw:2] for j in range(4)], -1) for i in range(4)], -2)  # [N, Ci, th, tw, 4, 4]
    y2 = torch.stack([torch.stack([yp[:, :, i::2, j::2] for j in range(2)], -1) for i in range(2)], -2)  # [N, Co, th, tw, 2, 2]
    bt, g, at = BT.to(dt), G.to(dt), AT.to(dt)
    mm = _mm32 if dt == torch.float32 else torch.matmul
    V = mm(mm(bt.expand(N, Ci, th, tw, 4, 4), d), bt.t().expand(N, Ci, th, tw, 4, 4))
    D = mm(mm(at.t().expand(N, Co, th, tw, 4, 2), y2), at.expand(N, Co, th, tw, 2, 4))
    slabs = torch.zeros((2, nsplit, Co, Ci, 4, 4), dtype=dt)
    for s, (g0, g1) in enumerate(wino_ranges(groups, nsplit)):
        order = [(n, t) for gq in range(g0, g1) for n, tiles in [wino_group_tiles(N, H, W, lin, gq)] for t in tiles]
        for k, seq in enumerate((order, order[::-1])):
            for n, (ty, tx) in seq:
                slabs[k, s] = slabs[k, s] + D[n, :, ty, tx][:, None] * V[n, :, ty, tx][None]
    dU = slabs[0].double().sum(0)
    dg = torch.matmul(torch.matmul(G.double().t().expand(Co, Ci, 3, 4), dU), G.double().expand(Co, Ci, 4, 3))
    return dict(D=D, V=V, slabs=slabs[0], slabs_rev=slabs[1], dg=dg.float())


def fold_slabs(slab, scale=1.0):
    """Phase 2 of the Winograd weight gradient on the host: slab [nsplit, nob, nib, 4, 4, 64, 64] (any float type) -> float64 sum over the
    splits, G^T . G per (o, i), times scale, cast to float32: [nob 64, nib 64, 3, 3]."""
    nsplit, nob, nib = slab.shape[:3]
    dU = slab.double().sum(0).permute(0, 4, 1, 5, 2, 3).reshape(nob * 64, nib * 64, 4, 4)
    dg = torch.matmul(torch.matmul(G.double().t(), dU), G.double())
    return (dg * scale).float()


def wino_wgrad_data(case, kind):
    """(x [N, Ci, H, W], dy [N, Co, H, W]) in float64 of a WINO_WGRAD_CASES case.  'dense': both on {-4..4} / 4; 'sparse dy' / 'sparse x':
    that operand zero except for impulses (1, -2, 1 / 2, in the last channel and in others) on winograd_wgrad_seams, the other dense."""
    N, Ci, Cs, Co, H, W = case
    form, groups, _, nsplit, _ = WINO_WGRAD_PLAN[case]
    x, dy = dense_x((N, Ci, H, W), 31), dense_x((N, Co, H, W), 34)
    if kind == 'sparse dy':
        (dy, ) = impulse_maps(N, Co, H, W, winograd_wgrad_seams(N, H, W, form, groups, nsplit), 0)
    elif kind == 'sparse x':
        (x, ) = impulse_maps(N, Ci, H, W, winograd_wgrad_seams(N, H, W, form, groups, nsplit), 0)
    else:
        assert kind == 'dense', kind
    return x, dy


def wino_sums_data(case, accumulate):
    """Dyadic operands of a Winograd data gradient with BatchNorm-backward sums, small enough that the two sums per channel are exact in
    fp32 in any order (tests/test_winograd_cases_cpu.py bounds sum |g| and sum |g xhat| on their grids): dy in {-1, 0, 1} / 4, w in
    {-2..2} / 2, the accumulate base in {-8..8} / 8 — dx on the 2^-3 grid —; y, y2 in {-2..2} / 2, rstd in {1, 2}, mean in {-1/2, 0, 1/2} —
    xhat = fma(y, rstd, -mean rstd) on the 2^-1 grid, |xhat| <= 3 —; the mask fma(y, msc, msh) with msc in {-1, -1/2, 1/2, 1}, msh an odd
    multiple of 1/8 (never zero, half of the channels positive: there a pixel read as 0 outside the map would count), or z in {-1, 1}."""
    N, Ci, Cs, Cd, H, W = case
    pm = lambda shape, seed: _ints(shape, 0, 1, seed) * 2 - 1
    d = dict(dy=_ints((N, Ci, H, W), -1, 1, 41) / 4, w=dense_w((Ci, Cd, 3, 3), 42, winograd=True),
             base=_ints((N, Cd, H, W), -8, 8, 43) / 8 if accumulate else None,
             y=_ints((N, Cd, H, W), -2, 2, 44) / 2, y2=_ints((N, Cd, H, W), -2, 2, 45) / 2, z=pm((N, Cd, H, W), 46),
             mean=_ints((Cd, ), -1, 1, 47) / 2, rstd=_ints((Cd, ), 1, 2, 48), mean2=_ints((Cd, ), -1, 1, 49) / 2, rstd2=_ints((Cd, ), 1, 2, 50),
             msc=pm((Cd, ), 51) * _ints((Cd, ), 1, 2, 52) / 2, msh=pm((Cd, ), 53) * (2 * _ints((Cd, ), 0, 3, 54) + 1) / 8)
    d['dx'] = conv2d_dgrad(d['dy'], d['w'], 1, 1, H, W) + (d['base'] if accumulate else 0)
    return d


def bn_backward_sums(dx, y, mean, rstd, m):
    """float64: g = dx [m > 0]; (sum g, sum g xhat, sum |g|, sum |g xhat|) per channel with xhat = (y - mean) rstd."""
    g = dx.double() * (m > 0)
    t = g * (y.double() - mean.double().view(1, -1, 1, 1)) * rstd.double().view(1, -1, 1, 1)
    return g.sum((0, 2, 3)), t.sum((0, 2, 3)), g.abs().sum((0, 2, 3)), t.abs().sum((0, 2, 3))
