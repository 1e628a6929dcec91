"""numpy restatement of db_text_minimal_amd.render (csrc/render.hip): the strokes of draw_outlines, the heat map of
overlay_heatmap and minmax_scale_u8, operation by operation in the kernels' order.  Integer work is int64 (the bounds
that make 64 bits enough are in csrc/render.hip; stroke_hit_exact is the same predicate on Python integers), float work is
numpy float32 / float64 element-wise arithmetic, which is IEEE and never contracted."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- strokes -----------------------------------------------------------------------------------------------------------
def on_line(px, py, xa, ya, xb, yb):
    """dbn_on_line of csrc/fillpoly.h (cv2 LineIterator, 8-connected, left to right) for int64 arrays px, py"""
    px, py = np.asarray(px, np.int64), np.asarray(py, np.int64)
    dx, dy, x1, y1 = xb - xa, yb - ya, xa, ya
    if dx < 0:
        x1, y1, dx, dy = xb, yb, -dx, -dy
    sy = -1 if dy < 0 else 1
    dy = abs(dy)
    if dy > dx:
        i = (py - y1) * sy
        ok = (i >= 0) & (i <= dy)
        m = (2 * dx * np.where(ok, i, 0) + dy - 1) // (2 * dy)
        return ok & (px == x1 + m)
    i = px - x1
    ok = (i >= 0) & (i <= dx)
    m = (2 * dy * np.where(ok, i, 0) + dx - 1) // (2 * dx) if dx else np.zeros_like(i)
    return ok & (py == y1 + sy * m)


def stroke_hit(px, py, xa, ya, xb, yb, t):
    """4 d^2 <= t^2 for the distance d of pixels (px, py) (int64 arrays) to the closed segment, as csrc/render.hip"""
    px, py = np.asarray(px, np.int64), np.asarray(py, np.int64)
    dx, dy = np.int64(xb - xa), np.int64(yb - ya)
    wx, wy = px - xa, py - ya
    len2, dot, t2 = dx * dx + dy * dy, dx * wx + dy * wy, np.int64(t * t)
    ex, ey = px - xb, py - yb
    cross = np.abs(dx * wy - dy * wx)
    near = cross < (1 << 30)
    side = near & (4 * np.where(near, cross, 0) ** 2 <= t2 * len2)
    return np.where(dot <= 0, 4 * (wx * wx + wy * wy) <= t2, np.where(dot > len2, 4 * (ex * ex + ey * ey) <= t2, side))


def stroke_hit_exact(px, py, xa, ya, xb, yb, t):
    """the same predicate on Python integers (no overflow possible), one pixel"""
    px, py, xa, ya, xb, yb, t = (int(v) for v in (px, py, xa, ya, xb, yb, t))
    dx, dy, wx, wy = xb - xa, yb - ya, px - xa, py - ya
    len2, dot = dx * dx + dy * dy, dx * wx + dy * wy
    if dot <= 0:  # also a zero-length edge: the disc about a
        return 4 * (wx * wx + wy * wy) <= t * t
    if dot > len2:
        return 4 * ((px - xb) ** 2 + (py - yb) ** 2) <= t * t
    return 4 * (dx * wy - dy * wx) ** 2 <= t * t * len2


def select_shapes(shapes):
    """one image's shapes ([K, P, 2] array or list of [P, 2]) -> list of int64 [P, 2], coordinate sums <= 0 dropped"""
    out = []
    for p in shapes:
        p = np.asarray(p).astype(np.int64).reshape(-1, 2)
        if p.sum() > 0:
            out.append(p)
    return out


def edge_mask(H, W, xa, ya, xb, yb, t):
    """(y0, x0, mask): the pixels of an H x W image one edge paints, as a mask over its clipped bounding box (None if empty)"""
    r = 0 if t == 1 else t // 2 + 1
    x0, x1 = max(min(xa, xb) - r, 0), min(max(xa, xb) + r, W - 1)
    y0, y1 = max(min(ya, yb) - r, 0), min(max(ya, yb) + r, H - 1)
    if x0 > x1 or y0 > y1:
        return None
    py, px = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.int64)
    m = on_line(px, py, xa, ya, xb, yb) if t == 1 else stroke_hit(px, py, xa, ya, xb, yb, t)
    return y0, x0, m


def stroke_mask(H, W, shapes, t):
    """bool [H, W]: the pixels draw_outlines paints for one image's shapes (closed, edge i from vertex i - 1 to vertex i;
    an edge that occurs several times is evaluated once)"""
    mask = np.zeros((H, W), bool)
    edges = [np.concatenate([np.roll(p, 1, 0), p], 1) for p in select_shapes(shapes)]
    if not edges:
        return mask
    for xa, ya, xb, yb in np.unique(np.concatenate(edges), axis=0).tolist():
        r = edge_mask(H, W, xa, ya, xb, yb, t)
        if r is not None:
            y0, x0, m = r
            mask[y0:y0 + m.shape[0], x0:x0 + m.shape[1]] |= m
    return mask


def draw_outlines(img, shapes, color=(255, 0, 0), thickness=3):
    out = img.copy()
    out[stroke_mask(img.shape[0], img.shape[1], shapes, thickness)] = np.array(color, np.uint8)
    return out


# ---- heat map ----------------------------------------------------------------------------------------------------------
def _src_coords(dst, src):
    """cv2.resize's table: fx = (float)((dx + 0.5) * scale - 0.5), sx = cvFloor(fx), fx -= sx"""
    scale = 1. / (float(dst) / float(src))
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    return s, f - s.astype(np.float32)


def resize_linear_f32(src, H, W):
    """cv2.resize(src, (W, H)), INTER_LINEAR, on a float32 [h, w] array: float weights, horizontal pass then vertical"""
    src = np.ascontiguousarray(src, np.float32)
    h, w = src.shape
    sx, fx = _src_coords(W, w)
    fx = np.where((sx < 0) | (sx >= w - 1), np.float32(0), fx).astype(np.float32)  # columns: reset to the edge, weight 0
    sx = np.clip(sx, 0, w - 1)
    sx1 = np.minimum(sx + 1, w - 1)
    sy, fy = _src_coords(H, h)
    y0, y1 = np.clip(sy, 0, h - 1), np.clip(sy + 1, 0, h - 1)  # rows: both taps clamped, the fraction kept
    a0, a1 = (np.float32(1) - fx)[None, :], fx[None, :]
    b0, b1 = (np.float32(1) - fy)[:, None], fy[:, None]
    r0 = src[y0][:, sx] * a0 + src[y0][:, sx1] * a1
    r1 = src[y1][:, sx] * a0 + src[y1][:, sx1] * a1
    out = b0 * r0 + b1 * r1
    assert out.dtype == np.float32
    return out


def normalize(v, vmin, vmax):
    """matplotlib.colors.Normalize(vmin, vmax)(v) for a float32 array: numpy runs `v -= vmin; v /= (vmax - vmin)` with
    float64 scalars in double and stores each result as float32; vmin == vmax gives zeros"""
    v = np.asarray(v, np.float32)
    vmin, vmax = np.float64(vmin), np.float64(vmax)
    if vmin == vmax:
        return np.zeros_like(v)
    s = (v.astype(np.float64) - vmin).astype(np.float32)
    return (s.astype(np.float64) / (vmax - vmin)).astype(np.float32)


def color_index(t):
    """Colormap.__call__'s index for float32 t: t * 256, 256 -> 255, truncated, below 0 -> 0, at / above 256 -> 255"""
    xa = np.asarray(t, np.float32) * np.float32(256)
    xa = np.where(xa == 256, np.float32(255), xa)
    idx = np.clip(xa, 0, 255).astype(np.int64)  # truncation (values are >= 0 after the clip)
    return np.where(xa < 0, 0, np.where(xa >= 256, 255, idx))


def table(name):
    path = os.path.join(ROOT, 'db_text_minimal_amd', 'cmaps', name + '.txt')
    return np.array([[int(v) for v in line.split()] for line in open(path)], np.uint8)


def colorize(v, cmap, vmin=None, vmax=None):
    """-> (uint8 [..., 3] colours, index, (vmin, vmax) used); None limits = the array's own minimum and maximum"""
    v = np.asarray(v, np.float32)
    if vmin is None:
        vmin, vmax = float(v.min()), float(v.max())
    idx = color_index(normalize(v, vmin, vmax))
    return table(cmap)[idx], idx, (vmin, vmax)


def blend(img, col, alpha):
    """rint(img * (1 - a) + colour * a) in float32, half to even"""
    a = np.float32(alpha)
    r = img.astype(np.float32) * (np.float32(1) - a) + col.astype(np.float32) * a
    assert r.dtype == np.float32
    return np.clip(np.rint(r), 0, 255).astype(np.uint8)


def resized_map(prob, hw, valid_hw=None, binary=None):
    p = np.asarray(prob, np.float32)
    if valid_hw is not None:
        p = p[:valid_hw[0], :valid_hw[1]]
    if binary is not None:
        p = (p > np.float32(binary)).astype(np.float32)
    return resize_linear_f32(p, hw[0], hw[1])


def overlay_heatmap(img, prob, valid_hw=None, cmap='inferno', alpha=0.6, vmin=None, vmax=None, binary=None):
    """one image: uint8 [H, W, 3] and its float32 map [H', W'] -> uint8 [H, W, 3]"""
    v = resized_map(prob, img.shape[:2], valid_hw, binary)
    col, _, _ = colorize(v, cmap, vmin, vmax)
    return blend(img, col, alpha)


# ---- utils.minmax_scaler_img ---------------------------------------------------------------------------------------------
def minmax_scale_u8(x):
    """x float32 [3, H, W] -> uint8 [H, W, 3]; float32 throughout, truncation; a constant image gives zeros"""
    x = np.asarray(x, np.float32).transpose(1, 2, 0)
    lo, hi = x.min(), x.max()
    if not hi > lo:
        return np.zeros(x.shape, np.uint8)
    f = (np.float32(1) / (hi - lo)) * np.float32(255)
    v = (x - lo) * f
    assert v.dtype == np.float32
    return np.clip(v.astype(np.int64), 0, 255).astype(np.uint8)
