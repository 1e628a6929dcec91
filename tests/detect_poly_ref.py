"""TEST MODEL of detect_polygons (db_text_minimal_amd/postprocess.py, csrc/detect.hip) in numpy and Python integers.

Semantics restated from the module docstring of db_text_minimal_amd.postprocess, independently of the kernels:
  crack       (pixel p of candidate C, side s) whose 4-neighbour across s is background or outside the image.  Sides
              L, B, R, T (0..3) are walked with C on the left on screen (y down): L down, B right, R up, T left.
  successor   of a crack: the pixel `ahead` (one step along the motion) and `diag` (ahead, one step toward the
              background): diag in the foreground -> (diag, s - 1); else ahead in the foreground -> (ahead, s); else
              (p, s + 1).  `crack_walk` follows it serially from the head, the L crack of C's raster-first pixel.
  visits      consecutive cracks of one pixel collapse into one visit (cyclically; the head's visit comes first).
  compress    CHAIN_APPROX_SIMPLE: a visit is kept where the step direction into it differs from the one out of it.
  arc_length  a + b * sqrt(2) over the compressed closed contour (a axis steps, b diagonal steps), fp64.
  approx      approxPolyDP(closed) as OpenCV 4.x approx.cpp: three passes for the initial split, the slice stack,
              the clean-up pass; fp64, integer coordinates.
  polygons    polygons_from_bitmap (the reference's src/postprocess.py:54-103) per candidate of detect_ref's labels:
              approx < 4 points -> skip; box_thresh > score64 -> skip; unclip by shapely's area * ratio / length through
              dbn_poly_offset_paths, more than one path -> skip; sside of the min-area rectangle < 5 -> skip; scale in
              fp64 with half-to-even rounding.
"""
import math

import numpy as np

from db_text_minimal_amd.gt_maps import _area, _length, offset_polygon_paths
import detect_ref as R

SIDE_D = [(0, 1), (1, 0), (0, -1), (-1, 0)]  # (dx, dy) of the motion along L, B, R, T
SIDE_N = [(-1, 0), (0, 1), (1, 0), (0, -1)]  # (dx, dy) toward the background across L, B, R, T


def crack_next(bm, y, x, s):
    H, W = bm.shape

    def fg(v, u):
        return 0 <= v < H and 0 <= u < W and bool(bm[v, u])

    dx, dy = SIDE_D[s]
    nx, ny = SIDE_N[s]
    ay, ax = y + dy, x + dx
    gy, gx = ay + ny, ax + nx
    if fg(gy, gx):
        return gy, gx, (s + 3) % 4
    if fg(ay, ax):
        return ay, ax, s
    return y, x, (s + 1) % 4


def crack_walk(bm, y, x):
    """the crack cycle of the outer border from the L crack of the raster-first pixel (y, x): [(y, x, side), ...]"""
    bm = np.asarray(bm, bool)
    head = (y, x, 0)
    out = [head]
    c = crack_next(bm, *head)
    while c != head:
        out.append(c)
        c = crack_next(bm, *c)
    return out


def pixel_visits(cracks):
    """[(y, x), ...]: cyclic runs of cracks on one pixel collapsed; the run holding the head first."""
    pix = [(c[0], c[1]) for c in cracks]
    starts = [i for i in range(len(pix)) if pix[i] != pix[i - 1]]
    if not starts:
        return [pix[0]]
    if starts[0] != 0:  # the head's run wraps round the end of the list: it begins at the last start
        starts = [starts[-1]] + starts[:-1]
    return [pix[i] for i in starts]


def compress(visits):
    """CHAIN_APPROX_SIMPLE of a closed pixel sequence [(y, x), ...] -> [(y, x), ...]"""
    n = len(visits)
    if n == 1:
        return list(visits)
    out = []
    for k in range(n):
        (py, px), (cy, cx), (ny, nx) = visits[k - 1], visits[k], visits[(k + 1) % n]
        if (cy - py, cx - px) != (ny - cy, nx - cx):
            out.append(visits[k])
    return out


def contour(bm, y, x):
    """compressed outer border of the component whose raster-first pixel is (y, x): int64 [P, 2] of (x, y)"""
    c = compress(pixel_visits(crack_walk(bm, y, x)))
    return np.array([(b, a) for a, b in c], np.int64).reshape(-1, 2)


def arc_length(c):
    a = b = 0
    n = len(c)
    for i in range(n):
        dx, dy = abs(int(c[(i + 1) % n][0]) - int(c[i][0])), abs(int(c[(i + 1) % n][1]) - int(c[i][1]))
        if dx == 0 or dy == 0:
            a += dx + dy
        else:
            assert dx == dy
            b += dx
    return a + b * math.sqrt(2.0)


def approx_poly_dp(c, eps, cleanup=True):
    """approxPolyDP(c, eps, closed=True) of OpenCV 4.x approx.cpp on integer points [(x, y), ...] -> [(x, y), ...]"""
    src = [(int(p[0]), int(p[1])) for p in c]
    count = len(src)
    if count == 0:
        return []
    eps = eps * eps
    # 1. the initial split: three passes, each from the farthest point of the previous one (first strict maximum)
    pos, rs = 0, 0
    le_eps = False
    for _ in range(3):
        pos = (pos + rs) % count
        sx, sy = src[pos]
        max_dist = 0.0
        for j in range(1, count):
            px, py = src[(pos + j) % count]
            dx, dy = float(px - sx), float(py - sy)
            d = dx * dx + dy * dy
            if d > max_dist:
                max_dist, rs = d, j
        le_eps = max_dist <= eps
    dst = []
    stack = []
    if not le_eps:
        s0 = pos % count
        e0 = (rs + s0) % count
        stack.append((e0, s0))
        stack.append((s0, e0))
    else:
        dst.append(src[pos])
    # 2. slices: accept, writing the start point, or split at the point of largest |cross| (first strict maximum)
    while stack:
        a, e = stack.pop()
        ex, ey = src[e]
        sx, sy = src[a]
        p = (a + 1) % count
        if p != e:
            dx, dy = float(ex - sx), float(ey - sy)
            max_dist, split = 0.0, None
            while p != e:
                px, py = src[p]
                d = abs((py - sy) * dx - (px - sx) * dy)
                if d > max_dist:
                    max_dist, split = d, p
                p = (p + 1) % count
            le = max_dist * max_dist <= eps * (dx * dx + dy * dy)
        else:
            le = True
        if le:
            dst.append((sx, sy))
        else:
            stack.append((split, e))
            stack.append((a, split))
    # 3. clean-up, in place as approx.cpp does it (its reads may see its own writes once they wrap)
    if not cleanup:
        return dst
    count = new_count = len(dst)
    pos = count - 1

    def read():
        nonlocal pos
        v = dst[pos]
        pos = pos + 1 if pos + 1 < count else 0
        return v

    start = read()
    wpos = pos
    pt = read()
    i = 0
    while i < count and new_count > 2:
        end = read()
        dx, dy = float(end[0] - start[0]), float(end[1] - start[1])
        dist = abs((pt[0] - start[0]) * dy - (pt[1] - start[1]) * dx)
        inner = (pt[0] - start[0]) * (end[0] - pt[0]) + (pt[1] - start[1]) * (end[1] - pt[1])
        if dist * dist <= 0.5 * eps * (dx * dx + dy * dy) and dx != 0 and dy != 0 and inner >= 0:
            new_count -= 1
            dst[wpos] = start = end
            wpos = wpos + 1 if wpos + 1 < count else 0
            pt = read()
            i += 2
            continue
        dst[wpos] = start = pt
        wpos = wpos + 1 if wpos + 1 < count else 0
        pt = end
        i += 1
    return dst[:new_count]


def filled_sums(pred, lab, bm, cands):
    """per candidate: (T, count) with T = sum over filled(C) of floor(v * 2^56) (v clamped to [-127, 127]: the device's
    fixed point, exact for |v| >= 2^-33)"""
    H, W = bm.shape
    flat = lab.ravel().astype(np.int64)
    bflat = bm.ravel()
    v = np.clip(pred.ravel().astype(np.float64), -127.0, 127.0)
    hi = np.trunc(v * 2.0 ** 24).astype(np.int64)
    lo = np.trunc((v - hi * 2.0 ** -24) * 2.0 ** 56).astype(np.int64)
    order = np.argsort(flat, kind='stable')
    sl = flat[order]
    roots, starts = np.unique(sl, return_index=True)
    shi, slo = np.add.reduceat(hi[order], starts), np.add.reduceat(lo[order], starts)
    cnt = np.diff(np.r_[starts, len(sl)])
    border = np.unique(np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]]))
    outside = set(int(r) for r in border if not bflat[r])
    slot = {r: k for k, r in enumerate(cands)}
    T = [0] * len(cands)
    C = [0] * len(cands)
    for r, a_hi, a_lo, c in zip(roots.tolist(), shi.tolist(), slo.tolist(), cnt.tolist()):
        if r in outside:
            continue
        a = r
        while True:
            if bflat[a] and a in slot:
                T[slot[a]] += a_hi * 2 ** 32 + a_lo
                C[slot[a]] += c
            if a % W == 0:
                break
            b = int(flat[a - 1])
            if b in outside:
                break
            a = b
    return T, C


def polygons(pred, thresh=0.3, box_thresh=0.7, max_candidates=1000, unclip_ratio=1.5, dest_hw=None):
    """polygons_from_bitmap for pred [H, W] fp32 -> dict(roots, contours (compressed, per candidate), score64,
    approx, paths, sside, polys (kept: int64 [P, 2]), scores (kept: float), near (scaled coordinates within 1e-6 of a
    rounding boundary))."""
    pred = np.asarray(pred, np.float32)
    H, W = pred.shape
    bm = pred > np.float32(thresh)
    lab = R.label(bm)
    flat = lab.ravel()
    idx = np.arange(H * W)
    roots = idx[(flat == idx) & bm.ravel()][::-1]
    cands = [int(r) for r in roots[:max_candidates]]
    T, C = filled_sums(pred, lab, bm, cands)
    dh, dw = dest_hw if dest_hw is not None else (H, W)
    res = dict(labels=lab, count=len(roots), roots=np.array(cands, np.int64), contours=[], score64=[], approx=[], paths=[], sside=[],
               polys=[], scores=[], near=0)
    for k, r in enumerate(cands):
        y, x = divmod(r, W)
        c = contour(bm, y, x)
        s64 = T[k] / (C[k] << 56)
        ap, paths, sside, poly, near = host_stage(c, s64, H, W, box_thresh, unclip_ratio, (dh, dw))
        for key, v in (('contours', c), ('score64', s64), ('approx', ap), ('paths', paths), ('sside', sside)):
            res[key].append(v)
        res['near'] += near
        if poly is not None:
            res['polys'].append(poly)
            res['scores'].append(s64)
    return res


def host_stage(c, s64, H, W, box_thresh=0.7, unclip_ratio=1.5, dest_hw=None):
    """postprocess.py:72-101 for one compressed contour c (int [P, 2] (x, y)) with fp64 score s64 -> (approx int64
    [A, 2], offset paths (0 if not reached), sside (-1 if not reached), scaled int64 [Q, 2] polygon or None if skipped,
    number of scaled coordinates within 1e-6 of a rounding boundary)."""
    dh, dw = dest_hw if dest_hw is not None else (H, W)
    ap = approx_poly_dp(c, 0.005 * arc_length(c))
    apa = np.array(ap, np.int64).reshape(-1, 2)
    paths, sside = 0, -1.0
    if len(ap) < 4 or box_thresh > s64:
        return apa, paths, sside, None, 0
    a = apa.astype(np.float64)
    off, paths = offset_polygon_paths(a, _area(a) * unclip_ratio / _length(a))
    if paths > 1:
        return apa, paths, sside, None, 0
    if len(off):
        q = sorted(set((int(v), int(u)) for u, v in off))
        sside = float(R.rect_corners(R.min_area_rect(R.hull([(u, v) for v, u in q])))[1])
    if sside < 5:
        return apa, paths, sside, None, 0
    sx, sy = off[:, 0] / W * dw, off[:, 1] / H * dh
    near = int(np.sum(np.abs(np.abs(sx - np.floor(sx)) - 0.5) < 1e-6) + np.sum(np.abs(np.abs(sy - np.floor(sy)) - 0.5) < 1e-6))
    p = off.copy()
    p[:, 0] = np.clip(np.round(sx), 0, dw)
    p[:, 1] = np.clip(np.round(sy), 0, dh)
    return apa, paths, sside, p, near
