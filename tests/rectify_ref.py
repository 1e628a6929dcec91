"""Restatement of db_text_minimal_amd.word_crops' polygon path (dbn_polygon_ribbons and csrc/rectify.hip rectify_u8) in
numpy: the yardstick of tests/test_rectify_*.py.  Written from the definition, not from the C++:
float64 for the ribbon, one operation at a time, and int64 for the pixels.

  boundary_points(poly)            the 2n points: vertices and edge midpoints
  resample(points, S)              S + 1 points of a polyline at equal arclength fractions, and its length
  chains(pts, i, j)                the two boundary chains from point i to point j
  pair_energy(pts, i, j, S)        E(i, j) with the samples A, B
  energies(poly, S)                {(i, j): E} over every non-adjacent pair
  ribbon(poly, S, ends)            dict: knots int32 [S + 1, 4], valid, ends, E, width, length
  rectify(img, knots, valid, h, w) uint8 [h, w, 3]
"""
import numpy as np


def boundary_points(poly):
    v = np.asarray(poly, np.float64)
    n = len(v)
    pts = np.zeros((2 * n, 2), np.float64)
    pts[0::2] = v
    pts[1::2] = (v + np.roll(v, -1, axis=0)) * 0.5
    return pts


def resample(p, S):
    """p [np, 2], np >= 2 -> (points [S + 1, 2] at arclength L k / S, L): on the first segment s whose end lies at or past
    the position, p[s] + ((t - start of s) / length of s) (p[s + 1] - p[s]); the two ends are p[0] and p[-1]"""
    d = p[1:] - p[:-1]
    sl = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    cum = np.concatenate([[0.0], np.cumsum(sl)])  # a running sum, in order
    L = cum[-1]
    t = L * np.arange(S + 1, dtype=np.float64) / S
    s = np.minimum(np.searchsorted(cum[1:], t, side='left'), len(sl) - 1)
    with np.errstate(divide='ignore', invalid='ignore'):
        u = np.where(sl[s] > 0, (t - cum[s]) / sl[s], 0.0)
    out = p[s] + u[:, None] * d[s]
    out[0], out[S] = p[0], p[-1]
    return out, L


def chains(pts, i, j):
    m = len(pts)
    fw = pts[np.arange(i, i + (j - i) % m + 1) % m]
    bw = pts[np.arange(i, i - (i - j) % m - 1, -1) % m]
    return fw, bw


def pair_energy(pts, i, j, S):
    fw, bw = chains(pts, i, j)
    A, _ = resample(fw, S)
    B, _ = resample(bw, S)
    d = A - B
    d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    return np.cumsum(d2)[-1] / (S + 1), A, B, d2


def energies(poly, S=32):
    pts = boundary_points(poly)
    m = len(pts)
    return {(i, j): pair_energy(pts, i, j, S)[0] for i in range(m) for j in range(i + 2, m) if j - i <= m - 2}


def best_pair(E):
    """the smallest E; ties to the smallest (i, j)"""
    best = None
    for ij in sorted(E):
        if best is None or E[ij] < E[best]:
            best = ij
    return best


def energy_gap(E):
    """(second smallest E - smallest E) / smallest E over the pairs other than the chosen one"""
    b = best_pair(E)
    rest = min(v for ij, v in E.items() if ij != b)
    return (rest - E[b]) / max(E[b], np.finfo(np.float64).tiny)


def ribbon(poly, S=32, ends='auto', E=None):
    v = np.asarray(poly, np.float64)
    n = len(v)
    pts = boundary_points(v)
    if ends == 'half':
        i, j = 2 * n - 1, n - 1
    else:
        i, j = best_pair(energies(v, S) if E is None else E)
    e, A, B, d2 = pair_energy(pts, i, j, S)
    W = np.sqrt(d2.max())
    C, length = resample((A + B) * 0.5, S)
    a, b = v[1:-1] - v[0], v[2:] - v[0]
    area2 = np.cumsum(a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1])[-1]
    valid = bool(length > 0 and W > 0 and area2 != 0)
    if ends != 'half':
        d = C[S] - C[0]
        if (C[0, 0] > C[S, 0]) if abs(d[0]) >= abs(d[1]) else (C[0, 1] > C[S, 1]):
            C = C[::-1].copy()
    T = C[np.minimum(np.arange(S + 1) + 1, S)] - C[np.maximum(np.arange(S + 1) - 1, 0)]
    tl = np.sqrt(T[:, 0] * T[:, 0] + T[:, 1] * T[:, 1])
    with np.errstate(divide='ignore', invalid='ignore'):
        N = np.where(tl[:, None] > 0, np.stack([W * (-T[:, 1] / tl), W * (T[:, 0] / tl)], 1), 0.0)
    k = np.rint(1024.0 * np.concatenate([C, N], 1))
    valid = valid and bool((np.abs(k) <= 2 ** 31 - 1).all())
    knots = k.astype(np.int64).astype(np.int32) if valid else np.zeros((S + 1, 4), np.int32)
    return dict(knots=knots, valid=int(valid), ends=(i, j), E=e, width=W, length=length, centre=C, start=pts[i], stop=pts[j])


def rectify(img, knots, valid, h, w):
    """img uint8 [H, W, 3], knots int32 [S + 1, 4] -> uint8 [h, w, 3], all in int64"""
    out = np.zeros((h, w, 3), np.uint8)
    if not valid:
        return out
    H, Wd = img.shape[:2]
    kn = np.asarray(knots).astype(np.int64)
    S = len(kn) - 1
    x, y = np.arange(w, dtype=np.int64), np.arange(h, dtype=np.int64)
    k, r = x * S // w, x * S % w
    c = w * kn[k, 0:2] + r[:, None] * (kn[k + 1, 0:2] - kn[k, 0:2])   # [w, 2]
    n = w * kn[k, 2:4] + r[:, None] * (kn[k + 1, 2:4] - kn[k, 2:4])
    num = 2 * h * c[None] + (2 * y - h)[:, None, None] * n[None]      # [h, w, 2]
    P = (num + h * w) // (2 * h * w)                                  # round half up: the divisor is even
    P5 = (P + 16) >> 5
    i, f = P5 >> 5, P5 & 31
    acc = np.zeros((h, w, 3), np.int64)
    for dy in (0, 1):
        for dx in (0, 1):
            wt = (f[..., 0] if dx else 32 - f[..., 0]) * (f[..., 1] if dy else 32 - f[..., 1])
            xi, yi = i[..., 0] + dx, i[..., 1] + dy
            inside = (xi >= 0) & (xi < Wd) & (yi >= 0) & (yi < H)
            px = img[np.clip(yi, 0, H - 1), np.clip(xi, 0, Wd - 1)].astype(np.int64)
            acc += np.where(inside, wt, 0)[..., None] * px
    return ((acc + 512) >> 10).astype(np.uint8)
