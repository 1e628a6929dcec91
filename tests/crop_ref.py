"""Scalar restatement of db_text_minimal_amd.word_crops (dbn_perspective_maps and csrc/resample.hip
warp_perspective_u8), written as OpenCV 4.2 computes it: the yardstick of tests/test_word_crops_*.py.
  perspective_map   cv2.getPerspectiveTransform: the 8 x 8 system (float x float products, as Point2f holds them) solved
                    by LUImpl (partial pivoting, eps = DBL_EPSILON * 100, zeros when singular), then M[8] = 1
  invert3           cv2.invert(DECOMP_LU) of a 3 x 3 double matrix: det3, cofactors times 1/d, zeros when d == 0
  warp_perspective  cv2.warpPerspective INTER_LINEAR, BORDER_CONSTANT 0 (WarpPerspectiveInvoker's blocks + remapBilinear)
Double arithmetic in Python floats / numpy float64 (IEEE, no FMA); rounding is cvRound (half to even)."""
import numpy as np

DBL_EPS = 2.220446049250313e-16


def perspective_map(quad, h, w):
    """quad [4][2] (x, y) -> 9 doubles: getPerspectiveTransform onto (0, 0), (w, 0), (w, h), (0, h)"""
    q = np.asarray(quad, np.float32).reshape(4, 2)
    u = [np.float32(0), np.float32(w), np.float32(w), np.float32(0)]
    v = [np.float32(0), np.float32(0), np.float32(h), np.float32(h)]
    a = [[0.0] * 8 for _ in range(8)]
    b = [0.0] * 8
    for i in range(4):
        x, y = q[i, 0], q[i, 1]
        a[i][0] = a[i + 4][3] = float(x)
        a[i][1] = a[i + 4][4] = float(y)
        a[i][2] = a[i + 4][5] = 1.0
        a[i][6] = float(np.float32(-x) * u[i])
        a[i][7] = float(np.float32(-y) * u[i])
        a[i + 4][6] = float(np.float32(-x) * v[i])
        a[i + 4][7] = float(np.float32(-y) * v[i])
        b[i] = float(u[i])
        b[i + 4] = float(v[i])
    ok = True
    for i in range(8):
        k = i
        for j in range(i + 1, 8):
            if abs(a[j][i]) > abs(a[k][i]):
                k = j
        if abs(a[k][i]) < DBL_EPS * 100:
            ok = False
            break
        if k != i:
            a[i], a[k] = a[k], a[i]  # the whole rows: columns < i are dead below the diagonal
            b[i], b[k] = b[k], b[i]
        d = -1.0 / a[i][i]
        for j in range(i + 1, 8):
            alpha = a[j][i] * d
            for c in range(i + 1, 8):
                a[j][c] += alpha * a[i][c]
            b[j] += alpha * b[i]
    if ok:
        for i in range(7, -1, -1):
            s = b[i]
            for c in range(i + 1, 8):
                s -= a[i][c] * b[c]
            b[i] = s / a[i][i]
    return (b if ok else [0.0] * 8) + [1.0]


def invert3(S):
    S = [float(s) for s in S]
    det = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6])
    if det == 0.0:
        return [0.0] * 9
    d = 1.0 / det
    return [(S[4] * S[8] - S[5] * S[7]) * d, (S[2] * S[7] - S[1] * S[8]) * d, (S[1] * S[5] - S[2] * S[4]) * d,
            (S[5] * S[6] - S[3] * S[8]) * d, (S[0] * S[8] - S[2] * S[6]) * d, (S[2] * S[3] - S[0] * S[5]) * d,
            (S[3] * S[7] - S[4] * S[6]) * d, (S[1] * S[6] - S[0] * S[7]) * d, (S[0] * S[4] - S[1] * S[3]) * d]


def maps(quads, h, w):
    """-> (forward, inverse) fp64 [K, 3, 3]"""
    fwd = np.array([perspective_map(q, h, w) for q in np.asarray(quads, np.float32).reshape(-1, 4, 2)], np.float64).reshape(-1, 3, 3)
    inv = np.array([invert3(m) for m in fwd.reshape(-1, 9)], np.float64).reshape(-1, 3, 3)
    return fwd, inv


def block_width(h, w):
    """WarpPerspectiveInvoker (BLOCK_SZ = 32): bh0 = min(16, rows), bw0 = min(1024 / bh0, cols)"""
    bh0 = min(16, h)
    return min(1024 // bh0, w)


def _clamp_int_range(v):
    """max((double)INT_MIN, min((double)INT_MAX, v)) with std::min / std::max's comparisons (NaN -> INT_MAX)"""
    m = np.where(v < 2147483647.0, v, 2147483647.0)
    return np.where(-2147483648.0 < m, m, -2147483648.0)


def warp_perspective(img, inv, h, w):
    """uint8 [H, W, 3] -> uint8 [h, w, 3]: warpPerspective sampling through the inverse map inv (9 doubles)"""
    H, W, _ = img.shape
    M = [float(m) for m in np.asarray(inv, np.float64).reshape(9)]
    y, x = np.mgrid[0:h, 0:w]
    y = y.astype(np.float64)
    bw0 = block_width(h, w)
    xb = ((x // bw0) * bw0).astype(np.float64)
    x1 = (x - (x // bw0) * bw0).astype(np.float64)
    with np.errstate(all='ignore'):
        X0 = M[0] * xb + M[1] * y + M[2]
        Y0 = M[3] * xb + M[4] * y + M[5]
        W0 = M[6] * xb + M[7] * y + M[8]
        Wd = W0 + M[6] * x1
        Wd = np.where(Wd != 0.0, 32.0 / np.where(Wd != 0.0, Wd, 1.0), 0.0)
        fX = _clamp_int_range((X0 + M[0] * x1) * Wd)
        fY = _clamp_int_range((Y0 + M[3] * x1) * Wd)
    X, Y = np.rint(fX).astype(np.int64), np.rint(fY).astype(np.int64)
    sx, sy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
    fx, fy = X & 31, Y & 31
    wt = [(32 - fy) * (32 - fx) * 32, (32 - fy) * fx * 32, fy * (32 - fx) * 32, fy * fx * 32]
    z = (fx == 0) & (fy == 0)
    wt[0] = np.where(z, 32767, wt[0])
    wt[3] = np.where(z, 1, wt[3])
    acc = np.zeros((h, w, 3), np.int64)
    for k in range(4):
        yy, xx = sy + (k >> 1), sx + (k & 1)
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        px = img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.int64)
        acc += np.where(ok[..., None], px * wt[k][..., None], 0)
    return np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)


def crop(img, quad, h=32, w=100):
    """cv2.warpPerspective(img, cv2.getPerspectiveTransform(quad, dst), (w, h)) of one box"""
    fwd = perspective_map(quad, h, w)
    return warp_perspective(img, invert3(fwd), h, w)
