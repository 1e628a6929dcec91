"""numpy restatement of the three device stages of db_text_minimal_amd.augment (csrc/resample.hip), written as the
kernels compute: the yardstick of tests/test_augment_gpu.py.  OpenCV 4.2's scalar 8-bit paths:
  warp_affine     cv2.warpAffine INTER_LINEAR, BORDER_CONSTANT 0 (WarpAffineInvoker + remapBilinear), the flip folded in
  resize_cubic    cv2.resize INTER_CUBIC (HResizeCubic + VResizeCubic, FixedPtCast 22), a window of the output
  resize_linear   cv2.resize INTER_LINEAR (HResizeLinear + the uchar VResizeLinear), then the normalisation / padding
Float formulas run in np.float32 (IEEE, no FMA), double ones in Python floats; rounding is cvRound (half to even)."""
import numpy as np

from db_text_minimal_amd import augment as A
from db_text_minimal_amd.gt_maps import MEAN


def _rint_i(v):
    return np.rint(v).astype(np.int64)


def _sat_short(v):
    return np.clip(_rint_i(v), -32768, 32767)


def resize_src(d, scale):
    """fx = (float)((dx + 0.5) * scale - 0.5), sx = floor(fx), fx -= sx"""
    f = (np.asarray(d, np.float64) + 0.5) * scale - 0.5
    f = f.astype(np.float32)
    s = np.floor(f).astype(np.int64)
    return s, (f - s.astype(np.float32)).astype(np.float32)


def cubic_coeffs(x):
    x = np.asarray(x, np.float32)
    A_ = np.float32(-0.75)
    one, five, eight, four, two, three = (np.float32(v) for v in (1, 5, 8, 4, 2, 3))
    k0 = ((A_ * (x + one) - five * A_) * (x + one) + eight * A_) * (x + one) - four * A_
    k1 = ((A_ + two) * x - (A_ + three)) * x * x + one
    k2 = ((A_ + two) * (one - x) - (A_ + three)) * (one - x) * (one - x) + one
    k3 = one - k0 - k1 - k2
    return np.stack([_sat_short(k * np.float32(2048)) for k in (k0, k1, k2, k3)], -1)


def warp_affine(img, M_inv, flip):
    """uint8 [H, W, 3] -> uint8 [H, W, 3]: warpAffine of (flip ? img[:, ::-1] : img) by the inverse map M_inv[6]"""
    H, W, _ = img.shape
    src = img[:, ::-1] if flip else img
    M = [float(v) for v in M_inv]
    xs, ys = np.arange(W), np.arange(H)
    ad = np.array([int(np.rint(M[0] * x * 1024)) for x in xs], np.int64)
    bd = np.array([int(np.rint(M[3] * x * 1024)) for x in xs], np.int64)
    x0 = np.array([int(np.rint((M[1] * y + M[2]) * 1024)) for y in ys], np.int64) + 16
    y0 = np.array([int(np.rint((M[4] * y + M[5]) * 1024)) for y in ys], np.int64) + 16
    X = (x0[:, None] + ad[None, :]) >> 5
    Y = (y0[:, None] + bd[None, :]) >> 5
    sx, sy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
    fx, fy = X & 31, Y & 31
    w = [(32 - fy) * (32 - fx) * 32, (32 - fy) * fx * 32, fy * (32 - fx) * 32, fy * fx * 32]
    z = (fx == 0) & (fy == 0)
    w[0] = np.where(z, 32767, w[0])
    w[3] = np.where(z, 1, w[3])
    acc = np.zeros((H, W, 3), np.int64)
    for k in range(4):
        yy, xx = sy + (k >> 1), sx + (k & 1)
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        v = src[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.int64)
        acc += np.where(ok[..., None], v * w[k][..., None], 0)
    return np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)


def resize_cubic(img, dh, dw, window=None):
    """uint8 [H, W, 3] -> the window (y0, y1, x0, x1) of cv2.resize(img, (dw, dh), INTER_CUBIC)"""
    H, W, _ = img.shape
    y0, y1, x0, x1 = window if window is not None else (0, dh, 0, dw)
    sx, fx = resize_src(np.arange(x0, x1), A._resize_coef(W, dw))
    sy, fy = resize_src(np.arange(y0, y1), A._resize_coef(H, dh))
    ca, rb = cubic_coeffs(fx), cubic_coeffs(fy)
    im = img.astype(np.int64)
    rows = np.zeros((H, x1 - x0, 3), np.int64)
    for k in range(4):
        rows += im[:, np.clip(sx - 1 + k, 0, W - 1)] * ca[None, :, k, None]
    acc = np.zeros((y1 - y0, x1 - x0, 3), np.int64)
    for k in range(4):
        acc += rows[np.clip(sy - 1 + k, 0, H - 1)] * rb[:, k, None, None]
    return np.clip((acc + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def resize_linear_u8(img, dh, dw):
    """cv2.resize(img, (dw, dh), INTER_LINEAR) of uint8 [H, W, 3]"""
    H, W, _ = img.shape
    sx, fx = resize_src(np.arange(dw), A._resize_coef(W, dw))
    lo, hi = sx < 0, sx >= W - 1
    fx = np.where(lo | hi, np.float32(0), fx).astype(np.float32)
    sx = np.where(lo, 0, np.where(hi, W - 1, sx))
    a0, a1 = _sat_short((np.float32(1) - fx) * np.float32(2048)), _sat_short(fx * np.float32(2048))
    sy, fy = resize_src(np.arange(dh), A._resize_coef(H, dh))
    b0, b1 = _sat_short((np.float32(1) - fy) * np.float32(2048)), _sat_short(fy * np.float32(2048))
    im = img.astype(np.int64)
    rows = im[:, sx] * a0[None, :, None] + im[:, np.minimum(sx + 1, W - 1)] * a1[None, :, None]
    h0, h1 = rows[np.clip(sy, 0, H - 1)], rows[np.clip(sy + 1, 0, H - 1)]
    v = (((b0[:, None, None] * (h0 >> 4)) >> 16) + ((b1[:, None, None] * (h1 >> 4)) >> 16) + 2) >> 2
    return (v & 255).astype(np.uint8)


def letterbox_norm(img, dh, dw, CH, CW, mean=MEAN):
    """resize_linear_u8 into the top-left corner of a CH x CW canvas, normalised: fp32 [3, CH, CW]"""
    m = np.array([np.float32(v) for v in mean], np.float32)
    out = np.empty((3, CH, CW), np.float32)
    out[:] = (np.float32(0) - m)[:, None, None]
    u = resize_linear_u8(img, dh, dw)
    out[:, :dh, :dw] = u.transpose(2, 0, 1).astype(np.float32) - m[:, None, None]
    return out


def augment_one(img, plan, size=640, mean=MEAN):
    """one image through the plan of augment.plan_augment / plan_letterbox: fp32 [3, size, size]"""
    nh, nw = plan['out_hw']
    if plan['M'] is None:
        return letterbox_norm(img, nh, nw, size, size, mean)
    w = warp_affine(img, A.invert_affine(plan['M']), plan['flip'])
    h2, w2 = plan['scaled_hw']
    c = resize_cubic(w, h2, w2, plan['window'])
    return letterbox_norm(c, nh, nw, size, size, mean)
