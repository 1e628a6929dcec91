"""Numpy restatement of the photometric augmentation of csrc/photometric.hip (db_text_minimal_amd/photometric.py, DESIGN.md
section 37): torchvision's ColorJitter as it acts on a PIL image, that is Pillow's ImageEnhance.Brightness / Contrast / Color
(Image.blend against black, the mean grey, the grey image) and the HSV round trip of torchvision's adjust_hue.  Every function
here answers to Pillow alone (tests/test_photometric_cpu.py compares them byte for byte); the device answers to these.

Images are uint8 [H, W, 3] RGB.  A plan is the ordered list of (name, factor) of one image, names out of OPS.
"""
import numpy as np

OPS = ('brightness', 'contrast', 'saturation', 'hue')


def blend(d, x, f):
    """Pillow's Image.blend(d, x, f) per channel: t = float32(d) + float32(f) * float32(x - d), a float32 multiply and a
    float32 add, clipped to [0, 255] and truncated toward zero (for 0 <= f <= 1 the clip does nothing, as in Pillow)."""
    d = np.asarray(d)
    x = np.asarray(x)
    a = np.float32(f)
    diff = (x.astype(np.int32) - d.astype(np.int32)).astype(np.float32)
    t = d.astype(np.float32) + (a * diff).astype(np.float32)
    return np.clip(t, np.float32(0), np.float32(255)).astype(np.uint8)


def luma(rgb):
    """convert('L'): (19595 r + 38470 g + 7471 b + 32768) >> 16"""
    v = rgb.astype(np.int64)
    return ((19595 * v[..., 0] + 38470 * v[..., 1] + 7471 * v[..., 2] + 32768) >> 16).astype(np.uint8)


def grey_mean(rgb):
    """int(ImageStat.Stat(img.convert('L')).mean[0] + 0.5): an exact integer sum, the division and the + 0.5 in float64"""
    L = luma(rgb)
    return int(float(int(L.astype(np.int64).sum())) / float(L.size) + 0.5)


def _round_half_away(x):
    """C's round() of non-negative float64 values (x - trunc(x) is exact)"""
    r = np.trunc(x)
    return r + (x - r >= 0.5)


def rgb_to_hsv(rgb):
    """convert('HSV') of Pillow (Convert.c rgb2hsv_row): float32 variables, float64 where a double constant takes part"""
    v = rgb.astype(np.int32)
    r, g, b = v[..., 0], v[..., 1], v[..., 2]
    maxc = np.maximum(r, np.maximum(g, b))
    minc = np.minimum(r, np.minimum(g, b))
    grey = maxc == minc
    f32, f64 = np.float32, np.float64
    cr = np.where(grey, 1, maxc - minc).astype(f32)
    sat = cr / np.where(grey, 1, maxc).astype(f32)
    rc = (maxc - r).astype(f32) / cr
    gc = (maxc - g).astype(f32) / cr
    bc = (maxc - b).astype(f32) / cr
    h = np.where(r == maxc, bc - gc,
                 np.where(g == maxc, (2.0 + rc.astype(f64) - bc.astype(f64)).astype(f32),
                          (4.0 + gc.astype(f64) - rc.astype(f64)).astype(f32))).astype(f32)
    h = np.fmod(h.astype(f64) / 6.0 + 1.0, 1.0).astype(f32)
    H = np.clip((h.astype(f64) * 255.0).astype(np.int32), 0, 255)
    S = np.clip((sat.astype(f64) * 255.0).astype(np.int32), 0, 255)
    H = np.where(grey, 0, H)
    S = np.where(grey, 0, S)
    return np.stack([H, S, maxc], -1).astype(np.uint8)


def hsv_to_rgb(hsv):
    """HSV -> RGB of Pillow (Convert.c hsv2rgb): f and fs are float32 variables, fs * f a float32 product, the rest float64"""
    f32, f64 = np.float32, np.float64
    H, S, V = (hsv[..., k].astype(np.int32) for k in range(3))
    hf = H.astype(f64) * 6.0 / 255.0
    i = np.floor(hf)
    f = (hf - i).astype(f32)
    fs = (S.astype(f64) / 255.0).astype(f32)
    Vd = V.astype(f64)
    p = _round_half_away(Vd * (1.0 - fs.astype(f64)))
    q = _round_half_away(Vd * (1.0 - (fs * f).astype(f32).astype(f64)))
    t = _round_half_away(Vd * (1.0 - fs.astype(f64) * (1.0 - f.astype(f64))))
    p, q, t = (np.clip(a, 0, 255).astype(np.int32) for a in (p, q, t))
    k = i.astype(np.int32) % 6
    table = (((V, t, p), (q, V, p), (p, V, t), (p, q, V), (t, p, V), (V, p, q)))
    out = np.empty(hsv.shape, np.uint8)
    for c in range(3):
        out[..., c] = np.where(S == 0, V, np.choose(k, [table[j][c] for j in range(6)]))
    return out


def hue_shift(h):
    """the uint8 that torchvision adds to the H plane: trunc(h * 255) mod 256"""
    return int(h * 255) % 256  # int() truncates toward zero


def brightness(img, f):
    return blend(np.zeros_like(img), img, f)


def saturation(img, f):
    return blend(luma(img)[..., None], img, f)


def contrast(img, f):
    return blend(np.full_like(img, grey_mean(img)), img, f)


def hue(img, h):
    """RGB -> HSV, H + shift mod 256, HSV -> RGB.  A shift of 0 still makes the round trip, which is not the identity."""
    hsv = rgb_to_hsv(img)
    hsv[..., 0] = ((hsv[..., 0].astype(np.int32) + hue_shift(h)) & 255).astype(np.uint8)
    return hsv_to_rgb(hsv)


_APPLY = {'brightness': brightness, 'contrast': contrast, 'saturation': saturation, 'hue': hue}


def apply_plan(img, plan):
    """one image through its plan, in order"""
    out = np.ascontiguousarray(img, dtype=np.uint8)
    for name, factor in plan:
        out = _APPLY[name](out, factor)
    return out


def jitter_packed(images, plans):
    """what color_jitter_images returns for these images: the results, flattened and concatenated"""
    return np.concatenate([apply_plan(im, p).reshape(-1) for im, p in zip(images, plans)])
