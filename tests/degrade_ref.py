"""Numpy restatement of the degradation augmentation of csrc/degrade.hip (db_text_minimal_amd/degrade.py):
the Gaussian blur and the additive Gaussian noise of one uint8 [H, W, 3] image, in int64, written from the definition alone and
sharing no code with the package.  tests/test_degrade_cpu.py anchors the blur to scipy.ndimage.gaussian_filter and the generator
to Philox4x32-10's published answers; the device answers to these functions byte for byte (tests/test_degrade_gpu.py).
"""
import math
from statistics import NormalDist

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def radius(sigma):
    return int(4.0 * float(sigma) + 0.5)


def weights(sigma):
    """q_0 .. q_r: the 16-bit fixed-point Gaussian of the definition, summing (two-sided) to exactly 65536"""
    r = radius(sigma)
    if r == 0:
        return [65536]
    w = [math.exp(-(i * i) / (2.0 * float(sigma) * float(sigma))) for i in range(-r, r + 1)]
    total = sum(w)
    q = [int(math.floor(w[r + i] / total * 65536.0 + 0.5)) for i in range(r + 1)]
    q[0] = 65536 - 2 * sum(q[1:])
    return q


def mirror(i, n):
    """scipy's 'mirror' (d c b | a b c d | c b a): an index array folded with period 2 (n - 1)"""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    m = np.mod(i, p)
    return np.where(m >= n, p - m, m)


def blur(img, sigma):
    q = weights(sigma)
    r = len(q) - 1
    if r == 0:
        return img.copy()
    H, W = img.shape[:2]
    p = img.astype(np.int64)
    rows = np.zeros_like(p)
    for i in range(-r, r + 1):
        rows += q[abs(i)] * p[:, mirror(np.arange(W) + i, W)]
    total = np.zeros_like(p)
    for j in range(-r, r + 1):
        total += q[abs(j)] * rows[mirror(np.arange(H) + j, H)]
    return ((total + (1 << 31)) >> 32).astype(np.uint8)


def philox(counter, key):
    """one Philox4x32-10 block: counter (4 words), key (2 words) -> 4 words; words may be equal-shaped uint64 arrays"""
    c = [np.asarray(v, np.uint64) & np.uint64(MASK) for v in counter]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK), (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(MASK)]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


_table = []


def normal_table():
    """Z[4096]: the standard normal's quantiles at (k + 0.5) / 4096 in units of 1 / 4096"""
    if not _table:
        inv = NormalDist().inv_cdf
        _table.append(np.array([int(round(inv((k + 0.5) / 4096.0) * 4096.0)) for k in range(4096)], np.int64))
    return _table[0]


def noise_delta(H, W, scale, seed, per_channel):
    """d of every byte: int64 [H, W, 3]"""
    S8 = int(round(float(scale) * 256.0))
    seed = int(seed)
    g = np.arange(H * W, dtype=np.uint64)
    zero = np.zeros_like(g)
    words = philox((g, zero, zero, zero), (seed & MASK, seed >> 32))
    Z = normal_table()
    d = np.stack([(Z[(words[c if per_channel else 0] >> np.uint64(20)).astype(np.int64)] * S8 + (1 << 19)) >> 20 for c in range(3)], -1)
    return d.reshape(H, W, 3)


def noise(img, scale, seed, per_channel=True):
    H, W = img.shape[:2]
    return np.clip(img.astype(np.int64) + noise_delta(H, W, scale, seed, per_channel), 0, 255).astype(np.uint8)


def degrade(img, plan):
    """blur, then noise on the blurred byte"""
    out = blur(img, plan['sigma'])
    if int(round(float(plan['scale']) * 256.0)) > 0:
        out = noise(out, plan['scale'], plan['seed'], bool(plan['per_channel']))
    return out


def degrade_packed(imgs, plans):
    """what degrade_images returns for these images: the results, flattened and concatenated"""
    return np.concatenate([degrade(im, p).reshape(-1) for im, p in zip(imgs, plans)])
