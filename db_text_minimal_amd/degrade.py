"""Degradation augmentation on the device: Gaussian blur (focus softness) and additive Gaussian noise (sensor noise), the two
augmenters a scene-text loader adds first (imgaug's GaussianBlur and AdditiveGaussianNoise), on the packed uint8 batch the loader
passes around (csrc/degrade.hip; definition: DESIGN.md section 40).

  plan_degrade(n, rng, blur, blur_p, noise, noise_p, per_channel)   host: per image the drawn sigma, scale, flag and seed (no pixels)
  degrade_records(shapes, plans)                                    host: the records and the tile list of dbn_degrade_u8
  degrade_images(packed_u8, shapes, plans, out=None)                device: the packed uint8 batch after its plans
  gaussian_blur(img, sigma) / gaussian_noise(img, scale, seed)      one [H, W, 3] or [N, H, W, 3] device tensor

Everything is exact integer arithmetic.  Blur(sigma), 0 <= sigma <= 8: radius r = int(4 sigma + 0.5) (scipy's truncate = 4), the
normalised Gaussian quantised to 16 fractional bits with the centre weight taking the rounding (blur_weights: the weights sum to
2^16), the border mirrored without repeating the edge pixel (scipy 'mirror', cv2 REFLECT_101), the 2-D sum of 32 fractional bits
rounded half up once.  Noise(scale, seed, per_channel), 0 <= scale <= 64 grey levels: per pixel one Philox4x32-10 block (counter =
the pixel's row-major index, key = the seed), per channel the top 12 bits of a word index a 4096-entry table of normal quantiles
(NORMAL_TABLE), and the byte moves by floor((Z S8 + 2^19) / 2^20) with S8 = round(256 scale), clamped to 0 .. 255.  Blur comes
first, noise acts on the blurred byte; both in one launch.  PARITY UNPINNED by construction: imgaug's and cv2's own roundings and
random streams (neither library is a dependency); the blur is anchored to scipy.ndimage.gaussian_filter within one level
(tests/test_degrade_cpu.py).
"""
import math
from statistics import NormalDist

import numpy as np
import torch

from ._lib import check, lib
from .packed import check_bytes, flat_u8, on_device, upload

MAX_SIGMA, MAX_SCALE, MAX_RADIUS = 8.0, 64.0, 32
TILE_W, TILE_H, RUN = 64, 32, 3072 # a stencil tile in pixels; the pixels of a run, the tile of an image without blur (DG_*)
_DESC = 25
_MAX_IMAGES, _MAX_SIDE = 65535, 16384

_inv = NormalDist().inv_cdf
NORMAL_TABLE = np.array([int(round(_inv((k + 0.5) / 4096.0) * 4096.0)) for k in range(4096)], np.int16)
NORMAL_TABLE.setflags(write=False)


# ---- host plan -----------------------------------------------------------------------------------------------------
def blur_radius(sigma):
    return int(4.0 * float(sigma) + 0.5)


def blur_weights(sigma):
    """q_0 .. q_r of a blur by sigma: exp(-i^2 / 2 sigma^2) over |i| <= r, normalised in float64, times 65536 and rounded half up
    for i != 0; q_0 = 65536 - 2 sum(q_i, i > 0).  r = 0 (sigma < 0.125) gives [65536], the identity."""
    sigma = float(sigma)
    if not 0 <= sigma <= MAX_SIGMA:
        raise ValueError('sigma %g outside [0, %g]' % (sigma, MAX_SIGMA))
    r = blur_radius(sigma)
    if r == 0:
        return [65536]
    w = [math.exp(-(i * i) / (2.0 * sigma * sigma)) for i in range(-r, r + 1)]
    total = sum(w)
    q = [int(math.floor(w[r + i] / total * 65536.0 + 0.5)) for i in range(r + 1)]
    q[0] = 65536 - 2 * sum(q[1:])
    return q


def noise_scale8(scale):
    """S8 = round(256 scale)"""
    return int(np.rint(float(scale) * 256.0))


def _range(name, value, top):
    """a number v is the range (0, v), a pair is itself; None or 0 leaves the operation out -> (low, high) or None"""
    if value is None:
        return None
    if isinstance(value, (int, float, np.integer, np.floating)):
        lo, hi = 0.0, float(value)
    elif isinstance(value, (tuple, list)) and len(value) == 2:
        lo, hi = float(value[0]), float(value[1])
    else:
        raise TypeError('%s is a number or a pair (min, max)' % name)
    if not 0 <= lo <= hi <= top:
        raise ValueError('%s range (%g, %g) is not an ascending pair inside [0, %g]' % (name, lo, hi, top))
    return None if hi == 0 else (lo, hi)


def _probability(name, p):
    p = float(p)
    if not 0 <= p <= 1:
        raise ValueError('%s %g is not a probability' % (name, p))
    return p


def degrade_ranges(blur=None, blur_p=0.5, noise=None, noise_p=0.5, per_channel=0.5):
    """The ranges these arguments leave present: {'blur': (low, high), 'noise': (low, high)} without the operations left out.
    Raises on a range outside 0 .. MAX_SIGMA / 0 .. MAX_SCALE and on a probability outside 0 .. 1."""
    for name, p in (('blur_p', blur_p), ('noise_p', noise_p), ('per_channel', per_channel)):
        _probability(name, p)
    ranges = {'blur': _range('blur', blur, MAX_SIGMA), 'noise': _range('noise', noise, MAX_SCALE)}
    return {k: v for k, v in ranges.items() if v is not None}


def plan_degrade(n, rng, blur=None, blur_p=0.5, noise=None, noise_p=0.5, per_channel=0.5):
    """Plans for n images: {'sigma', 'scale', 'per_channel', 'seed'} each.  Per image seven draws are always made from `rng` (a
    np.random.RandomState), in this order: uniform() against blur_p, uniform(lo, hi) for sigma, uniform() against noise_p,
    uniform(lo, hi) for the scale, uniform() against per_channel, and two randint(0, 2**32, dtype=uint32) for the low and the high
    word of the seed — so an image's plan does not depend on what another image drew.  An operation that is absent (degrade_ranges)
    draws from (0, 0); one left out by its probability gets sigma = 0 or scale = 0."""
    present = degrade_ranges(blur, blur_p, noise, noise_p, per_channel)
    b, s = present.get('blur', (0.0, 0.0)), present.get('noise', (0.0, 0.0))
    plans = []
    for _ in range(int(n)):
        u_blur, sigma = rng.uniform(), float(rng.uniform(b[0], b[1]))
        u_noise, scale = rng.uniform(), float(rng.uniform(s[0], s[1]))
        u_channel = rng.uniform()
        low, high = int(rng.randint(0, 2**32, dtype=np.uint32)), int(rng.randint(0, 2**32, dtype=np.uint32))
        plans.append({'sigma': sigma if 'blur' in present and u_blur < blur_p else 0.0,
                      'scale': scale if 'noise' in present and u_noise < noise_p else 0.0,
                      'per_channel': bool(u_channel < per_channel), 'seed': low | high << 32})
    return plans


def degrade_records(shapes, plans):
    """The records and the tile list of dbn_degrade_u8 for packed images (include/dbnet_hip.h): (int64 [N, 25], int32 [T, 3]).
    A tile is (image, y0, x0), TILE_H x TILE_W pixels of an image that is blurred (cut at the image's edges), or (image, first
    pixel, 0), a run of RUN pixels in row-major order of an image that is not; every pixel of every image lies in exactly one."""
    N = len(shapes)
    if not 1 <= N <= _MAX_IMAGES:
        raise ValueError('%d images: a batch holds 1 .. %d' % (N, _MAX_IMAGES))
    if len(plans) != N:
        raise ValueError('%d plans for %d images: one plan per image' % (len(plans), N))
    desc = np.zeros((N, _DESC), np.int64)
    taps = desc[:, 8:].view(np.uint32)  # q_0 .. q_32, two to an int64
    tiles = []
    off = tile = 0
    for n, ((H, W), plan) in enumerate(zip(shapes, plans)):
        H, W = int(H), int(W)
        if not (1 <= H <= _MAX_SIDE and 1 <= W <= _MAX_SIDE):
            raise ValueError('image size %d x %d outside 1 .. %d' % (H, W, _MAX_SIDE))
        sigma, scale, seed = float(plan['sigma']), float(plan['scale']), int(plan['seed'])
        if not 0 <= sigma <= MAX_SIGMA:
            raise ValueError('plan %d: sigma %g outside [0, %g]' % (n, sigma, MAX_SIGMA))
        if not 0 <= scale <= MAX_SCALE:
            raise ValueError('plan %d: noise scale %g outside [0, %g]' % (n, scale, MAX_SCALE))
        if not 0 <= seed < 1 << 64:
            raise ValueError('plan %d: the seed is a 64-bit number, not %d' % (n, seed))
        q = blur_weights(sigma)
        r = len(q) - 1 if q[0] < 65536 else 0  # (neighbour weights that all round to 0: the identity, as r = 0 is)
        if r:
            taps[n, :r + 1] = q
        desc[n, :7] = (off, H, W, tile, r, noise_scale8(scale) | int(bool(plan['per_channel'])) << 32,
                       np.uint64(seed).astype(np.int64))
        if r:
            ty, tx = np.meshgrid(np.arange(0, H, TILE_H, dtype=np.int32), np.arange(0, W, TILE_W, dtype=np.int32), indexing='ij')
            t = np.stack([np.full(ty.size, n, np.int32), ty.reshape(-1), tx.reshape(-1)], 1)
        else:
            first = np.arange(0, H * W, RUN, dtype=np.int32)
            t = np.stack([np.full(first.size, n, np.int32), first, np.zeros(first.size, np.int32)], 1)
        tiles.append(t)
        off += 3 * H * W
        tile += len(t)
    return desc, np.concatenate(tiles)


# ---- device --------------------------------------------------------------------------------------------------------
_tables = {}


def _normal_table(dev):
    if dev not in _tables:
        _tables[dev] = torch.from_numpy(NORMAL_TABLE.copy()).to(dev)
    return _tables[dev]


def degrade_images(packed_u8, shapes, plans, out=None):
    """Packed uint8 RGB images on the device (image_collate's layout: [H, W, 3] each, end to end) -> the packed uint8 tensor after
    each image's plan ({'sigma', 'scale', 'per_channel', 'seed'}: plan_degrade).  One launch for the whole batch on the current
    stream, whatever the plans hold, no host sync.  The input is left as it is; out=None allocates; an `out` that overlaps the
    input, the input itself included, is refused: a stencil cannot run in place."""
    shapes = [(int(h), int(w)) for h, w in shapes]
    desc, tiles = degrade_records(shapes, plans)
    src = flat_u8(packed_u8, what='packed_u8')
    need = int(sum(3 * h * w for h, w in shapes))
    check_bytes(src.numel(), need, 'packed_u8 holds')
    dst = torch.empty_like(src) if out is None else flat_u8(out, what='out')
    if dst.numel() != need or dst.device != src.device:
        raise ValueError('out must hold %d bytes on %s' % (need, src.device))
    a, b = src.data_ptr(), dst.data_ptr()
    if a < b + need and b < a + need:
        raise ValueError('out must not overlap the input (a blur cannot run in place)')
    dev = src.device
    with on_device(dev) as stream:
        table = _normal_table(dev)
        d, t = upload(desc, dev), upload(tiles, dev)
        check(lib().dbn_degrade_u8(src.data_ptr(), dst.data_ptr(), need, desc.ctypes.data, d.data_ptr(), len(shapes),
                                   tiles.ctypes.data, t.data_ptr(), len(tiles), table.data_ptr(), stream), 'degrade_u8')
    return dst


def _single(img, who, plan):
    if not (isinstance(img, torch.Tensor) and img.is_cuda and img.dtype == torch.uint8 and img.dim() in (3, 4) and img.shape[-1] == 3):
        raise ValueError('%s takes a uint8 [H, W, 3] or [N, H, W, 3] tensor on a GPU device' % who)
    n = 1 if img.dim() == 3 else int(img.shape[0])
    H, W = int(img.shape[-3]), int(img.shape[-2])
    return degrade_images(img.contiguous().reshape(-1), [(H, W)] * n, [plan] * n).reshape(img.shape)


def gaussian_blur(img, sigma):
    """every image blurred by sigma (0 <= sigma <= 8; below 0.125 the image itself)"""
    return _single(img, 'gaussian_blur', {'sigma': sigma, 'scale': 0.0, 'per_channel': False, 'seed': 0})


def gaussian_noise(img, scale, seed, per_channel=True):
    """Gaussian noise of `scale` grey levels (0 .. 64) added to every image and clamped; per_channel=False moves the three channels of
    a pixel by the same amount.  The noise field depends on the seed and the pixel's place alone: images of one call get the same."""
    return _single(img, 'gaussian_noise', {'sigma': 0.0, 'scale': scale, 'per_channel': per_channel, 'seed': seed})
