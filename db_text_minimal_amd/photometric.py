"""Photometric augmentation on the device: torchvision's ColorJitter (brightness, contrast, saturation, hue) as it acts on PIL
images, on the packed uint8 batch the loader passes around (csrc/photometric.hip; definition: DESIGN.md section 37).

  plan_color_jitter(n, rng, brightness, contrast, saturation, hue)   host: per image the drawn order and factors (no pixels)
  color_jitter_images(packed_u8, shapes, plans, out=None)            device: the packed uint8 batch after its plans
  adjust_brightness / adjust_contrast / adjust_saturation / adjust_hue   one [H, W, 3] or [N, H, W, 3] device tensor, one factor

A plan is the ordered list of (name, factor) of one image, names out of OPS, each at most once.  brightness(f) blends the image
with black, contrast(f) with the mean grey of the image as that step meets it, saturation(f) with its grey version (all
Image.blend: f = 0 gives the other image, 1 the image itself, more than 1 extrapolates and clips); hue(h), -0.5 <= h <= 0.5,
converts to HSV as Pillow does, adds trunc(h * 255) to H mod 256 and converts back.  A hue step with h = 0 still makes the
round trip through 8-bit HSV, which is not the identity (up to 7 levels per channel): that is what torchvision does on a PIL
image.  The pixels are Pillow's bit for bit (tests/test_photometric_*.py).  PARITY UNPINNED by construction: the sampling.
torchvision draws from torch's generator; plan_color_jitter draws the same distributions (a uniform random order of the
operations present, one uniform factor each) from a np.random.RandomState.
"""
import numpy as np
import torch

from ._lib import check, lib
from .packed import check_bytes, flat_u8, on_device, upload

OPS = ('brightness', 'contrast', 'saturation', 'hue')
_CODE = {name: k + 1 for k, name in enumerate(OPS)}
_DESC = 8
_CHUNK = 1024  # pixels of one image a workgroup takes per step (PH_CHUNK_PIXELS)
_MAX_IMAGES, _MAX_SIDE = 65535, 16384


# ---- host plan -----------------------------------------------------------------------------------------------------
def _range(name, value, centre, bound, clip_at_zero):
    """torchvision's ColorJitter._check_input: a number v is [centre - v, centre + v] (its low end clipped at 0 for the three
    factors), a pair is itself; None, or a range that holds the centre alone, leaves the operation out -> (low, high) or None"""
    if value is None:
        return None
    if isinstance(value, (int, float, np.integer, np.floating)):
        if value < 0:
            raise ValueError('%s as a single number must not be negative' % name)
        lo, hi = centre - float(value), centre + float(value)
        if clip_at_zero:
            lo = max(lo, 0.0)
    elif isinstance(value, (tuple, list)) and len(value) == 2:
        lo, hi = float(value[0]), float(value[1])
    else:
        raise TypeError('%s is a number or a pair (min, max)' % name)
    if not bound[0] <= lo <= hi <= bound[1]:
        raise ValueError('%s range (%g, %g) is not an ascending pair inside %s' % (name, lo, hi, bound))
    return None if lo == hi == centre else (lo, hi)


def color_jitter_ranges(brightness=None, contrast=None, saturation=None, hue=None):
    """The operations these ColorJitter arguments leave present, in the order of OPS: [(name, (low, high))].  A number b
    means the range [max(0, 1 - b), 1 + b], for hue [-h, h] with 0 <= h <= 0.5; a pair means itself; None or 0 leaves the
    operation out; anything else raises as torchvision does."""
    ranges = [(name, _range(name, value, 1.0, (0.0, float('inf')), True)) for name, value in
              (('brightness', brightness), ('contrast', contrast), ('saturation', saturation))]
    ranges.append(('hue', _range('hue', hue, 0.0, (-0.5, 0.5), False)))
    return [(name, r) for name, r in ranges if r is not None]


def plan_color_jitter(n, rng, brightness=None, contrast=None, saturation=None, hue=None):
    """Plans for n images as torchvision's ColorJitter draws them: per image a uniform random permutation of the operations
    present (one rng.permutation), then one rng.uniform per factor in the order of OPS (color_jitter_ranges reads the
    arguments).  `rng` is a np.random.RandomState; torch's own stream is not reproduced."""
    present = color_jitter_ranges(brightness, contrast, saturation, hue)
    plans = []
    for _ in range(int(n)):
        if not present:
            plans.append([])
            continue
        order = rng.permutation(len(present))
        factors = [float(rng.uniform(lo, hi)) for _, (lo, hi) in present]
        plans.append([(present[k][0], factors[k]) for k in order])
    return plans


def hue_shift(h):
    """the value added to H mod 256: trunc(h * 255) mod 256"""
    return int(h * 255) % 256


def plan_records(shapes, plans):
    """The records of dbn_color_jitter_u8 for packed images (include/dbnet_hip.h): int64 [N, 8]."""
    N = len(shapes)
    if not 1 <= N <= _MAX_IMAGES:
        raise ValueError('%d images: a batch holds 1 .. %d' % (N, _MAX_IMAGES))
    if len(plans) != N:
        raise ValueError('%d plans for %d images: one plan per image' % (len(plans), N))
    desc = np.zeros((N, _DESC), np.int64)
    off = chunk = 0
    for n, ((H, W), plan) in enumerate(zip(shapes, plans)):
        H, W = int(H), int(W)
        if not (1 <= H <= _MAX_SIDE and 1 <= W <= _MAX_SIDE):
            raise ValueError('image size %d x %d outside 1 .. %d' % (H, W, _MAX_SIDE))
        names = [name for name, _ in plan]
        if len(set(names)) != len(names) or any(name not in _CODE for name in names):
            raise ValueError('plan %d: operations out of %s, each at most once, not %s' % (n, OPS, names))
        ops, vals = len(plan), [0, 0, 0, 0]
        for k, (name, f) in enumerate(plan):
            f = float(f)
            ops |= _CODE[name] << (4 * (k + 1))
            if name == 'hue':
                if not -0.5 <= f <= 0.5:
                    raise ValueError('plan %d: hue factor %g outside [-0.5, 0.5]' % (n, f))
                vals[k] = hue_shift(f)
            else:
                if not (0 <= f and np.isfinite(np.float32(f))):
                    raise ValueError('plan %d: %s factor %g is negative or not finite' % (n, name, f))
                vals[k] = int(np.float32(f).view(np.uint32))
        f01, f23 = (np.uint64(lo | hi << 32).astype(np.int64) for lo, hi in (vals[:2], vals[2:]))
        desc[n, :7] = off, H, W, chunk, ops, f01, f23
        off += 3 * H * W
        chunk += (H * W + _CHUNK - 1) // _CHUNK
    return desc


# ---- device --------------------------------------------------------------------------------------------------------
def color_jitter_images(packed_u8, shapes, plans, out=None):
    """Packed uint8 RGB images on the device (image_collate's layout: [H, W, 3] each, end to end) -> the packed uint8 tensor
    after each image's plan.  Two launches for the whole batch on the current stream (one when no plan holds contrast), no
    host sync.  The input is left as it is unless `out` is the input; out=None allocates; an `out` that overlaps the input
    without being it is refused."""
    shapes = [(int(h), int(w)) for h, w in shapes]
    desc = plan_records(shapes, plans)
    src = flat_u8(packed_u8, what='packed_u8')
    need = int(sum(3 * h * w for h, w in shapes))
    check_bytes(src.numel(), need, 'packed_u8 holds')
    dst = torch.empty_like(src) if out is None else flat_u8(out, what='out')
    if dst.numel() != need or dst.device != src.device:
        raise ValueError('out must hold %d bytes on %s' % (need, src.device))
    a, b = src.data_ptr(), dst.data_ptr()
    if a != b and a < b + need and b < a + need:  # a shifted view of the input: lanes would read what others have written
        raise ValueError('out must be the input itself or must not overlap it')
    N, dev = len(shapes), src.device
    with on_device(dev) as stream:
        contrast = any(name == 'contrast' for plan in plans for name, _ in plan)
        sums = torch.empty(N, dtype=torch.int64, device=dev) if contrast else None
        d = upload(desc, dev)
        check(lib().dbn_color_jitter_u8(src.data_ptr(), dst.data_ptr(), need, desc.ctypes.data, d.data_ptr(), N,
                                        sums.data_ptr() if contrast else None, stream), 'color_jitter_u8')
    return dst


def _adjust(img, name, factor):
    if not (isinstance(img, torch.Tensor) and img.is_cuda and img.dtype == torch.uint8 and img.dim() in (3, 4) and img.shape[-1] == 3):
        raise ValueError('adjust_%s takes a uint8 [H, W, 3] or [N, H, W, 3] tensor on a GPU device' % name)
    n = 1 if img.dim() == 3 else int(img.shape[0])
    H, W = int(img.shape[-3]), int(img.shape[-2])
    out = color_jitter_images(img.contiguous().reshape(-1), [(H, W)] * n, [[(name, factor)]] * n)
    return out.reshape(img.shape)


def adjust_brightness(img, factor):
    """ImageEnhance.Brightness(img).enhance(factor) of every image: 0 black, 1 the image, 2 twice as bright (clipped)"""
    return _adjust(img, 'brightness', factor)


def adjust_contrast(img, factor):
    """ImageEnhance.Contrast(img).enhance(factor) of every image: 0 the mean grey of that image, 1 the image"""
    return _adjust(img, 'contrast', factor)


def adjust_saturation(img, factor):
    """ImageEnhance.Color(img).enhance(factor) of every image: 0 its grey version, 1 the image"""
    return _adjust(img, 'saturation', factor)


def adjust_hue(img, factor):
    """torchvision's adjust_hue of a PIL image: H of Pillow's HSV moved by trunc(factor * 255) mod 256, -0.5 <= factor <= 0.5.
    factor = 0 still makes the 8-bit round trip, which changes a channel by up to 7 levels."""
    return _adjust(img, 'hue', factor)
