"""The geometric stage of the reference's loader on the device: training augmentation (imgaug Fliplr(0.5),
Affine(rotate=(-10, 10)), Resize((0.5, 3.0)) cubic, then db_transforms.crop), the letterbox db_transforms.resize to
size x size, and the inference resize of utils.test_preprocess — each fused with the normalisation of
data_loaders.py:161-167, so a DataLoader ships decoded uint8 images of any size plus their polygons.

  image_collate(items)                       collate_fn: packed pinned uint8 + shapes + polygons + tags
  plan_augment(shapes, polys, rng, size)     host: per image the drawn parameters, the crop window, the letterbox and
                                             the moved polygons (no pixels)
  plan_letterbox(shapes, polys, size)        host: the evaluation plan (letterbox only)
  augment_images(packed, shapes, plans)      device: fp32 [N, 3, S, S], normalised; plans=None is the letterbox
  preprocess_image(u8, size, pad)            device: utils.test_preprocess of one image
  DeviceBatches(loader, device, training)    raw batches -> the dicts fit / evaluate consume (img + GT maps); with
                                             color_jitter the photometric stage (photometric.py) runs in front,
                                             with degrade the blur and noise stage (degrade.py) behind it

Device stages (csrc/resample.hip), one launch each per batch on the current stream, no host sync: warp (flip + rotate,
cv2.warpAffine INTER_LINEAR) -> cubic resize of the crop window only (cv2.resize INTER_CUBIC) -> linear letterbox resize
fused with the normalisation (cv2.resize INTER_LINEAR; the padding is 0 - mean[c], as the reference pads in uint8 and
normalises after).  The evaluation and inference paths run the last stage alone.

Polygon geometry uses one map for the image and its polygons, in the pixel-centre convention of fillPoly: flip
x -> W-1-x; rotation by `angle` about ((W-1)/2, (H-1)/2), output the size of the input; scale to
(h2, w2) = (max(1, int(round(H*scale))), max(1, int(round(W*scale)))) with x *= w2/W, y *= h2/H; every vertex clamped to
[0, w2-1] x [0, h2-1] (db_transforms.transform).  The crop and the letterbox restate db_transforms.crop / resize exactly
(the same legacy RandomState calls in the same order, the same numpy arithmetic): pinned by a golden made with the
reference's own functions.  PARITY UNPINNED: imgaug's random stream is not reproduced (same distributions), nor its keypoint
conventions (flip as W - x, a rotation centre half a pixel away, float32 keypoints, its rounding of the new size), and the
pixel arithmetic restates OpenCV 4.2's scalar 8-bit paths, which its SIMD loops and IPP can round differently.
"""
import math

import numpy as np
import torch

from ._lib import check, lib
from .degrade import degrade_images, degrade_ranges, plan_degrade
from .gt_maps import GT_KEYS, MEAN, make_gt_maps, plan_polygons
from .jpeg import JpegCoefficients, JpegStreams, decode_coefficients, entropy_decode_device, stream_orientations
from .packed import MAX_SIDE, check_shape, cuda_device, image_offsets, on_device, packed_on, pin_default, polys_tags, upload
from .packed import offsets as _offsets
from .photometric import color_jitter_images, color_jitter_ranges, plan_color_jitter
from .png import PngScanlines, unfilter_png

ROTATE = (-10.0, 10.0)  # data_loaders.py:62-66
SCALE = (0.5, 3.0)
_DESC, _COEF = 12, 6


# ---- host plan -----------------------------------------------------------------------------------------------------
def rotation_matrix(angle, H, W):
    """forward 2 x 3 map (fp64) of a rotation by `angle` degrees about ((W-1)/2, (H-1)/2): dst = M @ (x, y, 1)"""
    r = math.radians(angle)
    c, s = math.cos(r), math.sin(r)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    return np.array([[c, -s, cx - c * cx + s * cy], [s, c, cy - s * cx - c * cy]], np.float64)


def invert_affine(M):
    """cv2.warpAffine's inverse of the forward matrix (imgwarp.cpp, fp64, OpenCV's operation order) -> 6 doubles"""
    M = [float(v) for v in np.asarray(M, np.float64).reshape(6)]
    D = M[0] * M[4] - M[1] * M[3]
    D = 1. / D if D != 0 else 0.
    A11, A22 = M[4] * D, M[0] * D
    M[0] = A11
    M[1] *= -D
    M[3] *= -D
    M[4] = A22
    b1 = -M[0] * M[2] - M[1] * M[5]
    b2 = -M[3] * M[2] - M[4] * M[5]
    M[2], M[5] = b1, b2
    return M


def _split_regions(axis):
    regions = []
    min_axis_index = 0
    for i in range(1, axis.shape[0]):
        if axis[i] != axis[i - 1] + 1:
            regions.append(axis[min_axis_index:i])
            min_axis_index = i
    return regions


def _random_select(axis, rng):
    xx = rng.choice(axis, size=2)
    return np.min(xx), np.max(xx)


def _region_wise_random_select(regions, rng):
    selected_index = list(rng.choice(len(regions), 2))
    selected_values = []
    for index in selected_index:
        axis = regions[index]
        selected_values.append(int(rng.choice(axis, size=1)[0]))
    return min(selected_values), max(selected_values)


def crop_window(h, w, polys, rng, max_tries=10, min_crop_side_ratio=0.1):
    """db_transforms.crop (:132-182) on an h x w image with `rng` in place of np.random: -> (window (ymin, ymax, xmin,
    xmax) or None for the whole image, cropped polygons (fp64), indices of the polygons kept)."""
    h_array = np.zeros(h, dtype=np.int32)
    w_array = np.zeros(w, dtype=np.int32)
    for poly in polys:
        points = np.round(poly, decimals=0).astype(np.int32)
        minx, maxx = np.min(points[:, 0]), np.max(points[:, 0])
        w_array[minx:maxx] = 1
        miny, maxy = np.min(points[:, 1]), np.max(points[:, 1])
        h_array[miny:maxy] = 1
    h_axis = np.where(h_array == 0)[0]
    w_axis = np.where(w_array == 0)[0]
    whole = (None, [np.array(p, np.float64) for p in polys], list(range(len(polys))))
    if len(h_axis) == 0 or len(w_axis) == 0:
        return whole
    h_regions = _split_regions(h_axis)
    w_regions = _split_regions(w_axis)
    for _ in range(max_tries):
        if len(w_regions) > 1:
            xmin, xmax = _region_wise_random_select(w_regions, rng)
        else:
            xmin, xmax = _random_select(w_axis, rng)
        if len(h_regions) > 1:
            ymin, ymax = _region_wise_random_select(h_regions, rng)
        else:
            ymin, ymax = _random_select(h_axis, rng)
        if xmax - xmin < min_crop_side_ratio * w or ymax - ymin < min_crop_side_ratio * h:
            continue
        new, keep = [], []
        for j, p in enumerate(polys):
            poly = np.array(p)
            if not (poly[:, 0].min() > xmax or poly[:, 0].max() < xmin or poly[:, 1].min() > ymax or poly[:, 1].max() < ymin):
                poly[:, 0] -= xmin
                poly[:, 0] = np.clip(poly[:, 0], 0., (xmax - xmin - 1) * 1.)
                poly[:, 1] -= ymin
                poly[:, 1] = np.clip(poly[:, 1], 0., (ymax - ymin - 1) * 1.)
                new.append(poly)
                keep.append(j)
        if len(new) > 0:
            return (int(ymin), int(ymax), int(xmin), int(xmax)), new, keep
    return whole


def letterbox(h, w, polys, size):
    """db_transforms.resize (:185-200) / utils.test_resize: -> (scale, new h, new w, polygons * scale in fp64)"""
    scale = min(size / w, size / h)
    nh, nw = int(h * scale), int(w * scale)
    out = []
    for p in polys:
        poly = np.array(p).astype(np.float64)
        poly *= scale
        out.append(poly)
    return scale, nh, nw, out


def _polys_of(polys, i):
    return [np.asarray(p, np.float64).reshape(-1, 2) for p in (polys[i] if polys is not None else [])]


def _letterbox_plan(plan, h, w, polys, size):
    s, nh, nw, out = letterbox(h, w, polys, size)
    if nh < 1 or nw < 1:
        raise ValueError('a %d x %d image letterboxes to %d x %d at size %d' % (h, w, nh, nw, size))
    plan.update(letterbox_scale=s, out_hw=(nh, nw), polys=out)
    return plan


def plan_augment(shapes, polys, rng, size=640, rotate=ROTATE, scale=SCALE):
    """The training plan of a batch, per image a dict: flip, angle, scale (drawn from `rng`, a np.random.RandomState, in
    that order, then the crop's own draws), the forward matrix `M`, `scaled_hw` (h2, w2), `window` (ymin, ymax, xmin,
    xmax) of the scaled image, `letterbox_scale`, `out_hw`, `polys` (fp64, output-image coordinates) and `keep` (indices
    of the source polygons that survive the crop, for their tags)."""
    plans = []
    for i, shape in enumerate(shapes):
        H, W = check_shape(shape)
        flip = bool(rng.random_sample() < 0.5)
        angle = float(rng.uniform(*rotate))
        sc = float(rng.uniform(*scale))
        h2, w2 = max(1, int(round(H * sc))), max(1, int(round(W * sc)))
        if h2 > MAX_SIDE or w2 > MAX_SIDE:
            raise ValueError('image %d scales to %d x %d' % (i, h2, w2))
        M = rotation_matrix(angle, H, W)
        moved = []
        for p in _polys_of(polys, i):
            x = W - 1 - p[:, 0] if flip else p[:, 0].copy()
            y = p[:, 1]
            x, y = M[0, 0] * x + M[0, 1] * y + M[0, 2], M[1, 0] * x + M[1, 1] * y + M[1, 2]
            x, y = x * (w2 / W), y * (h2 / H)
            moved.append(np.stack([np.clip(x, 0, w2 - 1), np.clip(y, 0, h2 - 1)], 1))
        window, cropped, keep = crop_window(h2, w2, moved, rng)
        if window is None:
            window = (0, h2, 0, w2)
        ch, cw = window[1] - window[0], window[3] - window[2]
        plan = dict(flip=flip, angle=angle, scale=sc, M=M, src_hw=(H, W), scaled_hw=(h2, w2), window=window, keep=keep)
        plans.append(_letterbox_plan(plan, ch, cw, cropped, size))
    return plans


def plan_letterbox(shapes, polys=None, size=640):
    """The evaluation plan (letterbox only): per image a dict with window = the whole image, letterbox_scale, out_hw,
    polys (fp64, scaled) and keep (every polygon)."""
    plans = []
    for i, shape in enumerate(shapes):
        H, W = check_shape(shape)
        src = _polys_of(polys, i)
        plan = dict(flip=False, angle=None, scale=None, M=None, src_hw=(H, W), scaled_hw=(H, W), window=(0, H, 0, W),
                    keep=list(range(len(src))))
        plans.append(_letterbox_plan(plan, H, W, src, size))
    return plans


# ---- device stages -------------------------------------------------------------------------------------------------
def _resize_coef(src, dst):
    """cv2.resize: inv_scale = (double)dst / src, scale = 1. / inv_scale"""
    return 1. / (float(dst) / float(src))


def letterbox_args(src_off, src_hw, plans, CH, CW):
    """descriptors of dbn_resize_linear_norm_u8: (desc, coef)"""
    N = len(plans)
    desc = np.zeros((N, _DESC), np.int64)
    coef = np.zeros((N, _COEF), np.float64)
    for n, p in enumerate(plans):
        (h, w), (nh, nw) = src_hw[n], p['out_hw']
        if nh > CH or nw > CW:
            raise ValueError('image %d letterboxes to %d x %d, past the %d x %d canvas' % (n, nh, nw, CH, CW))
        desc[n, :10] = src_off[n], h, w, 0, nh, nw, 0, 0, nh, nw
        coef[n, :2] = _resize_coef(w, nw), _resize_coef(h, nh)
    return desc, coef


def _letterbox_launch(src, src_off, src_hw, plans, CH, CW, mean, dev):
    """launch 3: linear resize + normalisation into fp32 [N, 3, CH, CW] (dbn_resize_linear_norm_u8)"""
    N = len(plans)
    desc, coef = letterbox_args(src_off, src_hw, plans, CH, CW)
    out = torch.empty((N, 3, CH, CW), device=dev, dtype=torch.float32)
    m = [float(np.float32(v)) for v in mean]
    with on_device(dev) as st:
        d, c = upload(desc, dev), upload(coef, dev)
        check(lib().dbn_resize_linear_norm_u8(src.data_ptr(), src.numel(), d.data_ptr(), c.data_ptr(), N, CH, CW, m[0], m[1], m[2],
                                              out.data_ptr(), st), 'resize_linear_norm_u8')
    return out


def warp_args(src_off, shapes, plans):
    """descriptors of dbn_warp_affine_u8: (desc int64 [N, 12], coef fp64 [N, 6], max_h, max_w)"""
    N = len(shapes)
    desc = np.zeros((N, _DESC), np.int64)
    coef = np.zeros((N, _COEF), np.float64)
    for n, ((H, W), p) in enumerate(zip(shapes, plans)):
        if tuple(p['src_hw']) != (H, W):
            raise ValueError('plan %d was made for a %s image, not %s' % (n, p['src_hw'], (H, W)))
        desc[n, :11] = src_off[n], H, W, src_off[n], H, W, 0, 0, H, W, int(p['flip'])
        coef[n] = invert_affine(p['M'])
    return desc, coef, max(h for h, _ in shapes), max(w for _, w in shapes)


def warp_stage(src, src_off, shapes, plans, dev):
    """launch 1: flip + rotate (dbn_warp_affine_u8) -> packed uint8 warped images, laid out as the source"""
    desc, coef, max_h, max_w = warp_args(src_off, shapes, plans)
    warped = torch.empty(int(src_off[-1]), device=dev, dtype=torch.uint8)
    with on_device(dev) as st:
        d, c = upload(desc, dev), upload(coef, dev)
        check(lib().dbn_warp_affine_u8(src.data_ptr(), src.numel(), d.data_ptr(), c.data_ptr(), len(shapes), max_h, max_w,
                                       warped.data_ptr(), warped.numel(), st), 'warp_affine_u8')
    return warped


def cubic_args(src_off, shapes, plans):
    """descriptors of dbn_resize_cubic_u8: (desc, coef, output byte offsets [N + 1], window sizes [(h, w)], max_h, max_w)"""
    N = len(shapes)
    win_hw = []
    for p in plans:
        y0, y1, x0, x1 = p['window']
        h2, w2 = p['scaled_hw']
        if not (0 <= y0 < y1 <= h2 and 0 <= x0 < x1 <= w2 and h2 <= MAX_SIDE and w2 <= MAX_SIDE):
            raise ValueError('crop window %s outside the %d x %d scaled image' % (p['window'], h2, w2))
        win_hw.append((y1 - y0, x1 - x0))
    dst_off = image_offsets(win_hw)
    desc = np.zeros((N, _DESC), np.int64)
    coef = np.zeros((N, _COEF), np.float64)
    for n, ((H, W), p, (ch, cw)) in enumerate(zip(shapes, plans, win_hw)):
        h2, w2 = p['scaled_hw']
        y0, _, x0, _ = p['window']
        desc[n, :10] = src_off[n], H, W, dst_off[n], h2, w2, y0, x0, ch, cw
        coef[n, :2] = _resize_coef(W, w2), _resize_coef(H, h2)
    return desc, coef, dst_off, win_hw, max(h for h, _ in win_hw), max(w for _, w in win_hw)


def cubic_stage(warped, src_off, shapes, plans, dev):
    """launch 2: cubic resize to scaled_hw, the crop window only (dbn_resize_cubic_u8) -> (packed uint8 crops, their
    byte offsets, their (h, w))"""
    desc, coef, dst_off, win_hw, max_h, max_w = cubic_args(src_off, shapes, plans)
    cropped = torch.empty(int(dst_off[-1]), device=dev, dtype=torch.uint8)
    with on_device(dev) as st:
        d, c = upload(desc, dev), upload(coef, dev)
        check(lib().dbn_resize_cubic_u8(warped.data_ptr(), warped.numel(), d.data_ptr(), c.data_ptr(), len(shapes), max_h, max_w,
                                        cropped.data_ptr(), cropped.numel(), st), 'resize_cubic_u8')
    return cropped, dst_off, win_hw


def augment_images(packed_u8, shapes, plans, size=640, mean=MEAN, device=None):
    """packed uint8 images (image_collate; host or device) -> fp32 [N, 3, size, size] on the device, normalised, after
    the plans' warp, cubic resize and crop, and the letterbox.  plans=None: the evaluation letterbox alone."""
    shapes = [check_shape(s) for s in shapes]
    N, S = len(shapes), int(size)
    if N == 0:
        raise ValueError('augment_images needs at least one image')
    if plans is None:
        plans = plan_letterbox(shapes, None, S)
    if len(plans) != N:
        raise ValueError('one plan per image')
    dev = cuda_device('augment_images', device, packed_u8)
    src = packed_on(packed_u8, shapes, dev)
    src_off = image_offsets(shapes)
    if all(p['M'] is None for p in plans):
        for p, hw in zip(plans, shapes):
            if p['window'] != (0, hw[0], 0, hw[1]) or tuple(p['scaled_hw']) != hw:
                raise ValueError('a letterbox plan must cover its whole image')
        return _letterbox_launch(src, src_off, shapes, plans, S, S, mean, dev)
    if any(p['M'] is None for p in plans):
        raise ValueError('plans of one batch are all training plans or all letterbox plans')
    warped = warp_stage(src, src_off, shapes, plans, dev)
    cropped, dst_off, win_hw = cubic_stage(warped, src_off, shapes, plans, dev)
    # letterbox of the crop, normalised
    return _letterbox_launch(cropped, dst_off, win_hw, plans, S, S, mean, dev)


def preprocess_image(u8, size=640, pad=False, mean=MEAN):
    """utils.test_preprocess (:183-199) of one uint8 [H, W, 3] device image: the long side resized to `size`
    (cv2.resize INTER_LINEAR), normalised -> fp32 [1, 3, int(H*s), int(W*s)], or [1, 3, size, size] with pad=True
    (padding 0 - mean[c])."""
    if not (u8.is_cuda and u8.dtype == torch.uint8 and u8.dim() == 3 and u8.shape[2] == 3):
        raise ValueError('preprocess_image takes a uint8 [H, W, 3] device tensor')
    H, W = check_shape(u8.shape)
    plan = plan_letterbox([(H, W)], None, size)
    nh, nw = plan[0]['out_hw']
    CH, CW = (int(size), int(size)) if pad else (nh, nw)
    return _letterbox_launch(u8.contiguous().reshape(-1), np.zeros(2, np.int64), [(H, W)], plan, CH, CW, mean, u8.device)


# ---- loader surface ------------------------------------------------------------------------------------------------
def image_collate(items):
    """collate_fn for items (uint8 [H, W, 3] of any size, polys, tags): -> (packed uint8 tensor (pinned when a GPU is
    visible and this is not a DataLoader worker; the loader's pin_memory=True pins it otherwise), shapes [(H, W)], per-image
    lists of fp64 [V, 2] polygons, per-image tag lists)."""
    imgs = [np.ascontiguousarray(np.asarray(b[0], dtype=np.uint8)) for b in items]
    for im in imgs:
        if im.ndim != 3 or im.shape[2] != 3:
            raise ValueError('image_collate takes uint8 [H, W, 3] images')
    shapes = [(int(im.shape[0]), int(im.shape[1])) for im in imgs]
    off = _offsets([im.size for im in imgs])
    packed = torch.empty(int(off[-1]), dtype=torch.uint8, pin_memory=pin_default())
    view = packed.numpy()
    for im, o in zip(imgs, off):
        view[o:o + im.size] = im.reshape(-1)
    return (packed, shapes) + polys_tags(items)


class DeviceBatches:
    """Turns each (packed, shapes, polys, tags) batch of `loader` (collate_fn=image_collate, or jpeg_collate for JPEG bytes:
    the first element is then a JpegCoefficients and its device half runs here; png_collate and PngScanlines likewise) into the dict fit / evaluate consume: `img` (augment_images) and the four GT_KEYS maps (make_gt_maps), on `device`.  training=True draws the
    augmentation from np.random.RandomState(seed), continued across passes; False is the letterbox, and adds `anns`
    (per image, the scaled polygons) and `ignore_tags` (per image, the GT ignore flags) as the reference's test loader
    returns them.  orient=True: JPEG batches are decoded with their Exif orientation applied (decode_coefficients), as the
    reference's cv2.imread does; the polygons are then those of the displayed image.  gt_kwargs go to make_gt_maps
    (shrink_ratio, thresh_min, thresh_max, min_text_size, ignore_tags).  color_jitter: a dict of plan_color_jitter's
    keyword arguments (brightness, contrast, saturation, hue), e.g. {'brightness': 32 / 255, 'saturation': 0.5}; with
    training=True the decoded uint8 batch then goes through color_jitter_images in front of the geometric steps, where
    MMOCR's DBNet pipeline has its ColorJitter.  Its plans are drawn from a second RandomState (seeded with
    [seed, JITTER_STREAM]), so the geometric plans of a seed are the same with and without it; None (the default), or
    arguments that leave no operation present, make no draw and no launch.  degrade: a dict of plan_degrade's keyword
    arguments (blur, blur_p, noise, noise_p, per_channel), e.g. {'blur': 3.0, 'noise': 10.0}; with training=True the batch
    goes through degrade_images (degrade.py) behind the colour step and in front of the geometric ones, its plans drawn
    from a third RandomState (seeded with [seed, DEGRADE_STREAM]); None, or arguments that leave neither operation
    present, make no draw and no launch."""

    JITTER_STREAM = 0x636A  # second word of the colour stream's seed
    DEGRADE_STREAM = 0x6467  # ... of the degradation stream's

    def __init__(self, loader, device, training, size=640, seed=None, mean=MEAN, orient=False, color_jitter=None, degrade=None, **gt_kwargs):
        self.loader, self.device, self.training, self.size, self.mean = loader, torch.device(device), bool(training), int(size), mean
        self.orient = bool(orient)
        self.rng = np.random.RandomState(seed)
        self.color_jitter = self.jitter_rng = None
        # (a bad range or key raises here, not in the first batch)
        if color_jitter is not None and color_jitter_ranges(**color_jitter):
            self.color_jitter = dict(color_jitter)
            words = None if seed is None else np.append(np.asarray(seed, np.uint32).reshape(-1), np.uint32(self.JITTER_STREAM))
            self.jitter_rng = np.random.RandomState(words)
        self.degrade = self.degrade_rng = None
        if degrade is not None and degrade_ranges(**degrade):
            self.degrade = dict(degrade)
            words = None if seed is None else np.append(np.asarray(seed, np.uint32).reshape(-1), np.uint32(self.DEGRADE_STREAM))
            self.degrade_rng = np.random.RandomState(words)
        self.gt_kwargs = gt_kwargs

    def __len__(self):
        return len(self.loader)

    def convert(self, batch):
        packed, shapes, polys, tags = batch
        if isinstance(packed, JpegStreams):  # jpeg_stream_collate: the Huffman stage on the device too
            exif = stream_orientations([packed.blob[int(a):int(b)].numpy() for a, b in zip(packed.offs[:-1], packed.offs[1:])]) if self.orient else None
            packed = entropy_decode_device(packed, self.device)
            packed.orientation = exif
            packed.raise_errors()
        if isinstance(packed, JpegCoefficients):  # jpeg_collate: the device half of the decode
            packed, shapes = decode_coefficients(packed, self.device, self.orient)
        if isinstance(packed, PngScanlines):  # png_collate: the device half of the decode
            packed, shapes = unfilter_png(packed, self.device)
        if self.training:
            if (self.color_jitter is not None or self.degrade is not None) and not (isinstance(packed, torch.Tensor) and packed.is_cuda):
                packed = packed_on(packed, shapes, self.device)  # image_collate's pinned host batch
            if self.color_jitter is not None:
                colour_plans = plan_color_jitter(len(shapes), self.jitter_rng, **self.color_jitter)
                packed = color_jitter_images(packed, shapes, colour_plans)
            if self.degrade is not None:
                packed = degrade_images(packed, shapes, plan_degrade(len(shapes), self.degrade_rng, **self.degrade))
            plans = plan_augment(shapes, polys, self.rng, self.size)
        else:
            plans = plan_letterbox(shapes, polys, self.size)
        img = augment_images(packed, shapes, plans, self.size, self.mean, self.device)
        out_polys = [p['polys'] for p in plans]
        out_tags = [[tags[i][j] for j in p['keep']] for i, p in enumerate(plans)]
        kw = dict(self.gt_kwargs)
        offsets = None
        out = {'img': img}
        if not self.training:
            g = plan_polygons(out_polys, out_tags, self.size, **{k: kw[k] for k in ('shrink_ratio', 'min_text_size', 'ignore_tags') if k in kw})
            out['anns'] = out_polys
            out['ignore_tags'] = [[q['ignored'] for q in img_plan] for img_plan in g]
            offsets = [[(np.zeros((0, 2), np.int64), None) if q['ignored'] else (q['fill'], q['padded']) for q in img_plan] for img_plan in g]
        maps = make_gt_maps(out_polys, out_tags, self.size, self.device, offsets=offsets, **kw)
        for k, key in enumerate(GT_KEYS):
            out[key] = maps[k]
        return out

    def __iter__(self):
        for batch in self.loader:
            yield self.convert(batch)
