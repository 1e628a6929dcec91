"""Word images from detected text boxes on the device: the crop step of the reference's inference path
(test_ocr.py:160-177, test_webcam.py:260-271, utils.py:257-270), which hands each box to a text recogniser as

    M = cv2.getPerspectiveTransform(box.astype(float32), [[0, 0], [w, 0], [w, h], [0, h]])
    warp = cv2.warpPerspective(img, M, (w, h))            # INTER_LINEAR, BORDER_CONSTANT 0, h, w = 32, 100

  perspective_maps(quads, size)                      host: forward and inverse 3 x 3 maps (fp64) of K quads, one C call
  crop_words(images, boxes, size, scores, min_score) device: uint8 [K, h, w, 3] crops of every kept box of every image,
                                                     one launch (csrc/resample.hip warp_perspective_u8), and their
                                                     (image, box row) index

The maps restate OpenCV 4.2's getPerspectiveTransform (the 8 x 8 system solved by its LU) and its 3 x 3 invert; the pixels
restate WarpPerspectiveInvoker + remapBilinear on 8-bit data.  PARITY UNPINNED against cv2 itself, which could not be run
here: its SIMD / IPP paths, and whether the restated LU and invert match it in every operation.

The reference stops there (test_ocr.py:162 crops only `if not opt.is_output_polygon`).  For polygon output, its default:

  polygon_ribbons(polygons, segments, ends)          host: the ribbon of every polygon (centre line and cross-sections,
                                                     fp64 -> int32 units of 1 / 1024 px), one C call
  polygon_ribbons_device(polygons, segments, ends)   device: the same ribbons with the same bits, one launch (csrc/rectify.hip
                                                     polygon_ribbons_kernel); rectify_words(..., ribbons='device') uses it
  rectify_words(images, polygons, size, ...)         device: every kept polygon straightened into an h x w crop, one launch
                                                     (csrc/rectify.hip rectify_u8), and their (image, polygon row) index
  rectify_from_ribbons(images, knots, valid, ...)    the device half alone, on knots of the caller's choosing

What a straightened polygon is is THIS PROJECT'S DEFINITION, in exact integers on the device.
"""
import numpy as np
import torch

from ._lib import check, lib
from .packed import MAX_SIDE, as_images, cuda_device, image_table, on_device, packed_on, upload
from .packed import offsets as _offsets

SIZE = (32, 100)  # (h, w) of test_ocr.py / test_webcam.py / utils.py
_WP_PX, _INT_MAX = 1024, 2 ** 31 - 1  # output pixels per workgroup of warp_perspective_u8
_MIN_SEG, _MAX_SEG, _MAX_VERTS, _MAX_COORD, _HOST_THREADS = 4, 64, 256, 2.0 ** 20, 16  # dbn_polygon_ribbons
_RC_PX, _RC_MAX_HW = 1024, 2 ** 30  # dbn_rectify_u8: output pixels per workgroup, the largest crop


def _size(size):
    try:
        h, w = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError('size must be (height, width), got %r' % (size, ))
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError('crop size %d x %d outside 1 .. %d' % (h, w, MAX_SIDE))
    return h, w


def _quads(quads):
    q = np.asarray(quads)
    if q.ndim != 3 or q.shape[1:] != (4, 2):
        raise ValueError('quads must be [K, 4, 2], got shape %s' % (q.shape, ))
    q = np.ascontiguousarray(q, dtype=np.float32)  # np.array(box.tolist(), dtype=np.float32), as the reference builds them
    if not np.isfinite(q).all():
        raise ValueError('quads must be finite')
    return q


def perspective_maps(quads, size=SIZE):
    """quads [K, 4, 2] (x, y), corner i mapped to (0, 0), (w, 0), (w, h), (0, h) -> (forward, inverse), fp64 [K, 3, 3]:
    cv2.getPerspectiveTransform (zeros with M[2, 2] = 1 for a singular system) and the inverse cv2.warpPerspective samples
    through (zeros for a singular map).  One host call for the batch (dbn_perspective_maps)."""
    q = _quads(quads)
    h, w = _size(size)
    K = q.shape[0]
    fwd = np.zeros((K, 3, 3), np.float64)
    inv = np.zeros((K, 3, 3), np.float64)
    check(lib().dbn_perspective_maps(q.ctypes.data, K, h, w, fwd.ctypes.data, inv.ctypes.data), 'perspective_maps')
    return fwd, inv


def select_boxes(boxes, scores=None, min_score=None):
    """The boxes crop_words cuts out: per image int16 [K, 4, 2] boxes (or the (boxes, scores) pairs of detect_boxes),
    rows with box.reshape(-1).sum() <= 0 dropped (test_ocr.py:150) and, with min_score, rows scoring below it
    (test_webcam.py:265).  -> (quads fp32 [K, 4, 2], index int64 [K, 2] of (image, box row))."""
    if isinstance(boxes, np.ndarray) and boxes.ndim == 3:
        boxes = [boxes]
    boxes = list(boxes)
    pairs = [isinstance(b, tuple) and len(b) == 2 for b in boxes]
    if any(pairs):
        if not all(pairs):
            raise ValueError('boxes mixes (boxes, scores) pairs with plain box arrays')
        if scores is None:
            scores = [s for _, s in boxes]
        boxes = [b for b, _ in boxes]
    if scores is not None and len(scores) != len(boxes):
        raise ValueError('%d score arrays for %d images' % (len(scores), len(boxes)))
    if min_score is not None and scores is None:
        raise ValueError('min_score needs the scores')
    quads, index = [], []
    for n, b in enumerate(boxes):
        b = np.asarray(b)
        if b.size == 0:
            continue
        if b.ndim != 3 or b.shape[1:] != (4, 2):
            raise ValueError('boxes of image %d must be [K, 4, 2], got shape %s' % (n, b.shape))
        keep = b.reshape(b.shape[0], -1).sum(axis=1) > 0
        if min_score is not None:
            s = np.asarray(scores[n]).reshape(-1)
            if s.shape[0] != b.shape[0]:
                raise ValueError('image %d has %d boxes and %d scores' % (n, b.shape[0], s.shape[0]))
            keep &= s.astype(np.float64) >= float(min_score)  # a float32 score against a Python float, in double
        rows = np.flatnonzero(keep)
        quads.append(_quads(b[rows]))
        index.append(np.stack([np.full(rows.shape, n, np.int64), rows.astype(np.int64)], 1))
    if not quads:
        return np.zeros((0, 4, 2), np.float32), np.zeros((0, 2), np.int64)
    return np.concatenate(quads), np.concatenate(index)


def crop_words(images, boxes, size=SIZE, scores=None, min_score=None, device=None):
    """cv2.warpPerspective of every kept box of every image into an h x w word image, on the device.

    images: (packed uint8, shapes) as image_collate gives them (its extra items are ignored), on the host or the device,
    or one uint8 [H, W, 3] tensor.  boxes: per image the int16 [K, 4, 2] boxes of detect_boxes(..., dest_sizes=...) /
    SegDetectorRepresenter()(batch, preds) in original-image coordinates (or detect_boxes' (boxes, scores) pairs).
    Dropped: all-zero rows (sum <= 0) and, with min_score, rows whose score is below it.  Returns (crops, index): crops
    uint8 [K, h, w, 3] on the device in the source's channel order, index int64 [K, 2] numpy of (image, box row).
    device: where to crop (default: the packed images' device, else the current one).  One launch on the current
    stream; the maps are one host call."""
    h, w = _size(size)
    packed, shapes = as_images(images)
    quads, index = select_boxes(boxes, scores, min_score)
    if index.size and int(index[:, 0].max()) >= len(shapes):
        raise ValueError('boxes for %d images, but %d images' % (int(index[:, 0].max()) + 1, len(shapes)))
    dev = cuda_device('crop_words', device, packed)
    K = quads.shape[0]
    if h * w + _WP_PX > _INT_MAX or -(-K * h * w // _WP_PX) > _INT_MAX // 256:  # dbn_warp_perspective_u8's grid
        raise ValueError('%d crops of %d x %d are too many for one call' % (K, h, w))
    src = packed_on(packed, shapes, dev)
    crops = torch.empty((K, h, w, 3), device=dev, dtype=torch.uint8)
    if K == 0:
        return crops, index
    _, inv = perspective_maps(quads, (h, w))
    with on_device(dev) as st:
        d, m = image_table(shapes, dev, index[:, 0]), upload(inv, dev)
        check(lib().dbn_warp_perspective_u8(src.data_ptr(), src.numel(), d.data_ptr(), m.data_ptr(), K, h, w, crops.data_ptr(), crops.numel(), st),
              'warp_perspective_u8')
    return crops, index


# ---- word images of text polygons (csrc/rectify.hip; this project's definition) ------------------------
def _segments(segments):
    s = int(segments)
    if s != segments or not (_MIN_SEG <= s <= _MAX_SEG):
        raise ValueError('segments must be an integer in %d .. %d, got %r' % (_MIN_SEG, _MAX_SEG, segments))
    return s


def _polygon(p, ends):
    p = np.asarray(p)
    if p.ndim != 2 or p.shape[1] != 2 or p.dtype.kind not in 'iuf':
        raise ValueError('a polygon must be a numeric [P, 2] array, got shape %s' % (p.shape, ))
    n = p.shape[0]
    if not (3 <= n <= _MAX_VERTS):
        raise ValueError('a polygon has 3 .. %d vertices, got %d' % (_MAX_VERTS, n))
    if ends == 'half' and n % 2:
        raise ValueError("ends='half' needs an even number of vertices, got %d" % n)
    p = p.astype(np.float64)
    if not (np.abs(p) <= _MAX_COORD).all():  # false for a NaN
        raise ValueError('polygon coordinates must be finite and within +-2^20')
    return p


def polygon_ribbons(polygons, segments=32, ends='auto', return_info=False):
    """The ribbon of every polygon, the host half of rectify_words (dbn_polygon_ribbons: one C call, fp64, up to 16 threads).

    polygons: a sequence of [P, 2] (x, y) arrays in border order, either orientation, 3 <= P <= 256, finite and within
    +-2^20.  The word's two ends are two of the 2P boundary points (vertices and edge midpoints): with ends='auto' the
    non-adjacent pair whose two boundary chains lie closest to each other (detector output), with ends='half' the middles
    of the edges (v[P-1], v[0]) and (v[P/2-1], v[P/2]), the annotation order of Total-Text and CTW1500 (first half one side,
    second half the other side back).  Returns (knots int32 [K, S + 1, 4], valid uint8 [K]): per knot the centre-line point
    and the cross-section vector (width times unit normal) in units of 1 / 1024 pixel; valid = 0 (zero knots) for a
    polygon without area, width or length[, and with return_info a dict: ends int32 [K, 2] (the boundary-point indices
    i, j), E, width, length fp64 [K]]."""
    S = _segments(segments)
    if ends not in ('auto', 'half'):
        raise ValueError("ends must be 'auto' or 'half', got %r" % (ends, ))
    polys = [_polygon(p, ends) for p in polygons]
    K = len(polys)
    knots, valid = np.zeros((K, S + 1, 4), np.int32), np.zeros(K, np.uint8)
    found, info = np.zeros((K, 2), np.int32), np.zeros((K, 3), np.float64)
    if K:
        xy = np.ascontiguousarray(np.concatenate(polys))
        offs = _offsets([len(p) for p in polys])
        check(lib().dbn_polygon_ribbons(xy.ctypes.data, offs.ctypes.data, K, S, int(ends == 'half'), _HOST_THREADS, knots.ctypes.data,
                                        valid.ctypes.data, found.ctypes.data, info.ctypes.data), 'polygon_ribbons')
    if return_info:
        return knots, valid, dict(ends=found, E=info[:, 0].copy(), width=info[:, 1].copy(), length=info[:, 2].copy())
    return knots, valid


def _checked_vertices(polygons, ends):
    """_polygon's checks for a whole batch -> (vertex counts, fp64 [total, 2]): shapes and counts per polygon, the values
    once on the concatenated vertices (a batch waits for these checks longer than for the kernel); anything out of order
    goes through _polygon one by one, which raises what polygon_ribbons raises"""
    arrs = [np.asarray(p) for p in polygons]
    if arrs and all(a.ndim == 2 and a.shape[1] == 2 and a.dtype.kind in 'iuf' and 3 <= a.shape[0] <= _MAX_VERTS and
                    not (ends == 'half' and a.shape[0] % 2) for a in arrs):
        xy = np.concatenate(arrs).astype(np.float64, copy=False)
        if (np.abs(xy) <= _MAX_COORD).all():
            return [a.shape[0] for a in arrs], xy
    polys = [_polygon(p, ends) for p in arrs]
    return [len(p) for p in polys], (np.concatenate(polys) if polys else np.zeros((0, 2), np.float64))


def polygon_ribbons_device(polygons, segments=32, ends='auto', return_info=False, device=None):
    """polygon_ribbons on the device (dbn_polygon_ribbons_device, one workgroup per polygon): the same
    arguments, the same ValueErrors before any work, and the same bits, as torch tensors on the device: (knots int32
    [K, S + 1, 4], valid uint8 [K])[, and with return_info a dict of device tensors: ends int32 [K, 2], E, width, length
    fp64 [K]].  One pinned, non-blocking copy of the vertices and their offsets, one launch on the current stream, no
    synchronisation; K = 0: empty tensors, no launch."""
    S = _segments(segments)
    if ends not in ('auto', 'half'):
        raise ValueError("ends must be 'auto' or 'half', got %r" % (ends, ))
    counts, xy = _checked_vertices(polygons, ends)
    dev = cuda_device('polygon_ribbons_device', device)
    K = len(counts)
    knots, valid = torch.empty((K, S + 1, 4), device=dev, dtype=torch.int32), torch.empty(K, device=dev, dtype=torch.uint8)
    found, info = torch.empty((K, 2), device=dev, dtype=torch.int32), torch.empty((K, 3), device=dev, dtype=torch.float64)
    if K:
        offs = _offsets(counts)
        total = int(offs[-1])
        both = np.empty(K + 1 + 2 * total, np.float64)  # the K + 1 offsets (as int64) and the vertices behind them: one copy
        both[:K + 1].view(np.int64)[:] = offs
        both[K + 1:] = xy.reshape(-1)
        with on_device(dev) as st:
            d = upload(both, dev)
            check(lib().dbn_polygon_ribbons_device(d.data_ptr() + 8 * (K + 1), d.data_ptr(), K, total, S, int(ends == 'half'), knots.data_ptr(),
                                                   valid.data_ptr(), found.data_ptr(), info.data_ptr(), st), 'polygon_ribbons_device')
    if return_info:
        return knots, valid, dict(ends=found, E=info[:, 0].contiguous(), width=info[:, 1].contiguous(), length=info[:, 2].contiguous())
    return knots, valid


def select_polygons(polygons, scores=None, min_score=None):
    """The polygons rectify_words straightens: per image a list of [P, 2] arrays (or the (polygons, scores) pairs of
    detect_polygons), those with a coordinate sum <= 0 dropped and, with min_score, those scoring below it: select_boxes'
    rule.  -> (list of [P, 2] arrays, index int64 [K, 2] of (image, polygon row))."""
    polygons = list(polygons)
    pairs = [isinstance(p, tuple) and len(p) == 2 for p in polygons]
    if any(pairs):
        if not all(pairs):
            raise ValueError('polygons mixes (polygons, scores) pairs with plain polygon lists')
        if scores is None:
            scores = [s for _, s in polygons]
        polygons = [p for p, _ in polygons]
    if scores is not None and len(scores) != len(polygons):
        raise ValueError('%d score lists for %d images' % (len(scores), len(polygons)))
    if min_score is not None and scores is None:
        raise ValueError('min_score needs the scores')
    kept, index = [], []
    for n, ps in enumerate(polygons):
        if min_score is not None and len(scores[n]) != len(ps):
            raise ValueError('image %d has %d polygons and %d scores' % (n, len(ps), len(scores[n])))
        for k, p in enumerate(ps):
            p = np.asarray(p)
            if p.size == 0 or p.sum() <= 0:
                continue
            if min_score is not None and float(scores[n][k]) < float(min_score):
                continue
            kept.append(p)
            index.append((n, k))
    return kept, np.array(index, np.int64).reshape(-1, 2)


def rectify_from_ribbons(images, knots, valid, image_index, size=SIZE, device=None):
    """The device half of rectify_words alone (dbn_rectify_u8, one launch): crop q is read from image image_index[q] along
    the ribbon knots[q] (int32 [S + 1, 4], polygon_ribbons' layout, any values); valid[q] = 0 gives a zero crop.  images as
    crop_words takes them.  knots and valid are numpy arrays, or both CUDA tensors (int32 / uint8, contiguous, on the
    device that cuts the crops, as polygon_ribbons_device returns them), which are used in place.  -> uint8 [K, h, w, 3]
    on the device."""
    h, w = _size(size)
    packed, shapes = as_images(images)
    ribbons_there = isinstance(knots, torch.Tensor) or isinstance(valid, torch.Tensor)
    if ribbons_there:  # polygon_ribbons_device's tensors, used where they are
        for name, a, dtype in (('knots', knots, torch.int32), ('valid', valid, torch.uint8)):
            if not (isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == dtype and a.is_contiguous()):
                raise ValueError('%s on the device must be a contiguous %s CUDA tensor (and so must the other)' % (name, dtype))
    else:
        knots = np.ascontiguousarray(knots, dtype=np.int32)
    if knots.ndim != 3 or knots.shape[2] != 4:
        raise ValueError('knots must be int32 [K, S + 1, 4], got shape %s' % (tuple(knots.shape), ))
    K, S = knots.shape[0], _segments(knots.shape[1] - 1)
    valid = valid.reshape(-1) if ribbons_there else np.ascontiguousarray(valid, dtype=np.uint8).reshape(-1)
    image_index = np.ascontiguousarray(image_index, dtype=np.int64).reshape(-1)
    if valid.shape[0] != K or image_index.shape[0] != K:
        raise ValueError('%d ribbons, %d valid flags, %d image indices' % (K, valid.shape[0], image_index.shape[0]))
    if K and not (0 <= int(image_index.min()) and int(image_index.max()) < len(shapes)):
        raise ValueError('image indices outside the %d images' % len(shapes))
    # dbn_rectify_u8: h w <= 2^30 keeps the 64-bit pixel arithmetic exact for any int32 knots; the grid is one run of blocks
    if h * w > _RC_MAX_HW or K * -(-h * w // _RC_PX) > _INT_MAX:
        raise ValueError('%d crops of %d x %d are too many or too large for one call' % (K, h, w))
    dev = cuda_device('rectify_words', device, packed)
    if ribbons_there and {knots.device, valid.device} != {dev}:
        raise ValueError('knots on %s and valid on %s, the crops are cut on %s' % (knots.device, valid.device, dev))
    src = packed_on(packed, shapes, dev)
    crops = torch.empty((K, h, w, 3), device=dev, dtype=torch.uint8)
    if K == 0:
        return crops
    with on_device(dev) as st:
        d = image_table(shapes, dev, image_index)
        kn, va = (knots, valid) if ribbons_there else (upload(knots, dev), upload(valid, dev))
        check(lib().dbn_rectify_u8(src.data_ptr(), src.numel(), d.data_ptr(), kn.data_ptr(), va.data_ptr(), K, S, h, w, crops.data_ptr(),
                                   crops.numel(), st), 'rectify_u8')
    return crops


def rectify_words(images, polygons, size=SIZE, scores=None, min_score=None, segments=32, ends='auto', device=None, ribbons='host'):
    """Every kept text polygon of every image straightened into an h x w word image, on the device: crop_words for curved
    text.  The reference crops boxes only (test_ocr.py:162), so what a straightened polygon is is this project's
    definition: the ribbon of polygon_ribbons, sampled with x = 0 on its start cap and y = 0 on its top
    side, bilinearly with a zero border, in integers.  An axis-aligned rectangle of the crop's size is the plain slice, as
    crop_words gives for that box.

    images: as crop_words takes them.  polygons: per image a list of [P, 2] arrays in the images' pixel coordinates, or
    the (polygons, scores) pairs of detect_polygons(..., dest_sizes=...).  Dropped: polygons whose coordinates sum to <= 0
    and, with min_score, those scoring below it.  Returns (crops, index): crops uint8 [K, h, w, 3] on the device, index
    int64 [K, 2] numpy of (image, polygon row).  One host call for the ribbons, one launch on the current stream; with
    ribbons='device' the ribbons are found on the device too (polygon_ribbons_device: the same knots, so the same bytes)
    and stay there: the vertices cross to the device, no knots."""
    _size(size)
    if not (isinstance(ribbons, str) and ribbons in ('host', 'device')):
        raise ValueError("ribbons must be 'host' or 'device', got %r" % (ribbons, ))
    packed, shapes = as_images(images)
    kept, index = select_polygons(polygons, scores, min_score)
    if index.size and int(index[:, 0].max()) >= len(shapes):
        raise ValueError('polygons for %d images, but %d images' % (int(index[:, 0].max()) + 1, len(shapes)))
    if ribbons == 'device':
        # where rectify_from_ribbons will cut them: the packed images' device, else the current one
        knots, valid = polygon_ribbons_device(kept, segments, ends, device=device if device is not None or not packed.is_cuda else packed.device)
    else:
        knots, valid = polygon_ribbons(kept, segments, ends)
    return rectify_from_ribbons((packed, shapes), knots, valid, index[:, 0], size, device), index
