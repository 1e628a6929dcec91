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
"""
import numpy as np
import torch

from ._lib import check, lib
from .augment import _MAX_SIDE, _check_shape, _offsets, _packed, _stream, _to_device

SIZE = (32, 100)  # (h, w) of test_ocr.py / test_webcam.py / utils.py
_WP_PX, _INT_MAX = 1024, 2 ** 31 - 1  # output pixels per workgroup of warp_perspective_u8


def _size(size):
    try:
        h, w = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError('size must be (height, width), got %r' % (size, ))
    if not (1 <= h <= _MAX_SIDE and 1 <= w <= _MAX_SIDE):
        raise ValueError('crop size %d x %d outside 1 .. %d' % (h, w, _MAX_SIDE))
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


def _images(images):
    """-> (packed uint8 tensor, [(H, W)]): image_collate's (packed, shapes, ...) or one uint8 [H, W, 3] tensor"""
    if isinstance(images, torch.Tensor):
        if images.dtype != torch.uint8 or images.dim() != 3 or images.shape[2] != 3:
            raise ValueError('a single image must be a uint8 [H, W, 3] tensor')
        return images.contiguous().reshape(-1), [_check_shape(images.shape)]
    if not isinstance(images, (tuple, list)) or len(images) < 2 or not isinstance(images[0], torch.Tensor):
        raise ValueError('images must be (packed uint8 tensor, shapes) as image_collate gives them, or a uint8 [H, W, 3] tensor')
    packed, shapes = images[0], [_check_shape(s) for s in images[1]]
    if packed.dtype != torch.uint8 or packed.dim() != 1:
        raise ValueError('the packed images must be a flat uint8 tensor (image_collate)')
    need = sum(h * w * 3 for h, w in shapes)
    if packed.numel() != need:
        raise ValueError('the packed images hold %d bytes, the shapes need %d' % (packed.numel(), need))
    return packed, shapes


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
    packed, shapes = _images(images)
    quads, index = select_boxes(boxes, scores, min_score)
    if index.size and int(index[:, 0].max()) >= len(shapes):
        raise ValueError('boxes for %d images, but %d images' % (int(index[:, 0].max()) + 1, len(shapes)))
    if device is not None:
        dev = torch.device(device)
    else:
        dev = packed.device if packed.is_cuda else torch.device('cuda', torch.cuda.current_device())
    if dev.type != 'cuda':
        raise ValueError('crop_words runs on a GPU device, not %s' % dev)
    K = quads.shape[0]
    if h * w + _WP_PX > _INT_MAX or -(-K * h * w // _WP_PX) > _INT_MAX // 256:  # dbn_warp_perspective_u8's grid
        raise ValueError('%d crops of %d x %d are too many for one call' % (K, h, w))
    src = _packed(packed, shapes, dev)
    crops = torch.empty((K, h, w, 3), device=dev, dtype=torch.uint8)
    if K == 0:
        return crops, index
    src_off = _offsets([sh * sw * 3 for sh, sw in shapes])
    hw = np.array(shapes, np.int64)[index[:, 0]]
    desc = np.stack([src_off[index[:, 0]], hw[:, 0], hw[:, 1]], 1)
    _, inv = perspective_maps(quads, (h, w))
    d, m = _to_device(desc, dev), _to_device(inv, dev)
    check(lib().dbn_warp_perspective_u8(src.data_ptr(), src.numel(), d.data_ptr(), m.data_ptr(), K, h, w, crops.data_ptr(), crops.numel(),
                                        _stream(dev)), 'warp_perspective_u8')
    return crops, index
