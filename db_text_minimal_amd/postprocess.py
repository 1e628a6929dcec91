"""Device-side array work of the reference's SegDetectorRepresenter (src/postprocess.py), SURVEY §8(f-3).

For a caller that keeps the host contour code (cv2.findContours / minAreaRect / pyclipper unclip), two operations that
touch whole probability maps run on the GPU:

  binarize_u8(preds, thresh)        postprocess.py:51-52   `pred[:, 0] > thresh` as uint8 — the bitmap findContours needs
                                                           crosses PCIe at 1 B/px instead of the 4 B/px float map
  box_scores(prob_map, boxes)       postprocess.py:186-198 box_score_fast for all candidate boxes of an image in one
                                                           launch — the float map never has to leave the device

A maintainer's change in SegDetectorRepresenter.boxes_from_bitmap (postprocess.py:105-141) is two lines: collect the
candidate boxes first, then `scores = box_scores(pred, np.stack(boxes))` instead of calling self.box_score_fast per box.

Text boxes without OpenCV or pyclipper (csrc/detect.hip):

  detect_boxes(preds, ...)          boxes_from_bitmap (postprocess.py:105-141, is_output_polygon=False) for a batch:
                                    per image int16 boxes [K, 4, 2] and fp32 scores [K], K = min(#candidates,
                                    max_candidates), skipped rows zero.  The map never leaves the device.
  SegDetectorRepresenter            the reference's class over detect_boxes (polygon output: NotImplementedError)

Semantics.  A candidate is a foreground component of `pred[n, 0] > thresh`, 8-connected: the region one outer border
of cv2.findContours encloses.  Candidates come in DESCENDING raster order of their first pixel (cv2's RETR_LIST
prepends each border it finds; this order is UNPINNED).  Hole borders, which RETR_LIST also returns, are NOT emitted.
For each candidate C: R1 = the minimum-area rectangle of C's pixel centres (same hull as the contour, so the same
minAreaRect up to ties: among equal areas the first hull edge counter-clockwise in (x, y) from the vertex of least
(y, x) wins); sside1 = its shorter side; score = mean of pred over filled(C) = C plus every component it encloses (the
pixels cv2.fillPoly of C's outer border sets), summed in fixed point and rounded once to fp32.  Then, as the
reference: skip if sside1 < 3 or score < box_thresh; order R1 as get_mini_boxes; unclip by area * unclip_ratio /
length (shapely's formulas) with the Clipper restatement of gt_maps.offset_polygon; R2 = min-area rectangle of the
unclipped points, skip if its shorter side < 5; order R2 and scale to dest size in fp32 with half-to-even rounding.
PARITY UNPINNED against cv2 / pyclipper: R1 / R2 corners come from exact integer calipers, not cv2's float
minAreaRect, and unclip keeps the largest piece of the offset where pyclipper returns all of them.
"""
import numpy as np
import torch

from ._lib import check, lib


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def binarize_u8(preds, thresh=0.3):
    """preds: [N, C, H, W] fp32 device tensor (the DBTextModel output) -> uint8 [N, H, W] bitmap of channel 0 > thresh."""
    assert preds.is_cuda and preds.dtype == torch.float32 and preds.dim() == 4 and preds.is_contiguous()
    N, C, H, W = preds.shape
    out = torch.empty((N, H, W), device=preds.device, dtype=torch.uint8)
    check(lib().dbn_binarize_u8(preds.data_ptr(), N, C, H, W, float(thresh), out.data_ptr(), _stream(preds)), 'binarize_u8')
    return out


def box_scores(prob_map, boxes):
    """prob_map: [H, W] fp32 device tensor (pred[n, 0]); boxes: array-like [K, P, 2] of (x, y) vertices, P <= 64
    -> numpy float32 [K] = box_score_fast(prob_map, boxes[k]) of the reference."""
    assert prob_map.is_cuda and prob_map.dtype == torch.float32 and prob_map.dim() == 2 and prob_map.is_contiguous()
    b = torch.as_tensor(np.ascontiguousarray(np.asarray(boxes, dtype=np.float32)))
    assert b.dim() == 3 and b.shape[2] == 2 and 1 <= b.shape[1] <= 64, b.shape
    K, P = int(b.shape[0]), int(b.shape[1])
    if K == 0:
        return np.zeros((0, ), np.float32)
    bd = b.to(prob_map.device)
    scores = torch.empty(K, device=prob_map.device, dtype=torch.float32)
    H, W = prob_map.shape
    check(lib().dbn_box_scores(prob_map.data_ptr(), H, W, bd.data_ptr(), K, P, scores.data_ptr(), _stream(prob_map)), 'box_scores')
    return scores.cpu().numpy()


# dbn_detect_rec of include/dbnet_hip.h
REC_DTYPE = np.dtype([('root', '<i4'), ('hull_n', '<i4'), ('ex', '<i4'), ('ey', '<i4'), ('dmin', '<i8'), ('dmax', '<i8'),
                      ('cmin', '<i8'), ('cmax', '<i8'), ('sum_hi', '<i8'), ('sum_lo', '<i8'), ('count', '<i8')])
assert REC_DTYPE.itemsize == 72


def detect_records(preds, thresh=0.3, max_candidates=1000, return_labels=False, prefill=None):
    """Device stage of detect_boxes, enqueued on the current stream: (records [N, max_candidates] REC_DTYPE, counts [N]
    int32 = foreground components per image[, labels [N, H, W] int32 device tensor]), copied to the host in one transfer.
    prefill: a byte value written over the workspace, labels and record buffer first (tests: results must not depend on
    their previous contents)."""
    assert preds.is_cuda and preds.dtype == torch.float32 and preds.dim() == 4, (preds.device, preds.dtype, preds.shape)
    preds = preds.contiguous()
    N, C, H, W = preds.shape
    M = int(max_candidates)
    assert M > 0
    L = lib()
    ws_bytes = L.dbn_detect_ws_bytes(N, H, W, M)
    if ws_bytes < 0:
        raise RuntimeError('libdbnet_hip: invalid argument in detect_ws_bytes')
    dev = preds.device
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    labels = torch.empty((N, H, W), device=dev, dtype=torch.int32)
    rec_bytes = N * M * REC_DTYPE.itemsize
    out = torch.empty(rec_bytes + 4 * N, device=dev, dtype=torch.uint8)  # records, then counts: one D2H copy
    if prefill is not None:
        for t in (ws, labels.view(torch.uint8), out):
            t.fill_(int(prefill))
    check(L.dbn_detect(preds.data_ptr(), N, C, H, W, float(thresh), M, ws.data_ptr(), labels.data_ptr(), out.data_ptr(),
                       out.data_ptr() + rec_bytes, _stream(preds)), 'detect')
    host = out.cpu().numpy()
    recs = host[:rec_bytes].view(REC_DTYPE).reshape(N, M)
    counts = host[rec_bytes:].view(np.int32).copy()
    return (recs, counts, labels) if return_labels else (recs, counts)


def detect_host(recs, counts, H, W, box_thresh=0.7, unclip_ratio=1.5, dest_sizes=None, return_info=False):
    """Host stage of detect_boxes (dbn_detect_host, one call for the batch) on records of detect_records.  dest_sizes:
    per image (height, width) to scale to (default (H, W)).  Returns boxes int16 [N, M, 4, 2], scores fp32 [N, M] (rows
    past min(counts[n], M) are zero)[, info fp32 [N, M, 10]: R1 corners, R1's shorter side, score of every candidate]."""
    recs = np.ascontiguousarray(recs, dtype=REC_DTYPE)
    N, M = recs.shape
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    dest = np.array([(H, W)] * N if dest_sizes is None else [(int(h), int(w)) for h, w in dest_sizes], dtype=np.int32).reshape(N, 2)
    params = np.array([float(box_thresh), float(unclip_ratio)], np.float64)
    boxes = np.zeros((N, M, 4, 2), np.int16)
    scores = np.zeros((N, M), np.float32)
    info = np.zeros((N, M, 10), np.float32)
    check(lib().dbn_detect_host(recs.ctypes.data, counts.ctypes.data, N, M, H, W, params.ctypes.data, dest.ctypes.data, boxes.ctypes.data,
                                scores.ctypes.data, info.ctypes.data), 'detect_host')
    return (boxes, scores, info) if return_info else (boxes, scores)


def detect_boxes(preds, thresh=0.3, box_thresh=0.7, max_candidates=1000, unclip_ratio=1.5, dest_sizes=None):
    """boxes_from_bitmap of the reference (is_output_polygon=False) for every image of preds [N, C, H, W] (fp32 device
    tensor, channel 0 = probability map).  dest_sizes: per image (height, width), default the map's.  Returns a list of
    (boxes int16 [K, 4, 2], scores fp32 [K]) with K = min(#candidates, max_candidates); skipped candidates are zero rows."""
    recs, counts = detect_records(preds, thresh, max_candidates)
    H, W = preds.shape[2], preds.shape[3]
    boxes, scores = detect_host(recs, counts, H, W, box_thresh, unclip_ratio, dest_sizes)
    K = np.minimum(counts, int(max_candidates))
    return [(boxes[n, :K[n]].copy(), scores[n, :K[n]].copy()) for n in range(len(K))]


class SegDetectorRepresenter:
    """The reference's SegDetectorRepresenter (postprocess.py:7-48) over detect_boxes; box output only."""

    def __init__(self, thresh=0.3, box_thresh=0.7, max_candidates=1000, unclip_ratio=1.5):
        self.min_size = 3
        self.thresh = thresh
        self.box_thresh = box_thresh
        self.max_candidates = max_candidates
        self.unclip_ratio = unclip_ratio

    def __call__(self, batch, pred, is_output_polygon=False):
        """batch['shape'][i] = (height, width) of image i; pred [N, C, H, W] fp32 device tensor -> (boxes_batch,
        scores_batch), one (int16 [K, 4, 2], fp32 [K]) pair per image."""
        if is_output_polygon:
            raise NotImplementedError('polygon output (approxPolyDP of traced contours) is not implemented')
        dest = [(int(h), int(w)) for h, w in batch['shape']]
        res = detect_boxes(pred, self.thresh, self.box_thresh, self.max_candidates, self.unclip_ratio, dest)
        return [b for b, _ in res], [s for _, s in res]
