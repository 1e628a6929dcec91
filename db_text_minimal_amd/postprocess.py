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
  detect_polygons(preds, ...)       polygons_from_bitmap (postprocess.py:54-103, is_output_polygon=True) for a batch:
                                    per image a list of int64 [P, 2] polygons and a list of float scores, kept
                                    candidates only.  detect_contours is its device stage, detect_poly_host its host stage.
  SegDetectorRepresenter            the reference's class: __call__ over detect_boxes, .polygons over detect_polygons
                                    (__call__(..., is_output_polygon=True) still raises NotImplementedError)

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

Polygons.  Same candidates, order and max_candidates truncation as the boxes; hole borders are
NOT emitted (RETR_LIST would return them as candidates too).  Per candidate C: contour = C's outer border as
cv2.findContours(RETR_LIST, CHAIN_APPROX_SIMPLE) traces it, from C's raster-first pixel, counter-clockwise on screen,
keeping the pixels where the step direction changes.  The device traces every border at once: a crack is (pixel of C,
side) with background or the frame across it, its successor is a function of a 2 x 2 block, and Wyllie pointer
jumping ranks the cracks of each cycle from its head (the left crack of C's first pixel).  Host, as the reference:
eps = 0.005 * arcLength (a + b sqrt(2) over a axis and b diagonal steps), approxPolyDP (OpenCV 4.x's closed-curve
algorithm, fp64); skip if fewer than 4 points; score = mean of pred over filled(C) rounded once to fp64 (float32 of it
is the box score), skip if box_thresh > score; unclip by area * unclip_ratio / length; skip if the offset has more
than one path (pieces or holes); skip if the shorter side of its min-area rectangle is < 5 (-1 for an empty offset);
scale the int64 vertices as clip(round(v / size * dest), 0, dest) in fp64, half to even.  PARITY UNPINNED against cv2
/ pyclipper: approxPolyDP and arcLength rounding are restated, not checked against cv2; the offset is the Clipper
restatement of gt_maps.offset_polygon.
"""
import numpy as np
import torch

from ._lib import check, lib
from .packed import stream


def binarize_u8(preds, thresh=0.3):
    """preds: [N, C, H, W] fp32 device tensor (the DBTextModel output) -> uint8 [N, H, W] bitmap of channel 0 > thresh."""
    assert preds.is_cuda and preds.dtype == torch.float32 and preds.dim() == 4 and preds.is_contiguous()
    N, C, H, W = preds.shape
    out = torch.empty((N, H, W), device=preds.device, dtype=torch.uint8)
    check(lib().dbn_binarize_u8(preds.data_ptr(), N, C, H, W, float(thresh), out.data_ptr(), stream(preds.device)), 'binarize_u8')
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
    check(lib().dbn_box_scores(prob_map.data_ptr(), H, W, bd.data_ptr(), K, P, scores.data_ptr(), stream(prob_map.device)), 'box_scores')
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
                       out.data_ptr() + rec_bytes, stream(preds.device)), 'detect')
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


def _poly_table_layout(N, M):
    rec = N * M * REC_DTYPE.itemsize
    return rec, rec + 4 * N, rec + 4 * N + 4 * N * M, rec + 4 * N + 8 * N * M, rec + 4 * N + 8 * N * M + 16


def detect_contours(preds, thresh=0.3, max_candidates=1000, prefill=None):
    """Device stage of detect_polygons, enqueued on the current stream: dbn_detect, then the outer border of every kept
    candidate traced in parallel.  Returns dict(recs [N, M] REC_DTYPE, counts [N] int32, nv [N, M] int32 (compressed
    vertices per candidate), voff [N, M] int32 (offsets into verts), verts int16 [V, 2] (x, y) packed over the batch,
    info int32 [4] = (vertices, cracks, pointer-jumping rounds run, rounds launched)).  Two transfers: the fixed-size
    table, then exactly the V vertices.  prefill: a byte value written over every workspace and output buffer first."""
    assert preds.is_cuda and preds.dtype == torch.float32 and preds.dim() == 4, (preds.device, preds.dtype, preds.shape)
    preds = preds.contiguous()
    N, C, H, W = preds.shape
    M = int(max_candidates)
    assert M > 0
    L = lib()
    ws_bytes, pws_bytes, cap = L.dbn_detect_ws_bytes(N, H, W, M), L.dbn_detect_poly_ws_bytes(N, H, W, M), L.dbn_detect_poly_verts_cap(N, H, W)
    if min(ws_bytes, pws_bytes, cap) < 0:
        raise RuntimeError('libdbnet_hip: invalid argument in detect_poly_ws_bytes')
    dev = preds.device
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    pws = torch.empty(pws_bytes, device=dev, dtype=torch.uint8)
    labels = torch.empty((N, H, W), device=dev, dtype=torch.int32)
    o_counts, o_nv, o_voff, o_info, size = _poly_table_layout(N, M)
    table = torch.empty(size, device=dev, dtype=torch.uint8)
    verts = torch.empty((cap, 2), device=dev, dtype=torch.int16)
    if prefill is not None:
        for t in (ws, pws, labels.view(torch.uint8), table, verts.view(torch.uint8)):
            t.fill_(int(prefill))
    check(L.dbn_detect_poly(preds.data_ptr(), N, C, H, W, float(thresh), M, ws.data_ptr(), pws.data_ptr(), labels.data_ptr(), table.data_ptr(),
                            verts.data_ptr(), stream(preds.device)), 'detect_poly')
    host = table.cpu().numpy()
    info = host[o_info:].view(np.int32).copy()
    return dict(recs=host[:o_counts].view(REC_DTYPE).reshape(N, M), counts=host[o_counts:o_nv].view(np.int32).copy(),
                nv=host[o_nv:o_voff].view(np.int32).reshape(N, M).copy(), voff=host[o_voff:o_info].view(np.int32).reshape(N, M).copy(),
                verts=verts[:int(info[0])].cpu().numpy(), info=info)


def contour_of(c, n, k):
    """the compressed outer border of candidate k of image n from detect_contours' result: int64 [P, 2] (x, y)"""
    o = int(c['voff'][n, k])
    return c['verts'][o:o + int(c['nv'][n, k])].astype(np.int64)


def detect_poly_host(c, H, W, box_thresh=0.7, unclip_ratio=1.5, dest_sizes=None, return_info=False):
    """Host stage of detect_polygons (dbn_detect_poly_host, one call for the batch) on the result of detect_contours.
    Returns per image (list of int64 [P, 2] polygons, list of float scores), kept candidates only[, info dict: score64,
    n_approx, paths, sside as [N, M] arrays (paths 0 / sside -1 where the candidate was skipped first), approx (per
    image, per candidate: int64 [A, 2] approxPolyDP vertices)]."""
    recs = np.ascontiguousarray(c['recs'], dtype=REC_DTYPE)
    N, M = recs.shape
    counts = np.ascontiguousarray(c['counts'], dtype=np.int32)
    nv, voff = np.ascontiguousarray(c['nv'], np.int32), np.ascontiguousarray(c['voff'], np.int32)
    verts = np.ascontiguousarray(c['verts'], np.int16).reshape(-1, 2)
    if len(verts) == 0:
        verts = np.zeros((1, 2), np.int16)
    dest = np.array([(H, W)] * N if dest_sizes is None else [(int(h), int(w)) for h, w in dest_sizes], dtype=np.int32).reshape(N, 2)
    params = np.array([float(box_thresh), float(unclip_ratio)], np.float64)
    pn, poff = np.zeros((N, M), np.int32), np.zeros((N, M), np.int32)
    scores = np.zeros((N, M), np.float64)
    info = np.zeros((N, M, 4), np.float64)
    approx = np.zeros((max(len(verts), 1), 2), np.int32)
    total = np.zeros(1, np.int32)
    cap = 4096
    while True:
        pxy = np.zeros((cap, 2), np.int32)
        rc = lib().dbn_detect_poly_host(recs.ctypes.data, counts.ctypes.data, nv.ctypes.data, voff.ctypes.data, verts.ctypes.data, N, M, H, W,
                                        params.ctypes.data, dest.ctypes.data, pn.ctypes.data, poff.ctypes.data, pxy.ctypes.data, cap,
                                        total.ctypes.data, scores.ctypes.data, info.ctypes.data, approx.ctypes.data)
        if rc == 1 and total[0] > cap:
            cap = int(total[0])
            continue
        check(rc, 'detect_poly_host')
        break
    res = []
    for n in range(N):
        K = min(int(counts[n]), M)
        ks = [k for k in range(K) if pn[n, k] > 0]
        res.append(([pxy[poff[n, k]:poff[n, k] + pn[n, k]].astype(np.int64) for k in ks], [float(scores[n, k]) for k in ks]))
    if not return_info:
        return res
    K = np.minimum(counts, M)
    ap = [[approx[voff[n, k]:voff[n, k] + int(info[n, k, 1])].astype(np.int64) for k in range(K[n])] for n in range(N)]
    return res, dict(score64=info[..., 0].copy(), n_approx=info[..., 1].astype(np.int64), paths=info[..., 2].astype(np.int64),
                     sside=info[..., 3].copy(), approx=ap)


def detect_polygons(preds, thresh=0.3, box_thresh=0.7, max_candidates=1000, unclip_ratio=1.5, dest_sizes=None):
    """polygons_from_bitmap of the reference (is_output_polygon=True) for every image of preds [N, C, H, W] (fp32 device
    tensor, channel 0 = probability map).  dest_sizes: per image (height, width), default the map's.  Returns per image
    (list of int64 [P, 2] polygons, list of float scores), the kept candidates only, as the reference."""
    c = detect_contours(preds, thresh, max_candidates)
    return detect_poly_host(c, preds.shape[2], preds.shape[3], box_thresh, unclip_ratio, dest_sizes)


class SegDetectorRepresenter:
    """The reference's SegDetectorRepresenter (postprocess.py:7-48): __call__ over detect_boxes (box output), .polygons
    over detect_polygons (polygon output)."""

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
            raise NotImplementedError('is_output_polygon=True is not routed here: use SegDetectorRepresenter.polygons or detect_polygons')
        dest = [(int(h), int(w)) for h, w in batch['shape']]
        res = detect_boxes(pred, self.thresh, self.box_thresh, self.max_candidates, self.unclip_ratio, dest)
        return [b for b, _ in res], [s for _, s in res]

    def polygons(self, batch, pred):
        """The reference's __call__(batch, pred, is_output_polygon=True): (boxes_batch, scores_batch), per image a list
        of int64 [P, 2] polygons and a list of float scores."""
        dest = [(int(h), int(w)) for h, w in batch['shape']]
        res = detect_polygons(pred, self.thresh, self.box_thresh, self.max_candidates, self.unclip_ratio, dest)
        return [p for p, _ in res], [s for _, s in res]
