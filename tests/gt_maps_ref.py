"""TEST INFRASTRUCTURE ONLY — a numpy model of the ground-truth maps the reference's loader draws
(data_loaders.py:98-167 with db_transforms.draw_thresh_map), given the host plan of
db_text_minimal_amd.gt_maps.plan_polygons (ignore flags, D, shrunk / padded / truncated integer polygons).

It is written as the device kernel computes, one polygon at a time with all of its edges at once:

  threshold term at a pixel g of the padded box (box-local coordinates, edge a -> b, all fp64):
      ga = |g - a|^2, gb = |g - b|^2, ab = |a - b|^2           (each |.|^2 = x-square + y-square, in that order)
      c  = ((ab - ga) - gb) / (2 sqrt(ga gb))
      h  = sqrt(((ga gb) nan_to_num(1 - c^2)) / ab)            distance to the edge's line
      e  = sqrt(fmin(ga, gb)) where c < 0, else h              (the nearer endpoint when the angle at g is acute)
      per edge: fp32(clip(e / D, 0, 1)); over edges: min, NaN-propagating; then fp32 1 - min
  canvas = fmax(term, canvas) over the pixels `box_to_canvas` maps; thresh_map = canvas * fp32(max - min) + fp32(min).
cv2.fillPoly is oracle.postprocess_oracle.fill_poly_mask.  Pinned bit-exact against tests/golden/gt_maps.npz, which
the reference's own code produced (tests/golden/make_gt_golden.py).  Where the reference's box-to-canvas copy has an
empty source it raises; here the polygon adds no threshold, as the kernel documents.  tools/gt_maps_probe.py times
this model as the CPU baseline.
"""
import numpy as np

from oracle.postprocess_oracle import fill_poly_mask


def box_to_canvas(lo, hi, size):
    """Along one axis: (canvas pixels, box indices) of the reference's copy of box lo..hi into a canvas of `size` pixels,
    or None where its source is empty.  Both ends are clamped into the canvas and the box is indexed by numpy's rules, so
    a box starting k >= 2 pixels past the last pixel hands index width - k to pixel size - 1."""
    first, last = min(max(lo, 0), size - 1), min(max(hi, 0), size - 1)
    src = np.arange(hi - lo + 1)[first - lo:last - lo + 1]
    dst = np.arange(first, last + 1)
    return (dst, src) if len(src) == len(dst) else None


def threshold_term(poly_local, gx, gy, D):
    """fp32 [len(gy), len(gx)]: 1 - min over edges of fp32(clip(e / D, 0, 1)) at box-local pixels (gx, gy)."""
    a = poly_local[:, None, None, :]
    b = np.roll(poly_local, -1, axis=0)[:, None, None, :]
    x, y = gx[None, None, :], gy[None, :, None]
    ga = np.square(x - a[..., 0]) + np.square(y - a[..., 1])
    gb = np.square(x - b[..., 0]) + np.square(y - b[..., 1])
    ab = np.square(a[..., 0] - b[..., 0]) + np.square(a[..., 1] - b[..., 1])
    with np.errstate(divide='ignore', invalid='ignore'):
        c = (ab - ga - gb) / (2 * np.sqrt(ga * gb))
        to_line = np.sqrt(ga * gb * np.nan_to_num(1 - np.square(c)) / ab)
        e = np.where(c < 0, np.sqrt(np.fmin(ga, gb)), to_line)
        per_edge = np.clip(e / D, 0, 1).astype(np.float32)
    return np.float32(1) - per_edge.min(axis=0)


def add_threshold(canvas, poly, padded, D):
    """canvas = fmax(threshold term, canvas) over the padded polygon's box, clipped as the reference clips it."""
    padded = np.asarray(padded)
    (x0, y0), (x1, y1) = padded.min(axis=0), padded.max(axis=0)
    cols, rows = box_to_canvas(x0, x1, canvas.shape[1]), box_to_canvas(y0, y1, canvas.shape[0])
    if cols is None or rows is None:
        return
    local = np.asarray(poly, np.float64) - np.array([x0, y0], np.float64)
    term = threshold_term(local, cols[1].astype(np.float64), rows[1].astype(np.float64), D)
    sel = np.ix_(rows[0], cols[0])
    canvas[sel] = np.fmax(term, canvas[sel])


def maps_for_image(plan, size, thresh_min=0.3, thresh_max=0.7):
    """[4, S, S] float32 in GT_KEYS order for one image's plan (list of dicts of gt_maps.plan_polygons)."""
    S = int(size)
    out = np.zeros((4, S, S), np.float32)
    out[1] = 1
    for p in plan:
        if p['ignored']:
            out[1][fill_poly_mask(S, S, p['fill']) != 0] = 0
            continue
        out[0][fill_poly_mask(S, S, p['fill']) != 0] = 1
        out[3][fill_poly_mask(S, S, p['padded']) != 0] = 1
        add_threshold(out[2], p['poly'], p['padded'], p['D'])
    out[2] = out[2] * np.float32(thresh_max - thresh_min) + np.float32(thresh_min)
    return out


def maps_for_batch(plans, size, **kw):
    return np.stack([maps_for_image(p, size, **kw) for p in plans], axis=1)


def normalize(u8, mean=(103.939, 116.779, 123.68)):
    """one uint8 [H, W, 3] image -> fp32 [3, H, W]: fp32(u8) - fp32(mean[c]) per channel."""
    return (u8.astype(np.float32) - np.asarray(mean, np.float32)).transpose(2, 0, 1)
