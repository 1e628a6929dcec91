"""DBNet ground truth on the device: the four maps of train.py GT_KEYS from text polygons, and uint8 image
normalisation — what the reference's BaseDatasetIter.__getitem__ (data_loaders.py:87-172) and draw_thresh_map
(db_transforms.py:8-82) compute per image on the CPU.

  make_gt_maps(polys, tags, size, device)   [4, N, S, S] fp32 (prob_map, supervision_mask, thresh_map, text_area_map),
                                            one launch for the batch (csrc/gtmaps.hip), on the current stream
  normalize_images(u8)                      uint8 [N, H, W, 3] -> fp32 [N, 3, H, W], (float)u8 - (float)mean[c]
  offset_polygon(poly, delta)               the shrink / pad of pyclipper's PyclipperOffset, JT_ROUND, on the host
  gt_collate                                DataLoader collate: uint8 images + polygons, not maps

A loader then ships a uint8 image and its polygons (about 1.2 MB per 640^2 image) instead of 11.4 MB of fp32 maps and
image, and the maps cost no loader CPU time beyond the polygon offsets:

    u8, polys, tags = batch                                   # from DataLoader(..., collate_fn=gt_collate)
    img = normalize_images(u8.to(dev, non_blocking=True))
    trainer.step(img, make_gt_maps(polys, tags, img.shape[-1], dev))

Ignore rules (data_loaders.py:108-148), decided on the host: a polygon is ignored (supervision_mask set to 0 over the
fillPoly of poly.astype(int32)) if its area < 1, min(height, width) < min_text_size, its tag is in ignore_tags, its shrink
is empty, or the shrink has <= 2 points.  The reference's `Polygon(...).buffer(0).is_valid` filters (data_loaders.py:87,
130) are not applied: for a simple polygon, and for the output of a polygon offset, they are always true.  Area and
perimeter are shapely's (GEOS Area::ofRing / Length::ofLine, restated in `_area` / `_length`).

Where the reference's numpy slicing of draw_thresh_map produces an empty slice (a padded box wholly left of / above the
image, or starting exactly one pixel or more than its width past the right / bottom edge) the reference raises
ValueError; here that polygon adds nothing to thresh_map (its other maps are drawn).

PARITY UNPINNED against pyclipper: offset_polygon restates Clipper 6's ClipperOffset (csrc/gtmaps.hip) and is pinned by
analytic cases (tests/test_gt_maps_cpu.py); the shrunk / padded vertices can differ from pyclipper's by the rounding of
intersection points, and when a shrink splits into several pieces this routine takes the one of largest area where the
reference takes pyclipper's first.  A boundary chain whose rounded intersection points do not close is dropped, so a
shrink can come back smaller or empty (the polygon then ignored) where pyclipper's would not.  A caller who has pyclipper
passes its results in with `offsets=`.
"""
import ctypes

import numpy as np
import torch

from ._lib import check, lib
from .packed import stream

GT_KEYS = ('prob_map', 'supervision_mask', 'thresh_map', 'text_area_map')
MEAN = (103.939, 116.779, 123.68)  # data_loaders.py:30, applied in RGB channel order as the reference does
MAX_VERTS = 64  # vertices of one source polygon (csrc/gtmaps.hip GT_MAX_VERTS)
MAX_OFF_PTS = 1024  # vertices of one shrunk / padded polygon (GT_MAX_OFF_PTS)
_META = 20


def _area(poly):
    """shapely Polygon(poly).area: GEOS Area::ofRing on the closed ring, |signed area|."""
    r = np.concatenate([poly, poly[:1]]).astype(np.float64)
    if len(r) < 4:
        return 0.0
    x0 = r[0, 0]
    s = 0.0
    for i in range(1, len(r) - 1):
        s += (r[i, 0] - x0) * (r[i - 1, 1] - r[i + 1, 1])
    return abs(s / 2.0)


def _length(poly):
    """shapely Polygon(poly).length: GEOS Length::ofLine over the closed ring."""
    r = np.concatenate([poly, poly[:1]]).astype(np.float64)
    s = 0.0
    for i in range(1, len(r)):
        dx, dy = r[i, 0] - r[i - 1, 0], r[i, 1] - r[i - 1, 1]
        s += np.sqrt(dx * dx + dy * dy)
    return float(s)


def shrink_distance(poly, shrink_ratio=0.4):
    """D = area * (1 - r^2) / perimeter (data_loaders.py:120-121, db_transforms.py:16-17), fp64 in the reference's order."""
    poly = np.asarray(poly, dtype=np.float64)
    return _area(poly) * (1 - np.power(shrink_ratio, 2)) / _length(poly)


def offset_polygon(poly, delta):
    """Clipper 6 ClipperOffset(JT_ROUND, ET_CLOSEDPOLYGON, ArcTolerance 0.25).Execute(delta) of one closed path, on the
    host (dbn_poly_offset).  Coordinates are cast to integers toward zero first, as pyclipper converts a float.  Returns
    int64 [K, 2]: the piece of largest area (shape (0, 2) if the offset vanishes).  PARITY UNPINNED against pyclipper
    (module docstring)."""
    xy = np.ascontiguousarray(np.asarray(poly, dtype=np.float64).reshape(-1, 2))
    d = np.array([float(delta)], np.float64)
    n = np.zeros(1, np.int32)
    cap = 1024
    while True:
        out = np.zeros((cap, 2), np.int32)
        rc = lib().dbn_poly_offset(xy.ctypes.data, len(xy), d.ctypes.data, out.ctypes.data, cap, n.ctypes.data)
        if rc == 1 and n[0] > cap:
            cap = int(n[0])
            continue
        check(rc, 'poly_offset')
        return out[:n[0]].astype(np.int64)


def offset_polygon_paths(poly, delta):
    """offset_polygon plus the number of paths Clipper's Execute returns, outer loops and holes
    (dbn_poly_offset_paths): (int64 [K, 2] piece of largest area, paths)."""
    xy = np.ascontiguousarray(np.asarray(poly, dtype=np.float64).reshape(-1, 2))
    d = np.array([float(delta)], np.float64)
    n = np.zeros(1, np.int32)
    paths = np.zeros(1, np.int32)
    cap = 1024
    while True:
        out = np.zeros((cap, 2), np.int32)
        rc = lib().dbn_poly_offset_paths(xy.ctypes.data, len(xy), d.ctypes.data, out.ctypes.data, cap, n.ctypes.data, paths.ctypes.data)
        if rc == 1 and n[0] > cap:
            cap = int(n[0])
            continue
        check(rc, 'poly_offset_paths')
        return out[:n[0]].astype(np.int64), int(paths[0])


def _bbox(pts):
    return int(pts[:, 0].min()), int(pts[:, 0].max()), int(pts[:, 1].min()), int(pts[:, 1].max())


def _slice_range(lo, hi, S):
    """canvas pixels draw_thresh_map's numpy slicing writes along one axis (csrc/gtmaps.hip gt_slice_index)."""
    width = hi - lo + 1
    if lo <= S - 1:
        return (max(lo, 0), min(hi, S - 1)) if hi >= 0 else (0, -1)
    k = lo - (S - 1)
    return (S - 1, S - 1) if 2 <= k <= width else (0, -1)


def plan_polygons(polys, tags, size, shrink_ratio=0.4, min_text_size=8, ignore_tags=('###', ), offsets=None):
    """The host half of make_gt_maps: per image, per polygon, a dict with the source polygon (fp64), `ignored`, D, and
    the integer polygons `fill` (shrunk, or poly.astype(int32) if ignored) and `padded` (None if ignored)."""
    plans = []
    for i, img_polys in enumerate(polys):
        img_tags = tags[i] if tags is not None else None
        out = []
        for j, poly in enumerate(img_polys):
            poly = np.asarray(poly, dtype=np.float64).reshape(-1, 2)
            if not 1 <= len(poly) <= MAX_VERTS:
                raise ValueError('image %d polygon %d: %d vertices (1 .. %d supported)' % (i, j, len(poly), MAX_VERTS))
            if not np.isfinite(poly).all():
                raise ValueError('image %d polygon %d: non-finite coordinates' % (i, j))
            height = poly[:, 1].max() - poly[:, 1].min()
            width = poly[:, 0].max() - poly[:, 0].min()
            tag = img_tags[j] if img_tags is not None else None
            p = dict(poly=poly, ignored=True, D=0.0, fill=poly.astype(np.int32), padded=None)
            out.append(p)
            if _area(poly) < 1 or min(height, width) < min_text_size or tag in ignore_tags:
                continue
            D = shrink_distance(poly, shrink_ratio)
            if offsets is not None:
                shrunk, padded = offsets[i][j]
            else:
                shrunk, padded = offset_polygon(poly, -D), None
            shrunk = np.asarray(shrunk, dtype=np.int64).reshape(-1, 2)
            if len(shrunk) <= 2:
                continue
            if padded is None:
                padded = offset_polygon(poly, D)
            padded = np.asarray(padded, dtype=np.int64).reshape(-1, 2)
            if len(padded) == 0:
                raise ValueError('image %d polygon %d: empty padded polygon' % (i, j))
            p.update(ignored=False, D=D, fill=shrunk.astype(np.int32), padded=padded.astype(np.int32))
        plans.append(out)
    return plans


def pack_plans(plans, size):
    """-> (verts fp64 [V, 2], dist fp64 [P], meta int32 [P, 20], img_off int32 [N + 1], ixy int32 [Q, 2], max_verts,
    max_off_pts): the CSR arguments of dbn_gt_maps (include/dbnet_hip.h)."""
    S = int(size)
    verts, dist, meta, ixy, img_off = [], [], [], [], [0]
    nv = nq = 0
    max_v = max_o = 0
    for img in plans:
        for p in img:
            m = np.zeros(_META, np.int64)
            fill, padded = p['fill'], p['padded']
            if len(fill) > MAX_OFF_PTS or (padded is not None and len(padded) > MAX_OFF_PTS):
                raise ValueError('offset polygon over %d vertices' % MAX_OFF_PTS)
            m[0], m[1], m[2] = nv, len(p['poly']), int(p['ignored'])
            m[3], m[4] = nq, len(fill)
            ixy.append(fill)
            nq += len(fill)
            sx0, sx1, sy0, sy1 = _bbox(fill)
            m[15:19] = sx0, sx1, sy0, sy1
            bx0, bx1, by0, by1 = sx0, sx1, sy0, sy1
            if padded is not None:
                m[5], m[6] = nq, len(padded)
                ixy.append(padded)
                nq += len(padded)
                px0, px1, py0, py1 = _bbox(padded)
                m[11:15] = px0, px1, py0, py1
                (tx0, tx1), (ty0, ty1) = _slice_range(px0, px1, S), _slice_range(py0, py1, S)
                bx0, bx1, by0, by1 = min(bx0, px0), max(bx1, px1), min(by0, py0), max(by1, py1)
                if tx0 <= tx1 and ty0 <= ty1:
                    bx0, bx1, by0, by1 = min(bx0, tx0), max(bx1, tx1), min(by0, ty0), max(by1, ty1)
                max_o = max(max_o, len(padded))
            max_o = max(max_o, len(fill))
            max_v = max(max_v, len(p['poly']))
            m[7:11] = max(bx0, 0), min(bx1, S - 1), max(by0, 0), min(by1, S - 1)
            verts.append(p['poly'])
            nv += len(p['poly'])
            dist.append(p['D'])
            meta.append(m)
        img_off.append(len(meta))
    P = len(meta)
    return (np.ascontiguousarray(np.concatenate(verts) if verts else np.zeros((0, 2)), dtype=np.float64),
            np.asarray(dist, np.float64), np.asarray(meta, np.int32).reshape(P, _META), np.asarray(img_off, np.int32),
            np.ascontiguousarray(np.concatenate(ixy) if ixy else np.zeros((0, 2)), dtype=np.int32), max_v, max_o)


def make_gt_maps(polys, tags, size, device, shrink_ratio=0.4, thresh_min=0.3, thresh_max=0.7, min_text_size=8,
                 ignore_tags=('###', ), offsets=None, out=None):
    """The four GT maps of a batch, [4, N, S, S] fp32 on `device` in GT_KEYS order (what DBTrainer.step takes as gts),
    computed by one launch on the current stream.

    polys: per image, a list of [V, 2] (x, y) polygons in output-image coordinates (V <= 64); tags: per image, a list of
    strings (the annotation text; tags in `ignore_tags` are ignored) or None.  offsets: optional, per image, per polygon,
    (shrunk, padded) integer polygons — e.g. (pco.Execute(-D)[0] or [], pco.Execute(D)[0]) from pyclipper — in place of
    offset_polygon; entries of polygons ignored before the shrink are not read.  out: optional [4, N, S, S] fp32 tensor."""
    N, S = len(polys), int(size)
    if N == 0 or S <= 0:
        raise ValueError('make_gt_maps needs at least one image and size > 0')
    if tags is not None and len(tags) != N:
        raise ValueError('tags must have one list per image')
    dev = torch.device(device) if out is None else out.device
    if dev.type != 'cuda':
        raise ValueError('make_gt_maps runs on a GPU device, not %s' % dev)
    plans = plan_polygons(polys, tags, S, shrink_ratio, min_text_size, ignore_tags, offsets)
    verts, dist, meta, img_off, ixy, max_v, max_o = pack_plans(plans, S)
    if out is None:
        out = torch.empty((4, N, S, S), device=dev, dtype=torch.float32)
    elif not (out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (4, N, S, S) and out.is_contiguous()):
        raise ValueError('out must be a contiguous fp32 device tensor of shape [4, %d, %d, %d]' % (N, S, S))
    args = [torch.from_numpy(a).to(out.device) for a in (verts, dist, meta, img_off, ixy)]
    scale = float(np.float32(thresh_max - thresh_min))
    ptr = [a.data_ptr() if a.numel() else None for a in args]
    ptr[3] = args[3].data_ptr()
    check(lib().dbn_gt_maps(*ptr, N, len(meta), S, max_v, max_o, scale, float(np.float32(thresh_min)), out.data_ptr(), stream(out.device)),
          'gt_maps')
    return out


def normalize_images(u8, mean=MEAN):
    """uint8 [N, H, W, 3] device tensor (RGB, as the reference's loader holds it) -> fp32 [N, 3, H, W] = (float)u8 -
    (float)mean[c], bit-exact to data_loaders.py:161-167 (numpy: float32 array minus a Python float)."""
    if not (u8.is_cuda and u8.dtype == torch.uint8 and u8.dim() == 4 and u8.shape[3] == 3):
        raise ValueError('normalize_images takes a uint8 [N, H, W, 3] device tensor')
    u8 = u8.contiguous()
    N, H, W, _ = u8.shape
    out = torch.empty((N, 3, H, W), device=u8.device, dtype=torch.float32)
    m = [float(np.float32(v)) for v in mean]
    check(lib().dbn_normalize_u8(u8.data_ptr(), N, H, W, m[0], m[1], m[2], out.data_ptr(), stream(u8.device)), 'normalize_u8')
    return out


def gt_collate(batch):
    """collate_fn for torch.utils.data.DataLoader over items (img_u8 [S, S, 3], polys, tags): -> (uint8 [N, S, S, 3]
    tensor, list of per-image polygon lists, list of per-image tag lists).  Maps are built on the device afterwards."""
    imgs = torch.stack([torch.as_tensor(np.ascontiguousarray(b[0]), dtype=torch.uint8) for b in batch])
    polys = [[np.asarray(p, dtype=np.float64) for p in b[1]] for b in batch]
    tags = [list(b[2]) if b[2] is not None else [None] * len(b[1]) for b in batch]
    return imgs, polys, tags
