"""Text-detection scoring: the reference's detection metric (src/iou.py, src/deteval.py, text_metrics.QuadMetric) without
shapely.

  polygon_overlaps(gt_polys, det_polys, device)   per image the fp64 G x D overlap matrix, per polygon the area and the
                                                  non-simple flag: one upload, two launches (csrc/det_eval.hip), one copy back
  DetectionIoUEvaluator / DetectionDetEvalEvaluator
                                                  the reference's classes: evaluate_image, evaluate_batch (one device
                                                  launch plus one host call, dbn_det_eval_match_host, for the whole batch),
                                                  combine_results
  QuadMetric                                      validate_measure / gather_measure of text_metrics.py
  python -m db_text_minimal_amd.det_eval {iou,deteval} ...
                                                  the reference's `make ioueval` / `make deteval` on the same pickles

Semantics.  Each polygon is oriented so that its shoelace signed area is >= 0, area = |signed area| and
overlap(A, B) = the integral of w_A * w_B (winding numbers): exactly area(A n B) for simple polygons.  The reference's
union is area_g + area_d - inter here.  Its `Polygon(p).buffer(0)` validity filter removes nothing; a self-intersecting
polygon is kept, flagged (`nonsimple`), and scored by its winding-weighted overlap where GEOS's buffer(0) may drop lobes
(UNPINNED).  GEOS's rounding of the areas (about 1e-12 relative) is UNPINNED too; away from exact ties it changes no decision.
Matching restates the reference's order and quirks, including Python's round(x, 4) of the DetEval sums.  iouMat /
recallMat / precisionMat are [] beyond 100 detections as there; where the reference returns its uninitialised
np.empty([1, 1]) they are [[0.0]].  evaluationLog is ''.

QuadMetric scores EVERY image of a batch; the reference's scores image 0 only (and requires test_batch_size: 1).  At batch
size 1 the two are the same.
"""
import argparse
import pickle
import sys

import numpy as np
import torch

from ._lib import check, lib
from .packed import on_device

IOU, DETEVAL = 0, 1


def _as_poly(points):
    a = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    if len(a) < 3:
        raise ValueError('a polygon needs at least 3 vertices, got %d' % len(a))
    return a


def _pack(gt_polys, det_polys):
    """packed vertices, polygon offsets and the per-image table {gt begin, G, det begin, D, pair offset}"""
    polys, img = [], []
    pair_off = 0
    for g, d in zip(gt_polys, det_polys):
        g0 = len(polys)
        polys.extend(_as_poly(p) for p in g)
        d0 = len(polys)
        polys.extend(_as_poly(p) for p in d)
        img.append((g0, len(g), d0, len(d), pair_off))
        pair_off += len(g) * len(d)
    counts = np.array([len(p) for p in polys], np.int64)
    poff = np.zeros(len(polys) + 1, np.int64)
    np.cumsum(counts, out=poff[1:])
    if poff[-1] >= 2**31:
        raise ValueError('too many vertices in one batch')
    verts = np.concatenate(polys) if polys else np.zeros((0, 2), np.float64)
    return verts, poff.astype(np.int32), np.array(img, np.int64).reshape(-1, 5), pair_off


def polygon_overlaps(gt_polys, det_polys, device=None, cull=True, prefill=None):
    """gt_polys, det_polys: per image a list of [V, 2] (x, y) polygons, V >= 3.  Returns per image dict(inter fp64 [G, D],
    gt_area [G], det_area [D], gt_nonsimple bool [G], det_nonsimple bool [D]).  cull=False: pairs with disjoint bounding
    boxes are computed too (measurement only).  prefill: a byte value written over the workspace and the output buffer first."""
    assert len(gt_polys) == len(det_polys)
    N = len(gt_polys)
    verts, poff, img, n_pairs = _pack(gt_polys, det_polys)
    P = len(poff) - 1
    out = []
    if P > 0:
        dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        assert dev.type == 'cuda', 'polygon_overlaps runs on the GPU'
        # one upload: verts | img | poff
        up = np.concatenate([verts.reshape(-1).view(np.uint8), img.reshape(-1).view(np.uint8), poff.view(np.uint8)])
        d_up = torch.from_numpy(up).to(dev)
        ws = torch.empty(int(lib().dbn_det_eval_ws_bytes(P)), dtype=torch.uint8, device=dev)
        # one result buffer: inter | area | nonsimple
        d_out = torch.empty(8 * n_pairs + 8 * P + 4 * P, dtype=torch.uint8, device=dev)
        base, o_img, o_poff = d_up.data_ptr(), verts.nbytes, verts.nbytes + img.nbytes
        ob = d_out.data_ptr()
        if prefill is not None:
            ws.fill_(int(prefill))
            d_out.fill_(int(prefill))
        with on_device(dev) as st:
            check(lib().dbn_det_eval_overlaps(base, base + o_poff, P, base + o_img, N, n_pairs, 1 if cull else 0, ws.data_ptr(),
                                              ob if n_pairs else None, ob + 8 * n_pairs, ob + 8 * n_pairs + 8 * P, st), 'det_eval_overlaps')
            host = d_out.cpu().numpy()
        inter = host[:8 * n_pairs].view(np.float64)
        area = host[8 * n_pairs:8 * (n_pairs + P)].view(np.float64)
        nonsimple = host[8 * (n_pairs + P):].view(np.int32) != 0
    for g0, G, d0, D, po in img.tolist():
        out.append(dict(inter=inter[po:po + G * D].reshape(G, D).copy() if G * D else np.zeros((G, D)),
                        gt_area=area[g0:g0 + G].copy() if G else np.zeros(0), det_area=area[d0:d0 + D].copy() if D else np.zeros(0),
                        gt_nonsimple=nonsimple[g0:g0 + G].copy() if G else np.zeros(0, bool),
                        det_nonsimple=nonsimple[d0:d0 + D].copy() if D else np.zeros(0, bool)))
    return out


def _centre_diag(points):
    """(mean x, mean y, bounding-box diagonal) as deteval.py's center_distance / diag compute them"""
    m = np.mean(points, axis=0)
    r = np.array(points)
    return m[0], m[1], ((r[:, 0].max() - r[:, 0].min())**2 + (r[:, 1].max() - r[:, 1].min())**2)**0.5


def match(protocol, params, ov, gt_ignore, gt_cd=None, det_cd=None):
    """dbn_det_eval_match_host on per-image overlaps (polygon_overlaps' result, or the same fields from elsewhere):
    per image (stats fp64 [8], det don't-care bool [D], pair rows int [R, 4])"""
    N = len(ov)
    if N == 0:
        return []
    sizes = np.array([[o['inter'].shape[0], o['inter'].shape[1]] for o in ov], np.int32).reshape(N, 2)
    cat = lambda xs, dt: np.ascontiguousarray(np.concatenate(xs).astype(dt)) if xs else np.zeros(0, dt)  # noqa: E731
    inter = cat([np.ascontiguousarray(o['inter'], np.float64).reshape(-1) for o in ov], np.float64)
    ga = cat([np.asarray(o['gt_area'], np.float64) for o in ov], np.float64)
    da = cat([np.asarray(o['det_area'], np.float64) for o in ov], np.float64)
    ig = cat([np.asarray(i, bool).reshape(-1) for i in gt_ignore], np.uint8)
    assert len(ig) == len(ga)
    cd = [None, None]
    if protocol == DETEVAL:
        cd = [np.ascontiguousarray(np.asarray(c, np.float64).reshape(-1, 3)) for c in (gt_cd, det_cd)]
    params = np.ascontiguousarray(params, np.float64)
    stats = np.zeros((N, 8), np.float64)
    ddc = np.zeros(max(len(da), 1), np.uint8)
    rows = np.zeros((max(2 * int(sizes.sum()), 1), 4), np.int32)
    n_rows = np.zeros(max(N, 1), np.int32)
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
    check(lib().dbn_det_eval_match_host(protocol, N, ptr(sizes), ptr(inter), ptr(ga), ptr(da), ptr(ig), ptr(cd[0]), ptr(cd[1]), params.ctypes.data,
                                        stats.ctypes.data, ddc.ctypes.data, rows.ctypes.data, n_rows.ctypes.data), 'det_eval_match_host')
    res, db, rb = [], 0, 0
    for n in range(N):
        G, D = int(sizes[n, 0]), int(sizes[n, 1])
        res.append((stats[n].copy(), ddc[db:db + D].astype(bool), rows[rb:rb + n_rows[n]].copy()))
        db += D
        rb += 2 * (G + D)
    return res


def _pairs(rows, deteval):
    """the reference's `pairs` list from the host call's rows {pair, kind, gt, det}"""
    if not deteval:
        return [{'gt': int(g), 'det': int(d)} for _, _, g, d in rows.tolist()]
    groups = []
    for idx, kind, g, d in rows.tolist():
        if not groups or groups[-1][0] != idx:
            groups.append((idx, kind, []))
        groups[-1][2].append((g, d))
    out = []
    for _, kind, members in groups:
        if kind == 0:
            out.append({'gt': members[0][0], 'det': members[0][1], 'type': 'OO'})
        elif kind == 1:
            ds = [d for _, d in members if d >= 0]
            out.append({'gt': members[0][0], 'det': ds, 'type': 'OO' if len(ds) == 1 else 'OM'})
        else:
            gs = [g for g, _ in members if g >= 0]
            out.append({'gt': gs, 'det': members[0][1], 'type': 'OO' if len(gs) == 1 else 'MO'})
    return out


class _Evaluator:
    protocol = None

    def _params(self):
        raise NotImplementedError

    def evaluate_image(self, gt, pred):
        return self.evaluate_batch([gt], [pred])[0]

    def evaluate_batch(self, gts, preds, overlaps=None, device=None):
        """gts / preds: per image a list of {'points': [V, 2], 'ignore': bool}.  overlaps: polygon_overlaps' result for
        them (computed here when None)."""
        assert len(gts) == len(preds)
        gpts = [[g['points'] for g in gt] for gt in gts]
        dpts = [[p['points'] for p in pred] for pred in preds]
        if overlaps is None:
            overlaps = polygon_overlaps(gpts, dpts, device)
        ignore = [[bool(g['ignore']) for g in gt] for gt in gts]
        deteval = self.protocol == DETEVAL
        cd = (None, None)
        if deteval:
            cd = ([_centre_diag(p) for ps in gpts for p in ps], [_centre_diag(p) for ps in dpts for p in ps])
        res = match(self.protocol, self._params(), overlaps, ignore, *cd)
        out = []
        for n, (stats, ddc, rows) in enumerate(res):
            o = overlaps[n]
            G, D = o['inter'].shape
            gdc = [g for g in range(G) if ignore[n][g]]
            ga, da, inter = np.asarray(o['gt_area']), np.asarray(o['det_area']), np.asarray(o['inter'])
            r = {'precision': float(stats[0]), 'recall': float(stats[1]), 'hmean': float(stats[2]), 'pairs': _pairs(rows, deteval)}
            if deteval:
                if D > 0:
                    with np.errstate(divide='ignore', invalid='ignore'):
                        rm = np.where(ga[:, None] == 0, 0.0, inter / np.where(ga == 0, 1.0, ga)[:, None])
                        pm = np.where(da[None, :] == 0, 0.0, inter / np.where(da == 0, 1.0, da)[None, :])
                else:
                    rm = pm = np.zeros((1, 1))
                r['recallMat'] = [] if D > 100 else rm.tolist()
                r['precisionMat'] = [] if D > 100 else pm.tolist()
            else:
                if G > 0 and D > 0:
                    with np.errstate(divide='ignore', invalid='ignore'):
                        im = inter / ((ga[:, None] + da[None, :]) - inter)
                else:
                    im = np.zeros((1, 1))
                r['iouMat'] = [] if D > 100 else im.tolist()
            r.update(gtPolPoints=gpts[n], detPolPoints=dpts[n], gtCare=int(stats[3]), detCare=int(stats[4]), gtDontCare=gdc,
                     detDontCare=[int(d) for d in np.nonzero(ddc)[0]])
            if deteval:
                r.update(recallAccum=float(stats[6]), precisionAccum=float(stats[7]))
            else:
                r['detMatched'] = int(stats[5])
            r['evaluationLog'] = ''
            out.append(r)
        return out


class DetectionIoUEvaluator(_Evaluator):
    """iou.py: greedy GT-major matching with IoU > iou_constraint; a detection is don't-care at the first ignored GT that
    covers more than area_precision_constraint of it."""
    protocol = IOU

    def __init__(self, iou_constraint=0.5, area_precision_constraint=0.5):
        self.iou_constraint = iou_constraint
        self.area_precision_constraint = area_precision_constraint

    def _params(self):
        return [self.iou_constraint, self.area_precision_constraint]

    @staticmethod
    def combine_results(results):
        gc = sum(r['gtCare'] for r in results)
        dc = sum(r['detCare'] for r in results)
        matched = sum(r['detMatched'] for r in results)
        R = 0 if gc == 0 else float(matched) / gc
        P = 0 if dc == 0 else float(matched) / dc
        H = 0 if R + P == 0 else 2 * R * P / (R + P)
        return {'precision': P, 'recall': R, 'hmean': H}


class DetectionDetEvalEvaluator(_Evaluator):
    """deteval.py: one-to-one matches (single overlap and centre distance), then one-to-many and many-to-one."""
    protocol = DETEVAL

    def __init__(self, area_recall_constraint=0.8, area_precision_constraint=0.4, ev_param_ind_center_diff_thr=1, mtype_oo_o=1.0,
                 mtype_om_o=0.8, mtype_om_m=1.0):
        self.area_recall_constraint = area_recall_constraint
        self.area_precision_constraint = area_precision_constraint
        self.ev_param_ind_center_diff_thr = ev_param_ind_center_diff_thr
        self.mtype_oo_o = mtype_oo_o
        self.mtype_om_o = mtype_om_o
        self.mtype_om_m = mtype_om_m

    def _params(self):
        return [self.area_recall_constraint, self.area_precision_constraint, self.ev_param_ind_center_diff_thr, self.mtype_oo_o,
                self.mtype_om_o, self.mtype_om_m]

    @staticmethod
    def combine_results(results):
        gc, dc, rs, ps = 0, 0, 0, 0
        for r in results:
            gc += r['gtCare']
            dc += r['detCare']
            rs += r['recallAccum']
            ps += r['precisionAccum']
        R = 0 if gc == 0 else rs / gc
        P = 0 if dc == 0 else ps / dc
        H = 0 if R + P == 0 else 2 * R * P / (R + P)
        return {'precision': P, 'recall': R, 'hmean': H}


class AverageMeter:
    """text_metrics.AverageMeter"""

    def __init__(self):
        self.val, self.avg, self.sum, self.count = 0, 0, 0, 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count
        return self


def gather_counts(combined, n_images):
    """gather_measure's AverageMeters from combine_results' dict over n_images images"""
    precision, recall, fmeasure = AverageMeter(), AverageMeter(), AverageMeter()
    precision.update(combined['precision'], n=n_images)
    recall.update(combined['recall'], n=n_images)
    fmeasure.update(2 * precision.val * recall.val / (precision.val + recall.val + 1e-8))
    return {'precision': precision, 'recall': recall, 'fmeasure': fmeasure}


class QuadMetric:
    """text_metrics.QuadMetric.  batch['anns'][n]: the GT polygons of image n ([V, 2] each); batch['ignore_tags'][n]: their
    ignore flags; output = (boxes_batch, scores_batch) of SegDetectorRepresenter (box rows [K, 4, 2] — all-zero rows count as
    detections of area 0, as in the reference — or polygon lists).  Every image of the batch is scored (the reference: image
    0 only)."""

    def __init__(self, evaluator=None):
        self.evaluator = evaluator if evaluator is not None else DetectionIoUEvaluator()

    def measure(self, batch, output, is_output_polygon=False, box_thresh=0.6):
        boxes_batch = output[0]
        anns, tags = batch['anns'], batch['ignore_tags']
        gts = [[{'points': np.asarray(p), 'ignore': bool(t)} for p, t in zip(a, ig)] for a, ig in zip(anns, tags)]
        preds = [[{'points': np.asarray(p), 'ignore': False} for p in boxes] for boxes in boxes_batch]
        assert len(gts) == len(preds), (len(gts), len(preds))
        return self.evaluator.evaluate_batch(gts, preds)

    def validate_measure(self, batch, output, is_output_polygon=False, box_thresh=0.6):
        return self.measure(batch, output, is_output_polygon, box_thresh)

    def gather_measure(self, raw_metrics):
        raw = [m for batch_metrics in raw_metrics for m in batch_metrics]
        return gather_counts(self.evaluator.combine_results(raw), len(raw))


def main(argv=None, overlaps_fn=None):
    """`python -m db_text_minimal_amd.det_eval {iou,deteval}`: the reference's iou.py / deteval.py command lines"""
    ap = argparse.ArgumentParser(prog='python -m db_text_minimal_amd.det_eval')
    sub = ap.add_subparsers(dest='protocol', required=True)
    a = sub.add_parser('iou')
    a.add_argument('--iou', type=float, default=0.5)
    a.add_argument('--area', type=float, default=0.5)
    b = sub.add_parser('deteval')
    b.add_argument('--tp', type=float, default=0.4)
    b.add_argument('--tr', type=float, default=0.8)
    for p in (a, b):
        p.add_argument('--poly_gts_fp', type=str, default='./data/result_poly_gts.pkl')
        p.add_argument('--poly_preds_fp', type=str, default='./data/result_poly_preds.pkl')
    args = ap.parse_args(argv)
    if args.protocol == 'iou':
        ev = DetectionIoUEvaluator(iou_constraint=args.iou, area_precision_constraint=args.area)
    else:
        ev = DetectionDetEvalEvaluator(area_recall_constraint=args.tr, area_precision_constraint=args.tp)
    with open(args.poly_gts_fp, 'rb') as f:
        gts = pickle.load(f)
    with open(args.poly_preds_fp, 'rb') as f:
        preds = pickle.load(f)
    gts, preds = list(gts)[:len(preds)], list(preds)[:len(gts)]  # zip() of the reference
    ov = None
    if overlaps_fn is not None:
        ov = overlaps_fn([[g['points'] for g in gt] for gt in gts], [[p['points'] for p in pr] for pr in preds])
    metrics = ev.combine_results(ev.evaluate_batch(gts, preds, overlaps=ov))
    print(metrics)
    return metrics


if __name__ == '__main__':
    main(sys.argv[1:])
