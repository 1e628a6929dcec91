#!/usr/bin/env python3
"""Generate tests/golden/eval_kats.npz from the REFERENCE's own detection metric code.

Run in the build container only (needs the reference checkout; nothing in the test suite or on the GPU box runs this):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_eval_golden.py

It imports the reference's iou.py (DetectionIoUEvaluator), deteval.py (DetectionDetEvalEvaluator) and
text_metrics.QuadMetric and runs their own matching code, with the third-party modules the image lacks replaced:
  shapely.geometry.Polygon   backed by the exact oracle of tests/eval_ref.py: .area, .intersection(o).area and
                             .union(o).area are exact Fractions rounded once to fp64; buffer(0) returns the polygon;
                             is_valid / is_simple are True (every input here is simple)
  utils.to_list_tuples_coords  the collated-annotation unpacking of utils.py (x[0], y[0] per vertex)
The per-image dicts (without evaluationLog and the echoed points), combine_results and gather_measure's values are stored
next to the inputs as one JSON document (floats round-trip exactly).
"""
import json
import math
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import eval_ref as E  # noqa: E402


class Polygon:
    def __init__(self, points):
        self.points = [(float(x), float(y)) if not isinstance(x, (int, np.integer)) else (int(x), int(y)) for x, y in
                       np.asarray(points, dtype=object).reshape(-1, 2).tolist()]

    def buffer(self, _):
        return self

    is_valid = True
    is_simple = True

    @property
    def area(self):
        return float(E.area_exact(self.points))

    def intersection(self, other):
        return _Area(E.overlap_exact(self.points, other.points))

    def union(self, other):
        return _Area(E.area_exact(self.points) + E.area_exact(other.points) - E.overlap_exact(self.points, other.points))


class _Area:
    def __init__(self, v):
        self.area = float(v)


def _install_stubs():
    shapely = types.ModuleType('shapely')
    geom = types.ModuleType('shapely.geometry')
    geom.Polygon = Polygon
    shapely.geometry = geom
    sys.modules['shapely'] = shapely
    sys.modules['shapely.geometry'] = geom
    utils = types.ModuleType('utils')

    def to_list_tuples_coords(anns):
        return [[(x[0].tolist(), y[0].tolist()) for x, y in ann] for ann in anns]

    utils.to_list_tuples_coords = to_list_tuples_coords
    sys.modules['utils'] = utils
    sys.path.insert(0, '/root/reference/src')


def star(rng, cx, cy, r, n, integer):
    """a simple star-shaped polygon around (cx, cy)"""
    angs = sorted(rng.uniform(0, 2 * math.pi) for _ in range(n))
    pts = []
    for a in angs:
        rr = r * rng.uniform(0.5, 1.0)
        x, y = cx + rr * math.cos(a), cy + rr * math.sin(a)
        pts.append((int(round(x)), int(round(y))) if integer else (x, y))
    if rng.random() < 0.3:
        pts = pts[::-1]  # clockwise
    return pts


def rect(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def random_image(rng, integer):
    G, D = rng.randint(1, 5), rng.randint(1, 6)
    gts = []
    for _ in range(G):
        gts.append({'points': star(rng, rng.uniform(20, 180), rng.uniform(20, 180), rng.uniform(10, 30), rng.randint(3, 8), integer),
                    'ignore': rng.random() < 0.2})
    dets = []
    for k in range(D):
        if k < G and rng.random() < 0.8:
            src = gts[k]['points']
            cx, cy = np.mean(np.array(src, float), axis=0)
            s = rng.uniform(0.8, 1.25)
            dx, dy = rng.uniform(-4, 4), rng.uniform(-4, 4)
            pts = [(cx + s * (x - cx) + dx, cy + s * (y - cy) + dy) for x, y in src]
            if integer:
                pts = [(int(round(x)), int(round(y))) for x, y in pts]
            if len(set(pts)) < 3 or not E.is_simple(pts):
                pts = star(rng, cx, cy, 15, 5, integer)
        else:
            pts = star(rng, rng.uniform(20, 180), rng.uniform(20, 180), rng.uniform(10, 30), rng.randint(3, 8), integer)
        dets.append({'points': pts, 'ignore': False})
    return gts, dets


def spike_det():
    """a detection covering the GT [0, 1]^2 whose vertex mean sits far out on a thin spike: one-to-one by area, rejected by
    the centre distance"""
    pts = [(0.0, 0.0), (1.0, 0.0), (1.0, 0.495)]
    for i in range(31):
        a = -math.pi / 2 * 0.9 + math.pi * 0.9 * i / 30
        pts.append((100.0 + 0.001 * math.cos(a), 0.5 + 0.001 * math.sin(a)))
    pts += [(1.0, 0.505), (1.0, 1.0), (0.0, 1.0)]
    return pts


def kat_images():
    imgs = []
    g = lambda p, ig=False: {'points': p, 'ignore': ig}  # noqa: E731
    d = lambda p: {'points': p, 'ignore': False}  # noqa: E731
    # IoU exactly 0.5 (no match), just above 0.5, exactly-contained
    imgs.append(([g(rect(0, 0, 4, 2)), g(rect(10, 0, 14, 4))], [d(rect(0, 0, 4, 4)), d(rect(10, 0, 14, 3))]))
    # don't-care: ignored GT covering a detection by more than half, one by exactly half (kept)
    imgs.append(([g(rect(0, 0, 10, 10), True), g(rect(20, 0, 30, 10))],
                 [d(rect(1, 1, 5, 5)), d(rect(5, 0, 15, 10)), d(rect(20, 0, 30, 10)), d(rect(40, 40, 50, 50))]))
    # no GT, detections / GT, no detections / neither / only ignored GT
    imgs.append(([], [d(rect(0, 0, 3, 3))]))
    imgs.append(([g(rect(0, 0, 3, 3))], []))
    imgs.append(([], []))
    imgs.append(([g(rect(0, 0, 3, 3), True)], [d(rect(0, 0, 3, 3)), d(rect(10, 10, 12, 12))]))
    # DetEval: one-to-one rejected by the centre distance
    imgs.append(([g(rect(0.0, 0.0, 1.0, 1.0))], [d(spike_det())]))
    # DetEval: one-to-many split, many-to-one merge
    imgs.append(([g(rect(0, 0, 10, 2))], [d(rect(0, 0, 5, 2)), d(rect(5, 0, 10, 2))]))
    imgs.append(([g(rect(0, 0, 5, 2)), g(rect(5, 0, 10, 2))], [d(rect(0, 0, 10, 2))]))
    # DetEval: round(sum, 4) at the decimal tie 0.79995: the double nearest it lies above (0.8, a one-to-many match), the
    # next double below lies below (0.7999, none)
    below = float(np.nextafter(0.79995, 0))
    imgs.append(([g(rect(0, 0, 20000, 1))], [d(rect(0, 0, 7999.5, 1)), d(rect(7999.5, 0, 15999, 1))]))
    imgs.append(([g(rect(0.0, 0.0, 1.0, 1.0))], [d(rect(0.0, 0.0, 0.5, 1.0)), d(rect(0.5, 0.0, below, 1.0))]))
    return imgs


def strip(r):
    return {k: v for k, v in r.items() if k not in ('evaluationLog', 'gtPolPoints', 'detPolPoints')}


def main():
    _install_stubs()
    from iou import DetectionIoUEvaluator  # reference
    from deteval import DetectionDetEvalEvaluator  # reference
    from text_metrics import QuadMetric  # reference
    rng = random.Random(2026)
    batches = {}
    batches['random_int'] = [random_image(rng, True) for _ in range(6)]
    batches['random_float'] = [random_image(rng, False) for _ in range(6)]
    batches['kats'] = kat_images()
    doc = {'batches': {}, 'quad': []}
    evs = {'iou': DetectionIoUEvaluator(), 'deteval': DetectionDetEvalEvaluator(),
           'iou_04_08': DetectionIoUEvaluator(iou_constraint=0.4, area_precision_constraint=0.8)}
    for name, imgs in batches.items():
        entry = {'gts': [[{'points': [list(p) for p in x['points']], 'ignore': x['ignore']} for x in gt] for gt, _ in imgs],
                 'preds': [[{'points': [list(p) for p in x['points']], 'ignore': False} for x in pr] for _, pr in imgs]}
        for ename, ev in evs.items():
            res = [ev.evaluate_image(gt, pr) for gt, pr in imgs]
            entry[ename] = {'images': [strip(r) for r in res], 'combined': ev.combine_results(res)}
            print(name, ename, entry[ename]['combined'])
        doc['batches'][name] = entry
    # QuadMetric (batch size 1, the reference's requirement): box output with all-zero rows, polygon output (equal vertex
    # counts: the reference's np.array(output[0]) rejects ragged polygon lists)
    qm = QuadMetric()
    quad_cases = []
    gts = [rect(10, 10, 50, 30), rect(60, 10, 100, 30), rect(10, 60, 40, 90)]
    boxes = np.zeros((5, 4, 2), np.int16)
    boxes[0] = rect(11, 10, 50, 31)
    boxes[1] = rect(60, 12, 98, 30)
    quad_cases.append((gts, [False, False, True], boxes))
    quad_cases.append((gts, [False, True, False], [np.array(rect(10, 10, 50, 30)), np.array(rect(12, 62, 40, 90)),
                                                    np.array([(60, 10), (100, 10), (95, 32), (60, 30)])]))
    raws = []
    for anns, tags, out in quad_cases:
        batch = {'anns': [[(np.array([x]), np.array([y])) for x, y in a] for a in anns], 'ignore_tags': [np.array([t]) for t in tags]}
        raw = qm.validate_measure(batch, ([out], [np.ones(len(out))]))
        raws.append(raw)
        m = qm.gather_measure([raw])
        doc['quad'].append({'anns': [[list(p) for p in a] for a in anns], 'tags': tags, 'dets': [np.asarray(p).tolist() for p in out],
                            'images': [strip(r) for r in raw], 'measure': {k: [v.val, v.avg] for k, v in m.items()}})
        print('quad', doc['quad'][-1]['measure'])
    m = qm.gather_measure(raws)
    doc['quad_all'] = {k: [v.val, v.avg] for k, v in m.items()}
    print('quad all', doc['quad_all'])
    np.savez_compressed(os.path.join(HERE, 'eval_kats.npz'), json=np.array(json.dumps(doc)))


if __name__ == '__main__':
    main()
