"""CPU (-m "not gpu"): the detection scoring of csrc/det_eval.hip / det_eval.py without a GPU.

The exact overlap oracle (tests/eval_ref.py) against analytic cases; the device's boundary formula with its symbolic
perturbation, restated in Fractions, against the oracle EXACTLY on random pairs (a 0..4 integer grid forces shared edges,
vertices on edges, identical and self-touching polygons); the host matching call (dbn_det_eval_match_host through ctypes)
on oracle overlaps against the goldens the reference's own iou.py / deteval.py / QuadMetric produced
(tests/golden/eval_kats.npz); and the command line on pickles."""
import io
import json
import math
import os
import pickle
import random
from contextlib import redirect_stdout
from fractions import Fraction

import numpy as np
import pytest

from db_text_minimal_amd import det_eval as DE
import eval_ref as E

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'eval_kats.npz')


def rect(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def golden():
    return json.loads(str(np.load(GOLDEN)['json']))


def oracle_overlaps(gt_polys, det_polys):
    """polygon_overlaps' result from the exact oracle, each value rounded once to fp64"""
    out = []
    for gs, ds in zip(gt_polys, det_polys):
        out.append(dict(inter=np.array([[float(E.overlap_exact(g, d)) for d in ds] for g in gs], np.float64).reshape(len(gs), len(ds)),
                        gt_area=np.array([float(E.area_exact(g)) for g in gs], np.float64),
                        det_area=np.array([float(E.area_exact(d)) for d in ds], np.float64),
                        gt_nonsimple=np.array([not E.is_simple(g) for g in gs], bool),
                        det_nonsimple=np.array([not E.is_simple(d) for d in ds], bool)))
    return out


# ---- the oracle ----------------------------------------------------------------------------------------------------------

def test_oracle_analytic():
    sq = rect(0, 0, 2, 2)
    assert E.overlap_exact(sq, rect(1, 1, 3, 3)) == 1
    assert E.overlap_exact(sq, sq) == 4 and E.area_exact(sq) == 4
    assert E.overlap_exact(rect(0, 0, 10, 10), rect(2, 3, 5, 7)) == 12  # nested
    assert E.overlap_exact(sq, rect(2, 0, 4, 2)) == 0  # touching along an edge
    assert E.overlap_exact(sq, rect(2, 2, 4, 4)) == 0  # touching at a corner
    assert E.overlap_exact(sq, rect(5, 5, 6, 6)) == 0  # disjoint
    assert E.overlap_exact(sq[::-1], rect(1, 1, 3, 3)) == 1  # orientation does not matter
    assert E.overlap_exact(sq, rect(1, 0, 3, 2)[::-1]) == 2  # a shared edge in the same direction, the other reversed
    assert E.overlap_exact(rect(0, 0, 2, 1), rect(0, 1, 2, 2)) == 0  # shared edge, opposite directions
    # a square rotated by 45 degrees inside the axis square of the same centre, and its halves and corners
    diamond = [(1, 0), (2, 1), (1, 2), (0, 1)]
    assert E.overlap_exact(diamond, sq) == 2
    assert E.overlap_exact(diamond, rect(1, 0, 2, 2)) == 1
    assert E.overlap_exact(diamond, rect(0, 0, 1, 1)) == Fraction(1, 2)


def test_oracle_combs():
    """two interleaved combs: many crossings, the overlap is the sum of the tooth intersections"""
    def comb(n, x0):
        pts = [(x0, 0)]
        for i in range(n):
            pts += [(x0 + 2 * i, 10), (x0 + 2 * i + 1, 10), (x0 + 2 * i + 1, 1), (x0 + 2 * i + 2, 1)]
        pts += [(x0 + 2 * n, 0)]
        return pts
    A = comb(4, 0)
    B = [(x, 11 - y) for x, y in comb(4, 0)][::-1]  # upside down: teeth from y = 11 down to 1
    assert E.is_simple(A) and E.is_simple(B)
    # A's teeth [2i, 2i + 1] x [1, 10] and its base [0, 8] x [0, 1]; B's teeth the same columns from 1 to 10, base [10, 11]
    assert E.overlap_exact(A, B) == 4 * 9
    assert E.overlap_boundary(A, B) == 4 * 9
    C = [(x + Fraction(1, 2), y) for x, y in B]  # shifted half a tooth: each tooth overlaps half of one
    assert E.overlap_exact(A, C) == E.overlap_boundary(A, C) == 18


def test_oracle_bowtie():
    """a bow-tie: winding +1 in one lobe and -1 in the other (signed area 0, so it keeps its orientation)"""
    bow = [(0, 0), (2, 2), (2, 0), (0, 2)]
    assert not E.is_simple(bow)
    assert E.signed_area2(bow) == 0
    left, right = E.overlap_exact(bow, rect(0, 0, 1, 2)), E.overlap_exact(bow, rect(1, 0, 2, 2))
    assert abs(left) == 1 and abs(right) == 1 and left == -right
    assert E.overlap_exact(bow, rect(0, 0, 2, 2)) == 0


def test_is_simple():
    assert E.is_simple(rect(0, 0, 1, 1))
    assert E.is_simple(rect(0, 0, 1, 1) + [(0, 0)])  # a closing duplicate is a zero-length edge
    assert not E.is_simple([(0, 0), (2, 0), (1, 0), (1, 1)])  # adjacent edges overlap collinearly
    assert not E.is_simple([(0, 0), (4, 0), (4, 4), (2, 0), (0, 4)])  # a vertex on a non-adjacent edge
    assert not E.is_simple([(0, 0), (1, 0), (2, 0)])
    assert E.is_simple([(0, 0), (1, 0), (2, 0), (2, 1)])  # collinear, same direction: fine


def _rand_poly(rng, n, grid):
    if grid:
        return [(rng.randint(0, grid), rng.randint(0, grid)) for _ in range(n)]
    return [(rng.uniform(0, 10), rng.uniform(0, 10)) for _ in range(n)]


@pytest.mark.parametrize('grid', [4, None])
def test_boundary_formula_equals_oracle(grid):
    """the device's formula with the symbolic perturbation, restated in Fractions, equals the slab oracle exactly"""
    rng = random.Random(11 if grid else 12)
    for i in range(150):
        A, B = _rand_poly(rng, rng.randint(3, 6), grid), _rand_poly(rng, rng.randint(3, 6), grid)
        if i % 10 == 0:
            B = list(A) if i % 20 == 0 else A[1:] + A[:1]
        assert E.overlap_boundary(A, B) == E.overlap_exact(A, B), (A, B)


# ---- host matching against the reference's goldens -------------------------------------------------------------------------

EVALUATORS = {'iou': lambda: DE.DetectionIoUEvaluator(), 'deteval': lambda: DE.DetectionDetEvalEvaluator(),
              'iou_04_08': lambda: DE.DetectionIoUEvaluator(iou_constraint=0.4, area_precision_constraint=0.8)}


def _check_image(got, ref, deteval):
    for k in ('precision', 'recall', 'hmean'):
        assert float(got[k]) == float(ref[k]), (k, got[k], ref[k])
    for k in ('gtCare', 'detCare', 'gtDontCare', 'detDontCare'):
        assert got[k] == ref[k], (k, got[k], ref[k])
    assert got['pairs'] == ref['pairs']
    if deteval:
        assert float(got['recallAccum']) == float(ref['recallAccum']) and float(got['precisionAccum']) == float(ref['precisionAccum'])
        assert len(got['recallMat']) == len(ref['recallMat'])
    else:
        assert got['detMatched'] == ref['detMatched']
        assert len(got['iouMat']) == len(ref['iouMat'])


@pytest.mark.parametrize('batch', ['random_int', 'random_float', 'kats'])
@pytest.mark.parametrize('ename', list(EVALUATORS))
def test_host_matching_reproduces_golden(batch, ename):
    b = golden()['batches'][batch]
    ov = oracle_overlaps([[g['points'] for g in gt] for gt in b['gts']], [[p['points'] for p in pr] for pr in b['preds']])
    ev = EVALUATORS[ename]()
    res = ev.evaluate_batch(b['gts'], b['preds'], overlaps=ov)
    ref = b[ename]
    assert len(res) == len(ref['images'])
    for n, (got, r) in enumerate(zip(res, ref['images'])):
        _check_image(got, r, ename == 'deteval')
        if b['preds'][n] and (ename == 'deteval' or b['gts'][n]):  # (elsewhere the reference's matrix is np.empty's)
            if ename == 'deteval':  # inter / area: the same fp64 division
                assert got['recallMat'] == r['recallMat'] and got['precisionMat'] == r['precisionMat'], n
            else:  # the union is area_g + area_d - inter here, the exact union rounded once there
                assert np.allclose(np.array(got['iouMat']), np.array(r['iouMat']), rtol=1e-14, atol=0), n
    assert ev.combine_results(res) == ref['combined']


def test_round4_tie_decides():
    """DetEval's one-to-many sum at the decimal tie 0.79995: round(sum, 4) on the binary value decides"""
    r = golden()['batches']['kats']['deteval']['images']
    assert r[-2]['pairs'] == [{'gt': 0, 'det': [0, 1], 'type': 'OM'}] and r[-1]['pairs'] == []
    assert round(0.79995, 4) == 0.8 and round(float(np.nextafter(0.79995, 0)), 4) == 0.7999


class _OracleIoU(DE.DetectionIoUEvaluator):
    def evaluate_batch(self, gts, preds, overlaps=None, device=None):
        ov = oracle_overlaps([[g['points'] for g in gt] for gt in gts], [[p['points'] for p in pr] for pr in preds])
        return super().evaluate_batch(gts, preds, overlaps=ov)


def test_quad_metric_golden():
    doc = golden()
    qm = DE.QuadMetric(_OracleIoU())
    raws = []
    for case in doc['quad']:
        dets = [np.array(d) for d in case['dets']]
        if len(dets) == 5:  # the box path: an int16 [K, 4, 2] array with all-zero rows
            dets = np.array(case['dets'], np.int16)
        batch = {'anns': [[np.array(a) for a in case['anns']]], 'ignore_tags': [case['tags']]}
        raw = qm.validate_measure(batch, ([dets], [np.ones(len(dets))]))
        raws.append(raw)
        for got, ref in zip(raw, case['images']):
            _check_image(got, ref, False)
        m = qm.gather_measure([raw])
        assert {k: [v.val, v.avg] for k, v in m.items()} == case['measure']
    m = qm.gather_measure(raws)
    assert {k: [v.val, v.avg] for k, v in m.items()} == doc['quad_all']


def test_quad_metric_scores_every_image():
    """a batch of two images scores both (the reference: image 0 only): the counts add up"""
    doc = golden()
    qm = DE.QuadMetric(_OracleIoU())
    a, b = doc['quad']
    batch = {'anns': [[np.array(x) for x in a['anns']], [np.array(x) for x in b['anns']]], 'ignore_tags': [a['tags'], b['tags']]}
    raw = qm.validate_measure(batch, ([np.array(a['dets'], np.int16), [np.array(d) for d in b['dets']]], [None, None]))
    assert len(raw) == 2
    m = qm.gather_measure([raw])
    assert {k: [v.val, v.avg] for k, v in m.items()} == doc['quad_all']


def test_matching_restatement_agrees():
    """tests/eval_ref.py's protocol restatements agree with the host call on the golden batches"""
    b = golden()['batches']['random_float']
    gp = [[g['points'] for g in gt] for gt in b['gts']]
    dp = [[p['points'] for p in pr] for pr in b['preds']]
    ov = oracle_overlaps(gp, dp)
    for n, o in enumerate(ov):
        ig = [g['ignore'] for g in b['gts'][n]]
        r1 = E.iou_image(o['inter'].tolist(), o['gt_area'].tolist(), o['det_area'].tolist(), ig)
        r2 = E.deteval_image(o['inter'].tolist(), o['gt_area'].tolist(), o['det_area'].tolist(), ig, [E.centre_diag(p) for p in gp[n]],
                             [E.centre_diag(p) for p in dp[n]])
        for r, ref in ((r1, b['iou']['images'][n]), (r2, b['deteval']['images'][n])):
            for k in r:
                assert r[k] == ref[k], (n, k)


@pytest.mark.parametrize('protocol,flags,ename', [('iou', [], 'iou'), ('deteval', [], 'deteval'),
                                                  ('iou', ['--iou', '0.4', '--area', '0.8'], 'iou_04_08')])
def test_cli_on_pickles(tmp_path, protocol, flags, ename):
    b = golden()['batches']['kats']
    gts = [[{'points': [tuple(p) for p in g['points']], 'text': 'x', 'ignore': g['ignore']} for g in gt] for gt in b['gts']]
    preds = [[{'points': [tuple(p) for p in d['points']], 'text': 'x', 'ignore': False} for d in pr] for pr in b['preds']]
    gf, pf = tmp_path / 'gts.pkl', tmp_path / 'preds.pkl'
    gf.write_bytes(pickle.dumps(gts))
    pf.write_bytes(pickle.dumps(preds))
    buf = io.StringIO()
    with redirect_stdout(buf):
        m = DE.main([protocol] + flags + ['--poly_gts_fp', str(gf), '--poly_preds_fp', str(pf)], overlaps_fn=oracle_overlaps)
    assert m == b[ename]['combined']
    assert buf.getvalue().strip() == str(b[ename]['combined'])


def test_python_round_restatement():
    """py_round4 of the host call is Python's round(x, 4): exercised through one-to-many sums at and around ties"""
    for x in (0.79995, 0.80005, 0.39995, 0.40005, 0.7999500000000001, 1.00005, 0.12345):
        assert (round(x, 4) >= 0.8) == (float('%.4f' % x) >= 0.8)
        assert round(x, 4) == float('%.4f' % x)
    assert not math.isnan(round(1e300, 4))
