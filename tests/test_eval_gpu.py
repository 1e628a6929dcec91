"""GPU (-m gpu): detection scoring (csrc/det_eval.hip dbn_det_eval_overlaps, det_eval.py) against the exact oracle of
tests/eval_ref.py and the reference's goldens (tests/golden/eval_kats.npz).

The device overlap matrix must lie within 1e-12 of the larger area of the exact overlap on random batches (integer and
float), equal it exactly for axis-aligned integer rectangles and for a polygon against itself, be symmetric under swapping
GT and detections and independent of orientation; the non-simple flags must equal the oracle's test; a polygon of more
vertices than one LDS chunk must work; two runs on poisoned workspaces must agree bit for bit.  evaluate_batch must
reproduce the goldens, a GT map used as the prediction must score P = R = H = 1 end to end, and fit(detection=...) must
record the test HMean and save its best checkpoint."""
import os
import pickle
import random
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

from db_text_minimal_amd import det_eval as DE
from db_text_minimal_amd.gt_maps import make_gt_maps
from db_text_minimal_amd.postprocess import detect_polygons
import eval_ref as E
from gpu_util import DEV
from test_eval_cpu import EVALUATORS, _check_image, golden, rect

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def star(rng, cx, cy, r, n, integer):
    angs = sorted(rng.uniform(0, 2 * np.pi) for _ in range(n))
    pts = [(cx + r * rng.uniform(0.4, 1.0) * np.cos(a), cy + r * rng.uniform(0.4, 1.0) * np.sin(a)) for a in angs]
    if integer:
        pts = [(int(round(x)), int(round(y))) for x, y in pts]
    return pts[::-1] if rng.random() < 0.3 else pts


def random_batch(rng, integer, N=3, G=4, D=5):
    gts, dets = [], []
    for _ in range(N):
        gts.append([star(rng, rng.uniform(10, 50), rng.uniform(10, 50), rng.uniform(5, 20), rng.randint(3, 7), integer) for _ in range(G)])
        dets.append([star(rng, rng.uniform(10, 50), rng.uniform(10, 50), rng.uniform(5, 20), rng.randint(3, 7), integer) for _ in range(D)])
    return gts, dets


@pytest.mark.parametrize('integer', [True, False])
def test_overlaps_match_oracle(integer):
    rng = random.Random(5 if integer else 6)
    gts, dets = random_batch(rng, integer)
    ov = DE.polygon_overlaps(gts, dets, DEV)
    for n in range(len(gts)):
        o = ov[n]
        for g, A in enumerate(gts[n]):
            assert o['gt_area'][g] == pytest.approx(float(E.area_exact(A)), rel=1e-12, abs=0)
            assert bool(o['gt_nonsimple'][g]) == (not E.is_simple(A))
            for d, B in enumerate(dets[n]):
                ref = E.overlap_exact(A, B)
                scale = max(E.area_exact(A), E.area_exact(B))
                assert abs(Fraction(o['inter'][g, d]) - ref) <= Fraction(1, 10**12) * scale, (n, g, d, o['inter'][g, d], float(ref))
        for d, B in enumerate(dets[n]):
            assert bool(o['det_nonsimple'][d]) == (not E.is_simple(B))


def test_degenerate_grid_and_flags():
    """polygons on a 0..4 integer grid: shared edges, vertices on edges, identical and non-simple polygons; every overlap is
    checked against the oracle, the flags against its simplicity test"""
    rng = random.Random(9)
    polys = [[(rng.randint(0, 4), rng.randint(0, 4)) for _ in range(rng.randint(3, 6))] for _ in range(24)]
    polys = [p for p in polys if len(set(p)) >= 1]
    gts, dets = [polys[:12]], [polys[12:] + polys[:3]]
    o = DE.polygon_overlaps(gts, dets, DEV)[0]
    for g, A in enumerate(gts[0]):
        assert bool(o['gt_nonsimple'][g]) == (not E.is_simple(A)), A
        for d, B in enumerate(dets[0]):
            ref = E.overlap_exact(A, B)
            assert abs(Fraction(o['inter'][g, d]) - ref) <= Fraction(1, 10**12) * 16, (A, B, o['inter'][g, d], float(ref))
    assert o['gt_nonsimple'].any() and not o['gt_nonsimple'].all()


def test_axis_aligned_integer_exact_and_symmetric():
    rng = random.Random(3)
    rs = []
    for _ in range(40):
        x0, y0 = rng.randint(0, 30), rng.randint(0, 30)
        rs.append(rect(x0, y0, x0 + rng.randint(1, 15), y0 + rng.randint(1, 15)))
        if rng.random() < 0.4:
            rs[-1] = rs[-1][::-1]
    gts, dets = [rs[:20]], [rs[20:] + rs[:5]]
    o = DE.polygon_overlaps(gts, dets, DEV)[0]
    ref = np.array([[float(E.overlap_exact(A, B)) for B in dets[0]] for A in gts[0]])
    assert np.array_equal(o['inter'], ref)
    sw = DE.polygon_overlaps(dets, gts, DEV)[0]
    assert np.array_equal(sw['inter'], o['inter'].T)
    # against itself: overlap(A, A) == area(A), exactly for integer polygons of any shape
    rng = random.Random(4)
    ps = [star(rng, 50, 50, 30, rng.randint(3, 12), True) for _ in range(10)] + rs[:5]
    s = DE.polygon_overlaps([ps], [ps], DEV)[0]
    assert np.array_equal(np.diag(s['inter']), s['gt_area'])
    assert np.array_equal(s['gt_area'], np.array([float(E.area_exact(p)) for p in ps]))


def test_orientation_and_swap_independent():
    rng = random.Random(8)
    gts, dets = random_batch(rng, False, N=2)
    a = DE.polygon_overlaps(gts, dets, DEV)
    b = DE.polygon_overlaps([[p[::-1] for p in x] for x in gts], [[p[::-1] for p in x] for x in dets], DEV)
    c = DE.polygon_overlaps(dets, gts, DEV)
    for n in range(2):
        scale = np.maximum(a[n]['gt_area'][:, None], a[n]['det_area'][None, :])
        assert (np.abs(a[n]['inter'] - b[n]['inter']) <= 1e-12 * scale).all()
        assert (np.abs(a[n]['inter'] - c[n]['inter'].T) <= 1e-12 * scale).all()


def _clip_left(P, c):
    """exact area of polygon P (simple) left of x = c (Sutherland-Hodgman on one half-plane, Fractions)"""
    P = E.fr(P)
    out = []
    for i in range(len(P)):
        p, q = P[i], P[(i + 1) % len(P)]
        pin, qin = p[0] <= c, q[0] <= c
        if pin:
            out.append(p)
        if pin != qin:
            t = (c - p[0]) / (q[0] - p[0])
            out.append((c, p[1] + t * (q[1] - p[1])))
    return E.area_exact(out) if len(out) >= 3 else Fraction(0)


def test_polygon_longer_than_one_chunk():
    """a 700-vertex star-shaped polygon (more than one 256-vertex LDS chunk, in both roles) against half-planes and itself"""
    n = 700
    ang = np.linspace(0, 2 * np.pi, n, endpoint=False)
    rad = 300 + 100 * np.sin(7 * ang)
    big = [(int(round(1000 + r * np.cos(a))), int(round(1000 + r * np.sin(a)))) for r, a in zip(rad, ang)]
    cuts = [rect(0, 0, c, 2000) for c in (700, 1000, 1234)]
    o = DE.polygon_overlaps([[big]], [cuts + [big]], DEV)[0]
    for k, c in enumerate((700, 1000, 1234)):
        assert abs(Fraction(o['inter'][0, k]) - _clip_left(big, c)) <= Fraction(1, 10**12) * E.area_exact(big), k
    assert o['inter'][0, 3] == o['gt_area'][0] == float(E.area_exact(big))
    assert not o['gt_nonsimple'][0]
    sw = DE.polygon_overlaps([cuts], [[big]], DEV)[0]
    assert np.allclose(sw['inter'][:, 0], o['inter'][0, :3], rtol=1e-12, atol=0)


def test_poisoned_workspace_bitwise():
    rng = random.Random(12)
    gts, dets = random_batch(rng, False, N=4, G=6, D=7)
    a = DE.polygon_overlaps(gts, dets, DEV, prefill=0x00)
    b = DE.polygon_overlaps(gts, dets, DEV, prefill=0xFF)
    for x, y in zip(a, b):
        for k in x:
            assert np.array_equal(x[k].view(np.uint8), y[k].view(np.uint8)), k


@pytest.mark.parametrize('batch', ['random_int', 'random_float', 'kats'])
@pytest.mark.parametrize('ename', list(EVALUATORS))
def test_evaluate_batch_reproduces_golden(batch, ename):
    b = golden()['batches'][batch]
    ev = EVALUATORS[ename]()
    res = ev.evaluate_batch(b['gts'], b['preds'], device=DEV)
    for got, ref in zip(res, b[ename]['images']):
        _check_image(got, ref, ename == 'deteval')
    assert ev.combine_results(res) == b[ename]['combined']
    # one image at a time: the same
    one = [ev.evaluate_image(g, p) for g, p in zip(b['gts'], b['preds'])]
    assert [(r['precision'], r['recall'], r['pairs']) for r in one] == [(r['precision'], r['recall'], r['pairs']) for r in res]


def test_cli_on_pickles(tmp_path):
    b = golden()['batches']['kats']
    gf, pf = tmp_path / 'gts.pkl', tmp_path / 'preds.pkl'
    gf.write_bytes(pickle.dumps(b['gts']))
    pf.write_bytes(pickle.dumps(b['preds']))
    for args, key in ((['iou'], 'iou'), (['deteval'], 'deteval'), (['iou', '--iou', '0.4', '--area', '0.8'], 'iou_04_08')):
        out = subprocess.run([sys.executable, '-m', 'db_text_minimal_amd.det_eval'] + args + ['--poly_gts_fp', str(gf), '--poly_preds_fp', str(pf)],
                             cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        assert out.stdout.strip().splitlines()[-1] == str(b[key]['combined'])


def _text_rects(n_img, S=128):
    rng = random.Random(17)
    polys = []
    for _ in range(n_img):
        ps = []
        for k in range(4):
            x0, y0 = 8 + 60 * (k % 2) + rng.randint(0, 6), 8 + 60 * (k // 2) + rng.randint(0, 6)
            ps.append(np.array(rect(x0, y0, x0 + rng.randint(36, 48), y0 + rng.randint(20, 30)), np.float64))
        polys.append(ps)
    return polys


def test_end_to_end_perfect_prediction():
    """GT polygons -> make_gt_maps' prob map as the prediction -> detect_polygons -> QuadMetric: P = R = H = 1; a map
    without one GT gives recall (G - 1) / G"""
    S = 128
    polys = _text_rects(3, S)
    maps = make_gt_maps(polys, None, S, DEV)
    preds = torch.stack([maps[0], 1 - maps[0]], dim=1).contiguous()
    res = detect_polygons(preds, thresh=0.25, box_thresh=0.5, unclip_ratio=1.5)
    qm = DE.QuadMetric()
    batch = {'anns': polys, 'ignore_tags': [[False] * len(p) for p in polys]}
    raw = qm.validate_measure(batch, ([p for p, _ in res], [s for _, s in res]), is_output_polygon=True)
    m = qm.gather_measure([raw])
    assert m['precision'].avg == 1 and m['recall'].avg == 1 and m['fmeasure'].avg == pytest.approx(1, abs=1e-8)
    G = sum(len(p) for p in polys)
    dropped = [p[1:] if i == 0 else p for i, p in enumerate(polys)]
    maps2 = make_gt_maps(dropped, None, S, DEV)
    res2 = detect_polygons(torch.stack([maps2[0], 1 - maps2[0]], dim=1).contiguous(), thresh=0.25, box_thresh=0.5, unclip_ratio=1.5)
    m2 = qm.gather_measure([qm.validate_measure(batch, ([p for p, _ in res2], [s for _, s in res2]))])
    assert m2['recall'].avg == (G - 1) / G and m2['precision'].avg == 1


def test_fit_with_detection(tmp_path):
    from db_text_minimal_amd import DBLoss, DBTextModel, FusedAdam
    from db_text_minimal_amd.train import evaluate, fit
    from oracle import dbnet_oracle as O
    S = 64

    def loader(n, base):
        out = []
        for i in range(n):
            img, _ = O.synthetic_batch(2, S, seed=base + i)
            polys = [[np.array(rect(4, 6, 40, 20), np.float64), np.array(rect(10, 34, 56, 52), np.float64)]] * 2
            maps = make_gt_maps(polys, None, S, DEV)
            out.append({'img': img, 'prob_map': maps[0], 'supervision_mask': maps[1], 'thresh_map': maps[2], 'text_area_map': maps[3],
                        'anns': polys, 'ignore_tags': [[False, False]] * 2})
        return out

    def model():
        m = DBTextModel()
        m.load_state_dict(O.new_state(7))
        return m.to(DEV).train()

    train_loader, test_loader = loader(2, 300), loader(2, 400)
    m = model()
    best = str(tmp_path / 'best_hmean.pth')
    hist = fit(m, DBLoss(), FusedAdam(m, lr=0.005), train_loader, test_loader, epochs=2, device=DEV, detection={'protocol': 'iou'},
               best_hmean_cp_path=best)
    assert all('test_hmean' in h and 'test_precision' in h and 'test_recall' in h for h in hist)
    assert all(0 <= h['test_hmean'] <= 1 for h in hist)
    assert hist[0].get('saved_best_hmean') and os.path.exists(best)
    m2 = model()
    plain = fit(m2, DBLoss(), FusedAdam(m2, lr=0.005), train_loader, test_loader, epochs=1, device=DEV)
    assert set(plain[0]) == set(hist[0]) - {'test_hmean', 'test_precision', 'test_recall', 'saved_best_hmean'}
    loss, score = evaluate(m, DBLoss(), test_loader, device=DEV, detection=True)
    assert set(score) >= {'precision', 'recall', 'hmean'}
    assert set(evaluate(m, DBLoss(), test_loader, device=DEV)[1]) == set(score) - {'precision', 'recall', 'hmean'}
