"""GPU (-m gpu): detect_boxes (csrc/detect.hip + the host stage) against the test model tests/detect_ref.py: labels, the
candidate list, R1 corners, scores and final int16 boxes, on odd sizes, 640^2, 1280^2, a 32 x 1280^2 batch and
adversarial maps (spirals, stripes across every tile, checkerboard, all-ones / all-zeros, more dots than
max_candidates); determinism with poisoned workspaces; SegDetectorRepresenter on a DBTextModel output."""
import math

import numpy as np
import pytest
import torch

from db_text_minimal_amd import DBTextModel
from db_text_minimal_amd import postprocess as P
import detect_ref as R
from gpu_util import DEV

pytestmark = pytest.mark.gpu


def blobs(H, W, n, seed):
    """probability map with n rotated text-like blobs: values 0.75..1 inside, 0..0.28 outside, some blobs touching."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    inside = np.zeros((H, W), bool)
    for _ in range(n):
        cx, cy = rng.uniform(0, W), rng.uniform(0, H)
        a = rng.uniform(0, math.pi)
        L, T = rng.uniform(3, max(4, W / 8)), rng.uniform(1.5, max(2, H / 40))
        u = (xx - cx) * math.cos(a) + (yy - cy) * math.sin(a)
        v = -(xx - cx) * math.sin(a) + (yy - cy) * math.cos(a)
        inside |= (np.abs(u) <= L) & (np.abs(v) <= T)
    lo = rng.uniform(0, 0.28, (H, W)).astype(np.float32)
    hi = rng.uniform(0.75, 1.0, (H, W)).astype(np.float32)
    return np.where(inside, hi, lo).astype(np.float32)


def spiral(H, W):
    """one rectangular spiral, arms two pixels apart, from the top-left corner inwards."""
    bm = np.zeros((H, W), bool)
    y, x = 0, 0
    t, l, b, r = 0, 0, H - 1, W - 1
    while t <= b and l <= r:
        bm[y, x:r + 1] = True
        x = r
        bm[y:b + 1, x] = True
        y = b
        bm[y, l:x + 1] = True
        x = l
        if y > t + 2:
            bm[t + 2:y + 1, x] = True
            y = t + 2
        t, l, b, r = t + 2, l + 2, b - 2, r - 2
    return bm


def as_pred(bm, seed=0):
    rng = np.random.default_rng(seed)
    return np.where(bm, rng.uniform(0.75, 1.0, bm.shape), rng.uniform(0, 0.35, bm.shape)).astype(np.float32)


def run(maps, **kw):
    """maps: list of [H, W] fp32 -> (records, counts, labels np, boxes, scores, info)"""
    preds = torch.from_numpy(np.stack([np.stack([m, 1 - m]) for m in maps])).to(DEV)
    M = kw.get('max_candidates', 1000)
    recs, counts, labels = P.detect_records(preds, kw.get('thresh', 0.3), M, return_labels=True, prefill=kw.get('prefill'))
    H, W = maps[0].shape
    boxes, scores, info = P.detect_host(recs, counts, H, W, kw.get('box_thresh', 0.7), 1.5, None, return_info=True)
    return recs, counts, labels.cpu().numpy(), boxes, scores, info


def ulps(a, b):
    ia, ib = np.asarray(a, np.float32).view(np.int32).astype(np.int64), np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return int(np.abs(ia - ib).max()) if ia.size else 0


def check_image(got, n, m, box_thresh=0.7, max_candidates=1000):
    recs, counts, labels, boxes, scores, info = got
    ref = R.detect(m, 0.3, box_thresh, max_candidates)
    assert np.array_equal(labels[n], ref['labels'])
    assert counts[n] == ref['count']
    K = len(ref['roots'])
    assert np.array_equal(recs[n, :K]['root'], ref['roots'])
    assert (recs[n, :K]['hull_n'] > 0).all()
    assert np.abs(info[n, :K, :8].reshape(K, 4, 2) - ref['r1']).max(initial=0) <= 1e-4
    assert ulps(info[n, :K, 9], ref['score']) <= 1
    assert ref['near'] == 0  # no final coordinate within 1e-3 of a rounding boundary on these fixtures
    assert np.array_equal(boxes[n, :K], ref['boxes'])
    assert np.array_equal(scores[n, :K], ref['scores'])
    return ref


@pytest.mark.parametrize('H,W,nb,seed', [(97, 131, 12, 10), (640, 640, 50, 12)])
def test_blobs_against_the_model(H, W, nb, seed):
    m = blobs(H, W, nb, seed)
    ref = check_image(run([m]), 0, m)
    assert (ref['scores'] > 0).sum() >= nb // 3  # real boxes, not only skips


def test_one_1280_image():
    m = blobs(1280, 1280, 50, 3)
    check_image(run([m]), 0, m)


def test_32_x_1280_batch_images_do_not_leak():
    a, b, c = blobs(1280, 1280, 50, 10), blobs(1280, 1280, 50, 5), blobs(1280, 1280, 40, 6)
    got = run([a, b] + [c] * 30)
    check_image(got, 0, a)
    check_image(got, 1, b)
    recs, counts, labels, boxes, scores, info = got
    for n in range(3, 32):
        assert np.array_equal(labels[n], labels[2]) and counts[n] == counts[2]
        assert recs[n].tobytes() == recs[2].tobytes() and np.array_equal(boxes[n], boxes[2]) and np.array_equal(scores[n], scores[2])


def adversarial():
    H, W = 150, 203  # neither a multiple of the 64 x 16 tile nor of 4
    yy, xx = np.mgrid[0:H, 0:W]
    cases = {
        'spiral': spiral(H, W),
        'hstripes': (yy % 3) == 0,
        'vstripes': (xx % 4) < 2,
        'dstripes': ((xx + yy) % 5) < 2,
        'checker': ((xx + yy) % 2) == 0,
        'ones': np.ones((H, W), bool),
        'zeros': np.zeros((H, W), bool),
        'rings': (np.maximum(np.abs(yy - 75), np.abs(xx - 100)) % 4) == 0,
    }
    return cases


@pytest.mark.parametrize('name', list(adversarial()))
def test_adversarial_maps(name):
    m = as_pred(adversarial()[name], seed=7)
    check_image(run([m], box_thresh=0.5), 0, m, box_thresh=0.5)


def test_more_dots_than_max_candidates():
    H, W = 120, 160
    bm = np.zeros((H, W), bool)
    bm[1::4, 2::4] = True  # 30 x 40 = 1200 isolated dots
    bm[40:60, 50:110] = True  # and one real block
    m = as_pred(bm, seed=8)
    got = run([m], max_candidates=300, box_thresh=0.5)
    ref = check_image(got, 0, m, box_thresh=0.5, max_candidates=300)
    assert len(ref['roots']) == 300 and got[1][0] > 300
    assert (np.diff(ref['roots']) < 0).all()  # descending raster order: the last rows' dots are kept


@pytest.mark.parametrize('prefill', [0xFF, 0x7F, 0x00])
def test_two_runs_bitwise_equal_with_poisoned_workspaces(prefill):
    maps = [blobs(200, 300, 20, 11), as_pred(spiral(200, 300), 9)]
    a = run(maps, prefill=0xFF)
    b = run(maps, prefill=prefill)
    for x, y in zip(a, b):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


def test_seg_detector_representer_on_model_output():
    torch.manual_seed(0)
    model = DBTextModel().to(DEV).eval()
    img = torch.randn(2, 3, 128, 160, device=DEV)
    with torch.no_grad():
        pred = model(img)
    torch.cuda.synchronize()
    rep = P.SegDetectorRepresenter(box_thresh=0.3)
    batch = {'shape': [(256, 320), (128, 160)]}
    boxes, scores = rep(batch, pred)
    maps = pred[:, 0].float().cpu().numpy()
    assert len(boxes) == 2
    for n in range(2):
        ref = R.detect(maps[n], 0.3, 0.3, 1000, 1.5, batch['shape'][n])
        assert ref['near'] == 0
        assert boxes[n].dtype == np.int16 and scores[n].dtype == np.float32
        assert np.array_equal(boxes[n], ref['boxes']) and np.array_equal(scores[n], ref['scores'])
    with pytest.raises(NotImplementedError):
        rep(batch, pred, is_output_polygon=True)
