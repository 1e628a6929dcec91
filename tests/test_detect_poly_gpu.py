"""GPU (-m gpu): detect_polygons (csrc/detect.hip dbn_detect_poly + dbn_detect_poly_host) against the test model
tests/detect_poly_ref.py. The device's compressed outer borders must equal the model's for every kept candidate, and so
must the final polygons and fp64 scores. Maps: odd sizes, 640², 1280², a 32 x 1280² batch, spiral, stripes across every
tile, checkerboard, all-ones / all-zeros, more dots than max_candidates. The fp64 score must round to the box path's
fp32 score, runs with poisoned workspaces must agree bit for bit, and SegDetectorRepresenter.polygons must work on a
DBTextModel output."""
import numpy as np
import pytest
import torch

from db_text_minimal_amd import DBTextModel
from db_text_minimal_amd import postprocess as P
import detect_poly_ref as M
from gpu_util import DEV
from test_detect_gpu import adversarial, as_pred, blobs, spiral

pytestmark = pytest.mark.gpu


def to_preds(maps):
    return torch.from_numpy(np.stack([np.stack([m, 1 - m]) for m in maps])).to(DEV)


def check_image(c, n, m, box_thresh=0.7, max_candidates=1000, dest_hw=None, res=None):
    """device contours of image n equal the model's; res (detect_poly_host's result), if given, equals the model's
    polygons and scores"""
    ref = M.polygons(m, 0.3, box_thresh, max_candidates, 1.5, dest_hw)
    assert c['counts'][n] == ref['count']
    K = len(ref['roots'])
    assert np.array_equal(c['recs'][n, :K]['root'], ref['roots'])
    for k in range(K):
        assert np.array_equal(P.contour_of(c, n, k), ref['contours'][k]), (n, k)
    assert (c['nv'][n, K:] == 0).all()
    if res is not None:
        polys, scores = res[n]
        assert ref['near'] == 0  # no scaled coordinate next to a rounding boundary on these fixtures
        assert scores == ref['scores'] and len(polys) == len(ref['polys'])
        for a, b in zip(polys, ref['polys']):
            assert a.dtype == np.int64 and np.array_equal(a, b)
    return ref


def run(maps, box_thresh=0.7, max_candidates=1000, prefill=None):
    c = P.detect_contours(to_preds(maps), 0.3, max_candidates, prefill=prefill)
    H, W = maps[0].shape
    info = c['info']
    assert info[0] == len(c['verts']) == c['nv'].sum() and 1 <= info[2] <= info[3]
    return c, P.detect_poly_host(c, H, W, box_thresh, 1.5)


@pytest.mark.parametrize('H,W,nb,seed', [(97, 131, 12, 10), (640, 640, 50, 12)])
def test_blobs_against_the_model(H, W, nb, seed):
    m = blobs(H, W, nb, seed)
    c, res = run([m])
    ref = check_image(c, 0, m, res=res)
    assert len(ref['polys']) >= nb // 3  # real polygons, not only skips


def test_one_1280_image():
    m = blobs(1280, 1280, 50, 3)
    c, res = run([m])
    check_image(c, 0, m, res=res)


def test_32_x_1280_batch_images_do_not_leak():
    a, b, d = blobs(1280, 1280, 50, 10), blobs(1280, 1280, 50, 5), blobs(1280, 1280, 40, 6)
    c, res = run([a, b] + [d] * 30)
    check_image(c, 0, a, res=res)
    check_image(c, 1, b, res=res)
    for n in range(3, 32):
        assert c['counts'][n] == c['counts'][2] and np.array_equal(c['nv'][n], c['nv'][2])
        for k in range(min(int(c['counts'][2]), 1000)):
            assert np.array_equal(P.contour_of(c, n, k), P.contour_of(c, 2, k))
        assert res[n][1] == res[2][1] and all(np.array_equal(x, y) for x, y in zip(res[n][0], res[2][0]))


@pytest.mark.parametrize('name', list(adversarial()))
def test_adversarial_maps(name):
    m = as_pred(adversarial()[name], seed=7)
    c, res = run([m], box_thresh=0.5)
    check_image(c, 0, m, box_thresh=0.5, res=res)


@pytest.mark.parametrize('H,W', [(150, 203), (640, 640)])
def test_clean_spiral_one_long_border(H, W):
    # without noise the corridor between the arms reaches the image edge: the outer border runs along both sides of
    # every arm, about H * W / 2 cracks in one cycle
    m = np.where(spiral(H, W), np.float32(0.9), np.float32(0.1)).astype(np.float32)
    c, res = run([m], box_thresh=0.5)
    ref = check_image(c, 0, m, box_thresh=0.5, res=res)
    assert len(ref['roots']) == 1 and len(ref['contours'][0]) > H + W
    assert c['info'][1] > H * W // 2 and c['info'][2] >= np.log2(H * W // 2)


def test_more_dots_than_max_candidates():
    H, W = 120, 160
    bm = np.zeros((H, W), bool)
    bm[1::4, 2::4] = True  # 1200 isolated dots
    bm[40:60, 50:110] = True  # and one real block
    bm[20:34, 10:40] = True
    m = np.where(bm, np.float32(0.9), np.float32(0.1)).astype(np.float32)  # no noise: the dots stay single pixels
    c, res = run([m], box_thresh=0.5, max_candidates=300)
    ref = check_image(c, 0, m, box_thresh=0.5, max_candidates=300, res=res)
    assert len(ref['roots']) == 300 and c['counts'][0] > 300
    assert all(len(x) == 1 for x in ref['contours'])  # the last 300 in raster order: single pixels, one vertex each


def test_detect_polygons_end_to_end_with_dest_sizes():
    maps = [blobs(160, 224, 14, 21), blobs(160, 224, 14, 22)]
    dest = [(480, 672), (120, 150)]
    res = P.detect_polygons(to_preds(maps), 0.3, 0.6, 1000, 1.5, dest)
    assert len(res) == 2
    for n in range(2):
        ref = M.polygons(maps[n], 0.3, 0.6, 1000, 1.5, dest[n])
        polys, scores = res[n]
        assert len(ref['polys']) >= 3  # (scale 0.75 meets exact halves: both sides round them to even in fp64)
        assert all(type(s) is float for s in scores) and scores == ref['scores']
        assert len(polys) == len(ref['polys']) and all(np.array_equal(a, b) for a, b in zip(polys, ref['polys']))
        for p in polys:  # the reference's consumers: make_eval.py filters on x.sum() > 0
            assert p.dtype == np.int64 and p.ndim == 2 and p.shape[1] == 2 and p.sum() > 0
            assert (p[:, 0] <= dest[n][1]).all() and (p[:, 1] <= dest[n][0]).all() and (p >= 0).all()


def test_score64_rounds_to_the_box_score():
    maps = [blobs(200, 300, 20, 31), as_pred(adversarial()['rings'], seed=3)]
    H, W = 200, 300
    maps[1] = np.pad(maps[1], ((0, H - maps[1].shape[0]), (0, W - maps[1].shape[1])))
    preds = to_preds(maps)
    c = P.detect_contours(preds, 0.3, 1000)
    _, info = P.detect_poly_host(c, H, W, 0.7, 1.5, return_info=True)
    recs, counts = P.detect_records(preds, 0.3, 1000)
    _, _, binfo = P.detect_host(recs, counts, H, W, 0.7, 1.5, return_info=True)
    assert recs.tobytes() == c['recs'].tobytes() and np.array_equal(counts, c['counts'])
    for n in range(2):
        K = min(int(counts[n]), 1000)
        assert K > 5
        assert np.array_equal(info['score64'][n, :K].astype(np.float32), binfo[n, :K, 9])


@pytest.mark.parametrize('prefill', [0x7F, 0x00])
def test_two_runs_bitwise_equal_with_poisoned_workspaces(prefill):
    maps = [blobs(200, 300, 20, 11), as_pred(spiral(200, 300), 9)]
    a = P.detect_contours(to_preds(maps), 0.3, 1000, prefill=0xFF)
    b = P.detect_contours(to_preds(maps), 0.3, 1000, prefill=prefill)
    for key in ('recs', 'counts', 'nv', 'voff', 'verts', 'info'):
        assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), key
    ra, rb = P.detect_poly_host(a, 200, 300), P.detect_poly_host(b, 200, 300)
    for (pa, sa), (pb, sb) in zip(ra, rb):
        assert sa == sb and all(np.array_equal(x, y) for x, y in zip(pa, pb))


def test_seg_detector_representer_polygons_on_model_output():
    torch.manual_seed(0)
    model = DBTextModel().to(DEV).eval()
    img = torch.randn(2, 3, 128, 160, device=DEV)
    with torch.no_grad():
        pred = model(img)
    torch.cuda.synchronize()
    rep = P.SegDetectorRepresenter(box_thresh=0.3)
    batch = {'shape': [(256, 320), (128, 160)]}
    boxes, scores = rep.polygons(batch, pred)
    maps = pred[:, 0].float().cpu().numpy()
    assert len(boxes) == 2 and len(scores) == 2
    for n in range(2):
        ref = M.polygons(maps[n], 0.3, 0.3, 1000, 1.5, batch['shape'][n])
        assert ref['near'] == 0
        assert scores[n] == ref['scores'] and len(boxes[n]) == len(ref['polys'])
        assert all(np.array_equal(a, b) for a, b in zip(boxes[n], ref['polys']))
    with pytest.raises(NotImplementedError):
        rep(batch, pred, is_output_polygon=True)
