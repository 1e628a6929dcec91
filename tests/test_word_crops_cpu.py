"""CPU: the host maps of db_text_minimal_amd.word_crops (dbn_perspective_maps) against the scalar restatement
tests/crop_ref.py bit for bit and against numpy's solver, the restatement itself on crops with a known answer, and the
argument checks of crop_words (they raise before any launch)."""
import numpy as np
import pytest
import torch

from db_text_minimal_amd import crop_words, perspective_maps
from db_text_minimal_amd.word_crops import select_boxes
import crop_ref as R


def rotated_boxes(rng, n, integer=True):
    """n rotated rectangles, 20-400 x 8-60 px around centres in [100, 1200]^2, corners jittered by up to 3 px; in the
    corner order of detect_boxes (top-left first, clockwise on screen) up to the rotation"""
    c = rng.uniform(100, 1200, (n, 2))
    w, h, a = rng.uniform(20, 400, n), rng.uniform(8, 60, n), rng.uniform(-np.pi, np.pi, n)
    base = np.stack([np.stack([-w, -h], 1), np.stack([w, -h], 1), np.stack([w, h], 1), np.stack([-w, h], 1)], 1) / 2
    ca, sa = np.cos(a)[:, None], np.sin(a)[:, None]
    q = np.stack([base[..., 0] * ca - base[..., 1] * sa, base[..., 0] * sa + base[..., 1] * ca], -1) + c[:, None, :]
    q = q + rng.uniform(-3, 3, (n, 4, 2))
    return np.round(q).astype(np.float32) if integer else q.astype(np.float32)


def degenerate_quads(rng):
    """collinear, repeated points, zero area, nearly singular, sub-pixel"""
    out = [
        [[0, 0], [1, 1], [2, 2], [3, 3]],            # collinear
        [[5, 5], [5, 5], [5, 5], [5, 5]],            # one point
        [[0, 0], [10, 0], [10, 0], [0, 0]],          # a segment twice
        [[0, 0], [10, 0], [10, 10], [10, 10]],       # a repeated corner (a triangle)
        [[0, 0], [10, 0], [0, 10], [10, 10]],        # self-crossing (bow tie)
        [[0, 0], [0, 0], [0, 0], [1, 0]],
        [[3, 4], [3.25, 4], [3.25, 4.5], [3, 4.5]],  # sub-pixel
        [[0, 0], [1e-3, 0], [1e-3, 1e-3], [0, 1e-3]],
        [[-32768, -32768], [32767, -32768], [32767, 32767], [-32768, 32767]],
        [[100, 100], [100, 200], [200, 200], [200, 100]],  # turned 90 degrees
    ]
    q = np.array(out, np.float32)
    return np.concatenate([q, rng.integers(-5, 5, (200, 4, 2)).astype(np.float32)])  # many degenerate small-integer quads


def _system(q, h, w):
    x = q.astype(np.float64)
    u, v = np.array([0, w, w, 0.]), np.array([0, 0, h, h], np.float64)
    A = np.zeros((8, 8))
    for j in range(4):
        A[j, :3] = A[j + 4, 3:6] = x[j, 0], x[j, 1], 1
        A[j, 6:] = -x[j, 0] * u[j], -x[j, 1] * u[j]
        A[j + 4, 6:] = -x[j, 0] * v[j], -x[j, 1] * v[j]
    return A, np.r_[u, v]


@pytest.mark.parametrize('size', [(32, 100), (17, 40), (1, 1), (64, 2000)])
def test_maps_bit_identical_to_restatement(size):
    rng = np.random.default_rng(size[0] * 7 + size[1])
    q = np.concatenate([rotated_boxes(rng, 300), rotated_boxes(rng, 300, integer=False), degenerate_quads(rng),
                        rng.uniform(-2000, 2000, (300, 4, 2)).astype(np.float32)])
    fwd, inv = perspective_maps(q, size)
    fr, ir = R.maps(q, *size)
    assert fwd.dtype == np.float64 and fwd.shape == (len(q), 3, 3) and inv.shape == (len(q), 3, 3)
    assert np.array_equal(fwd.view(np.int64), fr.view(np.int64))  # bit for bit, signed zeros included
    assert np.array_equal(inv.view(np.int64), ir.view(np.int64))


def test_maps_agree_with_numpy_on_well_conditioned_quads():
    rng = np.random.default_rng(3)
    q = rotated_boxes(rng, 400)
    fwd, inv = perspective_maps(q)
    n = 0
    for k in range(len(q)):
        A, b = _system(q[k], 32, 100)
        if np.linalg.cond(A) > 1e8:
            continue
        n += 1
        m = np.r_[np.linalg.solve(A, b), 1].reshape(3, 3)
        assert np.abs(fwd[k] - m).max() <= 1e-12 * np.abs(m).max(), k
        mi = np.linalg.inv(fwd[k])
        assert np.abs(inv[k] - mi).max() <= 1e-12 * np.abs(mi).max(), k
        # the map sends the corners where they belong
        p = np.c_[q[k].astype(np.float64), np.ones(4)] @ fwd[k].T
        assert np.allclose(p[:, :2] / p[:, 2:], [[0, 0], [100, 0], [100, 32], [0, 32]], atol=1e-8)
    assert n >= 200


def test_singular_quads_give_zero_maps():
    q = np.array([[[0, 0], [1, 1], [2, 2], [3, 3]], [[5, 5]] * 4, [[0, 0], [10, 0], [10, 0], [0, 0]]], np.float32)
    fwd, inv = perspective_maps(q)
    expect = np.zeros((3, 3))
    expect[2, 2] = 1
    for k in range(len(q)):
        assert np.array_equal(fwd[k], expect) and np.array_equal(inv[k], np.zeros((3, 3)))
    # and the restatement agrees on its own
    assert R.perspective_map(q[0], 32, 100) == [0.0] * 8 + [1.0]
    assert R.invert3(R.perspective_map(q[0], 32, 100)) == [0.0] * 9


def test_empty_batch_of_maps():
    fwd, inv = perspective_maps(np.zeros((0, 4, 2), np.float32))
    assert fwd.shape == (0, 3, 3) and inv.shape == (0, 3, 3)


# ---- the restatement on crops with a known answer (checked here before the GPU tests use it as their yardstick) ----
def _image(rng, H, W):
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


def _expected_slice(img, y0, x0, h, w, step=1):
    """img[y0 : y0 + step*h : step, x0 : x0 + step*w : step], zero where it leaves the image"""
    H, W, _ = img.shape
    ys, xs = y0 + step * np.arange(h), x0 + step * np.arange(w)
    ok = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
    return np.where(ok[..., None], img[np.clip(ys, 0, H - 1)][:, np.clip(xs, 0, W - 1)], 0).astype(np.uint8)


def analytic_cases(rng, img):
    """(quad, (h, w), expected crop) for crops that sample integer source positions only"""
    H, W, _ = img.shape
    cases = []
    for (x0, y0, h, w) in [(10, 20, 32, 100), (0, 0, 32, 100), (W - 60, H - 20, 32, 100), (-7, -5, 32, 100), (W - 3, 4, 8, 40),
                           (3, 2, 17, 40), (5, 9, 1, 1), (1, 1, 3, 1100), (-50, 30, 20, 30)]:
        box = [[x0, y0], [x0 + w, y0], [x0 + w, y0 + h], [x0, y0 + h]]
        cases.append((box, (h, w), _expected_slice(img, y0, x0, h, w)))
        box2 = [[x0, y0], [x0 + 2 * w, y0], [x0 + 2 * w, y0 + 2 * h], [x0, y0 + 2 * h]]  # exact 2x decimation
        cases.append((box2, (h, w), _expected_slice(img, y0, x0, h, w, 2)))
        mirror = [[x0 + w, y0], [x0, y0], [x0, y0 + h], [x0 + w, y0 + h]]  # column u samples x0 + w - u
        cases.append((mirror, (h, w), _expected_slice(img, y0, x0 + 1, h, w)[:, ::-1]))
        # turned by 90 degrees: a source region w rows x h columns; out[v, u] = img[y0 + w - u, x0 + v]
        turned = [[x0, y0 + w], [x0, y0], [x0 + h, y0], [x0 + h, y0 + w]]
        cases.append((turned, (h, w), np.rot90(_expected_slice(img, y0 + 1, x0, w, h), -1)))
    return cases


def test_restatement_on_analytic_crops():
    rng = np.random.default_rng(5)
    img = _image(rng, 90, 150)
    for quad, (h, w), expect in analytic_cases(rng, img):
        got = R.crop(img, np.array(quad, np.float32), h, w)
        assert got.shape == expect.shape and np.array_equal(got, expect), (quad, (h, w))


# ---- box selection and argument checks (no launch) ------------------------------------------------------------------
def test_select_boxes_drops_zero_rows_and_low_scores():
    b0 = np.array([[[1, 1], [5, 1], [5, 4], [1, 4]], [[0, 0]] * 4, [[2, 2], [9, 2], [9, 6], [2, 6]]], np.int16)
    b1 = np.array([[[3, 3], [8, 3], [8, 7], [3, 7]], [[-5, 0], [1, 0], [1, 1], [1, 1]]], np.int16)  # sum 0: dropped
    s0, s1 = np.array([0.9, 0.0, 0.6], np.float32), np.array([0.7, 0.95], np.float32)
    q, idx = select_boxes([b0, b1])
    assert idx.dtype == np.int64 and idx.tolist() == [[0, 0], [0, 2], [1, 0]]
    assert q.dtype == np.float32 and np.array_equal(q, np.stack([b0[0], b0[2], b1[0]]).astype(np.float32))
    _, idx = select_boxes([b0, b1], [s0, s1], min_score=0.8)
    assert idx.tolist() == [[0, 0]]
    _, idx = select_boxes([(b0, s0), (b1, s1)], min_score=0.65)  # detect_boxes' (boxes, scores) pairs
    assert idx.tolist() == [[0, 0], [1, 0]]
    _, idx = select_boxes([np.zeros((0, 4, 2), np.int16), b1])
    assert idx.tolist() == [[1, 0]]
    q, idx = select_boxes([np.zeros((0, 4, 2), np.int16)])
    assert q.shape == (0, 4, 2) and idx.shape == (0, 2)


def test_select_boxes_compares_scores_in_double():
    b = np.array([[[1, 1], [5, 1], [5, 4], [1, 4]]], np.int16)
    s = np.array([0.7], np.float32)  # 0.699999988079071 as a double
    assert select_boxes([b], [s], min_score=0.7)[1].shape == (0, 2)
    assert select_boxes([b], [s], min_score=float(np.float32(0.7)))[1].tolist() == [[0, 0]]


@pytest.mark.parametrize('kwargs, match', [
    (dict(size=(0, 100)), 'crop size'),
    (dict(size=(32, 70000)), 'crop size'),
    (dict(size=32), 'size must be'),
    (dict(min_score=0.5), 'needs the scores'),
    (dict(scores=[np.zeros(1, np.float32)] * 3), 'score arrays'),
])
def test_crop_words_argument_errors(kwargs, match):
    img = torch.zeros((10, 12, 3), dtype=torch.uint8)
    boxes = [np.array([[[1, 1], [5, 1], [5, 4], [1, 4]]], np.int16)]
    with pytest.raises(ValueError, match=match):
        crop_words(img, boxes, **kwargs)


def test_crop_words_rejects_bad_images_and_boxes():
    boxes = [np.array([[[1, 1], [5, 1], [5, 4], [1, 4]]], np.int16)]
    with pytest.raises(ValueError, match='uint8'):
        crop_words(torch.zeros((10, 12, 3), dtype=torch.float32), boxes)
    with pytest.raises(ValueError, match='uint8'):
        crop_words(torch.zeros((10, 12), dtype=torch.uint8), boxes)
    with pytest.raises(ValueError, match='image_collate'):
        crop_words(np.zeros((10, 12, 3), np.uint8), boxes)
    with pytest.raises(ValueError, match='hold'):
        crop_words((torch.zeros(100, dtype=torch.uint8), [(10, 12)]), boxes)
    with pytest.raises(ValueError, match='image size'):
        crop_words((torch.zeros(0, dtype=torch.uint8), [(0, 12)]), boxes)
    with pytest.raises(ValueError, match='2 images'):
        crop_words(torch.zeros((10, 12, 3), dtype=torch.uint8), boxes * 2)
    with pytest.raises(ValueError, match=r'\[K, 4, 2\]'):
        crop_words(torch.zeros((10, 12, 3), dtype=torch.uint8), [np.zeros((2, 3, 2), np.int16)])
    with pytest.raises(ValueError, match='finite'):
        crop_words(torch.zeros((10, 12, 3), dtype=torch.uint8), [np.full((1, 4, 2), np.inf, np.float32)])
    with pytest.raises(ValueError, match='mixes'):
        crop_words(torch.zeros((10, 12, 3), dtype=torch.uint8), [(boxes[0], np.ones(1)), boxes[0]])
    with pytest.raises(ValueError, match='scores'):
        crop_words(torch.zeros((10, 12, 3), dtype=torch.uint8), boxes, scores=[np.ones(2)], min_score=0.1)
    with pytest.raises(ValueError, match='quads'):
        perspective_maps(np.zeros((3, 4), np.float32))
