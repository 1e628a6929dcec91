"""CPU: the host plan of db_text_minimal_amd.augment (crop and letterbox against the reference-produced
tests/golden/augment_crop.npz, bit for bit) and the numpy restatement tests/augment_ref.py on cases with a known answer."""
import os

import numpy as np
import pytest

from db_text_minimal_amd import augment as A
import augment_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'augment_crop.npz')


def _split(verts, counts):
    out, o = [], 0
    for c in counts:
        out.append(verts[o:o + c])
        o += c
    return out


def golden_cases():
    g = np.load(GOLDEN)
    polys = _split(g['in_verts'], g['poly_count'])
    crops = _split(g['crop_verts'], g['crop_poly_count'])
    lbs = _split(g['lb_verts'], g['crop_poly_count'])
    kept = _split(g['kept'], g['kept_count'])
    cases, p, q = [], 0, 0
    for c in range(len(g['hw'])):
        n, k = int(g['in_count'][c]), int(g['kept_count'][c])
        cases.append(dict(hw=tuple(int(v) for v in g['hw'][c]), seed=int(g['seed'][c]), size=int(g['size'][c]), polys=polys[p:p + n],
                          window=tuple(int(v) for v in g['window'][c]), kept=[int(v) for v in kept[c]], crop=crops[q:q + k],
                          lb_scale=float(g['lb_scale'][c]), lb_hw=tuple(int(v) for v in g['lb_hw'][c]), lb=lbs[q:q + k]))
        p += n
        q += k
    return cases


def test_golden_has_cropped_and_uncropped_cases():
    cases = golden_cases()
    cropped = [c for c in cases if c['window'] != (0, c['hw'][0], 0, c['hw'][1])]
    assert len(cases) >= 40 and len(cropped) >= 8 and len(cases) - len(cropped) >= 8
    assert any(len(c['kept']) < len(c['polys']) for c in cropped)


def test_crop_windows_and_polygons_bit_identical_to_reference():
    for c in golden_cases():
        h, w = c['hw']
        window, polys, keep = A.crop_window(h, w, c['polys'], np.random.RandomState(c['seed']))
        assert (window or (0, h, 0, w)) == c['window'], c['seed']
        assert keep == c['kept']
        assert len(polys) == len(c['crop'])
        for a, b in zip(polys, c['crop']):
            assert a.dtype == np.float64 and np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def test_letterbox_polygons_bit_identical_to_reference():
    for c in golden_cases():
        y0, y1, x0, x1 = c['window']
        s, nh, nw, polys = A.letterbox(y1 - y0, x1 - x0, c['crop'], c['size'])
        assert s == c['lb_scale'] and (nh, nw) == c['lb_hw']
        for a, b in zip(polys, c['lb']):
            assert np.array_equal(a, b)


def test_plan_augment_uses_the_crop_of_the_moved_polygons():
    """plan_augment = draws (flip, angle, scale) + moved polygons + crop_window with the same rng + letterbox"""
    rng = np.random.default_rng(5)
    polys = [[np.array([[100, 80], [400, 90], [395, 160], [98, 150]], np.float64) + rng.uniform(0, 300, 2) for _ in range(6)]]
    p = A.plan_augment([(720, 1280)], polys, np.random.RandomState(11), size=640)[0]
    r = np.random.RandomState(11)
    flip, angle, sc = r.random_sample() < 0.5, r.uniform(-10, 10), r.uniform(0.5, 3.0)
    assert (p['flip'], p['angle'], p['scale']) == (flip, angle, sc)
    h2, w2 = max(1, int(round(720 * sc))), max(1, int(round(1280 * sc)))
    assert p['scaled_hw'] == (h2, w2)
    M = A.rotation_matrix(angle, 720, 1280)
    moved = []
    for q in polys[0]:
        x = 1279 - q[:, 0] if flip else q[:, 0]
        xy = np.stack([x, q[:, 1], np.ones(len(q))], 1) @ M.T
        moved.append(np.stack([np.clip(xy[:, 0] * (w2 / 1280), 0, w2 - 1), np.clip(xy[:, 1] * (h2 / 720), 0, h2 - 1)], 1))
    window, cropped, keep = A.crop_window(h2, w2, moved, r)
    assert p['window'] == (window or (0, h2, 0, w2)) and p['keep'] == keep
    s, nh, nw, lb = A.letterbox(p['window'][1] - p['window'][0], p['window'][3] - p['window'][2], cropped, 640)
    assert p['out_hw'] == (nh, nw) and max(nh, nw) == 640
    for a, b in zip(p['polys'], lb):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-9)


def test_rotation_matrix_and_its_cv2_inverse():
    M = A.rotation_matrix(7.5, 37, 53)
    c = np.array([26.0, 18.0, 1.0])
    assert np.allclose(M @ c, c[:2])  # the centre ((W-1)/2, (H-1)/2) stays
    Mi = np.array(A.invert_affine(M)).reshape(2, 3)
    p = np.array([3.0, 30.0, 1.0])
    assert np.allclose(Mi @ np.append(M @ p, 1), p[:2])
    assert A.invert_affine(np.array([[1., 0, 0], [0, 1, 0]])) == [1, 0, 0, 0, 1, 0]


def _img(rng, h, w):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize('hw', [(37, 53), (64, 48), (1, 7)])
def test_restatement_identities(hw):
    rng = np.random.default_rng(1)
    img = _img(rng, *hw)
    assert np.array_equal(R.resize_cubic(img, *hw), img)  # scale 1
    assert np.array_equal(R.resize_linear_u8(img, *hw), img)
    ident = A.invert_affine(A.rotation_matrix(0.0, *hw))
    assert np.array_equal(R.warp_affine(img, ident, False), img)  # angle 0, no flip
    once = R.warp_affine(img, ident, True)
    assert np.array_equal(once, img[:, ::-1])
    assert np.array_equal(R.warp_affine(once, ident, True), img)  # double flip
    win = (hw[0] // 3, hw[0], hw[1] // 4, hw[1])
    assert np.array_equal(R.resize_cubic(img, *hw, window=win), img[win[0]:win[1], win[2]:win[3]])


def test_exact_2x_linear_downscale_is_rounded_2x2_mean():
    rng = np.random.default_rng(2)
    img = _img(rng, 46, 62)
    got = R.resize_linear_u8(img, 23, 31).astype(np.int64)
    q = img.astype(np.int64)
    want = (q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2] + 2) >> 2
    assert np.array_equal(got, want)


def test_cubic_window_is_the_window_of_the_full_resize():
    rng = np.random.default_rng(3)
    img = _img(rng, 29, 41)
    full = R.resize_cubic(img, 67, 90)
    assert np.array_equal(R.resize_cubic(img, 67, 90, window=(5, 60, 0, 33)), full[5:60, 0:33])
    down = R.resize_cubic(img, 15, 21)
    assert down.shape == (15, 21, 3)


def test_cubic_coefficients_sum_and_shape():
    x = np.linspace(0, 1, 33, dtype=np.float32)[:-1]
    c = R.cubic_coeffs(x)
    assert (c[0] == [0, 2048, 0, 0]).all()
    assert (np.abs(c.sum(1) - 2048) <= 2).all()
    assert (c[16] == [-192, 1216, 1216, -192]).all()  # x = 0.5: A = -0.75 gives -0.09375 / 0.59375


def test_letterbox_norm_pads_with_minus_mean():
    rng = np.random.default_rng(4)
    img = _img(rng, 30, 50)
    s, nh, nw, _ = A.letterbox(30, 50, [], 64)
    out = R.letterbox_norm(img, nh, nw, 64, 64)
    m = np.array([np.float32(v) for v in A.MEAN], np.float32)
    assert (nh, nw) == (38, 64)
    assert (out[:, nh:, :] == -m[:, None, None]).all()
    assert np.array_equal(out[:, :nh, :nw], R.resize_linear_u8(img, nh, nw).transpose(2, 0, 1).astype(np.float32) - m[:, None, None])


def test_image_collate_packs_in_order():
    rng = np.random.default_rng(6)
    imgs = [_img(rng, 5, 7), _img(rng, 3, 2)]
    items = [(imgs[0], [np.zeros((4, 2))], ['a']), (imgs[1], [], None)]
    packed, shapes, polys, tags = A.image_collate(items)
    assert shapes == [(5, 7), (3, 2)] and packed.numel() == 5 * 7 * 3 + 3 * 2 * 3
    assert np.array_equal(packed.numpy()[:105].reshape(5, 7, 3), imgs[0]) and np.array_equal(packed.numpy()[105:].reshape(3, 2, 3), imgs[1])
    assert tags == [['a'], []] and polys[0][0].dtype == np.float64


def test_plan_letterbox_and_errors():
    p = A.plan_letterbox([(720, 1280)], [[np.array([[10., 20.], [30., 40.], [5., 60.]])]], 640)[0]
    assert p['out_hw'] == (360, 640) and p['window'] == (0, 720, 0, 1280) and p['M'] is None
    assert np.array_equal(p['polys'][0], np.array([[10., 20.], [30., 40.], [5., 60.]]) * 0.5)
    with pytest.raises(ValueError):
        A.plan_letterbox([(1, 2000)], None, 640)  # letterboxes to 0 rows
    with pytest.raises(ValueError):
        A.plan_augment([(0, 5)], None, np.random.RandomState(0))
