"""GPU (-m gpu): the resample stages of csrc/resample.hip through db_text_minimal_amd.augment, bit for bit against the
numpy restatement tests/augment_ref.py and the reference-produced tests/golden/gt_maps.npz, plus registration of image
and polygons and fit() over DeviceBatches."""
import numpy as np
import pytest
import torch

from db_text_minimal_amd import augment as A
from db_text_minimal_amd import packed as Pk
from db_text_minimal_amd import (DBLoss, DBTextModel, DeviceBatches, FusedAdam, augment_images, image_collate, plan_augment,
                                 preprocess_image)
from oracle import dbnet_oracle as O
from oracle.postprocess_oracle import fill_poly_mask
import augment_ref as R
from gpu_util import DEV
from test_gt_maps_cpu import golden_batch

pytestmark = pytest.mark.gpu

MEAN32 = np.array([np.float32(v) for v in A.MEAN], np.float32)


def _plan(H, W, flip, angle, scale, window=None, size=640):
    """a training plan with chosen parameters (plan_augment draws them)"""
    h2, w2 = max(1, int(round(H * scale))), max(1, int(round(W * scale)))
    window = window or (0, h2, 0, w2)
    p = dict(flip=flip, angle=angle, scale=scale, M=A.rotation_matrix(angle, H, W), src_hw=(H, W), scaled_hw=(h2, w2), window=window,
             keep=[])
    return A._letterbox_plan(p, window[1] - window[0], window[3] - window[2], [], size)


def _images(rng, shapes):
    """smooth-ish content with sharp edges, so both interpolation and saturation are exercised"""
    out = []
    for h, w in shapes:
        y, x = np.mgrid[0:h, 0:w]
        base = (np.stack([x * 7 + y * 3, x * 2 - y * 5, (x ^ y) * 11], -1) % 256).astype(np.uint8)
        noise = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        out.append(np.where(rng.random((h, w, 1)) < 0.3, noise, base).astype(np.uint8))
    return out


def _packed(imgs):
    return torch.from_numpy(np.concatenate([i.reshape(-1) for i in imgs])).to(DEV)


# mixed sizes, angles +-10, scales 0.5 / 3.0, windows at the image edges
SHAPES = [(37, 53), (720, 1280), (64, 48), (5, 3), (200, 311)]
PLANS = [
    dict(flip=True, angle=-10.0, scale=3.0, window=(0, 111, 100, 159)),     # 111 x 159 scaled: right / top edges
    dict(flip=False, angle=10.0, scale=0.5, window=None),                   # 360 x 640, whole
    dict(flip=True, angle=3.3, scale=3.0, window=(150, 192, 0, 30)),        # bottom-left corner of 192 x 144
    dict(flip=False, angle=-7.25, scale=1.7, window=(1, 8, 2, 5)),          # 8 x 5 (round(8.5) = 8)
    dict(flip=True, angle=0.0, scale=0.5, window=(3, 100, 40, 156)),        # 100 x 156: bottom-right edges
]


def _stage_plans():
    return [_plan(H, W, p['flip'], p['angle'], p['scale'], p['window']) for (H, W), p in zip(SHAPES, PLANS)]


def test_each_stage_bit_exact_on_mixed_batch():
    rng = np.random.default_rng(0)
    imgs = _images(rng, SHAPES)
    plans = _stage_plans()
    src = _packed(imgs)
    off = Pk.offsets([h * w * 3 for h, w in SHAPES])
    warped = A.warp_stage(src, off, SHAPES, plans, torch.device(DEV))
    cropped, coff, win_hw = A.cubic_stage(warped, off, SHAPES, plans, torch.device(DEV))
    out = A._letterbox_launch(cropped, coff, win_hw, plans, 640, 640, A.MEAN, torch.device(DEV))
    torch.cuda.synchronize()
    warped, cropped, out = warped.cpu().numpy(), cropped.cpu().numpy(), out.cpu().numpy()
    for n, (img, p, (H, W)) in enumerate(zip(imgs, plans, SHAPES)):
        w_ref = R.warp_affine(img, A.invert_affine(p['M']), p['flip'])
        assert np.array_equal(warped[off[n]:off[n + 1]].reshape(H, W, 3), w_ref), ('warp', n)
        c_ref = R.resize_cubic(w_ref, *p['scaled_hw'], window=p['window'])
        assert np.array_equal(cropped[coff[n]:coff[n + 1]].reshape(c_ref.shape), c_ref), ('cubic', n)
        o_ref = R.letterbox_norm(c_ref, *p['out_hw'], 640, 640)
        assert np.array_equal(out[n], o_ref), ('letterbox', n, np.argwhere(out[n] != o_ref)[:5])
    assert not np.array_equal(warped[off[1]:off[2]], _packed([imgs[1]]).cpu().numpy())  # the rotation did something


def test_augment_images_equals_restatement_and_pads_minus_mean():
    rng = np.random.default_rng(1)
    imgs = _images(rng, SHAPES)
    plans = _stage_plans()
    got = augment_images(_packed(imgs).cpu(), SHAPES, plans, 640).cpu().numpy()
    assert got.shape == (5, 3, 640, 640) and got.dtype == np.float32
    for n, (img, p) in enumerate(zip(imgs, plans)):
        assert np.array_equal(got[n], R.augment_one(img, p, 640)), n
        nh, nw = p['out_hw']
        assert (got[n][:, nh:, :] == -MEAN32[:, None, None]).all() and (got[n][:, :, nw:] == -MEAN32[:, None, None]).all()


def test_eval_letterbox_of_mixed_sizes_and_odd_canvas():
    rng = np.random.default_rng(2)
    shapes = [(37, 53), (720, 1280), (1, 7), (500, 120)]
    imgs = _images(rng, shapes)
    for S in (640, 97):
        got = augment_images(_packed(imgs), shapes, None, S).cpu().numpy()
        for n, (img, p) in enumerate(zip(imgs, A.plan_letterbox(shapes, None, S))):
            assert np.array_equal(got[n], R.letterbox_norm(img, *p['out_hw'], S, S)), (S, n)


@pytest.mark.parametrize('S', [640, 128])
def test_letterbox_reproduces_golden_normalised_img(S):
    g = golden_batch(S)
    u8 = g['u8']
    N = len(u8)
    packed, shapes, _, _ = image_collate([(u8[i], [], None) for i in range(N)])
    got = augment_images(packed, shapes, None, S).cpu().numpy()
    assert np.array_equal(got, g['img'])


@pytest.mark.parametrize('pad', [False, True])
def test_preprocess_image(pad):
    rng = np.random.default_rng(3)
    img = _images(rng, [(720, 1280)])[0]
    got = preprocess_image(torch.from_numpy(img).to(DEV), 640, pad=pad).cpu().numpy()
    assert got.shape == ((1, 3, 640, 640) if pad else (1, 3, 360, 640))
    want = R.letterbox_norm(img, 360, 640, *((640, 640) if pad else (360, 640)))
    assert np.array_equal(got[0], want)
    odd = _images(rng, [(101, 67)])[0]
    got = preprocess_image(torch.from_numpy(odd).to(DEV), 640).cpu().numpy()
    assert got.shape == (1, 3, 640, 424) and np.array_equal(got[0], R.letterbox_norm(odd, 640, 424, 640, 424))


def _text_image(rng, H=360, W=640, n=6, margin=80):
    img = np.zeros((H, W, 3), np.uint8)
    polys = []
    for _ in range(n):
        cx, cy = rng.uniform(margin + 40, W - margin - 40), rng.uniform(margin + 15, H - margin - 15)
        w, h, a = rng.uniform(30, 80), rng.uniform(14, 30), rng.uniform(-0.5, 0.5)
        c, s = np.cos(a), np.sin(a)
        p = np.round(np.array([[-w, -h], [w, -h], [w, h], [-w, h]]) / 2 @ np.array([[c, s], [-s, c]]) + [cx, cy])
        polys.append(p)  # integral vertices: the drawn text is the fillPoly of the polygon itself
        img[fill_poly_mask(H, W, p.astype(np.int32)).astype(bool)] = 255
    return img, polys


def _edge_distance(px, polys):
    """distance of pixel centres px [K, 2] (x, y) to the nearest edge of any polygon"""
    best = np.full(len(px), np.inf)
    for p in polys:
        for i in range(len(p)):
            a, b = p[i], p[(i + 1) % len(p)]
            ab = b - a
            t = np.clip(((px - a) @ ab) / max(ab @ ab, 1e-12), 0, 1)
            best = np.minimum(best, np.hypot(*(px - (a + t[:, None] * ab)).T))
    return best


def _all_moved(polys, p):
    """every source polygon through the plan's geometry to output coordinates, unclamped (the crop drops polygons
    outside its window, but the resampling can carry a sliver of one across the window's edge)"""
    H, W = p['src_hw']
    (h2, w2), (y0, _, x0, _) = p['scaled_hw'], p['window']
    M, out = p['M'], []
    for q in polys:
        x = W - 1 - q[:, 0] if p['flip'] else q[:, 0]
        xx, yy = M[0, 0] * x + M[0, 1] * q[:, 1] + M[0, 2], M[1, 0] * x + M[1, 1] * q[:, 1] + M[1, 2]
        out.append(np.stack([xx * (w2 / W) - x0, yy * (h2 / H) - y0], 1) * p['letterbox_scale'])
    return out


def registration_error(out_img, polys, p):
    """largest distance, in source pixels, from a pixel where the thresholded image and the fillPoly of the planned polygons
    disagree to the nearest polygon edge (of a planned polygon, or of a source polygon moved without clamping)"""
    S = out_img.shape[-1]
    text = (out_img[0] + MEAN32[0]) > 127.5
    mask = np.zeros((S, S), bool)
    for q in p['polys']:
        mask |= fill_poly_mask(S, S, q.astype(np.int32)).astype(bool)
    bad = np.argwhere(text != mask)[:, ::-1].astype(np.float64)
    if not len(bad):
        return 0.0, int(mask.sum())
    edges = _all_moved(polys, p) + p['polys']  # the crop clamps the vertices of a polygon it cuts (db_transforms.crop)
    return float(_edge_distance(bad, edges).max()) / max(1.0, p['scale'] * p['letterbox_scale']), int(mask.sum())


def test_registration_of_image_and_polygons():
    """text filled at 255 through the whole chain, thresholded, against fillPoly of the planned polygons: they differ only
    within 2 source pixels of a polygon edge (2 * max(1, scale * letterbox_scale) output pixels).  The rest is the
    keypoint convention (x * w2 / W where the resize maps pixel centres, (x + 0.5) * w2 / W - 0.5) and fillPoly's edges."""
    rng = np.random.default_rng(4)
    items = [_text_image(rng) + (None, ) for _ in range(6)]
    packed, shapes, polys, _ = image_collate(items)
    plans = plan_augment(shapes, polys, np.random.RandomState(9), 640)
    got = augment_images(packed, shapes, plans, 640).cpu().numpy()
    checked = 0
    for n, p in enumerate(plans):
        err, area = registration_error(got[n], polys[n], p)
        assert area > 0 and err <= 2.0, (n, err)
        checked += area
    assert checked > 1000


def test_same_seed_same_output():
    rng = np.random.default_rng(5)
    items = [_text_image(rng, 300 + 20 * i, 500 + 10 * i) + (['t'] * 6, ) for i in range(3)]
    packed, shapes, polys, _ = image_collate(items)
    outs = []
    for _ in range(2):
        plans = plan_augment(shapes, polys, np.random.RandomState(42), 320)
        outs.append((augment_images(packed, shapes, plans, 320).cpu().numpy(), plans))
    assert np.array_equal(outs[0][0], outs[1][0])
    for a, b in zip(outs[0][1], outs[1][1]):
        assert a['window'] == b['window'] and all(np.array_equal(x, y) for x, y in zip(a['polys'], b['polys']))


class _Items(torch.utils.data.Dataset):
    def __init__(self, n, seed):
        rng = np.random.default_rng(seed)
        self.items = []
        for i in range(n):
            img, polys = _text_image(rng, 150 + 17 * i, 200 + 23 * i, n=3, margin=30)
            self.items.append((img, polys, ['t', '###', 't']))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def test_fit_over_device_batches():
    from db_text_minimal_amd.train import evaluate, fit
    S = 96
    train = DeviceBatches(torch.utils.data.DataLoader(_Items(4, 1), batch_size=2, collate_fn=image_collate), DEV, True, size=S, seed=3)
    test = DeviceBatches(torch.utils.data.DataLoader(_Items(2, 2), batch_size=2, collate_fn=image_collate), DEV, False, size=S)
    assert len(train) == 2 and len(test) == 1
    b = next(iter(test))
    assert b['img'].shape == (2, 3, S, S) and b['prob_map'].shape == (2, S, S)
    assert [len(a) for a in b['anns']] == [3, 3] and b['ignore_tags'][0][1] is True
    m = DBTextModel()
    m.load_state_dict(O.new_state(7))
    m = m.to(DEV).train()
    hist = fit(m, DBLoss(), FusedAdam(m, lr=0.005), train, test, epochs=2, device=DEV, detection={'protocol': 'iou'})
    assert len(hist) == 2
    for h in hist:
        assert np.isfinite(h['train_loss']) and np.isfinite(h['test_loss']) and 0 <= h['test_hmean'] <= 1
    loss, score = evaluate(m, DBLoss(), test, device=DEV, detection=True)
    assert np.isfinite(loss) and set(score) >= {'precision', 'recall', 'hmean'}
