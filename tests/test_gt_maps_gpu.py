"""GPU (-m gpu): dbn_gt_maps / dbn_normalize_u8 (csrc/gtmaps.hip) through db_text_minimal_amd.gt_maps, against the
reference-produced tests/golden/gt_maps.npz and the numpy restatement tests/gt_maps_ref.py."""
import numpy as np
import pytest
import torch

from db_text_minimal_amd import DBLoss, DBTextModel, DBTrainer, FusedAdam, gt_maps as G, make_gt_maps, normalize_images
from oracle import dbnet_oracle as O
import gt_maps_ref as R
from gpu_util import DEV
from test_gt_maps_cpu import golden_batch, rect

pytestmark = pytest.mark.gpu


def _ulps(a, b):
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    return int(np.abs(ia - ib).max()) if a.size else 0


@pytest.mark.parametrize('S', [640, 128])
@pytest.mark.parametrize('own', [False, True])
def test_golden_maps(S, own):
    g = golden_batch(S)
    got = make_gt_maps(g['polys'], g['tags'], S, DEV, offsets=None if own else g['table'])
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    for c in (0, 1, 3):
        assert np.array_equal(got[c], g['maps'][c]), G.GT_KEYS[c]
    assert np.array_equal(got[2], g['maps'][2]), 'thresh_map: max %d ulp' % _ulps(got[2], g['maps'][2])


@pytest.mark.parametrize('S', [640, 128])
def test_normalize_images_bit_exact(S):
    g = golden_batch(S)
    got = normalize_images(torch.from_numpy(g['u8']).to(DEV)).cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got, g['img'])
    u8 = np.random.default_rng(3).integers(0, 256, (3, 40, 56, 3), dtype=np.uint8)
    got = normalize_images(torch.from_numpy(u8).to(DEV)).cpu().numpy()
    assert np.array_equal(got, np.stack([R.normalize(u) for u in u8]))


def _random_image_polys(rng, n, S):
    polys = []
    for _ in range(n):
        kind = rng.integers(0, 3)
        cx, cy = rng.uniform(-20, S + 20, 2)
        if kind == 0:  # rotated quad
            w, h, a = rng.uniform(6, 160), rng.uniform(6, 50), rng.uniform(-1, 1)
            c, s = np.cos(a), np.sin(a)
            p = np.array([[-w, -h], [w, -h], [w, h], [-w, h]]) / 2 @ np.array([[c, s], [-s, c]]) + [cx, cy]
        else:  # curved band with 7 or 10 points per side (14 / 20 vertices)
            m = 7 if kind == 1 else 10
            r, th, a0 = rng.uniform(30, 150), rng.uniform(8, 40), rng.uniform(0, 6)
            t = np.linspace(a0, a0 + rng.uniform(0.5, 2.5), m)
            outer = np.stack([cx + (r + th) * np.cos(t), cy + (r + th) * np.sin(t)], 1)
            inner = np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], 1)[::-1]
            p = np.concatenate([outer, inner])
        polys.append(p + rng.uniform(-0.5, 0.5, p.shape))
    tags = ['###' if rng.random() < 0.1 else 't' for _ in range(n)]
    return polys, tags


def test_batch_16x640_matches_restatement():
    S, rng = 640, np.random.default_rng(7)
    counts = [0, 1, 40] + [int(rng.integers(0, 40)) for _ in range(13)]
    polys, tags = zip(*[_random_image_polys(rng, c, S) for c in counts])
    got = make_gt_maps(list(polys), list(tags), S, DEV)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    want = R.maps_for_batch(G.plan_polygons(list(polys), list(tags), S), S)
    assert got.shape == (4, 16, S, S)
    for c in range(4):
        assert np.array_equal(got[c], want[c]), (G.GT_KEYS[c], np.argwhere(got[c] != want[c])[:5])
    empty = got[:, 0]
    assert (empty[0] == 0).all() and (empty[1] == 1).all() and (empty[2] == np.float32(0.3)).all() and (empty[3] == 0).all()


def test_past_edge_quirk_and_raise_cases_match_restatement():
    """one polygon per image, slid past the right and the bottom edge: padded boxes that start inside, 1, 2, ... up to
    past their own width beyond the last pixel (numpy's negative slice start; where the reference raises, nothing is
    drawn here, as in the restatement)."""
    S = 128
    polys = [[rect(S - 10 + t, 20, 40, 20)] for t in range(72)] + [[rect(30, S - 10 + t, 20, 40)] for t in range(72)]
    got = make_gt_maps(polys, None, S, DEV).cpu().numpy()
    want = R.maps_for_batch(G.plan_polygons(polys, None, S), S)
    assert np.array_equal(got, want)
    assert (got[2, :, :, S - 1] > np.float32(0.3)).sum() > 0


def test_argument_checks_leave_nothing_launched():
    S = 128
    out = torch.full((4, 1, S, S), 7.0, device=DEV)
    big = np.stack([60 + 40 * np.cos(np.linspace(0, 6, 65)), 60 + 40 * np.sin(np.linspace(0, 6, 65))], 1)
    for polys in ([[big]], [[np.zeros((0, 2))]], [[np.array([[1.0, 2.0], [np.nan, 3.0], [5.0, 9.0]])]]):
        with pytest.raises(ValueError):
            make_gt_maps(polys, None, S, DEV, out=out)
    with pytest.raises(ValueError):
        make_gt_maps([[rect(10, 10, 50, 20)]], None, S, DEV, out=torch.empty((4, 2, S, S), device=DEV))
    # the C ABI refuses a vertex bound over 64 and an empty batch by itself
    L = G.lib()
    img_off = torch.zeros(2, dtype=torch.int32, device=DEV)
    assert L.dbn_gt_maps(None, None, None, img_off.data_ptr(), None, 1, 0, S, 65, 0, 0.4, 0.3, out.data_ptr(), None) == 1
    assert L.dbn_gt_maps(None, None, None, img_off.data_ptr(), None, 0, 0, S, 4, 4, 0.4, 0.3, out.data_ptr(), None) == 1
    assert L.dbn_gt_maps(None, None, None, img_off.data_ptr(), None, 1, 1, S, 4, 4, 0.4, 0.3, out.data_ptr(), None) == 1
    torch.cuda.synchronize()
    assert (out == 7.0).all()


def test_end_to_end_step_on_device_built_batch():
    g = golden_batch(128)
    seed = 5
    sd = O.new_state(seed)
    model = DBTextModel()
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    trainer = DBTrainer(model, DBLoss(), FusedAdam(model, lr=0.005))
    img = normalize_images(torch.from_numpy(g['u8']).to(DEV))
    gts = make_gt_maps(g['polys'], g['tags'], 128, DEV, offsets=g['table'])
    preds, losses = trainer.step(img, gts)
    torch.cuda.synchronize()
    _, losses_o, _ = O.loss_and_grads(sd, torch.from_numpy(g['img']), torch.from_numpy(g['maps']))
    err = max(abs(a - b) for a, b in zip(losses.cpu().tolist(), losses_o))
    assert err < 1e-3, (losses.cpu().tolist(), losses_o)
