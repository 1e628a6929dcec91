"""GPU (-m gpu): word crops of csrc/resample.hip warp_perspective_u8 through db_text_minimal_amd.word_crops: exact
against crops with a known answer, bit for bit against the restatement tests/crop_ref.py on mixed batches (image sizes,
output sizes, boxes outside the image, more than 65535 crops), every output byte written, and end to end from a
probability map through detect_boxes."""
import numpy as np
import pytest
import torch

from db_text_minimal_amd import crop_words, detect_boxes, image_collate, perspective_maps
from db_text_minimal_amd import word_crops as Wc
from db_text_minimal_amd import packed as Pk
from db_text_minimal_amd._lib import check, lib
import crop_ref as R
from gpu_util import DEV
from test_word_crops_cpu import analytic_cases, degenerate_quads, rotated_boxes

pytestmark = pytest.mark.gpu


def _image(rng, H, W):
    """smooth content with sharp edges and noise, so interpolation and saturation both show"""
    y, x = np.mgrid[0:H, 0:W]
    base = (np.stack([x * 7 + y * 3, x * 2 - y * 5, (x ^ y) * 11], -1) % 256).astype(np.uint8)
    noise = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return np.where(rng.random((H, W, 1)) < 0.3, noise, base).astype(np.uint8)


def _packed(imgs):
    return torch.from_numpy(np.concatenate([i.reshape(-1) for i in imgs])).to(DEV), [i.shape[:2] for i in imgs]


def test_analytic_crops_exact():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (90, 150, 3), dtype=np.uint8)
    by_size = {}
    for quad, size, expect in analytic_cases(rng, img):
        by_size.setdefault(size, []).append((quad, expect))
    t = torch.from_numpy(img).to(DEV)
    for size, cases in by_size.items():
        quads = np.array([q for q, _ in cases], np.float32)
        crops, index = crop_words(t, [quads], size)
        torch.cuda.synchronize()
        assert crops.shape == (len(cases), size[0], size[1], 3) and crops.dtype == torch.uint8 and crops.is_cuda
        assert index.tolist() == [[0, k] for k in range(len(cases))]
        got = crops.cpu().numpy()
        for k, (quad, expect) in enumerate(cases):
            assert np.array_equal(got[k], expect), (size, quad)


def _general_quads(rng, H, W, n):
    """genuinely perspective quads (independent corners), some straddling or outside the image, sub-pixel and very large
    ones, rotated boxes and degenerate ones"""
    out = []
    for _ in range(n):
        kind = rng.integers(0, 6)
        c = rng.uniform(-0.2, 1.2, 2) * (W, H)
        if kind == 0:    # a perspective quad of moderate size
            s = rng.uniform(5, 0.6 * max(H, W) + 5)
            q = c + rng.uniform(-s, s, (4, 2))
        elif kind == 1:  # sub-pixel
            q = c + rng.uniform(-0.7, 0.7, (4, 2))
        elif kind == 2:  # much larger than the image
            q = c + rng.uniform(-4, 4, (4, 2)) * max(H, W)
        elif kind == 3:  # fully outside
            q = rng.uniform(1.5, 3, 2) * (W + 10, H + 10) * rng.choice([-1, 1], 2) + rng.uniform(-20, 20, (4, 2))
        elif kind == 4:  # a trapezoid, like a word seen at an angle
            w, h = rng.uniform(10, 300), rng.uniform(5, 60)
            q = c + np.array([[-w, -h], [w, -0.6 * h], [w, 0.6 * h], [-w, h]]) / 2
        else:
            q = c + np.round(rng.uniform(-30, 30, (4, 2)))
        out.append(q)
    q = np.array(out, np.float32).reshape(-1, 4, 2)
    q[::7] = np.round(q[::7])
    return q


SHAPES = [(1, 1), (5, 3), (37, 53), (64, 1), (720, 1280), (2160, 3840)]


@pytest.mark.parametrize('size', [(32, 100), (17, 40), (1, 1), (2, 1100), (300, 300)])
def test_bit_exact_against_restatement_on_mixed_batch(size):
    rng = np.random.default_rng(size[0] * 1000 + size[1])
    imgs = [_image(rng, H, W) for H, W in SHAPES]
    n_per = 40 if size[0] * size[1] < 20000 else 6
    boxes = []
    for (H, W) in SHAPES:
        q = np.concatenate([_general_quads(rng, H, W, n_per), rotated_boxes(rng, 4) * (min(H, W) / 1300.0),
                            degenerate_quads(rng)[:8]])
        boxes.append(q.astype(np.float32))
    packed, shapes = _packed(imgs)
    crops, index = crop_words((packed, shapes), boxes, size)
    torch.cuda.synchronize()
    got = crops.cpu().numpy()
    q_all = np.concatenate([boxes[n][k][None] for n, k in index])
    _, inv = perspective_maps(q_all, size)
    _, inv_ref = R.maps(q_all, *size)
    assert np.array_equal(inv.view(np.int64), inv_ref.view(np.int64))
    nonzero = 0
    for j, (n, k) in enumerate(index):
        ref = R.warp_perspective(imgs[n], inv_ref[j], *size)
        assert np.array_equal(got[j], ref), (size, int(n), int(k), np.argwhere(got[j] != ref)[:4])
        nonzero += int(ref.any())
    assert nonzero > len(index) // 3  # most crops see some of their image


def test_more_than_65535_crops_in_one_call():
    rng = np.random.default_rng(17)
    imgs = [_image(rng, 37, 53), _image(rng, 200, 311)]
    size = (8, 20)
    boxes = [_general_quads(rng, 37, 53, 45000), _general_quads(rng, 200, 311, 40001)]
    packed, shapes = _packed(imgs)
    crops, index = crop_words((packed, shapes), boxes, size)
    torch.cuda.synchronize()
    K = crops.shape[0]
    assert K > 65535 and np.array_equal(index, Wc.select_boxes(boxes)[1])  # boxes with a coordinate sum <= 0 are dropped
    first1 = int(np.searchsorted(index[:, 0], 1))
    got = crops.cpu().numpy()
    sample = np.unique(np.r_[rng.integers(0, K, 300), np.arange(65530, 65545), first1 - 1, first1, K - 1])
    for j in sample:
        n, k = index[j]
        ref = R.crop(imgs[n], boxes[n][k], *size)
        assert np.array_equal(got[j], ref), j


def _launch(packed, shapes, quads, img_of, size, dst, src_off_override=None):
    """dbn_warp_perspective_u8 into a caller's buffer, with the descriptors crop_words builds"""
    off = Pk.offsets([h * w * 3 for h, w in shapes])
    hw = np.array(shapes, np.int64)[img_of]
    desc = np.stack([off[img_of], hw[:, 0], hw[:, 1]], 1)
    if src_off_override is not None:
        for k, v in src_off_override.items():
            desc[k, 0] = v
    _, inv = perspective_maps(quads, size)
    d, m = torch.from_numpy(desc).to(DEV), torch.from_numpy(inv).to(DEV)
    check(lib().dbn_warp_perspective_u8(packed.data_ptr(), packed.numel(), d.data_ptr(), m.data_ptr(), len(quads), size[0], size[1],
                                        dst.data_ptr(), dst.numel(), torch.cuda.current_stream().cuda_stream), 'warp_perspective_u8')


@pytest.mark.parametrize('K, size', [(7, (3, 5)), (1, (1, 1)), (13, (32, 100)), (5, (33, 1025))])
def test_every_byte_written_and_reproducible(K, size):
    rng = np.random.default_rng(K)
    imgs = [_image(rng, 37, 53), _image(rng, 64, 1)]
    packed, shapes = _packed(imgs)
    quads = np.concatenate([_general_quads(rng, 37, 53, K - K // 2), _general_quads(rng, 64, 1, K // 2)])
    img_of = np.r_[np.zeros(K - K // 2, np.int64), np.ones(K // 2, np.int64)]
    n = K * size[0] * size[1] * 3
    dst = torch.full((n + 4096, ), 0xA5, dtype=torch.uint8, device=DEV)  # poison, plus a guard past the end
    _launch(packed, shapes, quads, img_of, size, dst)
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert (out[n:] == 0xA5).all()  # nothing past the crops
    got = out[:n].reshape(K, size[0], size[1], 3)
    _, inv_ref = R.maps(quads, *size)
    for k in range(K):
        assert np.array_equal(got[k], R.warp_perspective(imgs[img_of[k]], inv_ref[k], *size)), k
    crops, index = crop_words((packed, shapes), [quads[:K - K // 2], quads[K - K // 2:]], size)
    crops2, _ = crop_words((packed, shapes), [quads[:K - K // 2], quads[K - K // 2:]], size)
    torch.cuda.synchronize()
    rows = [k if n == 0 else K - K // 2 + k for n, k in index]  # crop_words drops boxes with a coordinate sum <= 0
    assert np.array_equal(crops.cpu().numpy(), got[rows]) and torch.equal(crops, crops2)


def test_bad_descriptor_gives_a_zero_crop():
    rng = np.random.default_rng(2)
    img = _image(rng, 40, 60)
    packed, shapes = _packed([img])
    quads = np.array([[[2, 3], [50, 3], [50, 30], [2, 30]]] * 3, np.float32)
    dst = torch.full((3 * 32 * 100 * 3, ), 0xA5, dtype=torch.uint8, device=DEV)
    _launch(packed, shapes, quads, np.zeros(3, np.int64), (32, 100), dst, {1: 1, 2: -3})  # past the end / negative
    torch.cuda.synchronize()
    got = dst.cpu().numpy().reshape(3, 32, 100, 3)
    ref = R.crop(img, quads[0])
    assert np.array_equal(got[0], ref) and ref.any()
    assert not got[1].any() and not got[2].any()


def test_host_batch_and_empty_selection():
    rng = np.random.default_rng(4)
    imgs = [_image(rng, 30, 40), _image(rng, 50, 20)]
    packed, shapes, _, _ = image_collate([(i, [], None) for i in imgs])
    assert not packed.is_cuda
    boxes = [np.array([[[1, 2], [30, 2], [30, 20], [1, 20]]], np.int16), np.zeros((1, 4, 2), np.int16)]
    crops, index = crop_words(image_collate([(i, [], None) for i in imgs]), boxes)
    torch.cuda.synchronize()
    assert index.tolist() == [[0, 0]] and crops.shape == (1, 32, 100, 3) and crops.is_cuda
    assert np.array_equal(crops[0].cpu().numpy(), R.crop(imgs[0], boxes[0][0].astype(np.float32)))
    crops, index = crop_words((packed, shapes), [np.zeros((2, 4, 2), np.int16), []])
    assert crops.shape == (0, 32, 100, 3) and index.shape == (0, 2)


def test_end_to_end_from_probability_map():
    """rectangles of known probability -> detect_boxes(dest_sizes) -> crop_words on images whose pixels hold their own
    coordinates: each crop's centre pixel reads back its box's centre"""
    Hm, Wm, S = 128, 128, 2  # map 128^2, images 256^2
    rects = [  # (x0, x1, y0, y1) on the map, probability
        [((10, 40, 10, 20), 0.9), ((60, 110, 30, 45), 0.99), ((20, 70, 70, 80), 0.75), ((100, 102, 100, 102), 0.9),
         ((20, 50, 100, 115), 0.5)],
        [((5, 120, 5, 25), 0.95), ((30, 60, 60, 100), 0.72)],
    ]
    pred = torch.zeros((2, 1, Hm, Wm), dtype=torch.float32)
    for n, rs in enumerate(rects):
        for (x0, x1, y0, y1), p in rs:
            pred[n, 0, y0:y1, x0:x1] = p
    res = detect_boxes(pred.to(DEV), dest_sizes=[(Hm * S, Wm * S)] * 2)
    imgs = []
    for n in range(2):
        y, x = np.mgrid[0:Hm * S, 0:Wm * S]
        imgs.append(np.stack([x, y, np.full_like(x, 100 + n)], -1).astype(np.uint8))
    batch = image_collate([(i, [], None) for i in imgs])
    crops, index = crop_words(batch, res)
    torch.cuda.synchronize()
    kept = [[k for k in range(len(b)) if b[k].reshape(-1).astype(np.int64).sum() > 0] for b, _ in res]
    assert [len(k) for k in kept] == [3, 2]  # the 2 x 2 blob and the 0.5 rectangle are zero rows
    assert index.tolist() == [[n, k] for n in range(2) for k in kept[n]]
    got = crops.cpu().numpy()
    for j, (n, k) in enumerate(index):
        box = res[n][0][k].astype(np.float64)
        cx, cy = box.mean(0)
        px = got[j, 16, 50]
        assert abs(int(px[0]) - cx) <= 1 and abs(int(px[1]) - cy) <= 1 and px[2] == 100 + n, (n, k, px, cx, cy)
    # min_score: the 0.75 and 0.72 rectangles go
    crops2, index2 = crop_words(batch, res, min_score=0.8)
    scores = [[float(res[n][1][k]) for k in kept[n]] for n in range(2)]
    assert index2.tolist() == [[n, k] for n in range(2) for k, s in zip(kept[n], scores[n]) if s >= 0.8]
    assert len(index2) == 3
    sel = [j for j, (n, k) in enumerate(index) if [n, k] in index2.tolist()]
    assert torch.equal(crops2, crops[sel])
