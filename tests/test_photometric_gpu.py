"""GPU (-m gpu): the photometric augmentation on the device (csrc/photometric.hip, db_text_minimal_amd/photometric.py, DESIGN.md
section 37) against the numpy restatement of tests/photometric_ref.py, which tests/test_photometric_cpu.py pins to Pillow.  Every
comparison is of every byte.  The batch is five packed images of (1, 1), (2, 3), (5, 7), (33, 65) and (130, 257) pixels: odd byte
offsets, an image smaller than a wave, and one of 33 chunks, whose grey sum is folded by several workgroups."""
import itertools

import numpy as np
import pytest
import torch
from PIL import Image

import photometric_ref as R
from db_text_minimal_amd import (DeviceBatches, adjust_brightness, adjust_contrast, adjust_hue, adjust_saturation, augment_images,
                                 color_jitter_images, image_collate, make_gt_maps, plan_augment, plan_color_jitter)
from db_text_minimal_amd.gt_maps import GT_KEYS
from gpu_util import DEV

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 3), (5, 7), (33, 65), (130, 257)]
FACTOR = {'brightness': 1.3, 'contrast': 0.6, 'saturation': 1.7, 'hue': 0.21}
_made = {}


def images():
    if 'images' not in _made:
        rng = np.random.RandomState(7)
        _made['images'] = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SHAPES]
    return _made['images']


def pack(imgs):
    return torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs])).to(DEV)


def same_as_restatement(plans, imgs=None, tag=''):
    imgs = images() if imgs is None else imgs
    got = color_jitter_images(pack(imgs), [im.shape[:2] for im in imgs], plans)
    assert got.is_cuda and got.dtype == torch.uint8
    want = R.jitter_packed(imgs, plans)
    got = got.cpu().numpy()
    assert got.shape == want.shape
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, '%s: %d of %d bytes differ, the first at %d: got %d, want %d' % (tag, bad.size, want.size, bad[0], got[bad[0]], want[bad[0]])


@pytest.mark.parametrize('name', R.OPS)
def test_each_operation_alone(name):
    for f in ((-0.5, -0.05, 0, 0.05, 0.5) if name == 'hue' else (0, 0.4, 1, 1.8, 3.0)):
        same_as_restatement([[(name, f)]] * len(SHAPES), tag='%s %g' % (name, f))


def test_all_24_orders_a_different_one_per_image():
    orders = list(itertools.permutations(R.OPS))
    for k in range(0, 25, 5):  # five launches of five orders; the last wraps round to the first
        plans = [[(name, FACTOR[name]) for name in orders[(k + i) % 24]] for i in range(5)]
        same_as_restatement(plans, tag='orders %d ..' % k)


def test_the_15_subsets():
    subsets = [[(name, FACTOR[name]) for j, name in enumerate(R.OPS) if mask >> j & 1] for mask in range(1, 16)]
    assert len(subsets) == 15 and len(set(map(tuple, subsets))) == 15
    for k in range(0, 15, 5):
        same_as_restatement(subsets[k:k + 5], tag='subsets %d ..' % k)


def test_contrast_in_some_images_only():
    plans = [[('contrast', 1.5)], [], [('hue', -0.2), ('contrast', 0.3)], [('brightness', 0.8)],
             [('saturation', 1.9), ('contrast', 2.2), ('brightness', 1.1)]]
    same_as_restatement(plans, tag='mixed')
    same_as_restatement([[]] * 5, tag='empty plans copy')


def test_grey_sums_over_runs_of_chunks():
    """A batch of more than 2 x 4096 chunks, as every loader batch is: the grey-sum grid is capped at 4096 workgroups, so each takes
    a run of three consecutive chunks and a lane adds up greys over them.  No image ends on a multiple of three chunks, so a run
    crosses every image boundary (fold, add, start again in the middle of a run); contrast stands at step 0, 1, 2 and 3 of its
    plan, and the image in the middle has none (its chunks are passed while a sum is held)."""
    shapes = [(1601, 1104), (1097, 1509), (1303, 1402), (1611, 1099), (1400, 1307)]
    chunks = [-(-h * w // 1024) for h, w in shapes]
    per = -(-sum(chunks) // 4096)
    assert sum(chunks) > 2 * 4096 and per == 3 and all(int(e) % per for e in np.cumsum(chunks)[:-1])
    rng = np.random.RandomState(13)
    imgs = [rng.randint(0, top, (h, w, 3), dtype=np.uint8) for (h, w), top in zip(shapes, (256, 200, 256, 150, 100))]
    plans = [[('contrast', 1.6), ('brightness', 0.9)], [('saturation', 1.4), ('contrast', 0.5)], [('brightness', 1.2)],
             [('brightness', 1.1), ('hue', 0.07), ('contrast', 1.3)], [('saturation', 0.6), ('brightness', 1.3), ('hue', -0.2), ('contrast', 2.0)]]
    same_as_restatement(plans, imgs, tag='runs of chunks')
    means = [R.grey_mean(R.apply_plan(im, p[:[n for n, _ in p].index('contrast')])) for im, p in zip(imgs, plans) if len(p) > 1]
    assert len(set(means)) == 4, means  # a sum added to another image would show
    src, shp = pack(imgs), [im.shape[:2] for im in imgs]
    assert torch.equal(color_jitter_images(src, shp, plans), color_jitter_images(src, shp, plans))


def test_black_and_white_images():
    imgs = [np.zeros((130, 257, 3), np.uint8), np.full((130, 257, 3), 255, np.uint8), np.zeros((1, 1, 3), np.uint8), np.full((5, 7, 3), 255, np.uint8)]
    for order in (R.OPS, R.OPS[::-1]):
        same_as_restatement([[(name, FACTOR[name]) for name in order]] * 4, imgs, tag='flat')
    same_as_restatement([[('contrast', 3.0)], [('contrast', 0)], [('brightness', 3.0)], [('saturation', 0)]], imgs, tag='flat extremes')


def test_hue_on_every_colour_is_pillows():
    v = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([v >> 16, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    got = adjust_hue(torch.from_numpy(rgb).to(DEV), 37 / 255).cpu().numpy()
    hh, s, vv = Image.fromarray(rgb).convert('HSV').split()
    np_h = np.array(hh, dtype=np.uint8)
    with np.errstate(over='ignore'):
        np_h += np.uint8(37)
    want = np.asarray(Image.merge('HSV', (Image.fromarray(np_h, 'L'), s, vv)).convert('RGB'))
    assert R.hue_shift(37 / 255) == 37
    bad = np.nonzero((got != want).any(-1).reshape(-1))[0]
    assert bad.size == 0, '%d colours differ, the first %06x' % (bad.size, bad[0])


def test_two_runs_give_the_same_bytes_and_the_input_is_kept():
    imgs = images()
    shapes = [im.shape[:2] for im in imgs]
    plans = [[('saturation', 1.4), ('contrast', 1.7), ('hue', 0.1), ('brightness', 0.9)]] * 5
    src = pack(imgs)
    keep = src.clone()
    a = color_jitter_images(src, shapes, plans)
    b = color_jitter_images(src, shapes, plans)
    assert torch.equal(a, b) and torch.equal(src, keep) and a.data_ptr() != src.data_ptr()
    assert not torch.equal(a, src)
    out = torch.full_like(src, 0xA5)
    assert color_jitter_images(src, shapes, plans, out=out) is out and torch.equal(out, a) and torch.equal(src, keep)
    assert color_jitter_images(src, shapes, plans, out=src) is src and torch.equal(src, a)  # in place


def test_adjust_functions():
    imgs = images()
    one = torch.from_numpy(imgs[4]).to(DEV)
    four = torch.from_numpy(np.stack([np.roll(imgs[3], k, 1) for k in range(4)])).to(DEV)
    for fn, name, f in ((adjust_brightness, 'brightness', 1.25), (adjust_contrast, 'contrast', 0.5), (adjust_saturation, 'saturation', 2.0),
                        (adjust_hue, 'hue', -0.3)):
        got = fn(one, f)
        assert got.shape == one.shape and np.array_equal(got.cpu().numpy(), R.apply_plan(imgs[4], [(name, f)])), name
        got = fn(four, f)
        assert got.shape == four.shape
        for k in range(4):  # contrast takes each image's own mean
            assert np.array_equal(got[k].cpu().numpy(), R.apply_plan(four[k].cpu().numpy(), [(name, f)])), (name, k)
    ramp = torch.arange(2 * 3 * 3, dtype=torch.uint8, device=DEV).reshape(2, 3, 3) * 14
    assert torch.equal(adjust_brightness(ramp, 1), ramp) and not torch.equal(adjust_hue(ramp, 0), ramp)  # the HSV round trip is no identity


class _Items(torch.utils.data.Dataset):
    def __init__(self):
        rng = np.random.RandomState(9)
        self.imgs = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((96, 80), (71, 113), (64, 64), (120, 97))]

    def __len__(self):
        return len(self.imgs)

    def __getitem__(self, i):
        h, w = self.imgs[i].shape[:2]
        polys = [np.array([[5, 5], [w // 2, 6], [w // 2, h // 2], [5, h // 2]], np.float64),
                 np.array([[w // 2 + 4, h // 2 + 4], [w - 6, h // 2 + 4], [w - 6, h - 5], [w // 2 + 4, h - 5]], np.float64)]
        return self.imgs[i], polys, ['word', '###']


def _by_hand(loader, seed, size, jitter=None):
    """what DeviceBatches yields, composed from its parts with identically seeded streams"""
    rng = np.random.RandomState(seed)
    jrng = np.random.RandomState([seed, DeviceBatches.JITTER_STREAM])
    outs = []
    for packed, shapes, polys, tags in loader:
        packed = packed.to(DEV)
        if jitter is not None:
            packed = color_jitter_images(packed, shapes, plan_color_jitter(len(shapes), jrng, **jitter))
        plans = plan_augment(shapes, polys, rng, size)
        img = augment_images(packed, shapes, plans, size, device=DEV)
        maps = make_gt_maps([p['polys'] for p in plans], [[tags[i][j] for j in p['keep']] for i, p in enumerate(plans)], size, DEV)
        outs.append((img, maps))
    return outs


def test_device_batches_with_and_without_color_jitter():
    S, seed = 96, 11
    loader = torch.utils.data.DataLoader(_Items(), batch_size=2, collate_fn=image_collate, num_workers=0)
    jitter = {'brightness': 32 / 255, 'saturation': 0.5}
    off = list(DeviceBatches(loader, DEV, True, size=S, seed=seed))
    on = list(DeviceBatches(loader, DEV, True, size=S, seed=seed, color_jitter=jitter))
    hand_off, hand_on = _by_hand(loader, seed, S), _by_hand(loader, seed, S, jitter)
    assert len(off) == len(on) == len(hand_off) == len(hand_on) == 2
    for a, b, (img0, maps0), (img1, maps1) in zip(off, on, hand_off, hand_on):
        assert torch.equal(a['img'], img0)  # color_jitter=None: the path as it was
        assert torch.equal(b['img'], img1) and not torch.equal(b['img'], a['img'])
        for k, key in enumerate(GT_KEYS):  # the geometric plans do not see the colour stream
            assert torch.equal(a[key], maps0[k]) and torch.equal(b[key], maps0[k]) and torch.equal(maps1[k], maps0[k]), key
    # evaluation batches take no colour step
    ev = list(DeviceBatches(loader, DEV, False, size=S, color_jitter=jitter))
    ev0 = list(DeviceBatches(loader, DEV, False, size=S))
    assert all(torch.equal(x['img'], y['img']) for x, y in zip(ev, ev0))
    with pytest.raises(ValueError):
        DeviceBatches(loader, DEV, True, color_jitter={'hue': 0.6})


def test_refusals():
    imgs = images()
    shapes = [im.shape[:2] for im in imgs]
    src = pack(imgs)
    with pytest.raises(ValueError, match='one plan per image'):
        color_jitter_images(src, shapes, [[]] * 4)
    with pytest.raises(ValueError, match='GPU'):
        color_jitter_images(src.cpu(), shapes, [[]] * 5)
    with pytest.raises(ValueError, match='uint8'):
        color_jitter_images(src.float(), shapes, [[]] * 5)
    with pytest.raises(ValueError, match='bytes'):
        color_jitter_images(src[:-3], shapes, [[]] * 5)
    with pytest.raises(ValueError, match='out must hold'):
        color_jitter_images(src, shapes, [[]] * 5, out=torch.empty(src.numel() + 1, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        adjust_contrast(src.reshape(-1, 1, 3).float(), 1.0)
    wide = torch.zeros(src.numel() + 5, dtype=torch.uint8, device=DEV)  # an output that overlaps the input without being it
    with pytest.raises(ValueError, match='overlap'):
        color_jitter_images(wide[:-5], shapes, [[]] * 5, out=wide[5:])
    with pytest.raises(ValueError, match='overlap'):
        color_jitter_images(wide[5:], shapes, [[]] * 5, out=wide[:-5])
    assert color_jitter_images(wide[5:], shapes, [[]] * 5, out=wide[5:]).data_ptr() == wide[5:].data_ptr()
