"""GPU (-m gpu): the degradation augmentation on the device (csrc/degrade.hip, db_text_minimal_amd/degrade.py)
against the numpy restatement of tests/degrade_ref.py, which tests/test_degrade_cpu.py anchors to scipy and to Philox's published
answers.  Every comparison is of every byte.  The batch is the photometric tests' five packed images of (1, 1), (2, 3), (5, 7),
(33, 65) and (130, 257) pixels: odd byte offsets, images smaller than a wave and smaller than the radius, and one image of 5 x 5
tiles whose last column of tiles is one pixel wide."""
import numpy as np
import pytest
import torch

import degrade_ref as R
from db_text_minimal_amd import (DeviceBatches, augment_images, degrade_images, gaussian_blur, gaussian_noise, image_collate, make_gt_maps,
                                 plan_augment, plan_degrade)
from db_text_minimal_amd.gt_maps import GT_KEYS
from gpu_util import DEV

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 3), (5, 7), (33, 65), (130, 257)]
SIGMAS = (0.1, 0.5, 2.0, 8.0, 3.3)
_made = {}


def images():
    if 'images' not in _made:
        rng = np.random.RandomState(7)
        _made['images'] = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SHAPES]
    return _made['images']


def blurred(i, sigma):
    """the restated blur of image i of the batch, made once"""
    if (i, sigma) not in _made:
        _made[i, sigma] = R.blur(images()[i], sigma)
        _made[i, sigma].setflags(write=False)
    return _made[i, sigma]


def plan(sigma=0.0, scale=0.0, per_channel=False, seed=0):
    return {'sigma': sigma, 'scale': scale, 'per_channel': per_channel, 'seed': seed}


def pack(imgs):
    return torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs])).to(DEV)


def restated(plans):
    out = []
    for i, p in enumerate(plans):
        im = blurred(i, p['sigma'])
        out.append((R.noise(im, p['scale'], p['seed'], p['per_channel']) if p['scale'] else im).reshape(-1))
    return np.concatenate(out)


def same(got, want, tag):
    assert got.is_cuda and got.dtype == torch.uint8
    got = got.cpu().numpy()
    assert got.shape == want.shape
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, '%s: %d of %d bytes differ, the first at %d: got %d, want %d' % (tag, bad.size, want.size, bad[0], got[bad[0]], want[bad[0]])


def same_as_restatement(plans, tag=''):
    imgs = images()
    same(degrade_images(pack(imgs), SHAPES, plans), restated(plans), tag)


@pytest.mark.parametrize('shift', range(5))
def test_blur_alone(shift):
    """every image meets every sigma over the five cases: r = 0, 2, 8, 32 and 13"""
    same_as_restatement([plan(SIGMAS[(i + shift) % 5]) for i in range(5)], 'blur, shift %d' % shift)


@pytest.mark.parametrize('per_channel', (False, True))
def test_noise_alone(per_channel):
    for scale in (0, 0.5, 10, 64):
        same_as_restatement([plan(0.0, scale, per_channel, 0x9E3779B97F4A7C15 * (i + 1) % 2**64) for i in range(5)], 'noise %g' % scale)


def test_noise_uses_the_high_word_of_the_seed():
    imgs = images()
    a, b = [plan(0.0, 10, True, 0x00000001_12345678)] * 5, [plan(0.0, 10, True, 0x00000002_12345678)] * 5
    got_a, got_b = degrade_images(pack(imgs), SHAPES, a), degrade_images(pack(imgs), SHAPES, b)
    same(got_a, restated(a), 'seed a')
    same(got_b, restated(b), 'seed b')
    assert not torch.equal(got_a[-3 * 130 * 257:], got_b[-3 * 130 * 257:])


def test_blur_and_noise_together():
    for shift in (0, 2):
        plans = [plan(SIGMAS[(i + shift) % 5], (64, 3.5, 10, 0.5, 20)[i], i % 2 == 0, 1000003 * i + (i << 40)) for i in range(5)]
        same_as_restatement(plans, 'both, shift %d' % shift)


def test_only_one_image_has_work():
    for busy, p in ((3, plan(2.0)), (4, plan(0.0, 10, True, 5)), (0, plan(8.0, 64, False, 6)), (2, plan(0.5, 1, True, 7))):
        same_as_restatement([p if i == busy else plan() for i in range(5)], 'image %d alone' % busy)
    same_as_restatement([plan()] * 5, 'identity plans copy')


def test_tile_edges():
    """rows of tiles that end 3, 2 and 0 pixels into a group of four, heights that end inside and on a tile, and a column strip of
    the vertical pass that ends outside the image"""
    shapes = [(35, 67), (9, 130), (64, 64), (32, 128)]
    rng = np.random.RandomState(21)
    imgs = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes]
    plans = [plan(1.0, 6, True, 11), plan(3.3, 0, False, 0), plan(0.5, 2, False, 12), plan(2.0, 30, True, 13)]
    same(degrade_images(pack(imgs), shapes, plans), R.degrade_packed(imgs, plans), 'tile edges')


def test_flat_images_stay_flat_under_blur():
    imgs = [np.full((40, 70, 3), v, np.uint8) for v in (0, 255, 1, 254)]
    shapes = [im.shape[:2] for im in imgs]
    got = degrade_images(pack(imgs), shapes, [plan(8.0), plan(8.0), plan(3.3), plan(0.5)])
    same(got, np.concatenate([im.reshape(-1) for im in imgs]), 'flat')  # the weights sum to 2^16 exactly


def test_out_and_the_input_is_kept():
    imgs = images()
    plans = [plan(SIGMAS[(i + 2) % 5], 5, True, i) for i in range(5)]
    src = pack(imgs)
    keep = src.clone()
    a, b = degrade_images(src, SHAPES, plans), degrade_images(src, SHAPES, plans)
    assert torch.equal(a, b) and torch.equal(src, keep) and a.data_ptr() != src.data_ptr() and not torch.equal(a, src)
    out = torch.full_like(src, 0xA5)
    assert degrade_images(src, SHAPES, plans, out=out) is out and torch.equal(out, a) and torch.equal(src, keep)
    same(out, restated(plans), 'out=')


def test_refusals():
    imgs = images()
    src = pack(imgs)
    plans = [plan()] * 5
    with pytest.raises(ValueError, match='overlap'):
        degrade_images(src, SHAPES, plans, out=src)  # a stencil cannot run in place
    wide = torch.zeros(src.numel() + 5, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match='overlap'):
        degrade_images(wide[:-5], SHAPES, plans, out=wide[5:])
    with pytest.raises(ValueError, match='overlap'):
        degrade_images(wide[5:], SHAPES, plans, out=wide[:-5])
    with pytest.raises(ValueError, match='one plan per image'):
        degrade_images(src, SHAPES, plans[:4])
    with pytest.raises(ValueError, match='GPU'):
        degrade_images(src.cpu(), SHAPES, plans)
    with pytest.raises(ValueError, match='uint8'):
        degrade_images(src.float(), SHAPES, plans)
    with pytest.raises(ValueError, match='bytes'):
        degrade_images(src[:-3], SHAPES, plans)
    with pytest.raises(ValueError, match='out must hold'):
        degrade_images(src, SHAPES, plans, out=torch.empty(src.numel() + 1, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match='sigma'):
        degrade_images(src, SHAPES, [plan(9.0)] * 5)
    with pytest.raises(ValueError):
        gaussian_blur(src.reshape(-1, 1, 3).float(), 1.0)


def test_single_tensor_functions():
    imgs = images()
    one = torch.from_numpy(imgs[4]).to(DEV)
    four_np = np.stack([np.roll(imgs[3], k, 1) for k in range(4)])
    four = torch.from_numpy(four_np).to(DEV)
    got = gaussian_blur(one, 2.0)
    assert got.shape == one.shape and np.array_equal(got.cpu().numpy(), blurred(4, 2.0))
    got = gaussian_blur(four, 3.3)
    assert got.shape == four.shape
    for k in range(4):
        assert np.array_equal(got[k].cpu().numpy(), R.blur(four_np[k], 3.3)), k
    for per_channel in (True, False):
        got = gaussian_noise(one, 10, 99, per_channel)
        assert got.shape == one.shape and np.array_equal(got.cpu().numpy(), R.noise(imgs[4], 10, 99, per_channel))
        got = gaussian_noise(four, 10, 99, per_channel)
        for k in range(4):  # the field depends on the seed and the place alone
            assert np.array_equal(got[k].cpu().numpy(), R.noise(four_np[k], 10, 99, per_channel)), k
    assert torch.equal(gaussian_blur(one, 0.1), one) and torch.equal(gaussian_noise(one, 0, 1), one)


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


def _by_hand(loader, seed, size, degrade=None):
    """what DeviceBatches yields, composed from its parts with identically seeded streams; also the geometric plans"""
    rng = np.random.RandomState(seed)
    drng = np.random.RandomState([seed, DeviceBatches.DEGRADE_STREAM])
    outs = []
    for packed, shapes, polys, tags in loader:
        packed = packed.to(DEV)
        if degrade is not None:
            packed = degrade_images(packed, shapes, plan_degrade(len(shapes), drng, **degrade))
        plans = plan_augment(shapes, polys, rng, size)
        img = augment_images(packed, shapes, plans, size, device=DEV)
        maps = make_gt_maps([p['polys'] for p in plans], [[tags[i][j] for j in p['keep']] for i, p in enumerate(plans)], size, DEV)
        outs.append((img, maps))
    return outs


def test_device_batches_with_and_without_degrade():
    S, seed = 96, 11
    loader = torch.utils.data.DataLoader(_Items(), batch_size=2, collate_fn=image_collate, num_workers=0)
    kw = {'blur': 2.0, 'blur_p': 1.0, 'noise': (4.0, 10.0), 'noise_p': 1.0}
    off = list(DeviceBatches(loader, DEV, True, size=S, seed=seed))
    on = list(DeviceBatches(loader, DEV, True, size=S, seed=seed, degrade=kw))
    zero = list(DeviceBatches(loader, DEV, True, size=S, seed=seed, degrade={'blur': 0}))
    hand_off, hand_on = _by_hand(loader, seed, S), _by_hand(loader, seed, S, kw)
    assert len(off) == len(on) == len(zero) == len(hand_off) == len(hand_on) == 2
    for a, b, z, (img0, maps0), (img1, maps1) in zip(off, on, zero, hand_off, hand_on):
        assert torch.equal(a['img'], img0)  # degrade=None: the path as it was
        assert torch.equal(b['img'], img1) and not torch.equal(b['img'], a['img'])
        for k, key in enumerate(GT_KEYS):  # the geometric plans do not see the degradation stream
            assert torch.equal(a[key], maps0[k]) and torch.equal(b[key], maps0[k]) and torch.equal(maps1[k], maps0[k]), key
        assert sorted(z) == sorted(a) and all(torch.equal(z[key], a[key]) for key in a)
    both = list(DeviceBatches(loader, DEV, True, size=S, seed=seed, degrade=kw, color_jitter={'brightness': 0.2}))
    jitter = list(DeviceBatches(loader, DEV, True, size=S, seed=seed, color_jitter={'brightness': 0.2}))
    for a, b, j in zip(off, both, jitter):
        assert not torch.equal(b['img'], j['img']) and all(torch.equal(a[key], b[key]) for key in GT_KEYS)
    # evaluation batches take no degradation step
    ev = list(DeviceBatches(loader, DEV, False, size=S, degrade=kw))
    ev0 = list(DeviceBatches(loader, DEV, False, size=S))
    assert all(torch.equal(x['img'], y['img']) for x, y in zip(ev, ev0))
    with pytest.raises(ValueError):
        DeviceBatches(loader, DEV, True, degrade={'blur': 9.0})
