"""CPU (-m "not gpu"): the photometric augmentation without a device.  The numpy restatement of
tests/photometric_ref.py against Pillow, byte for byte (Image.blend, convert('L'), convert('HSV') and back over every colour,
the ImageEnhance chain plus torchvision's PIL hue recipe in all 24 orders); the same arithmetic as the library compiles it
(csrc/photometric.h, walked on the host by dbn_color_jitter_host) against the restatement; and plan_color_jitter."""
import itertools

import numpy as np
import pytest
from PIL import Image, ImageEnhance

import photometric_ref as R
from db_text_minimal_amd import _lib, plan_color_jitter
from db_text_minimal_amd import photometric as P

FACTORS = (0, 0.3, 0.8745098, 1, 1.1254902, 1.5, 2.7, -0.4)


def pil_hue(img, h):
    """torchvision's adjust_hue on a PIL image (functional_pil.py)"""
    hh, s, v = img.convert('HSV').split()
    np_h = np.array(hh, dtype=np.uint8)
    with np.errstate(over='ignore'):
        np_h += np.array(int(h * 255)).astype(np.uint8)
    return Image.merge('HSV', (Image.fromarray(np_h, 'L'), s, v)).convert('RGB')


PIL_OPS = {'brightness': lambda im, f: ImageEnhance.Brightness(im).enhance(f), 'contrast': lambda im, f: ImageEnhance.Contrast(im).enhance(f),
           'saturation': lambda im, f: ImageEnhance.Color(im).enhance(f), 'hue': pil_hue}


def pil_plan(arr, plan):
    im = Image.fromarray(arr)
    for name, f in plan:
        im = PIL_OPS[name](im, f)
    return np.asarray(im)


@pytest.fixture(scope='module')
def all_colours():
    """the 4096 x 4096 image that holds every colour once"""
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([v >> 16, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


def host_jitter(images, plans):
    """dbn_color_jitter_host on packed images -> packed result"""
    packed = np.concatenate([np.ascontiguousarray(im, dtype=np.uint8).reshape(-1) for im in images])
    desc = P.plan_records([im.shape[:2] for im in images], plans)
    out = np.full_like(packed, 0xA5)
    _lib.check(_lib.lib().dbn_color_jitter_host(packed.ctypes.data, out.ctypes.data, packed.size, desc.ctypes.data, len(images)), 'color_jitter_host')
    return out


@pytest.mark.parametrize('f', FACTORS)
def test_blend_is_pillows_over_every_pair(f):
    d, x = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing='ij')
    want = np.asarray(Image.blend(Image.fromarray(d), Image.fromarray(x), f))
    assert np.array_equal(R.blend(d, x, f), want)


def test_luma_is_pillows():
    img = np.random.RandomState(0).randint(0, 256, (512, 512, 3)).astype(np.uint8)
    assert np.array_equal(R.luma(img), np.asarray(Image.fromarray(img).convert('L')))


def test_hsv_both_ways_is_pillows_over_every_colour(all_colours):
    hsv = np.asarray(Image.fromarray(all_colours).convert('HSV'))
    assert np.array_equal(R.rgb_to_hsv(all_colours), hsv)
    # the same 2^24 triples read as HSV
    assert np.array_equal(R.hsv_to_rgb(all_colours), np.asarray(Image.fromarray(all_colours, 'HSV').convert('RGB')))


@pytest.mark.parametrize('order', list(itertools.permutations(R.OPS)), ids=lambda o: '-'.join(n[:3] for n in o))
def test_chain_is_pillows_in_every_order(order):
    img = np.random.RandomState(1).randint(0, 256, (33, 65, 3)).astype(np.uint8)
    factor = {'brightness': 1.2, 'contrast': 0.7, 'saturation': 1.6, 'hue': -0.13}
    plan = [(name, factor[name]) for name in order]
    want = pil_plan(img, plan)
    assert np.array_equal(R.apply_plan(img, plan), want)
    assert np.array_equal(host_jitter([img], [plan]).reshape(img.shape), want)  # ... and so is what the library compiles


def test_hue_shift_wraps_like_the_uint8_addition():
    for h in (-0.5, -0.3, -0.05, -0.001, 0, 0.001, 0.05, 0.3, 0.5):
        assert R.hue_shift(h) == int(np.array(int(h * 255)).astype(np.uint8)) == P.hue_shift(h)
    assert [R.hue_shift(h) for h in (-0.5, 0.5, 0)] == [129, 127, 0]


def test_library_arithmetic_equals_the_restatement(all_colours):
    """csrc/photometric.h on the host: hue over every colour against Pillow's recipe, the blends at factors inside and outside
    [0, 1], a packed batch with odd byte offsets, and the refusals of the record check."""
    assert np.array_equal(host_jitter([all_colours], [[('hue', 37 / 255)]]).reshape(all_colours.shape), np.asarray(pil_hue(Image.fromarray(all_colours), 37 / 255)))
    rng = np.random.RandomState(2)
    images = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((1, 1), (2, 3), (5, 7), (33, 65))]
    for f in (0, 0.4, 1, 1.8, 3.0):
        for name in ('brightness', 'contrast', 'saturation'):
            plans = [[(name, f)]] * len(images)
            assert np.array_equal(host_jitter(images, plans), R.jitter_packed(images, plans)), (name, f)
    desc = P.plan_records([(2, 3)], [[('contrast', 1.5)]])
    buf = np.zeros(18, np.uint8)
    call = lambda d, n=18: _lib.lib().dbn_color_jitter_host(buf.ctypes.data, buf.ctypes.data, n, d.ctypes.data, 1)
    assert call(desc) == 0 and call(desc, 17) == 1  # the image does not fit
    for field, value in ((1, 0), (2, 16385), (3, 1), (4, 5), (4, 2 | 2 << 4 | 2 << 8), (4, 1 | 7 << 4), (0, -1)):
        bad = desc.copy()
        bad[0, field] = value
        assert call(bad) == 1, (field, value)


def test_plan_color_jitter_ranges_and_orders():
    plans = plan_color_jitter(1000, np.random.RandomState(3), brightness=0.4, contrast=1.5, saturation=(0.5, 2.0), hue=0.1)
    lim = {'brightness': (0.6, 1.4), 'contrast': (0.0, 2.5), 'saturation': (0.5, 2.0), 'hue': (-0.1, 0.1)}
    orders = set()
    for plan in plans:
        assert sorted(name for name, _ in plan) == sorted(R.OPS)  # every operation exactly once
        for name, f in plan:
            assert lim[name][0] <= f <= lim[name][1], (name, f)
        orders.add(tuple(name for name, _ in plan))
    assert len(orders) == 24
    again = plan_color_jitter(1000, np.random.RandomState(3), brightness=0.4, contrast=1.5, saturation=(0.5, 2.0), hue=0.1)
    assert again == plans
    assert plan_color_jitter(1000, np.random.RandomState(4), brightness=0.4, contrast=1.5, saturation=(0.5, 2.0), hue=0.1) != plans
    spread = np.array([dict(p)['contrast'] for p in plans])
    assert spread.min() < 0.1 and spread.max() > 2.4  # the low end is clipped at 0, not folded


def test_plan_color_jitter_leaves_out_and_refuses():
    rs = np.random.RandomState(5)
    plans = plan_color_jitter(50, rs, brightness=32 / 255, contrast=None, saturation=0.5, hue=0)
    assert all(sorted(name for name, _ in p) == ['brightness', 'saturation'] for p in plans)
    before = rs.get_state()[1].copy(), rs.get_state()[2]
    assert plan_color_jitter(3, rs) == [[], [], []] and plan_color_jitter(2, rs, brightness=0, hue=(0, 0)) == [[], []]
    after = rs.get_state()
    assert np.array_equal(before[0], after[1]) and before[1] == after[2]  # nothing present: nothing drawn
    for kw in ({'hue': 0.6}, {'brightness': -0.1}, {'contrast': (1.5, 0.5)}, {'hue': (-0.6, 0.1)}, {'saturation': (-1, 1)}):
        with pytest.raises(ValueError):
            plan_color_jitter(1, rs, **kw)


def test_device_batches_takes_no_colour_step_when_no_operation_is_present():
    from db_text_minimal_amd import DeviceBatches
    assert P.color_jitter_ranges(brightness=0, hue=(0, 0)) == [] and P.color_jitter_ranges(saturation=0.5) == [('saturation', (0.5, 1.5))]
    for kw in ({'brightness': 0}, {}, {'hue': (0, 0), 'contrast': None}):
        b = DeviceBatches(None, 'cuda', True, seed=3, color_jitter=kw)
        assert b.color_jitter is None and b.jitter_rng is None
    b = DeviceBatches(None, 'cuda', True, seed=3, color_jitter={'brightness': 32 / 255, 'saturation': 0.5})
    assert b.color_jitter == {'brightness': 32 / 255, 'saturation': 0.5}
    want = np.random.RandomState([3, DeviceBatches.JITTER_STREAM]).random_sample(4)
    assert np.array_equal(b.jitter_rng.random_sample(4), want)
    assert np.array_equal(b.rng.random_sample(4), np.random.RandomState(3).random_sample(4))  # the geometric stream is the seed's own
    for kw in ({'hue': 0.6}, {'brightness': -1}):
        with pytest.raises(ValueError):
            DeviceBatches(None, 'cuda', True, color_jitter=kw)
    with pytest.raises(TypeError):
        DeviceBatches(None, 'cuda', True, color_jitter={'gamma': 1})


def test_plan_records_refuse_bad_plans():
    with pytest.raises(ValueError, match='one plan per image'):
        P.plan_records([(2, 2), (3, 3)], [[]])
    for plan in ([('hue', 0.6)], [('brightness', -1)], [('contrast', 1), ('contrast', 1)], [('gamma', 1)], [('saturation', float('inf'))]):
        with pytest.raises(ValueError):
            P.plan_records([(2, 2)], [plan])
    with pytest.raises(ValueError):
        P.plan_records([(16385, 2)], [[]])
    d = P.plan_records([(1, 1), (33, 65)], [[('hue', -0.5), ('brightness', 1.5)], []])
    assert d[:, 0].tolist() == [0, 3] and d[:, 3].tolist() == [0, 1] and d[0, 4] == 2 | 4 << 4 | 1 << 8 and d[1, 4] == 0
    assert d[0, 5] == 129 | int(np.float32(1.5).view(np.uint32)) << 32


def test_color_jitter_refuses_host_tensors():
    import torch
    with pytest.raises(ValueError, match='GPU'):
        P.color_jitter_images(torch.zeros(12, dtype=torch.uint8), [(2, 2)], [[]])
    with pytest.raises(ValueError, match='GPU'):
        P.adjust_hue(torch.zeros(2, 2, 3, dtype=torch.uint8), 0.1)
