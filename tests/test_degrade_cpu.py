"""CPU (-m "not gpu"): the degradation augmentation without a device.  The numpy restatement of
tests/degrade_ref.py is held against what it restates: Philox4x32-10's published answers, scipy's normal quantiles and
scipy.ndimage.gaussian_filter within the bound that the 16-bit weights allow; the package's host side (the table, blur_weights,
plan_degrade's draw order, degrade_records' checks and tile list, the entry point's refusal of a wrong tile list) is held against
the definition.  The device answers to the restatement byte for byte in tests/test_degrade_gpu.py."""
import math

import numpy as np
import pytest
import scipy.ndimage
import scipy.special

import degrade_ref as R
from db_text_minimal_amd import _lib, blur_weights, degrade_images, degrade_records, plan_degrade
from db_text_minimal_amd import degrade as D

SIGMAS = (0.1, 0.13, 0.5, 1, 2, 3.3, 8)
BLUR_SHAPES = ((1, 1), (1, 7), (2, 3), (5, 64), (33, 17), (70, 65))


@pytest.mark.parametrize('counter, key, want', [
    ((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ((0xffffffff, ) * 4, (0xffffffff, ) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1')])
def test_philox_known_answers(counter, key, want):
    assert ' '.join('%08x' % int(w) for w in R.philox(counter, key)) == want
    many = R.philox(tuple(np.full(3, c, np.uint64) for c in counter), key)  # the array form the noise uses
    assert all(' '.join('%08x' % int(w[i]) for w in many) == want for i in range(3))


def test_normal_table_is_scipys_quantiles():
    want = np.rint(scipy.special.ndtri((np.arange(4096) + 0.5) / 4096.0) * 4096.0).astype(np.int64)
    assert D.NORMAL_TABLE.dtype == np.int16 and D.NORMAL_TABLE.shape == (4096, )
    assert np.array_equal(D.NORMAL_TABLE.astype(np.int64), want) and np.array_equal(R.normal_table(), want)
    assert want.min() == -15025 and want.max() == 15025 and np.array_equal(want, -want[::-1])


@pytest.mark.parametrize('sigma', SIGMAS)
def test_blur_weights(sigma):
    q = blur_weights(sigma)
    r = int(4 * sigma + 0.5)
    assert len(q) == r + 1 and q == R.weights(sigma)
    assert q[0] + 2 * sum(q[1:]) == 65536
    assert all(a >= b >= 0 for a, b in zip(q, q[1:]))  # (symmetric by construction: q_i serves -i and i)
    if r == 0:
        assert q == [65536]


def test_blur_weights_limits():
    assert blur_weights(0) == [65536] and blur_weights(0.1249) == [65536] and len(blur_weights(0.125)) == 2 and len(blur_weights(8)) == 33
    for bad in (-0.1, 8.01, float('nan')):
        with pytest.raises(ValueError, match='sigma'):
            blur_weights(bad)


def kernel_error(sigma):
    """the L1 distance between the quantised 2-D kernel q_j q_i / 2^32 and the float one w_j w_i, and the radius"""
    q = R.weights(sigma)
    r = len(q) - 1
    w = np.array([math.exp(-(i * i) / (2.0 * sigma * sigma)) for i in range(-r, r + 1)])
    w /= w.sum()
    q1 = np.array([q[abs(i)] for i in range(-r, r + 1)], np.float64) / 65536.0
    return float(np.abs(np.outer(q1, q1) - np.outer(w, w)).sum()), r


@pytest.mark.parametrize('sigma', SIGMAS)
def test_restated_blur_against_scipy(sigma):
    """The exact sum S / 2^32 differs from the float filter by at most 255 times the L1 error of the quantised 2-D kernel, and the
    output byte by at most 0.5 more.  Each of the 2 r neighbour weights is rounded (error <= 2^-17) and the centre takes the sum of
    their errors (<= 2 r 2^-17): the 1-D L1 error is at most 4 r 2^-17, and that of the outer product, |a b - a' b'| <=
    |a - a'| |b| + |a'| |b - b'| summed with both kernels of sum 1, at most twice that: 8 r 2^-17, which times 255 is 0.498 at
    r = 32.  So every byte is within one level of the float result."""
    err, r = kernel_error(sigma)
    assert err <= 8 * r * 2.0**-17 and 255 * 8 * 32 * 2.0**-17 <= 0.4981
    rng = np.random.RandomState(0)
    for H, W in BLUR_SHAPES:
        for img in (rng.randint(0, 256, (H, W, 3)).astype(np.uint8), (rng.randint(0, 2, (H, W, 3)) * 255).astype(np.uint8)):
            got = R.blur(img, sigma).astype(np.float64)
            want = scipy.ndimage.gaussian_filter(img.astype(np.float64), sigma=(sigma, sigma, 0), mode='mirror', truncate=4.0)
            worst = float(np.abs(got - want).max())
            assert worst <= 0.5 + 255 * err + 1e-9 and worst <= 1.0, (H, W, worst)
            if img.size >= 900:
                differ = float((got != np.rint(want)).mean())
                assert differ <= 0.02, (H, W, differ)
            if r == 0:
                assert np.array_equal(got, img)


def test_mirror_is_scipys():
    for n in (1, 2, 3, 7):
        line = np.arange(n, dtype=np.float64) + 1
        for reach in (1, 5, 40):
            k = np.zeros(2 * reach + 1)
            k[0] = 1.0  # correlate1d: output[i] = input[i - reach]
            want = scipy.ndimage.correlate1d(line, k, mode='mirror')
            assert np.array_equal(line[R.mirror(np.arange(n) - reach, n)], want), (n, reach)


def test_noise_statistics_of_the_restatement():
    img = np.full((64, 64, 3), 128, np.uint8)
    delta = R.noise(img, 10, 0x1234567890ABCDEF, True).astype(np.float64) - 128
    assert abs(delta.mean()) <= 4 * 10 / math.sqrt(12288)
    assert abs(delta.std() - math.sqrt(100 + 1 / 12)) <= 4 * 10 / math.sqrt(2 * 12288)
    d = R.noise_delta(64, 64, 10, 0x1234567890ABCDEF, True)
    assert not np.array_equal(d[..., 0], d[..., 1]) and not np.array_equal(d[..., 1], d[..., 2])


def test_noise_one_draw_for_three_channels():
    d = R.noise_delta(9, 11, 10, 77, False)
    assert np.array_equal(d[..., 0], d[..., 1]) and np.array_equal(d[..., 0], d[..., 2]) and d.std() > 5
    assert np.array_equal(d[..., 0], R.noise_delta(9, 11, 10, 77, True)[..., 0])


def test_noise_clamps_and_zero_scale_is_the_identity():
    for level in (0, 255):
        img = np.full((16, 16, 3), level, np.uint8)
        out = R.noise(img, 64, 5, True)
        d = R.noise_delta(16, 16, 64, 5, True)
        assert (d > 0).any() and (d < 0).any() and np.abs(d).max() > 64
        assert np.array_equal(out, np.maximum(d, 0) if level == 0 else 255 + np.minimum(d, 0))  # clamped, not wrapped
        assert np.array_equal(R.noise(img, 0, 5, True), img)
    assert np.abs(R.noise_delta(4, 4, 64, 1, True)).max() <= (15025 * 16384 + (1 << 19)) >> 20


def test_plan_degrade_draw_order():
    kw = dict(blur=(0.5, 3.0), blur_p=0.6, noise=12.0, noise_p=0.4, per_channel=0.3)
    plans = plan_degrade(6, np.random.RandomState(3), **kw)
    rng = np.random.RandomState(3)
    for p in plans:
        ub, sigma, un, scale, uc = rng.uniform(), rng.uniform(0.5, 3.0), rng.uniform(), rng.uniform(0.0, 12.0), rng.uniform()
        lo, hi = int(rng.randint(0, 2**32, dtype=np.uint32)), int(rng.randint(0, 2**32, dtype=np.uint32))
        assert p == {'sigma': sigma if ub < 0.6 else 0.0, 'scale': scale if un < 0.4 else 0.0, 'per_channel': uc < 0.3, 'seed': lo | hi << 32}
    assert len({p['seed'] for p in plans}) == 6 and any(p['sigma'] for p in plans) and any(p['scale'] for p in plans)


def test_plan_degrade_probabilities_and_omissions():
    never = plan_degrade(20, np.random.RandomState(1), blur=2.0, blur_p=0, noise=5.0, noise_p=0, per_channel=0)
    assert all(p['sigma'] == 0 and p['scale'] == 0 and p['per_channel'] is False for p in never)
    always = plan_degrade(20, np.random.RandomState(1), blur=(1.0, 2.0), blur_p=1, noise=(3.0, 5.0), noise_p=1, per_channel=1)
    assert all(1 <= p['sigma'] <= 2 and 3 <= p['scale'] <= 5 and p['per_channel'] is True for p in always)
    # an operation left out makes the same draws: the other operation's values and the seeds do not move, nor does the stream's end
    a = np.random.RandomState(8)
    both = plan_degrade(5, a, blur=2.0, blur_p=1, noise=5.0, noise_p=1)
    after = a.uniform()
    for kw in (dict(blur=None), dict(blur=0), dict(blur=(0, 0))):
        b = np.random.RandomState(8)
        alone = plan_degrade(5, b, noise=5.0, noise_p=1, blur_p=1, **kw)
        assert [(p['scale'], p['per_channel'], p['seed']) for p in alone] == [(p['scale'], p['per_channel'], p['seed']) for p in both]
        assert all(p['sigma'] == 0 for p in alone) and b.uniform() == after
    assert plan_degrade(0, a) == []


def test_plan_degrade_refuses_bad_ranges():
    rng = np.random.RandomState(0)
    for kw in (dict(blur=8.5), dict(blur=(-1, 2)), dict(blur=(3, 2)), dict(noise=65), dict(noise=(5, 100)), dict(noise=-1)):
        with pytest.raises(ValueError, match='range'):
            plan_degrade(1, rng, **kw)
    for kw in (dict(blur_p=1.5), dict(noise_p=-0.1), dict(per_channel=2)):
        with pytest.raises(ValueError, match='probability'):
            plan_degrade(1, rng, blur=1.0, **kw)
    with pytest.raises(TypeError):
        plan_degrade(1, rng, blur='soft')


def plan(sigma=0.0, scale=0.0, per_channel=False, seed=0):
    return {'sigma': sigma, 'scale': scale, 'per_channel': per_channel, 'seed': seed}


def test_degrade_records_fields():
    shapes = [(5, 7), (33, 65), (2, 3)]
    desc, tiles = degrade_records(shapes, [plan(), plan(2.0, 10.0, True, 0xFEDCBA9876543210), plan(0.13, 0.5)])
    assert desc.shape == (3, 25) and desc.dtype == np.int64 and tiles.dtype == np.int32 and tiles.shape == (1 + 4 + 1, 3)
    assert desc[:, 0].tolist() == [0, 105, 105 + 33 * 65 * 3] and desc[:, 1:3].tolist() == [list(s) for s in shapes]
    assert desc[:, 3].tolist() == [0, 1, 5] and desc[:, 4].tolist() == [0, 8, 0]  # sigma 0.13: r = 1 with q_1 = 0 is the identity
    assert desc[:, 5].tolist() == [0, 2560 | 1 << 32, 128] and int(desc[1, 6]) & (2**64 - 1) == 0xFEDCBA9876543210
    taps = np.ascontiguousarray(desc[:, 8:]).view(np.uint32)
    assert taps[1, :9].tolist() == blur_weights(2.0) and not taps[1, 9:].any() and not taps[0].any() and not taps[2].any()


def test_degrade_records_refusals():
    with pytest.raises(ValueError, match='one plan per image'):
        degrade_records([(4, 4)] * 2, [plan()])
    with pytest.raises(ValueError, match='a batch holds'):
        degrade_records([], [])
    with pytest.raises(ValueError, match='image size'):
        degrade_records([(0, 4)], [plan()])
    with pytest.raises(ValueError, match='image size'):
        degrade_records([(4, 16385)], [plan()])
    with pytest.raises(ValueError, match='plan 1: sigma'):
        degrade_records([(4, 4)] * 2, [plan(), plan(sigma=8.1)])
    with pytest.raises(ValueError, match='plan 0: noise scale'):
        degrade_records([(4, 4)], [plan(scale=64.5)])
    with pytest.raises(ValueError, match='plan 0: noise scale'):
        degrade_records([(4, 4)], [plan(scale=-1)])
    with pytest.raises(ValueError, match='64-bit'):
        degrade_records([(4, 4)], [plan(seed=1 << 64)])
    with pytest.raises(ValueError, match='GPU'):
        degrade_images(np.zeros(48, np.uint8), [(4, 4)], [plan()])


def test_tile_list_covers_every_image_exactly_once():
    shapes = [(1, 1), (2, 3), (33, 65), (130, 257), (64, 128), (47, 2049)]
    sigmas = (2.0, 0.0, 0.5, 8.0, 1.0, 0.0)
    desc, tiles = degrade_records(shapes, [plan(s) for s in sigmas])
    assert tiles[:, 0].tolist() == sorted(tiles[:, 0].tolist())
    for n, ((H, W), s) in enumerate(zip(shapes, sigmas)):
        mine = tiles[tiles[:, 0] == n]
        assert desc[n, 3] == np.nonzero(tiles[:, 0] == n)[0][0]
        seen = np.zeros(H * W, np.int64)
        for _, a, b in mine:
            if s:
                assert a % D.TILE_H == 0 and b % D.TILE_W == 0 and a < H and b < W
                seen.reshape(H, W)[a:a + D.TILE_H, b:b + D.TILE_W] += 1
            else:
                assert a % D.RUN == 0 and b == 0 and a < H * W
                seen[a:a + D.RUN] += 1
        assert (seen == 1).all(), n


def test_entry_point_refuses_a_wrong_tile_list_before_any_launch():
    """dbn_degrade_u8 checks the host copies first and returns 1 without touching a device"""
    shapes = [(33, 65), (5, 7)]
    desc, tiles = degrade_records(shapes, [plan(2.0), plan()])
    need = sum(3 * h * w for h, w in shapes)
    src, dst, table = np.zeros(need, np.uint8), np.zeros(need, np.uint8), np.ascontiguousarray(D.NORMAL_TABLE)

    def call(desc, tiles, need=need):
        return _lib.lib().dbn_degrade_u8(src.ctypes.data, dst.ctypes.data, need, desc.ctypes.data, desc.ctypes.data, len(shapes), tiles.ctypes.data,
                                         tiles.ctypes.data, len(tiles), table.ctypes.data, None)

    def changed(a, at, value):
        a = a.copy()
        a[at] = value
        return a

    assert call(desc, tiles[:-1]) == 1 and call(desc, tiles[[0, 1, 3, 2, 4]]) == 1 and call(desc, tiles, need - 1) == 1
    for at, value in (((1, 2), 1), ((0, 0), 1), ((3, 1), 31), ((4, 1), D.RUN)):
        assert call(desc, changed(tiles, at, value)) == 1, at
    for at, value in (((0, 4), 33), ((0, 4), 7), ((0, 8), 0), ((0, 5), 16385), ((1, 0), 10), ((1, 3), 3), ((0, 2), 66)):
        assert call(changed(desc, at, value), tiles) == 1, at
