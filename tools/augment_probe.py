#!/usr/bin/env python3
"""Cost of the loader's geometric stage on the device (db_text_minimal_amd.augment) for one training batch: 16 images of
1280 x 720 (the ICDAR2015 size) with 12 polygons each, scales spread over [0.5, 3], angles and flips drawn.

Prints:
  host     plan_augment for the batch (draws, polygon moves, crop, letterbox), one core, median
  device   each launch alone (descriptors already on the device), median of timed launches after warm-up (device events),
           against its byte floor at 8 TB/s computed from the shapes here; then augment_images end to end from a device
           batch (descriptor copies included), and the host-to-device copy of the packed uint8 batch for scale
  numpy    tests/augment_ref.py (the restatement the kernels are pinned to) per image, one core
Usage: python tools/augment_probe.py [--reps 50] [--out file]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from db_text_minimal_amd import augment as A  # noqa: E402
from db_text_minimal_amd import packed as Pk  # noqa: E402
from db_text_minimal_amd._lib import check, lib  # noqa: E402
import augment_ref as R  # noqa: E402

N, H, W, S, PER_IMAGE = 16, 720, 1280, 640, 12
BW = 8e12  # bytes / s


def batch(rng):
    imgs, polys = [], []
    for _ in range(N):
        imgs.append(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
        ps = []
        for _ in range(PER_IMAGE):
            cx, cy = rng.uniform(80, W - 80), rng.uniform(40, H - 40)
            w, h, a = rng.uniform(40, 200), rng.uniform(14, 40), rng.uniform(-0.4, 0.4)
            c, s = np.cos(a), np.sin(a)
            ps.append(np.array([[-w, -h], [w, -h], [w, h], [-w, h]]) / 2 @ np.array([[c, s], [-s, c]]) + [cx, cy])
        polys.append(ps)
    return imgs, polys


def plans_for(shapes, polys, seed):
    """plan_augment's draws, with the scales replaced by an even spread over [0.5, 3] (the crop re-planned for them)"""
    plans = A.plan_augment(shapes, polys, np.random.RandomState(seed), S)
    rng = np.random.RandomState(seed + 1)
    out = []
    for n, p in enumerate(plans):
        sc = 0.5 + 2.5 * n / (N - 1)
        out.append(A.plan_augment([shapes[n]], [polys[n]], _Fixed(p['flip'], p['angle'], sc, rng), S)[0])
    return out


class _Fixed:
    """a RandomState stand-in that returns the given flip / angle / scale draws, then defers to `rng` (the crop)"""

    def __init__(self, flip, angle, scale, rng):
        self.q = [0.0 if flip else 0.9, angle, scale]
        self.rng = rng

    def random_sample(self):
        return self.q.pop(0)

    def uniform(self, *_):
        return self.q.pop(0)

    def choice(self, *a, **k):
        return self.rng.choice(*a, **k)


def time_launch(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'the probe times the device: it needs a GPU'
    dev = torch.device('cuda')
    rng = np.random.default_rng(0)
    imgs, polys = batch(rng)
    shapes = [(H, W)] * N
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    t_plan = []
    for r in range(max(5, args.reps // 5)):
        t0 = time.perf_counter()
        A.plan_augment(shapes, polys, np.random.RandomState(r), S)
        t_plan.append(time.perf_counter() - t0)
    plans = plans_for(shapes, polys, 7)
    say('augment_probe: %d x %dx%d uint8, %d polygons per image, scales %.2f .. %.2f, out %d^2 fp32' %
        (N, H, W, PER_IMAGE, plans[0]['scale'], plans[-1]['scale'], S))
    say('host  plan_augment (measured, one core): %.2f ms per batch (median of %d)' % (1e3 * statistics.median(t_plan), len(t_plan)))

    packed_host = torch.from_numpy(np.concatenate([i.reshape(-1) for i in imgs])).pin_memory()
    src = packed_host.to(dev)
    off = Pk.offsets([H * W * 3] * N)
    L = lib()
    stream = torch.cuda.current_stream().cuda_stream
    dd = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731

    wd, wc, wh, ww = A.warp_args(off, shapes, plans)
    warped = torch.empty(int(off[-1]), device=dev, dtype=torch.uint8)
    wd_, wc_ = dd(wd), dd(wc)
    cd, cc, coff, win_hw, chh, cww = A.cubic_args(off, shapes, plans)
    cropped = torch.empty(int(coff[-1]), device=dev, dtype=torch.uint8)
    cd_, cc_ = dd(cd), dd(cc)
    ld, lc = A.letterbox_args(coff, win_hw, plans, S, S)
    out = torch.empty((N, 3, S, S), device=dev, dtype=torch.float32)
    ld_, lc_ = dd(ld), dd(lc)
    m = [float(np.float32(v)) for v in A.MEAN]

    def warp():
        check(L.dbn_warp_affine_u8(src.data_ptr(), src.numel(), wd_.data_ptr(), wc_.data_ptr(), N, wh, ww, warped.data_ptr(),
                                   warped.numel(), stream), 'warp')

    def cubic():
        check(L.dbn_resize_cubic_u8(warped.data_ptr(), warped.numel(), cd_.data_ptr(), cc_.data_ptr(), N, chh, cww,
                                    cropped.data_ptr(), cropped.numel(), stream), 'cubic')

    def linear():
        check(L.dbn_resize_linear_norm_u8(cropped.data_ptr(), cropped.numel(), ld_.data_ptr(), lc_.data_ptr(), N, S, S, *m,
                                          out.data_ptr(), stream), 'linear')

    img_bytes = N * H * W * 3
    crop_bytes = int(coff[-1])
    # cubic: the source rows / columns the window's taps reach (about window / scale), at most the warped image
    cubic_read = sum(min(H, int(np.ceil(ch / p['scale'])) + 3) * min(W, int(np.ceil(cw / p['scale'])) + 3) * 3
                     for p, (ch, cw) in zip(plans, win_hw))
    lin_read = sum(min(ch, 2 * p['out_hw'][0]) * min(cw, 2 * p['out_hw'][1]) * 3 for p, (ch, cw) in zip(plans, win_hw))
    out_bytes = N * 3 * S * S * 4
    total = 0.0
    for name, fn, rd, wr in (('warp_affine_u8', warp, img_bytes, img_bytes), ('resize_cubic_u8', cubic, cubic_read, crop_bytes),
                             ('resize_linear_norm_u8', linear, lin_read, out_bytes)):
        t = time_launch(fn, args.reps)
        total += t
        floor = (rd + wr) / BW * 1e3
        say('device %-22s (measured) %.3f ms   floor %.3f ms (%.1f MB read + %.1f MB written at 8 TB/s)  %.0f%% of floor rate' %
            (name, t, floor, rd / 1e6, wr / 1e6, 100 * floor / t))
    say('device three launches (measured, sum of medians): %.3f ms per batch' % total)
    t_e2e = time_launch(lambda: A.augment_images(src, shapes, plans, S), args.reps)
    say('device augment_images end to end from a device batch (measured, with descriptor copies): %.3f ms' % t_e2e)
    t_h2d = time_launch(lambda: packed_host.to(dev, non_blocking=True), args.reps)
    say('copy  packed uint8 batch host -> device, pinned (measured): %.3f ms for %.1f MB' % (t_h2d, img_bytes / 1e6))

    ref = A.augment_images(src, shapes, plans, S).cpu().numpy()
    t_np = []
    for n in (0, N // 2, N - 1):
        t0 = time.perf_counter()
        r = R.augment_one(imgs[n], plans[n], S)
        t_np.append(time.perf_counter() - t0)
        assert np.array_equal(r, ref[n]), 'device output differs from the numpy restatement (image %d)' % n
    say('numpy restatement (measured, one core): %.0f ms per image (mean of scales %.2f, %.2f, %.2f); device == numpy on them' %
        (1e3 * np.mean(t_np), plans[0]['scale'], plans[N // 2]['scale'], plans[-1]['scale']))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
