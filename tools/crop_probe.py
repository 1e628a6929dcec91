#!/usr/bin/env python3
"""Cost of the word crops on the device (db_text_minimal_amd.word_crops) for one dense inference batch: 32 images of
1280 x 1280 with 300 rotated word boxes each (int16 corners, as detect_boxes gives them), 9 600 crops of 32 x 100.

Prints:
  host     perspective_maps for the batch (dbn_perspective_maps, one call, one core), median
  device   dbn_warp_perspective_u8 alone (descriptors and maps already on the device), median of timed launches after
           warm-up (device events), against its byte floor at 8 TB/s: the crops written plus the source bytes inside the
           quads (their shoelace areas, 3 bytes per pixel)
  e2e      crop_words from a device batch: box selection, the maps call, the descriptor copies and the launch, wall clock
           to a synchronised device, median
  numpy    tests/crop_ref.py per crop, one core: a CPU stand-in for the reference's per-box cv2 calls, NOT cv2 (which is
           not installed here and would be faster); device == numpy on the crops it times
Usage: python tools/crop_probe.py [--reps 50] [--out file]
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

from db_text_minimal_amd import crop_words, perspective_maps  # noqa: E402
from db_text_minimal_amd import word_crops as Wc  # noqa: E402
from db_text_minimal_amd import packed as Pk  # noqa: E402
from db_text_minimal_amd._lib import check, lib  # noqa: E402
import crop_ref as R  # noqa: E402

N, H, W, PER_IMAGE, SIZE = 32, 1280, 1280, 300, (32, 100)
BW = 8e12  # bytes / s


def boxes_for(rng):
    """per image int16 [300, 4, 2]: rotated rectangles 20-300 x 10-50 px, angles +-30 degrees, inside the image"""
    out = []
    for _ in range(N):
        c = rng.uniform(200, W - 200, (PER_IMAGE, 2))
        w, h, a = rng.uniform(20, 300, PER_IMAGE), rng.uniform(10, 50, PER_IMAGE), rng.uniform(-0.5, 0.5, PER_IMAGE)
        base = np.stack([np.stack([-w, -h], 1), np.stack([w, -h], 1), np.stack([w, h], 1), np.stack([-w, h], 1)], 1) / 2
        ca, sa = np.cos(a)[:, None], np.sin(a)[:, None]
        q = np.stack([base[..., 0] * ca - base[..., 1] * sa, base[..., 0] * sa + base[..., 1] * ca], -1) + c[:, None, :]
        out.append(np.round(q).astype(np.int16))
    return out


def shoelace(q):
    x, y = q[..., 0].astype(np.float64), q[..., 1].astype(np.float64)
    return 0.5 * np.abs((x * np.roll(y, -1, -1) - np.roll(x, -1, -1) * y).sum(-1))


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


def time_wall(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'the probe times the device: it needs a GPU'
    dev = torch.device('cuda')
    rng = np.random.default_rng(0)
    imgs = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(N)]
    boxes = boxes_for(rng)
    shapes = [(H, W)] * N
    src = torch.from_numpy(np.concatenate([i.reshape(-1) for i in imgs])).to(dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    quads, index = Wc.select_boxes(boxes)
    K = len(quads)
    h, w = SIZE
    say('crop_probe: %d x %dx%d uint8, %d boxes per image, %d crops of %d x %d' % (N, H, W, PER_IMAGE, K, h, w))

    t_maps = []
    for _ in range(max(5, args.reps // 5)):
        t0 = time.perf_counter()
        _, inv = perspective_maps(quads, SIZE)
        t_maps.append(1e3 * (time.perf_counter() - t0))
    say('host   perspective_maps (measured, one core): %.3f ms for %d quads (median of %d)' % (statistics.median(t_maps), K, len(t_maps)))

    off = Pk.offsets([H * W * 3] * N)
    desc = np.stack([off[index[:, 0]], np.full(K, H, np.int64), np.full(K, W, np.int64)], 1)
    d, m = torch.from_numpy(desc).to(dev), torch.from_numpy(inv).to(dev)
    crops = torch.empty((K, h, w, 3), device=dev, dtype=torch.uint8)
    L = lib()
    stream = torch.cuda.current_stream().cuda_stream

    def launch():
        check(L.dbn_warp_perspective_u8(src.data_ptr(), src.numel(), d.data_ptr(), m.data_ptr(), K, h, w, crops.data_ptr(), crops.numel(),
                                        stream), 'warp_perspective_u8')

    t = time_launch(launch, args.reps)
    out_bytes = K * h * w * 3
    src_bytes = int(shoelace(quads).sum()) * 3
    floor = (out_bytes + src_bytes) / BW * 1e3
    say('device warp_perspective_u8 (measured) %.3f ms   floor %.3f ms (%.1f MB written + %.1f MB of source inside the quads at '
        '8 TB/s)  %.0f%% of floor rate' % (t, floor, out_bytes / 1e6, src_bytes / 1e6, 100 * floor / t))
    t_e2e = time_wall(lambda: crop_words((src, shapes), boxes, SIZE), max(10, args.reps // 2))
    say('e2e    crop_words from a device batch (measured, wall clock to a synchronised device): %.3f ms' % t_e2e)

    got, _ = crop_words((src, shapes), boxes, SIZE)
    got = got.cpu().numpy()
    sample = np.linspace(0, K - 1, 40).astype(np.int64)
    t_np = []
    for j in sample:
        n, k = index[j]
        t0 = time.perf_counter()
        ref = R.crop(imgs[n], boxes[n][k].astype(np.float32), h, w)
        t_np.append(time.perf_counter() - t0)
        assert np.array_equal(ref, got[j]), 'device crop %d differs from the numpy restatement' % j
    per = 1e3 * statistics.median(t_np)
    say('numpy  restatement per crop (measured, one core; a CPU stand-in, NOT cv2): %.3f ms, %.0f ms for the %d crops; '
        'device == numpy on %d crops' % (per, per * K, K, len(sample)))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
