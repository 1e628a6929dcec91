#!/usr/bin/env python3
"""Cost of rendering detection results on the device (db_text_minimal_amd.render) for two workloads: a dense inference
batch of 32 images of 1280 x 1280 with 300 rotated boxes each, and one 2160 x 3840 frame with 300 boxes; thickness 3, one
640 x 640 probability map per image.

Prints, per workload:
  strokes  dbn_draw_strokes alone (the copy of the images plus the stroke launch; descriptors and edges already on the
           device), median of timed calls after warm-up (device events), against its byte floor at 8 TB/s: the copy's
           3 bytes read and 3 written per pixel
  minmax   dbn_render_minmax alone (the autoscale reduction: reads the maps, writes 8 bytes per image); floor: the maps
  paint    dbn_render_paint alone, in place over the outlined images; floor: 3 bytes read and 3 written per pixel plus the maps
  e2e      render_detections from device inputs: edge building on the host, the descriptor copies and the three calls, wall
           clock to a synchronised device, median
  numpy    tests/render_ref.py on one image, one core: a CPU stand-in for the reference's cv2.polylines / cv2.resize /
           matplotlib calls, NOT those libraries (cv2 is not installed here and would be faster); device == numpy on it
Usage: python tools/render_probe.py [--reps 30] [--out file]
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

from db_text_minimal_amd import image_views, render_detections  # noqa: E402
from db_text_minimal_amd import render as Rn  # noqa: E402
from db_text_minimal_amd import packed as Pk  # noqa: E402
from db_text_minimal_amd._lib import check, lib  # noqa: E402
import render_ref as R  # noqa: E402

PER_IMAGE, THICKNESS, MAP = 300, 3, 640
BW = 8e12  # bytes / s


def boxes_for(rng, N, H, W):
    """per image int16 [300, 4, 2]: rotated rectangles 20-300 x 10-50 px, angles +-30 degrees, inside the image"""
    out = []
    for _ in range(N):
        c = rng.uniform(200, [W - 200, H - 200], (PER_IMAGE, 2))
        w, h, a = rng.uniform(20, 300, PER_IMAGE), rng.uniform(10, 50, PER_IMAGE), rng.uniform(-0.5, 0.5, PER_IMAGE)
        base = np.stack([np.stack([-w, -h], 1), np.stack([w, -h], 1), np.stack([w, h], 1), np.stack([-w, h], 1)], 1) / 2
        ca, sa = np.cos(a)[:, None], np.sin(a)[:, None]
        q = np.stack([base[..., 0] * ca - base[..., 1] * sa, base[..., 0] * sa + base[..., 1] * ca], -1) + c[:, None, :]
        out.append(np.round(q).astype(np.int16))
    return out


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


def workload(say, rng, N, H, W, reps):
    dev = torch.device('cuda')
    imgs = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(N)]
    boxes = boxes_for(rng, N, H, W)
    shapes = [(H, W)] * N
    y, x = np.mgrid[0:MAP, 0:MAP].astype(np.float32)
    prob = np.stack([np.exp(-(((x - rng.uniform(0, MAP)) / 120) ** 2 + ((y - rng.uniform(0, MAP)) / 80) ** 2)).astype(np.float32)
                     for _ in range(N)])[:, None]
    src = torch.from_numpy(np.concatenate([i.reshape(-1) for i in imgs])).to(dev)
    pd = torch.from_numpy(prob).to(dev)
    say('render_probe: %d x %dx%d uint8, %d boxes per image at thickness %d, maps %d x %d' % (N, H, W, PER_IMAGE, THICKNESS, MAP, MAP))
    L, st = lib(), torch.cuda.current_stream().cuda_stream
    edges = Rn.stroke_edges(boxes, N)
    off = Pk.offsets([H * W * 3] * N)
    idesc = torch.from_numpy(np.stack([off[:-1], np.full(N, H), np.full(N, W)], 1).astype(np.int64)).to(dev)
    e = torch.from_numpy(edges).to(dev)
    out = torch.empty_like(src)
    img_bytes, map_bytes = src.numel(), pd.numel() * 4

    def strokes():
        check(L.dbn_draw_strokes(src.data_ptr(), out.data_ptr(), src.numel(), idesc.data_ptr(), N, e.data_ptr(), len(edges), THICKNESS, 255, 0, 0, st),
              'draw_strokes')

    def report(tag, t, floor_bytes, what):
        floor = floor_bytes / BW * 1e3
        say('%s (measured) %.3f ms   floor %.3f ms (%s at 8 TB/s)  %.0f%% of floor rate' % (tag, t, floor, what, 100 * floor / t))

    report('strokes dbn_draw_strokes, %d edges, copy + launch' % len(edges), time_launch(strokes, reps), 2 * img_bytes,
           '%.1f MB read + %.1f MB written by the copy' % (img_bytes / 1e6, img_bytes / 1e6))
    desc, coef, _ = Rn.overlay_plan(shapes, (MAP, MAP))
    d, c = torch.from_numpy(desc).to(dev), torch.from_numpy(coef).to(dev)
    mm = torch.empty(2 * N, dtype=torch.int32, device=dev)
    tab = Rn.colormap_table('inferno').astype(np.int64)
    lut = torch.from_numpy((tab[:, 0] | tab[:, 1] << 8 | tab[:, 2] << 16).astype(np.int32)).to(dev)
    common = (d.data_ptr(), c.data_ptr(), N, N * H * W, pd.data_ptr(), pd.numel(), MAP * MAP, MAP, 0, 0.0)

    def minmax():
        check(L.dbn_render_minmax(*common, mm.data_ptr(), st), 'render_minmax')

    def paint():
        check(L.dbn_render_paint(out.data_ptr(), out.data_ptr(), *common, mm.data_ptr(), lut.data_ptr(), 0.6, st), 'render_paint')

    report('minmax  dbn_render_minmax', time_launch(minmax, reps), map_bytes, '%.1f MB of maps' % (map_bytes / 1e6))
    report('paint   dbn_render_paint, in place', time_launch(paint, reps), 2 * img_bytes + map_bytes,
           '%.1f MB read + %.1f MB written + %.1f MB of maps' % (img_bytes / 1e6, img_bytes / 1e6, map_bytes / 1e6))
    t_e2e = time_wall(lambda: render_detections((src, shapes), pd, boxes, thickness=THICKNESS), max(5, reps // 3))
    say('e2e     render_detections from device inputs (measured, wall clock to a synchronised device): %.3f ms' % t_e2e)
    got = image_views(render_detections((src, shapes), pd, boxes, thickness=THICKNESS), shapes)[N - 1].cpu().numpy()
    t0 = time.perf_counter()
    ref = R.overlay_heatmap(R.draw_outlines(imgs[N - 1], boxes[N - 1], thickness=THICKNESS), prob[N - 1, 0])
    per = 1e3 * (time.perf_counter() - t0)
    assert np.array_equal(ref, got), 'the device picture differs from the numpy restatement'
    say('numpy   restatement per image (measured once, one core; a CPU stand-in, NOT cv2 / matplotlib): %.0f ms, %.0f ms for the %d '
        'images; device == numpy on that image' % (per, per * N, N))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'the probe times the device: it needs a GPU'
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(0)
    workload(say, rng, 32, 1280, 1280, args.reps)
    workload(say, rng, 1, 2160, 3840, args.reps)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
