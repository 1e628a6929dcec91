#!/usr/bin/env python3
"""Cost of the polygon word crops on the device (db_text_minimal_amd.word_crops.rectify_words) for one dense inference
batch, beside crop_words on the same count: 32 images of 1280 x 1280 with 300 curved words each, 9 600 polygons of 20
vertices (10 a side, as an unclipped detection or a Total-Text annotation has them), 9 600 crops of 32 x 100.

Prints:
  host     polygon_ribbons for the batch (dbn_polygon_ribbons, one call, up to 16 threads), ends='auto' (the search) and
           ends='half' (no search), median
  ribbons  dbn_polygon_ribbons_device alone (vertices and offsets already on the device), both ends, the same way as the
           launches below, and its knots, valid flags, ends and info against the host's: equal or not
  largest  one polygon of 256 vertices at 64 segments, device launch and host call: one workgroup owns a polygon, so this is
           the latency floor of the kernel's shape
  device   dbn_rectify_u8 alone (descriptors and knots already on the device), median of timed launches after warm-up
           (device events), against its byte floor at 8 TB/s: the crops written plus the source bytes inside the polygons
           (their shoelace areas, 3 bytes per pixel)
  boxes    dbn_warp_perspective_u8 alone on the same number of boxes (each polygon's end-to-end rectangle), the same way
  e2e      rectify_words from a device batch: selection, the ribbons (ribbons='host' and ribbons='device'), the copies and
           the launch, wall clock to a synchronised device, median; and whether both gave the same crops
  check    device == the numpy restatement tests/rectify_ref.py on the crops it samples
Usage: python tools/rectify_probe.py [--reps 50] [--out file]
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

from db_text_minimal_amd import perspective_maps, polygon_ribbons, polygon_ribbons_device, rectify_words  # noqa: E402
from db_text_minimal_amd import word_crops as Wc  # noqa: E402
from db_text_minimal_amd import packed as Pk  # noqa: E402
from db_text_minimal_amd._lib import check, lib  # noqa: E402
import rectify_ref as R  # noqa: E402
from crop_probe import time_launch, time_wall  # noqa: E402

N, H, W, PER_IMAGE, SIDE, SIZE, SEGMENTS = 32, 1280, 1280, 300, 10, (32, 100), 32
BW = 8e12  # bytes / s


def polygons_for(rng):
    """per image 300 arcs: centre line 60-300 px long on a circle of radius 150-2000 px (either way up), 12-50 px wide,
    at any angle, 10 points a side, rounded to integers as the detector gives them; (polygons, their rectangles)"""
    polys, boxes = [], []
    for _ in range(N):
        ps, bs = [], []
        for _ in range(PER_IMAGE):
            length, width, radius = rng.uniform(60, 300), rng.uniform(12, 50), rng.uniform(150, 2000) * rng.choice([-1, 1])
            a = np.linspace(-0.5, 0.5, SIDE) * length / radius
            top = np.stack([(radius + width / 2) * np.sin(a), radius - (radius + width / 2) * np.cos(a)], 1)
            bot = np.stack([(radius - width / 2) * np.sin(a), radius - (radius - width / 2) * np.cos(a)], 1)
            p = np.concatenate([top, bot[::-1]])  # the upper side from the left, the lower side back
            t = rng.uniform(-0.5, 0.5)
            p = p @ np.array([[np.cos(t), np.sin(t)], [-np.sin(t), np.cos(t)]]) + rng.uniform(250, W - 250, 2)
            p = np.round(p).astype(np.int64)
            ps.append(p)
            bs.append(np.stack([p[0], p[SIDE - 1], p[SIDE], p[-1]]))
        polys.append(ps)
        boxes.append(np.array(bs).astype(np.int16))
    return polys, boxes


def shoelace(p):
    x, y = p[:, 0].astype(np.float64), p[:, 1].astype(np.float64)
    return 0.5 * abs((x * np.roll(y, -1) - np.roll(x, -1) * y).sum())


def time_device_ribbons(L, polys, S, half, dev, stream, reps):
    """dbn_polygon_ribbons_device alone on polygons already on the device -> (median ms, its outputs on the host)"""
    K = len(polys)
    xy = torch.from_numpy(np.concatenate(polys).astype(np.float64)).to(dev)
    offs = torch.from_numpy(Pk.offsets([len(p) for p in polys])).to(dev)
    knots, valid = torch.empty((K, S + 1, 4), device=dev, dtype=torch.int32), torch.empty(K, device=dev, dtype=torch.uint8)
    found, info = torch.empty((K, 2), device=dev, dtype=torch.int32), torch.empty((K, 3), device=dev, dtype=torch.float64)

    def launch():
        check(L.dbn_polygon_ribbons_device(xy.data_ptr(), offs.data_ptr(), K, xy.shape[0], S, half, knots.data_ptr(), valid.data_ptr(),
                                           found.data_ptr(), info.data_ptr(), stream), 'polygon_ribbons_device')

    t = time_launch(launch, reps)
    return t, (knots.cpu().numpy(), valid.cpu().numpy(), found.cpu().numpy(), info.cpu().numpy())


def same_ribbons(got, polys, S, ends):
    knots, valid, info = polygon_ribbons(polys, S, ends, return_info=True)
    want = (knots, valid, info['ends'], np.stack([info['E'], info['width'], info['length']], 1))
    return all(np.array_equal(g.view(np.int64) if g.dtype == np.float64 else g, w.view(np.int64) if w.dtype == np.float64 else w)
               for g, w in zip(got, want))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'the probe times the device: it needs a GPU'
    dev = torch.device('cuda')
    rng = np.random.default_rng(0)
    imgs = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(N)]
    polys, boxes = polygons_for(rng)
    shapes = [(H, W)] * N
    src = torch.from_numpy(np.concatenate([i.reshape(-1) for i in imgs])).to(dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    kept, index = Wc.select_polygons(polys)
    K = len(kept)
    h, w = SIZE
    say('rectify_probe: %d x %dx%d uint8, %d polygons of %d vertices per image, %d crops of %d x %d, %d segments'
        % (N, H, W, PER_IMAGE, 2 * SIDE, K, h, w, SEGMENTS))

    for ends in ('auto', 'half'):
        ts = []
        for _ in range(max(3, args.reps // 10)):
            t0 = time.perf_counter()
            knots_e, valid_e = polygon_ribbons(kept, SEGMENTS, ends)
            ts.append(1e3 * (time.perf_counter() - t0))
        say("host   polygon_ribbons ends='%s' (measured, up to 16 threads of %d cores): %.1f ms for %d polygons (median of %d), %d valid"
            % (ends, os.cpu_count(), statistics.median(ts), K, len(ts), int(valid_e.sum())))
        if ends == 'auto':
            knots, valid = knots_e, valid_e

    L = lib()
    stream = torch.cuda.current_stream().cuda_stream
    for ends in ('auto', 'half'):
        t, got = time_device_ribbons(L, kept, SEGMENTS, int(ends == 'half'), dev, stream, args.reps)
        say("ribbons polygon_ribbons_device ends='%s' (measured, the launch alone): %.3f ms for %d polygons; knots, valid, ends and info %s the host's"
            % (ends, t, K, 'EQUAL' if same_ribbons(got, kept, SEGMENTS, ends) else 'DIFFER FROM'))
    big = [np.round(np.stack([600 + 500 * np.cos(a) * (1 + 0.1 * np.sin(5 * a)), 600 + 300 * np.sin(a)], 1) * 4) / 4
           for a in [np.linspace(0, 2 * np.pi, 256, endpoint=False)]]
    t, got = time_device_ribbons(L, big, 64, 0, dev, stream, max(5, args.reps // 5))
    t0 = time.perf_counter()
    same = same_ribbons(got, big, 64, 'auto')
    say("largest one polygon of 256 vertices, 64 segments, ends='auto' (measured): device launch %.3f ms, host call %.1f ms (one thread, with "
        "its early exit); %s" % (t, 1e3 * (time.perf_counter() - t0), 'EQUAL' if same else 'DIFFERENT'))

    off = Pk.offsets([H * W * 3] * N)
    desc = np.stack([off[index[:, 0]], np.full(K, H, np.int64), np.full(K, W, np.int64)], 1)
    d, kn, va = torch.from_numpy(desc).to(dev), torch.from_numpy(knots).to(dev), torch.from_numpy(valid).to(dev)
    crops = torch.empty((K, h, w, 3), device=dev, dtype=torch.uint8)

    def launch():
        check(L.dbn_rectify_u8(src.data_ptr(), src.numel(), d.data_ptr(), kn.data_ptr(), va.data_ptr(), K, SEGMENTS, h, w, crops.data_ptr(),
                               crops.numel(), stream), 'rectify_u8')

    t = time_launch(launch, args.reps)
    out_bytes = K * h * w * 3
    src_bytes = int(sum(shoelace(p) for p in kept)) * 3
    floor = (out_bytes + src_bytes) / BW * 1e3
    say('device rectify_u8 (measured) %.3f ms   floor %.3f ms (%.1f MB written + %.1f MB of source inside the polygons at 8 TB/s)  '
        '%.0f%% of floor rate' % (t, floor, out_bytes / 1e6, src_bytes / 1e6, 100 * floor / t))

    quads, _ = Wc.select_boxes(boxes)
    assert len(quads) == K
    _, inv = perspective_maps(quads, SIZE)
    m = torch.from_numpy(inv).to(dev)
    box_crops = torch.empty((K, h, w, 3), device=dev, dtype=torch.uint8)

    def launch_boxes():
        check(L.dbn_warp_perspective_u8(src.data_ptr(), src.numel(), d.data_ptr(), m.data_ptr(), K, h, w, box_crops.data_ptr(), box_crops.numel(),
                                        stream), 'warp_perspective_u8')

    say('boxes  warp_perspective_u8 on the same count (measured) %.3f ms' % time_launch(launch_boxes, args.reps))
    for how in ('host', 'device'):
        t_e2e = time_wall(lambda: rectify_words((src, shapes), polys, SIZE, ribbons=how), max(3, args.reps // 10))
        say("e2e    rectify_words(ribbons='%s') from a device batch (measured, wall clock to a synchronised device): %.1f ms" % (how, t_e2e))

    got, _ = rectify_words((src, shapes), polys, SIZE)
    on_device, _ = rectify_words((src, shapes), polys, SIZE, ribbons='device')
    say("check  ribbons='device' and ribbons='host' gave %s crops (%d x %d x %d x 3 bytes)" % (('EQUAL' if torch.equal(on_device, got) else 'DIFFERENT', ) + tuple(got.shape[:3])))
    got = got.cpu().numpy()
    sample = np.linspace(0, K - 1, 40).astype(np.int64)
    for j in sample:
        assert np.array_equal(R.rectify(imgs[index[j, 0]], knots[j], valid[j], h, w), got[j]), 'device crop %d differs from the numpy restatement' % j
    say('check  device == numpy restatement on %d crops, %d of them not empty' % (len(sample), sum(bool(got[j].any()) for j in sample)))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
