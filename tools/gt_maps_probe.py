#!/usr/bin/env python3
"""Cost of building the DBNet ground-truth maps (db_text_minimal_amd.gt_maps) for one 16 x 640^2 step.

For 4-, 14- and 20-vertex polygons (12 per image), prints:
  host     plan_polygons (ignore rules, D, the two polygon offsets per polygon) for the 16 images, one core
  device   dbn_gt_maps alone (arguments already on the device), median of timed launches, against the write roofline
  numpy    tests/gt_maps_ref.py (the restatement pinned to the reference's own output) per image, same host
Usage: python tools/gt_maps_probe.py [--reps 50] [--out file] [--label name]
A deletion build (tools/flavour.sh gtmaps.hip -DDBN_GT_ABLATE=n, selected with DBN_LIB_PATH) times the kernel without the
threshold term (1) or without the fills (2); its maps then differ from numpy by construction.
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

from db_text_minimal_amd import gt_maps as G  # noqa: E402
import gt_maps_ref as R  # noqa: E402

N, S, PER_IMAGE = 16, 640, 12


def polygons(rng, V):
    """12 non-degenerate text polygons of V vertices: quads, or curved bands of V / 2 points per side."""
    out = []
    for _ in range(PER_IMAGE):
        cx, cy = rng.uniform(60, S - 60, 2)
        if V == 4:
            w, h, a = rng.uniform(60, 220), rng.uniform(16, 48), rng.uniform(-0.6, 0.6)
            c, s = np.cos(a), np.sin(a)
            p = np.array([[-w, -h], [w, -h], [w, h], [-w, h]]) / 2 @ np.array([[c, s], [-s, c]]) + [cx, cy]
        else:
            m = V // 2
            r, th, a0 = rng.uniform(60, 160), rng.uniform(16, 40), rng.uniform(0, 6.2)
            t = np.linspace(a0, a0 + rng.uniform(0.8, 2.0), m)
            p = np.concatenate([np.stack([cx + (r + th) * np.cos(t), cy + (r + th) * np.sin(t)], 1),
                                np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], 1)[::-1]])
        out.append(p + rng.uniform(-0.5, 0.5, p.shape))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--numpy-images', type=int, default=4)
    ap.add_argument('--out', default=None)
    ap.add_argument('--label', default='product library')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    lines = ['gt_maps_probe [%s]: %d x %d^2, %d polygons per image, device %s' % (a.label, N, S, PER_IMAGE, torch.cuda.get_device_name(0))]
    write_bytes = 4 * N * S * S * 4
    lines.append('write roofline: %.1f MB of maps -> %.1f us at 8 TB/s' % (write_bytes / 1e6, write_bytes / 8e12 * 1e6))
    for V in (4, 14, 20):
        rng = np.random.default_rng(V)
        polys = [polygons(rng, V) for _ in range(N)]
        t0 = time.perf_counter()
        plans = G.plan_polygons(polys, None, S)
        host_ms = (time.perf_counter() - t0) * 1e3
        verts, dist, meta, img_off, ixy, max_v, max_o = G.pack_plans(plans, S)
        args = [torch.from_numpy(x).to(dev) for x in (verts, dist, meta, img_off, ixy)]
        out = torch.empty((4, N, S, S), device=dev)
        L, stream = G.lib(), torch.cuda.current_stream().cuda_stream
        scale, tmin = float(np.float32(0.7 - 0.3)), float(np.float32(0.3))

        def launch():
            G.check(L.dbn_gt_maps(*[x.data_ptr() for x in args], N, len(meta), S, max_v, max_o, scale, tmin, out.data_ptr(), stream))
        for _ in range(5):
            launch()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
        dev_us = statistics.median(times)
        got = out.cpu().numpy()
        t0 = time.perf_counter()
        want = [R.maps_for_image(plans[i], S) for i in range(a.numpy_images)]
        np_ms = (time.perf_counter() - t0) * 1e3 / a.numpy_images
        same = all(np.array_equal(got[:, i], want[i]) for i in range(a.numpy_images))
        lines.append('V=%2d: device %7.1f us per step (min %.1f, %.2fx the write roofline, %.0f GB/s) | host plan %6.1f ms per step '
                     '(%.2f ms/polygon) | numpy restatement %6.1f ms per image = %.0f ms per step on one core | device == numpy: %s'
                     % (V, dev_us, min(times), dev_us / (write_bytes / 8e12 * 1e6), write_bytes / dev_us / 1e3, host_ms,
                        host_ms / (N * PER_IMAGE), np_ms, np_ms * N, same))
    txt = '\n'.join(lines)
    print(txt)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(txt + '\n')


if __name__ == '__main__':
    main()
