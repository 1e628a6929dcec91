"""Time detect_boxes (csrc/detect.hip + dbn_detect_host) on synthetic probability maps.

    python tools/detect_probe.py [--reps 10] [--out profiles/r08_detect_probe.txt]
    python tools/detect_probe.py --poly [--reps 10] [--out profiles/r09_detect_poly_probe.txt]

For 16 x 640^2 and 32 x 1280^2 maps of each kind (about 50 text blobs per image; a spiral; a checkerboard) it reports
  device   median time of the dbn_detect launch sequence (HIP events on the current stream, buffers preallocated)
  host     median wall time of the host stage (dbn_detect_host, one call per batch)
  floor    one pass over the fp32 probability map (channel 0) at 8 TB/s, and the device stage's own bytes per pixel
  d2h      bytes copied to the host (records + counts) against the 4 B/px fp32 map the host route copies
No target is set: these are the first numbers for this path.

--poly times detect_polygons (dbn_detect_poly + dbn_detect_poly_host) on the same maps instead:
  contour  median time of dbn_detect_poly minus median time of dbn_detect: the contour launches alone
  rounds   pointer-jumping rounds run / launched, cracks and compressed vertices per image
  host     median wall time of the host stage (dbn_detect_poly_host, one call per batch)
  d2h      bytes of the two copies: the fixed-size table, then exactly the packed vertices
  serial   for the spiral: a serial walk's estimate for its one border, at 94-250 ns per dependent step"""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from db_text_minimal_amd import postprocess as P  # noqa: E402
from db_text_minimal_amd._lib import check, lib  # noqa: E402

# global-memory bytes per pixel the device stage moves by construction (reads + writes, excluding the hull kernel's
# bounding-box scans and the per-run atomics): tile_label 4 (pred) + 1 + 4 (bitmap, L); flatten >= 4 + 4 (L, labels);
# row_count 4 + 1; rank 4 + 1; run_stats 4 + 4 + 1 (labels, pred, bitmap at run ends, bounded by 1); tree 4 (labels)
DESIGN_BYTES_PER_PX = 4 + 1 + 4 + 4 + 4 + 5 + 5 + 9 + 4


def blobs(H, W, n, rng):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    inside = np.zeros((H, W), bool)
    for _ in range(n):
        cx, cy, a = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(0, math.pi)
        L, T = rng.uniform(3, W / 16), rng.uniform(1.5, H / 60)
        u = (xx - cx) * math.cos(a) + (yy - cy) * math.sin(a)
        v = -(xx - cx) * math.sin(a) + (yy - cy) * math.cos(a)
        inside |= (np.abs(u) <= L) & (np.abs(v) <= T)
    return inside


def spiral(H, W):
    bm = np.zeros((H, W), bool)
    y, x, t, l, b, r = 0, 0, 0, 0, H - 1, W - 1
    while t <= b and l <= r:
        bm[y, x:r + 1] = True
        x = r
        bm[y:b + 1, x] = True
        y = b
        bm[y, l:x + 1] = True
        x = l
        if y > t + 2:
            bm[t + 2:y + 1, x] = True
            y = t + 2
        t, l, b, r = t + 2, l + 2, b - 2, r - 2
    return bm


def make(kind, N, S, rng):
    if kind == 'blobs':
        bms = [blobs(S, S, 50, rng) for _ in range(min(N, 4))]
    elif kind == 'spiral':
        bms = [spiral(S, S)]
    else:
        yy, xx = np.mgrid[0:S, 0:S]
        bms = [((xx + yy) % 2) == 0]
    maps = np.empty((N, 2, S, S), np.float32)
    for n in range(N):
        bm = bms[n % len(bms)]
        maps[n, 0] = np.where(bm, rng.uniform(0.75, 1.0, (S, S)), rng.uniform(0, 0.28, (S, S)))
        maps[n, 1] = 0
    return torch.from_numpy(maps).cuda()


def probe(kind, N, S, reps, M=1000):
    rng = np.random.default_rng(0)
    preds = make(kind, N, S, rng)
    L = lib()
    ws = torch.empty(L.dbn_detect_ws_bytes(N, S, S, M), device='cuda', dtype=torch.uint8)
    labels = torch.empty((N, S, S), device='cuda', dtype=torch.int32)
    rec_bytes = N * M * P.REC_DTYPE.itemsize
    out = torch.empty(rec_bytes + 4 * N, device='cuda', dtype=torch.uint8)
    st = torch.cuda.current_stream().cuda_stream

    def launch():
        check(L.dbn_detect(preds.data_ptr(), N, 2, S, S, 0.3, M, ws.data_ptr(), labels.data_ptr(), out.data_ptr(), out.data_ptr() + rec_bytes,
                           st), 'detect')

    for _ in range(2):
        launch()
    torch.cuda.synchronize()
    dev = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        dev.append(a.elapsed_time(b) * 1e3)
    host_buf = out.cpu().numpy()
    recs = host_buf[:rec_bytes].view(P.REC_DTYPE).reshape(N, M)
    counts = host_buf[rec_bytes:].view(np.int32).copy()
    hst = []
    for _ in range(max(3, reps // 2)):
        t0 = time.perf_counter()
        boxes, scores = P.detect_host(recs, counts, S, S)
        hst.append((time.perf_counter() - t0) * 1e6)
    kept = int((scores > 0).sum())
    map_bytes = N * S * S * 4
    floor_us = map_bytes / 8e12 * 1e6
    d2h = rec_bytes + 4 * N
    return ('%-12s %2d x %4d^2  device %9.1f us  host %9.1f us  candidates/img %6d  boxes %5d  | map pass floor %6.1f us (x%.0f)  '
            'design %d B/px vs 4  | d2h %.2f MB vs %.1f MB' % (kind, N, S, statistics.median(dev), statistics.median(hst),
                                                             int(np.minimum(counts, M).mean()), kept, floor_us,
                                                             statistics.median(dev) / floor_us, DESIGN_BYTES_PER_PX, d2h / 1e6,
                                                             map_bytes / 1e6))


def timed(launch, reps):
    for _ in range(2):
        launch()
    torch.cuda.synchronize()
    dev = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        dev.append(a.elapsed_time(b) * 1e3)
    return statistics.median(dev)


def probe_poly(kind, N, S, reps, M=1000):
    rng = np.random.default_rng(0)
    preds = make(kind, N, S, rng)
    L = lib()
    ws = torch.empty(L.dbn_detect_ws_bytes(N, S, S, M), device='cuda', dtype=torch.uint8)
    pws = torch.empty(L.dbn_detect_poly_ws_bytes(N, S, S, M), device='cuda', dtype=torch.uint8)
    labels = torch.empty((N, S, S), device='cuda', dtype=torch.int32)
    o_counts, o_nv, o_voff, o_info, size = P._poly_table_layout(N, M)
    table = torch.empty(size, device='cuda', dtype=torch.uint8)
    verts = torch.empty((L.dbn_detect_poly_verts_cap(N, S, S), 2), device='cuda', dtype=torch.int16)
    st = torch.cuda.current_stream().cuda_stream

    def launch_detect():
        check(L.dbn_detect(preds.data_ptr(), N, 2, S, S, 0.3, M, ws.data_ptr(), labels.data_ptr(), table.data_ptr(), table.data_ptr() + o_counts,
                           st), 'detect')

    def launch_poly():
        check(L.dbn_detect_poly(preds.data_ptr(), N, 2, S, S, 0.3, M, ws.data_ptr(), pws.data_ptr(), labels.data_ptr(), table.data_ptr(),
                                verts.data_ptr(), st), 'detect_poly')

    t_det = timed(launch_detect, reps)
    t_poly = timed(launch_poly, reps)
    host = table.cpu().numpy()
    info = host[o_info:].view(np.int32).copy()
    c = dict(recs=host[:o_counts].view(P.REC_DTYPE).reshape(N, M), counts=host[o_counts:o_nv].view(np.int32).copy(),
             nv=host[o_nv:o_voff].view(np.int32).reshape(N, M).copy(), voff=host[o_voff:o_info].view(np.int32).reshape(N, M).copy(),
             verts=verts[:int(info[0])].cpu().numpy())
    hst = []
    for _ in range(max(3, reps // 2)):
        t0 = time.perf_counter()
        res = P.detect_poly_host(c, S, S)
        hst.append((time.perf_counter() - t0) * 1e6)
    kept = sum(len(r[0]) for r in res)
    d2h = size + 4 * int(info[0])
    line = ('%-8s %2d x %4d^2  detect %9.1f us  poly %9.1f us  contour %9.1f us  rounds %2d/%2d  cracks/img %8d  verts/img %7d  '
            'host %9.1f us  polygons %5d  | d2h %.2f MB + %.2f MB' % (kind, N, S, t_det, t_poly, t_poly - t_det, info[2], info[3], info[1] // N,
                                                                 info[0] // N, statistics.median(hst), kept, size / 1e6,
                                                                 4 * int(info[0]) / 1e6))
    if kind == 'spiral':
        longest = int(info[1]) // N  # one candidate per image
        line += '  | serial walk of its border: %.0f-%.0f ms per image' % (longest * 94e-6, longest * 250e-6)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--poly', action='store_true', help='time detect_polygons instead of detect_boxes')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = ['detect_probe%s: median of %d launches; %s' % (' --poly' if a.poly else '', a.reps, torch.cuda.get_device_name(0))]
    for N, S in ((16, 640), (32, 1280)):
        for kind in ('blobs', 'spiral', 'checker'):
            lines.append(probe_poly(kind, N, S, a.reps) if a.poly else probe(kind, N, S, a.reps))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
