"""Time the detection scoring of csrc/det_eval.hip on a synthetic batch.

    python tools/eval_probe.py [--reps 20] [--out profiles/r10_eval_probe.txt]

Batch: 16 images, each 64 GT polygons of 16 vertices and 128 detections of 64 vertices on a 1280^2 canvas (half of the
detections jittered copies of GTs, half elsewhere), fp64 non-integer coordinates.  It reports
  overlap   median time of dbn_det_eval_overlaps (both launches; HIP events on the current stream, buffers uploaded once),
            with the bounding-box cull (the product) and without it (every pair through the boundary formula)
  pairs     GT x detection pairs and how many survive the cull
  host      median wall time of dbn_det_eval_match_host for the batch, IoU and DetEval protocols (ctypes call only)
  batch     median wall time of DetectionIoUEvaluator.evaluate_batch end to end (packing, upload, launches, copy, matching)
No target is set: these are the first numbers for this path."""
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

from db_text_minimal_amd import det_eval as DE  # noqa: E402
from db_text_minimal_amd._lib import check, lib  # noqa: E402


def blob(rng, cx, cy, rx, ry, n):
    a = np.sort(rng.uniform(0, 2 * math.pi, n))
    r = rng.uniform(0.85, 1.0, n)
    return np.stack([cx + rx * r * np.cos(a), cy + ry * r * np.sin(a)], 1)


def batch(seed=0, N=16, G=64, D=128, S=1280.0):
    rng = np.random.default_rng(seed)
    gts, dets = [], []
    for _ in range(N):
        cs = [(rng.uniform(60, S - 60), rng.uniform(30, S - 30), rng.uniform(20, 60), rng.uniform(8, 20)) for _ in range(G)]
        gts.append([blob(rng, cx, cy, rx, ry, 16) for cx, cy, rx, ry in cs])
        d = [blob(rng, cx + rng.uniform(-4, 4), cy + rng.uniform(-3, 3), rx * rng.uniform(0.9, 1.1), ry * rng.uniform(0.9, 1.1), 64)
             for cx, cy, rx, ry in cs[:D // 2]]
        d += [blob(rng, rng.uniform(60, S - 60), rng.uniform(30, S - 30), rng.uniform(20, 60), rng.uniform(8, 20), 64) for _ in range(D - len(d))]
        dets.append(d)
    return gts, dets


def time_launch(gts, dets, cull, reps, dev):
    verts, poff, img, n_pairs = DE._pack(gts, dets)
    P = len(poff) - 1
    dv, dp, di = (torch.from_numpy(a).to(dev) for a in (verts, poff, img))
    ws = torch.empty(int(lib().dbn_det_eval_ws_bytes(P)), dtype=torch.uint8, device=dev)
    inter = torch.empty(n_pairs, dtype=torch.float64, device=dev)
    area = torch.empty(P, dtype=torch.float64, device=dev)
    ns = torch.empty(P, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev)
    ts = []
    for i in range(reps + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        check(lib().dbn_det_eval_overlaps(dv.data_ptr(), dp.data_ptr(), P, di.data_ptr(), len(gts), n_pairs, cull, ws.data_ptr(), inter.data_ptr(),
                                          area.data_ptr(), ns.data_ptr(), st.cuda_stream), 'det_eval_overlaps')
        e1.record(st)
        e1.synchronize()
        if i >= 3:
            ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), n_pairs, inter.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    gts, dets = batch()
    lines = ['detection scoring probe: 16 images x 64 GT (16 vertices) x 128 detections (64 vertices), fp64, %s' % torch.cuda.get_device_name(dev)]
    t_cull, n_pairs, inter = time_launch(gts, dets, 1, args.reps, dev)
    t_all, _, inter_all = time_launch(gts, dets, 0, args.reps, dev)
    # the cull changes which pairs are computed, not their values beyond rounding of pairs that only touch
    kept = 0
    verts, poff, img, _ = DE._pack(gts, dets)
    for g0, G, d0, D, po in img.tolist():
        for g in range(G):
            a = verts[poff[g0 + g]:poff[g0 + g + 1]]
            for d in range(D):
                b = verts[poff[d0 + d]:poff[d0 + d + 1]]
                kept += not (a[:, 0].max() <= b[:, 0].min() or b[:, 0].max() <= a[:, 0].min() or a[:, 1].max() <= b[:, 1].min()
                             or b[:, 1].max() <= a[:, 1].min())
    dmax = float(np.abs(inter - inter_all).max())
    lines.append('overlap   cull on  %.3f ms   cull off  %.3f ms   (median of %d; both launches)' % (t_cull, t_all, args.reps))
    lines.append('pairs     %d, %d with overlapping bounding boxes (%.2f %%); max |cull on - cull off| = %.3g' %
                 (n_pairs, kept, 100.0 * kept / n_pairs, dmax))
    ov = DE.polygon_overlaps(gts, dets, dev)
    ig = [[i % 10 == 0 for i in range(len(g))] for g in gts]
    cd = ([DE._centre_diag(p) for ps in gts for p in ps], [DE._centre_diag(p) for ps in dets for p in ps])
    for name, proto, prm, c in (('iou', DE.IOU, [0.5, 0.5], (None, None)), ('deteval', DE.DETEVAL, [0.8, 0.4, 1, 1.0, 0.8, 1.0], cd)):
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            DE.match(proto, prm, ov, ig, *c)
            ts.append(time.perf_counter() - t0)
        lines.append('host      %-8s %.3f ms (median wall time of the match call, %d reps)' % (name, 1e3 * statistics.median(ts), args.reps))
    ev = DE.DetectionIoUEvaluator()
    g_in = [[{'points': p, 'ignore': i % 10 == 0} for i, p in enumerate(g)] for g in gts]
    p_in = [[{'points': p, 'ignore': False} for p in d] for d in dets]
    ts = []
    for _ in range(max(3, args.reps // 4)):
        t0 = time.perf_counter()
        res = ev.evaluate_batch(g_in, p_in, device=dev)
        ts.append(time.perf_counter() - t0)
    lines.append('batch     evaluate_batch (IoU) %.1f ms end to end; combined %s' % (1e3 * statistics.median(ts), ev.combine_results(res)))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
