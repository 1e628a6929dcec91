#!/usr/bin/env python3
"""Times the JPEG encode (db_text_minimal_amd.jpeg: forward_coefficients on the device, entropy_encode on the host) on the two
workloads the pipeline ends in, both 4:2:0 at quality 75:
  render   32 rendered images of 1280 x 1280 (render_detections' output)
  crops    9 600 word crops of 32 x 100 (crop_words' output)
and prints, per workload: the device stage (both kernels, device events) against its algorithmic bytes (3 B per pixel in,
2 B per coefficient out), the coefficient copy to pinned memory, the host stage at 1 and 16 threads, images/s end to end,
and Pillow encoding the same arrays in 16 worker processes (when Pillow is installed); then the device Huffman coder
(csrc/jpeg_huff.hip): entropy_encode_device on coefficients that stayed on the device and the whole entropy='device' call,
each against the host path at 16 threads in the same run, and the total file bytes with and without optimize.  Needs a
GPU; there is no fallback.

  python tools/jpeg_encode_probe.py [--workload render|crops|both] [--reps 5] [--no-pillow]
Run each workload as a step of its own under a time limit, e.g.
  timeout -k 10 300 python tools/jpeg_encode_probe.py --workload render && timeout -k 10 300 python tools/jpeg_encode_probe.py --workload crops
"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from db_text_minimal_amd import jpeg as J  # noqa: E402
from db_text_minimal_amd import packed as Pk  # noqa: E402


def images(kind):
    """seeded content with text-like strokes over smooth colour: uint8 [N, H, W, 3]"""
    rng = np.random.default_rng(3)
    n, h, w = (32, 1280, 1280) if kind == 'render' else (9600, 32, 100)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 0.2 + y * 0.1) % 256, (x * 0.05 + 64) % 256, (y * 0.3) % 256], -1).astype(np.uint8)
    out = np.empty((n, h, w, 3), np.uint8)
    for i in range(n):
        img = np.roll(base, int(rng.integers(0, w)), 1).copy()
        for _ in range(max(4, h * w // 4000)):
            x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
            img[y0:y0 + int(rng.integers(1, 5)), x0:x0 + int(rng.integers(4, 60))] = 0
        out[i] = img
    return out


def _pil_chunk(arrs):
    from PIL import Image
    n = 0
    for a in arrs:
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, 'JPEG')
        n += buf.tell()
    return n


def pillow_rate(arr, workers=16):
    import multiprocessing as mp
    chunks = [arr[i::workers] for i in range(workers)]
    with mp.get_context('spawn').Pool(workers) as pool:
        pool.map(_pil_chunk, [c[:1] for c in chunks])  # start the workers and import PIL
        t0 = time.perf_counter()
        pool.map(_pil_chunk, chunks)
        dt = time.perf_counter() - t0
    return len(arr) / dt, dt


def median(v):
    return float(np.median(v))


def probe(kind, reps, pillow):
    arr = images(kind)
    dev = torch.device('cuda')
    x = torch.from_numpy(arr).to(dev)
    n, h, w, _ = arr.shape
    items = [(i * h * w * 3, h, w, 3) for i in range(n)]
    tables = J.quant_tables(75)
    hdesc, qtabs, total, tp, tf = J.forward_plan(items, '420', tables)
    desc, qt, a, b = (Pk.upload(v, dev) for v in (hdesc, qtabs.view(np.int16), tp, tf))
    coef = torch.empty(total, dtype=torch.int16, device=dev)
    planes = torch.empty(total, dtype=torch.uint8, device=dev)
    host = torch.empty(total, dtype=torch.int16, pin_memory=True)
    stream = torch.cuda.current_stream(dev)

    def launch():
        J.check(J.lib().dbn_jpeg_forward(x.data_ptr(), x.numel(), desc.data_ptr(), qt.data_ptr(), n, a.data_ptr(), len(tp), b.data_ptr(), len(tf),
                                         planes.data_ptr(), coef.data_ptr(), total, stream.cuda_stream), 'jpeg_forward')
    for _ in range(3):
        launch()
        host.copy_(coef, non_blocking=True)
    torch.cuda.synchronize()
    kern, copy = [], []
    for _ in range(reps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        launch()
        e[1].record()
        host.copy_(coef, non_blocking=True)
        e[2].record()
        torch.cuda.synchronize()
        kern.append(e[0].elapsed_time(e[1]))
        copy.append(e[1].elapsed_time(e[2]))
    obj = J.forward_coefficients(x).wait()
    hostt = {}
    for t in (1, 16):
        ts = []
        for _ in range(max(2, reps // 2)):
            t0 = time.perf_counter()
            streams = J.entropy_encode(obj, threads=t)
            ts.append((time.perf_counter() - t0) * 1e3)
        hostt[t] = median(ts)
    e2e = []
    for _ in range(max(2, reps // 2)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        streams = J.encode_jpeg_batch(x)
        e2e.append(time.perf_counter() - t0)
    # the device coder against the host path (the coefficient copy is part of the host path, not of the device one)
    def timed(f):
        ts = []
        for _ in range(max(3, reps // 2 + 1)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = f()
            ts.append((time.perf_counter() - t0) * 1e3)
        return median(ts[1:]), r
    dobj = J.forward_coefficients(x, host_copy=False)
    dev_ms, dstreams = timed(lambda: J.entropy_encode_device(dobj))
    dev_opt_ms, dopt = timed(lambda: J.entropy_encode_device(dobj, optimize=True))
    host_opt_ms, hopt = timed(lambda: J.entropy_encode(obj, threads=16, optimize=True))
    e2e_dev_ms, s2 = timed(lambda: J.encode_jpeg_batch(x, entropy='device'))
    e2e_host_ms, s1 = timed(lambda: J.encode_jpeg_batch(x))
    e2e_dev_opt_ms, _ = timed(lambda: J.encode_jpeg_batch(x, entropy='device', optimize=True))
    e2e_host_opt_ms, _ = timed(lambda: J.encode_jpeg_batch(x, optimize=True))
    assert dstreams == streams and s2 == s1 and dopt == hopt
    device = dict(device_entropy_ms=dev_ms, device_entropy_optimize_ms=dev_opt_ms, host_entropy_optimize_ms_16_threads=host_opt_ms,
                  end_to_end_device_ms=e2e_dev_ms, end_to_end_host_ms=e2e_host_ms, end_to_end_device_optimize_ms=e2e_dev_opt_ms,
                  end_to_end_host_optimize_ms=e2e_host_opt_ms, jpeg_bytes_optimize=sum(len(d) for d in dopt),
                  device_to_host_bytes_device_path=sum(len(d) for d in dstreams), device_to_host_bytes_host_path=total * 2)
    bytes_alg = n * h * w * 3 + total * 2
    res = dict(workload=kind, images=n, height=h, width=w, coefficients=total, algorithmic_bytes=bytes_alg,
               device_stage_ms=median(kern), device_stage_GBps=bytes_alg / median(kern) / 1e6, coefficient_copy_ms=median(copy),
               coefficient_copy_GBps=total * 2 / median(copy) / 1e6, host_stage_ms_1_thread=hostt[1], host_stage_ms_16_threads=hostt[16],
               end_to_end_images_per_s=n / median(e2e), end_to_end_ms=median(e2e) * 1e3, jpeg_bytes=sum(len(s) for s in streams),
               planes_workgroups=len(tp), fdct_workgroups=len(tf), **device)
    if pillow:
        try:
            rate, dt = pillow_rate(arr)
            res.update(pillow_16_processes_images_per_s=rate, pillow_16_processes_ms=dt * 1e3)
        except ImportError:
            res.update(pillow_16_processes_images_per_s=None)
    print(json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--workload', default='both', choices=('render', 'crops', 'both'))
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-pillow', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('jpeg_encode_probe needs a GPU')
    for kind in (('render', 'crops') if args.workload == 'both' else (args.workload, )):
        probe(kind, args.reps, not args.no_pillow)


if __name__ == '__main__':
    main()
