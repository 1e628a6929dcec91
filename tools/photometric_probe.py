#!/usr/bin/env python3
"""Times the photometric augmentation (db_text_minimal_amd.photometric, csrc/photometric.hip) on two sets of synthetic RGB "photo"
images (a ramp plus +-6 noise) already on the device:
  hd       16 images of 1280 x 720
  square   32 images of 1280 x 1280
and prints, per workload and case (each operation alone, the brightness + saturation recipe of the DBNet pipelines, all four):
the median of --reps runs after warm-up of the launches alone (device events around dbn_color_jitter_u8 with the records already
uploaded: the grey-sum memset and launch where a plan holds contrast, the apply launch), the bytes the kernels must move (every
image read and written once, read once more for the grey sums) per second and as a fraction of the 8 TB/s HBM figure, one
color_jitter_images call end to end on the host clock (records built and uploaded, synchronised), and the same plans through Pillow
(ImageEnhance and torchvision's HSV recipe on PIL images) in 16 worker processes, best of 5, with no upload or download counted.
Needs a GPU; there is no fallback.

  python tools/photometric_probe.py --workload hd|square [--reps 10] [--no-pillow] [--out FILE (appended)]
Run each workload as a step of its own under a time limit:
  timeout -k 10 300 python tools/photometric_probe.py --workload hd --out profiles/photometric_probe.txt && \\
  timeout -k 10 300 python tools/photometric_probe.py --workload square --out profiles/photometric_probe.txt
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOADS = {'hd': (16, 720, 1280), 'square': (32, 1280, 1280)}
HBM_PEAK = 8e12
CASES = [('brightness', {'brightness': 32 / 255}), ('contrast', {'contrast': 0.5}), ('saturation', {'saturation': 0.5}), ('hue', {'hue': 0.1}),
         ('brightness + saturation', {'brightness': 32 / 255, 'saturation': 0.5}),
         ('all four', {'brightness': 32 / 255, 'contrast': 0.5, 'saturation': 0.5, 'hue': 0.1})]


def images(kind):
    n, h, w = WORKLOADS[kind]
    rng = np.random.default_rng(5)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 0.2 + y * 0.1) % 256, (x * 0.05 + 64) % 200, (y * 0.3) % 256], -1)
    return [np.clip(np.roll(base, 37 * i, 1) + rng.integers(-6, 7, size=base.shape), 0, 255).astype(np.uint8) for i in range(n)]


_worker_images = None


def _pil_init(kind):
    global _worker_images
    _worker_images = images(kind)  # every worker makes its own copy once: no pixels travel with a job


def _pil_chunk(job):
    from PIL import Image, ImageEnhance
    acc = 0
    for index, plan in job:
        im = Image.fromarray(_worker_images[index])
        for name, f in plan:
            if name == 'brightness':
                im = ImageEnhance.Brightness(im).enhance(f)
            elif name == 'contrast':
                im = ImageEnhance.Contrast(im).enhance(f)
            elif name == 'saturation':
                im = ImageEnhance.Color(im).enhance(f)
            else:
                h, s, v = im.convert('HSV').split()
                np_h = np.array(h, dtype=np.uint8)
                np_h += np.array(int(f * 255)).astype(np.uint8)
                im = Image.merge('HSV', (Image.fromarray(np_h, 'L'), s, v)).convert('RGB')
        acc += int(np.asarray(im)[0, 0, 0])
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', choices=sorted(WORKLOADS), required=True)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--no-pillow', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    from db_text_minimal_amd import color_jitter_images, plan_color_jitter
    from db_text_minimal_amd import packed as Pk
    from db_text_minimal_amd import photometric as P
    from db_text_minimal_amd._lib import lib
    dev = torch.device('cuda')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def device_ms(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return float(np.median(ts))

    def host_ms(fn):
        fn()
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t)
        return float(np.median(ts)) * 1e3

    arrs = images(args.workload)
    n, h, w = WORKLOADS[args.workload]
    L, stream = lib(), torch.cuda.current_stream().cuda_stream
    sums = torch.empty(n, dtype=torch.int64, device=dev)
    shapes = [(h, w)] * n
    packed = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrs])).to(dev)
    out = torch.empty_like(packed)
    nbytes = packed.numel()
    pool = None
    if not args.no_pillow:
        import multiprocessing as mp
        pool = mp.get_context('spawn').Pool(16, initializer=_pil_init, initargs=(args.workload, ))
    say('== photometric_probe %s: %d x %d x %d RGB, %.1f MB, median of %d, %s' % (args.workload, n, w, h, nbytes / 1e6, args.reps,
                                                                                 torch.cuda.get_device_name(0)))
    say('%-24s %9s %9s %8s %7s %9s %12s' % ('case', 'device ms', 'moved MB', 'GB/s', 'of HBM', 'call ms', 'Pillow x16 ms'))
    for name, kw in CASES:
        plans = plan_color_jitter(n, np.random.RandomState(1), **kw)
        moved = nbytes * (3 if 'contrast' in kw else 2)
        hdesc = P.plan_records(shapes, plans)
        desc = Pk.upload(hdesc, dev)

        def launches():
            P.check(L.dbn_color_jitter_u8(packed.data_ptr(), out.data_ptr(), nbytes, hdesc.ctypes.data, desc.data_ptr(), n, sums.data_ptr(), stream),
                    'color_jitter_u8')

        ms = device_ms(launches)
        call_ms = host_ms(lambda: color_jitter_images(packed, shapes, plans, out=out))
        pil = ''
        if pool is not None:
            jobs = [list(zip(range(i, n, 16), plans[i::16])) for i in range(16)]
            for _ in range(3):  # start-up, imports, every worker's own images: a worker that is late leaves its jobs to others once
                pool.map(_pil_chunk, jobs, chunksize=1)
            best = 1e9
            for _ in range(5):
                t = time.perf_counter()
                pool.map(_pil_chunk, jobs, chunksize=1)
                best = min(best, time.perf_counter() - t)
            pil = '%12.1f' % (best * 1e3)
        say('%-24s %9.3f %9.1f %8.1f %6.1f%% %9.3f %s' % (name, ms, moved / 1e6, moved / ms / 1e6, 100 * moved / (ms * 1e-3) / HBM_PEAK, call_ms, pil))
    if pool is not None:
        pool.close()
        pool.join()
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()
