#!/usr/bin/env python3
"""Times the degradation augmentation (db_text_minimal_amd.degrade, csrc/degrade.hip) on 32 synthetic RGB "photo" images of
1280 x 1280 (a ramp plus +-6 noise, the photometric probe's) already on the device, every image with the same plan, for
  blur at sigma = 1, 3 and 8 (r = 4, 12, 32), noise alone (scale 10, per channel), and blur at sigma = 1 with that noise,
and, in the same run, one adjust_brightness blend of the same batch (dbn_color_jitter_u8, one step): the memory-bound yardstick,
which moves the same bytes as every case here.  Per case: the median over --reps samples, after warm-up, of the launch alone
(device events around --inner calls of dbn_degrade_u8 with records and tiles already uploaded, divided by --inner), the bytes that
must move (every image read once and written once) per second and against the 8 TB/s HBM figure, the time over the blend's, and
one degrade_images call end to end on the host clock (records and tiles built and uploaded, synchronised).  Needs a GPU; there is no
fallback.

  python tools/degrade_probe.py [--reps 10] [--inner 10] [--out FILE (appended)]
Run it as one step under a time limit:
  timeout -k 10 300 python tools/degrade_probe.py --out profiles/degrade_probe.txt
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, H, W = 32, 1280, 1280
HBM_PEAK = 8e12
CASES = [('blur sigma 1', 1.0, 0.0), ('blur sigma 3', 3.0, 0.0), ('blur sigma 8', 8.0, 0.0), ('noise 10', 0.0, 10.0), ('blur sigma 1 + noise 10', 1.0, 10.0)]


def images():
    rng = np.random.default_rng(5)
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([(x * 0.2 + y * 0.1) % 256, (x * 0.05 + 64) % 200, (y * 0.3) % 256], -1)
    return [np.clip(np.roll(base, 37 * i, 1) + rng.integers(-6, 7, size=base.shape), 0, 255).astype(np.uint8) for i in range(N)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    from db_text_minimal_amd import degrade as D
    from db_text_minimal_amd import packed as Pk
    from db_text_minimal_amd import photometric as P
    from db_text_minimal_amd._lib import check, lib
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
            for _ in range(args.inner):
                fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) / args.inner)
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

    L, stream = lib(), torch.cuda.current_stream().cuda_stream
    shapes = [(H, W)] * N
    packed = torch.from_numpy(np.concatenate([a.reshape(-1) for a in images()])).to(dev)
    out = torch.empty_like(packed)
    nbytes = packed.numel()
    moved = 2 * nbytes
    table = torch.from_numpy(D.NORMAL_TABLE.copy()).to(dev)
    say('== degrade_probe: %d x %d x %d RGB, %.1f MB, median of %d x %d launches, %s' % (N, W, H, nbytes / 1e6, args.reps, args.inner,
                                                                                        torch.cuda.get_device_name(0)))
    say('%-26s %9s %9s %8s %7s %9s %9s' % ('case', 'device ms', 'moved MB', 'GB/s', 'of HBM', 'x blend', 'call ms'))

    bdesc = P.plan_records(shapes, [[('brightness', 1.1)]] * N)
    bdev = Pk.upload(bdesc, dev)
    blend = device_ms(lambda: check(L.dbn_color_jitter_u8(packed.data_ptr(), out.data_ptr(), nbytes, bdesc.ctypes.data, bdev.data_ptr(), N, None, stream),
                                    'color_jitter_u8'))

    def row(name, ms, call_ms):
        say('%-26s %9.3f %9.1f %8.1f %6.1f%% %9.2f %9s' % (name, ms, moved / 1e6, moved / ms / 1e6, 100 * moved / (ms * 1e-3) / HBM_PEAK, ms / blend,
                                                          '' if call_ms is None else '%.3f' % call_ms))

    row('adjust_brightness (blend)', blend, None)
    for name, sigma, scale in CASES:
        plans = [{'sigma': sigma, 'scale': scale, 'per_channel': True, 'seed': 1000 + i} for i in range(N)]
        hdesc, htiles = D.degrade_records(shapes, plans)
        desc, tiles = Pk.upload(hdesc, dev), Pk.upload(htiles, dev)

        def launch():
            check(L.dbn_degrade_u8(packed.data_ptr(), out.data_ptr(), nbytes, hdesc.ctypes.data, desc.data_ptr(), N, htiles.ctypes.data,
                                   tiles.data_ptr(), len(htiles), table.data_ptr(), stream), 'degrade_u8')

        row(name, device_ms(launch), host_ms(lambda: D.degrade_images(packed, shapes, plans, out=out)))
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()
