#!/usr/bin/env python3
"""Times the PNG paths (db_text_minimal_amd.png, csrc/png.hip) on two sets of synthetic RGB "photo" images (a ramp plus +-6
noise), Pillow-encoded when Pillow is installed, otherwise written by the project's own encoder:
  hd       16 images of 1280 x 720
  square   32 images of 1280 x 1280
and prints, per workload: host inflate (inflate_png) on 1 and 16 threads, the unfilter launch and the pixel launch (device
events, each against the bytes it moves), decode_png_batch end to end, the encoder's filter launch, encode_png_batch end to
end, the file bytes against Pillow's at the same compress_level, and Pillow decoding the same files in 16 worker processes
(when it is installed).  Needs a GPU; there is no fallback.

  python tools/png_probe.py --workload hd|square [--reps 5] [--no-pillow] [--out FILE (appended)]
Run each workload as a step of its own under a time limit:
  timeout -k 10 300 python tools/png_probe.py --workload hd --out profiles/png_probe.txt && \\
  timeout -k 10 300 python tools/png_probe.py --workload square --out profiles/png_probe.txt
"""
import argparse
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOADS = {'hd': (16, 720, 1280), 'square': (32, 1280, 1280)}


def images(kind):
    n, h, w = WORKLOADS[kind]
    rng = np.random.default_rng(5)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 0.2 + y * 0.1) % 256, (x * 0.05 + 64) % 200, (y * 0.3) % 256], -1)
    return [np.clip(np.roll(base, 37 * i, 1) + rng.integers(-6, 7, size=base.shape), 0, 255).astype(np.uint8) for i in range(n)]


def have_pillow():
    try:
        import PIL.Image  # noqa: F401
        return True
    except ImportError:
        return False


def pillow_encode(arrs, level=6):
    from PIL import Image
    out = []
    for a in arrs:
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, 'PNG', compress_level=level)
        out.append(buf.getvalue())
    return out


def _pil_decode_chunk(datas):
    from PIL import Image
    return sum(int(np.asarray(Image.open(io.BytesIO(d)).convert('RGB'))[0, 0, 0]) for d in datas)


def pillow_decode_ms(datas, workers=16, reps=3):
    import multiprocessing as mp
    chunks = [datas[i::workers] for i in range(workers)]
    with mp.get_context('spawn').Pool(workers) as pool:
        pool.map(_pil_decode_chunk, chunks)  # start-up and imports
        best = 1e9
        for _ in range(reps):
            t = time.perf_counter()
            pool.map(_pil_decode_chunk, chunks)
            best = min(best, time.perf_counter() - t)
    return best * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', choices=sorted(WORKLOADS), required=True)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-pillow', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    from db_text_minimal_amd import packed as Pk
    from db_text_minimal_amd import png as P
    from db_text_minimal_amd._lib import lib
    dev = torch.device('cuda')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def host_ms(fn):
        fn()
        ts = []
        for _ in range(args.reps):
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t)
        return float(np.median(ts)) * 1e3

    def device_ms(fn):
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

    arrs = images(args.workload)
    n, h, w = WORKLOADS[args.workload]
    pil = have_pillow() and not args.no_pillow
    own = P.encode_png_batch(arrs, device=dev)
    datas = pillow_encode(arrs) if pil else own
    say('== png_probe %s: %d x %d x %d RGB, files written by %s, %.2f MB (%.2f B/pixel), %s' % (
        args.workload, n, w, h, 'Pillow' if pil else 'encode_png_batch', sum(map(len, datas)) / 1e6, sum(map(len, datas)) / (n * h * w),
        torch.cuda.get_device_name(0)))
    obj = P.inflate_png(datas)
    types = np.bincount(np.concatenate([obj.blob.numpy()[int(d[8]):int(d[8]) + h * (3 * w + 1):3 * w + 1] for d in obj.desc]), minlength=5)
    say('filter types of the files (rows of type 0 .. 4): %s' % types.tolist())
    for t in (1, 16):
        say('host inflate_png, %2d threads: %8.2f ms' % (t, host_ms(lambda: P.inflate_png(datas, threads=t))))
    # the two launches, on tensors already on the device
    hdesc, hsubs = np.ascontiguousarray(obj.desc), np.ascontiguousarray(obj.subs)
    out_bytes = n * h * w * 3
    blob, desc, subs, pal = obj.blob.to(dev), Pk.upload(hdesc, dev), Pk.upload(hsubs, dev), Pk.upload(obj.palettes, dev)
    raw = torch.empty(obj.raw_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
    L, stream = lib(), torch.cuda.current_stream().cuda_stream

    def unfilter():
        P.check(L.dbn_png_unfilter(blob.data_ptr(), obj.blob_len, blob.numel(), hdesc.ctypes.data, desc.data_ptr(), n, hsubs.ctypes.data,
                                   subs.data_ptr(), len(hsubs), raw.data_ptr(), obj.raw_bytes, out_bytes, stream), 'png_unfilter')

    def pixels():
        P.check(L.dbn_png_pixels(raw.data_ptr(), obj.raw_bytes, hdesc.ctypes.data, desc.data_ptr(), pal.data_ptr(), n, obj.blob_len, out.data_ptr(),
                                 out_bytes, stream), 'png_pixels')

    ms = device_ms(unfilter)
    say('unfilter launch (%d workgroups, one per image):   %8.3f ms  (%.1f GB/s of %.1f MB read + written)' % (
        len(hsubs), ms, (obj.blob_len + obj.raw_bytes) / ms / 1e6, (obj.blob_len + obj.raw_bytes) / 1e6))
    ms = device_ms(pixels)
    say('pixel launch:                                      %8.3f ms  (%.1f GB/s of %.1f MB read + written)' % (
        ms, (obj.raw_bytes + out_bytes) / ms / 1e6, (obj.raw_bytes + out_bytes) / 1e6))
    say('upload + both launches (unfilter_png):             %8.2f ms' % host_ms(lambda: P.unfilter_png(obj, dev)))
    ms = host_ms(lambda: P.decode_png_batch(datas, dev))
    say('decode_png_batch end to end, 16 threads:           %8.2f ms  (%.0f images/s)' % (ms, n / ms * 1e3))
    if pil:
        ms = pillow_decode_ms(datas)
        say('Pillow decode, 16 worker processes (no upload):    %8.2f ms  (%.0f images/s)' % (ms, n / ms * 1e3))
    # encode
    packed = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrs])).to(dev)
    shapes = [(h, w)] * n
    ms = device_ms(lambda: P._filter_launch(packed, shapes, 'adaptive', dev))
    say('encoder filter launch (adaptive, with its tables): %8.3f ms  (%.1f GB/s of %.1f MB read + written)' % (
        ms, 2 * out_bytes / ms / 1e6, 2 * out_bytes / 1e6))
    for level in (1, 6):
        ms = host_ms(lambda: P.encode_png_batch(packed, shapes, compress_level=level))
        size = sum(map(len, P.encode_png_batch(packed, shapes, compress_level=level)))
        line = 'encode_png_batch level %d, 16 threads:              %8.2f ms  (%.0f images/s), %.2f MB' % (level, ms, n / ms * 1e3, size / 1e6)
        if pil:
            line += '; Pillow compress_level=%d: %.2f MB' % (level, sum(map(len, pillow_encode(arrs, level))) / 1e6)
        say(line)
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()
