#!/usr/bin/env python3
"""Cost of decoding JPEG batches for the device pipeline (db_text_minimal_amd.jpeg) against PIL in 16 worker processes, for
two workloads encoded once from synthetic text-like images, 4:2:0 at quality 90: 16 images of 1280 x 720 and 32 of 1280 x 1280.

Prints, per workload (medians of timed repetitions after warm-up):
  pil16    PIL (libjpeg-turbo) decoding the same files to RGB arrays in a pool of 16 worker processes, results returned to
           the parent as the packed uint8 batch a loader would ship: wall clock; the baseline the hybrid replaces
  pil1     the same decode in this process, one core: ms per image
  host     dbn_jpeg_entropy_batch (Huffman stage, C++ threads) into a pinned buffer at 1 and at 16 threads: wall clock
  h2d      the coefficients' copy to the device (device events), and its GB/s
  kernels  dbn_jpeg_pixels (both launches; tables and descriptors already on the device), device events, against its
           algorithmic bytes — coefficients in (2 B each), RGB out (3 B per pixel) — in GB/s and as a share of 8 TB/s
  e2e      decode_jpeg_batch from byte strings to a synchronised device, wall clock, images/s; and pil16 + the H2D copy of
           its 3 B/pixel for the same end point
--workloads scans: the 16 x 1280 x 720 set twice more.  Saved progressive (Pillow's scan script): the host entropy stage with
multiscan=True at 1 and 16 threads against the baseline-coded set in the same run and against PIL in 16 worker processes.
With Exif tag 6: jpeg_rgb_oriented_kernel (the 32 x 32 tile kernel) against jpeg_rgb_kernel on the same images, each launched
behind a one-workgroup IDCT table so that the device events time that kernel, with the bytes both move per second (1.5 B per
pixel of planes in, 3 B out).
One process touches the GPU; the PIL pool is forked before the GPU is initialised and never touches it; every step runs
under its own alarm.  The alarm ends a step that is slow on the host; it cannot interrupt a device synchronise that never
returns, so run the probe under an outer time limit as well.
Usage: timeout -k 10 600 python tools/jpeg_probe.py [--reps 20] [--out file] [--workloads baseline|scans]
"""
import argparse
import io
import multiprocessing
import os
import signal
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKERS = 16
BW = 8e12  # bytes / s


def text_image(rng, H, W):
    """a page-like picture: a soft paper gradient, dark text-like strokes in lines, mild sensor noise"""
    y, x = np.mgrid[0:H, 0:W]
    img = (225 + 20 * np.sin(x / 301.0) * np.cos(y / 173.0))[:, :, None] + np.array([0, -6, -14])[None, None, :]
    for row in range(40, H - 40, 38):
        xs = 30
        while xs < W - 60:
            wl = int(rng.integers(20, 140))
            for cx in range(xs, min(xs + wl, W - 30), 9):
                h0 = int(rng.integers(6, 22))
                img[row + 22 - h0:row + 22, cx:cx + int(rng.integers(2, 6))] = rng.integers(10, 60)
                if rng.random() < 0.5:
                    img[row + 22 - h0 // 2:row + 24 - h0 // 2, cx:cx + 8] = rng.integers(10, 60)
            xs += wl + int(rng.integers(12, 30))
    img = img + rng.normal(0, 2.0, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def encode(img, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, 'JPEG', quality=90, subsampling=2, **kw)
    return buf.getvalue()


def with_orientation(data, tag):
    """the stream with an Exif APP1 segment that holds the orientation tag alone"""
    tiff = b'II' + (42).to_bytes(2, 'little') + (8).to_bytes(4, 'little') + (1).to_bytes(2, 'little') + (0x0112).to_bytes(2, 'little') + \
        (3).to_bytes(2, 'little') + (1).to_bytes(4, 'little') + tag.to_bytes(2, 'little') + b'\0\0' + (0).to_bytes(4, 'little')
    body = b'Exif\0\0' + tiff
    return data[:2] + b'\xff\xe1' + (len(body) + 2).to_bytes(2, 'big') + body + data[2:]


def pil_decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))


class StepTimeout(Exception):
    pass


def step(seconds, fn):
    def on_alarm(signum, frame):
        raise StepTimeout('step exceeded %d s' % seconds)
    signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(seconds)
    try:
        return fn()
    finally:
        signal.alarm(0)


def wall(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts)


def events(fn, reps):
    import torch
    for _ in range(3):
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


def scans_workloads(args, say):
    """the progressive set and the tag-6 set (see the module docstring)"""
    rng = np.random.default_rng(0)
    N, H, W = 16, 720, 1280
    imgs = step(300, lambda: [text_image(rng, H, W) for _ in range(N)])
    base = step(300, lambda: [encode(im) for im in imgs])
    prog = step(300, lambda: [encode(im, progressive=True) for im in imgs])
    pool = multiprocessing.get_context('fork').Pool(WORKERS)  # before the GPU is initialised; CPU only
    try:
        def run():
            return np.concatenate([a.reshape(-1) for a in pool.map(pil_decode, prog, chunksize=1)])
        t_pil = step(300, lambda: wall(run, max(5, args.reps // 2)))
    finally:
        pool.close()
        pool.join()
    import torch
    from db_text_minimal_amd import decode_jpeg_batch, entropy_decode, jpeg_info
    from db_text_minimal_amd import jpeg as J
    from db_text_minimal_amd._lib import check, lib
    assert torch.cuda.is_available(), 'the probe times the device: it needs a GPU'
    dev = torch.device('cuda', 0)
    reps = max(5, args.reps // 2)
    say('jpeg_probe scans: %d x %dx%d, 4:2:0 quality 90; progressive %.2f MB in %d scans each, baseline-coded %.2f MB'
        % (N, W, H, sum(map(len, prog)) / 1e6, jpeg_info(prog[0], multiscan=True)['scans'], sum(map(len, base)) / 1e6))
    tp = {t: step(300, lambda: wall(lambda: entropy_decode(prog, threads=t, pin=True, multiscan=True), reps)) for t in (1, 16)}
    tb = {t: step(300, lambda: wall(lambda: entropy_decode(base, threads=t, pin=True, multiscan=True), reps)) for t in (1, 16)}
    say('host    progressive set, multiscan=True, into pinned memory (measured, wall): 1 thread %.1f ms (%.2f ms per image), 16 threads %.1f ms  %.0f images/s'
        % (tp[1], tp[1] / N, tp[16], 1e3 * N / tp[16]))
    say('        the baseline-coded set in the same run: 1 thread %.1f ms (%.2f ms per image), 16 threads %.1f ms  %.0f images/s; progressive / baseline %.2fx at 1 thread, %.2fx at 16'
        % (tb[1], tb[1] / N, tb[16], 1e3 * N / tb[16], tp[1] / tb[1], tp[16] / tb[16]))
    say('pil16   PIL on the progressive set in %d worker processes -> packed uint8 in the parent (measured, wall): %.1f ms  %.0f images/s' % (WORKERS, t_pil, 1e3 * N / t_pil))
    a, b = entropy_decode(prog, pin=False, multiscan=True), entropy_decode(base, pin=False)
    assert not a.status.any() and torch.equal(a.coef, b.coef), 'progressive and baseline coefficients differ'
    say('        progressive and baseline coefficient buffers are equal bit for bit')

    turned = [with_orientation(d, 6) for d in base]
    obj = entropy_decode(turned, pin=True)
    assert not obj.status.any() and obj.orientation.tolist() == [6] * N
    ta, tr = J.work_tables(obj.desc, obj.status)
    tt = J.tile_table(obj.desc, obj.status, obj.orientation)
    coef = obj.coef.to(dev)
    d, q, ia, ir, it, o = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (obj.desc, obj.qtabs.view(np.int16), ta, tr, tt, obj.orientation))
    planes = torch.empty(coef.numel(), dtype=torch.uint8, device=dev)
    out = torch.empty(N * H * W * 3, dtype=torch.uint8, device=dev)
    L, st = lib(), torch.cuda.current_stream().cuda_stream

    def call(n_idct, n_rgb, n_tile):
        check(L.dbn_jpeg_pixels_ex(coef.data_ptr(), coef.numel(), d.data_ptr(), q.data_ptr(), N, ia.data_ptr(), n_idct, ir.data_ptr(), n_rgb, o.data_ptr(),
                                   it.data_ptr(), n_tile, planes.data_ptr(), out.data_ptr(), out.numel(), st), 'jpeg_pixels_ex')

    call(len(ta), len(tr), 0)  # the planes, for both kernels
    t_rgb = step(120, lambda: events(lambda: call(1, len(tr), 0), args.reps))
    t_tile = step(120, lambda: events(lambda: call(1, 0, len(tt)), args.reps))
    t_one = step(120, lambda: events(lambda: call(1, 1, 0), args.reps))
    byt = N * H * W * 4.5
    say('kernels tag 6, behind a one-workgroup IDCT launch (measured, device events; the two launches with one workgroup each take %.3f ms):' % t_one)
    say('        jpeg_rgb_kernel          %d workgroups: %.3f ms  %.0f GB/s of planes in (1.5 B / pixel) and RGB out (3 B / pixel)' % (len(tr), t_rgb, byt / t_rgb / 1e6))
    say('        jpeg_rgb_oriented_kernel %d workgroups: %.3f ms  %.0f GB/s of the same bytes; oriented / plain %.2fx' % (len(tt), t_tile, byt / t_tile / 1e6, t_tile / t_rgb))
    packed, shapes = decode_jpeg_batch(turned, dev, orient=True)
    got = packed.view(N, W, H, 3)[N - 1].cpu().numpy()
    assert shapes == [(W, H)] * N and np.array_equal(got, np.rot90(pil_decode(base[N - 1]), -1)), 'oriented device pixels differ from PIL turned'
    say('        decode_jpeg_batch(orient=True) == PIL rotated, on the last image')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--workloads', choices=('baseline', 'scans'), default='baseline')
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if args.workloads == 'scans':
        scans_workloads(args, say)
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
        return
    rng = np.random.default_rng(0)
    loads = []
    for N, H, W in ((16, 720, 1280), (32, 1280, 1280)):
        datas = step(300, lambda: [encode(text_image(rng, H, W)) for _ in range(N)])
        loads.append((N, H, W, datas))
    pool = multiprocessing.get_context('fork').Pool(WORKERS)  # before the GPU is initialised; CPU only
    try:
        pil = {}
        for N, H, W, datas in loads:
            def run():
                return np.concatenate([a.reshape(-1) for a in pool.map(pil_decode, datas, chunksize=1)])
            pil[(N, H)] = step(300, lambda: wall(run, max(5, args.reps // 2)))
    finally:
        pool.close()
        pool.join()

    import torch
    from db_text_minimal_amd import decode_jpeg_batch, entropy_decode
    from db_text_minimal_amd import jpeg as J
    from db_text_minimal_amd._lib import check, lib
    assert torch.cuda.is_available(), 'the probe times the device: it needs a GPU'
    dev = torch.device('cuda', 0)

    for N, H, W, datas in loads:
        jb = sum(len(d) for d in datas)
        say('jpeg_probe: %d x %dx%d, 4:2:0 quality 90, %.2f MB of JPEG (%.2f bits per pixel)' % (N, W, H, jb / 1e6, 8 * jb / (N * H * W)))
        t_pil = pil[(N, H)]
        say('pil16   PIL in %d worker processes -> packed uint8 in the parent (measured, wall): %.1f ms  %.0f images/s' % (WORKERS, t_pil, 1e3 * N / t_pil))
        t1 = step(300, lambda: wall(lambda: pil_decode(datas[0]), 5, 1))
        say('pil1    PIL, this process, one core (measured): %.2f ms per image' % t1)
        th = {t: step(300, lambda: wall(lambda: entropy_decode(datas, threads=t, pin=True), max(5, args.reps // 2))) for t in (1, 16)}
        say('host    dbn_jpeg_entropy_batch into pinned memory (measured, wall): 1 thread %.1f ms (%.2f ms per image), 16 threads %.1f ms  %.0f images/s'
            % (th[1], th[1] / N, th[16], 1e3 * N / th[16]))
        obj = entropy_decode(datas, pin=True)
        assert not obj.status.any()
        cb = obj.coef.numel() * 2
        dst = torch.empty_like(obj.coef, device=dev)
        t_h2d = step(120, lambda: events(lambda: dst.copy_(obj.coef, non_blocking=True), args.reps))
        say('h2d     %.1f MB of coefficients (%.2f B per pixel) (measured, device events): %.3f ms  %.1f GB/s' % (cb / 1e6, cb / (N * H * W), t_h2d, cb / t_h2d / 1e6))
        ta, tb = J.work_tables(obj.desc, obj.status)
        d, q, a, b = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (obj.desc, obj.qtabs.view(np.int16), ta, tb))
        planes = torch.empty(dst.numel(), dtype=torch.uint8, device=dev)
        out = torch.empty(N * H * W * 3, dtype=torch.uint8, device=dev)
        L, st = lib(), torch.cuda.current_stream().cuda_stream

        def kernels():
            check(L.dbn_jpeg_pixels(dst.data_ptr(), dst.numel(), d.data_ptr(), q.data_ptr(), N, a.data_ptr(), len(ta), b.data_ptr(), len(tb),
                                    planes.data_ptr(), out.data_ptr(), out.numel(), st), 'jpeg_pixels')

        t_k = step(120, lambda: events(kernels, args.reps))
        alg = cb + out.numel()
        say('kernels dbn_jpeg_pixels, %d + %d workgroups (measured, device events): %.3f ms; algorithmic bytes %.1f MB in + %.1f MB out: %.0f GB/s, '
            '%.0f%% of the 8 TB/s floor rate (floor %.3f ms)' % (len(ta), len(tb), t_k, cb / 1e6, out.numel() / 1e6, alg / t_k / 1e6,
                                                                 100 * (alg / BW * 1e3) / t_k, alg / BW * 1e3))
        want = pil_decode(datas[N - 1])
        got = out.view(N, H, W, 3)[N - 1].cpu().numpy()
        assert np.array_equal(got, want), 'device pixels differ from PIL'

        def e2e():
            decode_jpeg_batch(datas, dev)
            torch.cuda.synchronize()

        t_e = step(300, lambda: wall(e2e, max(5, args.reps // 2)))
        rgb_host = torch.empty(N * H * W * 3, dtype=torch.uint8).pin_memory()
        t_rgb = step(120, lambda: events(lambda: out.copy_(rgb_host, non_blocking=True), args.reps))
        say('e2e     decode_jpeg_batch, bytes -> synchronised device (measured, wall): %.1f ms  %.0f images/s; device == PIL on the last image' % (t_e, 1e3 * N / t_e))
        say('        baseline to the same end point: pil16 %.1f ms + H2D of %.1f MB RGB %.3f ms (measured) = %.1f ms  %.0f images/s'
            % (t_pil, out.numel() / 1e6, t_rgb, t_pil + t_rgb, 1e3 * N / (t_pil + t_rgb)))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
