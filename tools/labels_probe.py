#!/usr/bin/env python3
"""Cost of writing labels on the device (draw_labels of db_text_minimal_amd.render, dbn_draw_glyphs) for a dense inference
batch: 32 images of 1280 x 1280 with 300 six-character labels each, at cap height 16 and at cap height 64.

Prints, per height:
  kernel   dbn_draw_glyphs alone, in place (records and font already on the device; no copy of the images), median of
           timed calls after warm-up (device events), with the glyph instances and the pixels of their boxes
  e2e      draw_labels from device images: records built on the host, their copy, the copy of the images and the launch,
           wall clock to a synchronised device, median
  PIL      ImageDraw.text of the same strings with DejaVu Sans at the matching size in 16 worker processes (forked before
           the GPU is initialised, CPU only), wall clock for the 32 images; PIL anti-aliases, so this is a yardstick for
           the cost, not for the bytes; the font file is matplotlib's (PIL or matplotlib missing: "not measured")
  numpy    device == tests/labels_ref.py on the last image
Usage: python tools/labels_probe.py [--reps 30] [--out file]
"""
import argparse
import multiprocessing
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

N, H, W, PER_IMAGE, CHARS, WORKERS = 32, 1280, 1280, 300, 6, 16
ALPHABET = 'ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789.%'


def make_labels(rng, height):
    out = []
    for _ in range(N):
        xs, ys = rng.integers(0, W - 5 * height, PER_IMAGE), rng.integers(2 * height, H - height, PER_IMAGE)
        out.append([(''.join(ALPHABET[i] for i in rng.integers(0, len(ALPHABET), CHARS)), (int(x), int(y))) for x, y in zip(xs, ys)])
    return out


def _pil_image(job):
    labels, px, path = job
    from PIL import Image, ImageDraw, ImageFont
    font = ImageFont.truetype(path, px)
    img = Image.new('RGB', (W, H))
    draw = ImageDraw.Draw(img)
    for text, (x, y) in labels:
        draw.text((x, y), text, fill=(255, 0, 0), font=font, anchor='ls')
    return img.size[0]


def pil_time(pool, labels, height):
    """wall clock of the 32 images through the pool, median of 3; None when PIL or the font file is missing"""
    try:
        import matplotlib
        import PIL  # noqa: F401
    except ImportError:
        return None
    path = os.path.join(matplotlib.get_data_path(), 'fonts', 'ttf', 'DejaVuSans.ttf')
    px = max(1, int(round(height * 2048 / 1493)))  # the em size in pixels
    jobs = [(l, px, path) for l in labels]
    pool.map(_pil_image, jobs)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        pool.map(_pil_image, jobs)
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(0)
    work = {h: make_labels(rng, h) for h in (16, 64)}
    pool = multiprocessing.get_context('fork').Pool(WORKERS)  # before the GPU is initialised; CPU only
    pil = {h: pil_time(pool, work[h], h) for h in work}
    pool.close()
    pool.join()

    import torch
    from db_text_minimal_amd import draw_labels, image_views
    from db_text_minimal_amd import packed as Pk
    from db_text_minimal_amd import render as Rn
    from db_text_minimal_amd._lib import check, lib
    import labels_ref as LR
    assert torch.cuda.is_available(), 'the probe times the device: it needs a GPU'
    dev = torch.device('cuda')
    shapes = [(H, W)] * N
    src = torch.from_numpy(rng.integers(0, 256, N * H * W * 3, dtype=np.uint8)).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    say('labels_probe: %d x %dx%d uint8, %d labels of %d characters per image (DejaVu Sans outlines, on / off)' % (N, H, W, PER_IMAGE, CHARS))
    for height, labels in work.items():
        s = Rn._size64(height)
        recs = Rn.label_records(labels, N)
        f = Rn.glyph_table()
        ext = (f['index'][recs[:, 1], 4:6].astype(np.int64) - f['index'][recs[:, 1], 2:4]) * s / (64 * 2048)
        fe, fg = Rn._font_on(dev)
        r, d, out = torch.from_numpy(recs).to(dev), Pk.image_table(shapes, dev), src.clone()
        rows = Rn._rows_bound(f['index'], s)

        def kernel():
            check(lib().dbn_draw_glyphs(out.data_ptr(), out.data_ptr(), out.numel(), d.data_ptr(), N, fe.data_ptr(), fe.shape[0], fg.data_ptr(),
                                        fg.shape[0], r.data_ptr(), len(recs), s, rows, 255, 0, 0, st), 'draw_glyphs')

        for _ in range(5):
            kernel()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            kernel()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        say('height %d: kernel dbn_draw_glyphs, in place, %d glyph instances, %.1f M box pixels (measured) %.3f ms'
            % (height, len(recs), float((ext[:, 0] * ext[:, 1]).sum()) / 1e6, statistics.median(ts)))
        for _ in range(3):
            draw_labels((src, shapes), labels, height=height)
        torch.cuda.synchronize()
        ts = []
        for _ in range(max(5, args.reps // 3)):
            t0 = time.perf_counter()
            draw_labels((src, shapes), labels, height=height)
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        say('height %d: e2e draw_labels from device images, copy included (measured, wall clock to a synchronised device) %.3f ms'
            % (height, statistics.median(ts)))
        say('height %d: PIL ImageDraw.text, %d worker processes, the %d images (measured, wall clock) %s'
            % (height, WORKERS, N, 'not measured' if pil[height] is None else '%.1f ms' % pil[height]))
        got = image_views(draw_labels((src, shapes), labels, height=height), shapes)[N - 1].cpu().numpy()
        img = image_views(src, shapes)[N - 1].cpu().numpy()
        assert np.array_equal(got, LR.draw_labels(img, labels[N - 1], height=height)), 'the device picture differs from the numpy restatement'
        say('height %d: device == numpy restatement on the last image' % height)
    if args.out:
        with open(args.out, 'w') as fo:
            fo.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
