#!/usr/bin/env python3
"""Cost of generating synthetic scene text on the device (db_text_minimal_amd.synth, csrc/synth.hip), and a short pre-training run on it.

  --part time      for 16 images of 640 x 640 and 32 of 1280 x 1280 at the default plan, medians after warm-up:
      plan      plan_synth_text on the host (the float64 planner), host clock
      records   synth_records (records, bins, descriptors), host clock
      launch    dbn_synth_text_u8 alone, device events around --inner launches with every table already uploaded
      render    render_synth_text end to end: records built, uploaded, launched, synchronised; host clock
      PIL       the same plans drawn by PIL's ImageDraw.text with the same font in 16 worker processes (every word on a layer of its own,
                rotated and pasted, as host renderers of synthetic text do): a cost yardstick, not a byte comparison.  The workers are
                started and ended before the GPU is touched.
    and the bf16 training step of 16 x 640 x 640 in the same run (the consumer generation has to keep ahead of).
  --part pretrain  random initialisation, FusedAdam(lr 0.005), bf16, 16 x 640 x 640 from SynthTextBatches through DeviceBatches(training=True) for
      --seconds (default 150); the loss every --every steps, then evaluate(..., detection=True) on 64 held-out images of another seed.

  python tools/synth_probe.py --part time [--out FILE (appended)]
Run each part as one step under a time limit:
  timeout -k 10 300 python tools/synth_probe.py --part time --out profiles/synth_probe.txt
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIGS = [(16, 640), (32, 1280)]
_font_cache = {}


def pil_image(job):
    """one image of its plan by PIL: the flat base colour, every word drawn on a layer, rotated and pasted"""
    import matplotlib
    from PIL import Image, ImageDraw, ImageFont
    (H, W), plan = job
    path = os.path.join(matplotlib.get_data_path(), 'fonts', 'ttf', 'DejaVuSans.ttf')
    img = Image.new('RGB', (W, H), tuple(plan['base']))
    for w in plan['words']:
        size = max(4, int(round(w['height'] / 0.729)))  # cap height / em of DejaVu Sans
        if size not in _font_cache:
            _font_cache[size] = ImageFont.truetype(path, size)
        font = _font_cache[size]
        box = font.getbbox(w['text'])
        layer = Image.new('L', (box[2] + 4, box[3] + 4), 0)
        ImageDraw.Draw(layer).text((2, 2), w['text'], fill=255, font=font)
        p = np.asarray(w['polygon'])
        angle = -np.degrees(np.arctan2(p[1, 1] - p[0, 1], p[1, 0] - p[0, 0])) if len(p) == 4 else 0.0
        layer = layer.rotate(angle, resample=Image.BICUBIC, expand=True)
        img.paste(tuple(w['colour']), (int(p[:, 0].min()), int(p[:, 1].min())), layer)
    return np.asarray(img).shape


def plans_of(S, n, size, seed):
    src = S.SynthTextBatches(1, n, (size, size), seed=seed)
    return src.plan(0)


def part_time(args, say):
    from db_text_minimal_amd import synth as S
    median = lambda ts: float(np.median(ts)) * 1e3
    pil = {}
    try:
        import multiprocessing as mp
        import matplotlib  # noqa: F401
        import PIL  # noqa: F401
        with mp.get_context('fork').Pool(16) as pool:  # before the GPU is initialised: the workers never see it
            for n, size in CONFIGS:
                shapes, plans = plans_of(S, n, size, 0)
                jobs = list(zip(shapes, plans))
                pool.map(pil_image, jobs)
                ts = []
                for _ in range(5):
                    t = time.perf_counter()
                    pool.map(pil_image, jobs, chunksize=max(1, n // 16))
                    ts.append(time.perf_counter() - t)
                pil[(n, size)] = median(ts)
    except ImportError as e:
        say('(no PIL yardstick: %s)' % e)

    import torch
    from db_text_minimal_amd import DBLoss, DBTextModel, DBTrainer, FusedAdam
    from db_text_minimal_amd import packed as Pk
    from db_text_minimal_amd._lib import check, lib
    from db_text_minimal_amd.render import glyph_table
    dev = torch.device('cuda')
    L, stream = lib(), torch.cuda.current_stream().cuda_stream
    f = glyph_table()
    say('== synth_probe --part time: default plan, median of %d, %s' % (args.reps, torch.cuda.get_device_name(0)))
    say('%-16s %6s %7s %9s %10s %10s %10s %12s %10s' % ('batch', 'words', 'glyphs', 'plan ms', 'records ms', 'launch ms', 'render ms', 'plan+render', 'PIL x16 ms'))
    for n, size in CONFIGS:
        ts = []
        for rep in range(args.reps):
            t = time.perf_counter()
            shapes, plans = plans_of(S, n, size, rep)
            ts.append(time.perf_counter() - t)
        plan_ms = median(ts)
        shapes, plans = plans_of(S, n, size, 0)
        ts = []
        for _ in range(args.reps):
            t = time.perf_counter()
            recs, bins, desc = S.synth_records(shapes, plans)
            ts.append(time.perf_counter() - t)
        rec_ms = median(ts)
        need = sum(3 * h * w for h, w in shapes)
        out = torch.empty(need, dtype=torch.uint8, device=dev)
        d, r, b = Pk.upload(desc, dev), Pk.upload(recs, dev), Pk.upload(bins, dev)
        fe, fg = Pk.upload(f['edges_all'], dev), Pk.upload(f['index_all'], dev)
        T = S.tile_count(shapes)

        def launch():
            check(L.dbn_synth_text_u8(None, out.data_ptr(), need, desc.ctypes.data, d.data_ptr(), n, recs.ctypes.data, r.data_ptr(), len(recs), bins.ctypes.data,
                                      b.data_ptr(), T, len(bins), fe.data_ptr(), len(f['edges_all']), f['index_all'].ctypes.data, fg.data_ptr(), len(f['index_all']),
                                      stream), 'synth_text_u8')

        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.inner):
                launch()
            e.record()
            e.synchronize()
            ts.append(a.elapsed_time(e) / args.inner * 1e-3)
        launch_ms = median(ts)
        S.render_synth_text(shapes, plans, dev, out=out)
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            S.render_synth_text(shapes, plans, dev, out=out)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t)
        render_ms = median(ts)
        say('%-16s %6d %7d %9.2f %10.2f %10.3f %10.2f %12.2f %10s' % ('%d x %d x %d' % (n, size, size), sum(len(p['words']) for p in plans), len(recs), plan_ms, rec_ms,
                                                                   launch_ms, render_ms, plan_ms + render_ms, '%.1f' % pil[(n, size)] if (n, size) in pil else '-'))
    torch.manual_seed(42)
    model = DBTextModel().to(dev).train()
    model.engine.set_conv_math('bf16')
    trainer = DBTrainer(model, DBLoss(), FusedAdam(model, lr=0.005), distributed=False)
    img, gts = torch.randn(16, 3, 640, 640, device=dev), (torch.rand(4, 16, 640, 640, device=dev) > 0.7).float()
    for _ in range(5):
        trainer.step(img, gts)
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        t = time.perf_counter()
        for _ in range(5):
            trainer.step(img, gts)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) / 5)
    say('bf16 training step, 16 x 640 x 640 (random tensors, same run): %.2f ms' % median(ts))


def part_pretrain(args, say):
    import torch
    from db_text_minimal_amd import DBLoss, DBTextModel, DBTrainer, FusedAdam
    from db_text_minimal_amd import synth as S
    from db_text_minimal_amd.augment import DeviceBatches
    from db_text_minimal_amd.train import evaluate
    dev = torch.device('cuda')
    torch.manual_seed(0)
    model = DBTextModel().to(dev).train()
    model.engine.set_conv_math('bf16')
    trainer = DBTrainer(model, DBLoss(), FusedAdam(model, lr=0.005), distributed=False)
    say('== synth_probe --part pretrain: random initialisation, FusedAdam lr 0.005, bf16, 16 x 640 x 640, %g s, %s' % (args.seconds, torch.cuda.get_device_name(0)))
    train = DeviceBatches(S.SynthTextBatches(1 << 20, 16, (640, 640), seed=0, device=dev), dev, training=True, seed=0)
    start, steps, window = time.perf_counter(), 0, []
    for batch in train:
        preds, losses = trainer.step(batch, None)
        window.append(losses)
        steps += 1
        if steps % args.every == 0:
            mean = torch.stack(window).float().mean(0).cpu().tolist()
            window = []
            say('step %5d  %6.1f s  loss (mean of %d steps) %s' % (steps, time.perf_counter() - start, args.every, ' '.join('%.4f' % v for v in mean)))
            if time.perf_counter() - start > args.seconds:
                break
    torch.cuda.synchronize()
    took = time.perf_counter() - start
    say('%d steps in %.1f s: %.1f ms per step with generation, augmentation and ground-truth maps in the loop' % (steps, took, 1e3 * took / steps))
    held = DeviceBatches(S.SynthTextBatches(4, 16, (640, 640), seed=1, device=dev), dev, training=False)
    loss, score = evaluate(model, DBLoss(), held, device=dev, detection=True)
    say('64 held-out images (seed 1): test loss %.4f, IoU-metric precision %.4f recall %.4f hmean %.4f' % (loss, score['precision'], score['recall'], score['hmean']))
    say('pixel metric: %s' % ' '.join('%s %.4f' % (k, v) for k, v in sorted(score.items()) if k not in ('precision', 'recall', 'hmean') and isinstance(v, float)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', choices=['time', 'pretrain'], required=True)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--seconds', type=float, default=150.0)
    ap.add_argument('--every', type=int, default=100)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    (part_time if args.part == 'time' else part_pretrain)(args, say)
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()
