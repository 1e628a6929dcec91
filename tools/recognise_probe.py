#!/usr/bin/env python3
"""Cost of the stage around the text recogniser (db_text_minimal_amd.recognise) at the sizes of one dense inference batch.

Steps (each a child process under its own `timeout`; the first that fails ends the probe):
  input   words_to_input on 9 600 crops of 32 x 100 (grey, float32)
  ctc     greedy_decode 'ctc' on logits [9600, 26, 37] float32
  attn    greedy_decode 'attn' on logits [2048, 40, 6625] float16
Each prints
  device  the launches alone, median of timed calls after warm-up (device events), against the byte floor at 8 TB/s:
          the input read once and every output written once (the decode's 8-byte-per-step workspace written and read)
  torch   the composition a user would write today on the same device (softmax, max, cumprod; for `input` a float grey),
          device events, and for the decode the reference's per-character Python loop for the strings, wall clock
  e2e     greedy_decode + converter.decode to strings, wall clock to the host
Usage: python tools/recognise_probe.py [--reps 50] [--out file]        (all steps)
       python tools/recognise_probe.py --step input|ctc|attn [--reps 50]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

STEPS = {'input': 180, 'ctc': 240, 'attn': 300}  # seconds each child may take
BW = 8e12  # bytes / s
CHARS = '0123456789abcdefghijklmnopqrstuvwxyz'


def time_launch(fn, reps):
    import torch
    for _ in range(5):
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


def time_wall(fn, reps):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts)


def step_input(reps):
    import numpy as np
    import torch
    from db_text_minimal_amd import words_to_input
    import recognise_ref as R
    K, h, w = 9600, 32, 100
    crops = np.random.default_rng(0).integers(0, 256, (K, h, w, 3), dtype=np.uint8)
    dev = torch.from_numpy(crops).cuda()
    t = time_launch(lambda: words_to_input(dev), reps)
    nbytes = K * h * w * (3 + 4)
    floor = nbytes / BW * 1e3
    print('input  %d crops of %d x %d, grey float32' % (K, h, w))
    print('device words_to_input (measured) %.4f ms   floor %.4f ms (%.1f MB at 8 TB/s)  %.0f%% of floor rate' % (t, floor, nbytes / 1e6, 100 * floor / t))
    wts = torch.tensor([0.299, 0.587, 0.114], device='cuda')

    def composed():
        return (dev.float() * wts).sum(-1).round_().div_(255).sub_(0.5).div_(0.5).unsqueeze(1)

    print('torch  float grey + normalise, composed (measured) %.4f ms' % time_launch(composed, reps))
    got = words_to_input(dev[:64]).cpu().numpy()
    assert np.array_equal(got.view(np.int32), R.words_to_input(crops[:64]).view(np.int32)), 'device differs from the restatement'
    print('check  device == restatement on 64 crops')


def _reference_strings(idx, prob, table, attn):
    """the reference's host work per word: the converter's per-character loop, '[s]' by str.find, cumprod of the prefix"""
    out = []
    for b in range(idx.shape[0]):
        t = idx[b].tolist()
        if attn:
            s = ''.join(table[i] for i in t)
            e = s.find('[s]')
            out.append((s[:e], float(prob[b][:e].cumprod(0)[-1]) if e > 0 else 1.0))
        else:
            chars = [table[t[i]] for i in range(len(t)) if t[i] != 0 and not (i > 0 and t[i - 1] == t[i])]
            out.append((''.join(chars), float(prob[b].cumprod(0)[-1])))
    return out


def step_decode(mode, reps):
    import numpy as np
    import torch
    import torch.nn.functional as F
    from db_text_minimal_amd import AttnLabelConverter, CTCLabelConverter, greedy_decode
    import recognise_ref as R
    if mode == 'ctc':
        B, T, C, dtype, conv = 9600, 26, 37, torch.float32, CTCLabelConverter(CHARS)
    else:
        B, T, C, dtype = 2048, 40, 6625, torch.float16
        conv = AttnLabelConverter([chr(0x4E00 + i) for i in range(C - 2)])
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(B, T, C, generator=g) * 2
    win = torch.randint(0, C, (B, T), generator=g)
    logits.scatter_add_(2, win[..., None], torch.full((B, T, 1), 12.0))  # a confident recogniser: scores stay above fp32's underflow
    if mode == 'attn':
        logits[torch.arange(B), torch.randint(3, T, (B, ), generator=g), 1] += 30
    dev = logits.to(dtype).cuda()
    t = time_launch(lambda: greedy_decode(dev, mode), reps)
    nbytes = B * T * C * dev.element_size() + B * T * 16 + B * T * 4 + B * 8
    floor = nbytes / BW * 1e3
    print('%s    logits [%d, %d, %d] %s' % (mode, B, T, C, str(dtype).replace('torch.', '')))
    print('device greedy_decode, both launches (measured) %.4f ms   floor %.4f ms (%.1f MB at 8 TB/s)  %.0f%% of floor rate' % (
        t, floor, nbytes / 1e6, 100 * floor / t))

    def composed():
        _, idx = dev.max(2)
        prob, _ = F.softmax(dev, dim=2).max(dim=2)
        return idx, prob, prob.cumprod(1)[:, -1]

    print('torch  max + softmax + max + cumprod, composed (measured) %.4f ms' % time_launch(composed, reps))
    idx, prob, _ = composed()
    idx_h, prob_h = idx.cpu(), prob.float().cpu()
    t0 = time.perf_counter()
    ref = _reference_strings(idx_h, prob_h, conv.character, mode == 'attn')
    print('torch  ... plus the reference\'s Python loop for the %d strings on the host (measured, wall clock) %.1f ms' % (B, 1e3 * (time.perf_counter() - t0)))

    def e2e():
        codes, count, score = greedy_decode(dev, mode)
        return conv.decode(codes, count), score.cpu()

    print('e2e    greedy_decode + decode to %d strings on the host (measured, wall clock) %.2f ms' % (B, time_wall(e2e, max(5, reps // 5))))
    words, score = e2e()
    assert words == [r[0] for r in ref], 'device strings differ from the torch composition'
    n = 256
    codes, count, want = R.greedy_decode(logits[:n].to(dtype).double().numpy(), mode)
    err = np.abs(score[:n].double().numpy() - want) / want
    print('check  strings == torch composition on all %d; score against fp64 on %d: worst relative error %.2e (bound %.2e)' % (
        B, n, err.max(), T * (C + 8) * 2.0 ** -23))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--step', choices=sorted(STEPS), default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), 'the probe times the device: it needs a GPU'
        if args.step == 'input':
            step_input(args.reps)
        else:
            step_decode(args.step, args.reps)
        return 0
    lines = []
    for step in ('input', 'ctc', 'attn'):
        cmd = ['timeout', '-k', '10', str(STEPS[step]), sys.executable, os.path.abspath(__file__), '--step', step, '--reps', str(args.reps)]
        res = subprocess.run(cmd, capture_output=True, text=True)
        print(res.stdout, end='', flush=True)
        lines.append(res.stdout)
        if res.returncode != 0:  # a fault, an abort or a time limit: nothing more is started on the device
            print(res.stderr[-3000:], file=sys.stderr)
            print('recognise_probe: step %s ended with status %d; stopping' % (step, res.returncode), file=sys.stderr)
            return res.returncode
    if args.out:
        with open(args.out, 'w') as f:
            f.write(''.join(lines))
    return 0


if __name__ == '__main__':
    sys.exit(main())
