#!/usr/bin/env python3
"""Achieved HBM rate of the optimizer kernels at the flat buffer of ResNet-18-FPN-DBHead (12 269 378 fp32 parameters), all timed with
HIP events in ONE run so that they can be read beside each other (csrc/optim.hip):

  adam       adam_kernel through dbn_adam_step: reads p, g, m, v, writes p, m, v                               28 B / parameter
  adam_ex    dbn_adam_step_ex without vmax (no clipping, no decay: the same arithmetic)                        28 B
  amsgrad    dbn_adam_step_ex with vmax, the clip coefficient read from device memory and weight decay        36 B
  norm       dbn_grad_sqnorm: both launches (the chunk sums and the one-workgroup index-order sum)              4 B
  fold       dbn_grad_accumulate, first = 0 (reads acc and g, writes acc)                                      12 B
  fold0      dbn_grad_accumulate, first = 1 (reads g, writes acc)                                               8 B

Each line: median milliseconds of `--reps` launches after warm-up, GB/s = bytes moved by construction / time, and that rate relative
to adam's of the same run.  The buffers (49 MB each) exceed no cache level's reach on purpose: nothing is flushed between launches, as
in a training step, where the optimizer follows the backward pass.
Usage: python tools/optim_probe.py [--reps 50] [--n 12269378] [--out profiles/optim_probe.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))  # (crop_probe imports its reference from there)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from db_text_minimal_amd._lib import check, lib  # noqa: E402
from crop_probe import time_launch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--n', type=int, default=12269378)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'the probe times the device: it needs a GPU'
    dev, n, L = torch.device('cuda'), args.n, lib()
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device=dev).manual_seed(0)
    p, g, acc = (torch.randn(n, device=dev, generator=gen) * s for s in (1.0, 1e-2, 1e-2))
    m, v, vmax = (torch.zeros(n, device=dev) for _ in range(3))
    ws = torch.empty(L.dbn_grad_sqnorm_ws_doubles(n), device=dev, dtype=torch.float64)
    sq = torch.zeros(1, device=dev, dtype=torch.float64)
    hp = (0.005, 0.9, 0.999, 1e-8)
    step = [0]

    def adam():
        step[0] += 1
        check(L.dbn_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, *hp, step[0], 1.0, st), 'adam_step')

    def adam_ex():
        step[0] += 1
        check(L.dbn_adam_step_ex(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), None, n, *hp, 0.0, step[0], 1.0, None, 0.0, st), 'adam_step_ex')

    def amsgrad():
        step[0] += 1
        check(L.dbn_adam_step_ex(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), vmax.data_ptr(), n, *hp, 0.01, step[0], 1.0,
                                 sq.data_ptr(), 1.0, st), 'adam_step_ex')

    def norm():
        check(L.dbn_grad_sqnorm(g.data_ptr(), n, ws.data_ptr(), sq.data_ptr(), st), 'grad_sqnorm')

    def fold(first):
        return lambda: check(L.dbn_grad_accumulate(acc.data_ptr(), g.data_ptr(), n, first, st), 'grad_accumulate')

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('optim_probe: n = %d fp32 elements (%.1f MB a buffer), %d launches each, HIP events, one run' % (n, 4 * n / 1e6, args.reps))
    norm()  # (amsgrad reads the squared norm)
    base = None
    for name, fn, bpp in (('adam', adam, 28), ('adam_ex', adam_ex, 28), ('amsgrad', amsgrad, 36), ('norm', norm, 4), ('fold', fold(0), 12),
                          ('fold0', fold(1), 8), ('adam', adam, 28)):
        ms = time_launch(fn, args.reps)
        rate = bpp * n / ms / 1e6
        base = rate if base is None else base
        say('%-8s (measured) %7.4f ms  %2d B/param  %7.1f GB/s  %.2f x adam' % (name, ms, bpp, rate, rate / base))
    assert bool(torch.isfinite(p).all()), 'the parameters left the finite range'
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
