#!/usr/bin/env python3
"""Achieved HBM rate of the optimizer family (csrc/optim_groups.hip) at the flat buffer of ResNet-18-FPN-DBHead
(12 269 378 fp32 parameters), beside dbn_adam_step_ex of the SAME run, in the form of tools/optim_probe.py: HIP events, medians of
`--reps` launches after warm-up.  The variants ALTERNATE: every round launches each of them once, so that a drift of the machine (clocks,
other tenants) falls on all of them alike.

  adam_ex          dbn_adam_step_ex without vmax, no clipping, no decay                                           28 B / parameter
  sgd              dbn_sgd_step, momentum 0: reads p, g, writes p                                                 12 B
  sgd_mom / _nest  ... with the momentum buffer (read and written), plain and nesterov                           20 B
  adamw            dbn_adamw_step, one group, decoupled decay, no table: the traffic and arithmetic of adam_ex    28 B
  adamw_split      ... two groups under the run table split_decay() gives ResNet-18                              28 B
  adamw_maxruns    ... eight groups under the maximum number of runs (1024, evenly spaced)                       28 B
  *_ema            each of these with the shadow read and written                                                +8 B

Each line: median milliseconds with the 10th and 90th percentile of the launches, B/param by construction, GB/s from the median, and
the median relative to adam_ex's.  One figure is a condition: `adamw`
within 5 % of `adam_ex` (the margin is for a shared machine, not for a slower kernel); the probe exits with status 1 when it is missed.
Nothing is flushed between launches and the buffers (49 MB each) sit partly in the Infinity Cache: upper bounds on what a training
step sees, as in optim_probe.py.
Usage: python tools/optim_family_probe.py [--reps 50] [--n 12269378] [--out profiles/optim_family_probe.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from db_text_minimal_amd import DBTextModel, FusedSGD, split_decay  # noqa: E402
from db_text_minimal_amd._lib import check, lib  # noqa: E402
from db_text_minimal_amd.engine import flat_layout  # noqa: E402
from db_text_minimal_amd.optim import MAX_RUNS, build_runs  # noqa: E402


def resnet18_split_runs(n4):
    """the run table of split_decay() on DBTextModel (host only), cut to n4 quads"""
    m = DBTextModel()
    opt = FusedSGD(m, lr=0.1, param_groups=split_decay(m, 1e-4))
    sizes = [p.numel() for _, p in m.engine.live_params]
    ends, groups = build_runs(flat_layout(sizes)[0], sizes, opt.group_of_params())
    keep = [(min(e, n4), g) for e, g in zip(ends, groups)]
    keep = [eg for i, eg in enumerate(keep) if i == 0 or eg[0] > keep[i - 1][0]]
    return [e for e, _ in keep[:-1]] + [n4], [g for _, g in keep]


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
    p, g = (torch.randn(n, device=dev, generator=gen) * s for s in (1.0, 1e-2))
    m, v, buf = (torch.zeros(n, device=dev) for _ in range(3))
    shadow = p.clone()
    n4 = (n + 3) // 4
    floats = lambda xs: (ctypes.c_float * len(xs))(*xs)

    def table(ends, groups):
        t = torch.tensor([ends, groups], dtype=torch.int32, device=dev)
        return t, t[0].data_ptr(), t[1].data_ptr(), len(ends)

    split = table(*resnet18_split_runs(n4))
    most = table([n4 * (i + 1) // MAX_RUNS for i in range(MAX_RUNS)], [(3 * i + 1) % 8 for i in range(MAX_RUNS)])
    one = (floats([1e-3]), floats([1e-2]), 1, None, None, 0)
    two = (floats([1e-3, 5e-4]), floats([1e-2, 0.0]), 2) + split[1:]
    eight = (floats([1e-3 / (i + 1) for i in range(8)]), floats([1e-2 * i for i in range(8)]), 8) + most[1:]
    step = [0]

    def adam_ex():
        step[0] += 1
        check(L.dbn_adam_step_ex(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), None, n, 1e-3, 0.9, 0.999, 1e-8, 0.0, step[0], 1.0, None, 0.0,
                                 st), 'adam_step_ex')

    def adamw(groups, ema):
        def fn():
            step[0] += 1
            check(L.dbn_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), None, n, *groups, 0.9, 0.999, 1e-8, 1, step[0], 1.0, None,
                                   0.0, shadow.data_ptr() if ema else None, 0.999, 0.001, st), 'adamw_step')
        return fn

    def sgd(mu, nesterov, ema):
        return lambda: check(L.dbn_sgd_step(p.data_ptr(), g.data_ptr(), buf.data_ptr() if mu else None, n, *one, mu, 0.0, nesterov, 0, 1.0, None, 0.0,
                                            shadow.data_ptr() if ema else None, 0.999, 0.001, st), 'sgd_step')

    variants = [('adam_ex', adam_ex, 28)]
    for ema in (False, True):
        tag, extra = ('_ema', 8) if ema else ('', 0)
        # (adamw directly behind adam_ex: the two launches of the condition find the same buffers in the cache)
        variants += [('adamw' + tag, adamw(one, ema), 28 + extra), ('adamw_split' + tag, adamw(two, ema), 28 + extra),
                     ('adamw_maxruns' + tag, adamw(eight, ema), 28 + extra), ('sgd' + tag, sgd(0.0, 0, ema), 12 + extra),
                     ('sgd_mom' + tag, sgd(0.9, 0, ema), 20 + extra), ('sgd_nest' + tag, sgd(0.9, 1, ema), 20 + extra)]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('optim_family_probe: n = %d fp32 elements (%.1f MB a buffer), %d rounds over %d alternating variants, HIP events, one run; '
        'split_decay table: %d runs' % (n, 4 * n / 1e6, args.reps, len(variants), split[3]))
    for _ in range(5):
        for _, fn, _ in variants:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in variants}
    for _ in range(args.reps):
        for name, fn, _ in variants:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    med = {name: statistics.median(ts) for name, ts in times.items()}
    for name, _, bpp in variants:
        ts = sorted(times[name])
        lo, hi = ts[len(ts) // 10], ts[-1 - len(ts) // 10]  # the middle 80 % of the launches: the spread behind the median
        say('%-18s (measured) %7.4f ms [%.4f .. %.4f]  %2d B/param  %7.1f GB/s  %.3f x adam_ex' % (name, med[name], lo, hi, bpp,
                                                                                                   bpp * n / med[name] / 1e6,
                                                                                                   med[name] / med['adam_ex']))
    ratio = med['adamw'] / med['adam_ex']
    ok = ratio <= 1.05
    say('condition: adamw (one group, no shadow) takes %.3f x adam_ex of this run: %s 5 %%' % (ratio, 'within' if ok else 'NOT within'))
    assert bool(torch.isfinite(p).all()), 'the parameters left the finite range'
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
