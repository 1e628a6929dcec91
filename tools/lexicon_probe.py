#!/usr/bin/env python3
"""Times the edit-distance kernels (db_text_minimal_amd.spotting, csrc/lexicon.hip) on the words of one batch:
  generic   9 600 queries of 3 - 12 classes against 90 000 lexicon entries of 2 - 15 classes, one group (Lexicon.nearest)
  strong    the same queries against 32 groups of 100 entries, query k in group k % 32 (Lexicon.nearest)
  pairs     9 600 pairs for edit_distances: those queries against 9 600 texts of 2 - 15 classes
All inputs are on the device before the clock starts (codes as greedy_decode returns them, the lexicon uploaded).  Per workload:
the median over --reps samples, after warm-up, of one call on the device clock (events around the call: the remap lookup and the
entry point's launches), the pairs (query, entry) scored per second, and the text classes (entry characters, one step of the
recurrence each) consumed per second.  No host baseline is claimed: there is no edit-distance library to compare with.  Needs a
GPU; there is no fallback.

  python tools/lexicon_probe.py [--reps 20] [--out FILE (appended)]
Run it as one step under a time limit:
  timeout -k 10 300 python tools/lexicon_probe.py --out profiles/lexicon_probe.txt
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHARS = '0123456789abcdefghijklmnopqrstuvwxyz'
K, GENERIC, GROUPS, PER_GROUP = 9600, 90000, 32, 100


def words(rng, n, lo, hi):
    return [''.join(CHARS[c] for c in rng.integers(10, 36, int(rng.integers(lo, hi + 1)))) for _ in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error('--reps must be at least 20')
    import torch
    sys.path.insert(0, ROOT)
    from db_text_minimal_amd import CTCLabelConverter, Lexicon, TextClasses, edit_distances
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
        return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))

    rng = np.random.default_rng(42)
    tc = TextClasses(CTCLabelConverter(CHARS))
    generic = words(rng, GENERIC, 2, 15)
    strong = [words(rng, PER_GROUP, 2, 15) for _ in range(GROUPS)]
    queries = words(rng, K, 3, 12)
    texts = words(rng, K, 2, 15)
    T = 26
    codes = np.full((K, T), -1, np.int32)
    for i, w in enumerate(queries):
        codes[i, :len(w)] = [CHARS.index(ch) + 1 for ch in w]
    codes = torch.from_numpy(codes).to(dev)
    count = torch.tensor([len(w) for w in queries], dtype=torch.int32, device=dev)
    group = torch.arange(K, dtype=torch.int32, device=dev) % GROUPS
    lex_generic, lex_strong = Lexicon(generic, tc, dev), Lexicon(strong, tc, dev)
    t_text, t_off = tc.encode(texts)
    # the pairs workload through the entry point's own form: the texts uploaded once, as edit_distances uploads them
    from db_text_minimal_amd._lib import check, lib
    pattern = tc.lookup(codes).contiguous()
    d_text, d_off = torch.from_numpy(t_text).to(dev), torch.from_numpy(t_off).to(dev)
    dist = torch.empty((K, ), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def pairs_launch():
        check(lib().dbn_edit_distance_pairs(pattern.data_ptr(), T, count.data_ptr(), d_text.data_ptr(), len(t_text), d_off.data_ptr(), None, K,
                                            dist.data_ptr(), stream), 'edit_distance_pairs')

    pairs_launch()
    assert torch.equal(dist, edit_distances((codes, count), texts, tc))  # the launch timed is the function's
    chars = lambda ws: sum(len(w) for w in ws)  # noqa: E731
    work = [('generic 9600 x 90000', lambda: lex_generic.nearest(codes, count), K * GENERIC, K * chars(generic)),
            ('strong 9600 x 100 of 32', lambda: lex_strong.nearest(codes, count, group),
             K * PER_GROUP, sum(chars(strong[k % GROUPS]) for k in range(K))),
            ('pairs 9600 (launch)', pairs_launch, K, chars(texts)),
            ('pairs 9600 (texts encoded, uploaded)', lambda: edit_distances((codes, count), texts, tc), K, chars(texts))]
    say('== lexicon_probe: %d queries of 3 - 12 classes, median of %d calls (one call per sample), %s' % (K, args.reps, torch.cuda.get_device_name(0)))
    say('%-38s %10s %9s %9s %12s %14s' % ('workload', 'median ms', 'min ms', 'max ms', 'pairs / s', 'classes / s'))
    for name, fn, n_pairs, n_classes in work:
        ms, lo, hi = device_ms(fn)
        say('%-38s %10.3f %9.3f %9.3f %12.3e %14.3e' % (name, ms, lo, hi, n_pairs / (ms * 1e-3), n_classes / (ms * 1e-3)))
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()
