#!/usr/bin/env python3
"""Huffman decoding on the device against the host path, for the two workloads of tools/jpeg_probe.py (16 x 1280 x 720 and
32 x 1280 x 1280, 4:2:0, quality 90), both paths in the same run with their pixels compared.

Prints, per workload (medians of timed repetitions after warm-up):
  host      decode_jpeg_batch(entropy='host'), bytes -> synchronised device, wall clock; int16 coefficients over PCIe
  device    decode_jpeg_batch(entropy='device'), the same end point; compressed bytes and plan arrays over PCIe
  plan      parse_streams alone (host, wall clock)
  passes    dbn_jpeg_dhuff on the device (device events) with the default rounds, with 0 rounds, and so per propagation
            launch; the launch after which no state of any image changed; images handed to the host decoder
One process touches the GPU; every step runs under its own alarm; run the probe under an outer time limit as well.
Usage: timeout -k 10 600 python tools/jpeg_dhuff_probe.py [--reps 20] [--out file]
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from jpeg_probe import encode, step, text_image, wall  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(0)
    loads = [(N, H, W, step(300, lambda: [encode(text_image(rng, H, W)) for _ in range(N)])) for N, H, W in ((16, 720, 1280), (32, 1280, 1280))]
    import torch
    from db_text_minimal_amd import decode_jpeg_batch, entropy_decode_device, parse_streams
    from db_text_minimal_amd import jpeg as J
    assert torch.cuda.is_available(), 'the probe times the device: it needs a GPU'
    dev = torch.device('cuda', 0)

    def events(fn, reps):
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

    for N, H, W, datas in loads:
        px, jb = N * H * W, sum(len(d) for d in datas)
        say('jpeg_dhuff_probe: %d x %dx%d, 4:2:0 quality 90, %.2f MB of JPEG (%.2f B per pixel)' % (N, W, H, jb / 1e6, jb / px))

        def run(entropy):
            out = decode_jpeg_batch(datas, dev, entropy=entropy)
            torch.cuda.synchronize()
            return out

        a, b = run('host'), run('device')
        assert torch.equal(a[0], b[0]) and a[1] == b[1], 'the two paths give different pixels'
        t_h = step(300, lambda: wall(lambda: run('host'), max(5, args.reps // 2)))
        t_d = step(300, lambda: wall(lambda: run('device'), max(5, args.reps // 2)))
        st = parse_streams(datas)
        plan = sum(getattr(st, k).nbytes for k in ('desc', 'tables', 'info', 'segments', 'sub_base', 'wgtab'))
        say('host    entropy=\'host\', bytes -> synchronised device (measured, wall): %.1f ms  %.0f images/s; %.1f MB of coefficients over PCIe (%.2f B per pixel)'
            % (t_h, 1e3 * N / t_h, st.coef_elems * 2 / 1e6, st.coef_elems * 2 / px))
        say('device  entropy=\'device\', the same end point, pixels equal (measured, wall): %.1f ms  %.0f images/s; %.2f MB of streams + %.2f MB of plan over PCIe (%.2f B per pixel)'
            % (t_d, 1e3 * N / t_d, jb / 1e6, plan / 1e6, (jb + plan) / px))
        t_p = step(300, lambda: wall(lambda: parse_streams(datas), max(5, args.reps // 2)))
        say('plan    parse_streams, %d segments, %d subsequences, %d workgroups (measured, wall): %.2f ms' % (len(st.segments), st.sub_base[-1], len(st.wgtab), t_p))
        coef = torch.empty(st.coef_elems, dtype=torch.int16, device=dev)
        ws = torch.empty(J.dhuff_workspace_bytes(st), dtype=torch.uint8, device=dev)
        t = {r: step(120, lambda: events(lambda: J._dhuff_launch(st, dev, r, coef, ws), args.reps)) for r in (J.DHUFF_ROUNDS, 0)}
        res = J._dhuff_launch(st, dev, J.DHUFF_ROUNDS, coef, ws).cpu().numpy()
        used = [int(np.nonzero(res[1:, n] == 0)[0][0]) if (res[1:, n] == 0).any() else -1 for n in range(N)]
        obj = entropy_decode_device(st, dev)
        say('passes  uploads + dbn_jpeg_dhuff (measured, device events): %.3f ms with %d rounds, %.3f ms with 0: %.3f ms per propagation launch; '
            'no state changed from launch %d on (worst image); %d of %d images handed to the host decoder; workspace %.2f MB'
            % (t[J.DHUFF_ROUNDS], J.DHUFF_ROUNDS, t[0], (t[J.DHUFF_ROUNDS] - t[0]) / J.DHUFF_ROUNDS, max(used), int(obj.host_decoded.sum()), N, ws.numel() / 1e6))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
