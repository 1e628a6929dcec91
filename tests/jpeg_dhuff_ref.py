"""A plain Python restatement of the device Huffman decoder (csrc/jpeg_dhuff.hip): the scan cut at its markers into restart
intervals, each cut into subsequences of S bits of the stuffed stream, the decoder state (bit position, block in the MCU,
zigzag index) propagated to a fixed point with the device's launch structure (W subsequences per workgroup, rounds
inside a workgroup until it stands, one round across workgroups per launch), block counts, their scan, the write pass with
its checks, and the segmented DC prefix sum.  Same S, same speculative rule (a code in no table is one bit, a run past 63
ends the block, a symbol that would end behind the segment is not taken).

  segments(data)                 -> (Header, [(first byte, end byte, first MCU, MCUs, n of the RSTn in front or -1)]) or (Header, None)
  decode(data, max_rounds=R)     -> Result: .coefs (as jpeg_ref.entropy_decode's), .flagged, .converged, .rounds (launches after
                                    the first until nothing changed; None if that was not seen), .host (the device path would
                                    hand this image to the host decoder)
"""
import numpy as np

import jpeg_ref as R

S, W, ROUNDS = 1024, 256, 4
CAP = S + 64


def segments(data):
    data = bytes(data)
    h = R.parse(data)
    n, mcus = len(data), h.mcux * h.mcuy
    want = -(-mcus // h.ri) if h.ri else 1
    p = first = h.scan_start
    out = []
    while True:
        q = data.find(b'\xff', p)
        if q < 0 or q + 1 >= n:
            return h, None
        m = data[q + 1]
        if m == 0:
            p = q + 2
            continue
        if m == 0xFF:
            return h, None
        k = len(out)
        rst = 0xD0 <= m <= 0xD7
        if (k >= want - 1 or m != 0xD0 + (k & 7)) if rst else k != want - 1:
            return h, None
        out.append((first, q, k * h.ri if h.ri else 0, min(h.ri, mcus - k * h.ri) if h.ri else mcus, (k - 1) & 7 if k else -1))
        if not rst:
            return h, out
        first = p = q + 2


class _Tab:
    def __init__(self, table):
        self.tab, self.vals = table

    def symbol(self, w):
        """(length, symbol) of the code at the top of the 32-bit window w, or None"""
        for l in range(1, 17):
            code = w >> (32 - l)
            lo, hi, first = self.tab[l - 1]
            if hi >= 0 and lo <= code <= hi:
                i = first + code - lo
                return (l, self.vals[i]) if i < len(self.vals) else None
        return None


class _Seg:
    def __init__(self, data, h, row, tabs, bpm, nl):
        self.d, self.first, self.end, self.mcu0, self.mcus, _ = (data, ) + tuple(row)
        self.bits = (self.end - self.first) * 8
        self.ns = -(-self.bits // S) if self.bits else 1
        self.tabs, self.bpm, self.nl, self.want = tabs, bpm, nl, row[3] * bpm
        self.memo = {}

    def guess(self, i):
        b = self.first + i * (S // 8)
        pos = i * S
        if i > 0 and b < self.end and self.d[b] == 0 and self.d[b - 1] == 0xFF:
            pos += 8
        return (pos, 0, 0)

    def walk(self, i, st, stop=0, put=None):
        """-> (state, blocks completed, first error, overran)"""
        if put is None and stop == 0 and (i, st) in self.memo:
            return self.memo[(i, st)]
        d, first, end = self.d, self.first, self.end
        pos, j, k = st
        E = min((i + 1) * S, self.bits)
        blocks, err, over = 0, 0, False
        it = 0
        while it < CAP and pos < E:
            it += 1
            if stop > 0 and blocks >= stop:
                break
            b, bit = first + (pos >> 3), pos & 7
            idx, acc, nx = b, 0, []
            for _ in range(5):
                v = d[idx] if idx < end else 0
                acc = acc << 8 | v
                idx += 2 if (v == 0xFF and idx + 1 < end and d[idx + 1] == 0) else 1
                nx.append(idx)
            w = (acc >> (8 - bit)) & 0xFFFFFFFF
            c = 0 if j < self.nl else j - self.nl + 1
            hit = self.tabs[2 * c + (1 if k else 0)].symbol(w)
            total, nk, zz, val, e, done = 1, k, -1, 0, 0, False
            if hit is None:
                e = 2
            else:
                ln, sym = hit
                s, r = sym & 15, sym >> 4
                v = ((w << ln) & 0xFFFFFFFF) >> (32 - s) if s else 0
                x = v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v
                if k == 0:
                    if sym > 11:
                        e = 2
                    total, zz, val, nk = ln + s, 0, x, 1
                elif s == 0:
                    total = ln
                    if r != 15:
                        done = True
                    else:
                        nk = k + 16
                        if nk > 64:
                            e = 3
                        done = nk >= 64
                else:
                    total = ln + s
                    if k + r > 63:
                        e, done = 3, True
                    else:
                        zz, val = k + r, x
                        nk = zz + 1
                        done = nk == 64
            adv = (bit + total) >> 3
            npos = ((nx[adv - 1] if adv else b) - first) * 8 + ((bit + total) & 7)
            if npos > self.bits:
                over = True
                break
            if e and not err:
                err = e
            if zz >= 0 and put is not None:
                put(blocks, zz, val)
            pos = npos
            if done:
                k, j, blocks = 0, (j + 1) % self.bpm, blocks + 1
            else:
                k = nk
        out = ((pos, j, k), blocks, err, over)
        if put is None and stop == 0:
            self.memo[(i, st)] = out
        return out


class Result:
    pass


KNOWN = (0, 0, 0)


def decode(data, max_rounds=ROUNDS, lanes=W):
    data = bytes(data)
    h, rows = segments(data)
    res = Result()
    res.header, res.coefs, res.rounds, res.launch_changed = h, None, None, []
    if rows is None:
        res.flagged, res.converged, res.host = True, False, True
        return res
    nl = h.samp[0][0] * h.samp[0][1] if h.ncomp == 3 else 1
    bpm = nl + 2 if h.ncomp == 3 else 1
    tabs = []
    for c in range(h.ncomp):
        tabs += [_Tab(h.dc[h.scan[c][0]]), _Tab(h.ac[h.scan[c][1]])]
    segs = [_Seg(data, h, r, tabs, bpm, nl) for r in rows]
    subs = [(s, i) for s in segs for i in range(s.ns)]  # the image's subsequences in order
    n = len(subs)
    prev = cur = None
    for launch in range(max_rounds + 1):
        cur = [None] * n
        changed = False
        for g0 in range(0, n, lanes):
            cnt = min(lanes, n - g0)
            ins, outs = [], []
            for t in range(cnt):
                s, i = subs[g0 + t]
                st = KNOWN if i == 0 else (s.guess(i) if launch == 0 else prev[g0 + t - 1])
                ins.append(st)
                outs.append(s.walk(i, st)[0])
            for _ in range(cnt + 1):
                any_ch = False
                new = list(outs)
                for t in range(1, cnt):
                    s, i = subs[g0 + t]
                    if i > 0 and outs[t - 1] != ins[t]:
                        ins[t] = outs[t - 1]
                        new[t] = s.walk(i, ins[t])[0]
                        any_ch = True
                outs = new
                if not any_ch:
                    break
            cur[g0:g0 + cnt] = outs
            if launch == 0:
                changed = changed or subs[g0][1] > 0
            else:
                changed = changed or any(outs[t] != prev[g0 + t] for t in range(cnt))
        res.launch_changed.append(changed)
        if not changed and res.rounds is None:
            res.rounds = launch
        prev = cur
    res.converged = not res.launch_changed[-1]
    # counting, scan, writing
    coefs = [np.zeros((bh * bw, 64), np.int16) for bh, bw in h.grid]
    entry = [KNOWN if i == 0 else cur[g - 1] for g, (s, i) in enumerate(subs)]
    counts = [s.walk(i, entry[g])[1] for g, (s, i) in enumerate(subs)]
    scan = np.concatenate([[0], np.cumsum(counts)])
    flagged = False
    sfirst = {}
    for g, (s, i) in enumerate(subs):
        if i == 0:
            sfirst[id(s)] = g
    for g, (s, i) in enumerate(subs):
        base = int(scan[g] - scan[sfirst[id(s)]])
        if base >= s.want:
            continue

        def put(blocks, zz, val, s=s, base=base):
            blk = base + blocks
            if blk >= s.want or val == 0:
                return
            mcu, j = s.mcu0 + blk // bpm, blk % bpm
            my, mx = divmod(mcu, h.mcux)
            if j < nl:
                v, u = divmod(j, h.samp[0][0])
                coefs[0][(my * h.samp[0][1] + v) * h.grid[0][1] + mx * h.samp[0][0] + u, R.ZIGZAG[zz]] = R._wrap16(val)
            else:
                coefs[j - nl + 1][mcu, R.ZIGZAG[zz]] = R._wrap16(val)

        (pos, _, _), blocks, err, over = s.walk(i, entry[g], s.want - base, put)
        if err:
            flagged = True
        if base + blocks >= s.want:
            b = s.first + (pos >> 3)  # less than a byte of data may be left: the rest of this byte (and its stuffed 00)
            if pos & 7:
                b += 2 if (data[b] == 0xFF and b + 1 < s.end and data[b + 1] == 0) else 1
            if b < s.end:
                flagged = True
        elif over or i == s.ns - 1:
            flagged = True
    # DC differences -> values, per component over scan order within each restart interval
    for c in range(h.ncomp):
        bc = nl if c == 0 else 1
        pred = 0
        for q in range(h.mcux * h.mcuy * bc):
            mcu, jj = divmod(q, bc)
            if jj == 0 and (mcu % h.ri == 0 if h.ri else mcu == 0):
                pred = 0
            my, mx = divmod(mcu, h.mcux)
            if c == 0:
                v, u = divmod(jj, h.samp[0][0])
                at = (my * h.samp[0][1] + v) * h.grid[0][1] + mx * h.samp[0][0] + u
            else:
                at = mcu
            pred = R._wrap16(pred + int(coefs[c][at, 0]))
            coefs[c][at, 0] = pred
    res.coefs, res.flagged = coefs, flagged
    res.host = flagged or not res.converged
    return res
