"""numpy restatement of the synthetic scene text of csrc/synth.hip (db_text_minimal_amd/synth.py), read from the
committed table db_text_minimal_amd/fonts/dejavu_sans.txt alone.  No code is shared with the package.  All arithmetic is int64,
vectorised over the pixels of each instance's box (the bounds that make 64 bits enough are the definition's: |a| < 2^19, |t| <= 2^35,
spans < 2^30); winding_exact and blend_exact are the same on Python integers."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, 'db_text_minimal_amd', 'fonts', 'dejavu_sans.txt')
L = 1 << 20  # lattice units per pixel
A_LIM, T_LIM, SPAN_LIM = 1 << 19, 1 << 35, 1 << 30
_cache = {}


def font():
    """{'head': {name: int}, 'adv': [advance of glyph g], 'contours': [per glyph a list of int64 [P, 2]]}, glyph g = code point 32 + g"""
    if not _cache:
        head, adv, contours = {}, [], []
        for line in open(TABLE):
            t = line.split()
            if not t:
                continue
            if t[0] == '#':
                if len(t) == 3 and t[2].lstrip('-').isdigit():
                    head[t[1]] = int(t[2])
            elif t[0] == 'glyph':
                assert int(t[1]) == 32 + len(adv)
                adv.append(int(t[2]))
                contours.append([])
            else:
                contours[-1].append(np.array(t, np.int64).reshape(-1, 2))
        _cache.update(head=head, adv=adv, contours=contours)
    return _cache


def glyph_of(ch):
    return (ord(ch) if 32 <= ord(ch) <= 126 else ord('?')) - 32


def edges_of(contours):
    """every edge of closed contours: int64 [E, 4] of ax, ay, bx, by (font units), horizontal ones included"""
    return np.concatenate([np.concatenate([c, np.roll(c, -1, 0)], 1) for c in contours]) if contours else np.zeros((0, 4), np.int64)


def box_of(contours):
    p = np.concatenate(contours)
    return int(p[:, 0].min()), int(p[:, 1].min()), int(p[:, 0].max()), int(p[:, 1].max())


def transform(edges, a):
    """font-unit edges under the matrix a = (a00, a01, a10, a11): lattice units relative to t"""
    e = np.asarray(edges, np.int64)
    return np.stack([a[0] * e[:, 0] + a[1] * e[:, 1], a[2] * e[:, 0] + a[3] * e[:, 1], a[0] * e[:, 2] + a[1] * e[:, 3], a[2] * e[:, 2] + a[3] * e[:, 3]], 1)


def winding(te, X, Y):
    """the winding sum of transformed edges te [E, 4] about the points X, Y (int64 arrays, relative to t)"""
    wn = np.zeros(X.shape, np.int64)
    for ax, ay, bx, by in te.tolist():
        if ay == by:
            continue
        cr = (bx - ax) * (Y - ay) - (by - ay) * (X - ax)
        wn += ((ay <= Y) & (Y < by) & (cr > 0)).astype(np.int64) - ((by <= Y) & (Y < ay) & (cr < 0)).astype(np.int64)
    return wn


def winding_exact(edges, a, X, Y):
    """the same on Python integers, one point, from the font-unit edges"""
    wn = 0
    a = [int(v) for v in a]
    for ex, ey, fx, fy in np.asarray(edges).tolist():
        ax, ay, bx, by = a[0] * ex + a[1] * ey, a[2] * ex + a[3] * ey, a[0] * fx + a[1] * fy, a[2] * fx + a[3] * fy
        cr = (bx - ax) * (Y - ay) - (by - ay) * (X - ax)
        wn += (1 if ay <= Y < by and cr > 0 else 0) - (1 if by <= Y < ay and cr < 0 else 0)
    return wn


def instance_box(a, t, box):
    """(x0, y0, x1, y1) of the glyph box (xmin, ymin, xmax, ymax) under a, relative to t, or None: the instance is not evaluated"""
    a, t = [int(v) for v in a], [int(v) for v in t]
    if any(abs(v) >= A_LIM for v in a) or any(abs(v) > T_LIM for v in t):
        return None
    xs = [a[0] * x + a[1] * y for x in (box[0], box[2]) for y in (box[1], box[3])]
    ys = [a[2] * x + a[3] * y for x in (box[0], box[2]) for y in (box[1], box[3])]
    if max(xs) - min(xs) >= SPAN_LIM or max(ys) - min(ys) >= SPAN_LIM:
        return None
    return min(xs), min(ys), max(xs), max(ys)


def samples_inside(H, W, contours, a, t, n=4):
    """bool [H n, W n]: the samples (n per axis and pixel, at (2 i + 1) L / (2 n)) inside the glyph; only those in its box are tested"""
    inside = np.zeros((H * n, W * n), bool)
    if not contours:
        return inside
    box = instance_box(a, t, box_of(contours))
    if box is None:
        return inside
    step, half = L // n, L // (2 * n)
    # sample index k along an axis sits at k * step + half - t
    k0 = [max(0, -((-(box[i] + int(t[i]) - half)) // step)) for i in range(2)]
    k1 = [min((W, H)[i] * n - 1, (box[i + 2] + int(t[i]) - half) // step) for i in range(2)]
    if k0[0] > k1[0] or k0[1] > k1[1]:
        return inside
    ky, kx = np.mgrid[k0[1]:k1[1] + 1, k0[0]:k1[0] + 1].astype(np.int64)
    wn = winding(transform(edges_of(contours), [int(v) for v in a]), kx * step + half - int(t[0]), ky * step + half - int(t[1]))
    inside[k0[1]:k1[1] + 1, k0[0]:k1[0] + 1] = wn != 0
    return inside


def coverage(H, W, contours, a, t):
    """int64 [H, W]: the samples of each pixel, of 16, inside the instance"""
    return samples_inside(H, W, contours, a, t).reshape(H, 4, W, 4).sum((1, 3)).astype(np.int64)


def blend(cur, cov, fg):
    """cur uint8 [H, W, 3] painted with colour fg by coverage cov [H, W] -> uint8"""
    c = cov[:, :, None]
    return ((c * np.array(fg, np.int64) + (16 - c) * cur.astype(np.int64) + 8) >> 4).astype(np.uint8)


def blend_exact(cur, cov, fg):
    return (cov * fg + (16 - cov) * cur + 8) // 16


M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox(counter, key):
    """Philox4x32-10: counter = four uint64 arrays (or ints) holding 32-bit values, key = (k0, k1) -> four words"""
    c = [np.asarray(v, np.uint64) for v in counter]
    k0, k1 = int(key[0]), int(key[1])
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def lattice_value(ix, iy, o, seed):
    return (philox((ix, iy, np.full_like(np.asarray(ix, np.uint64), o), np.zeros_like(np.asarray(ix, np.uint64))),
                   (seed & 0xFFFFFFFF, seed >> 32))[0] >> np.uint64(24)).astype(np.int64)


def background(H, W, base, amps, seed):
    """uint8 [H, W, 3]: the procedural background"""
    py, px = np.mgrid[0:H, 0:W].astype(np.int64)
    D = np.zeros((H, W), np.int64)
    for o, C in enumerate((64, 16, 4)):
        ix, iy, fx, fy = px // C, py // C, px % C, py % C
        T = np.zeros((H, W), np.int64)
        for cx, wx in ((0, C - fx), (1, fx)):
            for cy, wy in ((0, C - fy), (1, fy)):
                T += wx * wy * lattice_value((ix + cx).astype(np.uint64), (iy + cy).astype(np.uint64), o, int(seed))
        D += int(amps[o]) * (T - 128 * C * C) * (1 << (12 - 2 * (C.bit_length() - 1)))
    move = (D + (1 << 18)) >> 19  # floor
    return np.clip(np.array(base, np.int64)[None, None, :] + move[:, :, None], 0, 255).astype(np.uint8)


def render(shapes, backgrounds, recs, glyphs=None):
    """The images [uint8 [H, W, 3]] of shapes [(H, W)]: backgrounds[n] is (base, amps, seed) or a uint8 [H, W, 3] array; recs int64
    [R, 9] of {image, glyph, a00, a01, a10, a11, tx, ty, colour} painted in ascending order; glyphs: per glyph index its contours
    (default: the font).  A record with an image or glyph out of range, or one that is not evaluated, paints nothing."""
    glyphs = font()['contours'] if glyphs is None else glyphs
    out = []
    for n, (H, W) in enumerate(shapes):
        b = backgrounds[n]
        img = np.array(b, np.uint8).copy() if isinstance(b, np.ndarray) else background(H, W, *b)
        for rec in np.asarray(recs, np.int64).reshape(-1, 9).tolist():
            if rec[0] != n or not 0 <= rec[1] < len(glyphs) or not glyphs[rec[1]]:
                continue
            cov = coverage(H, W, glyphs[rec[1]], rec[2:6], rec[6:8])
            if cov.any():
                img = blend(img, cov, [rec[8] & 255, rec[8] >> 8 & 255, rec[8] >> 16 & 255])
        out.append(img)
    return out
