"""numpy restatement of the labels of db_text_minimal_amd.render (draw_glyphs of csrc/render.hip): layout and the winding
predicate of DESIGN section 29, read from the committed table db_text_minimal_amd/fonts/dejavu_sans.txt alone.  No code is
shared with render.py.  All arithmetic is int64, vectorised over each glyph's bounding box (the bounds that make 64 bits
enough are in csrc/render.hip; winding_exact is the same predicate on Python integers)."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, 'db_text_minimal_amd', 'fonts', 'dejavu_sans.txt')
L = 64 * 2048  # lattice units per pixel
_cache = {}


def font():
    """{'head': {name: int}, 'adv': {code point: advance}, 'contours': {code point: [int64 [P, 2]]}}"""
    if not _cache:
        head, adv, contours, cp = {}, {}, {}, None
        for line in open(TABLE):
            t = line.split()
            if not t:
                continue
            if t[0] == '#':
                if len(t) == 3 and t[2].lstrip('-').isdigit():
                    head[t[1]] = int(t[2])
            elif t[0] == 'glyph':
                cp = int(t[1])
                adv[cp], contours[cp] = int(t[2]), []
            else:
                contours[cp].append(np.array(t, np.int64).reshape(-1, 2))
        _cache.update(head=head, adv=adv, contours=contours)
    return _cache


def size64(height):
    h = font()['head']
    return int(np.rint(float(height) * 64 * h['units_per_EM'] / h['cap_height']))


def code(ch):
    return ord(ch) if 32 <= ord(ch) <= 126 else ord('?')


def winding(contours, s, Px, Py):
    """the winding number of closed polylines (font units, scaled by s) about lattice points Px, Py (int64 arrays)"""
    wn = np.zeros(Px.shape, np.int64)
    for c in contours:
        a, b = c * s, np.roll(c, -1, 0) * s
        for (ax, ay), (bx, by) in zip(a.tolist(), b.tolist()):
            if ay == by:
                continue
            cr = (bx - ax) * (Py - ay) - (by - ay) * (Px - ax)
            wn += ((ay <= Py) & (Py < by) & (cr > 0)).astype(np.int64) - ((by <= Py) & (Py < ay) & (cr < 0)).astype(np.int64)
    return wn


def winding_exact(contours, s, Px, Py):
    """the same on Python integers (no overflow possible), one point"""
    wn = 0
    for c in contours:
        pts = [(int(x) * s, int(y) * s) for x, y in c]
        for (ax, ay), (bx, by) in zip(pts, pts[1:] + pts[:1]):
            cr = (bx - ax) * (Py - ay) - (by - ay) * (Px - ax)
            wn += (1 if ay <= Py < by and cr > 0 else 0) - (1 if by <= Py < ay and cr < 0 else 0)
    return wn


def paint(mask, contours, s, pen, x, y, sub=(0, 0)):
    """mask |= the pixels of closed contours (font units) drawn at pen `pen` of a label with origin (x, y); sub: 64ths of a
    pixel added to the origin (the product takes whole pixels only; the pin against matplotlib uses a generic position)"""
    H, W = mask.shape
    if not contours:
        return
    p = np.concatenate(contours)
    # Px = L px + L / 2 - L x - pen s, Py = L y - L py - L / 2; the pixels with their centre in the scaled bounding box
    bx, by = L * x + 2048 * sub[0] + pen * s - L // 2, L * y + 2048 * sub[1] - L // 2
    x0, x1 = -((-(int(p[:, 0].min()) * s + bx)) // L), (int(p[:, 0].max()) * s + bx) // L
    y0, y1 = -((-(by - int(p[:, 1].max()) * s)) // L), (by - int(p[:, 1].min()) * s) // L
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1)
    if x0 > x1 or y0 > y1:
        return
    py, px = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.int64)
    mask[y0:y1 + 1, x0:x1 + 1] |= winding(contours, s, L * px - bx, by - L * py) != 0


def label_mask(H, W, labels, height=16, sub=(0, 0)):
    """bool [H, W]: the pixels the labels [(text, (x, y))] of one image paint at cap height `height`"""
    f, s = font(), size64(height)
    mask = np.zeros((H, W), bool)
    for text, (x, y) in labels:
        pen = 0
        for ch in text:
            paint(mask, f['contours'][code(ch)], s, pen, int(x), int(y), sub)
            pen += f['adv'][code(ch)]
    return mask


def advance(text):
    return sum(font()['adv'][code(ch)] for ch in text)


def background_mask(H, W, labels, height=16):
    """the rectangles behind the labels: from the pen's start to its end and from descender to ascender, plus a margin of
    2 pixels rounded up to whole font units"""
    f, s = font(), size64(height)
    m = -((-2 * L) // s)
    mask = np.zeros((H, W), bool)
    for text, (x, y) in labels:
        x0, x1, y0, y1 = -m, advance(text) + m, f['head']['descender'] - m, f['head']['ascender'] + m
        paint(mask, [np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.int64)], s, 0, int(x), int(y))
    return mask


def draw_labels(img, labels, color=(255, 0, 0), height=16, background=None):
    out = img.copy()
    if background is not None:
        out[background_mask(img.shape[0], img.shape[1], labels, height)] = np.array(background, np.uint8)
    out[label_mask(img.shape[0], img.shape[1], labels, height)] = np.array(color, np.uint8)
    return out
