#!/usr/bin/env python3
"""Writes dejavu_sans.txt, the glyph table render.py's labels are filled from: the outlines of DejaVu Sans (the font
matplotlib bundles, freely redistributable) for code points 32 .. 126, in integer font units, every quadratic flattened
into 8 chords.  Run once with matplotlib installed (the committed table comes from matplotlib 3.10.8); the package itself
never imports matplotlib, and tests/test_labels_cpu.py compares the table with what this script regenerates.

Format.  `#` lines: the header (matplotlib version, units_per_EM, ascender, descender, cap_height = the top of 'H').  Then
per glyph `glyph <code point> <advance> <contours>` followed by one line `x y x y ...` per closed contour (the closing
edge from the last point back to the first is implied).

Flattening.  FT2Font(path, hinting_factor=1).load_char(cp, flags=NO_SCALE).get_path() gives the outline in 1/64 font units
as floats: times 64 they are the font's integers.  Straight segments stay; a quadratic (p0; control p1, end p2) becomes the
chords through t = j / 8, j = 1 .. 8, each point (1-t)^2 p0 + 2t(1-t) p1 + t^2 p2 in float64, rounded with rint.  Consecutive
duplicate points and the CLOSEPOLY vertex are dropped.  The range holds no cubics (asserted)."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIRST, LAST, CHORDS = 32, 126, 8
MOVETO, LINETO, CURVE3, CURVE4, CLOSEPOLY = 1, 2, 3, 4, 79


def flatten(verts, codes):
    """path of one glyph (float64 [n, 2] font units, codes [n]) -> list of int64 [P, 2] closed contours"""
    contours, cur, i = [], [], 0
    while i < len(codes):
        c = int(codes[i])
        assert c != CURVE4, 'a cubic: not expected in DejaVu Sans 32 .. 126'
        if c == MOVETO:
            if cur:
                contours.append(cur)
            cur = [verts[i]]
            i += 1
        elif c == LINETO:
            cur.append(verts[i])
            i += 1
        elif c == CURVE3:
            assert int(codes[i + 1]) == CURVE3
            p0, p1, p2 = np.asarray(cur[-1], np.float64), verts[i], verts[i + 1]
            for j in range(1, CHORDS + 1):
                t = j / CHORDS
                cur.append(np.rint((1 - t) ** 2 * p0 + 2 * t * (1 - t) * p1 + t ** 2 * p2))
            i += 2
        else:
            assert c == CLOSEPOLY, c
            i += 1
    if cur:
        contours.append(cur)
    out = []
    for pts in contours:
        p = np.rint(np.asarray(pts, np.float64)).astype(np.int64)
        keep = np.ones(len(p), bool)
        keep[1:] = (p[1:] != p[:-1]).any(1)
        p = p[keep]
        if len(p) > 1 and (p[0] == p[-1]).all():  # the outline returns to its start: the closing edge is implied
            p = p[:-1]
        if len(p) >= 3:  # the font holds a few one-point contours ('u'): no area, no edges
            out.append(p)
    return out


def generate():
    """-> the text of the table"""
    import matplotlib
    from matplotlib.ft2font import FT2Font, LoadFlags
    font = FT2Font(os.path.join(matplotlib.get_data_path(), 'fonts', 'ttf', 'DejaVuSans.ttf'), hinting_factor=1)
    glyphs, points = [], 0
    for cp in range(FIRST, LAST + 1):
        g = font.load_char(cp, flags=LoadFlags.NO_SCALE)
        verts, codes = font.get_path()
        v = np.asarray(verts, np.float64) * 64
        assert (v == np.rint(v)).all(), 'the outline is not in whole font units'
        glyphs.append((cp, int(g.horiAdvance), flatten(v, codes)))
        points += sum(len(c) for c in glyphs[-1][2])
    adv = {cp: a for cp, a, _ in glyphs}
    cap = max(int(c[:, 1].max()) for c in glyphs[ord('H') - FIRST][2])
    assert (cap, adv[ord('A')], adv[32]) == (1493, 1401, 651), (cap, adv[ord('A')], adv[32])
    lines = ['# DejaVu Sans outlines, code points %d .. %d, quadratics as %d chords; written by make_glyphs.py' % (FIRST, LAST, CHORDS),
             '# matplotlib %s' % matplotlib.__version__,
             '# units_per_EM %d' % font.units_per_EM, '# ascender %d' % font.ascender, '# descender %d' % font.descender,
             '# cap_height %d' % cap, '# points %d' % points]
    for cp, a, contours in glyphs:
        lines.append('glyph %d %d %d' % (cp, a, len(contours)))
        lines += [' '.join('%d %d' % (int(x), int(y)) for x, y in c) for c in contours]
    return '\n'.join(lines) + '\n'


if __name__ == '__main__':
    with open(os.path.join(HERE, 'dejavu_sans.txt'), 'w') as f:
        f.write(generate())
