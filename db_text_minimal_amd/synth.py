"""Synthetic scene-text batches on the device: rendered words with polygon ground truth, the stand-in for the SynthText pre-training of
the DB paper when nothing can be downloaded (csrc/synth.hip; definition: DESIGN.md section 41).

  plan_synth_text(shapes, rng, ...)                                    host: per image a background plan and the placed words
  synth_records(shapes, plans)                                         host: instance records, tile bins, image descriptors of dbn_synth_text_u8
  render_synth_text(shapes, plans, device, backgrounds=None, out=None) device: the packed uint8 batch, one launch
  SynthTextBatches(batches, batch_size, shapes, seed, device, ...)     a loader source: (packed_device, shapes, polys, tags) per batch
  python -m db_text_minimal_amd.synth --out DIR --count 8 --size 640 --seed 0     img_<k>.png and gt_img_<k>.txt

A word is a run of glyph instances {image, glyph, a00, a01, a10, a11, tx, ty, colour}: the outline of DejaVu Sans (glyph_table) under an
integer matrix in lattice units (2^20 per pixel) per font unit, with the pen at the lattice point t.  The device fills it by the
non-zero winding rule of draw_labels at 16 samples per pixel and blends the colour by the coverage, over a
procedural background (three octaves of value noise from Philox4x32-10) or over the caller's text-free images.  Everything on the
device is exact integer arithmetic, so the bytes follow from the integer records alone; the planner works in float64 and rounds every
matrix entry and pen position to the lattice.

THIS PROJECT'S DEFINITION, PARITY UNPINNED by construction against SynthText or any renderer.  There is no host rendering path.
Out of scope: perspective, other fonts, non-Latin scripts, clutter and distractor shapes, text effects such as borders and shadows.
"""
import math
import os

import numpy as np
import torch

from ._lib import check, lib
from .packed import check_bytes, check_shape, cuda_device, flat_u8, image_offsets, on_device, upload
from .render import glyph_table

LATTICE = 1 << 20  # lattice units per pixel
TILE = 32          # a tile in pixels (SY_TILE of csrc/synth.hip)
MIN_HEIGHT, MAX_HEIGHT = 4.0, 256.0  # cap heights in pixels
MAX_POLYGON = 28   # points of a curved word's polygon, at most
STREAM = 0x7374    # second word of the seed of an image of SynthTextBatches
CHARSET = 'ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789'
_A_LIM, _T_LIM, _SPAN_LIM = 1 << 19, 1 << 35, 1 << 30
_REC, _DESC, _MAX_IMAGES, _MAX_SIDE = 9, 8, 65535, 16384
_FIRST, _LAST = 32, 126


# ---- host plan -----------------------------------------------------------------------------------------------------
def _pair(name, value, lo, hi, integer=False):
    try:
        a, b = value
        a, b = (int(a), int(b)) if integer else (float(a), float(b))
    except (TypeError, ValueError):
        raise ValueError('%s is a pair (min, max), got %r' % (name, value))
    if not lo <= a <= b <= hi:
        raise ValueError('%s range (%g, %g) is not an ascending pair inside [%g, %g]' % (name, a, b, lo, hi))
    return a, b


def _luma(c):
    return (299 * int(c[0]) + 587 * int(c[1]) + 114 * int(c[2])) / 1000.0


def _rot(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s], [s, c]])


def _segment_distance(c, a, b):
    """distance of the point c from the segment a b"""
    d = b - a
    t = min(1.0, max(0.0, float(np.dot(c - a, d)) / max(float(np.dot(d, d)), 1e-300)))
    return float(np.hypot(*(a + t * d - c)))


def instance_box(rec, box):
    """The transformed glyph box of an instance, relative to t, in exact integers: (x0, y0, x1, y1) on the lattice, or None when the
    instance is not evaluated (|a| >= 2^19, |t| > 2^35, a span >= 2^30).  rec: the nine fields; box: (xmin, ymin, xmax, ymax)."""
    a, t = [int(v) for v in rec[2:6]], [int(v) for v in rec[6:8]]
    xmin, ymin, xmax, ymax = (int(v) for v in box)
    if any(abs(v) >= _A_LIM for v in a) or any(abs(v) > _T_LIM for v in t):
        return None
    out = []
    for ax, ay in ((a[0], a[1]), (a[2], a[3])):
        out.append((min(ax * xmin, ax * xmax) + min(ay * ymin, ay * ymax), max(ax * xmin, ax * xmax) + max(ay * ymin, ay * ymax)))
    if out[0][1] - out[0][0] >= _SPAN_LIM or out[1][1] - out[1][0] >= _SPAN_LIM:
        return None
    return out[0][0], out[1][0], out[0][1], out[1][1]


def _draw_word(rng, f, cfg):
    """every attribute of one attempt, in a fixed order of draws -> a word about the origin (no position yet), or None"""
    if cfg['vocabulary'] is not None:
        text = cfg['vocabulary'][int(rng.randint(len(cfg['vocabulary'])))]
    else:
        n = int(rng.randint(cfg['length'][0], cfg['length'][1] + 1))
        text = ''.join(cfg['charset'][int(k)] for k in rng.randint(0, len(cfg['charset']), n))
    cap = math.exp(rng.uniform(math.log(cfg['height'][0]), math.log(cfg['height'][1])))
    theta, shear = math.radians(rng.uniform(*cfg['angle'])), float(rng.uniform(*cfg['shear']))
    sx, sy = float(rng.uniform(*cfg['aspect'])), float(rng.uniform(*cfg['aspect']))
    curved, arc = bool(rng.uniform() < cfg['curve_p']), math.radians(rng.uniform(-cfg['max_arc'], cfg['max_arc']))
    colours = rng.randint(0, 256, (8, 3))
    colour = next((c for c in colours if abs(_luma(c) - _luma(cfg['base'])) >= cfg['min_contrast']), None)
    if colour is None:
        colour = (0, 0, 0) if _luma(cfg['base']) >= 127.5 else (255, 255, 255)
    u = (float(rng.uniform()), float(rng.uniform()))  # the place inside the room the image leaves

    g = np.array([(ord(ch) if _FIRST <= ord(ch) <= _LAST else ord('?')) - _FIRST for ch in text], np.int64)
    index, adv = f['index_all'], f['advance']
    if not len(g) or not (index[g, 1] > 0).any():
        return None
    pen = np.cumsum(adv[g]) - adv[g]
    total = int(adv[g].sum())
    has = index[g, 1] > 0
    k = cap / f['cap_height']  # pixels per font unit
    m = cfg['pad'] * f['cap_height']
    y0, y1 = float(index[g[has], 3].min()) - m, float(index[g[has], 5].max()) + m
    x0 = min(-m, float((pen + index[g, 2])[has].min()))  # (an outline may overhang its advance: 'J' starts left of its pen)
    x1 = max(total + m, float((pen + index[g, 4])[has].max()))
    local = np.array([[1.0, -shear], [0.0, 1.0]]) @ np.diag([k * sx, -k * sy])  # font units (y up) -> the upright word's pixels (y down)
    mats, pens = [], []
    if curved:
        length, tall = k * sx * total, k * sy * (y1 - y0)
        arc = math.copysign(min(abs(arc), length / (2.0 * tall)), arc)  # the centre stays two band heights away
        if abs(arc) < math.radians(1.0):
            curved = False
    if not curved:
        A = _rot(theta) @ local
        mats = [A] * len(g)
        pens = [A @ np.array([float(p), 0.0]) for p in pen]
        poly = np.array([[x0, y1], [x1, y1], [x1, y0], [x0, y0]]) @ A.T  # top-left, top-right, bottom-right, bottom-left
    else:
        R = length / arc  # signed: R > 0 bends the ends down
        centre = _rot(theta) @ np.array([0.0, R])
        for gi, p in zip(g, pen):
            s = k * sx * (float(p) + adv[gi] / 2.0) - length / 2.0  # arc length of the glyph's baseline midpoint from the word's
            A = _rot(theta + s / R) @ local
            mid = _rot(theta) @ np.array([R * math.sin(s / R), R * (1.0 - math.cos(s / R))])
            mats.append(A)
            pens.append(mid - A @ np.array([adv[gi] / 2.0, 0.0]))
        # the band in polar coordinates about the centre that holds every glyph's padded box
        rho_lo, rho_hi, phis = math.inf, 0.0, []
        mid_dir = -centre / abs(R)
        for gi, A, t in zip(g[has], [a for a, h in zip(mats, has) if h], [t for t, h in zip(pens, has) if h]):
            bx0, bx1 = min(-m, float(index[gi, 2]) - m), max(adv[gi] + m, float(index[gi, 4]) + m)
            c = np.array([[bx0, y0], [bx1, y0], [bx1, y1], [bx0, y1]]) @ A.T + t
            for a, b in zip(c, np.roll(c, -1, 0)):
                rho_lo = min(rho_lo, _segment_distance(centre, a, b))
            d = c - centre
            rho_hi = max(rho_hi, float(np.hypot(d[:, 0], d[:, 1]).max()))
            # the angle from the word's middle, positive towards its end
            phis += [math.atan2(mid_dir[0] * q[1] - mid_dir[1] * q[0], float(np.dot(mid_dir, q))) * (1.0 if R > 0 else -1.0) for q in d]
        if rho_lo <= 0.0:
            return None
        K = min(max(2, -(-len(text) // 2)), MAX_POLYGON // 2 - 1)
        phi = np.linspace(min(phis), max(phis), K + 1)
        push = 1.0 / math.cos((phi[1] - phi[0]) / 2.0)  # the chords of the outer curve stay outside it (the sagitta)
        ang = math.atan2(mid_dir[1], mid_dir[0]) + phi * (1.0 if R > 0 else -1.0)
        ray = np.stack([np.cos(ang), np.sin(ang)], 1)
        outer, inner = centre + rho_hi * push * ray, centre + rho_lo * ray
        top, bottom = (outer, inner) if R > 0 else (inner, outer)  # R > 0: the centre lies below the baseline
        poly = np.concatenate([top, bottom[::-1]])
    return {'text': text, 'height': cap, 'curved': curved, 'colour': tuple(int(c) for c in colour), 'glyphs': g, 'mats': mats, 'pens': pens,
            'poly': poly, 'u': u}


def plan_synth_text(shapes, rng, words=(1, 8), vocabulary=None, charset=CHARSET, length=(1, 12), height=(8, 64), angle=(-30, 30),
                    shear=(-0.2, 0.2), aspect=(0.8, 1.25), curve_p=0.2, max_arc=120, min_contrast=64, tries=20, pad=0.08, ignore_below=0,
                    texture=(0, 24)):
    """Plans for images of `shapes` [(H, W)], drawn from `rng` (a np.random.RandomState): per image
      {'base': (r, g, b), 'amps': (A_0, A_1, A_2), 'seed': 64-bit int, 'words': [word]}, word =
      {'text', 'tag', 'height' (cap height in pixels), 'curved', 'colour': (r, g, b), 'polygon': fp64 [V, 2] in image coordinates,
       'instances': int64 [K, 7] of (glyph, a00, a01, a10, a11, tx, ty), one row per character that has an outline}.
    Per image: the word count from `words`, the base colour uniform, the three noise amplitudes from `texture` (grey levels, within
    0 .. 64), the seed from two randint(0, 2**32, dtype=uint32).  Per word, at most `tries` attempts with a fresh draw of every
    attribute: the text from `vocabulary` (a list of strings) or else `length` characters of `charset`; the cap height log-uniform in
    `height` (within 4 .. 256 px); `angle` in degrees; `shear`; a scale per axis from `aspect`; with probability `curve_p` a circular arc
    as the baseline, subtending at most `max_arc` degrees (and little enough that its centre stays two band heights away), each glyph
    placed rigidly with its baseline midpoint on the arc and the tangent there as its baseline; the colour redrawn up to 8 times until
    |luma(fg) - luma(base)| >= min_contrast (luma = (299 r + 587 g + 114 b) / 1000), then black or white, whichever is further
    from the base; the place uniform where the polygon lies inside the image.  An attempt is kept when the polygon's axis-aligned
    box grown by 2 px meets no earlier word's; a word that finds no place is dropped, as is one without an outlined glyph.
    The polygon of a straight word is the quad from -m to the advance + m and from the lowest glyph's ymin - m to the highest
    glyph's ymax + m, m = pad cap_height font units (widened to an outline that overhangs its advance), under the word's float64
    affine, in the order top-left, top-right, bottom-right, bottom-left of the word's own frame; of a curved word K + 1 points along the
    top and K + 1 back along the bottom of the ring sector that holds every glyph's padded box, K = max(2, ceil(len / 2)), at most 28
    points, the outer points pushed out by the chord's sagitta.  tag: the text, or '###' below `ignore_below` px of cap height.
    The contrast is against the plan's base colour: over the caller's `backgrounds` (render_synth_text) it is not checked.
    Raises ValueError for a range outside its bounds and for an instance the device would not evaluate (a span of 2^30 or more)."""
    f = glyph_table()
    cfg = {'words': _pair('words', words, 0, 1 << 16, True), 'length': _pair('length', length, 1, 256, True),
           'height': _pair('height', height, MIN_HEIGHT, MAX_HEIGHT), 'angle': _pair('angle', angle, -360.0, 360.0),
           'shear': _pair('shear', shear, -1.0, 1.0), 'aspect': _pair('aspect', aspect, 0.25, 4.0), 'texture': _pair('texture', texture, 0, 64, True),
           'curve_p': float(curve_p), 'max_arc': float(max_arc), 'min_contrast': float(min_contrast), 'pad': float(pad), 'vocabulary': None,
           'charset': str(charset)}
    if not 0 <= cfg['curve_p'] <= 1:
        raise ValueError('curve_p %g is not a probability' % cfg['curve_p'])
    if not 0 < cfg['max_arc'] <= 180:
        raise ValueError('max_arc %g outside (0, 180] degrees' % cfg['max_arc'])
    if not 0 <= cfg['pad'] <= 1:
        raise ValueError('pad %g outside [0, 1]' % cfg['pad'])
    if int(tries) < 1:
        raise ValueError('tries must be at least 1, got %r' % (tries, ))
    if vocabulary is not None:
        cfg['vocabulary'] = [str(w) for w in vocabulary]
        if not cfg['vocabulary']:
            raise ValueError('vocabulary is empty')
    elif not cfg['charset']:
        raise ValueError('charset is empty')
    plans = []
    for shape in shapes:
        H, W = check_shape(shape)
        count = int(rng.randint(cfg['words'][0], cfg['words'][1] + 1))
        base = tuple(int(c) for c in rng.randint(0, 256, 3))
        amps = tuple(int(a) for a in rng.randint(cfg['texture'][0], cfg['texture'][1] + 1, 3))
        low, high = int(rng.randint(0, 2**32, dtype=np.uint32)), int(rng.randint(0, 2**32, dtype=np.uint32))
        cfg['base'] = base
        placed, boxes = [], []
        for _ in range(count):
            for _ in range(int(tries)):
                w = _draw_word(rng, f, cfg)
                if w is None:
                    break  # no outline: not placed
                lo, hi = w['poly'].min(0), w['poly'].max(0)
                room = np.array([W, H], np.float64) - (hi - lo)
                if (room < 0).any():
                    continue
                origin = room * np.array(w['u']) - lo
                poly = w['poly'] + origin
                if poly.min() < 0 or poly[:, 0].max() > W or poly[:, 1].max() > H:  # (rounding at the far edge)
                    continue
                box = (poly[:, 0].min() - 2, poly[:, 1].min() - 2, poly[:, 0].max() + 2, poly[:, 1].max() + 2)
                if any(box[0] <= b[2] and b[0] <= box[2] and box[1] <= b[3] and b[1] <= box[3] for b in boxes):
                    continue
                has = f['index_all'][w['glyphs'], 1] > 0
                inst = np.array([[gi] + [int(v) for v in np.rint(A.reshape(-1) * LATTICE)] + [int(v) for v in np.rint((origin + t) * LATTICE)]
                                 for gi, A, t, h in zip(w['glyphs'], w['mats'], w['pens'], has) if h], np.int64).reshape(-1, 7)
                for row in inst:
                    if instance_box([0, 0] + row[1:].tolist(), f['index_all'][row[0], 2:]) is None:
                        raise ValueError('a glyph of %r at cap height %g has a matrix entry of 2^19 or more or spans 2^30 lattice units or more: the device would skip it'
                                         % (w['text'], w['height']))
                placed.append({'text': w['text'], 'tag': w['text'] if w['height'] >= ignore_below else '###', 'height': w['height'],
                               'curved': w['curved'], 'colour': w['colour'], 'polygon': poly, 'instances': inst})
                boxes.append(box)
                break
        plans.append({'base': base, 'amps': amps, 'seed': low | high << 32, 'words': placed})
    return plans


def tile_count(shapes):
    """the tiles of TILE x TILE pixels that images of `shapes` are cut into"""
    return int(sum(-(-int(h) // TILE) * -(-int(w) // TILE) for h, w in shapes))


def synth_records(shapes, plans):
    """What dbn_synth_text_u8 takes for packed images (include/dbnet_hip.h): (recs int64 [R, 9], bins int32 [B], desc int64 [N, 8]).
    recs: the instances of every word in plan order, images in order.  bins: per tile of TILE x TILE pixels {image, y0, x0, end}, then
    per tile the ascending records whose transformed glyph box holds a sample of the tile; an instance the device would not evaluate
    (instance_box) is in no list."""
    N = len(shapes)
    if not 1 <= N <= _MAX_IMAGES:
        raise ValueError('%d images: a batch holds 1 .. %d' % (N, _MAX_IMAGES))
    if len(plans) != N:
        raise ValueError('%d plans for %d images: one plan per image' % (len(plans), N))
    f = glyph_table()
    index = f['index_all']
    desc, rows, tiles = np.zeros((N, _DESC), np.int64), [], []
    off = tile = 0
    for n, (shape, plan) in enumerate(zip(shapes, plans)):
        H, W = int(shape[0]), int(shape[1])
        if not (1 <= H <= _MAX_SIDE and 1 <= W <= _MAX_SIDE):
            raise ValueError('image size %d x %d outside 1 .. %d' % (H, W, _MAX_SIDE))
        base, amps, seed = [int(c) for c in plan['base']], [int(a) for a in plan['amps']], int(plan['seed'])
        if len(base) != 3 or not all(0 <= c <= 255 for c in base):
            raise ValueError('plan %d: the base colour is three bytes, not %r' % (n, plan['base']))
        if len(amps) != 3 or not all(0 <= a <= 64 for a in amps):
            raise ValueError('plan %d: three amplitudes in 0 .. 64, not %r' % (n, plan['amps']))
        if not 0 <= seed < 1 << 64:
            raise ValueError('plan %d: the seed is a 64-bit number, not %d' % (n, seed))
        desc[n, :7] = (off, H, W, tile, base[0] | base[1] << 8 | base[2] << 16, amps[0] | amps[1] << 8 | amps[2] << 16,
                       np.uint64(seed).astype(np.int64))
        for w in plan['words']:
            c = [int(v) for v in w['colour']]
            if len(c) != 3 or not all(0 <= v <= 255 for v in c):
                raise ValueError('plan %d: a colour is three bytes, not %r' % (n, w['colour']))
            inst = np.asarray(w['instances'], np.int64).reshape(-1, 7)
            if len(inst) and not ((inst[:, 0] >= 0) & (inst[:, 0] < len(index))).all():
                raise ValueError('plan %d: a glyph outside 0 .. %d' % (n, len(index) - 1))
            r = np.empty((len(inst), _REC), np.int64)
            r[:, 0], r[:, 1:8], r[:, 8] = n, inst, c[0] | c[1] << 8 | c[2] << 16
            rows.append(r)
        ty, tx = np.meshgrid(np.arange(0, H, TILE, dtype=np.int64), np.arange(0, W, TILE, dtype=np.int64), indexing='ij')
        tiles.append(np.stack([np.full(ty.size, n, np.int64), ty.reshape(-1), tx.reshape(-1)], 1))
        off += 3 * H * W
        tile += ty.size
    recs = np.concatenate(rows) if rows else np.zeros((0, _REC), np.int64)
    tiles = np.concatenate(tiles)
    T = len(tiles)
    pairs = np.zeros((0, 2), np.int64)
    if len(recs):
        # the box on the lattice (the products stay below 2^63 for any evaluated instance; the others are masked out before use)
        a, t, box = recs[:, 2:6], recs[:, 6:8], index[recs[:, 1], 2:6].astype(np.int64)
        ok = (np.abs(a) < _A_LIM).all(1) & (np.abs(t) <= _T_LIM).all(1) & (index[recs[:, 1], 1] > 0)
        a = np.where(ok[:, None], a, 0)
        lo, hi = np.empty((len(recs), 2), np.int64), np.empty((len(recs), 2), np.int64)
        for axis in range(2):
            px, qx = a[:, 2 * axis] * box[:, 0], a[:, 2 * axis] * box[:, 2]
            py, qy = a[:, 2 * axis + 1] * box[:, 1], a[:, 2 * axis + 1] * box[:, 3]
            lo[:, axis] = np.minimum(px, qx) + np.minimum(py, qy)
            hi[:, axis] = np.maximum(px, qx) + np.maximum(py, qy)
        ok &= ((hi - lo) < _SPAN_LIM).all(1)
        t = np.where(ok[:, None], t, 0)
        # pixels with a sample inside: lo <= L p + (2 i + 1) L / 8 - t <= hi for some i in 0 .. 3
        p0 = -((-(lo + t - 7 * LATTICE // 8)) // LATTICE)
        p1 = (hi + t - LATTICE // 8) // LATTICE
        hw = desc[recs[:, 0], 1:3][:, ::-1]  # (W, H) per record
        p0, p1 = np.maximum(p0, 0), np.minimum(p1, hw - 1)
        ok &= (p0 <= p1).all(1)
        c0, c1 = p0 // TILE, p1 // TILE
        across = -(-desc[:, 2] // TILE)
        chunks = []
        for r in np.flatnonzero(ok):
            n = recs[r, 0]
            yy, xx = np.meshgrid(np.arange(c0[r, 1], c1[r, 1] + 1), np.arange(c0[r, 0], c1[r, 0] + 1), indexing='ij')
            chunks.append(np.stack([(desc[n, 3] + yy * across[n] + xx).reshape(-1), np.full(yy.size, r, np.int64)], 1))
        if chunks:
            pairs = np.concatenate(chunks)
            pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]
    if 4 * T + len(pairs) > 0x7FFFFFFF:
        raise ValueError('%d tiles and %d bin entries are too many for one call' % (T, len(pairs)))
    ends = 4 * T + np.cumsum(np.bincount(pairs[:, 0], minlength=T))
    bins = np.concatenate([np.concatenate([tiles, ends[:, None]], 1).reshape(-1), pairs[:, 1]]).astype(np.int32)
    return recs, bins, desc


# ---- device --------------------------------------------------------------------------------------------------------
_font_dev = {}


def _font_on(dev):
    if dev not in _font_dev:
        f = glyph_table()
        _font_dev[dev] = (upload(f['edges_all'], dev), upload(f['index_all'], dev))
    return _font_dev[dev]


def render_synth_text(shapes, plans, device=None, backgrounds=None, out=None):
    """The packed uint8 RGB batch (image_collate's layout) of images of `shapes` after their plans (plan_synth_text), on `device`: the
    background, then every word's glyphs in plan order, anti-aliased.  One launch for the whole batch on the current stream, no host
    sync.  backgrounds: a packed uint8 device batch of the same shapes (text-free images of the caller's), read instead of the
    procedural background; the planner's colour contrast is then not checked against anything.  out=None allocates; an `out` that
    overlaps `backgrounds` is refused."""
    shapes = [(int(h), int(w)) for h, w in shapes]
    recs, bins, desc = synth_records(shapes, plans)
    need = int(image_offsets(shapes)[-1])
    like = out if out is not None else backgrounds
    dev = cuda_device('render_synth_text', device, like)
    src = None
    if backgrounds is not None:
        src = flat_u8(backgrounds, what='backgrounds')
        check_bytes(src.numel(), need, 'backgrounds holds')
        if src.device != dev:
            raise ValueError('backgrounds must be on %s' % (dev, ))
    dst = torch.empty(need, dtype=torch.uint8, device=dev) if out is None else flat_u8(out, what='out')
    if dst.numel() != need or dst.device != dev:
        raise ValueError('out must hold %d bytes on %s' % (need, dev))
    if src is not None:
        a, b = src.data_ptr(), dst.data_ptr()
        if a < b + need and b < a + need:
            raise ValueError('out must not overlap backgrounds')
    f = glyph_table()
    with on_device(dev) as stream:
        fe, fg = _font_on(dev)
        d, r, b = upload(desc, dev), upload(recs, dev) if len(recs) else None, upload(bins, dev)
        check(lib().dbn_synth_text_u8(src.data_ptr() if src is not None else None, dst.data_ptr(), need, desc.ctypes.data, d.data_ptr(), len(shapes),
                                      recs.ctypes.data if len(recs) else None, r.data_ptr() if r is not None else None, len(recs), bins.ctypes.data,
                                      b.data_ptr(), tile_count(shapes), len(bins), fe.data_ptr(),
                                      len(f['edges_all']), f['index_all'].ctypes.data, fg.data_ptr(), len(f['index_all']), stream), 'synth_text_u8')
    return dst


class SynthTextBatches:
    """A loader source of synthetic scene text: an iterable of `batches` batches of `batch_size` images, each
    (packed uint8 device tensor, shapes, polys, tags) in image_collate's layout, so DeviceBatches(SynthTextBatches(...), 'cuda',
    training=True), fit and evaluate consume it as they are.  shapes: one (H, W) or a list to draw from per image.  Image i of batch b
    is planned from np.random.RandomState([seed, 0x7374, b, i]) (its shape first, when there is a choice), so it depends neither on
    its neighbours nor on the batch size, and every pass gives the same batches.  plan_kwargs go to plan_synth_text."""

    def __init__(self, batches, batch_size, shapes=(640, 640), seed=0, device='cuda', **plan_kwargs):
        self.batches, self.batch_size, self.seed = int(batches), int(batch_size), int(seed)
        if self.batches < 0 or self.batch_size < 1:
            raise ValueError('batches >= 0 and batch_size >= 1, got %r and %r' % (batches, batch_size))
        if not 0 <= self.seed < 1 << 32:
            raise ValueError('seed is a 32-bit number, got %r' % (seed, ))
        one = len(shapes) == 2 and not isinstance(shapes[0], (tuple, list))
        self.shapes = [check_shape(s) for s in ([shapes] if one else shapes)]
        if not self.shapes:
            raise ValueError('shapes is empty')
        self.device = torch.device(device)
        self.plan_kwargs = plan_kwargs
        plan_synth_text([], np.random.RandomState(0), **plan_kwargs)  # (a bad range or key raises here, not in the first batch)

    def __len__(self):
        return self.batches

    def plan(self, b):
        """(shapes, plans) of batch b: host only"""
        shapes, plans = [], []
        for i in range(self.batch_size):
            rng = np.random.RandomState([self.seed, STREAM, b, i])
            shape = self.shapes[int(rng.randint(len(self.shapes)))] if len(self.shapes) > 1 else self.shapes[0]
            shapes.append(shape)
            plans.append(plan_synth_text([shape], rng, **self.plan_kwargs)[0])
        return shapes, plans

    def __iter__(self):
        for b in range(self.batches):
            shapes, plans = self.plan(b)
            packed = render_synth_text(shapes, plans, self.device)
            yield packed, shapes, [[w['polygon'] for w in p['words']] for p in plans], [[w['tag'] for w in p['words']] for p in plans]


def main(argv=None):
    import argparse
    from .png import save_pngs
    ap = argparse.ArgumentParser(description='write synthetic scene-text images and their polygon ground truth')
    ap.add_argument('--out', required=True)
    ap.add_argument('--count', type=int, default=8)
    ap.add_argument('--size', type=int, default=640)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args(argv)
    os.makedirs(args.out, exist_ok=True)
    batch = 16
    source = SynthTextBatches(-(-args.count // batch), batch, (args.size, args.size), args.seed)  # (CHARSET has no comma)
    k = 0
    for packed, shapes, polys, tags in source:
        keep = min(batch, args.count - k)
        keep_bytes = int(image_offsets(shapes[:keep])[-1])
        save_pngs([os.path.join(args.out, 'img_%d.png' % (k + i)) for i in range(keep)], packed[:keep_bytes], shapes[:keep])
        for i in range(keep):
            with open(os.path.join(args.out, 'gt_img_%d.txt' % (k + i)), 'w') as fh:
                for poly, tag in zip(polys[i], tags[i]):
                    fh.write(','.join('%d' % int(round(v)) for v in np.asarray(poly).reshape(-1)) + ',' + tag + '\n')
        k += keep
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
