"""Showing a detection result on the device: the last step of the reference's inference path.  test.py, test_ocr.py and
test_webcam.py end in utils.draw_bbox (cv2.polylines of every box on a copy of the original image, utils.py:202-212), and
test.py lays the probability map, resized to the original image with cv2.resize and coloured by a matplotlib colormap,
over it at alpha = 0.6 (utils.visualize_polygon :252-283, utils.visualize_heatmap :215-228).

  draw_outlines(images, shapes_per_image, color, thickness)   utils.draw_bbox for a batch: one copy, one launch
  overlay_heatmap(images, prob, valid_hw, cmap, alpha, ...)    the resized, coloured, blended map: one launch, plus one
                                                              reduction launch when the colour limits are autoscaled
  render_detections(images, prob, shapes, ...)                both, in the reference's order (outlines, then the map)
  draw_labels(images, labels_per_image, color, height, ...)   the cv2.putText step of test_ocr.py:197-210: one launch
  draw_words / draw_scores / draw_dots / text_size            recognised strings with anchor dots; scores; the label's box
  minmax_scale_u8(x)                                          utils.minmax_scaler_img (:110-113) of fp32 [N, 3, H, W]
  image_views(packed, shapes)                                 per-image [H, W, 3] views of a packed result

Images are (packed uint8, shapes) as image_collate gives them, on the host or the device, or one uint8 [H, W, 3] tensor;
results are packed uint8 on the device in the same layout.  The input images are never written.  Everything runs on the
current stream without a host synchronisation (csrc/render.hip).

Strokes.  thickness 1 paints cv2's LINE_8 pixels (LineIterator, restated as dbn_on_line in csrc/fillpoly.h): the border
fillPoly draws here.  THICK STROKES (thickness >= 2) ARE THIS PROJECT'S DEFINITION, not OpenCV's ThickLine: a pixel is
painted iff its distance d to the closed segment satisfies 4 d^2 <= thickness^2, decided exactly in integers; joins and
caps are round, and pixels on the rim of a stroke may differ from cv2's.

Heat map, per pixel: v = cv2.resize(prob[:vh, :vw], (W, H)) INTER_LINEAR on float data (PARITY UNPINNED against cv2, like
every resize here); t = matplotlib.colors.Normalize(vmin, vmax)(v) as numpy evaluates it for a float32 array (the
subtraction and the division in double, each stored as float32); index = Colormap.__call__'s (t * 256 in float32, 256 ->
255, truncated, clipped); colour = the colormap's byte table (cmaps/*.txt, pinned against matplotlib); out = rint(img *
(1 - a) + colour * a) in fp32, half to even.  The blend stands for matplotlib's Agg compositing of two imshow layers at
figure resolution (the reference saves a 200-dpi figure), which is not reproducible pixel for pixel: UNPINNED.  The map
must be finite.  DESIGN section 21.

Labels.  LABEL TEXT IS THIS PROJECT'S DEFINITION, not cv2.putText's Hershey strokes (neither cv2 nor the Hershey table is
available here): the outlines of DejaVu Sans (fonts/dejavu_sans.txt, generated from the font matplotlib bundles by
fonts/make_glyphs.py), filled by the non-zero winding rule at pixel centres in exact integers; a pixel is on or off.
PARITY UNPINNED against cv2 by construction; pinned against matplotlib's own containment test on the CPU.  DESIGN section 29.

  python -m db_text_minimal_amd.render --image X --model_path M [--is_output_polygon] [--heatmap] [--scores] [--out Y]
"""
import os

import numpy as np
import torch

from ._lib import check, lib
from .packed import as_images, check_bytes, check_shape, cuda_device, image_offsets, image_table, on_device, packed_on, upload
from .packed import offsets as _offsets

CMAPS = ('inferno', 'jet')
_VERT_MAX = 2 ** 20  # |vertex coordinate| of a shape (csrc/render.hip)
_INT_MAX = 2 ** 31 - 1
_EDGE, _IDESC, _PDESC, _COEF = 5, 3, 5, 4
_GEDGE, _GLYPH, _REC = 4, 6, 5  # int32 per edge, glyph and glyph instance of dbn_draw_glyphs
_FIRST, _LAST, _LABEL_MAX, _GLYPH_EDGES = 32, 126, 256, 512
_LATTICE = 64 * 2048  # label coordinates are 1 / _LATTICE pixel
LAUNCH_LOG = []  # the C entry points called, in order (tests clear it and read it back)
_tables = {}
_font, _font_dev = {}, {}


def colormap_table(name):
    """the 256 x 3 uint8 table of a shipped colormap ('inferno', 'jet'): matplotlib's (lut * 255).astype(uint8)"""
    if name not in CMAPS:
        raise ValueError('cmap must be one of %s, got %r' % (CMAPS, name))
    if name not in _tables:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'cmaps', name + '.txt')
        t = np.array([[int(v) for v in line.split()] for line in open(path) if line.strip()], np.int64)
        if t.shape != (256, 3) or t.min() < 0 or t.max() > 255:
            raise ValueError('%s is not a 256 x 3 byte table' % path)
        _tables[name] = t.astype(np.uint8)
    return _tables[name]


def _call(name, dev, *args):
    """the C entry point `name` on the current stream of `dev`, its handle the last argument"""
    LAUNCH_LOG.append(name)
    with on_device(dev) as st:
        check(getattr(lib(), name)(*args, st), name)


def image_views(packed, shapes):
    """per-image uint8 [H, W, 3] views of a packed result"""
    shapes = [check_shape(s) for s in shapes]
    off = image_offsets(shapes)
    check_bytes(packed.numel(), int(off[-1]), 'the packed images hold', packed.dim() == 1)
    return [packed[int(off[n]):int(off[n + 1])].view(h, w, 3) for n, (h, w) in enumerate(shapes)]


# ---- outlines --------------------------------------------------------------------------------------------------------
def _is_pair(e):
    return isinstance(e, tuple) and len(e) == 2


def _shapes_of_image(entry, n):
    """one image's shapes -> list of int64 [P, 2] arrays (or [K, P, 2] blocks), those with a coordinate sum <= 0 dropped
    (utils.py:243-248, test_ocr.py:144-151)"""
    if _is_pair(entry):  # (boxes, scores) of detect_boxes / (polygons, scores) of detect_polygons
        entry = entry[0]
    if isinstance(entry, np.ndarray) and entry.ndim == 3:  # K shapes of P vertices each, kept as one block
        if entry.shape[0] == 0:
            return []
        if entry.shape[2] != 2 or entry.shape[1] < 1 or entry.dtype.kind not in 'iu':
            raise ValueError('shapes of image %d must be an integer [K, P, 2] array with P >= 1, got %s %s' % (n, entry.dtype, entry.shape))
        b = entry.astype(np.int64)
        b = b[b.reshape(len(b), -1).sum(1) > 0]
        if len(b) and np.abs(b).max() > _VERT_MAX:
            raise ValueError('a vertex of image %d lies outside +-%d' % (n, _VERT_MAX))
        return [b] if len(b) else []
    elif isinstance(entry, np.ndarray) and entry.size == 0:
        polys = []
    elif isinstance(entry, (list, tuple)):
        polys = list(entry)
    else:
        raise ValueError('shapes of image %d must be a [K, P, 2] array or a list of [P, 2] polygons' % n)
    out = []
    for p in polys:
        p = np.asarray(p)
        if p.ndim != 2 or p.shape[1] != 2 or p.shape[0] < 1 or p.dtype.kind not in 'iu':
            raise ValueError('a shape of image %d must be an integer [P, 2] array with P >= 1, got %s %s' % (n, p.dtype, p.shape))
        p = p.astype(np.int64)
        if p.sum() <= 0:
            continue
        if np.abs(p).max() > _VERT_MAX:
            raise ValueError('a vertex of image %d lies outside +-%d' % (n, _VERT_MAX))
        out.append(p)
    return out


def _per_image(shapes_per_image, N):
    s = shapes_per_image
    if N == 1 and (_is_pair(s) or (isinstance(s, np.ndarray) and s.ndim == 3)
                   or (isinstance(s, list) and len(s) > 0 and all(isinstance(p, np.ndarray) and p.ndim == 2 for p in s))):
        s = [s]
    if not isinstance(s, (list, tuple)) or len(s) != N:
        raise ValueError('shapes for %s images, but %d images' % (len(s) if isinstance(s, (list, tuple)) else '?', N))
    return [_shapes_of_image(e, n) for n, e in enumerate(s)]


def stroke_edges(shapes_per_image, N):
    """-> int32 [E, 5] of (image, xa, ya, xb, yb): every shape closed (cv2.polylines isClosed=True), edge i from vertex
    i - 1 (the last one for i = 0) to vertex i; a single point is one zero-length edge."""
    rows = []
    for n, polys in enumerate(_per_image(shapes_per_image, N)):
        for p in polys:
            p = p if p.ndim == 3 else p[None]
            a = np.roll(p, 1, 1) if p.shape[1] > 1 else p
            rows.append(np.concatenate([np.full((p.shape[0] * p.shape[1], 1), n, np.int64), a.reshape(-1, 2), p.reshape(-1, 2)], 1))
    if not rows:
        return np.zeros((0, _EDGE), np.int32)
    return np.concatenate(rows).astype(np.int32)


def _color(color):
    try:
        c = [int(v) for v in color]
    except (TypeError, ValueError):
        raise ValueError('color must be three bytes, got %r' % (color, ))
    if len(c) != 3 or min(c) < 0 or max(c) > 255 or any(float(v) != int(v) for v in color):
        raise ValueError('color must be three bytes, got %r' % (color, ))
    return c


def draw_outlines(images, shapes_per_image, color=(255, 0, 0), thickness=3, device=None):
    """utils.draw_bbox for a batch: cv2.polylines(img.copy(), [pts], True, color, thickness) of every shape of every image.

    shapes_per_image: per image the int16 [K, 4, 2] boxes of detect_boxes(..., dest_sizes=...) (or its (boxes, scores)
    pair), or the list of int64 [P, 2] polygons of detect_polygons (or its pair); for a single image also that entry
    itself.  Shapes whose coordinate sum is <= 0 are dropped, as the reference drops them.  Vertices may lie outside the
    image (within +-2^20); only pixels inside it are written.  color: three bytes in the image's channel order;
    1 <= thickness <= 255.  thickness 1 is cv2's LINE_8 line; thickness >= 2 is this project's own stroke (every pixel
    within thickness / 2 of the segment, exactly; round joins and caps): pixels on the rim may differ from cv2's.
    Returns the packed uint8 device copy with the outlines (image_views splits it).  One copy and one launch on the
    current stream."""
    packed, shapes = as_images(images)
    c = _color(color)
    if isinstance(thickness, bool) or int(thickness) != thickness or not 1 <= int(thickness) <= 255:
        raise ValueError('thickness must be an integer in 1 .. 255, got %r' % (thickness, ))
    edges = stroke_edges(shapes_per_image, len(shapes))
    if -(-len(edges) // 4) > _INT_MAX:
        raise ValueError('%d edges are too many for one call' % len(edges))
    dev = cuda_device('rendering', device, packed)
    src = packed_on(packed, shapes, dev)
    out = torch.empty_like(src)
    if src.numel() == 0:
        return out
    d = image_table(shapes, dev)
    e = upload(edges, dev) if len(edges) else None
    _call('dbn_draw_strokes', dev, src.data_ptr(), out.data_ptr(), src.numel(), d.data_ptr(), len(shapes), e.data_ptr() if e is not None else None,
          len(edges), int(thickness), c[0], c[1], c[2])
    return out


# ---- heat map --------------------------------------------------------------------------------------------------------
def _limits(v, N, what):
    a = np.asarray(v, np.float64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, N)
    if a.size != N or not np.isfinite(a).all():
        raise ValueError('%s must be one finite number or one per image' % what)
    return a


def overlay_plan(shapes, map_hw, valid_hw=None, vmin=None, vmax=None):
    """host: the descriptors of the heat-map launches: (desc int64 [N, 5], coef fp64 [N, 4], autoscale)"""
    N = len(shapes)
    Hm, Wm = map_hw
    if valid_hw is None:
        valid_hw = [(Hm, Wm)] * N
    if len(valid_hw) != N:
        raise ValueError('%d valid_hw for %d images' % (len(valid_hw), N))
    if (vmin is None) != (vmax is None):
        raise ValueError('give both vmin and vmax, or neither (the limits of the resized map)')
    auto = vmin is None
    lo, hi = (np.zeros(N), np.zeros(N)) if auto else (_limits(vmin, N, 'vmin'), _limits(vmax, N, 'vmax'))
    if (lo > hi).any():
        raise ValueError('vmin must be less than or equal to vmax')
    first = _offsets([h * w for h, w in shapes])
    desc = np.zeros((N, _PDESC), np.int64)
    coef = np.zeros((N, _COEF), np.float64)
    for n, ((H, W), vhw) in enumerate(zip(shapes, valid_hw)):
        vh, vw = int(vhw[0]), int(vhw[1])
        if not (1 <= vh <= Hm and 1 <= vw <= Wm):
            raise ValueError('valid_hw %d x %d of image %d outside the %d x %d map' % (vh, vw, n, Hm, Wm))
        desc[n] = first[n], H, W, vh, vw
        coef[n] = 1. / (float(W) / vw), 1. / (float(H) / vh), lo[n], hi[n]  # cv2.resize: scale = 1. / ((double)dst / src)
    return desc, coef, auto


def overlay_heatmap(images, prob, valid_hw=None, cmap='inferno', alpha=0.6, vmin=None, vmax=None, binary=None, out=None):
    """The heat map of utils.visualize_polygon (:253, :274-275) over a batch: per image the probability map, resized to
    the image (cv2.resize, INTER_LINEAR on float data), normalised, coloured and blended over it at `alpha`.

    prob: fp32 device tensor [N, H', W'] or [N, C, H', W'] (channel 0), the model's output for these N images;
    valid_hw[n] = (rows, columns) of it that belong to image n (default the whole map; `out_hw` of the letterbox plan for
    padded batches).  vmin / vmax: both None = the minimum and maximum of each image's RESIZED map (what plt.imshow
    autoscales to; found on the device by one more launch), else numbers (one, or one per image); a constant map paints
    table entry 0, as matplotlib does.  cmap: 'inferno' or 'jet'.  0 <= alpha <= 1.  binary=thresh: the map is first set
    to 1 where prob > thresh and 0 elsewhere (utils.visualize_heatmap :217-218, with cmap='jet' there).  out: a packed
    uint8 device buffer that already holds the picture to paint over, e.g. the result of draw_outlines: it is painted in
    place and returned, and `images` then only gives the shapes.  Without it the images are read, never written, and a
    new packed buffer is returned.  The blend stands for matplotlib's compositing at figure resolution: unpinned."""
    packed, shapes = as_images(images)
    N = len(shapes)
    if not (isinstance(prob, torch.Tensor) and prob.is_cuda and prob.dtype == torch.float32 and prob.dim() in (3, 4)):
        raise ValueError('prob must be a float32 device tensor [N, H, W] or [N, C, H, W]')
    if prob.shape[0] != N:
        raise ValueError('prob holds %d maps, but %d images' % (prob.shape[0], N))
    a = float(alpha)
    if not 0.0 <= a <= 1.0:
        raise ValueError('alpha must lie in 0 .. 1, got %r' % (alpha, ))
    table = colormap_table(cmap)
    Hm, Wm = int(prob.shape[-2]), int(prob.shape[-1])
    desc, coef, auto = overlay_plan(shapes, (Hm, Wm), valid_hw, vmin, vmax)
    dev = prob.device
    if out is not None:
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == dev and out.dtype == torch.uint8 and out.dim() == 1
                and out.is_contiguous() and out.numel() == packed.numel()):
            raise ValueError('out must be a packed uint8 tensor of %d bytes on %s' % (packed.numel(), dev))
        src = out
    else:
        src = packed_on(packed, shapes, dev)
        out = torch.empty_like(src)
    n_px = src.numel() // 3
    if -(-n_px // 1024) > _INT_MAX:
        raise ValueError('%d pixels are too many for one call' % n_px)
    if n_px == 0:
        return out
    prob = prob.contiguous()
    img_stride = prob.numel() // N
    d, c = upload(desc, dev), upload(coef, dev)
    lut = upload((table[:, 0].astype(np.int64) | table[:, 1].astype(np.int64) << 8 | table[:, 2].astype(np.int64) << 16).astype(np.int32), dev)
    is_bin, thresh = (0, 0.0) if binary is None else (1, float(binary))
    common = (d.data_ptr(), c.data_ptr(), N, n_px, prob.data_ptr(), prob.numel(), img_stride, Wm, is_bin, thresh)
    mm = None
    if auto:
        mm = torch.empty(2 * N, device=dev, dtype=torch.int32)
        _call('dbn_render_minmax', dev, *common, mm.data_ptr())
    _call('dbn_render_paint', dev, src.data_ptr(), out.data_ptr(), *common, mm.data_ptr() if auto else None, lut.data_ptr(), a)
    return out


# ---- labels ----------------------------------------------------------------------------------------------------------
def glyph_table():
    """the shipped font (fonts/dejavu_sans.txt, written by fonts/make_glyphs.py): a dict of `units_per_EM`, `ascender`,
    `descender`, `cap_height`, `first` (code point of glyph 0), `advance` (int64 [G]), `contours` (per glyph a list of
    int64 [P, 2] closed polylines in font units), and what the kernel takes: `edges` (int32 [E, 4] of ax, ay, bx, by;
    every contour closed, horizontal edges left out: the winding rule never counts them) and `index` (int32 [G, 6] of
    first edge, edges, xmin, ymin, xmax, ymax); `edges_all` and `index_all` are the same with EVERY edge of the closed
    contours, for a glyph under a rotation, where an edge that is horizontal in font units counts (synth.py)"""
    if _font:
        return _font
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'fonts', 'dejavu_sans.txt')
    head, adv, contours, want = {}, [], [], 0
    for line in open(path):
        f = line.split()
        if not f:
            continue
        if f[0] == '#':
            if len(f) == 3 and f[1] in ('units_per_EM', 'ascender', 'descender', 'cap_height'):
                head[f[1]] = int(f[2])
        elif f[0] == 'glyph':
            if want or int(f[1]) != _FIRST + len(adv):
                raise ValueError('%s: glyph %s out of order' % (path, f[1]))
            adv.append(int(f[2]))
            contours.append([])
            want = int(f[3])
        else:
            v = np.array([int(t) for t in f], np.int64)
            if not want or len(v) % 2 or len(v) < 6:
                raise ValueError('%s: a stray contour line' % path)
            contours[-1].append(v.reshape(-1, 2))
            want -= 1
    if len(adv) != _LAST - _FIRST + 1 or want or len(head) != 4:
        raise ValueError('%s is not the table of code points %d .. %d' % (path, _FIRST, _LAST))
    edges, index, every = [], np.zeros((len(adv), _GLYPH), np.int32), []
    for g, cs in enumerate(contours):
        first = sum(len(e) for e in edges)
        for c in cs:
            e = np.concatenate([c, np.roll(c, -1, 0)], 1)
            edges.append(e[e[:, 1] != e[:, 3]])
            every.append(e)
        if cs:
            p = np.concatenate(cs)
            index[g] = first, sum(len(e) for e in edges) - first, p[:, 0].min(), p[:, 1].min(), p[:, 0].max(), p[:, 1].max()
    if index[:, 1].max() > _GLYPH_EDGES:
        raise ValueError('%s: a glyph of more than %d edges' % (path, _GLYPH_EDGES))
    index_all = index.copy()
    index_all[:, 1] = [sum(len(c) for c in cs) for cs in contours]
    index_all[:, 0] = np.cumsum(index_all[:, 1]) - index_all[:, 1]
    index_all[index_all[:, 1] == 0, 0] = 0
    _font.update(head, first=_FIRST, advance=np.array(adv, np.int64), contours=contours, edges=np.concatenate(edges).astype(np.int32), index=index,
                 edges_all=np.concatenate(every).astype(np.int32), index_all=index_all)
    return _font


def _font_on(dev):
    if dev not in _font_dev:
        f = glyph_table()
        _font_dev[dev] = (upload(f['edges'], dev), upload(f['index'], dev))
    return _font_dev[dev]


def _size64(height):
    """the em size in 1/64 pixel of a cap height in pixels: rint(height * 64 * units_per_EM / cap_height)"""
    try:
        h = float(height)
    except (TypeError, ValueError):
        raise ValueError('height must be a number in 4 .. 512, got %r' % (height, ))
    if isinstance(height, bool) or not 4.0 <= h <= 512.0:
        raise ValueError('height (the cap height in pixels) must lie in 4 .. 512, got %r' % (height, ))
    f = glyph_table()
    return int(np.rint(h * 64 * f['units_per_EM'] / f['cap_height']))


def _glyphs_of(text):
    if not isinstance(text, str):
        raise ValueError('a label\'s text must be a str, got %r' % (text, ))
    if len(text) > _LABEL_MAX:
        raise ValueError('a label holds at most %d characters, got %d' % (_LABEL_MAX, len(text)))
    return [(ord(ch) if _FIRST <= ord(ch) <= _LAST else ord('?')) - _FIRST for ch in text]


def _ceil_px(v, size64):
    return -((-int(v) * size64) // _LATTICE)


def text_size(text, height=16):
    """(width, ascent, descent) of a label in whole pixels, rounded up, as cv2.getTextSize gives its box: the advances of
    the characters, the font's ascender above the baseline and its descender below it, at cap height `height`.  Host only."""
    s, f = _size64(height), glyph_table()
    return _ceil_px(f['advance'][_glyphs_of(text)].sum(), s), _ceil_px(f['ascender'], s), _ceil_px(-f['descender'], s)


def _labels_of(labels_per_image, N):
    ls = labels_per_image
    if N == 1 and isinstance(ls, (list, tuple)) and len(ls) > 0 and isinstance(ls[0], (list, tuple)) and len(ls[0]) == 2 and isinstance(ls[0][0], str):
        ls = [ls]
    if not isinstance(ls, (list, tuple)) or len(ls) != N:
        raise ValueError('labels for %s images, but %d images' % (len(ls) if isinstance(ls, (list, tuple)) else '?', N))
    out = []
    for n, entry in enumerate(ls):
        rows = []
        for lab in entry:
            try:
                text, (x, y) = lab
                ok = int(x) == x and int(y) == y and abs(int(x)) <= _VERT_MAX and abs(int(y)) <= _VERT_MAX
            except (TypeError, ValueError):
                raise ValueError('a label of image %d must be (text, (x, y)), got %r' % (n, lab))
            if not ok:
                raise ValueError('the origin of a label of image %d must be integers within +-%d, got %r' % (n, _VERT_MAX, (x, y)))
            if not isinstance(text, str) or len(text) > _LABEL_MAX:
                _glyphs_of(text)  # raises
            rows.append((text, int(x), int(y)))
        out.append(rows)
    return out


def label_records(labels_per_image, N):
    """-> int32 [R, 5] of (image, glyph, pen, x, y): one row per character that has an outline, the pen of character k
    the sum of the advances before it (font units)"""
    f = glyph_table()
    flat = [(n, ) + lab for n, labs in enumerate(_labels_of(labels_per_image, N)) for lab in labs if lab[0]]
    if not flat:
        return np.zeros((0, _REC), np.int32)
    lens = np.array([len(lab[1]) for lab in flat], np.int64)
    codes = np.frombuffer(''.join(lab[1] for lab in flat).encode('utf-32-le', 'surrogatepass'), np.uint32).astype(np.int64)
    g = np.where((codes >= _FIRST) & (codes <= _LAST), codes, ord('?')) - _FIRST
    adv = f['advance'][g]
    before = np.cumsum(adv) - adv  # the advances before each character in the whole run; minus those before its label's first
    pen = before - np.repeat(before[np.cumsum(lens) - lens], lens)
    nxy = np.repeat(np.array([(lab[0], lab[2], lab[3]) for lab in flat], np.int64), lens, 0)
    recs = np.stack([nxy[:, 0], g, pen, nxy[:, 1], nxy[:, 2]], 1)
    return recs[f['index'][g, 1] > 0].astype(np.int32)


def label_backgrounds(labels_per_image, N, size64):
    """the rectangles behind the labels, as a font of their own: (edges int32 [2 B, 4], index int32 [B, 6], records
    int32 [B, 5]), one four-point contour per label (its two horizontal edges left out) from -m to the label's advance
    + m and from descender - m to ascender + m, m = a 2-pixel margin rounded up to whole font units at this size"""
    f = glyph_table()
    m = -((-2 * _LATTICE) // size64)
    y0, y1 = f['descender'] - m, f['ascender'] + m
    edges, index, recs = [], [], []
    for n, labs in enumerate(_labels_of(labels_per_image, N)):
        for text, x, y in labs:
            x0, x1 = -m, int(f['advance'][_glyphs_of(text)].sum()) + m
            index.append((len(edges), 2, x0, y0, x1, y1))
            edges += [(x1, y0, x1, y1), (x0, y1, x0, y0)]  # counter-clockwise with y up: right side up, left side down
            recs.append((n, len(recs), 0, x, y))
    return np.array(edges, np.int32).reshape(-1, _GEDGE), np.array(index, np.int32).reshape(-1, _GLYPH), np.array(recs, np.int32).reshape(-1, _REC)


def _rows_bound(index, size64):
    """an upper bound of the pixel rows of any glyph's box at this size"""
    ext = int((index[:, 5].astype(np.int64) - index[:, 3]).max()) if len(index) else 0
    return min(ext * size64 // _LATTICE + 2, 65535)


def _out_buffer(packed, shapes, out, device):
    """(src, out, device) of a paint-over: `out` holds the picture already and is painted in place, or the images are copied"""
    if out is not None:
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and out.dim() == 1 and out.is_contiguous()
                and out.numel() == packed.numel() and (device is None or out.device == torch.device(device))):
            raise ValueError('out must be a packed uint8 device tensor of %d bytes%s' % (packed.numel(), '' if device is None else ' on %s' % (device, )))
        return out, out, out.device
    dev = cuda_device('rendering', device, packed)
    src = packed_on(packed, shapes, dev)
    return src, torch.empty_like(src), dev


def draw_labels(images, labels_per_image, color=(255, 0, 0), height=16, background=None, out=None, device=None):
    """The cv2.putText step of test_ocr.py:197-210 / test_webcam.py:274-284 for a batch: every label written onto its image.

    labels_per_image: per image a list of (text, (x, y)); for a single image also that list itself.  (x, y), integers
    within +-2^20, is the left end of the baseline, as cv2's org; text may run off the image or lie outside it.  height: the
    cap height in pixels (a float in 4 .. 512; 16 is about what FONT_HERSHEY_SIMPLEX gives at scale 0.75).  Characters
    are laid left to right by their advances, no kerning, no line breaks; one outside ASCII 32 .. 126 is drawn as '?'; at
    most 256 per label; empty strings and empty lists are legal.  background=(r, g, b) first fills each label's
    rectangle (its advance by ascender to descender, plus a 2-pixel margin) in a launch of its own.

    LABEL TEXT IS THIS PROJECT'S DEFINITION, not cv2's Hershey strokes: the outlines of DejaVu Sans (fonts/dejavu_sans.txt),
    filled by the non-zero winding rule at pixel centres in exact integers: a pixel is on or off, nothing is
    anti-aliased (neither is cv2's LINE_8 text).  PARITY UNPINNED against cv2.putText by construction.  DESIGN section 29.

    Returns the packed uint8 device copy with the labels; out: a packed uint8 device buffer that already holds the picture
    (e.g. the result of draw_outlines), painted in place and returned, `images` then only gives the shapes.  One launch
    (dbn_draw_glyphs), two with a background, on the current stream."""
    packed, shapes = as_images(images)
    c = _color(color)
    bg = _color(background) if background is not None else None
    s = _size64(height)
    N = len(shapes)
    recs = label_records(labels_per_image, N)
    src, out, dev = _out_buffer(packed, shapes, out, device)
    if src.numel() == 0:
        return out
    d = image_table(shapes, dev)
    if bg is not None:
        e, g, r = label_backgrounds(labels_per_image, N, s)
        te, tg, tr = (upload(a, dev) if len(a) else None for a in (e, g, r))
        _call('dbn_draw_glyphs', dev, src.data_ptr(), out.data_ptr(), src.numel(), d.data_ptr(), N, te.data_ptr() if len(r) else None, len(e),
              tg.data_ptr() if len(r) else None, len(g), tr.data_ptr() if len(r) else None, len(r), s, _rows_bound(g, s), bg[0], bg[1], bg[2])
        src = out
    fe, fg = _font_on(dev)
    tr = upload(recs, dev) if len(recs) else None
    _call('dbn_draw_glyphs', dev, src.data_ptr(), out.data_ptr(), src.numel(), d.data_ptr(), N, fe.data_ptr(), fe.shape[0], fg.data_ptr(), fg.shape[0],
          tr.data_ptr() if tr is not None else None, len(recs), s, _rows_bound(glyph_table()['index'], s), c[0], c[1], c[2])
    return out


def draw_dots(images, points_per_image, color=(0, 255, 0), out=None, device=None):
    """The anchor dots of test_ocr.py:202-205, cv2.circle(img, (x, y), radius=0, thickness=int(H * 0.01)): per image of
    height H a disc of diameter d = int(H * 0.01) about every (x, y) of points_per_image[n], none where d is 0.  A disc is
    one zero-length edge through dbn_draw_strokes (d = 1: the pixel itself; d >= 2: 4 r^2 <= d^2, this project's stroke):
    one launch per distinct d > 0, in ascending order.  out: as draw_labels."""
    packed, shapes = as_images(images)
    c = _color(color)
    if not isinstance(points_per_image, (list, tuple)) or len(points_per_image) != len(shapes):
        raise ValueError('points for %s images, but %d images' % (len(points_per_image) if isinstance(points_per_image, (list, tuple)) else '?', len(shapes)))
    by_d = {}
    for n, pts in enumerate(points_per_image):
        d = min(int(shapes[n][0] * 0.01), 255)
        for x, y in pts:
            if int(x) != x or int(y) != y or abs(int(x)) > _VERT_MAX or abs(int(y)) > _VERT_MAX:
                raise ValueError('a point of image %d must be integers within +-%d, got %r' % (n, _VERT_MAX, (x, y)))
            if d > 0:
                by_d.setdefault(d, []).append((n, int(x), int(y), int(x), int(y)))
    src, out, dev = _out_buffer(packed, shapes, out, device)
    if src.numel() == 0:
        return out
    desc = image_table(shapes, dev)
    if not by_d and src is not out:
        out.copy_(src)
    for d in sorted(by_d):
        e = upload(np.array(by_d[d], np.int32), dev)
        _call('dbn_draw_strokes', dev, src.data_ptr(), out.data_ptr(), src.numel(), desc.data_ptr(), len(shapes), e.data_ptr(), len(by_d[d]), d, c[0],
              c[1], c[2])
        src = out
    return out


def _words_of(words_per_image, N):
    ws = words_per_image
    if N == 1 and isinstance(ws, (list, tuple)) and len(ws) > 0 and isinstance(ws[0], dict):
        ws = [ws]
    if not isinstance(ws, (list, tuple)) or len(ws) != N:
        raise ValueError('words for %s images, but %d images' % (len(ws) if isinstance(ws, (list, tuple)) else '?', N))
    out = []
    for n, words in enumerate(ws):
        rows = []
        for w in words:
            box = None if not isinstance(w, dict) or w.get('box') is None else np.asarray(w['box'])
            if box is None or box.ndim != 2 or box.shape[0] < 1 or box.shape[1] != 2 or box.dtype.kind not in 'iu':
                raise ValueError('a word of image %d must be {\'box\': integer [P, 2], \'pred\': str, ...} as recognize_words gives it' % n)
            rows.append((str(w['pred']), (int(box[0, 0]), int(box[0, 1]))))
        out.append(rows)
    return out


def draw_words(images, words_per_image, color=(255, 0, 0), height=16, dots=True, dot_color=(0, 255, 0), background=None, out=None, device=None):
    """test_ocr.py:201-207 for a batch: words_per_image is the output of recognize_words (per image a list of {'box', 'pred',
    'score'}); each `pred` is written at box[0], the first corner of its box, and with `dots` the anchor disc is drawn
    there first.  The same bytes and launches as draw_dots(images, anchors, dot_color) followed by
    draw_labels(..., out=that result), which is how it runs (all dots, then all text: the reference goes word by word, so
    there a later dot may cover earlier text).  Label text is this project's definition (draw_labels), not cv2's."""
    packed, shapes = as_images(images)
    labels = _words_of(words_per_image, len(shapes))
    if dots:
        out = draw_dots((packed, shapes), [[p for _, p in labs] for labs in labels], dot_color, out=out, device=device)
    return draw_labels((packed, shapes), labels, color, height, background, out=out, device=device)


def score_labels(detections_per_image, N, fmt='%.2f'):
    """per image the (text, (x, y)) labels draw_scores writes: fmt % score at the first vertex of every shape that
    draw_outlines draws (coordinate sum > 0)"""
    d = detections_per_image
    if N == 1 and _is_pair(d):
        d = [d]
    if not isinstance(d, (list, tuple)) or len(d) != N:
        raise ValueError('detections for %s images, but %d images' % (len(d) if isinstance(d, (list, tuple)) else '?', N))
    out = []
    for n, entry in enumerate(d):
        if not _is_pair(entry) or len(entry[0]) != len(entry[1]):
            raise ValueError('detections of image %d must be the (shapes, scores) pair of detect_boxes / detect_polygons' % n)
        rows = []
        for p, sc in zip(entry[0], entry[1]):
            p = np.asarray(p).astype(np.int64).reshape(-1, 2)
            if len(p) and p.sum() > 0:
                rows.append((fmt % float(sc), (int(p[0, 0]), int(p[0, 1]))))
        out.append(rows)
    return out


def draw_scores(images, detections_per_image, fmt='%.2f', color=(255, 0, 0), height=16, background=None, out=None, device=None):
    """Every detection's score written at its first vertex, for the (boxes, scores) pairs of detect_boxes and the (polygons,
    scores) pairs of detect_polygons alike: draw_labels(images, score_labels(detections, N, fmt), ...).  Needs no
    recogniser.  Label text is this project's definition (draw_labels), not cv2's."""
    packed, shapes = as_images(images)
    return draw_labels((packed, shapes), score_labels(detections_per_image, len(shapes), fmt), color, height, background, out=out, device=device)


def render_detections(images, prob, shapes_per_image, valid_hw=None, color=(255, 0, 0), thickness=3, cmap='inferno', alpha=0.6, vmin=None,
                      vmax=None, heatmap=True, words=None, scores=False, height=16):
    """utils.visualize_polygon's picture for a batch, in the reference's order (utils.py:252-275): the outlines of every
    shape on a copy of the images, then the heat map over everything.  The same bytes as draw_outlines followed by
    overlay_heatmap(out=...), which is how it runs.  heatmap=False stops after the outlines (test_ocr.py / test_webcam.py).
    scores=True then writes every detection's score (draw_scores(images, shapes_per_image, out=...)) and words= (the
    output of recognize_words) the recognised strings with their anchor dots (draw_words(images, words, out=...)), in
    that order, in `color` at cap height `height`, after the map so that they stay readable.  Label text is this
    project's definition (draw_labels), not cv2.putText's."""
    packed, shapes = as_images(images)
    out = draw_outlines((packed, shapes), shapes_per_image, color, thickness, device=prob.device if isinstance(prob, torch.Tensor) else None)
    if heatmap:
        out = overlay_heatmap((packed, shapes), prob, valid_hw, cmap, alpha, vmin, vmax, out=out)
    if scores:
        out = draw_scores((packed, shapes), shapes_per_image, color=color, height=height, out=out)
    if words is not None:
        out = draw_words((packed, shapes), words, color, height, out=out)
    return out


def minmax_scale_u8(x):
    """utils.minmax_scaler_img (:110-113) of a device fp32 [N, 3, H, W] (or [3, H, W]) batch, per image:
    ((x - min) * (1 / (max - min) * 255)).astype(uint8) -> uint8 [N, H, W, 3] (or [H, W, 3]).  As numpy evaluates it on
    float32 data: the factor and the product in float32, astype truncating.  A constant image gives zeros (numpy: NaN)."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() in (3, 4) and x.shape[-3] == 3):
        raise ValueError('minmax_scale_u8 takes a float32 device tensor [N, 3, H, W] or [3, H, W]')
    single = x.dim() == 3
    x4 = (x[None] if single else x).contiguous()
    N, _, H, W = x4.shape
    if not (1 <= N <= 65535 and H >= 1 and W >= 1):
        raise ValueError('minmax_scale_u8: empty input or more than 65535 images')
    out = torch.empty((N, H, W, 3), device=x.device, dtype=torch.uint8)
    mm = torch.empty(2 * N, device=x.device, dtype=torch.int32)
    _call('dbn_minmax_scale_u8', x.device, x4.data_ptr(), N, H, W, mm.data_ptr(), out.data_ptr())
    return out[0] if single else out


# ---- python -m db_text_minimal_amd.render: the shape of the reference's test.py ----------------------------------------
def _is_jpeg(path):
    return path.lower().endswith(('.jpg', '.jpeg'))


def _is_png(path):
    return path.lower().endswith('.png')


def _read_image(path, orient=False):
    if path.endswith('.npy'):
        img = np.load(path)
    elif _is_jpeg(path):  # the project's own decoder, progressive and multi-scan files included; a kind it refuses (CMYK, ...) goes through PIL when that is installed
        from .jpeg import decode_jpeg
        with open(path, 'rb') as f:
            return decode_jpeg(f.read(), fallback=True, multiscan=True, orient=orient)
    elif _is_png(path):  # the project's own decoder; a kind it refuses (CgBI, larger than its limits) goes through PIL when that is installed
        from .png import decode_png
        with open(path, 'rb') as f:
            return decode_png(f.read(), fallback=True)
    else:
        from PIL import Image  # only when the suffix asks for it
        img = np.asarray(Image.open(path).convert('RGB'))
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError('%s must hold a uint8 [H, W, 3] image' % path)
    return np.ascontiguousarray(img)


def _write_image(path, img):
    """img: uint8 [H, W, 3] device tensor"""
    if _is_jpeg(path):  # the project's own encoder (quality 75, 4:2:0: what Pillow writes by default); PIL is not imported
        from .jpeg import encode_jpeg
        with open(path, 'wb') as f:
            f.write(encode_jpeg(img))
        return
    if _is_png(path):  # lossless, filters chosen on the GPU; PIL is not imported
        from .png import encode_png
        with open(path, 'wb') as f:
            f.write(encode_png(img))
        return
    img = img.cpu().numpy()
    if path.endswith('.npy'):
        np.save(path, img)
    else:
        from PIL import Image
        Image.fromarray(img).save(path)


def main(argv=None):
    import argparse

    from .augment import preprocess_image
    from .models import DBTextModel
    from .postprocess import detect_boxes, detect_polygons
    ap = argparse.ArgumentParser(description='detect text in one image and draw the result (the reference\'s test.py)')
    ap.add_argument('--image', required=True, help='.npy uint8 [H, W, 3], a .jpg / .jpeg or .png file, or another image file when PIL is installed')
    ap.add_argument('--model_path', required=True)
    ap.add_argument('--is_output_polygon', action='store_true')
    ap.add_argument('--heatmap', action='store_true', help='lay the probability map over the outlines (test.py)')
    ap.add_argument('--scores', action='store_true', help='write every detection\'s score at its first vertex (draw_scores)')
    ap.add_argument('--out', default=None, help='.npy, .jpg / .jpeg (written by encode_jpeg), .png (encode_png), or another suffix when PIL is installed')
    ap.add_argument('--thresh', type=float, default=0.25)
    ap.add_argument('--box_thresh', type=float, default=0.5)
    ap.add_argument('--unclip_ratio', type=float, default=1.5)
    ap.add_argument('--alpha', type=float, default=0.6)
    ap.add_argument('--orient', action='store_true', help='apply a JPEG file\'s Exif orientation, as cv2.imread does (default: as stored)')
    args = ap.parse_args(argv)
    dev = torch.device('cuda')
    img = _read_image(args.image, args.orient)
    img = (img if isinstance(img, torch.Tensor) else torch.from_numpy(img)).to(dev)
    model = DBTextModel().to(dev)
    model.load_state_dict(torch.load(args.model_path, map_location=dev))
    model.eval()
    with torch.no_grad():
        preds = model(preprocess_image(img, 640, pad=False))
    if isinstance(preds, (tuple, list)):
        preds = torch.stack([p.reshape(p.shape[0], p.shape[-2], p.shape[-1]) for p in preds], 1)
    detect = detect_polygons if args.is_output_polygon else detect_boxes
    res = detect(preds, args.thresh, args.box_thresh, unclip_ratio=args.unclip_ratio, dest_sizes=[tuple(img.shape[:2])])
    out = render_detections(img, preds, res, alpha=args.alpha, heatmap=args.heatmap, scores=args.scores)
    path = args.out or os.path.splitext(args.image)[0] + ('_poly' if args.is_output_polygon else '_rect') + '_result.npy'
    _write_image(path, image_views(out, [tuple(img.shape[:2])])[0])
    print(path)


if __name__ == '__main__':
    main()
