"""Showing a detection result on the device: the last step of the reference's inference path.  test.py, test_ocr.py and
test_webcam.py end in utils.draw_bbox (cv2.polylines of every box on a copy of the original image, utils.py:202-212), and
test.py lays the probability map, resized to the original image with cv2.resize and coloured by a matplotlib colormap,
over it at alpha = 0.6 (utils.visualize_polygon :252-283, utils.visualize_heatmap :215-228).

  draw_outlines(images, shapes_per_image, color, thickness)   utils.draw_bbox for a batch: one copy, one launch
  overlay_heatmap(images, prob, valid_hw, cmap, alpha, ...)    the resized, coloured, blended map: one launch, plus one
                                                              reduction launch when the colour limits are autoscaled
  render_detections(images, prob, shapes, ...)                both, in the reference's order (outlines, then the map)
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

  python -m db_text_minimal_amd.render --image X --model_path M [--is_output_polygon] [--heatmap] [--out Y]
"""
import os

import numpy as np
import torch

from ._lib import check, lib
from .augment import _check_shape, _offsets, _packed, _resize_coef, _stream, _to_device
from .word_crops import _images

CMAPS = ('inferno', 'jet')
_VERT_MAX = 2 ** 20  # |vertex coordinate| of a shape (csrc/render.hip)
_INT_MAX = 2 ** 31 - 1
_EDGE, _IDESC, _PDESC, _COEF = 5, 3, 5, 4
LAUNCH_LOG = []  # the C entry points called, in order (tests clear it and read it back)
_tables = {}


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


def _call(name, *args):
    LAUNCH_LOG.append(name)
    check(getattr(lib(), name)(*args), name)


def _device(packed, device):
    dev = torch.device(device) if device is not None else (packed.device if packed.is_cuda else torch.device('cuda', torch.cuda.current_device()))
    if dev.type != 'cuda':
        raise ValueError('rendering runs on a GPU device, not %s' % dev)
    return dev


def image_views(packed, shapes):
    """per-image uint8 [H, W, 3] views of a packed result"""
    shapes = [_check_shape(s) for s in shapes]
    off = _offsets([h * w * 3 for h, w in shapes])
    if packed.dim() != 1 or packed.numel() != int(off[-1]):
        raise ValueError('the packed images hold %d bytes, the shapes need %d' % (packed.numel(), int(off[-1])))
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
    packed, shapes = _images(images)
    c = _color(color)
    if isinstance(thickness, bool) or int(thickness) != thickness or not 1 <= int(thickness) <= 255:
        raise ValueError('thickness must be an integer in 1 .. 255, got %r' % (thickness, ))
    edges = stroke_edges(shapes_per_image, len(shapes))
    if -(-len(edges) // 4) > _INT_MAX:
        raise ValueError('%d edges are too many for one call' % len(edges))
    dev = _device(packed, device)
    src = _packed(packed, shapes, dev)
    out = torch.empty_like(src)
    if src.numel() == 0:
        return out
    desc = np.stack([_offsets([h * w * 3 for h, w in shapes])[:-1], [h for h, _ in shapes], [w for _, w in shapes]], 1).astype(np.int64)
    d = _to_device(desc, dev)
    e = _to_device(edges, dev) if len(edges) else None
    _call('dbn_draw_strokes', src.data_ptr(), out.data_ptr(), src.numel(), d.data_ptr(), len(shapes), e.data_ptr() if e is not None else None,
          len(edges), int(thickness), c[0], c[1], c[2], _stream(dev))
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
        coef[n] = _resize_coef(vw, W), _resize_coef(vh, H), lo[n], hi[n]
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
    packed, shapes = _images(images)
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
        src = _packed(packed, shapes, dev)
        out = torch.empty_like(src)
    n_px = src.numel() // 3
    if -(-n_px // 1024) > _INT_MAX:
        raise ValueError('%d pixels are too many for one call' % n_px)
    if n_px == 0:
        return out
    prob = prob.contiguous()
    img_stride = prob.numel() // N
    d, c = _to_device(desc, dev), _to_device(coef, dev)
    lut = _to_device((table[:, 0].astype(np.int64) | table[:, 1].astype(np.int64) << 8 | table[:, 2].astype(np.int64) << 16).astype(np.int32), dev)
    is_bin, thresh = (0, 0.0) if binary is None else (1, float(binary))
    common = (d.data_ptr(), c.data_ptr(), N, n_px, prob.data_ptr(), prob.numel(), img_stride, Wm, is_bin, thresh)
    mm = None
    if auto:
        mm = torch.empty(2 * N, device=dev, dtype=torch.int32)
        _call('dbn_render_minmax', *common, mm.data_ptr(), _stream(dev))
    _call('dbn_render_paint', src.data_ptr(), out.data_ptr(), *common, mm.data_ptr() if auto else None, lut.data_ptr(), a, _stream(dev))
    return out


def render_detections(images, prob, shapes_per_image, valid_hw=None, color=(255, 0, 0), thickness=3, cmap='inferno', alpha=0.6, vmin=None,
                      vmax=None, heatmap=True):
    """utils.visualize_polygon's picture for a batch, in the reference's order (utils.py:252-275): the outlines of every
    shape on a copy of the images, then the heat map over everything.  The same bytes as draw_outlines followed by
    overlay_heatmap(out=...), which is how it runs.  heatmap=False stops after the outlines (test_ocr.py / test_webcam.py)."""
    packed, shapes = _images(images)
    out = draw_outlines((packed, shapes), shapes_per_image, color, thickness, device=prob.device if isinstance(prob, torch.Tensor) else None)
    if not heatmap:
        return out
    return overlay_heatmap((packed, shapes), prob, valid_hw, cmap, alpha, vmin, vmax, out=out)


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
    _call('dbn_minmax_scale_u8', x4.data_ptr(), N, H, W, mm.data_ptr(), out.data_ptr(), _stream(x.device))
    return out[0] if single else out


# ---- python -m db_text_minimal_amd.render: the shape of the reference's test.py ----------------------------------------
def _is_jpeg(path):
    return path.lower().endswith(('.jpg', '.jpeg'))


def _read_image(path, orient=False):
    if path.endswith('.npy'):
        img = np.load(path)
    elif _is_jpeg(path):  # the project's own decoder, progressive and multi-scan files included; a kind it refuses (CMYK, ...) goes through PIL when that is installed
        from .jpeg import decode_jpeg
        with open(path, 'rb') as f:
            return decode_jpeg(f.read(), fallback=True, multiscan=True, orient=orient)
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
    ap.add_argument('--image', required=True, help='.npy uint8 [H, W, 3], a .jpg / .jpeg file, or another image file when PIL is installed')
    ap.add_argument('--model_path', required=True)
    ap.add_argument('--is_output_polygon', action='store_true')
    ap.add_argument('--heatmap', action='store_true', help='lay the probability map over the outlines (test.py)')
    ap.add_argument('--out', default=None, help='.npy, .jpg / .jpeg (written by encode_jpeg), or another suffix when PIL is installed')
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
    out = render_detections(img, preds, res, alpha=args.alpha, heatmap=args.heatmap)
    path = args.out or os.path.splitext(args.image)[0] + ('_poly' if args.is_output_polygon else '_rect') + '_result.npy'
    _write_image(path, image_views(out, [tuple(img.shape[:2])])[0])
    print(path)


if __name__ == '__main__':
    main()
