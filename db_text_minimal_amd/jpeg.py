"""JPEG decode in front of the device pipeline, in the place of the reference's cv2.imread(path)[:, :, ::-1]
(data_loaders.py:78, utils.py:179): the Huffman stage on the host in C++ (threaded over the images of a batch, no GIL), the
rest — dequantisation, libjpeg's slow-integer inverse DCT, fancy chroma upsampling, YCbCr -> RGB — as gfx950 kernels that
write the packed uint8 layout augment_images, crop_words and draw_outlines take (csrc/jpeg.hip).  Bit for bit libjpeg's
baseline decode (pinned against Pillow / libjpeg-turbo, tests/test_jpeg_cpu.py).

  jpeg_info(data)                          -> dict (size, components, sampling, restart interval, Exif orientation, support)
  decode_jpeg_batch(datas, device)         -> (packed uint8 device tensor, shapes): what augment_images(packed, shapes, plans) takes
  decode_jpeg(data, device)                -> uint8 [H, W, 3] device tensor (preprocess_image, crop_words, render)
  entropy_decode(datas)                    -> JpegCoefficients (host half; runs anywhere, e.g. in a DataLoader worker)
  decode_coefficients(obj, device)         -> (packed, shapes) (device half)
  jpeg_collate(items)                      collate_fn for items (jpeg bytes, polys, tags): the host half in the worker;
                                           DeviceBatches.convert runs the device half

Supported: baseline and 8-bit extended sequential Huffman streams, grey or YCbCr, 4:4:4 / 4:2:2 / 4:2:0, restart markers.
Every other kind raises UnsupportedJpeg(reason); a damaged stream raises CorruptJpeg.  The Exif orientation is reported
(jpeg_info(...)['orientation']) and NOT applied: PIL does not apply it either, cv2.imread does.
"""
import numpy as np
import torch

from ._lib import check, lib

_DESC, _INFO = 24, 24
_D_COEF, _D_W, _D_H, _D_NC, _D_OUT, _D_QT, _D_COMP, _D_STATUS = 0, 1, 2, 3, 4, 5, 6, 22
IDCT_BLOCKS, RGB_PIXELS = 32, 1024  # per workgroup (csrc/jpeg.hip)
MAX_THREADS = 16

REASONS = {
    1: 'not a JPEG stream', 2: 'truncated stream', 3: 'progressive (SOF2) is not supported', 4: 'arithmetic coding is not supported',
    5: 'lossless / hierarchical processes are not supported', 6: 'sample precision is not 8 bits (12-bit is not supported)',
    7: '4-component / Adobe-transform files are not supported',
    8: 'sampling factors other than 4:4:4, 4:2:2 (2x1) and 4:2:0 (2x2) are not supported',
    9: 'non-interleaved multi-scan files are not supported', 10: 'malformed header or missing table', 11: 'invalid Huffman code',
    12: 'coefficient run past index 63', 13: 'entropy data and markers disagree (too few or too many MCUs before a marker)',
}
_REFUSED = (3, 4, 5, 6, 7, 8, 9)  # valid JPEG kinds this decoder does not take (another decoder can)


class JpegError(ValueError):
    """a stream that was not decoded: .code is the status of include/dbnet_hip.h, .index the image's place in its batch"""

    def __init__(self, code, index=None):
        self.code, self.index, self.reason = int(code), index, REASONS.get(int(code), 'status %d' % code)
        ValueError.__init__(self, self.reason if index is None else 'image %d: %s' % (index, self.reason))


class UnsupportedJpeg(JpegError):
    """a kind of JPEG this decoder refuses (progressive, arithmetic, lossless, 12-bit, CMYK, other samplings, multi-scan)"""


class CorruptJpeg(JpegError):
    """not a JPEG, or one that is truncated or damaged"""


def _error(code, index=None):
    return (UnsupportedJpeg if code in _REFUSED else CorruptJpeg)(code, index)


def _bytes_view(data):
    a = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8).reshape(-1)
    return a


def jpeg_info(data):
    """Markers of one stream, without decoding it: dict(width, height, components, sampling [(h, v)], restart_interval,
    orientation (Exif tag 0x0112, 0 when absent; reported, not applied), process ('baseline' / 'extended'), jfif, adobe_transform
    (None without the marker), precision, status, supported, reason)."""
    a = _bytes_view(data)
    out = np.zeros(_INFO, np.int64)
    buf = a if a.size else np.zeros(1, np.uint8)
    check(lib().dbn_jpeg_info(buf.ctypes.data, int(a.size), out.ctypes.data), 'jpeg_info')
    st, nc = int(out[0]), int(out[3])
    return dict(width=int(out[1]), height=int(out[2]), components=nc, sampling=[(int(out[6 + 2 * c]), int(out[7 + 2 * c])) for c in range(min(nc, 4))],
                restart_interval=int(out[4]), orientation=int(out[5]), process={0: 'baseline', 1: 'extended'}.get(int(out[14])),
                jfif=bool(out[16]), adobe_transform=None if out[17] < 0 else int(out[17]), precision=int(out[18]), status=st,
                supported=st == 0, reason=None if st == 0 else REASONS.get(st), coefficients=int(out[15]))


class JpegCoefficients:
    """The host half's result for a batch: `coef` int16 tensor (pinned when asked for), `desc` int64 [N, 24], `qtabs` uint16
    [N, 3, 64], `status` int32 [N] (0: decoded) and `shapes` [(H, W)] ((0, 0) for an image that failed).  Layouts:
    include/dbnet_hip.h.  Picklable, and pin_memory() makes it what a DataLoader with pin_memory=True hands on."""

    def __init__(self, coef, desc, qtabs, status):
        self.coef, self.desc, self.qtabs, self.status = coef, desc, qtabs, status

    @property
    def shapes(self):
        return [(int(d[_D_H]), int(d[_D_W])) if s == 0 else (0, 0) for d, s in zip(self.desc, self.status)]

    def __len__(self):
        return len(self.status)

    def pin_memory(self):
        if not self.coef.is_pinned():
            self.coef = self.coef.pin_memory()
        return self

    def errors(self):
        """per image None or the JpegError that describes why it was not decoded"""
        return [None if s == 0 else _error(int(s), i) for i, s in enumerate(self.status)]


def entropy_decode(datas, threads=MAX_THREADS, pin=None):
    """Host half: Huffman-decode the JPEG byte strings `datas` on min(len(datas), 16, threads) threads -> JpegCoefficients.
    pin: pinned coefficient memory; default when a GPU is visible and this is not a DataLoader worker (a loader's
    pin_memory=True pins it otherwise).  A stream that fails is reported in .status and fails alone."""
    views = [_bytes_view(d) for d in datas]
    N = len(views)
    if N == 0:
        raise ValueError('entropy_decode needs at least one stream')
    offs = np.zeros(N + 1, np.int64)
    offs[1:] = np.cumsum([v.size for v in views])
    blob = np.concatenate(views) if offs[-1] else np.zeros(1, np.uint8)
    L = lib()
    total = int(L.dbn_jpeg_coef_elems(blob.ctypes.data, offs.ctypes.data, N, None))
    if total < 0:
        raise RuntimeError('libdbnet_hip: jpeg_coef_elems failed')
    if pin is None:
        pin = torch.utils.data.get_worker_info() is None and torch.cuda.is_available()
    coef = torch.empty(max(total, 1), dtype=torch.int16, pin_memory=bool(pin))
    desc = np.zeros((N, _DESC), np.int64)
    qtabs = np.zeros((N, 3, 64), np.uint16)
    status = np.zeros(N, np.int32)
    check(L.dbn_jpeg_entropy_batch(blob.ctypes.data, offs.ctypes.data, N, coef.data_ptr(), total, desc.ctypes.data, qtabs.ctypes.data,
                                   status.ctypes.data, int(threads)), 'jpeg_entropy_batch')
    return JpegCoefficients(coef[:total], desc, qtabs, status)


def work_tables(desc, status):
    """the per-workgroup tables of dbn_jpeg_pixels: (int32 [n_idct, 4] {image, component, first block, 0}, int32 [n_rgb, 4] {image, chunk, 0, 0})"""
    ta, tb = [], []
    for n in np.nonzero(np.asarray(status) == 0)[0]:
        d = desc[n]
        for c in range(int(d[_D_NC])):
            first = np.arange(0, int(d[_D_COMP + 4 * c]) * int(d[_D_COMP + 4 * c + 1]), IDCT_BLOCKS, dtype=np.int32)
            e = np.zeros((first.size, 4), np.int32)
            e[:, 0], e[:, 1], e[:, 2] = n, c, first
            ta.append(e)
        chunks = np.arange(-(-int(d[_D_W]) * int(d[_D_H]) // RGB_PIXELS), dtype=np.int32)
        e = np.zeros((chunks.size, 4), np.int32)
        e[:, 0], e[:, 1] = n, chunks
        tb.append(e)
    if not ta:
        return np.zeros((0, 4), np.int32), np.zeros((0, 4), np.int32)
    return np.concatenate(ta), np.concatenate(tb)


def _up(a, dev):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.pin_memory() if torch.cuda.is_available() else t).to(dev, non_blocking=True)


def decode_coefficients(obj, device=None):
    """Device half: JpegCoefficients -> (packed uint8 device tensor, shapes), on the current stream of `device`, no host
    sync.  Images whose status is not 0 take no bytes and have shape (0, 0) (see obj.errors())."""
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    if dev.type != 'cuda':
        raise ValueError('decode_coefficients runs on a GPU device, not %s' % dev)
    if dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    shapes = obj.shapes
    out_bytes = int(sum(h * w * 3 for h, w in shapes))
    out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
    if out_bytes == 0:
        return out, shapes
    ta, tb = work_tables(obj.desc, obj.status)
    hdesc = obj.desc.copy()  # pixels of the decoded images only, packed: an image whose scan failed gives its slot up
    hdesc[:, _D_OUT] = np.concatenate([[0], np.cumsum([h * w * 3 for h, w in shapes])[:-1]])
    with torch.cuda.device(dev):
        coef = obj.coef.to(dev, non_blocking=True)
        desc, qt, a, b = _up(hdesc, dev), _up(obj.qtabs.view(np.int16), dev), _up(ta, dev), _up(tb, dev)
        planes = torch.empty(coef.numel(), dtype=torch.uint8, device=dev)
        check(lib().dbn_jpeg_pixels(coef.data_ptr(), coef.numel(), desc.data_ptr(), qt.data_ptr(), len(obj), a.data_ptr(), len(ta), b.data_ptr(),
                                    len(tb), planes.data_ptr(), out.data_ptr(), out_bytes, torch.cuda.current_stream(dev).cuda_stream),
              'jpeg_pixels')
    return out, shapes


def _pil_rgb(data):
    import io

    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(bytes(data))).convert('RGB')))


def splice_images(packed, shapes, spliced):
    """put the uint8 [H, W, 3] arrays spliced[i] into the packed batch at the places of images i, which took no bytes in
    it (shape (0, 0)) -> (packed, shapes)"""
    parts, out_shapes, o = [], [], 0
    for i, (h, w) in enumerate(shapes):
        if i in spliced:
            if (h, w) != (0, 0):
                raise ValueError('image %d is already in the packed batch' % i)
            a = np.ascontiguousarray(spliced[i], np.uint8)
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError('a spliced image is uint8 [H, W, 3]')
            parts.append(torch.from_numpy(a.reshape(-1)).to(packed.device))
            out_shapes.append((int(a.shape[0]), int(a.shape[1])))
        else:
            parts.append(packed[o:o + h * w * 3])
            out_shapes.append((h, w))
            o += h * w * 3
    if o != packed.numel():
        raise ValueError('packed holds %d bytes, the shapes need %d' % (packed.numel(), o))
    return torch.cat(parts), out_shapes


def decode_jpeg_batch(datas, device=None, threads=MAX_THREADS, fallback=False, errors='raise'):
    """JPEG byte strings -> (packed uint8 device tensor, shapes [(H, W)]): RGB, image after image, what
    augment_images(packed, shapes, plans) takes.  A refused kind raises UnsupportedJpeg, a damaged stream CorruptJpeg (both
    name the image); fallback=True decodes refused kinds through PIL, when it is importable, and splices them in.
    errors='report': nothing raises; -> (packed, shapes, errs) with errs[i] None or the exception, a failed image taking
    no bytes and shape (0, 0)."""
    if errors not in ('raise', 'report'):
        raise ValueError("errors is 'raise' or 'report'")
    datas = list(datas)
    obj = entropy_decode(datas, threads)
    errs = obj.errors()
    spliced = {}
    if fallback:
        for i, e in enumerate(errs):
            if isinstance(e, UnsupportedJpeg):
                try:
                    spliced[i] = _pil_rgb(datas[i])
                    errs[i] = None
                except ImportError:
                    break
                except Exception:  # PIL could not read it either: the refusal stands
                    pass
    if errors == 'raise':
        for e in errs:
            if e is not None:
                raise e
    packed, shapes = decode_coefficients(obj, device)
    if spliced:
        packed, shapes = splice_images(packed, shapes, spliced)
    return (packed, shapes) if errors == 'raise' else (packed, shapes, errs)


def decode_jpeg(data, device=None, fallback=False):
    """one JPEG byte string -> uint8 [H, W, 3] device tensor (RGB; grey replicated)"""
    packed, shapes = decode_jpeg_batch([data], device, 1, fallback)
    return packed.view(shapes[0][0], shapes[0][1], 3)


def jpeg_collate(items):
    """collate_fn for items (jpeg bytes, polys, tags): the host half of the decode, here (in the DataLoader worker) ->
    (JpegCoefficients, shapes, per-image lists of fp64 [V, 2] polygons, per-image tag lists); DeviceBatches.convert runs the
    device half.  A stream that cannot be decoded raises (UnsupportedJpeg / CorruptJpeg)."""
    obj = entropy_decode([b[0] for b in items], threads=min(len(items), MAX_THREADS))
    for e in obj.errors():
        if e is not None:
            raise e
    polys = [[np.asarray(p, dtype=np.float64).reshape(-1, 2) for p in b[1]] for b in items]
    tags = [list(b[2]) if b[2] is not None else [None] * len(b[1]) for b in items]
    return obj, obj.shapes, polys, tags
