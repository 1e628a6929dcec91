"""JPEG at both ends of the device pipeline.  Decode in front of it, in the place of the reference's cv2.imread(path)[:, :, ::-1]
(data_loaders.py:78, utils.py:179): the Huffman stage on the host in C++ (threaded over the images of a batch, no GIL), the
rest — dequantisation, libjpeg's slow-integer inverse DCT, fancy chroma upsampling, YCbCr -> RGB — as gfx950 kernels that
write the packed uint8 layout augment_images, crop_words and draw_outlines take (csrc/jpeg.hip).  Bit for bit libjpeg's
baseline decode (pinned against Pillow / libjpeg-turbo, tests/test_jpeg_cpu.py).

  jpeg_info(data, multiscan)               -> dict (size, components, sampling, restart interval, Exif orientation, support)
  decode_jpeg_batch(datas, device)         -> (packed uint8 device tensor, shapes): what augment_images(packed, shapes, plans) takes
  decode_jpeg(data, device)                -> uint8 [H, W, 3] device tensor (preprocess_image, crop_words, render)
  entropy_decode(datas)                    -> JpegCoefficients (host half; runs anywhere, e.g. in a DataLoader worker)
  decode_coefficients(obj, device)         -> (packed, shapes) (device half)
  jpeg_collate(items)                      collate_fn for items (jpeg bytes, polys, tags): the host half in the worker;
                                           DeviceBatches.convert runs the device half
  jpeg_multiscan_collate(items)            the same with multiscan=True
  parse_streams(datas)                     -> JpegStreams (headers and the scans cut at their markers; no entropy decoding)
  entropy_decode_device(streams, device)   -> JpegCoefficients on the device: Huffman decoding as gfx950 kernels
                                           (csrc/jpeg_dhuff.hip); only the compressed bytes cross to the device
  jpeg_stream_collate(items)               jpeg_collate with parse_streams in the worker and the Huffman stage on the device

Encode behind it, in the place of the reference's imageio / Pillow writes (utils.py:225,272,280, test_ocr.py:176,210,
ts_request.py:38-39): the decoder turned round (csrc/jpeg_enc.hip).  Colour conversion, chroma downsampling, libjpeg's
slow-integer forward DCT and quantisation run as gfx950 kernels, Huffman coding on the host threads or, with
entropy='device', as gfx950 kernels too (csrc/jpeg_huff.hip: only the compressed scans cross to the host); the Annex K
tables, or with optimize=True each image's own (libjpeg's optimize_coding).  JpegCoefficients is the hand-over in both
directions.  Bit for bit libjpeg's baseline output for the same settings (pinned against Pillow / libjpeg-turbo,
tests/test_jpeg_encode_cpu.py, tests/test_jpeg_optimize_cpu.py).

  quant_tables(quality)                    -> uint16 [2, 64] (jpeg_set_quality's scaling of the Annex K tables)
  forward_coefficients(images, ...)        -> JpegCoefficients (device half; decode_coefficients(...) of it is the lossy round trip)
  entropy_encode(obj, restart_interval)    -> [bytes] (host half; runs anywhere; entropy_encode(entropy_decode(x)) transcodes losslessly)
  entropy_encode_device(obj, ...)          -> [bytes] (the same streams, coded on the device; coefficients on either side)
  optimal_huffman_table(freq)              -> (counts [16], symbols): libjpeg's optimised table for 256 symbol counts
  encode_jpeg_batch(images, ...)           -> [bytes]; encode_jpeg(image, ...) -> bytes; save_jpegs(paths, images, ...) writes files

Supported: baseline and 8-bit extended sequential Huffman streams, grey or YCbCr, 4:4:4 / 4:2:2 / 4:2:0, restart markers; with
multiscan=True (entropy_decode, decode_jpeg_batch, decode_jpeg, jpeg_info) also progressive (SOF2) Huffman streams and
sequential streams whose components come in several scans, decoded by the host entropy stage into the same coefficients
(not by entropy='device').  Every other kind raises UnsupportedJpeg(reason); a damaged stream raises CorruptJpeg.  The Exif
orientation is reported (jpeg_info(...)['orientation'], JpegCoefficients.orientation) and applied only with orient=True
(decode_jpeg_batch, decode_jpeg, decode_coefficients, DeviceBatches), as cv2.imread applies it; by default, as in PIL, it is not.
"""
import os

import numpy as np
import torch

from ._lib import check, lib
from .packed import DecodedBatch, DecodeError, check_bytes, cuda_device, flat_u8, image_offsets, offsets, on_device, pin_default, polys_tags, stream, upload

_DESC, _INFO = 24, 24
_D_COEF, _D_W, _D_H, _D_NC, _D_OUT, _D_QT, _D_COMP, _D_STATUS = 0, 1, 2, 3, 4, 5, 6, 22
IDCT_BLOCKS, RGB_PIXELS, ORIENT_TILE = 32, 1024, 32  # per workgroup (csrc/jpeg.hip); the oriented kernel's tile is 32 x 32 pixels
MAX_THREADS = 16
_MULTISCAN = 1  # flags of the _ex entry points (include/dbnet_hip.h)

REASONS = {
    1: 'not a JPEG stream', 2: 'truncated stream', 3: 'progressive (SOF2) is not supported', 4: 'arithmetic coding is not supported',
    5: 'lossless / hierarchical processes are not supported', 6: 'sample precision is not 8 bits (12-bit is not supported)',
    7: '4-component / Adobe-transform files are not supported',
    8: 'sampling factors other than 4:4:4, 4:2:2 (2x1) and 4:2:0 (2x2) are not supported',
    9: 'non-interleaved multi-scan files are not supported', 10: 'malformed header or missing table', 11: 'invalid Huffman code',
    12: 'coefficient run past index 63', 13: 'entropy data and markers disagree (too few or too many MCUs before a marker)',
}
# status 14 exists with multiscan=True only; REASONS stays the table of the plain entry points (tests/jpeg_ref.py restates it)
MULTISCAN_REASONS = {14: 'scan script incomplete at the end of the image, or longer than 100 scans'}
_REFUSED = (3, 4, 5, 6, 7, 8, 9, 14)  # valid JPEG kinds this decoder does not take (another decoder can)


class JpegError(DecodeError):
    """a stream that was not decoded: .code is the status of include/dbnet_hip.h, .index the image's place in its batch"""
    reasons, refused = {**REASONS, **MULTISCAN_REASONS}, _REFUSED


class UnsupportedJpeg(JpegError):
    """a kind of JPEG this decoder refuses (progressive, arithmetic, lossless, 12-bit, CMYK, other samplings, multi-scan)"""


class CorruptJpeg(JpegError):
    """not a JPEG, or one that is truncated or damaged"""


JpegError.unsupported, JpegError.corrupt = UnsupportedJpeg, CorruptJpeg


def _bytes_view(data):
    a = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8).reshape(-1)
    return a


def _concat_streams(datas, pin):
    """byte strings -> (uint8 tensor that holds them end to end, pinned if asked, one byte long when they are empty; int64
    offsets [N + 1])"""
    views = [_bytes_view(d) for d in datas]
    offs = offsets([v.size for v in views])
    blob = torch.empty(max(int(offs[-1]), 1), dtype=torch.uint8, pin_memory=bool(pin))
    if offs[-1]:
        np.concatenate(views, out=blob.numpy()[:int(offs[-1])])
    return blob, offs


class _JpegBatch(DecodedBatch):
    """what a batch's results share, from `desc` and `status`; errors(): for JpegStreams the ones the headers give"""
    error, _hw = JpegError, (_D_H, _D_W)

    @property
    def oriented_shapes(self):
        """`shapes` as they are once the Exif orientation is applied: (W, H) for tags 5 .. 8"""
        o = getattr(self, 'orientation', None)
        return [(w, h) if o is not None and 5 <= int(o[i]) <= 8 else (h, w) for i, (h, w) in enumerate(self.shapes)]


def jpeg_info(data, multiscan=False):
    """Markers of one stream, without decoding it: dict(width, height, components, sampling [(h, v)], restart_interval,
    orientation (Exif tag 0x0112, 0 when absent; applied by orient=True only), process ('baseline' / 'extended'), jfif,
    adobe_transform (None without the marker), precision, status, supported, reason).  multiscan=True: what entropy_decode(...,
    multiscan=True) takes is `supported` (process may be 'progressive'), and `scans` counts the SOS markers (0 unless supported)."""
    a = _bytes_view(data)
    out = np.zeros(_INFO, np.int64)
    buf = a if a.size else np.zeros(1, np.uint8)
    if multiscan:
        check(lib().dbn_jpeg_info_ex(buf.ctypes.data, int(a.size), _MULTISCAN, out.ctypes.data), 'jpeg_info')
    else:
        check(lib().dbn_jpeg_info(buf.ctypes.data, int(a.size), out.ctypes.data), 'jpeg_info')
    st, nc = int(out[0]), int(out[3])
    more = dict(scans=int(out[19])) if multiscan else {}
    return dict(width=int(out[1]), height=int(out[2]), components=nc, sampling=[(int(out[6 + 2 * c]), int(out[7 + 2 * c])) for c in range(min(nc, 4))],
                restart_interval=int(out[4]), orientation=int(out[5]), process={0: 'baseline', 1: 'extended', 2: 'progressive'}.get(int(out[14])),
                jfif=bool(out[16]), adobe_transform=None if out[17] < 0 else int(out[17]), precision=int(out[18]), status=st,
                supported=st == 0, reason=None if st == 0 else JpegError.reasons.get(st), coefficients=int(out[15]), **more)


class JpegCoefficients(_JpegBatch):
    """The host half's result for a batch: `coef` int16 tensor (pinned when asked for), `desc` int64 [N, 24], `qtabs` uint16
    [N, 3, 64], `status` int32 [N] (0: decoded) and `shapes` [(H, W)] ((0, 0) for an image that failed): the stored shapes.
    `orientation` int32 [N]: the Exif tags (0 or None: none), which decode_coefficients(orient=True) applies; `oriented_shapes` are
    the shapes after that.  Layouts: include/dbnet_hip.h.  Picklable, and pin_memory() makes it what a DataLoader with
    pin_memory=True hands on."""

    orientation = None
    ready = None  # forward_coefficients: the event after which the pinned `coef` holds the device's result
    host_decoded = None  # entropy_decode_device: bool [N], the images the host decoder was asked for

    def __init__(self, coef, desc, qtabs, status):
        self.coef, self.desc, self.qtabs, self.status = coef, desc, qtabs, status

    def wait(self):
        """block the host until `coef` is filled (a result of forward_coefficients arrives on its stream)"""
        if self.ready is not None:
            self.ready.synchronize()
            self.ready = None
        return self

    def __getstate__(self):
        self.wait()
        return dict(self.__dict__)

    def pin_memory(self):
        if not self.coef.is_pinned():
            self.coef = self.coef.pin_memory()
        return self


def entropy_decode(datas, threads=MAX_THREADS, pin=None, multiscan=False):
    """Host half: Huffman-decode the JPEG byte strings `datas` on min(len(datas), 16, threads) threads -> JpegCoefficients.
    pin: pinned coefficient memory; default when a GPU is visible and this is not a DataLoader worker (a loader's
    pin_memory=True pins it otherwise).  A stream that fails is reported in .status and fails alone.  multiscan=True:
    progressive (SOF2) streams and sequential streams of several scans are decoded too, into the same coefficients; every
    other stream gives what it gives without the keyword."""
    blob, offs = _concat_streams(datas, False)
    N = len(offs) - 1
    if N == 0:
        raise ValueError('entropy_decode needs at least one stream')
    L = lib()
    flags = _MULTISCAN if multiscan else 0
    total = int(L.dbn_jpeg_coef_elems_ex(blob.data_ptr(), offs.ctypes.data, N, flags, None))
    if total < 0:
        raise RuntimeError('libdbnet_hip: jpeg_coef_elems failed')
    coef = torch.empty(max(total, 1), dtype=torch.int16, pin_memory=pin_default(pin))
    desc = np.zeros((N, _DESC), np.int64)
    qtabs = np.zeros((N, 3, 64), np.uint16)
    status = np.zeros(N, np.int32)
    orientation = np.zeros(N, np.int32)
    check(L.dbn_jpeg_entropy_batch_ex(blob.data_ptr(), offs.ctypes.data, N, coef.data_ptr(), total, desc.ctypes.data, qtabs.ctypes.data,
                                      status.ctypes.data, orientation.ctypes.data, int(threads), flags), 'jpeg_entropy_batch')
    obj = JpegCoefficients(coef[:total], desc, qtabs, status)
    obj.orientation = orientation
    return obj


def stream_orientations(datas):
    """the Exif orientation tags of JPEG byte strings (0: none), from their markers alone -> int32 [N]"""
    return np.array([jpeg_info(d)['orientation'] for d in datas], np.int32)


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


def tile_table(desc, status, orientation):
    """dbn_jpeg_pixels_ex's table of the oriented images (tag 2 .. 8, status 0): int32 [n_tile, 4] {image, tile row, tile column, 0}
    over the 32 x 32 tiles of each ORIENTED image"""
    tt, orientation = [], np.asarray(orientation)
    for n in np.nonzero((np.asarray(status) == 0) & (orientation >= 2) & (orientation <= 8))[0]:
        h, w = int(desc[n][_D_H]), int(desc[n][_D_W])
        oh, ow = (w, h) if orientation[n] >= 5 else (h, w)
        ty, tx = np.divmod(np.arange(-(-oh // ORIENT_TILE) * -(-ow // ORIENT_TILE), dtype=np.int32), -(-ow // ORIENT_TILE))
        e = np.zeros((ty.size, 4), np.int32)
        e[:, 0], e[:, 1], e[:, 2] = n, ty, tx
        tt.append(e)
    return np.concatenate(tt) if tt else np.zeros((0, 4), np.int32)


def decode_coefficients(obj, device=None, orient=False):
    """Device half: JpegCoefficients -> (packed uint8 device tensor, shapes), on the current stream of `device`, no host
    sync.  Images whose status is not 0 take no bytes and have shape (0, 0) (see obj.errors()).  orient=True: an image whose
    obj.orientation is 2 .. 8 is written turned as cv2.imread turns it (a tiled kernel of its own, in the same call), and
    the shapes returned are obj.oriented_shapes."""
    dev = cuda_device('decode_coefficients', device)
    tags = np.zeros(len(obj), np.int32)
    if orient and obj.orientation is not None:
        tags = np.where(np.asarray(obj.status) == 0, np.asarray(obj.orientation, np.int32), 0).astype(np.int32)
        tags[(tags < 2) | (tags > 8)] = 0
    turned = bool(tags.any())
    shapes = obj.oriented_shapes if turned else obj.shapes
    out_off = image_offsets(shapes)
    out_bytes = int(out_off[-1])
    out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
    if out_bytes == 0:
        return out, shapes
    ta, tb = work_tables(obj.desc, obj.status)
    if turned:
        tb, tt = tb[tags[tb[:, 0]] == 0], tile_table(obj.desc, obj.status, tags)
    hdesc = obj.desc.copy()  # pixels of the decoded images only, packed: an image whose scan failed gives its slot up
    hdesc[:, _D_OUT] = out_off[:-1]
    with on_device(dev) as sh:
        if obj.ready is not None:  # coefficients still on their way from forward_coefficients' stream
            torch.cuda.current_stream(dev).wait_event(obj.ready)
        coef = obj.coef.to(dev, non_blocking=True)
        desc, qt, a, b = upload(hdesc, dev), upload(obj.qtabs.view(np.int16), dev), upload(ta, dev), upload(tb, dev)
        planes = torch.empty(coef.numel(), dtype=torch.uint8, device=dev)
        if turned:
            o, t = upload(tags, dev), upload(tt, dev)
            check(lib().dbn_jpeg_pixels_ex(coef.data_ptr(), coef.numel(), desc.data_ptr(), qt.data_ptr(), len(obj), a.data_ptr(), len(ta),
                                           b.data_ptr() if len(tb) else None, len(tb), o.data_ptr(), t.data_ptr(), len(tt), planes.data_ptr(),
                                           out.data_ptr(), out_bytes, sh), 'jpeg_pixels')
        else:
            check(lib().dbn_jpeg_pixels(coef.data_ptr(), coef.numel(), desc.data_ptr(), qt.data_ptr(), len(obj), a.data_ptr(), len(ta), b.data_ptr(),
                                        len(tb), planes.data_ptr(), out.data_ptr(), out_bytes, sh), 'jpeg_pixels')
    return out, shapes


def _pil_rgb(data):
    """the PIL fallback's decode of a refused stream -> uint8 [H, W, 3] array (tests patch it under this name)"""
    import io

    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(bytes(data))).convert('RGB')))


pil_rgb = _pil_rgb  # the name png imports it by


def orient_array(a, tag):
    """the array [H, W, ...] turned as Exif orientation `tag` says (what cv2.imread and PIL's ImageOps.exif_transpose do)"""
    if tag in (2, 3, 7, 8):
        a = a[:, ::-1]
    if tag in (3, 4, 6, 7):
        a = a[::-1]
    return np.ascontiguousarray(np.swapaxes(a, 0, 1) if 5 <= tag <= 8 else a)


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
    check_bytes(packed.numel(), o)
    return torch.cat(parts), out_shapes


def decode_jpeg_batch(datas, device=None, threads=MAX_THREADS, fallback=False, errors='raise', entropy='host', multiscan=False, orient=False):
    """JPEG byte strings -> (packed uint8 device tensor, shapes [(H, W)]): RGB, image after image, what
    augment_images(packed, shapes, plans) takes.  A refused kind raises UnsupportedJpeg, a damaged stream CorruptJpeg (both
    name the image); fallback=True decodes refused kinds through PIL, when it is importable, and splices them in.
    errors='report': nothing raises; -> (packed, shapes, errs) with errs[i] None or the exception, a failed image taking
    no bytes and shape (0, 0).  entropy='device': the Huffman stage runs on the GPU too (entropy_decode_device): only the
    compressed bytes cross to the device; the pixels are the same.  multiscan=True: progressive and multi-scan streams are
    decoded by the host entropy stage instead of being refused (not with entropy='device', whose kernels do not take them).
    orient=True: the Exif orientation is applied, as cv2.imread applies it: the shapes are (W, H) for tags 5 .. 8; both entropy
    paths, and the PIL fallback's images too."""
    if errors not in ('raise', 'report'):
        raise ValueError("errors is 'raise' or 'report'")
    if entropy not in ('host', 'device'):
        raise ValueError("entropy is 'host' or 'device', got %r" % (entropy, ))
    if entropy == 'device' and multiscan:
        raise ValueError("multiscan=True is the host entropy stage's: the device Huffman decoder does not take progressive or multi-scan streams")
    datas = list(datas)
    if entropy == 'host':
        obj = entropy_decode(datas, threads, multiscan=multiscan)
    else:
        obj = entropy_decode_device(datas, device)
        if orient:
            obj.orientation = stream_orientations(datas)
    errs = obj.errors()
    spliced = {}
    if fallback:
        for i, e in enumerate(errs):
            if isinstance(e, UnsupportedJpeg):
                try:
                    spliced[i] = _pil_rgb(datas[i])
                    if orient:
                        spliced[i] = orient_array(spliced[i], int(obj.orientation[i]))
                    errs[i] = None
                except ImportError:
                    break
                except Exception:  # PIL could not read it either: the refusal stands
                    pass
    if errors == 'raise':
        for e in errs:
            if e is not None:
                raise e
    packed, shapes = decode_coefficients(obj, device, orient)
    if spliced:
        packed, shapes = splice_images(packed, shapes, spliced)
    return (packed, shapes) if errors == 'raise' else (packed, shapes, errs)


def decode_jpeg(data, device=None, fallback=False, entropy='host', multiscan=False, orient=False):
    """one JPEG byte string -> uint8 [H, W, 3] device tensor (RGB; grey replicated); multiscan, orient: as decode_jpeg_batch"""
    packed, shapes = decode_jpeg_batch([data], device, 1, fallback, entropy=entropy, multiscan=multiscan, orient=orient)
    return packed.view(shapes[0][0], shapes[0][1], 3)


def jpeg_collate(items):
    """collate_fn for items (jpeg bytes, polys, tags): the host half of the decode, here (in the DataLoader worker) ->
    (JpegCoefficients, shapes, per-image lists of fp64 [V, 2] polygons, per-image tag lists); DeviceBatches.convert runs the
    device half.  A stream that cannot be decoded raises (UnsupportedJpeg / CorruptJpeg)."""
    return jpeg_multiscan_collate(items, False)


def jpeg_multiscan_collate(items, multiscan=True):
    """jpeg_collate that takes progressive and multi-scan streams as well (entropy_decode(..., multiscan=True)); the keyword
    is there for functools.partial"""
    obj = entropy_decode([b[0] for b in items], threads=min(len(items), MAX_THREADS), multiscan=multiscan)
    obj.raise_errors()
    return (obj, obj.shapes) + polys_tags(items)


# ---- entropy decoding on the device ------------------------------------------------------------------------------------
DHUFF_BITS, DHUFF_LANES = 1024, 256  # bits per subsequence, subsequences per workgroup (csrc/jpeg_dhuff.h)
DHUFF_ROUNDS = 4  # propagation launches after the first: twice the most any surveyed stream needed
_SEG, _DINFO, _SPEC = 6, 8, 273
_DI_HOST = 1


class JpegStreams(_JpegBatch):
    """parse_streams' result for a batch, the input of entropy_decode_device: the streams themselves (`blob` uint8 tensor,
    `offs` int64 [N + 1]), `desc` / `qtabs` / `status` as in JpegCoefficients (from the headers alone: what is wrong inside a
    scan is found when it is decoded), `tables` uint8 [N, 8, 273] (Huffman table specs), `info` int64 [N, 8], `segments`
    int64 [S, 6] = {image, first byte, end byte, first MCU, MCUs, n of the RSTn in front or -1} (one row per restart
    interval), `sub_base` int64 [S + 1], `wgtab` int32 [G, 4] and `coef_elems`.  Layouts: include/dbnet_hip.h.  Picklable."""

    def __init__(self, blob, offs, desc, qtabs, status, tables, info, segments, sub_base, wgtab, coef_elems):
        self.blob, self.offs, self.desc, self.qtabs, self.status = blob, offs, desc, qtabs, status
        self.tables, self.info, self.segments, self.sub_base, self.wgtab, self.coef_elems = tables, info, segments, sub_base, wgtab, int(coef_elems)

    @property
    def host_only(self):
        """bool [N]: scans whose markers are not the ones the header calls for; the host decoder says what is wrong"""
        return self.info[:, _DI_HOST] != 0

    def pin_memory(self):
        if not self.blob.is_pinned():
            self.blob = self.blob.pin_memory()
        return self

    def stream(self, i):
        """the bytes of stream i"""
        return self.blob[int(self.offs[i]):int(self.offs[i + 1])].numpy().tobytes()


def parse_streams(datas, pin=None):
    """Host half of the device entropy stage: the headers of the JPEG byte strings `datas` (the kinds and status codes of
    entropy_decode) and their scans cut into restart intervals at the markers -> JpegStreams.  No bit of the entropy data
    is read.  Runs anywhere, e.g. in a DataLoader worker.  pin: as entropy_decode."""
    blob, offs = _concat_streams(datas, pin_default(pin))
    N = len(offs) - 1
    if N == 0:
        raise ValueError('parse_streams needs at least one stream')
    desc, qtabs, status = np.zeros((N, _DESC), np.int64), np.zeros((N, 3, 64), np.uint16), np.zeros(N, np.int32)
    tables, info, counts = np.zeros((N, 8, _SPEC), np.uint8), np.zeros((N, _DINFO), np.int64), np.zeros(4, np.int64)
    L = lib()
    head = (blob.data_ptr(), offs.ctypes.data, N, desc.ctypes.data, qtabs.ctypes.data, status.ctypes.data, tables.ctypes.data, info.ctypes.data)
    check(L.dbn_jpeg_stream_plan(*head, None, 0, None, None, 0, counts.ctypes.data), 'jpeg_stream_plan')
    nseg, nwg = int(counts[0]), int(counts[2])
    seg, sub_base, wgtab = np.zeros((nseg, _SEG), np.int64), np.zeros(nseg + 1, np.int64), np.zeros((nwg, 4), np.int32)
    one = np.zeros(8, np.int64)  # ctypes has no address for an empty array
    check(L.dbn_jpeg_stream_plan(*head, seg.ctypes.data if nseg else one.ctypes.data, nseg, sub_base.ctypes.data,
                                 wgtab.ctypes.data if nwg else one.ctypes.data, nwg, counts.ctypes.data), 'jpeg_stream_plan')
    return JpegStreams(blob, offs, desc, qtabs, status, tables, info, seg, sub_base, wgtab, counts[3])


def dhuff_workspace_bytes(streams):
    return int(lib().dbn_jpeg_dhuff_ws_bytes(int(streams.sub_base[-1])))


def _dhuff_launch(st, dev, rounds, coef, ws):
    """the launches of dbn_jpeg_dhuff on the current stream of `dev` into coef (int16 [st.coef_elems]) and the workspace ws
    (uint8) -> the result words, still on the device: uint64 [rounds + 2, N] as int64"""
    N = len(st)
    res = torch.empty((rounds + 2) * N, dtype=torch.int64, device=dev)
    blob = st.blob.to(dev, non_blocking=True)
    desc = st.desc.copy()
    desc[:, _D_STATUS] = st.status
    arrs = [upload(a, dev) for a in (desc, st.tables, st.info, st.segments if len(st.segments) else np.zeros((1, _SEG), np.int64), st.sub_base,
                                  st.wgtab if len(st.wgtab) else np.zeros((1, 4), np.int32))]
    check(lib().dbn_jpeg_dhuff(blob.data_ptr(), blob.numel(), *[a.data_ptr() for a in arrs], N, len(st.segments), int(st.sub_base[-1]), len(st.wgtab),
                               rounds, coef.data_ptr(), st.coef_elems, ws.data_ptr(), ws.numel(), res.data_ptr(), stream(dev)), 'jpeg_dhuff')
    return res.view(rounds + 2, N)


def entropy_decode_device(streams, device=None, max_rounds=None):
    """entropy_decode on the device (csrc/jpeg_dhuff.hip): JpegStreams (or JPEG byte strings, parsed here) -> JpegCoefficients
    whose `coef` is a device tensor, the same coefficients, descriptors and status.  Runs on the current stream; the host
    waits once, for one result word per image and launch.  An image the device flagged (damaged data, markers that
    disagree with the header) or that had not reached the fixed point after max_rounds propagation launches (default
    DHUFF_ROUNDS) is decoded by the host decoder alone and uploaded: `host_decoded` names these images, and every status
    is the host decoder's."""
    st = streams if isinstance(streams, JpegStreams) else parse_streams(list(streams))
    rounds = DHUFF_ROUNDS if max_rounds is None else int(max_rounds)
    if not 0 <= rounds <= 64:
        raise ValueError('max_rounds is 0 .. 64, got %r' % (max_rounds, ))
    dev = cuda_device('entropy_decode_device', device)
    N = len(st)
    status, desc = st.status.copy(), st.desc.copy()
    with on_device(dev):
        coef = torch.empty(max(st.coef_elems, 1), dtype=torch.int16, device=dev)
        ws = torch.empty(max(dhuff_workspace_bytes(st), 8), dtype=torch.uint8, device=dev)
        res = _dhuff_launch(st, dev, rounds, coef, ws).cpu().numpy()  # the one wait
        redo = (status == 0) & (st.host_only | (res[0] != -1) | (res[rounds + 1] != 0))
        idx = np.nonzero(redo)[0]
        if idx.size:
            sub = entropy_decode([st.stream(i) for i in idx], pin=False)
            for k, i in enumerate(idx):
                o, e = int(sub.desc[k, _D_COEF]), int(desc[i, _D_COEF])
                n = int(sub.desc[k + 1, _D_COEF]) if k + 1 < len(idx) else sub.coef.numel()
                coef[e:e + n - o].copy_(sub.coef[o:n], non_blocking=False)
                status[i] = sub.status[k]
    desc[:, _D_STATUS] = status
    obj = JpegCoefficients(coef[:st.coef_elems], desc, st.qtabs.copy(), status)
    obj.host_decoded = redo
    return obj


def jpeg_stream_collate(items):
    """jpeg_collate for the device entropy stage: the worker only parses (parse_streams) -> (JpegStreams, shapes, polys,
    tags); DeviceBatches.convert runs the Huffman stage and the pixel stage on the device.  A header that cannot be decoded
    raises here; a damaged scan raises in convert."""
    obj = parse_streams([b[0] for b in items])
    obj.raise_errors()
    return (obj, obj.shapes) + polys_tags(items)


# ---- encode ----------------------------------------------------------------------------------------------------------
SUBSAMPLING = {'444': (1, 1), '422': (2, 1), '420': (2, 2)}
PLANE_CELLS, FDCT_BLOCKS = 256, 32  # per workgroup (csrc/jpeg_enc.hip)
ENCODE_REASONS = {
    1: 'the image was not decoded, there are no coefficients to code', 2: 'descriptor and coefficient buffer disagree',
    3: 'a quantisation value lies outside 1 .. 255', 4: 'a DC difference needs more than 11 bits: not baseline-codable',
    5: 'an AC coefficient needs more than 10 bits: not baseline-codable', 6: 'the output slot is too small',
    7: 'the optimised Huffman code would need more than 32 bits before limiting: libjpeg refuses it too',
}
# Annex K.1 / K.2, natural order
_BASE_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
              18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
              103, 99)
_BASE_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99,
                99) + (99, ) * 32


class JpegEncodeError(ValueError):
    """an image that was not encoded: .index its place in the batch, .code the status of dbn_jpeg_encode_batch, .reason"""

    def __init__(self, index, reason, code=None):
        self.index, self.reason, self.code = index, reason, code
        ValueError.__init__(self, 'image %d: %s' % (index, reason))


def quant_tables(quality):
    """libjpeg's jpeg_set_quality(quality, force_baseline): the Annex K luma and chroma tables scaled by 5000 / q (q < 50) or
    200 - 2 q percent, rounded, clamped to 1 .. 255 -> uint16 [2, 64] in natural order.  quality: 1 .. 100."""
    if isinstance(quality, bool) or int(quality) != quality or not 1 <= int(quality) <= 100:
        raise ValueError('quality must be an integer in 1 .. 100, got %r' % (quality, ))
    q = int(quality)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    base = np.array([_BASE_LUMA, _BASE_CHROMA], np.int64)
    return np.clip((base * scale + 50) // 100, 1, 255).astype(np.uint16)


def _tables(quality, qtables):
    if qtables is None:
        return quant_tables(quality)
    t = np.asarray(qtables)
    if t.dtype.kind not in 'iu' or t.ndim != 2 or t.shape[1] != 64 or not 1 <= t.shape[0] <= 3 or t.min() < 1 or t.max() > 255:
        raise ValueError('qtables must be 1 to 3 integer tables of 64 values in 1 .. 255 (natural order)')
    return t.astype(np.uint16)


def encode_inputs(images, shapes, dev):
    """the layouts the encoders take -> (uint8 1-D device tensor, [(byte offset, H, W, components)])"""
    if shapes is not None:
        if not (isinstance(images, torch.Tensor) and images.dim() == 1):
            raise ValueError('with shapes, images is the packed 1-D uint8 batch')
        items, o = [], 0
        for h, w in shapes:
            items.append((o, int(h), int(w), 3))
            o += int(h) * int(w) * 3
        check_bytes(images.numel(), o)
        flat = flat_u8(images, dev)
    elif isinstance(images, (list, tuple)):
        parts, items, o = [], [], 0
        for a in images:
            if a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
                raise ValueError('an image of a list is uint8 [H, W] or [H, W, 3], got %s' % (tuple(a.shape), ))
            nc = 1 if a.ndim == 2 else 3
            parts.append(flat_u8(a, dev))
            items.append((o, int(a.shape[0]), int(a.shape[1]), nc))
            o += parts[-1].numel()
        if not parts:
            raise ValueError('no images')
        flat = parts[0] if len(parts) == 1 else torch.cat(parts)
    else:
        a = images
        nd, sh = a.ndim, tuple(int(v) for v in a.shape)
        if nd == 2:
            n, h, w, nc = 1, sh[0], sh[1], 1
        elif nd == 3 and sh[2] == 3:  # one RGB image (a grey stack of width 3 goes in as a list)
            n, h, w, nc = 1, sh[0], sh[1], 3
        elif nd == 3:
            n, h, w, nc = sh[0], sh[1], sh[2], 1
        elif nd == 4 and sh[3] == 3:
            n, h, w, nc = sh[0], sh[1], sh[2], 3
        else:
            raise ValueError('images must be uint8 [H, W], [N, H, W], [H, W, 3] or [N, H, W, 3], got %s' % (sh, ))
        if n < 1:
            raise ValueError('no images')
        items = [(i * h * w * nc, h, w, nc) for i in range(n)]
        flat = flat_u8(a, dev)
    for _, h, w, _ in items:
        if not (1 <= h <= 65535 and 1 <= w <= 65535):
            raise ValueError('a JPEG image is 1 .. 65535 pixels on a side, got %d x %d' % (h, w))
    return flat, items


def _expand(counts):
    """counts [K] -> (owner of each of the sum(counts) entries, its index within the owner)"""
    counts = np.asarray(counts, np.int64)
    owner = np.repeat(np.arange(len(counts)), counts)
    return owner, np.arange(int(counts.sum())) - np.repeat(np.cumsum(counts) - counts, counts)


def forward_plan(items, subsampling, tables):
    """host: the descriptors, tables and work tables of dbn_jpeg_forward for images (offset, H, W, components) ->
    (desc int64 [N, 24] with the input byte offset in field 4, qtabs uint16 [N, 3, 64], coefficient count,
    int32 [n_planes, 4] {image, chunk of 256 cells}, int32 [n_fdct, 4] {image, component, first block})"""
    if subsampling not in SUBSAMPLING:
        raise ValueError("subsampling is '444', '422' or '420', got %r" % (subsampling, ))
    it = np.asarray(items, np.int64).reshape(-1, 4)
    N = len(it)
    off, H, W, nc = it[:, 0], it[:, 1], it[:, 2], it[:, 3]
    hs = np.where(nc == 3, SUBSAMPLING[subsampling][0], 1)
    vs = np.where(nc == 3, SUBSAMPLING[subsampling][1], 1)
    mcux, mcuy = -(-W // (8 * hs)), -(-H // (8 * vs))
    desc = np.zeros((N, _DESC), np.int64)
    desc[:, _D_W], desc[:, _D_H], desc[:, _D_NC], desc[:, _D_OUT], desc[:, _D_QT] = W, H, nc, off, np.arange(N) * 192
    blocks = np.zeros((N, 3), np.int64)
    for c in range(3):
        on = nc > c
        h, v = (hs, vs) if c == 0 else (1, 1)
        desc[:, _D_COMP + 4 * c] = np.where(on, mcux * h, 0)
        desc[:, _D_COMP + 4 * c + 1] = np.where(on, mcuy * v, 0)
        desc[:, _D_COMP + 4 * c + 2] = np.where(on, h, 0)
        desc[:, _D_COMP + 4 * c + 3] = np.where(on, v, 0)
        blocks[:, c] = np.where(on, mcux * h * mcuy * v, 0)
    desc[:, 18], desc[:, 19], desc[:, 20], desc[:, 21] = hs, vs, mcux, mcuy
    per = blocks.sum(1) * 64
    desc[:, _D_COEF] = np.cumsum(per) - per
    qtabs = np.zeros((N, 3, 64), np.uint16)
    for c in range(3):
        qtabs[nc > c, c] = tables[min(c, len(tables) - 1)]
    n, chunk = _expand(-(-(mcux * 8 * mcuy * 8) // PLANE_CELLS))
    tp = np.zeros((len(n), 4), np.int32)
    tp[:, 0], tp[:, 1] = n, chunk
    k, first = _expand(-(-blocks.reshape(-1) // FDCT_BLOCKS))
    tf = np.zeros((len(k), 4), np.int32)
    tf[:, 0], tf[:, 1], tf[:, 2] = k // 3, k % 3, first * FDCT_BLOCKS
    return desc, qtabs, int(per.sum()), tp, tf


def forward_coefficients(images, shapes=None, quality=75, subsampling='420', qtables=None, device=None, host_copy=True):
    """Device half of the encode: uint8 images -> JpegCoefficients, libjpeg's quantised coefficients over the MCU-padded grid
    (dummy blocks as libjpeg codes them), copied into pinned host memory on the current stream; no host synchronisation
    (the result's wait() blocks until they have arrived; entropy_encode and decode_coefficients order themselves after it).

    images: the packed 1-D uint8 RGB batch with shapes [(H, W)] (decode_jpeg_batch's output, augment_images' input); or
    uint8 [H, W, 3] / [N, H, W, 3] RGB; or uint8 [H, W] / [N, H, W] grey (a one-component stream); or a list of [H, W, 3]
    and [H, W] images of any sizes.  Tensors or arrays, on the host or the device.  A 3-D input whose last extent is 3 is
    one RGB image.  quality 1 .. 100 (quant_tables) or qtables: 1 to 3 tables [64] in natural order, values 1 .. 255, for
    luma, Cb and Cr (the last one given serves the remaining components).  subsampling '444' | '422' | '420' for RGB.
    host_copy=False: the coefficients stay on the device (`coef.is_cuda`; no pinned buffer, no copy), for
    entropy_encode_device and decode_coefficients."""
    tables = _tables(quality, qtables)
    dev = cuda_device('forward_coefficients', device, images)
    with on_device(dev) as sh:
        flat, items = encode_inputs(images, shapes, dev)
        hdesc, qtabs, total, tp, tf = forward_plan(items, subsampling, tables)
        desc, qt, a, b = upload(hdesc, dev), upload(qtabs.view(np.int16), dev), upload(tp, dev), upload(tf, dev)
        coef = torch.empty(total, dtype=torch.int16, device=dev)
        planes = torch.empty(total, dtype=torch.uint8, device=dev)
        check(lib().dbn_jpeg_forward(flat.data_ptr(), flat.numel(), desc.data_ptr(), qt.data_ptr(), len(items), a.data_ptr(), len(tp),
                                     b.data_ptr(), len(tf), planes.data_ptr(), coef.data_ptr(), total, sh), 'jpeg_forward')
        if host_copy:
            host = torch.empty(total, dtype=torch.int16, pin_memory=True)
            host.copy_(coef, non_blocking=True)
        else:
            host = coef
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(dev))
    hdesc[:, _D_OUT] = np.cumsum(hdesc[:, _D_W] * hdesc[:, _D_H] * 3) - hdesc[:, _D_W] * hdesc[:, _D_H] * 3  # as entropy_decode leaves it
    obj = JpegCoefficients(host, hdesc, qtabs, np.zeros(len(items), np.int32))
    obj.ready = ready
    return obj


def optimal_huffman_table(freq):
    """256 symbol counts -> (counts uint8 [16]: symbols per code length 1 .. 16, symbols uint8 [n] by length, then value): the
    table libjpeg's jpeg_gen_optimal_table builds (a pseudo-symbol of count 1 keeps the all-ones code free, ties go to the
    larger symbol, lengths are limited to 16), which is the payload of a DHT segment Pillow writes with optimize=True."""
    f = np.asarray(freq)
    if f.shape != (256, ) or f.dtype.kind not in 'iu' or f.min() < 0 or not f.any():
        raise ValueError('freq is 256 non-negative integer counts, not all of them 0')
    f = np.ascontiguousarray(f, np.int64)
    bits, vals, n = np.zeros(16, np.uint8), np.zeros(256, np.uint8), np.zeros(1, np.int32)
    check(lib().dbn_jpeg_optimal_table(f.ctypes.data, bits.ctypes.data, vals.ctypes.data, n.ctypes.data), 'jpeg_optimal_table')
    return bits, vals[:int(n[0])].copy()


def _check_encode_args(restart_interval, errors):
    if errors not in ('raise', 'report'):
        raise ValueError("errors is 'raise' or 'report'")
    if isinstance(restart_interval, bool) or int(restart_interval) != restart_interval or not 0 <= int(restart_interval) <= 65535:
        raise ValueError('restart_interval must be an integer in 0 .. 65535, got %r' % (restart_interval, ))
    return int(restart_interval)


def _encode_result(streams, status, errors):
    errs = [None if s == 0 else JpegEncodeError(i, ENCODE_REASONS.get(int(s), 'status %d' % s), int(s)) for i, s in enumerate(status)]
    if errors == 'raise':
        for e in errs:
            if e is not None:
                raise e
    streams = [None if e is not None else d for d, e in zip(streams, errs)]
    return streams if errors == 'raise' else (streams, errs)


def entropy_encode_device(obj, restart_interval=0, optimize=False, errors='raise', device=None):
    """entropy_encode on the device (csrc/jpeg_huff.hip): the same byte strings, the same errors.  obj: a JpegCoefficients
    whose coefficients are on the device (forward_coefficients(..., host_copy=False)) or on the host (they are uploaded:
    entropy_encode_device(entropy_decode(datas)) transcodes without the DCT kernels).  The kernels run on the current
    stream; the host waits once, for the lengths, and then copies the streams' own bytes.  optimize=True adds one round
    trip before that: the per-image symbol histograms come to the host, which builds the tables."""
    ri, N = _check_encode_args(restart_interval, errors), len(obj)
    if N == 0:
        raise ValueError('entropy_encode_device needs at least one image')
    desc = np.ascontiguousarray(obj.desc, np.int64).copy()
    desc[:, _D_STATUS] = np.asarray(obj.status)
    qtabs = np.ascontiguousarray(obj.qtabs, np.uint16)
    if obj.coef.dtype != torch.int16 or desc.shape != (N, _DESC) or qtabs.shape != (N, 3, 64):
        raise ValueError('not the layout of JpegCoefficients')
    dev = cuda_device('entropy_encode_device', device, obj.coef)
    L = lib()
    blk, ivl = np.zeros(N + 1, np.int64), np.zeros(N + 1, np.int64)
    status, sizes = np.zeros(N, np.int32), np.zeros(2, np.int64)
    check(L.dbn_jpeg_huff_plan(desc.ctypes.data, qtabs.ctypes.data, N, obj.coef.numel(), ri, blk.ctypes.data, ivl.ctypes.data,
                               status.ctypes.data, sizes.ctypes.data), 'jpeg_huff_plan')
    total, intervals = int(blk[N]), int(ivl[N])
    specs, codes = np.zeros((N if optimize else 1, 4, 273), np.uint16), np.zeros((N if optimize else 1, 4, 256), np.uint32)
    scans = [b''] * N
    if total:
        with on_device(dev) as sh:
            if obj.ready is not None:
                torch.cuda.current_stream(dev).wait_event(obj.ready)
            coef = obj.coef.contiguous().to(dev, non_blocking=True)
            ddesc, dblk, divl = upload(desc, dev), upload(blk, dev), upload(ivl, dev)
            res = torch.full((2 * N + 1, ), -1, dtype=torch.int64, device=dev)
            if optimize:
                hist = torch.empty((N, 4, 256), dtype=torch.int32, device=dev)
                check(L.dbn_jpeg_huff_hist(coef.data_ptr(), coef.numel(), ddesc.data_ptr(), N, dblk.data_ptr(), total, ri, hist.data_ptr(),
                                           res.data_ptr(), sh), 'jpeg_huff_hist')
                hhist = hist.cpu().numpy().view(np.uint32)  # the one host step between launches
                check(L.dbn_jpeg_huff_tables(hhist.ctypes.data, desc.ctypes.data, N, status.ctypes.data, specs.ctypes.data, codes.ctypes.data,
                                             MAX_THREADS), 'jpeg_huff_tables')
            else:
                check(L.dbn_jpeg_huff_annex_k(specs.ctypes.data, codes.ctypes.data), 'jpeg_huff_annex_k')
            dcodes = upload(codes.view(np.int32), dev)
            ws = torch.empty(int(sizes[0]), dtype=torch.uint8, device=dev)
            out = torch.empty(int(sizes[1]), dtype=torch.uint8, device=dev)
            check(L.dbn_jpeg_huff_code(coef.data_ptr(), coef.numel(), ddesc.data_ptr(), N, dblk.data_ptr(), divl.data_ptr(), total, intervals, ri,
                                       dcodes.data_ptr(), int(bool(optimize)), ws.data_ptr(), ws.numel(), out.data_ptr(), out.numel(),
                                       res.data_ptr(), sh), 'jpeg_huff_code')
            hres = res.cpu().numpy().view(np.uint64)  # the one wait: error keys and offsets
            offs = hres[N:].astype(np.int64)
            if not (np.all(np.diff(offs) >= 0) and 0 <= offs[0] and offs[N] <= out.numel()):
                raise RuntimeError('libdbnet_hip: jpeg_huff_code returned offsets outside its buffer')
            blob = out[int(offs[0]):int(offs[N])].cpu().numpy()
            blob = blob.tobytes()
        bad = hres[:N] != np.uint64(0xFFFFFFFFFFFFFFFF)
        status = np.where((status == 0) & bad, (hres[:N] & np.uint64(7)).astype(np.int32), status).astype(np.int32)
        o0 = int(offs[0])
        scans = [blob[int(a) - o0:int(b) - o0] for a, b in zip(offs[:-1], offs[1:])]
    heads, hlens = np.zeros((N, 704), np.uint8), np.zeros(N, np.int64)
    check(L.dbn_jpeg_huff_headers(desc.ctypes.data, qtabs.ctypes.data, N, ri, specs.ctypes.data, int(bool(optimize)), status.ctypes.data,
                                  heads.ctypes.data, hlens.ctypes.data), 'jpeg_huff_headers')
    streams = [heads[n, :int(hlens[n])].tobytes() + scans[n] + b'\xff\xd9' if status[n] == 0 else None for n in range(N)]
    return _encode_result(streams, status, errors)


def entropy_encode(obj, restart_interval=0, threads=MAX_THREADS, errors='raise', optimize=False):
    """Host half of the encode: JpegCoefficients -> list of JPEG byte strings (SOI, JFIF APP0, DQT, SOF0, DHT, DRI, SOS, one
    interleaved scan with the Annex K Huffman tables, EOI), on min(len(obj), 16, threads) threads.  Coefficients are
    taken as given, dummy blocks included: entropy_encode(entropy_decode(data), restart_interval=that stream's) reproduces
    the scan bytes of a stream that uses the Annex K tables.  restart_interval: MCUs between RSTn markers, 0 .. 65535.
    An image that cannot be coded raises JpegEncodeError(index, reason); errors='report': nothing raises; ->
    (streams, errs) with streams[i] None and errs[i] the exception for such an image, which fails alone.
    optimize=True: every image is walked twice and carries its own Huffman tables, the ones libjpeg's optimize_coding
    (Pillow's optimize=True) builds, in its four DHT segments (two for grey); everything else in the stream is unchanged."""
    ri, N = _check_encode_args(restart_interval, errors), len(obj)
    if N == 0:
        raise ValueError('entropy_encode needs at least one image')
    if obj.coef.is_cuda:
        raise ValueError('the coefficients are on the device (host_copy=False): entropy_encode_device codes them there')
    obj.wait()
    coef = obj.coef.contiguous()
    desc = np.ascontiguousarray(obj.desc, np.int64).copy()
    desc[:, _D_STATUS] = np.asarray(obj.status)
    qtabs = np.ascontiguousarray(obj.qtabs, np.uint16)
    if coef.dtype != torch.int16 or coef.is_cuda or desc.shape != (N, _DESC) or qtabs.shape != (N, 3, 64):
        raise ValueError('not the layout of JpegCoefficients')
    L = lib()
    per = np.zeros(N, np.int64)
    total = int(L.dbn_jpeg_encode_bound(desc.ctypes.data, N, ri, per.ctypes.data))
    if total < 0:
        raise RuntimeError('libdbnet_hip: jpeg_encode_bound failed')
    offs = offsets(per)
    out = np.empty(max(total, 1), np.uint8)  # the worst case; only the pages a stream reaches are ever touched
    lens, status = np.zeros(N, np.int64), np.zeros(N, np.int32)
    check(L.dbn_jpeg_encode_batch_opt(coef.data_ptr(), coef.numel(), desc.ctypes.data, qtabs.ctypes.data, N, ri, out.ctypes.data, total,
                                      offs.ctypes.data, lens.ctypes.data, status.ctypes.data, int(threads), int(bool(optimize))), 'jpeg_encode_batch')
    return _encode_result([out[o:o + n].tobytes() for o, n in zip(offs[:-1], lens)], status, errors)


def encode_jpeg_batch(images, shapes=None, quality=75, subsampling='420', qtables=None, restart_interval=0, threads=MAX_THREADS, device=None,
                      optimize=False, entropy='host'):
    """uint8 images (the layouts of forward_coefficients) -> list of baseline JPEG byte strings.  The defaults are Pillow's /
    imageio's (quality 75, 4:2:0, the Annex K Huffman tables): the file decodes to the pixels of the file the reference's
    imageio.imwrite(path, img) writes.  optimize=True: each image's own Huffman tables (Pillow's optimize=True).
    entropy='host' codes on the host threads, 'device' on the GPU (no coefficient crosses to the host); the bytes are the same."""
    if entropy not in ('host', 'device'):
        raise ValueError("entropy is 'host' or 'device', got %r" % (entropy, ))
    if entropy == 'device':
        obj = forward_coefficients(images, shapes, quality, subsampling, qtables, device, host_copy=False)
        return entropy_encode_device(obj, restart_interval, optimize)
    return entropy_encode(forward_coefficients(images, shapes, quality, subsampling, qtables, device), restart_interval, threads, optimize=optimize)


def encode_jpeg(image, quality=75, subsampling='420', qtables=None, restart_interval=0, device=None, optimize=False, entropy='host'):
    """one uint8 [H, W, 3] (or grey [H, W]) image -> bytes"""
    if getattr(image, 'ndim', 0) not in (2, 3) or (image.ndim == 3 and image.shape[2] != 3):
        raise ValueError('encode_jpeg takes one uint8 [H, W, 3] or [H, W] image')
    return encode_jpeg_batch([image], None, quality, subsampling, qtables, restart_interval, 1, device, optimize, entropy)[0]


def save_jpegs(paths, images, shapes=None, **kw):
    """encode_jpeg_batch(images, shapes, **kw) written to `paths`, one file per image: the reference's per-crop
    word_<i>.jpg loop (test_ocr.py:176, utils.py:272) for crop_words' [M, 32, 100, 3] output in one call -> the paths"""
    paths = [os.fspath(p) for p in paths]
    datas = encode_jpeg_batch(images, shapes, **kw)
    if len(paths) != len(datas):
        raise ValueError('%d paths for %d images' % (len(paths), len(datas)))
    for p, d in zip(paths, datas):
        with open(p, 'wb') as f:
            f.write(d)
    return paths
