"""PNG at both ends of the device pipeline, in the shape of jpeg.py: the serial entropy stage on the host, the pixels on the GPU.
Decode stands in the place of the reference's cv2.imread(path)[:, :, ::-1] (data_loaders.py:78, utils.py:179) for the other
everyday format; encode in the place of its imageio / matplotlib writes, and is the lossless container for the probability
and binary maps.  zlib's inflate and deflate are serial per stream and run on host threads (Python's zlib releases the GIL);
undoing the five scanline filters, Adam7 de-interlacing, bit-depth, palette and colour conversion and the packing are gfx950
kernels (csrc/png.hip), as are the encoder's filter choice and application.

  png_info(data)                           -> dict (width, height, bit_depth, colour_type, interlace, channels, status, supported, reason)
  inflate_png(datas)                       -> PngScanlines (host half; runs anywhere, e.g. in a DataLoader worker)
  unfilter_png(obj, device)                -> (packed uint8 device tensor, shapes) (device half)
  decode_png_batch(datas, device)          -> (packed, shapes): what augment_images(packed, shapes, plans) takes
  decode_png(data, device)                 -> uint8 [H, W, 3] device tensor
  png_collate(items)                       collate_fn for items (png bytes, polys, tags); DeviceBatches.convert runs the device half
  decode_image_batch(datas, device)        a mixed list of JPEG and PNG byte strings -> one packed batch in the callers' order
  filter_png_rows(images, ...)             -> per image uint8 [H, 1 + W * C]: the filtered scanlines, type bytes included (device half)
  encode_png_batch(images, ...)            -> [bytes]; encode_png(image, ...) -> bytes; save_pngs(paths, images, ...) writes files

What a decoded pixel is: cv2.imread's IMREAD_COLOR rule, given as RGB.  The output is always 8-bit, 3 channels.  Grey is
replicated into the three channels; 1-, 2- and 4-bit grey is scaled by 255 / (2^depth - 1) (x255, x85, x17).  Palette indices are
looked up in PLTE, an index past its end giving black.  Alpha is dropped, not composited; tRNS, gAMA, sRGB and iCCP are
ignored.  16-bit samples give their high byte.  Adam7 files decode to the pixels of their non-interlaced form.  All 15 valid
colour-type / depth pairs are taken.  Pinned against Pillow, which gives these pixels for every kind but 16-bit grey without
alpha (there it clips, and the high byte of its raw image is the pin): tests/golden/png_cases.npz.

Limits: each side at most 65535 pixels and the inflated scanlines of one image below 2^31 bytes; a larger image raises
UnsupportedPng, as does Apple's CgBI variant.  Everything else that cannot be decoded raises CorruptPng: a bad signature, a
chunk that runs past the end or fails its CRC, a zero dimension, an invalid colour-type / depth pair, a zlib error, fewer
scanline bytes than IHDR implies (surplus ones are ignored, as libpng does), a filter-type byte above 4, and a missing IEND
(stricter than cv2, which reads such a file when its data is complete).  Only the default image of an APNG is decoded.

Written files are 8-bit, colour type 2 (RGB) or 0 (grey), non-interlaced: IHDR, one IDAT, IEND and nothing else.
"""
import os
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from ._lib import check, lib
from .jpeg import MAX_THREADS, decode_jpeg_batch, encode_inputs, splice_images
from .jpeg import pil_rgb as _pil_rgb  # called through this module's name, where tests patch it
from .packed import MAX_SIDE, DecodedBatch, DecodeError, cuda_device, image_offsets, on_device, pin_default, polys_tags, upload

SIGNATURE = b'\x89PNG\r\n\x1a\n'
_DESC = 32  # int64 fields per image (include/dbnet_hip.h)
_D_W, _D_H, _D_DEPTH, _D_CTYPE, _D_LACE, _D_OUT, _D_NPAL, _D_STATUS, _D_SRC, _D_RAW = 0, 1, 2, 3, 4, 5, 6, 7, 8, 16
_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
_DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}
_ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))  # x0, y0, dx, dy of passes 1 .. 7
UNFILTER_ROWS, UNFILTER_CHUNK = 256, 16  # rows of a band, bytes of a chunk (csrc/png.hip)
MAX_RAW = (1 << 31) - 1
_BLOB_PAD = 32  # bytes allocated past the blob's end: the unfilter kernel reads whole aligned words

REASONS = {
    1: 'not a PNG stream', 2: 'truncated: a chunk runs past the end of the data', 3: 'a chunk fails its CRC',
    4: 'IHDR is missing, not first, or holds a zero dimension, an invalid colour type / bit depth pair or an unknown method',
    5: 'PLTE is malformed or missing in a palette image, or there is no IDAT chunk', 6: 'the zlib stream is damaged', 7: 'fewer scanline bytes than IHDR implies',
    8: 'a filter-type byte above 4', 9: 'IEND is missing', 20: "Apple's CgBI variant is not supported",
    21: 'the image is larger than 65535 pixels on a side or 2^31 - 1 scanline bytes',
}
_REFUSED = (20, 21)


class PngError(DecodeError):
    """a file that was not decoded: .code is the status (REASONS), .index the image's place in its batch"""
    reasons, refused = REASONS, _REFUSED


class UnsupportedPng(PngError):
    """a kind of PNG this decoder refuses (CgBI, larger than the limits); another decoder may take it"""


class CorruptPng(PngError):
    """not a PNG, or one that is truncated or damaged"""


PngError.unsupported, PngError.corrupt = UnsupportedPng, CorruptPng


class _Fail(Exception):
    def __init__(self, code):
        self.code = code


def _chunks(data):
    """the chunks of a PNG byte string, every CRC checked: yields (type, body)"""
    if bytes(data[:8]) != SIGNATURE:
        raise _Fail(1)
    pos, n = 8, len(data)
    while pos < n:
        if pos + 12 > n:
            raise _Fail(2)
        size, kind = struct.unpack_from('>I4s', data, pos)
        if pos + 12 + size > n:
            raise _Fail(2)
        if zlib.crc32(data[pos + 4:pos + 8 + size]) != struct.unpack_from('>I', data, pos + 8 + size)[0]:
            raise _Fail(3)
        yield kind, data[pos + 8:pos + 8 + size]
        pos += 12 + size


def _ihdr(body):
    if len(body) != 13:
        raise _Fail(4)
    w, h, depth, ctype, comp, flt, lace = struct.unpack('>IIBBBBB', body)
    if w == 0 or h == 0 or depth not in _DEPTHS.get(ctype, ()) or comp or flt or lace > 1:
        raise _Fail(4)
    return w, h, depth, ctype, lace


def _subimages(w, h, bits, lace):
    """[(slot, pass width, pass height, row bytes)] of the sub-images that hold bytes: slot 0 is the image itself, 1 .. 7 the Adam7 passes"""
    if not lace:
        return [(0, w, h, (w * bits + 7) // 8)]
    out = []
    for s, (x0, y0, dx, dy) in enumerate(_ADAM7):
        pw, ph = (w - x0 + dx - 1) // dx, (h - y0 + dy - 1) // dy
        if pw > 0 and ph > 0:
            out.append((s + 1, pw, ph, (pw * bits + 7) // 8))
    return out


def png_info(data):
    """IHDR of one file, without inflating it: dict(width, height, bit_depth, colour_type, interlace, channels, status, supported,
    reason).  Host only."""
    data = memoryview(data).cast('B') if not isinstance(data, (bytes, bytearray)) else data
    w = h = depth = ctype = lace = 0
    status = 0
    try:
        for kind, body in _chunks(data):
            if kind == b'CgBI':
                raise _Fail(20)
            if kind != b'IHDR':
                raise _Fail(4)
            w, h, depth, ctype, lace = _ihdr(bytes(body))
            if w > MAX_SIDE or h > MAX_SIDE or sum(ph * (rb + 1) for _, _, ph, rb in _subimages(w, h, depth * _CHANNELS[ctype], lace)) > MAX_RAW:
                raise _Fail(21)
            break
        else:
            raise _Fail(4)
    except _Fail as e:
        status = e.code
    return dict(width=w, height=h, bit_depth=depth, colour_type=ctype, interlace=bool(lace), channels=_CHANNELS.get(ctype, 0), status=status,
                supported=status == 0, reason=None if status == 0 else REASONS[status])


def _inflate_one(data):
    """-> (status, (w, h, depth, ctype, lace), palette uint8 [n, 3] or None, the filtered scanlines as bytes)"""
    data = bytes(data) if not isinstance(data, (bytes, bytearray)) else data
    hdr, pal, end, need, got, z = None, None, False, 0, [], None
    try:
        for kind, body in _chunks(memoryview(data)):
            if kind == b'CgBI':
                raise _Fail(20)
            if hdr is None:
                if kind != b'IHDR':
                    raise _Fail(4)
                hdr = _ihdr(bytes(body))
                w, h, depth, ctype, lace = hdr
                subs = _subimages(w, h, depth * _CHANNELS[ctype], lace)
                need = sum(ph * (rb + 1) for _, _, ph, rb in subs)
                if w > MAX_SIDE or h > MAX_SIDE or need > MAX_RAW:
                    raise _Fail(21)
                left, z = need, zlib.decompressobj()
            elif kind == b'IHDR':
                raise _Fail(4)
            elif kind == b'PLTE':
                if len(body) % 3 or not 3 <= len(body) <= 768:
                    raise _Fail(5)
                pal = np.frombuffer(bytes(body), np.uint8).reshape(-1, 3)
            elif kind == b'IDAT':
                if left > 0 and len(body):  # never more than IHDR implies: a crafted stream allocates nothing past it
                    try:
                        piece = z.decompress(body, left)
                    except zlib.error:
                        raise _Fail(6)
                    left -= len(piece)
                    got.append(piece)
                got.append(b'')
            elif kind == b'IEND':
                end = True
                break
        if hdr is None:
            raise _Fail(4)
        if not end:
            raise _Fail(9)
        if not got or (hdr[3] == 3 and pal is None):
            raise _Fail(5)
        if left > 0:
            raise _Fail(7)
        raw = b''.join(got)
        view, o = np.frombuffer(raw, np.uint8), 0
        for _, _, ph, rb in subs:
            if view[o:o + ph * (rb + 1):rb + 1].max() > 4:
                raise _Fail(8)
            o += ph * (rb + 1)
        return 0, hdr, pal, raw
    except _Fail as e:
        return e.code, hdr, None, b''


class PngScanlines(DecodedBatch):
    """The host half's result for a batch: `blob` uint8 tensor, the still filtered scanlines of every image end to end (pinned when
    asked for; 32 spare bytes behind them), `blob_len` their count, `desc` int64 [N, 32] (width, height, bit depth, colour type,
    interlace, output offset, palette entries, status, and per sub-image the offsets in the blob and in the device workspace:
    include/dbnet_hip.h), `palettes` uint8 [N, 256, 3], `status` int32 [N] (0: inflated), `subs` int32 [S, 2] (image, sub-image: one
    workgroup each), `raw_bytes` the workspace the device half needs.  Picklable; pin_memory() makes it what a DataLoader with
    pin_memory=True hands on."""
    error, _hw = PngError, (_D_H, _D_W)

    def __init__(self, blob, blob_len, desc, palettes, status, subs, raw_bytes):
        self.blob, self.blob_len, self.desc, self.palettes, self.status = blob, int(blob_len), desc, palettes, status
        self.subs, self.raw_bytes = subs, int(raw_bytes)

    def pin_memory(self):
        if not self.blob.is_pinned():
            self.blob = self.blob.pin_memory()
        return self


def inflate_png(datas, threads=MAX_THREADS, pin=None):
    """Host half: the PNG byte strings `datas` -> PngScanlines, on min(len(datas), 16, threads) threads.  Per file: the signature,
    every chunk's CRC, IHDR and PLTE are read, the IDAT chunks are inflated one after another (zlib.decompressobj), never past the
    size IHDR implies; tRNS and every other ancillary chunk are skipped, APNG's acTL / fcTL / fdAT among them (only the default
    image is decoded).  Fewer bytes than IHDR implies, or a filter-type byte above 4, is CorruptPng; surplus bytes are ignored.
    A file that fails is reported in .status and fails alone.  The limits: each side <= 65535 pixels, scanlines < 2^31 bytes
    (UnsupportedPng).  pin: pinned blob memory; default when a GPU is visible and this is not a DataLoader worker."""
    datas = list(datas)
    N = len(datas)
    if N == 0:
        raise ValueError('inflate_png needs at least one stream')
    workers = max(1, min(N, MAX_THREADS, int(threads)))
    if workers == 1:
        res = [_inflate_one(d) for d in datas]
    else:
        with ThreadPoolExecutor(workers) as pool:
            res = list(pool.map(_inflate_one, datas))
    desc, palettes, status = np.zeros((N, _DESC), np.int64), np.zeros((N, 256, 3), np.uint8), np.zeros(N, np.int32)
    subs, src, raw, out = [], 0, 0, 0
    for n, (st, hdr, pal, data) in enumerate(res):
        status[n] = st
        desc[n, _D_STATUS], desc[n, _D_OUT] = st, out
        if st:
            continue
        w, h, depth, ctype, lace = hdr
        desc[n, :5] = w, h, depth, ctype, lace
        if pal is not None:
            palettes[n, :len(pal)] = pal
            desc[n, _D_NPAL] = len(pal)
        for slot, _, ph, rb in _subimages(w, h, depth * _CHANNELS[ctype], lace):
            desc[n, _D_SRC + slot], desc[n, _D_RAW + slot] = src, raw
            subs.append((n, slot))
            src += ph * (rb + 1)
            raw += ph * (-(-rb // UNFILTER_CHUNK) * UNFILTER_CHUNK)
        out += h * w * 3
    blob = torch.empty(src + _BLOB_PAD, dtype=torch.uint8, pin_memory=pin_default(pin))
    view = blob.numpy()
    view[src:] = 0
    o = 0
    for st, _, _, data in res:
        if st == 0:
            need = len(data)
            view[o:o + need] = np.frombuffer(data, np.uint8)
            o += need
    return PngScanlines(blob, src, desc, palettes, status, np.array(subs, np.int32).reshape(-1, 2), raw)


def unfilter_png(obj, device=None, _raw=None):
    """Device half: PngScanlines -> (packed uint8 device tensor, shapes), on the current stream of `device`, no host sync: one
    upload of the blob and the tables, the unfilter launch (one workgroup per sub-image), the pixel launch.  Images whose status
    is not 0 take no bytes and have shape (0, 0) (see obj.errors()).  _raw: a workspace of obj.raw_bytes to use (tests)."""
    dev = cuda_device('unfilter_png', device)
    shapes = obj.shapes
    out_bytes = int(image_offsets(shapes)[-1])
    out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
    if out_bytes == 0:
        return out, shapes
    hdesc, hsubs = np.ascontiguousarray(obj.desc, np.int64), np.ascontiguousarray(obj.subs, np.int32)
    L = lib()
    check(L.dbn_png_check(hdesc.ctypes.data, len(obj), hsubs.ctypes.data, len(hsubs), obj.blob_len, obj.raw_bytes, out_bytes), 'png_check')
    with on_device(dev) as stream:
        blob = obj.blob.to(dev, non_blocking=True)
        desc, subs, pal = upload(hdesc, dev), upload(hsubs, dev), upload(obj.palettes, dev)
        raw = torch.empty(obj.raw_bytes, dtype=torch.uint8, device=dev) if _raw is None else _raw
        if raw.numel() < obj.raw_bytes or raw.dtype != torch.uint8 or raw.device != blob.device:
            raise ValueError('the workspace is %d uint8 on the device' % obj.raw_bytes)
        check(L.dbn_png_unfilter(blob.data_ptr(), obj.blob_len, blob.numel(), hdesc.ctypes.data, desc.data_ptr(), len(obj), hsubs.ctypes.data,
                                 subs.data_ptr(), len(hsubs), raw.data_ptr(), obj.raw_bytes, out_bytes, stream), 'png_unfilter')
        check(L.dbn_png_pixels(raw.data_ptr(), obj.raw_bytes, hdesc.ctypes.data, desc.data_ptr(), pal.data_ptr(), len(obj), obj.blob_len,
                               out.data_ptr(), out_bytes, stream), 'png_pixels')
    return out, shapes


def decode_png_batch(datas, device=None, threads=MAX_THREADS, fallback=False, errors='raise'):
    """PNG byte strings -> (packed uint8 device tensor, shapes [(H, W)]): RGB by cv2.imread's rule (the module's docstring), image
    after image, what augment_images(packed, shapes, plans) takes.  A refused kind raises UnsupportedPng, a damaged file CorruptPng
    (both name the image); fallback=True decodes refused kinds through PIL, when it is importable, and splices them in.
    errors='report': nothing raises; -> (packed, shapes, errs) with errs[i] None or the exception, a failed image taking no bytes
    and shape (0, 0)."""
    if errors not in ('raise', 'report'):
        raise ValueError("errors is 'raise' or 'report'")
    datas = list(datas)
    obj = inflate_png(datas, threads)
    errs = obj.errors()
    spliced = {}
    if fallback:
        for i, e in enumerate(errs):
            if isinstance(e, UnsupportedPng):
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
    packed, shapes = unfilter_png(obj, device)
    if spliced:
        packed, shapes = splice_images(packed, shapes, spliced)
    return (packed, shapes) if errors == 'raise' else (packed, shapes, errs)


def decode_png(data, device=None, fallback=False):
    """one PNG byte string -> uint8 [H, W, 3] device tensor (RGB; grey replicated, alpha dropped)"""
    packed, shapes = decode_png_batch([data], device, 1, fallback)
    return packed.view(shapes[0][0], shapes[0][1], 3)


def png_collate(items):
    """collate_fn for items (png bytes, polys, tags): the host half of the decode, here (in the DataLoader worker) ->
    (PngScanlines, shapes, per-image lists of fp64 [V, 2] polygons, per-image tag lists); DeviceBatches.convert runs the device
    half.  A file that cannot be decoded raises (UnsupportedPng / CorruptPng)."""
    obj = inflate_png([b[0] for b in items], threads=min(len(items), MAX_THREADS), pin=None)
    obj.raise_errors()
    return (obj, obj.shapes) + polys_tags(items)


def decode_image_batch(datas, device=None, **kw):
    """A mixed list of JPEG and PNG byte strings (a folder read with cv2.imread) -> one packed batch in the callers' order:
    (packed, shapes), or (packed, shapes, errs) with errors='report'.  The first bytes decide: FF D8 is JPEG and goes to
    decode_jpeg_batch, everything else to decode_png_batch (which names what is not a PNG); each decoder runs once.  kw:
    threads, fallback, errors for both; entropy, multiscan, orient for the JPEGs.  Error indices are the callers'."""
    datas = list(datas)
    if not datas:
        raise ValueError('decode_image_batch needs at least one stream')
    is_jpeg = [bytes(memoryview(d)[:2]) == b'\xff\xd8' for d in datas]
    groups = [([i for i, j in enumerate(is_jpeg) if j], decode_jpeg_batch, kw),
              ([i for i, j in enumerate(is_jpeg) if not j], decode_png_batch, {k: v for k, v in kw.items() if k in ('threads', 'fallback', 'errors')})]
    report = kw.get('errors', 'raise') == 'report'
    parts, shapes, errs = [None] * len(datas), [None] * len(datas), [None] * len(datas)
    for idx, fn, args in groups:
        if not idx:
            continue
        try:
            res = fn([datas[i] for i in idx], device, **args)
        except ValueError as e:
            if getattr(e, 'index', None) is not None:  # the index within the whole list
                raise type(e)(e.code, idx[e.index])
            raise
        o = 0
        for k, i in enumerate(idx):
            h, w = res[1][k]
            parts[i], shapes[i] = res[0][o:o + h * w * 3], (h, w)
            o += h * w * 3
            if report and res[2][k] is not None:
                errs[i] = type(res[2][k])(res[2][k].code, i)
    packed = parts[0] if len(parts) == 1 else torch.cat(parts)
    return (packed, shapes, errs) if report else (packed, shapes)


# ---- encode ------------------------------------------------------------------------------------------------------------
def _filter_arg(filter):
    if filter == 'adaptive':
        return -1
    if isinstance(filter, bool) or not isinstance(filter, (int, np.integer)) or not 0 <= int(filter) <= 4:
        raise ValueError("filter is 'adaptive' or a type 0 .. 4, got %r" % (filter, ))
    return int(filter)


def _filter_launch(images, shapes, filter, device):
    """-> (uint8 device tensor of every image's filtered rows, [(offset, H, row bytes + 1, channels, W)])"""
    f = _filter_arg(filter)
    dev = cuda_device('filter_png_rows', device, images)
    with on_device(dev) as stream:
        try:
            flat, items = encode_inputs(images, shapes, dev)  # the layouts, and the 65535-pixel limit, are the JPEG encoder's
        except ValueError as e:
            raise ValueError(str(e).replace('a JPEG image', 'a PNG image written here')) from None
        hdesc = np.zeros((len(items), 8), np.int64)
        o = rows = 0
        layout = []
        for n, (off, h, w, nc) in enumerate(items):
            hdesc[n, :6] = off, h, w, nc, o, rows
            layout.append((o, h, w * nc + 1, nc, w))
            o += h * (w * nc + 1)
            rows += h
        out = torch.empty(o, dtype=torch.uint8, device=dev)
        desc = upload(hdesc, dev)
        check(lib().dbn_png_filter_rows(flat.data_ptr(), flat.numel(), hdesc.ctypes.data, desc.data_ptr(), len(items), f, out.data_ptr(), o, stream),
              'png_filter_rows')
    return out, layout


def filter_png_rows(images, shapes=None, filter='adaptive', device=None):
    """Device half of the encode: uint8 images (the layouts of encode_png_batch) -> per image a uint8 [H, 1 + W * C] host array: every
    row's filter-type byte and the filtered row, what deflate then takes.  filter='adaptive': per row the type whose sum of
    min(f, 256 - f) over the filtered bytes is lowest, the lowest type of equal ones (libpng's heuristic); 0 .. 4: that type for
    every row (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth).  One launch, parallel over rows; the host waits for the copy."""
    out, layout = _filter_launch(images, shapes, filter, device)
    host = out.cpu().numpy()
    return [host[o:o + h * rb1].reshape(h, rb1) for o, h, rb1, _, _ in layout]


def _chunk(kind, body):
    return struct.pack('>I', len(body)) + kind + body + struct.pack('>I', zlib.crc32(kind + body))


def encode_png_batch(images, shapes=None, compress_level=6, filter='adaptive', threads=MAX_THREADS, device=None):
    """uint8 images -> list of PNG byte strings: 8-bit, colour type 2 (RGB) or 0 (grey), not interlaced; IHDR, one IDAT, IEND.
    images: the packed 1-D uint8 RGB batch with shapes [(H, W)] (decode_png_batch's output); or uint8 [H, W, 3] / [N, H, W, 3] RGB;
    or uint8 [H, W] / [N, H, W] grey; or a list of [H, W, 3] and [H, W] images of any sizes.  Tensors or arrays, on the host or the
    device.  The filters are chosen and applied on the GPU (filter_png_rows); zlib.compress(rows, compress_level) runs on
    min(N, 16, threads) host threads.  compress_level 0 .. 9 (zlib's; 6 is Pillow's default too)."""
    if isinstance(compress_level, bool) or int(compress_level) != compress_level or not 0 <= int(compress_level) <= 9:
        raise ValueError('compress_level must be an integer in 0 .. 9, got %r' % (compress_level, ))
    level = int(compress_level)
    out, layout = _filter_launch(images, shapes, filter, device)
    host = out.cpu().numpy()

    def one(item):
        o, h, rb1, nc, w = item
        return (SIGNATURE + _chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 0 if nc == 1 else 2, 0, 0, 0))
                + _chunk(b'IDAT', zlib.compress(host[o:o + h * rb1].tobytes(), level)) + _chunk(b'IEND', b''))

    workers = max(1, min(len(layout), MAX_THREADS, int(threads)))
    if workers == 1:
        return [one(it) for it in layout]
    with ThreadPoolExecutor(workers) as pool:
        return list(pool.map(one, layout))


def encode_png(image, compress_level=6, filter='adaptive', device=None):
    """one uint8 [H, W, 3] (or grey [H, W]) image -> bytes"""
    if getattr(image, 'ndim', 0) not in (2, 3) or (image.ndim == 3 and image.shape[2] != 3):
        raise ValueError('encode_png takes one uint8 [H, W, 3] or [H, W] image')
    return encode_png_batch([image], None, compress_level, filter, 1, device)[0]


def save_pngs(paths, images, shapes=None, **kw):
    """encode_png_batch(images, shapes, **kw) written to `paths`, one file per image -> the paths"""
    paths = [os.fspath(p) for p in paths]
    datas = encode_png_batch(images, shapes, **kw)
    if len(paths) != len(datas):
        raise ValueError('%d paths for %d images' % (len(paths), len(datas)))
    for p, d in zip(paths, datas):
        with open(p, 'wb') as f:
            f.write(d)
    return paths
