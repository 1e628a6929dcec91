"""The packed-batch contract of the image pipeline, and what every stage needs to honour it.

A packed batch is (packed, shapes): a flat uint8 tensor that holds N images [H, W, 3] end to end, on the host or the device, and
their [(H, W)]; image n starts at byte image_offsets(shapes)[n].  An image that was not decoded has shape (0, 0) and takes no bytes.
The decoders write it; image_collate, color_jitter_images, degrade_images, augment_images, crop_words, the draw_* functions and the encoders take it.

  check_shape, offsets, image_offsets, check_bytes, as_images, packed_on, flat_u8, image_table   the layout and its checks
  cuda_device, upload, stream, on_device                                                          where and how a stage launches
  pin_default, polys_tags                                                                         what the collate functions share
  DecodeError, DecodedBatch                                                                       the base of the decoders' errors and results

Error texts belong to the callers (tests match them), so a check takes its wording as an argument.  Imports nothing from the
package but _lib: every stage can import this module.
"""
import numpy as np
import torch

MAX_SIDE = 65535


def check_shape(shape):
    """(H, W, ...) -> (int H, int W), both in 1 .. MAX_SIDE"""
    H, W = int(shape[0]), int(shape[1])
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError('image size %d x %d outside 1 .. %d' % (H, W, MAX_SIDE))
    return H, W


def offsets(sizes):
    """[0, cumsum(sizes)]: int64 [len(sizes) + 1]"""
    off = np.zeros(len(sizes) + 1, np.int64)
    off[1:] = np.cumsum(np.asarray(sizes, np.int64))
    return off


def image_offsets(shapes):
    """the byte offset of every image of a packed batch, and behind them its length: int64 [N + 1]"""
    return offsets([int(h) * int(w) * 3 for h, w in shapes])


def check_bytes(numel, need, holds='packed holds', flat=True):
    """the one size check: a buffer of `numel` bytes (flat: and one dimension) against the `need` bytes of its shapes"""
    if numel != need or not flat:
        raise ValueError('%s %d bytes, the shapes need %d' % (holds, numel, need))


def _check_packed(packed, shapes, name, holds):
    if packed.dtype != torch.uint8 or packed.dim() != 1:
        raise ValueError('%s must be a flat uint8 tensor (image_collate)' % name)
    check_bytes(packed.numel(), sum(int(h) * int(w) * 3 for h, w in shapes), '%s %s' % (name, holds))


def as_images(images):
    """image_collate's (packed, shapes, ...) or one uint8 [H, W, 3] tensor -> (packed uint8 tensor, [(H, W)]), checked"""
    if isinstance(images, torch.Tensor):
        if images.dtype != torch.uint8 or images.dim() != 3 or images.shape[2] != 3:
            raise ValueError('a single image must be a uint8 [H, W, 3] tensor')
        return images.contiguous().reshape(-1), [check_shape(images.shape)]
    if not isinstance(images, (tuple, list)) or len(images) < 2 or not isinstance(images[0], torch.Tensor):
        raise ValueError('images must be (packed uint8 tensor, shapes) as image_collate gives them, or a uint8 [H, W, 3] tensor')
    packed, shapes = images[0], [check_shape(s) for s in images[1]]
    _check_packed(packed, shapes, 'the packed images', 'hold')
    return packed, shapes


def packed_on(packed_u8, shapes, dev):
    """the packed batch, checked against its shapes, on `dev` (a non-blocking copy when it is not there yet)"""
    _check_packed(packed_u8, shapes, 'packed_u8', 'holds')
    return packed_u8.to(dev, non_blocking=True).contiguous()


def flat_u8(a, dev=None, what='images'):
    """With `dev`: a uint8 tensor or array of any shape, on the host or a device -> flat on `dev`.  Without: `a` (named `what`) must
    already be a flat contiguous uint8 tensor on a GPU and is returned as it is (for stages that have no host path)."""
    if dev is None:
        if not isinstance(a, torch.Tensor) or not a.is_cuda:
            raise ValueError('%s must be a tensor on a GPU device (there is no host path)' % what)
        if a.dtype != torch.uint8 or a.dim() != 1 or not a.is_contiguous():
            raise ValueError('%s must be a flat contiguous uint8 tensor' % what)
        return a
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
        raise ValueError('images must be uint8 tensors or arrays')
    return t.contiguous().view(-1).to(dev, non_blocking=True)


def image_table(shapes, dev, rows=None):
    """the kernels' image table on `dev`: int64 [N, 3] of (byte offset, H, W); rows: the images to list instead, one row each"""
    hw = np.array(shapes, np.int64).reshape(-1, 2)
    table = np.concatenate([image_offsets(shapes)[:-1, None], hw], 1)
    return upload(table if rows is None else table[rows], dev)


def cuda_device(who, device, like=None):
    """`device`, else the device of the tensor `like` when that is on a GPU, else the current GPU: as a cuda device with an index.
    `who`: the caller's name for the error."""
    dev = torch.device(device) if device is not None else like.device if isinstance(like, torch.Tensor) and like.is_cuda else None
    if dev is not None and dev.type != 'cuda':
        raise ValueError('%s runs on a GPU device, not %s' % (who, dev))
    return dev if dev is not None and dev.index is not None else torch.device('cuda', torch.cuda.current_device())


def upload(a, dev):
    """a small numpy table -> device tensor: a non-blocking copy, from pinned memory when a GPU is visible"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.pin_memory() if torch.cuda.is_available() else t).to(dev, non_blocking=True)


def stream(dev):
    """the raw handle of the current stream of `dev`, as the C entry points take it"""
    return torch.cuda.current_stream(dev).cuda_stream


class on_device(torch.cuda.device):
    """how a stage launches: `with on_device(dev) as st:` makes `dev` the current device and gives the handle of its current stream"""

    def __enter__(self):
        super().__enter__()
        return torch.cuda.current_stream(self.idx).cuda_stream


def pin_default(pin=None):
    """pin=None: pin when a GPU is visible and this is not a DataLoader worker (a loader's pin_memory=True pins there)"""
    return bool(torch.utils.data.get_worker_info() is None and torch.cuda.is_available() if pin is None else pin)


def polys_tags(items):
    """collate items (_, polys, tags) -> (per-image lists of fp64 [V, 2] polygons, per-image tag lists; tags=None: a None per polygon)"""
    polys = [[np.asarray(p, dtype=np.float64).reshape(-1, 2) for p in b[1]] for b in items]
    tags = [list(b[2]) if b[2] is not None else [None] * len(b[1]) for b in items]
    return polys, tags


class DecodeError(ValueError):
    """a stream that was not decoded: .code is its status, .index the image's place in its batch, .reason the text of the code.
    A family (JpegError, PngError) sets `reasons`, the `refused` codes, and its `unsupported` and `corrupt` classes."""
    reasons, refused, unsupported, corrupt = {}, (), None, None

    def __init__(self, code, index=None):
        self.code, self.index, self.reason = int(code), index, self.reasons.get(int(code)) or 'status %d' % code
        ValueError.__init__(self, self.reason if index is None else 'image %d: %s' % (index, self.reason))

    @classmethod
    def of(cls, code, index=None):
        """the family's exception for a status: `unsupported` for a refused kind (another decoder may take it), else `corrupt`"""
        return (cls.unsupported if code in cls.refused else cls.corrupt)(code, index)


class DecodedBatch:
    """what the host halves' results share, from `desc` and `status` (0: decoded); a class sets `error` (its DecodeError family) and
    `_hw`, the fields of a `desc` row that hold the height and the width"""

    @property
    def shapes(self):
        h, w = self._hw
        return [(int(d[h]), int(d[w])) if s == 0 else (0, 0) for d, s in zip(self.desc, self.status)]

    def __len__(self):
        return len(self.status)

    def errors(self):
        """per image None, or the exception that says why it was not decoded"""
        return [None if s == 0 else self.error.of(int(s), i) for i, s in enumerate(self.status)]

    def raise_errors(self):
        """raise the first of errors(), if there is one"""
        for e in self.errors():
            if e is not None:
                raise e
