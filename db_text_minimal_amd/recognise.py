"""Reading word crops on the device: everything around the text recogniser of the reference's full pipeline
(test_ocr.py:59-108,179-200, test_webcam.py), batched.  The recogniser itself (clova_ocr's Model) stays the user's nn.Module.

  words_to_input(crops, rgb, bgr, dtype)       rec_preprocess of every crop in one launch: uint8 [K, h, w, 3] ->
                                               [K, 1 | 3, h, w] in fp32 / fp16 / bf16
  greedy_decode(logits, mode, lengths)         predict()'s argmax, softmax, maximum probability, cumprod and the CTC /
                                               attention collapse: (codes, count, score) on the device, two launches
  CTCLabelConverter / AttnLabelConverter       codes -> strings, from one device-to-host copy
  recognize_words(images, boxes, model, ...)   crop_words (rectify_words for polygons=) -> words_to_input -> model ->
                                               greedy_decode -> strings

Pinned: the grey formula against PIL's convert('L') and the normalisation against torch's ToTensor arithmetic (on the
CPU, tests/test_recognise_cpu.py); the decode against a numpy restatement that equals the reference's torch ops.
UNPINNED: clova_ocr's own preprocessing and converters, which are not in the reference tree.
"""
import numpy as np
import torch

from ._lib import check, lib
from .packed import on_device
from .word_crops import SIZE, crop_words, rectify_words

_INT_MAX = 2 ** 31 - 1
_AT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}  # DBN_AT_* of include/dbnet_hip.h
BLANK, EOS = 0, 1  # '[blank]' of the CTC table, '[s]' of the attention table
_MODES = {'ctc': 0, 'attn': 1}
_LEXICON_STEPS = 64  # decode steps recognize_words(lexicon=) takes: the pattern of dbn_lexicon_nearest is one 64-bit word


def input_table():
    """fp32 [256]: ToTensor then sub_(0.5).div_(0.5) of every byte, (g / 255 - 0.5) / 0.5 in float32, in that order"""
    g = np.arange(256, dtype=np.float32)
    return (g / np.float32(255) - np.float32(0.5)) / np.float32(0.5)


_tables = {}


def _table_on(dev):
    if dev not in _tables:
        _tables[dev] = torch.from_numpy(input_table()).to(dev)
    return _tables[dev]


def words_to_input(crops, rgb=False, bgr=False, dtype=torch.float32):
    """uint8 device crops [K, h, w, 3] (crop_words) -> the recogniser's input [K, 1, h, w] (grey) or [K, 3, h, w] (rgb=True,
    planar, the crops' channel order), in `dtype` (float32, float16 or bfloat16), one launch on the current stream.

    Grey is PIL's convert('L') in integers, (19595 c0 + 38470 c1 + 7471 c2 + 32768) >> 16 with c0 .. c2 in the crops'
    channel order (RGB crops when the images were RGB); bgr=True swaps the weights for BGR crops.  The value is
    (g / 255 - 0.5) / 0.5 from a 256-entry float32 table (input_table), so float32 output is that arithmetic bit for bit and
    the 16-bit types are its round-to-nearest-even conversions."""
    if not isinstance(crops, torch.Tensor) or crops.dtype != torch.uint8 or crops.dim() != 4 or crops.shape[3] != 3:
        raise ValueError('crops must be a uint8 [K, h, w, 3] tensor')
    if not crops.is_cuda:
        raise ValueError('words_to_input runs on a GPU device, not %s' % crops.device)
    if dtype not in _AT:
        raise ValueError('dtype must be float32, float16 or bfloat16, got %r' % (dtype, ))
    K, h, w, _ = crops.shape
    if h < 1 or w < 1:
        raise ValueError('crop size %d x %d' % (h, w))
    n_px = K * h * w
    if -(-n_px // 1024) > _INT_MAX:  # dbn_words_to_input's grid: four pixels per thread, 256 threads
        raise ValueError('%d crops of %d x %d are too many for one call' % (K, h, w))
    out = torch.empty((K, 3 if rgb else 1, h, w), device=crops.device, dtype=dtype)
    if K == 0:
        return out
    crops = crops.contiguous()
    table = _table_on(crops.device)
    with on_device(crops.device) as st:
        check(lib().dbn_words_to_input(_AT[dtype], crops.data_ptr(), n_px, h * w, int(bool(rgb)), int(bool(bgr)), table.data_ptr(), out.data_ptr(), st),
              'words_to_input')
    return out


def greedy_decode(logits, mode='ctc', lengths=None):
    """Greedy decode of a recogniser's output logits [B, T, C] (float32, float16 or bfloat16 on the device; widened to
    float32 exactly) -> (codes int32 [B, T], count int32 [B], score float32 [B]), device tensors.  Two launches on the current
    stream, no host synchronisation.  lengths: optional int32 [B], the steps of each sequence (clamped to 0 .. T; default T).

    Per step t < len_b: m = max_c x, k_t = the smallest index with x == m (exact), p_t = 1 / sum_c exp(x_c - m) accumulated in
    float32.  A row that contains a NaN gives k_t = the index of its first NaN and p_t = NaN, which is torch.max on the CPU.
      mode 'ctc'   step t is kept iff k_t != 0 ([blank]) and (t == 0 or k_t != k_{t-1}); score = the product of p_t over ALL
                   len_b steps (the reference's cumprod covers every step, not only the kept ones).
      mode 'attn'  e = the first t with k_t == 1 ([s]), or len_b if there is none; the steps t < e are kept and score = the
                   product of their p_t; the empty product is 1.0.
    The product is formed in float32 in ascending t, so two runs agree bit for bit.  codes holds the kept k_t packed to the
    left and -1 after them; every element of all three outputs is written.

    Two quirks of the reference's predict() are deliberately not reproduced: str.find returning -1 drops the last character
    when no '[s]' occurs, and cumprod(...)[-1] raises on an empty prefix ('[s]' first)."""
    if mode not in _MODES:
        raise ValueError("mode must be 'ctc' or 'attn', got %r" % (mode, ))
    if not isinstance(logits, torch.Tensor) or logits.dim() != 3 or logits.dtype not in _AT:
        raise ValueError('logits must be a float32, float16 or bfloat16 [B, T, C] tensor')
    if not logits.is_cuda:
        raise ValueError('greedy_decode runs on a GPU device, not %s' % logits.device)
    B, T, C = logits.shape
    if C < 1:
        raise ValueError('logits need at least one class')
    if C > _INT_MAX or B * T > _INT_MAX:
        raise ValueError('logits [%d, %d, %d] are too large for one call' % (B, T, C))
    dev = logits.device
    codes = torch.empty((B, T), device=dev, dtype=torch.int32)
    count = torch.empty((B, ), device=dev, dtype=torch.int32)
    score = torch.empty((B, ), device=dev, dtype=torch.float32)
    len_ptr = None
    if lengths is not None:
        lengths = torch.as_tensor(lengths).to(device=dev, dtype=torch.int32).contiguous()
        if lengths.shape != (B, ):
            raise ValueError('lengths must have shape [%d], got %s' % (B, tuple(lengths.shape)))
        len_ptr = lengths.data_ptr()
    if B == 0:
        return codes, count, score
    if T == 0:
        return codes, count.zero_(), score.fill_(1.0)
    logits = logits.contiguous()
    ws = torch.empty((lib().dbn_greedy_decode_ws_bytes(B, T) // 4, ), device=dev, dtype=torch.int32)
    with on_device(dev) as st:
        check(lib().dbn_greedy_decode(_AT[logits.dtype], logits.data_ptr(), B, T, C, len_ptr, _MODES[mode], ws.data_ptr(), codes.data_ptr(),
                                      count.data_ptr(), score.data_ptr(), st), 'greedy_decode')
    return codes, count, score


def _fetch(codes, count, score=None, more=()):
    """codes [B, T], count [B] (and score [B], and further int32 [B] columns `more`) on the host from ONE device-to-host copy"""
    parts = [codes, count[:, None]] + ([score.view(torch.int32)[:, None]] if score is not None else []) + [m[:, None] for m in more]
    host = torch.cat(parts, 1).cpu().numpy()
    T = codes.shape[1]
    got = host[:, :T], host[:, T], (host[:, T + 1].copy().view(np.float32) if score is not None else None)
    return got + tuple(host[:, host.shape[1] - len(more) + j] for j in range(len(more))) if more else got


class _LabelConverter:
    def __init__(self, head, character):
        self.character = list(head) + list(character)
        self._table = np.array(self.character, dtype=object)

    def decode_host(self, codes, count):
        """numpy codes [B, T], count [B] -> list of B strings"""
        codes, count = np.asarray(codes), np.asarray(count).astype(np.int64)
        B, T = codes.shape
        if count.shape != (B, ) or (count < 0).any() or (count > T).any():
            raise ValueError('count must be [%d] within 0 .. %d' % (B, T))
        kept = np.arange(T)[None, :] < count[:, None]
        flat = codes[kept].astype(np.int64)
        if flat.size and (flat.min() < 0 or flat.max() >= len(self.character)):
            raise ValueError('codes outside the %d entries of the character table' % len(self.character))
        chars = self._table[flat]
        ends = np.cumsum(count)
        return [''.join(chars[e - n:e]) for e, n in zip(ends.tolist(), count.tolist())]

    def decode(self, codes, count):
        """codes [B, T], count [B] as greedy_decode returns them (device tensors; host arrays are taken as they are) -> list of
        B strings, from one device-to-host copy; a kept code outside the table raises ValueError"""
        if isinstance(codes, torch.Tensor):
            codes, count, _ = _fetch(codes, count)
        return self.decode_host(codes, count)


class CTCLabelConverter(_LabelConverter):
    """table ['[blank]'] + list(character): index 0 is the CTC blank (greedy_decode mode 'ctc')"""

    def __init__(self, character):
        super().__init__(['[blank]'], character)


class AttnLabelConverter(_LabelConverter):
    """table ['[GO]', '[s]'] + list(character): index 1 ends a word (greedy_decode mode 'attn')"""

    def __init__(self, character):
        super().__init__(['[GO]', '[s]'], character)


def _box_rows(boxes):
    if isinstance(boxes, np.ndarray) and boxes.ndim == 3:
        boxes = [boxes]
    return [np.asarray(b[0] if isinstance(b, tuple) and len(b) == 2 else b) for b in boxes]


def recognize_words(images, boxes, model, converter, prediction='CTC', batch_size=512, batch_max_length=25, rgb=False, size=SIZE,
                    scores=None, min_score=None, polygons=None, segments=32, ends='auto', ribbons='host', lexicon=None, max_distance=None):
    """From images and detected boxes to strings: crop_words -> words_to_input -> model -> greedy_decode -> converter.decode.

    images, boxes, size, scores, min_score: as crop_words takes them.  Or polygons= (with boxes = None) instead of boxes:
    images, polygons, size, scores, min_score, segments, ends, ribbons as rectify_words takes them, which then cuts the crops.  Or
    ready crops: images = a uint8 device tensor [K, h, w, 3] with boxes = None.
    model: the user's recogniser, called under no_grad in chunks of batch_size as the reference calls it, with text_for_pred a zero LongTensor [b, batch_max_length + 1]: model(image, text_for_pred) for
    prediction 'CTC', model(image, text_for_pred, is_train=False) for 'Attn'; it returns logits [b, T, C].
    Returns, per image, a list of {'box': the box row (int16 [4, 2]), 'pred': str, 'score': float} in box order ('box': the
    polygon as given, [P, 2], for polygons=); for ready crops one flat list with 'box': None.  One device-to-host copy for
    all words.
    lexicon: a spotting.Lexicon built over the classes of this converter.  Every dict gains 'word', the lexicon's nearest entry
    by edit distance (the smallest index among equals), or None when there is none within max_distance (None: any distance)
    or the group is empty, and 'distance' (-1 for an empty group); 'pred' and 'score' are as without it.  A lexicon of more than
    one group is searched per image: the group of a word is its image index.  The search runs on the device codes (one more
    entry point, dbn_lexicon_nearest) before the copy back, which then carries index and distance with the codes.  It takes
    recognisers of at most 64 decode steps (logits [b, T <= 64, C]: the query is the one-word pattern of the kernel); a
    longer one raises ValueError before the model runs where the steps are known then ('Attn': batch_max_length + 1), else
    at the model's first chunk."""
    if boxes is not None and polygons is not None:
        raise ValueError('boxes or polygons, not both')
    if not (isinstance(ribbons, str) and ribbons in ('host', 'device')):
        raise ValueError("ribbons must be 'host' or 'device', got %r" % (ribbons, ))
    if 'CTC' in prediction:
        mode = 'ctc'
    elif 'Attn' in prediction:
        mode = 'attn'
    else:
        raise ValueError("prediction must be 'CTC' or 'Attn', got %r" % (prediction, ))
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError('batch_size must be positive')
    if lexicon is not None and lexicon.n_groups != 1 and boxes is None and polygons is None:
        raise ValueError('a lexicon of %d groups needs images: ready crops have no image index' % lexicon.n_groups)
    if lexicon is not None and mode == 'attn' and batch_max_length + 1 > _LEXICON_STEPS:
        raise ValueError('lexicon=: an attention recogniser of %d steps; at most %d' % (batch_max_length + 1, _LEXICON_STEPS))
    if polygons is not None:
        polygons = list(polygons)
        crops, index = rectify_words(images, polygons, size, scores, min_score, segments, ends, ribbons=ribbons)
        rows = [[np.asarray(p) for p in (ps[0] if isinstance(ps, tuple) and len(ps) == 2 else ps)] for ps in polygons]
        n_images = 1 if isinstance(images, torch.Tensor) else len(images[1])
    elif boxes is None:
        crops, index, rows, n_images = images, None, None, None
    else:
        crops, index = crop_words(images, boxes, size, scores, min_score)
        rows = _box_rows(boxes)
        n_images = 1 if isinstance(images, torch.Tensor) else len(images[1])
    x = words_to_input(crops, rgb=rgb)
    K = x.shape[0]
    outs = []
    with torch.no_grad():
        for k0 in range(0, K, batch_size):
            image = x[k0:k0 + batch_size]
            text_for_pred = torch.zeros((image.shape[0], batch_max_length + 1), dtype=torch.long, device=x.device)
            logits = model(image, text_for_pred) if mode == 'ctc' else model(image, text_for_pred, is_train=False)
            if lexicon is not None and logits.shape[1] > _LEXICON_STEPS:  # (known only from the model's output: at its first chunk)
                raise ValueError('lexicon=: the recogniser gives %d steps; at most %d' % (logits.shape[1], _LEXICON_STEPS))
            outs.append(greedy_decode(logits, mode))
    words = []
    if outs:
        T = max(c.shape[1] for c, _, _ in outs)
        pad = [torch.nn.functional.pad(c, (0, T - c.shape[1]), value=-1) for c, _, _ in outs]
        d_codes, d_count, d_score = torch.cat(pad), torch.cat([n for _, n, _ in outs]), torch.cat([s for _, _, s in outs])
        if lexicon is None:
            codes, count, score = _fetch(d_codes, d_count, d_score)
        else:
            group = index[:, 0].astype(np.int32) if lexicon.n_groups != 1 else None
            near = lexicon.nearest(d_codes, d_count, group, head=converter)
            codes, count, score, near_index, near_dist = _fetch(d_codes, d_count, d_score, near)
            found = lexicon.words_of(near_index, near_dist, np.zeros(len(near_index), np.int64) if group is None else group, max_distance)
        words = list(zip(converter.decode_host(codes, count), score.tolist()))
    made = [{'pred': p, 'score': s} for p, s in words]
    if lexicon is not None:
        for w, (word, distance) in zip(made, found if outs else []):
            w['word'], w['distance'] = word, distance
    if index is None:
        return [dict(box=None, **w) for w in made]
    result = [[] for _ in range(n_images)]
    for (n, k), w in zip(index.tolist(), made):
        result[n].append(dict(box=rows[n][k], **w))
    return result
