"""Scoring and correcting the recognised text on the device: edit distances, the nearest word of a lexicon, and the
end-to-end (detection + transcription) precision / recall / HMean (csrc/lexicon.hip).

  TextClasses(converter_or_character, ...)     characters -> classes 0 .. 254 (case folded as ICDAR compares), and the
                                               table from greedy_decode's codes to those classes
  edit_distances(a, b, classes)                unit-cost Levenshtein distance of P pairs, one launch -> int32 [P] on the device
  Lexicon(words, classes)                      a word list resident on the device: nearest() -> (index, distance) per decoded
                                               word without a host synchronisation, correct() -> the words from one copy
  recognize_words(..., lexicon=, max_distance=)
                                               recognise.recognize_words; with a lexicon every word gains 'word' and 'distance'
  TextSpottingEvaluator                        DetectionIoUEvaluator's matching, then a pair counts only if its transcription
                                               is right; '1-ned' beside it

Everything here is exact in integers: the device results equal the plain dynamic programme (tests/spotting_ref.py) in every
bit, and two runs agree in every bit.  The pattern side of a pair is limited to 64 classes (one machine word of the
bit-vector recurrence); the other side may have any length.

UNPINNED: the end-to-end protocol is ICDAR's as this project states it; the RRC evaluation script is not in the reference
tree, so the parity with it is not pinned.  Its word-spotting variant (short and non-alphabetic words as don't-care) is not
implemented.
"""
import numpy as np
import torch

from ._lib import check, lib
from .det_eval import DetectionIoUEvaluator
from .packed import cuda_device, offsets, on_device, upload
from .recognise import AttnLabelConverter, CTCLabelConverter, recognize_words  # noqa: F401

MAX_PATTERN = 64   # classes of a pair's pattern side: one 64-bit word of the recurrence
MAX_ENTRY = 255    # characters of a lexicon entry
NO_CLASS = 255     # the class that matches nothing, not even itself
BLOCK = 64         # lexicon entries per block: one per lane of a wave
_INT_MAX = 2 ** 31 - 1


class TextClasses:
    """The map from characters to the classes 0 .. 254 that the kernels compare.

    converter_or_character: a CTCLabelConverter / AttnLabelConverter, or the recogniser's characters alone (a string or a
    list).  These take the first classes in their order; with case_sensitive=False two characters share a class when their
    ch.upper() agrees (ICDAR's comparison).  Any further distinct character met in a lexicon or a ground-truth string
    (encode) takes the next class as it is met; a 256th class raises ValueError."""

    def __init__(self, converter_or_character, case_sensitive=False):
        self.case_sensitive = bool(case_sensitive)
        if isinstance(converter_or_character, AttnLabelConverter):
            self.head = 2
        elif isinstance(converter_or_character, CTCLabelConverter):
            self.head = 1
        elif hasattr(converter_or_character, 'character'):
            raise ValueError('a converter must be a CTCLabelConverter or an AttnLabelConverter; pass its characters and give remap() the head')
        else:
            self.head = None
        chars = converter_or_character.character[self.head:] if self.head is not None else converter_or_character
        self.character = list(chars)
        self._class = {}
        self._of_character = np.array([self._add(ch) for ch in self.character], np.uint8)
        self._remaps = {}

    def __len__(self):
        return len(self._class)

    def _add(self, ch):
        key = ch if self.case_sensitive else ch.upper()
        c = self._class.get(key)
        if c is None:
            if len(self._class) >= NO_CLASS:
                raise ValueError('more than %d distinct classes: %r would be class %d' % (NO_CLASS, ch, NO_CLASS))
            c = self._class[key] = len(self._class)
        return c

    def encode(self, texts):
        """list of n strings -> (classes uint8 [total], offsets int32 [n + 1]) on the host; string i is
        classes[offsets[i]:offsets[i + 1]], one class per character"""
        texts = list(texts)
        for t in texts:
            if not isinstance(t, str):
                raise TypeError('texts must be strings, got %r' % (type(t).__name__, ))
        off = offsets([len(t) for t in texts])
        if off[-1] > _INT_MAX:
            raise ValueError('%d characters are too many for one call' % int(off[-1]))
        data = np.fromiter((self._add(ch) for t in texts for ch in t), np.uint8, count=int(off[-1]))
        return data, off.astype(np.int32)

    def _head(self, head):
        head = self.head if head is None else head
        if isinstance(head, AttnLabelConverter):
            head = 2
        elif isinstance(head, CTCLabelConverter):
            head = 1
        if head is None:
            raise ValueError('the number of special codes is unknown: build TextClasses from the converter, or pass head= (1 for CTC, 2 for attention)')
        head = int(head)
        if head < 0:
            raise ValueError('head must not be negative')
        return head

    def remap_host(self, head=None):
        """uint8 [head + len(character) + 1]: greedy_decode's code -> class.  The `head` special codes ('[blank]' of the CTC
        table; '[GO]', '[s]' of the attention table) and one extra last entry are 255."""
        head = self._head(head)
        table = np.full(head + len(self.character) + 1, NO_CLASS, np.uint8)
        table[head:head + len(self.character)] = self._of_character
        return table

    def remap(self, head=None, device=None):
        """remap_host as a tensor on `device` (default: the current GPU), uploaded once"""
        head = self._head(head)
        dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        if (head, dev) not in self._remaps:
            self._remaps[head, dev] = torch.from_numpy(self.remap_host(head)).to(dev)
        return self._remaps[head, dev]

    def lookup(self, codes, head=None):
        """codes [B, T] as greedy_decode returns them -> classes uint8 [B, T] on the same device, remap[codes.clamp(0, n)]
        with n the table's extra last entry: no code value indexes outside the table.  (The -1 padding becomes a special;
        it lies beyond `count` and is never read.)"""
        table = self.remap(head, codes.device)
        return table[codes.clamp(0, table.shape[0] - 1).long()]


def _is_codes(x):
    return isinstance(x, (tuple, list)) and len(x) == 2 and isinstance(x[0], torch.Tensor)


def _check_codes(codes, count, who):
    if codes.dim() != 2 or codes.dtype not in (torch.int32, torch.int64) or not isinstance(count, torch.Tensor) or count.shape != (codes.shape[0], ):
        raise ValueError('%s: codes must be an integer [B, T] tensor and count [B], as greedy_decode returns them' % who)
    if not codes.is_cuda:
        raise ValueError('%s runs on a GPU device, not %s' % (who, codes.device))
    if codes.shape[1] > MAX_PATTERN:
        raise ValueError('%s: device codes of T = %d steps; at most %d' % (who, codes.shape[1], MAX_PATTERN))


def _pattern_of(codes, count, classes, head):
    """device codes -> (classes uint8 [B, max(T, 1)] contiguous, lengths int32 [B])"""
    B, T = codes.shape
    q = classes.lookup(codes, head).contiguous() if T else torch.full((B, 1), NO_CLASS, dtype=torch.uint8, device=codes.device)
    return q, count.to(device=codes.device, dtype=torch.int32).contiguous()


def pair_layout(ta, oa, tb, ob):
    """Two encoded string lists of P members each -> (pattern uint8 [P, T], pattern lengths int32 [P], text uint8 [total],
    text offsets int32 [P + 1]) on the host: of each pair the shorter member is the pattern (the distance is symmetric).
    ValueError if both members of a pair exceed 64 classes."""
    la, lb = np.diff(oa).astype(np.int64), np.diff(ob).astype(np.int64)
    P = len(la)
    swap = la > lb
    pl, tl = np.minimum(la, lb), np.maximum(la, lb)
    if P and pl.max() > MAX_PATTERN:
        raise ValueError('pair %d: both strings exceed %d classes (%d and %d)' % (int(np.argmax(pl)), MAX_PATTERN, la[np.argmax(pl)], lb[np.argmax(pl)]))
    T = max(int(pl.max()) if P else 0, 1)
    cat = np.concatenate([ta, tb, np.full(1, NO_CLASS, np.uint8)])
    sa, sb = oa[:-1].astype(np.int64), len(ta) + ob[:-1].astype(np.int64)
    ps, ts = np.where(swap, sb, sa), np.where(swap, sa, sb)
    pos = np.arange(T, dtype=np.int64)[None, :]
    pattern = np.where(pos < pl[:, None], cat[np.minimum(ps[:, None] + pos, len(cat) - 1)], NO_CLASS).astype(np.uint8)
    toff = offsets(tl)
    if toff[-1] > _INT_MAX:
        raise ValueError('%d classes of text are too many for one call' % int(toff[-1]))
    text = cat[np.repeat(ts - toff[:-1], tl) + np.arange(toff[-1], dtype=np.int64)]
    return pattern, pl.astype(np.int32), text, toff.astype(np.int32)


def edit_distances(a, b, classes, head=None, device=None):
    """The unit-cost Levenshtein distance (insert, delete, substitute) of P pairs (a[i], b[i]) in the classes of `classes`:
    int32 [P] on the device, one launch (dbn_edit_distance_pairs), no host synchronisation.

    a, b: each a list of P strings, or a (codes, count) pair as greedy_decode returns it (device tensors [P, T], [P]; head:
    the number of special codes, when `classes` was not built from the converter).  The side with at most 64 classes per
    row becomes the pattern; ValueError if both members of a pair exceed 64, and for device codes of T > 64 steps.  P = 0:
    an empty tensor, nothing is launched."""
    ca, cb = _is_codes(a), _is_codes(b)
    for x, is_c, name in ((a, ca, 'a'), (b, cb, 'b')):
        if is_c:
            _check_codes(x[0], x[1], 'edit_distances (%s)' % name)
    if not ca:
        a = list(a)
    if not cb:
        b = list(b)
    P = a[0].shape[0] if ca else len(a)
    if P != (b[0].shape[0] if cb else len(b)):
        raise ValueError('%d strings against %d' % (P, b[0].shape[0] if cb else len(b)))
    like = a[0] if ca else b[0] if cb else None
    if ca and cb and a[0].device != b[0].device:
        raise ValueError('the two sides are on different devices')
    enc = [None if is_c else classes.encode(x) for x, is_c in ((a, ca), (b, cb))]  # (raises before anything is launched)
    dev = cuda_device('edit_distances', device, like)
    dist = torch.empty((P, ), dtype=torch.int32, device=dev)
    if P == 0:
        return dist
    text_len = None
    if ca and cb:
        pattern, pat_len = _pattern_of(a[0], a[1], classes, head)
        text, text_len = _pattern_of(b[0], b[1], classes, head)
        if P * text.shape[1] > _INT_MAX:
            raise ValueError('%d pairs are too many for one call' % P)
        text_off = torch.arange(P + 1, dtype=torch.int32, device=dev) * text.shape[1]
    elif ca or cb:
        pattern, pat_len = _pattern_of(*(a if ca else b), classes, head)
        t, o = enc[1] if ca else enc[0]
        up = upload(np.concatenate([o.view(np.uint8), t]), dev)
        text_off, text = up[:o.nbytes].view(torch.int32), up[o.nbytes:]
    else:
        pattern, pat_len, t, o = pair_layout(*enc[0], *enc[1])
        up = upload(np.concatenate([pat_len.view(np.uint8), o.view(np.uint8), pattern.reshape(-1), t]), dev)
        n0, n1, n2 = pat_len.nbytes, pat_len.nbytes + o.nbytes, pat_len.nbytes + o.nbytes + pattern.size
        pat_len, text_off, pattern, text = up[:n0].view(torch.int32), up[n0:n1].view(torch.int32), up[n1:n2].view(P, -1), up[n2:]
    n_text = text.numel()
    with on_device(dev) as st:
        check(lib().dbn_edit_distance_pairs(pattern.data_ptr(), pattern.shape[1], pat_len.data_ptr(), text.data_ptr() if n_text else None, n_text,
                                            text_off.data_ptr(), None if text_len is None else text_len.data_ptr(), P, dist.data_ptr(), st),
              'edit_distance_pairs')
    return dist


class Lexicon:
    """A word list resident on the device, searched by edit distance.

    words: a list of strings (one group), or a list of lists (one group per image: ICDAR's "strong" per-image lexicons).
    An entry over 255 characters raises ValueError.  The device layout (dbn_lexicon_nearest of include/dbnet_hip.h: entries
    ordered by (group, length) in blocks of 64, position-major) is built here on the host without touching a GPU, and uploaded
    once on first use or by to(device).  An empty entry ('') is an entry like any other."""

    def __init__(self, words, classes, device=None):
        words = list(words)
        groups = [words] if all(isinstance(w, str) for w in words) else [list(g) for g in words]
        for g in groups:
            for w in g:
                if not isinstance(w, str):
                    raise TypeError('lexicon entries must be strings, got %r' % (type(w).__name__, ))
                if len(w) > MAX_ENTRY:
                    raise ValueError('a lexicon entry of %d characters; at most %d' % (len(w), MAX_ENTRY))
        self.classes, self.groups = classes, groups
        blocks, ent_len, ent_idx, blk_off, grp_blk = [], [], [], [0], [0]
        for g in groups:
            data, off = classes.encode(g)
            data = np.concatenate([data, np.full(1, NO_CLASS, np.uint8)])
            ln = np.diff(off).astype(np.int64)
            order = np.argsort(ln, kind='stable')
            for e0 in range(0, len(g), BLOCK):
                sel = order[e0:e0 + BLOCK]
                rows = -(-int(ln[sel].max()) // 4) * 4
                pos = np.arange(rows, dtype=np.int64)[:, None]
                blk = np.full((rows, BLOCK), NO_CLASS, np.uint8)
                blk[:, :len(sel)] = np.where(pos < ln[sel][None, :], data[np.minimum(off[sel][None, :] + pos, len(data) - 1)], NO_CLASS)
                blocks.append(blk.reshape(-1))
                blk_off.append(blk_off[-1] + blk.size)
                pad = np.full(BLOCK - len(sel), -1, np.int64)
                ent_len.append(np.concatenate([ln[sel], pad]))
                ent_idx.append(np.concatenate([sel, pad]))
            grp_blk.append(len(blocks))
        if blk_off[-1] > _INT_MAX:
            raise ValueError('the lexicon needs %d bytes; at most %d' % (blk_off[-1], _INT_MAX))
        cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)  # noqa: E731
        self.data, self.ent_len, self.ent_idx = cat(blocks, np.uint8), cat(ent_len, np.int32), cat(ent_idx, np.int32)
        self.blk_off, self.grp_blk = np.array(blk_off, np.int32), np.array(grp_blk, np.int32)
        self.n_blocks = len(blocks)
        self.max_blocks = int(np.diff(self.grp_blk).max())
        self._on = {}
        if device is not None:
            self.to(device)

    @property
    def n_groups(self):
        return len(self.groups)

    def word(self, group, index):
        """the entry `index` of `group`, in the caller's order"""
        return self.groups[group][index]

    def host_entries(self, group):
        """what the layout holds for `group`: [(original index, classes uint8 [length])] in layout order"""
        out = []
        for b in range(int(self.grp_blk[group]), int(self.grp_blk[group + 1])):
            blk = self.data[self.blk_off[b]:self.blk_off[b + 1]].reshape(-1, BLOCK)
            for lane in range(BLOCK):
                n = int(self.ent_len[b * BLOCK + lane])
                if n >= 0:
                    out.append((int(self.ent_idx[b * BLOCK + lane]), blk[:n, lane].copy()))
        return out

    def to(self, device):
        self._tables(cuda_device('Lexicon', device))
        return self

    def _tables(self, dev):
        """one upload: ent_len | ent_idx | blk_off | grp_blk | data -> their device views"""
        if dev not in self._on:
            ints = [self.ent_len, self.ent_idx, self.blk_off, self.grp_blk]
            up = upload(np.concatenate([a.view(np.uint8) for a in ints] + [self.data]), dev)
            views, at = [], 0
            for a in ints:
                views.append(up[at:at + a.nbytes].view(torch.int32))
                at += a.nbytes
            self._on[dev] = views + [up[at:]]
        return self._on[dev]

    def _group(self, group, K, dev):
        if group is None:
            if self.n_groups != 1:
                raise ValueError('the lexicon has %d groups: every query needs its group' % self.n_groups)
            return None
        if isinstance(group, torch.Tensor):
            group = group.to(device=dev, dtype=torch.int32).contiguous()
        else:
            group = upload(np.asarray(group, dtype=np.int32), dev)
        if group.shape != (K, ):
            raise ValueError('group must have shape [%d], got %s' % (K, tuple(group.shape)))
        return group

    def nearest(self, codes, count, group=None, head=None):
        """codes [K, T], count [K] as greedy_decode returns them (T <= 64) -> (index int32 [K], distance int32 [K]) on the
        device, no host synchronisation: of the query's group the entry with the smallest edit distance and, among equals,
        the smallest index in the caller's order within the group.  group: None (a lexicon of one group), a host sequence or
        an int32 device tensor [K]; a query whose group is empty or outside 0 .. n_groups - 1 gets (-1, -1).  K = 0: nothing
        is launched."""
        _check_codes(codes, count, 'Lexicon.nearest')
        K, dev = codes.shape[0], codes.device
        index = torch.empty((K, ), dtype=torch.int32, device=dev)
        dist = torch.empty((K, ), dtype=torch.int32, device=dev)
        if K == 0:
            return index, dist
        group = self._group(group, K, dev)
        query, qlen = _pattern_of(codes, count, self.classes, head)
        ent_len, ent_idx, blk_off, grp_blk, data = self._tables(dev)
        ws = torch.empty((lib().dbn_lexicon_ws_bytes(K) // 8, ), dtype=torch.int64, device=dev)
        nb = self.n_blocks
        with on_device(dev) as st:
            check(lib().dbn_lexicon_nearest(query.data_ptr(), query.shape[1], qlen.data_ptr(), None if group is None else group.data_ptr(), K,
                                            data.data_ptr() if nb else None, blk_off.data_ptr(), ent_len.data_ptr() if nb else None,
                                            ent_idx.data_ptr() if nb else None, grp_blk.data_ptr(), self.n_groups, nb, self.max_blocks, ws.data_ptr(),
                                            index.data_ptr(), dist.data_ptr(), st), 'lexicon_nearest')
        return index, dist

    def correct(self, codes, count, group=None, max_distance=None, head=None):
        """nearest(), then one device-to-host copy -> a list of K (word, distance): the entry, or None when the group has no
        entry (distance -1) or none within max_distance"""
        index, dist = self.nearest(codes, count, group, head)
        cols = [index, dist] + ([group.to(device=index.device, dtype=torch.int32)] if isinstance(group, torch.Tensor) else [])
        host = torch.stack(cols, 1).cpu().numpy()
        groups = host[:, 2] if isinstance(group, torch.Tensor) else np.zeros(len(host), np.int64) if group is None else np.asarray(group)
        return self.words_of(host[:, 0], host[:, 1], groups, max_distance)

    def words_of(self, index, dist, groups, max_distance=None):
        """host (index, distance, group) of nearest() -> [(word | None, distance)]"""
        out = []
        for i, d, g in zip(np.asarray(index).tolist(), np.asarray(dist).tolist(), np.asarray(groups).tolist()):
            near = i >= 0 and (max_distance is None or d <= max_distance)
            out.append((self.groups[g][i] if near else None, d))
        return out


class TextSpottingEvaluator:
    """End-to-end text spotting: DetectionIoUEvaluator's geometry (overlaps, greedy matching, don't-cares, pairs), then a
    matched pair is correct only if the detection's text equals the ground truth's, compared in the folded classes of
    TextClasses (case_sensitive=False: ICDAR's comparison).

    Per image: everything DetectionIoUEvaluator reports under its own names, except that its precision / recall / hmean
    move to det_precision / det_recall / det_hmean; `pairs` with 'correct' and 'distance' added; detCorrect; precision =
    detCorrect / detCare, recall = detCorrect / gtCare and their hmean, with the zero-denominator rules of the detection
    metric (no care GT: recall 1 and precision 1 without care detections, else 0; no care detection: precision 0); and
    nedSum, the sum over the image's pairs of distance / max(len_gt, len_det, 1), which combine_results needs for '1-ned'.

    Limits: the texts of one evaluate_batch call are mapped to classes by a TextClasses of their own, so the matched texts of
    one call may hold at most 255 distinct characters (after folding), and of every pair one text has at most 64 characters;
    beyond either, evaluate_batch raises ValueError.  Passing distances= lifts both."""

    def __init__(self, iou_constraint=0.5, area_precision_constraint=0.5, case_sensitive=False):
        self.detection = DetectionIoUEvaluator(iou_constraint, area_precision_constraint)
        self.case_sensitive = bool(case_sensitive)

    def evaluate_image(self, gt, pred):
        return self.evaluate_batch([gt], [pred])[0]

    def evaluate_batch(self, gts, preds, overlaps=None, distances=None, device=None):
        """gts: per image a list of {'points', 'ignore', 'text'}; preds: per image a list of {'points', 'text'}.  overlaps:
        polygon_overlaps' result for them (computed on the device when None).  distances: per image the edit distance of
        every pair, in the order of `pairs` (computed when None: all pairs of the batch in ONE edit_distances launch and one
        copy back; of a pair at least one text must have at most 64 characters)."""
        base = self.detection.evaluate_batch(gts, preds, overlaps=overlaps, device=device)
        texts = [[(str(gts[n][p['gt']]['text']), str(preds[n][p['det']]['text'])) for p in r['pairs']] for n, r in enumerate(base)]
        if distances is None:
            flat = [t for ts in texts for t in ts]
            if flat:
                classes = TextClasses('', self.case_sensitive)
                try:
                    dev_dist = edit_distances([g for g, _ in flat], [d for _, d in flat], classes, device=device)
                except ValueError as e:
                    raise ValueError('TextSpottingEvaluator: the matched texts of one batch are beyond what one launch scores (%s); '
                                     'evaluate fewer images per call, or pass distances=' % e) from e
                host = dev_dist.cpu().numpy().tolist()
            else:
                host = []
            distances, at = [], 0
            for ts in texts:
                distances.append(host[at:at + len(ts)])
                at += len(ts)
        out = []
        for r, ts, ds in zip(base, texts, distances):
            if len(ds) != len(ts):
                raise ValueError('%d distances for %d pairs' % (len(ds), len(ts)))
            r = dict(r)
            r['det_precision'], r['det_recall'], r['det_hmean'] = r['precision'], r['recall'], r['hmean']
            r['pairs'] = [dict(p, correct=int(d) == 0, distance=int(d)) for p, d in zip(r['pairs'], ds)]
            correct = sum(p['correct'] for p in r['pairs'])
            gc, dc = r['gtCare'], r['detCare']
            if gc == 0:
                recall, precision = 1.0, (0.0 if dc > 0 else 1.0)
            else:
                recall, precision = float(correct) / gc, (0.0 if dc == 0 else float(correct) / dc)
            r['detCorrect'] = correct
            r['precision'], r['recall'] = precision, recall
            r['hmean'] = 0.0 if precision + recall == 0 else 2.0 * precision * recall / (precision + recall)
            r['nedSum'] = float(sum(int(d) / max(len(g), len(t), 1) for (g, t), d in zip(ts, ds)))
            out.append(r)
        return out

    @staticmethod
    def combine_results(results):
        """-> the end-to-end precision / recall / hmean, the detection-only det_precision / det_recall / det_hmean, and
        '1-ned' = 1 - (the sum over pairs of distance / max(len_gt, len_det, 1) + unmatched care GTs + unmatched care
        detections) / (pairs + those two counts); 1.0 when that denominator is 0"""
        gc = sum(r['gtCare'] for r in results)
        dc = sum(r['detCare'] for r in results)
        matched = sum(r['detMatched'] for r in results)
        correct = sum(r['detCorrect'] for r in results)

        def prh(hits):
            R = 0 if gc == 0 else float(hits) / gc
            P = 0 if dc == 0 else float(hits) / dc
            return P, R, 0 if R + P == 0 else 2 * R * P / (R + P)

        P, R, H = prh(correct)
        dP, dR, dH = prh(matched)
        pairs = sum(len(r['pairs']) for r in results)
        miss = (gc - matched) + (dc - matched)
        ned = 1.0 if pairs + miss == 0 else 1.0 - (sum(r['nedSum'] for r in results) + miss) / (pairs + miss)
        return {'precision': P, 'recall': R, 'hmean': H, 'det_precision': dP, 'det_recall': dR, 'det_hmean': dH, '1-ned': ned}
