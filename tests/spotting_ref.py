"""Restatements for the edit distances, the lexicon search and the end-to-end score of csrc/lexicon.hip
(db_text_minimal_amd/spotting.py).  All of it is exact in integers.

  dp_pairs / dp / dp_lexicon   the plain Wagner-Fischer dynamic programme in numpy, vectorised over pairs (over the entries of
                               a lexicon); class 255 matches nothing
  myers                        the bit-vector recurrence of the kernels in Python integers, the pattern in one 64-bit word
  nearest                      smallest distance, then smallest index
  spotting_image / combine     the end-to-end arithmetic on given overlaps and texts (matching: eval_ref.iou_image)
"""
import numpy as np

import eval_ref as E

NO_CLASS = 255
M64 = (1 << 64) - 1


def padded(rows, fill=NO_CLASS):
    """list of P integer sequences -> (uint8-valued int array [P, max(longest, 1)], lengths [P])"""
    ln = np.array([len(r) for r in rows], np.int64)
    out = np.full((len(rows), max(int(ln.max()) if len(rows) else 0, 1)), fill, np.int64)
    for i, r in enumerate(rows):
        out[i, :len(r)] = np.asarray(r, np.int64)
    return out, ln


def dp_pairs(a, la, b, lb):
    """a [P, Ma], la [P], b [P, Mb], lb [P] -> the Levenshtein distance of a[p, :la[p]] and b[p, :lb[p]], int64 [P].
    Row i of the table is formed from row i - 1 for all pairs and all columns at once: the insertion chain
    row[j] = min(row[j], row[j - 1] + 1) is j + the running minimum of row[k] - k."""
    a, b, la, lb = np.asarray(a, np.int64), np.asarray(b, np.int64), np.asarray(la, np.int64), np.asarray(lb, np.int64)
    P, Mb = b.shape
    cols = np.arange(Mb + 1, dtype=np.int64)[None, :]
    prev = np.broadcast_to(cols, (P, Mb + 1)).copy()
    out = np.where(la == 0, lb, -1)
    for i in range(1, int(la.max()) + 1 if P else 0):
        ai = a[:, i - 1][:, None]
        cost = ((ai != b) | (ai == NO_CLASS) | (b == NO_CLASS)).astype(np.int64)
        cur = np.empty_like(prev)
        cur[:, 0] = i
        cur[:, 1:] = np.minimum(prev[:, 1:] + 1, prev[:, :-1] + cost)
        cur = np.minimum.accumulate(cur - cols, axis=1) + cols
        hit = la == i
        out[hit] = cur[hit, lb[hit]]
        prev = cur
    return out


def dp(x, y):
    """one pair of integer sequences"""
    a, la = padded([x])
    b, lb = padded([y])
    return int(dp_pairs(a, la, b, lb)[0])


def dp_lexicon(query, entries):
    """one query against every entry: int64 [len(entries)]"""
    b, lb = padded(entries)
    a, la = padded([query])
    return dp_pairs(np.repeat(a, len(entries), 0), np.repeat(la, len(entries)), b, lb)


def myers(pattern, text):
    """The kernels' recurrence.  pattern: at most 64 classes; text: any length."""
    m = len(pattern)
    assert m <= 64
    if m == 0:
        return len(text)
    peq = {}
    for j, c in enumerate(pattern):
        if c != NO_CLASS:
            peq[c] = peq.get(c, 0) | (1 << j)
    pv, mv, score, top = M64, 0, m, 1 << (m - 1)
    for c in text:
        eq = peq.get(c, 0) if c != NO_CLASS else 0
        xv = eq | mv
        xh = ((((eq & pv) + pv) & M64) ^ pv) | eq
        ph = mv | (~(xh | pv) & M64)
        mh = pv & xh
        score += (ph & top) != 0
        score -= (mh & top) != 0
        ph = ((ph << 1) | 1) & M64
        mh = (mh << 1) & M64
        pv = mh | (~(xv | ph) & M64)
        mv = ph & xv
    return score


def nearest(query, entries):
    """(index, distance) of the nearest entry: the smallest distance, then the smallest index; (-1, -1) for no entries"""
    if not len(entries):
        return -1, -1
    d = dp_lexicon(query, entries)
    i = int(np.argmin(d))  # (the first minimum)
    return i, int(d[i])


def fold(text, case_sensitive=False):
    return list(text) if case_sensitive else [ch.upper() for ch in text]


def text_distance(x, y, case_sensitive=False):
    """the Levenshtein distance of two strings in folded characters"""
    fx, fy = fold(x, case_sensitive), fold(y, case_sensitive)
    ids = {ch: i for i, ch in enumerate(dict.fromkeys(fx + fy))}
    return dp([ids[c] for c in fx], [ids[c] for c in fy])


def spotting_image(inter, ga, da, gts, preds, case_sensitive=False, distances=None, **constraints):
    """one image on given overlaps: eval_ref.iou_image's matching, then the transcription of every pair"""
    r = E.iou_image(inter, ga, da, [bool(g['ignore']) for g in gts], **constraints)
    r['det_precision'], r['det_recall'], r['det_hmean'] = r['precision'], r['recall'], r['hmean']
    pairs, ned = [], 0.0
    for j, p in enumerate(r['pairs']):
        g, t = gts[p['gt']]['text'], preds[p['det']]['text']
        d = text_distance(g, t, case_sensitive) if distances is None else int(distances[j])
        pairs.append(dict(p, correct=d == 0, distance=d))
        ned += d / max(len(g), len(t), 1)
    correct = sum(p['correct'] for p in pairs)
    gc, dc = r['gtCare'], r['detCare']
    if gc == 0:
        rec, prec = 1.0, (0.0 if dc > 0 else 1.0)
    else:
        rec, prec = correct / gc, (0.0 if dc == 0 else correct / dc)
    r.update(pairs=pairs, detCorrect=correct, precision=prec, recall=rec, hmean=0.0 if prec + rec == 0 else 2.0 * prec * rec / (prec + rec),
             nedSum=ned)
    return r


def combine(results):
    gc, dc = sum(r['gtCare'] for r in results), sum(r['detCare'] for r in results)
    matched, correct = sum(r['detMatched'] for r in results), sum(r['detCorrect'] for r in results)
    out = {}
    for tag, hits in (('', correct), ('det_', matched)):
        R = 0 if gc == 0 else hits / gc
        P = 0 if dc == 0 else hits / dc
        out.update({tag + 'precision': P, tag + 'recall': R, tag + 'hmean': 0 if P + R == 0 else 2 * P * R / (P + R)})
    pairs = sum(len(r['pairs']) for r in results)
    miss = (gc - matched) + (dc - matched)
    out['1-ned'] = 1.0 if pairs + miss == 0 else 1.0 - (sum(r['nedSum'] for r in results) + miss) / (pairs + miss)
    return out
