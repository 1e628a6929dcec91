"""numpy restatement of db_text_minimal_amd.recognise: the recogniser's input from uint8 crops (integer grey, the float32
normalisation), and the greedy decode of predict() (test_ocr.py:59-108) with fp64 probabilities and Python loops for the
collapse.  Written from the formulas, not from the kernels."""
import numpy as np

BLANK, EOS = 0, 1


def grey(crops, bgr=False):
    """PIL convert('L') of uint8 [..., 3]: (19595 R + 38470 G + 7471 B + 32768) >> 16 in integers"""
    c = crops.astype(np.int64)
    w = (7471, 38470, 19595) if bgr else (19595, 38470, 7471)
    return ((w[0] * c[..., 0] + w[1] * c[..., 1] + w[2] * c[..., 2] + 32768) >> 16).astype(np.uint8)


def normalise(g):
    """ToTensor then sub_(0.5).div_(0.5) of uint8 values, in float32 in that order"""
    return (g.astype(np.float32) / np.float32(255) - np.float32(0.5)) / np.float32(0.5)


def words_to_input(crops, rgb=False, bgr=False):
    """uint8 [K, h, w, 3] -> float32 [K, 1 | 3, h, w]"""
    if rgb:
        return normalise(np.ascontiguousarray(crops.transpose(0, 3, 1, 2)))
    return normalise(grey(crops, bgr))[:, None]


def steps(logits):
    """logits [B, T, C] (any float type, taken to fp64 exactly) -> (k int64 [B, T], p fp64 [B, T]): the first index of the
    maximum (of the first NaN in a row that has one) and 1 / sum exp(x - max)"""
    x = np.asarray(logits, np.float64)
    with np.errstate(all='ignore'):
        k = np.argmax(x, axis=2)  # numpy: the first maximum, a NaN counting as one
        m = np.max(x, axis=2, keepdims=True)
        p = 1.0 / np.exp(x - m).sum(axis=2)
    return k, p


def collapse(k, p, mode, lengths=None):
    """-> (codes int32 [B, T] packed left and -1 after, count int32 [B], score fp64 [B])"""
    B, T = k.shape
    codes = np.full((B, T), -1, np.int32)
    count = np.zeros(B, np.int32)
    score = np.ones(B, np.float64)
    for b in range(B):
        n = T if lengths is None else min(max(int(lengths[b]), 0), T)
        kb, pb = k[b].tolist(), p[b].tolist()  # Python ints and floats (fp64)
        kept, s = [], 1.0
        if mode == 'ctc':
            for t in range(n):
                if kb[t] != BLANK and (t == 0 or kb[t] != kb[t - 1]):
                    kept.append(kb[t])
                s = s * pb[t]
        else:
            for t in range(n):
                if kb[t] == EOS:
                    break
                kept.append(kb[t])
                s = s * pb[t]
        codes[b, :len(kept)] = kept
        count[b] = len(kept)
        score[b] = s
    return codes, count, score


def greedy_decode(logits, mode='ctc', lengths=None):
    k, p = steps(logits)
    return collapse(k, p, mode, lengths)


def strings(codes, count, table):
    return [''.join(table[c] for c in codes[b, :count[b]]) for b in range(codes.shape[0])]
