"""GPU (-m gpu): csrc/recognise.hip through db_text_minimal_amd.recognise against the restatement tests/recognise_ref.py:
words_to_input bit for bit, the codes and counts of greedy_decode exactly, its scores within a derived bound, and
recognize_words end to end from a probability map with stub recognisers."""
import numpy as np
import pytest
import torch

from db_text_minimal_amd import (AttnLabelConverter, CTCLabelConverter, crop_words, detect_boxes, greedy_decode, image_collate, recognize_words,
                                 words_to_input)
from db_text_minimal_amd import recognise as Rc
from db_text_minimal_amd._lib import check, lib
import recognise_ref as R
from gpu_util import DEV, stream

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
CHARS = '0123456789abcdefghijklmnopqrstuvwxyz'


def _bits(t):
    """the bit patterns of a float tensor, as a host integer array"""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


def _wide(t):
    """a host float array holding the tensor's values exactly"""
    return t.detach().cpu().to(torch.float64).numpy()


# ---- words_to_input -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('K, size', [(0, (32, 100)), (1, (32, 100)), (7, (32, 100)), (5, (17, 41)), (3, (1, 1)), (9, (3, 5)), (2, (64, 256))])
def test_words_to_input_bit_exact(K, size, dtype):
    rng = np.random.default_rng(K * 100 + size[0])
    crops = rng.integers(0, 256, (K, size[0], size[1], 3), dtype=np.uint8)
    dev = torch.from_numpy(crops).to(DEV)
    for rgb, bgr in ((False, False), (False, True), (True, False)):
        out = words_to_input(dev, rgb=rgb, bgr=bgr, dtype=dtype)
        torch.cuda.synchronize()
        assert out.shape == (K, 3 if rgb else 1, size[0], size[1]) and out.dtype == dtype and out.is_cuda
        want = torch.from_numpy(R.words_to_input(crops, rgb, bgr)).to(dtype)  # torch's conversion rounds to nearest even
        assert np.array_equal(_bits(out), _bits(want)), (rgb, bgr)
    assert np.array_equal(dev.cpu().numpy(), crops)


def test_words_to_input_more_than_65535_crops():
    rng = np.random.default_rng(1)
    crops = rng.integers(0, 256, (70001, 4, 9, 3), dtype=np.uint8)
    dev = torch.from_numpy(crops).to(DEV)
    for rgb in (False, True):
        out = words_to_input(dev, rgb=rgb)
        assert np.array_equal(_bits(out), _bits(torch.from_numpy(R.words_to_input(crops, rgb))))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('rgb', [False, True])
def test_words_to_input_overwrites_poison_and_keeps_guards(rgb, dtype):
    """through the C entry point into a caller's buffer, at an offset that breaks the 16-byte alignment of the stores"""
    rng = np.random.default_rng(7)
    for (K, h, w), shift in (((3, 5, 7), 0), ((2, 32, 100), 0), ((2, 32, 100), 1), ((4, 6, 6), 3)):
        crops = rng.integers(0, 256, (K, h, w, 3), dtype=np.uint8)
        src = torch.from_numpy(np.concatenate([np.zeros(shift, np.uint8), crops.reshape(-1)])).to(DEV)[shift:]
        n = K * (3 if rgb else 1) * h * w
        guard = 64
        poison = float('nan') if dtype != torch.float32 else 12345.0
        buf = torch.full((guard + shift + n + guard, ), poison, dtype=dtype, device=DEV)
        out = buf[guard + shift:guard + shift + n]
        check(lib().dbn_words_to_input(Rc._AT[dtype], src.data_ptr(), K * h * w, h * w, int(rgb), 0, Rc._table_on(src.device).data_ptr(),
                                       out.data_ptr(), stream()), 'words_to_input')
        torch.cuda.synchronize()
        want = torch.from_numpy(R.words_to_input(crops, rgb)).to(dtype).reshape(-1)
        assert np.array_equal(_bits(out), _bits(want)), (K, h, w, shift)
        fresh = torch.full((guard + shift, ), poison, dtype=dtype)
        assert np.array_equal(_bits(buf[:guard + shift]), _bits(fresh)) and np.array_equal(_bits(buf[guard + shift + n:]), _bits(fresh[:guard]))


# ---- greedy_decode: codes and counts --------------------------------------------------------------------------------------
def _tied_logits(rng, B, T, C, dtype):
    """small integers, exact in every dtype: equal maxima at several indices in most rows; plus rows of all-equal values,
    +-inf and NaN"""
    x = rng.integers(-2, 3, (B, T, C)).astype(np.float32)
    x[..., 0] += rng.integers(0, 2, (B, T))  # blanks ...
    if C > 1:
        x[..., 1] += rng.integers(0, 2, (B, T))  # ... and [s] often enough
    flat = x.reshape(B * T, C)
    rows = rng.permutation(B * T)
    n = max(1, B * T // 64)
    flat[rows[:n]] = 1.0                                                   # all equal
    flat[rows[n:2 * n]] = -np.inf                                          # all -inf
    for r in rows[2 * n:3 * n]:
        flat[r, rng.integers(0, C, 2)] = np.inf                            # +inf, maybe twice
    for r in rows[3 * n:4 * n]:
        flat[r, rng.integers(0, C, 3)] = np.nan                            # NaNs
        flat[r, rng.integers(0, C)] = np.inf
    for r in rows[4 * n:5 * n]:
        flat[r, rng.integers(0, C, 2)] = -np.inf
    return torch.from_numpy(x).to(dtype)


def _check_exact(logits, mode, lengths=None):
    dev = logits.to(DEV)
    keep = dev.clone()
    len_dev = None if lengths is None else torch.from_numpy(lengths).to(DEV)
    codes, count, score = greedy_decode(dev, mode, len_dev)
    codes2, count2, score2 = greedy_decode(dev, mode, len_dev)
    torch.cuda.synchronize()
    B, T, C = logits.shape
    assert codes.shape == (B, T) and codes.dtype == torch.int32 and count.shape == (B, ) and count.dtype == torch.int32
    assert score.shape == (B, ) and score.dtype == torch.float32
    want_codes, want_count, want_score = R.greedy_decode(_wide(logits), mode, lengths)
    assert np.array_equal(count.cpu().numpy(), want_count)
    assert np.array_equal(codes.cpu().numpy(), want_codes)
    assert np.array_equal(np.isnan(score.cpu().numpy()), np.isnan(want_score))
    assert torch.equal(codes, codes2) and torch.equal(count, count2) and np.array_equal(_bits(score), _bits(score2))  # two runs, bit for bit
    assert np.array_equal(_bits(dev), _bits(keep))  # the input is not written
    return score.cpu().numpy(), want_score


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('mode', ['ctc', 'attn'])
@pytest.mark.parametrize('B, T, C', [(37, 1, 2), (300, 26, 2), (64, 26, 37), (9600, 26, 37), (3, 1024, 37), (70, 26, 96), (5, 1024, 96),
                                     (6, 26, 6625), (41, 1, 6625), (2, 1024, 6625), (2600, 26, 5), (9, 26, 512), (9, 26, 513), (11, 70, 33)])
def test_codes_and_counts_exact(B, T, C, mode, dtype):
    rng = np.random.default_rng(B * 7 + T * 3 + C)
    logits = _tied_logits(rng, B, T, C, dtype)
    _check_exact(logits, mode)
    lengths = rng.integers(0, T + 1, B).astype(np.int32)  # ragged, zeros included
    lengths[:3] = [0, T, T // 2][:min(B, 3)]
    _check_exact(logits, mode, lengths)


def test_more_than_65535_steps_and_lengths_outside_0_T():
    rng = np.random.default_rng(12)
    logits = _tied_logits(rng, 70000, 3, 11, torch.float32)
    lengths = rng.integers(-2, 6, 70000).astype(np.int32)  # clamped to 0 .. T
    _check_exact(logits, 'ctc', lengths)
    _check_exact(logits, 'attn', lengths)


@pytest.mark.parametrize('dtype', DTYPES)
def test_logits_at_an_unaligned_offset(dtype):
    """a contiguous slice of a larger tensor: its first row starts wherever the slice does"""
    rng = np.random.default_rng(3)
    for T, C in ((3, 37), (5, 6625), (1, 7)):
        big = _tied_logits(rng, 9, T, C, dtype)
        flat = torch.cat([torch.zeros(1, dtype=dtype), big.reshape(-1)]).to(DEV)
        view = flat[1:].view(9, T, C)
        assert view.data_ptr() % 16 != 0
        codes, count, _ = greedy_decode(view, 'ctc')
        want_codes, want_count, _ = R.greedy_decode(_wide(big), 'ctc')
        assert np.array_equal(codes.cpu().numpy(), want_codes) and np.array_equal(count.cpu().numpy(), want_count)


def _one_hot(seqs, C):
    x = np.zeros((len(seqs), len(seqs[0]), C), np.float32)
    for b, s in enumerate(seqs):
        x[b, np.arange(len(s)), s] = 9.0
    return torch.from_numpy(x)


def test_kept_step_rules_on_constructed_sequences():
    T = 70  # more than one 64-step chunk: the repeat rule and the [s] search cross the boundary
    seqs = [[0] * T, [3] * T, [3] * 63 + [3] * 7, [2] * 63 + [4] * 7, [0, 5] * 35, [5, 5, 0, 5, 6, 6, 0] * 10, [4] * 64 + [0] + [4] * 5,
            list(range(2, 9)) * 10]
    logits = _one_hot(seqs, 9)
    codes, count, score = greedy_decode(logits.to(DEV), 'ctc')
    want = [[], [3], [3], [2, 4], [5] * 35, [5, 5, 6] * 10, [4, 4], list(range(2, 9)) * 10]
    assert count.tolist() == [len(w) for w in want]
    for b, w in enumerate(want):
        assert codes[b].tolist() == w + [-1] * (T - len(w)), b
    ref = R.greedy_decode(logits.numpy(), 'ctc')
    assert np.array_equal(codes.cpu().numpy(), ref[0])
    seqs = [[1] + [2] * (T - 1), [2] * T, [3] * 64 + [1] + [4] * 5, [0, 4] * 32 + [4, 4, 1, 1, 4, 4], [5] * 63 + [1] + [5] * 6, [6, 1] * 35]
    logits = _one_hot(seqs, 9)
    codes, count, score = greedy_decode(logits.to(DEV), 'attn')
    want = [[], [2] * T, [3] * 64, [0, 4] * 32 + [4, 4], [5] * 63, [6]]
    assert count.tolist() == [len(w) for w in want]
    for b, w in enumerate(want):
        assert codes[b].tolist() == w + [-1] * (T - len(w)), b
    assert score[0].item() == 1.0  # the empty product
    p = 1.0 / (1.0 + 8 * np.exp(-9.0))
    np.testing.assert_allclose(score.cpu().numpy()[1:], [p ** len(w) for w in want[1:]], rtol=T * 17 * 2.0 ** -23)


def test_nan_rows():
    """a row with a NaN: k = the index of its first NaN (torch.max on the CPU), p = NaN, so the score is NaN once such a
    step enters it"""
    nan = float('nan')
    x = torch.zeros(4, 3, 6)
    x[:, :, 2] = 5.0                       # every step reads 2 ...
    x[1, 1, 4], x[1, 1, 3] = nan, nan      # ... but b = 1, t = 1: the first NaN is at 3
    x[2, 2, 0] = nan                       # a NaN at the blank
    x[3, 0, 1], x[3, 1, 5] = 7.0, nan      # attn: [s] first, the NaN after it never enters
    for dtype in DTYPES:
        dev = x.to(dtype).to(DEV)
        assert torch.equal(x.max(2)[1], torch.from_numpy(R.steps(x.numpy())[0]))
        codes, count, score = greedy_decode(dev, 'ctc')
        assert codes.tolist() == [[2, -1, -1], [2, 3, 2], [2, -1, -1], [1, 5, 2]] and count.tolist() == [1, 3, 1, 3]
        assert torch.isnan(score).tolist() == [False, True, True, True]
        codes, count, score = greedy_decode(dev, 'attn')
        assert codes.tolist() == [[2, 2, 2], [2, 3, 2], [2, 2, 0], [-1, -1, -1]] and count.tolist() == [3, 3, 3, 0]
        assert torch.isnan(score).tolist() == [False, True, True, False] and score[3].item() == 1.0


# ---- greedy_decode: scores ----------------------------------------------------------------------------------------------
def _margin_logits(rng, B, T, C, dtype):
    """one class ahead of the others by a margin that keeps the fp64 score of a whole sequence above 1e-30: with the
    others <= 0 and the winner >= margin, -ln p_t <= (C - 1) exp(-margin), so T (C - 1) exp(-margin) <= 60 < ln 1e30"""
    margin = max(0.0, float(np.log(T * (C - 1) / 60.0))) + 0.25  # 0.25: the 16-bit rounding of values below 16 moves them by < 0.07
    x = -rng.uniform(0, 4, (B, T, C)).astype(np.float32)
    win = rng.integers(0, C, (B, T))
    np.put_along_axis(x, win[..., None], (margin + rng.uniform(0, 2, (B, T, 1))).astype(np.float32), axis=2)
    return torch.from_numpy(x).to(dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('mode', ['ctc', 'attn'])
@pytest.mark.parametrize('B, T, C', [(50, 1, 2), (50, 26, 2), (2000, 26, 37), (4, 1024, 37), (200, 26, 96), (3, 1024, 96), (40, 26, 6625),
                                     (2, 1024, 6625), (20, 40, 513)])
def test_scores_within_the_derived_bound(B, T, C, mode, dtype):
    """relative error <= len_b (C + 8) 2^-23 against the fp64 restatement: per step one subtraction, an exp good to 2 ulp
    (OCML's expf is documented at 1), C - 1 additions, a reciprocal, and one multiply into the score"""
    rng = np.random.default_rng(B + T + C)
    logits = _margin_logits(rng, B, T, C, dtype)
    lengths = rng.integers(0, T + 1, B).astype(np.int32)
    lengths[0] = T
    for ln in (None, lengths):
        got, want = _check_exact(logits, mode, ln)
        assert (want >= 1e-30).all() and (want <= 1.0).all()
        if mode == 'ctc':
            steps = np.full(B, T) if ln is None else ln
        else:
            steps = R.greedy_decode(_wide(logits), mode, ln)[1]  # the kept steps are the ones in the product
        tol = steps * (C + 8) * 2.0 ** -23
        err = np.abs(got.astype(np.float64) - want) / want
        print('B %d T %d C %d %s %s: worst relative error %.3e, worst error / bound %.3f' % (B, T, C, mode, dtype, err.max(),
                                                                                        (err / np.maximum(tol, 1e-300)).max()))
        assert (err <= tol).all(), (err.max(), tol[np.argmax(err - tol)])


# ---- recognize_words ------------------------------------------------------------------------------------------------------
class _StubCTC(torch.nn.Module):
    """a CTC-style recogniser: forward(image, text) -> [b, 26, C]; records what it was given"""

    def __init__(self, C, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.proj = torch.nn.Parameter(torch.randn(32, C, generator=g) * 4)
        self.calls, self.logits = [], []

    def features(self, image):
        b, c, h, w = image.shape
        assert (c, h, w) == (1, 32, 100)
        cols = image[:, 0, :, :78].float().reshape(b, 32, 26, 3).mean(3)  # 26 steps of three columns
        return cols.permute(0, 2, 1) @ self.proj                          # [b, 26, C]

    def forward(self, image, text):
        assert not torch.is_grad_enabled()
        self.calls.append((tuple(image.shape), tuple(text.shape), text.dtype, int(text.abs().sum())))
        out = self.features(image)
        out[:, 1::2, 0] += 6  # blanks between the letters
        self.logits.append(out)
        return out


class _StubAttn(_StubCTC):
    """an attention-style recogniser: forward(image, text, is_train=True) -> [b, text.shape[1], C]"""

    def forward(self, image, text, is_train=True):
        assert not torch.is_grad_enabled() and is_train is False
        self.calls.append((tuple(image.shape), tuple(text.shape), text.dtype, int(text.abs().sum())))
        out = self.features(image)[:, :text.shape[1]].contiguous()
        out[:, :, 0] -= 50  # no [GO]
        rows = torch.arange(out.shape[0], device=out.device)
        out[rows, 4 + (rows % 3) * 5, 1] += 100  # an [s] at step 4, 9 or 14 at the latest
        self.logits.append(out)
        return out


def _scene():
    """two probability maps with rectangles, images with texture, and what detect_boxes makes of them"""
    Hm, Wm, S = 128, 128, 2
    rects = [[((10, 40, 10, 20), 0.9), ((60, 110, 30, 45), 0.99), ((20, 70, 70, 80), 0.75), ((100, 102, 100, 102), 0.9), ((20, 50, 100, 115), 0.5)],
             [((5, 120, 5, 25), 0.95), ((30, 60, 60, 100), 0.72)]]
    pred = torch.zeros((2, 1, Hm, Wm), dtype=torch.float32)
    for n, rs in enumerate(rects):
        for (x0, x1, y0, y1), p in rs:
            pred[n, 0, y0:y1, x0:x1] = p
    res = detect_boxes(pred.to(DEV), dest_sizes=[(Hm * S, Wm * S)] * 2)
    rng = np.random.default_rng(8)
    imgs = [rng.integers(0, 256, (Hm * S, Wm * S, 3), dtype=np.uint8) for _ in range(2)]
    return res, image_collate([(i, [], None) for i in imgs])


@pytest.mark.parametrize('prediction', ['CTC', 'Attn'])
def test_recognize_words_end_to_end(prediction):
    res, batch = _scene()
    crops, index = crop_words(batch, res)
    kept = [[k for k in range(len(b)) if b[k].reshape(-1).astype(np.int64).sum() > 0] for b, _ in res]
    assert [len(k) for k in kept] == [3, 2] and index.tolist() == [[n, k] for n in range(2) for k in kept[n]]  # zero rows are dropped
    if prediction == 'CTC':
        conv, model, mode = CTCLabelConverter(CHARS), _StubCTC(37, 1).to(DEV), 'ctc'
    else:
        conv, model, mode = AttnLabelConverter(CHARS), _StubAttn(38, 2).to(DEV), 'attn'
    out = recognize_words(batch, res, model, conv, prediction=prediction, batch_size=2)
    assert [c[0][0] for c in model.calls] == [2, 2, 1] and all(c[1] == (c[0][0], 26) and c[2] == torch.long and c[3] == 0 for c in model.calls)
    logits = torch.cat(model.logits)
    codes, count, score = R.greedy_decode(_wide(logits), mode)
    want = R.strings(codes, count, conv.character)
    assert len(set(want)) == 5 and all(0 < len(w) for w in want) and (mode == 'ctc' or all(n < 15 for n in count))  # the stubs say something
    assert [len(o) for o in out] == [3, 2]
    flat = [w for o in out for w in o]
    for j, ((n, k), w) in enumerate(zip(index.tolist(), flat)):
        assert np.array_equal(w['box'], res[n][0][k]) and w['box'].dtype == np.int16
        assert w['pred'] == want[j] and isinstance(w['score'], float), (j, w, want[j])
        steps = 26 if mode == 'ctc' else count[j]
        assert score[j] >= 1e-30 and abs(w['score'] - score[j]) <= steps * (logits.shape[2] + 8) * 2.0 ** -23 * score[j], (j, w['score'], score[j])
    # the same from ready crops in one chunk, and with a score threshold: each against the logits the stub gave in that call
    # (the attention stub places its [s] by the row within a chunk)
    def restated():
        c, n, _ = R.greedy_decode(_wide(torch.cat(model.logits)), mode)
        model.calls.clear(), model.logits.clear()
        return R.strings(c, n, conv.character)

    restated()
    ready = recognize_words(crops, None, model, conv, prediction=prediction)
    assert len(model.calls) == 1 and [w['pred'] for w in ready] == restated() and all(w['box'] is None for w in ready)
    few = recognize_words(batch, res, model, conv, prediction=prediction, min_score=0.8)
    sel = [[j for j, (n, k) in enumerate(index.tolist()) if n == i and res[n][1][k] >= 0.8] for i in range(2)]
    assert [len(v) for v in sel] == [2, 1] and [w['pred'] for o in few for w in o] == restated()
    assert [[w['box'].tolist() for w in o] for o in few] == [[res[index[j][0]][0][index[j][1]].tolist() for j in v] for v in sel]
    none = recognize_words(batch, [np.zeros((0, 4, 2), np.int16)] * 2, model, conv, prediction=prediction)
    assert none == [[], []]
    # decode() of the device tensors: one copy, the same strings
    dc, dn, _ = greedy_decode(logits, mode)
    assert conv.decode(dc, dn) == want
