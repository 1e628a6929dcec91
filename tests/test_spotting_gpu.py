"""GPU (-m gpu): csrc/lexicon.hip through db_text_minimal_amd/spotting.py against the restatement tests/spotting_ref.py (DESIGN.md
section 42).  Everything is compared exactly: the distances of dbn_edit_distance_pairs and the (index, distance) of
dbn_lexicon_nearest against the plain dynamic programme, the two kernels against each other, the C entry points into guarded
and poisoned caller buffers, recognize_words(lexicon=) with a stub recogniser, and TextSpottingEvaluator on a hand-built batch."""
import numpy as np
import pytest
import torch

from db_text_minimal_amd import (CTCLabelConverter, Lexicon, TextClasses, TextSpottingEvaluator, edit_distances, image_collate, polygon_overlaps,
                                 recognize_words)
from db_text_minimal_amd._lib import check, lib
import spotting_ref as R
from gpu_util import DEV, stream

pytestmark = pytest.mark.gpu

CHARS = '0123456789abcdefghijklmnopqrstuvwxyz'
PATTERN_LENGTHS = [0, 1, 2, 31, 32, 33, 63, 64]
TEXT_LENGTHS = [0, 1, 7, 63, 64, 65, 255, 1000]
ALPHABETS = [2, 3, 36]


def classes():
    return TextClasses(CTCLabelConverter(CHARS))


def rand_words(rng, n, lo, hi, k):
    return [''.join(CHARS[c] for c in rng.integers(0, k, int(rng.integers(lo, hi + 1)))) for _ in range(n)]


def class_rows(words):
    return [[CHARS.index(ch) for ch in w] for w in words]


def device_codes(words, T=None):
    """strings over CHARS -> (codes int32 [P, T], count int32 [P]) as greedy_decode gives them for the CTC table: code = 1 + the
    character's index, -1 behind the word"""
    T = max([len(w) for w in words] + [1]) if T is None else T
    codes = np.full((len(words), T), -1, np.int32)
    for i, w in enumerate(words):
        codes[i, :len(w)] = [CHARS.index(ch) + 1 for ch in w]
    return torch.from_numpy(codes).to(DEV), torch.tensor([len(w) for w in words], dtype=torch.int32, device=DEV)


def dp_words(a, b):
    pa, la = R.padded(class_rows(a))
    pb, lb = R.padded(class_rows(b))
    return R.dp_pairs(pa, la, pb, lb)


# ---- pairs ------------------------------------------------------------------------------------------------------------------
def test_pairs_length_grid_in_one_launch():
    rng = np.random.default_rng(0)
    pats, texts = [], []
    for seed in range(3):
        for k in ALPHABETS:
            for m in PATTERN_LENGTHS:
                for n in TEXT_LENGTHS:
                    pats += rand_words(rng, 1, m, m, k)
                    t = rand_words(rng, 1, n, n, k)[0]
                    if seed == 2 and m and n >= m:  # a near copy of the pattern inside the text: small distances too
                        at = int(rng.integers(0, n - m + 1))
                        t = t[:at] + pats[-1] + t[at + m:]
                    texts.append(t)
    want = dp_words(pats, texts)
    assert len(want) == 576 and len(set(want.tolist())) > 30
    tc = classes()
    for a, b in ((pats, texts), (texts, pats), (device_codes(pats, 64), texts), (texts, device_codes(pats))):
        got = edit_distances(a, b, tc)
        assert got.dtype == torch.int32 and got.is_cuda and got.shape == (576, )
        assert np.array_equal(got.cpu().numpy(), want)
    assert [R.myers(p, t) for p, t in zip(class_rows(pats), class_rows(texts))] == want.tolist()


def test_pairs_carry_through_bits_31_32_and_63():
    pats, texts = [], []
    for m in (32, 33, 64):
        pats += ['a' * m, 'a' * m]
        texts += ['a' * m, 'a' * (m - 1) + 'b']
    tc = classes()
    assert edit_distances(pats, texts, tc).tolist() == [0, 1, 0, 1, 0, 1]
    assert edit_distances(device_codes(pats), device_codes(texts), tc).tolist() == [0, 1, 0, 1, 0, 1]


def test_pairs_class_255_matches_nothing():
    """code 0 ('[blank]') maps to class 255; as device codes it can stand on both sides"""
    tc = classes()
    rows = [[11, 0, 12], [0], [0, 0, 0, 0], [11, 12], [11, 0, 12]]
    others = [[11, 0, 12], [0], [0, 0, 0, 0, 0, 0], [11, 12], [11, 12]]

    def dev(rs):
        codes = np.full((len(rs), 6), -1, np.int32)
        for i, r in enumerate(rs):
            codes[i, :len(r)] = r
        return torch.from_numpy(codes).to(DEV), torch.tensor([len(r) for r in rs], dtype=torch.int32, device=DEV)

    got = edit_distances(dev(rows), dev(others), tc).tolist()
    assert got == [1, 1, 6, 0, 1]
    as_class = lambda rs: [[255 if c == 0 else c - 1 for c in r] for r in rs]  # noqa: E731
    assert got == [R.dp(x, y) for x, y in zip(as_class(rows), as_class(others))]
    # codes beyond the table and negative ones are 255 as well, never an index outside the table
    wild = (torch.tensor([[11, 1000, -5]], dtype=torch.int32, device=DEV), torch.tensor([3], dtype=torch.int32, device=DEV))
    assert edit_distances(wild, ['a'], tc).tolist() == [2]


def test_pairs_more_than_65535_pairs():
    rng = np.random.default_rng(2)
    a, b = rand_words(rng, 70001, 0, 3, 3), rand_words(rng, 70001, 0, 3, 3)
    got = edit_distances(a, b, classes())
    assert np.array_equal(got.cpu().numpy(), dp_words(a, b))


def test_pairs_arguments():
    tc = classes()
    got = edit_distances([], [], tc)
    assert got.shape == (0, ) and got.dtype == torch.int32 and got.is_cuda
    with pytest.raises(ValueError, match='both strings exceed 64'):
        edit_distances(['a' * 65], ['b' * 65], tc)
    with pytest.raises(ValueError, match='T = 65'):
        edit_distances(device_codes(['a'], 65), ['a'], tc)
    with pytest.raises(ValueError, match='1 strings against 2'):
        edit_distances(['a'], ['a', 'b'], tc)
    assert edit_distances(['a' * 65], ['b' * 3], tc).tolist() == [65]
    with pytest.raises(ValueError, match='head'):
        edit_distances(device_codes(['a']), ['a'], TextClasses(CHARS))
    assert edit_distances(device_codes(['a7']), ['A8'], TextClasses(CHARS), head=1).tolist() == [1]


# ---- nearest ----------------------------------------------------------------------------------------------------------------
def lexicon_words(rng, n):
    """n entries of lengths 0 .. 255 over two letters, drawn with repeats from a pool: ties exist, duplicates exist"""
    pool = rand_words(rng, max(n // 3, 1), 0, 255, 2) + rand_words(rng, max(n // 3, 1), 0, 12, 2)
    return [pool[i] for i in rng.integers(0, len(pool), n)]


def queries_for(rng, words):
    """lengths 0, 1, 32, 33, 64: random ones, and cuts of entries with one class changed"""
    qs = []
    for m in (0, 1, 32, 33, 64):
        qs += rand_words(rng, 1, m, m, 2)
        w = words[int(rng.integers(0, len(words)))][:m]
        qs.append(w[:-1] + 'c' if w else w)
    return qs


@pytest.mark.parametrize('n', [1, 63, 64, 65, 257, 1500])
def test_nearest_against_dp(n):
    rng = np.random.default_rng(n)
    words = lexicon_words(rng, n)
    qs = queries_for(rng, words)
    lex = Lexicon(words, classes())
    codes, count = device_codes(qs, 64)
    index, dist = lex.nearest(codes, count)
    assert index.dtype == dist.dtype == torch.int32 and index.is_cuda and index.shape == dist.shape == (len(qs), )
    want = [R.nearest(q, class_rows(words)) for q in class_rows(qs)]
    assert list(zip(index.tolist(), dist.tolist())) == want
    if n >= 257:
        assert any(words.index(words[i]) == i and words.count(words[i]) > 1 for i, _ in want)  # a tie was decided by the index
    assert lex.correct(codes, count, max_distance=3) == [(words[i] if d <= 3 else None, d) for i, d in want]


def test_nearest_more_than_65535_queries():
    rng = np.random.default_rng(5)
    words = ['ab', 'b', 'ab']
    qs = rand_words(rng, 70001, 0, 3, 2)
    index, dist = Lexicon(words, classes()).nearest(*device_codes(qs))
    d = np.stack([dp_words(qs, [w] * len(qs)) for w in words], 1)
    assert np.array_equal(index.cpu().numpy(), d.argmin(1)) and np.array_equal(dist.cpu().numpy(), d.min(1))
    assert set(index.tolist()) == {0, 1}  # entry 2 repeats entry 0 and never wins


def test_nearest_groups_and_group_tensor():
    rng = np.random.default_rng(6)
    groups = [lexicon_words(rng, 70), [], ['dog', 'dig', 'cat', '']]
    lex = Lexicon(groups, classes()).to(DEV)
    qs = ['dug', 'cot', '', 'abab', 'dug', 'dug', 'cat']
    group = [2, 2, 2, 0, 1, 0, 2]
    codes, count = device_codes(qs)
    want = [R.nearest(q, class_rows(groups[g])) for q, g in zip(class_rows(qs), group)]
    assert want[:3] == [(0, 1), (2, 1), (3, 0)] and want[4] == (-1, -1) and want[6] == (2, 0)
    index, dist = lex.nearest(codes, count, group)
    assert list(zip(index.tolist(), dist.tolist())) == want
    dev_group = torch.tensor([2, -1, 3, 0, 1, 1000, 2], dtype=torch.int32, device=DEV)
    index, dist = lex.nearest(codes, count, dev_group)
    want_dev = [want[0], (-1, -1), (-1, -1), want[3], (-1, -1), (-1, -1), want[6]]
    assert list(zip(index.tolist(), dist.tolist())) == want_dev
    assert lex.correct(codes, count, dev_group) == [('dog', 1), (None, -1), (None, -1), (groups[0][want[3][0]], want[3][1]), (None, -1), (None, -1),
                                                     ('cat', 0)]
    with pytest.raises(ValueError, match='3 groups'):
        lex.nearest(codes, count)
    with pytest.raises(ValueError, match='shape'):
        lex.nearest(codes, count, [0, 1])
    # K = 0, an empty lexicon, T > 64
    i0, d0 = lex.nearest(codes[:0], count[:0], [])
    assert i0.shape == d0.shape == (0, )
    none = Lexicon([], classes()).nearest(codes, count)
    assert none[0].tolist() == [-1] * 7 and none[1].tolist() == [-1] * 7
    with pytest.raises(ValueError, match='T = 65'):
        lex.nearest(*device_codes(['a'], 65), [0])


def test_the_two_kernels_agree():
    """nearest == the first minimum of edit_distances over all K x L pairs"""
    rng = np.random.default_rng(7)
    words = rand_words(rng, 150, 0, 255, 3) + rand_words(rng, 150, 0, 20, 3)
    qs = rand_words(rng, 25, 0, 64, 3) + rand_words(rng, 25, 0, 20, 3)
    K, L = len(qs), len(words)
    tc = classes()
    index, dist = Lexicon(words, tc).nearest(*device_codes(qs, 64))
    codes, count = device_codes(qs, 64)
    all_pairs = edit_distances((codes.repeat_interleave(L, 0), count.repeat_interleave(L)), words * K, tc).view(K, L).cpu().numpy()
    assert np.array_equal(dist.cpu().numpy(), all_pairs.min(1)) and np.array_equal(index.cpu().numpy(), all_pairs.argmin(1))
    assert len(set(dist.tolist())) > 5


# ---- the C entry points into caller buffers -----------------------------------------------------------------------------------
GUARD, POISON = 64, -123456789


def _guarded(n):
    buf = torch.full((GUARD + n + GUARD, ), POISON, dtype=torch.int32, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n):
    host = buf.cpu().numpy()
    return (host[:GUARD] == POISON).all() and (host[GUARD + n:] == POISON).all()


def test_pairs_entry_point_guards_and_poison():
    rng = np.random.default_rng(8)
    a, b = rand_words(rng, 203, 0, 64, 3), rand_words(rng, 203, 0, 150, 3)
    P, want = len(a), dp_words(a, b)
    tc = classes()
    pattern, pat_len = device_codes(a, 64)
    pattern = tc.lookup(pattern).contiguous()
    text, off = tc.encode(b)
    d_text, d_off = torch.from_numpy(text).to(DEV), torch.from_numpy(off).to(DEV)
    runs = []
    for _ in range(2):
        buf, out = _guarded(P)
        check(lib().dbn_edit_distance_pairs(pattern.data_ptr(), 64, pat_len.data_ptr(), d_text.data_ptr(), len(text), d_off.data_ptr(), None, P,
                                            out.data_ptr(), stream()), 'pairs')
        torch.cuda.synchronize()
        assert _guards_intact(buf, P)
        runs.append(out.cpu().numpy())
    assert np.array_equal(runs[0], want) and np.array_equal(runs[1], want)  # every element overwritten, the same bits twice
    # tables that point outside the text are clamped to it: nothing outside text[0 .. n_text) is read
    bad_off = torch.tensor([-5, 10 ** 9, 3], dtype=torch.int32, device=DEV)
    buf, out = _guarded(2)
    check(lib().dbn_edit_distance_pairs(pattern.data_ptr(), 64, pat_len.data_ptr(), d_text.data_ptr(), len(text), bad_off.data_ptr(), None, 2,
                                        out.data_ptr(), stream()), 'pairs')
    torch.cuda.synchronize()
    assert _guards_intact(buf, 2)
    assert out.tolist() == [R.dp(class_rows([a[0]])[0], text.tolist()), len(a[1])]  # the whole text; an empty text
    assert lib().dbn_edit_distance_pairs(pattern.data_ptr(), 65, pat_len.data_ptr(), d_text.data_ptr(), len(text), d_off.data_ptr(), None, P,
                                         out.data_ptr(), stream()) == 1


def test_nearest_entry_point_guards_poison_and_workspace_contents():
    rng = np.random.default_rng(9)
    groups = [lexicon_words(rng, 200), [], rand_words(rng, 40, 0, 9, 2)]
    tc = classes()
    lex = Lexicon(groups, tc)
    qs = rand_words(rng, 90, 0, 64, 2) + rand_words(rng, 43, 0, 9, 2)
    K = len(qs)
    group = rng.integers(-1, 4, K).astype(np.int32)
    want = [R.nearest(q, class_rows(groups[g])) if 0 <= g < 3 else (-1, -1) for q, g in zip(class_rows(qs), group.tolist())]
    assert sum(w == (-1, -1) for w in want) > 10 and sum(w != (-1, -1) for w in want) > 20
    codes, count = device_codes(qs, 64)
    query = tc.lookup(codes).contiguous()
    d_group = torch.from_numpy(group).to(DEV)
    ent_len, ent_idx, blk_off, grp_blk, data = lex._tables(torch.device(DEV, torch.cuda.current_device()))
    assert lib().dbn_lexicon_ws_bytes(K) == 8 * K and lib().dbn_lexicon_ws_bytes(0) == 0
    runs = []
    for fill in (0x00, 0xFF, 0xFF):
        ws_buf = torch.full((GUARD * 4 + 8 * K + GUARD * 4, ), fill, dtype=torch.uint8, device=DEV)
        ws = ws_buf[GUARD * 4:GUARD * 4 + 8 * K]
        ibuf, index = _guarded(K)
        dbuf, dist = _guarded(K)
        check(lib().dbn_lexicon_nearest(query.data_ptr(), 64, count.data_ptr(), d_group.data_ptr(), K, data.data_ptr(), blk_off.data_ptr(),
                                        ent_len.data_ptr(), ent_idx.data_ptr(), grp_blk.data_ptr(), 3, lex.n_blocks, lex.max_blocks, ws.data_ptr(),
                                        index.data_ptr(), dist.data_ptr(), stream()), 'nearest')
        torch.cuda.synchronize()
        assert _guards_intact(ibuf, K) and _guards_intact(dbuf, K)
        host = ws_buf.cpu().numpy()
        assert (host[:GUARD * 4] == fill).all() and (host[GUARD * 4 + 8 * K:] == fill).all()
        runs.append((index.cpu().numpy(), dist.cpu().numpy()))
    for index, dist in runs:  # every element overwritten; the workspace's contents and the run make no difference
        assert list(zip(index.tolist(), dist.tolist())) == want


# ---- recognize_words(lexicon=) --------------------------------------------------------------------------------------------------
class _Speller(torch.nn.Module):
    """a CTC-style recogniser whose logits spell the given words in order, a blank between the letters"""

    def __init__(self, words, T=26):
        super().__init__()
        self.words, self.T, self.at = words, T, 0

    def forward(self, image, text):
        b = image.shape[0]
        out = torch.zeros((b, self.T, len(CHARS) + 1))
        out[:, :, 0] = 5.0
        for i, w in enumerate(self.words[self.at:self.at + b]):
            for j, ch in enumerate(w):
                out[i, 2 * j, CHARS.index(ch) + 1] = 9.0
        self.at += b
        return out.to(image.device)


def test_recognize_words_with_a_lexicon():
    rng = np.random.default_rng(10)
    imgs = [rng.integers(0, 256, (64, 128, 3), dtype=np.uint8) for _ in range(2)]
    batch = image_collate([(i, [], None) for i in imgs])
    box = lambda x0, y0, x1, y1: [[x0, y0], [x1, y0], [x1, y1], [x0, y1]]  # noqa: E731
    boxes = [np.array([box(2, 2, 60, 20), box(5, 30, 90, 50), box(70, 2, 120, 25)], np.int16), np.array([box(4, 4, 100, 30), box(10, 35, 80, 60)], np.int16)]
    spelled = ['he1lo', 'zzzzzz', 'world', 'he1lo', 'w0rld']
    conv = CTCLabelConverter(CHARS)
    tc = TextClasses(conv)
    plain = recognize_words(batch, boxes, _Speller(spelled), conv, batch_size=2)
    assert [[w['pred'] for w in o] for o in plain] == [spelled[:3], spelled[3:]] and all(list(w) == ['box', 'pred', 'score'] for o in plain for w in o)
    # one group: every word against the same entries
    one = recognize_words(batch, boxes, _Speller(spelled), conv, batch_size=2, lexicon=Lexicon(['hello', 'world', 'help'], tc), max_distance=1)
    assert [[(w['word'], w['distance']) for w in o] for o in one] == [[('hello', 1), (None, 6), ('world', 0)], [('hello', 1), ('world', 1)]]
    # per-image groups: the group of a word is its image
    strong = Lexicon([['hello', 'world'], ['jello', 'w0rld']], tc)
    per = recognize_words(batch, boxes, _Speller(spelled), conv, batch_size=2, lexicon=strong)
    assert [[(w['word'], w['distance']) for w in o] for o in per] == [[('hello', 1), ('hello', 6), ('world', 0)], [('jello', 2), ('w0rld', 0)]]
    for with_lex in (one, per):  # 'box', 'pred' and 'score' are what they are without a lexicon, key for key
        for o, q in zip(with_lex, plain):
            assert len(o) == len(q)
            for w, v in zip(o, q):
                assert list(w) == ['box', 'pred', 'score', 'word', 'distance']
                assert np.array_equal(w['box'], v['box']) and w['pred'] == v['pred'] and w['score'] == v['score']
    # ready crops: one flat list; a lexicon of several groups has no image to go by
    crops = torch.from_numpy(rng.integers(0, 256, (2, 32, 100, 3), dtype=np.uint8)).to(DEV)
    ready = recognize_words(crops, None, _Speller(['he1p', 'wxyz']), conv, lexicon=Lexicon(['hello', 'world', 'help'], tc), max_distance=2)
    assert [(w['box'], w['pred'], w['word'], w['distance']) for w in ready] == [(None, 'he1p', 'help', 1), (None, 'wxyz', None, 4)]
    with pytest.raises(ValueError, match='2 groups'):
        recognize_words(crops, None, _Speller(['he1p', 'wxyz']), conv, lexicon=strong)
    assert recognize_words(batch, [np.zeros((0, 4, 2), np.int16)] * 2, _Speller([]), conv, lexicon=strong) == [[], []]
    # more than 64 decode steps: refused at the model's first chunk, and before the model runs where the steps are known
    long_model = _Speller(spelled, T=65)
    with pytest.raises(ValueError, match='65 steps; at most 64'):
        recognize_words(batch, boxes, long_model, conv, batch_size=2, lexicon=strong)
    assert long_model.at == 2
    assert [len(o) for o in recognize_words(batch, boxes, _Speller(spelled, T=65), conv)] == [3, 2]  # (without a lexicon there is no limit)
    untouched = _Speller(spelled)
    with pytest.raises(ValueError, match='65 steps; at most 64'):
        recognize_words(batch, boxes, untouched, conv, prediction='Attn', batch_max_length=64, lexicon=strong)
    assert untouched.at == 0


# ---- TextSpottingEvaluator ------------------------------------------------------------------------------------------------------
def _rect(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def _scene():
    """image 0: a right word; a wrong word over a matching box; a word that differs in case only; a don't-care GT with a
    detection inside it; an unmatched GT and a stray detection.  image 1: a GT and no detection.  image 2: nothing."""
    gts = [[{'points': _rect(0, 0, 100, 20), 'ignore': False, 'text': 'hello'},
            {'points': _rect(0, 30, 100, 50), 'ignore': False, 'text': 'world'},
            {'points': _rect(0, 60, 100, 80), 'ignore': False, 'text': 'Exit'},
            {'points': _rect(0, 90, 100, 110), 'ignore': True, 'text': '###'},
            {'points': _rect(0, 120, 100, 140), 'ignore': False, 'text': 'missed'}],
           [{'points': _rect(0, 0, 50, 10), 'ignore': False, 'text': 'alone'}], []]
    preds = [[{'points': _rect(2, 0, 100, 20), 'text': 'hello'},
              {'points': _rect(0, 30, 98, 50), 'text': 'w0rld!'},
              {'points': _rect(1, 60, 100, 80), 'text': 'EXIT'},
              {'points': _rect(10, 92, 90, 108), 'text': 'junk'},
              {'points': _rect(200, 200, 250, 220), 'text': 'stray'}], [], []]
    return gts, preds


def test_spotting_evaluator_hand_built_batch():
    gts, preds = _scene()
    folded = TextSpottingEvaluator().evaluate_batch(gts, preds)
    r = folded[0]
    assert r['pairs'] == [{'gt': 0, 'det': 0, 'correct': True, 'distance': 0}, {'gt': 1, 'det': 1, 'correct': False, 'distance': 2},
                          {'gt': 2, 'det': 2, 'correct': True, 'distance': 0}]
    assert (r['gtCare'], r['detCare'], r['detMatched'], r['detCorrect'], r['gtDontCare'], r['detDontCare']) == (4, 4, 3, 2, [3], [3])
    assert (r['precision'], r['recall'], r['hmean']) == (2 / 4, 2 / 4, 0.5) and (r['det_precision'], r['det_recall']) == (3 / 4, 3 / 4)
    assert r['nedSum'] == 2 / 6
    assert (folded[1]['gtCare'], folded[1]['detCare'], folded[1]['pairs'], folded[1]['precision'], folded[1]['recall']) == (1, 0, [], 0.0, 0.0)
    assert (folded[2]['precision'], folded[2]['recall'], folded[2]['hmean']) == (1.0, 1.0, 1.0)
    total = TextSpottingEvaluator.combine_results(folded)
    assert total == {'precision': 2 / 4, 'recall': 2 / 5, 'hmean': 2 * (2 / 5) * (2 / 4) / (2 / 5 + 2 / 4), 'det_precision': 3 / 4, 'det_recall': 3 / 5,
                     'det_hmean': 2 * (3 / 5) * (3 / 4) / (3 / 5 + 3 / 4), '1-ned': 1.0 - (2 / 6 + 3) / (3 + 3)}
    exact = TextSpottingEvaluator(case_sensitive=True).evaluate_batch(gts, preds)
    assert [(p['correct'], p['distance']) for p in exact[0]['pairs']] == [(True, 0), (False, 2), (False, 3)] and exact[0]['detCorrect'] == 1
    assert TextSpottingEvaluator(case_sensitive=True).combine_results(exact)['precision'] == 1 / 4
    assert TextSpottingEvaluator().evaluate_image(gts[0], preds[0]) == r


@pytest.mark.parametrize('case_sensitive', [False, True])
def test_spotting_evaluator_against_the_restatement(case_sensitive):
    rng = np.random.default_rng(11)
    gts, preds = _scene()
    letters = list('aAbé')
    batches_g, batches_p = [], []
    for _ in range(6):  # random texts over the fixed geometry; short ones over few letters, so that equal texts occur
        for src, dst in ((gts, batches_g), (preds, batches_p)):
            dst += [[dict(o, text=''.join(rng.choice(letters, int(rng.integers(0, 3))))) for o in image] for image in src]
    batches_g[0][1]['text'], batches_p[0][1]['text'] = 'a' * 70, 'ab' * 20  # one side of a pair may exceed 64 characters
    ov = polygon_overlaps([[g['points'] for g in gt] for gt in batches_g], [[p['points'] for p in pr] for pr in batches_p])
    ev = TextSpottingEvaluator(case_sensitive=case_sensitive)
    got = ev.evaluate_batch(batches_g, batches_p)
    want = [R.spotting_image(o['inter'].tolist(), o['gt_area'].tolist(), o['det_area'].tolist(), g, p, case_sensitive)
            for o, g, p in zip(ov, batches_g, batches_p)]
    for a, w in zip(got, want):
        for key, v in w.items():
            assert a[key] == v, key
    assert ev.combine_results(got) == R.combine(want)
    n_right = sum(r['detCorrect'] for r in want)
    assert 0 < n_right < sum(r['detMatched'] for r in want)
