"""CPU (-m "not gpu"): the edit distances, the lexicon and the end-to-end score without a device.  The
restatement tests/spotting_ref.py (what the GPU tests compare the kernels with) is checked here: the dynamic programme against
known values and an independent recursion, the bit-vector recurrence against the dynamic programme.  Then the host side of
db_text_minimal_amd/spotting.py: the class map, the lexicon's device layout, the evaluator's arithmetic, the C ABI."""
import functools

import numpy as np
import pytest

from db_text_minimal_amd import AttnLabelConverter, CTCLabelConverter, Lexicon, TextClasses, TextSpottingEvaluator, _lib
from db_text_minimal_amd import spotting as S
import spotting_ref as R
from test_host_cpu import PARSER_SPELLINGS

CHARS = '0123456789abcdefghijklmnopqrstuvwxyz'
PATTERN_LENGTHS = [0, 1, 2, 31, 32, 33, 63, 64]
TEXT_LENGTHS = [0, 1, 7, 63, 64, 65, 255, 1000]
ALPHABETS = [2, 3, 36]


def ids(s):
    return [ord(c) for c in s]


def recursion(x, y):
    """the definition, memoised: nothing shared with the table of spotting_ref.dp_pairs"""
    @functools.lru_cache(maxsize=None)
    def d(i, j):
        if i == 0 or j == 0:
            return i + j
        same = x[i - 1] == y[j - 1] and x[i - 1] != 255
        return min(d(i - 1, j) + 1, d(i, j - 1) + 1, d(i - 1, j - 1) + (0 if same else 1))
    return d(len(x), len(y))


# ---- the restatement ------------------------------------------------------------------------------------------------------
def test_dp_known_values():
    assert R.dp(ids('kitten'), ids('sitting')) == 3
    assert R.dp(ids('flaw'), ids('lawn')) == 2
    assert R.dp(ids('saturday'), ids('sunday')) == 3
    assert R.dp([], []) == 0 and R.dp([], ids('abc')) == 3 and R.dp(ids('abcd'), []) == 4
    assert R.dp(ids('hello'), ids('hello')) == 0 and R.dp(ids('a'), ids('b')) == 1
    assert R.text_distance('Hello', 'hELLO') == 0 and R.text_distance('Hello', 'hELLO', case_sensitive=True) == 5


def test_dp_equals_the_recursion_on_short_strings():
    rng = np.random.default_rng(3)
    xs, ys = [], []
    for _ in range(400):
        k = int(rng.choice([2, 3, 5]))
        xs.append(tuple(rng.integers(0, k, int(rng.integers(0, 9))).tolist()))
        ys.append(tuple(rng.integers(0, k, int(rng.integers(0, 9))).tolist()))
    a, la = R.padded(xs)
    b, lb = R.padded(ys)
    got = R.dp_pairs(a, la, b, lb).tolist()
    assert got == [recursion(x, y) for x, y in zip(xs, ys)]
    assert len(set(got)) > 5
    e = [list(y) for y in ys[:50]]
    assert R.dp_lexicon(list(xs[0]), e).tolist() == [recursion(xs[0], tuple(y)) for y in e]


def test_bit_vector_recurrence_equals_dp():
    rng = np.random.default_rng(4)
    pats, texts = [], []
    for k in ALPHABETS:
        for m in PATTERN_LENGTHS:
            for n in TEXT_LENGTHS:
                pats.append(rng.integers(0, k, m).tolist())
                texts.append(rng.integers(0, k, n).tolist())
    # carries through bits 31 / 32 and 63: one repeated class against itself and against one changed last class
    for m in (32, 33, 64):
        pats += [[5] * m, [5] * m]
        texts += [[5] * m, [5] * (m - 1) + [6]]
    a, la = R.padded(pats)
    b, lb = R.padded(texts)
    want = R.dp_pairs(a, la, b, lb).tolist()
    assert [R.myers(p, t) for p, t in zip(pats, texts)] == want
    assert want[-6:] == [0, 1, 0, 1, 0, 1]
    assert R.myers([], [1, 2, 3]) == 3 and R.myers([1] * 64, []) == 64


def test_class_255_never_matches():
    for fn in (R.dp, R.myers, lambda x, y: recursion(tuple(x), tuple(y))):
        assert fn([255], [255]) == 1
        assert fn([1, 255, 2], [1, 255, 2]) == 1
        assert fn([255] * 4, [255] * 6) == 6
        assert fn([1, 2], [1, 2]) == 0


# ---- TextClasses ----------------------------------------------------------------------------------------------------------
def test_text_classes_fold_and_extend():
    tc = TextClasses(CTCLabelConverter(CHARS))
    assert tc.head == 1 and tc.character == list(CHARS) and len(tc) == 36
    data, off = tc.encode(['aB9', '', 'Ab9'])
    assert data.dtype == np.uint8 and off.dtype == np.int32 and off.tolist() == [0, 3, 3, 6]
    assert data.tolist() == [10, 11, 9, 10, 11, 9]
    data, _ = tc.encode(['a-é', 'É-'])  # further characters take the next classes as they are met, folded too
    assert data.tolist() == [10, 36, 37, 37, 36] and len(tc) == 38
    cs = TextClasses(AttnLabelConverter('abAB'), case_sensitive=True)
    assert cs.head == 2 and cs.encode(['abAB'])[0].tolist() == [0, 1, 2, 3]
    folded = TextClasses('abAB')  # characters alone; the recogniser's own characters fold as well
    assert folded.head is None and folded.encode(['abAB'])[0].tolist() == [0, 1, 0, 1] and len(folded) == 2
    with pytest.raises(TypeError):
        tc.encode([b'bytes'])


def test_text_classes_256th_class_raises():
    tc = TextClasses('', case_sensitive=True)
    tc.encode([''.join(chr(0x4E00 + i) for i in range(255))])
    assert len(tc) == 255
    assert tc.encode([chr(0x4E00 + 254)])[0].tolist() == [254]  # the 255 classes 0 .. 254 are all usable
    with pytest.raises(ValueError, match='255'):
        tc.encode([chr(0x4E00 + 255)])
    with pytest.raises(ValueError):
        TextClasses([chr(0x4E00 + i) for i in range(256)], case_sensitive=True)


def test_remap_specials_and_last_entry():
    ctc = TextClasses(CTCLabelConverter(CHARS)).remap_host()
    assert ctc.dtype == np.uint8 and ctc.shape == (38, ) and ctc[0] == 255 and ctc[-1] == 255 and ctc[1:-1].tolist() == list(range(36))
    attn = TextClasses(AttnLabelConverter('abAB')).remap_host()
    assert attn.tolist() == [255, 255, 0, 1, 0, 1, 255]
    plain = TextClasses('ab')
    with pytest.raises(ValueError, match='head'):
        plain.remap_host()
    assert plain.remap_host(1).tolist() == [255, 0, 1, 255] and plain.remap_host(AttnLabelConverter('ab')).tolist() == [255, 255, 0, 1, 255]
    on_host = TextClasses(CTCLabelConverter('ab')).remap(device='cpu')
    assert on_host.tolist() == [255, 0, 1, 255]
    # the lookup as the device does it: any code value lands inside the table
    import torch
    codes = torch.tensor([[1, 2, 0, -1, 3, 1000, -7]], dtype=torch.int32)
    assert on_host[codes.clamp(0, on_host.shape[0] - 1).long()].tolist() == [[0, 1, 255, 255, 255, 255, 255]]


# ---- Lexicon: the host layout -----------------------------------------------------------------------------------------------
def _words(rng, n, lo, hi, alphabet='abc'):
    return [''.join(rng.choice(list(alphabet), int(rng.integers(lo, hi + 1)))) for _ in range(n)]


def _check_layout(lex, groups, tc):
    assert lex.grp_blk.tolist()[0] == 0 and len(lex.grp_blk) == len(groups) + 1 and lex.grp_blk[-1] == lex.n_blocks
    assert len(lex.ent_len) == len(lex.ent_idx) == lex.n_blocks * 64 and len(lex.blk_off) == lex.n_blocks + 1
    assert lex.blk_off[-1] == len(lex.data) and lex.max_blocks == max(-(-len(g) // 64) for g in groups)
    for g, words in enumerate(groups):
        got = lex.host_entries(g)
        assert sorted(i for i, _ in got) == list(range(len(words)))  # the permutation returns every original index once
        for i, cls in got:
            assert cls.tolist() == tc.encode([words[i]])[0].tolist()
        lens = [len(c) for _, c in got]
        assert lens == sorted(lens)  # ordered by length within the group ...
        for (i0, c0), (i1, c1) in zip(got, got[1:]):
            assert len(c0) < len(c1) or i0 < i1  # ... and by original index among equal lengths
        for b in range(lex.grp_blk[g], lex.grp_blk[g + 1]):
            rows = (lex.blk_off[b + 1] - lex.blk_off[b]) // 64
            ln = lex.ent_len[b * 64:(b + 1) * 64]
            assert rows % 4 == 0 and (lex.blk_off[b + 1] - lex.blk_off[b]) % 64 == 0 and ln.max() <= rows < ln.max() + 4
            blk = lex.data[lex.blk_off[b]:lex.blk_off[b + 1]].reshape(rows, 64)
            assert (blk[np.arange(rows)[:, None] >= np.maximum(ln, 0)[None, :]] == 255).all()  # 255 behind every entry
            assert ((ln >= 0) == (np.arange(64) < min(64, len(words) - (b - lex.grp_blk[g]) * 64))).all()


@pytest.mark.parametrize('n', [0, 1, 63, 64, 65, 257])
def test_lexicon_layout_one_group(n):
    rng = np.random.default_rng(n)
    tc = TextClasses(CHARS)
    words = _words(rng, n, 0, 20)
    lex = Lexicon(words, tc)
    assert lex.n_groups == 1 and lex.groups == [words]
    _check_layout(lex, [words], tc)


def test_lexicon_layout_groups_and_long_entries():
    rng = np.random.default_rng(9)
    tc = TextClasses(CHARS)
    groups = [_words(rng, 70, 0, 255), [], _words(rng, 5, 250, 255), ['', '', 'a']]
    lex = Lexicon(groups, tc)
    assert lex.n_groups == 4 and np.diff(lex.grp_blk).tolist() == [2, 0, 1, 1]
    _check_layout(lex, groups, tc)
    assert lex.word(3, 2) == 'a' and lex.word(0, 69) == groups[0][69]
    assert lex.words_of([2, -1, 0], [1, -1, 3], [3, 1, 2], max_distance=2) == [('a', 1), (None, -1), (None, 3)]
    with pytest.raises(ValueError, match='256 characters'):
        Lexicon(['ok', 'x' * 256], tc)
    Lexicon(['x' * 255], tc)
    with pytest.raises(TypeError):
        Lexicon([['ok'], [3]], tc)


def test_pair_layout_takes_the_shorter_side_as_pattern():
    tc = TextClasses(CHARS)
    a = ['abc', 'x' * 70, '', 'q' * 64]
    b = ['abcdef', 'xy', 'zz', 'q' * 65]
    pattern, pl, text, toff = S.pair_layout(*tc.encode(a), *tc.encode(b))
    assert pattern.shape == (4, 64) and pl.tolist() == [3, 2, 0, 64] and toff.tolist() == [0, 6, 76, 78, 143]
    enc = lambda s: tc.encode([s])[0].tolist()  # noqa: E731
    for p, (short, long_) in enumerate([('abc', 'abcdef'), ('xy', 'x' * 70), ('', 'zz'), ('q' * 64, 'q' * 65)]):
        assert pattern[p, :pl[p]].tolist() == enc(short) and (pattern[p, pl[p]:] == 255).all()
        assert text[toff[p]:toff[p + 1]].tolist() == enc(long_)
    with pytest.raises(ValueError, match='both strings exceed 64'):
        S.pair_layout(*tc.encode(['a' * 65]), *tc.encode(['b' * 66]))
    pattern, pl, text, toff = S.pair_layout(*tc.encode([]), *tc.encode([]))
    assert pattern.shape == (0, 1) and len(pl) == 0 and len(text) == 0 and toff.tolist() == [0]


# ---- the evaluator's arithmetic -----------------------------------------------------------------------------------------------
def _ov(inter, ga, da):
    return dict(inter=np.array(inter, np.float64).reshape(len(ga), len(da)), gt_area=np.array(ga, np.float64), det_area=np.array(da, np.float64))


def _gt(text, ignore=False):
    return {'points': [(0, 0), (1, 0), (1, 1)], 'ignore': ignore, 'text': text}


def _batch():
    """image 0: GT 0 matched and right, GT 1 matched and wrong by 2 of 5, GT 2 unmatched, detection 3 unmatched;
    image 1: a don't-care GT that swallows the only detection; image 2: nothing at all; image 3: one GT, no detection"""
    gts = [[_gt('Hello'), _gt('world'), _gt('lost')], [_gt('###', True)], [], [_gt('alone')]]
    preds = [[_gt('hello'), _gt('wor'), _gt('spare'), _gt('x')], [_gt('any')], [], []]
    ov = [_ov([[90, 0, 0, 0], [0, 80, 0, 0], [0, 0, 10, 0]], [100, 100, 100], [100, 100, 100, 100]), _ov([[60]], [100], [100]),
          _ov([], [], []), _ov([], [100], [])]
    return gts, preds, ov


def test_evaluator_arithmetic_with_injected_overlaps_and_distances():
    gts, preds, ov = _batch()
    ev = TextSpottingEvaluator()
    res = ev.evaluate_batch(gts, preds, overlaps=ov, distances=[[0, 2], [], [], []])
    r = res[0]
    assert r['pairs'] == [{'gt': 0, 'det': 0, 'correct': True, 'distance': 0}, {'gt': 1, 'det': 1, 'correct': False, 'distance': 2}]
    assert (r['gtCare'], r['detCare'], r['detMatched'], r['detCorrect']) == (3, 4, 2, 1)
    assert (r['precision'], r['recall'], r['hmean']) == (1 / 4, 1 / 3, 2 * (1 / 4) * (1 / 3) / (1 / 4 + 1 / 3))
    assert (r['det_precision'], r['det_recall']) == (2 / 4, 2 / 3) and r['nedSum'] == 2 / 5
    assert len(r['iouMat']) == 3 and r['gtDontCare'] == [] and r['evaluationLog'] == ''
    # zero denominators, per image: the detection metric's rules
    assert (res[1]['gtCare'], res[1]['detCare'], res[1]['detDontCare']) == (0, 0, [0])
    assert (res[1]['precision'], res[1]['recall'], res[1]['hmean'], res[1]['detCorrect']) == (1.0, 1.0, 1.0, 0)
    assert (res[2]['precision'], res[2]['recall'], res[2]['hmean']) == (1.0, 1.0, 1.0)
    assert (res[3]['precision'], res[3]['recall'], res[3]['hmean'], res[3]['pairs']) == (0.0, 0.0, 0.0, [])
    total = ev.combine_results(res)
    assert total['precision'] == 1 / 4 and total['recall'] == 1 / 4 and total['hmean'] == 1 / 4
    assert total['det_precision'] == 2 / 4 and total['det_recall'] == 2 / 4
    assert total['1-ned'] == 1.0 - (2 / 5 + (2 + 2)) / (2 + 2 + 2)  # 2 pairs, 2 unmatched care GTs, 2 unmatched care detections
    # and the whole of it equals the restatement
    want = [R.spotting_image(o['inter'].tolist(), o['gt_area'].tolist(), o['det_area'].tolist(), g, p, distances=d)
            for o, g, p, d in zip(ov, gts, preds, [[0, 2], [], [], []])]
    for got, w in zip(res, want):
        for key, v in w.items():
            assert got[key] == v, key
    assert total == R.combine(want)
    empty = ev.combine_results(res[1:3])
    assert empty == {'precision': 0, 'recall': 0, 'hmean': 0, 'det_precision': 0, 'det_recall': 0, 'det_hmean': 0, '1-ned': 1.0}
    assert ev.combine_results([]) == empty
    with pytest.raises(ValueError, match='distances'):
        ev.evaluate_batch(gts, preds, overlaps=ov, distances=[[0], [], [], []])


def test_evaluator_restatement_distances_fold_case():
    gts, preds, ov = _batch()
    o, g, p = ov[0], gts[0], preds[0]
    folded = R.spotting_image(o['inter'].tolist(), o['gt_area'].tolist(), o['det_area'].tolist(), g, p)
    exact = R.spotting_image(o['inter'].tolist(), o['gt_area'].tolist(), o['det_area'].tolist(), g, p, case_sensitive=True)
    assert [q['distance'] for q in folded['pairs']] == [0, 2] and [q['distance'] for q in exact['pairs']] == [1, 2]
    assert folded['detCorrect'] == 1 and exact['detCorrect'] == 0 and exact['nedSum'] == 1 / 5 + 2 / 5


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_signatures_of_the_three_entries():
    assert _lib.SIGNATURES['dbn_edit_distance_pairs'] == 'pipplppipp'
    assert _lib.SIGNATURES['dbn_lexicon_ws_bytes'] == 'i' and 'dbn_lexicon_ws_bytes' in _lib.LONG_RETURN
    assert _lib.SIGNATURES['dbn_lexicon_nearest'] == 'pippi' + 'ppppp' + 'iii' + 'pppp'
    assert not {'dbn_edit_distance_pairs', 'dbn_lexicon_nearest'} & _lib.LONG_RETURN


def test_header_spellings_unchanged():
    assert _lib.parse_header(open(_lib.HEADER).read())[3] == PARSER_SPELLINGS
