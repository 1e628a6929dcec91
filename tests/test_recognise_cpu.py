"""CPU (-m "not gpu"): the host side of db_text_minimal_amd.recognise and the restatement tests/recognise_ref.py that the
GPU tests compare against: the restatement equals the reference's torch ops (test_ocr.py:73-103), the converters on
hand-written cases, the grey formula against PIL, the normalisation table against torch bit for bit."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from db_text_minimal_amd import AttnLabelConverter, CTCLabelConverter, greedy_decode, words_to_input
from db_text_minimal_amd import recognise as Rc
import recognise_ref as R

CHARS = '0123456789abcdefghijklmnopqrstuvwxyz'


def _reference_predict(preds, table, attn):
    """predict() of test_ocr.py:73-103 for one sequence preds [1, T, C], the converters' decode written out: -> (str, score)"""
    _, preds_index = preds.max(2)
    preds_prob = F.softmax(preds, dim=2)
    preds_max_prob, _ = preds_prob.max(dim=2)
    idx = preds_index[0].tolist()
    pred_max_prob = preds_max_prob[0]
    if attn:
        pred = ''.join(table[i] for i in idx)
        pred_EOS = pred.find('[s]')
        pred = pred[:pred_EOS]
        pred_max_prob = pred_max_prob[:pred_EOS]  # a character index used as a step index: equal while '[GO]' does not occur
    else:
        pred = ''.join(table[c] for i, c in enumerate(idx) if c != 0 and not (i > 0 and idx[i - 1] == c))
    return pred, float(pred_max_prob.cumprod(dim=0)[-1])


@pytest.mark.parametrize('mode', ['ctc', 'attn'])
def test_restatement_equals_the_reference_torch_ops(mode):
    g = torch.Generator().manual_seed(3 if mode == 'ctc' else 4)
    conv = CTCLabelConverter(CHARS) if mode == 'ctc' else AttnLabelConverter(CHARS)
    B, T, C = 40, 26, len(conv.character)
    logits = torch.randn(B, T, C, generator=g) * 3
    if mode == 'ctc':  # blanks and repeats, as a trained CTC head gives them
        logits[:, ::3, 0] += 8
        logits[:, 1:25:3] = logits[:, 2:26:3]
    else:  # an [s] somewhere after the first step in every sequence (the reference's quirks are for the cases without)
        logits[:, :, 0] -= 30  # no '[GO]' (four characters for one step, see _reference_predict)
        for b in range(B):
            logits[b, 1 + b % (T - 1), 1] += 30
            logits[b, 0, 1] -= 30
    codes, count, score = R.greedy_decode(logits.numpy(), mode)
    got = R.strings(codes, count, conv.character)
    assert got == conv.decode_host(codes, count)
    for b in range(B):
        pred, s = _reference_predict(logits[b:b + 1], conv.character, mode == 'attn')
        assert got[b] == pred, b
        assert abs(score[b] - s) <= 1e-5 * s, (b, score[b], s)  # torch forms it in float32
    assert len(set(got)) > B // 2 and any(count < T - 3)
    k, p = R.steps(logits.numpy())
    assert np.array_equal(k, logits.max(2)[1].numpy())
    np.testing.assert_allclose(p, F.softmax(logits, 2).max(2)[0].numpy(), rtol=1e-5)


def test_restatement_nan_rows_follow_torch_max():
    x = torch.tensor([[[1.0, float('nan'), 5.0, float('nan')], [2.0, 2.0, 1.0, 2.0], [float('-inf')] * 4, [0.0, float('inf'), float('inf'), 1.0]]])
    k, p = R.steps(x.numpy())
    assert k.tolist() == [[1, 0, 0, 1]] and k.tolist() == x.max(2)[1].tolist()
    assert np.isnan(p[0, 0]) and p[0, 1] == 1 / (3 + np.exp(-1.0)) and np.isnan(p[0, 2]) and np.isnan(p[0, 3])


def test_converters_on_hand_written_cases():
    ctc, attn = CTCLabelConverter('abc'), AttnLabelConverter('abc')
    assert ctc.character == ['[blank]', 'a', 'b', 'c'] and attn.character == ['[GO]', '[s]', 'a', 'b', 'c']
    k = np.array([[0, 0, 0, 0, 0, 0],    # all blank
                  [1, 1, 0, 1, 2, 2],    # repeats across a blank: a, a, b
                  [3, 3, 3, 3, 3, 3],    # one run
                  [0, 2, 0, 2, 2, 1]])   # b, b, a
    p = np.full(k.shape, 0.5)
    codes, count, score = R.collapse(k, p, 'ctc')
    assert count.tolist() == [0, 3, 1, 3] and codes.tolist() == [[-1] * 6, [1, 1, 2, -1, -1, -1], [3] + [-1] * 5, [2, 2, 1, -1, -1, -1]]
    assert (score == 0.5 ** 6).all()  # every step enters the CTC score, kept or not
    assert ctc.decode_host(codes, count) == ['', 'aab', 'c', 'bba']
    codes, count, score = R.collapse(k, p, 'ctc', lengths=[6, 4, 0, 9])
    assert count.tolist() == [0, 2, 0, 3] and score.tolist() == [0.5 ** 6, 0.5 ** 4, 1.0, 0.5 ** 6]
    k = np.array([[1, 2, 3, 4, 2, 2],    # [s] first: the empty word, score 1
                  [2, 3, 4, 2, 3, 4],    # no [s]: all six steps kept (the reference would drop the last)
                  [2, 2, 1, 3, 1, 4],    # the first [s] ends the word
                  [0, 4, 4, 1, 1, 1]])   # [GO] is an ordinary entry
    codes, count, score = R.collapse(k, p, 'attn')
    assert count.tolist() == [0, 6, 2, 3] and score.tolist() == [1.0, 0.5 ** 6, 0.25, 0.125]
    assert attn.decode_host(codes, count) == ['', 'abcabc', 'aa', '[GO]cc']
    codes, count, _ = R.collapse(k, p, 'attn', lengths=[6, 2, 1, 6])
    assert count.tolist() == [0, 2, 1, 3]
    with pytest.raises(ValueError):
        ctc.decode_host(np.array([[4, 0]]), np.array([1]))   # past the table
    with pytest.raises(ValueError):
        ctc.decode_host(np.array([[-1, 0]]), np.array([1]))  # a kept -1
    with pytest.raises(ValueError):
        ctc.decode_host(np.array([[1, 0]]), np.array([3]))   # count past T
    assert ctc.decode_host(np.array([[7, -1]]), np.array([0])) == ['']  # codes past count are not read
    assert ctc.decode_host(np.zeros((0, 5), np.int32), np.zeros(0, np.int32)) == []


def _every_colour():
    c = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], -1).astype(np.uint8)


def test_grey_table_is_the_formula_for_every_colour():
    rgb = _every_colour()
    g = R.grey(rgb)
    r_, g_, b_ = (rgb[:, i].astype(np.uint64) for i in range(3))
    assert np.array_equal(g, ((19595 * r_ + 38470 * g_ + 7471 * b_ + 32768) >> 16).astype(np.uint8))
    assert g.min() == 0 and g.max() == 255 and g[0xFFFFFF] == 255  # the weights sum to 65536: no overflow past 255
    assert np.array_equal(R.grey(rgb[:, ::-1], bgr=True), g)


def test_grey_equals_pil_convert_l_for_every_colour():
    """the pin of the formula itself; reported as skipped where PIL is not importable"""
    Image = pytest.importorskip('PIL.Image')
    rgb = _every_colour()
    pil = np.asarray(Image.frombuffer('RGB', (4096, 4096), rgb.tobytes(), 'raw', 'RGB', 0, 1).convert('L')).reshape(-1)
    assert np.array_equal(pil, R.grey(rgb))


def test_normalisation_table_equals_torch_bit_for_bit():
    g = np.arange(256, dtype=np.uint8)
    want = torch.tensor(g).float().div(255).sub_(0.5).div_(0.5).numpy()
    table = Rc.input_table()
    assert table.dtype == np.float32 and np.array_equal(table.view(np.int32), want.view(np.int32))
    assert np.array_equal(R.normalise(g).view(np.int32), want.view(np.int32))
    assert table[0] == -1 and table[255] == 1


def test_argument_errors_without_a_gpu():
    with pytest.raises(ValueError, match='uint8'):
        words_to_input(torch.zeros(2, 32, 100, 3))
    with pytest.raises(ValueError, match='GPU'):
        words_to_input(torch.zeros(2, 32, 100, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match='mode'):
        greedy_decode(torch.zeros(1, 2, 3), mode='beam')
    with pytest.raises(ValueError, match='GPU'):
        greedy_decode(torch.zeros(1, 2, 3))
    with pytest.raises(ValueError, match=r'\[B, T, C\]'):
        greedy_decode(torch.zeros(2, 3))
    with pytest.raises(ValueError, match=r'\[B, T, C\]'):
        greedy_decode(torch.zeros(1, 2, 3, dtype=torch.float64))
