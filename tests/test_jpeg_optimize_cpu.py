"""CPU (-m "not gpu"): optimised Huffman tables on the host (csrc/jpeg_enc.hip dbn_jpeg_optimal_table / dbn_jpeg_encode_batch_opt
through db_text_minimal_amd.jpeg): the table builder against every DHT segment of Pillow's optimize=True streams
(tests/golden/jpeg_optimize_cases.npz, the optimised streams of jpeg_cases.npz, fresh Pillow output where Pillow imports) and
against the restatement tests/jpeg_opt_ref.py on degenerate histograms; entropy_encode(optimize=True) reproducing those
streams' DHT payloads and scan bytes; optimize=False unchanged; thread counts; refusals that fail alone."""
import io
import json
import os

import numpy as np
import pytest

from db_text_minimal_amd import JpegCoefficients, JpegEncodeError, entropy_decode, entropy_encode, jpeg_info, optimal_huffman_table
import jpeg_enc_ref as E
import jpeg_opt_ref as O
import jpeg_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
_cache = {}


def golden():
    """[(case, image, Pillow's optimize=True stream)]"""
    if 'g' not in _cache:
        g = np.load(os.path.join(HERE, 'golden', 'jpeg_optimize_cases.npz'))
        _cache['g'] = [(c, g['img_%d' % i], g['jpeg_%d' % i].tobytes()) for i, c in enumerate(json.loads(str(g['cases'])))]
    return _cache['g']


def optimised_streams():
    """[(name, stream)]: the new archive's, and the optimised ones of the decoder's archive"""
    if 's' not in _cache:
        g = np.load(os.path.join(HERE, 'golden', 'jpeg_cases.npz'))
        names = json.loads(str(g['names']))
        old = [(n, g['jpeg_%d' % i].tobytes()) for i, n in enumerate(names) if n.endswith('_opt')]
        assert len(old) == 3
        _cache['s'] = [(c['name'], d) for c, _, d in golden()] + old
    return _cache['s']


def stream_histograms(data):
    h, coefs = R.entropy_decode(data)
    return O.histograms(h.width, h.height, h.samp, coefs, h.ri)


def _pil():
    try:
        from PIL import Image, features
        return Image if features.check('jpg') else None
    except ImportError:
        return None


def same_table(got, want):
    return [int(v) for v in got[0]] == list(want[0]) and [int(v) for v in got[1]] == list(want[1])


def check_stream(name, data):
    """the builder on the stream's own histograms gives its DHT segments; the transcode gives its DHT payloads and scan bytes"""
    hist = stream_histograms(data)
    theirs = O.dht_tables(data)
    assert len(theirs) in (2, 4), name
    for (tc, th), t in theirs.items():
        assert same_table(optimal_huffman_table(hist[2 * th + tc]), t), (name, tc, th)
    obj = entropy_decode([data], pin=False)
    assert not obj.status.any()
    mine = entropy_encode(obj, restart_interval=jpeg_info(data)['restart_interval'], optimize=True)[0]
    assert O.dht_tables(mine) == theirs, name
    assert list(O.dht_tables(mine)) == [(0, 0), (1, 0), (0, 1), (1, 1)][:len(theirs)], name
    assert E.scan_bytes(mine) == E.scan_bytes(data), name
    return mine


def test_builder_and_transcode_equal_every_golden_stream():
    assert len(optimised_streams()) >= 23
    kinds = set()
    for name, data in optimised_streams():
        mine = check_stream(name, data)
        info = jpeg_info(mine)
        kinds.add((info['components'], tuple(info['sampling'][0]), bool(info['restart_interval'])))
        back = entropy_decode([mine], pin=False)
        want = entropy_decode([data], pin=False)
        assert not back.status.any() and np.array_equal(back.coef.numpy(), want.coef.numpy()) and np.array_equal(back.qtabs, want.qtabs)
    assert {(1, (1, 1)), (3, (1, 1)), (3, (2, 1)), (3, (2, 2))} == {k[:2] for k in kinds} and any(k[2] for k in kinds)


def test_whole_files_equal_the_restatement():
    for c, img, data in golden():
        nc = 1 if img.ndim == 2 else 3
        tabs = E.component_tables(nc, c['quality'], None)
        samp, _, coefs = E.forward(img, tabs, c['sub'] if nc == 3 else '444')
        obj = entropy_decode([data], pin=False)
        for ri in (c['ri'], 2):
            assert entropy_encode(obj, restart_interval=ri, optimize=True)[0] == O.write_stream(img.shape[1], img.shape[0], samp, tabs, coefs, ri), c['name']
        # without optimize: the bytes of before, the restatement's Annex K file
        assert entropy_encode(obj, restart_interval=c['ri'])[0] == entropy_encode(obj, restart_interval=c['ri'], optimize=False)[0] \
            == E.write_stream(img.shape[1], img.shape[0], samp, tabs, coefs, c['ri']), c['name']


def test_degenerate_histograms_equal_the_restatement():
    hs = {}
    hs['one'] = np.zeros(256, np.int64)
    hs['one'][17] = 5
    hs['two'] = np.zeros(256, np.int64)
    hs['two'][[0, 255]] = 3, 3
    hs['equal'] = np.full(256, 7, np.int64)
    fib = np.zeros(256, np.int64)
    a, b = 1, 1
    for k in range(28):  # depth 28 before limiting: the bits[] adjustment runs
        fib[3 * k] = a
        a, b = b, a + b
    hs['fibonacci'] = fib
    rng = np.random.default_rng(5)
    for k in range(20):
        h = rng.integers(0, 4, 256) * rng.integers(0, 1000, 256) ** int(rng.integers(1, 4))
        h[int(rng.integers(0, 256))] += 1
        hs['random%d' % k] = h.astype(np.int64)
    for name, h in hs.items():
        got, want = optimal_huffman_table(h), O.optimal_table(h)
        assert same_table(got, want), name
        assert got[0].dtype == np.uint8 and got[0].shape == (16, ) and len(got[1]) == int((h > 0).sum()) == int(got[0].sum()), name
    # 28 Fibonacci counts make a Huffman tree 28 deep; after limiting, the pseudo-symbol held the one 16-bit code or shares that length
    assert max(l + 1 for l, n in enumerate(O.optimal_table(fib)[0]) if n) in (15, 16)
    assert [int(v) for v in optimal_huffman_table(hs['one'])[0]] == [1] + [0] * 15
    assert sum((int(n) << (16 - l - 1)) for l, n in enumerate(optimal_huffman_table(hs['equal'])[0])) < 1 << 16  # Kraft, with room for all-ones
    for bad in (np.zeros(256, np.int64), np.ones(255, np.int64), -np.ones(256, np.int64), np.ones(256)):
        with pytest.raises(ValueError):
            optimal_huffman_table(bad)
    deep = np.zeros(256, np.int64)
    deep[:36] = 3 ** np.arange(36)  # every count above the sum of the smaller ones: a chain 36 deep
    with pytest.raises(RuntimeError):  # a code of more than 32 bits before limiting: libjpeg gives up, and so does the builder
        optimal_huffman_table(deep)


def test_thread_counts_and_batches_give_identical_bytes():
    datas = [d for c, _, d in golden() if not c['ri']]
    obj = entropy_decode(datas, pin=False)
    want = entropy_encode(obj, threads=1, optimize=True)
    for t in (3, 16):
        assert entropy_encode(obj, threads=t, optimize=True) == want
    for n, d in enumerate(datas):
        assert E.scan_bytes(want[n]) == E.scan_bytes(d) and O.dht_tables(want[n]) == O.dht_tables(d), n
        assert len(want[n]) <= len(entropy_encode(entropy_decode([d], pin=False))[0])


def test_an_image_that_cannot_be_coded_fails_alone():
    cases = golden()
    names = [c['name'] for c, _, _ in cases]
    datas = [d for _, _, d in cases]
    obj = entropy_decode(datas, pin=False)
    want = entropy_encode(obj, optimize=True)
    bad_ac, bad_dc, bad_q, gone = 8, 4, 6, 0
    o = JpegCoefficients(obj.coef.clone(), obj.desc.copy(), obj.qtabs.copy(), obj.status.copy())
    o.coef[int(o.desc[bad_ac, 0]) + 5] = 1024
    o.coef[int(o.desc[bad_dc, 0])] = 2048
    o.qtabs[bad_q, 0, 3] = 256
    o.status[gone] = 2
    with pytest.raises(JpegEncodeError, match='image 0'):
        entropy_encode(o, optimize=True)
    got, errs = entropy_encode(o, errors='report', optimize=True)
    failed = {bad_ac: (5, 'AC'), bad_dc: (4, 'DC'), bad_q: (3, 'quantisation'), gone: (1, 'not decoded')}
    for n in range(len(obj)):
        if n in failed:
            assert got[n] is None and errs[n].index == n and errs[n].code == failed[n][0] and failed[n][1] in errs[n].reason, (n, errs[n])
        else:
            assert errs[n] is None and got[n] == want[n], names[n]


@pytest.mark.skipif(_pil() is None, reason='Pillow with JPEG support is not installed')
def test_fresh_pillow_streams():
    Image = _pil()
    import sys
    sys.path.insert(0, os.path.join(HERE, 'golden'))
    from make_jpeg_golden import SUBSAMPLING, content
    rng = np.random.default_rng(99)
    for k in range(200):
        w, h = int(rng.integers(1, 70)), int(rng.integers(1, 50))
        sub = ('444', '422', '420', 'grey')[k % 4]
        q = int(rng.integers(30, 101))
        img = content(('noise', 'ramp', 'strokes')[k % 3], rng, w, h) if k % 17 else np.full((h, w, 3), int(rng.integers(0, 256)), np.uint8)
        kw = {} if k % 5 else {'restart_marker_blocks': int(rng.integers(1, 6))}
        buf = io.BytesIO()
        if sub == 'grey':
            img = np.ascontiguousarray(img[:, :, 0])
            Image.fromarray(img).save(buf, 'JPEG', quality=q, optimize=True, **kw)
        else:
            Image.fromarray(img).save(buf, 'JPEG', quality=q, optimize=True, subsampling=SUBSAMPLING[sub], **kw)
        mine = check_stream('fresh %d' % k, buf.getvalue())
        a, b = (np.asarray(Image.open(io.BytesIO(d))) for d in (mine, buf.getvalue()))
        assert a.shape == b.shape and np.array_equal(a, b), k
