"""GPU (-m gpu): labels on the device (dbn_draw_glyphs of csrc/render.hip through db_text_minimal_amd.render), bit for bit
against the restatement tests/labels_ref.py: everything is integer arithmetic, so nothing here is a tolerance.  A packed batch
of small odd-sized images with guard bytes, labels inside, across every border and corner, outside, at the ends of the
coordinate range, empty, of all 95 characters and of 256; backgrounds; the in-place form; records the kernel must skip;
draw_words / draw_scores / render_detections against the calls they are documented as; detect_boxes -> draw_scores."""
import numpy as np
import pytest
import torch

from db_text_minimal_amd import (detect_boxes, draw_dots, draw_labels, draw_outlines, draw_scores, draw_words, image_views, overlay_heatmap,
                                 render_detections, text_size)
from db_text_minimal_amd import render as Rn
from db_text_minimal_amd import packed as Pk
from db_text_minimal_amd._lib import check, lib
import labels_ref as LR
import render_ref as R
from gpu_util import DEV

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (5, 3), (37, 53), (64, 1), (200, 333)]
GUARD = 4099  # odd: the batch starts at an odd address offset, and images 1 .. 4 at odd byte offsets of it
ALL95 = ''.join(chr(c) for c in range(32, 127))
_images_cache = {}


def _image(rng, H, W):
    y, x = np.mgrid[0:H, 0:W]
    base = (np.stack([x * 7 + y * 3, x * 2 - y * 5, (x ^ y) * 11], -1) % 256).astype(np.uint8)
    noise = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return np.where(rng.random((H, W, 1)) < 0.3, noise, base).astype(np.uint8)


def _batch(shapes=SHAPES):
    """(host images, guarded device buffer, its packed view): computed once per shape list, never written"""
    key = tuple(shapes)
    if key not in _images_cache:
        rng = np.random.default_rng(29)
        _images_cache[key] = [_image(rng, H, W) for H, W in shapes]
    imgs = _images_cache[key]
    flat = np.concatenate([i.reshape(-1) for i in imgs])
    buf = torch.full((2 * GUARD + len(flat), ), 0xA5, dtype=torch.uint8, device=DEV)
    buf[GUARD:GUARD + len(flat)] = torch.from_numpy(flat).to(DEV)
    return imgs, buf, buf[GUARD:GUARD + len(flat)]


def _guards_intact(buf):
    host = buf.cpu().numpy()
    return bool((host[:GUARD] == 0xA5).all() and (host[-GUARD:] == 0xA5).all())


def _split(packed, shapes):
    return [v.cpu().numpy() for v in image_views(packed, shapes)]


def _labels_for(H, W, height):
    """inside; across each border and corner; outside; the ends of the coordinate range; empty and blank; all 95
    characters; 256 characters running off the image; two that overlap; one that leaves through the bottom right corner
    into what follows the image in the packed run"""
    w, asc, desc = text_size('Ag', height)
    cx, cy = W // 2, H // 2
    return [('Ag', (cx - w // 2, cy + asc // 3)),
            ('Ag', (-w // 2, cy)), ('Ag', (W - w // 2, cy)), ('Ag', (cx, asc // 2)), ('Ag', (cx, H + asc // 2 - 1)),
            ('gQ', (-w // 2, asc // 2)), ('gQ', (W - w // 2, asc // 2)), ('gQ', (-w // 2, H + asc // 3)), ('jy@', (W - w // 2, H + asc // 3)),
            ('Out', (W + 3, cy)), ('Out', (0, -desc - 3)), ('Out', (-3 * w - 40, cy)), ('Out', (0, H + asc + 3)),
            ('M', (2 ** 20, 2 ** 20)), ('M', (-2 ** 20, -2 ** 20)), ('M', (2 ** 20, cy)), ('M', (cx, -2 ** 20)),
            ('', (cx, cy)), ('   ', (cx, cy)),
            (ALL95, (-int(0.35 * w), max(asc, H // 3))),
            ('Wm#' * 85 + 'W', (1, H - desc)),
            ('Over', (cx // 2, H // 2 + asc)), ('lap', (cx // 2 + w // 2, H // 2 + asc + asc // 4))]


@pytest.mark.parametrize('height', [4, 7.5, 16, 40, 200])
def test_labels_bit_exact_on_mixed_batch(height):
    imgs, buf, packed = _batch()
    labels = [_labels_for(H, W, height) for H, W in SHAPES]
    assert len(labels[0][20][0]) == 256 and len(ALL95) == 95
    before = buf.clone()
    color = (255, 0, 0) if height != 16 else (7, 250, 33)
    Rn.LAUNCH_LOG.clear()
    out = draw_labels((packed, SHAPES), labels, color, height)
    assert Rn.LAUNCH_LOG == ['dbn_draw_glyphs']
    out2 = draw_labels((packed, SHAPES), labels, color, height)
    # in place, into a guarded buffer of its own that already holds the picture
    buf2 = before.clone()
    inplace = draw_labels((packed, SHAPES), labels, color, height, out=buf2[GUARD:GUARD + packed.numel()])
    torch.cuda.synchronize()
    assert out.is_cuda and out.dtype == torch.uint8 and out.shape == packed.shape and out.data_ptr() != packed.data_ptr()
    assert torch.equal(buf, before) and torch.equal(out, out2)  # the input and its guards are not written; two runs agree
    assert inplace.data_ptr() == buf2[GUARD:].data_ptr() and torch.equal(inplace, out) and _guards_intact(buf2)
    painted = 0
    for n, got in enumerate(_split(out, SHAPES)):
        ref = LR.draw_labels(imgs[n], labels[n], color, height)
        assert np.array_equal(got, ref), (height, n, np.argwhere((got != ref).any(-1))[:4])
        mask = LR.label_mask(SHAPES[n][0], SHAPES[n][1], labels[n], height)
        assert np.array_equal(got[~mask], imgs[n][~mask])  # every unpainted byte is the source's
        painted += int(mask.sum())
    assert painted > 500


@pytest.mark.parametrize('height', [7.5, 16])
def test_background_then_text(height):
    imgs, buf, packed = _batch()
    labels = [_labels_for(H, W, height)[:9] + [('', (W // 2, H // 2))] for H, W in SHAPES]
    before = buf.clone()
    Rn.LAUNCH_LOG.clear()
    out = draw_labels((packed, SHAPES), labels, (250, 240, 0), height, background=(0, 0, 64))
    assert Rn.LAUNCH_LOG == ['dbn_draw_glyphs', 'dbn_draw_glyphs']
    buf2 = before.clone()
    inplace = draw_labels((packed, SHAPES), labels, (250, 240, 0), height, background=(0, 0, 64), out=buf2[GUARD:GUARD + packed.numel()])
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and torch.equal(inplace, out) and _guards_intact(buf2)
    for n, got in enumerate(_split(out, SHAPES)):
        ref = LR.draw_labels(imgs[n], labels[n], (250, 240, 0), height, background=(0, 0, 64))
        assert np.array_equal(got, ref), (height, n)
    bm = LR.background_mask(200, 333, labels[4], height)
    assert bm.sum() > 4 * LR.label_mask(200, 333, labels[4], height).sum() > 0


def test_no_glyphs_at_all():
    """R = 0: empty lists, empty strings, blanks; the result is the copy (or, in place, nothing happens); an empty batch"""
    imgs, buf, packed = _batch()
    before = buf.clone()
    for labels in ([[] for _ in SHAPES], [[('', (0, 0)), ('  ', (0, 0))] for _ in SHAPES]):
        for bg in (None, (1, 2, 3)):
            Rn.LAUNCH_LOG.clear()
            out = draw_labels((packed, SHAPES), labels, background=bg)
            assert Rn.LAUNCH_LOG == ['dbn_draw_glyphs'] * (2 if bg else 1)
            torch.cuda.synchronize()
            if bg is None or not labels[0]:
                assert torch.equal(out, packed)
            else:  # a blank label still has its background
                for n, got in enumerate(_split(out, SHAPES)):
                    assert np.array_equal(got, LR.draw_labels(imgs[n], labels[n], background=bg)), n
    buf2 = before.clone()
    same = draw_labels((packed, SHAPES), [[] for _ in SHAPES], out=buf2[GUARD:GUARD + packed.numel()])
    torch.cuda.synchronize()
    assert torch.equal(buf2, before) and same.data_ptr() == buf2[GUARD:].data_ptr() and torch.equal(buf, before)
    one = torch.from_numpy(imgs[2]).to(DEV)
    single = draw_labels(one, [('Hi', (3, 30))])  # a single image takes the list of labels itself
    torch.cuda.synchronize()
    assert np.array_equal(single.cpu().numpy().reshape(37, 53, 3), LR.draw_labels(imgs[2], [('Hi', (3, 30))]))


def test_records_the_kernel_must_skip():
    """the C entry point itself: records whose image, glyph, pen or origin is out of range, an image whose descriptor
    leaves the buffer or is degenerate, a glyph whose index entry is broken: all skipped, the good record beside them drawn"""
    imgs, buf, packed = _batch()
    before = buf.clone()
    N, n = len(SHAPES), packed.numel()
    off = Pk.offsets([h * w * 3 for h, w in SHAPES])
    desc = np.stack([off[:-1], [h for h, _ in SHAPES], [w for _, w in SHAPES]], 1).astype(np.int64)
    desc[0] = 0, 1, 65536             # a side past 65535
    desc[1] = -3, 5, 3                # starts before the buffer
    desc[2] = n - 10, 37, 53          # runs past its end
    desc[3] = off[3], 0, 1            # no rows
    f = Rn.glyph_table()
    index = np.concatenate([f['index'], f['index'][[ord('A') - 32] * 4]])
    G0 = len(f['index'])
    index[G0 + 0, 1] = 513                                  # more edges than the stage holds
    index[G0 + 1, 0] = len(f['edges']) - 3                  # its edges leave the array
    index[G0 + 2, 5] = 2 ** 20 + 1                          # a box outside the range
    index[G0 + 3, 5] = index[G0 + 3, 3] + (2 ** 27) // 1405 + 1  # a box too tall for 64-bit products at this size
    A, big = ord('A') - 32, 2 ** 20
    recs = np.array([[4, A, 0, 10, 100],                                             # the good one
                     [-1, A, 0, 1, 1], [N, A, 0, 1, 1], [2 ** 31 - 1, A, 0, 1, 1],    # image
                     [4, -1, 0, 1, 20], [4, len(index), 0, 1, 20],                    # glyph
                     [4, A, -1, 1, 20], [4, A, big + 1, 1, 20],                       # pen
                     [4, A, 0, big + 1, 20], [4, A, 0, 1, -big - 1], [4, A, 0, -2 ** 31, 2 ** 31 - 1],  # origin
                     [0, A, 0, 0, 1], [1, A, 0, 0, 4], [2, A, 0, 1, 20], [3, A, 0, 0, 20],  # descriptors
                     [4, G0, 0, 1, 20], [4, G0 + 1, 0, 1, 20], [4, G0 + 2, 0, 1, 20], [4, G0 + 3, 0, 1, 20],
                     [4, 0, 0, 1, 20]], np.int32)                                     # the space: no edges
    d, e, g, r = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (desc, f['edges'], index.astype(np.int32), recs))
    buf2 = before.clone()
    dst = buf2[GUARD:GUARD + n]
    st = torch.cuda.current_stream().cuda_stream
    check(lib().dbn_draw_glyphs(packed.data_ptr(), dst.data_ptr(), n, d.data_ptr(), N, e.data_ptr(), len(f['edges']), g.data_ptr(), len(index),
                                r.data_ptr(), len(recs), 1405, 40, 9, 8, 7, st), 'draw_glyphs')
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and _guards_intact(buf2)
    for i, got in enumerate(_split(dst, SHAPES)):
        ref = LR.draw_labels(imgs[i], [('A', (10, 100))], (9, 8, 7)) if i == 4 else imgs[i]
        assert np.array_equal(got, ref), i
    assert (ref != imgs[4]).any()
    # `rows` only sizes the grid: 1 and 65535 give the same bytes
    recs2 = torch.from_numpy(Rn.label_records([[], [], [], [], [('Qg', (5, 150))]], N)).to(DEV)
    d = torch.from_numpy(np.stack([off[:-1], [h for h, _ in SHAPES], [w for _, w in SHAPES]], 1).astype(np.int64)).to(DEV)
    want = LR.draw_labels(imgs[4], [('Qg', (5, 150))], (9, 8, 7), 100)
    for rows in (1, 65535):
        check(lib().dbn_draw_glyphs(packed.data_ptr(), dst.data_ptr(), n, d.data_ptr(), N, e.data_ptr(), len(f['edges']), g.data_ptr(), G0,
                                    recs2.data_ptr(), len(recs2), LR.size64(100), rows, 9, 8, 7, st), 'draw_glyphs')
        torch.cuda.synchronize()
        assert np.array_equal(_split(dst, SHAPES)[4], want) and _guards_intact(buf2)


WORD_SHAPES = [(100, 60), (250, 333), (37, 53)]  # anchor dots of diameter 1, 2 and none


def _words(shapes):
    out = []
    for k, (H, W) in enumerate(shapes):
        out.append([{'box': np.array([[W // 4, H // 2], [W, H // 2], [W, H], [W // 4, H]], np.int16), 'pred': 'word%d' % k, 'score': 0.5},
                    {'box': np.array([[0, 0], [5, 0], [5, 5], [0, 5]], np.int16), 'pred': 'at0', 'score': 0.25},
                    {'box': np.array([[W - 1, H - 1], [W + 5, H - 1], [W + 5, H + 5], [W - 1, H + 5]], np.int16), 'pred': '', 'score': 0.0}])
    return out


def test_draw_words_is_dots_then_labels():
    imgs, buf, packed = _batch(WORD_SHAPES)
    before = buf.clone()
    words = _words(WORD_SHAPES)
    anchors = [[(int(w['box'][0, 0]), int(w['box'][0, 1])) for w in ws] for ws in words]
    labels = [[(w['pred'], a) for w, a in zip(ws, an)] for ws, an in zip(words, anchors)]
    Rn.LAUNCH_LOG.clear()
    got = draw_words((packed, WORD_SHAPES), words)
    log = list(Rn.LAUNCH_LOG)
    assert log == ['dbn_draw_strokes', 'dbn_draw_strokes', 'dbn_draw_glyphs']
    Rn.LAUNCH_LOG.clear()
    dots = draw_dots((packed, WORD_SHAPES), anchors, (0, 255, 0))
    kept = dots.clone()
    two = draw_labels((packed, WORD_SHAPES), labels, (255, 0, 0), 16, out=dots)
    assert Rn.LAUNCH_LOG == log
    Rn.LAUNCH_LOG.clear()
    plain = draw_words((packed, WORD_SHAPES), words, dots=False, height=12)
    assert Rn.LAUNCH_LOG == ['dbn_draw_glyphs']
    torch.cuda.synchronize()
    assert torch.equal(got, two) and two.data_ptr() == dots.data_ptr() and torch.equal(buf, before)
    assert torch.equal(plain, draw_labels((packed, WORD_SHAPES), labels, height=12))
    for n, (H, W) in enumerate(WORD_SHAPES):
        d = int(H * 0.01)
        ref = imgs[n].copy()
        for x, y in anchors[n]:
            if d:
                y0, x0, m = R.edge_mask(H, W, x, y, x, y, d)
                ref[y0:y0 + m.shape[0], x0:x0 + m.shape[1]][m] = (0, 255, 0)
        assert (d > 0) == bool((ref != imgs[n]).any())
        assert np.array_equal(_split(kept, WORD_SHAPES)[n], ref), n  # the dots against the stroke restatement
        assert np.array_equal(_split(got, WORD_SHAPES)[n], LR.draw_labels(ref, labels[n])), n


def test_draw_scores_is_draw_labels_of_the_formatted_scores():
    imgs, buf, packed = _batch(WORD_SHAPES)
    boxes = [np.array([[[W // 5, H // 2], [W, H // 2], [W, H], [W // 5, H]], [[0, 0], [0, 0], [0, 0], [0, 0]]], np.int16) for H, W in WORD_SHAPES]
    dets = [(boxes[0], np.array([0.87654, 0.5], np.float32)), ([np.array([[3, 30], [9, 30], [5, 40]], np.int64)], [0.5]), (boxes[2][:0], [])]
    want_labels = [[('0.88', (12, 50))], [('0.50', (3, 30))], []]
    assert Rn.score_labels(dets, 3) == want_labels
    Rn.LAUNCH_LOG.clear()
    got = draw_scores((packed, WORD_SHAPES), dets, color=(0, 0, 255), height=10)
    assert Rn.LAUNCH_LOG == ['dbn_draw_glyphs']
    same = draw_labels((packed, WORD_SHAPES), want_labels, (0, 0, 255), 10)
    pct = draw_scores((packed, WORD_SHAPES), dets, fmt='%.0f%%', height=10)
    torch.cuda.synchronize()
    assert torch.equal(got, same)
    for n, g in enumerate(_split(got, WORD_SHAPES)):
        assert np.array_equal(g, LR.draw_labels(imgs[n], want_labels[n], (0, 0, 255), 10)), n
    assert np.array_equal(_split(pct, WORD_SHAPES)[0], LR.draw_labels(imgs[0], [('1%', (12, 50))], height=10))


def test_render_detections_defaults_unchanged_and_labels_last():
    imgs, buf, packed = _batch(WORD_SHAPES)
    before = buf.clone()
    rng = np.random.default_rng(31)
    prob = torch.from_numpy(rng.random((3, 1, 32, 48)).astype(np.float32)).to(DEV)
    boxes = [np.array([[[W // 5, H // 2], [W - 2, H // 2], [W - 2, H - 2], [W // 5, H - 2]]], np.int16) for H, W in WORD_SHAPES]
    dets = [(b, np.array([0.5 + 0.1 * k], np.float32)) for k, b in enumerate(boxes)]
    words = _words(WORD_SHAPES)
    Rn.LAUNCH_LOG.clear()
    base = render_detections((packed, WORD_SHAPES), prob, dets)
    assert Rn.LAUNCH_LOG == ['dbn_draw_strokes', 'dbn_render_minmax', 'dbn_render_paint']
    lines = draw_outlines((packed, WORD_SHAPES), dets)
    two = overlay_heatmap((packed, WORD_SHAPES), prob, out=lines)
    Rn.LAUNCH_LOG.clear()
    no_map = render_detections((packed, WORD_SHAPES), prob, dets, heatmap=False)
    assert Rn.LAUNCH_LOG == ['dbn_draw_strokes']
    Rn.LAUNCH_LOG.clear()
    full = render_detections((packed, WORD_SHAPES), prob, dets, words=words, scores=True, height=12)
    assert Rn.LAUNCH_LOG == ['dbn_draw_strokes', 'dbn_render_minmax', 'dbn_render_paint', 'dbn_draw_glyphs', 'dbn_draw_strokes', 'dbn_draw_strokes',
                             'dbn_draw_glyphs']
    seq = draw_words((packed, WORD_SHAPES), words, (255, 0, 0), 12, out=draw_scores((packed, WORD_SHAPES), dets, color=(255, 0, 0), height=12, out=two.clone()))
    only_words = render_detections((packed, WORD_SHAPES), prob, dets, heatmap=False, words=words)
    torch.cuda.synchronize()
    assert torch.equal(base, two) and torch.equal(no_map, draw_outlines((packed, WORD_SHAPES), dets)) and torch.equal(buf, before)
    assert torch.equal(full, seq) and not torch.equal(full, base)
    assert torch.equal(only_words, draw_words((packed, WORD_SHAPES), words, out=draw_outlines((packed, WORD_SHAPES), dets)))


def test_end_to_end_scores_from_probability_map():
    """rectangles in a probability map -> detect_boxes(dest_sizes) -> draw_scores: the painted pixels are exactly the
    restatement's for the formatted scores at the boxes' first corners, every other pixel is the source's"""
    Hm, Wm = 128, 128
    sizes = [(256, 256), (200, 380)]
    rects = [[((10, 40, 10, 20), 0.9), ((60, 110, 30, 45), 0.99), ((20, 70, 70, 80), 0.75)], [((5, 120, 5, 25), 0.95), ((30, 60, 60, 100), 0.72)]]
    pred = torch.zeros((2, 1, Hm, Wm), dtype=torch.float32)
    for n, rs in enumerate(rects):
        for (x0, x1, y0, y1), p in rs:
            pred[n, 0, y0:y1, x0:x1] = p
    res = detect_boxes(pred.to(DEV), dest_sizes=sizes)
    rng = np.random.default_rng(33)
    imgs = [_image(rng, H, W) for H, W in sizes]
    packed = torch.from_numpy(np.concatenate([i.reshape(-1) for i in imgs])).to(DEV)
    out = draw_scores((packed, sizes), res, color=(0, 255, 255), height=14)
    torch.cuda.synchronize()
    texts = []
    for n, got in enumerate(_split(out, sizes)):
        labels = [('%.2f' % float(s), (int(b[0, 0]), int(b[0, 1]))) for b, s in zip(res[n][0], res[n][1]) if b.astype(np.int64).sum() > 0]
        texts += [t for t, _ in labels]
        mask = LR.label_mask(sizes[n][0], sizes[n][1], labels, 14)
        assert mask.sum() > 100 and (got[mask] == (0, 255, 255)).all() and np.array_equal(got[~mask], imgs[n][~mask])
    assert len(texts) == 5 and all(len(t) == 4 and t[:2] in ('0.', '1.') for t in texts)
