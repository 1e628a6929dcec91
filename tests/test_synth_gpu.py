"""GPU (-m gpu): the synthetic scene text on the device (csrc/synth.hip, db_text_minimal_amd/synth.py), every
byte against the numpy restatement tests/synth_ref.py; SynthTextBatches through DeviceBatches, one training step, detection and scoring."""
import math

import numpy as np
import pytest
import torch

from db_text_minimal_amd import DBLoss, DBTextModel, DBTrainer, DetectionIoUEvaluator, FusedAdam, detect_boxes
from db_text_minimal_amd import _lib
from db_text_minimal_amd import augment as A
from db_text_minimal_amd import synth as S
from db_text_minimal_amd.gt_maps import GT_KEYS, make_gt_maps, plan_polygons
from db_text_minimal_amd.render import glyph_table
import synth_ref as R

pytestmark = pytest.mark.gpu
L = R.L
DEV = 'cuda:0'


def inst(ch, cap, x, y, degrees=0.0, shear=0.0, mirror=False):
    """one instance row (glyph, a00, a01, a10, a11, tx, ty): the pen at pixel (x, y)"""
    k = cap / 1493.0
    c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    M = np.array([[c, -s], [s, c]]) @ np.array([[1.0, -shear], [0.0, 1.0]]) @ np.diag([-k if mirror else k, -k])
    return [R.glyph_of(ch)] + [int(v) for v in np.rint(M.reshape(-1) * L)] + [int(round(x * L)), int(round(y * L))]


def word(text, cap, x, y, colour, degrees=0.0, shear=0.0):
    """a straight word: the pen moves along the rotated baseline"""
    rows, pen = [], 0.0
    c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    for ch in text:
        if R.font()['contours'][R.glyph_of(ch)]:
            rows.append(inst(ch, cap, x + c * pen, y + s * pen, degrees, shear))
        pen += R.font()['adv'][R.glyph_of(ch)] * cap / 1493.0
    return {'colour': colour, 'instances': np.array(rows, np.int64).reshape(-1, 7)}


def one(row, colour):
    return {'colour': colour, 'instances': np.array([row], np.int64)}


def plan(base, amps, seed, words):
    return {'base': base, 'amps': amps, 'seed': seed, 'words': words}


def batch():
    most = chr(32 + int(np.argmax([sum(len(c) for c in cs) for cs in R.font()['contours']])))  # the glyph with the most edges
    T = S.TILE
    shapes = [(1, 1), (5, 3), (37, 53), (64, 1), (T + 1, T + 1), (96, 130), (40, 90), (40, 90), (300, 300)]
    a, b = word('Wg', 20, 8, 26, (250, 20, 30)), word('oM', 20, 20, 30, (10, 240, 60))  # overlapping, of different colours
    big = [one(inst(ch, 12, x - 4, y + 6, 20), (255, 255, 0)) for x in (32, 64, 96, 128) for y in (32, 64) for ch in 'O']  # across every tile corner
    border = [one(inst('B', 14, x, y), (0, 255, 255)) for x, y in ((-5, 40), (125, 50), (60, 5), (60, 100), (-4, 6), (126, 6), (-4, 99), (126, 99))]
    outside = [one(inst('B', 14, x, y), (9, 9, 9)) for x, y in ((-100, 50), (500, 500), (60, -40), (60, 4000))]
    turned = [one(inst('R', 16, 20 + 24 * q, 60, 90 * q), (200, 0, 200)) for q in range(4)]
    turned += [one(inst('k', 18, 70, 90, 17, 0.2), (0, 0, 0)), one(inst('F', 16, 120, 88, 0, 0, True), (255, 255, 255))]
    caps = [word('ag8', 4, 3, 12, (255, 0, 0)), word('ag8', 7.5, 3, 24, (0, 0, 255)), one(inst(most, 40, 85, 60), (30, 60, 90))]
    plans = [plan((255, 0, 10), (0, 0, 0), 1, [one(inst('I', 8, -2, 4), (0, 9, 0))]),
             plan((0, 0, 0), (64, 64, 64), 2, [word('ab', 4, 0, 4, (255, 255, 255))]),
             plan((128, 100, 90), (24, 8, 3), 3 << 32, [word('Synth', 12, 2, 20, (20, 20, 20), 25)]),
             plan((200, 200, 50), (10, 20, 30), 4, [one(inst('l', 40, -5.5, 50), (0, 0, 0))]),
             plan((90, 128, 255), (64, 0, 0), 5, [one(inst('X', 16, T - 7, T + 1), (255, 128, 0)), one(inst('.', 30, T - 2, T + 1), (1, 2, 3))]),
             plan((60, 70, 80), (20, 20, 20), 6 | 7 << 32, big + border + outside + turned + caps),
             plan((128, 128, 128), (0, 24, 0), 8, [a, b]), plan((128, 128, 128), (0, 24, 0), 8, [b, a]),
             plan((250, 250, 250), (3, 3, 3), 9, [one(inst('W', 256, 10, 280), (0, 60, 0)),
                                                  word(''.join(chr(c) for c in range(32, 127)), 4, 6, 12, (200, 0, 0), 40, 0.1)])]
    return shapes, plans


def reference(shapes, plans, backgrounds=None):
    recs = S.synth_records(shapes, plans)[0]
    bgs = [(p['base'], p['amps'], p['seed']) for p in plans] if backgrounds is None else backgrounds
    return R.render(shapes, bgs, recs)


_shared = {}


def shared():
    """the batch and its restatement, computed once"""
    if not _shared:
        shapes, plans = batch()
        _shared.update(shapes=shapes, plans=plans, want=reference(shapes, plans))
    return _shared['shapes'], _shared['plans'], _shared['want']


def split(packed, shapes):
    host, off = packed.cpu().numpy(), 0
    out = []
    for h, w in shapes:
        out.append(host[off:off + 3 * h * w].reshape(h, w, 3))
        off += 3 * h * w
    return out


def test_one_packed_batch_equals_the_restatement_between_guards():
    shapes, plans, want = shared()
    need = sum(3 * h * w for h, w in shapes)
    buf = torch.full((need + 64, ), 0xA5, dtype=torch.uint8, device=DEV)
    out = S.render_synth_text(shapes, plans, DEV, out=buf[7:7 + need])  # an odd address; image offsets 3, 48, 5931, ... are odd too
    assert out.data_ptr() == buf.data_ptr() + 7
    got = split(out, shapes)
    for n, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (n, int((g != w).sum()))
    host = buf.cpu().numpy()
    assert (host[:7] == 0xA5).all() and (host[7 + need:] == 0xA5).all()
    # the instances did paint: each image differs from its background, the two record orders from each other
    for n, p in enumerate(plans):
        assert not np.array_equal(want[n], R.background(*shapes[n], p['base'], p['amps'], p['seed'])), n
    assert not np.array_equal(want[6], want[7]) and (want[6] != want[7]).sum() > 30
    recs, bins, _ = S.synth_records(shapes, plans)
    T = sum(-(-h // S.TILE) * -(-w // S.TILE) for h, w in shapes)
    assert np.diff(np.concatenate([[4 * T], bins[3:4 * T:4]])).max() >= 6 and len(recs) > 130


def test_empty_batch_and_flat_background():
    shapes = [(33, 70), (2, 2)]
    plans = [plan((1, 2, 3), (64, 64, 64), 1 << 63 | 5, []), plan((7, 8, 9), (0, 0, 0), 0, [])]  # R = 0
    got = split(S.render_synth_text(shapes, plans, DEV), shapes)
    assert np.array_equal(got[0], R.background(33, 70, (1, 2, 3), (64, 64, 64), 1 << 63 | 5)) and (got[1] == np.array([7, 8, 9], np.uint8)).all()
    assert len(np.unique(got[0])) > 20


def test_kernel_skips_what_it_must():
    """Through the entry point with every record listed in every tile: an instance with |a| >= 2^19, |t| > 2^35 or a span >= 2^30 is
    skipped by its numbers; a device record whose image or glyph disagrees with the checked host copy is skipped too."""
    shapes = [(40, 40), (20, 50)]
    f = glyph_table()
    G = len(f['index_all'])
    lim = (1 << 19) - 1
    rows = [[0] + inst('A', 20, 5, 30) + [0x0000FF], [0, R.glyph_of('W'), 1 << 19, 0, 0, -5000, 0, 30 * L, 0x00FF00], [0] + inst('A', 20, 5, 30)[:5] + [(1 << 35) + 1, 30 * L, 0x00FF00],
            [0, R.glyph_of('W'), lim, lim, 0, -lim, -(1 << 29), (1 << 29), 0xFF0000], [0] + inst('B', 20, 15, 32) + [0x00FFFF], [0] + inst('C', 20, 20, 34) + [0xFFFF00],
            [0] + inst('e', 24, 12, 36, 30) + [0x102030], [1] + inst('D', 16, 5, 18) + [0xFF00FF], [1] + inst('E', 16, 25, 18) + [0x80FF80]]
    recs = np.array(rows, np.int64)
    dev_recs = recs.copy()
    dev_recs[4, 0], dev_recs[5, 1], dev_recs[7, 0], dev_recs[8, 1] = 2, G, -1, -1  # only the device copies
    desc = S.synth_records(shapes, [plan((10, 20, 30), (5, 5, 5), 1, []), plan((200, 100, 50), (0, 0, 9), 2, [])])[2]
    tiles = [[0, y, x] for y in (0, 32) for x in (0, 32)] + [[1, 0, x] for x in (0, 32)]
    lists = [[r for r in range(len(recs)) if recs[r, 0] == t[0]] for t in tiles]
    ends = 4 * len(tiles) + np.cumsum([len(m) for m in lists])
    bins = np.array([v for t, e in zip(tiles, ends) for v in t + [int(e)]] + [r for m in lists for r in m], np.int32)
    need = sum(3 * h * w for h, w in shapes)
    out = torch.zeros(need, dtype=torch.uint8, device=DEV)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    d, r, b, e, g = up(desc), up(dev_recs), up(bins), up(f['edges_all']), up(f['index_all'])
    index = np.ascontiguousarray(f['index_all'])
    _lib.check(_lib.lib().dbn_synth_text_u8(None, out.data_ptr(), need, desc.ctypes.data, d.data_ptr(), 2, recs.ctypes.data, r.data_ptr(), len(recs), bins.ctypes.data,
                                            b.data_ptr(), len(tiles), len(bins), e.data_ptr(), len(f['edges_all']), index.ctypes.data, g.data_ptr(), G,
                                            torch.cuda.current_stream().cuda_stream), 'synth')
    got = split(out, shapes)
    want = R.render(shapes, [((10, 20, 30), (5, 5, 5), 1), ((200, 100, 50), (0, 0, 9), 2)], dev_recs)
    only = R.render(shapes, [((10, 20, 30), (5, 5, 5), 1), ((200, 100, 50), (0, 0, 9), 2)], recs[[0, 6]])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(want[0], only[0]) and np.array_equal(want[1], R.background(20, 50, (200, 100, 50), (0, 0, 9), 2))  # the rest was skipped


def test_backgrounds_out_and_refusals():
    shapes, plans, _ = shared()
    shapes, plans = shapes[2:7], plans[2:7]
    need = sum(3 * h * w for h, w in shapes)
    rng = np.random.RandomState(3)
    photos = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes]
    packed = torch.from_numpy(np.concatenate([p.reshape(-1) for p in photos])).to(DEV)
    before = packed.clone()
    got = split(S.render_synth_text(shapes, plans, backgrounds=packed), shapes)
    want = reference(shapes, plans, photos)
    recs = S.synth_records(shapes, plans)[0]
    for n, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), n
        cov = sum(R.coverage(*shapes[n], R.font()['contours'][r[1]], r[2:6], r[6:8]) for r in recs.tolist() if r[0] == n and R.font()['contours'][r[1]])
        assert np.array_equal(g[cov == 0], photos[n][cov == 0]) and (cov == 0).any() and (g[cov > 0] != photos[n][cov > 0]).any()  # untouched where nothing covers
    assert torch.equal(packed, before)
    out = torch.zeros(need, dtype=torch.uint8, device=DEV)
    assert S.render_synth_text(shapes, plans, out=out, backgrounds=packed) is out and np.array_equal(split(out, shapes)[3], want[3])
    both = torch.zeros(2 * need, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match='overlap'):
        S.render_synth_text(shapes, plans, backgrounds=both[:need], out=both[need - 1:2 * need - 1])
    with pytest.raises(ValueError, match='overlap'):
        S.render_synth_text(shapes, plans, backgrounds=packed, out=packed)
    with pytest.raises(ValueError, match='bytes'):
        S.render_synth_text(shapes, plans, DEV, out=both)
    with pytest.raises(ValueError, match='bytes'):
        S.render_synth_text(shapes, plans, backgrounds=both)
    with pytest.raises(ValueError, match='GPU'):
        S.render_synth_text(shapes, plans, DEV, backgrounds=packed.cpu())
    with pytest.raises(ValueError, match='GPU'):
        S.render_synth_text(shapes, plans, 'cpu')
    with pytest.raises(ValueError, match='one plan per image'):
        S.render_synth_text(shapes[:2], plans, DEV)


def _inside_polygon(poly, pts, slack):
    a, b = poly, np.roll(poly, -1, 0)
    x, y = pts[:, 0][:, None], pts[:, 1][:, None]
    cross = ((a[:, 1] <= y) != (b[:, 1] <= y)) & (x < a[:, 0] + (y - a[:, 1]) * (b[:, 0] - a[:, 0]) / np.where(b[:, 1] == a[:, 1], 1.0, b[:, 1] - a[:, 1]))
    d = b - a
    t = np.clip(((x - a[:, 0]) * d[:, 0] + (y - a[:, 1]) * d[:, 1]) / np.maximum((d * d).sum(1), 1e-300), 0.0, 1.0)
    return (cross.sum(1) % 2 == 1) | (np.hypot(a[:, 0] + t * d[:, 0] - x, a[:, 1] + t * d[:, 1] - y).min(1) <= slack)


KW = dict(height=(24, 40), words=(1, 3), length=(2, 5))


@pytest.mark.parametrize('training', [True, False])
def test_synth_batches_through_device_batches(training):
    size = 64
    source = S.SynthTextBatches(2, 2, (96, 128), seed=11, device=DEV, **KW)
    batches = list(A.DeviceBatches(source, DEV, training=training, size=size, seed=4, min_text_size=4))
    again = list(A.DeviceBatches(S.SynthTextBatches(2, 2, (96, 128), seed=11, device=DEV, **KW), DEV, training=training, size=size, seed=4, min_text_size=4))
    assert len(batches) == len(source) == 2
    rng = np.random.RandomState(4)
    positives = 0
    for b, (batch, twice) in enumerate(zip(batches, again)):
        shapes, plans = source.plan(b)
        assert shapes == [(96, 128)] * 2
        packed = S.render_synth_text(shapes, plans, DEV)
        assert all(np.array_equal(g, w) for g, w in zip(split(packed, shapes), reference(shapes, plans)))  # the loader's bytes are the restatement's
        polys, tags = [[w['polygon'] for w in p['words']] for p in plans], [[w['tag'] for w in p['words']] for p in plans]
        aug = A.plan_augment(shapes, polys, rng, size) if training else A.plan_letterbox(shapes, polys, size)
        img = A.augment_images(packed, shapes, aug, size, A.MEAN, torch.device(DEV))
        out_polys, out_tags = [p['polys'] for p in aug], [[tags[i][j] for j in p['keep']] for i, p in enumerate(aug)]
        offsets = None
        if not training:  # as DeviceBatches does for a test batch: the offset polygons planned once
            g = plan_polygons(out_polys, out_tags, size, min_text_size=4)
            offsets = [[(np.zeros((0, 2), np.int64), None) if q['ignored'] else (q['fill'], q['padded']) for q in img_plan] for img_plan in g]
        maps = make_gt_maps(out_polys, out_tags, size, torch.device(DEV), offsets=offsets, min_text_size=4)
        assert batch['img'].shape == (2, 3, size, size) and torch.equal(batch['img'], img) and torch.equal(batch['img'], twice['img'])
        for k, key in enumerate(GT_KEYS):
            assert torch.equal(batch[key], maps[k]) and torch.equal(batch[key], twice[key]), key
        prob = batch['prob_map'].cpu().numpy()
        for i in range(2):
            ys, xs = np.nonzero(prob[i] > 0)
            positives += len(ys)
            if len(ys):
                pts = np.stack([xs, ys], 1).astype(np.float64)
                inside = np.zeros(len(pts), bool)
                for q in out_polys[i]:
                    inside |= _inside_polygon(np.asarray(q, np.float64), pts, 1.0)  # (the fill takes the pixels of the integer outline with it)
                assert inside.all(), (b, i)
    assert positives > 50


def test_one_training_step_detection_and_scoring():
    size = 64
    source = S.SynthTextBatches(1, 2, (96, 128), seed=12, device=DEV, **KW)
    torch.manual_seed(0)
    model = DBTextModel().to(DEV).train()
    trainer = DBTrainer(model, DBLoss(), FusedAdam(model, lr=0.005), distributed=False)
    batch = next(iter(A.DeviceBatches(source, DEV, training=True, size=size, seed=1, min_text_size=4)))
    preds, losses = trainer.step(batch, None)
    assert preds.shape[0] == 2 and torch.isfinite(losses).all() and torch.isfinite(preds).all()
    test = next(iter(A.DeviceBatches(source, DEV, training=False, size=size, min_text_size=4)))
    found = detect_boxes(preds.detach().float().contiguous(), thresh=0.3, box_thresh=0.3)
    gts = [[{'points': np.asarray(p, np.float64), 'ignore': bool(ig)} for p, ig in zip(test['anns'][i], test['ignore_tags'][i])] for i in range(2)]
    dets = [[{'points': bx.astype(np.float64), 'ignore': False} for bx, sc in zip(*found[i]) if sc > 0] for i in range(2)]
    ev = DetectionIoUEvaluator()
    results = ev.evaluate_batch(gts, dets)
    total = ev.combine_results(results)
    assert len(results) == 2 and all(0.0 <= total[k] <= 1.0 for k in ('precision', 'recall', 'hmean'))
    assert sum(r['gtCare'] for r in results) >= 1


def test_command_line_writes_images_and_ground_truth(tmp_path):
    from db_text_minimal_amd.png import decode_png
    assert S.main(['--out', str(tmp_path / 'set'), '--count', '3', '--size', '96', '--seed', '2']) == 0
    shapes, plans = S.SynthTextBatches(1, 16, (96, 96), seed=2).plan(0)
    want = reference(shapes[:3], plans[:3])
    for k in range(3):
        got = decode_png(open(tmp_path / 'set' / ('img_%d.png' % k), 'rb').read(), DEV).cpu().numpy()
        assert np.array_equal(got, want[k]), k
        lines = open(tmp_path / 'set' / ('gt_img_%d.txt' % k)).read().splitlines()
        assert len(lines) == len(plans[k]['words'])
        for line, w in zip(lines, plans[k]['words']):  # x1,y1,...,xV,yV,text
            fields = line.split(',')
            assert fields[-1] == w['text'] and len(fields) == 2 * len(w['polygon']) + 1
            assert np.abs(np.array(fields[:-1], np.float64).reshape(-1, 2) - w['polygon']).max() <= 0.5
    assert not (tmp_path / 'set' / 'img_3.png').exists() and sum(len(p['words']) for p in plans[:3]) > 0
