#!/usr/bin/env python3
"""Generate tests/golden/gt_maps.npz from the REFERENCE's own ground-truth code.

Run in the build container only (needs the reference checkout, and the built library for the offset table; nothing in
the test suite or on the GPU box runs this):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_gt_golden.py

It runs data_loaders.BaseDatasetIter.__getitem__ (is_training=False: no augmentation) and, through it,
db_transforms.resize / draw_thresh_map, with the third-party modules the image lacks replaced by stubs:
  cv2.imread       a seeded uint8 image (8 x 8 blocks, so the fixture compresses); cv2.resize is the identity (the
                   images are generated at the target size, so resize's scale is exactly 1)
  cv2.fillPoly     oracle.postprocess_oracle.fill_poly_mask (the pinned restatement, imported unchanged)
  shapely Polygon  area / length as GEOS computes them (Area::ofRing, Length::ofLine); buffer(0).is_valid is True
  pyclipper        PyclipperOffset.Execute(delta) returns [db_text_minimal_amd.gt_maps.offset_polygon(path, delta)]
                   (or [] if empty) and records it: the offset table stored beside the maps
The fixture holds data only: polygons, tags, the offset table, the uint8 and normalised images and the four maps.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, '/root/reference/src')
sys.dont_write_bytecode = True

from oracle.postprocess_oracle import fill_poly_mask  # noqa: E402
from db_text_minimal_amd.gt_maps import offset_polygon  # noqa: E402

IMAGES = {}
TABLE = {}


def _imread(path):
    return IMAGES[path][:, :, ::-1].copy()  # BGR on disk; the loader flips it back


def _fill_poly(img, pts, color):
    for p in pts:
        img[fill_poly_mask(img.shape[0], img.shape[1], np.asarray(p).reshape(-1, 2)).astype(bool)] = color
    return img


class _Polygon:
    def __init__(self, pts):
        self.r = np.concatenate([np.asarray(pts, np.float64), np.asarray(pts, np.float64)[:1]])

    @property
    def area(self):
        r, s = self.r, 0.0
        if len(r) < 4:
            return 0.0
        for i in range(1, len(r) - 1):
            s += (r[i, 0] - r[0, 0]) * (r[i - 1, 1] - r[i + 1, 1])
        return abs(s / 2.0)

    @property
    def length(self):
        d = np.diff(self.r, axis=0)
        s = 0.0
        for dx, dy in d:
            s += np.sqrt(dx * dx + dy * dy)
        return float(s)

    def buffer(self, _):
        return types.SimpleNamespace(is_valid=True)


class _Offset:
    def AddPath(self, path, *_):
        self.path = tuple(tuple(p) for p in path)

    def Execute(self, delta):
        got = offset_polygon(np.array(self.path), delta)
        TABLE[(self.path, delta > 0)] = got
        return [got.tolist()] if len(got) else []


def _install_stubs():
    cv2 = types.ModuleType('cv2')
    cv2.imread, cv2.resize, cv2.fillPoly = _imread, (lambda img, wh: img), _fill_poly
    shapely, geom = types.ModuleType('shapely'), types.ModuleType('shapely.geometry')
    geom.Polygon = _Polygon
    shapely.geometry = geom
    pyclipper = types.ModuleType('pyclipper')
    pyclipper.PyclipperOffset, pyclipper.JT_ROUND, pyclipper.ET_CLOSEDPOLYGON = _Offset, 1, 2
    iaa = types.ModuleType('imgaug.augmenters')
    imgaug = types.ModuleType('imgaug')
    imgaug.augmenters = iaa
    utils = types.ModuleType('utils')
    utils.dict_to_device = utils.minmax_scaler_img = None
    hydra = types.ModuleType('hydra')
    hydra.main = lambda *a, **k: (lambda f: f)
    for name, mod in (('cv2', cv2), ('shapely', shapely), ('shapely.geometry', geom), ('pyclipper', pyclipper), ('imgaug', imgaug),
                      ('imgaug.augmenters', iaa), ('hydra', hydra), ('utils', utils)):
        sys.modules[name] = mod


def quad(cx, cy, w, h, ang, rng):
    c, s = np.cos(ang), np.sin(ang)
    pts = np.array([[-w / 2, -h / 2], [w / 2, -h / 2], [w / 2, h / 2], [-w / 2, h / 2]])
    pts = pts @ np.array([[c, s], [-s, c]]) + [cx, cy]
    return pts + rng.uniform(-0.49, 0.49, pts.shape)


def curved(cx, cy, r, thick, a0, a1, n, rng):
    """a 2n-point curved text band (CTW1500 / TotalText style: n points on each side)."""
    t = np.linspace(a0, a1, n)
    outer = np.stack([cx + (r + thick) * np.cos(t), cy + (r + thick) * np.sin(t)], 1)
    inner = np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], 1)[::-1]
    return np.concatenate([outer, inner]) + rng.uniform(-0.3, 0.3, (2 * n, 2))


def cases(S, seed):
    """two images of S x S: per image a list of (poly [V, 2] float64, tag)."""
    rng = np.random.default_rng(seed)
    k = S / 640.0
    a = [(quad(120 * k, 90 * k, 150 * k, 36 * k, 0.1, rng), 'abc'),
         (quad(170 * k, 105 * k, 120 * k, 30 * k, -0.2, rng), 'ovl'),  # overlaps the first (fmax, fills)
         (curved(320 * k, 330 * k, 120 * k, 30 * k, 0.3, 2.2, 7, rng), 'curve'),  # 14 points
         (quad(-5 * k + 10, 400 * k, 80 * k, 40 * k, 0.0, rng), 'border'),  # cut by the left border
         (np.array([[S + 12.3, 200.6 * k], [S + 70.2, 200.1 * k], [S + 70.7, 200 * k + 40.4], [S + 12.1, 200 * k + 40.9]]), 'past'),
         (quad(500 * k, 560 * k, 90 * k, 24 * k, 0.4, rng), '###'),
         (quad(400 * k, 80 * k, 30 * k, 5.5, 0.0, rng), 'tiny'),  # min(h, w) < 8
         (np.array([[300.4 * k, 500.2 * k], [300.4 * k + 40.3, 500.2 * k + 8.1], [300.4 * k + 40.9, 500.2 * k + 8.6]]), 'sliver')]
    b = [(curved(200 * k, 250 * k, 90 * k, 26 * k, 3.4, 5.6, 7, rng), 'c2'),
         (quad(420 * k, 420 * k, 200 * k, 50 * k, 0.7, rng), 'q2'),
         (np.array([[100.2 * k, S + 9.6], [180.8 * k, S + 9.1], [181.1 * k, S + 35.4], [99.7 * k, S + 36.0]]), 'below'),
         (quad(60 * k, S - 20 * k, 100 * k, 60 * k, -0.1, rng), 'bottom-cut')]
    return [a, b]


def main():
    _install_stubs()
    import data_loaders  # noqa: E402  (reference)
    out = {}
    for S, seed in ((640, 11), (128, 12)):
        imgs = cases(S, seed)
        ds = data_loaders.BaseDatasetIter.__new__(data_loaders.BaseDatasetIter)
        ds.ignore_tags, ds.is_training, ds.image_size, ds.min_text_size = ['###'], False, S, 8
        ds.shrink_ratio, ds.thresh_min, ds.thresh_max, ds.augment, ds.debug = 0.4, 0.3, 0.7, None, False
        ds.mean = [103.939, 116.779, 123.68]
        ds.image_paths, ds.all_anns = [], []
        rng = np.random.default_rng(seed + 100)
        for i, polys in enumerate(imgs):
            path = 'img_%d_%d' % (S, i)
            IMAGES[path] = np.kron(rng.integers(0, 256, (S // 8, S // 8, 3), dtype=np.uint8), np.ones((8, 8, 1), np.uint8))
            ds.image_paths.append(path)
            ds.all_anns.append([{'poly': p.tolist(), 'text': t} for p, t in polys])
        maps, norm, verts, counts, tags, shr, pad = [], [], [], [], [], [], []
        for i, polys in enumerate(imgs):
            TABLE.clear()
            d = ds[i]
            maps.append(np.stack([d[k] for k in ('prob_map', 'supervision_mask', 'thresh_map', 'text_area_map')]))
            norm.append(d['img'])
            for p, t in polys:
                key = tuple(tuple(q) for q in p.tolist())
                verts.append(p)
                counts.append(len(p))
                tags.append(t)
                shr.append(TABLE.get((key, False)))
                pad.append(TABLE.get((key, True)))
        pref = 's%d/' % S
        out[pref + 'maps'] = np.stack(maps, 1)  # [4, N, S, S]
        out[pref + 'u8'] = np.stack([IMAGES['img_%d_%d' % (S, i)] for i in range(len(imgs))])
        out[pref + 'img'] = np.stack(norm)
        out[pref + 'verts'] = np.concatenate(verts)
        out[pref + 'counts'] = np.array(counts, np.int32)
        out[pref + 'per_image'] = np.array([len(p) for p in imgs], np.int32)
        out[pref + 'tags'] = np.array(tags)
        # offset table: -1 = not asked for (polygon ignored before the shrink / pad), else the point count
        for name, tab in (('shrunk', shr), ('padded', pad)):
            out[pref + name + '_counts'] = np.array([-1 if x is None else len(x) for x in tab], np.int32)
            out[pref + name] = np.concatenate([x for x in tab if x is not None and len(x)]).astype(np.int32)
        print('S=%d: %d polygons, shrunk asked %d, kept %d' % (S, len(counts), sum(x is not None for x in shr), sum(x is not None for x in pad)))
    np.savez_compressed(os.path.join(HERE, 'gt_maps.npz'), **out)
    print('wrote', os.path.join(HERE, 'gt_maps.npz'), os.path.getsize(os.path.join(HERE, 'gt_maps.npz')))


if __name__ == '__main__':
    main()
