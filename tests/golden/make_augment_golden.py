#!/usr/bin/env python3
"""Generate tests/golden/augment_crop.npz from the REFERENCE's own crop and letterbox code.

Needs a checkout of the reference (nothing in the test suite or on the GPU box runs this):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_augment_golden.py <reference checkout>/src

It runs db_transforms.crop and db_transforms.resize on seeded synthetic annotation sets and image shapes, each case under
np.random.seed(seed), with the third-party modules db_transforms imports replaced by stubs (cv2.resize returns zeros of
the requested size and records that size: only the geometry is recorded).  The image handed to crop holds its own coordinates (channel 0 = row,
channel 1 = column), so the crop window is read off the returned image; each annotation's text is its index, so the kept
polygons are read off the returned annotations.
The fixture holds data only: shapes, seeds, input polygons, windows, kept indices, cropped polygons, letterbox scales,
sizes and polygons.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

RESIZED = []  # the (w, h) each cv2.resize call was asked for


def _install_stubs():
    cv2 = types.ModuleType('cv2')
    cv2.resize = lambda img, wh: RESIZED.append(wh) or np.zeros((wh[1], wh[0]) + img.shape[2:], img.dtype)
    shapely, geom = types.ModuleType('shapely'), types.ModuleType('shapely.geometry')
    geom.Polygon = None
    shapely.geometry = geom
    pyclipper = types.ModuleType('pyclipper')
    imgaug = types.ModuleType('imgaug')
    for name, mod in (('cv2', cv2), ('shapely', shapely), ('shapely.geometry', geom), ('pyclipper', pyclipper), ('imgaug', imgaug)):
        sys.modules[name] = mod


def _poly(rng, h, w):
    """a quad or a curved band, clamped to the image as db_transforms.transform leaves it; some vertices integral"""
    cx, cy = rng.uniform(-0.1 * w, 1.1 * w), rng.uniform(-0.1 * h, 1.1 * h)
    if rng.random() < 0.6:
        bw, bh, a = rng.uniform(2, 0.5 * w + 2), rng.uniform(2, 0.2 * h + 2), rng.uniform(-0.4, 0.4)
        c, s = np.cos(a), np.sin(a)
        p = np.array([[-bw, -bh], [bw, -bh], [bw, bh], [-bw, bh]]) / 2 @ np.array([[c, s], [-s, c]]) + [cx, cy]
    else:
        m = int(rng.integers(4, 9))
        r, th, a0 = rng.uniform(5, 0.4 * min(h, w) + 5), rng.uniform(2, 0.1 * min(h, w) + 2), rng.uniform(0, 6)
        t = np.linspace(a0, a0 + rng.uniform(0.3, 2.0), m)
        outer = np.stack([cx + (r + th) * np.cos(t), cy + (r + th) * np.sin(t)], 1)
        inner = np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], 1)[::-1]
        p = np.concatenate([outer, inner])
    if rng.random() < 0.3:
        p = np.round(p)
    p[:, 0] = np.clip(p[:, 0], 0, w - 1)
    p[:, 1] = np.clip(p[:, 1], 0, h - 1)
    return p


def cases():
    rng = np.random.default_rng(2024)
    out = []
    fixed = [(5, 7, 0), (37, 53, 3), (720, 1280, 12), (2160, 3840, 12), (360, 640, 0), (1, 9, 1), (640, 640, 40)]
    for h, w, k in fixed:
        out.append((h, w, [_poly(rng, h, w) for _ in range(k)]))
    out.append((100, 80, [np.array([[0., 10.], [79., 10.], [79., 30.], [0., 30.]])]))   # text across the whole width
    out.append((90, 120, [np.array([[5., 0.], [30., 0.], [30., 89.], [5., 89.]])]))     # ... and the whole height
    for _ in range(33):
        h, w = int(rng.integers(20, 2400)), int(rng.integers(20, 2400))
        out.append((h, w, [_poly(rng, h, w) for _ in range(int(rng.integers(0, 14)))]))
    return out


def main():
    sys.path.insert(0, sys.argv[1])
    _install_stubs()
    import db_transforms as T
    rec = {k: [] for k in ('hw', 'seed', 'size', 'in_count', 'in_verts', 'window', 'kept', 'kept_count', 'crop_verts',
                           'lb_scale', 'lb_hw', 'lb_verts')}
    for c, (h, w, polys) in enumerate(cases()):
        seed = 1000 + 7 * c
        size = 640 if c % 3 else 320
        img = np.zeros((h, w, 3), np.int32)
        img[..., 0] = np.arange(h)[:, None]
        img[..., 1] = np.arange(w)[None, :]
        anns = [{'poly': [tuple(v) for v in p.tolist()], 'text': str(j)} for j, p in enumerate(polys)]
        np.random.seed(seed)
        cimg, canns = T.crop(img, anns)
        y0, x0 = int(cimg[0, 0, 0]), int(cimg[0, 0, 1])
        window = (y0, y0 + cimg.shape[0], x0, x0 + cimg.shape[1])
        limg, lanns = T.resize(size, cimg, canns)
        rec['hw'].append((h, w))
        rec['seed'].append(seed)
        rec['size'].append(size)
        rec['in_count'].append(len(polys))
        rec['in_verts'].extend(polys)
        rec['window'].append(window)
        rec['kept'].extend(int(a['text']) for a in canns)
        rec['kept_count'].append(len(canns))
        rec['crop_verts'].extend(np.asarray(a['poly'], np.float64) for a in canns)
        scale = min(size / cimg.shape[1], size / cimg.shape[0])
        rec['lb_scale'].append(scale)
        rec['lb_hw'].append(RESIZED[-1][::-1])
        rec['lb_verts'].extend(np.asarray(a['poly'], np.float64) for a in lanns)
        assert limg.shape[:2] == (size, size)
    arrays = {}
    for k, v in rec.items():
        if k.endswith('verts'):
            arrays[k] = np.concatenate(v).astype(np.float64) if v else np.zeros((0, 2))
        else:
            arrays[k] = np.asarray(v)
    arrays['poly_count'] = np.asarray([len(p) for p in rec['in_verts']], np.int64)
    arrays['crop_poly_count'] = np.asarray([len(p) for p in rec['crop_verts']], np.int64)
    np.savez_compressed(os.path.join(HERE, 'augment_crop.npz'), **arrays)
    print('cases', len(rec['hw']), 'polygons', len(rec['in_verts']), 'cropped', int(np.sum(arrays['window'][:, 1] - arrays['window'][:, 0] <
                                                                                     arrays['hw'][:, 0])))


if __name__ == '__main__':
    main()
