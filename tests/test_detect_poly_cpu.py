"""CPU (-m "not gpu"): the test model of detect_polygons (tests/detect_poly_ref.py). The collapsed crack cycle equals the
Suzuki outer border (same start, same orientation) on random and adversarial bitmaps, and compression keeps the start
vertex. approxPolyDP and the path count are checked on analytic cases. The library's host stage
(dbn_detect_poly_host, through ctypes) must equal the model bit for bit on synthetic contours."""
import math

import numpy as np
import pytest

from db_text_minimal_amd import postprocess as P
from db_text_minimal_amd.gt_maps import offset_polygon_paths
import detect_poly_ref as M
import detect_ref as R
from test_detect_cpu import outer_border


def roots_of(bm):
    lab = R.label(bm)
    fl = lab.ravel()
    return [int(r) for r in np.nonzero((fl == np.arange(fl.size)) & np.asarray(bm, bool).ravel())[0]]


def check_all_borders(bm):
    bm = np.asarray(bm, bool)
    W = bm.shape[1]
    n = 0
    for r in roots_of(bm):
        y, x = divmod(r, W)
        visits = M.pixel_visits(M.crack_walk(bm, y, x))
        assert visits == outer_border(bm, y, x), (bm.astype(int), y, x)
        c = M.compress(visits)
        assert c[0] == (y, x)  # compression keeps the start vertex
        n += 1
    return n


def spiral(H, W):
    bm = np.zeros((H, W), bool)
    y, x, t, l, b, r = 0, 0, 0, 0, H - 1, W - 1
    while t <= b and l <= r:
        bm[y, x:r + 1] = True
        x = r
        bm[y:b + 1, x] = True
        y = b
        bm[y, l:x + 1] = True
        x = l
        if y > t + 2:
            bm[t + 2:y + 1, x] = True
            y = t + 2
        t, l, b, r = t + 2, l + 2, b - 2, r - 2
    return bm


def test_crack_walk_equals_suzuki_on_random_bitmaps():
    rng = np.random.default_rng(0)
    n = 0
    for trial in range(320):
        kind = trial % 8
        if kind == 0:
            H, W = 1, int(rng.integers(1, 40))
        elif kind == 1:
            H, W = int(rng.integers(1, 40)), 1
        else:
            H, W = int(rng.integers(2, 24)) | 1, int(rng.integers(2, 24)) | 1
        bm = rng.random((H, W)) < [0.15, 0.35, 0.5, 0.65, 0.85][trial % 5]
        n += check_all_borders(bm)
    assert n > 1500


def test_crack_walk_equals_suzuki_on_adversarial_bitmaps():
    yy, xx = np.mgrid[0:23, 0:29]
    cases = [
        (xx + yy) % 2 == 0,  # checkerboard: diagonal-only contacts
        ((xx - yy) % 3 == 0) & (yy < 20),  # diagonal lines
        yy % 3 == 0,  # one-pixel lines
        xx % 4 == 1,
        (xx % 3 == 0) & (yy % 3 == 0),  # single pixels
        np.ones((23, 29), bool),  # touches every edge and corner
        spiral(23, 29),
        spiral(40, 41),
    ]
    ring = np.zeros((15, 15), bool)
    ring[1:14, 1:14] = True
    ring[3:12, 3:12] = False
    ring[6:9, 6:9] = True  # an island in the hole
    ring[7, 7] = False
    cases.append(ring)
    corners = np.zeros((9, 11), bool)
    corners[0, 0] = corners[0, -1] = corners[-1, 0] = corners[-1, -1] = True
    corners[1, 1] = corners[4, 5] = corners[3:6, 0] = True
    cases.append(corners)
    x_shape = np.zeros((7, 7), bool)
    for i in range(7):
        x_shape[i, i] = x_shape[i, 6 - i] = True
    cases.append(x_shape)
    for bm in cases:
        check_all_borders(bm)


def test_compression_of_known_shapes():
    bm = np.zeros((8, 9), bool)
    bm[2:6, 3:8] = True
    c = M.contour(bm, 2, 3)
    assert c.tolist() == [[3, 2], [3, 5], [7, 5], [7, 2]]  # counter-clockwise on screen from the first pixel
    assert M.arc_length(c) == 14.0
    one = np.zeros((3, 3), bool)
    one[1, 1] = True
    assert M.contour(one, 1, 1).tolist() == [[1, 1]]
    diamond = np.zeros((7, 7), bool)
    for d in range(4):
        diamond[3 - d:4 + d, d] = diamond[3 - d:4 + d, 6 - d] = True
    c = M.contour(diamond, 0, 3)
    assert c.tolist() == [[3, 0], [0, 3], [3, 6], [6, 3]]
    assert M.arc_length(c) == 12 * math.sqrt(2.0)


def test_approx_axis_rectangle_gives_its_corners_in_contour_order():
    bm = np.zeros((30, 40), bool)
    bm[4:21, 6:35] = True
    c = M.contour(bm, 4, 6)
    ap = M.approx_poly_dp(c, 0.005 * M.arc_length(c))
    # the initial split starts at vertex 0, goes to its farthest vertex (2) and back (0): output from vertex 0 on
    assert ap == [(6, 4), (6, 20), (34, 20), (34, 4)]


def test_approx_digitised_disk():
    H = W = 61
    yy, xx = np.mgrid[0:H, 0:W]
    bm = (xx - 30) ** 2 + (yy - 30) ** 2 <= 25 ** 2
    r = roots_of(bm)
    assert len(r) == 1
    c = M.contour(bm, *divmod(r[0], W))
    eps = 0.005 * M.arc_length(c)
    ap = M.approx_poly_dp(c, eps)
    assert 8 <= len(ap) <= 40
    cs = set(map(tuple, c.tolist()))
    assert all(tuple(p) in cs for p in ap)
    a = np.array(ap, np.float64)
    for p in c.astype(np.float64):  # every contour vertex within 2 eps of the approximating polygon
        d = min(seg_dist(p, a[i], a[(i + 1) % len(a)]) for i in range(len(a)))
        assert d <= 2 * eps
    # symmetric disk: vertices spread over all four quadrants
    assert all(((a[:, 0] - 30) * sx > 0).any() and ((a[:, 1] - 30) * sy > 0).any() for sx in (1, -1) for sy in (1, -1))


def seg_dist(p, a, b):
    d = b - a
    t = 0.0 if not d.any() else min(1.0, max(0.0, float((p - a) @ d / (d @ d))))
    return float(np.hypot(*(a + t * d - p)))


def test_approx_cleanup_pass_removes_a_vertex():
    pts = [(39, 20), (37, 26), (24, 31), (18, 32), (12, 33), (3, 26)]
    eps = 2.6865
    before = M.approx_poly_dp(pts, eps, cleanup=False)
    after = M.approx_poly_dp(pts, eps)
    assert before == [(39, 20), (37, 26), (24, 31), (12, 33), (3, 26)]
    assert after == [(39, 20), (37, 26), (12, 33), (3, 26)]  # (24, 31): within eps / sqrt(2) of (37, 26) - (12, 33)


def test_approx_tie_at_maximum_distance_takes_the_first():
    # from vertex 0 the farthest is (2, -6); from there (1, 2) and (3, 2) tie at 65: the first in contour order wins
    pts = [(0, 0), (1, 2), (3, 2), (4, 0), (2, -6)]
    ap = M.approx_poly_dp(pts, 0.5)
    assert ap[0] == (1, 2)  # output starts at the third pass's start point
    assert sorted(ap) == sorted(pts)
    # (0, 4) and (8, 4) tie at 592 from (4, -20): the first after it in contour order starts the split, and the
    # slice (0, 4) -> (4, -20) then keeps (8, 4) as its farthest point; the last-wins rule would start at (8, 4)
    sq = [(0, 0), (0, 4), (8, 4), (8, 0), (4, -20)]
    assert M.approx_poly_dp(sq, 3.0) == [(0, 4), (8, 4), (4, -20)]


def test_offset_path_count():
    sq = np.array([[0, 0], [20, 0], [20, 10], [0, 10]], np.float64)
    off, paths = offset_polygon_paths(sq, 3.0)
    assert paths == 1 and len(off) > 4
    # a hook whose 4-pixel mouth closes when grown by 3: outer loop + hole
    hook = np.array([[0, 0], [40, 0], [40, 30], [22, 30], [22, 27], [37, 27], [37, 3], [3, 3], [3, 27], [18, 27], [18, 30], [0, 30]],
                    np.float64)
    off, paths = offset_polygon_paths(hook, 3.0)
    assert paths == 2
    assert offset_polygon_paths(hook, 1.0)[1] == 1  # grown by 1 the mouth stays open


def contours_of(bm):
    W = bm.shape[1]
    return [M.contour(bm, *divmod(r, W)) for r in roots_of(bm)]


def test_host_stage_through_ctypes_equals_the_model():
    rng = np.random.default_rng(4)
    H, W, Mx = 120, 150, 48
    yy, xx = np.mgrid[0:H, 0:W]
    cs = []
    for _ in range(120):  # rotated rectangles, some with a notch cut in
        cx, cy, a = rng.uniform(10, W - 10), rng.uniform(10, H - 10), rng.uniform(0, math.pi)
        L, T = rng.uniform(3, 30), rng.uniform(1.5, 10)
        u = (xx - cx) * math.cos(a) + (yy - cy) * math.sin(a)
        v = -(xx - cx) * math.sin(a) + (yy - cy) * math.cos(a)
        bm = (np.abs(u) <= L) & (np.abs(v) <= T)
        if rng.random() < 0.3:
            bm &= ~((np.abs(u) <= L - 3) & (np.abs(v) <= T - 3) & (u < L / 2))
        cs += contours_of(bm)
    cs += contours_of(spiral(40, 50)) + contours_of((xx % 7 == 0) & (yy < 30))
    rng.shuffle(cs)
    N = 2
    recs = np.zeros((N, Mx), P.REC_DTYPE)
    counts = np.array([Mx + 5, Mx - 7], np.int32)
    nv = np.zeros((N, Mx), np.int32)
    voff = np.zeros((N, Mx), np.int32)
    verts, s64, byslot = [], {}, {}
    at = 0
    for n in range(N):
        for k in range(min(counts[n], Mx)):
            c = cs[n * Mx + k]
            cnt = int(rng.integers(1, 5000))
            tot = int(rng.uniform(0.3, 1.0) * cnt * 2 ** 56) + int(rng.integers(0, 2 ** 20))
            recs[n, k] = (int(c[0, 1]) * W + int(c[0, 0]), 4, 1, 0, 0, 0, 0, 0, tot >> 32, tot & (2 ** 32 - 1), cnt)
            s64[n, k] = tot / (cnt << 56)
            nv[n, k], voff[n, k] = len(c), at
            verts.append(c)
            byslot[n, k] = c
            at += len(c)
    table = dict(recs=recs, counts=counts, nv=nv, voff=voff, verts=np.concatenate(verts).astype(np.int16))
    dest = [(H, W), (360, 450)]
    res, info = P.detect_poly_host(table, H, W, box_thresh=0.6, unclip_ratio=1.5, dest_sizes=dest, return_info=True)
    kept = 0
    for n in range(N):
        polys, scores = res[n]
        want_p, want_s = [], []
        for k in range(min(counts[n], Mx)):
            c = byslot[n, k]
            ap, paths, sside, poly, near = M.host_stage(c, s64[n, k], H, W, 0.6, 1.5, dest[n])
            assert info['score64'][n, k] == s64[n, k] and np.float32(s64[n, k]) == R.fixed_score(recs[n, k]['sum_hi'], recs[n, k]['sum_lo'],
                                                                                                  recs[n, k]['count'])
            assert np.array_equal(info['approx'][n][k], ap), (n, k)
            assert info['n_approx'][n, k] == len(ap) and info['paths'][n, k] == paths and info['sside'][n, k] == sside, (n, k)
            assert near == 0
            if poly is not None:
                want_p.append(poly)
                want_s.append(s64[n, k])
        assert len(polys) == len(want_p) and scores == want_s
        for a, b in zip(polys, want_p):
            assert a.dtype == np.int64 and np.array_equal(a, b)
        kept += len(polys)
    assert kept >= 25  # the fixtures exercise unclip and scaling, not only the skips
    assert (info['paths'] > 0).sum() > kept - 1


def test_polygon_output_stays_on_its_own_entry():
    with pytest.raises(NotImplementedError, match='polygons'):
        P.SegDetectorRepresenter()(None, None, is_output_polygon=True)
    assert callable(P.SegDetectorRepresenter().polygons)
