"""Independent models for the detection scoring of csrc/det_eval.hip, all in exact arithmetic.

  overlap_exact(A, B)     the exact overlap oracle: vertical slab integration in fractions.Fraction.  Events are every
                          vertex x and every x where two edges (of A, of B, or one of each) meet; inside a slab the
                          integral of w_A * w_B over y is linear in x, so its value at the slab's midpoint times the slab's
                          width is exact.  Works for non-simple polygons, so it pins the winding-weighted definition.
  overlap_boundary(A, B)  a restatement of the device's boundary formula with its symbolic perturbation, in Fractions
                          (equal to the oracle exactly, not approximately)
  is_simple(P)            the non-simple flag's definition, exact
  iou_image / deteval_image / combine_iou / combine_deteval
                          restatements of the two matching protocols on given overlap matrices and areas

Polygons are sequences of (x, y) numbers (int or float); every float is taken at its exact binary value.
"""
import math
from fractions import Fraction

import numpy as np


def fr(P):
    return [(Fraction(x), Fraction(y)) for x, y in np.asarray(P, dtype=object).reshape(-1, 2).tolist()]


def _sgn(v):
    return (v > 0) - (v < 0)


def _cross(ox, oy, ax, ay, bx, by):
    return (ax - ox) * (by - oy) - (ay - oy) * (bx - ox)


def signed_area2(P):
    """twice the shoelace signed area, exact"""
    P = fr(P)
    n = len(P)
    return sum(P[i][0] * P[(i + 1) % n][1] - P[i][1] * P[(i + 1) % n][0] for i in range(n))


def area_exact(P):
    return abs(signed_area2(P)) / 2


def orientation(P):
    """+1 when the shoelace signed area is >= 0, else -1 (the device orients every polygon this way)"""
    return 1 if signed_area2(P) >= 0 else -1


def _edges(P):
    n = len(P)
    return [(P[i], P[(i + 1) % n]) for i in range(n) if P[i] != P[(i + 1) % n]]


def _meet_x(e, f):
    """x of the point where closed segments e and f meet, when they meet in one point (parallel pairs: None; their
    shared points are vertices, which are events already)"""
    (px, py), (qx, qy) = e
    (rx, ry), (sx, sy) = f
    den = (qx - px) * (sy - ry) - (qy - py) * (sx - rx)
    if den == 0:
        return None
    t = ((rx - px) * (sy - ry) - (ry - py) * (sx - rx)) / den
    u = ((rx - px) * (qy - py) - (ry - py) * (qx - px)) / den
    if 0 <= t <= 1 and 0 <= u <= 1:
        return px + t * (qx - px)
    return None


def overlap_exact(A, B):
    """integral of w_A * w_B over the plane, each polygon oriented to a signed area >= 0: a Fraction"""
    A, B = fr(A), fr(B)
    ea = [(e, 0, orientation(A)) for e in _edges(A)]
    eb = [(e, 1, orientation(B)) for e in _edges(B)]
    if not ea or not eb:
        return Fraction(0)
    ax0, ax1 = min(x for x, _ in A), max(x for x, _ in A)
    bx0, bx1 = min(x for x, _ in B), max(x for x, _ in B)
    lo, hi = max(ax0, bx0), min(ax1, bx1)
    if lo >= hi:
        return Fraction(0)
    xs = {x for x, _ in A + B if lo <= x <= hi} | {lo, hi}
    alle = ea + eb
    for i in range(len(alle)):
        for j in range(i + 1, len(alle)):
            x = _meet_x(alle[i][0], alle[j][0])
            if x is not None and lo <= x <= hi:
                xs.add(x)
    xs = sorted(xs)
    total = Fraction(0)
    for x0, x1 in zip(xs, xs[1:]):
        xm = (x0 + x1) / 2
        cuts = []
        for ((px, py), (qx, qy)), k, o in alle:
            if min(px, qx) < xm < max(px, qx):
                y = py + (xm - px) * (qy - py) / (qx - px)
                cuts.append((y, k, o if qx > px else -o))  # an edge towards +x raises the winding number above it
        cuts.sort(key=lambda c: c[0])
        w = [0, 0]
        prev = None
        col = Fraction(0)
        for y, k, d in cuts:
            if prev is not None and w[0] and w[1]:
                col += w[0] * w[1] * (y - prev)
            w[k] += d
            prev = y
        total += col * (x1 - x0)
    return total


# ---- the device formula, restated ----------------------------------------------------------------------------------------

def _orient_pert(u1, u2, v, sg):
    """sign of orient(u1, u2, v + sg (eps, eps^2)), eps -> 0+"""
    d0 = _cross(u1[0], u1[1], u2[0], u2[1], v[0], v[1])
    if d0:
        return _sgn(d0)
    if u2[1] != u1[1]:
        return -sg if u2[1] > u1[1] else sg
    return sg if u2[0] > u1[0] else -sg


def _boundary_part(E, F, sg, o):
    """sum over the edges e of E of 2 * int_e w_F (x dy - y dx)/2, E translated by sg (eps, eps^2) relative to F"""
    total = Fraction(0)
    n = len(E)
    for i in range(n):
        p, q = E[i], E[(i + 1) % n]
        if p == q:
            continue
        w = 0
        acc = Fraction(0)
        for b1, b2 in _edges(F):
            below1 = b1[1] <= p[1] if sg > 0 else b1[1] < p[1]
            below2 = b2[1] <= p[1] if sg > 0 else b2[1] < p[1]
            op = _orient_pert(b1, b2, p, sg)
            if below1 != below2:
                if b2[1] > b1[1] and op > 0:
                    w += 1
                elif b2[1] < b1[1] and op < 0:
                    w -= 1
            if op == _orient_pert(b1, b2, q, sg):
                continue
            if _orient_pert(p, q, b1, -sg) == _orient_pert(p, q, b2, -sg):
                continue
            dp = _cross(b1[0], b1[1], b2[0], b2[1], p[0], p[1])
            dq = _cross(b1[0], b1[1], b2[0], b2[1], q[0], q[1])
            t = dp / (dp - dq)
            X = (p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1]))
            c = _cross(o[0], o[1], X[0], X[1], q[0], q[1])
            acc += c if op < 0 else -c
        total += w * _cross(o[0], o[1], p[0], p[1], q[0], q[1]) + acc
    return total


def overlap_boundary(A, B):
    """Green's theorem on both boundaries, A translated by (eps, eps^2): a Fraction"""
    A, B = fr(A), fr(B)
    o = A[0]
    s = _boundary_part(A, B, 1, o) + _boundary_part(B, A, -1, o)
    return orientation(A) * orientation(B) * s / 2


def is_simple(P):
    """False when two non-adjacent non-zero edges touch or cross, two adjacent ones overlap collinearly, or there are
    fewer than 3 non-zero edges (zero-length edges are skipped; adjacency is between consecutive non-zero edges)"""
    P = fr(P)
    n = len(P)
    nd = [i for i in range(n) if P[i] != P[(i + 1) % n]]
    if len(nd) < 3:
        return False
    nxt = {nd[k]: nd[(k + 1) % len(nd)] for k in range(len(nd))}

    def fold(a, m, b):
        if _cross(a[0], a[1], m[0], m[1], b[0], b[1]):
            return False
        return _sgn(a[0] - m[0]) == _sgn(b[0] - m[0]) and _sgn(a[1] - m[1]) == _sgn(b[1] - m[1])

    def on_seg(a, b, c):
        return min(a[0], b[0]) <= c[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= c[1] <= max(a[1], b[1])

    for ii, e in enumerate(nd):
        p1, q1 = P[e], P[(e + 1) % n]
        for f in nd[ii + 1:]:
            p2, q2 = P[f], P[(f + 1) % n]
            if f == nxt[e] or e == nxt[f]:
                if f == nxt[e] and fold(p1, q1, q2):
                    return False
                if e == nxt[f] and fold(p2, q2, q1):
                    return False
                continue
            o1, o2 = _sgn(_cross(*p1, *q1, *p2)), _sgn(_cross(*p1, *q1, *q2))
            o3, o4 = _sgn(_cross(*p2, *q2, *p1)), _sgn(_cross(*p2, *q2, *q1))
            if o1 * o2 < 0 and o3 * o4 < 0:
                return False
            if (o1 == 0 and on_seg(p1, q1, p2)) or (o2 == 0 and on_seg(p1, q1, q2)) or (o3 == 0 and on_seg(p2, q2, p1)) or \
                    (o4 == 0 and on_seg(p2, q2, q1)):
                return False
    return True


# ---- matching protocols, restated on given matrices ---------------------------------------------------------------------

IOU_DEFAULTS = dict(iou_constraint=0.5, area_precision_constraint=0.5)
DETEVAL_DEFAULTS = dict(area_recall_constraint=0.8, area_precision_constraint=0.4, ev_param_ind_center_diff_thr=1, mtype_oo_o=1.0,
                        mtype_om_o=0.8, mtype_om_m=1.0)


def _dont_care(inter, ga, da, ignore, area_c):
    gdc = [g for g in range(len(ga)) if ignore[g]]
    ddc = []
    for d in range(len(da)):
        for g in gdc:
            if (0 if da[d] == 0 else inter[g][d] / da[d]) > area_c:
                ddc.append(d)
                break
    return gdc, ddc


def iou_image(inter, ga, da, ignore, iou_constraint=0.5, area_precision_constraint=0.5):
    """iou.py's decisions on fp64 overlaps inter[g][d] and areas: dict of the counts, pairs and don't-care lists"""
    G, D = len(ga), len(da)
    gdc, ddc = _dont_care(inter, ga, da, ignore, area_precision_constraint)
    gm, dm = [0] * G, [0] * D
    pairs = []
    for g in range(G):
        for d in range(D):
            if gm[g] or dm[d] or g in gdc or d in ddc:
                continue
            if inter[g][d] / ((ga[g] + da[d]) - inter[g][d]) > iou_constraint:
                gm[g] = dm[d] = 1
                pairs.append({'gt': g, 'det': d})
    gc, dc = G - len(gdc), D - len(ddc)
    if gc == 0:
        r, p = 1.0, (0.0 if dc > 0 else 1.0)
    else:
        r, p = len(pairs) / gc, (0 if dc == 0 else len(pairs) / dc)
    h = 0 if p + r == 0 else 2.0 * p * r / (p + r)
    return dict(precision=p, recall=r, hmean=h, pairs=pairs, gtCare=gc, detCare=dc, gtDontCare=gdc, detDontCare=ddc, detMatched=len(pairs))


def deteval_image(inter, ga, da, ignore, gt_cd, det_cd, area_recall_constraint=0.8, area_precision_constraint=0.4,
                  ev_param_ind_center_diff_thr=1, mtype_oo_o=1.0, mtype_om_o=0.8, mtype_om_m=1.0):
    """deteval.py's decisions; gt_cd / det_cd: per polygon (mean x, mean y, bbox diagonal)"""
    tr, tp = area_recall_constraint, area_precision_constraint
    G, D = len(ga), len(da)
    gdc, ddc = _dont_care(inter, ga, da, ignore, tp)
    p, r, h, racc, pacc = 0, 0, 0, 0.0, 0.0
    if G == 0:
        r, p = 1, (0 if D > 0 else 1)
    pairs = []
    if D > 0:
        R = [[0 if ga[g] == 0 else inter[g][d] / ga[g] for d in range(D)] for g in range(G)]
        Pm = [[0 if da[d] == 0 else inter[g][d] / da[d] for d in range(D)] for g in range(G)]
        gm, dm = [0] * G, [0] * D

        def q(g, d):
            return R[g][d] >= tr and Pm[g][d] >= tp

        def ov_g(g):
            return sum(1 for d in range(D) if d not in ddc and R[g][d] > 0)

        def ov_d(d):
            return sum(1 for g in range(G) if g not in gdc and R[g][d] > 0)

        for g in range(G):
            for d in range(D):
                if gm[g] or dm[d] or g in gdc or d in ddc:
                    continue
                if sum(q(g, j) for j in range(D)) != 1 or sum(q(i, d) for i in range(G)) != 1 or not q(g, d):
                    continue
                if ov_g(g) != 1 or ov_d(d) != 1:
                    continue
                dx, dy = gt_cd[g][0] - det_cd[d][0], gt_cd[g][1] - det_cd[d][1]
                nd = math.pow(dx * dx + dy * dy, 0.5)
                nd /= gt_cd[g][2] + det_cd[d][2]
                nd *= 2.0
                if nd < ev_param_ind_center_diff_thr:
                    gm[g] = dm[d] = 1
                    racc += mtype_oo_o
                    pacc += mtype_oo_o
                    pairs.append({'gt': g, 'det': d, 'type': 'OO'})
        for g in range(G):
            if g in gdc:
                continue
            s, lst = 0, []
            for d in range(D):
                if not gm[g] and not dm[d] and d not in ddc and Pm[g][d] >= tp:
                    s += R[g][d]
                    lst.append(d)
            if round(s, 4) >= tr and ov_g(g) >= 2:
                gm[g] = 1
                racc += mtype_oo_o if len(lst) == 1 else mtype_om_o
                pacc += mtype_oo_o if len(lst) == 1 else mtype_om_o * len(lst)
                pairs.append({'gt': g, 'det': lst, 'type': 'OO' if len(lst) == 1 else 'OM'})
                for d in lst:
                    dm[d] = 1
        for d in range(D):
            if d in ddc:
                continue
            s, lst = 0, []
            for g in range(G):
                if not gm[g] and not dm[d] and g not in gdc and R[g][d] >= tr:
                    s += Pm[g][d]
                    lst.append(g)
            if round(s, 4) >= tp and ov_d(d) >= 2:
                dm[d] = 1
                racc += mtype_oo_o if len(lst) == 1 else mtype_om_m * len(lst)
                pacc += mtype_oo_o if len(lst) == 1 else mtype_om_m
                pairs.append({'gt': lst, 'det': d, 'type': 'OO' if len(lst) == 1 else 'MO'})
                for g in lst:
                    gm[g] = 1
        gc = G - len(gdc)
        if gc == 0:
            r, p = 1.0, 0.0
        else:
            r = racc / gc
            p = 0.0 if D - len(ddc) == 0 else pacc / (D - len(ddc))
        h = 0 if p + r == 0 else 2.0 * p * r / (p + r)
    return dict(precision=p, recall=r, hmean=h, pairs=pairs, gtCare=G - len(gdc), detCare=D - len(ddc), gtDontCare=gdc, detDontCare=ddc,
                recallAccum=racc, precisionAccum=pacc)


def centre_diag(P):
    """(mean x, mean y, bbox diagonal) as deteval.py's center_distance / diag compute them (numpy, fp64)"""
    m = np.mean(P, axis=0)
    r = np.array(P)
    dg = ((r[:, 0].max() - r[:, 0].min())**2 + (r[:, 1].max() - r[:, 1].min())**2)**0.5
    return float(m[0]), float(m[1]), float(dg)


def combine(results, deteval=False):
    gc = sum(r['gtCare'] for r in results)
    dc = sum(r['detCare'] for r in results)
    if deteval:
        rs, ps = 0, 0
        for r in results:
            rs += r['recallAccum']
            ps += r['precisionAccum']
    else:
        rs = ps = sum(r['detMatched'] for r in results)
    R = 0 if gc == 0 else float(rs) / gc
    P = 0 if dc == 0 else float(ps) / dc
    H = 0 if R + P == 0 else 2 * R * P / (R + P)
    return {'precision': P, 'recall': R, 'hmean': H}
