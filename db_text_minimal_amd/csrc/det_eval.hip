// Text-detection scoring: the polygon overlap matrices of the reference's evaluators (src/iou.py,
// src/deteval.py, through shapely) on the device, and their matching protocols on the host.
//
// Definition.  Each polygon is oriented so that its shoelace signed area is >= 0; area(P) = |signed area|;
// overlap(A, B) = the integral of w_A * w_B over the plane, w the winding number.  For simple polygons of either orientation
// that is exactly area(A n B); for a non-simple polygon it is a winding-weighted overlap (flagged, see nonsimple below).
//
// Device, two launches:
//   poly_kernel     one workgroup per polygon: shoelace signed area (origin at vertex 0, fixed-order tree sum), bounding
//                   box, orientation sign, and the non-simple flag (two non-adjacent edges touch or cross, or two adjacent
//                   edges overlap collinearly; zero-length edges are skipped; fewer than three non-zero edges is non-simple).
//   overlap_kernel  one wavefront per (image, gt, det) pair: 0 when the bounding boxes are disjoint or touch, else Green's
//                   theorem on both boundaries,
//                       overlap = sum_{e in dA} int_e w_B (x dy - y dx)/2 + sum_{f in dB} int_f w_A (x dy - y dx)/2,
//                   and along an edge p -> q the integral is w(p) cross(p - o, q - o)/2 + sum_i s_i cross(X_i - o, q - o)/2
//                   over its crossings X_i with the other boundary (s_i = +1 entering from the right of the crossed edge).
//                   One pass over the other polygon's edges per edge; no sort.  Lanes take the edges of one polygon, the
//                   other is staged in LDS in chunks of DE_CHUNK vertices (any vertex count), then the roles swap.
//
// Degeneracies (shared edges, a vertex on an edge, identical polygons, T-junctions) are resolved by symbolic perturbation:
// A is translated by (eps, eps^2), eps -> 0+.  The overlap is continuous under translation, so its value is unchanged, and
// no A vertex lies on a B edge line or the other way round.  Every predicate is exact in sign for any fp64 input: side of
// line through an error-bounded determinant with an exact expansion fallback; when the determinant is exactly 0 the sign
// comes from the eps terms, signs of coordinate differences, which fp64 comparisons give exactly.  Only the crossing points
// X_i and the sums are rounded; X_i is a vertex when a determinant is exactly 0 and keeps the exact coordinate of an axis-
// parallel edge, so axis-aligned integer inputs (|coordinates| < 2^25) give exact overlaps.  Sums run in a fixed order and
// the wave reduction is a fixed butterfly: results are bitwise reproducible whatever the workspace held.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "common.h"

namespace {

constexpr int DE_CHUNK = 256;  // vertices of the staged polygon per LDS chunk (4 KB)

struct P2 {
    double x, y;
};

__device__ __forceinline__ void two_sum(double a, double b, double& s, double& e) {
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}

__device__ __forceinline__ void two_prod(double a, double b, double& p, double& e) {
    p = a * b;
    e = fma(a, b, -p);
}

// exact sign of (ax - cx)(by - cy) - (ay - cy)(bx - cx) = ax by - ax cy - by cx - ay bx + ay cx + bx cy: six products, each
// exactly two doubles, summed by Grow-Expansion (Shewchuk 1997, Theorem 10); the last non-zero component carries the sign
__device__ __noinline__ int orient_exact(double ax, double ay, double bx, double by, double cx, double cy) {
    double t[12];
    two_prod(ax, by, t[1], t[0]);
    two_prod(-ax, cy, t[3], t[2]);
    two_prod(-by, cx, t[5], t[4]);
    two_prod(-ay, bx, t[7], t[6]);
    two_prod(ay, cx, t[9], t[8]);
    two_prod(bx, cy, t[11], t[10]);
    double h[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        double q = t[k];
#pragma unroll
        for (int i = 0; i < k; ++i) {
            double s, e;
            two_sum(q, h[i], s, e);
            h[i] = e;
            q = s;
        }
        h[k] = q;
    }
    int sign = 0;
#pragma unroll
    for (int k = 0; k < 12; ++k)
        if (h[k] != 0.0) sign = h[k] > 0.0 ? 1 : -1;
    return sign;
}

// sign of orient(a, b, c) = cross(b - a, c - a): the fp64 determinant when its error bound (Shewchuk's ccwerrboundA, no
// fused multiply-add: -ffp-contract=off) separates it from 0, else exact
__device__ __forceinline__ int orient_sign(P2 a, P2 b, P2 c) {
    constexpr double eps = 0x1p-53;
    constexpr double bound_a = (3.0 + 16.0 * eps) * eps;
    const double dl = (a.x - c.x) * (b.y - c.y), dr = (a.y - c.y) * (b.x - c.x);
    const double det = dl - dr, bound = bound_a * (fabs(dl) + fabs(dr));
    if (det > bound) return 1;
    if (-det > bound) return -1;
    return orient_exact(a.x, a.y, b.x, b.y, c.x, c.y);
}

// sign of orient(u1, u2, v + sg (eps, eps^2)), u1 != u2: D0 + sg (dx eps^2 - dy eps), never 0
__device__ __forceinline__ int orient_pert(P2 u1, P2 u2, P2 v, int sg) {
    const int s = orient_sign(u1, u2, v);
    if (s) return s;
    if (u2.y != u1.y) return u2.y > u1.y ? -sg : sg;
    return u2.x > u1.x ? sg : -sg;
}

// the crossing point of segments p q and b1 b2 (known to cross under the perturbation), from the unperturbed lines
__device__ __forceinline__ P2 cross_point(P2 p, P2 q, P2 b1, P2 b2) {
    const double fx = b2.x - b1.x, fy = b2.y - b1.y;
    const double dp = fx * (p.y - b1.y) - fy * (p.x - b1.x), dq = fx * (q.y - b1.y) - fy * (q.x - b1.x);
    if (dp == 0.0) return p;
    if (dq == 0.0) return q;
    const double ex = q.x - p.x, ey = q.y - p.y;
    if (ex * (b1.y - p.y) - ey * (b1.x - p.x) == 0.0) return b1;
    if (ex * (b2.y - p.y) - ey * (b2.x - p.x) == 0.0) return b2;
    const double t = fmin(fmax(dp / (dp - dq), 0.0), 1.0);  // (NaN -> 0)
    P2 X;
    X.x = ex == 0.0 ? p.x : (fx == 0.0 ? b1.x : p.x + t * ex);
    X.y = ey == 0.0 ? p.y : (fy == 0.0 ? b1.y : p.y + t * ey);
    return X;
}

// this lane's share of sum over edges e of E of int_e w_F (x dy - y dx), E translated by sg (eps, eps^2) relative to F
// (twice the boundary term).  Every lane of the (one-wave) workgroup must call it: it stages F through lds.
__device__ double boundary_part(const P2* __restrict__ E, int VE, const P2* __restrict__ F, int VF, int sg, P2 o, P2* lds, int lane) {
    double sum = 0.0;
    for (int e0 = 0; e0 < VE; e0 += 64) {
        const int e = e0 + lane;
        P2 p{0.0, 0.0}, q{0.0, 0.0};
        if (e < VE) {
            p = E[e];
            q = E[e + 1 == VE ? 0 : e + 1];
        }
        const bool live = e < VE && (p.x != q.x || p.y != q.y);
        const double exlo = fmin(p.x, q.x), exhi = fmax(p.x, q.x), eylo = fmin(p.y, q.y), eyhi = fmax(p.y, q.y);
        int w = 0;
        double acc = 0.0;
        for (int c0 = 0; c0 < VF; c0 += DE_CHUNK) {
            const int nc = min(DE_CHUNK, VF - c0);
            __syncthreads();
            for (int j = lane; j <= nc; j += 64) {
                int k = c0 + j;
                if (k >= VF) k -= VF;
                lds[j] = F[k];
            }
            __syncthreads();
            if (!live) continue;
            for (int j = 0; j < nc; ++j) {
                const P2 b1 = lds[j], b2 = lds[j + 1];
                if (b1.x == b2.x && b1.y == b2.y) continue;
                const double bxlo = fmin(b1.x, b2.x), bxhi = fmax(b1.x, b2.x);
                int op = 0;
                // w_F(p'): signed crossings of the ray from p' = p + sg (eps, eps^2) towards +x (p'.y is never a vertex y)
                const bool s1 = sg > 0 ? b1.y <= p.y : b1.y < p.y, s2 = sg > 0 ? b2.y <= p.y : b2.y < p.y;
                if (s1 != s2) {
                    bool right;
                    if (bxlo > p.x) {
                        right = true;
                    } else if (bxhi < p.x) {
                        right = false;
                    } else {
                        op = orient_pert(b1, b2, p, sg);
                        right = b2.y > b1.y ? op > 0 : op < 0;
                    }
                    if (right) w += b2.y > b1.y ? 1 : -1;
                }
                // crossing of e' with f (strictly separated boxes cannot cross under the perturbation)
                if (bxhi < exlo || bxlo > exhi || fmax(b1.y, b2.y) < eylo || fmin(b1.y, b2.y) > eyhi) continue;
                if (op == 0) op = orient_pert(b1, b2, p, sg);
                if (op == orient_pert(b1, b2, q, sg)) continue;
                if (orient_pert(p, q, b1, -sg) == orient_pert(p, q, b2, -sg)) continue;
                const P2 X = cross_point(p, q, b1, b2);
                const double c = (X.x - o.x) * (q.y - o.y) - (X.y - o.y) * (q.x - o.x);
                acc += op < 0 ? c : -c;  // from the right of f to its left: w_F rises by one
            }
        }
        if (live) sum += (double)w * ((p.x - o.x) * (q.y - o.y) - (p.y - o.y) * (q.x - o.x)) + acc;
    }
    return sum;
}

// meta per polygon: xmin, ymin, xmax, ymax, orientation sign (+1 / -1), 0
__global__ __launch_bounds__(256) void poly_kernel(const P2* __restrict__ verts, const int* __restrict__ poff, double* __restrict__ meta,
                                                   double* __restrict__ area, int* __restrict__ nonsimple) {
    __shared__ double red[5][256];
    __shared__ int nz, flag;
    const int i = blockIdx.x, tid = threadIdx.x;
    const P2* v = verts + poff[i];
    const int V = poff[i + 1] - poff[i];
    if (tid == 0) nz = 0, flag = 0;
    __syncthreads();
    const P2 o = v[0];
    double s = 0.0, x0 = INFINITY, y0 = INFINITY, x1 = -INFINITY, y1 = -INFINITY;
    int cnt = 0;
    for (int k = tid; k < V; k += 256) {
        const P2 a = v[k], b = v[k + 1 == V ? 0 : k + 1];
        s += (a.x - o.x) * (b.y - o.y) - (a.y - o.y) * (b.x - o.x);
        x0 = fmin(x0, a.x), y0 = fmin(y0, a.y), x1 = fmax(x1, a.x), y1 = fmax(y1, a.y);
        cnt += (a.x != b.x || a.y != b.y);
    }
    red[0][tid] = s, red[1][tid] = x0, red[2][tid] = y0, red[3][tid] = x1, red[4][tid] = y1;
    if (cnt) atomicAdd(&nz, cnt);
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) {
            red[0][tid] += red[0][tid + st];
            red[1][tid] = fmin(red[1][tid], red[1][tid + st]);
            red[2][tid] = fmin(red[2][tid], red[2][tid + st]);
            red[3][tid] = fmax(red[3][tid], red[3][tid + st]);
            red[4][tid] = fmax(red[4][tid], red[4][tid + st]);
        }
        __syncthreads();
    }
    // non-simple: every pair of non-zero edges e < f
    auto nondeg = [&](int k) {
        const P2 a = v[k], b = v[k + 1 == V ? 0 : k + 1];
        return a.x != b.x || a.y != b.y;
    };
    auto next_nd = [&](int k) {
        int j = k + 1 == V ? 0 : k + 1;
        while (j != k && !nondeg(j)) j = j + 1 == V ? 0 : j + 1;
        return j;
    };
    // adjacent edges a -> m and m -> b overlap iff a, m, b are collinear and a, b lie on the same side of m
    auto fold = [](P2 a, P2 m, P2 b) {
        if (orient_sign(a, m, b) != 0) return false;
        const int sax = (a.x > m.x) - (a.x < m.x), sbx = (b.x > m.x) - (b.x < m.x);
        const int say = (a.y > m.y) - (a.y < m.y), sby = (b.y > m.y) - (b.y < m.y);
        return sax == sbx && say == sby;
    };
    auto on_seg = [](P2 a, P2 b, P2 c) {  // c collinear with a b: within its box
        return fmin(a.x, b.x) <= c.x && c.x <= fmax(a.x, b.x) && fmin(a.y, b.y) <= c.y && c.y <= fmax(a.y, b.y);
    };
    if (nz >= 3) {
        for (int e = tid; e < V && !*(volatile int*)&flag; e += 256) {
            if (!nondeg(e)) continue;
            const P2 p1 = v[e], q1 = v[e + 1 == V ? 0 : e + 1];
            const int ne = next_nd(e);
            bool hit = false;
            for (int f = e + 1; f < V && !hit; ++f) {
                if (!nondeg(f)) continue;
                const P2 p2 = v[f], q2 = v[f + 1 == V ? 0 : f + 1];
                const int nf = next_nd(f);
                if (f == ne || e == nf) {
                    if (f == ne && fold(p1, q1, q2)) hit = true;
                    if (e == nf && fold(p2, q2, q1)) hit = true;
                    continue;
                }
                if (fmax(p1.x, q1.x) < fmin(p2.x, q2.x) || fmax(p2.x, q2.x) < fmin(p1.x, q1.x) || fmax(p1.y, q1.y) < fmin(p2.y, q2.y) ||
                    fmax(p2.y, q2.y) < fmin(p1.y, q1.y))
                    continue;
                const int o1 = orient_sign(p1, q1, p2), o2 = orient_sign(p1, q1, q2);
                const int o3 = orient_sign(p2, q2, p1), o4 = orient_sign(p2, q2, q1);
                if (o1 * o2 < 0 && o3 * o4 < 0) hit = true;
                else if ((o1 == 0 && on_seg(p1, q1, p2)) || (o2 == 0 && on_seg(p1, q1, q2)) || (o3 == 0 && on_seg(p2, q2, p1)) ||
                         (o4 == 0 && on_seg(p2, q2, q1)))
                    hit = true;
            }
            if (hit) atomicOr(&flag, 1);
        }
    }
    __syncthreads();
    if (tid == 0) {
        double* m = meta + 6L * i;
        m[0] = red[1][0], m[1] = red[2][0], m[2] = red[3][0], m[3] = red[4][0];
        m[4] = red[0][0] >= 0.0 ? 1.0 : -1.0;
        m[5] = 0.0;
        area[i] = 0.5 * fabs(red[0][0]);
        nonsimple[i] = (nz < 3 || flag) ? 1 : 0;
    }
}

// img[n] = {gt begin, G, det begin, D, pair offset}: polygons are numbered over the batch
__global__ __launch_bounds__(64) void overlap_kernel(const P2* __restrict__ verts, const int* __restrict__ poff,
                                                     const long long* __restrict__ img, int N, long n_pairs, const double* __restrict__ meta,
                                                     int cull, double* __restrict__ inter) {
    __shared__ P2 lds[DE_CHUNK + 1];
    const int lane = threadIdx.x;
    for (long w = blockIdx.x; w < n_pairs; w += gridDim.x) {
        int lo = 0, hi = N - 1;  // the last image whose pair offset is <= w
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (img[5L * mid + 4] <= w) lo = mid;
            else hi = mid - 1;
        }
        const long long* im = img + 5L * lo;
        const long local = w - im[4];
        const int D = (int)im[3];
        const int a = (int)(im[0] + local / D), b = (int)(im[2] + local % D);
        const double* ma = meta + 6L * a;
        const double* mb = meta + 6L * b;
        double r = 0.0;
        if (!cull || !(ma[2] <= mb[0] || mb[2] <= ma[0] || ma[3] <= mb[1] || mb[3] <= ma[1])) {
            const P2* A = verts + poff[a];
            const P2* B = verts + poff[b];
            const int VA = poff[a + 1] - poff[a], VB = poff[b + 1] - poff[b];
            const P2 o = A[0];
            double s = boundary_part(A, VA, B, VB, 1, o, lds, lane) + boundary_part(B, VB, A, VA, -1, o, lds, lane);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
            r = 0.5 * s * ma[4] * mb[4] + 0.0;  // (+0.0: no negative zero)
        }
        if (lane == 0) inter[w] = r;
        __syncthreads();
    }
}

// ---- host matching ----------------------------------------------------------------------------------------------------------

// Python's round(x, 4): correctly rounded to 4 decimals (ties to even on the exact binary value), then back to the nearest double
double py_round4(double x) {
    char buf[512];
    snprintf(buf, sizeof buf, "%.4f", x);
    return strtod(buf, nullptr);
}

struct Img {
    int G, D;
    const double *I, *ga, *da;
    const unsigned char* ig;
    const double *gcd, *dcd;
    double* stats;
    unsigned char* ddc;
    int* rows;
    int cap, n_rows;
};

bool emit(Img& m, int pair, int kind, int g, int d) {
    if (m.n_rows >= m.cap) return false;
    int* r = m.rows + 4L * m.n_rows++;
    r[0] = pair, r[1] = kind, r[2] = g, r[3] = d;
    return true;
}

// dets that a don't-care GT covers: the first ignored GT with inter / area_det > area_precision_constraint
int dont_care(Img& m, double area_c, std::vector<char>& gdc) {
    int ngdc = 0;
    for (int g = 0; g < m.G; ++g) ngdc += (gdc[g] = m.ig[g] ? 1 : 0);
    for (int d = 0; d < m.D; ++d) {
        m.ddc[d] = 0;
        if (!ngdc) continue;
        for (int g = 0; g < m.G; ++g) {
            if (!gdc[g]) continue;
            const double prec = m.da[d] == 0.0 ? 0.0 : m.I[(long)g * m.D + d] / m.da[d];
            if (prec > area_c) {
                m.ddc[d] = 1;
                break;
            }
        }
    }
    return ngdc;
}

bool match_iou(Img& m, const double* prm) {
    const double iou_c = prm[0], area_c = prm[1];
    const int G = m.G, D = m.D;
    std::vector<char> gdc(G), gm(G, 0), dm(D, 0);
    const int ngdc = dont_care(m, area_c, gdc);
    int ndd = 0;
    for (int d = 0; d < D; ++d) ndd += m.ddc[d];
    int matched = 0;
    for (int g = 0; g < G; ++g)
        for (int d = 0; d < D; ++d) {
            if (gm[g] || dm[d] || gdc[g] || m.ddc[d]) continue;
            const double in = m.I[(long)g * D + d];
            if (in / ((m.ga[g] + m.da[d]) - in) > iou_c) {
                gm[g] = dm[d] = 1;
                if (!emit(m, matched, 0, g, d)) return false;
                ++matched;
            }
        }
    const int gcare = G - ngdc, dcare = D - ndd;
    double recall, precision;
    if (gcare == 0) {
        recall = 1.0;
        precision = dcare > 0 ? 0.0 : 1.0;
    } else {
        recall = (double)matched / gcare;
        precision = dcare == 0 ? 0.0 : (double)matched / dcare;
    }
    const double hmean = precision + recall == 0.0 ? 0.0 : 2.0 * precision * recall / (precision + recall);
    double* s = m.stats;
    s[0] = precision, s[1] = recall, s[2] = hmean, s[3] = gcare, s[4] = dcare, s[5] = matched, s[6] = 0.0, s[7] = 0.0;
    return true;
}

// prm = {area_recall_constraint, area_precision_constraint, ev_param_ind_center_diff_thr, mtype_oo_o, mtype_om_o, mtype_om_m}
bool match_deteval(Img& m, const double* prm) {
    const double tr = prm[0], tp = prm[1], center_thr = prm[2], oo = prm[3], om_o = prm[4], om_m = prm[5];
    const int G = m.G, D = m.D;
    std::vector<char> gdc(G), gm(G, 0), dm(D, 0);
    const int ngdc = dont_care(m, tp, gdc);
    int ndd = 0;
    for (int d = 0; d < D; ++d) ndd += m.ddc[d];
    double recall = 0.0, precision = 0.0, hmean = 0.0, racc = 0.0, pacc = 0.0;
    if (G == 0) {
        recall = 1.0;
        precision = D > 0 ? 0.0 : 1.0;
    }
    int npairs = 0;
    if (D > 0) {
        std::vector<double> R((size_t)G * D), P((size_t)G * D);
        for (int g = 0; g < G; ++g)
            for (int d = 0; d < D; ++d) {
                const double in = m.I[(long)g * D + d];
                R[(size_t)g * D + d] = m.ga[g] == 0.0 ? 0.0 : in / m.ga[g];
                P[(size_t)g * D + d] = m.da[d] == 0.0 ? 0.0 : in / m.da[d];
            }
        auto qual = [&](int g, int d) { return R[(size_t)g * D + d] >= tr && P[(size_t)g * D + d] >= tp; };
        auto overlaps_gt = [&](int g) {
            int c = 0;
            for (int d = 0; d < D; ++d) c += !m.ddc[d] && R[(size_t)g * D + d] > 0.0;
            return c;
        };
        auto overlaps_det = [&](int d) {
            int c = 0;
            for (int g = 0; g < G; ++g) c += !gdc[g] && R[(size_t)g * D + d] > 0.0;
            return c;
        };
        // one-to-one
        for (int g = 0; g < G; ++g)
            for (int d = 0; d < D; ++d) {
                if (gm[g] || dm[d] || gdc[g] || m.ddc[d]) continue;
                int c = 0;
                for (int j = 0; j < D; ++j) c += qual(g, j);
                if (c != 1) continue;
                c = 0;
                for (int i = 0; i < G; ++i) c += qual(i, d);
                if (c != 1 || !qual(g, d)) continue;
                if (overlaps_gt(g) != 1 || overlaps_det(d) != 1) continue;
                const double* cg = m.gcd + 3L * g;
                const double* cd = m.dcd + 3L * d;
                const double dx = cg[0] - cd[0], dy = cg[1] - cd[1];
                double nd = pow(dx * dx + dy * dy, 0.5);
                nd /= cg[2] + cd[2];
                nd *= 2.0;
                if (nd < center_thr) {
                    gm[g] = dm[d] = 1;
                    racc += oo;
                    pacc += oo;
                    if (!emit(m, npairs++, 0, g, d)) return false;
                }
            }
        // one-to-many
        std::vector<int> list;
        for (int g = 0; g < G; ++g) {
            if (gdc[g]) continue;
            double sum = 0.0;
            list.clear();
            for (int d = 0; d < D; ++d)
                if (!gm[g] && !dm[d] && !m.ddc[d] && P[(size_t)g * D + d] >= tp) {
                    sum += R[(size_t)g * D + d];
                    list.push_back(d);
                }
            if (!(py_round4(sum) >= tr)) continue;
            if (overlaps_gt(g) < 2) continue;
            const int k = (int)list.size();
            gm[g] = 1;
            racc += k == 1 ? oo : om_o;
            pacc += k == 1 ? oo : om_o * k;
            if (k == 0 && !emit(m, npairs, 1, g, -1)) return false;
            for (int d : list) {
                if (!emit(m, npairs, 1, g, d)) return false;
                dm[d] = 1;
            }
            ++npairs;
        }
        // many-to-one
        for (int d = 0; d < D; ++d) {
            if (m.ddc[d]) continue;
            double sum = 0.0;
            list.clear();
            for (int g = 0; g < G; ++g)
                if (!gm[g] && !dm[d] && !gdc[g] && R[(size_t)g * D + d] >= tr) {
                    sum += P[(size_t)g * D + d];
                    list.push_back(g);
                }
            if (!(py_round4(sum) >= tp)) continue;
            if (overlaps_det(d) < 2) continue;
            const int k = (int)list.size();
            dm[d] = 1;
            racc += k == 1 ? oo : om_m * k;
            pacc += k == 1 ? oo : om_m;
            if (k == 0 && !emit(m, npairs, 2, -1, d)) return false;
            for (int g : list) {
                if (!emit(m, npairs, 2, g, d)) return false;
                gm[g] = 1;
            }
            ++npairs;
        }
        const int gcare = G - ngdc;
        if (gcare == 0) {
            recall = 1.0;
            precision = 0.0;  // (D > 0 here)
        } else {
            recall = racc / gcare;
            precision = D - ndd == 0 ? 0.0 : pacc / (D - ndd);
        }
        hmean = precision + recall == 0.0 ? 0.0 : 2.0 * precision * recall / (precision + recall);
    }
    double* s = m.stats;
    s[0] = precision, s[1] = recall, s[2] = hmean, s[3] = G - ngdc, s[4] = D - ndd, s[5] = 0.0, s[6] = racc, s[7] = pacc;
    return true;
}

}  // namespace

extern "C" {

long dbn_det_eval_ws_bytes(int n_polys) {
    if (n_polys < 0) return -1;
    return 48L * (n_polys > 0 ? n_polys : 1);
}

int dbn_det_eval_overlaps(const double* verts, const int* poff, int n_polys, const long long* img, int N, long n_pairs, int cull, void* ws,
                          double* inter, double* area, int* nonsimple, void* stream) {
    DBN_REQUIRE(verts && poff && img && ws && area && nonsimple && n_polys > 0 && N > 0 && n_pairs >= 0);
    DBN_REQUIRE(n_pairs == 0 || inter);
    const hipStream_t st = (hipStream_t)stream;
    double* meta = (double*)ws;
    hipLaunchKernelGGL(poly_kernel, dim3(n_polys), dim3(256), 0, st, (const P2*)verts, poff, meta, area, nonsimple);
    if (n_pairs > 0) {
        const long grid = n_pairs < (1L << 20) ? n_pairs : (1L << 20);
        hipLaunchKernelGGL(overlap_kernel, dim3((unsigned)grid), dim3(64), 0, st, (const P2*)verts, poff, img, N, n_pairs, (const double*)meta,
                           cull, inter);
    }
    return dbn_status();
}

int dbn_det_eval_match_host(int protocol, int N, const int* sizes, const double* inter, const double* gt_area, const double* det_area,
                            const unsigned char* gt_ignore, const double* gt_cd, const double* det_cd, const double* params, double* stats,
                            unsigned char* det_dc, int* rows, int* n_rows) {
    DBN_REQUIRE((protocol == 0 || protocol == 1) && N >= 0 && sizes && params && stats && n_rows);
    long gb = 0, db = 0, pb = 0, rb = 0;
    for (int n = 0; n < N; ++n) {
        const int G = sizes[2 * n], D = sizes[2 * n + 1];
        DBN_REQUIRE(G >= 0 && D >= 0);
        DBN_REQUIRE((G == 0 || (gt_area && gt_ignore)) && (D == 0 || (det_area && det_dc)) && ((long)G * D == 0 || inter));
        DBN_REQUIRE(protocol == 0 || (long)G * D == 0 || (gt_cd && det_cd));
        DBN_REQUIRE(G + D == 0 || rows);
        Img m;
        m.G = G, m.D = D;
        m.I = inter ? inter + pb : nullptr;
        m.ga = gt_area ? gt_area + gb : nullptr;
        m.da = det_area ? det_area + db : nullptr;
        m.ig = gt_ignore ? gt_ignore + gb : nullptr;
        m.gcd = gt_cd ? gt_cd + 3 * gb : nullptr;
        m.dcd = det_cd ? det_cd + 3 * db : nullptr;
        m.stats = stats + 8L * n;
        m.ddc = det_dc ? det_dc + db : nullptr;
        m.rows = rows ? rows + 4 * rb : nullptr;
        m.cap = 2 * (G + D);
        m.n_rows = 0;
        if (!(protocol == 0 ? match_iou(m, params) : match_deteval(m, params))) return DBN_ERR_ARG;
        n_rows[n] = m.n_rows;
        gb += G, db += D, pb += (long)G * D, rb += 2L * (G + D);
    }
    return DBN_OK;
}

}  // extern "C"
