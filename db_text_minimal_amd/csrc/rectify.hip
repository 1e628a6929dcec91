// Word images from text POLYGONS: a curved word is straightened into the out_h x out_w image a recogniser takes, beside
// the box crops of resample.hip (warp_perspective_u8).  The reference has no such step (test_ocr.py:162 crops boxes only),
// so both halves are THIS PROJECT'S DEFINITION, stated so that a restatement can follow them exactly:
//   host    dbn_polygon_ribbons  per polygon the ribbon that follows the word: S + 1 knots of a centre line with the
//                                cross-section vector at each, in fp64, rounded to int32 units of 1 / 1024 pixel
//   device  dbn_rectify_u8       every pixel of every crop in one launch: the knot pair of its column interpolated and the
//                                source sampled bilinearly (5 fractional bits), all in 64-bit integers, so the bytes
//                                depend on the knots alone
//   device  dbn_polygon_ribbons_device  the host half again, one workgroup per polygon, with the host's bits (DESIGN
//                                section 34): every sum in the host's order, its tie rule, a square root rounded in integers
// The fp64 formulas of the ribbons, host and device, must not be contracted into FMAs (the Makefile builds with -ffp-contract=off).
#include <math.h>

#include <algorithm>

#include "common.h"
#include "jpeg_common.h"  // on_threads: the host thread pool of the batch entry points

namespace {

constexpr int RC_MIN_SEG = 4, RC_MAX_SEG = 64, RC_MAX_VERTS = 256;
constexpr int RC_THREADS = 256, RC_PPT = 4, RC_PX = RC_THREADS * RC_PPT, RC_DESC = 3;
constexpr long RC_MAX_HW = 1L << 30;  // see dbn_rectify_u8

// floor(a / d) for d > 0, exactly: the fp64 estimate is within 1 of it (|a / d| < 2^33, each rounding 2^-53 relative), and
// the remainder, exact in 64 bits, says which way
__device__ __forceinline__ long long floor_div(long long a, long long d, double rd) {
    long long q = (long long)floor((double)a * rd);
    const long long r = a - q * d;
    if (r < 0) q -= 1;
    else if (r >= d) q += 1;
    return q;
}

// One workgroup: RC_PX consecutive pixels (row-major) of ONE crop, so its knots are read into LDS once; a thread owns
// RC_PPT consecutive pixels, 12 bytes, stored as three dwords where the destination allows.  A crop whose ribbon is
// invalid, or whose descriptor leaves src_bytes or 1 .. 65535 a side, is written as zeros.
__global__ void __launch_bounds__(RC_THREADS) rectify_u8_kernel(const unsigned char* __restrict__ src, long src_bytes,
                                                                 const long long* __restrict__ desc, const int* __restrict__ knots,
                                                                 const unsigned char* __restrict__ valid, int S, int oh, int ow, int bpc,
                                                                 unsigned char* __restrict__ dst) {
    __shared__ int s_k[(RC_MAX_SEG + 1) * 4];
    const int t = threadIdx.x;
    const long q = blockIdx.x / bpc;
    const int b = (int)(blockIdx.x - q * bpc);
    const int hw = oh * ow;  // <= 2^30 (checked at the launch)
    const long long* dq = desc + q * RC_DESC;
    const long long off = dq[0], sh = dq[1], sw = dq[2];
    const bool ok = valid[q] != 0 && sh >= 1 && sw >= 1 && sh <= 65535 && sw <= 65535 && off >= 0 && off + sh * sw * 3 <= src_bytes;
    if (ok)
        for (int i = t; i < (S + 1) * 4; i += RC_THREADS) s_k[i] = knots[q * (S + 1) * 4 + i];
    __syncthreads();
    const int p0 = b * RC_PX + t * RC_PPT;  // b * RC_PX < hw
    if (p0 >= hw) return;
    const int np = min(RC_PPT, hw - p0);
    unsigned char v[RC_PPT * 3];
#pragma unroll
    for (int i = 0; i < RC_PPT * 3; ++i) v[i] = 0;
    if (ok) {
        const unsigned char* im = src + off;
        const int ih = (int)sh, iw = (int)sw;
        const long long den = 2LL * hw;
        const double rd = 1.0 / (double)den;
#pragma unroll
        for (int i = 0; i < RC_PPT; ++i) {
            if (i < np) {
                const int p = p0 + i, y = p / ow, x = p - y * ow;
                const int xk = x * S, k = xk / ow, r = xk - k * ow;  // k <= S - 1
                const int* a = s_k + k * 4;
                int ip[2], fp[2];
#pragma unroll
                for (int ax = 0; ax < 2; ++ax) {
                    const long long c = (long long)ow * a[ax] + (long long)r * ((long long)a[4 + ax] - a[ax]);
                    const long long n = (long long)ow * a[2 + ax] + (long long)r * ((long long)a[6 + ax] - a[2 + ax]);
                    const long long P = floor_div(2LL * oh * c + (long long)(2 * y - oh) * n + hw, den, rd);  // |.| < 2^63: dbn_rectify_u8
                    const int P5 = (int)((P + 16) >> 5);
                    ip[ax] = P5 >> 5;
                    fp[ax] = P5 & 31;
                }
                const int x0 = ip[0], y0 = ip[1];
                if (x0 >= -1 && x0 < iw && y0 >= -1 && y0 < ih) {
                    const bool xa = x0 >= 0, xb = x0 + 1 < iw, ya = y0 >= 0, yb = y0 + 1 < ih;
                    const int w00 = (32 - fp[0]) * (32 - fp[1]), w01 = fp[0] * (32 - fp[1]), w10 = (32 - fp[0]) * fp[1], w11 = fp[0] * fp[1];
                    const unsigned char* r0 = im + ((long)y0 * iw + x0) * 3;
                    const unsigned char* r1 = r0 + (long)iw * 3;
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const int t00 = ya && xa ? r0[ch] : 0, t01 = ya && xb ? r0[3 + ch] : 0;
                        const int t10 = yb && xa ? r1[ch] : 0, t11 = yb && xb ? r1[3 + ch] : 0;
                        v[i * 3 + ch] = (unsigned char)((w00 * t00 + w01 * t01 + w10 * t10 + w11 * t11 + 512) >> 10);
                    }
                }
            }
        }
    }
    unsigned char* o = dst + ((long)q * hw + p0) * 3;
    if (np == RC_PPT && (reinterpret_cast<size_t>(o) & 3) == 0) {
        unsigned int* o4 = reinterpret_cast<unsigned int*>(o);
#pragma unroll
        for (int j = 0; j < 3; ++j)
            o4[j] = (unsigned)v[4 * j] | ((unsigned)v[4 * j + 1] << 8) | ((unsigned)v[4 * j + 2] << 16) | ((unsigned)v[4 * j + 3] << 24);
    } else {
        for (int j = 0; j < np * 3; ++j) o[j] = v[j];
    }
}

// ---- host: the ribbon of a polygon (fp64, no contraction) ------------------------------------------------------------
struct P2 {
    double x, y;
};

// An open polyline of np >= 2 points with its arclength table: len[s] = |p[s + 1] - p[s]|, cum[0] = 0, cum[s + 1] = cum[s] + len[s]
struct Line {
    const P2* p;
    const double *len, *cum;
};

// the point of the first np points of the line at arclength t: on segment s = the first with cum[s + 1] >= t (the last
// segment if none), p[s] + ((t - cum[s]) / len[s]) (p[s + 1] - p[s]); p[s] itself on a segment of no length
static P2 point_at(const Line& l, int np, double t) {
    int s = (int)(std::lower_bound(l.cum + 1, l.cum + np, t) - (l.cum + 1));
    if (s > np - 2) s = np - 2;
    const double u = l.len[s] > 0.0 ? (t - l.cum[s]) / l.len[s] : 0.0;
    return {l.p[s].x + u * (l.p[s + 1].x - l.p[s].x), l.p[s].y + u * (l.p[s + 1].y - l.p[s].y)};
}

// the S + 1 points of the line's first np points at arclength L k / S, L = cum[np - 1]; the two ends are the end points
static void sample(const Line& l, int np, int S, P2* out) {
    const double L = l.cum[np - 1];
    out[0] = l.p[0];
    for (int k = 1; k < S; ++k) out[k] = point_at(l, np, L * k / S);
    out[S] = l.p[np - 1];
}

static void arclengths(const P2* p, int np, double* len, double* cum) {
    cum[0] = 0.0;
    for (int s = 0; s + 1 < np; ++s) {
        const double dx = p[s + 1].x - p[s].x, dy = p[s + 1].y - p[s].y;
        len[s] = sqrt(dx * dx + dy * dy);
        cum[s + 1] = cum[s] + len[s];
    }
}

// One polygon of n vertices -> knots[(S + 1) * 4], ends[2], info[3] = {E, W, centre-line length}; returns valid.
// (DESIGN section 32 states every step; tests/rectify_ref.py restates them.)
static int ribbon(const double* xy, int n, int S, bool half, int* knots, int* ends, double* info) {
    const int m = 2 * n;
    // boundary points: vertices and edge midpoints, once forward (twice round) and once backward (twice round), so that
    // every chain is a contiguous run; fwd[t] = pts[t mod m], bwd[t] = pts[-t mod m]
    std::vector<P2> fwd(2 * m), bwd(2 * m);
    for (int i = 0; i < n; ++i) {
        const double x0 = xy[2 * i], y0 = xy[2 * i + 1], x1 = xy[2 * ((i + 1) % n)], y1 = xy[2 * ((i + 1) % n) + 1];
        fwd[2 * i] = {x0, y0};
        fwd[2 * i + 1] = {(x0 + x1) * 0.5, (y0 + y1) * 0.5};
    }
    for (int t = 0; t < m; ++t) fwd[m + t] = fwd[t];
    for (int t = 0; t < 2 * m; ++t) bwd[t] = fwd[(2 * m - t) % m];
    std::vector<double> lenA(m), cumA(m + 1), lenB(m), cumB(m + 1);
    std::vector<P2> A(S + 1), B(S + 1), M(S + 1), C(S + 1);
    int bi = -1, bj = -1;
    double bE = 0.0;
    if (half) {
        bi = m - 1, bj = n - 1;
    } else {
        for (int i = 0; i < m - 2; ++i) {
            // the arclength tables of the two chains from point i do not depend on where they end
            const Line la = {fwd.data() + i, lenA.data(), cumA.data()}, lb = {bwd.data() + (m - i) % m, lenB.data(), cumB.data()};
            arclengths(la.p, m + 1, lenA.data(), cumA.data());
            arclengths(lb.p, m + 1, lenB.data(), cumB.data());
            for (int j = i + 2; j < m && j - i <= m - 2; ++j) {
                // samples 0 and S are the two end points on both chains and add an exact 0; the sum only grows, and the
                // division is monotonic, so a pair is out as soon as its partial mean reaches the best one
                const int na = j - i + 1, nb = m - (j - i) + 1;
                const double La = cumA[na - 1], Lb = cumB[nb - 1];
                double sum = 0.0;
                bool out = false;
                for (int k = 1; k < S && !out; ++k) {
                    const P2 a = point_at(la, na, La * k / S), b = point_at(lb, nb, Lb * k / S);
                    const double dx = a.x - b.x, dy = a.y - b.y;
                    sum += dx * dx + dy * dy;
                    out = bi >= 0 && sum / (S + 1) >= bE;
                }
                if (!out) bi = i, bj = j, bE = sum / (S + 1);
            }
        }
    }
    ends[0] = bi, ends[1] = bj;
    const int steps = ((bj - bi) % m + m) % m;  // forward steps from point bi to point bj
    const Line la = {fwd.data() + bi, lenA.data(), cumA.data()}, lb = {bwd.data() + (m - bi) % m, lenB.data(), cumB.data()};
    arclengths(la.p, steps + 1, lenA.data(), cumA.data());
    arclengths(lb.p, m - steps + 1, lenB.data(), cumB.data());
    sample(la, steps + 1, S, A.data());
    sample(lb, m - steps + 1, S, B.data());
    double sum = 0.0, w2 = 0.0;
    for (int k = 0; k <= S; ++k) {
        const double dx = A[k].x - B[k].x, dy = A[k].y - B[k].y, d2 = dx * dx + dy * dy;
        sum += d2;
        if (d2 > w2) w2 = d2;
        M[k] = {(A[k].x + B[k].x) * 0.5, (A[k].y + B[k].y) * 0.5};
    }
    const double W = sqrt(w2);
    std::vector<double> lenM(S), cumM(S + 1);
    arclengths(M.data(), S + 1, lenM.data(), cumM.data());
    sample({M.data(), lenM.data(), cumM.data()}, S + 1, S, C.data());
    info[0] = sum / (S + 1), info[1] = W, info[2] = cumM[S];
    // twice the signed area, about vertex 0 (exact for integer vertices)
    double area2 = 0.0;
    for (int i = 1; i + 1 < n; ++i) {
        const double ax = xy[2 * i] - xy[0], ay = xy[2 * i + 1] - xy[1], bx = xy[2 * i + 2] - xy[0], by = xy[2 * i + 3] - xy[1];
        area2 += ax * by - bx * ay;
    }
    bool valid = cumM[S] > 0.0 && W > 0.0 && area2 != 0.0;
    if (!half) {
        const double dx = C[S].x - C[0].x, dy = C[S].y - C[0].y;
        if (fabs(dx) >= fabs(dy) ? C[0].x > C[S].x : C[0].y > C[S].y) std::reverse(C.begin(), C.end());
    }
    for (int j = 0; j <= S && valid; ++j) {
        const P2 &a = C[j > 0 ? j - 1 : 0], &b = C[j < S ? j + 1 : S];
        const double tx = b.x - a.x, ty = b.y - a.y, tl = sqrt(tx * tx + ty * ty);
        const double nx = tl > 0.0 ? W * (-ty / tl) : 0.0, ny = tl > 0.0 ? W * (tx / tl) : 0.0;
        const double o[4] = {rint(1024.0 * C[j].x), rint(1024.0 * C[j].y), rint(1024.0 * nx), rint(1024.0 * ny)};
        for (int e = 0; e < 4; ++e) {
            valid = valid && fabs(o[e]) <= 2147483647.0;  // a cross-section too long for int32: no crop
            if (valid) knots[j * 4 + e] = (int)o[e];
        }
    }
    if (!valid)
        for (int e = 0; e < (S + 1) * 4; ++e) knots[e] = 0;
    return valid ? 1 : 0;
}

// ---- device: the same ribbons, bit for bit --------------------------------------------------------
// Every fp64 operation of ribbon() above is repeated in its order; +, -, *, / and rint are IEEE on the device as on the
// host (no contraction, see the Makefile), and the square root is made correctly rounded in integers below.
constexpr int RB_THREADS = 256, RB_WAVES = RB_THREADS / 64, RB_MAX_M = 2 * RC_MAX_VERTS;
constexpr double RB_MAX_COORD = 1048576.0;
typedef unsigned long long rb_u64;
typedef unsigned __int128 rb_u128;

// floor(sqrt(N)) for N < 2^108, from any estimate r < 2^54: up to 8 steps of one, which an estimate within a few units
// needs, else bit by bit.  Exact 128-bit products decide, so the result does not depend on the estimate.
__device__ rb_u64 rb_isqrt(rb_u128 N, rb_u64 r) {
    for (int it = 0; it < 8; ++it) {
        if ((rb_u128)r * r > N) --r;
        else if ((rb_u128)(r + 1) * (r + 1) <= N) ++r;
        else return r;
    }
    r = 0;
    for (int b = 53; b >= 0; --b) {
        const rb_u64 c = r | (1ULL << b);
        if ((rb_u128)c * c <= N) r = c;
    }
    return r;
}

// sqrt(x) rounded to nearest for a finite x >= 0, as the host's sqrt gives it.  x = M 2^q with q even and M an integer in
// [2^52, 2^54); r = floor(sqrt(M 2^54)) has 54 bits, one more than a double holds, and sqrt(M 2^54) is not an integer when r is
// odd (the square root of a double is never the midpoint of two doubles), so (r + 1) >> 1 is sqrt(M) 2^26 rounded to nearest.
__device__ double rb_sqrt(double x) {
    if (!(x > 0.0)) return 0.0;
    rb_u64 bits = __builtin_bit_cast(rb_u64, x);
    int ex = (int)(bits >> 52);
    rb_u64 M = bits & ((1ULL << 52) - 1);
    if (ex == 0) {  // subnormal: x = M 2^-1074; bring the leading bit to bit 52
        const int sh = __builtin_clzll(M) - 11;
        M <<= sh;
        ex = 1 - sh;
    } else {
        M |= 1ULL << 52;
    }
    int q = ex - 1075;  // x = M 2^q
    if (q & 1) M <<= 1, q -= 1;
    const rb_u64 est = (rb_u64)(sqrt((double)M) * 134217728.0);  // < 2^54 for any sqrt that is roughly right; only an estimate
    const rb_u64 r = rb_isqrt((rb_u128)M << 54, est < (1ULL << 54) ? est : (1ULL << 54) - 1);
    const rb_u64 R = (r + 1) >> 1;  // [2^52, 2^53]: exact as a double
    const double scale = __builtin_bit_cast(double, (rb_u64)(q / 2 - 26 + 1023) << 52);  // 2^(q / 2 - 26), a normal number
    return (double)R * scale;  // exact: a power of two, and the result is normal
}

// the segment of point_at: the first s with cum[s + 1] >= t, np - 2 if none, searched upward from s.  Equal to the host's
// lower_bound because cum never decreases, and in a loop over k because t = L k / S never decreases either.
__device__ __forceinline__ int rb_segment(const double* cum, int np, double t, int s) {
    while (s < np - 2 && cum[s + 1] < t) ++s;
    return s;
}

// point_at on the chain that starts at boundary point i and runs forward (back = false) or backward round the m points:
// its point s is pts[i +- s], its segment s has the length len[] of that pair of points (len[e] = |pts[e + 1] - pts[e]|, which
// is the same in both directions: dx dx has no sign)
__device__ __forceinline__ P2 rb_point(const P2* pts, const double* len, const double* cum, int m, int i, bool back, int np, double t, int& s) {
    s = rb_segment(cum, np, t, s);
    int a = back ? i - s : i + s;
    a += a < 0 ? m : 0;
    a -= a >= m ? m : 0;
    int b = back ? a - 1 : a + 1;
    b += b < 0 ? m : 0;
    b -= b >= m ? m : 0;
    const double l = len[back ? b : a];
    const double u = l > 0.0 ? (t - cum[s]) / l : 0.0;
    const P2 pa = pts[a], pb = pts[b];
    return {pa.x + u * (pb.x - pa.x), pa.y + u * (pb.y - pa.y)};
}

__device__ __forceinline__ void rb_take_smaller(rb_u64& e, unsigned& ij, rb_u64 e2, unsigned ij2) {
    if (e2 < e || (e2 == e && ij2 < ij)) e = e2, ij = ij2;
}

// One workgroup per polygon.  LDS: 8 KB of boundary points, 4 KB of segment lengths, per wave the two arclength tables of
// its start point (8.2 KB), and the final stage's S + 1 samples: 48.6 KB.  A polygon the host entry would refuse (offs or a
// coordinate out of range) is written as valid 0, zero knots, ends (-1, -1), info 0, and nothing of xy outside
// [0, 2 total) is read.
__global__ void __launch_bounds__(RB_THREADS) polygon_ribbons_kernel(const double* __restrict__ xy, const long long* __restrict__ offs, long total,
                                                                     int S, int half, int* __restrict__ knots, unsigned char* __restrict__ valid,
                                                                     int* __restrict__ ends, double* __restrict__ info) {
    __shared__ P2 s_pts[RB_MAX_M];
    __shared__ double s_len[RB_MAX_M];
    __shared__ double s_cum[RB_WAVES][2][RB_MAX_M + 1];
    __shared__ P2 s_M[RC_MAX_SEG + 1], s_C[RC_MAX_SEG + 1];
    __shared__ double s_d2[RC_MAX_SEG + 1], s_lenM[RC_MAX_SEG + 1], s_cumM[RC_MAX_SEG + 1];
    __shared__ rb_u64 s_bestE[RB_WAVES];
    __shared__ unsigned s_bestIJ[RB_WAVES];
    __shared__ double s_sum, s_W, s_area2;
    __shared__ int s_bad;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long q = blockIdx.x;
    int* kq = knots + q * (S + 1) * 4;
    const long long o0 = offs[q], o1 = offs[q + 1];
    const bool range = o0 >= 0 && o1 <= total && o1 >= o0 && o1 - o0 >= 3 && o1 - o0 <= RC_MAX_VERTS && !(half && ((o1 - o0) & 1));
    const int n = range ? (int)(o1 - o0) : 0, m = 2 * n;
    const double* v = xy + 2 * (range ? o0 : 0);
    if (t == 0) s_bad = 0;
    __syncthreads();
    double x0 = 0.0, y0 = 0.0;
    if (t < n) {
        x0 = v[2 * t], y0 = v[2 * t + 1];
        if (!(fabs(x0) <= RB_MAX_COORD && fabs(y0) <= RB_MAX_COORD)) s_bad = 1;  // also a NaN
    }
    __syncthreads();
    if (!range || s_bad) {  // the same for every lane
        for (int e = t; e < (S + 1) * 4; e += RB_THREADS) kq[e] = 0;
        if (t == 0) {
            valid[q] = 0;
            ends[2 * q] = ends[2 * q + 1] = -1;
            info[3 * q] = info[3 * q + 1] = info[3 * q + 2] = 0.0;
        }
        return;
    }
    // boundary points: vertex i at 2 i, the middle of edge (i, i + 1) at 2 i + 1
    if (t < n) {
        const int nx = t + 1 < n ? t + 1 : 0;
        const double x1 = v[2 * nx], y1 = v[2 * nx + 1];
        s_pts[2 * t] = {x0, y0};
        s_pts[2 * t + 1] = {(x0 + x1) * 0.5, (y0 + y1) * 0.5};
    }
    __syncthreads();
    for (int e = t; e < m; e += RB_THREADS) {
        const int b = e + 1 < m ? e + 1 : 0;
        const double dx = s_pts[b].x - s_pts[e].x, dy = s_pts[b].y - s_pts[e].y;
        s_len[e] = rb_sqrt(dx * dx + dy * dy);
    }
    __syncthreads();

    int bi = m - 1, bj = n - 1;  // half
    if (!half) {
        // every pair in full; the smallest E wins and ties go to the smallest (i, j), which is what the host's early exit
        // and strict comparison leave.  E >= 0 and is no NaN, so its bits order as an unsigned integer.
        rb_u64 bE = ~0ULL;
        unsigned bIJ = ~0u;
        double *cumA = s_cum[wave][0], *cumB = s_cum[wave][1];
        for (int i0 = 0; i0 < m - 2; i0 += RB_WAVES) {
            const int i = i0 + wave;
            if (i < m - 2 && lane < 2) {  // lane 0: the forward table from point i, lane 1: the backward one; running sums in order
                double* c = lane ? cumB : cumA;
                const int step = lane ? -1 : 1;
                int e = lane ? (i > 0 ? i - 1 : m - 1) : i;
                double acc = 0.0;
                c[0] = 0.0;
                for (int s = 0; s < m; ++s) {
                    acc += s_len[e];
                    c[s + 1] = acc;
                    e += step;
                    e += e < 0 ? m : 0;
                    e -= e >= m ? m : 0;
                }
            }
            __syncthreads();
            if (i < m - 2) {
                for (int j = i + 2 + lane; j < m && j - i <= m - 2; j += 64) {
                    const int na = j - i + 1, nb = m - (j - i) + 1;
                    const double La = cumA[na - 1], Lb = cumB[nb - 1];
                    double sum = 0.0;
                    int sa = 0, sb = 0;
                    for (int k = 1; k < S; ++k) {
                        const P2 a = rb_point(s_pts, s_len, cumA, m, i, false, na, La * k / S, sa);
                        const P2 b = rb_point(s_pts, s_len, cumB, m, i, true, nb, Lb * k / S, sb);
                        const double dx = a.x - b.x, dy = a.y - b.y;
                        sum += dx * dx + dy * dy;
                    }
                    rb_take_smaller(bE, bIJ, __builtin_bit_cast(rb_u64, sum / (S + 1)), (unsigned)(i * RB_MAX_M + j));
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const rb_u64 e2 = __shfl_xor(bE, o, 64);
            const unsigned ij2 = __shfl_xor(bIJ, o, 64);
            rb_take_smaller(bE, bIJ, e2, ij2);
        }
        if (lane == 0) s_bestE[wave] = bE, s_bestIJ[wave] = bIJ;
        __syncthreads();
        bE = s_bestE[0], bIJ = s_bestIJ[0];
#pragma unroll
        for (int w = 1; w < RB_WAVES; ++w) rb_take_smaller(bE, bIJ, s_bestE[w], s_bestIJ[w]);
        bi = (int)(bIJ / RB_MAX_M), bj = (int)(bIJ % RB_MAX_M);  // m >= 6: at least the pair (0, 2) was taken
    }

    // the final stage of ribbon(), lane k on sample k where the steps are independent, one lane where they are a running sum
    const int steps = ((bj - bi) % m + m) % m, na = steps + 1, nb = m - steps + 1;
    double *cumA = s_cum[0][0], *cumB = s_cum[0][1];
    if (t == 0 || t == 64) {
        const bool back = t != 0;
        double* c = back ? cumB : cumA;
        const int cnt = back ? nb - 1 : na - 1;
        int e = back ? (bi > 0 ? bi - 1 : m - 1) : bi;
        double acc = 0.0;
        c[0] = 0.0;
        for (int s = 0; s < cnt; ++s) {
            acc += s_len[e];
            c[s + 1] = acc;
            e += back ? -1 : 1;
            e += e < 0 ? m : 0;
            e -= e >= m ? m : 0;
        }
    }
    if (t == 128) {  // twice the signed area about vertex 0
        double area2 = 0.0;
        const P2 p0 = s_pts[0];
        for (int i = 1; i + 1 < n; ++i) {
            const double ax = s_pts[2 * i].x - p0.x, ay = s_pts[2 * i].y - p0.y, bx = s_pts[2 * i + 2].x - p0.x, by = s_pts[2 * i + 2].y - p0.y;
            area2 += ax * by - bx * ay;
        }
        s_area2 = area2;
    }
    __syncthreads();
    if (t <= S) {
        P2 a, b;
        if (t == 0) {
            a = b = s_pts[bi];
        } else if (t == S) {
            a = b = s_pts[bj];  // point bi + steps forward, point bi - (m - steps) backward
        } else {
            int sa = 0, sb = 0;
            a = rb_point(s_pts, s_len, cumA, m, bi, false, na, cumA[na - 1] * t / S, sa);
            b = rb_point(s_pts, s_len, cumB, m, bi, true, nb, cumB[nb - 1] * t / S, sb);
        }
        const double dx = a.x - b.x, dy = a.y - b.y;
        s_d2[t] = dx * dx + dy * dy;
        s_M[t] = {(a.x + b.x) * 0.5, (a.y + b.y) * 0.5};
    }
    __syncthreads();
    if (t < S) {
        const double dx = s_M[t + 1].x - s_M[t].x, dy = s_M[t + 1].y - s_M[t].y;
        s_lenM[t] = rb_sqrt(dx * dx + dy * dy);
    }
    if (t == 64) {
        double sum = 0.0, w2 = 0.0;
        for (int k = 0; k <= S; ++k) {
            sum += s_d2[k];
            if (s_d2[k] > w2) w2 = s_d2[k];
        }
        s_sum = sum;
        s_W = rb_sqrt(w2);
    }
    __syncthreads();
    if (t == 0) {
        double acc = 0.0;
        s_cumM[0] = 0.0;
        for (int s = 0; s < S; ++s) {
            acc += s_lenM[s];
            s_cumM[s + 1] = acc;
        }
    }
    __syncthreads();
    const double W = s_W, Lm = s_cumM[S];
    if (t <= S) {
        int s = 0;
        s_C[t] = t == 0 || t == S ? s_M[t] : rb_point(s_M, s_lenM, s_cumM, S + 1, 0, false, S + 1, Lm * t / S, s);
    }
    if (t == 0) {
        info[3 * q] = s_sum / (S + 1), info[3 * q + 1] = W, info[3 * q + 2] = Lm;
        ends[2 * q] = bi, ends[2 * q + 1] = bj;
    }
    __syncthreads();
    bool rev = false;
    if (!half) {
        const double dx = s_C[S].x - s_C[0].x, dy = s_C[S].y - s_C[0].y;
        rev = fabs(dx) >= fabs(dy) ? s_C[0].x > s_C[S].x : s_C[0].y > s_C[S].y;
    }
    const bool base = Lm > 0.0 && W > 0.0 && s_area2 != 0.0;
    double o[4] = {0.0, 0.0, 0.0, 0.0};
    if (t <= S && base) {
        const int ja = t > 0 ? t - 1 : 0, jb = t < S ? t + 1 : S;
        const P2 a = s_C[rev ? S - ja : ja], b = s_C[rev ? S - jb : jb], c = s_C[rev ? S - t : t];
        const double tx = b.x - a.x, ty = b.y - a.y, tl = rb_sqrt(tx * tx + ty * ty);
        const double nx = tl > 0.0 ? W * (-ty / tl) : 0.0, ny = tl > 0.0 ? W * (tx / tl) : 0.0;
        o[0] = rint(1024.0 * c.x), o[1] = rint(1024.0 * c.y), o[2] = rint(1024.0 * nx), o[3] = rint(1024.0 * ny);
        for (int e = 0; e < 4; ++e)
            if (!(fabs(o[e]) <= 2147483647.0)) s_bad = 1;  // a cross-section too long for int32: no crop
    }
    __syncthreads();
    const bool ok = base && !s_bad;
    if (t <= S)
        for (int e = 0; e < 4; ++e) kq[t * 4 + e] = ok ? (int)o[e] : 0;
    if (t == 0) valid[q] = ok ? 1 : 0;
}

}  // namespace

extern "C" {

int dbn_polygon_ribbons(const double* xy, const long long* offs, int K, int segments, int half, int threads, int* knots,
                        unsigned char* valid, int* ends, double* info) {
    DBN_REQUIRE(K >= 0 && segments >= RC_MIN_SEG && segments <= RC_MAX_SEG && (half == 0 || half == 1));
    if (K == 0) return DBN_OK;
    DBN_REQUIRE(xy && offs && knots && valid && ends && info && offs[0] == 0);
    for (int k = 0; k < K; ++k) {
        const long long n = offs[k + 1] - offs[k];
        DBN_REQUIRE(n >= 3 && n <= RC_MAX_VERTS && (!half || n % 2 == 0));
        for (long long i = 2 * offs[k]; i < 2 * offs[k + 1]; ++i) DBN_REQUIRE(fabs(xy[i]) <= 1048576.0);  // false for a NaN
    }
    dbn_jpeg::on_threads(K, threads, [&](int k) {
        valid[k] = (unsigned char)ribbon(xy + 2 * offs[k], (int)(offs[k + 1] - offs[k]), segments, half != 0,
                                         knots + (long)k * (segments + 1) * 4, ends + 2 * k, info + 3 * k);
    });
    return DBN_OK;
}

int dbn_polygon_ribbons_device(const double* xy, const long long* offs, int K, long total_vertices, int segments, int half, int* knots,
                               unsigned char* valid, int* ends, double* info, void* stream) {
    DBN_REQUIRE(K >= 0 && total_vertices >= 0 && segments >= RC_MIN_SEG && segments <= RC_MAX_SEG && (half == 0 || half == 1));
    if (K == 0) return DBN_OK;
    DBN_REQUIRE(xy && offs && knots && valid && ends && info);  // device pointers: what they hold is the kernel's to check
    hipLaunchKernelGGL(polygon_ribbons_kernel, dim3((unsigned)K), dim3(RB_THREADS), 0, (hipStream_t)stream, xy, offs, total_vertices, segments,
                       half, knots, valid, ends, info);
    return dbn_status();
}

int dbn_rectify_u8(const unsigned char* src, long src_bytes, const long long* desc, const int* knots, const unsigned char* valid, int K,
                   int segments, int out_h, int out_w, unsigned char* dst, long dst_bytes, void* stream) {
    DBN_REQUIRE(K >= 0 && segments >= RC_MIN_SEG && segments <= RC_MAX_SEG && out_h > 0 && out_w > 0 && out_h <= 65535 && out_w <= 65535);
    // any int32 knots: |c|, |n| <= out_w 2^31 after the interpolation, so the numerator stays below
    // 3 out_h out_w 2^31 + out_h out_w < 2^63 while out_h out_w <= 2^30
    const long hw = (long)out_h * out_w;
    DBN_REQUIRE(hw <= RC_MAX_HW);
    if (K == 0) return DBN_OK;
    DBN_REQUIRE(src && desc && knots && valid && dst && dst_bytes >= (long)K * hw * 3);
    const long bpc = (hw + RC_PX - 1) / RC_PX, blocks = (long)K * bpc;
    DBN_REQUIRE(blocks <= 2147483647L);
    hipLaunchKernelGGL(rectify_u8_kernel, dim3((unsigned)blocks), dim3(RC_THREADS), 0, (hipStream_t)stream, src, src_bytes, desc, knots, valid,
                       segments, out_h, out_w, (int)bpc, dst);
    return dbn_status();
}

}  // extern "C"
