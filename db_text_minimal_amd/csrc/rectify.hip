// Word images from text POLYGONS: a curved word is straightened into the out_h x out_w image a recogniser takes, beside
// the box crops of resample.hip (warp_perspective_u8).  The reference has no such step (test_ocr.py:162 crops boxes only),
// so both halves are THIS PROJECT'S DEFINITION, stated so that a restatement can follow them exactly:
//   host    dbn_polygon_ribbons  per polygon the ribbon that follows the word: S + 1 knots of a centre line with the
//                                cross-section vector at each, in fp64, rounded to int32 units of 1 / 1024 pixel
//   device  dbn_rectify_u8       every pixel of every crop in one launch: the knot pair of its column interpolated and the
//                                source sampled bilinearly (5 fractional bits), all in 64-bit integers, so the bytes
//                                depend on the knots alone
// The fp64 formulas of the host half must not be contracted into FMAs (the Makefile builds with -ffp-contract=off).
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
