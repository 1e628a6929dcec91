// DBNet ground truth on the device (the reference's data_loaders.py:87-172 + db_transforms.py:8-82), three parts:
//   gt_maps        the four maps of train.py GT_KEYS for a batch in one launch, pixel-major: a workgroup owns a 64 x 16
//                  tile of one image, culls that image's polygons to those whose influence box meets the tile, stages
//                  each one's vertices in LDS and writes every pixel of the four maps exactly once (background included:
//                  no memset, no global atomics).  Every per-polygon operation is order-independent (fill to 1, fill
//                  to 0, fmax), so the polygons need no ordering.
//   normalize_u8   uint8 [N][H][W][3] -> fp32 [N][3][H][W], (float)u8 - (float)mean[c] (data_loaders.py:161-167)
//   poly_offset    host: a restatement of Clipper 6's ClipperOffset (JT_ROUND, ET_CLOSEDPOLYGON, ArcTolerance 0.25) for
//                  one closed path, the shrink / pad the reference gets from pyclipper.  PARITY UNPINNED (see below).
#include <math.h>
#include <float.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "fillpoly.h"

namespace {

constexpr int GT_TW = 64, GT_TH = 16, GT_THREADS = 256;
constexpr int GT_MAX_VERTS = 64;      // vertices of one source polygon (the existing MAX_PTS of postproc.hip)
constexpr int GT_MAX_OFF_PTS = 1024;  // vertices of one shrunk / padded / truncated polygon
constexpr int GT_META = 20;           // ints per polygon, see dbn_gt_maps in include/dbnet_hip.h

// Deletion switch for measurement only (tools/flavour.sh gtmaps.hip -DDBN_GT_ABLATE=n, profiles/r07_gt_maps_ablation.txt):
// 1 drops the threshold term, 2 drops the three fillPoly evaluations.  The product library is built with 0.
#ifndef DBN_GT_ABLATE
#define DBN_GT_ABLATE 0
#endif

// numpy's slicing of draw_thresh_map (db_transforms.py:48-63) along one axis: the index into the polygon's distance map
// (box lo..hi) that lands on canvas pixel X, or -1.  Inside the image this is X - lo.  A box starting k >= 2 pixels past
// the last pixel makes the slice start negative: numpy counts it from the end, and pixel S-1 receives index width - k.
// Where the reference's slice is empty (box wholly before pixel 0, or k == 1, or k > width) it raises; the polygon then
// adds nothing here.
__device__ __forceinline__ int gt_slice_index(int X, int lo, int hi, int S) {
    const int width = hi - lo + 1;
    if (lo <= S - 1) {
        if (hi < 0) return -1;
        return (X >= max(lo, 0) && X <= min(hi, S - 1)) ? X - lo : -1;
    }
    const int k = lo - (S - 1);
    return (X == S - 1 && k >= 2 && k <= width) ? width - k : -1;
}

// 1 - min over the polygon's edges a -> b of fp32(clip(e / D, 0, 1)), e the distance the reference's compute_distance
// returns (db_transforms.py:67-82): with ga = |g - a|^2, gb = |g - b|^2, ab = |a - b|^2 and c = ((ab - ga) - gb) /
// (2 sqrt(ga gb)), e = sqrt(fmin(ga, gb)) if c < 0, else sqrt(((ga gb) nan_to_num(1 - c^2)) / ab).  numpy's operation
// order: fp64 throughout, one rounding to fp32 per edge, NaN-propagating min (np.min), then fp32 1 - m.
__device__ __forceinline__ float gt_thresh_at(double gx, double gy, const double* lx, const double* ly, int V, double D) {
    float m = 0.f;
    for (int i = 0; i < V; ++i) {
        const int j = i + 1 == V ? 0 : i + 1;
        const double uax = gx - lx[i], uay = gy - ly[i], ubx = gx - lx[j], uby = gy - ly[j];
        const double ga = uax * uax + uay * uay, gb = ubx * ubx + uby * uby;
        const double ex = lx[i] - lx[j], ey = ly[i] - ly[j];
        const double ab = ex * ex + ey * ey;
        const double c = ((ab - ga) - gb) / (2.0 * sqrt(ga * gb));
        double s2 = 1.0 - c * c;
        s2 = isnan(s2) ? 0.0 : isinf(s2) ? (s2 > 0 ? DBL_MAX : -DBL_MAX) : s2;  // np.nan_to_num
        double e = sqrt(((ga * gb) * s2) / ab);
        if (c < 0) e = sqrt(fmin(ga, gb));
        e = e / D;
        const double t = isnan(e) ? e : fmin(fmax(e, 0.0), 1.0);  // np.clip keeps NaN
        const float v = (float)t;
        if (i == 0 || isnan(v) || v < m) m = v;  // once NaN, stays NaN
    }
    return 1.f - m;
}

__global__ __launch_bounds__(GT_THREADS) void gt_maps_kernel(const double* __restrict__ verts, const double* __restrict__ dist,
                                                              const int* __restrict__ meta, const int* __restrict__ img_off,
                                                              const int* __restrict__ ixy, int N, int S, int max_verts, int max_off_pts,
                                                              float scale, float tmin, float* __restrict__ out) {
    __shared__ int list[GT_THREADS];
    __shared__ int nlist;
    __shared__ double lx[GT_MAX_VERTS], ly[GT_MAX_VERTS];
    __shared__ int sx[GT_MAX_OFF_PTS], sy[GT_MAX_OFF_PTS], qx[GT_MAX_OFF_PTS], qy[GT_MAX_OFF_PTS];
    const int n = blockIdx.z, x0 = blockIdx.x * GT_TW, y0 = blockIdx.y * GT_TH;
    const int px = x0 + (threadIdx.x & (GT_TW - 1)), py0 = y0 + (threadIdx.x >> 6);
    constexpr int ROWS = GT_TH / (GT_THREADS / GT_TW);  // 4 rows per thread, one wave per row: 256 B coalesced stores
    float prob[ROWS], mask[ROWS], text[ROWS], canvas[ROWS];
#pragma unroll
    for (int k = 0; k < ROWS; ++k) { prob[k] = 0.f; mask[k] = 1.f; text[k] = 0.f; canvas[k] = 0.f; }
    const int pbeg = img_off[n], pend = img_off[n + 1];
    for (int base = pbeg; base < pend; base += GT_THREADS) {
        if (threadIdx.x == 0) nlist = 0;
        __syncthreads();
        const int p = base + (int)threadIdx.x;
        if (p < pend) {
            const int* m = meta + (long)p * GT_META;
            if (m[7] <= x0 + GT_TW - 1 && m[8] >= x0 && m[9] <= y0 + GT_TH - 1 && m[10] >= y0) list[atomicAdd(&nlist, 1)] = p;
        }
        __syncthreads();
        const int cnt = nlist;
        for (int li = 0; li < cnt; ++li) {
            const int* m = meta + (long)list[li] * GT_META;
            const int voff = m[0], vcnt = m[1], ign = m[2], soff = m[3], scnt = m[4], poff = m[5], pcnt = m[6];
            // precondition of dbn_gt_maps: counts <= max_verts / max_off_pts (<= the LDS arrays).  A polygon that breaks it
            // is not drawn at all (never clipped); the uniform branch keeps every thread at the barriers below.
            const bool bad = vcnt < 0 || vcnt > max_verts || scnt < 0 || scnt > max_off_pts || (!ign && (pcnt < 0 || pcnt > max_off_pts));
            if (bad) continue;
            const int bxl = m[11], bxh = m[12], byl = m[13], byh = m[14];  // padded polygon's bbox (the threshold box)
            const int sxl = m[15], sxh = m[16], syl = m[17], syh = m[18];  // bbox of the polygon in sx / sy
            for (int i = threadIdx.x; i < scnt; i += GT_THREADS) { sx[i] = ixy[2L * (soff + i)]; sy[i] = ixy[2L * (soff + i) + 1]; }
            if (!ign) {
                for (int i = threadIdx.x; i < pcnt; i += GT_THREADS) { qx[i] = ixy[2L * (poff + i)]; qy[i] = ixy[2L * (poff + i) + 1]; }
                if (threadIdx.x < vcnt) {  // polygon - (xmin, ymin) of the padded box, in fp64 (db_transforms.py:30-31)
                    lx[threadIdx.x] = verts[2L * (voff + threadIdx.x)] - (double)bxl;
                    ly[threadIdx.x] = verts[2L * (voff + threadIdx.x) + 1] - (double)byl;
                }
            }
            __syncthreads();
            const double D = dist[list[li]];
            const int ix = gt_slice_index(px, bxl, bxh, S);
#pragma unroll
            for (int k = 0; k < ROWS; ++k) {
                const int py = py0 + k * (GT_THREADS / GT_TW);
                if (px >= S || py >= S) continue;
                const bool in_s = px >= sxl && px <= sxh && py >= syl && py <= syh;
                if (ign) {  // supervision_mask: fillPoly(poly.astype(int32), 0)
                    if (DBN_GT_ABLATE != 2 && in_s && mask[k] != 0.f && dbn_fillpoly_hit(px, py, sx, sy, scnt)) mask[k] = 0.f;
                    continue;
                }
                if (DBN_GT_ABLATE != 2) {
                    if (in_s && prob[k] == 0.f && dbn_fillpoly_hit(px, py, sx, sy, scnt)) prob[k] = 1.f;  // fillPoly(shrunk, 1)
                    const bool in_p = px >= bxl && px <= bxh && py >= byl && py <= byh;
                    if (in_p && text[k] == 0.f && dbn_fillpoly_hit(px, py, qx, qy, pcnt)) text[k] = 1.f;  // fillPoly(padded, 1)
                }
                const int iy = gt_slice_index(py, byl, byh, S);
                if (DBN_GT_ABLATE != 1 && ix >= 0 && iy >= 0)
                    canvas[k] = fmaxf(gt_thresh_at((double)ix, (double)iy, lx, ly, vcnt, D), canvas[k]);
            }
            __syncthreads();
        }
    }
    const long plane = (long)N * S * S;
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
        const int py = py0 + k * (GT_THREADS / GT_TW);
        if (px >= S || py >= S) continue;
        const long o = ((long)n * S + py) * S + px;
        out[o] = prob[k];
        out[plane + o] = mask[k];
        out[2 * plane + o] = __fadd_rn(__fmul_rn(canvas[k], scale), tmin);  // thresh_map * (max - min) + min, fp32, no FMA
        out[3 * plane + o] = text[k];
    }
}

__global__ void normalize_u8_kernel(const unsigned char* __restrict__ in, long hw, long total, float m0, float m1, float m2,
                                    float* __restrict__ out) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long n = i / hw, r = i - n * hw;
        const unsigned char* s = in + 3 * i;
        float* d = out + 3 * n * hw + r;
        d[0] = (float)s[0] - m0;
        d[hw] = (float)s[1] - m1;
        d[2 * hw] = (float)s[2] - m2;
    }
}

// ---- host: ClipperOffset (Clipper 6.4, the library pyclipper wraps) for one closed path -------------------------------
struct IPt { long long x, y; };
struct DPt { double x, y; };
inline bool operator==(const IPt& a, const IPt& b) { return a.x == b.x && a.y == b.y; }
inline bool operator!=(const IPt& a, const IPt& b) { return !(a == b); }

inline long long clip_round(double v) { return v < 0 ? (long long)(v - 0.5) : (long long)(v + 0.5); }  // Clipper's Round

// Clipper's Area: positive for the orientation ClipperOffset offsets outwards with delta > 0
double clip_area(const std::vector<IPt>& p) {
    const int n = (int)p.size();
    if (n < 3) return 0;
    double a = 0;
    for (int i = 0, j = n - 1; i < n; ++i) { a += ((double)p[j].x + p[i].x) * ((double)p[j].y - p[i].y); j = i; }
    return -a * 0.5;
}

DPt unit_normal(const IPt& a, const IPt& b) {
    if (a == b) return {0, 0};
    double dx = (double)(b.x - a.x), dy = (double)(b.y - a.y);
    const double f = 1 * 1.0 / sqrt(dx * dx + dy * dy);
    dx *= f; dy *= f;
    return {dy, -dx};
}

// AddPath + FixOrientations + DoOffset: the raw offset path, before Clipper's union clean-up
std::vector<IPt> raw_offset(const std::vector<IPt>& path, double delta) {
    std::vector<IPt> src;
    int high = (int)path.size() - 1;
    if (high < 0) return {};
    while (high > 0 && path[0] == path[high]) --high;  // strip the closing duplicate, then consecutive duplicates
    src.push_back(path[0]);
    for (int i = 1; i <= high; ++i)
        if (src.back() != path[i]) src.push_back(path[i]);
    if (src.size() < 3) return {};  // Clipper drops a closed path with fewer than 3 distinct vertices
    if (clip_area(src) < 0) std::reverse(src.begin(), src.end());  // FixOrientations
    if (fabs(delta) < 1e-20) return src;
    const double y = 0.25 > fabs(delta) * 0.25 ? fabs(delta) * 0.25 : 0.25;  // ArcTolerance 0.25
    double steps = M_PI / acos(1 - y / fabs(delta));
    if (steps > fabs(delta) * M_PI) steps = fabs(delta) * M_PI;
    double sn = sin(2 * M_PI / steps);
    const double cs = cos(2 * M_PI / steps), steps_per_rad = steps / (2 * M_PI);
    if (delta < 0.0) sn = -sn;
    const int len = (int)src.size();
    std::vector<DPt> nrm(len);
    for (int j = 0; j < len; ++j) nrm[j] = unit_normal(src[j], src[(j + 1) % len]);
    std::vector<IPt> dst;
    auto at = [&](int j, const DPt& nv) { return IPt{clip_round(src[j].x + nv.x * delta), clip_round(src[j].y + nv.y * delta)}; };
    for (int j = 0, k = len - 1; j < len; ++j) {  // OffsetPoint(j, k, jtRound)
        double sinA = nrm[k].x * nrm[j].y - nrm[j].x * nrm[k].y;
        if (fabs(sinA * delta) < 1.0) {
            const double cosA = nrm[k].x * nrm[j].x + nrm[j].y * nrm[k].y;
            if (cosA > 0) { dst.push_back(at(j, nrm[k])); continue; }  // (Clipper returns here without k = j)
        } else if (sinA > 1.0) sinA = 1.0;
        else if (sinA < -1.0) sinA = -1.0;
        if (sinA * delta < 0) {  // concave for this offset direction: the three-point case
            dst.push_back(at(j, nrm[k]));
            dst.push_back(src[j]);
            dst.push_back(at(j, nrm[j]));
        } else {  // DoRound
            const double a = atan2(sinA, nrm[k].x * nrm[j].x + nrm[k].y * nrm[j].y);
            const int st = std::max((int)clip_round(steps_per_rad * fabs(a)), 1);
            double X = nrm[k].x, Y = nrm[k].y, X2;
            for (int i = 0; i < st; ++i) {
                dst.push_back(at(j, DPt{X, Y}));
                X2 = X;
                X = X * cs - sn * Y;
                Y = X2 * sn + Y * cs;
            }
            dst.push_back(at(j, nrm[j]));
        }
        k = j;
    }
    return dst;
}

long long cross(long long ax, long long ay, long long bx, long long by) { return ax * by - ay * bx; }

int winding(const std::vector<IPt>& p, double x, double y) {  // nonzero winding number, counter-clockwise (math axes) +1
    int w = 0;
    const int n = (int)p.size();
    for (int i = 0; i < n; ++i) {
        const IPt& a = p[i];
        const IPt& b = p[(i + 1) % n];
        const double side = (double)(b.x - a.x) * (y - a.y) - (x - a.x) * (double)(b.y - a.y);
        if (a.y <= y) { if (b.y > y && side > 0) ++w; }
        else if (b.y <= y && side < 0) --w;
    }
    return w;
}

// Clipper's clean-up of the raw path: the union with positive fill (delta > 0), or for delta < 0 the negative-fill union
// inside an outer rectangle whose first path is dropped.  For a path oriented as FixOrientations leaves it both select
// the region of winding number > 0; that region's boundary is traced here from the path's arrangement: every edge is split
// at every crossing, a piece is kept when the winding number changes from <= 0 to > 0 across it (oriented with the
// region on its left), and kept pieces, with end points rounded to integers as Clipper rounds its intersections, are
// linked into loops.  Returns the loops of positive area (outer boundaries); holes, the loops of negative area, are
// dropped and counted in *holes when it is given.
std::vector<std::vector<IPt>> positive_region(const std::vector<IPt>& p, int* holes = nullptr) {
    const int n = (int)p.size();
    struct Edge { IPt a, b; };
    std::vector<Edge> kept;
    for (int i = 0; i < n; ++i) {
        const IPt a = p[i], b = p[(i + 1) % n];
        if (a == b) continue;
        const long long rx = b.x - a.x, ry = b.y - a.y;
        std::vector<double> ts{0.0, 1.0};
        for (int j = 0; j < n; ++j) {
            const IPt c = p[j], d = p[(j + 1) % n];
            if (j == i || c == d) continue;
            const long long sx = d.x - c.x, sy = d.y - c.y, qx = c.x - a.x, qy = c.y - a.y;
            const long long den = cross(rx, ry, sx, sy);
            if (den != 0) {
                long long tn = cross(qx, qy, sx, sy), un = cross(qx, qy, rx, ry), dd = den;
                if (dd < 0) { tn = -tn; un = -un; dd = -dd; }
                if (tn > 0 && tn < dd && un >= 0 && un <= dd) ts.push_back((double)tn / (double)dd);
            } else if (cross(qx, qy, rx, ry) == 0) {  // collinear: split at the other edge's end points
                const double rr = (double)(rx * rx + ry * ry);
                for (const IPt& e : {c, d}) {
                    const double t = (double)((e.x - a.x) * rx + (e.y - a.y) * ry) / rr;
                    if (t > 0 && t < 1) ts.push_back(t);
                }
            }
        }
        std::sort(ts.begin(), ts.end());
        ts.erase(std::unique(ts.begin(), ts.end()), ts.end());
        for (size_t s = 0; s + 1 < ts.size(); ++s) {
            const double ax = a.x + ts[s] * rx, ay = a.y + ts[s] * ry, bx = a.x + ts[s + 1] * rx, by = a.y + ts[s + 1] * ry;
            const double mx = 0.5 * (ax + bx), my = 0.5 * (ay + by), nl = sqrt((double)(rx * rx + ry * ry));
            const double ex = -ry / nl * 1e-7, ey = rx / nl * 1e-7;  // left of the edge
            const int wl = winding(p, mx + ex, my + ey), wr = winding(p, mx - ex, my - ey);
            const IPt ia{clip_round(ax), clip_round(ay)}, ib{clip_round(bx), clip_round(by)};
            if (ia == ib) continue;
            if (wl > 0 && wr <= 0) kept.push_back({ia, ib});
            else if (wr > 0 && wl <= 0) kept.push_back({ib, ia});
        }
    }
    std::sort(kept.begin(), kept.end(), [](const Edge& u, const Edge& v) {
        return u.a.x != v.a.x ? u.a.x < v.a.x : u.a.y != v.a.y ? u.a.y < v.a.y : u.b.x != v.b.x ? u.b.x < v.b.x : u.b.y < v.b.y;
    });
    kept.erase(std::unique(kept.begin(), kept.end(), [](const Edge& u, const Edge& v) { return u.a == v.a && u.b == v.b; }), kept.end());
    std::vector<char> used(kept.size(), 0);
    std::vector<std::vector<IPt>> loops;
    for (size_t s = 0; s < kept.size(); ++s) {
        if (used[s]) continue;
        std::vector<IPt> loop;
        size_t cur = s;
        bool closed = false;
        for (;;) {
            used[cur] = 1;
            loop.push_back(kept[cur].a);
            const IPt at = kept[cur].b;
            if (at == kept[s].a) { closed = true; break; }
            // next: the unused piece leaving `at` met first turning clockwise from the way back (keeps touching loops apart)
            const double bx = (double)(kept[cur].a.x - at.x), by = (double)(kept[cur].a.y - at.y);
            long best = -1;
            double best_ang = 0;
            for (size_t e = 0; e < kept.size(); ++e) {
                if (used[e] || kept[e].a != at) continue;
                const double ox = (double)(kept[e].b.x - at.x), oy = (double)(kept[e].b.y - at.y);
                double ang = -atan2(bx * oy - by * ox, bx * ox + by * oy);
                if (ang <= 0) ang += 2 * M_PI;
                if (best < 0 || ang < best_ang) { best = (long)e; best_ang = ang; }
            }
            if (best < 0) break;
            cur = (size_t)best;
        }
        // A chain whose rounded end points do not lead back to its start is dropped.  Rounding intersection points can do
        // that where Clipper, which rounds as it goes, still closes a loop; a shrink can then come back smaller or empty
        // (and the polygon be ignored) where pyclipper's would not.  Part of PARITY UNPINNED.
        if (!closed) continue;
        // drop collinear and repeated vertices (Clipper's default: PreserveCollinear off)
        bool changed = true;
        while (changed && loop.size() >= 3) {
            changed = false;
            for (size_t i = 0; i < loop.size() && loop.size() >= 3; ++i) {
                const IPt& a = loop[(i + loop.size() - 1) % loop.size()];
                const IPt& b = loop[i];
                const IPt& c = loop[(i + 1) % loop.size()];
                if (cross(b.x - a.x, b.y - a.y, c.x - b.x, c.y - b.y) == 0) { loop.erase(loop.begin() + i); changed = true; --i; }
            }
        }
        if (loop.size() < 3) continue;
        const double a = clip_area(loop);
        if (a > 0) loops.push_back(loop);
        else if (a < 0 && holes) ++*holes;
    }
    return loops;
}

}  // namespace

extern "C" {

int dbn_gt_maps(const double* verts, const double* dist, const int* meta, const int* img_off, const int* ixy, int N, int P, int S,
                int max_verts, int max_off_pts, float scale, float tmin, float* out, void* stream) {
    DBN_REQUIRE(out && img_off && N > 0 && N <= 65535 && S > 0 && S <= 16384 && P >= 0);
    DBN_REQUIRE(max_verts >= 0 && max_verts <= GT_MAX_VERTS && max_off_pts >= 0 && max_off_pts <= GT_MAX_OFF_PTS);
    DBN_REQUIRE(P == 0 || (verts && dist && meta && ixy));
    const dim3 grid(dbn_ceil_div(S, GT_TW), dbn_ceil_div(S, GT_TH), N);
    hipLaunchKernelGGL(gt_maps_kernel, grid, dim3(GT_THREADS), 0, (hipStream_t)stream, verts, dist, meta, img_off, ixy, N, S, max_verts,
                       max_off_pts, scale, tmin, out);
    return dbn_status();
}

int dbn_normalize_u8(const unsigned char* in, int N, int H, int W, float m0, float m1, float m2, float* out, void* stream) {
    DBN_REQUIRE(in && out && N > 0 && H > 0 && W > 0);
    const long hw = (long)H * W, total = (long)N * hw;
    hipLaunchKernelGGL(normalize_u8_kernel, dim3(dbn_grid(total)), dim3(256), 0, (hipStream_t)stream, in, hw, total, m0, m1, m2, out);
    return dbn_status();
}

// the offset of dbn_poly_offset: the piece of largest area, and the number of paths Clipper's Execute returns (outer
// loops and holes)
static int poly_offset(const double* xy, int n, const double* delta, int* out_xy, int cap, int* out_n, int* out_paths) {
    DBN_REQUIRE(xy && delta && out_n && n >= 0 && cap >= 0 && (cap == 0 || out_xy));
    std::vector<IPt> path(n);
    for (int i = 0; i < n; ++i) {
        DBN_REQUIRE(isfinite(xy[2 * i]) && isfinite(xy[2 * i + 1]) && fabs(xy[2 * i]) < 1e9 && fabs(xy[2 * i + 1]) < 1e9);
        path[i] = {(long long)xy[2 * i], (long long)xy[2 * i + 1]};  // pyclipper's conversion: a C cast (toward zero)
    }
    DBN_REQUIRE(isfinite(*delta));
    const std::vector<IPt> raw = raw_offset(path, *delta);
    std::vector<IPt> best;
    int paths = 0;
    if (!raw.empty()) {
        double best_area = 0;
        int holes = 0;
        const std::vector<std::vector<IPt>> loops = positive_region(raw, &holes);
        for (const auto& l : loops) {  // several pieces: the one of largest area (ties: the first traced)
            const double a = clip_area(l);
            if (a > best_area) { best_area = a; best = l; }
        }
        paths = (int)loops.size() + holes;
    }
    if (out_paths) *out_paths = paths;
    *out_n = (int)best.size();
    if ((int)best.size() > cap) return DBN_ERR_ARG;
    for (size_t i = 0; i < best.size(); ++i) { out_xy[2 * i] = (int)best[i].x; out_xy[2 * i + 1] = (int)best[i].y; }
    return DBN_OK;
}

int dbn_poly_offset(const double* xy, int n, const double* delta, int* out_xy, int cap, int* out_n) {
    return poly_offset(xy, n, delta, out_xy, cap, out_n, nullptr);
}

int dbn_poly_offset_paths(const double* xy, int n, const double* delta, int* out_xy, int cap, int* out_n, int* out_paths) {
    DBN_REQUIRE(out_paths);
    return poly_offset(xy, n, delta, out_xy, cap, out_n, out_paths);
}

}  // extern "C"
