// Showing a detection result on the device: the last step of the reference's inference path (utils.py:202-283, test.py,
// test_ocr.py, test_webcam.py), on packed ragged uint8 HWC images (the layout of image_collate):
//   draw_strokes     utils.draw_bbox: cv2.polylines(img.copy(), [pts], True, color, thickness) of every box / polygon
//   draw_glyphs      the cv2.putText step of test_ocr.py / test_webcam.py: labels as filled DejaVu Sans outlines (this
//                    project's definition, see "labels" below)
//   render_minmax    the minimum and maximum, per image, of the probability map resized to that image (what
//                    plt.imshow(tmp_pred) autoscales to); the resized values are never stored
//   render_paint     cv2.resize(prob, (W, H)) INTER_LINEAR in float -> matplotlib Normalize -> Colormap byte table ->
//                    alpha blend over the image, one pass: every pixel read once and written once
//   minmax_scale_u8  utils.minmax_scaler_img of fp32 [N][3][H][W] -> uint8 [N][H][W][3]
//
// Strokes.  thickness 1 paints the pixels of dbn_on_line (fillpoly.h: LineIterator, 8-connected; evaluated in 64 bits
// here, on_line64), so a thickness-1 outline is exactly the border fillPoly draws here.  thickness t >= 2 is THIS
// PROJECT'S DEFINITION, not OpenCV's ThickLine (a fixed-point quadrilateral plus end discs; pixels on the rim of a stroke
// may differ from cv2's): pixel p is painted iff its squared
// distance to the closed segment a-b satisfies 4 d^2 <= t^2 (a stadium; joins and caps are round).  In integers, with
// d = b - a, w = p - a, len2 = |d|^2, dot = d.w, cross = d x w:
//   dot <= 0       4 |p - a|^2 <= t^2     (a zero-length edge has dot = 0 everywhere: the disc about a)
//   dot > len2     4 |p - b|^2 <= t^2
//   else           4 cross^2 <= t^2 len2
// 64 bits suffice.  Vertices lie within +-2^20 and pixels within 0 .. 65534, so |d|, |w| < 2^21.1 per component: dot and
// cross are below 2^44 and len2, |p - a|^2 below 2^44, t^2 len2 below 2^60.  Only cross^2 could overflow, and a painted
// pixel has |cross| <= t sqrt(len2) / 2 < 2^29: a candidate with |cross| >= 2^30 is rejected before squaring, the others
// have 4 cross^2 < 2^62.
//
// One wave owns one edge.  It walks the edge's major axis (x when |dx| >= |dy|), clipped to the image and extended by the
// cap radius; a lane owns a column u, finds the line's minor coordinate there (vc = floor of the exact rational, at u
// clamped into the edge's span) and tests the 2 t + 4 candidates vc - t - 1 .. vc + t + 2 with the exact predicate.  Every
// painted pixel of column u is among them: inside the span its distance to the line is at most t / 2, so its minor offset
// from the line is at most (t / 2) sqrt(2) < t; past an end its closest point q of the segment is within t / 2 in both
// coordinates, q is within t / 2 of the end along the major axis and hence (slope <= 1) along the minor one: |v - v_end| <=
// t.  All shapes of a call have one colour, so overlapping strokes store the same bytes and the result does not depend
// on scheduling.
//
// Float arithmetic is IEEE fp32 / fp64 in the order written, never contracted (the Makefile builds with
// -ffp-contract=off).  PARITY UNPINNED against cv2.resize itself; the colour layer is pinned against
// matplotlib on the CPU.
#include <math.h>

#include "common.h"

namespace {

constexpr int RD_THREADS = 256, RD_PPT = 4, RD_PX = RD_THREADS * RD_PPT;
constexpr int RD_IDESC = 3;  // int64 per image of draw_strokes: byte offset, height, width
constexpr int RD_PDESC = 5;  // int64 per image of the heat map: first pixel in the packed run, height, width, valid map rows, columns
constexpr int RD_COEF = 4;   // doubles per image: scale_x, scale_y, vmin, vmax

// ---- strokes ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long floor_div(long long a, long long b) {  // b > 0
    const long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// is pixel (px, py) within t / 2 of the closed segment (xa, ya)-(xb, yb)?  (the bounds above)
__device__ __forceinline__ bool stroke_hit(int px, int py, int xa, int ya, int xb, int yb, int t) {
    const long long dx = (long long)xb - xa, dy = (long long)yb - ya, wx = (long long)px - xa, wy = (long long)py - ya;
    const long long len2 = dx * dx + dy * dy, dot = dx * wx + dy * wy, t2 = (long long)t * t;
    if (dot <= 0) return 4 * (wx * wx + wy * wy) <= t2;
    if (dot > len2) {
        const long long ex = (long long)px - xb, ey = (long long)py - yb;
        return 4 * (ex * ex + ey * ey) <= t2;
    }
    long long cross = dx * wy - dy * wx;
    cross = cross < 0 ? -cross : cross;
    if (cross >= (1LL << 30)) return false;
    return 4 * cross * cross <= t2 * len2;
}

// dbn_on_line of fillpoly.h, the same formula in 64 bits: its int products 2 * dx * i pass 2^31 once an edge is longer than
// 32 767 pixels, which full-resolution boxes (int16 corners, sides to 65 535) and polygon vertices (+-2^20) can be
__device__ __forceinline__ bool on_line64(int px, int py, int xa, int ya, int xb, int yb) {
    long long dx = (long long)xb - xa, dy = (long long)yb - ya, x1 = xa, y1 = ya;
    if (dx < 0) { x1 = xb; y1 = yb; dx = -dx; dy = -dy; }
    const long long sy = dy < 0 ? -1 : 1;
    dy = dy < 0 ? -dy : dy;
    if (dy > dx) {  // steep: one pixel per row
        const long long i = (py - y1) * sy;
        if (i < 0 || i > dy) return false;
        return px == x1 + (2 * dx * i + dy - 1) / (2 * dy);
    }
    const long long i = px - x1;
    if (i < 0 || i > dx) return false;
    const long long m = dx == 0 ? 0 : (2 * dy * i + dx - 1) / (2 * dx);
    return py == y1 + sy * m;
}

constexpr int ST_WAVES = RD_THREADS / 64, ST_EDGE = 5;  // int per edge: image, xa, ya, xb, yb
constexpr int ST_VMAX = 1 << 20;

__global__ void __launch_bounds__(RD_THREADS) draw_strokes_kernel(unsigned char* __restrict__ dst, long bytes, const long long* __restrict__ desc,
                                                                   int N, const int* __restrict__ edges, long E, int t, int c0, int c1, int c2) {
    const long e = (long)blockIdx.x * ST_WAVES + (threadIdx.x >> 6);
    if (e >= E) return;
    const int lane = threadIdx.x & 63;
    const int* ed = edges + e * ST_EDGE;
    const int n = ed[0], xa = ed[1], ya = ed[2], xb = ed[3], yb = ed[4];
    if (n < 0 || n >= N) return;
    const long long off = desc[(long)n * RD_IDESC], H = desc[(long)n * RD_IDESC + 1], W = desc[(long)n * RD_IDESC + 2];
    if (H < 1 || W < 1 || H > 65535 || W > 65535 || off < 0 || off + H * W * 3 > bytes) return;
    if (xa < -ST_VMAX || xa > ST_VMAX || ya < -ST_VMAX || ya > ST_VMAX || xb < -ST_VMAX || xb > ST_VMAX || yb < -ST_VMAX || yb > ST_VMAX) return;
    const int adx = xb > xa ? xb - xa : xa - xb, ady = yb > ya ? yb - ya : ya - yb;
    const bool steep = ady > adx;  // the major axis u is y
    const int ua = steep ? ya : xa, va = steep ? xa : ya, ub = steep ? yb : xb, vb = steep ? xb : yb;
    const int U = steep ? (int)H : (int)W, V = steep ? (int)W : (int)H;
    const int cap = t == 1 ? 0 : t / 2 + 1;
    const int smin = ua < ub ? ua : ub, smax = ua < ub ? ub : ua;
    const int ulo = smin - cap > 0 ? smin - cap : 0, uhi = smax + cap < U - 1 ? smax + cap : U - 1;
    unsigned char* img = dst + off;
    for (int u = ulo + lane; u <= uhi; u += 64) {
        const int uc = u < smin ? smin : (u > smax ? smax : u);
        const int vc = ub == ua ? va : va + (int)floor_div(((long long)vb - va) * ((long long)uc - ua) * (ub > ua ? 1 : -1), smax - smin);
        int v0 = vc - t - 1, v1 = vc + t + 2;
        v0 = v0 < 0 ? 0 : v0;
        v1 = v1 > V - 1 ? V - 1 : v1;
        for (int v = v0; v <= v1; ++v) {
            const int px = steep ? v : u, py = steep ? u : v;
            const bool hit = t == 1 ? on_line64(px, py, xa, ya, xb, yb) : stroke_hit(px, py, xa, ya, xb, yb, t);
            if (hit) {
                unsigned char* o = img + ((long)py * W + px) * 3;
                o[0] = (unsigned char)c0;
                o[1] = (unsigned char)c1;
                o[2] = (unsigned char)c2;
            }
        }
    }
}

// ---- labels: filled glyph outlines ---------------------------------------------------------------------------------------
// The last step of test_ocr.py:197-210 / test_webcam.py:274-284 (cv2.putText of every recognised string).  THIS PROJECT'S
// DEFINITION, not cv2's Hershey strokes: the outlines of DejaVu Sans (fonts/dejavu_sans.txt: integer font units, 2048 per
// em, quadratics already flattened into chords), filled by the non-zero winding rule at pixel centres, on or off, in
// exact integers.  PARITY UNPINNED against cv2.putText by construction.
//
// The lattice is 1 / L pixel, L = 64 * 2048 = 2^17; size64 is the em size in 1/64 pixel.  Relative to the pen of a glyph
// instance (org = the left end of the baseline, pen = the advances before it in font units) a vertex v sits at
// v * size64 and the centre of pixel (px, py) at
//   Px = ((64 px + 32) - 64 org.x) * 2048 - pen * size64,   Py = (64 org.y - (64 py + 32)) * 2048     (font y points up)
// and an edge a -> b counts +1 if ay <= Py < by and cr > 0, -1 if by <= Py < ay and cr < 0, with
// cr = (bx - ax)(Py - ay) - (by - ay)(Px - ax); the pixel is painted iff the sum over the glyph's edges is not 0.
//
// 64 bits suffice.  Only pixels whose centre lies inside the glyph's bounding box (xmin, ymin, xmax, ymax of the index,
// scaled) are evaluated, and an instance is skipped unless X = (xmax - xmin) size64 < 2^35 and Y = (ymax - ymin) size64 <
// 2^27.  Edge ends and the centre then lie in one X by Y rectangle, so both products of cr are below 2^62 and cr below
// 2^63.  The font's own glyphs stay far inside: |v| <= 2048 + 106 font units and size64 <= rint(512 * 64 * 2048 / 1493) =
// 44 949 < 2^15.5 give coordinates below 2^29 and products below 2^58.  The background rectangle of a label (at most 256
// advances of at most 2048 units wide, ascender - descender = 2384 units high, plus its margin) reaches X < 2^34.5, Y <
// 2^26.8.  Before the box is known, L org (|org| <= 2^20), pen size64 (pen < 2^20) and L px (px < 2^16) are below 2^37.
//
// One workgroup owns one glyph instance; its waves stage the glyph's scaled edges in LDS once (at most GL_EDGES; a glyph
// with more is skipped) and walk the clipped box in bands of GL_BAND rows, blockIdx.y striding the bands.  A pixel reads
// every edge (all lanes read the same LDS address: a broadcast) and skips those whose y range misses it.  Only painted
// pixels are stored, as three bytes.  One colour per launch: overlapping glyphs store the same bytes, as the strokes do.
constexpr int GL_EDGES = 512, GL_BAND = 16;
constexpr int GL_GLYPH = 6;  // int per glyph of the index: first edge, edges, xmin, ymin, xmax, ymax (font units)
constexpr int GL_REC = 5;    // int per instance: image, glyph, pen (font units), org x, org y
constexpr int GL_EDGE = 4;   // int per edge: ax, ay, bx, by (font units)
constexpr long long GL_L = 64LL * 2048;

__global__ void __launch_bounds__(RD_THREADS) draw_glyphs_kernel(unsigned char* __restrict__ dst, long bytes, const long long* __restrict__ desc,
                                                                  int N, const int* __restrict__ edges, long E, const int* __restrict__ glyphs,
                                                                  int G, const int* __restrict__ recs, int size64, int c0, int c1, int c2) {
    __shared__ long long s_e[GL_EDGES * GL_EDGE];
    const int* rc = recs + (long)blockIdx.x * GL_REC;
    const int n = rc[0], g = rc[1], pen = rc[2], ox = rc[3], oy = rc[4];
    if (n < 0 || n >= N || g < 0 || g >= G || pen < 0 || pen > ST_VMAX || ox < -ST_VMAX || ox > ST_VMAX || oy < -ST_VMAX || oy > ST_VMAX) return;
    const long long off = desc[(long)n * RD_IDESC], H = desc[(long)n * RD_IDESC + 1], W = desc[(long)n * RD_IDESC + 2];
    if (H < 1 || W < 1 || H > 65535 || W > 65535 || off < 0 || off + H * W * 3 > bytes) return;
    const int* gi = glyphs + (long)g * GL_GLYPH;
    const long e0 = gi[0];
    const int ne = gi[1];
    const long long s = size64;
    const long long gx0 = gi[2], gy0 = gi[3], gx1 = gi[4], gy1 = gi[5];
    if (e0 < 0 || ne < 1 || ne > GL_EDGES || e0 + ne > E || gx1 < gx0 || gy1 < gy0) return;
    if (gx0 < -ST_VMAX || gx1 > ST_VMAX || gy0 < -ST_VMAX || gy1 > ST_VMAX || (gx1 - gx0) * s >= (1LL << 35) || (gy1 - gy0) * s >= (1LL << 27)) return;
    // the pixels whose centre lies in the box: gx0 s <= Px <= gx1 s, gy0 s <= Py <= gy1 s
    const long long bx = GL_L * ox + pen * s - GL_L / 2, by = GL_L * oy - GL_L / 2;  // Px = L px - bx, Py = by - L py
    long long x_lo = floor_div(gx0 * s + bx + GL_L - 1, GL_L), x_hi = floor_div(gx1 * s + bx, GL_L);
    long long y_lo = floor_div(by - gy1 * s + GL_L - 1, GL_L), y_hi = floor_div(by - gy0 * s, GL_L);
    x_lo = x_lo < 0 ? 0 : x_lo;
    y_lo = y_lo < 0 ? 0 : y_lo;
    x_hi = x_hi > W - 1 ? W - 1 : x_hi;
    y_hi = y_hi > H - 1 ? H - 1 : y_hi;
    if (x_lo > x_hi || y_lo > y_hi) return;
    const int cols = (int)(x_hi - x_lo + 1), rows = (int)(y_hi - y_lo + 1);
    if ((long)blockIdx.y * GL_BAND >= rows) return;
    for (int i = threadIdx.x; i < ne * GL_EDGE; i += RD_THREADS) s_e[i] = (long long)edges[e0 * GL_EDGE + i] * s;
    __syncthreads();
    unsigned char* img = dst + off;
    for (int r0 = blockIdx.y * GL_BAND; r0 < rows; r0 += gridDim.y * GL_BAND) {
        const int nr = rows - r0 < GL_BAND ? rows - r0 : GL_BAND;
        const unsigned cnt = (unsigned)nr * (unsigned)cols;  // <= 16 * 65535
        for (unsigned i = threadIdx.x; i < cnt; i += RD_THREADS) {
            const unsigned r = i / (unsigned)cols;
            const long long px = x_lo + (i - r * (unsigned)cols), py = y_lo + r0 + r;
            const long long Px = GL_L * px - bx, Py = by - GL_L * py;
            int wn = 0;
            for (int e = 0; e < ne; ++e) {
                const long long ay = s_e[e * GL_EDGE + 1], byy = s_e[e * GL_EDGE + 3];
                const bool up = ay <= Py && Py < byy, down = byy <= Py && Py < ay;
                if (up || down) {
                    const long long ax = s_e[e * GL_EDGE], bxx = s_e[e * GL_EDGE + 2];
                    const long long cr = (bxx - ax) * (Py - ay) - (byy - ay) * (Px - ax);
                    wn += (up && cr > 0) ? 1 : ((down && cr < 0) ? -1 : 0);
                }
            }
            if (wn != 0) {
                unsigned char* o = img + ((long)py * W + px) * 3;
                o[0] = (unsigned char)c0;
                o[1] = (unsigned char)c1;
                o[2] = (unsigned char)c2;
            }
        }
    }
}

// ---- the resized probability map ----------------------------------------------------------------------------------------
// cv2.resize INTER_LINEAR on float data (resize.cpp: the table loop of resize, HResizeLinear / VResizeLinear with float
// weights): fx = (float)((dx + 0.5) * scale - 0.5), sx = cvFloor(fx), fx -= sx; a column below 0 or at / past the last one is
// reset to the edge with fx = 0; rows keep their fraction and clamp both taps.  D = b0 * (S[sx] a0 + S[sx+1] a1) + b1 * (...).
struct MapSrc {
    const float* p;  // channel 0 of the image's map
    int vh, vw, stride;
    int binary;
    float thresh;
};

__device__ __forceinline__ float map_tap(const MapSrc& m, int y, int x) {
    const float s = m.p[(long)y * m.stride + x];
    return m.binary ? (s > m.thresh ? 1.f : 0.f) : s;
}

__device__ __forceinline__ float resized_value(const MapSrc& m, int x, int y, double scale_x, double scale_y) {
    float fx = (float)(((double)x + 0.5) * scale_x - 0.5);
    int sx = (int)floorf(fx);
    fx -= (float)sx;
    if (sx < 0) fx = 0.f, sx = 0;
    if (sx >= m.vw - 1) fx = 0.f, sx = m.vw - 1;
    const int sx1 = sx + 1 < m.vw ? sx + 1 : m.vw - 1;
    float fy = (float)(((double)y + 0.5) * scale_y - 0.5);
    const int sy = (int)floorf(fy);
    fy -= (float)sy;
    const int y0 = sy < 0 ? 0 : (sy > m.vh - 1 ? m.vh - 1 : sy), y1 = sy + 1 < 0 ? 0 : (sy + 1 > m.vh - 1 ? m.vh - 1 : sy + 1);
    const float a0 = 1.f - fx, a1 = fx, b0 = 1.f - fy, b1 = fy;
    const float r0 = map_tap(m, y0, sx) * a0 + map_tap(m, y0, sx1) * a1;
    const float r1 = map_tap(m, y1, sx) * a0 + map_tap(m, y1, sx1) * a1;
    return b0 * r0 + b1 * r1;
}

// floats as unsigned keys in numeric order (finite values and infinities; -0 sorts below +0)
__device__ __forceinline__ unsigned f2key(float f) {
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key2f(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// mm[n] = {key(min), ~key(max)}: both fold with atomicMin from a buffer of 0xFF bytes, and the order of the folds does not
// enter the result.  The words only ever decrease, so a plain (possibly stale) read that is already at or below the
// candidate proves the atomic would change nothing: after the first few folds almost every wave skips it, which keeps
// thousands of waves from queueing on two addresses per image.
__device__ __forceinline__ void mm_flush(unsigned* mm, int n, unsigned kmin, unsigned kmax_inv) {
    volatile unsigned* v = mm + 2 * (long)n;
    if (kmin < v[0]) atomicMin(mm + 2 * (long)n, kmin);
    if (kmax_inv < v[1]) atomicMin(mm + 2 * (long)n + 1, kmax_inv);
}

// the image that holds pixel p of the packed run: the last n in [lo, hi] with first_pixel[n] <= p
__device__ __forceinline__ int image_of(const long long* __restrict__ desc, int lo, int hi, long p) {
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (desc[(long)mid * RD_PDESC] <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

struct Pixel {
    int n, x, y;
    MapSrc m;
    bool ok;
};

// descriptor of image n and the position of packed pixel p inside it; ok = the descriptor is sane (the Python layer
// checks the same before the launch)
__device__ __forceinline__ Pixel locate(const long long* __restrict__ desc, int n, long p, const float* __restrict__ prob, long map_elems,
                                        long img_stride, int row_stride, int binary, float thresh) {
    const long long* d = desc + (long)n * RD_PDESC;
    const long long first = d[0], H = d[1], W = d[2], vh = d[3], vw = d[4];
    Pixel r;
    r.n = n;
    r.ok = H >= 1 && W >= 1 && H <= 65535 && W <= 65535 && vh >= 1 && vw >= 1 && vw <= row_stride && p >= first && p - first < H * W &&
           img_stride >= 0 && (long)n * img_stride + (vh - 1) * (long)row_stride + vw <= map_elems;
    const unsigned q = r.ok ? (unsigned)(p - first) : 0u, w = r.ok ? (unsigned)W : 1u;
    r.y = (int)(q / w);
    r.x = (int)(q - (unsigned)r.y * w);
    r.m = {prob + (long)n * img_stride, (int)vh, (int)vw, row_stride, binary, thresh};
    return r;
}

__global__ void __launch_bounds__(RD_THREADS) render_minmax_kernel(const long long* __restrict__ desc, const double* __restrict__ coef, int N,
                                                                    long n_px, const float* __restrict__ prob, long map_elems, long img_stride,
                                                                    int row_stride, int binary, float thresh, unsigned* __restrict__ mm) {
    __shared__ int s_n[2];
    const int t = threadIdx.x;
    const long p0 = (long)blockIdx.x * RD_PX, pend = min(p0 + RD_PX, n_px) - 1;
    if (t < 2) s_n[t] = image_of(desc, 0, N - 1, t == 0 ? p0 : pend);
    __syncthreads();
    const int n_lo = s_n[0], n_hi = s_n[1];
    int cur = -1;
    unsigned kmin = 0xFFFFFFFFu, kmaxi = 0xFFFFFFFFu;
#pragma unroll
    for (int i = 0; i < RD_PPT; ++i) {
        const long p = p0 + i * RD_THREADS + t;
        if (p >= n_px) break;
        const int n = n_lo == n_hi ? n_lo : image_of(desc, n_lo, n_hi, p);
        const Pixel px = locate(desc, n, p, prob, map_elems, img_stride, row_stride, binary, thresh);
        if (!px.ok) continue;
        if (n != cur) {
            if (cur >= 0) mm_flush(mm, cur, kmin, kmaxi);
            cur = n, kmin = 0xFFFFFFFFu, kmaxi = 0xFFFFFFFFu;
        }
        const unsigned k = f2key(resized_value(px.m, px.x, px.y, coef[(long)n * RD_COEF], coef[(long)n * RD_COEF + 1]));
        kmin = k < kmin ? k : kmin;
        kmaxi = ~k < kmaxi ? ~k : kmaxi;
    }
    // a wave whose lanes all end in the same image folds once
    const int first = __shfl(cur, 0, 64);
    if (__all(cur == first)) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned a = __shfl_xor(kmin, o, 64), b = __shfl_xor(kmaxi, o, 64);
            kmin = a < kmin ? a : kmin;
            kmaxi = b < kmaxi ? b : kmaxi;
        }
        if ((t & 63) == 0 && cur >= 0) mm_flush(mm, cur, kmin, kmaxi);
    } else if (cur >= 0) {
        mm_flush(mm, cur, kmin, kmaxi);
    }
}

// matplotlib.colors.Normalize on a float32 array with float64 limits, then Colormap.__call__'s index:
// t = (float)((double)(float)((double)v - vmin) / (vmax - vmin)) (numpy computes `resdat -= vmin; resdat /= (vmax - vmin)`
// in double and stores float32), 0 where vmin == vmax; xa = t * 256 in float, 256 -> 255, below 0 -> 0, at / above 256 -> 255,
// else truncated.
__device__ __forceinline__ int color_index(float v, double vmin, double vmax) {
    float tt = 0.f;
    if (vmin != vmax) {
        const float s = (float)((double)v - vmin);
        tt = (float)((double)s / (vmax - vmin));
    }
    const float xa = tt * 256.f;
    if (xa == 256.f) return 255;
    if (!(xa >= 0.f)) return 0;  // negative (and NaN, which a finite map never gives)
    if (xa >= 256.f) return 255;
    return (int)xa;
}

// out = rint(img * (1 - a) + colour * a): one fp32 subtraction, two products, one sum, half to even
__device__ __forceinline__ unsigned char blend(unsigned char img, unsigned col, float ia, float a) {
    const float r = (float)img * ia + (float)col * a;
    const int q = __float2int_rn(r);
    return (unsigned char)(q < 0 ? 0 : (q > 255 ? 255 : q));
}

// Each workgroup owns RD_PX consecutive pixels of the packed run (they may span images): it loads their bytes as dwords
// into LDS, every thread repaints its own pixels there, and the run is stored as dwords.  src may be dst.
__global__ void __launch_bounds__(RD_THREADS) render_paint_kernel(const unsigned char* src, unsigned char* dst,
                                                                   const long long* __restrict__ desc, const double* __restrict__ coef, int N,
                                                                   long n_px, const float* __restrict__ prob, long map_elems, long img_stride,
                                                                   int row_stride, int binary, float thresh, const unsigned* __restrict__ mm,
                                                                   const unsigned* __restrict__ lut, float alpha) {
    __shared__ unsigned s_px[RD_PX * 3 / 4];
    __shared__ unsigned s_lut[256];
    __shared__ int s_n[2];
    unsigned char* sb = reinterpret_cast<unsigned char*>(s_px);
    const int t = threadIdx.x;
    const long p0 = (long)blockIdx.x * RD_PX, pend = min(p0 + RD_PX, n_px) - 1;
    const long b0 = p0 * 3, nb = min((long)RD_PX * 3, n_px * 3 - b0);
    const bool wide = nb == RD_PX * 3 && ((reinterpret_cast<size_t>(src + b0) | reinterpret_cast<size_t>(dst + b0)) & 3) == 0;
    if (wide) {
        const unsigned* s4 = reinterpret_cast<const unsigned*>(src + b0);
#pragma unroll
        for (int j = 0; j < 3; ++j) s_px[j * RD_THREADS + t] = s4[j * RD_THREADS + t];
    } else {
        for (long j = t; j < nb; j += RD_THREADS) sb[j] = src[b0 + j];
    }
    s_lut[t] = lut[t];
    if (t < 2) s_n[t] = image_of(desc, 0, N - 1, t == 0 ? p0 : pend);
    __syncthreads();
    const int n_lo = s_n[0], n_hi = s_n[1];
    const float ia = 1.f - alpha;
#pragma unroll
    for (int i = 0; i < RD_PPT; ++i) {
        const int lp = i * RD_THREADS + t;
        const long p = p0 + lp;
        if (p >= n_px) break;
        const int n = n_lo == n_hi ? n_lo : image_of(desc, n_lo, n_hi, p);
        const Pixel px = locate(desc, n, p, prob, map_elems, img_stride, row_stride, binary, thresh);
        if (!px.ok) continue;  // the pixel keeps the source's bytes
        const double* c = coef + (long)n * RD_COEF;
        const float v = resized_value(px.m, px.x, px.y, c[0], c[1]);
        const double vmin = mm ? (double)key2f(mm[2 * (long)n]) : c[2], vmax = mm ? (double)key2f(~mm[2 * (long)n + 1]) : c[3];
        const unsigned col = s_lut[color_index(v, vmin, vmax)];
        sb[lp * 3] = blend(sb[lp * 3], col & 255u, ia, alpha);
        sb[lp * 3 + 1] = blend(sb[lp * 3 + 1], (col >> 8) & 255u, ia, alpha);
        sb[lp * 3 + 2] = blend(sb[lp * 3 + 2], (col >> 16) & 255u, ia, alpha);
    }
    __syncthreads();
    if (wide) {
        unsigned* o4 = reinterpret_cast<unsigned*>(dst + b0);
#pragma unroll
        for (int j = 0; j < 3; ++j) o4[j * RD_THREADS + t] = s_px[j * RD_THREADS + t];
    } else {
        for (long j = t; j < nb; j += RD_THREADS) dst[b0 + j] = sb[j];
    }
}

// ---- utils.minmax_scaler_img ----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RD_THREADS) plane_minmax_kernel(const float* __restrict__ x, long per_image, unsigned* __restrict__ mm) {
    const int n = blockIdx.y;
    const float* p = x + (long)n * per_image;
    unsigned kmin = 0xFFFFFFFFu, kmaxi = 0xFFFFFFFFu;
    for (long i = (long)blockIdx.x * RD_THREADS + threadIdx.x; i < per_image; i += (long)gridDim.x * RD_THREADS) {
        const unsigned k = f2key(p[i]);
        kmin = k < kmin ? k : kmin;
        kmaxi = ~k < kmaxi ? ~k : kmaxi;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned a = __shfl_xor(kmin, o, 64), b = __shfl_xor(kmaxi, o, 64);
        kmin = a < kmin ? a : kmin;
        kmaxi = b < kmaxi ? b : kmaxi;
    }
    if ((threadIdx.x & 63) == 0) mm_flush(mm, n, kmin, kmaxi);
}

// numpy on float32 data: ((x - min) * (1 / (max - min) * 255)).astype(uint8): the factor is float32 (a float32 scalar
// against Python ints stays float32), the product float32, astype truncates.  max == min gives 0 * inf = NaN in numpy, whose
// cast to uint8 is undefined: here such an image is all zeros.  Four pixels per thread, stored as three dwords.
__global__ void __launch_bounds__(RD_THREADS) minmax_scale_u8_kernel(const float* __restrict__ x, int N, long hw, const unsigned* __restrict__ mm,
                                                                      unsigned char* __restrict__ out) {
    const long quads = (hw + 3) / 4;
    const long g = (long)blockIdx.x * RD_THREADS + threadIdx.x;
    if (g >= quads * N) return;
    const int n = (int)(g / quads);
    const long q = (g - (long)n * quads) * 4;
    const float lo = key2f(mm[2 * (long)n]), hi = key2f(~mm[2 * (long)n + 1]);
    const bool flat = !(hi > lo);
    const float f = (1.f / (hi - lo)) * 255.f;
    const float* p = x + (long)n * 3 * hw;
    unsigned char b[12];
    const int cnt = hw - q < 4 ? (int)(hw - q) : 4;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = 0.f;
            if (j < cnt && !flat) v = (p[c * hw + q + j] - lo) * f;
            const int iv = (int)v;
            b[j * 3 + c] = (unsigned char)(iv < 0 ? 0 : (iv > 255 ? 255 : iv));
        }
    unsigned char* o = out + ((long)n * hw + q) * 3;
    if (cnt == 4 && (reinterpret_cast<size_t>(o) & 3) == 0) {
        unsigned* o4 = reinterpret_cast<unsigned*>(o);
#pragma unroll
        for (int j = 0; j < 3; ++j) o4[j] = b[4 * j] | (b[4 * j + 1] << 8) | (b[4 * j + 2] << 16) | ((unsigned)b[4 * j + 3] << 24);
    } else {
        for (int j = 0; j < cnt * 3; ++j) o[j] = b[j];
    }
}

}  // namespace

extern "C" {

int dbn_draw_strokes(const unsigned char* src, unsigned char* dst, long bytes, const long long* desc, int N, const int* edges, long E,
                     int thickness, int c0, int c1, int c2, void* stream) {
    DBN_REQUIRE(src && dst && desc && bytes > 0 && N > 0 && E >= 0 && (E == 0 || edges) && thickness >= 1 && thickness <= 255);
    DBN_REQUIRE(c0 >= 0 && c0 <= 255 && c1 >= 0 && c1 <= 255 && c2 >= 0 && c2 <= 255);
    const long blocks = (E + ST_WAVES - 1) / ST_WAVES;
    DBN_REQUIRE(blocks <= 2147483647L);
    if (src != dst) {
        const hipError_t e = hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream);
        if (e != hipSuccess) return 1000 + (int)e;
    }
    if (E > 0)
        hipLaunchKernelGGL(draw_strokes_kernel, dim3((unsigned)blocks), dim3(RD_THREADS), 0, (hipStream_t)stream, dst, bytes, desc, N, edges, E,
                           thickness, c0, c1, c2);
    return dbn_status();
}

int dbn_draw_glyphs(const unsigned char* src, unsigned char* dst, long bytes, const long long* desc, int N, const int* edges, long E,
                    const int* glyphs, int G, const int* recs, long R, int size64, int rows, int c0, int c1, int c2, void* stream) {
    DBN_REQUIRE(src && dst && desc && bytes > 0 && N > 0 && R >= 0 && R <= 2147483647L && (R == 0 || (edges && glyphs && recs && E > 0 && G > 0)));
    DBN_REQUIRE(size64 >= 1 && size64 <= 65536 && rows >= 1 && rows <= 65535);
    DBN_REQUIRE(c0 >= 0 && c0 <= 255 && c1 >= 0 && c1 <= 255 && c2 >= 0 && c2 <= 255);
    if (src != dst) {
        const hipError_t e = hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream);
        if (e != hipSuccess) return 1000 + (int)e;
    }
    if (R > 0)
        hipLaunchKernelGGL(draw_glyphs_kernel, dim3((unsigned)R, (unsigned)((rows + GL_BAND - 1) / GL_BAND)), dim3(RD_THREADS), 0, (hipStream_t)stream,
                           dst, bytes, desc, N, edges, E, glyphs, G, recs, size64, c0, c1, c2);
    return dbn_status();
}

int dbn_render_minmax(const long long* desc, const double* coef, int N, long n_px, const float* prob, long map_elems, long img_stride,
                      int row_stride, int binary, float thresh, void* mm, void* stream) {
    DBN_REQUIRE(desc && coef && prob && mm && N > 0 && n_px > 0 && map_elems > 0 && img_stride >= 0 && row_stride > 0);
    const long blocks = (n_px + RD_PX - 1) / RD_PX;
    DBN_REQUIRE(blocks <= 2147483647L);
    const hipError_t e = hipMemsetAsync(mm, 0xFF, (size_t)N * 8, (hipStream_t)stream);
    if (e != hipSuccess) return 1000 + (int)e;
    hipLaunchKernelGGL(render_minmax_kernel, dim3((unsigned)blocks), dim3(RD_THREADS), 0, (hipStream_t)stream, desc, coef, N, n_px, prob, map_elems,
                       img_stride, row_stride, binary, thresh, (unsigned*)mm);
    return dbn_status();
}

int dbn_render_paint(const unsigned char* src, unsigned char* dst, const long long* desc, const double* coef, int N, long n_px, const float* prob,
                     long map_elems, long img_stride, int row_stride, int binary, float thresh, const void* mm, const void* lut, float alpha,
                     void* stream) {
    DBN_REQUIRE(src && dst && desc && coef && prob && lut && N > 0 && n_px > 0 && map_elems > 0 && img_stride >= 0 && row_stride > 0);
    DBN_REQUIRE(alpha >= 0.f && alpha <= 1.f);
    const long blocks = (n_px + RD_PX - 1) / RD_PX;
    DBN_REQUIRE(blocks <= 2147483647L);
    hipLaunchKernelGGL(render_paint_kernel, dim3((unsigned)blocks), dim3(RD_THREADS), 0, (hipStream_t)stream, src, dst, desc, coef, N, n_px, prob,
                       map_elems, img_stride, row_stride, binary, thresh, (const unsigned*)mm, (const unsigned*)lut, alpha);
    return dbn_status();
}

int dbn_minmax_scale_u8(const float* x, int N, int H, int W, void* mm, unsigned char* out, void* stream) {
    DBN_REQUIRE(x && mm && out && N > 0 && N <= 65535 && H > 0 && W > 0);
    const long hw = (long)H * W, quads = (hw + 3) / 4;
    const long blocks = (quads * N + RD_THREADS - 1) / RD_THREADS;
    DBN_REQUIRE(blocks <= 2147483647L);
    const hipError_t e = hipMemsetAsync(mm, 0xFF, (size_t)N * 8, (hipStream_t)stream);
    if (e != hipSuccess) return 1000 + (int)e;
    hipLaunchKernelGGL(plane_minmax_kernel, dim3(dbn_grid(3 * hw, RD_THREADS, 512), N), dim3(RD_THREADS), 0, (hipStream_t)stream, x, 3 * hw,
                       (unsigned*)mm);
    hipLaunchKernelGGL(minmax_scale_u8_kernel, dim3((unsigned)blocks), dim3(RD_THREADS), 0, (hipStream_t)stream, x, N, hw, (const unsigned*)mm, out);
    return dbn_status();
}

}  // extern "C"
