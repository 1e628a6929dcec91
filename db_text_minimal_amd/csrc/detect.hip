// Text boxes from probability maps: SegDetectorRepresenter.boxes_from_bitmap (the reference's src/postprocess.py:105-141,
// is_output_polygon=False) for a whole batch, in two stages.
//
// Device stage (dbn_detect), per image n with bitmap = pred[n][0] > thresh (fp32 compare, as dbn_binarize_u8):
//   tile_label    union-find of one 64 x 16 tile in LDS: foreground 8-connected, background 4-connected, in one pass
//                 (a pixel only ever joins pixels of its own class).  Union by atomicMin, so a root is always the
//                 smallest raster index of its set: labels do not depend on the schedule.
//   merge         the union across tile borders in global memory; every access of the parent array in this launch is
//                 an agent-scope atomic (other workgroups write it in the same launch).
//   flatten       labels[p] = root of p, into a separate array (no in-place compression, so no cross-workgroup race).
//   row_count     fg roots per row; marks every component touching the image edge (a bg one is then not a hole).
//   row_scan      suffix sums of the row counts: candidates come in DESCENDING raster order of their first pixel.
//   rank          a candidate's slot = number of fg roots after it; slots >= max_candidates are dropped.
//   run_stats     pred summed over each component in exact fixed point (integer atomics on the root's accumulator)
//                 and the bounding box of each candidate.
//   tree          filled(C) = C and every component it encloses: each component adds its own sum to every candidate
//                 on its chain of enclosing components.  The parent of X is the component of the pixel left of X's
//                 first pixel, or the outside when that pixel is in column 0 or in a background component that
//                 touches the image edge.
//   hull          one workgroup per candidate: per-row extreme pixels -> monotone chain -> the min-area rectangle of
//                 the hull, all in integers, into a fixed-size record.
// Nothing is a float atomic; every sum is an integer, so two runs give the same bits.
//
// Host stage (dbn_detect_host): the per-box geometry of postprocess.py:118-140 on the records: R1 corners, score,
// get_mini_boxes order, unclip (shapely area / length + the Clipper restatement of gtmaps.hip), R2, scaling to
// dest size.  PARITY UNPINNED against cv2 / pyclipper: see DESIGN.md "Text boxes on the device".
//
// Polygons (dbn_detect_poly, dbn_detect_poly_host): polygons_from_bitmap (postprocess.py:54-103) on the same candidates.
// The device traces every kept candidate's outer border at once: cracks (pixel, side) with a successor from a 2 x 2 block,
// Wyllie pointer jumping to each border's head, weights that mark CHAIN_APPROX_SIMPLE vertices, and a scatter of the
// packed int16 vertices.  The host runs approxPolyDP, the fp64 score, the unclip with its path count, the min-area
// rectangle check and the fp64 scaling.  See DESIGN.md section 17.
#include <limits.h>
#include <math.h>

#include <algorithm>
#include <vector>

#include "common.h"

extern "C" int dbn_poly_offset(const double* xy, int n, const double* delta, int* out_xy, int cap, int* out_n);  // gtmaps.hip
extern "C" int dbn_poly_offset_paths(const double* xy, int n, const double* delta, int* out_xy, int cap, int* out_n, int* out_paths);

namespace {

constexpr int DT_TW = 64, DT_TH = 16, DT_TPX = DT_TW * DT_TH;  // label tile
constexpr int DT_RUN = 64;                                     // pixels per thread in run_stats
constexpr int DT_CHAIN = 2048;                                 // vertices of one hull chain (>= 3.6 * 16384^(2/3) / 2)
constexpr int DT_MAX_SIDE = 16384;                             // H, W limit: hull vertices are stored as int16
constexpr int DT_HULL_ROWS = 64;                               // rows of per-row extremes staged per step in the hull kernel

// the record of include/dbnet_hip.h (dbn_detect_rec)
struct Rec {
    int root, hull_n, ex, ey;
    long long dmin, dmax, cmin, cmax;
    long long sum_hi, sum_lo, count;
};
static_assert(sizeof(Rec) == 72, "dbn_detect_rec is 72 bytes");

typedef __attribute__((address_space(1))) int gi32;
typedef __attribute__((address_space(3))) int li32;

// ---- union-find, root = smallest index (L[x] <= x always) ---------------------------------------------------------
template <typename P, int SCOPE>
__device__ __forceinline__ int uf_find(P* L, int x) {
    for (;;) {
        const int p = __hip_atomic_load(L + x, __ATOMIC_RELAXED, SCOPE);
        if (p == x) return x;
        x = p;
    }
}

template <typename P, int SCOPE>
__device__ __forceinline__ void uf_union(P* L, int a, int b) {
    for (;;) {
        a = uf_find<P, SCOPE>(L, a);
        b = uf_find<P, SCOPE>(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }  // link the larger root under the smaller
        const int old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, SCOPE);
        if (old == a) return;
        a = old;  // a was linked meanwhile: retry from where it points
    }
}

__global__ __launch_bounds__(256) void tile_label_kernel(const float* __restrict__ pred, long plane_stride, int H, int W, float thresh,
                                                         unsigned char* __restrict__ bitmap, int* __restrict__ L) {
    __shared__ int lab[DT_TPX];
    __shared__ unsigned char cls[DT_TPX];
    const int n = blockIdx.z, x0 = blockIdx.x * DT_TW, y0 = blockIdx.y * DT_TH;
    const long hw = (long)H * W;
    for (int li = threadIdx.x; li < DT_TPX; li += 256) {
        const int x = x0 + (li & (DT_TW - 1)), y = y0 + li / DT_TW;
        unsigned char c = 2;  // outside the image: joins nothing
        if (x < W && y < H) {
            c = pred[n * plane_stride + (long)y * W + x] > thresh;
            bitmap[n * hw + (long)y * W + x] = c;
        }
        cls[li] = c;
        lab[li] = li;
    }
    __syncthreads();
    li32* lab3 = (li32*)lab;
    for (int li = threadIdx.x; li < DT_TPX; li += 256) {
        const int c = cls[li];
        if (c == 2) continue;
        const int lx = li & (DT_TW - 1), ly = li / DT_TW;
        if (lx > 0 && cls[li - 1] == c) uf_union<li32, __HIP_MEMORY_SCOPE_WORKGROUP>(lab3, li, li - 1);
        if (ly > 0 && cls[li - DT_TW] == c) uf_union<li32, __HIP_MEMORY_SCOPE_WORKGROUP>(lab3, li, li - DT_TW);
        if (c == 1 && ly > 0) {  // foreground: 8-connected
            if (lx > 0 && cls[li - DT_TW - 1] == 1) uf_union<li32, __HIP_MEMORY_SCOPE_WORKGROUP>(lab3, li, li - DT_TW - 1);
            if (lx < DT_TW - 1 && cls[li - DT_TW + 1] == 1) uf_union<li32, __HIP_MEMORY_SCOPE_WORKGROUP>(lab3, li, li - DT_TW + 1);
        }
    }
    __syncthreads();
    for (int li = threadIdx.x; li < DT_TPX; li += 256) {
        const int x = x0 + (li & (DT_TW - 1)), y = y0 + li / DT_TW;
        if (x >= W || y >= H) continue;
        const int r = uf_find<li32, __HIP_MEMORY_SCOPE_WORKGROUP>(lab3, li);  // the tile's local order is raster order
        L[n * hw + (long)y * W + x] = (y0 + r / DT_TW) * W + x0 + (r & (DT_TW - 1));
    }
}

// Union of every neighbour pair that crosses a tile border.  A pixel's forward neighbours are left, up (both classes),
// up-left and up-right (foreground); a pair crosses only from the left column, top row or right column of a tile.
__global__ __launch_bounds__(128) void merge_kernel(const unsigned char* __restrict__ bitmap, int H, int W, int* L) {
    constexpr int NB = DT_TH + DT_TW + DT_TH;
    const int t = threadIdx.x;
    if (t >= NB) return;
    const int n = blockIdx.z, x0 = blockIdx.x * DT_TW, y0 = blockIdx.y * DT_TH;
    const int lx = t < DT_TH ? 0 : t < DT_TH + DT_TW ? t - DT_TH : DT_TW - 1;
    const int ly = t < DT_TH ? t : t < DT_TH + DT_TW ? 0 : t - DT_TH - DT_TW;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= W || y >= H) return;
    const long hw = (long)H * W;
    const unsigned char* bm = bitmap + n * hw;
    gi32* Ln = (gi32*)(L + n * hw);
    const int p = y * W + x, c = bm[p];
    if (lx == 0 && x > 0 && bm[p - 1] == c) uf_union<gi32, __HIP_MEMORY_SCOPE_AGENT>(Ln, p, p - 1);
    if (ly == 0 && y > 0 && bm[p - W] == c) uf_union<gi32, __HIP_MEMORY_SCOPE_AGENT>(Ln, p, p - W);
    if (c == 1 && y > 0) {
        if ((lx == 0 || ly == 0) && x > 0 && bm[p - W - 1]) uf_union<gi32, __HIP_MEMORY_SCOPE_AGENT>(Ln, p, p - W - 1);
        if ((lx == DT_TW - 1 || ly == 0) && x + 1 < W && bm[p - W + 1]) uf_union<gi32, __HIP_MEMORY_SCOPE_AGENT>(Ln, p, p - W + 1);
    }
}

__global__ void flatten_kernel(const int* __restrict__ L, long hw, long total, int* __restrict__ labels, long long* __restrict__ acc,
                               int* __restrict__ edge) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long base = i / hw * hw;
        int r = (int)(i - base);
        for (int q = L[base + r]; q != r; q = L[base + r]) r = q;  // L is read-only in this launch
        labels[i] = r;
        if (base + r == i) {  // a root: clear its accumulators
            acc[3 * i] = 0; acc[3 * i + 1] = 0; acc[3 * i + 2] = 0;
            edge[i] = 0;
        }
    }
}

__device__ __forceinline__ int block_sum_256(int v, int* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void row_count_kernel(const unsigned char* __restrict__ bitmap, const int* __restrict__ labels, int H, int W,
                                                        int* __restrict__ edge, int* __restrict__ rowcnt) {
    __shared__ int red[4];
    const int n = blockIdx.y, y = blockIdx.x;
    const long hw = (long)H * W, row = n * hw + (long)y * W;
    int cnt = 0;
    for (int x = threadIdx.x; x < W; x += 256) {
        const int lab = labels[row + x];
        if (lab == y * W + x && bitmap[row + x]) ++cnt;
        if (y == 0 || y == H - 1 || x == 0 || x == W - 1) atomicOr(edge + n * hw + lab, 1);
    }
    cnt = block_sum_256(cnt, red);
    if (threadIdx.x == 0) rowcnt[(long)n * H + y] = cnt;
}

// rowoff[y] = fg roots in rows > y; counts[n] = all fg roots of the image
__global__ __launch_bounds__(256) void row_scan_kernel(const int* __restrict__ rowcnt, int H, int* __restrict__ rowoff, int* __restrict__ counts) {
    __shared__ int part[256];
    const int n = blockIdx.x, t = threadIdx.x, ch = (H + 255) / 256;
    const int* rc = rowcnt + (long)n * H;
    int* ro = rowoff + (long)n * H;
    const int lo = min(t * ch, H), hi = min(lo + ch, H);
    int s = 0;
    for (int y = lo; y < hi; ++y) s += rc[y];
    part[t] = s;
    __syncthreads();
    if (t == 0) {  // suffix sums over the 256 chunks
        int acc = 0;
        for (int k = 255; k >= 0; --k) { const int v = part[k]; part[k] = acc; acc += v; }
        counts[n] = acc;
    }
    __syncthreads();
    int acc = part[t];
    for (int y = hi - 1; y >= lo; --y) { ro[y] = acc; acc += rc[y]; }
}

__global__ __launch_bounds__(256) void rank_kernel(const unsigned char* __restrict__ bitmap, const int* __restrict__ labels, int H, int W,
                                                   const int* __restrict__ rowoff, int max_cand, int* __restrict__ slot, int* __restrict__ cand_root,
                                                   int* __restrict__ cand_box, long long* __restrict__ cand_sum) {
    __shared__ int wc[4];
    const int n = blockIdx.y, y = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long hw = (long)H * W, row = n * hw + (long)y * W;
    int running = rowoff[(long)n * H + y];
    for (int c0 = 0; c0 < W; c0 += 256) {  // columns from the right
        const int x = W - 1 - (c0 + (int)threadIdx.x);
        const bool f = x >= 0 && labels[row + x] == y * W + x && bitmap[row + x];
        const unsigned long long m = __ballot(f);
        if (lane == 0) wc[w] = __popcll(m);
        __syncthreads();
        int before = running;
        for (int k = 0; k < w; ++k) before += wc[k];
        const int rank = before + __popcll(m & ((1ull << lane) - 1));
        if (f) {
            const int s = rank < max_cand ? rank : -1;
            slot[row + x] = s;
            if (s >= 0) {
                const long k = (long)n * max_cand + s;
                cand_root[k] = y * W + x;
                cand_box[4 * k] = W; cand_box[4 * k + 1] = -1; cand_box[4 * k + 2] = y; cand_box[4 * k + 3] = y;
                cand_sum[3 * k] = 0; cand_sum[3 * k + 1] = 0; cand_sum[3 * k + 2] = 0;
            }
        }
        running += wc[0] + wc[1] + wc[2] + wc[3];
        __syncthreads();
    }
}

// fixed point of an fp32 value: v = hi * 2^-24 + lo * 2^-56 + (bits below 2^-56, dropped: exact for |v| >= 2^-33), with v
// clamped to [-127, 127].  Per pixel |hi| < 2^31 and |lo| < 2^32, so the sums over H * W <= 2^28 pixels fit in int64.
__device__ __forceinline__ void fixed_split(float v, long long& hi, long long& lo) {
    const double x = fmin(fmax((double)v, -127.0), 127.0);  // (NaN -> -127; a NaN pixel is background)
    hi = (long long)(x * 0x1p24);
    const double r = x - (double)hi * 0x1p-24;  // exact
    lo = (long long)(r * 0x1p56);
}

__global__ void run_stats_kernel(const float* __restrict__ pred, long plane_stride, const unsigned char* __restrict__ bitmap,
                                 const int* __restrict__ labels, const int* __restrict__ slot, int N, int H, int W, int max_cand,
                                 unsigned long long* __restrict__ acc, int* __restrict__ cand_box) {
    const int chunks = (W + DT_RUN - 1) / DT_RUN;
    const long total = (long)N * H * chunks, hw = (long)H * W;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % chunks);
        const long ny = i / chunks;
        const int n = (int)(ny / H), y = (int)(ny % H);
        const long row = n * hw + (long)y * W;
        const float* pr = pred + n * plane_stride + (long)y * W;
        const int xa = c * DT_RUN, xb = min(xa + DT_RUN, W);
        int cur = labels[row + xa], start = xa;
        long long shi = 0, slo = 0;
        for (int x = xa; x <= xb; ++x) {
            const int lab = x < xb ? labels[row + x] : -1;
            if (lab != cur) {  // flush the run start .. x-1 of component `cur`
                unsigned long long* a = acc + 3 * (n * hw + cur);
                atomicAdd(a, (unsigned long long)shi);
                atomicAdd(a + 1, (unsigned long long)slo);
                atomicAdd(a + 2, (unsigned long long)(x - start));
                if (bitmap[n * hw + cur]) {
                    const int s = slot[n * hw + cur];
                    if (s >= 0) {
                        int* b = cand_box + 4 * ((long)n * max_cand + s);
                        atomicMin(b, start);
                        atomicMax(b + 1, x - 1);
                        atomicMax(b + 3, y);
                    }
                }
                if (x == xb) break;
                cur = lab; start = x; shi = 0; slo = 0;
            }
            long long h, l;
            fixed_split(pr[x], h, l);
            shi += h; slo += l;
        }
    }
}

__global__ void tree_kernel(const unsigned char* __restrict__ bitmap, const int* __restrict__ labels, const int* __restrict__ edge,
                            const int* __restrict__ slot, const long long* __restrict__ acc, int W, long hw, long total, int max_cand,
                            unsigned long long* __restrict__ cand_sum) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long base = i / hw * hw;
        const int p = (int)(i - base);
        if (labels[i] != p) continue;
        const unsigned char* bm = bitmap + base;
        if (!bm[p] && edge[i]) continue;  // background reaching the edge: the outside
        const long long s0 = acc[3 * i], s1 = acc[3 * i + 1], s2 = acc[3 * i + 2];
        const long nc = base / hw * max_cand;
        for (int a = p;;) {
            if (bm[a]) {
                const int s = slot[base + a];
                if (s >= 0) {
                    unsigned long long* d = cand_sum + 3 * (nc + s);
                    atomicAdd(d, (unsigned long long)s0);
                    atomicAdd(d + 1, (unsigned long long)s1);
                    atomicAdd(d + 2, (unsigned long long)s2);
                }
            }
            if (a % W == 0) break;
            const int b = labels[base + a - 1];
            if (!bm[b] && edge[base + b]) break;
            a = b;
        }
    }
}

// ---- min-area rectangle of a convex polygon (host and device) ------------------------------------------------------
// For hull edge i (v_i -> v_i+1, e = its vector) the rectangle with a side along e spans dot(e, v) over [dmin, dmax]
// and cross(e, v) over [cmin, cmax]; its area is (dmax - dmin)(cmax - cmin) / |e|^2.  All integers.
struct EdgeRect { long long ex, ey, dmin, dmax, cmin, cmax; };

template <typename T>
__host__ __device__ inline EdgeRect edge_rect(const T* hx, const T* hy, int h, int i) {
    EdgeRect r;
    const int j = i + 1 == h ? 0 : i + 1;
    r.ex = (long long)hx[j] - hx[i]; r.ey = (long long)hy[j] - hy[i];
    if (h == 1) { r.ex = 1; r.ey = 0; }
    r.dmin = r.cmin = LLONG_MAX; r.dmax = r.cmax = LLONG_MIN;
    for (int k = 0; k < h; ++k) {
        const long long d = r.ex * hx[k] + r.ey * hy[k], c = r.ex * hy[k] - r.ey * hx[k];
        r.dmin = d < r.dmin ? d : r.dmin; r.dmax = d > r.dmax ? d : r.dmax;
        r.cmin = c < r.cmin ? c : r.cmin; r.cmax = c > r.cmax ? c : r.cmax;
    }
    return r;
}

__host__ __device__ inline unsigned __int128 rect_num(const EdgeRect& r) {
    return (unsigned __int128)(unsigned long long)(r.dmax - r.dmin) * (unsigned long long)(r.cmax - r.cmin);
}
__host__ __device__ inline unsigned long long rect_den(const EdgeRect& r) { return (unsigned long long)(r.ex * r.ex + r.ey * r.ey); }

// area(a) < area(b), exactly.  (num < 2^62, den < 2^31: the products stay below 2^93.)
__host__ __device__ inline bool rect_less(unsigned __int128 na, unsigned long long da, unsigned __int128 nb, unsigned long long db) {
    return na * db < nb * da;
}

// monotone chain over points given in (y, x) order: chain 0 keeps left turns, chain 1 right turns (cross in (x, y))
template <typename T>
__host__ __device__ inline bool chain_push(T* cx, T* cy, int& m, int cap, int x, int y, int side) {
    while (m >= 2) {
        const long long ax = cx[m - 2], ay = cy[m - 2], bx = cx[m - 1], by = cy[m - 1];
        const long long cr = (bx - ax) * ((long long)y - ay) - (by - ay) * ((long long)x - ax);
        if (side == 0 ? cr <= 0 : cr >= 0) --m;
        else break;
    }
    if (m >= cap) return false;
    cx[m] = (T)x; cy[m] = (T)y; ++m;
    return true;
}

__global__ __launch_bounds__(256) void hull_kernel(const int* __restrict__ labels, int H, int W, int max_cand, const int* __restrict__ counts,
                                                   const int* __restrict__ cand_root, const int* __restrict__ cand_box,
                                                   const long long* __restrict__ cand_sum, Rec* __restrict__ recs) {
    __shared__ short cx[2][DT_CHAIN], cy[2][DT_CHAIN];
    __shared__ short hx[2 * DT_CHAIN], hy[2 * DT_CHAIN];
    __shared__ int ext[DT_HULL_ROWS][2];
    __shared__ int chain_m[2], hull_h, overflow;
    __shared__ unsigned long long best_den[256];
    __shared__ unsigned __int128 best_num[256];
    __shared__ int best_i[256];
    const int n = blockIdx.y, s = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const long k = (long)n * max_cand + s;
    Rec* out = recs + k;
    if (s >= min(counts[n], max_cand)) {  // no candidate in this slot
        if (t == 0) *out = Rec{-1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        return;
    }
    const long hw = (long)H * W;
    const int root = cand_root[k], xmin = cand_box[4 * k], xmax = cand_box[4 * k + 1], ymin = cand_box[4 * k + 2], ymax = cand_box[4 * k + 3];
    const int* lab = labels + n * hw;
    if (t == 0) { chain_m[0] = chain_m[1] = 0; overflow = 0; }
    for (int y0 = ymin; y0 <= ymax; y0 += DT_HULL_ROWS) {
        for (int r = w; r < DT_HULL_ROWS; r += 4) {  // one wave per row: leftmost and rightmost pixel of the component
            const int y = y0 + r;
            if (y > ymax) break;
            int lo = INT_MAX, hi = -1;
            for (int x = xmin + lane; x <= xmax; x += 64)
                if (lab[(long)y * W + x] == root) { lo = min(lo, x); hi = max(hi, x); }
            for (int o = 32; o > 0; o >>= 1) { lo = min(lo, __shfl_xor(lo, o, 64)); hi = max(hi, __shfl_xor(hi, o, 64)); }
            if (lane == 0) { ext[r][0] = lo; ext[r][1] = hi; }
        }
        __syncthreads();
        if (t < 2) {  // one lane per chain; every row of a connected component has a pixel
            int m = chain_m[t];
            bool ok = true;
            for (int r = 0; r < DT_HULL_ROWS && y0 + r <= ymax; ++r) {
                ok = ok && chain_push(cx[t], cy[t], m, DT_CHAIN, ext[r][0], y0 + r, t);
                if (ext[r][1] != ext[r][0]) ok = ok && chain_push(cx[t], cy[t], m, DT_CHAIN, ext[r][1], y0 + r, t);
            }
            chain_m[t] = m;
            if (!ok) atomicOr(&overflow, 1);
        }
        __syncthreads();
    }
    if (t == 0) {  // counter-clockwise in (x, y) from the first vertex in (y, x) order: chain 0, then chain 1 backwards
        const int m0 = chain_m[0], m1 = chain_m[1];
        int h = 0;
        for (int i = 0; i < m0; ++i) { hx[h] = cx[0][i]; hy[h] = cy[0][i]; ++h; }
        for (int i = m1 - 2; i >= 1; --i) { hx[h] = cx[1][i]; hy[h] = cy[1][i]; ++h; }
        hull_h = h;
    }
    __syncthreads();
    const int h = hull_h;
    // every thread takes the first strict minimum of its own edges (i = t, t + 256, ...), then thread 0 the overall one
    int bi = -1;
    unsigned __int128 bn = 0;
    unsigned long long bd = 1;
    for (int i = t; i < h; i += 256) {
        const EdgeRect r = edge_rect(hx, hy, h, i);
        const unsigned __int128 nm = rect_num(r);
        const unsigned long long dn = rect_den(r);
        if (bi < 0 || rect_less(nm, dn, bn, bd)) { bi = i; bn = nm; bd = dn; }
    }
    best_i[t] = bi; best_num[t] = bn; best_den[t] = bd;
    __syncthreads();
    if (t == 0) {
        int i0 = -1;
        unsigned __int128 n0 = 0;
        unsigned long long d0 = 1;
        for (int u = 0; u < 256; ++u) {
            const int i = best_i[u];
            if (i < 0) continue;
            if (i0 < 0 || rect_less(best_num[u], best_den[u], n0, d0) || (!rect_less(n0, d0, best_num[u], best_den[u]) && i < i0)) {
                i0 = i; n0 = best_num[u]; d0 = best_den[u];
            }
        }
        const EdgeRect r = edge_rect(hx, hy, h, i0);
        *out = Rec{root, overflow ? -1 : h, (int)r.ex, (int)r.ey, r.dmin, r.dmax, r.cmin, r.cmax,
                   cand_sum[3 * k], cand_sum[3 * k + 1], cand_sum[3 * k + 2]};
    }
}

// ---- outer borders of the kept candidates (dbn_detect_poly) -------------------------------------------------------
// A crack is (pixel p of candidate C, side s) whose 4-neighbour across s is background or outside the image.  Sides
// L, B, R, T (s = 0..3) are walked with C on the left on screen (y down): L down, B right, R up, T left.  Cracks facing
// a hole of C (a background component X with parent(X) = C, see tree_kernel) are not enumerated, nor are the cracks of
// components past max_candidates: every enumerated crack lies on the outer-border cycle of a kept candidate, and every
// such cycle holds exactly one head, the L crack of C's first pixel.
__constant__ int PC_DX[4] = {0, 1, 0, -1}, PC_DY[4] = {1, 0, -1, 0};  // motion along L, B, R, T
__constant__ int PC_NX[4] = {-1, 0, 1, 0}, PC_NY[4] = {0, 1, 0, -1};  // toward the background across L, B, R, T
constexpr int PC_MAX_ROUNDS = 32;                                     // > log2 of the cracks of a 16384^2 image

__device__ __forceinline__ bool pc_fg(const unsigned char* bm, int H, int W, int x, int y) {
    return x >= 0 && y >= 0 && x < W && y < H && bm[(long)y * W + x];
}

// bit s set: (p, s) is an enumerated crack.  bm, lab, edge, slot: one image's planes.
__device__ __forceinline__ int pc_mask(const unsigned char* bm, const int* lab, const int* edge, const int* slot, int H, int W, int x, int y) {
    const long p = (long)y * W + x;
    if (!bm[p]) return 0;
    const int c = lab[p];
    if (slot[c] < 0) return 0;
    int m = 0;
    for (int s = 0; s < 4; ++s) {
        const int nx = x + PC_NX[s], ny = y + PC_NY[s];
        if (nx < 0 || ny < 0 || nx >= W || ny >= H) { m |= 1 << s; continue; }
        const long q = (long)ny * W + nx;
        if (bm[q]) continue;
        const int b = lab[q];
        if (!edge[b] && lab[b - 1] == c) continue;  // a hole of C (b is not in column 0: it does not touch the edge)
        m |= 1 << s;
    }
    return m;
}

// exclusive prefix of v over the 256 threads of the block; *total = the block's sum
__device__ __forceinline__ int block_scan_256(int v, int* red, int* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    __syncthreads();
    if (lane == 63) red[w] = inc;
    __syncthreads();
    int before = 0;
    for (int k = 0; k < w; ++k) before += red[k];
    *total = red[0] + red[1] + red[2] + red[3];
    return before + inc - v;
}

__global__ __launch_bounds__(256) void crack_count_kernel(const unsigned char* __restrict__ bitmap, const int* __restrict__ labels,
                                                          const int* __restrict__ edge, const int* __restrict__ slot, int H, int W,
                                                          int* __restrict__ rowcnt) {
    __shared__ int red[4];
    const int n = blockIdx.y, y = blockIdx.x;
    const long hw = (long)H * W, o = n * hw;
    int cnt = 0;
    for (int x = threadIdx.x; x < W; x += 256) cnt += __popc(pc_mask(bitmap + o, labels + o, edge + o, slot + o, H, W, x, y));
    cnt = block_sum_256(cnt, red);
    if (threadIdx.x == 0) rowcnt[(long)n * H + y] = cnt;
}

// exclusive prefix over all rows of the batch (crack ids are global); hdr[0] = total cracks; clears the round flags
__global__ __launch_bounds__(1024) void crack_scan_kernel(const int* __restrict__ rowcnt, long rows, int* __restrict__ rowbase, int* __restrict__ hdr) {
    __shared__ int part[1024];
    const int t = threadIdx.x;
    const long ch = (rows + 1023) / 1024, lo = min(t * ch, rows), hi = min(lo + ch, rows);
    int s = 0;
    for (long r = lo; r < hi; ++r) s += rowcnt[r];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        int acc = 0;
        for (int k = 0; k < 1024; ++k) { const int v = part[k]; part[k] = acc; acc += v; }
        hdr[0] = acc;
    }
    if (t < PC_MAX_ROUNDS) hdr[1 + t] = 0;
    __syncthreads();
    int acc = part[t];
    for (long r = lo; r < hi; ++r) { rowbase[r] = acc; acc += rowcnt[r]; }
}

// per pixel: its crack mask and the id of its first crack (row base + prefix in the row, left to right)
__global__ __launch_bounds__(256) void crack_emit_kernel(const unsigned char* __restrict__ bitmap, const int* __restrict__ labels,
                                                         const int* __restrict__ edge, const int* __restrict__ slot, int H, int W,
                                                         const int* __restrict__ rowbase, unsigned char* __restrict__ mask, int* __restrict__ pxbase) {
    __shared__ int red[4];
    const int n = blockIdx.y, y = blockIdx.x;
    const long hw = (long)H * W, o = n * hw, row = o + (long)y * W;
    int base = rowbase[(long)n * H + y];
    for (int x0 = 0; x0 < W; x0 += 256) {
        const int x = x0 + (int)threadIdx.x;
        const int m = x < W ? pc_mask(bitmap + o, labels + o, edge + o, slot + o, H, W, x, y) : 0;
        int tot;
        const int pre = block_scan_256(__popc(m), red, &tot);
        if (x < W) { mask[row + x] = (unsigned char)m; pxbase[row + x] = base + pre; }
        base += tot;
    }
}

__device__ __forceinline__ int pc_id(const unsigned char* mask, const int* pxbase, long p, int s) {
    return pxbase[p] + __popc(mask[p] & ((1 << s) - 1));
}

// per crack: successor (the 8-connected turning rule), key p * 4 + s, candidate n * M + slot, head flag; the successor
// learns its predecessor's pixel
__global__ __launch_bounds__(256) void crack_link_kernel(const unsigned char* __restrict__ bitmap, const int* __restrict__ labels,
                                                         const int* __restrict__ slot, int H, int W, int max_cand,
                                                         const unsigned char* __restrict__ mask, const int* __restrict__ pxbase,
                                                         int* __restrict__ succ, int* __restrict__ ckey, int* __restrict__ ccand,
                                                         int* __restrict__ prevpix, unsigned char* __restrict__ wflag) {
    const int n = blockIdx.y, y = blockIdx.x;
    const long hw = (long)H * W, o = n * hw;
    const unsigned char* bm = bitmap + o;
    for (int x = threadIdx.x; x < W; x += 256) {
        const long p = (long)y * W + x;
        const int m = mask[o + p];
        if (!m) continue;
        const int c = labels[o + p];
        const int cand = (int)((long)n * max_cand + slot[o + c]);
        for (int s = 0; s < 4; ++s) {
            if (!((m >> s) & 1)) continue;
            const int id = pc_id(mask, pxbase, o + p, s);
            const int ax = x + PC_DX[s], ay = y + PC_DY[s], gx = ax + PC_NX[s], gy = ay + PC_NY[s];
            int qx = x, qy = y, qs = (s + 1) & 3;
            if (pc_fg(bm, H, W, gx, gy)) { qx = gx; qy = gy; qs = (s + 3) & 3; }
            else if (pc_fg(bm, H, W, ax, ay)) { qx = ax; qy = ay; qs = s; }
            const long q = (long)qy * W + qx;
            int nx = id;  // (cannot happen: the successor is an enumerated crack of the same cycle)
            if ((mask[o + q] >> qs) & 1) {
                nx = pc_id(mask, pxbase, o + q, qs);
                prevpix[nx] = (int)p;
            }
            succ[id] = nx;
            ckey[id] = (int)(p * 4 + s);
            ccand[id] = cand;
            wflag[id] = (s == 0 && c == (int)p) ? 2 : 0;  // bit 1: the head of the cycle
        }
    }
}

// weight = 1 where a compressed vertex starts: the first crack of a pixel visit whose arrival and departure steps
// differ.  Initialises the ranking: head -> itself with weight 0 (the terminal), any other crack -> its successor.
__global__ void crack_weight_kernel(const int* __restrict__ hdr, int W, const int* __restrict__ succ, const int* __restrict__ ckey,
                                    const int* __restrict__ prevpix, unsigned char* __restrict__ wflag, int* __restrict__ nA, int* __restrict__ dA) {
    const long total = hdr[0];
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int p = ckey[i] >> 2, pp = prevpix[i];
        int kept = 0;
        if (pp != p) {  // a visit starts here: leave the pixel (at most 4 cracks of one pixel in a row)
            int j = (int)i, q = p;
            for (int k = 0; k < 4; ++k) {
                j = succ[j];
                q = ckey[j] >> 2;
                if (q != p) break;
            }
            const int px = p % W, py = p / W;
            const int adx = px - pp % W, ady = py - pp / W, ddx = q % W - px, ddy = q / W - py;
            kept = (adx != ddx || ady != ddy) ? 1 : 0;
        }
        const int head = wflag[i] & 2;
        wflag[i] = (unsigned char)(head | kept);
        nA[i] = head ? (int)i : succ[i];
        dA[i] = head ? 0 : kept;
    }
}

// one round of Wyllie's pointer jumping: d += d[next], next = next[next].  flags[r] = something changed; a round after
// one that changed nothing returns at once.
__global__ void crack_jump_kernel(const int* __restrict__ hdr, int r, const int* __restrict__ sn, const int* __restrict__ sd,
                                  int* __restrict__ dn, int* __restrict__ dd, int* __restrict__ flags) {
    if (r > 0 && flags[r - 1] == 0) return;
    const long total = hdr[0];
    bool changed = false;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int nx = sn[i];
        const int nn = sn[nx];
        dd[i] = sd[i] + sd[nx];
        dn[i] = nn;
        changed |= nn != nx;
    }
    if (__ballot(changed) && (threadIdx.x & 63) == 0) atomicOr(flags + r, 1);
}

// rounds run: round 0 always, round r when round r - 1 changed something
__device__ __forceinline__ int pc_rounds(const int* flags, int R) {
    int e = 1;
    while (e < R && flags[e - 1]) ++e;
    return e;
}

// per candidate slot: compressed vertices K = weight from the head's successor to the head (1 for a single pixel, whose
// only visit has no start), offsets (exclusive prefix over the batch); a single pixel writes its vertex here
__global__ __launch_bounds__(1024) void cand_verts_kernel(const Rec* __restrict__ recs, long slots, int W, long hw, int max_cand,
                                                          const int* __restrict__ hdr, int R, const unsigned char* __restrict__ mask,
                                                          const int* __restrict__ pxbase, const int* __restrict__ succ,
                                                          const int* __restrict__ dA, const int* __restrict__ dB, int* __restrict__ nv,
                                                          int* __restrict__ voff, int* __restrict__ info, short* __restrict__ verts) {
    __shared__ int part[1024];
    const int t = threadIdx.x;
    const int E = pc_rounds(hdr + 1, R);
    const int* d = (E - 1) % 2 == 0 ? dB : dA;
    const long ch = (slots + 1023) / 1024, lo = min(t * ch, slots), hi = min(lo + ch, slots);
    int s = 0;
    for (long k = lo; k < hi; ++k) {
        int K = 0;
        const int root = recs[k].root;
        if (root >= 0) {
            const long o = k / max_cand * hw;
            const int head = pc_id(mask, pxbase, o + root, 0);
            K = max(d[succ[head]], 1);
        }
        nv[k] = K;
        s += K;
    }
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        int acc = 0;
        for (int k = 0; k < 1024; ++k) { const int v = part[k]; part[k] = acc; acc += v; }
        info[0] = acc;        // packed vertices
        info[1] = hdr[0];     // cracks
        info[2] = E;          // rounds run
        info[3] = R;          // rounds launched
    }
    __syncthreads();
    int acc = part[t];
    for (long k = lo; k < hi; ++k) {
        voff[k] = acc;
        const int root = recs[k].root;
        if (root >= 0) {
            const long o = k / max_cand * hw;
            const int head = pc_id(mask, pxbase, o + root, 0);
            if (d[succ[head]] == 0) { verts[2L * acc] = (short)(root % W); verts[2L * acc + 1] = (short)(root / W); }
        }
        acc += nv[k];
    }
}

// every kept vertex to its place: index (K - d + 1) mod K, d = weight from it to the head (the start pixel's vertex,
// the last in rank order, is index 0)
__global__ void crack_out_kernel(const int* __restrict__ hdr, int R, int W, const int* __restrict__ ckey, const int* __restrict__ ccand,
                                 const unsigned char* __restrict__ wflag, const int* __restrict__ dA, const int* __restrict__ dB,
                                 const int* __restrict__ nv, const int* __restrict__ voff, short* __restrict__ verts) {
    const long total = hdr[0];
    const int E = pc_rounds(hdr + 1, R);
    const int* d = (E - 1) % 2 == 0 ? dB : dA;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        if (!(wflag[i] & 1)) continue;
        const int c = ccand[i], K = nv[c], di = d[i];
        if (di < 1 || di > K) continue;  // (cannot happen: 1 <= d <= K for a kept vertex)
        const int idx = (K - di + 1) % K, p = ckey[i] >> 2;
        const long at = 2L * ((long)voff[c] + idx);
        verts[at] = (short)(p % W);
        verts[at + 1] = (short)(p / W);
    }
}

// ---- host stage ----------------------------------------------------------------------------------------------------
struct Corners { float x[4], y[4]; };

// corners (dmin, cmin), (dmax, cmin), (dmax, cmax), (dmin, cmax): v = (d e + c (-ey, ex)) / |e|^2, fp64 rounded to fp32
Corners rect_corners(const EdgeRect& r, double* side_min) {
    const double ex = (double)r.ex, ey = (double)r.ey, E = ex * ex + ey * ey;
    const double d[4] = {(double)r.dmin, (double)r.dmax, (double)r.dmax, (double)r.dmin};
    const double c[4] = {(double)r.cmin, (double)r.cmin, (double)r.cmax, (double)r.cmax};
    Corners q;
    for (int i = 0; i < 4; ++i) {
        q.x[i] = (float)((d[i] * ex - c[i] * ey) / E);
        q.y[i] = (float)((d[i] * ey + c[i] * ex) / E);
    }
    const double se = sqrt(E), w = (double)(r.dmax - r.dmin) / se, hgt = (double)(r.cmax - r.cmin) / se;
    *side_min = w < hgt ? w : hgt;
    return q;
}

// get_mini_boxes' order: stable sort on x, then (left pair) the larger y last, (right pair) the smaller y first
Corners mini_box_order(const Corners& q) {
    int idx[4] = {0, 1, 2, 3};
    std::stable_sort(idx, idx + 4, [&](int a, int b) { return q.x[a] < q.x[b]; });
    int i1, i2, i3, i4;
    if (q.y[idx[1]] > q.y[idx[0]]) { i1 = idx[0]; i4 = idx[1]; } else { i1 = idx[1]; i4 = idx[0]; }
    if (q.y[idx[3]] > q.y[idx[2]]) { i2 = idx[2]; i3 = idx[3]; } else { i2 = idx[3]; i3 = idx[2]; }
    const int o[4] = {i1, i2, i3, i4};
    Corners r;
    for (int i = 0; i < 4; ++i) { r.x[i] = q.x[o[i]]; r.y[i] = q.y[o[i]]; }
    return r;
}

// shapely Polygon(box).area / .length (GEOS Area::ofRing, Length::ofLine), as gt_maps._area / _length
double ring_area(const double* x, const double* y, int n) {
    double s = 0.0;
    for (int i = 1; i < n; ++i) s += (x[i] - x[0]) * (y[i - 1] - y[i + 1 == n ? 0 : i + 1]);
    return fabs(s / 2.0);
}
double ring_length(const double* x, const double* y, int n) {
    double s = 0.0;
    for (int i = 1; i <= n; ++i) {
        const double dx = x[i % n] - x[i - 1], dy = y[i % n] - y[i - 1];
        s += sqrt(dx * dx + dy * dy);
    }
    return s;
}

// min-area rectangle of integer points: hull by the same monotone chain as the device, same edge rule
EdgeRect min_area_rect(std::vector<std::pair<long long, long long>> pts) {  // (y, x)
    std::sort(pts.begin(), pts.end());
    pts.erase(std::unique(pts.begin(), pts.end()), pts.end());
    const int cap = (int)pts.size() + 1;
    std::vector<long long> cx[2], cy[2];
    int m[2] = {0, 0};
    for (int sd = 0; sd < 2; ++sd) {
        cx[sd].resize(cap); cy[sd].resize(cap);
        for (const auto& p : pts) chain_push(cx[sd].data(), cy[sd].data(), m[sd], cap, (int)p.second, (int)p.first, sd);
    }
    std::vector<long long> hx, hy;
    for (int i = 0; i < m[0]; ++i) { hx.push_back(cx[0][i]); hy.push_back(cy[0][i]); }
    for (int i = m[1] - 2; i >= 1; --i) { hx.push_back(cx[1][i]); hy.push_back(cy[1][i]); }
    const int h = (int)hx.size();
    EdgeRect best = edge_rect(hx.data(), hy.data(), h, 0);
    for (int i = 1; i < h; ++i) {
        const EdgeRect r = edge_rect(hx.data(), hy.data(), h, i);
        if (rect_less(rect_num(r), rect_den(r), rect_num(best), rect_den(best))) best = r;
    }
    return best;
}

// mean of the fixed-point sum (hi * 2^-24 + lo * 2^-56) / count, rounded once to fp32
float fixed_mean(long long hi, long long lo, long long count) {
    if (count <= 0) return 0.f;
    const __int128 T = (__int128)hi * ((__int128)1 << 32) + lo;
    if (T == 0) return 0.f;
    const bool neg = T < 0;
    const unsigned __int128 A = neg ? (unsigned __int128)(-T) : (unsigned __int128)T;
    int top = 127;
    while (!((A >> top) & 1)) --top;
    const int sh = 125 - top;  // A << sh in [2^125, 2^126): the quotient keeps >= 100 bits, so bit 0 can be the sticky bit
    const unsigned __int128 num = A << sh;
    const unsigned __int128 q = num / (unsigned __int128)count, rem = num % (unsigned __int128)count;
    const float f = (float)(q | (rem != 0 ? 1 : 0));
    const float v = ldexpf(f, -(56 + sh));
    return neg ? -v : v;
}

// the same mean rounded once to fp64 (the polygon path's score: cv2.mean returns a double)
double fixed_mean64(long long hi, long long lo, long long count) {
    if (count <= 0) return 0.0;
    const __int128 T = (__int128)hi * ((__int128)1 << 32) + lo;
    if (T == 0) return 0.0;
    const bool neg = T < 0;
    const unsigned __int128 A = neg ? (unsigned __int128)(-T) : (unsigned __int128)T;
    int top = 127;
    while (!((A >> top) & 1)) --top;
    const int sh = 125 - top;  // the quotient keeps >= 97 bits: bit 0 as the sticky bit rounds once
    const unsigned __int128 num = A << sh;
    const unsigned __int128 q = num / (unsigned __int128)count, rem = num % (unsigned __int128)count;
    const double f = (double)(q | (rem != 0 ? 1 : 0));
    const double v = ldexp(f, -(56 + sh));
    return neg ? -v : v;
}

struct IP { int x, y; };

// approxPolyDP(src, eps, closed) as OpenCV 4.x approx.cpp reads: squared eps; the initial split from three passes of
// "farthest point from the last one" (first strict maximum); a stack of slices, each accepted (its start point
// written) when max |cross|^2 <= eps^2 |d|^2, else split at the first strict maximum (right half pushed first); then
// one in-place clean-up pass.  All coordinates are integers, so every product below is exact in fp64.
std::vector<IP> approx_poly_dp(const std::vector<IP>& src, double eps) {
    const int count = (int)src.size();
    std::vector<IP> dst;
    if (count == 0) return dst;
    eps *= eps;
    int pos = 0, rs = 0;
    bool le_eps = false;
    for (int it = 0; it < 3; ++it) {
        pos = (pos + rs) % count;
        const IP st = src[pos];
        double max_dist = 0;
        for (int j = 1; j < count; ++j) {
            const IP pt = src[(pos + j) % count];
            const double dx = pt.x - st.x, dy = pt.y - st.y, d = dx * dx + dy * dy;
            if (d > max_dist) { max_dist = d; rs = j; }
        }
        le_eps = max_dist <= eps;
    }
    std::vector<std::pair<int, int>> stack;
    if (!le_eps) {
        const int s0 = pos % count, e0 = (rs + s0) % count;
        stack.push_back({e0, s0});
        stack.push_back({s0, e0});
    } else {
        dst.push_back(src[pos]);
    }
    while (!stack.empty()) {
        const int a = stack.back().first, e = stack.back().second;
        stack.pop_back();
        const IP ep = src[e], sp = src[a];
        int p = (a + 1) % count, split = -1;
        bool le = true;
        if (p != e) {
            const double dx = ep.x - sp.x, dy = ep.y - sp.y;
            double max_dist = 0;
            while (p != e) {
                const IP pt = src[p];
                const double d = fabs((pt.y - sp.y) * dx - (pt.x - sp.x) * dy);
                if (d > max_dist) { max_dist = d; split = p; }
                p = (p + 1) % count;
            }
            le = max_dist * max_dist <= eps * (dx * dx + dy * dy);
        }
        if (le) dst.push_back(sp);
        else { stack.push_back({split, e}); stack.push_back({a, split}); }
    }
    // clean-up: drop a point on an [almost] straight line between its neighbours (reads may see the pass's own writes)
    const int cnt = (int)dst.size();
    int new_count = cnt, rpos = cnt - 1;
    auto rd = [&]() { const IP v = dst[rpos]; if (++rpos >= cnt) rpos = 0; return v; };
    IP start = rd();
    int wpos = rpos;
    IP pt = rd();
    for (int i = 0; i < cnt && new_count > 2; ++i) {
        const IP end = rd();
        const double dx = end.x - start.x, dy = end.y - start.y;
        const double dist = fabs((pt.x - start.x) * dy - (pt.y - start.y) * dx);
        const double inner = (double)(pt.x - start.x) * (end.x - pt.x) + (double)(pt.y - start.y) * (end.y - pt.y);
        if (dist * dist <= 0.5 * eps * (dx * dx + dy * dy) && dx != 0 && dy != 0 && inner >= 0) {
            --new_count;
            dst[wpos] = start = end;
            if (++wpos >= cnt) wpos = 0;
            pt = rd();
            ++i;
            continue;
        }
        dst[wpos] = start = pt;
        if (++wpos >= cnt) wpos = 0;
        pt = end;
    }
    dst.resize(new_count);
    return dst;
}

}  // namespace

extern "C" {

long dbn_detect_ws_bytes(int N, int H, int W, int max_candidates) {
    if (N <= 0 || H <= 0 || W <= 0 || max_candidates <= 0) return -1;
    const long px = (long)N * H * W, c = (long)N * max_candidates;
    // L, bitmap, acc, edge, slot | rowcnt, rowoff | cand_root, cand_box, cand_sum   (each part 256-byte aligned)
    auto al = [](long b) { return (b + 255) / 256 * 256; };
    return al(4 * px) + al(px) + al(24 * px) + al(4 * px) + al(4 * px) + 2 * al(4L * N * H) + al(4 * c) + al(16 * c) + al(24 * c);
}

int dbn_detect(const float* pred, int N, int channels, int H, int W, float thresh, int max_candidates, void* ws, int* labels,
               void* recs, int* counts, void* stream) {
    DBN_REQUIRE(pred && ws && labels && recs && counts && N > 0 && N <= 65535 && channels > 0);
    DBN_REQUIRE(H > 0 && W > 0 && H <= DT_MAX_SIDE && W <= DT_MAX_SIDE && max_candidates > 0 && max_candidates <= (1 << 20));
    const hipStream_t st = (hipStream_t)stream;
    const long hw = (long)H * W, px = (long)N * hw, c = (long)N * max_candidates, plane = (long)channels * hw;
    auto al = [](long b) { return (b + 255) / 256 * 256; };
    char* p = (char*)ws;
    int* L = (int*)p; p += al(4 * px);
    unsigned char* bitmap = (unsigned char*)p; p += al(px);
    long long* acc = (long long*)p; p += al(24 * px);
    int* edge = (int*)p; p += al(4 * px);
    int* slot = (int*)p; p += al(4 * px);
    int* rowcnt = (int*)p; p += al(4L * N * H);
    int* rowoff = (int*)p; p += al(4L * N * H);
    int* cand_root = (int*)p; p += al(4 * c);
    int* cand_box = (int*)p; p += al(16 * c);
    long long* cand_sum = (long long*)p;
    const dim3 tiles(dbn_ceil_div(W, DT_TW), dbn_ceil_div(H, DT_TH), N);
    hipLaunchKernelGGL(tile_label_kernel, tiles, dim3(256), 0, st, pred, plane, H, W, thresh, bitmap, L);
    hipLaunchKernelGGL(merge_kernel, tiles, dim3(128), 0, st, bitmap, H, W, L);
    hipLaunchKernelGGL(flatten_kernel, dim3(dbn_grid(px, 256, 8192)), dim3(256), 0, st, L, hw, px, labels, acc, edge);
    hipLaunchKernelGGL(row_count_kernel, dim3(H, N), dim3(256), 0, st, bitmap, labels, H, W, edge, rowcnt);
    hipLaunchKernelGGL(row_scan_kernel, dim3(N), dim3(256), 0, st, rowcnt, H, rowoff, counts);
    hipLaunchKernelGGL(rank_kernel, dim3(H, N), dim3(256), 0, st, bitmap, labels, H, W, rowoff, max_candidates, slot, cand_root, cand_box,
                       cand_sum);
    const long runs = (long)N * H * dbn_ceil_div(W, DT_RUN);
    hipLaunchKernelGGL(run_stats_kernel, dim3(dbn_grid(runs, 256, 8192)), dim3(256), 0, st, pred, plane, bitmap, labels, slot, N, H, W,
                       max_candidates, (unsigned long long*)acc, cand_box);
    hipLaunchKernelGGL(tree_kernel, dim3(dbn_grid(px, 256, 8192)), dim3(256), 0, st, bitmap, labels, edge, slot, acc, W, hw, px,
                       max_candidates, (unsigned long long*)cand_sum);
    hipLaunchKernelGGL(hull_kernel, dim3(max_candidates, N), dim3(256), 0, st, labels, H, W, max_candidates, counts, cand_root, cand_box,
                       cand_sum, (Rec*)recs);
    return dbn_status();
}

int dbn_detect_host(const void* recs, const int* counts, int N, int max_candidates, int H, int W, const double* params, const int* dest_hw,
                    short* boxes, float* scores, float* info) {
    DBN_REQUIRE(recs && counts && params && dest_hw && boxes && scores && N > 0 && max_candidates > 0 && H > 0 && W > 0);
    const double box_thresh = params[0], unclip_ratio = params[1];
    const Rec* R = (const Rec*)recs;
    std::vector<int> off(4096);
    for (int n = 0; n < N; ++n) {
        DBN_REQUIRE(counts[n] >= 0 && dest_hw[2 * n] >= 0 && dest_hw[2 * n + 1] >= 0 && dest_hw[2 * n] <= 32767 && dest_hw[2 * n + 1] <= 32767);
        const int K = std::min(counts[n], max_candidates);
        const float dw = (float)dest_hw[2 * n + 1], dh = (float)dest_hw[2 * n];
        for (int k = 0; k < K; ++k) {
            const long o = (long)n * max_candidates + k;
            const Rec& r = R[o];
            short* bx = boxes + 8 * o;
            for (int i = 0; i < 8; ++i) bx[i] = 0;
            scores[o] = 0.f;
            DBN_REQUIRE(r.hull_n > 0);  // -1: the hull outgrew its chain buffer (cannot happen for H, W <= 16384)
            double sside;
            const Corners r1 = rect_corners(EdgeRect{r.ex, r.ey, r.dmin, r.dmax, r.cmin, r.cmax}, &sside);
            const float score = fixed_mean(r.sum_hi, r.sum_lo, r.count);
            if (info) {
                float* f = info + 10 * o;
                for (int i = 0; i < 4; ++i) { f[2 * i] = r1.x[i]; f[2 * i + 1] = r1.y[i]; }
                f[8] = (float)sside;
                f[9] = score;
            }
            if (sside < 3) continue;
            if (box_thresh > (double)score) continue;
            const Corners p = mini_box_order(r1);
            double xs[4], ys[4], xy[8];
            for (int i = 0; i < 4; ++i) { xs[i] = p.x[i]; ys[i] = p.y[i]; xy[2 * i] = xs[i]; xy[2 * i + 1] = ys[i]; }
            const double distance = ring_area(xs, ys, 4) * unclip_ratio / ring_length(xs, ys, 4);
            int cnt = 0;
            int rc = dbn_poly_offset(xy, 4, &distance, off.data(), (int)off.size() / 2, &cnt);
            if (rc != DBN_OK && cnt > (int)off.size() / 2) {
                off.resize(2 * (size_t)cnt);
                rc = dbn_poly_offset(xy, 4, &distance, off.data(), cnt, &cnt);
            }
            if (rc != DBN_OK) return rc;
            if (cnt == 0) continue;
            std::vector<std::pair<long long, long long>> pts(cnt);
            for (int i = 0; i < cnt; ++i) pts[i] = {off[2 * i + 1], off[2 * i]};
            double sside2;
            const Corners r2 = mini_box_order(rect_corners(min_area_rect(pts), &sside2));
            if (sside2 < 5) continue;
            for (int i = 0; i < 4; ++i) {  // np.clip(np.round(v / size * dest), 0, dest) in fp32, then int16
                float vx = rintf(r2.x[i] / (float)W * dw), vy = rintf(r2.y[i] / (float)H * dh);
                vx = vx < 0.f ? 0.f : vx > dw ? dw : vx;
                vy = vy < 0.f ? 0.f : vy > dh ? dh : vy;
                bx[2 * i] = (short)vx;
                bx[2 * i + 1] = (short)vy;
            }
            scores[o] = score;
        }
    }
    return DBN_OK;
}

// ---- polygons ------------------------------------------------------------------------------------------------------
// contour workspace: per pixel mask (1 B) + first crack id (4 B); per crack slot (N (2HW + H + W), every unit edge of
// the pixel grid) succ, key, candidate, predecessor pixel, 2 x (next, weight) (4 B each) + flags (1 B); rows; header
static long pc_cracks(int N, int H, int W) { return (long)N * (2L * H * W + H + W); }

long dbn_detect_poly_ws_bytes(int N, int H, int W, int max_candidates) {
    if (N <= 0 || H <= 0 || W <= 0 || max_candidates <= 0) return -1;
    const long px = (long)N * H * W, B = pc_cracks(N, H, W);
    auto al = [](long b) { return (b + 255) / 256 * 256; };
    return al(px) + al(4 * px) + 2 * al(4L * N * H) + al(4 * (1 + PC_MAX_ROUNDS)) + 8 * al(4 * B) + al(B);
}

long dbn_detect_poly_verts_cap(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return -1;
    return pc_cracks(N, H, W);
}

int dbn_detect_poly(const float* pred, int N, int channels, int H, int W, float thresh, int max_candidates, void* ws, void* poly_ws,
                    int* labels, void* table, short* verts, void* stream) {
    DBN_REQUIRE(poly_ws && table && verts);
    DBN_REQUIRE(pc_cracks(N, H, W) < (1L << 31) && (long)N * max_candidates < (1L << 31));
    const int rc = dbn_detect(pred, N, channels, H, W, thresh, max_candidates, ws, labels, table, (int*)((char*)table + 72L * N * max_candidates),
                              stream);
    if (rc != DBN_OK) return rc;
    const hipStream_t st = (hipStream_t)stream;
    const long hw = (long)H * W, px = (long)N * hw, c = (long)N * max_candidates, B = pc_cracks(N, H, W);
    auto al = [](long b) { return (b + 255) / 256 * 256; };
    // dbn_detect's workspace: L, bitmap, acc, edge, slot (its layout)
    char* q = (char*)ws;
    q += al(4 * px);
    const unsigned char* bitmap = (const unsigned char*)q; q += al(px);
    q += al(24 * px);
    const int* edge = (const int*)q; q += al(4 * px);
    const int* slot = (const int*)q;
    char* p = (char*)poly_ws;
    unsigned char* mask = (unsigned char*)p; p += al(px);
    int* pxbase = (int*)p; p += al(4 * px);
    int* rowcnt = (int*)p; p += al(4L * N * H);
    int* rowbase = (int*)p; p += al(4L * N * H);
    int* hdr = (int*)p; p += al(4 * (1 + PC_MAX_ROUNDS));
    int* succ = (int*)p; p += al(4 * B);
    int* ckey = (int*)p; p += al(4 * B);
    int* ccand = (int*)p; p += al(4 * B);
    int* prevpix = (int*)p; p += al(4 * B);
    int* nA = (int*)p; p += al(4 * B);
    int* dA = (int*)p; p += al(4 * B);
    int* nB = (int*)p; p += al(4 * B);
    int* dB = (int*)p; p += al(4 * B);
    unsigned char* wflag = (unsigned char*)p;
    // table: recs [c] | counts [N] | nv [c] | voff [c] | info [4]
    int* nv = (int*)((char*)table + 72L * c + 4L * N);
    int* voff = nv + c;
    int* info = voff + c;
    const Rec* recs = (const Rec*)table;
    int R = 1;  // rounds: 2^R >= the cracks of one image >= the longest cycle
    while ((1L << R) < B / N && R < PC_MAX_ROUNDS) ++R;
    const int G = dbn_grid(B, 256, 8192);
    hipLaunchKernelGGL(crack_count_kernel, dim3(H, N), dim3(256), 0, st, bitmap, labels, edge, slot, H, W, rowcnt);
    hipLaunchKernelGGL(crack_scan_kernel, dim3(1), dim3(1024), 0, st, rowcnt, (long)N * H, rowbase, hdr);
    hipLaunchKernelGGL(crack_emit_kernel, dim3(H, N), dim3(256), 0, st, bitmap, labels, edge, slot, H, W, rowbase, mask, pxbase);
    hipLaunchKernelGGL(crack_link_kernel, dim3(H, N), dim3(256), 0, st, bitmap, labels, slot, H, W, max_candidates, mask, pxbase, succ, ckey,
                       ccand, prevpix, wflag);
    hipLaunchKernelGGL(crack_weight_kernel, dim3(G), dim3(256), 0, st, hdr, W, succ, ckey, prevpix, wflag, nA, dA);
    for (int r = 0; r < R; ++r) {
        const bool ev = r % 2 == 0;
        hipLaunchKernelGGL(crack_jump_kernel, dim3(G), dim3(256), 0, st, hdr, r, ev ? nA : nB, ev ? dA : dB, ev ? nB : nA, ev ? dB : dA, hdr + 1);
    }
    hipLaunchKernelGGL(cand_verts_kernel, dim3(1), dim3(1024), 0, st, recs, c, W, hw, max_candidates, hdr, R, mask, pxbase, succ, dA, dB, nv,
                       voff, info, verts);
    hipLaunchKernelGGL(crack_out_kernel, dim3(G), dim3(256), 0, st, hdr, R, W, ckey, ccand, wflag, dA, dB, nv, voff, verts);
    return dbn_status();
}

int dbn_detect_poly_host(const void* recs, const int* counts, const int* nv, const int* voff, const short* verts, int N, int max_candidates,
                         int H, int W, const double* params, const int* dest_hw, int* poly_n, int* poly_off, int* poly_xy, int poly_cap,
                         int* poly_total, double* scores, double* info, int* approx_xy) {
    DBN_REQUIRE(recs && counts && nv && voff && verts && params && dest_hw && poly_n && poly_off && poly_total && scores);
    DBN_REQUIRE(N > 0 && max_candidates > 0 && H > 0 && W > 0 && poly_cap >= 0 && (poly_cap == 0 || poly_xy));
    const double box_thresh = params[0], unclip_ratio = params[1];
    const Rec* R = (const Rec*)recs;
    std::vector<int> off(4096);
    long total = 0;
    for (int n = 0; n < N; ++n) {
        DBN_REQUIRE(counts[n] >= 0 && dest_hw[2 * n] >= 0 && dest_hw[2 * n + 1] >= 0);
        const int K = std::min(counts[n], max_candidates);
        const double dw = (double)dest_hw[2 * n + 1], dh = (double)dest_hw[2 * n];
        for (int k = 0; k < max_candidates; ++k) {
            const long o = (long)n * max_candidates + k;
            poly_n[o] = 0;
            poly_off[o] = (int)std::min(total, (long)INT_MAX);
            scores[o] = 0.0;
            if (info) { info[4 * o] = 0; info[4 * o + 1] = 0; info[4 * o + 2] = 0; info[4 * o + 3] = -1; }
            if (k >= K) continue;
            const Rec& r = R[o];
            const int nc = nv[o];
            DBN_REQUIRE(nc >= 1 && voff[o] >= 0);
            const short* cv = verts + 2L * voff[o];
            std::vector<IP> c(nc);
            long a = 0, b = 0;  // axis and diagonal steps: cv2.arcLength without its summation order
            for (int i = 0; i < nc; ++i) {
                c[i] = {cv[2 * i], cv[2 * i + 1]};
                const int j = i + 1 == nc ? 0 : i + 1;
                const int dx = abs(cv[2 * j] - cv[2 * i]), dy = abs(cv[2 * j + 1] - cv[2 * i + 1]);
                if (dx == 0 || dy == 0) a += dx + dy;
                else b += dx;
            }
            const double len = (double)a + (double)b * sqrt(2.0);
            const std::vector<IP> ap = approx_poly_dp(c, 0.005 * len);
            const double score = fixed_mean64(r.sum_hi, r.sum_lo, r.count);
            if (info) { info[4 * o] = score; info[4 * o + 1] = (double)ap.size(); }
            if (approx_xy)
                for (size_t i = 0; i < ap.size(); ++i) { approx_xy[2 * (voff[o] + i)] = ap[i].x; approx_xy[2 * (voff[o] + i) + 1] = ap[i].y; }
            if (ap.size() < 4) continue;
            if (box_thresh > score) continue;
            const int m = (int)ap.size();
            std::vector<double> xs(m), ys(m), xy(2 * m);
            for (int i = 0; i < m; ++i) { xs[i] = ap[i].x; ys[i] = ap[i].y; xy[2 * i] = xs[i]; xy[2 * i + 1] = ys[i]; }
            const double distance = ring_area(xs.data(), ys.data(), m) * unclip_ratio / ring_length(xs.data(), ys.data(), m);
            int cnt = 0, paths = 0;
            int rc = dbn_poly_offset_paths(xy.data(), m, &distance, off.data(), (int)off.size() / 2, &cnt, &paths);
            if (rc != DBN_OK && cnt > (int)off.size() / 2) {
                off.resize(2 * (size_t)cnt);
                rc = dbn_poly_offset_paths(xy.data(), m, &distance, off.data(), cnt, &cnt, &paths);
            }
            if (rc != DBN_OK) return rc;
            if (info) info[4 * o + 2] = paths;
            if (paths > 1) continue;  // the reference skips an offset of several paths (pieces or holes)
            double sside = -1;  // get_mini_boxes of an empty path
            if (cnt > 0) {
                std::vector<std::pair<long long, long long>> pts(cnt);
                for (int i = 0; i < cnt; ++i) pts[i] = {off[2 * i + 1], off[2 * i]};
                rect_corners(min_area_rect(pts), &sside);
            }
            if (info) info[4 * o + 3] = sside;
            if (sside < 5) continue;
            poly_n[o] = cnt;
            for (int i = 0; i < cnt; ++i, ++total) {  // np.clip(np.round(v / size * dest), 0, dest) in fp64 on int64
                if (total >= poly_cap) continue;
                double vx = rint((double)off[2 * i] / (double)W * dw), vy = rint((double)off[2 * i + 1] / (double)H * dh);
                vx = vx < 0 ? 0 : vx > dw ? dw : vx;
                vy = vy < 0 ? 0 : vy > dh ? dh : vy;
                poly_xy[2 * total] = (int)vx;
                poly_xy[2 * total + 1] = (int)vy;
            }
            scores[o] = score;
        }
    }
    DBN_REQUIRE(total < INT_MAX);
    *poly_total = (int)total;
    return total > poly_cap ? DBN_ERR_ARG : DBN_OK;
}

}  // extern "C"
