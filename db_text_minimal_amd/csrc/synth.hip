// Synthetic scene text on a packed uint8 RGB batch (db_text_minimal_amd/synth.py; ABI and the records: include/dbnet_hip.h; the definition:
// DESIGN.md section 41): a background (procedural value noise of three octaves, or the caller's packed images) and over it glyph instances
// under any affine map, anti-aliased by 16 samples per pixel, all in exact integers, in one launch.  A workgroup owns one tile of SY_TILE x
// SY_TILE pixels of the host-built list, a lane four neighbouring pixels of one row of it:
//   (1) the background of the lane's pixels: 12 bytes of `bg`, or the noise from the tile's 94 lattice values (one Philox block each, staged
//       in LDS by the first 94 lanes);
//   (2) for every instance of the tile's bin, in ascending record order: the glyph's edges under the instance's matrix go to LDS once,
//       relative to the low corner of the transformed glyph box (int32: the box spans less than 2^30); a lane whose samples meet the box
//       walks the edges, skips those that cross none of its four sample rows, and counts the winding number of its 64 samples (the cross
//       product once per edge and row, then one 64-bit addition per sample along the row); the coverage blends the colour into the
//       lane's registers;
//   (3) one 12-byte store at any alignment (the last one to three pixels of a row byte by byte).
// Every output byte is stored once, by the lane that owns its pixel: no atomics, no float arithmetic.  Addresses are formed from descriptor,
// tile, bin and glyph values that the host entry point has checked before the launch; what the kernel reads from the device copies of
// records and glyphs it checks again against R, G, E and the tile's image, and skips the instance otherwise.
#include "common.h"

namespace {

constexpr int SY_D = 8;  // int64 fields of an image's descriptor
enum { SY_OFF = 0, SY_H = 1, SY_W = 2, SY_FIRST = 3, SY_BASE = 4, SY_AMP = 5, SY_SEED = 6 };
constexpr int SY_REC = 9;  // int64 fields of an instance
enum { SR_IMAGE = 0, SR_GLYPH = 1, SR_A00 = 2, SR_A01 = 3, SR_A10 = 4, SR_A11 = 5, SR_TX = 6, SR_TY = 7, SR_COLOUR = 8 };
constexpr int SY_TILE = 32, SY_THREADS = 256, SY_MAX_EDGES = 512, SY_LATTICE_VALUES = 4 + 9 + 81;
constexpr long SY_MAX_IMAGES = 65535, SY_MAX_SIDE = 16384, SY_MAX_GLYPHS = 65535, SY_MAX_UNITS = 1 << 14;
constexpr long long SY_L = 1ll << 20, SY_Q = SY_L / 4;  // lattice units per pixel, per sample step
constexpr long long SY_A_LIM = 1ll << 19, SY_T_LIM = 1ll << 35, SY_SPAN_LIM = 1ll << 30;
constexpr unsigned SY_M0 = 0xD2511F53u, SY_M1 = 0xCD9E8D57u, SY_W0 = 0x9E3779B9u, SY_W1 = 0xBB67AE85u;

// three dwords at any byte alignment
struct __attribute__((packed, aligned(1))) sy_bytes12 {
    unsigned w[3];
};

// word 0 of the Philox4x32-10 block of counter (c0, c1, c2, 0)
__device__ __forceinline__ unsigned sy_philox(unsigned c0, unsigned c1, unsigned c2, unsigned k0, unsigned k1) {
    unsigned c3 = 0;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned long long p0 = (unsigned long long)SY_M0 * c0, p1 = (unsigned long long)SY_M1 * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1, c3 = (unsigned)p0, c0 = n0, c2 = n2;
        k0 += SY_W0, k1 += SY_W1;
    }
    return c0;
}

__device__ __forceinline__ long long sy_min(long long a, long long b) { return a < b ? a : b; }
__device__ __forceinline__ long long sy_max(long long a, long long b) { return a > b ? a : b; }

// The box of the glyph's font-unit box {xmin, ymin, xmax, ymax} under the instance's matrix, relative to t -> false: the instance is not
// evaluated (|a| >= 2^19, |t| > 2^35, a font coordinate beyond 2^14 or a span >= 2^30).  With these every product below is < 2^33.
__device__ __forceinline__ bool sy_box(const long long* __restrict__ rec, const int* __restrict__ g, long long (&lo)[2], long long (&span)[2]) {
    bool ok = rec[SR_TX] >= -SY_T_LIM && rec[SR_TX] <= SY_T_LIM && rec[SR_TY] >= -SY_T_LIM && rec[SR_TY] <= SY_T_LIM;
#pragma unroll
    for (int k = 2; k < 6; ++k) ok = ok && g[k] >= -SY_MAX_UNITS && g[k] <= SY_MAX_UNITS;
#pragma unroll
    for (int k = SR_A00; k <= SR_A11; ++k) ok = ok && rec[k] > -SY_A_LIM && rec[k] < SY_A_LIM;
    if (!ok || g[2] > g[4] || g[3] > g[5]) return false;
#pragma unroll
    for (int axis = 0; axis < 2; ++axis) {
        const long long ax = rec[SR_A00 + 2 * axis], ay = rec[SR_A01 + 2 * axis];
        lo[axis] = sy_min(ax * g[2], ax * g[4]) + sy_min(ay * g[3], ay * g[5]);
        span[axis] = sy_max(ax * g[2], ax * g[4]) + sy_max(ay * g[3], ay * g[5]) - lo[axis];
    }
    return span[0] < SY_SPAN_LIM && span[1] < SY_SPAN_LIM;
}

__global__ __launch_bounds__(SY_THREADS) void synth_kernel(const unsigned char* __restrict__ bg, unsigned char* __restrict__ out,
                                                           const long long* __restrict__ desc, const long long* __restrict__ recs, long R,
                                                           const int* __restrict__ bins, long T, const int* __restrict__ edges, long E,
                                                           const int* __restrict__ glyphs, int G) {
    __shared__ int s_edge[4][SY_MAX_EDGES];  // ax, ay, bx, by of the instance's edges, relative to its box
    __shared__ unsigned char s_n[96];        // the lattice values of the three octaves under this tile
    // (everything up to the lane's own indices is the same in all lanes of the workgroup)
    const int* tile = bins + 4 * (long)blockIdx.x;
    const int n = tile[0], y0 = tile[1], x0 = tile[2];
    const long first = blockIdx.x ? (long)tile[-1] : 4 * T, end = tile[3];
    const long long* d = desc + (long)n * SY_D;
    const int H = (int)d[SY_H], W = (int)d[SY_W];
    const int tid = threadIdx.x, py = y0 + (tid >> 3), px = x0 + 4 * (tid & 7);
    const int count = py < H && px < W ? (W - px < 4 ? W - px : 4) : 0;  // the lane's pixels: px .. px + count - 1 of row py
    const long at = d[SY_OFF] + 3 * ((long)py * W + px);

    // (1) the background
    int cur[4][3];
#pragma unroll
    for (int p = 0; p < 4; ++p) cur[p][0] = cur[p][1] = cur[p][2] = 0;
    if (bg) {
        if (count == 4) {
            const sy_bytes12 v = *reinterpret_cast<const sy_bytes12*>(bg + at);
#pragma unroll
            for (int k = 0; k < 12; ++k) cur[k / 3][k % 3] = (int)((v.w[k >> 2] >> (8 * (k & 3))) & 255u);
        } else {
#pragma unroll
            for (int p = 0; p < 3; ++p)
                if (p < count)
#pragma unroll
                    for (int k = 0; k < 3; ++k) cur[p][k] = bg[at + 3 * p + k];
        }
    } else {
        const unsigned long long seed = (unsigned long long)d[SY_SEED];
        if (tid < SY_LATTICE_VALUES) {  // octave 0: 2 x 2 corners of cells of 64 pixels, octave 1: 3 x 3 of 16, octave 2: 9 x 9 of 4
            const int o = tid < 4 ? 0 : tid < 13 ? 1 : 2, k = tid - (o == 0 ? 0 : o == 1 ? 4 : 13), side = o == 0 ? 2 : o == 1 ? 3 : 9;
            const int sh = 6 - 2 * o;
            s_n[tid] = (unsigned char)(sy_philox((unsigned)((x0 >> sh) + k % side), (unsigned)((y0 >> sh) + k / side), (unsigned)o, (unsigned)seed,
                                                 (unsigned)(seed >> 32)) >> 24);
        }
        __syncthreads();
        const int base = (int)d[SY_BASE], amp = (int)d[SY_AMP];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            int D = 0;
#pragma unroll
            for (int o = 0; o < 3; ++o) {
                const int sh = 6 - 2 * o, C = 1 << sh, side = o == 0 ? 2 : o == 1 ? 3 : 9, from = o == 0 ? 0 : o == 1 ? 4 : 13;
                const int lx = ((px + p) >> sh) - (x0 >> sh), ly = (py >> sh) - (y0 >> sh), fx = (px + p) & (C - 1), fy = py & (C - 1);
                const unsigned char* c = s_n + from + ly * side + lx;  // lx + 1 < side and ly + 1 < side: the tile is 32 pixels from a multiple of 32
                const int t = (C - fy) * ((C - fx) * c[0] + fx * c[1]) + fy * ((C - fx) * c[side] + fx * c[side + 1]);  // <= 255 C^2
                D += ((amp >> (8 * o)) & 255) * ((t - 128 * C * C) * (1 << (12 - 2 * sh)));                          // |.| <= 64 * 2^19
            }
            const int move = (D + (1 << 18)) >> 19;  // >> of a negative value is floor
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int v = ((base >> (8 * k)) & 255) + move;
                cur[p][k] = v < 0 ? 0 : v > 255 ? 255 : v;
            }
        }
    }

    // (2) the instances of this tile's bin, in ascending record order
    for (long b = first; b < end; ++b) {
        const long r = bins[b];
        if (r < 0 || r >= R) continue;
        const long long* rec = recs + r * SY_REC;
        const long long glyph = rec[SR_GLYPH];
        if (rec[SR_IMAGE] != n || glyph < 0 || glyph >= G) continue;
        const int* g = glyphs + 6 * glyph;
        const int e0 = g[0], ne = g[1];
        long long lo[2], span[2];
        if (e0 < 0 || ne < 1 || ne > SY_MAX_EDGES || (long)e0 + ne > E || !sy_box(rec, g, lo, span)) continue;

        __syncthreads();  // the lanes have read the edges of the instance before
        for (int e = tid; e < ne; e += SY_THREADS) {
            const int4 v = reinterpret_cast<const int4*>(edges)[e0 + e];
            s_edge[0][e] = (int)(rec[SR_A00] * v.x + rec[SR_A01] * v.y - lo[0]);
            s_edge[1][e] = (int)(rec[SR_A10] * v.x + rec[SR_A11] * v.y - lo[1]);
            s_edge[2][e] = (int)(rec[SR_A00] * v.z + rec[SR_A01] * v.w - lo[0]);
            s_edge[3][e] = (int)(rec[SR_A10] * v.z + rec[SR_A11] * v.w - lo[1]);
        }
        __syncthreads();

        // the lane's first sample relative to the box: sample (i, j) of pixel p sits at (X0 + (4 p + i) Q, Y0 + j Q)
        const long long X0 = SY_L * px + SY_L / 8 - rec[SR_TX] - lo[0], Y0 = SY_L * py + SY_L / 8 - rec[SR_TY] - lo[1];
        if (count == 0 || X0 > span[0] || X0 + (4 * count - 1) * SY_Q < 0 || Y0 > span[1] || Y0 + 3 * SY_Q < 0) continue;
        // now -4 L < X0, Y0 <= 2^30: every difference below fits 32 bits, every product 62
        const int Yl = (int)Y0;
        int wn[4][16];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) wn[j][i] = 0;
        for (int e = 0; e < ne; ++e) {
            const int ax = s_edge[0][e], ay = s_edge[1][e], bx = s_edge[2][e], by = s_edge[3][e];
            const bool up = ay < by;
            const int el = up ? ay : by, eh = up ? by : ay;  // the edge counts for el <= Y < eh (never when it is horizontal)
            if (eh <= Yl || el > Yl + 3 * (int)SY_Q) continue;
            const long long dx = (long long)bx - ax, dy = (long long)by - ay, xa = X0 - ax;
            const int sign = up ? 1 : -1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int Y = Yl + j * (int)SY_Q;
                if (el <= Y && Y < eh) {
                    // cr = dx (Y - ay) - dy (X - ax); an upward edge counts +1 where cr > 0, a downward one -1 where cr < 0
                    long long c = dx * (Y - ay) - dy * xa, step = -dy * SY_Q;
                    if (!up) c = -c, step = -step;
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        wn[j][i] += c > 0 ? sign : 0;
                        c += step;
                    }
                }
            }
        }
        const int colour = (int)rec[SR_COLOUR];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            int cov = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) cov += wn[j][4 * p + i] != 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) cur[p][k] = (cov * ((colour >> (8 * k)) & 255) + (16 - cov) * cur[p][k] + 8) >> 4;
        }
    }

    // (3) out
    if (count == 4) {
        sy_bytes12 v = {{0u, 0u, 0u}};
#pragma unroll
        for (int k = 0; k < 12; ++k) v.w[k >> 2] |= (unsigned)cur[k / 3][k % 3] << (8 * (k & 3));
        *reinterpret_cast<sy_bytes12*>(out + at) = v;
    } else {
#pragma unroll
        for (int p = 0; p < 3; ++p)
            if (p < count)
#pragma unroll
                for (int k = 0; k < 3; ++k) out[at + 3 * p + k] = (unsigned char)cur[p][k];
    }
}

// Every value the kernel forms an address or bounds a loop with, from the host copies: descriptors against `bytes`, the canonical tile
// list, the glyph table against E, the records against N and G, the bins against R and their tile's image.
int sy_validate(const long long* hdesc, int N, long bytes, const long long* hrecs, long R, const int* hbins, long T, long B, long E,
                const int* hglyphs, int G) {
    DBN_REQUIRE(hdesc && hbins && hglyphs && N >= 1 && N <= SY_MAX_IMAGES && bytes > 0 && G >= 1 && G <= SY_MAX_GLYPHS && E >= 0 &&
                E <= 0x7FFFFFFFl && R >= 0 && R <= 0x7FFFFFFFl && (R == 0 || hrecs) && T >= 1 && T <= 0x1FFFFFFFl && B >= 4 * T &&
                B <= 0x7FFFFFFFl);
    for (int k = 0; k < G; ++k) {
        const int* g = hglyphs + 6 * (long)k;
        DBN_REQUIRE(g[0] >= 0 && g[1] >= 0 && g[1] <= SY_MAX_EDGES && (long)g[0] + g[1] <= E);
        for (int f = 2; f < 6; ++f) DBN_REQUIRE(g[f] >= -SY_MAX_UNITS && g[f] <= SY_MAX_UNITS);
        DBN_REQUIRE(g[2] <= g[4] && g[3] <= g[5]);
    }
    for (long r = 0; r < R; ++r) {
        const long long* rec = hrecs + r * SY_REC;
        DBN_REQUIRE(rec[SR_IMAGE] >= 0 && rec[SR_IMAGE] < N && rec[SR_GLYPH] >= 0 && rec[SR_GLYPH] < G && rec[SR_COLOUR] >= 0 &&
                    rec[SR_COLOUR] < (1 << 24));
    }
    long end = 0, tile = 0, list = 4 * T;
    for (int n = 0; n < N; ++n) {
        const long long* d = hdesc + (long)n * SY_D;
        const long h = d[SY_H], w = d[SY_W];
        DBN_REQUIRE(h >= 1 && h <= SY_MAX_SIDE && w >= 1 && w <= SY_MAX_SIDE);
        DBN_REQUIRE(d[SY_OFF] >= end && d[SY_OFF] <= bytes && 3 * h * w <= bytes - d[SY_OFF]);  // in order: no two images overlap
        end = d[SY_OFF] + 3 * h * w;
        DBN_REQUIRE(d[SY_BASE] >= 0 && d[SY_BASE] < (1 << 24) && d[SY_AMP] >= 0 && d[SY_AMP] < (1 << 24));
        for (int o = 0; o < 3; ++o) DBN_REQUIRE(((d[SY_AMP] >> (8 * o)) & 255) <= 64);
        DBN_REQUIRE(d[SY_FIRST] == tile);
        const long across = (w + SY_TILE - 1) / SY_TILE, tiles = across * ((h + SY_TILE - 1) / SY_TILE);
        DBN_REQUIRE(tiles <= T - tile);
        for (long k = 0; k < tiles; ++k) {  // every tile of the image once, in row-major order; its list follows the one before
            const int* t = hbins + 4 * (tile + k);
            DBN_REQUIRE(t[0] == n && t[1] == k / across * SY_TILE && t[2] == k % across * SY_TILE && t[3] >= list && t[3] <= B);
            for (long b = list; b < t[3]; ++b)
                DBN_REQUIRE(hbins[b] >= 0 && hbins[b] < R && (b == list || hbins[b] > hbins[b - 1]) && hrecs[hbins[b] * SY_REC + SR_IMAGE] == n);
            list = t[3];
        }
        tile += tiles;
    }
    DBN_REQUIRE(tile == T && list == B);
    return DBN_OK;
}

}  // namespace

int dbn_synth_text_u8(const unsigned char* backgrounds, unsigned char* out, long bytes, const long long* hdesc, const long long* desc, int N,
                      const long long* hrecs, const long long* recs, long R, const int* hbins, const int* bins, long T, long B, const int* edges,
                      long E, const int* hglyphs, const int* glyphs, int G, void* stream) {
    const int rc = sy_validate(hdesc, N, bytes, hrecs, R, hbins, T, B, E, hglyphs, G);
    if (rc != DBN_OK) return rc;
    DBN_REQUIRE(out && desc && bins && glyphs && (R == 0 || recs) && (E == 0 || edges));
    DBN_REQUIRE(!backgrounds || out + bytes <= backgrounds || backgrounds + bytes <= out);
    hipLaunchKernelGGL(synth_kernel, dim3((unsigned)T), dim3(SY_THREADS), 0, (hipStream_t)stream, backgrounds, out, desc, recs, R, bins, T, edges, E,
                       glyphs, G);
    return dbn_status();
}
