// PNG at both ends of the device pipeline (db_text_minimal_amd/png.py; ABI and layouts: include/dbnet_hip.h).  zlib's inflate and
// deflate are serial per stream and stay on the host; here is everything around them:
//   png_unfilter_kernel  undoes the five scanline filters: one workgroup per sub-image (an image, or one Adam7 pass of one), lanes are
//                        rows, a wavefront over 16-byte chunks with one barrier per step;
//   png_pixels_kernel    grid-stride over the output pixels of the batch: bit unpacking, palette, high byte of 16-bit samples, grey
//                        replication, alpha dropped, Adam7 placement -> packed uint8 RGB at any byte alignment;
//   png_filter_kernel    the encoder's filter choice and application, one wave per row.
// No workgroup waits for another one anywhere in this unit, and every loop bound is a descriptor value that the host entry point
// has checked against the buffer lengths (png_validate) before the launch.
#include "common.h"

namespace {

constexpr int PD = 32;  // int64 fields of an image's descriptor
enum { P_W = 0, P_H = 1, P_DEPTH = 2, P_CTYPE = 3, P_LACE = 4, P_OUT = 5, P_NPAL = 6, P_STATUS = 7, P_SRC = 8, P_RAW = 16 };
constexpr int UF_ROWS = 256;  // rows of a band = lanes of the workgroup
constexpr int UF_CHUNK = 16;  // bytes a lane reconstructs per step
constexpr long PNG_MAX_SIDE = 65535;

__host__ __device__ inline int png_channels(int ct) { return ct == 2 ? 3 : ct == 4 ? 2 : ct == 6 ? 4 : 1; }

// slot 0: the whole image (not interlaced); 1 .. 7: the Adam7 passes
__host__ __device__ inline void png_pass(int slot, int& x0, int& y0, int& dx, int& dy) {
    switch (slot) {
        case 1: x0 = 0, y0 = 0, dx = 8, dy = 8; break;
        case 2: x0 = 4, y0 = 0, dx = 8, dy = 8; break;
        case 3: x0 = 0, y0 = 4, dx = 4, dy = 8; break;
        case 4: x0 = 2, y0 = 0, dx = 4, dy = 4; break;
        case 5: x0 = 0, y0 = 2, dx = 2, dy = 4; break;
        case 6: x0 = 1, y0 = 0, dx = 2, dy = 2; break;
        case 7: x0 = 0, y0 = 1, dx = 1, dy = 2; break;
        default: x0 = 0, y0 = 0, dx = 1, dy = 1; break;
    }
}

// the sub-image of `slot`: its width and height in pixels (0: empty), the bytes of a row without the type byte
__host__ __device__ inline void png_sub(long w, long h, int bits, int slot, long& pw, long& ph, long& rb) {
    int x0, y0, dx, dy;
    png_pass(slot, x0, y0, dx, dy);
    pw = w > x0 ? (w - x0 + dx - 1) / dx : 0;
    ph = h > y0 ? (h - y0 + dy - 1) / dy : 0;
    rb = (pw * bits + 7) / 8;
}
__host__ __device__ inline long png_stride(long rb) { return (rb + UF_CHUNK - 1) / UF_CHUNK * UF_CHUNK; }

inline bool png_pair_ok(int ct, int depth) {
    if (ct == 0) return depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16;
    if (ct == 3) return depth == 1 || depth == 2 || depth == 4 || depth == 8;
    return (ct == 2 || ct == 4 || ct == 6) && (depth == 8 || depth == 16);
}

// every value a kernel of this unit bounds a loop or forms an address with, against the lengths of the buffers
int png_validate(const long long* hdesc, int N, long blob_len, long raw_bytes, long out_bytes) {
    DBN_REQUIRE(hdesc && N > 0 && blob_len > 0 && raw_bytes > 0 && out_bytes > 0);
    long acc = 0, src = 0, raw = 0;
    for (int n = 0; n < N; ++n) {
        const long long* d = hdesc + (long)n * PD;
        DBN_REQUIRE(d[P_OUT] == acc);  // packed, in order: the pixel kernel searches these
        if (d[P_STATUS] != 0) continue;
        const long w = d[P_W], h = d[P_H];
        const int depth = (int)d[P_DEPTH], ct = (int)d[P_CTYPE];
        DBN_REQUIRE(w >= 1 && w <= PNG_MAX_SIDE && h >= 1 && h <= PNG_MAX_SIDE && d[P_DEPTH] == depth && d[P_CTYPE] == ct && png_pair_ok(ct, depth));
        DBN_REQUIRE((d[P_LACE] == 0 || d[P_LACE] == 1) && d[P_NPAL] >= 0 && d[P_NPAL] <= 256);
        acc += w * h * 3;
        DBN_REQUIRE(acc <= out_bytes);
        for (int slot = d[P_LACE] ? 1 : 0; slot <= (d[P_LACE] ? 7 : 0); ++slot) {
            long pw, ph, rb;
            png_sub(w, h, depth * png_channels(ct), slot, pw, ph, rb);
            if (pw == 0 || ph == 0) continue;
            DBN_REQUIRE(d[P_SRC + slot] == src && ph * (rb + 1) <= blob_len - src);  // end to end, in order: no two overlap
            DBN_REQUIRE(d[P_RAW + slot] == raw && ph * png_stride(rb) <= raw_bytes - raw);
            src += ph * (rb + 1);
            raw += ph * png_stride(rb);  // stays a multiple of 16
        }
    }
    DBN_REQUIRE(acc == out_bytes && src == blob_len);
    return DBN_OK;
}

__device__ __forceinline__ unsigned png_paeth(unsigned a, unsigned b, unsigned c) {
    const int p = (int)a + (int)b - (int)c;
    const int pa = abs(p - (int)a), pb = abs(p - (int)b), pc = abs(p - (int)c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
__device__ __forceinline__ unsigned png_pred(unsigned ft, unsigned a, unsigned b, unsigned c) {
    return ft == 0 ? 0u : ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : png_paeth(a, b, c);
}

typedef unsigned png_u32x4 __attribute__((ext_vector_type(4)));

// One sub-image: `rows` rows of 1 + rb filtered bytes at src -> rows of rb reconstructed bytes at raw, `stride` apart.  Bands of
// UF_ROWS rows in turn; in a band lane r owns row R0 + r and at step t reconstructs chunk t - r, whose row above (chunk t - r of
// lane r - 1) was finished at step t - 1 and waits in LDS; lane 0 reads the last row of the band before from raw.
template <int BPP>
__device__ void png_unfilter_sub(const unsigned char* __restrict__ src, unsigned char* raw, long rows, long rb, long stride,
                                 png_u32x4 (*above)[UF_ROWS]) {
    const int r = threadIdx.x;
    const int nchunks = (int)((rb + UF_CHUNK - 1) / UF_CHUNK);
    for (long R0 = 0; R0 < rows; R0 += UF_ROWS) {
        const int nb = (int)(rows - R0 < UF_ROWS ? rows - R0 : UF_ROWS);
        const long row = R0 + r;
        const bool active = r < nb;
        const unsigned char* frow = src + (active ? row : 0) * (rb + 1);
        const unsigned ft = active ? frow[0] : 0u;
        unsigned left[8], ul[8];  // the last 8 bytes of the chunk before: of this row, and of the row above
        const int steps = nchunks + nb - 1;
        for (int t = 0; t < steps; ++t) {
            const int k = t - r;
            if (active && k >= 0 && k < nchunks) {
                if (k == 0) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) left[j] = ul[j] = 0u;
                }
                // 16 filtered bytes at any alignment: five aligned words, shifted (the blob is padded past its end)
                const unsigned char* p = frow + 1 + (long)k * UF_CHUNK;
                const unsigned sh = (unsigned)(reinterpret_cast<size_t>(p) & 3) * 8;
                const unsigned* q = reinterpret_cast<const unsigned*>(p - (sh >> 3));
                const unsigned d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3], d4 = q[4];
                const unsigned fw[4] = {__funnelshift_r(d0, d1, sh), __funnelshift_r(d1, d2, sh), __funnelshift_r(d2, d3, sh),
                                        __funnelshift_r(d3, d4, sh)};
                png_u32x4 upw = {0u, 0u, 0u, 0u};
                if (r > 0)
                    upw = above[(t + 1) & 1][r - 1];
                else if (row > 0)
                    upw = *reinterpret_cast<const png_u32x4*>(raw + (row - 1) * stride + (long)k * UF_CHUNK);
                unsigned cur[UF_CHUNK], up[UF_CHUNK];
#pragma unroll
                for (int i = 0; i < UF_CHUNK; ++i) up[i] = (upw[i >> 2] >> (8 * (i & 3))) & 255u;
#pragma unroll
                for (int i = 0; i < UF_CHUNK; ++i) {
                    const unsigned f = (fw[i >> 2] >> (8 * (i & 3))) & 255u;
                    const unsigned a = i >= BPP ? cur[i >= BPP ? i - BPP : 0] : left[i < BPP ? 8 - BPP + i : 0];
                    const unsigned c = i >= BPP ? up[i >= BPP ? i - BPP : 0] : ul[i < BPP ? 8 - BPP + i : 0];
                    cur[i] = (f + png_pred(ft, a, up[i], c)) & 255u;
                }
                png_u32x4 cw;
#pragma unroll
                for (int v = 0; v < 4; ++v) cw[v] = cur[4 * v] | (cur[4 * v + 1] << 8) | (cur[4 * v + 2] << 16) | (cur[4 * v + 3] << 24);
                above[t & 1][r] = cw;
                *reinterpret_cast<png_u32x4*>(raw + row * stride + (long)k * UF_CHUNK) = cw;
#pragma unroll
                for (int j = 0; j < 8; ++j) left[j] = cur[8 + j], ul[j] = up[8 + j];
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(UF_ROWS) void png_unfilter_kernel(const unsigned char* __restrict__ blob, const long long* __restrict__ desc,
                                                               const int* __restrict__ subs, unsigned char* raw) {
    __shared__ png_u32x4 above[2][UF_ROWS];
    const int n = subs[2 * blockIdx.x], slot = subs[2 * blockIdx.x + 1];
    const long long* d = desc + (long)n * PD;
    const int bits = (int)d[P_DEPTH] * png_channels((int)d[P_CTYPE]);
    long pw, ph, rb;
    png_sub(d[P_W], d[P_H], bits, slot, pw, ph, rb);
    const unsigned char* src = blob + d[P_SRC + slot];
    unsigned char* dst = raw + d[P_RAW + slot];
    const long stride = png_stride(rb);
    switch (bits >> 3) {  // bytes per pixel, at least 1: the distance of the filters' left neighbour
        case 2: png_unfilter_sub<2>(src, dst, ph, rb, stride, above); break;
        case 3: png_unfilter_sub<3>(src, dst, ph, rb, stride, above); break;
        case 4: png_unfilter_sub<4>(src, dst, ph, rb, stride, above); break;
        case 6: png_unfilter_sub<6>(src, dst, ph, rb, stride, above); break;
        case 8: png_unfilter_sub<8>(src, dst, ph, rb, stride, above); break;
        default: png_unfilter_sub<1>(src, dst, ph, rb, stride, above); break;
    }
}

constexpr int PX_THREADS = 256;

__global__ __launch_bounds__(PX_THREADS) void png_pixels_kernel(const unsigned char* __restrict__ raw, const long long* __restrict__ desc,
                                                                const unsigned char* __restrict__ pal, int N, unsigned char* __restrict__ out,
                                                                long out_pixels) {
    for (long px = (long)blockIdx.x * PX_THREADS + threadIdx.x; px < out_pixels; px += (long)gridDim.x * PX_THREADS) {
        int lo = 0, hi = N - 1;  // the last image whose first byte is at or before this pixel's (failed images take no bytes)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (desc[(long)mid * PD + P_OUT] <= 3 * px) lo = mid; else hi = mid - 1;
        }
        const long long* d = desc + (long)lo * PD;
        const unsigned w = (unsigned)d[P_W];
        const int depth = (int)d[P_DEPTH], ct = (int)d[P_CTYPE], ch = png_channels(ct);
        const long q = px - d[P_OUT] / 3;
        const unsigned y = (unsigned)(q / w), x = (unsigned)(q - (long)y * w);
        int slot = 0;
        unsigned sx = x, sy = y;
        long rb = ((long)w * depth * ch + 7) / 8;
        if (d[P_LACE]) {
            const unsigned xm = x & 7, ym = y & 7;
            slot = (ym & 1) ? 7 : (xm & 1) ? 6 : (ym & 2) ? 5 : (xm & 2) ? 4 : (ym & 4) ? 3 : (xm & 4) ? 2 : 1;
            int x0, y0, dx, dy;
            png_pass(slot, x0, y0, dx, dy);
            sx = (x - x0) / dx, sy = (y - y0) / dy;
            long pw, ph;
            png_sub(w, d[P_H], depth * ch, slot, pw, ph, rb);
        }
        const unsigned char* row = raw + d[P_RAW + slot] + (long)sy * png_stride(rb);
        unsigned v0, v1, v2;
        if (depth >= 8) {
            const int bs = depth >> 3;  // 16-bit samples are big-endian: the high byte comes first
            const unsigned char* s = row + (long)sx * ch * bs;
            v0 = s[0];
            v1 = ct == 2 || ct == 6 ? s[bs] : v0;
            v2 = ct == 2 || ct == 6 ? s[2 * bs] : v0;
        } else {
            const unsigned bit = sx * depth;
            v0 = (row[bit >> 3] >> (8 - depth - (bit & 7))) & ((1u << depth) - 1);
            if (ct == 0) v0 *= depth == 1 ? 255u : depth == 2 ? 85u : 17u;
            v1 = v2 = v0;
        }
        if (ct == 3) {
            const unsigned idx = v0;
            const unsigned char* e = pal + ((long)lo * 256 + idx) * 3;
            const bool in = idx < (unsigned)d[P_NPAL];
            v0 = in ? e[0] : 0u, v1 = in ? e[1] : 0u, v2 = in ? e[2] : 0u;
        }
        unsigned char* o = out + 3 * px;
        o[0] = (unsigned char)v0, o[1] = (unsigned char)v1, o[2] = (unsigned char)v2;
    }
}

// ---- encode: filter choice and application -------------------------------------------------------------------------------
constexpr int ED = 8;  // int64 fields: {input byte offset, H, W, channels, output byte offset, first row over the batch, 0, 0}
constexpr int FL_THREADS = 256;

__global__ __launch_bounds__(FL_THREADS) void png_filter_kernel(const unsigned char* __restrict__ pixels, const long long* __restrict__ desc, int N,
                                                                long total_rows, int fixed, unsigned char* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long waves = (long)gridDim.x * (FL_THREADS / 64);
    for (long gr = (long)blockIdx.x * (FL_THREADS / 64) + (threadIdx.x >> 6); gr < total_rows; gr += waves) {
        int lo = 0, hi = N - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (desc[(long)mid * ED + 5] <= gr) lo = mid; else hi = mid - 1;
        }
        const long long* d = desc + (long)lo * ED;
        const long y = gr - d[5];
        const int bpp = (int)d[3];
        const long rb = d[2] * bpp;
        const unsigned char* cur = pixels + d[0] + y * rb;
        const unsigned char* up = cur - rb;
        const bool top = y == 0;
        int pick = fixed;
        if (fixed < 0) {
            int s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
            for (long x = lane; x < rb; x += 64) {
                const bool first = x < bpp;
                const unsigned v = cur[x], a = first ? 0u : cur[x - bpp], b = top ? 0u : up[x], c = (top || first) ? 0u : up[x - bpp];
                const unsigned f0 = v, f1 = (v - a) & 255u, f2 = (v - b) & 255u, f3 = (v - ((a + b) >> 1)) & 255u, f4 = (v - png_paeth(a, b, c)) & 255u;
                s0 += min(f0, 256u - f0), s1 += min(f1, 256u - f1), s2 += min(f2, 256u - f2), s3 += min(f3, 256u - f3), s4 += min(f4, 256u - f4);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                s0 += __shfl_xor(s0, o, 64), s1 += __shfl_xor(s1, o, 64), s2 += __shfl_xor(s2, o, 64), s3 += __shfl_xor(s3, o, 64), s4 += __shfl_xor(s4, o, 64);
            }
            pick = 0;
            int best = s0;  // the lowest score; of equal ones the lowest type
            if (s1 < best) best = s1, pick = 1;
            if (s2 < best) best = s2, pick = 2;
            if (s3 < best) best = s3, pick = 3;
            if (s4 < best) best = s4, pick = 4;
        }
        unsigned char* o = out + d[4] + y * (rb + 1);
        if (lane == 0) o[0] = (unsigned char)pick;
        for (long x = lane; x < rb; x += 64) {
            const bool first = x < bpp;
            const unsigned v = cur[x], a = first ? 0u : cur[x - bpp], b = top ? 0u : up[x], c = (top || first) ? 0u : up[x - bpp];
            o[1 + x] = (unsigned char)(v - png_pred((unsigned)pick, a, b, c));
        }
    }
}

}  // namespace

int dbn_png_check(const long long* hdesc, int N, const int* hsubs, int n_subs, long blob_len, long raw_bytes, long out_bytes) {
    const int rc = png_validate(hdesc, N, blob_len, raw_bytes, out_bytes);
    if (rc != DBN_OK) return rc;
    DBN_REQUIRE(hsubs && n_subs > 0);
    for (int s = 0; s < n_subs; ++s) {
        const int n = hsubs[2 * s], slot = hsubs[2 * s + 1];
        DBN_REQUIRE(n >= 0 && n < N);
        const long long* d = hdesc + (long)n * PD;
        DBN_REQUIRE(d[P_STATUS] == 0 && (d[P_LACE] ? slot >= 1 && slot <= 7 : slot == 0));
        long pw, ph, rb;
        png_sub(d[P_W], d[P_H], (int)d[P_DEPTH] * png_channels((int)d[P_CTYPE]), slot, pw, ph, rb);
        DBN_REQUIRE(pw > 0 && ph > 0);
    }
    return DBN_OK;
}

int dbn_png_unfilter(const unsigned char* blob, long blob_len, long blob_cap, const long long* hdesc, const long long* desc, int N,
                     const int* hsubs, const int* subs, int n_subs, unsigned char* raw, long raw_bytes, long out_bytes, void* stream) {
    DBN_REQUIRE(blob && desc && subs && raw && blob_cap >= blob_len + 32);
    DBN_REQUIRE((reinterpret_cast<size_t>(blob) & 3) == 0 && (reinterpret_cast<size_t>(raw) & 15) == 0);
    const int rc = dbn_png_check(hdesc, N, hsubs, n_subs, blob_len, raw_bytes, out_bytes);
    if (rc != DBN_OK) return rc;
    hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)n_subs), dim3(UF_ROWS), 0, (hipStream_t)stream, blob, desc, subs, raw);
    return dbn_status();
}

int dbn_png_pixels(const unsigned char* raw, long raw_bytes, const long long* hdesc, const long long* desc, const unsigned char* palettes, int N,
                   long blob_len, unsigned char* out, long out_bytes, void* stream) {
    DBN_REQUIRE(raw && desc && palettes && out);
    const int rc = png_validate(hdesc, N, blob_len, raw_bytes, out_bytes);
    if (rc != DBN_OK) return rc;
    const long pixels = out_bytes / 3;
    hipLaunchKernelGGL(png_pixels_kernel, dim3((unsigned)dbn_grid(pixels, PX_THREADS, 2048)), dim3(PX_THREADS), 0, (hipStream_t)stream, raw, desc,
                       palettes, N, out, pixels);
    return dbn_status();
}

int dbn_png_filter_rows(const unsigned char* pixels, long in_bytes, const long long* hdesc, const long long* desc, int N, int filter,
                        unsigned char* out, long out_bytes, void* stream) {
    DBN_REQUIRE(pixels && hdesc && desc && out && N > 0 && in_bytes > 0 && out_bytes > 0 && filter >= -1 && filter <= 4);
    long rows = 0;
    for (int n = 0; n < N; ++n) {
        const long long* d = hdesc + (long)n * ED;
        const long h = d[1], w = d[2], nc = d[3];
        DBN_REQUIRE(h >= 1 && h <= PNG_MAX_SIDE && w >= 1 && w <= PNG_MAX_SIDE && (nc == 1 || nc == 3) && d[5] == rows);
        DBN_REQUIRE(d[0] >= 0 && d[0] <= in_bytes && h * w * nc <= in_bytes - d[0]);
        DBN_REQUIRE(d[4] >= 0 && d[4] <= out_bytes && h * (w * nc + 1) <= out_bytes - d[4]);
        rows += h;
    }
    hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)dbn_grid(rows, FL_THREADS / 64, 4096)), dim3(FL_THREADS), 0, (hipStream_t)stream, pixels,
                       desc, N, rows, filter, out);
    return dbn_status();
}
