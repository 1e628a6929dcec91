// Around a text recogniser, on the device: the last stage of the reference's "full pipeline" (test_ocr.py:59-108,179-200,
// test_webcam.py), batched.  The recogniser itself is the user's module.
//   words_to_input   rec_preprocess of every crop: uint8 [K][h][w][3] -> [K][1 | 3][h][w] in fp32 / bf16 / fp16
//   greedy_decode    predict(): logits [B][T][C] -> codes, count, score per sequence, two launches
//
// words_to_input.  Grey is PIL's convert('L') in integers, (19595 c0 + 38470 c1 + 7471 c2 + 32768) >> 16; the value is
// lut[g], a 256-entry fp32 table the caller builds on the host as (g / 255 - 0.5) / 0.5 in numpy fp32, so the fp32 result
// is that table bit for bit and the 16-bit ones are its round-to-nearest-even conversions.  A thread owns four
// consecutive pixels: three dword loads, one 16- or 8-byte store per plane.
//
// greedy_decode.  Launch 1 (rec_step_*): per step row x[0 .. C)
//   m = max x (NaNs skipped), k = the smallest index with x == m, p = 1 / sum_c expf(x_c - m) in fp32;
//   a row with a NaN: k = the index of its first NaN, p = NaN (torch.max on the CPU; the sum is NaN by itself).
// k and p go to a workspace of B * T ints and B * T floats.  Rows of up to 512 classes (rec_step_small) are staged into
// LDS by whole workgroups with 16-byte loads -- rows are element-aligned only, the run of a workgroup's rows is
// contiguous -- and a team of 1, 2, 4 ... 64 lanes (the smallest with eight elements per lane) reduces each; longer rows
// (rec_step_wide) take one wave each, which walks the row's 16-byte-aligned body twice and its unaligned ends by element.
// Launch 2 (rec_collapse): one wave per sequence, 64 steps at a time: the kept steps by ballot and prefix count, the
// score as a serial fp32 product in ascending t (readlane), every element of codes / count / score written.
// Sums are folded in a fixed order (lane-strided partial sums, then xor butterflies), so two runs agree bit for bit.
// expf is the OCML one (1 ulp); 1.0f / s is the correctly rounded division (hipcc's default).
#include <math.h>

#include "common.h"

namespace {

constexpr int RC_THREADS = 256;
constexpr int RC_SMALL_C = 512, RC_PER_LANE = 8;  // rec_step_small: classes per row, elements per lane of a team
constexpr int RC_NONE = 0x7FFFFFFF;

// ---- words_to_input ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ int grey_l(unsigned c0, unsigned c1, unsigned c2) { return (int)((19595u * c0 + 38470u * c1 + 7471u * c2 + 32768u) >> 16); }

template <int AT>
__global__ void __launch_bounds__(RC_THREADS) words_to_input_kernel(const unsigned char* __restrict__ src, long n_px, long hw, int rgb, int bgr,
                                                                     const float* __restrict__ lut, void* __restrict__ out, int aligned) {
    __shared__ float s_lut[256];
    s_lut[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    const long p0 = ((long)blockIdx.x * RC_THREADS + threadIdx.x) * 4;
    if (p0 >= n_px) return;
    const int cnt = n_px - p0 < 4 ? (int)(n_px - p0) : 4;
    unsigned char b[12];
    if (cnt == 4 && (aligned & 1)) {
        const unsigned* s4 = reinterpret_cast<const unsigned*>(src + p0 * 3);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const unsigned w = s4[j];
            b[4 * j] = w & 255u, b[4 * j + 1] = (w >> 8) & 255u, b[4 * j + 2] = (w >> 16) & 255u, b[4 * j + 3] = w >> 24;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j) b[j] = j < cnt * 3 ? src[p0 * 3 + j] : 0;
    }
    const bool vec = cnt == 4 && (aligned & 2);
    if (!rgb) {
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = s_lut[bgr ? grey_l(b[3 * j + 2], b[3 * j + 1], b[3 * j]) : grey_l(b[3 * j], b[3 * j + 1], b[3 * j + 2])];
        if (vec) {
            dbn_st4<AT>(out, p0 >> 2, v);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < cnt) dbn_st1<AT>(out, p0 + j, v[j]);
        }
        return;
    }
    const long k = p0 / hw, q = p0 - k * hw;
    if (vec && (hw & 3) == 0) {  // the four pixels share a crop, and every plane starts on a store boundary
#pragma unroll
        for (int c = 0; c < 3; ++c) dbn_st4<AT>(out, ((k * 3 + c) * hw + q) >> 2, f32x4{s_lut[b[c]], s_lut[b[3 + c]], s_lut[b[6 + c]], s_lut[b[9 + c]]});
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= cnt) break;
            const long kj = q + j < hw ? k : (p0 + j) / hw, qj = p0 + j - kj * hw;
#pragma unroll
            for (int c = 0; c < 3; ++c) dbn_st1<AT>(out, (kj * 3 + c) * hw + qj, s_lut[b[3 * j + c]]);
        }
    }
}

// ---- greedy decode: launch 1 -------------------------------------------------------------------------------------------
struct Best {  // running maximum, its smallest index, the smallest index of a NaN
    float m;
    int k, nan;
};

__device__ __forceinline__ void best_take(Best& b, float x, int j) {
    if (x != x) b.nan = j < b.nan ? j : b.nan;
    else if (x > b.m || (x == b.m && j < b.k)) b.m = x, b.k = j;
}

template <int G>
__device__ __forceinline__ Best best_fold(Best b) {  // over the G lanes of a team; every lane returns the result
#pragma unroll
    for (int o = G >> 1; o > 0; o >>= 1) {
        const float om = __shfl_xor(b.m, o, 64);
        const int ok = __shfl_xor(b.k, o, 64), on = __shfl_xor(b.nan, o, 64);
        if (om > b.m || (om == b.m && ok < b.k)) b.m = om, b.k = ok;
        b.nan = on < b.nan ? on : b.nan;
    }
    return b;
}

template <int G>
__device__ __forceinline__ float sum_fold(float s) {
#pragma unroll
    for (int o = G >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

// LDS bytes of rec_step_small: a workgroup's rows (at most RC_THREADS / G rows of RC_PER_LANE * G elements, G >= 1) plus the
// 15 bytes that mirror the run's misalignment in global memory, rounded up
constexpr int RC_SMALL_LDS = RC_THREADS * RC_PER_LANE * 4 + 16;

template <int AT, int G>
__global__ void __launch_bounds__(RC_THREADS) rec_step_small_kernel(const void* __restrict__ x, long n_rows, int C, int* __restrict__ ws_k,
                                                                     float* __restrict__ ws_p) {
    constexpr int ES = dbn_esize(AT), ROWS = RC_THREADS / G;
    __shared__ __attribute__((aligned(16))) unsigned char s_raw[RC_SMALL_LDS];
    const int t = threadIdx.x;
    const long r0 = (long)blockIdx.x * ROWS;
    const int rows = n_rows - r0 < ROWS ? (int)(n_rows - r0) : ROWS;
    const unsigned char* g = reinterpret_cast<const unsigned char*>(x) + r0 * C * ES;
    const int nbytes = rows * C * ES;  // <= ROWS * 8 G * 4 = 8192
    const int mis = (int)(reinterpret_cast<size_t>(g) & 15);  // a multiple of ES; LDS byte mis + i mirrors global byte i
    int head = (16 - mis) & 15;
    head = head < nbytes ? head : nbytes;
    const int nvec = (nbytes - head) >> 4, tail0 = head + (nvec << 4);
    for (int i = t * ES; i < head; i += RC_THREADS * ES) {
        if constexpr (ES == 4) *reinterpret_cast<unsigned*>(s_raw + mis + i) = *reinterpret_cast<const unsigned*>(g + i);
        else *reinterpret_cast<unsigned short*>(s_raw + mis + i) = *reinterpret_cast<const unsigned short*>(g + i);
    }
    {
        const uint4* g4 = reinterpret_cast<const uint4*>(g + head);
        uint4* s4 = reinterpret_cast<uint4*>(s_raw + mis + head);  // mis + head is 0 or 16
        for (int v = t; v < nvec; v += RC_THREADS) s4[v] = g4[v];
    }
    for (int i = tail0 + t * ES; i < nbytes; i += RC_THREADS * ES) {
        if constexpr (ES == 4) *reinterpret_cast<unsigned*>(s_raw + mis + i) = *reinterpret_cast<const unsigned*>(g + i);
        else *reinterpret_cast<unsigned short*>(s_raw + mis + i) = *reinterpret_cast<const unsigned short*>(g + i);
    }
    __syncthreads();
    const int row = t / G, l = t % G;
    const bool live = row < rows;
    const void* srow = s_raw + mis + (live ? row : 0) * C * ES;
    float v[RC_PER_LANE];
    Best b = {-INFINITY, RC_NONE, RC_NONE};
#pragma unroll
    for (int i = 0; i < RC_PER_LANE; ++i) {
        const int j = l + i * G;
        if (live && j < C) {
            v[i] = dbn_ld1<AT>(srow, j);
            best_take(b, v[i], j);
        }
    }
    b = best_fold<G>(b);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < RC_PER_LANE; ++i)
        if (live && l + i * G < C) s += expf(v[i] - b.m);
    s = sum_fold<G>(s);
    if (live && l == 0) {
        ws_k[r0 + row] = b.nan != RC_NONE ? b.nan : b.k;
        ws_p[r0 + row] = 1.0f / s;
    }
}

// one wave per row.  lengths (optional): a row at step t >= lengths[b] is never read by launch 2 and is skipped.
template <int AT>
__global__ void __launch_bounds__(RC_THREADS) rec_step_wide_kernel(const void* __restrict__ x, long n_rows, int T, int C, const int* __restrict__ lengths,
                                                                    int* __restrict__ ws_k, float* __restrict__ ws_p) {
    constexpr int ES = dbn_esize(AT), EPV = 16 / ES;
    const long r = (long)blockIdx.x * (RC_THREADS / 64) + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    if (lengths) {
        const long bq = r / T;
        if ((int)(r - bq * T) >= lengths[bq]) return;
    }
    const int lane = threadIdx.x & 63;
    const unsigned char* g = reinterpret_cast<const unsigned char*>(x) + r * C * ES;
    const int mis = (int)(reinterpret_cast<size_t>(g) & 15);
    int head = ((16 - mis) & 15) / ES;  // elements before the first 16-byte boundary: < EPV <= 8
    head = head < C ? head : C;
    const int nvec = (C - head) / EPV, tail0 = head + nvec * EPV, tail = C - tail0;  // tail < EPV
    const void* body = g + head * ES;

    Best b = {-INFINITY, RC_NONE, RC_NONE};
    if (lane < head) best_take(b, dbn_ld1<AT>(g, lane), lane);
    for (int v = lane; v < nvec; v += 64) {
        f32x4 q[dbn_quads<AT>::Q];
        dbn_ldq<AT>(body, v, q);
#pragma unroll
        for (int e = 0; e < EPV; ++e) best_take(b, q[e >> 2][e & 3], head + v * EPV + e);
    }
    if (lane < tail) best_take(b, dbn_ld1<AT>(g, tail0 + lane), tail0 + lane);
    b = best_fold<64>(b);

    float s = 0.f;
    if (lane < head) s += expf(dbn_ld1<AT>(g, lane) - b.m);
    for (int v = lane; v < nvec; v += 64) {
        f32x4 q[dbn_quads<AT>::Q];
        dbn_ldq<AT>(body, v, q);
#pragma unroll
        for (int e = 0; e < EPV; ++e) s += expf(q[e >> 2][e & 3] - b.m);
    }
    if (lane < tail) s += expf(dbn_ld1<AT>(g, tail0 + lane) - b.m);
    s = sum_fold<64>(s);
    if (lane == 0) {
        ws_k[r] = b.nan != RC_NONE ? b.nan : b.k;
        ws_p[r] = 1.0f / s;
    }
}

// ---- greedy decode: launch 2 -------------------------------------------------------------------------------------------
// mode 0 (ctc): step t is kept iff k_t != blank and (t == 0 or k_t != k_{t-1}); the score runs over all len steps.
// mode 1 (attn): the steps before the first k_t == eos are kept, and the score runs over them (1.0 for none).
__global__ void __launch_bounds__(RC_THREADS) rec_collapse_kernel(const int* __restrict__ ws_k, const float* __restrict__ ws_p, int B, int T,
                                                                   const int* __restrict__ lengths, int mode, int special, int* __restrict__ codes,
                                                                   int* __restrict__ count, float* __restrict__ score) {
    const int bq = blockIdx.x * (RC_THREADS / 64) + (threadIdx.x >> 6);
    if (bq >= B) return;
    const int lane = threadIdx.x & 63;
    int len = lengths ? lengths[bq] : T;
    len = len < 0 ? 0 : (len > T ? T : len);
    const int* k = ws_k + (long)bq * T;
    const float* p = ws_p + (long)bq * T;
    int* out = codes + (long)bq * T;
    float sc = 1.f;
    int n_kept = 0, carry = -1;
    bool done = false;
    for (int base = 0; base < len && !done; base += 64) {
        const int t = base + lane;
        const bool valid = t < len;
        const int kt = valid ? k[t] : -1;
        const float pt = valid ? p[t] : 1.f;
        int n = len - base < 64 ? len - base : 64;  // steps of this chunk that enter the score
        bool keep;
        if (mode == 1) {
            const unsigned long long eos = __ballot(valid && kt == special);
            if (eos) n = __builtin_ctzll(eos), done = true;
            keep = lane < n;
        } else {
            int prev = __shfl_up(kt, 1, 64);
            if (lane == 0) prev = carry;
            keep = valid && kt != special && (t == 0 || kt != prev);
            carry = __shfl(kt, 63, 64);
        }
        for (int i = 0; i < n; ++i) sc *= __shfl(pt, i, 64);
        const unsigned long long kept = __ballot(keep);
        if (keep) out[n_kept + __builtin_popcountll(kept & ((1ull << lane) - 1ull))] = kt;
        n_kept += __builtin_popcountll(kept);
    }
    for (int t = n_kept + lane; t < T; t += 64) out[t] = -1;
    if (lane == 0) {
        count[bq] = n_kept;
        score[bq] = sc;
    }
}

template <int AT>
int launch_step(const void* x, long n_rows, int T, int C, const int* lengths, int* ws_k, float* ws_p, hipStream_t st) {
    if (C > RC_SMALL_C) {
        const long blocks = (n_rows + RC_THREADS / 64 - 1) / (RC_THREADS / 64);
        DBN_REQUIRE(blocks <= 2147483647L);
        hipLaunchKernelGGL(rec_step_wide_kernel<AT>, dim3((unsigned)blocks), dim3(RC_THREADS), 0, st, x, n_rows, T, C, lengths, ws_k, ws_p);
        return DBN_OK;
    }
    int G = 1;  // the smallest team whose RC_PER_LANE elements per lane cover the row
    while (G * RC_PER_LANE < C) G <<= 1;
    const long rows = RC_THREADS / G, blocks = (n_rows + rows - 1) / rows;
    DBN_REQUIRE(blocks <= 2147483647L);
    const dim3 grid((unsigned)blocks), block(RC_THREADS);
#define RC_LAUNCH_SMALL(G_) hipLaunchKernelGGL((rec_step_small_kernel<AT, G_>), grid, block, 0, st, x, n_rows, C, ws_k, ws_p)
    switch (G) {
        case 1: RC_LAUNCH_SMALL(1); break;
        case 2: RC_LAUNCH_SMALL(2); break;
        case 4: RC_LAUNCH_SMALL(4); break;
        case 8: RC_LAUNCH_SMALL(8); break;
        case 16: RC_LAUNCH_SMALL(16); break;
        case 32: RC_LAUNCH_SMALL(32); break;
        default: RC_LAUNCH_SMALL(64); break;
    }
#undef RC_LAUNCH_SMALL
    return DBN_OK;
}

}  // namespace

extern "C" {

int dbn_words_to_input(int at, const unsigned char* crops, long n_px, long hw, int rgb, int bgr, const float* lut, void* out, void* stream) {
    DBN_REQUIRE(crops && lut && out && n_px > 0 && hw > 0 && n_px % hw == 0);
    const long blocks = ((n_px + 3) / 4 + RC_THREADS - 1) / RC_THREADS;
    DBN_REQUIRE(blocks <= 2147483647L);
    const int aligned = ((reinterpret_cast<size_t>(crops) & 3) == 0 ? 1 : 0) | ((reinterpret_cast<size_t>(out) & 15) == 0 ? 2 : 0);
    DBN_DISPATCH_AT(at, hipLaunchKernelGGL(words_to_input_kernel<AT>, dim3((unsigned)blocks), dim3(RC_THREADS), 0, (hipStream_t)stream, crops, n_px,
                                           hw, rgb, bgr, lut, out, aligned));
    return dbn_status();
}

long dbn_greedy_decode_ws_bytes(int B, int T) { return B > 0 && T > 0 ? (long)B * T * 8 : 0; }

int dbn_greedy_decode(int at, const void* logits, int B, int T, int C, const int* lengths, int mode, void* ws, int* codes, int* count,
                      float* score, void* stream) {
    DBN_REQUIRE(logits && ws && codes && count && score && B > 0 && T > 0 && C > 0 && (mode == 0 || mode == 1));
    DBN_REQUIRE((reinterpret_cast<size_t>(logits) & (at == 0 ? 3u : 1u)) == 0 && (reinterpret_cast<size_t>(ws) & 3) == 0);
    const long n_rows = (long)B * T;
    int* ws_k = reinterpret_cast<int*>(ws);
    float* ws_p = reinterpret_cast<float*>(ws) + n_rows;
    int rc = DBN_OK;
    DBN_DISPATCH_AT(at, rc = launch_step<AT>(logits, n_rows, T, C, lengths, ws_k, ws_p, (hipStream_t)stream));
    if (rc != DBN_OK) return rc;
    hipLaunchKernelGGL(rec_collapse_kernel, dim3((unsigned)((B + RC_THREADS / 64 - 1) / (RC_THREADS / 64))), dim3(RC_THREADS), 0, (hipStream_t)stream,
                       ws_k, ws_p, B, T, lengths, mode, mode == 1 ? 1 : 0, codes, count, score);
    return dbn_status();
}

}  // extern "C"
