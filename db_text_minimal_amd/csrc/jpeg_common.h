// What every stage of the JPEG pipeline agrees on (jpeg.hip, jpeg_enc.hip, jpeg_huff.hip, jpeg_dhuff.hip), defined once: the
// int64 [N][24] descriptor and the one function that turns it into checked scan geometry, on the host and in a kernel alike;
// the zigzag order; the canonical Huffman code ranges of 16 counts; the host thread pool of the batch entry points.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <thread>
#include <vector>

namespace dbn_jpeg {

constexpr int JP_DESC = 24;  // int64 per image, see include/dbnet_hip.h
enum { D_COEF = 0, D_W, D_H, D_NC, D_OUT, D_QT, D_COMP /* 4 per component: bw, bh, h, v */, D_HMAX = 18, D_VMAX, D_MCUX, D_MCUY, D_STATUS, D_RI };

// natural index of zigzag position k: the same 64 numbers as a host table and as a device table
#define DBN_JPEG_ZIGZAG                                                                                                                  \
    {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, \
     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}
const unsigned char kZigzag[64] = DBN_JPEG_ZIGZAG;
__device__ constexpr unsigned char kZZ[64] = DBN_JPEG_ZIGZAG;

// The scan geometry of a descriptor.  Scalars only: a member array that a kernel indexes at run time would put the struct
// into scratch memory.
struct Scan {
    long long coef, off1, off2, blocks, mcus;  // first coefficient; Cb's and Cr's blocks from it; blocks and MCUs of the image
    int nc, hs, vs, mcux, mcuy, nl, bpm;       // components, luma sampling, the MCU grid, luma blocks and blocks per MCU
};

// A descriptor is followed only if its status is 0, its size 1 .. 65535 a side, its components 1 or 3, its luma sampling
// 1 x 1 (or 2 x 1 / 2 x 2 for three components) with 1 x 1 chroma, its grids exactly the ones that size and sampling give, and
// [coef, coef + blocks * 64) inside coef_elems.  What only some callers ask (the alignment of coef, the restart interval, the
// tables, the pixels) is theirs to check.
__host__ __device__ __forceinline__ bool read_scan(const long long* __restrict__ d, long long coef_elems, Scan& g) {
    if (d[D_STATUS] != 0) return false;
    const long long W = d[D_W], H = d[D_H], nc = d[D_NC];
    if (W < 1 || H < 1 || W > 65535 || H > 65535 || (nc != 1 && nc != 3)) return false;
    const long long h0 = d[D_COMP + 2], v0 = d[D_COMP + 3];
    if (!((h0 == 1 && v0 == 1) || (nc == 3 && h0 == 2 && (v0 == 1 || v0 == 2)))) return false;
    g.nc = (int)nc, g.hs = (int)h0, g.vs = (int)v0;  // int from here on: a kernel pays for every 64-bit division
    g.mcux = ((int)W + 8 * g.hs - 1) / (8 * g.hs), g.mcuy = ((int)H + 8 * g.vs - 1) / (8 * g.vs);
    g.mcus = (long long)g.mcux * g.mcuy;
    if (d[D_COMP] != g.mcux * g.hs || d[D_COMP + 1] != g.mcuy * g.vs) return false;
    for (int c = 1; c < nc; ++c)
        if (d[D_COMP + 4 * c] != g.mcux || d[D_COMP + 4 * c + 1] != g.mcuy || d[D_COMP + 4 * c + 2] != 1 || d[D_COMP + 4 * c + 3] != 1) return false;
    g.nl = nc == 3 ? g.hs * g.vs : 1;
    g.bpm = nc == 3 ? g.nl + 2 : 1;
    g.off1 = g.mcus * g.nl * 64, g.off2 = g.off1 + g.mcus * 64;
    g.blocks = g.mcus * g.bpm;
    g.coef = d[D_COEF];
    return g.coef >= 0 && g.coef + g.blocks * 64 <= coef_elems;
}

// element offset of block j of an MCU (luma blocks row by row, then Cb, Cr); always inside [g.coef, g.coef + g.blocks * 64)
// for 0 <= mcu < g.mcus and 0 <= j < g.bpm
__host__ __device__ __forceinline__ long long block_at(const Scan& g, long long mcu, int j) {
    const long long my = mcu / g.mcux, mx = mcu - my * g.mcux;
    if (j < g.nl) {
        const int v = j / g.hs, u = j - v * g.hs;
        return g.coef + ((my * g.vs + v) * ((long long)g.mcux * g.hs) + mx * g.hs + u) * 64;
    }
    return g.coef + (j == g.nl ? g.off1 : g.off2) + mcu * 64;
}

// The canonical code of a DHT segment's 16 counts: per length l = 1 .. 16 the least and the greatest code (-1: none) and the
// index of its first symbol; entry 0 is the empty length.  *nvals: the symbols.  false: the counts are not a prefix code.
__host__ __device__ __forceinline__ bool code_ranges(const unsigned char* counts, int* mincode, int* maxcode, int* first, int* nvals) {
    int code = 0, k = 0;
    bool ok = true;
    mincode[0] = 0, maxcode[0] = -1, first[0] = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = counts[l - 1];
        if (code + n > (1 << l)) ok = false;
        mincode[l] = code, maxcode[l] = n ? code + n - 1 : -1, first[l] = k;
        code = (code + n) << 1;
        k += n;
    }
    *nvals = k;
    return ok;
}

// f(n) for n = 0 .. N - 1 on min(N, 16, threads) host threads (the caller's among them), handed out over one counter
template <typename F>
void on_threads(int N, int threads, F f) {
    int T = threads < 1 ? 1 : (threads > 16 ? 16 : threads);
    T = T > N ? N : T;
    std::atomic<int> next(0);
    auto work = [&]() {
        for (int n; (n = next.fetch_add(1)) < N;) f(n);
    };
    std::vector<std::thread> pool;
    for (int i = 1; i < T; ++i) pool.emplace_back(work);
    work();
    for (auto& th : pool) th.join();
}

}  // namespace dbn_jpeg
