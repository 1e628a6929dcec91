// Degradation augmentation of a packed uint8 RGB batch (db_text_minimal_amd/degrade.py; ABI and the record: include/dbnet_hip.h; the
// definition: DESIGN.md section 40): a Gaussian blur with a per-image radius, then additive Gaussian noise on the blurred byte, all in
// exact integers, in one launch.  A workgroup takes one tile of the host-built list:
//   an image with r = 0     a run of DG_RUN pixels in row-major order: 12 bytes (four pixels) per lane through the noise and out again,
//                           no LDS, no barrier (the last one to three pixels of the image byte by byte);
//   an image with r > 0     DG_TH x DG_TW output pixels.  (1) the tile and its halo of r pixels, the border mirrored, go to LDS as three
//                           byte planes; (2) the horizontal pass reads them four taps at a time (v_dot4_u32_u8 on the low and on the
//                           high byte of the 16-bit weights) and leaves 24-bit row sums in LDS; (3) the vertical pass walks a column of
//                           eight outputs over its 8 + 2 r row sums, each split into two 12-bit halves so that both products of a tap
//                           stay 24 x 24 -> 32-bit multiply-adds, joins the halves in 64 bits, rounds, and puts the byte into LDS in the
//                           order of the image; (4) rows of the tile leave through the noise as the runs do.
// The wide intermediate exists in LDS only.  Every address is formed from record and tile values that the host entry point has checked
// against the buffer length before the launch: the tile list must be the canonical one of its records.
#include "common.h"

namespace {

constexpr int DG_D = 25;  // int64 fields of an image's record
enum { DG_OFF = 0, DG_H = 1, DG_W = 2, DG_TILE = 3, DG_R = 4, DG_NOISE = 5, DG_SEED = 6, DG_TAPS = 8 };
// 768 lanes: the 3 x 64 columns x 4 strips of pass 3 in one round, and three waves per SIMD where r = 32 leaves room for one workgroup
constexpr int DG_TW = 64, DG_TH = 32, DG_RMAX = 32, DG_THREADS = 768, DG_STRIP = 8, DG_RUN = 4 * DG_THREADS;
constexpr int DG_GROUPS = (2 * DG_RMAX + 1 + 3) / 4;        // tap groups of four, at most
constexpr int DG_WINDOW = DG_STRIP + 2 * DG_RMAX;           // row sums under a column strip, at most
constexpr long DG_MAX_IMAGES = 65535, DG_MAX_SIDE = 16384;
constexpr unsigned DG_M0 = 0xD2511F53u, DG_M1 = 0xCD9E8D57u, DG_W0 = 0x9E3779B9u, DG_W1 = 0xBB67AE85u;

// three dwords at any byte alignment
struct __attribute__((packed, aligned(1))) dg_bytes12 {
    unsigned w[3];
};

struct dg_noise {
    int s8;  // round(256 scale); 0: no noise
    bool per_channel;
    unsigned k0, k1;
};

__host__ __device__ constexpr int dg_row_bytes(int r) { return (DG_TW + 2 * r + 4 + 3) & ~3; }  // one row of a byte plane (see pass 2)
__host__ __device__ constexpr int dg_plane_bytes(int r) { return (3 * (DG_TH + 2 * r) * dg_row_bytes(r) + 15) & ~15; }
constexpr int DG_HEAD = DG_WINDOW + 2 * ((DG_GROUPS + 3) & ~3);  // dwords of weights in front of the planes: a multiple of four
__host__ __device__ constexpr int dg_lds_bytes(int r) { return 4 * DG_HEAD + dg_plane_bytes(r) + 3 * (DG_TH + 2 * r) * DG_TW * 4; }

// scipy's 'mirror': period 2 (n - 1), the edge pixel not repeated; n = 1 maps every index to 0
__device__ __forceinline__ int dg_mirror(int i, int n) {
    if ((unsigned)i < (unsigned)n) return i;  // inside: no division
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    int m = i % p;
    if (m < 0) m += p;
    return m >= n ? p - m : m;
}

// words 0 .. 2 of the Philox4x32-10 block of counter (g, 0, 0, 0)
__device__ __forceinline__ void dg_philox(unsigned g, unsigned k0, unsigned k1, unsigned (&w)[3]) {
    unsigned c0 = g, c1 = 0, c2 = 0, c3 = 0;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned long long p0 = (unsigned long long)DG_M0 * c0, p1 = (unsigned long long)DG_M1 * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1, c3 = (unsigned)p0, c0 = n0, c2 = n2;
        k0 += DG_W0, k1 += DG_W1;
    }
    w[0] = c0, w[1] = c1, w[2] = c2;
}

// the three bytes of pixel g of its image after the noise
__device__ __forceinline__ void dg_noise_pixel(const dg_noise& nz, const short* __restrict__ Z, unsigned g, int (&c)[3]) {
    unsigned w[3];
    dg_philox(g, nz.k0, nz.k1, w);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int z = Z[(nz.per_channel ? w[k] : w[0]) >> 20];
        const int v = c[k] + ((z * nz.s8 + (1 << 19)) >> 20);  // |z| <= 15025, s8 <= 16384: int32; >> of a negative value is floor
        c[k] = v < 0 ? 0 : v > 255 ? 255 : v;
    }
}

// four pixels, g .. g + 3 of their image, as 12 bytes
__device__ __forceinline__ dg_bytes12 dg_noise_four(const dg_noise& nz, const short* __restrict__ Z, unsigned g, const dg_bytes12& in) {
    dg_bytes12 out = {{0u, 0u, 0u}};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = (int)((in.w[(3 * j + k) >> 2] >> (8 * ((3 * j + k) & 3))) & 255u);
        dg_noise_pixel(nz, Z, g + j, c);
#pragma unroll
        for (int k = 0; k < 3; ++k) out.w[(3 * j + k) >> 2] |= (unsigned)c[k] << (8 * ((3 * j + k) & 3));
    }
    return out;
}

// pixels g .. g + 3 of the image at dst, held in v, through the noise and out with one 12-byte store at any alignment
__device__ __forceinline__ void dg_emit_four(const dg_noise& nz, const short* __restrict__ Z, dg_bytes12 v, unsigned char* dst, unsigned g) {
    if (nz.s8) v = dg_noise_four(nz, Z, g, v);
    *reinterpret_cast<dg_bytes12*>(dst + 3 * (long)g) = v;
}

// `count` pixels (1 .. 3) from g on, byte by byte from `from` (global or LDS): the end of an image or of a tile's row
__device__ __forceinline__ void dg_emit_tail(const dg_noise& nz, const short* __restrict__ Z, const unsigned char* from, unsigned char* dst, unsigned g,
                                             int count) {
    for (int j = 0; j < count; ++j) {
        int c[3] = {from[3 * j], from[3 * j + 1], from[3 * j + 2]};
        if (nz.s8) dg_noise_pixel(nz, Z, g + j, c);
        unsigned char* o = dst + 3 * (long)(g + j);
        o[0] = (unsigned char)c[0], o[1] = (unsigned char)c[1], o[2] = (unsigned char)c[2];
    }
}

__global__ __launch_bounds__(DG_THREADS) void degrade_kernel(const unsigned char* __restrict__ in, unsigned char* __restrict__ out,
                                                             const long long* __restrict__ desc, const int* __restrict__ tiles,
                                                             const short* __restrict__ Z) {
    extern __shared__ __attribute__((aligned(16))) unsigned dg_lds[];  // all of the kernel's LDS, every part a multiple of 16 bytes
    // (everything up to the lane's own indices is the same in all lanes of the workgroup)
    const int* tile = tiles + 3 * (long)blockIdx.x;
    const long long* d = desc + (long)tile[0] * DG_D;
    const int a = tile[1], b = tile[2];
    const int H = (int)d[DG_H], W = (int)d[DG_W], r = (int)d[DG_R];
    const unsigned long long seed = (unsigned long long)d[DG_SEED];
    const dg_noise nz = {(int)(d[DG_NOISE] & 0xFFFFFFFFll), (d[DG_NOISE] >> 32 & 1) != 0, (unsigned)seed, (unsigned)(seed >> 32)};
    const unsigned char* src = in + d[DG_OFF];
    unsigned char* dst = out + d[DG_OFF];
    const int tid = threadIdx.x;

    if (r == 0) {  // a run of pixels from a: no stencil
        const int pixels = H * W;
#pragma unroll
        for (int s = 0; s < DG_RUN / (4 * DG_THREADS); ++s) {
            const int g = a + 4 * (s * DG_THREADS + tid);
            if (g + 4 <= pixels)
                dg_emit_four(nz, Z, *reinterpret_cast<const dg_bytes12*>(src + 3 * (long)g), dst, (unsigned)g);
            else if (g < pixels)
                dg_emit_tail(nz, Z, src + 3 * (long)g, dst, (unsigned)g, pixels - g);
        }
        return;
    }

    const int rows = DG_TH + 2 * r, cols = DG_TW + 2 * r, stride = dg_row_bytes(r);
    unsigned *s_q = dg_lds, *s_qlo = dg_lds + DG_WINDOW, *s_qhi = s_qlo + ((DG_GROUPS + 3) & ~3);
    unsigned char* plane = reinterpret_cast<unsigned char*>(dg_lds + DG_HEAD);  // [3][rows][stride] bytes: the tile and its halo
    unsigned* sums = dg_lds + DG_HEAD + dg_plane_bytes(r) / 4;                  // [3][rows][DG_TW] row sums, < 2^24

    // the window of weights q[|t - r|], t = 0 .. 2 r, zero behind it: as dwords for pass 3, as low and high bytes for pass 2
    if (tid < DG_WINDOW) {
        const unsigned* taps = reinterpret_cast<const unsigned*>(d + DG_TAPS);
        const unsigned q = tid <= 2 * r ? taps[tid < r ? r - tid : tid - r] : 0u;  // < 65536 (checked by the host)
        s_q[tid] = q;
        if (tid < 4 * DG_GROUPS) {
            reinterpret_cast<unsigned char*>(s_qlo)[tid] = (unsigned char)(q & 255u);
            reinterpret_cast<unsigned char*>(s_qhi)[tid] = (unsigned char)(q >> 8);
        }
    }

    // pass 1: 32 lanes take a row of the window, a lane the same four neighbouring columns in every row it meets (columns behind `cols`
    // lie inside the row's stride and are never used).  Where the four lie side by side in the image they come as one 12-byte load;
    // at a mirrored border byte by byte.
    {
        const int wx = 4 * (tid & 31), x = b - r + wx;
        const bool straight = x >= 0 && x + 3 < W;
        int mx[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) mx[j] = 3 * dg_mirror(x + j, W);
        if (wx < cols) {
#pragma unroll 2
            for (int wy = tid >> 5; wy < rows; wy += DG_THREADS / 32) {
                const unsigned char* row = src + 3 * (long)dg_mirror(a - r + wy, H) * W;
                unsigned p[3] = {0u, 0u, 0u};
                if (straight) {
                    const dg_bytes12 v = *reinterpret_cast<const dg_bytes12*>(row + 3 * x);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int k = 0; k < 3; ++k) p[k] |= ((v.w[(3 * j + k) >> 2] >> (8 * ((3 * j + k) & 3))) & 255u) << (8 * j);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int k = 0; k < 3; ++k) p[k] |= (unsigned)row[mx[j] + k] << (8 * j);
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) *reinterpret_cast<unsigned*>(plane + (k * rows + wy) * stride + wx) = p[k];
            }
        }
    }
    __syncthreads();

    // pass 2: an item is four consecutive row sums of one row of one plane.  Output x takes the bytes x .. x + 2 r of its row; group g
    // holds taps 4 g .. 4 g + 3, so the item reads dwords x / 4 .. x / 4 + groups: up to byte 63 + 4 groups < stride, and whatever lies
    // behind column `cols` meets a zero weight.
    {
        const int groups = (2 * r + 1 + 3) / 4;
        for (int item = tid; item < 3 * rows * (DG_TW / 4); item += DG_THREADS) {
            const int xg = item & (DG_TW / 4 - 1), row = item >> 4;  // row = plane * rows + wy
            const unsigned* from = reinterpret_cast<const unsigned*>(plane + row * stride) + xg;
            unsigned lo[4] = {0u, 0u, 0u, 0u}, hi[4] = {0u, 0u, 0u, 0u};
            unsigned d0 = from[0];
            for (int g = 0; g < groups; ++g) {
                const unsigned d1 = from[g + 1], wl = s_qlo[g], wh = s_qhi[g];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned w = k ? __builtin_amdgcn_alignbyte(d1, d0, k) : d0;
                    lo[k] = __builtin_amdgcn_udot4(w, wl, lo[k], false);
                    hi[k] = __builtin_amdgcn_udot4(w, wh, hi[k], false);
                }
                d0 = d1;
            }
            uint4 v;
            v.x = lo[0] + (hi[0] << 8), v.y = lo[1] + (hi[1] << 8), v.z = lo[2] + (hi[2] << 8), v.w = lo[3] + (hi[3] << 8);
            reinterpret_cast<uint4*>(sums + row * DG_TW)[xg] = v;
        }
    }
    __syncthreads();

    // pass 3: an item is DG_STRIP outputs below each other in one column of one plane.  Row sum t of its window meets output k with
    // weight q[t - k]: the eight weights in use slide by one per row sum (they are the same in every lane).  h = hh 2^12 + hl with both
    // halves < 2^12, so sum(q hl) and sum(q hh) stay below 2^16 * 2^12.
    {
        unsigned char* bytes = plane;  // [DG_TH][DG_TW][3]: pass 2 has read the planes, the tile's result takes their place
        for (int item = tid; item < 3 * DG_TW * (DG_TH / DG_STRIP); item += DG_THREADS) {
            const int strip = item / (3 * DG_TW), col = item - strip * (3 * DG_TW);  // col = plane * DG_TW + x; one strip per wave
            const int k3 = col >> 6, x = col & (DG_TW - 1);
            const unsigned* from = sums + (k3 * rows + strip * DG_STRIP) * DG_TW + x;
            unsigned accl[DG_STRIP], acch[DG_STRIP], wq[DG_STRIP];
#pragma unroll
            for (int k = 0; k < DG_STRIP; ++k) accl[k] = acch[k] = wq[k] = 0u;
            for (int t = 0; t < DG_STRIP + 2 * r; ++t) {
                const unsigned h = from[t * DG_TW], hl = h & 0xFFFu, hh = h >> 12;
#pragma unroll
                for (int k = DG_STRIP - 1; k > 0; --k) wq[k] = wq[k - 1];
                wq[0] = __builtin_amdgcn_readfirstlane(s_q[t]);
#pragma unroll
                for (int k = 0; k < DG_STRIP; ++k) {
                    accl[k] += __umul24(wq[k], hl);
                    acch[k] += __umul24(wq[k], hh);
                }
            }
#pragma unroll
            for (int k = 0; k < DG_STRIP; ++k) {
                const unsigned long long S = ((unsigned long long)acch[k] << 12) + accl[k];
                bytes[((strip * DG_STRIP + k) * DG_TW + x) * 3 + k3] = (unsigned char)((S + (1ull << 31)) >> 32);
            }
        }
    }
    __syncthreads();

    // pass 4: sixteen lanes per row of the tile, four pixels each, through the noise to the image
    {
        const int th = H - a < DG_TH ? H - a : DG_TH, tw = W - b < DG_TW ? W - b : DG_TW;
        const int x = 4 * (tid & 15);
        if (x < tw)
            for (int y = tid >> 4; y < th; y += DG_THREADS / 16) {
                const unsigned g = (unsigned)((a + y) * W + b + x);
                const unsigned* from = reinterpret_cast<const unsigned*>(plane) + (y * DG_TW + x) * 3 / 4;  // 12 bytes from a multiple of 12
                if (x + 4 <= tw)
                    dg_emit_four(nz, Z, dg_bytes12{{from[0], from[1], from[2]}}, dst, g);
                else
                    dg_emit_tail(nz, Z, reinterpret_cast<const unsigned char*>(from), dst, g, tw - x);
            }
    }
}

// Every value the kernel bounds a loop or forms an address with, against the length of the buffers; the tile list must be the one
// these records imply, tile for tile -> the largest radius of the batch
int dg_validate(const long long* hdesc, int N, long bytes, const int* htiles, long T, int* rmax) {
    DBN_REQUIRE(hdesc && htiles && N >= 1 && N <= DG_MAX_IMAGES && bytes > 0 && T >= 1 && T <= 0x7FFFFFFFl);
    long end = 0, tile = 0;
    *rmax = 0;
    for (int n = 0; n < N; ++n) {
        const long long* d = hdesc + (long)n * DG_D;
        const long h = d[DG_H], w = d[DG_W], r = d[DG_R];
        DBN_REQUIRE(h >= 1 && h <= DG_MAX_SIDE && w >= 1 && w <= DG_MAX_SIDE && r >= 0 && r <= DG_RMAX);
        DBN_REQUIRE(d[DG_OFF] >= end && d[DG_OFF] <= bytes && 3 * h * w <= bytes - d[DG_OFF]);  // in order: no two images overlap
        end = d[DG_OFF] + 3 * h * w;
        DBN_REQUIRE((d[DG_NOISE] & 0xFFFFFFFFll) <= 64 * 256 && (unsigned long long)d[DG_NOISE] >> 33 == 0);
        const unsigned* taps = reinterpret_cast<const unsigned*>(d + DG_TAPS);
        if (r > 0) {  // 16-bit weights that sum to 2^16: what the byte split of pass 2 and the bounds of pass 3 rest on
            unsigned long sum = taps[0];
            for (int i = 0; i <= DG_RMAX; ++i) {
                DBN_REQUIRE(taps[i] < 65536u && (i <= r || taps[i] == 0u));
                if (i > 0) sum += 2ul * taps[i];
            }
            DBN_REQUIRE(sum == 65536ul);
            if (r > *rmax) *rmax = (int)r;
        }
        DBN_REQUIRE(d[DG_TILE] == tile);
        const long across = (w + DG_TW - 1) / DG_TW;
        const long count = r > 0 ? across * ((h + DG_TH - 1) / DG_TH) : (h * w + DG_RUN - 1) / DG_RUN;
        DBN_REQUIRE(count <= T - tile);
        for (long k = 0; k < count; ++k) {
            const int* t = htiles + 3 * (tile + k);
            DBN_REQUIRE(t[0] == n && t[1] == (r > 0 ? k / across * DG_TH : k * DG_RUN) && t[2] == (r > 0 ? k % across * DG_TW : 0));
        }
        tile += count;
    }
    DBN_REQUIRE(tile == T);
    return DBN_OK;
}

}  // namespace

int dbn_degrade_u8(const unsigned char* in, unsigned char* out, long bytes, const long long* hdesc, const long long* desc, int N, const int* htiles,
                   const int* tiles, long T, const short* normal, void* stream) {
    int rmax = 0;
    const int rc = dg_validate(hdesc, N, bytes, htiles, T, &rmax);
    if (rc != DBN_OK) return rc;
    DBN_REQUIRE(in && out && desc && tiles && normal && (out + bytes <= in || in + bytes <= out));
    const int lds = rmax > 0 ? dg_lds_bytes(rmax) : 0;  // sized by the largest radius of the batch
    if (lds > 48 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(degrade_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
        return dbn_status();
    hipLaunchKernelGGL(degrade_kernel, dim3((unsigned)T), dim3(DG_THREADS), (size_t)lds, (hipStream_t)stream, in, out, desc, tiles, normal);
    return dbn_status();
}
