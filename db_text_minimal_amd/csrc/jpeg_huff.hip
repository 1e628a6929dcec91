// Huffman coding of JPEG scans on the device: the last stage of the encode (jpeg_enc.hip) without the coefficients crossing
// to the host.  Input is the coefficient layout of dbn_jpeg_entropy_batch / dbn_jpeg_forward in device memory; output is
// every image's entropy-coded segment (FF00 stuffing, RSTn markers, ones-padded intervals), image after image in one compact
// buffer, and its length.  Headers and EOI stay on the host (dbn_jpeg_huff_headers, the writer of jpeg_enc.hip).
//
// The unit of work is a block in SCAN order: g = blk_base[image] + MCU * blocks_per_MCU + j over the whole batch.  The DC
// predecessor of a block and the first block of its restart interval are address computations, so no pass walks an image.
//   jh_blocks_kernel<HIST>  one lane per block.  HIST: counts the block's symbols into per-image 4 x 256 histograms (LDS
//                           first, integer global atomics after).  Otherwise: the block's length in bits under the
//                           image's code table, and the sum of the workgroup's 256 lengths.
//   jh_scan_sums_kernel     one workgroup: exclusive scan of the per-workgroup sums (64-bit)
//   jh_scan_apply_kernel    P[g]: 64-bit exclusive scan of the bit lengths over the batch, P[total] the sum
//   jh_zero_kernel          zeroes the part of the unstuffed stream and of its marks that this batch reaches
//   jh_write_kernel         one lane per block: codes it again and ORs its bits into the unstuffed stream.  Interval i
//                           (numbered over the batch) starts at byte U(i) = (P[its first block] >> 3) + i: intervals start
//                           on bytes, do not overlap and leave at most one unused byte between them, which the last
//                           block of an interval marks (mark 1); the first block of an interval inside an image marks
//                           its first byte 2 + k for the RSTk in front of it.  Only a block's first and last word can be
//                           shared with a neighbour, and OR commutes: the bytes do not depend on the order of arrival.
//   jh_stuff_count_kernel   a byte's weight is what it becomes in the stream: 0 unused, 1, 2 for FF (FF 00), + 2 behind
//                           an RSTn; sums of 4096-byte chunks, scanned by jh_scan_sums_kernel
//   jh_stuff_scatter_kernel every byte to its place, 00 and RSTn inserted
//   jh_offsets_kernel       where each image's segment starts in the output: the weight of everything before U(first
//                           interval of the image)
// Every address is checked against the buffer it goes into; a descriptor that disagrees with its slice is not followed (the
// image is marked ES_BAD_DESC).  An AC coefficient of more than 10 bits or a DC difference of more than 11 is left out of the
// code, and the image's status becomes the one the host coder gives: the first failing block in scan order decides.
// The descriptor, its checked geometry (read_scan, block_at), the zigzag order and the thread pool are jpeg_common.h's.
#include <string.h>

#include "common.h"
#include "jpeg_enc.h"

using namespace dbn_jpeg;

namespace {

constexpr int JH_THREADS = 256;
constexpr long JH_CHUNK = 4096;  // bytes of the unstuffed stream per workgroup of the stuffing passes, 16 per lane
constexpr int JH_SLOTS = 4;      // images whose histograms a workgroup keeps in LDS
typedef unsigned long long u64;
typedef short short8 __attribute__((ext_vector_type(8)));

// the image of scan block gb: the last n with blk_base[n] <= gb (images without blocks share their successor's base)
__device__ __forceinline__ int find_image(const long long* __restrict__ blk_base, int N, long long gb) {
    int lo = 0, hi = N;  // blk_base[lo] <= gb < blk_base[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (blk_base[mid] <= gb) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct Where {
    Scan g;
    int n, j;
    long long base, mcu, mcu0, k;  // first scan block of the image; the block's MCU; first MCU and number of its interval
};

__device__ __forceinline__ bool locate(const long long* __restrict__ desc, int N, const long long* __restrict__ blk_base, long long total, long coef_elems,
                                       int ri, long long gb, u64* __restrict__ errkey, Where& w) {
    if (gb >= total) return false;
    w.n = find_image(blk_base, N, gb);
    w.base = blk_base[w.n];
    // the kernels load a block as 16-byte vectors; the image has the number of blocks the plan gave it
    if (!read_scan(desc + (long)w.n * JP_DESC, coef_elems, w.g) || (w.g.coef & 7) || w.g.blocks != blk_base[w.n + 1] - w.base) {
        atomicMin(errkey + w.n, (u64)ES_BAD_DESC);
        return false;
    }
    const long long s = gb - w.base;
    w.mcu = s / w.g.bpm, w.j = (int)(s - w.mcu * w.g.bpm);
    w.k = ri > 0 ? w.mcu / ri : 0;
    w.mcu0 = w.k * ri;
    return true;
}

__device__ __forceinline__ int nbits_dev(int v) {
    v = v < 0 ? -v : v;
    return v ? 32 - __clz(v) : 0;
}

// One block handed to `sink` as the host coder's walk_scan hands it: dc(table, category, extra bits), ac(table, run << 4 |
// size, size, extra bits).  -> 0, ES_DC_RANGE or ES_AC_RANGE; what cannot be coded is left out (a DC category 0, a zero AC).
template <typename Sink>
__device__ __forceinline__ int walk_block(const short* __restrict__ coef, const Where& w, Sink& sink) {
    const long long at = block_at(w.g, w.mcu, w.j);
    const int nl = w.g.nl;
    const int t = w.j < nl ? 0 : 1;
    int pred = 0;
    if (w.j > 0 && w.j < nl) pred = coef[block_at(w.g, w.mcu, w.j - 1)];
    else if (w.mcu != w.mcu0) pred = coef[block_at(w.g, w.mcu - 1, w.j < nl ? nl - 1 : w.j)];
    short k64[64];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const short8 v = *reinterpret_cast<const short8*>(coef + at + 8 * r);
#pragma unroll
        for (int e = 0; e < 8; ++e) k64[8 * r + e] = v[e];
    }
    int err = 0;
    const int d = (int)k64[0] - pred;
    int s = nbits_dev(d);
    if (s > 11) err = ES_DC_RANGE, s = 0;
    sink.dc(t, s, (unsigned)(d < 0 ? d - 1 : d) & ((1u << s) - 1));
    int run = 0;
#pragma unroll
    for (int k = 1; k < 64; ++k) {
        const int x = k64[kZZ[k]];
        s = nbits_dev(x);
        if (s > 10) {
            if (!err) err = ES_AC_RANGE;
            s = 0;
        }
        if (s == 0) {
            ++run;
        } else {
            while (run > 15) {
                sink.ac(t, 0xF0, 0, 0);
                run -= 16;
            }
            sink.ac(t, run << 4 | s, s, (unsigned)(x < 0 ? x - 1 : x) & ((1u << s) - 1));
            run = 0;
        }
    }
    if (run) sink.ac(t, 0, 0, 0);
    return err;
}

__device__ __forceinline__ void report(u64* __restrict__ errkey, const Where& w, long long gb, int err) {
    if (err) atomicMin(errkey + w.n, (u64)(gb - w.base) << 3 | (u64)err);
}

// inclusive scan over the workgroup's 256 values through LDS -> this lane's exclusive prefix; *total the sum
template <typename T>
__device__ __forceinline__ T block_scan(T v, T* s, T* total) {
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int o = 1; o < JH_THREADS; o <<= 1) {
        const T x = t >= o ? s[t - o] : (T)0;
        __syncthreads();
        s[t] += x;
        __syncthreads();
    }
    const T incl = s[t];
    *total = s[JH_THREADS - 1];
    __syncthreads();
    return incl - v;
}

// ---- pass 1: lengths, or histograms ------------------------------------------------------------------------------------
struct SizeSink {
    const unsigned* __restrict__ tab;  // [4][256] code | size << 16
    unsigned bits = 0;
    __device__ __forceinline__ void dc(int t, int s, unsigned) { bits += (tab[512 * t + s] >> 16) + s; }
    __device__ __forceinline__ void ac(int t, int rs, int s, unsigned) { bits += (tab[512 * t + 256 + rs] >> 16) + s; }
};

struct HistSink {
    unsigned* lds;   // this image's [4][256] in LDS, or NULL
    unsigned* glob;  // this image's [4][256] in global memory
    __device__ __forceinline__ void add(int i) {
        if (lds) atomicAdd(lds + i, 1u);
        else atomicAdd(glob + i, 1u);
    }
    __device__ __forceinline__ void dc(int t, int s, unsigned) { add(512 * t + s); }
    __device__ __forceinline__ void ac(int t, int rs, int, unsigned) { add(512 * t + 256 + rs); }
};

template <bool HIST>
__global__ void __launch_bounds__(JH_THREADS) jh_blocks_kernel(const short* __restrict__ coef, long coef_elems, const long long* __restrict__ desc, int N,
                                                                const long long* __restrict__ blk_base, long long total, int ri,
                                                                const unsigned* __restrict__ codes, int per_image, unsigned* __restrict__ bits,
                                                                unsigned* __restrict__ sums, unsigned* __restrict__ hist, u64* __restrict__ errkey) {
    __shared__ unsigned s_mem[HIST ? JH_SLOTS * 1024 : JH_THREADS];
    __shared__ int s_first;
    const long long gb = (long long)blockIdx.x * JH_THREADS + threadIdx.x;
    Where w;
    const bool live = locate(desc, N, blk_base, total, coef_elems, ri, gb, errkey, w);
    if (HIST) {
        for (int i = threadIdx.x; i < JH_SLOTS * 1024; i += JH_THREADS) s_mem[i] = 0;
        if (threadIdx.x == 0) s_first = live ? w.n : find_image(blk_base, N, gb < total ? gb : total - 1);
        __syncthreads();
        const int first = s_first;
        if (live) {
            const int slot = w.n - first;
            HistSink sink{slot >= 0 && slot < JH_SLOTS ? s_mem + slot * 1024 : nullptr, hist + (long)w.n * 1024};
            report(errkey, w, gb, walk_block(coef, w, sink));
        }
        __syncthreads();
        for (int i = threadIdx.x; i < JH_SLOTS * 1024; i += JH_THREADS) {
            const int n = first + (i >> 10);
            if (s_mem[i] && n < N) atomicAdd(hist + (long)n * 1024 + (i & 1023), s_mem[i]);
        }
    } else {
        unsigned b = 0;
        if (live) {
            SizeSink sink{codes + (per_image ? (long)w.n * 1024 : 0)};
            report(errkey, w, gb, walk_block(coef, w, sink));
            b = sink.bits;
        }
        if (gb < total) bits[gb] = b;
        unsigned sum;
        block_scan(b, s_mem, &sum);
        if (threadIdx.x == 0) sums[blockIdx.x] = sum;
    }
}

// ---- scans -------------------------------------------------------------------------------------------------------------
// One workgroup: off[i] = sums[0] + .. + sums[i - 1] for i <= T, 2048 entries per round.  limit: only as many entries as the
// chunks of JH_CHUNK bytes that (*limit >> 3) + add bytes reach are scanned (the stuffing passes look at no others).
__global__ void __launch_bounds__(JH_THREADS) jh_scan_sums_kernel(const unsigned* __restrict__ sums, long T, u64* __restrict__ off,
                                                                   const u64* __restrict__ limit, long long add) {
    __shared__ u64 s_mem[JH_THREADS];
    if (limit) {
        const long need = (long)(((*limit >> 3) + (u64)add) / JH_CHUNK) + 1;
        T = need < T ? need : T;
    }
    u64 carry = 0;
    for (long base = 0; base < T; base += JH_THREADS * 8) {
        const long i0 = base + threadIdx.x * 8;
        unsigned v[8];
        u64 mine = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = i0 + e < T ? sums[i0 + e] : 0, mine += v[e];
        u64 total;
        u64 pre = carry + block_scan(mine, s_mem, &total);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (i0 + e < T) off[i0 + e] = pre;
            pre += v[e];
        }
        carry += total;
    }
    if (threadIdx.x == 0) off[T] = carry;
}

__global__ void __launch_bounds__(JH_THREADS) jh_scan_apply_kernel(const unsigned* __restrict__ bits, const u64* __restrict__ tile_off, long long total,
                                                                    long tiles, u64* __restrict__ P) {
    __shared__ unsigned s_mem[JH_THREADS];
    const long long gb = (long long)blockIdx.x * JH_THREADS + threadIdx.x;
    const unsigned b = gb < total ? bits[gb] : 0;
    unsigned sum;
    const unsigned pre = block_scan(b, s_mem, &sum);
    if (gb < total) P[gb] = tile_off[blockIdx.x] + pre;
    if (gb == 0) P[total] = tile_off[tiles];
}

// ---- pass 2: the unstuffed stream ----------------------------------------------------------------------------------------
__device__ __forceinline__ long long reach(const u64* __restrict__ P, long long total, long long intervals) {
    return (long long)(P[total] >> 3) + intervals;  // bytes of the unstuffed stream in use: U(one past the last interval)
}

__global__ void __launch_bounds__(JH_THREADS) jh_zero_kernel(const u64* __restrict__ P, long long total, long long intervals, uint4* __restrict__ unst,
                                                              uint4* __restrict__ marks, long cap) {
    const long long end = (reach(P, total, intervals) / JH_CHUNK + 1) * JH_CHUNK;
    const long long p = ((long long)blockIdx.x * JH_THREADS + threadIdx.x) * 16;
    if (p >= end || p + 16 > cap) return;
    unst[p >> 4] = make_uint4(0, 0, 0, 0);
    marks[p >> 4] = make_uint4(0, 0, 0, 0);
}

struct WriteSink {
    const unsigned* __restrict__ tab;
    unsigned* __restrict__ words;
    long long word, cap_words;
    u64 acc;
    int n;
    bool first;
    __device__ __forceinline__ void put(unsigned code, int size) {
        acc = acc << size | code;
        n += size;
        if (n >= 32) {
            const unsigned v = __builtin_bswap32((unsigned)(acc >> (n - 32)));
            if (word < cap_words) {
                if (first) atomicOr(words + word, v);  // may hold the end of the block before
                else words[word] = v;                  // every bit of it is this block's
            }
            first = false;
            ++word;
            n -= 32;
            acc &= (1ull << n) - 1;
        }
    }
    __device__ __forceinline__ void finish() {
        if (n && word < cap_words) atomicOr(words + word, __builtin_bswap32((unsigned)(acc << (32 - n))));
    }
    __device__ __forceinline__ void dc(int t, int s, unsigned extra) {
        const unsigned c = tab[512 * t + s];
        put(c & 0xffff, (int)(c >> 16));
        if (s) put(extra, s);
    }
    __device__ __forceinline__ void ac(int t, int rs, int s, unsigned extra) {
        const unsigned c = tab[512 * t + 256 + rs];
        put(c & 0xffff, (int)(c >> 16));
        if (s) put(extra, s);
    }
};

__global__ void __launch_bounds__(JH_THREADS) jh_write_kernel(const short* __restrict__ coef, long coef_elems, const long long* __restrict__ desc, int N,
                                                               const long long* __restrict__ blk_base, const long long* __restrict__ int_base,
                                                               long long total, int ri, const unsigned* __restrict__ codes, int per_image,
                                                               const u64* __restrict__ P, unsigned* __restrict__ unst, unsigned char* __restrict__ marks,
                                                               long cap, u64* __restrict__ errkey) {
    const long long gb = (long long)blockIdx.x * JH_THREADS + threadIdx.x;
    Where w;
    if (!locate(desc, N, blk_base, total, coef_elems, ri, gb, errkey, w)) return;
    const long long g0 = w.base + w.mcu0 * w.g.bpm;  // first block of the interval
    const long long ival = int_base[w.n] + w.k;
    const u64 p0 = P[g0];
    const long long U = (long long)(p0 >> 3) + ival;
    const u64 rel = P[gb] - p0;
    const long long bit = U * 8 + (long long)rel;
    if (gb == g0 && w.k > 0 && U < cap) marks[U] = (unsigned char)(2 + ((w.k - 1) & 7));
    WriteSink sink{codes + (per_image ? (long)w.n * 1024 : 0), unst, bit >> 5, cap >> 2, 0, (int)(bit & 31), true};
    walk_block(coef, w, sink);
    const long long mcu_end = ri > 0 && w.mcu0 + ri < w.g.mcus ? w.mcu0 + ri : w.g.mcus;
    if (w.mcu == mcu_end - 1 && w.j == w.g.bpm - 1) {  // the interval's last block: ones up to the byte, and the unused byte behind it
        const u64 len = P[gb + 1] - p0;
        const int pad = (int)((8 - (len & 7)) & 7);
        if (pad) sink.put((1u << pad) - 1, pad);
        const long long E = U + (long long)((len + 7) >> 3), next = (long long)(P[gb + 1] >> 3) + ival + 1;
        if (E < next && E < cap) marks[E] = 1;
    }
    sink.finish();
}

// ---- pass 3: stuffing ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ int byte_weight(unsigned b, unsigned m) { return m == 1 ? 0 : 1 + (b == 255) + (m >= 2 ? 2 : 0); }

// the weight of the 16 bytes at p (a multiple of 16) that lie below `end`
__device__ __forceinline__ int weight16(const uint4* __restrict__ unst, const uint4* __restrict__ marks, long long p, long long end) {
    if (p >= end) return 0;
    const uint4 d = unst[p >> 4], m = marks[p >> 4];
    const unsigned dw[4] = {d.x, d.y, d.z, d.w}, mw[4] = {m.x, m.y, m.z, m.w};
    int sum = 0;
#pragma unroll
    for (int e = 0; e < 16; ++e)
        if (p + e < end) sum += byte_weight((dw[e >> 2] >> (8 * (e & 3))) & 255, (mw[e >> 2] >> (8 * (e & 3))) & 255);
    return sum;
}

__global__ void __launch_bounds__(JH_THREADS) jh_stuff_count_kernel(const u64* __restrict__ P, long long total, long long intervals,
                                                                     const uint4* __restrict__ unst, const uint4* __restrict__ marks, long cap,
                                                                     unsigned* __restrict__ sums) {
    __shared__ unsigned s_mem[JH_THREADS];
    const long long r = reach(P, total, intervals), end = r < cap ? r : cap;
    const long long p = (long long)blockIdx.x * JH_CHUNK + threadIdx.x * 16;
    if ((long long)blockIdx.x * JH_CHUNK > end) return;  // the scan does not read this chunk's sum
    unsigned sum;
    block_scan((unsigned)weight16(unst, marks, p, end), s_mem, &sum);
    if (threadIdx.x == 0) sums[blockIdx.x] = sum;
}

__global__ void __launch_bounds__(JH_THREADS) jh_stuff_scatter_kernel(const u64* __restrict__ P, long long total, long long intervals,
                                                                       const uint4* __restrict__ unst, const uint4* __restrict__ marks, long cap,
                                                                       const u64* __restrict__ chunk_off, unsigned char* __restrict__ out, long out_bytes) {
    __shared__ unsigned s_mem[JH_THREADS];
    const long long r = reach(P, total, intervals), end = r < cap ? r : cap;
    const long long p = (long long)blockIdx.x * JH_CHUNK + threadIdx.x * 16;
    if ((long long)blockIdx.x * JH_CHUNK >= end) return;
    unsigned sum;
    const unsigned pre = block_scan((unsigned)weight16(unst, marks, p, end), s_mem, &sum);
    if (p >= end) return;
    u64 o = chunk_off[blockIdx.x] + pre;
    const uint4 d = unst[p >> 4], m = marks[p >> 4];
    const unsigned dw[4] = {d.x, d.y, d.z, d.w}, mw[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const unsigned b = (dw[e >> 2] >> (8 * (e & 3))) & 255, k = (mw[e >> 2] >> (8 * (e & 3))) & 255;
        if (p + e >= end || k == 1) continue;
        if (o + 4 > (u64)out_bytes) return;
        if (k >= 2) out[o++] = 255, out[o++] = (unsigned char)(0xD0 + k - 2);
        out[o++] = (unsigned char)b;
        if (b == 255) out[o++] = 0;
    }
}

// one wave per image n <= N: offs[n] = the weight of every byte before U(first interval of image n)
__global__ void __launch_bounds__(64) jh_offsets_kernel(const u64* __restrict__ P, const long long* __restrict__ blk_base,
                                                         const long long* __restrict__ int_base, int N, long long total, long long intervals,
                                                         const uint4* __restrict__ unst, const uint4* __restrict__ marks, long cap,
                                                         const u64* __restrict__ chunk_off, u64* __restrict__ offs) {
    const int n = blockIdx.x;
    if (n > N) return;
    const long long r = reach(P, total, intervals), end = r < cap ? r : cap;
    long long U = (long long)(P[blk_base[n]] >> 3) + int_base[n];
    U = U < end ? U : end;
    const long long c = U / JH_CHUNK;
    int sum = 0;
    for (int i = 0; i < 4; ++i) sum += weight16(unst, marks, c * JH_CHUNK + (threadIdx.x * 4 + i) * 16, U);
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o, 64);
    if (threadIdx.x == 0) offs[n] = chunk_off[c] + (u64)sum;
}

// ---- host ----------------------------------------------------------------------------------------------------------------
constexpr int SPEC = 16 + 1 + 256;  // uint16 per table: symbols per length, the number of symbols, the symbols

struct Layout {
    long tiles, chunks, cap;  // workgroups of the block passes; chunks and bytes of the unstuffed stream at its bound
    long bits, sums, tile_off, P, unst, marks, chunk_sums, chunk_off, bytes;
    long out_bytes;
};

long up16(long v) { return (v + 15) & ~15L; }

Layout layout(long total, long intervals) {
    Layout l;
    l.tiles = (total + JH_THREADS - 1) / JH_THREADS;
    l.cap = ((total * kBlockBits + 7) / 8 + intervals + JH_CHUNK) / JH_CHUNK * JH_CHUNK;
    l.chunks = l.cap / JH_CHUNK;
    long o = 0;
    l.bits = o, o = up16(o + l.tiles * JH_THREADS * 4);
    l.sums = o, o = up16(o + l.tiles * 4);
    l.tile_off = o, o = up16(o + (l.tiles + 1) * 8);
    l.P = o, o = up16(o + (total + 1) * 8);
    l.unst = o, o = up16(o + l.cap);
    l.marks = o, o = up16(o + l.cap);
    l.chunk_sums = o, o = up16(o + l.chunks * 4);
    l.chunk_off = o, o = up16(o + (l.chunks + 1) * 8);
    l.bytes = o;
    l.out_bytes = 2 * l.cap + 2 * intervals;  // every byte FF, an RSTn in front of every interval
    return l;
}

void pack_codes(const HuffSpec* specs, unsigned* codes) {
    for (int t = 0; t < 4; ++t) {
        const Codes c(specs[t].bits, specs[t].vals);
        for (int i = 0; i < 256; ++i) codes[256 * t + i] = (unsigned)c.code[i] | (unsigned)c.size[i] << 16;
    }
}

void store_specs(const HuffSpec* specs, unsigned short* out) {
    for (int t = 0; t < 4; ++t) {
        unsigned short* o = out + t * SPEC;
        for (int i = 0; i < 16; ++i) o[i] = specs[t].bits[i];
        o[16] = (unsigned short)specs[t].nvals;
        for (int i = 0; i < 256; ++i) o[17 + i] = specs[t].vals[i];
    }
}

void load_specs(const unsigned short* in, HuffSpec* specs) {
    for (int t = 0; t < 4; ++t) {
        const unsigned short* o = in + t * SPEC;
        memset(&specs[t], 0, sizeof(HuffSpec));
        for (int i = 0; i < 16; ++i) specs[t].bits[i] = (unsigned char)o[i];
        specs[t].nvals = o[16] > 256 ? 256 : o[16];
        for (int i = 0; i < 256; ++i) specs[t].vals[i] = (unsigned char)o[17 + i];
    }
}

}  // namespace

extern "C" {

// Host: what the device coder needs to know of a batch before it starts.  desc / qtabs as dbn_jpeg_encode_batch takes them.
// status[n]: 0, or the host coder's 1 (not decoded), 2 (bad descriptor), 3 (quantisation value); such an image gets no blocks.
// blk_base / int_base int64 [N + 1]: the first scan block and the first restart interval of each image over the batch.
// sizes int64 [2]: bytes of workspace and of output buffer dbn_jpeg_huff_code wants.  1: bad arguments, or a batch whose
// unstuffed stream could pass 2^60 bits (the offsets are 64-bit).
int dbn_jpeg_huff_plan(const long long* desc, const unsigned short* qtabs, int N, long coef_elems, int restart_interval, long long* blk_base,
                       long long* int_base, int* status, long long* sizes) {
    DBN_REQUIRE(desc && qtabs && blk_base && int_base && status && sizes && N > 0 && coef_elems >= 0);
    DBN_REQUIRE(restart_interval >= 0 && restart_interval <= 65535);
    long long blocks = 0, intervals = 0;
    for (int n = 0; n < N; ++n) {
        Geo g;
        int s = load_geo(desc + (long)n * JP_DESC, coef_elems, (long)N * 192, g);
        if (s == ES_OK && (g.coef & 7)) s = ES_BAD_DESC;  // the kernels load a block as 16-byte vectors
        if (s == ES_OK) s = check_qtabs(qtabs, g);
        status[n] = s;
        blk_base[n] = blocks, int_base[n] = intervals;
        if (s != ES_OK) continue;
        const long long mcus = (long long)g.mcux * g.mcuy;
        blocks += g.blocks;
        intervals += restart_interval > 0 ? (mcus + restart_interval - 1) / restart_interval : 1;
    }
    blk_base[N] = blocks, int_base[N] = intervals;
    DBN_REQUIRE(blocks < (1LL << 48));
    const Layout l = layout((long)blocks, (long)intervals);
    DBN_REQUIRE(l.tiles < (1L << 31) && l.chunks < (1L << 31));  // one workgroup each
    sizes[0] = l.bytes, sizes[1] = l.out_bytes;
    return DBN_OK;
}

// Device: per-image symbol histograms hist uint32 [N][4][256] (DC 0, AC 0, DC 1, AC 1; zeroed here) of the scan as the coder
// will walk it: DC predictors reset at every restart interval, dummy blocks counted.  errkey uint64 [N], all ones before the
// first call: (first failing scan block << 3 | status), lowered atomically.
int dbn_jpeg_huff_hist(const short* coef, long coef_elems, const long long* desc, int N, const long long* blk_base, long total_blocks,
                       int restart_interval, unsigned* hist, unsigned long long* errkey, void* stream) {
    DBN_REQUIRE(coef && desc && blk_base && hist && errkey && N > 0 && total_blocks >= 0 && restart_interval >= 0);
    DBN_REQUIRE((reinterpret_cast<size_t>(coef) & 15) == 0);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(hist, 0, (size_t)N * 4096, st) != hipSuccess) return dbn_status();
    if (total_blocks == 0) return dbn_status();
    const unsigned grid = (unsigned)((total_blocks + JH_THREADS - 1) / JH_THREADS);
    hipLaunchKernelGGL(jh_blocks_kernel<true>, dim3(grid), dim3(JH_THREADS), 0, st, coef, coef_elems, desc, N, blk_base, (long long)total_blocks,
                       restart_interval, (const unsigned*)nullptr, 0, (unsigned*)nullptr, (unsigned*)nullptr, hist, errkey);
    return dbn_status();
}

// Host: Annex K as specs uint16 [4][273] (symbols per length [16], symbol count, symbols [256]) and codes uint32 [4][256]
// (code | length << 16, 0 for a symbol without one), the forms dbn_jpeg_huff_headers and dbn_jpeg_huff_code take.
int dbn_jpeg_huff_annex_k(unsigned short* specs, unsigned* codes) {
    DBN_REQUIRE(specs && codes);
    store_specs(annex_k(), specs);
    pack_codes(annex_k(), codes);
    return DBN_OK;
}

// Host: each image's own tables from its histograms (dbn_jpeg_optimal_table's rule), on min(N, 16, threads) threads: specs
// uint16 [N][4][273], codes uint32 [N][4][256].  A grey image's tables 2 and 3 repeat 0 and 1.  Images whose status is not 0
// are left alone; status[n] becomes 7 where the builder gives up.
int dbn_jpeg_huff_tables(const unsigned* hist, const long long* desc, int N, int* status, unsigned short* specs, unsigned* codes, int threads) {
    DBN_REQUIRE(hist && desc && status && specs && codes && N > 0);
    on_threads(N, threads, [&](int n) {
        if (status[n] != ES_OK) return;
        HuffSpec own[4];
        const int nt = desc[(long)n * JP_DESC + D_NC] == 3 ? 4 : 2;
        for (int t = 0; t < nt; ++t) {
            long long freq[256];
            for (int i = 0; i < 256; ++i) freq[i] = hist[(long)n * 1024 + 256 * t + i];
            if (optimal_table(freq, own[t]) != ES_OK) {
                status[n] = ES_CODE_LENGTH;
                return;
            }
        }
        if (nt == 2) own[2] = own[0], own[3] = own[1];
        store_specs(own, specs + (long)n * 4 * SPEC);
        pack_codes(own, codes + (long)n * 1024);
    });
    return DBN_OK;
}

// Device: codes every image with status 0 of the plan.  codes uint32 [N or 1][4][256] on the device (per_image: one set per
// image); ws / out: buffers of the sizes dbn_jpeg_huff_plan gave, 16-byte aligned; res uint64 [2 N + 1] on the device: the
// error keys [N] (all ones before the first call, see dbn_jpeg_huff_hist), then offs [N + 1]: image n's entropy-coded segment
// is out[offs[n] .. offs[n + 1]).  Nine launches on `stream`, no synchronisation.
int dbn_jpeg_huff_code(const short* coef, long coef_elems, const long long* desc, int N, const long long* blk_base, const long long* int_base,
                       long total_blocks, long total_intervals, int restart_interval, const unsigned* codes, int per_image, void* ws, long ws_bytes,
                       unsigned char* out, long out_bytes, unsigned long long* res, void* stream) {
    DBN_REQUIRE(coef && desc && blk_base && int_base && codes && ws && out && res && N > 0 && total_blocks > 0 && total_intervals > 0);
    DBN_REQUIRE(restart_interval >= 0 && restart_interval <= 65535);
    DBN_REQUIRE((reinterpret_cast<size_t>(coef) & 15) == 0 && (reinterpret_cast<size_t>(ws) & 15) == 0);
    const Layout l = layout(total_blocks, total_intervals);
    DBN_REQUIRE(ws_bytes >= l.bytes && out_bytes >= l.out_bytes);
    char* w = (char*)ws;
    unsigned *bits = (unsigned*)(w + l.bits), *sums = (unsigned*)(w + l.sums), *chunk_sums = (unsigned*)(w + l.chunk_sums);
    u64 *tile_off = (u64*)(w + l.tile_off), *P = (u64*)(w + l.P), *chunk_off = (u64*)(w + l.chunk_off);
    uint4 *unst = (uint4*)(w + l.unst), *marks = (uint4*)(w + l.marks);
    u64 *errkey = res, *offs = res + N;
    hipStream_t st = (hipStream_t)stream;
    const long long total = total_blocks, ivs = total_intervals;
    const dim3 T(JH_THREADS);
    hipLaunchKernelGGL(jh_blocks_kernel<false>, dim3((unsigned)l.tiles), T, 0, st, coef, coef_elems, desc, N, blk_base, total, restart_interval, codes,
                       per_image, bits, sums, (unsigned*)nullptr, errkey);
    hipLaunchKernelGGL(jh_scan_sums_kernel, dim3(1), T, 0, st, (const unsigned*)sums, l.tiles, tile_off, (const u64*)nullptr, 0LL);
    hipLaunchKernelGGL(jh_scan_apply_kernel, dim3((unsigned)l.tiles), T, 0, st, (const unsigned*)bits, (const u64*)tile_off, total, l.tiles, P);
    hipLaunchKernelGGL(jh_zero_kernel, dim3((unsigned)(l.cap / 16 / JH_THREADS)), T, 0, st, (const u64*)P, total, ivs, unst, marks, l.cap);
    hipLaunchKernelGGL(jh_write_kernel, dim3((unsigned)l.tiles), T, 0, st, coef, coef_elems, desc, N, blk_base, int_base, total, restart_interval, codes,
                       per_image, (const u64*)P, (unsigned*)unst, (unsigned char*)marks, l.cap, errkey);
    hipLaunchKernelGGL(jh_stuff_count_kernel, dim3((unsigned)l.chunks), T, 0, st, (const u64*)P, total, ivs, (const uint4*)unst, (const uint4*)marks,
                       l.cap, chunk_sums);
    hipLaunchKernelGGL(jh_scan_sums_kernel, dim3(1), T, 0, st, (const unsigned*)chunk_sums, l.chunks, chunk_off, (const u64*)(P + total), ivs);
    hipLaunchKernelGGL(jh_stuff_scatter_kernel, dim3((unsigned)l.chunks), T, 0, st, (const u64*)P, total, ivs, (const uint4*)unst, (const uint4*)marks,
                       l.cap, (const u64*)chunk_off, out, out_bytes);
    hipLaunchKernelGGL(jh_offsets_kernel, dim3((unsigned)(N + 1)), dim3(64), 0, st, (const u64*)P, blk_base, int_base, N, total, ivs,
                       (const uint4*)unst, (const uint4*)marks, l.cap, (const u64*)chunk_off, offs);
    return dbn_status();
}

// Host: SOI .. SOS of every image with status 0 into out[n * 704 ..], its length into lens[n] (0 otherwise).  specs uint16
// [N or 1][4][273] (per_image: one set per image): the tables of the DHT segments.
int dbn_jpeg_huff_headers(const long long* desc, const unsigned short* qtabs, int N, int restart_interval, const unsigned short* specs, int per_image,
                          const int* status, unsigned char* out, long long* lens) {
    DBN_REQUIRE(desc && qtabs && specs && status && out && lens && N > 0 && restart_interval >= 0 && restart_interval <= 65535);
    HuffSpec shared[4];
    if (!per_image) load_specs(specs, shared);
    for (int n = 0; n < N; ++n) {
        lens[n] = 0;
        Geo g;
        if (status[n] != ES_OK || load_geo(desc + (long)n * JP_DESC, 0x7fffffffffffffffL, (long)N * 192, g) != ES_OK) continue;
        HuffSpec own[4];
        if (per_image) load_specs(specs + (long)n * 4 * SPEC, own);
        const long len = write_header(qtabs, g, restart_interval, per_image ? own : shared, out + (long)n * kHeaderBytes, kHeaderBytes);
        lens[n] = len < 0 ? 0 : len;
    }
    return DBN_OK;
}

}  // extern "C"
