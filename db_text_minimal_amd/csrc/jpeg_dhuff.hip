// Huffman decoding of JPEG scans on the device: the entropy stage of the decode (jpeg.hip) without the coefficients crossing
// PCIe.  Input is the batch's compressed bytes and the host plan of dbn_jpeg_stream_plan (headers, Huffman table specs and the
// scans cut at their markers; the host reads no bit of the entropy data); output is the coefficient layout dbn_jpeg_pixels
// reads.  The scheme is parallel decoding by subsequences with the decoder state propagated to a fixed point
// (Weissenberger and Schmidt, "Massively parallel Huffman decoding on GPUs", ICPP 2018, and their JPEG decoder, 2021):
//
// A restart interval (segment) is cut into subsequences of DH_S = 1024 bits of the stuffed stream, one lane each.  The state of
// the decoder between two symbols is (bit position, block within the MCU, zigzag index).  F_i takes a state in front of
// subsequence i to the first symbol boundary at or behind the subsequence's end.  The first subsequence of a segment
// starts in the known state, every other one from a guess (a block starts at its first bit); out[i] = F_i(out[i - 1]) is
// then iterated until nothing changes.  After k rounds the first k states of a segment are exact whatever the data; that
// Huffman codes resynchronise only makes the fixed point arrive early.
//   dh_prop_kernel    one launch = one round across workgroups, and inside the workgroup rounds until its 256 states stand
//                     (bounded by 256).  Launch r reads the states of launch r - 1 and writes its own (two buffers): no
//                     workgroup waits for another.  It records per image whether a state changed; an image whose last
//                     launch changed nothing is at the fixed point.
//   dh_count_kernel   blocks each subsequence completes, from its exact entry state
//   dh_scan_kernel    one workgroup: exclusive scan of the counts -> the first scan-order block of each subsequence
//   dh_write_kernel   decodes once more and stores the non-zero coefficients at their natural index into the (zeroed)
//                     buffer, DC values as differences; checks what the host decoder checks and lowers the image's key
//   dh_dc_kernel      per image and component: segmented prefix sum of the DC differences over scan order within each
//                     restart interval, with the host's int16 wrap
// FF00 stuffing is skipped inline: a position never rests on a stuffed 00, the reader steps over it when it leaves the FF.
// Decoding from a wrong state writes nothing and cannot fail: a code in no table is one bit that changes nothing, a run past
// 63 ends the block; a symbol that would end behind the segment is not taken.  Every loop is bounded by the bits of a
// subsequence.  An image is given to the host decoder (by the caller) when its key was lowered or its last launch still
// changed a state: the device never decides a status.  Every read is checked against the segment's end and the blob, every
// write against the image's slice; table entries that disagree with the plan are not followed (the image is flagged).
// The descriptor, its checked geometry (read_scan, block_at), the zigzag order and the canonical code ranges are jpeg_common.h's.
#include "common.h"
#include "jpeg_common.h"
#include "jpeg_dhuff.h"

using namespace dbn_dhuff;
using namespace dbn_jpeg;

namespace {

typedef unsigned long long u64;
// why an image was flagged (the low bits of its key; the host decoder gives the status that is reported)
enum { DE_PLAN = 1, DE_CODE, DE_RUN, DE_BITS, DE_MCUS };
#define DH_TRY(x)                                         \
    do {                                                  \
        const hipError_t e_ = (x);                        \
        if (e_ != hipSuccess) return 1000 + (int)e_;      \
    } while (0)
constexpr int DH_CAP = DH_S + 64;  // symbols one F_i may take: each is at least one bit

// the host reader's lookup (jpeg.hip Huff): 9-bit prefix table, min / max code per longer length
struct Tab {
    unsigned short fast[512];
    int mincode[17], maxcode[17], first[17];
    int nvals;
    unsigned char vals[256];
};

// the decoder's own conditions on a descriptor: a block is loaded as 16-byte vectors, the restart interval is one a DRI holds
__device__ __forceinline__ bool load_desc(const long long* __restrict__ d, long coef_elems, Scan& g) {
    return read_scan(d, coef_elems, g) && (g.coef & 7) == 0 && d[D_RI] >= 0 && d[D_RI] <= 65535;
}

// ---- the image of a workgroup: its plan rows checked, its tables in LDS -------------------------------------------------------
struct Batch {
    const unsigned char* __restrict__ blob;
    long blob_len;
    const long long* __restrict__ desc;
    const unsigned char* __restrict__ hspec;
    const long long* __restrict__ info;
    const long long* __restrict__ seg;
    const long long* __restrict__ sub_base;
    const int* __restrict__ wgtab;
    int N;
    long nseg, nsub;
    long coef_elems;
    u64* __restrict__ res;  // [N] keys, then per launch [N] "a state changed"
};

struct Image {
    Scan g;
    int n, cnt;
    long g0;  // first subsequence of the workgroup
    long long begin, end, seg0, nseg, sub0, nsub;
};

__device__ __forceinline__ void flag(const Batch& B, int n, long sub, int why) { atomicMin(B.res + n, (u64)sub << 4 | (u64)why); }

// false: the workgroup has nothing to do (and the image is flagged if its rows disagree with one another)
__device__ bool load_image(const Batch& B, Image& I) {
    const int* w = B.wgtab + 4 * (long)blockIdx.x;
    I.n = w[0], I.g0 = w[1], I.cnt = w[2];
    if (I.n < 0 || I.n >= B.N) return false;
    const long long* in = B.info + (long)I.n * DH_INFO;
    I.begin = in[DI_BEGIN], I.end = in[DI_END], I.seg0 = in[DI_SEG0], I.nseg = in[DI_NSEG], I.sub0 = in[DI_SUB0], I.nsub = in[DI_NSUB];
    bool ok = in[DI_HOST] == 0 && I.begin >= 0 && I.begin <= I.end && I.end <= B.blob_len && I.seg0 >= 0 && I.nseg >= 1 &&
              I.seg0 + I.nseg <= B.nseg && I.sub0 >= 0 && I.nsub >= 1 && I.sub0 + I.nsub <= B.nsub && I.cnt >= 1 && I.cnt <= DH_THREADS &&
              I.g0 >= I.sub0 && I.g0 + I.cnt <= I.sub0 + I.nsub && B.sub_base[I.seg0] == I.sub0 && B.sub_base[I.seg0 + I.nseg] == I.sub0 + I.nsub;
    ok = ok && load_desc(B.desc + (long)I.n * JP_DESC, B.coef_elems, I.g);
    if (!ok && threadIdx.x == 0) flag(B, I.n, 0, DE_PLAN);
    return ok;
}

// the image's tables, one pair per component, from their specs; false (for every lane) when a spec is not a prefix code
__device__ bool build_tables(const Batch& B, const Image& I, Tab* tabs, int* s_bad) {
    const int t = threadIdx.x, nt = 2 * I.g.nc;
    const long long sel = B.info[(long)I.n * DH_INFO + DI_SEL];
    const unsigned char* spec = B.hspec + (long)I.n * 8 * DH_SPEC;
    if (t == 0) *s_bad = 0;
    __syncthreads();
    for (int q = 0; q < nt; ++q) {
        const int id = (int)(sel >> (8 * (q >> 1) + 4 * (q & 1))) & 15;
        const unsigned char* s = spec + ((q & 1) * 4 + (id & 3)) * DH_SPEC;
        Tab& T = tabs[q];
        for (int i = t; i < 512; i += DH_THREADS) T.fast[i] = 0;
        T.vals[t] = s[17 + t];
        if (t == 0) {
            const bool prefix = code_ranges(s + 1, T.mincode, T.maxcode, T.first, &T.nvals);
            if (id > 3 || s[0] != 1 || !prefix || T.nvals > 256) *s_bad = 1;
        }
    }
    __syncthreads();
    if (*s_bad) {
        if (t == 0) flag(B, I.n, 0, DE_PLAN);
        return false;
    }
    for (int q = 0; q < nt; ++q) {
        Tab& T = tabs[q];
        for (int i = t; i < T.nvals; i += DH_THREADS) {
            int l = 1;
            while (l < 16 && !(T.maxcode[l] >= 0 && i < T.first[l] + T.maxcode[l] - T.mincode[l] + 1)) ++l;
            if (l > 9) continue;
            const int base = (T.mincode[l] + i - T.first[l]) << (9 - l);
            for (int j = 0; j < (1 << (9 - l)); ++j)
                if (base + j < 512) T.fast[base + j] = (unsigned short)(l << 8 | T.vals[i]);
        }
    }
    __syncthreads();
    return true;
}

// ---- a subsequence ---------------------------------------------------------------------------------------------------------
struct Sub {
    long long first, end;  // the segment's bytes in the blob
    long long mcu0, want;  // its first MCU; the blocks it holds
    long sfirst;           // its first subsequence
    unsigned bits;         // its length in bits
    int i, ns;             // this subsequence's number in it, and how many it has
};

__device__ bool load_sub(const Batch& B, const Image& I, long gs, Sub& S) {
    long lo = I.seg0, hi = I.seg0 + I.nseg;  // sub_base[lo] <= gs < sub_base[hi]
    while (hi - lo > 1) {
        const long mid = (lo + hi) >> 1;
        if (B.sub_base[mid] <= gs) lo = mid;
        else hi = mid;
    }
    const long long* r = B.seg + lo * DH_SEG;
    S.first = r[SG_FIRST], S.end = r[SG_END], S.mcu0 = r[SG_MCU0];
    const long long mcus = r[SG_MCUS];
    S.sfirst = B.sub_base[lo];
    const long long len = S.end - S.first, nb = len * 8;
    const long long ns = nb ? (nb + DH_S - 1) / DH_S : 1;
    if (r[SG_IMAGE] != I.n || S.first < I.begin || len < 0 || S.end > I.end || nb > 0xFFFFFFF0LL || S.mcu0 < 0 || mcus < 1 ||
        S.mcu0 + mcus > I.g.mcus || B.sub_base[lo + 1] - S.sfirst != ns || gs < S.sfirst || gs - S.sfirst >= ns)
        return false;
    S.bits = (unsigned)nb, S.want = mcus * I.g.bpm, S.i = (int)(gs - S.sfirst), S.ns = (int)ns;
    return true;
}

// a state: bit position in the segment (of the stuffed stream; never on a stuffed 00) | block in the MCU << 32 | zigzag index << 40
__device__ __forceinline__ u64 pack(unsigned pos, int j, int k) { return (u64)pos | (u64)j << 32 | (u64)k << 40; }

__device__ __forceinline__ u64 guess(const Batch& B, const Sub& S) {
    const long long b = S.first + (long long)S.i * (DH_S / 8);
    unsigned pos = (unsigned)S.i * DH_S;
    if (S.i > 0 && b < S.end && B.blob[b] == 0 && B.blob[b - 1] == 0xFF) pos += 8;
    return pack(pos, 0, 0);
}

struct NoSink {
    __device__ __forceinline__ void put(int, int, int) {}
};

// F_i and everything that walks like it: from state `st` to the first symbol boundary at or behind the subsequence's end
// (or the segment's), at most DH_CAP symbols; `stop` > 0: not beyond that many completed blocks.  sink.put(blocks completed
// so far, zigzag index, value) for every coefficient taken.  -> the state; blocks: completed; err: DE_CODE / DE_RUN met (first);
// over: a symbol would have ended behind the segment.
template <typename Sink>
__device__ u64 walk(const unsigned char* __restrict__ blob, const Sub& S, const Tab* __restrict__ tabs, const Scan& g, u64 st, long long stop,
                    Sink& sink, int& blocks, int& err, bool& over) {
    long long pos = (unsigned)st;
    int j = (int)(st >> 32) & 255, k = (int)(st >> 40) & 255;
    const long long E = min((long long)(S.i + 1) * DH_S, (long long)S.bits);
    blocks = 0, err = 0, over = false;
    if (j >= g.bpm || k > 63) return st;  // never a state of this image
    for (int it = 0; it < DH_CAP && pos < E; ++it) {
        if (stop > 0 && blocks >= stop) break;
        // 32 bits from pos: five data bytes, each FF's 00 stepped over; nx[i] the byte behind the first i + 1
        const long long b = S.first + (pos >> 3);
        const int bit = (int)(pos & 7);
        long long idx = b, nx[5];
        u64 acc = 0;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const unsigned v = idx < S.end ? blob[idx] : 0u;
            acc = acc << 8 | v;
            idx += (v == 0xFF && idx + 1 < S.end && blob[idx + 1] == 0) ? 2 : 1;
            nx[i] = idx;
        }
        const unsigned w = (unsigned)(acc >> (8 - bit));
        const int c = j < g.nl ? 0 : j - g.nl + 1;
        const Tab& T = tabs[2 * c + (k ? 1 : 0)];
        int len = 0, sym = -1;
        const unsigned f = T.fast[w >> 23];
        if (f) {
            len = f >> 8, sym = f & 255;
        } else {
            for (int l = 10; l <= 16; ++l) {
                const int code = (int)(w >> (32 - l));
                if (T.maxcode[l] >= 0 && code >= T.mincode[l] && code <= T.maxcode[l]) {
                    const int i = T.first[l] + code - T.mincode[l];
                    if (i < T.nvals && i < 256) len = l, sym = T.vals[i];
                    break;
                }
            }
        }
        int total = 1, nk = k, zz = -1, val = 0, e = 0;
        bool done = false;
        if (sym < 0) {
            e = DE_CODE;  // one bit, nothing else
        } else {
            const int s = sym & 15, r = sym >> 4;
            const int v = s ? (int)((w << len) >> (32 - s)) : 0;
            const int x = s && v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
            if (k == 0) {
                if (sym > 11) e = DE_CODE;
                total = len + s, zz = 0, val = x, nk = 1;
            } else if (s == 0) {
                total = len;
                if (r != 15) {
                    done = true;
                } else {
                    nk = k + 16;
                    if (nk > 64) e = DE_RUN;
                    done = nk >= 64;
                }
            } else {
                total = len + s;
                if (k + r > 63) {
                    e = DE_RUN, done = true;
                } else {
                    zz = k + r, val = x, nk = zz + 1, done = nk == 64;
                }
            }
        }
        const int adv = (bit + total) >> 3;
        const long long npos = ((adv ? nx[adv - 1] : b) - S.first) * 8 + ((bit + total) & 7);
        if (npos > (long long)S.bits) {
            over = true;
            break;
        }
        if (e && !err) err = e;
        if (zz >= 0) sink.put(blocks, zz, val);
        pos = npos;
        if (done) {
            k = 0, j = j + 1 == g.bpm ? 0 : j + 1, ++blocks;
        } else {
            k = nk;
        }
    }
    return pack((unsigned)pos, j, k);
}

constexpr u64 KNOWN = 0;  // position 0, block 0, DC next

// ---- propagation -------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DH_THREADS) dh_prop_kernel(Batch B, int launch, const u64* __restrict__ prev, u64* __restrict__ cur) {
    __shared__ Tab s_tab[6];
    __shared__ u64 s_out[DH_THREADS];
    __shared__ int s_bad;
    Image I;
    if (!load_image(B, I)) return;
    if (!build_tables(B, I, s_tab, &s_bad)) return;
    const int t = threadIdx.x;
    const long gs = I.g0 + t;
    Sub S;
    const bool live = t < I.cnt && load_sub(B, I, gs, S);
    if (t < I.cnt && !live) flag(B, I.n, gs, DE_PLAN);
    const bool head = live && S.i == 0;
    NoSink sink;
    int blocks, err;
    bool over;
    u64 in = KNOWN, out = 0;
    if (live) {
        if (!head) in = launch == 0 ? guess(B, S) : prev[gs - 1];
        out = walk(B.blob, S, s_tab, I.g, in, 0, sink, blocks, err, over);
    }
    s_out[t] = out;
    for (int it = 0; it <= I.cnt; ++it) {
        __syncthreads();
        const u64 nin = t > 0 ? s_out[t - 1] : in;
        const bool ch = live && !head && t > 0 && nin != in;
        if (!__syncthreads_or(ch)) break;
        if (ch) {
            in = nin;
            s_out[t] = walk(B.blob, S, s_tab, I.g, in, 0, sink, blocks, err, over);
        }
    }
    if (!live) return;
    out = s_out[t];
    cur[gs] = out;
    const bool changed = launch == 0 ? (t == 0 && !head) : out != prev[gs];
    if (changed) atomicOr(B.res + (long)B.N * (1 + launch) + I.n, (u64)1);
}

// ---- counting ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DH_THREADS) dh_count_kernel(Batch B, const u64* __restrict__ state, unsigned* __restrict__ count) {
    __shared__ Tab s_tab[6];
    __shared__ int s_bad;
    Image I;
    if (!load_image(B, I)) return;
    if (!build_tables(B, I, s_tab, &s_bad)) return;
    const long gs = I.g0 + threadIdx.x;
    Sub S;
    if (threadIdx.x >= I.cnt || !load_sub(B, I, gs, S)) return;
    NoSink sink;
    int blocks, err;
    bool over;
    walk(B.blob, S, s_tab, I.g, S.i == 0 ? KNOWN : state[gs - 1], 0, sink, blocks, err, over);
    count[gs] = (unsigned)blocks;
}

// one workgroup: scan[i] = count[0] + ... + count[i - 1], i = 0 .. n
constexpr int SC_THREADS = 1024;
__global__ void __launch_bounds__(SC_THREADS) dh_scan_kernel(const unsigned* __restrict__ count, unsigned* __restrict__ scan, long n) {
    __shared__ unsigned s[SC_THREADS];
    const int t = threadIdx.x;
    unsigned carry = 0;
    for (long c0 = 0; c0 < n; c0 += SC_THREADS) {
        const unsigned v = c0 + t < n ? count[c0 + t] : 0u;
        s[t] = v;
        __syncthreads();
        for (int o = 1; o < SC_THREADS; o <<= 1) {
            const unsigned x = t >= o ? s[t - o] : 0u;
            __syncthreads();
            s[t] += x;
            __syncthreads();
        }
        if (c0 + t < n) scan[c0 + t] = carry + s[t] - v;
        carry += s[SC_THREADS - 1];
        __syncthreads();
    }
    if (t == 0) scan[n] = carry;
}

// ---- writing -----------------------------------------------------------------------------------------------------------------
struct CoefSink {
    short* __restrict__ coef;
    const Scan& g;
    long long mcu0, base, want;
    long long at = -1, at_blk = -1;
    __device__ __forceinline__ void put(int blocks, int zz, int val) {
        const long long blk = base + blocks;
        if (blk >= want) return;
        if (blk != at_blk) {
            at_blk = blk;
            const long long mcu = mcu0 + blk / g.bpm;
            at = mcu < g.mcus ? block_at(g, mcu, (int)(blk % g.bpm)) : -1;
        }
        if (at >= g.coef && at + 64 <= g.coef + g.blocks * 64 && val != 0) coef[at + kZZ[zz & 63]] = (short)val;
    }
};

__global__ void __launch_bounds__(DH_THREADS) dh_write_kernel(Batch B, const u64* __restrict__ state, const unsigned* __restrict__ scan,
                                                               short* __restrict__ coef) {
    __shared__ Tab s_tab[6];
    __shared__ int s_bad;
    Image I;
    if (!load_image(B, I)) return;
    if (!build_tables(B, I, s_tab, &s_bad)) return;
    const long gs = I.g0 + threadIdx.x;
    Sub S;
    if (threadIdx.x >= I.cnt || !load_sub(B, I, gs, S)) return;
    const long long base = (long long)(scan[gs] - scan[S.sfirst]);
    if (base >= S.want) return;  // behind the segment's last block: the lane that completed it has checked the rest
    CoefSink sink{coef, I.g, S.mcu0, base, S.want};
    int blocks, err;
    bool over;
    const u64 out = walk(B.blob, S, s_tab, I.g, S.i == 0 ? KNOWN : state[gs - 1], S.want - base, sink, blocks, err, over);
    if (err) flag(B, I.n, gs, err);
    if (base + blocks >= S.want) {
        // what is left in front of the marker must be less than a byte of data: the rest of the byte the position is in
        // (and that byte's stuffed 00)
        const long long pos = (unsigned)out, b = S.first + (pos >> 3);
        long long nb = b;
        if (pos & 7) nb = b + ((b < S.end && B.blob[b] == 0xFF && b + 1 < S.end && B.blob[b + 1] == 0) ? 2 : 1);
        if (nb < S.end) flag(B, I.n, gs, DE_MCUS);
    } else if (over) {
        flag(B, I.n, gs, DE_BITS);
    } else if (S.i == S.ns - 1) {
        flag(B, I.n, gs, DE_MCUS);  // the segment ends with blocks missing
    }
}

// ---- DC differences -> values --------------------------------------------------------------------------------------------------
// workgroup (image, component): the component's blocks in scan order, 256 at a time, a restart interval's first block of
// the component starting the sum again
__global__ void __launch_bounds__(DH_THREADS) dh_dc_kernel(Batch B, short* __restrict__ coef) {
    __shared__ int s_v[DH_THREADS], s_f[DH_THREADS];
    const int n = blockIdx.x / 3, c = blockIdx.x % 3, t = threadIdx.x;
    if (n >= B.N || B.info[(long)n * DH_INFO + DI_HOST] != 0 || B.info[(long)n * DH_INFO + DI_NSUB] < 1) return;
    Scan g;
    if (!load_desc(B.desc + (long)n * JP_DESC, B.coef_elems, g) || c >= g.nc) return;
    const int ri = (int)B.desc[(long)n * JP_DESC + D_RI];
    const int bc = c == 0 ? g.nl : 1;
    const long long total = g.mcus * bc;
    int carry = 0;
    for (long long q0 = 0; q0 < total; q0 += DH_THREADS) {
        const long long q = q0 + t;
        long long at = -1;
        int v = 0, f = 0;
        if (q < total) {
            const long long mcu = q / bc;
            const int jj = (int)(q - mcu * bc);
            at = block_at(g, mcu, c == 0 ? jj : g.nl + c - 1);
            v = coef[at];
            f = jj == 0 && (ri ? mcu % ri == 0 : mcu == 0);
        }
        s_v[t] = v, s_f[t] = f;
        __syncthreads();
        for (int o = 1; o < DH_THREADS; o <<= 1) {
            const int xv = t >= o ? s_v[t - o] : 0, xf = t >= o ? s_f[t - o] : 0;
            __syncthreads();
            if (!s_f[t]) s_v[t] += xv, s_f[t] = xf;
            __syncthreads();
        }
        const int sum = s_v[t] + (s_f[t] ? 0 : carry);
        if (at >= 0) coef[at] = (short)sum;
        __syncthreads();
        if (t == DH_THREADS - 1) s_v[0] = sum;
        __syncthreads();
        carry = (short)s_v[0];
        __syncthreads();
    }
}

}  // namespace

extern "C" {

// bytes of workspace for nsub subsequences: two state buffers (8 bytes each), block counts and their scan (4 bytes each)
long dbn_jpeg_dhuff_ws_bytes(long nsub) { return nsub < 0 ? -1 : 16 * nsub + 4 * nsub + 4 * (nsub + 1) + 4; }

// Everything in device memory; the plan arrays as dbn_jpeg_stream_plan wrote them (desc with the status in field 22).  rounds:
// propagation launches after the first, 0 .. 64.  coef: coef_elems int16, zeroed here, then every image's slice written.
// res: uint64 [N * (rounds + 2)], set here: res[n] stays all ones unless image n was flagged; res[N * (1 + r) + n] != 0 when
// launch r changed a state of image n (the image is decoded when res[n] is all ones and res[N * (1 + rounds) + n] == 0).
int dbn_jpeg_dhuff(const unsigned char* blob, long blob_len, const long long* desc, const unsigned char* hspec, const long long* info,
                   const long long* seg, const long long* sub_base, const int* wgtab, int N, long nseg, long nsub, int nwg, int rounds, short* coef,
                   long coef_elems, void* ws, long ws_bytes, unsigned long long* res, void* stream) {
    DBN_REQUIRE(blob && desc && hspec && info && seg && sub_base && wgtab && res && N > 0 && blob_len > 0 && nseg >= 0 && nsub >= 0 && nwg >= 0);
    DBN_REQUIRE(rounds >= 0 && rounds <= DH_MAX_ROUNDS && coef_elems >= 0 && (coef || coef_elems == 0) && nsub < 0x7FFFFF00L);
    DBN_REQUIRE((ws || nsub == 0) && ws_bytes >= dbn_jpeg_dhuff_ws_bytes(nsub) && (reinterpret_cast<size_t>(ws) & 7) == 0);
    hipStream_t st = (hipStream_t)stream;
    DH_TRY(hipMemsetAsync(res, 0xFF, sizeof(u64) * N, st));
    DH_TRY(hipMemsetAsync(res + N, 0, sizeof(u64) * N * (rounds + 1), st));
    if (coef_elems) DH_TRY(hipMemsetAsync(coef, 0, sizeof(short) * coef_elems, st));
    if (nwg == 0 || nsub == 0 || coef_elems == 0) return dbn_status();
    u64* state[2] = {static_cast<u64*>(ws), static_cast<u64*>(ws) + nsub};
    unsigned* count = reinterpret_cast<unsigned*>(state[1] + nsub);
    unsigned* scan = count + nsub;
    DH_TRY(hipMemsetAsync(count, 0, sizeof(unsigned) * nsub, st));
    const Batch B{blob, blob_len, desc, hspec, info, seg, sub_base, wgtab, N, nseg, nsub, coef_elems, res};
    for (int r = 0; r <= rounds; ++r)
        hipLaunchKernelGGL(dh_prop_kernel, dim3((unsigned)nwg), dim3(DH_THREADS), 0, st, B, r, state[(r + 1) & 1], state[r & 1]);
    const u64* fin = state[rounds & 1];
    hipLaunchKernelGGL(dh_count_kernel, dim3((unsigned)nwg), dim3(DH_THREADS), 0, st, B, fin, count);
    hipLaunchKernelGGL(dh_scan_kernel, dim3(1), dim3(SC_THREADS), 0, st, count, scan, nsub);
    hipLaunchKernelGGL(dh_write_kernel, dim3((unsigned)nwg), dim3(DH_THREADS), 0, st, B, fin, scan, coef);
    hipLaunchKernelGGL(dh_dc_kernel, dim3((unsigned)N * 3), dim3(DH_THREADS), 0, st, B, coef);
    return dbn_status();
}

}  // extern "C"
