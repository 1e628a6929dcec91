// Baseline JPEG encode behind the device pipeline, in the place of the reference's imageio / Pillow writes (utils.py:225,272,280,
// data_loaders.py:388, test_ocr.py:176,210, ts_request.py:38-39): csrc/jpeg.hip turned round.  The dense integer work runs on
// the device, the serial, bit-granular Huffman stage on the host; the coefficient layout of dbn_jpeg_entropy_batch is the
// hand-over in both directions.
//   device  dbn_jpeg_forward         two kernels on one stream: jpeg_planes_kernel (RGB -> YCbCr, edge replication, chroma
//                                    downsampling -> uint8 sample planes in a workspace) and jpeg_fdct_kernel (libjpeg's
//                                    slow-integer 8 x 8 forward DCT on samples - 128, quantisation, the dummy blocks of the
//                                    MCU-padded grid -> int16 coefficients, 64 per block in NATURAL order).  Mixed sizes and
//                                    samplings run in one call: each workgroup looks its work up in a host-built table.
//   host    dbn_jpeg_encode_bound    bytes a batch's streams can need at most (per image and in total)
//           dbn_jpeg_optimal_table   libjpeg's optimised Huffman table for 256 symbol counts
//           dbn_jpeg_encode_batch    (_opt: with each image's own optimised tables) Huffman-codes N images (Annex K tables) on up to min(N, 16, threads) threads, each
//                                    into its own slot of one output buffer: SOI, JFIF APP0, DQT, SOF0, DHT, DRI, SOS, one
//                                    interleaved scan, EOI.  Coefficients are taken as given, dummy blocks included, so
//                                    decoding a stream and encoding the result reproduces its scan bytes.
// The arithmetic is libjpeg's, in int32: jccolor.c's 16-bit fixed-point colour conversion, jcsample.c's h2v1 / h2v2
// downsampling without smoothing (alternating bias), jfdctint.c jpeg_fdct_islow (CONST_BITS 13 / PASS1_BITS 2), jcdctmgr.c's
// rounding division by 8 q, and jccoefct.c's dummy blocks (zero AC, the DC of the previous block in MCU order).  Edges:
// the last column is replicated at full resolution; the last row at full resolution only up to a multiple of the vertical
// sampling factor, then the last DOWNSAMPLED row down to the block grid (what libjpeg's row-group buffering does).
// The descriptor, its checked geometry (read_scan), the zigzag order and the thread pool are jpeg_common.h's.
#include <string.h>

#include "common.h"
#include "jpeg_enc.h"

using namespace dbn_jpeg;

namespace {

// ---- device -------------------------------------------------------------------------------------------------------------
struct Enc {
    long long coef, in, qt;
    int W, H, nc, hs, vs, mcux, mcuy;
    int bw[3], bh[3];  // the MCU-padded grid
    int rw[3], rh[3];  // the component's own block columns / rows
    long long comp_off[3];
};

// A descriptor is used only if everything it makes a kernel touch lies inside the buffers: the pixels [in, in + H * W * nc)
// inside in_bytes, the coefficient / plane range inside coef_elems, the tables inside qt_elems, and the grids exactly the
// ones the size and the sampling give (read_scan).
__device__ __forceinline__ bool load_enc(const long long* __restrict__ d, long in_bytes, long coef_elems, long qt_elems, Enc& g) {
    Scan s;
    if (!read_scan(d, coef_elems, s) || (s.coef & 63)) return false;
    g.W = (int)d[D_W], g.H = (int)d[D_H], g.nc = s.nc, g.hs = s.hs, g.vs = s.vs, g.mcux = s.mcux, g.mcuy = s.mcuy;
    g.coef = s.coef, g.in = d[D_OUT], g.qt = d[D_QT];
    g.comp_off[0] = 0, g.comp_off[1] = s.off1, g.comp_off[2] = s.off2;  // of a grey image: unused (no kernel takes c >= nc)
    for (int c = 0; c < 3; ++c) {
        const int h = c == 0 ? g.hs : 1, v = c == 0 ? g.vs : 1, on = c < g.nc;
        g.bw[c] = on * g.mcux * h, g.bh[c] = on * g.mcuy * v;
        const int cw = c == 0 ? g.W : (g.W + g.hs - 1) / g.hs, ch = c == 0 ? g.H : (g.H + g.vs - 1) / g.vs;
        g.rw[c] = on * ((cw + 7) / 8), g.rh[c] = on * ((ch + 7) / 8);
    }
    if (g.qt < 0 || (g.qt & 63) || g.qt + g.nc * 64 > qt_elems) return false;
    if (g.in < 0 || g.in + (long long)g.W * g.H * g.nc > in_bytes) return false;
    return true;
}

// element c of a three-element member without a runtime index (which would put the struct into scratch memory)
template <typename T>
__device__ __forceinline__ T pick(const T (&a)[3], int c) { return c == 0 ? a[0] : (c == 1 ? a[1] : a[2]); }

// ---- kernel 1: pixels -> sample planes ----------------------------------------------------------------------------------
// A lane takes one cell of the chroma grid (hs x vs luma samples; tab[wg] = {image, chunk of PL_THREADS cells} over the
// 8 mcux x 8 mcuy cells of the padded grid): it converts the cell's pixels, stores the luma samples and, for a colour
// image, the downsampled Cb and Cr.  Source coordinates are clamped as libjpeg's buffers make them: luma to the image;
// chroma rows to the last downsampled row first and only then, at full resolution, to the image.
constexpr int PL_THREADS = 256;

__global__ void __launch_bounds__(PL_THREADS) jpeg_planes_kernel(const unsigned char* __restrict__ in, long in_bytes,
                                                                  const long long* __restrict__ desc, int N, long coef_elems,
                                                                  long qt_elems, const int* __restrict__ tab,
                                                                  unsigned char* __restrict__ planes) {
    const int n = tab[4 * blockIdx.x], chunk = tab[4 * blockIdx.x + 1];
    Enc g;
    if (!(n >= 0 && n < N && chunk >= 0 && load_enc(desc + (long)n * JP_DESC, in_bytes, coef_elems, qt_elems, g))) return;
    const int cellsx = g.mcux * 8, cellsy = g.mcuy * 8;
    const long cell = (long)chunk * PL_THREADS + threadIdx.x;
    if (cell >= (long)cellsx * cellsy) return;
    const int cy = (int)(cell / cellsx), cx = (int)(cell - (long)cy * cellsx);
    const unsigned char* src = in + g.in;
    unsigned char* PY = planes + g.coef;
    const int pitchY = g.bw[0] * 8;
    if (g.nc == 1) {
        const int sx = min(cx, g.W - 1), sy = min(cy, g.H - 1);
        PY[(long)cy * pitchY + cx] = src[(long)sy * g.W + sx];
        return;
    }
    const int ch = (g.H + g.vs - 1) / g.vs;
    const int cyc = min(cy, ch - 1);
    int sb = 0, sr = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (j >= g.vs) break;
        const int y = g.vs * cy + j;
        const int ly = min(y, g.H - 1), qy = min(g.vs * cyc + j, g.H - 1);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (i >= g.hs) break;
            const int x = g.hs * cx + i, sx = min(x, g.W - 1);
            const unsigned char* p = src + ((long)ly * g.W + sx) * 3;
            int r = p[0], gg = p[1], b = p[2];
            PY[(long)y * pitchY + x] = (unsigned char)((19595 * r + 38470 * gg + 7471 * b + 32768) >> 16);
            if (qy != ly) {
                p = src + ((long)qy * g.W + sx) * 3;
                r = p[0], gg = p[1], b = p[2];
            }
            sb += (-11059 * r - 21709 * gg + 32768 * b + (128 << 16) + 32767) >> 16;
            sr += (32768 * r - 27439 * gg - 5329 * b + (128 << 16) + 32767) >> 16;
        }
    }
    if (g.hs == 2 && g.vs == 2) {
        const int bias = 1 + (cx & 1);
        sb = (sb + bias) >> 2, sr = (sr + bias) >> 2;
    } else if (g.hs == 2) {
        const int bias = cx & 1;
        sb = (sb + bias) >> 1, sr = (sr + bias) >> 1;
    }
    const long o = (long)cy * cellsx + cx;  // the chroma planes' pitch is 8 mcux
    PY[g.comp_off[1] + o] = (unsigned char)sb;
    PY[g.comp_off[2] + o] = (unsigned char)sr;
}

// ---- kernel 2: sample planes -> quantised coefficients ------------------------------------------------------------------
// jpeg_fdct_islow's one-dimensional pass on eight values (CONST_BITS = 13, PASS1_BITS = 2).  ROWS: the first pass (outputs 0
// and 4 shifted left by 2, the others descaled by 11); otherwise the column pass (descaled by 2 and by 15).
template <bool ROWS>
__device__ __forceinline__ void fdct_1d(const int (&d)[8], int (&o)[8]) {
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int S = ROWS ? 11 : 15, R = 1 << (S - 1);
    if (ROWS) {
        o[0] = (int)((unsigned)(t10 + t11) << 2), o[4] = (int)((unsigned)(t10 - t11) << 2);
    } else {
        o[0] = (t10 + t11 + 2) >> 2, o[4] = (t10 - t11 + 2) >> 2;
    }
    int z1 = (t12 + t13) * 4433;
    o[2] = (z1 + t13 * 6270 + R) >> S;
    o[6] = (z1 - t12 * 15137 + R) >> S;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373, z2 *= -20995, z3 = z3 * (-16069) + z5, z4 = z4 * (-3196) + z5;
    o[7] = (a4 + z1 + z3 + R) >> S;
    o[5] = (a5 + z2 + z4 + R) >> S;
    o[3] = (a6 + z2 + z3 + R) >> S;
    o[1] = (a7 + z1 + z4 + R) >> S;
}

// A workgroup takes FD_BLOCKS consecutive blocks of one component's padded grid (tab[wg] = {image, component, first block}),
// eight lanes per block.  Lane j loads sample row j as one 8-byte vector and runs the row pass; the results cross to the
// lanes as columns through LDS (block stride 72 dwords, row stride 9, as in jpeg_idct_kernel: neither the row-wise nor the
// column-wise accesses meet a bank twice), lane j runs column j, the coefficients cross back, and lane j quantises
// coefficient row j against table row j and stores it as one 16-byte vector.  A dummy block (beyond the component's own
// block columns / rows) transforms the block whose DC it repeats — in a real block row the last real block of the row, in
// a dummy row the last block of the row above within its MCU — and keeps the DC alone.
constexpr int FD_THREADS = 256, FD_BLOCKS = FD_THREADS / 8, FD_BSTRIDE = 72, FD_RSTRIDE = 9;
typedef short short8 __attribute__((ext_vector_type(8)));
typedef unsigned short ushort8 __attribute__((ext_vector_type(8)));

__global__ void __launch_bounds__(FD_THREADS) jpeg_fdct_kernel(const unsigned char* __restrict__ planes, long in_bytes,
                                                                const long long* __restrict__ desc, int N,
                                                                const unsigned short* __restrict__ qtabs, long qt_elems,
                                                                const int* __restrict__ tab, short* __restrict__ coef, long coef_elems) {
    __shared__ int s_t[FD_BLOCKS * FD_BSTRIDE];
    const int n = tab[4 * blockIdx.x], c = tab[4 * blockIdx.x + 1], blk0 = tab[4 * blockIdx.x + 2];
    Enc g;
    bool ok = n >= 0 && n < N && c >= 0 && c < 3 && blk0 >= 0 && load_enc(desc + (long)n * JP_DESC, in_bytes, coef_elems, qt_elems, g);
    ok = ok && c < g.nc;
    const int t = threadIdx.x, lb = t >> 3, j = t & 7;
    const int bw = ok ? pick(g.bw, c) : 1, bh = ok ? pick(g.bh, c) : 0, rw = ok ? pick(g.rw, c) : 1, rh = ok ? pick(g.rh, c) : 1;
    const long long off = ok ? g.coef + pick(g.comp_off, c) : 0;
    const long nblk = (long)bw * bh;
    const long blk = (long)blk0 + lb;
    const bool live = ok && blk < nblk;
    int a[8], o[8];
    bool dummy = false;
    if (live) {
        const int by = (int)(blk / bw), bx = (int)(blk - (long)by * bw);
        const int h = c == 0 ? g.hs : 1;
        int sx = bx, sy = by;
        if (by >= rh) {
            dummy = true;
            sy = rh - 1;
            sx = bx / h * h + h - 1;
        }
        if (sx >= rw) {
            dummy = true;
            sx = rw - 1;
        }
        const unsigned char* src = planes + off + ((long)sy * 8 + j) * ((long)bw * 8) + sx * 8;
        const uint2 v = *reinterpret_cast<const uint2*>(src);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            a[e] = (int)((v.x >> (8 * e)) & 255) - 128;
            a[e + 4] = (int)((v.y >> (8 * e)) & 255) - 128;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = 0;
    }
    fdct_1d<true>(a, o);  // row j
    int* sb = s_t + lb * FD_BSTRIDE;
#pragma unroll
    for (int e = 0; e < 8; ++e) sb[j * FD_RSTRIDE + e] = o[e];
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = sb[e * FD_RSTRIDE + j];  // column j
    fdct_1d<false>(a, o);
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 8; ++e) sb[e * FD_RSTRIDE + j] = o[e];
    __syncthreads();
    if (!live) return;
    const ushort8 q = *reinterpret_cast<const ushort8*>(qtabs + g.qt + c * 64 + j * 8);
    short8 k;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int x = sb[j * FD_RSTRIDE + e];  // coefficient (row j, column e)
        const unsigned d = 8u * (q[e] ? (unsigned)q[e] : 1u);
        const unsigned m = ((unsigned)(x < 0 ? -x : x) + d / 2) / d;
        const int r = x < 0 ? -(int)m : (int)m;
        k[e] = (short)((dummy && (j | e)) ? 0 : r);
    }
    *reinterpret_cast<short8*>(coef + off + blk * 64 + j * 8) = k;
}

// ---- host: the Huffman stage --------------------------------------------------------------------------------------------
// Annex K.3: counts per code length 1 .. 16, then the values
const unsigned char kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const unsigned char kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const unsigned char kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const unsigned char kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
const unsigned char kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
    0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
    0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};
const unsigned char kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
const unsigned char kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
    0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
    0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
    0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};


HuffSpec make_spec(const unsigned char* bits, const unsigned char* vals, int nvals) {
    HuffSpec s;
    memset(&s, 0, sizeof(s));
    memcpy(s.bits, bits, 16);
    memcpy(s.vals, vals, nvals);
    s.nvals = nvals;
    return s;
}

struct Tables {
    Codes t[4];  // DC 0, AC 0, DC 1, AC 1
    explicit Tables(const HuffSpec* s) {
        for (int i = 0; i < 4; ++i) t[i] = Codes(s[i].bits, s[i].vals);
    }
};

const Tables& tables() {
    static const Tables t(annex_k());
    return t;
}

long image_bound(const Geo& g, int ri) {
    const long mcus = (long)g.mcux * g.mcuy;
    return kHeaderBytes + g.blocks * kBlockBytes + (ri > 0 ? (mcus - 1) / ri * 4 : 0);
}

// bytes into [p, end): a write that does not fit is dropped and remembered
struct Put {
    unsigned char *p, *end;
    unsigned long long acc = 0;
    int n = 0;
    bool over = false;
    inline void byte(unsigned b) {
        if (p < end) *p++ = (unsigned char)b;
        else over = true;
    }
    inline void be16(unsigned v) { byte(v >> 8), byte(v & 255); }
    inline void bits(unsigned code, int size) {
        acc = acc << size | code;
        n += size;
        while (n >= 8) {
            const unsigned b = (unsigned)(acc >> (n - 8)) & 255;
            byte(b);
            if (b == 255) byte(0);
            n -= 8;
        }
    }
    inline void flush() {
        if (n) bits((1u << (8 - n)) - 1, 8 - n);
        acc = 0;
    }
};

inline int nbits(int v) {
    v = v < 0 ? -v : v;
    return v ? 32 - __builtin_clz((unsigned)v) : 0;
}

void put_dht(Put& w, int tc_th, const HuffSpec& s) {
    w.be16(0xFFC4), w.be16(2 + 1 + 16 + s.nvals), w.byte(tc_th);
    for (int i = 0; i < 16; ++i) w.byte(s.bits[i]);
    for (int i = 0; i < s.nvals; ++i) w.byte(s.vals[i]);
}

void put_header(Put& w, const unsigned short* q, const Geo& g, int ri, const HuffSpec* specs) {
    int tq[3] = {0, 1, 1};
    if (g.nc == 3 && memcmp(q + 64, q + 128, 64 * sizeof(unsigned short)) != 0) tq[2] = 2;
    w.be16(0xFFD8);
    w.be16(0xFFE0), w.be16(16);
    const unsigned char jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    for (int i = 0; i < 14; ++i) w.byte(jfif[i]);
    for (int c = 0; c < g.nc; ++c) {
        if (c == 2 && tq[2] == 1) break;
        w.be16(0xFFDB), w.be16(67), w.byte(tq[c]);
        for (int k = 0; k < 64; ++k) w.byte(q[64 * c + kZigzag[k]]);
    }
    w.be16(0xFFC0), w.be16(8 + 3 * g.nc), w.byte(8), w.be16(g.H), w.be16(g.W), w.byte(g.nc);
    for (int c = 0; c < g.nc; ++c) w.byte(c + 1), w.byte(g.h[c] << 4 | g.v[c]), w.byte(tq[c]);
    put_dht(w, 0x00, specs[0]);
    put_dht(w, 0x10, specs[1]);
    if (g.nc == 3) {
        put_dht(w, 0x01, specs[2]);
        put_dht(w, 0x11, specs[3]);
    }
    if (ri > 0) w.be16(0xFFDD), w.be16(4), w.be16(ri);
    w.be16(0xFFDA), w.be16(6 + 2 * g.nc), w.byte(g.nc);
    for (int c = 0; c < g.nc; ++c) w.byte(c + 1), w.byte(c == 0 ? 0x00 : 0x11);
    w.byte(0), w.byte(63), w.byte(0);
}

// The scan of one image, block after block in MCU order with the DC predictors reset at every restart interval, handed to
// `sink`: restart(k) before interval k > 0, then per block dc(table, category, extra bits) and ac(table, run << 4 | size,
// size, extra bits).  The gather pass of optimize and the coding pass walk the same way; a status other than ES_OK ends it.
template <typename Sink>
int walk_scan(const short* coef, const Geo& g, int ri, Sink& sink) {
    int pred[3] = {0, 0, 0};
    const long mcus = (long)g.mcux * g.mcuy;
    long to_restart = ri;
    int next_rst = 0;
    for (long mcu = 0; mcu < mcus; ++mcu) {
        if (ri > 0 && mcu && to_restart == 0) {
            sink.restart(next_rst);
            next_rst = (next_rst + 1) & 7;
            pred[0] = pred[1] = pred[2] = 0;
            to_restart = ri;
        }
        --to_restart;
        const long my = mcu / g.mcux, mx = mcu - my * g.mcux;
        for (int c = 0; c < g.nc; ++c) {
            const int t = c ? 1 : 0;
            for (int v = 0; v < g.v[c]; ++v)
                for (int u = 0; u < g.h[c]; ++u) {
                    const short* k64 = coef + g.coef + g.comp_off[c] + ((my * g.v[c] + v) * g.bw[c] + mx * g.h[c] + u) * 64;
                    const int d = (int)k64[0] - pred[c];
                    pred[c] = k64[0];
                    int s = nbits(d);
                    if (s > 11) return ES_DC_RANGE;
                    sink.dc(t, s, (unsigned)(d < 0 ? d - 1 : d) & ((1u << s) - 1));
                    int run = 0;
                    for (int k = 1; k < 64; ++k) {
                        const int x = k64[kZigzag[k]];
                        if (x == 0) {
                            ++run;
                            continue;
                        }
                        while (run > 15) {
                            sink.ac(t, 0xF0, 0, 0);
                            run -= 16;
                        }
                        s = nbits(x);
                        if (s > 10) return ES_AC_RANGE;
                        sink.ac(t, run << 4 | s, s, (unsigned)(x < 0 ? x - 1 : x) & ((1u << s) - 1));
                        run = 0;
                    }
                    if (run) sink.ac(t, 0, 0, 0);
                }
        }
        if (sink.mcu_done()) return ES_NO_ROOM;
    }
    return ES_OK;
}

struct CountSink {
    long long freq[4][256];
    CountSink() { memset(freq, 0, sizeof(freq)); }
    inline void restart(int) {}
    inline void dc(int t, int s, unsigned) { ++freq[2 * t][s]; }
    inline void ac(int t, int rs, int, unsigned) { ++freq[2 * t + 1][rs]; }
    inline bool mcu_done() { return false; }
};

struct CodeSink {
    Put& w;
    const Codes* T;
    inline void restart(int k) {
        w.flush();
        w.be16(0xFFD0 + k);
    }
    inline void dc(int t, int s, unsigned extra) {
        w.bits(T[2 * t].code[s], T[2 * t].size[s]);
        if (s) w.bits(extra, s);
    }
    inline void ac(int t, int rs, int s, unsigned extra) {
        w.bits(T[2 * t + 1].code[rs], T[2 * t + 1].size[rs]);
        if (s) w.bits(extra, s);
    }
    inline bool mcu_done() { return w.over; }
};

// one stream into [out, out + room): a status and the stream's length.  optimize: a gather pass over the scan first, and
// the image's own tables (libjpeg's jpeg_gen_optimal_table) in its DHT segments and its scan.
int encode_image(const short* coef, const unsigned short* qtabs, const Geo& g, int ri, unsigned char* out, long room, long long* len, bool optimize) {
    int s = check_qtabs(qtabs, g);
    if (s != ES_OK) return s;
    HuffSpec own[4];
    Tables* mine = nullptr;
    if (optimize) {
        CountSink cs;
        if ((s = walk_scan(coef, g, ri, cs)) != ES_OK) return s;
        for (int t = 0; t < (g.nc == 3 ? 4 : 2); ++t)
            if ((s = optimal_table(cs.freq[t], own[t])) != ES_OK) return s;
        if (g.nc != 3) own[2] = own[0], own[3] = own[1];
        mine = new Tables(own);
    }
    Put w{out, out + room};
    put_header(w, qtabs + g.qt, g, ri, optimize ? own : annex_k());
    CodeSink code{w, optimize ? mine->t : tables().t};
    s = walk_scan(coef, g, ri, code);
    delete mine;
    if (s != ES_OK) return s;
    w.flush();
    w.be16(0xFFD9);
    if (w.over) return ES_NO_ROOM;
    *len = w.p - out;
    return ES_OK;
}

}  // namespace

namespace dbn_jpeg {

Codes::Codes(const unsigned char* bits, const unsigned char* vals) {
    memset(code, 0, sizeof(code));
    memset(size, 0, sizeof(size));
    int c = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < bits[l - 1]; ++i, ++k, ++c) code[vals[k]] = (unsigned short)c, size[vals[k]] = (unsigned char)l;
        c <<= 1;
    }
}

const HuffSpec* annex_k() {
    static const HuffSpec s[4] = {make_spec(kDcLumaBits, kDcVals, 12), make_spec(kAcLumaBits, kAcLumaVals, 162),
                                  make_spec(kDcChromaBits, kDcVals, 12), make_spec(kAcChromaBits, kAcChromaVals, 162)};
    return s;
}

int load_geo(const long long* d, long coef_elems, long qt_elems, Geo& g) {
    if (d[D_STATUS] != 0) return ES_NO_IMAGE;
    Scan s;
    if (!read_scan(d, coef_elems, s)) return ES_BAD_DESC;
    g.W = (int)d[D_W], g.H = (int)d[D_H], g.nc = s.nc, g.mcux = s.mcux, g.mcuy = s.mcuy;
    g.coef = (long)s.coef, g.qt = (long)d[D_QT], g.blocks = (long)s.blocks;
    g.comp_off[0] = 0, g.comp_off[1] = (long)s.off1, g.comp_off[2] = (long)s.off2;
    for (int c = 0; c < s.nc; ++c) {
        g.h[c] = c == 0 ? s.hs : 1, g.v[c] = c == 0 ? s.vs : 1;
        g.bw[c] = s.mcux * g.h[c], g.bh[c] = s.mcuy * g.v[c];
    }
    if (g.qt < 0 || g.qt + s.nc * 64 > qt_elems) return ES_BAD_DESC;
    return ES_OK;
}

int check_qtabs(const unsigned short* qtabs, const Geo& g) {
    const unsigned short* q = qtabs + g.qt;
    for (int i = 0; i < 64 * g.nc; ++i)
        if (q[i] < 1 || q[i] > 255) return ES_TABLE;
    return ES_OK;
}

long write_header(const unsigned short* qtabs, const Geo& g, int ri, const HuffSpec* specs, unsigned char* out, long room) {
    Put w{out, out + room};
    put_header(w, qtabs + g.qt, g, ri, specs);
    return w.over ? -1 : (long)(w.p - out);
}

// jchuff.c jpeg_gen_optimal_table: a pseudo-symbol 256 of count 1 keeps the all-ones code unused; the two least counts are
// merged until one tree is left, a tie going to the larger symbol; code lengths above 16 are shortened by moving pairs of
// symbols up (the bits[] adjustment of section K.2); the pseudo-symbol's place, the longest code, is dropped; symbols are
// listed by length, then by value.  A DC table has at most 12 symbols and an AC table at most 162 (runs 0 .. 15 with sizes
// 1 .. 10, EOB and ZRL), so four such DHT segments are never longer than the Annex K ones kHeaderBytes counts.
int optimal_table(const long long* freq_in, HuffSpec& out) {
    constexpr int MAX_CLEN = 32;
    long long freq[257];
    int bits[MAX_CLEN + 1] = {0}, codesize[257] = {0}, others[257];
    for (int i = 0; i < 256; ++i) freq[i] = freq_in[i] > 0 ? freq_in[i] : 0;
    freq[256] = 1;
    for (int i = 0; i < 257; ++i) others[i] = -1;
    for (;;) {
        int c1 = -1, c2 = -1;
        long long v = 0x7fffffffffffffffLL;
        for (int i = 0; i <= 256; ++i)
            if (freq[i] && freq[i] <= v) v = freq[i], c1 = i;
        v = 0x7fffffffffffffffLL;
        for (int i = 0; i <= 256; ++i)
            if (freq[i] && freq[i] <= v && i != c1) v = freq[i], c2 = i;
        if (c2 < 0) break;
        freq[c1] += freq[c2];
        freq[c2] = 0;
        for (++codesize[c1]; others[c1] >= 0;) c1 = others[c1], ++codesize[c1];
        others[c1] = c2;
        for (++codesize[c2]; others[c2] >= 0;) c2 = others[c2], ++codesize[c2];
    }
    for (int i = 0; i <= 256; ++i)
        if (codesize[i]) {
            if (codesize[i] > MAX_CLEN) return ES_CODE_LENGTH;
            ++bits[codesize[i]];
        }
    int i;
    for (i = MAX_CLEN; i > 16; --i)
        while (bits[i] > 0) {
            int j = i - 2;
            while (bits[j] == 0) --j;
            bits[i] -= 2, ++bits[i - 1], bits[j + 1] += 2, --bits[j];
        }
    while (bits[i] == 0) --i;
    --bits[i];
    memset(&out, 0, sizeof(out));
    for (int l = 1; l <= 16; ++l) out.bits[l - 1] = (unsigned char)bits[l];
    int p = 0;
    for (int l = 1; l <= MAX_CLEN; ++l)
        for (int j = 0; j < 256; ++j)
            if (codesize[j] == l) out.vals[p++] = (unsigned char)j;
    out.nvals = p;
    return ES_OK;
}

}  // namespace dbn_jpeg

extern "C" {
// pixels: in_bytes bytes holding every image; desc int64 [N][24] as dbn_jpeg_entropy_batch writes it, with field 4 the byte
// offset of the image's first pixel in `pixels` (any alignment) and `components` 1 for uint8 [H][W] grey, 3 for uint8
// [H][W][3] RGB; qtabs uint16 [N][3][64] natural order; tab_planes int32 [n_planes][4] = {image, chunk of 256 cells, 0, 0} over
// the 8 mcux x 8 mcuy cells of the image; tab_fdct int32 [n_fdct][4] = {image, component, first block, 0}, one entry per 32
// blocks of the padded grid; planes: a workspace of coef_elems bytes; coef: coef_elems int16, every block of every image
// with status 0 written once.
int dbn_jpeg_forward(const unsigned char* pixels, long in_bytes, const long long* desc, const unsigned short* qtabs, int N,
                     const int* tab_planes, int n_planes, const int* tab_fdct, int n_fdct, unsigned char* planes, short* coef, long coef_elems,
                     void* stream) {
    DBN_REQUIRE(pixels && desc && qtabs && tab_planes && tab_fdct && planes && coef && N > 0 && n_planes > 0 && n_fdct > 0 && in_bytes > 0 &&
                coef_elems > 0);
    DBN_REQUIRE((reinterpret_cast<size_t>(coef) & 15) == 0 && (reinterpret_cast<size_t>(qtabs) & 15) == 0 &&
                (reinterpret_cast<size_t>(planes) & 7) == 0);
    const long qt_elems = (long)N * 192;
    hipLaunchKernelGGL(jpeg_planes_kernel, dim3((unsigned)n_planes), dim3(PL_THREADS), 0, (hipStream_t)stream, pixels, in_bytes, desc, N,
                       coef_elems, qt_elems, tab_planes, planes);
    hipLaunchKernelGGL(jpeg_fdct_kernel, dim3((unsigned)n_fdct), dim3(FD_THREADS), 0, (hipStream_t)stream, planes, in_bytes, desc, N, qtabs,
                       qt_elems, tab_fdct, coef, coef_elems);
    return dbn_status();
}

// per_image[n] (may be NULL) = bytes image n's stream can need at most (0 for a descriptor that cannot be encoded); the sum, -1
// for bad arguments.  restart_interval in MCUs, 0 .. 65535.
long dbn_jpeg_encode_bound(const long long* desc, int N, int restart_interval, long long* per_image) {
    if (!desc || N < 0 || restart_interval < 0 || restart_interval > 65535) return -1;
    long total = 0;
    for (int n = 0; n < N; ++n) {
        Geo g;
        const long b = load_geo(desc + (long)n * JP_DESC, 0x7fffffffffffffffL, 0x7fffffffffffffffL, g) == ES_OK ? image_bound(g, restart_interval) : 0;
        if (per_image) per_image[n] = b;
        total += b;
    }
    return total;
}

// freq int64 [256] -> bits uint8 [16] (symbols per code length 1 .. 16), vals uint8 [256] and *nvals: the table libjpeg's
// jpeg_gen_optimal_table makes of these counts (what Pillow's optimize=True writes).  1: no count is positive, a count is
// negative, or libjpeg itself gives up (a code of more than 32 bits).
int dbn_jpeg_optimal_table(const long long* freq, unsigned char* bits, unsigned char* vals, int* nvals) {
    DBN_REQUIRE(freq && bits && vals && nvals);
    bool any = false;
    for (int i = 0; i < 256; ++i) {
        DBN_REQUIRE(freq[i] >= 0);
        any = any || freq[i] > 0;
    }
    DBN_REQUIRE(any);
    HuffSpec s;
    DBN_REQUIRE(optimal_table(freq, s) == ES_OK);
    memcpy(bits, s.bits, 16);
    memcpy(vals, s.vals, 256);
    *nvals = s.nvals;
    return DBN_OK;
}

// coef / desc / qtabs: the layout of dbn_jpeg_entropy_batch, on the host.  Image n's stream goes to out[offs[n] .. offs[n + 1])
// (offs int64 [N + 1], ascending, offs[N] <= out_bytes) and lens[n] receives its length; no byte outside an image's slot is
// written.  status[n]: 0 coded, 1 the descriptor's own status is not 0, 2 bad descriptor, 3 a quantisation value outside
// 1 .. 255, 4 a DC difference of more than 11 bits, 5 an AC coefficient of more than 10 bits, 6 the slot is too small, 7
// (optimize only) libjpeg's table builder gives up; an image that is not coded has length 0 and fails alone.  optimize: each
// image's own Huffman tables, as libjpeg's optimize_coding makes them, in place of the Annex K ones.
int dbn_jpeg_encode_batch_opt(const short* coef, long coef_elems, const long long* desc, const unsigned short* qtabs, int N, int restart_interval,
                              unsigned char* out, long out_bytes, const long long* offs, long long* lens, int* status, int threads, int optimize) {
    DBN_REQUIRE(coef && desc && qtabs && out && offs && lens && status && N > 0 && coef_elems >= 0 && out_bytes >= 0);
    DBN_REQUIRE(restart_interval >= 0 && restart_interval <= 65535 && offs[0] >= 0 && offs[N] <= out_bytes);
    for (int n = 0; n < N; ++n) DBN_REQUIRE(offs[n + 1] >= offs[n]);
    const long qt_elems = (long)N * 192;
    on_threads(N, threads, [&](int n) {
        Geo g;
        lens[n] = 0;
        int s = load_geo(desc + (long)n * JP_DESC, coef_elems, qt_elems, g);
        if (s == ES_OK) s = encode_image(coef, qtabs, g, restart_interval, out + offs[n], (long)(offs[n + 1] - offs[n]), lens + n, optimize != 0);
        if (s != ES_OK) lens[n] = 0;
        status[n] = s;
    });
    return DBN_OK;
}

int dbn_jpeg_encode_batch(const short* coef, long coef_elems, const long long* desc, const unsigned short* qtabs, int N, int restart_interval,
                          unsigned char* out, long out_bytes, const long long* offs, long long* lens, int* status, int threads) {
    return dbn_jpeg_encode_batch_opt(coef, coef_elems, desc, qtabs, N, restart_interval, out, out_bytes, offs, lens, status, threads, 0);
}

}  // extern "C"
