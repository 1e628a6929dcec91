// Photometric augmentation of a packed uint8 RGB batch (db_text_minimal_amd/photometric.py; ABI and the record: include/dbnet_hip.h;
// the arithmetic: photometric.h): torchvision's ColorJitter as it acts on PIL images, bit for bit.
//   photo_sums_kernel   only when a plan holds contrast: per such image the sum of convert('L') over the image as the contrast step
//                       meets it (the steps before it applied on the fly); per workgroup a partial sum, then one 64-bit integer
//                       atomic add per image the workgroup has touched, so the sums do not depend on the order of arrival;
//   photo_apply_kernel  every pixel through its image's plan, the mean grey formed from the sum in float64 in the kernel.
// A workgroup takes chunks of PH_CHUNK_PIXELS pixels of one image (apply: grid-stride over the chunks of the batch; sums: a run of
// consecutive ones); the image of a chunk is found by a bisection that is the same in every lane.  A lane takes four pixels, 12
// bytes, with byte-aligned wide accesses (images start at any byte), and the last one to three pixels of an image byte by byte.  No
// workgroup waits for another one, and every address is formed from record values that the host entry point has checked against the
// buffer length before the launch.
#include "common.h"
#include "photometric.h"

namespace {

constexpr int PH_THREADS = PH_CHUNK_PIXELS / 4;
constexpr long PH_MAX_IMAGES = 65535, PH_MAX_SIDE = 16384;

// three dwords at any byte alignment
struct __attribute__((packed, aligned(1))) ph_bytes12 {
    unsigned w[3];
};

__device__ __forceinline__ int ph_image_of(const long long* __restrict__ desc, int N, long chunk) {
    int lo = 0, hi = N - 1;  // the last image whose first chunk is at or before this one
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (desc[(long)mid * PH_D + PH_CHUNK] <= chunk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The pixels of one chunk that this lane owns, each through steps [0, end) of the plan.  SUM: returns the sum of their greys and
// writes nothing; otherwise writes them to dst and returns 0.
template <bool SUM>
__device__ __forceinline__ unsigned ph_lane(const unsigned char* src, unsigned char* dst, long first, long pixels, const ph_plan& plan, int end, int m) {
    const long px = first + 4 * (long)threadIdx.x;
    unsigned grey = 0;
    if (px + 4 <= pixels) {
        const ph_bytes12 in = *reinterpret_cast<const ph_bytes12*>(src + 3 * px);
        ph_bytes12 out = {{0u, 0u, 0u}};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int c[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) c[k] = (int)((in.w[(3 * j + k) >> 2] >> (8 * ((3 * j + k) & 3))) & 255u);
            ph_steps(plan, end, m, c[0], c[1], c[2]);
            if (SUM) grey += (unsigned)ph_luma(c[0], c[1], c[2]);
#pragma unroll
            for (int k = 0; k < 3; ++k) out.w[(3 * j + k) >> 2] |= (unsigned)c[k] << (8 * ((3 * j + k) & 3));
        }
        if (!SUM) *reinterpret_cast<ph_bytes12*>(dst + 3 * px) = out;
    } else {
        for (long q = px; q < px + 4 && q < pixels; ++q) {  // the tail of the image: at most three pixels
            int r = src[3 * q], g = src[3 * q + 1], b = src[3 * q + 2];
            ph_steps(plan, end, m, r, g, b);
            if (SUM) grey += (unsigned)ph_luma(r, g, b);
            else dst[3 * q] = (unsigned char)r, dst[3 * q + 1] = (unsigned char)g, dst[3 * q + 2] = (unsigned char)b;
        }
    }
    return grey;
}

// the sum of v over the workgroup, added to *dst by one atomic; every lane of the workgroup calls it
__device__ __forceinline__ void ph_flush(unsigned long long v, unsigned long long* dst, unsigned long long* part) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long total = 0;
#pragma unroll
        for (int w = 0; w < PH_THREADS / 64; ++w) total += part[w];
        atomicAdd(dst, total);
    }
    __syncthreads();
}

// A workgroup takes a run of consecutive chunks, not a stride: the chunks of one image that it meets follow each other, each lane
// keeps its own sum over them, and the workgroup folds and adds once per image it has touched (a stride would put every chunk of a
// workgroup into another image: one atomic per chunk, all on a few addresses).
__global__ __launch_bounds__(PH_THREADS) void photo_sums_kernel(const unsigned char* __restrict__ in, const long long* __restrict__ desc, int N,
                                                                long chunks, unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long part[PH_THREADS / 64];
    const long per = (chunks + gridDim.x - 1) / gridDim.x;
    const long begin = (long)blockIdx.x * per, end = begin + per < chunks ? begin + per : chunks;
    int held = -1;  // the image whose greys `acc` holds
    unsigned long long acc = 0;
    for (long chunk = begin; chunk < end; ++chunk) {  // every condition below is the same in all lanes of the workgroup
        const int n = ph_image_of(desc, N, chunk);
        const long long* d = desc + (long)n * PH_D;
        const ph_plan plan = ph_unpack(d);
        const int at = ph_contrast_step(plan);
        if (at < 0) continue;
        if (n != held) {
            if (held >= 0) ph_flush(acc, sums + held, part);
            held = n, acc = 0;
        }
        acc += ph_lane<true>(in + d[PH_OFF], nullptr, (chunk - d[PH_CHUNK]) * PH_CHUNK_PIXELS, d[PH_H] * d[PH_W], plan, at, 0);
    }
    if (held >= 0) ph_flush(acc, sums + held, part);
}

// in == out is allowed: a lane reads the bytes of its pixels before it writes them, and no other lane touches them
__global__ __launch_bounds__(PH_THREADS) void photo_apply_kernel(const unsigned char* in, unsigned char* out, const long long* __restrict__ desc, int N,
                                                                 long chunks, const unsigned long long* __restrict__ sums) {
    for (long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const int n = ph_image_of(desc, N, chunk);
        const long long* d = desc + (long)n * PH_D;
        const ph_plan plan = ph_unpack(d);
        const long pixels = d[PH_H] * d[PH_W];
        const int m = ph_contrast_step(plan) >= 0 ? ph_mean(sums[n], pixels) : 0;
        ph_lane<false>(in + d[PH_OFF], out + d[PH_OFF], (chunk - d[PH_CHUNK]) * PH_CHUNK_PIXELS, pixels, plan, ph_count(plan), m);
    }
}

// every value a kernel bounds a loop or forms an address with, against the length of the buffers -> chunks of the batch, whether a
// plan holds contrast
int photo_validate(const long long* hdesc, int N, long bytes, long* chunks, bool* contrast) {
    DBN_REQUIRE(hdesc && N >= 1 && N <= PH_MAX_IMAGES && bytes > 0);
    long end = 0, chunk = 0;
    *contrast = false;
    for (int n = 0; n < N; ++n) {
        const long long* d = hdesc + (long)n * PH_D;
        const long h = d[PH_H], w = d[PH_W];
        DBN_REQUIRE(h >= 1 && h <= PH_MAX_SIDE && w >= 1 && w <= PH_MAX_SIDE);
        DBN_REQUIRE(d[PH_OFF] >= end && d[PH_OFF] <= bytes && 3 * h * w <= bytes - d[PH_OFF]);  // in order: no two images overlap
        end = d[PH_OFF] + 3 * h * w;
        DBN_REQUIRE(d[PH_CHUNK] == chunk);
        chunk += (h * w + PH_CHUNK_PIXELS - 1) / PH_CHUNK_PIXELS;
        const ph_plan plan = ph_unpack(d);
        const int steps = ph_count(plan);
        DBN_REQUIRE(steps <= 4 && (unsigned long long)d[PH_OPS] >> (4 * (steps + 1)) == 0);
        unsigned seen = 0;
        for (int k = 0; k < steps; ++k) {
            const int op = ph_op(plan, k);
            DBN_REQUIRE(op >= PH_BRIGHTNESS && op <= PH_HUE && !(seen & (1u << op)));  // each operation at most once: one sum per image
            seen |= 1u << op;
            if (op == PH_HUE)
                DBN_REQUIRE(ph_val(plan, k) <= 255u);
            else
                DBN_REQUIRE(isfinite(ph_factor(ph_val(plan, k))));
        }
        if (seen & (1u << PH_CONTRAST)) *contrast = true;
    }
    *chunks = chunk;
    return DBN_OK;
}

}  // namespace

int dbn_color_jitter_u8(const unsigned char* in, unsigned char* out, long bytes, const long long* hdesc, const long long* desc, int N,
                        unsigned long long* sums, void* stream) {
    long chunks = 0;
    bool contrast = false;
    const int rc = photo_validate(hdesc, N, bytes, &chunks, &contrast);
    if (rc != DBN_OK) return rc;
    DBN_REQUIRE(in && out && desc && (sums || !contrast));
    const unsigned grid = (unsigned)dbn_grid(chunks, 1, 4096);
    if (contrast) {
        if (hipMemsetAsync(sums, 0, sizeof(unsigned long long) * (size_t)N, (hipStream_t)stream) != hipSuccess) return dbn_status();
        hipLaunchKernelGGL(photo_sums_kernel, dim3(grid), dim3(PH_THREADS), 0, (hipStream_t)stream, in, desc, N, chunks, sums);
    }
    hipLaunchKernelGGL(photo_apply_kernel, dim3(grid), dim3(PH_THREADS), 0, (hipStream_t)stream, in, out, desc, N, chunks, sums);
    return dbn_status();
}

int dbn_color_jitter_host(const unsigned char* in, unsigned char* out, long bytes, const long long* hdesc, int N) {
    long chunks = 0;
    bool contrast = false;
    const int rc = photo_validate(hdesc, N, bytes, &chunks, &contrast);
    if (rc != DBN_OK) return rc;
    DBN_REQUIRE(in && out);
    for (int n = 0; n < N; ++n) {
        const long long* d = hdesc + (long)n * PH_D;
        const ph_plan plan = ph_unpack(d);
        const long pixels = d[PH_H] * d[PH_W];
        const int at = ph_contrast_step(plan);
        int m = 0;
        if (at >= 0) {
            unsigned long long sum = 0;
            for (long q = 0; q < pixels; ++q) {
                const unsigned char* s = in + d[PH_OFF] + 3 * q;
                int r = s[0], g = s[1], b = s[2];
                ph_steps(plan, at, 0, r, g, b);
                sum += (unsigned)ph_luma(r, g, b);
            }
            m = ph_mean(sum, pixels);
        }
        for (long q = 0; q < pixels; ++q) {
            const unsigned char* s = in + d[PH_OFF] + 3 * q;
            int r = s[0], g = s[1], b = s[2];
            ph_steps(plan, ph_count(plan), m, r, g, b);
            unsigned char* o = out + d[PH_OFF] + 3 * q;
            o[0] = (unsigned char)r, o[1] = (unsigned char)g, o[2] = (unsigned char)b;
        }
    }
    return DBN_OK;
}
