// Optimizer extensions over the flat fp32 buffers (include/dbnet_hip.h "optimizer extensions"): gradient accumulation, the global
// gradient norm in float64, and Adam with AMSGrad, L2 weight decay and norm clipping.  adam_kernel of pointwise.hip stays the default
// step; adam_ex_kernel<false> with no clipping and no decay performs the same fp32 operations in the same order (-ffp-contract=off:
// no fused multiply-add is formed in either), so the two agree bit for bit.
#include "common.h"

// ----------------------------------------------------------------------------------
// acc = g (first) or acc += g: one fp32 add per element
// ----------------------------------------------------------------------------------
__global__ void grad_accumulate_kernel(float* __restrict__ acc, const float* __restrict__ g, long n, int first) {
    const long n4 = n >> 2;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
        reinterpret_cast<f32x4*>(acc)[i] = first ? gg : reinterpret_cast<f32x4*>(acc)[i] + gg;
    }
    // tail
    const long t = (n4 << 2) + blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (t < n) acc[t] = first ? g[t] : acc[t] + g[t];
}

// ----------------------------------------------------------------------------------
// sum of squares in float64.  Workgroup b owns the elements [b SQ_CHUNK, (b + 1) SQ_CHUNK): thread t adds quads t, t + 256, ... of the
// chunk in that order, the 64 lanes of a wave are folded by a fixed butterfly and the four waves in wave order.  Nothing depends on the
// grid size or on which workgroup runs when, so partials[b] and their index-order sum are functions of (g, n) alone.
// ----------------------------------------------------------------------------------
constexpr int SQ_THREADS = 256;
constexpr int SQ_QUADS = 16;                             // f32x4 loads per thread
constexpr long SQ_CHUNK = 4L * SQ_THREADS * SQ_QUADS;    // 16384 elements = 64 KiB per workgroup
constexpr int SQ_TILE = 2048;                            // partials staged in LDS per round of the final sum

__global__ __launch_bounds__(SQ_THREADS) void grad_sqnorm_part_kernel(const float* __restrict__ g, long n, double* __restrict__ partials) {
    __shared__ double wave_sum[SQ_THREADS / 64];
    const long base = blockIdx.x * SQ_CHUNK;
    double s = 0.0;
#pragma unroll 4
    for (int j = 0; j < SQ_QUADS; ++j) {
        const long e0 = base + 4L * (j * SQ_THREADS + threadIdx.x);
        if (e0 + 3 < n) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(g + e0);
#pragma unroll
            for (int e = 0; e < 4; ++e) s += (double)q[e] * (double)q[e];
        } else {
            for (int e = 0; e < 4; ++e)
                if (e0 + e < n) s += (double)g[e0 + e] * (double)g[e0 + e];
        }
    }
    s = dbn_wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = wave_sum[0];
        for (int w = 1; w < SQ_THREADS / 64; ++w) t += wave_sum[w];
        partials[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(SQ_THREADS) void grad_sqnorm_final_kernel(const double* __restrict__ partials, long nparts, double* __restrict__ out) {
    __shared__ double tile[SQ_TILE];
    double total = 0.0;
    for (long lo = 0; lo < nparts; lo += SQ_TILE) {
        const int cnt = (int)(nparts - lo < SQ_TILE ? nparts - lo : SQ_TILE);
        for (int i = threadIdx.x; i < cnt; i += SQ_THREADS) tile[i] = partials[lo + i];
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll 8
            for (int i = 0; i < cnt; ++i) total += tile[i];  // index order
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = total;
}

// ----------------------------------------------------------------------------------
// Adam over one flat fp32 buffer with the options torch.optim.Adam / clip_grad_norm_ add to the plain step
// ----------------------------------------------------------------------------------
struct AdamCoef {
    float lr_over_bc1, b1, b2, eps, inv_sqrt_bc2, wd;
};

// one element: the arithmetic of adam_kernel (pointwise.hip), operation for operation, plus the decay term and the running maximum
template <bool AMS>
__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, float& vmax, float gs, const AdamCoef& c) {
    float gg = g * gs;
    if (c.wd != 0.f) gg = gg + c.wd * p;
    m = c.b1 * m + (1.f - c.b1) * gg;
    v = c.b2 * v + (1.f - c.b2) * gg * gg;
    float root = v;
    if constexpr (AMS) {
        vmax = (v > vmax || v != v) ? v : vmax;  // torch.maximum: a NaN propagates
        root = vmax;
    }
    const float denom = sqrtf(root) * c.inv_sqrt_bc2 + c.eps;
    p -= c.lr_over_bc1 * (m / denom);
}

template <bool AMS>
__global__ void adam_ex_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                               float* __restrict__ vmax, long n, AdamCoef c, float gscale, const double* __restrict__ sqnorm,
                               float max_norm) {
    float gs = gscale;
    if (sqnorm) {  // every thread forms the clip coefficient from the device value: the host never reads the norm
        const double norm = fabs((double)gscale) * sqrt(sqnorm[0]);
        const double q = (double)max_norm / (norm + 1e-6);
        gs = (float)((q > 1.0 ? 1.0 : q) * (double)gscale);  // (a NaN q stays NaN)
    }
    const long n4 = n >> 2;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        f32x4 pp = reinterpret_cast<f32x4*>(p)[i];
        const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
        f32x4 mm = reinterpret_cast<f32x4*>(m)[i];
        f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
        f32x4 vx = {0.f, 0.f, 0.f, 0.f};
        if constexpr (AMS) vx = reinterpret_cast<f32x4*>(vmax)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {  // (a reference cannot bind to a vector element)
            float pe = pp[e], me = mm[e], ve = vv[e], xe = vx[e];
            adam_element<AMS>(pe, gg[e], me, ve, xe, gs, c);
            pp[e] = pe, mm[e] = me, vv[e] = ve, vx[e] = xe;
        }
        reinterpret_cast<f32x4*>(p)[i] = pp;
        reinterpret_cast<f32x4*>(m)[i] = mm;
        reinterpret_cast<f32x4*>(v)[i] = vv;
        if constexpr (AMS) reinterpret_cast<f32x4*>(vmax)[i] = vx;
    }
    // tail
    const long t = (n4 << 2) + blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (t < n) {
        float pp = p[t], mm = m[t], vv = v[t], vx = 0.f;
        if constexpr (AMS) vx = vmax[t];
        adam_element<AMS>(pp, g[t], mm, vv, vx, gs, c);
        p[t] = pp;
        m[t] = mm;
        v[t] = vv;
        if constexpr (AMS) vmax[t] = vx;
    }
}

extern "C" {

int dbn_grad_accumulate(float* acc, const float* g, long n, int first, void* stream) {
    DBN_REQUIRE(acc && g && n > 0);
    hipLaunchKernelGGL(grad_accumulate_kernel, dim3(dbn_grid(n / 4 + 256)), dim3(256), 0, (hipStream_t)stream, acc, g, n, first);
    return dbn_status();
}

long dbn_grad_sqnorm_ws_doubles(long n) { return n <= 0 ? 0 : (n + SQ_CHUNK - 1) / SQ_CHUNK; }

int dbn_grad_sqnorm(const float* g, long n, double* partials, double* out, void* stream) {
    DBN_REQUIRE(g && partials && out && n > 0);
    const long nparts = dbn_grad_sqnorm_ws_doubles(n);
    DBN_REQUIRE(nparts <= 0x7fffffffL);
    hipLaunchKernelGGL(grad_sqnorm_part_kernel, dim3((unsigned)nparts), dim3(SQ_THREADS), 0, (hipStream_t)stream, g, n, partials);
    hipLaunchKernelGGL(grad_sqnorm_final_kernel, dim3(1), dim3(SQ_THREADS), 0, (hipStream_t)stream, partials, nparts, out);
    return dbn_status();
}

int dbn_adam_step_ex(float* p, const float* g, float* m, float* v, float* vmax, long n, float lr, float beta1, float beta2, float eps,
                     float weight_decay, int step, float grad_scale, const double* sqnorm, float max_norm, void* stream) {
    DBN_REQUIRE(p && g && m && v && n > 0 && step >= 1);
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    const AdamCoef c = {(float)(lr / bc1), beta1, beta2, eps, (float)(1.0 / sqrt(bc2)), weight_decay};
    const dim3 grid(dbn_grid(n / 4 + 256));
    if (vmax)
        hipLaunchKernelGGL(adam_ex_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, p, g, m, v, vmax, n, c, grad_scale, sqnorm, max_norm);
    else
        hipLaunchKernelGGL(adam_ex_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, p, g, m, v, vmax, n, c, grad_scale, sqnorm, max_norm);
    return dbn_status();
}

}  // extern "C"
