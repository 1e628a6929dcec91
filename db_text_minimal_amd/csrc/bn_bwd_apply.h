// The apply pass of the train-mode BatchNorm backward, shared by pointwise.hip (the gradient is a stored tensor) and
// head_loss.hip (the gradient of the DB head's 64-channel 320^2 ConvT outputs is formed again from the maps, never stored).
// One body serves both: it is templated on a GRADIENT SOURCE, so the item-to-thread mapping, the unrolled order, the rounding and
// the block reduction of the bias sums are the same code — and the results the same bits — whichever way the gradient arrives.
#pragma once
#include "common.h"

namespace {

// The streaming kernels run beside the matrix kernels of the step's other stream.  A small fixed footprint —
// 3 workgroups of 256 threads per CU, 12 of its 32 wave slots — leaves the MFMA kernels their residency, and UNROLL
// independent 16-byte loads per lane keep HBM busy without relying on occupancy (8 TB/s x ~1 us needs ~32 KB in flight per CU).
constexpr int STREAM_BLOCKS = 768;
constexpr int UNROLL = 4;

// grid of a streaming BN kernel whose threads keep their channel quad: (grid * 256) % (C/4) == 0
inline int bn_stream_grid(long total4, int C) {
    int g = dbn_grid(total4, 256, STREAM_BLOCKS);
    int a = C / 4, b = 256;
    while (b) { const int t = a % b; a = b; b = t; }  // a = gcd(C/4, 256)
    const int m = (C / 4) / a;                       // grid must be a multiple of m
    return (g + m - 1) / m * m;
}

// the value a store in the storage type leaves in memory (round to nearest even), as fp32
template <int AT>
__device__ __forceinline__ float round_to_storage(float v) {
    if constexpr (AT == 1) return (float)(__bf16)v;
    else if constexpr (AT == 2) return (float)(_Float16)v;
    else return v;
}

// Gradient source of bn_bwd_apply_body: fetch(i, raw) issues the loads of item i (the body calls it for i0, i0 + stride, ... in this
// order, once per item), grad(raw, g) turns them into the item's gradient.  This one reads the stored tensor `dout`.
template <int AT, int QW>
struct BnGradStored {
    const void* __restrict__ dout;
    struct Raw { f32x4 g[QW]; };
    __device__ __forceinline__ void fetch(long i, Raw& r) const {
        if constexpr (QW == 1) r.g[0] = dbn_ld4<AT>(dout, i);
        else dbn_ldq<AT>(dout, i, r.g);
    }
    __device__ __forceinline__ void grad(const Raw& r, f32x4 (&g)[QW]) const {
#pragma unroll
        for (int q = 0; q < QW; ++q) g[q] = r.g[q];
    }
};

// dy = gamma*rstd*(g - c1 - xhat*c2); optionally also emits g (the ReLU-masked dout).
// bias_part (optional, needs 256 % (C/4) == 0): per-block column sums of dy, [C][gridDim.x] — the gradient of the bias of the
// conv that feeds this BatchNorm (analytically zero; the reference's value is the round-off of exactly this sum), so that no
// separate pass re-reads dy for it.  The sum is over dy AS STORED (rounded to the storage type), which is what a dbn_col_sum_t
// pass over dy — and the convolution's own backward — reads.
// Uses blockIdx.x / gridDim.x only: a caller may run independent problems in the y dimension of its grid.
template <int AT, int QW, class SRC>
__device__ __forceinline__ void bn_bwd_apply_body(const void* __restrict__ y, const void* __restrict__ zmask, const float* __restrict__ msc,
                                                  const float* __restrict__ msh, SRC& src, const float* __restrict__ mean,
                                                  const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                  const float* __restrict__ c1, const float* __restrict__ c2, void* __restrict__ dy,
                                                  void* __restrict__ gout, int gout_acc, long total, int C, float* __restrict__ bias_part) {
    // an item = QW channel quads moved by one 16-byte access (QW = 2: 16-bit storage, C % 8 == 0; see bn_apply_kernel)
    static_assert(QW == 1 || (QW == 2 && AT != 0), "two quads per access: 16-bit storage");
    const int cin = C / (4 * QW);
    const long i0 = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    const int c = (int)(i0 % cin) * 4 * QW;  // constant per thread: the grid stride is a multiple of the items per pixel (host side)
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 s_[QW], h_[QW], mu[QW], rs[QW], k1[QW], k2[QW], gr[QW], bsum[QW];
#pragma unroll
    for (int q = 0; q < QW; ++q) {
        s_[q] = h_[q] = zero;
        if (msc) {
            s_[q] = *reinterpret_cast<const f32x4*>(msc + c + 4 * q);
            h_[q] = *reinterpret_cast<const f32x4*>(msh + c + 4 * q);
        }
        mu[q] = *reinterpret_cast<const f32x4*>(mean + c + 4 * q);
        rs[q] = *reinterpret_cast<const f32x4*>(rstd + c + 4 * q);
        k1[q] = *reinterpret_cast<const f32x4*>(c1 + c + 4 * q);
        k2[q] = *reinterpret_cast<const f32x4*>(c2 + c + 4 * q);
        gr[q] = *reinterpret_cast<const f32x4*>(gamma + c + 4 * q) * rs[q];
        bsum[q] = zero;
    }
    const bool acc = gout && gout_acc;
    auto ld = [&](const void* ptr, long i, f32x4 (&v)[QW]) {
        if constexpr (QW == 1) v[0] = dbn_ld4<AT>(ptr, i);
        else dbn_ldq<AT>(ptr, i, v);
    };
    auto st = [&](void* ptr, long i, const f32x4 (&v)[QW]) {
        if constexpr (QW == 1) dbn_st4<AT>(ptr, i, v[0]);
        else dbn_stq<AT>(ptr, i, v);
    };
    auto one = [&](long i, const typename SRC::Raw& raw, const f32x4 (&v)[QW], const f32x4 (&z)[QW], const f32x4 (&old)[QW]) {
        f32x4 g[QW], d[QW], go[QW];
        src.grad(raw, g);
#pragma unroll
        for (int q = 0; q < QW; ++q) {
            if (zmask) {
#pragma unroll
                for (int e = 0; e < 4; ++e) g[q][e] = z[q][e] > 0.f ? g[q][e] : 0.f;
            } else if (msc) {
#pragma unroll
                for (int e = 0; e < 4; ++e) g[q][e] = dbn_affine(v[q][e], s_[q][e], h_[q][e]) > 0.f ? g[q][e] : 0.f;
            }
            const f32x4 xh = (v[q] - mu[q]) * rs[q];
            d[q] = gr[q] * (g[q] - k1[q] - xh * k2[q]);
            // rounded to the storage type ONCE, here: the store below converts this value exactly, and the bias sum reads the same
            // bits.  The empty asm keeps the conversion apart from the product: fused with it (v_fma_mixlo_f16) the product is
            // rounded to fp16 once, while a second conversion of the same expression, left as v_cvt_pk_f16_f32, rounds the fp32
            // product again — the two then differ by one fp16 ulp in about one element of 2^13, and the sum no longer is that of dy.
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float t = d[q][e];
                asm("" : "+v"(t));
                d[q][e] = round_to_storage<AT>(t);
            }
            bsum[q] += d[q];
            go[q] = acc ? g[q] + old[q] : g[q];
        }
        st(dy, i, d);
        if (gout) st(gout, i, go);
    };
    auto zeros = [&](f32x4 (&v)[QW]) {
#pragma unroll
        for (int q = 0; q < QW; ++q) v[q] = zero;
    };
    long i = i0;
    for (; i + (UNROLL - 1) * stride < total; i += UNROLL * stride) {  // 2..4 x UNROLL independent loads in flight per lane
        typename SRC::Raw g[UNROLL];
        f32x4 v[UNROLL][QW], z[UNROLL][QW], o[UNROLL][QW];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            src.fetch(i + u * stride, g[u]);
            ld(y, i + u * stride, v[u]);
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            if (zmask) ld(zmask, i + u * stride, z[u]);
            else zeros(z[u]);
            if (acc) ld(gout, i + u * stride, o[u]);
            else zeros(o[u]);
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) one(i + u * stride, g[u], v[u], z[u], o[u]);
    }
    for (; i < total; i += stride) {
        typename SRC::Raw g;
        f32x4 v[QW], z[QW], o[QW];
        src.fetch(i, g);
        ld(y, i, v);
        if (zmask) ld(zmask, i, z);
        else zeros(z);
        if (acc) ld(gout, i, o);
        else zeros(o);
        one(i, g, v, z, o);
    }
    if (bias_part) {  // threads t, t + cin, t + 2 cin, ... of the block hold the same channels
        __shared__ f32x4 red[QW][256];
#pragma unroll
        for (int q = 0; q < QW; ++q) red[q][threadIdx.x] = bsum[q];
        __syncthreads();
        if ((int)threadIdx.x < cin) {
            const int cq = (int)((blockIdx.x * (long)blockDim.x + threadIdx.x) % cin) * 4 * QW;
#pragma unroll
            for (int q = 0; q < QW; ++q) {
                f32x4 t = zero;
                for (int k = threadIdx.x; k < 256; k += cin) t += red[q][k];
#pragma unroll
                for (int e = 0; e < 4; ++e) bias_part[(long)(cq + 4 * q + e) * gridDim.x + blockIdx.x] = t[e];
            }
        }
    }
}

}  // namespace
