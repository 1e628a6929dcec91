// Shared device/host helpers for the DBNet gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The public C ABI: every unit sees the declarations, so a definition that disagrees with the header does not compile.
#include "../../include/dbnet_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#include <stdlib.h>

// Build flavour.  The default library carries the product kernels only.  -DDBN_EXPERIMENTS adds the variants that were
// measured and rejected (kept for the record, each with its own test): pre-split bf16 planes (AT = 3, dbn_split3), the
// LDS-DMA fp32 weight gradient (wgrad_dma_kernel), and the environment overrides of the tile / split heuristics.
#ifdef DBN_EXPERIMENTS
#define DBN_HAS_EXPERIMENTS 1
static inline int dbn_env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
static inline double dbn_env_double(const char* name, double dflt) { const char* e = getenv(name); return e ? atof(e) : dflt; }
#else
#define DBN_HAS_EXPERIMENTS 0
static inline constexpr int dbn_env_int(const char*, int dflt) { return dflt; }
static inline constexpr double dbn_env_double(const char*, double dflt) { return dflt; }
#endif

// -DDBN_RACE=1 (make RACE=1 -> ../libdbnet_hip_race.so; never the product library): every workgroup barrier — __syncthreads()
// and the raw s_barrier of the LDS-DMA rings — and every cross-workgroup counter increment (DBN_RACE_JITTER) is preceded AND
// followed by a delay of 0..7 x 512 cycles hashed from (wave, workgroup, source line).  Correct kernels return the same bits as the
// product build; a missing barrier, a counted wait that is one short, or a hand-over that relies on arrival order turns from a
// once-per-thousand transient into a wrong result on (nearly) every launch.  tools/probes/repro.hip and the -m gpu suite run
// against this library through DBN_LIB_PATH (profiles/r04_repro.md).
#ifndef DBN_RACE
#define DBN_RACE 0
#endif
#if DBN_RACE
__device__ __forceinline__ void dbn_race_jitter(unsigned site) {
    unsigned h = (threadIdx.x >> 6) * 2654435761u + blockIdx.x * 40503u + site * 2246822519u;
    h ^= h >> 15;
    h *= 2654435761u;
    h ^= h >> 13;
    const unsigned n = __builtin_amdgcn_readfirstlane(h & 7u);
    for (unsigned i = 0; i < n; ++i) __builtin_amdgcn_s_sleep(8);
}
__device__ __forceinline__ void dbn_race_raw_barrier(unsigned site) {
    dbn_race_jitter(site);
    __builtin_amdgcn_s_barrier();
    dbn_race_jitter(site + 7919u);
}
#define __syncthreads() (dbn_race_jitter(__LINE__), (__syncthreads)(), dbn_race_jitter(__LINE__ + 7919u))
#define __builtin_amdgcn_s_barrier() dbn_race_raw_barrier(__LINE__)
#define DBN_RACE_JITTER() dbn_race_jitter(__LINE__ + 104729u)
#else
#define DBN_RACE_JITTER() ((void)0)
#endif

#define DBN_OK 0
#define DBN_ERR_ARG 1

#define DBN_REQUIRE(cond) \
    do {                  \
        if (!(cond)) return DBN_ERR_ARG; \
    } while (0)

static inline int dbn_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? DBN_OK : 1000 + (int)e;
}

static inline int dbn_ceil_div(long a, long b) { return (int)((a + b - 1) / b); }

// Grid for a grid-stride pointwise kernel: enough blocks to fill 256 CUs x 8, capped.
static inline int dbn_grid(long work_items, int block = 256, int cap = 4096) {
    long g = (work_items + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

// MI355X: 8 XCDs, block b runs on XCD b % 8 (observed; used for L2 locality only).
// Bijective remap that gives each XCD a contiguous run of tiles.
__device__ __forceinline__ int dbn_xcd_remap(int bid, int nblk) {
    const int q = nblk >> 3, r = nblk & 7;
    const int xcd = bid & 7, idx = bid >> 3;
    const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + idx;
}

__device__ __forceinline__ float dbn_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ double dbn_wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Partial sums are stored transposed, part[idx*nb + b] (b = producing block), so that the 32 lanes
// folding one output read one contiguous 128-byte line per step.  Call with all 32 lanes of an
// aligned half-wave (lane32 = threadIdx.x & 31); every lane returns the total (fp64 fold).
__device__ __forceinline__ double dbn_team32_fold(const float* __restrict__ part, int nb, long idx, int lane32) {
    const float* row = part + idx * nb;
    double s = 0.0;
    int b = lane32;
    for (; b + 96 < nb; b += 128) {  // four independent loads in flight per lane
        const float v0 = row[b], v1 = row[b + 32], v2 = row[b + 64], v3 = row[b + 96];
        s += ((double)v0 + (double)v1) + ((double)v2 + (double)v3);
    }
    for (; b < nb; b += 32) s += (double)row[b];
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

// BatchNorm affine + optional ReLU written once so that every kernel that
// recomputes an activation gets bit-identical values (maxpool backward relies
// on float equality with the forward).
__device__ __forceinline__ float dbn_affine(float y, float sc, float sh) { return fmaf(y, sc, sh); }
__device__ __forceinline__ float dbn_affine_relu(float y, float sc, float sh) { return fmaxf(fmaf(y, sc, sh), 0.f); }

// ---- activation storage types ---------------------------------------------------------------------------------------
// AT = 0: fp32 (BASELINE configs[1]), 1: bf16 (configs[2]/[3]: bf16 activations, gradients and weight panels in HBM; fp32
// accumulators, BatchNorm statistics, loss sums, master weights), 2: fp16 (configs[4]: inference).  Every kernel computes
// in fp32 registers; only what crosses HBM changes.  Helpers move FOUR consecutive elements (16 B fp32 / 8 B 16-bit).
// (DBN_AT_F32 / DBN_AT_BF16 / DBN_AT_F16: include/dbnet_hip.h)
typedef unsigned dbn_u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 dbn_f16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 dbn_bf16x2 __attribute__((ext_vector_type(2)));

__host__ __device__ constexpr int dbn_esize(int at) { return at == 0 ? 4 : 2; }

template <int AT>
__device__ __forceinline__ f32x4 dbn_ld4(const void* __restrict__ p, long i4) {
    if constexpr (AT == 0) {
        return reinterpret_cast<const f32x4*>(p)[i4];
    } else if constexpr (AT == 1) {
        const dbn_u32x2 v = reinterpret_cast<const dbn_u32x2*>(p)[i4];
        return f32x4{__builtin_bit_cast(float, v[0] << 16), __builtin_bit_cast(float, v[0] & 0xFFFF0000u),
                     __builtin_bit_cast(float, v[1] << 16), __builtin_bit_cast(float, v[1] & 0xFFFF0000u)};
    } else {
        const dbn_f16x4 v = reinterpret_cast<const dbn_f16x4*>(p)[i4];
        return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
    }
}

// Q consecutive channel quads per item with ONE 16-byte access: Q = 1 for fp32 (dbn_ld4), Q = 2 for the 16-bit types (eight elements:
// the 8-byte accesses of dbn_ld4<1|2> reach 0.54-0.70x the rate of 16-byte ones, MI355X_MICROARCH.md; round 5)
template <int AT>
struct dbn_quads { static constexpr int Q = AT == 0 ? 1 : 2; };
template <int AT>
__device__ __forceinline__ void dbn_ldq(const void* __restrict__ p, long i, f32x4 (&v)[dbn_quads<AT>::Q]) {
    if constexpr (AT == 0) {
        v[0] = reinterpret_cast<const f32x4*>(p)[i];
    } else if constexpr (AT == 1) {
        typedef unsigned dbn_u32x4_ __attribute__((ext_vector_type(4)));
        const dbn_u32x4_ w = reinterpret_cast<const dbn_u32x4_*>(p)[i];
#pragma unroll
        for (int q = 0; q < 2; ++q)
            v[q] = f32x4{__builtin_bit_cast(float, w[2 * q] << 16), __builtin_bit_cast(float, w[2 * q] & 0xFFFF0000u),
                         __builtin_bit_cast(float, w[2 * q + 1] << 16), __builtin_bit_cast(float, w[2 * q + 1] & 0xFFFF0000u)};
    } else {
        typedef _Float16 dbn_f16x8_ __attribute__((ext_vector_type(8)));
        const dbn_f16x8_ w = reinterpret_cast<const dbn_f16x8_*>(p)[i];
#pragma unroll
        for (int q = 0; q < 2; ++q) v[q] = f32x4{(float)w[4 * q], (float)w[4 * q + 1], (float)w[4 * q + 2], (float)w[4 * q + 3]};
    }
}
template <int AT>
__device__ __forceinline__ void dbn_st4(void* __restrict__ p, long i4, f32x4 v) {
    if constexpr (AT == 0) {
        reinterpret_cast<f32x4*>(p)[i4] = v;
    } else if constexpr (AT == 1) {  // v_cvt_pk_bf16_f32: round to nearest even
        const dbn_bf16x2 lo = {(__bf16)v[0], (__bf16)v[1]}, hi = {(__bf16)v[2], (__bf16)v[3]};
        reinterpret_cast<dbn_u32x2*>(p)[i4] = dbn_u32x2{__builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi)};
    } else {
        reinterpret_cast<dbn_f16x4*>(p)[i4] = dbn_f16x4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
    }
}
template <int AT>
__device__ __forceinline__ void dbn_stq(void* __restrict__ p, long i, const f32x4 (&v)[dbn_quads<AT>::Q]) {
    if constexpr (AT == 0) {
        reinterpret_cast<f32x4*>(p)[i] = v[0];
    } else if constexpr (AT == 1) {
        typedef unsigned dbn_u32x4_ __attribute__((ext_vector_type(4)));
        dbn_u32x4_ w;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const dbn_bf16x2 lo = {(__bf16)v[q][0], (__bf16)v[q][1]}, hi = {(__bf16)v[q][2], (__bf16)v[q][3]};
            w[2 * q] = __builtin_bit_cast(unsigned, lo);
            w[2 * q + 1] = __builtin_bit_cast(unsigned, hi);
        }
        reinterpret_cast<dbn_u32x4_*>(p)[i] = w;
    } else {
        typedef _Float16 dbn_f16x8_ __attribute__((ext_vector_type(8)));
        dbn_f16x8_ w;
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) w[4 * q + e] = (_Float16)v[q][e];
        reinterpret_cast<dbn_f16x8_*>(p)[i] = w;
    }
}

// one element
template <int AT>
__device__ __forceinline__ float dbn_ld1(const void* __restrict__ p, long i) {
    if constexpr (AT == 0) return reinterpret_cast<const float*>(p)[i];
    else if constexpr (AT == 1) return __builtin_bit_cast(float, (unsigned)reinterpret_cast<const unsigned short*>(p)[i] << 16);
    else return (float)reinterpret_cast<const _Float16*>(p)[i];
}
template <int AT>
__device__ __forceinline__ void dbn_st1(void* __restrict__ p, long i, float v) {
    if constexpr (AT == 0) reinterpret_cast<float*>(p)[i] = v;
    else if constexpr (AT == 1) reinterpret_cast<__bf16*>(p)[i] = (__bf16)v;
    else reinterpret_cast<_Float16*>(p)[i] = (_Float16)v;
}

// run `stmt` with a constexpr AT for a runtime activation type
#define DBN_DISPATCH_AT(at, ...)                          \
    do {                                                  \
        if ((at) == 0) { constexpr int AT = 0; __VA_ARGS__; }      \
        else if ((at) == 1) { constexpr int AT = 1; __VA_ARGS__; } \
        else if ((at) == 2) { constexpr int AT = 2; __VA_ARGS__; } \
        else return DBN_ERR_ARG;                          \
    } while (0)
