// The optimizer family over the flat fp32 buffers (include/dbnet_hip.h "optimizer family"): SGD with momentum and
// AdamW, both with per-group learning rate and weight decay, norm clipping as in adam_ex_kernel (optim.hip) and an optional exponential
// moving average of the weights written by the thread that holds p'.  The kernels have the shape of adam_ex_kernel: an f32x4 body and a
// scalar tail over one element function, grid from dbn_grid, -ffp-contract=off (no fused multiply-add is formed).
//
// Groups.  flat_layout (engine.py) aligns every parameter to 4 floats, so a quad of the flat buffer never straddles two parameters and a
// parameter's padding belongs to it.  A group assignment is a list of runs, maximal stretches of consecutive quads of one group:
// run_end[r] (exclusive quad index, ascending) and run_group[r], uploaded once.  The per-group coefficients travel by value in the kernel
// arguments, so a schedule that changes them every step uploads nothing.  The GROUPED instantiations stage the table and the coefficients
// in LDS once per workgroup and find a quad's run by binary search; the others know one group and have no LDS and no search.
#include "common.h"

constexpr int OG_MAX_GROUPS = 8;
constexpr int OG_MAX_RUNS = 1024;
constexpr int OG_THREADS = 256;

// per-group coefficients by value.  a: SGD lr | AdamW lr / bc1;  wd: the L2 decay added to the gradient (0: none);
// pf: AdamW's decoupled factor fp32(1 - lr wd) on p (1: none)
struct GroupCoef {
    float a[OG_MAX_GROUPS], wd[OG_MAX_GROUPS], pf[OG_MAX_GROUPS];
};
struct OneCoef {
    float a, wd, pf;
};
struct RunTable {
    const int* end;
    const int* group;
    int n;
};
struct Ema {
    float* shadow;
    float d, omd;  // d and 1 - d, each rounded to fp32 once by the host
};

struct GroupLds {
    int end[OG_MAX_RUNS];
    unsigned char group[OG_MAX_RUNS];
    OneCoef coef[OG_MAX_GROUPS];
};

__device__ __forceinline__ void stage_groups(GroupLds& s, const RunTable& rt, const GroupCoef& gc) {
    for (int r = threadIdx.x; r < rt.n; r += OG_THREADS) {
        s.end[r] = rt.end[r];
        s.group[r] = (unsigned char)(rt.group[r] & (OG_MAX_GROUPS - 1));
    }
    if (threadIdx.x < OG_MAX_GROUPS) s.coef[threadIdx.x] = {gc.a[threadIdx.x], gc.wd[threadIdx.x], gc.pf[threadIdx.x]};
    __syncthreads();
}

// the coefficients of quad q: the first run whose end lies beyond q (a quad beyond the last end takes the last run)
__device__ __forceinline__ OneCoef coef_of_quad(const GroupLds& s, int nruns, long q) {
    int lo = 0, hi = nruns - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((long)s.end[mid] > q) hi = mid;
        else lo = mid + 1;
    }
    return s.coef[s.group[lo]];
}

// the clip coefficient of adam_ex_kernel, formula for formula: every thread forms it from the device value
__device__ __forceinline__ float clip_scale(float gscale, const double* __restrict__ sqnorm, float max_norm) {
    float gs = gscale;
    if (sqnorm) {
        const double norm = fabs((double)gscale) * sqrt(sqnorm[0]);
        const double q = (double)max_norm / (norm + 1e-6);
        gs = (float)((q > 1.0 ? 1.0 : q) * (double)gscale);  // (a NaN q stays NaN)
    }
    return gs;
}

__device__ __forceinline__ float ema_element(float shadow, float p, float d, float omd) { return d * shadow + omd * p; }

// ----------------------------------------------------------------------------------
// SGD.  MODE 0: no momentum (no buffer is read or written), 1: momentum, 2: nesterov
// ----------------------------------------------------------------------------------
struct SgdCoef {
    float mu, omd;  // momentum, fp32(1 - dampening)
    int first;      // the first update: buf' = g (torch clones the gradient: no dampening there)
};

template <int MODE>
__device__ __forceinline__ void sgd_element(float& p, float g, float& buf, float gs, const OneCoef& c, const SgdCoef& s) {
    float gg = g * gs;
    if (c.wd != 0.f) gg = gg + c.wd * p;
    float d = gg;
    if constexpr (MODE > 0) {
        buf = s.first ? gg : s.mu * buf + s.omd * gg;
        d = MODE == 2 ? gg + s.mu * buf : buf;
    }
    p = p - c.a * d;
}

template <int MODE, bool GROUPED, bool EMA>
__global__ __launch_bounds__(OG_THREADS) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, long n,
                                                         GroupCoef gc, RunTable rt, SgdCoef sc, float gscale,
                                                         const double* __restrict__ sqnorm, float max_norm, Ema ema) {
    OneCoef c = {gc.a[0], gc.wd[0], gc.pf[0]};
    GroupLds* lds = nullptr;
    if constexpr (GROUPED) {  // (the other instantiations declare no LDS)
        __shared__ GroupLds table;
        lds = &table;
        stage_groups(table, rt, gc);
    }
    const float gs = clip_scale(gscale, sqnorm, max_norm);
    const long n4 = n >> 2;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        if constexpr (GROUPED) c = coef_of_quad(*lds, rt.n, i);
        f32x4 pp = reinterpret_cast<f32x4*>(p)[i];
        const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
        f32x4 bb = {0.f, 0.f, 0.f, 0.f};
        if constexpr (MODE > 0)
            if (!sc.first) bb = reinterpret_cast<f32x4*>(buf)[i];
        f32x4 ss = {0.f, 0.f, 0.f, 0.f};
        if constexpr (EMA) ss = reinterpret_cast<f32x4*>(ema.shadow)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float pe = pp[e], be = bb[e];
            sgd_element<MODE>(pe, gg[e], be, gs, c, sc);
            pp[e] = pe, bb[e] = be;
            if constexpr (EMA) ss[e] = ema_element(ss[e], pe, ema.d, ema.omd);
        }
        reinterpret_cast<f32x4*>(p)[i] = pp;
        if constexpr (MODE > 0) reinterpret_cast<f32x4*>(buf)[i] = bb;
        if constexpr (EMA) reinterpret_cast<f32x4*>(ema.shadow)[i] = ss;
    }
    // tail: the elements past the last whole quad take the last run's group
    const long t = (n4 << 2) + blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (t < n) {
        if constexpr (GROUPED) c = lds->coef[lds->group[rt.n - 1]];
        float pp = p[t], bb = 0.f;
        if constexpr (MODE > 0)
            if (!sc.first) bb = buf[t];
        sgd_element<MODE>(pp, g[t], bb, gs, c, sc);
        p[t] = pp;
        if constexpr (MODE > 0) buf[t] = bb;
        if constexpr (EMA) ema.shadow[t] = ema_element(ema.shadow[t], pp, ema.d, ema.omd);
    }
}

// ----------------------------------------------------------------------------------
// AdamW: adam_element of optim.hip, operation for operation, with the group's lr / bc1 and decay.  Coupled (pf = 1): g + wd p after the
// clip, the sequence of adam_ex_kernel.  Decoupled (wd = 0): p pf first, then the update with the undecayed gradient.
// ----------------------------------------------------------------------------------
struct AdamWCoef {
    float b1, b2, eps, inv_sqrt_bc2;
};

template <bool AMS>
__device__ __forceinline__ void adamw_element(float& p, float g, float& m, float& v, float& vmax, float gs, const OneCoef& c,
                                              const AdamWCoef& k) {
    if (c.pf != 1.f) p = p * c.pf;
    float gg = g * gs;
    if (c.wd != 0.f) gg = gg + c.wd * p;
    m = k.b1 * m + (1.f - k.b1) * gg;
    v = k.b2 * v + (1.f - k.b2) * gg * gg;
    float root = v;
    if constexpr (AMS) {
        vmax = (v > vmax || v != v) ? v : vmax;  // torch.maximum: a NaN propagates
        root = vmax;
    }
    const float denom = sqrtf(root) * k.inv_sqrt_bc2 + k.eps;
    p -= c.a * (m / denom);
}

template <bool AMS, bool GROUPED, bool EMA>
__global__ __launch_bounds__(OG_THREADS) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, float* __restrict__ vmax, long n, GroupCoef gc, RunTable rt,
                                                           AdamWCoef k, float gscale, const double* __restrict__ sqnorm, float max_norm,
                                                           Ema ema) {
    OneCoef c = {gc.a[0], gc.wd[0], gc.pf[0]};
    GroupLds* lds = nullptr;
    if constexpr (GROUPED) {  // (the other instantiations declare no LDS)
        __shared__ GroupLds table;
        lds = &table;
        stage_groups(table, rt, gc);
    }
    const float gs = clip_scale(gscale, sqnorm, max_norm);
    const long n4 = n >> 2;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        if constexpr (GROUPED) c = coef_of_quad(*lds, rt.n, i);
        f32x4 pp = reinterpret_cast<f32x4*>(p)[i];
        const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
        f32x4 mm = reinterpret_cast<f32x4*>(m)[i];
        f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
        f32x4 vx = {0.f, 0.f, 0.f, 0.f};
        if constexpr (AMS) vx = reinterpret_cast<f32x4*>(vmax)[i];
        f32x4 ss = {0.f, 0.f, 0.f, 0.f};
        if constexpr (EMA) ss = reinterpret_cast<f32x4*>(ema.shadow)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {  // (a reference cannot bind to a vector element)
            float pe = pp[e], me = mm[e], ve = vv[e], xe = vx[e];
            adamw_element<AMS>(pe, gg[e], me, ve, xe, gs, c, k);
            pp[e] = pe, mm[e] = me, vv[e] = ve, vx[e] = xe;
            if constexpr (EMA) ss[e] = ema_element(ss[e], pe, ema.d, ema.omd);
        }
        reinterpret_cast<f32x4*>(p)[i] = pp;
        reinterpret_cast<f32x4*>(m)[i] = mm;
        reinterpret_cast<f32x4*>(v)[i] = vv;
        if constexpr (AMS) reinterpret_cast<f32x4*>(vmax)[i] = vx;
        if constexpr (EMA) reinterpret_cast<f32x4*>(ema.shadow)[i] = ss;
    }
    // tail: the elements past the last whole quad take the last run's group
    const long t = (n4 << 2) + blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (t < n) {
        if constexpr (GROUPED) c = lds->coef[lds->group[rt.n - 1]];
        float pp = p[t], mm = m[t], vv = v[t], vx = 0.f;
        if constexpr (AMS) vx = vmax[t];
        adamw_element<AMS>(pp, g[t], mm, vv, vx, gs, c, k);
        p[t] = pp;
        m[t] = mm;
        v[t] = vv;
        if constexpr (AMS) vmax[t] = vx;
        if constexpr (EMA) ema.shadow[t] = ema_element(ema.shadow[t], pp, ema.d, ema.omd);
    }
}

// GROUPED and EMA as compile-time constants of the launch
#define OG_DISPATCH(grouped, ema, ...)                                                 \
    do {                                                                               \
        if (grouped) {                                                                 \
            if (ema) { constexpr bool GROUPED = true, EMA = true; __VA_ARGS__; }       \
            else { constexpr bool GROUPED = true, EMA = false; __VA_ARGS__; }          \
        } else {                                                                       \
            if (ema) { constexpr bool GROUPED = false, EMA = true; __VA_ARGS__; }      \
            else { constexpr bool GROUPED = false, EMA = false; __VA_ARGS__; }         \
        }                                                                              \
    } while (0)

// the arguments every entry point of the family shares
static bool groups_ok(const float* lr, const float* wd, int ngroups, const int* run_end, const int* run_group, int nruns) {
    if (!lr || !wd || ngroups < 1 || ngroups > OG_MAX_GROUPS || nruns < 0 || nruns > OG_MAX_RUNS) return false;
    if (nruns == 0) return ngroups == 1;  // no table: one group
    return run_end && run_group;
}

extern "C" {

int dbn_optim_max_groups(void) { return OG_MAX_GROUPS; }
int dbn_optim_max_runs(void) { return OG_MAX_RUNS; }

int dbn_sgd_step(float* p, const float* g, float* buf, long n, const float* lr, const float* weight_decay, int ngroups, const int* run_end,
                 const int* run_group, int nruns, float momentum, float dampening, int nesterov, int first, float grad_scale,
                 const double* sqnorm, float max_norm, float* shadow, float ema_decay, float ema_one_minus, void* stream) {
    DBN_REQUIRE(p && g && n > 0 && groups_ok(lr, weight_decay, ngroups, run_end, run_group, nruns));
    DBN_REQUIRE(momentum == 0.f ? !nesterov : buf != nullptr);
    DBN_REQUIRE(!nesterov || dampening == 0.f);
    GroupCoef gc = {};
    for (int i = 0; i < ngroups; ++i) gc.a[i] = lr[i], gc.wd[i] = weight_decay[i], gc.pf[i] = 1.f;
    const RunTable rt = {run_end, run_group, nruns};
    const SgdCoef sc = {momentum, (float)(1.0 - (double)dampening), first ? 1 : 0};
    const Ema ema = {shadow, ema_decay, ema_one_minus};
    const dim3 grid(dbn_grid(n / 4 + 256)), block(OG_THREADS);
    const hipStream_t st = (hipStream_t)stream;
    const int mode = momentum == 0.f ? 0 : (nesterov ? 2 : 1);
    OG_DISPATCH(nruns > 0, shadow != nullptr, {
        if (mode == 0)
            hipLaunchKernelGGL((sgd_kernel<0, GROUPED, EMA>), grid, block, 0, st, p, g, buf, n, gc, rt, sc, grad_scale, sqnorm, max_norm, ema);
        else if (mode == 1)
            hipLaunchKernelGGL((sgd_kernel<1, GROUPED, EMA>), grid, block, 0, st, p, g, buf, n, gc, rt, sc, grad_scale, sqnorm, max_norm, ema);
        else
            hipLaunchKernelGGL((sgd_kernel<2, GROUPED, EMA>), grid, block, 0, st, p, g, buf, n, gc, rt, sc, grad_scale, sqnorm, max_norm, ema);
    });
    return dbn_status();
}

int dbn_adamw_step(float* p, const float* g, float* m, float* v, float* vmax, long n, const float* lr, const float* weight_decay, int ngroups,
                   const int* run_end, const int* run_group, int nruns, float beta1, float beta2, float eps, int decoupled, int step,
                   float grad_scale, const double* sqnorm, float max_norm, float* shadow, float ema_decay, float ema_one_minus,
                   void* stream) {
    DBN_REQUIRE(p && g && m && v && n > 0 && step >= 1 && groups_ok(lr, weight_decay, ngroups, run_end, run_group, nruns));
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    GroupCoef gc = {};
    for (int i = 0; i < ngroups; ++i) {
        gc.a[i] = (float)(lr[i] / bc1);
        gc.wd[i] = decoupled ? 0.f : weight_decay[i];
        gc.pf[i] = decoupled ? (float)(1.0 - (double)lr[i] * (double)weight_decay[i]) : 1.f;
    }
    const RunTable rt = {run_end, run_group, nruns};
    const AdamWCoef k = {beta1, beta2, eps, (float)(1.0 / sqrt(bc2))};
    const Ema ema = {shadow, ema_decay, ema_one_minus};
    const dim3 grid(dbn_grid(n / 4 + 256)), block(OG_THREADS);
    const hipStream_t st = (hipStream_t)stream;
    OG_DISPATCH(nruns > 0, shadow != nullptr, {
        if (vmax)
            hipLaunchKernelGGL((adamw_kernel<true, GROUPED, EMA>), grid, block, 0, st, p, g, m, v, vmax, n, gc, rt, k, grad_scale, sqnorm,
                               max_norm, ema);
        else
            hipLaunchKernelGGL((adamw_kernel<false, GROUPED, EMA>), grid, block, 0, st, p, g, m, v, vmax, n, gc, rt, k, grad_scale, sqnorm,
                               max_norm, ema);
    });
    return dbn_status();
}

}  // extern "C"
