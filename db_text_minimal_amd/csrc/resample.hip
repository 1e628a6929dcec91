// The geometric stage of the reference's loader on the device (data_loaders.py:60-84, db_transforms.py:85-200,
// utils.py:160-199), uint8 HWC images in, one launch per stage per batch, three stages:
//   warp_affine_u8         imgaug Fliplr + Affine(rotate): cv2.warpAffine INTER_LINEAR, BORDER_CONSTANT 0, output the size
//                          of the input, with the flip folded into the source column
//   resize_cubic_u8        imgaug Resize (cubic): cv2.resize INTER_CUBIC, only the rows and columns of a window of the
//                          resized image (the crop of db_transforms.crop); every output pixel of a resize is independent,
//                          so the window is exact
//   resize_linear_norm_u8  db_transforms.resize / utils.test_resize: cv2.resize INTER_LINEAR into the top-left corner of
//                          a CH x CW canvas, fused with the normalisation of data_loaders.py:161-167: fp32 [N][3][CH][CW],
//                          every pixel written once, the padding as 0 - mean[c] (the reference pads in uint8)
// and, for the inference path, the word crops of test_ocr.py:160-177 (one launch per batch of boxes):
//   warp_perspective_u8    cv2.warpPerspective INTER_LINEAR, BORDER_CONSTANT 0 of K quads into K out_h x out_w crops, with
//                          dbn_perspective_maps (host) restating cv2.getPerspectiveTransform and the 3 x 3 invert
// The arithmetic restates OpenCV 4.2's scalar 8-bit paths (imgwarp.cpp WarpAffineInvoker / WarpPerspectiveInvoker +
// remapBilinear, resize.cpp resize / HResize* / VResize*).  PARITY UNPINNED against cv2 itself (not available to test
// against): OpenCV's SIMD row loops (the cubic vertical pass converts to float) and IPP can round some pixels differently
// (DESIGN sections 19 and 20).
//
// Each workgroup of the first three owns a 64 x 16 tile of one image's output.  Its column and row tables (source index and fixed-point
// weights) are computed once per tile column / row into LDS; pixels then use integer arithmetic only.  The float and
// double coefficient formulas must not be contracted into FMAs (the Makefile builds with -ffp-contract=off).
#include <math.h>

#include <utility>

#include "common.h"

namespace {

constexpr int RS_TW = 64, RS_TH = 16, RS_THREADS = 256, RS_RPT = RS_TH / (RS_THREADS / RS_TW);
constexpr int RS_DESC = 12;  // int64 per image, see include/dbnet_hip.h
constexpr int RS_COEF = 6;   // doubles per image

struct Desc {
    long long src_off, sh, sw, dst_off, dh, dw, oy, ox, oh, ow, flip;
};

__device__ __forceinline__ Desc load_desc(const long long* d) {
    return {d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10]};
}

// the descriptor's source and destination stay inside the buffers, and the window inside the resized image; a
// descriptor that breaks this is skipped (the Python layer builds them and checks the same before the launch)
__device__ __forceinline__ bool desc_ok(const Desc& d, long src_bytes, long dst_elems, long dst_per_px) {
    if (d.sh <= 0 || d.sw <= 0 || d.dh <= 0 || d.dw <= 0 || d.oh <= 0 || d.ow <= 0) return false;
    if (d.sh > 65535 || d.sw > 65535 || d.dh > 65535 || d.dw > 65535) return false;
    if (d.oy < 0 || d.ox < 0 || d.oy + d.oh > d.dh || d.ox + d.ow > d.dw) return false;
    if (d.src_off < 0 || d.src_off + d.sh * d.sw * 3 > src_bytes) return false;
    if (d.dst_off < 0 || d.dst_off + d.oh * d.ow * dst_per_px > dst_elems) return false;
    return true;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// saturate_cast<short>(float): cvRound (round half to even), then clamped
__device__ __forceinline__ int sat_short(float v) { return clampi(__float2int_rn(v), -32768, 32767); }
// saturate_cast<int>(double): cvRound
__device__ __forceinline__ int sat_int(double v) {
    return v >= 2147483647.0 ? 2147483647 : (v <= -2147483648.0 ? (-2147483647 - 1) : __double2int_rn(v));
}

// resize.cpp: fx = (float)((dx + 0.5) * scale - 0.5), sx = cvFloor(fx), fx -= sx
__device__ __forceinline__ float resize_src(int d, double scale, int* s) {
    const float f = (float)(((double)d + 0.5) * scale - 0.5);
    const int i = (int)floorf(f);
    *s = i;
    return f - (float)i;
}

// interpolateCubic, A = -0.75, in float
__device__ __forceinline__ void cubic_coeffs(float x, int* c) {
    const float A = -0.75f;
    float k0 = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
    float k1 = ((A + 2) * x - (A + 3)) * x * x + 1;
    float k2 = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
    float k3 = 1.f - k0 - k1 - k2;
    c[0] = sat_short(k0 * 2048);  // INTER_RESIZE_COEF_SCALE
    c[1] = sat_short(k1 * 2048);
    c[2] = sat_short(k2 * 2048);
    c[3] = sat_short(k3 * 2048);
}

// remapBilinear for CV_8U, 3 channels, BORDER_CONSTANT 0, at the fixed-point source position (X, Y) in 1/32 pixels: source
// column saturate_cast<short>(X >> 5), weight index X & 31 (Y likewise).  The bilinear table holds products of 1/32 steps
// scaled to 32768 (exact), except at (0, 0) where 32768 saturates to 32767 and initInterTab2D's sum correction puts the
// missing 1 on the (1, 1) tap.  Out-of-image taps read the border value 0; v = saturate_cast<uchar>((sum w*v + 2^14) >> 15).
// flip reads column W-1-x for x (the warp of a flipped image).
__device__ __forceinline__ void bilinear_u8(const unsigned char* S, int H, int W, int flip, int X, int Y, int* v) {
    const int sx = clampi(X >> 5, -32768, 32767), sy = clampi(Y >> 5, -32768, 32767);  // saturate_cast<short>
    const int fx = X & 31, fy = Y & 31;
    int w[4] = {(32 - fy) * (32 - fx) * 32, (32 - fy) * fx * 32, fy * (32 - fx) * 32, fy * fx * 32};
    if (fx == 0 && fy == 0) w[0] = 32767, w[3] = 1;
    int acc[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int yy = sy + (k >> 1), xx = sx + (k & 1);
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
        const unsigned char* p = S + ((long)yy * W + (flip ? W - 1 - xx : xx)) * 3;
        acc[0] += p[0] * w[k];
        acc[1] += p[1] * w[k];
        acc[2] += p[2] * w[k];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = clampi((acc[c] + (1 << 14)) >> 15, 0, 255);
}

// ---- warp: cv2.warpAffine(flags=INTER_LINEAR, BORDER_CONSTANT, 0) of the flipped image --------------------------------
// coef = the inverse map M[6] (warpAffine inverts the forward matrix in double).  AB_BITS = 10, INTER_BITS = 5:
// X = (saturate_cast<int>((M1*y + M2)*1024) + 16 + saturate_cast<int>(M0*x*1024)) >> 5 (Y likewise), then bilinear_u8.
__global__ void __launch_bounds__(RS_THREADS) warp_affine_u8_kernel(const unsigned char* __restrict__ src, long src_bytes,
                                                                     const long long* __restrict__ desc, const double* __restrict__ coef,
                                                                     unsigned char* __restrict__ dst, long dst_bytes) {
    __shared__ int s_ad[RS_TW], s_bd[RS_TW], s_x0[RS_TH], s_y0[RS_TH];
    const int n = blockIdx.z;
    const Desc d = load_desc(desc + (long)n * RS_DESC);
    if (!desc_ok(d, src_bytes, dst_bytes, 3) || d.oh != d.sh || d.ow != d.sw) return;
    const int tx0 = blockIdx.x * RS_TW, ty0 = blockIdx.y * RS_TH;
    if (tx0 >= d.ow || ty0 >= d.oh) return;
    const double* M = coef + (long)n * RS_COEF;
    const int t = threadIdx.x;
    if (t < RS_TW) {
        const int x = tx0 + t;
        s_ad[t] = sat_int(M[0] * x * 1024);
        s_bd[t] = sat_int(M[3] * x * 1024);
    } else if (t < RS_TW + RS_TH) {
        const int y = ty0 + t - RS_TW;
        s_x0[t - RS_TW] = sat_int((M[1] * y + M[2]) * 1024) + 16;
        s_y0[t - RS_TW] = sat_int((M[4] * y + M[5]) * 1024) + 16;
    }
    __syncthreads();
    const int lx = t % RS_TW, x = tx0 + lx;
    if (x >= d.ow) return;
    const int H = (int)d.sh, W = (int)d.sw;
    const unsigned char* S = src + d.src_off;
    for (int r = 0; r < RS_RPT; ++r) {
        const int ly = t / RS_TW + r * (RS_THREADS / RS_TW), y = ty0 + ly;
        if (y >= d.oh) break;
        const int X = (s_x0[ly] + s_ad[lx]) >> 5, Y = (s_y0[ly] + s_bd[lx]) >> 5;
        int v[3];
        bilinear_u8(S, H, W, (int)d.flip, X, Y, v);
        unsigned char* o = dst + d.dst_off + ((long)y * d.ow + x) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = (unsigned char)v[c];
    }
}

// ---- cubic resize of the warped image to dh x dw, window rows oy .. oy+oh-1, columns ox .. ox+ow-1 ---------------------
// coef[0] / coef[1] = scale_x / scale_y = 1 / ((double)dw / sw) as resize computes them.  Taps s-1 .. s+2 clamped to the
// image on both axes (HResizeCubic's border loop, resizeGeneric's clip of rows); horizontal sums in int, then
// D = saturate_cast<uchar>((sum_k h_k * beta_k + 2^21) >> 22) (VResizeCubic + FixedPtCast<int, uchar, 22>).
__global__ void __launch_bounds__(RS_THREADS) resize_cubic_u8_kernel(const unsigned char* __restrict__ src, long src_bytes,
                                                                      const long long* __restrict__ desc, const double* __restrict__ coef,
                                                                      unsigned char* __restrict__ dst, long dst_bytes) {
    __shared__ int s_cx[RS_TW][4], s_ca[RS_TW][4], s_ry[RS_TH][4], s_rb[RS_TH][4];
    const int n = blockIdx.z;
    const Desc d = load_desc(desc + (long)n * RS_DESC);
    if (!desc_ok(d, src_bytes, dst_bytes, 3)) return;
    const int tx0 = blockIdx.x * RS_TW, ty0 = blockIdx.y * RS_TH;
    if (tx0 >= d.ow || ty0 >= d.oh) return;
    const int H = (int)d.sh, W = (int)d.sw;
    const int t = threadIdx.x;
    if (t < RS_TW) {
        int s;
        const float f = resize_src((int)d.ox + tx0 + t, coef[(long)n * RS_COEF], &s);
        cubic_coeffs(f, s_ca[t]);
        for (int k = 0; k < 4; ++k) s_cx[t][k] = clampi(s - 1 + k, 0, W - 1);
    } else if (t < RS_TW + RS_TH) {
        const int r = t - RS_TW;
        int s;
        const float f = resize_src((int)d.oy + ty0 + r, coef[(long)n * RS_COEF + 1], &s);
        cubic_coeffs(f, s_rb[r]);
        for (int k = 0; k < 4; ++k) s_ry[r][k] = clampi(s - 1 + k, 0, H - 1);
    }
    __syncthreads();
    const int lx = t % RS_TW, x = tx0 + lx;
    if (x >= d.ow) return;
    const unsigned char* S = src + d.src_off;
    const int c0 = s_cx[lx][0] * 3, c1 = s_cx[lx][1] * 3, c2 = s_cx[lx][2] * 3, c3 = s_cx[lx][3] * 3;
    const int a0 = s_ca[lx][0], a1 = s_ca[lx][1], a2 = s_ca[lx][2], a3 = s_ca[lx][3];
    for (int r = 0; r < RS_RPT; ++r) {
        const int ly = t / RS_TW + r * (RS_THREADS / RS_TW), y = ty0 + ly;
        if (y >= d.oh) break;
        int acc[3] = {0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned char* row = S + (long)s_ry[ly][k] * W * 3;
            const int b = s_rb[ly][k];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int h = row[c0 + c] * a0 + row[c1 + c] * a1 + row[c2 + c] * a2 + row[c3 + c] * a3;
                acc[c] += h * b;
            }
        }
        unsigned char* o = dst + d.dst_off + ((long)y * d.ow + x) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = (unsigned char)clampi((acc[c] + (1 << 21)) >> 22, 0, 255);
    }
}

// ---- linear resize to dh x dw into a CH x CW canvas, normalised, fp32 NCHW ------------------------------------------
// coef[0] / coef[1] = scale_x / scale_y.  Columns: a source index below 0 or at / past the last column is reset to the
// edge with fx = 0 (resize's table loop); rows keep their fraction and clamp both taps (resizeGeneric's clip).  Weights
// saturate_cast<short>((1 - f) * 2048), saturate_cast<short>(f * 2048); horizontal sums in int; the 8-bit vertical pass
// of VResizeLinear<uchar, int, short, ...>: uchar((((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2).
// out = (float)u8 - m_c inside the dh x dw corner, -m_c elsewhere.  desc: oy = ox = 0, oh = dh, ow = dw, dst_off = 0 (image n
// goes to out[n]); the canvas CH x CW holds the dh x dw corner.
__global__ void __launch_bounds__(RS_THREADS) resize_linear_norm_u8_kernel(const unsigned char* __restrict__ src, long src_bytes,
                                                                            const long long* __restrict__ desc,
                                                                            const double* __restrict__ coef, int CH, int CW, float m0,
                                                                            float m1, float m2, float* __restrict__ out) {
    __shared__ int s_cx[RS_TW][2], s_ca[RS_TW][2], s_ry[RS_TH][2], s_rb[RS_TH][2];
    const int n = blockIdx.z;
    const long plane = (long)CH * CW;
    const Desc d = load_desc(desc + (long)n * RS_DESC);
    if (!desc_ok(d, src_bytes, plane, 1) || d.oy != 0 || d.ox != 0 || d.oh != d.dh || d.ow != d.dw || d.dh > CH || d.dw > CW ||
        d.dst_off != 0)
        return;
    const int tx0 = blockIdx.x * RS_TW, ty0 = blockIdx.y * RS_TH;
    const int H = (int)d.sh, W = (int)d.sw;
    const int t = threadIdx.x;
    if (t < RS_TW) {
        int s;
        float f = resize_src(tx0 + t, coef[(long)n * RS_COEF], &s);
        if (s < 0) f = 0, s = 0;
        if (s >= W - 1) f = 0, s = W - 1;
        s_cx[t][0] = s * 3;
        s_cx[t][1] = min(s + 1, W - 1) * 3;  // weight 0 where clamped
        s_ca[t][0] = sat_short((1.f - f) * 2048);
        s_ca[t][1] = sat_short(f * 2048);
    } else if (t < RS_TW + RS_TH) {
        const int r = t - RS_TW;
        int s;
        const float f = resize_src(ty0 + r, coef[(long)n * RS_COEF + 1], &s);
        s_ry[r][0] = clampi(s, 0, H - 1);
        s_ry[r][1] = clampi(s + 1, 0, H - 1);
        s_rb[r][0] = sat_short((1.f - f) * 2048);
        s_rb[r][1] = sat_short(f * 2048);
    }
    __syncthreads();
    const int lx = t % RS_TW, x = tx0 + lx;
    if (x >= CW) return;
    const unsigned char* S = src + d.src_off;
    float* o = out + (long)n * 3 * plane;
    const int c0 = s_cx[lx][0], c1 = s_cx[lx][1], a0 = s_ca[lx][0], a1 = s_ca[lx][1];
    for (int r = 0; r < RS_RPT; ++r) {
        const int ly = t / RS_TW + r * (RS_THREADS / RS_TW), y = ty0 + ly;
        if (y >= CH) break;
        const long p = (long)y * CW + x;
        if (y >= d.dh || x >= d.dw) {
            o[p] = 0.f - m0;
            o[plane + p] = 0.f - m1;
            o[2 * plane + p] = 0.f - m2;
            continue;
        }
        const unsigned char* r0 = S + (long)s_ry[ly][0] * W * 3;
        const unsigned char* r1 = S + (long)s_ry[ly][1] * W * 3;
        const int b0 = s_rb[ly][0], b1 = s_rb[ly][1];
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int h0 = r0[c0 + c] * a0 + r0[c1 + c] * a1;
            const int h1 = r1[c0 + c] * a0 + r1[c1 + c] * a1;
            const unsigned char u = (unsigned char)((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2);
            v[c] = (float)u;
        }
        o[p] = v[0] - m0;
        o[plane + p] = v[1] - m1;
        o[2 * plane + p] = v[2] - m2;
    }
}


// ---- word crops: cv2.warpPerspective(flags=INTER_LINEAR, BORDER_CONSTANT, 0) of K quads into K out_h x out_w crops ---------
// desc[k][3] int64 = {byte offset of crop k's source image in src, its height, its width}; inv[k][9] = the inverse map of
// crop k (row-major, as warpPerspective inverts the forward matrix).  WarpPerspectiveInvoker works in blocks of bw0
// columns (bw0 from the output size, see dbn_warp_perspective_u8) and computes, for the block origin xb and row y,
// X0 = M0*xb + M1*y + M2, Y0 = M3*xb + M4*y + M5, W0 = M6*xb + M7*y + M8, then per pixel at x1 = x - xb:
// W = W0 + M6*x1, W = W ? 32/W : 0, fX = max(INT_MIN, min(INT_MAX, (X0 + M0*x1)*W)) (std::min / std::max: NaN -> INT_MAX),
// X = cvRound(fX) (Y likewise), then bilinear_u8.  IEEE double throughout (no contraction, a true division).
// The output of the batch is one run of K*out_h*out_w pixels, and each workgroup owns WP_PX consecutive ones (they may span
// crops): it samples them into LDS and stores the run's bytes as dwords.  A crop whose descriptor leaves src_bytes or whose
// sides leave 1 .. 65535 is written as zeros (the Python layer checks the same before the launch).
constexpr int WP_THREADS = 256, WP_PPT = 4, WP_PX = WP_THREADS * WP_PPT, WP_DESC = 3;

__device__ __forceinline__ double clamp_int_range(double v) {
    const double m = v < 2147483647.0 ? v : 2147483647.0;  // std::min((double)INT_MAX, v)
    return -2147483648.0 < m ? m : -2147483648.0;         // std::max((double)INT_MIN, m)
}

__global__ void __launch_bounds__(WP_THREADS) warp_perspective_u8_kernel(const unsigned char* __restrict__ src, long src_bytes,
                                                                          const long long* __restrict__ desc,
                                                                          const double* __restrict__ inv, long n_px, int hw, int ow,
                                                                          int bw0, unsigned char* __restrict__ dst) {
    __shared__ unsigned int s_out[WP_PX * 3 / 4];
    unsigned char* sb = reinterpret_cast<unsigned char*>(s_out);
    const int t = threadIdx.x;
    const long p0 = (long)blockIdx.x * WP_PX;
    const long k0 = p0 / hw;
    const int q0 = (int)(p0 - k0 * hw);  // < hw, and hw + WP_PX fits an int (checked at the launch)
#pragma unroll
    for (int i = 0; i < WP_PPT; ++i) {
        const int lp = i * WP_THREADS + t;
        int v[3] = {0, 0, 0};
        if (p0 + lp < n_px) {
            const int q = q0 + lp;
            const long k = k0 + q / hw;
            const int r = q % hw, y = r / ow, x = r - y * ow;
            const long long* dk = desc + k * WP_DESC;
            const long long off = dk[0], sh = dk[1], sw = dk[2];
            if (sh >= 1 && sw >= 1 && sh <= 65535 && sw <= 65535 && off >= 0 && off + sh * sw * 3 <= src_bytes) {
                const double* M = inv + k * 9;
                const int xb = (x / bw0) * bw0, x1 = x - xb;
                const double X0 = M[0] * xb + M[1] * y + M[2];
                const double Y0 = M[3] * xb + M[4] * y + M[5];
                const double W0 = M[6] * xb + M[7] * y + M[8];
                double W = W0 + M[6] * x1;
                W = W != 0.0 ? 32.0 / W : 0.0;  // NaN != 0: 32 / NaN, as `W ? ... : 0` does
                const int X = sat_int(clamp_int_range((X0 + M[0] * x1) * W));
                const int Y = sat_int(clamp_int_range((Y0 + M[3] * x1) * W));
                bilinear_u8(src + off, (int)sh, (int)sw, 0, X, Y, v);
            }
        }
        sb[lp * 3] = (unsigned char)v[0];
        sb[lp * 3 + 1] = (unsigned char)v[1];
        sb[lp * 3 + 2] = (unsigned char)v[2];
    }
    __syncthreads();
    const long b0 = p0 * 3, nb = min((long)WP_PX * 3, n_px * 3 - b0);
    unsigned char* o = dst + b0;
    if (nb == WP_PX * 3 && (reinterpret_cast<size_t>(o) & 3) == 0) {
        unsigned int* o4 = reinterpret_cast<unsigned int*>(o);
#pragma unroll
        for (int j = 0; j < 3; ++j) o4[j * WP_THREADS + t] = s_out[j * WP_THREADS + t];
    } else {
        for (long j = t; j < nb; j += WP_THREADS) o[j] = sb[j];
    }
}

// ---- host: the maps of the word crops (cv2.getPerspectiveTransform + invert(DECOMP_LU), OpenCV 4.2, fp64) --------------
// getPerspectiveTransform: the 8 x 8 system of imgwarp.cpp (the products -x*u are float x float, as Point2f holds them),
// solved by LUImpl (lapack.cpp): partial pivoting on |a| (first maximum), a pivot below DBL_EPSILON*100 is singular and
// the solution all zeros; d = -1/pivot, alpha = a[j][i]*d added to the rows below (b too); back substitution
// s -= a[i][k]*b[k], b[i] = s / a[i][i]; then M[8] = 1.  invert of a 3 x 3 double matrix: det3, the cofactors times 1/d,
// the zero matrix when d == 0.  No contraction (-ffp-contract=off).
static void perspective_map(const float* q, float w, float h, double* M) {
    const float u[4] = {0.f, w, w, 0.f}, v[4] = {0.f, 0.f, h, h};
    double a[8][8], b[8];
    for (int i = 0; i < 4; ++i) {
        const float x = q[2 * i], y = q[2 * i + 1];
        a[i][0] = a[i + 4][3] = x;
        a[i][1] = a[i + 4][4] = y;
        a[i][2] = a[i + 4][5] = 1;
        a[i][3] = a[i][4] = a[i][5] = a[i + 4][0] = a[i + 4][1] = a[i + 4][2] = 0;
        a[i][6] = -x * u[i];
        a[i][7] = -y * u[i];
        a[i + 4][6] = -x * v[i];
        a[i + 4][7] = -y * v[i];
        b[i] = u[i];
        b[i + 4] = v[i];
    }
    const double eps = 2.220446049250313e-16 * 100;  // DBL_EPSILON * 100
    bool ok = true;
    for (int i = 0; i < 8 && ok; ++i) {
        int k = i;
        for (int j = i + 1; j < 8; ++j)
            if (fabs(a[j][i]) > fabs(a[k][i])) k = j;
        if (fabs(a[k][i]) < eps) {
            ok = false;
            break;
        }
        if (k != i) {
            for (int j = i; j < 8; ++j) std::swap(a[i][j], a[k][j]);
            std::swap(b[i], b[k]);
        }
        const double d = -1 / a[i][i];
        for (int j = i + 1; j < 8; ++j) {
            const double alpha = a[j][i] * d;
            for (k = i + 1; k < 8; ++k) a[j][k] += alpha * a[i][k];
            b[j] += alpha * b[i];
        }
    }
    if (ok) {
        for (int i = 7; i >= 0; --i) {
            double s = b[i];
            for (int k = i + 1; k < 8; ++k) s -= a[i][k] * b[k];
            b[i] = s / a[i][i];
        }
    }
    for (int i = 0; i < 8; ++i) M[i] = ok ? b[i] : 0.0;
    M[8] = 1.;
}

static void invert3(const double* S, double* D) {
    const double det = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6]);
    if (det == 0.) {
        for (int i = 0; i < 9; ++i) D[i] = 0.;
        return;
    }
    const double d = 1. / det;
    double t[9];
    t[0] = (S[4] * S[8] - S[5] * S[7]) * d;
    t[1] = (S[2] * S[7] - S[1] * S[8]) * d;
    t[2] = (S[1] * S[5] - S[2] * S[4]) * d;
    t[3] = (S[5] * S[6] - S[3] * S[8]) * d;
    t[4] = (S[0] * S[8] - S[2] * S[6]) * d;
    t[5] = (S[2] * S[3] - S[0] * S[5]) * d;
    t[6] = (S[3] * S[7] - S[4] * S[6]) * d;
    t[7] = (S[1] * S[6] - S[0] * S[7]) * d;
    t[8] = (S[0] * S[4] - S[1] * S[3]) * d;
    for (int i = 0; i < 9; ++i) D[i] = t[i];
}

}  // namespace

extern "C" {

int dbn_warp_affine_u8(const unsigned char* src, long src_bytes, const long long* desc, const double* coef, int N, int max_h, int max_w,
                       unsigned char* dst, long dst_bytes, void* stream) {
    DBN_REQUIRE(src && desc && coef && dst && N > 0 && N <= 65535 && max_h > 0 && max_w > 0 && max_h <= 65535 && max_w <= 65535);
    const dim3 grid(dbn_ceil_div(max_w, RS_TW), dbn_ceil_div(max_h, RS_TH), N);
    hipLaunchKernelGGL(warp_affine_u8_kernel, grid, dim3(RS_THREADS), 0, (hipStream_t)stream, src, src_bytes, desc, coef, dst, dst_bytes);
    return dbn_status();
}

int dbn_resize_cubic_u8(const unsigned char* src, long src_bytes, const long long* desc, const double* coef, int N, int max_h, int max_w,
                        unsigned char* dst, long dst_bytes, void* stream) {
    DBN_REQUIRE(src && desc && coef && dst && N > 0 && N <= 65535 && max_h > 0 && max_w > 0 && max_h <= 65535 && max_w <= 65535);
    const dim3 grid(dbn_ceil_div(max_w, RS_TW), dbn_ceil_div(max_h, RS_TH), N);
    hipLaunchKernelGGL(resize_cubic_u8_kernel, grid, dim3(RS_THREADS), 0, (hipStream_t)stream, src, src_bytes, desc, coef, dst, dst_bytes);
    return dbn_status();
}

int dbn_resize_linear_norm_u8(const unsigned char* src, long src_bytes, const long long* desc, const double* coef, int N, int CH, int CW,
                              float m0, float m1, float m2, float* out, void* stream) {
    DBN_REQUIRE(src && desc && coef && out && N > 0 && N <= 65535 && CH > 0 && CW > 0 && CH <= 65535 && CW <= 65535);
    const dim3 grid(dbn_ceil_div(CW, RS_TW), dbn_ceil_div(CH, RS_TH), N);
    hipLaunchKernelGGL(resize_linear_norm_u8_kernel, grid, dim3(RS_THREADS), 0, (hipStream_t)stream, src, src_bytes, desc, coef, CH, CW, m0,
                       m1, m2, out);
    return dbn_status();
}

int dbn_perspective_maps(const float* quads, int K, int out_h, int out_w, double* fwd, double* inv) {
    DBN_REQUIRE(quads && fwd && inv && K >= 0 && out_h > 0 && out_w > 0 && out_h <= 65535 && out_w <= 65535);
    for (long k = 0; k < K; ++k) {
        perspective_map(quads + k * 8, (float)out_w, (float)out_h, fwd + k * 9);
        invert3(fwd + k * 9, inv + k * 9);
    }
    return DBN_OK;
}

int dbn_warp_perspective_u8(const unsigned char* src, long src_bytes, const long long* desc, const double* inv, int K, int out_h, int out_w,
                            unsigned char* dst, long dst_bytes, void* stream) {
    DBN_REQUIRE(src && desc && inv && dst && K > 0 && out_h > 0 && out_w > 0 && out_h <= 65535 && out_w <= 65535);
    const long hw = (long)out_h * out_w, n_px = (long)K * hw;
    DBN_REQUIRE(hw + WP_PX <= 2147483647L && dst_bytes >= n_px * 3);
    const long blocks = (n_px + WP_PX - 1) / WP_PX;
    DBN_REQUIRE(blocks <= 2147483647L / WP_THREADS);
    // WarpPerspectiveInvoker's block width (BLOCK_SZ = 32): bh0 = min(16, rows), bw0 = min(1024 / bh0, cols); the block
    // height and the row stripes of parallel_for_ do not enter the arithmetic (rows are absolute)
    const int bh0 = out_h < 16 ? out_h : 16;
    const int bw0 = 1024 / bh0 < out_w ? 1024 / bh0 : out_w;
    hipLaunchKernelGGL(warp_perspective_u8_kernel, dim3((unsigned)blocks), dim3(WP_THREADS), 0, (hipStream_t)stream, src, src_bytes, desc, inv,
                       n_px, (int)hw, out_w, bw0, dst);
    return dbn_status();
}

}  // extern "C"
