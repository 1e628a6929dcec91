// The pixel arithmetic of the photometric augmentation (csrc/photometric.hip; definition: DESIGN.md section 37), written once for the
// kernels and for the host walk of dbn_color_jitter_host.  It restates Pillow as torchvision's ColorJitter drives it on a PIL image:
// Image.blend (ImageEnhance.Brightness / Contrast / Color), convert('L'), convert('HSV') and back.  Every rounding below is one
// Pillow's C code makes: float32 variables, float64 wherever a double constant takes part.  The library is built with
// -ffp-contract=off: the multiply and the add of a blend stay two roundings.
#pragma once
#include <math.h>

#define PH_FN __host__ __device__ __forceinline__

constexpr int PH_D = 8;  // int64 fields of an image's record
enum { PH_OFF = 0, PH_H = 1, PH_W = 2, PH_CHUNK = 3, PH_OPS = 4, PH_F01 = 5, PH_F23 = 6 };
enum { PH_BRIGHTNESS = 1, PH_CONTRAST = 2, PH_COLOUR = 3, PH_HUE = 4 };
constexpr int PH_CHUNK_PIXELS = 1024;  // pixels of one image that a workgroup takes per step

// an image's plan as its record packs it: ops = steps | code of step k << 4 (k + 1); f01 / f23 hold per step 32 bits, the float32
// factor, or the hue shift 0 .. 255.  Fields are taken by shifts, so a step index that is a variable never indexes an array.
struct ph_plan {
    unsigned long long ops, f01, f23;
};

PH_FN ph_plan ph_unpack(const long long* d) {
    return ph_plan{(unsigned long long)d[PH_OPS], (unsigned long long)d[PH_F01], (unsigned long long)d[PH_F23]};
}
PH_FN int ph_count(const ph_plan& p) { return (int)(p.ops & 15); }
PH_FN int ph_op(const ph_plan& p, int k) { return (int)((p.ops >> (4 * (k + 1))) & 15); }
PH_FN unsigned ph_val(const ph_plan& p, int k) { return (unsigned)(((k & 2) ? p.f23 : p.f01) >> (32 * (k & 1))); }

// the step at which the plan takes the grey mean, or -1
PH_FN int ph_contrast_step(const ph_plan& p) {
    int at = -1;
    for (int k = 0; k < ph_count(p); ++k)
        if (ph_op(p, k) == PH_CONTRAST) at = k;
    return at;
}

PH_FN float ph_factor(unsigned bits) { return __builtin_bit_cast(float, bits); }

// Image.blend(d, x, a) of one channel
PH_FN int ph_blend(int d, int x, float a) {
    const float t = (float)d + a * (float)(x - d);
    return t <= 0.f ? 0 : t >= 255.f ? 255 : (int)t;
}

// convert('L')
PH_FN int ph_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }

PH_FN int ph_clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// C's round() of a value that is not negative (v - trunc(v) is exact)
PH_FN int ph_round(double v) {
    const double t = trunc(v);
    return (int)t + (v - t >= 0.5 ? 1 : 0);
}

// RGB -> HSV (Convert.c rgb2hsv_row), H + shift mod 256, HSV -> RGB (hsv2rgb)
PH_FN void ph_hue(int& r, int& g, int& b, int shift) {
    const int maxc = r > g ? (r > b ? r : b) : (g > b ? g : b);
    const int minc = r < g ? (r < b ? r : b) : (g < b ? g : b);
    int H = 0, S = 0;
    const int V = maxc;
    if (maxc != minc) {
        const float cr = (float)(maxc - minc);
        const float sat = cr / (float)maxc;
        const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
        float h;
        if (r == maxc)
            h = bc - gc;
        else if (g == maxc)
            h = (float)(2.0 + (double)rc - (double)bc);
        else
            h = (float)(4.0 + (double)gc - (double)rc);
        const double u = (double)h / 6.0 + 1.0;  // in [5 / 6, 11 / 6]: fmod(u, 1.0) is u - trunc(u), exactly
        h = (float)(u - trunc(u));
        H = ph_clip8((int)((double)h * 255.0));
        S = ph_clip8((int)((double)sat * 255.0));
    }
    H = (H + shift) & 255;
    if (S == 0) {
        r = g = b = V;
        return;
    }
    const double hf = (double)H * 6.0 / 255.0;
    const int i = (int)hf;  // floor: hf is not negative
    const float f = (float)(hf - (double)i);
    const float fs = (float)((double)S / 255.0);
    const int p = ph_clip8(ph_round((double)V * (1.0 - (double)fs)));
    const int q = ph_clip8(ph_round((double)V * (1.0 - (double)(fs * f))));
    const int t = ph_clip8(ph_round((double)V * (1.0 - (double)fs * (1.0 - (double)f))));
    switch (i % 6) {
        case 0: r = V, g = t, b = p; break;
        case 1: r = q, g = V, b = p; break;
        case 2: r = p, g = V, b = t; break;
        case 3: r = p, g = q, b = V; break;
        case 4: r = t, g = p, b = V; break;
        default: r = V, g = p, b = q; break;
    }
}

// steps [0, end) of the plan on one pixel; m is the mean grey of the image as the contrast step meets it
PH_FN void ph_steps(const ph_plan& p, int end, int m, int& r, int& g, int& b) {
    for (int k = 0; k < end; ++k) {
        const int op = ph_op(p, k);
        if (op == PH_HUE) {
            ph_hue(r, g, b, (int)ph_val(p, k));
            continue;
        }
        const float a = ph_factor(ph_val(p, k));
        if (op == PH_COLOUR) {
            const int l = ph_luma(r, g, b);
            r = ph_blend(l, r, a), g = ph_blend(l, g, a), b = ph_blend(l, b, a);
        } else {
            const int d = op == PH_CONTRAST ? m : 0;
            r = ph_blend(d, r, a), g = ph_blend(d, g, a), b = ph_blend(d, b, a);
        }
    }
}

// int(sum / count + 0.5) in float64: ImageEnhance.Contrast's mean
PH_FN int ph_mean(unsigned long long sum, long count) { return (int)((double)sum / (double)count + 0.5); }
