// Multi-scale Retinex (MSRCP) arithmetic shared by the kernels (retinex.hip) and the host (havc_retinex_coefficients, havc_retinex_frame_params, which
// the CPU tests call).  Everything is float64 in a stated order; every function that multiplies and adds switches FMA contraction off, as numpy rounds
// after every operation.  The gate and the blend weight are the reference's Python around the plugin (vsslib/vsretinex.py:62-84) on top of
// equalize_ops.h's f_luma; the pixel work is the published MSRCP (Petro / Sbert / Morel, IPOL 2014) with the Young - van Vliet recursive Gaussian.
#pragma once
#include "equalize_ops.h"

#define RET_MAX_SIGMAS 8
#define RET_BINS 4096                    // histogram bins of the percentile stretch
#define RET_THR 0.001                    // lower_thr = upper_thr of the reference's call

// what the passes leave of a frame on the device.  min_inv / max_key: the ordered bit patterns (ret_key) of the frame's smallest and largest MSR value,
// the smallest one inverted so that both start from zero and grow under an integer atomic maximum.
struct RetFrameRec {
    unsigned long long sum_y, min_inv, max_key;
    double lo, inv;                      // stretch: O' = clamp((O - lo) * inv, 0, 1)
    int gate, use_i;                     // gate: 0 = the frame comes back as it went in; use_i: 1 = O' = I (mx <= mn or hi <= lo)
    float weight;                        // Pillow blend weight, -1 = none
    int reserved;
};

// Young - van Vliet coefficients of one sigma -> out4 = {B, B1, B2, B3}
__host__ __device__ inline void ret_coefficients(double sigma, double* out4) {
#pragma clang fp contract(off)
    double q;
    if (sigma >= 2.5) {
        const double m = 0.98711 * sigma;
        q = m - 0.96330;
    } else {
        const double m = 0.26891 * sigma;
        const double r = sqrt(1.0 - m);
        const double n = 4.14554 * r;
        q = 3.97156 - n;
    }
    const double q2 = q * q;
    const double q3 = q2 * q;
    const double a1 = 2.44413 * q, a2 = 1.4281 * q2, a3 = 0.422205 * q3;
    const double b0 = ((1.57825 + a1) + a2) + a3;
    const double c2 = 2.85619 * q2, c3 = 1.26661 * q3;
    const double b1 = (a1 + c2) + c3;
    const double b2 = -(a2 + c3);
    const double b3 = a3;
    const double s = (b1 + b2) + b3;
    out4[0] = 1.0 - s / b0;
    out4[1] = b1 / b0;
    out4[2] = b2 / b0;
    out4[3] = b3 / b0;
}

// one step of the recursion: ((B * x + B1 * p1) + B2 * p2) + B3 * p3
__host__ __device__ inline double ret_step(double x, double p1, double p2, double p3, double B, double B1, double B2, double B3) {
#pragma clang fp contract(off)
    const double t0 = B * x, t1 = B1 * p1, t2 = B2 * p2, t3 = B3 * p3;
    return ((t0 + t1) + t2) + t3;
}

// I = ((R - sF) + (G - sF) + (B - sF)) * (1.0 / (3 * sR)): the sum is an exact integer
__host__ __device__ inline double ret_intensity(int r, int g, int b, int sF, double inv3sR) {
    return (double)(r + g + b - 3 * sF) * inv3sR;
}

// one factor of the MSR product
__host__ __device__ inline double ret_factor(double i, double g) {
#pragma clang fp contract(off)
    if (g <= 0.0) return 1.0;
    const double q = i / g;
    return q + 1.0;
}

// a double as an unsigned integer that orders the way the doubles do
__host__ __device__ inline unsigned long long ret_key(double v) {
    unsigned long long u;
    __builtin_memcpy(&u, &v, 8);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__host__ __device__ inline double ret_unkey(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    double v;
    __builtin_memcpy(&v, &u, 8);
    return v;
}

// histogram bin of an MSR value; scale = 4095.0 / (mx - mn).  The clamp changes nothing for mn <= o <= mx; it keeps a NaN inside the table.
__host__ __device__ inline int ret_bin(double o, double mn, double scale) {
#pragma clang fp contract(off)
    const double d = o - mn;
    const double p = d * scale;
    if (!(p > 0.0)) return 0;
    return p >= (double)(RET_BINS - 1) ? RET_BINS - 1 : (int)p;
}
// the count a running sum has to exceed: (int)(npix * thr + 0.5)
__host__ __device__ inline long long ret_threshold_count(long long npix) {
#pragma clang fp contract(off)
    const double p = (double)npix * RET_THR;
    return (long long)(p + 0.5);
}
// the MSR value of a histogram bin: k / 4095.0 * (mx - mn) + mn
__host__ __device__ inline double ret_bin_value(int k, double mn, double mx) {
#pragma clang fp contract(off)
    const double f = (double)k / (double)(RET_BINS - 1);
    const double p = f * (mx - mn);
    return p + mn;
}

__host__ __device__ inline double ret_stretch(double o, double lo, double inv) {
#pragma clang fp contract(off)
    const double d = o - lo;
    const double p = d * inv;
    return p < 0.0 ? 0.0 : (p > 1.0 ? 1.0 : p);
}

// gain of a pixel: O' / I, capped so that the largest channel stays inside the source range
__host__ __device__ inline double ret_gain(double o, double i, int max_c_minus_sF, int sR) {
    double gain = i <= 0.0 ? 1.0 : o / i;
    if (max_c_minus_sF > 0) {
        const double cap = (double)sR / (double)max_c_minus_sF;
        gain = gain < cap ? gain : cap;
    }
    return gain;
}
// one output sample: clamp((int)floor((c - sF) * gain * (dR / (double)sR) + dF + 0.5), 0, 255); range_scale = dR / (double)sR
__host__ __device__ inline int ret_out_channel(int c_minus_sF, double gain, double range_scale, int dF) {
#pragma clang fp contract(off)
    const double a = (double)c_minus_sF * gain;
    const double b = a * range_scale;
    const double s = b + (double)dF;
    const double v = floor(s + 0.5);
    return v < 0.0 ? 0 : (v > 255.0 ? 255 : (int)v);
}

// the reference's gate around the plugin (vsretinex.py:74-77) and image_luma_blend(img, img_new, f_luma, 0.40, 0.90, 0.25, 3.0) (:80)
__host__ __device__ inline bool ret_gate(double f_luma, double luma_dark, double luma_bright) { return luma_dark <= f_luma && f_luma <= luma_bright; }
__host__ __device__ inline float ret_blend_weight(double f_luma, int blend) { return blend ? eq_blend_weight(f_luma, 0.40, 0.90, 0.25, 3.0) : -1.f; }
