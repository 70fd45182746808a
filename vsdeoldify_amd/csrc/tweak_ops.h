// Arithmetic of HAVC_tweak / HAVC_adjust_rgb shared by the kernels (tweak.hip) and the host (rt_filters.cpp: the filter weights, havc_adjust_frame_params,
// which the CPU tests call): the stand-in of zimg's RGB <-> YUV420P8 conversion (BT.709, full range, Mitchell bicubic chroma resampling, Floyd - Steinberg
// error diffusion on the way back) and of the std.Expr / std.Levels steps of vs_tweak (vsslib/vsfilters.py:753-850) and adjust_rgb (havc_utils.py:664-749).
// tests/tweak_util.py is the definition; every float32 expression here is that file's sequence, one rounding per operation.  Every function that multiplies
// and adds switches FMA contraction off.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

#define TW_KR 0.2126                     // BT.709
#define TW_KB 0.0722
#define TW_KG (1.0 - TW_KR - TW_KB)
#define TW_DOWN_TAPS 8                   // 2 : 1 pass: taps 2j - 3 .. 2j + 4
#define TW_DOWN_FIRST (-3)
#define TW_UP_TAPS 4                     // 1 : 2 pass: taps m + first .. m + first + 3 of output sample 2m + parity
#define TW_UP_FIRST_V_EVEN (-2)          // centred siting: centre (i + 0.5) / 2 - 0.5 -> floor(centre) - 1
#define TW_UP_FIRST_V_ODD (-1)
#define TW_UP_FIRST_H (-1)               // left siting: centre i / 2, either parity

// -1 -> 0, -2 -> 1, n -> n - 1, n + 1 -> n - 2, repeated while outside (planes narrower than the kernel)
__host__ __device__ inline int tw_mirror(int p, int n) {
    while (p < 0 || p >= n) p = p < 0 ? -1 - p : 2 * n - 1 - p;
    return p;
}

// Mitchell - Netravali bicubic, b = c = 1/3, in float64: the products and sums in the order tests/tweak_util.py writes them
inline double tw_mitchell(double x) {
#pragma clang fp contract(off)
    const double b = 1.0 / 3.0, c = 1.0 / 3.0;
    x = fabs(x);
    const double x2 = x * x, x3 = x2 * x;
    if (x < 1.0) {
        const double p0 = (12.0 - 9.0 * b) - 6.0 * c, p1 = (-18.0 + 12.0 * b) + 6.0 * c, p2 = 6.0 - 2.0 * b;
        return ((p0 * x3 + p1 * x2) + p2) / 6.0;
    }
    if (x < 2.0) {
        const double q0 = -b - 6.0 * c, q1 = 6.0 * b + 30.0 * c, q2 = -12.0 * b - 48.0 * c, q3 = 8.0 * b + 24.0 * c;
        return (((q0 * x3 + q1 * x2) + q2 * x) + q3) / 6.0;
    }
    return 0.0;
}

// n weights at distances (first + k - centre) / stretch, normalised to sum 1 in float64 (summed in tap order), then float32
inline void tw_weights(int n, double first, double centre, double stretch, float* out) {
#pragma clang fp contract(off)
    double w[8], s = 0.0;
    for (int k = 0; k < n; ++k) { w[k] = tw_mitchell(((first + (double)k) - centre) / stretch); s += w[k]; }
    for (int k = 0; k < n; ++k) out[k] = (float)(w[k] / s);
}

// the filters of both directions (TweakWeights: kernels.h): down_v (centre 2j + 0.5), down_h (centre 2j), up_v[parity], up_h[parity]
inline void tw_all_weights(TweakWeights& t) {
    tw_weights(TW_DOWN_TAPS, TW_DOWN_FIRST, 0.5, 2.0, t.down_v);
    tw_weights(TW_DOWN_TAPS, TW_DOWN_FIRST, 0.0, 2.0, t.down_h);
    tw_weights(TW_UP_TAPS, TW_UP_FIRST_V_EVEN, 0.25 - 0.5, 1.0, t.up_v[0]);
    tw_weights(TW_UP_TAPS, TW_UP_FIRST_V_ODD, 0.75 - 0.5, 1.0, t.up_v[1]);
    tw_weights(TW_UP_TAPS, TW_UP_FIRST_H, 0.0, 1.0, t.up_h[0]);
    tw_weights(TW_UP_TAPS, TW_UP_FIRST_H, 0.5, 1.0, t.up_h[1]);
}

__host__ __device__ inline int tw_quant(float v) {
    const int r = (int)rintf(v);
    return r < 0 ? 0 : (r > 255 ? 255 : r);
}

// forward matrix on r, g, b = sample / 255: Y = (KR r + KG g) + KB b, Cb = (b - Y) / (2 (1 - KB)), Cr = (r - Y) / (2 (1 - KR))
__host__ __device__ inline void tw_rgb2ycc(float r, float g, float b, float& y, float& cb, float& cr) {
#pragma clang fp contract(off)
    const float pr = (float)TW_KR * r, pg = (float)TW_KG * g, pb = (float)TW_KB * b;
    const float s = pr + pg;
    y = s + pb;
    cb = (b - y) / (float)(2.0 * (1.0 - TW_KB));
    cr = (r - y) / (float)(2.0 * (1.0 - TW_KR));
}
__host__ __device__ inline int tw_quant_y(float y) {
#pragma clang fp contract(off)
    const float p = y * 255.f;
    return tw_quant(p);
}
__host__ __device__ inline int tw_quant_c(float c) {
#pragma clang fp contract(off)
    const float p = c * 255.f;
    const float s = p + 128.f;
    return tw_quant(s);
}

// inverse matrix, scaled to 0..255: R = Y + 2(1 - KR) Cr, B = Y + 2(1 - KB) Cb, G = (Y - (2(1 - KR) KR / KG) Cr) - (2(1 - KB) KB / KG) Cb
__host__ __device__ inline void tw_ycc2rgb(float y, float cb, float cr, float& r, float& g, float& b) {
#pragma clang fp contract(off)
    const float rc = (float)(2.0 * (1.0 - TW_KR)) * cr, bc = (float)(2.0 * (1.0 - TW_KB)) * cb;
    const float gr = (float)(2.0 * (1.0 - TW_KR) * TW_KR / TW_KG) * cr, gb = (float)(2.0 * (1.0 - TW_KB) * TW_KB / TW_KG) * cb;
    const float r1 = y + rc, b1 = y + bc, g0 = y - gr;
    const float g1 = g0 - gb;
    r = r1 * 255.f; g = g1 * 255.f; b = b1 * 255.f;
}

// the two std.Expr of vs_tweak (:809-812) on 8-bit U, V: ((x - 128) c + (y - 128) s) + 128 and ((y - 128) c - (x - 128) s) + 128, max 0 min 255, stored
// rounded half to even
__host__ __device__ inline void tw_hue_sat(int u, int v, float c, float s, int& un, int& vn) {
#pragma clang fp contract(off)
    const float x = (float)u - 128.f, y = (float)v - 128.f;
    const float xc = x * c, ys = y * s, yc = y * c, xs = x * s;
    const float a = xc + ys, b = yc - xs;
    float pu = a + 128.f, pv = b + 128.f;
    pu = fminf(fmaxf(pu, 0.f), 255.f);
    pv = fminf(fmaxf(pv, 0.f), 255.f);
    un = tw_quant(pu);
    vn = tw_quant(pv);
}

// one step of the error diffusion: e = ((left 7/16 + topright 3/16) + top 5/16) + topleft 1/16; v = clamp(x + e, 0, 255); q = rint(v); the pixel keeps v - q
__host__ __device__ inline float tw_diffuse(float x, float left, float topright, float top, float topleft, float& q) {
#pragma clang fp contract(off)
    const float a = left * 0.4375f, b = topright * 0.1875f, c = top * 0.3125f, d = topleft * 0.0625f;
    const float ab = a + b;
    const float abc = ab + c;
    const float e = abc + d;
    const float s = x + e;
    const float v = fminf(fmaxf(s, 0.f), 255.f);
    q = rintf(v);
    return v - q;
}

// vs_rgb_normalize's frame function (vsslib/vsfilters.py:1019-1033) from the channel sums: the gains in float64, NOT rounded (they reach std.Expr through repr)
__host__ __device__ inline void tw_normalize_gains(const unsigned long long chan[3], long long npix, double gain[3]) {
#pragma clang fp contract(off)
    const double small_number = 0.000000001, den = (double)npix * 255.0;
    const double red = (double)chan[0] / den, green = (double)chan[1] / den, blue = (double)chan[2] / den;
    double max_rgb = red;
    max_rgb = green > max_rgb ? green : max_rgb;
    max_rgb = blue > max_rgb ? blue : max_rgb;
    const double rc = max_rgb / (red > small_number ? red : small_number);
    const double gc = max_rgb / (green > small_number ? green : small_number);
    const double bc = max_rgb / (blue > small_number ? blue : small_number);
    const double rr = rc * rc, gg = gc * gc, bb = bc * bc;
    const double s = (rr + gg) + bb;
    const double q = sqrt(s) / sqrt(3.0);
    double norm = blue;
    norm = q > norm ? q : norm;
    norm = small_number > norm ? small_number : norm;
    gain[0] = rc / norm; gain[1] = gc / norm; gain[2] = bc / norm;
}

// std.Expr "x r * rb +" on an 8-bit sample: float32 product, float32 sum, round half to even, clamp
__host__ __device__ inline int tw_affine(int v, float gain, float bias) {
#pragma clang fp contract(off)
    const float p = (float)v * gain;
    const float s = p + bias;
    return tw_quant(s);
}
