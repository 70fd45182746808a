// Arithmetic of havc_planes_to_rgb24 / havc_rgb24_to_planes shared by the kernels (vformat.hip) and the host (the constants, set by the launchers): what
// tweak_ops.h does for BT.709 full range 8 bit, with the matrix, the range and the depth as parameters.  tests/vformat_util.py is the definition; every
// float32 expression here is that file's sequence, one rounding per operation.  Every function that multiplies and adds switches FMA contraction off.
// UNPINNED like the rest of the zimg stand-in: the scalings below are written down by this project, not recorded from zimg.
//     limited, depth b:  Y code = Y 219 2^(b - 8) + 16 2^(b - 8),  C code = C 224 2^(b - 8) + 2^(b - 1)
//     full,    depth b:  Y code = Y (2^b - 1) + 0,                 C code = C (2^b - 1) + 2^(b - 1)
//     8-bit codes back:  Y = (y - 16) / 219, C = (c - 128) / 224 (limited);  Y = (y - 0) / 255, C = (c - 128) / 255 (full)
//     depth b > 8 to 8 bit, no dither, round half to even, clamped:  limited v 2^-(b - 8) (luma and chroma alike);  full luma v (255 / (2^b - 1)), full chroma
//                        ((v - 2^(b - 1)) (255 / (2^b - 1))) + 128
#pragma once
#include "tweak_ops.h"

// KR, KB of H.273 matrix_coefficients 1 (BT.709), 5 (BT.470BG), 6 (SMPTE 170M), 9 (BT.2020 NCL); false: not one of them
inline bool vf_matrix(int code, double& kr, double& kb) {
    switch (code) {
        case 1: kr = 0.2126; kb = 0.0722; return true;
        case 5: case 6: kr = 0.299; kb = 0.114; return true;
        case 9: kr = 0.2627; kb = 0.0593; return true;
    }
    return false;
}

// every derived constant of VfArgs (kernels.h) in float64, in the order tests/vformat_util.py writes them, then float32
inline void vf_constants(VfArgs& a) {
#pragma clang fp contract(off)
    double kr = 0.2126, kb = 0.0722;
    (void)vf_matrix(a.matrix, kr, kb);
    const double kg = 1.0 - kr - kb;
    a.kr = (float)kr; a.kg = (float)kg; a.kb = (float)kb;
    a.cb_div = (float)(2.0 * (1.0 - kb)); a.cr_div = (float)(2.0 * (1.0 - kr));
    a.r_cr = (float)(2.0 * (1.0 - kr)); a.b_cb = (float)(2.0 * (1.0 - kb));
    a.g_cr = (float)(2.0 * (1.0 - kr) * kr / kg); a.g_cb = (float)(2.0 * (1.0 - kb) * kb / kg);
    a.y_off = a.full_range ? 0.f : 16.f; a.y_scale = a.full_range ? 255.f : 219.f; a.c_scale = a.full_range ? 255.f : 224.f;
    const double top = (double)((1 << a.bits) - 1), step = (double)(1 << (a.bits - 8));
    a.depth_mul = (float)(a.depth_full_range ? 255.0 / top : 1.0 / step);
    a.depth_half = (float)(1 << (a.bits - 1));
    a.ys = (float)(a.full_range ? top : 219.0 * step); a.yo = (float)(a.full_range ? 0.0 : 16.0 * step);
    a.cs = (float)(a.full_range ? top : 224.0 * step); a.co = (float)(1 << (a.bits - 1));
    a.hi = (float)top;
    tw_all_weights(a.wt);
}

// a stored sample as the 8-bit code the matrix step sees: the depth step of its own (uint8 planes pass)
template <typename T>
__host__ __device__ inline int vf_code8(T raw, bool chroma, const VfArgs& a) {
#pragma clang fp contract(off)
    if (sizeof(T) == 1) return (int)raw;
    const float v = (float)raw;
    float p;
    if (!a.depth_full_range || !chroma) {
        p = v * a.depth_mul;
    } else {
        const float d = v - a.depth_half;
        const float m = d * a.depth_mul;
        p = m + 128.f;
    }
    return tw_quant(p);
}

// tw_rgb2ycc / tw_ycc2rgb with the matrix of a
__host__ __device__ inline void vf_rgb2ycc(float r, float g, float b, const VfArgs& a, float& y, float& cb, float& cr) {
#pragma clang fp contract(off)
    const float pr = a.kr * r, pg = a.kg * g, pb = a.kb * b;
    const float s = pr + pg;
    y = s + pb;
    cb = (b - y) / a.cb_div;
    cr = (r - y) / a.cr_div;
}
__host__ __device__ inline void vf_ycc2rgb(float y, float cb, float cr, const VfArgs& a, float& r, float& g, float& b) {
#pragma clang fp contract(off)
    const float rc = a.r_cr * cr, bc = a.b_cb * cb;
    const float gr = a.g_cr * cr, gb = a.g_cb * cb;
    const float r1 = y + rc, b1 = y + bc, g0 = y - gr;
    const float g1 = g0 - gb;
    r = r1 * 255.f; g = g1 * 255.f; b = b1 * 255.f;
}

// a normalised sample as a code value before rounding: x scale + offset
__host__ __device__ inline float vf_scale(float x, float scale, float offset) {
#pragma clang fp contract(off)
    const float p = x * scale;
    return p + offset;
}
__host__ __device__ inline int vf_quant(float v, float hi) {
    const float r = rintf(v);
    return (int)fminf(fmaxf(r, 0.f), hi);
}

// tw_diffuse with the clamp at [0, hi]
__host__ __device__ inline float vf_diffuse(float x, float left, float topright, float top, float topleft, float hi, float& q) {
#pragma clang fp contract(off)
    const float a = left * 0.4375f, b = topright * 0.1875f, c = top * 0.3125f, d = topleft * 0.0625f;
    const float ab = a + b;
    const float abc = ab + c;
    const float e = abc + d;
    const float s = x + e;
    const float v = fminf(fmaxf(s, 0.f), hi);
    q = rintf(v);
    return v - q;
}
