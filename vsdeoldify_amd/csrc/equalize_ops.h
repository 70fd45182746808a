// Histogram-equalisation arithmetic shared by the kernels (equalize.hip) and the host (havc_equalize_frame_params, which the CPU tests call): the
// per-frame scalars of rgb_equalizer / rgb_balance (vsdeoldify/havc_utils.py:836-1145) in the reference's float64 sequence, the stand-ins of
// std.Merge / std.Expr, and the float32 steps of OpenCV's CLAHE and equalizeHist.  Every function that multiplies and adds switches FMA contraction
// off: numpy and Python round after every operation.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

#define EQ_GRID 8                        // tileGridSize (8, 8): the only one the reference passes
#define EQ_TILES (EQ_GRID * EQ_GRID)
#define EQ_THT_DARK_BLACK 0.15           // vsslib/constants.py:45-46
#define EQ_THT_BRIGHT_WHITE 0.70

// what the first pass leaves of a frame on the device: the sum of cv2's Y over the frame and (rgb_balance) the three channel sums
struct EqFrameRec { unsigned long long sum_y, chan[3]; };

// cv::borderInterpolate(p, len, BORDER_REFLECT_101) for p >= 0; len >= 2
__host__ __device__ inline int eq_reflect101(int p, int len) {
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}

// CLAHE's padded plane (clahe.cpp: copyMakeBorder by tiles - size % tiles on BOTH axes as soon as one of them is ragged) -> size of one tile
__host__ __device__ inline void eq_tile_size(int w, int h, int& tile_w, int& tile_h) {
    const bool ragged = (w % EQ_GRID) != 0 || (h % EQ_GRID) != 0;
    tile_w = (ragged ? w + EQ_GRID - w % EQ_GRID : w) / EQ_GRID;
    tile_h = (ragged ? h + EQ_GRID - h % EQ_GRID : h) / EQ_GRID;
}

// clipLimit of a tile: max(int(clip_limit * tile_area / 256), 1); clip_limit <= 0 = no clipping (0)
__host__ __device__ inline int eq_clip_limit(double clip_limit, int tile_area) {
    if (!(clip_limit > 0.0)) return 0;
    const int c = (int)(clip_limit * (double)tile_area / 256.0);
    return c > 1 ? c : 1;
}

// saturate_cast<uchar>(cvRound(sum * scale)): int -> float, one float32 product, round half to even
__host__ __device__ inline int eq_lut_value(int sum, float scale) {
#pragma clang fp contract(off)
    const float v = (float)sum * scale;
    const int r = (int)rintf(v);
    return r < 0 ? 0 : (r > 255 ? 255 : r);
}

// CLAHE_Interpolation_Body: (l11 * xa1 + l12 * xa) * ya1 + (l21 * xa1 + l22 * xa) * ya in float32, every product and sum rounded
__host__ __device__ inline int eq_interp(int l11, int l12, int l21, int l22, float xa, float xa1, float ya, float ya1) {
#pragma clang fp contract(off)
    const float p11 = (float)l11 * xa1, p12 = (float)l12 * xa, p21 = (float)l21 * xa1, p22 = (float)l22 * xa;
    const float top = p11 + p12, bot = p21 + p22;
    const float a = top * ya1, b = bot * ya;
    const float res = a + b;
    const int r = (int)rintf(res);
    return r < 0 ? 0 : (r > 255 ? 255 : r);
}

// tile index and weights of a coordinate: txf = x * (1.0f / tile) - 0.5f; floor; xa = txf - t1; both indices clamped afterwards
__host__ __device__ inline void eq_tile_coord(int x, float inv_tile, int& t1, int& t2, float& xa, float& xa1) {
#pragma clang fp contract(off)
    const float prod = (float)x * inv_tile;
    const float txf = prod - 0.5f;
    const int f = (int)floorf(txf);
    xa = txf - (float)f;
    xa1 = 1.0f - xa;
    t1 = f < 0 ? 0 : f;
    t2 = f + 1 > EQ_GRID - 1 ? EQ_GRID - 1 : f + 1;
}

// numpy's round(x, 6) on a float64 scalar: multiply, rint, divide
__host__ __device__ inline double eq_round6(double x) { return rint(x * 1e6) / 1e6; }

// Python's round(x, 8) on a float: the double nearest to the EXACT decimal rounding (half to even) of x.  x * 1e8 is taken exactly as p + err
// (one FMA); the rounded product can only mislead rint when it is a half-integer itself.  0 <= x < 2^20.
__host__ __device__ inline double eq_round8(double x) {
    const double p = x * 1e8;
    const double err = fma(x, 1e8, -p);
    double r = rint(p);
    const double fl = floor(p);
    if (p - fl == 0.5 && err != 0.0) r = err > 0.0 ? fl + 1.0 : fl;
    return r / 1e8;
}

// f_luma of a frame (havc_utils.py:878-885, imfilters.py:597-601): round(mean(Y) / maxrange, 6), with range_tv max(.. - 0.07, 0)
__host__ __device__ inline double eq_f_luma(unsigned long long sum_y, long long npix, int range_tv) {
    const double mean = (double)sum_y / (double)npix;
    const double r = eq_round6(mean / (range_tv ? 235.0 : 255.0));
    if (!range_tv) return r;
    const double d = r - 0.07;
    return d > 0.0 ? d : 0.0;
}
__host__ __device__ inline bool eq_gate(double f_luma) { return EQ_THT_DARK_BLACK <= f_luma && f_luma <= EQ_THT_BRIGHT_WHITE; }

// image_luma_blend (imfilters.py:612-624): the weight Image.blend gets as a C float, or -1 when the new image is taken as it is
__host__ __device__ inline float eq_blend_weight(double f_luma, double luma_limit, double alpha, double min_w, double decay) {
    if (!(f_luma < luma_limit)) return -1.f;
    double bs = pow(f_luma / luma_limit, decay);
    bs = bs > 0.0 ? bs : 0.0;
    bs = bs < 1.0 ? bs : 1.0;
    const double aw = alpha * bs;
    return (float)eq_round6(aw > min_w ? aw : min_w);
}

// Pillow's ImagingBlend for 0 <= alpha <= 1: (UINT8)((int)a + alpha * ((int)b - (int)a)) in float32
__host__ __device__ inline int eq_pil_blend(int a, int b, float alpha) {
#pragma clang fp contract(off)
    const float prod = alpha * (float)(b - a);
    const float t = (float)a + prod;
    return (int)(uint8_t)(int)t;
}

// std.Merge(a, b, w) on 8-bit samples (stand-in): a + (((b - a) * w15 + 16384) >> 15), w15 = int(w * 32768 + 0.5)
__host__ __device__ inline int eq_w15(double w) { return (int)(w * 32768.0 + 0.5); }
__host__ __device__ inline int eq_merge15(int a, int b, int w15) { return a + (((b - a) * w15 + 16384) >> 15); }

// std.Expr "x g *" on an 8-bit sample (stand-in): float32 product, round half to even, clamp
__host__ __device__ inline int eq_expr_mul(int v, float g) {
#pragma clang fp contract(off)
    const float p = (float)v * g;
    const int r = (int)rintf(p);
    return r < 0 ? 0 : (r > 255 ? 255 : r);
}

// frame_autowhite (havc_utils.py:1103-1122) from the channel sums: PlaneStatsAverage = sum / (npix * 255), the gains with their round(.., 8), as the
// float32 constants std.Expr makes of them
__host__ __device__ inline void eq_balance_gains(const unsigned long long chan[3], long long npix, const double factor[3], float gain[3]) {
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
    const double corr[3] = {rc, gc, bc};
    for (int c = 0; c < 3; ++c) {
        const double fc = factor[c] * corr[c];
        gain[c] = (float)eq_round8(fc / norm);
    }
}
