// Arithmetic of the scene filter shared by the kernels (scfilter.hip) and the host (havc_scene_gray / havc_scene_ssim_value, which the CPU tests call).
#pragma once
#include <stdint.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

// OpenCV's 8-bit gray (color.simd / color_yuv.simd: yuv_shift 14, CV_DESCALE): COLOR_RGB2GRAY and the Y of COLOR_RGB2YUV are the same integer expression
// (oracle/cvcolor.py: R2Y / G2Y / B2Y); the coefficients sum to 16384, so Y <= 255 for any input.
__host__ __device__ inline int scf_gray(int r, int g, int b) { return (4899 * r + 9617 * g + 1868 * b + 8192) >> 14; }

// the four gray values of a 12-byte group of four pixels held in three little-endian dwords
__host__ __device__ inline void scf_gray4(const uint32_t w[3], int y[4]) {
    y[0] = scf_gray(w[0] & 255u, (w[0] >> 8) & 255u, (w[0] >> 16) & 255u);
    y[1] = scf_gray(w[0] >> 24, w[1] & 255u, (w[1] >> 8) & 255u);
    y[2] = scf_gray((w[1] >> 16) & 255u, w[1] >> 24, w[2] & 255u);
    y[3] = scf_gray((w[2] >> 8) & 255u, (w[2] >> 16) & 255u, w[2] >> 24);
}

// skimage.metrics.structural_similarity at one window position (win_size 7 -> 49 samples, uniform window, data_range 255, K1 0.01, K2 0.03, sample
// covariance) from the window's integer sums sx = sum x, sy = sum y, sxx = sum x^2, syy = sum y^2, sxy = sum x * y:
//     ux = sx / 49, vx = (49 sxx - sx^2) / (49 * 48), vxy = (49 sxy - sx sy) / (49 * 48)
//     S  = (2 ux uy + C1) (2 vxy + C2) / ((ux^2 + uy^2 + C1) (vx + vy + C2)),   C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2
// Numerator and denominator are multiplied through by 49^2 * (49 * 48): every data term is then an exact integer below 2^30 (no difference of rounded
// means), only the two constants are rounded, and one division is left.  Against the form with the divisions written out the quotient moves by a few
// ulp (1e-16 relative).
__host__ __device__ inline double scf_ssim_value(int sx, int sy, int sxx, int syy, int sxy) {
    const double c1 = 2401.0 * ((0.01 * 255.0) * (0.01 * 255.0)), c2 = 2352.0 * ((0.03 * 255.0) * (0.03 * 255.0));
    const long long pxx = (long long)sx * sx, pyy = (long long)sy * sy, pxy = (long long)sx * sy;
    const double a1 = (double)(2 * pxy) + c1;
    const double a2 = (double)(2 * (49ll * sxy - pxy)) + c2;
    const double b1 = (double)(pxx + pyy) + c1;
    const double b2 = (double)((49ll * sxx - pxx) + (49ll * syy - pyy)) + c2;
    return (a1 * a2) / (b1 * b2);
}
