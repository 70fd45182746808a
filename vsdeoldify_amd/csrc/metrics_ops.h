// Arithmetic of havc_delta_e_clip shared by the kernel (metrics.hip) and the host: CIEDE2000 (Sharma, Wu, Dalal 2005) between two sRGB pixels in float64.
// oracle/imaging.py srgb_to_lab / ciede2000 is the definition; this file restates it statement by statement, with the oracle's constants, its branches on
// C1' C2' == 0 and on the +-180 degree hue wraps as written there.  What is NOT the oracle's bits: cbrt, hypot, atan2, sin, cos, exp of this platform's
// library against numpy's, x^7 by multiplication, the matrix row as a plain sum of products, and whatever the compiler fuses into FMAs.  The sRGB -> linear
// step is a table of the 256 byte values that the caller builds (de_srgb_linear is the formula); the Python package hands in numpy's own.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

#define DE_HIST_BINS 1025                         // bin i: floor(dE * 64) == i; the last one: dE >= 16
#define DE_HIST_SCALE 64.0

struct DeLab { double L, a, b; };

// (c / 255 > 0.04045) ? ((c / 255 + 0.055) / 1.055) ^ 2.4 : c / 255 / 12.92 -- the table entry of byte v (host only: the runtime's default table)
inline double de_srgb_linear(int v) {
    const double c = (double)v / 255.0;
    return c > 0.04045 ? pow((c + 0.055) / 1.055, 2.4) : c / 12.92;
}

__host__ __device__ inline double de_lab_f(double t) { return t > 0.008856 ? cbrt(t) : 7.787 * t + 16.0 / 116.0; }

// srgb_to_lab on linear r, g, b (table entries)
__host__ __device__ inline DeLab de_lab(double r, double g, double b) {
    const double x = (0.412453 * r + 0.357580 * g + 0.180423 * b) / 0.95047;
    const double y = (0.212671 * r + 0.715160 * g + 0.072169 * b) / 1.0;
    const double z = (0.019334 * r + 0.119193 * g + 0.950227 * b) / 1.08883;
    const double fx = de_lab_f(x), fy = de_lab_f(y), fz = de_lab_f(z);
    return DeLab{116.0 * fy - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz)};
}

__host__ __device__ inline double de_pow7(double c) {
    const double c2 = c * c, c4 = c2 * c2;
    return c4 * c2 * c;
}

// np.degrees(np.arctan2(y, x)) % 360: a negative angle gains 360
__host__ __device__ inline double de_hue(double y, double x) {
    const double h = atan2(y, x) * (180.0 / 3.141592653589793);
    return h < 0.0 ? h + 360.0 : h;
}

__host__ __device__ inline double de_rad(double deg) { return deg * (3.141592653589793 / 180.0); }

// ciede2000(lab1, lab2)
__host__ __device__ inline double de_ciede2000(DeLab p, DeLab q) {
    const double k25_7 = 6103515625.0;                           // 25 ^ 7
    const double C1 = hypot(p.a, p.b), C2 = hypot(q.a, q.b);
    const double Cb = (C1 + C2) / 2, Cb7 = de_pow7(Cb);
    const double G = 0.5 * (1 - sqrt(Cb7 / (Cb7 + k25_7)));
    const double a1p = (1 + G) * p.a, a2p = (1 + G) * q.a;
    const double C1p = hypot(a1p, p.b), C2p = hypot(a2p, q.b);
    const double h1p = de_hue(p.b, a1p), h2p = de_hue(q.b, a2p);
    const double dLp = q.L - p.L, dCp = C2p - C1p;
    const bool achromatic = C1p * C2p == 0;
    double dh = h2p - h1p;
    dh = achromatic ? 0 : (dh > 180 ? dh - 360 : (dh < -180 ? dh + 360 : dh));
    const double dHp = 2 * sqrt(C1p * C2p) * sin(de_rad(dh / 2));
    const double Lbp = (p.L + q.L) / 2, Cbp = (C1p + C2p) / 2;
    const double hs = h1p + h2p;
    const double hbp = achromatic ? hs : (fabs(h1p - h2p) <= 180 ? hs / 2 : (hs < 360 ? (hs + 360) / 2 : (hs - 360) / 2));
    const double T = 1 - 0.17 * cos(de_rad(hbp - 30)) + 0.24 * cos(de_rad(2 * hbp)) + 0.32 * cos(de_rad(3 * hbp + 6)) - 0.20 * cos(de_rad(4 * hbp - 63));
    const double u = (hbp - 275) / 25;
    const double dth = 30 * exp(-(u * u));
    const double Cbp7 = de_pow7(Cbp);
    const double Rc = 2 * sqrt(Cbp7 / (Cbp7 + k25_7));
    const double l50 = (Lbp - 50) * (Lbp - 50);
    const double Sl = 1 + 0.015 * l50 / sqrt(20 + l50);
    const double Sc = 1 + 0.045 * Cbp, Sh = 1 + 0.015 * Cbp * T;
    const double Rt = -sin(de_rad(2 * dth)) * Rc;
    const double tl = dLp / Sl, tc = dCp / Sc, th = dHp / Sh;
    return sqrt(tl * tl + tc * tc + th * th + Rt * tc * th);
}

// the histogram bin of a dE; always inside the histogram, whatever comes in (a NaN counts as bin 0)
__host__ __device__ inline int de_bin(double de) {
    const double v = floor(de * DE_HIST_SCALE);
    return v >= (double)(DE_HIST_BINS - 1) ? DE_HIST_BINS - 1 : (v >= 0 ? (int)v : 0);
}

// one pixel pair: the two pixels' bytes through the table `lin`
__host__ __device__ inline double de_pixel(const double* lin, const uint8_t* a, const uint8_t* b) {
    return de_ciede2000(de_lab(lin[a[0]], lin[a[1]], lin[a[2]]), de_lab(lin[b[0]], lin[b[1]], lin[b[2]]));
}
