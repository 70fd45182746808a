// Edge-masked scene statistics: the arithmetic shared by the kernel (scedge.hip) and the host (havc_scene_edge_tables, which the CPU tests call).
// tests/scedges_util.py is the definition; every function here restates one line of it.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

constexpr int EDGE_MAX_RADIUS = 8;                        // sigma <= 2.5
constexpr int EDGE_MAX_TAPS = 2 * EDGE_MAX_RADIUS + 1;

// reflect-101 with period 2 (n - 1), applied as often as needed: the image coordinate g of the unbounded position u, and the direction dir (+1 / -1)
// in which positions around u run through the image: reflect(u + k) == reflect(g + dir * k) for every k.  n == 1: g = 0.
__host__ __device__ inline int edge_fold(int u, int n, int* dir) {
    *dir = 1;
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    int m = u % p;
    if (m < 0) m += p;
    if (m <= n - 1) return m;
    *dir = -1;
    return p - m;
}
__host__ __device__ inline int edge_reflect(int u, int n) { int d; return edge_fold(u, n, &d); }

// TCanny's blur radius for a sigma: max(int(3 sigma + 0.5), 1)
inline int edge_radius(double sigma) {
    const int r = (int)(3.0 * sigma + 0.5);
    return r < 1 ? 1 : r;
}

// the 2 r + 1 blur weights, tap -r first: exp(-x^2 / (2 sigma^2)) in float64, rounded to float32, normalised by their float32 sum taken from tap -r to +r
inline void edge_weights(double sigma, int r, float* w) {
#pragma clang fp contract(off)
    float sum = 0.f;
    for (int k = -r; k <= r; ++k) {
        w[k + r] = (float)exp(-(double)(k * k) / (2.0 * sigma * sigma));
        sum = sum + w[k + r];
    }
    for (int k = 0; k <= 2 * r; ++k) w[k] = w[k] / sum;
}

// the enhanced plane's table ('x 255 / sqrt 255 *' in float32, rounded half up)
inline void edge_enhance_table(uint8_t* t) {
#pragma clang fp contract(off)
    for (int x = 0; x < 256; ++x) {
        const float q = (float)x / 255.0f;
        const float s = sqrtf(q);
        const float v = s * 255.0f;
        const float f = floorf(v + 0.5f);
        t[x] = (uint8_t)(f > 255.f ? 255 : (int)f);
    }
}

// one std.Convolution pass of kirsch(): the three neighbours weighted 5 (sum s3) and all eight (sum s8) -> min(|5 s3 - 3 (s8 - s3)|, 255)
__host__ __device__ inline int edge_kirsch_pass(int s3, int s8) {
    int v = 8 * s3 - 3 * s8;
    v = v < 0 ? -v : v;
    return v > 255 ? 255 : v;
}

// std.MaskedMerge(blank, diff, mask) on one value
__host__ __device__ inline int edge_masked(int diff, int mask) { return (diff * mask + 127) / 255; }
