// Arithmetic of havc_overlay_clip shared by the kernel (overlay.hip) and the host: the stand-ins of the std.Expr blend strings and of std.MaskedMerge in
// HAVC_clip_overlay (vsdeoldify/__init__.py:3029-3148).  tests/overlay_util.py is the definition; every float32 expression here is that file's sequence in
// the RPN order of the reference's strings, one rounding per operation, never fused, the divisions IEEE.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

enum OverlayMode { OV_NORMAL = 0, OV_ADDITION, OV_AVERAGE, OV_DIFFERENCE, OV_DIVIDE, OV_EXCLUSION, OV_MULTIPLY, OV_OVERLAY, OV_SUBTRACT, OV_MODES };

// std.Expr's store to 8 bit: clamp, add one half, truncate
__host__ __device__ inline int ov_expr8(float v) {
#pragma clang fp contract(off)
    return (int)(fminf(fmaxf(v, 0.f), 255.f) + 0.5f);
}

// x = the overlay's sample, y = the base's; peak 255, neutral 128
__host__ __device__ inline int ov_blend(int mode, int xi, int yi) {
#pragma clang fp contract(off)
    const float x = (float)xi, y = (float)yi, peak = 255.f;
    float v;
    switch (mode) {
    case OV_ADDITION: v = x + y; break;
    case OV_AVERAGE: v = (x + y) / 2.f; break;
    case OV_DIFFERENCE: v = fabsf(x - y); break;
    case OV_DIVIDE: v = y <= 0.f ? peak : (peak * x) / y; break;
    case OV_EXCLUSION: v = (x + y) - ((2.f * x) * y) / peak; break;
    case OV_MULTIPLY: v = (x * y) / peak; break;
    case OV_OVERLAY: v = x < 128.f ? 2.f * ((x * y) / peak) : peak - 2.f * (((peak - x) * (peak - y)) / peak); break;
    case OV_SUBTRACT: v = x - y; break;
    default: return xi;
    }
    return ov_expr8(v);
}

// the mask sample after "x opacity *" (opacity < 1 only)
__host__ __device__ inline int ov_mask(int m, float opacity) {
#pragma clang fp contract(off)
    return opacity < 1.f ? ov_expr8((float)m * opacity) : m;
}

// std.MaskedMerge, 8 bit (the stand-in tiles.hip uses)
__host__ __device__ inline int ov_merge(int base, int o, int m) { return (base * (255 - m) + o * m + 127) / 255; }
