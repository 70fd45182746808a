// Arithmetic of havc_lut3d_clip shared by the kernel (lut3d.hip) and the host: the stand-in of the timecube.Cube plugin, trilinear interpolation in a 3D
// table.  tests/timecube_util.py is the definition; every float32 expression here is that file's sequence, one rounding per operation, never fused.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

#define LUT3D_MIN_SIZE 2
#define LUT3D_MAX_SIZE 256

struct Lut3dPoint { float r, g, b, pad; };       // a lattice point padded to one aligned 16-byte load

__host__ __device__ inline float lut3d_lerp(float a, float b, float f) {
#pragma clang fp contract(off)
    return a + (b - a) * f;
}

// the eight points around a cell (c[k]: bit 0 = red + 1, bit 1 = green + 1, bit 2 = blue + 1) -> one channel: 4 lerps along red, 2 along green, 1 along blue
__host__ __device__ inline float lut3d_cell(const float c[8], float fr, float fg, float fb) {
    const float r0 = lut3d_lerp(c[0], c[1], fr), r1 = lut3d_lerp(c[2], c[3], fr), r2 = lut3d_lerp(c[4], c[5], fr), r3 = lut3d_lerp(c[6], c[7], fr);
    return lut3d_lerp(lut3d_lerp(r0, r1, fg), lut3d_lerp(r2, r3, fg), fb);
}

// v -> min(max(v, 0), 1) * 255, rounded half to even
__host__ __device__ inline int lut3d_quant(float v) {
#pragma clang fp contract(off)
    return (int)rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.f);
}
