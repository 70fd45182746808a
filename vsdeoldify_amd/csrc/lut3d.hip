// HAVC_TimeCube's 3D LUT (vsdeoldify/__init__.py:2995-3026 -> vs_timecube_load, vsslib/vsplugins.py:283-323 -> the timecube.Cube plugin) on a clip [n][h][w][3]
// in HBM.  The plugin cannot be executed where the fixtures are made: trilinear interpolation with one written definition, tests/timecube_util.py, which this
// kernel equals byte for byte (lut3d_ops.h has the arithmetic; this file is built with -ffp-contract=off: a fused a + (b - a) * f changes the bytes).
//     lut3d_pad_kernel     the caller's table [size^3][3] -> [size^3] points of 16 bytes in the scratch slot: a corner is ONE aligned 16-byte load
//     lut3d_apply_kernel   the input is 8 bit, so cell and fraction depend on the sample alone: the six 256-entry axis tables (the host's: havc_lut3d_clip) sit
//                          in LDS, the table stays in global memory (33^3 points are 575 KB, 65^3 4.4 MB: neither fits LDS, both fit or nearly fit an XCD's
//                          L2).  A thread owns four pixels = 12 bytes = three dwords, as lut3_apply_kernel (tweak.hip); the eight corners of a pixel are loaded
//                          unconditionally, so all of them are in flight together.  The interpolation is per pixel and knows no frame: the clip is one run of
//                          n * h * w pixels.
#include "kernels.h"
#include "lut3d_ops.h"

#define LUT3D_THREADS 256

__global__ void __launch_bounds__(LUT3D_THREADS) lut3d_pad_kernel(const float* __restrict__ table, Lut3dPoint* __restrict__ points, int npoints) {
    const int i = blockIdx.x * LUT3D_THREADS + threadIdx.x;
    if (i < npoints) points[i] = Lut3dPoint{table[3 * (int64_t)i], table[3 * (int64_t)i + 1], table[3 * (int64_t)i + 2], 0.f};
}

__device__ __forceinline__ void lut3d_pixel(const float4* __restrict__ points, int N, const int (*cell)[256], const float (*frac)[256], uint8_t* px) {
    const int r = px[0], g = px[1], b = px[2];
    const float4* p = points + ((int64_t)cell[2][b] * N + cell[1][g]) * N + cell[0][r];
    float4 c[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) c[k] = p[((k >> 2) * N + ((k >> 1) & 1)) * N + (k & 1)];
    const float fr = frac[0][r], fg = frac[1][g], fb = frac[2][b];
    float ch[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) ch[k] = c[k].x;
    px[0] = (uint8_t)lut3d_quant(lut3d_cell(ch, fr, fg, fb));
#pragma unroll
    for (int k = 0; k < 8; ++k) ch[k] = c[k].y;
    px[1] = (uint8_t)lut3d_quant(lut3d_cell(ch, fr, fg, fb));
#pragma unroll
    for (int k = 0; k < 8; ++k) ch[k] = c[k].z;
    px[2] = (uint8_t)lut3d_quant(lut3d_cell(ch, fr, fg, fb));
}

// idx / frac: [3][256] in device memory.  A cell outside 0 .. size - 2 would read outside the table: it is clamped here, whatever the caller wrote.
__global__ void __launch_bounds__(LUT3D_THREADS) lut3d_apply_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const float4* __restrict__ points,
                                                                   const int* __restrict__ idx, const float* __restrict__ fr, Lut3dArgs a) {
    __shared__ int cell[3][256];
    __shared__ float frac[3][256];
    const int t = threadIdx.x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        cell[c][t] = min(max(idx[c * 256 + t], 0), a.size - 2);
        frac[c][t] = fr[c * 256 + t];
    }
    __syncthreads();
    const int64_t npix = a.npix, ngroups = (npix + 3) >> 2;
    for (int64_t i = (int64_t)blockIdx.x * LUT3D_THREADS + t; i < ngroups; i += (int64_t)gridDim.x * LUT3D_THREADS) {
        if (i * 4 + 4 <= npix) {
            uint8_t b[12];
            __builtin_memcpy(b, src + i * 12, 12);
#pragma unroll
            for (int k = 0; k < 4; ++k) lut3d_pixel(points, a.size, cell, frac, b + 3 * k);
            __builtin_memcpy(dst + i * 12, b, 12);
        } else {
            for (int64_t p = i * 4; p < npix; ++p) {
                uint8_t b[3] = {src[p * 3], src[p * 3 + 1], src[p * 3 + 2]};
                lut3d_pixel(points, a.size, cell, frac, b);
                dst[p * 3] = b[0]; dst[p * 3 + 1] = b[1]; dst[p * 3 + 2] = b[2];
            }
        }
    }
}

int launch_lut3d(const uint8_t* src, uint8_t* dst, const float* table, void* points, const int* idx, const float* frac, Lut3dArgs a, hipStream_t s) {
    if (a.npix <= 0 || a.size < LUT3D_MIN_SIZE || a.size > LUT3D_MAX_SIZE) return (int)hipErrorInvalidValue;
    const int npoints = a.size * a.size * a.size;
    hipLaunchKernelGGL(lut3d_pad_kernel, dim3((unsigned)((npoints + LUT3D_THREADS - 1) / LUT3D_THREADS)), dim3(LUT3D_THREADS), 0, s, table, (Lut3dPoint*)points, npoints);
    const int64_t groups = (a.npix + 3) >> 2, want = (groups + LUT3D_THREADS - 1) / LUT3D_THREADS;
    const unsigned blocks = (unsigned)(want < 1 ? 1 : (want > 8192 ? 8192 : want));
    hipLaunchKernelGGL(lut3d_apply_kernel, dim3(blocks), dim3(LUT3D_THREADS), 0, s, src, dst, (const float4*)points, idx, frac, a);
    return (int)hipGetLastError();
}

void preload_lut3d() { hipFuncAttributes at; (void)hipFuncGetAttributes(&at, reinterpret_cast<const void*>(lut3d_apply_kernel)); (void)hipGetLastError(); }
