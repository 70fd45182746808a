// HAVC_clip_overlay (vsdeoldify/__init__.py:3029-3148) on RGB24 clips in HBM: the overlay [n or 1][oh][ow][3], placed at (x, y) of the base [n][bh][bw][3],
// blended by one of nine modes and merged through an optional mask and an opacity.  std.Crop / std.AddBorders / std.Expr / std.MaskedMerge are native
// VapourSynth: a stand-in with one written definition, tests/overlay_util.py, which this kernel equals byte for byte (overlay_ops.h has the arithmetic; this file
// is built with -ffp-contract=off and without fast-math: the divisions stay IEEE).
//     overlay_kernel   one launch.  The reference crops the overlay and pads it with borders whose mask is 0; here nothing is cropped or padded: a thread owns
//                      four consecutive pixels of the base = 12 bytes = three dwords, and a pixel outside the placed rectangle keeps the base's bytes.
#include "kernels.h"
#include "overlay_ops.h"

#define OV_THREADS 256

__device__ __forceinline__ void overlay_pixel(uint8_t* px, int64_t p, const uint8_t* __restrict__ ov, const uint8_t* __restrict__ mask, const OverlayArgs& a) {
    const int64_t fpix = (int64_t)a.bw * a.bh;
    const int f = (int)(p / fpix);
    const int rem = (int)(p - (int64_t)f * fpix);
    const int yy = rem / a.bw, xx = rem - yy * a.bw;
    const int oy = yy - a.y, ox = xx - a.x;
    if (ox < 0 || ox >= a.ow || oy < 0 || oy >= a.oh) return;
    const int64_t o = ((int64_t)(a.overlay_frames == 1 ? 0 : f) * a.oh + oy) * a.ow + ox;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (!((a.plane_mask >> k) & 1)) continue;
        int m = 255;
        if (a.mask_planes == 1) m = mask[o];
        else if (a.mask_planes == 3) m = mask[o * 3 + (a.first_plane ? 0 : k)];
        m = ov_mask(m, a.opacity);
        px[k] = (uint8_t)ov_merge(px[k], ov_blend(a.mode, ov[o * 3 + k], px[k]), m);
    }
}

__global__ void __launch_bounds__(OV_THREADS) overlay_kernel(const uint8_t* __restrict__ base, const uint8_t* __restrict__ ov, const uint8_t* __restrict__ mask,
                                                            uint8_t* __restrict__ dst, OverlayArgs a) {
    const int64_t npix = (int64_t)a.n * a.bw * a.bh, ngroups = (npix + 3) >> 2;
    for (int64_t i = (int64_t)blockIdx.x * OV_THREADS + threadIdx.x; i < ngroups; i += (int64_t)gridDim.x * OV_THREADS) {
        if (i * 4 + 4 <= npix) {
            uint8_t b[12];
            __builtin_memcpy(b, base + i * 12, 12);
#pragma unroll
            for (int k = 0; k < 4; ++k) overlay_pixel(b + 3 * k, i * 4 + k, ov, mask, a);
            __builtin_memcpy(dst + i * 12, b, 12);
        } else {
            for (int64_t p = i * 4; p < npix; ++p) {
                uint8_t b[3] = {base[p * 3], base[p * 3 + 1], base[p * 3 + 2]};
                overlay_pixel(b, p, ov, mask, a);
                dst[p * 3] = b[0]; dst[p * 3 + 1] = b[1]; dst[p * 3 + 2] = b[2];
            }
        }
    }
}

int launch_overlay(const uint8_t* base, const uint8_t* ov, const uint8_t* mask, uint8_t* dst, OverlayArgs a, hipStream_t s) {
    if (a.n <= 0 || a.bw <= 0 || a.bh <= 0 || a.ow <= 0 || a.oh <= 0 || a.mode < 0 || a.mode >= OV_MODES || (a.mask_planes != 0 && a.mask_planes != 1 && a.mask_planes != 3) ||
        (a.mask_planes != 0) != (mask != nullptr) || (a.overlay_frames != 1 && a.overlay_frames != a.n))
        return (int)hipErrorInvalidValue;
    const int64_t groups = (((int64_t)a.n * a.bw * a.bh) + 3) >> 2, want = (groups + OV_THREADS - 1) / OV_THREADS;
    const unsigned blocks = (unsigned)(want < 1 ? 1 : (want > 16384 ? 16384 : want));
    hipLaunchKernelGGL(overlay_kernel, dim3(blocks), dim3(OV_THREADS), 0, s, base, ov, mask, dst, a);
    return (int)hipGetLastError();
}

void preload_overlay() { hipFuncAttributes at; (void)hipFuncGetAttributes(&at, reinterpret_cast<const void*>(overlay_kernel)); (void)hipGetLastError(); }
