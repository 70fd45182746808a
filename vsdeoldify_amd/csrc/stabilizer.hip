// HAVC_stabilizer's per-pixel filter chain in one launch (vsdeoldify/__init__.py:2850-2860): vs_dark_tweak -> vs_chroma_bright_tweak -> vs_colormap
// (vsslib/vsfilters.py:525-641) are image_tweak / image_chroma_tweak followed by a luma-masked merge with the stage's input -- five launches and ten
// passes over the clip through the stand-alone kernels.  Here a thread reads four pixels (three dwords) once, runs up to three stages in registers and
// writes once.  The arithmetic is pixel_ops.h's, the very functions the stand-alone kernels call: same bytes.  No LDS, no scratch.
// Built with -ffp-contract=off like tweaks.hip / colorfilters.hip.
#include "kernels.h"

#pragma clang fp contract(off)
#include "pixel_ops.h"

__device__ __forceinline__ void stab_chain_pixel(const StabChainArgs& c, int& r, int& g, int& b) {
    for (int s = 0; s < c.n; ++s) {
        const StabStage& st = c.st[s];
        const int r0 = r, g0 = g, b0 = b;
        int tr = r0, tg = g0, tb = b0;
        if (st.kind == 0) {
            image_tweak_head(st.tw, tr, tg, tb);
            image_tweak_tail(st.tw, r0, g0, b0, tr, tg, tb);
        } else if (!st.identity) {
            chroma_tweak_pixel(st.ct, r0, g0, b0, tr, tg, tb);
        }
        if (st.merge_mode >= 0) luma_merge_pixel(st.merge_mode, st.tresh, st.grad, tr, tg, tb, r0, g0, b0, r, g, b);
        else { r = tr; g = tg; b = tb; }
    }
}

// VEC: img / out are dword-aligned; a thread owns the 12 bytes of pixels 4i .. 4i + 3.  The four pixels go through ONE copy of the chain's code (the
// 96-bit group is rotated by a pixel per turn: the pixel in the low 24 bits is processed, the result enters at the top), so the kernel stays a few
// KB of instructions whatever the stage mix.  The last npix % 4 pixels -- and every pixel of an unaligned image (!VEC: a frame view at an odd offset)
// -- go byte by byte: nothing is read or written beyond npix * 3.
template <bool VEC>
__global__ void __launch_bounds__(256) stabilizer_chain_kernel(const uint8_t* img, uint8_t* out, int64_t npix, StabChainArgs c) {
    const int64_t ngroups = VEC ? (npix + 3) >> 2 : npix;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < ngroups; i += (int64_t)gridDim.x * blockDim.x) {
        if (VEC && i * 4 + 4 <= npix) {
            const uint32_t* p = reinterpret_cast<const uint32_t*>(img + i * 12);
            uint32_t w0 = p[0], w1 = p[1], w2 = p[2];
#pragma unroll 1
            for (int q = 0; q < 4; ++q) {
                int r = (int)(w0 & 255u), g = (int)((w0 >> 8) & 255u), b = (int)((w0 >> 16) & 255u);
                stab_chain_pixel(c, r, g, b);
                const uint32_t res = (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16);
                w0 = (w0 >> 24) | (w1 << 8);
                w1 = (w1 >> 24) | (w2 << 8);
                w2 = (w2 >> 24) | (res << 8);
            }
            uint32_t* o = reinterpret_cast<uint32_t*>(out + i * 12);
            o[0] = w0; o[1] = w1; o[2] = w2;
        } else {
            const int64_t j0 = VEC ? i * 4 : i, j1 = VEC ? npix : i + 1;
            for (int64_t j = j0; j < j1; ++j) {
                int r = img[j * 3], g = img[j * 3 + 1], b = img[j * 3 + 2];
                stab_chain_pixel(c, r, g, b);
                out[j * 3] = (uint8_t)r; out[j * 3 + 1] = (uint8_t)g; out[j * 3 + 2] = (uint8_t)b;
            }
        }
    }
}

int launch_stabilizer_chain(const uint8_t* img, uint8_t* out, int64_t npix, const StabChainArgs& a, hipStream_t s) {
    const bool vec = ((reinterpret_cast<uintptr_t>(img) | reinterpret_cast<uintptr_t>(out)) & 3) == 0;
    const int64_t blocks = ((vec ? (npix + 3) >> 2 : npix) + 255) / 256;
    const dim3 grid((unsigned)(blocks < 1 ? 1 : (blocks > 16384 ? 16384 : blocks)));
    if (vec) hipLaunchKernelGGL((stabilizer_chain_kernel<true>), grid, dim3(256), 0, s, img, out, npix, a);
    else hipLaunchKernelGGL((stabilizer_chain_kernel<false>), grid, dim3(256), 0, s, img, out, npix, a);
    return (int)hipGetLastError();
}

// Eager module load (havc_create, under the library's set-up mutex), like every other translation unit ("set-up is serialised").
void preload_stabilizer() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(stabilizer_chain_kernel<true>)); (void)hipGetLastError(); }
