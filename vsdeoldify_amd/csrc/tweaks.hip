// HBM-bound u8 per-pixel filters of SURVEY.md §8 a17 / a19: image_tweak (Pillow ImageEnhance chain + hue shift + hue-range
// mask), the Y look-up table of luma_adjusted_levels, restore_color_gradient (ChromaRetentionMerge).  Interleaved RGB in
// HBM, one thread per pixel, everything in registers.  Arithmetic restates Pillow's C (libImaging Convert.c / Blend.c:
// float locals, double intermediates, truncating casts) and OpenCV's 8-bit HSV integer path; see oracle/tweaks.py,
// oracle/cvcolor.py.  Built with -ffp-contract=off: Pillow's / numpy's products are rounded before the add.
#include "kernels.h"

#pragma clang fp contract(off)
#include "pixel_ops.h"

static inline int grid_for_px(int64_t work) {
    int64_t b = (work + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 16384 ? 16384 : b));
}

// ---- image_tweak (imfilters.py:463-504) ----
// SUM_L: stop in front of the contrast step and accumulate the Pillow-L sum of the intermediate image (ImageEnhance.Contrast
// needs its mean); otherwise the whole chain.
template <bool SUM_L>
__global__ void image_tweak_kernel(const uint8_t* __restrict__ img, uint8_t* __restrict__ out, int64_t npix, TweakArgs a,
                                   unsigned long long* __restrict__ sum) {
    unsigned long long local = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
        const int r0 = img[i * 3], g0 = img[i * 3 + 1], b0 = img[i * 3 + 2];
        int r = r0, g = g0, b = b0;
        image_tweak_head(a, r, g, b);
        if (SUM_L) { local += (unsigned)pil_L(r, g, b); continue; }
        image_tweak_tail(a, r0, g0, b0, r, g, b);
        out[i * 3] = (uint8_t)r; out[i * 3 + 1] = (uint8_t)g; out[i * 3 + 2] = (uint8_t)b;
    }
    if (SUM_L) {
        for (int o = 32; o > 0; o >>= 1) local += __shfl_down(local, o);
        if ((threadIdx.x & 63) == 0 && local) atomicAdd(sum, local);
    }
}

int launch_image_tweak(const uint8_t* img, uint8_t* out, int64_t npix, const TweakArgs& a, unsigned long long* d_sum, bool sum_only,
                       hipStream_t s) {
    if (sum_only) {
        hipError_t e = hipMemsetAsync(d_sum, 0, sizeof(unsigned long long), s);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL((image_tweak_kernel<true>), dim3(grid_for_px(npix)), dim3(256), 0, s, img, out, npix, a, d_sum);
    } else {
        hipLaunchKernelGGL((image_tweak_kernel<false>), dim3(grid_for_px(npix)), dim3(256), 0, s, img, out, npix, a, d_sum);
    }
    return (int)hipGetLastError();
}

// ---- luma_adjusted_levels (imfilters.py:335-372): cv2 YUV, Y through a 256-entry table, back ----
__device__ __forceinline__ int descale14t(int x) { return (x + (1 << 13)) >> 14; }
__global__ void luma_lut_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ lut, uint8_t* __restrict__ out, int64_t npix) {
    __shared__ uint8_t sl[256];
    sl[threadIdx.x & 255] = lut[threadIdx.x & 255];
    __syncthreads();
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
        const int r = img[i * 3], g = img[i * 3 + 1], b = img[i * 3 + 2];
        int y = descale14t(r * 4899 + g * 9617 + b * 1868);
        const int u = clip8i(descale14t((b - y) * 8061 + (128 << 14))) - 128;
        const int v = clip8i(descale14t((r - y) * 14369 + (128 << 14))) - 128;
        y = sl[clip8i(y)];
        out[i * 3] = (uint8_t)clip8i(y + descale14t(v * 18678));
        out[i * 3 + 1] = (uint8_t)clip8i(y + descale14t(u * -6472 + v * -9519));
        out[i * 3 + 2] = (uint8_t)clip8i(y + descale14t(u * 33292));
    }
}
int launch_luma_lut(const uint8_t* img, const uint8_t* d_lut, uint8_t* out, int64_t npix, hipStream_t s) {
    hipLaunchKernelGGL(luma_lut_kernel, dim3(grid_for_px(npix)), dim3(256), 0, s, img, d_lut, out, npix);
    return (int)hipGetLastError();
}

// ---- restore_color_gradient (restcolor.py:98-217): one frame; the pixel is pixel_ops.h's restore_gradient_pixel, shared with recover.hip ----
__global__ void restore_color_gradient_kernel(const uint8_t* __restrict__ color, const uint8_t* __restrict__ gray, uint8_t* __restrict__ out,
                                              int64_t npix, double sat, int tht, double alpha, double weight, int algo, int return_mask) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
        int o[3];
        restore_gradient_pixel(color[i * 3], color[i * 3 + 1], color[i * 3 + 2], gray[i * 3], gray[i * 3 + 1], gray[i * 3 + 2], sat, tht, alpha, weight, algo,
                               return_mask, o);
        out[i * 3] = (uint8_t)o[0]; out[i * 3 + 1] = (uint8_t)o[1]; out[i * 3 + 2] = (uint8_t)o[2];
    }
}
int launch_restore_color_gradient(const uint8_t* color, const uint8_t* gray, uint8_t* out, int64_t npix, double sat, int tht, double alpha,
                                  double weight, int algo, int return_mask, hipStream_t s) {
    hipLaunchKernelGGL(restore_color_gradient_kernel, dim3(grid_for_px(npix)), dim3(256), 0, s, color, gray, out, npix, sat, tht, alpha, weight,
                       algo, return_mask);
    return (int)hipGetLastError();
}

// ---- image_chroma_tweak (imfilters.py:540-548 -> restcolor.py:288-350): cv2 HSV hue / saturation / value tweak, then the optional
// "hue_adjust" stage (hue range on the TWEAKED hue -> re-tweaked colour, everything else the ORIGINAL pixel, weighted merges) ----
__global__ void chroma_tweak_kernel(const uint8_t* __restrict__ img, uint8_t* __restrict__ out, int64_t npix, ChromaTweakArgs a) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
        const int r0 = img[i * 3], g0 = img[i * 3 + 1], b0 = img[i * 3 + 2];
        int r, g, b;
        chroma_tweak_pixel(a, r0, g0, b0, r, g, b);
        out[i * 3] = (uint8_t)r; out[i * 3 + 1] = (uint8_t)g; out[i * 3 + 2] = (uint8_t)b;
    }
}
int launch_chroma_tweak(const uint8_t* img, uint8_t* out, int64_t npix, const ChromaTweakArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(chroma_tweak_kernel, dim3(grid_for_px(npix)), dim3(256), 0, s, img, out, npix, a);
    return (int)hipGetLastError();
}

// Eager module load (havc_create, under the library's set-up mutex): the HIP runtime loads a translation unit's code object on the first use
// of one of its kernels; querying one here moves that -- and the big-LDS opt-ins below -- out of the first launch, which may come from
// several host threads at once ("set-up is serialised").
void preload_tweaks() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(chroma_tweak_kernel)); (void)hipGetLastError(); }
