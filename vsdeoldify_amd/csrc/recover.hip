// HAVC_recover_clip_color = ChromaRetentionMerge (vsdeoldify/__init__.py:2956-2992 -> vsslib/mcomb.py:450-516) on a whole clip: the two per-frame selectors
// of the reference -- vs_sc_recover_gradient_color (vsslib/vsfilters.py:391-412 -> restcolor.restore_color_gradient, restcolor.py:98-134) and, with a binary
// mask, vs_sc_recover_clip_color (vsfilters.py:327-351 -> restcolor.restore_color, restcolor.py:38-83, tht_scen = 1.0, hue_adjust 'none') -- as TWO dependent
// launches over the clip [n][h][w][3], the second reading the first one's per-frame results from device memory (no host round trip):
//     1. sums[f] = sum of cv2's Y (pixel_ops.h rgb2yuv, what havc_image_luma sums) over frame f of `gray`
//     2. f_luma = round(sums[f] / npix / 255, 6) (equalize_ops.h eq_f_luma, range_tv = 0); outside DEF_STANDARD_DARK (0.22) <= f_luma <= DEF_STANDARD_BRIGHT
//        (0.78) the weight and alpha of the frame are overridden; then the per-pixel restore (pixel_ops.h: restore_gradient_pixel, the body of
//        havc_restore_color_gradient, or restore_binary_pixel)
// The binary selector hands frames with clip index first_frame + f < 15 on unchanged (`if n < 15`, in front of everything else, return_mask included): those
// frames are copied, and the first launch skips them.
//
// Access pattern (as tiles.hip / scdetect.hip): a thread owns four neighbouring pixels = 12 bytes, one 96-bit access at any byte alignment (frames whose pixel
// count is no multiple of four start at odd offsets); the last npix % 4 pixels of a frame go byte by byte.  Nothing is read or written beyond a frame.
// A frame is split over several blocks in both launches (a block works on one frame: its gate is block-uniform).  Reduction of the sums: registers -> wave
// (shuffles) -> block (LDS) -> one 64-bit integer atomic add per block into the frame's slot.  Integer sums do not depend on the order: bit-identical from
// run to run.  No scratch.
#include "kernels.h"

#pragma clang fp contract(off)
#include "pixel_ops.h"
#include "equalize_ops.h"

#define RECOVER_STANDARD_DARK 0.22       // vsslib/constants.py:28-29
#define RECOVER_STANDARD_BRIGHT 0.78
#define RECOVER_BINARY_FIRST 15          // vsfilters.py:339: `if n < 15: return f_out`

__device__ __forceinline__ bool recover_passthrough(const RecoverArgs& a, int f) { return a.binary_mask && (int64_t)a.first_frame + f < RECOVER_BINARY_FIRST; }

__device__ __forceinline__ unsigned recover_y(int r, int g, int b) {
    int y, u, v;
    rgb2yuv(r, g, b, y, u, v);
    return (unsigned)y;
}

// Grid: luma_blocks blocks for each frame, block b works on frame b / luma_blocks.  sums: n slots, zeroed on the same stream in front of the launch.
__global__ void __launch_bounds__(256) recover_luma_kernel(const uint8_t* __restrict__ gray, unsigned long long* sums, RecoverArgs a) {
    __shared__ unsigned red[4];
    const int f = (int)(blockIdx.x / (unsigned)a.luma_blocks), chunk = (int)(blockIdx.x % (unsigned)a.luma_blocks);
    if (recover_passthrough(a, f)) return;                                           // block-uniform
    const int64_t npix = (int64_t)a.h * a.w, ngroups = (npix + 3) >> 2;
    const uint8_t* src = gray + (int64_t)f * npix * 3;
    // a thread adds at most 1020 per turn and takes at most 2^14 groups of a frame of 2^31 pixels (luma_blocks = 128): a WAVE's 32-bit sum stays below
    // 1.1e9; the four wave sums are added in 64 bits
    unsigned acc = 0;
    for (int64_t i = (int64_t)chunk * blockDim.x + threadIdx.x; i < ngroups; i += (int64_t)a.luma_blocks * blockDim.x) {
        if (i * 4 + 4 <= npix) {
            int v[12];
            load12(src + i * 12, v);
#pragma unroll
            for (int q = 0; q < 4; ++q) acc += recover_y(v[q * 3], v[q * 3 + 1], v[q * 3 + 2]);
        } else {
            for (int64_t p = i * 4; p < npix; ++p) acc += recover_y(src[p * 3], src[p * 3 + 1], src[p * 3 + 2]);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int k = 0; k < 4; ++k) t += red[k];
        atomicAdd(sums + f, t);
    }
}

// one pixel of either path; weight / alpha are the frame's (after the gate)
__device__ __forceinline__ void recover_pixel(const RecoverArgs& a, double weight, double alpha, int cr, int cg, int cb, int gr, int gg, int gb, int o[3]) {
    if (a.binary_mask) restore_binary_pixel(cr, cg, cb, gr, gg, gb, a.sat, a.tht, weight, a.return_mask, o);
    else restore_gradient_pixel(cr, cg, cb, gr, gg, gb, a.sat, a.tht, alpha, weight, a.algo, a.return_mask, o);
}

// Grid: apply_blocks blocks for each frame.  Every byte of `out` inside n * h * w * 3 is written exactly once; nothing beyond.
__global__ void __launch_bounds__(256) recover_apply_kernel(const uint8_t* __restrict__ gray, const uint8_t* __restrict__ color, uint8_t* __restrict__ out,
                                                            const unsigned long long* __restrict__ sums, RecoverArgs a) {
    const int f = (int)(blockIdx.x / (unsigned)a.apply_blocks), chunk = (int)(blockIdx.x % (unsigned)a.apply_blocks);
    const int64_t npix = (int64_t)a.h * a.w, ngroups = (npix + 3) >> 2, base = (int64_t)f * npix * 3;
    const uint8_t *g = gray + base, *c = color + base;
    uint8_t* dst = out + base;
    const bool copy = recover_passthrough(a, f);
    double weight = a.weight, alpha = a.alpha;
    if (!copy) {
        const double f_luma = eq_f_luma(sums[f], npix, 0);
        if (!(RECOVER_STANDARD_DARK <= f_luma && f_luma <= RECOVER_STANDARD_BRIGHT)) {
            if (a.binary_mask) weight = fmin(weight, -0.8);                          // vsfilters.py:348-349
            else { weight = fmin(weight, -0.5); alpha = fmax(alpha, 4.0); }          // vsfilters.py:403-409
        }
    }
    for (int64_t i = (int64_t)chunk * blockDim.x + threadIdx.x; i < ngroups; i += (int64_t)a.apply_blocks * blockDim.x) {
        if (i * 4 + 4 <= npix) {
            int vg[12], vc[12], vo[12];
            load12(g + i * 12, vg);
            if (copy) { store12(dst + i * 12, vg); continue; }
            if (a.return_mask) {
#pragma unroll
                for (int k = 0; k < 12; ++k) vc[k] = 0;                              // the mask is made of the gray pixel alone
            } else {
                load12(c + i * 12, vc);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                int o[3];
                recover_pixel(a, weight, alpha, vc[q * 3], vc[q * 3 + 1], vc[q * 3 + 2], vg[q * 3], vg[q * 3 + 1], vg[q * 3 + 2], o);
                vo[q * 3] = o[0]; vo[q * 3 + 1] = o[1]; vo[q * 3 + 2] = o[2];
            }
            store12(dst + i * 12, vo);
        } else {
            for (int64_t p = i * 4; p < npix; ++p) {
                const int gr = g[p * 3], gg = g[p * 3 + 1], gb = g[p * 3 + 2];
                int o[3] = {gr, gg, gb};
                if (!copy) recover_pixel(a, weight, alpha, c[p * 3], c[p * 3 + 1], c[p * 3 + 2], gr, gg, gb, o);
                dst[p * 3] = (uint8_t)o[0]; dst[p * 3 + 1] = (uint8_t)o[1]; dst[p * 3 + 2] = (uint8_t)o[2];
            }
        }
    }
}

// sums: n slots of device memory.  All pointers are device pointers; out aliases neither input.
int launch_recover_color(const uint8_t* gray, const uint8_t* color, uint8_t* out, unsigned long long* sums, RecoverArgs a, hipStream_t s) {
    const int64_t npix = (int64_t)a.h * a.w;
    if (a.n <= 0 || npix <= 0 || npix > ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
    const int64_t ngroups = (npix + 3) >> 2;
    // sums: eight groups per thread, at most 128 blocks per frame -- every block ends in an atomic on its frame's slot (scdetect.hip measured the limit)
    int64_t lb = (ngroups + 2047) / 2048;
    a.luma_blocks = (int)(lb < 1 ? 1 : (lb > 128 ? 128 : lb));
    // apply: one group per thread up to 4096 blocks per frame, then a stride loop
    int64_t ab = (ngroups + 255) / 256;
    a.apply_blocks = (int)(ab < 1 ? 1 : (ab > 4096 ? 4096 : ab));
    if ((int64_t)a.n * a.apply_blocks > 0x7FFFFFFFll) return (int)hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(sums, 0, (size_t)a.n * sizeof(unsigned long long), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(recover_luma_kernel, dim3((unsigned)((int64_t)a.n * a.luma_blocks)), dim3(256), 0, s, gray, sums, a);
    hipLaunchKernelGGL(recover_apply_kernel, dim3((unsigned)((int64_t)a.n * a.apply_blocks)), dim3(256), 0, s, gray, color, out, sums, a);
    return (int)hipGetLastError();
}

// Eager module load (havc_create, under the library's set-up mutex), like every other translation unit ("set-up is serialised").
void preload_recover() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(recover_apply_kernel)); (void)hipGetLastError(); }
