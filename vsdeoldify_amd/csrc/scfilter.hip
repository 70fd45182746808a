// The pixel work of the reference's SSIM / histogram scene filter (vsslib/vsscdect.py:352-495, SceneDetectFilter): of every candidate frame it takes
//     cv2.calcHist of the gray plane, 256 bins                                          -> scene_hist_kernel: exact integer counts
//     skimage.metrics.structural_similarity(gray, gray of the last accepted frame)      -> scene_ssim_kernel + scene_ssim_finish_kernel: one float64
// with gray = cv2's Y = (4899 R + 9617 G + 1868 B + 8192) >> 14 (scfilter_ops.h: COLOR_RGB2GRAY and the Y of COLOR_RGB2YUV are this one expression).  Both
// kernels read the small RGB clip u8 [n][h][w][3] in place and take their frames from index lists: no gray plane is stored, so memory does not grow with
// the number of candidates, and one launch serves every candidate of a clip.
//
// Histogram: blocks_per_frame blocks per listed frame, a thread owns four neighbouring pixels = 12 bytes at any byte alignment (as scdetect.hip).  Every
// wave counts into a histogram of its own in LDS (LDS integer atomics: a flat frame sends all 64 lanes to one bin, which serialises but cannot lose a
// count), the four are added and the non-zero bins go to the frame's row of the output with one 32-bit global atomic each.
//
// SSIM: a block owns a 32 x 32 tile of window positions of one frame pair.  The 38 x 38 gray values under it of both frames go to LDS, then the
// separable 7-tap sums: horizontally into LDS (x and y packed into one word, x^2, y^2, x * y one word each: a row sum is below 2^19), vertically in registers,
// four positions of a column per thread.  49 * 255^2 < 2^22: every window sum is an exact 32-bit integer.  The quotient of a position is float64
// (scf_ssim_value).  Reduction: wave shuffle tree -> four wave sums in LDS, added by thread 0 -> one float64 partial per block; scene_ssim_finish_kernel adds a
// pair's partials in a fixed order (lane l takes tiles l, l + 64, ..., then the same tree) and divides by the number of positions.  No floating-point atomic
// anywhere: the same input gives the same bits on every run, and a pair's value does not depend on what else is in the launch.
#include "kernels.h"
#include "scfilter_ops.h"

constexpr int SCF_IN = SCF_SSIM_TILE + 6;        // gray rows / columns under a tile of window positions
constexpr int SCF_PITCH = SCF_IN + 2;            // 40: rows of the gray tiles start on a dword

static_assert(SCF_SSIM_TILE == 32, "scene_ssim_kernel: 256 threads = 32 columns x 8 groups of 4 rows");

__device__ __forceinline__ double scf_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// out: k rows of 256 counters, ZERO-FILLED by the caller in front of the launch (on the same stream); idx: k frame numbers, each checked by the caller
__global__ void __launch_bounds__(256) scene_hist_kernel(const uint8_t* __restrict__ clip, const int* __restrict__ idx, unsigned* out, int64_t npix,
                                                         int blocks_per_frame) {
    __shared__ unsigned hist[4][256];
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) hist[k][t] = 0u;
    __syncthreads();
    const int j = (int)(blockIdx.x / (unsigned)blocks_per_frame), chunk = (int)(blockIdx.x % (unsigned)blocks_per_frame);
    const uint8_t* cur = clip + (int64_t)idx[j] * npix * 3;
    unsigned* mine = hist[t >> 6];
    const int64_t ngroups = (npix + 3) >> 2, stride = (int64_t)blocks_per_frame * 256;
    for (int64_t i = (int64_t)chunk * 256 + t; i < ngroups; i += stride) {
        if (i * 4 + 4 <= npix) {
            uint32_t w[3];
            int y[4];
            __builtin_memcpy(w, cur + i * 12, 12);
            scf_gray4(w, y);
#pragma unroll
            for (int q = 0; q < 4; ++q) atomicAdd(&mine[y[q]], 1u);
        } else {
            for (int64_t px = i * 4; px < npix; ++px) atomicAdd(&mine[scf_gray(cur[px * 3], cur[px * 3 + 1], cur[px * 3 + 2])], 1u);
        }
    }
    __syncthreads();
    const unsigned v = hist[0][t] + hist[1][t] + hist[2][t] + hist[3][t];
    if (v) atomicAdd(&out[(int64_t)j * 256 + t], v);
}

// partial: one float64 per block = the sum of S over the tile's positions inside the (h - 6) x (w - 6) valid range.  Block b works on pair b / tiles,
// tile b % tiles (row-major, tiles = tiles_x * tiles_y).
__global__ void __launch_bounds__(256) scene_ssim_kernel(const uint8_t* __restrict__ clip, const int* __restrict__ pairs, double* __restrict__ partial,
                                                         int h, int w, int tiles_x, int tiles_y) {
    __shared__ uint8_t ga[SCF_IN][SCF_PITCH], gb[SCF_IN][SCF_PITCH];
    __shared__ unsigned hs[4][SCF_IN][SCF_SSIM_TILE];          // 0: sum x | sum y << 16, 1: sum x^2, 2: sum y^2, 3: sum x * y -- over 7 columns
    __shared__ double red[4];
    const int t = threadIdx.x;
    const unsigned tiles = (unsigned)tiles_x * (unsigned)tiles_y;
    const int p = (int)(blockIdx.x / tiles), tile = (int)(blockIdx.x % tiles);
    const int y0 = (tile / tiles_x) * SCF_SSIM_TILE, x0 = (tile % tiles_x) * SCF_SSIM_TILE;
    const int64_t fb = (int64_t)h * w * 3;
    const uint8_t* fa = clip + (int64_t)pairs[2 * p] * fb;
    const uint8_t* fq = clip + (int64_t)pairs[2 * p + 1] * fb;
    // gray of both frames under the tile; outside the frame (only under positions that are masked below): 0, nothing is read there
    for (int i = t; i < SCF_IN * SCF_IN; i += 256) {
        const int r = i / SCF_IN, c = i - r * SCF_IN;
        const int y = y0 + r, x = x0 + c;
        int va = 0, vb = 0;
        if (y < h && x < w) {
            const int64_t o = ((int64_t)y * w + x) * 3;
            va = scf_gray(fa[o], fa[o + 1], fa[o + 2]);
            vb = scf_gray(fq[o], fq[o + 1], fq[o + 2]);
        }
        ga[r][c] = (uint8_t)va;
        gb[r][c] = (uint8_t)vb;
    }
    __syncthreads();
    for (int i = t; i < SCF_IN * SCF_SSIM_TILE; i += 256) {
        const int r = i >> 5, c = i & 31;
        unsigned sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const unsigned a = ga[r][c + k], b = gb[r][c + k];
            sx += a; sy += b; sxx += a * a; syy += b * b; sxy += a * b;
        }
        hs[0][r][c] = sx | (sy << 16);
        hs[1][r][c] = sxx;
        hs[2][r][c] = syy;
        hs[3][r][c] = sxy;
    }
    __syncthreads();
    const int c = t & 31, r0 = (t >> 5) * 4;
    unsigned row[4][10];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int k = 0; k < 10; ++k) row[q][k] = hs[q][r0 + k][c];
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned s[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int k = 0; k < 7; ++k) s[q] += row[q][j + k];
        // 7 * 1785 = 12495 < 2^16: the packed halves did not carry into each other
        const double v = scf_ssim_value((int)(s[0] & 0xFFFFu), (int)(s[0] >> 16), (int)s[1], (int)s[2], (int)s[3]);
        if (y0 + r0 + j <= h - 7 && x0 + c <= w - 7) acc += v;
    }
    acc = scf_wave_sum(acc);
    if ((t & 63) == 0) red[t >> 6] = acc;
    __syncthreads();
    if (t == 0) partial[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one wave per pair
__global__ void __launch_bounds__(64) scene_ssim_finish_kernel(const double* __restrict__ partial, double* __restrict__ out, int tiles, double count) {
    const double* mine = partial + (int64_t)blockIdx.x * tiles;
    double acc = 0.0;
    for (int i = threadIdx.x; i < tiles; i += 64) acc += mine[i];
    acc = scf_wave_sum(acc);
    if (threadIdx.x == 0) out[blockIdx.x] = acc / count;
}

int scene_hist_blocks_per_frame(int64_t npix) {
    // 32 pixels per thread and at most 64 blocks per frame: a block ends in up to 256 global atomics on its frame's 1 KiB row
    const int64_t b = (((npix + 3) >> 2) + 2047) / 2048;
    return (int)(b < 1 ? 1 : (b > 64 ? 64 : b));
}

int scene_ssim_tiles(int h, int w, int* tiles_x, int* tiles_y) {
    const int tx = (w - 6 + SCF_SSIM_TILE - 1) / SCF_SSIM_TILE, ty = (h - 6 + SCF_SSIM_TILE - 1) / SCF_SSIM_TILE;
    if (tiles_x) *tiles_x = tx;
    if (tiles_y) *tiles_y = ty;
    return tx * ty;
}

int launch_scene_hist(const uint8_t* clip, const int* idx, int k, unsigned* out, int h, int w, hipStream_t s) {
    const int64_t npix = (int64_t)h * w;
    if (k <= 0 || npix <= 0 || npix > ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
    const int bpf = scene_hist_blocks_per_frame(npix);
    const int64_t blocks = (int64_t)k * bpf;
    if (blocks > 0x7FFFFFFFll) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(scene_hist_kernel, dim3((unsigned)blocks), dim3(256), 0, s, clip, idx, out, npix, bpf);
    return (int)hipGetLastError();
}

int launch_scene_ssim(const uint8_t* clip, const int* pairs, int m, double* partial, double* out, int h, int w, hipStream_t s) {
    if (m <= 0 || h < 7 || w < 7 || (int64_t)h * w > ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
    int tx, ty;
    const int tiles = scene_ssim_tiles(h, w, &tx, &ty);
    const int64_t blocks = (int64_t)m * tiles;
    if (blocks > 0x7FFFFFFFll) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(scene_ssim_kernel, dim3((unsigned)blocks), dim3(256), 0, s, clip, pairs, partial, h, w, tx, ty);
    hipLaunchKernelGGL(scene_ssim_finish_kernel, dim3((unsigned)m), dim3(64), 0, s, (const double*)partial, out, tiles,
                       (double)((int64_t)(h - 6) * (w - 6)));
    return (int)hipGetLastError();
}

void preload_scfilter() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(scene_ssim_kernel)); (void)hipGetLastError(); }
