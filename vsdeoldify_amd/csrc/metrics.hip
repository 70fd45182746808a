// havc_delta_e_clip: per-pixel CIEDE2000 between two RGB24 clips [n][h][w][3] in HBM, in float64 -- the project's parity metric (oracle/imaging.py
// delta_e00_images) as one pass over the pixels.  metrics_ops.h has the arithmetic.
//     delta_e_kernel   grid (blocks of a frame, frames): a block never straddles frames.  A thread owns four pixels of each clip = 12 bytes = three dwords and
//                      walks them one after the other (the pixel function is some hundred float64 operations and a dozen library calls: four copies of it in
//                      flight would only cost registers; the kernel is ALU-bound and lives on occupancy).  The 256-entry sRGB -> linear table sits in LDS
//                      (2 KiB).  Per frame, all of it independent of the order the blocks run in:
//                        hist   LDS counters (4 KiB), flushed with global integer atomics;
//                        max    integer max on the bit pattern of the non-negative double;
//                        sse    exact integer sums of squared byte differences;
//                        sum    a thread adds its pixels in pixel order, the block adds its threads in a fixed tree, and the block's sum goes to
//                               partials[frame][block];
//     delta_e_sum_kernel   one thread per frame adds the partials in block order: the sum has the same bits every run.
#include "kernels.h"
#include "metrics_ops.h"

#define DE_THREADS 256
static_assert(DE_THREADS * 4 == DE_BLOCK_PIXELS && DE_BINS == DE_HIST_BINS, "metrics.hip geometry");

__global__ void __launch_bounds__(DE_THREADS) delta_e_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, const double* __restrict__ lin_g,
                                                              DeRec* __restrict__ rec, double* __restrict__ partials, double* __restrict__ map, int64_t npix) {
    __shared__ double lin[256];
    __shared__ double red[DE_THREADS];
    __shared__ unsigned hist[DE_BINS];
    __shared__ unsigned sse[3];
    __shared__ unsigned long long smax;
    const int t = threadIdx.x, f = blockIdx.y;
    lin[t] = lin_g[t];
    for (int i = t; i < DE_BINS; i += DE_THREADS) hist[i] = 0;
    if (t < 3) sse[t] = 0;
    if (t == 0) smax = 0;
    __syncthreads();

    const int64_t p0 = ((int64_t)blockIdx.x * DE_THREADS + t) * 4;
    const int cnt = p0 >= npix ? 0 : (npix - p0 >= 4 ? 4 : (int)(npix - p0));          // the ragged end of a frame is masked
    const uint8_t* pa = a + ((int64_t)f * npix + p0) * 3;
    const uint8_t* pb = b + ((int64_t)f * npix + p0) * 3;
    // the pixels of a thread as 96 bits per clip: lo holds bytes 0..7, hi bytes 8..11; a pixel is taken from the bottom and the rest shifted down
    unsigned long long alo = 0, blo = 0;
    unsigned ahi = 0, bhi = 0;
    if (cnt == 4) {
        unsigned wa[3], wb[3];
        __builtin_memcpy(wa, pa, 12);
        __builtin_memcpy(wb, pb, 12);
        alo = wa[0] | ((unsigned long long)wa[1] << 32); ahi = wa[2];
        blo = wb[0] | ((unsigned long long)wb[1] << 32); bhi = wb[2];
    } else {
        for (int j = 0; j < cnt * 3; ++j) {                                            // at most 9 bytes: all of them in lo and the first of hi
            if (j < 8) { alo |= (unsigned long long)pa[j] << (8 * j); blo |= (unsigned long long)pb[j] << (8 * j); }
            else { ahi |= (unsigned)pa[j] << (8 * (j - 8)); bhi |= (unsigned)pb[j] << (8 * (j - 8)); }
        }
    }
    double sum = 0.0, mx = 0.0;
    unsigned s0 = 0, s1 = 0, s2 = 0;
    double* mp = map ? map + (int64_t)f * npix + p0 : nullptr;
#pragma unroll 1
    for (int k = 0; k < cnt; ++k) {
        const int ar = (int)(alo & 255), ag = (int)((alo >> 8) & 255), ab = (int)((alo >> 16) & 255);
        const int br = (int)(blo & 255), bg = (int)((blo >> 8) & 255), bb = (int)((blo >> 16) & 255);
        alo = (alo >> 24) | ((unsigned long long)ahi << 40); ahi >>= 24;
        blo = (blo >> 24) | ((unsigned long long)bhi << 40); bhi >>= 24;
        const double de = de_ciede2000(de_lab(lin[ar], lin[ag], lin[ab]), de_lab(lin[br], lin[bg], lin[bb]));
        sum += de;
        mx = de > mx ? de : mx;
        atomicAdd(&hist[de_bin(de)], 1u);
        s0 += (unsigned)((ar - br) * (ar - br)); s1 += (unsigned)((ag - bg) * (ag - bg)); s2 += (unsigned)((ab - bb) * (ab - bb));
        if (mp) mp[k] = de;
    }
    if (cnt) {
        if (s0) atomicAdd(&sse[0], s0);
        if (s1) atomicAdd(&sse[1], s1);
        if (s2) atomicAdd(&sse[2], s2);
        if (mx > 0.0) atomicMax(&smax, (unsigned long long)__double_as_longlong(mx));
    }
    red[t] = sum;
    __syncthreads();
    for (int s = DE_THREADS / 2; s > 0; s >>= 1) {                                      // the fixed tree: red[t] += red[t + s], s = 128, 64, .. 1
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    DeRec* r = rec + f;
    if (t == 0) {
        partials[(int64_t)f * gridDim.x + blockIdx.x] = red[0];
        if (smax) atomicMax(&r->max_bits, smax);
    }
    if (t < 3 && sse[t]) atomicAdd(&r->sse[t], (unsigned long long)sse[t]);
    for (int i = t; i < DE_BINS; i += DE_THREADS)
        if (hist[i]) atomicAdd(&r->hist[i], hist[i]);
}

__global__ void __launch_bounds__(DE_THREADS) delta_e_sum_kernel(const double* __restrict__ partials, DeRec* __restrict__ rec, int n, int64_t nblocks) {
    const int f = blockIdx.x * DE_THREADS + threadIdx.x;
    if (f >= n) return;
    const double* p = partials + (int64_t)f * nblocks;
    double s = 0.0;
    for (int64_t i = 0; i < nblocks; ++i) s += p[i];
    rec[f].sum = s;
}

int launch_delta_e(const uint8_t* a, const uint8_t* b, const double* lin, DeRec* rec, double* partials, double* map, int n, int64_t npix, hipStream_t s) {
    if (n <= 0 || n > 65535 || npix <= 0 || npix > ((int64_t)1 << 30)) return (int)hipErrorInvalidValue;
    const int64_t nb = delta_e_blocks(npix);
    hipLaunchKernelGGL(delta_e_kernel, dim3((unsigned)nb, (unsigned)n), dim3(DE_THREADS), 0, s, a, b, lin, rec, partials, map, npix);
    hipLaunchKernelGGL(delta_e_sum_kernel, dim3((unsigned)((n + DE_THREADS - 1) / DE_THREADS)), dim3(DE_THREADS), 0, s, partials, rec, n, nb);
    return (int)hipGetLastError();
}

void preload_metrics() { hipFuncAttributes at; (void)hipFuncGetAttributes(&at, reinterpret_cast<const void*>(delta_e_kernel)); (void)hipGetLastError(); }
