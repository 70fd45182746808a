// HAVC_stabilizer(stab=True): vs_chroma_stabilizer_ex (vsslib/vsfilters.py:38-63, 84-157, 216-356) and vs_reduce_flicker on a clip [n][h][w][3] in HBM.
// VapourSynth, zimg and the ReduceFlicker plugin cannot be executed where the fixtures are made: tests/stab_util.py is THE DEFINITION of the stand-ins, these
// kernels (and tweak.hip's, which do the conversions) equal it byte for byte.  A chunk of frames goes through (rt_filters.cpp: havc_chroma_stab_clip)
//     stab_tables_kernel             the index tables of the chunk, on the device, from a handful of integers and the scene-change bit masks
//     tweak_forward_kernel           RGB24 -> Y, U, V of the chunk's source frames (tweak.hip)
//   tht > 0 (_average_clips_ex):
//     tweak_back_indexed_kernel      the N - 1 shifted clips: Y of frame n, U / V of frame m = clamp(n + d), error diffusion -> RGB24 (tweak.hip)
//     stab_stats_kernel              per frame of a shifted clip: the sum of cv2's Y and the count of pixels with cv2 S < tht, 64-bit integer atomics
//     tweak_forward_restore_kernel   restore_color on the fly, from those sums (luma band, tht_scen gate) -> U, V of the restored clips only (tweak.hip)
//   both:
//     stab_average_kernel            std.AverageFrames on U and V: clamp((sum w_i s_i + 50) / 100, 0, 255), plane numbers from the table
//     tweak_back_kernel              Y of the clip, averaged U / V -> RGB24 with error diffusion (tweak.hip)
//     reduce_flicker_kernel          ReduceFlicker's five-frame window, one pass over the chunk
// Integer sums do not depend on the order of the atomics, every float sequence is stated: the bytes are identical from run to run.  Nothing is read back.
// KEPT: the weighted average as a launch of its own.  Fused into the load side of the back kernel it would multiply that kernel's chroma loads by N (each
// chroma sample is a tap of four rows and is re-read for every 64-column chunk of a band), in a kernel that is one block per frame and waits on exactly
// those loads (tweak.hip, REJECTED variants); the planes it writes are a sixth of a frame.  MEASURED (profiles/chroma_stab.txt, 64 frames at 384 x 384,
// N = 5): the average is 9 us of the 1 670 us the eight launches take; the two back conversions are 615 + 577 us, the restoring forward one 355 us.
#include "kernels.h"

#pragma clang fp contract(off)
#include "pixel_ops.h"
#include "chroma_stab_ops.h"

// ---- the tables ---------------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int stab_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ bool stab_bit(const uint32_t* bits, int i) { return (bits[i >> 5] >> (i & 31)) & 1u; }

// thread j: output frame s0 + j
__global__ void __launch_bounds__(64) stab_tables_kernel(StabTableArgs a, int* __restrict__ pair_y, int* __restrict__ pair_c, uint8_t* __restrict__ pair_mode,
                                                        int* __restrict__ avg_tab) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.S) return;
    const int s = a.s0 + j, N = a.N, nh = (N - 1) >> 1;
    int* tab = avg_tab + (int64_t)j * N;
    if (a.restore) {
        const uint8_t mode = (int64_t)a.first_frame + s >= CS_BINARY_FIRST ? 1 : 0;
        for (int di = 0; di < N - 1; ++di) {
            const int d = di < nh ? di - nh : di - nh + 1, P = j * (N - 1) + di;
            pair_y[P] = s - a.a0;
            pair_c[P] = stab_clampi(s + d, 0, a.last) - a.a0;
            pair_mode[P] = mode;
            tab[di < nh ? di : di + 1] = a.A + P;                 // the restored clip's plane, behind the A source planes of the pool
        }
        tab[nh] = s - a.a0;
        return;
    }
    int slot[CS_MAX_WEIGHTS];
    for (int k = 0; k < N; ++k) slot[k] = stab_clampi(s + k - nh, 0, a.last) - a.a0;
    for (int i = nh; i > 0; --i)
        if (stab_bit(a.prev_bits, slot[i])) { for (int q = 0; q < i; ++q) slot[q] = slot[i]; break; }
    for (int i = nh; i < N - 1; ++i)
        if (stab_bit(a.next_bits, slot[i])) { for (int q = i + 1; q < N; ++q) slot[q] = slot[i]; break; }
    for (int k = 0; k < N; ++k) tab[k] = slot[k];
}

int launch_stab_tables(StabTableArgs a, int* pair_y, int* pair_c, uint8_t* pair_mode, int* avg_tab, hipStream_t s) {
    if (a.S <= 0 || a.A <= 0 || a.A > CS_MAX_WINDOW || a.N < 3 || a.N > CS_MAX_WEIGHTS || !(a.N & 1) || a.s0 < a.a0 || a.s0 + a.S > a.a0 + a.A ||
        a.a0 < 0 || a.a0 + a.A - 1 > a.last || a.s0 - a.a0 > (a.N - 1) / 2 + 2 || (int64_t)a.S * (a.N - 1) > 65535)
        return (int)hipErrorInvalidValue;
    // every slot is a frame within (N - 1) / 2 of an output frame, clamped to the clip: the caller's window holds them (checked by the caller's arithmetic,
    // and here for its two ends)
    const int nh = (a.N - 1) / 2;
    if (std::max(a.s0 - nh, 0) < a.a0 || std::min(a.s0 + a.S - 1 + nh, a.last) > a.a0 + a.A - 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(stab_tables_kernel, dim3((unsigned)((a.S + 63) / 64)), dim3(64), 0, s, a, pair_y, pair_c, pair_mode, avg_tab);
    return (int)hipGetLastError();
}

// ---- the sums of the shifted clips ------------------------------------------------------------------------------------------------------------------------------
#define STAB_STATS_BLOCKS_MAX 128        // every block ends in two atomics on its frame's slots (as recover.hip)

// Grid: blocks_per blocks for each frame.  A thread owns four neighbouring pixels = 12 bytes per turn (pixel_ops.h load12; h * w is a multiple of four).
__global__ void __launch_bounds__(256) stab_stats_kernel(const uint8_t* __restrict__ gray, const uint8_t* __restrict__ mode, unsigned long long* stats, int h,
                                                        int w, int tht, int blocks_per) {
    __shared__ unsigned red[2][4];
    const int f = (int)(blockIdx.x / (unsigned)blocks_per), part = (int)(blockIdx.x % (unsigned)blocks_per);
    if (!mode[f]) return;                                                              // block-uniform
    const int64_t npix = (int64_t)h * w, ngroups = npix >> 2;
    const uint8_t* src = gray + (int64_t)f * npix * 3;
    // at most 2^24 pixels per frame: a wave's 32-bit sums stay below 2^24 * 255
    unsigned sum = 0, cnt = 0;
    for (int64_t i = (int64_t)part * blockDim.x + threadIdx.x; i < ngroups; i += (int64_t)blocks_per * blockDim.x) {
        int v[12];
        load12(src + i * 12, v);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int y, cu, cv, hh, ss, vv;
            rgb2yuv(v[q * 3], v[q * 3 + 1], v[q * 3 + 2], y, cu, cv);
            cv_rgb2hsv(v[q * 3], v[q * 3 + 1], v[q * 3 + 2], hh, ss, vv);
            sum += (unsigned)y;
            cnt += ss < tht ? 1u : 0u;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { sum += __shfl_down(sum, o, 64); cnt += __shfl_down(cnt, o, 64); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sum; red[1][threadIdx.x >> 6] = cnt; }
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned long long t = 0;
        for (int k = 0; k < 4; ++k) t += red[threadIdx.x][k];
        atomicAdd(stats + 2 * (int64_t)f + threadIdx.x, t);
    }
}

int launch_stab_stats(const uint8_t* gray, const uint8_t* mode, unsigned long long* stats, int n, int h, int w, int tht, hipStream_t s) {
    if (n <= 0 || h < 2 || w < 2 || (h & 1) || (w & 1) || h > TW_MAX_SIDE || w > TW_MAX_SIDE) return (int)hipErrorInvalidValue;
    const int64_t ngroups = ((int64_t)h * w) >> 2;
    int64_t b = (ngroups + 2047) / 2048;
    b = b < 1 ? 1 : (b > STAB_STATS_BLOCKS_MAX ? STAB_STATS_BLOCKS_MAX : b);
    if ((int64_t)n * b > 0x7FFFFFFFll) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(stab_stats_kernel, dim3((unsigned)((int64_t)n * b)), dim3(256), 0, s, gray, mode, stats, h, w, tht, (int)b);
    return (int)hipGetLastError();
}

// ---- std.AverageFrames on the quarter planes --------------------------------------------------------------------------------------------------------------------
// Grid: (groups of four bytes, S, 2 planes).  A thread owns four neighbouring samples of one output plane; the last plane_bytes % 4 go byte by byte.
__global__ void __launch_bounds__(256) stab_average_kernel(const uint8_t* __restrict__ upool, const uint8_t* __restrict__ vpool, uint8_t* __restrict__ uo,
                                                          uint8_t* __restrict__ vo, const int* __restrict__ avg_tab, StabAverageArgs a) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, at = g * 4;
    if (at >= a.plane_bytes) return;
    const int j = blockIdx.y;
    const uint8_t* pool = blockIdx.z ? vpool : upool;
    uint8_t* out = (blockIdx.z ? vo : uo) + (int64_t)j * a.plane_bytes + at;
    const int* tab = avg_tab + (int64_t)j * a.N;
    const int cnt = (int)(a.plane_bytes - at < 4 ? a.plane_bytes - at : 4);
    int acc[4] = {0, 0, 0, 0};
    for (int k = 0; k < a.N; ++k) {
        const uint8_t* p = pool + (int64_t)tab[k] * a.plane_bytes + at;
        uint32_t word = 0;
        if (cnt == 4) __builtin_memcpy(&word, p, 4);
        else for (int q = 0; q < cnt; ++q) word |= (uint32_t)p[q] << (8 * q);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] += a.weights[k] * (int)((word >> (8 * q)) & 255u);
    }
    uint32_t word = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int s = acc[q] + 50;
        const int v = (s >= 0 ? s / 100 : -((-s + 99) / 100));                         // floor division, as Python's //
        word |= (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)) << (8 * q);
    }
    if (cnt == 4) __builtin_memcpy(out, &word, 4);
    else for (int q = 0; q < cnt; ++q) out[q] = (uint8_t)(word >> (8 * q));
}

int launch_stab_average(const uint8_t* upool, const uint8_t* vpool, uint8_t* uo, uint8_t* vo, const int* avg_tab, StabAverageArgs a, hipStream_t s) {
    if (a.S <= 0 || a.S > 65535 || a.N < 3 || a.N > CS_MAX_WEIGHTS || a.plane_bytes <= 0 || a.plane_bytes > (int64_t)TW_MAX_SIDE * TW_MAX_SIDE / 4)
        return (int)hipErrorInvalidValue;
    const int64_t groups = (a.plane_bytes + 3) >> 2;
    hipLaunchKernelGGL(stab_average_kernel, dim3((unsigned)((groups + 255) / 256), (unsigned)a.S, 2u), dim3(256), 0, s, upool, vpool, uo, vo, avg_tab, a);
    return (int)hipGetLastError();
}

// ---- ReduceFlicker(strength = 2, aggressive = 0) (stand-in, restated from memory: tests/stab_util.py reduce_flicker) --------------------------------------------
__device__ __forceinline__ uint32_t stab_load4(const uint8_t* p, int cnt) {
    uint32_t word = 0;
    if (cnt == 4) __builtin_memcpy(&word, p, 4);
    else for (int q = 0; q < cnt; ++q) word |= (uint32_t)p[q] << (8 * q);
    return word;
}

// Grid: (groups of four bytes, count).  Output frame n = f0 + blockIdx.y; frames n < 2 and n > last - 2 are copied.
__global__ void __launch_bounds__(256) reduce_flicker_kernel(const uint8_t* __restrict__ frames, int t0, uint8_t* __restrict__ out, int f0, int last,
                                                            int64_t frame_bytes) {
    const int64_t at = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (at >= frame_bytes) return;
    const int n = f0 + (int)blockIdx.y;
    const int cnt = (int)(frame_bytes - at < 4 ? frame_bytes - at : 4);
    const uint8_t* c = frames + (int64_t)(n - t0) * frame_bytes + at;
    uint32_t word = stab_load4(c, cnt);
    if (n >= 2 && n <= last - 2) {
        const uint32_t wp2 = stab_load4(c - 2 * frame_bytes, cnt), wp1 = stab_load4(c - frame_bytes, cnt);
        const uint32_t wn1 = stab_load4(c + frame_bytes, cnt), wn2 = stab_load4(c + 2 * frame_bytes, cnt);
        uint32_t res = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int sh = 8 * q;
            const int p2 = (wp2 >> sh) & 255, p1 = (wp1 >> sh) & 255, cc = (word >> sh) & 255, n1 = (wn1 >> sh) & 255, n2 = (wn2 >> sh) & 255;
            const int d = min(abs(cc - p2), abs(cc - n2));
            const int avg = (p1 + 2 * cc + n1 + 2) >> 2;
            const int ul = max(min(p1, n1) - d, cc), ll = min(max(p1, n1) + d, cc);
            res |= (uint32_t)min(max(avg, ll), ul) << sh;
        }
        word = res;
    }
    uint8_t* o = out + (int64_t)blockIdx.y * frame_bytes + at;
    if (cnt == 4) __builtin_memcpy(o, &word, 4);
    else for (int q = 0; q < cnt; ++q) o[q] = (uint8_t)(word >> (8 * q));
}

int launch_reduce_flicker(const uint8_t* frames, int t0, uint8_t* out, int f0, int count, int last, int64_t frame_bytes, hipStream_t s) {
    if (count <= 0 || count > 65535 || frame_bytes <= 0 || t0 < 0 || f0 < t0 || f0 + count - 1 > last || t0 > std::max(f0 - 2, 0)) return (int)hipErrorInvalidValue;
    const int64_t groups = (frame_bytes + 3) >> 2;
    if ((groups + 255) / 256 > 0x7FFFFFFFll) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(reduce_flicker_kernel, dim3((unsigned)((groups + 255) / 256), (unsigned)count), dim3(256), 0, s, frames, t0, out, f0, last, frame_bytes);
    return (int)hipGetLastError();
}

void preload_chroma_stab() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(stab_average_kernel)); (void)hipGetLastError(); }
