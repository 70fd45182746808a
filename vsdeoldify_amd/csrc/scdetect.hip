// Per-frame scene statistics of a whole clip (vsslib/vsscdect.py:200-238, 281-298): what the reference's scene detector reads of a frame is the mean of
// its gray plane and std.PlaneStats' difference against the frame `offset` frames before it.  Both are integer reductions over a clip already in HBM:
//     Y      = (cr * R + cg * G + cb * B + bias) >> 16                    the gray plane (stand-in of zimg's RGB -> GRAY8, coefficients from the caller)
//     sum_y  = sum of Y over the frame,  min_y / max_y
//     sad    = sum of |Y_n - Y_p|,  p = max(n - offset, 0)                  (DuplicateFrames(frames=0) `offset` times, then Trim: vsscdect.py:283-286)
// Without normalisation ONE launch produces all of it.  With normalisation (sc_clip_normalize -> vsutils.frame_normalize) a frame whose mean luma lies
// strictly between the thresholds is stretched to uint8(255 * ((Y - min) / (max - min))) before sum_y and sad are taken, which needs every frame's raw
// sum / min / max first: two dependent launches, the second reading the first one's records from device memory (no host round trip, no stored gray
// plane -- the plane is recomputed from the RGB bytes, 3 integer multiply-adds per pixel against 1 byte written and read back per pixel).  The stretch of
// a frame is a 256-entry table that each block builds in LDS from the frame's record (scdetect_ops.h: the float64 sequence of numpy).
//
// Access pattern (as stabilizer.hip / tiles.hip): a thread owns four neighbouring pixels = 12 bytes, one 96-bit load at any byte alignment (frames of a
// clip whose pixel count is no multiple of four start at odd offsets); the last npix % 4 pixels of a frame go byte by byte.  Nothing is read beyond the
// frame.  Reduction: registers -> wave (shuffles) -> block (LDS) -> one 64-bit atomic add per block and quantity, atomic max for the extrema.  All sums are
// integers: the result does not depend on the order and is bit-identical from run to run.
#include "kernels.h"
#include "scdetect_ops.h"

__device__ __forceinline__ unsigned sc_wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned sc_wave_max(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_down(v, o, 64));
    return v;
}

// MODE 0: everything in one launch (no normalisation).  MODE 1: first pass of the normalised form: sum_raw / min / max.  MODE 2: its second pass: sum_y
// and sad of the stretched planes, the tables built from rec[] as MODE 1 left it.
// Grid: blocks_per_frame blocks for each frame, block b works on frame b / blocks_per_frame.  rec[f].min_y holds 255 - min while on the device (the
// records start as zeros, so both extrema are atomic maxima); the host turns it round after the download.
template <int MODE>
__global__ void __launch_bounds__(256) scene_stats_kernel(const uint8_t* __restrict__ clip, SceneRec* rec, SceneStatsArgs a) {
    __shared__ unsigned red[4][4];
    __shared__ uint8_t lut[2][256];
    const int f = (int)(blockIdx.x / (unsigned)a.blocks_per_frame), chunk = (int)(blockIdx.x % (unsigned)a.blocks_per_frame);
    const int p = f > a.offset ? f - a.offset : 0;
    const int64_t npix = (int64_t)a.h * a.w;
    const uint8_t* cur = clip + (int64_t)f * npix * 3;
    const uint8_t* prv = clip + (int64_t)p * npix * 3;
    const bool diff = MODE != 1 && p != f;
    if (MODE == 2) {
        // blockDim.x == 256: thread t makes entry t of the frame's table and of the compared frame's
        const int t = threadIdx.x;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const SceneRec* r = rec + (k == 0 ? f : p);                  // only the fields the first pass left: this pass adds to sum_y / sad meanwhile
            lut[k][t] = (uint8_t)scene_lut_entry(t, r->sum_raw, 255 - r->min_y, r->max_y, npix, a.tht_black, a.tht_white);
        }
        __syncthreads();
    }
    const SceneLuma c{a.cr, a.cg, a.cb, a.bias};
    SceneSums acc{0u, 0u, 0u, 0u};
    scene_accumulate<MODE>(c, cur, prv, diff, npix, lut[0], lut[1], (int64_t)chunk * blockDim.x + threadIdx.x, (int64_t)a.blocks_per_frame * blockDim.x, acc);
    unsigned s_sum = acc.sum, s_sad = acc.sad, s_max = acc.max, s_imin = acc.imin;
    // a thread adds at most 1020 per turn and takes at most 2^14 groups of a frame of 2^31 pixels (launch_scene_stats): a WAVE's 32-bit sum stays below
    // 1.1e9.  A block's would not: the four wave sums are added in 64 bits below.
    s_sum = sc_wave_sum(s_sum);
    s_sad = sc_wave_sum(s_sad);
    s_max = sc_wave_max(s_max);
    s_imin = sc_wave_max(s_imin);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wave][0] = s_sum; red[wave][1] = s_sad; red[wave][2] = s_max; red[wave][3] = s_imin; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t_sum = 0, t_sad = 0;
        unsigned t_max = 0, t_imin = 0;
        for (int k = 0; k < 4; ++k) { t_sum += red[k][0]; t_sad += red[k][1]; t_max = max(t_max, red[k][2]); t_imin = max(t_imin, red[k][3]); }
        SceneRec* r = rec + f;
        if (MODE != 2) {
            atomicAdd(reinterpret_cast<unsigned long long*>(&r->sum_raw), t_sum);
            atomicMax(&r->max_y, (int)t_max);
            atomicMax(&r->min_y, (int)t_imin);
        }
        if (MODE != 1) {
            atomicAdd(reinterpret_cast<unsigned long long*>(&r->sum_y), t_sum);
            atomicAdd(reinterpret_cast<unsigned long long*>(&r->sad), t_sad);
        }
    }
}

int scene_stats_blocks_per_frame(int64_t npix) {
    const int64_t ngroups = (npix + 3) >> 2;
    // eight groups = 32 pixels per thread, at most 128 blocks per frame: every block ends in four atomics on its frame's 32-byte record, and with more
    // blocks those serialise on one cache line (measured: 507 blocks per 1080p frame ran at half the rate of 101 blocks per 480p frame)
    const int64_t b = (ngroups + 2047) / 2048;
    return (int)(b < 1 ? 1 : (b > 128 ? 128 : b));
}

// rec: n records in device memory, ZERO-FILLED by the caller in front of the launch (on the same stream)
int launch_scene_stats(const uint8_t* clip, SceneRec* rec, SceneStatsArgs a, hipStream_t s) {
    const int64_t npix = (int64_t)a.h * a.w;
    if (a.n <= 0 || npix <= 0 || npix > ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
    a.blocks_per_frame = scene_stats_blocks_per_frame(npix);
    const int64_t blocks = (int64_t)a.n * a.blocks_per_frame;
    if (blocks > 0x7FFFFFFFll) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks);
    if (!a.normalize) {
        hipLaunchKernelGGL((scene_stats_kernel<0>), grid, dim3(256), 0, s, clip, rec, a);
    } else {
        hipLaunchKernelGGL((scene_stats_kernel<1>), grid, dim3(256), 0, s, clip, rec, a);
        hipLaunchKernelGGL((scene_stats_kernel<2>), grid, dim3(256), 0, s, clip, rec, a);
    }
    return (int)hipGetLastError();
}

void preload_scdetect() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(scene_stats_kernel<0>)); (void)hipGetLastError(); }
