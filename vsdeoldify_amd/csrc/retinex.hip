// HAVC_retinex (vsdeoldify/__init__.py:1073-1101 -> vsslib/vsretinex.py:25-88) on a chunk of a clip [n][h][w][3] in HBM: multi-scale Retinex with colour
// preservation (MSRCP) between the reference's luma gate and its luma blend.  The plugin the reference calls (retinex.MSRCP) cannot be executed where the
// fixtures are made: its pixel work is restated from the published algorithm (Petro / Sbert / Morel, IPOL 2014; Young - van Vliet recursive Gaussian) and
// that restatement -- tests/retinex_util.py -- is the definition (retinex_ops.h has every expression).
// Launches (one stream, each reading what the one before left in device memory; nothing comes back to the host in between):
//     ret_luma_kernel     per frame the integer sum of cv2's Y (the gate and the blend weight hang off it)
//     ret_hpass_kernel    the horizontal recursion of every (frame, sigma, row): a block = one wave = 64 rows, one lane per row.  The rows are walked
//                         in tiles of 64 rows x 32 columns staged through LDS: the wave loads a tile row by row (a row's 32 columns by 32 neighbouring
//                         lanes: coalesced), every lane walks its own row inside the tile, the tile goes back row by row.  The intensity is computed
//                         from the RGB bytes while the tile is loaded: no intensity plane is stored.  The last tile of the forward sweep stays in
//                         LDS and the backward sweep starts on it.  Tile pitch 33 doubles: lane L reads double L * 33 + j, so the 32 lanes of an
//                         8-byte LDS access group fall into 32 different bank pairs, and the row-wise stores of 16 neighbouring doubles do as well.
//     ret_vpass_kernel    the vertical recursion in place, one lane per (frame, sigma, column): neighbouring lanes read neighbouring columns, so every
//                         access is coalesced as it stands; eight rows are loaded ahead of the recursion that consumes them.
//     ret_msr_kernel      per pixel the product P of I / g + 1 over the sigmas, O = log(P) / n_sigmas written over the first Gaussian plane, and the
//                         frame's smallest and largest O: block reduction on the ordered bit pattern, then one integer atomic maximum each.
//     ret_hist_kernel     4096-bin histogram of O per frame: LDS counters, then integer global atomics for the occupied bins.
//     ret_params_kernel   one block per frame: the two histogram walks as a prefix sum, lo / hi, the gate and the blend weight.
//     ret_apply_kernel    per pixel: stretch, gain with the saturation cap, range conversion, Pillow's blend; a gated-out frame is copied.
// Integer sums, integer atomics on ordered bit patterns and stated float64 sequences throughout (this file is built with -ffp-contract=off): the bytes are
// identical from run to run.  The recursions, the planes and the MSR product are float64: in float32 the rounding of B1..B3 at sigma = 250 alone moves the
// filter's DC gain by tens of percent (DESIGN.md "Retinex" has the measurement).
// Every index into a plane or a clip is formed in 64 bits; a lane outside the frame neither loads nor stores.
#include "kernels.h"
#include "retinex_ops.h"
#include "pixel_ops.h"

#define RT_THREADS 256
#define RT_ROWS 64                       // rows of a horizontal tile = lanes of the wave that walks it
#define RT_COLS 32
#define RT_PITCH 33                      // doubles per tile row in LDS (file comment)
#define RT_AHEAD 8                       // rows the vertical pass loads ahead

__device__ __forceinline__ unsigned long long rt_wave_max(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}

// the four pixels of a 12-byte group held in three little-endian dwords (as equalize.hip)
__device__ __forceinline__ void rt_unpack(const uint32_t w[3], int px[4][3]) {
    px[0][0] = w[0] & 255u; px[0][1] = (w[0] >> 8) & 255u; px[0][2] = (w[0] >> 16) & 255u;
    px[1][0] = w[0] >> 24; px[1][1] = w[1] & 255u; px[1][2] = (w[1] >> 8) & 255u;
    px[2][0] = (w[1] >> 16) & 255u; px[2][1] = w[1] >> 24; px[2][2] = w[2] & 255u;
    px[3][0] = (w[2] >> 8) & 255u; px[3][1] = (w[2] >> 16) & 255u; px[3][2] = w[2] >> 24;
}
__device__ __forceinline__ void rt_pack(const int px[4][3], uint32_t w[3]) {
    w[0] = (uint32_t)px[0][0] | (uint32_t)px[0][1] << 8 | (uint32_t)px[0][2] << 16 | (uint32_t)px[1][0] << 24;
    w[1] = (uint32_t)px[1][1] | (uint32_t)px[1][2] << 8 | (uint32_t)px[2][0] << 16 | (uint32_t)px[2][1] << 24;
    w[2] = (uint32_t)px[2][2] | (uint32_t)px[3][0] << 8 | (uint32_t)px[3][1] << 16 | (uint32_t)px[3][2] << 24;
}

// ---- the frame's sum of cv2's Y.  Grid: blocks_per_frame blocks per frame. ----
__global__ void __launch_bounds__(RT_THREADS) ret_luma_kernel(const uint8_t* __restrict__ clip, RetFrameRec* rec, RetArgs a) {
    const int f = (int)(blockIdx.x / (unsigned)a.blocks_per_frame), part = (int)(blockIdx.x % (unsigned)a.blocks_per_frame);
    const int64_t npix = (int64_t)a.h * a.w;
    const uint8_t* src = clip + (int64_t)f * npix * 3;
    unsigned long long s = 0;
    for (int64_t i = (int64_t)part * RT_THREADS + threadIdx.x; i < npix; i += (int64_t)a.blocks_per_frame * RT_THREADS) {
        const uint8_t* p = src + i * 3;
        s += (unsigned)sat8(descale14(p[0] * 4899 + p[1] * 9617 + p[2] * 1868));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&rec[f].sum_y, s);
}

// ---- horizontal pass.  Grid: n * ns * ceil(h / 64) blocks of one wave. ----
__global__ void __launch_bounds__(RT_ROWS) ret_hpass_kernel(const uint8_t* __restrict__ clip, double* __restrict__ planes, RetArgs a) {
    __shared__ double tile[RT_ROWS * RT_PITCH];
    const int groups = (a.h + RT_ROWS - 1) / RT_ROWS;
    int b = (int)blockIdx.x;
    const int r0 = (b % groups) * RT_ROWS;
    b /= groups;
    const int s = b % a.ns, f = b / a.ns;
    const int lane = threadIdx.x, half = lane >> 5, cl = lane & 31;
    const int64_t npix = (int64_t)a.h * a.w;
    const uint8_t* src = clip + (int64_t)f * npix * 3;
    double* pl = planes + ((int64_t)f * a.ns + s) * npix;
    const double B = a.coef[s][0], B1 = a.coef[s][1], B2 = a.coef[s][2], B3 = a.coef[s][3];
    const double inv3sR = 1.0 / (double)(3 * a.sR);
    const int nt = (a.w + RT_COLS - 1) / RT_COLS;
    double* row = tile + lane * RT_PITCH;
    double p1 = 0.0, p2 = 0.0, p3 = 0.0;
    // forward: tiles left to right, the intensity from the bytes
    for (int t = 0; t < nt; ++t) {
        const int c0 = t * RT_COLS, cols = a.w - c0 < RT_COLS ? a.w - c0 : RT_COLS;
        for (int rr = 0; rr < RT_ROWS; rr += 2) {
            const int r = rr + half, gr = r0 + r, c = c0 + cl;
            double v = 0.0;
            if (gr < a.h && c < a.w) {
                const uint8_t* p = src + ((int64_t)gr * a.w + c) * 3;
                v = ret_intensity(p[0], p[1], p[2], a.sF, inv3sR);
            }
            tile[r * RT_PITCH + cl] = v;
        }
        __syncthreads();
        if (t == 0) p1 = p2 = p3 = row[0];
        if (cols == RT_COLS) {
#pragma unroll
            for (int j = 0; j < RT_COLS; ++j) {
                const double y = ret_step(row[j], p1, p2, p3, B, B1, B2, B3);
                row[j] = y;
                p3 = p2; p2 = p1; p1 = y;
            }
        } else {
            for (int j = 0; j < cols; ++j) {
                const double y = ret_step(row[j], p1, p2, p3, B, B1, B2, B3);
                row[j] = y;
                p3 = p2; p2 = p1; p1 = y;
            }
        }
        __syncthreads();
        if (t != nt - 1) {                       // the last tile stays where the backward sweep starts
            for (int rr = 0; rr < RT_ROWS; rr += 2) {
                const int r = rr + half, gr = r0 + r, c = c0 + cl;
                if (gr < a.h && c < a.w) pl[(int64_t)gr * a.w + c] = tile[r * RT_PITCH + cl];
            }
            __syncthreads();
        }
    }
    // backward: tiles right to left, in place
    for (int t = nt - 1; t >= 0; --t) {
        const int c0 = t * RT_COLS, cols = a.w - c0 < RT_COLS ? a.w - c0 : RT_COLS;
        if (t != nt - 1) {
            for (int rr = 0; rr < RT_ROWS; rr += 2) {
                const int r = rr + half, gr = r0 + r, c = c0 + cl;
                tile[r * RT_PITCH + cl] = (gr < a.h && c < a.w) ? pl[(int64_t)gr * a.w + c] : 0.0;
            }
            __syncthreads();
        } else {
            p1 = p2 = p3 = row[cols - 1];
        }
        if (cols == RT_COLS) {
#pragma unroll
            for (int j = RT_COLS - 1; j >= 0; --j) {
                const double y = ret_step(row[j], p1, p2, p3, B, B1, B2, B3);
                row[j] = y;
                p3 = p2; p2 = p1; p1 = y;
            }
        } else {
            for (int j = cols - 1; j >= 0; --j) {
                const double y = ret_step(row[j], p1, p2, p3, B, B1, B2, B3);
                row[j] = y;
                p3 = p2; p2 = p1; p1 = y;
            }
        }
        __syncthreads();
        for (int rr = 0; rr < RT_ROWS; rr += 2) {
            const int r = rr + half, gr = r0 + r, c = c0 + cl;
            if (gr < a.h && c < a.w) pl[(int64_t)gr * a.w + c] = tile[r * RT_PITCH + cl];
        }
        __syncthreads();
    }
}

// ---- vertical pass, in place.  Grid: n * ns * ceil(w / 64) blocks of one wave; a lane owns a column. ----
__global__ void __launch_bounds__(64) ret_vpass_kernel(double* __restrict__ planes, RetArgs a) {
    const int groups = (a.w + 63) / 64;
    int b = (int)blockIdx.x;
    const int c = (b % groups) * 64 + (int)threadIdx.x;
    b /= groups;
    const int s = b % a.ns, f = b / a.ns;
    if (c >= a.w) return;
    const int64_t npix = (int64_t)a.h * a.w, w = a.w;
    double* col = planes + ((int64_t)f * a.ns + s) * npix + c;
    const double B = a.coef[s][0], B1 = a.coef[s][1], B2 = a.coef[s][2], B3 = a.coef[s][3];
    double x[RT_AHEAD];
    double p1 = col[0], p2 = p1, p3 = p1;
    int r = 0;
    for (; r + RT_AHEAD <= a.h; r += RT_AHEAD) {
#pragma unroll
        for (int k = 0; k < RT_AHEAD; ++k) x[k] = col[(int64_t)(r + k) * w];
#pragma unroll
        for (int k = 0; k < RT_AHEAD; ++k) {
            const double y = ret_step(x[k], p1, p2, p3, B, B1, B2, B3);
            col[(int64_t)(r + k) * w] = y;
            p3 = p2; p2 = p1; p1 = y;
        }
    }
    for (; r < a.h; ++r) {
        const double y = ret_step(col[(int64_t)r * w], p1, p2, p3, B, B1, B2, B3);
        col[(int64_t)r * w] = y;
        p3 = p2; p2 = p1; p1 = y;
    }
    p1 = p2 = p3 = col[(int64_t)(a.h - 1) * w];
    r = a.h - 1;
    for (; r - RT_AHEAD + 1 >= 0; r -= RT_AHEAD) {
#pragma unroll
        for (int k = 0; k < RT_AHEAD; ++k) x[k] = col[(int64_t)(r - k) * w];
#pragma unroll
        for (int k = 0; k < RT_AHEAD; ++k) {
            const double y = ret_step(x[k], p1, p2, p3, B, B1, B2, B3);
            col[(int64_t)(r - k) * w] = y;
            p3 = p2; p2 = p1; p1 = y;
        }
    }
    for (; r >= 0; --r) {
        const double y = ret_step(col[(int64_t)r * w], p1, p2, p3, B, B1, B2, B3);
        col[(int64_t)r * w] = y;
        p3 = p2; p2 = p1; p1 = y;
    }
}

// ---- MSR product, log, the frame's extremes.  Grid: blocks_per_frame blocks per frame.  tap_p (optional): the product planes [n][h][w]. ----
__global__ void __launch_bounds__(RT_THREADS) ret_msr_kernel(const uint8_t* __restrict__ clip, double* planes, RetFrameRec* rec, double* tap_p, RetArgs a) {
    __shared__ unsigned long long red[2][4];
    const int f = (int)(blockIdx.x / (unsigned)a.blocks_per_frame), part = (int)(blockIdx.x % (unsigned)a.blocks_per_frame);
    const int64_t npix = (int64_t)a.h * a.w;
    const uint8_t* src = clip + (int64_t)f * npix * 3;
    double* pl = planes + (int64_t)f * a.ns * npix;
    const double inv3sR = 1.0 / (double)(3 * a.sR), dn = (double)a.ns;
    unsigned long long kmax = 0, kmin_inv = 0;                   // a thread without pixels leaves both atomics unchanged
    for (int64_t i = (int64_t)part * RT_THREADS + threadIdx.x; i < npix; i += (int64_t)a.blocks_per_frame * RT_THREADS) {
        const uint8_t* p = src + i * 3;
        const double in = ret_intensity(p[0], p[1], p[2], a.sF, inv3sR);
        double prod = 1.0;
        for (int s = 0; s < a.ns; ++s) prod *= ret_factor(in, pl[(int64_t)s * npix + i]);
        if (tap_p) tap_p[(int64_t)f * npix + i] = prod;
        const double o = log(prod) / dn;
        pl[i] = o;                                               // over the first Gaussian plane, which this thread has read
        const unsigned long long k = ret_key(o);
        kmax = k > kmax ? k : kmax;
        kmin_inv = ~k > kmin_inv ? ~k : kmin_inv;
    }
    kmax = rt_wave_max(kmax);
    kmin_inv = rt_wave_max(kmin_inv);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = kmax; red[1][threadIdx.x >> 6] = kmin_inv; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const unsigned long long* q = red[threadIdx.x];
        unsigned long long v = q[0];
        for (int k = 1; k < 4; ++k) v = q[k] > v ? q[k] : v;
        if (v) atomicMax(threadIdx.x == 0 ? &rec[f].max_key : &rec[f].min_inv, v);
    }
}

// ---- histogram of O.  Grid: blocks_per_frame blocks per frame. ----
__global__ void __launch_bounds__(RT_THREADS) ret_hist_kernel(const double* __restrict__ planes, const RetFrameRec* rec, unsigned* hist, RetArgs a) {
    __shared__ unsigned bins[RET_BINS];
    const int f = (int)(blockIdx.x / (unsigned)a.blocks_per_frame), part = (int)(blockIdx.x % (unsigned)a.blocks_per_frame);
    const int64_t npix = (int64_t)a.h * a.w;
    const double mn = ret_unkey(~rec[f].min_inv), mx = ret_unkey(rec[f].max_key);
    if (!(mx > mn)) return;                                      // the same for every thread: the frame takes O' = I
    const double* o = planes + (int64_t)f * a.ns * npix;
    const double scale = (double)(RET_BINS - 1) / (mx - mn);
    for (int k = threadIdx.x; k < RET_BINS; k += RT_THREADS) bins[k] = 0u;
    __syncthreads();
    for (int64_t i = (int64_t)part * RT_THREADS + threadIdx.x; i < npix; i += (int64_t)a.blocks_per_frame * RT_THREADS)
        atomicAdd(&bins[ret_bin(o[i], mn, scale)], 1u);
    __syncthreads();
    unsigned* gh = hist + (int64_t)f * RET_BINS;
    for (int k = threadIdx.x; k < RET_BINS; k += RT_THREADS)
        if (bins[k]) atomicAdd(&gh[k], bins[k]);
}

// ---- per-frame scalars.  Grid: one block per frame.  Thread t owns the 16 bins from 16 t on. ----
__global__ void __launch_bounds__(RT_THREADS) ret_params_kernel(RetFrameRec* rec, const unsigned* hist, RetArgs a) {
    __shared__ long long wave_sum[4];
    __shared__ int k_lo, k_hi;
    const int f = (int)blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t npix = (int64_t)a.h * a.w;
    const double mn = ret_unkey(~rec[f].min_inv), mx = ret_unkey(rec[f].max_key);
    const bool ranged = mx > mn;
    constexpr int PER = RET_BINS / RT_THREADS;
    const unsigned* gh = hist + (int64_t)f * RET_BINS + t * PER;
    unsigned cnt[PER];
    long long mine = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) { cnt[k] = gh[k]; mine += cnt[k]; }
    long long incl = mine;                                       // inclusive prefix sum over the block
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long u = __shfl_up(incl, o, 64);
        if (lane >= o) incl += u;
    }
    if (lane == 63) wave_sum[wave] = incl;
    if (t == 0) { k_lo = 0; k_hi = RET_BINS - 1; }
    __syncthreads();
    for (int k = 0; k < wave; ++k) incl += wave_sum[k];
    const long long before = incl - mine, thr = ret_threshold_count(npix), total = npix;
    if (ranged) {
        // from bin 0 upward: the first bin at which the running count exceeds thr
        if (before <= thr && thr < incl) {
            long long run = before;
            for (int k = 0; k < PER; ++k) { run += cnt[k]; if (run > thr) { k_lo = t * PER + k; break; } }
        }
        // from the last bin downward the running count at bin k is total - (count in front of k): the largest k whose front count is below total - thr
        if (before < total - thr && total - thr <= incl) {
            long long front = before;
            int best = t * PER;
            for (int k = 0; k < PER; ++k) { if (front < total - thr) best = t * PER + k; front += cnt[k]; }
            k_hi = best;
        }
    }
    __syncthreads();
    if (t == 0) {
        RetFrameRec& r = rec[f];
        const double fl = eq_f_luma(r.sum_y, (long long)npix, a.range_tv);
        r.gate = ret_gate(fl, a.luma_dark, a.luma_bright) ? 1 : 0;
        r.weight = ret_blend_weight(fl, a.blend);
        double lo = 0.0, hi = 0.0;
        if (ranged) { lo = ret_bin_value(k_lo, mn, mx); hi = ret_bin_value(k_hi, mn, mx); }
        r.use_i = (ranged && hi > lo) ? 0 : 1;
        r.lo = lo;
        r.inv = r.use_i ? 0.0 : 1.0 / (hi - lo);
    }
}

// ---- the output.  Grid: blocks_per_frame blocks per frame; a thread owns four neighbouring pixels = 12 bytes (as equalize.hip). ----
__global__ void __launch_bounds__(RT_THREADS) ret_apply_kernel(const uint8_t* __restrict__ clip, uint8_t* __restrict__ out, const double* __restrict__ planes,
                                                              const RetFrameRec* rec, RetArgs a) {
    const int f = (int)(blockIdx.x / (unsigned)a.blocks_per_frame), part = (int)(blockIdx.x % (unsigned)a.blocks_per_frame);
    const int64_t npix = (int64_t)a.h * a.w, ngroups = (npix + 3) >> 2;
    const uint8_t* src = clip + (int64_t)f * npix * 3;
    uint8_t* dst = out + (int64_t)f * npix * 3;
    const double* o = planes + (int64_t)f * a.ns * npix;
    const RetFrameRec r = rec[f];
    const double inv3sR = 1.0 / (double)(3 * a.sR), range_scale = (double)a.dR / (double)a.sR;
    for (int64_t i = (int64_t)part * RT_THREADS + threadIdx.x; i < ngroups; i += (int64_t)a.blocks_per_frame * RT_THREADS) {
        const bool full = i * 4 + 4 <= npix;
        const int cnt = full ? 4 : (int)(npix - i * 4);
        int px[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        if (full) {
            uint32_t w[3];
            __builtin_memcpy(w, src + i * 12, 12);
            rt_unpack(w, px);
        } else {
            for (int j = 0; j < cnt; ++j) { px[j][0] = src[(i * 4 + j) * 3]; px[j][1] = src[(i * 4 + j) * 3 + 1]; px[j][2] = src[(i * 4 + j) * 3 + 2]; }
        }
        if (r.gate) {
            for (int j = 0; j < cnt; ++j) {
                const int c0 = px[j][0], c1 = px[j][1], c2 = px[j][2];
                const double in = ret_intensity(c0, c1, c2, a.sF, inv3sR);
                const double os = r.use_i ? in : ret_stretch(o[i * 4 + j], r.lo, r.inv);
                const int m = (c0 > c1 ? (c0 > c2 ? c0 : c2) : (c1 > c2 ? c1 : c2)) - a.sF;
                const double gain = ret_gain(os, in, m, a.sR);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int v = ret_out_channel(px[j][c] - a.sF, gain, range_scale, a.dF);
                    px[j][c] = r.weight >= 0.f ? eq_pil_blend(px[j][c], v, r.weight) : v;
                }
            }
        }
        if (full) {
            uint32_t w[3];
            rt_pack(px, w);
            __builtin_memcpy(dst + i * 12, w, 12);
        } else {
            for (int j = 0; j < cnt; ++j) { dst[(i * 4 + j) * 3] = (uint8_t)px[j][0]; dst[(i * 4 + j) * 3 + 1] = (uint8_t)px[j][1]; dst[(i * 4 + j) * 3 + 2] = (uint8_t)px[j][2]; }
        }
    }
}

size_t retinex_record_bytes(int n) { return (size_t)n * (sizeof(RetFrameRec) + RET_BINS * sizeof(unsigned)); }

static int rt_blocks_per_frame(int64_t npix) {
    // 16 pixels per thread and turn; at most 256 blocks a frame, so that a frame's atomics on its record stay few
    const int64_t b = (npix + RT_THREADS * 16 - 1) / (RT_THREADS * 16);
    return (int)(b < 1 ? 1 : (b > 256 ? 256 : b));
}

int launch_retinex(const uint8_t* src, uint8_t* dst, double* planes, void* recs, double* tap_g, double* tap_p, RetArgs a, hipStream_t s) {
    const int64_t npix = (int64_t)a.h * a.w;
    if (a.n <= 0 || a.h <= 0 || a.w <= 0 || npix > ((int64_t)1 << 30) || a.ns < 1 || a.ns > RET_MAX_SIGMAS || !src || !dst || !planes || !recs ||
        (tap_g == nullptr) != (tap_p == nullptr)) return (int)hipErrorInvalidValue;
    a.blocks_per_frame = rt_blocks_per_frame(npix);
    const int64_t hb = (int64_t)a.n * a.ns * ((a.h + RT_ROWS - 1) / RT_ROWS), vb = (int64_t)a.n * a.ns * ((a.w + 63) / 64);
    if ((int64_t)a.n * a.blocks_per_frame > 0x7FFFFFFFll || hb > 0x7FFFFFFFll || vb > 0x7FFFFFFFll) return (int)hipErrorInvalidValue;
    RetFrameRec* rec = (RetFrameRec*)recs;
    unsigned* hist = (unsigned*)(rec + a.n);
    const dim3 grid((unsigned)((int64_t)a.n * a.blocks_per_frame)), block(RT_THREADS);
    hipLaunchKernelGGL(ret_luma_kernel, grid, block, 0, s, src, rec, a);
    hipLaunchKernelGGL(ret_hpass_kernel, dim3((unsigned)hb), dim3(RT_ROWS), 0, s, src, planes, a);
    hipLaunchKernelGGL(ret_vpass_kernel, dim3((unsigned)vb), dim3(64), 0, s, planes, a);
    if (tap_g) {
        const hipError_t e = hipMemcpyAsync(tap_g, planes, (size_t)a.n * a.ns * npix * sizeof(double), hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(ret_msr_kernel, grid, block, 0, s, src, planes, rec, tap_p, a);
    hipLaunchKernelGGL(ret_hist_kernel, grid, block, 0, s, planes, rec, hist, a);
    hipLaunchKernelGGL(ret_params_kernel, dim3((unsigned)a.n), block, 0, s, rec, hist, a);
    hipLaunchKernelGGL(ret_apply_kernel, grid, block, 0, s, src, dst, planes, rec, a);
    return (int)hipGetLastError();
}

void preload_retinex() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(ret_hpass_kernel)); (void)hipGetLastError(); }
