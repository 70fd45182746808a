// rgb_equalizer (vsdeoldify/havc_utils.py:836-1075, methods 0-3) with rgb_balance (:1087-1145) in front of it, on a whole clip [n][h][w][3] in HBM: what
// HAVC_bw_tune (vsdeoldify/__init__.py:1266-1339) and HAVC_auto_levels (:3150-3179) do to a frame, without cv2 and without a host round trip.
//     method 0   cv2 RGB2YUV, CLAHE (8 x 8 tiles) on Y, clamp to the range, YUV2RGB, image_luma_blend(.., 0.40, 0.90, 0.35, 2.0)
//     method 1   cv2.equalizeHist on R, G and B (whole-frame histograms), image_luma_blend(.., 0.40, 0.90, 0.15, 4.0)
//     method 2   CLAHE on R, G and B, the same blend constants as method 1
//     method 3   std.Merge(method 0, method 1, weight3)
// then std.Merge(result, input, 1 - strength).  Frames whose f_luma lies outside [0.15, 0.70] come back as they are.
// Launches (all on one stream, each reading what the one before left in device memory):
//     eq_chan_sum_kernel    only with rgb_balance: the three channel sums of every frame (PlaneStatsAverage), integer atomics
//     eq_lut_kernel         one block per (frame, tile): 256-bin histograms in LDS of every plane the method needs -- Y recomputed from the RGB bytes, no
//                           plane is stored; BORDER_REFLECT_101 padding by index arithmetic -- then, in the same block, CLAHE's clip / redistribute /
//                           prefix sum -> 256 bytes per (plane, tile).  Method 1 / 3: the tile's histograms of the REAL pixels are added to the frame's
//                           256-bin global histograms (integer atomics: order-free).  sum_y of the frame for the gate.
//     eq_apply_kernel       per pixel: the plane value again, bilinear blend of the four neighbouring tile tables (the frame's tables staged in LDS,
//                           16 KiB per plane), clamp, YUV2RGB, the frame's gate and blend weights (float64, from sum_y, by thread 0 of each block),
//                           Pillow's blend, the method-3 merge, the strength merge.  A thread owns four neighbouring pixels = 12 bytes, one 96-bit
//                           access at any alignment (as stabilizer.hip / scdetect.hip); the last npix % 4 pixels of a frame go byte by byte.
// "First load" and "last store": every sample read goes through a 256-entry table `pre` (the caller's lut_in -- std.Levels + the range conversion of
// HAVC_bw_tune -- composed with the frame's rgb_balance, which is a per-channel table once the gains are known: each block builds it in LDS from the
// frame's channel sums) and every sample written through the caller's lut_out.
// All sums are integers and every float expression is a stated sequence (equalize_ops.h; this file is built with -ffp-contract=off): bit-identical from
// run to run and equal to the numpy restatement in tests/equalize_util.py.
// LDS / occupancy: eq_lut_kernel 4 waves x 4 planes x 1 KiB private histograms (a flat patch makes every lane of a wave hit one bin: those atomics
// serialise inside the wave whatever the layout; private copies keep the four waves from serialising against each other) = 17 KiB.  eq_apply_kernel:
// 17.3 KiB (method 0), 18 KiB (method 3), 49.3 KiB (method 2: three blocks = 12 waves per CU of the 160 KiB, enough for a kernel that waits on HBM).
#include "kernels.h"
#include "equalize_ops.h"
#include "pixel_ops.h"

#define EQ_THREADS 256

__device__ __forceinline__ int eq_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// sum / minimum / inclusive prefix sum over the 256 threads of a block; red: 4 ints of LDS.  Every thread of the block must call them.
__device__ __forceinline__ int eq_block_sum(int v, int* red) {
    v = eq_wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const int t = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return t;
}
__device__ __forceinline__ int eq_block_min(int v, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const int t = min(min(red[0], red[1]), min(red[2], red[3]));
    __syncthreads();
    return t;
}
__device__ __forceinline__ int eq_block_scan(int v, int* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    if (lane == 63) red[wave] = v;
    __syncthreads();
    for (int k = 0; k < wave; ++k) v += red[k];
    __syncthreads();
    return v;
}

// entry threadIdx.x of the frame's three `pre` tables (file comment)
__device__ __forceinline__ void eq_build_pre(uint8_t (*pre)[256], const EqArgs& a, const EqFrameRec* rec) {
    const int t = threadIdx.x;
    const int v = a.lut_in[t];
    if (!a.balance) {
        pre[0][t] = pre[1][t] = pre[2][t] = (uint8_t)v;
        return;
    }
    float gain[3];
    eq_balance_gains(rec->chan, (long long)a.h * a.w, a.factor, gain);
#pragma unroll
    for (int c = 0; c < 3; ++c) pre[c][t] = (uint8_t)eq_merge15(eq_expr_mul(v, gain[c]), v, a.bal_w15);
}

// the four pixels of a 12-byte group held in three little-endian dwords
__device__ __forceinline__ void eq_unpack(const uint32_t w[3], int px[4][3]) {
    px[0][0] = w[0] & 255u; px[0][1] = (w[0] >> 8) & 255u; px[0][2] = (w[0] >> 16) & 255u;
    px[1][0] = w[0] >> 24; px[1][1] = w[1] & 255u; px[1][2] = (w[1] >> 8) & 255u;
    px[2][0] = (w[1] >> 16) & 255u; px[2][1] = w[1] >> 24; px[2][2] = w[2] & 255u;
    px[3][0] = (w[2] >> 8) & 255u; px[3][1] = (w[2] >> 16) & 255u; px[3][2] = w[2] >> 24;
}
__device__ __forceinline__ void eq_pack(const int px[4][3], uint32_t w[3]) {
    w[0] = (uint32_t)px[0][0] | (uint32_t)px[0][1] << 8 | (uint32_t)px[0][2] << 16 | (uint32_t)px[1][0] << 24;
    w[1] = (uint32_t)px[1][1] | (uint32_t)px[1][2] << 8 | (uint32_t)px[2][0] << 16 | (uint32_t)px[2][1] << 24;
    w[2] = (uint32_t)px[2][2] | (uint32_t)px[3][0] << 8 | (uint32_t)px[3][1] << 16 | (uint32_t)px[3][2] << 24;
}

// ---- rgb_balance's channel sums: sum over the frame of lut_in[sample], per channel.  Grid: blocks_per_frame blocks per frame. ----
__global__ void __launch_bounds__(EQ_THREADS) eq_chan_sum_kernel(const uint8_t* __restrict__ clip, EqFrameRec* rec, EqArgs a) {
    __shared__ uint8_t lut[256];
    __shared__ unsigned long long red[4][3];
    const int f = (int)(blockIdx.x / (unsigned)a.blocks_per_frame), chunk = (int)(blockIdx.x % (unsigned)a.blocks_per_frame);
    const int64_t npix = (int64_t)a.h * a.w, ngroups = (npix + 3) >> 2;
    const uint8_t* src = clip + (int64_t)f * npix * 3;
    lut[threadIdx.x] = a.lut_in[threadIdx.x];
    __syncthreads();
    // a thread takes at most 2^28 / (256 blocks x 256 threads) = 4096 groups of 4 pixels x 255 (launch_equalize): far below 2^32
    unsigned s[3] = {0u, 0u, 0u};
    for (int64_t i = (int64_t)chunk * EQ_THREADS + threadIdx.x; i < ngroups; i += (int64_t)a.blocks_per_frame * EQ_THREADS) {
        if (i * 4 + 4 <= npix) {
            uint32_t w[3];
            int px[4][3];
            __builtin_memcpy(w, src + i * 12, 12);
            eq_unpack(w, px);
#pragma unroll
            for (int j = 0; j < 4; ++j) { s[0] += lut[px[j][0]]; s[1] += lut[px[j][1]]; s[2] += lut[px[j][2]]; }
        } else {
            for (int64_t p = i * 4; p < npix; ++p) { s[0] += lut[src[p * 3]]; s[1] += lut[src[p * 3 + 1]]; s[2] += lut[src[p * 3 + 2]]; }
        }
    }
    // the lanes are added in 64 bits; one atomic per block and channel (the records of a frame share a cache line: scdetect.hip measured what many
    // atomics on one line cost)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        unsigned long long v = s[c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][c] = v;
    }
    __syncthreads();
    if (threadIdx.x < 3) atomicAdd(&rec[f].chan[threadIdx.x], red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// ---- histograms and CLAHE tables.  Grid: EQ_TILES blocks per frame, block b = tile b % 64 of frame b / 64. ----
// planes of the LDS histograms -- method 0: Y | method 1: R G B (real pixels) | method 2: R G B | method 3: Y, then R G B (real pixels)
__global__ void __launch_bounds__(EQ_THREADS) eq_lut_kernel(const uint8_t* __restrict__ clip, EqFrameRec* rec, unsigned* ghist, uint8_t* luts, EqArgs a) {
    __shared__ unsigned hist[4][4][256];          // [wave][plane][bin]
    __shared__ uint8_t pre[3][256];
    __shared__ int red[4];
    const int f = (int)(blockIdx.x / EQ_TILES), tile = (int)(blockIdx.x % EQ_TILES);
    const int t = threadIdx.x, wave = t >> 6;
    const int64_t npix = (int64_t)a.h * a.w;
    const uint8_t* src = clip + (int64_t)f * npix * 3;
    eq_build_pre(pre, a, rec + f);
#pragma unroll
    for (int k = 0; k < 16; ++k) (&hist[0][0][0])[k * 256 + t] = 0u;
    __syncthreads();
    const int x0 = (tile % EQ_GRID) * a.tile_w, y0 = (tile / EQ_GRID) * a.tile_h, area = a.tile_w * a.tile_h;
    const int method = a.method;
    unsigned sum_y = 0;                           // at most 2^30 / 64 / 256 pixels x 255 per thread
    for (int i = t; i < area; i += EQ_THREADS) {
        const int ly = i / a.tile_w, lx = i - ly * a.tile_w;
        const int px = x0 + lx, py = y0 + ly;
        const bool real = px < a.w && py < a.h;
        const uint8_t* p = src + ((int64_t)eq_reflect101(py, a.h) * a.w + eq_reflect101(px, a.w)) * 3;
        const int r = pre[0][p[0]], g = pre[1][p[1]], b = pre[2][p[2]];
        const int y = sat8(descale14(r * 4899 + g * 9617 + b * 1868));
        if (real) sum_y += (unsigned)y;
        if (method == 0 || method == 3) atomicAdd(&hist[wave][0][y], 1u);
        if (method == 2 || (real && method == 1)) {
            atomicAdd(&hist[wave][0][r], 1u); atomicAdd(&hist[wave][1][g], 1u); atomicAdd(&hist[wave][2][b], 1u);
        }
        if (real && method == 3) { atomicAdd(&hist[wave][1][r], 1u); atomicAdd(&hist[wave][2][g], 1u); atomicAdd(&hist[wave][3][b], 1u); }
    }
    {
        unsigned long long v = sum_y;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((t & 63) == 0 && v) atomicAdd(&rec[f].sum_y, v);
    }
    __syncthreads();
    // bin t of every plane: the four waves' copies added; only thread t touches bin t from here on
    int h[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) h[p] = (int)(hist[0][p][t] + hist[1][p][t] + hist[2][p][t] + hist[3][p][t]);
    // whole-frame histograms of equalizeHist
    if (method == 1 || method == 3) {
        const int first = method == 3 ? 1 : 0;
        unsigned* gh = ghist + (int64_t)f * 3 * 256;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (h[first + c]) atomicAdd(&gh[c * 256 + t], (unsigned)h[first + c]);
    }
    if (method == 1) return;
    // CLAHE (clahe.cpp CLAHE_CalcLut_Body): clip, redistribute, prefix sum, scale
    const int n_planes = method == 2 ? 3 : 1;
    for (int p = 0; p < n_planes; ++p) {
        int v = h[p];
        if (a.clip > 0) {
            const int excess = v > a.clip ? v - a.clip : 0;
            const int clipped = eq_block_sum(excess, red);
            v = v > a.clip ? a.clip : v;
            const int batch = clipped / 256, residual = clipped - batch * 256;
            v += batch;
            if (residual != 0) {
                const int step = 256 / residual > 1 ? 256 / residual : 1;
                if (t % step == 0 && t / step < residual) ++v;
            }
        }
        const int sum = eq_block_scan(v, red);
        luts[(((int64_t)f * n_planes + p) * EQ_TILES + tile) * 256 + t] = (uint8_t)eq_lut_value(sum, a.lut_scale);
    }
}

// ---- apply.  Grid: blocks_per_frame blocks per frame.  NCL: CLAHE planes staged in LDS (method 0 / 3: 1, method 2: 3, method 1: 0). ----
struct EqFrameScalars { int gate; float w_yuv, w_rgb; };

// cl: the frame's staged tables [plane][tile][256]
__device__ __forceinline__ int eq_clahe_at(const uint8_t* cl, int plane, int v, int tx1, int tx2, int ty1, int ty2, float xa, float xa1, float ya, float ya1) {
    const uint8_t* p = cl + plane * EQ_TILES * 256 + v;
    return eq_interp(p[(ty1 * EQ_GRID + tx1) * 256], p[(ty1 * EQ_GRID + tx2) * 256], p[(ty2 * EQ_GRID + tx1) * 256], p[(ty2 * EQ_GRID + tx2) * 256], xa, xa1,
                     ya, ya1);
}

template <int METHOD>
__global__ void __launch_bounds__(EQ_THREADS) eq_apply_kernel(const uint8_t* __restrict__ clip, uint8_t* __restrict__ out, const EqFrameRec* rec,
                                                             const unsigned* ghist, const uint8_t* luts, EqArgs a) {
    constexpr int NCL = METHOD == 2 ? 3 : (METHOD == 1 ? 0 : 1);
    constexpr bool HAS_EQ = METHOD == 1 || METHOD == 3;
    __shared__ __attribute__((aligned(16))) uint8_t cl[NCL ? NCL * EQ_TILES * 256 : 16];
    __shared__ uint8_t pre[3][256], post[256], eq[HAS_EQ ? 3 : 1][256];
    __shared__ int red[4];
    __shared__ EqFrameScalars fs;
    const int f = (int)(blockIdx.x / (unsigned)a.blocks_per_frame), chunk = (int)(blockIdx.x % (unsigned)a.blocks_per_frame);
    const int t = threadIdx.x;
    const int64_t npix = (int64_t)a.h * a.w, ngroups = (npix + 3) >> 2;
    const uint8_t* src = clip + (int64_t)f * npix * 3;
    uint8_t* dst = out + (int64_t)f * npix * 3;
    eq_build_pre(pre, a, rec + f);
    post[t] = a.lut_out[t];
    if (t == 0) {
        const double fl = eq_f_luma(rec[f].sum_y, (long long)npix, a.range_tv);
        fs.gate = eq_gate(fl) ? 1 : 0;
        fs.w_yuv = a.luma_blend ? eq_blend_weight(fl, 0.40, 0.90, 0.35, 2.0) : -1.f;
        fs.w_rgb = a.luma_blend ? eq_blend_weight(fl, 0.40, 0.90, 0.15, 4.0) : -1.f;
    }
    __syncthreads();
    const bool gate = fs.gate != 0;               // the same for every thread of the block
    if (gate) {
        if (NCL) {
            const uint4* g = reinterpret_cast<const uint4*>(luts + (int64_t)f * NCL * EQ_TILES * 256);
            uint4* s = reinterpret_cast<uint4*>(cl);
            for (int i = t; i < NCL * EQ_TILES * 256 / 16; i += EQ_THREADS) s[i] = g[i];
        }
        if (HAS_EQ) {
            // cv::equalizeHist: skip to the first occupied bin i0, scale = 255 / (total - hist[i0]), lut[i] = saturate(cvRound(sum(hist[i0 + 1 .. i]) * scale));
            // a constant plane (total == hist[i0]) keeps its value
            for (int c = 0; c < 3; ++c) {
                const int hv = (int)ghist[((int64_t)f * 3 + c) * 256 + t];
                const int i0 = eq_block_min(hv ? t : 256, red);
                const int h0 = eq_block_sum(t == i0 ? hv : 0, red);
                const int sum = eq_block_scan(t > i0 ? hv : 0, red);
                int v;
                if ((int64_t)h0 == npix) v = t;
                else {
                    const float scale = 255.f / (float)(int)(npix - h0);
                    v = t <= i0 ? 0 : eq_lut_value(sum, scale);
                }
                eq[c][t] = (uint8_t)v;
            }
        }
    }
    __syncthreads();
    const float inv_tw = 1.0f / (float)a.tile_w, inv_th = 1.0f / (float)a.tile_h;
    const int lo = a.range_tv ? 16 : 0, hi = a.range_tv ? 235 : 255;
    const float w_yuv = fs.w_yuv, w_rgb = fs.w_rgb;
    for (int64_t i = (int64_t)chunk * EQ_THREADS + t; i < ngroups; i += (int64_t)a.blocks_per_frame * EQ_THREADS) {
        const bool full = i * 4 + 4 <= npix;
        const int cnt = full ? 4 : (int)(npix - i * 4);
        int px[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        if (full) {
            uint32_t w[3];
            __builtin_memcpy(w, src + i * 12, 12);
            eq_unpack(w, px);
        } else {
            for (int j = 0; j < cnt; ++j) { px[j][0] = src[(i * 4 + j) * 3]; px[j][1] = src[(i * 4 + j) * 3 + 1]; px[j][2] = src[(i * 4 + j) * 3 + 2]; }
        }
        int y = (int)((i * 4) / a.w), x = (int)((i * 4) - (int64_t)y * a.w);
        for (int j = 0; j < cnt; ++j) {
            const int r0 = pre[0][px[j][0]], g0 = pre[1][px[j][1]], b0 = pre[2][px[j][2]];
            int o[3] = {r0, g0, b0};
            if (gate) {
                int tx1 = 0, tx2 = 0, ty1 = 0, ty2 = 0;
                float xa = 0.f, xa1 = 0.f, ya = 0.f, ya1 = 0.f;
                if (NCL) { eq_tile_coord(x, inv_tw, tx1, tx2, xa, xa1); eq_tile_coord(y, inv_th, ty1, ty2, ya, ya1); }
                int m0[3] = {r0, g0, b0}, m1[3] = {r0, g0, b0};
                if (METHOD == 0 || METHOD == 3) {
                    int yy, u, v;
                    rgb2yuv(r0, g0, b0, yy, u, v);
                    int ye = eq_clahe_at(cl, 0, yy, tx1, tx2, ty1, ty2, xa, xa1, ya, ya1);
                    ye = ye < lo ? lo : (ye > hi ? hi : ye);
                    yuv2rgb(ye, u, v, m0[0], m0[1], m0[2]);
                    if (w_yuv >= 0.f) { m0[0] = eq_pil_blend(r0, m0[0], w_yuv); m0[1] = eq_pil_blend(g0, m0[1], w_yuv); m0[2] = eq_pil_blend(b0, m0[2], w_yuv); }
                }
                if (METHOD == 2) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        m0[c] = eq_clahe_at(cl, c, o[c], tx1, tx2, ty1, ty2, xa, xa1, ya, ya1);
                        if (w_rgb >= 0.f) m0[c] = eq_pil_blend(o[c], m0[c], w_rgb);
                    }
                }
                if (HAS_EQ) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        m1[c] = eq[c][o[c]];
                        if (w_rgb >= 0.f) m1[c] = eq_pil_blend(o[c], m1[c], w_rgb);
                    }
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int m = METHOD == 1 ? m1[c] : (METHOD == 3 ? eq_merge15(m0[c], m1[c], a.w3_15) : m0[c]);
                    o[c] = eq_merge15(m, o[c], a.w15);
                }
            }
            px[j][0] = post[o[0]]; px[j][1] = post[o[1]]; px[j][2] = post[o[2]];
            if (++x == a.w) { x = 0; ++y; }
        }
        if (full) {
            uint32_t w[3];
            eq_pack(px, w);
            __builtin_memcpy(dst + i * 12, w, 12);
        } else {
            for (int j = 0; j < cnt; ++j) { dst[(i * 4 + j) * 3] = (uint8_t)px[j][0]; dst[(i * 4 + j) * 3 + 1] = (uint8_t)px[j][1]; dst[(i * 4 + j) * 3 + 2] = (uint8_t)px[j][2]; }
        }
    }
}

size_t equalize_workspace_bytes(int n, int method) {
    const size_t n_cl = method == 2 ? 3 : (method == 1 ? 0 : 1);
    return (size_t)n * (sizeof(EqFrameRec) + 3 * 256 * sizeof(unsigned) + n_cl * EQ_TILES * 256);
}

static int eq_blocks_per_frame(int64_t npix) {
    // 32 groups = 128 pixels per thread and turn: a block that stages up to 48 KiB of tables should move several times that in pixels
    const int64_t b = (((npix + 3) >> 2) + 8191) / 8192;
    return (int)(b < 1 ? 1 : (b > 256 ? 256 : b));
}

// ws: equalize_workspace_bytes(n, method) bytes of device memory, 16-byte aligned; the records and the global histograms (the first
// n * (32 + 3072) bytes) ZERO-FILLED by the caller in front of the launch, on the same stream.  src == dst is allowed for nobody: the tile pass reads
// what the apply pass of another block may already have written -- the caller refuses it.
int launch_equalize(const uint8_t* src, uint8_t* dst, void* ws, EqArgs a, hipStream_t s) {
    const int64_t npix = (int64_t)a.h * a.w;
    if (a.n <= 0 || a.w < EQ_GRID || a.h < EQ_GRID || npix > ((int64_t)1 << 30) || a.method < 0 || a.method > 3) return (int)hipErrorInvalidValue;
    eq_tile_size(a.w, a.h, a.tile_w, a.tile_h);
    a.clip = eq_clip_limit(a.clip_limit, a.tile_w * a.tile_h);
    a.lut_scale = 255.f / (float)(a.tile_w * a.tile_h);
    a.blocks_per_frame = eq_blocks_per_frame(npix);
    if ((int64_t)a.n * a.blocks_per_frame > 0x7FFFFFFFll || (int64_t)a.n * EQ_TILES > 0x7FFFFFFFll) return (int)hipErrorInvalidValue;
    EqFrameRec* rec = (EqFrameRec*)ws;
    unsigned* ghist = (unsigned*)(rec + a.n);
    uint8_t* luts = (uint8_t*)(ghist + (size_t)a.n * 3 * 256);
    const dim3 grid((unsigned)((int64_t)a.n * a.blocks_per_frame)), block(EQ_THREADS);
    if (a.balance) hipLaunchKernelGGL(eq_chan_sum_kernel, grid, block, 0, s, src, rec, a);
    hipLaunchKernelGGL(eq_lut_kernel, dim3((unsigned)(a.n * EQ_TILES)), block, 0, s, src, rec, ghist, luts, a);
    switch (a.method) {
        case 0: hipLaunchKernelGGL((eq_apply_kernel<0>), grid, block, 0, s, src, dst, rec, ghist, luts, a); break;
        case 1: hipLaunchKernelGGL((eq_apply_kernel<1>), grid, block, 0, s, src, dst, rec, ghist, luts, a); break;
        case 2: hipLaunchKernelGGL((eq_apply_kernel<2>), grid, block, 0, s, src, dst, rec, ghist, luts, a); break;
        default: hipLaunchKernelGGL((eq_apply_kernel<3>), grid, block, 0, s, src, dst, rec, ghist, luts, a); break;
    }
    return (int)hipGetLastError();
}

// the channel sums alone (HAVC_adjust_rgb's normalisation): identity table, rec[f].chan only
int launch_equalize_chan_sums(const uint8_t* src, void* rec, int n, int h, int w, hipStream_t s) {
    const int64_t npix = (int64_t)h * w;
    if (n <= 0 || h <= 0 || w <= 0 || npix > ((int64_t)1 << 30)) return (int)hipErrorInvalidValue;
    EqArgs a{};
    a.n = n; a.h = h; a.w = w;
    for (int v = 0; v < 256; ++v) a.lut_in[v] = (uint8_t)v;
    a.blocks_per_frame = eq_blocks_per_frame(npix);
    if ((int64_t)n * a.blocks_per_frame > 0x7FFFFFFFll) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(eq_chan_sum_kernel, dim3((unsigned)((int64_t)n * a.blocks_per_frame)), dim3(EQ_THREADS), 0, s, src, (EqFrameRec*)rec, a);
    return (int)hipGetLastError();
}

void preload_equalize() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(eq_lut_kernel)); (void)hipGetLastError(); }
