// HAVC_tweak (vsdeoldify/__init__.py:1377-1408 -> vs_tweak, vsslib/vsfilters.py:753-850) and HAVC_adjust_rgb (:1342-1374) on a clip [n][h][w][3] in HBM.
// vs_tweak takes the clip through YUV420P8 and back; zimg cannot be executed where the fixtures are made, so both directions are a stand-in with one
// written definition, tests/tweak_util.py, which these kernels equal byte for byte (tweak_ops.h has the arithmetic; this file is built with
// -ffp-contract=off: a fused a * b + c changes the bytes).
//     tweak_forward_kernel   RGB24 -> Y plane and the U, V quarter planes.  A block owns 16 x 32 chroma samples = 32 x 64 pixels: the float Cb / Cr of the tile
//                            and of its 8-tap halo (38 x 70) go to LDS through the optional gamma table, Y is quantised, sent through the optional luma table
//                            and stored; the vertical pass writes 16 x 70 floats back into LDS, the horizontal pass reads them, quantises, applies the
//                            hue / sat expression and stores.  One launch for all frames of a chunk.
//     tweak_back_kernel      Y, U, V -> RGB24: chroma 1 : 2, the inverse matrix and the error diffusion in one kernel; the float planes never reach HBM.
//                            One block per frame; waves 0..2 walk one channel each, all 16 waves stage and flush.  The diffusion is a skewed
//                            wavefront: lane l owns row r0 + l of a 64-row band and works on column t - 2 l at step t, so the three errors it needs from the row above are the last three results of lane l - 1:
//                            the newest comes over by a whole-wave shift by one lane (DPP wave_shr:1), the other two are what came over one and two steps
//                            earlier, kept in registers.  Lane 0 takes its row above from `erow` (LDS, w floats per channel), where lane 63 left the last
//                            row of the band before; reads run 127 columns ahead of the writes, so one row serves both.  A band goes through in chunks of 64
//                            steps: the block computes the chunk's 64 x 64 x 3 float samples (a parallelogram of the frame) into LDS coalesced -- vertical
//                            chroma pass, then horizontal pass and matrix -- each wave runs its 64 steps reading its lane's row of that tile and writing
//                            bytes into an LDS tile of interleaved RGB, and the block flushes that tile row by row.
//                            KEPT: bands one after the other, one walking wave per plane, 16 waves staging (7.7 ms for 64 frames of 1080p).  REJECTED:
//                            a block of the three walking waves alone (18.8 ms: the staging passes waited for their own global loads).  Pipelining
//                            several bands of a plane across the waves of a block was not built (profiles/tweak.txt, DESIGN.md section 4 "Tweak").
//     tweak_back_indexed_kernel, tweak_forward_restore_kernel   the same two bodies for havc_chroma_stab_clip (chroma_stab.hip): the back conversion with Y of
//                            frame yidx[f] and U, V of frame cidx[f] (the shifted clips of vs_get_clip_frame need no gathered planes), and the forward one
//                            with restore_color's pixel (pixel_ops.h) computed in the load, U and V stored only.  The templates leave the plain kernels'
//                            code as it was.
//     adjust_tables_kernel   HAVC_adjust_rgb is a function of the sample's own value and the frame's channel means: normalise (gain from the means),
//                            std.Merge by strength, "x r * rb +", gamma.  One block per frame composes the 3 x 256 bytes from the channel sums in float64;
//                            nothing is read back.
//     lut3_apply_kernel      applies a frame's three tables; a thread owns four pixels = 12 bytes (as equalize.hip).
#include "kernels.h"
#include "equalize_ops.h"
#include "tweak_ops.h"
#include "pixel_ops.h"
#include "chroma_stab_ops.h"

// ---- forward ------------------------------------------------------------------------------------------------------------------------------------------------
#define TWF_TH 16                                  // chroma rows of a tile
#define TWF_TW 32                                  // chroma columns
#define TWF_LH (2 * TWF_TH + TW_DOWN_TAPS - 2)     // 38 pixel rows: local row ly is pixel row 2 * TWF_TH * by + TW_DOWN_FIRST + ly
#define TWF_LW (2 * TWF_TW + TW_DOWN_TAPS - 2)     // 70
#define TWF_PITCH (TWF_LW + 1)
#define TWF_THREADS 256

// RESTORE (havc_chroma_stab_clip, chroma_stab.hip): frame f of `src` is a shifted clip's frame; what enters the matrix is restore_color's pixel (pixel_ops.h
// restore_binary_pixel) of it and of frame color_idx[f] of ra.color, unless the frame passes as it is (mode[f] == 0, or the tht_scen gate taken from the
// frame's two integer sums: chroma_stab_ops.h, block-uniform).  The restored frame exists in registers only; Y is not stored.
template <bool RESTORE>
__device__ __forceinline__ void tweak_forward_body(const uint8_t* __restrict__ src, uint8_t* __restrict__ yp, uint8_t* __restrict__ up,
                                                   uint8_t* __restrict__ vp, const TweakFwdArgs& a, const TweakRestoreArgs& ra) {
    __shared__ float cc[2][TWF_LH][TWF_PITCH];     // Cb, Cr of the tile and its halo
    __shared__ float vv[2][TWF_TH][TWF_PITCH];     // after the vertical pass
    __shared__ float unit[256];                    // sample / 255
    __shared__ uint8_t gam[256], lum[256];
    const int t = threadIdx.x, f = blockIdx.z;
    const int h = a.h, w = a.w, ch = h >> 1, cw = w >> 1;
    const int j0 = blockIdx.y * TWF_TH, i0 = blockIdx.x * TWF_TW;
    unit[t] = (float)t / 255.f;
    gam[t] = a.has_gamma ? a.gamma_lut[t] : (uint8_t)t;
    lum[t] = a.has_luma ? a.luma_lut[t] : (uint8_t)t;
    __syncthreads();
    const uint8_t* frame = src + (int64_t)f * h * w * 3;
    uint8_t* yf = RESTORE ? nullptr : yp + (int64_t)f * h * w;
    const uint8_t* cframe = nullptr;
    bool restore = false;
    double rweight = 0.0;
    if constexpr (RESTORE) {
        cframe = ra.color + (int64_t)ra.color_idx[f] * h * w * 3;
        if (ra.mode[f]) restore = !cs_frame_decision(ra.stats[2 * f], ra.stats[2 * f + 1], (long long)h * w, ra.weight, ra.tht_scen, rweight);
    }
    for (int idx = t; idx < TWF_LH * TWF_LW; idx += TWF_THREADS) {
        const int ly = idx / TWF_LW, lx = idx - ly * TWF_LW;
        const int py = 2 * j0 + TW_DOWN_FIRST + ly, px = 2 * i0 + TW_DOWN_FIRST + lx;
        float cb = 0.f, cr = 0.f;
        if (py < h + TW_DOWN_TAPS && px < w + TW_DOWN_TAPS) {                 // beyond that no sample of the plane has a tap
            const int my = tw_mirror(py, h), mx = tw_mirror(px, w);
            const int64_t po = ((int64_t)my * w + mx) * 3;
            const uint8_t* p = frame + po;
            int px3[3] = {p[0], p[1], p[2]};
            if constexpr (RESTORE) {
                if (restore) {
                    const uint8_t* q = cframe + po;
                    int o[3];
                    restore_binary_pixel(q[0], q[1], q[2], px3[0], px3[1], px3[2], ra.sat, ra.tht, rweight, 0, o);
                    px3[0] = o[0]; px3[1] = o[1]; px3[2] = o[2];
                }
            }
            float y;
            tw_rgb2ycc(unit[gam[px3[0]]], unit[gam[px3[1]]], unit[gam[px3[2]]], y, cb, cr);
            if (!RESTORE && my == py && mx == px && ly >= -TW_DOWN_FIRST && ly < -TW_DOWN_FIRST + 2 * TWF_TH && lx >= -TW_DOWN_FIRST && lx < -TW_DOWN_FIRST + 2 * TWF_TW)
                yf[(int64_t)py * w + px] = lum[tw_quant_y(y)];
        }
        cc[0][ly][lx] = cb;
        cc[1][ly][lx] = cr;
    }
    __syncthreads();
    for (int idx = t; idx < TWF_TH * TWF_LW; idx += TWF_THREADS) {
        const int j = idx / TWF_LW, lx = idx - j * TWF_LW;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            float acc = a.wt.down_v[0] * cc[p][2 * j][lx];
#pragma unroll
            for (int k = 1; k < TW_DOWN_TAPS; ++k) acc = acc + a.wt.down_v[k] * cc[p][2 * j + k][lx];
            vv[p][j][lx] = acc;
        }
    }
    __syncthreads();
    for (int idx = t; idx < TWF_TH * TWF_TW; idx += TWF_THREADS) {
        const int j = idx / TWF_TW, i = idx - j * TWF_TW;
        if (j0 + j >= ch || i0 + i >= cw) continue;
        float acc[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            acc[p] = a.wt.down_h[0] * vv[p][j][2 * i];
#pragma unroll
            for (int k = 1; k < TW_DOWN_TAPS; ++k) acc[p] = acc[p] + a.wt.down_h[k] * vv[p][j][2 * i + k];
        }
        int u = tw_quant_c(acc[0]), v = tw_quant_c(acc[1]);
        if (a.has_hue_sat) tw_hue_sat(u, v, a.hue_c, a.hue_s, u, v);
        const int64_t o = ((int64_t)f * ch + j0 + j) * cw + i0 + i;
        up[o] = (uint8_t)u;
        vp[o] = (uint8_t)v;
    }
}

__global__ void __launch_bounds__(TWF_THREADS) tweak_forward_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ yp, uint8_t* __restrict__ up,
                                                                   uint8_t* __restrict__ vp, TweakFwdArgs a) {
    tweak_forward_body<false>(src, yp, up, vp, a, TweakRestoreArgs{});
}
__global__ void __launch_bounds__(TWF_THREADS) tweak_forward_restore_kernel(const uint8_t* __restrict__ gray, uint8_t* __restrict__ up, uint8_t* __restrict__ vp,
                                                                           TweakFwdArgs a, TweakRestoreArgs ra) {
    tweak_forward_body<true>(gray, nullptr, up, vp, a, ra);
}

int launch_tweak_forward(const uint8_t* src, uint8_t* y, uint8_t* u, uint8_t* v, TweakFwdArgs a, hipStream_t s) {
    if (a.n <= 0 || a.n > 65535 || a.h < 2 || a.w < 2 || (a.h & 1) || (a.w & 1) || a.h > TW_MAX_SIDE || a.w > TW_MAX_SIDE) return (int)hipErrorInvalidValue;
    tw_all_weights(a.wt);
    const dim3 grid((unsigned)((a.w / 2 + TWF_TW - 1) / TWF_TW), (unsigned)((a.h / 2 + TWF_TH - 1) / TWF_TH), (unsigned)a.n);
    hipLaunchKernelGGL(tweak_forward_kernel, grid, dim3(TWF_THREADS), 0, s, src, y, u, v, a);
    return (int)hipGetLastError();
}

// gray: a.n frames; U and V of frame f go to u / v + f * (h / 2) * (w / 2).  The tables of a are off (identity).
int launch_tweak_forward_restore(const uint8_t* gray, uint8_t* u, uint8_t* v, TweakFwdArgs a, TweakRestoreArgs ra, hipStream_t s) {
    if (a.n <= 0 || a.n > 65535 || a.h < 2 || a.w < 2 || (a.h & 1) || (a.w & 1) || a.h > TW_MAX_SIDE || a.w > TW_MAX_SIDE) return (int)hipErrorInvalidValue;
    a.has_gamma = a.has_luma = a.has_hue_sat = false;
    tw_all_weights(a.wt);
    const dim3 grid((unsigned)((a.w / 2 + TWF_TW - 1) / TWF_TW), (unsigned)((a.h / 2 + TWF_TH - 1) / TWF_TH), (unsigned)a.n);
    hipLaunchKernelGGL(tweak_forward_restore_kernel, grid, dim3(TWF_THREADS), 0, s, gray, u, v, a, ra);
    return (int)hipGetLastError();
}

// ---- back ---------------------------------------------------------------------------------------------------------------------------------------------------
#define TWB_ROWS 64                                // rows of a band = lanes of a wave
#define TWB_T 64                                   // steps of a chunk
#define TWB_XP (TWB_T + 1)                         // floats per lane row of the sample tile: lane l reads bank (65 l + j) % 32, all different
#define TWB_VC (TWB_T / 2 + 3)                     // 35 chroma columns under the 64 pixel columns of a chunk row
#define TWB_VP (TWB_VC + 1)
#define TWB_OP (TWB_T * 3 + 4)                     // bytes per lane row of the output tile: 49 dwords, lane l writes bank (49 l + ..) % 32
#define TWB_THREADS 1024                           // 16 waves stage and flush; waves 0..2 walk the wavefront, one channel each
#define TWB_ITER(n) (((n) + TWB_THREADS - 1) / TWB_THREADS)

// lane l <- lane l - 1, lane 0 <- 0: DPP wave_shr:1 with an old value of 0 and bound_ctrl off
__device__ __forceinline__ float tw_from_lane_above(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, false));
}

// INDEXED (havc_chroma_stab_clip's shifted clips): output frame f takes Y from frame yidx[f] and U, V from frame cidx[f] of the planes
template <bool INDEXED>
__device__ __forceinline__ void tweak_back_body(const uint8_t* __restrict__ yp, const uint8_t* __restrict__ up, const uint8_t* __restrict__ vp,
                                                uint8_t* __restrict__ dst, const TweakBackArgs& a, const int* __restrict__ yidx, const int* __restrict__ cidx) {
    __shared__ float erow[3][TW_MAX_SIDE];         // the error row a band hands to the next one, per channel
    __shared__ float xs[3][TWB_ROWS][TWB_XP];      // the chunk's samples: xs[c][l][j] = channel c at row r0 + l, column t0 - 2 l + j
    __shared__ float vb[2][TWB_ROWS][TWB_VP];      // Cb, Cr after the vertical pass: vb[p][l][jj] = chroma column (t0 / 2 - l) - 1 + jj
    __shared__ uint8_t ob[TWB_ROWS][TWB_OP];       // the chunk's bytes, interleaved
    __shared__ float unit[256], cunit[256];        // y / 255, (c - 128) / 255
    const int tid = threadIdx.x, lane = tid & 63, f = blockIdx.x;
    const bool walker = (tid >> 6) < 3;            // wave-uniform
    const int c = walker ? tid >> 6 : 0;
    const int h = a.h, w = a.w, ch = h >> 1, cw = w >> 1;
    const int fy = INDEXED ? yidx[f] : f, fc = INDEXED ? cidx[f] : f;
    const uint8_t* yf = yp + (int64_t)fy * h * w;
    const uint8_t* cf[2] = {up + (int64_t)fc * ch * cw, vp + (int64_t)fc * ch * cw};
    uint8_t* df = dst + (int64_t)f * h * w * 3;
    if (tid < 256) { unit[tid] = (float)tid / 255.f; cunit[tid] = ((float)tid - 128.f) / 255.f; }
    for (int i = tid; i < 3 * w; i += TWB_THREADS) erow[i / w][i % w] = 0.f;
    __syncthreads();
    float* er = erow[c];
    for (int r0 = 0; r0 < h; r0 += TWB_ROWS) {
        const int rows = min(TWB_ROWS, h - r0), steps = w + 2 * (rows - 1);
        const bool row_ok = lane < rows;
        float left = 0.f, top = lane == 0 ? er[0] : 0.f, topleft = 0.f;
        for (int t0 = 0; t0 < steps; t0 += TWB_T) {
            // the vertical chroma pass under the chunk.  The loops of both passes have constant trip counts and are unrolled: a thread's global loads of
            // all its turns are in flight together (a block is the only one on its CU; nothing else hides their latency)
#pragma unroll
            for (int it = 0; it < TWB_ITER(2 * TWB_ROWS * TWB_VC); ++it) {
                const int idx = tid + it * TWB_THREADS;
                if (idx >= 2 * TWB_ROWS * TWB_VC) break;
                const int p = idx / (TWB_ROWS * TWB_VC), rem = idx - p * (TWB_ROWS * TWB_VC);
                const int l = rem / TWB_VC, jj = rem - l * TWB_VC;
                const int row = r0 + l, pc = (t0 >> 1) - l - 1 + jj;
                float acc = 0.f;
                if (row < h && pc >= -2 && pc <= cw + 1) {                   // the taps of chroma columns 0 .. cw - 1 reach no further
                    const int mx = tw_mirror(pc, cw), par = row & 1, base = (row >> 1) + (par ? TW_UP_FIRST_V_ODD : TW_UP_FIRST_V_EVEN);
                    acc = a.wt.up_v[par][0] * cunit[cf[p][(int64_t)tw_mirror(base, ch) * cw + mx]];
#pragma unroll
                    for (int k = 1; k < TW_UP_TAPS; ++k) acc = acc + a.wt.up_v[par][k] * cunit[cf[p][(int64_t)tw_mirror(base + k, ch) * cw + mx]];
                }
                vb[p][l][jj] = acc;
            }
            // the Y samples of the chunk, asked for before the barrier
            int yv[TWB_ITER(TWB_ROWS * TWB_T)];
#pragma unroll
            for (int it = 0; it < TWB_ITER(TWB_ROWS * TWB_T); ++it) {
                const int idx = tid + it * TWB_THREADS, l = idx >> 6, j = idx & 63;
                const int row = r0 + l, col = t0 - 2 * l + j;
                yv[it] = (row < h && col >= 0 && col < w) ? (int)yf[(int64_t)row * w + col] : -1;
            }
            __syncthreads();
            // the horizontal pass and the matrix
#pragma unroll
            for (int it = 0; it < TWB_ITER(TWB_ROWS * TWB_T); ++it) {
                const int idx = tid + it * TWB_THREADS, l = idx >> 6, j = idx & 63;
                float r = 0.f, g = 0.f, b = 0.f;
                if (yv[it] >= 0) {
                    const int par = j & 1, jb = (j >> 1) + 1 + TW_UP_FIRST_H;        // t0 - 2 l is even: the column's parity is j's
                    float cbr[2];
#pragma unroll
                    for (int p = 0; p < 2; ++p) {
                        cbr[p] = a.wt.up_h[par][0] * vb[p][l][jb];
#pragma unroll
                        for (int k = 1; k < TW_UP_TAPS; ++k) cbr[p] = cbr[p] + a.wt.up_h[par][k] * vb[p][l][jb + k];
                    }
                    tw_ycc2rgb(unit[yv[it]], cbr[0], cbr[1], r, g, b);
                }
                xs[0][l][j] = r; xs[1][l][j] = g; xs[2][l][j] = b;
            }
            __syncthreads();
            // 64 steps of the wavefront, one channel per wave
            if (walker) {
                const float ahead = t0 + 1 + lane < w ? er[t0 + 1 + lane] : 0.f;      // lane 0's top-right errors of this chunk, one per lane
                float hand = 0.f;                                                       // lane 63's errors of this chunk, one per lane
#pragma unroll 8
                for (int j = 0; j < TWB_T; ++j) {
                    const int col = t0 + j - 2 * lane;
                    const bool valid = row_ok && col >= 0 && col < w;
                    const float above = tw_from_lane_above(left);
                    const float first = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ahead), j));
                    const float topright = lane == 0 ? first : above;
                    float q;
                    const float e = tw_diffuse(xs[c][lane][j], left, topright, top, topleft, q);
                    topleft = top;
                    top = topright;
                    left = valid ? e : 0.f;
                    const float last = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(left), TWB_ROWS - 1));
                    if (lane == j) hand = last;
                    ob[lane][j * 3 + c] = (uint8_t)(int)q;
                }
                if (rows == TWB_ROWS) {
                    const int col = t0 + lane - 2 * (TWB_ROWS - 1);
                    if (col >= 0 && col < w) er[col] = hand;
                }
            }
            __syncthreads();
            // flush: row l of the tile is 192 consecutive bytes of the frame
            for (int idx = tid; idx < rows * TWB_T * 3; idx += TWB_THREADS) {
                const int l = idx / (TWB_T * 3), b = idx - l * (TWB_T * 3);
                const int col = t0 - 2 * l + b / 3;
                if (col >= 0 && col < w) df[((int64_t)(r0 + l) * w + t0 - 2 * l) * 3 + b] = ob[l][b];
            }
        }
    }
}

__global__ void __launch_bounds__(TWB_THREADS) tweak_back_kernel(const uint8_t* __restrict__ yp, const uint8_t* __restrict__ up, const uint8_t* __restrict__ vp,
                                                                uint8_t* __restrict__ dst, TweakBackArgs a) {
    tweak_back_body<false>(yp, up, vp, dst, a, nullptr, nullptr);
}
__global__ void __launch_bounds__(TWB_THREADS) tweak_back_indexed_kernel(const uint8_t* __restrict__ yp, const uint8_t* __restrict__ up,
                                                                        const uint8_t* __restrict__ vp, uint8_t* __restrict__ dst, TweakBackArgs a,
                                                                        const int* __restrict__ yidx, const int* __restrict__ cidx) {
    tweak_back_body<true>(yp, up, vp, dst, a, yidx, cidx);
}

int launch_tweak_back_indexed(const uint8_t* y, const uint8_t* u, const uint8_t* v, uint8_t* dst, const int* yidx, const int* cidx, TweakBackArgs a,
                              hipStream_t s) {
    if (a.n <= 0 || a.h < 2 || a.w < 2 || (a.h & 1) || (a.w & 1) || a.h > TW_MAX_SIDE || a.w > TW_MAX_SIDE || !yidx || !cidx) return (int)hipErrorInvalidValue;
    tw_all_weights(a.wt);
    hipLaunchKernelGGL(tweak_back_indexed_kernel, dim3((unsigned)a.n), dim3(TWB_THREADS), 0, s, y, u, v, dst, a, yidx, cidx);
    return (int)hipGetLastError();
}

int launch_tweak_back(const uint8_t* y, const uint8_t* u, const uint8_t* v, uint8_t* dst, TweakBackArgs a, hipStream_t s) {
    if (a.n <= 0 || a.h < 2 || a.w < 2 || (a.h & 1) || (a.w & 1) || a.h > TW_MAX_SIDE || a.w > TW_MAX_SIDE) return (int)hipErrorInvalidValue;
    tw_all_weights(a.wt);
    hipLaunchKernelGGL(tweak_back_kernel, dim3((unsigned)a.n), dim3(TWB_THREADS), 0, s, y, u, v, dst, a);
    return (int)hipGetLastError();
}

// ---- HAVC_adjust_rgb ------------------------------------------------------------------------------------------------------------------------------------------
#define ADJ_THREADS 256

// tables[f][c][v]: block f, thread v
__global__ void __launch_bounds__(ADJ_THREADS) adjust_tables_kernel(const EqFrameRec* __restrict__ rec, uint8_t* __restrict__ tables, AdjustArgs a) {
    const int f = blockIdx.x, v = threadIdx.x;
    double gain[3] = {1.0, 1.0, 1.0};
    if (a.mode) tw_normalize_gains(rec[f].chan, (long long)a.h * a.w, gain);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int s = v;
        if (a.mode) {
            const int nv = eq_expr_mul(v, (float)gain[c]);
            s = a.mode == 1 ? nv : eq_merge15(v, nv, a.w15);
        }
        tables[((int64_t)f * 3 + c) * 256 + v] = a.gamma_lut[c][tw_affine(s, a.gain[c], a.bias[c])];
    }
}

__global__ void __launch_bounds__(ADJ_THREADS) lut3_apply_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const uint8_t* __restrict__ tables,
                                                                AdjustArgs a) {
    __shared__ uint8_t tab[3][256];
    const int f = (int)(blockIdx.x / (unsigned)a.blocks_per_frame), part = (int)(blockIdx.x % (unsigned)a.blocks_per_frame);
    const int t = threadIdx.x;
    const int64_t npix = (int64_t)a.h * a.w, ngroups = (npix + 3) >> 2;
    const uint8_t* s = src + (int64_t)f * npix * 3;
    uint8_t* d = dst + (int64_t)f * npix * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) tab[c][t] = tables[((int64_t)f * 3 + c) * 256 + t];
    __syncthreads();
    for (int64_t i = (int64_t)part * ADJ_THREADS + t; i < ngroups; i += (int64_t)a.blocks_per_frame * ADJ_THREADS) {
        if (i * 4 + 4 <= npix) {
            uint8_t b[12];
            __builtin_memcpy(b, s + i * 12, 12);
#pragma unroll
            for (int k = 0; k < 12; ++k) b[k] = tab[k % 3][b[k]];
            __builtin_memcpy(d + i * 12, b, 12);
        } else {
            for (int64_t p = i * 12; p < npix * 3; ++p) d[p] = tab[p % 3][s[p]];
        }
    }
}

int launch_adjust_rgb(const uint8_t* src, uint8_t* dst, void* rec, uint8_t* tables, AdjustArgs a, hipStream_t s) {
    const int64_t npix = (int64_t)a.h * a.w;
    if (a.n <= 0 || a.h <= 0 || a.w <= 0 || npix > ((int64_t)1 << 30) || a.mode < 0 || a.mode > 2) return (int)hipErrorInvalidValue;
    const int64_t b = (((npix + 3) >> 2) + 8191) / 8192;
    a.blocks_per_frame = (int)(b < 1 ? 1 : (b > 256 ? 256 : b));
    if ((int64_t)a.n * a.blocks_per_frame > 0x7FFFFFFFll) return (int)hipErrorInvalidValue;
    if (a.mode) {
        const int e = launch_equalize_chan_sums(src, rec, a.n, a.h, a.w, s);
        if (e) return e;
    }
    hipLaunchKernelGGL(adjust_tables_kernel, dim3((unsigned)a.n), dim3(ADJ_THREADS), 0, s, (const EqFrameRec*)rec, tables, a);
    hipLaunchKernelGGL(lut3_apply_kernel, dim3((unsigned)((int64_t)a.n * a.blocks_per_frame)), dim3(ADJ_THREADS), 0, s, src, dst, (const uint8_t*)tables, a);
    return (int)hipGetLastError();
}

void preload_tweak_clip() { hipFuncAttributes at; (void)hipFuncGetAttributes(&at, reinterpret_cast<const void*>(tweak_back_kernel)); (void)hipGetLastError(); }
