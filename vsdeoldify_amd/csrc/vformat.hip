// convert_format_RGB24 / restore_format (vsdeoldify/havc_utils.py:57-237) on a clip's own planes: YUV 4:2:0 / 4:2:2 / 4:4:4 or GRAY, 8..16 bit, limited or
// full range, BT.709 / 470BG / 170M / 2020 NCL  <->  RGB24 [n][h][w][3].  zimg cannot be executed where the fixtures are made: both directions are an
// UNPINNED stand-in with one written definition, tests/vformat_util.py (on top of tests/tweak_util.py: the same Mitchell resampler, mirroring and Floyd -
// Steinberg weights), which these kernels equal byte for byte.  vformat_ops.h has the arithmetic and writes the scalings down; this file is built with
// -ffp-contract=off.  At BT.709 / full range / 8 bit / 4:2:0 the bytes are those of tweak.hip's two kernels, whose code is untouched.
//     vf_back_kernel<T, SW, SH>   planes -> RGB24.  tweak_back_kernel's design: one block per frame, waves 0..2 walk the error diffusion of one channel each
//                            as a skewed wavefront (lane l owns row r0 + l of a 64-row band, errors cross lanes by DPP wave_shr:1, `erow` hands a band's last
//                            row to the next band), all 16 waves stage a chunk of 64 steps -- vertical chroma pass, horizontal pass, matrix -- into LDS and
//                            flush the interleaved bytes.  Generalised: T = uint8_t / uint16_t loads through the depth step (vf_code8: > 8 bit planes go to 8
//                            bit first, as the reference does in a call of its own), the unit tables carry the range, the matrix comes as constants, SH = 0
//                            drops the vertical pass (4:2:2), SW = 0 the chroma staging altogether (4:4:4).  dither = 0: the walk is replaced by a plain
//                            rounding of the staged samples and the bands of a frame become blocks of their own (grid y).
//     vf_gray_kernel<T>      GRAY -> RGB24: limited -> full on the 8-bit code, no dither (the reference asks for none), a thread per pixel.
//     vf_fwd_kernel<T, SW, SH>    RGB24 -> planes with error diffusion.  Y is diffused over w x h, U and V each over their own cw x ch plane in raster order,
//                            so the three planes are three independent problems: one block per (frame, plane), ONE walking wave, 16 waves staging.  The
//                            walk is the back kernel's (same DPP hand-over, same `erow`), clamped to [0, 2^bits - 1].  Staging a chunk of a chroma plane:
//                            lane row l needs the 2 : 1 horizontal pass over 64 + 7 taps = 134 pixel columns, each the 8-tap vertical pass over Cb (or Cr)
//                            of the RGB pixels read straight from HBM / L2 (`vbuf`), then the horizontal pass and the scaling into `xs`.  The float planes
//                            never reach HBM.  The Y block's staging is the matrix alone.  The vertical pass recomputes the matrix per tap (8 x per staged column):
//                            the chroma blocks do about 17 matrix evaluations per output sample.  Accepted: a block is bound by the 64 dependent steps of
//                            its one walking wave per chunk, which the other 15 waves' staging only has to keep up with.
//     vf_fwd_tiled_kernel<T, SW, SH>   RGB24 -> planes with dither = 0: nothing is carried from sample to sample, so this is tweak_forward_kernel's body --
//                            a block owns 16 x 32 chroma samples, Cb / Cr of the tile and its halo in LDS, vertical pass, horizontal pass -- with the
//                            matrix, the scaling and the depth as parameters and the passes dropped where the chroma is not subsampled.
// LDS per block (160 KiB per CU, one block of 1024 threads per CU either way):
//     vf_back_kernel   erow 3 x 4096 x 4 = 48 KiB, xs 3 x 64 x 65 x 4 = 48.75 KiB, vb 2 x 64 x 36 x 4 = 18 KiB, ob 64 x 196 = 12.25 KiB, tables 2 KiB: 129 KiB
//                      (tweak_back_kernel's budget)
//     vf_fwd_kernel    erow 4096 x 4 = 16 KiB, xs 64 x 65 x 4 = 16.25 KiB, vbuf 64 x 135 x 4 = 33.75 KiB, ob 64 x 66 x 2 = 8.25 KiB, unit 1 KiB: 75.25 KiB
//     vf_fwd_tiled_kernel   cc 2 x 38 x 71 x 4 = 21.1 KiB, vv 2 x 16 x 71 x 4 = 8.9 KiB, unit 1 KiB: 31 KiB at 4:2:0 (tweak_forward_kernel's), less otherwise
// Bank notes (ds_read_b32 / ds_write_b32: bank = dword address mod 32, groups of 32 lanes): xs rows are 65 dwords, so the walker's lane l reads bank
// (65 l + j) mod 32, all different; vbuf rows are 135 dwords (odd), the horizontal pass reads vbuf[l][2 j + k] with j the fast index: stride 2 dwords, a
// 2-way conflict per half wave, accepted (the pass is 8 reads per sample behind 134 x 8 global loads per row).
#include "kernels.h"
#include "vformat_ops.h"

#define VF_ROWS 64                                 // rows of a band = lanes of a wave
#define VF_T 64                                    // steps of a chunk
#define VF_XP (VF_T + 1)
#define VF_VC (VF_T / 2 + 3)                       // back: 35 chroma columns under the 64 pixel columns of a chunk row
#define VF_VP (VF_VC + 1)
#define VF_OP (VF_T * 3 + 4)
#define VF_DC (2 * VF_T + TW_DOWN_TAPS - 2)        // forward: 134 pixel columns over the 64 chroma columns of a chunk row
#define VF_DP (VF_DC + 1)
#define VF_OW (VF_T + 2)                           // forward: uint16 codes per lane row of the output tile
#define VF_THREADS 1024
#define VF_ITER(n) (((n) + VF_THREADS - 1) / VF_THREADS)

// lane l <- lane l - 1, lane 0 <- 0: DPP wave_shr:1 with an old value of 0 and bound_ctrl off
__device__ __forceinline__ float vf_from_lane_above(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, false));
}

// 64 steps of the skewed wavefront over xs_row (this lane's row of the chunk's samples), one wave: see tweak_back_kernel.  store(j, q) keeps the code.
template <typename Store>
__device__ __forceinline__ void vf_walk_chunk(const float* xs_row, float* er, int t0, int w, int rows, int lane, float hi, float& left, float& top, float& topleft,
                                              Store store) {
    const bool row_ok = lane < rows;
    const float ahead = t0 + 1 + lane < w ? er[t0 + 1 + lane] : 0.f;              // lane 0's top-right errors of this chunk, one per lane
    float hand = 0.f;                                                               // lane 63's errors of this chunk, one per lane
#pragma unroll 8
    for (int j = 0; j < VF_T; ++j) {
        const int col = t0 + j - 2 * lane;
        const bool valid = row_ok && col >= 0 && col < w;
        const float above = vf_from_lane_above(left);
        const float first = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ahead), j));
        const float topright = lane == 0 ? first : above;
        float q;
        const float e = vf_diffuse(xs_row[j], left, topright, top, topleft, hi, q);
        topleft = top;
        top = topright;
        left = valid ? e : 0.f;
        const float last = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(left), VF_ROWS - 1));
        if (lane == j) hand = last;
        store(j, (int)q);
    }
    if (rows == VF_ROWS) {
        const int col = t0 + lane - 2 * (VF_ROWS - 1);
        if (col >= 0 && col < w) er[col] = hand;
    }
}

// ---- planes -> RGB24 ------------------------------------------------------------------------------------------------------------------------------------------
template <typename T, int SW, int SH>
__global__ void __launch_bounds__(VF_THREADS) vf_back_kernel(const T* __restrict__ yp, const T* __restrict__ up, const T* __restrict__ vp, uint8_t* __restrict__ dst,
                                                             VfArgs a) {
    __shared__ float erow[3][TW_MAX_SIDE];
    __shared__ float xs[3][VF_ROWS][VF_XP];        // xs[c][l][j] = channel c at row r0 + l, column t0 - 2 l + j
    __shared__ float vb[2][VF_ROWS][VF_VP];        // SW: Cb, Cr after the vertical pass, vb[p][l][jj] = chroma column (t0 / 2 - l) - 1 + jj
    __shared__ uint8_t ob[VF_ROWS][VF_OP];
    __shared__ float unit[256], cunit[256];        // (y - y_off) / y_scale, (c - 128) / c_scale on 8-bit codes
    const int tid = threadIdx.x, lane = tid & 63, f = blockIdx.x;
    const bool walker = (tid >> 6) < 3;            // wave-uniform
    const int c = walker ? tid >> 6 : 0;
    const int h = a.h, w = a.w, ch = h >> SH, cw = w >> SW;
    const T* yf = yp + (int64_t)f * h * w;
    const T* cf[2] = {up + (int64_t)f * ch * cw, vp + (int64_t)f * ch * cw};
    uint8_t* df = dst + (int64_t)f * h * w * 3;
    if (tid < 256) { unit[tid] = ((float)tid - a.y_off) / a.y_scale; cunit[tid] = ((float)tid - 128.f) / a.c_scale; }
    for (int i = tid; i < 3 * w; i += VF_THREADS) erow[i / w][i % w] = 0.f;
    __syncthreads();
    float* er = erow[c];
    // dither: every band of the frame, one after the other; no dither: the band of this block
    const int r_first = a.dither ? 0 : (int)blockIdx.y * VF_ROWS, r_end = a.dither ? h : min(h, r_first + VF_ROWS);
    for (int r0 = r_first; r0 < r_end; r0 += VF_ROWS) {
        const int rows = min(VF_ROWS, h - r0), steps = w + 2 * (rows - 1);
        float left = 0.f, top = lane == 0 ? er[0] : 0.f, topleft = 0.f;
        for (int t0 = 0; t0 < steps; t0 += VF_T) {
            if constexpr (SW) {
#pragma unroll
                for (int it = 0; it < VF_ITER(2 * VF_ROWS * VF_VC); ++it) {
                    const int idx = tid + it * VF_THREADS;
                    if (idx >= 2 * VF_ROWS * VF_VC) break;
                    const int p = idx / (VF_ROWS * VF_VC), rem = idx - p * (VF_ROWS * VF_VC);
                    const int l = rem / VF_VC, jj = rem - l * VF_VC;
                    const int row = r0 + l, pc = (t0 >> 1) - l - 1 + jj;
                    float acc = 0.f;
                    if (row < h && pc >= -2 && pc <= cw + 1) {                   // the taps of chroma columns 0 .. cw - 1 reach no further
                        const int mx = tw_mirror(pc, cw);
                        if constexpr (SH) {
                            const int par = row & 1, base = (row >> 1) + (par ? TW_UP_FIRST_V_ODD : TW_UP_FIRST_V_EVEN);
                            acc = a.wt.up_v[par][0] * cunit[vf_code8(cf[p][(int64_t)tw_mirror(base, ch) * cw + mx], true, a)];
#pragma unroll
                            for (int k = 1; k < TW_UP_TAPS; ++k)
                                acc = acc + a.wt.up_v[par][k] * cunit[vf_code8(cf[p][(int64_t)tw_mirror(base + k, ch) * cw + mx], true, a)];
                        } else {
                            acc = cunit[vf_code8(cf[p][(int64_t)row * cw + mx], true, a)];
                        }
                    }
                    vb[p][l][jj] = acc;
                }
            }
            // the Y samples of the chunk (4:4:4: U and V too), asked for before the barrier
            int yv[VF_ITER(VF_ROWS * VF_T)], uv[SW ? 1 : VF_ITER(VF_ROWS * VF_T)][2];
#pragma unroll
            for (int it = 0; it < VF_ITER(VF_ROWS * VF_T); ++it) {
                const int idx = tid + it * VF_THREADS, l = idx >> 6, j = idx & 63;
                const int row = r0 + l, col = t0 - 2 * l + j;
                const bool in = row < h && col >= 0 && col < w;
                yv[it] = in ? vf_code8(yf[(int64_t)row * w + col], false, a) : -1;
                if constexpr (!SW) {
                    uv[it][0] = in ? vf_code8(cf[0][(int64_t)row * w + col], true, a) : 128;
                    uv[it][1] = in ? vf_code8(cf[1][(int64_t)row * w + col], true, a) : 128;
                }
            }
            __syncthreads();
            // the horizontal pass and the matrix
#pragma unroll
            for (int it = 0; it < VF_ITER(VF_ROWS * VF_T); ++it) {
                const int idx = tid + it * VF_THREADS, l = idx >> 6, j = idx & 63;
                float r = 0.f, g = 0.f, b = 0.f;
                if (yv[it] >= 0) {
                    float cbr[2];
                    if constexpr (SW) {
                        const int par = j & 1, jb = (j >> 1) + 1 + TW_UP_FIRST_H;    // t0 - 2 l is even: the column's parity is j's
#pragma unroll
                        for (int p = 0; p < 2; ++p) {
                            cbr[p] = a.wt.up_h[par][0] * vb[p][l][jb];
#pragma unroll
                            for (int k = 1; k < TW_UP_TAPS; ++k) cbr[p] = cbr[p] + a.wt.up_h[par][k] * vb[p][l][jb + k];
                        }
                    } else {
                        cbr[0] = cunit[uv[it][0]]; cbr[1] = cunit[uv[it][1]];
                    }
                    vf_ycc2rgb(unit[yv[it]], cbr[0], cbr[1], a, r, g, b);
                }
                xs[0][l][j] = r; xs[1][l][j] = g; xs[2][l][j] = b;
            }
            __syncthreads();
            if (a.dither) {
                if (walker)
                    vf_walk_chunk(xs[c][lane], er, t0, w, rows, lane, 255.f, left, top, topleft, [&](int j, int q) { ob[lane][j * 3 + c] = (uint8_t)q; });
            } else {
                for (int idx = tid; idx < VF_ROWS * VF_T * 3; idx += VF_THREADS) {
                    const int l = idx / (VF_T * 3), b = idx - l * (VF_T * 3);
                    ob[l][b] = (uint8_t)tw_quant(xs[b % 3][l][b / 3]);
                }
            }
            __syncthreads();
            // flush: row l of the tile is 192 consecutive bytes of the frame
            for (int idx = tid; idx < rows * VF_T * 3; idx += VF_THREADS) {
                const int l = idx / (VF_T * 3), b = idx - l * (VF_T * 3);
                const int col = t0 - 2 * l + b / 3;
                if (col >= 0 && col < w) df[((int64_t)(r0 + l) * w + t0 - 2 * l) * 3 + b] = ob[l][b];
            }
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(256) vf_gray_kernel(const T* __restrict__ yp, uint8_t* __restrict__ dst, int64_t npix, VfArgs a) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
        const float y = ((float)vf_code8(yp[i], false, a) - a.y_off) / a.y_scale;
        const uint8_t q = (uint8_t)tw_quant(y * 255.f);
        dst[i * 3] = q; dst[i * 3 + 1] = q; dst[i * 3 + 2] = q;
    }
}

static bool vf_size_ok(const VfArgs& a) {
    return a.n > 0 && a.h >= 1 && a.w >= 1 && a.h <= TW_MAX_SIDE && a.w <= TW_MAX_SIDE && a.bits >= 8 && a.bits <= 16 && !(a.sub_w && (a.w & 1)) &&
           !(a.sub_h && (a.h & 1)) && !(a.sub_h && !a.sub_w) && (a.sub_w | a.sub_h) <= 1 && a.sub_w >= 0 && a.sub_h >= 0;
}

template <typename T>
static void vf_launch_back(const void* y, const void* u, const void* v, uint8_t* dst, const VfArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)a.n, a.dither ? 1u : (unsigned)((a.h + VF_ROWS - 1) / VF_ROWS));
    const T *yy = (const T*)y, *uu = (const T*)u, *vv = (const T*)v;
    if (a.gray) {
        const int64_t npix = (int64_t)a.n * a.h * a.w;
        const int64_t blocks = (npix + 255) / 256;
        hipLaunchKernelGGL(vf_gray_kernel<T>, dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), dim3(256), 0, s, yy, dst, npix, a);
    } else if (a.sub_h) {
        hipLaunchKernelGGL((vf_back_kernel<T, 1, 1>), grid, dim3(VF_THREADS), 0, s, yy, uu, vv, dst, a);
    } else if (a.sub_w) {
        hipLaunchKernelGGL((vf_back_kernel<T, 1, 0>), grid, dim3(VF_THREADS), 0, s, yy, uu, vv, dst, a);
    } else {
        hipLaunchKernelGGL((vf_back_kernel<T, 0, 0>), grid, dim3(VF_THREADS), 0, s, yy, uu, vv, dst, a);
    }
}

int launch_vformat_to_rgb(const void* y, const void* u, const void* v, uint8_t* dst, VfArgs a, hipStream_t s) {
    if (!vf_size_ok(a) || (a.gray && (a.sub_w || a.sub_h || a.dither)) || a.n > 65535) return (int)hipErrorInvalidValue;
    a.full_range = a.gray ? 0 : a.full_range;      // GRAY -> RGB24 is limited -> full
    vf_constants(a);
    if (a.bits == 8) vf_launch_back<uint8_t>(y, u, v, dst, a, s);
    else vf_launch_back<uint16_t>(y, u, v, dst, a, s);
    return (int)hipGetLastError();
}

// ---- RGB24 -> planes ------------------------------------------------------------------------------------------------------------------------------------------
// plane 0: Y of pixel (row, col); planes 1, 2: Cb, Cr, normalised (before the scaling into codes)
template <int PLANE>
__device__ __forceinline__ float vf_pixel(const uint8_t* __restrict__ frame, int row, int col, int w, const float* unit, const VfArgs& a) {
    const uint8_t* p = frame + ((int64_t)row * w + col) * 3;
    float y, cb, cr;
    vf_rgb2ycc(unit[p[0]], unit[p[1]], unit[p[2]], a, y, cb, cr);
    return PLANE == 0 ? y : (PLANE == 1 ? cb : cr);
}

// the chunk's samples of plane PLANE into xs: xs[l][j] = the code before rounding at plane row r0 + l, plane column t0 - 2 l + j (0 outside the plane)
template <int PLANE, int SW, int SH>
__device__ __forceinline__ void vf_stage_fwd(const uint8_t* __restrict__ frame, float (*xs)[VF_XP], float (*vbuf)[VF_DP], const float* unit, int r0, int t0, int ph,
                                             int pw, const VfArgs& a) {
    const int tid = threadIdx.x, h = a.h, w = a.w;
    if constexpr (PLANE != 0 && SW) {
        // vbuf[l][jj] = the plane's sample at row r0 + l after the vertical pass (SH) at pixel column 2 (t0 - 2 l) + TW_DOWN_FIRST + jj, mirrored
        for (int idx = tid; idx < VF_ROWS * VF_DC; idx += VF_THREADS) {
            const int l = idx / VF_DC, jj = idx - l * VF_DC;
            const int row = r0 + l, px = 2 * (t0 - 2 * l) + TW_DOWN_FIRST + jj;
            float acc = 0.f;
            if (row < ph && px >= TW_DOWN_FIRST && px < w + TW_DOWN_TAPS) {       // the taps of columns 0 .. pw - 1 reach no further
                const int mx = tw_mirror(px, w);
                if constexpr (SH) {
                    const int base = 2 * row + TW_DOWN_FIRST;
                    acc = a.wt.down_v[0] * vf_pixel<PLANE>(frame, tw_mirror(base, h), mx, w, unit, a);
#pragma unroll
                    for (int k = 1; k < TW_DOWN_TAPS; ++k) acc = acc + a.wt.down_v[k] * vf_pixel<PLANE>(frame, tw_mirror(base + k, h), mx, w, unit, a);
                } else {
                    acc = vf_pixel<PLANE>(frame, row, mx, w, unit, a);
                }
            }
            vbuf[l][jj] = acc;
        }
        __syncthreads();
    }
#pragma unroll
    for (int it = 0; it < VF_ITER(VF_ROWS * VF_T); ++it) {
        const int idx = tid + it * VF_THREADS, l = idx >> 6, j = idx & 63;
        const int row = r0 + l, col = t0 - 2 * l + j;
        float x = 0.f;
        if (row < ph && col >= 0 && col < pw) {
            if constexpr (PLANE == 0) {
                x = vf_scale(vf_pixel<0>(frame, row, col, w, unit, a), a.ys, a.yo);
            } else if constexpr (SW) {
                float acc = a.wt.down_h[0] * vbuf[l][2 * j];
#pragma unroll
                for (int k = 1; k < TW_DOWN_TAPS; ++k) acc = acc + a.wt.down_h[k] * vbuf[l][2 * j + k];
                x = vf_scale(acc, a.cs, a.co);
            } else {
                x = vf_scale(vf_pixel<PLANE>(frame, row, col, w, unit, a), a.cs, a.co);
            }
        }
        xs[l][j] = x;
    }
}

template <typename T, int SW, int SH>
__global__ void __launch_bounds__(VF_THREADS) vf_fwd_kernel(const uint8_t* __restrict__ src, T* __restrict__ yp, T* __restrict__ up, T* __restrict__ vp, VfArgs a) {
    __shared__ float erow[TW_MAX_SIDE];
    __shared__ float xs[VF_ROWS][VF_XP];
    __shared__ float vbuf[VF_ROWS][VF_DP];
    __shared__ uint16_t ob[VF_ROWS][VF_OW];
    __shared__ float unit[256];                    // sample / 255
    const int tid = threadIdx.x, lane = tid & 63, f = blockIdx.x, plane = blockIdx.y;
    const int ph = plane ? a.h >> SH : a.h, pw = plane ? a.w >> SW : a.w;
    const uint8_t* frame = src + (int64_t)f * a.h * a.w * 3;
    T* out = (plane == 0 ? yp : (plane == 1 ? up : vp)) + (int64_t)f * ph * pw;
    if (tid < 256) unit[tid] = (float)tid / 255.f;
    for (int i = tid; i < pw; i += VF_THREADS) erow[i] = 0.f;
    __syncthreads();
    for (int r0 = 0; r0 < ph; r0 += VF_ROWS) {
        const int rows = min(VF_ROWS, ph - r0), steps = pw + 2 * (rows - 1);
        float left = 0.f, top = lane == 0 ? erow[0] : 0.f, topleft = 0.f;
        for (int t0 = 0; t0 < steps; t0 += VF_T) {
            if (plane == 0) vf_stage_fwd<0, SW, SH>(frame, xs, vbuf, unit, r0, t0, ph, pw, a);
            else if (plane == 1) vf_stage_fwd<1, SW, SH>(frame, xs, vbuf, unit, r0, t0, ph, pw, a);
            else vf_stage_fwd<2, SW, SH>(frame, xs, vbuf, unit, r0, t0, ph, pw, a);
            __syncthreads();
            if (tid < 64) vf_walk_chunk(xs[lane], erow, t0, pw, rows, lane, a.hi, left, top, topleft, [&](int j, int q) { ob[lane][j] = (uint16_t)q; });
            __syncthreads();
            // flush: row l of the tile is 64 consecutive samples of the plane
#pragma unroll
            for (int it = 0; it < VF_ITER(VF_ROWS * VF_T); ++it) {
                const int idx = tid + it * VF_THREADS, l = idx >> 6, j = idx & 63;
                const int col = t0 - 2 * l + j;
                if (l < rows && col >= 0 && col < pw) out[(int64_t)(r0 + l) * pw + col] = (T)ob[l][j];
            }
        }
    }
}

// ---- RGB24 -> planes without dither: tweak_forward_kernel's tiles ------------------------------------------------------------------------------------------
#define VFT_TH 16                                  // chroma rows of a tile
#define VFT_TW 32                                  // chroma columns
#define VFT_THREADS 256

// A block owns 16 x 32 chroma samples = (16 << SH) x (32 << SW) pixels: the float Cb / Cr of the tile and of the halo its 8-tap passes need go to LDS, Y is
// scaled, rounded and stored on the way; the vertical pass (SH) writes 16 rows back into LDS, the horizontal pass (SW) reads them, scales, rounds and stores.
template <typename T, int SW, int SH>
__global__ void __launch_bounds__(VFT_THREADS) vf_fwd_tiled_kernel(const uint8_t* __restrict__ src, T* __restrict__ yp, T* __restrict__ up, T* __restrict__ vp,
                                                                   VfArgs a) {
    constexpr int LH = SH ? 2 * VFT_TH + TW_DOWN_TAPS - 2 : VFT_TH, LW = SW ? 2 * VFT_TW + TW_DOWN_TAPS - 2 : VFT_TW, PITCH = LW + 1;
    constexpr int HY = SH ? -TW_DOWN_FIRST : 0, HX = SW ? -TW_DOWN_FIRST : 0;       // halo in front of the tile's own pixels
    __shared__ float cc[2][LH][PITCH];             // Cb, Cr of the tile and its halo
    __shared__ float vv[2][SH ? VFT_TH : 1][PITCH];    // after the vertical pass
    __shared__ float unit[256];                    // sample / 255
    const int t = threadIdx.x, f = blockIdx.z;
    const int h = a.h, w = a.w, ch = h >> SH, cw = w >> SW;
    const int j0 = blockIdx.y * VFT_TH, i0 = blockIdx.x * VFT_TW;
    unit[t] = (float)t / 255.f;
    __syncthreads();
    const uint8_t* frame = src + (int64_t)f * h * w * 3;
    T* yf = yp + (int64_t)f * h * w;
    for (int idx = t; idx < LH * LW; idx += VFT_THREADS) {
        const int ly = idx / LW, lx = idx - ly * LW;
        const int py = (j0 << SH) - HY + ly, px = (i0 << SW) - HX + lx;
        float cb = 0.f, cr = 0.f;
        if (py < h + TW_DOWN_TAPS && px < w + TW_DOWN_TAPS) {                       // beyond that no sample of the plane has a tap
            const int my = SH ? tw_mirror(py, h) : min(py, h - 1), mx = SW ? tw_mirror(px, w) : min(px, w - 1);
            const uint8_t* p = frame + ((int64_t)my * w + mx) * 3;
            float y;
            vf_rgb2ycc(unit[p[0]], unit[p[1]], unit[p[2]], a, y, cb, cr);
            if (my == py && mx == px && ly >= HY && ly < HY + (VFT_TH << SH) && lx >= HX && lx < HX + (VFT_TW << SW))
                yf[(int64_t)py * w + px] = (T)vf_quant(vf_scale(y, a.ys, a.yo), a.hi);
        }
        cc[0][ly][lx] = cb;
        cc[1][ly][lx] = cr;
    }
    __syncthreads();
    if constexpr (SH) {
        for (int idx = t; idx < VFT_TH * LW; idx += VFT_THREADS) {
            const int j = idx / LW, lx = idx - j * LW;
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                float acc = a.wt.down_v[0] * cc[p][2 * j][lx];
#pragma unroll
                for (int k = 1; k < TW_DOWN_TAPS; ++k) acc = acc + a.wt.down_v[k] * cc[p][2 * j + k][lx];
                vv[p][j][lx] = acc;
            }
        }
        __syncthreads();
    }
    for (int idx = t; idx < VFT_TH * VFT_TW; idx += VFT_THREADS) {
        const int j = idx / VFT_TW, i = idx - j * VFT_TW;
        if (j0 + j >= ch || i0 + i >= cw) continue;
        float acc[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const float* row = SH ? vv[p][j] : cc[p][j];
            if constexpr (SW) {
                acc[p] = a.wt.down_h[0] * row[2 * i];
#pragma unroll
                for (int k = 1; k < TW_DOWN_TAPS; ++k) acc[p] = acc[p] + a.wt.down_h[k] * row[2 * i + k];
            } else {
                acc[p] = row[i];
            }
        }
        const int64_t o = ((int64_t)f * ch + j0 + j) * cw + i0 + i;
        up[o] = (T)vf_quant(vf_scale(acc[0], a.cs, a.co), a.hi);
        vp[o] = (T)vf_quant(vf_scale(acc[1], a.cs, a.co), a.hi);
    }
}

template <typename T>
static void vf_launch_fwd(const uint8_t* src, void* y, void* u, void* v, const VfArgs& a, hipStream_t s) {
    T *yy = (T*)y, *uu = (T*)u, *vv = (T*)v;
    if (!a.dither) {
        const dim3 grid((unsigned)(((a.w >> a.sub_w) + VFT_TW - 1) / VFT_TW), (unsigned)(((a.h >> a.sub_h) + VFT_TH - 1) / VFT_TH), (unsigned)a.n);
        if (a.sub_h) hipLaunchKernelGGL((vf_fwd_tiled_kernel<T, 1, 1>), grid, dim3(VFT_THREADS), 0, s, src, yy, uu, vv, a);
        else if (a.sub_w) hipLaunchKernelGGL((vf_fwd_tiled_kernel<T, 1, 0>), grid, dim3(VFT_THREADS), 0, s, src, yy, uu, vv, a);
        else hipLaunchKernelGGL((vf_fwd_tiled_kernel<T, 0, 0>), grid, dim3(VFT_THREADS), 0, s, src, yy, uu, vv, a);
        return;
    }
    const dim3 grid((unsigned)a.n, 3u);
    if (a.sub_h) hipLaunchKernelGGL((vf_fwd_kernel<T, 1, 1>), grid, dim3(VF_THREADS), 0, s, src, yy, uu, vv, a);
    else if (a.sub_w) hipLaunchKernelGGL((vf_fwd_kernel<T, 1, 0>), grid, dim3(VF_THREADS), 0, s, src, yy, uu, vv, a);
    else hipLaunchKernelGGL((vf_fwd_kernel<T, 0, 0>), grid, dim3(VF_THREADS), 0, s, src, yy, uu, vv, a);
}

int launch_vformat_from_rgb(const uint8_t* src, void* y, void* u, void* v, VfArgs a, hipStream_t s) {
    if (!vf_size_ok(a) || a.gray || a.n > 65535) return (int)hipErrorInvalidValue;
    a.depth_full_range = 0;
    vf_constants(a);
    if (a.bits == 8) vf_launch_fwd<uint8_t>(src, y, u, v, a, s);
    else vf_launch_fwd<uint16_t>(src, y, u, v, a, s);
    return (int)hipGetLastError();
}
