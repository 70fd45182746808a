// Edge-masked scene statistics of a whole clip (vsslib/vsscdetect_edge.py:168-182): what the reference's second detector reads of a frame is four integers.
//     Y          = (cr * R + cg * G + cb * B + bias) >> 16                   the gray plane, as in scdetect.hip
//     kirsch     = max over the four std.Convolution passes of min(|8 S3 - 3 S8|, 255)       (3 x 3, scedge_ops.h)
//     tcanny     = TCanny(mode = 1, sigma) of E = table[Y]: separable Gaussian of radius r (vertical pass, then horizontal, float32, every product and
//                  sum rounded), Prewitt gradient * 0.5, magnitude, int(gm + 0.5) clamped to 255
//     mask       = min(kirsch + tcanny, 255)
//     sum_y, sad_prev = sum |Y_n - Y_max(n - 1, 0)|, sad_next = sum |Y_n - Y_j|, sum_masked = sum (|Y_n - Y_j| * mask + 127) / 255
// with j = n + offset for n < N - offset and N - offset otherwise.  tests/scedges_util.py is the definition, value for value.
//
// One launch: blocks_per_frame blocks per frame, each walking the frame's 32 x 64 tiles with a stride of blocks_per_frame.  A tile stages the gray plane of
// the positions [y0 - r - 1, y0 + 32 + r + 1) x [x0 - r - 1, x0 + 64 + r + 1) in LDS -- recomputed from the RGB bytes, no gray plane lives in HBM -- and
// everything else runs out of LDS: the vertical pass leaves 34 rows, the horizontal pass 34 x 66 blurred values, and a thread finishes four pixels from
// those and the 3 x 3 gray neighbourhood.  The two compared frames are read at the pixel itself only.
//
// Borders.  LDS positions are UNBOUNDED image positions u; what a plane holds at u is the definition's value at reflect(u) (reflect-101 of the IMAGE, however
// small it is and wherever the tile lies).  For the integer stencils that is all there is to it.  A float32 sum depends on the order of its terms, and the
// definition adds tap -r first around the IMAGE coordinate: around a position behind an odd number of folds that is the opposite direction in u, so both
// blur passes step through LDS with the position's direction (edge_fold).  The weights are symmetric, so the products are the same and only their order
// changes.  Nothing outside the clip is read: every global address comes from a reflected coordinate or from a pixel of the frame.
//
// Reduction: registers -> wave (shuffles) -> block (LDS) -> one 64-bit atomic add per block and quantity on the frame's record.  Integers throughout: the
// records are bit-identical from run to run.
#include "kernels.h"
#include "scdetect_ops.h"
#include "scedge_ops.h"

constexpr int ET_H = 32, ET_W = 64;                                        // output tile
constexpr int ET_HALO = EDGE_MAX_RADIUS + 1;
constexpr int ET_EH = ET_H + 2 * ET_HALO, ET_EW = ET_W + 2 * ET_HALO;       // staged gray positions at the largest radius
constexpr int ET_VH = ET_H + 2, ET_BW = ET_W + 2;                           // rows after the vertical pass, columns after the horizontal pass

__device__ __forceinline__ unsigned edge_wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

__global__ void __launch_bounds__(256) scene_edge_kernel(const uint8_t* __restrict__ clip, EdgeRec* rec, uint8_t* __restrict__ tap, EdgeStatsArgs a) {
    __shared__ uint8_t s_y[ET_EH * ET_EW];
    __shared__ float s_v[ET_VH * ET_EW];
    __shared__ float s_b[ET_VH * ET_BW];
    __shared__ float s_lut[256];
    __shared__ float s_w[EDGE_MAX_TAPS];
    __shared__ int s_gx[ET_EW], s_gy[ET_EH];
    __shared__ signed char s_dx[ET_EW], s_dy[ET_EH];
    __shared__ unsigned red[4][4];

    const int t = threadIdx.x;
    const int f = (int)(blockIdx.x / (unsigned)a.blocks_per_frame), chunk = (int)(blockIdx.x % (unsigned)a.blocks_per_frame);
    const int r = a.radius, halo = r + 1;
    const int eh = ET_H + 2 * halo, ew = ET_W + 2 * halo;                   // positions staged at this radius; rows of ew values in s_y and s_v
    const int p = f > 0 ? f - 1 : 0;
    const int j = f < a.n - a.offset ? f + a.offset : a.n - a.offset;
    const int64_t npix = (int64_t)a.h * a.w;
    const uint8_t* cur = clip + (int64_t)f * npix * 3;
    const uint8_t* prv = clip + (int64_t)p * npix * 3;
    const uint8_t* nxt = clip + (int64_t)j * npix * 3;
    const SceneLuma c{a.cr, a.cg, a.cb, a.bias};

    s_lut[t] = (float)a.enh[t];                                             // blockDim.x == 256
    if (t <= 2 * r) s_w[t] = a.wt[t];

    unsigned acc_y = 0, acc_prev = 0, acc_next = 0, acc_masked = 0;
    const int n_tiles = a.tiles_x * a.tiles_y;
    for (int tile = chunk; tile < n_tiles; tile += a.blocks_per_frame) {
        const int y0 = (tile / a.tiles_x) * ET_H, x0 = (tile % a.tiles_x) * ET_W;
        __syncthreads();                                                    // the previous tile is finished with every plane
        for (int i = t; i < ew + eh; i += 256) {
            int d;
            if (i < ew) { s_gx[i] = edge_fold(x0 - halo + i, a.w, &d); s_dx[i] = (signed char)d; }
            else { s_gy[i - ew] = edge_fold(y0 - halo + (i - ew), a.h, &d); s_dy[i - ew] = (signed char)d; }
        }
        __syncthreads();
        for (int i = t; i < eh * ew; i += 256) {
            const int ly = i / ew, lx = i - ly * ew;
            const uint8_t* px = cur + ((int64_t)s_gy[ly] * a.w + s_gx[lx]) * 3;
            s_y[i] = (uint8_t)scene_gray(c, px[0], px[1], px[2]);
        }
        __syncthreads();
        // vertical pass: row vy is position y0 - 1 + vy = staged row vy + r
        for (int i = t; i < ET_VH * ew; i += 256) {
            const int vy = i / ew, lx = i - vy * ew;
            const int ly = vy + r, d = s_dy[ly];
            float s = __fmul_rn(s_w[0], s_lut[s_y[(ly - d * r) * ew + lx]]);
            for (int k = 1 - r; k <= r; ++k) s = __fadd_rn(s, __fmul_rn(s_w[k + r], s_lut[s_y[(ly + d * k) * ew + lx]]));
            s_v[i] = s;
        }
        __syncthreads();
        // horizontal pass: column bx is position x0 - 1 + bx = staged column bx + r
        for (int i = t; i < ET_VH * ET_BW; i += 256) {
            const int vy = i / ET_BW, bx = i - vy * ET_BW;
            const int lx = bx + r, d = s_dx[lx];
            const float* row = s_v + vy * ew;
            float s = __fmul_rn(s_w[0], row[lx - d * r]);
            for (int k = 1 - r; k <= r; ++k) s = __fadd_rn(s, __fmul_rn(s_w[k + r], row[lx + d * k]));
            s_b[i] = s;
        }
        __syncthreads();
        for (int i = t; i < ET_H * ET_W; i += 256) {
            const int ty = i / ET_W, tx = i - ty * ET_W;
            const int y = y0 + ty, x = x0 + tx;
            if (y >= a.h || x >= a.w) continue;
            const float* b0 = s_b + ty * ET_BW + tx;                        // the blurred plane at (y - 1, x - 1)
            const float* b1 = b0 + ET_BW;
            const float* b2 = b1 + ET_BW;
            const float gx = __fmul_rn(__fsub_rn(__fadd_rn(__fadd_rn(b0[2], b1[2]), b2[2]), __fadd_rn(__fadd_rn(b0[0], b1[0]), b2[0])), 0.5f);
            const float gy = __fmul_rn(__fsub_rn(__fadd_rn(__fadd_rn(b0[0], b0[1]), b0[2]), __fadd_rn(__fadd_rn(b2[0], b2[1]), b2[2])), 0.5f);
            const float gm = __fsqrt_rn(__fadd_rn(__fmul_rn(gx, gx), __fmul_rn(gy, gy)));
            const float gr = __fadd_rn(gm, 0.5f);
            const int tc = gr >= 255.f ? 255 : (int)gr;
            const uint8_t* g0 = s_y + (ty + halo - 1) * ew + (tx + halo - 1);   // the gray plane at (y - 1, x - 1)
            const uint8_t* g1 = g0 + ew;
            const uint8_t* g2 = g1 + ew;
            const int tl = g0[0], tp = g0[1], tr = g0[2], lf = g1[0], yc = g1[1], rt = g1[2], bl = g2[0], bt = g2[1], br = g2[2];
            const int s8 = tl + tp + tr + lf + rt + bl + bt + br;
            int kir = edge_kirsch_pass(tl + tp + tr, s8);
            kir = max(kir, edge_kirsch_pass(tp + tr + lf, s8));
            kir = max(kir, edge_kirsch_pass(tr + lf + rt, s8));
            kir = max(kir, edge_kirsch_pass(lf + rt + bl, s8));
            const int mask = min(kir + tc, 255);
            const int64_t o = ((int64_t)y * a.w + x) * 3;
            acc_y += (unsigned)yc;
            if (p != f) {
                const int q = scene_gray(c, prv[o], prv[o + 1], prv[o + 2]);
                acc_prev += (unsigned)(yc > q ? yc - q : q - yc);
            }
            if (j != f) {
                const int q = scene_gray(c, nxt[o], nxt[o + 1], nxt[o + 2]);
                const int d = yc > q ? yc - q : q - yc;
                acc_next += (unsigned)d;
                acc_masked += (unsigned)edge_masked(d, mask);
            }
            if (tap) tap[(int64_t)f * npix + (int64_t)y * a.w + x] = (uint8_t)mask;
        }
    }
    // a thread adds at most 255 for each of its 8 pixels of a tile and walks at most 1024 tiles (launch_scene_edge_stats): a WAVE's 32-bit sum stays
    // below 1.4e8.  The four wave sums are added in 64 bits.
    acc_y = edge_wave_sum(acc_y);
    acc_prev = edge_wave_sum(acc_prev);
    acc_next = edge_wave_sum(acc_next);
    acc_masked = edge_wave_sum(acc_masked);
    const int wave = t >> 6;
    if ((t & 63) == 0) { red[wave][0] = acc_y; red[wave][1] = acc_prev; red[wave][2] = acc_next; red[wave][3] = acc_masked; }
    __syncthreads();
    if (t < 4) {
        unsigned long long s = 0;
        for (int k = 0; k < 4; ++k) s += red[k][t];
        EdgeRec* rr = rec + f;
        long long* q = t == 0 ? &rr->sum_y : (t == 1 ? &rr->sad_prev : (t == 2 ? &rr->sad_next : &rr->sum_masked));
        atomicAdd(reinterpret_cast<unsigned long long*>(q), s);
    }
}

// at most 128 blocks add to a frame's 32-byte record (scdetect.hip measured what more of them cost); the tiles are dealt evenly
int scene_edge_blocks_per_frame(int n_tiles) {
    const int rounds = (n_tiles + 127) / 128;
    return (n_tiles + rounds - 1) / rounds;
}

// rec: n records in device memory, ZERO-FILLED by the caller in front of the launch (on the same stream); tap: n * h * w bytes or null
int launch_scene_edge_stats(const uint8_t* clip, EdgeRec* rec, uint8_t* tap, EdgeStatsArgs a, hipStream_t s) {
    if (a.n <= 0 || a.h <= 0 || a.w <= 0 || a.h > EDGE_MAX_SIDE || a.w > EDGE_MAX_SIDE || a.offset < 1 || a.offset >= a.n || a.radius < 1 ||
        a.radius > EDGE_MAX_RADIUS)
        return (int)hipErrorInvalidValue;
    a.tiles_x = (a.w + ET_W - 1) / ET_W;
    a.tiles_y = (a.h + ET_H - 1) / ET_H;
    a.blocks_per_frame = scene_edge_blocks_per_frame(a.tiles_x * a.tiles_y);
    const int64_t blocks = (int64_t)a.n * a.blocks_per_frame;
    if (blocks > 0x7FFFFFFFll) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(scene_edge_kernel, dim3((unsigned)blocks), dim3(256), 0, s, clip, rec, tap, a);
    return (int)hipGetLastError();
}

void preload_scedge() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(scene_edge_kernel)); (void)hipGetLastError(); }
