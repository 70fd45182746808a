// HBM-bound u8 per-pixel filters of the HAVC post path (vsslib/imfilters.py), interleaved RGB in HBM.
// Integer arithmetic follows OpenCV's 8-bit BT.601 "YUV" fixed point (yuv_shift = 14) and Pillow's
// ImagingBlend exactly (bit-exact targets; see oracle/cvcolor.py, oracle/imaging.py).
#include "kernels.h"
#include "pixel_ops.h"

static inline int grid_for(int64_t work) {
    int64_t b = (work + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

// ---- PIL Image.blend(a, b, w): (UINT8)((int)a + w * ((int)b - (int)a)) in float32 with the product
// ROUNDED before the add (Pillow's x86-64 build has no FMA).  HIP's __fmul_rn/__fadd_rn are plain operators
// and hipcc contracts a + w*d into v_fma_f32 by default, so contraction is switched off explicitly here
// (and the whole file is built with -ffp-contract=off). ----
__device__ __forceinline__ uint8_t blend1(uint8_t a, uint8_t b, float w) {
#pragma clang fp contract(off)
    const float prod = w * (float)((int)b - (int)a);
    const float sum = (float)(int)a + prod;
    return (uint8_t)(int)sum;
}

__global__ void blend_u8_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, float w,
                                uint8_t* __restrict__ out, int64_t n) {
    // 4 bytes per thread when aligned
    const int64_t n4 = n >> 2;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const uchar4 va = reinterpret_cast<const uchar4*>(a)[i], vb = reinterpret_cast<const uchar4*>(b)[i];
        uchar4 o;
        o.x = blend1(va.x, vb.x, w); o.y = blend1(va.y, vb.y, w);
        o.z = blend1(va.z, vb.z, w); o.w = blend1(va.w, vb.w, w);
        reinterpret_cast<uchar4*>(out)[i] = o;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const int64_t i = (n4 << 2) + threadIdx.x;
        out[i] = blend1(a[i], b[i], w);
    }
}

int launch_blend_u8(const uint8_t* a, const uint8_t* b, float w, uint8_t* out, int64_t nbytes, hipStream_t s) {
    hipLaunchKernelGGL(blend_u8_kernel, dim3(grid_for(nbytes / 4 + 1)), dim3(256), 0, s, a, b, w, out, nbytes);
    return (int)hipGetLastError();
}

// ---- frame_to_image / image_to_frame (vsslib/vsutils.py:60-110): three u8 planes [3][npix] <-> interleaved RGB ----
__global__ void planar_to_rgb8_kernel(const uint8_t* __restrict__ planes, uint8_t* __restrict__ rgb, int64_t npix) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
        rgb[i * 3] = planes[i]; rgb[i * 3 + 1] = planes[npix + i]; rgb[i * 3 + 2] = planes[2 * npix + i];
    }
}
__global__ void rgb8_to_planar_kernel(const uint8_t* __restrict__ rgb, uint8_t* __restrict__ planes, int64_t npix) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
        planes[i] = rgb[i * 3]; planes[npix + i] = rgb[i * 3 + 1]; planes[2 * npix + i] = rgb[i * 3 + 2];
    }
}
int launch_planar_to_rgb8(const uint8_t* planes, uint8_t* rgb, int64_t npix, hipStream_t s) {
    hipLaunchKernelGGL(planar_to_rgb8_kernel, dim3(grid_for(npix)), dim3(256), 0, s, planes, rgb, npix);
    return (int)hipGetLastError();
}
int launch_rgb8_to_planar(const uint8_t* rgb, uint8_t* planes, int64_t npix, hipStream_t s) {
    hipLaunchKernelGGL(rgb8_to_planar_kernel, dim3(grid_for(npix)), dim3(256), 0, s, rgb, planes, npix);
    return (int)hipGetLastError();
}

// ---- chroma_post_process / ColorizerFilter._post_process: Y from orig, U,V from colour ----
__global__ void yuv_merge_kernel(const uint8_t* __restrict__ color, const uint8_t* __restrict__ orig,
                                 uint8_t* __restrict__ out, int64_t npix) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
        int r, g, b;
        yuv_merge_pixel(color[i * 3], color[i * 3 + 1], color[i * 3 + 2], orig[i * 3], orig[i * 3 + 1], orig[i * 3 + 2], r, g, b);
        out[i * 3] = (uint8_t)r; out[i * 3 + 1] = (uint8_t)g; out[i * 3 + 2] = (uint8_t)b;
    }
}

int launch_yuv_merge(const uint8_t* color, const uint8_t* orig, uint8_t* out, int64_t npix, hipStream_t s) {
    hipLaunchKernelGGL(yuv_merge_kernel, dim3(grid_for(npix)), dim3(256), 0, s, color, orig, out, npix);
    return (int)hipGetLastError();
}

// ---- chroma_stabilizer (imfilters.py:160-200): clip U,V of img_new into [u8(U1(1-a)), u8(U1(1+a))] of
// img_stable (float64 products, truncating casts, as numpy does), Y from img_stable, optional blend ----
__global__ void chroma_stabilizer_kernel(const uint8_t* __restrict__ st, const uint8_t* __restrict__ nw, double alpha,
                                         float weight, int do_blend, uint8_t* __restrict__ out, int64_t npix) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
        int y1, u1, v1, y2, u2, v2, r, g, b;
        const int sr = st[i * 3], sg = st[i * 3 + 1], sb = st[i * 3 + 2];
        rgb2yuv(sr, sg, sb, y1, u1, v1);
        rgb2yuv(nw[i * 3], nw[i * 3 + 1], nw[i * 3 + 2], y2, u2, v2);
        const int u_up = (int)fmin(fmax((double)u1 * (1.0 + alpha), 0.0), 255.0);
        const int v_up = (int)fmin(fmax((double)v1 * (1.0 + alpha), 0.0), 255.0);
        const int u_dn = (int)fmin(fmax((double)u1 * (1.0 - alpha), 0.0), 255.0);
        const int v_dn = (int)fmin(fmax((double)v1 * (1.0 - alpha), 0.0), 255.0);
        u2 = u2 > u_up ? u_up : u2;  u2 = u2 < u_dn ? u_dn : u2;   // array_clip: cap to max, then floor to min
        v2 = v2 > v_up ? v_up : v2;  v2 = v2 < v_dn ? v_dn : v2;
        yuv2rgb(y1, u2, v2, r, g, b);
        if (do_blend) {
            r = blend1((uint8_t)sr, (uint8_t)r, weight);
            g = blend1((uint8_t)sg, (uint8_t)g, weight);
            b = blend1((uint8_t)sb, (uint8_t)b, weight);
        }
        out[i * 3] = (uint8_t)r; out[i * 3 + 1] = (uint8_t)g; out[i * 3 + 2] = (uint8_t)b;
    }
}

int launch_chroma_stabilizer(const uint8_t* stable, const uint8_t* inew, double alpha, float weight, uint8_t* out,
                             int64_t npix, hipStream_t s) {
    hipLaunchKernelGGL(chroma_stabilizer_kernel, dim3(grid_for(npix)), dim3(256), 0, s, stable, inew, alpha, weight,
                       weight < 1.0f ? 1 : 0, out, npix);
    return (int)hipGetLastError();
}

// ---- separable polyphase resample (Spline64 taps computed on the host; harness stand-in for zimg) ----
// Arithmetic contract (oracle/resample.py is the CPU twin): horizontal pass first, fp32, taps accumulated in ascending order,
// product rounded before the add (no FMA: this file is built with -ffp-contract=off); vertical pass the same; round half up.
// pass 1 (horizontal): u8 [rows][sw][3] -> float [rows][dw][3].  One block per source row: the row is staged in LDS with
// aligned dword loads (a 1920-pixel row is read 29 times by the 560 outputs of the squash), then every thread produces
// outputs x = tid, tid + 256, ...
__global__ void __launch_bounds__(256) resize_h_kernel(const uint8_t* __restrict__ src, float* __restrict__ tmp, const int* __restrict__ start,
                                                       const float* __restrict__ wts, int taps, int sw, int dw, int64_t rows) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rowbuf[];
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const uint8_t* sp = src + row * sw * 3;
        const int a0 = (int)(reinterpret_cast<uintptr_t>(sp) & 3);
        const uint32_t* wp = reinterpret_cast<const uint32_t*>(sp - a0);
        const int nwords = (a0 + sw * 3 + 3) >> 2;            // an over-read stays inside the last aligned dword of the row
        __syncthreads();
        for (int i = threadIdx.x; i < nwords; i += 256) reinterpret_cast<uint32_t*>(rowbuf)[i] = wp[i];
        __syncthreads();
        for (int x = threadIdx.x; x < dw; x += 256) {
            const int s0 = start[x];
            const float* w = wts + (int64_t)x * taps;
            float r = 0.f, g = 0.f, b = 0.f;
            for (int t = 0; t < taps; ++t) {
                int sx = s0 + t;
                sx = sx < 0 ? 0 : (sx >= sw ? sw - 1 : sx);
                const float wt = w[t];
                // the pixel's three bytes through one aligned two-dword LDS read + v_alignbyte (byte / unaligned halfword LDS reads cost ~30 clocks each)
                const unsigned addr = (unsigned)(a0 + sx * 3);
                const uint32_t* pw = reinterpret_cast<const uint32_t*>(rowbuf + (addr & ~3u));
                const uint32_t px = __builtin_amdgcn_alignbyte(pw[1], pw[0], addr & 3u);
                r += wt * (float)(px & 255u); g += wt * (float)((px >> 8) & 255u); b += wt * (float)((px >> 16) & 255u);
            }
            float* o = tmp + (row * dw + x) * 3;
            o[0] = r; o[1] = g; o[2] = b;
        }
    }
}

// Round 4: the same pass with the taps in REGISTERS.  resize_h_kernel above fetches w[x * taps + t] inside the tap loop: 64 lanes, 64 different cache
// lines per load instruction, 87 such instructions per output row segment -- the texture-address unit, not the arithmetic, set its 3.0 ms per 64
// squashed 1080p frames.  Here a thread owns ONE output column of a 256-column tile for a chunk of rows: its taps and its (edge-clamped) byte
// offsets are loaded once, the tile's source span of each row is staged in LDS, and the tap loop is LDS byte reads + the same mul / add sequence
// (ascending taps, product rounded before the add): bit-identical to resize_h_kernel.  TMAX bounds the unrolled tap loop (taps <= TMAX).
template <int TMAX>
__global__ void __launch_bounds__(256) resize_h_rows_kernel(const uint8_t* __restrict__ src, float* __restrict__ tmp, const int* __restrict__ start,
                                                            const float* __restrict__ wts, int taps, int sw, int dw, int64_t rows, int rows_per_block, int out_off, int vec_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rowbuf[];
    const int x0 = blockIdx.x * 256, x = x0 + threadIdx.x;
    const bool active = x < dw;
    const int xl = min(x0 + 255, dw - 1);
    int lo = start[x0], hi = start[xl] + taps - 1;             // the tile's source span (start[] ascends with x)
    lo = lo < 0 ? 0 : (lo >= sw ? sw - 1 : lo);
    hi = hi < 0 ? 0 : (hi >= sw ? sw - 1 : hi);
    const int span_bytes = (hi - lo + 1) * 3;
    float w[TMAX];
    int off[TMAX];
    {
        const int s0 = active ? start[x] : 0;
#pragma unroll
        for (int t = 0; t < TMAX; ++t) {
            w[t] = (active && t < taps) ? wts[(int64_t)x * taps + t] : 0.f;
            int sx = s0 + t;
            sx = sx < 0 ? 0 : (sx >= sw ? sw - 1 : sx);
            sx = sx < lo ? lo : (sx > hi ? hi : sx);               // (inactive lanes / t >= taps: any address inside the span)
            off[t] = (sx - lo) * 3;
        }
    }
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_block, r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
    // The span of row r + 1 is fetched into registers (<= 4 dwords per thread: spans up to 4 KiB) while row r is multiplied: the staging loop of the first
    // version waited for every pair of loads before the LDS write -- two or three exposed memory latencies per row, 17 000 clocks per row on the counters.
    uint32_t pre[4];
    int a0 = 0;
    auto fetch = [&](int64_t row) {
        const uint8_t* sp = src + (row * sw + lo) * 3;
        a0 = (int)(reinterpret_cast<uintptr_t>(sp) & 3);
        const uint32_t* wp = reinterpret_cast<const uint32_t*>(sp - a0);
        const int nwords = (a0 + span_bytes + 3) >> 2;            // an over-read stays inside the last aligned dword of the span's row
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = threadIdx.x + k * 256;
            pre[k] = i < nwords ? wp[i] : 0u;
        }
    };
    fetch(r0);
    for (int64_t row = r0; row < r1; ++row) {
        const int a0_row = a0;
        __syncthreads();                                           // the previous row's taps and its output tile are read
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = threadIdx.x + k * 256;
            if (i * 4 < out_off) reinterpret_cast<uint32_t*>(rowbuf)[i] = pre[k];
        }
        __syncthreads();
        if (row + 1 < r1) fetch(row + 1);
        float r = 0.f, g = 0.f, b = 0.f;
        // every one of the TMAX taps, no test: taps beyond the table's count carry weight 0 (x + 0 * q == x: same bits) -- the LDS reads of a
        // row can then be issued together instead of one latency per tap
        // a pixel = the three bytes at an arbitrary byte address: ONE aligned two-dword read + v_alignbyte instead of byte / halfword reads (the
        // compiler merged q[0], q[1] into ds_read_u16 at odd addresses: ~30 clocks per LDS instruction on the counters, and the pass scaled with them)
#pragma unroll
        for (int t = 0; t < TMAX; ++t) {
            const unsigned addr = (unsigned)(a0_row + off[t]);
            const uint32_t* pw = reinterpret_cast<const uint32_t*>(rowbuf + (addr & ~3u));
            const uint32_t px = __builtin_amdgcn_alignbyte(pw[1], pw[0], addr & 3u);
            const float wt = w[t];
            r += wt * (float)(px & 255u); g += wt * (float)((px >> 8) & 255u); b += wt * (float)((px >> 16) & 255u);
        }
        if (vec_out) {            // dw % 4 == 0: the tile's 3 x 256 floats leave through LDS as 16-byte stores
            float* ob = reinterpret_cast<float*>(rowbuf + out_off);
            ob[threadIdx.x * 3] = r; ob[threadIdx.x * 3 + 1] = g; ob[threadIdx.x * 3 + 2] = b;
            __syncthreads();
            const int nvec = (min(256, dw - x0) * 3) >> 2;
            if ((int)threadIdx.x < nvec)
                reinterpret_cast<float4*>(tmp + (row * dw + x0) * 3)[threadIdx.x] = reinterpret_cast<const float4*>(ob)[threadIdx.x];
        } else if (active) {
            float* o = tmp + (row * dw + x) * 3;
            o[0] = r; o[1] = g; o[2] = b;
        }
    }
}

// pass 2 (vertical): float [n][sh][dw][3] -> u8 [n][dh][dw][3]; if orig != null, fuse chroma_post_process
// (vsfilters.py:863-899 -> imfilters.py:312-321): keep luma of orig, take U,V of the resampled colour.
// A thread produces VR consecutive output rows of one column: their tap windows overlap almost entirely (the window start
// advances by src/dst rows per output), so the column of the intermediate image is read once for the group instead of once
// per output -- the pass was L2-bandwidth bound (9 or 29 row reads per output pixel).  Every output still accumulates its
// own taps in ascending order, edge rows replicated, exactly as one thread per output did.
constexpr int VR = 4;
__global__ void __launch_bounds__(256) resize_v_kernel(const float* __restrict__ tmp, uint8_t* __restrict__ dst, const uint8_t* __restrict__ orig,
                                                       const int* __restrict__ start, const float* __restrict__ wts, int taps, int sh, int dh,
                                                       int dw, int n_frames) {
    const int groups = (dh + VR - 1) / VR;
    const int64_t total = (int64_t)n_frames * groups * dw;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % dw);
        const int gy = (int)((i / dw) % groups);
        const int f = (int)(i / ((int64_t)dw * groups));
        const int y0 = gy * VR;
        int s0[VR];
        float acc[VR][3];
        int lo = 0x7fffffff, hi = -0x7fffffff;
#pragma unroll
        for (int k = 0; k < VR; ++k) {
            const int y = y0 + k < dh ? y0 + k : dh - 1;
            s0[k] = start[y];
            lo = s0[k] < lo ? s0[k] : lo;
            hi = s0[k] + taps - 1 > hi ? s0[k] + taps - 1 : hi;
            acc[k][0] = acc[k][1] = acc[k][2] = 0.f;
        }
        const float* base = tmp + (int64_t)f * sh * dw * 3 + (int64_t)x * 3;
        for (int su = lo; su <= hi; ++su) {
            const int sy = su < 0 ? 0 : (su >= sh ? sh - 1 : su);
            const float* p = base + (int64_t)sy * dw * 3;
            const float pr = p[0], pg = p[1], pb = p[2];
#pragma unroll
            for (int k = 0; k < VR; ++k) {
                const int t = su - s0[k];
                if (t >= 0 && t < taps) {
                    const int y = y0 + k < dh ? y0 + k : dh - 1;
                    const float wt = wts[(int64_t)y * taps + t];
                    acc[k][0] += wt * pr; acc[k][1] += wt * pg; acc[k][2] += wt * pb;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < VR; ++k) {
            const int y = y0 + k;
            if (y >= dh) break;
            int ri = sat8((int)floorf(acc[k][0] + 0.5f)), gi = sat8((int)floorf(acc[k][1] + 0.5f)), bi = sat8((int)floorf(acc[k][2] + 0.5f));
            const int64_t o = ((int64_t)(f * dh + y) * dw + x) * 3;
            if (orig) {
                int yy, u, v, y2, u2, v2;
                rgb2yuv(ri, gi, bi, yy, u, v);
                rgb2yuv(orig[o], orig[o + 1], orig[o + 2], y2, u2, v2);
                yuv2rgb(y2, u, v, ri, gi, bi);
            }
            dst[o] = (uint8_t)ri; dst[o + 1] = (uint8_t)gi; dst[o + 2] = (uint8_t)bi;
        }
    }
}

// Round 4: the vertical pass with FOUR consecutive pixels per thread (dw % 4 == 0, dword-aligned images): a tap row is three 16-byte loads of the
// fp32 intermediate instead of twelve scalar ones, the source-luma pixels and the result are three dwords each instead of twelve byte accesses.
// Per output the same taps in the same order with the same mul / add sequence as resize_v_kernel: bit-identical.
__global__ void __launch_bounds__(256) resize_v4_kernel(const float* __restrict__ tmp, uint8_t* __restrict__ dst, const uint8_t* __restrict__ orig,
                                                        const int* __restrict__ start, const float* __restrict__ wts, int taps, int sh, int dh,
                                                        int dw, int n_frames) {
    const int groups = (dh + VR - 1) / VR, dw4 = dw >> 2;
    const int64_t total = (int64_t)n_frames * groups * dw4;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % dw4) * 4;
        const int gy = (int)((i / dw4) % groups);
        const int f = (int)(i / ((int64_t)dw4 * groups));
        const int y0 = gy * VR;
        int s0[VR];
        float acc[VR][12];
        int lo = 0x7fffffff, hi = -0x7fffffff;
#pragma unroll
        for (int k = 0; k < VR; ++k) {
            const int y = y0 + k < dh ? y0 + k : dh - 1;
            s0[k] = start[y];
            lo = s0[k] < lo ? s0[k] : lo;
            hi = s0[k] + taps - 1 > hi ? s0[k] + taps - 1 : hi;
#pragma unroll
            for (int j = 0; j < 12; ++j) acc[k][j] = 0.f;
        }
        const float* base = tmp + (int64_t)f * sh * dw * 3 + (int64_t)x * 3;
        for (int su = lo; su <= hi; ++su) {
            const int sy = su < 0 ? 0 : (su >= sh ? sh - 1 : su);
            const float4* p4 = reinterpret_cast<const float4*>(base + (int64_t)sy * dw * 3);
            const float4 a = p4[0], b = p4[1], c = p4[2];
            const float p[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
#pragma unroll
            for (int k = 0; k < VR; ++k) {
                const int t = su - s0[k];
                if (t >= 0 && t < taps) {
                    const int y = y0 + k < dh ? y0 + k : dh - 1;
                    const float wt = wts[(int64_t)y * taps + t];
#pragma unroll
                    for (int j = 0; j < 12; ++j) acc[k][j] += wt * p[j];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < VR; ++k) {
            const int y = y0 + k;
            if (y >= dh) break;
            const int64_t o = ((int64_t)(f * dh + y) * dw + x) * 3;
            int v[12];
#pragma unroll
            for (int j = 0; j < 12; ++j) v[j] = sat8((int)floorf(acc[k][j] + 0.5f));
            if (orig) {
                const uint32_t* op = reinterpret_cast<const uint32_t*>(orig + o);
                const uint32_t o0 = op[0], o1 = op[1], o2 = op[2];
                const int ob[12] = {(int)(o0 & 255), (int)((o0 >> 8) & 255), (int)((o0 >> 16) & 255), (int)(o0 >> 24), (int)(o1 & 255), (int)((o1 >> 8) & 255),
                                    (int)((o1 >> 16) & 255), (int)(o1 >> 24), (int)(o2 & 255), (int)((o2 >> 8) & 255), (int)((o2 >> 16) & 255), (int)(o2 >> 24)};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    int yy, u, vv, y2, u2, v2;
                    rgb2yuv(v[q * 3], v[q * 3 + 1], v[q * 3 + 2], yy, u, vv);
                    rgb2yuv(ob[q * 3], ob[q * 3 + 1], ob[q * 3 + 2], y2, u2, v2);
                    yuv2rgb(y2, u, vv, v[q * 3], v[q * 3 + 1], v[q * 3 + 2]);
                }
            }
            uint32_t* dp = reinterpret_cast<uint32_t*>(dst + o);
            dp[0] = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
            dp[1] = (uint32_t)v[4] | ((uint32_t)v[5] << 8) | ((uint32_t)v[6] << 16) | ((uint32_t)v[7] << 24);
            dp[2] = (uint32_t)v[8] | ((uint32_t)v[9] << 8) | ((uint32_t)v[10] << 16) | ((uint32_t)v[11] << 24);
        }
    }
}

// Which horizontal pass launch_resize_passes runs: 0 = resize_h_kernel (one block per row), otherwise the TMAX of the resize_h_rows_kernel instance.
// The batched kernel needs taps <= 48, a tile's staged source span within 4 KiB (four prefetched dwords per thread) and enough blocks to fill the chip.
// *span_lds (optional): the LDS bytes reserved for the span, whichever kernel is chosen.  Pure host arithmetic: havc_resize_plan reports it to the tests.
int resize_h_variant(int sw, int dw, int h_taps, int64_t rows, int* span_lds) {
    // source span of a 256-column tile: 256 outputs step (sw / dw) source pixels each, plus the taps
    const size_t span_px = (size_t)((255.0 * sw) / dw) + h_taps + 4;
    const size_t lds_t = (span_px * 3 + 8 + 15) & ~(size_t)15;
    if (span_lds) *span_lds = lds_t < 0x7fffffff ? (int)lds_t : 0x7fffffff;
    if (h_taps > 48 || lds_t > 4096) return 0;          // (spans up to 4 KiB: four prefetched dwords per thread)
    // 16 rows per block amortise the per-thread tap loads; a single frame (ColorMNet: one squash per call) does not fill the chip that way and
    // keeps the one-block-per-row pass (measured: c5 -0.7 % with one row per block here)
    const int64_t chunks = (rows + RESIZE_H_ROWS_PER_BLOCK - 1) / RESIZE_H_ROWS_PER_BLOCK, xt = (dw + 255) / 256;
    if (chunks * xt < 2048 || chunks > 65535) return 0;
    return h_taps <= 9 ? 9 : h_taps <= 17 ? 17 : h_taps <= 29 ? 29 : h_taps <= 32 ? 32 : 48;
}

int launch_resize_passes(const uint8_t* src, int sw, int sh, uint8_t* dst, int dw, int dh, int n_frames, float* tmp,
                         const int* h_start, const float* h_w, int h_taps, const int* v_start, const float* v_w,
                         int v_taps, const uint8_t* orig, hipStream_t s) {
    const int64_t rows = (int64_t)n_frames * sh;
    int span_lds = 0;
    const int variant = resize_h_variant(sw, dw, h_taps, rows, &span_lds);
    if (variant) {
        const int xt = (dw + 255) / 256, rpb = RESIZE_H_ROWS_PER_BLOCK;
        const int64_t chunks = (rows + rpb - 1) / rpb;
        const int vec_out = ((dw & 3) == 0 && (reinterpret_cast<uintptr_t>(tmp) & 15) == 0) ? 1 : 0;
        const int out_off = span_lds;                                      // [256][3] floats behind the staged span
        const size_t lds_all = (size_t)span_lds + 256 * 3 * sizeof(float);
#define HAVC_RH(T) hipLaunchKernelGGL(resize_h_rows_kernel<T>, dim3(xt, (unsigned)chunks), dim3(256), lds_all, s, src, tmp, h_start, h_w, h_taps, sw, dw, rows, rpb, out_off, vec_out)
        if (variant == 9) HAVC_RH(9);                 // every up-sampling pass
        else if (variant == 17) HAVC_RH(17);
        else if (variant == 29) HAVC_RH(29);          // 1920 -> 560 (c2), 1920 -> 512 is 31 taps
        else if (variant == 32) HAVC_RH(32);
        else HAVC_RH(48);                             // 1920 -> 384 (c4): 41 taps
#undef HAVC_RH
    } else {
        const size_t lds = (size_t)(sw * 3 + 8 + 15) & ~(size_t)15;
        if (lds > 64 * 1024) return (int)hipErrorInvalidValue;            // rows beyond 21 800 pixels: not a video frame
        hipLaunchKernelGGL(resize_h_kernel, dim3((unsigned)(rows < 65535 * 16 ? rows : 65535 * 16)), dim3(256), lds, s, src, tmp, h_start, h_w,
                           h_taps, sw, dw, rows);
    }
    const int groups = (dh + VR - 1) / VR;
    const bool quad = (dw & 3) == 0 && ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(orig)) & 3) == 0 &&
                      (reinterpret_cast<uintptr_t>(tmp) & 15) == 0;
    if (quad)
        hipLaunchKernelGGL(resize_v4_kernel, dim3(grid_for((int64_t)n_frames * groups * (dw >> 2))), dim3(256), 0, s, tmp, dst, orig,
                           v_start, v_w, v_taps, sh, dh, dw, n_frames);
    else
        hipLaunchKernelGGL(resize_v_kernel, dim3(grid_for((int64_t)n_frames * groups * dw)), dim3(256), 0, s, tmp, dst, orig,
                           v_start, v_w, v_taps, sh, dh, dw, n_frames);
    return (int)hipGetLastError();
}

// ---- luma-masked merges (imfilters.py:66-100 -> nputils.py:101-253).  luma = R*0.299 + G*0.587 + B*0.114 in float64,
// exactly as numpy evaluates it ((R*0.299 + G*0.587) + B*0.114).  mode 0: image_luma_merge — hard mask, pixel of
// img_white where luma(img_white) > tresh else img_dark.  mode 1: w_image_luma_merge — weight
// w = float32(clip((luma - tresh) * grad, 0, 1)) (mode 2: w = luma / 255), out = uint8(img_dark*(1-w) + img_white*w). ----
__global__ void luma_merge_kernel(const uint8_t* __restrict__ dark, const uint8_t* __restrict__ white, int mode, double tresh,
                                  double grad, uint8_t* __restrict__ out, int64_t npix) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
        int r, g, b;
        luma_merge_pixel(mode, tresh, grad, dark[i * 3], dark[i * 3 + 1], dark[i * 3 + 2], white[i * 3], white[i * 3 + 1], white[i * 3 + 2], r, g, b);
        out[i * 3] = (uint8_t)r; out[i * 3 + 1] = (uint8_t)g; out[i * 3 + 2] = (uint8_t)b;
    }
}

int launch_luma_merge(const uint8_t* dark, const uint8_t* white, int mode, double tresh, double grad, uint8_t* out, int64_t npix,
                      hipStream_t s) {
    hipLaunchKernelGGL(luma_merge_kernel, dim3(grid_for(npix)), dim3(256), 0, s, dark, white, mode, tresh, grad, out, npix);
    return (int)hipGetLastError();
}

// ---- get_image_luma (imfilters.py:597-601): sum of cv2 Y over the frame (exact integer sum; the host divides) ----
__global__ void luma_sum_kernel(const uint8_t* __restrict__ img, unsigned long long* __restrict__ sum, int64_t npix) {
    unsigned long long acc = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
        int y, u, v;
        rgb2yuv(img[i * 3], img[i * 3 + 1], img[i * 3 + 2], y, u, v);
        acc += (unsigned)y;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) atomicAdd(sum, acc);
}

int launch_luma_sum(const uint8_t* img, unsigned long long* d_sum, int64_t npix, hipStream_t s) {
    (void)hipMemsetAsync(d_sum, 0, sizeof(unsigned long long), s);
    hipLaunchKernelGGL(luma_sum_kernel, dim3(grid_for(npix) > 1024 ? 1024 : grid_for(npix)), dim3(256), 0, s, img, d_sum, npix);
    return (int)hipGetLastError();
}

// ---- _chroma_temporal_limiter (imfilters.py:638-666): U,V of cur clipped into [U_prv(1-a), U_prv(1+a)] with FLOAT64
// bounds (not truncated to uint8 first, unlike chroma_stabilizer), Y,U,V otherwise from cur ----
__global__ void chroma_temporal_limiter_kernel(const uint8_t* __restrict__ cur, const uint8_t* __restrict__ prv, double alpha,
                                               uint8_t* __restrict__ out, int64_t npix) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
        int y1, u1, v1, y2, u2, v2, r, g, b;
        rgb2yuv(prv[i * 3], prv[i * 3 + 1], prv[i * 3 + 2], y1, u1, v1);
        rgb2yuv(cur[i * 3], cur[i * 3 + 1], cur[i * 3 + 2], y2, u2, v2);
        const double u_up = (double)u1 * (1.0 + alpha), u_dn = (double)u1 * (1.0 - alpha);
        const double v_up = (double)v1 * (1.0 + alpha), v_dn = (double)v1 * (1.0 - alpha);
        if ((double)u2 > u_up) u2 = (int)(uint8_t)(int)u_up;
        if ((double)u2 < u_dn) u2 = (int)(uint8_t)(int)u_dn;
        if ((double)v2 > v_up) v2 = (int)(uint8_t)(int)v_up;
        if ((double)v2 < v_dn) v2 = (int)(uint8_t)(int)v_dn;
        yuv2rgb(y2, u2, v2, r, g, b);
        out[i * 3] = (uint8_t)r; out[i * 3 + 1] = (uint8_t)g; out[i * 3 + 2] = (uint8_t)b;
    }
}

int launch_chroma_temporal_limiter(const uint8_t* cur, const uint8_t* prv, double alpha, uint8_t* out, int64_t npix, hipStream_t s) {
    hipLaunchKernelGGL(chroma_temporal_limiter_kernel, dim3(grid_for(npix)), dim3(256), 0, s, cur, prv, alpha, out, npix);
    return (int)hipGetLastError();
}

// ---- chroma_stabilizer_adaptive (imfilters.py:202-269): per-pixel chroma tolerance base_tol + max_extra * texture,
// texture = clip(|Laplacian(Y_stable)| / 255, 0, 1) (cv2.Laplacian CV_32F, aperture 1: [[0,1,0],[1,-4,1],[0,1,0]],
// BORDER_REFLECT_101), on signed chroma (U-128, V-128); float32 like the numpy code ----
__device__ __forceinline__ float y_at(const uint8_t* __restrict__ img, int x, int y, int w, int h) {
    x = w == 1 ? 0 : (x < 0 ? -x : (x >= w ? 2 * w - 2 - x : x));          // BORDER_REFLECT_101; a 1-pixel axis reflects onto itself
    y = h == 1 ? 0 : (y < 0 ? -y : (y >= h ? 2 * h - 2 - y : y));          // (cv::borderInterpolate returns 0 when len == 1)
    const uint8_t* p = img + ((int64_t)y * w + x) * 3;
    int yy, u, v;
    rgb2yuv(p[0], p[1], p[2], yy, u, v);
    return (float)yy;
}

__global__ void chroma_stabilizer_adaptive_kernel(const uint8_t* __restrict__ st, const uint8_t* __restrict__ nw, float base_tol,
                                                  float max_extra, float weight, int do_blend, uint8_t* __restrict__ out, int w, int h) {
    const int64_t npix = (int64_t)w * h;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % w), y = (int)(i / w);
        int y1, u1, v1, y2, u2, v2, r, g, b;
        const int sr = st[i * 3], sg = st[i * 3 + 1], sb = st[i * 3 + 2];
        rgb2yuv(sr, sg, sb, y1, u1, v1);
        rgb2yuv(nw[i * 3], nw[i * 3 + 1], nw[i * 3 + 2], y2, u2, v2);
        const float lap = ((y_at(st, x, y - 1, w, h) + y_at(st, x, y + 1, w, h)) + (y_at(st, x - 1, y, w, h) + y_at(st, x + 1, y, w, h))) -
                          4.0f * (float)y1;
        float tex = fabsf(lap) / 255.0f;
        tex = fminf(fmaxf(tex, 0.0f), 1.0f);
        const float tol = base_tol + max_extra * tex;
        const float su1 = (float)(u1 - 128), sv1 = (float)(v1 - 128);
        const float ul = fminf(fmaxf(su1 - tol, -128.f), 127.f), uh = fminf(fmaxf(su1 + tol, -128.f), 127.f);
        const float vl = fminf(fmaxf(sv1 - tol, -128.f), 127.f), vh = fminf(fmaxf(sv1 + tol, -128.f), 127.f);
        const float um = fminf(fmaxf((float)(u2 - 128), ul), uh), vm = fminf(fmaxf((float)(v2 - 128), vl), vh);
        yuv2rgb(y1, (int)(uint8_t)(int)(um + 128.f), (int)(uint8_t)(int)(vm + 128.f), r, g, b);
        if (do_blend) {
            r = blend1((uint8_t)sr, (uint8_t)r, weight);
            g = blend1((uint8_t)sg, (uint8_t)g, weight);
            b = blend1((uint8_t)sb, (uint8_t)b, weight);
        }
        out[i * 3] = (uint8_t)r; out[i * 3 + 1] = (uint8_t)g; out[i * 3 + 2] = (uint8_t)b;
    }
}

int launch_chroma_stabilizer_adaptive(const uint8_t* stable, const uint8_t* inew, float base_tol, float max_extra, float weight,
                                      uint8_t* out, int w, int h, hipStream_t s) {
    hipLaunchKernelGGL(chroma_stabilizer_adaptive_kernel, dim3(grid_for((int64_t)w * h)), dim3(256), 0, s, stable, inew, base_tol, max_extra,
                       weight, weight < 1.0f ? 1 : 0, out, w, h);
    return (int)hipGetLastError();
}

// ---- _color_temporal_stabilizer (imfilters.py:680-705): U,V = weighted mean over the frame window (float64, centre frame
// first, then the others in list order), truncated to uint8; Y of the centre frame ----
struct FrameList { const uint8_t* f[9]; double w[9]; int n, centre; };

__global__ void color_temporal_stabilizer_kernel(FrameList fl, uint8_t* __restrict__ out, int64_t npix) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
        int yc, u, v, y, r, g, b;
        const uint8_t* pc = fl.f[fl.centre] + i * 3;
        rgb2yuv(pc[0], pc[1], pc[2], yc, u, v);
        double um = (double)u * fl.w[fl.centre], vm = (double)v * fl.w[fl.centre];
        for (int k = 0; k < fl.n; ++k) {
            if (k == fl.centre) continue;
            const uint8_t* p = fl.f[k] + i * 3;
            rgb2yuv(p[0], p[1], p[2], y, u, v);
            um += (double)u * fl.w[k];
            vm += (double)v * fl.w[k];
        }
        yuv2rgb(yc, (int)(uint8_t)(int)um, (int)(uint8_t)(int)vm, r, g, b);
        out[i * 3] = (uint8_t)r; out[i * 3 + 1] = (uint8_t)g; out[i * 3 + 2] = (uint8_t)b;
    }
}

int launch_color_temporal_stabilizer(const uint8_t* const* frames, const double* weights, int n, uint8_t* out, int64_t npix,
                                     hipStream_t s) {
    if (n < 1 || n > 9) return (int)hipErrorInvalidValue;
    FrameList fl;
    fl.n = n;
    fl.centre = (int)lrint((n - 1) / 2.0);      // Python round((n-1)/2): banker's rounding, like lrint
    for (int k = 0; k < n; ++k) { fl.f[k] = frames[k]; fl.w[k] = weights[k]; }
    hipLaunchKernelGGL(color_temporal_stabilizer_kernel, dim3(grid_for(npix)), dim3(256), 0, s, fl, out, npix);
    return (int)hipGetLastError();
}

// Eager module load (havc_create, under the library's set-up mutex): the HIP runtime loads a translation unit's code object on the first use
// of one of its kernels; querying one here moves that -- and the big-LDS opt-ins below -- out of the first launch, which may come from
// several host threads at once ("set-up is serialised").
void preload_colorfilters() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(resize_h_kernel)); (void)hipGetLastError(); }
