// HAVC_clip_slice / HAVC_clip_reconstruct (vsdeoldify/__init__.py:2886-2945 -> vsslib/vstiles4.py), the tiling of the Placebo / VerySlow presets.
//
// slice: std.AddBorders (black, right / bottom by the overlaps) + four (two) std.CropAbs -> ONE launch that writes every tile clip; the black border
// is produced here (a tile pixel whose source lies outside the clip is 0), there is no memset and no per-tile loop on the host.
//
// reconstruct: _blend_horizontal(tl, tr), _blend_horizontal(bl, br), _blend_vertical(top, bottom), std.CropAbs to the clip's size and the optional luma
// re-attach -> ONE launch that reads each tile pixel it needs once and writes the output once.  The reference's blends are std.MaskedMerge with a
// position mask (akarin.Expr); MaskedMerge itself is VapourSynth native code, its stand-in here is out = (a * (255 - m) + b * m + 127) / 255 per channel
// (m = 0 -> a, m = 255 -> b exactly).  Each stage is rounded to u8 like the reference's two MaskedMerge passes.  A tile is only READ where its mask is
// not at the other end -- which is also what keeps every read inside the tile: left / top tiles are read for x < base + overlap, right / bottom tiles for
// x >= base - overlap, the ranges they cover.  The luma re-attach is pixel_ops.h's yuv_merge_pixel, the body of havc_chroma_post_process.
//
// Access pattern (as stabilizer.hip): a thread owns four neighbouring pixels of one row = 12 bytes, moved as one 96-bit access.  Tile row pitches
// (base_w + overlap_x) * 3 and odd widths put those 12 bytes at any byte offset, so they are moved with memcpy semantics: correct for every alignment, and
// the gfx950 code object (unaligned access mode) gets one global_load_dwordx3 / global_store_dwordx3 for each.  Groups that straddle the end of a row, the
// edge of a tile or of the clip go pixel by pixel.  No LDS, no scratch.
#include "kernels.h"
#include "pixel_ops.h"

// load12 / store12: pixel_ops.h
__device__ __forceinline__ uint8_t* tile_ptr(const TileArgs& a, int t) { return t == 0 ? a.tile[0] : (t == 1 ? a.tile[1] : (t == 2 ? a.tile[2] : a.tile[3])); }

// ---- slice -------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) tile_slice_kernel(const uint8_t* __restrict__ clip, TileArgs a) {
    const int tw = a.base_w + a.ox, th = a.base_h + a.oy;
    const int gpr = (tw + 3) >> 2;                                                   // groups of four pixels per tile row
    const int64_t total = (int64_t)a.n_tiles * a.n * th * gpr;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int g = (int)(i % gpr);
        int64_t r = i / gpr;
        const int ty = (int)(r % th);
        r /= th;
        const int f = (int)(r % a.n), t = (int)(r / a.n);
        const int left = (t & 1) ? a.base_w - a.ox : 0, top = (t & 2) ? a.base_h - a.oy : 0;       // vstiles4.py:89-98, 147-149
        const int tx0 = g * 4, sx0 = tx0 + left, sy = ty + top;
        uint8_t* dst = tile_ptr(a, t) + (((int64_t)f * th + ty) * tw + tx0) * 3;
        const int64_t src_off = (((int64_t)f * a.h + sy) * a.w + sx0) * 3;                         // dereferenced only where (sx, sy) is inside the clip
        const int cnt = min(4, tw - tx0);
        int v[12];
        if (cnt == 4 && sy < a.h && sx0 + 4 <= a.w) {
            load12(clip + src_off, v);
            store12(dst, v);
        } else if (cnt == 4 && (sy >= a.h || sx0 >= a.w)) {
#pragma unroll
            for (int k = 0; k < 12; ++k) v[k] = 0;
            store12(dst, v);
        } else {
            for (int q = 0; q < cnt; ++q) {
                const bool inside = sy < a.h && sx0 + q < a.w;
                for (int c = 0; c < 3; ++c) dst[q * 3 + c] = inside ? clip[src_off + q * 3 + c] : (uint8_t)0;
            }
        }
    }
}

// ---- reconstruct -------------------------------------------------------------------------------------------------------------------------------
// _make_horizontal_blend_mask_akarin / _make_vertical_blend_mask_akarin (vstiles4.py:281-312) at position x; overlap <= 0: the blend is a plain stack
// (:316-317, :337-338).  The linear ramp divides by the overlap, not by twice the overlap: it reaches 255 at x = base.
__device__ __forceinline__ int tile_mask(int x, int base, int ov, int mask_val) {
    if (ov <= 0) return x >= base ? 255 : 0;
    const int start = base - ov, end = base + ov;
    if (x >= end) return 255;
    if (mask_val != 0) return x < start ? 0 : mask_val;
    if (x <= start) return 0;
    const int v = ((x - start) * 510 + ov) / (2 * ov);                               // floor((x - start) * 255 / ov + 0.5)
    return v > 255 ? 255 : v;
}
__device__ __forceinline__ int blend255(int a, int b, int m) { return (a * (255 - m) + b * m + 127) / 255; }

// _blend_horizontal of one pixel: l / r = the row in the left / right tile, sx = base_w - ox = where the right tile starts
__device__ __forceinline__ void tile_h_pixel(const uint8_t* l, const uint8_t* r, int x, int sx, int m, int px[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (m == 0) px[c] = l[x * 3 + c];
        else if (m == 255) px[c] = r[(x - sx) * 3 + c];
        else px[c] = blend255(l[x * 3 + c], r[(x - sx) * 3 + c], m);
    }
}
// ... of four pixels x0 .. x0 + 3 whose reads stay inside the tiles (tile_group_ok)
__device__ __forceinline__ void tile_h_group(const uint8_t* l, const uint8_t* r, int x0, int sx, const int m[4], int o[12]) {
    if (m[3] == 0) load12(l + x0 * 3, o);                                            // the masks do not decrease along a row
    else if (m[0] == 255) load12(r + (x0 - sx) * 3, o);
    else {
        int va[12], vb[12];
        load12(l + x0 * 3, va);
        load12(r + (x0 - sx) * 3, vb);
#pragma unroll
        for (int k = 0; k < 12; ++k) o[k] = blend255(va[k], vb[k], m[k / 3]);
    }
}

__global__ void __launch_bounds__(256) tile_reconstruct_kernel(TileArgs a, const uint8_t* __restrict__ orig, uint8_t* __restrict__ out) {
    const int tw = a.base_w + a.ox, th = a.base_h + a.oy;
    const int sx = a.base_w - a.ox, sy = a.base_h - a.oy;
    const int gpr = (a.w + 3) >> 2;
    const int64_t total = (int64_t)a.n * a.h * gpr;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int x0 = (int)(i % gpr) * 4;
        const int64_t r = i / gpr;
        const int y = (int)(r % a.h);
        const int64_t f = r / a.h;
        const int my = tile_mask(y, a.base_h, a.oy, a.mask_val);                     // 2 tiles: base_h = h, oy = 0 -> 0 on every row
        // rows of the four tiles this output row blends; a pointer is only formed for a tile that is read
        const uint8_t *tl = nullptr, *tr = nullptr, *bl = nullptr, *br = nullptr;
        if (my < 255) { const int64_t o = (f * th + y) * tw * 3; tl = a.tile[0] + o; tr = a.tile[1] + o; }
        if (my > 0) { const int64_t o = (f * th + (y - sy)) * tw * 3; bl = a.tile[2] + o; br = a.tile[3] + o; }
        const int64_t off = ((f * a.h + y) * a.w + x0) * 3;
        int m[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) m[q] = tile_mask(x0 + q, a.base_w, a.ox, a.mask_val);
        const bool group_ok = x0 + 4 <= a.w && (m[3] == 0 || m[0] == 255 || (x0 + 4 <= tw && x0 >= sx));
        if (group_ok) {
            int v[12];
            if (my == 0) tile_h_group(tl, tr, x0, sx, m, v);
            else if (my == 255) tile_h_group(bl, br, x0, sx, m, v);
            else {
                int vt[12], vb[12];
                tile_h_group(tl, tr, x0, sx, m, vt);
                tile_h_group(bl, br, x0, sx, m, vb);
#pragma unroll
                for (int k = 0; k < 12; ++k) v[k] = blend255(vt[k], vb[k], my);
            }
            if (orig) {
                int vo[12];
                load12(orig + off, vo);
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    yuv_merge_pixel(v[q * 3], v[q * 3 + 1], v[q * 3 + 2], vo[q * 3], vo[q * 3 + 1], vo[q * 3 + 2], v[q * 3], v[q * 3 + 1], v[q * 3 + 2]);
            }
            store12(out + off, v);
        } else {
            const int cnt = min(4, a.w - x0);
            for (int q = 0; q < cnt; ++q) {
                const int x = x0 + q;
                int p[3], pb[3];
                if (my < 255) tile_h_pixel(tl, tr, x, sx, m[q], p);
                if (my > 0) tile_h_pixel(bl, br, x, sx, m[q], pb);
#pragma unroll
                for (int c = 0; c < 3; ++c) p[c] = my == 0 ? p[c] : (my == 255 ? pb[c] : blend255(p[c], pb[c], my));
                if (orig) {
                    const uint8_t* po = orig + off + q * 3;
                    yuv_merge_pixel(p[0], p[1], p[2], po[0], po[1], po[2], p[0], p[1], p[2]);
                }
                for (int c = 0; c < 3; ++c) out[off + q * 3 + c] = (uint8_t)p[c];
            }
        }
    }
}

static dim3 tile_grid(int64_t groups) {
    const int64_t blocks = (groups + 255) / 256;
    return dim3((unsigned)(blocks < 1 ? 1 : (blocks > 16384 ? 16384 : blocks)));
}

int launch_tile_slice(const uint8_t* clip, const TileArgs& a, hipStream_t s) {
    const int64_t groups = (int64_t)a.n_tiles * a.n * (a.base_h + a.oy) * ((a.base_w + a.ox + 3) >> 2);
    hipLaunchKernelGGL(tile_slice_kernel, tile_grid(groups), dim3(256), 0, s, clip, a);
    return (int)hipGetLastError();
}

int launch_tile_reconstruct(const TileArgs& a, const uint8_t* orig, uint8_t* out, hipStream_t s) {
    const int64_t groups = (int64_t)a.n * a.h * ((a.w + 3) >> 2);
    hipLaunchKernelGGL(tile_reconstruct_kernel, tile_grid(groups), dim3(256), 0, s, a, orig, out);
    return (int)hipGetLastError();
}

// Eager module load (havc_create, under the library's set-up mutex), like every other translation unit ("set-up is serialised").
void preload_tiles() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(tile_reconstruct_kernel)); (void)hipGetLastError(); }
