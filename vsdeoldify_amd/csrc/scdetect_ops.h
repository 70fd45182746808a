// Scene-detection arithmetic shared by the kernel (scdetect.hip) and the host (havc_scene_norm_value, which the CPU tests call).
#pragma once
#include <stdint.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

// vsutils.frame_normalize (vsslib/vsutils.py:304-318) on one gray value: uint8(255 * ((y - min) / (max - min))) in numpy's float64 sequence -- an IEEE
// double division, then the multiplication, then truncation.  k = y - min, d = max - min, 0 <= k <= d <= 255.  d == 0 (a flat frame) is NaN in the
// reference; defined as 0 here.
__host__ __device__ inline int scene_norm_value(int k, int d) {
    if (d <= 0 || k <= 0) return 0;
    if (k >= d) return 255;
    const double q = (double)k / (double)d;
    return (int)(255.0 * q);
}

// frame_normalize's test on the frame's own mean luma: normalised only when tht_black < mean / 255 < tht_white (float64, as np.mean(u8) / 255.0)
__host__ __device__ inline bool scene_norm_applies(long long sum_y, long long npix, double tht_black, double tht_white) {
    const double luma = ((double)sum_y / (double)npix) / 255.0;
    return !(luma <= tht_black || luma >= tht_white);
}

// entry t (a raw gray value) of a frame's table: the stretched value when frame_normalize applies to the frame, t itself otherwise
__host__ __device__ inline int scene_lut_entry(int t, long long sum_raw, int min_y, int max_y, long long npix, double tht_black, double tht_white) {
    if (!scene_norm_applies(sum_raw, npix, tht_black, tht_white)) return t;
    const int d = max_y > min_y ? max_y - min_y : 0;
    const int k = t - min_y;
    return scene_norm_value(k < 0 ? 0 : (k > d ? d : k), max_y - min_y);
}

// havc_scene_stats only lets coefficients through that keep Y <= 255; the mask is what keeps the table index of the second pass inside its 256 entries
// for any other caller of launch_scene_stats: such a caller gets wrong sums, never a read outside the table.
struct SceneLuma { int cr, cg, cb, bias; };
__host__ __device__ inline int scene_gray(const SceneLuma& c, int r, int g, int b) { return ((c.cr * r + c.cg * g + c.cb * b + c.bias) >> 16) & 255; }

// the four gray values of a 12-byte group of four pixels held in three little-endian dwords
__host__ __device__ inline void scene_gray4(const SceneLuma& c, const uint32_t w[3], int y[4]) {
    y[0] = scene_gray(c, w[0] & 255u, (w[0] >> 8) & 255u, (w[0] >> 16) & 255u);
    y[1] = scene_gray(c, w[0] >> 24, w[1] & 255u, (w[1] >> 8) & 255u);
    y[2] = scene_gray(c, (w[1] >> 16) & 255u, w[1] >> 24, w[2] & 255u);
    y[3] = scene_gray(c, (w[2] >> 8) & 255u, (w[2] >> 16) & 255u, w[2] >> 24);
}

struct SceneSums { unsigned sum, sad, max, imin; };       // imin = 255 - min

// What ONE thread adds up: the groups first, first + stride, ... of a frame of npix pixels at `cur`, compared with the frame at `prv` when diff.  A group is
// the 12 bytes of pixels 4i .. 4i + 3, moved as one access at any alignment; the last npix % 4 pixels go byte by byte.  Nothing beyond npix * 3 bytes of
// either frame is read.  lut0 / lut1 (MODE 2): the tables of the frame and of the compared frame.  MODE as scene_stats_kernel's.
template <int MODE>
__host__ __device__ inline void scene_accumulate(const SceneLuma& c, const uint8_t* cur, const uint8_t* prv, bool diff, int64_t npix, const uint8_t* lut0,
                                                 const uint8_t* lut1, int64_t first, int64_t stride, SceneSums& s) {
    const int64_t ngroups = (npix + 3) >> 2;
    for (int64_t i = first; i < ngroups; i += stride) {
        int y[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
        int cnt = 4;
        if (i * 4 + 4 <= npix) {
            uint32_t w[3];
            __builtin_memcpy(w, cur + i * 12, 12);
            scene_gray4(c, w, y);
            if (diff) {
                __builtin_memcpy(w, prv + i * 12, 12);
                scene_gray4(c, w, q);
            }
        } else {
            cnt = (int)(npix - i * 4);
            for (int j = 0; j < cnt; ++j) {
                const int64_t o = (i * 4 + j) * 3;
                y[j] = scene_gray(c, cur[o], cur[o + 1], cur[o + 2]);
                if (diff) q[j] = scene_gray(c, prv[o], prv[o + 1], prv[o + 2]);
            }
        }
        for (int j = 0; j < cnt; ++j) {
            int v = y[j], u = q[j];
            if (MODE != 2) {
                s.max = s.max > (unsigned)v ? s.max : (unsigned)v;
                s.imin = s.imin > (unsigned)(255 - v) ? s.imin : (unsigned)(255 - v);
            } else {
                v = lut0[v];
                u = lut1[u];
            }
            s.sum += (unsigned)v;
            if (diff) s.sad += (unsigned)(v > u ? v - u : u - v);
        }
    }
}
