// The frame-level decisions of havc_chroma_stab_clip, shared by the kernels (tweak.hip's restoring forward kernel, chroma_stab.hip) and the host
// (rt_filters.cpp: havc_chroma_stab_frame_params, which the CPU tests call).  tests/stab_util.py `frame_decision` is the definition.
#pragma once
#include "equalize_ops.h"

#define CS_STANDARD_DARK 0.22            // vsslib/constants.py:28-29
#define CS_STANDARD_BRIGHT 0.78
#define CS_BINARY_FIRST 15               // vsfilters.py:337: `if n < 15: return f_out`
#define CS_MAX_WEIGHTS 15
#define CS_MAX_WINDOW 1024               // source frames of a chunk: their scene-change flags travel as two 1024-bit masks in the kernel arguments

// One frame of a shifted clip, from the sum of cv2's Y and the count of pixels with cv2 HSV saturation < tht, both over the whole frame:
//   color_frame (vsfilters.py:343-348): f_luma = round(sum / n_pixels / 255, 6); outside 0.22 <= f_luma <= 0.78 the weight becomes min(weight, -0.8)
//   restore_color (restcolor.py:53-61): scenechange = np.mean(mask) / 255 with the mask 255 / 0 = ((255 count) / n_pixels) / 255 in float64; with
//   0 < tht_scen < 1 and scenechange > tht_scen the frame comes back untouched
// -> true when the gate is taken; eff: the weight the per-pixel path uses
__host__ __device__ inline bool cs_frame_decision(unsigned long long sum_y, unsigned long long gray_count, long long npix, double weight, double tht_scen,
                                                  double& eff) {
#pragma clang fp contract(off)
    const double f_luma = eq_f_luma(sum_y, npix, 0);
    eff = weight;
    if (!(CS_STANDARD_DARK <= f_luma && f_luma <= CS_STANDARD_BRIGHT)) eff = weight < -0.8 ? weight : -0.8;
    const double mean = (double)(255ull * gray_count) / (double)npix;
    const double frac = mean / 255.0;
    return tht_scen > 0.0 && tht_scen < 1.0 && frac > tht_scen;
}
