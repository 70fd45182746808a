// Per-pixel bodies of the u8 RGB tweak / luma-merge filters, shared by their stand-alone kernels (tweaks.hip, colorfilters.hip) and by the fused
// HAVC_stabilizer chain (stabilizer.hip) and the tile reconstruct (tiles.hip): ONE statement of the arithmetic, so that the fused launch and the chain of single launches give the same bytes.
// Arithmetic restates Pillow's C (libImaging Convert.c / Blend.c: float locals, double intermediates, truncating casts), OpenCV's 8-bit HSV integer
// path and numpy's float64 merges; see oracle/tweaks.py, oracle/cvcolor.py.  Every translation unit that includes this file is built with
// -ffp-contract=off: Pillow's / numpy's products are rounded before the add.
#pragma once
#include "kernels.h"

__device__ __forceinline__ int clip8i(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// ---- four neighbouring pixels = 12 bytes as one 96-bit access at any byte alignment (memcpy semantics; the gfx950 code object runs in unaligned access
// mode and gets one global_load_dwordx3 / global_store_dwordx3 for each): the access pattern of tiles.hip and recover.hip ----
__device__ __forceinline__ void load12(const uint8_t* p, int v[12]) {
    uint32_t w[3];
    __builtin_memcpy(w, p, 12);
#pragma unroll
    for (int i = 0; i < 12; ++i) v[i] = (int)((w[i >> 2] >> ((i & 3) * 8)) & 255u);
}
__device__ __forceinline__ void store12(uint8_t* p, const int v[12]) {
    uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 12; ++i) w[i >> 2] |= (uint32_t)v[i] << ((i & 3) * 8);
    __builtin_memcpy(p, w, 12);
}

// ---- OpenCV RGB2YUV / YUV2RGB, 8-bit (color_yuv.simd.hpp RGB2YCrCb_i / YCrCb2RGB_i, isCrCb=false) ----
__device__ __forceinline__ int descale14(int x) { return (x + (1 << 13)) >> 14; }
__device__ __forceinline__ int sat8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__device__ __forceinline__ void rgb2yuv(int r, int g, int b, int& y, int& u, int& v) {
    y = descale14(r * 4899 + g * 9617 + b * 1868);
    u = sat8(descale14((b - y) * 8061 + (128 << 14)));
    v = sat8(descale14((r - y) * 14369 + (128 << 14)));
    y = sat8(y);
}
__device__ __forceinline__ void yuv2rgb(int y, int u, int v, int& r, int& g, int& b) {
    u -= 128;
    v -= 128;
    b = sat8(y + descale14(u * 33292));
    g = sat8(y + descale14(u * -6472 + v * -9519));
    r = sat8(y + descale14(v * 18678));
}
// chroma_post_process / vs_recover_clip_luma (imfilters.py:312-321, vsfilters.py:863-899), one pixel: Y of the original, U and V of the colour pixel
__device__ __forceinline__ void yuv_merge_pixel(int cr, int cg, int cb, int or_, int og, int ob, int& r, int& g, int& b) {
    int y, u, v, y2, u2, v2;
    rgb2yuv(cr, cg, cb, y, u, v);
    rgb2yuv(or_, og, ob, y2, u2, v2);
    yuv2rgb(y2, u, v, r, g, b);
}

// ---- Pillow rgb2hsv_row / hsv2rgb (Convert.c, "following colorsys.py") ----
__device__ __forceinline__ void pil_rgb2hsv(int r, int g, int b, int& uh, int& us, int& uv) {
    const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
    uv = maxc;
    if (minc == maxc) { uh = 0; us = 0; return; }
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = ((float)(maxc - r)) / cr, gc = ((float)(maxc - g)) / cr, bc = ((float)(maxc - b)) / cr;
    float h;
    if (r == maxc) h = bc - gc;
    else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    h = (float)fmod((double)h / 6.0 + 1.0, 1.0);
    uh = clip8i((int)((double)h * 255.0));
    us = clip8i((int)((double)s * 255.0));
}
__device__ __forceinline__ void pil_hsv2rgb(int h, int s, int v, int& r, int& g, int& b) {
    if (s == 0) { r = g = b = v; return; }
    const double hd = (double)(float)h * 6.0 / 255.0;
    const int i = (int)floor(hd);
    const float f = (float)(hd - (double)(float)i);
    const float fs = (float)((double)(float)s / 255.0);
    const double vd = (double)(float)v;
    const int p = clip8i((int)round(vd * (1.0 - (double)fs)));
    const int q = clip8i((int)round(vd * (1.0 - (double)fs * (double)f)));
    const int t = clip8i((int)round(vd * (1.0 - (double)fs * (1.0 - (double)f))));
    switch (i % 6) {
        case 0: r = v; g = t; b = p; break;
        case 1: r = q; g = v; b = p; break;
        case 2: r = p; g = v; b = t; break;
        case 3: r = p; g = q; b = v; break;
        case 4: r = t; g = p; b = v; break;
        default: r = v; g = p; b = q; break;
    }
}
// Pillow ImagingBlend(im1 = degenerate a, im2 = image b, alpha) incl. the extrapolating branch (ImageEnhance factors > 1)
__device__ __forceinline__ int pil_blendx(int a, int b, float alpha) {
    const float prod = alpha * (float)(b - a);
    const float t = (float)a + prod;
    if (alpha >= 0.f && alpha <= 1.f) return (int)(uint8_t)(int)t;
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}
__device__ __forceinline__ int pil_L(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// ---- OpenCV RGB2HSV_b (hrange 180): 12-bit reciprocal tables built with cvRound ----
__device__ __forceinline__ void cv_rgb2hsv(int r, int g, int b, int& h, int& s, int& v) {
    v = max(r, max(g, b));
    const int vmin = min(r, min(g, b)), diff = v - vmin;
    const int sdiv = v ? __double2int_rn((double)(255 << 12) / (double)v) : 0;
    const int hdiv = diff ? __double2int_rn((double)(180 << 12) / (6.0 * (double)diff)) : 0;
    s = (diff * sdiv + (1 << 11)) >> 12;
    int hh = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
    hh = (hh * hdiv + (1 << 11)) >> 12;
    h = hh < 0 ? hh + 180 : hh;
}
// OpenCV HSV2RGB_b -> HSV2RGB_f (float32 throughout, reciprocal multiplies), saturate_cast<uchar>(cvRound(x * 255))
__device__ __forceinline__ void cv_hsv2rgb(int h8, int s8, int v8, int& r, int& g, int& b) {
    const float hscale = 6.0f / 180.0f, inv255 = 1.0f / 255.0f;
    float h = (float)h8 * hscale;
    const float s = (float)s8 * inv255, v = (float)v8 * inv255;
    if (s8 == 0) { r = g = b = clip8i((int)rintf(v * 255.0f)); return; }
    if (h >= 6.0f) h -= 6.0f;
    const int i = (int)floorf(h);
    const float f = h - (float)i;
    const float p = v * (1.f - s), q = v * (1.f - s * f), t = v * (1.f - s * (1.f - f));
    float rf, gf, bf;
    switch (i) {
        case 0: rf = v; gf = t; bf = p; break;
        case 1: rf = q; gf = v; bf = p; break;
        case 2: rf = p; gf = v; bf = t; break;
        case 3: rf = p; gf = q; bf = v; break;
        case 4: rf = t; gf = p; bf = v; break;
        default: rf = v; gf = p; bf = q; break;
    }
    r = clip8i((int)rintf(rf * 255.0f)); g = clip8i((int)rintf(gf * 255.0f)); b = clip8i((int)rintf(bf * 255.0f));
}

// ---- image_tweak (imfilters.py:463-504), one pixel, in the two halves the Contrast step cuts it into (ImageEnhance.Contrast needs the mean Pillow-L
// of the image BETWEEN them).  head: hue shift + Brightness; tail: Contrast, Color, hue-range mask against the original (r0, g0, b0). ----
__device__ __forceinline__ void image_tweak_head(const TweakArgs& a, int& r, int& g, int& b) {
    if (a.hue_offset != 0) {
        int h, s, v;
        pil_rgb2hsv(r, g, b, h, s, v);
        h = ((h + a.hue_offset) % 256 + 256) % 256;           // numpy int16 %: non-negative
        pil_hsv2rgb(h, s, v, r, g, b);
    }
    if (a.brightness != 1.f) { r = pil_blendx(0, r, a.brightness); g = pil_blendx(0, g, a.brightness); b = pil_blendx(0, b, a.brightness); }
}
__device__ __forceinline__ void image_tweak_tail(const TweakArgs& a, int r0, int g0, int b0, int& r, int& g, int& b) {
    if (a.contrast != 1.f) { r = pil_blendx(a.mean_l, r, a.contrast); g = pil_blendx(a.mean_l, g, a.contrast); b = pil_blendx(a.mean_l, b, a.contrast); }
    if (a.color != 1.f) {
        const int L = pil_L(r, g, b);
        r = pil_blendx(L, r, a.color); g = pil_blendx(L, g, a.color); b = pil_blendx(L, b, a.color);
    }
    if (a.n_ranges > 0) {                                     // np_adjust_chroma2: tweaked pixel only inside the hue ranges of the ORIGINAL
        int h, s, v;
        cv_rgb2hsv(r0, g0, b0, h, s, v);
        bool cond = false;
        for (int k = 0; k < a.n_ranges; ++k) cond |= ((double)h > a.range_lo[k] * 0.5) && ((double)h < a.range_hi[k] * 0.5);
        if (!cond) { r = r0; g = g0; b = b0; }
    }
}

// ---- image_chroma_tweak (imfilters.py:540-548 -> restcolor.py:288-350), one pixel: cv2 HSV hue / saturation / value tweak, then the optional
// "hue_adjust" stage (hue range on the TWEAKED hue -> re-tweaked colour, everything else the ORIGINAL pixel, weighted merges) ----
__device__ __forceinline__ int cv_hue_add(int h, double hue_half) {          // nputils.py:330-340 + the uint8 slice assignment
    double t = (double)h + hue_half;
    t = t > 180.0 ? t - 180.0 : t;
    t = t < 0.0 ? t + 180.0 : t;
    return (int)(uint8_t)(long long)t;
}
__device__ __forceinline__ int wmerge1(int a, int b, double w) {
    const double m = (double)a * (1.0 - w) + (double)b * w;
    return (int)(m < 0.0 ? 0.0 : (m > 255.0 ? 255.0 : m));
}
__device__ __forceinline__ void chroma_tweak_pixel(const ChromaTweakArgs& a, int r0, int g0, int b0, int& r, int& g, int& b) {
    int h, s, v;
    cv_rgb2hsv(r0, g0, b0, h, s, v);
    if (a.has_hue) h = cv_hue_add(h, a.hue_half);
    s = (int)(uint8_t)(long long)((double)s * a.satc);
    v = (int)(uint8_t)(long long)((double)v * a.brightc);
    if (a.has_adjust == 2) { r = r0; g = g0; b = b0; }      // adjust_chroma (restcolor.py:243-286): no tweak stage, no HSV round trip in front
    else cv_hsv2rgb(h, s, v, r, g, b);
    if (a.has_adjust) {
        int hg, sg, vg;
        cv_rgb2hsv(r, g, b, hg, sg, vg);
        if (a.has_hue2) hg = cv_hue_add(hg, a.hue_half2);
        if (a.has_sat2) sg = (int)(uint8_t)(long long)((double)sg * a.sat2c);
        int gr, gg, gb;
        cv_hsv2rgb(hg, sg, vg, gr, gg, gb);
        bool cond = false;
        for (int k = 0; k < a.n_ranges; ++k) cond |= ((double)h > a.range_lo[k] * 0.5) && ((double)h < a.range_hi[k] * 0.5);
        r = cond ? gr : r0; g = cond ? gg : g0; b = cond ? gb : b0;
        if (a.weight > 0.0) {
            const bool to_gray = !a.has_hue2;
            r = wmerge1(r, to_gray ? gr : r0, a.weight); g = wmerge1(g, to_gray ? gg : g0, a.weight); b = wmerge1(b, to_gray ? gb : b0, a.weight);
        }
        if (a.weight < 0.0) { r = wmerge1(r, r0, -a.weight); g = wmerge1(g, g0, -a.weight); b = wmerge1(b, b0, -a.weight); }
    }
}

// ---- luma-masked merges (imfilters.py:66-100 -> nputils.py:101-253), one pixel.  luma = R*0.299 + G*0.587 + B*0.114 of the WHITE pixel in float64,
// exactly as numpy evaluates it ((R*0.299 + G*0.587) + B*0.114).  mode 0: image_luma_merge -- hard mask, pixel of img_white where luma > tresh else
// img_dark.  mode 1: w_image_luma_merge -- weight w = float32(clip((luma - tresh) * grad, 0, 1)); mode 2: w = luma / 255; mode 3: w = uint8(luma) / 255;
// out = uint8(img_dark*(1-w) + img_white*w). ----
__device__ __forceinline__ void luma_merge_pixel(int mode, double tresh, double grad, int dr, int dg, int db, int r2, int g2, int b2, int& r, int& g,
                                                 int& b) {
    double luma = ((double)r2 * 0.299 + (double)g2 * 0.587) + (double)b2 * 0.114;
    luma = fmin(fmax(luma, 0.0), 255.0);
    if (mode == 0) {
        const bool wsel = luma > tresh;
        r = wsel ? r2 : dr; g = wsel ? g2 : dg; b = wsel ? b2 : db;
        return;
    }
    double wgt;
    if (mode == 1) {
        double lg = (luma - tresh) * grad;
        float w32 = (float)(lg > 1.0 ? 1.0 : lg);          // array_max(.., 1.0).astype(float32)
        w32 = w32 < 0.0f ? 0.0f : w32;                      // array_min(.., 0.0).astype(float32)
        wgt = (double)w32;
    } else if (mode == 2) {
        wgt = luma / 255.0;                                 // w_np_rgb_to_gray(as_weight=True, dark_luma <= 0)
    } else {
        wgt = (double)(int)luma / 255.0;                    // image_luma_merge(luma=0): mask stored as uint8, then / 255
    }
    const double wb = 1.0 - wgt;
    const int dark_px[3] = {dr, dg, db}, white_px[3] = {r2, g2, b2};
    int o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double p1 = (double)dark_px[c] * wb;
        const double p2 = (double)white_px[c] * wgt;
        const double v = fmin(fmax(p1 + p2, 0.0), 255.0);
        o[c] = (int)(uint8_t)(int)v;
    }
    r = o[0]; g = o[1]; b = o[2];
}

// ---- restore_color_gradient / restore_color (restcolor.py:98-217, 38-83), one pixel: the body of havc_restore_color_gradient (tweaks.hip) and of both
// paths of havc_recover_color_clip (recover.hip) ----
// w_np_gradient_mask (restcolor.py:137-217) from the cv2 HSV saturation s of the GRAY pixel: white (255) where it is gray.  algo 0: float64; 1, 2: float32
// steps, then float64
__device__ __forceinline__ int restore_gradient_mask(int s, int tht, double alpha, int algo) {
    if (algo == 0) {
        const double sd = (double)s;
        const double grad = s < tht ? 2.0 * sd / alpha - (double)tht : 2.0 * (sd - (double)tht) * alpha;
        double m = 255.0 - (double)tht - grad;
        m = m < 0.0 ? 0.0 : (m > 255.0 ? 255.0 : m);
        return (int)m;
    }
    const int t = tht < 0 ? 0 : (tht > 255 ? 255 : tht);
    if (t == 0) return 0;
    const float sf = (float)s;
    double mn;
    if (algo == 1) {
        const float max_s = (float)min(2 * t, 200);
        const float sc = fminf(fmaxf(sf, 0.f), max_s);
        mn = (double)powf(1.0f - sc / max_s, (float)alpha);
    } else {
        const float s_rel = fminf(fmaxf(sf / (float)t, 0.f), 2.f);
        mn = exp((double)((float)(-alpha) * s_rel) * 0.6931471805599453);
        if (sf >= (float)(2 * t)) mn = 0.0;
    }
    double m = mn * 255.0;
    m = m < 0.0 ? 0.0 : (m > 255.0 ? 255.0 : m);
    return (int)m;
}
// the colour pixel with its cv2 HSV saturation scaled by clip(sat, 0, 10): numpy float64 -> uint8 assignment (wraps above 255)
__device__ __forceinline__ void restore_desaturate(int& cr, int& cg, int& cb, double sat, bool scale) {
    int ch, cs, cv;
    cv_rgb2hsv(cr, cg, cb, ch, cs, cv);
    if (scale) {
        const double sc = sat < 0.0 ? 0.0 : (sat > 10.0 ? 10.0 : sat);
        cs = (int)(uint8_t)(long long)((double)cs * sc);
    }
    cv_hsv2rgb(ch, cs, cv, cr, cg, cb);
}
// restore_color_gradient: w_np_image_mask_merge(gray, colour, mask, normalize=True), then np_weighted_merge towards the colour pixel (weight > 0) or the
// gray one (weight < 0); sat == 1.0 leaves the saturation alone (the HSV round trip still runs); return_mask: the mask on the three channels
__device__ __forceinline__ void restore_gradient_pixel(int cr, int cg, int cb, int gr, int gg, int gb, double sat, int tht, double alpha, double weight,
                                                       int algo, int return_mask, int o[3]) {
    int h, s, v;
    cv_rgb2hsv(gr, gg, gb, h, s, v);
    const int mask = restore_gradient_mask(s, tht, alpha, algo);
    if (return_mask) { o[0] = o[1] = o[2] = mask; return; }
    restore_desaturate(cr, cg, cb, sat, sat != 1.0);
    const double mw = (double)mask / 255.0, mb = 1.0 - mw;
    const int src_g[3] = {gr, gg, gb}, src_c[3] = {cr, cg, cb};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double m = (double)src_g[k] * mb + (double)src_c[k] * mw;
        int r = (int)(m < 0.0 ? 0.0 : (m > 255.0 ? 255.0 : m));
        if (weight > 0.0) r = wmerge1(r, src_c[k], weight);
        if (weight < 0.0) r = wmerge1(r, src_g[k], -weight);
        o[k] = r;
    }
}
// restore_color with tht_scen = 1.0 and hue_adjust 'none' (restcolor.py:38-83; its early return needs tht_scen < 1): mask = 255 where s < tht, else 0;
// np_image_mask_merge picks the desaturated colour pixel under a white mask (products by exactly 0.0 and 1.0); the saturation product runs for every sat;
// the weighted merge goes the OTHER way round: weight > 0 towards the gray pixel, weight < 0 towards the desaturated colour pixel
__device__ __forceinline__ void restore_binary_pixel(int cr, int cg, int cb, int gr, int gg, int gb, double sat, int tht, double weight, int return_mask,
                                                     int o[3]) {
    int h, s, v;
    cv_rgb2hsv(gr, gg, gb, h, s, v);
    const bool white = s < tht;
    if (return_mask) { o[0] = o[1] = o[2] = white ? 255 : 0; return; }
    restore_desaturate(cr, cg, cb, sat, true);
    const int src_g[3] = {gr, gg, gb}, src_c[3] = {cr, cg, cb};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int r = white ? src_c[k] : src_g[k];
        if (weight > 0.0) r = wmerge1(r, src_g[k], weight);
        if (weight < 0.0) r = wmerge1(r, src_c[k], -weight);
        o[k] = r;
    }
}
