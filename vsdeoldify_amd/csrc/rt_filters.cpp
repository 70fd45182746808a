// libhavc_mi355.so runtime, filters: the per-pixel filter entry points, tiles, scene statistics and equalisation.
#include "runtime_internal.h"
#include "scdetect_ops.h"
#include "scfilter_ops.h"
#include "scedge_ops.h"
#include "equalize_ops.h"
#include "retinex_ops.h"
#include "tweak_ops.h"
#include "vformat_ops.h"
#include "chroma_stab_ops.h"
#include "lut3d_ops.h"
#include "overlay_ops.h"
#include "metrics_ops.h"
#include <cstddef>

extern "C" {

int havc_blend(havc_ctx* c, const uint8_t* a, const uint8_t* b, float w, uint8_t* out, int width, int height) {
    if (!c || !a || !b || !out || width <= 0 || height <= 0) return fail(c, HAVC_E_INVALID, "blend: bad args");
    const size_t nb = (size_t)width * height * 3;
    return run_filter(c, a, b, out, nb, "blend", [&](const uint8_t* da, const uint8_t* db, uint8_t* dout) {
        return launch_blend_u8(da, db, w, dout, (int64_t)nb, c->stream); });
}

int havc_chroma_post_process(havc_ctx* c, const uint8_t* color, const uint8_t* orig, uint8_t* out, int width, int height) {
    if (!c || !color || !orig || !out || width <= 0 || height <= 0) return fail(c, HAVC_E_INVALID, "chroma_post_process: bad args");
    return run_filter(c, color, orig, out, (size_t)width * height * 3, "chroma_post_process", [&](const uint8_t* da, const uint8_t* db, uint8_t* dout) {
        return launch_yuv_merge(da, db, dout, (int64_t)width * height, c->stream); });
}

int havc_chroma_stabilizer(havc_ctx* c, const uint8_t* img_stable, const uint8_t* img_new, double alpha, double weight,
                           uint8_t* out, int width, int height) {
    if (!c || !img_stable || !img_new || !out || width <= 0 || height <= 0) return fail(c, HAVC_E_INVALID, "chroma_stabilizer: bad args");
    return run_filter(c, img_stable, img_new, out, (size_t)width * height * 3, "chroma_stabilizer", [&](const uint8_t* da, const uint8_t* db, uint8_t* dout) {
        return launch_chroma_stabilizer(da, db, alpha, (float)weight, dout, (int64_t)width * height, c->stream); });
}

int havc_chroma_stabilizer_adaptive(havc_ctx* c, const uint8_t* img_stable, const uint8_t* img_new, double base_tol, double max_extra,
                                    double weight, uint8_t* out, int width, int height) {
    if (!c || !img_stable || !img_new || !out || width <= 0 || height <= 0) return fail(c, HAVC_E_INVALID, "chroma_stabilizer_adaptive: bad args");
    if (out == img_stable) return fail(c, HAVC_E_INVALID, "chroma_stabilizer_adaptive: out must not alias img_stable (Laplacian neighbourhood)");
    return run_filter(c, img_stable, img_new, out, (size_t)width * height * 3, "chroma_stabilizer_adaptive", [&](const uint8_t* da, const uint8_t* db, uint8_t* dout) {
        return launch_chroma_stabilizer_adaptive(da, db, (float)base_tol, (float)max_extra, (float)weight, dout, width, height, c->stream); });
}

int havc_chroma_temporal_limiter(havc_ctx* c, const uint8_t* cur, const uint8_t* prv, double alpha, uint8_t* out, int width, int height) {
    if (!c || !cur || !prv || !out || width <= 0 || height <= 0) return fail(c, HAVC_E_INVALID, "chroma_temporal_limiter: bad args");
    return run_filter(c, cur, prv, out, (size_t)width * height * 3, "chroma_temporal_limiter", [&](const uint8_t* da, const uint8_t* db, uint8_t* dout) {
        return launch_chroma_temporal_limiter(da, db, alpha, dout, (int64_t)width * height, c->stream); });
}

int havc_image_luma_merge(havc_ctx* c, const uint8_t* img_dark, const uint8_t* img_white, int mode, double tresh, double grad, uint8_t* out,
                          int width, int height) {
    if (!c || !img_dark || !img_white || !out || width <= 0 || height <= 0 || mode < 0 || mode > 3) return fail(c, HAVC_E_INVALID, "image_luma_merge: bad args");
    return run_filter(c, img_dark, img_white, out, (size_t)width * height * 3, "image_luma_merge", [&](const uint8_t* da, const uint8_t* db, uint8_t* dout) {
        return launch_luma_merge(da, db, mode, tresh, grad, dout, (int64_t)width * height, c->stream); });
}

int havc_image_luma(havc_ctx* c, const uint8_t* img, int width, int height, double* mean_y) {
    if (!c || !img || !mean_y || width <= 0 || height <= 0) return fail(c, HAVC_E_INVALID, "image_luma: bad args");
    Call call(c, "image_luma");
    unsigned long long sum = 0;
    const uint8_t* din = call.in(SCR_IN, img, (size_t)width * height * 3);
    void* d_sum = call.download(&sum, call.scratch(SCR_SMALL, 256), sizeof(sum));
    if (call.rc) return call.rc;
    call.launched(launch_luma_sum(din, (unsigned long long*)d_sum, (int64_t)width * height, c->stream));
    if (call.done()) return call.rc;
    *mean_y = (double)sum / ((double)width * (double)height);
    return HAVC_OK;
}

int havc_image_tweak(havc_ctx* c, const uint8_t* img, uint8_t* out, int width, int height, int hue_offset, float brightness, float contrast,
                     float color, const double* hue_ranges, int n_ranges) {
    if (!c || !img || !out || width <= 0 || height <= 0 || n_ranges < 0 || n_ranges > HAVC_MAX_HUE_RANGES || (n_ranges && !hue_ranges))
        return fail(c, HAVC_E_INVALID, "image_tweak: bad args (at most 8 hue ranges)");
    Call call(c, "image_tweak");
    const size_t nb = (size_t)width * height * 3;
    const int64_t npix = (int64_t)width * height;
    const uint8_t* din = call.in(SCR_IN, img, nb);
    uint8_t* dout = call.out(SCR_OUT, out, nb);
    unsigned long long* d_sum = (unsigned long long*)call.scratch(SCR_SMALL, 256);
    if (call.rc) return call.rc;
    TweakArgs a{};
    a.hue_offset = hue_offset; a.brightness = brightness; a.contrast = contrast; a.color = color; a.mean_l = 0; a.n_ranges = n_ranges;
    for (int k = 0; k < n_ranges; ++k) { a.range_lo[k] = hue_ranges[2 * k]; a.range_hi[k] = hue_ranges[2 * k + 1]; }
    if (contrast != 1.f) {
        // ImageEnhance.Contrast: degenerate = solid int(mean(L) + 0.5) of the image as it enters the step
        unsigned long long sum = 0;
        call.launched(launch_image_tweak(din, dout, npix, a, d_sum, true, c->stream));
        call.copy(&sum, d_sum, sizeof(sum), hipMemcpyDeviceToHost);
        call.sync();
        if (call.rc) return call.rc;
        a.mean_l = (int)((double)sum / (double)npix + 0.5);
    }
    call.launched(launch_image_tweak(din, dout, npix, a, d_sum, false, c->stream));
    return call.done();
}

// the argument normalisation of np_image_chroma_tweak (restcolor.py:288-350): clamps, half-degree hue steps, which sub-steps run
static ChromaTweakArgs chroma_tweak_args(double sat, double bright, int hue, int has_adjust, const double* hue_ranges, int n_ranges, double adj_sat,
                                         int adj_hue, double adj_weight) {
    auto clampd = [](double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); };
    ChromaTweakArgs a{};
    a.has_hue = hue != 0; a.hue_half = 0.5 * (double)std::min(std::max(hue, -360), 360);
    a.satc = clampd(sat, 0.0, 10.0); a.brightc = clampd(1.0 + bright, 0.0, 10.0);
    a.has_adjust = has_adjust == 2 ? 2 : (has_adjust != 0); a.n_ranges = has_adjust ? n_ranges : 0;
    if (has_adjust == 2) { a.has_hue = 0; a.satc = 1.0; a.brightc = 1.0; }
    for (int k = 0; k < a.n_ranges; ++k) { a.range_lo[k] = hue_ranges[2 * k]; a.range_hi[k] = hue_ranges[2 * k + 1]; }
    a.has_hue2 = adj_hue != 0; a.hue_half2 = 0.5 * (double)std::min(std::max(adj_hue, -360), 360);
    a.has_sat2 = adj_sat != 1.0; a.sat2c = clampd(adj_sat, 0.0, 10.0);
    a.weight = adj_weight;
    return a;
}

int havc_image_chroma_tweak(havc_ctx* c, const uint8_t* img, uint8_t* out, int width, int height, double sat, double bright, int hue,
                            int has_adjust, const double* hue_ranges, int n_ranges, double adj_sat, int adj_hue, double adj_weight) {
    if (!c || !img || !out || width <= 0 || height <= 0 || n_ranges < 0 || n_ranges > HAVC_MAX_HUE_RANGES || (has_adjust && (!hue_ranges || n_ranges < 1)))
        return fail(c, HAVC_E_INVALID, "image_chroma_tweak: bad args (1..8 hue ranges with an adjust stage)");
    const ChromaTweakArgs a = chroma_tweak_args(sat, bright, hue, has_adjust, hue_ranges, n_ranges, adj_sat, adj_hue, adj_weight);
    return run_filter(c, img, nullptr, out, (size_t)width * height * 3, "image_chroma_tweak", [&](const uint8_t* da, const uint8_t*, uint8_t* dout) {
        return launch_chroma_tweak(da, dout, (int64_t)width * height, a, c->stream); });
}

int havc_stabilizer_chain(havc_ctx* c, const uint8_t* img, uint8_t* out, int width, int height, const havc_stab_stage* stages, int n_stages) {
    if (!c || !img || !out || width <= 0 || height <= 0 || n_stages < 0 || n_stages > HAVC_MAX_STAB_STAGES || (n_stages && !stages))
        return fail(c, HAVC_E_INVALID, "stabilizer_chain: bad args (0..3 stages)");
    StabChainArgs a{};
    a.n = n_stages;
    for (int i = 0; i < n_stages; ++i) {
        const havc_stab_stage& s = stages[i];
        if (s.kind < 0 || s.kind > 1 || s.merge_mode < -1 || s.merge_mode > 3 || s.n_ranges < 0 || s.n_ranges > HAVC_MAX_HUE_RANGES ||
            (s.kind == 1 && (s.has_adjust < 0 || s.has_adjust > 1 || (s.has_adjust && s.n_ranges < 1))))
            return fail(c, HAVC_E_INVALID, "stabilizer_chain: bad stage (kind 0 / 1, merge_mode -1..3, at most 8 hue ranges, 1..8 with an adjust stage)");
        StabStage& d = a.st[i];
        d.kind = s.kind; d.identity = s.kind == 1 && s.identity; d.merge_mode = s.merge_mode; d.tresh = s.tresh; d.grad = s.grad;
        if (s.kind == 0) {
            d.tw.hue_offset = s.hue_offset; d.tw.brightness = s.brightness; d.tw.contrast = 1.f; d.tw.color = s.color; d.tw.mean_l = 0;
            d.tw.n_ranges = s.n_ranges;
            for (int k = 0; k < s.n_ranges; ++k) { d.tw.range_lo[k] = s.hue_ranges[2 * k]; d.tw.range_hi[k] = s.hue_ranges[2 * k + 1]; }
        } else {
            d.ct = chroma_tweak_args(s.sat, s.bright, s.hue, s.has_adjust, s.hue_ranges, s.n_ranges, s.adj_sat, s.adj_hue, s.adj_weight);
        }
    }
    const size_t nb = (size_t)width * height * 3;
    return run_filter(c, img, nullptr, out, nb, "stabilizer_chain", [&](const uint8_t* da, const uint8_t*, uint8_t* dout) {
        if (a.n == 0) return da == dout ? 0 : (int)hipMemcpyAsync(dout, da, nb, hipMemcpyDeviceToDevice, c->stream);
        return launch_stabilizer_chain(da, dout, (int64_t)width * height, a, c->stream); });
}

// ---- HAVC_clip_slice / HAVC_clip_reconstruct (tiles.hip) ----
// what keeps every read and write of the two kernels inside its buffer: the tiles cover the clip, the overlaps are smaller than the base tile
static const char* tile_geom_error(const havc_tile_geom* g) {
    if (!g || g->width <= 0 || g->height <= 0 || g->n_frames <= 0) return "bad args";
    if (g->n_tiles != 2 && g->n_tiles != 4) return "n_tiles must be 2 or 4";
    if (g->base_w <= 0 || g->base_h <= 0 || g->width > 2 * g->base_w) return "the tiles do not cover the clip's width";
    if (g->n_tiles == 4 ? g->height > 2 * g->base_h : (g->height != g->base_h || g->overlap_y != 0))
        return "the tiles do not cover the clip's height (2 tiles: base_h = height, overlap_y = 0)";
    if (g->overlap_x < 0 || g->overlap_y < 0 || g->overlap_x >= g->base_w || (g->n_tiles == 4 && g->overlap_y >= g->base_h))
        return "an overlap must be >= 0 and smaller than the base tile";
    if (g->mask_val < 0 || g->mask_val > 255) return "mask_val must be 0..255";
    return nullptr;
}
static TileArgs tile_args(const havc_tile_geom* g) {
    TileArgs a{};
    a.w = g->width; a.h = g->height; a.n = g->n_frames; a.n_tiles = g->n_tiles;
    a.base_w = g->base_w; a.base_h = g->base_h; a.ox = g->overlap_x; a.oy = g->overlap_y; a.mask_val = g->mask_val;
    return a;
}

int havc_tile_slice(havc_ctx* c, const uint8_t* clip, uint8_t* const* tiles, const havc_tile_geom* g) {
    if (!c || !clip || !tiles) return fail(c, HAVC_E_INVALID, "tile_slice: bad args");
    if (const char* why = tile_geom_error(g)) return fail(c, HAVC_E_INVALID, (std::string("tile_slice: ") + why).c_str());
    for (int t = 0; t < g->n_tiles; ++t) if (!tiles[t]) return fail(c, HAVC_E_INVALID, "tile_slice: NULL tile");
    Call call(c, "tile_slice");
    TileArgs a = tile_args(g);
    const size_t cb = (size_t)a.n * a.h * a.w * 3, tb = (size_t)a.n * (a.base_h + a.oy) * (a.base_w + a.ox) * 3;
    const uint8_t* d_clip = call.in(SCR_IN, clip, cb);
    Call::Pack host_tiles(SCR_OUT);
    for (int t = 0; t < a.n_tiles; ++t) call.add(host_tiles, tiles[t], tb);
    call.reserve(host_tiles);
    for (int t = 0; t < a.n_tiles; ++t) a.tile[t] = call.out(host_tiles, tiles[t], tb);
    if (call.rc) return call.rc;
    call.launched(launch_tile_slice(d_clip, a, c->stream));
    return call.done();
}

int havc_tile_reconstruct(havc_ctx* c, const uint8_t* const* tiles, const uint8_t* clip_orig, uint8_t* out, const havc_tile_geom* g) {
    if (!c || !tiles || !out) return fail(c, HAVC_E_INVALID, "tile_reconstruct: bad args");
    if (const char* why = tile_geom_error(g)) return fail(c, HAVC_E_INVALID, (std::string("tile_reconstruct: ") + why).c_str());
    if (g->recover_luma && !clip_orig) return fail(c, HAVC_E_INVALID, "tile_reconstruct: recover_luma needs clip_orig");
    for (int t = 0; t < g->n_tiles; ++t)
        if (!tiles[t] || tiles[t] == out) return fail(c, HAVC_E_INVALID, "tile_reconstruct: NULL tile, or out is a tile");
    if (g->recover_luma && clip_orig == out) return fail(c, HAVC_E_INVALID, "tile_reconstruct: out must not be clip_orig");
    Call call(c, "tile_reconstruct");
    TileArgs a = tile_args(g);
    const size_t cb = (size_t)a.n * a.h * a.w * 3, tb = (size_t)a.n * (a.base_h + a.oy) * (a.base_w + a.ox) * 3;
    const uint8_t* orig = g->recover_luma ? clip_orig : nullptr;
    Call::Pack inputs(SCR_IN);                                           // the host tiles and a host clip_orig share one staging buffer
    for (int t = 0; t < a.n_tiles; ++t) call.add(inputs, tiles[t], tb);
    if (orig) call.add(inputs, orig, cb);
    call.reserve(inputs);
    uint8_t* dout = call.out(SCR_OUT, out, cb);
    for (int t = 0; t < a.n_tiles; ++t) a.tile[t] = const_cast<uint8_t*>(call.in(inputs, tiles[t], tb));
    if (orig) orig = call.in(inputs, orig, cb);
    if (call.rc) return call.rc;
    call.launched(launch_tile_reconstruct(a, orig, dout, c->stream));
    return call.done();
}

// ---- HAVC_SceneDetect's per-frame statistics (scdetect.hip) ----
static_assert(sizeof(SceneRec) == sizeof(havc_scene_rec) && sizeof(havc_scene_rec) == 32, "havc_scene_rec layout");

int havc_scene_norm_value(int k, int d) { return scene_norm_value(k, d); }

// what scdetect.hip and scedge.hip ask of the integer luma coefficients: the 16.16 sum stays a byte
static int luma_coef_check(havc_ctx* c, const char* what, int cr, int cg, int cb, int bias) {
    if (cr < 0 || cg < 0 || cb < 0 || bias < 0 || ((int64_t)cr + cg + cb) * 255 + bias >= ((int64_t)256 << 16))
        return fail(c, HAVC_E_INVALID, std::string(what) + ": luma coefficients must be >= 0 and keep Y = (cr*R + cg*G + cb*B + bias) >> 16 below 256");
    return HAVC_OK;
}

int havc_scene_stats(havc_ctx* c, const uint8_t* clip, const havc_scene_params* p, havc_scene_rec* out) {
    if (!c || !clip || !p || !out) return fail(c, HAVC_E_INVALID, "scene_stats: bad args");
    if (p->width <= 0 || p->height <= 0 || p->n_frames <= 0 || (int64_t)p->width * p->height > ((int64_t)1 << 31))
        return fail(c, HAVC_E_INVALID, "scene_stats: bad clip size (at most 2^31 pixels per frame)");
    if (p->offset < 1 || p->offset > 25) return fail(c, HAVC_E_INVALID, "scene_stats: offset must be 1..25");
    if (int rc = luma_coef_check(c, "scene_stats", p->cr, p->cg, p->cb, p->bias)) return rc;
    if (p->normalize && !(p->tht_black >= 0.0 && p->tht_white <= 1.0 && p->tht_black <= p->tht_white))
        return fail(c, HAVC_E_INVALID, "scene_stats: normalize needs 0 <= tht_black <= tht_white <= 1");
    if (is_device_ptr(out)) return fail(c, HAVC_E_INVALID, "scene_stats: the records are downloaded: out must be host memory");
    Call call(c, "scene_stats");
    SceneStatsArgs a{};
    a.n = p->n_frames; a.h = p->height; a.w = p->width; a.offset = p->offset;
    a.cr = p->cr; a.cg = p->cg; a.cb = p->cb; a.bias = p->bias;
    a.normalize = p->normalize != 0; a.tht_black = p->tht_black; a.tht_white = p->tht_white;
    const size_t cb = (size_t)a.n * a.h * a.w * 3, rb = (size_t)a.n * sizeof(SceneRec);
    const uint8_t* d_clip = call.in(SCR_IN, clip, cb);
    SceneRec* d_rec = (SceneRec*)call.download(out, call.scratch(SCR_SMALL, rb), rb);
    if (call.rc) return call.rc;
    call.zero(d_rec, rb);
    call.launched(launch_scene_stats(d_clip, d_rec, a, c->stream), a.normalize ? 2 : 1);
    if (call.done()) return call.rc;
    for (int i = 0; i < a.n; ++i) out[i].min_y = 255 - out[i].min_y;       // kept as 255 - min on the device (scdetect.hip)
    return HAVC_OK;
}

// ---- the SSIM / histogram scene filter's pixel work (scfilter.hip) ----
int havc_scene_gray(int r, int g, int b) { return scf_gray(r & 255, g & 255, b & 255); }

double havc_scene_ssim_value(int sx, int sy, int sxx, int syy, int sxy) { return scf_ssim_value(sx, sy, sxx, syy, sxy); }

// what both entry points ask of their clip and index list; the list is host memory and every entry a frame of the clip, so no kernel reads outside it
static int scene_list_check(havc_ctx* c, const char* what, const void* clip, int n_frames, int width, int height, const int* list, int count, const void* out) {
    const std::string w(what);
    if (!c || !clip || !list || !out) return fail(c, HAVC_E_INVALID, w + ": bad args");
    if (n_frames <= 0 || width <= 0 || height <= 0 || (int64_t)width * height > ((int64_t)1 << 31))
        return fail(c, HAVC_E_INVALID, w + ": bad clip size (at most 2^31 pixels per frame)");
    if (count <= 0 || count > (1 << 24)) return fail(c, HAVC_E_INVALID, w + ": the list must have 1..2^24 entries");
    if (is_device_ptr(list) || is_device_ptr(out)) return fail(c, HAVC_E_INVALID, w + ": the list and the result are host memory");
    return HAVC_OK;
}

int havc_scene_hist(havc_ctx* c, const uint8_t* clip, int n_frames, int width, int height, const int* idx, int k, uint32_t* out) {
    int rc = scene_list_check(c, "scene_hist", clip, n_frames, width, height, idx, k, out);
    if (rc) return rc;
    for (int i = 0; i < k; ++i)
        if (idx[i] < 0 || idx[i] >= n_frames) return fail(c, HAVC_E_INVALID, "scene_hist: a frame number is outside the clip");
    Call call(c, "scene_hist");
    const size_t cb = (size_t)n_frames * height * width * 3, ib = (size_t)k * sizeof(int), ob = (size_t)k * 256 * sizeof(uint32_t);
    const uint8_t* d_clip = call.in(SCR_IN, clip, cb);
    const int* d_idx = call.in(SCR_IN2, idx, ib);
    unsigned* d_hist = (unsigned*)call.download(out, call.scratch(SCR_SMALL, ob), ob);
    if (call.rc) return call.rc;
    call.zero(d_hist, ob);
    call.launched(launch_scene_hist(d_clip, d_idx, k, d_hist, height, width, c->stream));
    return call.done();
}

int havc_scene_ssim(havc_ctx* c, const uint8_t* clip, int n_frames, int width, int height, const int* pairs, int m, double* out) {
    int rc = scene_list_check(c, "scene_ssim", clip, n_frames, width, height, pairs, m, out);
    if (rc) return rc;
    if (width < 7 || height < 7) return fail(c, HAVC_E_INVALID, "scene_ssim: the 7 x 7 window needs frames of at least 7 x 7");
    for (int i = 0; i < 2 * m; ++i)
        if (pairs[i] < 0 || pairs[i] >= n_frames) return fail(c, HAVC_E_INVALID, "scene_ssim: a frame number is outside the clip");
    const int64_t tiles = scene_ssim_tiles(height, width);
    if ((int64_t)m * tiles > 0x7FFFFFFFll) return fail(c, HAVC_E_INVALID, "scene_ssim: too many pairs for one launch at this size");
    Call call(c, "scene_ssim");
    const size_t cb = (size_t)n_frames * height * width * 3, pb = (size_t)m * 2 * sizeof(int), ob = (size_t)m * sizeof(double);
    const uint8_t* d_clip = call.in(SCR_IN, clip, cb);
    const int* d_pairs = call.in(SCR_IN2, pairs, pb);
    double* d_out = (double*)call.download(out, call.scratch(SCR_SMALL, ob * (size_t)(1 + tiles)), ob);      // m results, then m * tiles partials
    if (call.rc) return call.rc;
    call.launched(launch_scene_ssim(d_clip, d_pairs, m, d_out + m, d_out, height, width, c->stream), 2);
    return call.done();
}

// ---- HAVC_SceneDetectEdges' per-frame statistics (scedge.hip) ----
static_assert(sizeof(EdgeRec) == sizeof(havc_edge_rec) && sizeof(havc_edge_rec) == 32, "havc_edge_rec layout");
static_assert(sizeof(havc_edge_params) == 40, "havc_edge_params layout");

int havc_scene_edge_tables(double sigma, uint8_t* enh256, float* weights17, int* radius) {
    if (!enh256 || !weights17 || !radius || !(sigma > 0.0 && sigma <= 2.5)) return HAVC_E_INVALID;
    *radius = edge_radius(sigma);
    for (int k = 0; k < EDGE_MAX_TAPS; ++k) weights17[k] = 0.f;
    edge_weights(sigma, *radius, weights17);
    edge_enhance_table(enh256);
    return HAVC_OK;
}

int havc_scene_edge_stats(havc_ctx* c, const uint8_t* clip, const havc_edge_params* p, havc_edge_rec* out, uint8_t* mask_tap) {
    if (!c || !clip || !p || !out) return fail(c, HAVC_E_INVALID, "scene_edge_stats: bad args");
    if (p->width <= 0 || p->height <= 0 || p->n_frames <= 0 || p->width > EDGE_MAX_SIDE || p->height > EDGE_MAX_SIDE)
        return fail(c, HAVC_E_INVALID, "scene_edge_stats: bad clip size (at most 16384 x 16384)");
    if (p->offset < 1 || p->offset > 25) return fail(c, HAVC_E_INVALID, "scene_edge_stats: offset must be 1..25");
    if (p->offset >= p->n_frames) return fail(c, HAVC_E_INVALID, "scene_edge_stats: offset must be smaller than the number of frames");
    if (int rc = luma_coef_check(c, "scene_edge_stats", p->cr, p->cg, p->cb, p->bias)) return rc;
    if (!(p->sigma > 0.0 && p->sigma <= 2.5)) return fail(c, HAVC_E_INVALID, "scene_edge_stats: sigma must be in (0, 2.5]");
    if (is_device_ptr(out)) return fail(c, HAVC_E_INVALID, "scene_edge_stats: the records are downloaded: out must be host memory");
    Call call(c, "scene_edge_stats");
    EdgeStatsArgs a{};
    a.n = p->n_frames; a.h = p->height; a.w = p->width; a.offset = p->offset;
    a.cr = p->cr; a.cg = p->cg; a.cb = p->cb; a.bias = p->bias;
    a.radius = edge_radius(p->sigma);
    edge_weights(p->sigma, a.radius, a.wt);
    edge_enhance_table(a.enh);
    const size_t pb = (size_t)a.n * a.h * a.w, cb = pb * 3, rb = (size_t)a.n * sizeof(EdgeRec);
    const uint8_t* d_clip = call.in(SCR_IN, clip, cb);
    EdgeRec* d_rec = (EdgeRec*)call.download(out, call.scratch(SCR_SMALL, rb), rb);
    uint8_t* d_tap = call.out(SCR_OUT, mask_tap, pb);                    // NULL without a tap
    if (call.rc) return call.rc;
    call.zero(d_rec, rb);
    call.launched(launch_scene_edge_stats(d_clip, d_rec, d_tap, a, c->stream));
    return call.done();
}

// ---- HAVC_bw_tune / HAVC_auto_levels: rgb_balance + rgb_equalizer on a clip (equalize.hip) ----
static_assert(sizeof(havc_equalize_params) == 600, "havc_equalize_params layout");

int havc_equalize_frame_params(int64_t sum_y, const int64_t* chan_sums, int64_t n_pixels, int range_tv, const double* rgb_factor, double* out) {
    if (sum_y < 0 || n_pixels <= 0 || !out) return HAVC_E_INVALID;
    const double fl = eq_f_luma((unsigned long long)sum_y, n_pixels, range_tv);
    out[0] = fl;
    out[1] = eq_gate(fl) ? 1.0 : 0.0;
    out[2] = (double)eq_blend_weight(fl, 0.40, 0.90, 0.35, 2.0);
    out[3] = (double)eq_blend_weight(fl, 0.40, 0.90, 0.15, 4.0);
    out[4] = out[5] = out[6] = 1.0;
    if (chan_sums && rgb_factor) {
        if (chan_sums[0] < 0 || chan_sums[1] < 0 || chan_sums[2] < 0) return HAVC_E_INVALID;
        const unsigned long long ch[3] = {(unsigned long long)chan_sums[0], (unsigned long long)chan_sums[1], (unsigned long long)chan_sums[2]};
        float g[3];
        eq_balance_gains(ch, n_pixels, rgb_factor, g);
        for (int k = 0; k < 3; ++k) out[4 + k] = (double)g[k];
    }
    return HAVC_OK;
}

int havc_equalize_clip(havc_ctx* c, const uint8_t* src, uint8_t* dst, const havc_equalize_params* p) {
    if (!c || !src || !dst || !p) return fail(c, HAVC_E_INVALID, "equalize_clip: bad args");
    if (src == dst) return fail(c, HAVC_E_INVALID, "equalize_clip: dst must not be src (the histograms are taken of the whole frame first)");
    if (p->n_frames <= 0 || p->width < EQ_GRID || p->height < EQ_GRID || (int64_t)p->width * p->height > ((int64_t)1 << 30))
        return fail(c, HAVC_E_INVALID, "equalize_clip: bad clip size (at least 8 x 8, at most 2^30 pixels per frame)");
    if (p->method < 0 || p->method > 3) return fail(c, HAVC_E_INVALID, "equalize_clip: method must be 0..3");
    auto unit = [](double v) { return v >= 0.0 && v <= 1.0; };
    if (!unit(p->weight) || !unit(p->weight3) || !unit(p->balance_weight)) return fail(c, HAVC_E_INVALID, "equalize_clip: weights must be in [0, 1]");
    if (!(p->clip_limit >= 0.0 && p->clip_limit <= 1e6)) return fail(c, HAVC_E_INVALID, "equalize_clip: clip_limit must be in [0, 1e6]");
    for (int k = 0; k < 3; ++k)
        if (p->balance && !(p->rgb_factor[k] >= 0.0 && p->rgb_factor[k] <= 16.0)) return fail(c, HAVC_E_INVALID, "equalize_clip: rgb_factor must be in [0, 16]");
    Call call(c, "equalize_clip");
    EqArgs a{};
    a.n = p->n_frames; a.h = p->height; a.w = p->width; a.method = p->method;
    a.luma_blend = p->luma_blend != 0; a.range_tv = p->range_tv != 0; a.balance = p->balance != 0;
    a.w15 = eq_w15(p->weight); a.w3_15 = eq_w15(p->weight3); a.bal_w15 = eq_w15(p->balance_weight);
    a.clip_limit = p->clip_limit;
    for (int k = 0; k < 3; ++k) a.factor[k] = p->rgb_factor[k];
    memcpy(a.lut_in, p->lut_in, 256);
    memcpy(a.lut_out, p->lut_out, 256);
    const size_t cb = (size_t)a.n * a.h * a.w * 3, wb = equalize_workspace_bytes(a.n, a.method);
    const uint8_t* d_src = call.in(SCR_IN, src, cb);
    uint8_t* d_dst = call.out(SCR_OUT, dst, cb);
    void* d_ws = call.scratch(SCR_SMALL, wb);
    if (call.rc) return call.rc;
    call.zero(d_ws, (size_t)a.n * (sizeof(EqFrameRec) + 3 * 256 * sizeof(unsigned)));
    call.launched(launch_equalize(d_src, d_dst, d_ws, a, c->stream), a.balance ? 3 : 2);
    return call.done();
}

// ---- HAVC_retinex: multi-scale Retinex (MSRCP) on a clip, chunk by chunk (retinex.hip) ----
static_assert(sizeof(havc_retinex_params) == 120, "havc_retinex_params layout");
static_assert(sizeof(RetFrameRec) == 56, "RetFrameRec layout");

int havc_retinex_coefficients(double sigma, double* out4) {
    if (!out4 || !(sigma >= 0.5 && sigma <= 10000.0)) return HAVC_E_INVALID;
    ret_coefficients(sigma, out4);
    return HAVC_OK;
}

int havc_retinex_frame_params(int64_t sum_y, int64_t n_pixels, int range_tv, double luma_dark, double luma_bright, int blend, double* out) {
    if (sum_y < 0 || n_pixels <= 0 || !out) return HAVC_E_INVALID;
    const double fl = eq_f_luma((unsigned long long)sum_y, n_pixels, range_tv);
    out[0] = fl;
    out[1] = ret_gate(fl, luma_dark, luma_bright) ? 1.0 : 0.0;
    out[2] = (double)ret_blend_weight(fl, blend);
    return HAVC_OK;
}

// Frames per chunk.  The recursions of a launch are rows x frames x sigmas (horizontal) or columns x frames x sigmas (vertical), one lane each; the step
// is a dependent chain of one product and three sums behind seven issued instructions, so about two waves per SIMD keep a SIMD issuing: 256 CUs x 4
// SIMDs x 2 waves x 64 lanes = 131072 lanes for the smaller of the two launches.  The planes of a chunk are capped at 2 GiB.
static int retinex_chunk_frames(const havc_retinex_params* p) {
    if (p->chunk_frames > 0) return std::min(p->chunk_frames, p->n_frames);
    const int64_t lanes = (int64_t)std::min(p->width, p->height) * p->n_sigmas;
    const int64_t want = (131072 + lanes - 1) / lanes;
    const int64_t cap = std::max<int64_t>(1, ((int64_t)2 << 30) / ((int64_t)p->width * p->height * p->n_sigmas * (int64_t)sizeof(double)));
    return (int)std::max<int64_t>(1, std::min<int64_t>(std::min(want, cap), p->n_frames));
}

int havc_retinex_clip(havc_ctx* c, const uint8_t* src, uint8_t* dst, const havc_retinex_params* p, double* tap) {
    if (!c || !src || !dst || !p) return fail(c, HAVC_E_INVALID, "retinex_clip: bad args");
    if (src == dst) return fail(c, HAVC_E_INVALID, "retinex_clip: dst must not be src (the blend and the gate read the input frame)");
    if (p->n_frames <= 0 || p->width <= 0 || p->height <= 0 || (int64_t)p->width * p->height > ((int64_t)1 << 28))
        return fail(c, HAVC_E_INVALID, "retinex_clip: bad clip size (at most 2^28 pixels per frame)");
    if (p->n_sigmas < 1 || p->n_sigmas > RET_MAX_SIGMAS) return fail(c, HAVC_E_INVALID, "retinex_clip: n_sigmas must be 1..8");
    for (int k = 0; k < p->n_sigmas; ++k)
        if (!(p->sigma[k] >= 0.5 && p->sigma[k] <= 10000.0)) return fail(c, HAVC_E_INVALID, "retinex_clip: every sigma must be in [0.5, 10000]");
    if (!(p->luma_dark == p->luma_dark) || !(p->luma_bright == p->luma_bright)) return fail(c, HAVC_E_INVALID, "retinex_clip: luma_dark / luma_bright is NaN");
    if (p->chunk_frames < 0) return fail(c, HAVC_E_INVALID, "retinex_clip: chunk_frames must be >= 0");
    Call call(c, "retinex_clip");
    RetArgs a{};
    a.h = p->height; a.w = p->width; a.ns = p->n_sigmas;
    a.sF = p->fulls ? 0 : 16; a.sR = p->fulls ? 255 : 219;
    a.dF = p->fulld ? 0 : 16; a.dR = p->fulld ? 255 : 219;
    a.range_tv = p->range_tv != 0; a.blend = p->blend != 0;
    a.luma_dark = p->luma_dark; a.luma_bright = p->luma_bright;
    for (int k = 0; k < a.ns; ++k) ret_coefficients(p->sigma[k], a.coef[k]);
    const int chunk = retinex_chunk_frames(p);
    const size_t npix = (size_t)a.h * a.w, fb = npix * 3, cb = (size_t)p->n_frames * fb, pb = npix * sizeof(double);
    const uint8_t* d_src = call.in(SCR_IN, src, cb);
    uint8_t* d_dst = call.out(SCR_OUT, dst, cb);
    void* d_rec = call.scratch(SCR_SMALL, retinex_record_bytes(chunk));
    double* d_planes = (double*)call.scratch(SCR_RETINEX_PLANES, (size_t)chunk * a.ns * pb);
    double* d_tap_g = tap ? (double*)call.scratch(SCR_RETINEX_TAP, (size_t)chunk * (a.ns + 1) * pb) : nullptr;
    if (call.rc) return call.rc;
    double* d_tap_p = tap ? d_tap_g + (size_t)chunk * a.ns * npix : nullptr;
    const hipMemcpyKind tap_kind = is_device_ptr(tap) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    for (int f0 = 0; f0 < p->n_frames; f0 += chunk) {
        a.n = std::min(chunk, p->n_frames - f0);
        call.zero(d_rec, retinex_record_bytes(a.n));
        if (!call.launched(launch_retinex(d_src + (size_t)f0 * fb, d_dst + (size_t)f0 * fb, d_planes, d_rec, d_tap_g, d_tap_p, a, c->stream), 7)) return call.rc;
        for (int f = 0; tap && f < a.n; ++f) {                   // per frame: the n_sigmas Gaussian planes, then the product plane; the next chunk reuses the slot
            double* t = tap + (size_t)(f0 + f) * (a.ns + 1) * npix;
            call.copy(t, d_tap_g + (size_t)f * a.ns * npix, a.ns * pb, tap_kind);
            call.copy(t + (size_t)a.ns * npix, d_tap_p + (size_t)f * npix, pb, tap_kind);
        }
    }
    return call.done();
}

// ---- HAVC_tweak: RGB24 -> YUV420P8 -> RGB24 with vs_tweak's steps in between, and HAVC_adjust_rgb as per-frame tables (tweak.hip) ----
static_assert(sizeof(havc_tweak_params) == 560, "havc_tweak_params layout");
static_assert(sizeof(havc_adjust_params) == 816, "havc_adjust_params layout");

int havc_tweak_weights(float* out32) {
    if (!out32) return HAVC_E_INVALID;
    TweakWeights t;
    tw_all_weights(t);
    memcpy(out32, &t, sizeof(t));
    return HAVC_OK;
}

static int tweak_size_check(havc_ctx* c, const char* what, int width, int height, int n_frames) {
    if (width < 2 || height < 2 || n_frames <= 0 || (width & 1) || (height & 1) || width > TW_MAX_SIDE || height > TW_MAX_SIDE)
        return fail(c, HAVC_E_INVALID, std::string(what) + ": bad clip size (YUV420 needs an even width and height; at most 4096 x 4096)");
    return HAVC_OK;
}

// Frames per forward / back launch pair: the planes of a chunk stay under 256 MiB, and a launch takes at most 65535 frames (grid z).
static int tweak_chunk_frames(int width, int height, int n_frames, int want) {
    const int64_t per_frame = (int64_t)width * height * 3 / 2;
    const int64_t cap = std::max<int64_t>(1, ((int64_t)256 << 20) / per_frame);
    int64_t k = want > 0 ? want : cap;
    k = std::min<int64_t>(std::min<int64_t>(k, 65535), n_frames);
    return (int)k;
}

int havc_rgb_to_yuv420(havc_ctx* c, const uint8_t* src, uint8_t* y, uint8_t* u, uint8_t* v, int width, int height, int n_frames) {
    if (!c || !src || !y || !u || !v) return fail(c, HAVC_E_INVALID, "rgb_to_yuv420: bad args");
    int rc = tweak_size_check(c, "rgb_to_yuv420", width, height, n_frames);
    if (rc) return rc;
    Call call(c, "rgb_to_yuv420");
    const size_t pb = (size_t)width * height, qb = pb / 4;
    const uint8_t* d_src = call.in(SCR_IN, src, (size_t)n_frames * pb * 3);
    Call::Pack planes(SCR_TWEAK_YUV);                                    // the host planes among y, u, v
    call.add(planes, y, n_frames * pb); call.add(planes, u, n_frames * qb); call.add(planes, v, n_frames * qb);
    call.reserve(planes);
    uint8_t *d_y = call.out(planes, y, n_frames * pb), *d_u = call.out(planes, u, n_frames * qb), *d_v = call.out(planes, v, n_frames * qb);
    if (call.rc) return call.rc;
    TweakFwdArgs a{};
    a.h = height; a.w = width;
    const int chunk = tweak_chunk_frames(width, height, n_frames, 0);
    for (int f0 = 0; f0 < n_frames; f0 += chunk) {
        a.n = std::min(chunk, n_frames - f0);
        const int e = launch_tweak_forward(d_src + (size_t)f0 * pb * 3, d_y + (size_t)f0 * pb, d_u + (size_t)f0 * qb, d_v + (size_t)f0 * qb, a, c->stream);
        if (!call.launched(e)) return call.rc;
    }
    return call.done();
}

int havc_yuv420_to_rgb(havc_ctx* c, const uint8_t* y, const uint8_t* u, const uint8_t* v, uint8_t* dst, int width, int height, int n_frames) {
    if (!c || !y || !u || !v || !dst) return fail(c, HAVC_E_INVALID, "yuv420_to_rgb: bad args");
    int rc = tweak_size_check(c, "yuv420_to_rgb", width, height, n_frames);
    if (rc) return rc;
    Call call(c, "yuv420_to_rgb");
    const size_t pb = (size_t)width * height, qb = pb / 4, cb = (size_t)n_frames * pb * 3;
    Call::Pack planes(SCR_TWEAK_YUV);                                    // the host planes among y, u, v
    call.add(planes, y, n_frames * pb); call.add(planes, u, n_frames * qb); call.add(planes, v, n_frames * qb);
    call.reserve(planes);
    const uint8_t *d_y = call.in(planes, y, n_frames * pb), *d_u = call.in(planes, u, n_frames * qb), *d_v = call.in(planes, v, n_frames * qb);
    uint8_t* d_dst = call.out(SCR_OUT, dst, cb);
    if (call.rc) return call.rc;
    TweakBackArgs a{};
    a.h = height; a.w = width;
    const int chunk = tweak_chunk_frames(width, height, n_frames, 0);
    for (int f0 = 0; f0 < n_frames; f0 += chunk) {
        a.n = std::min(chunk, n_frames - f0);
        const int e = launch_tweak_back(d_y + (size_t)f0 * pb, d_u + (size_t)f0 * qb, d_v + (size_t)f0 * qb, d_dst + (size_t)f0 * pb * 3, a, c->stream);
        if (!call.launched(e)) return call.rc;
    }
    return call.done();
}

// ---- convert_format_RGB24 / restore_format: a clip's own planes <-> RGB24 (vformat.hip) ----
static_assert(sizeof(havc_vformat) == 52, "havc_vformat layout");

static int vformat_check(havc_ctx* c, const char* what, const havc_vformat* f, bool to_rgb, VfArgs& a) {
    const std::string w(what);
    if (f->width < 1 || f->height < 1 || f->n_frames <= 0 || f->width > TW_MAX_SIDE || f->height > TW_MAX_SIDE)
        return fail(c, HAVC_E_INVALID, w + ": bad clip size (at most 4096 x 4096)");
    if (f->family != 0 && f->family != 1) return fail(c, HAVC_E_INVALID, w + ": family must be 0 (YUV) or 1 (GRAY)");
    if (f->family == 1 && !to_rgb) return fail(c, HAVC_E_INVALID, w + ": GRAY is not a destination (restore_format sends a GRAY original back as YUV420P8)");
    const bool sub_ok = f->family == 1 ? (f->sub_w == 0 && f->sub_h == 0) : ((f->sub_w == 1 && (f->sub_h == 0 || f->sub_h == 1)) || (f->sub_w == 0 && f->sub_h == 0));
    if (!sub_ok) return fail(c, HAVC_E_INVALID, w + ": (sub_w, sub_h) must be (1, 1), (1, 0) or (0, 0), and (0, 0) for GRAY");
    if ((f->sub_w && (f->width & 1)) || (f->sub_h && (f->height & 1))) return fail(c, HAVC_E_INVALID, w + ": subsampled chroma needs an even width (4:2:x) / height (4:2:0)");
    if (f->bits < 8 || f->bits > 16) return fail(c, HAVC_E_INVALID, w + ": bits must be 8..16");
    double kr, kb;
    if (f->family == 0 && !vf_matrix(f->matrix, kr, kb)) return fail(c, HAVC_E_INVALID, w + ": matrix must be 1 (709), 5 (470bg), 6 (170m) or 9 (2020ncl)");
    if ((f->full_range | 1) != 1 || (f->depth_full_range | 1) != 1 || (f->dither | 1) != 1)
        return fail(c, HAVC_E_INVALID, w + ": full_range, depth_full_range and dither must be 0 or 1");
    if (!to_rgb && f->depth_full_range) return fail(c, HAVC_E_INVALID, w + ": depth_full_range belongs to planes_to_rgb24 and must be 0 here");
    if (f->family == 1 && f->dither) return fail(c, HAVC_E_INVALID, w + ": GRAY -> RGB24 is not dithered (the reference asks for none)");
    if (f->chunk_frames < 0 || f->reserved != 0) return fail(c, HAVC_E_INVALID, w + ": chunk_frames must be >= 0 and reserved 0");
    a = VfArgs{};
    a.h = f->height; a.w = f->width; a.gray = f->family; a.sub_w = f->sub_w; a.sub_h = f->sub_h; a.bits = f->bits; a.matrix = f->family ? 1 : f->matrix;
    a.full_range = f->full_range; a.depth_full_range = f->depth_full_range; a.dither = f->dither;
    return HAVC_OK;
}

// Frames per launch: havc_yuv420_to_rgb's rule (tweak_chunk_frames), so the same clip goes through in the same number of launches.  The diffusing kernels
// are one block per frame (and plane): every launch pays a whole frame's latency, and a clip split in two takes twice as long.
static int vformat_chunk_frames(const havc_vformat* f) { return tweak_chunk_frames(f->width, f->height, f->n_frames, f->chunk_frames); }

int havc_planes_to_rgb24(havc_ctx* c, const void* y, const void* u, const void* v, uint8_t* dst, const havc_vformat* f) {
    if (!c || !y || !dst || !f || (f->family == 0 && (!u || !v))) return fail(c, HAVC_E_INVALID, "planes_to_rgb24: bad args");
    VfArgs a;
    int rc = vformat_check(c, "planes_to_rgb24", f, true, a);
    if (rc) return rc;
    Call call(c, "planes_to_rgb24");
    const bool yuv = f->family == 0;
    const size_t bps = f->bits > 8 ? 2 : 1, n = (size_t)f->n_frames, npix = (size_t)f->width * f->height;
    const size_t pb = npix * bps, qb = yuv ? (size_t)(f->width >> f->sub_w) * (f->height >> f->sub_h) * bps : 0;
    Call::Pack planes(SCR_TWEAK_YUV);                                    // the host planes among y, u, v
    call.add(planes, y, n * pb);
    if (yuv) { call.add(planes, u, n * qb); call.add(planes, v, n * qb); }
    call.reserve(planes);
    const uint8_t* d_y = call.in(planes, (const uint8_t*)y, n * pb);
    const uint8_t *d_u = yuv ? call.in(planes, (const uint8_t*)u, n * qb) : nullptr, *d_v = yuv ? call.in(planes, (const uint8_t*)v, n * qb) : nullptr;
    uint8_t* d_dst = call.out(SCR_OUT, dst, n * npix * 3);
    if (call.rc) return call.rc;
    const int chunk = vformat_chunk_frames(f);
    for (int f0 = 0; f0 < f->n_frames; f0 += chunk) {
        a.n = std::min(chunk, f->n_frames - f0);
        const int e = launch_vformat_to_rgb(d_y + (size_t)f0 * pb, yuv ? d_u + (size_t)f0 * qb : nullptr, yuv ? d_v + (size_t)f0 * qb : nullptr,
                                            d_dst + (size_t)f0 * npix * 3, a, c->stream);
        if (!call.launched(e)) return call.rc;
    }
    return call.done();
}

int havc_rgb24_to_planes(havc_ctx* c, const uint8_t* src, void* y, void* u, void* v, const havc_vformat* f) {
    if (!c || !src || !y || !u || !v || !f) return fail(c, HAVC_E_INVALID, "rgb24_to_planes: bad args");
    VfArgs a;
    int rc = vformat_check(c, "rgb24_to_planes", f, false, a);
    if (rc) return rc;
    Call call(c, "rgb24_to_planes");
    const size_t bps = f->bits > 8 ? 2 : 1, n = (size_t)f->n_frames, npix = (size_t)f->width * f->height;
    const size_t pb = npix * bps, qb = (size_t)(f->width >> f->sub_w) * (f->height >> f->sub_h) * bps;
    const uint8_t* d_src = call.in(SCR_IN, src, n * npix * 3);
    Call::Pack planes(SCR_TWEAK_YUV);                                    // the host planes among y, u, v
    call.add(planes, y, n * pb); call.add(planes, u, n * qb); call.add(planes, v, n * qb);
    call.reserve(planes);
    uint8_t *d_y = call.out(planes, (uint8_t*)y, n * pb), *d_u = call.out(planes, (uint8_t*)u, n * qb), *d_v = call.out(planes, (uint8_t*)v, n * qb);
    if (call.rc) return call.rc;
    const int chunk = vformat_chunk_frames(f);
    for (int f0 = 0; f0 < f->n_frames; f0 += chunk) {
        a.n = std::min(chunk, f->n_frames - f0);
        const int e = launch_vformat_from_rgb(d_src + (size_t)f0 * npix * 3, d_y + (size_t)f0 * pb, d_u + (size_t)f0 * qb, d_v + (size_t)f0 * qb, a, c->stream);
        if (!call.launched(e)) return call.rc;
    }
    return call.done();
}

int havc_tweak_clip(havc_ctx* c, const uint8_t* src, uint8_t* dst, const havc_tweak_params* p) {
    if (!c || !src || !dst || !p) return fail(c, HAVC_E_INVALID, "tweak_clip: bad args");
    int rc = tweak_size_check(c, "tweak_clip", p->width, p->height, p->n_frames);
    if (rc) return rc;
    if (p->chunk_frames < 0) return fail(c, HAVC_E_INVALID, "tweak_clip: chunk_frames must be >= 0");
    if (p->has_hue_sat && !(std::isfinite(p->hue_c) && std::isfinite(p->hue_s))) return fail(c, HAVC_E_INVALID, "tweak_clip: hue_c / hue_s must be finite");
    Call call(c, "tweak_clip");
    TweakFwdArgs fa{};
    fa.h = p->height; fa.w = p->width;
    fa.has_gamma = p->has_gamma != 0; fa.has_hue_sat = p->has_hue_sat != 0; fa.has_luma = p->has_luma != 0;
    fa.hue_c = (float)p->hue_c; fa.hue_s = (float)p->hue_s;
    memcpy(fa.gamma_lut, p->gamma_lut, 256);
    memcpy(fa.luma_lut, p->luma_lut, 256);
    TweakBackArgs ba{};
    ba.h = p->height; ba.w = p->width;
    const int chunk = tweak_chunk_frames(p->width, p->height, p->n_frames, p->chunk_frames);
    const size_t pb = (size_t)p->width * p->height, qb = pb / 4, fb = pb * 3, cb = (size_t)p->n_frames * fb;
    const uint8_t* d_src = call.in(SCR_IN, src, cb);
    uint8_t* d_dst = call.out(SCR_OUT, dst, cb);
    uint8_t* d_y = (uint8_t*)call.scratch(SCR_TWEAK_YUV, (size_t)chunk * (pb + 2 * qb));
    if (call.rc) return call.rc;
    uint8_t* d_u = d_y + (size_t)chunk * pb;
    uint8_t* d_v = d_u + (size_t)chunk * qb;
    for (int f0 = 0; f0 < p->n_frames; f0 += chunk) {
        fa.n = ba.n = std::min(chunk, p->n_frames - f0);
        int e = launch_tweak_forward(d_src + (size_t)f0 * fb, d_y, d_u, d_v, fa, c->stream);
        if (!e) e = launch_tweak_back(d_y, d_u, d_v, d_dst + (size_t)f0 * fb, ba, c->stream);
        if (!call.launched(e, 2)) return call.rc;
    }
    return call.done();
}

// ---- HAVC_stabilizer(stab=True): vs_chroma_stabilizer_ex + vs_reduce_flicker on a clip, chunk by chunk (chroma_stab.hip, tweak.hip) ----
static_assert(sizeof(havc_chroma_stab_params) == 136, "havc_chroma_stab_params layout");

int havc_chroma_stab_frame_params(int64_t sum_y, int64_t gray_count, int64_t n_pixels, double weight, double tht_scen, double* out) {
    if (sum_y < 0 || gray_count < 0 || n_pixels <= 0 || gray_count > n_pixels || !out || !std::isfinite(weight) || !std::isfinite(tht_scen)) return HAVC_E_INVALID;
    double eff;
    const bool gate = cs_frame_decision((unsigned long long)sum_y, (unsigned long long)gray_count, n_pixels, weight, tht_scen, eff);
    out[0] = eff;
    out[1] = gate ? 1.0 : 0.0;
    return HAVC_OK;
}

// Frames a chunk stabilises (its output frames plus, with flicker, two on either side).  The shifted clips of a chunk stay under 512 MiB (at 256 MiB a 64-frame clip at 384 x 384 with N = 15 went through in two chunks, and each chunk pays the
// back kernel's latency again -- it is one block per frame: 5.67 ms a call against one chunk's figure in profiles/chroma_stab.txt); a chunk's source
// window (those frames and (N - 1) / 2 on either side) holds at most CS_MAX_WINDOW frames, and its N - 1 shifted clips at most 65535 frames (one launch).
static int chroma_stab_span(const havc_chroma_stab_params* p, int halo) {
    const int64_t fb = (int64_t)p->width * p->height * 3;
    const int64_t by_bytes = std::max<int64_t>(1, ((int64_t)512 << 20) / ((int64_t)(p->n_weights - 1) * fb));
    int64_t span = std::min<int64_t>(by_bytes, CS_MAX_WINDOW - (p->n_weights - 1));
    span = std::min<int64_t>(span, 65535 / (p->n_weights - 1));
    if (p->chunk_frames > 0) span = std::min<int64_t>(span, (int64_t)p->chunk_frames + 2 * halo);
    return (int)std::max<int64_t>(span, 2 * halo + 1);
}

int havc_chroma_stab_clip(havc_ctx* c, const uint8_t* src, uint8_t* dst, const havc_chroma_stab_params* p) {
    if (!c || !src || !dst || !p) return fail(c, HAVC_E_INVALID, "chroma_stab_clip: bad args");
    if (src == dst) return fail(c, HAVC_E_INVALID, "chroma_stab_clip: dst must not be src (every output frame reads its neighbours)");
    int rc = tweak_size_check(c, "chroma_stab_clip", p->width, p->height, p->n_frames);
    if (rc) return rc;
    if (p->n_weights < 3 || p->n_weights > CS_MAX_WEIGHTS || !(p->n_weights & 1)) return fail(c, HAVC_E_INVALID, "chroma_stab_clip: n_weights must be odd and 3..15");
    for (int k = 0; k < p->n_weights; ++k)
        if (p->weights[k] < -1000 || p->weights[k] > 1000) return fail(c, HAVC_E_INVALID, "chroma_stab_clip: a weight is outside -1000..1000");
    if (p->first_frame < 0 || p->chunk_frames < 0) return fail(c, HAVC_E_INVALID, "chroma_stab_clip: first_frame and chunk_frames must be >= 0");
    if (p->tht < 0 || p->tht > 256 || !(std::isfinite(p->sat) && std::isfinite(p->weight) && std::isfinite(p->tht_scen)))
        return fail(c, HAVC_E_INVALID, "chroma_stab_clip: tht must be 0..256, sat / weight / tht_scen finite");
    if ((p->scene_prev && is_device_ptr(p->scene_prev)) || (p->scene_next && is_device_ptr(p->scene_next)))
        return fail(c, HAVC_E_INVALID, "chroma_stab_clip: the scene-change arrays are host memory");
    Call call(c, "chroma_stab_clip");
    const int n = p->n_frames, N = p->n_weights, nh = (N - 1) / 2, halo = p->flicker ? 2 : 0, last = n - 1;
    const bool restore = p->tht > 0;
    const int span = chroma_stab_span(p, halo), core = span - 2 * halo;
    const size_t pb = (size_t)p->width * p->height, qb = pb / 4, fb = pb * 3, cb = (size_t)n * fb;
    const size_t S_max = (size_t)std::min(span, n), A_max = std::min<size_t>(S_max + 2 * nh, (size_t)n), P_max = restore ? S_max * (N - 1) : 0;
    // the chunk's workspace, one allocation: Y planes | U pool | V pool (source planes, then the restored clips') | averaged U, V | the shifted clips |
    // the stabilised frames in front of the flicker pass | tables | sums
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t off = 0;
    auto take = [&](size_t nb) { const size_t at = off; off += up(nb); return at; };
    const size_t o_y = take(A_max * pb), o_u = take((A_max + P_max) * qb), o_v = take((A_max + P_max) * qb), o_au = take(S_max * qb), o_av = take(S_max * qb);
    const size_t o_pairs = take(P_max * fb), o_t = take(p->flicker ? S_max * fb : 0), o_py = take(P_max * sizeof(int)), o_pc = take(P_max * sizeof(int));
    const size_t o_tab = take(S_max * N * sizeof(int)), o_mode = take(P_max), o_stats = take(P_max * 2 * sizeof(unsigned long long));
    const uint8_t* d_src = call.in(SCR_IN, src, cb);
    uint8_t* d_dst = call.out(SCR_OUT, dst, cb);
    uint8_t* ws = (uint8_t*)call.scratch(SCR_CHROMA_STAB, off);
    if (call.rc) return call.rc;
    uint8_t *d_y = ws + o_y, *d_u = ws + o_u, *d_v = ws + o_v, *d_au = ws + o_au, *d_av = ws + o_av, *d_pairs = ws + o_pairs, *d_t = ws + o_t, *d_mode = ws + o_mode;
    int *d_py = (int*)(ws + o_py), *d_pc = (int*)(ws + o_pc), *d_tab = (int*)(ws + o_tab);
    unsigned long long* d_stats = (unsigned long long*)(ws + o_stats);
    TweakFwdArgs fa{};
    fa.h = p->height; fa.w = p->width;
    TweakBackArgs ba{};
    ba.h = p->height; ba.w = p->width;
    StabAverageArgs aa{};
    aa.N = N; aa.plane_bytes = (int64_t)qb;
    for (int k = 0; k < N; ++k) aa.weights[k] = p->weights[k];
    for (int f0 = 0; f0 < n; f0 += core) {
        const int f1 = std::min(f0 + core, n), s0 = std::max(f0 - halo, 0), s1 = std::min(f1 + halo, n), S = s1 - s0;
        const int a0 = std::max(s0 - nh, 0), a1 = std::min(s1 + nh, n), A = a1 - a0, P = restore ? S * (N - 1) : 0;
        StabTableArgs ta{};
        ta.S = S; ta.s0 = s0; ta.A = A; ta.a0 = a0; ta.last = last; ta.first_frame = p->first_frame; ta.N = N; ta.restore = restore;
        for (int i = 0; i < A; ++i) {
            if (p->scene_prev && p->scene_prev[a0 + i]) ta.prev_bits[i >> 5] |= 1u << (i & 31);
            if (p->scene_next && p->scene_next[a0 + i]) ta.next_bits[i >> 5] |= 1u << (i & 31);
        }
        int e = launch_stab_tables(ta, d_py, d_pc, d_mode, d_tab, c->stream);
        fa.n = A;
        if (!e) e = launch_tweak_forward(d_src + (size_t)a0 * fb, d_y, d_u, d_v, fa, c->stream);
        c->stats.launches += 2;
        if (!e && restore) {
            ba.n = P;
            e = launch_tweak_back_indexed(d_y, d_u, d_v, d_pairs, d_py, d_pc, ba, c->stream);
            if (!e) e = (int)hipMemsetAsync(d_stats, 0, (size_t)P * 2 * sizeof(unsigned long long), c->stream);
            if (!e) e = launch_stab_stats(d_pairs, d_mode, d_stats, P, p->height, p->width, p->tht, c->stream);
            TweakRestoreArgs ra{};
            ra.color = d_src + (size_t)a0 * fb; ra.color_idx = d_py; ra.mode = d_mode; ra.stats = d_stats;
            ra.sat = p->sat; ra.weight = p->weight; ra.tht_scen = p->tht_scen; ra.tht = p->tht;
            fa.n = P;
            if (!e) e = launch_tweak_forward_restore(d_pairs, d_u + (size_t)A * qb, d_v + (size_t)A * qb, fa, ra, c->stream);
            c->stats.launches += 3;
        }
        aa.S = S;
        if (!e) e = launch_stab_average(d_u, d_v, d_au, d_av, d_tab, aa, c->stream);
        ba.n = S;
        if (!e) e = launch_tweak_back(d_y + (size_t)(s0 - a0) * pb, d_au, d_av, p->flicker ? d_t : d_dst + (size_t)s0 * fb, ba, c->stream);
        c->stats.launches += 2;
        if (!e && p->flicker) { e = launch_reduce_flicker(d_t, s0, d_dst + (size_t)f0 * fb, f0, f1 - f0, last, (int64_t)fb, c->stream); c->stats.launches++; }
        if (!call.launched(e, 0)) return call.rc;                        // (counted above, launch by launch)
    }
    return call.done();
}

int havc_reduce_flicker_clip(havc_ctx* c, const uint8_t* src, uint8_t* dst, int width, int height, int n_frames) {
    if (!c || !src || !dst || width <= 0 || height <= 0 || n_frames <= 0 || (int64_t)width * height > ((int64_t)1 << 30))
        return fail(c, HAVC_E_INVALID, "reduce_flicker_clip: bad args (at most 2^30 pixels per frame)");
    if (src == dst) return fail(c, HAVC_E_INVALID, "reduce_flicker_clip: dst must not be src (every output frame reads its neighbours)");
    Call call(c, "reduce_flicker_clip");
    const size_t fb = (size_t)width * height * 3, cb = (size_t)n_frames * fb;
    const uint8_t* d_src = call.in(SCR_IN, src, cb);
    uint8_t* d_dst = call.out(SCR_OUT, dst, cb);
    if (call.rc) return call.rc;
    for (int f0 = 0; f0 < n_frames; f0 += 65535) {
        const int e = launch_reduce_flicker(d_src, 0, d_dst + (size_t)f0 * fb, f0, std::min(65535, n_frames - f0), n_frames - 1, (int64_t)fb, c->stream);
        if (!call.launched(e)) return call.rc;
    }
    return call.done();
}

int havc_adjust_frame_params(const int64_t* chan_sums, int64_t n_pixels, double* out3) {
    if (!chan_sums || !out3 || n_pixels <= 0 || chan_sums[0] < 0 || chan_sums[1] < 0 || chan_sums[2] < 0) return HAVC_E_INVALID;
    const unsigned long long ch[3] = {(unsigned long long)chan_sums[0], (unsigned long long)chan_sums[1], (unsigned long long)chan_sums[2]};
    tw_normalize_gains(ch, n_pixels, out3);
    return HAVC_OK;
}

int havc_adjust_rgb_clip(havc_ctx* c, const uint8_t* src, uint8_t* dst, const havc_adjust_params* p) {
    if (!c || !src || !dst || !p) return fail(c, HAVC_E_INVALID, "adjust_rgb_clip: bad args");
    if (src == dst) return fail(c, HAVC_E_INVALID, "adjust_rgb_clip: dst must not be src");
    if (p->n_frames <= 0 || p->width <= 0 || p->height <= 0 || (int64_t)p->width * p->height > ((int64_t)1 << 30))
        return fail(c, HAVC_E_INVALID, "adjust_rgb_clip: bad clip size (at most 2^30 pixels per frame)");
    if (p->normalize < 0 || p->normalize > 2) return fail(c, HAVC_E_INVALID, "adjust_rgb_clip: normalize must be 0..2");
    if (p->normalize == 2 && !(p->strength > 0.0 && p->strength < 1.0)) return fail(c, HAVC_E_INVALID, "adjust_rgb_clip: strength must be in (0, 1) with normalize 2");
    for (int k = 0; k < 3; ++k)
        if (!(std::isfinite(p->gain[k]) && std::isfinite(p->bias[k]))) return fail(c, HAVC_E_INVALID, "adjust_rgb_clip: gain / bias must be finite");
    Call call(c, "adjust_rgb_clip");
    AdjustArgs a{};
    a.n = p->n_frames; a.h = p->height; a.w = p->width; a.mode = p->normalize;
    a.w15 = p->normalize == 2 ? eq_w15(p->strength) : 0;
    for (int k = 0; k < 3; ++k) { a.gain[k] = p->gain[k]; a.bias[k] = p->bias[k]; }
    memcpy(a.gamma_lut, p->gamma_lut, sizeof(a.gamma_lut));
    const size_t cb = (size_t)a.n * a.h * a.w * 3, rb = (size_t)a.n * sizeof(EqFrameRec), tb = (size_t)a.n * 3 * 256;
    const uint8_t* d_src = call.in(SCR_IN, src, cb);
    uint8_t* d_dst = call.out(SCR_OUT, dst, cb);
    uint8_t* d_sums = (uint8_t*)call.scratch(SCR_ADJUST_TABLES, rb + tb);           // the channel sums, then the tables
    if (call.rc) return call.rc;
    call.zero(d_sums, rb);
    call.launched(launch_adjust_rgb(d_src, d_dst, d_sums, d_sums + rb, a, c->stream), a.mode ? 3 : 2);
    return call.done();
}

int havc_luma_lut(havc_ctx* c, const uint8_t* img, const uint8_t* lut256, uint8_t* out, int width, int height) {
    if (!c || !img || !lut256 || !out || width <= 0 || height <= 0) return fail(c, HAVC_E_INVALID, "luma_lut: bad args");
    Call call(c, "luma_lut");
    const size_t nb = (size_t)width * height * 3;
    uint8_t* d_lut = (uint8_t*)call.scratch(SCR_SMALL, 256);
    call.copy(d_lut, lut256, 256, hipMemcpyDefault);                     // (the table may be host or device memory)
    const uint8_t* din = call.in(SCR_IN, img, nb);
    uint8_t* dout = call.out(SCR_OUT, out, nb);
    if (call.rc) return call.rc;
    call.launched(launch_luma_lut(din, d_lut, dout, (int64_t)width * height, c->stream));
    return call.done();
}

int havc_restore_color_gradient(havc_ctx* c, const uint8_t* img_color, const uint8_t* img_gray, uint8_t* out, int width, int height, double sat,
                                int tht, double weight, double alpha, int algo, int return_mask) {
    if (!c || !img_color || !img_gray || !out || width <= 0 || height <= 0 || algo < 0 || algo > 2)
        return fail(c, HAVC_E_INVALID, "restore_color_gradient: bad args (algo 0..2)");
    return run_filter(c, img_color, img_gray, out, (size_t)width * height * 3, "restore_color_gradient", [&](const uint8_t* da, const uint8_t* db, uint8_t* dout) {
        return launch_restore_color_gradient(da, db, dout, (int64_t)width * height, sat, tht, alpha, weight, algo, return_mask, c->stream); });
}

// ---- HAVC_recover_clip_color: ChromaRetentionMerge's selectors on a clip (recover.hip) ----
static_assert(sizeof(havc_recover_params) == 56, "havc_recover_params layout");

int havc_recover_color_clip(havc_ctx* c, const uint8_t* gray, const uint8_t* color, uint8_t* out, const havc_recover_params* p) {
    if (!c || !gray || !color || !out || !p) return fail(c, HAVC_E_INVALID, "recover_color_clip: bad args");
    if (p->n_frames < 1 || p->width <= 0 || p->height <= 0 || (int64_t)p->width * p->height > ((int64_t)1 << 31))
        return fail(c, HAVC_E_INVALID, "recover_color_clip: bad clip size (at most 2^31 pixels per frame)");
    if (p->algo < 0 || p->algo > 2) return fail(c, HAVC_E_INVALID, "recover_color_clip: algo must be 0..2");
    if (p->first_frame < 0) return fail(c, HAVC_E_INVALID, "recover_color_clip: first_frame must be >= 0");
    const size_t cb = (size_t)p->n_frames * p->height * p->width * 3;
    auto overlaps = [&](const uint8_t* q) { return (uintptr_t)out < (uintptr_t)q + cb && (uintptr_t)q < (uintptr_t)out + cb; };
    if (overlaps(gray) || overlaps(color)) return fail(c, HAVC_E_INVALID, "recover_color_clip: out must not alias an input");
    Call call(c, "recover_color_clip");
    RecoverArgs a{};
    a.n = p->n_frames; a.h = p->height; a.w = p->width; a.first_frame = p->first_frame;
    a.sat = p->sat; a.weight = p->weight; a.alpha = p->alpha; a.tht = p->tht; a.algo = p->algo;
    a.binary_mask = p->binary_mask != 0; a.return_mask = p->return_mask != 0;
    const uint8_t *d_gray = call.in(SCR_IN, gray, cb), *d_color = call.in(SCR_IN2, color, cb);
    uint8_t* d_out = call.out(SCR_OUT, out, cb);
    unsigned long long* d_sums = (unsigned long long*)call.scratch(SCR_SMALL, (size_t)a.n * sizeof(unsigned long long));
    if (call.rc) return call.rc;
    call.launched(launch_recover_color(d_gray, d_color, d_out, d_sums, a, c->stream), 2);
    return call.done();
}

int havc_color_temporal_stabilizer(havc_ctx* c, const uint8_t* const* frames, const double* weights, int n, uint8_t* out, int width, int height) {
    if (!c || !frames || !weights || !out || n < 1 || n > 9 || width <= 0 || height <= 0) return fail(c, HAVC_E_INVALID, "color_temporal_stabilizer: bad args (1..9 frames)");
    Call call(c, "color_temporal_stabilizer");
    const size_t nb = (size_t)width * height * 3;
    Call::Pack host_frames(SCR_IN);
    for (int k = 0; k < n; ++k) {
        if (!frames[k]) return fail(c, HAVC_E_INVALID, "color_temporal_stabilizer: NULL frame");
        call.add(host_frames, frames[k], nb);
    }
    call.reserve(host_frames);
    uint8_t* dout = call.out(SCR_OUT, out, nb);
    const uint8_t* d_frames[9];
    for (int k = 0; k < n; ++k) d_frames[k] = call.in(host_frames, frames[k], nb);
    if (call.rc) return call.rc;
    call.launched(launch_color_temporal_stabilizer(d_frames, weights, n, dout, (int64_t)width * height, c->stream));
    return call.done();
}

// ---- HAVC_TimeCube's 3D LUT on a clip (lut3d.hip) ----
static_assert(sizeof(havc_lut3d_params) == 16, "havc_lut3d_params layout");

int havc_lut3d_clip(havc_ctx* c, const uint8_t* src, uint8_t* dst, const float* table, const int32_t* idx, const float* frac, const havc_lut3d_params* p) {
    if (!c || !src || !dst || !table || !idx || !frac || !p) return fail(c, HAVC_E_INVALID, "lut3d_clip: bad args");
    if (src == dst) return fail(c, HAVC_E_INVALID, "lut3d_clip: dst must not be src");
    if (p->n_frames <= 0 || p->width <= 0 || p->height <= 0 || (int64_t)p->width * p->height > ((int64_t)1 << 30))
        return fail(c, HAVC_E_INVALID, "lut3d_clip: bad clip size (at most 2^30 pixels per frame)");
    if (p->size < LUT3D_MIN_SIZE || p->size > LUT3D_MAX_SIZE) return fail(c, HAVC_E_INVALID, "lut3d_clip: size must be 2..256");
    Call call(c, "lut3d_clip");
    Lut3dArgs a{};
    a.npix = (int64_t)p->n_frames * p->height * p->width; a.size = p->size;
    const size_t cb = (size_t)a.npix * 3, points = (size_t)a.size * a.size * a.size, pb = points * sizeof(Lut3dPoint), tb = points * 3 * sizeof(float);
    const size_t ab = 3 * 256 * sizeof(int32_t);
    const bool host_table = !is_device_ptr(table);
    const uint8_t* d_src = call.in(SCR_IN, src, cb);
    uint8_t* d_dst = call.out(SCR_OUT, dst, cb);
    uint8_t* d_points = (uint8_t*)call.scratch(SCR_LUT3D, pb + (host_table ? tb : 0));      // the points, then a host table on its way in
    uint8_t* d_axes = (uint8_t*)call.scratch(SCR_SMALL, 2 * ab);                            // idx, then frac
    if (call.rc) return call.rc;
    if (host_table) { call.copy(d_points + pb, table, tb, hipMemcpyHostToDevice); table = (const float*)(d_points + pb); }
    call.copy(d_axes, idx, ab, hipMemcpyDefault);                        // (the axis tables may be host or device memory)
    call.copy(d_axes + ab, frac, ab, hipMemcpyDefault);
    if (call.rc) return call.rc;
    call.launched(launch_lut3d(d_src, d_dst, table, d_points, (const int*)d_axes, (const float*)(d_axes + ab), a, c->stream), 2);
    return call.done();
}

// ---- HAVC_clip_overlay (overlay.hip) ----
static_assert(sizeof(havc_overlay_params) == 56, "havc_overlay_params layout");

int havc_overlay_clip(havc_ctx* c, const uint8_t* base, const uint8_t* overlay, const uint8_t* mask, uint8_t* dst, const havc_overlay_params* p) {
    if (!c || !base || !overlay || !dst || !p) return fail(c, HAVC_E_INVALID, "overlay_clip: bad args");
    if (dst == base || dst == overlay || dst == mask) return fail(c, HAVC_E_INVALID, "overlay_clip: dst must not be an input");
    const int64_t lim = (int64_t)1 << 30;
    if (p->n_frames <= 0 || p->base_w <= 0 || p->base_h <= 0 || p->ov_w <= 0 || p->ov_h <= 0 || (int64_t)p->base_w * p->base_h > lim || (int64_t)p->ov_w * p->ov_h > lim)
        return fail(c, HAVC_E_INVALID, "overlay_clip: bad clip size (at most 2^30 pixels per frame)");
    if (p->x <= -lim || p->x >= lim || p->y <= -lim || p->y >= lim) return fail(c, HAVC_E_INVALID, "overlay_clip: x and y must lie within +-2^30");
    if (p->mode < 0 || p->mode >= OV_MODES) return fail(c, HAVC_E_INVALID, "overlay_clip: mode must be 0..8");
    if (p->plane_mask < 0 || p->plane_mask > 7) return fail(c, HAVC_E_INVALID, "overlay_clip: plane_mask must be 0..7");
    if ((p->mask_planes != 0 && p->mask_planes != 1 && p->mask_planes != 3) || (p->mask_planes != 0) != (mask != nullptr))
        return fail(c, HAVC_E_INVALID, "overlay_clip: mask_planes must be 0 (and no mask), 1 or 3 (and a mask)");
    if (p->overlay_frames != 1 && p->overlay_frames != p->n_frames) return fail(c, HAVC_E_INVALID, "overlay_clip: overlay_frames must be 1 or n_frames");
    if (!(p->opacity >= 0.f && p->opacity <= 1.f)) return fail(c, HAVC_E_INVALID, "overlay_clip: opacity must be in [0, 1]");
    Call call(c, "overlay_clip");
    OverlayArgs a{};
    a.n = p->n_frames; a.bw = p->base_w; a.bh = p->base_h; a.ow = p->ov_w; a.oh = p->ov_h; a.x = p->x; a.y = p->y;
    a.mode = p->mode; a.plane_mask = p->plane_mask; a.mask_planes = p->mask_planes; a.first_plane = p->mask_first_plane != 0;
    a.overlay_frames = p->overlay_frames; a.opacity = p->opacity;
    const size_t bb = (size_t)a.n * a.bh * a.bw * 3, op = (size_t)a.overlay_frames * a.oh * a.ow;
    const uint8_t* d_base = call.in(SCR_IN, base, bb);
    const uint8_t* d_ov = call.in(SCR_IN2, overlay, op * 3);
    const uint8_t* d_mask = call.in(SCR_IN3, mask, op * (size_t)a.mask_planes);               // NULL without a mask
    uint8_t* d_dst = call.out(SCR_OUT, dst, bb);
    if (call.rc) return call.rc;
    call.launched(launch_overlay(d_base, d_ov, d_mask, d_dst, a, c->stream));
    return call.done();
}

// ---- per-pixel CIEDE2000 between two clips (metrics.hip) ----
static_assert(sizeof(DeRec) == sizeof(havc_de_rec) && sizeof(havc_de_rec) == 4144 && HAVC_DE_BINS == DE_BINS && DE_BINS == DE_HIST_BINS, "havc_de_rec layout");
static_assert(offsetof(DeRec, max_bits) == offsetof(havc_de_rec, max) && offsetof(DeRec, sse) == offsetof(havc_de_rec, sse) &&
              offsetof(DeRec, hist) == offsetof(havc_de_rec, hist), "havc_de_rec layout");

// the context's sRGB -> linear table: its own 2 KiB, allocated once; the copy has left the caller's memory when this returns
static void de_table_upload(Call& call, const double* host256) {
    havc_ctx* c = call.c;
    if (call.rc) return;
    if (!c->de_table) {
        SetupLock setup;
        if (!call.check(hipMalloc((void**)&c->de_table, 256 * sizeof(double)), "hipMalloc")) { c->de_table = nullptr; return; }
        c->stats.bytes_resident += 256 * sizeof(double);
    }
    call.copy(c->de_table, host256, 256 * sizeof(double), hipMemcpyHostToDevice);
    call.sync();
}

int havc_delta_e_set_table(havc_ctx* c, const double* srgb_to_linear256) {
    if (!c || !srgb_to_linear256) return fail(c, HAVC_E_INVALID, "delta_e_set_table: bad args");
    if (is_device_ptr(srgb_to_linear256)) return fail(c, HAVC_E_INVALID, "delta_e_set_table: the table is host memory");
    Call call(c, "delta_e_set_table");
    de_table_upload(call, srgb_to_linear256);
    return call.done();
}

int havc_delta_e_clip(havc_ctx* c, const uint8_t* a, const uint8_t* b, int width, int height, int n_frames, havc_de_rec* recs, double* map) {
    if (!c || !a || !b || !recs) return fail(c, HAVC_E_INVALID, "delta_e_clip: bad args");
    if (n_frames <= 0 || width <= 0 || height <= 0 || (int64_t)width * height > ((int64_t)1 << 30))
        return fail(c, HAVC_E_INVALID, "delta_e_clip: bad clip size (at most 2^30 pixels per frame)");
    Call call(c, "delta_e_clip");
    if (!c->de_table) {
        double lin[256];
        for (int v = 0; v < 256; ++v) lin[v] = de_srgb_linear(v);
        de_table_upload(call, lin);
    }
    const int64_t npix = (int64_t)width * height, nb = delta_e_blocks(npix);
    const size_t cb = (size_t)n_frames * npix * 3, rb = (size_t)n_frames * sizeof(DeRec), mb = (size_t)npix * sizeof(double);
    const bool host_map = map && !is_device_ptr(map);
    // frames per chunk: a launch takes at most 65535 (grid y), the partial sums stay inside their slot, a host map is staged in pieces under 256 MiB
    int64_t chunk = std::min<int64_t>(n_frames, 65535);
    chunk = std::min<int64_t>(chunk, (int64_t)(c->de_partials_limit / sizeof(double)) / nb);
    if (host_map) chunk = std::min<int64_t>(chunk, (int64_t)(((size_t)256 << 20) / mb));
    chunk = std::max<int64_t>(chunk, 1);
    const uint8_t* d_a = call.in(SCR_IN, a, cb);
    const uint8_t* d_b = call.in(SCR_IN2, b, cb);
    DeRec* d_rec = (DeRec*)call.out(SCR_SMALL, recs, rb);
    double* d_part = (double*)call.scratch(SCR_DE_PARTIALS, (size_t)chunk * nb * sizeof(double));
    double* d_map = host_map ? (double*)call.scratch(SCR_OUT, (size_t)chunk * mb) : map;
    if (call.rc) return call.rc;
    call.zero(d_rec, rb);
    for (int64_t f0 = 0; f0 < n_frames; f0 += chunk) {
        const int n = (int)std::min<int64_t>(chunk, n_frames - f0);
        double* m = !map ? nullptr : (host_map ? d_map : d_map + f0 * npix);
        if (!call.launched(launch_delta_e(d_a + f0 * npix * 3, d_b + f0 * npix * 3, c->de_table, d_rec + f0, d_part, m, n, npix, c->stream), 2)) break;
        if (host_map) call.copy(map + f0 * npix, d_map, (size_t)n * mb, hipMemcpyDeviceToHost);             // the next chunk reuses the slot
    }
    return call.done();
}

}  // extern "C"
