// libhavc_mi355.so runtime, resampling: the Spline64 / Spline36 and Pillow coefficient tables and their resize entry points.
#include "runtime_internal.h"

namespace {

// ---- Spline64 polyphase tables (Avisynth/zimg Spline64 kernel, support 4, widened when downscaling) ----
double spline64(double x) {
    x = std::fabs(x);
    if (x < 1.0) return ((49.0 / 41.0 * x - 6387.0 / 2911.0) * x - 3.0 / 2911.0) * x + 1.0;
    if (x < 2.0) { x -= 1.0; return ((-24.0 / 41.0 * x + 4032.0 / 2911.0) * x - 2328.0 / 2911.0) * x; }
    if (x < 3.0) { x -= 2.0; return ((6.0 / 41.0 * x - 1008.0 / 2911.0) * x + 582.0 / 2911.0) * x; }
    if (x < 4.0) { x -= 3.0; return ((-1.0 / 41.0 * x + 168.0 / 2911.0) * x - 97.0 / 2911.0) * x; }
    return 0.0;
}

// ---- Spline36 (Avisynth/zimg Spline36 kernel, support 3): the same polyphase tables with another kernel ----
double spline36(double x) {
    x = std::fabs(x);
    if (x < 1.0) return ((13.0 / 11.0 * x - 453.0 / 209.0) * x - 3.0 / 209.0) * x + 1.0;
    if (x < 2.0) { x -= 1.0; return ((-6.0 / 11.0 * x + 270.0 / 209.0) * x - 156.0 / 209.0) * x; }
    if (x < 3.0) { x -= 2.0; return ((1.0 / 11.0 * x - 45.0 / 209.0) * x + 26.0 / 209.0) * x; }
    return 0.0;
}

bool resize_filter_ok(int filter) { return filter == HAVC_RESIZE_SPLINE64 || filter == HAVC_RESIZE_SPLINE36; }
double resize_support(int filter) { return filter == HAVC_RESIZE_SPLINE36 ? 3.0 : 4.0; }

// kernel stretch for anti-aliasing when downscaling, and the taps per output of a src -> dst pass (the table below and havc_resize_plan)
double resize_fscale(int src, int dst) { const double scale = (double)dst / (double)src; return scale < 1.0 ? scale : 1.0; }
int resize_taps(int src, int dst, int filter) { return (int)std::ceil(2.0 * (resize_support(filter) / resize_fscale(src, dst))) + 1; }

int get_resize_table(havc_ctx* c, int src, int dst, int filter, ResizeTable** out) {
    auto key = std::make_tuple(src, dst, filter);
    auto it = c->resize_tables.find(key);
    if (it != c->resize_tables.end()) { *out = &it->second; return HAVC_OK; }
    const double scale = (double)dst / (double)src;
    const double fscale = resize_fscale(src, dst);
    const double support = resize_support(filter) / fscale;
    const int taps = resize_taps(src, dst, filter);
    std::vector<int> start(dst);
    std::vector<float> w((size_t)dst * taps);
    for (int i = 0; i < dst; ++i) {
        const double center = (i + 0.5) / scale - 0.5;
        const int s0 = (int)std::floor(center - support) + 1;
        double sum = 0;
        std::vector<double> tmp(taps);
        for (int t = 0; t < taps; ++t) { const double xk = (s0 + t - center) * fscale; tmp[t] = filter == HAVC_RESIZE_SPLINE36 ? spline36(xk) : spline64(xk); sum += tmp[t]; }
        for (int t = 0; t < taps; ++t) w[(size_t)i * taps + t] = (float)(tmp[t] / sum);
        start[i] = s0;
    }
    ResizeTable tb;
    tb.taps = taps;
    SetupLock setup;
    HIP_TRY(c, hipMalloc((void**)&tb.d_start, dst * sizeof(int)));
    HIP_TRY(c, hipMalloc((void**)&tb.d_w, w.size() * sizeof(float)));
    HIP_TRY(c, hipMemcpy(tb.d_start, start.data(), dst * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(tb.d_w, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
    auto res = c->resize_tables.emplace(key, tb);
    *out = &res.first->second;
    return HAVC_OK;
}

}  // namespace

int resize_rgb8(havc_ctx* c, const uint8_t* d_src, int sw, int sh, uint8_t* d_dst, int dw, int dh, int n,
                const uint8_t* d_orig, int filter) {
    ResizeTable *th, *tv;
    int rc = get_resize_table(c, sw, dw, filter, &th);
    if (rc) return rc;
    rc = get_resize_table(c, sh, dh, filter, &tv);
    if (rc) return rc;
    rc = ensure_scratch(c, SCR_RESIZE_ROWS, (size_t)n * sh * dw * 3 * sizeof(float));
    if (rc) return rc;
    int e = launch_resize_passes(d_src, sw, sh, d_dst, dw, dh, n, (float*)c->scratch[SCR_RESIZE_ROWS], th->d_start, th->d_w, th->taps,
                                 tv->d_start, tv->d_w, tv->taps, d_orig, c->stream);
    c->stats.launches += 2;
    if (e) return hip_fail(c, (hipError_t)e, "resize");
    return HAVC_OK;
}

namespace {

// ---- Pillow ImagingResample coefficient tables (libImaging/Resample.c precompute_coeffs + normalize_coeffs_8bpc) ----
struct PilTable { int ksize = 0; int* d_bounds = nullptr; int* d_kk = nullptr; };

double pil_filter(int resample, double x) {
    if (resample == 1) {                                                      // LANCZOS: lanczos_filter, a = 3, on [-3, 3) of the signed x
        auto sinc = [](double v) { if (v == 0.0) return 1.0; v *= M_PI; return std::sin(v) / v; };
        return (-3.0 <= x && x < 3.0) ? sinc(x) * sinc(x / 3.0) : 0.0;
    }
    if (x < 0.0) x = -x;
    if (resample == 2) return x < 1.0 ? 1.0 - x : 0.0;                       // BILINEAR
    const double a = -0.5;                                                    // BICUBIC
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

int build_pil_table(havc_ctx* c, int in_size, int out_size, int resample, PilTable* tb) {
    const double fsupport = resample == 2 ? 1.0 : (resample == 1 ? 3.0 : 2.0);
    const double scale = (double)in_size / (double)out_size;
    double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = fsupport * filterscale;
    const int ksize = (int)std::ceil(support) * 2 + 1;
    std::vector<int> bounds(out_size * 2), kk((size_t)out_size * ksize, 0);
    std::vector<double> w(ksize);
    const double ss = 1.0 / filterscale;
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) { w[x] = pil_filter(resample, (x + xmin - center + 0.5) * ss); ww += w[x]; }
        for (int x = 0; x < xmax; ++x) {
            const double v = ww != 0.0 ? w[x] / ww : w[x];
            kk[(size_t)xx * ksize + x] = v < 0 ? (int)(-0.5 + v * (double)(1 << 22)) : (int)(0.5 + v * (double)(1 << 22));
        }
        bounds[xx * 2] = xmin; bounds[xx * 2 + 1] = xmax;
    }
    tb->ksize = ksize;
    SetupLock setup;
    HIP_TRY(c, hipMalloc((void**)&tb->d_bounds, bounds.size() * sizeof(int)));
    HIP_TRY(c, hipMalloc((void**)&tb->d_kk, kk.size() * sizeof(int)));
    HIP_TRY(c, hipMemcpy(tb->d_bounds, bounds.data(), bounds.size() * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(tb->d_kk, kk.data(), kk.size() * sizeof(int), hipMemcpyHostToDevice));
    return HAVC_OK;
}

void free_pil_table(PilTable& t) { if (t.d_bounds) (void)hipFree(t.d_bounds); if (t.d_kk) (void)hipFree(t.d_kk); t = PilTable{}; }

}  // namespace

// Image.resize on device buffers; tmp must hold n*sh*dw*3 bytes
int pil_resize_dev(havc_ctx* c, const uint8_t* d_src, int sw, int sh, uint8_t* d_tmp, uint8_t* d_dst, int dw, int dh, int n, int resample) {
    PilTable th, tv;
    int rc = HAVC_OK;
    if (sw != dw && (rc = build_pil_table(c, sw, dw, resample, &th))) return rc;
    if (sh != dh && (rc = build_pil_table(c, sh, dh, resample, &tv))) { free_pil_table(th); return rc; }
    int e = launch_pil_resize_passes(d_src, sw, sh, d_tmp, d_dst, dw, dh, n, th.d_bounds, th.d_kk, th.ksize, tv.d_bounds, tv.d_kk,
                                     tv.ksize, c->stream);
    c->stats.launches += 2;
    hipError_t se = hipStreamSynchronize(c->stream);       // tables are freed right away (tiny, rebuilt per call)
    free_pil_table(th); free_pil_table(tv);
    if (e) return hip_fail(c, (hipError_t)e, "pil resize");
    if (se != hipSuccess) return hip_fail(c, se, "pil resize sync");
    return HAVC_OK;
}

extern "C" {

int havc_pil_resize(havc_ctx* c, const uint8_t* src, int sw, int sh, uint8_t* dst, int dw, int dh, int resample) {
    return havc_pil_resize_n(c, src, sw, sh, dst, dw, dh, resample, 1);
}

int havc_pil_resize_n(havc_ctx* c, const uint8_t* src, int sw, int sh, uint8_t* dst, int dw, int dh, int resample, int n_frames) {
    if (!c || !src || !dst || sw <= 0 || sh <= 0 || dw <= 0 || dh <= 0 || n_frames < 1 || (resample != 1 && resample != 2 && resample != 3))
        return fail(c, HAVC_E_INVALID, "pil_resize: bad args (resample must be 1 = LANCZOS, 2 = BILINEAR or 3 = BICUBIC)");
    Call call(c, "pil_resize");
    const size_t sb = (size_t)sw * sh * 3 * n_frames, tb = (size_t)sh * dw * 3 * n_frames, db = (size_t)dw * dh * 3 * n_frames;
    const uint8_t* d_src = call.in(SCR_IN, src, sb);
    uint8_t* d_rows = (uint8_t*)call.scratch(SCR_PIL_ROWS, tb);
    uint8_t* d_dst = call.out(SCR_OUT, dst, db);
    if (call.rc || (call.rc = pil_resize_dev(c, d_src, sw, sh, d_rows, d_dst, dw, dh, n_frames, resample))) return call.rc;   // (counts its own launches)
    return call.done();
}

int havc_resize_plan(int sw, int dw, int n_rows, int* h_taps, int* h_variant) {
    return havc_resize_plan_filter(sw, dw, n_rows, HAVC_RESIZE_SPLINE64, h_taps, h_variant);
}

int havc_resize_plan_filter(int sw, int dw, int n_rows, int filter, int* h_taps, int* h_variant) {
    if (sw <= 0 || dw <= 0 || n_rows <= 0 || !resize_filter_ok(filter)) return HAVC_E_INVALID;
    const int taps = resize_taps(sw, dw, filter);
    int span_lds = 0;
    const int variant = resize_h_variant(sw, dw, taps, n_rows, &span_lds);
    if (h_taps) *h_taps = taps;
    if (h_variant) *h_variant = variant;
    return span_lds;
}

int havc_spline64_resize(havc_ctx* c, const uint8_t* src, int sw, int sh, uint8_t* dst, int dw, int dh, const uint8_t* luma_from) {
    return havc_spline64_resize_n(c, src, sw, sh, dst, dw, dh, luma_from, 1);
}

int havc_spline64_resize_n(havc_ctx* c, const uint8_t* src, int sw, int sh, uint8_t* dst, int dw, int dh, const uint8_t* luma_from, int n_frames) {
    return havc_resize_n(c, src, sw, sh, dst, dw, dh, luma_from, n_frames, HAVC_RESIZE_SPLINE64);
}

int havc_resize_n(havc_ctx* c, const uint8_t* src, int sw, int sh, uint8_t* dst, int dw, int dh, const uint8_t* luma_from, int n_frames, int filter) {
    if (!c || !src || !dst || sw <= 0 || sh <= 0 || dw <= 0 || dh <= 0 || n_frames < 1) return fail(c, HAVC_E_INVALID, "resize_n: bad args");
    if (!resize_filter_ok(filter)) return fail(c, HAVC_E_INVALID, "resize: filter must be 0 = Spline64 or 1 = Spline36");
    Call call(c, "resize_n");
    const size_t sb = (size_t)sw * sh * 3 * n_frames, db = (size_t)dw * dh * 3 * n_frames;
    const uint8_t* d_src = call.in(SCR_IN, src, sb);
    uint8_t* d_dst = call.out(SCR_OUT, dst, db);
    const uint8_t* d_luma = call.in(SCR_IN3, luma_from, db);             // optional: NULL stays NULL
    if (call.rc) return call.rc;
    if (sw == dw && sh == dh && !luma_from) call.copy(d_dst, d_src, sb, hipMemcpyDeviceToDevice);
    else if ((call.rc = resize_rgb8(c, d_src, sw, sh, d_dst, dw, dh, n_frames, d_luma, filter))) return call.rc;   // (counts its own launches, sizes SCR_RESIZE_ROWS itself)
    return call.done();
}

}  // extern "C"
