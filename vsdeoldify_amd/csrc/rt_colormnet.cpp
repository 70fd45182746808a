// libhavc_mi355.so runtime, ColorMNet: memory reads, local correlation / attention, Lab transforms, the fast per-frame step and its side-stream protocol.
#include "runtime_internal.h"

extern "C" {

// ---- ColorMNet memory kernels.  fp32 operands in the reference's layouts, host or device pointers. ----
int havc_memory_read_topk(havc_ctx* c, const float* mk, const float* ms, const float* qk, const float* qe, const float* mv, float* out, int B, int CK,
                          int CV, int N, int HW, int top_k) {
    return havc_memory_read_topk_usage(c, mk, ms, qk, qe, mv, out, nullptr, B, CK, CV, N, HW, top_k);
}

int havc_memory_read_topk_usage(havc_ctx* c, const float* mk, const float* ms, const float* qk, const float* qe, const float* mv, float* out,
                                float* usage, int B, int CK, int CV, int N, int HW, int top_k) {
    if (!c || !mk || !qk || !mv || !out || B < 1 || CK < 1 || CV < 1 || N < 1 || HW < 1 || top_k < 1 || top_k > 64)
        return fail(c, HAVC_E_INVALID, "memory_read_topk: bad args (top_k 1..64)");
    Call call(c, "memory_read_topk");
    const size_t fmk = (size_t)B * CK * N * 4, fq = (size_t)B * CK * HW * 4, fms = (size_t)B * N * 4, fmv = (size_t)B * CV * N * 4, fo = (size_t)B * CV * HW * 4;
    const float *d_mk = call.in(SCR_IN, mk, fmk), *d_qk = call.in(SCR_IN2, qk, fq), *d_mv = call.in(SCR_IN3, mv, fmv);
    const float *d_ms = call.in(SCR_IN4, ms, fms), *d_qe = call.in(SCR_IN5, qe, fq);                        // optional: NULL stays NULL
    float* d_out = call.out(SCR_OUT, out, fo);
    // SCR_TOPK_IDX / SCR_TOPK_W also hold the level-1 survivors of the two-level top-k behind the final lists: [B][k][HW] + [B][S][k][HW]
    const size_t lst = (size_t)B * top_k * HW, cand = lst * (mem_topk_splits(N) > 1 ? mem_topk_splits(N) : 0);
    float* d_sim = (float*)call.scratch(SCR_SIM, (size_t)B * N * HW * 4);
    int* d_idx = (int*)call.scratch(SCR_TOPK_IDX, (lst + cand) * 4);
    float* d_w = (float*)call.scratch(SCR_TOPK_W, (lst + cand) * 4);
    unsigned long long* d_acc = usage ? (unsigned long long*)call.scratch(SCR_USAGE_ACC, (size_t)B * N * 8) : nullptr;
    float* d_us = call.out(SCR_SMALL, usage, (size_t)B * N * 4);
    if (call.rc) return call.rc;
    // wave-per-query selection on a query-major similarity; beyond 16 384 memory elements the two-level kernels
    int e;
    if (mem_topk_select_supported(N)) {
        e = launch_mem_similarity_t(d_mk, d_ms, d_qk, d_qe, d_sim, B, CK, N, HW, c->stream);
        if (!e) e = launch_mem_topk_select_readout(d_sim, d_mv, d_idx, d_w, d_out, B, CV, N, HW, top_k, c->stream);
    } else {
        e = launch_mem_similarity(d_mk, d_ms, d_qk, d_qe, d_sim, B, CK, N, HW, c->stream);
        if (!e) e = launch_mem_topk_readout(d_sim, d_mv, d_idx, d_w, d_w + lst, d_idx + lst, d_out, B, CV, N, HW, top_k, c->stream);
    }
    if (!call.launched(e, 3)) return call.rc;
    if (usage) call.launched(launch_mem_usage(d_idx, d_w, d_acc, d_us, B, N, HW, top_k, c->stream), 2);   // row sums of the sparse affinity (do_softmax(..., return_usage=True))
    return call.done();
}

int havc_memory_dense_readout(havc_ctx* c, const float* mk, const float* ms, const float* qk, const float* qe, const float* mv, float* out, int B, int CK,
                              int CV, int N, int P) {
    if (!c || !mk || !qk || !mv || !out || B < 1 || CK < 1 || CV < 1 || CV > 2048 || N < 1 || P < 1)
        return fail(c, HAVC_E_INVALID, "memory_dense_readout: bad args (CV <= 2048)");
    Call call(c, "memory_dense_readout");
    const size_t fmk = (size_t)B * CK * N * 4, fq = (size_t)B * CK * P * 4, fms = (size_t)B * N * 4, fmv = (size_t)B * CV * N * 4, fo = (size_t)B * CV * P * 4;
    const float *d_mk = call.in(SCR_IN, mk, fmk), *d_qk = call.in(SCR_IN2, qk, fq), *d_mv = call.in(SCR_IN3, mv, fmv);
    const float *d_ms = call.in(SCR_IN4, ms, fms), *d_qe = call.in(SCR_IN5, qe, fq);                        // optional: NULL stays NULL
    float* d_out = call.out(SCR_OUT, out, fo);
    float* d_sim = (float*)call.scratch(SCR_SIM, (size_t)B * N * P * 4);
    if (call.rc) return call.rc;
    int e = launch_mem_similarity(d_mk, d_ms, d_qk, d_qe, d_sim, B, CK, N, P, c->stream);
    if (!e) e = launch_mem_dense_readout(d_sim, d_mv, d_out, B, CV, N, P, c->stream);
    call.launched(e, 2);
    return call.done();
}

int havc_memory_similarity(havc_ctx* c, const float* mk, const float* ms, const float* qk, const float* qe, float* sim, int B, int CK, int N, int HW) {
    if (!c || !mk || !qk || !sim || B < 1 || CK < 1 || N < 1 || HW < 1) return fail(c, HAVC_E_INVALID, "memory_similarity: bad args");
    Call call(c, "memory_similarity");
    const size_t fmk = (size_t)B * CK * N * 4, fq = (size_t)B * CK * HW * 4, fms = (size_t)B * N * 4, fo = (size_t)B * N * HW * 4;
    const float *d_mk = call.in(SCR_IN, mk, fmk), *d_qk = call.in(SCR_IN2, qk, fq);
    const float *d_ms = call.in(SCR_IN4, ms, fms), *d_qe = call.in(SCR_IN5, qe, fq);                        // optional: NULL stays NULL
    float* d_out = call.out(SCR_OUT, sim, fo);
    if (call.rc) return call.rc;
    call.launched(launch_mem_similarity(d_mk, d_ms, d_qk, d_qe, d_out, B, CK, N, HW, c->stream));
    return call.done();
}

int havc_local_correlation(havc_ctx* c, const float* q, const float* k, float* out, int n, int C, int H, int W, int max_dis, int dilation, float q_scale) {
    if (!c || !q || !k || !out || n < 1 || C < 1 || H < 1 || W < 1 || max_dis < 0 || max_dis > 7 || dilation < 1)
        return fail(c, HAVC_E_INVALID, "local_correlation: bad args (max_dis 0..7, dilation >= 1)");
    Call call(c, "local_correlation");
    const int ws = 2 * max_dis + 1;
    const size_t fi = (size_t)n * C * H * W * 4, fo = (size_t)n * ws * ws * H * W * 4;
    const float *d_q = call.in(SCR_IN, q, fi), *d_k = call.in(SCR_IN2, k, fi);
    float* d_out = call.out(SCR_OUT, out, fo);
    if (call.rc) return call.rc;
    call.launched(launch_local_correlation(d_q, d_k, d_out, n, C, H, W, max_dis, dilation, q_scale, c->stream));
    return call.done();
}

int havc_local_attention(havc_ctx* c, const float* q, const float* k, const float* v, const float* rel_w, const float* rel_b, float* agg, float* attn,
                         int n, int C, int CV, int H, int W, int max_dis, int dilation) {
    if (!c || !q || !k || !v || !rel_w || !rel_b || !agg || n < 1 || C < 1 || CV < 1 || H < 1 || W < 1 || max_dis < 0 || max_dis > 7 || dilation < 1)
        return fail(c, HAVC_E_INVALID, "local_attention: bad args (max_dis 0..7, dilation >= 1)");
    Call call(c, "local_attention");
    const int ws = 2 * max_dis + 1, WW = ws * ws;
    const size_t fi = (size_t)n * C * H * W * 4, fv = (size_t)n * CV * H * W * 4, fa = (size_t)n * WW * H * W * 4, fo = (size_t)H * W * n * CV * 4;
    const float *d_q = call.in(SCR_IN, q, fi), *d_k = call.in(SCR_IN2, k, fi), *d_v = call.in(SCR_IN3, v, fv);
    const float *d_rw = call.in(SCR_IN4, rel_w, (size_t)WW * C * 4), *d_rb = call.in(SCR_IN5, rel_b, (size_t)WW * 4);
    float* d_agg = call.out(SCR_OUT, agg, fo);
    float* d_attn = attn ? call.out(SCR_SIM, attn, fa) : (float*)call.scratch(SCR_SIM, fa);                 // a result if asked for, a workspace anyway
    if (call.rc) return call.rc;
    // q / T with T = sqrt(d_att) = sqrt(C) (attention.py:742, 809); the relative embedding is taken from the UNSCALED q (:806)
    int e = launch_local_correlation(d_q, d_k, d_attn, n, C, H, W, max_dis, dilation, 1.0f / sqrtf((float)C), c->stream);
    if (!e) e = launch_local_softmax(d_attn, d_q, d_rw, d_rb, n, C, H, W, max_dis, dilation, c->stream);
    if (!e) e = launch_local_agg(d_attn, d_v, d_agg, n, CV, H, W, max_dis, dilation, c->stream);
    call.launched(e, 3);
    return call.done();
}

// ---- ColorMNetRender's frame transforms (colormnet_render.py:285-301, 276-279) ----
int havc_colormnet_rgb_to_lab(havc_ctx* c, const uint8_t* rgb, float* lab, int width, int height) {
    if (!c || !rgb || !lab || width < 1 || height < 1) return fail(c, HAVC_E_INVALID, "colormnet_rgb_to_lab: bad args");
    Call call(c, "colormnet_rgb_to_lab");
    const size_t npix = (size_t)width * height;
    const uint8_t* d_in = call.in(SCR_IN, rgb, npix * 3);
    float* d_out = call.out(SCR_OUT, lab, npix * 12);
    if (call.rc) return call.rc;
    call.launched(launch_cmn_rgb_to_lab(d_in, d_out, (int64_t)npix, c->stream));
    return call.done();
}

int havc_colormnet_lab_to_rgb(havc_ctx* c, const float* l_plane, const float* ab, uint8_t* rgb, int width, int height) {
    if (!c || !l_plane || !ab || !rgb || width < 1 || height < 1) return fail(c, HAVC_E_INVALID, "colormnet_lab_to_rgb: bad args");
    Call call(c, "colormnet_lab_to_rgb");
    const size_t npix = (size_t)width * height;
    const float *d_l = call.in(SCR_IN, l_plane, npix * 4), *d_ab = call.in(SCR_IN2, ab, npix * 8);
    uint8_t* d_out = call.out(SCR_OUT, rgb, npix * 3);
    if (call.rc) return call.rc;
    call.launched(launch_cmn_lab_to_rgb(d_l, d_ab, d_out, (int64_t)npix, c->stream));
    return call.done();
}

// ---- ColorMNet: the per-frame step without tensor bookkeeping between the kernels (include/havc_mi355.h, "fast step") -----------------------
int havc_cmn_frame_in(havc_ctx* c, const uint8_t* rgb, float* lab, float* img, int width, int height, int padded_w, int padded_h, int pad_left, int pad_top) {
    if (!c || !rgb || !lab || width < 1 || height < 1 || padded_w < width + pad_left || padded_h < height + pad_top || pad_left < 0 || pad_top < 0 ||
        is_device_ptr(lab) == false || (img && !is_device_ptr(img)))
        return fail(c, HAVC_E_INVALID, "cmn_frame_in: bad args (lab / img are device buffers)");
    Call call(c, "cmn_frame_in");
    const uint8_t* d_in = call.in(SCR_IN, rgb, (size_t)width * height * 3);
    if (call.rc) return call.rc;
    call.launched(launch_cmn_frame_in(d_in, lab, img, width, height, img ? padded_w : width, img ? padded_h : height, img ? pad_left : 0, img ? pad_top : 0, c->stream));
    return call.done();
}

int havc_cmn_frame_out(havc_ctx* c, const float* l_plane, const float* ab_padded, uint8_t* rgb, int width, int height, int padded_w, int padded_h,
                       int pad_left, int pad_top) {
    if (!c || !l_plane || !ab_padded || !rgb || width < 1 || height < 1 || padded_w < width + pad_left || padded_h < height + pad_top || pad_left < 0 || pad_top < 0 ||
        !is_device_ptr(l_plane) || !is_device_ptr(ab_padded))
        return fail(c, HAVC_E_INVALID, "cmn_frame_out: bad args (the Lab planes are device buffers)");
    Call call(c, "cmn_frame_out");
    uint8_t* d_out = call.out(SCR_OUT, rgb, (size_t)width * height * 3);
    if (call.rc) return call.rc;
    call.launched(launch_cmn_frame_out(l_plane, ab_padded, d_out, width, height, padded_w, padded_h, pad_left, pad_top, c->stream));
    return call.done();
}

// use_count += usage, life_count += 1 from the top-k lists in SCR_BANK_IDX / SCR_BANK_W.  The accumulators (SCR_BANK_ACC) are kept at zero BETWEEN reads by the
// update kernel itself; they are cleared here only when the buffer is new (first use, re-grown).
static int usage_update_locked(havc_ctx* c, float* use, float* life, int from, int N, int HW, int top_k, hipStream_t st) {
    if (c->acc_clean_sz != c->scratch_sz[SCR_BANK_ACC] || !c->acc_clean_sz) {
        hipError_t m = hipMemsetAsync(c->scratch[SCR_BANK_ACC], 0, c->scratch_sz[SCR_BANK_ACC], st);
        if (m != hipSuccess) return (int)m;
        c->acc_clean_sz = c->scratch_sz[SCR_BANK_ACC];
        c->stats.launches += 1;
    }
    c->stats.launches += 2;
    return launch_mem_usage_update((const int*)c->scratch[SCR_BANK_IDX], (const float*)c->scratch[SCR_BANK_W], (unsigned long long*)c->scratch[SCR_BANK_ACC], use, life, from, N, HW, top_k, st);
}

int havc_memory_read_banked(havc_ctx* c, const float* mk, const float* ms, const float* qk, const float* qe, const float* mv, float* out, float* use_count,
                            float* life_count, int usage_from, int CK, int CV, int N, int64_t pitch, int HW, int top_k) {
    if (!c || !mk || !qk || !mv || !out || CK < 1 || CV < 1 || N < 1 || HW < 1 || pitch < N || top_k < 1 || top_k > 64 || usage_from < 0 ||
        (use_count && !life_count))
        return fail(c, HAVC_E_INVALID, "memory_read_banked: bad args (top_k 1..64, pitch >= N)");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, hipSetDevice(c->dev));
    int rc;
    const size_t lst = (size_t)top_k * HW, cand = lst * (mem_topk_splits(N) > 1 ? mem_topk_splits(N) : 0);
    if ((rc = ensure_scratch(c, SCR_BANK_SIM, (size_t)N * HW * 4)) || (rc = ensure_scratch(c, SCR_BANK_IDX, (lst + cand) * 4)) || (rc = ensure_scratch(c, SCR_BANK_W, (lst + cand) * 4))) return rc;
    const hipStream_t st = c->side ? c->stream2 : c->stream;       // a read-ahead (havc_cmn_side_begin) runs next to the previous frame's decoder
    stream_jitter(st);
    int e;
    if (mem_topk_select_supported(N)) {
        e = launch_mem_similarity_t(mk, ms, qk, qe, (float*)c->scratch[SCR_BANK_SIM], 1, CK, N, HW, st, pitch);
        if (!e) e = launch_mem_topk_select_readout((const float*)c->scratch[SCR_BANK_SIM], mv, (int*)c->scratch[SCR_BANK_IDX], (float*)c->scratch[SCR_BANK_W], out, 1, CV, N, HW, top_k, st, pitch);
    } else {
        e = launch_mem_similarity(mk, ms, qk, qe, (float*)c->scratch[SCR_BANK_SIM], 1, CK, N, HW, st, pitch);
        if (!e) e = launch_mem_topk_readout((const float*)c->scratch[SCR_BANK_SIM], mv, (int*)c->scratch[SCR_BANK_IDX], (float*)c->scratch[SCR_BANK_W], (float*)c->scratch[SCR_BANK_W] + lst,
                                            (int*)c->scratch[SCR_BANK_IDX] + lst, out, 1, CV, N, HW, top_k, st, pitch);
    }
    c->stats.launches += 3;
    if (!e && use_count) {
        if ((rc = ensure_scratch(c, SCR_BANK_ACC, (size_t)N * 8))) return rc;
        if (c->side) {
            // a read that runs ahead must not touch the counters before its frame is really stepped (a caller may leave the announced order): the
            // top-k lists stay in SCR_BANK_IDX / SCR_BANK_W until the next read, havc_cmn_side_wait(apply = 1) launches the update from them on the main stream
            c->side_usage.use = use_count; c->side_usage.life = life_count; c->side_usage.from = usage_from;
            c->side_usage.N = N; c->side_usage.HW = HW; c->side_usage.top_k = top_k;
        } else {
            e = usage_update_locked(c, use_count, life_count, usage_from, N, HW, top_k, st);
        }
    }
    if (e) return hip_fail(c, (hipError_t)e, "memory_read_banked");
    return HAVC_OK;
}

int havc_memory_read_reserve(havc_ctx* c, int N_max, int HW, int top_k) {
    if (!c || N_max < 1 || HW < 1 || top_k < 1 || top_k > 64) return fail(c, HAVC_E_INVALID, "memory_read_reserve: bad args");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, hipSetDevice(c->dev));
    // the largest request havc_memory_read_banked can make for N <= N_max: the candidate lists of the two-level selection peak at the largest slice count
    size_t splits = 1;
    for (int n = 64; n <= N_max + 63; n += 64) splits = std::max(splits, (size_t)mem_topk_splits(std::min(n, N_max)));
    const size_t lst = (size_t)top_k * HW, cand = lst * (splits > 1 ? splits : 0);
    int rc;
    if ((rc = ensure_scratch(c, SCR_BANK_SIM, (size_t)N_max * HW * 4)) || (rc = ensure_scratch(c, SCR_BANK_IDX, (lst + cand) * 4)) || (rc = ensure_scratch(c, SCR_BANK_W, (lst + cand) * 4)) ||
        (rc = ensure_scratch(c, SCR_BANK_ACC, (size_t)N_max * 8)))
        return rc;
    return HAVC_OK;
}

int havc_cmn_short_term(havc_ctx* c, havc_net* net, int first_op, int n_ops, int agg_buf, int short_buf, const float* q, const float* k, const float* v,
                        const float* rel_w, const float* rel_b, float* agg, float* attn, float* short_out, int C, int CV, int H, int W, int max_dis) {
    if (!c || !net || net->ctx != c || !q || !k || !v || !rel_w || !rel_b || !agg || !attn || !short_out || C < 1 || CV < 1 || H < 1 || W < 1 || max_dis < 0 ||
        max_dis > 7 || agg_buf < 0 || agg_buf >= (int)net->bufs.size() || short_buf < 0 || short_buf >= (int)net->bufs.size())
        return fail(c, HAVC_E_INVALID, "cmn_short_term: bad args");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, hipSetDevice(c->dev));
    // fork: stream2 starts behind everything the main stream holds so far (the producers of q / k / v), runs the local attention and the plan's
    // `short` slice there, and records the join event havc_cmn_join_add waits for -- the main stream is free for the memory read meanwhile
    if (!c->side) {                                                // (a read-ahead is on stream2 from its first launch on)
        HIP_TRY(c, hipEventRecord(c->ev_fork, c->stream));
        HIP_TRY(c, hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
    }
    stream_jitter(c->stream2);
    int e = launch_local_correlation(q, k, attn, 1, C, H, W, max_dis, 1, 1.0f / sqrtf((float)C), c->stream2);
    if (!e) e = launch_local_softmax(attn, q, rel_w, rel_b, 1, C, H, W, max_dis, 1, c->stream2);
    if (!e) e = launch_local_agg(attn, v, agg, 1, CV, H, W, max_dis, 1, c->stream2);
    c->stats.launches += 3;
    if (e) { (void)hipStreamSynchronize(c->stream2); return hip_fail(c, (hipError_t)e, "cmn_short_term"); }
    if (net->bound.empty()) net->bound.assign(net->bufs.size(), nullptr);
    net->bound[agg_buf] = agg;
    net->bound[short_buf] = short_out;
    c->cur = c->stream2;
    int rc = run_ops_locked(net, first_op, n_ops, 1);
    c->cur = nullptr;
    if (rc) { (void)hipStreamSynchronize(c->stream2); return rc; }
    HIP_TRY(c, hipEventRecord(c->ev_join, c->stream2));
    return HAVC_OK;
}

int havc_cmn_join_add(havc_ctx* c, float* readout, const float* short_out, int64_t n) {
    if (!c || !readout || !short_out || n < 1) return fail(c, HAVC_E_INVALID, "cmn_join_add: bad args");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, hipSetDevice(c->dev));
    const hipStream_t st = c->side ? c->stream2 : c->stream;
    if (!c->side) HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
    stream_jitter(st);
    int e = launch_vec_add(readout, short_out, n, st);
    c->stats.launches++;
    if (e) return hip_fail(c, (hipError_t)e, "cmn_join_add");
    return HAVC_OK;
}

int havc_cmn_side_mark(havc_ctx* c) {
    if (!c) return HAVC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->side) return fail(c, HAVC_E_INVALID, "cmn_side_mark: inside a side section");
    HIP_TRY(c, hipSetDevice(c->dev));
    HIP_TRY(c, hipEventRecord(c->ev_mark, c->stream));             // everything the main stream holds NOW: the previous read, the banks, the look-ahead keys it waited for
    c->marked = true;
    return HAVC_OK;
}

int havc_cmn_side_begin(havc_ctx* c) {
    if (!c) return HAVC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->side) return fail(c, HAVC_E_INVALID, "cmn_side_begin: already inside a side section");
    if (c->side_usage.use) return fail(c, HAVC_E_INVALID, "cmn_side_begin: the previous section has not been waited for");
    HIP_TRY(c, hipSetDevice(c->dev));
    // behind the main stream's work up to the last havc_cmn_side_mark (what was enqueued after it -- this frame's decoder -- runs NEXT to the section), or,
    // without a mark, behind everything it holds
    if (!c->marked) HIP_TRY(c, hipEventRecord(c->ev_mark, c->stream));
    c->marked = false;
    HIP_TRY(c, hipStreamWaitEvent(c->stream2, c->ev_mark, 0));
    stream_jitter(c->stream2);
    c->side = true;
    return HAVC_OK;
}

int havc_cmn_side_end(havc_ctx* c) {
    if (!c) return HAVC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->side) return fail(c, HAVC_E_INVALID, "cmn_side_end: no side section open");
    c->side = false;
    HIP_TRY(c, hipSetDevice(c->dev));
    HIP_TRY(c, hipEventRecord(c->ev_side, c->stream2));
    return HAVC_OK;
}

int havc_cmn_side_wait(havc_ctx* c, int apply_usage) {
    if (!c) return HAVC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->side) return fail(c, HAVC_E_INVALID, "cmn_side_wait: inside a side section");
    HIP_TRY(c, hipSetDevice(c->dev));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_side, 0));
    stream_jitter(c->stream);
    auto u = c->side_usage;
    c->side_usage = {};
    if (apply_usage && u.use) {
        int e = usage_update_locked(c, u.use, u.life, u.from, u.N, u.HW, u.top_k, c->stream);
        if (e) return hip_fail(c, (hipError_t)e, "cmn_side_wait: usage update");
    }
    return HAVC_OK;
}

int havc_cmn_value_in(havc_ctx* c, const float* image, const float* planes, float* value_in, int64_t pixels) {
    if (!c || !image || !planes || !value_in || pixels < 1) return fail(c, HAVC_E_INVALID, "cmn_value_in: bad args");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, hipSetDevice(c->dev));
    int e = launch_cmn_value_in(image, planes, value_in, pixels, c->stream);
    c->stats.launches++;
    if (e) return hip_fail(c, (hipError_t)e, "cmn_value_in");
    return HAVC_OK;
}

}  // extern "C"
