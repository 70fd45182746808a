// libhavc_mi355.so runtime, model drivers: the DeOldify / Zhang / DDColor frame and clip entry points, the frame coalescer, planar <-> interleaved.
#include "runtime_internal.h"

#include <chrono>
#include <condition_variable>
#include <deque>

namespace {

// colour + blend tail at S x S for a batch already on the device.
// d_in: source frames; d_v / d_s: raw colour of the video / second model (d_s may be null); result -> d_out.
int deoldify_tail(havc_ctx* c, const uint8_t* d_in, uint8_t* d_v, uint8_t* d_s, float video_weight, int post_process,
                  uint8_t* d_out, int64_t npix) {
    int e;
    if (!d_s) {
        if (post_process) { e = launch_yuv_merge(d_v, d_in, d_out, npix, c->stream); c->stats.launches++; }
        else e = (int)hipMemcpyAsync(d_out, d_v, npix * 3, hipMemcpyDeviceToDevice, c->stream);
        if (e) return hip_fail(c, (hipError_t)e, "tail");
        return HAVC_OK;
    }
    if (post_process) {
        e = launch_yuv_merge(d_v, d_in, d_v, npix, c->stream);
        if (e) return hip_fail(c, (hipError_t)e, "yuv_merge");
        e = launch_yuv_merge(d_s, d_in, d_s, npix, c->stream);
        if (e) return hip_fail(c, (hipError_t)e, "yuv_merge");
        c->stats.launches += 2;
    }
    // Image.blend(img_second, img_video, video_weight)  (deoldify/visualize.py:129,135)
    e = launch_blend_u8(d_s, d_v, video_weight, d_out, npix * 3, c->stream);
    c->stats.launches++;
    if (e) return hip_fail(c, (hipError_t)e, "blend");
    return HAVC_OK;
}

// Two generators per frame (video + stable/artistic).  Their encoder / bottleneck / decoder-block phases fill well under
// 256 CUs at small batch, so those phases of the two networks run CONCURRENTLY on two streams; the GPU-filling tails
// (ops from the first one tagged 1 = the 560x560 res-block convs onward) then run one after the other, each alone:
//   stream : A.small ------------\  wait(B.small) -> A.tail -> record(A.done) ............ wait(B.done)
//   stream2: wait(fork) B.small --/--------------------------- wait(A.done) -> B.tail -> record(B.done)
int run_generators(havc_ctx* c, havc_net* video, havc_net* second, const uint8_t* d_in, uint8_t* d_v, uint8_t* d_s, int b) {
    int rc;
    if (!second) return net_run_rgb8_locked(video, d_in, d_v, b);
    const int ta = video->tail_first, tb = second->tail_first;
    if (!c->two_streams || ta < 0 || tb < 0) {
        if ((rc = net_run_rgb8_locked(video, d_in, d_v, b))) return rc;
        return net_run_rgb8_locked(second, d_in, d_s, b);
    }
    auto part = [&](havc_net* n, const uint8_t* in, uint8_t* out, int first, int count, hipStream_t on) {
        n->in_override = in; n->out_override = out; c->cur = on;
        int r = run_ops_locked(n, first, count, b);
        n->in_override = nullptr; n->out_override = nullptr; c->cur = nullptr;
        return r;
    };
    // After the fork stream2 holds kernels that use the caller's scratch and the second net's buffers: on ANY failure both
    // streams are drained before the error is returned, so a later realloc / free cannot race with queued work.
    auto body = [&]() -> int {
        HIP_TRY(c, hipEventRecord(c->ev_fork, c->stream));
        HIP_TRY(c, hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
        if ((rc = part(video, d_in, d_v, 0, ta, nullptr))) return rc;
        if ((rc = part(second, d_in, d_s, 0, tb, c->stream2))) return rc;
        HIP_TRY(c, hipEventRecord(c->ev_join, c->stream2));                        // B.small done
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
        if ((rc = part(video, d_in, d_v, ta, (int)video->ops.size() - ta, nullptr))) return rc;
        HIP_TRY(c, hipEventRecord(c->ev_main_done, c->stream));                    // A.tail done
        HIP_TRY(c, hipStreamWaitEvent(c->stream2, c->ev_main_done, 0));
        if ((rc = part(second, d_in, d_s, tb, (int)second->ops.size() - tb, c->stream2))) return rc;
        HIP_TRY(c, hipEventRecord(c->ev_join, c->stream2));                        // B.tail done
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
        return HAVC_OK;
    };
    if ((rc = body())) {
        const std::string keep = c->err;
        (void)sync_streams(c);
        (void)hipGetLastError();
        c->err = keep;
        return rc;
    }
    c->stats.total_flops += (video->flops_per_frame + second->flops_per_frame) * b;
    return HAVC_OK;
}

}  // namespace

extern "C" {

int havc_deoldify_frames(havc_ctx* c, havc_net* video, havc_net* second, float video_weight, int post_process,
                         const uint8_t* rgb_in, uint8_t* rgb_out, int n_frames) {
    if (!c || !video || !rgb_in || !rgb_out || n_frames < 0) return fail(c, HAVC_E_INVALID, "deoldify_frames: bad args");
    if (video->ctx != c || (second && (second->ctx != c || second->S != video->S))) return fail(c, HAVC_E_INVALID, "deoldify_frames: nets from another ctx / size");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, hipSetDevice(c->dev));
    const int S = video->S;
    const int64_t npix1 = (int64_t)S * S;
    int maxb = video->max_batch;
    if (second) maxb = std::min(maxb, second->max_batch);
    const size_t fb = (size_t)npix1 * 3;
    const bool in_dev = is_device_ptr(rgb_in), out_dev = is_device_ptr(rgb_out);
    int rc;
    for (int slot = SCR_IN; slot <= SCR_RESULT; ++slot) {                // SCR_IN, SCR_VIDEO, SCR_SECOND, SCR_RESULT
        if ((slot == SCR_IN && in_dev) || (slot == SCR_RESULT && out_dev)) continue;
        if ((rc = ensure_scratch(c, slot, fb * maxb))) return rc;
    }
    uint8_t *d_v = (uint8_t*)c->scratch[SCR_VIDEO], *d_s = (uint8_t*)c->scratch[SCR_SECOND];
    Timer t(c);
    for (int f0 = 0; f0 < n_frames; f0 += maxb) {
        const int b = std::min(maxb, n_frames - f0);
        const uint8_t* d_in = in_dev ? rgb_in + (size_t)f0 * fb : (const uint8_t*)c->scratch[SCR_IN];
        uint8_t* d_out = out_dev ? rgb_out + (size_t)f0 * fb : (uint8_t*)c->scratch[SCR_RESULT];
        if (!in_dev) HIP_TRY(c, hipMemcpyAsync(c->scratch[SCR_IN], rgb_in + (size_t)f0 * fb, fb * b, hipMemcpyHostToDevice, c->stream));
        if ((rc = run_generators(c, video, second, d_in, d_v, d_s, b))) return rc;
        if ((rc = deoldify_tail(c, d_in, d_v, second ? d_s : nullptr, video_weight, post_process, d_out, npix1 * b))) return rc;
        if (!out_dev) {
            HIP_TRY(c, hipMemcpyAsync(rgb_out + (size_t)f0 * fb, d_out, fb * b, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
    }
    c->stats.frames += n_frames;
    return out_dev ? HAVC_OK : t.finish();
}

// ---- frame coalescer: the reference calls get_transformed_image ONCE PER FRAME from several VapourSynth worker threads (vsmodels.py:201-230,
// one call per std.ModifyFrame selector).  A batch of one leaves the encoder at 5 blocks on 256 CUs; here concurrent callers are
// merged: the first caller to arrive leads, waits up to wait_us (or until `callers` requests are queued), runs ONE havc_deoldify_frames
// over everything queued and hands every caller its frame.  Bytes are those of a call of its own (all tile configurations and batch sizes
// produce the same result).  ----
struct havc_batcher {
    havc_ctx* ctx = nullptr;
    int kind = 0;                                              // 0 DeOldify (video [+ second]), 1 DDColor, 2 Zhang: `video` is the net
    int width = 0, height = 0;                                 // frame size (kinds 1, 2; kind 0: S x S)
    havc_net *video = nullptr, *second = nullptr;
    float video_weight = 0.f;
    int post_process = 1, S = 0, max_batch = 1, wait_us = 200, callers = 0;
    size_t fb = 0;
    struct Req { const uint8_t* in; uint8_t* out; int rc; bool done; };
    std::mutex m;
    std::condition_variable cv;
    std::deque<Req*> q;
    bool leader = false;
    int inflight = 0;                                          // callers inside havc_batcher_submit (free waits for them to LEAVE, not only for an empty queue)
    uint8_t *h_in = nullptr, *h_out = nullptr;                 // pinned [max_batch][S * S * 3]
    int64_t calls = 0, batches = 0;
};

int havc_batcher_create(havc_ctx* c, havc_net* video, havc_net* second, float video_weight, int post_process, int wait_us, int callers,
                        havc_batcher** out) {
    if (!c || !video || !out || video->ctx != c || (second && (second->ctx != c || second->S != video->S)))
        return fail(c, HAVC_E_INVALID, "batcher_create: bad args / nets of another ctx or size");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, hipSetDevice(c->dev));
    auto* b = new havc_batcher();
    b->ctx = c; b->video = video; b->second = second; b->video_weight = video_weight; b->post_process = post_process;
    b->S = video->S;
    b->max_batch = second ? std::min(video->max_batch, second->max_batch) : video->max_batch;
    b->wait_us = wait_us < 0 ? 0 : wait_us;
    b->callers = callers;
    b->fb = (size_t)b->S * b->S * 3;
    if (hipHostMalloc((void**)&b->h_in, b->fb * b->max_batch, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&b->h_out, b->fb * b->max_batch, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        if (b->h_in) (void)hipHostFree(b->h_in);
        delete b;
        return fail(c, HAVC_E_OOM, "batcher_create: pinned staging");
    }
    *out = b;
    return HAVC_OK;
}

int havc_batcher_create_frames(havc_ctx* c, int kind, havc_net* net, int width, int height, int wait_us, int callers, havc_batcher** out) {
    if (!c || !net || !out || net->ctx != c || (kind != 1 && kind != 2) || width <= 0 || height <= 0)
        return fail(c, HAVC_E_INVALID, "batcher_create_frames: kind 1 (DDColor) or 2 (Zhang), a net of this ctx, a frame size");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, hipSetDevice(c->dev));
    auto* b = new havc_batcher();
    b->ctx = c; b->kind = kind; b->video = net; b->width = width; b->height = height; b->S = net->S;
    b->max_batch = net->max_batch;
    b->wait_us = wait_us < 0 ? 0 : wait_us;
    b->callers = callers;
    b->fb = (size_t)width * height * 3;
    if (hipHostMalloc((void**)&b->h_in, b->fb * b->max_batch, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&b->h_out, b->fb * b->max_batch, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        if (b->h_in) (void)hipHostFree(b->h_in);
        delete b;
        return fail(c, HAVC_E_OOM, "batcher_create_frames: pinned staging");
    }
    *out = b;
    return HAVC_OK;
}

void havc_batcher_free(havc_batcher* b) {
    if (!b) return;
    {
        std::unique_lock<std::mutex> lk(b->m);
        // a follower woken by the leader still has to re-acquire b->m before it returns: wait until every submitter has left
        b->cv.wait(lk, [&] { return !b->leader && b->q.empty() && b->inflight == 0; });
    }
    (void)hipHostFree(b->h_in);
    (void)hipHostFree(b->h_out);
    delete b;
}

int havc_batcher_stats(havc_batcher* b, int64_t* calls, int64_t* batches) {
    if (!b) return HAVC_E_INVALID;
    std::lock_guard<std::mutex> lk(b->m);
    if (calls) *calls = b->calls;
    if (batches) *batches = b->batches;
    return HAVC_OK;
}

int havc_batcher_submit(havc_batcher* b, const uint8_t* rgb_in, uint8_t* rgb_out) {
    if (!b || !rgb_in || !rgb_out) return HAVC_E_INVALID;
    havc_batcher::Req r{rgb_in, rgb_out, HAVC_OK, false};
    std::unique_lock<std::mutex> lk(b->m);
    ++b->inflight;
    b->q.push_back(&r);
    ++b->calls;
    b->cv.notify_all();                                        // a leader collecting its batch re-checks the queue length
    while (!r.done) {
        if (b->leader) { b->cv.wait(lk); continue; }
        b->leader = true;
        const int want = b->callers > 0 ? std::min(b->callers, b->max_batch) : b->max_batch;
        const auto deadline = std::chrono::steady_clock::now() + std::chrono::microseconds(b->wait_us);
        while ((int)b->q.size() < want && b->cv.wait_until(lk, deadline) != std::cv_status::timeout) {}
        std::vector<havc_batcher::Req*> batch;
        while (!b->q.empty() && (int)batch.size() < b->max_batch) { batch.push_back(b->q.front()); b->q.pop_front(); }
        lk.unlock();
        const int n = (int)batch.size();
        for (int i = 0; i < n; ++i) memcpy(b->h_in + (size_t)i * b->fb, batch[i]->in, b->fb);
        const int rc = b->kind == 0   ? havc_deoldify_frames(b->ctx, b->video, b->second, b->video_weight, b->post_process, b->h_in, b->h_out, n)
                       : b->kind == 1 ? havc_ddcolor_frames(b->ctx, b->video, b->h_in, b->h_out, n, b->width, b->height)
                                      : havc_zhang_frames(b->ctx, b->video, b->h_in, b->h_out, n, b->width, b->height);
        if (rc == HAVC_OK)
            for (int i = 0; i < n; ++i) memcpy(batch[i]->out, b->h_out + (size_t)i * b->fb, b->fb);
        lk.lock();
        for (auto* q : batch) { q->rc = rc; q->done = true; }
        ++b->batches;
        b->leader = false;
        b->cv.notify_all();
    }
    if (--b->inflight == 0) b->cv.notify_all();                // (still under b->m) havc_batcher_free may be waiting for the last caller
    return r.rc;
}

int havc_zhang_frames(havc_ctx* c, havc_net* net, const uint8_t* rgb_in, uint8_t* rgb_out, int n_frames, int width, int height) {
    if (!c || !net || !rgb_in || !rgb_out || n_frames < 0 || width <= 0 || height <= 0) return fail(c, HAVC_E_INVALID, "zhang_frames: bad args");
    if (net->ctx != c || net->bufdesc[net->out_buf].elem_bytes != 4) return fail(c, HAVC_E_INVALID, "zhang_frames: not a Zhang net of this ctx");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, hipSetDevice(c->dev));
    const int S = net->S, maxb = net->max_batch;
    const size_t fb = (size_t)width * height * 3, sq = (size_t)S * S * 3;
    const bool in_dev = is_device_ptr(rgb_in), out_dev = is_device_ptr(rgb_out);
    int rc;
    if ((!in_dev && (rc = ensure_scratch(c, SCR_IN, fb * maxb))) || (rc = ensure_scratch(c, SCR_PIL_ROWS, (size_t)height * S * 3 * maxb)) ||
        (rc = ensure_scratch(c, SCR_SQUARE, sq * maxb)) || (!out_dev && (rc = ensure_scratch(c, SCR_RESULT, fb * maxb)))) return rc;
    uint8_t *d_tmp = (uint8_t*)c->scratch[SCR_PIL_ROWS], *d_sq = (uint8_t*)c->scratch[SCR_SQUARE];
    Timer t(c);
    for (int f0 = 0; f0 < n_frames; f0 += maxb) {
        const int b = std::min(maxb, n_frames - f0);
        const uint8_t* d_in = in_dev ? rgb_in + (size_t)f0 * fb : (const uint8_t*)c->scratch[SCR_IN];
        uint8_t* d_out = out_dev ? rgb_out + (size_t)f0 * fb : (uint8_t*)c->scratch[SCR_RESULT];
        if (!in_dev) HIP_TRY(c, hipMemcpyAsync(c->scratch[SCR_IN], rgb_in + (size_t)f0 * fb, fb * b, hipMemcpyHostToDevice, c->stream));
        if ((rc = pil_resize_dev(c, d_in, width, height, d_tmp, d_sq, S, S, b, 3))) return rc;                  // PIL BICUBIC -> 256x256
        net->in_override = d_sq;
        rc = run_ops_locked(net, 0, (int)net->ops.size(), b);
        net->in_override = nullptr;
        if (rc) return rc;
        c->stats.total_flops += net->flops_per_frame * b;
        int e = launch_zhang_post(d_in, (const float*)net->bufs[net->out_buf], S, S, d_out, b, width, height, c->stream);
        c->stats.launches++;
        if (e) return hip_fail(c, (hipError_t)e, "zhang post");
        if (!out_dev) {
            HIP_TRY(c, hipMemcpyAsync(rgb_out + (size_t)f0 * fb, d_out, fb * b, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
    }
    c->stats.frames += n_frames;
    return out_dev ? HAVC_OK : t.finish();
}

// shared body of the DDColor entry points.  out_planes != NULL: float / half planar output (the RGBS / RGBH shape of
// vsddcolor.ddcolor) instead of interleaved u8.
static int ddcolor_batch_locked(havc_ctx* c, havc_net* net, const uint8_t* d_in, uint8_t* d_out_u8, void* d_out_planes, int planes_half,
                                int b, int width, int height) {
    const int S = net->S;
    const int ab_pitch = (int)(net->bufdesc[net->out_buf].elems_per_frame / ((size_t)S * S));
    const bool squash = width != S || height != S;
    const size_t sq = (size_t)S * S * 3;
    int rc;
    const uint8_t* d_net_in = d_in;
    if (squash) {                                           // frame != input_size: Pillow BILINEAR to S x S (build's choice)
        if ((rc = ensure_scratch(c, SCR_PIL_ROWS, (size_t)height * S * 3 * b)) || (rc = ensure_scratch(c, SCR_SQUARE, sq * b))) return rc;
        d_net_in = (uint8_t*)c->scratch[SCR_SQUARE];
        if ((rc = pil_resize_dev(c, d_in, width, height, (uint8_t*)c->scratch[SCR_PIL_ROWS], (uint8_t*)c->scratch[SCR_SQUARE], S, S, b, 2))) return rc;
    }
    net->in_override = d_net_in;
    rc = run_ops_locked(net, 0, (int)net->ops.size(), b);
    net->in_override = nullptr;
    if (rc) return rc;
    c->stats.total_flops += net->flops_per_frame * b;
    const bool precise = !net->ops.empty() && (net->ops[0].flags & HAVC_F_PRECISE);          // precise nets: the ab map is a hi / lo pair tensor
    int e = launch_ddcolor_post(d_in, (const half_t*)net->bufs[net->out_buf], ab_pitch, 0, S, S, d_out_u8, d_out_planes, planes_half, b, width, height, c->stream,
                                precise ? ab_pitch >> 1 : 0);
    c->stats.launches++;
    if (e) return hip_fail(c, (hipError_t)e, "ddcolor post");
    return HAVC_OK;
}

int havc_ddcolor_frames(havc_ctx* c, havc_net* net, const uint8_t* rgb_in, uint8_t* rgb_out, int n_frames, int width, int height) {
    if (!c || !net || !rgb_in || !rgb_out || n_frames < 0 || width <= 0 || height <= 0) return fail(c, HAVC_E_INVALID, "ddcolor_frames: bad args");
    if (net->ctx != c || net->bufdesc[net->out_buf].elem_bytes != 2) return fail(c, HAVC_E_INVALID, "ddcolor_frames: not a DDColor net of this ctx");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, hipSetDevice(c->dev));
    const int maxb = net->max_batch;
    const size_t fb = (size_t)width * height * 3;
    const bool in_dev = is_device_ptr(rgb_in), out_dev = is_device_ptr(rgb_out);
    int rc;
    if ((!in_dev && (rc = ensure_scratch(c, SCR_IN, fb * maxb))) || (!out_dev && (rc = ensure_scratch(c, SCR_RESULT, fb * maxb)))) return rc;
    Timer t(c);
    for (int f0 = 0; f0 < n_frames; f0 += maxb) {
        const int b = std::min(maxb, n_frames - f0);
        const uint8_t* d_in = in_dev ? rgb_in + (size_t)f0 * fb : (const uint8_t*)c->scratch[SCR_IN];
        uint8_t* d_out = out_dev ? rgb_out + (size_t)f0 * fb : (uint8_t*)c->scratch[SCR_RESULT];
        if (!in_dev) HIP_TRY(c, hipMemcpyAsync(c->scratch[SCR_IN], rgb_in + (size_t)f0 * fb, fb * b, hipMemcpyHostToDevice, c->stream));
        if ((rc = ddcolor_batch_locked(c, net, d_in, d_out, nullptr, 0, b, width, height))) return rc;
        if (!out_dev) {
            HIP_TRY(c, hipMemcpyAsync(rgb_out + (size_t)f0 * fb, d_out, fb * b, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
    }
    c->stats.frames += n_frames;
    return out_dev ? HAVC_OK : t.finish();
}

int havc_ddcolor_frame_planar_f(havc_ctx* c, havc_net* net, const void* const in_planes[3], int in_stride_bytes, void* const out_planes[3],
                                int out_stride_bytes, int is_half, int width, int height) {
    if (!c || !net || !in_planes || !out_planes || width <= 0 || height <= 0) return fail(c, HAVC_E_INVALID, "ddcolor_frame_planar_f: bad args");
    for (int p = 0; p < 3; ++p) if (!in_planes[p] || !out_planes[p]) return fail(c, HAVC_E_INVALID, "ddcolor_frame_planar_f: NULL plane");
    if (net->ctx != c || net->bufdesc[net->out_buf].elem_bytes != 2) return fail(c, HAVC_E_INVALID, "ddcolor_frame_planar_f: not a DDColor net of this ctx");
    const size_t esz = is_half ? 2 : 4, row = (size_t)width * esz;
    if ((size_t)in_stride_bytes < row || (size_t)out_stride_bytes < row) return fail(c, HAVC_E_INVALID, "ddcolor_frame_planar_f: stride smaller than a row");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, hipSetDevice(c->dev));
    const size_t plane = row * height, fb = (size_t)width * height * 3;
    int rc;
    if ((rc = ensure_scratch(c, SCR_IN, fb)) || (rc = ensure_scratch(c, SCR_PLANES, 3 * plane)) || (rc = ensure_scratch(c, SCR_PLANES_OUT, 3 * plane))) return rc;
    uint8_t* d_planes_in = (uint8_t*)c->scratch[SCR_PLANES];
    uint8_t* d_planes_out = (uint8_t*)c->scratch[SCR_PLANES_OUT];
    for (int p = 0; p < 3; ++p)
        HIP_TRY(c, hipMemcpy2DAsync(d_planes_in + p * plane, row, in_planes[p], (size_t)in_stride_bytes, row, (size_t)height, hipMemcpyDefault, c->stream));
    // RGBH / RGBS full range [0, 1] -> the u8 frame the float clip was cast from (vsmodels.py:354,358): round(x * 255)
    int e = launch_planar_f_to_rgb8(d_planes_in, is_half, (uint8_t*)c->scratch[SCR_IN], (int64_t)width * height, c->stream);
    c->stats.launches++;
    if (e) return hip_fail(c, (hipError_t)e, "planar float -> rgb8");
    if ((rc = ddcolor_batch_locked(c, net, (const uint8_t*)c->scratch[SCR_IN], nullptr, d_planes_out, is_half, 1, width, height))) return rc;
    for (int p = 0; p < 3; ++p)
        HIP_TRY(c, hipMemcpy2DAsync(out_planes[p], (size_t)out_stride_bytes, d_planes_out + p * plane, row, row, (size_t)height, hipMemcpyDefault, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->stats.frames += 1;
    return HAVC_OK;
}

// one batch of the HAVC_colorizer(method=0) clip flow on device frames (the body of havc_colorize_clip[_host])
static int colorize_batch_locked(havc_ctx* c, havc_net* video, havc_net* second, float video_weight, const uint8_t* src, uint8_t* dst, int b,
                                 int width, int height) {
    const int S = video->S;
    const int64_t npix1 = (int64_t)S * S;
    const size_t fb = (size_t)npix1 * 3;
    uint8_t *d_sq = (uint8_t*)c->scratch[SCR_IN], *d_v = (uint8_t*)c->scratch[SCR_VIDEO], *d_s = (uint8_t*)c->scratch[SCR_SECOND], *d_col = (uint8_t*)c->scratch[SCR_RESULT];
    int rc;
    if (width == S && height == S) {
        HIP_TRY(c, hipMemcpyAsync(d_sq, src, fb * b, hipMemcpyDeviceToDevice, c->stream));
    } else if ((rc = resize_rgb8(c, src, width, height, d_sq, S, S, b, nullptr))) return rc;
    if ((rc = run_generators(c, video, second, d_sq, d_v, d_s, b))) return rc;
    if ((rc = deoldify_tail(c, d_sq, d_v, second ? d_s : nullptr, video_weight, 1, d_col, npix1 * b))) return rc;
    // Spline64 back to full size fused with vs_recover_clip_luma (chroma_post_process vs the source frame)
    return resize_rgb8(c, d_col, S, S, dst, width, height, b, src);
}

int havc_colorize_clip(havc_ctx* c, havc_net* video, havc_net* second, float video_weight, const uint8_t* d_src,
                       uint8_t* d_dst, int n_frames, int width, int height) {
    if (!c || !video || !d_src || !d_dst || n_frames < 0 || width <= 0 || height <= 0) return fail(c, HAVC_E_INVALID, "colorize_clip: bad args");
    if (video->ctx != c || (second && (second->ctx != c || second->S != video->S))) return fail(c, HAVC_E_INVALID, "colorize_clip: nets from another ctx / size");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, hipSetDevice(c->dev));
    const int S = video->S;
    int maxb = video->max_batch;
    if (second) maxb = std::min(maxb, second->max_batch);
    const size_t fb = (size_t)S * S * 3, fbig = (size_t)width * height * 3;
    int rc;
    for (int slot = SCR_IN; slot <= SCR_RESULT; ++slot)                  // SCR_IN, SCR_VIDEO, SCR_SECOND, SCR_RESULT
        if ((rc = ensure_scratch(c, slot, fb * maxb))) return rc;
    Timer t(c);
    for (int f0 = 0; f0 < n_frames; f0 += maxb) {
        const int b = std::min(maxb, n_frames - f0);
        if ((rc = colorize_batch_locked(c, video, second, video_weight, d_src + (size_t)f0 * fbig, d_dst + (size_t)f0 * fbig, b, width, height))) return rc;
    }
    c->stats.frames += n_frames;
    return t.finish();
}

// Host frames in, host frames out, PIPELINED: batch i+1 is uploaded and batch i-1 downloaded on two copy streams while batch i
// is on the compute stream (double-buffered device staging, events between the three streams).  With pinned host memory
// (havc_host_alloc) the copies are true DMA transfers: 6.2 MB per 1080p frame each way against 63 GB/s of PCIe Gen5.
int havc_colorize_clip_host(havc_ctx* c, havc_net* video, havc_net* second, float video_weight, const uint8_t* h_src, uint8_t* h_dst,
                            int n_frames, int width, int height) {
    if (!c || !video || !h_src || !h_dst || n_frames < 0 || width <= 0 || height <= 0) return fail(c, HAVC_E_INVALID, "colorize_clip_host: bad args");
    if (video->ctx != c || (second && (second->ctx != c || second->S != video->S))) return fail(c, HAVC_E_INVALID, "colorize_clip_host: nets from another ctx / size");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, hipSetDevice(c->dev));
    const int S = video->S;
    int maxb = video->max_batch;
    if (second) maxb = std::min(maxb, second->max_batch);
    const size_t fb = (size_t)S * S * 3, fbig = (size_t)width * height * 3;
    int rc;
    for (int slot = SCR_IN; slot <= SCR_RESULT; ++slot)                  // SCR_IN, SCR_VIDEO, SCR_SECOND, SCR_RESULT
        if ((rc = ensure_scratch(c, slot, fb * maxb))) return rc;
    for (int slot = SCR_CLIP_SRC; slot < SCR_CLIP_DST + 2; ++slot)     // both source batches, both result batches
        if ((rc = ensure_scratch(c, slot, fbig * maxb))) return rc;
    if (!c->stream_h2d) {
        HIP_TRY(c, hipStreamCreateWithFlags(&c->stream_h2d, hipStreamNonBlocking));
        HIP_TRY(c, hipStreamCreateWithFlags(&c->stream_d2h, hipStreamNonBlocking));
        for (int k = 0; k < 2; ++k) {
            HIP_TRY(c, hipEventCreateWithFlags(&c->ev_up[k], hipEventDisableTiming));
            HIP_TRY(c, hipEventCreateWithFlags(&c->ev_comp[k], hipEventDisableTiming));
            HIP_TRY(c, hipEventCreateWithFlags(&c->ev_down[k], hipEventDisableTiming));
        }
    }
    auto body = [&]() -> int {
        int i = 0;
        for (int f0 = 0; f0 < n_frames; f0 += maxb, ++i) {
            const int b = std::min(maxb, n_frames - f0), s = i & 1;
            uint8_t *src = (uint8_t*)c->scratch[SCR_CLIP_SRC + s], *dst = (uint8_t*)c->scratch[SCR_CLIP_DST + s];
            if (i >= 2) HIP_TRY(c, hipStreamWaitEvent(c->stream_h2d, c->ev_comp[s], 0));      // batch i-2 has consumed this source slot
            HIP_TRY(c, hipMemcpyAsync(src, h_src + (size_t)f0 * fbig, fbig * b, hipMemcpyHostToDevice, c->stream_h2d));
            HIP_TRY(c, hipEventRecord(c->ev_up[s], c->stream_h2d));
            HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_up[s], 0));
            if (i >= 2) HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_down[s], 0));           // batch i-2's result has left this slot
            int r = colorize_batch_locked(c, video, second, video_weight, src, dst, b, width, height);
            if (r) return r;
            HIP_TRY(c, hipEventRecord(c->ev_comp[s], c->stream));
            HIP_TRY(c, hipStreamWaitEvent(c->stream_d2h, c->ev_comp[s], 0));
            HIP_TRY(c, hipMemcpyAsync(h_dst + (size_t)f0 * fbig, dst, fbig * b, hipMemcpyDeviceToHost, c->stream_d2h));
            HIP_TRY(c, hipEventRecord(c->ev_down[s], c->stream_d2h));
        }
        return HAVC_OK;
    };
    rc = body();
    const std::string keep = c->err;
    hipError_t e1 = hipStreamSynchronize(c->stream_h2d), e2 = sync_streams(c), e3 = hipStreamSynchronize(c->stream_d2h);
    if (rc) { (void)hipGetLastError(); c->err = keep; return rc; }
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) return hip_fail(c, e1 != hipSuccess ? e1 : (e2 != hipSuccess ? e2 : e3), "colorize_clip_host drain");
    c->stats.frames += n_frames;
    return HAVC_OK;
}

// ---- planar <-> interleaved (vsslib/vsutils.py:60-110: frame_to_image / image_to_frame / frame_to_np_array / np_array_to_frame) ----
int havc_planar_to_rgb8(havc_ctx* c, const uint8_t* const planes[3], int stride, uint8_t* rgb, int width, int height) {
    if (!c || !planes || !rgb || width <= 0 || height <= 0 || stride < width) return fail(c, HAVC_E_INVALID, "planar_to_rgb8: bad args");
    for (int p = 0; p < 3; ++p) if (!planes[p]) return fail(c, HAVC_E_INVALID, "planar_to_rgb8: NULL plane");
    Call call(c, "planar_to_rgb8");
    const size_t plane = (size_t)width * height, nb = plane * 3;
    uint8_t* d_pl = (uint8_t*)call.scratch(SCR_PLANES, nb);
    uint8_t* dout = call.out(SCR_OUT, rgb, nb);
    for (int p = 0; p < 3 && !call.rc; ++p)                              // rows with a stride: packed on their way in
        call.check(hipMemcpy2DAsync(d_pl + p * plane, (size_t)width, planes[p], (size_t)stride, (size_t)width, (size_t)height, hipMemcpyDefault, c->stream), "hipMemcpy2DAsync");
    if (call.rc) return call.rc;
    call.launched(launch_planar_to_rgb8(d_pl, dout, (int64_t)plane, c->stream));
    return call.done();
}

int havc_rgb8_to_planar(havc_ctx* c, const uint8_t* rgb, uint8_t* const planes[3], int stride, int width, int height) {
    if (!c || !planes || !rgb || width <= 0 || height <= 0 || stride < width) return fail(c, HAVC_E_INVALID, "rgb8_to_planar: bad args");
    for (int p = 0; p < 3; ++p) if (!planes[p]) return fail(c, HAVC_E_INVALID, "rgb8_to_planar: NULL plane");
    Call call(c, "rgb8_to_planar");
    const size_t plane = (size_t)width * height, nb = plane * 3;
    const uint8_t* din = call.in(SCR_IN, rgb, nb);
    uint8_t* d_pl = (uint8_t*)call.scratch(SCR_PLANES, nb);
    if (call.rc) return call.rc;
    call.launched(launch_rgb8_to_planar(din, d_pl, (int64_t)plane, c->stream));
    for (int p = 0; p < 3 && !call.rc; ++p)                              // rows with a stride: spread on their way out
        call.check(hipMemcpy2DAsync(planes[p], (size_t)stride, d_pl + p * plane, (size_t)width, (size_t)width, (size_t)height, hipMemcpyDefault, c->stream), "hipMemcpy2DAsync");
    call.sync();                                                         // whatever the planes' kind, as ever
    return call.done();
}

// One VapourSynth frame through ModelImageRender: the selector body of vs_sc_deoldify (vsslib/vsmodels.py:214-230) --
// frame_to_image, get_transformed_image, image_to_frame -- with the plane <-> interleaved shuffles on the GPU.
int havc_deoldify_frame_planar(havc_ctx* c, havc_net* video, havc_net* second, float video_weight, int post_process,
                               const uint8_t* const in_planes[3], int in_stride, uint8_t* const out_planes[3], int out_stride) {
    if (!c || !video || !in_planes || !out_planes) return fail(c, HAVC_E_INVALID, "deoldify_frame_planar: bad args");
    if (video->ctx != c || (second && (second->ctx != c || second->S != video->S))) return fail(c, HAVC_E_INVALID, "deoldify_frame_planar: nets from another ctx / size");
    const int S = video->S;
    if (in_stride < S || out_stride < S) return fail(c, HAVC_E_INVALID, "deoldify_frame_planar: stride smaller than the render size");
    for (int p = 0; p < 3; ++p) if (!in_planes[p] || !out_planes[p]) return fail(c, HAVC_E_INVALID, "deoldify_frame_planar: NULL plane");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, hipSetDevice(c->dev));
    const size_t plane = (size_t)S * S, fb = plane * 3;
    int rc;
    for (int slot = SCR_IN; slot <= SCR_PLANES; ++slot)                  // SCR_IN, SCR_VIDEO, SCR_SECOND, SCR_RESULT, SCR_PLANES
        if ((rc = ensure_scratch(c, slot, fb))) return rc;
    uint8_t *d_in = (uint8_t*)c->scratch[SCR_IN], *d_v = (uint8_t*)c->scratch[SCR_VIDEO], *d_s = (uint8_t*)c->scratch[SCR_SECOND], *d_out = (uint8_t*)c->scratch[SCR_RESULT],
            *d_pl = (uint8_t*)c->scratch[SCR_PLANES];
    Timer t(c);
    for (int p = 0; p < 3; ++p)
        HIP_TRY(c, hipMemcpy2DAsync(d_pl + p * plane, (size_t)S, in_planes[p], (size_t)in_stride, (size_t)S, (size_t)S, hipMemcpyDefault, c->stream));
    int e = launch_planar_to_rgb8(d_pl, d_in, (int64_t)plane, c->stream);
    if (e) return hip_fail(c, (hipError_t)e, "planar_to_rgb8");
    if ((rc = run_generators(c, video, second, d_in, d_v, d_s, 1))) return rc;
    if ((rc = deoldify_tail(c, d_in, d_v, second ? d_s : nullptr, video_weight, post_process, d_out, (int64_t)plane))) return rc;
    e = launch_rgb8_to_planar(d_out, d_pl, (int64_t)plane, c->stream);
    c->stats.launches += 2;
    if (e) return hip_fail(c, (hipError_t)e, "rgb8_to_planar");
    for (int p = 0; p < 3; ++p)
        HIP_TRY(c, hipMemcpy2DAsync(out_planes[p], (size_t)out_stride, d_pl + p * plane, (size_t)S, (size_t)S, (size_t)S, hipMemcpyDefault, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->stats.frames += 1;
    return t.finish();
}

}  // extern "C"
