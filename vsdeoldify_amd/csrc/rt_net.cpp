// libhavc_mi355.so runtime, plan executor: packed weights, nets (create / free / bind / run), the per-op dispatch, autotuner, profiler, range check.
#include "runtime_internal.h"
#include "conv_common.h"

namespace {

int run_op(havc_net* n, const havc_op& op, int batch) {
    havc_ctx* c = n->ctx;
    hipStream_t s = c->cur ? c->cur : c->stream;
    int e = 0;
    const bool timed = (op.tag == c->timed_tag && c->timed_tag >= 0 && op.type == HAVC_OP_CONV);
    std::pair<hipEvent_t, hipEvent_t> evp{nullptr, nullptr};
    auto open_tag_pair = [&]() -> int {                     // tag timing: take the next event pair and record its start
        if (c->tag_used == c->tag_events.size()) {
            hipEvent_t a, b;
            HIP_TRY(c, hipEventCreate(&a));
            HIP_TRY(c, hipEventCreate(&b));
            c->tag_events.emplace_back(a, b);
        }
        evp = c->tag_events[c->tag_used++];
        HIP_TRY(c, hipEventRecord(evp.first, s));
        return HAVC_OK;
    };
    if (timed) if (int rc = open_tag_pair()) return rc;
    const bool precise = op.flags & HAVC_F_PRECISE;         // fast / precise twins with one parameter list: pick the function, write the call once
    // Dense-frame ops (MAXPOOL, BLUR_RESIZE, AFFINE, COPY_CH, PREP_RGB8, fast ATTENTION, SUBSAMPLE2, PROJ2, DWCONV7, DWCONV7_LN, SHUF4_BLUR_AB, LAYERNORM,
    // PIXSHUF4_BLUR): their kernels place frame b at b x rows x pitch.  That is the
    // buffer's own frame only where the view fills it; a view that covers part of its buffer's frame (the h x w patch rows of a token buffer whose
    // frame also holds a class row) runs one launch per frame, each pointer advanced by its buffer's own frame size -- as the conv op does.
    auto fills = [&](int id, uint64_t elems) { return (uint64_t)n->bufdesc[id].elems_per_frame == elems; };
    auto frame_at = [&](int id, int f) { return (char*)bufptr(n, id) + (uint64_t)f * n->bufdesc[id].elems_per_frame * n->bufdesc[id].elem_bytes; };
    auto by_frame = [&](bool dense, auto&& launch) -> int {     // launch(first frame, frames) -> hipError
        if (dense || batch == 1) return launch(0, batch);
        int rc = 0;
        for (int f = 0; f < batch && rc == 0; ++f) {
            rc = launch(f, 1);
            if (f > 0) c->stats.launches += 1;
        }
        return rc;
    };
    const uint64_t src_rows = (uint64_t)op.Hi * op.Wi, dst_rows = (uint64_t)op.Ho * op.Wo;
    switch (op.type) {
        case HAVC_OP_CONV: {
            ConvArgs a{};
            a.x = (const half_t*)bufptr(n, op.src);
            a.w = wptr<half_t>(n, op.w_off);
            if (op.flags & HAVC_F_W_FROM_BUF) {
                if (op.src2 < 0 || op.src2 >= (int)n->bufs.size() || (op.flags & HAVC_F_RESIDUAL))
                    return fail(c, HAVC_E_INVALID, "conv op: W_FROM_BUF needs a weight buffer in src2 and no residual");
                if ((uint64_t)n->bufdesc[op.src2].elems_per_frame * n->bufdesc[op.src2].elem_bytes < (uint64_t)op.Npad * op.Kc * 16)
                    return fail(c, HAVC_E_INVALID, "conv op: W_FROM_BUF buffer smaller than Npad x Kc x 16 bytes per frame");
                a.w = (const half_t*)bufptr(n, op.src2);
            }
            a.bias = wptr<float>(n, op.bias_off);
            a.scale = wptr<float>(n, op.scale_off);
            a.shift = wptr<float>(n, op.shift_off);
            int rows_per_frame = op.Ho * op.Wo;
            if (op.flags & HAVC_F_PS_BLUR) {
                if (!(op.flags & HAVC_F_OUT_PIXSHUF) || op.kh != 1 || op.kw != 1 || op.stride != 1 || op.pad != 0 || (op.Co & 63) ||
                    op.Npad != 4 * op.Co || (op.Npad & 255) || op.out_step > 1 || (op.flags & (HAVC_F_RESIDUAL | HAVC_F_RELU_POST)))
                    return fail(c, HAVC_E_INVALID, "conv op: PS_BLUR needs a 1x1 stride-1 pixel-shuffle conv with Co % 64 == 0");
                if (op.aux0 < 0 || (op.aux0 & 7) || op.aux0 > op.Co) return fail(c, HAVC_E_INVALID, "conv op: PS_BLUR aux0 = stored channels (multiple of 8, <= Co)");
                a.cstore = op.aux0;
                a.tiles_y = (op.Ho + 14) / 15;
                a.tiles_x = (op.Wo + 14) / 15;
                rows_per_frame = a.tiles_y * a.tiles_x * 256;
            }
            if (op.flags & HAVC_F_FUSE_RGB8) {
                if (op.Npad != 272 || !a.scale || !a.shift || op.aux0 < 0 || op.aux0 >= (int)n->bufs.size())
                    return fail(c, HAVC_E_INVALID, "conv op: FUSE_RGB8 needs Npad 272, fused weights/bias and an RGB8 buffer");
                a.fuse_w = a.scale; a.fuse_b = a.shift; a.scale = a.shift = nullptr;
                a.fuse_rgb = (uint8_t*)bufptr(n, op.aux0);
            }
            uint64_t proj_wf = 0, proj_of = 0;                 // FUSE_PROJ: bytes per frame of the projection matrix / of the output
            if (op.flags & HAVC_F_FUSE_PROJ) {
                if ((op.Npad & 255) || ((op.Ho * op.Wo) & 15) || (op.flags & (HAVC_F_RESIDUAL | HAVC_F_W_FROM_BUF | HAVC_F_OUT_PIXSHUF)) || op.src2 < 0 ||
                    op.src2 >= (int)n->bufs.size() || op.aux0 < 0 || op.aux0 >= (int)n->bufs.size())
                    return fail(c, HAVC_E_INVALID, "conv op: FUSE_PROJ needs Npad % 256 == 0, Ho*Wo % 16 == 0, a matrix buffer (src2) and an output buffer (aux0)");
                proj_wf = (uint64_t)n->bufdesc[op.src2].elems_per_frame * n->bufdesc[op.src2].elem_bytes;
                proj_of = (uint64_t)n->bufdesc[op.aux0].elems_per_frame * n->bufdesc[op.aux0].elem_bytes;
                if (proj_wf != 2 * 256 * 4 || proj_of < (uint64_t)op.Ho * op.Wo * (op.Npad / 256) * 8)
                    return fail(c, HAVC_E_INVALID, "conv op: FUSE_PROJ buffers: fp32 [2][256] matrix per frame, fp32 [Ho*Wo][Npad/256][2] output");
                a.fuse_w = (const float*)bufptr(n, op.src2);
                a.fuse_out = (float*)bufptr(n, op.aux0);
            }
            a.res = (op.flags & HAVC_F_RESIDUAL) ? (const half_t*)bufptr(n, op.src2) : nullptr;
            a.y = bufptr(n, op.dst);
            a.x_cpitch = op.src_cpitch; a.x_coff = op.src_coff;
            a.res_cpitch = op.res_cpitch; a.res_coff = op.res_coff;
            a.y_cpitch = op.dst_cpitch; a.y_coff = op.dst_coff;
            a.Hi = op.Hi; a.Wi = op.Wi; a.C8 = op.Ci / 8;
            a.Ho = op.Ho; a.Wo = op.Wo; a.Co = op.Co;
            a.kh = op.kh; a.kw = op.kw; a.stride = op.stride; a.pad = op.pad; a.dil = op.dil;
            a.pad_w = op.pad + op.pad_w_delta;
            a.oss = op.out_step == 2 ? 2 : 1; a.ooy = op.out_oy; a.oox = op.out_ox;
            a.Kc = op.Kc; a.Npad = op.Npad;
            a.M = batch * op.Ho * op.Wo;   // (PS_BLUR: set below)
            a.flags = op.flags;
            if (c->nt_store_bytes && (uint64_t)batch * n->bufdesc[op.dst].elems_per_frame * n->bufdesc[op.dst].elem_bytes >= c->nt_store_bytes)
                a.flags |= HAVC_F_NT_STORE;
            a.pix_pitch = (op.flags & HAVC_F_PS_BLUR) ? 0 : op.aux0;
            a.C8a = (op.aux1 > 0 && op.aux1 < op.Ci / 8) ? op.aux1 : op.Ci / 8;
            a.f0 = op.f0; a.f1 = op.f1; a.f2 = op.f2;
            a.cfg = op.reserved;
            conv_set_divisors(a);          // Ho, Wo, tiles_y, tiles_x stand: multiplier + shift of the kernels' index divisions (a few host divisions per op)
            a.k_half_empty = n->k_half_empty[(size_t)(&op - n->ops.data())];
            { static const int prio = [] { const char* e = getenv("HAVC_SETPRIO"); return e ? atoi(e) != 0 : 1; }(); a.prio = prio; }
            a.splitk = HAVC_F_SPLITK_COUNT(op.flags);
            if (a.splitk == 1) a.splitk = 0;
            a.pscale = 1.f;
            if (op.flags & HAVC_F_PRECISE) {
                if ((op.flags & HAVC_F_W_FROM_BUF) || a.splitk ||
                    !(op.f3 > 0.f) || (op.src_cpitch & 15) || (!(op.flags & HAVC_F_OUT_RGB8) && (op.dst_cpitch & 15)))
                    return fail(c, HAVC_E_INVALID, "conv op: PRECISE needs a plain conv (no fused / transposed / split-K form), f3 = accumulator scale > 0, hi|lo pixel rows");
                a.pscale = op.f3;
            }
            if (a.splitk) {
                if ((op.flags & (HAVC_F_PS_BLUR | HAVC_F_FUSE_RGB8 | HAVC_F_FUSE_PROJ | HAVC_F_W_FROM_BUF | HAVC_F_OUT_RGB8)) || (op.Kc >> 3) < 2 * a.splitk)
                    return fail(c, HAVC_E_INVALID, "conv op: SPLITK needs a plain conv with at least 2 K stages per part");
                if (s != c->stream && s != c->stream2) return fail(c, HAVC_E_INVALID, "conv op: SPLITK ops run on the ctx's own streams (one workspace per stream)");
                const int slot = s == c->stream ? SCR_SPLITK_MAIN : SCR_SPLITK_SIDE;         // the two generators of a stable / artistic render run side by side on the two streams
                const size_t need = (size_t)a.splitk * batch * op.Ho * op.Wo * op.Npad * 4;
                if (int rc2 = ensure_scratch(c, slot, need)) return rc2;
                a.ws = (float*)c->scratch[slot];
            }
            {
                const int oi = (int)(&op - n->ops.data());
                a.ktab = n->ktab_off[oi] >= 0 ? n->d_ktab + n->ktab_off[oi] : nullptr;
                const uint64_t xb = (uint64_t)n->bufdesc[op.src].elems_per_frame * n->bufdesc[op.src].elem_bytes * n->max_batch + 256;
                a.x_bytes = xb < 0xF0000000ull ? (unsigned)xb : 0u;          // 0: descriptor path unavailable
                const uint64_t wb = (uint64_t)op.Npad * op.Kc * 16;
                a.w_bytes = wb < 0xF0000000ull ? (unsigned)wb : 0xFFFFFFFFu;
            }
            const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
            for (int i = 0; i < 3; ++i) { a.mean[i] = mean[i]; a.istd[i] = stdv[i]; }
            if (!a.w || (op.Kc & 7) || a.C8 <= 0 || !a.ktab) return fail(c, HAVC_E_INVALID, "conv op: bad weights / Kc / Ci");
            if ((op.flags & HAVC_F_AFFINE) && (!a.scale || !a.shift)) return fail(c, HAVC_E_INVALID, "conv op: AFFINE without scale/shift");
            {
                // frames per launch: keep every operand within the 32-bit range of a buffer descriptor (and of the
                // kernels' int pixel indices); big batches of the 560x560 tail run as several launches.
                const uint64_t lim = c->desc_limit;
                const uint64_t xf = (uint64_t)n->bufdesc[op.src].elems_per_frame * n->bufdesc[op.src].elem_bytes;
                const uint64_t yf = (uint64_t)n->bufdesc[op.dst].elems_per_frame * n->bufdesc[op.dst].elem_bytes;
                const uint64_t rf = a.res ? (uint64_t)n->bufdesc[op.src2].elems_per_frame * n->bufdesc[op.src2].elem_bytes : 0;
                int chunk = batch;
                const uint64_t big = std::max(xf, std::max(yf, rf));
                if (big * (uint64_t)batch > lim) {
                    chunk = (int)std::max<uint64_t>(1, lim / big);
                    const int nch = (batch + chunk - 1) / chunk;           // equal launches (32 frames of the 560 x 560 tail: 16 + 16, not 18 + 14)
                    chunk = (batch + nch - 1) / nch;
                }
                // A multi-frame launch walks M = frames x rows CONTIGUOUS rows.  A view that covers only part of its buffer's frame (the h0 x w0
                // patch rows of a DINOv2 token buffer whose frame also holds the class row) does not continue into the next frame:
                // one launch per frame, each at its buffer's own frame stride.
                {
                    const bool plain_out = !(op.flags & (HAVC_F_OUT_PIXSHUF | HAVC_F_OUT_TRANSPOSED | HAVC_F_OUT_RGB8 | HAVC_F_FUSE_RGB8 | HAVC_F_FUSE_PROJ | HAVC_F_PS_BLUR)) && a.oss == 1;
                    bool contiguous = (uint64_t)op.Hi * op.Wi * op.src_cpitch == (uint64_t)n->bufdesc[op.src].elems_per_frame;
                    if (plain_out && (uint64_t)op.Ho * op.Wo * op.dst_cpitch != (uint64_t)n->bufdesc[op.dst].elems_per_frame) contiguous = false;
                    if (plain_out && a.res && !(op.flags & HAVC_F_W_FROM_BUF) && (uint64_t)op.Ho * op.Wo * op.res_cpitch != (uint64_t)n->bufdesc[op.src2].elems_per_frame)
                        contiguous = false;
                    if (!contiguous && batch > 1) chunk = 1;
                }
                const char* w0 = (const char*)a.w;
                uint64_t wf = 0;
                if (op.flags & HAVC_F_W_FROM_BUF) {        // per-frame weights taken from an activation buffer: one launch per frame
                    chunk = 1;
                    wf = (uint64_t)n->bufdesc[op.src2].elems_per_frame * n->bufdesc[op.src2].elem_bytes;
                }
                const char* x0 = (const char*)a.x; const char* r0 = (const char*)a.res; char* y0 = (char*)a.y;
                uint8_t* rgb0 = a.fuse_rgb;
                for (int f0 = 0; f0 < batch && e == 0; f0 += chunk) {
                    const int nb = std::min(chunk, batch - f0);
                    if (timed && f0 > 0) {                                 // tag timing is per LAUNCH: close this pair, open the next
                        HIP_TRY(c, hipEventRecord(evp.second, s));
                        if (int rc2 = open_tag_pair()) return rc2;
                    }
                    a.x = (const half_t*)(x0 + (uint64_t)f0 * xf);
                    a.y = y0 + (uint64_t)f0 * yf;
                    if (r0) a.res = (const half_t*)(r0 + (uint64_t)f0 * rf);
                    if (wf) a.w = (const half_t*)(w0 + (uint64_t)f0 * wf);
                    if (rgb0) a.fuse_rgb = rgb0 + (uint64_t)f0 * op.Ho * op.Wo * 3;
                    if (proj_wf) {
                        a.fuse_w = (const float*)((const char*)bufptr(n, op.src2) + (uint64_t)f0 * proj_wf);
                        a.fuse_out = (float*)((char*)bufptr(n, op.aux0) + (uint64_t)f0 * proj_of);
                    }
                    a.M = nb * rows_per_frame;
                    a.x_bytes = (unsigned)std::min<uint64_t>(xf * (uint64_t)nb + 256, 0xEFFFFFFFull);
                    e = launch_conv(a, s);
                    if (f0 > 0) c->stats.launches += 1;
                }
            }
            break;
        }
        case HAVC_OP_MAXPOOL:
            e = by_frame(fills(op.src, src_rows * op.src_cpitch) && fills(op.dst, dst_rows * op.dst_cpitch), [&](int f, int nb) {
                return (precise ? launch_maxpool3x3s2_p : launch_maxpool3x3s2)((const half_t*)frame_at(op.src, f), (half_t*)frame_at(op.dst, f), nb, op.Hi, op.Wi,
                                                                               op.Ho, op.Wo, op.Ci, op.src_cpitch, op.src_coff, op.dst_cpitch, op.dst_coff, s);
            });
            break;
        case HAVC_OP_BLUR_RESIZE:
            e = by_frame(fills(op.src, src_rows * op.src_cpitch) && fills(op.dst, dst_rows * op.dst_cpitch), [&](int f, int nb) {
                return (precise ? launch_blur_resize_p : launch_blur_resize)((const half_t*)frame_at(op.src, f), (half_t*)frame_at(op.dst, f), nb, op.Hi, op.Wi,
                                                                             op.Ho, op.Wo, op.Ci, op.src_cpitch, op.src_coff, op.dst_cpitch, op.dst_coff, s);
            });
            break;
        case HAVC_OP_AFFINE:
            e = by_frame(fills(op.src, src_rows * op.src_cpitch) && fills(op.dst, src_rows * op.dst_cpitch), [&](int f, int nb) {
                return (precise ? launch_affine_p : launch_affine)((const half_t*)frame_at(op.src, f), (half_t*)frame_at(op.dst, f), wptr<float>(n, op.scale_off),
                                                                   wptr<float>(n, op.shift_off), (op.flags & HAVC_F_RELU_POST) ? 1 : 0,
                                                                   (int64_t)nb * op.Hi * op.Wi, op.Ci, op.src_cpitch, op.src_coff, op.dst_cpitch, op.dst_coff, s);
            });
            break;
        case HAVC_OP_COPY_CH:
            e = by_frame(fills(op.src, src_rows * op.src_cpitch) && fills(op.dst, src_rows * op.dst_cpitch), [&](int f, int nb) {
                return launch_copy_ch((const half_t*)frame_at(op.src, f), (half_t*)frame_at(op.dst, f), (int64_t)nb * op.Hi * op.Wi, op.Ci, op.src_cpitch,
                                      op.src_coff, op.dst_cpitch, op.dst_coff, s);
            });
            break;
        case HAVC_OP_ATTENTION:
            if (op.flags & HAVC_F_PRECISE) {
                // aux1 = NHWC value buffer (pixel pitch Kc), kh = fp32 scratch buffer [N][2] per frame (row maximum and sum of the softmax)
                if (op.kh < 0 || op.kh >= (int)n->bufs.size() || n->bufdesc[op.kh].elem_bytes != 4 ||
                    (uint64_t)n->bufdesc[op.kh].elems_per_frame < (uint64_t)op.Hi * op.Wi * 2 || !attention_p_supported(op.aux0, op.Ci))
                    return fail(c, HAVC_E_INVALID, "attention op: PRECISE needs an fp32 [N][2] scratch buffer in kh, d <= 128, C % 128 == 0");
                if (op.flags & HAVC_F_OUT_TRANSPOSED) {
                    // round 5: the value map arrives TRANSPOSED ([2][C][Kc] fp16 per frame: hi plane, lo plane; written by the value conv's transposed precise
                    // epilogue) and the P . H product runs on MFMA with the three-term splitting (csrc/precise.hip pattn_apply_mfma_kernel)
                    if (!attention_pm_supported(op.aux0, op.Ci, op.Kc) || (uint64_t)n->bufdesc[op.aux1].elems_per_frame < (uint64_t)2 * op.Ci * op.Kc ||
                        op.Kc < ((op.Hi * op.Wi + 31) & ~31))
                        return fail(c, HAVC_E_INVALID, "attention op: PRECISE | OUT_TRANSPOSED needs C % 256 == 0 and a [2][C][Kc] value buffer, Kc % 32 == 0, Kc >= N");
                    e = launch_attention_pm((const half_t*)bufptr(n, op.src2), op.res_cpitch, op.res_coff, op.res_coff + op.aux0, op.aux0,
                                            n->bufdesc[op.src2].elems_per_frame, (const half_t*)bufptr(n, op.aux1), op.Kc, n->bufdesc[op.aux1].elems_per_frame,
                                            (const half_t*)bufptr(n, op.src), op.src_cpitch, op.src_coff, n->bufdesc[op.src].elems_per_frame,
                                            (half_t*)bufptr(n, op.dst), op.dst_cpitch, op.dst_coff, n->bufdesc[op.dst].elems_per_frame, (float*)bufptr(n, op.kh),
                                            batch, op.Hi * op.Wi, op.Ci, op.f0, s);
                    c->stats.launches += 1;
                    break;
                }
                e = launch_attention_p((const half_t*)bufptr(n, op.src2), op.res_cpitch, op.res_coff, op.res_coff + op.aux0, op.aux0,
                                       n->bufdesc[op.src2].elems_per_frame, (const half_t*)bufptr(n, op.aux1), op.Kc, 0, n->bufdesc[op.aux1].elems_per_frame,
                                       (const half_t*)bufptr(n, op.src), op.src_cpitch, op.src_coff, n->bufdesc[op.src].elems_per_frame,
                                       (half_t*)bufptr(n, op.dst), op.dst_cpitch, op.dst_coff, n->bufdesc[op.dst].elems_per_frame, (float*)bufptr(n, op.kh),
                                       batch, op.Hi * op.Wi, op.Ci, op.f0, s);
                c->stats.launches += 1;
                break;
            }
            {
                // fast form: qk = [N][res_cpitch] with f at res_coff and g at res_coff + d, aux1 = V^T [C][Kc], x / y = C-channel views.  Everything the
                // kernels take on trust is checked here, before any launch.
                const int d = op.aux0, C = op.Ci;
                const uint64_t N = src_rows;
                if (d != 32 && d != 64 && d != 96) return fail(c, HAVC_E_INVALID, "attention op: d (aux0) must be 32, 64 or 96");
                if (C < 128 || (C & 127)) return fail(c, HAVC_E_INVALID, "attention op: C % 128 == 0");
                if (N < 1 || op.Kc < 64 || (op.Kc & 63) || (uint64_t)op.Kc < N) return fail(c, HAVC_E_INVALID, "attention op: value pitch Kc % 64 == 0, Kc >= N");
                if (op.src2 < 0 || op.res_coff < 0 || op.src_coff < 0 || op.dst_coff < 0 || op.res_coff + 2 * d > op.res_cpitch || op.src_coff + C > op.src_cpitch ||
                    op.dst_coff + C > op.dst_cpitch || ((op.res_coff | op.res_cpitch | op.src_coff | op.src_cpitch | op.dst_coff | op.dst_cpitch) & 7))
                    return fail(c, HAVC_E_INVALID, "attention op: views inside their pixel rows (res_coff + 2 d <= res_cpitch, coff + C <= cpitch), in units of 8 channels");
                const havc_buf &bq = n->bufdesc[op.src2], &bv = n->bufdesc[op.aux1], &bx = n->bufdesc[op.src], &by = n->bufdesc[op.dst];
                if (bq.elem_bytes != 2 || bv.elem_bytes != 2 || bx.elem_bytes != 2 || by.elem_bytes != 2 || (uint64_t)bq.elems_per_frame < N * op.res_cpitch ||
                    (uint64_t)bx.elems_per_frame < N * op.src_cpitch || (uint64_t)by.elems_per_frame < N * op.dst_cpitch ||
                    (uint64_t)bv.elems_per_frame < (uint64_t)C * op.Kc)
                    return fail(c, HAVC_E_INVALID, "attention op: fp16 buffers of N x pitch elements per frame, V^T of C x Kc");
                const bool dense = fills(op.src2, N * op.res_cpitch) && fills(op.aux1, (uint64_t)C * op.Kc) && fills(op.src, N * op.src_cpitch) &&
                                   fills(op.dst, N * op.dst_cpitch);
                e = by_frame(dense, [&](int f, int nb) {
                    return launch_attention((const half_t*)frame_at(op.src2, f), op.res_cpitch, op.res_coff, op.res_coff + d, d, (const half_t*)frame_at(op.aux1, f), C,
                                            op.Kc, (const half_t*)frame_at(op.src, f), op.src_cpitch, op.src_coff, (half_t*)frame_at(op.dst, f), op.dst_cpitch,
                                            op.dst_coff, nb, (int)N, op.f0, s);
                });
            }
            break;
        case HAVC_OP_PREP_RGB8:
            e = by_frame(fills(op.src, src_rows * 3) && fills(op.dst, src_rows * op.dst_cpitch) && (op.src2 < 0 || fills(op.src2, src_rows * op.res_cpitch)),
                         [&](int f, int nb) {
                const uint8_t* rgb = (const uint8_t*)frame_at(op.src, f);
                half_t *y0 = (half_t*)frame_at(op.dst, f), *y1 = op.src2 >= 0 ? (half_t*)frame_at(op.src2, f) : nullptr;
                if (precise) return launch_prep_rgb8_p(rgb, y0, op.dst_cpitch, op.dst_coff, y1, op.res_cpitch, op.res_coff, (int64_t)nb * op.Hi * op.Wi, s);
                return launch_prep_rgb8(rgb, y0, op.dst_cpitch, op.dst_coff, y1, op.res_cpitch, op.res_coff, (int64_t)nb * op.Hi * op.Wi, s,
                                        op.aux0 > 0 && op.res_coff + 8 + op.aux0 <= op.res_cpitch ? op.aux0 : 0);
            });
            break;
        case HAVC_OP_SUBSAMPLE2:
            e = by_frame(fills(op.src, src_rows * op.src_cpitch) && fills(op.dst, dst_rows * op.dst_cpitch), [&](int f, int nb) {
                return (precise ? launch_subsample2_p : launch_subsample2)((const half_t*)frame_at(op.src, f), (half_t*)frame_at(op.dst, f), nb, op.Ho, op.Wo, op.Hi,
                                                                           op.Wi, op.Ci, op.src_cpitch, op.src_coff, op.dst_cpitch, op.dst_coff, s);
            });
            break;
        case HAVC_OP_PROJ2:
            if (!precise && (op.w_off < 0 || op.Ci < 1 || op.Ci > 512)) return fail(c, HAVC_E_INVALID, "proj2 op: weights, 1 <= C <= 512 (eight channels per lane)");
            e = by_frame(fills(op.src, src_rows * op.src_cpitch) && fills(op.dst, src_rows * 2), [&](int f, int nb) {
                if (precise)
                    return launch_proj2_p((const half_t*)frame_at(op.src, f), op.src_cpitch, op.src_coff, op.Ci, wptr<float>(n, op.w_off), wptr<float>(n, op.bias_off),
                                          op.flags & 3, op.f0, (float*)frame_at(op.dst, f), (int64_t)nb * op.Hi * op.Wi, s);
                return launch_proj2((const half_t*)frame_at(op.src, f), op.src_cpitch, op.src_coff, op.Ci, wptr<float>(n, op.w_off),
                                    wptr<float>(n, op.bias_off), op.flags, op.f0, (float*)frame_at(op.dst, f), (int64_t)nb * op.Hi * op.Wi, s);
            });
            break;
        case HAVC_OP_BILINEAR2:
            e = launch_bilinear2((const float*)bufptr(n, op.src), (float*)bufptr(n, op.dst), batch, op.Hi, op.Wi, op.Ho, op.Wo, op.f0, s);
            break;
        case HAVC_OP_PREP_LAB_L:
            e = launch_prep_lab_l((const uint8_t*)bufptr(n, op.src), (half_t*)bufptr(n, op.dst), op.dst_cpitch, op.dst_coff,
                                  (int64_t)batch * op.Hi * op.Wi, s, (op.flags & HAVC_F_PRECISE) ? op.dst_cpitch >> 1 : 0);
            break;
        case HAVC_OP_DWCONV7:
            if (op.w_off < 0 || (op.Ci & 7)) return fail(c, HAVC_E_INVALID, "dwconv7 op: weights / channel count");
            e = by_frame(fills(op.src, src_rows * op.src_cpitch) && fills(op.dst, src_rows * op.dst_cpitch), [&](int f, int nb) {
                if (precise)                                       // fp32 weights [49][Kc]
                    return launch_dwconv7_p((const half_t*)frame_at(op.src, f), wptr<float>(n, op.w_off), wptr<float>(n, op.bias_off), (half_t*)frame_at(op.dst, f),
                                            nb, op.Hi, op.Wi, op.Ci, op.src_cpitch, op.src_coff, op.dst_cpitch, op.dst_coff, op.Kc, s);
                return launch_dwconv7((const half_t*)frame_at(op.src, f), wptr<half_t>(n, op.w_off), wptr<float>(n, op.bias_off), (half_t*)frame_at(op.dst, f),
                                      nb, op.Hi, op.Wi, op.Ci, op.src_cpitch, op.src_coff, op.dst_cpitch, op.dst_coff, op.Kc, s);
            });
            break;
        case HAVC_OP_DWCONV7_LN:
            if (op.w_off < 0 || op.scale_off < 0 || op.shift_off < 0 || !dwconv7_ln_supported(op.Ci))
                return fail(c, HAVC_E_INVALID, "dwconv7+layernorm op: weights / gamma / beta / channel count");
            if (precise && !dwconv7_ln_p_supported(op.Ci))         // pair tensors, fp32 weights (round 6)
                return fail(c, HAVC_E_INVALID, "dwconv7+layernorm op: the precise form exists for 192 / 384 / 768 channels");
            e = by_frame(fills(op.src, src_rows * op.src_cpitch) && fills(op.dst, src_rows * op.dst_cpitch), [&](int f, int nb) {
                if (precise)
                    return launch_dwconv7_ln_p((const half_t*)frame_at(op.src, f), wptr<float>(n, op.w_off), wptr<float>(n, op.bias_off), wptr<float>(n, op.scale_off),
                                               wptr<float>(n, op.shift_off), op.f0, (half_t*)frame_at(op.dst, f), nb, op.Hi, op.Wi, op.Ci, op.src_cpitch,
                                               op.src_coff, op.dst_cpitch, op.dst_coff, op.Kc, s);
                return launch_dwconv7_ln((const half_t*)frame_at(op.src, f), wptr<half_t>(n, op.w_off), wptr<float>(n, op.bias_off), wptr<float>(n, op.scale_off),
                                         wptr<float>(n, op.shift_off), op.f0, (half_t*)frame_at(op.dst, f), nb, op.Hi, op.Wi, op.Ci, op.src_cpitch,
                                         op.src_coff, op.dst_cpitch, op.dst_coff, op.Kc, s);
            });
            break;
        case HAVC_OP_FOLD_QUERIES:
            if (op.w_off < 0 || op.Ho < 1 || op.Ho > op.Kc || op.Ho > op.Wi || (op.Ci & 7) || n->bufdesc[op.dst].elem_bytes != 4 ||
                (uint64_t)n->bufdesc[op.dst].elems_per_frame < (uint64_t)2 * op.Ci)
                return fail(c, HAVC_E_INVALID, "fold-queries op: R weights, query count, fp32 [2][Ci] destination");
            e = (precise ? launch_fold_queries_p : launch_fold_queries)((const half_t*)bufptr(n, op.src), op.src_cpitch, op.src_coff, op.Wi, wptr<float>(n, op.w_off),
                                                                        op.Kc, op.Ho, (float*)bufptr(n, op.dst), batch, op.Ci, s);
            break;
        case HAVC_OP_SHUF4_BLUR_AB:
            if ((op.flags & HAVC_F_PRECISE) && op.Ci == 2) {
                // precise plan with the projection fused into the last_shuf conv (round 6): src = its fp32 [Hi*Wi][16][2] output, image and ab map as pairs
                if (op.w_off < 0 || op.bias_off < 0 || op.src2 < 0 || n->bufdesc[op.src].elem_bytes != 4 ||
                    (uint64_t)n->bufdesc[op.src].elems_per_frame < (uint64_t)op.Hi * op.Wi * 32)
                    return fail(c, HAVC_E_INVALID, "shuffle+blur(ab) op, precise: weights, image view, fp32 [Hi*Wi][16][2] source");
                e = by_frame(fills(op.src, src_rows * 32) && fills(op.src2, dst_rows * op.res_cpitch) && fills(op.dst, dst_rows * op.dst_cpitch), [&](int f, int nb) {
                    return launch_shuf4_blur_ab_p((const float*)frame_at(op.src, f), (const half_t*)frame_at(op.src2, f), op.res_cpitch, op.res_coff,
                                                  wptr<float>(n, op.w_off), wptr<float>(n, op.bias_off), (half_t*)frame_at(op.dst, f), op.dst_cpitch, op.dst_coff,
                                                  nb, op.Hi, op.Wi, s);
                });
                break;
            }
            if (op.flags & HAVC_F_PRECISE) {
                // precise form without the fused conv (no plan of the package emits it; the op accepts it): src = the last_shuf conv's pair tensor [Hi][Wi][16 x 256], aux0 = the folded projection (fp32 [2][256] per frame, FOLD_QUERIES)
                if (op.w_off < 0 || op.bias_off < 0 || op.src2 < 0 || op.aux0 < 0 || op.aux0 >= (int)n->bufs.size() || n->bufdesc[op.aux0].elem_bytes != 4 ||
                    (uint64_t)n->bufdesc[op.aux0].elems_per_frame < 512 || n->bufdesc[op.src].elem_bytes != 2 || op.Ci != 16 * 256)
                    return fail(c, HAVC_E_INVALID, "shuffle+blur(ab) op, precise: weights, image view, projection buffer (aux0), 4096-channel pair source");
                e = launch_shuf4_blur_proj_p((const half_t*)bufptr(n, op.src), op.src_cpitch, op.src_coff, (const float*)bufptr(n, op.aux0),
                                             (const half_t*)bufptr(n, op.src2), op.res_cpitch, op.res_coff, wptr<float>(n, op.w_off), wptr<float>(n, op.bias_off),
                                             (half_t*)bufptr(n, op.dst), op.dst_cpitch, op.dst_coff, batch, op.Hi, op.Wi, s);
                break;
            }
            if (op.w_off < 0 || op.bias_off < 0 || op.src2 < 0 || n->bufdesc[op.src].elem_bytes != 4 ||
                (uint64_t)n->bufdesc[op.src].elems_per_frame < (uint64_t)op.Hi * op.Wi * 32)
                return fail(c, HAVC_E_INVALID, "shuffle+blur(ab) op: weights, image view, fp32 [Hi*Wi][16][2] source");
            e = by_frame(fills(op.src, src_rows * 32) && fills(op.src2, dst_rows * op.res_cpitch) && fills(op.dst, dst_rows * op.dst_cpitch), [&](int f, int nb) {
                return launch_shuf4_blur_ab((const float*)frame_at(op.src, f), (const half_t*)frame_at(op.src2, f), op.res_cpitch, op.res_coff,
                                            wptr<float>(n, op.w_off), wptr<float>(n, op.bias_off), (half_t*)frame_at(op.dst, f), op.dst_cpitch, op.dst_coff,
                                            nb, op.Hi, op.Wi, s);
            });
            break;
        case HAVC_OP_LAYERNORM:
            if (op.scale_off < 0 || op.shift_off < 0) return fail(c, HAVC_E_INVALID, "layernorm op: gamma / beta");
            if (!precise && (op.Ci < 1 || op.Ci > 2048)) return fail(c, HAVC_E_INVALID, "layernorm op: 1 <= C <= 2048 (four 8-channel chunks per lane, 64 lanes)");
            e = by_frame(fills(op.src, src_rows * op.src_cpitch) && fills(op.dst, src_rows * op.dst_cpitch), [&](int f, int nb) {
                if (precise)
                    return launch_layernorm_p((const half_t*)frame_at(op.src, f), (half_t*)frame_at(op.dst, f), wptr<float>(n, op.scale_off),
                                              wptr<float>(n, op.shift_off), op.f0, (int64_t)nb * op.Hi * op.Wi, op.Ci, op.src_cpitch, op.src_coff, op.dst_cpitch,
                                              op.dst_coff, (op.flags & HAVC_F_RELU_POST) ? 1 : 0, s);
                return launch_layernorm_c((const half_t*)frame_at(op.src, f), (half_t*)frame_at(op.dst, f), wptr<float>(n, op.scale_off),
                                          wptr<float>(n, op.shift_off), op.f0, (int64_t)nb * op.Hi * op.Wi, op.Ci, op.src_cpitch, op.src_coff,
                                          op.dst_cpitch, op.dst_coff, s, (op.flags & HAVC_F_RELU_POST) ? 1 : 0);
            });
            break;
        case HAVC_OP_MHA:
            if (op.src2 < 0 || op.Ci != op.kh * 32) return fail(c, HAVC_E_INVALID, "mha op: K/V buffer, head dim 32");
            if (!precise && op.Hi <= 128 && op.aux1 >= 0 && op.aux1 < (int)n->bufs.size() && n->bufdesc[op.aux1].elem_bytes == 4) {
                // keys split over blocks (K / V staged in LDS once per block), partial softmax states in the fp32 buffer aux1.  A block of the split kernel
                // holds 128 queries (four waves x two 16-query fragments): more queries run on the one-wave-per-query kernel below, which has no such limit
                if ((size_t)n->bufdesc[op.aux1].elems_per_frame < (size_t)op.kh * mha32_nsplit(op.Ho) * op.Hi * 34)
                    return fail(c, HAVC_E_INVALID, "mha op: partial-state buffer too small");
                e = launch_mha32_split((const half_t*)bufptr(n, op.src), op.src_cpitch, op.src_coff, op.Wi, (const half_t*)bufptr(n, op.src2),
                                       op.res_cpitch, op.res_coff, op.aux0, op.Wo, (half_t*)bufptr(n, op.dst), op.dst_cpitch, op.dst_coff, op.Wi,
                                       (float*)bufptr(n, op.aux1), batch, op.kh, op.Hi, op.Ho, op.f0, s);
                c->stats.launches += 1;
                break;
            }
            e = (precise ? launch_mha32_p : launch_mha32)((const half_t*)bufptr(n, op.src), op.src_cpitch, op.src_coff, op.Wi, (const half_t*)bufptr(n, op.src2),
                                                          op.res_cpitch, op.res_coff, op.aux0, op.Wo, (half_t*)bufptr(n, op.dst), op.dst_cpitch, op.dst_coff, op.Wi,
                                                          batch, op.kh, op.Hi, op.Ho, op.f0, s);
            break;
        case HAVC_OP_PIXSHUF4_BLUR:
            e = by_frame(fills(op.src, src_rows * op.src_cpitch) && fills(op.dst, dst_rows * op.dst_cpitch), [&](int f, int nb) {
                return launch_pixshuf4_blur((const half_t*)frame_at(op.src, f), (half_t*)frame_at(op.dst, f), nb, op.Hi, op.Wi, op.Co, op.src_cpitch,
                                            op.src_coff, op.dst_cpitch, op.dst_coff, s);
            });
            break;
        case HAVC_OP_PREP_DDCOLOR:
            e = launch_prep_ddcolor((const uint8_t*)bufptr(n, op.src), (half_t*)bufptr(n, op.dst), op.dst_cpitch, op.dst_coff,
                                    op.src2 >= 0 ? (half_t*)bufptr(n, op.src2) : nullptr, op.res_cpitch, op.res_coff,
                                    (int64_t)batch * op.Hi * op.Wi, s, (op.flags & HAVC_F_PRECISE) ? 1 : 0);
            break;
        case HAVC_OP_EW: {
            EwArgs a{};
            const bool dual = op.flags & HAVC_EW_DUAL, res = op.flags & HAVC_EW_RES;
            if ((op.Ci & 7) || op.kh < 0 || op.kh > 2 || (res && op.src2 < 0) || (dual && (op.aux0 < 0 || op.aux0 >= (int)n->bufs.size())) ||
                (op.kh == 0 && (op.Hi != op.Ho || op.Wi != op.Wo)) || (op.kh == 2 && (op.kw < 1 || op.Ho * op.kw != op.Hi || op.Wo * op.kw != op.Wi)))
                return fail(c, HAVC_E_INVALID, "ew op: channels / mode / sizes / buffers");
            a.x = (const half_t*)bufptr(n, op.src); a.y = (half_t*)bufptr(n, op.dst);
            a.res = res ? (const half_t*)bufptr(n, op.src2) : nullptr;
            a.y2 = dual ? (half_t*)bufptr(n, op.aux0) : nullptr;
            a.B = batch; a.Hi = op.Hi; a.Wi = op.Wi; a.Ho = op.Ho; a.Wo = op.Wo; a.C8 = op.Ci / 8;
            a.x_cp = op.src_cpitch; a.x_co = op.src_coff; a.y_cp = op.dst_cpitch; a.y_co = op.dst_coff;
            a.r_cp = op.res_cpitch; a.r_co = op.res_coff; a.y2_cp = op.Kc; a.y2_co = op.aux1;
            a.x_fs = (op.flags & HAVC_EW_SRC_BCAST) ? 0 : n->bufdesc[op.src].elems_per_frame;
            a.y_fs = n->bufdesc[op.dst].elems_per_frame;
            a.r_fs = (!res || (op.flags & HAVC_EW_RES_BCAST)) ? 0 : n->bufdesc[op.src2].elems_per_frame;
            a.y2_fs = dual ? n->bufdesc[op.aux0].elems_per_frame : 0;
            a.mode = op.kh; a.factor = op.kw; a.flags = op.flags; a.rh = op.f0; a.rw = op.f1;
            e = launch_ew(a, s);
            break;
        }
        case HAVC_OP_DWCONV:
            if (op.w_off < 0 || (op.Ci & 7) || (op.kh != 3 && op.kh != 5)) return fail(c, HAVC_E_INVALID, "dwconv op: weights / channels / kernel size");
            e = launch_dwconv((const half_t*)bufptr(n, op.src), wptr<half_t>(n, op.w_off), wptr<float>(n, op.bias_off), (half_t*)bufptr(n, op.dst), batch,
                              op.Hi, op.Wi, op.Ci, op.kh, op.src_cpitch, op.src_coff, n->bufdesc[op.src].elems_per_frame, op.dst_cpitch, op.dst_coff,
                              n->bufdesc[op.dst].elems_per_frame, op.Kc, s);
            break;
        case HAVC_OP_CHAN_ATTN: {
            const int heads = op.kh, cc = heads > 0 ? op.Ci / heads : 0, P = op.Hi * op.Wi;
            if (heads < 1 || cc * heads != op.Ci || cc > 256 || (cc & 7) || op.src2 < 0 || op.scale_off < 0 || op.aux0 < 0 || op.aux1 < 0 ||
                op.aux0 >= (int)n->bufs.size() || op.aux1 >= (int)n->bufs.size())
                return fail(c, HAVC_E_INVALID, "channel-attention op: heads / channels per head (<= 256) / buffers");
            const int S = chan_attn_splits(P, heads, cc);
            if ((uint64_t)n->bufdesc[op.aux0].elems_per_frame < (uint64_t)heads * S * cc * cc || (uint64_t)n->bufdesc[op.aux1].elems_per_frame < (uint64_t)S * 2 * op.Ci ||
                (uint64_t)n->bufdesc[op.dst].elems_per_frame < (uint64_t)op.Ci * op.Kc * 8)
                return fail(c, HAVC_E_INVALID, "channel-attention op: scratch / matrix buffers too small");
            e = launch_chan_attn((const half_t*)bufptr(n, op.src), op.src_cpitch, op.src_coff, n->bufdesc[op.src].elems_per_frame,
                                 (const half_t*)bufptr(n, op.src2), op.res_cpitch, op.res_coff, n->bufdesc[op.src2].elems_per_frame, wptr<float>(n, op.scale_off),
                                 (float*)bufptr(n, op.aux0), (float*)bufptr(n, op.aux1), (half_t*)bufptr(n, op.dst), n->bufdesc[op.dst].elems_per_frame,
                                 op.Kc * 8, batch, P, heads, cc, s);
            c->stats.launches += 1;
            break;
        }
        case HAVC_OP_MHA64:
            if (op.Ci != op.kh * 64 || op.Ho < 1 || op.Ho > op.Wi) return fail(c, HAVC_E_INVALID, "mha64 op: head dim 64, live tokens <= tokens per frame");
            e = launch_mha64((const half_t*)bufptr(n, op.src), op.src_cpitch, op.src_coff, op.res_coff, op.aux0, op.Wi, (half_t*)bufptr(n, op.dst),
                             op.dst_cpitch, op.dst_coff, op.Wi, batch, op.kh, op.Ho, op.f0, s);
            break;
        case HAVC_OP_CBAM: {
            const int C = op.Ci, Ch = C / 16;
            const bool dual = op.flags & HAVC_EW_DUAL;
            if (op.w_off < 0 || (C & 15) || op.aux0 < 0 || op.aux1 < 0 || (dual && op.src2 < 0) || (uint64_t)n->bufdesc[op.aux0].elems_per_frame != 3 * (uint64_t)C ||
                (uint64_t)n->bufdesc[op.aux1].elems_per_frame < (uint64_t)op.Hi * op.Wi * 2)
                return fail(c, HAVC_E_INVALID, "cbam op: weights / channels / scratch buffers");
            const float* w1 = wptr<float>(n, op.w_off);
            const float *b1 = w1 + (size_t)Ch * C, *w2 = b1 + Ch, *b2 = w2 + (size_t)C * Ch, *w7 = b2 + C, *b7 = w7 + 98;
            e = launch_cbam((const half_t*)bufptr(n, op.src), op.src_cpitch, op.src_coff, n->bufdesc[op.src].elems_per_frame, batch, op.Hi, op.Wi, C, w1, b1,
                            w2, b2, w7, b7, (float*)bufptr(n, op.aux0), (float*)bufptr(n, op.aux1), (half_t*)bufptr(n, op.dst), op.dst_cpitch, op.dst_coff,
                            n->bufdesc[op.dst].elems_per_frame, dual ? (half_t*)bufptr(n, op.src2) : nullptr, op.res_cpitch, op.res_coff,
                            dual ? n->bufdesc[op.src2].elems_per_frame : 0, s);
            c->stats.launches += 3;
            break;
        }
        case HAVC_OP_GRU:
            if (op.src2 < 0 || n->bufdesc[op.src2].elem_bytes != 4 || n->bufdesc[op.dst].elem_bytes != 4 || op.Co < 1)
                return fail(c, HAVC_E_INVALID, "gru op: fp32 planar hidden buffers");
            e = launch_gru((const half_t*)bufptr(n, op.src), op.src_cpitch, op.src_coff, n->bufdesc[op.src].elems_per_frame, (const float*)bufptr(n, op.src2),
                           (float*)bufptr(n, op.dst), batch, op.Hi * op.Wi, op.Co, s);
            break;
        case HAVC_OP_PLANAR_IN:
            if (n->bufdesc[op.src].elem_bytes != 4 || (op.Co & 7) || op.Ci > op.Co) return fail(c, HAVC_E_INVALID, "planar-in op: fp32 source, Ci <= Co, Co % 8 == 0");
            e = launch_planar_in((const float*)bufptr(n, op.src), n->bufdesc[op.src].elems_per_frame, (half_t*)bufptr(n, op.dst), op.dst_cpitch, op.dst_coff,
                                 n->bufdesc[op.dst].elems_per_frame, batch, op.Hi * op.Wi, op.Ci, op.Co, op.flags & 1, (op.flags & 2) ? 1 : 0, s);
            break;
        case HAVC_OP_CMN_DECODER_IN:
            if (op.src2 < 0 || op.src2 >= (int)n->bufs.size() || op.aux0 < 0 || op.aux0 >= (int)n->bufs.size() || op.aux1 < 0 || op.aux1 >= (int)n->bufs.size() ||
                n->bufdesc[op.src2].elem_bytes != 4 || n->bufdesc[op.aux0].elem_bytes != 4 || n->bufdesc[op.src].elem_bytes != 2 ||
                n->bufdesc[op.aux1].elem_bytes != 2 || n->bufdesc[op.aux1].elems_per_frame != n->bufdesc[op.dst].elems_per_frame || op.kh < 8 || op.kw < 8 ||
                op.Co != op.Ci + op.kh + op.kw || op.dst_coff + op.Co > op.dst_cpitch)
                return fail(c, HAVC_E_INVALID, "decoder-in op: fp16 features, fp32 planar readout (kh channels) and hidden (kw), twin destination buffers, Co = Ci + kh + kw");
            e = launch_cmn_decoder_in((const half_t*)bufptr(n, op.src), op.src_cpitch, op.src_coff, (const float*)bufptr(n, op.src2), n->bufdesc[op.src2].elems_per_frame,
                                      (const float*)bufptr(n, op.aux0), n->bufdesc[op.aux0].elems_per_frame, (half_t*)bufptr(n, op.dst), (half_t*)bufptr(n, op.aux1),
                                      op.dst_cpitch, op.dst_coff, n->bufdesc[op.dst].elems_per_frame, batch, op.Hi * op.Wi, op.Ci, op.kh, op.kw, s);
            break;
        case HAVC_OP_PLANAR_OUT:
            if (n->bufdesc[op.dst].elem_bytes != 4 || op.kh < 0 || op.kh > 3) return fail(c, HAVC_E_INVALID, "planar-out op: fp32 destination, activation 0..3");
            e = launch_planar_out((const half_t*)bufptr(n, op.src), op.src_cpitch, op.src_coff, n->bufdesc[op.src].elems_per_frame, (float*)bufptr(n, op.dst),
                                  n->bufdesc[op.dst].elems_per_frame, batch, op.Hi * op.Wi, op.Ci, op.kh, s);
            break;
        case HAVC_OP_SRCREF_ATTN: {
            const int nb = (int)n->bufs.size();
            const int Tr = op.kw > 0 ? op.kw : batch, nk = op.Ho * op.Wo;
            if (op.src2 < 0 || op.aux0 < 0 || op.aux0 >= nb || op.aux1 < 0 || op.aux1 >= nb || !srcref_attention_supported(op.kh, op.Ci) || nk < 1 ||
                op.src_coff + op.Ci > op.src_cpitch || op.dst_coff + op.Ci > op.dst_cpitch || op.res_coff + op.kh > op.res_cpitch)
                return fail(c, HAVC_E_INVALID, "source-reference attention op: query / key / value buffers, 64 key and 512 value channels");
            const uint64_t q_fs = n->bufdesc[op.src2].elems_per_frame, k_fs = n->bufdesc[op.aux0].elems_per_frame, v_fs = n->bufdesc[op.aux1].elems_per_frame;
            const uint64_t x_fs = n->bufdesc[op.src].elems_per_frame, o_fs = n->bufdesc[op.dst].elems_per_frame, nq = (uint64_t)op.Hi * op.Wi;
            // the net's own allocations hold max_batch frames; a bound buffer (the reference ring) is the caller's to size
            const bool own_kv = n->bound.empty() || (!n->bound[op.aux0] && !n->bound[op.aux1]);
            if (n->bufdesc[op.src2].elem_bytes != 2 || n->bufdesc[op.aux0].elem_bytes != 2 || n->bufdesc[op.aux1].elem_bytes != 2 || q_fs < nq * op.res_cpitch ||
                x_fs < nq * op.src_cpitch || o_fs < nq * op.dst_cpitch || k_fs < (uint64_t)nk * op.kh || (op.Kc & 63) || op.Kc < nk ||
                v_fs < (uint64_t)op.Ci * op.Kc || (own_kv && Tr > n->max_batch))
                return fail(c, HAVC_E_INVALID, "source-reference attention op: buffer sizes / value pitch (Kc % 64 == 0, Kc >= keys per frame) / reference frames");
            e = launch_srcref_attention((const half_t*)bufptr(n, op.src2), op.res_cpitch, op.res_coff, (int64_t)q_fs, (const half_t*)bufptr(n, op.aux0), (int64_t)k_fs,
                                        (const half_t*)bufptr(n, op.aux1), op.Kc, (int64_t)v_fs, (const half_t*)bufptr(n, op.src), op.src_cpitch, op.src_coff,
                                        (int64_t)x_fs, (half_t*)bufptr(n, op.dst), op.dst_cpitch, op.dst_coff, (int64_t)o_fs, batch, (int)nq, Tr, nk, op.f0, s);
            break;
        }
        case HAVC_OP_TSTACK:
            if ((op.Ci & 7) || op.Co != 3 * op.Ci || op.src_coff + op.Ci > op.src_cpitch || op.dst_coff + op.Co > op.dst_cpitch ||
                (uint64_t)n->bufdesc[op.src].elems_per_frame < (uint64_t)op.Hi * op.Wi * op.src_cpitch ||
                (uint64_t)n->bufdesc[op.dst].elems_per_frame < (uint64_t)op.Hi * op.Wi * op.dst_cpitch || op.src == op.dst)
                return fail(c, HAVC_E_INVALID, "temporal-stack op: Co = 3 Ci, views inside their buffers, distinct buffers");
            e = launch_tstack((const half_t*)bufptr(n, op.src), (half_t*)bufptr(n, op.dst), batch, (int64_t)op.Hi * op.Wi, op.Ci, op.src_cpitch, op.src_coff,
                              n->bufdesc[op.src].elems_per_frame, op.dst_cpitch, op.dst_coff, n->bufdesc[op.dst].elems_per_frame, s);
            break;
        case HAVC_OP_ELU:
            if ((op.Ci & 7) || op.src_coff + op.Ci > op.src_cpitch || op.dst_coff + op.Ci > op.dst_cpitch ||
                (uint64_t)n->bufdesc[op.src].elems_per_frame < (uint64_t)op.Hi * op.Wi * op.src_cpitch ||
                (uint64_t)n->bufdesc[op.dst].elems_per_frame < (uint64_t)op.Hi * op.Wi * op.dst_cpitch)
                return fail(c, HAVC_E_INVALID, "elu op: views inside their buffers");
            e = launch_elu((const half_t*)bufptr(n, op.src), (half_t*)bufptr(n, op.dst), batch, (int64_t)op.Hi * op.Wi, op.Ci, op.src_cpitch, op.src_coff,
                           n->bufdesc[op.src].elems_per_frame, op.dst_cpitch, op.dst_coff, n->bufdesc[op.dst].elems_per_frame, s);
            break;
        case HAVC_OP_PREP_REMASTER: {
            const int refs = op.flags & 1, padv = refs ? 0 : 2;
            if (op.Hi < 1 || op.Wi < 1 || op.Ho != op.Hi + padv || op.Wo != op.Wi + padv || n->bufdesc[op.src].elem_bytes != 1 ||
                (uint64_t)n->bufdesc[op.src].elems_per_frame != (uint64_t)op.Hi * op.Wi * 3 || op.dst_coff + 8 > op.dst_cpitch ||
                (uint64_t)n->bufdesc[op.dst].elems_per_frame < (uint64_t)op.Ho * op.Wo * op.dst_cpitch)
                return fail(c, HAVC_E_INVALID, "remaster prep op: u8 RGB source of Hi x Wi, destination of Hi + 2 x Wi + 2 (frames) or Hi x Wi (references)");
            e = launch_prep_remaster((const uint8_t*)bufptr(n, op.src), (half_t*)bufptr(n, op.dst), batch, op.Hi, op.Wi, op.Ho, op.Wo, refs, op.dst_cpitch, op.dst_coff,
                                     n->bufdesc[op.dst].elems_per_frame, s);
            break;
        }
        case HAVC_OP_REMASTER_OUT: {
            const uint64_t P = (uint64_t)op.Hi * op.Wi;
            const bool tap = op.aux0 >= 0;
            if (op.src2 < 0 || n->bufdesc[op.src2].elem_bytes != 1 || (uint64_t)n->bufdesc[op.src2].elems_per_frame != P * 3 || n->bufdesc[op.dst].elem_bytes != 1 ||
                (uint64_t)n->bufdesc[op.dst].elems_per_frame != P * 3 || op.src_coff + 2 > op.src_cpitch ||
                (uint64_t)n->bufdesc[op.src].elems_per_frame < P * op.src_cpitch ||
                (tap && (op.aux0 >= (int)n->bufs.size() || n->bufdesc[op.aux0].elem_bytes != 4 || (uint64_t)n->bufdesc[op.aux0].elems_per_frame != P * 2)))
                return fail(c, HAVC_E_INVALID, "remaster output op: u8 RGB input (src2) and output of Hi x Wi, optional fp32 [Hi * Wi][2] tap buffer (aux0)");
            e = launch_remaster_out((const half_t*)bufptr(n, op.src), op.src_cpitch, op.src_coff, n->bufdesc[op.src].elems_per_frame, (const uint8_t*)bufptr(n, op.src2),
                                    (uint8_t*)bufptr(n, op.dst), tap ? (float*)bufptr(n, op.aux0) : nullptr, batch, (int64_t)P, s);
            break;
        }
        default:
            return fail(c, HAVC_E_INVALID, "unknown op type");
    }
    c->stats.launches += 1;
    if (e) return hip_fail(c, (hipError_t)e, "kernel launch");
    if (timed) HIP_TRY(c, hipEventRecord(evp.second, s));
    return HAVC_OK;
}

}  // namespace

int run_ops_locked(havc_net* n, int first, int count, int batch) {
    if (batch < 1 || batch > n->max_batch) return fail(n->ctx, HAVC_E_INVALID, "batch out of range");
    if (first < 0 || count < 0 || first + count > (int)n->ops.size()) return fail(n->ctx, HAVC_E_INVALID, "op range");
    havc_ctx* c = n->ctx;
    const bool check = c->range_check;
    if (check && !n->range_ready) return fail(c, HAVC_E_INVALID, "range check: enable it before the net is created (its buffers must start zero-filled)");
    hipStream_t s = c->cur ? c->cur : c->stream;
    stream_jitter(s);
    for (int i = first; i < first + count; ++i) {
        int rc = run_op(n, n->ops[i], batch);
        if (rc) return rc;
        if (check) {
            const havc_op& op = n->ops[i];
            const havc_buf& bd = n->bufdesc[op.dst];
            int e = launch_range_stats(bufptr(n, op.dst), bd.elem_bytes, (int64_t)batch * bd.elems_per_frame, n->d_range + 4 * (size_t)i, s);
            if (e) return hip_fail(c, (hipError_t)e, "range-check kernel");
        }
    }
    if (check) {
        std::vector<unsigned> host((size_t)n->ops.size() * 4);
        HIP_TRY(c, hipStreamSynchronize(s));
        HIP_TRY(c, hipMemcpy(host.data(), n->d_range, host.size() * 4, hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemset(n->d_range, 0, host.size() * 4));
        n->range_absmax.assign(n->ops.size(), 0.f);
        n->range_bad.assign(n->ops.size(), 0);
        int first_bad = -1;
        for (size_t i = 0; i < n->ops.size(); ++i) {
            float f;
            memcpy(&f, &host[4 * i], 4);
            unsigned long long b;
            memcpy(&b, &host[4 * i + 2], 8);
            n->range_absmax[i] = f;
            n->range_bad[i] = (int64_t)b;
            if (b && first_bad < 0) first_bad = (int)i;
        }
        if (first_bad >= 0) {
            char msg[256];
            snprintf(msg, sizeof msg, "range check: op %d (type %d, tag %d) left %lld non-finite values in buffer %d -- an activation exceeded the fp16 range "
                     "(65504); largest finite magnitude there %.4g", first_bad, n->ops[first_bad].type, n->ops[first_bad].tag, (long long)n->range_bad[first_bad],
                     n->ops[first_bad].dst, (double)n->range_absmax[first_bad]);
            return fail(c, HAVC_E_RANGE, msg);
        }
    }
    return HAVC_OK;
}

int net_run_rgb8_locked(havc_net* n, const uint8_t* d_in, uint8_t* d_out, int batch, hipStream_t on) {
    n->in_override = d_in;
    n->out_override = d_out;
    n->ctx->cur = on;
    int rc = run_ops_locked(n, 0, (int)n->ops.size(), batch);
    n->ctx->cur = nullptr;
    n->in_override = nullptr;
    n->out_override = nullptr;
    if (rc == HAVC_OK) {
        n->ctx->stats.total_flops += n->flops_per_frame * batch;
    }
    return rc;
}

extern "C" {

int havc_weights_load(havc_ctx* c, const void* blob, size_t nbytes, havc_weights** out) {
    if (!c || !blob || !out || nbytes == 0) return fail(c, HAVC_E_INVALID, "weights_load: bad args");
    std::lock_guard<std::mutex> lk(c->mu);
    SetupLock setup;
    HIP_TRY(c, hipSetDevice(c->dev));
    uint8_t* d = nullptr;
    HIP_TRY(c, hipMalloc((void**)&d, nbytes));
    hipError_t e = hipMemcpy(d, blob, nbytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d); return hip_fail(c, e, "weights H2D"); }
    c->stats.bytes_resident += (int64_t)nbytes;
    *out = new havc_weights{c, d, nbytes};
    return HAVC_OK;
}

void havc_weights_free(havc_weights* w) {
    if (!w) return;
    std::lock_guard<std::mutex> lk(w->ctx->mu);
    SetupLock setup;
    (void)sync_streams(w->ctx);
    (void)hipFree(w->d_blob);
    w->ctx->stats.bytes_resident -= (int64_t)w->nbytes;
    delete w;
}

int havc_conv_fast_div(uint32_t divisor, const uint32_t* dividends, uint32_t* quotients, int64_t count) {
    if (divisor < 1 || divisor > 0x80000000u || count < 0 || (count > 0 && (!dividends || !quotients))) return HAVC_E_INVALID;
    const FastDiv fd = fast_div_make(divisor);
    for (int64_t i = 0; i < count; ++i) quotients[i] = fast_div(dividends[i], fd);
    return HAVC_OK;
}

int havc_net_create(havc_ctx* c, havc_weights* w, const havc_op* ops, int n_ops, const havc_buf* bufs, int n_bufs,
                    int in_buf, int out_buf, int S, int max_batch, havc_net** out) {
    if (!c || !w || !ops || !bufs || !out || n_ops <= 0 || n_bufs <= 0 || max_batch < 1)
        return fail(c, HAVC_E_INVALID, "net_create: bad args");
    if (in_buf < 0 || in_buf >= n_bufs || out_buf < 0 || out_buf >= n_bufs) return fail(c, HAVC_E_INVALID, "net_create: in/out buffer id");
    std::lock_guard<std::mutex> lk(c->mu);
    SetupLock setup;
    HIP_TRY(c, hipSetDevice(c->dev));
    for (int i = 0; i < n_ops; ++i) {
        const havc_op& o = ops[i];
        auto bad = [&](int id) { return id < -1 || id >= n_bufs; };
        if (bad(o.src) || bad(o.src2) || bad(o.dst) || o.src < 0 || o.dst < 0) return fail(c, HAVC_E_INVALID, "net_create: op buffer id out of range");
        if (o.type == HAVC_OP_ATTENTION && (o.aux1 < 0 || o.aux1 >= n_bufs)) return fail(c, HAVC_E_INVALID, "net_create: attention V^T buffer id");
        if (o.type == HAVC_OP_CONV && (o.flags & (HAVC_F_RESIDUAL | HAVC_F_W_FROM_BUF)) && o.src2 < 0)
            return fail(c, HAVC_E_INVALID, "net_create: conv op with RESIDUAL / W_FROM_BUF needs a buffer in src2");
        for (int64_t off : {o.w_off, o.bias_off, o.scale_off, o.shift_off})
            if (off >= 0 && ((size_t)off >= w->nbytes || (off & 15))) return fail(c, HAVC_E_INVALID, "net_create: weight offset out of range / unaligned");
    }
    havc_net* n = new havc_net();
    n->ctx = c; n->w = w;
    n->ops.assign(ops, ops + n_ops);
    n->bufdesc.assign(bufs, bufs + n_bufs);
    n->bufs.assign(n_bufs, nullptr);
    n->in_buf = in_buf; n->out_buf = out_buf; n->S = S; n->max_batch = max_batch;
    for (int i = 0; i < n_ops; ++i) n->flops_per_frame += (double)ops[i].flops;
    for (int i = 0; i < n_ops; ++i)
        if (ops[i].tag == 1) { n->tail_first = i; break; }
    size_t ktab_bytes = 0;
    // ---- per-conv K tables: chunk kidx -> (byte offset from the tap-0 pixel, tap displacement) -----------------
    // K order (must match plan.py pack_conv): main segment = chunks [0, C8a) of every tap, then chunks [C8a, C8), each
    // segment padded to a multiple of 8 chunks.  A main segment with C8a % 8 == 0 is CHANNEL-GROUP MAJOR (group of 8
    // chunks, then tap): the 9 taps of one 128-byte line group are consecutive stages -> re-reads hit L1/L2.
    {
        std::vector<int2> host;
        n->ktab_off.assign(n_ops, -1);
        n->k_half_empty.assign(n_ops, 0);
        for (int i = 0; i < n_ops; ++i) {
            const havc_op& o = ops[i];
            if (o.type != HAVC_OP_CONV) continue;
            n->ktab_off[i] = (int64_t)host.size();
            const int C8 = o.Ci / 8, C8a = (o.aux1 > 0 && o.aux1 < C8) ? o.aux1 : C8;
            const size_t start = host.size();
            auto emit = [&](int kh, int kw, int c) {
                int2 e;
                e.x = ((kh * o.dil * o.Wi + kw * o.dil) * o.src_cpitch + c * 8) * 2;
                e.y = (int)(((unsigned)(kh * o.dil) & 0xffffu) | ((unsigned)(kw * o.dil) << 16));
                host.push_back(e);
            };
            auto emit_seg = [&](int c_lo, int c_hi) {
                if (c_hi <= c_lo) return;
                if (c_lo == 0 && c_hi % 8 == 0) {
                    for (int g = 0; g < c_hi / 8; ++g)
                        for (int kh = 0; kh < o.kh; ++kh)
                            for (int kw = 0; kw < o.kw; ++kw)
                                for (int c = 0; c < 8; ++c) emit(kh, kw, g * 8 + c);
                } else {
                    for (int kh = 0; kh < o.kh; ++kh)
                        for (int kw = 0; kw < o.kw; ++kw)
                            for (int c = c_lo; c < c_hi; ++c) emit(kh, kw, c);
                }
                while ((host.size() - start) % 8) host.push_back(int2{0, HAVC_KTAB_PAD_DH});
            };
            emit_seg(0, C8a);
            emit_seg(C8a, C8);
            if (o.flags & HAVC_F_PRECISE) {
                // precise conv: the K walk above three times -- x_hi (x 2^11 w_hi), x_hi (x 2^11 w_lo), x_lo (x w_hi; the lo plane of a pixel
                // sits src_cpitch / 2 elements = src_cpitch BYTES behind its hi plane) -- matching plan.py pack_conv(precise=True)
                const size_t len = host.size() - start;
                for (int rep = 1; rep < 3; ++rep)
                    for (size_t k = 0; k < len; ++k) {
                        int2 e = host[start + k];
                        if (rep == 2 && (short)(e.y & 0xffff) != HAVC_KTAB_PAD_DH) e.x += o.src_cpitch;
                        host.push_back(e);
                    }
            }
            if ((int)(host.size() - start) != o.Kc) {
                delete n;
                return fail(c, HAVC_E_INVALID, "net_create: conv op Kc does not match its K layout (Ci, kh, kw, aux1)");
            }
            // The last stage (8 chunks) of a K table whose chunks 4..7 are all pad entries: those chunks bring zero pixels against zero-padded weight
            // columns, and the pipelined kernels skip that K half (the 259-channel convs: a remainder segment of 9 chunks padded to 16).  Left off for
            // precise ops and for weights that come from an activation buffer (nothing pads those with zeros but the producer).
            if (o.Kc >= 8 && !(o.Kc & 7) && !(o.flags & (HAVC_F_PRECISE | HAVC_F_W_FROM_BUF))) {
                bool empty = true;
                for (int k = 4; k < 8; ++k) empty = empty && (short)(host[start + o.Kc - 8 + k].y & 0xffff) == HAVC_KTAB_PAD_DH;
                n->k_half_empty[i] = empty;
            }
        }
        if (!host.empty()) {
            hipError_t e = hipMalloc((void**)&n->d_ktab, host.size() * sizeof(int2));
            if (e == hipSuccess) e = hipMemcpy(n->d_ktab, host.data(), host.size() * sizeof(int2), hipMemcpyHostToDevice);
            if (e != hipSuccess) {
                if (n->d_ktab) (void)hipFree(n->d_ktab);
                delete n;
                return hip_fail(c, e, "K table upload");
            }
            ktab_bytes = host.size() * sizeof(int2);
            c->stats.bytes_resident += (int64_t)ktab_bytes;
        }
    }
    for (int i = 0; i < n_bufs; ++i) {
        // +256 B tail so a predicated-off 16-byte vector address is never formed past the allocation
        size_t nb = (size_t)bufs[i].elems_per_frame * bufs[i].elem_bytes * max_batch + 256;
        hipError_t e = hipMalloc(&n->bufs[i], nb);
        if (e == hipSuccess && (bufs[i].zero_init || c->range_check)) e = hipMemset(n->bufs[i], 0, nb);
        if (e != hipSuccess) {
            for (int k = 0; k <= i; ++k) {
                if (!n->bufs[k]) continue;
                (void)hipFree(n->bufs[k]);
                if (k < i) c->stats.bytes_resident -= (int64_t)((size_t)bufs[k].elems_per_frame * bufs[k].elem_bytes * max_batch + 256);
            }
            if (n->d_ktab) {
                (void)hipFree(n->d_ktab);
                c->stats.bytes_resident -= (int64_t)ktab_bytes;
            }
            delete n;
            return hip_fail(c, e, "activation buffer allocation");
        }
        c->stats.bytes_resident += (int64_t)nb;
    }
    if (c->range_check) {
        if (hipMalloc((void**)&n->d_range, (size_t)n_ops * 16) != hipSuccess || hipMemset(n->d_range, 0, (size_t)n_ops * 16) != hipSuccess)
            return fail(c, HAVC_E_HIP, "range-check buffer allocation");
        n->range_ready = true;
    }
    *out = n;
    return HAVC_OK;
}

void havc_net_free(havc_net* n) {
    if (!n) return;
    std::lock_guard<std::mutex> lk(n->ctx->mu);
    SetupLock setup;
    (void)sync_streams(n->ctx);
    if (n->d_ktab) {
        (void)hipFree(n->d_ktab);
        size_t chunks = 0;
        for (const havc_op& o : n->ops) if (o.type == HAVC_OP_CONV) chunks += (size_t)o.Kc;
        n->ctx->stats.bytes_resident -= (int64_t)(chunks * sizeof(int2));
    }
    if (n->d_range) (void)hipFree(n->d_range);
    for (size_t i = 0; i < n->bufs.size(); ++i) {
        if (n->bufs[i]) (void)hipFree(n->bufs[i]);
        n->ctx->stats.bytes_resident -= (int64_t)((size_t)n->bufdesc[i].elems_per_frame * n->bufdesc[i].elem_bytes * n->max_batch + 256);
    }
    delete n;
}

int havc_net_run_rgb8(havc_net* n, const uint8_t* d_in, uint8_t* d_out, int batch) {
    if (!n || !d_in || !d_out) return HAVC_E_INVALID;
    havc_ctx* c = n->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, hipSetDevice(c->dev));
    Timer t(c);
    int rc = net_run_rgb8_locked(n, d_in, d_out, batch);
    if (rc) return rc;
    c->stats.frames += batch;
    return t.finish();
}

int havc_net_upload(havc_net* n, int buf, const void* host, size_t nbytes) {
    if (!n || buf < 0 || buf >= (int)n->bufs.size() || !host) return HAVC_E_INVALID;
    havc_ctx* c = n->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    if (nbytes > (size_t)n->bufdesc[buf].elems_per_frame * n->bufdesc[buf].elem_bytes * n->max_batch) return fail(c, HAVC_E_INVALID, "upload too large");
    HIP_TRY(c, hipSetDevice(c->dev));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(n->bufs[buf], host, nbytes, hipMemcpyHostToDevice));
    return HAVC_OK;
}

int havc_net_download(havc_net* n, int buf, void* host, size_t nbytes) {
    if (!n || buf < 0 || buf >= (int)n->bufs.size() || !host) return HAVC_E_INVALID;
    havc_ctx* c = n->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    if (nbytes > (size_t)n->bufdesc[buf].elems_per_frame * n->bufdesc[buf].elem_bytes * n->max_batch) return fail(c, HAVC_E_INVALID, "download too large");
    HIP_TRY(c, hipSetDevice(c->dev));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(host, n->bufs[buf], nbytes, hipMemcpyDeviceToHost));
    return HAVC_OK;
}

int havc_range_check_enable(havc_ctx* c, int enable) {
    if (!c) return HAVC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    c->range_check = enable != 0;
    return HAVC_OK;
}

int havc_net_range_stats(havc_net* n, float* abs_max, int64_t* non_finite, int n_ops) {
    if (!n || !abs_max || !non_finite || n_ops != (int)n->ops.size()) return HAVC_E_INVALID;
    std::lock_guard<std::mutex> lk(n->ctx->mu);
    if (n->range_absmax.size() != n->ops.size()) return fail(n->ctx, HAVC_E_INVALID, "range stats: no checked run of this net yet");
    for (int i = 0; i < n_ops; ++i) { abs_max[i] = n->range_absmax[i]; non_finite[i] = n->range_bad[i]; }
    return HAVC_OK;
}

int havc_net_bind(havc_net* n, int buf, void* device_ptr) {
    if (!n || buf < 0 || buf >= (int)n->bufs.size()) return HAVC_E_INVALID;
    std::lock_guard<std::mutex> lk(n->ctx->mu);
    if (n->bound.empty()) n->bound.assign(n->bufs.size(), nullptr);
    n->bound[buf] = device_ptr;
    return HAVC_OK;
}

int havc_net_enqueue_ops(havc_net* n, int first_op, int n_ops, int batch) {
    if (!n) return HAVC_E_INVALID;
    havc_ctx* c = n->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, hipSetDevice(c->dev));
    return run_ops_locked(n, first_op, n_ops, batch);
}

int havc_net_run_ops(havc_net* n, int first_op, int n_ops, int batch) {
    if (!n) return HAVC_E_INVALID;
    havc_ctx* c = n->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, hipSetDevice(c->dev));
    Timer t(c);
    int rc = run_ops_locked(n, first_op, n_ops, batch);
    if (rc) return rc;
    return t.finish();
}

// Per-op choice of the conv tile configuration by measurement.  Every candidate computes the same bytes (same packed K order,
// same MFMA sequence per output), so tuning never changes a result; ops with the same shape signature are tuned once.
// tile configurations an op may run with (all produce the same bytes); empty = the op has exactly one legal configuration
static std::vector<int> tune_candidates(const havc_op& op) {
    if (op.type != HAVC_OP_CONV || (op.flags & (HAVC_F_PS_BLUR | HAVC_F_FUSE_RGB8 | HAVC_F_OUT_RGB8 | HAVC_F_FUSE_PROJ))) return {};
    if (HAVC_F_SPLITK_COUNT(op.flags) > 1) {                               // split-K: the plain pipelined tiles (same bytes for a given count)
        std::vector<int> sk = {0};
        if (op.Npad % 256 == 0 || op.Npad % 256 >= 192) for (int k : {60, 71, 90, 91, 96, 97}) sk.push_back(k);
        for (int k : {70, 72, 93, 95, 98}) sk.push_back(k);
        if (op.Npad <= 192) { sk.push_back(99); sk.push_back(92); }
        return sk;
    }
    std::vector<int> cand = {0};
    if (op.Npad <= 16) return cand;                                        // thin N: the 128x16 kernel only
    if (op.flags & HAVC_F_PRECISE) {
        // precise convs: the PIPELINED tile geometries instantiated with the precise epilogue, and nothing else: nothing is rounded to fp16
        // before the hi / lo split, so the bytes follow the fp32 accumulation order -- the pipelined tiles share one K walk, the register-staged
        // kernels (cfg 1, 2, 3, 7) and whatever the heuristic (cfg 0) picks per batch size do not.  The heuristic stays only where no pipelined tile fits.
        std::vector<int> pc;
        if (op.Npad % 256 == 0 || op.Npad % 256 >= 192) { for (int k : {60, 71, 96}) pc.push_back(k); }
        if (op.Npad == 272) pc.push_back(61);
        if (op.Npad % 128 == 0 || op.Npad % 128 >= 96 || op.Npad > 256) { for (int k : {70, 72, 98}) pc.push_back(k); }
        if (op.Npad % 64 == 0 && op.Npad <= 192) { pc.push_back(99); pc.push_back(92); }
        if (pc.empty()) { for (int k : {72, 92}) pc.push_back(k); }
        return pc;
    }
    // column tiles of 256 / 128 channels: also when the last tile is >= 75 % full (ConvNeXt pwconv2 at stage 0, 768 -> 192: the
    // 256 x 256 tile beats every narrower one by 30 %)
    if (op.Npad % 256 == 0 || op.Npad % 256 >= 192) { for (int k : {60, 71, 90, 91, 96, 97}) cand.push_back(k); }
    if (op.Npad == 272) cand.push_back(61);                                // (launch_pipe<.., EXTRA = 1> takes exactly 256 + 16 columns)
    // 128-wide tiles for every wide layer: the DynamicUnetDeep (artistic) channel counts 304 / 320 / 672 / 1344 fit no tile exactly and
    // a partly empty last tile on the pipelined kernel still beats the register-staged kernels there
    if (op.Npad % 128 == 0 || op.Npad % 128 >= 96 || op.Npad > 256) { for (int k : {70, 72, 93, 95, 98}) cand.push_back(k); }
    if (op.Npad % 64 == 0 && op.Npad <= 192) { cand.push_back(99); cand.push_back(92); }      // 64-wide pipelined tiles (ResNet layer1, stem)
    for (int k : {1, 2, 3, 7}) cand.push_back(k);                          // register-staged 128x128 / 128x64 / 64x64 / 64x128
    return cand;
}

int havc_net_set_cfg(havc_net* n, int op_index, int cfg) {
    if (!n || op_index < 0 || op_index >= (int)n->ops.size()) return HAVC_E_INVALID;
    const std::vector<int> cand = tune_candidates(n->ops[op_index]);
    if (std::find(cand.begin(), cand.end(), cfg) == cand.end())
        return cfg == 0 ? HAVC_OK : fail(n->ctx, HAVC_E_INVALID, "net_set_cfg: not a legal tile configuration for this op");
    std::lock_guard<std::mutex> lk(n->ctx->mu);
    n->ops[op_index].reserved = cfg;
    return HAVC_OK;
}

int havc_net_autotune(havc_net* n, int batch, int* n_changed) {
    if (!n) return HAVC_E_INVALID;
    havc_ctx* c = n->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    // The process-wide set-up mutex is taken PER TRIAL (round 5): a trial launch is the first launch of most kernel instantiations, which is
    // what the mutex serialises -- but held over the whole tuning run (seconds) it stalled every other thread's havc_dev_alloc / scratch regrowth.
    HIP_TRY(c, hipSetDevice(c->dev));
    if (batch < 1 || batch > n->max_batch) return fail(c, HAVC_E_INVALID, "autotune: batch out of range");
    HIP_TRY(c, sync_streams(c));
    hipEvent_t e0, e1;
    HIP_TRY(c, hipEventCreate(&e0));
    HIP_TRY(c, hipEventCreate(&e1));
    std::map<std::vector<int64_t>, int> seen;
    int changed = 0, rc = HAVC_OK;
    const havc_stats keep = c->stats;
    for (size_t i = 0; i < n->ops.size() && rc == HAVC_OK; ++i) {
        havc_op& op = n->ops[i];
        if (tune_candidates(op).empty()) continue;                          // not a conv, or one legal config
        const std::vector<int64_t> sig = {op.flags, op.Hi, op.Wi, op.Ci, op.Ho, op.Wo, op.Co, op.kh, op.kw, op.stride, op.pad, op.dil, op.Kc,
                                          op.Npad, op.src_cpitch, op.dst_cpitch, op.res_cpitch, op.aux1, op.out_step};
        auto it = seen.find(sig);
        if (it != seen.end()) { if (op.reserved != it->second) { op.reserved = it->second; ++changed; } continue; }
        const std::vector<int> cand = tune_candidates(op);
        const int before = op.reserved;
        int best = before;
        float best_ms = 1e30f;
        for (int cfg : cand) {
            SetupLock setup;
            op.reserved = cfg;
            float tot = 0.f;
            bool ok = true;
            for (int rep = 0; rep < 4 && ok; ++rep) {                      // rep 0 = warm-up
                if (hipEventRecord(e0, c->stream) != hipSuccess) { ok = false; break; }
                if (run_op(n, op, batch) != HAVC_OK) { ok = false; (void)hipGetLastError(); break; }
                if (hipEventRecord(e1, c->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess) { ok = false; break; }
                float ms = 0.f;
                if (hipEventElapsedTime(&ms, e0, e1) != hipSuccess) { ok = false; break; }
                if (rep) tot += ms;
            }
            if (ok && (best_ms > 1e29f || tot < best_ms * 0.98f)) { best_ms = tot; best = cfg; }   // 2 % hysteresis towards earlier candidates
        }
        op.reserved = best;
        seen[sig] = best;
        if (best != before) ++changed;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    c->stats = keep;
    c->err.clear();
    if (n_changed) *n_changed = changed;
    return rc;
}

int havc_net_get_cfg(havc_net* n, int op_index) {
    if (!n || op_index < 0 || op_index >= (int)n->ops.size()) return HAVC_E_INVALID;
    return n->ops[op_index].reserved;
}

int havc_net_profile(havc_net* n, int batch, float* ms_per_op, int n_ops) {
    if (!n || !ms_per_op || n_ops != (int)n->ops.size()) return HAVC_E_INVALID;
    havc_ctx* c = n->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, hipSetDevice(c->dev));
    if (batch < 1 || batch > n->max_batch) return fail(c, HAVC_E_INVALID, "batch out of range");
    std::vector<hipEvent_t> ev(n_ops + 1);
    for (auto& e : ev) HIP_TRY(c, hipEventCreate(&e));
    HIP_TRY(c, hipEventRecord(ev[0], c->stream));
    int rc = HAVC_OK;
    for (int i = 0; i < n_ops && rc == HAVC_OK; ++i) {
        rc = run_op(n, n->ops[i], batch);
        if (rc == HAVC_OK && hipEventRecord(ev[i + 1], c->stream) != hipSuccess) rc = HAVC_E_HIP;
    }
    if (rc == HAVC_OK) {
        if (hipStreamSynchronize(c->stream) != hipSuccess) rc = HAVC_E_HIP;
        for (int i = 0; i < n_ops && rc == HAVC_OK; ++i)
            if (hipEventElapsedTime(&ms_per_op[i], ev[i], ev[i + 1]) != hipSuccess) rc = HAVC_E_HIP;
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    if (rc == HAVC_E_HIP) return fail(c, rc, "profile failed");
    return rc;
}

int havc_net_bind_many(havc_net* n, int count, const int32_t* bufs, void* const* device_ptrs) {
    if (!n || count < 0 || (count && (!bufs || !device_ptrs))) return HAVC_E_INVALID;
    std::lock_guard<std::mutex> lk(n->ctx->mu);
    for (int i = 0; i < count; ++i)
        if (bufs[i] < 0 || bufs[i] >= (int)n->bufs.size()) return fail(n->ctx, HAVC_E_INVALID, "net_bind_many: buffer id out of range");
    if (n->bound.empty()) n->bound.assign(n->bufs.size(), nullptr);
    for (int i = 0; i < count; ++i) n->bound[bufs[i]] = device_ptrs[i];
    return HAVC_OK;
}

int havc_net_enqueue_slices(havc_net* n, int count, const int32_t* first_op, const int32_t* n_ops, const int32_t* batch) {
    if (!n || count < 0 || (count && (!first_op || !n_ops || !batch))) return HAVC_E_INVALID;
    havc_ctx* c = n->ctx;
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, hipSetDevice(c->dev));
    for (int i = 0; i < count; ++i)
        if (int rc = run_ops_locked(n, first_op[i], n_ops[i], batch[i])) return rc;
    return HAVC_OK;
}

}  // extern "C"
