// What the units of the libhavc_mi355.so runtime (rt_*.cpp) share: the context / weights / net structs, error and set-up helpers, the scratch pool and
// its slot names, operand staging, and the few functions that cross units.  Not installed; include/havc_mi355.h is the public interface.
#pragma once
#include "../../include/havc_mi355.h"
#include "kernels.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

// Set-up is serialised process-wide (rt_context.cpp says what counts as set-up and why).
extern std::recursive_mutex g_setup_mu;      // recursive: the autotuner's trial launches may regrow the split-K workspace (ensure_scratch)
// HAVC_SETUP_MUTEX=0 turns the lock into a no-op (tools/setup_stress.py bisects with it; never a production setting)
struct SetupLock {
    bool on;
    SetupLock() {
        static const bool enabled = [] { const char* e = getenv("HAVC_SETUP_MUTEX"); return e ? atoi(e) != 0 : true; }();
        on = enabled;
        if (on) g_setup_mu.lock();
    }
    ~SetupLock() { if (on) g_setup_mu.unlock(); }
    SetupLock(const SetupLock&) = delete;
    SetupLock& operator=(const SetupLock&) = delete;
};

extern thread_local std::string g_create_error;            // havc_last_error(NULL): why the last havc_create of this thread failed

// HAVC_STREAM_JITTER / havc_debug_stream_jitter (rt_context.cpp): off, one predictable branch, unless switched on
struct JitterState {
    bool on = false;
    unsigned max_us = 300;
    std::atomic<uint64_t> rng{0x9E3779B97F4A7C15ull};
    JitterState() {
        const char* e = getenv("HAVC_STREAM_JITTER");
        if (e && *e && atoll(e) != 0) {
            on = true;
            rng = 0x9E3779B97F4A7C15ull * (uint64_t)(atoll(e) + 1);
            if (const char* m = getenv("HAVC_STREAM_JITTER_US")) max_us = (unsigned)std::max(1, atoi(m));
        }
    }
};
extern JitterState g_jitter;
void stream_jitter_delay(hipStream_t st);
// one call = at most one delay kernel on `st` (two calls in three launch nothing: the un-delayed interleavings stay in the mix)
inline void stream_jitter(hipStream_t st) {
    if (!g_jitter.on) return;
    stream_jitter_delay(st);
}

struct ResizeTable {
    int taps = 0;
    int* d_start = nullptr;
    float* d_w = nullptr;
};

// ---- the scratch pool: havc_ctx::scratch[slot], grow-only (ensure_scratch), reused every call.  This enum is the one record of who owns which slot. ----
// Enumerators that share a value sit on adjacent lines.  Sharing is safe because every user of a shared slot holds c->mu for its whole call and leaves
// nothing behind in it; WITHIN a call the scope (Call, below) refuses a second claim of a slot, so two names of one value cannot meet in one entry point
// unnoticed.  The exception are SCR_BANK_*: they carry state ACROSS calls and therefore share with nobody.
enum ScratchSlot {
    // 0-5: host operands on their way to the device and results on their way back (Call::in / Call::out; device operands are used in place)
    SCR_IN = 0,                        // first operand: the image / clip of a filter, the frames entering a model; fp32 ColorMNet ops: mk / q / L plane
    SCR_IN2 = 1,                       // second operand: image b of a two-input filter; ColorMNet: qk / k / ab
    SCR_VIDEO = SCR_IN2,               //   DeOldify drivers: raw colour of the video model
    SCR_PIL_ROWS = SCR_IN2,            //   u8 row pass of a Pillow resize (havc_pil_resize, the Zhang / DDColor squash to S x S)
    SCR_RETINEX_TAP = SCR_IN2,         //   havc_retinex_clip with a tap (tests only): a chunk's Gaussian and product planes on their way out
    SCR_OUT = 2,                       // result of a filter / resize / ColorMNet op on its way to the host; the host tiles of havc_tile_slice
    SCR_SECOND = SCR_OUT,              //   DeOldify drivers: raw colour of the second (stable / artistic) model
    SCR_SQUARE = SCR_OUT,              //   Zhang / DDColor: the frames squashed to the net's S x S input
    SCR_IN3 = 3,                       // third operand: luma_from of the Spline64 resize; ColorMNet: mv / v
    SCR_RESULT = SCR_IN3,              //   model drivers: the finished frames (blend / post-process output) on their way to the host
    SCR_IN4 = 4,                       // ColorMNet: ms (shrinkage) / rel_w
    SCR_PLANES = SCR_IN4,              //   planar entry points: the three planes of a frame, in and (u8) out
    SCR_IN5 = 5,                       // ColorMNet: qe (selection) / rel_b
    SCR_PLANES_OUT = SCR_IN5,          //   havc_ddcolor_frame_planar_f: the float / half planes on their way out
    SCR_SMALL = 6,                     // small results and tables: luma sums, a 256-byte LUT, scene records, the equalisation workspace, a usage vector,
                                       // the Retinex records and histograms of a chunk
    SCR_ADJUST_TABLES = SCR_SMALL,     //   havc_adjust_rgb_clip: the channel sums of every frame, then its three 256-byte tables
    SCR_RESIZE_ROWS = 7,               // fp32 rows between the two passes of the Spline64 resize
    SCR_RETINEX_PLANES = SCR_RESIZE_ROWS,   //   havc_retinex_clip: the float64 Gaussian planes of a CHUNK of frames (n_sigmas per frame; bounded by the chunk)
    SCR_TWEAK_YUV = SCR_RESIZE_ROWS,        //   havc_tweak_clip: the Y, then U, then V planes of a CHUNK of frames between the two conversions; the two halves on
                                            //   their own (havc_rgb_to_yuv420 / havc_yuv420_to_rgb): host planes on their way in or out
    SCR_CHROMA_STAB = SCR_RESIZE_ROWS,      //   havc_chroma_stab_clip: the workspace of a CHUNK of frames -- planes, the shifted clips, tables, sums (bounded by the chunk)
    SCR_LUT3D = SCR_RESIZE_ROWS,            //   havc_lut3d_clip: the table as 16-byte points, and in front of them a host table on its way in
    SCR_DE_PARTIALS = SCR_RESIZE_ROWS,      //   havc_delta_e_clip: the per-block partial sums [frame][block] of a CHUNK of frames (bounded by de_partials_limit)
    // 8-11: the pipelined host clip (havc_colorize_clip_host), double-buffered by batch parity; the ONE-SHOT ColorMNet reads reuse them
    SCR_CLIP_SRC = 8,                  // 8, 9: source batches, SCR_CLIP_SRC + (batch & 1)
    SCR_SIM = SCR_CLIP_SRC,            //   one-shot read: similarity map [B][N][HW]; havc_local_attention: the attention map
    SCR_TOPK_IDX = SCR_CLIP_SRC + 1,   //   one-shot read: top-k indices (and, behind them, the level-1 survivors of the two-level selection)
    SCR_CLIP_DST = 10,                 // 10, 11: result batches, SCR_CLIP_DST + (batch & 1)
    SCR_TOPK_W = SCR_CLIP_DST,         //   one-shot read: top-k weights (and level-1 survivors)
    SCR_USAGE_ACC = SCR_CLIP_DST + 1,  //   one-shot read: usage accumulators
    // 12, 13: split-K partial sums, one workspace per stream: the two generators of a stable / artistic render run side by side
    SCR_SPLITK_MAIN = 12,              // launches on havc_ctx::stream
    SCR_SPLITK_SIDE = 13,              // launches on havc_ctx::stream2
    // 14-17: the BANKED memory read of the ColorMNet frame loop (havc_memory_read_banked / _reserve, usage_update_locked).  Its own slots, because a read
    // that runs ahead (havc_cmn_side_begin) leaves its top-k lists here until its frame is stepped (havc_cmn_side_wait): between a read-ahead and its
    // step NO other entry point may touch them.
    SCR_BANK_SIM = 14,                 // similarity map [N][HW]
    SCR_BANK_IDX = 15,                 // top-k indices (+ level-1 survivors)
    SCR_BANK_W = 16,                   // top-k weights (+ level-1 survivors)
    SCR_BANK_ACC = 17,                 // usage accumulators, kept at zero between reads (havc_ctx::acc_clean_sz)
    SCR_COUNT = 18
};

struct havc_ctx {
    int dev = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;        // the second generator of a stable/artistic render runs here, concurrently
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_main_done = nullptr, ev_side = nullptr, ev_mark = nullptr;
    bool marked = false;                  // havc_cmn_side_mark recorded ev_mark: the next side section starts behind THAT point of the main stream
    bool stream_exported = false;         // havc_get_stream handed a stream handle out: the streams may not be re-created any more (havc_ctx_set_stream_*)
    bool side = false;                    // between havc_cmn_side_begin / _end: the ColorMNet read (short-term attention, memory read, join) is enqueued on stream2
    size_t acc_clean_sz = 0;              // SCR_BANK_ACC holds zeros over this many bytes (0: unknown -> cleared before use)
    struct { float* use = nullptr; float* life = nullptr; int from = 0, N = 0, HW = 0, top_k = 0; } side_usage;   // its usage update, owed until havc_cmn_side_wait
    hipStream_t cur = nullptr;            // stream the plan executor launches on (stream or stream2)
    bool two_streams = true;              // HAVC_TWO_STREAMS=0 serialises the two generators (A/B measurements)
    bool range_check = false;             // HAVC_RANGE_CHECK / havc_range_check_enable: scan every op's destination for inf / NaN / abs-max
    uint64_t nt_store_bytes = 0;          // conv outputs at least this large are written with non-temporal stores (0 = never); HAVC_NT_STORE_MB
    double* de_table = nullptr;           // havc_delta_e_clip: the sRGB -> linear table (256 float64), its own allocation: it outlives every call
    uint64_t de_partials_limit = 64ull << 20;   // bytes of partial sums one chunk of havc_delta_e_clip may take; HAVC_DE_SCRATCH_BYTES lowers it (tests)
    uint64_t desc_limit = 0xE0000000ull;  // bytes one conv launch may address per operand (32-bit buffer descriptors);
                                          // HAVC_DESC_LIMIT_BYTES lowers it so tests reach the frame-chunking path at small sizes
    std::mutex mu;
    std::string err;
    havc_stats stats{};
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    void* scratch[SCR_COUNT] = {nullptr};  // grow-only scratch, indexed by ScratchSlot: allocated once, reused every call
    size_t scratch_sz[SCR_COUNT] = {0};
    hipStream_t stream_h2d = nullptr, stream_d2h = nullptr;      // copy streams of havc_colorize_clip_host (created on first use)
    hipEvent_t ev_up[2] = {nullptr, nullptr}, ev_comp[2] = {nullptr, nullptr}, ev_down[2] = {nullptr, nullptr};
    std::map<std::tuple<int, int, int>, ResizeTable> resize_tables;       // (src, dst, filter)
    // per-tag timing
    int timed_tag = -1;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> tag_events;
    size_t tag_used = 0;
    double tag_ms = 0;
    int64_t tag_launches = 0;
};

struct havc_weights {
    havc_ctx* ctx;
    uint8_t* d_blob;
    size_t nbytes;
};

struct havc_net {
    havc_ctx* ctx;
    havc_weights* w;
    std::vector<havc_op> ops;
    std::vector<havc_buf> bufdesc;
    std::vector<void*> bufs;
    int in_buf, out_buf, S, max_batch;
    int tail_first = -1;                  // index of the first op tagged 1 (exclusive tail), -1 if none
    int2* d_ktab = nullptr;               // all conv K tables, one allocation
    std::vector<int64_t> ktab_off;        // per op: element offset into d_ktab, -1 for non-conv ops
    std::vector<uint8_t> k_half_empty;    // per op: 1 = chunks 4..7 of the last stage of its K table are all pad entries (ConvArgs::k_half_empty)
    const void* in_override = nullptr;
    void* out_override = nullptr;
    unsigned* d_range = nullptr;          // range check: per op {abs-max bits, -, non-finite count (64 bit)}
    bool range_ready = false;             // buffers were zero-filled at creation (never-written padding cannot trip the scan)
    std::vector<float> range_absmax;
    std::vector<int64_t> range_bad;
    std::vector<void*> bound;             // havc_net_bind: caller-owned device memory standing in for a buffer (nullptr = own allocation)
    double flops_per_frame = 0;
};

inline int fail(havc_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}

inline int hip_fail(havc_ctx* c, hipError_t e, const char* what) {
    std::string m = std::string(what) + ": " + hipGetErrorString(e);
    (void)hipGetLastError();
    return fail(c, e == hipErrorOutOfMemory ? HAVC_E_OOM : HAVC_E_HIP, m);
}

#define HIP_TRY(ctx, expr)                                         \
    do {                                                           \
        hipError_t _e = (expr);                                    \
        if (_e != hipSuccess) return hip_fail((ctx), _e, #expr);   \
    } while (0)

// Both streams idle: required before anything either of them may still touch is freed or re-allocated.
inline hipError_t sync_streams(havc_ctx* c) {
    hipError_t a = hipStreamSynchronize(c->stream);
    hipError_t b = c->stream2 ? hipStreamSynchronize(c->stream2) : hipSuccess;
    return a != hipSuccess ? a : b;
}

int ensure_scratch(havc_ctx* c, int slot, size_t nbytes);                                   // rt_context.cpp

// ---- functions that cross units ----
int run_ops_locked(havc_net* n, int first, int count, int batch);                           // rt_net.cpp
int net_run_rgb8_locked(havc_net* n, const uint8_t* d_in, uint8_t* d_out, int batch, hipStream_t on = nullptr);
int resize_rgb8(havc_ctx* c, const uint8_t* d_src, int sw, int sh, uint8_t* d_dst, int dw, int dh, int n, const uint8_t* d_orig, int filter = 0);   // rt_resize.cpp
int pil_resize_dev(havc_ctx* c, const uint8_t* d_src, int sw, int sh, uint8_t* d_tmp, uint8_t* d_dst, int dw, int dh, int n, int resample);

inline void* bufptr(havc_net* n, int id) {
    if (id == n->in_buf && n->in_override) return const_cast<void*>(n->in_override);
    if (id == n->out_buf && n->out_override) return n->out_override;
    if (!n->bound.empty() && n->bound[id]) return n->bound[id];
    return n->bufs[id];
}

template <typename T>
inline const T* wptr(havc_net* n, int64_t off) {
    return off < 0 ? nullptr : reinterpret_cast<const T*>(n->w->d_blob + off);
}

struct Timer {
    havc_ctx* c;
    explicit Timer(havc_ctx* ctx) : c(ctx) { (void)hipEventRecord(c->ev0, c->stream); }
    int finish() {
        HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
        HIP_TRY(c, hipEventSynchronize(c->ev1));
        float ms = 0;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
        c->stats.last_ms = ms;
        c->stats.total_ms += ms;
        return HAVC_OK;
    }
};

// ---- pointer-agnostic operands ---------------------------------------------------------------------------------------
// Every frame / filter entry point accepts HOST or DEVICE pointers for its image operands (unified addressing tells them apart).
// Host operands are staged through the ctx scratch buffers and the call blocks until the result is back in host memory; device
// operands (havc_dev_alloc, or any hipMalloc of this device) are used in place, nothing is copied and the call only ENQUEUES
// work on the ctx stream (havc_synchronize / a later host-output call / havc_dev_download order against it).  This is what
// lets a whole HAVC merge graph run without leaving HBM (vsdeoldify_amd/device.py).
inline bool is_device_ptr(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeDevice;
}

// One entry point's use of that protocol.  The scope holds c->mu and has made c->dev current; it stages operands, counts launches, and hands host results
// back with ONE synchronisation at the end.  Its rc, once non-zero, turns every later member into a no-op that returns NULL: an entry point stages all
// its operands, looks at rc once, launches, and returns done().  Stream order within a call: uploads, memsets, launches, downloads.
struct Call {
    havc_ctx* const c;
    const char* const what;            // the entry point: every message of the scope starts with it
    int rc = HAVC_OK;

    // Several operands in ONE slot: add() each, reserve(), then in() / out() each in the order of the add()s.  The slot is sized before the first copy into
    // it, because ensure_scratch frees and re-allocates a slot that grows, and growing it after a copy would lose that copy: placing an operand before
    // reserve(), or beyond what the add()s reserved, is refused and never regrows the slot.
    struct Pack {
        int slot;
        size_t need = 0, at = 0;       // bytes the host operands take (each rounded up to 256) / bytes placed so far
        unsigned host = 0;             // bit i: operand i is host memory (asked once, in add())
        int n = 0, placed = 0;
        uint8_t* base = nullptr;       // set by reserve()
        explicit Pack(int s) : slot(s) {}
    };

    Call(havc_ctx* ctx, const char* w) : c(ctx), what(w), lk(ctx->mu) { check(hipSetDevice(c->dev), "hipSetDevice"); }

    // a HIP status: the first failure becomes rc; true while the call is good
    bool check(hipError_t e, const char* op) {
        if (!rc && e != hipSuccess) rc = hip_fail(c, e, (std::string(what) + ": " + op).c_str());
        return !rc;
    }

    // A slot's memory, at least nbytes of it.  A call claims a slot ONCE, whatever the kinds of its operands: slots are shared between entry points on the
    // strength of "one user at a time" (ScratchSlot), and two operands of one call in one slot would overwrite each other.  They belong in a Pack.
    void* scratch(int slot, size_t nbytes) {
        if (!claim(slot) || (rc = ensure_scratch(c, slot, nbytes))) return nullptr;
        return c->scratch[slot];
    }

    // an input operand on the device: p itself, or its upload into `slot`.  An absent (NULL) optional operand stays NULL.
    template <typename T>
    const T* in(int slot, const T* p, size_t nbytes) {
        if (!p || !claim(slot) || is_device_ptr(p)) return rc ? nullptr : p;
        return (const T*)upload(scratch_of(slot, nbytes), p, nbytes);
    }
    template <typename T>
    const T* in(Pack& k, const T* p, size_t nbytes) {
        bool host;
        void* d = place(k, p, nbytes, &host);
        return (const T*)(host ? upload(d, p, nbytes) : d);
    }

    // where the kernels write a result: p itself, or room in `slot` that done() copies back to p
    template <typename T>
    T* out(int slot, T* p, size_t nbytes) {
        if (!p || !claim(slot) || is_device_ptr(p)) return rc ? nullptr : p;
        return (T*)download(p, scratch_of(slot, nbytes), nbytes);
    }
    template <typename T>
    T* out(Pack& k, T* p, size_t nbytes) {
        bool host;
        void* d = place(k, p, nbytes, &host);
        return (T*)(host ? download(p, d, nbytes) : d);
    }

    void add(Pack& k, const void* p, size_t nbytes) {
        if (!is_device_ptr(p)) { k.host |= 1u << k.n; k.need += pack_room(nbytes); }
        ++k.n;
    }
    void reserve(Pack& k) {
        if (claim(k.slot) && k.need && !(rc = ensure_scratch(c, k.slot, k.need))) k.base = (uint8_t*)c->scratch[k.slot];
    }

    // a host result that is no operand (records, sums): done() copies nbytes from d to host.  Returns d.
    void* download(void* host, void* d, size_t nbytes) {
        if (rc) return nullptr;
        if (n_back == MAX_BACK) { rc = fail(c, HAVC_E_INVALID, std::string(what) + ": too many host results in one call"); return nullptr; }
        back[n_back++] = {host, d, nbytes};
        return d;
    }

    void zero(void* d, size_t nbytes) { if (!rc) check(hipMemsetAsync(d, 0, nbytes, c->stream), "hipMemsetAsync"); }
    // a copy enqueued NOW: a table on its way in, a result that leaves a buffer the call is about to reuse.  One into host memory makes done() wait for it.
    void copy(void* dst, const void* src, size_t nbytes, hipMemcpyKind kind) {
        if (!rc && check(hipMemcpyAsync(dst, src, nbytes, kind, c->stream), "hipMemcpyAsync") && kind == hipMemcpyDeviceToHost) pending = true;
    }
    // for the call that needs a result in the middle (a sum the next launch depends on)
    void sync() {
        if (!rc) check(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
        pending = false;
    }

    bool launched(int e, int n = 1) {
        if (rc) return false;
        c->stats.launches += n;
        if (e) rc = hip_fail(c, (hipError_t)e, what);
        return !rc;
    }

    // every host result goes back, then ONE synchronisation -- if and only if there was one: a call with device results only has enqueued and returns
    int done() {
        for (int i = 0; i < n_back; ++i) copy(back[i].host, back[i].dev, back[i].nbytes, hipMemcpyDeviceToHost);
        if (pending) sync();
        return rc;
    }

  private:
    enum { MAX_BACK = 8 };
    std::lock_guard<std::mutex> lk;
    unsigned claimed = 0;              // bit per ScratchSlot this call has claimed
    bool pending = false;              // a device-to-host copy is on the stream and nobody has waited for it yet
    struct { void* host; const void* dev; size_t nbytes; } back[MAX_BACK];
    int n_back = 0;

    static size_t pack_room(size_t nbytes) { return (nbytes + 255) & ~(size_t)255; }
    bool claim(int slot) {
        if (rc) return false;
        if (claimed & (1u << slot)) { rc = fail(c, HAVC_E_INVALID, std::string(what) + ": scratch slot " + std::to_string(slot) + " claimed twice in one call"); return false; }
        claimed |= 1u << slot;
        return true;
    }
    void* scratch_of(int slot, size_t nbytes) { return (rc = ensure_scratch(c, slot, nbytes)) ? nullptr : c->scratch[slot]; }   // of a slot already claimed
    void* upload(void* d, const void* p, size_t nbytes) {
        if (d) copy(d, p, nbytes, hipMemcpyHostToDevice);
        return rc ? nullptr : d;
    }
    void* place(Pack& k, const void* p, size_t nbytes, bool* host) {
        *host = false;
        if (rc) return nullptr;
        const int i = k.placed++;
        const bool added = i < k.n, on_host = added && ((k.host >> i) & 1);
        if (added && !on_host) return const_cast<void*>(p);
        if (!added || !k.base || k.at + pack_room(nbytes) > k.need) {
            rc = fail(c, HAVC_E_INVALID, std::string(what) + ": the pack in scratch slot " + std::to_string(k.slot) + " places an operand before reserve(), or beyond what was reserved");
            return nullptr;
        }
        *host = true;
        void* d = k.base + k.at;
        k.at += pack_room(nbytes);
        return d;
    }
};

// two-input (b may be NULL) / one-output per-pixel filter: stage, launch, hand back
template <typename Launch>
inline int run_filter(havc_ctx* c, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t nbytes, const char* what, Launch launch) {
    Call call(c, what);
    const uint8_t *da = call.in(SCR_IN, a, nbytes), *db = call.in(SCR_IN2, b, nbytes);
    uint8_t* dout = call.out(SCR_OUT, out, nbytes);
    if (call.rc) return call.rc;
    call.launched(launch(da, db, dout));
    return call.done();
}
