// libhavc_mi355.so runtime, context unit: the set-up lock, the stream-jitter hook, context life cycle and stats, the scratch pool, allocators and copies.
// The runtime (rt_*.cpp) implements include/havc_mi355.h.  No torch, no Python: plain HIP runtime + the kernels in this directory.
#include "runtime_internal.h"
#include "build_stamp.h"

// ---- set-up is serialised process-wide -------------------------------------------------------------------------------------------------
// The reference's glue builds its models from whichever VapourSynth worker thread asks first (vsslib/vsmodels.py:196-233), so contexts,
// weights and nets of SEVERAL models can be created -- and autotuned -- from several host threads at once.  Everything that is set-up rather
// than steady-state work takes this one mutex (after the context's own): context creation (streams, eager code-object load, big-LDS opt-ins,
// the per-queue scratch warm-up below), weight upload, net creation / destruction (hipMalloc / hipFree of the activation arenas), the
// autotuner's trial launches, scratch regrowth and the device / pinned allocators.  Steady-state launches never take it.  History: before
// round 4 concurrent set-up of two models from two threads preceded a "HW Exception: GPU Hang" (1 in ~15 runs).
std::recursive_mutex g_setup_mu;

// Kernels that spill use per-queue scratch memory which the HIP runtime sizes on the FIRST launch that needs it (and re-sizes when a later
// kernel needs more).  The largest private segment of any kernel of this library is 624 bytes per lane (conv_igemm_kernel<128,304>): this
// kernel declares more than that and does nothing, so launching it once on each stream of a new context -- under the set-up mutex -- gives
// every hardware queue its final scratch size before any product launch.
__global__ void scratch_warm_kernel(int* out, int n) {
    volatile int a[192];
    for (int i = 0; i < n; ++i) a[i % 192] = i;
    if (n == 12345) out[0] = a[n % 192];
}

// HAVC_STREAM_JITTER=<seed> (race hunting, tools/cmn_race_stress.py): a kernel that does nothing for `ticks` of the 100 MHz wall clock, launched with a
// pseudo-random length in front of the work of the multi-stream entry points (plan slices, the ColorMNet read / short-term attention / side sections,
// device copies).  It moves the streams of a context -- and the look-ahead context -- against each other by up to a few hundred microseconds per call, so
// that an ordering that only holds by timing shows up as different bytes.  Results must not depend on it.  Off (one predictable branch) unless the variable is set.
__global__ void jitter_delay_kernel(unsigned long long ticks) {
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}

thread_local std::string g_create_error;

JitterState g_jitter;

void stream_jitter_delay(hipStream_t st) {
    uint64_t x = g_jitter.rng.load(std::memory_order_relaxed);
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    g_jitter.rng.store(x, std::memory_order_relaxed);
    if (x % 3) return;
    const unsigned us = 1 + (unsigned)((x >> 20) % g_jitter.max_us);
    hipLaunchKernelGGL(jitter_delay_kernel, dim3(1), dim3(64), 0, st, (unsigned long long)us * 100ull);
    (void)hipGetLastError();
}

int ensure_scratch(havc_ctx* c, int slot, size_t nbytes) {
    if (c->scratch_sz[slot] >= nbytes) return HAVC_OK;
    // a regrow costs a device synchronisation (hipFree / hipMalloc): grow by at least half, so that a request that creeps up call after call
    // (ColorMNet's memory read: the memory gains a frame every fifth frame) stalls the stream a handful of times, not every time
    const size_t exact = (nbytes + 4095) & ~(size_t)4095;
    if (c->scratch[slot]) nbytes = std::max(nbytes, c->scratch_sz[slot] + c->scratch_sz[slot] / 2);
    nbytes = (nbytes + 4095) & ~(size_t)4095;
    SetupLock setup;
    if (c->scratch[slot]) {
        HIP_TRY(c, sync_streams(c));
        (void)hipFree(c->scratch[slot]);
        c->stats.bytes_resident -= (int64_t)c->scratch_sz[slot];
        c->scratch[slot] = nullptr;
        c->scratch_sz[slot] = 0;
    }
    hipError_t e = hipMalloc(&c->scratch[slot], nbytes);
    if (e == hipErrorOutOfMemory && nbytes > exact) {      // the head-room is a convenience: near the memory limit fall back to the exact size
        (void)hipGetLastError();
        nbytes = exact;
        e = hipMalloc(&c->scratch[slot], nbytes);
    }
    if (e != hipSuccess) { c->scratch[slot] = nullptr; return hip_fail(c, e, "workspace allocation"); }
    c->scratch_sz[slot] = nbytes;
    c->stats.bytes_resident += (int64_t)nbytes;
    return HAVC_OK;
}

extern "C" {

const char* havc_version(void) { return "havc_mi355 0.1.0 (gfx950)"; }

static void havc_destroy_unlocked(havc_ctx* c);

int havc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

static void preload_device_locked(int dev) {
    static uint64_t done = 0;                              // guarded by g_setup_mu
    if (done & (1ull << (dev & 63))) return;
    preload_conv_pipe(); preload_conv_igemm(); preload_elementwise(); preload_zhang(); preload_attention(); preload_colorfilters();
    preload_tweaks(); preload_stabilizer(); preload_tiles(); preload_scdetect(); preload_scfilter(); preload_scedge(); preload_equalize(); preload_retinex(); preload_tweak_clip(); preload_chroma_stab(); preload_lut3d(); preload_overlay(); preload_metrics(); preload_recover(); preload_ddcolor(); preload_colormnet(); preload_colormnet_net(); preload_precise(); preload_precise2(); preload_remaster();
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(scratch_warm_kernel));
    (void)hipGetLastError();
    done |= 1ull << (dev & 63);
}

int havc_create(havc_ctx** out, int device_id) {
    if (!out) return fail(nullptr, HAVC_E_INVALID, "out is NULL");
    *out = nullptr;
    SetupLock setup;
    int n = havc_device_count();
    if (n <= 0) return fail(nullptr, HAVC_E_NODEVICE, "no HIP device visible (libhavc_mi355 needs an MI355X / gfx950 GPU)");
    if (device_id < 0 || device_id >= n) return fail(nullptr, HAVC_E_INVALID, "device_id out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) return fail(nullptr, HAVC_E_HIP, "hipGetDeviceProperties failed");
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return fail(nullptr, HAVC_E_NODEVICE, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
    havc_ctx* c = new havc_ctx();
    c->dev = device_id;
    if (const char* e = getenv("HAVC_TWO_STREAMS")) c->two_streams = atoi(e) != 0;
    if (const char* e = getenv("HAVC_NT_STORE_MB")) c->nt_store_bytes = strtoull(e, nullptr, 0) << 20;
    if (const char* e = getenv("HAVC_RANGE_CHECK")) c->range_check = atoi(e) != 0;
    if (const char* e = getenv("HAVC_DESC_LIMIT_BYTES")) {
        const unsigned long long v = strtoull(e, nullptr, 0);
        if (v >= 4096 && v <= 0xE0000000ull) c->desc_limit = v;
    }
    if (const char* e = getenv("HAVC_DE_SCRATCH_BYTES")) {
        const unsigned long long v = strtoull(e, nullptr, 0);
        if (v >= 8 && v <= (64ull << 20)) c->de_partials_limit = v;
    }
    if (hipSetDevice(device_id) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_main_done, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_side, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_mark, hipEventDisableTiming) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) {
        delete c;
        return fail(nullptr, HAVC_E_HIP, "failed to create stream/events");
    }
    static const bool eager = [] { const char* e = getenv("HAVC_EAGER_SETUP"); return e ? atoi(e) != 0 : true; }();
    if (eager) {
        preload_device_locked(device_id);
        for (hipStream_t st : {c->stream, c->stream2}) hipLaunchKernelGGL(scratch_warm_kernel, dim3(1), dim3(64), 0, st, (int*)nullptr, 0);
        if (hipGetLastError() != hipSuccess || sync_streams(c) != hipSuccess) {
            (void)hipGetLastError();
            havc_destroy_unlocked(c);
            return fail(nullptr, HAVC_E_HIP, "scratch warm-up launch failed");
        }
    }
    *out = c;
    return HAVC_OK;
}

void havc_destroy(havc_ctx* c) {
    if (!c) return;
    SetupLock setup;
    havc_destroy_unlocked(c);
}

static void havc_destroy_unlocked(havc_ctx* c) {
    (void)hipSetDevice(c->dev);
    (void)hipStreamSynchronize(c->stream);
    if (c->stream_h2d) {
        (void)hipStreamSynchronize(c->stream_h2d);
        (void)hipStreamSynchronize(c->stream_d2h);
        for (int k = 0; k < 2; ++k) { (void)hipEventDestroy(c->ev_up[k]); (void)hipEventDestroy(c->ev_comp[k]); (void)hipEventDestroy(c->ev_down[k]); }
        (void)hipStreamDestroy(c->stream_h2d);
        (void)hipStreamDestroy(c->stream_d2h);
    }
    for (int i = 0; i < SCR_COUNT; ++i)
        if (c->scratch[i]) (void)hipFree(c->scratch[i]);
    if (c->de_table) (void)hipFree(c->de_table);
    for (auto& kv : c->resize_tables) { (void)hipFree(kv.second.d_start); (void)hipFree(kv.second.d_w); }
    for (auto& p : c->tag_events) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    (void)hipEventDestroy(c->ev0);
    (void)hipEventDestroy(c->ev1);
    (void)hipStreamSynchronize(c->stream2);
    (void)hipEventDestroy(c->ev_fork);
    (void)hipEventDestroy(c->ev_join);
    (void)hipEventDestroy(c->ev_main_done);
    (void)hipEventDestroy(c->ev_side);
    (void)hipEventDestroy(c->ev_mark);
    (void)hipStreamDestroy(c->stream2);
    (void)hipStreamDestroy(c->stream);
    delete c;
}

const char* havc_last_error(const havc_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int havc_synchronize(havc_ctx* c) {
    if (!c) return HAVC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, sync_streams(c));
    return HAVC_OK;
}

int havc_get_stats(havc_ctx* c, havc_stats* out) {
    if (!c || !out) return HAVC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    *out = c->stats;
    return HAVC_OK;
}

int havc_reset_stats(havc_ctx* c) {
    if (!c) return HAVC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    int64_t res = c->stats.bytes_resident;
    c->stats = havc_stats{};
    c->stats.bytes_resident = res;
    c->tag_used = 0;
    c->tag_ms = 0;
    c->tag_launches = 0;
    return HAVC_OK;
}

void* havc_get_stream(havc_ctx* c) {
    if (!c) return nullptr;
    std::lock_guard<std::mutex> lk(c->mu);
    c->stream_exported = true;            // (a wrapped torch ExternalStream would dangle if the stream were re-created: ADVICE r5)
    return (void*)c->stream;
}

int havc_device_name(havc_ctx* c, char* buf, int nbuf) {
    if (!c || !buf || nbuf < 2) return HAVC_E_INVALID;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->dev) != hipSuccess) return fail(c, HAVC_E_HIP, "hipGetDeviceProperties failed");
    snprintf(buf, (size_t)nbuf, "%s/%s/%d", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return HAVC_OK;
}

int havc_host_alloc(havc_ctx* c, size_t nbytes, void** out) {
    if (!c || !out) return HAVC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, hipSetDevice(c->dev));
    SetupLock setup;
    HIP_TRY(c, hipHostMalloc(out, nbytes, hipHostMallocDefault));
    return HAVC_OK;
}

int havc_host_free(havc_ctx* c, void* p) {
    if (!c) return HAVC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, hipSetDevice(c->dev));
    HIP_TRY(c, sync_streams(c));
    SetupLock setup;
    HIP_TRY(c, hipHostFree(p));
    return HAVC_OK;
}

int havc_dev_alloc(havc_ctx* c, size_t nbytes, void** out) {
    if (!c || !out) return HAVC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, hipSetDevice(c->dev));
    SetupLock setup;
    HIP_TRY(c, hipMalloc(out, nbytes));
    return HAVC_OK;
}
int havc_dev_free(havc_ctx* c, void* p) {
    if (!c) return HAVC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, hipSetDevice(c->dev));
    HIP_TRY(c, sync_streams(c));
    SetupLock setup;
    HIP_TRY(c, hipFree(p));
    return HAVC_OK;
}
int havc_dev_upload(havc_ctx* c, void* d_dst, const void* h_src, size_t nbytes) {
    if (!c || !d_dst || !h_src) return HAVC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, hipSetDevice(c->dev));
    HIP_TRY(c, hipMemcpyAsync(d_dst, h_src, nbytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HAVC_OK;
}
int havc_dev_download(havc_ctx* c, void* h_dst, const void* d_src, size_t nbytes) {
    if (!c || !h_dst || !d_src) return HAVC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, hipSetDevice(c->dev));
    HIP_TRY(c, hipMemcpyAsync(h_dst, d_src, nbytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HAVC_OK;
}

int havc_ctx_set_stream_cus(havc_ctx* c, int n_cus) {
    if (!c || n_cus < 1) return fail(c, HAVC_E_INVALID, "set_stream_cus: n_cus >= 1");
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->side) return fail(c, HAVC_E_INVALID, "set_stream_cus: inside a side section");
    if (c->stream_exported) return fail(c, HAVC_E_INVALID, "set_stream_cus: a stream handle of this context has been handed out (havc_get_stream): call it before");
    HIP_TRY(c, hipSetDevice(c->dev));
    hipDeviceProp_t prop;
    HIP_TRY(c, hipGetDeviceProperties(&prop, c->dev));
    const int total = prop.multiProcessorCount;
    if (n_cus > total) n_cus = total;
    // bit i of the mask = CU i in the driver's enumeration, which deals consecutive bits round-robin over the XCDs: the first n bits are n / 8 CUs of every XCD
    std::vector<uint32_t> mask((total + 31) / 32, 0u);
    for (int i = 0; i < n_cus; ++i) mask[i >> 5] |= 1u << (i & 31);
    HIP_TRY(c, sync_streams(c));
    hipStream_t a = nullptr, b = nullptr;
    if (hipExtStreamCreateWithCUMask(&a, (uint32_t)mask.size(), mask.data()) != hipSuccess ||
        hipExtStreamCreateWithCUMask(&b, (uint32_t)mask.size(), mask.data()) != hipSuccess) {
        (void)hipGetLastError();
        if (a) (void)hipStreamDestroy(a);
        return fail(c, HAVC_E_HIP, "set_stream_cus: hipExtStreamCreateWithCUMask failed");
    }
    (void)hipStreamDestroy(c->stream);
    (void)hipStreamDestroy(c->stream2);
    c->stream = a;
    c->stream2 = b;
    return HAVC_OK;
}

int havc_ctx_set_stream_priority(havc_ctx* c, int level) {
    if (!c) return HAVC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->side) return fail(c, HAVC_E_INVALID, "set_stream_priority: inside a side section");
    if (c->stream_exported) return fail(c, HAVC_E_INVALID, "set_stream_priority: a stream handle of this context has been handed out (havc_get_stream): call it before");
    HIP_TRY(c, hipSetDevice(c->dev));
    int least = 0, greatest = 0;
    HIP_TRY(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
    const int prio = level < 0 ? least : level > 0 ? greatest : 0;
    HIP_TRY(c, sync_streams(c));
    hipStream_t a = nullptr, b = nullptr;
    if (hipStreamCreateWithPriority(&a, hipStreamNonBlocking, prio) != hipSuccess || hipStreamCreateWithPriority(&b, hipStreamNonBlocking, prio) != hipSuccess) {
        (void)hipGetLastError();
        if (a) (void)hipStreamDestroy(a);
        return fail(c, HAVC_E_HIP, "set_stream_priority: hipStreamCreateWithPriority failed");
    }
    (void)hipStreamDestroy(c->stream);
    (void)hipStreamDestroy(c->stream2);
    c->stream = a;
    c->stream2 = b;
    return HAVC_OK;
}

int havc_dev_copy_2d(havc_ctx* c, void* d_dst, size_t dst_pitch, const void* d_src, size_t src_pitch, size_t width_bytes, size_t rows) {
    if (!c || !d_dst || !d_src || width_bytes == 0 || rows == 0 || dst_pitch < width_bytes || src_pitch < width_bytes) return HAVC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, hipSetDevice(c->dev));
    stream_jitter(c->stream);
    HIP_TRY(c, hipMemcpy2DAsync(d_dst, dst_pitch, d_src, src_pitch, width_bytes, rows, hipMemcpyDeviceToDevice, c->stream));
    return HAVC_OK;
}

const char* havc_build_stamp(void) { return HAVC_BUILD_STAMP; }

int havc_debug_stream_jitter(int seed, int max_us) {
    g_jitter.on = false;
    if (seed != 0) {
        g_jitter.rng.store(0x9E3779B97F4A7C15ull * (uint64_t)((int64_t)seed + 1) | 1ull);
        g_jitter.max_us = (unsigned)std::max(1, max_us);
        g_jitter.on = true;
    }
    return HAVC_OK;
}

int havc_dev_copy(havc_ctx* c, void* d_dst, const void* d_src, size_t nbytes) {
    if (!c || !d_dst || !d_src) return HAVC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, hipSetDevice(c->dev));
    HIP_TRY(c, hipMemcpyAsync(d_dst, d_src, nbytes, hipMemcpyDeviceToDevice, c->stream));     // ordered on the ctx stream, does not block
    return HAVC_OK;
}

int havc_dev_memset(havc_ctx* c, void* d_dst, int value, size_t nbytes) {
    if (!c || !d_dst) return HAVC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, hipSetDevice(c->dev));
    HIP_TRY(c, hipMemsetAsync(d_dst, value, nbytes, c->stream));                               // ordered on the ctx stream, does not block
    return HAVC_OK;
}

int havc_tag_timing_enable(havc_ctx* c, int tag, int enable) {
    if (!c) return HAVC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    c->timed_tag = enable ? tag : -1;
    c->tag_used = 0;
    return HAVC_OK;
}

int havc_tag_timing_read(havc_ctx* c, double* avg_ms, int64_t* launches) {
    if (!c || !avg_ms || !launches) return HAVC_E_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(c, hipSetDevice(c->dev));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    double total = 0;
    for (size_t i = 0; i < c->tag_used; ++i) {
        float ms = 0;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->tag_events[i].first, c->tag_events[i].second));
        total += ms;
    }
    *launches = (int64_t)c->tag_used;
    *avg_ms = c->tag_used ? total / (double)c->tag_used : 0.0;
    return HAVC_OK;
}

}  // extern "C"
