// api.hip — the C-ABI of include/ggr_raster.h: orchestration of the gfx950 kernels.
//
// Replaces `RasterizeGaussiansCUDA` / `RasterizeGaussiansBackwardCUDA` of the extension GGRt
// imports at reference ggrt/model/pixelsplat/decoder/cuda_splatting.py:6-9.
// No global mutable state: the only statics are thread_local — an error string and, per device, one pinned word +
// one event for the num_rendered read-back, a side stream — handed back to a process-wide pool when the thread ends (below).
#include "../../include/ggr_raster.h"
#include "ggr_common.h"
#include "blend_feat.h"
#include "blend_contrib.h"
#include "blend_pick.h"
#include "blend_hits.h"
#include "blend_hits_grad.h"
#include "blend_dist.h"
#include "blend_absgrad.h"
#include "projection.h"
#include "adapter.h"
#include "depth_head.h"
#include "epipolar.h"
#include "epipolar_attn.h"
#include "epipolar_attn_enc.h"
#include "image_loss.h"
#include "photometric_loss.h"
#include "warp_cost.h"
#include "upsample_depth.h"
#include "gru_gates.h"
#include "gru_conv.h"
#include <algorithm>
#include <mutex>
#include <vector>

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

namespace {

thread_local char g_err[512] = "";
const char kSpinFault[] = "depth sort: a look-back spin hit its bound (GPU preempted or halted?); frame not rendered";
const char kRangeFault[] = "depth sort: a sort key beyond 30 bits reached the sort (keys must come from preprocess_fwd); frame not rendered";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                           \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) return fail(GGR_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

#define KCHECK(dbg, s, what)                                                                    \
    do {                                                                                        \
        hipError_t e_ = hipGetLastError();                                                      \
        if (e_ == hipSuccess && (dbg)) e_ = hipStreamSynchronize(s);                            \
        if (e_ != hipSuccess) return fail(GGR_E_HIP, "%s: %s", what, hipGetErrorString(e_));    \
    } while (0)

// Optional per-stage HIP-event timing (profiling mode only: stage_ms != NULL).  mark(stage): the time since the previous
// mark belongs to `stage` (the forward's stages are not walked in index order: the per-tile depth sort sits behind the scatter).
struct StageTimer {
    hipStream_t s;
    float* out;
    int n;
    hipEvent_t ev[24];
    int stage_of[24];
    int used = 0;
    StageTimer(hipStream_t s_, float* out_, int n_) : s(s_), out(out_), n(n_) {
        if (out) for (int i = 0; i < 24; i++) (void)hipEventCreate(&ev[i]);
        mark(-1);
    }
    void mark(int stage) {
        if (out && used < 24) { (void)hipEventRecord(ev[used], s); stage_of[used] = stage; used++; }
    }
    void finish() {
        if (!out) return;
        (void)hipStreamSynchronize(s);
        for (int i = 1; i < used; i++) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, ev[i - 1], ev[i]);
            if (stage_of[i] >= 0 && stage_of[i] < n) out[stage_of[i]] += ms;
        }
        for (int i = 0; i < 24; i++) (void)hipEventDestroy(ev[i]);
        out = nullptr;
    }
    ~StageTimer() { finish(); }
};

// GgrForwardOptions: NULL = the defaults of ggr_forward; checked before anything is enqueued
int validate_options(const GgrForwardOptions* opt, int* antialiasing) {
    *antialiasing = 0;
    if (!opt) return GGR_OK;
    if (opt->struct_size < (int32_t)(offsetof(GgrForwardOptions, antialiasing) + sizeof(int32_t)))
        return fail(GGR_E_INVALID, "GgrForwardOptions.struct_size %d is smaller than the %d bytes of its fields", (int)opt->struct_size,
                    (int)(offsetof(GgrForwardOptions, antialiasing) + sizeof(int32_t)));
    if (opt->antialiasing != 0 && opt->antialiasing != 1)
        return fail(GGR_E_INVALID, "GgrForwardOptions.antialiasing must be 0 or 1, not %d", (int)opt->antialiasing);
    *antialiasing = opt->antialiasing;
    return GGR_OK;
}

// GgrForwardExtra / GgrBackwardExtra: NULL = no extra plane; checked before anything is enqueued
template <typename E>
int validate_extra(const E* ex, const char* name) {
    if (!ex) return GGR_OK;
    if (ex->struct_size < (int32_t)sizeof(E))
        return fail(GGR_E_INVALID, "%s.struct_size %d is smaller than the %d bytes of its fields", name, (int)ex->struct_size,
                    (int)sizeof(E));
    if (ex->reserved != 0) return fail(GGR_E_INVALID, "%s.reserved must be 0, not %d", name, (int)ex->reserved);
    return GGR_OK;
}

// GgrBackwardExtra2.dL_dtanfov of an (already validated) backward extra; a struct_size that ends before the field: absent
float* extra_dtanfov(const GgrBackwardExtra* ex) {
    if (!ex || ex->struct_size < (int32_t)sizeof(GgrBackwardExtra2)) return nullptr;
    return reinterpret_cast<const GgrBackwardExtra2*>(ex)->dL_dtanfov;
}

int validate(const GgrSettings* st, const GgrForwardIn* in) {
    if (!st || !in) return fail(GGR_E_INVALID, "null settings / inputs");
    if (st->num_points < 0 || st->image_width < 0 || st->image_height < 0)
        return fail(GGR_E_INVALID, "negative size");
    if ((in->shs == nullptr) == (in->colors_precomp == nullptr) && st->num_points > 0)
        return fail(GGR_E_INVALID, "Please provide excatly one of either SHs or precomputed colors!");
    const bool has_sr = in->scales != nullptr && in->rotations != nullptr;
    const bool any_sr = in->scales != nullptr || in->rotations != nullptr;
    if (st->num_points > 0 && ((!has_sr && in->cov3D_precomp == nullptr) || (any_sr && in->cov3D_precomp != nullptr)))
        return fail(GGR_E_INVALID,
                    "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
    if (st->sh_max_degree != 0 && st->sh_max_degree != 3 && st->sh_max_degree != 4)
        return fail(GGR_E_INVALID, "sh_max_degree must be 0 (default), 3 or 4");
    if ((st->depth_sort & ~GGR_DEPTH_SORT_NO_BUCKETS) < GGR_DEPTH_SORT_AUTO || (st->depth_sort & ~GGR_DEPTH_SORT_NO_BUCKETS) > GGR_DEPTH_SORT_PER_TILE)
        return fail(GGR_E_INVALID, "depth_sort must be 0 (auto), 1 (global) or 2 (per tile), optionally | GGR_DEPTH_SORT_NO_BUCKETS");
    if ((st->scissor[0] | st->scissor[1] | st->scissor[2] | st->scissor[3]) &&
        (st->scissor[0] < 0 || st->scissor[1] < 0 || st->scissor[2] <= st->scissor[0] || st->scissor[3] <= st->scissor[1]))
        return fail(GGR_E_INVALID, "scissor must be x0 < x1, y0 < y1, all >= 0 (or all zero for none)");
    if (in->shs && st->sh_stride < (st->sh_degree > 3 ? 16 : (st->sh_degree + 1) * (st->sh_degree + 1)))
        return fail(GGR_E_INVALID, "sh_stride %d too small for sh_degree %d", st->sh_stride, st->sh_degree);
    const int64_t tiles = (int64_t)((st->image_width + GGR_TILE - 1) / GGR_TILE) * ((st->image_height + GGR_TILE - 1) / GGR_TILE);
    if (tiles > (1 << 24)) return fail(GGR_E_LIMIT, "image has %lld tiles; at most 2^24 supported", (long long)tiles);
    if (st->image_width > 65535 * GGR_TILE)   // (the packed tile rect holds 16-bit tile coordinates)
        return fail(GGR_E_LIMIT, "image width %d exceeds %d px (65535 tile columns)", st->image_width, 65535 * GGR_TILE);
    if (st->image_height > 65535 * GGR_TILE)
        return fail(GGR_E_LIMIT, "image height %d exceeds %d px (65535 tile rows)", st->image_height, 65535 * GGR_TILE);
    return GGR_OK;
}

// Per host thread and device: the library's two small host-side resources (the read-back slot and the side stream below).
// A thread OWNS its slot while it lives — no lock on the forward's path — and hands it back to a process-wide pool when it
// ends, without a HIP call (a thread_local destructor can run after the HIP runtime is gone): the next thread that needs
// one for that device takes it from the pool, so short-lived host threads (autograd workers, data-loader threads that
// render) reuse a handful of slots instead of leaking a pinned line, a stream and six events each.  The pool
// itself is never destroyed (static destruction order).
#define GGR_MAX_DEVICES 64
template <class T>
struct SlotPool {
    std::mutex mu;
    std::vector<T*> free_slots[GGR_MAX_DEVICES];
    int created = 0;   // slots ever allocated (ggr_debug_host_slots)
    static SlotPool& get() { static SlotPool* p = new SlotPool; return *p; }
};
template <class T>
struct ThreadSlots {
    T* slot[GGR_MAX_DEVICES] = {};
    ~ThreadSlots() {
        SlotPool<T>& pool = SlotPool<T>::get();
        std::lock_guard<std::mutex> lk(pool.mu);
        for (int d = 0; d < GGR_MAX_DEVICES; d++)
            if (slot[d]) pool.free_slots[d].push_back(slot[d]);
    }
    // this thread's slot for the current device (nullptr: no current device, or its index is beyond GGR_MAX_DEVICES)
    T* current() {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= GGR_MAX_DEVICES) { (void)hipGetLastError(); return nullptr; }
        if (!slot[dev]) {
            SlotPool<T>& pool = SlotPool<T>::get();
            std::lock_guard<std::mutex> lk(pool.mu);
            if (!pool.free_slots[dev].empty()) { slot[dev] = pool.free_slots[dev].back(); pool.free_slots[dev].pop_back(); }
            else { slot[dev] = new T; pool.created++; }
        }
        return slot[dev];
    }
};
// per host thread and device: one pinned word + one event for the num_rendered read-back of the exact mode (a
// thread has at most one forward between its launch and its sync, so the slot is never shared)
#define GGR_READBACK_ARMED GGR_HOST_ARMED  // (counts stop at 0x7FFFFFFF; GGR_HOST_FAULT_* report a sort fault)
struct ReadbackSlot {
    uint32_t* host = nullptr;
    hipEvent_t ev = nullptr;        // behind the kernel that writes the word
    hipEvent_t ev_start = nullptr;  // in front of the tile-list kernels: the wait's time bound starts here
};
ReadbackSlot* readback_slot() {
    static thread_local ThreadSlots<ReadbackSlot> slots;
    ReadbackSlot* rp = slots.current();
    if (!rp) return nullptr;
    ReadbackSlot& r = *rp;
    if (!r.host) {
        void* p = nullptr;
        // coherent (fine-grained) on purpose: the kernel's system-scope store must become visible to the spinning
        // host while the kernel is still running; a non-coherent mapping would only show it at the kernel's end
        if (hipHostMalloc(&p, 64, hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) return nullptr;
        if (hipEventCreateWithFlags(&r.ev, hipEventDisableTiming) != hipSuccess) { (void)hipHostFree(p); return nullptr; }
        if (hipEventCreateWithFlags(&r.ev_start, hipEventDisableTiming) != hipSuccess) {
            (void)hipEventDestroy(r.ev); r.ev = nullptr; (void)hipHostFree(p); return nullptr;
        }
        r.host = (uint32_t*)p;
    }
    return &r;
}

// The forward's side stream (forward_impl): the SH colour half of the per-Gaussian stage runs on it beside the depth sort and
// the tile-list kernels.  One per (host thread, device), like the read-back slot: created on first use, lowest priority (the
// kernels of the caller's stream — the critical path — win the CUs whenever both have workgroups to place), ordered against
// the caller's stream by two events per forward (fork behind the geometry kernel, join in front of the blend).  Holds no
// state between calls; two forwards of one thread on two streams share it and merely serialise their colour kernels.
// ROCm maps a process's streams onto a FEW hardware queues (four by default, GPU_MAX_HW_QUEUES): a side stream created after
// the host has made three or more streams of its own lands on the queue of the caller's stream, and then every kernel the
// forward chains on the caller's stream behind the fork is held up while the colour kernel runs — measured at C5' 0.80-0.86
// instead of 0.69 ms per step (geometry stage 35 -> 63 µs, depth sort 113 -> 169-250, tile counts 47 -> 78;
// tools/experiments/r06_slow_after_graph.py; bench.py's own graph legs did it to the legs behind them).  So a side stream is
// PROBED against the caller's stream before it is used — the forward's own pattern in miniature: a kernel on the caller's
// stream, the fork, a 100 µs one-wave spin on the candidate, a chain of eight empty kernels on the caller's stream, HIP events
// around the chain, against the same with an empty kernel instead of the spin.  A candidate that stretches the chain is
// dropped and the next one tried (the runtime hands its queues out round robin); no candidate after six: no split for this
// caller stream.  Once per (host thread, device, caller stream): ≈ 0.5 ms and one synchronisation of the caller's stream.
// GPU_MAX_HW_QUEUES=16 in the environment of the process avoids the sharing at its root (measured: 0.69 with eight host streams).
struct SideStream {
    hipStream_t stream = nullptr;     // for the caller stream the call came with (set by side_stream())
    hipEvent_t fork = nullptr, join = nullptr;
    hipEvent_t t0 = nullptr, t1 = nullptr;   // timing brackets of the colour kernel (stage profiling; the probe)
    bool failed = false;
    struct Pair { hipStream_t caller; hipStream_t side; bool usable; } pairs[4];
    int npairs = 0;
};
// true: `cand` runs concurrently with `s`
bool side_stream_is_concurrent(SideStream& r, hipStream_t s, hipStream_t cand) {
    if (hipStreamSynchronize(s) != hipSuccess || hipStreamSynchronize(cand) != hipSuccess) { (void)hipGetLastError(); return false; }
    ReadbackSlot* rb = readback_slot();   // (its pinned, coherent line: word 8 tells the host that the spin is on the device)
    if (!rb) return false;
    volatile uint32_t* started = rb->host + 8;
    // the forward's own pattern: a kernel on the caller's stream, the fork (event on the caller's stream, the candidate waits
    // for it), a kernel on the candidate, then a CHAIN of kernels on the caller's stream — timed with the candidate's kernel a
    // 200 µs spin that is known to be running, and, for comparison, an empty one
    float best = 1e9f, base = 1e9f;
    for (int rep = 0; rep < 4; rep++) {   // (the first launches of a fresh stream pay for its set-up)
        const bool spin = (rep & 1) != 0;
        ggr::launch_noop(s);
        if (hipEventRecord(r.fork, s) != hipSuccess || hipStreamWaitEvent(cand, r.fork, 0) != hipSuccess) break;
        if (spin) {
            *started = 0u;
            ggr::launch_spin(20000ull /*200 µs*/, (uint32_t*)started, cand);
            timespec t0, t1;
            clock_gettime(CLOCK_MONOTONIC, &t0);
            while (*started == 0u) {   // (bounded: 50 ms)
                clock_gettime(CLOCK_MONOTONIC, &t1);
                if ((t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) * 1e-6 > 50.0) break;
            }
        } else {
            ggr::launch_noop(cand);
        }
        if (hipEventRecord(r.t0, s) != hipSuccess) break;
        for (int k = 0; k < 8; k++) ggr::launch_noop(s);
        if (hipEventRecord(r.t1, s) != hipSuccess || hipEventSynchronize(r.t1) != hipSuccess) break;
        float ms = 1e9f;
        if (hipEventElapsedTime(&ms, r.t0, r.t1) == hipSuccess) { if (spin) best = std::min(best, ms); else base = std::min(base, ms); }
        (void)hipStreamSynchronize(cand);
    }
    (void)hipGetLastError();
    // measured: 0.017-0.018 ms either way on a candidate with a queue of its own, 0.017-0.023 against 0.053-0.054 on one that
    // shares the caller's
    const bool ok = best < 1.5f * base + 0.010f;
    if (getenv("GGR_SIDE_STREAM_DEBUG"))
        fprintf(stderr, "[ggr] side-stream probe: caller %p candidate %p: chain of 8 kernels %.3f ms beside an empty kernel, %.3f beside a "
                        "running spin -> %s\n", (void*)s, (void*)cand, base, best, ok ? "concurrent" : "shares the caller's queue");
    return ok;
}
SideStream* side_stream(hipStream_t caller) {
    static thread_local ThreadSlots<SideStream> slots;
    SideStream* rp = slots.current();
    if (!rp) return nullptr;
    SideStream& r = *rp;
    if (r.failed) return nullptr;
    if (!r.fork) {
        bool ok = hipEventCreateWithFlags(&r.fork, hipEventDisableTiming) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&r.join, hipEventDisableTiming) == hipSuccess;
        ok = ok && hipEventCreate(&r.t0) == hipSuccess && hipEventCreate(&r.t1) == hipSuccess;
        if (!ok) { r.failed = true; (void)hipGetLastError(); return nullptr; }
    }
    for (int i = 0; i < r.npairs; i++)
        if (r.pairs[i].caller == caller) { r.stream = r.pairs[i].side; return r.pairs[i].usable ? &r : nullptr; }
    if (r.npairs == 4) return nullptr;   // (a fifth caller stream of one thread: no split for it)
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);   // lo = least priority (numerically greatest)
    const char* pe = getenv("GGR_COLOUR_PRIO");   // dev: "high" / "normal" instead of the lowest priority
    const int prio = (pe && *pe == 'h') ? hi : (pe && *pe == 'n') ? (lo + hi) / 2 : lo;
    const char* np = getenv("GGR_SIDE_STREAM_PROBE");   // "0": take the first stream unprobed (the behaviour until round 5)
    const bool probe = !(np && *np == '0');
    SideStream::Pair pr{caller, nullptr, false};
    // (an earlier caller stream's side stream may serve this one too)
    for (int i = 0; i < r.npairs && !pr.usable; i++)
        if (r.pairs[i].usable && (!probe || side_stream_is_concurrent(r, caller, r.pairs[i].side))) { pr.side = r.pairs[i].side; pr.usable = true; }
    hipStream_t rejected[6];
    int nrej = 0;
    for (int attempt = 0; attempt < 6 && !pr.usable; attempt++) {
        hipStream_t cand = nullptr;
        if (hipStreamCreateWithPriority(&cand, hipStreamNonBlocking, prio) != hipSuccess) { (void)hipGetLastError(); break; }
        if (!probe || side_stream_is_concurrent(r, caller, cand)) { pr.side = cand; pr.usable = true; }
        else rejected[nrej++] = cand;   // (kept until the search ends: destroyed at once, its queue slot would be handed out again)
    }
    for (int i = 0; i < nrej; i++) (void)hipStreamDestroy(rejected[i]);
    r.pairs[r.npairs++] = pr;
    r.stream = pr.side;
    return pr.usable ? &r : nullptr;
}
// GGR_SPLIT_COLOUR=0: the per-Gaussian stage as ONE kernel on the caller's stream (dev / A-B measurements)
// (read on every forward: a test or a host can switch within a process)
bool split_colour_enabled() {
    const char* e = getenv("GGR_SPLIT_COLOUR");
    return !(e && *e == '0');
}

// Blocks of the colour kernel's launch (per Gaussian set): a few PERSISTENT blocks per CU.  Unthrottled (one block per
// 256-Gaussian chunk) the kernel finishes in 50 µs at C3 and doubles the duration of the depth-sort passes it runs beside (a
// sort tile waits for a CU's wave slots and LDS, every later tile for its look-back): forward +13 µs instead of −30.  One
// block per CU streams ≈ 2.7 TB/s and has until the blend needs the colours — the depth sort and the tile-list kernels,
// whose duration grows with the number of (view, Gaussian) pairs as the colour kernel's bytes do; beyond ≈ 2 M pairs one
// block per CU is no longer enough (C6′, 4.9 M pairs: the blend waited 0.35 ms for the colours), so the count grows with the
// pairs: 1 + pairs / 2 M, at most 4.  GGR_COLOUR_BLOCKS_PER_CU overrides (0 = unthrottled).
#define GGR_SPLIT_MAX_POINTS 2500000
int colour_grid_blocks(size_t pairs) {
    const char* e_blocks = getenv("GGR_COLOUR_BLOCKS_PER_CU");   // (read per call, like GGR_SPLIT_COLOUR)
    const int forced = (e_blocks && *e_blocks) ? atoi(e_blocks) : -1;
    // (the CU count of the CURRENT device, looked up once per device — ADVICE r5: a process that drives several devices must
    //  not throttle all of them by the first one's count)
    static int cus_of[GGR_MAX_DEVICES] = {0};
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < GGR_MAX_DEVICES) {
        int c = __atomic_load_n(&cus_of[dev], __ATOMIC_RELAXED);
        if (c == 0) {
            hipDeviceProp_t prop;
            c = (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
            __atomic_store_n(&cus_of[dev], c, __ATOMIC_RELAXED);
        }
        cus = c;
    } else {
        (void)hipGetLastError();
    }
    const int per_cu = forced >= 0 ? forced : (int)std::min<size_t>(4, 1 + pairs / 2000000);
    return per_cu <= 0 ? 0 : per_cu * cus;
}

// The exact mode's wait for num_rendered: the host watches the pinned word (armed with a sentinel no count can take)
// and, every 1024 polls, asks `query` (hipEventQuery of the event behind the kernel that writes the word) whether the
// kernel has ended.  Leaves on: the word changed; the query says "done" (the word is then re-read once — a
// non-coherent mapping shows it only now); the query returns ANYTHING other than hipErrorNotReady (stream in error,
// device lost: the word will never change) → GGR_E_HIP; or `timeout_s` seconds without either (a hung GPU) →
// GGR_E_HIP.  The clock of that bound only starts once `query_start` (the event recorded on the stream right IN FRONT
// of the tile-list kernels, or NULL: at once) reports completion: work that was queued on the stream ahead of this
// forward — a long evaluation queue, a device shared with another process — is not this forward's hang.
// The bound itself is GGR_READBACK_TIMEOUT_S seconds (environment, default 30; ≤ 0 = wait for as long as the event
// query keeps answering "not ready").  Work queued AHEAD of the forward has its own, generous bound from this function's
// entry (GGR_READBACK_QUEUE_TIMEOUT_S, default 600 s, ≤ 0 = none): a device hung in earlier work never starts the first
// clock.  The device-side spins are bounded the same way — with both bounds at their defaults nothing in a forward waits
// forever, on a GPU that makes progress or on one that does not.
typedef hipError_t (*ReadbackQueryFn)(void*);
double readback_timeout_s() {
    const char* e = getenv("GGR_READBACK_TIMEOUT_S");
    if (e && *e) { char* end = nullptr; const double v = strtod(e, &end); if (end != e) return v; }
    return 30.0;
}
// bound on the wait for work queued on the stream BEFORE this forward (the per-forward bound above only runs from the
// tile-list kernels' turn): generous, since a caller may legitimately have minutes of work in front; <= 0 disables
double readback_queue_timeout_s() {
    const char* e = getenv("GGR_READBACK_QUEUE_TIMEOUT_S");
    if (e && *e) { char* end = nullptr; const double v = strtod(e, &end); if (end != e) return v; }
    return 600.0;
}
int wait_readback(volatile uint32_t* hw, ReadbackQueryFn query, void* ctx, double timeout_s, uint32_t* value,
                  ReadbackQueryFn query_start = nullptr, void* ctx_start = nullptr) {
    timespec t0;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    const timespec t_entry = t0;
    const double queue_timeout_s = readback_queue_timeout_s();
    bool started = query_start == nullptr;
    uint32_t v = *hw;
    for (uint32_t spins = 0; v == GGR_READBACK_ARMED; v = *hw) {
        if ((++spins & 0x3FFu) == 0) {
            const hipError_t q = query(ctx);
            if (q == hipSuccess) { v = *hw; break; }
            if (q != hipErrorNotReady)
                return fail(GGR_E_HIP, "num_rendered read-back: the stream is in error (%s); frame not rendered", hipGetErrorString(q));
            if (!started) {   // still behind earlier work of the stream: the bound does not run yet
                const hipError_t qs = query_start(ctx_start);
                if (qs == hipSuccess) { started = true; clock_gettime(CLOCK_MONOTONIC, &t0); }
                else if (qs != hipErrorNotReady)
                    return fail(GGR_E_HIP, "num_rendered read-back: the stream is in error (%s); frame not rendered", hipGetErrorString(qs));
                else {   // a device hung in work queued BEFORE this forward never starts the clock above: second, absolute bound
                    timespec t1;
                    clock_gettime(CLOCK_MONOTONIC, &t1);
                    if (queue_timeout_s > 0.0 &&
                        (double)(t1.tv_sec - t_entry.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t_entry.tv_nsec) > queue_timeout_s)
                        return fail(GGR_E_HIP, "num_rendered read-back: the stream's earlier work has not finished within %.0f s "
                                               "(GGR_READBACK_QUEUE_TIMEOUT_S); frame not rendered", queue_timeout_s);
                }
                __builtin_ia32_pause();
                continue;
            }
            timespec t1;
            clock_gettime(CLOCK_MONOTONIC, &t1);
            if (timeout_s > 0.0 && (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec) > timeout_s)
                return fail(GGR_E_HIP, "num_rendered read-back: no answer from the GPU within %.0f s of the tile-list kernels' turn "
                                       "(GGR_READBACK_TIMEOUT_S); frame not rendered", timeout_s);
        }
        __builtin_ia32_pause();
    }
    if (v == GGR_READBACK_ARMED) return fail(GGR_E_HIP, "num_rendered read-back: the tile-list kernel ended without writing the count");
    *value = v;
    return GGR_OK;
}
hipError_t query_event(void* ev) { return hipEventQuery((hipEvent_t)ev); }

InputForm input_form(const GgrSettings* st, const GgrForwardIn* in, int sets, const void* dL_dshs = nullptr) {
    InputForm f;
    // flat float4 staging of odd-length SH rows needs every set's rows (and gradient rows) to start 16-B aligned
    f.sh_aligned = (((uintptr_t)in->shs | (uintptr_t)dL_dshs) & 15) == 0 &&
                   (sets <= 1 || ((int64_t)st->num_points * st->sh_stride * 3) % 4 == 0);
    f.cov_stride = in->cov3D_full ? 9 : 6;
    f.sh_channel_major = in->sh_channel_major ? 1 : 0;
    f.aux_affine = (in->aux_affine && !in->aux_precomp) ? 1 : 0;
    f.aux_a = in->aux_a;
    f.aux_b = in->aux_b;
    f.sh_cap = st->sh_max_degree == 4 ? 4 : 3;  // default 3: INTEGRATION.md §7
    f.tight_rects = st->reference_rects ? 0 : 1;
    const int gx = (st->image_width + GGR_TILE - 1) / GGR_TILE, gy = (st->image_height + GGR_TILE - 1) / GGR_TILE;
    f.sc_x0 = 0; f.sc_y0 = 0; f.sc_x1 = gx; f.sc_y1 = gy;
    const int32_t* sc = st->scissor;
    if (sc[0] | sc[1] | sc[2] | sc[3]) {   // the tiles that overlap the pixel window (validate() checked its shape)
        f.sc_x0 = min(gx, sc[0] / GGR_TILE); f.sc_y0 = min(gy, sc[1] / GGR_TILE);
        f.sc_x1 = min(gx, (sc[2] + GGR_TILE - 1) / GGR_TILE); f.sc_y1 = min(gy, (sc[3] + GGR_TILE - 1) / GGR_TILE);
    }
    return f;
}

size_t tiles_of(int W, int H) { return (size_t)((W + GGR_TILE - 1) / GGR_TILE) * ((H + GGR_TILE - 1) / GGR_TILE); }

// the reference's call: one camera, taken from the settings
ViewSet single_view(const GgrSettings* st, const GgrForwardIn* in) {
    ViewSet vs;
    vs.V = 1; vs.sets = 1; vs.vps = 1;
    vs.view = st->viewmatrix; vs.proj = st->projmatrix; vs.campos = st->campos; vs.bg = st->bg;
    vs.tanfov = st->tanfov_dev; vs.input_scale = in->input_scale;
    vs.tanfovx = st->tanfovx; vs.tanfovy = st->tanfovy;
    return vs;
}

int view_set(const GgrSettings* st, const GgrViews* v, ViewSet* vs) {
    if (!v || v->num_views < 1) return fail(GGR_E_INVALID, "GgrViews: num_views must be >= 1");
    if (!v->viewmatrix || !v->projmatrix || !v->campos || !v->bg)
        return fail(GGR_E_INVALID, "GgrViews: null camera array");
    const int64_t V = v->num_views;
    const int64_t sets = v->num_sets > 1 ? v->num_sets : 1;
    if (V % sets != 0) return fail(GGR_E_INVALID, "GgrViews: num_views must be a multiple of num_sets");
    if (sets > GGR_SORT_MAX_SEGMENTS) return fail(GGR_E_LIMIT, "GgrViews: at most 64 Gaussian sets per launch set");
    const int64_t gy = (st->image_height + GGR_TILE - 1) / GGR_TILE;
    if (V * st->num_points >= 0x7FFFFFFFll) return fail(GGR_E_LIMIT, "num_views x num_points too large");
    if (V * gy > 65535) return fail(GGR_E_LIMIT, "num_views x tile rows exceeds 65535");
    if (V * (int64_t)tiles_of(st->image_width, st->image_height) > (1 << 24)) return fail(GGR_E_LIMIT, "more than 2^24 tiles over all views");
    vs->V = (int)V; vs->sets = (int)sets; vs->vps = (int)(V / sets);
    vs->view = v->viewmatrix; vs->proj = v->projmatrix; vs->campos = v->campos; vs->bg = v->bg;
    vs->tanfov = v->tanfov; vs->input_scale = v->input_scale;
    vs->tanfovx = st->tanfovx; vs->tanfovy = st->tanfovy;
    return GGR_OK;
}

}  // namespace

extern "C" {

int ggr_abi_version(void) { return GGR_ABI_VERSION; }
// the sha256 of the sources this library was compiled from (ggrt_official_amd/_build.py source_hash(): the build passes
// it as -DGGR_SOURCE_HASH).  The marker in front lets the build read it from the file's bytes without loading it.
#ifndef GGR_SOURCE_HASH
#define GGR_SOURCE_HASH "0000000000000000000000000000000000000000000000000000000000000000"
#endif
const char* ggr_source_hash(void) {
    static const char tagged[] = "ggr-source-hash:" GGR_SOURCE_HASH;
    return tagged + 16;
}
const char* ggr_last_error(void) { return g_err; }

size_t ggr_geom_bytes(int32_t P) { return ggr_carve_geom(nullptr, (size_t)(P > 0 ? P : 0)).bytes; }
size_t ggr_image_bytes(int32_t W, int32_t H) { return ggr_carve_image(nullptr, W, H).bytes; }
size_t ggr_binning_bytes(int64_t N, int32_t, int32_t) { return ggr_point_list_bytes((size_t)(N > 0 ? N : 0)); }
size_t ggr_work_bytes(int32_t P, int32_t W, int32_t H) {
    return ggr::plan_tile_lists((size_t)(P > 0 ? P : 0), tiles_of(W, H)).work_bytes;
}
size_t ggr_backward_scratch_bytes(int32_t P) { return ggr_carve_bwd(nullptr, (size_t)(P > 0 ? P : 0)).bytes; }

}  // extern "C"

namespace {

// forward of V views of the same P Gaussians (V = 1: ggr_forward).  All per-Gaussian state is per (view, Gaussian),
// the tiles of the views are stacked (ggr_common.h ViewSet): one preprocess launch, ONE depth sort over the V·P keys,
// one tile-list build over the V·T tiles, one blend launch.
int forward_impl(const GgrSettings* st, const ViewSet& vs, const GgrForwardIn* in, GgrForwardOut* out, GgrAllocFn alloc,
                 void* alloc_ctx, void* stream, int antialiasing, float* out_alpha) {
    if (!out || !out->out_color || !out->geom_buffer || !out->image_buffer || !alloc)
        return fail(GGR_E_INVALID, "null output / buffer / allocator");
    if (st->num_points > 0 && !out->radii) return fail(GGR_E_INVALID, "null radii");
    hipStream_t s = (hipStream_t)stream;
    const int P1 = st->num_points, W = st->image_width, H = st->image_height, NV = vs.V;
    const int P = P1 * NV;                      // (view, Gaussian) pairs
    const int gx = (W + GGR_TILE - 1) / GGR_TILE;
    const size_t tiles = tiles_of(W, H) * (size_t)NV;
    const bool dbg = st->debug != 0;

    const size_t segs = ggr_sort_segments((size_t)NV);  // the depth sort runs one segment per view
    // (no_backward: the caller may have brought the smaller ggr_geom_bytes_inference buffer — nothing beyond it is touched)
    GeomLayout g = ggr_carve_geom(out->geom_buffer, (size_t)P, segs, /*with_jac=*/out->no_backward == 0);
    ImageLayout im = ggr_carve_image(out->image_buffer, W, H, NV);
    StageTimer tm(s, out->stage_ms, GGR_FWD_STAGES);

    // How the lists get their depth order (GgrSettings.depth_sort; tile_sort.hip).  Per tile: no global depth sort — the
    // tile-list builder walks the Gaussians in id order and every tile's list is sorted on its own afterwards.  A list longer
    // than GGR_TSORT_CAP_LARGE cannot be sorted that way: with a read-back (exact mode, capacity_is_hint) the call then
    // rebuilds the lists with the global sort; the pure sync-free mode has no read-back, so AUTO keeps the global sort there.
    const bool sync_free = out->binning_capacity > 0 && out->binning_buffer != nullptr;
    const bool hinted = sync_free && out->capacity_is_hint != 0;   // exact mode with a guessed buffer: N is awaited at the END
    if (out->binning_capacity >= 0x7FFFFFFF) return fail(GGR_E_LIMIT, "binning_capacity too large");
    int depth_sort = st->depth_sort;
    // The global sort has two forms (binning.hip): three stable passes, or ONE partition pass into depth buckets + every bucket
    // sorted in LDS.  The bucket form can meet a bucket it cannot sort (> 8192 different keys inside 1/4096 of the frame's
    // depth range): it says so through the read-back and the call then sorts again in three passes — so it needs a read-back,
    // like the per-tile form.  GGR_DEPTH_SORT_NO_BUCKETS (or GGR_GLOBAL_SORT=3pass) keeps the three passes.
    bool three_pass = (depth_sort & GGR_DEPTH_SORT_NO_BUCKETS) != 0;
    depth_sort &= ~GGR_DEPTH_SORT_NO_BUCKETS;
    if (const char* e = getenv("GGR_DEPTH_SORT")) {   // dev / A-B override of AUTO (read per call): "global" | "per_tile"
        if (depth_sort == GGR_DEPTH_SORT_AUTO && *e)
            depth_sort = (*e == 'g' || *e == '1') ? GGR_DEPTH_SORT_GLOBAL : (*e == 'p' || *e == '2') ? GGR_DEPTH_SORT_PER_TILE : depth_sort;
    }
    if (const char* e = getenv("GGR_GLOBAL_SORT")) { if (*e == '3' || *e == 'l') three_pass = true; }   // dev / A-B: "3pass" | "buckets"
    // AUTO: per tile where its lists are short — at most 256 (view, Gaussian) pairs per tile on average (a 1080p frame with 1 M
    // Gaussians: 123; its longest list: 1 100 entries) and, when the caller knows, a longest list of at most 4096 entries — and
    // the call has a read-back to fall back with.  Measured (NOTES r6, fwd+bwd): C3 0.78 against 0.80 ms, 200 k Gaussians at
    // 504 × 378 0.22 against 0.30; GGRt's own shapes — 1 M pixel-aligned Gaussians on 660 tiles, every list 4 000-6 000 entries —
    // 0.77 against 0.69: those keep the global sort.
    const uint32_t len_hint_in = out->max_list_len > 0 ? (uint32_t)out->max_list_len : 0u;
    if (depth_sort == GGR_DEPTH_SORT_AUTO)
        depth_sort = ((!sync_free || hinted) && (size_t)P <= 256 * tiles && len_hint_in <= 4096) ? GGR_DEPTH_SORT_PER_TILE
                                                                                             : GGR_DEPTH_SORT_GLOBAL;
    bool per_tile = depth_sort == GGR_DEPTH_SORT_PER_TILE && P > 0 && tiles > 0;
    const bool buckets = !three_pass && (!sync_free || hinted) && P > 0 && ggr::radix_sort_buckets_ok((size_t)P / segs);
    out->depth_sort_used = per_tile ? GGR_DEPTH_SORT_PER_TILE : buckets ? GGR_DEPTH_SORT_GLOBAL : GGR_DEPTH_SORT_GLOBAL_3PASS;
    const uint32_t len_hint = len_hint_in;
    out->max_list_len = -1;

    const ggr::TileListPlan plan = ggr::plan_tile_lists((size_t)P, tiles);
    // (per tile: the id-order scatter writes (id, key) entries that the per-tile sort reads — 8 B per list entry of scratch.
    //  With the list buffer's size known up front it rides on the work area; in the exact mode on the list buffer's tail)
    const size_t pairs_up_front = (per_tile && sync_free) ? ggr_pair_list_bytes((size_t)out->binning_capacity) : 0;
    void* work = alloc(alloc_ctx, plan.work_bytes + pairs_up_front);  // 1st allocator call: transient work area
    if (!work) return fail(GGR_E_ALLOC, "work-area allocator returned NULL");
    uint2* pair_list = pairs_up_front ? (uint2*)((char*)work + plan.work_bytes) : nullptr;
    uint2* rect_sorted = nullptr;
    uint32_t *totals_area = nullptr, totals_words = 0;   // the tile-list builder's per-tile / per-group totals (start from zero)
    ggr::tile_list_gather_targets(plan, work, tiles, &rect_sorted, &totals_area, &totals_words);

    // 1. per-Gaussian projection.  With SH colours the stage is split (preprocess.hip PART): the geometry half runs here, in
    //    front of the depth sort; the colour half — the SH rows, 4/5 of the stage's bytes, needed by the blend only — runs on
    //    the side stream beside the latency-bound sort / tile-list kernels (which leave HBM and most CUs idle) and is joined
    //    in front of the blend.  Not while the caller's stream is being captured into a graph (a thread-local side stream
    //    would be pulled into the capture), not in debug mode (one kernel at a time), not for precomputed colours.
    InputForm inf = input_form(st, in, vs.sets);
    inf.antialiasing = antialiasing;   // (preprocess_fwd also records it in the geometry buffer for the backward)
    SideStream* side = nullptr;
    // … nor for more than GGR_SPLIT_MAX_POINTS Gaussians per set: the colour kernel's bytes grow with them faster than the
    // window beside the binning does (C6′, 4.9 M Gaussians of 25 coefficients: 1.9 GB to move within ≈ 0.47 ms — at that rate
    // the depth sort beside it takes 0.66 instead of 0.29 ms; step 2.43 ms as one kernel, 2.51 split)
    // … nor per tile: beside the tile counts and the scatter the colour kernel costs them what it saves (count +22, scatter +12 µs
    // at C3), beside the per-tile sort it takes twice its time and the blend waits for it (NOTES r6)
    if (in->shs && P1 > 0 && P1 <= GGR_SPLIT_MAX_POINTS && !dbg && split_colour_enabled() &&
        (!per_tile || getenv("GGR_COLOUR_FORK") != nullptr)) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone) side = side_stream(s);
        else (void)hipGetLastError();
    }
    // (per tile: the kernel also clears the tile-list totals — the depth sort's last pass does it otherwise — and leaves the
    //  sort's work area alone)
    ggr::launch_preprocess_fwd(P1, st->sh_degree, st->sh_stride, in->means3D, in->shs, in->colors_precomp,
                               in->opacities, in->scales, in->rotations, st->scale_modifier, in->cov3D_precomp,
                               in->aux_precomp, vs, W, H, out->radii, g, inf, s, side ? GGR_PRE_GEOMETRY : GGR_PRE_ALL, 0,
                               out->no_backward ? 0 : 1, per_tile ? totals_area : nullptr, per_tile ? totals_words : 0u,
                               per_tile ? 1 : 0);
    KCHECK(dbg, s, "preprocess_fwd");
    bool colour_pending = side != nullptr;
    auto fork_colour = [&]() -> int {   // the colour kernel behind everything queued on `s` so far, on the side stream
        if (!colour_pending) return GGR_OK;
        colour_pending = false;
        HIP_TRY(hipEventRecord(side->fork, s));
        HIP_TRY(hipStreamWaitEvent(side->stream, side->fork, 0));
        // (the launch's grid is (blocks, Gaussian sets): the persistent blocks are shared out between the sets)
        const int cg = colour_grid_blocks((size_t)P);
        const int colour_grid = cg <= 0 ? 0 : std::max(1, cg / std::max(1, vs.sets));
        if (out->stage_ms) (void)hipEventRecord(side->t0, side->stream);
        ggr::launch_preprocess_fwd(P1, st->sh_degree, st->sh_stride, in->means3D, in->shs, in->colors_precomp,
                                   in->opacities, in->scales, in->rotations, st->scale_modifier, in->cov3D_precomp,
                                   in->aux_precomp, vs, W, H, out->radii, g, inf, side->stream, GGR_PRE_COLOUR,
                                   colour_grid, out->no_backward ? 0 : 1);
        if (out->stage_ms) (void)hipEventRecord(side->t1, side->stream);
        HIP_TRY(hipEventRecord(side->join, side->stream));
        return GGR_OK;
    };
    // (started right behind the geometry kernel: started behind the depth sort, or behind the tile counts, it delays the
    //  blend by more than it spares the sort — NOTES r5)
    int colour_fork_at = 0;   // 0: behind the geometry kernel, 1: behind the tile counts, 2: behind the scatter (dev: NOTES r6)
    if (const char* e = getenv("GGR_COLOUR_FORK")) { if (*e >= '0' && *e <= '2') colour_fork_at = *e - '0'; }
    if (colour_fork_at == 0) { const int rc = fork_colour(); if (rc != GGR_OK) return rc; }
    // (every return below this point must leave the caller's stream ordered behind the side stream: JoinGuard.  The guard
    //  also covers a colour kernel that was never started: join() launches it first)
    struct JoinGuard {
        SideStream* sd; hipStream_t s; bool done = false;
        void join() { if (sd && !done) { (void)hipStreamWaitEvent(s, sd->join, 0); done = true; } }
        ~JoinGuard() { join(); }
    } joiner{side, s};
    auto fork_colour_at = [&](int where) -> int { return (colour_pending && colour_fork_at == where) ? fork_colour() : GGR_OK; };
    tm.mark(GGR_FWD_PREPROCESS);

    // sync-free mode: the caller brought a list buffer of `binning_capacity` entries → no read-back, no host
    // sync, no second allocator call; the whole forward (and backward) is then hipGraph-capturable
    uint32_t capacity = sync_free ? (uint32_t)out->binning_capacity : 0xFFFFFFFFu;
    // exact mode: num_rendered travels to the host through a pinned word written by the scan kernel, with an
    // event right behind that kernel — the host wakes up while the last scan kernel still runs and has the list
    // buffer allocated and the scatter queued by the time the GPU gets there (a device→host memcpy into pageable
    // memory + stream sync left the GPU idle for that long)
    ReadbackSlot* rb = ((!sync_free || hinted) && P > 0) ? readback_slot() : nullptr;
    const uint32_t* sort_fault = ggr::radix_sort_fault_word(g.hist);

    // ---- the pieces of the list build --------------------------------------------------------------------------------
    // 2. stable sort of the Gaussians by depth bits (ties keep ascending id).  Its last pass also drops every
    //    Gaussian's tile rect at its sorted position (into the tile-list work area) and clears the per-tile totals.
    uint32_t *dk = nullptr, *order = nullptr;
    auto global_sort = [&](bool area_cleared, bool bucket_form) {
        // (preprocess already wrote the keys into g.keys_a; the values are the identity, formed by the sort's first pass)
        ggr::radix_sort_pairs(g.keys_a, g.keys_b, g.vals_a, g.vals_b, g.hist, (size_t)P, (uint32_t)segs, &dk, &order, s,
                              /*hist_zeroed=*/area_cleared /*by preprocess_fwd*/,
                              /*block_max_ready=*/(uint32_t)((P1 + GGR_PRE_THREADS - 1) / GGR_PRE_THREADS) * (uint32_t)vs.sets /*likewise*/,
                              /*identity_vals=*/true /*preprocess_fwd writes no values: the first pass forms them*/,
                              g.rect, rect_sorted, totals_area, totals_words, bucket_form);
    };
    // 3. per-(chunk, tile) counts → list positions, tile ranges, num_rendered (+ the longest list)
    auto count_pass = [&](bool id_order, bool to_host) {
        if (to_host && rb) {
            ((volatile uint32_t*)rb->host)[1] = 0u;
            *(volatile uint32_t*)rb->host = GGR_READBACK_ARMED;
            (void)hipEventRecord(rb->ev_start, s);
        }
        ggr::launch_tile_list_count(plan, (size_t)P, tiles, gx, order, g.rect, work, im.ranges, g.counters, capacity, s,
                                    /*rects_gathered=*/true, (to_host && rb) ? rb->host : nullptr, (to_host && rb) ? rb->ev : nullptr,
                                    id_order ? nullptr : sort_fault, id_order, id_order ? GGR_TSORT_CAP_LARGE : 0xFFFFFFFFu);
    };
    // 4. in-order scatter of the ids into the per-tile lists (+ per tile: the depth order, list by list)
    uint32_t* point_list = nullptr;
    uint32_t sorted_upto = 0;   // per tile: lists of up to this many entries have been depth-sorted in `point_list`
    // the per-tile sort of the lists with sorted_upto < length <= upto: one launch per length class it spans (tile_sort.hip)
    auto tile_sort_upto = [&](uint32_t upto) {
        upto = std::min<uint32_t>(upto, GGR_TSORT_CAP_LARGE);
        if (upto <= sorted_upto) return;
        // One launch when a class with at least four workgroups per CU covers everything (lists up to 3072 entries: a few tiles
        // just beyond 2048 do not pay for a launch of their own); otherwise the lists up to 2048 in their class and the
        // longer ones in theirs.  The launch with the largest class also copies the ids of lists beyond it: unsorted, but
        // nothing uninitialised is left for the blend.
        const uint32_t one_launch = 3072;
        if (upto <= one_launch || sorted_upto >= GGR_TSORT_CAP_SMALL) {
            ggr::launch_tile_depth_sort(tiles, im.ranges, point_list, pair_list, sorted_upto, upto, s, 1, g.counters + 3);
        } else {
            ggr::launch_tile_depth_sort(tiles, im.ranges, point_list, pair_list, sorted_upto, GGR_TSORT_CAP_SMALL, s, 0, g.counters + 3);
            ggr::launch_tile_depth_sort(tiles, im.ranges, point_list, pair_list, GGR_TSORT_CAP_SMALL, upto, s, 1, g.counters + 3);
        }
        sorted_upto = upto;
    };
    auto scatter_pass = [&](bool id_order, uint32_t cap_entries, uint32_t expect_longest) {
        ggr::launch_tile_list_scatter(plan, (size_t)P, tiles, gx, id_order ? nullptr : order, g.rect, work, point_list,
                                      cap_entries, s, id_order ? g.keys_a : nullptr, id_order ? pair_list : nullptr);
        tm.mark(GGR_FWD_TILE_SCATTER);
        (void)fork_colour_at(2);
        sorted_upto = 0;
        if (id_order) {
            tile_sort_upto(expect_longest);
            tm.mark(GGR_FWD_TILE_SORT);
        }
    };
    // 5. blend (clears the caller's backward scratch on the side; an image without tiles launches nothing)
    const bool scissored = (st->scissor[0] | st->scissor[1] | st->scissor[2] | st->scissor[3]) != 0;
    auto blend_pass = [&]() {
        if (colour_pending) (void)fork_colour();   // (a frame without list entries: nothing started it yet)
        joiner.join();   // the colour records (side stream) are complete before the blend reads them
        ggr::launch_blend_fwd(W, H, im.ranges, point_list, g.splat, g.colour, vs.bg, out->out_color, out->no_backward ? nullptr : im.final_T,
                              im.n_contrib, out->out_depth, out_alpha, out->no_backward ? nullptr : im.ckpt, im.ckpt_slots, im.tile_top, NV,
                              scissored ? 1 : 0, out->backward_scratch, ggr_carve_bwd(nullptr, (size_t)P1, (size_t)NV).bytes, s);
    };
    // what the host word(s) said: N, or a fault; the longest list
    uint32_t num_rendered = 0, longest = 0;
    bool bucket_fault = false;   // the depth sort's bucket form left a bucket unsorted: the lists must be built again
    bool bucket_slow = false;    // … or sorted everything, much of it the slow way: advisory (GGR_DEPTH_SORT_GLOBAL_SLOW)
    auto read_counts = [&]() -> int {
        if (rb) {
            // the single host sync of forward.  N is written by the FIRST block of the last tile-list kernel: the host
            // watches the pinned word instead of waiting for that kernel's end (wait_readback above)
            const int rc = wait_readback((volatile uint32_t*)rb->host, query_event, (void*)rb->ev, readback_timeout_s(), &num_rendered,
                                         query_event, (void*)rb->ev_start);
            if (rc != GGR_OK) return rc;
            longest = ((volatile uint32_t*)rb->host)[1];   // (stored before N's release store)
            bucket_fault = (longest >> 31) != 0u;
            bucket_slow = ((longest >> 30) & 1u) != 0u;
            longest &= 0x3FFFFFFFu;
        } else {   // no pinned slot (hipHostMalloc / hipEventCreate failed): copy + sync — a frame is never returned unchecked
            uint32_t w4[4] = {0u, 0u, 0u, 0u};
            HIP_TRY(hipMemcpyAsync(w4, g.counters, 16, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            num_rendered = (w4[1] & 2u) ? GGR_HOST_FAULT_SPIN : (w4[1] & 4u) ? GGR_HOST_FAULT_RANGE : w4[0];
            longest = w4[2];
            bucket_fault = (w4[1] & 16u) != 0u;
            bucket_slow = (w4[1] & 32u) != 0u;
        }
        // raised by the tile-list kernel that writes N (bin_group_prefix_kernel)
        if (num_rendered == GGR_HOST_FAULT_SPIN) return fail(GGR_E_HIP, "%s", kSpinFault);
        if (num_rendered == GGR_HOST_FAULT_RANGE) return fail(GGR_E_LIMIT, "%s", kRangeFault);
        if (num_rendered >= 0x7FFFFFFFu) return fail(GGR_E_LIMIT, "num_rendered %u too large", num_rendered);
        out->num_rendered = (int64_t)num_rendered;
        out->max_list_len = (int32_t)longest;
        return GGR_OK;
    };
    // a list too long for the per-tile sort: the lists once more, through the global depth sort (the counts restart from zero:
    // the sort's last pass clears the totals; its own work area was left untouched by preprocess_fwd)
    bool rebuilt = false;
    auto rebuild_global = [&]() {
        out->depth_sort_used = per_tile ? GGR_DEPTH_SORT_GLOBAL_3PASS : GGR_DEPTH_SORT_GLOBAL_FELL_BACK;
        per_tile = false;
        rebuilt = true;
        global_sort(/*area_cleared=*/false, /*bucket_form=*/false);
        tm.mark(GGR_FWD_DEPTH_SORT);
        count_pass(/*id_order=*/false, /*to_host=*/false);
        tm.mark(GGR_FWD_TILE_COUNT);
    };

    if (P > 0 && tiles > 0) {
        if (!per_tile) {
            global_sort(/*area_cleared=*/true, buckets);
            KCHECK(dbg, s, "depth sort");
        }
        tm.mark(GGR_FWD_DEPTH_SORT);
        count_pass(per_tile, /*to_host=*/true);
    } else {
        tm.mark(GGR_FWD_DEPTH_SORT);
        HIP_TRY(hipMemsetAsync(im.ranges, 0, (tiles ? tiles : 1) * sizeof(uint2), s));
        HIP_TRY(hipMemsetAsync(g.counters, 0, 16, s));
        rb = nullptr;
    }
    KCHECK(dbg, s, "tile_list_count");
    { const int rc = fork_colour_at(1); if (rc != GGR_OK) return rc; }
    if (dbg && sync_free && P > 0 && tiles > 0) {  // debug mode may sync: check the sort's fault bit right here
        uint32_t two[2] = {0u, 0u};
        HIP_TRY(hipMemcpy(two, g.counters, 8, hipMemcpyDeviceToHost));
        if (two[1] & 2u) return fail(GGR_E_HIP, "%s", kSpinFault);
        if (two[1] & 4u) return fail(GGR_E_LIMIT, "%s", kRangeFault);
    }
    if (!sync_free) {
        if (P > 0 && tiles > 0) { const int rc = read_counts(); if (rc != GGR_OK) return rc; }
        else { out->num_rendered = 0; out->max_list_len = 0; }
        tm.mark(GGR_FWD_TILE_COUNT);
        if ((per_tile && longest > GGR_TSORT_CAP_LARGE) || (!per_tile && bucket_fault)) rebuild_global();
        // 2nd call: kept for backward (per tile: + the (id, key) scratch on its tail)
        void* bin_mem = alloc(alloc_ctx, ggr_point_list_bytes(num_rendered) + (per_tile ? ggr_pair_list_bytes(num_rendered) : 0));
        if (!bin_mem) return fail(GGR_E_ALLOC, "binning allocator returned NULL");
        out->binning_buffer = bin_mem;
        point_list = (uint32_t*)bin_mem;
        if (per_tile) pair_list = (uint2*)((char*)bin_mem + ggr_point_list_bytes(num_rendered));
    } else {
        out->num_rendered = -1;  // known on the device only: ggr_forward_status reads it (and the overflow flag)
        tm.mark(GGR_FWD_TILE_COUNT);
        point_list = (uint32_t*)out->binning_buffer;
    }
    if (P > 0 && tiles > 0 && (sync_free || num_rendered > 0)) {
        // (how long the lists are that the per-tile sort is launched for: known in the exact mode, the caller's guess with a
        //  guessed buffer — checked and repaired at the end —, everything it can take in the pure sync-free mode)
        const uint32_t expect = !sync_free ? longest : hinted ? (len_hint ? len_hint : GGR_TSORT_CAP_SMALL) : GGR_TSORT_CAP_LARGE;
        scatter_pass(per_tile, capacity, expect);
        KCHECK(dbg, s, "tile_list_scatter");
    } else {
        tm.mark(GGR_FWD_TILE_SCATTER);
    }

    if (out->backward_scratch && tiles == 0)
        HIP_TRY(hipMemsetAsync(out->backward_scratch, 0, ggr_carve_bwd(nullptr, (size_t)P1, (size_t)NV).bytes, s));
    blend_pass();
    KCHECK(dbg, s, "blend_fwd");
    tm.mark(GGR_FWD_BLEND);
    if (hinted && P > 0 && tiles > 0) {   // num_rendered, while the device works on scatter and blend; the guesses must have held
        out->num_rendered = 0;
        { const int rc = read_counts(); if (rc != GGR_OK) return rc; }
        const bool cut = num_rendered > capacity;
        const bool too_long = (per_tile && longest > GGR_TSORT_CAP_LARGE) || (!per_tile && bucket_fault);   // → the lists once more, three-pass global sort
        const bool unsorted_left = per_tile && !too_long && longest > sorted_upto;   // the length guess was too small
        if (cut) {
            // The guess did not hold.  Everything up to the tile ranges is valid (the counts do not depend on the list
            // buffer); only the ranges and the lists were cut at the guessed capacity and the blend ran on cut lists.  With an allocator at hand the call repairs
            // itself: the exact buffer (the allocator's second call, as in the exact mode), the tile ranges, the scatter and the blend once
            // more — 0.21 ms at C3 instead of a whole second forward (round 5; until then GGR_E_CAPACITY and the host
            // repeated the call: 1.25 instead of 0.90 ms).  capacity_is_hint = 2 tells the host that this happened.
            void* bin_mem = alloc ? alloc(alloc_ctx, ggr_point_list_bytes(num_rendered) +
                                                         ((per_tile && !too_long) ? ggr_pair_list_bytes(num_rendered) : 0)) : nullptr;
            if (!bin_mem)
                return fail(GGR_E_CAPACITY, "num_rendered %u exceeds the hinted capacity %u", num_rendered, capacity);
            if (per_tile && !too_long) pair_list = (uint2*)((char*)bin_mem + ggr_point_list_bytes(num_rendered));
            out->binning_buffer = bin_mem;
            out->binning_capacity = (int64_t)num_rendered;
            out->capacity_is_hint = 2;
            point_list = (uint32_t*)bin_mem;
            capacity = 0xFFFFFFFFu;
        }
        if (too_long) {
            rebuild_global();    // (also rewrites the ranges, uncut)
        } else if (cut) {
            ggr::launch_tile_list_ranges(plan, tiles, work, im.ranges, s);   // (they were cut at the guessed capacity)
            // … which also leaves the status word's overflow bit standing: cleared below
        }
        if (cut || too_long) {
            if (!too_long) {
                HIP_TRY(hipMemsetAsync(g.counters + 1, 0, 4, s));   // the frame is complete after all (ggr_forward_status)
                HIP_TRY(hipMemsetAsync(g.counters + 3, 0, 4, s));   // (the per-tile sort below counts its slow route anew)
            }
            scatter_pass(per_tile, 0xFFFFFFFFu, longest);
            KCHECK(dbg, s, "tile_list_scatter (repair)");
        } else if (unsorted_left) {
            tile_sort_upto(longest);
            KCHECK(dbg, s, "tile_depth_sort (repair)");
        }
        if (cut || too_long || unsorted_left) {
            if (!cut) out->capacity_is_hint = 3;   // repaired for the list LENGTH guess alone: the caller's buffer stays
            blend_pass();
            KCHECK(dbg, s, "blend_fwd (repair)");
        }
    } else if (hinted) {
        out->num_rendered = 0;
        out->max_list_len = 0;
    }
    if (rebuilt) {   // the global sort of the rebuild ran behind the read-back: its fault word is checked here (rare path: one sync)
        uint32_t two[2] = {0u, 0u};
        HIP_TRY(hipMemcpyAsync(two, g.counters, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (two[1] & 2u) return fail(GGR_E_HIP, "%s", kSpinFault);
        if (two[1] & 4u) return fail(GGR_E_LIMIT, "%s", kRangeFault);
    }
    if (bucket_slow && out->depth_sort_used == GGR_DEPTH_SORT_GLOBAL) out->depth_sort_used = GGR_DEPTH_SORT_GLOBAL_SLOW;
    tm.finish();
    if (out->stage_ms && side) {   // the colour kernel's own duration (it ran BESIDE stages 1-3, not in addition to them)
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, side->t0, side->t1) == hipSuccess) out->stage_ms[GGR_FWD_COLOUR] += ms;
        else (void)hipGetLastError();
    }
    return GGR_OK;
}

int backward_impl(const GgrSettings* st, const ViewSet& vs, const GgrBackwardIn* in, GgrBackwardOut* out, void* stream,
                  const float* dL_dalpha, float* dL_dtanfov) {
    if (!out) return fail(GGR_E_INVALID, "null gradient output struct");
    const int NV = vs.V;
    if (dL_dtanfov && (!out->dL_dviewmatrix || !out->dL_dprojmatrix || !out->dL_dcampos))
        return fail(GGR_E_INVALID, "dL_dtanfov needs the three camera gradient outputs (dL_dviewmatrix, dL_dprojmatrix, dL_dcampos)");
    if (st->num_points == 0) {  // nothing to differentiate; camera gradients are zero
        hipStream_t s0 = (hipStream_t)stream;
        if (out->dL_dviewmatrix) HIP_TRY(hipMemsetAsync(out->dL_dviewmatrix, 0, 64 * (size_t)NV, s0));
        if (out->dL_dprojmatrix) HIP_TRY(hipMemsetAsync(out->dL_dprojmatrix, 0, 64 * (size_t)NV, s0));
        if (out->dL_dcampos) HIP_TRY(hipMemsetAsync(out->dL_dcampos, 0, 12 * (size_t)NV, s0));
        if (dL_dtanfov) HIP_TRY(hipMemsetAsync(dL_dtanfov, 0, 8 * (size_t)NV, s0));
        return GGR_OK;
    }
    if (!out->dL_dmeans3D || !out->dL_dmeans2D || !out->dL_dopacities || !out->dL_dcov3D)
        return fail(GGR_E_INVALID, "null gradient output");
    if (!in->geom_buffer || !in->image_buffer || !in->scratch || !in->dL_dout_color)
        return fail(GGR_E_INVALID, "null saved buffer / scratch / upstream gradient");
    const bool has_cp = in->fwd.colors_precomp != nullptr;
    if (has_cp ? !out->dL_dcolors_precomp : !out->dL_dshs) return fail(GGR_E_INVALID, "null colour gradient output");
    const bool has_sr = in->fwd.scales != nullptr;
    if (has_sr && (!out->dL_dscales || !out->dL_drotations)) return fail(GGR_E_INVALID, "null scale/rotation gradient output");
    if (in->fwd.aux_precomp && in->dL_dout_depth && !out->dL_daux) return fail(GGR_E_INVALID, "null dL_daux output");
    const int npose = (out->dL_dviewmatrix != nullptr) + (out->dL_dprojmatrix != nullptr) + (out->dL_dcampos != nullptr);
    if (npose != 0 && npose != 3) return fail(GGR_E_INVALID, "camera gradients: give all three outputs or none");
    hipStream_t s = (hipStream_t)stream;
    const int P = st->num_points, W = st->image_width, H = st->image_height;
    const bool dbg = st->debug != 0;
    if (in->num_rendered != 0 && !in->binning_buffer) return fail(GGR_E_INVALID, "null binning buffer");

    GeomLayout g = ggr_carve_geom((void*)in->geom_buffer, (size_t)P * NV, ggr_sort_segments((size_t)NV));
    ImageLayout im = ggr_carve_image((void*)in->image_buffer, W, H, NV);
    const uint32_t* point_list = (const uint32_t*)in->binning_buffer;
    BwdScratch sc = ggr_carve_bwd(in->scratch, (size_t)P, (size_t)NV);

    StageTimer tm(s, out->stage_ms, GGR_BWD_STAGES);
    if (!in->scratch_zeroed)  // (else: this frame's forward cleared it inside its blend kernel)
        HIP_TRY(hipMemsetAsync(in->scratch, 0, sc.bytes, s));  // dL_dmeans2D / dL_dopacities are written by preprocess_bwd
    tm.mark(GGR_BWD_CLEAR);

    if (in->num_rendered != 0) {  // (-1: sync-free forward, count known on the device only)
        ggr::launch_blend_bwd(W, H, im.ranges, point_list, g.splat, g.colour, vs.bg, im.final_T, im.n_contrib,
                              in->dL_dout_color, in->dL_dout_depth, dL_dalpha, sc.grad2d, im.tile_top, im.ckpt,
                              im.ckpt_slots, im.bwd_segments, NV, s);
        KCHECK(dbg, s, "blend_bwd");
    }
    tm.mark(GGR_BWD_BLEND);
    const float* cov = in->fwd.cov3D_precomp ? in->fwd.cov3D_precomp : g.cov3D;
    ggr::launch_preprocess_bwd(P, st->sh_degree, st->sh_stride, in->fwd.means3D, in->fwd.shs, g.sh_jac, has_cp ? 1 : 0,
                               in->fwd.scales, in->fwd.rotations, st->scale_modifier, cov, vs, W, H, in->radii, g.clamped,
                               sc.grad2d, in->dL_dout_depth ? 1 : 0, out->dL_dmeans3D, out->dL_dmeans2D,
                               out->dL_dopacities, out->dL_dshs, out->dL_dcolors_precomp, out->dL_dcov3D,
                               out->dL_dscales, out->dL_drotations, in->fwd.aux_precomp ? out->dL_daux : nullptr,
                               npose ? sc.pose_acc : nullptr, out->dL_dviewmatrix, out->dL_dprojmatrix,
                               out->dL_dcampos, input_form(st, &in->fwd, vs.sets, out->dL_dshs), in->fwd.cov3D_precomp ? 1 : 0,
                               in->fwd.opacities, g.counters + GGR_CTR_ANTIALIAS /*the forward's mode*/, s, dL_dtanfov);
    KCHECK(dbg, s, "preprocess_bwd");
    tm.mark(GGR_BWD_PREPROCESS);
    return GGR_OK;
}

}  // namespace

extern "C" {

int ggr_forward_ext(const GgrSettings* st, const GgrForwardOptions* opt, const GgrForwardExtra* ex, const GgrForwardIn* in,
                    GgrForwardOut* out, GgrAllocFn alloc, void* alloc_ctx, void* stream) {
    g_err[0] = 0;
    int aa = 0;
    int rc = validate_options(opt, &aa);
    if (rc) return rc;
    if ((rc = validate_extra(ex, "GgrForwardExtra")) != 0) return rc;
    rc = validate(st, in);
    if (rc) return rc;
    return forward_impl(st, single_view(st, in), in, out, alloc, alloc_ctx, stream, aa, ex ? ex->out_alpha : nullptr);
}

int ggr_forward_opt(const GgrSettings* st, const GgrForwardOptions* opt, const GgrForwardIn* in, GgrForwardOut* out,
                    GgrAllocFn alloc, void* alloc_ctx, void* stream) {
    return ggr_forward_ext(st, opt, nullptr, in, out, alloc, alloc_ctx, stream);
}

int ggr_forward(const GgrSettings* st, const GgrForwardIn* in, GgrForwardOut* out, GgrAllocFn alloc,
                void* alloc_ctx, void* stream) {
    return ggr_forward_ext(st, nullptr, nullptr, in, out, alloc, alloc_ctx, stream);
}

int ggr_backward_ext(const GgrSettings* st, const GgrBackwardExtra* ex, const GgrBackwardIn* in, GgrBackwardOut* out,
                     void* stream) {
    g_err[0] = 0;
    int rc = validate_extra(ex, "GgrBackwardExtra");
    if (rc) return rc;
    if (!in) return fail(GGR_E_INVALID, "null inputs");
    rc = validate(st, &in->fwd);
    if (rc) return rc;
    return backward_impl(st, single_view(st, &in->fwd), in, out, stream, ex ? ex->dL_dout_alpha : nullptr, extra_dtanfov(ex));
}

int ggr_backward(const GgrSettings* st, const GgrBackwardIn* in, GgrBackwardOut* out, void* stream) {
    return ggr_backward_ext(st, nullptr, in, out, stream);
}

int ggr_forward_views_ext(const GgrSettings* st, const GgrForwardOptions* opt, const GgrForwardExtra* ex, const GgrViews* views,
                          const GgrForwardIn* in, GgrForwardOut* out, GgrAllocFn alloc, void* alloc_ctx, void* stream) {
    g_err[0] = 0;
    int aa = 0;
    int rc = validate_options(opt, &aa);
    if (rc) return rc;
    if ((rc = validate_extra(ex, "GgrForwardExtra")) != 0) return rc;
    rc = validate(st, in);
    if (rc) return rc;
    ViewSet vs;
    if ((rc = view_set(st, views, &vs)) != 0) return rc;
    return forward_impl(st, vs, in, out, alloc, alloc_ctx, stream, aa, ex ? ex->out_alpha : nullptr);
}

int ggr_forward_views_opt(const GgrSettings* st, const GgrForwardOptions* opt, const GgrViews* views, const GgrForwardIn* in,
                          GgrForwardOut* out, GgrAllocFn alloc, void* alloc_ctx, void* stream) {
    return ggr_forward_views_ext(st, opt, nullptr, views, in, out, alloc, alloc_ctx, stream);
}

int ggr_forward_views(const GgrSettings* st, const GgrViews* views, const GgrForwardIn* in, GgrForwardOut* out,
                      GgrAllocFn alloc, void* alloc_ctx, void* stream) {
    return ggr_forward_views_ext(st, nullptr, nullptr, views, in, out, alloc, alloc_ctx, stream);
}

int ggr_backward_views_ext(const GgrSettings* st, const GgrBackwardExtra* ex, const GgrViews* views, const GgrBackwardIn* in,
                           GgrBackwardOut* out, void* stream) {
    g_err[0] = 0;
    int rc = validate_extra(ex, "GgrBackwardExtra");
    if (rc) return rc;
    if (!in) return fail(GGR_E_INVALID, "null inputs");
    rc = validate(st, &in->fwd);
    if (rc) return rc;
    ViewSet vs;
    if ((rc = view_set(st, views, &vs)) != 0) return rc;
    return backward_impl(st, vs, in, out, stream, ex ? ex->dL_dout_alpha : nullptr, extra_dtanfov(ex));
}

int ggr_backward_views(const GgrSettings* st, const GgrViews* views, const GgrBackwardIn* in, GgrBackwardOut* out,
                       void* stream) {
    return ggr_backward_views_ext(st, nullptr, views, in, out, stream);
}

// ---- the feature pass (blend_feat.hip): replays of a forward's lists ------------------------------------------------------
namespace {
int feature_pass_check(const GgrSettings* st, const GgrViews* views, const GgrFeaturePass* fp, bool backward, int* V, int* vps) {
    if (!st || !fp) return fail(GGR_E_INVALID, "null settings / feature pass");
    if (fp->struct_size < (int32_t)sizeof(GgrFeaturePass))
        return fail(GGR_E_INVALID, "GgrFeaturePass.struct_size %d is smaller than the %d bytes of its fields", (int)fp->struct_size,
                    (int)sizeof(GgrFeaturePass));
    if (fp->reserved != 0) return fail(GGR_E_INVALID, "GgrFeaturePass.reserved must be 0, not %d", (int)fp->reserved);
    if (fp->num_features < 1 || fp->num_features > GGR_MAX_FEATURES)
        return fail(GGR_E_INVALID, "GgrFeaturePass.num_features must be 1..%d, not %d", GGR_MAX_FEATURES, (int)fp->num_features);
    if (st->num_points < 0 || st->image_width < 0 || st->image_height < 0) return fail(GGR_E_INVALID, "negative size");
    if (!fp->out_features) return fail(GGR_E_INVALID, "GgrFeaturePass.out_features is NULL");
    if (!fp->geom_buffer || !fp->image_buffer) return fail(GGR_E_INVALID, "GgrFeaturePass: null geom / image buffer of the forward");
    if (st->num_points > 0 && !fp->features) return fail(GGR_E_INVALID, "GgrFeaturePass.features is NULL");
    if (fp->num_rendered != 0 && !fp->binning_buffer) return fail(GGR_E_INVALID, "GgrFeaturePass.binning_buffer is NULL");
    if (backward) {
        if (!fp->dL_dout_features) return fail(GGR_E_INVALID, "GgrFeaturePass.dL_dout_features is NULL");
        if (st->num_points > 0 && !fp->dL_dfeatures) return fail(GGR_E_INVALID, "GgrFeaturePass.dL_dfeatures is NULL");
        if (!fp->scratch) return fail(GGR_E_INVALID, "GgrFeaturePass.scratch is NULL");
    }
    *V = 1; *vps = 1;
    if (views) {
        if (views->num_views < 1) return fail(GGR_E_INVALID, "GgrViews: num_views must be >= 1");
        const int sets = views->num_sets > 1 ? views->num_sets : 1;
        if (views->num_views % sets != 0) return fail(GGR_E_INVALID, "GgrViews: num_views must be a multiple of num_sets");
        if ((int64_t)views->num_views * st->num_points >= 0x7FFFFFFFll) return fail(GGR_E_LIMIT, "num_views x num_points too large");
        if ((int64_t)views->num_views * (int64_t)tiles_of(st->image_width, st->image_height) > (1 << 24))
            return fail(GGR_E_LIMIT, "more than 2^24 tiles over all views");
        *V = views->num_views; *vps = views->num_views / sets;
    }
    return GGR_OK;
}
}  // namespace

int ggr_features_forward(const GgrSettings* st, const GgrViews* views, const GgrFeaturePass* fp, void* stream) {
    g_err[0] = 0;
    int V = 1, vps = 1;
    const int rc = feature_pass_check(st, views, fp, false, &V, &vps);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int P1 = st->num_points, W = st->image_width, H = st->image_height, K = fp->num_features;
    if ((size_t)W * H == 0) return GGR_OK;
    if (P1 == 0 || fp->num_rendered == 0) {   // no list entry anywhere: every plane is zero
        HIP_TRY(hipMemsetAsync(fp->out_features, 0, (size_t)V * K * W * H * sizeof(float), s));
        return GGR_OK;
    }
    GeomLayout g = ggr_carve_geom((void*)fp->geom_buffer, (size_t)P1 * V, ggr_sort_segments((size_t)V), /*with_jac=*/false);
    ImageLayout im = ggr_carve_image((void*)fp->image_buffer, W, H, V);
    const bool scissored = (st->scissor[0] | st->scissor[1] | st->scissor[2] | st->scissor[3]) != 0;
    ggr::launch_blend_feat_fwd(W, H, im.ranges, (const uint32_t*)fp->binning_buffer, g.splat, fp->features, K, P1, vps,
                               fp->out_features, V, scissored ? 1 : 0, s);
    KCHECK(st->debug != 0, s, "blend_feat_fwd");
    return GGR_OK;
}

int ggr_features_backward(const GgrSettings* st, const GgrViews* views, const GgrFeaturePass* fp, void* stream) {
    g_err[0] = 0;
    int V = 1, vps = 1;
    const int rc = feature_pass_check(st, views, fp, true, &V, &vps);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int P1 = st->num_points, W = st->image_width, H = st->image_height, K = fp->num_features;
    BwdScratch sc = ggr_carve_bwd(fp->scratch, (size_t)P1, (size_t)V);
    if (!fp->scratch_zeroed) HIP_TRY(hipMemsetAsync(fp->scratch, 0, sc.bytes, s));
    if (P1 == 0) return GGR_OK;
    HIP_TRY(hipMemsetAsync(fp->dL_dfeatures, 0, (size_t)(V / vps) * P1 * K * sizeof(float), s));
    if (fp->num_rendered == 0 || (size_t)W * H == 0) return GGR_OK;
    GeomLayout g = ggr_carve_geom((void*)fp->geom_buffer, (size_t)P1 * V, ggr_sort_segments((size_t)V), /*with_jac=*/false);
    ImageLayout im = ggr_carve_image((void*)fp->image_buffer, W, H, V);
    ggr::launch_blend_feat_bwd(W, H, im.ranges, (const uint32_t*)fp->binning_buffer, g.splat, fp->features, K, P1, vps,
                               fp->out_features, fp->dL_dout_features, fp->dL_dfeatures, sc.grad2d, V, s);
    KCHECK(st->debug != 0, s, "blend_feat_bwd");
    return GGR_OK;
}

// ---- the contribution pass (blend_contrib.hip): per-Gaussian statistics of the blend weight over a forward's lists -------------
int ggr_contributions(const GgrSettings* st, const GgrViews* views, const GgrContributionPass* cp, void* stream) {
    g_err[0] = 0;
    if (!st || !cp) return fail(GGR_E_INVALID, "null settings / contribution pass");
    if (cp->struct_size < (int32_t)sizeof(GgrContributionPass))
        return fail(GGR_E_INVALID, "GgrContributionPass.struct_size %d is smaller than the %d bytes of its fields",
                    (int)cp->struct_size, (int)sizeof(GgrContributionPass));
    if (cp->reserved != 0) return fail(GGR_E_INVALID, "GgrContributionPass.reserved must be 0, not %d", (int)cp->reserved);
    if (!cp->out_weight_sum && !cp->out_weight_max && !cp->out_pixel_count)
        return fail(GGR_E_INVALID, "GgrContributionPass: every output is NULL");
    if (st->num_points < 0 || st->image_width < 0 || st->image_height < 0) return fail(GGR_E_INVALID, "negative size");
    if (!cp->geom_buffer || !cp->image_buffer) return fail(GGR_E_INVALID, "GgrContributionPass: null geom / image buffer of the forward");
    if (cp->num_rendered != 0 && !cp->binning_buffer) return fail(GGR_E_INVALID, "GgrContributionPass.binning_buffer is NULL");
    int V = 1;
    if (views) {
        if (views->num_views < 1) return fail(GGR_E_INVALID, "GgrViews: num_views must be >= 1");
        const int sets = views->num_sets > 1 ? views->num_sets : 1;
        if (views->num_views % sets != 0) return fail(GGR_E_INVALID, "GgrViews: num_views must be a multiple of num_sets");
        if ((int64_t)views->num_views * st->num_points >= 0x7FFFFFFFll) return fail(GGR_E_LIMIT, "num_views x num_points too large");
        if ((int64_t)views->num_views * (int64_t)tiles_of(st->image_width, st->image_height) > (1 << 24))
            return fail(GGR_E_LIMIT, "more than 2^24 tiles over all views");
        V = views->num_views;
    }
    hipStream_t s = (hipStream_t)stream;
    const int P1 = st->num_points, W = st->image_width, H = st->image_height;
    const size_t rows = (size_t)V * (size_t)P1;
    if (rows == 0) return GGR_OK;
    if (cp->out_weight_sum) HIP_TRY(hipMemsetAsync(cp->out_weight_sum, 0, rows * sizeof(float), s));
    if (cp->out_weight_max) HIP_TRY(hipMemsetAsync(cp->out_weight_max, 0, rows * sizeof(float), s));
    if (cp->out_pixel_count) HIP_TRY(hipMemsetAsync(cp->out_pixel_count, 0, rows * sizeof(int32_t), s));
    if (cp->num_rendered == 0 || (size_t)W * H == 0) return GGR_OK;   // no list entry anywhere
    GeomLayout g = ggr_carve_geom((void*)cp->geom_buffer, rows, ggr_sort_segments((size_t)V), /*with_jac=*/false);
    ImageLayout im = ggr_carve_image((void*)cp->image_buffer, W, H, V);
    const bool scissored = (st->scissor[0] | st->scissor[1] | st->scissor[2] | st->scissor[3]) != 0;
    ggr::launch_blend_contrib(W, H, im.ranges, (const uint32_t*)cp->binning_buffer, g.splat, cp->out_weight_sum,
                              cp->out_weight_max, cp->out_pixel_count, V, scissored ? 1 : 0, s);
    KCHECK(st->debug != 0, s, "blend_contrib");
    return GGR_OK;
}

// ---- the pick pass (blend_pick.hip): per-pixel median-depth Gaussian, dominant Gaussian and contributor count -----------------
int ggr_pixel_picks(const GgrSettings* st, const GgrViews* views, const GgrPickPass* pp, void* stream) {
    g_err[0] = 0;
    if (!st || !pp) return fail(GGR_E_INVALID, "null settings / pick pass");
    if (pp->struct_size < (int32_t)sizeof(GgrPickPass))
        return fail(GGR_E_INVALID, "GgrPickPass.struct_size %d is smaller than the %d bytes of its fields", (int)pp->struct_size,
                    (int)sizeof(GgrPickPass));
    if (pp->reserved != 0) return fail(GGR_E_INVALID, "GgrPickPass.reserved must be 0, not %d", (int)pp->reserved);
    if (!pp->out_median_index && !pp->out_median_depth && !pp->out_max_index && !pp->out_max_weight && !pp->out_count)
        return fail(GGR_E_INVALID, "GgrPickPass: every output is NULL");
    if (st->num_points < 0 || st->image_width < 0 || st->image_height < 0) return fail(GGR_E_INVALID, "negative size");
    if (!pp->geom_buffer || !pp->image_buffer) return fail(GGR_E_INVALID, "GgrPickPass: null geom / image buffer of the forward");
    if (pp->num_rendered != 0 && !pp->binning_buffer) return fail(GGR_E_INVALID, "GgrPickPass.binning_buffer is NULL");
    int V = 1;
    if (views) {
        if (views->num_views < 1) return fail(GGR_E_INVALID, "GgrViews: num_views must be >= 1");
        const int sets = views->num_sets > 1 ? views->num_sets : 1;
        if (views->num_views % sets != 0) return fail(GGR_E_INVALID, "GgrViews: num_views must be a multiple of num_sets");
        if ((int64_t)views->num_views * st->num_points >= 0x7FFFFFFFll) return fail(GGR_E_LIMIT, "num_views x num_points too large");
        if ((int64_t)views->num_views * (int64_t)tiles_of(st->image_width, st->image_height) > (1 << 24))
            return fail(GGR_E_LIMIT, "more than 2^24 tiles over all views");
        V = views->num_views;
    }
    hipStream_t s = (hipStream_t)stream;
    const int P1 = st->num_points, W = st->image_width, H = st->image_height;
    const size_t pixels = (size_t)V * (size_t)W * (size_t)H;
    if (pixels == 0) return GGR_OK;
    if (P1 == 0 || pp->num_rendered == 0) {   // no list entry anywhere: every pixel gets the "none" values (−1 = all bits set)
        if (pp->out_median_index) HIP_TRY(hipMemsetAsync(pp->out_median_index, 0xFF, pixels * sizeof(int32_t), s));
        if (pp->out_median_depth) HIP_TRY(hipMemsetAsync(pp->out_median_depth, 0, pixels * sizeof(float), s));
        if (pp->out_max_index) HIP_TRY(hipMemsetAsync(pp->out_max_index, 0xFF, pixels * sizeof(int32_t), s));
        if (pp->out_max_weight) HIP_TRY(hipMemsetAsync(pp->out_max_weight, 0, pixels * sizeof(float), s));
        if (pp->out_count) HIP_TRY(hipMemsetAsync(pp->out_count, 0, pixels * sizeof(int32_t), s));
        return GGR_OK;
    }
    GeomLayout g = ggr_carve_geom((void*)pp->geom_buffer, (size_t)V * (size_t)P1, ggr_sort_segments((size_t)V), /*with_jac=*/false);
    ImageLayout im = ggr_carve_image((void*)pp->image_buffer, W, H, V);
    const bool scissored = (st->scissor[0] | st->scissor[1] | st->scissor[2] | st->scissor[3]) != 0;
    ggr::launch_blend_pick(W, H, im.ranges, (const uint32_t*)pp->binning_buffer, g.splat, pp->out_median_index,
                           pp->out_median_depth, pp->out_max_index, pp->out_max_weight, pp->out_count, V, P1, scissored ? 1 : 0, s);
    KCHECK(st->debug != 0, s, "blend_pick");
    return GGR_OK;
}

// ---- the hit pass (blend_hits.hip): per-pixel hit lists — the first K composited Gaussians, their weights, the rest, the count ---
int ggr_pixel_hits(const GgrSettings* st, const GgrViews* views, const GgrHitPass* hp, void* stream) {
    g_err[0] = 0;
    if (!st || !hp) return fail(GGR_E_INVALID, "null settings / hit pass");
    if (hp->struct_size < (int32_t)sizeof(GgrHitPass))
        return fail(GGR_E_INVALID, "GgrHitPass.struct_size %d is smaller than the %d bytes of its fields", (int)hp->struct_size,
                    (int)sizeof(GgrHitPass));
    if (hp->num_hits < 1 || hp->num_hits > GGR_MAX_HITS)
        return fail(GGR_E_INVALID, "GgrHitPass.num_hits must be 1..%d, not %d", GGR_MAX_HITS, (int)hp->num_hits);
    if ((hp->out_index == nullptr) != (hp->out_weight == nullptr))
        return fail(GGR_E_INVALID, "GgrHitPass: out_index and out_weight come as a pair (both, or neither)");
    if (!hp->out_index && !hp->out_rest && !hp->out_count) return fail(GGR_E_INVALID, "GgrHitPass: every output is NULL");
    if (st->num_points < 0 || st->image_width < 0 || st->image_height < 0) return fail(GGR_E_INVALID, "negative size");
    if (!hp->geom_buffer || !hp->image_buffer) return fail(GGR_E_INVALID, "GgrHitPass: null geom / image buffer of the forward");
    if (hp->num_rendered != 0 && !hp->binning_buffer) return fail(GGR_E_INVALID, "GgrHitPass.binning_buffer is NULL");
    int V = 1;
    if (views) {
        if (views->num_views < 1) return fail(GGR_E_INVALID, "GgrViews: num_views must be >= 1");
        const int sets = views->num_sets > 1 ? views->num_sets : 1;
        if (views->num_views % sets != 0) return fail(GGR_E_INVALID, "GgrViews: num_views must be a multiple of num_sets");
        if ((int64_t)views->num_views * st->num_points >= 0x7FFFFFFFll) return fail(GGR_E_LIMIT, "num_views x num_points too large");
        if ((int64_t)views->num_views * (int64_t)tiles_of(st->image_width, st->image_height) > (1 << 24))
            return fail(GGR_E_LIMIT, "more than 2^24 tiles over all views");
        V = views->num_views;
    }
    hipStream_t s = (hipStream_t)stream;
    const int P1 = st->num_points, W = st->image_width, H = st->image_height, K = hp->num_hits;
    const size_t pixels = (size_t)V * (size_t)W * (size_t)H;
    if (pixels == 0) return GGR_OK;
    if (P1 == 0 || hp->num_rendered == 0) {   // no list entry anywhere: every element gets its padding value (−1 = all bits set)
        if (hp->out_index) HIP_TRY(hipMemsetAsync(hp->out_index, 0xFF, pixels * K * sizeof(int32_t), s));
        if (hp->out_weight) HIP_TRY(hipMemsetAsync(hp->out_weight, 0, pixels * K * sizeof(float), s));
        if (hp->out_rest) HIP_TRY(hipMemsetAsync(hp->out_rest, 0, pixels * sizeof(float), s));
        if (hp->out_count) HIP_TRY(hipMemsetAsync(hp->out_count, 0, pixels * sizeof(int32_t), s));
        return GGR_OK;
    }
    GeomLayout g = ggr_carve_geom((void*)hp->geom_buffer, (size_t)V * (size_t)P1, ggr_sort_segments((size_t)V), /*with_jac=*/false);
    ImageLayout im = ggr_carve_image((void*)hp->image_buffer, W, H, V);
    const bool scissored = (st->scissor[0] | st->scissor[1] | st->scissor[2] | st->scissor[3]) != 0;
    ggr::launch_blend_hits(W, H, im.ranges, (const uint32_t*)hp->binning_buffer, g.splat, K, hp->out_index, hp->out_weight,
                           hp->out_rest, hp->out_count, V, P1, scissored ? 1 : 0, s);
    KCHECK(st->debug != 0, s, "blend_hits");
    return GGR_OK;
}

// ---- the hit pass's backward (blend_hits_grad.hip): a loss over the hit weights and the rest, into the backward scratch ---------
int ggr_pixel_hits_backward(const GgrSettings* st, const GgrViews* views, const GgrHitGradPass* hp, void* stream) {
    g_err[0] = 0;
    if (!st || !hp) return fail(GGR_E_INVALID, "null settings / hit gradient pass");
    if (hp->struct_size < (int32_t)sizeof(GgrHitGradPass))
        return fail(GGR_E_INVALID, "GgrHitGradPass.struct_size %d is smaller than the %d bytes of its fields", (int)hp->struct_size,
                    (int)sizeof(GgrHitGradPass));
    if (hp->reserved != 0) return fail(GGR_E_INVALID, "GgrHitGradPass.reserved must be 0, not %d", (int)hp->reserved);
    if (hp->num_hits < 1 || hp->num_hits > GGR_MAX_HITS)
        return fail(GGR_E_INVALID, "GgrHitGradPass.num_hits must be 1..%d, not %d", GGR_MAX_HITS, (int)hp->num_hits);
    if (st->num_points < 0 || st->image_width < 0 || st->image_height < 0) return fail(GGR_E_INVALID, "negative size");
    if (!hp->dL_dweight && !hp->dL_drest) return fail(GGR_E_INVALID, "GgrHitGradPass: dL_dweight and dL_drest are both NULL");
    if (!hp->geom_buffer || !hp->image_buffer) return fail(GGR_E_INVALID, "GgrHitGradPass: null geom / image buffer of the forward");
    if (hp->num_rendered != 0 && !hp->binning_buffer) return fail(GGR_E_INVALID, "GgrHitGradPass.binning_buffer is NULL");
    if (!hp->weight) return fail(GGR_E_INVALID, "GgrHitGradPass.weight is NULL");
    if (!hp->count) return fail(GGR_E_INVALID, "GgrHitGradPass.count is NULL");
    if (!hp->scratch) return fail(GGR_E_INVALID, "GgrHitGradPass.scratch is NULL");
    int V = 1;
    if (views) {
        if (views->num_views < 1) return fail(GGR_E_INVALID, "GgrViews: num_views must be >= 1");
        const int sets = views->num_sets > 1 ? views->num_sets : 1;
        if (views->num_views % sets != 0) return fail(GGR_E_INVALID, "GgrViews: num_views must be a multiple of num_sets");
        if ((int64_t)views->num_views * st->num_points >= 0x7FFFFFFFll) return fail(GGR_E_LIMIT, "num_views x num_points too large");
        if ((int64_t)views->num_views * (int64_t)tiles_of(st->image_width, st->image_height) > (1 << 24))
            return fail(GGR_E_LIMIT, "more than 2^24 tiles over all views");
        V = views->num_views;
    }
    hipStream_t s = (hipStream_t)stream;
    const int P1 = st->num_points, W = st->image_width, H = st->image_height;
    BwdScratch sc = ggr_carve_bwd(hp->scratch, (size_t)P1, (size_t)V);
    if (!hp->scratch_zeroed) HIP_TRY(hipMemsetAsync(hp->scratch, 0, sc.bytes, s));
    if (P1 == 0 || hp->num_rendered == 0 || (size_t)W * H == 0) return GGR_OK;
    GeomLayout g = ggr_carve_geom((void*)hp->geom_buffer, (size_t)P1 * V, ggr_sort_segments((size_t)V), /*with_jac=*/false);
    ImageLayout im = ggr_carve_image((void*)hp->image_buffer, W, H, V);
    ggr::launch_blend_hits_bwd(W, H, im.ranges, (const uint32_t*)hp->binning_buffer, g.splat, im.final_T, hp->num_hits, hp->weight,
                               hp->count, hp->dL_dweight, hp->dL_drest, sc.grad2d, V, s);
    KCHECK(st->debug != 0, s, "blend_hits_bwd");
    return GGR_OK;
}

// ---- the projection pass (projection.hip): the per-(view, Gaussian) projection outputs, and the seeding of their gradients -------
namespace {
int projection_pass_check(const GgrSettings* st, const GgrViews* views, const GgrProjectionPass* pp, bool backward, int* V) {
    if (!st || !pp) return fail(GGR_E_INVALID, "null settings / projection pass");
    if (pp->struct_size < (int32_t)sizeof(GgrProjectionPass))
        return fail(GGR_E_INVALID, "GgrProjectionPass.struct_size %d is smaller than the %d bytes of its fields", (int)pp->struct_size,
                    (int)sizeof(GgrProjectionPass));
    if (pp->reserved != 0 || pp->reserved2 != 0)
        return fail(GGR_E_INVALID, "GgrProjectionPass.reserved must be 0, not %d / %d", (int)pp->reserved, (int)pp->reserved2);
    if (st->num_points < 0 || st->image_width < 0 || st->image_height < 0) return fail(GGR_E_INVALID, "negative size");
    if (backward) {
        if (st->num_points > 0 && !pp->dL_dmeans2d && !pp->dL_ddepth && !pp->dL_dconic && !pp->dL_dopacity && !pp->dL_dcolor)
            return fail(GGR_E_INVALID, "GgrProjectionPass: all five gradients are NULL");
        if (!pp->scratch) return fail(GGR_E_INVALID, "GgrProjectionPass.scratch is NULL");
    } else {
        if (st->num_points > 0 && !pp->out_means2d && !pp->out_depth && !pp->out_conic && !pp->out_opacity && !pp->out_color && !pp->out_valid)
            return fail(GGR_E_INVALID, "GgrProjectionPass: all six outputs are NULL");
        if (!pp->geom_buffer) return fail(GGR_E_INVALID, "GgrProjectionPass: null geom buffer of the forward");
    }
    if (st->num_points > 0 && !pp->radii) return fail(GGR_E_INVALID, "GgrProjectionPass.radii is NULL");
    *V = 1;
    if (views) {
        if (views->num_views < 1) return fail(GGR_E_INVALID, "GgrViews: num_views must be >= 1");
        const int sets = views->num_sets > 1 ? views->num_sets : 1;
        if (views->num_views % sets != 0) return fail(GGR_E_INVALID, "GgrViews: num_views must be a multiple of num_sets");
        if ((int64_t)views->num_views * st->num_points >= 0x7FFFFFFFll) return fail(GGR_E_LIMIT, "num_views x num_points too large");
        *V = views->num_views;
    }
    return GGR_OK;
}
}  // namespace

int ggr_projection(const GgrSettings* st, const GgrViews* views, const GgrProjectionPass* pp, void* stream) {
    g_err[0] = 0;
    int V = 1;
    const int rc = projection_pass_check(st, views, pp, false, &V);
    if (rc) return rc;
    const size_t pairs = (size_t)st->num_points * (size_t)V;
    if (pairs == 0) return GGR_OK;
    hipStream_t s = (hipStream_t)stream;
    GeomLayout g = ggr_carve_geom((void*)pp->geom_buffer, pairs, ggr_sort_segments((size_t)V), /*with_jac=*/false);
    ggr::launch_projection_unpack(pairs, g.splat, g.colour, pp->radii, pp->out_means2d, pp->out_depth, pp->out_conic,
                                  pp->out_opacity, pp->out_color, pp->out_valid, s);
    KCHECK(st->debug != 0, s, "projection_unpack");
    return GGR_OK;
}

int ggr_projection_backward(const GgrSettings* st, const GgrViews* views, const GgrProjectionPass* pp, void* stream) {
    g_err[0] = 0;
    int V = 1;
    const int rc = projection_pass_check(st, views, pp, true, &V);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int P1 = st->num_points;
    BwdScratch sc = ggr_carve_bwd(pp->scratch, (size_t)P1, (size_t)V);
    if (P1 == 0) {
        if (!pp->scratch_zeroed) HIP_TRY(hipMemsetAsync(pp->scratch, 0, sc.bytes, s));
        return GGR_OK;
    }
    // not yet clear: the seeding writes every record whole (its clearing), what lies behind the records — the camera
    // gradients' partial rows — is cleared here
    if (!pp->scratch_zeroed)
        HIP_TRY(hipMemsetAsync(sc.pose_acc, 0, sc.bytes - (size_t)((char*)sc.pose_acc - (char*)pp->scratch), s));
    ggr::launch_projection_seed((size_t)P1 * (size_t)V, st->image_width, st->image_height, pp->radii, pp->dL_dmeans2d, pp->dL_ddepth,
                                pp->dL_dconic, pp->dL_dopacity, pp->dL_dcolor, sc.grad2d, pp->scratch_zeroed ? 1 : 0, s);
    KCHECK(st->debug != 0, s, "projection_seed");
    return GGR_OK;
}

// ---- the Gaussian adapter pass (adapter.hip): GGRt's encoder tail, one forward and one backward launch ----------------------------
namespace {
int adapter_pass_check(const GgrAdapterPass* ap, bool backward, ggr::AdapterArgs* a) {
    if (!ap) return fail(GGR_E_INVALID, "null GgrAdapterPass");
    if (ap->struct_size < (int32_t)sizeof(GgrAdapterPass))
        return fail(GGR_E_INVALID, "GgrAdapterPass.struct_size %d is smaller than the %d bytes of its fields", (int)ap->struct_size,
                    (int)sizeof(GgrAdapterPass));
    if (ap->reserved != 0 || ap->reserved2 != 0)
        return fail(GGR_E_INVALID, "GgrAdapterPass.reserved must be 0, not %d / %d", (int)ap->reserved, (int)ap->reserved2);
    if (ap->num_cameras < 0 || ap->gaussians_per_camera < 0) return fail(GGR_E_INVALID, "GgrAdapterPass: negative size");
    const int d = ap->d_sh;
    if (d != 1 && d != 4 && d != 9 && d != 16 && d != 25) return fail(GGR_E_INVALID, "GgrAdapterPass.d_sh must be 1, 4, 9, 16 or 25, not %d", d);
    if (ap->samples_per_row < 1 || ap->gaussians_per_camera % ap->samples_per_row != 0)
        return fail(GGR_E_INVALID, "GgrAdapterPass: gaussians_per_camera %d is no multiple of samples_per_row %d",
                    (int)ap->gaussians_per_camera, (int)ap->samples_per_row);
    if (ap->num_cameras > 65535) return fail(GGR_E_LIMIT, "GgrAdapterPass: more than 65535 cameras");
    if ((int64_t)ap->num_cameras * ap->gaussians_per_camera >= 0x7FFFFFFFll) return fail(GGR_E_LIMIT, "GgrAdapterPass: num_cameras x gaussians_per_camera too large");
    const bool any = ap->num_cameras > 0 && ap->gaussians_per_camera > 0;
    const void* need_fwd[] = {ap->depth, ap->coords, ap->raw, ap->c2w, ap->Kinv, ap->q_cam, ap->scale_mult, ap->sh_transform, ap->sh_mask};
    const char* name_fwd[] = {"depth", "coords", "raw", "c2w", "Kinv", "q_cam", "scale_mult", "sh_transform", "sh_mask"};
    for (int i = 0; i < 9; ++i)
        if (any && !need_fwd[i]) return fail(GGR_E_INVALID, "GgrAdapterPass.%s is NULL", name_fwd[i]);
    const void* need_out[] = {ap->out_means, ap->out_scales, ap->out_quats, ap->out_harmonics};
    const char* name_out[] = {"out_means", "out_scales", "out_quats", "out_harmonics"};
    const void* need_bwd[] = {ap->dL_dmeans, ap->dL_dscales, ap->dL_dquats, ap->dL_dharmonics, ap->dL_draw};
    const char* name_bwd[] = {"dL_dmeans", "dL_dscales", "dL_dquats", "dL_dharmonics", "dL_draw"};
    if (any && !backward)
        for (int i = 0; i < 4; ++i)
            if (!need_out[i]) return fail(GGR_E_INVALID, "GgrAdapterPass.%s is NULL", name_out[i]);
    if (any && backward)
        for (int i = 0; i < 5; ++i)
            if (!need_bwd[i]) return fail(GGR_E_INVALID, "GgrAdapterPass.%s is NULL", name_bwd[i]);
    const void* all[] = {ap->depth, ap->coords, ap->raw, ap->c2w, ap->Kinv, ap->q_cam, ap->scale_mult, ap->sh_transform, ap->sh_mask,
                         ap->out_means, ap->out_scales, ap->out_quats, ap->out_harmonics, ap->dL_dmeans, ap->dL_dscales, ap->dL_dquats,
                         ap->dL_dharmonics, ap->dL_draw, ap->dL_ddepth, ap->dL_dcoords, ap->dL_dc2w, ap->dL_dKinv, ap->dL_dq_cam,
                         ap->dL_dscale_mult, ap->dL_dsh_transform};
    for (const void* p : all)
        if (((uintptr_t)p & 3u) != 0) return fail(GGR_E_INVALID, "GgrAdapterPass: a buffer is misaligned (every array needs a float's 4 bytes)");
    a->C = ap->num_cameras; a->G = ap->gaussians_per_camera; a->spp = ap->samples_per_row; a->d_sh = d;
    a->scale_min = ap->scale_min; a->scale_max = ap->scale_max; a->eps = ap->eps;
    a->depth = ap->depth; a->coords = ap->coords; a->raw = ap->raw; a->c2w = ap->c2w; a->Kinv = ap->Kinv; a->q_cam = ap->q_cam;
    a->scale_mult = ap->scale_mult; a->sh_transform = ap->sh_transform; a->sh_mask = ap->sh_mask;
    a->means = ap->out_means; a->scales = ap->out_scales; a->quats = ap->out_quats; a->harmonics = ap->out_harmonics;
    a->g_means = ap->dL_dmeans; a->g_scales = ap->dL_dscales; a->g_quats = ap->dL_dquats; a->g_harmonics = ap->dL_dharmonics;
    a->g_raw = ap->dL_draw; a->g_depth = ap->dL_ddepth; a->g_coords = ap->dL_dcoords; a->g_c2w = ap->dL_dc2w; a->g_Kinv = ap->dL_dKinv;
    a->g_q_cam = ap->dL_dq_cam; a->g_scale_mult = ap->dL_dscale_mult; a->g_sh_transform = ap->dL_dsh_transform;
    return GGR_OK;
}
}  // namespace

int ggr_adapter_forward(const GgrAdapterPass* ap, void* stream) {
    g_err[0] = 0;
    ggr::AdapterArgs a;
    const int rc = adapter_pass_check(ap, false, &a);
    if (rc) return rc;
    if (a.C == 0 || a.G == 0) return GGR_OK;
    hipStream_t s = (hipStream_t)stream;
    ggr::launch_adapter_forward(a, s);
    KCHECK(ap->debug != 0, s, "adapter_forward");
    return GGR_OK;
}

int ggr_adapter_backward(const GgrAdapterPass* ap, void* stream) {
    g_err[0] = 0;
    ggr::AdapterArgs a;
    const int rc = adapter_pass_check(ap, true, &a);
    if (rc) return rc;
    if (a.C == 0 || a.G == 0) return GGR_OK;
    hipStream_t s = (hipStream_t)stream;
    ggr::launch_adapter_backward(a, s);
    KCHECK(ap->debug != 0, s, "adapter_backward");
    return GGR_OK;
}

// ---- the depth-head pass (depth_head.hip): GGRt's depth sampling, depth and opacity, one forward and one backward launch ----------
namespace {
int depth_head_pass_check(const GgrDepthHeadPass* dp, bool backward, ggr::DepthHeadArgs* a) {
    if (!dp) return fail(GGR_E_INVALID, "null GgrDepthHeadPass");
    if (dp->struct_size < (int32_t)sizeof(GgrDepthHeadPass))
        return fail(GGR_E_INVALID, "GgrDepthHeadPass.struct_size %d is smaller than the %d bytes of its fields", (int)dp->struct_size,
                    (int)sizeof(GgrDepthHeadPass));
    if (dp->reserved != 0 || dp->reserved2 != 0)
        return fail(GGR_E_INVALID, "GgrDepthHeadPass.reserved must be 0, not %d / %d", (int)dp->reserved, (int)dp->reserved2);
    if (dp->num_cameras < 0 || dp->rays_per_camera < 0)
        return fail(GGR_E_INVALID, "GgrDepthHeadPass: negative size (num_cameras %d, rays_per_camera %d)", (int)dp->num_cameras, (int)dp->rays_per_camera);
    const int s = dp->num_buckets, srf = dp->num_surfaces, spp = dp->samples_per_ray;
    if (s < 1) return fail(GGR_E_INVALID, "GgrDepthHeadPass.num_buckets must be at least 1, not %d", s);
    if (s > ggr::kDepthHeadMaxBuckets) return fail(GGR_E_LIMIT, "GgrDepthHeadPass.num_buckets %d is above %d", s, ggr::kDepthHeadMaxBuckets);
    if (spp < 1) return fail(GGR_E_INVALID, "GgrDepthHeadPass.samples_per_ray must be at least 1, not %d", spp);
    if (spp > ggr::kDepthHeadMaxSamples) return fail(GGR_E_LIMIT, "GgrDepthHeadPass.samples_per_ray %d is above %d", spp, ggr::kDepthHeadMaxSamples);
    if (dp->deterministic && spp > s)
        return fail(GGR_E_INVALID, "GgrDepthHeadPass.samples_per_ray %d is above num_buckets %d in deterministic mode", spp, s);
    if (srf < 1) return fail(GGR_E_INVALID, "GgrDepthHeadPass.num_surfaces must be at least 1, not %d", srf);
    if (dp->xy_raw_stride < 2) return fail(GGR_E_INVALID, "GgrDepthHeadPass.xy_raw_stride must be at least 2, not %d", (int)dp->xy_raw_stride);
    if ((int64_t)2 * s * srf >= 0x7FFFFFFFll) return fail(GGR_E_LIMIT, "GgrDepthHeadPass.num_surfaces %d: a logits row is too long", srf);
    if (dp->num_cameras > 65535) return fail(GGR_E_LIMIT, "GgrDepthHeadPass.num_cameras: more than 65535 cameras");
    // C·R·srf·spp < 2^31, factor by factor (no product may overflow on the way)
    int64_t total = dp->num_cameras;
    for (int64_t f : {(int64_t)dp->rays_per_camera, (int64_t)srf, (int64_t)spp}) {
        total *= f;
        if (total >= 0x7FFFFFFFll)
            return fail(GGR_E_LIMIT, "GgrDepthHeadPass: num_cameras x rays_per_camera x num_surfaces x samples_per_ray too large");
    }
    const bool any = dp->num_cameras > 0 && dp->rays_per_camera > 0;
    const void* need_in[] = {dp->logits, dp->xy_raw, dp->ray_xy, dp->near, dp->far};
    const char* name_in[] = {"logits", "xy_raw", "ray_xy", "near", "far"};
    for (int i = 0; i < 5; ++i)
        if (any && !need_in[i]) return fail(GGR_E_INVALID, "GgrDepthHeadPass.%s is NULL", name_in[i]);
    if (any && !backward) {
        if (!dp->deterministic && !dp->u) return fail(GGR_E_INVALID, "GgrDepthHeadPass.u is NULL in sampled mode");
        const void* need[] = {dp->out_depth, dp->out_opacity, dp->out_coords, dp->index};
        const char* name[] = {"out_depth", "out_opacity", "out_coords", "index"};
        for (int i = 0; i < 4; ++i)
            if (!need[i]) return fail(GGR_E_INVALID, "GgrDepthHeadPass.%s is NULL", name[i]);
    }
    if (any && backward) {
        if (!dp->index) return fail(GGR_E_INVALID, "GgrDepthHeadPass.index is NULL");
        if (!dp->dL_dlogits) return fail(GGR_E_INVALID, "GgrDepthHeadPass.dL_dlogits is NULL");
    }
    const void* all[] = {dp->logits, dp->xy_raw, dp->ray_xy, dp->near, dp->far, dp->u, dp->out_depth, dp->out_opacity, dp->out_coords,
                         dp->index, dp->dL_ddepth, dp->dL_dopacity, dp->dL_dcoords, dp->dL_dlogits, dp->dL_dxy_raw};
    for (const void* p : all)
        if (((uintptr_t)p & 3u) != 0) return fail(GGR_E_INVALID, "GgrDepthHeadPass: a buffer is misaligned (every array needs 4-byte alignment)");
    a->C = dp->num_cameras; a->R = dp->rays_per_camera; a->s = s; a->srf = srf; a->spp = spp;
    a->deterministic = dp->deterministic != 0; a->transmittance = dp->use_transmittance != 0; a->xy_stride = dp->xy_raw_stride;
    a->exponent = dp->opacity_exponent; a->opacity_scale = dp->opacity_scale; a->inv_w = dp->inv_w; a->inv_h = dp->inv_h;
    a->logits = dp->logits; a->xy_raw = dp->xy_raw; a->ray_xy = dp->ray_xy; a->near = dp->near; a->far = dp->far; a->u = dp->u;
    a->depth = dp->out_depth; a->opacity = dp->out_opacity; a->coords = dp->out_coords; a->index = dp->index;
    a->g_depth = dp->dL_ddepth; a->g_opacity = dp->dL_dopacity; a->g_coords = dp->dL_dcoords; a->g_logits = dp->dL_dlogits;
    a->g_xy = dp->dL_dxy_raw;
    return GGR_OK;
}
}  // namespace

int ggr_depth_head_forward(const GgrDepthHeadPass* dp, void* stream) {
    g_err[0] = 0;
    ggr::DepthHeadArgs a;
    const int rc = depth_head_pass_check(dp, false, &a);
    if (rc) return rc;
    if (a.C == 0 || a.R == 0) return GGR_OK;
    hipStream_t s = (hipStream_t)stream;
    ggr::launch_depth_head_forward(a, s);
    KCHECK(dp->debug != 0, s, "depth_head_forward");
    return GGR_OK;
}

int ggr_depth_head_backward(const GgrDepthHeadPass* dp, void* stream) {
    g_err[0] = 0;
    ggr::DepthHeadArgs a;
    const int rc = depth_head_pass_check(dp, true, &a);
    if (rc) return rc;
    if (a.C == 0 || a.R == 0) return GGR_OK;
    hipStream_t s = (hipStream_t)stream;
    ggr::launch_depth_head_backward(a, s);
    KCHECK(dp->debug != 0, s, "depth_head_backward");
    return GGR_OK;
}

// ---- the epipolar-sampler pass (epipolar.hip): GGRt's EpipolarSampler.forward and the depth lines behind it ---------------------
namespace {
int64_t epipolar_scratch_bytes(int64_t b, int64_t v, int64_t c, int64_t h, int64_t w) {
    if (b < 0 || v < ggr::kEpipolarMinViews || v > ggr::kEpipolarMaxViews || c < 1 || c > ggr::kEpipolarMaxChannels || h < 1 || w < 1) return -1;
    if (b * v > 65535) return -1;
    const int64_t pixels = b * v * h;            // < 2^16 · 2^31
    if (pixels >= 0x7FFFFFFFll || pixels * w >= 0x7FFFFFFFll) return -1;
    return pixels * w * c * (int64_t)sizeof(float);
}

int epipolar_pass_check(const GgrEpipolarPass* ep, bool backward, ggr::EpipolarArgs* a) {
    if (!ep) return fail(GGR_E_INVALID, "null GgrEpipolarPass");
    if (ep->struct_size < (int32_t)sizeof(GgrEpipolarPass))
        return fail(GGR_E_INVALID, "GgrEpipolarPass.struct_size %d is smaller than the %d bytes of its fields", (int)ep->struct_size,
                    (int)sizeof(GgrEpipolarPass));
    if (ep->reserved != 0) return fail(GGR_E_INVALID, "GgrEpipolarPass.reserved must be 0, not %d", (int)ep->reserved);
    const int b = ep->batch, v = ep->num_views, c = ep->channels, h = ep->height, w = ep->width, s = ep->num_samples;
    if (b < 0) return fail(GGR_E_INVALID, "GgrEpipolarPass.batch is negative (%d)", b);
    if (s < 1 || s > ggr::kEpipolarMaxSamples) return fail(GGR_E_INVALID, "GgrEpipolarPass.num_samples %d is outside 1..%d", s, ggr::kEpipolarMaxSamples);
    if (c < 1 || c > ggr::kEpipolarMaxChannels) return fail(GGR_E_INVALID, "GgrEpipolarPass.channels %d is outside 1..%d", c, ggr::kEpipolarMaxChannels);
    if (v < ggr::kEpipolarMinViews || v > ggr::kEpipolarMaxViews)
        return fail(GGR_E_INVALID, "GgrEpipolarPass.num_views %d is outside %d..%d", v, ggr::kEpipolarMinViews, ggr::kEpipolarMaxViews);
    if (h < 1 || w < 1) return fail(GGR_E_INVALID, "GgrEpipolarPass.height / width must be at least 1, not %d x %d", h, w);
    int y0 = 0, y1 = h, x0 = 0, x1 = w;
    if (ep->use_window) {
        y0 = ep->window_y0; y1 = ep->window_y1; x0 = ep->window_x0; x1 = ep->window_x1;
        if (y0 < 0 || y0 >= y1 || y1 > h || x0 < 0 || x0 >= x1 || x1 > w)
            return fail(GGR_E_INVALID, "GgrEpipolarPass: the window rows %d..%d, columns %d..%d is empty or leaves the %d x %d grid", y0, y1, x0, x1, h, w);
    }
    const int64_t need = epipolar_scratch_bytes(b, v, c, h, w);
    if (need < 0) return fail(GGR_E_INVALID, "GgrEpipolarPass: too large (batch x num_views above 65535, or 2^31 map pixels or more)");
    int64_t total = (int64_t)b * v * (v - 1);      // < 2^16 · 8
    for (int64_t f : {(int64_t)(y1 - y0), (int64_t)(x1 - x0), (int64_t)s}) {
        total *= f;
        if (total >= 0x7FFFFFFFll) return fail(GGR_E_INVALID, "GgrEpipolarPass: too large (2^31 or more of pair-rays x samples)");
    }
    const bool any = b > 0;
    if (any && !backward) {
        const void* need_in[] = {ep->c2w, ep->w2c, ep->K, ep->Kinv, ep->near, ep->far};
        const char* name_in[] = {"c2w", "w2c", "K", "Kinv", "near", "far"};
        for (int i = 0; i < 6; ++i)
            if (!need_in[i]) return fail(GGR_E_INVALID, "GgrEpipolarPass.%s is NULL", name_in[i]);
        if (ep->features && !ep->images) return fail(GGR_E_INVALID, "GgrEpipolarPass.images is NULL");
        if (ep->features && !ep->scratch) return fail(GGR_E_INVALID, "GgrEpipolarPass.scratch is NULL");
    }
    if (any && backward) {
        const void* need_in[] = {ep->valid, ep->segment, ep->dL_dfeatures, ep->dL_dimages, ep->scratch};
        const char* name_in[] = {"valid", "segment", "dL_dfeatures", "dL_dimages", "scratch"};
        for (int i = 0; i < 5; ++i)
            if (!need_in[i]) return fail(GGR_E_INVALID, "GgrEpipolarPass.%s is NULL", name_in[i]);
    }
    if (any && (backward || ep->features) && ep->scratch_bytes < need)
        return fail(GGR_E_INVALID, "GgrEpipolarPass.scratch_bytes %lld is below the %lld bytes needed", (long long)ep->scratch_bytes, (long long)need);
    const void* all[] = {ep->c2w, ep->w2c, ep->K, ep->Kinv, ep->near, ep->far, ep->images, ep->features, ep->xy_ray, ep->xy_sample,
                         ep->xy_sample_near, ep->xy_sample_far, ep->origins, ep->directions, ep->depth, ep->segment, ep->dL_dfeatures,
                         ep->dL_dimages, ep->scratch};
    for (const void* p : all)
        if (((uintptr_t)p & 3u) != 0) return fail(GGR_E_INVALID, "GgrEpipolarPass: a buffer is misaligned (every float array needs 4-byte alignment)");
    a->b = b; a->v = v; a->c = c; a->h = h; a->w = w; a->s = s;
    a->y0 = y0; a->y1 = y1; a->x0 = x0; a->x1 = x1;
    a->img_sb = ep->image_strides[0]; a->img_sv = ep->image_strides[1]; a->img_sc = ep->image_strides[2];
    a->img_sh = ep->image_strides[3]; a->img_sw = ep->image_strides[4];
    a->c2w = ep->c2w; a->w2c = ep->w2c; a->K = ep->K; a->Kinv = ep->Kinv; a->near = ep->near; a->far = ep->far; a->images = ep->images;
    a->features = ep->features; a->valid = ep->valid; a->xy_ray = ep->xy_ray; a->xy_sample = ep->xy_sample;
    a->xy_near = ep->xy_sample_near; a->xy_far = ep->xy_sample_far; a->origins = ep->origins; a->directions = ep->directions;
    a->depth = ep->depth; a->seg = ep->segment; a->g_features = ep->dL_dfeatures; a->g_images = ep->dL_dimages; a->scratch = ep->scratch;
    return GGR_OK;
}
}  // namespace

int64_t ggr_epipolar_scratch_bytes(int32_t batch, int32_t num_views, int32_t channels, int32_t height, int32_t width) {
    return epipolar_scratch_bytes(batch, num_views, channels, height, width);
}

int ggr_epipolar_forward(const GgrEpipolarPass* ep, void* stream) {
    g_err[0] = 0;
    ggr::EpipolarArgs a;
    const int rc = epipolar_pass_check(ep, false, &a);
    if (rc) return rc;
    if (a.b == 0) return GGR_OK;
    hipStream_t s = (hipStream_t)stream;
    ggr::launch_epipolar_forward(a, s);
    KCHECK(ep->debug != 0, s, "epipolar_forward");
    return GGR_OK;
}

int ggr_epipolar_backward(const GgrEpipolarPass* ep, void* stream) {
    g_err[0] = 0;
    ggr::EpipolarArgs a;
    const int rc = epipolar_pass_check(ep, true, &a);
    if (rc) return rc;
    if (a.b == 0) return GGR_OK;
    hipStream_t s = (hipStream_t)stream;
    ggr::launch_epipolar_backward(a, s);
    KCHECK(ep->debug != 0, s, "epipolar_backward");
    return GGR_OK;
}

// ---- the epipolar cross-attention core (epipolar_attn.hip): one query token per ray against the ray's raw samples -------------
namespace {
int epipolar_attn_pass_check(const GgrEpipolarAttnPass* ap, bool backward, ggr::EpiAttnArgs* a) {
    if (!ap) return fail(GGR_E_INVALID, "null GgrEpipolarAttnPass");
    if (ap->struct_size < (int32_t)sizeof(GgrEpipolarAttnPass))
        return fail(GGR_E_INVALID, "GgrEpipolarAttnPass.struct_size %d is smaller than the %d bytes of its fields", (int)ap->struct_size,
                    (int)sizeof(GgrEpipolarAttnPass));
    if (ap->reserved != 0) return fail(GGR_E_INVALID, "GgrEpipolarAttnPass.reserved must be 0, not %d", (int)ap->reserved);
    const int N = ap->N, S = ap->S, C = ap->C, H = ap->H;
    if (N < 0 || N > ggr::kEpiAttnMaxRays) return fail(GGR_E_INVALID, "GgrEpipolarAttnPass.N %d is outside 0..%d", N, ggr::kEpiAttnMaxRays);
    if (S < 1 || S > ggr::kEpiAttnMaxSamples) return fail(GGR_E_INVALID, "GgrEpipolarAttnPass.S %d is outside 1..%d", S, ggr::kEpiAttnMaxSamples);
    if (C < 1 || C > ggr::kEpiAttnMaxChannels) return fail(GGR_E_INVALID, "GgrEpipolarAttnPass.C %d is outside 1..%d", C, ggr::kEpiAttnMaxChannels);
    if (H < 1 || H > ggr::kEpiAttnMaxHeads) return fail(GGR_E_INVALID, "GgrEpipolarAttnPass.H %d is outside 1..%d", H, ggr::kEpiAttnMaxHeads);
    const int lds = ggr::epipolar_attn_lds_bytes(S, C);
    if (lds > ggr::kEpiAttnLdsLimit)      // (cannot happen inside the limits above: 64 rows of 260 floats are 66 560 bytes)
        return fail(GGR_E_INVALID, "GgrEpipolarAttnPass: S = %d, C = %d needs %d bytes of LDS, above the %d bytes of a workgroup", S, C, lds,
                    ggr::kEpiAttnLdsLimit);
    if (N > 0) {
        const void* fwd_in[] = {ap->qk, ap->z, ap->out_ctx, ap->out_attn};
        const char* fwd_name[] = {"qk", "z", "out_ctx", "out_attn"};
        const void* bwd_in[] = {ap->qk, ap->z, ap->attn, ap->dL_dctx, ap->dL_dqk, ap->dL_dz};
        const char* bwd_name[] = {"qk", "z", "attn", "dL_dctx", "dL_dqk", "dL_dz"};
        for (int i = 0; i < (backward ? 6 : 4); ++i)
            if (!(backward ? bwd_in : fwd_in)[i])
                return fail(GGR_E_INVALID, "GgrEpipolarAttnPass.%s is NULL", (backward ? bwd_name : fwd_name)[i]);
    }
    const void* all[] = {ap->qk, ap->z, ap->out_ctx, ap->out_attn, ap->attn, ap->dL_dctx, ap->dL_dqk, ap->dL_dz};
    for (const void* p : all)
        if (((uintptr_t)p & 3u) != 0) return fail(GGR_E_INVALID, "GgrEpipolarAttnPass: a buffer is misaligned (every float array needs 4-byte alignment)");
    a->N = N; a->S = S; a->C = C; a->H = H;
    a->qk = ap->qk; a->z = ap->z; a->ctx = ap->out_ctx; a->attn_out = ap->out_attn; a->attn = ap->attn; a->g_ctx = ap->dL_dctx;
    a->g_qk = ap->dL_dqk; a->g_z = ap->dL_dz;
    return GGR_OK;
}

int epipolar_attn_launched(hipError_t e, const ggr::EpiAttnArgs& a, const char* what) {
    if (e != hipSuccess)
        return fail(GGR_E_INVALID, "GgrEpipolarAttnPass: S = %d, C = %d needs %d bytes of LDS in one workgroup, which this device refused (%s)", a.S, a.C,
                    ggr::epipolar_attn_lds_bytes(a.S, a.C), hipGetErrorString(e));
    e = hipGetLastError();
    if (e != hipSuccess) return fail(GGR_E_HIP, "%s: %s", what, hipGetErrorString(e));
    return GGR_OK;
}
}  // namespace

int ggr_epipolar_attention_forward(const GgrEpipolarAttnPass* ap, void* stream) {
    g_err[0] = 0;
    ggr::EpiAttnArgs a;
    const int rc = epipolar_attn_pass_check(ap, false, &a);
    if (rc) return rc;
    if (a.N == 0) return GGR_OK;
    return epipolar_attn_launched(ggr::launch_epipolar_attn_forward(a, (hipStream_t)stream), a, "epipolar_attention_forward");
}

int ggr_epipolar_attention_backward(const GgrEpipolarAttnPass* ap, void* stream) {
    g_err[0] = 0;
    ggr::EpiAttnArgs a;
    const int rc = epipolar_attn_pass_check(ap, true, &a);
    if (rc) return rc;
    if (a.N == 0) return GGR_OK;
    return epipolar_attn_launched(ggr::launch_epipolar_attn_backward(a, (hipStream_t)stream), a, "epipolar_attention_backward");
}

// ---- the same core with the depth encoding folded in (epipolar_attn_enc.hip): the sampler's raw features and depth, no z ------
namespace {
int epipolar_attn_enc_pass_check(const GgrEpipolarAttnEncPass* ap, bool backward, ggr::EpiAttnEncArgs* a) {
    if (!ap) return fail(GGR_E_INVALID, "null GgrEpipolarAttnEncPass");
    if (ap->struct_size < (int32_t)sizeof(GgrEpipolarAttnEncPass))
        return fail(GGR_E_INVALID, "GgrEpipolarAttnEncPass.struct_size %d is smaller than the %d bytes of its fields", (int)ap->struct_size,
                    (int)sizeof(GgrEpipolarAttnEncPass));
    if (ap->reserved != 0 || ap->reserved2 != 0)
        return fail(GGR_E_INVALID, "GgrEpipolarAttnEncPass.reserved must be 0, not %d / %d", (int)ap->reserved, (int)ap->reserved2);
    const int N = ap->N, S = ap->S, C = ap->C, H = ap->H, O = ap->num_octaves;
    if (N < 0 || N > ggr::kEpiAttnMaxRays) return fail(GGR_E_INVALID, "GgrEpipolarAttnEncPass.N %d is outside 0..%d", N, ggr::kEpiAttnMaxRays);
    if (S < 1 || S > ggr::kEpiAttnMaxSamples) return fail(GGR_E_INVALID, "GgrEpipolarAttnEncPass.S %d is outside 1..%d", S, ggr::kEpiAttnMaxSamples);
    if (C < 1 || C > ggr::kEpiAttnMaxChannels) return fail(GGR_E_INVALID, "GgrEpipolarAttnEncPass.C %d is outside 1..%d", C, ggr::kEpiAttnMaxChannels);
    if (H < 1 || H > ggr::kEpiAttnMaxHeads) return fail(GGR_E_INVALID, "GgrEpipolarAttnEncPass.H %d is outside 1..%d", H, ggr::kEpiAttnMaxHeads);
    if (O < 1 || O > ggr::kEpiAttnEncMaxOctaves)
        return fail(GGR_E_INVALID, "GgrEpipolarAttnEncPass.num_octaves %d is outside 1..%d (without an encoding the pass to call is GgrEpipolarAttnPass)", O,
                    ggr::kEpiAttnEncMaxOctaves);
    const int lds = ggr::epipolar_attn_enc_lds_bytes(S, C, O);
    if (lds > ggr::kEpiAttnLdsLimit)      // (cannot happen inside the limits above: 64 rows of 292 floats are 74 752 bytes)
        return fail(GGR_E_INVALID, "GgrEpipolarAttnEncPass: S = %d, C = %d, num_octaves = %d needs %d bytes of LDS, above the %d bytes of a workgroup", S, C,
                    O, lds, ggr::kEpiAttnLdsLimit);
    if (N > 0) {
        const void* fwd_in[] = {ap->qk, ap->qe, ap->features, ap->depth, ap->out_ctx_f, ap->out_ctx_e, ap->out_attn};
        const char* fwd_name[] = {"qk", "qe", "features", "depth", "out_ctx_f", "out_ctx_e", "out_attn"};
        const void* bwd_in[] = {ap->qk, ap->qe, ap->features, ap->depth, ap->attn, ap->dL_dctx_f, ap->dL_dctx_e, ap->dL_dqk, ap->dL_dqe, ap->dL_dfeatures};
        const char* bwd_name[] = {"qk", "qe", "features", "depth", "attn", "dL_dctx_f", "dL_dctx_e", "dL_dqk", "dL_dqe", "dL_dfeatures"};
        for (int i = 0; i < (backward ? 10 : 7); ++i)
            if (!(backward ? bwd_in : fwd_in)[i])
                return fail(GGR_E_INVALID, "GgrEpipolarAttnEncPass.%s is NULL", (backward ? bwd_name : fwd_name)[i]);
    }
    const void* all[] = {ap->qk, ap->qe, ap->features, ap->depth, ap->out_ctx_f, ap->out_ctx_e, ap->out_attn, ap->attn, ap->dL_dctx_f, ap->dL_dctx_e,
                         ap->dL_dqk, ap->dL_dqe, ap->dL_dfeatures, ap->dL_ddepth};
    for (const void* p : all)
        if (((uintptr_t)p & 3u) != 0) return fail(GGR_E_INVALID, "GgrEpipolarAttnEncPass: a buffer is misaligned (every float array needs 4-byte alignment)");
    a->N = N; a->S = S; a->C = C; a->H = H; a->O = O;
    a->qk = ap->qk; a->qe = ap->qe; a->f = ap->features; a->d = ap->depth; a->ctx_f = ap->out_ctx_f; a->ctx_e = ap->out_ctx_e; a->attn_out = ap->out_attn;
    a->attn = ap->attn; a->g_f_ctx = ap->dL_dctx_f; a->g_e_ctx = ap->dL_dctx_e; a->g_qk = ap->dL_dqk; a->g_qe = ap->dL_dqe; a->g_f = ap->dL_dfeatures;
    a->g_d = ap->dL_ddepth;
    return GGR_OK;
}

int epipolar_attn_enc_launched(hipError_t e, const ggr::EpiAttnEncArgs& a, const char* what) {
    if (e != hipSuccess)
        return fail(GGR_E_INVALID, "GgrEpipolarAttnEncPass: S = %d, C = %d, num_octaves = %d needs %d bytes of LDS in one workgroup, which this device refused (%s)",
                    a.S, a.C, a.O, ggr::epipolar_attn_enc_lds_bytes(a.S, a.C, a.O), hipGetErrorString(e));
    e = hipGetLastError();
    if (e != hipSuccess) return fail(GGR_E_HIP, "%s: %s", what, hipGetErrorString(e));
    return GGR_OK;
}
}  // namespace

int ggr_epipolar_attention_encoded_forward(const GgrEpipolarAttnEncPass* ap, void* stream) {
    g_err[0] = 0;
    ggr::EpiAttnEncArgs a;
    const int rc = epipolar_attn_enc_pass_check(ap, false, &a);
    if (rc) return rc;
    if (a.N == 0) return GGR_OK;
    return epipolar_attn_enc_launched(ggr::launch_epipolar_attn_enc_forward(a, (hipStream_t)stream), a, "epipolar_attention_encoded_forward");
}

int ggr_epipolar_attention_encoded_backward(const GgrEpipolarAttnEncPass* ap, void* stream) {
    g_err[0] = 0;
    ggr::EpiAttnEncArgs a;
    const int rc = epipolar_attn_enc_pass_check(ap, true, &a);
    if (rc) return rc;
    if (a.N == 0) return GGR_OK;
    return epipolar_attn_enc_launched(ggr::launch_epipolar_attn_enc_backward(a, (hipStream_t)stream), a, "epipolar_attention_encoded_backward");
}

// ---- the image loss (image_loss.hip): masked MSE and SSIM of two images, and the gradient with respect to either --------------
namespace {
bool image_loss_sizes_ok(int B, int C, int H, int W) {
    return B >= 1 && C >= 1 && H >= 1 && W >= 1 && H <= ggr::kImageLossMaxSide && W <= ggr::kImageLossMaxSide &&
           (int64_t)B * C <= ggr::kImageLossMaxTiles && ggr::image_loss_tiles(1, 1, H, W) <= ggr::kImageLossMaxTiles / ((int64_t)B * C);
}

int image_loss_pass_check(const GgrImageLossPass* lp, bool backward, ggr::ImageLossArgs* a) {
    if (!lp) return fail(GGR_E_INVALID, "null GgrImageLossPass");
    if (lp->struct_size < (int32_t)sizeof(GgrImageLossPass))
        return fail(GGR_E_INVALID, "GgrImageLossPass.struct_size %d is smaller than the %d bytes of its fields", (int)lp->struct_size,
                    (int)sizeof(GgrImageLossPass));
    if (lp->reserved != 0) return fail(GGR_E_INVALID, "GgrImageLossPass.reserved must be 0, not %d", (int)lp->reserved);
    const int B = lp->batch, C = lp->channels, H = lp->height, W = lp->width, ws = lp->window_size;
    if (B < 1) return fail(GGR_E_INVALID, "GgrImageLossPass.batch %d is below 1", B);
    if (C < 1) return fail(GGR_E_INVALID, "GgrImageLossPass.channels %d is below 1", C);
    if (H < 1 || H > ggr::kImageLossMaxSide) return fail(GGR_E_INVALID, "GgrImageLossPass.height %d is outside 1..%d", H, ggr::kImageLossMaxSide);
    if (W < 1 || W > ggr::kImageLossMaxSide) return fail(GGR_E_INVALID, "GgrImageLossPass.width %d is outside 1..%d", W, ggr::kImageLossMaxSide);
    if (!image_loss_sizes_ok(B, C, H, W))
        return fail(GGR_E_INVALID, "GgrImageLossPass: batch %d x channels %d x height %d x width %d is more than %lld tiles", B, C, H, W,
                    (long long)ggr::kImageLossMaxTiles);
    if (ws < 1 || ws > ggr::kImageLossMaxWindow || ws % 2 == 0)
        return fail(GGR_E_INVALID, "GgrImageLossPass.window_size %d is not an odd number in 1..%d", ws, ggr::kImageLossMaxWindow);
    if (lp->size_average != 0 && lp->size_average != 1)
        return fail(GGR_E_INVALID, "GgrImageLossPass.size_average must be 0 or 1, not %d", (int)lp->size_average);
    if (!backward) {
        const void* in[] = {lp->pred, lp->target, lp->out_mse, lp->out_ssim, lp->mse_scale, lp->partials};
        const char* name[] = {"pred", "target", "out_mse", "out_ssim", "mse_scale", "partials"};
        for (int i = 0; i < 6; ++i)
            if (!in[i]) return fail(GGR_E_INVALID, "GgrImageLossPass.%s is NULL", name[i]);
        const int64_t need = ggr::image_loss_tiles(B, C, H, W) * ggr::kImageLossPartials * (int64_t)sizeof(double);
        if (lp->partials_bytes < need)
            return fail(GGR_E_INVALID, "GgrImageLossPass.partials_bytes %lld is smaller than the %lld bytes the pass needs", (long long)lp->partials_bytes,
                        (long long)need);
        if (((uintptr_t)lp->partials & 7u) != 0) return fail(GGR_E_INVALID, "GgrImageLossPass.partials is misaligned (it needs 8-byte alignment)");
    } else {
        const void* in[] = {lp->pred, lp->target, lp->mse_scale};
        const char* name[] = {"pred", "target", "mse_scale"};
        for (int i = 0; i < 3; ++i)
            if (!in[i]) return fail(GGR_E_INVALID, "GgrImageLossPass.%s is NULL", name[i]);
        if (!lp->dL_dmse && !lp->dL_dssim) return fail(GGR_E_INVALID, "GgrImageLossPass.dL_dmse and dL_dssim are both NULL");
        if (!lp->dL_dpred && !lp->dL_dtarget) return fail(GGR_E_INVALID, "GgrImageLossPass.dL_dpred and dL_dtarget are both NULL");
    }
    const void* all[] = {lp->pred, lp->target, lp->mask, lp->out_mse, lp->out_ssim, lp->mse_scale, lp->dL_dmse, lp->dL_dssim, lp->dL_dpred, lp->dL_dtarget};
    for (const void* p : all)
        if (((uintptr_t)p & 3u) != 0) return fail(GGR_E_INVALID, "GgrImageLossPass: a buffer is misaligned (every float array needs 4-byte alignment)");
    a->B = B; a->C = C; a->H = H; a->W = W; a->window = ws; a->size_average = lp->size_average;
    a->pred = lp->pred; a->target = lp->target; a->mask = lp->mask; a->mse = lp->out_mse; a->ssim = lp->out_ssim; a->mse_scale = lp->mse_scale;
    a->partials = (double*)lp->partials; a->g_mse = lp->dL_dmse; a->g_ssim = lp->dL_dssim; a->g_image = nullptr;
    ggr::image_loss_window(ws, a->w);
    return GGR_OK;
}
}  // namespace

int64_t ggr_image_loss_partials_bytes(int32_t batch, int32_t channels, int32_t height, int32_t width) {
    if (!image_loss_sizes_ok(batch, channels, height, width)) return -1;
    return ggr::image_loss_tiles(batch, channels, height, width) * ggr::kImageLossPartials * (int64_t)sizeof(double);
}

int ggr_image_loss_window(int32_t window_size, float* out) {
    g_err[0] = 0;
    if (window_size < 1 || window_size > ggr::kImageLossMaxWindow || window_size % 2 == 0)
        return fail(GGR_E_INVALID, "ggr_image_loss_window: window_size %d is not an odd number in 1..%d", (int)window_size, ggr::kImageLossMaxWindow);
    if (!out) return fail(GGR_E_INVALID, "ggr_image_loss_window: out is NULL");
    float w[ggr::kImageLossMaxWindow];
    ggr::image_loss_window(window_size, w);
    memcpy(out, w, sizeof(float) * (size_t)window_size);
    return GGR_OK;
}

int ggr_image_loss_forward(const GgrImageLossPass* lp, void* stream) {
    g_err[0] = 0;
    ggr::ImageLossArgs a;
    const int rc = image_loss_pass_check(lp, false, &a);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ggr::launch_image_loss_forward(a, s);
    KCHECK(false, s, "image_loss_forward");
    return GGR_OK;
}

int ggr_image_loss_backward(const GgrImageLossPass* lp, void* stream) {
    g_err[0] = 0;
    ggr::ImageLossArgs a;
    const int rc = image_loss_pass_check(lp, true, &a);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (lp->dL_dpred) {
        a.g_image = lp->dL_dpred;
        ggr::launch_image_loss_backward(a, s);
    }
    if (lp->dL_dtarget) {      // SSIM is symmetric and the MSE term changes its sign with the difference: the same kernel, roles exchanged
        a.pred = lp->target; a.target = lp->pred; a.g_image = lp->dL_dtarget;
        ggr::launch_image_loss_backward(a, s);
    }
    KCHECK(false, s, "image_loss_backward");
    return GGR_OK;
}

// ---- the multi-view photometric loss (photometric_loss.hip) ----------------------------------------------------------------------
namespace {
bool photo_loss_sizes_ok(int V, int n, int H, int W, int automask) {
    return V >= 1 && n >= 1 && n <= ggr::kPhotoMaxIters && H >= 2 && W >= 2 && H <= ggr::kPhotoMaxSide && W <= ggr::kPhotoMaxSide &&
           (automask == 0 || automask == 1) && (int64_t)V * (automask ? 2 : 1) <= ggr::kPhotoMaxCandidates;
}

int photo_loss_pass_check(const GgrPhotometricLossPass* lp, bool backward, ggr::PhotoLossArgs* a) {
    if (!lp) return fail(GGR_E_INVALID, "null GgrPhotometricLossPass");
    if (lp->struct_size < (int32_t)sizeof(GgrPhotometricLossPass))
        return fail(GGR_E_INVALID, "GgrPhotometricLossPass.struct_size %d is smaller than the %d bytes of its fields", (int)lp->struct_size,
                    (int)sizeof(GgrPhotometricLossPass));
    if (lp->reserved != 0 || lp->reserved2 != 0)
        return fail(GGR_E_INVALID, "GgrPhotometricLossPass.reserved must be 0, not %d / %d", (int)lp->reserved, (int)lp->reserved2);
    const int V = lp->num_views, n = lp->num_iters, H = lp->height, W = lp->width;
    if (V < 1) return fail(GGR_E_INVALID, "GgrPhotometricLossPass.num_views %d is below 1", V);
    if (n < 1 || n > ggr::kPhotoMaxIters) return fail(GGR_E_INVALID, "GgrPhotometricLossPass.num_iters %d is outside 1..%d", n, ggr::kPhotoMaxIters);
    if (H < 2 || H > ggr::kPhotoMaxSide) return fail(GGR_E_INVALID, "GgrPhotometricLossPass.height %d is outside 2..%d", H, ggr::kPhotoMaxSide);
    if (W < 2 || W > ggr::kPhotoMaxSide) return fail(GGR_E_INVALID, "GgrPhotometricLossPass.width %d is outside 2..%d", W, ggr::kPhotoMaxSide);
    if (lp->automask != 0 && lp->automask != 1) return fail(GGR_E_INVALID, "GgrPhotometricLossPass.automask must be 0 or 1, not %d", (int)lp->automask);
    const int C = V * (lp->automask ? 2 : 1);
    if (!photo_loss_sizes_ok(V, n, H, W, lp->automask))
        return fail(GGR_E_INVALID, "GgrPhotometricLossPass: %d views make %d candidates per pixel, more than the %d the pass takes", V, C,
                    ggr::kPhotoMaxCandidates);
    if (!(lp->ssim_loss_weight > 0.f && lp->ssim_loss_weight <= 1.f))
        return fail(GGR_E_INVALID, "GgrPhotometricLossPass.ssim_loss_weight %g is not in (0, 1]", (double)lp->ssim_loss_weight);
    const float nonneg[] = {lp->smooth_loss_weight, lp->C1, lp->C2, lp->clip_loss, lp->gamma};
    const char* nname[] = {"smooth_loss_weight", "C1", "C2", "clip_loss", "gamma"};
    for (int i = 0; i < 5; ++i)
        if (!(nonneg[i] >= 0.f && nonneg[i] <= 3.0e38f)) return fail(GGR_E_INVALID, "GgrPhotometricLossPass.%s %g is negative or not finite", nname[i], (double)nonneg[i]);
    {
        const void* in[] = {lp->image, lp->ref_imgs, lp->inv_depths, lp->K, lp->ref_Ks, lp->poses, lp->planes, lp->workspace, lp->out_thresholds, lp->state, lp->choice};
        const char* name[] = {"image", "ref_imgs", "inv_depths", "K", "ref_Ks", "poses", "planes", "workspace", "out_thresholds", "state", "choice"};
        for (int i = 0; i < 11; ++i)
            if (!in[i]) return fail(GGR_E_INVALID, "GgrPhotometricLossPass.%s is NULL", name[i]);
    }
    if (!backward) {
        const void* in[] = {lp->out_loss, lp->out_photometric, lp->out_smoothness};
        const char* name[] = {"out_loss", "out_photometric", "out_smoothness"};
        for (int i = 0; i < 3; ++i)
            if (!in[i]) return fail(GGR_E_INVALID, "GgrPhotometricLossPass.%s is NULL", name[i]);
    } else {
        const void* in[] = {lp->dL_dloss, lp->dL_dinv_depths, lp->dL_dposes};
        const char* name[] = {"dL_dloss", "dL_dinv_depths", "dL_dposes"};
        for (int i = 0; i < 3; ++i)
            if (!in[i]) return fail(GGR_E_INVALID, "GgrPhotometricLossPass.%s is NULL", name[i]);
    }
    const int64_t need_planes = ggr::photo_loss_planes(V, n, lp->automask) * H * W * (int64_t)sizeof(float);
    const int64_t need_ws = ggr::photo_loss_workspace_doubles(V, n, H, W, lp->automask) * (int64_t)sizeof(double);
    if (lp->planes_bytes < need_planes)
        return fail(GGR_E_INVALID, "GgrPhotometricLossPass.planes_bytes %lld is smaller than the %lld bytes the pass needs", (long long)lp->planes_bytes, (long long)need_planes);
    if (lp->workspace_bytes < need_ws)
        return fail(GGR_E_INVALID, "GgrPhotometricLossPass.workspace_bytes %lld is smaller than the %lld bytes the pass needs", (long long)lp->workspace_bytes, (long long)need_ws);
    if (((uintptr_t)lp->workspace & 7u) != 0) return fail(GGR_E_INVALID, "GgrPhotometricLossPass.workspace is misaligned (it needs 8-byte alignment)");
    const void* all[] = {lp->image, lp->ref_imgs, lp->inv_depths, lp->K, lp->ref_Ks, lp->poses, lp->planes, lp->out_thresholds, lp->state, lp->out_loss,
                         lp->out_photometric, lp->out_smoothness, lp->dL_dloss, lp->dL_dinv_depths, lp->dL_dposes};
    for (const void* p : all)
        if (((uintptr_t)p & 3u) != 0) return fail(GGR_E_INVALID, "GgrPhotometricLossPass: a buffer is misaligned (every float array needs 4-byte alignment)");
    a->V = V; a->n = n; a->H = H; a->W = W; a->automask = lp->automask; a->clip_on = lp->clip_loss > 0.f; a->C = C;
    a->w_ssim = lp->ssim_loss_weight; a->w_smooth = lp->smooth_loss_weight; a->C1 = lp->C1; a->C2 = lp->C2; a->clip = lp->clip_loss; a->gamma = lp->gamma;
    a->image = lp->image; a->ref_imgs = lp->ref_imgs; a->inv_depths = lp->inv_depths; a->K = lp->K; a->ref_Ks = lp->ref_Ks; a->poses = lp->poses;
    a->planes = lp->planes; a->workspace = (double*)lp->workspace; a->thresholds = lp->out_thresholds; a->state = lp->state; a->choice = lp->choice;
    a->loss = lp->out_loss; a->photo = lp->out_photometric; a->smooth = lp->out_smoothness;
    a->g_loss = lp->dL_dloss; a->g_inv = lp->dL_dinv_depths; a->g_poses = lp->dL_dposes;
    return GGR_OK;
}
}  // namespace

int64_t ggr_photometric_loss_planes_bytes(int32_t num_views, int32_t num_iters, int32_t height, int32_t width, int32_t automask) {
    if (!photo_loss_sizes_ok(num_views, num_iters, height, width, automask)) return -1;
    return ggr::photo_loss_planes(num_views, num_iters, automask) * height * width * (int64_t)sizeof(float);
}

int64_t ggr_photometric_loss_workspace_bytes(int32_t num_views, int32_t num_iters, int32_t height, int32_t width, int32_t automask) {
    if (!photo_loss_sizes_ok(num_views, num_iters, height, width, automask)) return -1;
    return ggr::photo_loss_workspace_doubles(num_views, num_iters, height, width, automask) * (int64_t)sizeof(double);
}

int ggr_photometric_loss_forward(const GgrPhotometricLossPass* lp, void* stream) {
    g_err[0] = 0;
    ggr::PhotoLossArgs a;
    const int rc = photo_loss_pass_check(lp, false, &a);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ggr::launch_photo_loss_forward(a, s);
    KCHECK(false, s, "photometric_loss_forward");
    return GGR_OK;
}

int ggr_photometric_loss_backward(const GgrPhotometricLossPass* lp, void* stream) {
    g_err[0] = 0;
    ggr::PhotoLossArgs a;
    const int rc = photo_loss_pass_check(lp, true, &a);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ggr::launch_photo_loss_backward(a, s);
    KCHECK(false, s, "photometric_loss_backward");
    return GGR_OK;
}

// ---- the feature-metric cost map (warp_cost.hip) -----------------------------------------------------------------------------------
namespace {
bool warp_cost_sizes_ok(int V, int h, int w) {
    return V >= 1 && V <= ggr::kWarpMaxViews && h >= 2 && w >= 2 && h <= ggr::kWarpMaxSide && w <= ggr::kWarpMaxSide;
}

int warp_cost_pass_check(const GgrWarpCostPass* wp, bool backward, ggr::WarpCostArgs* a) {
    if (!wp) return fail(GGR_E_INVALID, "null GgrWarpCostPass");
    if (wp->struct_size < (int32_t)sizeof(GgrWarpCostPass))
        return fail(GGR_E_INVALID, "GgrWarpCostPass.struct_size %d is smaller than the %d bytes of its fields", (int)wp->struct_size, (int)sizeof(GgrWarpCostPass));
    if (wp->reserved != 0 || wp->reserved2 != 0)
        return fail(GGR_E_INVALID, "GgrWarpCostPass.reserved must be 0, not %d / %d", (int)wp->reserved, (int)wp->reserved2);
    const int V = wp->num_views, C = wp->channels, h = wp->height, w = wp->width;
    if (V < 1 || V > ggr::kWarpMaxViews) return fail(GGR_E_INVALID, "GgrWarpCostPass.num_views %d is outside 1..%d", V, ggr::kWarpMaxViews);
    if (C < 1 || C > ggr::kWarpMaxChannels) return fail(GGR_E_INVALID, "GgrWarpCostPass.channels %d is outside 1..%d", C, ggr::kWarpMaxChannels);
    if (h < 2 || h > ggr::kWarpMaxSide) return fail(GGR_E_INVALID, "GgrWarpCostPass.height %d is outside 2..%d", h, ggr::kWarpMaxSide);
    if (w < 2 || w > ggr::kWarpMaxSide) return fail(GGR_E_INVALID, "GgrWarpCostPass.width %d is outside 2..%d", w, ggr::kWarpMaxSide);
    if (wp->reduce_mean != 0 && wp->reduce_mean != 1) return fail(GGR_E_INVALID, "GgrWarpCostPass.reduce_mean must be 0 or 1, not %d", (int)wp->reduce_mean);
    if (wp->fold_disp != 0 && wp->fold_disp != 1) return fail(GGR_E_INVALID, "GgrWarpCostPass.fold_disp must be 0 or 1, not %d", (int)wp->fold_disp);
    if (!(wp->scale_factor > 0.f && wp->scale_factor <= 3.0e38f))
        return fail(GGR_E_INVALID, "GgrWarpCostPass.scale_factor %g is not positive and finite", (double)wp->scale_factor);
    if (wp->fold_disp && !(wp->min_depth > 0.f && wp->min_depth < wp->max_depth && wp->max_depth <= 3.0e38f))
        return fail(GGR_E_INVALID, "GgrWarpCostPass.min_depth %g / .max_depth %g are not 0 < min_depth < max_depth < inf", (double)wp->min_depth, (double)wp->max_depth);
    {
        const void* in[] = {wp->fmap, wp->fmaps_ref, wp->inv_depth, wp->K, wp->ref_Ks, wp->poses};
        const char* name[] = {"fmap", "fmaps_ref", "inv_depth", "K", "ref_Ks", "poses"};
        for (int i = 0; i < 6; ++i)
            if (!in[i]) return fail(GGR_E_INVALID, "GgrWarpCostPass.%s is NULL", name[i]);
    }
    if (!backward) {
        if (!wp->out_cost) return fail(GGR_E_INVALID, "GgrWarpCostPass.out_cost is NULL");
    } else {
        if (!wp->dL_dcost) return fail(GGR_E_INVALID, "GgrWarpCostPass.dL_dcost is NULL");
        if (!wp->dL_dfmap && !wp->dL_dfmaps_ref && !wp->dL_dinv_depth && !wp->dL_dposes)
            return fail(GGR_E_INVALID, "GgrWarpCostPass: no output (dL_dfmap, dL_dfmaps_ref, dL_dinv_depth and dL_dposes are all NULL)");
        if (wp->dL_dposes) {
            const int64_t need = ggr::warp_cost_workspace_doubles(V, h, w) * (int64_t)sizeof(double);
            if (!wp->workspace) return fail(GGR_E_INVALID, "GgrWarpCostPass.workspace is NULL");
            if (wp->workspace_bytes < need)
                return fail(GGR_E_INVALID, "GgrWarpCostPass.workspace_bytes %lld is smaller than the %lld bytes the pass needs", (long long)wp->workspace_bytes, (long long)need);
            if (((uintptr_t)wp->workspace & 7u) != 0) return fail(GGR_E_INVALID, "GgrWarpCostPass.workspace is misaligned (it needs 8-byte alignment)");
        }
    }
    const void* all[] = {wp->fmap, wp->fmaps_ref, wp->inv_depth, wp->K, wp->ref_Ks, wp->poses, wp->out_cost, wp->out_cells, wp->dL_dcost, wp->dL_dfmap,
                         wp->dL_dfmaps_ref, wp->dL_dinv_depth, wp->dL_dposes};
    for (const void* p : all)
        if (((uintptr_t)p & 3u) != 0) return fail(GGR_E_INVALID, "GgrWarpCostPass: a buffer is misaligned (every array needs 4-byte alignment)");
    a->V = V; a->C = C; a->h = h; a->w = w; a->mean = wp->reduce_mean; a->disp_on = wp->fold_disp;
    a->scale = wp->scale_factor;
    a->disp_a = 0.f; a->disp_b = 1.f;
    if (wp->fold_disp) {        // disp_to_depth forms both numbers in double and the tensor arithmetic rounds them to float
        const double lo = 1.0 / (double)wp->max_depth, hi = 1.0 / (double)wp->min_depth;
        a->disp_a = (float)lo;
        a->disp_b = (float)(hi - lo);
    }
    a->fmap = wp->fmap; a->fmaps_ref = wp->fmaps_ref; a->inv_depth = wp->inv_depth; a->K = wp->K; a->ref_Ks = wp->ref_Ks; a->poses = wp->poses;
    a->cost = wp->out_cost; a->cells = backward ? nullptr : wp->out_cells; a->workspace = (double*)wp->workspace;
    a->g_cost = wp->dL_dcost; a->g_fmap = wp->dL_dfmap; a->g_fmaps_ref = wp->dL_dfmaps_ref; a->g_inv = wp->dL_dinv_depth; a->g_poses = wp->dL_dposes;
    return GGR_OK;
}
}  // namespace

int64_t ggr_warp_cost_workspace_bytes(int32_t num_views, int32_t height, int32_t width) {
    if (!warp_cost_sizes_ok(num_views, height, width)) return -1;
    return ggr::warp_cost_workspace_doubles(num_views, height, width) * (int64_t)sizeof(double);
}

int ggr_warp_cost_forward(const GgrWarpCostPass* wp, void* stream) {
    g_err[0] = 0;
    ggr::WarpCostArgs a;
    const int rc = warp_cost_pass_check(wp, false, &a);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ggr::launch_warp_cost_forward(a, s);
    KCHECK(false, s, "warp_cost_forward");
    return GGR_OK;
}

int ggr_warp_cost_backward(const GgrWarpCostPass* wp, void* stream) {
    g_err[0] = 0;
    ggr::WarpCostArgs a;
    const int rc = warp_cost_pass_check(wp, true, &a);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ggr::launch_warp_cost_backward(a, s);
    KCHECK(false, s, "warp_cost_backward");
    return GGR_OK;
}

// ---- the convex depth upsampling (upsample_depth.hip) ------------------------------------------------------------------------------
namespace {
// the kernels index with 32-bit ints: the mask (the largest input) and `up` must each stay below 2^31 elements
bool upsample_depth_sizes_ok(int64_t N, int64_t h, int64_t w, int64_t r) {
    if (N < 1 || h < 1 || w < 1 || r < 1 || r > ggr::kUpsampleMaxRatio) return false;
    if (h * r > ggr::kUpsampleMaxSide || w * r > ggr::kUpsampleMaxSide) return false;
    const int64_t cells = h * w;                                    // (at most 2^32 here)
    return N <= INT32_MAX / cells && N * cells <= INT32_MAX / (9 * r * r);
}

int upsample_depth_pass_check(const GgrUpsampleDepthPass* up, bool backward, ggr::UpsampleDepthArgs* a) {
    if (!up) return fail(GGR_E_INVALID, "null GgrUpsampleDepthPass");
    if (up->struct_size < (int32_t)sizeof(GgrUpsampleDepthPass))
        return fail(GGR_E_INVALID, "GgrUpsampleDepthPass.struct_size %d is smaller than the %d bytes of its fields", (int)up->struct_size, (int)sizeof(GgrUpsampleDepthPass));
    if (up->reserved != 0 || up->reserved2 != 0)
        return fail(GGR_E_INVALID, "GgrUpsampleDepthPass.reserved must be 0, not %d / %d", (int)up->reserved, (int)up->reserved2);
    const int N = up->batch, h = up->height, w = up->width, r = up->ratio, Ho = up->out_height, Wo = up->out_width;
    if (r < 1 || r > ggr::kUpsampleMaxRatio) return fail(GGR_E_INVALID, "GgrUpsampleDepthPass.ratio %d is outside 1..%d", r, ggr::kUpsampleMaxRatio);
    if (N < 1) return fail(GGR_E_INVALID, "GgrUpsampleDepthPass.batch %d is below 1", N);
    if (h < 1) return fail(GGR_E_INVALID, "GgrUpsampleDepthPass.height %d is below 1", h);
    if (w < 1) return fail(GGR_E_INVALID, "GgrUpsampleDepthPass.width %d is below 1", w);
    if (Ho < 1) return fail(GGR_E_INVALID, "GgrUpsampleDepthPass.out_height %d is below 1", Ho);
    if (Wo < 1) return fail(GGR_E_INVALID, "GgrUpsampleDepthPass.out_width %d is below 1", Wo);
    if (up->fold_disp != 0 && up->fold_disp != 1) return fail(GGR_E_INVALID, "GgrUpsampleDepthPass.fold_disp must be 0 or 1, not %d", (int)up->fold_disp);
    if (up->fold_disp && !(up->min_depth > 0.f && up->min_depth < up->max_depth && up->max_depth <= 3.0e38f))
        return fail(GGR_E_INVALID, "GgrUpsampleDepthPass.min_depth %g / .max_depth %g are not 0 < min_depth < max_depth < inf", (double)up->min_depth, (double)up->max_depth);
    if (!upsample_depth_sizes_ok(N, h, w, r) || Ho > ggr::kUpsampleMaxSide || Wo > ggr::kUpsampleMaxSide || (int64_t)N * Ho > INT32_MAX / (int64_t)Wo)
        return fail(GGR_E_INVALID, "GgrUpsampleDepthPass: batch %d, %d x %d cells at ratio %d to %d x %d is beyond 32-bit indexing (2^31 - 1 elements per array, "
                    "sides of %d)", N, h, w, r, Ho, Wo, ggr::kUpsampleMaxSide);
    if (!up->depth) return fail(GGR_E_INVALID, "GgrUpsampleDepthPass.depth is NULL");
    if (!up->mask) return fail(GGR_E_INVALID, "GgrUpsampleDepthPass.mask is NULL");
    if (!backward) {
        if (!up->out) return fail(GGR_E_INVALID, "GgrUpsampleDepthPass.out is NULL");
    } else {
        if (!up->dL_dout) return fail(GGR_E_INVALID, "GgrUpsampleDepthPass.dL_dout is NULL");
        if (!up->dL_dmask && !up->dL_ddepth) return fail(GGR_E_INVALID, "GgrUpsampleDepthPass: no output (dL_dmask and dL_ddepth are both NULL)");
    }
    const int64_t need = ggr::upsample_depth_workspace_floats(N, h, w, r) * (int64_t)sizeof(float);
    if (!up->workspace) return fail(GGR_E_INVALID, "GgrUpsampleDepthPass.workspace is NULL");
    if (up->workspace_bytes < need)
        return fail(GGR_E_INVALID, "GgrUpsampleDepthPass.workspace_bytes %lld is smaller than the %lld bytes the pass needs", (long long)up->workspace_bytes, (long long)need);
    const void* all[] = {up->depth, up->mask, up->out, up->workspace, up->dL_dout, up->dL_dmask, up->dL_ddepth};
    for (const void* p : all)
        if (((uintptr_t)p & 3u) != 0) return fail(GGR_E_INVALID, "GgrUpsampleDepthPass: a buffer is misaligned (every array needs 4-byte alignment)");
    a->N = N; a->h = h; a->w = w; a->r = r; a->Ho = Ho; a->Wo = Wo; a->disp_on = up->fold_disp;
    a->disp_a = 0.f; a->disp_b = 1.f;
    if (up->fold_disp) {        // disp_to_depth forms both numbers in double and the tensor arithmetic rounds them to float
        const double lo = 1.0 / (double)up->max_depth, hi = 1.0 / (double)up->min_depth;
        a->disp_a = (float)lo;
        a->disp_b = (float)(hi - lo);
    }
    const int H = h * r, W = w * r;     // torch's area_pixel_compute_scale: (float)(in - 1) / (out - 1), 0 for one output index
    a->sy = Ho > 1 ? (float)(H - 1) / (float)(Ho - 1) : 0.f;
    a->sx = Wo > 1 ? (float)(W - 1) / (float)(Wo - 1) : 0.f;
    a->inv_sy = (Ho > 1 && H > 1) ? (float)(Ho - 1) / (float)(H - 1) : 0.f;
    a->inv_sx = (Wo > 1 && W > 1) ? (float)(Wo - 1) / (float)(W - 1) : 0.f;
    a->depth = up->depth; a->mask = up->mask; a->out = up->out; a->workspace = (float*)up->workspace;
    a->g_out = up->dL_dout; a->g_mask = up->dL_dmask; a->g_depth = up->dL_ddepth;
    return GGR_OK;
}
}  // namespace

int64_t ggr_upsample_depth_workspace_bytes(int32_t batch, int32_t height, int32_t width, int32_t ratio) {
    if (!upsample_depth_sizes_ok(batch, height, width, ratio)) return -1;
    return ggr::upsample_depth_workspace_floats(batch, height, width, ratio) * (int64_t)sizeof(float);
}

int ggr_upsample_depth_forward(const GgrUpsampleDepthPass* up, void* stream) {
    g_err[0] = 0;
    ggr::UpsampleDepthArgs a;
    const int rc = upsample_depth_pass_check(up, false, &a);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ggr::launch_upsample_depth_forward(a, s);
    KCHECK(false, s, "upsample_depth_forward");
    return GGR_OK;
}

int ggr_upsample_depth_backward(const GgrUpsampleDepthPass* up, void* stream) {
    g_err[0] = 0;
    ggr::UpsampleDepthArgs a;
    const int rc = upsample_depth_pass_check(up, true, &a);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ggr::launch_upsample_depth_backward(a, s);
    KCHECK(false, s, "upsample_depth_backward");
    return GGR_OK;
}

// ---- the ConvGRU gate math (gru_gates.hip) ------------------------------------------------------------------------------------------
namespace {
enum GruCall { GRU_GATE_FWD, GRU_BLEND_FWD, GRU_BLEND_BWD, GRU_GATE_BWD };

int gru_pass_check(const GgrGruPass* gp, GruCall call, ggr::GruArgs* a) {
    if (!gp) return fail(GGR_E_INVALID, "null GgrGruPass");
    if (gp->struct_size < (int32_t)sizeof(GgrGruPass))
        return fail(GGR_E_INVALID, "GgrGruPass.struct_size %d is smaller than the %d bytes of its fields", (int)gp->struct_size, (int)sizeof(GgrGruPass));
    if (gp->reserved != 0) return fail(GGR_E_INVALID, "GgrGruPass.reserved must be 0, not %d", (int)gp->reserved);
    const int N = gp->batch, Ch = gp->channels, H = gp->height, W = gp->width;
    if (N < 1) return fail(GGR_E_INVALID, "GgrGruPass.batch %d is below 1", N);
    if (Ch < 1) return fail(GGR_E_INVALID, "GgrGruPass.channels %d is below 1", Ch);
    if (H < 1) return fail(GGR_E_INVALID, "GgrGruPass.height %d is below 1", H);
    if (W < 1) return fail(GGR_E_INVALID, "GgrGruPass.width %d is below 1", W);
    const int64_t M = (int64_t)Ch * H, lim = (int64_t)1 << 30;      // N M < 2^30: the [N,2Ch,H,W] arrays stay below 2^31 elements
    if (M >= lim || M * W >= lim || M * W * N >= lim)
        return fail(GGR_E_INVALID, "GgrGruPass: batch %d of %d x %d x %d is beyond 32-bit indexing (N 2 Ch H W must stay below 2^31)", N, Ch, H, W);
    *a = ggr::GruArgs{};
    a->N = N; a->M = (int)(M * W);
#define GRU_NEED(field) if (!gp->field) return fail(GGR_E_INVALID, "GgrGruPass." #field " is NULL")
    GRU_NEED(h);
    switch (call) {
    case GRU_GATE_FWD:
        GRU_NEED(a_zr_h); GRU_NEED(z); GRU_NEED(r); GRU_NEED(rh);
        a->a_zr_h = gp->a_zr_h; a->a_zr_x = gp->a_zr_x; a->z = gp->z; a->r = gp->r; a->rh = gp->rh;
        break;
    case GRU_BLEND_FWD:
        GRU_NEED(a_q_h); GRU_NEED(z); GRU_NEED(q); GRU_NEED(out_h);
        if (gp->out_h == gp->h) return fail(GGR_E_INVALID, "GgrGruPass.out_h is h itself: the blend does not run in place (the backward reads h)");
        a->a_q_h = gp->a_q_h; a->a_q_x = gp->a_q_x; a->z = gp->z; a->q = gp->q; a->out_h = gp->out_h;
        break;
    case GRU_BLEND_BWD:
        GRU_NEED(dL_dout_h); GRU_NEED(z); GRU_NEED(q);
        if (!gp->dL_da_q && !gp->dL_da_zr && !gp->dL_dh_part) return fail(GGR_E_INVALID, "GgrGruPass: no output (dL_da_q, dL_da_zr and dL_dh_part are all NULL)");
        a->g_out_h = gp->dL_dout_h; a->z = gp->z; a->q = gp->q; a->g_a_q = gp->dL_da_q; a->g_a_zr = gp->dL_da_zr; a->g_h_part = gp->dL_dh_part;
        break;
    case GRU_GATE_BWD:
        GRU_NEED(dL_drh); GRU_NEED(r);
        if (!gp->dL_da_zr && !gp->dL_dh) return fail(GGR_E_INVALID, "GgrGruPass: no output (dL_da_zr and dL_dh are both NULL)");
        a->g_rh = gp->dL_drh; a->r = gp->r; a->g_a_zr = gp->dL_da_zr; a->g_h_part = gp->dL_dh_part; a->g_h = gp->dL_dh;
        break;
    }
#undef GRU_NEED
    a->h = gp->h;
    const void* used[] = {a->a_zr_h, a->a_zr_x, a->h, a->z, a->r, a->rh, a->a_q_h, a->a_q_x, a->q, a->out_h, a->g_out_h, a->g_a_q, a->g_a_zr, a->g_h_part, a->g_rh, a->g_h};
    uintptr_t bits = 0;
    for (const void* p : used) bits |= (uintptr_t)p;
    if ((bits & 3u) != 0) return fail(GGR_E_INVALID, "GgrGruPass: a buffer is misaligned (every array needs 4-byte alignment)");
    a->vec = (a->M % 4 == 0 && (bits & 15u) == 0) ? 1 : 0;
    return GGR_OK;
}

int gru_call(const GgrGruPass* gp, void* stream, GruCall call, void (*launch)(const ggr::GruArgs&, hipStream_t), const char* what) {
    g_err[0] = 0;
    ggr::GruArgs a;
    const int rc = gru_pass_check(gp, call, &a);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    launch(a, s);
    KCHECK(false, s, what);
    return GGR_OK;
}
}  // namespace

int ggr_gru_gate_forward(const GgrGruPass* gp, void* stream) { return gru_call(gp, stream, GRU_GATE_FWD, ggr::launch_gru_gate_forward, "gru_gate_forward"); }
int ggr_gru_blend_forward(const GgrGruPass* gp, void* stream) { return gru_call(gp, stream, GRU_BLEND_FWD, ggr::launch_gru_blend_forward, "gru_blend_forward"); }
int ggr_gru_blend_backward(const GgrGruPass* gp, void* stream) { return gru_call(gp, stream, GRU_BLEND_BWD, ggr::launch_gru_blend_backward, "gru_blend_backward"); }
int ggr_gru_gate_backward(const GgrGruPass* gp, void* stream) { return gru_call(gp, stream, GRU_GATE_BWD, ggr::launch_gru_gate_backward, "gru_gate_backward"); }

// ---- the ConvGRU half-step's convolutions with the gate math on the accumulators (gru_conv.hip) --------------------------------------
namespace {
int gru_conv_pass_check(const GgrGruConvPass* cp, ggr::GruConvArgs* a) {
    if (!cp) return fail(GGR_E_INVALID, "null GgrGruConvPass");
    if (cp->struct_size < (int32_t)sizeof(GgrGruConvPass))
        return fail(GGR_E_INVALID, "GgrGruConvPass.struct_size %d is smaller than the %d bytes of its fields", (int)cp->struct_size, (int)sizeof(GgrGruConvPass));
    if (cp->reserved != 0) return fail(GGR_E_INVALID, "GgrGruConvPass.reserved must be 0, not %d", (int)cp->reserved);
    const int N = cp->batch, Ch = cp->channels, Cx = cp->in_channels, H = cp->height, W = cp->width, kh = cp->kernel_h, kw = cp->kernel_w;
    if (N < 1) return fail(GGR_E_INVALID, "GgrGruConvPass.batch %d is below 1", N);
    if (Ch < 1) return fail(GGR_E_INVALID, "GgrGruConvPass.channels %d is below 1", Ch);
    if (Cx < 1) return fail(GGR_E_INVALID, "GgrGruConvPass.in_channels %d is below 1", Cx);
    if (H < 1) return fail(GGR_E_INVALID, "GgrGruConvPass.height %d is below 1", H);
    if (W < 1) return fail(GGR_E_INVALID, "GgrGruConvPass.width %d is below 1", W);
    if (kh < 1 || kh > ggr::kGruConvMaxSide || kh % 2 == 0) return fail(GGR_E_INVALID, "GgrGruConvPass.kernel_h %d is not 1, 3 or 5", kh);
    if (kw < 1 || kw > ggr::kGruConvMaxSide || kw % 2 == 0) return fail(GGR_E_INVALID, "GgrGruConvPass.kernel_w %d is not 1, 3 or 5", kw);
    const int epi = cp->epilogue;
    if (epi != GGR_GRU_CONV_GATE && epi != GGR_GRU_CONV_BLEND && epi != GGR_GRU_CONV_RAW)
        return fail(GGR_E_INVALID, "GgrGruConvPass.epilogue %d is none of GGR_GRU_CONV_GATE, _BLEND, _RAW", epi);
    if (epi == GGR_GRU_CONV_RAW && cp->out_channels < 1) return fail(GGR_E_INVALID, "GgrGruConvPass.out_channels %d is below 1", (int)cp->out_channels);
    const int64_t lim = (int64_t)1 << 31, half = lim / 2, M = (int64_t)Ch * H;      // N M W < 2^30, as for GgrGruPass: no product overflows on the way
    if (M >= half || M * W >= half || M * W * N >= half)
        return fail(GGR_E_INVALID, "GgrGruConvPass: batch %d of %d x %d x %d is beyond 32-bit indexing (N 2 Ch H W must stay below 2^31)", N, Ch, H, W);
    const int64_t P = (int64_t)N * H * W, Cout = epi == GGR_GRU_CONV_GATE ? 2 * (int64_t)Ch : epi == GGR_GRU_CONV_BLEND ? Ch : cp->out_channels;
    const int64_t Cmax = Cx > Cout ? Cx : Cout, Kmax = (int64_t)(Ch > Cx ? Ch : Cx) * kh * kw;
    if (Cmax * P >= lim || Kmax >= lim - 64)
        return fail(GGR_E_INVALID, "GgrGruConvPass: batch %d, %d + %d -> %lld channels of %d x %d is beyond 32-bit indexing (every array must stay below 2^31 elements)",
                    N, Ch, Cx, (long long)Cout, H, W);
    *a = ggr::GruConvArgs{};
    a->N = N; a->Ch = Ch; a->Cx = Cx; a->H = H; a->W = W; a->KH = kh; a->KW = kw; a->Cout = (int)Cout;
    a->epilogue = epi == GGR_GRU_CONV_GATE ? ggr::kGruConvGate : epi == GGR_GRU_CONV_BLEND ? ggr::kGruConvBlend : ggr::kGruConvRaw;
#define GRUC_NEED(field) if (!cp->field) return fail(GGR_E_INVALID, "GgrGruConvPass." #field " is NULL")
    GRUC_NEED(a); GRUC_NEED(x); GRUC_NEED(w_h); GRUC_NEED(w_x);
    a->a = cp->a; a->x = cp->x; a->w_h = cp->w_h; a->w_x = cp->w_x; a->bias = cp->bias;
    if (epi == GGR_GRU_CONV_GATE) {
        GRUC_NEED(h); GRUC_NEED(z); GRUC_NEED(rh);
        a->h = cp->h; a->z = cp->z; a->rh = cp->rh;
    } else if (epi == GGR_GRU_CONV_BLEND) {
        GRUC_NEED(h); GRUC_NEED(z); GRUC_NEED(out_h);
        if (cp->out_h == cp->h) return fail(GGR_E_INVALID, "GgrGruConvPass.out_h is h itself: the blend does not run in place");
        a->h = cp->h; a->z = cp->z; a->out_h = cp->out_h;
    } else {
        GRUC_NEED(raw);
        a->raw = cp->raw;
    }
#undef GRUC_NEED
    const int64_t need = (int64_t)ggr_gru_conv_workspace_bytes(cp);
    if (cp->workspace_bytes < need || (need > 0 && !cp->workspace))
        return fail(GGR_E_INVALID, "GgrGruConvPass.workspace_bytes %lld is smaller than the %lld bytes the pass needs", (long long)cp->workspace_bytes, (long long)need);
    const void* used[] = {a->a, a->x, a->w_h, a->w_x, a->bias, a->h, a->z, a->rh, a->out_h, a->raw, cp->workspace};
    uintptr_t bits = 0;
    for (const void* p : used) bits |= (uintptr_t)p;
    if ((bits & 3u) != 0) return fail(GGR_E_INVALID, "GgrGruConvPass: a buffer is misaligned (every array needs 4-byte alignment)");
    return GGR_OK;
}
}  // namespace

size_t ggr_gru_conv_workspace_bytes(const GgrGruConvPass* cp) {
    (void)cp;
    return 0;       // the sum of an output element stays inside one wave: nothing passes through memory
}

int ggr_gru_conv_forward(const GgrGruConvPass* cp, void* stream) {
    g_err[0] = 0;
    ggr::GruConvArgs a;
    const int rc = gru_conv_pass_check(cp, &a);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ggr::launch_gru_conv(a, s);
    KCHECK(false, s, "gru_conv_forward");
    return GGR_OK;
}

// ---- the distortion pass (blend_dist.hip): the depth-distortion plane over a forward's lists, and its backward -----------------
namespace {
int distortion_pass_check(const GgrSettings* st, const GgrViews* views, const GgrDistortionPass* dp, bool backward, int* V) {
    if (!st || !dp) return fail(GGR_E_INVALID, "null settings / distortion pass");
    if (dp->struct_size < (int32_t)sizeof(GgrDistortionPass))
        return fail(GGR_E_INVALID, "GgrDistortionPass.struct_size %d is smaller than the %d bytes of its fields", (int)dp->struct_size,
                    (int)sizeof(GgrDistortionPass));
    if (dp->reserved != 0 || dp->reserved2 != 0)
        return fail(GGR_E_INVALID, "GgrDistortionPass.reserved must be 0, not %d / %d", (int)dp->reserved, (int)dp->reserved2);
    if (st->num_points < 0 || st->image_width < 0 || st->image_height < 0) return fail(GGR_E_INVALID, "negative size");
    if (!dp->out_distortion) return fail(GGR_E_INVALID, "GgrDistortionPass.out_distortion is NULL");
    if (!dp->geom_buffer || !dp->image_buffer) return fail(GGR_E_INVALID, "GgrDistortionPass: null geom / image buffer of the forward");
    if (dp->num_rendered != 0 && !dp->binning_buffer) return fail(GGR_E_INVALID, "GgrDistortionPass.binning_buffer is NULL");
    if (backward) {
        if (!dp->totals) return fail(GGR_E_INVALID, "GgrDistortionPass.totals is NULL");
        if (!dp->dL_dout_distortion) return fail(GGR_E_INVALID, "GgrDistortionPass.dL_dout_distortion is NULL");
        if (!dp->scratch) return fail(GGR_E_INVALID, "GgrDistortionPass.scratch is NULL");
    }
    *V = 1;
    if (views) {
        if (views->num_views < 1) return fail(GGR_E_INVALID, "GgrViews: num_views must be >= 1");
        const int sets = views->num_sets > 1 ? views->num_sets : 1;
        if (views->num_views % sets != 0) return fail(GGR_E_INVALID, "GgrViews: num_views must be a multiple of num_sets");
        if ((int64_t)views->num_views * st->num_points >= 0x7FFFFFFFll) return fail(GGR_E_LIMIT, "num_views x num_points too large");
        if ((int64_t)views->num_views * (int64_t)tiles_of(st->image_width, st->image_height) > (1 << 24))
            return fail(GGR_E_LIMIT, "more than 2^24 tiles over all views");
        *V = views->num_views;
    }
    return GGR_OK;
}
}  // namespace

int ggr_distortion_forward(const GgrSettings* st, const GgrViews* views, const GgrDistortionPass* dp, void* stream) {
    g_err[0] = 0;
    int V = 1;
    const int rc = distortion_pass_check(st, views, dp, false, &V);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int P1 = st->num_points, W = st->image_width, H = st->image_height;
    const size_t pixels = (size_t)V * (size_t)W * (size_t)H;
    if (pixels == 0) return GGR_OK;
    if (P1 == 0 || dp->num_rendered == 0) {   // no list entry anywhere: the plane and the totals are zero
        HIP_TRY(hipMemsetAsync(dp->out_distortion, 0, pixels * sizeof(float), s));
        if (dp->totals) HIP_TRY(hipMemsetAsync(dp->totals, 0, 2 * pixels * sizeof(float), s));
        return GGR_OK;
    }
    GeomLayout g = ggr_carve_geom((void*)dp->geom_buffer, (size_t)P1 * V, ggr_sort_segments((size_t)V), /*with_jac=*/false);
    ImageLayout im = ggr_carve_image((void*)dp->image_buffer, W, H, V);
    const bool scissored = (st->scissor[0] | st->scissor[1] | st->scissor[2] | st->scissor[3]) != 0;
    ggr::launch_blend_dist_fwd(W, H, im.ranges, (const uint32_t*)dp->binning_buffer, g.splat, dp->out_distortion, dp->totals, V,
                               scissored ? 1 : 0, s);
    KCHECK(st->debug != 0, s, "blend_dist_fwd");
    return GGR_OK;
}

int ggr_distortion_backward(const GgrSettings* st, const GgrViews* views, const GgrDistortionPass* dp, void* stream) {
    g_err[0] = 0;
    int V = 1;
    const int rc = distortion_pass_check(st, views, dp, true, &V);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int P1 = st->num_points, W = st->image_width, H = st->image_height;
    BwdScratch sc = ggr_carve_bwd(dp->scratch, (size_t)P1, (size_t)V);
    if (!dp->scratch_zeroed) HIP_TRY(hipMemsetAsync(dp->scratch, 0, sc.bytes, s));
    if (P1 == 0 || dp->num_rendered == 0 || (size_t)W * H == 0) return GGR_OK;
    GeomLayout g = ggr_carve_geom((void*)dp->geom_buffer, (size_t)P1 * V, ggr_sort_segments((size_t)V), /*with_jac=*/false);
    ImageLayout im = ggr_carve_image((void*)dp->image_buffer, W, H, V);
    ggr::launch_blend_dist_bwd(W, H, im.ranges, (const uint32_t*)dp->binning_buffer, g.splat, dp->out_distortion, dp->totals,
                               dp->dL_dout_distortion, sc.grad2d, V, s);
    KCHECK(st->debug != 0, s, "blend_dist_bwd");
    return GGR_OK;
}

// ---- the absgrad pass (blend_absgrad.hip): per-Gaussian absolute screen-space positional gradients over a forward's lists ------
int ggr_means2d_absgrad(const GgrSettings* st, const GgrViews* views, const GgrAbsgradPass* ap, void* stream) {
    g_err[0] = 0;
    if (!st || !ap) return fail(GGR_E_INVALID, "null settings / absgrad pass");
    if (ap->struct_size < (int32_t)sizeof(GgrAbsgradPass))
        return fail(GGR_E_INVALID, "GgrAbsgradPass.struct_size %d is smaller than the %d bytes of its fields", (int)ap->struct_size,
                    (int)sizeof(GgrAbsgradPass));
    if (ap->reserved != 0) return fail(GGR_E_INVALID, "GgrAbsgradPass.reserved must be 0, not %d", (int)ap->reserved);
    if (st->num_points < 0 || st->image_width < 0 || st->image_height < 0) return fail(GGR_E_INVALID, "negative size");
    const bool no_pixels = (size_t)st->image_width * (size_t)st->image_height == 0;   // (an empty frame has no planes)
    if (st->num_points > 0 && !ap->out_absgrad) return fail(GGR_E_INVALID, "GgrAbsgradPass.out_absgrad is NULL");
    if (!ap->geom_buffer || !ap->image_buffer) return fail(GGR_E_INVALID, "GgrAbsgradPass: null geom / image buffer of the forward");
    if (ap->num_rendered != 0 && !ap->binning_buffer) return fail(GGR_E_INVALID, "GgrAbsgradPass.binning_buffer is NULL");
    if (!no_pixels && !ap->out_color) return fail(GGR_E_INVALID, "GgrAbsgradPass.out_color is NULL");
    if (!no_pixels && !ap->dL_dout_color) return fail(GGR_E_INVALID, "GgrAbsgradPass.dL_dout_color is NULL");
    if (!no_pixels && ap->dL_dout_depth && !ap->out_depth) return fail(GGR_E_INVALID, "GgrAbsgradPass.out_depth is NULL but dL_dout_depth is given");
    int V = 1;
    if (views) {
        if (views->num_views < 1) return fail(GGR_E_INVALID, "GgrViews: num_views must be >= 1");
        const int sets = views->num_sets > 1 ? views->num_sets : 1;
        if (views->num_views % sets != 0) return fail(GGR_E_INVALID, "GgrViews: num_views must be a multiple of num_sets");
        if ((int64_t)views->num_views * st->num_points >= 0x7FFFFFFFll) return fail(GGR_E_LIMIT, "num_views x num_points too large");
        if ((int64_t)views->num_views * (int64_t)tiles_of(st->image_width, st->image_height) > (1 << 24))
            return fail(GGR_E_LIMIT, "more than 2^24 tiles over all views");
        V = views->num_views;
    }
    hipStream_t s = (hipStream_t)stream;
    const int P1 = st->num_points, W = st->image_width, H = st->image_height;
    const size_t rows = (size_t)V * (size_t)P1;
    if (rows == 0) return GGR_OK;
    HIP_TRY(hipMemsetAsync(ap->out_absgrad, 0, rows * 2 * sizeof(float), s));
    if (ap->out_grad) HIP_TRY(hipMemsetAsync(ap->out_grad, 0, rows * 2 * sizeof(float), s));
    if (ap->num_rendered == 0 || (size_t)W * H == 0) return GGR_OK;   // no list entry anywhere
    GeomLayout g = ggr_carve_geom((void*)ap->geom_buffer, rows, ggr_sort_segments((size_t)V), /*with_jac=*/false);
    ImageLayout im = ggr_carve_image((void*)ap->image_buffer, W, H, V);
    ggr::launch_blend_absgrad(W, H, im.ranges, (const uint32_t*)ap->binning_buffer, g.splat, g.colour, im.final_T, ap->out_color,
                              ap->out_depth, ap->dL_dout_color, ap->dL_dout_depth, ap->dL_dout_alpha, ap->out_absgrad,
                              ap->out_grad, V, s);
    KCHECK(st->debug != 0, s, "blend_absgrad");
    return GGR_OK;
}

size_t ggr_geom_bytes_inference(int32_t P, int32_t V) {
    const size_t v = (size_t)(V > 0 ? V : 1);
    return ggr_carve_geom(nullptr, (size_t)(P > 0 ? P : 0) * v, ggr_sort_segments(v), /*with_jac=*/false).bytes;
}
size_t ggr_image_bytes_inference(int32_t W, int32_t H, int32_t V) { return ggr_carve_image(nullptr, W, H, V > 0 ? V : 1).bytes_no_ckpt; }
size_t ggr_geom_bytes_views(int32_t P, int32_t V) {
    const size_t v = (size_t)(V > 0 ? V : 1);
    return ggr_carve_geom(nullptr, (size_t)(P > 0 ? P : 0) * v, ggr_sort_segments(v)).bytes;
}
size_t ggr_image_bytes_views(int32_t W, int32_t H, int32_t V) { return ggr_carve_image(nullptr, W, H, V > 0 ? V : 1).bytes; }
size_t ggr_work_bytes_views(int32_t P, int32_t W, int32_t H, int32_t V) {
    const size_t v = (size_t)(V > 0 ? V : 1);
    return ggr::plan_tile_lists((size_t)(P > 0 ? P : 0) * v, tiles_of(W, H) * v).work_bytes;
}
size_t ggr_backward_scratch_bytes_views(int32_t P, int32_t V) {
    return ggr_carve_bwd(nullptr, (size_t)(P > 0 ? P : 0), (size_t)(V > 0 ? V : 1)).bytes;
}

int ggr_camera_setup(int32_t n, const float* extrinsics, const float* intrinsics, const float* near, const float* far,
                     int32_t scale_invariant, float* viewmatrix, float* projmatrix, float* campos, float* tanfov,
                     float* scale, void* stream) {
    g_err[0] = 0;
    if (n < 0 || (n > 0 && (!extrinsics || !intrinsics || !near || !far || !viewmatrix || !projmatrix || !campos ||
                            !tanfov || !scale)))
        return fail(GGR_E_INVALID, "bad arguments");
    ggr::launch_camera_setup(n, extrinsics, intrinsics, near, far, scale_invariant, viewmatrix, projmatrix, campos,
                             tanfov, scale, (hipStream_t)stream);
    KCHECK(false, (hipStream_t)stream, "camera_setup");
    return GGR_OK;
}

int ggr_camera_setup_backward(int32_t n, const float* extrinsics, const float* intrinsics, const float* near, const float* far,
                              int32_t scale_invariant, const float* dL_dviewmatrix, const float* dL_dprojmatrix,
                              const float* dL_dcampos, const float* dL_dtanfov, float* dL_dextrinsics, float* dL_dintrinsics,
                              void* stream) {
    g_err[0] = 0;
    if (n < 0 || (n > 0 && (!extrinsics || !intrinsics || !near || !far || !dL_dviewmatrix || !dL_dprojmatrix || !dL_dcampos ||
                            !dL_dtanfov || !dL_dextrinsics || !dL_dintrinsics)))
        return fail(GGR_E_INVALID, "bad arguments");
    ggr::launch_camera_setup_bwd(n, extrinsics, intrinsics, near, far, scale_invariant, dL_dviewmatrix, dL_dprojmatrix,
                                 dL_dcampos, dL_dtanfov, dL_dextrinsics, dL_dintrinsics, (hipStream_t)stream);
    KCHECK(false, (hipStream_t)stream, "camera_setup_backward");
    return GGR_OK;
}

int ggr_sort_stats_async(const void* geom_buffer, int32_t P, uint32_t* host_words, void* stream) {
    g_err[0] = 0;
    if (!geom_buffer || !host_words) return fail(GGR_E_INVALID, "null geom buffer / destination");
    GeomLayout g = ggr_carve_geom((void*)geom_buffer, (size_t)(P > 0 ? P : 0));
    // (the counters' place in the buffer depends on P alone: whether the forward was an inference one does not matter)
    HIP_TRY(hipMemcpyAsync(host_words, g.counters, 16, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return GGR_OK;
}

int ggr_forward_status(const void* geom_buffer, int32_t P, int64_t* num_rendered, int32_t* overflow, void* stream) {
    g_err[0] = 0;
    if (!geom_buffer) return fail(GGR_E_INVALID, "null geom buffer");
    GeomLayout g = ggr_carve_geom((void*)geom_buffer, (size_t)(P > 0 ? P : 0));
    uint32_t host[2] = {0u, 0u};
    HIP_TRY(hipMemcpyAsync(host, g.counters, 8, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (num_rendered) *num_rendered = (int64_t)host[0];
    // (bit 3: a tile list too long for the per-tile depth sort in a forward that could not fall back — the frame is as
    //  incomplete as one whose lists were cut)
    if (overflow) *overflow = (int32_t)((host[1] & 1u) | ((host[1] >> 3) & 1u));
    if (host[1] & 2u) return fail(GGR_E_HIP, "%s", kSpinFault);
    if (host[1] & 4u) return fail(GGR_E_LIMIT, "%s", kRangeFault);
    return GGR_OK;
}

namespace {
struct FakeQuery { int scenario; int calls; volatile uint32_t* word; timespec t0; double late_s; };
hipError_t fake_query(void* p) {
    FakeQuery* q = (FakeQuery*)p;
    q->calls++;
    switch (q->scenario) {
        case 0: if (q->calls == 3) *q->word = 1234u; return hipErrorNotReady;
        case 1: return q->calls < 2 ? hipErrorNotReady : hipErrorLaunchFailure;
        case 2: return hipErrorNotReady;
        case 4: return hipErrorNotReady;   // (the word arrives through fake_start, below)
        default: return hipSuccess;
    }
}
// scenario 4: the stream is busy with EARLIER work for `late_s` seconds (longer than the time bound), then the
// tile-list kernels get their turn and the word arrives a few polls later — must succeed
hipError_t fake_start(void* p) {
    FakeQuery* q = (FakeQuery*)p;
    timespec t1;
    clock_gettime(CLOCK_MONOTONIC, &t1);
    const double dt = (double)(t1.tv_sec - q->t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - q->t0.tv_nsec);
    if (dt < q->late_s) return hipErrorNotReady;
    *q->word = 4321u;
    return hipSuccess;
}
}  // namespace

int ggr_debug_readback_wait(int32_t scenario, double timeout_s, uint32_t* value) {
    g_err[0] = 0;
    if (scenario < 0 || scenario > 4 || !value) return fail(GGR_E_INVALID, "bad arguments");
    volatile uint32_t word = GGR_READBACK_ARMED;
    FakeQuery q{scenario, 0, &word, {}, 3.0 * timeout_s};
    clock_gettime(CLOCK_MONOTONIC, &q.t0);
    if (scenario == 4) return wait_readback(&word, fake_query, &q, timeout_s, value, fake_start, &q);
    return wait_readback(&word, fake_query, &q, timeout_s, value);
}

int ggr_debug_counters(uint64_t* out, int32_t reset) {
    g_err[0] = 0;
    if (!out) return fail(GGR_E_INVALID, "null output");
    unsigned long long f[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
    HIP_TRY(hipDeviceSynchronize());
    ggr::blend_fwd_counters(f, reset);
    ggr::blend_bwd_counters(b, reset);
    for (int i = 0; i < 4; i++) { out[i] = f[i]; out[4 + i] = b[i]; }
#ifdef GGR_DEV_COUNTERS
    return GGR_OK;
#else
    return fail(GGR_E_INVALID, "this library was built without -DGGR_DEV_COUNTERS: the counters are zero");
#endif
}

int ggr_debug_host_slots(int32_t* readback_slots, int32_t* side_streams) {
    g_err[0] = 0;
    if (readback_slots) { SlotPool<ReadbackSlot>& p = SlotPool<ReadbackSlot>::get(); std::lock_guard<std::mutex> lk(p.mu); *readback_slots = p.created; }
    if (side_streams) { SlotPool<SideStream>& p = SlotPool<SideStream>::get(); std::lock_guard<std::mutex> lk(p.mu); *side_streams = p.created; }
    return GGR_OK;
}

int ggr_debug_copy(const void* src, void* dst, size_t bytes, int32_t blocks, void* stream) {
    g_err[0] = 0;
    if (!src || !dst || (bytes & 15) || (((uintptr_t)src | (uintptr_t)dst) & 15)) return fail(GGR_E_INVALID, "bad arguments (16-byte granularity)");
    ggr::launch_copy_f4(src, dst, bytes, blocks, (hipStream_t)stream);
    KCHECK(false, (hipStream_t)stream, "copy_f4");
    return GGR_OK;
}

int ggr_mark_visible(int32_t P, const float* means3D, const float* viewmatrix, const float*, uint8_t* present,
                     void* stream) {
    g_err[0] = 0;
    if (P < 0 || (P > 0 && (!means3D || !viewmatrix || !present))) return fail(GGR_E_INVALID, "bad arguments");
    ggr::launch_mark_visible(P, means3D, viewmatrix, present, (hipStream_t)stream);
    KCHECK(false, (hipStream_t)stream, "mark_visible");
    return GGR_OK;
}

int ggr_debug_unpack_geom(const void* geom_buffer, int32_t P, float* depth, float* xy, float* conic_opacity,
                          float* rgb, int32_t* tiles_touched, uint8_t* clamped, void* stream) {
    g_err[0] = 0;
    if (!geom_buffer) return fail(GGR_E_INVALID, "null geom buffer");
    GeomLayout g = ggr_carve_geom((void*)geom_buffer, (size_t)(P > 0 ? P : 0));
    ggr::launch_unpack_geom(g, P, depth, xy, conic_opacity, rgb, tiles_touched, clamped, (hipStream_t)stream);
    KCHECK(false, (hipStream_t)stream, "unpack_geom");
    return GGR_OK;
}

int ggr_debug_unpack_binning(const void* binning_buffer, const void* image_buffer, int64_t N, int32_t W, int32_t H,
                             uint32_t* point_list, int32_t* ranges, float* final_T, int32_t* n_contrib, void* stream) {
    g_err[0] = 0;
    hipStream_t s = (hipStream_t)stream;
    if (!image_buffer) return fail(GGR_E_INVALID, "null image buffer");
    ImageLayout im = ggr_carve_image((void*)image_buffer, W, H);
    const size_t tiles = tiles_of(W, H);
    if (point_list && N > 0) {
        if (!binning_buffer) return fail(GGR_E_INVALID, "null binning buffer");
        HIP_TRY(hipMemcpyAsync(point_list, binning_buffer, (size_t)N * 4, hipMemcpyDeviceToDevice, s));
    }
    if (ranges && tiles) HIP_TRY(hipMemcpyAsync(ranges, im.ranges, tiles * 8, hipMemcpyDeviceToDevice, s));
    if (final_T) HIP_TRY(hipMemcpyAsync(final_T, im.final_T, (size_t)W * H * 4, hipMemcpyDeviceToDevice, s));
    if (n_contrib) HIP_TRY(hipMemcpyAsync(n_contrib, im.n_contrib, (size_t)W * H * 4, hipMemcpyDeviceToDevice, s));
    return GGR_OK;
}

}  // extern "C"
