// common.h -- error plumbing shared by the HIP translation units of libeaofusion_hip.so
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/eao_fusion.h"
#include "ref_constants.inc"   // GENERATED from the reference text (tools/gen_ref_constants.py): namespace refc

namespace eao {

void set_error(const char* fmt, ...);

#define EAO_HIP(call)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (call);                                                                         \
        if (e_ != hipSuccess) {                                                                         \
            eao::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return EAO_ERR_NO_DEVICE;                                                                   \
        }                                                                                               \
    } while (0)

#define EAO_REQUIRE(cond, ...)           \
    do {                                 \
        if (!(cond)) {                   \
            eao::set_error(__VA_ARGS__); \
            return EAO_ERR_INVALID;      \
        }                                \
    } while (0)

// Fails loudly (EAO_ERR_NO_DEVICE) when no HIP device can run gfx950 code objects.  There is no CPU fallback.
eao_status require_device();

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    // grow-only allocation
    eao_status reserve(size_t count) {
        if (count <= n) return EAO_OK;
        release();
        EAO_HIP(hipMalloc((void**)&p, count * sizeof(T)));
        n = count;
        return EAO_OK;
    }
};

// Grow-only pinned host buffer.  With hipHostMallocMapped it is device-visible (kernels read and write it in place) and d is its device address; with
// hipHostMallocDefault it stages asynchronous copies and d stays null.
template <unsigned kFlags>
struct PinBuf {
    unsigned char* p = nullptr;
    unsigned char* d = nullptr;
    size_t n = 0;
    eao_status reserve(size_t need) {
        if (need <= n) return EAO_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr; d = nullptr; n = 0;
        const size_t cap = need + (need >> 2) + 4096;
        EAO_HIP(hipHostMalloc((void**)&p, cap, kFlags));
        if (kFlags & hipHostMallocMapped) EAO_HIP(hipHostGetDevicePointer((void**)&d, p, 0));
        n = cap;
        return EAO_OK;
    }
    ~PinBuf() { if (p) (void)hipHostFree(p); }
};

inline int cdiv(int a, int b) { return (a + b - 1) / b; }
// every slice of a device arena / staging block starts on a 256-byte boundary
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// Stream classes (round 6).  Upstream runs three threads at once on ONE device -- Tracking (per frame, real time), LocalMapping
// (LocalBundleAdjustment, src/LocalMapping.cc:75) and LoopClosing's global BundleAdjustment thread (src/LoopClosing.cc:594; all started
// in src/System.cc:98-138) -- so every stream the library creates says which of them it serves, and the HIP stream priority follows:
//   Latency    -- extractor handles, the tracked-frame chain, PoseOptimization, the guided searches (a frame waits for each of them),
//   Background -- LocalBundleAdjustment (one window and batches),
//   Bulk       -- map-scale BundleAdjustment.
// A priority class also has its own pool of hardware queues in the runtime, so a tracker stream no longer shares a queue with an LM
// stream (beyond four streams of one class they do share: measured in round 2 on the batch groups).  EAO_STREAM_PRIORITY=0: every
// stream at the default priority (the rounds 1-5 behaviour, for A/B runs).
enum class StreamClass { Latency = 0, Background = 1, Bulk = 2 };
hipError_t create_stream(hipStream_t* s, StreamClass c);
// The host's wait for a Latency-class stream: hipStreamSynchronize parks the thread on an interrupt, whose wake-up costs tens of microseconds and now and then
// milliseconds (tests/cpp/mixed_load.cpp: the 7-10 ms maxima of the tracked frame beside a looping bundle adjustment disappear under HSA_ENABLE_INTERRUPT=0).  A frame
// waits for each of these calls, so the caller's thread polls hipStreamQuery for up to 3 ms first (a Tracking thread has nothing else to do meanwhile; upstream's
// computes the features on that core) and only then blocks.  EAO_SPIN_WAIT=0: always block.
hipError_t wait_latency(hipStream_t s);
// A latency-class call is in progress / was made moments ago (stamped by wait_latency and by the tracked-frame chain's poll): eao_local_ba_batch deals its windows to TWO
// stream groups instead of four while a frame-rate caller is alive in the process.  Measured (tests/cpp/mixed_load.cpp, gpurun_out/r06n): four groups keep every CU's
// register file occupied without a gap, and the tracker's full-register-file workgroups wait for the batch's whole busy period (tracked frame p50 1.65 / p99 3.2 ms against
// 0.77 idle); with two groups 1.08 / 1.64 ms, the batch 2.87 -> 3.13 ms per call.  No latency-class call within the last 100 ms: four groups, as in the benchmark.
void note_latency_call();
bool latency_caller_alive();

// One host thread's stream (a member of the thread_local context of an entry point) and, on request, a pair of timing events.  ready() is the first thing a
// call does; nothing is taken for ready that was not created (a call after a failed one starts over), and whatever was created goes with the thread.
struct ThreadStream {
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    ThreadStream() = default;
    ThreadStream(const ThreadStream&) = delete;
    ThreadStream& operator=(const ThreadStream&) = delete;
    eao_status ready(StreamClass c) {
        eao_status st = require_device();
        if (st) return st;
        if (!stream) EAO_HIP(create_stream(&stream, c));
        return EAO_OK;
    }
    eao_status timing() {
        if (!ev0) EAO_HIP(hipEventCreate(&ev0));
        if (!ev1) EAO_HIP(hipEventCreate(&ev1));
        return EAO_OK;
    }
    ~ThreadStream() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// The end of a call on a thread's stream.  Whatever a call enqueues reads and writes the thread's staging block and device arena, and the next call on the thread
// rewrites both: nothing returns before the stream is empty.  Constructed right before the call's first enqueue (upload, memset or launch) and alive to the end of the
// call, so every EAO_HIP / EAO_REQUIRE return in between drains the stream on its way out (result ignored: the call already has its error).  wait() is the call's
// final wait and disarms; a call that waits mid-way and enqueues again uses wait_more(), which leaves the guard armed; disarm() is for the one call that sees the end
// of its last kernel without a stream wait (the done word of keyframe.hip).  The kind of each wait is the site's own choice: Latency polls first and stamps the
// process-wide latency marker (wait_latency above), Block is a plain hipStreamSynchronize.
struct Drain {
    enum Kind { Latency, Block };
    explicit Drain(hipStream_t s) : stream(s) {}
    Drain(const Drain&) = delete; Drain& operator=(const Drain&) = delete;
    ~Drain() { if (armed) (void)hipStreamSynchronize(stream); }
    hipError_t wait_more(Kind k) { return k == Latency ? wait_latency(stream) : hipStreamSynchronize(stream); }
    hipError_t wait(Kind k) { armed = false; return wait_more(k); }
    void disarm() { armed = false; }
private:
    hipStream_t stream;
    bool armed = true;
};

// Times each of the N kernels of this thread's last call (a diagnostic of the bench tools): N+1 marks around the launches, read() after the call.  A diagnostic cannot
// fail a product call: when an event call fails, that measurement is lost and the sticky error is cleared, so that the call's own hipGetLastError() does not take it
// for a launch error.  Results stay until the next arm(); a slot whose two marks were not both recorded in a call keeps what it had (-1: not measured).
template <int N>
struct KernelClock {
    KernelClock() { arm(false); }
    KernelClock(const KernelClock&) = delete; KernelClock& operator=(const KernelClock&) = delete;
    ~KernelClock() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    bool armed() const { return on; }
    void arm(bool v) { on = v; marked = 0; for (float& m : ms) m = -1.f; }
    // mark k goes before kernel k and after kernel k - 1
    void mark(int k, hipStream_t s) {
        if (!on) return;
        if ((ev[k] || hipEventCreate(&ev[k]) == hipSuccess) && hipEventRecord(ev[k], s) == hipSuccess) marked |= 1u << k;
        else (void)hipGetLastError();
    }
    // after the call's wait: this call's marks become milliseconds
    void collect() {
        for (int k = 0; k < N; k++)
            if ((marked >> k & 3u) == 3u && hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]) != hipSuccess) {
                ms[k] = -1.f;
                (void)hipGetLastError();
            }
        marked = 0;
    }
    // EAO_ERR_INVALID with the module's message when no slot is measured; -1 in a slot that is not
    eao_status read(float* out, const char* nothing) const {
        bool any = false;
        for (float m : ms) any = any || m >= 0.f;
        EAO_REQUIRE(any, "%s", nothing);
        for (int k = 0; k < N; k++) out[k] = ms[k];
        return EAO_OK;
    }
private:
    hipEvent_t ev[N + 1] = {};
    float ms[N];
    unsigned marked = 0;
    bool on = false;
};

#if defined(__HIPCC__)
// THE hand-over point between the lanes of ONE wavefront through LDS (or through memory the wave alone touches): the
// lanes' earlier stores are visible to the other lanes' later loads.  The hardware needs nothing for that -- a wave's
// LDS / memory instructions execute in order -- so a wavefront-scope fence lowers to NO instruction; what has to be
// stopped is the COMPILER: round 4 found the scheduler moving LDS reads above writes across a bare fence when the two
// sides used different access types (8-byte pairs in, 16-byte rows out: no alias in its view).  Hence: memory clobber +
// fence + wave_barrier (a scheduling barrier) + memory clobber.  Every such point in csrc/ goes through this one
// function (VERDICT r4 next #7a); the ISA of the kernels is unchanged by it (tools/isa_census.py, profiles/r05_wave_sync_isa.txt).
__device__ __forceinline__ void wave_sync() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}
#endif

// roctx range around a stage of the hot path (host side: the enqueue of its kernels); active only under EAO_ROCTX=1
void range_push(const char* name);
void range_pop();
struct Range {
    explicit Range(const char* name) { range_push(name); }
    ~Range() { range_pop(); }
    Range(const Range&) = delete;
    Range& operator=(const Range&) = delete;
};

}  // namespace eao
