// host_common.hpp -- what every unit of the host layer (the C ABI of include/acx.h and the code behind it) shares: the
// thread's error message, the HIP error check, the device scope, the one polling loop, the host trace.
// The host layer's own names live in namespace acxh, which is hidden: libacx_hip.so exports the acx_* entry points only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#if defined(__x86_64__)
#include <immintrin.h>
#endif

#include "../../include/acx.h"
#include "automaton.hpp"
#include "kernels.hpp"

#define ACX_HIDDEN __attribute__((visibility("hidden")))

namespace acxh ACX_HIDDEN {
using namespace acx;

inline thread_local std::string g_err;
inline thread_local int g_device = -1; // -1: use the current HIP device

inline int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
// The device's occurrence indexes are 32 bits wide: a call that would enumerate more is cut into byte ranges (run_chunked).
// The limit of ONE pass (ACX_MAX_OCC lowers it: tests) and what a pass returns when it hits it -- run_find's business,
// never the caller's.
constexpr int TOO_MANY_OCC = -1006;
inline uint64_t occ_limit() {
    const char *e = std::getenv("ACX_MAX_OCC");
    const uint64_t hard = (1ull << 32) - 2;
    if (!e) return hard;
    const uint64_t v = std::strtoull(e, nullptr, 10);
    return v && v < hard ? v : hard;
}
inline int fail_occ() { return fail(TOO_MANY_OCC, "more than 2^32 occurrences in one pass"); }
inline int hipfail(hipError_t e, const char *what) {
    (void)hipGetLastError(); // the runtime's "last error" is sticky: the next launch check must not see this one
    return fail(e == hipErrorOutOfMemory ? ACX_ENOMEM : ACX_EDEVICE, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIPCHK(expr)                                   \
    do {                                               \
        hipError_t e__ = (expr);                       \
        if (e__ != hipSuccess) return hipfail(e__, #expr); \
    } while (0)

inline void cpu_relax() {
#if defined(__x86_64__)
    _mm_pause();
#endif
}

// The one polling loop of the host layer: spins on `done` (cpu_relax between two looks), looks at the steady clock every
// clock_mask + 1 spins (a power of two), and once `deadline` has passed runs `fallback` -- a blocking synchronisation, as
// a rule: its wake-up costs 10-20 us, a poll costs one PCIe round trip -- and looks one last time.  Returns whether `done` held.
template <typename Done, typename Fallback>
inline bool poll_until(Done &&done, uint32_t clock_mask, std::chrono::milliseconds deadline, Fallback &&fallback) {
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spins = 0; !done(); spins++) {
        cpu_relax();
        if ((spins & clock_mask) == clock_mask && std::chrono::steady_clock::now() - t0 > deadline) {
            fallback();
            return done();
        }
    }
    return true;
}

// makes `dev` the calling thread's HIP device for a scope and restores the previous one
struct DeviceScope {
    int prev = -1;
    bool changed = false;
    explicit DeviceScope(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) changed = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceScope() {
        if (changed && prev >= 0) (void)hipSetDevice(prev);
    }
};

// ACX_HOST_TRACE=1 (measurements): where the host's microseconds go, the mean of every interval printed when the process
// ends.  mark(): steady-clock stamps at ten points of a device-resident call, acx_find_device .. acx_free_result;
// begin() / lap(): the host-memory entry point acx_find beyond K0's sizes (copy in, pipeline, copy out).
struct HostTrace {
    static constexpr int N = 10;
    bool on = std::getenv("ACX_HOST_TRACE") != nullptr;
    int64_t t[N] = {}, sum[N] = {};
    uint64_t rounds = 0;
    int64_t f_t0 = 0, f_sum[4] = {};
    uint64_t f_rounds = 0;
    static int64_t now() { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    void mark(int i) {
        if (!on) return;
        const int64_t v = now();
        if (i == 0 && t[N - 1]) sum[0] += v - t[N - 1]; // (from the end of the last round: the caller's own time)
        if (i > 0 && t[i - 1]) sum[i] += v - t[i - 1];
        t[i] = v;
        if (i == N - 1) rounds++;
    }
    void begin() { if (on) f_t0 = now(); }
    void lap(int i) { if (!on) return; const int64_t v = now(); f_sum[i] += v - f_t0; f_t0 = v; if (i == 3) f_rounds++; }
    ~HostTrace() {
        if (on && f_rounds) {
            static const char *what[4] = {"stage (host -> device copy queued)", "pipeline until the totals are known", "wait + device -> host copy", "free"};
            std::fprintf(stderr, "ACX_HOST_TRACE acx_find: %llu rounds, mean microseconds\n", (unsigned long long)f_rounds);
            for (int i = 0; i < 4; i++) std::fprintf(stderr, "  %-40s %8.2f\n", what[i], f_sum[i] / 1e3 / f_rounds);
        }
        if (on && rounds) {
            static const char *what[N] = {"caller (free .. next call)", "lease", "up to the scan's launch", "the scan's launch", "the post kernels' launches",
                                          "events up to the wait", "wait for the totals' line", "return", "caller (return .. free)", "free"};
            std::fprintf(stderr, "ACX_HOST_TRACE: %llu rounds, mean microseconds per interval\n", (unsigned long long)rounds);
            for (int i = 0; i < N; i++) std::fprintf(stderr, "  %-32s %8.2f\n", what[i], sum[i] / 1e3 / rounds);
        }
    }
};
inline HostTrace g_trace;

} // namespace acxh
