// ubench_split.hip -- the split kernel of csrc/columns.hip against the form it replaced and against a copy, on one box.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include -o build/ubench_split tools/ubench_split.hip
//   build/ubench_split [records = 33554432] [rounds = 30]
//
// n records of 24 bytes in HBM, three variants run in rotation (a round runs each once, the order rotates), each timed by a
// pair of events around it, the median over the rounds reported:
//   staged   k_col_split as the library launches it (a tile through LDS, 16-byte loads, whole lines out)
//   direct   k_col_split_direct below: a thread per record, three 8-byte loads 24 bytes apart, three 8-byte stores
//   copy     hipMemcpyAsync device to device of the same 24 n bytes (reads and writes what the split does)
// once with everything 16-byte aligned and once with the records and every column at 8 mod 16.  Both kernels' columns are
// compared with the expected values on the host before anything is timed.  One JSON line per alignment on stdout.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../ahocorasick_rs_amd/csrc/columns.hip"

#define CHECK(expr)                                                                                   \
    do {                                                                                              \
        hipError_t e__ = (expr);                                                                      \
        if (e__ != hipSuccess) {                                                                      \
            std::fprintf(stderr, "%s: %s (line %d)\n", #expr, hipGetErrorString(e__), __LINE__);      \
            return 1;                                                                                 \
        }                                                                                             \
    } while (0)

constexpr uint32_t DIRECT_THREADS = 256, DIRECT_MAX_GRID = 16384;

__global__ __launch_bounds__(DIRECT_THREADS) void k_col_split_direct(const uint64_t *__restrict__ w, uint64_t n,
                                                                     uint64_t *__restrict__ pattern, uint64_t *__restrict__ start,
                                                                     uint64_t *__restrict__ end) {
    const uint64_t stride = (uint64_t)gridDim.x * DIRECT_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * DIRECT_THREADS + threadIdx.x; i < n; i += stride) {
        const uint64_t p = w[3 * i], s = w[3 * i + 1], e = w[3 * i + 2];
        pattern[i] = p; start[i] = s; end[i] = e;
    }
}

__global__ void k_fill(uint64_t *w, uint64_t n) { // record i = (3 i, 3 i + 1 + 2^40, 3 i + 2 + 2^41)
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        w[3 * i] = 3 * i; w[3 * i + 1] = 3 * i + 1 + (1ull << 40); w[3 * i + 2] = 3 * i + 2 + (1ull << 41);
    }
}

static double median(std::vector<float> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

int main(int argc, char **argv) {
    const uint64_t n = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : (1ull << 25);
    const int rounds = argc > 2 ? std::atoi(argv[2]) : 30;
    if (!n || rounds < 1) { std::fprintf(stderr, "usage: ubench_split [records] [rounds]\n"); return 2; }
    uint64_t *rec = nullptr, *cols = nullptr;
    CHECK(hipMalloc((void **)&rec, (3 * n + 2) * 8));
    CHECK(hipMalloc((void **)&cols, (3 * (n + 2) + 2) * 8));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    for (int odd = 0; odd < 2; odd++) {
        uint64_t *w = rec + odd, *c0 = cols + odd, *c1 = c0 + n + 2, *c2 = c1 + n + 2; // (n + 2: an even step keeps the residue)
        hipLaunchKernelGGL(k_fill, dim3(4096), dim3(256), 0, nullptr, w, n);
        CHECK(hipGetLastError());
        auto staged = [&]() { return acx::col_split((const acx_match_t *)w, n, (int64_t *)c0, (int64_t *)c1, (int64_t *)c2, nullptr); };
        auto direct = [&]() {
            const uint32_t grid = (uint32_t)std::min<uint64_t>((n + DIRECT_THREADS - 1) / DIRECT_THREADS, DIRECT_MAX_GRID);
            hipLaunchKernelGGL(k_col_split_direct, dim3(grid), dim3(DIRECT_THREADS), 0, nullptr, w, n, c0, c1, c2);
            return hipGetLastError();
        };
        auto copy = [&]() { return hipMemcpyAsync(c0, w, 24 * n, hipMemcpyDeviceToDevice, nullptr); };
        // both kernels' output is right before it is timed: the first and the last 2^20 rows of every column
        const uint64_t chk = std::min<uint64_t>(n, 1ull << 20);
        std::vector<uint64_t> h(chk);
        for (int form = 0; form < 2; form++) {
            CHECK(hipMemset(cols, 0xEE, (3 * (n + 2) + 2) * 8));
            CHECK(form ? direct() : staged());
            CHECK(hipDeviceSynchronize());
            for (int k = 0; k < 3; k++)
                for (int tail = 0; tail < 2; tail++) {
                    const uint64_t at = tail ? n - chk : 0;
                    CHECK(hipMemcpy(h.data(), (k == 0 ? c0 : k == 1 ? c1 : c2) + at, chk * 8, hipMemcpyDeviceToHost));
                    for (uint64_t i = 0; i < chk; i++)
                        if (h[i] != 3 * (at + i) + k + (k ? (1ull << (39 + k)) : 0)) {
                            std::fprintf(stderr, "%s: column %d row %llu is wrong\n", form ? "direct" : "staged", k,
                                         (unsigned long long)(at + i));
                            return 1;
                        }
                }
        }
        std::vector<float> t[3];
        for (int r = -3; r < rounds; r++) // (three untimed rounds first)
            for (int j = 0; j < 3; j++) {
                const int v = (j + (r + 3)) % 3;
                CHECK(hipEventRecord(e0, nullptr));
                CHECK(v == 0 ? staged() : v == 1 ? direct() : copy());
                CHECK(hipEventRecord(e1, nullptr));
                CHECK(hipEventSynchronize(e1));
                float ms = 0;
                CHECK(hipEventElapsedTime(&ms, e0, e1));
                if (r >= 0) t[v].push_back(ms);
            }
        const double gb = 48.0 * n / 1e9; // read + written
        std::printf("{\"part\": \"pair\", \"records\": %llu, \"rounds\": %d, \"alignment\": \"%s\", \"ms\": {\"staged\": %.4f, "
                    "\"direct\": %.4f, \"copy\": %.4f}, \"min_ms\": {\"staged\": %.4f, \"direct\": %.4f, \"copy\": %.4f}, "
                    "\"gb_per_s\": {\"staged\": %.1f, \"direct\": %.1f, \"copy\": %.1f}}\n",
                    (unsigned long long)n, rounds, odd ? "8 mod 16" : "0 mod 16", median(t[0]), median(t[1]), median(t[2]),
                    *std::min_element(t[0].begin(), t[0].end()), *std::min_element(t[1].begin(), t[1].end()),
                    *std::min_element(t[2].begin(), t[2].end()), gb / median(t[0]) * 1e3, gb / median(t[1]) * 1e3,
                    gb / median(t[2]) * 1e3);
        std::fflush(stdout);
    }
    CHECK(hipFree(rec));
    CHECK(hipFree(cols));
    return 0;
}
