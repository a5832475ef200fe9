// ubench_snippets.hip -- the short-segment gather of csrc/snippets.hip against the row gather of csrc/filter.hip fed the same
// offsets and sources, and against a copy of the output's bytes, on one box.  Both launchers are linked directly: there is
// no switch.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include -o build/ubench_snippets tools/ubench_snippets.hip
//   build/ubench_snippets [haystack bytes = 1073741824] [rounds = 20]
//
// The shape is the snippet stage's on cfg2's batch: rows of 8 KiB, a match of 5 .. 12 bytes every 256, 64 and 32 bytes, a
// context of 0, 32 and 128 bytes on each side clipped to the row -- nine shapes.  The segments (offsets, src) are made on the
// host by the definition.  Three variants run in rotation (a round runs each once, the order rotates), each timed by a pair of
// events around it, the median over the rounds reported:
//   snip     acx::snip_gather as the library launches it (k_snip_tiles + k_snip_gather)
//   filter   acx::filter_gather (k_filter_tiles + k_filter_gather): a correct ragged gather, built for rows of kilobytes
//   copy     hipMemcpyAsync device to device of the output's bytes (into a second buffer of that size)
// Both kernels' outputs are compared with the expected bytes on the host (the first and the last 4 MiB) before anything is
// timed.  One JSON line per shape on stdout.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../ahocorasick_rs_amd/csrc/filter.hip"
#include "../ahocorasick_rs_amd/csrc/snippets.hip"

#define CHECK(expr)                                                                                   \
    do {                                                                                              \
        hipError_t e__ = (expr);                                                                      \
        if (e__ != hipSuccess) {                                                                      \
            std::fprintf(stderr, "%s: %s (line %d)\n", #expr, hipGetErrorString(e__), __LINE__);      \
            return 1;                                                                                 \
        }                                                                                             \
    } while (0)

constexpr uint64_t ROW = 8192;

__host__ __device__ inline uint8_t hay_byte(uint64_t i) { return (uint8_t)(((i * 0x9E3779B97F4A7C15ull) >> 29) % 251); }

__global__ void k_fill(uint8_t *hay, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) hay[i] = hay_byte(i);
}

static double median(std::vector<float> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

int main(int argc, char **argv) {
    const uint64_t len = (argc > 1 ? std::strtoull(argv[1], nullptr, 10) : (1ull << 30)) / ROW * ROW;
    const int rounds = argc > 2 ? std::atoi(argv[2]) : 20;
    if (!len || rounds < 1) { std::fprintf(stderr, "usage: ubench_snippets [haystack bytes] [rounds]\n"); return 2; }
    uint8_t *hay = nullptr;
    CHECK(hipMalloc((void **)&hay, len));
    hipLaunchKernelGGL(k_fill, dim3(8192), dim3(256), 0, nullptr, hay, len);
    CHECK(hipGetLastError());
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    for (const uint64_t every : {256ull, 64ull, 32ull})
        for (const uint64_t context : {0ull, 32ull, 128ull}) {
            const uint64_t n = len / every;
            std::vector<int64_t> off(n + 1);
            std::vector<uint64_t> src(n);
            uint64_t total = 0;
            for (uint64_t i = 0; i < n; i++) { // the definition: the match at s .. e of its row, `context` on each side, clipped
                const uint64_t at = i * every, rb = at / ROW * ROW, s = at - rb, e = std::min(s + 5 + (i * 7) % 8, ROW);
                const uint64_t lo = s - std::min(s, context), hi = e + std::min(context, ROW - e);
                off[i] = (int64_t)total;
                src[i] = rb + lo;
                total += hi - lo;
            }
            off[n] = (int64_t)total;
            int64_t *d_off = nullptr;
            uint64_t *d_src = nullptr, *d_tiles = nullptr;
            uint8_t *out = nullptr, *out2 = nullptr;
            const uint64_t tile_words = std::max(acx::snip_tile_words(total), acx::filter_tile_words(total));
            CHECK(hipMalloc((void **)&d_off, (n + 1) * 8));
            CHECK(hipMalloc((void **)&d_src, n * 8));
            CHECK(hipMalloc((void **)&d_tiles, tile_words * 8));
            CHECK(hipMalloc((void **)&out, total + 32));
            CHECK(hipMalloc((void **)&out2, total + 32));
            CHECK(hipMemcpy(d_off, off.data(), (n + 1) * 8, hipMemcpyHostToDevice));
            CHECK(hipMemcpy(d_src, src.data(), n * 8, hipMemcpyHostToDevice));
            auto snip = [&]() { return acx::snip_gather(hay, len, d_off, d_src, n, d_tiles, out, total, nullptr); };
            auto filter = [&]() { return acx::filter_gather(hay, len, d_off, d_src, n, d_tiles, out, total, nullptr); };
            auto copy = [&]() { return hipMemcpyAsync(out2, out, total, hipMemcpyDeviceToDevice, nullptr); };
            // both kernels' output is right before it is timed: the first and the last 4 MiB
            const uint64_t chk = std::min<uint64_t>(total, 4ull << 20);
            std::vector<uint8_t> h(chk);
            for (int form = 0; form < 2; form++) {
                CHECK(hipMemset(out, 0xEE, total + 32));
                CHECK(form ? filter() : snip());
                CHECK(hipDeviceSynchronize());
                for (int tail = 0; tail < 2; tail++) {
                    const uint64_t at = tail ? total - chk : 0;
                    CHECK(hipMemcpy(h.data(), out + at, chk, hipMemcpyDeviceToHost));
                    uint64_t seg = (uint64_t)(std::upper_bound(off.begin(), off.end(), (int64_t)at) - off.begin()) - 1;
                    for (uint64_t x = at; x < at + chk; x++) {
                        while ((uint64_t)off[seg + 1] <= x) seg++;
                        if (h[x - at] != hay_byte(src[seg] + (x - (uint64_t)off[seg]))) {
                            std::fprintf(stderr, "%s: every %llu, context %llu: output byte %llu is wrong\n", form ? "filter" : "snip",
                                         (unsigned long long)every, (unsigned long long)context, (unsigned long long)x);
                            return 1;
                        }
                    }
                }
                if (!form) { // nothing behind the total
                    uint8_t behind[16];
                    CHECK(hipMemcpy(behind, out + total, 16, hipMemcpyDeviceToHost));
                    for (int k = 0; k < 16; k++)
                        if (behind[k] != 0xEE) { std::fprintf(stderr, "snip: a byte behind the total was written\n"); return 1; }
                }
            }
            std::vector<float> t[3];
            for (int r = -3; r < rounds; r++) // (three untimed rounds first)
                for (int j = 0; j < 3; j++) {
                    const int v = (j + (r + 3)) % 3;
                    CHECK(hipEventRecord(e0, nullptr));
                    CHECK(v == 0 ? snip() : v == 1 ? filter() : copy());
                    CHECK(hipEventRecord(e1, nullptr));
                    CHECK(hipEventSynchronize(e1));
                    float ms = 0;
                    CHECK(hipEventElapsedTime(&ms, e0, e1));
                    if (r >= 0) t[v].push_back(ms);
                }
            const double gb = 2.0 * total / 1e9; // read + written
            std::printf("{\"part\": \"gather\", \"haystack_bytes\": %llu, \"planted_every\": %llu, \"context\": %llu, \"segments\": %llu, "
                        "\"output_bytes\": %llu, \"rounds\": %d, \"ms\": {\"snip\": %.4f, \"filter\": %.4f, \"copy\": %.4f}, "
                        "\"min_ms\": {\"snip\": %.4f, \"filter\": %.4f, \"copy\": %.4f}, \"gb_per_s\": {\"snip\": %.1f, \"filter\": %.1f}, "
                        "\"snip_vs_filter\": %.3f}\n",
                        (unsigned long long)len, (unsigned long long)every, (unsigned long long)context, (unsigned long long)n,
                        (unsigned long long)total, rounds, median(t[0]), median(t[1]), median(t[2]),
                        *std::min_element(t[0].begin(), t[0].end()), *std::min_element(t[1].begin(), t[1].end()),
                        *std::min_element(t[2].begin(), t[2].end()), gb / median(t[0]) * 1e3, gb / median(t[1]) * 1e3,
                        median(t[0]) / median(t[1]));
            std::fflush(stdout);
            CHECK(hipFree(d_off));
            CHECK(hipFree(d_src));
            CHECK(hipFree(d_tiles));
            CHECK(hipFree(out));
            CHECK(hipFree(out2));
        }
    CHECK(hipFree(hay));
    return 0;
}
