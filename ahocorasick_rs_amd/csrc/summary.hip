// summary.hip -- the reduction kernels behind acx_summarize / acx_summarize_device (summary.hpp says what each computes).
// The find pipeline (kernels.hip) is not touched: these kernels read the records its write kernel left in HBM, and the
// exclusive prefix of the per-haystack counts comes from replace.hip's scan.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "summary.hpp"

namespace acx {

// ---------------------------------------------------------------------------
// 1. per haystack: its first record and its bit of the `any` bitmap.  A thread per haystack; a wave's 64 haystacks are
//    one word of the bitmap: the ballot of "has a record", stored by lane 0 (an ordinary vector store).  The lanes of the
//    tail wave that lie beyond n_hay vote 0, and a wave that lies beyond it altogether stores nothing: the words written
//    are exactly (n_hay + 63) / 64.
// ---------------------------------------------------------------------------
constexpr uint32_t SG_THREADS = 256;

__global__ __launch_bounds__(SG_THREADS) void k_sum_gather(const acx_match_t *__restrict__ m, uint64_t n,
                                                           const int64_t *__restrict__ prefix, uint64_t n_hay,
                                                           acx_match_t *__restrict__ first, uint64_t *__restrict__ any) {
    const uint64_t h = (uint64_t)blockIdx.x * SG_THREADS + threadIdx.x;
    bool has = false;
    if (h < n_hay) {
        const uint64_t b = prefix ? (uint64_t)prefix[h] : 0, e = prefix ? (uint64_t)prefix[h + 1] : n;
        has = e > b && b < n;
        // (three 8-byte fields in registers: a record held as a struct across the branch is spilled to LDS by the compiler)
        uint64_t pattern = UINT64_MAX, start = 0, end = 0;
        if (has) {
            const uint64_t *src = reinterpret_cast<const uint64_t *>(m + b);
            pattern = src[0]; start = src[1]; end = src[2];
        }
        uint64_t *dst = reinterpret_cast<uint64_t *>(first + h);
        dst[0] = pattern; dst[1] = start; dst[2] = end;
    }
    const uint64_t word = __ballot(has);
    if ((threadIdx.x & 63) == 0 && h < n_hay) any[h >> 6] = word;
}

hipError_t summary_gather(const acx_match_t *m, uint64_t n, const int64_t *prefix, uint64_t n_hay, acx_match_t *first,
                          uint64_t *any, hipStream_t st) {
    if (!n_hay) return hipSuccess;
    const uint64_t nwg = (n_hay + SG_THREADS - 1) / SG_THREADS;
    if (nwg > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sum_gather, dim3((uint32_t)nwg), dim3(SG_THREADS), 0, st, m, n, prefix, n_hay, first, any);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// 2. per pattern: the histogram of m[i].pattern.
//
//    Small sets (n_patterns <= SUMMARY_LDS_BINS): a workgroup counts its records in 32-bit bins in LDS (ds_add_u32, no
//    return value) and then adds its non-zero bins to hist, one 64-bit global atomic each (device scope: the workgroups
//    sit on every XCD) -- at most one per record it saw, and one per bin however dense the input is.
//    The bound: 8192 bins x 4 B = 32 KiB of a CU's 160 KiB of LDS, so five workgroups of 256 threads share a CU: 20 waves,
//    five per SIMD -- the 4-byte LDS operations need about four waves per SIMD to reach their rate.  Twice the bins
//    (64 KiB) would leave two workgroups, two waves per SIMD, and nothing larger fits the 64 KiB a workgroup may take.
//    The LDS is allocated at launch for n_patterns bins, so a smaller set leaves room for more workgroups.
//
//    Larger sets (up to the 2^24 patterns of a handle): a 64-bit global atomic per record, device scope.  Equal patterns
//    within a wave are NOT aggregated: with more than 8192 bins a wave's 64 records rarely share one (the compiler's own
//    per-wave aggregation needs a wave-uniform address), and the cost of a match-any step per record would be paid by every
//    input.  An input dominated by a few patterns of a large set serialises on their bins.
//
//    Both forms read the `pattern` field alone: one 8-byte load per 24-byte record (global_load_dwordx2 in the ISA).
//    Whole records as 16-byte pieces are three loads for two records, of which the third holds no pattern: two 16-byte
//    loads for two records is the same one instruction per record, with twice the bytes in registers.
//
//    A workgroup's 32-bit bins cannot overflow while it sees fewer than 2^32 records: summary_hist_grid sizes the grid for
//    that and summary_hist checks it.
// ---------------------------------------------------------------------------
constexpr uint32_t SH_THREADS = 256, SH_PER_WG = 16 * SH_THREADS, SH_MAX_GRID = 1024;

__global__ __launch_bounds__(SH_THREADS) void k_sum_hist_lds(const acx_match_t *__restrict__ m, uint64_t n, uint32_t n_patterns,
                                                             unsigned long long *__restrict__ hist) {
    extern __shared__ uint32_t s_bins[]; // n_patterns words
    for (uint32_t b = threadIdx.x; b < n_patterns; b += SH_THREADS) s_bins[b] = 0;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * SH_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * SH_THREADS + threadIdx.x; i < n; i += stride) {
        const uint64_t p = m[i].pattern;
        if (p < n_patterns) atomicAdd(&s_bins[p], 1u);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < n_patterns; b += SH_THREADS) {
        const uint32_t v = s_bins[b];
        if (v) atomicAdd(&hist[b], (unsigned long long)v);
    }
}

__global__ __launch_bounds__(SH_THREADS) void k_sum_hist_global(const acx_match_t *__restrict__ m, uint64_t n,
                                                                uint64_t n_patterns, unsigned long long *__restrict__ hist) {
    const uint64_t stride = (uint64_t)gridDim.x * SH_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * SH_THREADS + threadIdx.x; i < n; i += stride) {
        const uint64_t p = m[i].pattern;
        if (p < n_patterns) atomicAdd(&hist[p], 1ull);
    }
}

uint32_t summary_hist_grid(uint64_t n) {
    uint64_t g = std::min<uint64_t>((n + SH_PER_WG - 1) / SH_PER_WG, SH_MAX_GRID);
    g = std::max<uint64_t>(g, (n >> 31) + 1); // (a workgroup sees at most n / g + SH_THREADS records: below 2^32)
    return (uint32_t)std::min<uint64_t>(g, 0x7FFFFFFFull);
}

hipError_t summary_hist(const acx_match_t *m, uint64_t n, uint64_t n_patterns, uint64_t *hist, hipStream_t st) {
    if (!n_patterns) return hipSuccess;
    hipError_t e = hipMemsetAsync(hist, 0, n_patterns * 8, st);
    if (e != hipSuccess || !n) return e;
    const uint32_t grid = summary_hist_grid(n);
    if (n / grid + SH_THREADS >= (1ull << 32)) return hipErrorInvalidValue; // (a workgroup's 32-bit bins would not hold its records)
    if (n_patterns <= SUMMARY_LDS_BINS)
        hipLaunchKernelGGL(k_sum_hist_lds, dim3(grid), dim3(SH_THREADS), (size_t)n_patterns * 4, st, m, n, (uint32_t)n_patterns,
                           (unsigned long long *)hist);
    else
        hipLaunchKernelGGL(k_sum_hist_global, dim3(grid), dim3(SH_THREADS), 0, st, m, n, n_patterns, (unsigned long long *)hist);
    return hipGetLastError();
}

} // namespace acx
