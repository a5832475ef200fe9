// score.hip -- the row-score kernels behind acx_score_device / acx_score_rows_device / acx_filter_scored_device (score.hpp
// says what each step computes).  The find pipeline (kernels.hip) and the other stages are not touched: the scan of the
// counts is replace_scan's, the compaction of the kept rows is the row filter's.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "score.hpp"
#include "stage_device.hpp"

namespace acx {

constexpr uint32_t SC_IPT = SCORE_TILE / SCORE_THREADS; // consecutive records of one thread
constexpr uint32_t SC_WAVES = SCORE_THREADS / 64;
constexpr uint32_t SC_WORDS = SCORE_TILE / 32;          // words of the bitmap with one bit per record a row may begin at
static_assert(SC_IPT * SCORE_THREADS == SCORE_TILE && SC_IPT == 8, "a thread reads its 8 weights as two 16-byte LDS loads");
static_assert(SCORE_THREADS % 64 == 0 && SC_WORDS + 1 <= SCORE_THREADS, "whole waves; one thread clears one bitmap word");

// per tile of SCORE_TILE records the rows that hold its first and its last record (stage_device.hpp)
__global__ void k_score_tiles(const int64_t *__restrict__ rec_off, uint64_t rows, uint64_t n, uint64_t ntiles,
                              uint64_t *__restrict__ U, uint64_t *__restrict__ L) {
    rec_tile_bounds<SCORE_TILE>(rec_off, rows, n, ntiles, U, L);
}

// ---------------------------------------------------------------------------
// The tile kernel.  Tile t is records [base, base + cnt); its rows are r0 = U[t] .. r1 = L[t].  A non-empty row is named
// by the record it begins at, relative to the tile -- its slot, below SCORE_TILE -- never by its distance from r0: there
// may be millions of empty rows between two records.
//
//   weights the pattern word of every record (one 8-byte load, lane l next to lane l + 1's record, all of a thread's loads
//           before the first gather), then weights[pattern] from the int32 table in global memory (pattern >= n_patterns:
//           0, and no load) into s_val; the slots behind the tile's end hold 0.
//   rows    the threads walk r0 .. r1, SCORE_THREADS rows at a step, each row once: a non-empty one sets the bit of its slot
//           in s_head and leaves its index in s_row[slot].  r0 begins at or before the tile: its slot is 0.  Empty rows
//           cost this walk and nothing else; those that sit exactly on a tile boundary belong to no tile at all.
//   sum     thread t owns slots 8 t .. 8 t + 7: its own segmented sum (the sum since the last row start, and that start),
//           an inclusive segmented scan across the wave's lanes (__shfl_up), the waves' totals through LDS.
//   write   the thread that holds a row's last record IN THE TILE writes.  The row lies wholly in the tile unless it is r0
//           and began before the tile, or it is r1 and goes on behind it: a plain 8-byte store.  Else a 64-bit atomic add
//           onto the cleared score -- at most two per tile.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(SCORE_THREADS) void k_score(const uint64_t *__restrict__ w, uint64_t n,
                                                         const int64_t *__restrict__ rec_off,
                                                         const int32_t *__restrict__ weights, uint64_t n_patterns,
                                                         const uint64_t *__restrict__ U, const uint64_t *__restrict__ L,
                                                         unsigned long long *__restrict__ score) {
    __shared__ __attribute__((aligned(16))) int32_t s_val[SCORE_TILE];
    __shared__ uint64_t s_row[SCORE_TILE];
    __shared__ uint32_t s_head[SC_WORDS + 1]; // (one word more: a thread reads the bit behind its last slot)
    __shared__ int64_t s_wsum[SC_WAVES];
    __shared__ int32_t s_whead[SC_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * SCORE_TILE;
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(SCORE_TILE, n - base);
    const uint64_t r0 = U[blockIdx.x], r1 = L[blockIdx.x];
    const bool open_lo = (uint64_t)rec_off[r0] < base, open_hi = (uint64_t)rec_off[r1 + 1] > base + cnt;

    if (tid <= SC_WORDS) s_head[tid] = 0;
    __syncthreads();

    uint64_t pat[SC_IPT];
#pragma unroll
    for (uint32_t k = 0; k < SC_IPT; k++) {
        const uint32_t j = tid + k * SCORE_THREADS;
        pat[k] = j < cnt ? w[(base + j) * 3] : ~0ull;
    }
#pragma unroll
    for (uint32_t k = 0; k < SC_IPT; k++) s_val[tid + k * SCORE_THREADS] = pat[k] < n_patterns ? weights[pat[k]] : 0;

    for (uint64_t h = r0 + tid; h <= r1; h += SCORE_THREADS) {
        const uint64_t s = (uint64_t)rec_off[h], e = (uint64_t)rec_off[h + 1];
        if (e > s) {
            const uint64_t slot = s > base ? s - base : 0;
            if (slot < cnt) { // (always, for offsets that rise)
                atomicOr(&s_head[(uint32_t)slot >> 5], 1u << ((uint32_t)slot & 31));
                s_row[slot] = h;
            }
        }
    }
    __syncthreads();

    // this thread's slots: their weights, and the row-start bits of j0 .. j0 + 8
    const uint32_t j0 = tid * SC_IPT;
    const uint64_t two = (uint64_t)s_head[j0 >> 5] | ((uint64_t)s_head[(j0 >> 5) + 1] << 32);
    const uint32_t bits = (uint32_t)(two >> (j0 & 31)) & ((2u << SC_IPT) - 1);
    const int4 va = *(const int4 *)&s_val[j0], vb = *(const int4 *)&s_val[j0 + 4];
    const int32_t v[SC_IPT] = {va.x, va.y, va.z, va.w, vb.x, vb.y, vb.z, vb.w};

    // (sum, head): the sum since the last row start and that start's slot; head < 0: no row start so far.  Joining a
    // stretch `a` with the stretch `b` behind it gives b where b holds a row start, else (a.sum + b.sum, a.head).
    int64_t sum = 0;
    int32_t head = -1;
#pragma unroll
    for (uint32_t i = 0; i < SC_IPT; i++) {
        if ((bits >> i) & 1) { sum = 0; head = (int32_t)(j0 + i); }
        sum += v[i];
    }
    int64_t inc = sum;
    int32_t inc_head = head;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const int64_t us = __shfl_up(inc, d);
        const int32_t uh = __shfl_up(inc_head, d);
        if (lane >= d && inc_head < 0) { inc += us; inc_head = uh; }
    }
    if (lane == 63) { s_wsum[wave] = inc; s_whead[wave] = inc_head; }
    int64_t run = __shfl_up(inc, 1); // what lies before this thread in its wave ...
    int32_t run_head = __shfl_up(inc_head, 1);
    if (lane == 0) { run = 0; run_head = -1; }
    __syncthreads();
    if (run_head < 0) { // ... and before the wave, as far back as the last row start
        for (uint32_t q = wave; q-- > 0;) {
            run += s_wsum[q];
            run_head = s_whead[q];
            if (run_head >= 0) break;
        }
    }

#pragma unroll
    for (uint32_t i = 0; i < SC_IPT; i++) {
        const uint32_t j = j0 + i;
        if ((bits >> i) & 1) { run = 0; run_head = (int32_t)j; }
        run += v[i];
        if (j < cnt && run_head >= 0 && (j == cnt - 1 || ((bits >> (i + 1)) & 1))) { // the row's last record in the tile
            const uint64_t h = s_row[run_head];
            const bool whole = !(run_head == 0 && open_lo) && !(j == cnt - 1 && open_hi);
            if (whole) score[h] = (unsigned long long)run;
            else atomicAdd(&score[h], (unsigned long long)run);
        }
    }
}

__global__ void k_score_flags(const int64_t *__restrict__ score, uint64_t rows, int64_t min_score, uint64_t *__restrict__ flag) {
    const uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h < rows) flag[h] = score[h] >= min_score ? 1 : 0;
}

uint64_t score_tile_words(uint64_t n) { return rec_tile_words(n, SCORE_TILE); }

hipError_t score_rows(const acx_match_t *m, uint64_t n, const int64_t *rec_off, uint64_t rows, const int32_t *weights,
                      uint64_t n_patterns, uint64_t *tiles, int64_t *score, hipStream_t st) {
    if (!rows) return hipSuccess;
    hipError_t e = hipMemsetAsync(score, 0, rows * 8, st);
    if (e != hipSuccess || !n) return e;
    const uint64_t ntiles = tiles_of(n, SCORE_TILE);
    if (ntiles >= (1ull << 31)) return hipErrorInvalidValue;
    uint64_t *U = tiles, *L = tiles + ntiles;
    hipLaunchKernelGGL(k_score_tiles, dim3((uint32_t)((ntiles + 255) / 256)), dim3(256), 0, st, rec_off, rows, n, ntiles, U, L);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_score, dim3((uint32_t)ntiles), dim3(SCORE_THREADS), 0, st, (const uint64_t *)m, n, rec_off, weights,
                       n_patterns, (const uint64_t *)U, (const uint64_t *)L, (unsigned long long *)score);
    return hipGetLastError();
}

hipError_t score_flags(const int64_t *score, uint64_t rows, int64_t min_score, uint64_t *flag, hipStream_t st) {
    if (!rows) return hipSuccess;
    hipLaunchKernelGGL(k_score_flags, dim3((uint32_t)((rows + 255) / 256)), dim3(256), 0, st, score, rows, min_score, flag);
    return hipGetLastError();
}

} // namespace acx
