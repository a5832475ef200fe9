// words.hip -- the whole-word kernels behind acx_words_rows_device / acx_find_words_device / acx_filter_words_device
// (words.hpp says what each step computes and what it relies on).  The find pipeline (kernels.hip) and the other stages are
// not touched: the tile counts are scanned by replace_scan, the sort and the two device-wide scans are rocprim's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "words.hpp"

namespace acx {

namespace {

constexpr uint32_t WD_IPT = WORDS_TILE / WORDS_THREADS; // items of one thread
constexpr uint32_t WD_WAVES = WORDS_THREADS / 64;
static_assert(WD_IPT * WORDS_THREADS == WORDS_TILE && WD_IPT == 4, "a thread reads its 4 flags as one 4-byte load");
static_assert(WORDS_THREADS % 64 == 0, "whole waves");

__device__ inline bool is_word(const uint32_t *w, uint8_t b) { return (w[b >> 5] >> (b & 31)) & 1; }

// the row that holds item i: the LAST row that begins at or before it (of several rows with one start all but the last are
// empty).  off[0] = 0 and off[rows] = n > i bound the search; the clamp keeps a caller's wrong offsets inside the rows.
__device__ inline uint64_t row_of(const int64_t *off, uint64_t rows, uint64_t i) {
    return std::min<uint64_t>(std::max<uint64_t>(count_le(off, rows + 1, i), 1) - 1, rows - 1);
}

// where row h's bytes begin and how many they are, inside the batch whatever the offsets say
__device__ inline void row_bytes(const RowCut &R, uint64_t h, uint64_t *begin, uint64_t *L) {
    const uint64_t b = std::min(row_begin(R, h), R.len), e = std::min(std::max(row_begin(R, h + 1), b), R.len);
    *begin = b;
    *L = e - b;
}

// ---------------------------------------------------------------------------
// 1. the test.  Tile t is records [base, base + cnt); thread 0 finds the rows of the tile's first and last record, every
// record's row lies between the two.  Thread `tid` takes records tid, tid + 256, ...: lane l next to lane l + 1's record.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(WORDS_THREADS) void k_words_test(const uint64_t *__restrict__ w, uint64_t n,
                                                              const int64_t *__restrict__ rec_off, uint64_t rows, RowCut R,
                                                              const uint8_t *__restrict__ hay, WordSet W,
                                                              uint8_t *__restrict__ flag) {
    __shared__ uint64_t s_lo, s_hi;
    __shared__ uint32_t s_w[8];
    const uint32_t tid = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * WORDS_TILE;
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(WORDS_TILE, n - base);
    if (tid == 0) {
        s_lo = row_of(rec_off, rows, base);
        s_hi = row_of(rec_off, rows, base + cnt - 1);
    }
    if (tid < 8) s_w[tid] = W.w[tid];
    __syncthreads();
    const uint64_t lo = s_lo, hi = std::max(s_hi, lo);
    uint64_t rs[WD_IPT], re[WD_IPT];
#pragma unroll
    for (uint32_t k = 0; k < WD_IPT; k++) { // all loads before anything depends on them
        const uint32_t j = tid + k * WORDS_THREADS;
        rs[k] = j < cnt ? w[(base + j) * 3 + 1] : 0;
        re[k] = j < cnt ? w[(base + j) * 3 + 2] : 0;
    }
#pragma unroll
    for (uint32_t k = 0; k < WD_IPT; k++) {
        const uint32_t j = tid + k * WORDS_THREADS;
        if (j >= cnt) continue;
        const uint64_t i = base + j, s = rs[k], e = re[k];
        const uint64_t h = lo + count_le(rec_off + lo + 1, hi - lo, i); // the rows in (lo, hi] that begin at or before i
        uint64_t rb, L;
        row_bytes(R, h, &rb, &L);
        bool whole = s < e && e <= L;
        if (whole && s && is_word(s_w, hay[rb + s - 1])) whole = false;
        if (whole && e < L && is_word(s_w, hay[rb + e])) whole = false;
        flag[i] = whole ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------
// 2. the compaction.  Thread `tid` owns the consecutive slots 4 tid .. 4 tid + 3 of its tile.
// ---------------------------------------------------------------------------
__device__ inline uint32_t tile_flags(const uint8_t *__restrict__ flag, uint64_t base, uint32_t cnt, uint32_t j0) {
    // (flag lies 256 bytes aligned in the stage's block and is a multiple of 256 bytes long: the load stays inside it)
    uint32_t f = j0 < cnt ? *(const uint32_t *)(flag + base + j0) : 0;
    if (j0 + WD_IPT > cnt) f &= j0 < cnt ? (0xFFFFFFFFu >> (8 * (j0 + WD_IPT - cnt))) : 0;
    return f & 0x01010101u;
}

__global__ __launch_bounds__(WORDS_THREADS) void k_words_count(const uint8_t *__restrict__ flag, uint64_t n,
                                                               uint64_t *__restrict__ counts) {
    __shared__ uint32_t s_c[WD_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * WORDS_TILE;
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(WORDS_TILE, n - base);
    uint32_t c = __popc(tile_flags(flag, base, cnt, tid * WD_IPT));
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) c += __shfl_down(c, d);
    if (lane == 0) s_c[wave] = c;
    __syncthreads();
    if (tid == 0) {
        for (uint32_t q = 1; q < WD_WAVES; q++) c += s_c[q];
        counts[blockIdx.x] = c;
    }
}

__global__ __launch_bounds__(WORDS_THREADS) void k_words_emit(const uint8_t *__restrict__ flag, uint64_t n,
                                                              const int64_t *__restrict__ tbase, uint64_t total,
                                                              const uint32_t *__restrict__ src, const uint64_t *__restrict__ w,
                                                              WordsOut out, const int64_t *__restrict__ rec_off, uint64_t rows,
                                                              int64_t *__restrict__ new_off) {
    using scan_t = rocprim::block_scan<uint32_t, WORDS_THREADS>;
    __shared__ typename scan_t::storage_type s_scan;
    __shared__ uint32_t s_rank[WORDS_TILE];
    __shared__ uint64_t s_lo, s_hi;
    const uint32_t tid = threadIdx.x, j0 = tid * WD_IPT;
    const uint64_t t = blockIdx.x, base = t * WORDS_TILE;
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(WORDS_TILE, n - base);
    if (new_off && tid == 0) { // the rows h with base <= rec_off[h] < base + cnt, empty ones included
        const uint64_t lo = std::min(count_lt(rec_off, rows + 1, base), rows + 1);
        s_lo = lo;
        s_hi = std::max(std::min(count_le(rec_off, rows + 1, base + cnt - 1), rows + 1), lo);
    }
    const uint32_t f = tile_flags(flag, base, cnt, j0);
    const uint32_t c = __popc(f);
    uint32_t ex = 0, tile_total = 0;
    scan_t().exclusive_scan(c, ex, 0u, tile_total, s_scan, rocprim::plus<uint32_t>());
    const uint64_t tb = (uint64_t)tbase[t];
    uint32_t r = ex;
#pragma unroll
    for (uint32_t k = 0; k < WD_IPT; k++) {
        s_rank[j0 + k] = r;
        if ((f >> (8 * k)) & 1) {
            const uint64_t at = tb + r, i = base + j0 + k;
            if (at < total) {
                const uint64_t q = src ? (uint64_t)src[i] : i;
                const uint64_t p = w[q * 3], s = w[q * 3 + 1], e = w[q * 3 + 2];
                if (out.rec) {
                    uint64_t *o = (uint64_t *)out.rec + at * 3;
                    o[0] = p;
                    o[1] = s;
                    o[2] = e;
                }
                if (out.pattern) out.pattern[at] = (int64_t)p;
                if (out.start) out.start[at] = (int64_t)s;
                if (out.end) out.end[at] = (int64_t)e;
            }
            r++;
        }
    }
    if (!new_off) return;
    __syncthreads();
    // (the last tile goes on to h = rows: what is left has rec_off[h] == n, its value the total)
    const uint64_t stop = t + 1 == gridDim.x ? rows + 1 : s_hi;
    for (uint64_t h = s_lo + tid; h < stop; h += WORDS_THREADS) {
        const uint64_t s = (uint64_t)rec_off[h];
        new_off[h] = (int64_t)(tb + (s >= base && s - base < cnt ? s_rank[s - base] : tile_total));
    }
}

__global__ void k_words_row_counts(const int64_t *__restrict__ off, uint64_t rows, uint64_t *__restrict__ counts) {
    const uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h < rows) counts[h] = (uint64_t)(off[h + 1] - off[h]);
}

// ---------------------------------------------------------------------------
// 3. the resolve, on the survivors.  One thread per survivor in every kernel.
// ---------------------------------------------------------------------------
// gs, ge: the global positions; mode 0 (Standard): rev[n1 - 1 - i] = gs (the reverse min-scan's input); mode 1
// (LeftmostFirst): key = gs << 24 | pattern; mode 2 (LeftmostLongest): key = (len - (e - s)) << 24 | pattern.  idx[i] = i.
__global__ __launch_bounds__(WORDS_THREADS) void k_words_keys(const uint64_t *__restrict__ w, uint64_t n1,
                                                              const int64_t *__restrict__ off1, uint64_t rows, RowCut R, int mode,
                                                              uint64_t *__restrict__ gs, uint64_t *__restrict__ ge,
                                                              uint64_t *__restrict__ rev, uint64_t *__restrict__ key,
                                                              uint32_t *__restrict__ idx, uint64_t *__restrict__ err) {
    const uint64_t i = (uint64_t)blockIdx.x * WORDS_THREADS + threadIdx.x;
    if (i >= n1) return;
    const uint64_t p = w[i * 3], s = w[i * 3 + 1], e = w[i * 3 + 2];
    uint64_t rb, L;
    row_bytes(R, row_of(off1, rows, i), &rb, &L);
    // (a survivor has s < e <= L: both positions lie inside the batch, below 2^38)
    const uint64_t a = rb + std::min(s, L), b = rb + std::min(e, L);
    gs[i] = a;
    ge[i] = b;
    if (mode == 0) {
        rev[n1 - 1 - i] = a;
        return;
    }
    if (p >> WORDS_PATTERN_BITS) *err = 1;
    const uint64_t low = p & ((1ull << WORDS_PATTERN_BITS) - 1);
    key[i] = ((mode == 1 ? a : R.len - (b - a)) << WORDS_PATTERN_BITS) | low;
    idx[i] = (uint32_t)i;
}

// key[j] = gs[idx[j]]: the second sort's keys (LeftmostLongest)
__global__ __launch_bounds__(WORDS_THREADS) void k_words_starts(const uint64_t *__restrict__ gs, const uint32_t *__restrict__ idx,
                                                                uint64_t n1, uint64_t *__restrict__ key) {
    const uint64_t j = (uint64_t)blockIdx.x * WORDS_THREADS + threadIdx.x;
    if (j < n1) key[j] = gs[idx[j]];
}

// the records' positions in key order
__global__ __launch_bounds__(WORDS_THREADS) void k_words_order(const uint64_t *__restrict__ gs, const uint64_t *__restrict__ ge,
                                                               const uint32_t *__restrict__ idx, uint64_t n1,
                                                               uint64_t *__restrict__ ks, uint64_t *__restrict__ ke) {
    const uint64_t j = (uint64_t)blockIdx.x * WORDS_THREADS + threadIdx.x;
    if (j >= n1) return;
    const uint64_t q = idx[j];
    ks[j] = gs[q];
    ke[j] = ge[q];
}

// Place j of the key order begins a cluster when j == 0 or A(j) >= B[j - 1], A(j) = rev ? A[n1 - 1 - j] : A[j] -- Standard:
// the suffix minimum of the starts against the previous end; the leftmost kinds: the start against the running maximum of
// the ends.  The head's thread walks the cluster; every place belongs to exactly one, so every acc[j] is written once.
__global__ __launch_bounds__(WORDS_THREADS) void k_words_greedy(const uint64_t *__restrict__ ks, const uint64_t *__restrict__ ke,
                                                                const uint64_t *__restrict__ A, const uint64_t *__restrict__ B,
                                                                int rev, uint64_t n1, uint8_t *__restrict__ acc) {
    const uint64_t i = (uint64_t)blockIdx.x * WORDS_THREADS + threadIdx.x;
    if (i >= n1) return;
    if (i && (rev ? A[n1 - 1 - i] : A[i]) < B[i - 1]) return; // inside a cluster: its head's thread comes here
    uint64_t pos = 0, j = i;
    do {
        const bool take = ks[j] >= pos;
        acc[j] = take ? 1 : 0;
        if (take) pos = ke[j];
        j++;
    } while (j < n1 && (rev ? A[n1 - 1 - j] : A[j]) < B[j - 1]);
}

uint32_t bits_of(uint64_t v) {
    uint32_t b = 0;
    while (b < 64 && (v >> b)) b++;
    return b;
}
uint32_t grid1(uint64_t n) { return (uint32_t)((n + WORDS_THREADS - 1) / WORDS_THREADS); }

} // namespace

uint64_t words_tiles(uint64_t n) { return tiles_of(n, WORDS_TILE); }

hipError_t words_test(const acx_match_t *m, uint64_t n, const int64_t *rec_off, uint64_t rows, const RowCut &R, const uint8_t *hay,
                      const WordSet &W, uint8_t *flag, hipStream_t st) {
    const uint64_t T = words_tiles(n);
    if (!n || !rows || T >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_words_test, dim3((uint32_t)T), dim3(WORDS_THREADS), 0, st, (const uint64_t *)m, n, rec_off, rows, R, hay, W,
                       flag);
    return hipGetLastError();
}

hipError_t words_count(const uint8_t *flag, uint64_t n, uint64_t *counts, hipStream_t st) {
    const uint64_t T = words_tiles(n);
    if (!n || T >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_words_count, dim3((uint32_t)T), dim3(WORDS_THREADS), 0, st, flag, n, counts);
    return hipGetLastError();
}

hipError_t words_emit(const uint8_t *flag, uint64_t n, const int64_t *base, uint64_t total, const uint32_t *src, const acx_match_t *m,
                      const WordsOut &out, const int64_t *rec_off, uint64_t rows, int64_t *new_off, hipStream_t st) {
    const uint64_t T = words_tiles(n);
    if (!n || !rows || T >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_words_emit, dim3((uint32_t)T), dim3(WORDS_THREADS), 0, st, flag, n, base, total, src, (const uint64_t *)m, out,
                       rec_off, rows, new_off);
    return hipGetLastError();
}

hipError_t words_row_counts(const int64_t *off, uint64_t rows, uint64_t *counts, hipStream_t st) {
    if (!rows) return hipSuccess;
    if (rows >= (1ull << 39)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_words_row_counts, dim3(grid1(rows)), dim3(WORDS_THREADS), 0, st, off, rows, counts);
    return hipGetLastError();
}

ResolveLayout::ResolveLayout(uint64_t n1) {
    size_t a_ = 0, b_ = 0, c_ = 0;
    (void)rocprim::radix_sort_pairs(nullptr, a_, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr,
                                    (uint32_t *)nullptr, (size_t)n1, 0u, 64u, (hipStream_t)0);
    (void)rocprim::inclusive_scan(nullptr, b_, (const uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)n1, rocprim::maximum<uint64_t>(),
                                  (hipStream_t)0);
    (void)rocprim::inclusive_scan(nullptr, c_, (const uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)n1, rocprim::minimum<uint64_t>(),
                                  (hipStream_t)0);
    prim_bytes = std::max(a_, std::max(b_, c_));
    uint64_t at = 0;
    auto part = [&](uint64_t wds) { const uint64_t here = at; at += (wds + 31) / 32 * 32; return here; };
    gs = part(n1);
    ge = part(n1);
    a = part(n1);
    b = part(n1);
    key0 = part(n1);
    key1 = part(n1);
    idx0 = part((n1 + 1) / 2);
    idx1 = part((n1 + 1) / 2);
    prim = part((prim_bytes + 7) / 8);
    words = at;
}

hipError_t words_resolve(const acx_match_t *S, uint64_t n1, const int64_t *off1, uint64_t rows, const RowCut &R, int kind,
                         uint64_t *scratch, uint8_t *acc, const uint32_t **src, uint64_t *err, hipStream_t st) {
    if (!n1 || !rows || n1 >= WORDS_MAX_RECORDS || R.len >= WORDS_MAX_LEN) return hipErrorInvalidValue;
    const ResolveLayout Y(n1);
    uint64_t *gs = scratch + Y.gs, *ge = scratch + Y.ge, *a = scratch + Y.a, *b = scratch + Y.b, *key0 = scratch + Y.key0,
             *key1 = scratch + Y.key1;
    uint32_t *idx0 = (uint32_t *)(scratch + Y.idx0), *idx1 = (uint32_t *)(scratch + Y.idx1);
    void *prim = (void *)(scratch + Y.prim);
    size_t bytes = Y.prim_bytes;
    const int mode = kind == ACX_MATCH_STANDARD ? 0 : kind == ACX_MATCH_LEFTMOST_FIRST ? 1 : 2;
    const dim3 grid(grid1(n1)), block(WORDS_THREADS);
    hipLaunchKernelGGL(k_words_keys, grid, block, 0, st, (const uint64_t *)S, n1, off1, rows, R, mode, gs, ge, a, key0, idx0, err);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (mode == 0) { // key0 = the suffix minimum of the starts, reversed
        e = rocprim::inclusive_scan(prim, bytes, (const uint64_t *)a, key0, (size_t)n1, rocprim::minimum<uint64_t>(), st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_words_greedy, grid, block, 0, st, (const uint64_t *)gs, (const uint64_t *)ge, (const uint64_t *)key0,
                           (const uint64_t *)ge, 1, n1, acc);
        *src = nullptr;
        return hipGetLastError();
    }
    const unsigned len_bits = bits_of(R.len);
    e = rocprim::radix_sort_pairs(prim, bytes, (const uint64_t *)key0, key1, (const uint32_t *)idx0, idx1, (size_t)n1, 0u,
                                  WORDS_PATTERN_BITS + len_bits, st);
    if (e != hipSuccess) return e;
    const uint32_t *order = idx1;
    if (mode == 2) { // stable: the ties of one start stay longer first, then by pattern
        hipLaunchKernelGGL(k_words_starts, grid, block, 0, st, (const uint64_t *)gs, (const uint32_t *)idx1, n1, key0);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        bytes = Y.prim_bytes;
        e = rocprim::radix_sort_pairs(prim, bytes, (const uint64_t *)key0, key1, (const uint32_t *)idx1, idx0, (size_t)n1, 0u,
                                      std::max(len_bits, 1u), st);
        if (e != hipSuccess) return e;
        order = idx0;
    }
    // key0 = the starts, a = the ends, b = the running maximum of the ends, all in key order
    hipLaunchKernelGGL(k_words_order, grid, block, 0, st, (const uint64_t *)gs, (const uint64_t *)ge, order, n1, key0, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    bytes = Y.prim_bytes;
    e = rocprim::inclusive_scan(prim, bytes, (const uint64_t *)a, b, (size_t)n1, rocprim::maximum<uint64_t>(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_words_greedy, grid, block, 0, st, (const uint64_t *)key0, (const uint64_t *)a, (const uint64_t *)key0,
                       (const uint64_t *)b, 0, n1, acc);
    *src = order;
    return hipGetLastError();
}

} // namespace acx
