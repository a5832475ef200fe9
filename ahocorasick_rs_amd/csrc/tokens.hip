// tokens.hip -- the token-label kernels behind acx_tokens_device / acx_tokens_rows_device (tokens.hpp has the definition and
// says what each step computes).  The find pipeline (kernels.hip) and the other stages are not touched: the scan of the counts
// is replace_scan's, the record-to-row assignment is k_mask_paint's idea, written again here.
//
// RELIED ON: atomicMin on a 64-bit word of global memory is performed at the L2 / memory side, device-wide, and min is
// commutative and associative: owner[t] ends as the smallest index of the records that touch t, whichever workgroup comes first
// and whether its records overlap another tile's or not.  The stream orders the clear before k_tok_own and k_tok_own before
// k_tok_label; no kernel here reads a word that the same kernel writes.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "tokens.hpp"

namespace acx {

constexpr uint32_t TK_IPT = TOK_TILE / TOK_THREADS; // records of one thread
constexpr uint32_t TK_WAVES = TOK_THREADS / 64;
constexpr uint64_t TK_NONE = ~0ull;                 // no owner
constexpr uint32_t TK_PER_THREAD = 4;               // tokens of one thread of k_tok_label
static_assert(TK_IPT * TOK_THREADS == TOK_TILE && TK_IPT == 4, "a thread reads its 4 row-start slots as one 16-byte LDS load");
static_assert(TOK_THREADS % 64 == 0 && TK_WAVES >= 2, "whole waves; the two bracket searches run in two waves");
static_assert(TOK_LONG >= 1, "a listed record touches a token");

// per tile of TOK_TILE records the rows that hold its first and its last record (stage_device.hpp)
__global__ void k_tok_tiles(const int64_t *__restrict__ rec_off, uint64_t rows, uint64_t n, uint64_t ntiles,
                            uint64_t *__restrict__ U, uint64_t *__restrict__ L) {
    rec_tile_bounds<TOK_TILE>(rec_off, rows, n, ntiles, U, L);
}

// ---------------------------------------------------------------------------
// The owner kernel.  Tile t is records [base, base + cnt); its rows are r0 = U[t] .. r1 = L[t].  A non-empty row is named by
// the record it begins at, relative to the tile -- its slot, below TOK_TILE -- never by its distance from r0.
//
//   records  the start and end words of every record, all of a thread's loads before anything depends on them.
//   rows     the threads walk r0 .. r1, TOK_THREADS rows at a step: a non-empty one writes its slot into s_head[slot] and leaves
//            its index in s_row[slot].  Empty rows cost this walk and nothing else.
//   owner    s_head[j] becomes the largest marked slot <= j, the slot of record j's row: thread t owns slots 4 t .. 4 t + 3,
//            an inclusive running maximum across the wave's lanes (__shfl_up), the waves' maxima through LDS.
//   ranges   record j's row, the row's first position and length (64-bit), the clip, g_s and g_e (an empty record: none).
//   bracket  the smallest g_s and the largest g_e of the tile's live records, across the wave (__shfl_xor) and the waves (LDS);
//            thread 0 searches te[0 .. T) for the first, thread 64 ts[0 .. T) for the second: tokens [s_lo, s_hi) hold
//            every token a record of the tile can touch.
//   tokens   every live record searches te and ts inside the bracket only; its touched tokens [first, end) lie in
//            [s_lo, s_hi), a part of [0, T), whatever the arrays hold.  Fewer than TOK_LONG: the thread's own atomics; else
//            an entry of s_long.
//   sweep    every listed record by the whole workgroup, a token per lane.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(TOK_THREADS) void k_tok_own(const uint64_t *__restrict__ w, uint64_t n,
                                                         const int64_t *__restrict__ rec_off, RowCut R,
                                                         const uint64_t *__restrict__ U, const uint64_t *__restrict__ L,
                                                         const int64_t *__restrict__ ts, const int64_t *__restrict__ te,
                                                         uint64_t T, unsigned long long *__restrict__ owner) {
    __shared__ uint64_t s_row[TOK_TILE];
    __shared__ __attribute__((aligned(16))) int32_t s_head[TOK_TILE];
    __shared__ uint32_t s_long[TOK_TILE][3]; // first token, end token, the record's slot
    __shared__ int32_t s_wmax[TK_WAVES];
    __shared__ uint64_t s_gmin[TK_WAVES], s_gmax[TK_WAVES];
    __shared__ uint64_t s_lo, s_hi;
    __shared__ uint32_t s_nlong;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * TOK_TILE;
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(TOK_TILE, n - base);
    const uint64_t r0 = U[blockIdx.x], r1 = L[blockIdx.x];

#pragma unroll
    for (uint32_t k = 0; k < TK_IPT; k++) s_head[tid + k * TOK_THREADS] = -1;
    if (tid == 0) s_nlong = 0;
    __syncthreads();

    uint64_t rs[TK_IPT], re[TK_IPT];
#pragma unroll
    for (uint32_t k = 0; k < TK_IPT; k++) {
        const uint32_t j = tid + k * TOK_THREADS;
        rs[k] = j < cnt ? w[(base + j) * 3 + 1] : 0;
        re[k] = j < cnt ? w[(base + j) * 3 + 2] : 0;
    }

    for (uint64_t h = r0 + tid; h <= r1; h += TOK_THREADS) {
        const uint64_t s = (uint64_t)rec_off[h], e = (uint64_t)rec_off[h + 1];
        if (e > s) {
            const uint64_t slot = s > base ? s - base : 0;
            if (slot < cnt) { // (always, for offsets that rise)
                s_head[slot] = (int32_t)slot;
                s_row[slot] = h;
            }
        }
    }
    __syncthreads();

    // the running maximum of the marks; -1: no row start so far (never at slot 0 for offsets that rise)
    const uint32_t j0 = tid * TK_IPT;
    int4 v = *(const int4 *)&s_head[j0];
    v.y = std::max(v.x, v.y);
    v.z = std::max(v.y, v.z);
    v.w = std::max(v.z, v.w);
    int32_t inc = v.w;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const int32_t up = __shfl_up(inc, d);
        if (lane >= d) inc = std::max(inc, up);
    }
    if (lane == 63) s_wmax[wave] = inc;
    int32_t run = __shfl_up(inc, 1); // what lies before this thread in its wave ...
    if (lane == 0) run = -1;
    __syncthreads();
    for (uint32_t q = 0; q < wave; q++) run = std::max(run, s_wmax[q]); // ... and before the wave
    v.x = std::max(v.x, run);
    v.y = std::max(v.y, run);
    v.z = std::max(v.z, run);
    v.w = std::max(v.w, run);
    *(int4 *)&s_head[j0] = v;
    __syncthreads();

    // every record's global range; gs >= ge: it touches nothing
    uint64_t gs[TK_IPT], ge[TK_IPT], gmin = TK_NONE, gmax = 0;
#pragma unroll
    for (uint32_t k = 0; k < TK_IPT; k++) {
        const uint32_t j = tid + k * TOK_THREADS;
        gs[k] = ge[k] = 0;
        if (j >= cnt) continue;
        const int32_t hs = s_head[j];
        if (hs < 0) continue;
        const uint64_t h = s_row[hs];
        uint64_t b0 = 0, rl = R.len; // the row's first position and its length
        if (R.off) {
            const uint64_t e0 = R.off[h + 1];
            b0 = R.off[h];
            rl = e0 > b0 ? e0 - b0 : 0;
        } else if (R.uniform_len) {
            b0 = h * R.uniform_len;
            rl = R.uniform_len;
        }
        b0 = std::min(b0, R.len); // (a caller's wrong offsets: every position stays inside [0, len])
        rl = std::min(rl, R.len - b0);
        const uint64_t e = std::min(re[k], rl), s = std::min(rs[k], e); // the record, clipped to its row
        if (e <= s) continue;
        gs[k] = b0 + s;
        ge[k] = b0 + e;
        gmin = std::min(gmin, gs[k]);
        gmax = std::max(gmax, ge[k]);
    }
#pragma unroll
    for (uint32_t d = 32; d >= 1; d >>= 1) {
        gmin = std::min<uint64_t>(gmin, __shfl_xor((unsigned long long)gmin, d));
        gmax = std::max<uint64_t>(gmax, __shfl_xor((unsigned long long)gmax, d));
    }
    if (lane == 0) {
        s_gmin[wave] = gmin;
        s_gmax[wave] = gmax;
    }
    __syncthreads();
    if (lane == 0 && wave < 2) { // two searches over the whole arrays, in two waves
        uint64_t lo = TK_NONE, hi = 0;
        for (uint32_t q = 0; q < TK_WAVES; q++) {
            lo = std::min(lo, s_gmin[q]);
            hi = std::max(hi, s_gmax[q]);
        }
        const bool live = lo < hi;
        if (wave == 0) s_lo = live ? count_le(te, T, lo) : 0; // the tokens that end at or before the smallest start
        else s_hi = live ? count_lt(ts, T, hi) : 0;           // the tokens that begin before the largest end
    }
    __syncthreads();
    const uint64_t lo = std::min(s_lo, T), hi = std::min(std::max(s_hi, lo), T); // lo <= hi <= T, whatever the arrays hold

#pragma unroll
    for (uint32_t k = 0; k < TK_IPT; k++) {
        if (ge[k] <= gs[k]) continue;
        const uint32_t j = tid + k * TOK_THREADS;
        // both inside [lo, hi]: every token index below is inside [0, T) BEFORE it is used as one
        const uint64_t first = lo + count_le(te + lo, hi - lo, gs[k]), end = lo + count_lt(ts + lo, hi - lo, ge[k]);
        if (end <= first) continue;
        if (end - first < TOK_LONG) {
            for (uint64_t t = first; t < end; t++) atomicMin(&owner[t], (unsigned long long)(base + j));
        } else {
            const uint32_t q = atomicAdd(&s_nlong, 1u);
            s_long[q][0] = (uint32_t)first;
            s_long[q][1] = (uint32_t)end;
            s_long[q][2] = j;
        }
    }
    __syncthreads();

    const uint32_t nlong = s_nlong;
    for (uint32_t q = 0; q < nlong; q++) {
        const uint64_t first = s_long[q][0], end = s_long[q][1], idx = base + s_long[q][2];
        for (uint64_t t = first + tid; t < end; t += TOK_THREADS) atomicMin(&owner[t], (unsigned long long)idx);
    }
}

// ---------------------------------------------------------------------------
// The label kernel: thread i has tokens 4 i .. 4 i + 3.  The owner words are padded to a multiple of four and cleared with
// the rest, so both 16-byte loads lie inside them; the owner before the thread's first token is one more 8-byte load.
// wide: bit 0 -- pattern is 16-byte aligned, bit 1 -- begin is 4-byte aligned (uniform: the host looked at the pointers).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tok_label(const uint64_t *__restrict__ w, const uint64_t *__restrict__ owner, uint64_t T,
                                                   uint32_t wide, int64_t *__restrict__ pattern, uint8_t *__restrict__ begin) {
    const uint64_t t0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * TK_PER_THREAD;
    if (t0 >= T) return;
    const ulonglong2 a = *(const ulonglong2 *)(owner + t0), b = *(const ulonglong2 *)(owner + t0 + 2);
    const uint64_t o[TK_PER_THREAD] = {a.x, a.y, b.x, b.y};
    uint64_t prev = t0 ? owner[t0 - 1] : TK_NONE;
    int64_t p[TK_PER_THREAD];
    uint32_t bits = 0;
#pragma unroll
    for (uint32_t k = 0; k < TK_PER_THREAD; k++) {
        p[k] = o[k] == TK_NONE ? -1 : (int64_t)w[o[k] * 3];
        if (o[k] != TK_NONE && o[k] != prev) bits |= 1u << (8 * k);
        prev = o[k];
    }
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(TK_PER_THREAD, T - t0);
    if (cnt == TK_PER_THREAD && (wide & 1)) {
        *(longlong2 *)(pattern + t0) = make_longlong2(p[0], p[1]);
        *(longlong2 *)(pattern + t0 + 2) = make_longlong2(p[2], p[3]);
    } else {
#pragma unroll
        for (uint32_t k = 0; k < TK_PER_THREAD; k++)
            if (k < cnt) pattern[t0 + k] = p[k];
    }
    if (cnt == TK_PER_THREAD && (wide & 2)) {
        *(uint32_t *)(begin + t0) = bits;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < TK_PER_THREAD; k++)
            if (k < cnt) begin[t0 + k] = (uint8_t)(bits >> (8 * k));
    }
}

uint64_t tokens_tile_words(uint64_t n) { return rec_tile_words(n, TOK_TILE); }
uint64_t tokens_owner_words(uint64_t T) { return (T + TK_PER_THREAD - 1) / TK_PER_THREAD * TK_PER_THREAD; }

hipError_t tokens_label(const acx_match_t *m, uint64_t n, const int64_t *rec_off, const RowCut &R, const int64_t *ts,
                        const int64_t *te, uint64_t T, uint64_t *tiles, uint64_t *owner, int64_t *pattern, uint8_t *begin,
                        hipStream_t st) {
    const uint64_t ntiles = tiles_of(n, TOK_TILE);
    if (!n || !R.n || !T || T >= TOK_MAX_TOKENS || ntiles >= (1ull << 31)) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(owner, 0xFF, tokens_owner_words(T) * 8, st);
    if (e != hipSuccess) return e;
    uint64_t *U = tiles, *L = tiles + ntiles;
    hipLaunchKernelGGL(k_tok_tiles, dim3((uint32_t)((ntiles + 255) / 256)), dim3(256), 0, st, rec_off, R.n, n, ntiles, U, L);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_tok_own, dim3((uint32_t)ntiles), dim3(TOK_THREADS), 0, st, (const uint64_t *)m, n, rec_off, R,
                       (const uint64_t *)U, (const uint64_t *)L, ts, te, T, (unsigned long long *)owner);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const uint64_t threads = (T + TK_PER_THREAD - 1) / TK_PER_THREAD;
    const uint32_t wide = (((uintptr_t)pattern & 15) == 0 ? 1u : 0u) | (((uintptr_t)begin & 3) == 0 ? 2u : 0u);
    hipLaunchKernelGGL(k_tok_label, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, st, (const uint64_t *)m,
                       (const uint64_t *)owner, T, wide, pattern, begin);
    return hipGetLastError();
}

} // namespace acx
