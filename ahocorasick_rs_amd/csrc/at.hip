// at.hip -- the match-at kernels behind acx_match_at / acx_match_at_device / acx_match_at_into_device (at.hpp has the
// definition and says what each phase computes).  The find pipeline (kernels.hip) and the post-find stages are not touched:
// this is a walk of its own over tables every handle has, and the scan of the overlapping form's counts is replace_scan's.
//
// RELIED ON: the tables are a compiled handle's -- first_child rises, first_child[n_states] = n_states, a child's id is never
// 0 (the root is nobody's child), own_off rises and own_pid holds a pattern per entry.  Whatever the data and the positions
// are, a walk reads haystack bytes p .. L - 1 only, with p < L <= len checked in phase A, and follows edges of the trie only:
// it ends when no child takes the byte, at the latest at the depth of the longest pattern.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "at.hpp"
#include "at_walk.hpp"

namespace acx {

constexpr uint32_t AT_IPT = AT_TILE / AT_THREADS; // anchors of one thread in phases A and C
constexpr int AT_MODE_WALK = 0, AT_MODE_COUNT = 1, AT_MODE_EMIT = 2;
static_assert(AT_IPT * AT_THREADS == AT_TILE && AT_THREADS % 64 == 0, "whole waves, whole tiles");
static_assert(AT_THREADS >= 256, "root_next is copied to LDS by the first 256 threads");
static_assert(AT_TILE <= 65536, "a slot of the survivor list is 16 bits wide");

// where the row of position p < R.len ends, never past R.len (the offsets are the caller's word: the row index is clamped
// into [0, R.n) before an offset is read; R.n > 0)
__device__ inline uint64_t at_row_end(const RowCut &R, uint64_t p) {
    if (R.off) {
        const uint64_t r = std::min<uint64_t>(std::max<uint64_t>(count_le(R.off, R.n + 1, p), 1) - 1, R.n - 1);
        return std::min<uint64_t>(R.off[r + 1], R.len);
    }
    if (R.uniform_len) return p + std::min<uint64_t>(R.uniform_len - p % R.uniform_len, R.len - p);
    return R.len;
}

template <int MODE>
__global__ __launch_bounds__(AT_THREADS) void k_at(const AtTrie T, const uint8_t *__restrict__ hay, const RowCut R,
                                                   const int64_t *__restrict__ pos, const uint64_t A, const int kind,
                                                   const uint32_t flags, const int64_t *__restrict__ base,
                                                   int64_t *__restrict__ pattern, int64_t *__restrict__ end,
                                                   uint64_t *__restrict__ counts) {
    __shared__ uint32_t s_root[256];
    __shared__ uint64_t s_pos[AT_TILE];
    __shared__ uint32_t s_lim[AT_TILE];  // A: the bytes the walk may read, min(L - p, 2^32 - 1); after B: the matched length
    __shared__ uint32_t s_res[AT_TILE];  // A: a survivor's depth-1 state; after B: the pattern or AT_NONE (count: the entries)
    __shared__ uint16_t s_list[AT_TILE]; // the survivors' slots
    __shared__ uint32_t s_n;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint64_t tile = (uint64_t)blockIdx.x * AT_TILE;
    const bool fold = (flags & AT_FOLD) != 0, full = (flags & AT_FULL) != 0, row_starts = (flags & AT_ROW_STARTS) != 0;
    if (tid < 256) s_root[tid] = T.root_next[tid];
    if (tid == 0) s_n = 0;
    __syncthreads();

    // ---- A: position, limit, first byte; the survivors into the list (walk_push)
#pragma unroll
    for (uint32_t k = 0; k < AT_IPT; k++) {
        const uint32_t slot = k * AT_THREADS + tid;
        const uint64_t idx = tile + slot;
        uint64_t p = 0, L = 0;
        if (idx < A && R.n) {
            if (row_starts) {
                if (idx < R.n) { // (A == R.n)
                    p = row_begin(R, idx);
                    L = std::min<uint64_t>(row_begin(R, idx + 1), R.len);
                }
            } else {
                p = (uint64_t)pos[idx];
                L = p < R.len ? at_row_end(R, p) : 0;
            }
        }
        uint32_t s1 = 0;
        if (p < L) { // (p < L <= R.len: the byte is the data's)
            const uint8_t b = hay[p];
            s1 = s_root[fold ? fold_byte(b) : b];
        }
        const bool survive = s1 != 0;
        s_pos[slot] = p;
        s_lim[slot] = survive ? (uint32_t)std::min<uint64_t>(L - p, 0xFFFFFFFFull) : 0u;
        s_res[slot] = survive ? s1 : (MODE == AT_MODE_WALK ? AT_NONE : 0u);
        walk_push(survive, slot, lane, &s_n, s_list);
    }
    __syncthreads();

    // ---- B: the walks, a survivor per lane
    const uint32_t n_live = s_n; // (<= AT_TILE: every slot is listed at most once)
    for (uint32_t j = tid; j < n_live; j += AT_THREADS) {
        const uint32_t slot = s_list[j];
        const uint64_t p = s_pos[slot];
        const uint32_t lim = s_lim[slot];
        const uint32_t s = s_res[slot];
        uint32_t best = AT_NONE, best_len = 0, cnt = 0;
        uint64_t w = 0, w_end = 0;
        if (MODE == AT_MODE_EMIT) {
            w = (uint64_t)base[tile + slot];
            w_end = (uint64_t)base[tile + slot + 1];
        }
        at_path(T, hay, p, lim, s, fold, [&](uint32_t q, uint32_t d) { // a pattern ends at state q
            if (full && d != lim) return true;                         // (FULL: and the row does)
            if (MODE == AT_MODE_WALK) return at_pick(T, q, d, kind, full, best, best_len);
            const uint32_t o0 = T.own_off[q], o1 = T.own_off[q + 1];
            if (MODE == AT_MODE_COUNT) {
                cnt += o1 - o0;
            } else {
                for (uint32_t o = o0; o < o1 && w < w_end; o++, w++) {
                    pattern[w] = (int64_t)T.own_pid[o];
                    end[w] = (int64_t)(row_starts ? (uint64_t)d : p + d);
                }
            }
            return true;
        });
        if (MODE == AT_MODE_WALK) {
            s_res[slot] = best;
            s_lim[slot] = best_len;
        } else if (MODE == AT_MODE_COUNT) {
            s_res[slot] = cnt;
        }
    }
    if (MODE == AT_MODE_EMIT) return; // (no barrier follows)
    __syncthreads();

    // ---- C: every thread stores its own anchors' results
#pragma unroll
    for (uint32_t k = 0; k < AT_IPT; k++) {
        const uint32_t slot = k * AT_THREADS + tid;
        const uint64_t idx = tile + slot;
        if (idx >= A) continue;
        const uint32_t r = s_res[slot];
        if (MODE == AT_MODE_WALK) {
            const uint64_t e = row_starts ? (uint64_t)s_lim[slot] : s_pos[slot] + s_lim[slot];
            pattern[idx] = r == AT_NONE ? -1 : (int64_t)r;
            end[idx] = r == AT_NONE ? -1 : (int64_t)e;
        } else {
            counts[idx] = r;
        }
    }
}

// a thread per row (and one more): the pieces that begin before the row does, clamped into [0, total]
__global__ __launch_bounds__(AT_THREADS) void k_piece_rows(const RowCut R, const int64_t *__restrict__ starts, const uint64_t total,
                                                           int64_t *__restrict__ row_offsets) {
    const uint64_t r = (uint64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (r > R.n) return;
    row_offsets[r] = (int64_t)(r == R.n ? total : std::min<uint64_t>(count_lt(starts, total, row_begin(R, r)), total));
}

hipError_t piece_rows(const RowCut &R, const int64_t *starts, uint64_t total, int64_t *row_offsets, hipStream_t st) {
    if (!row_offsets || R.n >= (1ull << 38)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_piece_rows, dim3((uint32_t)tiles_of(R.n + 1, AT_THREADS)), dim3(AT_THREADS), 0, st, R, starts, total, row_offsets);
    return hipGetLastError();
}

namespace {
template <int MODE>
hipError_t at_launch(const AtTrie &T, const uint8_t *hay, const RowCut &R, const int64_t *pos, uint64_t A, int kind, uint32_t flags,
                     const int64_t *base, int64_t *pattern, int64_t *end, uint64_t *counts, hipStream_t st) {
    if (!A || A >= AT_MAX_ANCHORS || (!(flags & AT_ROW_STARTS) && !pos) || ((flags & AT_ROW_STARTS) && A != R.n) ||
        (R.len && !hay))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_at<MODE>, dim3((uint32_t)tiles_of(A, AT_TILE)), dim3(AT_THREADS), 0, st, T, hay, R, pos, A, kind, flags,
                       base, pattern, end, counts);
    return hipGetLastError();
}
} // namespace

hipError_t at_walk(const AtTrie &T, const uint8_t *hay, const RowCut &R, const int64_t *pos, uint64_t A, int kind, uint32_t flags,
                   int64_t *pattern, int64_t *end, hipStream_t st) {
    return at_launch<AT_MODE_WALK>(T, hay, R, pos, A, kind, flags, nullptr, pattern, end, nullptr, st);
}

hipError_t at_count(const AtTrie &T, const uint8_t *hay, const RowCut &R, const int64_t *pos, uint64_t A, uint32_t flags,
                    uint64_t *counts, hipStream_t st) {
    return at_launch<AT_MODE_COUNT>(T, hay, R, pos, A, ACX_MATCH_STANDARD, flags, nullptr, nullptr, nullptr, counts, st);
}

hipError_t at_emit(const AtTrie &T, const uint8_t *hay, const RowCut &R, const int64_t *pos, uint64_t A, uint32_t flags,
                   const int64_t *base, int64_t *pattern, int64_t *end, hipStream_t st) {
    return at_launch<AT_MODE_EMIT>(T, hay, R, pos, A, ACX_MATCH_STANDARD, flags, base, pattern, end, nullptr, st);
}

} // namespace acx
