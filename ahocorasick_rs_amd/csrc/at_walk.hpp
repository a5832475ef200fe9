// at_walk.hpp -- what the walkers' kernels share (k_at in at.hip, k_seg in seg.hip, k_wp in wp.hip).
// The anchored walk of the trie: the child of a state, the path of one anchor, the candidate a match kind keeps (at.hpp has
// the definition).  And the workgroup's steps around it in a tile kernel: the survivors' list, the row starts inside a tile
// as marks, the suffix minimum of every thread's first mark and the rank of every thread's count.  Device code only: the
// three .hip units include it, nothing else does.
//
// RELIED ON: the tables are a compiled handle's -- first_child rises, first_child[n_states] = n_states, a child's id is never
// 0 (the root is nobody's child), own_off rises and own_pid holds a pattern per entry.  A path reads haystack bytes
// p + 1 .. p + lim - 1 only and follows edges of the trie only: it ends when no child takes the byte, at the latest at the
// depth of the longest pattern.  The workgroup helpers are called by every thread of the workgroup (whole waves of 64) and
// hold no barrier: the kernel's own barriers stand where the comments say.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "at.hpp"
#include "fold.hpp"

namespace acx {

constexpr uint32_t AT_NONE = 0xFFFFFFFFu; // no pattern (OWN1_NONE, automaton.hpp, has the same value)
constexpr uint32_t AT_MANY = 0xFFFFFFFEu; // own1: several patterns end here (OWN1_MANY, automaton.hpp)

// the child of s that byte b leads to, or 0
__device__ inline uint32_t at_child(const AtTrie &T, uint32_t s, uint32_t b) {
    uint32_t lo = T.first_child[s];
    const uint32_t end = T.first_child[s + 1];
    if (end - lo <= AT_PROBE) {
        for (; lo < end; lo++) {
            const uint32_t x = T.in_byte[lo];
            if (x >= b) return x == b ? lo : 0u;
        }
        return 0u;
    }
    uint32_t hi = end;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (T.in_byte[mid] < b) lo = mid + 1; else hi = mid;
    }
    return lo < end && T.in_byte[lo] == b ? lo : 0u;
}

// The path of the anchor at p from its depth-1 state s (root_next of the first byte, not 0) while bytes remain below
// p + lim (lim >= 1): visit(state, depth) at every state with the OWN bit, in depth order; false ends the walk.
template <class Visit>
__device__ inline void at_path(const AtTrie &T, const uint8_t *__restrict__ hay, uint64_t p, uint32_t lim, uint32_t s, bool fold,
                               Visit &&visit) {
    for (uint32_t d = 1;;) {
        if ((T.sflags[s] & 1) && !visit(s, d)) return;
        if (d >= lim) return;
        const uint8_t b = hay[p + d]; // (p + d < p + lim <= L)
        const uint32_t c = at_child(T, s, fold ? fold_byte(b) : b);
        if (!c) return;
        s = c;
        d++;
    }
}

// The candidate of depth d -- the first own pattern of state s (OWN bit set) -- against the best so far (AT_NONE: none), by
// the match kind; only: all candidates share one depth (AT_FULL), the first one is the answer.  false: the walk is over.
__device__ inline bool at_pick(const AtTrie &T, uint32_t s, uint32_t d, int kind, bool only, uint32_t &best, uint32_t &best_len) {
    uint32_t pid = T.own1[s];
    if (pid == AT_MANY) pid = T.own_pid[T.own_off[s]];
    if (kind == ACX_MATCH_LEFTMOST_FIRST && !only) {
        if (pid < best) { best = pid; best_len = d; }
        return true;
    }
    best = pid;
    best_len = d;
    return !(kind == ACX_MATCH_STANDARD || only); // the first match state; FULL: the only depth
}

// ... at_path with at_pick (not FULL) as one call: the candidate `kind` keeps among the patterns that begin at p, AT_NONE: none
__device__ inline void at_best(const AtTrie &T, const uint8_t *__restrict__ hay, uint64_t p, uint32_t lim, uint32_t s, bool fold, int kind,
                               uint32_t &best, uint32_t &best_len) {
    best = AT_NONE;
    best_len = 0;
    at_path(T, hay, p, lim, s, fold, [&](uint32_t q, uint32_t d) { return at_pick(T, q, d, kind, false, best, best_len); });
}

// ---- the workgroup's steps around the walk ----

constexpr uint32_t WALK_FAR = 0xFFFFFFFFu; // no mark behind this byte inside the tile

// The survivors' list: `slot` goes into list[0 .. *n) when `survive` -- a ballot per wave, one LDS atomic per wave.  *n was 0
// behind a barrier; slots < 65536.
__device__ inline void walk_push(bool survive, uint32_t slot, uint32_t lane, uint32_t *n, uint16_t *list) {
    const uint64_t mask = __ballot(survive);
    if (mask) { // (wave-uniform)
        const int leader = __ffsll((unsigned long long)mask) - 1;
        uint32_t at = 0;
        if ((int)lane == leader) at = atomicAdd(n, (uint32_t)__popcll(mask));
        at = __shfl(at, leader);
        if (survive) list[at + (uint32_t)__popcll(mask & ((1ull << lane) - 1))] = (uint16_t)slot;
    }
}

// bit q of a bitmap in LDS that several threads mark at once
__device__ inline void walk_mark(uint32_t *bits, uint32_t q) { atomicOr(&bits[q >> 5], 1u << (q & 31)); }

// The row starts inside the tile [tile, tile_end) as marks, in two halves around a barrier of the kernel's.  AT_FIRST says
// whether a row start AT the tile's first byte is a mark:
//   false (k_seg)  marks are limits of the bytes in FRONT of them, and the tile's first byte has none in front: tile < v.
//                  The offsets' range begins at count_le(tile): a run of empty rows at the tile's first byte is skipped by
//                  the search, not iterated.  Rows of one length: from the first row start strictly behind the first byte.
//   true (k_wp)    marks are word boundaries, the tile's first byte included: tile <= v, the range begins at count_lt(tile),
//                  rows of one length from the first row start at or behind the first byte -- and the data's first byte
//                  begins a row, whatever the offsets say.
// The first half: cut[0 .. 1], the range of the offsets' indexes that may lie inside the tile, by two threads.
template <bool AT_FIRST>
__device__ inline void walk_row_range(const RowCut &R, uint64_t tile, uint64_t tile_end, uint32_t tid, uint64_t *cut) {
    if (!R.off) return;
    if (tid == 0) cut[0] = AT_FIRST ? count_lt(R.off, R.n + 1, tile) : count_le(R.off, R.n + 1, tile);
    if (tid == 64) cut[1] = count_lt(R.off, R.n + 1, tile_end);
}
// ... behind the barrier: the marks into `bits` (zeroed in front of the barrier; read behind the next one).  Returns `tail`:
// where the row of a byte without a mark behind it ends, at most R.len.
template <bool AT_FIRST, uint32_t THREADS, uint32_t TILE>
__device__ inline uint64_t walk_row_marks(const RowCut &R, uint64_t tile, uint64_t tile_end, uint32_t tid, const uint64_t *cut,
                                          uint32_t *bits) {
    uint64_t tail = R.len;
    if (AT_FIRST && tile == 0 && tid == 0) walk_mark(bits, 0);
    if (R.off) {
        const uint64_t a = cut[0], b = cut[1]; // (both <= R.n + 1: every index read is the offsets')
        for (uint64_t i = a + tid; i < b; i += THREADS) {
            const uint64_t v = R.off[i];
            if ((AT_FIRST ? v >= tile : v > tile) && v < tile_end) walk_mark(bits, (uint32_t)(v - tile));
        }
        if (b <= R.n) tail = std::min<uint64_t>(R.off[b], R.len);
    } else if (R.uniform_len) {
        const uint64_t u = R.uniform_len, first = AT_FIRST ? (tile + u - 1) / u * u : (tile / u + 1) * u;
        if (u >= TILE) {
            if (tid == 0 && first < tile_end) walk_mark(bits, (uint32_t)(first - tile));
        } else {
            for (uint64_t v = first + tid * u; v < tile_end; v += THREADS * u) walk_mark(bits, (uint32_t)(v - tile));
        }
        tail = std::min<uint64_t>(((tile_end - 1) / u + 1) * u, R.len);
    }
    return tail;
}

// The suffix minimum of every thread's first mark over the workgroup (v: the first mark among the thread's own bytes as a
// tile offset, or WALK_FAR), in two halves around a barrier of the kernel's.  The wave's half: the wave's minimum goes to
// w_min[wave]; returns the first mark behind the thread's bytes within its wave.
__device__ inline uint32_t walk_behind_wave(uint32_t v, uint32_t lane, uint32_t wave, uint32_t *w_min) {
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_down(v, d);
        if (lane + d < 64) v = std::min(v, o);
    }
    if (lane == 0) w_min[wave] = v;
    const uint32_t behind = __shfl_down(v, 1);
    return lane == 63 ? WALK_FAR : behind;
}
// ... behind the barrier: the first mark behind the thread's bytes within the tile
template <uint32_t WAVES>
__device__ inline uint32_t walk_behind(uint32_t behind, uint32_t wave, const uint32_t *w_min) {
#pragma unroll
    for (uint32_t w = 0; w < WAVES; w++) behind = w > wave ? std::min(behind, w_min[w]) : behind;
    return behind;
}

// The exclusive rank of every thread's count c over the workgroup, likewise.  The wave's half: a scan by __shfl_up, the
// wave's sum goes to w_sum[wave]; returns the inclusive sum within the wave.
__device__ inline uint32_t walk_rank_wave(uint32_t c, uint32_t lane, uint32_t wave, uint32_t *w_sum) {
    uint32_t inc = c;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(inc, d);
        if (lane >= d) inc += up;
    }
    if (lane == 63) w_sum[wave] = inc;
    return inc;
}
// ... behind the barrier: the counts of the threads in front of this one
template <uint32_t WAVES>
__device__ inline uint32_t walk_rank(uint32_t inc, uint32_t c, uint32_t wave, const uint32_t *w_sum) {
    uint32_t before = inc - c;
#pragma unroll
    for (uint32_t w = 0; w < WAVES; w++) before += w < wave ? w_sum[w] : 0u;
    return before;
}

} // namespace acx
