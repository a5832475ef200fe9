// at_walk.hpp -- the anchored walk of the trie that the match-at kernels (at.hip) and the segmenter (seg.hip) share: the child
// of a state, the path of one anchor, and the candidate a match kind keeps (at.hpp has the definition).  Device code only:
// the two .hip units include it, nothing else does.
//
// RELIED ON: the tables are a compiled handle's -- first_child rises, first_child[n_states] = n_states, a child's id is never
// 0 (the root is nobody's child), own_off rises and own_pid holds a pattern per entry.  A path reads haystack bytes
// p + 1 .. p + lim - 1 only and follows edges of the trie only: it ends when no child takes the byte, at the latest at the
// depth of the longest pattern.
#pragma once
#include <hip/hip_runtime.h>

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

} // namespace acx
