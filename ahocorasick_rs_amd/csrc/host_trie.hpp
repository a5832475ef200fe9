// host_trie.hpp -- the host form of the anchored walk (at.hpp has the definition), for acx_match_at_host, acx_segment_host
// and acx_wordpiece_host: the compiled tables walked from the root or from a node along goto edges only, the match kind's
// choice among the candidates on that path (pick), and the characters of a host haystack for the entry points that speak in
// code points.  Host code only.
#pragma once
#include <algorithm>
#include <vector>

#include "fold.hpp"
#include "result_block.hpp"

namespace acxh ACX_HIDDEN {

struct HostTrie {
    const acx::Automaton &A;
    bool fold;
    uint32_t child(uint32_t s, uint8_t b) const {
        uint32_t lo = A.first_child[s], hi = A.first_child[s + 1];
        const uint32_t end = hi;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (A.in_byte[mid] < b) lo = mid + 1; else hi = mid;
        }
        return lo < end && A.in_byte[lo] == b ? lo : 0u;
    }
    // every state with own patterns on the path from `node` (0: the root) along h[p .. L), by the depth below the node:
    // visit(state, depth) -> go on?
    template <class Visit>
    void walk(const uint8_t *h, uint64_t p, uint64_t L, uint32_t node, Visit &&visit) const {
        uint32_t s = node;
        for (uint64_t d = 0; p + d < L;) {
            const uint8_t b = h[p + d];
            s = child(s, fold ? acx::fold_byte(b) : b);
            if (!s) return;
            d++;
            if (A.own_off[s + 1] > A.own_off[s] && !visit(s, d)) return;
        }
    }
    // The match kind's choice, stated once: the candidate `kind` keeps among the patterns that go on from `node` with
    // h[p .. L) -- match_at's result of the anchor (p, L) when node is the root; full: only candidates that end at L count,
    // and the first of them is the answer.  false: no candidate; *end: where the kept one ends.
    bool pick(const uint8_t *h, uint64_t p, uint64_t L, uint32_t node, int kind, bool full, int64_t *pid, uint64_t *end) const {
        int64_t best = -1;
        uint64_t best_end = 0;
        walk(h, p, L, node, [&](uint32_t s, uint64_t d) {
            if (full && p + d != L) return true;
            const int64_t i = (int64_t)A.own_pid[A.own_off[s]]; // (the lists are in id order)
            if (kind == ACX_MATCH_LEFTMOST_FIRST && !full && best >= 0 && best < i) return true;
            best = i;
            best_end = p + d;
            return !(kind == ACX_MATCH_STANDARD || full);
        });
        *pid = best;
        *end = best_end;
        return best >= 0;
    }
};

// the UTF-8 characters of a host haystack: where character k begins (units + 1 entries, the last one = len)
inline int char_starts(const uint8_t *hay, uint64_t len, std::vector<uint64_t> *cs) {
    try {
        cs->clear();
        for (uint64_t i = 0; i < len; i++)
            if ((hay[i] & 0xC0) != 0x80) cs->push_back(i);
        cs->push_back(len);
    } catch (...) { return fail(ACX_ENOMEM, "out of memory"); }
    return ACX_OK;
}
inline uint64_t char_of(const std::vector<uint64_t> &cs, uint64_t byte) { // the characters that begin before `byte`
    return (uint64_t)(std::lower_bound(cs.begin(), cs.end() - 1, byte) - cs.begin());
}

} // namespace acxh
