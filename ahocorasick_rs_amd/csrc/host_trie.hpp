// host_trie.hpp -- the host form of the anchored walk (at.hpp has the definition), for acx_match_at_host and
// acx_segment_host: the compiled tables walked from the root along goto edges only, and the characters of a host haystack
// for the entry points that speak in code points.  Host code only.
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
    // every state with own patterns on the path from the root along h[p .. L), by depth: visit(state, depth) -> go on?
    template <class Visit>
    void walk(const uint8_t *h, uint64_t p, uint64_t L, Visit &&visit) const {
        uint32_t s = 0;
        for (uint64_t d = 0; p + d < L;) {
            const uint8_t b = h[p + d];
            s = child(s, fold ? acx::fold_byte(b) : b);
            if (!s) return;
            d++;
            if (A.own_off[s + 1] > A.own_off[s] && !visit(s, d)) return;
        }
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
