// find_policy.hpp -- which path a find call takes, and what a context remembers for its next calls: the decisions of
// find_attempts.cpp as pure functions of the totals' line and the context's history.  No HIP, no context, no environment:
// a host compiler alone builds this (tests/test_find_policy_cpu.py exercises every comparison at its boundary); the steps
// that launch, clear and wait, and what a failed allocation does, are find_attempts.cpp's.
#pragma once
#include <algorithm>
#include <cstdint>

namespace acx_policy {

// the limits the decisions compare against (find_attempts.cpp fills them from device_types.hpp and its own constants)
struct Limits {
    uint64_t hit_slots, ovf_lists, group_max, group_max_wide, hot_sub, dt_gmax; // HIT_SLOTS .. DT_GMAX
    uint64_t match_bytes;                                                       // sizeof(acx_match_t)
    uint64_t hot_inline, hot_inline_max, pin_final_max;                         // HOT_INLINE, HOT_INLINE_MAX, PIN_FINAL_MAX
};

// ---- the line k_tile_write publishes (kernels.hpp): [1] matches, [2] occurrences, [3] prefix hits, [4] why | hot groups
// << 8, [5] overflow hits | the fullest overflow list << 32.  The only place that shifts or masks these words.
struct TotalsLine {
    uint64_t matches, occurrences, prefix_hits;
    uint64_t why;     // 0, 1: aborted (the hot pipeline: gave up), 2: an overflow list was too small
    uint64_t n_hot;   // groups left to the hot pipeline
    uint64_t n_ovf;   // hits beyond their tiles' slots
    uint64_t ovf_max; // ... in the fullest list
};
inline TotalsLine decode_totals(const uint64_t line[8]) {
    return TotalsLine{line[1], line[2], line[3], line[4] & 0xFF, line[4] >> 8, line[5] & 0xFFFFFFFFull, line[5] >> 32};
}

// ---- output room of a sparse attempt: every group's capacity + what hot_room hot groups can report beyond it (run_hot)
inline uint64_t cap_for(const Limits &L, uint64_t n_groups, uint64_t gmax, bool pre, uint64_t hot_room) {
    return n_groups * gmax + (pre ? std::min<uint64_t>(n_groups, hot_room) * L.hot_sub * L.dt_gmax : 0);
}
// a host call's records go to the CONTEXT's pinned buffer, which is not regrown in the middle of a call: there the room
// for hot groups is the full figure while the whole fits PIN_FINAL_MAX; a device result's buffer is the caller's to hold:
// the context's own figure
inline bool pin_result(const Limits &L, bool host_result, bool segmented, bool expands_overlapping, uint64_t n_groups,
                       uint64_t gmax, bool pre) {
    return host_result && !segmented && cap_for(L, n_groups, gmax, pre, L.hot_inline_max) * L.match_bytes <= L.pin_final_max &&
           !expands_overlapping;
}
// the hot pipeline's output: the groups' capacities bound the matches
inline uint64_t hot_bound(const Limits &L, uint64_t n_groups, uint64_t gmax, uint32_t n_hot) {
    return (n_groups - n_hot) * gmax + (uint64_t)n_hot * L.hot_sub * L.dt_gmax;
}

// ---- hit counts: contiguous per wave of the scan (K1b, k1a_scan: 16 waves a workgroup); the chunked walk: plain per-tile
// arrival counters
struct HitCounters { uint32_t nw, iters; };
inline HitCounters hit_counters(bool pre, bool pfac, uint32_t scan_grid, uint32_t pfac_grid, uint64_t tiles) {
    const uint32_t nw = pre ? scan_grid * 16 : pfac ? pfac_grid * 16 : 1;
    return HitCounters{nw, nw > 1 ? (uint32_t)((tiles + nw - 1) / nw) : (uint32_t)tiles};
}

// ---- the hot pipeline queued ahead of the knowledge that the call needs it: grids for this many hot groups, 0: not
// queued.  Not beyond the room the output buffer has for hot groups, nor where a call with that many would rather take the
// wide form.  spec_hot: the hot groups of the context's last call.
inline uint32_t spec_bound(const Limits &L, uint32_t spec_hot, bool pinned, uint64_t hot_inline, uint64_t n_groups) {
    if (!spec_hot) return 0;
    uint64_t b = std::min<uint64_t>(2ull * spec_hot, L.hot_inline_max);
    b = std::min<uint64_t>(b, pinned ? L.hot_inline_max : hot_inline);
    b = std::min<uint64_t>(b, n_groups >= 32 ? n_groups / 32 : n_groups);
    return b >= spec_hot ? (uint32_t)b : 0u;
}

// ---- the verdict on pass 0's line
// K1b found more hits beyond their tiles' slots than an overflow list holds (nothing else is wrong): with lists of the size
// this input needs the sparse kernels + the hot pipeline take it -- again, once
inline bool regrow_overflow(const Limits &L, const TotalsLine &t, bool ovf_grown, uint64_t tiles) {
    return t.why == 2 && !ovf_grown && t.ovf_max * L.ovf_lists <= 3 * tiles * L.hit_slots + (L.ovf_lists << 12);
}
inline uint64_t overflow_room(const TotalsLine &t) { return t.ovf_max + t.ovf_max / 4 + 64; } // records per list, regrown
// what the context's next call queues ahead: the hot pipeline, when this one had a few hot groups
struct Speculation { uint32_t hot, ovf; };
inline Speculation next_speculation(const Limits &L, const TotalsLine &t) {
    return Speculation{(!t.why && t.n_hot && t.n_hot <= L.hot_inline_max) ? (uint32_t)t.n_hot : 0u, (uint32_t)t.ovf_max};
}
// the speculative pipeline is this call's: its pass 1 publishes the totals
inline bool spec_is_ours(uint32_t bound, const TotalsLine &t) { return bound && !t.why && t.n_hot && t.n_hot <= bound; }

// what the call knows of itself when the line is in
struct SparseCall {
    bool pre, wide, wide_tried, no_wide, ovf_grown;
    uint64_t n_groups;
};
enum class Act {
    RedoWide, // this call again in the wide form of the post stage, the context's next calls from the start
    RunHot,   // groups the sparse kernels could not finish: the hot pipeline, then the write kernel again
    Sparse,   // the sparse kernels finished every group
    SpecDone, // ... and the hot pipeline queued ahead finished the others
    Dense,    // the slots could not hold the output
};
struct Verdict {
    bool count_hot;     // a hot call (hot_calls, hot_groups, overflow_hits) by the speculative pipeline
    bool count_regrown; // overflow_regrown: the regrown lists held the hits
    Act act;
};
// t: pass 0's line, behind regrow_overflow (taken and failed, or not taken).  spec_done: spec_is_ours -- spec_lost: that
// pipeline gave up (why becomes 1); hits: the prefix hits of the last line read (the speculative pipeline's when it was
// waited for).  The wide form is weighed AFTER the speculative pipeline is counted: many groups gave up on the narrow stage
// although their tiles' slots held the hits (a match every 100 - 500 bytes: more than 24 occurrences in a 4 KiB bucket,
// more than GROUP_MAX in a group).
inline Verdict verdict(const SparseCall &s, const TotalsLine &t, bool spec_done, bool spec_lost, uint64_t hits) {
    const uint64_t why = spec_done && spec_lost ? 1 : t.why;
    Verdict v{spec_done && !spec_lost, s.ovf_grown && why != 2, Act::Dense};
    if (!why && s.pre && !s.wide && !s.wide_tried && !s.no_wide && s.n_groups >= 32 && t.n_hot * 32 > s.n_groups &&
        t.n_ovf * 8 <= hits)
        v.act = Act::RedoWide;
    else if (!why && !spec_done)
        v.act = t.n_hot ? Act::RunHot : Act::Sparse;
    else if (!why)
        v.act = Act::SpecDone;
    return v;
}

// ---- after the verdict
// hot groups the output buffers of the context's next calls have room for
inline uint64_t grown_hot_inline(const Limits &L, uint64_t n_hot, uint64_t hot_inline) {
    return n_hot > hot_inline ? std::min<uint64_t>(L.hot_inline_max, 2 * n_hot) : hot_inline;
}
// an input that is dense (nearly) everywhere: the dense path proper takes the handle's next calls
inline bool dense_everywhere(uint32_t n_hot, uint64_t n_groups) { return (uint64_t)n_hot * 4 > n_groups && n_groups >= 8; }
// back to the narrow form -- twice the groups in flight -- when the input no longer needs the wide one
inline bool leave_wide(const Limits &L, bool wide, uint64_t n_hot, uint64_t n_raw, uint64_t n_groups) {
    return wide && n_hot == 0 && n_raw * 5 < n_groups * L.group_max * 2;
}

// ---- the density hold: calls the context's handle keeps on the dense path, and why
struct Hold {
    int calls;  // Ctx::dense_hold
    bool input; // Ctx::hold_dense_input: the INPUT was dense (the hold ends with the first call that is not) -- or the sparse
                // kernels gave up for another reason (counted down, first by the dense attempt of the call that gave up: one
                // failed attempt in eight calls)
};
constexpr int HOLD_CALLS = 8;
constexpr Hold hold_dense_input() { return Hold{HOLD_CALLS, true}; } // dense_everywhere, and below
constexpr Hold hold_gave_up() { return Hold{HOLD_CALLS, false}; }    // Act::Dense (unless the dense path finds the input dense)
// a call of either dense form found n_raw occurrences
// (round 5: a hold that a dense INPUT set ends with the first input that is not dense -- the dense path on a sparse input
// costs 2-3x, eight calls of it were the price of one dense call in front: bench.py's 8 GiB run behind its density sweep)
inline Hold hold_after_dense(Hold h, uint64_t n_raw, uint64_t tiles) {
    if (n_raw > 8 * tiles) return hold_dense_input();
    if (h.calls > 0) h.calls = h.input ? 0 : h.calls - 1;
    return h;
}
// the tile-ordered dense form: k_dense_main compact -- sixteen groups per CU -- unless a call of this context did not fit
// it lately (Ctx::dense_full: calls left in the full form; DENSE_FULL_CALLS once a group did not fit)
constexpr int DENSE_FULL_CALLS = 8;
struct DenseForm { bool compact; int dense_full; };
inline DenseForm dense_form(int dense_full, bool no_compact) {
    return DenseForm{dense_full == 0 && !no_compact, dense_full > 0 ? dense_full - 1 : dense_full};
}

// ---- run_pipeline: the first attempt, the dense form, and how often a call goes again
constexpr int MAX_ATTEMPTS = 6;
constexpr uint64_t TILE_LIMIT = 1ull << 26; // tiles the tile kernels index
inline bool start_sparse(bool sparse_ok, int dense_hold, bool no_bucket, uint64_t tiles) {
    return sparse_ok && dense_hold == 0 && !no_bucket && tiles < TILE_LIMIT;
}
inline bool dense_in_tiles(bool pre, bool sparse_ok, bool gave_up_on_tiles, bool no_dense_tiles, uint64_t tiles) {
    return pre && sparse_ok && !gave_up_on_tiles && !no_dense_tiles && tiles < TILE_LIMIT;
}

} // namespace acx_policy
