// find_attempts.hpp -- the state of one find call across its attempts, and the general pipeline (find_attempts.cpp).
#pragma once
#include "find_pipeline.hpp"

namespace acxh ACX_HIDDEN {

// what one call works on (all attempts of it)
struct FindCall {
    acx_automaton *a;
    Ctx *c;
    const uint8_t *d_hay;
    uint64_t len;
    const Segments &G;
    bool overlapping, codepoints, segmented;
    acx_result *r;
    int key_mode;
    bool pre;           // K1b (else K1a)
    uint32_t scan_grid; // workgroups of the scan kernel
    uint32_t lead;      // d_hay & 15: index = stream position + lead
    uint64_t tiles;     // 4 KiB tiles of index space
    // results
    uint64_t n_raw = 0, n_final = 0, n_hits = 0;
    bool exact_regions = false; // dense path, second pass: regions at the exclusive prefix of the first pass's counts
    bool chunked_walk = false;  // dense path, K1a: the failureless walk ran out of item room, walk in chunks
    bool no_dense_tiles = false; // dense path: the tile-ordered form gave up on this call (the radix-sort form takes it)
    bool ovf_grown = false;      // sparse path: the overflow list was grown for this call (one more attempt)
    bool wide_tried = false;     // sparse path: the call was repeated with the wide form of the post stage
    bool host_result = false;    // the caller reads the matches on the host right away (acx_find): the sparse path writes them
                                 // to the context's pinned buffer when its capacity fits (PIN_FINAL_MAX), no copy kernel-side
    acx_match_t *out = nullptr;  // sparse path: where the write kernels put the records (w.final, or w.pin_final)
    uint64_t out_cap = 0;
    bool counts_zeroed = false; // batch: the per-haystack counts are zero or being accumulated into
    uint64_t exact_total = 0;
    bool timed = false;         // this call carries the profiling events (every prof_every-th call of a context)
    bool early_event = false;   // the caller returns before the device work is done: fence it with r->done
    bool event_at_post = false; // r->done was recorded right behind the post kernels
    bool leads_counted = false; // the scan has written the lead-byte counts of every 64 bytes (str API)
    bool cp_done = false;       // the write kernel has already converted the offsets to code points
    bool queued = false;    // work queued on the stream that nobody waited for yet
    bool localized = false; // batch: offsets are already local and the counts taken
};

int run_pipeline(FindCall &c);    // the general pipeline on an allocated result
int zero_counts(FindCall &c);     // batch: the per-haystack counts start at zero (once per call)
int finish_matches(FindCall &c);  // everything after the matches exist: code points (str API), local offsets + counts (batches)

} // namespace acxh
