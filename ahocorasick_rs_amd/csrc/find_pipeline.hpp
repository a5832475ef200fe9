// find_pipeline.hpp -- a find call on a device haystack, its options and its result (find_pipeline.cpp).
#pragma once
#include "workspace.hpp"

struct ACX_HIDDEN acx_result {
    explicit acx_result(int device_) : device(device_) {} // an empty result on that device
    int device;
    acx_match_t *d_matches = nullptr;
    uint64_t n = 0;
    uint64_t *d_counts = nullptr;
    uint64_t n_hay = 0;
    hipEvent_t done = nullptr; // non-null: device work that fills the buffers may still be running
    bool borrowed = false;     // d_matches is the context's pinned host buffer (acx_find: the write kernel's records land where
                               // the host reads them); never handed to a caller, never given to the buffer cache
};

namespace acxh ACX_HIDDEN {

// the error of an overlapping search on a handle whose match kind has none (ACX_EOVERLAP), before any device state is touched
int check_overlapping(const acx_automaton *a);
// how a device entry point's byte stream is cut into haystacks: uniform_len, or n_hay + 1 device offsets, or one haystack
int make_segments(const uint64_t *d_offsets, uint64_t n_hay, uint64_t uniform_len, uint64_t len, Segments *G);
// ... a batch (offsets or a row length), not one haystack
inline bool is_segmented(const Segments &G) { return G.uniform_len != 0 || G.offsets != nullptr; }

struct FindOpts {
    bool allow_small = true;  // K0 may take the call (a small haystack)
    bool wait = false;        // return when the device work is done (else: when the totals are known, the rest fenced by r->done)
    int depth = 0;            // of a call in byte ranges / a batch in parts
    bool host_result = false; // the caller reads the matches on the host right away (acx_find)
};
// d_hay must stay valid until the result's device work is done (acx_result accessors wait for it)
int run_find(acx_automaton *a, Ctx *x, const uint8_t *d_hay, uint64_t len, const Segments &G, int overlapping, int codepoints,
             acx_result **out, const FindOpts &o = FindOpts());
// profiling: the scan time / the post-stage time of the context's last profiled call, if it has not been read yet
void settle_scan_profile(acx_automaton *a, Ctx *c);
void settle_post_profile(acx_automaton *a, Ctx *c);
// the result's buffers are complete after this
int result_wait(const acx_result *r);
// an overlapping search's K0 result on the host (*m: malloc, *n records): every occurrence becomes the run of its string's copies
int expand_copies_host(const acx_automaton *a, acx_match_t **m, uint64_t *n);

} // namespace acxh
