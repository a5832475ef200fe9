// replace.hpp -- launch wrappers of the splice kernels in replace.hip (acx_replace / acx_replace_device).
//
// A call's non-overlapping matches (p_i, s_i, e_i) and one replacement r[p] per pattern give
//   out = h[0:s_0] + r[p_0] + h[e_0:s_1] + r[p_1] + ... + r[p_last] + h[e_last:]
// The device form in three steps, all on the caller's stream and all offsets 64-bit (output can exceed 2^32 bytes):
//   1. replace_scan     P[i] = sum_{j<i} d_j, d_j = |r[p_j]| - (e_j - s_j), P[n] = the total; the same two-launch scan
//                       gives the first match of every haystack of a batch from the result's per-haystack counts
//   2. replace_positions o[i] = (global start of match i) + P[i]: where replacement i begins in the output; out_off[h] =
//                       (where h begins) + P[first match of h] for h = 0 .. n_hay (out_off[n_hay] = the output's length)
//   3. replace_gather   output side: a workgroup per 16 KiB output tile, 16-byte stores; every chunk is taken from the
//                       replacement blob or from the haystack at its segment's shift (input = output - P[j + 1])
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/acx.h"
#include "stage_device.hpp"

namespace acx {

// The input's haystacks (cut: stage_device.hpp).  first != null: the first match of every haystack (cut.n + 1 entries,
// first[cut.n] = n); null: one haystack.
struct RepSegs {
    RowCut cut;
    const uint64_t *first;
};

// u64 words of scratch replace_scan needs for n items
uint64_t replace_scan_words(uint64_t n);
// out[i] = sum_{j<i} v_j for i = 0 .. n (n + 1 entries); v_j = counts[j] (m == null) or d_j (m != null; roff: n_repl + 1
// offsets of the replacement blob, d_j = roff[p + 1] - roff[p] - (e_j - s_j)).  temp: replace_scan_words(n) words.
hipError_t replace_scan(const acx_match_t *m, const uint64_t *roff, const uint64_t *counts, uint64_t n, int64_t *out,
                        uint64_t *temp, hipStream_t st);
hipError_t replace_positions(const acx_match_t *m, uint64_t n, const int64_t *P, const RepSegs &S, uint64_t *o,
                             uint64_t *out_off, hipStream_t st);
// u64 words of scratch replace_gather needs for an output of `total` bytes (the segments of every output tile)
uint64_t replace_tile_words(uint64_t total);
// out: round_up(total, 16) bytes, 16-byte aligned; hay: `len` readable bytes; blob: blob_len readable bytes;
// tiles: replace_tile_words(total) words
hipError_t replace_gather(const uint8_t *hay, uint64_t len, const acx_match_t *m, uint64_t n, const uint64_t *o,
                          const int64_t *P, const uint8_t *blob, uint64_t blob_len, const uint64_t *roff, uint64_t *tiles,
                          uint8_t *out, uint64_t total, hipStream_t st);

} // namespace acx
