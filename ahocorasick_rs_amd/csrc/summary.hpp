// summary.hpp -- launch wrappers of the reduction kernels in summary.hip (acx_summarize / acx_summarize_device).
//
// A find result in HBM -- records m[0 .. n) grouped by haystack with local offsets, and counts[n_hay] -- is reduced where it
// lies; only the reduction crosses to the host.  All on the caller's stream behind the find's write kernel, all indexes 64-bit:
//   1. summary_gather   first[h] = the first record of haystack h (pattern = UINT64_MAX, start = end = 0: none) and bit h of
//                       the `any` bitmap ((n_hay + 63) / 64 words, LSB first within a word).  Where a haystack's records
//                       begin is the exclusive prefix of the counts: replace_scan (replace.hpp) over `counts`.
//   2. summary_hist     hist[p] = the records whose pattern is p.  Up to SUMMARY_LDS_BINS patterns: a 32-bit histogram per
//                       workgroup in LDS, flushed with one 64-bit global atomic per non-zero bin; beyond: a 64-bit global
//                       atomic per record.
// There is no early exit: a summary costs the find over the whole input plus these passes over its result.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/acx.h"

namespace acx {

// the largest pattern set whose histogram a workgroup keeps in LDS (summary.hip says where the number comes from)
constexpr uint32_t SUMMARY_LDS_BINS = 8192;

// prefix: n_hay + 1 entries, prefix[h] = the first record of haystack h, prefix[n_hay] = n (replace_scan over the counts);
// null: one haystack, records 0 .. n.  first: n_hay records, any: (n_hay + 63) / 64 words.  n_hay == 0: nothing is launched.
hipError_t summary_gather(const acx_match_t *m, uint64_t n, const int64_t *prefix, uint64_t n_hay, acx_match_t *first,
                          uint64_t *any, hipStream_t st);
// hist: n_patterns words, cleared here on the stream.  A record whose pattern is >= n_patterns is not counted (it cannot
// come from a find of the handle; no bin is ever written out of bounds).
hipError_t summary_hist(const acx_match_t *m, uint64_t n, uint64_t n_patterns, uint64_t *hist, hipStream_t st);
// the grid summary_hist launches for n records (the host asserts that no workgroup of it sees 2^32 records)
uint32_t summary_hist_grid(uint64_t n);

} // namespace acx
