// spans.hpp -- launch wrappers of the span kernels in spans.hip (acx_spans_device / acx_spans_rows_device).
//
// A batch's find result in HBM -- records m[0 .. n) of 24 bytes, ordered by haystack ("row"), and rec_off[0 .. rows], where
// every row's records begin (replace_scan over the per-row counts) -- becomes the merged spans of the matches: the union of
// every row's records, two of them joined when the later one starts at most `gap` positions behind the earlier one's end, as
// two int64 columns `start` / `end` of S entries and rows + 1 row offsets (the CSR form).  A record with start >= end is not
// live: it covers nothing and joins nothing.
//
// RELIED ON: within a row `end` never decreases.  With sufmin(i) = the smallest start of a live record
// at index >= i in record i's row (+inf: none),
//   a live record i CLOSES a span iff sufmin(i + 1) == +inf or sufmin(i + 1) - end_i > gap,
//   index a OPENS a span iff (a is its row's first record or record a - 1 closes) and sufmin(a) < +inf,
// the k-th opener's sufmin is span k's start, the k-th closer's end is span k's end, and both have k closers before them.
// For other orders the same formulas are evaluated: memory-safe, at most n spans, not the union.
//
// All on the caller's stream, every index into the records, the rows and the outputs 64-bit (32-bit within a tile only),
// plain vector stores only, no workgroup waits for another:
//   1. k_span_tiles  a workgroup per tile of SPANS_TILE records: by binary search in rec_off the rows whose first record
//                    lies in the tile and where the row of the tile's first record ends; the tile's head -- the smallest
//                    live start among the tile's records in that first row -- and whether the tile's first record begins a
//                    row ("fresh") and whether the whole tile lies in one row ("whole")
//   2. k_span_carry  ONE workgroup over the T tile heads from the last tile to the first, SPANS_CARRY_THREADS *
//                    SPANS_CARRY_PER at a step: a reverse segmented min-scan; carry[t] = the smallest live start of tile t's last row among the records
//                    of LATER tiles (+inf: none), chained through tiles that lie wholly in one row
//   3. k_span_count  a workgroup per tile: marks the row starts in LDS, the reverse segmented min inside the tile (in the
//                    thread, across the wave's lanes, across the waves through LDS) seeded with carry[t], the close flags,
//                    one u64 count of closers per tile
//   (replace_scan over the counts is the host's: its total S crosses the bus, the outputs are sized by it)
//   4. k_span_emit   step 3 again (the flags are recomputed, never stored), the closers ranked within the tile: `end` at
//                    base[t] + rank, sufmin at the opener's rank, row_offsets[h] for every row whose rec_off[h] lies in the
//                    tile (the last tile: rec_off[h] == n as well, row_offsets[rows] = S).  Every index is compared with S
//                    before its store.
// Of each record the start and end words are loaded (8-byte alignment is enough).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/acx.h"

namespace acx {

// STARTING SIZES, NOT MEASURED ONES.  A workgroup of SPANS_THREADS threads takes one tile of
// SPANS_TILE records: SPANS_TILE / SPANS_THREADS = 4 consecutive records per thread.  LDS per workgroup of k_span_count /
// k_span_emit: one 4-byte word per slot (the row-start marks, then the closers' ranks: 4 KiB) and the waves' carries (under
// 128 bytes) -- 4.2 KiB, so the 160 KiB of a CU never bound the eight workgroups of 256 threads its wave slots hold.
// k_span_carry: 12 bytes per thread, 12 KiB, one workgroup in all, SPANS_CARRY_PER consecutive tiles per thread.  One
// workgroup per tile: there is no maximal grid, the host refuses 2^31 tiles (2^41 records) or more; k_span_carry then makes
// 2^19 steps -- it was sized for the 2^15 tiles (8 steps) of 2^25 records, a 1 GiB batch with a match every 32 bytes.
constexpr uint32_t SPANS_THREADS = 256;
constexpr uint32_t SPANS_TILE = 1024;
constexpr uint32_t SPANS_CARRY_THREADS = 1024;
constexpr uint32_t SPANS_CARRY_PER = 4;

// tiles of n records
uint64_t spans_tiles(uint64_t n);
// u64 words of scratch spans_count / spans_emit need for n records (five per tile)
uint64_t spans_temp_words(uint64_t n);
// m: n records (n > 0); rec_off: rows + 1 entries from 0 to n (rows > 0; the caller's word: a kernel reads records by
// them); temp: spans_temp_words(n) words, kept for spans_emit; counts: spans_tiles(n) words, the closers of every tile.
hipError_t spans_count(const acx_match_t *m, uint64_t n, const int64_t *rec_off, uint64_t rows, uint64_t gap, uint64_t *temp,
                       uint64_t *counts, hipStream_t st);
// base: the exclusive scan of counts (spans_tiles(n) + 1 entries), S = base[tiles]; start, end: S words each; row_off:
// rows + 1 words, or null (no row offsets wanted).  Nothing is stored at or behind index S.
hipError_t spans_emit(const acx_match_t *m, uint64_t n, const int64_t *rec_off, uint64_t rows, uint64_t gap, const uint64_t *temp,
                      const int64_t *base, uint64_t S, int64_t *row_off, int64_t *start, int64_t *end, hipStream_t st);

} // namespace acx
