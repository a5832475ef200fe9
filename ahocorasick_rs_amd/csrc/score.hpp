// score.hpp -- launch wrappers of the row-score kernels in score.hip (acx_score_device / acx_score_rows_device and the
// hook of acx_filter_scored_device).
//
// A batch's find result in HBM -- records m[0 .. n) of 24 bytes, ordered by haystack ("row"), and rec_off[0 .. rows], where
// every row's records begin (replace_scan over the per-row counts) -- and one int32 weight per pattern become
//   score[h] = sum of weights[m[i].pattern] over row h's records, an int64 that wraps modulo 2^64;
// a record whose pattern is >= n_patterns adds nothing and never indexes the weights.  One pass over the records: O(n + rows).
// All on the caller's stream, every index into the records, the rows and the outputs 64-bit (32-bit within a tile only),
// vector stores only:
//   1. the score is cleared (an empty row's 0 is that zero)
//   2. k_score_tiles   per tile of SCORE_TILE records: the row that holds its first record and the row that holds its last
//                      one, by binary search in rec_off
//   3. k_score         a workgroup per tile: marks the tile's non-empty row starts in LDS, sums the weights of every row's
//                      records in the tile (a segmented sum: in the thread, across the wave's lanes, across the waves
//                      through LDS) and writes a row that lies wholly in the tile with one 8-byte store; a row that crosses
//                      a tile boundary -- at most two per tile -- is added with a 64-bit atomic.  Integer adds: the result
//                      does not depend on the order.
//   4. score_flags     flag[h] = score[h] >= min_score, a u64 word: what the row filter's stage takes as its counts
// The records need 8-byte alignment only: of each one the pattern word alone is loaded.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/acx.h"

namespace acx {

// STARTING SIZES, NOT MEASURED ONES (DESIGN.md section 17 has no table yet).  A workgroup of SCORE_THREADS threads sums one
// tile of SCORE_TILE records: SCORE_TILE / SCORE_THREADS = 8 consecutive records per thread.  LDS per workgroup: the
// records' weights (4 bytes each, 8 KiB), the row of every row start (8 bytes per slot, 16 KiB), the row-start bitmap and
// the waves' carries -- 24.3 KiB, six workgroups to a CU's 160 KiB.  One workgroup per tile: there is no maximal grid, the
// host refuses 2^31 tiles (2^42 records) or more.
constexpr uint32_t SCORE_THREADS = 256;
constexpr uint32_t SCORE_TILE = 2048;

// u64 words of scratch score_rows needs for n records (two rows per tile)
uint64_t score_tile_words(uint64_t n);
// score: rows words, cleared here; m: n records; rec_off: rows + 1 entries from 0 to n (the caller's word: a kernel reads
// records by them); weights: n_patterns int32 in device memory; tiles: score_tile_words(n) words.  rows == 0: nothing is
// launched; n == 0: the clear alone.
hipError_t score_rows(const acx_match_t *m, uint64_t n, const int64_t *rec_off, uint64_t rows, const int32_t *weights,
                      uint64_t n_patterns, uint64_t *tiles, int64_t *score, hipStream_t st);
// flag[h] = score[h] >= min_score ? 1 : 0 for h < rows.  rows == 0: nothing is launched.
hipError_t score_flags(const int64_t *score, uint64_t rows, int64_t min_score, uint64_t *flag, hipStream_t st);

} // namespace acx
