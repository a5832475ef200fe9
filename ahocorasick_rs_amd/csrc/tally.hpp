// tally.hpp -- launch wrappers of the tally kernels in tally.hip (acx_tally / acx_tally_device / acx_tally_rows_device).
//
// A batch's find result in HBM -- records m[0 .. n) of 24 bytes, ordered by haystack ("row") and then by the search's
// order, and counts[h] records per row -- becomes the CSR form of C[h][p] = the number of row h's records with pattern p:
// row_offsets (rows + 1 words from 0), pattern (nnz words, strictly ascending within a row) and count (nnz words >= 1).
// All on the caller's stream, every index into the records, the rows and the outputs 64-bit:
//   1. replace_scan (replace.hpp) over the counts: rec_off[0 .. rows], where every row's records begin
//   2. tally_tiles     rows of at most row_max records: a segmented sort and run-length count through LDS; a row's runs go
//                      to two temporaries of n words at rec_off[h] + the run's rank in the row, their number to nnz_row[h].
//                      *n_long receives the records of the rows that are longer (0: there is none)
//   3. tally_long      those rows, when there are any: 64-bit keys (rank among the long rows) << 24 | pattern, gathered,
//                      sorted by rocprim::radix_sort_keys, run-length counted into the same temporaries and nnz_row
//   4. replace_scan over nnz_row: row_offsets, its last entry = nnz
//   5. tally_compact   tmp[rec_off[h] + j] -> out[row_offsets[h] + j] for j < nnz_row[h]
// The records need 8-byte alignment only.  Pattern ids are below 2^TALLY_PATTERN_BITS (a handle has no more).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/acx.h"

namespace acx {

// STARTING SIZES, NOT MEASURED ONES (DESIGN.md section 15 has no table yet).  A workgroup of TALLY_THREADS threads turns a
// tile of TALLY_TILE records per pass of its grid-stride loop.  It owns the rows that BEGIN in its tile; such a row of at
// most TALLY_ROW_MAX = TALLY_TILE records may run past the tile's end, so up to 2 * TALLY_TILE - 1 keys are staged: 16 KiB
// of 32-bit keys or 32 KiB of 64-bit keys, and 1.4 KiB beside them (row-start and long-row bitmaps, scan scratch).  Four
// workgroups of the 64-bit form share a CU's 160 KiB (five would, were it not for those 1.4 KiB); TALLY_MAX_GRID = 256 CUs
// x 4 is every workgroup of the wider form resident at once.
constexpr uint32_t TALLY_THREADS = 256;
constexpr uint32_t TALLY_TILE = 2048;
constexpr uint32_t TALLY_MAX_GRID = 1024;
constexpr uint32_t TALLY_ROW_MAX = TALLY_TILE;
constexpr uint32_t TALLY_PATTERN_BITS = 24;

// the tile kernel sorts 32-bit keys when log2(TALLY_TILE) + bits(n_patterns - 1) <= 32, 64-bit keys otherwise
bool tally_keys32(uint64_t n_patterns);
// the grid tally_tiles launches for n records (the host asserts that no workgroup of it makes 2^32 passes)
uint32_t tally_tiles_grid(uint64_t n);
// nnz_row (rows words) and *n_long (one word) must be zero on the stream before this.  n == 0: nothing is launched.
// row_max <= TALLY_ROW_MAX.  tmp_pattern, tmp_count: n words each.
hipError_t tally_tiles(const acx_match_t *m, uint64_t n, const int64_t *rec_off, uint64_t rows, uint64_t n_patterns,
                       uint32_t row_max, int64_t *tmp_pattern, int64_t *tmp_count, uint64_t *nnz_row, uint64_t *n_long,
                       hipStream_t st);
// u64 words of scratch tally_long needs for n_long records of long rows among `rows` rows
uint64_t tally_long_words(uint64_t rows, uint64_t n_long, uint32_t row_max);
// n_long: what tally_tiles counted for the same arguments, read back by the host (> 0)
hipError_t tally_long(const acx_match_t *m, const int64_t *rec_off, uint64_t rows, uint32_t row_max, uint64_t n_long,
                      uint64_t *scratch, int64_t *tmp_pattern, int64_t *tmp_count, uint64_t *nnz_row, hipStream_t st);
// nnz == 0: nothing is launched.  The outputs must not overlap the temporaries.
hipError_t tally_compact(const int64_t *row_offsets, uint64_t rows, const int64_t *rec_off, uint64_t nnz,
                         const int64_t *tmp_pattern, const int64_t *tmp_count, int64_t *pattern, int64_t *count,
                         hipStream_t st);

} // namespace acx
