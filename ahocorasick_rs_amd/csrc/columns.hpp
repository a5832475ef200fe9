// columns.hpp -- launch wrapper of the split kernel in columns.hip (acx_find_columns / acx_find_columns_device,
// acx_split_device).
//
// A find result in HBM -- records m[0 .. n) of 24 bytes (pattern, start, end) -- becomes three columns of n 64-bit words where
// it lies: pattern[i] = m[i].pattern, start[i] = m[i].start, end[i] = m[i].end.  One pass on the caller's stream behind the
// find's write kernel, all indexes 64-bit.  The records and every column need 8-byte alignment only: a sub-range of a result
// that starts at an odd record, or a column that starts at an odd word, lies at 8 mod 16.
// The row offsets of a batch are not made here: they are the exclusive prefix of the result's per-haystack counts,
// replace_scan (replace.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/acx.h"

namespace acx {

// a workgroup turns COL_TILE records per pass of its grid-stride loop (one LDS tile: COL_TILE * 24 bytes), COL_THREADS
// threads each; at most COL_MAX_GRID workgroups are launched (columns.hip says where the numbers come from)
constexpr uint32_t COL_THREADS = 256;
constexpr uint32_t COL_TILE = 1024;
constexpr uint32_t COL_MAX_GRID = 1536;

// n == 0: nothing is launched.  The columns must not overlap the records or each other.
hipError_t col_split(const acx_match_t *m, uint64_t n, int64_t *pattern, int64_t *start, int64_t *end, hipStream_t st);
// the grid col_split launches for n records (the host asserts that no workgroup of it makes 2^32 passes)
uint32_t col_split_grid(uint64_t n);

} // namespace acx
