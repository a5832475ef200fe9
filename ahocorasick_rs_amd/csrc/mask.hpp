// mask.hpp -- launch wrappers of the cover kernels in mask.hip (acx_mask_device / acx_mask_rows_device).
//
// A batch's find result in HBM -- records m[0 .. n) of 24 bytes, ordered by haystack ("row"), and rec_off[0 .. rows], where
// every row's records begin (replace_scan over the per-row counts) -- and the rows' places in the byte stream (device offsets,
// a uniform length, or one row of `len` bytes) become the cover of the matches:
//   byte i of row h is covered iff some record of row h has start' <= i < end', with end' = min(end, row length) and
//   start' = min(start, end'): a record is clipped to its own row first, whatever it says, and an empty one covers nothing;
//   out[off[h] + i] = fill where covered, and is left as it is elsewhere.
// What `out` holds elsewhere is the caller's choice, made BEFORE the paint on the same stream: a copy of the haystack, zeros
// (the 0 / 1 mask), or -- in place -- the haystack itself.  One pass over the records, O(n + rows + covered bytes).  All on
// the caller's stream, every index into the records, the rows and the bytes 64-bit (32-bit within a tile only), plain vector
// stores only:
//   1. k_mask_tiles   per tile of MASK_TILE records: the row that holds its first record and the row that holds its last one,
//                     by binary search in rec_off
//   2. k_mask_paint   a workgroup per tile: marks the tile's non-empty row starts in LDS, gives every record the row it lies in
//                     (a running maximum over the marks: in the thread, across the wave's lanes, across the waves through
//                     LDS), clips it and stores `fill` over its bytes -- single bytes up to the first 16-byte boundary of
//                     `out` and behind the last one, aligned 8 / 4 / 2-byte pieces where fewer than 16 remain, aligned
//                     16-byte stores between.  No store is wider than what lies inside [start', end') at its address: `out`
//                     needs no alignment and no byte beyond `len` is written.  A record of MASK_LONG bytes or more is listed
//                     in LDS instead, and all the workgroup's threads sweep the listed ones 16 bytes per lane.
// EVERY WRITER STORES THE SAME VALUE: two records that overlap, in one tile or in two, need no order and no atomic.  The first
// order that matters is the stream's: the copy or the clear is complete before the paint begins.
// The records need 8-byte alignment only: of each one the start and end words are loaded.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/acx.h"
#include "stage_device.hpp"

namespace acx {

// STARTING SIZES, NOT MEASURED ONES (DESIGN.md section 18 has no table yet).  A workgroup of MASK_THREADS threads paints one
// tile of MASK_TILE records: MASK_TILE / MASK_THREADS = 4 records per thread.  A record shorter than MASK_LONG bytes is its
// thread's own; a longer one is swept by the workgroup, MASK_THREADS * 16 bytes at a step.  LDS per workgroup: the row of
// every row start (8 bytes per slot, 8 KiB), the slot of every record's row start (4 bytes, 4 KiB), the list of long records
// (16 bytes each, 16 KiB) and the waves' carries -- 28 KiB, five workgroups to a CU's 160 KiB.  One workgroup per tile:
// there is no maximal grid, the host refuses 2^31 tiles (2^41 records) or more.
constexpr uint32_t MASK_THREADS = 256;
constexpr uint32_t MASK_TILE = 1024;
constexpr uint32_t MASK_LONG = 512;

// u64 words of scratch mask_paint needs for n records (two rows per tile)
uint64_t mask_tile_words(uint64_t n);
// out: `len` writable bytes of any alignment; m: n records; rec_off: R.n + 1 entries from 0 to n (the caller's word: a
// kernel reads records by them); tiles: mask_tile_words(n) words.  Offsets that do not rise, or pass len, paint less: every
// store lies inside [0, len).  n == 0, R.n == 0 or len == 0: nothing is launched.
hipError_t mask_paint(const acx_match_t *m, uint64_t n, const int64_t *rec_off, const RowCut &R, uint8_t fill, uint64_t *tiles,
                      uint8_t *out, hipStream_t st);
// o[h] = where row h begins for h = 0 .. R.n (R.n + 1 int64 words, the last one len): the offsets a result carries
// beside its bytes
hipError_t mask_offsets(const RowCut &R, int64_t *o, hipStream_t st);

} // namespace acx
