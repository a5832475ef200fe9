// snippets.hpp -- launch wrappers of the snippet kernels in snippets.hip (acx_snippets_device / acx_snippets_rows_device).
//
// A batch's find result in HBM -- records m[0 .. n) of 24 bytes, ordered by haystack ("row"), and rec_off[0 .. rows], where
// every row's records begin (replace_scan over the per-row counts) -- and the caller's own bytes become one snippet per
// record: the record's bytes and up to `context` bytes on each side, clipped to the row.  THE DEFINITION, for a record
// (p, s, e) in a row of L bytes B (row-local byte offsets):
//   s' = min(s, L);  e' = min(max(e, s'), L)                        any record is memory-safe
//   lo = s' - min(s', context);  hi = e' + min(context, L - e')     no sum can wrap
//   SNIP_UTF8 only:  up to 3 times: if lo < s' and B[lo] in 0x80..0xBF: lo += 1
//                    up to 3 times: if e' < hi < L and B[hi] in 0x80..0xBF: hi -= 1
//   snippet = B[lo:hi];  lead = s' - lo
// The trim moves the ends INWARD to a character boundary and never into the match; three steps bound it for invalid UTF-8.
//
// All on the caller's stream, every index into the records, the rows, the input and the output 64-bit (32-bit within a tile
// only), plain vector stores only, no atomic, no workgroup waits for another:
//   1. k_snip_sizes   one thread per record: its row by binary search in rec_off -- one thread finds the rows of the tile's
//                     first and last record, every thread searches between the two -- the definition, len[i], src[i]
//                     (where the snippet begins in hay: row begin + lo), lead[i], pattern[i].  The trim reads at most 6
//                     bytes of hay.
//   (replace_scan over len is the host's: offsets[0 .. n]; its last entry, the output's bytes, crosses the bus)
//   2. k_snip_tiles   per tile boundary of the OUTPUT the segments that begin at or before it and before it
//   3. k_snip_gather  a ragged gather for SHORT segments, output side: a workgroup per SNIP_TILE output bytes, the segments
//                     that touch the tile staged in LDS SNIP_WIN at a time; a thread owns one 16-byte output chunk, walks the
//                     segments that intersect it and makes ONE aligned 16-byte store.  A piece of 4 bytes or more is
//                     fetched with aligned 4-byte loads and a funnel shift, a shorter one byte by byte.
// hay may lie at any byte address; no load touches a byte outside [hay, hay + len), no store a byte at or behind `total`.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/acx.h"
#include "stage_device.hpp"

namespace acx {

// STARTING SIZES, NOT MEASURED ONES.  A workgroup of SNIP_THREADS threads writes one tile of
// SNIP_TILE output bytes: SNIP_TILE / 16 / SNIP_THREADS = 1 chunk of 16 bytes per thread, thread t's at 16 * t -- a wave's 64
// stores are 1 KiB of whole lines.  The segments that touch the tile are staged in LDS SNIP_WIN at a time (16 bytes each:
// output start and source shift, 8 KiB per workgroup): a tile of 32-byte snippets holds 128 of them, one of 1-byte segments
// SNIP_TILE (rounds), and any number of empty ones.  One workgroup per tile: the host refuses 2^31 tiles (8 TiB) or more.
constexpr uint32_t SNIP_THREADS = 256;
constexpr uint32_t SNIP_TILE = 4096;
constexpr uint32_t SNIP_WIN = 512;

constexpr uint32_t SNIP_UTF8 = 1; // ACX_SNIPPET_UTF8: the ends move inward to a character boundary

// R: the input's rows (stage_device.hpp); a row's begin and end are clamped to len before a byte is read by them.
// m: n records (0 < n < 2^39); rec_off: R.n + 1 entries from 0 to n (R.n > 0); seg_len, src: n words each; lead, pattern: n
// words each.
hipError_t snip_sizes(const acx_match_t *m, uint64_t n, const int64_t *rec_off, const RowCut &R, const uint8_t *hay,
                      uint64_t context, uint32_t flags, uint64_t *seg_len, uint64_t *src, int64_t *lead, int64_t *pattern,
                      hipStream_t st);
// u64 words of scratch snip_gather needs for an output of `total` bytes (the segments of every output tile)
uint64_t snip_tile_words(uint64_t total);
// out: `total` bytes, 16-byte aligned; hay: `len` readable bytes at any address; offsets: n + 1 (the scan of seg_len), src: n
// (segment i is hay[src[i] .. src[i] + offsets[i + 1] - offsets[i])); tiles: snip_tile_words(total) words.  total == 0 or
// n == 0: nothing is launched.
hipError_t snip_gather(const uint8_t *hay, uint64_t len, const int64_t *offsets, const uint64_t *src, uint64_t n, uint64_t *tiles,
                       uint8_t *out, uint64_t total, hipStream_t st);

} // namespace acx
