// rows.hpp -- launch wrappers of the row-cut kernels in rows.hip (acx_split_rows_device / acx_split_rows_into_device).
//
// `len` bytes in HBM and a delimiter byte d become the offsets that cut them into rows:
//   offsets = 0, then p + 1 for every p with hay[p] == d (ascending), then len if len > 0 and hay[len - 1] != d
// -- rows + 1 int64 words that rise strictly from 0 to len (one word, 0, for no bytes); every row but possibly the last
// ends with its delimiter and no row is empty.  Two passes over the input with the library's scan between them, ordered by
// the stream and by nothing else -- no workgroup waits for another:
//   1. rows_count     a workgroup per tile of ROWS_TILE bytes: the tile's delimiters as one u64 word; the last tile's
//                     workgroup also writes whether the input's last byte is the delimiter
//   2. replace_scan (replace.hpp) over the tile counts: base[t] = the delimiters before tile t, base[tiles] = their total.
//                     The host reads the total and the flag back -- 16 bytes, all that crosses the bus -- and sizes the result.
//   3. rows_write     reads the tile again, ranks every delimiter inside it (popcounts in the lane, a scan across the
//                     wave's lanes, the waves' sums through LDS) and stores position + 1 at offsets[1 + base[t] + rank]:
//                     plain 8-byte stores, no atomics.  One thread writes offsets[0] = 0 and, behind an unterminated last
//                     row, offsets[rows] = len.
// hay may lie at any byte address: the tiles are cut at 16-byte lines of the ADDRESS, every whole line inside the input is
// one aligned 16-byte load, and the first and the last line -- where the input covers a part only -- are read byte by byte:
// no load touches a byte outside [hay, hay + len).  Positions and tile bases are 64-bit, ranks within a tile 32-bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace acx {

// STARTING SIZES, NOT MEASURED ONES.  A workgroup of ROWS_THREADS threads reads one tile of ROWS_TILE
// bytes: ROWS_TILE / 16 / ROWS_THREADS = 4 lines of 16 bytes per thread, line k of thread t at 16 * (k * ROWS_THREADS + t)
// -- a wave's 64 loads of one k are 1 KiB of whole lines (filter.hpp's shape).  One workgroup per tile: there is no maximal
// grid, the host refuses an input of 2^31 tiles (32 TiB) or more.
constexpr uint32_t ROWS_THREADS = 256;
constexpr uint32_t ROWS_TILE = 16384;

// the tiles of `len` bytes at hay (by hay's place in its first 16-byte line: at most one more than len / ROWS_TILE rounded up)
uint64_t rows_tiles(const void *hay, uint64_t len);
// counts: rows_tiles words; *last: 1 when hay[len - 1] is the delimiter, else 0.  len == 0: nothing is launched.
hipError_t rows_count(const uint8_t *hay, uint64_t len, uint8_t delimiter, uint64_t *counts, uint64_t *last, hipStream_t st);
// base: the scan of the counts (rows_tiles + 1 entries, the last one `total`); offsets: rows + 1 words, rows = total +
// (unterminated ? 1 : 0).  No store goes behind offsets[rows], whatever the bytes say by now.  len == 0: nothing is launched.
hipError_t rows_write(const uint8_t *hay, uint64_t len, uint8_t delimiter, const int64_t *base, uint64_t total, bool unterminated,
                      int64_t *offsets, hipStream_t st);

} // namespace acx
