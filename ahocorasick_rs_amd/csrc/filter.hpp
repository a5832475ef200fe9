// filter.hpp -- launch wrappers of the row-filter kernels in filter.hip (acx_filter_device / acx_filter_rows_device).
//
// A batch of n rows in HBM -- `len` bytes at hay, cut by offsets (n + 1 of them from 0), by uniform_len, or one row -- and
// counts[h] matches per row become the COMPACTED batch of the kept rows: row h is kept iff (counts[h] >= min_matches) ==
// keep_matched.  rows (k source row indexes, ascending), offsets (k + 1 words from 0) and data (the kept rows' bytes back
// to back).  All on the caller's stream, every offset and size 64-bit (32-bit indexes within a tile only), vector stores:
//   1. filter_flags    klen[h] = kept ? the row's length : 0, kflag[h] = kept (u64 words, one thread per row)
//   2. replace_scan (replace.hpp) over klen and over kflag: A[0 .. n] the byte prefix (A[n] = the output's bytes), B[0 .. n]
//                      the rank prefix (B[n] = k).  The host reads the two totals back and sizes the result.
//   3. filter_index    a kept row h of rank r = B[h]: rows[r] = h, offsets[r] = A[h], src[r] = where h begins in hay;
//                      offsets[k] = A[n]
//   4. filter_gather   output side: a workgroup per FILTER_TILE output bytes, 16-byte stores; every chunk is taken from hay
//                      at its row's shift (src[r] - offsets[r]).  k == 0 or no bytes: nothing is launched.
// hay may lie at any byte address; no load touches a byte outside [hay, hay + len).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "stage_device.hpp"

namespace acx {

// STARTING SIZES, NOT MEASURED ONES.  A workgroup of FILTER_THREADS threads writes one tile of
// FILTER_TILE output bytes: FILTER_TILE / 16 / FILTER_THREADS = 4 chunks of 16 bytes per thread, chunk c of thread t at
// 16 * (c * FILTER_THREADS + t) -- a wave's 64 stores of one c are 1 KiB of whole lines.  The kept rows that touch the tile
// are staged in LDS FILTER_WIN at a time (16 bytes each: output start and source shift, 16 KiB per workgroup).  One
// workgroup per tile: there is no maximal grid, the host refuses an output of 2^31 tiles (32 TiB) or more.
constexpr uint32_t FILTER_THREADS = 256;
constexpr uint32_t FILTER_TILE = 16384;
constexpr uint32_t FILTER_WIN = 1024;

// R: the input's rows (stage_device.hpp).  klen, kflag: n words each.  n == 0: nothing is launched.
hipError_t filter_flags(const RowCut &R, const uint64_t *counts, uint64_t min_matches, bool keep_matched, uint64_t *klen,
                        uint64_t *kflag, hipStream_t st);
// A, B: the scans' n + 1 entries; rows: k words, offsets: k + 1 words, src: k words (k = B[n]).  n == 0: nothing is launched.
hipError_t filter_index(const RowCut &R, const int64_t *A, const int64_t *B, int64_t *rows, int64_t *offsets, uint64_t *src,
                        hipStream_t st);
// u64 words of scratch filter_gather needs for an output of `total` bytes (the rows of every output tile)
uint64_t filter_tile_words(uint64_t total);
// out: round_up(total, 16) bytes, 16-byte aligned (the bytes behind `total` are written as zeros); hay: `len` readable bytes
// at any address; offsets: k + 1, src: k (what filter_index wrote); tiles: filter_tile_words(total) words
hipError_t filter_gather(const uint8_t *hay, uint64_t len, const int64_t *offsets, const uint64_t *src, uint64_t k,
                         uint64_t *tiles, uint8_t *out, uint64_t total, hipStream_t st);

} // namespace acx
