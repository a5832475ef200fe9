// tokens.hpp -- launch wrapper of the token-label kernels in tokens.hip (acx_tokens_device / acx_tokens_rows_device;
// DESIGN.md section 23).
//
// THE DEFINITION.  Inputs: a find's records m[0 .. n) of 24 bytes, ordered by haystack ("row"), with rec_off[0 .. rows] where
// every row's records begin (replace_scan over the per-row counts); the rows' places in the data (RowCut: device offsets, a
// uniform length, or one row of `len` positions); tokens t = 0 .. T - 1 given by two ascending arrays ts[t], te[t] with
// ts[t] <= te[t] <= ts[t + 1] -- GLOBAL positions in the unit of the row offsets (a partition by T + 1 boundaries `tok` is
// ts = tok, te = tok + 1).
//   * A record of row h (the row begins at b_h) is clipped to its row exactly as mask.hpp clips it: end' = min(end, row length),
//     start' = min(start, end').  Its global range is [g_s, g_e) = [b_h + start', b_h + end'); an empty one touches nothing.
//   * A record TOUCHES token t iff ts[t] < g_e and te[t] > g_s: a zero-length token strictly inside a match is touched, one on
//     a match's edge is not.
//   * The OWNER of token t is the touching record with the smallest index in the find's order -- whatever the schedule, also
//     for overlapping records and for two matches that share a token.
//   * pattern[t] (int64) is the owner's pattern, or -1; begin[t] (uint8) is 1 iff t has an owner and (t == 0 or token t - 1
//     has another owner or none), else 0: the B of BIO.  pattern >= 0 is the token mask.
//   * The token arrays are the caller's word, as row offsets are: nothing verifies that they rise.  The first and the last
//     touched token of every record are clamped into [0, T) BEFORE anything is stored: wrong arrays give wrong labels, never a
//     store outside the T-entry outputs (or the T owner words).
//
// For ascending arrays the touched tokens of a record are one range: first = count_le(te, T, g_s) (the tokens that end at or
// before g_s come before it), last = count_lt(ts, T, g_e) - 1.  All on the caller's stream, every index into the records,
// the rows and the positions 64-bit (32-bit within a tile; token indexes 32-bit: T < 2^32), plain vector stores and 64-bit
// global atomicMin only:
//   0. clear        owner[t] = all ones (8 bytes per token, the stage's temporaries): no owner
//   1. k_tok_tiles  per tile of TOK_TILE records the rows that hold its first and its last record (binary search in rec_off)
//   2. k_tok_own    a workgroup per tile: every record's row as k_mask_paint finds it (marks in LDS, a running maximum in the
//                   thread, across the wave, across the waves), the clip, g_s and g_e; the tile's smallest g_s and largest
//                   g_e (a reduction: under an overlapping find a tile's starts do not rise) are searched in ALL of te / ts
//                   by two threads, and every record searches only inside that bracket -- tens of KiB, so its probes hit L2
//                   instead of walking two 28-step searches into arrays of gigabytes; atomicMin(owner[t], record index)
//                   for every touched token.  A record that touches TOK_LONG tokens or more is listed in LDS instead, and
//                   all the workgroup's threads sweep the listed ones, a token per lane.
//   3. k_tok_label  a thread per four tokens: the owners by 16-byte loads (and the one before them), pattern[t] from the
//                   owner's record, begin[t] from owner[t - 1] != owner[t]; it reads owners and records only and writes the two
//                   columns: no neighbour's output is read.  The int64 column by 16-byte stores and the uint8 column by 4-byte
//                   words where the outputs' alignment allows, single entries at the tail.
// ORDER: atomicMin is commutative and associative -- the owner is the smallest touching index whichever workgroup comes first;
// the stream orders the clear before the atomics and the atomics before the labels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/acx.h"
#include "stage_device.hpp"

namespace acx {

// STARTING SIZES, NOT MEASURED ONES.  A workgroup of TOK_THREADS threads takes one tile of TOK_TILE
// records, TOK_TILE / TOK_THREADS = 4 per thread.  A record that touches fewer than TOK_LONG tokens is its thread's own; one
// that touches more is swept by the workgroup, TOK_THREADS tokens at a step.  LDS per workgroup: the row of every row start
// (8 bytes per slot, 8 KiB), the slot of every record's row start (4 bytes, 4 KiB), the list of long records (12 bytes each,
// 12 KiB), the waves' carries and the bracket -- 24 KiB, six workgroups to a CU's 160 KiB.
constexpr uint32_t TOK_THREADS = 256;
constexpr uint32_t TOK_TILE = 1024;
constexpr uint32_t TOK_LONG = 32;
constexpr uint64_t TOK_MAX_TOKENS = 1ull << 32; // token indexes are 32-bit in LDS and in the label kernel's grid

// u64 words of scratch tokens_label needs: the tiles' rows (two per tile), then the owners
uint64_t tokens_tile_words(uint64_t n);
uint64_t tokens_owner_words(uint64_t T);
// m: n records (n > 0); rec_off: R.n + 1 entries from 0 to n (the caller's word: a kernel reads records by them); ts, te: T
// words each (0 < T < TOK_MAX_TOKENS); tiles: tokens_tile_words(n) words; owner: tokens_owner_words(T) words, 16-byte aligned;
// pattern: T int64 words, 8-byte aligned; begin: T bytes at any address.  Every entry of both outputs is written.
hipError_t tokens_label(const acx_match_t *m, uint64_t n, const int64_t *rec_off, const RowCut &R, const int64_t *ts,
                        const int64_t *te, uint64_t T, uint64_t *tiles, uint64_t *owner, int64_t *pattern, uint8_t *begin,
                        hipStream_t st);

} // namespace acx
