// at.hpp -- launch wrappers of the match-at kernels in at.hip (acx_match_at / acx_match_at_device):
// the crate's anchored search -- "does a pattern begin exactly HERE" -- for a list of positions or for every row start.
//
// THE DEFINITION.  Inputs: the handle's patterns P_i; the data h[0 .. len) (a case-insensitive handle compares every byte
// through fold_byte); anchors (p, L): a position and a limit with p <= L <= len.
//   * The candidates of an anchor: C(p, L) = { (i, e) : e = p + len(P_i), e <= L, h[p .. e) == P_i }.  Empty patterns do not
//     exist (ACX_EEMPTY), so p == L has no candidate.
//   * Not overlapping, by the handle's own match kind: one (pattern, end) per anchor, or (-1, -1) when C is empty --
//       Standard         the smallest e, then the smallest i (the crate reports at the first match state)
//       LeftmostFirst    the smallest i                      (re.match of the alternation P_0|P_1|...)
//       LeftmostLongest  the largest e, then the smallest i
//   * Overlapping (Standard handles only): all of C, ordered by e ascending, then i ascending -- a CSR over the anchors.
//   * FULL (row starts only): C is first restricted to e == L -- the row equals the pattern.  All candidates then share e,
//     so every kind reports the smallest i.
// On the trie this is a walk from the root at h[p] along goto edges only -- never a failure link -- while bytes remain below
// L.  At every state with the OWN bit the state's first own pattern is the candidate of that depth: own1, or
// own_pid[own_off[s]] when own1 says "many" (the lists are in id order; the leftmost kinds keep only the first of identical
// patterns in them, automaton.cpp -- exactly "the smallest i").
// ROWS.  One haystack: L = len.  Data cut by offsets, a row length or neither (RowCut, stage_device.hpp): the row of p is the
// LAST row r with row_begin(r) <= p and L = row_begin(r + 1) -- of several rows with one start all but the last are empty; a
// match never crosses a row.  Row starts (AT_ROW_STARTS): the anchors ARE the rows, p = row_begin(r), L = row_begin(r + 1),
// one result per row, and `end` is local to the row: the length of the match.  Otherwise `end` is a position in the data.
// POSITIONS are the caller's word, as offsets and token boundaries are: one outside [0, len) -- a negative one is a large one
// -- has no candidate: (-1, -1), no entries.  L is clamped to len before a byte is read, a row index into [0, rows) before an
// offset is read: nothing outside the data is read and nothing outside the outputs is written.  Positions need not be sorted
// and may repeat.
//
// THE KERNEL, one template in three modes, all on the caller's stream; 64-bit indexes into positions and data (32-bit within
// a tile), plain vector stores, no atomics on global memory:
//   A. every thread takes AT_TILE / AT_THREADS anchors of its workgroup's tile, AT_THREADS apart (the positions are read by
//      coalesced 8-byte loads): position, limit (two words of the offsets, a multiplication, or count_le over the offsets),
//      the first byte through root_next -- 1 KiB copied to LDS.  Most anchors die there.  The survivors' slots are compacted
//      into a list in LDS (walk_push, at_walk.hpp: a ballot per wave, one LDS atomic per wave).
//   B. the threads take survivors from the list, so that the walking lanes are dense: children of s are the ids
//      [first_child[s], first_child[s + 1]) with in_byte ascending -- a linear probe up to AT_PROBE children, a binary search
//      beyond (a root-like node has up to 256); haystack bytes by byte loads, folded in the load for a case-insensitive
//      handle (no folded copy of the data is made, the caller's memory is never written).  The result goes to the slot in LDS.
//   C. every thread stores its own anchors' results, coalesced: every entry of the outputs is written by exactly one thread.
// at_walk: pattern and end.  Overlapping takes two passes: at_count (the own patterns on the path, a word per anchor), the
// library's scan (replace_scan), the total -- 8 bytes -- crosses the bus so that the result can be allocated, and at_emit
// walks again and stores each anchor's entries from its base, in the order of the definition, never past the next base.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/acx.h"
#include "device_types.hpp"
#include "stage_device.hpp"

namespace acx {

// STARTING SIZES, NOT MEASURED ONES.  A workgroup of AT_THREADS threads takes one tile of AT_TILE
// anchors, AT_TILE / AT_THREADS = 4 per thread in phases A and C; in phase B a thread walks every AT_THREADS-th survivor.
// LDS per workgroup: root_next (1 KiB), the positions (8 bytes per slot, 8 KiB), the limits / matched lengths (4 KiB), the
// depth-1 states / results (4 KiB), the survivor list (2 bytes per slot, 2 KiB) -- 19 KiB, eight workgroups to a CU's 160 KiB.
// Phase A tests ONE byte: the 64 Kibit depth-2 bitmap is not built (not measured whether it pays).  Measured: the survivor
// list against every thread walking its own anchors -- 1.35 to 1.86 times faster with a position every 64 / 16 / 4 bytes
// of 1 GiB (profiles/r20/match_at_compaction_ab.jsonl).
constexpr uint32_t AT_THREADS = 256;
constexpr uint32_t AT_TILE = 1024;
constexpr uint32_t AT_PROBE = 8;                 // children up to which a node is probed linearly
constexpr uint64_t AT_MAX_ANCHORS = 1ull << 32;  // the grid and the tiles index anchors with 32 bits

// kernel flags (the C ABI's ACX_AT_FULL / ACX_AT_ROW_STARTS, and whether the handle folds)
constexpr uint32_t AT_FULL = 1, AT_ROW_STARTS = 2, AT_FOLD = 4;

// the trie and the own lists of a handle, as the kernels take them (always present in DevAutomaton)
struct AtTrie {
    const uint32_t *first_child, *root_next, *own_off, *own_pid, *own1;
    const uint8_t *in_byte, *sflags;
};
inline AtTrie at_trie(const DevAutomaton &D) {
    return AtTrie{D.first_child, D.root_next, D.own_off, D.own_pid, D.own1, D.in_byte, D.sflags};
}

// hay: R.len readable bytes (any address; null when R.len == 0); pos: A int64 words, 8-byte aligned (ignored with
// AT_ROW_STARTS: A == R.n); 0 < A < AT_MAX_ANCHORS; kind: ACX_MATCH_*.
// pattern, end: A int64 words each, 8-byte aligned; every entry is written.
hipError_t at_walk(const AtTrie &T, const uint8_t *hay, const RowCut &R, const int64_t *pos, uint64_t A, int kind, uint32_t flags,
                   int64_t *pattern, int64_t *end, hipStream_t st);
// counts: A words; every entry is written
hipError_t at_count(const AtTrie &T, const uint8_t *hay, const RowCut &R, const int64_t *pos, uint64_t A, uint32_t flags,
                    uint64_t *counts, hipStream_t st);
// base: A + 1 words, the scan of at_count's counts over the SAME inputs; pattern, end: base[A] words each.  Anchor i writes
// entries base[i] .. base[i + 1] - 1 and never one at or past base[i + 1]
hipError_t at_emit(const AtTrie &T, const uint8_t *hay, const RowCut &R, const int64_t *pos, uint64_t A, uint32_t flags,
                   const int64_t *base, int64_t *pattern, int64_t *end, hipStream_t st);

// The row offsets of a result whose pieces lie in data order (the segmenter's, WordPiece's): row_offsets[r], r = 0 .. R.n, is
// count_lt(starts, total, row_begin(r)) clamped into [0, total], the last one total.  starts: total ascending int64 words
// (none read when total == 0); row_offsets: R.n + 1 words, 8-byte aligned; R.n < 2^38.  One kernel, a thread per entry.
hipError_t piece_rows(const RowCut &R, const int64_t *starts, uint64_t total, int64_t *row_offsets, hipStream_t st);

} // namespace acx
