// seg.hpp -- launch wrappers of the segmenter's kernels in seg.hip (acx_segment / acx_segment_device):
// greedy tokenization by the dictionary -- cut the data into dictionary entries from left to right, always the entry the
// handle's match kind prefers at the current position, and go on where it ended.  With LeftmostLongest this is MaxMatch
// (WordPiece's inner loop, forward maximum matching), with LeftmostFirst re.finditer of P_0|P_1|...|. .
//
// THE DEFINITION.  Inputs: the handle's patterns P_i and the data h[0 .. len), cut into rows by RowCut (offsets, a row length,
// or neither); a case-insensitive handle compares every byte through fold_byte.
// For a row [b, L) the pieces are built by a loop.  Start with p = b.  While p < L:
//   1. (i, e) = the non-overlapping match_at result of the anchor (p, L) under the handle's own match kind (at.hpp: Standard
//      the smallest e, LeftmostFirst the smallest i, LeftmostLongest the largest e) -- a match never crosses the row.
//   2. A match: the piece is (i, p, e), and p = e.
//   3. None: the piece is (-1, p, p + u), and p = p + u -- u is the UNKNOWN UNIT: 1 byte by default.  With SEG_UTF8, u is
//      the length the lead byte h[p] announces -- 2, 3, 4 for 0xC0..0xDF, 0xE0..0xEF, 0xF0..0xF7, and 1 for everything else, a
//      stray continuation byte included -- shortened to the run of continuation bytes (0x80..0xBF) that actually follows,
//      and clipped to L.
// The pieces of a row tile it exactly; an empty row has none; rows that rise from 0 to len give pieces that tile [0, len).
// THE RESULT, three parts: pattern (T int64 words: the pattern, or -1), offsets (T + 1 int64 words: the GLOBAL ascending
// piece boundaries, offsets[T] = len -- the token_offsets form of label_tokens_batch) and row_offsets (rows + 1 int64 words:
// entry r is the number of pieces that begin before row_begin(r), the last one T).  There is no overlapping form: the chain
// is defined by one choice per position.
// ROW OFFSETS on the device are the caller's word, as everywhere: wrong ones give wrong pieces, never a read outside [0, len)
// or a write outside the T, T + 1 and rows + 1 words.  The row of p ends at the smallest offset beyond p (clamped to len).
//
// THE KERNELS, all on the caller's stream; 64-bit positions in the data, 32-bit ones within a tile; plain vector stores, no
// atomics on global memory; no workgroup waits for another and no serial loop runs over all tiles:
//   k_seg<COUNT>  a workgroup per tile of SEG_TILE bytes.
//     A. step[q], pid[q] for EVERY byte q of the tile, in LDS: the row limit (the row starts behind the tile's first byte are
//        marked in a bitmap, every thread takes the first mark of its 16 bytes and a suffix minimum runs over the workgroup),
//        the first byte through root_next in LDS, the survivors compacted into a list, walked by dense lanes with the walk
//        of k_at -- it may read beyond the tile, up to the row's end.  The marks, the minimum, the list and the walk are
//        at_walk.hpp's: walk_row_marks<false>, walk_behind, walk_push, at_best.  step is the match length or u: at least 1, and
//        p + step never passes the row's end.
//     B. the ENTRY MAP: a chain that enters the tile lands at a tile offset e < E (E: the largest step -- max_pattern_len,
//        at least 4 with SEG_UTF8); the map says where in the next tile the chain from e lands and how many pieces it began
//        here.  It is read off a table of jumps over ALL positions of the tile: jump[q] = (hops, target) starts as one
//        step, and a round replaces it by the jump of its target on top of its own -- pointer jumping, in place: every word
//        is written by its owner alone and any word read is a true pair.  A round at least doubles every chain's hops: 13
//        rounds at most, each 16 independent LDS round trips per thread, instead of a chain of up to 4 096 dependent reads
//        in one lane.  An entry at or beyond len exits at once.
//   k_seg_compose  the up-sweep: maps [0, E) -> ([0, E), count) compose associatively.  A lane per entry folds SEG_FAN
//     consecutive child maps into the parent's -- SEG_FAN dependent steps; counts are 64-bit from level 1 on.  Levels repeat
//     until one map is left; T is its count at entry 0 -- 8 bytes cross the bus so that the result can be allocated.
//   k_seg_resolve  the down-sweep: from the root with entry 0 and base 0, a thread per parent gives every child its true
//     entry and the index of its first piece.
//   k_seg<EMIT>   phase A again (as at_emit walks again); the piece starts are the positions on the chain from the tile's
//     true entry: round k holds every position's 2^k-th successor (two 16-bit buffers swing), the flagged positions flag
//     theirs -- the flagged stretch of the chain doubles -- and the successors are squared; 13 rounds at most.  The
//     workgroup ranks the flags (popcounts in the lane, then walk_rank of at_walk.hpp: a scan across the wave, the waves'
//     sums through LDS) and stores offsets[base + rank] and pattern[base + rank]: every entry is written by exactly one
//     thread, none at or beyond T.  One thread stores offsets[T] = len.
//   k_piece_rows  (at.hip, piece_rows) a thread per row: row_offsets[r] = count_lt(offsets, T, row_begin(r)), clamped into
//     [0, T].
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/acx.h"
#include "at.hpp"
#include "device_types.hpp"
#include "stage_device.hpp"

namespace acx {

// STARTING SIZES, NOT MEASURED ONES.  LDS per workgroup of k_seg: root_next (1 KiB), step (2 bytes
// per byte of the tile, 8 KiB), pid (4 bytes, 16 KiB; COUNT: afterwards the jumps), the survivor list (2 bytes, 8 KiB; EMIT:
// afterwards the second buffer of the successors), the marks / flags bitmap (512 bytes) -- 33.8 KiB, four workgroups to a
// CU's 160 KiB.
constexpr uint32_t SEG_THREADS = 256;
constexpr uint32_t SEG_TILE = 4096;     // bytes of data per workgroup
constexpr uint32_t SEG_FAN = 64;        // child maps folded into one parent map
constexpr uint32_t SEG_MAX_STEP = 256;  // the longest pattern a handle may hold (ACX_ETOOBIG beyond): dictionary entries are words
constexpr uint64_t SEG_MAX_TILES = 0x7FFFFFFFull; // the grid indexes tiles with 32 bits
constexpr int SEG_MAX_LEVELS = 8;       // 64^6 > 2^31 tiles: the tree is at most 7 levels high

// kernel flags (the C ABI's ACX_SEG_UTF8, and whether the handle folds)
constexpr uint32_t SEG_UTF8 = 1, SEG_FOLD = 2;

// The scratch of one call, in u64 words of one block: the level-0 maps (a u32 per tile and entry: count << 16 | exit), per
// level l >= 1 the exits (u32) and counts (u64) of n[l] nodes, and per level the nodes' true entries (u32) and bases (u64).
struct SegPlan {
    uint64_t ntiles = 0;
    uint32_t E = 1;
    int levels = 0;                  // the root is level `levels` (>= 1 when ntiles > 0): n[levels] == 1
    uint64_t n[SEG_MAX_LEVELS] = {}; // nodes per level; n[0] = ntiles
    uint64_t map0 = 0;               // level 0: ntiles * E u32
    uint64_t exits[SEG_MAX_LEVELS] = {}, counts[SEG_MAX_LEVELS] = {}; // l >= 1: n[l] * E u32 / u64
    uint64_t entry[SEG_MAX_LEVELS] = {}, base[SEG_MAX_LEVELS] = {};   // l >= 0: n[l] u32 / u64
    uint64_t words = 0;
};
// len bytes and a handle whose longest pattern has max_len <= SEG_MAX_STEP bytes; ntiles <= SEG_MAX_TILES is the caller's check
inline SegPlan seg_plan(uint64_t len, uint32_t max_len, uint32_t flags) {
    SegPlan P;
    P.ntiles = tiles_of(len, SEG_TILE);
    P.E = max_len > 1 ? max_len : 1;
    if ((flags & SEG_UTF8) && P.E < 4) P.E = 4;
    Carver C;
    P.n[0] = P.ntiles;
    P.map0 = C.part((P.ntiles * P.E + 1) / 2);
    P.entry[0] = C.part((P.ntiles + 1) / 2);
    P.base[0] = C.part(P.ntiles);
    for (int l = 1; l < SEG_MAX_LEVELS && P.ntiles; l++) {
        P.n[l] = tiles_of(P.n[l - 1], SEG_FAN);
        P.exits[l] = C.part((P.n[l] * P.E + 1) / 2);
        P.counts[l] = C.part(P.n[l] * P.E);
        P.entry[l] = C.part((P.n[l] + 1) / 2);
        P.base[l] = C.part(P.n[l]);
        P.levels = l;
        if (P.n[l] == 1) break;
    }
    P.words = C.words();
    return P;
}

// hay: R.len readable bytes (any address), R.len > 0; scratch: P.words words, 8-byte aligned; kind: ACX_MATCH_*.
// k_seg<COUNT> and the up-sweep; afterwards (on st) T lies at seg_total(P, scratch).
hipError_t seg_count(const AtTrie &T, const uint8_t *hay, const RowCut &R, int kind, uint32_t flags, const SegPlan &P,
                     uint64_t *scratch, hipStream_t st);
inline const uint64_t *seg_total(const SegPlan &P, const uint64_t *scratch) { return scratch + P.counts[P.levels]; }
// ... and from there, over the SAME inputs: the down-sweep, k_seg<EMIT> and piece_rows.  total: what seg_total gave;
// pattern: total words, offsets: total + 1 words, row_offsets: R.n + 1 words, 8-byte aligned; every entry is written.
hipError_t seg_emit(const AtTrie &T, const uint8_t *hay, const RowCut &R, int kind, uint32_t flags, const SegPlan &P,
                    uint64_t *scratch, uint64_t total, int64_t *pattern, int64_t *offsets, int64_t *row_offsets, hipStream_t st);

} // namespace acx
