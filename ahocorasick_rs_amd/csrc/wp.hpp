// wp.hpp -- launch wrappers of the WordPiece kernels in wp.hip (acx_wordpiece / acx_wordpiece_device):
// WordPiece tokenization by the dictionary -- the data is cut into words by a class per byte value, and every word into the
// vocabulary entries the handle's match kind prefers, continuation entries behind the first one; a word that cannot be cut
// completely is ONE unknown piece.
//
// THE DEFINITION.  Inputs: the handle's patterns P_i, the vocabulary exactly as a vocab.txt lists it -- whole-word entries as
// they are, continuation entries with the prefix; a continuation prefix C, any bytes, possibly empty (default "##"); the data
// h[0 .. len), cut into rows by RowCut (offsets, a row length, or neither); a class per byte VALUE, cls[256], one of WORD,
// SPACE (a separator: it belongs to no word and yields no piece) and ALONE (a byte that is a word by itself, such as
// punctuation); M = max_word_bytes, 1 <= M <= WP_MAX_WORD; unk_id, any int64.  A case-insensitive handle compares pattern
// bytes through fold_byte; cls is applied to the caller's raw byte.
// THE WORDS of a row [b, L): every ALONE byte is a word of one byte, every maximal run of WORD bytes inside the row is a word;
// a word never crosses a row.  Equivalently, p starts a word iff cls[h[p]] != SPACE and one of p == b, cls[h[p]] == ALONE,
// cls[h[p - 1]] != WORD holds.
// THE PIECES of a word [ws, we):
//   1. we - ws > M: the word is ONE piece (unk_id, ws, we).
//   2. Otherwise p = ws, and while p < we the candidates at p are
//        at p == ws  every (i, e) with e = p + len(P_i) <= we and h[p .. e) == P_i -- match_at's C(p, we), entries that
//                    begin with C included (the bare substring is looked up at a word start);
//        at p > ws   every (i, e) such that P_i begins with C, len(P_i) > len(C), e = p + len(P_i) - len(C) <= we and
//                    h[p .. e) == P_i[len(C):] -- a pattern equal to C itself is never a continuation piece.
//      One candidate is picked by the handle's own match kind, exactly as at.hpp states it: Standard the smallest e, then the
//      smallest i; LeftmostFirst the smallest i; LeftmostLongest the largest e, then the smallest i.  No candidate: the WHOLE
//      word is ONE piece (unk_id, ws, we) -- the pieces found before it are withdrawn.  Otherwise the piece is (i, p, e) and
//      p = e.
// With LeftmostLongest and the default classes this is WordpieceTokenizer.tokenize of BERT applied to text.split(), except
// that the word limit is counted in bytes.
// THE RESULT, four columns of T entries in data order: id (int64), start and end (int64 GLOBAL byte positions, start strictly
// ascending), first (uint8: 1 on the first piece of its word); and row_offsets, rows + 1 int64 words: entry r is the number
// of pieces that begin before row_begin(r).  There is no overlapping form.
// ROW OFFSETS on the device are the caller's word, as everywhere: wrong ones give wrong pieces, never a read outside [0, len)
// or a write outside the T, T, T, T and rows + 1 entries.
//
// THE KERNELS, all on the caller's stream; 64-bit positions in the data, 32-bit ones within a tile; plain vector stores, no
// atomics on global memory; no workgroup waits for another; every output entry is written by exactly one thread.  A
// workgroup of WP_THREADS takes a tile of WP_TILE bytes; a word belongs to the tile it STARTS in.
//   k_wp<COUNT>
//     A. every thread loads its 16 consecutive bytes (16-byte loads where the aligned 16 bytes lie inside the data, guarded
//        byte loads at the data's two ends) and classifies them through cls in LDS.  The row starts inside the tile are
//        marked in a bitmap in LDS (walk_row_marks<true> of at_walk.hpp: two bounded searches for offsets, the multiples for
//        a row length).  A BOUNDARY is a byte that is not WORD, or a row start.  The word-start flags are ranked in position
//        order (popcounts in the lane, then walk_rank: a scan across the wave, the waves' sums through LDS) and the word
//        starts go into a list in LDS: the walking lanes are dense and the list order is the output order.  A suffix minimum
//        of every thread's first boundary over the workgroup (walk_behind) gives every word start its end when that end lies
//        inside the tile.
//     B. the threads take words from the list.  A word with no boundary behind it in the tile (at most the tile's last one)
//        scans forward at most M + 1 bytes from its start, clamped to the row's end and len: that decides length > M.
//        Otherwise the lane walks the chain: the first step through root_next, continuation steps through cont_next -- the
//        children of C's trie node, 1 KiB filled once per workgroup by 256 at_child calls -- and after the first byte the
//        walk is at_best of at_walk.hpp (at_path with at_pick) unchanged: depths count haystack bytes, lim = we - p, the handle folds in
//        the load.  The word's piece count goes to LDS: 1 if the word is too long or any step finds nothing.
//     C. counts[tile] = the tile's pieces; bound[tile] = the position of the tile's first boundary, or "none".
//   replace_scan turns counts into bases; T crosses the bus: 8 bytes.
//   k_wp_carry  one workgroup: a suffix minimum of bound over the tiles from the last to the first (k_span_carry's shape):
//     carry[tile] = the first boundary at or behind the tile's end, clamped to len -- the true end of a word that runs out of
//     its tile, however long it is.  No lane ever scans more than M + 1 bytes.
//   k_wp<EMIT>  A and B again (as at_emit walks again); an exclusive scan of the words' piece counts over the workgroup gives
//     every word its base; the walking lane walks its word once more and stores id, start, end and first at
//     base .. base + n - 1, never at or behind T.
//   k_piece_rows  (at.hip, piece_rows) a thread per row: row_offsets[r] = count_lt(start, T, row_begin(r)), clamped into
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

// STARTING SIZES, NOT MEASURED ONES.  LDS per workgroup of k_wp: root_next and cont_next (1 KiB
// each), the classes (64 bytes), the word list, the words' ends and their piece counts (2 bytes per byte of the tile each,
// 24 KiB), EMIT: the words' bases (8 KiB), the row-start bitmap (512 bytes) -- 27 / 35 KiB, four workgroups to a CU's 160 KiB.
constexpr uint32_t WP_THREADS = 256;
constexpr uint32_t WP_TILE = 4096;      // bytes of data per workgroup
constexpr uint32_t WP_MAX_WORD = 1024;  // the largest max_word_bytes: a word's piece count and a tile's fit 16 bits
constexpr uint64_t WP_MAX_TILES = 0x7FFFFFFFull; // the grid indexes tiles with 32 bits
constexpr uint32_t WP_CARRY_THREADS = 256;
constexpr uint32_t WP_CARRY_PER = 8;    // consecutive tiles of one thread in a step of k_wp_carry
constexpr uint32_t WP_NO_NODE = 0xFFFFFFFFu; // C's path is not in the trie: no continuation ever matches

// the classes of the byte values (the C ABI's ACX_WP_WORD ..)
constexpr uint32_t WP_WORD = 0, WP_SPACE = 1, WP_ALONE = 2;
// kernel flags (whether the handle folds)
constexpr uint32_t WP_FOLD = 1;

// cls[256] packed for the kernel's arguments: two bits per byte value, 16 values to a word
struct WpClasses {
    uint32_t w[16];
};
inline WpClasses wp_classes(const uint8_t cls[256]) {
    WpClasses K{};
    for (uint32_t b = 0; b < 256; b++) K.w[b >> 4] |= (uint32_t)(cls[b] & 3u) << (2 * (b & 15));
    return K;
}

struct WpArgs {
    WpClasses cls;
    uint32_t cont_node; // the trie node of C (0: C is empty, the root), or WP_NO_NODE
    uint32_t max_word;  // M
    uint32_t flags;     // WP_FOLD
    int kind;           // ACX_MATCH_*
    int64_t unk_id;
};

// The scratch of one call, in u64 words: counts (a word per tile), bound and carry (a word per tile each), base (tiles + 1),
// and replace_scan's own.
struct WpPlan {
    uint64_t ntiles = 0, counts = 0, bound = 0, carry = 0, base = 0, scan = 0, words = 32;
};
WpPlan wp_plan(uint64_t len);

// hay: R.len readable bytes (any address), R.len > 0; scratch: P.words words, 8-byte aligned.  k_wp<COUNT>, the scan and the
// carry; afterwards (on st) T lies at wp_total(P, scratch).
hipError_t wp_count(const AtTrie &T, const uint8_t *hay, const RowCut &R, const WpArgs &A, const WpPlan &P, uint64_t *scratch,
                    hipStream_t st);
inline const uint64_t *wp_total(const WpPlan &P, const uint64_t *scratch) { return scratch + P.base + P.ntiles; }
// ... and from there, over the SAME inputs: k_wp<EMIT> and piece_rows.  total: what wp_total gave; id, start, end: total int64
// words, 8-byte aligned; first: total bytes; row_offsets: R.n + 1 words; every entry is written.
hipError_t wp_emit(const AtTrie &T, const uint8_t *hay, const RowCut &R, const WpArgs &A, const WpPlan &P, const uint64_t *scratch,
                   uint64_t total, int64_t *id, int64_t *start, int64_t *end, uint8_t *first, int64_t *row_offsets, hipStream_t st);

} // namespace acx
