// words.hpp -- launch wrappers of the whole-word kernels in words.hip (acx_words_rows_device, acx_find_words_device,
// acx_filter_words_device; DESIGN.md section 22 has the definition).
//
// A batch's OVERLAPPING find result in HBM -- records m[0 .. n) of 24 bytes, ordered by haystack ("row") and within a row by
// end, then longer first, then pattern; rec_off[0 .. rows], where every row's records begin -- and the caller's own bytes with
// their row cut become the whole-word records: those whose neighbour bytes inside the row are no word bytes, and of those
// (overlapping = 0) the ones the match kind picks.  A record with start >= end or end beyond its row is never whole.
//
// All on the caller's stream, record and row indexes 64-bit (32-bit within a tile), plain vector stores only, no workgroup
// waits for another:
//   1. words_test     a workgroup per tile of WORDS_TILE records: the tile's first and last row by binary search in rec_off,
//                     every record's row by a search between the two, two one-byte loads per record; flag[i] = whole
//   2. words_compact  count (a word per tile), replace_scan over the counts, emit: the flagged items to base[t] + rank and
//                     new_off[h] = the flagged items before rec_off[h] for the rows whose rec_off[h] lies in the tile.
//                     Its total crosses the bus (the caller sizes what follows by it).
//   overlapping: done.  Otherwise, on the survivors S[0 .. n1) -- rows off1 -- with GLOBAL positions gs = (where the row
//   begins) + start, ge = (where it begins) + end, so that rows never need a segment: every position of a later row is at or
//   beyond every position of an earlier one.
//   3. words_resolve  Standard: S is in key order (e, s, p).  A record begins an independent cluster when no survivor at or
//                     behind it starts before the previous survivor's end: sufmin(gs)[j] >= ge[j - 1], a reverse inclusive
//                     min-scan (rocprim, over a reversed copy).
//                     Leftmost kinds: rocprim::radix_sort_pairs on 64-bit keys, the value a record's 32-bit index in S.
//                       LeftmostFirst    one sort: key = gs << 24 | pattern, bits 0 .. 24 + bits(len)
//                       LeftmostLongest  two stable sorts: first by (len - (e - s)) << 24 | pattern (longer first, then
//                                        pattern), then by gs
//                     The limits: len < 2^38 bytes, n < 2^32 records (the host refuses both: ACX_ETOOBIG), pattern < 2^24
//                     (a record beyond it sets *err: ACX_ETOOBIG, never a wrong answer).  A record begins a cluster when
//                     its gs is not below the running maximum of the ge in front of it (one inclusive max-scan).
//                     Greedy: one thread per cluster head walks its cluster in key order, pos = 0; a record with gs >= pos
//                     is accepted and pos becomes its ge.  Clusters are a few records on text; one of any length is walked
//                     correctly by its one thread (its speed is no goal: DESIGN.md section 22).
//   4. words_compact  again, over the accepted flags in key order, with off1 as the rows.
// Of a record all three words are loaded (8-byte alignment is enough); the haystack may lie at any address.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/acx.h"
#include "stage_device.hpp"

namespace acx {

// STARTING SIZES, NOT MEASURED ONES.  A workgroup of WORDS_THREADS threads takes one tile of WORDS_TILE records, four per
// thread.  LDS: the emit pass keeps one 4-byte rank per slot (4 KiB) and the block scan's storage; the test pass 48 bytes.
constexpr uint32_t WORDS_THREADS = 256;
constexpr uint32_t WORDS_TILE = 1024;
constexpr uint32_t WORDS_PATTERN_BITS = 24;
constexpr uint64_t WORDS_MAX_LEN = 1ull << 38;     // bytes of a batch
constexpr uint64_t WORDS_MAX_RECORDS = 1ull << 32; // records of a call

// the 256-bit set as eight words: byte v is a word byte iff w[v >> 5] >> (v & 31) & 1 (the C ABI's 32 bytes, little-endian)
struct WordSet {
    uint32_t w[8];
};

uint64_t words_tiles(uint64_t n);

// flag[i] (a byte per record) = record i is a whole word of its row.  n > 0, rows > 0; rec_off: rows + 1 entries from 0 to n.
hipError_t words_test(const acx_match_t *m, uint64_t n, const int64_t *rec_off, uint64_t rows, const RowCut &R, const uint8_t *hay,
                      const WordSet &W, uint8_t *flag, hipStream_t st);

// counts[t] = the flagged items of tile t (words_tiles(n) words)
hipError_t words_count(const uint8_t *flag, uint64_t n, uint64_t *counts, hipStream_t st);

// Where words_emit puts what it keeps; every pointer may be null (not wanted).  rec: records; pattern / start / end: the same
// as int64 columns.
struct WordsOut {
    acx_match_t *rec;
    int64_t *pattern, *start, *end;
};
// base: the exclusive scan of words_count's counts (tiles + 1 entries), total = base[tiles].  Item i is record
// m[src ? src[i] : i]; the flagged ones go to out at base[t] + their rank in the tile (nothing at or behind `total`), and
// new_off[h] (rows + 1 words, or null) = the flagged items in front of item rec_off[h].
hipError_t words_emit(const uint8_t *flag, uint64_t n, const int64_t *base, uint64_t total, const uint32_t *src, const acx_match_t *m,
                      const WordsOut &out, const int64_t *rec_off, uint64_t rows, int64_t *new_off, hipStream_t st);

// counts[h] = off[h + 1] - off[h]
hipError_t words_row_counts(const int64_t *off, uint64_t rows, uint64_t *counts, hipStream_t st);

// The scratch of words_resolve for n1 survivors, in u64 words, and the bytes rocprim wants inside it.
struct ResolveLayout {
    uint64_t gs, ge, a, b, key0, key1, idx0, idx1, prim, words;
    size_t prim_bytes;
    explicit ResolveLayout(uint64_t n1);
};
// S: n1 survivors (0 < n1 < 2^32) in the overlapping find's order, off1 their rows (rows + 1 entries), R the bytes' cut
// (R.len < 2^38); kind: ACX_MATCH_*.  scratch: ResolveLayout(n1).words words.  acc[j] (a byte per survivor) = the record at
// place j of the key order is reported; *src = which survivor that is (null: j itself; else a part of the scratch).  *err (a
// device word the caller has zeroed) becomes 1 when a pattern does not fit the key.
hipError_t words_resolve(const acx_match_t *S, uint64_t n1, const int64_t *off1, uint64_t rows, const RowCut &R, int kind,
                         uint64_t *scratch, uint8_t *acc, const uint32_t **src, uint64_t *err, hipStream_t st);

} // namespace acx
