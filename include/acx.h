/*
 * acx.h -- C ABI of the MI355X-native Aho-Corasick matcher (libacx_hip.so).
 *
 * This is the drop-in boundary for the ONE hot path this project replaces:
 * the match loop behind `find_matches_as_indexes` of G-Research/ahocorasick_rs.
 * Every entry point cites the reference interface it replaces
 * (paths relative to the reference repository).  Plain pointers and sizes
 * only; no torch / Python types.  A Rust/PyO3 host would bind these with an
 * `extern "C"` block; this repository's host shim is the
 * C++ CPython extension ahocorasick_rs_amd/csrc/pymodule.cpp.
 *
 * All functions return ACX_OK (0) or a negative ACX_E* code; the message of
 * the last failure on the calling thread is available from acx_last_error().
 * There is NO CPU fallback: without a usable HIP device every matching call
 * fails with ACX_EDEVICE.
 */
#ifndef ACX_H
#define ACX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 11: acx_build_ex / acx_compile_host_ex (build flags: ACX_BUILD_ASCII_CASE_INSENSITIVE) added; acx_info_t gained `flags`;
 *     acx_path_stats gained [13];
 *     addendum (additive: the number stays, a binding written against 11 still loads): acx_summarize / acx_summarize_device /
 *     acx_summarize_host, ACX_SUM_FIRST / ACX_SUM_BY_PATTERN and the acx_summary_t accessors (acx_summary_total, _on_device,
 *     _counts, _any, _first, _by_pattern, _device_counts, _device_any, _device_first, _device_by_pattern, acx_free_summary);
 *     second addendum (additive as well): acx_find_columns / acx_find_columns_device, ACX_COL_*, the acx_columns_t accessors
 *     (acx_columns_count, _rows, _on_device, _data, _copy, acx_free_columns), acx_split_host / acx_split_device;
 *     third addendum (additive as well): acx_tally / acx_tally_device / acx_tally_host / acx_tally_rows_device, ACX_TALLY_*,
 *     the acx_tally_t accessors (acx_tally_nnz, _rows, _on_device, _data, _copy, acx_free_tally);
 *     fourth addendum (additive as well): acx_filter / acx_filter_device / acx_filter_host / acx_filter_rows_device,
 *     ACX_FILTER_KEEP_MATCHED, ACX_FILT_*, the acx_filtered_t accessors (acx_filtered_rows, _bytes, _on_device, _data, _copy,
 *     acx_free_filtered);
 *     fifth addendum (additive as well): acx_score / acx_score_device / acx_score_host / acx_score_rows_device, the
 *     acx_scores_t accessors (acx_scores_rows, _on_device, _data, _copy, acx_free_scores), acx_filter_scored /
 *     acx_filter_scored_device;
 *     sixth addendum (additive as well): acx_mask / acx_mask_device / acx_mask_host / acx_mask_rows_device, ACX_MASK_ZERO,
 *     the acx_masked_t accessors (acx_masked_bytes, _rows, _on_device, _data, _offsets, _copy, _copy_offsets,
 *     acx_free_masked);
 *     seventh addendum (additive as well): acx_split_rows / acx_split_rows_device / acx_split_rows_host /
 *     acx_split_rows_into_device and the acx_rows_t accessors (acx_rows_count, _bytes, _on_device, _device, _offsets, _copy,
 *     acx_free_rows);
 *     eighth addendum (additive as well): acx_spans / acx_spans_device / acx_spans_host / acx_spans_rows_device, ACX_SPAN_*,
 *     the acx_spans_t accessors (acx_spans_count, _rows, _on_device, _data, _copy, acx_free_spans);
 *     ninth addendum (additive as well): acx_snippets / acx_snippets_device / acx_snippets_host / acx_snippets_rows_device,
 *     ACX_SNIP_*, the acx_snippets_t accessors (acx_snippets_count, _rows, _nbytes, _on_device, _data, _copy,
 *     acx_free_snippets);
 *     tenth addendum (additive as well): whole-word matching -- acx_words_host / acx_words_rows_device, acx_find_words /
 *     acx_find_words_device (an acx_columns_t), acx_filter_words / acx_filter_words_device (an acx_filtered_t);
 *     eleventh addendum (additive as well): acx_tokens / acx_tokens_device / acx_tokens_host / acx_tokens_rows_device and the
 *     acx_token_labels_t accessors (acx_token_labels_count, _on_device, _pattern, _begin, _copy_pattern, _copy_begin,
 *     acx_free_token_labels);
 *     twelfth addendum (additive as well): the anchored search -- acx_match_at / acx_match_at_device /
 *     acx_match_at_into_device / acx_match_at_host and the acx_at_t accessors (acx_at_count, _entries, _on_device, _pattern,
 *     _end, _row_offsets, _copy, acx_free_at);
 *     thirteenth addendum (additive as well): greedy segmentation by the dictionary -- acx_segment / acx_segment_device /
 *     acx_segment_into_device / acx_segment_host and the acx_seg_t accessors (acx_seg_count, _rows, _on_device, _pattern,
 *     _offsets, _row_offsets, _copy, acx_free_seg);
 *     fourteenth addendum (additive as well): WordPiece tokenization by the dictionary -- acx_wordpiece /
 *     acx_wordpiece_device / acx_wordpiece_into_device / acx_wordpiece_host and the acx_wp_t accessors (acx_wp_count, _rows,
 *     _on_device, _id, _start, _end, _first, _row_offsets, _copy, acx_free_wp);
 * 10: acx_replace / acx_replace_device / acx_splice_host and the acx_replaced_t accessors added; acx_path_stats gained [12];
 * 9: acx_path_stats gained [10], [11] (round 6: launches of a context's resident K0; mid-size host haystacks read in place);
 * 8: acx_path_stats gained [9] (round 6: calls repeated with the wide form of the sparse path's post stage);
 * 7: acx_path_stats gained [8] (byte ranges of calls that were cut); K0's result line carries end - 1 and a hash of the
 *    matches beside it (round 5);
 * 6: acx_path_stats added (round 5);
 * 5: acx_host_tables_t grew (short-pattern tables), acx_device_synchronize_on, acx_comm_* added (round 4);
 * 4: acx_host_tables_t grew (walk_t3b / walk_t3r / walk_grec, round 3);
 * 3: acx_replicate / acx_find_batch_multi / acx_shard_range / acx_automaton_device added (round 3);
 * 2: acx_prefix_slot gained `salt`, acx_host_tables_t grew (round 2).  A binding built against another
 * header must refuse to load: compare acx_version() with the ACX_VERSION it was compiled with. */
#define ACX_VERSION 11

/* status codes */
#define ACX_OK 0
#define ACX_EINVAL (-1)      /* bad argument                                  */
#define ACX_EEMPTY (-2)      /* empty pattern (src/lib.rs:204-208, 386-389)   */
#define ACX_EOVERLAP (-3)    /* overlapping search on a non-Standard automaton:
                                the crate's MatchError -> ValueError,
                                src/lib.rs:36-39, 52-54                        */
#define ACX_ENOMEM (-4)
#define ACX_EDEVICE (-5)     /* HIP runtime / no device / kernel failure      */
#define ACX_ETOOBIG (-6)     /* automaton or haystack exceeds an encoding limit: 2^24 patterns, 2^30
                                states, a haystack stream of 2^38 bytes.  A ONE-haystack call that
                                would enumerate 2^32 occurrences or more in one pass (the width of the
                                device's indexes) is cut into byte ranges that are searched one after
                                the other (round 5; acx_path_stats [8]) -- the error remains for a
                                BATCH that does (cut it at a haystack boundary) and for a range of
                                ~2 * max pattern length bytes that still does                     */

/* enum PyMatchKind, src/lib.rs:92-108 */
#define ACX_MATCH_STANDARD 0
#define ACX_MATCH_LEFTMOST_FIRST 1
#define ACX_MATCH_LEFTMOST_LONGEST 2

/* build flags (acx_build_ex, acx_compile_host_ex).  ASCII_CASE_INSENSITIVE: the crate's
 * AhoCorasickBuilder::ascii_case_insensitive -- an ASCII letter of a pattern matches either case of that letter in the
 * haystack; no other byte folds.  Pattern ids, match kinds and overlapping keep their meaning; patterns that are equal
 * after folding are copies of one string.  Offsets are the caller's, and a replacement splices the caller's own bytes
 * around its matches.  Other bits: ACX_EINVAL. */
#define ACX_BUILD_ASCII_CASE_INSENSITIVE 1

/* enum Implementation (+ None), src/lib.rs:111-128.  A hint only: every value
 * yields identical results (tests/test_ac.py:23-31) and NO value selects a slower
 * scan kernel (the reference recommends the contiguous NFA as the default trade-off,
 * README.md:173-177).  It decides how large a dense transition table is kept: at most
 * ACX_DENSE_LIMIT bytes (default 256 MiB; DFA: 16 GiB); beyond that the automaton stays
 * in its compressed form (trie edges + failure links) and the walking kernels step
 * that -- the reference's "DFA for small sets, NFA beyond".  The scan kernel is picked
 * from the pattern statistics (acx_info.kernel; override: acx_set_kernel / ACX_KERNEL). */
#define ACX_IMPL_AUTO (-1)
#define ACX_IMPL_NONCONTIGUOUS_NFA 0
#define ACX_IMPL_CONTIGUOUS_NFA 1
#define ACX_IMPL_DFA 2

/* scan kernels (acx_info.kernel, acx_set_kernel).  Haystacks of at most 16 KiB are
 * answered by K0 -- one workgroup does the whole call (the occurrences by direct comparison for a
 * handful of short patterns, else by an anchored walk from every position, over tables staged in LDS
 * when they are small; sort, resolve, output; one launch, the result -- one 64-byte line that carries
 * the call's number at both ends -- polled from pinned memory) -- unless a scan
 * kernel was chosen explicitly with acx_set_kernel / ACX_KERNEL or the output is too dense for it.
 * Since round 4 the library's own choice is the prefilter for EVERY pattern set (patterns of 1 and
 * 2 bytes through its side test); the DFA walk runs when it is asked for. */
#define ACX_KERNEL_AUTO 0
#define ACX_KERNEL_DFA_WALK 1   /* K1a: the DFA walk -- failureless form, first four levels in LDS;
                                 * chunked walk for automata of more than 32 byte classes */
#define ACX_KERNEL_PREFILTER 2  /* K1b: LDS q-gram prefilter + exact prefix keys + verification */

/* One match: the tuple `(u64, usize, usize)` of src/lib.rs:234, 427. */
typedef struct acx_match {
    uint64_t pattern; /* index into the patterns iterable                     */
    uint64_t start;   /* byte offset, or code-point index when codepoints != 0 */
    uint64_t end;     /* exclusive                                            */
} acx_match_t;

typedef struct acx_automaton acx_automaton_t; /* owns host + device tables    */
typedef struct acx_result acx_result_t;       /* owns device-resident results */

typedef struct acx_info {
    uint64_t n_patterns;
    uint64_t n_states;
    uint32_t n_classes;   /* byte equivalence classes                          */
    uint32_t stride;      /* row length of the dense table (pow2 >= n_classes) */
    uint32_t min_pattern_len;
    uint32_t max_pattern_len;
    uint64_t table_bytes; /* dense DFA in HBM                                  */
    uint32_t lds_hot_rows;/* rows staged in LDS by K1a's chunked walk          */
    int32_t kernel;       /* ACX_KERNEL_* actually selected                    */
    int32_t match_kind;
    int32_t device;       /* HIP device ordinal the tables live on             */
    uint32_t filter_q;    /* q-gram length of the K1b prefilter (0 = none)     */
    uint32_t flags;       /* ACX_BUILD_* the handle was built with             */
} acx_info_t;

typedef struct acx_profile {
    double scan_ms;        /* accumulated HIP-event time of the scan kernel (K1) */
    uint64_t scan_launches;
    double post_ms;        /* kernels after the scan (collected only when ACX_PROFILE_POST is
                              set: it costs every call a wait for the previous one) */
    uint64_t scan_bytes;   /* haystack bytes scanned by those launches          */
    uint64_t raw_occurrences; /* occurrences emitted by K1 before resolution    */
    uint64_t prefix_hits;     /* K1b: prefix hits handed to the walk kernel      */
    uint64_t small_calls;     /* calls answered by K0 (whole call in one workgroup;
                                 counted whether or not profiling is enabled)     */
} acx_profile_t;

/* ---- process-wide ---- */
int acx_version(void);
const char *acx_last_error(void);
int acx_device_count(int *n);
int acx_set_device(int ordinal); /* device for subsequent acx_build on this thread */

/* ---- construction: replaces AhoCorasickBuilder::new().kind(..).match_kind(..)
 * .build(patterns) at src/lib.rs:186-215 (str) and 401-406 (bytes).
 * `blob` is the concatenation of the pattern bytes (UTF-8 for str patterns),
 * `offsets[n_patterns + 1]` delimits them.  Patterns are copied. */
int acx_build(const uint8_t *blob, const uint64_t *offsets, uint64_t n_patterns,
              int match_kind, int implementation, acx_automaton_t **out);
/* acx_build with build flags (ACX_BUILD_*; acx_build is flags = 0).  ACX_BUILD_ASCII_CASE_INSENSITIVE: the patterns are
 * folded (A-Z -> a-z) before they are compiled, and every haystack of the handle is searched in a folded copy: the pinned
 * host copy the calling thread makes anyway (K0, the resident K0, mid-size haystacks read in place) is a folding copy,
 * the staging buffer of larger host haystacks is folded in place on the device, and a device haystack is folded into a
 * grow-only buffer of the calling context (as large as the largest device haystack that context has searched).  The
 * caller's memory is never written.  acx_replicate carries the flags. */
int acx_build_ex(const uint8_t *blob, const uint64_t *offsets, uint64_t n_patterns, int match_kind, int implementation,
                 uint32_t flags, acx_automaton_t **out);
void acx_free_automaton(acx_automaton_t *a);
int acx_automaton_info(const acx_automaton_t *a, acx_info_t *out);
int acx_set_kernel(acx_automaton_t *a, int kernel); /* override the selection  */

/* ---- host-only compilation (no device needed): the compiled tables exactly
 * as they are uploaded to HBM.  For sizing an automaton before committing
 * device memory, for tooling, and for the CPU-side tests of the compiler.
 * This is NOT a matching path. ---- */
typedef struct acx_host_automaton acx_host_automaton_t;
typedef struct acx_host_tables {
    uint64_t n_patterns, n_states;
    uint32_t n_classes, stride, min_pattern_len, max_pattern_len;
    const uint8_t *classes;       /* 256: byte -> class                              */
    const uint32_t *table;        /* n_states * stride: id | OUT<<31 | OWN<<30; NULL when the dense form
                                     is not kept (dense == 0: n_states * stride * 4 > ACX_DENSE_LIMIT,
                                     default 256 MiB -- the reference's own "DFA for small sets, NFA
                                     beyond", README.md:173-177)                        */
    const uint32_t *own_off;      /* n_states + 1                                    */
    const uint32_t *own_pid;      /* patterns ending exactly at a state, id order    */
    const uint32_t *dlink;        /* dictionary-suffix link or 0xFFFFFFFF            */
    const uint32_t *level_start;  /* max_pattern_len + 2: first BFS id of each depth */
    const uint32_t *pattern_len;  /* n_patterns                                      */
    const uint32_t *rank;         /* n_patterns: rank in (len desc, id asc)          */
    const uint32_t *filter_xy;    /* K1b level 1: 2^filter_entries_log2 x {X, Y} signature words
                                     (bit layout: csrc/automaton.hpp, filter_bit)      */
    const uint32_t *prefix_table; /* K1b level 2: 2^prefix_table_log2 x {key lo, key hi, meta, code}:
                                     meta = key length K (1..8) | next << 4 | MORE << 8 (0xFFFFFFFF =
                                     empty; MORE: 16-bit filter of the keys with this home slot that sit
                                     further along the probe sequence: bit ((hash >> 11) & 15) of each).  next = 0: code = the only pattern with this key, or
                                     0x80000000 | index into prefix_lists; next = N: redirect -- look the
                                     first N bytes up.  A key = the first min(8, shortest pattern of its
                                     group) bytes of a pattern, a group = the patterns sharing their
                                     first filter_q2 bytes; a group's single key sits at the hash of those
                                     bytes, several keys behind a redirect entry (csrc/automaton.cpp)   */
    const uint32_t *prefix_lists; /* {count, pattern id, ...} per key shared by several patterns   */
    uint32_t filter_q, filter_q2; /* prefix lengths used by level 1 / level 2 (first-level keys)   */
    uint32_t filter_entries_log2, prefix_table_log2;
    double filter_density;        /* fraction of X bits set                            */
    uint32_t n_prefix_keys;       /* entries of prefix_table in use                    */
    uint32_t n_prefix_lists;      /* u32 words of prefix_lists                         */
    const uint32_t *prefix_bitmap;/* 2^(prefix_table_log2 + 3) bits: bit (hash >> (29 - prefix_table_log2)) of
                                     the first filter_q2 bytes of every group (hash: acx_prefix_slot(gram,
                                     filter_q2, 32)); K1b asks it before the table when the table is large */
    /* the compressed form (always present): trie edges + failure links               */
    uint32_t dense;               /* 1: `table` exists                                 */
    const uint32_t *first_child;  /* n_states + 1: children of s = ids [first_child[s], first_child[s+1]) */
    const uint8_t *in_byte;       /* n_states: byte on the edge into the state (children ascending)     */
    const uint32_t *fail;         /* n_states: failure link                                             */
    const uint8_t *state_flags;   /* n_states: bit 1 = reports something, bit 0 = ends a pattern itself */
    /* K1a's failureless walk (n_classes <= 32, else NULL; layouts: csrc/automaton.hpp)                 */
    const uint32_t *walk_t3b;     /* 33 792 words: by the symbols (low five bits) s0, s1, s2 of three bytes,
                                     word ((s0 << 5 | s1) * 33 + s2): the symbols a fourth byte can have on a
                                     trie path of depth 4; ~0: a pattern of <= 3 bytes ends on the path       */
    const uint32_t *walk_t3r;     /* n_classes^3 x {children bitmap by class, first child | SHORT << 31}: the
                                     depth-3 node of a class triple ((c0 * n_classes + c1) * n_classes + c2) */
    const uint32_t *walk_grec;    /* n_states x 4: {children bitmap, first child | OWN << 31, own pattern, 0}
                                     or a tail {bytes 0-3, 1 << 30 | n << 24, pattern, bytes 4-7}: the rest
                                     of the only pattern below the node, n <= 8 bytes                         */
    /* K1b, short patterns (round 4; layouts: csrc/automaton.hpp).  Patterns of 1 and 2 bytes are kept out of
       the prefilter tables above (filter_q / filter_q2 are taken from the shortest of the OTHER patterns,
       long_min_len) and found by a side test instead                                                       */
    uint32_t long_min_len;        /* shortest pattern of 3 bytes or more (5 when there is none)             */
    uint32_t n_short;             /* patterns of 1 or 2 bytes (0: the two tables below are NULL)             */
    uint32_t short_min_len;       /* the shortest of them                                                    */
    const uint32_t *short_xy;     /* 256 x {X, Y} by middle byte b(j+1): bit (b(j) & 31) of X -- a short pattern
                                     may start at j; bit (b(j+2) & 31) of Y -- one may start at j+1 (superset)  */
    const uint32_t *short_codes;  /* [b0]: the 1-byte pattern b0; [256 + (b0 | b1 << 8)]: the 2-byte pattern
                                     (b0, b1): pattern id, 0x80000000 | index into prefix_lists, or 0xFFFFFFFF  */
    /* K1b, anchors (round 4; csrc/automaton.hpp): a pattern is filed under the bytes at offset
       pattern_shift[i] (0 .. 12; crowded beginnings move away from theirs); filter_xy, prefix_table keys and
       the 12 tail bytes of a pattern's info are taken from that anchored suffix; a code in prefix_table /
       prefix_lists is pattern id | shift << 24: "the pattern may start `shift` bytes in front of the hit"   */
    uint32_t max_shift;           /* largest shift in use (0: none, pattern_head is NULL)                    */
    const uint8_t *pattern_shift; /* n_patterns                                                              */
    const uint32_t *pattern_head; /* n_patterns x 4: the pattern's first 12 bytes (what lies in front of the anchor) */
} acx_host_tables_t;
int acx_compile_host(const uint8_t *blob, const uint64_t *offsets, uint64_t n_patterns,
                     int match_kind, acx_host_automaton_t **out);
/* the same with build flags: the tables acx_build_ex uploads (ACX_BUILD_ASCII_CASE_INSENSITIVE: those of the folded
 * patterns) */
int acx_compile_host_ex(const uint8_t *blob, const uint64_t *offsets, uint64_t n_patterns, int match_kind, uint32_t flags,
                        acx_host_automaton_t **out);
int acx_host_tables(const acx_host_automaton_t *h, acx_host_tables_t *out);
uint32_t acx_filter_hash(uint32_t gram);   /* level-1 hash of a little-endian (Q-1)-gram   */
uint32_t acx_prefix_slot(uint64_t gram, uint32_t salt, uint32_t log2); /* home slot of the `salt` low
                                                                         bytes of gram */
void acx_free_host(acx_host_automaton_t *h);

/* ---- concurrency: every function taking an acx_automaton_t may be called from several
 * threads on ONE handle at the same time (the reference lets threads search one object
 * concurrently: methods take a shared reference and release the GIL, src/lib.rs:238, 261,
 * 433, 438).  Calls run side by side on separate HIP streams (up to ACX_MAX_CONCURRENCY,
 * default 4, per handle); acx_free_automaton must not race with them. */

/* ---- the hot path, host-memory form.  Replaces get_matches + collect:
 * src/lib.rs:42-68 with consumers 229-249 (str: codepoints = 1 applies the
 * get_byte_to_code_point fix-up of 73-88 on the device) and 422-434 (bytes).
 * `hay` is borrowed for the call.  `*out` is library-owned (acx_free_matches).
 * Order and content are bit-exact with the reference iterator.
 * Large haystacks are staged through pinned chunks by several host threads, each chunk's DMA
 * under the next chunk's copy; large results are returned in pinned host memory.
 * Short haystacks (<= 16 KiB; round 6): a loop of calls is answered by a RESIDENT workgroup per calling context that stays on
 * the device between the calls and is fed through pinned host memory (a poll on either side instead of a kernel launch:
 * ~5 us per call instead of ~12; the reference's benchmark loop, benchmarks/test_comparison.py:113-124).  It leaves
 * 200 us after the last call and at most 1 ms after its launch (ACX_RESIDENT_IDLE_US / ACX_RESIDENT_LIFE_US), and at once
 * when its context is used for anything else or the handle is freed: a device-wide synchronisation elsewhere in the
 * process waits that long at most.  ACX_NO_RESIDENT=1: a launch per call.  Haystacks up to 1 MiB are copied into
 * pinned host memory by the calling thread and read there by the scan (ACX_INPLACE_MAX, bytes; 0: never). */
int acx_find(acx_automaton_t *a, const uint8_t *hay, uint64_t len,
             int overlapping, int codepoints, acx_match_t **out, uint64_t *n_out);
void acx_free_matches(acx_match_t *m);

/* Precondition of codepoints = 1 (all entry points): haystack AND patterns are valid UTF-8 -- what
 * the reference's str API guarantees by construction (src/lib.rs:147-160, 232).  The device converts
 * a match's start through the lead-byte counts and takes its end as start + the pattern's own code
 * points; for a pattern that ends inside a character the reference's table would hold usize::MAX
 * (src/lib.rs:73-88) -- that input cannot come from a str and is not supported here. */

/* ---- batched host form (new API; parity definition:
 * batch(hs)[i] == find(hs[i])).  `hay` is the concatenation
 * of n_hay haystacks delimited by offsets[n_hay + 1]; counts[n_hay] receives
 * the number of matches of each haystack; matches are grouped by haystack in
 * order, offsets LOCAL to each haystack. */
int acx_find_batch(acx_automaton_t *a, const uint8_t *hay, const uint64_t *offsets,
                   uint64_t n_hay, int overlapping, int codepoints,
                   acx_match_t **out, uint64_t *n_out, uint64_t *counts);

/* ---- one process, several devices (north_star: "a batched find_matches_as_indexes over many
 * haystacks shards naturally across the 8 GPUs"; the reference's shape is ONE call from ONE process,
 * benchmarks/test_comparison.py:113-124).  acx_replicate compiles the automaton of `a` again on
 * another device (same patterns, match kind, implementation hint).  acx_find_batch_multi cuts the
 * batch into n_handles contiguous ranges of haystacks (acx_shard_range: sizes differ by at most one),
 * runs acx_find_batch on every handle from its own host thread and concatenates: the result is
 * identical to acx_find_batch on one handle.  No device-to-device traffic; the shards' match counts
 * are combined on the host (the multi-PROCESS form all-gathers them over RCCL instead:
 * ahocorasick_rs_amd/distributed.py). */
int acx_replicate(const acx_automaton_t *a, int device, acx_automaton_t **out);
int acx_automaton_device(const acx_automaton_t *a);
void acx_shard_range(uint64_t n_items, int shard, int n_shards, uint64_t *lo, uint64_t *hi);
int acx_find_batch_multi(acx_automaton_t *const *handles, int n_handles, const uint8_t *hay,
                         const uint64_t *offsets, uint64_t n_hay, int overlapping, int codepoints,
                         acx_match_t **out, uint64_t *n_out, uint64_t *counts);

/* ---- one process PER device: the count exchange over RCCL (north_star: "RCCL over xGMI only to gather
 * per-shard match counts").  The search itself needs no communicator: every rank scans its own range of
 * the batch (acx_shard_range) with its own replica of the automaton.  What the ranks exchange is one u64
 * each -- their match counts -- from which acx_output_offsets gives every rank its place in the global
 * output.  acx_comm_init_all: one process holding n devices (ncclCommInitAll; local_counts has n entries, one
 * per device in the order given).  acx_comm_unique_id + acx_comm_init_rank: one process per device
 * (ncclCommInitRank; the 128-byte id is created on one rank and carried to the others by the host's own
 * means -- a file, a socket, MPI); local_counts has one entry.  all_counts receives `world` entries on
 * every caller.  librccl is loaded on first use.  (The torch.distributed form of the same exchange:
 * ahocorasick_rs_amd/distributed.py.) */
#define ACX_COMM_ID_BYTES 128
typedef struct acx_comm acx_comm_t;
int acx_comm_init_all(const int *devices, int n, acx_comm_t **out);
int acx_comm_unique_id(uint8_t id[ACX_COMM_ID_BYTES]);
int acx_comm_init_rank(const uint8_t id[ACX_COMM_ID_BYTES], int world, int rank, int device, acx_comm_t **out);
int acx_comm_world(const acx_comm_t *c);
int acx_comm_local_ranks(const acx_comm_t *c);
int acx_comm_allgather_counts(acx_comm_t *c, const uint64_t *local_counts, uint64_t *all_counts);
void acx_comm_free(acx_comm_t *c);
/* offsets[r] = the matches of the ranks in front of r, offsets[world] = their total (exclusive prefix) */
void acx_output_offsets(const uint64_t *counts, int world, uint64_t *offsets);

/* ---- device-resident form (what bench.py times).  d_hay is a device pointer
 * to `len` bytes on the automaton's device.  Batches: either d_offsets
 * (device, n_hay + 1 u64, ragged) or uniform_len > 0 (n_hay * uniform_len ==
 * len) or neither (one haystack).  Results stay in HBM inside *out.
 * The call returns as soon as the number of matches is known (acx_result_count is valid
 * at once); the kernels that write the records may still be running on the library's
 * stream -- every accessor of the records waits for them, d_hay (and d_offsets) must stay
 * valid until one of them or acx_free_result has returned. */
int acx_find_device(acx_automaton_t *a, const void *d_hay, uint64_t len,
                    const uint64_t *d_offsets, uint64_t n_hay, uint64_t uniform_len,
                    int overlapping, int codepoints, acx_result_t **out);
uint64_t acx_result_count(const acx_result_t *r);
const acx_match_t *acx_result_device_matches(const acx_result_t *r);
const uint64_t *acx_result_device_counts(const acx_result_t *r); /* per haystack, or NULL */
int acx_result_copy(const acx_result_t *r, acx_match_t *host_out);
int acx_result_copy_counts(const acx_result_t *r, uint64_t *host_counts);
void acx_free_result(acx_result_t *r);

/* ---- replacement: the crate's AhoCorasick::replace_all / replace_all_bytes (a feature the reference binding does not
 * expose).  For a haystack h, its NON-overlapping matches (p_i, s_i, e_i) in the order acx_find reports them and one
 * replacement r[p] per pattern: out = h[0:s_0] + r[p_0] + h[e_0:s_1] + ... + r[p_last] + h[e_last:].  `repl_blob` +
 * `repl_offsets[n_repl + 1]` delimit the replacements (host memory, uploaded per call); n_repl must equal the number of
 * patterns (ACX_EINVAL otherwise).  Batches: offsets[n_hay + 1] (host) / d_offsets (device, from 0 to len) or uniform_len,
 * as for acx_find_batch / acx_find_device; every haystack is replaced on its own, the outputs lie behind one another.
 * Two routes: up to ACX_REPLACE_HOST_MAX bytes (default 1 MiB, read per call) acx_replace runs acx_find / acx_find_batch
 * and splices on the host; beyond, and always for acx_replace_device, the haystack is searched and spliced in HBM
 * (acx_path_stats [12]) and the output stays there until acx_replaced_copy moves it.  Outputs may exceed 2^32 bytes. */
typedef struct acx_replaced acx_replaced_t;
int acx_replace(acx_automaton_t *a, const uint8_t *hay, uint64_t len,
                const uint64_t *offsets /* NULL: one haystack; else n_hay + 1 */, uint64_t n_hay,
                const uint8_t *repl_blob, const uint64_t *repl_offsets, uint64_t n_repl,
                acx_replaced_t **out);
int acx_replace_device(acx_automaton_t *a, const void *d_hay, uint64_t len,
                       const uint64_t *d_offsets, uint64_t n_hay, uint64_t uniform_len,
                       const uint8_t *repl_blob, const uint64_t *repl_offsets, uint64_t n_repl,
                       acx_replaced_t **out);                 /* output stays in HBM */
uint64_t acx_replaced_len(const acx_replaced_t *r);           /* total output bytes (known when the call returns) */
int acx_replaced_offsets(const acx_replaced_t *r, uint64_t *host_offsets /* n_hay + 1 */);
int acx_replaced_copy(const acx_replaced_t *r, void *host_dst); /* waits for the device's splice */
const void *acx_replaced_device_bytes(const acx_replaced_t *r); /* NULL if spliced on the host */
void acx_free_replaced(acx_replaced_t *r);
/* host only, no device: the splice itself (the host route).  ACX_EINVAL when the matches are unsorted, overlap, lie
 * beyond the haystack or name a pattern >= n_repl. */
int acx_splice_host(const uint8_t *hay, uint64_t len, const acx_match_t *m, uint64_t n_m,
                    const uint8_t *repl_blob, const uint64_t *repl_offsets, uint64_t n_repl,
                    uint8_t *dst /* NULL: size only */, uint64_t *dst_len);

/* ---- summaries: what most callers want of a find, without its match list.  For a haystack h and M = the matches acx_find
 * reports for it (same match kind, `overlapping`, `codepoints`):
 *   total / counts[h]   len(M): every haystack's number of matches (always present; the crate has no single call for it --
 *                       AhoCorasick::find_iter(..).count(), find_overlapping_iter for overlapping)
 *   any bit h           M is not empty: the crate's AhoCorasick::is_match (it depends neither on the match kind nor on
 *                       `overlapping`)
 *   first[h]            M[0]; with overlapping = 0 the crate's AhoCorasick::find for the handle's match kind (what the
 *                       Python find_first asks for); pattern = UINT64_MAX (start = end = 0) when there is none
 *   by_pattern[p]       the matches of the whole call whose pattern is p (find_iter / find_overlapping_iter folded by
 *                       Match::pattern); an overlapping search over a set with copies of a string counts every copy
 * `what` selects the parts beyond the counts (ACX_SUM_*; 0: the total and the counts only; other bits: ACX_EINVAL); the
 * accessor of a part that was not asked for returns ACX_EINVAL.  Batches as for acx_find_batch / acx_find_device; the `any`
 * bitmap has (n_hay + 63) / 64 words, bit h & 63 of word h >> 6 (LSB first).  An overlapping search on a non-Standard handle
 * fails with ACX_EOVERLAP as the find does.
 * There is NO early exit: a summary costs one find over the whole input (plus a pass over its result); what it saves is
 * the match list -- 24 bytes per match in HBM that are never copied to the host.
 * Two routes, as for acx_replace: up to ACX_SUMMARY_HOST_MAX bytes (default 1 MiB, read per call) acx_summarize runs
 * acx_find / acx_find_batch and reduces on the host (acx_summarize_host); beyond, and always for acx_summarize_device, the
 * result is reduced in HBM behind the find on the same stream, its records are given back as soon as the reduction is
 * queued, and only the parts an accessor asks for cross to the host.  acx_summary_on_device tells which route ran. */
#define ACX_SUM_FIRST 1       /* any-bitmap + first match per haystack */
#define ACX_SUM_BY_PATTERN 2  /* per-pattern totals over the call      */
typedef struct acx_summary acx_summary_t;
int acx_summarize(acx_automaton_t *a, const uint8_t *hay, uint64_t len,
                  const uint64_t *offsets /* NULL: one haystack */, uint64_t n_hay,
                  int overlapping, int codepoints, uint32_t what, acx_summary_t **out);
int acx_summarize_device(acx_automaton_t *a, const void *d_hay, uint64_t len,
                         const uint64_t *d_offsets, uint64_t n_hay, uint64_t uniform_len,
                         int overlapping, int codepoints, uint32_t what, acx_summary_t **out);
uint64_t acx_summary_total(const acx_summary_t *r);            /* matches of the call; valid at return */
int acx_summary_on_device(const acx_summary_t *r);             /* 1: reduced in HBM, 0: on the host    */
int acx_summary_counts(const acx_summary_t *r, uint64_t *host_counts /* n_hay */);
int acx_summary_any(const acx_summary_t *r, uint64_t *host_bits /* (n_hay + 63) / 64 */);
int acx_summary_first(const acx_summary_t *r, acx_match_t *host_first /* n_hay */);
int acx_summary_by_pattern(const acx_summary_t *r, uint64_t *host_hist /* n_patterns */);
/* the same parts where they lie in HBM (each waits for the reduction); NULL on the host route or for a part not asked for */
const uint64_t *acx_summary_device_counts(const acx_summary_t *r);
const uint64_t *acx_summary_device_any(const acx_summary_t *r);
const acx_match_t *acx_summary_device_first(const acx_summary_t *r);
const uint64_t *acx_summary_device_by_pattern(const acx_summary_t *r);
void acx_free_summary(acx_summary_t *r);
/* host only, no device: the reduction itself (the host route).  m: the matches of all haystacks behind one another,
 * counts[n_hay] how many each has (NULL: one haystack).  Outputs that `what` does not ask for may be NULL.  ACX_EINVAL when
 * the counts do not sum to n_m or a match names a pattern >= n_patterns. */
int acx_summarize_host(const acx_match_t *m, uint64_t n_m, const uint64_t *counts /* NULL: one haystack */,
                       uint64_t n_hay, uint64_t n_patterns, uint32_t what,
                       uint64_t *any_bits, acx_match_t *first, uint64_t *by_pattern);

/* ---- columns: the matches of a find as three int64 columns (pattern, start, end) instead of records, where the search
 * ran.  Row i of the columns is match i of acx_find / acx_find_batch / acx_find_device for the same arguments (same match
 * kind, `overlapping`, `codepoints`).  A batch (offsets != NULL; d_offsets or uniform_len on the device) also has
 * ACX_COL_ROW_OFFSETS: n_hay + 1 words, rows row_offsets[h] .. row_offsets[h + 1] are haystack h's matches, their offsets
 * local to it (the CSR form; the exclusive prefix of acx_find_batch's counts).
 * Two routes.  acx_find_columns: the find runs as acx_find / acx_find_batch do (the small-call kernel, the in-place read,
 * the staged pipeline), the records are split on the host (acx_split_host) and the columns are host memory.
 * acx_find_columns_device: acx_find_device's pipeline, then a split kernel (and, for a batch, the scan of the counts) on
 * the same stream; the columns and the row offsets are in HBM on the automaton's device and only the number of matches
 * crosses to the host.  The call returns when that number is known; the kernels may still run, and acx_columns_data /
 * acx_columns_copy wait for them -- a pointer they return is to finished data, whatever stream reads it.
 * Memory in HBM: the find writes its records (24 bytes per match) and the split writes the columns (24 bytes per match)
 * before the records go back to the library's buffer cache -- which happens as soon as the split is queued, behind an
 * event, never later than acx_free_columns.  The peak is therefore TWICE the result (until the find's write kernel writes
 * columns itself), the steady state once.
 * An empty column still has a valid, non-null address.  acx_columns_rows is 0 in the single form (and for an empty
 * batch: there acx_columns_data(c, ACX_COL_ROW_OFFSETS) is non-null and holds one 0). */
#define ACX_COL_PATTERN 0
#define ACX_COL_START 1
#define ACX_COL_END 2
#define ACX_COL_ROW_OFFSETS 3
typedef struct acx_columns acx_columns_t;
int acx_find_columns(acx_automaton_t *a, const uint8_t *hay, uint64_t len,
                     const uint64_t *offsets /* NULL: one haystack */, uint64_t n_hay,
                     int overlapping, int codepoints, acx_columns_t **out);
int acx_find_columns_device(acx_automaton_t *a, const void *d_hay, uint64_t len,
                            const uint64_t *d_offsets, uint64_t n_hay, uint64_t uniform_len,
                            int overlapping, int codepoints, acx_columns_t **out);
uint64_t acx_columns_count(const acx_columns_t *c);   /* matches = words per column; valid at return */
uint64_t acx_columns_rows(const acx_columns_t *c);    /* haystacks of a batch; 0: single form        */
int acx_columns_on_device(const acx_columns_t *c);    /* 1: the columns are in HBM, 0: host memory   */
/* host or device pointer by acx_columns_on_device; waits for the split.  NULL: no such column (row offsets of the single
 * form) or the wait failed.  Valid until acx_free_columns. */
const int64_t *acx_columns_data(const acx_columns_t *c, int which);
int acx_columns_copy(const acx_columns_t *c, int which, int64_t *host_dst);
void acx_free_columns(acx_columns_t *c);
/* the split itself.  acx_split_host: host memory, no device needed.  acx_split_device: the kernel's raw entry point for
 * callers that hold the result of acx_find_device (its records: acx_result_device_matches) -- records and columns in HBM on one device, 8-byte
 * alignment is all either needs (a sub-range that begins at an odd record lies at 8 mod 16), nothing may overlap;
 * synchronous: the columns are complete when it returns.  n = 0: nothing is touched. */
int acx_split_host(const acx_match_t *m, uint64_t n, int64_t *pattern, int64_t *start, int64_t *end);
int acx_split_device(const acx_match_t *d_m, uint64_t n, int64_t *d_pattern, int64_t *d_start, int64_t *d_end);

/* ---- tally: which patterns occur in which haystack of a batch, and how often, as a sparse matrix in CSR form.
 * C[h][p] = the number of haystack h's matches (acx_find_batch / acx_find_device for the same arguments) with pattern p:
 *   ACX_TALLY_ROW_OFFSETS  rows + 1 words from 0; entries row_offsets[h] .. row_offsets[h + 1] are haystack h's
 *   ACX_TALLY_PATTERN      nnz words, STRICTLY ASCENDING within a row (the canonical form: torch.sparse_csr_tensor takes the
 *                          three parts as they are)
 *   ACX_TALLY_COUNT        nnz words, all >= 1
 * nnz = the number of distinct (haystack, pattern) pairs.  Every match kind; an overlapping search over a set with copies
 * counts every copy.  No offset is reported, so the search runs on bytes whatever the caller's strings are.
 * acx_tally: host haystacks (offsets: n_hay + 1, or null: one haystack of len bytes), a host result.  Up to
 * ACX_TALLY_HOST_MAX bytes (environment, read per call; default 1 MiB -- ACX_SUMMARY_HOST_MAX's default, not a measured
 * crossover) acx_find_batch runs and acx_tally_host reduces; beyond that the batch is staged, searched and reduced on the
 * device and the compact block comes back in one copy.
 * acx_tally_device: acx_find_device's pipeline (d_offsets / uniform_len as there), then the device stage on the same
 * stream; the result stays in HBM on the automaton's device and only nnz (and the number of records in rows too long for
 * the tile kernel) crosses to the host.  The call returns when nnz is known; the last kernel may still run, and
 * acx_tally_data / acx_tally_copy wait for it.  ACX_TALLY_ROW_MAX (environment, read per call) lowers the longest row the
 * tile kernel takes (2048 records); 0 sends every row through the radix-sort form.
 * An empty part still has a valid, non-null address; an empty batch has one row offset, 0. */
#define ACX_TALLY_ROW_OFFSETS 0
#define ACX_TALLY_PATTERN 1
#define ACX_TALLY_COUNT 2
typedef struct acx_tally acx_tally_t;
int acx_tally(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay,
              int overlapping, acx_tally_t **out);
int acx_tally_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                     uint64_t uniform_len, int overlapping, acx_tally_t **out);
uint64_t acx_tally_nnz(const acx_tally_t *t);      /* entries of pattern / count; valid at return        */
uint64_t acx_tally_rows(const acx_tally_t *t);     /* haystacks                                          */
int acx_tally_on_device(const acx_tally_t *t);     /* 1: the parts are in HBM, 0: host memory            */
/* host or device pointer by acx_tally_on_device; waits for the device stage.  NULL: no such part or the wait failed.
 * Valid until acx_free_tally. */
const int64_t *acx_tally_data(const acx_tally_t *t, int which);
int acx_tally_copy(const acx_tally_t *t, int which, int64_t *host_dst);
void acx_free_tally(acx_tally_t *t);
/* the reduction itself.  acx_tally_host: host memory, no device needed; m: n_m matches, all haystacks behind one another,
 * counts[h] of them haystack h's (they must sum to n_m); row_offsets: n_hay + 1 words, pattern and count: room for n_m.
 * acx_tally_rows_device: the device stage alone on records and counts in HBM on one device (8-byte alignment is all they
 * and the outputs need; d_pattern and d_count: room for n words; pattern ids below n_patterns <= 2^24; the counts must sum
 * to n); synchronous: the outputs are complete when it returns. */
int acx_tally_host(const acx_match_t *m, uint64_t n_m, const uint64_t *counts, uint64_t n_hay, int64_t *row_offsets,
                   int64_t *pattern, int64_t *count, uint64_t *nnz);
int acx_tally_rows_device(const acx_match_t *d_records, uint64_t n, const uint64_t *d_counts, uint64_t n_hay,
                          uint64_t n_patterns, int64_t *d_row_offsets, int64_t *d_pattern, int64_t *d_count, uint64_t *nnz);

/* ---- filter: keep or drop the rows of a batch by match -- "drop every document that contains a blocked term", "keep the
 * rows that mention one of these names" -- as a compacted batch where the search ran.  For a batch of n rows, c[h] = the
 * number of row h's matches (acx_find_batch / acx_find_device for the same arguments): row h is MATCHED iff c[h] >=
 * min_matches (>= 1; 0: ACX_EINVAL), and KEPT iff matched == (flags & ACX_FILTER_KEEP_MATCHED != 0) -- flags = 0 keeps the
 * unmatched rows; any other bit: ACX_EINVAL.  The result is
 *   ACX_FILT_ROWS     k words: the kept source row indexes, strictly ascending
 *   ACX_FILT_OFFSETS  k + 1 words from 0
 *   ACX_FILT_DATA     offsets[k] bytes: the kept rows back to back, row rows[i] = data[offsets[i] .. offsets[i + 1]), the
 *                     caller's own bytes (a case-insensitive handle matches on a folded copy and copies the unfolded row)
 * Empty rows are rows: a kept one is an entry of rows and a repeated offset.  Every match kind; an overlapping search on a
 * non-Standard handle fails with ACX_EOVERLAP as the find does, and one over a set with copies counts every copy.  No offset
 * into a row is reported, so the search runs on bytes whatever the caller's strings are.
 * acx_filter: host haystacks (offsets: n_hay + 1, or null: one haystack of len bytes -- a batch of one row), a host result.
 * The counts come from acx_summarize (what = 0), which chooses its own route: 8 bytes per row come back; the rows are then
 * copied from the caller's memory by acx_filter_host, so the output never crosses the bus.
 * acx_filter_device: acx_find_device's pipeline (d_offsets / uniform_len as there; neither: a batch of one row), then the
 * device stage on the same stream -- two scans of the per-row counts and a ragged gather; the result stays in HBM on the
 * automaton's device and only its two sizes (16 bytes) cross to the host.  The call returns when they are known; the gather
 * may still run, and acx_filtered_data / acx_filtered_copy wait for it.  d_hay and d_offsets must stay valid until then.
 * Nothing kept: the offsets part holds one 0.  Everything kept: the data is a device-to-device copy of the input.
 * An empty part still has a valid, non-null address. */
#define ACX_FILTER_KEEP_MATCHED 1
#define ACX_FILT_ROWS 0
#define ACX_FILT_OFFSETS 1
#define ACX_FILT_DATA 2
typedef struct acx_filtered acx_filtered_t;
int acx_filter(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay,
               int overlapping, uint64_t min_matches, uint32_t flags, acx_filtered_t **out);
int acx_filter_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                      uint64_t uniform_len, int overlapping, uint64_t min_matches, uint32_t flags, acx_filtered_t **out);
uint64_t acx_filtered_rows(const acx_filtered_t *f);   /* k: the kept rows; valid at return                      */
uint64_t acx_filtered_bytes(const acx_filtered_t *f);  /* offsets[k]: the kept rows' bytes; valid at return      */
int acx_filtered_on_device(const acx_filtered_t *f);   /* 1: the parts are in HBM, 0: host memory                */
/* host or device pointer by acx_filtered_on_device (ROWS, OFFSETS: int64 words; DATA: bytes); waits for the device stage.
 * NULL: no such part or the wait failed.  Valid until acx_free_filtered. */
const void *acx_filtered_data(const acx_filtered_t *f, int which);
int acx_filtered_copy(const acx_filtered_t *f, int which, void *host_dst);
void acx_free_filtered(acx_filtered_t *f);
/* the filter itself.  acx_filter_host: host memory, no device needed -- the definition above inside the library; counts:
 * n_hay words; offsets: n_hay + 1 from 0 to len (ACX_EINVAL when they do not rise from 0 to len), or null: one row of len
 * bytes; rows: room for n_hay, out_offsets: n_hay + 1, dst: len bytes -- any of the three may be NULL (dst = NULL: sizes
 * only); *n_rows = k, *n_bytes = offsets[k].
 * acx_filter_rows_device: the device stage alone on a caller's bytes, offsets (or uniform_len, or neither: one row) and
 * counts in HBM on one device; needs no automaton; synchronous: the outputs are complete when it returns.  d_rows: room
 * for n_hay words, d_out_offsets: n_hay + 1, d_data: round_up(len, 16) bytes -- the bytes behind *n_bytes up to the next
 * multiple of 16 may be written.  The word arrays need 8-byte alignment, d_data 16-byte alignment, d_hay none. */
int acx_filter_host(const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay, const uint64_t *counts,
                    uint64_t min_matches, uint32_t flags, int64_t *rows, int64_t *out_offsets,
                    uint8_t *dst /* NULL: sizes only */, uint64_t *n_rows, uint64_t *n_bytes);
int acx_filter_rows_device(const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay, uint64_t uniform_len,
                           const uint64_t *d_counts, uint64_t min_matches, uint32_t flags, int64_t *d_rows,
                           int64_t *d_out_offsets, uint8_t *d_data, uint64_t *n_rows, uint64_t *n_bytes);

/* ---- scores: per-pattern weights, a score per row, and the row filter by score -- a block list with exceptions, a weighted
 * lexicon, a threshold on "how much" of a row matched.  A handle has P patterns; weights: P int32 (host memory; n_weights
 * != P: ACX_EINVAL).  score[h] = the sum of weights[pattern] over the matches acx_find_batch / acx_find_device reports for
 * row h with the same `overlapping`: an int64, two's complement (it wraps modulo 2^64, which no row of fewer than 2^32
 * matches reaches).  An overlapping search over a set with copies counts every copy with its own weight; a
 * case-insensitive handle matches on the folded copy; no offset is reported, so the search runs on bytes whatever the
 * caller's strings are; an empty row scores 0; a record whose pattern is >= P adds nothing and never indexes the weights.
 * An overlapping search on a non-Standard handle fails with ACX_EOVERLAP before any device state is touched.
 * acx_score: host haystacks (offsets: n_hay + 1, or null: one haystack of len bytes -- a batch of one row), a host result.
 * Up to ACX_SCORE_HOST_MAX bytes (environment, read per call; default 1 MiB, ACX_SUMMARY_HOST_MAX's: not a measured
 * crossover) acx_find / acx_find_batch runs and acx_score_host sums; beyond that the batch is staged, searched and scored in
 * HBM and only 8 bytes per row come back.
 * acx_score_device: acx_find_device's pipeline (d_offsets / uniform_len as there; neither: a batch of one row), then the
 * device stage on the same stream -- one pass over the records, no sort; the result stays in HBM on the automaton's device.
 * The call may return with the stage in flight: acx_scores_data / acx_scores_copy wait for it.  d_hay and d_offsets must
 * stay valid until then; the weights are copied before the call returns.
 * An empty result still has a valid, non-null address. */
typedef struct acx_scores acx_scores_t;
int acx_score(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay,
              int overlapping, const int32_t *weights, uint64_t n_weights, acx_scores_t **out);
int acx_score_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                     uint64_t uniform_len, int overlapping, const int32_t *weights /* host */, uint64_t n_weights,
                     acx_scores_t **out);
uint64_t acx_scores_rows(const acx_scores_t *s);     /* haystacks = int64 words of the result              */
int acx_scores_on_device(const acx_scores_t *s);     /* 1: the scores are in HBM, 0: host memory           */
/* host or device pointer by acx_scores_on_device; waits for the device stage.  NULL: the wait failed.  Valid until
 * acx_free_scores. */
const int64_t *acx_scores_data(const acx_scores_t *s);
int acx_scores_copy(const acx_scores_t *s, int64_t *host_dst);
void acx_free_scores(acx_scores_t *s);
/* the sum itself.  acx_score_host: host memory, no device needed -- the definition above inside the library; m: n_m matches,
 * all haystacks behind one another, counts[h] of them haystack h's (ACX_EINVAL when they do not sum to n_m), or counts =
 * NULL: one row holds them all (n_hay = 1); scores: n_hay words.
 * acx_score_rows_device: the device stage alone on records, counts (they must sum to n) and int32 weights in HBM on one
 * device (8-byte alignment is all the records need, the weights 4-byte); needs no automaton; synchronous: d_scores (n_hay
 * words) is complete when it returns.  n_hay = 0 launches nothing; n = 0 clears the scores. */
int acx_score_host(const acx_match_t *m, uint64_t n_m, const uint64_t *counts /* NULL: one row */, uint64_t n_hay,
                   const int32_t *weights, uint64_t n_weights, int64_t *scores);
int acx_score_rows_device(const acx_match_t *d_records, uint64_t n, const uint64_t *d_counts, uint64_t n_hay,
                          const int32_t *d_weights, uint64_t n_weights, int64_t *d_scores);
/* the row filter by score: row h is MATCHED iff score[h] >= min_score (signed, any int64) and KEPT iff matched == (flags &
 * ACX_FILTER_KEEP_MATCHED != 0); the result is an acx_filtered_t exactly as acx_filter / acx_filter_device make it.
 * acx_filter_scored: the scores from acx_score (its own choice of route), then acx_filter_host over their 0 / 1 verdicts.
 * acx_filter_scored_device: between the find and the filter's device stage, on the same stream, the scores and their
 * verdicts are made in HBM, and the stage runs on the verdicts as its counts with min_matches = 1. */
int acx_filter_scored(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay,
                      int overlapping, const int32_t *weights, uint64_t n_weights, int64_t min_score, uint32_t flags,
                      acx_filtered_t **out);
int acx_filter_scored_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                             uint64_t uniform_len, int overlapping, const int32_t *weights /* host */, uint64_t n_weights,
                             int64_t min_score, uint32_t flags, acx_filtered_t **out);

/* ---- cover / mask: every byte that a match covers becomes one fill byte, every other byte stays where it was -- fixed-fill
 * redaction, a highlight map, a loss mask -- as a same-length output in the caller's own layout.  For a batch of rows, row h
 * = hay[off[h] .. off[h + 1]) and M_h = the matches acx_find_batch / acx_find_device reports for row h with the same
 * `overlapping`: byte i of row h is COVERED iff some m in M_h has m.start <= i < m.end (an empty match covers nothing), and
 *   out[off[h] + i] = covered ? fill : (flags & ACX_MASK_ZERO ? 0 : hay[off[h] + i])
 * -- exactly len bytes.  flags = 0 is the haystack with its matches blanked; ACX_MASK_ZERO with fill = 1 is the 0 / 1 mask;
 * any other flag bit: ACX_EINVAL.  The uncovered bytes are the caller's own (a case-insensitive handle matches on a folded
 * copy and writes the unfolded bytes).  Every match kind; an overlapping search on a Standard handle covers the union of all
 * occurrences, one on a non-Standard handle fails with ACX_EOVERLAP before any device state is touched, and copies of a
 * pattern cover the same bytes once.  No offset is reported, so the search runs on bytes whatever the caller's strings are
 * (a str set's matches cover whole characters anyway).
 * acx_mask: host haystacks (offsets: n_hay + 1, or null: one haystack of len bytes -- a batch of one row), a host result.
 * acx_find / acx_find_batch runs as it is and chooses its own route; acx_mask_host then paints a copy of the caller's bytes:
 * the records cross the bus, the output never does (painting in HBM and sending len bytes back wins only for inputs denser
 * than one match per 24 bytes; the choice is not measured).
 * acx_mask_device: acx_find_device's pipeline (d_offsets / uniform_len as there; neither: a batch of one row), then the
 * device stage on the same stream -- a device-to-device copy (or a clear) and one pass over the records; the result stays in
 * HBM on the automaton's device.  The call may return with the stage in flight: acx_masked_data / _offsets / _copy wait for
 * it.  d_hay and d_offsets must stay valid until then.
 * The result carries the rows' offsets beside the bytes: rows + 1 int64 words from 0 to len, in the same memory.
 * An empty part still has a valid, non-null address. */
#define ACX_MASK_ZERO 1
typedef struct acx_masked acx_masked_t;
int acx_mask(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay,
             int overlapping, uint8_t fill, uint32_t flags, acx_masked_t **out);
int acx_mask_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                    uint64_t uniform_len, int overlapping, uint8_t fill, uint32_t flags, acx_masked_t **out);
uint64_t acx_masked_bytes(const acx_masked_t *m);    /* len: the output's bytes                               */
uint64_t acx_masked_rows(const acx_masked_t *m);     /* the rows of the batch                                 */
int acx_masked_on_device(const acx_masked_t *m);     /* 1: the parts are in HBM, 0: host memory               */
/* host or device pointer by acx_masked_on_device (the bytes; the offsets: rows + 1 int64 words); waits for the device stage.
 * NULL: the wait failed.  Valid until acx_free_masked. */
const void *acx_masked_data(const acx_masked_t *m);
const int64_t *acx_masked_offsets(const acx_masked_t *m);
int acx_masked_copy(const acx_masked_t *m, void *host_dst);
int acx_masked_copy_offsets(const acx_masked_t *m, int64_t *host_dst);
void acx_free_masked(acx_masked_t *m);
/* the cover itself.  Both take records from a caller, so both CLIP: a record's [start, end) is cut to its row first (end' =
 * min(end, row length), start' = min(start, end')) -- no record writes outside its own row, whatever it says.
 * acx_mask_host: host memory, no device needed -- the definition above inside the library; m: n_m matches, all haystacks
 * behind one another, counts[h] of them haystack h's (ACX_EINVAL when they do not sum to n_m), or counts = NULL: one row
 * holds them all; offsets: n_hay + 1 from 0 to len (ACX_EINVAL when they do not rise from 0 to len), or null: one row of len
 * bytes; dst: len bytes (dst == hay: in place, not with ACX_MASK_ZERO).
 * acx_mask_rows_device: the device stage alone on a caller's bytes, offsets (or uniform_len, or neither: one row), records
 * and counts (they must sum to n: checked before a kernel reads a record by them) in HBM on one device; needs no automaton;
 * synchronous: d_out is complete when it returns.  It writes exactly len bytes at d_out and nothing beyond them -- there is
 * no round-up.  No pointer needs any alignment except the word arrays (offsets, records, counts: 8 bytes).  d_out == d_hay:
 * in place -- no copy, only the covered bytes are written; not together with ACX_MASK_ZERO (ACX_EINVAL).  Any other overlap
 * of d_hay and d_out is the caller's error: it is not detected.  len = 0, n_hay = 0 and n = 0 launch nothing beyond the copy
 * or the clear (and with n = 0 the counts are not read). */
int acx_mask_host(const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay, const acx_match_t *m,
                  uint64_t n_m, const uint64_t *counts /* NULL: one row */, uint8_t fill, uint32_t flags, uint8_t *dst);
int acx_mask_rows_device(const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay, uint64_t uniform_len,
                         const acx_match_t *d_records, uint64_t n, const uint64_t *d_counts, uint8_t fill, uint32_t flags,
                         void *d_out);

/* ---- rows: a delimited buffer (newline-terminated records: web text, JSONL, logs) cut into the rows the batch entry points
 * take -- the step before acx_filter_device, acx_score_device, acx_mask_device, acx_tally_device and the rest.  No automaton is
 * involved.  For `len` bytes and a delimiter byte d the result is rows + 1 int64 words:
 *   0; then p + 1 for every position p with hay[p] == d, ascending; then len if len > 0 and hay[len - 1] != d
 * -- row i is hay[offsets[i] .. offsets[i + 1]).  Every row but possibly the last ends with its delimiter (the delimiter
 * belongs to the row, as in Python's splitlines(keepends=True) for '\n'), no row is empty, and the words rise strictly from 0
 * to len: exactly what `offsets` / `d_offsets` of the batch entry points must be.  No bytes: 0 rows and the one word 0.
 * acx_split_rows: host bytes, a host result.
 * acx_split_rows_device: bytes in HBM (any address), the result in HBM on the same device; the work is queued on that
 * device's null stream: two passes over the bytes with a scan of per-tile counts between them, and 16 bytes back to the host
 * (the number of rows).  It returns once the number of rows is known -- acx_rows_count is valid at return -- and the second
 * pass may still run: acx_rows_offsets / _copy wait for it.  d_hay must stay valid and unchanged until then.  A result of 8
 * bytes per input byte (every byte a delimiter) that cannot be allocated is ACX_ENOMEM.
 * len = 0 launches nothing and allows a null pointer; a null pointer with len > 0 is ACX_EINVAL. */
typedef struct acx_rows acx_rows_t;
int acx_split_rows(const uint8_t *hay, uint64_t len, uint8_t delimiter, acx_rows_t **out);
int acx_split_rows_device(const void *d_hay, uint64_t len, uint8_t delimiter, acx_rows_t **out);
uint64_t acx_rows_count(const acx_rows_t *r);      /* the rows; valid when the call has returned           */
uint64_t acx_rows_bytes(const acx_rows_t *r);      /* len                                                   */
int acx_rows_on_device(const acx_rows_t *r);       /* 1: the offsets are in HBM, 0: host memory             */
int acx_rows_device(const acx_rows_t *r);          /* the HIP ordinal they lie on (on_device)               */
/* host or device pointer by acx_rows_on_device: rows + 1 int64 words; waits for the device stage.  NULL: the wait failed.
 * Valid until acx_free_rows. */
const int64_t *acx_rows_offsets(const acx_rows_t *r);
int acx_rows_copy(const acx_rows_t *r, int64_t *host_dst);
void acx_free_rows(acx_rows_t *r);
/* the cut itself, into the caller's memory.  capacity: the int64 words `offsets` / `d_offsets` holds; *n_rows is set whenever
 * the bytes were counted.  rows + 1 > capacity: nothing is written behind the buffer (nothing at all), *n_rows says what is
 * needed and the call returns ACX_EINVAL with a message that names the number of words.
 * acx_split_rows_host: host memory, no device needed -- the definition above inside the library; offsets = NULL counts only.
 * acx_split_rows_into_device: the device stage alone; synchronous: d_offsets is complete when it returns.  d_offsets: 8-byte
 * aligned (ACX_EINVAL otherwise), or NULL: count only; d_hay: any address. */
int acx_split_rows_host(const uint8_t *hay, uint64_t len, uint8_t delimiter, int64_t *offsets /* NULL: count only */,
                        uint64_t capacity, uint64_t *n_rows);
int acx_split_rows_into_device(const void *d_hay, uint64_t len, uint8_t delimiter, int64_t *d_offsets, uint64_t capacity,
                               uint64_t *n_rows);

/* ---- merged spans: the union of a search's matches as `start` / `end` columns -- what a highlight, a snippet cut, a
 * redaction range or a map from matches to tokens needs -- 16 bytes per run of covered positions instead of the mask's byte
 * per haystack byte.  For a batch of rows, row h's matches M_h (what acx_find_batch / acx_find_device reports for the same
 * match kind, overlapping and codepoints, offsets local to the row; a match with start >= end covers nothing and is ignored)
 * and gap >= 0: the spans of row h are the coarsest partition of M_h into groups such that two matches are in one group when
 * the later one starts at most `gap` positions behind the end of the earlier one (start <= end of the other + gap, through
 * chains); a span is (min start, max end) of a group.  Within a row the spans are ascending and disjoint, and two consecutive
 * ones satisfy next.start - prev.end > gap; with gap = 0 they are exactly the maximal runs of ones in the 0 / 1 mask
 * (ACX_MASK_ZERO, fill 1) of the same search: touching matches are one span.  Spans never join across rows.
 * The result: two int64 columns of acx_spans_count words and -- for a batch -- rows + 1 row offsets from 0 to the count (the
 * CSR form: spans row_offsets[h] .. row_offsets[h + 1] - 1 are row h's).  gap >= 2^63 is ACX_EINVAL.
 * acx_spans: host haystacks (offsets: n_hay + 1, or NULL: one haystack of len bytes, no row offsets), a host result.
 * acx_find / acx_find_batch runs as it is and chooses its own route; the records cross the bus and acx_spans_host merges them.
 * acx_spans_device: acx_find_device's pipeline (d_offsets / uniform_len as there; neither: one haystack, acx_spans_rows is 0
 * and there are no row offsets), then the span stage on the same stream: the result lies in HBM on the automaton's device.
 * The call returns when the number of spans is known (8 bytes cross the bus); the last kernel may still run: acx_spans_data /
 * _copy wait for it.  d_hay and d_offsets must stay valid and unchanged until then.  An overlapping search on a handle that
 * is not Standard is ACX_EOVERLAP before any device state; a result block that cannot be allocated is ACX_ENOMEM. */
#define ACX_SPAN_START 0
#define ACX_SPAN_END 1
#define ACX_SPAN_ROW_OFFSETS 2
typedef struct acx_spans acx_spans_t;
int acx_spans(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets /* NULL: one haystack */,
              uint64_t n_hay, int overlapping, int codepoints, uint64_t gap, acx_spans_t **out);
int acx_spans_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                     uint64_t uniform_len, int overlapping, int codepoints, uint64_t gap, acx_spans_t **out);
uint64_t acx_spans_count(const acx_spans_t *s);    /* S: the spans; valid when the call has returned        */
uint64_t acx_spans_rows(const acx_spans_t *s);     /* the rows of the batch; 0: one haystack                */
int acx_spans_on_device(const acx_spans_t *s);     /* 1: the columns are in HBM, 0: host memory             */
/* host or device pointer by acx_spans_on_device: column `which` (ACX_SPAN_*: S words; the row offsets: rows + 1); waits for
 * the device stage.  NULL: no such column (the single form has no row offsets), or the wait failed.  Valid until
 * acx_free_spans. */
const int64_t *acx_spans_data(const acx_spans_t *s, int which);
int acx_spans_copy(const acx_spans_t *s, int which, int64_t *host_dst);
void acx_free_spans(acx_spans_t *s);
/* the merge itself, over a caller's records.  PRECONDITION: within a row the records' ends do not decrease -- the order of
 * every find of this library (overlapping: by end, then longer first; else by start).  With sufmin(i) = the smallest start of
 * a live record at index >= i of record i's row, a live record i closes a span iff no live record follows it in its row or
 * sufmin(i + 1) - end_i > gap, and an index opens one iff it is its row's first or follows a closer, and a live record lies
 * at or behind it; the k-th opener's sufmin and the k-th closer's end are span k.  For records in another order these same
 * formulas are evaluated: memory-safe, at most n spans, not the union.
 * acx_spans_host: host memory, no device needed -- the definition inside the library; m: n_m records, all rows behind one
 * another, counts[h] of them row h's (ACX_EINVAL when they do not sum to n_m), or counts = NULL: one row holds them all;
 * row_offsets: n_hay + 1 words (one row: 2), or NULL: not wanted; start, end: n_m words each, the first *n_spans are written.
 * acx_spans_rows_device: the device stage alone on a caller's records and counts (they must sum to n: checked before a kernel
 * reads a record by them, and before anything is written) in HBM on one device; needs no automaton; synchronous: the outputs
 * are complete when it returns.  d_start, d_end: n words each, the first *n_spans are written and nothing behind them;
 * d_row_offsets: n_hay + 1 words, all written.  Every pointer 8-byte aligned.  n = 0 writes the zero row offsets and launches
 * nothing else (the counts are not read). */
int acx_spans_host(const acx_match_t *m, uint64_t n_m, const uint64_t *counts /* NULL: one row */, uint64_t n_hay, uint64_t gap,
                   int64_t *row_offsets, int64_t *start, int64_t *end, uint64_t *n_spans);
int acx_spans_rows_device(const acx_match_t *d_records, uint64_t n, const uint64_t *d_counts, uint64_t n_hay, uint64_t gap,
                          int64_t *d_row_offsets, int64_t *d_start, int64_t *d_end, uint64_t *n_spans);

/* ---- snippets: the matched text and the text around it -- the audit line, the KWIC snippet, grep -o and grep -C in bytes --
 * as the caller's own bytes, where the search ran.  One snippet per match of acx_find_batch / acx_find_device for the same match
 * kind and overlapping, with byte offsets (codepoints = 0), in the find's order.  THE DEFINITION, for a record (p, s, e) in a row
 * of L bytes B (row-local byte offsets) and a budget of `context` bytes on each side:
 *   s' = min(s, L);  e' = min(max(e, s'), L)                        (any record is memory-safe)
 *   lo = s' - min(s', context);  hi = e' + min(context, L - e')     (no sum can wrap)
 *   ACX_SNIPPET_UTF8 only:  up to 3 times: if lo < s' and B[lo] in 0x80..0xBF: lo += 1
 *                        up to 3 times: if e' < hi < L and B[hi] in 0x80..0xBF: hi -= 1
 *   snippet = B[lo:hi];  lead = s' - lo
 * The context is clipped to the row: snippets never cross a row.  With ACX_SNIPPET_UTF8 the ends move INWARD to a character
 * boundary and never into the match, so a snippet of valid UTF-8 around a match on character boundaries decodes; the three
 * steps bound the trim for invalid UTF-8 too.  Snippets of an overlapping search, or with context > 0, may overlap one another:
 * they are independent copies.  The bytes are the caller's own (a case-insensitive handle matches on a folded copy and cuts
 * the unfolded bytes).  context >= 2^63 and any other flag bit: ACX_EINVAL.
 * The result, n = the number of matches:
 *   ACX_SNIP_DATA         offsets[n] bytes: the snippets back to back
 *   ACX_SNIP_OFFSETS      n + 1 int64 words from 0: snippet i = data[offsets[i] .. offsets[i + 1])
 *   ACX_SNIP_PATTERN      n int64 words: the pattern of match i (the column of acx_find_columns*)
 *   ACX_SNIP_LEAD         n int64 words: the bytes of snippet i in front of the match, which begins at data[offsets[i] + lead[i]]
 *   ACX_SNIP_ROW_OFFSETS  a batch only: rows + 1 int64 words from 0 to n, the CSR form over snippets
 * acx_snippets: host haystacks (offsets: n_hay + 1, or NULL: one haystack of len bytes, no row offsets), a host result.
 * acx_find / acx_find_batch runs as it is and chooses its own route; the records cross the bus and acx_snippets_host cuts.
 * acx_snippets_device: acx_find_device's pipeline (d_offsets / uniform_len as there; neither: one haystack, acx_snippets_rows is
 * 0 and there are no row offsets), then the stage on the same stream: the result lies in HBM on the automaton's device.  The
 * call returns when the size of the data is known (8 bytes cross the bus); the gather may still run: acx_snippets_data / _copy
 * wait for it.  d_hay and d_offsets must stay valid and unchanged until then.  An overlapping search on a handle that is not
 * Standard is ACX_EOVERLAP before any device state; a result block that cannot be allocated is ACX_ENOMEM. */
#define ACX_SNIP_DATA 0
#define ACX_SNIP_OFFSETS 1
#define ACX_SNIP_PATTERN 2
#define ACX_SNIP_LEAD 3
#define ACX_SNIP_ROW_OFFSETS 4
#define ACX_SNIPPET_UTF8 1 /* acx_snippets* flags: the ends move inward to a character boundary */
typedef struct acx_snippets acx_snippets_t;
int acx_snippets(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets /* NULL: one haystack */,
                 uint64_t n_hay, int overlapping, uint64_t context, uint32_t flags, acx_snippets_t **out);
int acx_snippets_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                        uint64_t uniform_len, int overlapping, uint64_t context, uint32_t flags, acx_snippets_t **out);
uint64_t acx_snippets_count(const acx_snippets_t *s);  /* n: the snippets; valid when the call has returned     */
uint64_t acx_snippets_rows(const acx_snippets_t *s);   /* the rows of the batch; 0: one haystack                */
uint64_t acx_snippets_nbytes(const acx_snippets_t *s); /* the size of the data; valid when the call has returned */
int acx_snippets_on_device(const acx_snippets_t *s);   /* 1: the parts are in HBM, 0: host memory               */
/* host or device pointer by acx_snippets_on_device: part `which` (ACX_SNIP_*); waits for the device stage.  NULL: no such part
 * (the single form has no row offsets), or the wait failed.  Valid until acx_free_snippets. */
const void *acx_snippets_data(const acx_snippets_t *s, int which);
int acx_snippets_copy(const acx_snippets_t *s, int which, void *host_dst);
void acx_free_snippets(acx_snippets_t *s);
/* the cut itself, over a caller's records: the definition above, whatever the records say.
 * acx_snippets_host: host memory, no device needed -- the definition inside the library; m: n_m records, all rows behind one
 * another, counts[h] of them row h's (ACX_EINVAL when they do not sum to n_m), or counts = NULL: one row holds them all;
 * offsets: n_hay + 1 from 0 to len (ACX_EINVAL when they do not rise from 0 to len), or NULL: one row of len bytes.  A
 * two-call form: every output may be NULL (not wanted) and *total is always set -- sizes first, then the fill.  out_offsets:
 * n_m + 1 words; pattern, lead: n_m words; row_offsets: n_hay + 1 words (one row: 2); data: *total bytes.
 * acx_snippets_rows_device: the device stage alone on a caller's records and counts (they must sum to n: checked before a
 * kernel reads a record by them, and before anything is written) and bytes, cut by d_offsets, by uniform_len, or one row, in
 * HBM on one device; needs no automaton; synchronous: the outputs are complete when it returns.  d_out_offsets: n + 1 words;
 * d_pattern, d_lead: n words; d_row_offsets: n_hay + 1 words -- all written, every pointer 8-byte aligned; d_data: 16-byte
 * aligned, data_capacity bytes.  *total is reported whenever the sizes were made; total > data_capacity: nothing is stored to
 * d_data and the call returns ACX_ETOOBIG (the other outputs are complete).  Exactly *total bytes are written at d_data and
 * nothing behind them -- there is no round-up.  n = 0 writes the zero offsets and launches nothing else (the counts are not
 * read). */
int acx_snippets_host(const acx_match_t *m, uint64_t n_m, const uint64_t *counts /* NULL: one row */, uint64_t n_hay,
                      const uint8_t *hay, uint64_t len, const uint64_t *offsets /* NULL: one row */, uint64_t context,
                      uint32_t flags, int64_t *out_offsets, int64_t *pattern, int64_t *lead, int64_t *row_offsets,
                      uint8_t *data /* NULL: sizes only */, uint64_t *total);
int acx_snippets_rows_device(const acx_match_t *d_records, uint64_t n, const uint64_t *d_counts, uint64_t n_hay, const void *d_hay,
                             uint64_t len, const uint64_t *d_offsets, uint64_t uniform_len, uint64_t context, uint32_t flags,
                             int64_t *d_out_offsets, int64_t *d_pattern, int64_t *d_lead, int64_t *d_row_offsets, uint8_t *d_data,
                             uint64_t data_capacity, uint64_t *total);

/* ---- whole-word matching: grep -w for a dictionary.  Per row B of L bytes, on the caller's own bytes (a case-insensitive
 * handle matches on its folded copy, the neighbour test reads the unfolded bytes), with a word set W of byte values:
 *   Occ  every (p, s, e) with B[s:e] equal to pattern p -- what the handle's overlapping find reports, copies of equal patterns
 *        included
 *   WW   the (p, s, e) of Occ with (s == 0 or B[s - 1] not in W) and (e == L or B[e] not in W).  A row's end is a boundary; the
 *        pattern's own bytes are not looked at: the lookaround form (?<![W])(?:...)(?![W]), not \b.
 * overlapping != 0: the result is WW in the overlapping find's order (end ascending, longer first, pattern index).
 * overlapping == 0: pos = 0; among the records of WW with s >= pos the least by the kind's key is reported, pos = its e, and
 * again -- the keys: ACX_MATCH_LEFTMOST_FIRST (s, p), ACX_MATCH_LEFTMOST_LONGEST (s, -e, p), ACX_MATCH_STANDARD (e, s, p).
 * That is not a filter over the kind's own find: with "he cat" and "cat" on "the cat" a leftmost find reports "he cat" at 1,
 * no whole word, which shadows the whole word "cat" at 4.
 * word_set: 32 bytes, byte v is a word byte iff word_set[v >> 3] >> (v & 7) & 1 -- host memory in every form; NULL: ASCII
 * [0-9A-Za-z_].  match_kind outside the three is ACX_EINVAL.
 * acx_find_words / acx_find_words_device: the haystack arguments of acx_find_columns / _device, byte offsets, the result an
 * acx_columns_t -- its accessors as they are.  The stage's find is an overlapping one: a handle that is not Standard is
 * ACX_EOVERLAP before any device state is touched, and match_kind is the resolve's kind, not the handle's.  Host haystacks
 * give a host result: up to ACX_WORDS_HOST_MAX bytes (the environment, read per call; 1 MiB) acx_find / acx_find_batch runs
 * as it is and acx_words_host resolves, beyond that the bytes are staged and the device route runs.  The device form returns
 * when the number of matches is known (overlapping == 0: the number of whole words crosses the bus before it); the last
 * kernel may still run and the accessors wait for it.  ACX_ETOOBIG: 2^38 bytes or 2^32 occurrences in one call.
 * acx_filter_words / acx_filter_words_device: acx_filter / acx_filter_device with a row's matches counted after the whole-word
 * stage -- the find, the stage, then the row filter on the new counts. */
int acx_find_words(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets /* NULL: one haystack */,
                   uint64_t n_hay, int overlapping, int match_kind, const uint8_t *word_set /* NULL: the default */,
                   acx_columns_t **out);
int acx_find_words_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                          uint64_t uniform_len, int overlapping, int match_kind, const uint8_t *word_set, acx_columns_t **out);
int acx_filter_words(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets /* NULL: one row */,
                     uint64_t n_hay, int overlapping, int match_kind, const uint8_t *word_set, uint64_t min_matches,
                     uint32_t flags, acx_filtered_t **out);
int acx_filter_words_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                            uint64_t uniform_len, int overlapping, int match_kind, const uint8_t *word_set, uint64_t min_matches,
                            uint32_t flags, acx_filtered_t **out);
/* The stage alone.  m: n_m records, all rows behind one another, counts[h] of them row h's (ACX_EINVAL when they do not sum to
 * n_m), or counts = NULL: one row holds them all; offsets: n_hay + 1 from 0 to len (ACX_EINVAL otherwise), or NULL: one row.
 * out_m: room for n_m records, the first *n_out are written, row by row in the definition's order; out_counts: n_hay words
 * (one row: 1), the rows' new counts.  A record with start >= end or end beyond its row is no occurrence and is dropped.
 * acx_words_host: host memory, no device needed -- the definition inside the library, memory-safe for any records (a row's
 * records are sorted by the kind's key, whatever their order).
 * acx_words_rows_device: the device stage on a caller's records, counts and bytes (d_offsets / uniform_len as for
 * acx_find_device, neither: one row; word_set stays host memory), synchronous: the outputs are complete when it returns.
 * Records, counts, offsets and outputs 8-byte aligned, d_hay at any address.  It relies on a row's records being in the
 * overlapping find's order (for other orders it is memory-safe, not the definition); d_out_m / d_out_counts feed every
 * acx_*_rows_device stage.  ACX_ETOOBIG: len >= 2^38, n_m >= 2^32, or (leftmost kinds) a pattern of 2^24 or more. */
int acx_words_host(const uint8_t *hay, uint64_t len, const uint64_t *offsets /* NULL: one row */, uint64_t n_hay,
                   const acx_match_t *m, uint64_t n_m, const uint64_t *counts /* NULL: one row */, int overlapping, int match_kind,
                   const uint8_t *word_set /* NULL: the default */, acx_match_t *out_m, uint64_t *out_counts /* NULL: not wanted */,
                   uint64_t *n_out);
int acx_words_rows_device(const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay, uint64_t uniform_len,
                          const acx_match_t *d_m, uint64_t n_m, const uint64_t *d_counts, int overlapping, int match_kind,
                          const uint8_t *word_set, acx_match_t *d_out_m, uint64_t *d_out_counts, uint64_t *n_out);

/* ---- token labels: a search's matches mapped onto token boundaries -- a loss mask over tokens, weak-NER (BIO) labels, "which
 * tokens does the block list touch" -- the step behind acx_mask ("after a byte-to-token map") and acx_spans.  It extends the
 * match list of src/lib.rs:229-249 (str: character indexes, 73-88) and 423-435 (bytes) by the map a tokenizer's offset_mapping
 * needs; the matches are those acx_find_batch / acx_find_device reports for the same match kind and `overlapping`.
 * THE DEFINITION.  Tokens t = 0 .. T - 1 are given by two ascending arrays ts[t], te[t] with ts[t] <= te[t] <= ts[t + 1]:
 * GLOBAL positions in the unit of the row offsets, counted from where the first row begins (a partition by T + 1 boundaries
 * `tok` is ts = tok, te = tok + 1; tokens may leave gaps, cross rows and be empty).  A record of row h is clipped to its row
 * first (end' = min(end, row length), start' = min(start, end')); its global range is [g_s, g_e) = [off[h] + start',
 * off[h] + end'), and an empty one touches nothing.  A record TOUCHES token t iff ts[t] < g_e and te[t] > g_s: a zero-length
 * token strictly inside a match is touched, one on a match's edge is not.  The OWNER of t is the touching record with the
 * smallest index in the find's order.  pattern[t] (int64) = the owner's pattern, or -1; begin[t] (uint8) = 1 iff t has an owner
 * and (t == 0 or token t - 1 has another owner or none): the B of BIO; pattern >= 0 is the token mask.
 * acx_tokens: host haystacks (offsets: n_hay + 1, or null: one haystack of len bytes) and host token arrays, a host result.
 * acx_find / acx_find_batch runs as it is, then acx_tokens_host.  codepoints != 0: the search reports character indexes, the
 * rows are measured in characters and so are the tokens (a tokenizer's offset_mapping over str rows).  Token arrays that do
 * not rise or pass the data: ACX_EINVAL before any device work.
 * acx_tokens_device: acx_find_device's pipeline (d_offsets / uniform_len as there; neither: one row; byte offsets), then the
 * device stage on the same stream; d_ts / d_te: n_tokens int64 words each in HBM on the automaton's device, 8-byte aligned.
 * The columns stay in HBM.  The call may return with the stage in flight: the accessors wait for it; d_hay, d_offsets, d_ts and
 * d_te must stay valid until then.  The device form does NOT verify the token arrays -- they are the caller's word, as row
 * offsets are: arrays that do not rise give wrong labels, never a store outside the n_tokens-entry columns.  A
 * case-insensitive handle searches its folded copy; no byte is output.  An overlapping search on a non-Standard handle:
 * ACX_EOVERLAP before any device state is touched.  ACX_ETOOBIG: 2^32 tokens or more, 2^41 records or more.
 * An empty part still has a valid, non-null address. */
typedef struct acx_token_labels acx_token_labels_t;
int acx_tokens(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets /* NULL: one haystack */,
               uint64_t n_hay, int overlapping, int codepoints, const int64_t *ts, const int64_t *te, uint64_t n_tokens,
               acx_token_labels_t **out);
int acx_tokens_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                      uint64_t uniform_len, int overlapping, const int64_t *d_ts, const int64_t *d_te, uint64_t n_tokens,
                      acx_token_labels_t **out);
uint64_t acx_token_labels_count(const acx_token_labels_t *l); /* T: the tokens                                   */
int acx_token_labels_on_device(const acx_token_labels_t *l);  /* 1: the columns are in HBM, 0: host memory       */
/* host or device pointer by acx_token_labels_on_device (T int64 words; T bytes); waits for the device stage.  NULL: the wait
 * failed.  Valid until acx_free_token_labels. */
const int64_t *acx_token_labels_pattern(const acx_token_labels_t *l);
const uint8_t *acx_token_labels_begin(const acx_token_labels_t *l);
int acx_token_labels_copy_pattern(const acx_token_labels_t *l, int64_t *host_dst);
int acx_token_labels_copy_begin(const acx_token_labels_t *l, uint8_t *host_dst);
void acx_free_token_labels(acx_token_labels_t *l);
/* the labels themselves, over a caller's records (both CLIP a record to its row, as acx_mask_host does).
 * acx_tokens_host: host memory, no device needed, any unit -- the definition above inside the library; m: n_m matches, all rows
 * behind one another, counts[h] of them row h's (ACX_EINVAL when they do not sum to n_m), or counts = NULL: one row holds them
 * all; offsets: n_hay + 1 from 0 to len (ACX_EINVAL otherwise), or NULL: one row of len positions; ts, te: n_tokens words each
 * -- ACX_EINVAL unless ts[t] <= te[t] <= ts[t + 1] and te[n_tokens - 1] <= len; pattern: n_tokens words, begin: n_tokens bytes.
 * acx_tokens_rows_device: the device stage alone on a caller's offsets (or uniform_len, or neither: one row of len), records,
 * counts (they must sum to n: checked before a kernel reads a record by them) and token arrays in HBM on one device; needs no
 * automaton and reads no haystack; synchronous: both columns are complete when it returns.  It writes exactly n_tokens words
 * at d_pattern and n_tokens bytes at d_begin.  The word arrays and d_pattern are 8-byte aligned, d_begin lies at any address.
 * n = 0, n_hay = 0 or len = 0: the fills (pattern = -1, begin = 0) and nothing else; n_tokens = 0: nothing at all. */
int acx_tokens_host(const acx_match_t *m, uint64_t n_m, const uint64_t *counts /* NULL: one row */, uint64_t n_hay,
                    const uint64_t *offsets /* NULL: one row */, uint64_t len, const int64_t *ts, const int64_t *te,
                    uint64_t n_tokens, int64_t *pattern, uint8_t *begin);
int acx_tokens_rows_device(uint64_t len, const uint64_t *d_offsets, uint64_t n_hay, uint64_t uniform_len,
                           const acx_match_t *d_records, uint64_t n, const uint64_t *d_counts, const int64_t *d_ts,
                           const int64_t *d_te, uint64_t n_tokens, int64_t *d_pattern, uint8_t *d_begin);

/* ---- match at: "does a pattern begin exactly HERE" -- the crate's anchored search (Anchored::Yes, StartKind::Anchored), for
 * a list of positions or for the start of every row: prefix classification of rows (block lists of URL schemes, log levels,
 * routing by key prefix), whole-row dictionary lookup (the row IS a pattern: strings become ids without a hash table),
 * dictionary entries that begin at a token start.  No find runs and no byte beyond the longest pattern is read per anchor.
 * THE DEFINITION.  Patterns P_i; data h[0 .. len) (a case-insensitive handle compares every byte folded); anchors (p, L), a
 * position and a limit with p <= L <= len.  The candidates of an anchor are C(p, L) = { (i, e) : e = p + len(P_i), e <= L,
 * h[p .. e) == P_i }; p == L has none.  Not overlapping, by the handle's own match kind, one (pattern, end) per anchor or
 * (-1, -1) when C is empty: Standard -- the smallest e, then the smallest i (the crate reports at the first match state);
 * LeftmostFirst -- the smallest i (re.match of the alternation P_0|P_1|...); LeftmostLongest -- the largest e, then the
 * smallest i.  ACX_AT_OVERLAPPING (Standard handles only, ACX_EOVERLAP otherwise, before any device state is touched): all
 * of C, ordered by e ascending, then i ascending, as a CSR over the anchors -- anchor k's entries are row_offsets[k] ..
 * row_offsets[k + 1] - 1.  ACX_AT_FULL (valid only with ACX_AT_ROW_STARTS, ACX_EINVAL otherwise): C is first restricted to
 * e == L -- the row equals the pattern; every kind then reports the smallest i.
 * ROWS.  One haystack: L = len.  Data cut by offsets, by uniform_len or by neither: the row of p is the LAST row r that
 * begins at or before p and L is where row r + 1 begins (of several rows with one start all but the last are empty): a match
 * never crosses a row, and `end` is a position in the data.  ACX_AT_ROW_STARTS: the anchors ARE the rows -- positions is NULL
 * and ignored, there is one result per row, and `end` is local to the row: the length of the match.
 * acx_match_at: host data (offsets: n_hay + 1 from 0 to len, or NULL: one haystack) and host positions, a host result.  The
 * data and the positions are staged to the device, the same kernels run and the columns come back: there is no CPU matching
 * route.  Before any device work: ACX_EINVAL for offsets that do not rise from 0 to len and for a position outside
 * [0, units].  codepoints != 0: positions and ends are CHARACTER indexes of UTF-8 data (units: its characters; else: len).
 * acx_match_at_device: everything in HBM on the automaton's device (d_offsets / uniform_len as for acx_find_device; neither:
 * one row); d_positions: n_pos int64 words, 8-byte aligned.  It runs on the handle's context and stream and returns when the
 * result's size is known; every accessor waits for the kernels, and d_hay, d_offsets and d_positions must stay valid until
 * then.  Device positions are the caller's word, as offsets are: one outside [0, len] -- a negative one included -- gives
 * (-1, -1) or no entry; nothing outside the data is read and nothing outside the outputs is written.  A case-insensitive
 * handle folds the bytes it loads: no folded copy is made and the caller's memory is never written.  Positions need not be
 * sorted and may repeat.  ACX_ETOOBIG: 2^32 anchors or more.
 * acx_match_at_into_device: the raw form, not overlapping -- the two columns go to the caller's d_pattern and d_end (an int64
 * word per anchor each, 8-byte aligned, in HBM on the automaton's device); exactly that many words are written, and both
 * columns are complete when it returns.
 * acx_match_at_host: host memory only, no device -- the definition walked over the compiled tables (first_child, in_byte,
 * own_off, own_pid of acx_host_tables), for match_kind's rule.  Not a matching path of the library: it documents the walk and
 * checks that the tables mean what the kernels assume.  Not overlapping: pattern, end: an entry per anchor.  Overlapping:
 * row_offsets (anchors + 1 words) is written, and -- unless both are NULL: count only -- pattern and end take
 * row_offsets[anchors] entries.  ACX_EINVAL for offsets that do not rise from 0 to len and positions outside [0, len].
 * An empty part still has a valid, non-null address. */
#define ACX_AT_OVERLAPPING 1u
#define ACX_AT_FULL 2u
#define ACX_AT_ROW_STARTS 4u
#define ACX_AT_PATTERN 0     /* acx_at_copy: the parts of a result */
#define ACX_AT_END 1
#define ACX_AT_ROW_OFFSETS 2
typedef struct acx_at acx_at_t;
int acx_match_at(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets /* NULL: one haystack */,
                 uint64_t n_hay, const int64_t *positions, uint64_t n_pos, uint32_t flags, int codepoints, acx_at_t **out);
int acx_match_at_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                        uint64_t uniform_len, const int64_t *d_positions /* int64, 8-byte aligned; NULL with ACX_AT_ROW_STARTS */,
                        uint64_t n_pos, uint32_t flags, acx_at_t **out);
int acx_match_at_into_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                             uint64_t uniform_len, const int64_t *d_positions, uint64_t n_pos, uint32_t flags,
                             int64_t *d_pattern, int64_t *d_end);
int acx_match_at_host(const acx_host_automaton_t *h, const uint8_t *hay, uint64_t len, const uint64_t *offsets /* NULL: one row */,
                      uint64_t n_hay, const int64_t *positions, uint64_t n_pos, uint32_t flags, int match_kind, int64_t *pattern,
                      int64_t *end, int64_t *row_offsets);
uint64_t acx_at_count(const acx_at_t *r);   /* the anchors                                         */
uint64_t acx_at_entries(const acx_at_t *r); /* the entries of the two columns (not overlapping: the anchors) */
int acx_at_on_device(const acx_at_t *r);    /* 1: the columns are in HBM, 0: host memory           */
/* host or device pointer by acx_at_on_device (entries int64 words; anchors + 1 words, NULL unless the call was overlapping);
 * waits for the device stage.  NULL: the wait failed.  Valid until acx_free_at. */
const int64_t *acx_at_pattern(const acx_at_t *r);
const int64_t *acx_at_end(const acx_at_t *r);
const int64_t *acx_at_row_offsets(const acx_at_t *r);
int acx_at_copy(const acx_at_t *r, int which /* ACX_AT_PATTERN .. */, void *host_dst);
void acx_free_at(acx_at_t *r);

/* ---- segment: greedy longest-match tokenization -- cut the data into dictionary entries from left to right, always the entry
 * the handle's match kind prefers at the current position, and go on where it ended.  A LeftmostLongest handle gives MaxMatch
 * (WordPiece's inner loop, forward maximum matching of CJK text, any vocabulary-driven tokenizer); a LeftmostFirst one gives
 * re.finditer of P_0|P_1|...|. .  No find runs.
 * THE DEFINITION.  Patterns P_i; data h[0 .. len) cut into rows (offsets, uniform_len, or neither: one row); a
 * case-insensitive handle compares every byte folded.  For a row [b, L) the pieces are built by a loop: p = b; while p < L:
 * (1) (i, e) = the non-overlapping acx_match_at result of the anchor (p, L) under the handle's own match kind -- a match never
 * crosses the row; (2) a match: the piece is (i, p, e) and p = e; (3) none: the piece is (-1, p, p + u) and p = p + u, u
 * being the unknown unit: 1 byte, or with ACX_SEG_UTF8 the length the lead byte h[p] announces -- 2, 3, 4 for 0xC0..0xDF,
 * 0xE0..0xEF, 0xF0..0xF7, 1 for everything else, a stray continuation byte included -- shortened to the run of continuation
 * bytes (0x80..0xBF) that actually follows, and clipped to L.  The pieces of a row tile it exactly; an empty row has none.
 * THE RESULT, three parts: pattern -- T int64 words, the pattern or -1; offsets -- T + 1 int64 words, the GLOBAL ascending piece
 * boundaries, offsets[T] = len (the token boundaries acx_tokens_device takes as d_ts = offsets, d_te = offsets + 1);
 * row_offsets -- rows + 1 int64 words, entry r the number of pieces that begin before row r does, the last one T.  There is
 * no overlapping form: the chain is defined by one choice per position.
 * acx_segment: host data and host offsets (n_hay + 1 from 0 to len, or NULL: one haystack), a host result.  The data is
 * staged to the device, the same kernels run and the block comes back: there is no CPU matching route.  codepoints != 0
 * implies ACX_SEG_UTF8, and `offsets` come back as CHARACTER indexes of UTF-8 data, converted on the host.
 * acx_segment_device: everything in HBM on the automaton's device (d_offsets / uniform_len as for acx_find_device; neither:
 * one row).  It runs on the handle's context and stream and returns when T is known -- 8 bytes cross the bus; every accessor
 * waits for the kernels, and d_hay and d_offsets must stay valid until then.  Device offsets are the caller's word: wrong
 * ones give wrong pieces, never a read outside the data or a write outside the result.  A case-insensitive handle folds the
 * bytes it loads: no folded copy is made and the caller's memory is never written.
 * acx_segment_into_device: the raw synchronous form -- d_pattern (cap words), d_offsets_out (cap + 1 words) and d_row_offsets
 * (rows + 1 words), int64, 8-byte aligned, in HBM on the automaton's device.  *n_pieces is always T; the three are written
 * only when T <= cap, exactly T, T + 1 and rows + 1 words, and are complete when it returns.
 * acx_segment_host: host memory only, no device -- the definition walked over the compiled tables (first_child, in_byte,
 * own_off, own_pid of acx_host_tables), for match_kind's rule.  Not a matching path of the library: it documents the chain and
 * checks the kernels.  Same outputs and the same cap rule as the raw form (cap = 0: count only, the three may be NULL).
 * Refusals, before any device work and in this order: ACX_EINVAL -- unknown flags, host offsets that do not rise from 0 to
 * len; ACX_ETOOBIG -- a handle with a pattern longer than 256 bytes (dictionary entries are words: the longest step of the
 * chain is the width of the per-tile entry maps); ACX_ETOOBIG -- more than 2^31 - 1 tiles of 4096 bytes, or 2^38 rows.
 * An empty part still has a valid, non-null address. */
#define ACX_SEG_UTF8 1u
#define ACX_SEG_PATTERN 0     /* acx_seg_copy: the parts of a result */
#define ACX_SEG_OFFSETS 1
#define ACX_SEG_ROW_OFFSETS 2
typedef struct acx_seg acx_seg_t;
int acx_segment(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets /* NULL: one haystack */,
                uint64_t n_hay, uint32_t flags, int codepoints, acx_seg_t **out);
int acx_segment_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                       uint64_t uniform_len, uint32_t flags, acx_seg_t **out);
int acx_segment_into_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                            uint64_t uniform_len, uint32_t flags, uint64_t cap, int64_t *d_pattern, int64_t *d_offsets_out,
                            int64_t *d_row_offsets, uint64_t *n_pieces);
int acx_segment_host(const acx_host_automaton_t *h, const uint8_t *hay, uint64_t len, const uint64_t *offsets /* NULL: one row */,
                     uint64_t n_hay, uint32_t flags, int match_kind, uint64_t cap, int64_t *pattern, int64_t *offsets_out,
                     int64_t *row_offsets, uint64_t *n_pieces);
uint64_t acx_seg_count(const acx_seg_t *r); /* T: the pieces                                      */
uint64_t acx_seg_rows(const acx_seg_t *r);  /* the rows (one haystack that is no batch: 1)        */
int acx_seg_on_device(const acx_seg_t *r);  /* 1: the columns are in HBM, 0: host memory          */
/* host or device pointer by acx_seg_on_device (T, T + 1 and rows + 1 int64 words); waits for the device stage.  NULL: the wait
 * failed.  Valid until acx_free_seg. */
const int64_t *acx_seg_pattern(const acx_seg_t *r);
const int64_t *acx_seg_offsets(const acx_seg_t *r);
const int64_t *acx_seg_row_offsets(const acx_seg_t *r);
int acx_seg_copy(const acx_seg_t *r, int which /* ACX_SEG_PATTERN .. */, void *host_dst);
void acx_free_seg(acx_seg_t *r);

/* ---- wordpiece: WordPiece tokenization by the dictionary -- the data is cut into words by a class per byte value and every
 * word into vocabulary entries, continuation entries behind the first one; a word that cannot be cut completely is ONE
 * unknown piece.  No find runs.
 * THE DEFINITION.  Patterns P_i: the vocabulary exactly as a vocab.txt lists it, whole-word entries as they are, continuation
 * entries with the prefix.  A continuation prefix C (prefix, prefix_len): any bytes, possibly none.  Data h[0 .. len) cut into
 * rows (offsets, uniform_len, or neither: one row).  cls[256]: a class per byte VALUE -- ACX_WP_WORD, ACX_WP_SPACE (a
 * separator: it belongs to no word and yields no piece) or ACX_WP_ALONE (a byte that is a word by itself, such as
 * punctuation).  M = max_word, 1 <= M <= ACX_WP_MAX_WORD.  unk_id: any int64.  A case-insensitive handle compares pattern
 * bytes folded; cls is applied to the caller's raw byte.
 * The words of a row [b, L): every ALONE byte is a word of one byte, every maximal run of WORD bytes inside the row is a word;
 * a word never crosses a row.  Equivalently p starts a word iff cls[h[p]] != SPACE and p == b, or cls[h[p]] == ALONE, or
 * cls[h[p - 1]] != WORD.
 * The pieces of a word [ws, we): (1) we - ws > M: ONE piece (unk_id, ws, we).  (2) Otherwise p = ws; while p < we the
 * candidates at p are -- at p == ws every (i, e) with e = p + len(P_i) <= we and h[p .. e) == P_i (acx_match_at's candidates
 * of the anchor (p, we), entries that begin with C included); at p > ws every (i, e) such that P_i begins with C,
 * len(P_i) > len(C), e = p + len(P_i) - len(C) <= we and h[p .. e) == P_i[len(C):] (a pattern equal to C itself is never a
 * continuation piece).  One candidate is picked by the handle's own match kind exactly as for acx_match_at: Standard the
 * smallest e, then the smallest i; LeftmostFirst the smallest i; LeftmostLongest the largest e, then the smallest i.  No
 * candidate: the WHOLE word is ONE piece (unk_id, ws, we), the pieces found before it are withdrawn.  Otherwise the piece is
 * (i, p, e) and p = e.  With LeftmostLongest and whitespace as the separators this is BERT's WordpieceTokenizer.tokenize
 * applied to text.split(), except that the word limit is counted in bytes.
 * THE RESULT, four columns of T entries in data order: id (int64), start and end (int64 GLOBAL byte positions, start strictly
 * ascending), first (uint8: 1 on the first piece of its word); and row_offsets -- rows + 1 int64 words, entry r the number of
 * pieces that begin before row r does, the last one T.  There is no overlapping form.
 * acx_wordpiece: host data and host offsets (n_hay + 1 from 0 to len, or NULL: one haystack), a host result.  The data is
 * staged to the device, the same kernels run and the block comes back: there is no CPU matching route.  codepoints != 0:
 * start and end come back as CHARACTER indexes of UTF-8 data, converted on the host.
 * acx_wordpiece_device: everything in HBM on the automaton's device (d_offsets / uniform_len as for acx_find_device; neither:
 * one row).  It runs on the handle's context and stream and returns when T is known -- 8 bytes cross the bus; every accessor
 * waits for the kernels, and d_hay and d_offsets must stay valid until then.  Device offsets are the caller's word: wrong
 * ones give wrong pieces, never a read outside the data or a write outside the result.  cls and prefix are host memory,
 * read before the call returns.
 * acx_wordpiece_into_device: the raw synchronous form -- d_id, d_start, d_end (cap int64 words each, 8-byte aligned), d_first
 * (cap bytes) and d_row_offsets (rows + 1 int64 words) in HBM on the automaton's device.  *n_pieces is always T; the five are
 * written only when cap != 0 and T <= cap, exactly T, T, T, T and rows + 1 entries, and are complete when it returns.
 * cap = 0 runs the count pass alone: nothing is written and the five may be NULL.
 * acx_wordpiece_host: host memory only, no device -- the definition walked over the compiled tables (first_child, in_byte,
 * own_off, own_pid of acx_host_tables), for match_kind's rule.  Not a matching path of the library: it documents the pieces
 * and checks the kernels.  Same outputs and the same cap rule as the raw form.
 * Refusals, before any device work and in this order: ACX_EINVAL -- unknown flags (none is defined), a cls value above 2,
 * max_word outside 1 .. ACX_WP_MAX_WORD, host offsets that do not rise from 0 to len; ACX_ETOOBIG -- more than 2^31 - 1 tiles
 * of 4096 bytes, or 2^38 rows.  Pattern length is not limited: a pattern longer than the word cannot match.  A prefix whose
 * path is not in the trie is valid: no continuation ever matches.  An empty part still has a valid, non-null address. */
#define ACX_WP_WORD 0         /* cls: the classes of the byte values */
#define ACX_WP_SPACE 1
#define ACX_WP_ALONE 2
#define ACX_WP_MAX_WORD 1024u /* the largest max_word */
#define ACX_WP_ID 0           /* acx_wp_copy: the parts of a result */
#define ACX_WP_START 1
#define ACX_WP_END 2
#define ACX_WP_FIRST 3
#define ACX_WP_ROW_OFFSETS 4
typedef struct acx_wp acx_wp_t;
int acx_wordpiece(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets /* NULL: one haystack */,
                  uint64_t n_hay, const uint8_t *cls /* 256 */, const uint8_t *prefix, uint64_t prefix_len, uint64_t max_word,
                  int64_t unk_id, uint32_t flags, int codepoints, acx_wp_t **out);
int acx_wordpiece_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                         uint64_t uniform_len, const uint8_t *cls /* 256 */, const uint8_t *prefix, uint64_t prefix_len,
                         uint64_t max_word, int64_t unk_id, uint32_t flags, acx_wp_t **out);
int acx_wordpiece_into_device(acx_automaton_t *a, const void *d_hay, uint64_t len, const uint64_t *d_offsets, uint64_t n_hay,
                              uint64_t uniform_len, const uint8_t *cls /* 256 */, const uint8_t *prefix, uint64_t prefix_len,
                              uint64_t max_word, int64_t unk_id, uint32_t flags, uint64_t cap, int64_t *d_id, int64_t *d_start,
                              int64_t *d_end, uint8_t *d_first, int64_t *d_row_offsets, uint64_t *n_pieces);
int acx_wordpiece_host(const acx_host_automaton_t *h, const uint8_t *hay, uint64_t len, const uint64_t *offsets /* NULL: one row */,
                       uint64_t n_hay, const uint8_t *cls /* 256 */, const uint8_t *prefix, uint64_t prefix_len, uint64_t max_word,
                       int64_t unk_id, uint32_t flags, int match_kind, uint64_t cap, int64_t *id, int64_t *start, int64_t *end,
                       uint8_t *first, int64_t *row_offsets, uint64_t *n_pieces);
uint64_t acx_wp_count(const acx_wp_t *r); /* T: the pieces                                      */
uint64_t acx_wp_rows(const acx_wp_t *r);  /* the rows (one haystack that is no batch: 1)        */
int acx_wp_on_device(const acx_wp_t *r);  /* 1: the columns are in HBM, 0: host memory          */
/* host or device pointer by acx_wp_on_device (T int64 words three times, T bytes, rows + 1 int64 words); waits for the device
 * stage.  NULL: the wait failed.  Valid until acx_free_wp. */
const int64_t *acx_wp_id(const acx_wp_t *r);
const int64_t *acx_wp_start(const acx_wp_t *r);
const int64_t *acx_wp_end(const acx_wp_t *r);
const uint8_t *acx_wp_first(const acx_wp_t *r);
const int64_t *acx_wp_row_offsets(const acx_wp_t *r);
int acx_wp_copy(const acx_wp_t *r, int which /* ACX_WP_ID .. */, void *host_dst);
void acx_free_wp(acx_wp_t *r);

/* ---- measurement hooks (HIP events on the library's stream) ---- */
/* on = 0: off; 1: every call carries the event pair around its scan kernel; N > 1: every N-th call of
 * a context does (the pair costs the dispatch ~6 us: a sampled measurement leaves the other calls
 * alone).  The totals of acx_profile_read cover the measured calls only. */
int acx_profile_enable(acx_automaton_t *a, int on);
int acx_profile_read(acx_automaton_t *a, acx_profile_t *out, int reset);
/* Which way the handle's calls went (always counted, no events involved): out[0] calls finished by the sparse kernels
 * alone, [1] calls that also ran the hot pipeline (a dense stretch of the input costs the groups it lies in, not the
 * call: reference behaviour /root/reference/src/lib.rs:59), [2] hot groups in all, [3] prefix hits beyond their tiles'
 * slots in all, [4] calls on the tile-ordered dense path, [5] calls on its radix-sort form, [6] calls that were redone
 * with a larger overflow list, [7] calls K0 answered, [8] byte ranges searched for calls that were cut (more than 2^32
 * occurrences in one pass: the pieces count in [0 .. 7] as well), [9] calls that were repeated with the WIDE form of the
 * sparse path's post stage (a match every 100 - 500 bytes: the context keeps that form while its inputs are like that),
 * [10] launches of a context's RESIDENT K0 (acx_find on short haystacks: one workgroup stays on the device between the
 * calls of a loop and is fed through pinned host memory -- [7] counts the calls, [10] the launches they cost), [11] calls
 * of acx_find whose haystack (beyond K0's sizes, up to 1 MiB) the scan read IN PLACE from pinned host memory instead of
 * a copy in HBM, [12] calls of acx_replace / acx_replace_device spliced on the device, [13] calls whose haystack a
 * case-insensitive handle folded on the device (the staging buffer in place, or a device haystack into the context's
 * buffer; the calling thread's folding copy into pinned host memory is not counted).  reset != 0 clears the counters. */
#define ACX_PATH_STATS 14
int acx_path_stats(acx_automaton_t *a, uint64_t out[ACX_PATH_STATS], int reset);

/* ---- device memory helpers so that a host without torch can stage data ---- */
int acx_device_alloc(void **d_ptr, uint64_t bytes);
int acx_device_free(void *d_ptr);
int acx_device_upload(void *d_dst, const void *h_src, uint64_t bytes);
int acx_device_download(void *h_dst, const void *d_src, uint64_t bytes);
int acx_device_synchronize(void);
int acx_device_synchronize_on(int device); /* the same on a given device (the calling thread's current device is left alone) */

/* ---- seeded synthetic haystacks generated in HBM (bench / tests).  Bit-exact
 * twins of tests/gen.py gen_uniform (kind 0, alphabet a-z) and gen_textlike
 * (kind 1, patterns of `a` planted every 1024 B). ---- */
int acx_generate_haystack(acx_automaton_t *a, void *d_dst, uint64_t len, int kind,
                          uint64_t seed, uint64_t stream_offset);

#ifdef __cplusplus
}
#endif
#endif /* ACX_H */
