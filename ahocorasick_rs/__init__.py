"""`ahocorasick_rs` -- the reference's package name, served by the MI355X-native build.

The reference package is a façade over its native submodule
(/root/reference/pysrc/ahocorasick_rs/__init__.py:2-7; module `ahocorasick_rs.ahocorasick_rs`
declared at /root/reference/src/lib.rs:438-445).  This package has the same shape:
`ahocorasick_rs.ahocorasick_rs` resolves to the C++ CPython extension of
`ahocorasick_rs_amd` (HIP kernels behind include/acx.h), so existing callers --
`import ahocorasick_rs; ahocorasick_rs.AhoCorasick(...)` -- run unchanged.

`__acx_amd__` marks this build: bench.py's probe for a genuine Rust wheel (BASELINE.md §2
step 1) skips any module that carries it, and searches with this repository removed from
sys.path, so a real wheel installed in site-packages is never shadowed during that probe.
"""
from .ahocorasick_rs import (
    AhoCorasick,
    BytesAhoCorasick,
    MatchKind,
    Implementation,
    MatchColumns,
    Column,
    PatternCounts,
    FilteredRows,
    RowScores,
    MaskedRows,
    MatchSpans,
    MatchSnippets,
    TokenLabels,
    MatchesAt,
    Segments,
    WordPieces,
    RowOffsets,
    split_rows,
    ASCII_WORD_BYTES,
    ASCII_WHITESPACE,
    ASCII_PUNCTUATION,
)

__acx_amd__ = True

# Backwards compatibility (reference __init__.py:10-12):
MATCHKIND_STANDARD = MatchKind.Standard
MATCHKIND_LEFTMOST_FIRST = MatchKind.LeftmostFirst
MATCHKIND_LEFTMOST_LONGEST = MatchKind.LeftmostLongest

__all__ = [
    "AhoCorasick",
    "BytesAhoCorasick",
    "MatchKind",
    "Implementation",
    # Extension: the result of find_matches_as_columns / find_matches_as_columns_batch
    "MatchColumns",
    "Column",
    # Extension: the result of count_by_pattern_sparse_batch
    "PatternCounts",
    "FilteredRows",
    # Extension: the result of score_batch
    "RowScores",
    # Extension: the result of mask_all_batch / match_mask_batch
    "MaskedRows",
    # Extension: the result of cover_spans / cover_spans_batch
    "MatchSpans",
    # Extension: the result of find_matches_as_snippets / find_matches_as_snippets_batch
    "MatchSnippets",
    # Extension: the result of label_tokens / label_tokens_batch
    "TokenLabels",
    # Extension: the result of match_at / match_prefix_batch
    "MatchesAt",
    # Extension: the result of segment / segment_batch
    "Segments",
    # Extension: the result of wordpiece / wordpiece_batch
    "WordPieces",
    # Extension: a delimited buffer cut into the rows the _batch methods take (offsets=), and its result
    "split_rows",
    "RowOffsets",
    # Extension: the default word set of find_whole_words_as_columns / _batch and filter_whole_words_batch
    "ASCII_WORD_BYTES",
    # Extension: the default separators of wordpiece / wordpiece_batch, and BertTokenizer's isolated bytes
    "ASCII_WHITESPACE",
    "ASCII_PUNCTUATION",
    # Deprecated:
    "MATCHKIND_STANDARD",
    "MATCHKIND_LEFTMOST_FIRST",
    "MATCHKIND_LEFTMOST_LONGEST",
]
