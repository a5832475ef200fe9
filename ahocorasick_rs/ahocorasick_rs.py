"""Stand-in for the reference's native submodule `ahocorasick_rs.ahocorasick_rs`
(/root/reference/src/lib.rs:438-445): the very same four classes (and the result classes of
find_matches_as_columns, count_by_pattern_sparse_batch, filter_batch, score_batch, mask_all_batch, cover_spans, find_matches_as_snippets, label_tokens, match_at, segment, wordpiece and split_rows, split_rows itself, the whole-word methods' ASCII_WORD_BYTES and wordpiece's ASCII_WHITESPACE and ASCII_PUNCTUATION), re-exported from the C++
CPython extension `ahocorasick_rs_amd.ahocorasick_rs` (one extension, one set of type objects,
so `ahocorasick_rs.MatchKind.Standard is ahocorasick_rs_amd.MatchKind.Standard`)."""
from ahocorasick_rs_amd.ahocorasick_rs import (  # noqa: F401
    AhoCorasick,
    BytesAhoCorasick,
    Column,
    Implementation,
    MatchColumns,
    MatchKind,
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

__all__ = ["ASCII_PUNCTUATION", "ASCII_WHITESPACE", "ASCII_WORD_BYTES", "AhoCorasick", "BytesAhoCorasick", "Column", "FilteredRows", "Implementation", "MatchColumns", "MaskedRows", "MatchKind", "MatchSnippets", "MatchSpans", "MatchesAt", "PatternCounts", "RowOffsets", "RowScores", "Segments", "TokenLabels", "WordPieces", "split_rows"]
