from __future__ import annotations

from typing import Any, Iterable, Optional, Sequence
import sys

if sys.version_info >= (3, 12):
    from collections.abc import Buffer
else:
    from typing_extensions import Buffer

class Implementation:
    NoncontiguousNFA: Implementation
    ContiguousNFA: Implementation
    DFA: Implementation

class MatchKind:
    Standard: MatchKind
    LeftmostFirst: MatchKind
    LeftmostLongest: MatchKind

# extension: the result of find_matches_as_columns / find_matches_as_columns_batch
class Column:
    """One column, 1-D and contiguous, in host memory or in HBM: int64, or uint8 for a FilteredRows' or a MaskedRows' data.  Every accessor
    waits for the device work that writes it first."""
    def __len__(self) -> int: ...
    def __dlpack__(self, stream: Any = None, **ignored: Any) -> Any: ...
    def __dlpack_device__(self) -> tuple[int, int]: ...
    def __buffer__(self, flags: int) -> memoryview: ...  # host columns only: format "q" (uint8: "B"), read-only

class MatchColumns:
    @property
    def pattern(self) -> Column: ...
    @property
    def start(self) -> Column: ...
    @property
    def end(self) -> Column: ...
    @property
    def row_offsets(self) -> Optional[Column]: ...  # None for one haystack; len(haystacks) + 1 entries for a batch
    @property
    def device(self) -> Optional[int]: ...  # None: host memory; otherwise the HIP ordinal
    def __len__(self) -> int: ...
    def tolist(self) -> Any: ...  # what find_matches_as_indexes / _batch returns for the same arguments

# extension: the result of count_by_pattern_sparse_batch -- the CSR form of the haystacks x patterns matrix of match counts
class PatternCounts:
    @property
    def row_offsets(self) -> Column: ...  # shape[0] + 1 entries from 0
    @property
    def pattern(self) -> Column: ...  # len(self) pattern indexes, strictly ascending within a row
    @property
    def count(self) -> Column: ...  # len(self) counts, all >= 1
    @property
    def shape(self) -> tuple[int, int]: ...  # (haystacks, patterns)
    @property
    def device(self) -> Optional[int]: ...  # None: host memory; otherwise the HIP ordinal
    def __len__(self) -> int: ...  # the number of non-zero entries
    def tolist(self) -> list[list[tuple[int, int]]]: ...  # per haystack: (pattern, count), patterns ascending

# extension: the result of filter_batch -- the kept rows of a batch as a compacted batch, where the search ran
class FilteredRows:
    @property
    def rows(self) -> Column: ...  # len(self) int64 entries: the kept source row indexes, strictly ascending
    @property
    def offsets(self) -> Column: ...  # len(self) + 1 int64 entries from 0
    @property
    def data(self) -> Column: ...  # nbytes uint8 entries: kept row i is data[offsets[i]:offsets[i + 1]], the caller's bytes
    @property
    def device(self) -> Optional[int]: ...  # None: host memory; otherwise the HIP ordinal
    @property
    def nbytes(self) -> int: ...  # the size of data
    @property
    def source_rows(self) -> int: ...  # the rows of the batch that was filtered
    def __len__(self) -> int: ...  # the number of kept rows
    def tolist(self) -> Any: ...  # the kept rows: list[str] of AhoCorasick, list[bytes] of BytesAhoCorasick

# extension: the result of score_batch -- one int64 score per row of the batch, where the search ran
class RowScores:
    @property
    def score(self) -> Column: ...  # len(self) int64 entries
    @property
    def device(self) -> Optional[int]: ...  # None: host memory; otherwise the HIP ordinal
    def __len__(self) -> int: ...  # the rows of the batch
    def tolist(self) -> list[int]: ...

# extension: the result of mask_all_batch / match_mask_batch -- the batch's bytes with every byte that a match covers filled
# (mask_all_batch) or the 0 / 1 mask (match_mask_batch), in the input's own layout, where the search ran
class MaskedRows:
    @property
    def data(self) -> Column: ...  # nbytes uint8 entries, one per byte of the input
    @property
    def offsets(self) -> Column: ...  # len(self) + 1 int64 entries from 0: row i is data[offsets[i]:offsets[i + 1]]
    @property
    def device(self) -> Optional[int]: ...  # None: host memory; otherwise the HIP ordinal
    @property
    def nbytes(self) -> int: ...  # the size of data: the input's
    def __len__(self) -> int: ...  # the rows of the batch
    # the rows: list[str] (AhoCorasick.mask_all_batch) or list[bytes].  A sequence of str gives one entry per CHARACTER (the
    # entries of continuation bytes are dropped on the host); a tensor gives the bytes as they are (decoded for list[str])
    def tolist(self) -> Any: ...

# extension: the result of cover_spans / cover_spans_batch -- the union of a search's matches as two int64 columns, where the
# search ran.  Within a row the spans are ascending and disjoint, and next.start - prev.end > gap
class MatchSpans:
    @property
    def start(self) -> Column: ...  # len(self) int64 entries
    @property
    def end(self) -> Column: ...  # len(self) int64 entries
    @property
    def row_offsets(self) -> Optional[Column]: ...  # None for one haystack; len(haystacks) + 1 entries from 0 for a batch
    @property
    def device(self) -> Optional[int]: ...  # None: host memory; otherwise the HIP ordinal
    def __len__(self) -> int: ...  # the number of spans
    def tolist(self) -> Any: ...  # list[tuple[int, int]] of (start, end), or one such list per row of a batch

# extension: the result of find_matches_as_snippets / find_matches_as_snippets_batch -- one snippet per match: the matched
# text and its context as the caller's own bytes, where the search ran.  Snippet i is data[offsets[i]:offsets[i + 1]] and its
# match begins at data[offsets[i] + lead[i]]
class MatchSnippets:
    @property
    def data(self) -> Column: ...  # nbytes uint8 entries: the snippets back to back
    @property
    def offsets(self) -> Column: ...  # len(self) + 1 int64 entries from 0
    @property
    def pattern(self) -> Column: ...  # len(self) int64 entries: the pattern column of find_matches_as_columns
    @property
    def lead(self) -> Column: ...  # len(self) int64 entries: the bytes of snippet i in front of its match
    @property
    def row_offsets(self) -> Optional[Column]: ...  # None for one haystack; len(haystacks) + 1 entries from 0 for a batch
    @property
    def device(self) -> Optional[int]: ...  # None: host memory; otherwise the HIP ordinal
    @property
    def nbytes(self) -> int: ...  # the size of data
    def __len__(self) -> int: ...  # the number of snippets
    def tolist(self) -> Any: ...  # list[str] (AhoCorasick) or list[bytes]; one such list per row of a batch

# extension: the result of label_tokens / label_tokens_batch -- a search's matches mapped onto token boundaries, one entry
# per token, where the search ran.  A match touches token t iff token_start[t] < match.end and token_end[t] > match.start; the
# token's owner is the first touching match in the search's order
class TokenLabels:
    @property
    def pattern(self) -> Column: ...  # len(self) int64 entries: the owner's pattern, or -1; pattern >= 0 is the token mask
    @property
    def begin(self) -> Column: ...  # len(self) uint8 entries: 1 iff the token is the first of its owner's (the B of BIO)
    @property
    def row_offsets(self) -> Optional[list[int]]: ...  # a sequence of haystacks: len(haystacks) + 1 entries from 0; else None
    @property
    def device(self) -> Optional[int]: ...  # None: host memory; otherwise the HIP ordinal
    def __len__(self) -> int: ...  # the number of tokens
    def tolist(self) -> Any: ...  # list[tuple[int, int]] of (pattern, begin), or one such list per haystack of a sequence

# extension: the result of match_at / match_prefix_batch -- the crate's anchored search: which pattern begins exactly at
# every anchor (a position, or the start of a row), where the walk ran.  The candidates of an anchor (p, L) are the patterns
# P_i with haystack[p : p + len(P_i)] == P_i and p + len(P_i) <= L, L being the end of p's row; Standard reports the
# shortest (then the lowest index), LeftmostFirst the lowest index, LeftmostLongest the longest; full=True keeps only
# candidates that end at L
class MatchesAt:
    @property
    def pattern(self) -> Column: ...  # int64: the pattern that begins at the anchor, or -1; overlapping: every such pattern
    @property
    def end(self) -> Column: ...  # int64: where it ends (match_prefix_batch: its length), or -1
    @property
    def row_offsets(self) -> Optional[Column]: ...  # overlapping=True: len(self) + 1 int64 entries that cut the entries by anchor; else None
    @property
    def device(self) -> Optional[int]: ...  # None: host memory; otherwise the HIP ordinal
    def __len__(self) -> int: ...  # the number of anchors
    def tolist(self) -> Any: ...  # list[tuple[int, int]] of (pattern, end), or -- overlapping -- one such list per anchor

# extension: the result of segment / segment_batch -- the data cut into dictionary entries from left to right, where the chain
# ran: at every position the pattern the object's match kind prefers there (what match_at reports), going on where it ended;
# where no pattern begins the piece is an unknown unit with pattern -1 -- one byte, or (utf8) one whole UTF-8 character.  The
# pieces of a row tile it exactly
class Segments:
    @property
    def pattern(self) -> Column: ...  # len(self) int64 entries: the pattern of the piece, or -1
    @property
    def offsets(self) -> Column: ...  # len(self) + 1 int64 GLOBAL ascending boundaries, the last one the data's length: label_tokens_batch's token_offsets
    @property
    def row_offsets(self) -> Optional[Column]: ...  # segment_batch: len(haystacks) + 1 int64 entries that cut the pieces by row; else None
    @property
    def device(self) -> Optional[int]: ...  # None: host memory; otherwise the HIP ordinal
    def __len__(self) -> int: ...  # the number of pieces
    def tolist(self) -> Any: ...  # list[tuple[int, int, int]] of (pattern, start, end) local to the row, or one such list per row

# extension: the result of wordpiece / wordpiece_batch -- the words of the data cut into vocabulary entries, where the chains
# ran: a word's first piece is looked up as it stands, the following ones behind the continuation prefix; a word that is too
# long or cannot be cut completely is ONE piece with unk_id
class WordPieces:
    @property
    def id(self) -> Column: ...  # len(self) int64 entries: the pattern of the piece, or unk_id
    @property
    def start(self) -> Column: ...  # len(self) int64 GLOBAL positions, strictly ascending (characters for a str)
    @property
    def end(self) -> Column: ...  # len(self) int64 GLOBAL positions
    @property
    def first(self) -> Column: ...  # len(self) uint8 entries: 1 iff the piece is the first of its word
    @property
    def row_offsets(self) -> Optional[Column]: ...  # wordpiece_batch: len(haystacks) + 1 int64 entries that cut the pieces by row; else None
    @property
    def device(self) -> Optional[int]: ...  # None: host memory; otherwise the HIP ordinal
    def __len__(self) -> int: ...  # the number of pieces
    def tolist(self) -> Any: ...  # list[tuple[int, int, int, int]] of (id, start, end, first) local to the row, or one such list per row

# extension: the result of split_rows -- the offsets that cut a delimited buffer into rows, where the data lies
class RowOffsets:
    @property
    def offsets(self) -> Column: ...  # len(self) + 1 int64 entries that rise strictly from 0 to nbytes
    @property
    def device(self) -> Optional[int]: ...  # None: host memory; otherwise the HIP ordinal
    @property
    def nbytes(self) -> int: ...  # the length of the data that was cut
    def __len__(self) -> int: ...  # the rows
    def tolist(self) -> list[int]: ...  # the offsets

# extension: 0, then p + 1 for every byte p of data that equals the delimiter, then len(data) if the last byte is not one: the
# delimiter ends its row (splitlines(keepends=True) for "\n") and no row is empty.  data: one 1-D contiguous uint8 __dlpack__
# tensor (on a ROCm device it is cut where it lies, and the offsets stay there) or any contiguous byte buffer; never written.
# delimiter: an int in range(256), a one-byte buffer or a one-character ASCII str (ValueError otherwise; TypeError for
# anything else).  The result's .offsets is what the _batch methods take as offsets= beside the same tensor.
def split_rows(data: Any, delimiter: Any = b"\n") -> RowOffsets: ...

# extension: the default word set of the find_whole_words_* methods, ASCII [0-9A-Za-z_]
ASCII_WORD_BYTES: bytes

# extension: the default separators of wordpiece / wordpiece_batch (b" \t\n\r\x0b\x0c"), and the 32 ASCII bytes BERT's
# _is_punctuation accepts (33-47, 58-64, 91-96, 123-126): isolated=ASCII_PUNCTUATION is the BertTokenizer recipe
ASCII_WHITESPACE: bytes
ASCII_PUNCTUATION: bytes

class AhoCorasick:
    def __init__(
        self,
        patterns: Iterable[str],
        matchkind: MatchKind = MatchKind.Standard,
        store_patterns: Optional[bool] = None,
        implementation: Optional[Implementation] = None,
        ascii_case_insensitive: bool = False,
    ) -> None: ...
    def find_matches_as_indexes(
        self, haystack: str, overlapping: bool = False
    ) -> list[tuple[int, int, int]]: ...
    def find_matches_as_strings(
        self, haystack: str, overlapping: bool = False
    ) -> list[str]: ...
    # extension (not in the reference): one device pass over many haystacks
    def find_matches_as_indexes_batch(
        self, haystacks: Sequence[str], overlapping: bool = False, devices: Optional[Sequence[int]] = None
    ) -> list[list[tuple[int, int, int]]]: ...
    def replace_all(self, haystack: str, replace_with: Iterable[str]) -> str: ...
    def replace_all_batch(self, haystacks: Sequence[str], replace_with: Iterable[str]) -> list[str]: ...
    # extension: summaries of a search without its match list (no early exit: one search over the whole input)
    def is_match(self, haystack: str) -> bool: ...
    def find_first(self, haystack: str) -> Optional[tuple[int, int, int]]: ...
    def count_matches(self, haystack: str, overlapping: bool = False) -> int: ...
    def count_by_pattern(self, haystack: str, overlapping: bool = False) -> list[int]: ...
    def is_match_batch(self, haystacks: Sequence[str]) -> list[bool]: ...
    def find_first_batch(self, haystacks: Sequence[str]) -> list[Optional[tuple[int, int, int]]]: ...
    def count_matches_batch(self, haystacks: Sequence[str], overlapping: bool = False) -> list[int]: ...
    def count_by_pattern_batch(self, haystacks: Sequence[str], overlapping: bool = False) -> list[int]: ...
    # extension: the matches as int64 columns exported through DLPack, no tuple list
    def find_matches_as_columns(self, haystack: str, overlapping: bool = False) -> MatchColumns: ...
    def find_matches_as_columns_batch(self, haystacks: Sequence[str], overlapping: bool = False) -> MatchColumns: ...
    # extension: which patterns occur in which haystack, and how often, as a CSR matrix.  haystacks: a sequence, or ONE 1-D
    # contiguous uint8 __dlpack__ tensor of UTF-8 rows back to back, cut by exactly one of offsets (a 1-D int64 __dlpack__
    # tensor of rows + 1 entries on the same device) and row_length; a tensor on the automaton's device stays there
    def count_by_pattern_sparse_batch(
        self, haystacks: Any, overlapping: bool = False, *, offsets: Any = None, row_length: Optional[int] = None
    ) -> PatternCounts: ...
    # extension: drop the rows that contain a pattern (keep="unmatched") or keep only those that do (keep="matched"; a row
    # is matched when it has at least min_matches matches), compacted where the search ran.  haystacks as for
    # count_by_pattern_sparse_batch: a sequence, or ONE uint8 __dlpack__ tensor cut by exactly one of offsets and row_length
    def filter_batch(
        self, haystacks: Any, overlapping: bool = False, *, keep: str = "unmatched", min_matches: int = 1,
        offsets: Any = None, row_length: Optional[int] = None
    ) -> FilteredRows: ...
    # extension: per-pattern weights (one int per pattern, |w| < 2^31: a sequence of ints or an int64 / int32 buffer).  A row's
    # score is the sum of weights[pattern] over the matches find_matches_as_indexes_batch reports for it (int64, wraps modulo
    # 2^64); filter_by_score_batch is filter_batch with a row matched when its score is at least min_score (any int64).
    # haystacks as for count_by_pattern_sparse_batch
    def score_batch(
        self, haystacks: Any, weights: Any, overlapping: bool = False, *, offsets: Any = None,
        row_length: Optional[int] = None
    ) -> RowScores: ...
    def filter_by_score_batch(
        self, haystacks: Any, weights: Any, overlapping: bool = False, *, keep: str = "unmatched", min_score: int = 1,
        offsets: Any = None, row_length: Optional[int] = None
    ) -> FilteredRows: ...
    # extension: the cover of a search's matches.  mask_all: the haystack with every character that a match covers replaced by
    # fill -- a one-character ASCII str, so the output stays valid UTF-8 (anything else that is a str: ValueError; not a str:
    # TypeError) -- and every other character where it was; match_mask: bytes, 1 where a match covers the character, else 0.
    # Both have one entry per CHARACTER: len(result) == len(haystack).  overlapping=True (Standard only) covers the union of
    # all occurrences.  The _batch forms take haystacks as count_by_pattern_sparse_batch does and return a MaskedRows whose
    # .data and .offsets are in UTF-8 BYTES (a covered k-byte character is k fills): with a tensor the result is byte for
    # byte, since the layout is the point; tolist() of a sequence of str gives one entry per character again
    def mask_all(self, haystack: str, fill: str, overlapping: bool = False) -> str: ...
    def match_mask(self, haystack: str, overlapping: bool = False) -> bytes: ...
    def mask_all_batch(
        self, haystacks: Any, fill: str, overlapping: bool = False, *, offsets: Any = None,
        row_length: Optional[int] = None
    ) -> MaskedRows: ...
    def match_mask_batch(
        self, haystacks: Any, overlapping: bool = False, *, offsets: Any = None, row_length: Optional[int] = None
    ) -> MaskedRows: ...
    # extension: the merged spans of a search's matches -- what find_matches_as_indexes(haystack, overlapping) reports, with
    # matches that overlap, touch or lie at most gap characters apart joined into one (start, end).  Character indexes (a
    # tensor of the _batch form: byte offsets local to the row).  gap: an int 0 .. 2**63 - 1 (ValueError outside; TypeError
    # for a bool or anything that is no int).  With gap=0 the spans are the runs of ones of match_mask.  The _batch form
    # takes haystacks as count_by_pattern_sparse_batch does; spans never join across rows
    def cover_spans(self, haystack: str, overlapping: bool = False, *, gap: int = 0) -> MatchSpans: ...
    def cover_spans_batch(
        self, haystacks: Any, overlapping: bool = False, *, gap: int = 0, offsets: Any = None,
        row_length: Optional[int] = None
    ) -> MatchSpans: ...
    # extension: the matched text and the text around it -- one snippet per match of find_matches_as_columns(haystack,
    # overlapping), in its order: the match and up to context BYTES on each side, clipped to the haystack (a row of the
    # _batch form).  Everything is in UTF-8 bytes, as for MaskedRows; a snippet never splits a character -- its ends move
    # inward to a character boundary, never into the match -- so tolist() is a list[str], and with context=0 it equals
    # find_matches_as_strings(haystack).  The bytes are the caller's own, also under ascii_case_insensitive.  context: an int
    # 0 .. 2**63 - 1 (ValueError outside; TypeError for a bool or anything that is no int).  The _batch form takes haystacks
    # as cover_spans_batch does
    def find_matches_as_snippets(self, haystack: str, overlapping: bool = False, *, context: int = 0) -> MatchSnippets: ...
    def find_matches_as_snippets_batch(
        self, haystacks: Any, overlapping: bool = False, *, context: int = 0, offsets: Any = None,
        row_length: Optional[int] = None
    ) -> MatchSnippets: ...
    # extension: whole-word matching (grep -w).  Of all occurrences of the patterns those whose neighbour bytes -- the byte in
    # front of the match and the byte behind it; the ends of the haystack (of a row) are boundaries -- are no word bytes; of
    # those the non-overlapping ones `matchkind` picks (overlapping=True: all of them).  The object must be a
    # MatchKind.Standard one (ValueError otherwise); matchkind resolves the whole-word occurrences only.  word_bytes: None
    # (ASCII_WORD_BYTES) or a bytes-like of the byte values that count (a str: TypeError).  The _batch forms take haystacks as
    # count_by_pattern_sparse_batch does; filter_whole_words_batch is filter_batch on these matches
    def find_whole_words_as_columns(
        self, haystack: str, overlapping: bool = False, *, matchkind: MatchKind = MatchKind.LeftmostLongest,
        word_bytes: Any = None
    ) -> MatchColumns: ...
    def find_whole_words_as_columns_batch(
        self, haystacks: Any, overlapping: bool = False, *, matchkind: MatchKind = MatchKind.LeftmostLongest,
        word_bytes: Any = None, offsets: Any = None, row_length: Optional[int] = None
    ) -> MatchColumns: ...
    def filter_whole_words_batch(
        self, haystacks: Any, overlapping: bool = False, *, matchkind: MatchKind = MatchKind.LeftmostLongest,
        word_bytes: Any = None, keep: str = "unmatched", min_matches: int = 1, offsets: Any = None,
        row_length: Optional[int] = None
    ) -> FilteredRows: ...
    # extension: the matches of find_matches_as_indexes(haystack, overlapping) mapped onto tokens.  token_offsets: the k + 1
    # boundaries of k tokens, non-decreasing, within 0 .. len(haystack), in CHARACTERS -- the unit of find_matches_as_indexes
    # and of a tokenizer's offset_mapping -- as a sequence of ints or an int64 buffer (ValueError otherwise).  The _batch form
    # takes a sequence of haystacks with one such entry per haystack (a token never crosses a haystack; .row_offsets cuts the
    # tokens by haystack), or ONE uint8 __dlpack__ tensor cut by offsets / row_length as mask_all_batch takes it, with ONE 1-D
    # contiguous int64 __dlpack__ tensor of T + 1 GLOBAL BYTE boundaries on the same device (tokens may cross rows; on the
    # automaton's device everything stays in HBM, the boundaries are the caller's word, as offsets are, and the TokenLabels
    # keeps the input tensors alive until it goes: they must not be written before an accessor of a column has returned)
    def label_tokens(self, haystack: str, token_offsets: Any, overlapping: bool = False) -> TokenLabels: ...
    def label_tokens_batch(
        self, haystacks: Any, token_offsets: Any, overlapping: bool = False, *, offsets: Any = None,
        row_length: Optional[int] = None
    ) -> TokenLabels: ...
    # extension: the anchored search -- for every position the pattern that begins exactly there, by the object's match kind,
    # as (pattern, end) or (-1, -1); overlapping=True (Standard objects only, ValueError otherwise): every such pattern,
    # ordered by end, then by index.  positions: a sequence of ints or an int64 buffer within 0 .. len(haystack), in
    # CHARACTERS, any order, repeats allowed (ValueError outside); ends are character indexes too.  match_prefix_batch: the
    # anchors are the starts of the rows -- a sequence of str -- and end is the length of the match; full=True: only a pattern
    # that IS the row counts (a dictionary lookup: every kind then reports the lowest index).  No search runs
    def match_at(
        self, haystack: str, positions: Any, overlapping: bool = False, *, offsets: Any = None, row_length: Optional[int] = None
    ) -> MatchesAt: ...
    def match_prefix_batch(
        self, haystacks: Any, overlapping: bool = False, *, full: bool = False, offsets: Any = None,
        row_length: Optional[int] = None
    ) -> MatchesAt: ...
    # extension: greedy tokenization by the dictionary (MaxMatch for a LeftmostLongest object, re.finditer of P_0|P_1|...|.
    # for a LeftmostFirst one): the pieces as (pattern, start, end) in CHARACTERS; an unknown piece (pattern -1) is one
    # character.  utf8: None or True (False: ValueError -- a str is cut at characters; anything else: TypeError).  Patterns
    # longer than 256 bytes: ValueError.  No search runs
    def segment(self, haystack: str, *, utf8: Optional[bool] = None) -> Segments: ...
    def segment_batch(
        self, haystacks: Any, *, utf8: Optional[bool] = None, offsets: Any = None, row_length: Optional[int] = None
    ) -> Segments: ...
    # extension: WordPiece tokenization by the dictionary -- the patterns are the vocabulary as a vocab.txt lists it.  A byte
    # in separators (None: ASCII_WHITESPACE) belongs to no word, a byte in isolated (None: none) is a word by itself, every
    # other run is a word; its first piece is looked up as it stands, the following ones behind continuation_prefix, each
    # the entry the object's match kind prefers (LeftmostLongest: BERT's WordpieceTokenizer, the limit counted in bytes).  A
    # word longer than max_word_bytes or with a step that finds nothing is ONE piece with unk_id.  The sets and the prefix:
    # bytes-like or str, the sets ASCII (ValueError otherwise; a byte in both: ValueError).  max_word_bytes: an int in
    # range(1, 1025), unk_id: an int64 (TypeError for a bool or a non-int, ValueError out of range).  Positions in CHARACTERS
    def wordpiece(
        self, haystack: str, *, continuation_prefix: Any = "##", separators: Any = None, isolated: Any = None,
        max_word_bytes: int = 100, unk_id: int = -1
    ) -> WordPieces: ...
    def wordpiece_batch(
        self, haystacks: Any, *, continuation_prefix: Any = "##", separators: Any = None, isolated: Any = None,
        max_word_bytes: int = 100, unk_id: int = -1, offsets: Any = None, row_length: Optional[int] = None
    ) -> WordPieces: ...
    def _info(self) -> dict[str, Any]: ...

class BytesAhoCorasick:
    def __init__(
        self,
        patterns: Iterable[Buffer],
        matchkind: MatchKind = MatchKind.Standard,
        implementation: Optional[Implementation] = None,
        ascii_case_insensitive: bool = False,
    ) -> None: ...
    def find_matches_as_indexes(
        self, haystack: Buffer, overlapping: bool = False
    ) -> list[tuple[int, int, int]]: ...
    def find_matches_as_indexes_batch(
        self, haystacks: Sequence[Buffer], overlapping: bool = False, devices: Optional[Sequence[int]] = None
    ) -> list[list[tuple[int, int, int]]]: ...
    def replace_all(self, haystack: Buffer, replace_with: Iterable[Buffer]) -> bytes: ...
    def replace_all_batch(self, haystacks: Sequence[Buffer], replace_with: Iterable[Buffer]) -> list[bytes]: ...
    # extension: summaries of a search without its match list (no early exit: one search over the whole input)
    def is_match(self, haystack: Buffer) -> bool: ...
    def find_first(self, haystack: Buffer) -> Optional[tuple[int, int, int]]: ...
    def count_matches(self, haystack: Buffer, overlapping: bool = False) -> int: ...
    def count_by_pattern(self, haystack: Buffer, overlapping: bool = False) -> list[int]: ...
    def is_match_batch(self, haystacks: Sequence[Buffer]) -> list[bool]: ...
    def find_first_batch(self, haystacks: Sequence[Buffer]) -> list[Optional[tuple[int, int, int]]]: ...
    def count_matches_batch(self, haystacks: Sequence[Buffer], overlapping: bool = False) -> list[int]: ...
    def count_by_pattern_batch(self, haystacks: Sequence[Buffer], overlapping: bool = False) -> list[int]: ...
    # extension: the matches as int64 columns exported through DLPack (a __dlpack__ tensor on the automaton's device is
    # searched and split where it lies: the columns stay in HBM), no tuple list
    def find_matches_as_columns(self, haystack: Buffer, overlapping: bool = False) -> MatchColumns: ...
    def find_matches_as_columns_batch(self, haystacks: Sequence[Buffer], overlapping: bool = False) -> MatchColumns: ...
    # extension: which patterns occur in which haystack, and how often, as a CSR matrix.  haystacks: a sequence, or ONE 1-D
    # contiguous uint8 __dlpack__ tensor of rows back to back, cut by exactly one of offsets (a 1-D int64 __dlpack__ tensor
    # of rows + 1 entries on the same device) and row_length; a tensor on the automaton's device stays there
    def count_by_pattern_sparse_batch(
        self, haystacks: Any, overlapping: bool = False, *, offsets: Any = None, row_length: Optional[int] = None
    ) -> PatternCounts: ...
    # extension: drop the rows that contain a pattern (keep="unmatched") or keep only those that do (keep="matched"; a row
    # is matched when it has at least min_matches matches), compacted where the search ran.  haystacks as for
    # count_by_pattern_sparse_batch: a sequence, or ONE uint8 __dlpack__ tensor cut by exactly one of offsets and row_length
    def filter_batch(
        self, haystacks: Any, overlapping: bool = False, *, keep: str = "unmatched", min_matches: int = 1,
        offsets: Any = None, row_length: Optional[int] = None
    ) -> FilteredRows: ...
    # extension: per-pattern weights (one int per pattern, |w| < 2^31: a sequence of ints or an int64 / int32 buffer).  A row's
    # score is the sum of weights[pattern] over the matches find_matches_as_indexes_batch reports for it (int64, wraps modulo
    # 2^64); filter_by_score_batch is filter_batch with a row matched when its score is at least min_score (any int64).
    # haystacks as for count_by_pattern_sparse_batch
    def score_batch(
        self, haystacks: Any, weights: Any, overlapping: bool = False, *, offsets: Any = None,
        row_length: Optional[int] = None
    ) -> RowScores: ...
    def filter_by_score_batch(
        self, haystacks: Any, weights: Any, overlapping: bool = False, *, keep: str = "unmatched", min_score: int = 1,
        offsets: Any = None, row_length: Optional[int] = None
    ) -> FilteredRows: ...
    # extension: the cover of a search's matches.  mask_all: the haystack with every byte that a match covers replaced by fill
    # -- an int in range(256) or a one-byte buffer (an int outside the range or a longer buffer: ValueError; anything else:
    # TypeError) -- and every other byte where it was; match_mask: 1 where a match covers the byte, else 0.  overlapping=True
    # (Standard only) covers the union of all occurrences.  The _batch forms take haystacks as
    # count_by_pattern_sparse_batch does and return a MaskedRows in the input's own layout
    def mask_all(self, haystack: Buffer, fill: Any, overlapping: bool = False) -> bytes: ...
    def match_mask(self, haystack: Buffer, overlapping: bool = False) -> bytes: ...
    def mask_all_batch(
        self, haystacks: Any, fill: Any, overlapping: bool = False, *, offsets: Any = None,
        row_length: Optional[int] = None
    ) -> MaskedRows: ...
    def match_mask_batch(
        self, haystacks: Any, overlapping: bool = False, *, offsets: Any = None, row_length: Optional[int] = None
    ) -> MaskedRows: ...
    # extension: the merged spans of a search's matches -- what find_matches_as_indexes(haystack, overlapping) reports, with
    # matches that overlap, touch or lie at most gap bytes apart joined into one (start, end); byte offsets local to the
    # row.  A __dlpack__ tensor on the automaton's device is searched and merged where it lies: the columns stay in HBM.
    # gap: an int 0 .. 2**63 - 1 (ValueError outside; TypeError for a bool or anything that is no int).  With gap=0 the
    # spans are the runs of ones of match_mask.  The _batch form takes haystacks as count_by_pattern_sparse_batch does
    def cover_spans(self, haystack: Any, overlapping: bool = False, *, gap: int = 0) -> MatchSpans: ...
    def cover_spans_batch(
        self, haystacks: Any, overlapping: bool = False, *, gap: int = 0, offsets: Any = None,
        row_length: Optional[int] = None
    ) -> MatchSpans: ...
    # extension: the matched text and the text around it -- one snippet per match of find_matches_as_columns(haystack,
    # overlapping), in its order: the match and up to context bytes on each side, clipped to the haystack (a row of the
    # _batch form); the bytes are the caller's own, also under ascii_case_insensitive.  A __dlpack__ tensor on the automaton's
    # device is searched and cut where it lies: every part stays in HBM.  context: an int 0 .. 2**63 - 1 (ValueError outside;
    # TypeError for a bool or anything that is no int).  The _batch form takes haystacks as cover_spans_batch does
    def find_matches_as_snippets(self, haystack: Any, overlapping: bool = False, *, context: int = 0) -> MatchSnippets: ...
    def find_matches_as_snippets_batch(
        self, haystacks: Any, overlapping: bool = False, *, context: int = 0, offsets: Any = None,
        row_length: Optional[int] = None
    ) -> MatchSnippets: ...
    # extension: whole-word matching (grep -w).  Of all occurrences of the patterns those whose neighbour bytes -- the byte in
    # front of the match and the byte behind it; the ends of the haystack (of a row) are boundaries -- are no word bytes; of
    # those the non-overlapping ones `matchkind` picks (overlapping=True: all of them).  The object must be a
    # MatchKind.Standard one (ValueError otherwise); matchkind resolves the whole-word occurrences only.  word_bytes: None
    # (ASCII_WORD_BYTES) or a bytes-like of the byte values that count (a str: TypeError).  The _batch forms take haystacks as
    # count_by_pattern_sparse_batch does; filter_whole_words_batch is filter_batch on these matches
    def find_whole_words_as_columns(
        self, haystack: Any, overlapping: bool = False, *, matchkind: MatchKind = MatchKind.LeftmostLongest,
        word_bytes: Any = None
    ) -> MatchColumns: ...
    def find_whole_words_as_columns_batch(
        self, haystacks: Any, overlapping: bool = False, *, matchkind: MatchKind = MatchKind.LeftmostLongest,
        word_bytes: Any = None, offsets: Any = None, row_length: Optional[int] = None
    ) -> MatchColumns: ...
    def filter_whole_words_batch(
        self, haystacks: Any, overlapping: bool = False, *, matchkind: MatchKind = MatchKind.LeftmostLongest,
        word_bytes: Any = None, keep: str = "unmatched", min_matches: int = 1, offsets: Any = None,
        row_length: Optional[int] = None
    ) -> FilteredRows: ...
    # extension: the matches of find_matches_as_indexes(haystack, overlapping) mapped onto tokens.  token_offsets: the k + 1
    # boundaries of k tokens, non-decreasing, within 0 .. len(haystack), in BYTES, as a sequence of ints or an int64 buffer
    # (ValueError otherwise); with a __dlpack__ tensor as haystack it is a 1-D contiguous int64 __dlpack__ tensor on the
    # haystack's device.  The _batch form takes a sequence of haystacks with one such entry per haystack (a token never
    # crosses a haystack; .row_offsets cuts the tokens by haystack), or ONE uint8 __dlpack__ tensor cut by offsets /
    # row_length as mask_all_batch takes it, with ONE 1-D contiguous int64 __dlpack__ tensor of T + 1 GLOBAL byte boundaries
    # on the same device (tokens may cross rows).  On the automaton's device everything stays in HBM, the boundaries are the
    # caller's word, as offsets are, and the TokenLabels keeps the input tensors alive until it goes: they must not be
    # written before an accessor of a column has returned
    def label_tokens(self, haystack: Any, token_offsets: Any, overlapping: bool = False) -> TokenLabels: ...
    def label_tokens_batch(
        self, haystacks: Any, token_offsets: Any, overlapping: bool = False, *, offsets: Any = None,
        row_length: Optional[int] = None
    ) -> TokenLabels: ...
    # extension: the anchored search -- for every position the pattern that begins exactly there, by the object's match kind,
    # as (pattern, end) or (-1, -1); overlapping=True (Standard objects only, ValueError otherwise): every such pattern,
    # ordered by end, then by index.  haystack: one bytes-like with positions a sequence of ints or an int64 buffer within
    # 0 .. len(haystack) (ValueError outside), or one uint8 __dlpack__ tensor with positions ONE 1-D contiguous int64
    # __dlpack__ tensor on the same device; offsets / row_length (a tensor only) cut it into rows as mask_all_batch takes
    # them, split_rows(t).offsets included: a match never crosses its position's row.  On the automaton's device everything
    # stays in HBM, positions are the caller's word -- one outside the data gives (-1, -1) -- and the MatchesAt keeps the
    # input tensors alive until it goes: they must not be written before an accessor of a column has returned.
    # match_prefix_batch: the anchors are the starts of the rows (haystacks as filter_batch takes them), end is the length of
    # the match; full=True: only a pattern that IS the row counts.  No search runs: a few bytes are read per anchor
    def match_at(
        self, haystack: Any, positions: Any, overlapping: bool = False, *, offsets: Any = None, row_length: Optional[int] = None
    ) -> MatchesAt: ...
    def match_prefix_batch(
        self, haystacks: Any, overlapping: bool = False, *, full: bool = False, offsets: Any = None,
        row_length: Optional[int] = None
    ) -> MatchesAt: ...
    # extension: greedy tokenization by the dictionary (MaxMatch for a LeftmostLongest object, re.finditer of P_0|P_1|...|.
    # for a LeftmostFirst one).  haystack: one bytes-like or one uint8 __dlpack__ tensor; segment_batch takes its haystacks as
    # filter_batch does, split_rows(t).offsets included, and a piece never crosses a row.  utf8 (None: False): an unknown
    # piece is one whole UTF-8 character instead of one byte; anything but a bool or None: TypeError.  Patterns longer than
    # 256 bytes: ValueError.  On the automaton's device everything stays in HBM -- .offsets is what label_tokens_batch takes
    # as token_offsets -- and the Segments keeps the input tensors alive until it goes.  No search runs
    def segment(self, haystack: Any, *, utf8: Optional[bool] = None) -> Segments: ...
    def segment_batch(
        self, haystacks: Any, *, utf8: Optional[bool] = None, offsets: Any = None, row_length: Optional[int] = None
    ) -> Segments: ...
    # extension: WordPiece tokenization by the dictionary, as AhoCorasick.wordpiece, on bytes.  haystack: one bytes-like or one
    # uint8 __dlpack__ tensor; wordpiece_batch takes its haystacks as segment_batch does, split_rows(t).offsets included, and
    # a word never crosses a row.  The sets and the prefix are bytes-like (a str: TypeError).  On the automaton's device
    # everything stays in HBM, and the WordPieces keeps the input tensors alive until it goes.  No search runs
    def wordpiece(
        self, haystack: Any, *, continuation_prefix: Any = b"##", separators: Any = None, isolated: Any = None,
        max_word_bytes: int = 100, unk_id: int = -1
    ) -> WordPieces: ...
    def wordpiece_batch(
        self, haystacks: Any, *, continuation_prefix: Any = b"##", separators: Any = None, isolated: Any = None,
        max_word_bytes: int = 100, unk_id: int = -1, offsets: Any = None, row_length: Optional[int] = None
    ) -> WordPieces: ...
    def _info(self) -> dict[str, Any]: ...
