"""CPU checks of whole-word matching (acx_words_host: of a row's occurrences those whose neighbour bytes are no word bytes,
and of those the ones a match kind picks; and what the header, the binding, the stubs and the extension classes declare for
find_whole_words_as_columns / _batch and filter_whole_words_batch).  Expected values come from Python -- str.find over the
patterns and the definition restated below, and `re` for the lookaround identity -- never from the library.
tests/test_gpu_words.py has the device side."""
import ast
import os
import re

import numpy as np
import pytest

capi = pytest.importorskip("ahocorasick_rs_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STD, LF, LL = capi.MATCH_STANDARD, capi.MATCH_LEFTMOST_FIRST, capi.MATCH_LEFTMOST_LONGEST
MODES = [("overlapping", True, STD), ("standard", False, STD), ("first", False, LF), ("longest", False, LL)]
NEW_EXPORTS = ("acx_words_host", "acx_words_rows_device", "acx_find_words", "acx_find_words_device", "acx_filter_words",
               "acx_filter_words_device")
DEFAULT = capi.ASCII_WORD_BYTES
ALL_BYTES = bytes(range(256))


def occurrences(row: bytes, patterns):
    """every (p, s, e) with row[s:e] == patterns[p], in the overlapping find's order: end ascending, longer first, pattern"""
    occ = []
    for p, pat in enumerate(patterns):
        s = row.find(pat)
        while s >= 0:
            occ.append((p, s, s + len(pat)))
            s = row.find(pat, s + 1)
    return sorted(occ, key=lambda r: (r[2], r[1], r[0]))


def definition(row: bytes, occ, overlapping, kind, word_bytes):
    """the issue's definition on one row's occurrences"""
    W = set(DEFAULT if word_bytes is None else bytes(word_bytes))
    L = len(row)
    ww = [(p, s, e) for p, s, e in occ if (s == 0 or row[s - 1] not in W) and (e == L or row[e] not in W)]
    if overlapping:
        return ww
    key = {STD: lambda r: (r[2], r[1], r[0]), LF: lambda r: (r[1], r[0]), LL: lambda r: (r[1], -r[2], r[0])}[kind]
    out, pos = [], 0
    while True:
        live = [r for r in ww if r[1] >= pos]
        if not live:
            return out
        r = min(live, key=key)
        out.append(r)
        pos = r[2]


def expected(rows, patterns, overlapping, kind, word_bytes):
    recs, counts = [], []
    for row in rows:
        got = definition(row, occurrences(row, patterns), overlapping, kind, word_bytes)
        recs += got
        counts.append(len(got))
    return recs, counts


def run_host(rows, patterns, overlapping, kind, word_bytes, single=False):
    occ, counts = [], []
    for row in rows:
        o = occurrences(row, patterns)
        occ += o
        counts.append(len(o))
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
    m = np.asarray(occ, dtype=np.uint64).reshape(-1, 3)
    got, cnt = capi.words_host(b"".join(rows), None if single else off, m, None if single else counts, overlapping, kind, word_bytes)
    return [(int(p), int(s), int(e)) for p, s, e in got.tolist()], cnt.tolist()


def check(rows, patterns, word_bytes=None, what=None):
    for name, overlapping, kind in MODES:
        got = run_host(rows, patterns, overlapping, kind, word_bytes)
        want = expected(rows, patterns, overlapping, kind, word_bytes)
        assert got == (want[0], want[1]), (what, name, rows[:4], patterns, got[0][:8], want[0][:8])


def random_case(rng, n_rows, alphabet=b"ab_ .-"):
    pats = []
    for _ in range(int(rng.integers(1, 7))):
        pats.append(bytes(alphabet[int(i)] for i in rng.integers(0, len(alphabet), int(rng.integers(1, 5)))))
    rows = []
    for _ in range(n_rows):
        k = 0 if rng.random() < 0.15 else int(rng.integers(0, 41))
        rows.append(bytes(alphabet[int(i)] for i in rng.integers(0, len(alphabet), k)))
    return rows, pats


@pytest.mark.parametrize("n_rows", [1, 2, 7, 64, 301])
def test_host_against_the_definition(n_rows):
    rng = np.random.default_rng(1000 + n_rows)
    for rep in range(12 if n_rows < 64 else 3):
        rows, pats = random_case(rng, n_rows)
        if rep == 0:
            rows[0] = b""  # an empty row among them
        check(rows, pats, what=(n_rows, rep))
        check(rows, pats, word_bytes=b"ab", what=("ab", n_rows, rep))


def test_leftmost_first_is_the_lookaround_regex():
    rng = np.random.default_rng(7)
    for rep in range(300):
        rows, pats = random_case(rng, 3, alphabet=b"ab_ .-9")
        rx = re.compile(rb"(?<!\w)(?:" + b"|".join(re.escape(p) for p in pats) + rb")(?!\w)")
        got, counts = run_host(rows, pats, False, LF, None)
        want = [[(m.start(), m.end()) for m in rx.finditer(row)] for row in rows]
        assert counts == [len(w) for w in want], (rows, pats)
        assert [(s, e) for _, s, e in got] == [se for w in want for se in w], (rows, pats, got, want)


def test_empty_set_keeps_every_occurrence_and_full_set_only_whole_rows():
    rng = np.random.default_rng(11)
    for rep in range(40):
        rows, pats = random_case(rng, 5)
        occ = [occurrences(r, pats) for r in rows]
        got, counts = run_host(rows, pats, True, STD, b"")
        assert got == [o for row in occ for o in row] and counts == [len(o) for o in occ]
        check(rows, pats, word_bytes=b"", what="empty set")
        got, counts = run_host(rows, pats, True, STD, ALL_BYTES)
        assert got == [o for row, r in zip(occ, rows) for o in row if o[1] == 0 and o[2] == len(r)]
    # a row that is a pattern: whole under the full set, whatever stands in the next row
    assert run_host([b"cat", b"cats", b"cat"], [b"cat"], True, STD, ALL_BYTES) == ([(0, 0, 3), (0, 0, 3)], [1, 0, 1])


def test_a_leftmost_find_shadows_the_whole_word():
    """the issue's example: `he cat` at 1 is no whole word and must not shadow `cat` at 4"""
    pats, row = [b"he cat", b"cat"], b"the cat"
    for name, overlapping, kind in MODES:
        assert run_host([row], pats, overlapping, kind, None) == ([(1, 4, 7)], [1]), name
    # with every occurrence whole (W empty) the leftmost kinds report `he cat` and Standard the earlier end -- both end at 7:
    # the longer one is first in the overlapping order
    assert run_host([row], pats, False, LF, b"")[0] == [(0, 1, 7)]
    assert run_host([row], pats, False, STD, b"")[0] == [(0, 1, 7)]
    assert run_host([row], pats, True, STD, b"")[0] == [(0, 1, 7), (1, 4, 7)]
    # the pattern's own bytes are not looked at
    assert run_host([b"c++ code"], [b"c++"], False, LL, None)[0] == [(0, 0, 3)]
    assert run_host([b"a+b"], [b"+"], False, LL, None)[0] == []


def test_a_rows_end_is_a_boundary():
    pats = [b"cat"]
    assert run_host([b"a cat", b"s are"], pats, False, LL, None) == ([(0, 2, 5)], [1, 0])
    assert run_host([b"a cats are"], pats, False, LL, None) == ([], [0])
    assert run_host([b"cat", b"cat"], pats, True, STD, None) == ([(0, 0, 3), (0, 0, 3)], [1, 1])
    assert run_host([b"catcat"], pats, True, STD, None) == ([], [0])
    assert run_host([b"cat cat"], pats, False, LF, None) == ([(0, 0, 3), (0, 4, 7)], [2])


def test_duplicate_patterns():
    pats = [b"ab", b"x", b"ab", b"ab"]
    assert run_host([b"ab x ab"], pats, True, STD, None)[0] == [(0, 0, 2), (2, 0, 2), (3, 0, 2), (1, 3, 4), (0, 5, 7), (2, 5, 7), (3, 5, 7)]
    for kind in (STD, LF, LL):
        assert run_host([b"ab x ab"], pats, False, kind, None)[0] == [(0, 0, 2), (1, 3, 4), (0, 5, 7)]


def test_the_longest_kind_prefers_the_longer_whole_word():
    pats = [b"new", b"new york", b"york"]
    row = b"in new york now"
    assert run_host([row], pats, False, LF, None)[0] == [(0, 3, 6), (2, 7, 11)]
    assert run_host([row], pats, False, LL, None)[0] == [(1, 3, 11)]
    assert run_host([row], pats, False, STD, None)[0] == [(0, 3, 6), (2, 7, 11)]


def test_null_counts_mean_one_row():
    rows, pats = [b"a cat, a cat-flap"], [b"cat", b"a", b"flap"]
    for name, overlapping, kind in MODES:
        assert run_host(rows, pats, overlapping, kind, None, single=True) == run_host(rows, pats, overlapping, kind, None), name
    got, counts = run_host(rows, pats, False, LF, None, single=True)
    assert got == [(1, 0, 1), (0, 2, 5), (1, 7, 8), (0, 9, 12), (2, 13, 17)] and counts == [5]


def test_records_that_are_no_occurrence_are_dropped():
    """memory-safe for any records: an end beyond the row, start >= end, any order"""
    hay = b"ab ab"
    recs = [(0, 3, 5), (0, 0, 2), (0, 4, 9), (0, 2, 2), (0, 3, 1), (7, 1 << 62, (1 << 62) + 1), (0, 0, 1 << 63)]
    got, counts = capi.words_host(hay, None, np.asarray(recs, dtype=np.uint64), None, True, STD, None)
    assert got.tolist() == [(0, 3, 5), (0, 0, 2)] and counts.tolist() == [2]
    got, _ = capi.words_host(hay, None, np.asarray(recs, dtype=np.uint64), None, False, LL, None)
    assert got.tolist() == [(0, 0, 2), (0, 3, 5)]


def test_refusals():
    recs = np.asarray([(0, 0, 1), (0, 2, 3)], dtype=np.uint64)
    for counts in ([1], [1, 2], [3, 0], [1 << 63, 1 << 63]):
        off = [0] + [3] * len(counts)
        with pytest.raises(ValueError) as e:
            capi.words_host(b"a a", off, recs, counts, False, LL, None)
        assert e.value.code == capi.EINVAL, counts
    for kind in (-1, 3, 99):
        with pytest.raises(ValueError) as e:
            capi.words_host(b"a a", None, recs, None, False, kind, None)
        assert e.value.code == capi.EINVAL
    for off in ([1, 3], [0, 2], [0, 4]):
        with pytest.raises(ValueError) as e:
            capi.words_host(b"a a", off, recs, [2], False, LL, None)
        assert e.value.code == capi.EINVAL
    with pytest.raises(TypeError):
        capi.word_set("abc")


def test_word_set_bits():
    ws = capi.word_set(b"a\x00\xffaa")
    assert ws.dtype == np.uint8 and ws.shape == (32,)
    assert [v for v in range(256) if ws[v >> 3] >> (v & 7) & 1] == [0, 97, 255]
    assert capi.word_set(None) is None and not capi.word_set(b"").any()
    assert bytes(sorted(DEFAULT)) == bytes(v for v in range(256) if re.fullmatch(rb"\w", bytes([v])))
    # the default spelled out is the default
    rows, pats = [b"a_b a.b a b9 9a"], [b"a", b"b", b"9"]
    for name, overlapping, kind in MODES:
        assert run_host(rows, pats, overlapping, kind, DEFAULT) == run_host(rows, pats, overlapping, kind, None), name


def test_header_binding_and_build_lists_declare_the_stage():
    header = open(os.path.join(ROOT, "include", "acx.h")).read()
    lib = capi.lib()
    for name in NEW_EXPORTS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert getattr(lib, name).argtypes is not None, name
    assert re.search(r"^#define\s+ACX_VERSION\s+11\b", header, flags=re.M)
    assert capi._PAIRS["find_words"] == [capi.i32, capi.i32, capi.vp]
    assert capi._PAIRS["filter_words"] == [capi.i32, capi.i32, capi.vp, capi.u64, capi.u32]
    assert len(capi._SINGLES["acx_words_host"]) == 13 and len(capi._SINGLES["acx_words_rows_device"]) == 14
    build = open(os.path.join(ROOT, "ahocorasick_rs_amd", "_build.py")).read()
    for name in ("words.hip", "words_api.cpp", "words.hpp"):
        assert '"' + name + '"' in build, name
        assert os.path.exists(os.path.join(ROOT, "ahocorasick_rs_amd", "csrc", name))


def test_stubs_declare_the_methods():
    tree = ast.parse(open(os.path.join(ROOT, "ahocorasick_rs_amd", "ahocorasick_rs.pyi")).read())
    classes = {c.name: c for c in tree.body if isinstance(c, ast.ClassDef)}
    want = {
        "find_whole_words_as_columns": (["self", "haystack", "overlapping"], ["matchkind", "word_bytes"], "MatchColumns"),
        "find_whole_words_as_columns_batch": (["self", "haystacks", "overlapping"], ["matchkind", "word_bytes", "offsets", "row_length"],
                                              "MatchColumns"),
        "filter_whole_words_batch": (["self", "haystacks", "overlapping"],
                                     ["matchkind", "word_bytes", "keep", "min_matches", "offsets", "row_length"], "FilteredRows"),
    }
    for cls in ("AhoCorasick", "BytesAhoCorasick"):
        for method, (pos, kwonly, ret) in want.items():
            mine = [f for f in classes[cls].body if isinstance(f, ast.FunctionDef) and f.name == method]
            assert len(mine) == 1, (cls, method)
            a = mine[0].args
            assert [x.arg for x in a.args] == pos and [x.arg for x in a.kwonlyargs] == kwonly, (cls, method)
            assert [ast.unparse(d) for d in a.defaults] == ["False"], (cls, method)
            assert ast.unparse(a.kw_defaults[0]) == "MatchKind.LeftmostLongest" and ast.unparse(a.kw_defaults[1]) == "None"
            assert ast.unparse(mine[0].returns) == ret, (cls, method)
    names = [n.target.id for n in tree.body if isinstance(n, ast.AnnAssign)]
    assert "ASCII_WORD_BYTES" in names


def test_extension_classes_have_the_methods():
    import ahocorasick_rs
    import ahocorasick_rs_amd
    sigs = (("find_whole_words_as_columns",
             "find_whole_words_as_columns(haystack, overlapping=False, *, matchkind=MatchKind.LeftmostLongest, word_bytes=None) -> MatchColumns"),
            ("find_whole_words_as_columns_batch",
             "find_whole_words_as_columns_batch(haystacks, overlapping=False, *, matchkind=MatchKind.LeftmostLongest, word_bytes=None, "
             "offsets=None, row_length=None) -> MatchColumns"),
            ("filter_whole_words_batch",
             "filter_whole_words_batch(haystacks, overlapping=False, *, matchkind=MatchKind.LeftmostLongest, word_bytes=None, "
             "keep='unmatched', min_matches=1, offsets=None, row_length=None) -> FilteredRows"))
    for mod in (ahocorasick_rs, ahocorasick_rs_amd, ahocorasick_rs.ahocorasick_rs):
        for cls in (mod.AhoCorasick, mod.BytesAhoCorasick):
            for method, sig in sigs:
                assert callable(getattr(cls, method)), (cls, method)
                assert getattr(cls, method).__doc__.startswith(sig), (cls, method)
        assert mod.ASCII_WORD_BYTES == DEFAULT and isinstance(mod.ASCII_WORD_BYTES, bytes)
    assert "ASCII_WORD_BYTES" in ahocorasick_rs.__all__
    assert set(ahocorasick_rs.__all__) == set(ahocorasick_rs_amd.__all__)
    # the parent's methods keep their signatures
    assert "filter_batch(haystacks, overlapping=False, *, keep='unmatched', min_matches=1, offsets=None, row_length=None)" in \
        ahocorasick_rs.AhoCorasick.filter_batch.__doc__
    assert ahocorasick_rs.AhoCorasick.find_matches_as_columns.__doc__.startswith("[extension] find_matches_as_indexes(haystack, overlapping)")
