"""CPU checks of the token labels (acx_tokens_host: a search's matches mapped onto token boundaries -- per token the pattern of
the first record that touches it and the begin flag -- and what the header, the binding, the stubs and the extension classes
declare for label_tokens / label_tokens_batch).  Expected values come from plain Python (the definition restated below over
synthetic records and tokens), never from the library.  tests/test_gpu_tokens.py has the device side."""
import ast
import os
import re

import numpy as np
import pytest

capi = pytest.importorskip("ahocorasick_rs_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_EXPORTS = ("acx_tokens", "acx_tokens_device", "acx_tokens_host", "acx_tokens_rows_device", "acx_token_labels_count",
               "acx_token_labels_on_device", "acx_token_labels_pattern", "acx_token_labels_begin", "acx_token_labels_copy_pattern",
               "acx_token_labels_copy_begin", "acx_free_token_labels")


def definition(records, counts, offsets, length, ts, te):
    """A record of row h, clipped to the row (end' = min(end, row length), start' = min(start, end')), has the global range
    [off[h] + start', off[h] + end'); it touches token t iff ts[t] < g_e and te[t] > g_s; the owner of t is the touching
    record with the smallest index; pattern[t] = the owner's pattern or -1, begin[t] = 1 iff t has an owner and t - 1 has
    another one or none.  Every record against every token: no search, no order relied on."""
    offsets = [0, length] if offsets is None else [int(x) for x in offsets]
    counts = [len(records)] if counts is None else [int(c) for c in counts]
    T = len(ts)
    owner = [None] * T
    at = 0
    for h, c in enumerate(counts):
        b, rowlen = offsets[h], offsets[h + 1] - offsets[h]
        for i in range(at, at + c):
            _, s, e = records[i]
            e = min(int(e), rowlen)
            s = min(int(s), e)
            if e <= s:
                continue
            for t in range(T):
                if owner[t] is None and int(ts[t]) < b + e and int(te[t]) > b + s:
                    owner[t] = i
        at += c
    pattern = np.asarray([-1 if o is None else int(records[o][0]) for o in owner], dtype=np.int64).reshape(-1)
    begin = np.asarray([int(o is not None and (t == 0 or owner[t - 1] != o)) for t, o in enumerate(owner)], dtype=np.uint8).reshape(-1)
    return pattern, begin


def check(records, counts, offsets, length, ts, te, what=None):
    records = [tuple(int(x) for x in r) for r in records]
    got_p, got_b = capi.tokens_host(np.asarray(records, dtype=np.uint64).reshape(-1, 3), counts, offsets, length, ts, te)
    want_p, want_b = definition(records, counts, offsets, length, ts, te)
    assert got_p.dtype == np.int64 and got_b.dtype == np.uint8
    assert np.array_equal(got_p, want_p), (what, got_p[:40], want_p[:40])
    assert np.array_equal(got_b, want_b), (what, got_b[:40], want_b[:40])
    return got_p, got_b


def partition(bounds):
    b = [int(x) for x in bounds]
    return b[:-1], b[1:]


def random_tokens(rng, length, gaps=False, empties=True):
    """ascending tokens over [0, length]: lengths 0 .. 8, optionally with gaps between them and uncovered ends"""
    ts, te, at = [], [], int(rng.integers(0, 4)) if gaps else 0
    while at < length:
        k = int(rng.integers(0 if empties else 1, 9))
        ts.append(at)
        te.append(min(at + k, length))
        at = te[-1] + (int(rng.integers(0, 3)) if gaps else 0)
        if gaps and rng.integers(0, 40) == 0:
            break
    if not gaps and (not te or te[-1] < length):
        ts.append(te[-1] if te else 0)
        te.append(length)
    return ts, te


def random_case(rng, row_lens, per_row=(0, 0, 1, 2, 5), longest=12, beyond=False, overlapping=False):
    """rows of the given lengths with a few records each, in a find's order within a row (by end; overlapping: starts that do
    not rise); beyond: some records end behind their row or begin behind it"""
    offsets = np.concatenate([[0], np.cumsum(row_lens)]).astype(np.int64)
    records, counts = [], []
    for n in row_lens:
        k = int(rng.choice(per_row))
        rec = []
        for _ in range(k):
            s = int(rng.integers(0, n + 1 + (3 if beyond else 0)))
            e = s + int(rng.integers(0 if beyond else 1, longest + 1))
            if not beyond:
                e = min(e, n)
            rec.append((int(rng.integers(0, 1 << 20)), s, e))
        rec.sort(key=(lambda r: (r[2], -r[1])) if overlapping else (lambda r: (r[1], r[2])))
        records += rec
        counts.append(k)
    return records, counts, offsets, int(offsets[-1])


def test_tokens_host_on_seeded_records_and_tokens():
    rng = np.random.default_rng(20261021)
    for rows in (1, 2, 7, 64, 150):
        lens = rng.choice([0, 0, 1, 5, 17, 64, 200], size=rows)
        for kw in ({}, {"beyond": True}, {"overlapping": True, "per_row": (0, 3, 6)}):
            rec, cnt, off, n = random_case(rng, lens, **kw)
            check(rec, cnt, off, n, *random_tokens(rng, n), ("partition", rows, kw))
            check(rec, cnt, off, n, *random_tokens(rng, n, gaps=True), ("gaps", rows, kw))
            check(rec, cnt, off, n, *partition(range(n + 1)), ("one position per token", rows, kw))
        rec, cnt, off, n = random_case(rng, [33] * rows)
        check(rec, cnt, off, n, *random_tokens(rng, n, empties=False), ("uniform", rows))


def test_boundaries_equal_to_match_ends_on_both_sides():
    # tokens [0,3) [3,6) [6,9): a match [3,6) touches the middle one only; [2,7) all three; [3,3) nothing
    ts, te = partition([0, 3, 6, 9])
    p, b = check([(7, 3, 6)], None, None, 9, ts, te)
    assert p.tolist() == [-1, 7, -1] and b.tolist() == [0, 1, 0]
    p, b = check([(7, 2, 7)], None, None, 9, ts, te)
    assert p.tolist() == [7, 7, 7] and b.tolist() == [1, 0, 0]
    p, b = check([(7, 3, 3)], None, None, 9, ts, te)
    assert p.tolist() == [-1, -1, -1] and b.tolist() == [0, 0, 0]
    p, b = check([(1, 0, 3), (2, 6, 9)], None, None, 9, ts, te)
    assert p.tolist() == [1, -1, 2] and b.tolist() == [1, 0, 1]


def test_a_token_shared_by_two_matches_goes_to_the_lower_index_and_the_next_token_still_begins():
    # tokens [0,4) [4,8) [8,12); matches [1,5) and [6,10): token 1 is touched by both, record 0 owns it; token 2 begins record 1
    ts, te = partition([0, 4, 8, 12])
    p, b = check([(5, 1, 5), (9, 6, 10)], None, None, 12, ts, te)
    assert p.tolist() == [5, 5, 9] and b.tolist() == [1, 0, 1]
    # two matches inside ONE token: the first owns it, the second has no token of its own
    p, b = check([(5, 0, 1), (9, 2, 3)], None, None, 12, ts, te)
    assert p.tolist() == [5, -1, -1] and b.tolist() == [1, 0, 0]
    # adjacent matches, adjacent tokens: two begins in a row
    p, b = check([(5, 0, 4), (5, 4, 8)], None, None, 12, ts, te)
    assert p.tolist() == [5, 5, -1] and b.tolist() == [1, 1, 0]


def test_nested_and_chained_overlapping_records():
    ts, te = partition(range(0, 21, 2))   # ten tokens of two positions
    # an overlapping find's order: by end, longer first -- the inner record comes first and owns its tokens
    rec = [(1, 4, 8), (2, 2, 8), (3, 0, 12), (4, 10, 14), (5, 13, 18)]
    p, b = check(rec, None, None, 20, ts, te)
    assert p.tolist() == [3, 2, 1, 1, 3, 3, 4, 5, 5, -1]
    assert b.tolist() == [1, 1, 1, 0, 1, 0, 1, 1, 0, 0]
    # identical records: the first of them
    p, b = check([(8, 2, 6), (9, 2, 6)], None, None, 20, ts, te)
    assert p.tolist() == [-1, 8, 8] + [-1] * 7 and b.tolist() == [0, 1, 0] + [0] * 7


def test_empty_tokens_inside_a_match_and_on_its_edge():
    # tokens: [0,2) [2,2) [2,5) [5,5) [5,5) [5,8) [8,8); the match [2,5): the empty tokens at 2 and 5 lie on its edges
    ts, te = [0, 2, 2, 5, 5, 5, 8], [2, 2, 5, 5, 5, 8, 8]
    p, b = check([(3, 2, 5)], None, None, 8, ts, te)
    assert p.tolist() == [-1, -1, 3, -1, -1, -1, -1] and b.tolist() == [0, 0, 1, 0, 0, 0, 0]
    # the match [1,6): the empty tokens at 2 and 5 are strictly inside
    p, b = check([(3, 1, 6)], None, None, 8, ts, te)
    assert p.tolist() == [3, 3, 3, 3, 3, 3, -1] and b.tolist() == [1, 0, 0, 0, 0, 0, 0]
    # an empty token at the data's end, a match that ends there
    p, b = check([(3, 6, 8)], None, None, 8, ts, te)
    assert p.tolist() == [-1] * 5 + [3, -1]


def test_tokens_that_leave_head_and_tail_uncovered():
    ts, te = [3, 5, 9], [5, 8, 11]       # nothing over [0,3), [8,9), [11,16)
    p, b = check([(1, 0, 3), (2, 4, 6), (3, 8, 9), (4, 10, 16)], None, None, 16, ts, te)
    assert p.tolist() == [2, 2, 4] and b.tolist() == [1, 0, 1]
    p, b = check([(1, 0, 2), (3, 12, 16)], None, None, 16, ts, te)
    assert p.tolist() == [-1, -1, -1] and b.tolist() == [0, 0, 0]


def test_records_clipped_to_their_row_and_empty_rows():
    # rows [0,4) [4,4) [4,4) [4,10) [10,10); tokens of two positions
    off = [0, 4, 4, 4, 10, 10]
    ts, te = partition(range(0, 11, 2))
    # row 0's record says [2, 9): clipped to [2,4) it must not reach row 3's tokens; row 3's record begins behind its row
    rec = [(1, 2, 9), (2, 1, 3), (3, 7, 8)]
    p, b = check(rec, [1, 0, 0, 2, 0], off, 10, ts, te)
    assert p.tolist() == [-1, 1, 2, 2, -1] and b.tolist() == [0, 1, 1, 0, 0]
    p, b = check([(4, 9, 12), (5, 0, 100)], [1, 0, 0, 1, 0], off, 10, ts, te)
    assert p.tolist() == [-1, -1, 5, 5, 5] and b.tolist() == [0, 0, 1, 0, 0]
    # records in empty rows touch nothing
    p, b = check([(4, 0, 5), (5, 0, 5)], [0, 1, 0, 0, 1], off, 10, ts, te)
    assert p.tolist() == [-1] * 5
    # a token that crosses the rows' boundary is touched from either side
    p, b = check([(6, 3, 4), (7, 0, 1)], [1, 0, 0, 1, 0], off, 10, [0, 3], [3, 10])
    assert p.tolist() == [-1, 6] and b.tolist() == [0, 1]


def test_no_token_and_no_record():
    p, b = check([(1, 0, 4)], None, None, 4, [], [])
    assert len(p) == 0 and len(b) == 0
    p, b = check([], None, None, 9, *partition([0, 4, 9]))
    assert p.tolist() == [-1, -1] and b.tolist() == [0, 0]
    p, b = check([], [0, 0], [0, 5, 9], 9, *partition([0, 4, 9]))
    assert p.tolist() == [-1, -1]
    p, b = check([], None, None, 0, [0, 0], [0, 0])
    assert p.tolist() == [-1, -1]


def test_refusals():
    L = capi.lib()
    rec = np.asarray([(1, 0, 4)], dtype=np.uint64).reshape(-1, 3)
    capi.tokens_host(rec, None, None, 8, [0, 5], [4, 8])                  # (a gap between two tokens is no refusal)
    for ts, te, what in (([0, 3], [4, 8], "overlapping tokens"), ([4, 0], [8, 4], "descending"), ([0, 6], [4, 5], "end before start"),
                         ([0, 4], [4, 9], "beyond the data"), ([-1, 4], [4, 8], "negative"), ([0, 4], [4, -1], "negative end")):
        with pytest.raises(ValueError) as e:
            capi.tokens_host(rec, None, None, 8, ts, te)
        assert e.value.code == capi.EINVAL, what
    with pytest.raises(ValueError):
        capi.tokens_host(rec, None, None, 8, [0, 4], [4])                 # one entry per token each
    with pytest.raises(ValueError) as e:
        capi.tokens_host(rec, [2], None, 8, [0], [8])                     # counts that do not sum
    assert e.value.code == capi.EINVAL
    with pytest.raises(ValueError) as e:
        capi.tokens_host(rec, [1, 1], [0, 4, 8], 8, [0], [8])
    assert e.value.code == capi.EINVAL
    with pytest.raises(ValueError) as e:
        capi.tokens_host(rec, [1, 0], [0, 4, 7], 8, [0], [8])             # offsets that do not end at the length
    assert e.value.code == capi.EINVAL
    with pytest.raises(ValueError) as e:
        capi.tokens_host(rec, [1, 0], [0, 9, 8], 8, [0], [8])             # offsets that do not rise
    assert e.value.code == capi.EINVAL
    # null arguments, straight at the C function
    ts, te = np.asarray([0], dtype=np.int64), np.asarray([8], dtype=np.int64)
    pat, beg = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.uint8)
    args = [rec.ctypes.data, 1, None, 1, None, 8, ts.ctypes.data, te.ctypes.data, 1, pat.ctypes.data, beg.ctypes.data]
    assert L.acx_tokens_host(*args) == capi.OK
    for k in (0, 6, 7, 9, 10):
        bad = list(args)
        bad[k] = None
        assert L.acx_tokens_host(*bad) == capi.EINVAL, k
    two = list(args)
    two[3] = 2                                                            # several rows need offsets (and counts)
    assert L.acx_tokens_host(*two) == capi.EINVAL
    assert L.acx_tokens(None, None, 0, None, 0, 0, 0, None, None, 0, None) == capi.EINVAL
    assert L.acx_tokens_device(None, None, 0, None, 0, 0, 0, None, None, 0, None) == capi.EINVAL
    assert L.acx_token_labels_count(None) == 0 and L.acx_token_labels_on_device(None) == 0
    assert not L.acx_token_labels_pattern(None) and not L.acx_token_labels_begin(None)
    L.acx_free_token_labels(None)


def test_the_abi_version_stays_and_the_symbols_are_exported():
    assert capi.ABI_VERSION == 11 and capi.lib().acx_version() == 11
    header = open(os.path.join(ROOT, "include", "acx.h")).read()
    assert re.search(r"^#define\s+ACX_VERSION\s+11\s*$", header, flags=re.M)
    for name in NEW_EXPORTS:
        assert hasattr(capi.lib(), name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
    for name in ("tokens", "tokens_device"):
        assert callable(getattr(capi.Automaton, name))
    assert callable(capi.tokens_host) and callable(capi.tokens_rows_device) and capi.DeviceTokenLabels


def test_the_stage_is_in_the_build_list():
    from ahocorasick_rs_amd import _build
    assert "tokens.hip" in _build.LIB_SOURCES and "tokens_api.cpp" in _build.LIB_SOURCES and "tokens.hpp" in _build.LIB_HEADERS
    for f in ("tokens.hip", "tokens_api.cpp", "tokens.hpp"):
        assert os.path.exists(os.path.join(ROOT, "ahocorasick_rs_amd", "csrc", f)), f
    hpp = open(os.path.join(ROOT, "ahocorasick_rs_amd", "csrc", "tokens.hpp")).read()
    for name in ("TOK_THREADS", "TOK_TILE", "TOK_LONG"):  # plain constants: the seam tests read them
        assert re.search(r"constexpr uint32_t %s\s*=\s*\d+\s*;" % name, hpp), name
    hip = open(os.path.join(ROOT, "ahocorasick_rs_amd", "csrc", "tokens.hip")).read()
    # the one atomic on global memory is the 64-bit minimum over the owner words
    assert set(re.findall(r"\batomic\w+\(([^,)]*)", hip)) == {"&owner[t]", "&s_nlong"}
    assert set(re.findall(r"\b(atomic\w+)\(&owner", hip)) == {"atomicMin"}
    assert "asm" not in hip, "plain C++ stores only"


def test_pyi_declares_the_methods_and_the_class():
    tree = ast.parse(open(os.path.join(ROOT, "ahocorasick_rs_amd", "ahocorasick_rs.pyi")).read())
    classes = {c.name: c for c in tree.body if isinstance(c, ast.ClassDef)}
    want = {
        "label_tokens": (["self", "haystack", "token_offsets", "overlapping"], []),
        "label_tokens_batch": (["self", "haystacks", "token_offsets", "overlapping"], ["offsets", "row_length"]),
    }
    for cls in ("AhoCorasick", "BytesAhoCorasick"):
        for method, (pos, kwonly) in want.items():
            mine = [f for f in classes[cls].body if isinstance(f, ast.FunctionDef) and f.name == method]
            assert len(mine) == 1, (cls, method)
            a = mine[0].args
            assert [x.arg for x in a.args] == pos, (cls, method)
            assert [x.arg for x in a.kwonlyargs] == kwonly, (cls, method)
            assert a.vararg is None and a.kwarg is None, (cls, method)
            assert [ast.unparse(d) for d in a.defaults] == ["False"], (cls, method)
            assert [ast.unparse(d) for d in a.kw_defaults] == ["None"] * len(kwonly), (cls, method)
            assert ast.unparse(mine[0].returns) == "TokenLabels", (cls, method)
    names = {f.name for f in classes["TokenLabels"].body if isinstance(f, ast.FunctionDef)}
    assert names >= {"pattern", "begin", "row_offsets", "device", "__len__", "tolist"}


def test_extension_classes_have_the_methods():
    import ahocorasick_rs
    import ahocorasick_rs_amd
    for mod in (ahocorasick_rs, ahocorasick_rs_amd, ahocorasick_rs.ahocorasick_rs):
        for cls in (mod.AhoCorasick, mod.BytesAhoCorasick):
            for method, sig in (("label_tokens", "(haystack, token_offsets, overlapping=False)"),
                                ("label_tokens_batch", "(haystacks, token_offsets, overlapping=False, *, offsets=None, row_length=None)")):
                assert callable(getattr(cls, method)), (cls, method)
                assert method + sig in getattr(cls, method).__doc__, (cls, method)
        assert isinstance(mod.TokenLabels, type)
        with pytest.raises(TypeError):
            mod.TokenLabels()  # (made by the methods only)
    for mod in (ahocorasick_rs, ahocorasick_rs_amd):
        assert "TokenLabels" in mod.__all__
    assert set(ahocorasick_rs.__all__) == set(ahocorasick_rs_amd.__all__)
    assert ahocorasick_rs.TokenLabels is ahocorasick_rs_amd.TokenLabels
    for name in ("pattern", "begin", "row_offsets", "device", "tolist", "__len__"):
        assert hasattr(ahocorasick_rs.TokenLabels, name)
    # the parent's methods keep their signatures
    assert "mask_all_batch(haystacks, fill, overlapping=False, *" in ahocorasick_rs.AhoCorasick.mask_all_batch.__doc__
    assert "MatchSnippets" in ahocorasick_rs.__all__ and "MaskedRows" in ahocorasick_rs.__all__
