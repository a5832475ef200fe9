"""CPU checks of the matched text and its context (acx_snippets_host: every record's bytes and up to `context` bytes on each
side, clipped to the row, the ends moved inward to a character boundary under the UTF-8 flag; and what the header, the
binding, the stubs and the extension classes declare for find_matches_as_snippets / find_matches_as_snippets_batch).
Expected values come from Python (the definition restated below over synthetic records), never from the library.
tests/test_gpu_snippets.py has the device side."""
import ast
import os
import re

import numpy as np
import pytest

capi = pytest.importorskip("ahocorasick_rs_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ahocorasick_rs_amd", "csrc")

NEW_EXPORTS = ("acx_snippets", "acx_snippets_device", "acx_snippets_host", "acx_snippets_rows_device", "acx_snippets_count",
               "acx_snippets_rows", "acx_snippets_nbytes", "acx_snippets_on_device", "acx_snippets_data", "acx_snippets_copy",
               "acx_free_snippets")
CONTEXT_MAX = (1 << 63) - 1
UTF8 = 1


def definition(records, counts, hay, offsets, context, utf8):
    """the issue's rule, record by record -> (snippets, pattern, lead, row_offsets)"""
    hay = bytes(hay)
    offsets = [0, len(hay)] if offsets is None else [int(o) for o in offsets]
    counts = [len(records)] if counts is None else [int(c) for c in counts]
    assert len(counts) == len(offsets) - 1
    snippets, pattern, lead, ro, at = [], [], [], [0], 0
    for h, c in enumerate(counts):
        B = hay[offsets[h]:offsets[h + 1]]
        L = len(B)
        for p, s, e in records[at:at + c]:
            s1 = min(int(s), L)
            e1 = min(max(int(e), s1), L)
            lo = s1 - min(s1, context)
            hi = e1 + min(context, L - e1)
            if utf8:
                for _ in range(3):
                    if lo < s1 and 0x80 <= B[lo] <= 0xBF:
                        lo += 1
                for _ in range(3):
                    if e1 < hi < L and 0x80 <= B[hi] <= 0xBF:
                        hi -= 1
            snippets.append(B[lo:hi])
            pattern.append(int(p))
            lead.append(s1 - lo)
        at += c
        ro.append(at)
    assert at == len(records)
    return snippets, pattern, lead, ro


def check(records, counts, hay, offsets=None, context=0, flags=0, what=None):
    records = [tuple(int(x) for x in r) for r in records]
    data, off, pat, lead, ro = capi.snippets_host(np.asarray(records, dtype=np.uint64).reshape(-1, 3), counts, hay, offsets, context, flags)
    want, want_pat, want_lead, want_ro = definition(records, counts, hay, offsets, context, bool(flags & UTF8))
    assert data.dtype == np.uint8 and off.dtype == pat.dtype == lead.dtype == ro.dtype == np.int64
    blob = data.tobytes()
    got = [blob[off[i]:off[i + 1]] for i in range(len(records))]
    assert got == want, (what, context, got[:8], want[:8])
    assert off[0] == 0 and off[-1] == len(blob) == sum(len(w) for w in want)
    assert pat.astype(np.uint64).tolist() == want_pat and lead.tolist() == want_lead and ro.tolist() == want_ro, (what, context)
    # the two-call form: the sizes alone say the same
    assert capi.snippets_host(np.asarray(records, dtype=np.uint64).reshape(-1, 3), counts, hay, offsets, context, flags,
                              sizes_only=True) == len(blob)
    return got


def test_snippets_host_every_clip_case():
    hay = b"0123456789abcdefghij"                                      # one row of 20 bytes
    assert check([(7, 5, 8)], None, hay) == [b"567"]                    # context 0: the match itself
    assert check([(7, 5, 8)], None, hay, context=2) == [b"3456789"]
    assert check([(7, 5, 8)], None, hay, context=5) == [b"0123456789abc"]   # the left side exactly reaches the row's begin
    assert check([(7, 5, 8)], None, hay, context=6) == [b"0123456789abcd"]  # ... and is clipped there
    assert check([(7, 5, 8)], None, hay, context=12) == [hay]               # the right side exactly reaches the row's end
    assert check([(7, 5, 8)], None, hay, context=13) == [hay]
    assert check([(7, 5, 8)], None, hay, context=CONTEXT_MAX) == [hay]      # no sum wraps
    assert check([(0, 0, 3)], None, hay, context=4) == [b"0123456"]         # a match at byte 0
    assert check([(0, 17, 20)], None, hay, context=4) == [b"defghij"]       # a match at the last byte
    assert check([(0, 0, 20)], None, hay, context=9) == [hay]
    assert check([(0, 6, 6)], None, hay, context=0) == [b""]                # an empty match: an empty snippet
    assert check([(0, 6, 6)], None, hay, context=1) == [b"56"]              # ... or its context alone
    # the lead is the clipped left side
    data, off, pat, lead, ro = capi.snippets_host([(3, 2, 4), (4, 9, 11)], None, hay, None, 5, 0)
    assert lead.tolist() == [2, 5] and pat.tolist() == [3, 4] and ro.tolist() == [0, 2]
    # snippets of neighbours overlap one another: independent copies
    assert check([(0, 2, 4), (0, 3, 6), (0, 5, 6)], None, hay, context=3) == [b"0123456", b"012345678", b"2345678"]


def test_snippets_host_rows_are_walls():
    hay = b"aaaaXbbbbbbXcc"
    offsets = [0, 5, 5, 12, 14]                                        # rows: aaaaX, (empty), bbbbbbX, cc
    rec = [(0, 4, 5), (1, 0, 1), (2, 6, 7), (3, 1, 2)]
    assert check(rec, [1, 0, 2, 1], hay, offsets, context=0) == [b"X", b"b", b"X", b"c"]
    assert check(rec, [1, 0, 2, 1], hay, offsets, context=3) == [b"aaaX", b"bbbb", b"bbbX", b"cc"]
    assert check(rec, [1, 0, 2, 1], hay, offsets, context=CONTEXT_MAX) == [b"aaaaX", b"bbbbbbX", b"bbbbbbX", b"cc"]
    # empty rows, empty records
    assert check([], [0, 0, 0, 0], hay, offsets) == []
    assert check([], None, b"") == [] and check([], [], b"", [0]) == []
    assert check([(0, 0, 0)], [0, 1, 0], b"", [0, 0, 0, 0], context=9) == [b""]     # a record in an empty row
    data, off, pat, lead, ro = capi.snippets_host(np.zeros((0, 3), np.uint64), [0, 0], b"xy", [0, 1, 2], 4, 0)
    assert off.tolist() == [0] and ro.tolist() == [0, 0, 0] and len(data) == len(pat) == len(lead) == 0


def test_snippets_host_junk_records_are_memory_safe():
    hay = b"0123456789"
    assert check([(0, 4, 99)], None, hay, context=1) == [b"3456789"]              # e > L
    assert check([(0, 99, 120)], None, hay, context=3) == [b"789"]                # s > L: an empty match at the row's end
    assert check([(0, 7, 3)], None, hay, context=2) == [b"5678"]                  # s > e: an empty match at s
    assert check([(0, (1 << 64) - 1, (1 << 64) - 1)], None, hay, context=CONTEXT_MAX) == [hay]
    assert check([(0, (1 << 64) - 1, 0)], None, hay, context=0) == [b""]
    assert check([(0, 5, 1 << 63)], [0, 1], hay, [0, 4, 10], context=1) == [b"89"]  # beyond its own row of 6 bytes


def test_snippets_host_trim_depths_and_directions():
    # left: the cut lands 1, 2 or 3 continuation bytes into a character and moves right to the next boundary
    four = "\U0001F600".encode()                                       # F0 9F 98 80
    hay = four + b"ab"
    for context, depth_left in ((3, 3), (2, 2), (1, 1)):
        rec = [(0, 4, 5)]                                              # "a"
        got = check(rec, None, hay, context=context, flags=UTF8, what=("left", depth_left))
        assert got == [b"ab"]                                          # the emoji's tail is gone, the right side is whole
        assert check(rec, None, hay, context=context, flags=0) == [hay[4 - context:6]]
    assert check([(0, 4, 5)], None, hay, context=4, flags=UTF8) == [hay]          # the whole character fits: nothing to trim
    # right: hi lands on a continuation byte and moves left, depth 1, 2, 3
    hay = b"ab" + four + b"c"
    for context, right in ((1, b""), (2, b""), (3, b""), (4, four), (5, four + b"c")):
        assert check([(0, 1, 2)], None, hay, context=context, flags=UTF8, what=("right", context)) == [b"ab" + right]
    # two- and three-byte characters
    hay = "xéy€z".encode()                                   # x C3 A9 y E2 82 AC z
    assert check([(0, 3, 4)], None, hay, context=1, flags=UTF8) == [b"y"]         # both sides cut a character: both trimmed away
    assert check([(0, 3, 4)], None, hay, context=2, flags=UTF8) == ["éy".encode()]
    assert check([(0, 3, 4)], None, hay, context=3, flags=UTF8) == ["xéy€".encode()]
    assert check([(0, 3, 4)], None, hay, context=4, flags=UTF8) == [hay]
    for context in range(9):
        check([(0, 3, 4), (1, 1, 3), (2, 4, 7)], None, hay, context=context, flags=UTF8)[0].decode()


def test_snippets_host_trim_never_enters_the_match_and_stops_at_row_edges():
    # a junk record that begins inside a character: lo stops at s', hi at e'
    hay = b"a\x80\x80\x80\x80\x80\x80b"
    assert check([(0, 3, 5)], None, hay, context=1, flags=UTF8) == [b"\x80\x80"]        # both sides trimmed back to the match
    assert check([(0, 3, 5)], None, hay, context=2, flags=UTF8) == [b"\x80" * 4]            # hi lands on "b": a boundary
    assert check([(0, 3, 5)], None, hay, context=0, flags=UTF8) == [b"\x80\x80"]
    # hi == L is a boundary whatever the last byte is; lo == 0 is read like any byte
    hay = b"\x80\x80ab\x80\x80"
    assert check([(0, 2, 4)], None, hay, context=2, flags=UTF8) == [b"ab\x80\x80"]       # left trimmed twice, right ends at L
    assert check([(0, 2, 4)], None, hay, context=1, flags=UTF8) == [b"ab"]               # B[5] is a continuation byte: hi moves in
    # rows: the byte behind the row's end is never looked at
    hay = b"ab\x80\x80cd"
    assert check([(0, 0, 2), (0, 2, 4)], [1, 1], hay, [0, 2, 6], context=5, flags=UTF8) == [b"ab", b"cd"]


def test_snippets_host_invalid_utf8_is_bounded_at_three_steps():
    hay = b"\x80" * 10 + b"MM" + b"\xbf" * 10
    assert check([(0, 10, 12)], None, hay, context=8, flags=UTF8) == [b"\x80" * 5 + b"MM" + b"\xbf" * 5]   # 8 - 3 on each side
    assert check([(0, 10, 12)], None, hay, context=3, flags=UTF8) == [b"MM"]
    assert check([(0, 10, 12)], None, hay, context=4, flags=UTF8) == [b"\x80MM\xbf"]
    assert check([(0, 10, 12)], None, hay, context=CONTEXT_MAX, flags=UTF8) == [hay[3:]]   # lo = 0 moves three; hi = L stays
    # 0x7F, 0xC0 are no continuation bytes
    hay = b"\x7f\xc0MM\xc0\x7f"
    assert check([(0, 2, 4)], None, hay, context=1, flags=UTF8) == [b"\xc0MM\xc0"]


def test_snippets_host_on_seeded_batches():
    rng = np.random.default_rng(20261020)
    alphabet = ["a", "b", " ", "é", "€", "\U0001F600"]
    for rows in (1, 3, 40):
        texts = ["".join(rng.choice(alphabet, size=int(rng.integers(0, 60)))).encode() for _ in range(rows)]
        offsets = np.concatenate([[0], np.cumsum([len(t) for t in texts])])
        counts = rng.choice([0, 1, 2, 9], size=rows)
        rec = []
        for h, k in enumerate(counts):
            L = len(texts[h])
            for _ in range(int(k)):
                s = int(rng.integers(0, L + 3))
                rec.append((int(rng.integers(0, 99)), s, max(0, s + int(rng.integers(-2, 9)))))
        for context in (0, 1, 2, 3, 7, 64, CONTEXT_MAX):
            for flags in (0, UTF8):
                check(rec, counts, b"".join(texts), offsets, context, flags, ("seeded", rows))


def test_snippets_host_refuses_bad_arguments():
    hay = b"0123456789"
    rec = [(0, 1, 2), (0, 3, 4), (0, 5, 6)]
    for counts in ([1, 1], [2, 2], [4, 0], [(1 << 64) - 1, 4]):        # the counts do not sum to the records
        with pytest.raises(ValueError) as ei:
            capi.snippets_host(rec, counts, hay, [0, 5, 10])
        assert ei.value.code == capi.EINVAL, counts
    for offsets in ([0, 5, 9], [1, 5, 10], [0, 11, 10]):               # the offsets do not rise from 0 to len
        with pytest.raises(ValueError) as ei:
            capi.snippets_host(rec, [1, 2], hay, offsets)
        assert ei.value.code == capi.EINVAL, offsets
    for context in (1 << 63, (1 << 64) - 1):
        with pytest.raises(ValueError) as ei:
            capi.snippets_host(rec, None, hay, None, context)
        assert ei.value.code == capi.EINVAL, context
    for flags in (2, 4, 1 << 31):
        with pytest.raises(ValueError) as ei:
            capi.snippets_host(rec, None, hay, None, 0, flags)
        assert ei.value.code == capi.EINVAL, flags
    L = capi.lib()
    m = np.asarray(rec, dtype=np.uint64)
    c = np.asarray([1, 2], dtype=np.uint64)
    o = np.asarray([0, 5, 10], dtype=np.uint64)
    h = np.frombuffer(hay, dtype=np.uint8)
    t = capi.ctypes.c_uint64(99)
    call = lambda *a: L.acx_snippets_host(*a, capi.ctypes.byref(t))  # noqa: E731
    nul = (None,) * 5
    assert call(m.ctypes.data, 3, c.ctypes.data, 2, h.ctypes.data, 10, o.ctypes.data, 1, 0, *nul) == capi.OK and t.value == 7
    assert call(None, 3, c.ctypes.data, 2, h.ctypes.data, 10, o.ctypes.data, 1, 0, *nul) == capi.EINVAL          # no records
    assert call(m.ctypes.data, 3, c.ctypes.data, 2, None, 10, o.ctypes.data, 1, 0, *nul) == capi.EINVAL          # no haystack
    assert call(m.ctypes.data, 3, None, 2, h.ctypes.data, 10, o.ctypes.data, 1, 0, *nul) == capi.EINVAL          # two rows, no counts
    assert call(m.ctypes.data, 3, c.ctypes.data, 2, h.ctypes.data, 10, None, 1, 0, *nul) == capi.EINVAL          # two rows, no offsets
    assert L.acx_snippets_host(m.ctypes.data, 3, c.ctypes.data, 2, h.ctypes.data, 10, o.ctypes.data, 1, 0, *nul, None) == capi.EINVAL
    assert call(None, 0, None, 0, None, 0, None, 0, 0, *nul) == capi.OK and t.value == 0
    # the fill writes nothing behind the total
    data = np.full(12, 0xEE, np.uint8)
    off = np.full(5, -7, np.int64)
    assert call(m.ctypes.data, 3, c.ctypes.data, 2, h.ctypes.data, 10, o.ctypes.data, 1, 0, off.ctypes.data, None, None, None,
                data.ctypes.data) == capi.OK
    assert data.tobytes() == b"012" + b"789" + b"9" + b"\xee" * 5 and off.tolist() == [0, 3, 6, 7, -7]


def test_header_and_binding_agree_on_the_snippets_abi():
    hdr = open(os.path.join(ROOT, "include", "acx.h")).read()
    L = capi.lib()
    for name in NEW_EXPORTS:
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert decl, name
        assert hasattr(L, name), name
        n_args = len([a for a in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",") if a.strip()])
        assert len(getattr(L, name).argtypes) == n_args, (name, n_args)  # bound with its argument types, one per argument
    names = ("DATA", "OFFSETS", "PATTERN", "LEAD", "ROW_OFFSETS")
    for k, name in enumerate(names):
        assert int(re.search(r"#define ACX_SNIP_%s (\d+)" % name, hdr).group(1)) == getattr(capi, "SNIP_" + name) == k
    assert sorted(re.findall(r"#define ACX_SNIP_(\w+) ", hdr)) == sorted(names)      # five, no more
    assert int(re.search(r"#define ACX_SNIPPET_UTF8 (\d+)", hdr).group(1)) == capi.SNIPPET_UTF8 == 1
    assert re.search(r"typedef struct acx_snippets acx_snippets_t;", hdr)
    u64, u32 = capi.ctypes.c_uint64, capi.ctypes.c_uint32
    # acx_snippets* take acx_spans*'s arguments without `codepoints`, `context` in gap's place and the flags behind it
    for mine, spans in (("acx_snippets", "acx_spans"), ("acx_snippets_device", "acx_spans_device")):
        want = list(getattr(L, spans).argtypes)
        del want[-3]
        want.insert(len(want) - 1, u32)
        assert list(getattr(L, mine).argtypes) == want, mine
    assert L.acx_snippets_data.restype is capi.ctypes.c_void_p and list(L.acx_snippets_data.argtypes) == list(L.acx_spans_data.argtypes)
    assert list(L.acx_snippets_copy.argtypes) == list(L.acx_spans_copy.argtypes)
    for name in ("count", "rows", "nbytes"):
        assert getattr(L, "acx_snippets_" + name).restype is u64
    assert L.acx_free_snippets.restype is None
    # additive: the version and the path counters are the parent's
    assert L.acx_version() == capi.ABI_VERSION == int(re.search(r"#define ACX_VERSION (\d+)", hdr).group(1)) == 11
    assert len(capi.Automaton.PATH_STATS) == int(re.search(r"#define ACX_PATH_STATS (\d+)", hdr).group(1)) == 14
    for name in ("snippets", "snippets_device"):
        assert callable(getattr(capi.Automaton, name))
    assert callable(capi.snippets_host) and callable(capi.snippets_rows_device) and capi.DeviceSnippets


def test_the_stage_is_in_the_build_list_and_its_sizes_are_plain_constants():
    from ahocorasick_rs_amd import _build
    assert "snippets.hip" in _build.LIB_SOURCES and "snippets_api.cpp" in _build.LIB_SOURCES and "snippets.hpp" in _build.LIB_HEADERS
    for f in ("snippets.hip", "snippets_api.cpp", "snippets.hpp"):
        assert os.path.exists(os.path.join(CSRC, f)), f
    hpp = open(os.path.join(CSRC, "snippets.hpp")).read()
    c = {}
    for name in ("SNIP_THREADS", "SNIP_TILE", "SNIP_WIN"):  # plain constants: the seam tests read them
        m = re.search(r"constexpr uint32_t %s\s*=\s*(\d+)\s*;" % name, hpp)
        assert m, name
        c[name] = int(m.group(1))
    assert c["SNIP_TILE"] % (16 * c["SNIP_THREADS"]) == 0 and c["SNIP_THREADS"] % 64 == 0 and c["SNIP_WIN"] >= 1
    hip = open(os.path.join(CSRC, "snippets.hip")).read()
    assert "asm" not in hip, "plain C++ stores only"
    assert "atomic" not in hip, "the stage needs no atomic"
    # one more entry of Layout::at, nothing else
    assert re.search(r"uint64_t at\[5\] = \{0, 0, 0, 0, 0\}, bytes = 0;", open(os.path.join(CSRC, "result_block.hpp")).read())


def test_pyi_declares_the_methods_and_the_class():
    tree = ast.parse(open(os.path.join(ROOT, "ahocorasick_rs_amd", "ahocorasick_rs.pyi")).read())
    classes = {c.name: c for c in tree.body if isinstance(c, ast.ClassDef)}
    want = {
        "find_matches_as_snippets": (["self", "haystack", "overlapping"], ["context"], ["0"]),
        "find_matches_as_snippets_batch": (["self", "haystacks", "overlapping"], ["context", "offsets", "row_length"],
                                           ["0", "None", "None"]),
    }
    for cls in ("AhoCorasick", "BytesAhoCorasick"):
        for method, (pos, kwonly, kwdefaults) in want.items():
            mine = [f for f in classes[cls].body if isinstance(f, ast.FunctionDef) and f.name == method]
            assert len(mine) == 1, (cls, method)
            a = mine[0].args
            assert [x.arg for x in a.args] == pos, (cls, method)
            assert [x.arg for x in a.kwonlyargs] == kwonly, (cls, method)
            assert a.vararg is None and a.kwarg is None, (cls, method)
            assert [ast.unparse(d) for d in a.defaults] == ["False"], (cls, method)
            assert [ast.unparse(d) for d in a.kw_defaults] == kwdefaults, (cls, method)
            assert ast.unparse(mine[0].returns) == "MatchSnippets", (cls, method)
            context = [x for x in a.kwonlyargs if x.arg == "context"][0]
            assert ast.unparse(context.annotation) == "int"
    names = {f.name for f in classes["MatchSnippets"].body if isinstance(f, ast.FunctionDef)}
    assert names == {"data", "offsets", "pattern", "lead", "row_offsets", "device", "nbytes", "__len__", "tolist"}
    assert "__init__" not in names


def test_extension_classes_have_the_methods():
    import ahocorasick_rs
    import ahocorasick_rs_amd
    sigs = (("find_matches_as_snippets", "find_matches_as_snippets(haystack, overlapping=False, *, context=0) -> MatchSnippets"),
            ("find_matches_as_snippets_batch",
             "find_matches_as_snippets_batch(haystacks, overlapping=False, *, context=0, offsets=None, row_length=None) -> MatchSnippets"))
    for mod in (ahocorasick_rs, ahocorasick_rs_amd, ahocorasick_rs.ahocorasick_rs):
        for cls in (mod.AhoCorasick, mod.BytesAhoCorasick):
            for method, sig in sigs:
                assert callable(getattr(cls, method)), (cls, method)
                assert getattr(cls, method).__doc__.startswith(sig), (cls, method)
        assert isinstance(mod.MatchSnippets, type) and "MatchSnippets" in mod.__all__
        with pytest.raises(TypeError):
            mod.MatchSnippets()  # (made by the methods only)
    assert ahocorasick_rs.MatchSnippets is ahocorasick_rs_amd.MatchSnippets
    assert set(ahocorasick_rs.__all__) == set(ahocorasick_rs_amd.__all__)
    members = {n for n in dir(ahocorasick_rs.MatchSnippets) if not n.startswith("__")} | {"__len__"}
    assert members == {"data", "offsets", "pattern", "lead", "row_offsets", "device", "nbytes", "tolist", "__len__"}
    assert hasattr(ahocorasick_rs.MatchSnippets, "__len__")
    # the parent's methods keep their signatures
    assert ahocorasick_rs.AhoCorasick.cover_spans.__doc__.startswith("cover_spans(haystack, overlapping=False, *, gap=0) -> MatchSpans")
    assert "MatchSpans" in ahocorasick_rs.__all__ and "MatchColumns" in ahocorasick_rs.__all__


def test_the_context_argument():
    """the one check both classes' find_matches_as_snippets and _batch make of `context` (the extension's _snippets_context:
    no automaton), which is the check of cover_spans' gap"""
    from ahocorasick_rs_amd.ahocorasick_rs import _snippets_context
    for context in (0, 1, 64, 1 << 32, CONTEXT_MAX):
        assert _snippets_context(context) == context
    for bad in (-1, -(1 << 70), 1 << 63, 1 << 64, 1 << 70):
        with pytest.raises(ValueError):
            _snippets_context(bad)
    for bad in (True, False, 1.0, "1", None, b"1", [1], np.float64(2)):
        with pytest.raises(TypeError):
            _snippets_context(bad)
