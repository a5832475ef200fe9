"""CPU checks of the greedy segmentation (acx_segment_host: the data cut into dictionary entries from left to right -- the
definition walked over the tables acx_compile_host(_ex) makes, the tables the device chain reads -- and what the header, the
binding, the stubs and the extension classes declare for segment / segment_batch).  Expected values come from plain Python
(the definition restated below: every pattern against the current position with startswith, no trie; for LeftmostFirst also
re.finditer of the alternation), never from the library.  tests/test_gpu_seg.py has the device side."""
import os
import re

import numpy as np
import pytest

capi = pytest.importorskip("ahocorasick_rs_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STD, LF, LL = capi.MATCH_STANDARD, capi.MATCH_LEFTMOST_FIRST, capi.MATCH_LEFTMOST_LONGEST
KINDS = (STD, LF, LL)
KEY = {STD: lambda c: (c[1], c[0]), LF: lambda c: c[0], LL: lambda c: (-c[1], c[0])}
NEW_EXPORTS = ("acx_segment", "acx_segment_device", "acx_segment_into_device", "acx_segment_host", "acx_seg_count",
               "acx_seg_rows", "acx_seg_on_device", "acx_seg_pattern", "acx_seg_offsets", "acx_seg_row_offsets", "acx_seg_copy",
               "acx_free_seg")


def unit(h, p, L, utf8):
    """the unknown unit at p < L: 1 byte, or the length the lead byte announces, shortened to the continuation bytes that
    follow and clipped to L"""
    b = h[p]
    if not utf8 or b < 0xC0 or b > 0xF7:
        return 1
    want = 2 if b < 0xE0 else 3 if b < 0xF0 else 4
    u = 1
    while u < want and p + u < L and 0x80 <= h[p + u] <= 0xBF:
        u += 1
    return u


def definition(patterns, hay, kind, *, offsets=None, utf8=False, fold=False):
    """the loop of the definition, every pattern against every position a piece begins at: (pattern, offsets, row_offsets)"""
    raw = bytes(hay)
    h = raw.lower() if fold else raw
    P = [bytes(x).lower() if fold else bytes(x) for x in patterns]
    off = [0, len(raw)] if offsets is None else [int(x) for x in offsets]
    pat, bounds, ro = [], [], []
    for r in range(len(off) - 1):
        p, L = off[r], off[r + 1]
        ro.append(len(pat))
        while p < L:
            C = [(i, p + len(x)) for i, x in enumerate(P) if h.startswith(x, p, L)]
            i, e = min(C, key=KEY[kind]) if C else (-1, p + unit(raw, p, L, utf8))
            pat.append(i)
            bounds.append(p)
            p = e
    ro.append(len(pat))
    bounds.append(len(raw))
    return np.asarray(pat, dtype=np.int64).reshape(-1), np.asarray(bounds, dtype=np.int64), np.asarray(ro, dtype=np.int64)


def check(patterns, hay, kind, *, offsets=None, utf8=False, fold=False, what=None):
    h = capi.HostAutomaton(patterns, kind, capi.BUILD_ASCII_CASE_INSENSITIVE if fold else 0)
    try:
        got = capi.segment_host(h, hay, offsets=offsets, flags=capi.SEG_UTF8 if utf8 else 0, match_kind=kind)
        want = definition(patterns, hay, kind, offsets=offsets, utf8=utf8, fold=fold)
        for g, w, name in zip(got, want, ("pattern", "offsets", "row_offsets")):
            assert g.dtype == np.int64 and np.array_equal(g, w), (what, name, g[:40], w[:40])
        pat, bounds, ro = got
        # the pieces tile every row, and a dictionary piece is what match_at reports at its start
        assert bounds[0] == 0 and bounds[-1] == len(hay) and np.all(np.diff(bounds) > 0)
        starts = [int(b) for b, i in zip(bounds[:-1], pat) if i >= 0]
        if starts:
            mp, me = capi.match_at_host(h, hay, starts, offsets=offsets, match_kind=kind)
            known = pat >= 0
            assert np.array_equal(mp, pat[known]) and np.array_equal(me, bounds[1:][known]), what
    finally:
        h.close()
    if kind == LF and offsets is None and not fold and not utf8:
        rx = re.compile(b"|".join(re.escape(bytes(x)) for x in patterns) + b"|(?s:.)")
        spans = [m.span() for m in rx.finditer(bytes(hay))]
        assert spans == list(zip(bounds[:-1].tolist(), bounds[1:].tolist())), what
        for (s, e), i in zip(spans, pat):
            assert (i < 0 and e - s == 1 and not any(bytes(hay).startswith(bytes(x), s) for x in patterns)) or \
                   bytes(patterns[i]) == bytes(hay)[s:e], what
    return got


NESTED = [b"a", b"ab", b"abc"]
FAN = [bytes([b]) + b"x" for b in range(256)]  # the root has 256 children, and so has the node behind "q"
FAN_DEEP = [b"q" + bytes([b]) for b in range(256)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("patterns", [NESTED, NESTED[::-1], [b"abc", b"a", b"ab", b"b"]])
def test_nested_prefixes_in_both_index_orders(kind, patterns):
    pat, bounds, ro = check(patterns, b"abcab abx aabcc", kind, what="nested")
    first = {STD: b"a", LF: bytes(patterns[0]), LL: b"abc"}[kind]
    assert bounds[1] == len(first) and bytes(patterns[pat[0]]) == first


def test_the_examples_of_the_issue():
    pat, bounds, ro = check([b"ab", b"bc"], b"xabc", LL)
    assert list(pat) == [-1, 0, -1] and list(bounds) == [0, 1, 3, 4]  # x | ab | c: the find would report ab at 1 as well
    pat, bounds, ro = check([b"abc", b"b"], b"abc", LL)
    assert list(pat) == [0] and list(bounds) == [0, 3]


def test_duplicates():
    patterns = [b"xy", b"x", b"xy", b"x", b"xy", b"zz"]
    hay = b"xyxzzx"
    assert list(check(patterns, hay, STD)[0]) == [1, -1, 1, 5, 1]  # the lowest index of the shortest
    assert list(check(patterns, hay, LF)[0]) == [0, 1, 5, 1]       # the first copy only
    assert list(check(patterns, hay, LL)[0]) == [0, 1, 5, 1]


@pytest.mark.parametrize("kind", KINDS)
def test_one_byte_pattern_and_bytes_0x00_0xff(kind):
    patterns = [b"\x00", b"\xff\x00", b"\xff", b"\x00\xff\xff", b"k"]
    hay = b"\x00\xff\xff\x00k\xff\x00\x00z\xfe"
    check(patterns, hay, kind)
    check(patterns, hay, kind, utf8=True)


@pytest.mark.parametrize("kind", KINDS)
def test_a_node_with_256_children(kind):
    patterns = FAN + FAN_DEEP + [b"q"]
    hay = bytes([0, ord("x"), 127, ord("x"), 255, ord("x"), ord("q"), 0, ord("q"), 128, ord("q"), 255, ord("q"), ord("x"), 7])
    check(patterns, hay, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_a_row_end_cuts_a_pattern_one_byte_short(kind):
    patterns = [b"abcd", b"ab"]
    hay = b"abcdabcdabc"
    off = [0, 4, 7, 11]  # "abcd" fits row 0 exactly, is one byte short in row 1 and in row 2
    pat, bounds, ro = check(patterns, hay, kind, offsets=off)
    assert list(ro) == ([0, 3, 5, 8] if kind == STD else [0, 1, 3, 6])  # ab c d | ab c | d ab c; abcd | ab c | d ab c
    assert set(off) <= set(bounds.tolist())  # a piece never crosses a row
    assert (0 in pat[ro[0]:ro[1]]) == (kind != STD) and 0 not in pat[ro[1]:]


CUTS = ([0, 11], [0, 0, 0, 3, 7, 11], [0, 3, 3, 3, 7, 11], [0, 1, 2, 4, 4, 8, 10, 11, 11, 11], [0, 0, 11, 11])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("offsets", CUTS)
def test_runs_of_empty_rows_at_the_front_in_the_middle_and_at_the_end(kind, offsets):
    pat, bounds, ro = check(NESTED + [b"bca"], b"abcabcababc", kind, offsets=offsets)
    for r in range(len(offsets) - 1):
        assert ro[r] == np.searchsorted(bounds[:-1], offsets[r], side="left")  # the pieces that begin before the row
        if offsets[r] == offsets[r + 1]:
            assert ro[r] == ro[r + 1]
    assert ro[-1] == len(pat)
    check(NESTED + [b"bca"], b"", kind, offsets=[0, 0, 0])
    check(NESTED, b"", kind)


@pytest.mark.parametrize("kind", KINDS)
def test_case_insensitive_tables_with_mixed_case_data(kind):
    patterns = [b"Http", b"HTTPS", b"ftp", b"h", b"\xc3\x84x"]
    hay = b"hTTps://x HTTP FtP h \xc3\x84X \xc3\xa4x"
    pat, bounds, ro = check(patterns, hay, kind, fold=True)
    assert pat[0] == {STD: 3, LF: 0, LL: 1}[kind]
    at = bounds[:-1].tolist()
    assert pat[at.index(hay.index(b"\xc3\x84X"))] == 4 and pat[at.index(hay.index(b"\xc3\xa4x"))] == -1  # ASCII letters fold only
    check(patterns, hay, kind, fold=True, utf8=True)


@pytest.mark.parametrize("kind", KINDS)
def test_utf8_unknown_units_in_bytes(kind):
    patterns = ["wort".encode(), "ä".encode(), "日本".encode()]
    text = "aäö €日本日 \U0001f600wort\U0001f601".encode()  # 2, 3 and 4 bytes
    pat, bounds, ro = check(patterns, text, kind, utf8=True)
    pieces = [text[s:e] for s, e in zip(bounds[:-1], bounds[1:])]
    assert "ö".encode() in pieces and "€".encode() in pieces and "\U0001f600".encode() in pieces
    assert all(len(x.decode()) == 1 or i >= 0 for x, i in zip(pieces, pat))  # whole characters
    off = check(patterns, text, kind)[1]  # without the flag: bytes
    assert len(off) > len(bounds)
    # a stray continuation byte, a lead byte with too few continuation bytes (then ASCII, then another lead, then the end)
    bad = b"\x80\xbfa\xe2\x82z\xf0\x9f\xc3\xa4\xf0\x9f\x98"
    pat, bounds, ro = check(patterns, bad, kind, utf8=True)
    assert list(bounds) == [0, 1, 2, 3, 5, 6, 8, 10, 13] and pat[6] == 1
    check([b"\x82z"], bad, kind, utf8=True)  # a pattern that begins inside an ill-formed character is not seen: the unit is taken
    # a character clipped by a row end: the unit stops at the row, and the next row begins with stray continuation bytes
    euro = "€€".encode()
    pat, bounds, ro = check(patterns, euro, kind, utf8=True, offsets=[0, 2, 4, 6])
    assert list(bounds) == [0, 2, 3, 4, 5, 6] and list(ro) == [0, 1, 3, 5]
    lead_beyond = bytes([0xF8, 0x80, 0xFF, 0xC0, 0x80])
    assert list(check([b"q"], lead_beyond, kind, utf8=True)[1]) == [0, 1, 2, 3, 5]  # 0xF8 and 0xFF announce nothing


def test_seeded_small_cases():
    rng = np.random.default_rng(25)
    for case in range(200):
        alphabet = b"ab" if case % 3 else b"abcA\xc3\xa4\xe2"
        n = int(rng.integers(1, 9))
        patterns = [rng.choice(list(alphabet), size=int(rng.integers(1, 5))).astype(np.uint8).tobytes() for _ in range(n)]
        hay = rng.choice(list(alphabet), size=int(rng.integers(0, 40))).astype(np.uint8).tobytes()
        cuts = sorted(int(x) for x in rng.integers(0, len(hay) + 1, size=int(rng.integers(0, 5))))
        offsets = None if case % 4 == 0 else [0] + cuts + [len(hay)]
        check(patterns, hay, KINDS[case % 3], offsets=offsets, fold=case % 5 == 0, utf8=case % 2 == 1, what=case)


def test_argument_errors():
    h = capi.HostAutomaton(NESTED, STD)
    long_ = capi.HostAutomaton([b"a" * 257, b"b"], LL)
    fits = capi.HostAutomaton([b"a" * 256, b"b"], LL)
    try:
        def code(fn):
            with pytest.raises(ValueError) as e:
                fn()
            return e.value.code

        assert code(lambda: capi.segment_host(h, b"abc", offsets=[0, 2, 1, 3])) == capi.EINVAL  # unsorted offsets
        assert code(lambda: capi.segment_host(h, b"abc", offsets=[0, 2])) == capi.EINVAL        # they do not span the data
        assert code(lambda: capi.segment_host(h, b"abc", offsets=[1, 3])) == capi.EINVAL
        assert code(lambda: capi.segment_host(h, b"abc", flags=2)) == capi.EINVAL               # an unknown flag
        assert code(lambda: capi.segment_host(h, b"abc", match_kind=3)) == capi.EINVAL
        assert code(lambda: capi.segment_host(long_, b"abc", match_kind=LL)) == capi.ETOOBIG     # SEG_MAX_STEP + 1
        assert code(lambda: capi.segment_host(long_, b"abc", offsets=[0, 2], match_kind=LL)) == capi.EINVAL  # EINVAL comes first
        pat, bounds, ro = capi.segment_host(fits, b"a" * 300 + b"b", match_kind=LL)
        assert list(pat[:2]) == [0, -1] and bounds[1] == 256 and pat[-1] == 1
        L = capi.lib()
        import ctypes
        n = ctypes.c_uint64(7)
        hay = np.frombuffer(b"abcabc", dtype=np.uint8)
        out = np.full(16, -7, dtype=np.int64)
        args = (hay.ctypes.data, 6, None, 0, 0, LL)
        assert L.acx_segment_host(None, *args, 0, None, None, None, ctypes.byref(n)) == capi.EINVAL  # null handle
        assert L.acx_segment_host(h._h, *args, 0, None, None, None, None) == capi.EINVAL              # nowhere to report T
        assert L.acx_segment_host(h._h, None, 6, None, 0, 0, LL, 0, None, None, None, ctypes.byref(n)) == capi.EINVAL
        assert L.acx_segment_host(h._h, *args, 4, None, out.ctypes.data, out.ctypes.data, ctypes.byref(n)) == capi.EINVAL
        # a cap smaller than T: T is reported, nothing is written
        assert L.acx_segment_host(h._h, *args, 1, out.ctypes.data, out[4:].ctypes.data, out[8:].ctypes.data, ctypes.byref(n)) == capi.OK
        assert n.value == 2 and np.all(out == -7)
        assert L.acx_segment_host(h._h, *args, 2, out.ctypes.data, out[4:].ctypes.data, out[8:].ctypes.data, ctypes.byref(n)) == capi.OK
        assert n.value == 2 and list(out[:3]) == [2, 2, -7] and list(out[4:8]) == [0, 3, 6, -7] and list(out[8:11]) == [0, 2, -7]
    finally:
        h.close()
        long_.close()
        fits.close()


def test_the_binding_and_the_extension_declare_the_new_names():
    L = capi.lib()
    for name in NEW_EXPORTS:
        assert hasattr(L, name), name
    with open(os.path.join(ROOT, "include", "acx.h")) as f:
        header = f.read()
    for name in NEW_EXPORTS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
    for name in ("segment", "segment_device", "segment_into_device"):
        assert callable(getattr(capi.Automaton, name)), name
    assert callable(capi.segment_host) and capi.DeviceSegments._PREFIX == "seg"
    assert capi.SEG_UTF8 == int(re.search(r"#define\s+ACX_SEG_UTF8\s+(\d+)u", header).group(1))
    assert (capi.SEG_PATTERN, capi.SEG_OFFSETS, capi.SEG_ROW_OFFSETS) == tuple(
        int(re.search(r"#define\s+ACX_SEG_" + n + r"\s+(\d+)", header).group(1)) for n in ("PATTERN", "OFFSETS", "ROW_OFFSETS"))
    assert int(re.search(r"#define\s+ACX_VERSION\s+(\d+)", header).group(1)) == 11 == capi.ABI_VERSION  # additive
    import ahocorasick_rs
    import ahocorasick_rs_amd
    for mod in (ahocorasick_rs, ahocorasick_rs_amd):
        assert "Segments" in mod.__all__ and isinstance(mod.Segments, type)
        for cls in (mod.AhoCorasick, mod.BytesAhoCorasick):
            assert callable(cls.segment) and callable(cls.segment_batch)
    assert ahocorasick_rs.Segments is ahocorasick_rs_amd.Segments
    with open(os.path.join(ROOT, "ahocorasick_rs_amd", "ahocorasick_rs.pyi")) as f:
        stubs = f.read()
    assert "class Segments" in stubs and stubs.count("def segment(") == 2 and stubs.count("def segment_batch(") == 2


def test_constants_of_the_kernel_header():
    with open(os.path.join(ROOT, "ahocorasick_rs_amd", "csrc", "seg.hpp")) as f:
        text = f.read()
    c = {n: int(re.search(r"constexpr uint32_t SEG_" + n + r"\s*=\s*(\d+)", text).group(1)) for n in ("THREADS", "TILE", "FAN", "MAX_STEP")}
    assert c["THREADS"] % 64 == 0 and c["TILE"] % c["THREADS"] == 0 and c["TILE"] <= 32768
    assert 2 <= c["FAN"] and 8 <= c["MAX_STEP"] <= c["THREADS"] and c["MAX_STEP"] < c["TILE"]
    assert c["FAN"] * c["FAN"] * c["TILE"] <= 1 << 24  # the three-level case of the GPU tests stays at 16 MiB
    assert "THE DEFINITION" in text and "SEG_UTF8" in text
