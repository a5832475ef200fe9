"""CPU checks of the anchored search (acx_match_at_host: which pattern begins exactly at a position, or at the start of
every row -- the definition walked over the tables acx_compile_host(_ex) makes, the tables the device walk reads -- and what
the header, the binding, the stubs and the extension classes declare for match_at / match_prefix_batch).  Expected values
come from plain Python (the definition restated below: every pattern against every anchor with startswith, no trie; for
LeftmostFirst also re.match of the alternation), never from the library.  tests/test_gpu_at.py has the device side."""
import os
import re

import numpy as np
import pytest

capi = pytest.importorskip("ahocorasick_rs_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STD, LF, LL = capi.MATCH_STANDARD, capi.MATCH_LEFTMOST_FIRST, capi.MATCH_LEFTMOST_LONGEST
KINDS = (STD, LF, LL)
NEW_EXPORTS = ("acx_match_at", "acx_match_at_device", "acx_match_at_into_device", "acx_match_at_host", "acx_at_count",
               "acx_at_entries", "acx_at_on_device", "acx_at_pattern", "acx_at_end", "acx_at_row_offsets", "acx_at_copy",
               "acx_free_at")


def anchors_of(length, positions, offsets):
    """(p, L) per anchor.  positions None: the rows themselves.  Else the row of p is the LAST row that begins at or before p
    (of several rows with one start all but the last are empty) and L is where the next one begins; p == length: L = p."""
    off = [0, length] if offsets is None else [int(x) for x in offsets]
    if positions is None:
        return [(off[r], off[r + 1]) for r in range(len(off) - 1)]
    out = []
    for p in positions:
        p = int(p)
        rows = [r for r in range(len(off) - 1) if off[r] <= p]
        out.append((p, off[rows[-1] + 1] if rows and p < length else p))
    return out


def definition(patterns, hay, anchors, kind, *, overlapping=False, full=False, fold=False, local=False):
    """C(p, L) = {(i, e): e = p + len(P_i), e <= L, h[p:e] == P_i}; full keeps e == L only.  Standard: smallest e, then
    smallest i; LeftmostFirst: smallest i; LeftmostLongest: largest e, then smallest i; overlapping: all of C by (e, i).
    local: ends count from p (the prefix form).  Every pattern against every anchor."""
    h = bytes(hay).lower() if fold else bytes(hay)
    P = [bytes(x).lower() if fold else bytes(x) for x in patterns]
    pat, end, ro = [], [], [0]
    for p, L in anchors:
        C = [(i, p + len(x)) for i, x in enumerate(P) if h.startswith(x, p, L)]
        if full:
            C = [c for c in C if c[1] == L]
        if overlapping:
            C.sort(key=lambda c: (c[1], c[0]))
        elif C:
            key = {STD: lambda c: (c[1], c[0]), LF: lambda c: c[0], LL: lambda c: (-c[1], c[0])}[kind]
            C = [min(C, key=key)]
        else:
            C = [(-1, -1)]
        pat += [c[0] for c in C]
        end += [c[1] - (p if local and c[0] >= 0 else 0) for c in C]
        ro.append(len(pat))
    return np.asarray(pat, dtype=np.int64).reshape(-1), np.asarray(end, dtype=np.int64).reshape(-1), np.asarray(ro, dtype=np.int64)


def check(patterns, hay, positions, kind, *, offsets=None, overlapping=False, full=False, fold=False, what=None):
    flags = (capi.AT_OVERLAPPING if overlapping else 0) | (capi.AT_FULL if full else 0) | \
            (capi.AT_ROW_STARTS if positions is None else 0)
    h = capi.HostAutomaton(patterns, kind, capi.BUILD_ASCII_CASE_INSENSITIVE if fold else 0)
    try:
        got = capi.match_at_host(h, hay, positions, offsets=offsets, flags=flags, match_kind=kind)
    finally:
        h.close()
    anchors = anchors_of(len(hay), positions, offsets)
    want = definition(patterns, hay, anchors, kind, overlapping=overlapping, full=full, fold=fold, local=positions is None)
    assert len(got) == (3 if overlapping else 2)
    for g, w, name in zip(got, want, ("pattern", "end", "row_offsets")):
        assert g.dtype == np.int64 and np.array_equal(g, w), (what, name, g[:40], w[:40])
    if kind == LF and not overlapping and not full and not fold:
        rx = re.compile(b"|".join(re.escape(bytes(x)) for x in patterns))
        for (p, L), gp, ge in zip(anchors, got[0], got[1]):
            m = rx.match(bytes(hay), p, L)
            assert (m is None) == (gp < 0), (what, p, L)
            if m:  # (the prefix form's ends are local to the row)
                assert bytes(patterns[gp]) == m.group(0) and ge == m.end() - (p if positions is None else 0), (what, p, L)
    return got


NESTED = [b"a", b"ab", b"abc"]
FAN = [bytes([b]) + b"x" for b in range(256)]  # the root has 256 children, and so has the node behind "q"
FAN_DEEP = [b"q" + bytes([b]) for b in range(256)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("patterns", [NESTED, NESTED[::-1], [b"abc", b"a", b"ab", b"b"]])
def test_nested_prefixes_in_both_index_orders(kind, patterns):
    hay = b"abcab abx a"
    check(patterns, hay, list(range(len(hay) + 1)), kind, what="nested")


def test_nested_prefixes_overlapping():
    hay = b"abcab abx a"
    for patterns in (NESTED, NESTED[::-1]):
        pat, end, ro = check(patterns, hay, list(range(len(hay) + 1)), STD, overlapping=True)
        assert ro[1] - ro[0] == 3 and list(end[:3]) == [1, 2, 3]


def test_duplicates():
    patterns = [b"xy", b"x", b"xy", b"x", b"xy", b"zz"]
    hay = b"xyxzzx"
    pos = list(range(len(hay) + 1))
    pat, end = check(patterns, hay, pos, STD)
    assert (pat[0], end[0]) == (1, 1)  # the lowest index of the shortest
    pat, end, ro = check(patterns, hay, pos, STD, overlapping=True)
    assert list(pat[ro[0]:ro[1]]) == [1, 3, 0, 2, 4] and list(end[ro[0]:ro[1]]) == [1, 1, 2, 2, 2]  # all of them
    pat, end = check(patterns, hay, pos, LF)
    assert (pat[0], end[0]) == (0, 2)  # the first only
    pat, end = check(patterns, hay, pos, LL)
    assert (pat[0], end[0]) == (0, 2)


@pytest.mark.parametrize("kind", KINDS)
def test_one_byte_pattern_and_bytes_0x00_0xff(kind):
    patterns = [b"\x00", b"\xff\x00", b"\xff", b"\x00\xff\xff", b"k"]
    hay = b"\x00\xff\xff\x00k\xff\x00\x00"
    check(patterns, hay, list(range(len(hay) + 1)), kind)
    if kind == STD:
        check(patterns, hay, list(range(len(hay) + 1)), kind, overlapping=True)


@pytest.mark.parametrize("kind", KINDS)
def test_a_node_with_256_children(kind):
    patterns = FAN + FAN_DEEP + [b"q"]
    hay = bytes([0, ord("x"), 127, ord("x"), 255, ord("x"), ord("q"), 0, ord("q"), 128, ord("q"), 255, ord("q"), ord("x"), 7])
    check(patterns, hay, list(range(len(hay) + 1)), kind)
    if kind == STD:
        check(patterns, hay, list(range(len(hay) + 1)), kind, overlapping=True)


@pytest.mark.parametrize("kind", KINDS)
def test_full_is_the_row_equals_a_pattern(kind):
    patterns = [b"ab", b"a", b"abc", b"ab"]
    rows = [b"ab", b"abc", b"abcd", b"a", b"", b"b", b"ab"]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    pat, end = check(patterns, b"".join(rows), None, kind, offsets=off, full=True)
    assert list(pat) == [0, 2, -1, 1, -1, -1, 0] and list(end) == [2, 3, -1, 1, -1, -1, 2]
    check(patterns, b"".join(rows), None, kind, offsets=off)  # the prefix form without full
    check(patterns, b"abc", None, kind, full=True)            # one row, no offsets
    if kind == STD:
        pat, end, ro = check(patterns, b"".join(rows), None, kind, offsets=off, full=True, overlapping=True)
        assert list(pat[ro[0]:ro[1]]) == [0, 3]
        check(patterns, b"".join(rows), None, kind, offsets=off, overlapping=True)


@pytest.mark.parametrize("kind", KINDS)
def test_case_insensitive_tables_with_mixed_case_data(kind):
    patterns = [b"Http", b"HTTPS", b"ftp", b"h", b"\xc3\x84x"]
    hay = b"hTTps://x HTTP FtP h \xc3\x84X \xc3\xa4x"
    pos = list(range(len(hay) + 1))
    pat, end = check(patterns, hay, pos, kind, fold=True)
    assert pat[0] == {STD: 3, LF: 0, LL: 1}[kind]
    assert pat[hay.index(b"\xc3\x84X")] == 4 and pat[hay.index(b"\xc3\xa4x")] == -1  # ASCII letters fold, nothing else does
    if kind == STD:
        check(patterns, hay, pos, kind, fold=True, overlapping=True)


CUTS = ([0, 11], [0, 3, 3, 3, 7, 11], [0, 1, 2, 4, 4, 8, 10, 11, 11], [0, 0, 0, 11, 11])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("offsets", CUTS)
def test_every_position_of_a_short_haystack_cut_into_rows(kind, offsets):
    hay = b"abcabcababc"
    pos = list(range(len(hay) + 1))
    check(NESTED + [b"bca"], hay, pos, kind, offsets=offsets)        # empty rows included: a position at several row starts
    check(NESTED + [b"bca"], hay, None, kind, offsets=offsets)       # ... and the rows themselves
    check(NESTED + [b"bca"], hay, pos[::-1] + [3, 3, 0], kind, offsets=offsets)  # unsorted, repeated
    if kind == STD:
        check(NESTED + [b"bca"], hay, pos, kind, offsets=offsets, overlapping=True)
        check(NESTED + [b"bca"], hay, None, kind, offsets=offsets, overlapping=True)


@pytest.mark.parametrize("kind", KINDS)
def test_a_row_end_cuts_a_pattern_one_byte_short(kind):
    patterns = [b"abcd", b"ab"]
    hay = b"abcdabcdabc"
    off = [0, 4, 7, 11]  # "abcd" fits row 0 exactly, is one byte short in row 1 and in row 2
    pat, end = check(patterns, hay, [0, 4, 8], kind, offsets=off)
    assert list(pat) == [{STD: 1, LF: 0, LL: 0}[kind], 1, 1]
    pat, end = check(patterns, hay, None, kind, offsets=off)
    assert list(end) == [{STD: 2, LF: 4, LL: 4}[kind], 2, -1]  # (row 2 is "dabc")
    pat, end = check([b"abcd"], hay, [0, 4, 8, 7, 11], kind, offsets=off)
    assert list(pat) == [0, -1, -1, -1, -1]


def test_seeded_small_cases():
    rng = np.random.default_rng(20)
    for case in range(150):
        alphabet = b"ab" if case % 3 else b"abcA"
        n = int(rng.integers(1, 9))
        patterns = [bytes(rng.choice(list(alphabet), size=int(rng.integers(1, 5)))) for _ in range(n)]
        hay = bytes(rng.choice(list(alphabet), size=int(rng.integers(0, 24))))
        cuts = sorted(int(x) for x in rng.integers(0, len(hay) + 1, size=int(rng.integers(0, 5))))
        offsets = None if case % 4 == 0 else [0] + cuts + [len(hay)]
        pos = [int(x) for x in rng.integers(0, len(hay) + 1, size=int(rng.integers(0, 12)))]
        kind = KINDS[case % 3]
        fold = case % 5 == 0
        check(patterns, hay, pos, kind, offsets=offsets, fold=fold, what=case)
        check(patterns, hay, None, kind, offsets=offsets, fold=fold, full=case % 2 == 0, what=case)
        if kind == STD:
            check(patterns, hay, pos, kind, offsets=offsets, fold=fold, overlapping=True, what=case)


def test_argument_errors():
    h = capi.HostAutomaton(NESTED, STD)
    hl = capi.HostAutomaton(NESTED, LF)
    try:
        def code(fn):
            with pytest.raises(ValueError) as e:
                fn()
            return e.value.code

        assert code(lambda: capi.match_at_host(h, b"abc", [0], offsets=[0, 2, 1, 3])) == capi.EINVAL   # unsorted offsets
        assert code(lambda: capi.match_at_host(h, b"abc", [0], offsets=[0, 2])) == capi.EINVAL         # they do not span the data
        assert code(lambda: capi.match_at_host(h, b"abc", [0], offsets=[1, 3])) == capi.EINVAL
        assert code(lambda: capi.match_at_host(h, b"abc", [4])) == capi.EINVAL                          # beyond len
        assert code(lambda: capi.match_at_host(h, b"abc", [-1])) == capi.EINVAL
        assert code(lambda: capi.match_at_host(h, b"abc", [0], flags=capi.AT_FULL)) == capi.EINVAL      # FULL without ROW_STARTS
        assert code(lambda: capi.match_at_host(h, b"abc", [0], flags=8)) == capi.EINVAL                 # an unknown flag
        assert code(lambda: capi.match_at_host(h, b"abc", [0], match_kind=3)) == capi.EINVAL
        assert code(lambda: capi.match_at_host(hl, b"abc", [0], flags=capi.AT_OVERLAPPING, match_kind=LF)) == capi.EOVERLAP
        L = capi.lib()
        one = np.zeros(2, dtype=np.int64)
        hay = np.frombuffer(b"abc", dtype=np.uint8)
        args = (hay.ctypes.data, 3, None, 0, one.ctypes.data, 1, 0, STD)
        assert L.acx_match_at_host(None, *args, one.ctypes.data, one.ctypes.data, None) == capi.EINVAL  # null handle
        assert L.acx_match_at_host(h._h, *args, None, one.ctypes.data, None) == capi.EINVAL             # null column
        assert L.acx_match_at_host(h._h, None, 3, None, 0, one.ctypes.data, 1, 0, STD, one.ctypes.data, one.ctypes.data, None) == capi.EINVAL
        assert L.acx_match_at_host(h._h, hay.ctypes.data, 3, None, 0, None, 1, 0, STD, one.ctypes.data, one.ctypes.data, None) == capi.EINVAL
        assert L.acx_match_at_host(h._h, *args[:6], capi.AT_OVERLAPPING, STD, None, None, None) == capi.EINVAL  # no row offsets
        # a position AT len is inside: no candidate
        pat, end = capi.match_at_host(h, b"abc", [3])
        assert list(pat) == [-1] and list(end) == [-1]
        # no anchors, no data
        pat, end = capi.match_at_host(h, b"", [])
        assert len(pat) == 0 and len(end) == 0
        pat, end = capi.match_at_host(h, b"", None, offsets=[0], flags=capi.AT_ROW_STARTS)
        assert len(pat) == 0
    finally:
        h.close()
        hl.close()


def test_the_tables_mean_what_the_walk_assumes():
    """children of s are the ids [first_child[s], first_child[s + 1]) with in_byte ascending, the root is nobody's child, bit 0
    of state_flags says own_off has entries, and the own lists are in id order: what at.hip relies on"""
    for kind in KINDS:
        h = capi.HostAutomaton(FAN + FAN_DEEP + [b"q", b"q", b"abc"], kind)
        try:
            fc, ib = h.first_child, h.in_byte
            assert fc[0] == 1 and fc[h.n_states] == h.n_states and np.all(np.diff(fc.astype(np.int64)) >= 0)
            assert fc[1] - fc[0] == 256
            for s in range(h.n_states):
                kids = ib[fc[s]:fc[s + 1]].astype(np.int64)
                assert np.all(np.diff(kids) > 0)
                own = h.own_pid[h.own_off[s]:h.own_off[s + 1]].astype(np.int64)
                assert bool(h.state_flags[s] & 1) == (len(own) > 0) and np.all(np.diff(own) > 0)
        finally:
            h.close()


def test_the_binding_and_the_extension_declare_the_new_names():
    L = capi.lib()
    for name in NEW_EXPORTS:
        assert hasattr(L, name), name
    with open(os.path.join(ROOT, "include", "acx.h")) as f:
        header = f.read()
    for name in NEW_EXPORTS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
    for name in ("match_at", "match_at_device", "match_at_into_device"):
        assert callable(getattr(capi.Automaton, name)), name
    assert callable(capi.match_at_host) and capi.DeviceMatchesAt._PREFIX == "at"
    assert (capi.AT_OVERLAPPING, capi.AT_FULL, capi.AT_ROW_STARTS) == tuple(
        int(re.search(r"#define\s+ACX_AT_" + n + r"\s+(\d+)u", header).group(1)) for n in ("OVERLAPPING", "FULL", "ROW_STARTS"))
    import ahocorasick_rs
    import ahocorasick_rs_amd
    for mod in (ahocorasick_rs, ahocorasick_rs_amd):
        assert "MatchesAt" in mod.__all__ and isinstance(mod.MatchesAt, type)
        for cls in (mod.AhoCorasick, mod.BytesAhoCorasick):
            assert callable(cls.match_at) and callable(cls.match_prefix_batch)
    assert ahocorasick_rs.MatchesAt is ahocorasick_rs_amd.MatchesAt
    with open(os.path.join(ROOT, "ahocorasick_rs_amd", "ahocorasick_rs.pyi")) as f:
        stubs = f.read()
    assert "class MatchesAt" in stubs and stubs.count("def match_at(") == 2 and stubs.count("def match_prefix_batch(") == 2


def test_constants_of_the_kernel_header():
    with open(os.path.join(ROOT, "ahocorasick_rs_amd", "csrc", "at.hpp")) as f:
        text = f.read()
    threads = int(re.search(r"constexpr uint32_t AT_THREADS\s*=\s*(\d+)", text).group(1))
    tile = int(re.search(r"constexpr uint32_t AT_TILE\s*=\s*(\d+)", text).group(1))
    assert threads % 64 == 0 and tile % threads == 0 and tile <= 65536
