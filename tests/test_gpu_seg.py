"""Greedy segmentation on the device (acx_segment / acx_segment_device / acx_segment_into_device; segment / segment_batch): the
raw form at the seams of its kernels -- data lengths around the tile, the fan of the composition tree and its third level;
chains that never converge, so that every entry offset of a tile is really taken; matches that cross a tile boundary by one
byte and by E - 1 bytes and end exactly on it; the longest pattern the stage takes; row starts at both ends of a tile and runs
of empty rows across a boundary and at the end of the data; the three row cuts; tiles in which no byte, every byte and one
byte per wave survives the first-byte test; a node at depth 2 with AT_PROBE children and with one more, at every outcome of
at_child's probe and search; a root with 256 children and an entry that stands four times in the list; a 4-byte character across a boundary; every alignment of the data -- with guard
bytes around all three outputs and every input verified unwritten; the kinds and routes through the C ABI, against
acx_segment_host and the definition; the Python methods with bytes, str (characters), sequences and tensors in HBM, torch as the
consumer and label_tokens_batch as the next stage.  Expected values come from the loop of the definition restated below in
plain Python -- the dictionary against the current position, no trie -- never from the library; the sizes are read from the
kernel's header."""
import gc
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
capi = pytest.importorskip("ahocorasick_rs_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ahocorasick_rs_amd", "csrc")

STD, LF, LL = capi.MATCH_STANDARD, capi.MATCH_LEFTMOST_FIRST, capi.MATCH_LEFTMOST_LONGEST
KINDS = (STD, LF, LL)
PY_KINDS = ("Standard", "LeftmostFirst", "LeftmostLongest")
UTF8 = capi.SEG_UTF8
GUARD = 0xC3


def hip_constants(path, names):
    src = open(os.path.join(CSRC, path)).read()
    out = {}
    for n in names:
        m = re.search(r"\b%s\s*=\s*(\d+)\s*[,;]" % n, src)
        assert m, f"{n} is no longer a plain constant of {path}"
        out[n] = int(m.group(1))
    return out


_C = hip_constants("seg.hpp", ("SEG_THREADS", "SEG_TILE", "SEG_FAN", "SEG_MAX_STEP"))
THREADS, TILE, FAN, MAX_STEP = _C["SEG_THREADS"], _C["SEG_TILE"], _C["SEG_FAN"], _C["SEG_MAX_STEP"]


def test_constants_are_what_the_sizes_below_assume():
    assert TILE % THREADS == 0 and THREADS % 64 == 0 and TILE >= 2 * THREADS and 16 <= MAX_STEP < TILE and FAN >= 2
    assert FAN * FAN * TILE + 1 <= (1 << 24) + 1


# ---------------------------------------------------------------------------
# the definition, restated: the dictionary against every position a piece begins at
# ---------------------------------------------------------------------------
def unit(h, p, L, utf8):
    b = h[p]
    if not utf8 or b < 0xC0 or b > 0xF7:
        return 1
    want = 2 if b < 0xE0 else 3 if b < 0xF0 else 4
    u = 1
    while u < want and p + u < L and 0x80 <= h[p + u] <= 0xBF:
        u += 1
    return u


def definition(patterns, hay, kind, *, offsets=None, utf8=False, fold=False):
    """(pattern, offsets, row_offsets).  The candidates at p are the patterns that stand there and end inside the row; of
    identical patterns every kind takes the lowest index, so a dict from the bytes to that index holds them all: one lookup
    per pattern length."""
    raw = bytes(hay)
    h = raw.lower() if fold else raw
    first = {}
    for i, x in enumerate(patterns):
        first.setdefault(bytes(x).lower() if fold else bytes(x), i)
    lengths = sorted({len(x) for x in first})
    key = {STD: lambda c: (c[1], c[0]), LF: lambda c: c[0], LL: lambda c: (-c[1], c[0])}[kind]
    off = [0, len(raw)] if offsets is None else [int(x) for x in offsets]
    pat, bounds, ro = [], [], []
    for r in range(len(off) - 1):
        p, L = off[r], off[r + 1]
        ro.append(len(pat))
        while p < L:
            C = [(first[h[p:p + n]], p + n) for n in lengths if p + n <= L and h[p:p + n] in first]
            i, e = min(C, key=key) if C else (-1, p + unit(raw, p, L, utf8))
            pat.append(i)
            bounds.append(p)
            p = e
    ro.append(len(pat))
    bounds.append(len(raw))
    return np.asarray(pat, dtype=np.int64).reshape(-1), np.asarray(bounds, dtype=np.int64), np.asarray(ro, dtype=np.int64)


def entries_taken(bounds, n):
    """the tile offsets at which the chain enters the tiles behind the first"""
    starts = np.arange(TILE, n, TILE)
    return set((bounds[np.searchsorted(bounds, starts, side="left")] - starts).tolist())


def host_chain(patterns, hay, kind, offsets=None, utf8=False, fold=False):
    h = capi.HostAutomaton(patterns, kind, capi.BUILD_ASCII_CASE_INSENSITIVE if fold else 0)
    try:
        return capi.segment_host(h, hay, offsets=offsets, flags=UTF8 if utf8 else 0, match_kind=kind)
    finally:
        h.close()


def same(got, want, what):
    for g, w, name in zip(got, want, ("pattern", "offsets", "row_offsets")):
        assert len(g) == len(w), (what, name, len(g), len(w))
        bad = np.flatnonzero(g != w)
        assert not len(bad), (what, name, int(bad[0]), g[bad[:8]], w[bad[:8]])


# ---------------------------------------------------------------------------
# the raw form: acx_segment_into_device with guards
# ---------------------------------------------------------------------------
def run_raw(a, hay, cap, *, offsets=None, uniform=0, flags=0, base_res=0):
    """hay at base_res modulo 16; the three outputs each between 64 guard bytes, sized for `cap` pieces -> (T, pattern,
    offsets, row_offsets as they lie in memory behind the call); the guards and every input checked unwritten"""
    hay = np.frombuffer(bytes(hay), dtype=np.uint8)
    n = len(hay)
    rows = (len(offsets) - 1) if offsets is not None else (n // uniform if uniform else 1)
    img_h = np.full(n + 48, GUARD, dtype=np.uint8)
    img_h[base_res:base_res + n] = hay
    d_hay = capi.DeviceBuffer(len(img_h)).upload(img_h)
    assert d_hay.ptr % 16 == 0
    sizes = (cap, cap + 1, rows + 1)
    imgs = [np.full(64 + 8 * k + 64, GUARD, dtype=np.uint8) for k in sizes]
    bufs = [capi.DeviceBuffer(len(img) + 16).upload(img) for img in imgs]
    d_off = None
    if offsets is not None:
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64))
        d_off = capi.DeviceBuffer(8 * len(off)).upload(off)
    try:
        T = a.segment_into_device(d_hay.ptr + base_res, n, cap, bufs[0].ptr + 64, bufs[1].ptr + 64, bufs[2].ptr + 64, flags,
                                  d_offsets=d_off.ptr if d_off else 0, n_hay=rows if (d_off or uniform) else 0, uniform_len=uniform)
        got = [b.download(len(img)) for b, img in zip(bufs, imgs)]
        assert np.array_equal(d_hay.download(len(img_h)), img_h), "the data (or a byte around it) was written"
        if d_off:
            assert np.array_equal(d_off.download(8 * len(off)).view(np.uint64), off), "the offsets were written"
    finally:
        for b in [d_hay, d_off] + bufs:
            if b:
                b.free()
    out = []
    for g, k, name in zip(got, sizes, ("pattern", "offsets", "row_offsets")):
        assert (g[:64] == GUARD).all(), ("a byte before the output was written", name)
        assert (g[64 + 8 * k:] == GUARD).all(), ("a byte behind the output was written", name)
        out.append(g[64:64 + 8 * k].copy())
    return T, out


def check_raw(patterns, kind, hay, *, offsets=None, uniform=0, utf8=False, fold=False, what=None, automaton=None, base_res=0,
              want=None):
    """want: the expected columns when they are not the definition's (the host form's)"""
    cut = offsets if offsets is not None else (np.arange(0, len(hay) + 1, uniform) if uniform else None)
    if want is None:
        want = definition(patterns, hay, kind, offsets=cut, utf8=utf8, fold=fold)
    a = automaton or capi.Automaton(patterns, kind, ascii_case_insensitive=fold)
    try:
        T, out = run_raw(a, hay, len(want[0]), offsets=offsets, uniform=uniform, flags=UTF8 if utf8 else 0, base_res=base_res)
    finally:
        if not automaton:
            a.close()
    assert T == len(want[0]), (what, T, len(want[0]))
    same([o.view(np.int64) for o in out], want, what)
    return want


LONG = b"gattacagattacagattacagattacagattacagatta"  # 40 bytes: the longest pattern of MIXED
MIXED = [b"a", b"bc", b"def", LONG, b"ab", b"abc", b"bcd", LONG[:7], b"de", b"g"]


def planted(n, seed, patterns=MIXED, alphabet=b"abcdefgxyz", every=9):
    rng = np.random.default_rng(seed)
    hay = bytearray(rng.choice(list(alphabet), size=n).astype(np.uint8).tobytes())
    for k in range(0, max(n - 48, 0), every):
        p = patterns[int(rng.integers(0, len(patterns)))]
        hay[k:k + len(p)] = p
    return bytes(hay[:n])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_raw_data_lengths_around_the_tile(kind, n):
    check_raw(MIXED, kind, planted(n, n), what=n)


def test_raw_one_level_of_the_tree_is_full_and_one_tile_more():
    n = FAN * TILE + 1
    check_raw(MIXED, LL, planted(n, 7, every=23), what=n)


def test_raw_three_tree_levels():
    """16 MiB: FAN * FAN tiles and one byte -- two words of 251 and MAX_STEP bytes in a seeded order, so that the pieces are
    few (the reference stays a Python loop) and the entries differ from tile to tile"""
    n = FAN * FAN * TILE + 1
    rng = np.random.default_rng(16)
    A, B = bytes(rng.integers(97, 123, size=251, dtype=np.uint8)), bytes(rng.integers(97, 123, size=MAX_STEP, dtype=np.uint8))
    order = rng.integers(0, 2, size=n // 251 + 2)
    hay = b"".join(A if k else B for k in order)[:n]
    want = check_raw([A, B, b"q"], LL, hay, what="three levels")
    assert len(entries_taken(want[1], n)) > 200 and want[0][-1] == -1  # (the last word is cut short: unknown bytes)


@pytest.mark.parametrize("residue", [0, 1, 2])
def test_raw_a_chain_of_aaa_never_converges(residue):
    n = 4 * TILE + residue
    while n % 3 != residue:
        n += 1
    want = check_raw([b"aaa"], LL, b"a" * n, what=residue)
    assert entries_taken(want[1], n) == {0, 1, 2} or TILE % 3 == 0
    assert len(want[0]) == n // 3 + residue and (want[0][-1] == -1) == (residue != 0)


def test_raw_words_of_5_and_7_bytes_take_every_entry_offset():
    rng = np.random.default_rng(57)
    P5, P7 = b"hello", b"goodbye"
    n = 48 * TILE + 3
    hay = b"".join(P5 if k else P7 for k in rng.integers(0, 2, size=n // 5 + 2))[:n]
    for kind in KINDS:
        want = check_raw([P5, P7], kind, hay, what="5 and 7")
        assert entries_taken(want[1], n) == set(range(7))  # E = 7: every entry of the map is a real one somewhere


W = b"gattacaXY"  # 9 bytes: E = 9


@pytest.mark.parametrize("kind", KINDS)
def test_raw_matches_across_and_on_a_tile_boundary(kind):
    m = len(W)
    for start, what in ((TILE - m + 1, "across by one byte"), (TILE - 1, "across by E - 1 bytes"), (TILE - m, "ends on the boundary"),
                        (TILE, "begins on the boundary")):
        hay = bytearray(b"z" * (2 * TILE + 5))
        hay[start:start + m] = W
        hay[2 * TILE - 1:2 * TILE - 1 + m] = W  # ... and one cut short by the end of the data
        want = check_raw([W, b"ga"], kind, bytes(hay), what=what)
        assert start in want[1].tolist() and (kind == STD or start + m in want[1].tolist()), what


def test_raw_the_longest_pattern_across_a_boundary_and_one_byte_more_is_refused():
    rng = np.random.default_rng(256)
    word = bytes(rng.integers(97, 123, size=MAX_STEP, dtype=np.uint8))
    hay = bytearray(b"." * (3 * TILE))
    for start in (TILE - 1, 2 * TILE - MAX_STEP + 1, 3 * TILE - MAX_STEP):
        hay[start:start + MAX_STEP] = word
    want = check_raw([word, word[:3]], LL, bytes(hay), what="MAX_STEP")
    assert (want[0] == 0).sum() == 3
    a = capi.Automaton([word + b"x", b"ab"], LL)
    try:
        with pytest.raises(ValueError) as e:
            a.segment_into_device(0, 0, 0, 0, 0, 0)
        assert e.value.code == capi.EINVAL  # (no outputs: the arguments come first)
        d = capi.DeviceBuffer(256)
        with pytest.raises(ValueError) as e:
            a.segment_into_device(d.ptr, 16, 0, d.ptr, d.ptr + 64, d.ptr + 128)
        assert e.value.code == capi.ETOOBIG
        with pytest.raises(ValueError) as e:
            a.segment_device(d.ptr, 16)
        assert e.value.code == capi.ETOOBIG
        with pytest.raises(ValueError) as e:
            a.segment(None, single=b"abab")
        assert e.value.code == capi.ETOOBIG
        d.free()
    finally:
        a.close()


@pytest.mark.parametrize("kind", KINDS)
def test_raw_row_starts_at_both_ends_of_a_tile_and_runs_of_empty_rows(kind):
    n = 3 * TILE + 11
    hay = planted(n, 33, every=5)
    off = [0, 0, 0, 5, TILE - 1, TILE - 1, TILE - 1, TILE, TILE, TILE, TILE + 1, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1,
           3 * TILE - 1, 3 * TILE - 1, 3 * TILE, 3 * TILE, 3 * TILE + 1, n, n, n]
    want = check_raw(MIXED, kind, hay, offsets=off, what="row starts")
    assert set(off) <= set(want[1].tolist())
    # a pattern cut by a row end at the tile boundary and one byte before it
    hay2 = bytearray(b"z" * (2 * TILE))
    hay2[TILE - 5:TILE + 4] = W
    hay2[2 * TILE - 9:2 * TILE] = W
    for cut in (TILE - 1, TILE, TILE + 1, TILE + 3, TILE + 4):
        check_raw([W, b"ga", b"tt"], kind, bytes(hay2), offsets=[0, cut, 2 * TILE - 1, 2 * TILE], what=cut)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form", ["offsets", "uniform", "neither"])
def test_raw_the_three_row_cuts(kind, form):
    n = 2 * 77 * (TILE // 77 + 1)  # three tiles, and 1, 2, 7 and 77 divide it
    hay = planted(n, 9, every=4)
    if form == "offsets":
        cuts = np.sort(np.random.default_rng(5).integers(0, n + 1, size=300))
        check_raw(MIXED, kind, hay, offsets=np.concatenate([[0], cuts, [n]]), what=form)
    elif form == "uniform":
        for u in (1, 2, 7, 77, n // 2, n):
            check_raw(MIXED, kind, hay, uniform=u, what=(form, u))
        check_raw(MIXED, kind, hay[:TILE + TILE // 2], uniform=TILE // 2, what=(form, "half tiles"))
        check_raw(MIXED, kind, hay[:2 * TILE], uniform=TILE, what=(form, "whole tiles"))
    else:
        check_raw(MIXED, kind, hay, what=form)


@pytest.mark.parametrize("u", [1, 16, TILE - 1, TILE, TILE + 1, 2 * TILE])
def test_raw_rows_of_one_length_that_begin_on_before_and_behind_a_tile_boundary(u):
    """Exactly u * n bytes, n the smallest number of rows that gives more than two tiles (3 for the three lengths around the
    tile): row starts fall on a tile's first byte, one byte before it and one byte behind it -- the marks of k_seg leave out
    the one ON the first byte.  Dictionary words among x, y and z, which no entry begins with; against acx_segment_host over
    the same cut written as offsets, entry for entry."""
    n = {1: 2 * TILE + 1, 16: 2 * TILE // 16 + 1, 2 * TILE: 2}.get(u, 3)
    assert u * n > 2 * TILE
    hay = planted(u * n, u, every=5)
    want = host_chain(MIXED, hay, LL, offsets=np.arange(n + 1, dtype=np.uint64) * u)
    assert len(want[2]) == n + 1 and (want[0] == -1).any() and (want[0] >= 0).any()
    check_raw(MIXED, LL, hay, uniform=u, what=("row length", u), want=want)


def test_raw_no_byte_every_byte_and_one_byte_per_wave_survive_the_first_byte():
    n = TILE + 300
    for kind in KINDS:
        want = check_raw([b"ab", b"abc", b"b"], kind, b"z" * n, what="no survivor")
        assert (want[0] == -1).all() and len(want[0]) == n
        hay = np.random.default_rng(3).choice(list(b"abc"), size=n).astype(np.uint8).tobytes()
        want = check_raw([b"a", b"b", b"c", b"ab"], kind, hay, what="every byte survives")
        assert (want[0] >= 0).all()
        one = bytearray(b"z" * n)
        one[5::64] = b"a" * len(one[5::64])
        one[6::128] = b"b" * len(one[6::128])
        want = check_raw([b"ab", b"ac", b"a"], kind, bytes(one), what="one survivor per wave")
        assert (want[0] >= 0).sum() == len(one[5::64])
        alone = bytearray(b"z" * n)
        alone[TILE - 1] = ord("a")  # a survivor whose walk finds nothing: the unknown unit behind the walk
        check_raw([b"ab"], kind, bytes(alone), what="a walk without a match")


PROBE = hip_constants("at.hpp", ("AT_PROBE",))["AT_PROBE"]  # children up to which at_child probes a node linearly


def deep_node(m, head=b"qw"):
    """patterns that put a node with exactly m children at depth len(head) -- child bytes 0x30, 0x34, .. -- and behind every
    child a short and a long pattern, in either index order: the three kinds pick differently, and all of them search the node"""
    pats = []
    for k in range(m):
        c = head + bytes([0x30 + 4 * k])
        pats += [c + b"xy", c] if k % 2 else [c, c + b"xy"]
    return pats


def deep_probes(m):
    """a byte for the node's first, a middle and its last child; one below the first, between two and above the last"""
    child = [0x30 + 4 * k for k in range(m)]
    return [child[0], child[m // 2], child[-1]], [child[0] - 1, child[1] + 1, child[-1] + 1]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m", [PROBE, PROBE + 1])
def test_raw_a_node_at_depth_2_with_probe_and_one_more_children(kind, m):
    """at_child below depth 1 inside k_seg: the linear probe at AT_PROBE children, the binary search at one more -- every
    outcome of either, and one walk that reads the node's byte from the last byte of a tile and one from the next tile"""
    pats = deep_node(m)
    hits, misses = deep_probes(m)
    hay = bytearray(b"." * (2 * TILE + 40))
    for k, b in enumerate(hits + misses):
        hay[3 + 7 * k:8 + 7 * k] = b"qw" + bytes([b]) + b"xy"
    hay[TILE - 3:TILE + 2] = b"qw" + bytes([hits[2]]) + b"xy"          # the node's byte is the tile's last one
    hay[2 * TILE - 2:2 * TILE + 3] = b"qw" + bytes([hits[1]]) + b"xy"  # ... and the next tile's first one
    want = check_raw(pats, kind, bytes(hay), what=(m, "one row"))
    at = {int(p): int(i) for i, p in zip(want[0], want[1][:-1])}
    for k, b in enumerate(hits):
        child = (b - 0x30) // 4
        short, long_ = (2 * child + 1, 2 * child) if child % 2 else (2 * child, 2 * child + 1)
        assert at[3 + 7 * k] == {STD: short, LF: min(short, long_), LL: long_}[kind], (m, k)
    assert [at[3 + 7 * k] for k in range(3, 6)] == [-1, -1, -1] and at[TILE - 3] >= 0 and at[2 * TILE - 2] >= 0
    assert (want[0] >= 0).sum() == 5
    check_raw(pats, kind, bytes(hay), offsets=[0, 8, TILE - 1, TILE, 2 * TILE, len(hay)], what=(m, "rows"))  # rows cut both tile walks short


@pytest.mark.parametrize("kind", KINDS)
def test_raw_a_root_with_256_children_and_an_entry_four_times(kind):
    """every first byte survives the first-byte test; "dup!" stands four times in the pattern list (own1 says "many": the first of
    the state's list is read) behind an extension of it with a lower index: the lowest of the four comes back under every kind"""
    fan = [bytes([b]) + b"z" for b in range(256)]
    pats = fan[:100] + [b"dup!x"] + fan[100:200] + [b"dup!", b"dup!"] + fan[200:] + [b"dup!", b"dup!"]
    low = pats.index(b"dup!")
    assert pats.count(b"dup!") == 4 and len({p[0] for p in pats}) == 256
    hay = bytearray(b"".join(bytes([b]) + b"z" for b in (0, 1, 0x64, 0x7F, 0x80, 0xFF)) + b"dup!dup!?dup!xdu" + bytes(range(256)))
    hay += b"." * (TILE - 2 - len(hay)) + b"dup!dup!"
    want = check_raw(pats, kind, bytes(hay), what="256 children")
    at = {int(p): int(i) for i, p in zip(want[0], want[1][:-1])}
    assert at[12] == low and at[16] == low and at[TILE - 2] == low and at[TILE + 2] == low
    assert at[21] == {STD: low, LF: pats.index(b"dup!x"), LL: pats.index(b"dup!x")}[kind]
    assert [at[2 * k] for k in range(6)] == [pats.index(bytes([b]) + b"z") for b in (0, 1, 0x64, 0x7F, 0x80, 0xFF)]
    a = capi.Automaton(pats, kind)
    try:
        check_raw(pats, kind, bytes(hay), automaton=a, offsets=[0, 14, 15, TILE, len(hay)], what="256 children, rows")
    finally:
        a.close()


@pytest.mark.parametrize("utf8", [False, True])
def test_raw_a_4_byte_character_across_a_tile_boundary(utf8):
    face = "\U0001f600".encode()
    for k in (1, 2, 3):
        hay = b"z" * (TILE - k) + face + "zä€".encode() + face[:2]  # ... and an ill-formed one at the end of the data
        want = check_raw(["ä".encode(), b"zz"], LL, hay, utf8=utf8, what=k)
        assert ((TILE - k + 4 in want[1].tolist()) and (TILE in want[1].tolist()) == (not utf8)) or TILE < 8
    rows = [0, TILE - 2, TILE + 1, len(hay)]  # a row end inside the character
    check_raw(["ä".encode()], LL, hay, offsets=rows, utf8=utf8, what="clipped by a row end")
    check_raw([b"x"], STD, b"\x80\xbf\xf0\x9f\xe2\x82z\xc3" * 700, utf8=utf8, what="stray and short")


@pytest.mark.parametrize("base_res", range(16))
def test_raw_every_alignment_of_the_data(base_res):
    n = TILE + 100 + base_res
    check_raw(MIXED, (STD, LF, LL)[base_res % 3], planted(n, base_res, every=6), base_res=base_res,
              offsets=[0, 3, TILE - base_res, n] if base_res % 2 else None, what=base_res)


def test_raw_a_cap_below_the_count_writes_nothing_and_reports_it():
    hay = planted(TILE + 50, 12)
    want = definition(MIXED, hay, LL)
    T = len(want[0])
    a = capi.Automaton(MIXED, LL)
    try:
        for cap in (0, 1, T - 1):
            got_T, out = run_raw(a, hay, cap)
            assert got_T == T and all((o == GUARD).all() for o in out), cap
        got_T, out = run_raw(a, hay, T + 5)  # room to spare: exactly T, T + 1 and rows + 1 words are written
        assert got_T == T
        same([out[0][:8 * T].view(np.int64), out[1][:8 * (T + 1)].view(np.int64), out[2].view(np.int64)], want, "spare room")
        assert (out[0][8 * T:] == GUARD).all() and (out[1][8 * (T + 1):] == GUARD).all()
        got_T, out = run_raw(a, b"", 0, offsets=[0, 0, 0])
        assert got_T == 0 and list(out[1].view(np.int64)) == [0] and list(out[2].view(np.int64)) == [0, 0, 0]
    finally:
        a.close()


# ---------------------------------------------------------------------------
# handles and routes through the C ABI
# ---------------------------------------------------------------------------
def device_call(a, hay, flags, offsets=None, uniform=0):
    hay = np.frombuffer(bytes(hay), dtype=np.uint8)
    d_hay = capi.DeviceBuffer(len(hay) + 16)
    if len(hay):
        d_hay.upload(hay)
    d_off, rows = None, 0
    if offsets is not None:
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64))
        d_off = capi.DeviceBuffer(8 * len(off)).upload(off)
        rows = len(off) - 1
    elif uniform:
        rows = len(hay) // uniform
    try:
        r = a.segment_device(d_hay.ptr, len(hay), flags, d_offsets=d_off.ptr if d_off else 0, n_hay=rows, uniform_len=uniform)
        try:
            assert r.on_device and r.pattern_ptr() and r.offsets_ptr() and r.row_offsets_ptr()
            out = (r.pattern(), r.offsets(), r.row_offsets())
            assert r.count == len(out[0]) and r.rows == len(out[2]) - 1
            assert np.array_equal(d_hay.download(len(hay)), hay), "the data was written"
        finally:
            r.free()
    finally:
        for b in (d_hay, d_off):
            if b:
                b.free()
    return out


def host_call(a, hay, flags, offsets=None, codepoints=False):
    if offsets is None:
        r = a.segment(None, flags, codepoints, single=bytes(hay))
    else:
        r = a.segment([bytes(hay[int(offsets[i]):int(offsets[i + 1])]) for i in range(len(offsets) - 1)], flags, codepoints)
    try:
        assert not r.on_device
        return r.pattern(), r.offsets(), r.row_offsets()
    finally:
        r.free()


def check_abi(patterns, kind, hay, *, offsets=None, utf8=False, fold=False, what=None):
    want = definition(patterns, hay, kind, offsets=offsets, utf8=utf8, fold=fold)
    flags = UTF8 if utf8 else 0
    a = capi.Automaton(patterns, kind, ascii_case_insensitive=fold)
    try:
        legs = [("device", device_call(a, hay, flags, offsets)), ("host", host_call(a, hay, flags, offsets))]
    finally:
        a.close()
    legs.append(("acx_segment_host", host_chain(patterns, hay, kind, offsets, utf8, fold)))
    for leg, got in legs:
        same(got, want, (what, leg))
    return want


@pytest.mark.parametrize("kind", KINDS)
def test_abi_three_kinds_host_and_device_inputs(kind):
    hay = planted(TILE + 700, 21, every=6)
    cuts = np.sort(np.random.default_rng(3).integers(0, len(hay) + 1, size=60))
    off = np.concatenate([[0], cuts, [len(hay)]])
    dup = MIXED + [b"a", b"abc", LONG]  # copies: the lowest index is reported
    check_abi(dup, kind, hay, what="one haystack")
    check_abi(dup, kind, hay, offsets=off, what="rows")
    check_abi(dup, kind, b"", what="no data")
    check_abi(dup, kind, b"", offsets=[0, 0, 0], what="empty rows only")
    check_abi(dup, kind, "aä€\U0001f600bc".encode() * 30, utf8=True, what="utf8")


def test_abi_codepoints_give_character_boundaries():
    text = "übergrößenträger 日本語のテキスト \U0001f600 ok"
    pats = ["größe".encode(), "日本".encode(), b"ok", "ü".encode()]
    a = capi.Automaton(pats, LL)
    try:
        pat, bounds, ro = host_call(a, text.encode(), 0, codepoints=True)  # (codepoints implies the flag)
    finally:
        a.close()
    want = definition(pats, text.encode(), LL, utf8=True)
    chars = [len(text.encode()[:b].decode()) for b in want[1]]
    assert list(bounds) == chars and list(pat) == list(want[0]) and bounds[-1] == len(text)


def test_abi_a_case_insensitive_handle_leaves_the_tensor_as_it_is():
    pats = [b"Http", b"HTTPS", b"ftp", b"h", b"\xc3\x84x"]
    hay = (b"hTTps://x HTTP FtP h \xc3\x84X \xc3\xa4x " * 150)
    for kind in KINDS:
        check_abi(pats, kind, hay, fold=True)  # (device_call asserts the data unchanged)
        check_abi(pats, kind, hay, offsets=np.concatenate([np.arange(0, len(hay), 31), [len(hay)]]), fold=True, utf8=True)


@pytest.mark.parametrize("kind", KINDS)
def test_abi_a_handle_kept_in_compressed_form_only(kind, monkeypatch):
    monkeypatch.setenv("ACX_DENSE_LIMIT", "0")
    hay = planted(TILE + 900, 5, every=6)
    a = capi.Automaton(MIXED, kind)
    try:
        assert a.info.table_bytes == 0, "the dense table was built after all"
    finally:
        a.close()
    check_abi(MIXED, kind, hay, what="compressed")
    check_abi(MIXED, kind, hay, offsets=np.arange(0, len(hay) + 1, 4), what="compressed, rows")


def test_abi_refusals():
    a = capi.Automaton(MIXED, LL)
    try:
        def code(fn):
            with pytest.raises(ValueError) as e:
                fn()
            return e.value.code

        assert code(lambda: a.segment(None, 2, single=b"abc")) == capi.EINVAL  # an unknown flag
        assert code(lambda: a.segment_device(0, 0, 4)) == capi.EINVAL
        assert code(lambda: a.segment_device(0, 5)) == capi.EINVAL              # bytes and nowhere to read them
        L = capi.lib()
        off = np.asarray([0, 2, 1, 3], dtype=np.uint64)
        hay = np.frombuffer(b"abc", dtype=np.uint8)
        out = capi.ctypes.c_void_p()
        assert L.acx_segment(a._h, hay.ctypes.data, 3, off.ctypes.data, 3, 0, 0, capi.ctypes.byref(out)) == capi.EINVAL
        assert L.acx_segment(a._h, hay.ctypes.data, 3, None, 2, 0, 0, capi.ctypes.byref(out)) == capi.EINVAL
        assert L.acx_segment(None, hay.ctypes.data, 3, None, 0, 0, 0, capi.ctypes.byref(out)) == capi.EINVAL
        assert L.acx_segment(a._h, hay.ctypes.data, 3, None, 0, 0, 0, None) == capi.EINVAL
        one = np.zeros(4, dtype=np.int64)
        assert L.acx_seg_copy(None, 0, one.ctypes.data) == capi.EINVAL and L.acx_seg_count(None) == 0
        r = a.segment(None, single=b"abc")
        assert L.acx_seg_copy(r._h, 3, one.ctypes.data) == capi.EINVAL
        assert r.count == 1 and r.rows == 1 and list(r.offsets()) == [0, 3] and list(r.row_offsets()) == [0, 1]
        r.free()
    finally:
        a.close()


# ---------------------------------------------------------------------------
# the Python methods
# ---------------------------------------------------------------------------
def triples(want, off=None):
    """what tolist() gives: (pattern, start, end) local to the row, one list per row when there are rows"""
    pat, bounds, ro = want
    rows = []
    for r in range(len(ro) - 1):
        b = int(bounds[ro[r]]) if ro[r] < len(pat) else 0
        rows.append([(int(pat[k]), int(bounds[k]) - b, int(bounds[k + 1]) - b) for k in range(ro[r], ro[r + 1])])
    return rows if off is not None else rows[0]


def test_python_bytes_and_sequences():
    import ahocorasick_rs as ar
    hay = planted(TILE + 333, 8, every=7)
    for k, kind in enumerate(KINDS):
        b = ar.BytesAhoCorasick(MIXED, matchkind=getattr(ar.MatchKind, PY_KINDS[k]))
        want = definition(MIXED, hay, kind)
        s = b.segment(hay)
        assert isinstance(s, ar.Segments) and len(s) == len(want[0]) and s.row_offsets is None and s.device is None
        assert s.tolist() == triples(want)
        assert np.array_equal(np.from_dlpack(s.pattern), want[0]) and np.array_equal(np.from_dlpack(s.offsets), want[1])
        assert s.tolist() == b.segment(bytearray(hay)).tolist() == b.segment(memoryview(hay)).tolist()
        rows = [hay[:10], b"", hay[10:TILE + 1], b"", b"", hay[TILE + 1:], b""]
        off = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
        want = definition(MIXED, hay, kind, offsets=off)
        s = b.segment_batch(rows)
        assert len(s) == len(want[0]) and s.tolist() == triples(want, off)
        assert np.array_equal(np.from_dlpack(s.row_offsets), want[2]) and np.array_equal(np.from_dlpack(s.offsets), want[1])
        assert b.segment_batch([]).tolist() == [] and b.segment(b"").tolist() == [] and b.segment_batch([b"", b""]).tolist() == [[], []]
        assert b.segment("ä€z".encode(), utf8=True).tolist() == [(-1, 0, 2), (-1, 2, 5), (-1, 5, 6)]
        assert len(b.segment("ä€z".encode())) == 6 == len(b.segment("ä€z".encode(), utf8=None))


def test_python_str_in_characters_with_multi_byte_text():
    import ahocorasick_rs as ar
    words = ["größe", "日本", "ok", "ü", "un", "##able", "日"]
    text = "übergrößenträger 日本語のテキスト \U0001f600 ok unable"
    for k, kind in enumerate(KINDS):
        a = ar.AhoCorasick(words, matchkind=getattr(ar.MatchKind, PY_KINDS[k]))
        want = definition([w.encode() for w in words], text.encode(), kind, utf8=True)
        chars = [len(text.encode()[:b].decode()) for b in want[1]]
        s = a.segment(text)
        assert s.tolist() == [(int(i), chars[j], chars[j + 1]) for j, i in enumerate(want[0])]
        assert all(e - b == 1 for i, b, e in s.tolist() if i < 0)  # an unknown piece is one character
        assert "".join(text[b:e] for _, b, e in s.tolist()) == text
        assert a.segment(text, utf8=True).tolist() == s.tolist() and a.segment("plain ok").tolist()[-1] == (2, 6, 8)
        rows = [text, "", "日本ok", "é"]
        got = a.segment_batch(rows).tolist()
        assert got == [a.segment(r).tolist() for r in rows]


def test_python_errors():
    import ahocorasick_rs as ar
    a = ar.AhoCorasick(["ab"], matchkind=ar.MatchKind.LeftmostLongest)
    b = ar.BytesAhoCorasick([b"ab"], matchkind=ar.MatchKind.LeftmostLongest)
    for ac, hay in ((a, "abc"), (b, b"abc")):
        for bad in (1, 0, "yes", b"", 1.0):
            with pytest.raises(TypeError):
                ac.segment(hay, utf8=bad)
            with pytest.raises(TypeError):
                ac.segment_batch([hay], utf8=bad)
        with pytest.raises(TypeError):
            ac.segment(hay, True)  # utf8 is keyword-only
        with pytest.raises(TypeError):
            ac.segment_batch([hay], offsets=[0, 3])  # offsets / row_length cut ONE tensor, not a sequence
        with pytest.raises(TypeError):
            ac.segment_batch([hay], row_length=3)
        with pytest.raises(TypeError):
            ac.segment()
    with pytest.raises(ValueError):
        a.segment("abc", utf8=False)  # a str is cut at characters
    with pytest.raises(TypeError):
        a.segment(b"abc")
    with pytest.raises(TypeError):
        b.segment("abc")
    host = np.frombuffer(b"abcabc", dtype=np.uint8).copy()  # (a writable array: numpy exports no read-only one)
    with pytest.raises(TypeError):
        b.segment_batch(host, offsets=np.asarray([0, 3, 6]), row_length=3)  # exactly one of the two
    with pytest.raises(ValueError):
        b.segment_batch(host, row_length=4)
    with pytest.raises(ValueError):
        b.segment_batch(host, offsets=np.asarray([0, 4, 3, 6]))
    assert b.segment_batch(host, row_length=3).tolist() == [[(0, 0, 2), (-1, 2, 3)]] * 2
    assert b.segment_batch(host, offsets=np.asarray([0, 1, 6])).tolist() == [[(-1, 0, 1)], [(-1, 0, 1), (-1, 1, 2), (0, 2, 4), (-1, 4, 5)]]
    long_ = ar.BytesAhoCorasick([b"x" * (MAX_STEP + 1)])
    with pytest.raises(ValueError):
        long_.segment(b"xxx")
    with pytest.raises(TypeError):
        ar.Segments()


def test_python_host_columns_outlive_the_result_and_the_automaton():
    import ahocorasick_rs as ar
    hay = planted(TILE + 400, 4, every=5)
    want = definition(MIXED, hay, STD)
    b = ar.BytesAhoCorasick(MIXED)
    s = b.segment(hay)
    pat, bounds = np.from_dlpack(s.pattern), np.from_dlpack(s.offsets)
    del s, b
    gc.collect()
    other = ar.BytesAhoCorasick(MIXED)
    for k in range(20):  # (other results come and go where the columns would be if they had been freed)
        other.segment(planted(TILE + 400, 50 + k))
    assert np.array_equal(pat, want[0]) and np.array_equal(bounds, want[1])


def test_python_seeded_random_cases():
    import ahocorasick_rs as ar
    rng = np.random.default_rng(2025)
    for case in range(120):
        alphabet = b"ab" if case % 3 else b"abcA\xc3\xa4\xe2"
        n = int(rng.integers(1, 9))
        patterns = [rng.choice(list(alphabet), size=int(rng.integers(1, 6))).astype(np.uint8).tobytes() for _ in range(n)]
        hay = rng.choice(list(alphabet), size=int(rng.integers(0, 60))).astype(np.uint8).tobytes()
        cuts = sorted(int(x) for x in rng.integers(0, len(hay) + 1, size=int(rng.integers(0, 6))))
        off = [0] + cuts + [len(hay)]
        rows = [hay[off[i]:off[i + 1]] for i in range(len(off) - 1)]
        k, fold, utf8 = case % 3, case % 5 == 0, case % 2 == 1
        b = ar.BytesAhoCorasick(patterns, matchkind=getattr(ar.MatchKind, PY_KINDS[k]), ascii_case_insensitive=fold)
        assert b.segment(hay, utf8=utf8).tolist() == triples(definition(patterns, hay, KINDS[k], utf8=utf8, fold=fold)), case
        assert b.segment_batch(rows, utf8=utf8).tolist() == triples(definition(patterns, hay, KINDS[k], offsets=off, utf8=utf8, fold=fold), off), case
        if case % 10 == 0:  # ... and the same through the C ABI on device inputs, rows included
            check_abi(patterns, KINDS[k], hay, offsets=off, utf8=utf8, fold=fold, what=case)


_TENSOR_SCRIPT = r"""
import gc
import sys
import torch  # first: one process holds ONE HIP runtime, and torch must be the one to load it
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
import ahocorasick_rs as ar
from test_gpu_seg import MIXED, LONG, KINDS, PY_KINDS, TILE, definition, planted, triples

dev = "cuda:0"
lines = [b"abc def", b"", b"gattaca", LONG, b"def", b"", b"", b"bcd!", b"xa", planted(700, 3)] * 12
data = b"\n".join(lines) + b"\n"
assert len(data) > 2 * TILE
t = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev)
ro = ar.split_rows(t)
off = torch.from_dlpack(ro.offsets)
off_np = off.cpu().numpy()

def same(s, want, where):
    p, o = torch.from_dlpack(s.pattern), torch.from_dlpack(s.offsets)
    assert p.dtype == torch.int64 and o.dtype == torch.int64 and p.is_contiguous() and o.is_contiguous(), where
    assert p.device.type == "cuda" and o.device.type == "cuda" and s.device == 0 and len(s) == len(want[0]), where
    assert torch.equal(p.cpu(), torch.from_numpy(want[0])) and torch.equal(o.cpu(), torch.from_numpy(want[1])), where

for k, kind in enumerate(KINDS):
    b = ar.BytesAhoCorasick(MIXED, matchkind=getattr(ar.MatchKind, PY_KINDS[k]))
    # one haystack: no rows
    s = b.segment(t)
    want = definition(MIXED, data, kind)
    same(s, want, ("one", k))
    assert s.row_offsets is None and s.tolist() == triples(want)
    # split_rows' offsets, a tensor of offsets, a row length
    want = definition(MIXED, data, kind, offsets=off_np)
    for o, where in ((ro.offsets, "split_rows"), (off, "tensor")):
        s = b.segment_batch(t, offsets=o)
        same(s, want, (where, k))
        assert torch.equal(torch.from_dlpack(s.row_offsets).cpu(), torch.from_numpy(want[2])), where
    assert s.tolist() == triples(want, off_np)
    n = len(data) // 64 * 64
    s = b.segment_batch(t[:n], row_length=64)
    same(s, definition(MIXED, data[:n], kind, offsets=np.arange(0, n + 1, 64)), ("row_length", k))
    # host tensors take the host route
    s = b.segment_batch(t.cpu(), offsets=off.cpu())
    assert s.device is None and s.tolist() == triples(want, off_np)

    # the chain: split_rows -> segment_batch -> label_tokens_batch, nothing leaves HBM; against the host composition
    s = b.segment_batch(t, offsets=ro.offsets)
    tok = torch.from_dlpack(s.offsets)
    labels = b.label_tokens_batch(t, tok, offsets=ro.offsets)
    assert labels.device == 0 and len(labels) == len(s)
    host = b.label_tokens_batch(t.cpu(), torch.from_numpy(want[1]), offsets=off.cpu())
    assert labels.tolist() == host.tolist()
    f = b.filter_batch(t, offsets=ro.offsets)  # ... and the rows' filter takes the same offsets
    assert f.device == 0

# utf8 on a tensor, a case-insensitive handle leaves the tensor as it is
u = ("aä€\U0001f600bc " * 700).encode()
ut = torch.from_numpy(np.frombuffer(u, dtype=np.uint8).copy()).to(dev)
b = ar.BytesAhoCorasick(["ä".encode(), b"bc"], matchkind=ar.MatchKind.LeftmostLongest)
same(b.segment(ut, utf8=True), definition(["ä".encode(), b"bc"], u, KINDS[2], utf8=True), "utf8")
same(b.segment(ut), definition(["ä".encode(), b"bc"], u, KINDS[2]), "bytes")
ci = ar.BytesAhoCorasick([b"GATTACA", b"Def"], ascii_case_insensitive=True)
same(ci.segment(t), definition([b"GATTACA", b"Def"], data, KINDS[0], fold=True), "fold")
assert torch.equal(t.cpu(), torch.from_numpy(np.frombuffer(data, dtype=np.uint8)))

# errors
def raises(exc, fn):
    try:
        fn()
    except exc:
        return
    raise AssertionError(f"{exc.__name__} not raised")

b = ar.BytesAhoCorasick(MIXED)
raises(TypeError, lambda: b.segment_batch(t))                                      # a tensor needs one of the two
raises(TypeError, lambda: b.segment_batch(t, offsets=off, row_length=8))
raises(TypeError, lambda: b.segment_batch(t, offsets=off.to(torch.int32)))
raises(ValueError, lambda: b.segment_batch(t, offsets=off.cpu()))                  # on another device
raises(ValueError, lambda: b.segment_batch(t, offsets=off[:-1]))                   # they do not end at len
raises(ValueError, lambda: b.segment_batch(t, row_length=len(data) + 1))
raises(TypeError, lambda: b.segment(t, utf8=1))
raises(TypeError, lambda: b.segment(t.reshape(2, -1) if len(data) % 2 == 0 else t[:-1].reshape(2, -1)))

# empty inputs
e = b.segment(torch.zeros(0, dtype=torch.uint8, device=dev))
assert len(e) == 0 and e.tolist() == [] and torch.from_dlpack(e.offsets).tolist() == [0]
e = b.segment_batch(torch.zeros(0, dtype=torch.uint8, device=dev), offsets=torch.zeros(3, dtype=torch.int64, device=dev))
assert e.tolist() == [[], []] and torch.from_dlpack(e.row_offsets).tolist() == [0, 0, 0]

# lifetime: the columns outlive the result, the inputs and the automaton; the inputs stay alive while kernels read them
want = definition(MIXED, data, KINDS[0], offsets=off_np)
s = b.segment_batch(t, offsets=ro.offsets)
p, o = torch.from_dlpack(s.pattern), torch.from_dlpack(s.offsets)
del s, b, t, ro, off
gc.collect()
for k in range(8):
    other = torch.from_numpy(np.frombuffer(planted(len(data), 40 + k), dtype=np.uint8).copy()).to(dev)
torch.cuda.synchronize()
assert torch.equal(p.cpu(), torch.from_numpy(want[0])) and torch.equal(o.cpu(), torch.from_numpy(want[1]))
print("OK")
"""


def test_tensors_in_and_torch_out():
    """segment and segment_batch on tensors in HBM with split_rows' offsets, a tensor of offsets, row_length and neither, all
    kinds; torch.from_dlpack of the columns on the automaton's device; the chain split_rows -> segment_batch ->
    label_tokens_batch against the host composition; utf8; a case-insensitive handle leaves the tensor as it is; errors;
    empty inputs; lifetime.  In a process of its own: torch has to be the first to load the HIP runtime."""
    pytest.importorskip("torch")
    p = subprocess.run([sys.executable, "-c", _TENSOR_SCRIPT, ROOT, os.path.join(ROOT, "tests")], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
