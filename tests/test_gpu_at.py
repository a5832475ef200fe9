"""The anchored search on the device (acx_match_at / acx_match_at_device / acx_match_at_into_device; match_at /
match_prefix_batch): the raw form at the seams of its kernel -- anchor counts around the wave, the workgroup and the tile,
positions unsorted, repeated, at the ends of the data and of rows, inside runs of empty rows, outside the data; patterns that end
at a row's end and one byte past it; pattern lengths on both sides of the first-byte test; tiles in which every anchor, none and
one lane per wave survives it; a 256-child node; every alignment of the data and both of the columns; the three row cuts -- with
guard bytes around both columns and every input verified unwritten; the kinds and flags through the C ABI for host and device
inputs, against the definition and against acx_match_at_host; the Python methods with str (characters), bytes, sequences and
tensors in HBM, torch as the consumer, lifetime and a seeded random loop.  Expected values come from the definition restated
below -- every pattern against every anchor with startswith, no trie; for LeftmostFirst also re.match of the alternation --
never from the library; the kernel's seams are read from its header."""
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
OV, FULL, ROWS = capi.AT_OVERLAPPING, capi.AT_FULL, capi.AT_ROW_STARTS
GUARD = 0xC3


def hip_constants(path, names):
    src = open(os.path.join(CSRC, path)).read()
    out = {}
    for n in names:
        m = re.search(r"\b%s\s*=\s*(\d+)\s*[,;]" % n, src)
        assert m, f"{n} is no longer a plain constant of {path}"
        out[n] = int(m.group(1))
    return out


_C = hip_constants("at.hpp", ("AT_THREADS", "AT_TILE", "AT_PROBE"))
THREADS, TILE, PROBE = _C["AT_THREADS"], _C["AT_TILE"], _C["AT_PROBE"]


def test_constants_are_what_the_sizes_below_assume():
    assert TILE % THREADS == 0 and THREADS % 64 == 0 and TILE >= 2 * THREADS and 2 <= PROBE < 256


# ---------------------------------------------------------------------------
# the definition, restated: every pattern against every anchor
# ---------------------------------------------------------------------------
def anchors_of(length, positions, offsets):
    """(p, L) per anchor.  positions None: the rows.  Else the row of p is the LAST row that begins at or before p and L is
    where the next one begins; a position outside [0, length) has no candidate: (0, 0)."""
    off = np.asarray([0, length] if offsets is None else offsets, dtype=np.int64)
    if positions is None:
        return [(int(off[r]), int(off[r + 1])) for r in range(len(off) - 1)]
    out = []
    for p in positions:
        p = int(p)
        if not 0 <= p < length:
            out.append((0, 0))
            continue
        r = int(np.searchsorted(off, p, side="right")) - 1
        out.append((p, int(off[r + 1])))
    return out


def definition(patterns, hay, anchors, kind, *, overlapping=False, full=False, fold=False, local=False):
    """C(p, L) = {(i, e): e = p + len(P_i), e <= L, h[p:e] == P_i}; full keeps e == L only.  Standard: smallest e, then
    smallest i; LeftmostFirst: smallest i; LeftmostLongest: largest e, then smallest i; overlapping: all of C by (e, i)."""
    h = bytes(hay).lower() if fold else bytes(hay)
    P = [bytes(x).lower() if fold else bytes(x) for x in patterns]
    rx = re.compile(b"|".join(re.escape(x) for x in P)) if kind == LF and not overlapping and not full else None
    pat, end, ro = [], [], [0]
    for p, L in anchors:
        C = [(i, p + len(x)) for i, x in enumerate(P) if p < L and h.startswith(x, p, L)]
        if full:
            C = [c for c in C if c[1] == L]
        if overlapping:
            C.sort(key=lambda c: (c[1], c[0]))
        elif C:
            key = {STD: lambda c: (c[1], c[0]), LF: lambda c: c[0], LL: lambda c: (-c[1], c[0])}[kind]
            C = [min(C, key=key)]
            if rx:  # re.match of the alternation says the same
                m = rx.match(h, p, L)
                assert m and m.end() == C[0][1] and P[C[0][0]] == m.group(0)
        else:
            assert not rx or p >= L or rx.match(h, p, L) is None
            C = [(-1, -1)]
        pat += [c[0] for c in C]
        end += [c[1] - (p if local and c[0] >= 0 else 0) for c in C]
        ro.append(len(pat))
    return (np.asarray(pat, dtype=np.int64).reshape(-1), np.asarray(end, dtype=np.int64).reshape(-1),
            np.asarray(ro, dtype=np.int64))


def host_walk(patterns, hay, positions, offsets, kind, flags, fold=False):
    """acx_match_at_host over the same tables (positions inside the data only: it refuses the others)"""
    h = capi.HostAutomaton(patterns, kind, capi.BUILD_ASCII_CASE_INSENSITIVE if fold else 0)
    try:
        return capi.match_at_host(h, hay, positions, offsets=offsets, flags=flags, match_kind=kind)
    finally:
        h.close()


# ---------------------------------------------------------------------------
# the raw form: acx_match_at_into_device with guards
# ---------------------------------------------------------------------------
def run_raw(a, hay, positions, *, offsets=None, uniform=0, flags=0, base_res=0, out_res=0):
    """hay at base_res modulo 16; positions (None: ROW_STARTS); the columns at 8 * out_res modulo 16, each between 64 guard
    bytes -> (pattern, end); the guards and every input checked unwritten"""
    hay = np.frombuffer(bytes(hay), dtype=np.uint8)
    n = len(hay)
    rows = (len(offsets) - 1) if offsets is not None else (n // uniform if uniform else 1)
    A = rows if positions is None else len(positions)
    img_h = np.full(n + 48, GUARD, dtype=np.uint8)
    img_h[base_res:base_res + n] = hay
    d_hay = capi.DeviceBuffer(len(img_h)).upload(img_h)
    assert d_hay.ptr % 16 == 0
    lead = 64 + 8 * out_res
    img = np.full(lead + 8 * A + 64, GUARD, dtype=np.uint8)
    d_pat, d_end = capi.DeviceBuffer(len(img) + 16).upload(img), capi.DeviceBuffer(len(img) + 16).upload(img)
    assert d_pat.ptr % 16 == 0 and d_end.ptr % 16 == 0
    d_pos = d_off = None
    if positions is not None:
        pos = np.ascontiguousarray(np.asarray(positions, dtype=np.int64))
        d_pos = capi.DeviceBuffer(8 * len(pos) + 16)
        if len(pos):
            d_pos.upload(pos)
    if offsets is not None:
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64))
        d_off = capi.DeviceBuffer(8 * len(off)).upload(off)
    try:
        a.match_at_into_device(d_hay.ptr + base_res, n, d_pos.ptr if d_pos else 0, 0 if positions is None else len(positions),
                               d_pat.ptr + lead, d_end.ptr + lead, flags | (ROWS if positions is None else 0),
                               d_offsets=d_off.ptr if d_off else 0, n_hay=rows if (d_off or uniform) else 0, uniform_len=uniform)
        got_p, got_e = d_pat.download(len(img)), d_end.download(len(img))
        assert np.array_equal(d_hay.download(len(img_h)), img_h), "the data (or a byte around it) was written"
        if d_pos and len(pos):
            assert np.array_equal(d_pos.download(8 * len(pos)).view(np.int64), pos), "the positions were written"
        if d_off:
            assert np.array_equal(d_off.download(8 * len(off)).view(np.uint64), off), "the offsets were written"
    finally:
        for b in (d_hay, d_pat, d_end, d_pos, d_off):
            if b:
                b.free()
    for got, name in ((got_p, "pattern"), (got_e, "end")):
        assert (got[:lead] == GUARD).all(), ("a byte before the column was written", name)
        assert (got[lead + 8 * A:] == GUARD).all(), ("a byte behind the column was written", name)
    return got_p[lead:lead + 8 * A].copy().view(np.int64), got_e[lead:lead + 8 * A].copy().view(np.int64)


def check_raw(patterns, kind, hay, positions, *, offsets=None, uniform=0, full=False, fold=False, what=None, automaton=None, **kw):
    a = automaton or capi.Automaton(patterns, kind, ascii_case_insensitive=fold)
    try:
        got = run_raw(a, hay, positions, offsets=offsets, uniform=uniform, flags=FULL if full else 0, **kw)
    finally:
        if not automaton:
            a.close()
    cut = offsets if offsets is not None else (np.arange(0, len(hay) + 1, uniform) if uniform else None)
    want = definition(patterns, hay, anchors_of(len(hay), positions, cut), kind, full=full, fold=fold, local=positions is None)
    for g, w, name in zip(got, want, ("pattern", "end")):
        bad = np.flatnonzero(g != w)
        assert not len(bad), (what, name, int(bad[0]), g[bad[:8]], w[bad[:8]])
    return got


LONG = b"gattacagattacagattacagattacagattacagatta"  # 40 bytes: the longest pattern
MIXED = [b"a", b"bc", b"def", LONG, b"ab", b"abc", b"bcd", LONG[:7], b"de", b"g"]


def planted(n, seed, patterns=MIXED, alphabet=b"abcdefgxyz", every=9):
    rng = np.random.default_rng(seed)
    hay = bytearray(bytes(rng.choice(list(alphabet), size=n)))
    for k in range(0, max(n - 48, 0), every):
        p = patterns[int(rng.integers(0, len(patterns)))]
        hay[k:k + len(p)] = p
    return bytes(hay[:n])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("A", [0, 1, 63, 64, 65, THREADS - 1, THREADS + 1, TILE - 1, TILE + 1, 2 * TILE + 1])
def test_raw_anchor_counts_around_the_wave_the_workgroup_and_the_tile(kind, A):
    hay = planted(3000, A)
    rng = np.random.default_rng(A + 1)
    pos = rng.integers(0, len(hay) + 1, size=A)  # unsorted, repeated
    if A >= 63:
        pos[:8] = [len(hay) - 1, len(hay), -1, len(hay) + 1, -(1 << 62), (1 << 62), 0, 0]
        pos[-1] = pos[-2]
    check_raw(MIXED, kind, hay, pos, what=A)


@pytest.mark.parametrize("kind", KINDS)
def test_raw_positions_at_the_ends_of_rows_and_in_runs_of_empty_rows(kind):
    #        row 0      1 (a pattern ends exactly at its end)   2, 3, 4 empty   5 ("def" one byte past its end)   6
    rows = [b"xabcx", b"zzdef", b"", b"", b"", b"ade", b"f" + LONG + b"bc"]
    lens = [len(r) for r in rows]
    off = np.concatenate([[0], np.cumsum(lens)])
    hay = b"".join(rows)
    pos = list(range(len(hay) + 1)) + [int(off[1]) - 1, int(off[1]), int(off[2]), int(off[2]), int(off[5]), int(off[6]) - 2, -5, len(hay) + 3]
    pat, end = check_raw(MIXED, kind, hay, pos, offsets=off)
    at = int(off[1]) + 2  # "def" ends exactly at the row's end ("de" one byte before it)
    assert (pat[at], end[at]) == {STD: (8, off[2] - 1), LF: (2, off[2]), LL: (2, off[2])}[kind]
    at = int(off[5]) + 1  # "de" fits, "def" would end one byte past the row's end
    assert (pat[at], end[at]) == (8, off[6])
    check_raw(MIXED, kind, hay, None, offsets=off)                               # the rows themselves: empty ones give (-1, -1)
    check_raw(MIXED, kind, hay, None, offsets=off, full=True)
    check_raw(MIXED, kind, hay, pos[::-1], offsets=off, out_res=1)


@pytest.mark.parametrize("kind", KINDS)
def test_raw_survivors_all_none_and_one_lane_per_wave(kind):
    n = 2 * TILE + 70
    pos = np.arange(n)
    check_raw(MIXED, kind, b"a" * n, pos, what="every anchor survives the first byte")
    check_raw(MIXED, kind, b"ab" * (n // 2), pos, what="every anchor survives, half of them walk on")
    check_raw(MIXED, kind, b"z" * n, pos, what="no anchor survives")
    one = bytearray(b"z" * n)
    for w in range(0, n - 128, 64):  # exactly one lane of each wave: another lane in every wave
        k = w + (w // 64 * 7) % 64
        one[k:k + 3] = b"def"
    pat, end = check_raw(MIXED, kind, bytes(one), pos, what="one lane of each wave survives")
    assert (pat >= 0).sum() >= n // 64 - 2
    walk = bytearray(b"z" * n)  # one lane of each wave walks 40 levels
    for w in range(0, n - 128, 64):
        walk[w + 11:w + 11 + len(LONG)] = LONG
    check_raw(MIXED, kind, bytes(walk), pos, what="one long walk per wave")


@pytest.mark.parametrize("kind", KINDS)
def test_raw_a_256_child_node_at_its_first_a_middle_and_its_last_child(kind):
    fan = [b"q" + bytes([b]) + b"!" for b in range(256)] + [bytes([b]) + b"x" for b in range(256)] + [b"q"]
    hay = b"q\x00!q\x7f!q\xff!q\x80?\x00x\x7fx\xffxq\x01"
    check_raw(fan, kind, hay, list(range(len(hay) + 1)))
    few = [b"k" + bytes([b]) for b in range(0, 2 * (PROBE + 1), 2)]  # PROBE + 1 children: the search; PROBE: the probe
    for pats in (few, few[:-1]):
        hay = b"".join(b"k" + bytes([b]) for b in range(0, 2 * PROBE + 4))
        check_raw(pats, kind, hay, list(range(len(hay) + 1)))


@pytest.mark.parametrize("base_res", range(16))
def test_raw_every_alignment_of_the_data_and_both_of_the_columns(base_res):
    hay = planted(700, base_res)
    pos = np.random.default_rng(base_res).integers(0, len(hay) + 1, size=THREADS + 3)
    for out_res in (0, 1):
        check_raw(MIXED, LL, hay, pos, base_res=base_res, out_res=out_res)
    check_raw(MIXED, STD, hay, None, uniform=7, base_res=base_res, out_res=base_res & 1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form", ["offsets", "uniform", "one"])
def test_raw_the_three_row_cuts(kind, form):
    U = 13
    hay = planted(U * 230, 3, every=5)
    pos = np.random.default_rng(7).integers(0, len(hay) + 1, size=TILE + 9)
    if form == "offsets":
        rng = np.random.default_rng(11)
        cuts = np.sort(rng.integers(0, len(hay) + 1, size=300))
        cuts[10:14] = cuts[10]  # a run of empty rows
        off = np.concatenate([[0], cuts, [len(hay)]])
        check_raw(MIXED, kind, hay, pos, offsets=off)
        check_raw(MIXED, kind, hay, None, offsets=off)
        check_raw(MIXED, kind, hay, None, offsets=off, full=True)
    elif form == "uniform":
        check_raw(MIXED, kind, hay, pos, uniform=U)
        check_raw(MIXED, kind, hay, None, uniform=U)
        check_raw([b"a", hay[U:2 * U], hay[:U][:5]], kind, hay, None, uniform=U, full=True)
    else:
        check_raw(MIXED, kind, hay, pos)
        check_raw(MIXED, kind, hay, None)
        check_raw([hay, b"a"], kind, hay, None, full=True)


def test_raw_refusals_and_nothing_to_write():
    a = capi.Automaton(MIXED, STD)
    buf = capi.DeviceBuffer(256)
    try:
        def code(fn):
            with pytest.raises(ValueError) as e:
                fn()
            return e.value.code

        p = buf.ptr
        assert code(lambda: a.match_at_into_device(p, 16, p + 64, 1, p + 128, p + 192, OV)) == capi.EINVAL
        assert code(lambda: a.match_at_into_device(p, 16, p + 64, 1, p + 128, p + 192, FULL)) == capi.EINVAL
        assert code(lambda: a.match_at_into_device(p, 16, p + 64, 1, p + 128, p + 192, 8)) == capi.EINVAL
        assert code(lambda: a.match_at_into_device(p, 16, p + 65, 1, p + 128, p + 192)) == capi.EINVAL   # alignment
        assert code(lambda: a.match_at_into_device(p, 16, p + 64, 1, p + 132, p + 192)) == capi.EINVAL
        assert code(lambda: a.match_at_into_device(p, 16, 0, 1, p + 128, p + 192)) == capi.EINVAL        # null positions
        assert code(lambda: a.match_at_into_device(p, 16, p + 64, 1, 0, p + 192)) == capi.EINVAL
        assert code(lambda: a.match_at_into_device(0, 16, p + 64, 1, p + 128, p + 192)) == capi.EINVAL
        assert code(lambda: a.match_at_into_device(p, 16, p + 64, 1, p + 128, p + 192, d_offsets=p, n_hay=1, uniform_len=16)) == capi.EINVAL
        assert code(lambda: a.match_at_into_device(p, 16, p + 64, 1, p + 128, p + 192, uniform_len=5, n_hay=3)) == capi.EINVAL
        assert code(lambda: a.match_at_into_device(p, 16, p + 64, 1 << 32, p + 128, p + 192)) == capi.ETOOBIG
        a.match_at_into_device(p, 16, 0, 0, 0, 0)  # no anchor: nothing to write
    finally:
        buf.free()
        a.close()


# ---------------------------------------------------------------------------
# kinds and flags through the C ABI, host and device inputs
# ---------------------------------------------------------------------------
def device_call(a, hay, positions, flags, offsets=None, uniform=0):
    hay = np.frombuffer(bytes(hay), dtype=np.uint8)
    d_hay = capi.DeviceBuffer(len(hay) + 16)
    if len(hay):
        d_hay.upload(hay)
    d_pos = d_off = None
    if positions is not None:
        pos = np.ascontiguousarray(np.asarray(positions, dtype=np.int64))
        d_pos = capi.DeviceBuffer(8 * len(pos) + 16)
        if len(pos):
            d_pos.upload(pos)
    rows = 0
    if offsets is not None:
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64))
        d_off = capi.DeviceBuffer(8 * len(off)).upload(off)
        rows = len(off) - 1
    elif uniform:
        rows = len(hay) // uniform
    try:
        r = a.match_at_device(d_hay.ptr, len(hay), d_pos.ptr if d_pos else 0, 0 if positions is None else len(positions),
                              flags | (ROWS if positions is None else 0), d_offsets=d_off.ptr if d_off else 0, n_hay=rows,
                              uniform_len=uniform)
        try:
            assert r.on_device and r.pattern_ptr() and r.end_ptr()
            out = (r.pattern(), r.end(), r.row_offsets())
            assert r.count == (len(out[2]) - 1 if out[2] is not None else len(out[0])) and r.entries == len(out[0])
            assert (out[2] is not None) == bool(flags & OV) and bool(r.row_offsets_ptr()) == bool(flags & OV)
            assert np.array_equal(d_hay.download(len(hay)), hay), "the data was written"
        finally:
            r.free()
    finally:
        for b in (d_hay, d_pos, d_off):
            if b:
                b.free()
    return out


def host_call(a, hay, positions, flags, offsets=None):
    if offsets is None:
        r = a.match_at(None, positions, flags | (ROWS if positions is None else 0), single=bytes(hay))
    else:
        rows = [bytes(hay[int(offsets[i]):int(offsets[i + 1])]) for i in range(len(offsets) - 1)]
        r = a.match_at(rows, positions, flags | (ROWS if positions is None else 0))
    try:
        assert not r.on_device
        return r.pattern(), r.end(), r.row_offsets()
    finally:
        r.free()


def check_abi(patterns, kind, hay, positions, *, offsets=None, overlapping=False, full=False, fold=False, what=None, host=True):
    flags = (OV if overlapping else 0) | (FULL if full else 0)
    want = definition(patterns, hay, anchors_of(len(hay), positions, offsets), kind, overlapping=overlapping, full=full, fold=fold,
                      local=positions is None)
    inside = positions is None or all(0 <= int(p) <= len(hay) for p in positions)
    a = capi.Automaton(patterns, kind, ascii_case_insensitive=fold)
    try:
        legs = [("device", device_call(a, hay, positions, flags, offsets))]
        if host and inside:
            legs.append(("host", host_call(a, hay, positions, flags, offsets)))
    finally:
        a.close()
    if inside:
        w = host_walk(patterns, hay, positions, offsets, kind, flags | (ROWS if positions is None else 0), fold)
        legs.append(("acx_match_at_host", (w[0], w[1], w[2] if overlapping else None)))
    for leg, got in legs:
        for g, w, name in zip(got, want, ("pattern", "end", "row_offsets")):
            if name == "row_offsets" and not overlapping:
                assert g is None
                continue
            assert g is not None and len(g) == len(w), (what, leg, name, len(g), len(w))
            bad = np.flatnonzero(g != w)
            assert not len(bad), (what, leg, name, int(bad[0]), g[bad[:8]], w[bad[:8]])
    return legs[0][1]


@pytest.mark.parametrize("kind", KINDS)
def test_abi_three_kinds_host_and_device_inputs(kind):
    hay = planted(1500, 21, every=6)
    pos = np.random.default_rng(2).integers(0, len(hay) + 1, size=THREADS + 40)
    cuts = np.sort(np.random.default_rng(3).integers(0, len(hay) + 1, size=60))
    off = np.concatenate([[0], cuts, [len(hay)]])
    dup = MIXED + [b"a", b"abc", LONG]  # copies: the lowest index is reported
    check_abi(dup, kind, hay, pos, what="one haystack")
    check_abi(dup, kind, hay, pos, offsets=off, what="rows")
    check_abi(dup, kind, hay, None, offsets=off, what="row starts")
    check_abi(dup, kind, hay, None, offsets=off, full=True, what="full")
    check_abi(dup, kind, hay, list(pos[:50]) + [-1, len(hay) + 1], offsets=off, what="outside the data")
    check_abi(dup, kind, b"", [0, 0], what="no data")
    check_abi(dup, kind, hay, [], what="no anchors")


def test_abi_overlapping_counts_that_straddle_a_tile_boundary():
    pats = [b"a", b"aa", b"aaa", b"a", b"aaaa", b"aa", b"b"]
    n = TILE + 40
    hay = bytearray(b"a" * n)
    hay[TILE - 2] = ord("z")  # an anchor with zero entries between two with many, at the tile's edge
    hay[5] = ord("b")
    pat, end, ro = check_abi(pats, STD, bytes(hay), list(range(n + 1)), overlapping=True, what="overlapping")
    k = np.diff(ro)
    assert k[TILE - 2] == 0 and k[TILE - 3] == 2 and k[TILE - 1] == 6 and k[0] == 6 and k[n] == 0
    cuts = np.concatenate([[0], np.arange(3, n, 5), [n]])
    check_abi(pats, STD, bytes(hay), list(range(n + 1))[::-1], offsets=cuts, overlapping=True)
    check_abi(pats, STD, bytes(hay), None, offsets=cuts, overlapping=True)
    check_abi(pats, STD, bytes(hay), None, offsets=cuts, overlapping=True, full=True)
    check_abi(pats, STD, b"zzzz", [0, 1, 2], overlapping=True, what="no entry at all")
    check_abi(pats, STD, bytes(hay), [], overlapping=True, what="no anchors")


def test_abi_refusals():
    a, al = capi.Automaton(MIXED, STD), capi.Automaton(MIXED, LL)
    try:
        def code(fn):
            with pytest.raises(ValueError) as e:
                fn()
            return e.value.code

        assert code(lambda: al.match_at(None, [0], OV, single=b"abc")) == capi.EOVERLAP
        assert code(lambda: al.match_at_device(0, 0, 0, 0, OV)) == capi.EOVERLAP
        assert code(lambda: a.match_at(None, [0], FULL, single=b"abc")) == capi.EINVAL
        assert code(lambda: a.match_at(None, [4], 0, single=b"abc")) == capi.EINVAL
        assert code(lambda: a.match_at(None, [-1], 0, single=b"abc")) == capi.EINVAL
        assert code(lambda: a.match_at(None, [3], 0, True, single="aé".encode())) == capi.EINVAL  # two characters
        off = np.asarray([0, 2, 1, 3], dtype=np.uint64)
        hay = np.frombuffer(b"abc", dtype=np.uint8)
        out = capi.ctypes.c_void_p()
        one = np.zeros(1, dtype=np.int64)
        L = capi.lib()
        assert L.acx_match_at(a._h, hay.ctypes.data, 3, off.ctypes.data, 3, one.ctypes.data, 1, 0, 0, capi.ctypes.byref(out)) == capi.EINVAL
        assert L.acx_match_at(a._h, hay.ctypes.data, 3, None, 0, None, 1, 0, 0, capi.ctypes.byref(out)) == capi.EINVAL
        assert L.acx_match_at(None, hay.ctypes.data, 3, None, 0, one.ctypes.data, 1, 0, 0, capi.ctypes.byref(out)) == capi.EINVAL
        assert L.acx_match_at(a._h, hay.ctypes.data, 3, None, 0, one.ctypes.data, 1, 0, 0, None) == capi.EINVAL
        assert L.acx_at_copy(None, 0, one.ctypes.data) == capi.EINVAL and L.acx_at_count(None) == 0
        r = a.match_at(None, [0], 0, single=b"abc")
        assert L.acx_at_copy(r._h, 3, one.ctypes.data) == capi.EINVAL and L.acx_at_copy(r._h, 2, one.ctypes.data) == capi.EINVAL
        assert r.row_offsets() is None and r.count == 1 and r.entries == 1
        r.free()
    finally:
        a.close()
        al.close()


def test_abi_a_case_insensitive_handle_leaves_the_tensor_as_it_is():
    pats = [b"Http", b"HTTPS", b"ftp", b"h", b"\xc3\x84x"]
    hay = (b"hTTps://x HTTP FtP h \xc3\x84X \xc3\xa4x " * 40)
    for kind in KINDS:
        check_abi(pats, kind, hay, list(range(len(hay) + 1)), fold=True)  # (device_call asserts the data unchanged)
        check_abi(pats, kind, hay, None, offsets=np.concatenate([np.arange(0, len(hay), 31), [len(hay)]]), fold=True)
    check_abi(pats, STD, hay, list(range(0, len(hay), 3)), fold=True, overlapping=True)


@pytest.mark.parametrize("kind", KINDS)
def test_abi_a_handle_kept_in_compressed_form_only(kind, monkeypatch):
    monkeypatch.setenv("ACX_DENSE_LIMIT", "0")
    hay = planted(900, 5, every=6)
    a = capi.Automaton(MIXED, kind)
    try:
        assert a.info.table_bytes == 0, "the dense table was built after all"
    finally:
        a.close()
    check_abi(MIXED, kind, hay, list(range(len(hay) + 1)), what="compressed")
    check_abi(MIXED, kind, hay, None, offsets=np.arange(0, len(hay) + 1, 9), full=True, what="compressed, full")


# ---------------------------------------------------------------------------
# the Python methods
# ---------------------------------------------------------------------------
PY_KINDS = ("Standard", "LeftmostFirst", "LeftmostLongest")


def py_check(result, want, overlapping=False):
    pat, end, ro = want
    assert len(result) == len(ro) - 1
    p, e = np.from_dlpack(result.pattern), np.from_dlpack(result.end)
    assert p.dtype == np.int64 and e.dtype == np.int64 and np.array_equal(p, pat) and np.array_equal(e, end)
    pairs = list(zip(pat.tolist(), end.tolist()))
    if overlapping:
        assert np.array_equal(np.from_dlpack(result.row_offsets), ro)
        assert result.tolist() == [pairs[ro[k]:ro[k + 1]] for k in range(len(ro) - 1)]
    else:
        assert result.row_offsets is None and result.tolist() == pairs
    assert result.device is None


def test_python_bytes_sequences_and_full_as_a_dictionary_lookup():
    import ahocorasick_rs as ar
    hay = planted(600, 9, every=5)
    pos = [int(x) for x in np.random.default_rng(1).integers(0, len(hay) + 1, size=150)]
    rows = [b"abc", b"", b"defx", LONG, LONG[:7] + b"!", b"zz", b"a"]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    for k, name in zip(KINDS, PY_KINDS):
        b = ar.BytesAhoCorasick(MIXED, matchkind=getattr(ar.MatchKind, name))
        py_check(b.match_at(hay, pos), definition(MIXED, hay, anchors_of(len(hay), pos, None), k))
        py_check(b.match_at(memoryview(hay), np.asarray(pos, dtype=np.int64)), definition(MIXED, hay, anchors_of(len(hay), pos, None), k))
        py_check(b.match_prefix_batch(rows), definition(MIXED, b"".join(rows), anchors_of(0, None, off), k, local=True))
        py_check(b.match_prefix_batch(rows, full=True), definition(MIXED, b"".join(rows), anchors_of(0, None, off), k, full=True, local=True))
        # a dictionary lookup: every pattern goes to its own lowest index
        words = MIXED + [b"a", LONG]
        d = ar.BytesAhoCorasick(words, matchkind=getattr(ar.MatchKind, name))
        got = d.match_prefix_batch(words + [b"nope", b"ax", b""], full=True).tolist()
        assert got == [(words.index(w), len(w)) for w in words] + [(-1, -1)] * 3
        assert d.match_prefix_batch([]).tolist() == [] and len(d.match_at(b"abc", [])) == 0
    b = ar.BytesAhoCorasick(MIXED)
    py_check(b.match_at(hay, pos, True), definition(MIXED, hay, anchors_of(len(hay), pos, None), STD, overlapping=True), True)
    py_check(b.match_at(hay, pos, overlapping=True), definition(MIXED, hay, anchors_of(len(hay), pos, None), STD, overlapping=True), True)
    py_check(b.match_prefix_batch(rows, True), definition(MIXED, b"".join(rows), anchors_of(0, None, off), STD, overlapping=True, local=True), True)


def test_python_str_in_characters_with_multi_byte_text():
    import ahocorasick_rs as ar
    pats = ["é", "éa", "日本", "日", "a", "本語x", "😀b"]
    hay = "éa日本語x a😀b日é"
    for k, name in zip(KINDS, PY_KINDS):
        s = ar.AhoCorasick(pats, matchkind=getattr(ar.MatchKind, name))
        got = s.match_at(hay, list(range(len(hay) + 1))).tolist()
        want = []
        for p in range(len(hay) + 1):
            C = [(i, p + len(x)) for i, x in enumerate(pats) if hay.startswith(x, p)]
            key = {STD: lambda c: (c[1], c[0]), LF: lambda c: c[0], LL: lambda c: (-c[1], c[0])}[k]
            want.append(min(C, key=key) if C else (-1, -1))
        assert got == want, name
        rows = ["éa", "日本語x!", "", "x", "😀b", "a"]
        got = s.match_prefix_batch(rows).tolist()
        assert [g[0] for g in got] == [{STD: 0, LF: 0, LL: 1}[k], {STD: 3, LF: 2, LL: 2}[k], -1, -1, 6, 4]
        assert [g[1] for g in got] == [{STD: 1, LF: 1, LL: 2}[k], {STD: 1, LF: 2, LL: 2}[k], -1, -1, 2, 1]  # characters
        assert s.match_prefix_batch(rows, full=True).tolist() == [(1, 2), (-1, -1), (-1, -1), (-1, -1), (6, 2), (4, 1)]
        assert s.match_at("plain ascii a", [12, 0]).tolist() == [(4, 13), (-1, -1)]
    s = ar.AhoCorasick(pats)
    assert s.match_at(hay, [0, 2], overlapping=True).tolist() == [[(0, 1), (1, 2)], [(3, 3), (2, 4)]]
    with pytest.raises(ValueError):
        s.match_at(hay, [len(hay) + 1])  # characters, not bytes: len(hay.encode()) would be inside


def test_python_errors():
    import ahocorasick_rs as ar
    b, bl, s = ar.BytesAhoCorasick(MIXED), ar.BytesAhoCorasick(MIXED, matchkind=ar.MatchKind.LeftmostFirst), ar.AhoCorasick(["a"])
    for bad in ([True], [1.5], ["1"], "12", 5, None):
        with pytest.raises(TypeError):
            b.match_at(b"abc", bad)
    for bad in ([-1], [4], [1 << 70], [-(1 << 70)]):
        with pytest.raises(ValueError):
            b.match_at(b"abc", bad)
    with pytest.raises(TypeError):
        b.match_at(b"abc", np.asarray([0], dtype=np.int32))
    with pytest.raises(TypeError):
        b.match_at(b"abc", [0], 1)          # overlapping is a real bool
    with pytest.raises(TypeError):
        b.match_prefix_batch([b"abc"], full=1)  # ... and so is full
    with pytest.raises(TypeError):
        b.match_prefix_batch([b"abc"], False, True)  # full is keyword-only
    with pytest.raises(TypeError):
        b.match_at(b"abc", [0], offsets=[0, 3])  # offsets go with a tensor
    with pytest.raises(TypeError):
        b.match_at(b"abc", [0], row_length=3)
    with pytest.raises(TypeError):
        s.match_at("abc", [0], row_length=3)
    with pytest.raises(TypeError):
        b.match_prefix_batch([b"abc"], row_length=3)
    with pytest.raises(TypeError):
        s.match_at(b"abc", [0])
    with pytest.raises(TypeError):
        b.match_at("abc", [0])
    with pytest.raises(ValueError):
        bl.match_at(b"abc", [0], overlapping=True)
    with pytest.raises(ValueError):
        bl.match_prefix_batch([b"abc"], overlapping=True)
    with pytest.raises(TypeError):
        ar.MatchesAt()


def test_python_host_columns_outlive_the_result_and_the_automaton():
    import ahocorasick_rs as ar
    hay = planted(400, 4, every=5)
    pos = list(range(len(hay) + 1))
    want = definition(MIXED, hay, anchors_of(len(hay), pos, None), STD)
    b = ar.BytesAhoCorasick(MIXED)
    r = b.match_at(hay, pos)
    pat, end = np.from_dlpack(r.pattern), np.from_dlpack(r.end)
    del r, b, pos
    gc.collect()
    other = ar.BytesAhoCorasick(MIXED)
    for k in range(20):  # (other results come and go where the columns would be if they had been freed)
        other.match_at(planted(400, 50 + k), list(range(300)))
    assert np.array_equal(pat, want[0]) and np.array_equal(end, want[1])


def test_python_seeded_random_cases():
    import ahocorasick_rs as ar
    rng = np.random.default_rng(2024)
    for case in range(200):
        alphabet = b"ab" if case % 3 else b"abcA"
        n = int(rng.integers(1, 9))
        patterns = [bytes(rng.choice(list(alphabet), size=int(rng.integers(1, 6)))) for _ in range(n)]
        hay = bytes(rng.choice(list(alphabet), size=int(rng.integers(0, 40))))
        pos = [int(x) for x in rng.integers(0, len(hay) + 1, size=int(rng.integers(0, 20)))]
        cuts = sorted(int(x) for x in rng.integers(0, len(hay) + 1, size=int(rng.integers(0, 6))))
        off = [0] + cuts + [len(hay)]
        rows = [hay[off[i]:off[i + 1]] for i in range(len(off) - 1)]
        k = case % 3
        fold = case % 5 == 0
        ov = k == 0 and case % 2 == 0
        full = case % 4 == 1
        b = ar.BytesAhoCorasick(patterns, matchkind=getattr(ar.MatchKind, PY_KINDS[k]), ascii_case_insensitive=fold)
        py_check(b.match_at(hay, pos, ov), definition(patterns, hay, anchors_of(len(hay), pos, None), KINDS[k], overlapping=ov, fold=fold), ov)
        py_check(b.match_prefix_batch(rows, ov, full=full),
                 definition(patterns, hay, anchors_of(len(hay), None, off), KINDS[k], overlapping=ov, full=full, fold=fold, local=True), ov)
        if case % 10 == 0:  # ... and the same through the C ABI on device inputs, rows included
            check_abi(patterns, KINDS[k], hay, pos, offsets=off, overlapping=ov, fold=fold, what=case, host=False)


_TENSOR_SCRIPT = r"""
import gc
import sys
import torch  # first: one process holds ONE HIP runtime, and torch must be the one to load it
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
import ahocorasick_rs as ar
from test_gpu_at import MIXED, LONG, KINDS, PY_KINDS, STD, anchors_of, definition, planted

dev = "cuda:0"
lines = [b"abc def", b"", b"gattaca", LONG, b"def", b"", b"", b"bcd!", b"xa"] * 20
data = b"\n".join(lines) + b"\n"
t = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev)
ro = ar.split_rows(t)
off = torch.from_dlpack(ro.offsets)
cuts = off.cpu().numpy()
pos_np = np.random.default_rng(3).integers(0, len(data) + 1, size=800).astype(np.int64)
pos = torch.from_numpy(pos_np).to(dev)

def same(r, want, ov, where):
    p, e = torch.from_dlpack(r.pattern), torch.from_dlpack(r.end)
    assert p.dtype == torch.int64 and e.dtype == torch.int64 and p.is_contiguous() and len(r) == len(want[2]) - 1, where
    if where != "host":
        assert r.device == 0 and p.device.type == "cuda" and e.device.type == "cuda", where
    assert torch.equal(p.cpu(), torch.from_numpy(want[0])) and torch.equal(e.cpu(), torch.from_numpy(want[1])), where
    if ov:
        assert torch.equal(torch.from_dlpack(r.row_offsets).cpu(), torch.from_numpy(want[2])), where
    else:
        assert r.row_offsets is None

for k, name in zip(KINDS, PY_KINDS):
    b = ar.BytesAhoCorasick(MIXED, matchkind=getattr(ar.MatchKind, name))
    for ov in ((False, True) if k == STD else (False,)):
        w_rows = definition(MIXED, data, anchors_of(len(data), pos_np, cuts), k, overlapping=ov)
        w_one = definition(MIXED, data, anchors_of(len(data), pos_np, None), k, overlapping=ov)
        w_uni = definition(MIXED, data, anchors_of(len(data), pos_np, np.arange(0, len(data) + 1, 10)), k, overlapping=ov)
        assert len(data) % 10 == 0
        same(b.match_at(t, pos, ov, offsets=ro.offsets), w_rows, ov, "split_rows offsets")
        same(b.match_at(t, pos, ov, offsets=off), w_rows, ov, "tensor offsets")
        same(b.match_at(t, pos, ov), w_one, ov, "one row")
        same(b.match_at(t, pos, ov, row_length=10), w_uni, ov, "row_length")
        same(b.match_at(t.cpu(), pos.cpu(), ov, offsets=off.cpu()), w_rows, ov, "host")
        w_pre = definition(MIXED, data, anchors_of(len(data), None, cuts), k, overlapping=ov, local=True)
        same(b.match_prefix_batch(t, ov, offsets=ro.offsets), w_pre, ov, "prefix")
        same(b.match_prefix_batch(t.cpu(), ov, offsets=off.cpu()), w_pre, ov, "host")
        w_pre = definition(MIXED, data, anchors_of(len(data), None, np.arange(0, len(data) + 1, 10)), k, overlapping=ov, full=True, local=True)
        same(b.match_prefix_batch(t, ov, full=True, row_length=10), w_pre, ov, "prefix, full, row_length")
    # the old way gives the same answer: an overlapping find, then a filter on the starts
    if k == STD:
        mc = b.find_matches_as_columns(t, overlapping=True)
        pt, st, en = (torch.from_dlpack(c) for c in (mc.pattern, mc.start, mc.end))
        keep = torch.isin(st, pos)
        r = b.match_at(t, torch.unique(pos), True)
        assert int(keep.sum()) == len(torch.from_dlpack(r.pattern))

# a case-insensitive handle folds in its loads: the tensor is as it was
ci = ar.BytesAhoCorasick([b"Needle", b"a n"], ascii_case_insensitive=True)
ct_np = np.frombuffer(b"A nEEdle, a Needle. " * 50, dtype=np.uint8).copy()
ct = torch.from_numpy(ct_np).to(dev)
got = ci.match_prefix_batch(ct, row_length=20).tolist()
assert got == [(1, 3)] * 50, got[:3]
got = ci.match_at(ct, torch.arange(2, 1000, 20, dtype=torch.int64, device=dev)).tolist()
assert got == [(0, 8 + 20 * i) for i in range(50)], got[:3]
assert torch.equal(ct.cpu(), torch.from_numpy(ct_np))

# positions outside the data are the caller's word: (-1, -1)
b = ar.BytesAhoCorasick(MIXED)
wild = torch.tensor([-1, len(data), len(data) + 5, -(1 << 62), 1 << 62, 0], dtype=torch.int64, device=dev)
assert b.match_at(t, wild, offsets=off).tolist()[:5] == [(-1, -1)] * 5
assert b.match_at(t, wild, True, offsets=off).tolist()[:5] == [[]] * 5

def raises(exc, fn):
    try:
        fn()
    except exc:
        return
    raise AssertionError(f"{exc.__name__} expected")

raises(TypeError, lambda: b.match_at(t, pos.to(torch.int32)))
raises(TypeError, lambda: b.match_at(t, pos_np.tolist()))            # a tensor haystack takes a tensor of positions
raises(ValueError, lambda: b.match_at(t, pos.cpu()))                  # positions on another device
raises(ValueError, lambda: b.match_at(t, pos, offsets=off.cpu()))
raises(ValueError, lambda: b.match_at(t, pos, offsets=off[:-1]))      # offsets that do not span the tensor
raises(TypeError, lambda: b.match_at(t, pos, offsets=off, row_length=10))
raises(ValueError, lambda: b.match_at(t, pos, row_length=7))
raises(ValueError, lambda: b.match_at(t.cpu(), torch.tensor([len(data) + 1]), offsets=off.cpu()))  # host positions are checked
raises(TypeError, lambda: b.match_prefix_batch(t))
raises(ValueError, lambda: ar.BytesAhoCorasick(MIXED, matchkind=ar.MatchKind.LeftmostLongest).match_at(t, pos, True))

# empty inputs
e = b.match_at(t, torch.zeros(0, dtype=torch.int64, device=dev))
assert len(e) == 0 and e.tolist() == [] and tuple(torch.from_dlpack(e.pattern).shape) == (0,)
e = b.match_at(torch.zeros(0, dtype=torch.uint8, device=dev), torch.zeros(3, dtype=torch.int64, device=dev), True)
assert e.tolist() == [[], [], []] and torch.from_dlpack(e.row_offsets).tolist() == [0, 0, 0, 0]
e = b.match_prefix_batch(torch.zeros(0, dtype=torch.uint8, device=dev), row_length=4)
assert len(e) == 0 and e.tolist() == []

# lifetime: the inputs go, other work comes, then the columns are read
want = definition(MIXED, data, anchors_of(len(data), pos_np, cuts), STD)
t2, pos2, off2 = t.clone(), pos.clone(), off.clone()
r = b.match_at(t2, pos2, offsets=off2)
p, en = torch.from_dlpack(r.pattern), torch.from_dlpack(r.end)
del r, t2, pos2, off2, b
gc.collect()
for k in range(8):
    other = torch.from_numpy(np.frombuffer(planted(len(data), 40 + k), dtype=np.uint8).copy()).to(dev)
    torch.full((len(pos_np),), 5, dtype=torch.int64, device=dev)
    del other
gc.collect()
torch.cuda.synchronize()
assert torch.equal(p.cpu(), torch.from_numpy(want[0])) and torch.equal(en.cpu(), torch.from_numpy(want[1]))
assert torch.equal(t.cpu(), torch.from_numpy(np.frombuffer(data, dtype=np.uint8))) and torch.equal(pos.cpu(), torch.from_numpy(pos_np))
print("OK")
"""


def test_tensors_in_and_torch_out():
    """match_at and match_prefix_batch on tensors in HBM with split_rows' offsets, a tensor of offsets, row_length and neither,
    all kinds; torch.from_dlpack of the columns on the automaton's device; a case-insensitive handle leaves the tensor as it
    is; positions outside the data; errors; empty inputs; lifetime after the inputs and the automaton are dropped.  In a
    process of its own: torch has to be the first to load the HIP runtime."""
    pytest.importorskip("torch")
    p = subprocess.run([sys.executable, "-c", _TENSOR_SCRIPT, ROOT, os.path.join(ROOT, "tests")], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
