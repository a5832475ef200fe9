"""Per-haystack pattern counts on the device (acx_tally / acx_tally_device / acx_tally_rows_device;
count_by_pattern_sparse_batch): the device stage alone at the seams of its tile kernel, for both key widths and with the
long rows' form forced at small sizes; parity with the oracle through the C ABI for every match kind, on host and device
inputs, for finds that were cut or took the dense path; the Python methods with sequences and with tensors in HBM, torch as
the consumer of the result, lifetime, threads and a seeded random loop.  Expected values come from numpy / collections.Counter
over synthetic records or over the oracle's matches (tests/oracle_lib.py), never from the library; the kernel's seams are
read from its header."""
import gc
import os
import random
import re
import subprocess
import sys
import threading
from collections import Counter

import numpy as np
import pytest

import gen
from oracle_lib import KIND_DFA, Oracle

pytestmark = pytest.mark.gpu
capi = pytest.importorskip("ahocorasick_rs_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ahocorasick_rs_amd", "csrc")
FOLD = bytes.maketrans(bytes(range(65, 91)), bytes(range(97, 123)))


def hip_constants(path: str, names):
    src = open(os.path.join(CSRC, path)).read()
    out = {}
    for n in names:
        m = re.search(r"\b%s\s*=\s*(\d+)\s*[,;]" % n, src)
        assert m, f"{n} is no longer a plain constant of {path}"
        out[n] = int(m.group(1))
    return out


_C = hip_constants("tally.hpp", ("TALLY_THREADS", "TALLY_TILE", "TALLY_MAX_GRID"))
THREADS, TILE, MAX_GRID = _C["TALLY_THREADS"], _C["TALLY_TILE"], _C["TALLY_MAX_GRID"]
LOG2_TILE = TILE.bit_length() - 1
P_SMALL = 1000                        # 32-bit keys
P_LIMIT = 1 << (32 - LOG2_TILE)       # the last set the 32-bit form takes: its highest key is the padding's value
P_WIDE = P_LIMIT + 1                  # 64-bit keys
BIG = TILE * MAX_GRID + TILE + 77     # records for the second turn of the grid-stride loop
GUARD = 0x5A5AA5A55A5AA5A5


def test_constants_are_what_the_sizes_below_assume():
    assert TILE == 1 << LOG2_TILE and THREADS % 64 == 0 and TILE % THREADS == 0 and THREADS + 1 < TILE - 1
    assert P_WIDE <= 1 << 24, "the 64-bit form can no longer be reached with a legal pattern set"
    assert BIG > TILE * MAX_GRID and BIG % TILE % THREADS != 0  # (a second turn of the loop, then a ragged tile)
    assert BIG * 24 <= 256 << 20, "the largest case no longer is a few seconds' worth of copies"


# ---------------------------------------------------------------------------
# the stage alone
# ---------------------------------------------------------------------------
def expected_csr(lengths, patterns):
    """numpy's answer: (row_offsets, pattern, count) of the rows' pattern counts"""
    lengths = np.asarray(lengths, dtype=np.int64)
    row = np.repeat(np.arange(len(lengths), dtype=np.int64), lengths)
    key, cnt = np.unique((row << 24) | patterns.astype(np.int64), return_counts=True)
    per_row = np.bincount(key >> 24, minlength=len(lengths)) if len(key) else np.zeros(len(lengths), np.int64)
    ro = np.concatenate([[0], np.cumsum(per_row)]).astype(np.int64)
    return ro, (key & ((1 << 24) - 1)).astype(np.int64), cnt.astype(np.int64)


def run_stage(lengths, patterns, n_patterns):
    """tally_rows_device on synthetic records (start and end words are distinct junk: a kernel that reads the wrong field
    shows) with guard words before, between and after the three outputs -> (row_offsets, pattern, count), checked guards"""
    lengths = np.asarray(lengths, dtype=np.uint64)
    n, rows = int(lengths.sum()), len(lengths)
    assert len(patterns) == n and (n == 0 or int(patterns.max()) < n_patterns)
    m = np.empty((n, 3), dtype=np.uint64)
    m[:, 0] = patterns
    m[:, 1] = np.arange(n, dtype=np.uint64) * np.uint64(7) + np.uint64(1 << 40)
    m[:, 2] = np.arange(n, dtype=np.uint64) * np.uint64(11) + np.uint64(1 << 41)
    d_m = capi.DeviceBuffer(max(24 * n, 8)).upload(m) if n else capi.DeviceBuffer(8)
    d_c = capi.DeviceBuffer(max(8 * rows, 8))
    if rows:
        d_c.upload(lengths)
    # [g][row offsets: rows + 1][g g][pattern: n][g g][count: n][g]
    at_ro, at_p = 1, 1 + rows + 1 + 2
    at_c = at_p + n + 2
    image = np.full(at_c + n + 1, GUARD, dtype=np.uint64)
    out = capi.DeviceBuffer(8 * len(image)).upload(image)
    nnz = capi.tally_rows_device(d_m.ptr if n else 0, n, d_c.ptr if rows else 0, rows, n_patterns, out.ptr + 8 * at_ro,
                                 out.ptr + 8 * at_p, out.ptr + 8 * at_c)
    got = np.empty(len(image), dtype=np.uint64)
    capi._check(capi.lib().acx_device_download(got.ctypes.data, out.ptr, 8 * len(image)))
    for b in (d_m, d_c, out):
        b.free()
    assert 0 <= nnz <= n
    for lo, hi in ((0, at_ro), (at_ro + rows + 1, at_p), (at_p + nnz, at_c), (at_c + nnz, len(image))):
        assert (got[lo:hi] == GUARD).all(), ("a word outside the outputs was written", lo, hi)
    return got[at_ro:at_ro + rows + 1].view(np.int64), got[at_p:at_p + nnz].view(np.int64), got[at_c:at_c + nnz].view(np.int64)


def check_stage(lengths, patterns, n_patterns, what):
    patterns = np.asarray(patterns, dtype=np.uint64)
    got = run_stage(lengths, patterns, n_patterns)
    want = expected_csr(lengths, patterns)
    for name, g, w in zip(("row_offsets", "pattern", "count"), got, want):
        if len(g) != len(w) or not np.array_equal(g, w):
            bad = int(np.flatnonzero(g[:min(len(g), len(w))] != w[:min(len(g), len(w))])[:1].sum())
            raise AssertionError((what, name, "lengths", len(g), len(w), "first difference at", bad, g[bad:bad + 4], w[bad:bad + 4]))


# row lengths: every seam of the tile kernel (tests/test_gpu_tally.py's docstring; the issue's list)
SHAPES = {
    "seams": [0, 1, 2, 63, 0, 64, 65, THREADS - 1, THREADS + 1, 0, 0, TILE - 1, TILE, 3, TILE + 1, 1],
    "widest-staging": [TILE - 1, TILE, 5],                       # a row of TILE records that begins at a tile's last record
    "ends-on-the-boundary": [TILE - 3, 3, 7, TILE - 7, TILE, 2],  # a row ends where a tile ends, the next begins there
    "tile-inside-a-long-row": [10, 3 * TILE + 5, 10],             # a tile in which no row begins
    "empty-rows": [0] * 5000 + [3] + [0] * 5000 + [4, 1] + [0] * 5000,
    "long-and-short": [TILE + 1, 5, 2 * TILE + 7, 0, 64, TILE + 300],  # alternating, a long row first and last
    "every-row-long": [TILE + 1, TILE + 2, 3 * TILE],
    "one-record": [1],
    "all-empty": [0, 0, 0],
}


def contents(n, n_patterns, kind, rng):
    if kind == "one":
        return np.full(n, n_patterns - 1, dtype=np.uint64)
    if kind == "distinct":  # (every record another pattern, as far as the set goes; descending: the sort has work)
        return (np.uint64(n_patterns - 1) - np.arange(n, dtype=np.uint64) % np.uint64(n_patterns))
    if kind == "few":       # equal patterns across every row boundary
        return rng.integers(0, 3, size=n).astype(np.uint64)
    return rng.integers(0, n_patterns, size=n).astype(np.uint64)


@pytest.mark.parametrize("row_max", [None, "0", "1", "64"])
@pytest.mark.parametrize("n_patterns", [P_SMALL, P_LIMIT, P_WIDE])
def test_stage_shapes(monkeypatch, n_patterns, row_max):
    """every shape x every kind of contents, for both key widths and the 32-bit form's last set, with the long rows' form
    taking rows beyond 0, 1, 64 and TILE records: the answer is numpy's whichever form a row took"""
    if row_max is not None:
        monkeypatch.setenv("ACX_TALLY_ROW_MAX", row_max)
    rng = np.random.default_rng(7)
    for name, lengths in SHAPES.items():
        n = sum(lengths)
        for kind in ("one", "distinct", "few", "random"):
            check_stage(lengths, contents(n, n_patterns, kind, rng), n_patterns, (name, kind, n_patterns, row_max))


@pytest.mark.parametrize("n_patterns", [P_SMALL, P_LIMIT, P_WIDE])
def test_stage_last_pattern_in_the_last_row_of_a_tile(n_patterns):
    """the key of (the last slot of a tile, the last pattern): all ones in the 32-bit form at its limit -- the value of the
    sort's padding, and of the keys of long rows' records"""
    last = n_patterns - 1
    rng = np.random.default_rng(11)
    for tail in ([last], [last, last, 0, last], [last] * 70, [5, last]):
        lengths = [TILE - 1, len(tail), 2, TILE - 1 - len(tail) - 2 + TILE, 3]  # (the fourth row ends at 2 * TILE - 1 ...)
        lengths[3] = 2 * TILE - 1 - sum(lengths[:3])
        assert sum(lengths[:4]) == 2 * TILE - 1                                 # (... so the fifth begins at a last slot too)
        pats = np.concatenate([rng.integers(0, n_patterns, size=TILE - 1), tail, [last, 0],
                               rng.integers(0, n_patterns, size=lengths[3]), [last, last, 1]]).astype(np.uint64)
        check_stage(lengths, pats, n_patterns, ("collision", n_patterns, tail[:4]))


@pytest.mark.parametrize("n_patterns", [P_SMALL, P_WIDE])
def test_stage_second_turn_of_the_grid_stride_loop(n_patterns):
    rng = np.random.default_rng(13)
    lengths = rng.integers(0, 41, size=BIG // 16).astype(np.int64)
    lengths = lengths[:int(np.searchsorted(np.cumsum(lengths), BIG))]
    lengths = np.append(lengths, BIG - lengths.sum())
    assert lengths.sum() == BIG and lengths[-1] <= TILE
    check_stage(lengths, rng.integers(0, min(n_patterns, 50), size=BIG).astype(np.uint64) * np.uint64(n_patterns // 50),
                n_patterns, ("big", n_patterns))


def test_stage_refuses_counts_that_do_not_sum():
    for lengths in ([3, 3], [1], [0, 9]):
        with pytest.raises(ValueError) as ei:
            run_stage_raw_counts(lengths, 5)
        assert ei.value.code == capi.EINVAL


def run_stage_raw_counts(lengths, n):
    m = np.zeros((n, 3), dtype=np.uint64)
    d_m, d_c = capi.DeviceBuffer(24 * n).upload(m), capi.DeviceBuffer(8 * len(lengths)).upload(np.asarray(lengths, np.uint64))
    out = capi.DeviceBuffer(8 * (len(lengths) + 1 + 2 * n))
    try:
        return capi.tally_rows_device(d_m.ptr, n, d_c.ptr, len(lengths), 10, out.ptr, out.ptr + 8 * (len(lengths) + 1),
                                      out.ptr + 8 * (len(lengths) + 1 + n))
    finally:
        for b in (d_m, d_c, out):
            b.free()


# ---------------------------------------------------------------------------
# end to end through the C ABI against the oracle
# ---------------------------------------------------------------------------
PATS = gen.gen_patterns(500, 3, 9, gen.AZ, 5) + [b"ab", b"abab", b"bab", b"ab"]  # (a copy: overlapping reports it)
KINDS = [(0, False), (0, True), (1, False), (2, False)]


def oracle_rows(o, hays, ov):
    """the definition: per haystack the (pattern, count) of its matches, patterns ascending"""
    return [sorted(Counter(int(p) for p in o.find_raw(h, overlapping=ov)[:, 0]).items()) for h in hays]


def csr_of(rows):
    ro, pat, cnt = [0], [], []
    for r in rows:
        pat += [p for p, _ in r]
        cnt += [c for _, c in r]
        ro.append(len(pat))
    return np.asarray(ro, np.int64), np.asarray(pat, np.int64), np.asarray(cnt, np.int64)


def download_words(ptr: int, n: int) -> np.ndarray:
    out = np.empty(n, dtype=np.int64)
    if n:
        capi._check(capi.lib().acx_device_download(out.ctypes.data, ptr, 8 * n))
    return out


def check_tally(t, rows, on_device, what=None):
    """a capi.DeviceTally against the oracle's rows, through the copies and through the raw addresses"""
    ro, pat, cnt = csr_of(rows)
    assert t.on_device == on_device and t.rows == len(rows) and t.nnz == len(pat), (what, t.rows, t.nnz, len(pat))
    for k, want in ((capi.TALLY_ROW_OFFSETS, ro), (capi.TALLY_PATTERN, pat), (capi.TALLY_COUNT, cnt)):
        assert np.array_equal(t.part(k), want), (what, k)
        p = t.data_ptr(k)
        assert p and p % 8 == 0, (what, k)  # (an empty part still has an address)
        if on_device:
            assert p % 256 == 0 and np.array_equal(download_words(p, len(want)), want), (what, k)
        else:
            assert np.array_equal(np.ctypeslib.as_array((capi.ctypes.c_int64 * max(len(want), 1)).from_address(p))[:len(want)], want)
    t.free()


def batch_with_empties(pats, n_hay, seed):
    """n_hay haystacks of 0 .. 3000 bytes: empty ones in front, in the middle (two in a row) and at the end, some without a
    match (the shape of tests/test_gpu_summary.py's)"""
    rng = gen.SplitMix64(seed)
    hays = []
    for i in range(n_hay):
        n = [0, 17, 300, 3000, 64][rng.next() % 5]
        h = gen.gen_textlike(n, seed + i, pats).tobytes() if i % 3 else gen.gen_uniform(n, b"0123", seed + i).tobytes()
        hays.append(h)
    for i in (0, 1, n_hay // 2, n_hay // 2 + 1, n_hay - 1):
        if 0 <= i < n_hay and n_hay > 4:
            hays[i] = b""
    return hays


def device_tally(a, hays, off, **kw):
    """the batch behind one another in HBM at `off` modulo 16, ragged offsets on the device -> DeviceTally"""
    blob = b"".join(hays)
    offs = np.concatenate([[0], np.cumsum([len(h) for h in hays])]).astype(np.uint64)
    d_hay = capi.DeviceBuffer(len(blob) + 32).upload(np.frombuffer(b"\xa5" * off + blob, dtype=np.uint8))
    d_off = capi.DeviceBuffer(8 * len(offs)).upload(offs)
    t = a.tally_device(d_hay.ptr + off, len(blob), d_offsets=d_off.ptr, n_hay=len(hays), **kw)
    t.nnz  # (known at return)
    return t, (d_hay, d_off)


@pytest.mark.parametrize("mk,ov", KINDS)
def test_parity_host_and_device_inputs(monkeypatch, mk, ov):
    o = Oracle(PATS, mk, KIND_DFA)
    a = capi.Automaton(PATS, mk)
    for n_hay in (1, 65, 323):
        hays = batch_with_empties(PATS, n_hay, 100 + n_hay)
        rows = oracle_rows(o, hays, ov)
        for host_max in ("0", str(1 << 40)):  # the device route and the host route of a host input: a host result either way
            monkeypatch.setenv("ACX_TALLY_HOST_MAX", host_max)
            check_tally(a.tally(hays, overlapping=ov), rows, False, (mk, ov, n_hay, host_max))
        monkeypatch.delenv("ACX_TALLY_HOST_MAX")
        for off in (0, 5):
            t, keep = device_tally(a, hays, off, overlapping=ov)
            check_tally(t, rows, True, (mk, ov, n_hay, off))
            for k in keep:
                k.free()
    # a uniform batch on the device, and the same bytes as a host batch
    L, nh = 512, 130
    full = gen.gen_textlike(L * nh, 61, PATS).tobytes()
    hays = [full[i * L:(i + 1) * L] for i in range(nh)]
    rows = oracle_rows(o, hays, ov)
    dev = capi.DeviceBuffer(len(full)).upload(np.frombuffer(full, dtype=np.uint8))
    check_tally(a.tally_device(dev.ptr, len(full), n_hay=nh, uniform_len=L, overlapping=ov), rows, True, "uniform")
    dev.free()
    check_tally(a.tally(hays, overlapping=ov), rows, False, "uniform, host")
    a.close()


def test_long_rows_form_end_to_end(monkeypatch):
    o, a = Oracle(PATS, 0, KIND_DFA), capi.Automaton(PATS, 0)
    hays = batch_with_empties(PATS, 97, 7) + [b"abab" * 3000, b"", gen.gen_textlike(400_000, 3, PATS).tobytes()]
    rows = oracle_rows(o, hays, True)
    assert max(sum(c for _, c in r) for r in rows) > TILE  # (a row the tile kernel leaves to the radix form as shipped)
    for row_max in (None, "0", "1", "64"):
        if row_max is not None:
            monkeypatch.setenv("ACX_TALLY_ROW_MAX", row_max)
        t, keep = device_tally(a, hays, 0, overlapping=True)
        check_tally(t, rows, True, row_max)
        for k in keep:
            k.free()
    a.close()


def test_results_freed_unread_and_in_reverse_order():
    """the seams of the result's owner: a result freed with no accessor ever called (the free waits for the stage) and the
    identical call after it, whose blocks come from the cache; eight results alive at once, four freed unread in the opposite
    order to their creation, a result made where their blocks went, and the other four read afterwards"""
    pats = [b"ab", b"abab", b"bab", b"needle", b"hay", b"stack", b"a", b"zz", b"0123", b"ab"]
    o, a = Oracle(pats, 0, KIND_DFA), capi.Automaton(pats, 0)
    batches = [[gen.gen_textlike([0, 7, 64, 255][(i + k) % 4], 50 + 8 * k + i, pats).tobytes() for i in range(5 + 7 * k)] for k in range(8)]
    want = [oracle_rows(o, hays, True) for hays in batches]
    t, keep = device_tally(a, batches[3], 0, overlapping=True)
    t.free()
    t, keep2 = device_tally(a, batches[3], 0, overlapping=True)
    check_tally(t, want[3], True, "the second call")
    made = [device_tally(a, hays, 0, overlapping=True) for hays in batches]
    for k in (7, 6, 5, 4):
        made[k][0].free()
    t, keep3 = device_tally(a, batches[6], 0, overlapping=True)
    check_tally(t, want[6], True, "behind the four freed")
    for k in (3, 2, 1, 0):
        check_tally(made[k][0], want[k], True, k)
    # one haystack that is no batch: the find kept no counts
    hay = b"".join(batches[7])
    dev = capi.DeviceBuffer(len(hay) + 16).upload(np.frombuffer(hay + b"\0", dtype=np.uint8))
    check_tally(a.tally_device(dev.ptr, len(hay), overlapping=True), oracle_rows(o, [hay], True), True, "no batch")
    for d in [dev, *keep, *keep2, *keep3] + [d for _, ks in made for d in ks]:
        d.free()
    a.close()


def test_case_insensitive_handle():
    pats = [b"Needle", b"hay", b"STACK"]
    o = Oracle([p.translate(FOLD) for p in pats], 1, KIND_DFA)
    hays = [b"a nEEdle in a HayStack, a NEEDLE in a haySTACK; " * k for k in (0, 1, 30, 3000)]
    rows = oracle_rows(o, [h.translate(FOLD) for h in hays], False)
    a = capi.Automaton(pats, 1, ascii_case_insensitive=True)
    check_tally(a.tally(hays), rows, False)
    t, keep = device_tally(a, hays, 5)
    check_tally(t, rows, True)
    assert np.array_equal(keep[0].download(5 + sum(map(len, hays)))[5:], np.frombuffer(b"".join(hays), dtype=np.uint8))
    for k in keep:
        k.free()
    a.close()


def test_a_batch_cut_by_a_lowered_occurrence_limit(monkeypatch):
    pats = [b"ab", b"b", b"bab"]
    r = random.Random(5)
    hays = [b"ab" * r.randint(1, 60_000) + bytes(r.choice(b"abc") for _ in range(r.randint(0, 300))) for _ in range(7)] + [b"", b"abab"]
    for mk, ov in KINDS:
        o, a = Oracle(pats, mk, KIND_DFA), capi.Automaton(pats, mk)
        rows = oracle_rows(o, hays, ov)
        monkeypatch.setenv("ACX_MAX_OCC", "50000")
        monkeypatch.setenv("ACX_NO_BUCKET", "1")
        a.path_stats(reset=True)
        t, keep = device_tally(a, hays, 0, overlapping=ov)
        st = a.path_stats()
        monkeypatch.delenv("ACX_MAX_OCC")
        monkeypatch.delenv("ACX_NO_BUCKET")
        assert st["byte_ranges"] >= 2, st
        check_tally(t, rows, True, (mk, ov))
        for k in keep:
            k.free()
        a.close()


def test_a_find_on_the_dense_path():
    pats = gen.gen_patterns(2000, 5, 12, gen.AZ, 1)
    a, o = capi.Automaton(pats, 0, capi.IMPL_DFA), Oracle(pats, 0, KIND_DFA)
    every = bytearray(gen.gen_uniform(8 << 20, gen.AZ, 13).tobytes())  # (the size tests/test_gpu_columns.py uses)
    rng = gen.SplitMix64(77)
    for k in range(0, len(every) - 32, 32):
        p = pats[rng.next() % len(pats)]
        every[k:k + len(p)] = p
    every = bytes(every)
    L = 1 << 16
    hays = [every[i:i + L] for i in range(0, len(every), L)]
    m = o.find_raw(every)  # (no pattern is longer than 12: cut at the rows' ends below, none is lost but those across them)
    rows = oracle_rows(o, hays, False)
    assert len(m) >= len(every) // 32 and sum(c for r in rows for _, c in r) >= len(every) // 33
    one = [sorted(Counter(int(p) for p in m[:, 0]).items())]
    dev = capi.DeviceBuffer(len(every)).upload(np.frombuffer(every, dtype=np.uint8))
    a.path_stats(reset=True)
    for _ in range(2):  # (one haystack that is no batch: the call tests/test_gpu_columns.py sees take that path)
        check_tally(a.tally_device(dev.ptr, len(every)), one, True)
    st = a.path_stats()
    assert st["hot_calls"] + st["dense_tiles"] + st["dense_radix"] >= 2, st
    check_tally(a.tally_device(dev.ptr, len(every), n_hay=len(hays), uniform_len=L), rows, True)
    dev.free()
    a.close()


def test_no_match_at_all_and_empty_batches(monkeypatch):
    a = capi.Automaton(PATS, 0)
    for hays in ([], [b"", b""], [b"0123", b"", b"4567" * 500]):
        rows = [[] for _ in hays]
        for host_max in ("0", str(1 << 40)):
            monkeypatch.setenv("ACX_TALLY_HOST_MAX", host_max)
            check_tally(a.tally(hays), rows, False, (len(hays), host_max))
        t, keep = device_tally(a, hays, 0)
        check_tally(t, rows, True, len(hays))
        for k in keep:
            k.free()
    dev = capi.DeviceBuffer(1 << 20).upload(np.frombuffer(b"0123" * (1 << 18), dtype=np.uint8))
    check_tally(a.tally_device(dev.ptr, 1 << 20, n_hay=1 << 10, uniform_len=1 << 10), [[]] * (1 << 10), True)
    check_tally(a.tally_device(dev.ptr, 0, n_hay=0, uniform_len=1 << 10), [], True)
    dev.free()
    b = capi.Automaton([b"ab", b"b"], 1)
    with pytest.raises(ValueError) as ei:
        b.tally([b"xxabxx"], overlapping=True)
    assert ei.value.code == capi.EOVERLAP
    b.close()
    a.close()


# ---------------------------------------------------------------------------
# the Python method: sequences of host objects (tensors in HBM and torch as the consumer: the script below)
# ---------------------------------------------------------------------------
def matchkind(ar, mk):
    return (ar.MatchKind.Standard, ar.MatchKind.LeftmostFirst, ar.MatchKind.LeftmostLongest)[mk]


def check_counts(pc, rows, n_patterns, device=None):
    """a PatternCounts in host memory (or, device given, through tolist() alone) against the oracle's rows"""
    ro, pat, cnt = csr_of(rows)
    assert pc.shape == (len(rows), n_patterns) and len(pc) == len(pat) and pc.device == device
    assert pc.tolist() == [[(int(p), int(c)) for p, c in r] for r in rows]
    if device is None:
        for col, want in ((pc.row_offsets, ro), (pc.pattern, pat), (pc.count, cnt)):
            assert len(col) == len(want) and col.__dlpack_device__() == (1, 0)
            got = np.from_dlpack(col)
            assert got.dtype == np.int64 and np.array_equal(got, want)
            assert np.array_equal(np.asarray(memoryview(col)), want)


@pytest.mark.parametrize("mk,ov", KINDS)
def test_python_sequences_both_classes(mk, ov):
    import ahocorasick_rs as ar
    o = Oracle(PATS, mk, KIND_DFA)
    b = ar.BytesAhoCorasick(PATS, matchkind=matchkind(ar, mk))
    s = ar.AhoCorasick([p.decode() for p in PATS], matchkind=matchkind(ar, mk))
    for n_hay in (0, 1, 64, 130):
        hays = batch_with_empties(PATS, n_hay, 500 + n_hay)
        rows = oracle_rows(o, hays, ov)
        twin = [sorted(Counter(p for p, _, _ in m).items()) for m in b.find_matches_as_indexes_batch(hays, overlapping=ov)]
        assert twin == rows  # (the definition, through the library's own match lists: the oracle's twin)
        check_counts(b.count_by_pattern_sparse_batch(hays, overlapping=ov), rows, len(PATS))
        check_counts(b.count_by_pattern_sparse_batch(tuple(bytearray(h) for h in hays), ov), rows, len(PATS))
        check_counts(s.count_by_pattern_sparse_batch([h.decode() for h in hays], overlapping=ov), rows, len(PATS))
    # text that is not ASCII: the counts need no code points
    pats = ["é☃", "ab", "b🤦", "☃", "ab"]
    o2 = Oracle([p.encode() for p in pats], mk, KIND_DFA)
    s2 = ar.AhoCorasick(pats, matchkind=matchkind(ar, mk))
    hays = ["", "ab☃é☃b🤦", "xxé☃" * 50, "🤦🤦ab", "é" * 3000 + "☃ab" * 4000]
    check_counts(s2.count_by_pattern_sparse_batch(hays, overlapping=ov), oracle_rows(o2, [h.encode() for h in hays], ov), len(pats))


def test_python_errors():
    import ahocorasick_rs as ar
    b, s = ar.BytesAhoCorasick([b"ab"]), ar.AhoCorasick(["ab"])
    off = np.array([0, 2], dtype=np.int64)
    for call in (lambda: b.count_by_pattern_sparse_batch([b"ab"], offsets=off),          # either keyword with a sequence
                 lambda: b.count_by_pattern_sparse_batch([b"ab"], row_length=2),
                 lambda: s.count_by_pattern_sparse_batch(["ab"], row_length=2),
                 lambda: b.count_by_pattern_sparse_batch(b"ab", row_length=2),            # (bytes is a sequence of ints)
                 lambda: b.count_by_pattern_sparse_batch([b"ab"], False, off),            # keyword-only
                 lambda: b.count_by_pattern_sparse_batch(["ab"]),                          # the items' types
                 lambda: s.count_by_pattern_sparse_batch([b"ab"]),
                 lambda: b.count_by_pattern_sparse_batch(5),
                 lambda: b.count_by_pattern_sparse_batch([b"ab"], overlapping=1)):
        with pytest.raises(TypeError):
            call()
    t = np.frombuffer(b"abxabx", dtype=np.uint8).copy()  # (writable: numpy exports no read-only array through DLPack)
    # a host tensor behind DLPack (numpy: it is a buffer too, so a keyword makes it THE tensor)
    assert b.count_by_pattern_sparse_batch(t, row_length=3).tolist() == [[(0, 1)], [(0, 1)]]
    assert b.count_by_pattern_sparse_batch(t, offsets=np.array([0, 1, 1, 6], dtype=np.int64)).tolist() == [[], [], [(0, 1)]]
    assert s.count_by_pattern_sparse_batch(t, row_length=6).tolist() == [[(0, 2)]]
    for call in (lambda: b.count_by_pattern_sparse_batch(t, row_length=3, offsets=np.array([0, 6], dtype=np.int64)),  # both
                 lambda: b.count_by_pattern_sparse_batch(t, row_length=3.0),
                 lambda: b.count_by_pattern_sparse_batch(t, offsets=[0, 6]),
                 lambda: b.count_by_pattern_sparse_batch(t, offsets=np.array([0, 6], dtype=np.int32)),
                 lambda: b.count_by_pattern_sparse_batch(t.reshape(2, 3), row_length=3)):
        with pytest.raises(TypeError):
            call()
    for call in (lambda: b.count_by_pattern_sparse_batch(t, row_length=4), lambda: b.count_by_pattern_sparse_batch(t, row_length=0),
                 lambda: b.count_by_pattern_sparse_batch(t, offsets=np.array([0, 5], dtype=np.int64)),
                 lambda: b.count_by_pattern_sparse_batch(t, offsets=np.array([1, 6], dtype=np.int64)),
                 lambda: b.count_by_pattern_sparse_batch(t, offsets=np.array([0, 4, 3, 6], dtype=np.int64)),
                 lambda: b.count_by_pattern_sparse_batch(t, offsets=np.array([], dtype=np.int64))):
        with pytest.raises(ValueError):
            call()
    for mk in (ar.MatchKind.LeftmostFirst, ar.MatchKind.LeftmostLongest):
        with pytest.raises(ValueError):
            ar.BytesAhoCorasick([b"ab"], matchkind=mk).count_by_pattern_sparse_batch([b"ab"], overlapping=True)
    with pytest.raises(TypeError):
        ar.PatternCounts()


def test_host_columns_outlive_the_pattern_counts():
    import ahocorasick_rs as ar
    o, b = Oracle(PATS, 0, KIND_DFA), ar.BytesAhoCorasick(PATS)
    hays = batch_with_empties(PATS, 300, 3)
    want = csr_of(oracle_rows(o, hays, False))
    pc = b.count_by_pattern_sparse_batch(hays)
    arrays = [np.from_dlpack(x) for x in (pc.row_offsets, pc.pattern, pc.count)]
    views = [memoryview(x) for x in (pc.row_offsets, pc.pattern, pc.count)]
    unused = pc.pattern.__dlpack__()  # (a capsule nobody consumes gives its reference back too)
    del pc, unused
    gc.collect()
    for k in range(20):  # (other results come and go where the parts' memory would be if it had been freed)
        b.count_by_pattern_sparse_batch(batch_with_empties(PATS, 300, 50 + k))
    for got, mv, w in zip(arrays, views, want):
        assert np.array_equal(got, w) and np.array_equal(np.asarray(mv), w)


def test_eight_threads_on_one_handle(monkeypatch):
    import ahocorasick_rs as ar
    b, a, o = ar.BytesAhoCorasick(PATS), capi.Automaton(PATS, 0), Oracle(PATS, 0, KIND_DFA)
    work = []
    for t in range(8):
        hays = batch_with_empties(PATS, 40 + 9 * t, 300 + t) + [gen.gen_textlike(150_000, t, PATS).tobytes()]
        work.append((hays, oracle_rows(o, hays, False)))
    errors = []

    def run(t):
        try:
            hays, rows = work[t]
            for _ in range(3):
                check_counts(b.count_by_pattern_sparse_batch(hays), rows, len(PATS))
                dt, keep = device_tally(a, hays, t)
                check_tally(dt, rows, True, t)
                for k in keep:
                    k.free()
        except BaseException as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=run, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    a.close()


def test_seeded_random_batches(monkeypatch):
    rng = random.Random(20261017)
    for case in range(40):
        mk = rng.choice([0, 0, 1, 2])
        ov = mk == 0 and rng.random() < 0.4
        alpha = rng.choice([b"ab", b"abcd", gen.AZ])
        pats = gen.gen_patterns(rng.choice([1, 3, 40, 600]), 1, rng.choice([2, 6, 12]), alpha, 1000 + case)
        text = rng.choice([alpha, alpha + b"xyz", b"0123"])
        o = Oracle(pats, mk, KIND_DFA)
        n_hay = rng.choice([1, 2, 7, 64, 65, 130, 700])
        hays = [bytes(rng.choices(text, k=rng.choice([0, 0, 1, 9, 200, 5000]))) for _ in range(n_hay)]
        per = [o.find_raw(h, overlapping=ov)[:, 0] for h in hays]
        while sum(len(p) for p in per) > 100_000:  # (cut down, never skipped)
            hays = [h[:len(h) // 2] for h in hays]
            per = [o.find_raw(h, overlapping=ov)[:, 0] for h in hays]
        rows = [sorted(Counter(int(p) for p in x).items()) for x in per]
        route, row_max = rng.choice(["host", "staged", "device"]), rng.choice([None, "0", "1", "64"])
        if row_max is None:
            monkeypatch.delenv("ACX_TALLY_ROW_MAX", raising=False)
        else:
            monkeypatch.setenv("ACX_TALLY_ROW_MAX", row_max)
        monkeypatch.setenv("ACX_TALLY_HOST_MAX", "0" if route == "staged" else str(1 << 40))
        a = capi.Automaton(pats, mk)
        what = (case, mk, ov, n_hay, route, row_max)
        try:
            if route == "device":
                t, keep = device_tally(a, hays, rng.randrange(16), overlapping=ov)
                check_tally(t, rows, True, what)
                for k in keep:
                    k.free()
            else:
                check_tally(a.tally(hays, overlapping=ov), rows, False, what)
        except AssertionError as e:
            raise AssertionError(f"case {what}: {e}") from e
        a.close()


# ---------------------------------------------------------------------------
# tensors in HBM through the Python method, and torch as the consumer of the result
# ---------------------------------------------------------------------------
_TENSOR_SCRIPT = r"""
import gc
import sys
from collections import Counter
import torch  # first: one process holds ONE HIP runtime, and torch must be the one to load it
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
import gen
from oracle_lib import KIND_DFA, Oracle
import ahocorasick_rs as ar
pats = gen.gen_patterns(300, 3, 9, gen.AZ, 5) + [b"ab", b"abab", b"bab", b"ab"]
L, nh = 4096, 200
hay = gen.gen_textlike(L * nh, 13, pats)
t = torch.from_numpy(hay.copy()).to("cuda:0")
kinds = (ar.MatchKind.Standard, ar.MatchKind.LeftmostFirst, ar.MatchKind.LeftmostLongest)
lens = [0, 0, 17, L, 3 * L, 5, 0, 2 * L + 1]
lens += [L * nh - sum(lens), 0]
cuts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)

def rows_of(o, hays, ov):
    return [sorted(Counter(int(p) for p in o.find_raw(h, overlapping=ov)[:, 0]).items()) for h in hays]

def dense_of(rows):
    d = torch.zeros((len(rows), len(pats)), dtype=torch.int64)
    for h, r in enumerate(rows):
        for p, c in r:
            d[h, p] = c
    return d

def check(pc, rows, where):
    assert pc.shape == (len(rows), len(pats)) and pc.device == (0 if where == "device" else None), (where, pc.shape, pc.device)
    assert len(pc) == sum(len(r) for r in rows)
    assert pc.tolist() == [[(int(p), int(c)) for p, c in r] for r in rows], where
    parts = [torch.from_dlpack(x) for x in (pc.row_offsets, pc.pattern, pc.count)]
    for x, n in zip(parts, (len(rows) + 1, len(pc), len(pc))):
        assert x.dtype == torch.int64 and tuple(x.shape) == (n,) and x.is_contiguous()
        assert x.device.type == ("cuda" if where == "device" else "cpu"), (where, x.device)
    if len(rows):
        m = torch.sparse_csr_tensor(*parts, size=pc.shape)   # the three parts as they are
        assert torch.equal(m.to_dense().cpu(), dense_of(rows)), where
    return parts

for mk, ov in ((0, False), (0, True), (1, False), (2, False)):
    o = Oracle(pats, mk, KIND_DFA)
    b = ar.BytesAhoCorasick(pats, matchkind=kinds[mk])
    s = ar.AhoCorasick([p.decode() for p in pats], matchkind=kinds[mk])
    uniform = [hay[i * L:(i + 1) * L].tobytes() for i in range(nh)]
    ragged = [hay[cuts[i]:cuts[i + 1]].tobytes() for i in range(len(lens))]
    ru, rr = rows_of(o, uniform, ov), rows_of(o, ragged, ov)
    d_cuts = torch.from_numpy(cuts).to("cuda:0")
    for obj in (b, s):
        pc = obj.count_by_pattern_sparse_batch(t, overlapping=ov, row_length=L)     # a tensor in HBM: the result stays there
        for x in (pc.row_offsets, pc.pattern, pc.count):
            assert x.__dlpack_device__() == (10, 0)
            try:
                memoryview(x)
                raise SystemExit("a device column exported a host buffer")
            except BufferError:
                pass
        check(pc, ru, "device")
        check(obj.count_by_pattern_sparse_batch(t, ov, offsets=d_cuts), rr, "device")
    check(b.count_by_pattern_sparse_batch(torch.from_numpy(hay), overlapping=ov, row_length=L), ru, "host")  # host memory behind DLPack
    check(b.count_by_pattern_sparse_batch(torch.from_numpy(hay), overlapping=ov, offsets=torch.from_numpy(cuts)), rr, "host")
    check(b.count_by_pattern_sparse_batch(uniform, overlapping=ov), ru, "host")

o, b = Oracle(pats, 0, KIND_DFA), ar.BytesAhoCorasick(pats)
# an odd device address; the consumer on a stream of its own
side = torch.cuda.Stream()
with torch.cuda.stream(side):
    parts = check(b.count_by_pattern_sparse_batch(t[5:5 + 100 * L], row_length=L), rows_of(o, [hay[5 + i * L:5 + (i + 1) * L].tobytes() for i in range(100)], False), "device")
    total = parts[2].sum()
assert int(total) == sum(len(o.find_raw(hay[5 + i * L:5 + (i + 1) * L].tobytes())) for i in range(100))

# the errors of the tensor form
d_cuts = torch.from_numpy(cuts).to("cuda:0")
def raises(exc, call):
    try:
        call()
    except exc:
        return
    raise SystemExit("no %s" % exc.__name__)
raises(TypeError, lambda: b.count_by_pattern_sparse_batch(t))                                   # neither
raises(TypeError, lambda: b.count_by_pattern_sparse_batch(t, row_length=L, offsets=d_cuts))     # both
raises(TypeError, lambda: b.count_by_pattern_sparse_batch(torch.from_numpy(hay)))               # neither, host
raises(ValueError, lambda: b.count_by_pattern_sparse_batch(t, offsets=torch.from_numpy(cuts)))  # offsets on another device
raises(ValueError, lambda: b.count_by_pattern_sparse_batch(torch.from_numpy(hay), offsets=d_cuts))
raises(ValueError, lambda: b.count_by_pattern_sparse_batch(t, row_length=L - 1))
raises(ValueError, lambda: b.count_by_pattern_sparse_batch(t, offsets=d_cuts[:-2]))             # does not end at the length
raises(ValueError, lambda: b.count_by_pattern_sparse_batch(t, offsets=d_cuts[1:] if cuts[1] else d_cuts[3:]))
raises(TypeError, lambda: b.count_by_pattern_sparse_batch(t, offsets=d_cuts.to(torch.int32)))
raises(BufferError, lambda: b.count_by_pattern_sparse_batch(t.to(torch.int32), row_length=L))   # (the haystack's own error)

# no match, no rows: the parts still become tensors
z = torch.full((1 << 20,), 48, dtype=torch.uint8, device="cuda:0")
pc = b.count_by_pattern_sparse_batch(z, row_length=1 << 10)
check(pc, [[]] * (1 << 10), "device")
pc = b.count_by_pattern_sparse_batch(torch.zeros(0, dtype=torch.uint8, device="cuda:0"), row_length=7)
assert pc.shape == (0, len(pats)) and len(pc) == 0 and pc.tolist() == []
assert torch.equal(torch.from_dlpack(pc.row_offsets).cpu(), torch.zeros(1, dtype=torch.int64))
assert tuple(torch.from_dlpack(pc.pattern).shape) == (0,)
pc = b.count_by_pattern_sparse_batch([])
assert torch.equal(torch.from_dlpack(pc.row_offsets), torch.zeros(1, dtype=torch.int64)) and pc.shape == (0, len(pats))

# lifetime: the tensors keep the result alive after the PatternCounts object is gone
rows = rows_of(o, [hay[i * L:(i + 1) * L].tobytes() for i in range(nh)], False)
pc = b.count_by_pattern_sparse_batch(t, row_length=L)
parts = [torch.from_dlpack(x) for x in (pc.row_offsets, pc.pattern, pc.count)]
unused = pc.count.__dlpack__()
del pc, unused
gc.collect()
for k in range(6):  # (other results come and go where the parts would be if they had been given back)
    other = torch.from_numpy(gen.gen_textlike(L * nh, 40 + k, pats).copy()).to("cuda:0")
    keep = b.count_by_pattern_sparse_batch(other, row_length=L)
    del keep
gc.collect()
torch.cuda.synchronize()
assert torch.equal(torch.sparse_csr_tensor(*parts, size=(nh, len(pats))).to_dense().cpu(), dense_of(rows))
del parts
gc.collect()
assert torch.equal(t.cpu(), torch.from_numpy(hay))
print("OK")
"""


def test_tensors_in_and_torch_out():
    """count_by_pattern_sparse_batch on tensors in HBM with offsets and with row_length, both classes; its errors;
    torch.sparse_csr_tensor of the parts against the dense oracle matrix; empty results; lifetime.  In a process of its own:
    torch has to be the first to load the HIP runtime."""
    pytest.importorskip("torch")
    p = subprocess.run([sys.executable, "-c", _TENSOR_SCRIPT, ROOT, os.path.join(ROOT, "tests")], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout + p.stderr
