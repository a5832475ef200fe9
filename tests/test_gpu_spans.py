"""The merged spans of a search's matches, on the device (acx_spans / acx_spans_device / acx_spans_rows_device; cover_spans /
cover_spans_batch): the device stage alone at the seams of its tile kernels -- record counts around the tile, spans that open,
close and break on and beside tile boundaries, a carry through a tile that is all one row, rows that cross tiles, runs of empty
rows, row counts around the scan's levels, empty, nested and identical records across a seam, gaps around the hole, words
beyond 2^32 -- with guard words around all three outputs and every input verified unwritten; parity with the definition
through the C ABI for every match kind, on host and device inputs, for finds that were cut or took the dense path; the
identity with match_mask; the Python methods with sequences and with tensors in HBM, torch as the consumer, lifetime, threads
and a seeded random loop.  Expected values come from numpy or Python over synthetic records or from the oracle's matches
(tests/oracle_lib.py) and the sort-and-sweep definition restated below, never from the library; the kernel's seams are read
from its header."""
import gc
import os
import random
import re
import subprocess
import sys
import threading

import numpy as np
import pytest

import gen
from oracle_lib import KIND_DFA, Oracle, byte_to_code_point

pytestmark = pytest.mark.gpu
capi = pytest.importorskip("ahocorasick_rs_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ahocorasick_rs_amd", "csrc")
FOLD = bytes.maketrans(bytes(range(65, 91)), bytes(range(97, 123)))
GAP_MAX = (1 << 63) - 1


def hip_constants(path, names):
    src = open(os.path.join(CSRC, path)).read()
    out = {}
    for n in names:
        m = re.search(r"\b%s\s*=\s*(\d+)\s*[,;]" % n, src)
        assert m, f"{n} is no longer a plain constant of {path}"
        out[n] = int(m.group(1))
    return out


_C = hip_constants("spans.hpp", ("SPANS_THREADS", "SPANS_TILE"))
THREADS, T = _C["SPANS_THREADS"], _C["SPANS_TILE"]
S = 2048  # replace_scan's items per workgroup (replace.hip RS_THREADS * RS_PER): beyond it the scan has two levels, beyond S * S three
GUARD = np.int64(-0x3C3C3C3C3C3C3C3D)
FRESH = np.int64(0x7777777777777777)  # what the outputs hold before the call


def test_constants_are_what_the_sizes_below_assume():
    assert T % THREADS == 0 and THREADS % 64 == 0 and T >= 256
    src = open(os.path.join(CSRC, "replace.hip")).read()
    assert re.search(r"RS_THREADS = 256, RS_PER = 8\b", src), "the scan's level size is no longer 2048"
    assert (capi.SPAN_START, capi.SPAN_END, capi.SPAN_ROW_OFFSETS) == (0, 1, 2)


# ---------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------
def sweep(records, counts, gap):
    """sort and sweep in Python: per row the live records (start < end) by start; a record joins the open span when its
    start is at most the span's end + gap, else it opens the next one -> (row_offsets, (S, 2) uint64)"""
    records = [tuple(int(x) for x in r) for r in np.asarray(records, dtype=np.uint64).reshape(-1, 3).tolist()]
    spans, ro, at = [], [0], 0
    for c in counts:
        c = int(c)
        live = sorted((s, e) for _, s, e in records[at:at + c] if s < e)
        at += c
        first = len(spans)
        for s, e in live:
            if len(spans) > first and s - spans[-1][1] <= gap:
                spans[-1] = (spans[-1][0], max(spans[-1][1], e))
            else:
                spans.append((s, e))
        ro.append(len(spans))
    assert at == len(records)
    return np.asarray(ro, dtype=np.int64), np.asarray(spans, dtype=np.uint64).reshape(-1, 2)


def sweep_np(records, counts, gap):
    """the same in numpy, for batches of many rows: the rows' records are moved K apart (K beyond every end and every
    gap that matters: a gap of max end + 1 already joins a whole row), sorted by start, and a span opens where the start
    exceeds the running maximum of the ends by more than the gap"""
    rec = np.asarray(records, dtype=np.uint64).reshape(-1, 3)
    counts = np.asarray(counts, dtype=np.int64)
    rows = len(counts)
    if not len(rec):
        return np.zeros(rows + 1, dtype=np.int64), np.zeros((0, 2), dtype=np.uint64)
    assert int(rec[:, 1:].max()) < 1 << 40
    st, en = rec[:, 1].astype(np.int64), rec[:, 2].astype(np.int64)
    row = np.repeat(np.arange(rows, dtype=np.int64), counts)
    assert len(row) == len(rec)
    live = st < en
    st, en, row = st[live], en[live], row[live]
    g = int(min(gap, int(en.max(initial=0)) + 1))
    K = 2 * (int(en.max(initial=0)) + 2) + g
    assert rows * K < 1 << 62
    order = np.lexsort((en, st, row))
    st, en, row = st[order] + row[order] * K, en[order] + row[order] * K, row[order]
    reach = np.maximum.accumulate(en)
    opens = np.ones(len(st), dtype=bool)
    opens[1:] = st[1:] - reach[:-1] > g
    first = np.flatnonzero(opens)
    last = np.concatenate([first[1:] - 1, [len(st) - 1]]).astype(np.int64) if len(first) else first
    spans = np.stack([st[first] - row[first] * K, reach[last] - row[first] * K], axis=1).astype(np.uint64)
    ro = np.concatenate([[0], np.cumsum(np.bincount(row[first], minlength=rows))]).astype(np.int64)
    return ro, spans


def test_the_two_forms_of_the_definition_agree():
    rng = np.random.default_rng(1)
    for gap in (0, 1, 3, 50, GAP_MAX):
        counts = rng.choice([0, 0, 1, 2, 7, 40], size=200)
        rec = records_in(counts, rng, span=300)
        a, b = sweep(rec, counts, gap), sweep_np(rec, counts, gap)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), gap


# ---------------------------------------------------------------------------
# the stage alone
# ---------------------------------------------------------------------------
def run_stage(records, counts, gap):
    """spans_rows_device on synthetic records: the three outputs between 8 guard words each, pre-filled -> (row_offsets,
    (S, 2) uint64); the guards, the words behind the S spans and every input checked unwritten"""
    rec = np.ascontiguousarray(np.asarray(records, dtype=np.uint64).reshape(-1, 3))
    counts = np.ascontiguousarray(np.asarray(counts, dtype=np.uint64))
    n, rows = len(rec), len(counts)
    sizes = (rows + 1, n, n)  # row offsets, start, end
    at, total = [], 0
    for w in sizes:
        at.append(total + 8)
        total += 8 + w + 8
    image = np.full(total, GUARD, dtype=np.int64)
    for a, w in zip(at, sizes):
        image[a:a + w] = FRESH
    d_out = capi.DeviceBuffer(image.nbytes + 16).upload(image)
    d_rec = capi.DeviceBuffer(24 * n + 16)
    d_cnt = capi.DeviceBuffer(8 * rows + 16)
    if n:
        d_rec.upload(rec.reshape(-1))
    if rows:
        d_cnt.upload(counts)
    try:
        p = [d_out.ptr + 8 * a for a in at]
        ns = capi.spans_rows_device(d_rec.ptr if n else 0, n, d_cnt.ptr if rows else 0, rows, gap, p[0], p[1], p[2])
        got = d_out.download(image.nbytes).view(np.int64)
        assert np.array_equal(d_rec.download(24 * n).view(np.uint64), rec.reshape(-1)), "the records were written"
        assert np.array_equal(d_cnt.download(8 * rows).view(np.uint64), counts), "the counts were written"
    finally:
        for b in (d_out, d_rec, d_cnt):
            b.free()
    keep = np.ones(total, dtype=bool)
    for a, w in zip(at, sizes):
        keep[a:a + w] = False
    assert (got[keep] == GUARD).all(), ("a guard word was written", int(np.flatnonzero(keep & (got != GUARD))[0]), at)
    assert 0 <= ns <= n
    for a in at[1:]:
        assert (got[a + ns:a + n] == FRESH).all(), ("a word behind the spans was written", int(np.flatnonzero(got[a + ns:a + n] != FRESH)[0]) + ns, ns)
    ro = got[at[0]:at[0] + rows + 1].copy()
    return ro, np.stack([got[at[1]:at[1] + ns], got[at[2]:at[2] + ns]], axis=1).view(np.uint64).reshape(-1, 2)


def check_stage(records, counts, gap=0, what=None, definition=sweep_np):
    ro, spans = run_stage(records, counts, gap)
    want_ro, want = definition(records, counts, gap)
    if len(spans) != len(want) or not np.array_equal(spans, want):
        k = min(len(spans), len(want))
        bad = int(np.flatnonzero((spans[:k] != want[:k]).any(axis=1))[0]) if k and (spans[:k] != want[:k]).any() else k
        raise AssertionError((what, gap, "spans", len(spans), "wanted", len(want), "first difference at", bad, spans[max(bad - 2, 0):bad + 3].tolist(),
                              want[max(bad - 2, 0):bad + 3].tolist()))
    if not np.array_equal(ro, want_ro):
        bad = int(np.flatnonzero(ro != want_ro)[0])
        raise AssertionError((what, gap, "row offsets differ first at row", bad, ro[max(bad - 2, 0):bad + 3].tolist(), want_ro[max(bad - 2, 0):bad + 3].tolist()))
    return want_ro, want


def records_in(counts, rng, span=400, lengths=(1, 1, 2, 3, 5, 8, 13, 40), empties=0.1, base=0):
    """counts[h] records in row h: random starts below `span` (an int, or one per row), some records empty (start == end)
    or reversed, ordered by (end, start) within a row as a search reports them"""
    counts = np.asarray(counts, dtype=np.int64)
    row = np.repeat(np.arange(len(counts)), counts)
    width = np.broadcast_to(np.asarray(span, dtype=np.int64), (len(counts),))[row]
    start = (rng.random(len(row)) * width).astype(np.int64) + base
    end = start + rng.choice(lengths, size=len(row))
    dead = rng.random(len(row)) < empties
    end[dead] = start[dead] - rng.integers(0, 2, size=int(dead.sum()))
    end = np.maximum(end, 0)
    order = np.lexsort((start, end, row))
    return np.stack([rng.integers(0, 1 << 24, size=len(row)), start[order], end[order]], axis=1).astype(np.uint64)


def ragged_counts(n, rng, choices=(0, 0, 1, 2, 3, 7, 40)):
    """per-row record counts from `choices` that sum to exactly n (at least one row)"""
    out, left = [], n
    while left:
        c = min(int(rng.choice(choices)), left)
        out.append(c)
        left -= c
    return out or [0]


@pytest.mark.parametrize("n", [1, T - 1, T, T + 1, 2 * T, 3 * T + 5])
def test_stage_record_counts_around_the_tile(n):
    rng = np.random.default_rng(n)
    for gap in (0, 2):
        counts = ragged_counts(n, rng)
        check_stage(records_in(counts, rng), counts, gap, ("ragged", n))
        counts = ragged_counts(n, rng, (0, 1, 300, 700))
        check_stage(records_in(counts, rng, span=3000), counts, gap, ("rows of many records", n))
        check_stage(records_in([1] * n, rng), [1] * n, gap, ("every row of one record", n))
        check_stage(records_in([n], rng, span=6 * n), [n], gap, ("one row holds everything", n))
        check_stage(records_in([0, 0, n, 0], rng, span=6 * n), [0, 0, n, 0], gap, ("one row between empty ones", n))


def chain(n, breaks=(), hole=1, width=10, dead=()):
    """n records of `width` positions, each one touching the next -- one span -- but for a hole of `hole` positions in front
    of every record in `breaks`; the records in `dead` are empty (start == end) where they would have stood"""
    i = np.arange(n, dtype=np.int64)
    shift = np.zeros(n, dtype=np.int64)
    for b in breaks:
        shift[b:] += hole
    st = i * width + shift
    en = st + width
    en[list(dead)] = st[list(dead)]
    return np.stack([i, st, en], axis=1).astype(np.uint64)


def test_stage_spans_and_tile_boundaries():
    n = 3 * T
    ro, spans = check_stage(chain(n), [n], 0, "all records one chain: one span over three whole tiles")
    assert spans.tolist() == [[0, 10 * n]] and ro.tolist() == [0, 1]
    for gap in (0, 3):
        hole = gap + 1
        for breaks, what in (([T], "a span closes on a tile's last record, the next opens on a tile's first"),
                             ([T - 1], "the chain breaks one record before the boundary"),
                             ([T + 1], "the chain breaks one record behind the boundary"),
                             ([T - 1, T, T + 1], "three breaks around the boundary: spans of one record"),
                             ([T, 2 * T], "a span that is exactly the middle tile"),
                             ([1, n - 1], "the first and the last record alone"),
                             (list(range(1, n)), "every record a span")):
            ro, spans = check_stage(chain(n, breaks, hole), [n], gap, what)
            assert len(spans) == len(breaks) + 1, what
            if gap:  # a hole of exactly the gap does not break
                ro, spans = check_stage(chain(n, breaks, gap), [n], gap, (what, "the hole is the gap"))
                assert len(spans) == 1
    # the same chains cut into rows on and beside the boundary: nothing joins across rows
    for counts in ([T, 2 * T], [T - 1, 2 * T + 1], [T + 1, 2 * T - 1], [T, T, T], [T - 1, 2, 2 * T - 1]):
        ro, spans = check_stage(chain(n), counts, GAP_MAX, ("one chain, cut into rows", counts))
        assert len(spans) == len(counts)


def test_stage_a_record_that_reaches_back_across_tiles():
    """ordered by end, a long record comes LAST and starts first: its start is the span's, tiles before it learn it from
    the carry"""
    n = 3 * T + 7
    for at in (T, T + 1, 2 * T - 1, 2 * T, n - 1):  # where the long record stands
        rec = chain(n, breaks=list(range(1, n)), hole=5)  # every record a span of its own ...
        first = 2 * T // 3
        rec[at, 1] = rec[first, 1] + 3                   # ... but for the one at `at`, which starts inside record `first`
        ro, spans = check_stage(rec, [n], 0, ("a record reaches back", at), definition=sweep)
        assert len(spans) == n - (at - first)
        # cut into rows in front of the long record: it reaches back to its row's first record only
        check_stage(rec, [T - 3, n - T + 3], 0, ("a record reaches back, two rows", at), definition=sweep)


def test_stage_a_carry_through_more_tiles_than_one_step_of_the_carry_kernel():
    """k_span_carry takes SPANS_CARRY_THREADS * SPANS_CARRY_PER tiles at a step, from the last tile down: with three tiles
    more than one step the last record reaches back into the first tile, through every thread's tiles and from one step into
    the next; then the same records with a row boundary in the middle, which stops the carry there"""
    c = hip_constants("spans.hpp", ("SPANS_CARRY_THREADS", "SPANS_CARRY_PER"))
    piece = c["SPANS_CARRY_THREADS"] * c["SPANS_CARRY_PER"]
    n = (piece + 2) * T + 5
    i = np.arange(n, dtype=np.uint64)
    rec = np.stack([i, i * np.uint64(15), i * np.uint64(15) + np.uint64(10)], axis=1)  # every record a span of its own ...
    first = T // 2
    rec[n - 1, 1] = rec[first, 1] + np.uint64(3)                                        # ... but for the last, which starts in tile 0
    ro, spans = check_stage(rec, [n], 0, "a record reaches back over every tile")
    assert len(spans) == first + 1 and spans[-1].tolist() == [15 * first, 15 * (n - 1) + 10]
    cut = (piece // 2) * T + 7
    ro, spans = check_stage(rec, [cut, n - cut], 0, "a row boundary stops the carry")
    assert ro.tolist() == [0, cut, cut + 1]


def test_stage_rows_and_tile_boundaries():
    rng = np.random.default_rng(7)
    for counts, what in (([T, T, 5], "a row boundary on a tile's last record"),
                         ([T - 1, 1, T - 1, 1, 3], "rows of one record that are a tile's last record"),
                         ([1, T - 1, 1, T - 1, 3], "rows of one record that are a tile's first record"),
                         ([T - 5, 2 * T + 10, 7], "a row whose records span three tiles"),
                         ([3 * T], "one row of exactly three tiles"),
                         ([1] * T + [3], "a tile of one-record rows"),
                         ([T, 0, T], "an empty row on a tile boundary"),
                         ([T, 0, 0, 0, 1], "empty rows on a tile boundary, one record behind them"),
                         ([0, 0, T, 0, 0, T, 0], "empty rows on every boundary and at both ends"),
                         ([0], "one row, no record"), ([0, 0, 0, 5, 0, 0], "empty rows at both ends")):
        for gap in (0, 4, GAP_MAX):
            check_stage(records_in(counts, rng, span=[max(6 * c, 50) for c in counts]), counts, gap, what)
    # rows whose records are all empty, between rows that have spans
    counts = [5, T, 3, T + 9, 2]
    rec = records_in(counts, rng, span=30, lengths=(0,), empties=0)
    rec[:5], rec[5 + T:8 + T], rec[-2:] = chain(5), chain(3), chain(2)
    ro, spans = check_stage(rec, counts, 0, "rows of empty records only")
    assert ro.tolist() == [0, 1, 1, 2, 2, 3]
    # 100 000 empty rows between two records (more than a tile has slots or a workgroup threads), at the start and at the end
    many = 100_000
    for counts, what in (([1] + [0] * many + [1], "between two records"), ([0] * many + [2, 3], "at the start"),
                         ([2, 3] + [0] * many, "at the end"), ([T] + [0] * many + [T], "between two tiles")):
        for gap in (0, GAP_MAX):
            ro, spans = check_stage(records_in(counts, rng, span=40, empties=0), counts, gap, what)
            assert len(ro) == len(counts) + 1 and ro[-1] == len(spans)


@pytest.mark.parametrize("rows", [S - 1, S, S + 1, S * S + 1])
def test_stage_row_counts_around_the_scans_levels(rows):
    rng = np.random.default_rng(rows)
    counts = np.zeros(rows, dtype=np.int64)
    some = rng.choice(rows, size=min(rows, 3000), replace=False)
    counts[some] = rng.choice([1, 1, 2, 5, 40], size=len(some))
    counts[[0, rows - 1]] = 3  # (the first and the last row)
    check_stage(records_in(counts, rng, span=120), counts, 1, ("rows", rows))


def test_stage_empty_nested_and_identical_records_on_a_seam():
    n = 2 * T + 90
    for seam in (T, 2 * T):
        for dead in ([seam - 1], [seam], [seam - 1, seam], [seam - 2, seam - 1, seam, seam + 1], list(range(seam - 40, seam + 40))):
            # empty records join nothing: they leave ONE hole of their width in the chain, which the gap may bridge
            ro, spans = check_stage(chain(n, dead=dead), [n], 0, ("empty records inside a chain", seam, dead))
            assert len(spans) == 2, (seam, dead)
            ro, spans = check_stage(chain(n, dead=dead), [n], 10 * len(dead) - 1, ("the hole - 1", seam, dead))
            assert len(spans) == 2, (seam, dead)
            ro, spans = check_stage(chain(n, dead=dead), [n], 10 * len(dead), ("the gap bridges the empty records", seam, dead))
            assert len(spans) == 1, (seam, dead)
            ro, spans = check_stage(chain(n, dead=dead), [seam, n - seam], 10 * len(dead), ("empty records, a row boundary on the seam", seam, dead))
            assert len(spans) == 2
        # identical records and nested ones (ordered by end: the inner first) across the seam
        rec = chain(n, breaks=list(range(1, n)), hole=100)
        rec[seam - 3:seam + 3, 1:] = rec[seam - 3, 1:]
        ro, spans = check_stage(rec, [n], 0, ("identical records across the seam", seam), definition=sweep)
        assert len(spans) == n - 5
        rec = chain(n, breaks=list(range(1, n)), hole=100)
        lo, hi = int(rec[seam - 4, 1]), int(rec[seam - 4, 2])
        for k in range(8):  # record seam - 4 + k holds every one before it
            rec[seam - 4 + k, 1:] = (lo + 40 - 5 * k, hi + 40 + 5 * k)
        ro, spans = check_stage(rec, [n], 0, ("nested records across the seam", seam), definition=sweep)
        assert len(spans) == n - 7 and [lo + 5, hi + 75] in spans.tolist()


@pytest.mark.parametrize("gap", [0, 1, 6, 7, GAP_MAX])
def test_stage_gaps_around_the_hole(gap):
    """holes of exactly 7 between the groups of a row: gap 6 keeps them apart, gap 7 joins them; 2^63 - 1 leaves one span per
    row that has a live record, and nothing joins across rows"""
    rng = np.random.default_rng(gap % 97)
    counts = ragged_counts(2 * T + 77, rng, (0, 1, 2, 9, 300))
    rec, groups = [], []
    for c in counts:
        breaks = sorted(set(int(x) for x in rng.integers(1, max(c, 2), size=c // 3))) if c > 1 else []
        rec.append(chain(c, breaks, hole=7, width=3))
        groups.append((len(breaks) + 1) if c else 0)
    rec = np.concatenate(rec)
    ro, spans = check_stage(rec, counts, gap, "holes of 7")
    assert np.array_equal(np.diff(ro), (np.asarray(counts) > 0).astype(np.int64) if gap >= 7 else groups)


def test_stage_words_beyond_32_bits():
    rng = np.random.default_rng(33)
    counts = [T - 1, 0, T + 3, 7]
    for base in ((1 << 32) - 200, 1 << 33, (1 << 62) + 5):
        for gap in (0, 3, GAP_MAX):
            check_stage(records_in(counts, rng, span=[5000, 1, 5000, 30], base=base), counts, gap, ("beyond 2^32", base), definition=sweep)
    # words beyond 2^63 compare as unsigned: no difference wraps
    rec = [[0, 5, 6], [0, (1 << 64) - 3, (1 << 64) - 2]]
    ro, spans = check_stage(rec, [2], GAP_MAX, "beyond 2^63", definition=sweep)
    assert spans.tolist() == [[5, 6], [(1 << 64) - 3, (1 << 64) - 2]]
    ro, spans = check_stage([[0, 1 << 40, (1 << 40) + 1], [0, (1 << 62), (1 << 62) + 1]], [2], (1 << 62) - (1 << 40) - 1, "a gap of 2^62", definition=sweep)
    assert len(spans) == 1


def test_stage_nothing_to_merge_and_bad_arguments():
    for rows in (1, 3, S + 1):
        ro, spans = check_stage([], [0] * rows, 0, "n = 0 with rows")
        assert ro.tolist() == [0] * (rows + 1) and len(spans) == 0
    ro, spans = check_stage([], [], 5, "no row at all")
    assert ro.tolist() == [0]
    # counts that do not sum: ACX_EINVAL, and nothing is written
    d = capi.DeviceBuffer(8 * 4096)
    image = np.full(4096, FRESH, dtype=np.int64)
    image[:2] = (2, 1)                                          # the counts of two rows: 3 records
    image[512:521] = (0, 1, 2, 0, 2, 3, 0, 9, 12)                # the records
    d.upload(image)
    p = d.ptr
    args = dict(d_records=p + 8 * 512, n=3, d_counts=p, n_hay=2, gap=0, d_row_offsets=p + 8 * 1024, d_start=p + 8 * 2048, d_end=p + 8 * 3072)
    for change in (dict(n=4), dict(n=2), dict(n_hay=1), dict(n_hay=0), dict(gap=1 << 63), dict(gap=(1 << 64) - 1), dict(d_records=p + 8 * 512 + 4),
                   dict(d_counts=p + 4), dict(d_start=p + 8 * 2048 + 4), dict(d_end=0), dict(d_start=0), dict(d_row_offsets=0), dict(d_records=0),
                   dict(d_counts=0)):
        with pytest.raises(ValueError) as ei:
            capi.spans_rows_device(**{**args, **change})
        assert ei.value.code == capi.EINVAL, change
        assert np.array_equal(d.download(image.nbytes).view(np.int64), image), ("something was written", change)
    assert capi.spans_rows_device(**args) == 2
    got = d.download(image.nbytes).view(np.int64)
    assert got[1024:1028].tolist() == [0, 1, 2, FRESH] and got[2048:2051].tolist() == [1, 9, FRESH] and got[3072:3075].tolist() == [3, 12, FRESH]
    d.free()


# ---------------------------------------------------------------------------
# end to end through the C ABI against the oracle
# ---------------------------------------------------------------------------
PATS = gen.gen_patterns(500, 3, 9, gen.AZ, 5) + [b"ab", b"abab", b"bab", b"ab", b"abcab", b"cabc"]  # (a copy; patterns that nest and chain)
KINDS = [(0, False), (0, True), (1, False), (2, False)]


def oracle_spans(o, hays, ov, gap, search=None, codepoints=False):
    """the definition from the oracle's matches, row by row -> (row_offsets, (S, 2) uint64).  search: the bytes the oracle
    sees (a case-insensitive handle's folded rows); codepoints: the matches' offsets in characters"""
    ro, out = [0], []
    for i, h in enumerate(hays):
        m = np.asarray(o.find_raw(h if search is None else search[i], overlapping=ov), dtype=np.uint64).reshape(-1, 3)
        if codepoints:
            cp = byte_to_code_point(h)
            m = np.stack([m[:, 0], cp[m[:, 1].astype(np.int64)], cp[m[:, 2].astype(np.int64)]], axis=1)
        _, s = sweep_np(m, [len(m)], gap)
        out.append(s)
        ro.append(ro[-1] + len(s))
    return np.asarray(ro, dtype=np.int64), (np.concatenate(out) if out else np.zeros((0, 2), dtype=np.uint64))


def download_words(ptr, n):
    out = np.empty(n, dtype=np.int64)
    if n:
        capi._check(capi.lib().acx_device_download(out.ctypes.data, ptr, 8 * n))
    return out


def check_spans(r, want, on_device, batch=True, what=None):
    """a capi.DeviceSpans against the definition, through the copies and through the raw addresses"""
    want_ro, want_sp = want
    assert r.on_device == on_device and r.count == len(want_sp) and r.rows == (len(want_ro) - 1 if batch else 0), (what, r.count, len(want_sp), r.rows)
    got = np.stack([r.start(), r.end()], axis=1).view(np.uint64).reshape(-1, 2)
    if not np.array_equal(got, want_sp):
        bad = int(np.flatnonzero((got != want_sp).any(axis=1))[0])
        raise AssertionError((what, "first difference at span", bad, got[max(bad - 2, 0):bad + 3].tolist(), want_sp[max(bad - 2, 0):bad + 3].tolist()))
    if batch:
        assert np.array_equal(r.row_offsets(), want_ro), what
    else:
        assert r.row_offsets() is None and r.data_ptr(capi.SPAN_ROW_OFFSETS) == 0, what
    for which, words in ((capi.SPAN_START, want_sp[:, 0]), (capi.SPAN_END, want_sp[:, 1])) + (((capi.SPAN_ROW_OFFSETS, want_ro),) if batch else ()):
        p = r.data_ptr(which)
        assert p and p % 8 == 0, what  # (an empty part still has an address)
        raw = download_words(p, len(words)) if on_device else np.ctypeslib.as_array((capi.ctypes.c_int64 * max(len(words), 1)).from_address(p))[:len(words)]
        assert np.array_equal(raw.view(np.uint64), np.asarray(words).view(np.uint64)), (what, which)
    r.free()


def batch_with_empties(pats, n_hay, seed):
    """n_hay haystacks of 0 .. 3000 bytes: empty ones in front, in the middle (two in a row) and at the end, some without a
    match (the shape of tests/test_gpu_mask.py's)"""
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


class OnDevice:
    """the batch behind one another in HBM at `off` modulo 16, ragged offsets on the device"""

    def __init__(self, hays, off=0):
        blob = b"".join(hays)
        offs = np.concatenate([[0], np.cumsum([len(h) for h in hays])]).astype(np.uint64)
        self.blob = blob
        self.lead = off
        self.hay = capi.DeviceBuffer(len(blob) + 32).upload(np.frombuffer(b"\xa5" * off + blob, dtype=np.uint8))
        self.off = capi.DeviceBuffer(8 * len(offs)).upload(offs)
        self.args = (self.hay.ptr + off, len(blob))
        self.kw = dict(d_offsets=self.off.ptr, n_hay=len(hays))

    def free(self):
        got = self.hay.download(self.lead + len(self.blob))  # (the caller's bytes stay the caller's)
        assert got[self.lead:].tobytes() == self.blob and (got[:self.lead] == 0xA5).all()
        self.hay.free()
        self.off.free()


@pytest.mark.parametrize("mk,ov", KINDS)
def test_spans_parity_host_and_device_inputs(mk, ov):
    o = Oracle(PATS, mk, KIND_DFA)
    a = capi.Automaton(PATS, mk)
    for n_hay in (1, 65, 323):
        hays = batch_with_empties(PATS, n_hay, 100 + n_hay)
        for gap in (0, 64):
            want = oracle_spans(o, hays, ov, gap)
            assert n_hay == 1 or len(want[1])
            check_spans(a.spans(hays, ov, gap=gap), want, False, what=(mk, ov, n_hay, gap))
            for off in (0, 5):
                d = OnDevice(hays, off)
                check_spans(a.spans_device(*d.args, overlapping=ov, gap=gap, **d.kw), want, True, what=(mk, ov, n_hay, off, gap))
                d.free()
    # a uniform batch on the device, and the same bytes as a host batch
    L, nh = 512, 130
    full = gen.gen_textlike(L * nh, 61, PATS).tobytes()
    hays = [full[i * L:(i + 1) * L] for i in range(nh)]
    dev = capi.DeviceBuffer(len(full)).upload(np.frombuffer(full, dtype=np.uint8))
    for gap in (0, 1, 9):
        want = oracle_spans(o, hays, ov, gap)
        check_spans(a.spans_device(dev.ptr, len(full), n_hay=nh, uniform_len=L, overlapping=ov, gap=gap), want, True, what="uniform")
        check_spans(a.spans(hays, ov, gap=gap), want, False, what="uniform, host")
    assert dev.download().tobytes() == full
    dev.free()
    a.close()


def test_spans_overlapping_patterns_that_nest_and_chain_and_copies():
    pats = [b"abcd", b"bc", b"cdef", b"bc", b"f", b"xabcdefx"]
    o, a = Oracle(pats, 0, KIND_DFA), capi.Automaton(pats, 0)
    hays = [b"xabcdefx", b"bcbc", b"", b"abcdxcdef", b"zzz", b"bc" * 3000 + b"q" + b"abcdef" * 500]
    plain, union = oracle_spans(o, hays, False, 0), oracle_spans(o, hays, True, 0)
    assert union[1][0].tolist() == [0, 8] and plain[1][:2].tolist() != union[1][:2].tolist()
    for ov, want in ((False, plain), (True, union)):
        check_spans(a.spans(hays, ov), want, False, what=ov)
        d = OnDevice(hays, 3)
        check_spans(a.spans_device(*d.args, overlapping=ov, **d.kw), want, True, what=ov)
        d.free()
        for gap in (1, 2):
            d = OnDevice(hays, 1)
            check_spans(a.spans_device(*d.args, overlapping=ov, gap=gap, **d.kw), oracle_spans(o, hays, ov, gap), True, what=(ov, gap))
            d.free()
    a.close()


def test_spans_one_haystack_that_is_no_batch_empty_batches_and_errors():
    o, a = Oracle(PATS, 0, KIND_DFA), capi.Automaton(PATS, 0)
    for hay in (gen.gen_textlike(5000, 3, PATS).tobytes(), gen.gen_textlike(300_000, 4, PATS).tobytes(), b"0123" * 100, b""):
        for ov, gap in ((False, 0), (True, 0), (False, 7)):
            want = oracle_spans(o, [hay], ov, gap)
            dev = capi.DeviceBuffer(len(hay) + 16).upload(np.frombuffer(hay + b"\0", dtype=np.uint8))
            check_spans(a.spans(None, ov, gap=gap, single=hay), want, False, batch=False, what=("single", len(hay), gap))
            check_spans(a.spans_device(dev.ptr, len(hay), overlapping=ov, gap=gap), want, True, batch=False, what=("single, device", len(hay), gap))
            dev.free()
    none = (np.zeros(1, dtype=np.int64), np.zeros((0, 2), dtype=np.uint64))
    check_spans(a.spans([], gap=3), none, False, what="empty batch")
    check_spans(a.spans([b"", b""]), (np.zeros(3, dtype=np.int64), none[1]), False, what="empty rows only")
    dev = capi.DeviceBuffer(64)
    check_spans(a.spans_device(dev.ptr, 0, n_hay=0, uniform_len=8), none, True, what="empty batch, device")
    for call in (lambda: a.spans([b"ab"], gap=1 << 63), lambda: a.spans_device(dev.ptr, 0, n_hay=0, uniform_len=8, gap=1 << 63),
                 lambda: a.spans_device(dev.ptr, 10, n_hay=3, uniform_len=4)):
        with pytest.raises(ValueError) as ei:
            call()
        assert ei.value.code == capi.EINVAL
    for mk in (1, 2):
        b = capi.Automaton([b"ab", b"b"], mk)
        for call in (lambda: b.spans([b"xxabxx"], overlapping=True), lambda: b.spans(None, overlapping=True, single=b"ab"),
                     lambda: b.spans_device(0, 0, n_hay=0, uniform_len=8, overlapping=True)):
            with pytest.raises(ValueError) as ei:
                call()
            assert ei.value.code == capi.EOVERLAP
        b.close()
    dev.free()
    a.close()


def test_spans_case_insensitive_handle():
    pats = [b"Needle", b"hay", b"STACK"]
    o = Oracle([p.translate(FOLD) for p in pats], 1, KIND_DFA)
    hays = [b"a nEEdle in a HayStack; " * 3, b"Nothing Here", b"", b"NEEDLE", b"x" * 5000 + b"hAY", b"NO", b"needle HAY stack Xyz" * 900]
    folded = [h.translate(FOLD) for h in hays]
    a = capi.Automaton(pats, 1, ascii_case_insensitive=True)
    for gap in (0, 1):
        want = oracle_spans(o, hays, False, gap, search=folded)
        assert want[1][:2].tolist() == [[2, 8], [14, 22]]  # ("hay" and "stack" touch)
        check_spans(a.spans(hays, gap=gap), want, False, what=gap)
        d = OnDevice(hays, 5)
        check_spans(a.spans_device(*d.args, gap=gap, **d.kw), want, True, what=gap)
        d.free()
    a.close()


def test_spans_in_code_points():
    """codepoints = 1: the offsets find_matches_as_indexes reports for a str, with 2-, 3- and 4-byte characters"""
    pats = ["é", "€uro", "\U0001F600", "ab", "naïve", "日本"]
    raw_pats = [p.encode() for p in pats]
    hays = ["café ab €uro \U0001F600!", "", "naïve 日本語 naive", "ascii ab only", "ééé\U0001F600\U0001F600€uro", "€ur", "é€\U0001F600" * 700 + "ab"]
    raw = [h.encode() for h in hays]
    for mk, ov in ((0, False), (0, True), (2, False)):
        o, a = Oracle(raw_pats, mk, KIND_DFA), capi.Automaton(raw_pats, mk)
        for gap in (0, 1, 2):
            want = oracle_spans(o, raw, ov, gap, codepoints=True)
            in_bytes = oracle_spans(o, raw, ov, gap)
            assert not np.array_equal(want[1], in_bytes[1])
            check_spans(a.spans(raw, ov, True, gap), want, False, what=("code points", mk, ov, gap))
            d = OnDevice(raw, 3)
            check_spans(a.spans_device(*d.args, overlapping=ov, codepoints=True, gap=gap, **d.kw), want, True, what=("code points, device", mk, ov, gap))
            check_spans(a.spans_device(*d.args, overlapping=ov, gap=gap, **d.kw), in_bytes, True, what=("bytes, device", mk, ov, gap))
            d.free()
        one = raw[-1]
        dev = capi.DeviceBuffer(len(one) + 16).upload(np.frombuffer(one, dtype=np.uint8))
        want = oracle_spans(o, [one], ov, 0, codepoints=True)
        check_spans(a.spans(None, ov, True, single=one), want, False, batch=False, what="single, code points")
        check_spans(a.spans_device(dev.ptr, len(one), overlapping=ov, codepoints=True), want, True, batch=False, what="single, code points, device")
        dev.free()
        a.close()


def test_spans_of_a_find_cut_into_byte_ranges(monkeypatch):
    o, a = Oracle(PATS, 0, KIND_DFA), capi.Automaton(PATS, 0)
    hay = gen.gen_textlike(3_000_000, 17, PATS).tobytes()
    dev = capi.DeviceBuffer(len(hay)).upload(np.frombuffer(hay, dtype=np.uint8))
    monkeypatch.setenv("ACX_CHUNK_BYTES", "700001")
    a.path_stats(reset=True)
    for ov in (False, True):
        check_spans(a.spans_device(dev.ptr, len(hay), overlapping=ov), oracle_spans(o, [hay], ov, 0), True, batch=False, what=("cut", ov))
    check_spans(a.spans_device(dev.ptr, len(hay), gap=16), oracle_spans(o, [hay], False, 16), True, batch=False, what="cut, gap")
    st = a.path_stats()
    monkeypatch.delenv("ACX_CHUNK_BYTES")
    assert st["byte_ranges"] >= 2, st
    dev.free()
    a.close()


def test_spans_of_a_batch_cut_over_the_occurrence_limit(monkeypatch):
    # the batch of test_gpu_chunked.py: one pass may index 50 000 occurrences, the batch is cut at haystack boundaries
    pats = [b"ab", b"b", b"bab"]
    r = random.Random(5)
    hs = [b"ab" * r.randint(1, 60_000) + bytes(r.choice(b"abc") for _ in range(r.randint(0, 300))) for _ in range(7)] + [b"", b"abab"]
    for mk in (0, 1):
        a, o = capi.Automaton(pats, mk), Oracle(pats, mk, KIND_DFA)
        want = oracle_spans(o, hs, False, 0)
        monkeypatch.setenv("ACX_MAX_OCC", "50000")
        monkeypatch.setenv("ACX_NO_BUCKET", "1")
        d = OnDevice(hs, 5)
        a.path_stats(reset=True)
        check_spans(a.spans_device(*d.args, **d.kw), want, True, what=("max_occ", mk))
        st = a.path_stats()
        monkeypatch.delenv("ACX_MAX_OCC")
        monkeypatch.delenv("ACX_NO_BUCKET")
        assert st["byte_ranges"] >= 2, st
        d.free()
        a.close()


def test_spans_of_a_find_on_the_dense_path():
    pats = gen.gen_patterns(2000, 5, 12, gen.AZ, 1)
    a, o = capi.Automaton(pats, 0, capi.IMPL_DFA), Oracle(pats, 0, KIND_DFA)
    every = bytearray(gen.gen_uniform(8 << 20, gen.AZ, 13).tobytes())  # (the size tests/test_gpu_filter.py uses)
    rng = gen.SplitMix64(77)
    for k in range(0, len(every) - 32, 32):
        if (k >> 16) % 3 == 0 and k % 4096:  # (every third row keeps a handful of plants only)
            continue
        p = pats[rng.next() % len(pats)]
        every[k:k + len(p)] = p
    every = bytes(every)
    L = 1 << 16
    hays = [every[i:i + L] for i in range(0, len(every), L)]
    dev = capi.DeviceBuffer(len(every)).upload(np.frombuffer(every, dtype=np.uint8))
    a.path_stats(reset=True)
    want = oracle_spans(o, [every], False, 0)
    for _ in range(2):  # (one haystack that is no batch: the call tests/test_gpu_columns.py sees take that path)
        check_spans(a.spans_device(dev.ptr, len(every)), want, True, batch=False, what="dense, one row")
    st = a.path_stats()
    assert st["hot_calls"] + st["dense_tiles"] + st["dense_radix"] >= 2, st
    check_spans(a.spans_device(dev.ptr, len(every), n_hay=len(hays), uniform_len=L, gap=24), oracle_spans(o, hays, False, 24), True, what="dense, gap 24")
    dev.free()
    a.close()


def test_eight_threads_on_one_handle():
    a, o = capi.Automaton(PATS, 0), Oracle(PATS, 0, KIND_DFA)
    work = []
    for t in range(8):
        hays = batch_with_empties(PATS, 40 + 9 * t, 300 + t) + [gen.gen_textlike(150_000, t, PATS).tobytes()]
        work.append((hays, oracle_spans(o, hays, False, 0), oracle_spans(o, hays, True, 5)))
    errors = []

    def run(t):
        try:
            hays, want, want5 = work[t]
            for i in range(3):
                check_spans(a.spans(hays), want, False, what=t)
                d = OnDevice(hays, t)
                check_spans(a.spans_device(*d.args, **d.kw), want, True, what=t)
                check_spans(a.spans_device(*d.args, overlapping=True, gap=5, **d.kw), want5, True, what=t)
                d.free()
        except BaseException as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=run, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    a.close()


def test_seeded_random_batches():
    rng = random.Random(20261020)
    made = {}  # (a handle and an oracle per set of patterns and match kind: the cases are about the data)
    for case in range(200):
        mk = rng.choice([0, 0, 1, 2])
        ov = mk == 0 and rng.random() < 0.5
        alpha = rng.choice([b"ab", b"abcd", gen.AZ])
        key = (mk, alpha, rng.choice([1, 3, 40]))
        if key not in made:
            pats = gen.gen_patterns(key[2], 1, 2 + 2 * key[2] % 11, alpha, 1000 + len(made))
            made[key] = (capi.Automaton(pats, mk), Oracle(pats, mk, KIND_DFA))
        a, o = made[key]
        text_ = rng.choice([alpha, alpha + b"xyz", alpha + b"0123456789" * 3])
        n_hay = rng.choice([1, 2, 7, 64, 65])
        hays = [bytes(rng.choices(text_, k=rng.choice([0, 0, 1, 9, 200, 2000]))) for _ in range(n_hay)]
        gap = rng.choice([0, 0, 1, 2, 5, 64, GAP_MAX])
        want = oracle_spans(o, hays, ov, gap)
        route = rng.choice(["host", "device", "device"])
        what = (case, mk, ov, n_hay, route, gap)
        try:
            if route == "device":
                d = OnDevice(hays, rng.randrange(16))
                check_spans(a.spans_device(*d.args, overlapping=ov, gap=gap, **d.kw), want, True, what=what)
                d.free()
            else:
                check_spans(a.spans(hays, ov, gap=gap), want, False, what=what)
        except AssertionError as e:
            raise AssertionError(f"case {what}: {e}") from e
    for a, _ in made.values():
        a.close()


# ---------------------------------------------------------------------------
# the Python methods: sequences of host objects (tensors in HBM and torch as the consumer: the script below)
# ---------------------------------------------------------------------------
def matchkind(ar, mk):
    return (ar.MatchKind.Standard, ar.MatchKind.LeftmostFirst, ar.MatchKind.LeftmostLongest)[mk]


def as_lists(want):
    ro, sp = want
    flat = [tuple(x) for x in sp.tolist()]
    return [flat[ro[h]:ro[h + 1]] for h in range(len(ro) - 1)]


def check_match_spans(ms, want, batch=True):
    """a MatchSpans in host memory against the definition"""
    ro, sp = want
    assert len(ms) == len(sp) and ms.device is None
    assert ms.tolist() == (as_lists(want) if batch else [tuple(x) for x in sp.tolist()])
    assert len(ms.start) == len(ms.end) == len(sp) and ms.start.__dlpack_device__() == (1, 0)
    for col, words in ((ms.start, sp[:, 0]), (ms.end, sp[:, 1])):
        got = np.from_dlpack(col)
        assert got.dtype == np.int64 and np.array_equal(got.view(np.uint64), words)
        mv = memoryview(col)
        assert mv.format == "q" and mv.readonly and np.array_equal(np.asarray(mv).view(np.uint64), words)
    if batch:
        assert len(ms.row_offsets) == len(ro) and np.array_equal(np.from_dlpack(ms.row_offsets), ro)
    else:
        assert ms.row_offsets is None


@pytest.mark.parametrize("mk,ov", KINDS)
def test_python_sequences_both_classes(mk, ov):
    import ahocorasick_rs as ar
    o = Oracle(PATS, mk, KIND_DFA)
    b = ar.BytesAhoCorasick(PATS, matchkind=matchkind(ar, mk))
    s = ar.AhoCorasick([p.decode() for p in PATS], matchkind=matchkind(ar, mk))
    for n_hay in (0, 1, 64, 130):
        hays = batch_with_empties(PATS, n_hay, 500 + n_hay)
        strs = [h.decode() for h in hays]
        for gap in (0, 12):
            want = oracle_spans(o, hays, ov, gap)
            check_match_spans(b.cover_spans_batch(hays, overlapping=ov, gap=gap), want)
            check_match_spans(b.cover_spans_batch(tuple(bytearray(h) for h in hays), ov, gap=gap), want)
            check_match_spans(s.cover_spans_batch(strs, ov, gap=gap), want)
            rows = as_lists(want)
            for h, row in list(zip(hays, rows))[:40]:  # the single forms agree with tolist()
                assert b.cover_spans(h, overlapping=ov, gap=gap).tolist() == row and s.cover_spans(h.decode(), ov, gap=gap).tolist() == row
    one = gen.gen_textlike(20_000, 9, PATS).tobytes()
    check_match_spans(b.cover_spans(one, ov), oracle_spans(o, [one], ov, 0), batch=False)
    check_match_spans(b.cover_spans(np.frombuffer(one, dtype=np.uint8), ov, gap=3), oracle_spans(o, [one], ov, 3), batch=False)
    check_match_spans(s.cover_spans(one.decode(), ov, gap=3), oracle_spans(o, [one], ov, 3), batch=False)


def test_python_str_gives_character_indexes():
    import ahocorasick_rs as ar
    pats = ["é", "€uro", "\U0001F600", "ab", "naïve", "日本"]
    s = ar.AhoCorasick(pats, matchkind=ar.MatchKind.LeftmostLongest)
    o = Oracle([p.encode() for p in pats], 2, KIND_DFA)
    hays = ["café ab €uro \U0001F600!", "", "naïve 日本語 naive", "ascii ab only", "ééé\U0001F600\U0001F600€uro", "€ur"]
    raw = [h.encode() for h in hays]
    for gap in (0, 1):
        want = oracle_spans(o, raw, False, gap, codepoints=True)
        check_match_spans(s.cover_spans_batch(hays, gap=gap), want)
        for h, row in zip(hays, as_lists(want)):
            assert s.cover_spans(h, gap=gap).tolist() == row, h
            # what the spans are for: the characters they cut out are the matches' own
            assert all(any(p in h[a:e] for p in pats) for a, e in row)
    assert s.cover_spans("café ab €uro \U0001F600!").tolist() == [(3, 4), (5, 7), (8, 12), (13, 14)]
    assert s.cover_spans("café ab €uro \U0001F600!", gap=1).tolist() == [(3, 14)]
    # a host tensor of the same UTF-8 bytes: byte offsets local to the row
    flat = np.frombuffer(b"".join(raw), dtype=np.uint8).copy()
    cuts = np.concatenate([[0], np.cumsum([len(r) for r in raw])]).astype(np.int64)
    assert s.cover_spans_batch(flat, offsets=cuts).tolist() == as_lists(oracle_spans(o, raw, False, 0))


def test_python_errors_and_host_tensors():
    import ahocorasick_rs as ar
    b, s = ar.BytesAhoCorasick([b"ab", b"c"]), ar.AhoCorasick(["ab", "c"])
    for call in (lambda: b.cover_spans(b"ab", gap=-1), lambda: s.cover_spans("ab", gap=1 << 63), lambda: b.cover_spans_batch([b"ab"], gap=-5),
                 lambda: s.cover_spans_batch(["ab"], gap=1 << 64)):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: b.cover_spans(b"ab", gap=True), lambda: s.cover_spans("ab", gap=1.5), lambda: b.cover_spans(b"ab", False, 3),
                 lambda: b.cover_spans_batch([b"ab"], False, 3), lambda: b.cover_spans(b"ab", overlapping=1), lambda: b.cover_spans("ab"),
                 lambda: s.cover_spans(b"ab"), lambda: b.cover_spans_batch([b"ab"], row_length=2), lambda: b.cover_spans(b"ab", row_length=2),
                 lambda: b.cover_spans_batch([b"ab"], gap=None), lambda: b.cover_spans_batch([b"ab"], offsets=np.array([0, 2], dtype=np.int64))):
        with pytest.raises(TypeError):
            call()
    assert b.cover_spans(b"xxabxcx").tolist() == [(2, 4), (5, 6)] and s.cover_spans("xxabxcx", gap=1).tolist() == [(2, 6)]
    got = b.cover_spans_batch([b"abab", b"", b"xcxxc"], gap=0)
    assert got.tolist() == [[(0, 4)], [], [(1, 2), (4, 5)]] and got.device is None and len(got) == 3
    assert b.cover_spans_batch([b"abab", b"", b"xcxxc"], gap=GAP_MAX).tolist() == [[(0, 4)], [], [(1, 5)]]
    t = np.frombuffer(b"abxcYxabab", dtype=np.uint8).copy()
    ms = b.cover_spans_batch(t, row_length=5)
    assert ms.tolist() == [[(0, 2), (3, 4)], [(1, 5)]] and np.array_equal(np.from_dlpack(ms.row_offsets), [0, 2, 3])
    ms = b.cover_spans_batch(t, gap=1, offsets=np.array([0, 1, 1, 6, 10], dtype=np.int64))
    assert ms.tolist() == [[], [], [(2, 3)], [(0, 4)]] and np.array_equal(np.from_dlpack(ms.row_offsets), [0, 0, 0, 1, 2])
    assert s.cover_spans_batch(t, row_length=2).tolist() == [[(0, 2)], [(1, 2)], [], [(0, 2)], [(0, 2)]]
    assert t.tobytes() == b"abxcYxabab"
    empty = b.cover_spans(b"")
    assert len(empty) == 0 and empty.tolist() == [] and empty.row_offsets is None and len(np.from_dlpack(empty.start)) == 0
    for mk in (ar.MatchKind.LeftmostFirst, ar.MatchKind.LeftmostLongest):
        for call in (lambda x: x.cover_spans(b"ab", overlapping=True), lambda x: x.cover_spans_batch([b"ab"], overlapping=True)):
            with pytest.raises(ValueError):
                call(ar.BytesAhoCorasick([b"ab"], matchkind=mk))
    assert ar.BytesAhoCorasick([b"abc", b"bcd"]).cover_spans(b"abcd", overlapping=True).tolist() == [(0, 4)]
    assert ar.BytesAhoCorasick([b"abc", b"bcd"]).cover_spans(b"abcd").tolist() == [(0, 3)]
    assert ar.BytesAhoCorasick([b"NeEdLe"], ascii_case_insensitive=True).cover_spans(b"A nEEdle, a Needle", gap=4).tolist() == [(2, 18)]
    with pytest.raises(TypeError):
        ar.MatchSpans()


def mask_runs(mask, offsets):
    """the maximal runs of ones of a 0 / 1 mask, cut by the rows' offsets, in numpy -> (row_offsets, (S, 2)) local to the rows"""
    m = np.asarray(mask, dtype=np.uint8).astype(bool)
    offsets = np.asarray(offsets, dtype=np.int64)
    prev, nxt = np.concatenate([[False], m]), np.concatenate([m, [False]])  # the byte before position i, the byte at it
    first = np.zeros(len(m) + 1, dtype=bool)
    first[offsets] = True  # a run that crosses a row's first byte is two
    st, en = np.flatnonzero(nxt & (~prev | first)), np.flatnonzero(prev & (~nxt | first))
    row = np.searchsorted(offsets, st, side="right") - 1  # (of several rows that begin at one byte the last: the others are empty)
    ro = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=len(offsets) - 1))]).astype(np.int64)
    return ro, np.stack([st - offsets[row], en - offsets[row]], axis=1).astype(np.uint64)


@pytest.mark.parametrize("ov", [False, True])
def test_the_identity_with_match_mask(ov):
    """for byte inputs and gap = 0 the spans are the runs of ones of match_mask_batch for the same arguments, cut by the rows"""
    import ahocorasick_rs as ar
    pats = PATS + [b"a", b"tt"]  # (short patterns: matches that touch across a row's end)
    b = ar.BytesAhoCorasick(pats)
    hay = np.frombuffer(gen.gen_textlike(300_000, 21, pats).tobytes(), dtype=np.uint8).copy()
    rng = np.random.default_rng(3)
    cuts = np.unique(np.concatenate([[0, len(hay)], rng.integers(0, len(hay), size=900)])).astype(np.int64)
    cuts = np.sort(np.concatenate([cuts, cuts[5:40]]))  # (empty rows)
    mask = np.from_dlpack(b.match_mask_batch(hay, ov, offsets=cuts).data)
    want = mask_runs(mask, cuts)
    assert len(want[1]) > 5000
    ms = b.cover_spans_batch(hay, ov, offsets=cuts)
    assert np.array_equal(np.from_dlpack(ms.row_offsets), want[0])
    assert np.array_equal(np.from_dlpack(ms.start).view(np.uint64), want[1][:, 0]) and np.array_equal(np.from_dlpack(ms.end).view(np.uint64), want[1][:, 1])
    L = 1000
    mask = np.from_dlpack(b.match_mask_batch(hay, ov, row_length=L).data)
    want = mask_runs(mask, np.arange(0, len(hay) + 1, L))
    check_match_spans(b.cover_spans_batch(hay, ov, row_length=L), want)


def test_host_columns_outlive_the_match_spans():
    import ahocorasick_rs as ar
    o, b = Oracle(PATS, 0, KIND_DFA), ar.BytesAhoCorasick(PATS)
    hays = batch_with_empties(PATS, 300, 3)
    want = oracle_spans(o, hays, False, 0)
    ms = b.cover_spans_batch(hays)
    st, mv, ro, unused = np.from_dlpack(ms.start), memoryview(ms.end), np.from_dlpack(ms.row_offsets), ms.start.__dlpack__()
    del ms, unused, hays
    gc.collect()
    for k in range(20):  # (other results come and go where the words would be if they had been freed)
        b.cover_spans_batch(batch_with_empties(PATS, 300, 50 + k), gap=k)
    assert np.array_equal(st.view(np.uint64), want[1][:, 0]) and np.array_equal(np.asarray(mv).view(np.uint64), want[1][:, 1]) and np.array_equal(ro, want[0])


_TENSOR_SCRIPT = r"""
import gc
import sys
import threading
import torch  # first: one process holds ONE HIP runtime, and torch must be the one to load it
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
import gen
from oracle_lib import KIND_DFA, Oracle
import ahocorasick_rs as ar
pats = gen.gen_patterns(300, 5, 9, gen.AZ, 5) + [b"abqab", b"abqabqab", b"bqab", b"abqab", b"a", b"tt"]
L, nh = 4096, 200
hay = gen.gen_textlike(L * nh, 13, pats).copy()
hay[3 * L:9 * L] = 48   # (rows without a match)
hay[50 * L:51 * L] = 48
t = torch.from_numpy(hay.copy()).to("cuda:0")
kinds = (ar.MatchKind.Standard, ar.MatchKind.LeftmostFirst, ar.MatchKind.LeftmostLongest)
lens = [0, 0, 17, L, 3 * L, 5, 0, 2 * L + 1, 4 * L, 7, 0]
lens += [L * nh - sum(lens), 0]
cuts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)

def spans(o, rows, ov, gap):
    # the definition: sort and sweep over every row's matches
    ro, out = [0], []
    for h in rows:
        live = sorted((int(s), int(e)) for _, s, e in o.find_raw(h, overlapping=ov) if s < e)
        mine = []
        for s, e in live:
            if mine and s - mine[-1][1] <= gap:
                mine[-1] = (mine[-1][0], max(mine[-1][1], e))
            else:
                mine.append((s, e))
        out += mine
        ro.append(len(out))
    return ro, out

def check(ms, want, where, batch=True):
    ro, sp = want
    assert ms.device == (0 if where == "device" else None), (where, ms.device)
    assert len(ms) == len(sp)
    st, en = torch.from_dlpack(ms.start), torch.from_dlpack(ms.end)
    for x in (st, en):
        assert x.dtype == torch.int64 and tuple(x.shape) == (len(sp),) and x.is_contiguous()
        assert x.device.type == ("cuda" if where == "device" else "cpu")
    assert st.tolist() == [s for s, _ in sp] and en.tolist() == [e for _, e in sp], where
    if batch:
        r = torch.from_dlpack(ms.row_offsets)
        assert r.dtype == torch.int64 and r.tolist() == ro and r.device.type == st.device.type
        assert ms.tolist() == [sp[ro[h]:ro[h + 1]] for h in range(len(ro) - 1)]
    else:
        assert ms.row_offsets is None and ms.tolist() == sp
    if where == "device":
        # no copy: the tensor IS the column (the same address on every export)
        assert st.device.index == 0 and ms.start.__dlpack_device__() == (10, 0)
        assert torch.from_dlpack(ms.start).data_ptr() == st.data_ptr() and torch.from_dlpack(ms.end).data_ptr() == en.data_ptr()
        if batch:
            assert torch.from_dlpack(ms.row_offsets).data_ptr() == r.data_ptr()
        try:
            memoryview(ms.start)
            raise SystemExit("a device column exported a host buffer")
        except BufferError:
            pass
    return st, en

uni_cuts = np.arange(nh + 1, dtype=np.int64) * L
for mk, ov in ((0, False), (0, True), (1, False), (2, False)):
    o = Oracle(pats, mk, KIND_DFA)
    b = ar.BytesAhoCorasick(pats, matchkind=kinds[mk])
    s = ar.AhoCorasick([p.decode() for p in pats], matchkind=kinds[mk])
    uniform = [hay[i * L:(i + 1) * L].tobytes() for i in range(nh)]
    ragged = [hay[cuts[i]:cuts[i + 1]].tobytes() for i in range(len(lens))]
    d_cuts = torch.from_numpy(cuts).to("cuda:0")
    for gap in ((0, 64) if mk == 0 else (3,)):
        wu, wr = spans(o, uniform, ov, gap), spans(o, ragged, ov, gap)
        for obj in (b, s):
            check(obj.cover_spans_batch(t, overlapping=ov, gap=gap, row_length=L), wu, "device")   # a tensor in HBM: the result stays there
            check(obj.cover_spans_batch(t, ov, gap=gap, offsets=d_cuts), wr, "device")
        check(b.cover_spans_batch(torch.from_numpy(hay), ov, gap=gap, row_length=L), wu, "host")
        check(b.cover_spans_batch(torch.from_numpy(hay), ov, gap=gap, offsets=torch.from_numpy(cuts)), wr, "host")
        check(b.cover_spans_batch(uniform, ov, gap=gap), wu, "host")
        check(b.cover_spans(t, ov, gap=gap), spans(o, [hay.tobytes()], ov, gap), "device", batch=False)   # one tensor that is no batch
        check(b.cover_spans(t[5:5 + 3 * L + 1], ov, gap=gap), spans(o, [hay[5:5 + 3 * L + 1].tobytes()], ov, gap), "device", batch=False)
    # the identity: gap = 0 gives the runs of ones of match_mask_batch for the same arguments, cut by the rows -- in torch
    for kw, offs in ((dict(row_length=L), uni_cuts), (dict(offsets=d_cuts), cuts)):
        m = torch.from_dlpack(b.match_mask_batch(t, ov, **kw).data).to(torch.int8)
        pad = torch.zeros(1, dtype=torch.int8, device=m.device)
        prev, nxt = torch.cat([pad, m]), torch.cat([m, pad])
        first = torch.zeros(len(m) + 1, dtype=torch.bool, device=m.device)
        first[torch.from_numpy(offs).to(m.device)] = True
        opens = (nxt == 1) & ((prev == 0) | first)
        closes = (prev == 1) & ((nxt == 0) | first)
        st_w, en_w = opens.nonzero().flatten(), closes.nonzero().flatten()
        d_offs = torch.from_numpy(offs).to(m.device)
        row = torch.searchsorted(d_offs, st_w, right=True) - 1
        ms = b.cover_spans_batch(t, ov, **kw)
        st, en, ro = (torch.from_dlpack(c) for c in (ms.start, ms.end, ms.row_offsets))
        assert torch.equal(st, st_w - d_offs[row]) and torch.equal(en, en_w - d_offs[row])
        assert torch.equal(ro[1:] - ro[:-1], torch.bincount(row, minlength=len(offs) - 1))
    # the only way before: the columns, sorted and swept in torch
    mc = b.find_matches_as_columns_batch(uniform, overlapping=ov)
    cs, ce, cro = (torch.from_dlpack(c).to("cuda:0") for c in (mc.start, mc.end, mc.row_offsets))
    row = torch.repeat_interleave(torch.arange(nh, device="cuda:0"), cro[1:] - cro[:-1])
    order = torch.argsort(row * L + cs, stable=True)
    gs, ge = (row * (2 * L) + cs)[order], (row * (2 * L) + ce)[order]
    reach = torch.cummax(ge, 0).values
    opens = torch.ones(len(gs), dtype=torch.bool, device="cuda:0")
    opens[1:] = gs[1:] > reach[:-1]
    ms = b.cover_spans_batch(t, ov, row_length=L)
    assert torch.equal(torch.from_dlpack(ms.start), (gs - row[order] * (2 * L))[opens])
    last = torch.cat([opens[1:], torch.ones(1, dtype=torch.bool, device="cuda:0")])
    assert torch.equal(torch.from_dlpack(ms.end), (reach - row[order] * (2 * L))[last])

o, b = Oracle(pats, 0, KIND_DFA), ar.BytesAhoCorasick(pats)
uniform = [hay[i * L:(i + 1) * L].tobytes() for i in range(nh)]
want = spans(o, uniform, False, 0)

# split_rows(t).offsets as offsets=: the rows of a delimited buffer, merged where they lie
lines = hay.copy()
lines[np.random.default_rng(1).integers(0, len(lines), size=3000)] = 10
lt = torch.from_numpy(lines).to("cuda:0")
ro = ar.split_rows(lt)
offs = torch.from_dlpack(ro.offsets).cpu().numpy()
rows = [lines[offs[i]:offs[i + 1]].tobytes() for i in range(len(offs) - 1)]
check(b.cover_spans_batch(lt, gap=2, offsets=ro.offsets), spans(o, rows, False, 2), "device")

# an odd device address; the consumer on a stream of its own
side = torch.cuda.Stream()
odd = [hay[5 + i * L:5 + (i + 1) * L].tobytes() for i in range(100)]
with torch.cuda.stream(side):
    st, en = check(b.cover_spans_batch(t[5:5 + 100 * L], row_length=L), spans(o, odd, False, 0), "device")
    covered = (en - st).sum()
assert int(covered) == sum(e - s for s, e in spans(o, odd, False, 0)[1])

# a case-insensitive handle
ci = ar.BytesAhoCorasick([b"NeEdLe"], ascii_case_insensitive=True)
ct = torch.from_numpy(np.frombuffer(b"A nEEdle, a Needle. " * 50, dtype=np.uint8).copy()).to("cuda:0")
assert ci.cover_spans_batch(ct, row_length=20).tolist() == [[(2, 8), (12, 18)]] * 50
assert ci.cover_spans_batch(ct, gap=4, row_length=20).tolist() == [[(2, 18)]] * 50

# str with multi-byte characters in HBM: byte offsets
sm = ar.AhoCorasick(["é", "€uro", "ab"])
u = "café ab €uro".encode()
ut = torch.from_numpy(np.frombuffer(u * 3, dtype=np.uint8).copy()).to("cuda:0")
r = sm.cover_spans_batch(ut, row_length=len(u))
assert r.tolist() == [[(3, 5), (6, 8), (9, 15)]] * 3 and r.device == 0

def raises(exc, call):
    try:
        call()
    except exc:
        return
    raise SystemExit("no %s" % exc.__name__)
raises(TypeError, lambda: b.cover_spans_batch(t))                                   # neither offsets nor row_length
raises(TypeError, lambda: b.cover_spans_batch(t, row_length=L, offsets=torch.from_numpy(cuts).to("cuda:0")))
raises(ValueError, lambda: b.cover_spans_batch(t, offsets=torch.from_numpy(cuts)))  # offsets on another device
raises(ValueError, lambda: b.cover_spans_batch(t, gap=-1, row_length=L))
raises(ValueError, lambda: b.cover_spans_batch(t, offsets=torch.from_numpy(cuts[:-2].copy()).to("cuda:0")))  # they do not span the tensor
raises(ValueError, lambda: ar.BytesAhoCorasick(pats, matchkind=kinds[1]).cover_spans_batch(t, overlapping=True, row_length=L))
raises(ValueError, lambda: ar.BytesAhoCorasick(pats, matchkind=kinds[1]).cover_spans(t, overlapping=True))

# no rows, and rows without a match: the columns still become tensors
ms = b.cover_spans_batch(torch.zeros(0, dtype=torch.uint8, device="cuda:0"), row_length=7)
assert len(ms) == 0 and ms.tolist() == [] and tuple(torch.from_dlpack(ms.start).shape) == (0,) and torch.from_dlpack(ms.row_offsets).tolist() == [0]
z = torch.full((1 << 20,), 48, dtype=torch.uint8, device="cuda:0")
ms = b.cover_spans_batch(z, row_length=1 << 10)
assert len(ms) == 0 and not torch.from_dlpack(ms.row_offsets).any() and len(ms.row_offsets) == 1025 and tuple(torch.from_dlpack(ms.end).shape) == (0,)
assert len(b.cover_spans(z)) == 0 and b.cover_spans(z).device == 0

# lifetime: the tensors keep the result alive after the MatchSpans object, its handle and its input are gone
b2 = ar.BytesAhoCorasick(pats)
t2 = t.clone()
ms = b2.cover_spans_batch(t2, row_length=L)
st, en, r = torch.from_dlpack(ms.start), torch.from_dlpack(ms.end), torch.from_dlpack(ms.row_offsets)
unused = ms.start.__dlpack__()
del ms, unused, b2, t2
gc.collect()
for k in range(6):  # (other results come and go where the words would be if they had been given back)
    other = torch.from_numpy(gen.gen_textlike(L * nh, 40 + k, pats).copy()).to("cuda:0")
    keep = b.cover_spans_batch(other, gap=k, row_length=L)
    del keep
gc.collect()
torch.cuda.synchronize()
assert st.tolist() == [s for s, _ in want[1]] and en.tolist() == [e for _, e in want[1]] and r.tolist() == want[0]
del st, en, r
gc.collect()

# eight threads on one handle, tensors in HBM
errors = []
def run(i):
    try:
        for k in range(3):
            lo = i * 20 + k
            ms = b.cover_spans_batch(t[lo * L:(lo + 20) * L], row_length=L)
            a, z_ = want[0][lo], want[0][lo + 20]
            assert torch.from_dlpack(ms.start).tolist() == [s for s, _ in want[1][a:z_]], (i, k)
            assert torch.from_dlpack(ms.end).tolist() == [e for _, e in want[1][a:z_]], (i, k)
            assert torch.from_dlpack(ms.row_offsets).tolist() == [x - a for x in want[0][lo:lo + 21]], (i, k)
    except BaseException as e:
        errors.append((i, repr(e)))
threads = [threading.Thread(target=run, args=(i,)) for i in range(8)]
for th in threads:
    th.start()
for th in threads:
    th.join()
assert not errors, errors
assert torch.equal(t.cpu(), torch.from_numpy(hay))
print("OK")
"""


def test_tensors_in_and_torch_out():
    """cover_spans_batch on tensors in HBM with offsets and with row_length, both classes, and cover_spans on one tensor;
    torch.from_dlpack of the three columns on the automaton's device without a copy; the identity with match_mask_batch and
    the sort-and-sweep over the columns, both in torch; split_rows' offsets as offsets=; errors; empty results; lifetime;
    threads.  In a process of its own: torch has to be the first to load the HIP runtime."""
    pytest.importorskip("torch")
    p = subprocess.run([sys.executable, "-c", _TENSOR_SCRIPT, ROOT, os.path.join(ROOT, "tests")], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
