"""The cover of a search's matches, on the device (acx_mask / acx_mask_device / acx_mask_rows_device; mask_all / match_mask
and their _batch forms): the device stage alone at the seams of its tile kernel -- record counts around the tile, every start
residue of a store crossed with every short length, lengths around the threshold of the cooperative sweep and around one
sweep, pointer residues of both buffers, rows that cross tiles, runs of empty rows, row counts around the scan's levels, the
three ways to cut the bytes into rows, clipping, in place, the 0 / 1 form -- with guard bytes around the output and every
input verified unwritten; parity with the definition through the C ABI for every match kind, on host and device inputs, for
finds that were cut or took the dense path; the Python methods with sequences and with tensors in HBM, torch as the consumer,
lifetime, threads and a seeded random loop.  Expected values come from numpy over synthetic records or from the oracle's
matches (tests/oracle_lib.py) and the definition restated below, never from the library; the kernel's seams are read from
its header."""
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
from oracle_lib import KIND_DFA, Oracle

pytestmark = pytest.mark.gpu
capi = pytest.importorskip("ahocorasick_rs_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ahocorasick_rs_amd", "csrc")
FOLD = bytes.maketrans(bytes(range(65, 91)), bytes(range(97, 123)))
ZERO = 1  # ACX_MASK_ZERO


def hip_constants(path, names):
    src = open(os.path.join(CSRC, path)).read()
    out = {}
    for n in names:
        m = re.search(r"\b%s\s*=\s*(\d+)\s*[,;]" % n, src)
        assert m, f"{n} is no longer a plain constant of {path}"
        out[n] = int(m.group(1))
    return out


_C = hip_constants("mask.hpp", ("MASK_THREADS", "MASK_TILE", "MASK_LONG"))
THREADS, T, LONG = _C["MASK_THREADS"], _C["MASK_TILE"], _C["MASK_LONG"]
SWEEP = THREADS * 16  # the bytes one cooperative sweep of a workgroup stores
S = 2048  # replace_scan's items per workgroup (replace.hip RS_THREADS * RS_PER): beyond it the scan has two levels, beyond S * S three
GUARD = 0xC3


def test_constants_are_what_the_sizes_below_assume():
    assert T % THREADS == 0 and THREADS % 64 == 0 and T >= 256 and 34 <= LONG < SWEEP
    src = open(os.path.join(CSRC, "replace.hip")).read()
    assert re.search(r"RS_THREADS = 256, RS_PER = 8\b", src), "the scan's level size is no longer 2048"
    assert capi.MASK_ZERO == ZERO


# ---------------------------------------------------------------------------
# the stage alone
# ---------------------------------------------------------------------------
def definition(hay, offsets, records, counts, fill, flags):
    """out[off[h] + i] = fill where a record of row h, clipped to the row (end' = min(end, row length), start' = min(start,
    end')), has start' <= i < end'; elsewhere the haystack's byte, or 0 with ACX_MASK_ZERO.  offsets: rows + 1 from 0."""
    hay = np.asarray(hay, dtype=np.uint8)
    out = np.zeros(len(hay), dtype=np.uint8) if flags & ZERO else hay.copy()
    rec = np.asarray(records, dtype=np.uint64).reshape(-1, 3)
    if not len(rec):
        return out
    off = np.asarray(offsets, dtype=np.int64)
    row = np.repeat(np.arange(len(counts)), np.asarray(counts, dtype=np.int64))
    assert len(row) == len(rec)
    b, rl = off[row], (off[row + 1] - off[row]).astype(np.uint64)
    e = np.minimum(rec[:, 2], rl)
    s = np.minimum(rec[:, 1], e)
    edge = np.zeros(len(hay) + 1, dtype=np.int64)
    np.add.at(edge, b + s.astype(np.int64), 1)
    np.add.at(edge, b + e.astype(np.int64), -1)
    out[np.cumsum(edge[:-1]) > 0] = fill
    return out


def run_stage(hay, offsets, uniform, records, counts, fill, flags=0, out_res=0, hay_res=0, inplace=False, prefill=0x77):
    """mask_rows_device on synthetic records: the bytes at hay_res modulo 16, cut by `offsets` (rows + 1, on the device), by
    `uniform` (a row length) or by neither (one row); the output at out_res modulo 16 between 64 guard bytes -> the output;
    the guards and every input checked unwritten"""
    hay = np.ascontiguousarray(np.asarray(hay, dtype=np.uint8))
    rec = np.ascontiguousarray(np.asarray(records, dtype=np.uint64).reshape(-1, 3))
    counts = np.ascontiguousarray(np.asarray(counts, dtype=np.uint64))
    n, rows, nb = len(rec), len(counts), len(hay)
    lead = 64 + out_res
    image = np.full(lead + nb + 64, GUARD, dtype=np.uint8)
    image[lead:lead + nb] = hay if inplace else prefill
    d_out = capi.DeviceBuffer(len(image) + 16).upload(image)
    assert d_out.ptr % 16 == 0
    d_hay = None
    if not inplace:
        d_hay = capi.DeviceBuffer(hay_res + nb + 16).upload(np.concatenate([np.full(hay_res, 0xA5, np.uint8), hay, np.full(1, 0xA5, np.uint8)]))
    d_rec = capi.DeviceBuffer(24 * n + 16)
    d_cnt = capi.DeviceBuffer(8 * rows + 16)
    if n:
        d_rec.upload(rec.reshape(-1))
    if rows:
        d_cnt.upload(counts)
    d_off = None
    if offsets is not None:
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64))
        assert len(off) == rows + 1
        d_off = capi.DeviceBuffer(8 * len(off)).upload(off)
    p_out = d_out.ptr + lead
    p_hay = p_out if inplace else d_hay.ptr + hay_res
    try:
        capi.mask_rows_device(p_hay, nb, d_off.ptr if d_off else 0, rows if (d_off or uniform) else 0, uniform, d_rec.ptr if n else 0, n,
                              d_cnt.ptr if rows else 0, fill, flags, p_out)
        got = d_out.download(len(image))
        assert np.array_equal(d_rec.download(24 * n).view(np.uint64), rec.reshape(-1)), "the records were written"
        assert np.array_equal(d_cnt.download(8 * rows).view(np.uint64), counts), "the counts were written"
        if d_off:
            assert np.array_equal(d_off.download(8 * (rows + 1)).view(np.uint64), off), "the offsets were written"
        if d_hay:
            after = d_hay.download(hay_res + nb + 1)
            assert np.array_equal(after[hay_res:hay_res + nb], hay) and (after[:hay_res] == 0xA5).all() and after[-1] == 0xA5, "the haystack was written"
    finally:
        for b in (d_out, d_hay, d_rec, d_cnt, d_off):
            if b:
                b.free()
    assert (got[:lead] == GUARD).all(), ("a byte before the output was written", int(np.flatnonzero(got[:lead] != GUARD)[-1]) - lead)
    assert (got[lead + nb:] == GUARD).all(), ("a byte behind the output was written", int(np.flatnonzero(got[lead + nb:] != GUARD)[0]))
    return got[lead:lead + nb]


def check_stage(hay, lens, records, counts, fill=0x2A, flags=0, what=None, form="offsets", **kw):
    """lens: the rows' lengths (form "offsets": cut by device offsets; "uniform": they are all equal and the row length cuts;
    "one": a single row, cut by nothing)"""
    offsets = np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.int64)
    assert int(offsets[-1]) == len(hay) and len(lens) == len(counts)
    if form == "uniform":
        assert len(set(int(x) for x in lens)) == 1
    if form == "one":
        assert len(lens) == 1
    got = run_stage(hay, offsets if form == "offsets" else None, int(lens[0]) if form == "uniform" else 0, records, counts, fill, flags, **kw)
    want = definition(hay, offsets, records, counts, fill, flags)
    if not np.array_equal(got, want):
        bad = int(np.flatnonzero(got != want)[0])
        row = int(np.searchsorted(offsets, bad, side="right")) - 1
        raise AssertionError((what, form, fill, flags, kw, "bytes", len(want), "first difference at", bad, "row", row, "which begins at",
                              int(offsets[row]), bytes(got[bad:bad + 24]), bytes(want[bad:bad + 24])))
    return want


def text(n, seed):
    return np.random.default_rng(seed).integers(97, 123, size=n, dtype=np.uint8)


def ragged_counts(n, seed, choices=(0, 0, 1, 2, 3, 7, 40)):
    """per-row record counts from `choices` that sum to exactly n (at least one row)"""
    rng = np.random.default_rng(seed)
    out, left = [], n
    while left:
        c = min(int(rng.choice(choices)), left)
        out.append(c)
        left -= c
    return out or [0]


def records_in(lens, counts, seed, lengths=(1, 1, 2, 3, 5, 8, 13, 16, 17, 31, 40), beyond=False):
    """counts[h] records in row h of lens[h] bytes, random starts, ordered by end within a row as a search reports them;
    beyond: a record may end a few bytes behind its row or begin behind it (the clip)"""
    rng = np.random.default_rng(seed)
    row = np.repeat(np.arange(len(counts)), np.asarray(counts, dtype=np.int64))
    rl = np.asarray(lens, dtype=np.int64)[row]
    start = (rng.random(len(row)) * (rl + (4 if beyond else 0))).astype(np.int64)
    end = start + rng.choice(lengths, size=len(row))
    if not beyond:
        end = np.minimum(end, rl)
    order = np.lexsort((start, end, row))
    return np.stack([rng.integers(0, 1 << 24, size=len(row)), start[order], end[order]], axis=1).astype(np.uint64)


def batch(n, seed, count_choices=(0, 0, 1, 2, 3, 7, 40), row_lens=(0, 1, 50, 130, 300), **kw):
    """a ragged batch with exactly n records -> (hay, lens, records, counts)"""
    counts = ragged_counts(n, seed, count_choices)
    rng = np.random.default_rng(seed + 1)
    lens = rng.choice(row_lens, size=len(counts))
    lens[np.asarray(counts) > 0] += 1  # (a row that has records has a byte)
    return text(int(lens.sum()), seed + 2), lens, records_in(lens, counts, seed + 3, **kw), counts


@pytest.mark.parametrize("n", [0, 1, T - 1, T, T + 1, 2 * T + 1])
def test_stage_record_counts_around_the_tile(n):
    for flags in (0, ZERO):
        check_stage(*batch(n, n + 10), 0x2A, flags, ("ragged", n))
        check_stage(*batch(n, n + 20, (0, 1, 300, 700)), 0x2A, flags, ("rows of many records", n))
        check_stage(*batch(n, n + 30, (1,)), 0x2A, flags, ("every row of one record", n))
    hay = text(5000, n)
    check_stage(hay, [5000], records_in([5000], [n], n + 40), [n], 0x2A, 0, ("one row holds everything", n), form="one")
    check_stage(hay, [0, 0, 5000, 0], records_in([0, 0, 5000, 0], [0, 0, n, 0], n + 50), [0, 0, n, 0], 0x2A, 0, ("one row between empty ones", n))


@pytest.mark.parametrize("out_res", [0, 5])
def test_stage_every_start_residue_and_every_short_length(out_res):
    """every residue 0 .. 15 of the first store's address crossed with every length 1 .. 33, all in one buffer: each record in a
    64-byte slot of its own, the bytes between them show a store that is too wide"""
    slots = [(r, n) for r in range(16) for n in range(1, 34)]
    start = np.asarray([64 * k + (r - out_res) % 16 for k, (r, n) in enumerate(slots)], dtype=np.uint64)
    length = np.asarray([n for _, n in slots], dtype=np.uint64)
    rec = np.stack([np.zeros(len(slots), np.uint64), start, start + length], axis=1)
    hay = text(64 * len(slots), 3)
    for flags in (0, ZERO):
        want = check_stage(hay, [len(hay)], rec, [len(slots)], 0xFF, flags, "one row", form="one", out_res=out_res)
        assert int((want == 0xFF).sum()) == int(length.sum())
        rel = rec.copy()
        rel[:, 1:] -= (64 * np.arange(len(slots), dtype=np.uint64))[:, None]
        check_stage(hay, [64] * len(slots), rel, [1] * len(slots), 0xFF, flags, "a row per slot", form="uniform", out_res=out_res)
    check_stage(hay, [len(hay)], rec, [len(slots)], 0x2A, 0, "in place", form="one", out_res=out_res, inplace=True)


def test_stage_lengths_around_the_sweep():
    """MASK_LONG - 1, MASK_LONG, MASK_LONG + 1; one cooperative sweep - 1, exact, + 1; six sweeps + 5 -- each at three start
    residues, all in one tile"""
    lengths = [LONG - 1, LONG, LONG + 1, SWEEP - 1, SWEEP, SWEEP + 1, 6 * SWEEP + 5, SWEEP + 16, SWEEP + 15, 2 * SWEEP]
    slot = 6 * SWEEP + 5 + 80
    cases = [(n, r) for n in lengths for r in (0, 1, 15)]
    start = np.asarray([slot * k + 32 + r for k, (n, r) in enumerate(cases)], dtype=np.uint64)
    rec = np.stack([np.zeros(len(cases), np.uint64), start, start + np.asarray([n for n, _ in cases], dtype=np.uint64)], axis=1)
    hay = text(slot * len(cases), 4)
    for flags in (0, ZERO):
        for out_res in (0, 7):
            check_stage(hay, [len(hay)], rec, [len(cases)], 0x2A, flags, "long records", form="one", out_res=out_res)
    check_stage(hay, [len(hay)], rec, [len(cases)], 0x00, 0, "long records in place", form="one", inplace=True, out_res=3)
    # long and short records that overlap: nested, identical, chained -- every writer stores the same value
    rec2 = np.asarray([[0, 100, 100 + LONG], [1, 90, 110 + LONG], [2, 90, 110 + LONG], [3, 50, 120 + 3 * SWEEP], [4, 100 + 3 * SWEEP, 130 + 3 * SWEEP],
                       [5, 125 + 3 * SWEEP, 130 + 4 * SWEEP + LONG], [6, 130 + 4 * SWEEP + LONG, 131 + 4 * SWEEP + LONG]], dtype=np.uint64)
    check_stage(hay, [len(hay)], rec2, [len(rec2)], 0x2A, 0, "long records that overlap", form="one", out_res=9)
    # a tile whose every record is long (the tile's list is full), one more tile behind it
    n = T + 3
    st = np.arange(n, dtype=np.uint64) * np.uint64(7)
    rec3 = np.stack([st, st, st + np.uint64(LONG + 1)], axis=1)
    want = check_stage(hay, [len(hay)], rec3, [n], 0x2A, ZERO, "a tile of long records", form="one", out_res=1)
    assert int((want == 0x2A).sum()) == 7 * (n - 1) + LONG + 1


def test_stage_pointer_residues():
    """the output and the haystack each at 0, 1, 5 and 15 modulo 16, never the same pair"""
    hay, lens, rec, counts = batch(700, 77, row_lens=(0, 50, 300, 2000), lengths=(1, 3, 16, 17, 40, LONG + 5))
    for o in (0, 1, 5, 15):
        for h in (0, 1, 5, 15):
            if o != h:
                check_stage(hay, lens, rec, counts, 0x2A, 0, "residues", out_res=o, hay_res=h)
    for o in (1, 15):
        check_stage(hay, lens, rec, counts, 0x01, ZERO, "residues, 0 / 1", out_res=o, hay_res=0)
        check_stage(hay, lens, rec, counts, 0x2A, 0, "residues, in place", out_res=o, inplace=True)


def rows_with(counts, seed, row_len=600, **kw):
    lens = [row_len] * len(counts)
    return text(row_len * len(counts), seed), lens, records_in(lens, counts, seed + 1, **kw), counts


def test_stage_row_seams():
    for counts, what in (([T, T, 5], "a row boundary on a tile's last record"),
                         ([T - 1, 1, T - 1, 1, 3], "rows of one record that are a tile's last record"),
                         ([1, T - 1, 1, T - 1, 3], "rows of one record that are a tile's first record"),
                         ([T - 5, 2 * T + 10, 7], "a row whose records span three tiles"),
                         ([3 * T], "one row of exactly three tiles"),
                         ([T, 0, T], "an empty row on a tile boundary"),
                         ([T, 0, 0, 0, 1], "empty rows on a tile boundary, one record behind them"),
                         ([0, 0, T, 0, 0, T, 0], "empty rows on every boundary")):
        for form in ("offsets", "uniform"):
            check_stage(*rows_with(counts, len(counts)), 0x2A, 0, what, form=form)
    # 100 000 empty rows between two records (more than a tile has slots or a workgroup threads), at the start and at the end
    many = 100_000
    for counts, what in (([1] + [0] * many + [1], "between two records"), ([0] * many + [2, 3], "at the start"),
                         ([2, 3] + [0] * many, "at the end"), ([T] + [0] * many + [T], "between two tiles")):
        check_stage(*rows_with(counts, 5, row_len=3, lengths=(1, 2, 3)), 0x2A, 0, what, form="uniform")
        lens = np.zeros(len(counts), dtype=np.int64)  # (rows without a byte, too)
        lens[np.asarray(counts) > 0] = 40
        check_stage(text(int(lens.sum()), 6), lens, records_in(lens, counts, 7), counts, 0x2A, ZERO, what)


@pytest.mark.parametrize("rows", [S - 1, S, S + 1, S * S + 1])
def test_stage_row_counts_around_the_scans_levels(rows):
    rng = np.random.default_rng(rows)
    counts = np.zeros(rows, dtype=np.int64)
    some = rng.choice(rows, size=min(rows, 3000), replace=False)
    counts[some] = rng.choice([1, 1, 2, 5, 40], size=len(some))
    counts[[0, rows - 1]] = 3  # (the first and the last row)
    lens = np.full(rows, 2, dtype=np.int64)
    lens[some] = rng.choice([1, 9, 70], size=len(some))
    hay = text(int(lens.sum()), rows + 1)
    check_stage(hay, lens, records_in(lens, counts, rows + 2), counts, 0x2A, 0, ("rows", rows))


def test_stage_the_three_ways_to_cut_the_bytes():
    rows, L = 300, 100
    counts = ragged_counts(900, 8)
    counts = (counts + [0] * rows)[:rows]
    counts[-1] += 900 - sum(counts)
    hay = text(rows * L, 9)
    rec = records_in([L] * rows, counts, 10)
    for flags in (0, ZERO):
        a = check_stage(hay, [L] * rows, rec, counts, 0x2A, flags, "cut", form="offsets")
        b = check_stage(hay, [L] * rows, rec, counts, 0x2A, flags, "cut", form="uniform")
        assert np.array_equal(a, b)
        # the same bytes as ONE row: the records' offsets become the buffer's
        row = np.repeat(np.arange(rows), counts).astype(np.uint64)
        one = rec.copy()
        one[:, 1:] += (row * np.uint64(L))[:, None]
        c = check_stage(hay, [rows * L], one, [len(one)], 0x2A, flags, "cut", form="one")
        assert np.array_equal(a, c)


def test_stage_row_edges():
    hay = text(40, 11)
    lens = [10, 10, 0, 20]
    for flags in (0, ZERO):
        want = check_stage(hay, lens, [[0, 7, 10]], [1, 0, 0, 0], 0xFF, flags, "a match that ends on the row's last byte")
        assert list(np.flatnonzero(want == 0xFF)) == [7, 8, 9]
        want = check_stage(hay, lens, [[0, 2, 5], [1, 5, 9]], [0, 2, 0, 0], 0xFF, flags, "adjacent matches")
        assert list(np.flatnonzero(want == 0xFF)) == list(range(12, 19))
        want = check_stage(hay, lens, [[0, 0, 1], [0, 17, 20]], [1, 0, 0, 1], 0xFF, flags, "the buffer's first and last byte")
        assert list(np.flatnonzero(want == 0xFF)) == [0, 37, 38, 39]
        want = check_stage(hay, lens, [[0, 9, 10], [0, 0, 1]], [1, 1, 0, 0], 0xFF, flags, "a row's last byte and the next row's first")
        assert list(np.flatnonzero(want == 0xFF)) == [9, 10]
        want = check_stage(hay, lens, [[0, 3, 3], [0, 0, 0], [0, 20, 20]], [1, 1, 0, 1], 0xFF, flags, "empty matches cover nothing")
        assert not (want == 0xFF).any()


def test_stage_all_or_nothing():
    hay = text(3 * SWEEP + 77, 12)
    n = len(hay)
    for flags in (0, ZERO):
        for out_res in (0, 13):
            want = check_stage(hay, [n], [[0, 0, n]], [1], 0x2A, flags, "one record covers every byte", form="one", out_res=out_res)
            assert (want == 0x2A).all()
            lens = [1000, 0, n - 1000]
            want = check_stage(hay, lens, [[0, 0, 600], [1, 600, 1000], [0, 0, 5], [1, 5, n - 1000]], [2, 0, 2], 0x2A, flags, "every byte covered", out_res=out_res)
            assert (want == 0x2A).all()
            # no record at all: a pure copy, or a pure clear
            want = check_stage(hay, lens, [], [0, 0, 0], 0x2A, flags, "no record", out_res=out_res, hay_res=3)
            assert np.array_equal(want, np.zeros(n, np.uint8) if flags else hay)
            check_stage(hay, [n], [], [0], 0x2A, flags, "no record, one row", form="one", out_res=out_res)
    got = run_stage(hay, None, 0, [], [0], 0x2A, 0, inplace=True)  # in place without a record: nothing is written
    assert np.array_equal(got, hay)
    # no byte, no row: nothing is launched, null pointers are taken
    assert len(run_stage([], [0], 0, [], [], 0x2A)) == 0 and len(run_stage([], None, 0, [], [0], 0x2A, ZERO)) == 0
    capi.mask_rows_device(0, 0, 0, 0, 0, 0, 0, 0, 0x2A, 0, 0)


def test_stage_clips_every_record_to_its_row():
    """an end a few bytes behind the row, a start behind the row: both point at bytes that still lie inside the allocation --
    the next row or the guard -- so a record that is not clipped shows as wrong bytes"""
    hay = text(60, 13)
    lens = [20, 20, 20]
    for flags in (0, ZERO):
        for form in ("offsets", "uniform"):
            want = check_stage(hay, lens, [[0, 15, 24]], [1, 0, 0], 0xFF, flags, "an end behind the row", form=form)
            assert list(np.flatnonzero(want == 0xFF)) == [15, 16, 17, 18, 19]
            want = check_stage(hay, lens, [[0, 15, 27]], [0, 0, 1], 0xFF, flags, "an end behind the last row: the guard", form=form)
            assert list(np.flatnonzero(want == 0xFF)) == [55, 56, 57, 58, 59]
            want = check_stage(hay, lens, [[0, 22, 26]], [0, 1, 0], 0xFF, flags, "a start behind the row", form=form)
            assert not (want == 0xFF).any()
            want = check_stage(hay, lens, [[0, 21, 23]], [0, 0, 1], 0xFF, flags, "a start behind the last row: the guard", form=form)
            assert not (want == 0xFF).any()
            want = check_stage(hay, lens, [[0, 9, 4], [1, 1 << 63, (1 << 64) - 1], [2, 5, (1 << 64) - 1]], [1, 1, 1], 0xFF, flags, "start > end; huge words", form=form)
            assert list(np.flatnonzero(want == 0xFF)) == list(range(45, 60))
        want = check_stage(hay, [60], [[0, 50, 70 + LONG], [0, 61, 64]], [2], 0xFF, flags, "one row", form="one")
        assert list(np.flatnonzero(want == 0xFF)) == list(range(50, 60))
    # the same over many rows with long records behind their rows: a sweep stays inside its row too
    hay2, lens2, _, counts2 = batch(2 * T + 9, 14, row_lens=(5, 60, 900))
    rec2 = records_in(lens2, counts2, 15, lengths=(1, 3, 17, 40, LONG, LONG + 17, SWEEP + 3), beyond=True)
    for flags in (0, ZERO):
        check_stage(hay2, lens2, rec2, counts2, 0x2A, flags, "random records, clipped", out_res=5)
    check_stage(hay2, lens2, rec2, counts2, 0x2A, 0, "random records, clipped, in place", out_res=11, inplace=True)


@pytest.mark.parametrize("fill", [0x00, 0xFF, 0x2A])
def test_stage_fills_in_place_and_the_zero_form(fill):
    hay, lens, rec, counts = batch(T + 77, 16 + fill, row_lens=(0, 50, 300, 3000), lengths=(1, 2, 7, 16, 33, 100, LONG + 1))
    hay[::7] = fill  # (the fill is a byte of the haystack, too)
    check_stage(hay, lens, rec, counts, fill, 0, "copy", out_res=2, hay_res=9)
    check_stage(hay, lens, rec, counts, fill, ZERO, "0 / fill", out_res=2, hay_res=9, prefill=0x55)
    check_stage(hay, lens, rec, counts, fill, 0, "in place", out_res=2, inplace=True)


def test_stage_refuses_bad_arguments():
    d = capi.DeviceBuffer(8192)
    d.upload(np.zeros(1024, dtype=np.uint64))
    d.upload(np.asarray([2, 1], dtype=np.uint64))                                   # the counts of two rows: 3 records
    capi.lib().acx_device_upload(d.ptr + 512, np.asarray([0, 40, 100], dtype=np.uint64).ctypes.data, 24)  # their offsets
    args = dict(d_hay=d.ptr + 2048, nbytes=100, d_offsets=d.ptr + 512, n_hay=2, uniform_len=0, d_records=d.ptr + 1024, n=3, d_counts=d.ptr,
                fill=1, flags=0, d_out=d.ptr + 4096)
    capi.mask_rows_device(**args)
    capi.mask_rows_device(**{**args, "d_out": args["d_hay"]})                       # in place
    capi.mask_rows_device(**{**args, "d_offsets": 0, "uniform_len": 50})
    capi.mask_rows_device(**{**args, "flags": ZERO, "d_hay": 0})                    # the 0 / 1 form reads no haystack
    for change in (dict(n=4), dict(n=2), dict(flags=2), dict(flags=3), dict(flags=1 << 31), dict(d_records=d.ptr + 1028), dict(d_counts=d.ptr + 4),
                   dict(d_offsets=d.ptr + 516), dict(d_out=0), dict(d_hay=0), dict(d_counts=0), dict(d_records=0), dict(uniform_len=50),
                   dict(d_offsets=0, uniform_len=7), dict(nbytes=99), dict(nbytes=101), dict(d_offsets=d.ptr + 520, n_hay=1),
                   dict(flags=ZERO, d_out=d.ptr + 2048)):
        with pytest.raises(ValueError) as ei:
            capi.mask_rows_device(**{**args, **change})
        assert ei.value.code == capi.EINVAL, change
    d.free()


# ---------------------------------------------------------------------------
# end to end through the C ABI against the oracle
# ---------------------------------------------------------------------------
PATS = gen.gen_patterns(500, 3, 9, gen.AZ, 5) + [b"ab", b"abab", b"bab", b"ab"]  # (a copy: it covers the same bytes once)
KINDS = [(0, False), (0, True), (1, False), (2, False)]


def oracle_cover(o, hays, ov, fill, flags, search=None):
    """the issue's definition from the oracle's matches: every row's bytes with the bytes of its matches filled.  search: the
    bytes the oracle sees (a case-insensitive handle's folded rows), the output keeps the caller's"""
    out = []
    for i, h in enumerate(hays):
        m = o.find_raw(h if search is None else search[i], overlapping=ov)
        out.append(definition(np.frombuffer(h, dtype=np.uint8), [0, len(h)], m, [len(m)], fill, flags))
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint8)


def download_bytes(ptr, n):
    out = np.empty(n, dtype=np.uint8)
    if n:
        capi._check(capi.lib().acx_device_download(out.ctypes.data, ptr, n))
    return out


def check_masked(m, want, hays, on_device, what=None):
    """a capi.DeviceMasked against the definition, through the copies and through the raw addresses"""
    offsets = np.concatenate([[0], np.cumsum([len(h) for h in hays])]).astype(np.int64)
    assert m.on_device == on_device and m.rows == len(hays) and m.nbytes == len(want), (what, m.rows, m.nbytes, len(hays), len(want))
    got = m.data()
    if not np.array_equal(got, want):
        bad = int(np.flatnonzero(got != want)[0])
        raise AssertionError((what, "first difference at", bad, bytes(got[max(bad - 8, 0):bad + 24]), bytes(want[max(bad - 8, 0):bad + 24])))
    assert np.array_equal(m.offsets(), offsets), what
    p, q = m.data_ptr(), m.offsets_ptr()
    assert p and q and q % 8 == 0, what  # (an empty part still has an address)
    if on_device:
        assert np.array_equal(download_bytes(p, len(want)), want) and np.array_equal(download_bytes(q, offsets.nbytes), offsets.view(np.uint8)), what
    else:
        assert np.array_equal(np.ctypeslib.as_array((capi.ctypes.c_uint8 * max(len(want), 1)).from_address(p))[:len(want)], want)
    m.free()


def batch_with_empties(pats, n_hay, seed):
    """n_hay haystacks of 0 .. 3000 bytes: empty ones in front, in the middle (two in a row) and at the end, some without a
    match (the shape of tests/test_gpu_filter.py's)"""
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
def test_mask_parity_host_and_device_inputs(mk, ov):
    o = Oracle(PATS, mk, KIND_DFA)
    a = capi.Automaton(PATS, mk)
    for n_hay in (1, 65, 323):
        hays = batch_with_empties(PATS, n_hay, 100 + n_hay)
        for fill, flags in ((0x2A, 0), (1, ZERO)):
            want = oracle_cover(o, hays, ov, fill, flags)
            assert n_hay == 1 or (want == fill).any()
            check_masked(a.mask(hays, fill, ov, flags), want, hays, False, (mk, ov, n_hay, flags))
            for off in (0, 5):
                d = OnDevice(hays, off)
                check_masked(a.mask_device(*d.args, fill, overlapping=ov, flags=flags, **d.kw), want, hays, True, (mk, ov, n_hay, off, flags))
                d.free()
    # a uniform batch on the device, and the same bytes as a host batch
    L, nh = 512, 130
    full = gen.gen_textlike(L * nh, 61, PATS).tobytes()
    hays = [full[i * L:(i + 1) * L] for i in range(nh)]
    dev = capi.DeviceBuffer(len(full)).upload(np.frombuffer(full, dtype=np.uint8))
    for fill, flags in ((0xFF, 0), (0x00, 0), (1, ZERO)):
        want = oracle_cover(o, hays, ov, fill, flags)
        check_masked(a.mask_device(dev.ptr, len(full), fill, n_hay=nh, uniform_len=L, overlapping=ov, flags=flags), want, hays, True, "uniform")
        check_masked(a.mask(hays, fill, ov, flags), want, hays, False, "uniform, host")
    assert dev.download().tobytes() == full
    dev.free()
    a.close()


def test_mask_overlapping_is_the_union_and_copies_cover_once():
    pats = [b"abcd", b"bc", b"cdef", b"bc", b"f"]
    o, a = Oracle(pats, 0, KIND_DFA), capi.Automaton(pats, 0)
    hays = [b"xabcdefx", b"bcbc", b"", b"abcdxcdef", b"zzz"]
    plain = oracle_cover(o, hays, False, 0x2A, 0)
    union = oracle_cover(o, hays, True, 0x2A, 0)
    assert bytes(union[:8]) == b"x******x" and bytes(plain[:8]) != bytes(union[:8])
    for ov, want in ((False, plain), (True, union)):
        check_masked(a.mask(hays, 0x2A, ov), want, hays, False, ov)
        d = OnDevice(hays, 3)
        check_masked(a.mask_device(*d.args, 0x2A, overlapping=ov, **d.kw), want, hays, True, ov)
        d.free()
    a.close()


def test_mask_long_matches_go_through_the_sweep():
    """matches of MASK_LONG bytes and more from a real find: a pattern of 601 bytes, one of 5000 and, overlapping, a run in
    which every second byte begins a match of 600"""
    pats = [b"ab" * 300 + b"c", b"q" * 5000, b"ab" * 300, b"zz"]
    assert LONG <= 600
    hays = [b"x" * 77 + pats[0] + b"yy" + pats[1] + b"zz", b"ab" * 2000 + b"c", b"", b"q" * 4999 + b"zz", b"zz" + b"q" * 12_000]
    for mk, ov in KINDS:
        o, a = Oracle(pats, mk, KIND_DFA), capi.Automaton(pats, mk)
        for fill, flags in ((0x2A, 0), (1, ZERO)):
            want = oracle_cover(o, hays, ov, fill, flags)
            assert int((want == fill).sum()) > 10_000
            check_masked(a.mask(hays, fill, ov, flags), want, hays, False, (mk, ov, flags))
            d = OnDevice(hays, 9)
            check_masked(a.mask_device(*d.args, fill, overlapping=ov, flags=flags, **d.kw), want, hays, True, (mk, ov, flags))
            d.free()
        a.close()


def test_mask_one_haystack_that_is_no_batch_empty_batches_and_errors():
    o, a = Oracle(PATS, 0, KIND_DFA), capi.Automaton(PATS, 0)
    for hay in (gen.gen_textlike(5000, 3, PATS).tobytes(), gen.gen_textlike(300_000, 4, PATS).tobytes(), b"0123" * 100, b""):
        for fill, flags in ((0x2A, 0), (1, ZERO)):
            want = oracle_cover(o, [hay], False, fill, flags)
            dev = capi.DeviceBuffer(len(hay) + 16).upload(np.frombuffer(hay + b"\0", dtype=np.uint8))
            check_masked(a.mask(None, fill, False, flags, single=hay), want, [hay], False, ("single", len(hay), flags))
            check_masked(a.mask_device(dev.ptr, len(hay), fill, flags=flags), want, [hay], True, ("single, device", len(hay), flags))
            dev.free()
    none = np.zeros(0, dtype=np.uint8)
    check_masked(a.mask([], 0x2A), none, [], False, "empty batch")
    check_masked(a.mask([b"", b""], 0x2A), none, [b"", b""], False, "empty rows only")
    dev = capi.DeviceBuffer(64)
    check_masked(a.mask_device(dev.ptr, 0, 0x2A, n_hay=0, uniform_len=8), none, [], True, "empty batch, device")
    for call in (lambda: a.mask([b"ab"], 1, flags=2), lambda: a.mask_device(dev.ptr, 0, 1, n_hay=0, uniform_len=8, flags=2),
                 lambda: a.mask_device(dev.ptr, 10, 1, n_hay=3, uniform_len=4)):
        with pytest.raises(ValueError) as ei:
            call()
        assert ei.value.code == capi.EINVAL
    for mk in (1, 2):
        b = capi.Automaton([b"ab", b"b"], mk)
        for call in (lambda: b.mask([b"xxabxx"], 1, overlapping=True), lambda: b.mask(None, 1, overlapping=True, single=b"ab"),
                     lambda: b.mask_device(0, 0, 1, n_hay=0, uniform_len=8, overlapping=True)):
            with pytest.raises(ValueError) as ei:
                call()
            assert ei.value.code == capi.EOVERLAP
        b.close()
    dev.free()
    a.close()


def test_mask_case_insensitive_handle_keeps_the_callers_case():
    pats = [b"Needle", b"hay", b"STACK"]
    o = Oracle([p.translate(FOLD) for p in pats], 1, KIND_DFA)
    hays = [b"a nEEdle in a HayStack; " * 3, b"Nothing Here", b"", b"NEEDLE", b"x" * 5000 + b"hAY", b"NO", b"needle HAY stack Xyz" * 900]
    folded = [h.translate(FOLD) for h in hays]
    a = capi.Automaton(pats, 1, ascii_case_insensitive=True)
    for fill, flags in ((0x2A, 0), (1, ZERO)):
        want = oracle_cover(o, hays, False, fill, flags, search=folded)
        if not flags:
            assert bytes(want[:24]) == b"a ****** in a ********; " and bytes(want[72:84]) == b"Nothing Here"
        check_masked(a.mask(hays, fill, False, flags), want, hays, False, flags)
        d = OnDevice(hays, 5)
        check_masked(a.mask_device(*d.args, fill, flags=flags, **d.kw), want, hays, True, flags)
        d.free()
    a.close()


def test_mask_of_a_find_cut_into_byte_ranges(monkeypatch):
    o, a = Oracle(PATS, 0, KIND_DFA), capi.Automaton(PATS, 0)
    hay = gen.gen_textlike(3_000_000, 17, PATS).tobytes()
    dev = capi.DeviceBuffer(len(hay)).upload(np.frombuffer(hay, dtype=np.uint8))
    monkeypatch.setenv("ACX_CHUNK_BYTES", "700001")
    a.path_stats(reset=True)
    for ov in (False, True):
        check_masked(a.mask_device(dev.ptr, len(hay), 0x2A, overlapping=ov), oracle_cover(o, [hay], ov, 0x2A, 0), [hay], True, ("cut", ov))
    check_masked(a.mask_device(dev.ptr, len(hay), 1, flags=ZERO), oracle_cover(o, [hay], False, 1, ZERO), [hay], True, "cut, 0 / 1")
    st = a.path_stats()
    monkeypatch.delenv("ACX_CHUNK_BYTES")
    assert st["byte_ranges"] >= 2, st
    dev.free()
    a.close()


def test_mask_of_a_batch_cut_over_the_occurrence_limit(monkeypatch):
    # the batch of test_gpu_chunked.py: one pass may index 50 000 occurrences, the batch is cut at haystack boundaries
    pats = [b"ab", b"b", b"bab"]
    r = random.Random(5)
    hs = [b"ab" * r.randint(1, 60_000) + bytes(r.choice(b"abc") for _ in range(r.randint(0, 300))) for _ in range(7)] + [b"", b"abab"]
    for mk in (0, 1):
        a, o = capi.Automaton(pats, mk), Oracle(pats, mk, KIND_DFA)
        want = oracle_cover(o, hs, False, 0x2A, 0)
        monkeypatch.setenv("ACX_MAX_OCC", "50000")
        monkeypatch.setenv("ACX_NO_BUCKET", "1")
        d = OnDevice(hs, 5)
        a.path_stats(reset=True)
        check_masked(a.mask_device(*d.args, 0x2A, **d.kw), want, hs, True, ("max_occ", mk))
        st = a.path_stats()
        monkeypatch.delenv("ACX_MAX_OCC")
        monkeypatch.delenv("ACX_NO_BUCKET")
        assert st["byte_ranges"] >= 2, st
        d.free()
        a.close()


def test_mask_of_a_find_on_the_dense_path():
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
    want = oracle_cover(o, [every], False, 0x2A, 0)
    dev = capi.DeviceBuffer(len(every)).upload(np.frombuffer(every, dtype=np.uint8))
    a.path_stats(reset=True)
    for _ in range(2):  # (one haystack that is no batch: the call tests/test_gpu_columns.py sees take that path)
        check_masked(a.mask_device(dev.ptr, len(every), 0x2A), want, [every], True, "dense, one row")
    st = a.path_stats()
    assert st["hot_calls"] + st["dense_tiles"] + st["dense_radix"] >= 2, st
    check_masked(a.mask_device(dev.ptr, len(every), 0x2A, n_hay=len(hays), uniform_len=L), oracle_cover(o, hays, False, 0x2A, 0), hays, True, "dense")
    check_masked(a.mask_device(dev.ptr, len(every), 1, n_hay=len(hays), uniform_len=L, flags=ZERO), oracle_cover(o, hays, False, 1, ZERO), hays, True,
                 "dense, 0 / 1")
    dev.free()
    a.close()


def test_eight_threads_on_one_handle():
    a, o = capi.Automaton(PATS, 0), Oracle(PATS, 0, KIND_DFA)
    work = []
    for t in range(8):
        hays = batch_with_empties(PATS, 40 + 9 * t, 300 + t) + [gen.gen_textlike(150_000, t, PATS).tobytes()]
        work.append((hays, oracle_cover(o, hays, False, 0x2A, 0), oracle_cover(o, hays, False, 1, ZERO)))
    errors = []

    def run(t):
        try:
            hays, want, want01 = work[t]
            for i in range(3):
                check_masked(a.mask(hays, 0x2A), want, hays, False, t)
                d = OnDevice(hays, t)
                check_masked(a.mask_device(*d.args, 0x2A, **d.kw), want, hays, True, t)
                check_masked(a.mask_device(*d.args, 1, flags=ZERO, **d.kw), want01, hays, True, t)
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
    rng = random.Random(20261018)
    for case in range(36):
        mk = rng.choice([0, 0, 1, 2])
        ov = mk == 0 and rng.random() < 0.4
        alpha = rng.choice([b"ab", b"abcd", gen.AZ])
        pats = gen.gen_patterns(rng.choice([1, 3, 40, 600]), 1, rng.choice([2, 6, 12]), alpha, 1000 + case)
        text_ = rng.choice([alpha, alpha + b"xyz", b"0123"])
        o = Oracle(pats, mk, KIND_DFA)
        n_hay = rng.choice([1, 2, 7, 64, 65, 130, 700])
        hays = [bytes(rng.choices(text_, k=rng.choice([0, 0, 1, 9, 200, 5000, 20000]))) for _ in range(n_hay)]
        while sum(len(o.find_raw(h, overlapping=ov)) for h in hays) > 100_000:  # (cut down, never skipped)
            hays = [h[:len(h) // 2] for h in hays]
        fill, flags = rng.choice([(0x2A, 0), (0x00, 0), (0xFF, 0), (1, ZERO), (0xFF, ZERO)])
        want = oracle_cover(o, hays, ov, fill, flags)
        route = rng.choice(["host", "device", "device"])
        a = capi.Automaton(pats, mk)
        what = (case, mk, ov, n_hay, route, fill, flags)
        try:
            if route == "device":
                d = OnDevice(hays, rng.randrange(16))
                check_masked(a.mask_device(*d.args, fill, overlapping=ov, flags=flags, **d.kw), want, hays, True, what)
                d.free()
            else:
                check_masked(a.mask(hays, fill, ov, flags), want, hays, False, what)
        except AssertionError as e:
            raise AssertionError(f"case {what}: {e}") from e
        a.close()


# ---------------------------------------------------------------------------
# the Python methods: sequences of host objects (tensors in HBM and torch as the consumer: the script below)
# ---------------------------------------------------------------------------
def matchkind(ar, mk):
    return (ar.MatchKind.Standard, ar.MatchKind.LeftmostFirst, ar.MatchKind.LeftmostLongest)[mk]


def rows_of(flat, hays):
    out, at = [], 0
    for h in hays:
        out.append(flat[at:at + len(h)].tobytes())
        at += len(h)
    return out


def check_masked_rows(mr, want, hays, rows=None):
    """a MaskedRows in host memory against the definition; rows: what tolist() gives (the rows of `want`)"""
    offsets = np.concatenate([[0], np.cumsum([len(h) for h in hays])]).astype(np.int64)
    assert len(mr) == len(hays) and mr.device is None and mr.nbytes == len(want)
    assert mr.tolist() == (rows_of(want, hays) if rows is None else rows)
    data, off = mr.data, mr.offsets
    assert len(data) == len(want) and len(off) == len(hays) + 1 and data.__dlpack_device__() == (1, 0)
    got = np.from_dlpack(data)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.from_dlpack(off).dtype == np.int64 and np.array_equal(np.from_dlpack(off), offsets)
    mv = memoryview(data)
    assert mv.format == "B" and mv.readonly and np.array_equal(np.asarray(mv), want) and memoryview(off).format == "q"


@pytest.mark.parametrize("mk,ov", KINDS)
def test_python_sequences_both_classes(mk, ov):
    import ahocorasick_rs as ar
    o = Oracle(PATS, mk, KIND_DFA)
    b = ar.BytesAhoCorasick(PATS, matchkind=matchkind(ar, mk))
    s = ar.AhoCorasick([p.decode() for p in PATS], matchkind=matchkind(ar, mk))
    for n_hay in (0, 1, 64, 130):
        hays = batch_with_empties(PATS, n_hay, 500 + n_hay)
        strs = [h.decode() for h in hays]
        want = oracle_cover(o, hays, ov, 0x2A, 0)
        want01 = oracle_cover(o, hays, ov, 1, ZERO)
        for fill in (0x2A, b"*", bytearray(b"*"), np.asarray([42], dtype=np.uint8)):
            check_masked_rows(b.mask_all_batch(hays, fill, overlapping=ov), want, hays)
        check_masked_rows(b.mask_all_batch(tuple(bytearray(h) for h in hays), 42, ov), want, hays)
        check_masked_rows(b.match_mask_batch(hays, overlapping=ov), want01, hays)
        check_masked_rows(s.mask_all_batch(strs, "*", overlapping=ov), want, hays, [r.decode() for r in rows_of(want, hays)])
        check_masked_rows(s.match_mask_batch(strs, ov), want01, hays)
        # the single forms agree with tolist()
        for h, row, row01 in list(zip(hays, rows_of(want, hays), rows_of(want01, hays)))[:40]:
            assert b.mask_all(h, 42, overlapping=ov) == row and b.mask_all(bytearray(h), b"*", ov) == row and b.match_mask(h, overlapping=ov) == row01
            assert s.mask_all(h.decode(), "*", overlapping=ov) == row.decode() and s.match_mask(h.decode(), ov) == row01
    assert b.mask_all(b"xxabxx", 0) == b"xx\0\0xx" and b.mask_all(b"xxabxx", 255) == b"xx\xff\xffxx" and b.match_mask(b"") == b""


def test_python_str_with_multi_byte_characters():
    """.data and .offsets are in UTF-8 bytes (a covered k-byte character is k fills); the single forms and tolist() give one
    entry per character: len(out) == len(s)"""
    import ahocorasick_rs as ar
    pats = ["é", "€uro", "\U0001F600", "ab", "naïve", "日本"]
    s = ar.AhoCorasick(pats, matchkind=ar.MatchKind.LeftmostLongest)
    o = Oracle([p.encode() for p in pats], 2, KIND_DFA)
    hays = ["café ab €uro \U0001F600!", "", "naïve 日本語 naive", "ascii ab only", "ééé\U0001F600\U0001F600€uro", "€ur"]
    raw = [h.encode() for h in hays]
    want = oracle_cover(o, raw, False, ord("#"), 0)
    want01 = oracle_cover(o, raw, False, 1, ZERO)

    def per_char(h, m01):
        """the matches' bytes -> one flag per character (a match covers whole characters)"""
        at = np.cumsum([0] + [len(c.encode()) for c in h])[:-1]
        return [bool(m01[i]) for i in at]

    texts, masks = [], []
    for h, m01 in zip(hays, rows_of(want01, raw)):
        flags = per_char(h, np.frombuffer(m01, dtype=np.uint8))
        texts.append("".join("#" if f else c for c, f in zip(h, flags)))
        masks.append(bytes(flags))
    assert texts[0] == "caf# ## #### #!" and texts[4] == "#########"
    check_masked_rows(s.mask_all_batch(hays, "#"), want, raw, texts)
    check_masked_rows(s.match_mask_batch(hays), want01, raw, masks)
    for h, t, m in zip(hays, texts, masks):
        got, got01 = s.mask_all(h, "#"), s.match_mask(h)
        assert got == t and len(got) == len(h) and got01 == m and len(got01) == len(h), h
    # a host tensor of the same UTF-8 bytes: byte for byte, since the layout is the point
    flat = np.frombuffer(b"".join(raw), dtype=np.uint8).copy()
    cuts = np.concatenate([[0], np.cumsum([len(r) for r in raw])]).astype(np.int64)
    mr = s.mask_all_batch(flat, "#", offsets=cuts)
    assert mr.tolist() == [r.decode() for r in rows_of(want, raw)] and np.array_equal(np.from_dlpack(mr.data), want)
    assert s.match_mask_batch(flat, offsets=cuts).tolist() == rows_of(want01, raw)


def test_python_errors_and_host_tensors():
    import ahocorasick_rs as ar
    b, s = ar.BytesAhoCorasick([b"ab", b"X"]), ar.AhoCorasick(["ab", "X"])
    for m in (b.mask_all, b.mask_all_batch):
        hay = b"ab" if m == b.mask_all else [b"ab"]
        for bad in (-1, 256, 1 << 70, b"", b"**"):
            with pytest.raises(ValueError):
                m(hay, bad)
        for bad in ("*", 1.0, None, True, [42]):
            with pytest.raises(TypeError):
                m(hay, bad)
        with pytest.raises(TypeError):
            m(hay)                                    # fill is required
        with pytest.raises(TypeError):
            m(hay, 42, overlapping=1)
    for m in (s.mask_all, s.mask_all_batch):
        hay = "ab" if m == s.mask_all else ["ab"]
        for bad in ("", "**", "é", "\x80"):
            with pytest.raises(ValueError):
                m(hay, bad)
        for bad in (42, b"*", None):
            with pytest.raises(TypeError):
                m(hay, bad)
    for call in (lambda: b.match_mask(b"ab", 42), lambda: b.match_mask_batch([b"ab"], fill=1), lambda: b.mask_all("ab", 42), lambda: s.mask_all(b"ab", "*"),
                 lambda: b.mask_all_batch([b"ab"], 42, False, None), lambda: b.mask_all_batch([b"ab"], 42, offsets=np.array([0, 2], dtype=np.int64)),
                 lambda: b.mask_all(b"ab", 42, row_length=2), lambda: s.mask_all_batch([b"ab"], "*")):
        with pytest.raises(TypeError):
            call()
    t = np.frombuffer(b"abxXYxabab", dtype=np.uint8).copy()
    mr = b.mask_all_batch(t, b".", row_length=5)
    assert mr.tolist() == [b"..x.Y", b"x...."] and mr.device is None and len(mr) == 2 and mr.nbytes == 10
    assert np.array_equal(np.from_dlpack(mr.offsets), [0, 5, 10])
    mr = b.match_mask_batch(t, offsets=np.array([0, 1, 1, 6, 10], dtype=np.int64))
    assert mr.tolist() == [b"\0", b"", b"\0\0\1\0\0", b"\1\1\1\1"] and np.array_equal(np.from_dlpack(mr.offsets), [0, 1, 1, 6, 10])
    assert s.mask_all_batch(t, "-", row_length=2).tolist() == ["--", "x-", "Yx", "--", "--"]
    assert t.tobytes() == b"abxXYxabab"
    for mk in (ar.MatchKind.LeftmostFirst, ar.MatchKind.LeftmostLongest):
        for call in (lambda x: x.mask_all(b"ab", 1, overlapping=True), lambda x: x.match_mask(b"ab", overlapping=True),
                     lambda x: x.mask_all_batch([b"ab"], 1, overlapping=True), lambda x: x.match_mask_batch([b"ab"], overlapping=True)):
            with pytest.raises(ValueError):
                call(ar.BytesAhoCorasick([b"ab"], matchkind=mk))
    assert ar.BytesAhoCorasick([b"abc", b"bcd"]).mask_all(b"abcd", 42, overlapping=True) == b"****"
    assert ar.BytesAhoCorasick([b"abc", b"bcd"]).mask_all(b"abcd", 42) == b"***d"
    assert ar.BytesAhoCorasick([b"NeEdLe"], ascii_case_insensitive=True).mask_all(b"A nEEdle, a Needle", 32) == b"A " + b" " * 6 + b", a " + b" " * 6
    with pytest.raises(TypeError):
        ar.MaskedRows()


def test_host_columns_outlive_the_masked_rows():
    import ahocorasick_rs as ar
    o, b = Oracle(PATS, 0, KIND_DFA), ar.BytesAhoCorasick(PATS)
    hays = batch_with_empties(PATS, 300, 3)
    want = oracle_cover(o, hays, False, 0x2A, 0)
    mr = b.mask_all_batch(hays, 42)
    arr, mv, off, unused = np.from_dlpack(mr.data), memoryview(mr.data), np.from_dlpack(mr.offsets), mr.data.__dlpack__()
    del mr, unused, hays
    gc.collect()
    for k in range(20):  # (other results come and go where the bytes would be if they had been freed)
        b.mask_all_batch(batch_with_empties(PATS, 300, 50 + k), 7)
    assert np.array_equal(arr, want) and np.array_equal(np.asarray(mv), want) and int(off[-1]) == len(want)


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
pats = gen.gen_patterns(300, 5, 9, gen.AZ, 5) + [b"abqab", b"abqabqab", b"bqab", b"abqab"]
L, nh = 4096, 200
hay = gen.gen_textlike(L * nh, 13, pats).copy()
hay[3 * L:9 * L] = 48   # (rows without a match)
hay[50 * L:51 * L] = 48
t = torch.from_numpy(hay.copy()).to("cuda:0")
kinds = (ar.MatchKind.Standard, ar.MatchKind.LeftmostFirst, ar.MatchKind.LeftmostLongest)
lens = [0, 0, 17, L, 3 * L, 5, 0, 2 * L + 1, 4 * L, 7, 0]
lens += [L * nh - sum(lens), 0]
cuts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)

def cover(o, rows, ov, fill, zero):
    # the definition: every byte that a match of its row covers becomes fill, every other byte stays (or becomes 0)
    out = []
    for h in rows:
        x = np.zeros(len(h), dtype=np.uint8) if zero else np.frombuffer(h, dtype=np.uint8).copy()
        for _, s, e in o.find_raw(h, overlapping=ov):
            x[int(s):int(e)] = fill
        out.append(x)
    return np.concatenate(out)

def check(mr, want, offsets, where, rows=None):
    assert mr.device == (0 if where == "device" else None), (where, mr.device)
    assert len(mr) == len(offsets) - 1 and mr.nbytes == len(want)
    x, off = torch.from_dlpack(mr.data), torch.from_dlpack(mr.offsets)
    assert x.dtype == torch.uint8 and tuple(x.shape) == (len(want),) and x.is_contiguous() and off.dtype == torch.int64
    assert x.device.type == off.device.type == ("cuda" if where == "device" else "cpu")
    assert torch.equal(x.cpu(), torch.from_numpy(want)), (where, int((x.cpu() != torch.from_numpy(want)).nonzero()[0]))
    assert off.tolist() == [int(c) for c in offsets], where
    if where == "device":
        assert x.device.index == 0 and mr.data.__dlpack_device__() == (10, 0)
        try:
            memoryview(mr.data)
            raise SystemExit("a device column exported a host buffer")
        except BufferError:
            pass
    if rows is not None:
        assert mr.tolist() == rows, where
    return x

uni_cuts = np.arange(nh + 1, dtype=np.int64) * L
for mk, ov in ((0, False), (0, True), (1, False), (2, False)):
    o = Oracle(pats, mk, KIND_DFA)
    b = ar.BytesAhoCorasick(pats, matchkind=kinds[mk])
    s = ar.AhoCorasick([p.decode() for p in pats], matchkind=kinds[mk])
    uniform = [hay[i * L:(i + 1) * L].tobytes() for i in range(nh)]
    ragged = [hay[cuts[i]:cuts[i + 1]].tobytes() for i in range(len(lens))]
    wu, wr = cover(o, uniform, ov, 42, False), cover(o, ragged, ov, 42, False)
    mu, mr_ = cover(o, uniform, ov, 1, True), cover(o, ragged, ov, 1, True)
    d_cuts = torch.from_numpy(cuts).to("cuda:0")
    rows_u = [wu[i * L:(i + 1) * L].tobytes() for i in range(nh)]
    rows_r = [wr[cuts[i]:cuts[i + 1]].tobytes() for i in range(len(lens))]
    for obj, fill, text in ((b, 42, False), (s, "*", True)):
        x = check(obj.mask_all_batch(t, fill, overlapping=ov, row_length=L), wu, uni_cuts, "device",
                  [r.decode() for r in rows_u] if text else rows_u)   # a tensor in HBM: the result stays there
        # the caller's own offsets cut the result: the layout is the input's
        for i in (2, 3, 7, 11):
            assert torch.equal(x[cuts[i]:cuts[i + 1]].cpu(), torch.from_numpy(wu[cuts[i]:cuts[i + 1]]))
        check(obj.mask_all_batch(t, fill, ov, offsets=d_cuts), wr, cuts, "device", [r.decode() for r in rows_r] if text else rows_r)
        m = check(obj.match_mask_batch(t, overlapping=ov, row_length=L), mu, uni_cuts, "device")
        check(obj.match_mask_batch(t, ov, offsets=d_cuts), mr_, cuts, "device")
        # the same mask from the columns, made in torch: +1 at every start, -1 at every end, a running sum
        mc = obj.find_matches_as_columns_batch(uniform if not text else [u.decode() for u in uniform], overlapping=ov)
        st, en, ro = (torch.from_dlpack(c).to("cuda:0") for c in (mc.start, mc.end, mc.row_offsets))
        row = torch.repeat_interleave(torch.arange(nh, device="cuda:0"), ro[1:] - ro[:-1])
        edge = torch.zeros(L * nh + 1, dtype=torch.int64, device="cuda:0")
        edge.index_add_(0, row * L + st, torch.ones_like(st))
        edge.index_add_(0, row * L + en, -torch.ones_like(en))
        assert torch.equal((edge.cumsum(0)[:-1] > 0).to(torch.uint8), m)
    check(b.mask_all_batch(torch.from_numpy(hay), 42, overlapping=ov, row_length=L), wu, uni_cuts, "host", rows_u)
    check(b.mask_all_batch(torch.from_numpy(hay), b"*", overlapping=ov, offsets=torch.from_numpy(cuts)), wr, cuts, "host", rows_r)
    check(b.match_mask_batch(uniform, overlapping=ov), mu, uni_cuts, "host")
    for i in (0, 2, 7, 60):  # the single forms agree
        assert b.mask_all(uniform[i], 42, overlapping=ov) == rows_u[i] and s.mask_all(uniform[i].decode(), "*", ov) == rows_u[i].decode()
        assert b.match_mask(uniform[i], ov) == mu[i * L:(i + 1) * L].tobytes()

o, b = Oracle(pats, 0, KIND_DFA), ar.BytesAhoCorasick(pats)
uniform = [hay[i * L:(i + 1) * L].tobytes() for i in range(nh)]
want = cover(o, uniform, False, 42, False)
# an odd device address; the consumer on a stream of its own
side = torch.cuda.Stream()
odd = [hay[5 + i * L:5 + (i + 1) * L].tobytes() for i in range(100)]
with torch.cuda.stream(side):
    x = check(b.mask_all_batch(t[5:5 + 100 * L], 42, row_length=L), cover(o, odd, False, 42, False), np.arange(101) * L, "device")
    stars = (x == 42).sum()
assert int(stars) == int((cover(o, odd, False, 42, False) == 42).sum())

# a case-insensitive handle keeps the case of the bytes it leaves alone
ci = ar.BytesAhoCorasick([b"NeEdLe"], ascii_case_insensitive=True)
ct = torch.from_numpy(np.frombuffer(b"A nEEdle, a Needle. " * 50, dtype=np.uint8).copy()).to("cuda:0")
assert bytes(torch.from_dlpack(ci.mask_all_batch(ct, 32, row_length=20).data).cpu().numpy()) == (b"A " + b" " * 6 + b", a " + b" " * 6 + b". ") * 50
assert bytes(ct.cpu().numpy()) == b"A nEEdle, a Needle. " * 50

# str with multi-byte characters in HBM: byte for byte
sm = ar.AhoCorasick(["é", "€uro", "ab"])
u = "café ab €uro".encode()
ut = torch.from_numpy(np.frombuffer(u * 3, dtype=np.uint8).copy()).to("cuda:0")
r = sm.mask_all_batch(ut, "#", row_length=len(u))
assert r.tolist() == ["caf## ## ######"] * 3 and r.nbytes == 3 * len(u) and r.device == 0
assert sm.match_mask_batch(ut, row_length=len(u)).tolist() == [bytes([0, 0, 0, 1, 1, 0, 1, 1, 0, 1, 1, 1, 1, 1, 1])] * 3

def raises(exc, call):
    try:
        call()
    except exc:
        return
    raise SystemExit("no %s" % exc.__name__)
raises(TypeError, lambda: b.mask_all_batch(t, 42))                                   # neither offsets nor row_length
raises(TypeError, lambda: b.mask_all_batch(t, 42, row_length=L, offsets=torch.from_numpy(cuts).to("cuda:0")))
raises(ValueError, lambda: b.mask_all_batch(t, 42, offsets=torch.from_numpy(cuts)))  # offsets on another device
raises(ValueError, lambda: b.mask_all_batch(t, 256, row_length=L))
raises(ValueError, lambda: b.match_mask_batch(t, offsets=torch.from_numpy(cuts[:-2].copy()).to("cuda:0")))  # they do not span the tensor
raises(ValueError, lambda: ar.BytesAhoCorasick(pats, matchkind=kinds[1]).mask_all_batch(t, 42, overlapping=True, row_length=L))

# no rows, and rows without a match: the data still becomes a tensor
mr = b.mask_all_batch(torch.zeros(0, dtype=torch.uint8, device="cuda:0"), 42, row_length=7)
assert len(mr) == 0 and mr.tolist() == [] and tuple(torch.from_dlpack(mr.data).shape) == (0,) and torch.from_dlpack(mr.offsets).tolist() == [0]
z = torch.full((1 << 20,), 48, dtype=torch.uint8, device="cuda:0")
assert not torch.from_dlpack(b.match_mask_batch(z, row_length=1 << 10).data).any()
assert torch.equal(torch.from_dlpack(b.mask_all_batch(z, 42, row_length=1 << 10).data), z)

# lifetime: the tensor keeps the result alive after the MaskedRows object, its handle and its input are gone
b2 = ar.BytesAhoCorasick(pats)
t2 = t.clone()
mr = b2.mask_all_batch(t2, 42, row_length=L)
x = torch.from_dlpack(mr.data)
unused = mr.data.__dlpack__()
del mr, unused, b2, t2
gc.collect()
for k in range(6):  # (other results come and go where the bytes would be if they had been given back)
    other = torch.from_numpy(gen.gen_textlike(L * nh, 40 + k, pats).copy()).to("cuda:0")
    keep = b.mask_all_batch(other, 7, row_length=L)
    del keep
gc.collect()
torch.cuda.synchronize()
assert torch.equal(x.cpu(), torch.from_numpy(want))
del x
gc.collect()

# eight threads on one handle, tensors in HBM
errors = []
def run(i):
    try:
        for k in range(3):
            lo = (i * 20 + k) * L
            got = torch.from_dlpack(b.mask_all_batch(t[lo:lo + 20 * L], 42, row_length=L).data)
            assert torch.equal(got.cpu(), torch.from_numpy(want[lo:lo + 20 * L])), (i, k)
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
    """mask_all_batch and match_mask_batch on tensors in HBM with offsets and with row_length, both classes; torch.from_dlpack
    of the data on the automaton's device, cut by the caller's own offsets; the torch form of the mask from the columns gives
    the same bytes; errors; empty results; lifetime; threads.  In a process of its own: torch has to be the first to load the
    HIP runtime."""
    pytest.importorskip("torch")
    p = subprocess.run([sys.executable, "-c", _TENSOR_SCRIPT, ROOT, os.path.join(ROOT, "tests")], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
