"""A search's matches mapped onto token boundaries, on the device (acx_tokens / acx_tokens_device / acx_tokens_rows_device;
label_tokens / label_tokens_batch): the device stage alone at the seams of its tile kernel -- record counts around the tile, a
token owned across a tile boundary by records of two workgroups, rows that span tiles, runs of empty rows on a tile boundary,
the three ways to cut the data into rows, one-byte tokens, one token over everything, records around the threshold of the
cooperative sweep and beyond one sweep, overlapping records whose starts descend inside a tile, odd token counts and
unaligned outputs, token arrays that do not rise -- with guard bytes around both outputs and every input verified unwritten;
parity with the definition through the C ABI for every match kind on host and device inputs; the Python methods with
sequences (str in characters) and with tensors in HBM, torch as the consumer, lifetime and a seeded random loop.  Expected
values come from numpy over synthetic records or from the oracle's matches (tests/oracle_lib.py) and the definition restated
below -- every record against every token, no search -- never from the library; the kernel's seams are read from its header."""
import gc
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import gen
from oracle_lib import KIND_DFA, Oracle

pytestmark = pytest.mark.gpu
capi = pytest.importorskip("ahocorasick_rs_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ahocorasick_rs_amd", "csrc")
FOLD = bytes.maketrans(bytes(range(65, 91)), bytes(range(97, 123)))


def hip_constants(path, names):
    src = open(os.path.join(CSRC, path)).read()
    out = {}
    for n in names:
        m = re.search(r"\b%s\s*=\s*(\d+)\s*[,;]" % n, src)
        assert m, f"{n} is no longer a plain constant of {path}"
        out[n] = int(m.group(1))
    return out


_C = hip_constants("tokens.hpp", ("TOK_THREADS", "TOK_TILE", "TOK_LONG"))
THREADS, TILE, LONG = _C["TOK_THREADS"], _C["TOK_TILE"], _C["TOK_LONG"]
GUARD = 0xC3


def test_constants_are_what_the_sizes_below_assume():
    assert TILE % THREADS == 0 and THREADS % 64 == 0 and TILE >= 256 and 2 <= LONG < THREADS


# ---------------------------------------------------------------------------
# the definition, restated: every record against every token
# ---------------------------------------------------------------------------
def definition(records, counts, offsets, ts, te):
    """A record of row h, clipped to the row, has the global range [off[h] + start', off[h] + end'); it touches token t iff
    ts[t] < g_e and te[t] > g_s; the owner of t is the touching record with the smallest index; pattern[t] = the owner's
    pattern or -1; begin[t] = 1 iff t has an owner and t - 1 has another one or none.  offsets: rows + 1 from 0."""
    rec = np.asarray(records, dtype=np.uint64).reshape(-1, 3)
    ts, te = np.asarray(ts, dtype=np.int64), np.asarray(te, dtype=np.int64)
    T = len(ts)
    owner = np.full(T, -1, dtype=np.int64)
    if len(rec) and T:
        off = np.asarray(offsets, dtype=np.int64)
        row = np.repeat(np.arange(len(counts)), np.asarray(counts, dtype=np.int64))
        assert len(row) == len(rec)
        b, rl = off[row], (off[row + 1] - off[row]).astype(np.uint64)
        e = np.minimum(rec[:, 2], rl)
        s = np.minimum(rec[:, 1], e)
        gs, ge = b + s.astype(np.int64), b + e.astype(np.int64)
        for i in range(len(rec) - 1, -1, -1):  # (from the back: the smallest index is written last)
            if ge[i] > gs[i]:
                owner[(ts < ge[i]) & (te > gs[i])] = i
    pattern = np.where(owner >= 0, rec[:, 0].astype(np.int64)[np.maximum(owner, 0)] if len(rec) else -1, -1).astype(np.int64)
    prev = np.concatenate([[-1], owner[:-1]]) if T else owner
    begin = ((owner >= 0) & (owner != prev)).astype(np.uint8)
    return pattern, begin, owner


def run_stage(length, offsets, uniform, records, counts, ts, te, begin_res=0, pattern_res=0):
    """tokens_rows_device on synthetic records: `length` positions cut by `offsets` (rows + 1, on the device), by `uniform` (a
    row length) or by neither (one row); the pattern column at 8 * pattern_res modulo 16 and the begin column at begin_res
    modulo 16, each between 64 guard bytes -> (pattern, begin); the guards and every input checked unwritten"""
    rec = np.ascontiguousarray(np.asarray(records, dtype=np.uint64).reshape(-1, 3))
    counts = np.ascontiguousarray(np.asarray(counts, dtype=np.uint64))
    ts, te = np.ascontiguousarray(np.asarray(ts, dtype=np.int64)), np.ascontiguousarray(np.asarray(te, dtype=np.int64))
    n, rows, T = len(rec), len(counts), len(ts)
    lead_p, lead_b = 64 + 8 * pattern_res, 64 + begin_res
    img_p = np.full(lead_p + 8 * T + 64, GUARD, dtype=np.uint8)
    img_b = np.full(lead_b + T + 64, GUARD, dtype=np.uint8)
    d_pat, d_beg = capi.DeviceBuffer(len(img_p) + 16).upload(img_p), capi.DeviceBuffer(len(img_b) + 16).upload(img_b)
    assert d_pat.ptr % 16 == 0 and d_beg.ptr % 16 == 0
    d_rec, d_cnt = capi.DeviceBuffer(24 * n + 16), capi.DeviceBuffer(8 * rows + 16)
    d_ts, d_te = capi.DeviceBuffer(8 * T + 16), capi.DeviceBuffer(8 * T + 16)
    if n:
        d_rec.upload(rec.reshape(-1))
    if rows:
        d_cnt.upload(counts)
    if T:
        d_ts.upload(ts)
        d_te.upload(te)
    d_off = None
    if offsets is not None:
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64))
        assert len(off) == rows + 1
        d_off = capi.DeviceBuffer(8 * len(off)).upload(off)
    try:
        capi.tokens_rows_device(length, d_off.ptr if d_off else 0, rows if (d_off or uniform) else 0, uniform, d_rec.ptr if n else 0, n,
                                d_cnt.ptr if rows else 0, d_ts.ptr, d_te.ptr, T, d_pat.ptr + lead_p, d_beg.ptr + lead_b)
        got_p, got_b = d_pat.download(len(img_p)), d_beg.download(len(img_b))
        assert np.array_equal(d_rec.download(24 * n).view(np.uint64), rec.reshape(-1)), "the records were written"
        assert np.array_equal(d_cnt.download(8 * rows).view(np.uint64), counts), "the counts were written"
        assert np.array_equal(d_ts.download(8 * T).view(np.int64), ts) and np.array_equal(d_te.download(8 * T).view(np.int64), te), "the tokens were written"
        if d_off:
            assert np.array_equal(d_off.download(8 * (rows + 1)).view(np.uint64), off), "the offsets were written"
    finally:
        for b in (d_pat, d_beg, d_rec, d_cnt, d_ts, d_te, d_off):
            if b:
                b.free()
    for got, lead, size, name in ((got_p, lead_p, 8 * T, "pattern"), (got_b, lead_b, T, "begin")):
        assert (got[:lead] == GUARD).all(), ("a byte before the column was written", name, int(np.flatnonzero(got[:lead] != GUARD)[-1]) - lead)
        assert (got[lead + size:] == GUARD).all(), ("a byte behind the column was written", name, int(np.flatnonzero(got[lead + size:] != GUARD)[0]))
    return got_p[lead_p:lead_p + 8 * T].copy().view(np.int64), got_b[lead_b:lead_b + T]


def check_stage(lens, records, counts, ts, te, what=None, form="offsets", **kw):
    """lens: the rows' lengths (form "offsets": cut by device offsets; "uniform": they are all equal and the row length cuts;
    "one": a single row, cut by nothing)"""
    offsets = np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.int64)
    assert len(lens) == len(counts)
    if form == "uniform":
        assert len(set(int(x) for x in lens)) == 1
    if form == "one":
        assert len(lens) == 1
    got_p, got_b = run_stage(int(offsets[-1]), offsets if form == "offsets" else None, int(lens[0]) if form == "uniform" else 0, records,
                             counts, ts, te, **kw)
    want_p, want_b, owner = definition(records, counts, offsets, ts, te)
    for got, want, name in ((got_p, want_p, "pattern"), (got_b, want_b, "begin")):
        if not np.array_equal(got, want):
            bad = int(np.flatnonzero(got != want)[0])
            raise AssertionError((what, form, kw, name, "tokens", len(want), "first difference at token", bad, "whose owner is record",
                                  int(owner[bad]), got[max(bad - 4, 0):bad + 8].tolist(), want[max(bad - 4, 0):bad + 8].tolist()))
    return want_p, want_b, owner


def tokens_over(length, seed, longest=8, shortest=1):
    """a partition of [0, length) into tokens of seeded lengths shortest .. longest"""
    rng = np.random.default_rng(seed)
    cuts = np.cumsum(rng.integers(shortest, longest + 1, size=length // max(shortest, 1) + 2))
    cuts = np.concatenate([[0], cuts[cuts < length], [length]]).astype(np.int64)
    return cuts[:-1], cuts[1:]


def ragged_counts(n, seed, choices=(0, 0, 1, 2, 3, 7, 40)):
    """per-row record counts from `choices` that sum to exactly n (at least one row)"""
    rng = np.random.default_rng(seed)
    out, left = [], n
    while left:
        c = min(int(rng.choice(choices)), left)
        out.append(c)
        left -= c
    return out or [0]


def records_in(lens, counts, seed, lengths=(1, 1, 2, 3, 5, 8, 13, 16, 17, 31, 40), beyond=False, overlapping=False):
    """counts[h] records in row h of lens[h] positions, random starts, ordered within a row as a search reports them (by start;
    overlapping: by end, so that starts do not rise); beyond: a record may end behind its row or begin behind it (the clip)"""
    rng = np.random.default_rng(seed)
    row = np.repeat(np.arange(len(counts)), np.asarray(counts, dtype=np.int64))
    rl = np.asarray(lens, dtype=np.int64)[row]
    start = (rng.random(len(row)) * (rl + (4 if beyond else 0))).astype(np.int64)
    end = start + rng.choice(lengths, size=len(row))
    if not beyond:
        end = np.minimum(end, rl)
    order = np.lexsort((-start, end, row)) if overlapping else np.lexsort((end, start, row))
    return np.stack([rng.integers(0, 1 << 24, size=len(row)), start[order], end[order]], axis=1).astype(np.uint64)


def batch(n, seed, count_choices=(0, 0, 1, 2, 3, 7, 40), row_lens=(0, 1, 50, 130, 300), **kw):
    """a ragged batch with exactly n records -> (lens, records, counts)"""
    counts = ragged_counts(n, seed, count_choices)
    rng = np.random.default_rng(seed + 1)
    lens = rng.choice(row_lens, size=len(counts))
    lens[np.asarray(counts) > 0] += 1  # (a row that has records has a position)
    return lens, records_in(lens, counts, seed + 3, **kw), counts


# ---------------------------------------------------------------------------
# the stage alone
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_stage_record_counts_around_the_tile(n):
    for k, choices in enumerate(((0, 0, 1, 2, 3, 7, 40), (0, 1, 300, 700), (1,))):
        lens, rec, counts = batch(n, n + 10 * k, choices)
        check_stage(lens, rec, counts, *tokens_over(int(lens.sum()), n + k), ("ragged", n, choices))
    lens, rec, counts = batch(n, n + 50, beyond=True)
    check_stage(lens, rec, counts, *tokens_over(int(lens.sum()), n + 5), ("clipped", n))
    rec = records_in([5000], [n], n + 40)
    check_stage([5000], rec, [n], *tokens_over(5000, n + 6), ("one row holds everything", n), form="one")
    check_stage([0, 0, 5000, 0], records_in([0, 0, 5000, 0], [0, 0, n, 0], n + 50), [0, 0, n, 0], *tokens_over(5000, n + 7),
                ("one row between empty ones", n))
    rows = max(n // 3, 1)
    counts = [3] * (rows - 1) + [n - 3 * (rows - 1)] if n >= 3 else [n]
    lens = [40] * len(counts)
    check_stage(lens, records_in(lens, counts, n + 60), counts, *tokens_over(40 * len(counts), n + 8), ("uniform rows", n), form="uniform")


def test_a_token_shared_across_a_tile_boundary_goes_to_the_lower_index():
    """records 4 i .. 4 i + 5 in one row, tokens of four positions at an offset of one: token k is touched by records k - 1 and
    k and by no other, records TILE - 1 and TILE (two workgroups) among them, and the lower index has to win whichever comes
    first"""
    n = 2 * TILE + 3
    rec = np.stack([np.arange(n) + 100, 4 * np.arange(n), 4 * np.arange(n) + 5], axis=1).astype(np.uint64)
    length = 4 * n + 8
    cuts = np.concatenate([[0], np.arange(1, length, 4), [length]]).astype(np.int64)
    for form, lens, counts in (("one", [length], [n]), ("offsets", [0, length, 0], [0, n, 0])):
        want_p, _, owner = check_stage(lens, rec, counts, cuts[:-1], cuts[1:], "chained", form=form)
        for edge in (TILE, 2 * TILE):
            shared = [t for t in range(len(owner)) if cuts[t] < rec[edge - 1, 2] and cuts[t + 1] > rec[edge, 1]]
            assert shared and all(owner[t] == edge - 1 and want_p[t] == 100 + edge - 1 for t in shared)
    # ONE token under the records of every tile: record 0 owns it
    want_p, want_b, _ = check_stage([length], rec, [n], [0], [length], "one token over the whole buffer", form="one")
    assert want_p.tolist() == [100] and want_b.tolist() == [1]
    # ... and when the first records are empty or clipped away, the first live one
    dead = rec.copy()
    dead[:TILE + 1, 2] = dead[:TILE + 1, 1]
    want_p, _, _ = check_stage([length], dead, [n], [0], [length], "the first tile touches nothing", form="one")
    assert want_p.tolist() == [100 + TILE + 1]


def test_rows_that_span_tiles_and_empty_rows_on_a_tile_boundary():
    # a row of 2.5 tiles between small ones; runs of empty rows exactly where a tile ends
    for counts in ([3, 2 * TILE + TILE // 2, 5], [TILE] + [0] * 300 + [TILE] + [0] * 5 + [7], [0] * 40 + [TILE - 1, 1] + [0] * 600 + [1, TILE],
                   [TILE // 2] * 5 + [0] * 1000):
        lens = [0 if c == 0 else 9000 if c > 100 else 70 for c in counts]
        rec = records_in(lens, counts, len(counts))
        ts, te = tokens_over(int(sum(lens)), len(counts) + 1)
        check_stage(lens, rec, counts, ts, te, ("rows across tiles", counts[:3], len(counts)))
    # empty rows that hold positions (no records) between rows with records, uniform cut
    counts = ([TILE // 4] + [0] * 3) * 9
    lens = [256] * len(counts)
    check_stage(lens, records_in(lens, counts, 5), counts, *tokens_over(256 * len(counts), 9), "uniform with recordless rows", form="uniform")


@pytest.mark.parametrize("form", ["offsets", "uniform", "one"])
def test_the_three_row_cuts_and_one_byte_tokens(form):
    counts = {"offsets": [0, 500, 0, 0, 700, 3, TILE], "uniform": [300] * 8, "one": [TILE + 200]}[form]
    lens = {"offsets": [5, 900, 0, 17, 1200, 40, 3000], "uniform": [640] * 8, "one": [4000]}[form]
    total = int(sum(lens))
    for ov in (False, True):
        rec = records_in(lens, counts, 11 + ov, beyond=True, overlapping=ov)
        check_stage(lens, rec, counts, np.arange(total), np.arange(total) + 1, ("one-byte tokens", ov), form=form)
        check_stage(lens, rec, counts, *tokens_over(total, 3, longest=8), ("1 .. 8", ov), form=form)
        check_stage(lens, rec, counts, *tokens_over(total, 4, longest=3, shortest=0), ("empty tokens among them", ov), form=form)
        check_stage(lens, rec, counts, [0], [total], ("one token", ov), form=form)
    # tokens with gaps, and a head and a tail that no token covers
    ts = np.arange(7, total - 9, 5)
    check_stage(lens, rec, counts, ts, ts + 3, "gaps", form=form)


def test_records_around_the_sweep_threshold_and_beyond_one_sweep():
    """one-byte tokens: a record of k positions touches k tokens -- k around TOK_LONG (the thread's own atomics against the
    listed form), around one sweep of the workgroup and several of them; long records that overlap one another and short ones"""
    ks = [LONG - 1, LONG, LONG + 1, THREADS - 1, THREADS, THREADS + 1, 2 * THREADS + 3, 5 * THREADS + 1]
    total = 16_000
    rec, at = [], 3
    for k in ks:
        rec.append((k, at, at + k))
        at += k + 2
    assert at < total
    tok = np.arange(total)
    check_stage([total], rec, [len(rec)], tok, tok + 1, "disjoint", form="one")
    # the same lengths nested in one another and crossed by short records, more than one listed record per tile
    rec = [(k, 100 + i, 100 + i + k) for i, k in enumerate(ks)] + [(9, s, s + 2) for s in range(90, 1500, 7)]
    rec.sort(key=lambda r: (r[2], -r[1]))
    check_stage([total], rec, [len(rec)], tok, tok + 1, "nested", form="one")
    check_stage([total], rec, [len(rec)], *tokens_over(total, 1, longest=2), "nested, tokens of 1 .. 2", form="one")
    # tokens of four positions: the threshold counts TOKENS, not positions
    cuts = np.arange(0, total + 1, 4)
    rec = [(k, 8 + 4000 * i + 1, 8 + 4000 * i + 1 + 4 * (LONG - 2 + i) + 2) for i, k in enumerate((1, 2, 3))]  # LONG - 1, LONG, LONG + 1 tokens
    _, _, owner = check_stage([total], rec, [3], cuts[:-1], cuts[1:], "threshold in tokens", form="one")
    assert [int((owner == i).sum()) for i in range(3)] == [LONG - 1, LONG, LONG + 1]
    # every record of a full tile is a listed one
    rec = [(i, 3 * i, 3 * i + LONG + 5) for i in range(TILE + 7)]
    check_stage([total], rec, [len(rec)], tok, tok + 1, "a tile of listed records", form="one")


def test_overlapping_records_whose_starts_descend_inside_a_tile():
    """an overlapping find's order is by end: the LAST record of a tile may begin before all the others, so the tile's bracket
    is a reduction and not its first record's start"""
    total = 60_000
    rec = [(i, 50_000 + i, 50_000 + i + 3) for i in range(TILE - 2)] + [(7, 10, 50_000 + TILE + 5), (8, 5, 50_000 + TILE + 6)]
    rec += [(i, 100 + 2 * i, 50_000 + TILE + 10 + i) for i in range(40)]  # the next tile: every record begins far in front
    ts, te = tokens_over(total, 2)
    check_stage([total], rec, [len(rec)], ts, te, "descending starts", form="one")
    check_stage([total // 2, total // 2], rec, [len(rec), 0], ts, te, "descending starts, clipped at the row")
    lens, r, counts = batch(2 * TILE + 50, 77, (0, 1, 300, 700), overlapping=True, lengths=(1, 2, 5, 40, 200, 290))
    check_stage(lens, r, counts, *tokens_over(int(lens.sum()), 8), "ragged, by end")


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 7, 1023, 1025])
def test_odd_token_counts_and_unaligned_columns(T):
    total = 4 * T + 3
    counts = [min(T, 40), 0, 3]
    lens = [total - 5, 0, 5]
    rec = records_in(lens, counts, T)
    cuts = np.linspace(0, total, T + 1).astype(np.int64)
    for begin_res in (0, 1, 2, 3, 5):
        for pattern_res in (0, 1):
            check_stage(lens, rec, counts, cuts[:-1], cuts[1:], ("T", T), begin_res=begin_res, pattern_res=pattern_res)


def test_token_arrays_that_do_not_rise_write_nothing_outside_the_columns():
    """the arrays are the caller's word: the labels are then whatever they are, but no store leaves the T entries (the guards)
    and no input is written"""
    rng = np.random.default_rng(20261021)
    lens, rec, counts = batch(2 * TILE + 9, 31, (0, 1, 300, 700))
    total = int(lens.sum())
    offsets = np.concatenate([[0], np.cumsum(lens)])
    for T in (1, 5, 1000, 4097):
        for kind in ("random", "descending", "huge", "negative", "ends before starts"):
            if kind == "random":
                ts, te = rng.integers(0, total + 1, size=T), rng.integers(0, total + 1, size=T)
            elif kind == "descending":
                ts = np.linspace(total, 0, T).astype(np.int64)
                te = ts + 3
            elif kind == "huge":
                ts, te = rng.integers(0, 1 << 62, size=T), rng.integers(0, 1 << 62, size=T)
            elif kind == "negative":
                ts, te = -rng.integers(1, total + 1, size=T), rng.integers(0, total + 1, size=T)
            else:
                te = np.sort(rng.integers(0, total + 1, size=T))
                ts = te + rng.integers(1, 9, size=T)
            p, b = run_stage(total, offsets, 0, rec, counts, ts, te, begin_res=T % 4)
            assert len(p) == T and len(b) == T and ((p == -1) | ((p >= 0) & (p < 1 << 24))).all() and (b <= 1).all(), (T, kind)


def test_no_record_no_row_no_token_and_refusals():
    ts, te = tokens_over(100, 1)
    for lens, counts, form in (([100], [0], "one"), ([60, 40], [0, 0], "offsets"), ([50, 50], [0, 0], "uniform")):
        p, b, _ = check_stage(lens, [], counts, ts, te, "no record", form=form)
        assert (p == -1).all() and not b.any()
    p, b = run_stage(0, [0, 0], 0, [], [0], [0, 0, 0], [0, 0, 0])   # no position: the fills
    assert p.tolist() == [-1, -1, -1] and b.tolist() == [0, 0, 0]
    p, b = run_stage(100, None, 0, [(1, 0, 9)], [1], [], [])        # no token: nothing at all
    assert len(p) == 0 and len(b) == 0
    d = capi.DeviceBuffer(8192)
    d.upload(np.zeros(1024, dtype=np.uint64))
    d.upload(np.asarray([2, 1], dtype=np.uint64))                                                          # the counts of two rows: 3 records
    capi.lib().acx_device_upload(d.ptr + 512, np.asarray([0, 40, 100], dtype=np.uint64).ctypes.data, 24)  # their offsets
    capi.lib().acx_device_upload(d.ptr + 2048, np.asarray([0, 50], dtype=np.int64).ctypes.data, 16)       # two tokens
    capi.lib().acx_device_upload(d.ptr + 2560, np.asarray([50, 100], dtype=np.int64).ctypes.data, 16)
    args = dict(nbytes=100, d_offsets=d.ptr + 512, n_hay=2, uniform_len=0, d_records=d.ptr + 1024, n=3, d_counts=d.ptr, d_ts=d.ptr + 2048,
                d_te=d.ptr + 2560, n_tokens=2, d_pattern=d.ptr + 4096, d_begin=d.ptr + 5001)
    capi.tokens_rows_device(**args)
    capi.tokens_rows_device(**{**args, "d_offsets": 0, "uniform_len": 50})
    capi.tokens_rows_device(**{**args, "d_offsets": 0, "n_hay": 0, "n": 2, "d_counts": d.ptr})           # one row of two records
    for change in (dict(n=4), dict(n=2), dict(d_records=d.ptr + 1028), dict(d_counts=d.ptr + 4), dict(d_offsets=d.ptr + 516),
                   dict(d_ts=d.ptr + 2052), dict(d_te=d.ptr + 2564), dict(d_pattern=d.ptr + 4100), dict(d_pattern=0), dict(d_begin=0),
                   dict(d_ts=0), dict(d_te=0), dict(d_counts=0), dict(d_records=0), dict(uniform_len=50), dict(d_offsets=0, uniform_len=7),
                   dict(nbytes=99), dict(nbytes=101), dict(d_offsets=d.ptr + 520, n_hay=1)):
        with pytest.raises(ValueError) as ei:
            capi.tokens_rows_device(**{**args, **change})
        assert ei.value.code == capi.EINVAL, change
    with pytest.raises(ValueError) as ei:
        capi.tokens_rows_device(**{**args, "n_tokens": 1 << 32})
    assert ei.value.code == capi.ETOOBIG
    d.free()


# ---------------------------------------------------------------------------
# end to end through the C ABI against the oracle
# ---------------------------------------------------------------------------
PATS = gen.gen_patterns(500, 3, 9, gen.AZ, 5) + [b"ab", b"abab", b"bab", b"ab"]
KINDS = [(0, False), (0, True), (1, False), (2, False)]


def oracle_labels(o, hays, ov, ts, te, search=None):
    """the definition from the oracle's matches: every row's records behind one another, the rows' offsets in bytes"""
    rec, counts = [], []
    for i, h in enumerate(hays):
        m = np.asarray(o.find_raw(h if search is None else search[i], overlapping=ov), dtype=np.uint64).reshape(-1, 3)
        rec.append(m)
        counts.append(len(m))
    offsets = np.concatenate([[0], np.cumsum([len(h) for h in hays])]).astype(np.int64)
    return definition(np.concatenate(rec) if rec else np.zeros((0, 3), np.uint64), counts, offsets, ts, te)[:2]


def download(ptr, n, dtype):
    out = np.empty(n, dtype=dtype)
    if n:
        capi._check(capi.lib().acx_device_download(out.ctypes.data, ptr, out.nbytes))
    return out


def check_labels(l, want, on_device, what=None):
    """a capi.DeviceTokenLabels against the definition, through the copies and through the raw addresses"""
    want_p, want_b = want
    assert l.on_device == on_device and l.count == len(want_p), (what, l.count, len(want_p))
    for got, w, name in ((l.pattern(), want_p, "pattern"), (l.begin(), want_b, "begin")):
        if not np.array_equal(got, w):
            bad = int(np.flatnonzero(got != w)[0])
            raise AssertionError((what, name, "first difference at token", bad, got[max(bad - 4, 0):bad + 8].tolist(), w[max(bad - 4, 0):bad + 8].tolist()))
    p, q = l.pattern_ptr(), l.begin_ptr()
    assert p and q and p % 8 == 0, what  # (an empty part still has an address)
    if on_device:
        assert np.array_equal(download(p, len(want_p), np.int64), want_p) and np.array_equal(download(q, len(want_b), np.uint8), want_b), what
    else:
        assert np.array_equal(np.ctypeslib.as_array((capi.ctypes.c_int64 * max(len(want_p), 1)).from_address(p))[:len(want_p)], want_p)
    l.free()


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
    """the batch behind one another in HBM at `off` modulo 16, ragged offsets and the token arrays on the device"""

    def __init__(self, hays, ts, te, off=0):
        blob = b"".join(hays)
        offs = np.concatenate([[0], np.cumsum([len(h) for h in hays])]).astype(np.uint64)
        self.blob, self.lead = blob, off
        self.ts, self.te = np.ascontiguousarray(ts, dtype=np.int64), np.ascontiguousarray(te, dtype=np.int64)
        self.hay = capi.DeviceBuffer(len(blob) + 32).upload(np.frombuffer(b"\xa5" * off + blob, dtype=np.uint8))
        self.off = capi.DeviceBuffer(8 * len(offs)).upload(offs)
        self.d_ts = capi.DeviceBuffer(8 * len(self.ts) + 16).upload(self.ts)
        self.d_te = capi.DeviceBuffer(8 * len(self.te) + 16).upload(self.te)
        self.args = (self.hay.ptr + off, len(blob), self.d_ts.ptr, self.d_te.ptr, len(self.ts))
        self.kw = dict(d_offsets=self.off.ptr, n_hay=len(hays))

    def free(self):
        got = self.hay.download(self.lead + len(self.blob))  # (the caller's bytes stay the caller's)
        assert got[self.lead:].tobytes() == self.blob and (got[:self.lead] == 0xA5).all()
        assert np.array_equal(self.d_ts.download(8 * len(self.ts)).view(np.int64), self.ts)
        assert np.array_equal(self.d_te.download(8 * len(self.te)).view(np.int64), self.te)
        for b in (self.hay, self.off, self.d_ts, self.d_te):
            b.free()


@pytest.mark.parametrize("mk,ov", KINDS)
def test_parity_host_and_device_inputs(mk, ov):
    o = Oracle(PATS, mk, KIND_DFA)
    a = capi.Automaton(PATS, mk)
    for n_hay in (1, 65, 200):
        hays = batch_with_empties(PATS, n_hay, 100 + n_hay)
        total = sum(len(h) for h in hays)
        for ts, te in (tokens_over(total, n_hay), tokens_over(total, n_hay + 1, longest=3, shortest=0)):  # (tokens cross rows)
            want = oracle_labels(o, hays, ov, ts, te)
            assert n_hay == 1 or (want[0] >= 0).any()
            check_labels(a.tokens(hays, ts, te, ov), want, False, (mk, ov, n_hay))   # host route ...
            for off in (0, 5):
                d = OnDevice(hays, ts, te, off)
                check_labels(a.tokens_device(*d.args, overlapping=ov, **d.kw), want, True, (mk, ov, n_hay, off))  # ... == device route
                d.free()
    # a uniform batch on the device, and the same bytes as a host batch; one haystack that is no batch
    L, nh = 512, 130
    full = gen.gen_textlike(L * nh, 61, PATS).tobytes()
    hays = [full[i * L:(i + 1) * L] for i in range(nh)]
    ts, te = tokens_over(len(full), 5)
    want = oracle_labels(o, hays, ov, ts, te)
    d = OnDevice([full], ts, te)
    check_labels(a.tokens_device(*d.args, n_hay=nh, uniform_len=L, overlapping=ov), want, True, "uniform")
    check_labels(a.tokens(hays, ts, te, ov), want, False, "uniform, host")
    one = oracle_labels(o, [full], ov, ts, te)
    check_labels(a.tokens_device(*d.args, overlapping=ov), one, True, "single, device")
    check_labels(a.tokens(None, ts, te, ov, single=full), one, False, "single")
    d.free()
    a.close()


def test_empty_batches_errors_and_the_overlapping_check():
    a = capi.Automaton(PATS, 0)
    none = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint8))
    check_labels(a.tokens([], [], []), none, False, "empty batch")
    check_labels(a.tokens([b"", b""], [0, 0], [0, 0]), (np.full(2, -1, dtype=np.int64), np.zeros(2, dtype=np.uint8)), False, "empty rows only")
    check_labels(a.tokens([b"xxabxx"], [], []), none, False, "no token")
    dev = capi.DeviceBuffer(64).upload(np.zeros(8, dtype=np.int64))
    check_labels(a.tokens_device(dev.ptr, 0, dev.ptr, dev.ptr, 3, n_hay=0, uniform_len=8), (np.full(3, -1, dtype=np.int64), np.zeros(3, dtype=np.uint8)),
                 True, "empty batch, device")
    check_labels(a.tokens_device(dev.ptr, 8, 0, 0, 0), none, True, "no token, device")
    for call in (lambda: a.tokens([b"abab"], [0, 3], [4, 4]), lambda: a.tokens([b"abab"], [0], [5]), lambda: a.tokens([b"abab"], [2, 0], [3, 1]),
                 lambda: a.tokens_device(dev.ptr, 8, dev.ptr + 4, dev.ptr, 1), lambda: a.tokens_device(dev.ptr, 10, dev.ptr, dev.ptr, 1, n_hay=3, uniform_len=4)):
        with pytest.raises(ValueError) as ei:
            call()
        assert ei.value.code == capi.EINVAL
    for mk in (1, 2):
        b = capi.Automaton([b"ab", b"b"], mk)
        for call in (lambda: b.tokens([b"xxabxx"], [0], [6], overlapping=True), lambda: b.tokens_device(0, 0, 0, 0, 0, n_hay=0, uniform_len=8, overlapping=True)):
            with pytest.raises(ValueError) as ei:
                call()
            assert ei.value.code == capi.EOVERLAP
        b.close()
    dev.free()
    a.close()


def test_long_matches_and_a_case_insensitive_handle():
    pats = [b"ab" * 300 + b"c", b"q" * 5000, b"ab" * 300, b"zz"]   # matches of ~150 and ~1250 tokens: the sweep, from a real find
    hays = [b"x" * 77 + pats[0] + b"yy" + pats[1] + b"zz", b"ab" * 2000 + b"c", b"", b"q" * 4999 + b"zz", b"zz" + b"q" * 12_000]
    ts, te = tokens_over(sum(len(h) for h in hays), 3)
    for mk, ov in KINDS:
        o, a = Oracle(pats, mk, KIND_DFA), capi.Automaton(pats, mk)
        want = oracle_labels(o, hays, ov, ts, te)
        assert int((want[0] >= 0).sum()) > 2000
        check_labels(a.tokens(hays, ts, te, ov), want, False, (mk, ov))
        d = OnDevice(hays, ts, te, 9)
        check_labels(a.tokens_device(*d.args, overlapping=ov, **d.kw), want, True, (mk, ov))
        d.free()
        a.close()
    pats = [b"Needle", b"hay", b"STACK"]
    o = Oracle([p.translate(FOLD) for p in pats], 1, KIND_DFA)
    hays = [b"a nEEdle in a HayStack; " * 3, b"Nothing Here", b"", b"NEEDLE", b"x" * 5000 + b"hAY", b"NO", b"needle HAY stack Xyz" * 900]
    ts, te = tokens_over(sum(len(h) for h in hays), 4)
    want = oracle_labels(o, hays, False, ts, te, search=[h.translate(FOLD) for h in hays])
    assert (want[0][:6] >= 0).any()
    a = capi.Automaton(pats, 1, ascii_case_insensitive=True)
    check_labels(a.tokens(hays, ts, te), want, False, "case-insensitive")
    d = OnDevice(hays, ts, te, 5)
    check_labels(a.tokens_device(*d.args, **d.kw), want, True, "case-insensitive, device")
    d.free()
    a.close()


def test_seeded_random_shapes():
    rng = random.Random(20261021)
    for case in range(50):
        mk = rng.choice([0, 0, 1, 2])
        ov = mk == 0 and rng.random() < 0.4
        alpha = rng.choice([b"ab", b"abcd", gen.AZ])
        pats = gen.gen_patterns(rng.choice([1, 3, 40, 600]), 1, rng.choice([2, 6, 12]), alpha, 1000 + case)
        text_ = rng.choice([alpha, alpha + b"xyz", b"0123"])
        o = Oracle(pats, mk, KIND_DFA)
        n_hay = rng.choice([1, 2, 7, 64, 65, 130])
        hays = [bytes(rng.choices(text_, k=rng.choice([0, 0, 1, 9, 200, 2000]))) for _ in range(n_hay)]
        while sum(len(o.find_raw(h, overlapping=ov)) for h in hays) > 20_000:  # (cut down, never skipped)
            hays = [h[:len(h) // 2] for h in hays]
        total = sum(len(h) for h in hays)
        ts, te = tokens_over(total, case, longest=rng.choice([1, 4, 8, 64]), shortest=rng.choice([0, 1]))
        if rng.random() < 0.3 and len(ts) > 4:   # gaps: every third token goes
            keep = np.arange(len(ts)) % 3 != 1
            ts, te = ts[keep], te[keep]
        want = oracle_labels(o, hays, ov, ts, te)
        route = rng.choice(["host", "device", "device"])
        a = capi.Automaton(pats, mk)
        what = (case, mk, ov, n_hay, route, len(ts))
        try:
            if route == "device":
                d = OnDevice(hays, ts, te, rng.randrange(16))
                check_labels(a.tokens_device(*d.args, overlapping=ov, **d.kw), want, True, what)
                d.free()
            else:
                check_labels(a.tokens(hays, ts, te, ov), want, False, what)
        except AssertionError as e:
            raise AssertionError(f"case {what}: {e}") from e
        a.close()


# ---------------------------------------------------------------------------
# the Python methods: sequences of host objects (tensors in HBM and torch as the consumer: the script below)
# ---------------------------------------------------------------------------
def matchkind(ar, mk):
    return (ar.MatchKind.Standard, ar.MatchKind.LeftmostFirst, ar.MatchKind.LeftmostLongest)[mk]


def local_tokens(lengths, seed, longest=8):
    """per row the local boundaries of a partition into tokens of 1 .. longest"""
    out = []
    for i, n in enumerate(lengths):
        ts, te = tokens_over(n, seed + i, longest=longest)
        out.append([0] + [int(x) for x in te] if n else [0])
    return out


def global_tokens(local, lengths):
    ts, te, base = [], [], 0
    for b, n in zip(local, lengths):
        ts += [base + x for x in b[:-1]]
        te += [base + x for x in b[1:]]
        base += n
    return np.asarray(ts, dtype=np.int64), np.asarray(te, dtype=np.int64)


def check_token_labels(tl, want, local):
    """a TokenLabels in host memory against the definition; tolist() is one list per row"""
    want_p, want_b = want
    ro = np.concatenate([[0], np.cumsum([len(b) - 1 for b in local])]).astype(np.int64)
    assert len(tl) == len(want_p) and tl.device is None and tl.row_offsets == [int(x) for x in ro]
    rows = [[(int(p), int(b)) for p, b in zip(want_p[ro[h]:ro[h + 1]], want_b[ro[h]:ro[h + 1]])] for h in range(len(local))]
    assert tl.tolist() == rows
    pat, beg = tl.pattern, tl.begin
    assert len(pat) == len(want_p) and len(beg) == len(want_b) and pat.__dlpack_device__() == (1, 0)
    assert np.from_dlpack(pat).dtype == np.int64 and np.array_equal(np.from_dlpack(pat), want_p)
    assert np.from_dlpack(beg).dtype == np.uint8 and np.array_equal(np.from_dlpack(beg), want_b)
    assert memoryview(pat).format == "q" and memoryview(beg).format == "B" and memoryview(beg).readonly


@pytest.mark.parametrize("mk,ov", KINDS)
def test_python_sequences_both_classes(mk, ov):
    import ahocorasick_rs as ar
    o = Oracle(PATS, mk, KIND_DFA)
    b = ar.BytesAhoCorasick(PATS, matchkind=matchkind(ar, mk))
    s = ar.AhoCorasick([p.decode() for p in PATS], matchkind=matchkind(ar, mk))
    for n_hay in (0, 1, 64, 130):
        hays = batch_with_empties(PATS, n_hay, 500 + n_hay)
        lengths = [len(h) for h in hays]
        local = local_tokens(lengths, n_hay)
        want = oracle_labels(o, hays, ov, *global_tokens(local, lengths))
        check_token_labels(b.label_tokens_batch(hays, local, overlapping=ov), want, local)
        check_token_labels(b.label_tokens_batch(tuple(bytearray(h) for h in hays), [np.asarray(x, dtype=np.int64) for x in local], ov), want, local)
        check_token_labels(s.label_tokens_batch([h.decode() for h in hays], local, ov), want, local)   # ASCII: characters are bytes
        at = 0
        for h, loc in list(zip(hays, local))[:40]:  # the single forms agree with the rows of the batch
            k = len(loc) - 1
            row = [(int(p), int(x)) for p, x in zip(want[0][at:at + k], want[1][at:at + k])]
            # (a token never crosses a haystack in the sequence form, so a row's labels are the single call's)
            got = b.label_tokens(h, loc, overlapping=ov)
            assert got.tolist() == row and got.row_offsets is None and len(got) == k
            assert s.label_tokens(h.decode(), tuple(loc), ov).tolist() == row
            at += k


def test_python_str_in_characters_with_multi_byte_text():
    """the str class takes token boundaries in CHARACTERS, the unit of find_matches_as_indexes and of a tokenizer's
    offset_mapping; the expected labels come from the oracle's byte matches converted to character indexes"""
    import ahocorasick_rs as ar
    pats = ["é", "€uro", "\U0001F600", "ab", "naïve", "日本"]
    s = ar.AhoCorasick(pats, matchkind=ar.MatchKind.LeftmostLongest)
    o = Oracle([p.encode() for p in pats], 2, KIND_DFA)
    hays = ["café ab €uro \U0001F600!", "", "naïve 日本語 naive", "ascii ab only", "ééé\U0001F600\U0001F600€uro", "€ur"]
    local = [[0, 3, 4, 5, 7, 8, 12, 13, 14, 15], [0], [0, 2, 5, 6, 8, 9, 15], [0, 13], [0, 1, 1, 3, 4, 9], [0, 0, 3]]
    rec, counts = [], []
    for h in hays:
        raw = h.encode()
        char_at = {0: 0}
        for i, c in enumerate(h):
            char_at[len(h[:i + 1].encode())] = i + 1
        m = [(int(p), char_at[int(a)], char_at[int(e)]) for p, a, e in o.find_raw(raw)]
        assert m == [tuple(x) for x in s.find_matches_as_indexes(h)]
        rec += m
        counts.append(len(m))
    lengths = [len(h) for h in hays]
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    want = definition(rec, counts, offsets, *global_tokens(local, lengths))[:2]
    assert want[0][:9].tolist() == [-1, 0, -1, 3, -1, 1, -1, 2, -1]   # caf|é| |ab| |€uro| |😀|!
    check_token_labels(s.label_tokens_batch(hays, local), want, local)
    at = 0
    for h, loc in zip(hays, local):
        k = len(loc) - 1
        assert s.label_tokens(h, loc).tolist() == [(int(p), int(b)) for p, b in zip(want[0][at:at + k], want[1][at:at + k])], h
        at += k
    # the bytes class on the same text takes byte boundaries
    b = ar.BytesAhoCorasick([p.encode() for p in pats], matchkind=ar.MatchKind.LeftmostLongest)
    raw = hays[0].encode()
    got = b.label_tokens(raw, [0, 3, 5, 6, 8, 9, 15, 16, 20, 21]).tolist()
    assert [p for p, _ in got] == [-1, 0, -1, 3, -1, 1, -1, 2, -1]


def test_python_errors_and_host_tensors():
    import ahocorasick_rs as ar
    b, s = ar.BytesAhoCorasick([b"ab", b"X"]), ar.AhoCorasick(["ab", "X"])
    assert b.label_tokens(b"xxabxX", [0, 2, 4, 6]).tolist() == [(-1, 0), (0, 1), (1, 1)]
    assert b.label_tokens(b"xxabxX", [0, 3, 6], overlapping=True).tolist() == [(0, 1), (0, 0)]
    assert s.label_tokens("xxabxX", np.asarray([0, 6], dtype=np.int64)).tolist() == [(0, 1)]
    assert b.label_tokens(b"", [0]).tolist() == [] and b.label_tokens(b"ab", [1, 1]).tolist() == [(0, 1)] and b.label_tokens(b"ab", [2, 2]).tolist() == [(-1, 0)]
    for bad in ([], [0, 3], [1, 0], [-1, 2], [0, 1 << 40]):
        with pytest.raises(ValueError):
            b.label_tokens(b"ab", bad)
        with pytest.raises(ValueError):
            s.label_tokens_batch(["ab"], [bad])
    with pytest.raises(ValueError):
        s.label_tokens("éé", [0, 3])                  # characters, not bytes
    assert s.label_tokens("éé", [0, 2]).tolist() == [(-1, 0)]
    with pytest.raises(ValueError):
        b.label_tokens_batch([b"ab", b"cd"], [[0, 2]])  # one entry per haystack
    for call in (lambda: b.label_tokens(b"ab"), lambda: b.label_tokens(b"ab", [0, 2], 1), lambda: b.label_tokens(b"ab", [0, 2.0]),
                 lambda: b.label_tokens(b"ab", [0, True]), lambda: b.label_tokens(b"ab", 5), lambda: b.label_tokens("ab", [0, 2]),
                 lambda: s.label_tokens(b"ab", [0, 2]), lambda: b.label_tokens(b"ab", np.asarray([0, 2], dtype=np.int32)),
                 lambda: b.label_tokens_batch([b"ab"], [[0, 2]], offsets=np.array([0, 2], dtype=np.int64)),
                 lambda: b.label_tokens(b"ab", [0, 2], row_length=2)):
        with pytest.raises(TypeError):
            call()
    # one host tensor cut into rows: token_offsets is ONE int64 tensor of global byte boundaries, tokens may cross rows
    t = np.frombuffer(b"abxXYxabab", dtype=np.uint8).copy()
    tok = np.asarray([0, 1, 4, 7, 10], dtype=np.int64)
    tl = b.label_tokens_batch(t, tok, row_length=5)
    assert tl.tolist() == [(0, 1), (0, 0), (0, 1), (0, 0)] and tl.row_offsets is None and tl.device is None and len(tl) == 4
    tl = b.label_tokens_batch(t, tok, offsets=np.array([0, 1, 1, 6, 10], dtype=np.int64))   # "a" | "" | "bxXYx" | "abab"
    assert tl.tolist() == [(-1, 0), (1, 1), (0, 1), (0, 0)]
    assert b.label_tokens(t, tok).tolist() == [(0, 1), (0, 0), (0, 1), (0, 0)]
    for call in (lambda: b.label_tokens_batch(t, [0, 10], row_length=5), lambda: b.label_tokens_batch(t, tok.astype(np.int32), row_length=5),
                 lambda: b.label_tokens_batch(t, tok.reshape(1, -1), row_length=5)):
        with pytest.raises(TypeError):
            call()
    for bad in (np.zeros(0, dtype=np.int64), np.asarray([0, 11], dtype=np.int64), np.asarray([3, 2], dtype=np.int64)):
        with pytest.raises(ValueError):
            b.label_tokens_batch(t, bad, row_length=5)
    assert t.tobytes() == b"abxXYxabab"
    for mk in (ar.MatchKind.LeftmostFirst, ar.MatchKind.LeftmostLongest):
        with pytest.raises(ValueError):
            ar.BytesAhoCorasick([b"ab"], matchkind=mk).label_tokens(b"ab", [0, 2], overlapping=True)
    with pytest.raises(TypeError):
        ar.TokenLabels()


def test_host_columns_outlive_the_result_and_the_automaton():
    import ahocorasick_rs as ar
    o, b = Oracle(PATS, 0, KIND_DFA), ar.BytesAhoCorasick(PATS)
    hays = batch_with_empties(PATS, 300, 3)
    lengths = [len(h) for h in hays]
    local = local_tokens(lengths, 7)
    want = oracle_labels(o, hays, False, *global_tokens(local, lengths))
    tl = b.label_tokens_batch(hays, local)
    pat, mv, beg, unused = np.from_dlpack(tl.pattern), memoryview(tl.begin), np.from_dlpack(tl.begin), tl.pattern.__dlpack__()
    del tl, unused, hays, b
    gc.collect()
    other = ar.BytesAhoCorasick(PATS)
    for k in range(20):  # (other results come and go where the columns would be if they had been freed)
        other.label_tokens_batch(batch_with_empties(PATS, 300, 50 + k), local_tokens([len(h) for h in batch_with_empties(PATS, 300, 50 + k)], k))
    assert np.array_equal(pat, want[0]) and np.array_equal(np.asarray(mv), want[1]) and np.array_equal(beg, want[1])


_TENSOR_SCRIPT = r"""
import gc
import sys
import torch  # first: one process holds ONE HIP runtime, and torch must be the one to load it
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
import gen
from oracle_lib import KIND_DFA, Oracle
import ahocorasick_rs as ar
pats = gen.gen_patterns(300, 5, 9, gen.AZ, 5) + [b"abqab", b"abqabqab", b"bqab", b"abqab"]
L, nh = 4096, 40
hay = gen.gen_textlike(L * nh, 13, pats).copy()
hay[3 * L:9 * L] = 48   # (rows without a match)
t = torch.from_numpy(hay.copy()).to("cuda:0")
kinds = (ar.MatchKind.Standard, ar.MatchKind.LeftmostFirst, ar.MatchKind.LeftmostLongest)
lens = [0, 0, 17, L, 3 * L, 5, 0, 2 * L + 1, 4 * L, 7, 0]
lens += [L * nh - sum(lens), 0]
cuts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
rng = np.random.default_rng(5)
tok = np.cumsum(rng.integers(1, 9, size=L * nh // 4))
tok = np.concatenate([[0], tok[tok < L * nh], [L * nh]]).astype(np.int64)   # T + 1 global boundaries, an odd count or not
T = len(tok) - 1

def labels(o, rows, offsets, ov):
    # the definition: every record against every token; the owner is the touching record of the smallest index
    owner = np.full(T, -1, dtype=np.int64)
    rec = []
    for h, row in enumerate(rows):
        for p, s, e in o.find_raw(row, overlapping=ov):
            rec.append((int(p), int(offsets[h]) + int(s), int(offsets[h]) + int(e)))
    for i in range(len(rec) - 1, -1, -1):
        owner[(tok[:-1] < rec[i][2]) & (tok[1:] > rec[i][1])] = i
    pat = np.where(owner >= 0, np.asarray([r[0] for r in rec] + [-1], dtype=np.int64)[owner], -1)
    beg = ((owner >= 0) & (owner != np.concatenate([[-1], owner[:-1]]))).astype(np.uint8)
    return pat, beg

def check(tl, want, where):
    assert tl.device == (0 if where == "device" else None), (where, tl.device)
    assert len(tl) == T and tl.row_offsets is None
    p, b = torch.from_dlpack(tl.pattern), torch.from_dlpack(tl.begin)
    assert p.dtype == torch.int64 and b.dtype == torch.uint8 and tuple(p.shape) == tuple(b.shape) == (T,) and p.is_contiguous()
    assert p.device.type == b.device.type == ("cuda" if where == "device" else "cpu")
    assert torch.equal(p.cpu(), torch.from_numpy(want[0])), (where, int((p.cpu() != torch.from_numpy(want[0])).nonzero()[0]))
    assert torch.equal(b.cpu(), torch.from_numpy(want[1])), (where, int((b.cpu() != torch.from_numpy(want[1])).nonzero()[0]))
    if where == "device":
        assert p.device.index == 0 and tl.pattern.__dlpack_device__() == (10, 0)
        try:
            memoryview(tl.begin)
            raise SystemExit("a device column exported a host buffer")
        except BufferError:
            pass
    return p, b

uni_cuts = np.arange(nh + 1, dtype=np.int64) * L
d_tok, d_cuts = torch.from_numpy(tok).to("cuda:0"), torch.from_numpy(cuts).to("cuda:0")
for mk, ov in ((0, False), (0, True), (1, False), (2, False)):
    o = Oracle(pats, mk, KIND_DFA)
    b = ar.BytesAhoCorasick(pats, matchkind=kinds[mk])
    s = ar.AhoCorasick([p.decode() for p in pats], matchkind=kinds[mk])
    uniform = [hay[i * L:(i + 1) * L].tobytes() for i in range(nh)]
    ragged = [hay[cuts[i]:cuts[i + 1]].tobytes() for i in range(len(lens))]
    wu, wr = labels(o, uniform, uni_cuts, ov), labels(o, ragged, cuts, ov)
    for obj in (b, s):
        p, _ = check(obj.label_tokens_batch(t, d_tok, overlapping=ov, row_length=L), wu, "device")   # a tensor in HBM: the result stays there
        check(obj.label_tokens_batch(t, d_tok, ov, offsets=d_cuts), wr, "device")
        if obj is s or mk == 2:
            continue
        # the same owner's pattern, made in torch from the columns: searchsorted x 2, repeat_interleave, scatter_reduce(amin), gather
        mc = obj.find_matches_as_columns_batch(uniform, overlapping=ov)
        pt, st, en, ro = (torch.from_dlpack(c).to("cuda:0") for c in (mc.pattern, mc.start, mc.end, mc.row_offsets))
        row = torch.repeat_interleave(torch.arange(nh, device="cuda:0"), ro[1:] - ro[:-1])
        gs, ge = row * L + st, row * L + en
        first = torch.searchsorted(d_tok[1:], gs, right=True)
        stop = torch.searchsorted(d_tok[:-1], ge, right=False)
        k = (stop - first).clamp(min=0)
        idx = torch.repeat_interleave(torch.arange(len(gs), device="cuda:0"), k)
        tokens = first[idx] + torch.arange(len(idx), device="cuda:0") - torch.repeat_interleave(torch.cumsum(k, 0) - k, k)
        owner = torch.full((T,), len(gs), dtype=torch.int64, device="cuda:0").scatter_reduce(0, tokens, idx, "amin")
        torch_pat = torch.where(owner < len(gs), torch.cat([pt, pt.new_zeros(1)])[owner], -1)
        assert torch.equal(torch_pat, p)
    check(b.label_tokens_batch(torch.from_numpy(hay), torch.from_numpy(tok), overlapping=ov, row_length=L), wu, "host")
    check(b.label_tokens_batch(torch.from_numpy(hay), torch.from_numpy(tok), ov, offsets=torch.from_numpy(cuts)), wr, "host")
    one = labels(o, [hay.tobytes()], [0], ov)
    check(b.label_tokens(t, d_tok, overlapping=ov), one, "device")   # one haystack, one flat boundary tensor
    check(b.label_tokens(torch.from_numpy(hay), torch.from_numpy(tok), ov), one, "host")

o, b = Oracle(pats, 0, KIND_DFA), ar.BytesAhoCorasick(pats)
uniform = [hay[i * L:(i + 1) * L].tobytes() for i in range(nh)]
want = labels(o, uniform, uni_cuts, False)
# the consumer on a stream of its own
side = torch.cuda.Stream()
with torch.cuda.stream(side):
    p, bg = check(b.label_tokens_batch(t, d_tok, row_length=L), want, "device")
    labelled = (p >= 0).sum()
assert int(labelled) == int((want[0] >= 0).sum())

# a case-insensitive handle searches its folded copy
ci = ar.BytesAhoCorasick([b"NeEdLe"], ascii_case_insensitive=True)
ct = torch.from_numpy(np.frombuffer(b"A nEEdle, a Needle. " * 50, dtype=np.uint8).copy()).to("cuda:0")
ctok = torch.arange(0, 1001, 2, dtype=torch.int64, device="cuda:0")
got = torch.from_dlpack(ci.label_tokens_batch(ct, ctok, row_length=20).pattern).cpu().tolist()
assert got[:10] == [-1, 0, 0, 0, -1, -1, 0, 0, 0, -1] and got == got[:10] * 50
assert bytes(ct.cpu().numpy()) == b"A nEEdle, a Needle. " * 50

def raises(exc, call):
    try:
        call()
    except exc:
        return
    raise SystemExit("no %s" % exc.__name__)
raises(TypeError, lambda: b.label_tokens_batch(t, d_tok))                                  # neither offsets nor row_length
raises(TypeError, lambda: b.label_tokens_batch(t, [0, L * nh], row_length=L))              # a tensor of haystacks takes a tensor of boundaries
raises(TypeError, lambda: b.label_tokens_batch(t, d_tok.to(torch.int32), row_length=L))
raises(ValueError, lambda: b.label_tokens_batch(t, torch.from_numpy(tok), row_length=L))   # boundaries on another device
raises(ValueError, lambda: b.label_tokens_batch(t, d_tok[:0], row_length=L))               # zero entries
raises(ValueError, lambda: b.label_tokens(t, torch.from_numpy(tok)))
raises(ValueError, lambda: ar.BytesAhoCorasick(pats, matchkind=kinds[1]).label_tokens_batch(t, d_tok, overlapping=True, row_length=L))

# no rows, no tokens, rows without a match: the columns still become tensors
tl = b.label_tokens_batch(torch.zeros(0, dtype=torch.uint8, device="cuda:0"), torch.zeros(3, dtype=torch.int64, device="cuda:0"), row_length=7)
assert len(tl) == 2 and tl.tolist() == [(-1, 0), (-1, 0)] and torch.from_dlpack(tl.pattern).tolist() == [-1, -1]
tl = b.label_tokens_batch(t, d_tok[:1], row_length=L)
assert len(tl) == 0 and tl.tolist() == [] and tuple(torch.from_dlpack(tl.pattern).shape) == (0,) and tuple(torch.from_dlpack(tl.begin).shape) == (0,)
z = torch.full((1 << 16,), 48, dtype=torch.uint8, device="cuda:0")
ztok = torch.arange(0, (1 << 16) + 1, 4, dtype=torch.int64, device="cuda:0")
tl = b.label_tokens_batch(z, ztok, row_length=1 << 10)
assert bool((torch.from_dlpack(tl.pattern) == -1).all()) and not torch.from_dlpack(tl.begin).any()

# lifetime: the tensors keep the result alive after the TokenLabels object, its automaton and its inputs are gone
b2 = ar.BytesAhoCorasick(pats)
t2, tok2 = t.clone(), d_tok.clone()
tl = b2.label_tokens_batch(t2, tok2, row_length=L)
p, bg = torch.from_dlpack(tl.pattern), torch.from_dlpack(tl.begin)
unused = tl.pattern.__dlpack__()
del tl, unused, b2, t2, tok2
gc.collect()
for k in range(3):  # (other results come and go where the columns would be if they had been given back)
    other = torch.from_numpy(gen.gen_textlike(L * nh, 40 + k, pats).copy()).to("cuda:0")
    keep = b.label_tokens_batch(other, d_tok, row_length=L)
    del keep
gc.collect()
torch.cuda.synchronize()
assert torch.equal(p.cpu(), torch.from_numpy(want[0])) and torch.equal(bg.cpu(), torch.from_numpy(want[1]))
assert torch.equal(t.cpu(), torch.from_numpy(hay)) and torch.equal(d_tok.cpu(), torch.from_numpy(tok))
print("OK")
"""


def test_tensors_in_and_torch_out():
    """label_tokens_batch and label_tokens on tensors in HBM with offsets and with row_length, both classes; torch.from_dlpack
    of both columns on the automaton's device; the torch form of the owner's pattern from the columns gives the same entries;
    errors; empty results; lifetime after the automaton is dropped.  In a process of its own: torch has to be the first to load
    the HIP runtime."""
    pytest.importorskip("torch")
    p = subprocess.run([sys.executable, "-c", _TENSOR_SCRIPT, ROOT, os.path.join(ROOT, "tests")], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
