"""The matched text and its context, on the device (acx_snippets / acx_snippets_device / acx_snippets_rows_device;
find_matches_as_snippets / find_matches_as_snippets_batch): the device stage alone at the seams of its gather -- record counts
around the scan's levels, segment lengths around the chunk and the tile, every pair of source and output alignment, segments
that end on and beside tile boundaries, empty segments on a boundary and in runs longer than a window, a tile of one-byte
segments, the haystack's first and last bytes, the haystack at every address modulo 16 inside a poisoned buffer -- with guard
words around all five outputs and every input verified unwritten; parity with the definition through the C ABI for every match
kind, on host and device inputs, for finds that were cut or took the dense path; the identities with find_matches_as_strings
and the columns; the Python methods with sequences and with tensors in HBM, torch as the consumer, lifetime, threads and a
seeded random loop.  Expected values come from Python over synthetic records or from the oracle's matches
(tests/oracle_lib.py) pushed through the definition restated below, never from the library; the kernel's seams are read from
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
CONTEXT_MAX = (1 << 63) - 1
UTF8 = 1


def hip_constants(path, names):
    src = open(os.path.join(CSRC, path)).read()
    out = {}
    for n in names:
        m = re.search(r"\b%s\s*=\s*(\d+)\s*[,;]" % n, src)
        assert m, f"{n} is no longer a plain constant of {path}"
        out[n] = int(m.group(1))
    return out


_C = hip_constants("snippets.hpp", ("SNIP_THREADS", "SNIP_TILE", "SNIP_WIN"))
THREADS, T, WIN = _C["SNIP_THREADS"], _C["SNIP_TILE"], _C["SNIP_WIN"]
S = 2048  # replace_scan's items per workgroup (replace.hip RS_THREADS * RS_PER): beyond it the scan has two levels
GUARD = np.int64(-0x3C3C3C3C3C3C3C3D)
FRESH = np.int64(0x7777777777777777)  # what the outputs hold before the call
POISON = 0xF5                          # what lies around the haystack: no haystack of these tests holds it


def test_constants_are_what_the_sizes_below_assume():
    assert T % (16 * THREADS) == 0 and THREADS % 64 == 0 and T >= 256 and WIN >= 16
    src = open(os.path.join(CSRC, "replace.hip")).read()
    assert re.search(r"RS_THREADS = 256, RS_PER = 8\b", src), "the scan's level size is no longer 2048"
    assert (capi.SNIP_DATA, capi.SNIP_OFFSETS, capi.SNIP_PATTERN, capi.SNIP_LEAD, capi.SNIP_ROW_OFFSETS) == (0, 1, 2, 3, 4)


# ---------------------------------------------------------------------------
# the definition (the issue's rule), in Python
# ---------------------------------------------------------------------------
def cut_one(B, s, e, context, utf8):
    """one record in the row B -> (lo, hi, lead)"""
    L = len(B)
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
    return lo, hi, s1 - lo


def definition(records, counts, rows, context, utf8=False):
    """records of all rows behind one another, counts[h] of them row h's, rows: the rows' bytes ->
    (snippets, pattern, lead, row_offsets)"""
    snippets, pattern, lead, ro, at = [], [], [], [0], 0
    for B, c in zip(rows, counts):
        for p, s, e in records[at:at + int(c)]:
            lo, hi, ld = cut_one(B, s, e, context, utf8)
            snippets.append(bytes(B[lo:hi]))
            pattern.append(int(p))
            lead.append(ld)
        at += int(c)
        ro.append(at)
    assert at == len(records) and len(rows) == len(counts)
    return snippets, pattern, lead, ro


# ---------------------------------------------------------------------------
# the stage alone
# ---------------------------------------------------------------------------
def run_stage(records, counts, hay, cut, context=0, flags=0, shift=0, capacity=None):
    """snippets_rows_device on synthetic records.  cut: ("offsets", [..]) | ("uniform", L) | ("single",).  The haystack lies
    `shift` bytes into a poisoned buffer; the four word outputs lie between 8 guard words each, the data between 64 guard
    bytes, all pre-filled -> (code, total, data, offsets, pattern, lead, row_offsets); the guards, the bytes behind the total
    and every input checked unwritten"""
    rec = np.ascontiguousarray(np.asarray(records, dtype=np.uint64).reshape(-1, 3))
    counts = np.ascontiguousarray(np.asarray(counts, dtype=np.uint64))
    hay = bytes(hay)
    assert POISON not in hay
    n, rows = len(rec), len(counts)
    sizes = (n + 1, n, n, rows + 1)  # offsets, pattern, lead, row offsets
    at, words = [], 0
    for w in sizes:
        at.append(words + 8)
        words += 8 + w + 8
    image = np.full(words, GUARD, dtype=np.int64)
    for a, w in zip(at, sizes):
        image[a:a + w] = FRESH
    d_out = capi.DeviceBuffer(image.nbytes + 16).upload(image)
    cap = capacity if capacity is not None else sum(len(x) for x in cut_all(rec, counts, hay, cut, context, flags))
    dimage = np.full(64 + cap + 64, 0xC3, dtype=np.uint8)
    dimage[64:64 + cap] = 0x77
    d_data = capi.DeviceBuffer(len(dimage) + 16).upload(dimage)
    himage = np.full(32 + len(hay) + 48, POISON, dtype=np.uint8)
    himage[16 + shift:16 + shift + len(hay)] = np.frombuffer(hay, dtype=np.uint8)
    d_hay = capi.DeviceBuffer(len(himage)).upload(himage)
    d_rec = capi.DeviceBuffer(24 * n + 16)
    d_cnt = capi.DeviceBuffer(8 * rows + 16)
    offs = np.asarray(cut[1], dtype=np.uint64) if cut[0] == "offsets" else np.zeros(0, dtype=np.uint64)
    d_off = capi.DeviceBuffer(8 * len(offs) + 16)
    if n:
        d_rec.upload(rec.reshape(-1))
    if rows:
        d_cnt.upload(counts)
    if len(offs):
        d_off.upload(offs)
    try:
        assert d_hay.ptr % 16 == 0 and d_data.ptr % 16 == 0
        p = [d_out.ptr + 8 * a for a in at]
        code, total = capi.snippets_rows_device(
            d_rec.ptr if n else 0, n, d_cnt.ptr if rows else 0, rows if cut[0] != "single" else 0, d_hay.ptr + 16 + shift, len(hay),
            d_off.ptr if cut[0] == "offsets" else 0, cut[1] if cut[0] == "uniform" else 0, context, flags, p[0], p[1], p[2], p[3],
            d_data.ptr + 64, cap)
        got = d_out.download(image.nbytes).view(np.int64)
        gdata = d_data.download(len(dimage))
        assert np.array_equal(d_rec.download(24 * n).view(np.uint64), rec.reshape(-1)), "the records were written"
        assert np.array_equal(d_cnt.download(8 * rows).view(np.uint64), counts), "the counts were written"
        assert np.array_equal(d_hay.download(len(himage)), himage), "the haystack or its surroundings were written"
        assert np.array_equal(d_off.download(8 * len(offs)).view(np.uint64), offs), "the offsets were written"
    finally:
        for b in (d_out, d_data, d_hay, d_rec, d_cnt, d_off):
            b.free()
    keep = np.ones(words, dtype=bool)
    for a, w in zip(at, sizes):
        keep[a:a + w] = False
    assert (got[keep] == GUARD).all(), ("a guard word was written", int(np.flatnonzero(keep & (got != GUARD))[0]), at)
    assert (gdata[:64] == 0xC3).all() and (gdata[64 + cap:] == 0xC3).all(), "a guard byte around the data was written"
    stored = min(total, cap) if code == capi.OK else 0
    assert (gdata[64 + stored:64 + cap] == 0x77).all(), ("a byte behind the total was written", total, cap)
    parts = [got[a:a + w].copy() for a, w in zip(at, sizes)]
    return code, total, gdata[64:64 + stored].tobytes(), parts[0], parts[1], parts[2], parts[3]


def rows_of(hay, cut):
    hay = bytes(hay)
    if cut[0] == "single":
        return [hay]
    if cut[0] == "uniform":
        return [hay[i:i + cut[1]] for i in range(0, len(hay), cut[1])]
    return [hay[int(cut[1][h]):int(cut[1][h + 1])] for h in range(len(cut[1]) - 1)]


def cut_all(rec, counts, hay, cut, context, flags):
    return definition([tuple(int(x) for x in r) for r in np.asarray(rec).reshape(-1, 3).tolist()], counts, rows_of(hay, cut), context,
                      bool(flags & UTF8))[0]


def check_stage(records, counts, hay, cut=("single",), context=0, flags=0, shift=0, what=None):
    records = [tuple(int(x) for x in r) for r in records]
    want, want_pat, want_lead, want_ro = definition(records, counts, rows_of(hay, cut), context, bool(flags & UTF8))
    code, total, data, off, pat, lead, ro = run_stage(records, counts, hay, cut, context, flags, shift)
    assert code == capi.OK and total == sum(len(w) for w in want) == len(data), (what, total)
    want_off = np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.int64)
    assert np.array_equal(off, want_off), (what, "offsets", int(np.flatnonzero(off != want_off)[0]))
    blob = b"".join(want)
    if data != blob:
        bad = next(i for i in range(len(blob)) if data[i] != blob[i])
        seg = int(np.searchsorted(want_off, bad, side="right")) - 1
        raise AssertionError((what, shift, "first wrong byte", bad, "of", len(blob), "in segment", seg, "at", int(want_off[seg]), "of length",
                              len(want[seg]), data[max(bad - 4, 0):bad + 8], blob[max(bad - 4, 0):bad + 8]))
    assert POISON not in data
    assert pat.view(np.uint64).tolist() == want_pat and lead.tolist() == want_lead and ro.tolist() == want_ro, what
    return want


def text(n, seed):
    """n bytes that are neither the poison nor a guard: letters, digits"""
    return gen.gen_uniform(n, b"abcdefghijklmnopqrstuvwxyz0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ", seed).tobytes()


def segments(hay_len, lengths, rng, starts=None):
    """one record per wanted length (context 0: the segment is the match), anywhere in a haystack of hay_len bytes"""
    rec = []
    for i, k in enumerate(lengths):
        s = int(rng.integers(0, hay_len - k + 1)) if starts is None else starts[i]
        rec.append((i, s, s + k))
    return rec


@pytest.mark.parametrize("n", [255, 256, 257, S - 1, S, S + 1])
def test_stage_record_counts_around_the_scans_levels(n):
    rng = np.random.default_rng(n)
    hay = text(3000, n)
    rec = segments(len(hay), rng.choice([0, 1, 2, 3, 4, 5, 9, 16, 17, 40], size=n).tolist(), rng)
    check_stage(rec, [n], hay, what=("one row", n))
    # ... and as a batch: rows with 0 .. 5 records, the context clipped by the rows
    cuts = np.unique(np.concatenate([[0, len(hay)], rng.integers(0, len(hay), size=n // 3)])).astype(np.int64)
    counts = rng.multinomial(n, np.ones(len(cuts) - 1) / (len(cuts) - 1))
    rec = [(i, int(rng.integers(0, 40)), int(rng.integers(0, 60))) for i in range(n)]  # (junk among them: e < s, beyond the row)
    check_stage(rec, counts, hay, ("offsets", cuts), context=int(rng.integers(0, 9)), what=("rows", n))


def test_stage_segment_lengths_around_the_chunk_and_the_tile():
    lengths = [0, 1, 3, 4, 5, 15, 16, 17, 31, 33, T - 1, T, T + 1, 3 * T + 5]  # (the last: a tile wholly inside one segment)
    hay = text(4 * T + 100, 1)
    rng = np.random.default_rng(1)
    for k, order in enumerate((lengths, lengths[::-1], list(rng.permutation(lengths)), list(rng.permutation(lengths)))):
        check_stage(segments(len(hay), order, rng), [len(order)], hay, shift=(5 * k) % 16, what=("lengths", k))
    for k in lengths:  # every length alone, and in front of and behind a short one
        check_stage(segments(len(hay), [k], rng), [1], hay, what=("alone", k))
        check_stage(segments(len(hay), [3, k, 2], rng), [3], hay, shift=9, what=("between", k))


@pytest.mark.parametrize("shift", [0, 5])
def test_stage_every_pair_of_source_and_output_alignment(shift):
    """a piece of 21 bytes (word loads, two chunks) and one of 2 (byte loads) at every (source address, output offset) mod 16"""
    hay = text(2000, 2)
    rec, out, seen = [], 0, set()
    for a in range(16):
        for b in range(16):
            fill = (b - out) % 16                     # a filler brings the output to b (empty when it is there already)
            rec.append((0, 700, 700 + fill))
            out += fill
            s = 16 * (a + 3 * b) + ((a - shift) % 16)  # hay byte s lies at device address = a (mod 16)
            assert (s + shift) % 16 == a and out % 16 == b
            seen.add(((s + shift) % 16, out % 16))
            rec.append((1, s, s + 21))
            out += 21
            fill = (b - out) % 16
            rec.append((0, 900, 900 + fill))
            out += fill
            rec.append((2, s + 1, s + 3))
            out += 2
    assert len(seen) == 256
    check_stage(rec, [len(rec)], hay, shift=shift, what="alignment pairs")


@pytest.mark.parametrize("shift", range(16))
def test_stage_the_haystack_at_every_address_modulo_16(shift):
    """segments that begin at haystack byte 0 and end at its last byte, len % 16 in {0, 1, 15}: the first and the last aligned
    word of the input straddle its ends"""
    rng = np.random.default_rng(shift)
    for hay_len in (160, 161, 175, 7, 3):
        hay = text(hay_len, 3 + hay_len)
        lens = [k for k in (1, 3, 4, 5, 16, 17, 33, hay_len) if k <= hay_len]
        rec = [(0, 0, k) for k in lens] + [(1, hay_len - k, hay_len) for k in lens] + segments(hay_len, [min(k, hay_len) for k in (2, 6, 20)], rng)
        check_stage(rec, [len(rec)], hay, shift=shift, what=("ends", hay_len))
        check_stage(rec, [len(rec)], hay, context=2, shift=shift, what=("ends, context", hay_len))


def test_stage_segments_and_tile_boundaries():
    hay = text(3 * T, 4)
    rng = np.random.default_rng(4)
    for delta in (-1, 0, 1):  # a segment ends one before, on and one behind the first and the second boundary
        first = T + delta
        rec = [(0, 10, 10 + first), (1, 5, 5 + T - delta - 20), (2, 100, 120), (3, 7, 7 + 33)]
        assert rec[0][2] - rec[0][1] == T + delta and sum(r[2] - r[1] for r in rec[:3]) == 2 * T
        check_stage(rec, [4], hay, shift=3, what=("ends beside a boundary", delta))
    # empty segments exactly on a tile boundary, in front of it and behind it; a run of them longer than a window
    for run in (1, 3, WIN - 1, WIN, WIN + 5, 2 * WIN + 1):
        rec = [(0, 0, T - 4), (1, 50, 54)] + [(9, 60, 60)] * run + [(2, 20, 29)] + [(9, 0, 0)] * run + [(3, 200, 200 + T - 9)] + [(9, 5, 5)] * run
        assert rec[0][2] + 4 == T
        check_stage(rec, [len(rec)], hay, what=("empty segments on a boundary", run))
        check_stage([(9, 3, 3)] * run + rec, [run + len(rec)], hay, shift=11, what=("empty segments first", run))
    check_stage([(9, 3, 3)] * (WIN + 2), [WIN + 2], hay, what="nothing but empty segments")
    # one tile that consists entirely of 1-byte segments, between longer ones; then two such tiles
    for ones in (T, 2 * T + 3):
        starts = rng.integers(0, len(hay) - 1, size=ones)
        rec = [(0, 40, 40 + T)] + [(1, int(s), int(s) + 1) for s in starts] + [(2, 9, 9 + 50)]
        check_stage(rec, [len(rec)], hay, shift=1, what=("a tile of 1-byte segments", ones))
    # ascending 1-byte segments with empty ones between them
    rec = []
    for i in range(T + 40):
        rec += [(1, i, i + 1)] + [(9, i, i)] * (i % 3)
    check_stage(rec, [len(rec)], hay, shift=7, what="1-byte segments and empties")


@pytest.mark.parametrize("cut", ["offsets", "uniform", "single"])
def test_stage_rows_cut_three_ways_and_records_that_cross_tiles_and_rows(cut):
    rng = np.random.default_rng(7)
    L, rows = 700, 40
    hay = text(L * rows, 5)
    if cut == "offsets":
        cuts = np.unique(np.concatenate([[0, len(hay)], rng.integers(0, len(hay), size=rows)])).astype(np.int64)
        cuts = np.sort(np.concatenate([cuts, cuts[3:9], cuts[-1:], cuts[:1]]))  # (empty rows, in front and at the end too)
        how = ("offsets", cuts)
        n_rows = len(cuts) - 1
    elif cut == "uniform":
        how, n_rows = ("uniform", L), rows
    else:
        how, n_rows = ("single",), 1
    lens = [len(r) for r in rows_of(hay, how)]
    counts = rng.choice([0, 0, 1, 3, 30], size=n_rows)
    rec = []
    for h, c in enumerate(counts):  # ends that do not decrease within a row, as a search reports them
        ends = np.sort(rng.integers(0, lens[h] + 5, size=int(c)))
        rec += [(int(rng.integers(0, 50)), max(0, int(e) - int(rng.integers(0, 12))), int(e)) for e in ends]
    for context in (0, 1, 30, 300, CONTEXT_MAX):  # (300: snippets of 600 bytes -- tiles, records and rows all cross)
        check_stage(rec, counts, hay, how, context=context, shift=13, what=(cut, context))
    check_stage([], np.zeros(n_rows, dtype=np.uint64), hay, how, context=3, what=(cut, "no record"))


def test_stage_the_utf8_trim_on_the_device():
    alphabet = ["a", "b", " ", "é", "€", "\U0001F600", "日"]
    rng = np.random.default_rng(9)
    rows = ["".join(rng.choice(alphabet, size=int(rng.integers(0, 90)))).encode() for _ in range(60)]
    rows += [b"\x80" * 9 + b"MM" + b"\xbf" * 9, b"\xbf", b""]  # (invalid: the trim stops after three steps)
    cuts = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    counts = rng.choice([0, 1, 2, 7], size=len(rows))
    rec = []
    for h, c in enumerate(counts):
        for _ in range(int(c)):
            s = int(rng.integers(0, len(rows[h]) + 2))
            rec.append((h, s, s + int(rng.integers(0, 7))))
    hay = b"".join(rows)
    for context in (0, 1, 2, 3, 4, 9, CONTEXT_MAX):
        check_stage(rec, counts, hay, ("offsets", cuts), context=context, flags=UTF8, shift=context % 16, what=("utf8", context))
        check_stage(rec, counts, hay, ("offsets", cuts), context=context, flags=0, what=("bytes", context))


def test_stage_too_big_nothing_to_cut_and_bad_arguments():
    hay = text(500, 6)
    rec = [(0, 10, 30), (1, 40, 45), (2, 100, 300)]
    want = definition(rec, [3], [hay], 2)[0]
    total = sum(len(w) for w in want)
    for cap in (total - 1, 16, 0):
        code, got_total, data, off, pat, lead, ro = run_stage(rec, [3], hay, ("single",), context=2, capacity=cap)
        assert code == capi.ETOOBIG and got_total == total and data == b""       # (run_stage saw the data unwritten)
        assert off.tolist() == [0, 24, 33, total] and pat.tolist() == [0, 1, 2] and lead.tolist() == [2, 2, 2] and ro.tolist() == [0, 3]
    code, got_total, data, *_ = run_stage(rec, [3], hay, ("single",), context=2, capacity=total + 40)  # more room than needed
    assert code == capi.OK and got_total == total and data == b"".join(want)
    # no record; no row; records without counts
    code, total0, data, off, pat, lead, ro = run_stage([], [0, 0], hay, ("uniform", 250), context=5)
    assert (code, total0, data, off.tolist(), ro.tolist()) == (capi.OK, 0, b"", [0], [0, 0, 0])
    code, total0, data, off, pat, lead, ro = run_stage([], [], b"", ("uniform", 8))
    assert (code, total0, off.tolist(), ro.tolist()) == (capi.OK, 0, [0], [0])
    for bad_counts in ([1, 1], [4, 0], [0, 0]):
        with pytest.raises(ValueError) as ei:
            run_stage(rec, bad_counts, hay, ("uniform", 250), capacity=64)
        assert ei.value.code == capi.EINVAL
    for kw in (dict(context=1 << 63), dict(flags=2)):
        with pytest.raises(ValueError) as ei:
            run_stage(rec, [3], hay, ("single",), capacity=64, **kw)
        assert ei.value.code == capi.EINVAL
    with pytest.raises(ValueError) as ei:  # rows of one length must fill the batch
        run_stage(rec, [3, 0], hay, ("uniform", 300), capacity=64)
    assert ei.value.code == capi.EINVAL
    with pytest.raises(ValueError) as ei:  # offsets that do not end at len
        run_stage(rec, [3, 0], hay, ("offsets", [0, 10, 499]), capacity=64)
    assert ei.value.code == capi.EINVAL


# ---------------------------------------------------------------------------
# end to end through the C ABI against the oracle
# ---------------------------------------------------------------------------
PATS = gen.gen_patterns(500, 3, 9, gen.AZ, 5) + [b"ab", b"abab", b"bab", b"ab", b"abcab", b"cabc"]  # (a copy; patterns that nest and chain)
KINDS = [(0, False), (0, True), (1, False), (2, False)]


def oracle_snippets(o, hays, ov, context, utf8=False, search=None):
    """the definition over the oracle's matches, row by row.  search: the bytes the oracle sees (a case-insensitive handle's
    folded rows) -- the snippets are cut of `hays`"""
    rec, counts = [], []
    for i, h in enumerate(hays):
        m = o.find_raw(h if search is None else search[i], overlapping=ov)
        rec += [tuple(int(x) for x in r) for r in m]
        counts.append(len(m))
    return definition(rec, counts, hays, context, utf8)


def check_snippets(r, want, on_device, batch=True, what=None):
    """a capi.DeviceSnippets against the definition, through the copies and through the raw addresses"""
    snippets, pattern, lead, ro = want
    n = len(snippets)
    assert r.on_device == on_device and r.count == n and r.rows == (len(ro) - 1 if batch else 0), (what, r.count, n, r.rows)
    blob = b"".join(snippets)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in snippets])]).astype(np.int64)
    assert r.nbytes == len(blob), (what, r.nbytes, len(blob))
    assert np.array_equal(r.offsets(), offs), what
    got = r.data().tobytes()
    if got != blob:
        bad = next(i for i in range(len(blob)) if got[i] != blob[i])
        raise AssertionError((what, "first wrong byte", bad, "in snippet", int(np.searchsorted(offs, bad, side="right")) - 1, got[max(bad - 4, 0):bad + 8],
                              blob[max(bad - 4, 0):bad + 8]))
    assert r.tolist() == snippets
    assert r.pattern().tolist() == pattern and r.lead().tolist() == lead, what
    if batch:
        assert r.row_offsets().tolist() == ro, what
    else:
        assert r.row_offsets() is None and r.data_ptr(capi.SNIP_ROW_OFFSETS) == 0, what
    for which in (capi.SNIP_DATA, capi.SNIP_OFFSETS, capi.SNIP_PATTERN, capi.SNIP_LEAD):
        p = r.data_ptr(which)
        assert p and p % 8 == 0, what  # (an empty part still has an address)
    if on_device and len(blob):
        raw = np.empty(len(blob), dtype=np.uint8)
        capi._check(capi.lib().acx_device_download(raw.ctypes.data, r.data_ptr(capi.SNIP_DATA), len(blob)))
        assert raw.tobytes() == blob, what
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
def test_snippets_parity_host_and_device_inputs(mk, ov):
    o = Oracle(PATS, mk, KIND_DFA)
    a = capi.Automaton(PATS, mk)
    for n_hay in (1, 65, 323):
        hays = batch_with_empties(PATS, n_hay, 100 + n_hay)
        for context in (0, 20):
            want = oracle_snippets(o, hays, ov, context)
            assert n_hay == 1 or len(want[0])
            check_snippets(a.snippets(hays, ov, context), want, False, what=(mk, ov, n_hay, context))
            for off in (0, 5):
                d = OnDevice(hays, off)
                check_snippets(a.snippets_device(*d.args, overlapping=ov, context=context, **d.kw), want, True, what=(mk, ov, n_hay, off, context))
                d.free()
    # a uniform batch on the device, and the same bytes as a host batch
    L, nh = 512, 130
    full = gen.gen_textlike(L * nh, 61, PATS).tobytes()
    hays = [full[i * L:(i + 1) * L] for i in range(nh)]
    dev = capi.DeviceBuffer(len(full)).upload(np.frombuffer(full, dtype=np.uint8))
    for context in (0, 3, CONTEXT_MAX):
        want = oracle_snippets(o, hays, ov, context)
        check_snippets(a.snippets_device(dev.ptr, len(full), n_hay=nh, uniform_len=L, overlapping=ov, context=context), want, True, what="uniform")
        check_snippets(a.snippets(hays, ov, context), want, False, what="uniform, host")
    assert dev.download().tobytes() == full
    dev.free()
    a.close()


def test_snippets_one_haystack_that_is_no_batch_empty_batches_and_errors():
    o, a = Oracle(PATS, 0, KIND_DFA), capi.Automaton(PATS, 0)
    for hay in (gen.gen_textlike(5000, 3, PATS).tobytes(), gen.gen_textlike(300_000, 4, PATS).tobytes(), b"0123" * 100, b""):
        for ov, context in ((False, 0), (True, 0), (False, 7)):
            want = oracle_snippets(o, [hay], ov, context)
            dev = capi.DeviceBuffer(len(hay) + 16).upload(np.frombuffer(hay + b"\0", dtype=np.uint8))
            check_snippets(a.snippets(None, ov, context, single=hay), want, False, batch=False, what=("single", len(hay), context))
            check_snippets(a.snippets_device(dev.ptr, len(hay), overlapping=ov, context=context), want, True, batch=False,
                           what=("single, device", len(hay), context))
            dev.free()
    none = ([], [], [], [0])
    check_snippets(a.snippets([], context=3), none, False, what="empty batch")
    check_snippets(a.snippets([b"", b""]), ([], [], [], [0, 0, 0]), False, what="empty rows only")
    dev = capi.DeviceBuffer(64)
    check_snippets(a.snippets_device(dev.ptr, 0, n_hay=0, uniform_len=8), none, True, what="empty batch, device")
    for call in (lambda: a.snippets([b"ab"], context=1 << 63), lambda: a.snippets_device(dev.ptr, 0, n_hay=0, uniform_len=8, context=1 << 63),
                 lambda: a.snippets([b"ab"], flags=2), lambda: a.snippets_device(dev.ptr, 10, n_hay=3, uniform_len=4)):
        with pytest.raises(ValueError) as ei:
            call()
        assert ei.value.code == capi.EINVAL
    for mk in (1, 2):
        b = capi.Automaton([b"ab", b"b"], mk)
        for call in (lambda: b.snippets([b"xxabxx"], overlapping=True), lambda: b.snippets(None, overlapping=True, single=b"ab"),
                     lambda: b.snippets_device(0, 0, n_hay=0, uniform_len=8, overlapping=True)):
            with pytest.raises(ValueError) as ei:
                call()
            assert ei.value.code == capi.EOVERLAP
        b.close()
    dev.free()
    a.close()


def test_snippets_case_insensitive_handle_returns_the_callers_bytes():
    pats = [b"Needle", b"hay", b"STACK"]
    o = Oracle([p.translate(FOLD) for p in pats], 1, KIND_DFA)
    hays = [b"a nEEdle in a HayStack; " * 3, b"Nothing Here", b"", b"NEEDLE", b"x" * 5000 + b"hAY", b"NO", b"needle HAY stack Xyz" * 900]
    folded = [h.translate(FOLD) for h in hays]
    a = capi.Automaton(pats, 1, ascii_case_insensitive=True)
    for context in (0, 4):
        want = oracle_snippets(o, hays, False, context, search=folded)
        assert want[0][:3] == ([b"nEEdle", b"Hay", b"Stack"] if context == 0 else [b"a nEEdle in ", b"n a HayStac", b" HayStack; a "])
        check_snippets(a.snippets(hays, context=context), want, False, what=context)
        d = OnDevice(hays, 5)
        check_snippets(a.snippets_device(*d.args, context=context, **d.kw), want, True, what=context)
        d.free()
    a.close()


def test_snippets_utf8_flag_through_the_c_abi():
    pats = ["é", "€uro", "\U0001F600", "ab", "naïve", "日本"]
    raw_pats = [p.encode() for p in pats]
    hays = ["café ab €uro \U0001F600!", "", "naïve 日本語 naive", "ascii ab only", "ééé\U0001F600\U0001F600€uro", "€ur", "é€\U0001F600" * 700 + "ab"]
    raw = [h.encode() for h in hays]
    for mk, ov in ((0, False), (0, True), (2, False)):
        o, a = Oracle(raw_pats, mk, KIND_DFA), capi.Automaton(raw_pats, mk)
        for context in (0, 1, 2, 3, 5):
            want = oracle_snippets(o, raw, ov, context, utf8=True)
            for s in want[0]:
                s.decode()  # (every snippet is whole characters)
            plain = oracle_snippets(o, raw, ov, context)
            assert context == 0 or want[0] != plain[0]
            check_snippets(a.snippets(raw, ov, context, UTF8), want, False, what=("utf8", mk, ov, context))
            d = OnDevice(raw, 3)
            check_snippets(a.snippets_device(*d.args, overlapping=ov, context=context, flags=UTF8, **d.kw), want, True, what=("utf8, device", mk, ov, context))
            check_snippets(a.snippets_device(*d.args, overlapping=ov, context=context, **d.kw), plain, True, what=("bytes, device", mk, ov, context))
            d.free()
        a.close()


def test_snippets_of_a_find_cut_into_byte_ranges(monkeypatch):
    o, a = Oracle(PATS, 0, KIND_DFA), capi.Automaton(PATS, 0)
    hay = gen.gen_textlike(3_000_000, 17, PATS).tobytes()
    dev = capi.DeviceBuffer(len(hay)).upload(np.frombuffer(hay, dtype=np.uint8))
    monkeypatch.setenv("ACX_CHUNK_BYTES", "700001")
    a.path_stats(reset=True)
    for ov in (False, True):
        check_snippets(a.snippets_device(dev.ptr, len(hay), overlapping=ov), oracle_snippets(o, [hay], ov, 0), True, batch=False, what=("cut", ov))
    check_snippets(a.snippets_device(dev.ptr, len(hay), context=16), oracle_snippets(o, [hay], False, 16), True, batch=False, what="cut, context")
    st = a.path_stats()
    monkeypatch.delenv("ACX_CHUNK_BYTES")
    assert st["byte_ranges"] >= 2, st
    dev.free()
    a.close()


def test_snippets_of_a_find_on_the_dense_path():
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
    want = oracle_snippets(o, [every], False, 0)
    for _ in range(2):  # (one haystack that is no batch: the call tests/test_gpu_columns.py sees take that path)
        check_snippets(a.snippets_device(dev.ptr, len(every)), want, True, batch=False, what="dense, one row")
    st = a.path_stats()
    assert st["hot_calls"] + st["dense_tiles"] + st["dense_radix"] >= 2, st
    check_snippets(a.snippets_device(dev.ptr, len(every), n_hay=len(hays), uniform_len=L, context=24), oracle_snippets(o, hays, False, 24), True,
                   what="dense, context 24")
    dev.free()
    a.close()


def test_eight_threads_on_one_handle():
    a, o = capi.Automaton(PATS, 0), Oracle(PATS, 0, KIND_DFA)
    work = []
    for t in range(8):
        hays = batch_with_empties(PATS, 40 + 9 * t, 300 + t) + [gen.gen_textlike(150_000, t, PATS).tobytes()]
        work.append((hays, oracle_snippets(o, hays, False, 0), oracle_snippets(o, hays, True, 5)))
    errors = []

    def run(t):
        try:
            hays, want, want5 = work[t]
            for i in range(3):
                check_snippets(a.snippets(hays), want, False, what=t)
                d = OnDevice(hays, t)
                check_snippets(a.snippets_device(*d.args, **d.kw), want, True, what=t)
                check_snippets(a.snippets_device(*d.args, overlapping=True, context=5, **d.kw), want5, True, what=t)
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
    for case in range(150):
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
        small = sum(len(h) for h in hays) <= 4000  # (with the largest budget every snippet is its whole row)
        context = rng.choice([0, 0, 1, 2, 5, 64, CONTEXT_MAX] if small else [0, 0, 1, 2, 5, 64])
        want = oracle_snippets(o, hays, ov, context)
        route = rng.choice(["host", "device", "device"])
        what = (case, mk, ov, n_hay, route, context)
        try:
            if route == "device":
                d = OnDevice(hays, rng.randrange(16))
                check_snippets(a.snippets_device(*d.args, overlapping=ov, context=context, **d.kw), want, True, what=what)
                d.free()
            else:
                check_snippets(a.snippets(hays, ov, context), want, False, what=what)
        except AssertionError as e:
            raise AssertionError(f"case {what}: {e}") from e
    for a, _ in made.values():
        a.close()


# ---------------------------------------------------------------------------
# the Python methods: sequences of host objects (tensors in HBM and torch as the consumer: the script below)
# ---------------------------------------------------------------------------
def matchkind(ar, mk):
    return (ar.MatchKind.Standard, ar.MatchKind.LeftmostFirst, ar.MatchKind.LeftmostLongest)[mk]


def per_row(want):
    snippets, _, _, ro = want
    return [snippets[ro[h]:ro[h + 1]] for h in range(len(ro) - 1)]


def check_match_snippets(ms, want, batch=True, decode=False):
    """a MatchSnippets in host memory against the definition"""
    snippets, pattern, lead, ro = want
    assert len(ms) == len(snippets) and ms.device is None and ms.nbytes == sum(len(s) for s in snippets)
    rows = per_row(want) if batch else snippets
    if decode:
        rows = [[s.decode() for s in r] for r in rows] if batch else [s.decode() for s in rows]
    assert ms.tolist() == rows
    data = np.from_dlpack(ms.data)
    assert data.dtype == np.uint8 and data.tobytes() == b"".join(snippets) and len(ms.data) == ms.nbytes
    mv = memoryview(ms.data)
    assert mv.format == "B" and mv.readonly
    offs = np.from_dlpack(ms.offsets)
    assert offs.dtype == np.int64 and offs.tolist() == np.concatenate([[0], np.cumsum([len(s) for s in snippets])]).astype(np.int64).tolist()
    assert np.from_dlpack(ms.pattern).tolist() == pattern and np.from_dlpack(ms.lead).tolist() == lead
    assert len(ms.offsets) == len(snippets) + 1 and len(ms.pattern) == len(ms.lead) == len(snippets)
    if batch:
        assert len(ms.row_offsets) == len(ro) and np.from_dlpack(ms.row_offsets).tolist() == ro
    else:
        assert ms.row_offsets is None


@pytest.mark.parametrize("mk,ov", KINDS)
def test_python_sequences_both_classes_and_the_identities(mk, ov):
    import ahocorasick_rs as ar
    o = Oracle(PATS, mk, KIND_DFA)
    b = ar.BytesAhoCorasick(PATS, matchkind=matchkind(ar, mk))
    s = ar.AhoCorasick([p.decode() for p in PATS], matchkind=matchkind(ar, mk))
    for n_hay in (0, 1, 64, 130):
        hays = batch_with_empties(PATS, n_hay, 500 + n_hay)
        strs = [h.decode() for h in hays]
        for context in (0, 12):
            want = oracle_snippets(o, hays, ov, context)
            check_match_snippets(b.find_matches_as_snippets_batch(hays, overlapping=ov, context=context), want)
            check_match_snippets(b.find_matches_as_snippets_batch(tuple(bytearray(h) for h in hays), ov, context=context), want)
            check_match_snippets(s.find_matches_as_snippets_batch(strs, ov, context=context), want, decode=True)
            for h, row in list(zip(hays, per_row(want)))[:40]:  # the single forms agree with tolist()
                assert b.find_matches_as_snippets(h, overlapping=ov, context=context).tolist() == row
                assert s.find_matches_as_snippets(h.decode(), ov, context=context).tolist() == [x.decode() for x in row]
        # the identities: context = 0 is hay[s:e] and find_matches_as_strings; .pattern and .row_offsets are the columns'
        ms, mc = b.find_matches_as_snippets_batch(hays, ov), b.find_matches_as_columns_batch(hays, overlapping=ov)
        assert np.array_equal(np.from_dlpack(ms.pattern), np.from_dlpack(mc.pattern))
        assert np.array_equal(np.from_dlpack(ms.row_offsets), np.from_dlpack(mc.row_offsets))
        st, en, ro = (np.from_dlpack(c) for c in (mc.start, mc.end, mc.row_offsets))
        flat = [x for r in ms.tolist() for x in r]
        row = np.repeat(np.arange(n_hay), np.diff(ro)) if n_hay else np.zeros(0, dtype=np.int64)
        assert flat == [hays[h][a:e] for h, a, e in zip(row.tolist(), st.tolist(), en.tolist())]
        wide = b.find_matches_as_snippets_batch(hays, ov, context=9)
        lead, offs = np.from_dlpack(wide.lead), np.from_dlpack(wide.offsets)
        assert ((lead >= 0) & (lead <= 9) & (lead + (en - st) <= np.diff(offs))).all()  # lead plus the match fits inside the snippet
        blob = np.from_dlpack(wide.data).tobytes()
        assert [blob[offs[i] + lead[i]:offs[i] + lead[i] + en[i] - st[i]] for i in range(len(flat))] == flat
        for h in strs[:40]:
            assert s.find_matches_as_snippets(h, ov).tolist() == s.find_matches_as_strings(h, overlapping=ov)
    one = gen.gen_textlike(20_000, 9, PATS).tobytes()
    check_match_snippets(b.find_matches_as_snippets(one, ov), oracle_snippets(o, [one], ov, 0), batch=False)
    check_match_snippets(b.find_matches_as_snippets(np.frombuffer(one, dtype=np.uint8), ov, context=3), oracle_snippets(o, [one], ov, 3), batch=False)
    check_match_snippets(s.find_matches_as_snippets(one.decode(), ov, context=3), oracle_snippets(o, [one], ov, 3), batch=False, decode=True)


def test_python_str_never_splits_a_character():
    import ahocorasick_rs as ar
    pats = ["é", "€uro", "\U0001F600", "ab", "naïve", "日本"]
    s = ar.AhoCorasick(pats, matchkind=ar.MatchKind.LeftmostLongest)
    o = Oracle([p.encode() for p in pats], 2, KIND_DFA)
    hays = ["café ab €uro \U0001F600!", "", "naïve 日本語 naive", "ascii ab only", "ééé\U0001F600\U0001F600€uro", "€ur"]
    raw = [h.encode() for h in hays]
    for context in (0, 1, 2, 3, 4, 7):
        want = oracle_snippets(o, raw, False, context, utf8=True)
        check_match_snippets(s.find_matches_as_snippets_batch(hays, context=context), want, decode=True)
        for h, row in zip(hays, per_row(want)):
            got = s.find_matches_as_snippets(h, context=context).tolist()
            assert got == [x.decode() for x in row] and all(g in h for g in got), h
    for h in hays:
        assert s.find_matches_as_snippets(h).tolist() == s.find_matches_as_strings(h)
    assert s.find_matches_as_snippets("café ab €uro \U0001F600!").tolist() == ["é", "ab", "€uro", "\U0001F600"]
    # a budget in BYTES: 1 byte of "é" is no character, 2 are
    assert s.find_matches_as_snippets("éabé", context=1).tolist() == ["éa", "ab", "bé"]
    assert s.find_matches_as_snippets("éabé", context=2).tolist() == ["éab", "éabé", "abé"]
    # a host tensor of the same UTF-8 bytes
    flat = np.frombuffer(b"".join(raw), dtype=np.uint8).copy()
    cuts = np.concatenate([[0], np.cumsum([len(r) for r in raw])]).astype(np.int64)
    want = oracle_snippets(o, raw, False, 3, utf8=True)
    assert s.find_matches_as_snippets_batch(flat, context=3, offsets=cuts).tolist() == [[x.decode() for x in r] for r in per_row(want)]


def test_python_errors_and_host_tensors():
    import ahocorasick_rs as ar
    b, s = ar.BytesAhoCorasick([b"ab", b"c"]), ar.AhoCorasick(["ab", "c"])
    for call in (lambda: b.find_matches_as_snippets(b"ab", context=-1), lambda: s.find_matches_as_snippets("ab", context=1 << 63),
                 lambda: b.find_matches_as_snippets_batch([b"ab"], context=-5), lambda: s.find_matches_as_snippets_batch(["ab"], context=1 << 64)):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: b.find_matches_as_snippets(b"ab", context=True), lambda: s.find_matches_as_snippets("ab", context=1.5),
                 lambda: b.find_matches_as_snippets(b"ab", False, 3), lambda: b.find_matches_as_snippets_batch([b"ab"], False, 3),
                 lambda: b.find_matches_as_snippets(b"ab", overlapping=1), lambda: b.find_matches_as_snippets("ab"),
                 lambda: s.find_matches_as_snippets(b"ab"), lambda: b.find_matches_as_snippets_batch([b"ab"], row_length=2),
                 lambda: b.find_matches_as_snippets(b"ab", row_length=2), lambda: b.find_matches_as_snippets_batch([b"ab"], context=None),
                 lambda: b.find_matches_as_snippets_batch([b"ab"], offsets=np.array([0, 2], dtype=np.int64))):
        with pytest.raises(TypeError):
            call()
    assert b.find_matches_as_snippets(b"xxabxcx").tolist() == [b"ab", b"c"]
    assert s.find_matches_as_snippets("xxabxcx", context=1).tolist() == ["xabx", "xcx"]
    got = b.find_matches_as_snippets_batch([b"abab", b"", b"xcxxc"], context=1)
    assert got.tolist() == [[b"aba", b"bab"], [], [b"xcx", b"xc"]] and got.device is None and len(got) == 4 and got.nbytes == 11
    assert np.from_dlpack(got.lead).tolist() == [0, 1, 1, 1] and np.from_dlpack(got.pattern).tolist() == [0, 0, 1, 1]
    assert b.find_matches_as_snippets_batch([b"abab", b"", b"xcxxc"], context=CONTEXT_MAX).tolist() == [[b"abab"] * 2, [], [b"xcxxc"] * 2]
    t = np.frombuffer(b"abxcYxabab", dtype=np.uint8).copy()
    ms = b.find_matches_as_snippets_batch(t, row_length=5, context=1)
    assert ms.tolist() == [[b"abx", b"xcY"], [b"xaba", b"bab"]] and np.from_dlpack(ms.row_offsets).tolist() == [0, 2, 4]
    ms = b.find_matches_as_snippets_batch(t, context=9, offsets=np.array([0, 1, 1, 6, 10], dtype=np.int64))
    assert ms.tolist() == [[], [], [b"bxcYx"], [b"abab", b"abab"]]
    assert s.find_matches_as_snippets_batch(t, row_length=2).tolist() == [["ab"], ["c"], [], ["ab"], ["ab"]]
    assert t.tobytes() == b"abxcYxabab"
    empty = b.find_matches_as_snippets(b"")
    assert len(empty) == 0 and empty.tolist() == [] and empty.row_offsets is None and empty.nbytes == 0
    assert len(np.from_dlpack(empty.data)) == 0 and np.from_dlpack(empty.offsets).tolist() == [0]
    for mk in (ar.MatchKind.LeftmostFirst, ar.MatchKind.LeftmostLongest):
        for call in (lambda x: x.find_matches_as_snippets(b"ab", overlapping=True), lambda x: x.find_matches_as_snippets_batch([b"ab"], overlapping=True)):
            with pytest.raises(ValueError):
                call(ar.BytesAhoCorasick([b"ab"], matchkind=mk))
    assert ar.BytesAhoCorasick([b"abc", b"bcd"]).find_matches_as_snippets(b"abcd", overlapping=True).tolist() == [b"abc", b"bcd"]
    ci = ar.BytesAhoCorasick([b"NeEdLe"], ascii_case_insensitive=True)
    assert ci.find_matches_as_snippets(b"A nEEdle, a Needle", context=2).tolist() == [b"A nEEdle, ", b"a Needle"]
    assert ar.AhoCorasick(["needle"], ascii_case_insensitive=True).find_matches_as_snippets("A nEEdle").tolist() == ["nEEdle"]
    with pytest.raises(TypeError):
        ar.MatchSnippets()


def test_host_parts_outlive_the_match_snippets():
    import ahocorasick_rs as ar
    o, b = Oracle(PATS, 0, KIND_DFA), ar.BytesAhoCorasick(PATS)
    hays = batch_with_empties(PATS, 300, 3)
    want = oracle_snippets(o, hays, False, 6)
    ms = b.find_matches_as_snippets_batch(hays, context=6)
    data, mv, ro, unused = np.from_dlpack(ms.data), memoryview(ms.offsets), np.from_dlpack(ms.row_offsets), ms.lead.__dlpack__()
    del ms, unused, hays
    gc.collect()
    for k in range(20):  # (other results come and go where the bytes would be if they had been freed)
        b.find_matches_as_snippets_batch(batch_with_empties(PATS, 300, 50 + k), context=k)
    assert data.tobytes() == b"".join(want[0]) and ro.tolist() == want[3]
    assert np.asarray(mv).tolist() == np.concatenate([[0], np.cumsum([len(s) for s in want[0]])]).tolist()


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

def snippets(o, rows, ov, context):
    # the definition over every row's matches (bytes: no trim)
    out, pattern, lead, ro = [], [], [], [0]
    for B in rows:
        n = len(B)
        for p, s, e in o.find_raw(B, overlapping=ov):
            s1 = min(int(s), n); e1 = min(max(int(e), s1), n)
            lo = s1 - min(s1, context); hi = e1 + min(context, n - e1)
            out.append(B[lo:hi]); pattern.append(int(p)); lead.append(s1 - lo)
        ro.append(len(out))
    return out, pattern, lead, ro

def check(ms, want, where, batch=True):
    out, pattern, lead, ro = want
    assert ms.device == (0 if where == "device" else None), (where, ms.device)
    assert len(ms) == len(out) and ms.nbytes == sum(len(x) for x in out)
    data, offs, pat, ld = (torch.from_dlpack(c) for c in (ms.data, ms.offsets, ms.pattern, ms.lead))
    assert data.dtype == torch.uint8 and tuple(data.shape) == (ms.nbytes,) and data.is_contiguous()
    for x, n in ((offs, len(out) + 1), (pat, len(out)), (ld, len(out))):
        assert x.dtype == torch.int64 and tuple(x.shape) == (n,) and x.is_contiguous()
        assert x.device.type == ("cuda" if where == "device" else "cpu")
    assert data.cpu().numpy().tobytes() == b"".join(out), where
    assert offs.tolist() == np.concatenate([[0], np.cumsum([len(x) for x in out])]).astype(np.int64).tolist()
    assert pat.tolist() == pattern and ld.tolist() == lead, where
    if batch:
        r = torch.from_dlpack(ms.row_offsets)
        assert r.dtype == torch.int64 and r.tolist() == ro and r.device.type == data.device.type
        assert ms.tolist() == [out[ro[h]:ro[h + 1]] for h in range(len(ro) - 1)]
    else:
        assert ms.row_offsets is None and ms.tolist() == out
    if where == "device":
        # no copy: the tensor IS the part (the same address on every export)
        assert data.device.index == 0 and ms.data.__dlpack_device__() == (10, 0)
        assert torch.from_dlpack(ms.data).data_ptr() == data.data_ptr() and torch.from_dlpack(ms.offsets).data_ptr() == offs.data_ptr()
        assert torch.from_dlpack(ms.lead).data_ptr() == ld.data_ptr() and data.data_ptr() % 16 == 0
        try:
            memoryview(ms.data)
            raise SystemExit("a device part exported a host buffer")
        except BufferError:
            pass
    return data, offs

for mk, ov in ((0, False), (0, True), (1, False), (2, False)):
    o = Oracle(pats, mk, KIND_DFA)
    b = ar.BytesAhoCorasick(pats, matchkind=kinds[mk])
    s = ar.AhoCorasick([p.decode() for p in pats], matchkind=kinds[mk])
    uniform = [hay[i * L:(i + 1) * L].tobytes() for i in range(nh)]
    ragged = [hay[cuts[i]:cuts[i + 1]].tobytes() for i in range(len(lens))]
    d_cuts = torch.from_numpy(cuts).to("cuda:0")
    for context in ((0, 40) if mk == 0 else (3,)):
        wu, wr = snippets(o, uniform, ov, context), snippets(o, ragged, ov, context)
        check(b.find_matches_as_snippets_batch(t, overlapping=ov, context=context, row_length=L), wu, "device")   # a tensor in HBM: the result stays there
        check(b.find_matches_as_snippets_batch(t, ov, context=context, offsets=d_cuts), wr, "device")
        sm = s.find_matches_as_snippets_batch(t, ov, context=context, row_length=L)                               # (ASCII: nothing to trim)
        assert sm.device == 0 and torch.from_dlpack(sm.data).cpu().numpy().tobytes() == b"".join(wu[0])
        assert sm.tolist() == [[x.decode() for x in wu[0][wu[3][h]:wu[3][h + 1]]] for h in range(nh)]
        check(b.find_matches_as_snippets_batch(torch.from_numpy(hay), ov, context=context, row_length=L), wu, "host")
        check(b.find_matches_as_snippets_batch(torch.from_numpy(hay), ov, context=context, offsets=torch.from_numpy(cuts)), wr, "host")
        check(b.find_matches_as_snippets_batch(uniform, ov, context=context), wu, "host")
        check(b.find_matches_as_snippets(t, ov, context=context), snippets(o, [hay.tobytes()], ov, context), "device", batch=False)   # one tensor that is no batch
        check(b.find_matches_as_snippets(t[5:5 + 3 * L + 1], ov, context=context), snippets(o, [hay[5:5 + 3 * L + 1].tobytes()], ov, context), "device", batch=False)
    # the identities on the device: .pattern and .row_offsets are the columns'; context = 0 is hay[s:e], cut in torch
    ms, mc = b.find_matches_as_snippets_batch(t, ov, row_length=L), b.find_matches_as_columns_batch(uniform, overlapping=ov)
    assert torch.equal(torch.from_dlpack(ms.pattern).cpu(), torch.from_dlpack(mc.pattern))
    assert torch.equal(torch.from_dlpack(ms.row_offsets).cpu(), torch.from_dlpack(mc.row_offsets))
    cs, ce, cro = (torch.from_dlpack(c).to("cuda:0") for c in (mc.start, mc.end, mc.row_offsets))
    row = torch.repeat_interleave(torch.arange(nh, device="cuda:0"), cro[1:] - cro[:-1])
    seg = ce - cs
    offs = torch.from_dlpack(ms.offsets)
    assert torch.equal(offs[1:] - offs[:-1], seg)
    idx = torch.repeat_interleave(row * L + cs - offs[:-1], seg) + torch.arange(int(seg.sum()), device="cuda:0")   # the only way before
    assert torch.equal(torch.from_dlpack(ms.data), t[idx])
    wide = b.find_matches_as_snippets_batch(t, ov, context=9, row_length=L)
    wl, wo = torch.from_dlpack(wide.lead), torch.from_dlpack(wide.offsets)
    assert bool(((wl >= 0) & (wl <= 9) & (wl + seg <= wo[1:] - wo[:-1])).all())
    idx = torch.repeat_interleave(wo[:-1] + wl - offs[:-1], seg) + torch.arange(int(seg.sum()), device="cuda:0")
    assert torch.equal(torch.from_dlpack(wide.data)[idx], torch.from_dlpack(ms.data))   # the match stands lead bytes into its snippet

o, b = Oracle(pats, 0, KIND_DFA), ar.BytesAhoCorasick(pats)
uniform = [hay[i * L:(i + 1) * L].tobytes() for i in range(nh)]
want = snippets(o, uniform, False, 8)

# split_rows(t).offsets as offsets=: the rows of a delimited buffer, cut where they lie
lines = hay.copy()
lines[np.random.default_rng(1).integers(0, len(lines), size=3000)] = 10
lt = torch.from_numpy(lines).to("cuda:0")
ro = ar.split_rows(lt)
offs = torch.from_dlpack(ro.offsets).cpu().numpy()
rows = [lines[offs[i]:offs[i + 1]].tobytes() for i in range(len(offs) - 1)]
check(b.find_matches_as_snippets_batch(lt, context=30, offsets=ro.offsets), snippets(o, rows, False, 30), "device")

# an odd device address; the consumer on a stream of its own
side = torch.cuda.Stream()
odd = [hay[5 + i * L:5 + (i + 1) * L].tobytes() for i in range(100)]
with torch.cuda.stream(side):
    data, offs_ = check(b.find_matches_as_snippets_batch(t[5:5 + 100 * L], context=2, row_length=L), snippets(o, odd, False, 2), "device")
    total = data.to(torch.int64).sum()
assert int(total) == sum(sum(x) for x in snippets(o, odd, False, 2)[0])

# a case-insensitive handle: the caller's own bytes
ci = ar.BytesAhoCorasick([b"NeEdLe"], ascii_case_insensitive=True)
ct = torch.from_numpy(np.frombuffer(b"A nEEdle, a Needle. " * 50, dtype=np.uint8).copy()).to("cuda:0")
assert ci.find_matches_as_snippets_batch(ct, row_length=20).tolist() == [[b"nEEdle", b"Needle"]] * 50
assert ci.find_matches_as_snippets_batch(ct, context=2, row_length=20).tolist() == [[b"A nEEdle, ", b"a Needle. "]] * 50
assert ci.find_matches_as_snippets(ct[:20], context=1).tolist() == [b" nEEdle,", b" Needle."]

# str with multi-byte characters in HBM: whole characters
sm = ar.AhoCorasick(["é", "€uro", "ab"])
u = "café ab €uro".encode()
ut = torch.from_numpy(np.frombuffer(u * 3, dtype=np.uint8).copy()).to("cuda:0")
r = sm.find_matches_as_snippets_batch(ut, row_length=len(u))
assert r.tolist() == [["é", "ab", "€uro"]] * 3 and r.device == 0
r = sm.find_matches_as_snippets_batch(ut, context=2, row_length=len(u))
assert r.tolist() == [["afé a", " ab ", "b €uro"]] * 3, r.tolist()   # (2 bytes of context; half a character is none)
assert torch.from_dlpack(r.lead).tolist() == [2, 1, 2] * 3

def raises(exc, call):
    try:
        call()
    except exc:
        return
    raise SystemExit("no %s" % exc.__name__)
raises(TypeError, lambda: b.find_matches_as_snippets_batch(t))                                   # neither offsets nor row_length
raises(TypeError, lambda: b.find_matches_as_snippets_batch(t, row_length=L, offsets=torch.from_numpy(cuts).to("cuda:0")))
raises(ValueError, lambda: b.find_matches_as_snippets_batch(t, offsets=torch.from_numpy(cuts)))  # offsets on another device
raises(ValueError, lambda: b.find_matches_as_snippets_batch(t, context=-1, row_length=L))
raises(ValueError, lambda: b.find_matches_as_snippets_batch(t, offsets=torch.from_numpy(cuts[:-2].copy()).to("cuda:0")))  # they do not span the tensor
raises(ValueError, lambda: ar.BytesAhoCorasick(pats, matchkind=kinds[1]).find_matches_as_snippets_batch(t, overlapping=True, row_length=L))
raises(ValueError, lambda: ar.BytesAhoCorasick(pats, matchkind=kinds[1]).find_matches_as_snippets(t, overlapping=True))

# no rows, and rows without a match: the parts still become tensors
ms = b.find_matches_as_snippets_batch(torch.zeros(0, dtype=torch.uint8, device="cuda:0"), row_length=7)
assert len(ms) == 0 and ms.tolist() == [] and tuple(torch.from_dlpack(ms.data).shape) == (0,) and torch.from_dlpack(ms.row_offsets).tolist() == [0]
assert torch.from_dlpack(ms.offsets).tolist() == [0]
z = torch.full((1 << 20,), 48, dtype=torch.uint8, device="cuda:0")
ms = b.find_matches_as_snippets_batch(z, context=5, row_length=1 << 10)
assert len(ms) == 0 and not torch.from_dlpack(ms.row_offsets).any() and len(ms.row_offsets) == 1025 and tuple(torch.from_dlpack(ms.lead).shape) == (0,)
assert len(b.find_matches_as_snippets(z)) == 0 and b.find_matches_as_snippets(z).device == 0

# lifetime: the tensors keep the result alive after the MatchSnippets object, its handle and its input are gone
b2 = ar.BytesAhoCorasick(pats)
t2 = t.clone()
ms = b2.find_matches_as_snippets_batch(t2, context=8, row_length=L)
data, ld, r = torch.from_dlpack(ms.data), torch.from_dlpack(ms.lead), torch.from_dlpack(ms.row_offsets)
unused = ms.offsets.__dlpack__()
del ms, unused, b2, t2
gc.collect()
for k in range(6):  # (other results come and go where the bytes would be if they had been given back)
    other = torch.from_numpy(gen.gen_textlike(L * nh, 40 + k, pats).copy()).to("cuda:0")
    keep = b.find_matches_as_snippets_batch(other, context=k, row_length=L)
    del keep
gc.collect()
torch.cuda.synchronize()
assert data.cpu().numpy().tobytes() == b"".join(want[0]) and ld.tolist() == want[2] and r.tolist() == want[3]
del data, ld, r
gc.collect()

# eight threads on one handle, tensors in HBM
errors = []
def run(i):
    try:
        for k in range(3):
            lo = i * 20 + k
            ms = b.find_matches_as_snippets_batch(t[lo * L:(lo + 20) * L], context=8, row_length=L)
            a, z_ = want[3][lo], want[3][lo + 20]
            assert torch.from_dlpack(ms.data).cpu().numpy().tobytes() == b"".join(want[0][a:z_]), (i, k)
            assert torch.from_dlpack(ms.lead).tolist() == want[2][a:z_], (i, k)
            assert torch.from_dlpack(ms.row_offsets).tolist() == [x - a for x in want[3][lo:lo + 21]], (i, k)
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
    """find_matches_as_snippets_batch on tensors in HBM with offsets and with row_length, both classes, and
    find_matches_as_snippets on one tensor; torch.from_dlpack of the five parts on the automaton's device without a copy; the
    identities with the columns and the torch index form; split_rows' offsets as offsets=; the case-insensitive form; whole
    characters; errors; empty results; lifetime; threads.  In a process of its own: torch has to be the first to load the HIP
    runtime."""
    pytest.importorskip("torch")
    p = subprocess.run([sys.executable, "-c", _TENSOR_SCRIPT, ROOT, os.path.join(ROOT, "tests")], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
