"""Row scores from per-pattern weights, on the device (acx_score / acx_score_device / acx_score_rows_device,
acx_filter_scored / acx_filter_scored_device; score_batch / filter_by_score_batch): the device stage alone at the seams of
its tile kernel -- record counts around the tile, rows that cross tiles, row boundaries around a tile's and a wave's end,
runs of empty rows, row counts around the scan's levels, the 64-bit carry -- with guards around the scores and the inputs
verified unwritten; parity with the definition through the C ABI for every match kind, on host and device inputs, both
routes, for finds that were cut or took the dense path; the filter by score against the definition and against the filter by
count; the Python methods with sequences and with tensors in HBM, torch as the consumer, lifetime, threads and a seeded
random loop.  Expected values come from numpy over synthetic records or from the oracle's matches (tests/oracle_lib.py) and
the definition restated below, never from the library; the kernel's seams are read from its header."""
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
MATCHED = 1  # ACX_FILTER_KEEP_MATCHED
W_MAX = (1 << 31) - 1


def hip_constants(path, names):
    src = open(os.path.join(CSRC, path)).read()
    out = {}
    for n in names:
        m = re.search(r"\b%s\s*=\s*(\d+)\s*[,;]" % n, src)
        assert m, f"{n} is no longer a plain constant of {path}"
        out[n] = int(m.group(1))
    return out


_C = hip_constants("score.hpp", ("SCORE_THREADS", "SCORE_TILE"))
THREADS, T = _C["SCORE_THREADS"], _C["SCORE_TILE"]
S = 2048  # replace_scan's items per workgroup (replace.hip RS_THREADS * RS_PER): beyond it the scan has two levels, beyond S * S three
GUARD = 0xC3


def test_constants_are_what_the_sizes_below_assume():
    assert T % THREADS == 0 and THREADS % 64 == 0 and T >= 256
    src = open(os.path.join(CSRC, "replace.hip")).read()
    assert re.search(r"RS_THREADS = 256, RS_PER = 8\b", src), "the scan's level size is no longer 2048"
    assert capi.FILTER_KEEP_MATCHED == MATCHED


# ---------------------------------------------------------------------------
# the stage alone
# ---------------------------------------------------------------------------
def definition_rows(pattern, counts, weights):
    """score[h] = sum of weights[pattern] over row h's records (pattern >= len(weights): nothing), modulo 2^64"""
    pattern = np.asarray(pattern, dtype=np.uint64)
    w = np.asarray(weights, dtype=np.int64)
    row = np.repeat(np.arange(len(counts)), np.asarray(counts, dtype=np.int64))
    ok = pattern < len(w)
    score = np.zeros(len(counts), dtype=np.int64)
    with np.errstate(over="ignore"):
        np.add.at(score, row[ok], w[pattern[ok].astype(np.int64)])
    return score


def run_stage(pattern, counts, weights, residue8=False, prefill=GUARD):
    """score_rows_device on synthetic records (their start and end fields are noise), counts and weights, with guard words
    before and behind the scores -> the scores; guards and inputs checked"""
    pattern = np.asarray(pattern, dtype=np.uint64)
    counts = np.asarray(counts, dtype=np.uint64)
    w = np.asarray(weights, dtype=np.int32)
    n, rows = len(pattern), len(counts)
    m = (np.arange(3 * n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)).reshape(n, 3)
    m[:, 0] = pattern
    shift = 8 if residue8 else 0
    d_m = capi.DeviceBuffer(24 * n + 32)
    d_m.upload(np.concatenate([np.full(shift, 0xEE, np.uint8), m.reshape(-1).view(np.uint8), np.full(16, 0xEE, np.uint8)]))
    assert d_m.ptr % 16 == 0
    d_c = capi.DeviceBuffer(max(8 * rows, 8))
    d_w = capi.DeviceBuffer(max(4 * len(w), 8))
    if rows:
        d_c.upload(counts)
    if len(w):
        d_w.upload(w)
    image = np.full(16 + 8 * rows + 16, prefill, dtype=np.uint8)
    image[:16] = image[16 + 8 * rows:] = GUARD
    out = capi.DeviceBuffer(len(image)).upload(image)
    capi.score_rows_device(d_m.ptr + shift if n else 0, n, d_c.ptr if rows else 0, rows, d_w.ptr if len(w) else 0, len(w), out.ptr + 16)
    got = out.download(len(image))
    m_after, c_after, w_after = d_m.download(shift + 24 * n), d_c.download(8 * rows), d_w.download(4 * len(w))
    for b in (d_m, d_c, d_w, out):
        b.free()
    assert np.array_equal(m_after[shift:], m.reshape(-1).view(np.uint8)), "the records were written"
    assert np.array_equal(c_after.view(np.uint64), counts) and np.array_equal(w_after.view(np.int32), w), "an input was written"
    assert (got[:16] == GUARD).all() and (got[16 + 8 * rows:] == GUARD).all(), "a word outside the scores was written"
    return got[16:16 + 8 * rows].view(np.int64)


def check_stage(pattern, counts, weights, what=None, **kw):
    got = run_stage(pattern, counts, weights, **kw)
    want = definition_rows(pattern, counts, weights)
    if not np.array_equal(got, want):
        bad = int(np.flatnonzero(got != want)[0])
        raise AssertionError((what, "rows", len(want), "first difference at row", bad, got[bad:bad + 4], want[bad:bad + 4],
                              "records before it", int(np.asarray(counts[:bad], dtype=np.int64).sum()), "its count", int(counts[bad])))
    return want


WEIGHTS = np.asarray([3, -7, 0, 1000003, -1, 2, -W_MAX, W_MAX, 11, -13], dtype=np.int64)


def patterns_for(n, seed=1):
    return np.random.default_rng(seed).integers(0, len(WEIGHTS), size=n)


def ragged_counts(n, seed, choices=(0, 0, 1, 2, 3, 7, 40)):
    """row lengths from `choices` that sum to exactly n"""
    rng = np.random.default_rng(seed)
    out, left = [], n
    while left:
        c = min(int(rng.choice(choices)), left)
        out.append(c)
        left -= c
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5])
def test_stage_record_counts_around_the_tile(n):
    check_stage(patterns_for(n), ragged_counts(n, n), WEIGHTS, ("ragged", n))
    check_stage(patterns_for(n, 2), ragged_counts(n, n + 1, (0, 1, 300, 700)), WEIGHTS, ("long rows", n))
    check_stage(patterns_for(n, 3), [n], WEIGHTS, ("one row holds everything: every tile adds to it", n))
    check_stage(patterns_for(n, 4), [0, 0, n, 0], WEIGHTS, ("one row between empty ones", n))
    check_stage(patterns_for(n, 5), [1] * n, WEIGHTS, ("every row of one record", n))
    check_stage(patterns_for(n, 6), ragged_counts(n, n + 2), WEIGHTS, ("records at 8 modulo 16", n), residue8=True)


def test_stage_rows_of_exactly_a_tile_and_boundaries_around_a_tiles_end():
    check_stage(patterns_for(5 * T), [T] * 5, WEIGHTS, "rows of exactly T")
    check_stage(patterns_for(5 * T + 3), [T, 0, T, T, 3, T, 0, T], WEIGHTS, "rows of exactly T, shifted behind the third")
    for first in (T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1):
        for second in (1, 2, T - 1, T, T + 1):
            n = first + second + 5
            check_stage(patterns_for(n, first), [first, second, 5], WEIGHTS, ("a boundary at", first, "then", second))
            check_stage(patterns_for(n, first), [first, 0, 0, second, 0, 5], WEIGHTS, ("with empty rows at it", first, second))


def test_stage_boundaries_around_a_waves_end_and_a_threads():
    per = T // THREADS
    for at in (63, 64, 65, per - 1, per, per + 1, 64 * per - 1, 64 * per, 64 * per + 1, 128 * per, T - 64 * per + 1):
        for tile in (0, 1):
            first = tile * T + at
            n = first + 100 + T
            check_stage(patterns_for(n, at), [first, 1, 1, 98, T], WEIGHTS, ("a boundary at", at, "of tile", tile))
    # every boundary position of one tile, in one batch: rows of 1 .. 9 records walk over every residue
    counts = [1 + (i * 5) % 9 for i in range(3000)]
    assert sum(counts) > 4 * T
    check_stage(patterns_for(sum(counts), 9), counts, WEIGHTS, "rows of 1 .. 9 records")


def test_stage_runs_of_empty_rows():
    """at the start, at the end, exactly on a tile boundary, and more of them between two records than a tile has slots or
    a workgroup threads"""
    long_run = 3 * T + 2 * THREADS + 7
    p = patterns_for(4 * T, 7)
    check_stage(p[:10], [0] * long_run + [4, 6], WEIGHTS, "at the start")
    check_stage(p[:10], [4, 6] + [0] * long_run, WEIGHTS, "at the end")
    check_stage(p[:10], [4] + [0] * long_run + [6], WEIGHTS, "between two records")
    check_stage(p[:2 * T], [T] + [0] * long_run + [T], WEIGHTS, "exactly on a tile boundary")
    check_stage(p[:2 * T], [T - 1, 1] + [0] * 5 + [T - 1] + [0] * 3 + [1], WEIGHTS, "on a boundary behind a row of one record")
    check_stage(p[:2 * T + 9], [T + 3] + [0] * long_run + [T - 3] + [0] * long_run + [9] + [0] * THREADS, WEIGHTS, "inside tiles")
    check_stage(p[:3 * T], [0] * THREADS + [3 * T] + [0] * THREADS, WEIGHTS, "around one row of three tiles")


def test_stage_no_records_and_no_rows():
    got = run_stage([], [0] * 1000, WEIGHTS, prefill=0x77)  # n = 0: the scores are cleared
    assert len(got) == 1000 and not got.any()
    got = run_stage([], [0], WEIGHTS, prefill=0x77)
    assert list(got) == [0]
    # n_hay = 0 launches nothing: no word is written (run_stage checks the guards), null pointers are taken
    assert len(run_stage([], [], WEIGHTS)) == 0
    capi.score_rows_device(0, 0, 0, 0, 0, 0, 0)


@pytest.mark.parametrize("rows", [S - 1, S, S + 1, S * S + 1])
def test_stage_row_counts_around_the_scans_levels(rows):
    rng = np.random.default_rng(rows)
    counts = np.zeros(rows, dtype=np.int64)
    some = rng.choice(rows, size=min(rows, 3000), replace=False)
    counts[some] = rng.choice([1, 1, 2, 5, 700], size=len(some))
    counts[[0, rows - 1]] = 3  # (the first and the last row)
    n = int(counts.sum())
    check_stage(patterns_for(n, rows), counts, WEIGHTS, ("rows", rows))


def test_stage_extreme_weights_carry_into_the_high_word():
    n = 3 * T + 5
    assert n * W_MAX > 1 << 40
    for w in (W_MAX, -W_MAX):
        want = check_stage(np.zeros(n, np.uint64), [n], [w], ("one row", w))
        assert int(want[0]) == n * w
        want = check_stage(np.zeros(n + 10, np.uint64), [4, n, 6], [w], ("between two rows", w))
        assert list(want) == [4 * w, n * w, 6 * w]
    want = check_stage(np.tile([0, 1], n), [2 * n], [W_MAX, -W_MAX], "the two cancel")
    assert list(want) == [0]
    check_stage(np.arange(4 * T) % 2, [T + 1, 2 * T - 2, T + 1], [W_MAX, -5], "mixed")


def test_stage_ignores_patterns_beyond_the_weights():
    n = 2 * T + 9
    p = patterns_for(n, 11).astype(np.uint64)
    p[::3] = len(WEIGHTS)              # the first id out of range
    p[1::7] = (1 << 64) - 1
    p[2::11] = 1 << 32                 # (its low word alone would be in range)
    p[5::13] = (1 << 63) + 1
    counts = ragged_counts(n, 12)
    want = check_stage(p, counts, WEIGHTS, "out of range")
    assert want.any()
    got = run_stage(p, counts, [])     # no weights at all: nothing is indexed, every score 0
    assert len(got) == len(counts) and not got.any()


def test_stage_refuses_bad_arguments():
    d = capi.DeviceBuffer(4096)
    d.upload(np.zeros(512, dtype=np.uint64))
    d.upload(np.asarray([2, 1], dtype=np.uint64))  # (the counts of two rows: 3 records)
    args = dict(d_records=d.ptr + 1024, n=3, d_counts=d.ptr, n_hay=2, d_weights=d.ptr + 512, n_weights=4, d_scores=d.ptr + 2048)
    capi.score_rows_device(**args)
    for change in (dict(n=4), dict(n=2), dict(d_records=d.ptr + 1028), dict(d_scores=d.ptr + 2052), dict(d_counts=d.ptr + 4),
                   dict(d_weights=d.ptr + 514), dict(d_scores=0), dict(d_counts=0), dict(d_records=0), dict(d_weights=0),
                   dict(n_hay=0)):
        with pytest.raises(ValueError) as ei:
            capi.score_rows_device(**{**args, **change})
        assert ei.value.code == capi.EINVAL, change
    d.free()


# ---------------------------------------------------------------------------
# end to end through the C ABI against the oracle
# ---------------------------------------------------------------------------
PATS = gen.gen_patterns(500, 3, 9, gen.AZ, 5) + [b"ab", b"abab", b"bab", b"ab"]  # (a copy: overlapping reports it)
PAT_W = [int(x) for x in np.random.default_rng(5).integers(-9, 10, size=len(PATS))]
PAT_W[-4:] = [5, -3, 2, 100]  # (the copy of "ab" carries a weight of its own)
KINDS = [(0, False), (0, True), (1, False), (2, False)]


def oracle_scores(o, hays, ov, weights):
    """the issue's definition from the oracle's matches"""
    w = np.asarray(weights, dtype=np.int64)
    return np.asarray([int(w[o.find_raw(h, overlapping=ov)[:, 0].astype(np.int64)].sum()) for h in hays], dtype=np.int64)


def filtered_definition(hays, scores, min_score, keep_matched):
    rows, offsets, data = [], [0], []
    for h, (hay, s) in enumerate(zip(hays, scores)):
        if (s >= min_score) == keep_matched:
            rows.append(h)
            data.append(hay)
            offsets.append(offsets[-1] + len(hay))
    return np.asarray(rows, np.int64), np.asarray(offsets, np.int64), np.frombuffer(b"".join(data), np.uint8)


def download_bytes(ptr, n):
    out = np.empty(n, dtype=np.uint8)
    if n:
        capi._check(capi.lib().acx_device_download(out.ctypes.data, ptr, n))
    return out


def check_scores(s, want, on_device, what=None):
    """a capi.DeviceScores against the definition, through the copy and through the raw address"""
    assert s.on_device == on_device and s.rows == len(want), (what, s.rows, len(want))
    got = s.scores()
    assert got.dtype == np.int64 and np.array_equal(got, want), (what, got[:8], want[:8])
    p = s.data_ptr()
    assert p and p % 8 == 0, what  # (an empty result still has an address)
    if on_device:
        assert p % 256 == 0 and np.array_equal(download_bytes(p, want.nbytes), want.view(np.uint8)), what
    else:
        assert np.array_equal(np.ctypeslib.as_array((capi.ctypes.c_uint8 * max(want.nbytes, 1)).from_address(p))[:want.nbytes], want.view(np.uint8))
    s.free()


def check_filtered(f, want, on_device, what=None):
    rows, offsets, data = want
    assert f.on_device == on_device and f.n_rows == len(rows) and f.nbytes == len(data), (what, f.n_rows, f.nbytes, len(rows), len(data))
    for k, w in ((capi.FILT_ROWS, rows), (capi.FILT_OFFSETS, offsets), (capi.FILT_DATA, data)):
        assert np.array_equal(f.part(k), w), (what, k)
        p = f.data_ptr(k)
        assert p and p % 8 == 0, (what, k)
        if on_device:
            assert p % 256 == 0 and np.array_equal(download_bytes(p, w.nbytes), w.view(np.uint8)), (what, k)
    f.free()


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
        self.hay = capi.DeviceBuffer(len(blob) + 32).upload(np.frombuffer(b"\xa5" * off + blob, dtype=np.uint8))
        self.off = capi.DeviceBuffer(8 * len(offs)).upload(offs)
        self.args = (self.hay.ptr + off, len(blob))
        self.kw = dict(d_offsets=self.off.ptr, n_hay=len(hays))

    def free(self):
        self.hay.free()
        self.off.free()


@pytest.mark.parametrize("mk,ov", KINDS)
def test_score_parity_host_and_device_inputs(monkeypatch, mk, ov):
    o = Oracle(PATS, mk, KIND_DFA)
    a = capi.Automaton(PATS, mk)
    for n_hay in (1, 65, 323):
        hays = batch_with_empties(PATS, n_hay, 100 + n_hay)
        want = oracle_scores(o, hays, ov, PAT_W)
        assert n_hay == 1 or (want != 0).any()
        for host_max in ("0", str(1 << 40)):  # staged and scored in HBM / scored on the host: a host result either way
            monkeypatch.setenv("ACX_SCORE_HOST_MAX", host_max)
            check_scores(a.score(hays, PAT_W, ov), want, False, (mk, ov, n_hay, host_max))
        monkeypatch.delenv("ACX_SCORE_HOST_MAX")
        for off in (0, 5):
            d = OnDevice(hays, off)
            check_scores(a.score_device(*d.args, PAT_W, overlapping=ov, **d.kw), want, True, (mk, ov, n_hay, off))
            d.free()
    # a uniform batch on the device, and the same bytes as a host batch
    L, nh = 512, 130
    full = gen.gen_textlike(L * nh, 61, PATS).tobytes()
    hays = [full[i * L:(i + 1) * L] for i in range(nh)]
    want = oracle_scores(o, hays, ov, PAT_W)
    dev = capi.DeviceBuffer(len(full)).upload(np.frombuffer(full, dtype=np.uint8))
    check_scores(a.score_device(dev.ptr, len(full), PAT_W, n_hay=nh, uniform_len=L, overlapping=ov), want, True, "uniform")
    check_scores(a.score(hays, PAT_W, ov), want, False, "uniform, host")
    dev.free()
    a.close()


def test_score_one_haystack_that_is_no_batch_empty_batches_and_errors(monkeypatch):
    o, a = Oracle(PATS, 0, KIND_DFA), capi.Automaton(PATS, 0)
    for hay in (gen.gen_textlike(5000, 3, PATS).tobytes(), b"0123" * 100, b""):
        want = oracle_scores(o, [hay], False, PAT_W)
        dev = capi.DeviceBuffer(len(hay) + 16).upload(np.frombuffer(hay + b"\0", dtype=np.uint8))
        for host_max in ("0", str(1 << 40)):
            monkeypatch.setenv("ACX_SCORE_HOST_MAX", host_max)
            check_scores(a.score(None, PAT_W, single=hay), want, False, ("single", len(hay), host_max))
        monkeypatch.delenv("ACX_SCORE_HOST_MAX")
        check_scores(a.score_device(dev.ptr, len(hay), PAT_W), want, True, ("single, device", len(hay)))
        for flags in (0, MATCHED):
            wf = filtered_definition([hay], want, 1, bool(flags))
            check_filtered(a.filter_scored(None, PAT_W, False, 1, flags, single=hay), wf, False, ("single", flags))
            check_filtered(a.filter_scored_device(dev.ptr, len(hay), PAT_W, flags=flags), wf, True, ("single, device", flags))
        dev.free()
    none = np.zeros(0, dtype=np.int64)
    check_scores(a.score([], PAT_W), none, False, "empty batch")
    dev = capi.DeviceBuffer(64)
    check_scores(a.score_device(dev.ptr, 0, PAT_W, n_hay=0, uniform_len=8), none, True, "empty batch, device")
    check_filtered(a.filter_scored([], PAT_W), filtered_definition([], [], 1, False), False, "empty batch")
    check_filtered(a.filter_scored_device(dev.ptr, 0, PAT_W, n_hay=0, uniform_len=8), filtered_definition([], [], 1, False), True, "empty, device")
    for bad in (PAT_W[:-1], PAT_W + [1], []):  # one weight per pattern
        for call in (lambda: a.score([b"ab"], bad), lambda: a.score_device(dev.ptr, 0, bad, n_hay=0, uniform_len=8),
                     lambda: a.filter_scored([b"ab"], bad), lambda: a.filter_scored_device(dev.ptr, 0, bad, n_hay=0, uniform_len=8)):
            with pytest.raises(ValueError) as ei:
                call()
            assert ei.value.code == capi.EINVAL
    for call in (lambda: a.filter_scored([b"ab"], PAT_W, flags=2), lambda: a.filter_scored_device(dev.ptr, 0, PAT_W, n_hay=0, uniform_len=8, flags=2)):
        with pytest.raises(ValueError) as ei:
            call()
        assert ei.value.code == capi.EINVAL
    b = capi.Automaton([b"ab", b"b"], 1)
    for call in (lambda: b.score([b"xxabxx"], [1, 1], overlapping=True),
                 lambda: b.score_device(0, 0, [1, 1], n_hay=0, uniform_len=8, overlapping=True),
                 lambda: b.filter_scored([b"xxabxx"], [1, 1], overlapping=True),
                 lambda: b.filter_scored_device(0, 0, [1, 1], n_hay=0, uniform_len=8, overlapping=True)):
        with pytest.raises(ValueError) as ei:
            call()
        assert ei.value.code == capi.EOVERLAP
    dev.free()
    b.close()
    a.close()


def test_score_copies_carry_their_own_weights_under_overlapping():
    pats, w = [b"ab", b"ab", b"ab", b"b"], [1, 10, 100, -1000]
    o, a = Oracle(pats, 0, KIND_DFA), capi.Automaton(pats, 0)
    hays = [b"ab", b"xx", b"abab", b"b", b"", b"xab"]
    for ov in (False, True):
        want = oracle_scores(o, hays, ov, w)
        assert int(want[0]) == (111 - 1000 if ov else 1)
        check_scores(a.score(hays, w, ov), want, False, ov)
        d = OnDevice(hays, 1)
        check_scores(a.score_device(*d.args, w, overlapping=ov, **d.kw), want, True, ov)
        for ms in (-889, 1, 2):
            for flags in (0, MATCHED):
                check_filtered(a.filter_scored_device(*d.args, w, overlapping=ov, min_score=ms, flags=flags, **d.kw),
                               filtered_definition(hays, want, ms, bool(flags)), True, (ov, ms, flags))
        d.free()
    a.close()


def test_score_case_insensitive_handle():
    pats, w = [b"Needle", b"hay", b"STACK"], [7, -2, 3]
    o = Oracle([p.translate(FOLD) for p in pats], 1, KIND_DFA)
    hays = [b"a nEEdle in a HayStack; " * 3, b"Nothing Here", b"", b"NEEDLE", b"x" * 5000 + b"hAY", b"NO", b"needle HAY stack" * 900]
    want = oracle_scores(o, [h.translate(FOLD) for h in hays], False, w)
    assert list(want[:5]) == [24, 0, 0, 7, -2]
    a = capi.Automaton(pats, 1, ascii_case_insensitive=True)
    check_scores(a.score(hays, w), want, False)
    d = OnDevice(hays, 5)
    check_scores(a.score_device(*d.args, w, **d.kw), want, True)
    for flags in (0, MATCHED):
        wf = filtered_definition(hays, want, 1, bool(flags))  # (the caller's unfolded bytes)
        check_filtered(a.filter_scored(hays, w, False, 1, flags), wf, False, flags)
        check_filtered(a.filter_scored_device(*d.args, w, flags=flags, **d.kw), wf, True, flags)
    assert np.array_equal(d.hay.download(5 + sum(map(len, hays)))[5:], np.frombuffer(b"".join(hays), dtype=np.uint8))
    d.free()
    a.close()


def test_score_of_a_find_cut_into_byte_ranges(monkeypatch):
    o, a = Oracle(PATS, 0, KIND_DFA), capi.Automaton(PATS, 0)
    hay = gen.gen_textlike(3_000_000, 17, PATS).tobytes()
    want = oracle_scores(o, [hay], False, PAT_W)
    dev = capi.DeviceBuffer(len(hay)).upload(np.frombuffer(hay, dtype=np.uint8))
    monkeypatch.setenv("ACX_CHUNK_BYTES", "700001")
    a.path_stats(reset=True)
    check_scores(a.score_device(dev.ptr, len(hay), PAT_W), want, True, "cut")
    for ms, flags in ((int(want[0]), MATCHED), (int(want[0]) + 1, MATCHED), (int(want[0]) + 1, 0)):
        check_filtered(a.filter_scored_device(dev.ptr, len(hay), PAT_W, min_score=ms, flags=flags),
                       filtered_definition([hay], want, ms, bool(flags)), True, (ms, flags))
    st = a.path_stats()
    monkeypatch.delenv("ACX_CHUNK_BYTES")
    assert st["byte_ranges"] >= 2, st
    dev.free()
    a.close()


def test_score_of_a_find_on_the_dense_path():
    pats = gen.gen_patterns(2000, 5, 12, gen.AZ, 1)
    w = [int(x) for x in np.random.default_rng(8).integers(-5, 6, size=len(pats))]
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
    want = oracle_scores(o, hays, False, w)
    dev = capi.DeviceBuffer(len(every)).upload(np.frombuffer(every, dtype=np.uint8))
    a.path_stats(reset=True)
    for _ in range(2):  # (one haystack that is no batch: the call tests/test_gpu_columns.py sees take that path)
        check_scores(a.score_device(dev.ptr, len(every), w), np.asarray([want.sum()], dtype=np.int64), True, "dense, one row")
    st = a.path_stats()
    assert st["hot_calls"] + st["dense_tiles"] + st["dense_radix"] >= 2, st
    check_scores(a.score_device(dev.ptr, len(every), w, n_hay=len(hays), uniform_len=L), want, True, "dense")
    ms = int(np.median(want))
    for flags in (0, MATCHED):
        check_filtered(a.filter_scored_device(dev.ptr, len(every), w, n_hay=len(hays), uniform_len=L, min_score=ms, flags=flags),
                       filtered_definition(hays, want, ms, bool(flags)), True, ("dense", flags))
    dev.free()
    a.close()


@pytest.mark.parametrize("mk,ov", KINDS)
def test_filter_scored_against_the_definition(monkeypatch, mk, ov):
    o = Oracle(PATS, mk, KIND_DFA)
    a = capi.Automaton(PATS, mk)
    hays = batch_with_empties(PATS, 131, 700 + mk)
    scores = oracle_scores(o, hays, ov, PAT_W)
    lo, hi = int(scores.min()), int(scores.max())
    assert lo < -3 and hi > 7
    d = OnDevice(hays, 3)
    for ms in (-3, 0, 1, 7, lo, hi + 1, -(1 << 63), (1 << 63) - 1):  # (lo: every row matched; hi + 1: none)
        for flags in (0, MATCHED):
            want = filtered_definition(hays, scores, ms, bool(flags))
            if ms in (lo, hi + 1):
                assert len(want[0]) == (len(hays) if (ms == lo) == bool(flags) else 0)  # k = n and k = 0
            for host_max in ("0", str(1 << 40)):
                monkeypatch.setenv("ACX_SCORE_HOST_MAX", host_max)
                check_filtered(a.filter_scored(hays, PAT_W, ov, ms, flags), want, False, (mk, ov, ms, flags, host_max))
            monkeypatch.delenv("ACX_SCORE_HOST_MAX")
            check_filtered(a.filter_scored_device(*d.args, PAT_W, overlapping=ov, min_score=ms, flags=flags, **d.kw), want, True,
                           (mk, ov, ms, flags))
    d.free()
    a.close()


@pytest.mark.parametrize("mk,ov", KINDS)
def test_filter_scored_with_weights_of_one_is_the_filter_by_count(mk, ov):
    a = capi.Automaton(PATS, mk)
    ones = [1] * len(PATS)
    hays = batch_with_empties(PATS, 200, 900 + mk)
    d = OnDevice(hays, 7)
    for m in (1, 2, 3, 10):
        for flags in (0, MATCHED):
            for scored, plain in ((a.filter_scored(hays, ones, ov, m, flags), a.filter(hays, ov, m, flags)),
                                  (a.filter_scored_device(*d.args, ones, overlapping=ov, min_score=m, flags=flags, **d.kw),
                                   a.filter_device(*d.args, overlapping=ov, min_matches=m, flags=flags, **d.kw))):
                assert scored.on_device == plain.on_device and (scored.n_rows, scored.nbytes) == (plain.n_rows, plain.nbytes)
                for k in (capi.FILT_ROWS, capi.FILT_OFFSETS, capi.FILT_DATA):
                    assert np.array_equal(scored.part(k), plain.part(k)), (mk, ov, m, flags, k)
                scored.free()
                plain.free()
    d.free()
    a.close()


def test_eight_threads_on_one_handle():
    a, o = capi.Automaton(PATS, 0), Oracle(PATS, 0, KIND_DFA)
    work = []
    for t in range(8):
        hays = batch_with_empties(PATS, 40 + 9 * t, 300 + t) + [gen.gen_textlike(150_000, t, PATS).tobytes()]
        work.append((hays, oracle_scores(o, hays, False, PAT_W)))
    errors = []

    def run(t):
        try:
            hays, want = work[t]
            for i in range(3):
                check_scores(a.score(hays, PAT_W), want, False, t)
                d = OnDevice(hays, t)
                check_scores(a.score_device(*d.args, PAT_W, **d.kw), want, True, t)
                check_filtered(a.filter_scored_device(*d.args, PAT_W, min_score=i, flags=(t + i) & 1, **d.kw),
                               filtered_definition(hays, want, i, bool((t + i) & 1)), True, t)
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


def test_seeded_random_batches(monkeypatch):
    rng = random.Random(20261018)
    for case in range(36):
        mk = rng.choice([0, 0, 1, 2])
        ov = mk == 0 and rng.random() < 0.4
        alpha = rng.choice([b"ab", b"abcd", gen.AZ])
        pats = gen.gen_patterns(rng.choice([1, 3, 40, 600]), 1, rng.choice([2, 6, 12]), alpha, 1000 + case)
        w = [rng.choice([0, 1, -1, 5, -7, W_MAX, -W_MAX, rng.randrange(-1000, 1000)]) for _ in pats]
        text = rng.choice([alpha, alpha + b"xyz", b"0123"])
        o = Oracle(pats, mk, KIND_DFA)
        n_hay = rng.choice([1, 2, 7, 64, 65, 130, 700])
        hays = [bytes(rng.choices(text, k=rng.choice([0, 0, 1, 9, 200, 5000, 20000]))) for _ in range(n_hay)]
        while sum(len(o.find_raw(h, overlapping=ov)) for h in hays) > 100_000:  # (cut down, never skipped)
            hays = [h[:len(h) // 2] for h in hays]
        want = oracle_scores(o, hays, ov, w)
        ms = rng.choice([-3, 0, 1, 7, int(np.median(want))])
        flags = rng.choice([0, MATCHED])
        route = rng.choice(["host", "staged", "device", "device"])
        monkeypatch.setenv("ACX_SCORE_HOST_MAX", "0" if route == "staged" else str(1 << 40))
        a = capi.Automaton(pats, mk)
        what = (case, mk, ov, n_hay, route, ms, flags)
        wf = filtered_definition(hays, want, ms, bool(flags))
        try:
            if route == "device":
                d = OnDevice(hays, rng.randrange(16))
                check_scores(a.score_device(*d.args, w, overlapping=ov, **d.kw), want, True, what)
                check_filtered(a.filter_scored_device(*d.args, w, overlapping=ov, min_score=ms, flags=flags, **d.kw), wf, True, what)
                d.free()
            else:
                check_scores(a.score(hays, w, ov), want, False, what)
                check_filtered(a.filter_scored(hays, w, ov, ms, flags), wf, False, what)
        except AssertionError as e:
            raise AssertionError(f"case {what}: {e}") from e
        a.close()


# ---------------------------------------------------------------------------
# the Python methods: sequences of host objects (tensors in HBM and torch as the consumer: the script below)
# ---------------------------------------------------------------------------
def matchkind(ar, mk):
    return (ar.MatchKind.Standard, ar.MatchKind.LeftmostFirst, ar.MatchKind.LeftmostLongest)[mk]


def check_row_scores(rs, want):
    """a RowScores in host memory against the definition"""
    assert len(rs) == len(want) and rs.device is None and rs.tolist() == [int(x) for x in want]
    col = rs.score
    assert len(col) == len(want) and col.__dlpack_device__() == (1, 0)
    got = np.from_dlpack(col)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    mv = memoryview(col)
    assert mv.format == "q" and mv.readonly and np.array_equal(np.asarray(mv), want)


@pytest.mark.parametrize("mk,ov", KINDS)
def test_python_sequences_both_classes(mk, ov):
    import ahocorasick_rs as ar
    o = Oracle(PATS, mk, KIND_DFA)
    b = ar.BytesAhoCorasick(PATS, matchkind=matchkind(ar, mk))
    s = ar.AhoCorasick([p.decode() for p in PATS], matchkind=matchkind(ar, mk))
    for n_hay in (0, 1, 64, 130):
        hays = batch_with_empties(PATS, n_hay, 500 + n_hay)
        want = oracle_scores(o, hays, ov, PAT_W)
        # the definition, from the library's own matches too: the same matches, the same `overlapping`
        assert [sum(PAT_W[p] for p, _, _ in m) for m in b.find_matches_as_indexes_batch(hays, overlapping=ov)] == list(want)
        for weights in (PAT_W, tuple(PAT_W), np.asarray(PAT_W, dtype=np.int64), np.asarray(PAT_W, dtype=np.int32)):
            check_row_scores(b.score_batch(hays, weights, overlapping=ov), want)
        check_row_scores(b.score_batch(tuple(bytearray(h) for h in hays), PAT_W, ov), want)
        check_row_scores(s.score_batch([h.decode() for h in hays], PAT_W, overlapping=ov), want)
        for keep in ("unmatched", "matched"):
            for ms in (-3, 0, 1, 7):
                rows, offsets, data = filtered_definition(hays, want, ms, keep == "matched")
                for fr, text in ((b.filter_by_score_batch(hays, PAT_W, overlapping=ov, keep=keep, min_score=ms), False),
                                 (s.filter_by_score_batch([h.decode() for h in hays], PAT_W, ov, keep=keep, min_score=ms), True)):
                    kept = [hays[h] for h in rows]
                    assert fr.tolist() == ([k.decode() for k in kept] if text else kept) and fr.source_rows == len(hays)
                    assert np.array_equal(np.from_dlpack(fr.rows), rows) and np.array_equal(np.from_dlpack(fr.offsets), offsets)
                    assert np.array_equal(np.from_dlpack(fr.data), data) and fr.device is None
    # the defaults: keep="unmatched", min_score=1
    three = [b"xx", b"ab", b"bab"]
    assert b.filter_by_score_batch(three, PAT_W).tolist() == [h for h, x in zip(three, oracle_scores(o, three, False, PAT_W)) if x < 1]


def test_python_errors_and_host_tensors():
    import ahocorasick_rs as ar
    b, s = ar.BytesAhoCorasick([b"ab", b"X"]), ar.AhoCorasick(["ab", "X"])
    for m in (b.score_batch, b.filter_by_score_batch, s.score_batch):
        hays = [b"ab"] if m.__self__ is b else ["ab"]
        for bad in ([1], [1, 2, 3], [], np.asarray([1], dtype=np.int64), [1 << 31, 0], [0, -(1 << 31)], [1 << 70, 0],
                    np.asarray([0, 1 << 31], dtype=np.int64)):  # a wrong length, a weight outside int32
            with pytest.raises(ValueError):
                m(hays, bad)
        for bad in ([1.0, 2], [1, "2"], [None, 1], [True, 1], 5, "12", b"12", np.asarray([1.0, 2.0]), np.asarray([1, 2], dtype=np.uint8),
                    np.asarray([[1, 2]], dtype=np.int64)):  # a weight that is no integer, weights that are no sequence of them
            with pytest.raises(TypeError):
                m(hays, bad)
        with pytest.raises(TypeError):
            m(hays)                                   # weights are required
        with pytest.raises(TypeError):
            m(hays, [1, 2], overlapping=1)
        with pytest.raises(TypeError):
            m(hays, [1, 2], offsets=np.array([0, 2], dtype=np.int64))  # a keyword of the tensor form with a sequence
    assert b.score_batch([b"abX"], [W_MAX, -W_MAX]).tolist() == [0] and b.score_batch([b"ab"], [-W_MAX, 0]).tolist() == [-W_MAX]
    for call in (lambda: b.filter_by_score_batch([b"ab"], [1, 2], False, "matched"),   # keyword-only
                 lambda: b.filter_by_score_batch([b"ab"], [1, 2], min_score=True),
                 lambda: b.filter_by_score_batch([b"ab"], [1, 2], min_score=2.0),
                 lambda: b.filter_by_score_batch([b"ab"], [1, 2], keep=1),
                 lambda: b.filter_by_score_batch([b"ab"], [1, 2], min_matches=1),        # (filter_batch's keyword)
                 lambda: b.score_batch([b"ab"], [1, 2], keep="matched")):
        with pytest.raises(TypeError):
            call()
    for call in (lambda: b.filter_by_score_batch([b"ab"], [1, 2], keep="both"), lambda: b.filter_by_score_batch([b"ab"], [1, 2], min_score=1 << 63),
                 lambda: b.filter_by_score_batch([b"ab"], [1, 2], min_score=-(1 << 63) - 1)):
        with pytest.raises(ValueError):
            call()
    assert b.filter_by_score_batch([b"ab", b"x"], [1, 2], min_score=-(1 << 63)).tolist() == []  # any int64: every row matched
    assert b.filter_by_score_batch([b"ab", b"x"], [1, 2], min_score=(1 << 63) - 1).tolist() == [b"ab", b"x"]
    assert b.filter_by_score_batch([b"abX", b"x", b"XX"], [1, -2], min_score=0, keep="matched").tolist() == [b"x"]  # abX: 1 - 2 < 0
    t = np.frombuffer(b"abxXYxabab", dtype=np.uint8).copy()
    rs = b.score_batch(t, [5, -1], row_length=5)
    assert rs.tolist() == [4, 10] and rs.device is None and len(rs) == 2
    assert b.score_batch(t, [5, -1], offsets=np.array([0, 1, 1, 6, 10], dtype=np.int64)).tolist() == [0, 0, -1, 10]
    assert s.score_batch(t, [5, -1], row_length=2).tolist() == [5, -1, 0, 5, 5]
    assert b.filter_by_score_batch(t, [5, -1], row_length=5, min_score=5, keep="matched").tolist() == [b"xabab"]
    for mk in (ar.MatchKind.LeftmostFirst, ar.MatchKind.LeftmostLongest):
        with pytest.raises(ValueError):
            ar.BytesAhoCorasick([b"ab"], matchkind=mk).score_batch([b"ab"], [1], overlapping=True)
        with pytest.raises(ValueError):
            ar.BytesAhoCorasick([b"ab"], matchkind=mk).filter_by_score_batch([b"ab"], [1], overlapping=True)
    with pytest.raises(TypeError):
        ar.RowScores()


def test_host_column_outlives_the_row_scores():
    import ahocorasick_rs as ar
    o, b = Oracle(PATS, 0, KIND_DFA), ar.BytesAhoCorasick(PATS)
    hays = batch_with_empties(PATS, 300, 3)
    want = oracle_scores(o, hays, False, PAT_W)
    rs = b.score_batch(hays, PAT_W)
    arr, mv, unused = np.from_dlpack(rs.score), memoryview(rs.score), rs.score.__dlpack__()
    del rs, unused
    gc.collect()
    for k in range(20):  # (other results come and go where the scores would be if they had been freed)
        b.score_batch(batch_with_empties(PATS, 300, 50 + k), PAT_W)
    assert np.array_equal(arr, want) and np.array_equal(np.asarray(mv), want)


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
w = [int(x) for x in np.random.default_rng(3).integers(-9, 10, size=len(pats))]
w[-4:] = [5, -3, 2, 100]
L, nh = 4096, 200
hay = gen.gen_textlike(L * nh, 13, pats).copy()
hay[3 * L:9 * L] = 48   # (rows without a match)
hay[50 * L:51 * L] = 48
t = torch.from_numpy(hay.copy()).to("cuda:0")
kinds = (ar.MatchKind.Standard, ar.MatchKind.LeftmostFirst, ar.MatchKind.LeftmostLongest)
lens = [0, 0, 17, L, 3 * L, 5, 0, 2 * L + 1, 4 * L, 7, 0]
lens += [L * nh - sum(lens), 0]
cuts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)

def scores_of(o, hays, ov):
    ww = np.asarray(w, dtype=np.int64)
    return [int(ww[o.find_raw(h, overlapping=ov)[:, 0].astype(np.int64)].sum()) for h in hays]

def check(rs, want, where):
    assert rs.device == (0 if where == "device" else None), (where, rs.device)
    assert len(rs) == len(want) and rs.tolist() == want, (where, rs.tolist()[:8], want[:8])
    x = torch.from_dlpack(rs.score)
    assert x.dtype == torch.int64 and tuple(x.shape) == (len(want),) and x.is_contiguous()
    assert x.device.type == ("cuda" if where == "device" else "cpu") and x.tolist() == want, where
    if where == "device":
        assert x.device.index == 0 and rs.score.__dlpack_device__() == (10, 0)
        try:
            memoryview(rs.score)
            raise SystemExit("a device column exported a host buffer")
        except BufferError:
            pass
    return x

def check_filtered(fr, hays, scores, ms, keep, where):
    rows = [h for h, s_ in enumerate(scores) if (s_ >= ms) == (keep == "matched")]
    assert fr.device == (0 if where == "device" else None) and fr.source_rows == len(hays)
    assert fr.tolist() == [hays[h] for h in rows] and torch.from_dlpack(fr.rows).tolist() == rows, (where, ms, keep)

for mk, ov in ((0, False), (0, True), (1, False), (2, False)):
    o = Oracle(pats, mk, KIND_DFA)
    b = ar.BytesAhoCorasick(pats, matchkind=kinds[mk])
    s = ar.AhoCorasick([p.decode() for p in pats], matchkind=kinds[mk])
    uniform = [hay[i * L:(i + 1) * L].tobytes() for i in range(nh)]
    ragged = [hay[cuts[i]:cuts[i + 1]].tobytes() for i in range(len(lens))]
    su, sr = scores_of(o, uniform, ov), scores_of(o, ragged, ov)
    d_cuts = torch.from_numpy(cuts).to("cuda:0")
    for obj in (b, s):
        x = check(obj.score_batch(t, w, overlapping=ov, row_length=L), su, "device")   # a tensor in HBM: the result stays there
        check(obj.score_batch(t, torch.tensor(w), ov, offsets=d_cuts), sr, "device")
        # the same numbers from the tally: the CSR matrix of per-row pattern counts times the weights
        pc = obj.count_by_pattern_sparse_batch(t, overlapping=ov, row_length=L)
        csr = torch.sparse_csr_tensor(*map(torch.from_dlpack, (pc.row_offsets, pc.pattern, pc.count)), size=pc.shape)
        dense = csr.to_dense().cpu()
        assert torch.equal(dense @ torch.tensor(w, dtype=torch.int64), x.cpu())
    check(b.score_batch(torch.from_numpy(hay), w, overlapping=ov, row_length=L), su, "host")
    check(b.score_batch(torch.from_numpy(hay), np.asarray(w, dtype=np.int32), overlapping=ov, offsets=torch.from_numpy(cuts)), sr, "host")
    check(b.score_batch(uniform, w, overlapping=ov), su, "host")
    for keep in ("unmatched", "matched"):
        for ms in (-3, 0, 1, 7):
            check_filtered(b.filter_by_score_batch(t, w, overlapping=ov, keep=keep, min_score=ms, row_length=L), uniform, su, ms, keep, "device")
            check_filtered(b.filter_by_score_batch(t, w, ov, keep=keep, min_score=ms, offsets=d_cuts), ragged, sr, ms, keep, "device")
        check_filtered(b.filter_by_score_batch(torch.from_numpy(hay), w, ov, keep=keep, row_length=L), uniform, su, 1, keep, "host")

o, b = Oracle(pats, 0, KIND_DFA), ar.BytesAhoCorasick(pats)
# an odd device address; the consumer on a stream of its own
side = torch.cuda.Stream()
odd = [hay[5 + i * L:5 + (i + 1) * L].tobytes() for i in range(100)]
with torch.cuda.stream(side):
    x = check(b.score_batch(t[5:5 + 100 * L], w, row_length=L), scores_of(o, odd, False), "device")
    total = x.sum()
assert int(total) == sum(scores_of(o, odd, False))

def raises(exc, call):
    try:
        call()
    except exc:
        return
    raise SystemExit("no %s" % exc.__name__)
raises(TypeError, lambda: b.score_batch(t, w))                                   # neither offsets nor row_length
raises(TypeError, lambda: b.score_batch(t, w, row_length=L, offsets=torch.from_numpy(cuts).to("cuda:0")))
raises(ValueError, lambda: b.score_batch(t, w, offsets=torch.from_numpy(cuts)))  # offsets on another device
raises(ValueError, lambda: b.score_batch(t, w[:-1], row_length=L))
raises(ValueError, lambda: b.filter_by_score_batch(t, w, row_length=L, keep="some"))

# no rows, and rows without a match: the score still becomes a tensor
rs = b.score_batch(torch.zeros(0, dtype=torch.uint8, device="cuda:0"), w, row_length=7)
assert len(rs) == 0 and rs.tolist() == [] and tuple(torch.from_dlpack(rs.score).shape) == (0,)
z = torch.full((1 << 20,), 48, dtype=torch.uint8, device="cuda:0")
assert not torch.from_dlpack(b.score_batch(z, w, row_length=1 << 10).score).any()

# lifetime: the tensor keeps the result alive after the RowScores object is gone
uniform = [hay[i * L:(i + 1) * L].tobytes() for i in range(nh)]
want = scores_of(o, uniform, False)
rs = b.score_batch(t, w, row_length=L)
x = torch.from_dlpack(rs.score)
unused = rs.score.__dlpack__()
del rs, unused
gc.collect()
for k in range(6):  # (other results come and go where the scores would be if they had been given back)
    other = torch.from_numpy(gen.gen_textlike(L * nh, 40 + k, pats).copy()).to("cuda:0")
    keep = b.score_batch(other, w, row_length=L)
    del keep
gc.collect()
torch.cuda.synchronize()
assert x.tolist() == want
del x
gc.collect()
assert torch.equal(t.cpu(), torch.from_numpy(hay))
print("OK")
"""


def test_tensors_in_and_torch_out():
    """score_batch and filter_by_score_batch on tensors in HBM with offsets and with row_length, both classes; torch.from_dlpack
    of the score on the automaton's device; the tally's CSR matrix times the weights gives the same numbers; errors; empty
    results; lifetime.  In a process of its own: torch has to be the first to load the HIP runtime."""
    pytest.importorskip("torch")
    p = subprocess.run([sys.executable, "-c", _TENSOR_SCRIPT, ROOT, os.path.join(ROOT, "tests")], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
