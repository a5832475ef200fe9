"""Rows of a batch kept or dropped by match, on the device (acx_filter / acx_filter_device / acx_filter_rows_device;
filter_batch): the device stage alone at the seams of its gather kernel -- source residues, rows around the tile size, row
boundaries at every residue, more rows in a tile than one LDS window, runs of kept empty rows, the shortcuts -- with guards
around the three outputs; parity with the definition through the C ABI for every match kind, on host and device inputs, for
finds that were cut or took the dense path; the Python method with sequences and with tensors in HBM, torch as the consumer
of the result, lifetime, threads and a seeded random loop.  Expected values come from numpy over synthetic counts or from
the oracle's matches (tests/oracle_lib.py) and the definition restated below, never from the library; the kernel's seams
are read from its header."""
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


def hip_constants(path, names):
    src = open(os.path.join(CSRC, path)).read()
    out = {}
    for n in names:
        m = re.search(r"\b%s\s*=\s*(\d+)\s*[,;]" % n, src)
        assert m, f"{n} is no longer a plain constant of {path}"
        out[n] = int(m.group(1))
    return out


_C = hip_constants("filter.hpp", ("FILTER_THREADS", "FILTER_TILE", "FILTER_WIN"))
THREADS, T, W = _C["FILTER_THREADS"], _C["FILTER_TILE"], _C["FILTER_WIN"]
SCAN_ITEMS = 2048  # replace_scan's items per workgroup (replace.hip RS_THREADS * RS_PER): beyond it the scan has two levels
GUARD = 0xC3


def test_constants_are_what_the_sizes_below_assume():
    assert T % (16 * THREADS) == 0 and THREADS % 64 == 0 and W < T and T >= 4096
    src = open(os.path.join(CSRC, "replace.hip")).read()
    assert re.search(r"RS_THREADS = 256, RS_PER = 8\b", src), "the scan's level size is no longer 2048"
    assert capi.FILTER_KEEP_MATCHED == MATCHED


# ---------------------------------------------------------------------------
# the stage alone
# ---------------------------------------------------------------------------
def source_bytes(lengths):
    """byte i = a value that depends on i and on its row: a shifted or misattributed byte shows"""
    lengths = np.asarray(lengths, dtype=np.int64)
    n = int(lengths.sum())
    i = np.arange(n, dtype=np.int64)
    row = np.repeat(np.arange(len(lengths), dtype=np.int64), lengths)
    return ((i * 7 + (i >> 8) * 3 + row * 13 + 1) & 0xFF).astype(np.uint8)


def expected_stage(lengths, counts, min_matches, flags, hay):
    lengths, counts = np.asarray(lengths, dtype=np.int64), np.asarray(counts, dtype=np.int64)
    kept = (counts >= min_matches) == bool(flags & MATCHED)
    rows = np.flatnonzero(kept).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(lengths[kept])]).astype(np.int64)
    return rows, offsets, hay[np.repeat(kept, lengths)]


def run_stage(lengths, counts, min_matches, flags, residue=0, uniform=False):
    """filter_rows_device on synthetic bytes and counts with guard bytes before, between and after the three outputs ->
    (rows, offsets, data), guards checked"""
    lengths = np.asarray(lengths, dtype=np.uint64)
    n, total_in = len(lengths), int(lengths.sum())
    hay = source_bytes(lengths)
    d_hay = capi.DeviceBuffer(total_in + 64)
    d_hay.upload(np.concatenate([np.full(residue, 0xEE, np.uint8), hay, np.full(64 - residue, 0xEE, np.uint8)]))
    d_c = capi.DeviceBuffer(max(8 * n, 8))
    d_o = capi.DeviceBuffer(8 * (n + 1))
    if n:
        d_c.upload(np.asarray(counts, dtype=np.uint64))
    d_o.upload(np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64))
    # [16 g][rows: n words][16 g][offsets: n + 1 words][16 .. 31 g][data: round_up(len, 16)][32 g]
    at_r = 16
    at_o = at_r + 8 * n + 16
    at_d = (at_o + 8 * (n + 1) + 16 + 15) // 16 * 16
    room = (total_in + 15) // 16 * 16
    image = np.full(at_d + room + 32, GUARD, dtype=np.uint8)
    out = capi.DeviceBuffer(len(image)).upload(image)
    assert out.ptr % 16 == 0
    ulen = int(lengths[0]) if uniform else 0
    if uniform:
        assert n and (lengths == lengths[0]).all() and ulen
    k, nb = capi.filter_rows_device(d_hay.ptr + residue, total_in, 0 if uniform else d_o.ptr, n, ulen, d_c.ptr if n else 0,
                                    min_matches, flags, out.ptr + at_r if n else 0, out.ptr + at_o, out.ptr + at_d if total_in else 0)
    got = np.empty(len(image), dtype=np.uint8)
    capi._check(capi.lib().acx_device_download(got.ctypes.data, out.ptr, len(image)))
    src_after = d_hay.download(total_in + 64)
    for b in (d_hay, d_c, d_o, out):
        b.free()
    assert np.array_equal(src_after[residue:residue + total_in], hay), "the input was written"
    assert 0 <= k <= n and 0 <= nb <= total_in
    written = (nb + 15) // 16 * 16  # (the bytes behind the data up to the next multiple of 16 may be written)
    for lo, hi in ((0, at_r), (at_r + 8 * k, at_o), (at_o + 8 * (k + 1), at_d), (at_d + written, len(image))):
        assert (got[lo:hi] == GUARD).all(), ("a byte outside the outputs was written", lo, hi, int(np.flatnonzero(got[lo:hi] != GUARD)[0]))
    return (got[at_r:at_r + 8 * k].view(np.int64), got[at_o:at_o + 8 * (k + 1)].view(np.int64), got[at_d:at_d + nb])


def check_stage(lengths, counts, min_matches=1, flags=0, residue=0, uniform=False, what=None):
    got = run_stage(lengths, counts, min_matches, flags, residue, uniform)
    want = expected_stage(lengths, counts, min_matches, flags, source_bytes(lengths))
    for name, g, w in zip(("rows", "offsets", "data"), got, want):
        if len(g) != len(w) or not np.array_equal(g, w):
            m = min(len(g), len(w))
            bad = int(np.flatnonzero(g[:m] != w[:m])[:1].sum())
            raise AssertionError((what, name, "lengths", len(g), len(w), "first difference at", bad, g[bad:bad + 8], w[bad:bad + 8]))
    return want


def alternate(n, first=1):
    return [(i + first) & 1 for i in range(n)]


def test_stage_source_residues_against_output_tiles():
    """every residue of the source pointer; rows of T - 1, T, T + 1 and 6 T + 5 bytes; the dropped rows between them move
    the kept ones' shifts to other residues; the last tile partly filled"""
    lengths = [5, T - 1, 3, T, 11, T + 1, 0, 6 * T + 5, 40, 9]
    for residue in range(16):
        for counts in (alternate(len(lengths)), alternate(len(lengths), 0)):
            check_stage(lengths, counts, residue=residue, what=("residue", residue, counts[0]))


def test_stage_row_that_begins_at_the_last_byte_of_a_tile_and_exact_totals():
    check_stage([T - 1, 7, 300, 2 * T], [0, 1, 0, 0], what="begins at a tile's last byte")       # output: T - 1, then 300 ...
    check_stage([T - 1, 5, 1, 9], [0, 1, 0, 1], what="a total of exactly T")
    check_stage([T - 1, 5, 2, 9], [0, 1, 0, 1], what="a total of T + 1")
    check_stage([T, 5], [0, 1], what="one row of exactly T")
    check_stage([3, T, 5, T, 1], [1, 0, 1, 0, 1], what="rows end where tiles end")
    want = check_stage([T - 1, 5, 1, 9], [0, 1, 0, 1])
    assert len(want[2]) == T
    want = check_stage([T - 1, 5, 2, 9], [0, 1, 0, 1])
    assert len(want[2]) == T + 1


def test_stage_row_boundaries_at_every_residue():
    rng = np.random.default_rng(3)
    lengths = [1 + (i * 5) % 41 for i in range(4000)]  # boundaries walk over every residue mod 16, over several tiles
    assert sum(lengths) > 4 * T and len({sum(lengths[:i]) % 16 for i in range(200)}) == 16
    for flags in (0, MATCHED):
        check_stage(lengths, rng.integers(0, 2, size=len(lengths)), flags=flags, residue=3, what=("boundaries", flags))
    check_stage(lengths, rng.choice([0, 0, 0, 1], size=len(lengths)), flags=MATCHED, what="sparse keep")


def test_stage_more_rows_in_a_tile_than_one_window_and_runs_of_empty_rows():
    """1-byte rows (more than W of them inside one tile: several rounds), and runs of kept empty rows -- longer than a window
    -- on both sides of a tile boundary and at the very end"""
    assert 3 * W + 100 < T
    lengths = [T - 2] + [0] * 5 + [1, 1] + [0] * (2 * W + 7) + [7] + [1] * (3 * W + 100) + [0] * 3 + [T] + [0] * (W + 9)
    n = len(lengths)
    check_stage(lengths, [0] * n, what="all kept goes the copy's way")
    counts = [0] * n
    counts[n // 2] = 1  # (one dropped row: the gather runs)
    check_stage(lengths, counts, what="all but one kept")
    counts = [0] * n
    counts[0] = 1       # (the first tile begins in the run of empty rows)
    check_stage(lengths, counts, what="empty rows first")
    rng = np.random.default_rng(9)
    for _ in range(2):
        check_stage(lengths, rng.choice([0, 0, 0, 1], size=n), residue=int(rng.integers(16)), what="random")
    only_bytes = [T - 5] + [1] * (2 * T + 11)
    check_stage(only_bytes, [1] + [0] * (2 * T + 11), what="whole tiles of 1-byte rows")
    check_stage(only_bytes, alternate(len(only_bytes)), what="every other 1-byte row")


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, THREADS - 1, THREADS, THREADS + 1, SCAN_ITEMS, SCAN_ITEMS + 1, 3 * SCAN_ITEMS + 5])
def test_stage_row_counts_and_keep_patterns(n):
    """n at the seams of the per-row kernels and of the scan (two levels beyond SCAN_ITEMS); none kept, all kept (the copy
    shortcut), all but the first, all but the last, every other row; both keep modes and min_matches"""
    rng = np.random.default_rng(n)
    lengths = rng.choice([0, 1, 15, 16, 17, 100], size=n)
    ones, zeros = [1] * n, [0] * n
    check_stage(lengths, ones, what="none kept")
    check_stage(lengths, zeros, what="all kept")
    check_stage(lengths, ones, flags=MATCHED, what="all kept, matched")
    if n:
        check_stage(lengths, [1] + [0] * (n - 1), what="all but the first")
        check_stage(lengths, [0] * (n - 1) + [1], what="all but the last")
        check_stage(lengths, alternate(n), what="every other")
        counts = rng.choice([0, 1, 2, 3, 5, 9], size=n)
        for mm in (1, 3, 5, 10):
            for flags in (0, MATCHED):
                check_stage(lengths, counts, mm, flags, what=("min_matches", mm, flags))


def test_stage_uniform_rows_and_one_row():
    for ulen, n in ((37, 1000), (1, 5), (T + 3, 5), (16, 64)):
        for counts in (alternate(n), [0] * n, [1] * n):
            check_stage([ulen] * n, counts, uniform=True, residue=ulen % 16, what=("uniform", ulen, n, counts[:2]))
    # one row that is no batch (neither offsets nor uniform_len)
    hay = source_bytes([1000])
    d_hay, d_c, out = capi.DeviceBuffer(1024).upload(hay), capi.DeviceBuffer(8), capi.DeviceBuffer(2048)
    for count, flags, kept in ((2, MATCHED, True), (2, 0, False), (0, 0, True)):
        d_c.upload(np.asarray([count], dtype=np.uint64))
        k, nb = capi.filter_rows_device(d_hay.ptr, 1000, 0, 1, 0, d_c.ptr, 1, flags, out.ptr, out.ptr + 256, out.ptr + 512)
        assert (k, nb) == ((1, 1000) if kept else (0, 0))
        words = out.download(2048)
        assert words[256:264].view(np.int64)[0] == 0
        if kept:
            assert words[0:8].view(np.int64)[0] == 0 and words[264:272].view(np.int64)[0] == 1000
            assert np.array_equal(words[512:1512], hay)
    for b in (d_hay, d_c, out):
        b.free()


def test_stage_refuses_bad_arguments():
    d = capi.DeviceBuffer(4096)
    d.upload(np.asarray([0, 8, 99], dtype=np.uint64))  # (a wrong last entry: refused before any kernel runs)
    args = dict(d_hay=d.ptr + 1024, nbytes=16, d_offsets=d.ptr, n_hay=2, uniform_len=0, d_counts=d.ptr + 512, min_matches=1,
                flags=0, d_rows=d.ptr + 2048, d_out_offsets=d.ptr + 2304, d_data=d.ptr + 3072)
    for change in (dict(), dict(flags=2), dict(min_matches=0), dict(d_data=d.ptr + 3080), dict(d_rows=d.ptr + 2052),
                   dict(uniform_len=8), dict(d_offsets=0, uniform_len=7)):
        with pytest.raises(ValueError) as ei:
            capi.filter_rows_device(**{**args, **change})
        assert ei.value.code == capi.EINVAL, change
    d.free()


# ---------------------------------------------------------------------------
# end to end through the C ABI against the oracle
# ---------------------------------------------------------------------------
PATS = gen.gen_patterns(500, 3, 9, gen.AZ, 5) + [b"ab", b"abab", b"bab", b"ab"]  # (a copy: overlapping reports it)
KINDS = [(0, False), (0, True), (1, False), (2, False)]


def definition(hays, counts, min_matches, keep_matched):
    """the issue's definition from the per-row match counts -> (rows, offsets, data)"""
    rows, offsets, data = [], [0], []
    for h, (hay, c) in enumerate(zip(hays, counts)):
        if (c >= min_matches) == keep_matched:
            rows.append(h)
            data.append(hay)
            offsets.append(offsets[-1] + len(hay))
    return np.asarray(rows, np.int64), np.asarray(offsets, np.int64), np.frombuffer(b"".join(data), np.uint8)


def oracle_counts(o, hays, ov):
    return [len(o.find_raw(h, overlapping=ov)) for h in hays]


def download_bytes(ptr, n):
    out = np.empty(n, dtype=np.uint8)
    if n:
        capi._check(capi.lib().acx_device_download(out.ctypes.data, ptr, n))
    return out


def check_filtered(f, want, on_device, what=None):
    """a capi.DeviceFiltered against the definition, through the copies and through the raw addresses"""
    rows, offsets, data = want
    assert f.on_device == on_device and f.n_rows == len(rows) and f.nbytes == len(data), (what, f.n_rows, f.nbytes, len(rows), len(data))
    for k, w in ((capi.FILT_ROWS, rows), (capi.FILT_OFFSETS, offsets), (capi.FILT_DATA, data)):
        assert np.array_equal(f.part(k), w), (what, k)
        p = f.data_ptr(k)
        assert p and p % 8 == 0, (what, k)  # (an empty part still has an address)
        if on_device:
            assert p % 256 == 0 and np.array_equal(download_bytes(p, w.nbytes), w.view(np.uint8)), (what, k)
        else:
            assert np.array_equal(np.ctypeslib.as_array((capi.ctypes.c_uint8 * max(w.nbytes, 1)).from_address(p))[:w.nbytes], w.view(np.uint8))
    f.free()


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


def device_filter(a, hays, off, **kw):
    """the batch behind one another in HBM at `off` modulo 16, ragged offsets on the device -> DeviceFiltered"""
    blob = b"".join(hays)
    offs = np.concatenate([[0], np.cumsum([len(h) for h in hays])]).astype(np.uint64)
    d_hay = capi.DeviceBuffer(len(blob) + 32).upload(np.frombuffer(b"\xa5" * off + blob, dtype=np.uint8))
    d_off = capi.DeviceBuffer(8 * len(offs)).upload(offs)
    f = a.filter_device(d_hay.ptr + off, len(blob), d_offsets=d_off.ptr, n_hay=len(hays), **kw)
    f.n_rows, f.nbytes  # (known at return)
    return f, (d_hay, d_off)


@pytest.mark.parametrize("mk,ov", KINDS)
def test_parity_host_and_device_inputs(monkeypatch, mk, ov):
    o = Oracle(PATS, mk, KIND_DFA)
    a = capi.Automaton(PATS, mk)
    for n_hay in (1, 65, 323):
        hays = batch_with_empties(PATS, n_hay, 100 + n_hay)
        counts = oracle_counts(o, hays, ov)
        for mm in (1, 3):
            for flags in (0, MATCHED):
                want = definition(hays, counts, mm, bool(flags))
                for host_max in ("0", str(1 << 40)):  # the summary's device route and its host route: a host result either way
                    monkeypatch.setenv("ACX_SUMMARY_HOST_MAX", host_max)
                    check_filtered(a.filter(hays, ov, mm, flags), want, False, (mk, ov, n_hay, mm, flags, host_max))
                monkeypatch.delenv("ACX_SUMMARY_HOST_MAX")
                for off in (0, 5):
                    f, keep = device_filter(a, hays, off, overlapping=ov, min_matches=mm, flags=flags)
                    check_filtered(f, want, True, (mk, ov, n_hay, mm, flags, off))
                    for k in keep:
                        k.free()
    # a uniform batch on the device, and the same bytes as a host batch
    L, nh = 512, 130
    full = gen.gen_textlike(L * nh, 61, PATS).tobytes()
    hays = [full[i * L:(i + 1) * L] for i in range(nh)]
    counts = oracle_counts(o, hays, ov)
    dev = capi.DeviceBuffer(len(full)).upload(np.frombuffer(full, dtype=np.uint8))
    for mm in (1, 3):
        for flags in (0, MATCHED):
            want = definition(hays, counts, mm, bool(flags))
            check_filtered(a.filter_device(dev.ptr, len(full), n_hay=nh, uniform_len=L, overlapping=ov, min_matches=mm, flags=flags),
                           want, True, ("uniform", mm, flags))
            check_filtered(a.filter(hays, ov, mm, flags), want, False, ("uniform, host", mm, flags))
    dev.free()
    a.close()


def test_one_haystack_that_is_no_batch_and_empty_batches():
    o, a = Oracle(PATS, 0, KIND_DFA), capi.Automaton(PATS, 0)
    for hay in (gen.gen_textlike(5000, 3, PATS).tobytes(), b"0123" * 100, b""):
        c = oracle_counts(o, [hay], False)
        dev = capi.DeviceBuffer(len(hay) + 16).upload(np.frombuffer(hay + b"\0", dtype=np.uint8))
        for flags in (0, MATCHED):
            want = definition([hay], c, 1, bool(flags))
            check_filtered(a.filter(None, False, 1, flags, single=hay), want, False, ("single", len(hay), flags))
            check_filtered(a.filter_device(dev.ptr, len(hay), flags=flags), want, True, ("single, device", len(hay), flags))
        dev.free()
    none = definition([], [], 1, False)
    check_filtered(a.filter([]), none, False, "empty batch")
    dev = capi.DeviceBuffer(64)
    check_filtered(a.filter_device(dev.ptr, 0, n_hay=0, uniform_len=8), none, True, "empty batch, device")
    dev.free()
    for bad in (dict(flags=2), dict(min_matches=0)):
        with pytest.raises(ValueError) as ei:
            a.filter([b"ab"], **bad)
        assert ei.value.code == capi.EINVAL
        with pytest.raises(ValueError) as ei:
            a.filter_device(0, 0, n_hay=0, uniform_len=8, **bad)
        assert ei.value.code == capi.EINVAL
    b = capi.Automaton([b"ab", b"b"], 1)
    for call in (lambda: b.filter([b"xxabxx"], overlapping=True), lambda: b.filter_device(0, 0, n_hay=0, uniform_len=8, overlapping=True)):
        with pytest.raises(ValueError) as ei:
            call()
        assert ei.value.code == capi.EOVERLAP
    b.close()
    a.close()


def test_results_freed_unread_and_in_reverse_order():
    """the seams of the result's owner: a result freed with no accessor ever called (the free waits for the stage) and the
    identical call after it, whose blocks come from the cache; eight results alive at once, four freed unread in the opposite
    order to their creation, a result made where their blocks went, and the other four read afterwards"""
    pats = [b"ab", b"abab", b"bab", b"needle", b"hay", b"stack", b"a", b"zz", b"0123", b"ab"]
    o, a = Oracle(pats, 0, KIND_DFA), capi.Automaton(pats, 0)
    batches = [[gen.gen_textlike([0, 7, 64, 255][(i + k) % 4], 50 + 8 * k + i, pats).tobytes() for i in range(5 + 7 * k)] for k in range(8)]
    want = [definition(hays, oracle_counts(o, hays, True), 2, bool(k % 2)) for k, hays in enumerate(batches)]
    kw = [dict(overlapping=True, min_matches=2, flags=MATCHED * (k % 2)) for k in range(8)]
    f, keep = device_filter(a, batches[3], 0, **kw[3])
    f.free()
    f, keep2 = device_filter(a, batches[3], 0, **kw[3])
    check_filtered(f, want[3], True, "the second call")
    made = [device_filter(a, hays, 0, **kw[k]) for k, hays in enumerate(batches)]
    for k in (7, 6, 5, 4):
        made[k][0].free()
    f, keep3 = device_filter(a, batches[6], 0, **kw[6])
    check_filtered(f, want[6], True, "behind the four freed")
    for k in (3, 2, 1, 0):
        check_filtered(made[k][0], want[k], True, k)
    for d in [*keep, *keep2, *keep3] + [d for _, ks in made for d in ks]:
        d.free()
    a.close()


def test_case_insensitive_handle_keeps_the_callers_case():
    pats = [b"Needle", b"hay", b"STACK"]
    o = Oracle([p.translate(FOLD) for p in pats], 1, KIND_DFA)
    hays = [b"a nEEdle in a HayStack; " * 3, b"Nothing Here", b"", b"NEEDLE", b"x" * 5000 + b"hAY", b"NO", b"needle HAY stack" * 900]
    counts = oracle_counts(o, [h.translate(FOLD) for h in hays], False)
    assert counts[0] and counts[3] == 1 and not counts[1]
    a = capi.Automaton(pats, 1, ascii_case_insensitive=True)
    for mm in (1, 3):
        for flags in (0, MATCHED):
            want = definition(hays, counts, mm, bool(flags))  # (the caller's unfolded bytes)
            check_filtered(a.filter(hays, False, mm, flags), want, False, (mm, flags))
            f, keep = device_filter(a, hays, 5, min_matches=mm, flags=flags)
            check_filtered(f, want, True, (mm, flags))
            assert np.array_equal(keep[0].download(5 + sum(map(len, hays)))[5:], np.frombuffer(b"".join(hays), dtype=np.uint8))
            for k in keep:
                k.free()
    a.close()


def test_copies_count_under_overlapping():
    pats = [b"ab", b"ab", b"ab", b"b"]
    o, a = Oracle(pats, 0, KIND_DFA), capi.Automaton(pats, 0)
    hays = [b"ab", b"xx", b"abab", b"b", b"", b"xab"]
    for ov in (False, True):
        counts = oracle_counts(o, hays, ov)
        assert counts[0] == (4 if ov else 1)
        for mm in (1, 3, 4, 5):
            for flags in (0, MATCHED):
                want = definition(hays, counts, mm, bool(flags))
                check_filtered(a.filter(hays, ov, mm, flags), want, False, (ov, mm, flags))
                f, keep = device_filter(a, hays, 1, overlapping=ov, min_matches=mm, flags=flags)
                check_filtered(f, want, True, (ov, mm, flags))
                for k in keep:
                    k.free()
    a.close()


def test_a_find_cut_into_byte_ranges(monkeypatch):
    o, a = Oracle(PATS, 0, KIND_DFA), capi.Automaton(PATS, 0)
    hay = gen.gen_textlike(3_000_000, 17, PATS).tobytes()
    c = oracle_counts(o, [hay], False)
    dev = capi.DeviceBuffer(len(hay)).upload(np.frombuffer(hay, dtype=np.uint8))
    monkeypatch.setenv("ACX_CHUNK_BYTES", "700001")
    a.path_stats(reset=True)
    for mm, flags in ((1, MATCHED), (c[0], MATCHED), (c[0] + 1, MATCHED), (c[0] + 1, 0)):
        check_filtered(a.filter_device(dev.ptr, len(hay), min_matches=mm, flags=flags), definition([hay], c, mm, bool(flags)), True, (mm, flags))
    st = a.path_stats()
    monkeypatch.delenv("ACX_CHUNK_BYTES")
    assert st["byte_ranges"] >= 2, st
    dev.free()
    a.close()


def test_a_find_on_the_dense_path():
    pats = gen.gen_patterns(2000, 5, 12, gen.AZ, 1)
    a, o = capi.Automaton(pats, 0, capi.IMPL_DFA), Oracle(pats, 0, KIND_DFA)
    every = bytearray(gen.gen_uniform(8 << 20, gen.AZ, 13).tobytes())  # (the size tests/test_gpu_columns.py uses)
    rng = gen.SplitMix64(77)
    for k in range(0, len(every) - 32, 32):
        if (k >> 16) % 3 == 0 and k % 4096:  # (every third row keeps a handful of plants only)
            continue
        p = pats[rng.next() % len(pats)]
        every[k:k + len(p)] = p
    every = bytes(every)
    L = 1 << 16
    hays = [every[i:i + L] for i in range(0, len(every), L)]
    counts = oracle_counts(o, hays, False)
    mm = (min(counts) + max(counts)) // 2
    assert min(counts) < mm < max(counts)
    dev = capi.DeviceBuffer(len(every)).upload(np.frombuffer(every, dtype=np.uint8))
    a.path_stats(reset=True)
    total = [len(o.find_raw(every))]
    for _ in range(2):  # (one haystack that is no batch: the call tests/test_gpu_columns.py sees take that path)
        check_filtered(a.filter_device(dev.ptr, len(every), min_matches=total[0], flags=MATCHED), definition([every], total, total[0], True), True)
    st = a.path_stats()
    assert st["hot_calls"] + st["dense_tiles"] + st["dense_radix"] >= 2, st
    for flags in (0, MATCHED):
        check_filtered(a.filter_device(dev.ptr, len(every), n_hay=len(hays), uniform_len=L, min_matches=mm, flags=flags),
                       definition(hays, counts, mm, bool(flags)), True, ("dense", flags))
    dev.free()
    a.close()


def test_eight_threads_on_one_handle():
    a, o = capi.Automaton(PATS, 0), Oracle(PATS, 0, KIND_DFA)
    work = []
    for t in range(8):
        hays = batch_with_empties(PATS, 40 + 9 * t, 300 + t) + [gen.gen_textlike(150_000, t, PATS).tobytes()]
        work.append((hays, oracle_counts(o, hays, False)))
    errors = []

    def run(t):
        try:
            hays, counts = work[t]
            for i in range(3):
                flags = (t + i) & 1
                want = definition(hays, counts, 1 + i, bool(flags))
                check_filtered(a.filter(hays, False, 1 + i, flags), want, False, t)
                f, keep = device_filter(a, hays, t, min_matches=1 + i, flags=flags)
                check_filtered(f, want, True, t)
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
    rng = random.Random(20261018)
    for case in range(40):
        mk = rng.choice([0, 0, 1, 2])
        ov = mk == 0 and rng.random() < 0.4
        alpha = rng.choice([b"ab", b"abcd", gen.AZ])
        pats = gen.gen_patterns(rng.choice([1, 3, 40, 600]), 1, rng.choice([2, 6, 12]), alpha, 1000 + case)
        text = rng.choice([alpha, alpha + b"xyz", b"0123"])
        o = Oracle(pats, mk, KIND_DFA)
        n_hay = rng.choice([1, 2, 7, 64, 65, 130, 700])
        hays = [bytes(rng.choices(text, k=rng.choice([0, 0, 1, 9, 200, 5000, 20000]))) for _ in range(n_hay)]
        counts = oracle_counts(o, hays, ov)
        while sum(counts) > 100_000:  # (cut down, never skipped)
            hays = [h[:len(h) // 2] for h in hays]
            counts = oracle_counts(o, hays, ov)
        mm = rng.choice([1, 1, 2, 3, max(1, sorted(counts)[len(counts) // 2])])
        flags = rng.choice([0, MATCHED])
        route = rng.choice(["host", "staged", "device", "device"])
        monkeypatch.setenv("ACX_SUMMARY_HOST_MAX", "0" if route == "staged" else str(1 << 40))
        a = capi.Automaton(pats, mk)
        what = (case, mk, ov, n_hay, route, mm, flags)
        want = definition(hays, counts, mm, bool(flags))
        try:
            if route == "device":
                f, keep = device_filter(a, hays, rng.randrange(16), overlapping=ov, min_matches=mm, flags=flags)
                check_filtered(f, want, True, what)
                for k in keep:
                    k.free()
            else:
                check_filtered(a.filter(hays, ov, mm, flags), want, False, what)
        except AssertionError as e:
            raise AssertionError(f"case {what}: {e}") from e
        a.close()


# ---------------------------------------------------------------------------
# the Python method: sequences of host objects (tensors in HBM and torch as the consumer: the script below)
# ---------------------------------------------------------------------------
def matchkind(ar, mk):
    return (ar.MatchKind.Standard, ar.MatchKind.LeftmostFirst, ar.MatchKind.LeftmostLongest)[mk]


def check_rows(fr, hays, want, text):
    """a FilteredRows in host memory against the definition"""
    rows, offsets, data = want
    assert len(fr) == len(rows) and fr.nbytes == len(data) and fr.source_rows == len(hays) and fr.device is None
    kept = [hays[h] for h in rows]
    assert fr.tolist() == ([k.decode() for k in kept] if text else kept)
    for col, w, fmt in ((fr.rows, rows, "q"), (fr.offsets, offsets, "q"), (fr.data, data, "B")):
        assert len(col) == len(w) and col.__dlpack_device__() == (1, 0)
        got = np.from_dlpack(col)
        assert got.dtype == w.dtype and np.array_equal(got, w)
        mv = memoryview(col)
        assert mv.format == fmt and mv.readonly and mv.itemsize == w.itemsize and np.array_equal(np.asarray(mv), w)


@pytest.mark.parametrize("mk,ov", KINDS)
def test_python_sequences_both_classes(mk, ov):
    import ahocorasick_rs as ar
    o = Oracle(PATS, mk, KIND_DFA)
    b = ar.BytesAhoCorasick(PATS, matchkind=matchkind(ar, mk))
    s = ar.AhoCorasick([p.decode() for p in PATS], matchkind=matchkind(ar, mk))
    for n_hay in (0, 1, 64, 130):
        hays = batch_with_empties(PATS, n_hay, 500 + n_hay)
        counts = oracle_counts(o, hays, ov)
        assert [len(m) for m in b.find_matches_as_indexes_batch(hays, overlapping=ov)] == counts  # (the definition's c[h])
        for keep in ("unmatched", "matched"):
            for mm in (1, 3):
                want = definition(hays, counts, mm, keep == "matched")
                check_rows(b.filter_batch(hays, overlapping=ov, keep=keep, min_matches=mm), hays, want, False)
                check_rows(b.filter_batch(tuple(bytearray(h) for h in hays), ov, keep=keep, min_matches=mm), hays, want, False)
                check_rows(s.filter_batch([h.decode() for h in hays], overlapping=ov, keep=keep, min_matches=mm), hays, want, True)
    check_rows(b.filter_batch([b"xx", b"ab"]), [b"xx", b"ab"], definition([b"xx", b"ab"], [0, 1 + ov], 1, False), False)  # the defaults
    # text that is not ASCII: rows are cut at their bytes, tolist() decodes them
    pats = ["é☃", "ab", "b🤦", "☃", "ab"]
    o2 = Oracle([p.encode() for p in pats], mk, KIND_DFA)
    s2 = ar.AhoCorasick(pats, matchkind=matchkind(ar, mk))
    hays = ["", "ab☃é☃b🤦", "xxé☃" * 50, "🤦🤦ab", "é" * 3000 + "☃ab" * 4000, "ü", "日本語"]
    enc = [h.encode() for h in hays]
    for keep in ("unmatched", "matched"):
        check_rows(s2.filter_batch(hays, overlapping=ov, keep=keep), enc, definition(enc, oracle_counts(o2, enc, ov), 1, keep == "matched"), True)


def test_python_errors_and_host_tensors():
    import ahocorasick_rs as ar
    b, s = ar.BytesAhoCorasick([b"ab"]), ar.AhoCorasick(["ab"])
    off = np.array([0, 2], dtype=np.int64)
    for call in (lambda: b.filter_batch([b"ab"], offsets=off),          # either keyword with a sequence
                 lambda: b.filter_batch([b"ab"], row_length=2),
                 lambda: b.filter_batch([b"ab"], False, "matched"),     # keyword-only
                 lambda: b.filter_batch(["ab"]),                        # the items' types
                 lambda: s.filter_batch([b"ab"]),
                 lambda: b.filter_batch(5),
                 lambda: b.filter_batch([b"ab"], overlapping=1),
                 lambda: b.filter_batch([b"ab"], min_matches=True),     # a bool or a non-int, as row_length
                 lambda: b.filter_batch([b"ab"], min_matches=2.0),
                 lambda: b.filter_batch([b"ab"], min_matches="2"),
                 lambda: b.filter_batch([b"ab"], keep=1),
                 lambda: b.filter_batch([b"ab"], keep=b"matched")):
        with pytest.raises(TypeError):
            call()
    for call in (lambda: b.filter_batch([b"ab"], keep="both"), lambda: b.filter_batch([b"ab"], keep="Matched"),
                 lambda: b.filter_batch([b"ab"], keep=""), lambda: b.filter_batch([b"ab"], min_matches=0),
                 lambda: s.filter_batch(["ab"], min_matches=-3), lambda: b.filter_batch([b"ab"], min_matches=-(1 << 70))):
        with pytest.raises(ValueError):
            call()
    assert b.filter_batch([b"ab", b"x"], min_matches=1 << 70).tolist() == [b"ab", b"x"]  # (more than any row can have)
    t = np.frombuffer(b"abxXYxabab", dtype=np.uint8).copy()  # (writable: numpy exports no read-only array through DLPack)
    # a host tensor behind DLPack (numpy: it is a buffer too, so a keyword makes it THE tensor)
    fr = b.filter_batch(t, row_length=5, keep="matched")
    assert fr.tolist() == [b"abxXY", b"xabab"] and fr.device is None and fr.source_rows == 2
    fr = b.filter_batch(t, offsets=np.array([0, 1, 1, 6, 10], dtype=np.int64), keep="matched", min_matches=2)
    assert fr.tolist() == [b"abab"] and list(np.from_dlpack(fr.rows)) == [3] and list(np.from_dlpack(fr.offsets)) == [0, 4]
    assert s.filter_batch(t, row_length=5).tolist() == [] and s.filter_batch(t, row_length=2).tolist() == ["xX", "Yx"]
    assert memoryview(fr.data).format == "B" and bytes(memoryview(fr.data)) == b"abab"
    for call in (lambda: b.filter_batch(t, row_length=5, offsets=np.array([0, 10], dtype=np.int64)),  # both
                 lambda: b.filter_batch(t, row_length=5.0), lambda: b.filter_batch(t, offsets=[0, 10]),
                 lambda: b.filter_batch(t, offsets=np.array([0, 10], dtype=np.int32))):
        with pytest.raises(TypeError):
            call()
    for call in (lambda: b.filter_batch(t, row_length=4), lambda: b.filter_batch(t, row_length=0),
                 lambda: b.filter_batch(t, offsets=np.array([0, 5], dtype=np.int64)),
                 lambda: b.filter_batch(t, offsets=np.array([1, 10], dtype=np.int64)),
                 lambda: b.filter_batch(t, offsets=np.array([0, 4, 3, 10], dtype=np.int64))):
        with pytest.raises(ValueError):
            call()
    for mk in (ar.MatchKind.LeftmostFirst, ar.MatchKind.LeftmostLongest):
        with pytest.raises(ValueError):
            ar.BytesAhoCorasick([b"ab"], matchkind=mk).filter_batch([b"ab"], overlapping=True)
    with pytest.raises(TypeError):
        ar.FilteredRows()


def test_host_columns_outlive_the_filtered_rows():
    import ahocorasick_rs as ar
    o, b = Oracle(PATS, 0, KIND_DFA), ar.BytesAhoCorasick(PATS)
    hays = batch_with_empties(PATS, 300, 3)
    want = definition(hays, oracle_counts(o, hays, False), 1, True)
    fr = b.filter_batch(hays, keep="matched")
    arrays = [np.from_dlpack(x) for x in (fr.rows, fr.offsets, fr.data)]
    views = [memoryview(x) for x in (fr.rows, fr.offsets, fr.data)]
    unused = fr.data.__dlpack__()  # (a capsule nobody consumes gives its reference back too)
    del fr, unused
    gc.collect()
    for k in range(20):  # (other results come and go where the parts' memory would be if it had been freed)
        b.filter_batch(batch_with_empties(PATS, 300, 50 + k))
    for got, mv, w in zip(arrays, views, want):
        assert np.array_equal(got, w) and np.array_equal(np.asarray(mv), w)


# ---------------------------------------------------------------------------
# tensors in HBM through the Python method, and torch as the consumer of the result
# ---------------------------------------------------------------------------
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
L, nh = 4096, 200
hay = gen.gen_textlike(L * nh, 13, pats).copy()
hay[3 * L:9 * L] = 48   # (rows without a match)
hay[50 * L:51 * L] = 48
t = torch.from_numpy(hay.copy()).to("cuda:0")
kinds = (ar.MatchKind.Standard, ar.MatchKind.LeftmostFirst, ar.MatchKind.LeftmostLongest)
lens = [0, 0, 17, L, 3 * L, 5, 0, 2 * L + 1, 4 * L, 7, 0]
lens += [L * nh - sum(lens), 0]
cuts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)

def counts_of(o, hays, ov):
    return [len(o.find_raw(h, overlapping=ov)) for h in hays]

def definition(hays, counts, mm, keep):
    rows = [h for h, c in enumerate(counts) if (c >= mm) == (keep == "matched")]
    offs = np.concatenate([[0], np.cumsum([len(hays[h]) for h in rows])]).astype(np.int64)
    return rows, offs, b"".join(hays[h] for h in rows)

def check(fr, hays, want, where, text=False):
    rows, offs, data = want
    assert fr.device == (0 if where == "device" else None), (where, fr.device)
    assert len(fr) == len(rows) and fr.nbytes == len(data) and fr.source_rows == len(hays), (where, len(fr), len(rows))
    kept = [hays[h] for h in rows]
    assert fr.tolist() == ([k.decode() for k in kept] if text else kept), where
    parts = [torch.from_dlpack(x) for x in (fr.rows, fr.offsets, fr.data)]
    for x, n, dt in zip(parts, (len(rows), len(rows) + 1, len(data)), (torch.int64, torch.int64, torch.uint8)):
        assert x.dtype == dt and tuple(x.shape) == (n,) and x.is_contiguous(), (where, x.dtype, x.shape)
        assert x.device.type == ("cuda" if where == "device" else "cpu"), (where, x.device)
    assert parts[0].tolist() == rows and torch.equal(parts[1].cpu(), torch.from_numpy(offs)), where
    assert bytes(parts[2].cpu().numpy()) == data, where
    # the kept rows rebuilt from the three tensors
    o_, d_ = parts[1].cpu().tolist(), parts[2].cpu().numpy()
    assert [bytes(d_[o_[i]:o_[i + 1]]) for i in range(len(rows))] == kept, where
    return parts

for mk, ov in ((0, False), (0, True), (1, False), (2, False)):
    o = Oracle(pats, mk, KIND_DFA)
    b = ar.BytesAhoCorasick(pats, matchkind=kinds[mk])
    s = ar.AhoCorasick([p.decode() for p in pats], matchkind=kinds[mk])
    uniform = [hay[i * L:(i + 1) * L].tobytes() for i in range(nh)]
    ragged = [hay[cuts[i]:cuts[i + 1]].tobytes() for i in range(len(lens))]
    cu, cr = counts_of(o, uniform, ov), counts_of(o, ragged, ov)
    d_cuts = torch.from_numpy(cuts).to("cuda:0")
    for keep in ("unmatched", "matched"):
        for mm in (1, 3):
            wu, wr = definition(uniform, cu, mm, keep), definition(ragged, cr, mm, keep)
            for obj in (b, s):
                fr = obj.filter_batch(t, overlapping=ov, keep=keep, min_matches=mm, row_length=L)   # a tensor in HBM: the result stays there
                for x in (fr.rows, fr.offsets, fr.data):
                    assert x.__dlpack_device__() == (10, 0)
                    try:
                        memoryview(x)
                        raise SystemExit("a device column exported a host buffer")
                    except BufferError:
                        pass
                check(fr, uniform, wu, "device", obj is s)
                check(obj.filter_batch(t, ov, keep=keep, min_matches=mm, offsets=d_cuts), ragged, wr, "device", obj is s)
            check(b.filter_batch(torch.from_numpy(hay), overlapping=ov, keep=keep, min_matches=mm, row_length=L), uniform, wu, "host")
            check(b.filter_batch(torch.from_numpy(hay), overlapping=ov, keep=keep, min_matches=mm, offsets=torch.from_numpy(cuts)), ragged, wr, "host")
            fr = b.filter_batch(uniform, overlapping=ov, keep=keep, min_matches=mm)
            assert memoryview(fr.data).format == "B"
            check(fr, uniform, wu, "host")

o, b = Oracle(pats, 0, KIND_DFA), ar.BytesAhoCorasick(pats)
# an odd device address; the consumer on a stream of its own
side = torch.cuda.Stream()
odd = [hay[5 + i * L:5 + (i + 1) * L].tobytes() for i in range(100)]
with torch.cuda.stream(side):
    parts = check(b.filter_batch(t[5:5 + 100 * L], row_length=L, keep="matched"), odd, definition(odd, counts_of(o, odd, False), 1, "matched"), "device")
    total = parts[2].to(torch.int64).sum()
assert int(total) == sum(sum(h) for h, c in zip(odd, counts_of(o, odd, False)) if c)

# the errors of the tensor form
d_cuts = torch.from_numpy(cuts).to("cuda:0")
def raises(exc, call):
    try:
        call()
    except exc:
        return
    raise SystemExit("no %s" % exc.__name__)
raises(TypeError, lambda: b.filter_batch(t))                                   # neither
raises(TypeError, lambda: b.filter_batch(t, row_length=L, offsets=d_cuts))     # both
raises(TypeError, lambda: b.filter_batch(torch.from_numpy(hay)))               # neither, host
raises(ValueError, lambda: b.filter_batch(t, offsets=torch.from_numpy(cuts)))  # offsets on another device
raises(ValueError, lambda: b.filter_batch(torch.from_numpy(hay), offsets=d_cuts))
raises(ValueError, lambda: b.filter_batch(t, row_length=L - 1))
raises(ValueError, lambda: b.filter_batch(t, offsets=d_cuts[:-2]))             # a wrong last entry: refused before any kernel runs
raises(TypeError, lambda: b.filter_batch(t, offsets=d_cuts.to(torch.int32)))
raises(ValueError, lambda: b.filter_batch(t, row_length=L, keep="some"))
raises(ValueError, lambda: b.filter_batch(t, row_length=L, min_matches=0))
raises(TypeError, lambda: b.filter_batch(t, row_length=L, min_matches=True))

# nothing kept, everything kept, no rows: the parts still become tensors
z = torch.full((1 << 20,), 48, dtype=torch.uint8, device="cuda:0")
zr = [b"0" * 1024] * 1024
check(b.filter_batch(z, row_length=1 << 10, keep="matched"), zr, ([], np.zeros(1, np.int64), b""), "device")
parts = check(b.filter_batch(z, row_length=1 << 10), zr, (list(range(1024)), np.arange(1025, dtype=np.int64) * 1024, b"0" * (1 << 20)), "device")
assert parts[2].data_ptr() != z.data_ptr()  # (a copy, not the caller's memory)
fr = b.filter_batch(torch.zeros(0, dtype=torch.uint8, device="cuda:0"), row_length=7)
assert len(fr) == 0 and fr.nbytes == 0 and fr.source_rows == 0 and fr.tolist() == []
assert torch.equal(torch.from_dlpack(fr.offsets).cpu(), torch.zeros(1, dtype=torch.int64))
assert tuple(torch.from_dlpack(fr.rows).shape) == (0,) and tuple(torch.from_dlpack(fr.data).shape) == (0,)
fr = b.filter_batch([])
assert torch.equal(torch.from_dlpack(fr.offsets), torch.zeros(1, dtype=torch.int64)) and len(fr) == 0

# lifetime: the tensors keep the result alive after the FilteredRows object is gone
uniform = [hay[i * L:(i + 1) * L].tobytes() for i in range(nh)]
want = definition(uniform, counts_of(o, uniform, False), 1, "matched")
fr = b.filter_batch(t, row_length=L, keep="matched")
parts = [torch.from_dlpack(x) for x in (fr.rows, fr.offsets, fr.data)]
unused = fr.data.__dlpack__()
del fr, unused
gc.collect()
for k in range(6):  # (other results come and go where the parts would be if they had been given back)
    other = torch.from_numpy(gen.gen_textlike(L * nh, 40 + k, pats).copy()).to("cuda:0")
    keep = b.filter_batch(other, row_length=L, keep="matched")
    del keep
gc.collect()
torch.cuda.synchronize()
assert parts[0].tolist() == want[0] and torch.equal(parts[1].cpu(), torch.from_numpy(want[1]))
assert bytes(parts[2].cpu().numpy()) == want[2]
del parts
gc.collect()
assert torch.equal(t.cpu(), torch.from_numpy(hay))
print("OK")
"""


def test_tensors_in_and_torch_out():
    """filter_batch on tensors in HBM with offsets and with row_length, both classes, both keep modes; its errors;
    torch.from_dlpack of the three columns (uint8 data on the automaton's device) and the kept rows rebuilt from them; empty
    results; lifetime.  In a process of its own: torch has to be the first to load the HIP runtime."""
    pytest.importorskip("torch")
    p = subprocess.run([sys.executable, "-c", _TENSOR_SCRIPT, ROOT, os.path.join(ROOT, "tests")], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
