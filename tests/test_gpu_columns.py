"""Matches as columns on the device (acx_find_columns / acx_find_columns_device / acx_split_device; find_matches_as_columns
and its batch form): the split kernel at its seams and at every 8-byte alignment, parity with the oracle for every match
kind on host and device inputs, batches with empty haystacks and their row offsets, results without a match, finds that were
cut or took the dense path, the lifetime of exported columns, threads on one handle and a seeded random loop.  Expected
values come from the oracle (tests/oracle_lib.py), never from the library; the kernel's seams are read from its sources."""
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
kDLCPU, kDLROCM = 1, 10


def hip_constants(path: str, names):
    src = open(os.path.join(CSRC, path)).read()
    out = {}
    for n in names:
        m = re.search(r"\b%s\s*=\s*(\d+)\s*[,;]" % n, src)
        assert m, f"{n} is no longer a plain constant of {path}"
        out[n] = int(m.group(1))
    return out


_C = hip_constants("columns.hpp", ("COL_THREADS", "COL_TILE", "COL_MAX_GRID"))
THREADS, TILE, MAX_GRID = _C["COL_THREADS"], _C["COL_TILE"], _C["COL_MAX_GRID"]
PASS = TILE * MAX_GRID  # records the whole grid turns in one pass of its loop
# a wave, a workgroup's threads, a workgroup's pass (= one LDS tile), the grid's pass, two passes and a ragged tail
SEAMS = sorted({0, 1, 2, 63, 64, 65, THREADS - 1, THREADS, THREADS + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1,
                PASS - 1, PASS, PASS + 1, 2 * PASS + TILE // 2 + 77})
GUARD = 0x5A5AA5A55A5AA5A5


def test_constants_are_what_the_sizes_below_assume():
    assert THREADS % 64 == 0 and TILE % THREADS == 0 and (3 * TILE) % 2 == 0
    assert SEAMS[-1] > 2 * PASS and SEAMS[-1] % TILE % THREADS != 0  # (two turns of the loop, then a ragged tile)
    assert SEAMS[-1] * 24 <= 256 << 20, "the largest case no longer is a few seconds' worth of copies"


def cols_of(rows):
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 3)
    return [np.ascontiguousarray(rows[:, k]).view(np.int64) for k in range(3)]


def download_words(ptr: int, n: int) -> np.ndarray:
    out = np.empty(n, dtype=np.int64)
    if n:
        capi._check(capi.lib().acx_device_download(out.ctypes.data, ptr, 8 * n))
    return out


# ---------------------------------------------------------------------------
# the split kernel at its seams
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def records():
    """SEAMS[-1] + 1 records in HBM, record i = (3 i, 3 i + 1 + 2^40, 3 i + 2 + 2^41): every word of the stream is distinct,
    a lane or a field that is mixed up shows.  (host image, device buffer)"""
    n = SEAMS[-1] + 1
    w = np.arange(3 * n, dtype=np.uint64).reshape(n, 3)
    w[:, 1] += np.uint64(1 << 40)
    w[:, 2] += np.uint64(1 << 41)
    buf = capi.DeviceBuffer(24 * n).upload(w)
    assert buf.ptr % 16 == 0
    yield w, buf
    buf.free()


@pytest.mark.parametrize("first_record", [0, 1])  # (record 1 begins 24 bytes in: at 8 mod 16)
@pytest.mark.parametrize("first_word", [0, 1])    # (columns at 0 or 8 mod 16)
def test_split_device_seams(records, first_record, first_word):
    w, rec = records
    big = capi.DeviceBuffer(8 * (3 * (SEAMS[-1] + 2) + 4))
    for n in SEAMS:
        # [guards][column][two guards][column][two guards][column][guards]: an even step keeps every column's residue
        step = n + 2
        image = np.full(first_word + 2 + 3 * step, GUARD, dtype=np.uint64)
        big.upload(image)
        at = [first_word + 2 + k * step for k in range(3)]
        capi.split_device(rec.ptr + 24 * first_record, n, *[big.ptr + 8 * a for a in at])
        assert (rec.ptr + 24 * first_record) % 16 == 8 * first_record and (big.ptr + 8 * at[0]) % 16 == 8 * first_word
        got = download_words(big.ptr, len(image)).view(np.uint64)
        for k in range(3):
            image[at[k]:at[k] + n] = w[first_record:first_record + n, k]
        bad = np.flatnonzero(got != image)
        assert len(bad) == 0, (n, first_record, first_word, "first wrong word", int(bad[0]), "columns begin at", at)
    big.free()


# ---------------------------------------------------------------------------
# parity with the oracle
# ---------------------------------------------------------------------------
PATS = gen.gen_patterns(500, 3, 9, gen.AZ, 5) + [b"ab", b"abab", b"bab", b"ab"]  # (a copy: overlapping reports it)
KINDS = [(0, False), (0, True), (1, False), (2, False)]


def matchkind(ar, mk):
    return (ar.MatchKind.Standard, ar.MatchKind.LeftmostFirst, ar.MatchKind.LeftmostLongest)[mk]


def check_host_columns(c, rows, batch_counts=None):
    """a MatchColumns in host memory against the oracle's rows"""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 3)
    assert c.device is None and len(c) == len(rows)
    for col, want in zip((c.pattern, c.start, c.end), cols_of(rows)):
        assert len(col) == len(rows) and col.__dlpack_device__() == (kDLCPU, 0)
        got = np.from_dlpack(col)
        assert got.dtype == np.int64 and got.shape == (len(rows),) and np.array_equal(got, want)
        mv = memoryview(col)
        assert mv.format == "q" and mv.readonly and mv.shape == (len(rows),) and np.array_equal(np.asarray(mv), want)
    if batch_counts is None:
        assert c.row_offsets is None
    else:
        ro = np.from_dlpack(c.row_offsets)
        assert len(c.row_offsets) == len(batch_counts) + 1
        assert np.array_equal(ro, np.concatenate([[0], np.cumsum(batch_counts)]).astype(np.int64))


def check_device_columns(c, rows, batch_counts=None):
    """a capi.DeviceColumns in HBM against the oracle's rows, through the copies and through the raw addresses"""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 3)
    assert c.on_device and c.count == len(rows)
    for k, want in enumerate(cols_of(rows)):
        assert np.array_equal(c.column(k), want), k
        p = c.data_ptr(k)
        assert p and p % 8 == 0 and np.array_equal(download_words(p, len(rows)), want), k
    if batch_counts is None:
        assert c.row_offsets() is None and c.data_ptr(capi.COL_ROW_OFFSETS) == 0 and c.rows == 0
    else:
        want = np.concatenate([[0], np.cumsum(batch_counts)]).astype(np.int64)
        assert c.rows == len(batch_counts) and np.array_equal(c.row_offsets(), want)
        assert np.array_equal(download_words(c.data_ptr(capi.COL_ROW_OFFSETS), len(want)), want)
    c.free()


@pytest.mark.parametrize("mk,ov", KINDS)
def test_parity_bytes_and_device(mk, ov):
    import ahocorasick_rs as ar
    o = Oracle(PATS, mk, KIND_DFA)
    b = ar.BytesAhoCorasick(PATS, matchkind=matchkind(ar, mk))
    a = capi.Automaton(PATS, mk)
    for n in (0, 5, 3000, 70_000, (1 << 20) + 4321):  # (K0's sizes, the in-place read, the staged pipeline)
        hay = gen.gen_textlike(n, 9 + n, PATS).tobytes()
        rows = o.find_raw(hay, overlapping=ov)
        c = b.find_matches_as_columns(hay, overlapping=ov)
        assert c.tolist() == o.find(hay, overlapping=ov) == b.find_matches_as_indexes(hay, overlapping=ov)
        check_host_columns(c, rows)
        check_host_columns(b.find_matches_as_columns(bytearray(hay), ov), rows)
        for off in (0, 3):  # (the device haystack at an even and at an odd address)
            dev = capi.DeviceBuffer(n + 16).upload(np.frombuffer(b"\xa5" * off + hay, dtype=np.uint8))
            check_device_columns(a.find_columns_device(dev.ptr + off, n, overlapping=ov), rows)
            dev.free()
    a.close()


@pytest.mark.parametrize("mk,ov", KINDS)
def test_parity_str_code_points(mk, ov):
    import ahocorasick_rs as ar
    pats = ["é☃", "ab", "b🤦", "☃", "ab"]
    o = Oracle([p.encode() for p in pats], mk, KIND_DFA)
    s = ar.AhoCorasick(pats, matchkind=matchkind(ar, mk))
    for hay in ("", "ab☃é☃b🤦", "xxé☃" * 50, "🤦🤦ab", "ascii only ab ab", "é" * 3000 + "☃ab" * 40000):
        want = o.find_str(hay, overlapping=ov)
        c = s.find_matches_as_columns(hay, overlapping=ov)
        assert c.tolist() == want == s.find_matches_as_indexes(hay, overlapping=ov)
        check_host_columns(c, want)


def test_case_insensitive_handle():
    import ahocorasick_rs as ar
    pats = [b"Needle", b"hay", b"STACK"]
    o = Oracle([p.translate(FOLD) for p in pats], 1, KIND_DFA)
    hay = (b"a nEEdle in a HayStack, a NEEDLE in a haySTACK; " * 3000)
    rows = o.find_raw(hay.translate(FOLD))
    b = ar.BytesAhoCorasick(pats, matchkind=ar.MatchKind.LeftmostFirst, ascii_case_insensitive=True)
    check_host_columns(b.find_matches_as_columns(hay), rows)
    a = capi.Automaton(pats, 1, ascii_case_insensitive=True)
    dev = capi.DeviceBuffer(len(hay) + 16).upload(np.frombuffer(b"\xa5" * 5 + hay, dtype=np.uint8))
    check_device_columns(a.find_columns_device(dev.ptr + 5, len(hay)), rows)
    assert np.array_equal(dev.download(len(hay) + 5)[5:], np.frombuffer(hay, dtype=np.uint8))  # (the caller's bytes are not folded)
    dev.free()
    a.close()


def test_the_errors_are_the_finds():
    import ahocorasick_rs as ar
    for mk in (ar.MatchKind.LeftmostFirst, ar.MatchKind.LeftmostLongest):
        b, s = ar.BytesAhoCorasick([b"ab"], matchkind=mk), ar.AhoCorasick(["ab"], matchkind=mk)
        for call in (lambda: b.find_matches_as_columns(b"ab", overlapping=True), lambda: b.find_matches_as_columns_batch([b"ab"], True),
                     lambda: s.find_matches_as_columns("ab", overlapping=True), lambda: s.find_matches_as_columns_batch(["ab"], True)):
            with pytest.raises(ValueError):
                call()
    b, s = ar.BytesAhoCorasick([b"ab"]), ar.AhoCorasick(["ab"])
    for obj, m, arg in ((s, "find_matches_as_columns", b"ab"), (s, "find_matches_as_columns_batch", [b"ab"]),
                        (b, "find_matches_as_columns", "ab"), (b, "find_matches_as_columns_batch", ["ab"]),
                        (b, "find_matches_as_columns", 5), (s, "find_matches_as_columns_batch", 5)):
        ref = m.replace("columns", "indexes")
        with pytest.raises(TypeError) as want:
            getattr(obj, ref)(arg)
        with pytest.raises(TypeError) as got:
            getattr(obj, m)(arg)
        assert str(got.value) == str(want.value), (m, arg)
    with pytest.raises(TypeError):
        b.find_matches_as_columns(b"ab", overlapping=1)
    a = capi.Automaton([b"ab", b"b"], 1)
    dev = capi.DeviceBuffer(64).upload(np.frombuffer(b"xxabxx", dtype=np.uint8))
    with pytest.raises(ValueError) as ei:
        a.find_columns_device(dev.ptr, 6, overlapping=True)
    assert ei.value.code == capi.EOVERLAP
    dev.free()
    a.close()


# ---------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------
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


def device_batch(a, hays, off, **kw):
    """the batch behind one another in HBM at `off` modulo 16, ragged offsets on the device -> DeviceColumns"""
    blob = b"".join(hays)
    offs = np.concatenate([[0], np.cumsum([len(h) for h in hays])]).astype(np.uint64)
    d_hay = capi.DeviceBuffer(len(blob) + 32).upload(np.frombuffer(b"\xa5" * off + blob, dtype=np.uint8))
    d_off = capi.DeviceBuffer(8 * len(offs)).upload(offs)
    c = a.find_columns_device(d_hay.ptr + off, len(blob), d_offsets=d_off.ptr, n_hay=len(hays), **kw)
    c.count  # (known at return)
    return c, (d_hay, d_off)


@pytest.mark.parametrize("mk,ov", KINDS)
def test_batches_host_and_device(mk, ov):
    import ahocorasick_rs as ar
    o = Oracle(PATS, mk, KIND_DFA)
    b = ar.BytesAhoCorasick(PATS, matchkind=matchkind(ar, mk))
    a = capi.Automaton(PATS, mk)
    for n_hay in (1, 63, 64, 65, 323):
        hays = batch_with_empties(PATS, n_hay, 100 + n_hay)
        per = [o.find_raw(h, overlapping=ov) for h in hays]
        rows, counts = np.concatenate(per), [len(r) for r in per]
        c = b.find_matches_as_columns_batch(hays, overlapping=ov)
        assert c.tolist() == [o.find(h, overlapping=ov) for h in hays]
        check_host_columns(c, rows, counts)
        ro, cs = np.from_dlpack(c.row_offsets), [np.from_dlpack(x) for x in (c.pattern, c.start, c.end)]
        for h in range(n_hay):  # every row's slice is that haystack's matches, offsets local to it
            got = np.stack([x[ro[h]:ro[h + 1]] for x in cs], 1).view(np.uint64)
            assert np.array_equal(got, per[h]), h
        check_host_columns(b.find_matches_as_columns_batch(tuple(hays), ov), rows, counts)
        dc, keep = device_batch(a, hays, 5 if n_hay % 2 else 0, overlapping=ov)
        check_device_columns(dc, rows, counts)
        for k in keep:
            k.free()
    # a uniform batch on the device
    L, nh = 512, 130
    full = gen.gen_textlike(L * nh, 61, PATS).tobytes()
    per = [o.find_raw(full[i * L:(i + 1) * L], overlapping=ov) for i in range(nh)]
    dev = capi.DeviceBuffer(len(full)).upload(np.frombuffer(full, dtype=np.uint8))
    check_device_columns(a.find_columns_device(dev.ptr, len(full), n_hay=nh, uniform_len=L, overlapping=ov),
                         np.concatenate(per), [len(r) for r in per])
    dev.free()
    a.close()


def test_results_freed_unread_and_in_reverse_order():
    """the seams of the result's owner: a result freed with no accessor ever called (the free waits for the stage) and the
    identical call after it, whose blocks come from the cache; eight results alive at once, four freed unread in the opposite
    order to their creation, a result made where their blocks went, and the other four read afterwards"""
    pats = [b"ab", b"abab", b"bab", b"needle", b"hay", b"stack", b"a", b"zz", b"0123", b"ab"]
    o, a = Oracle(pats, 0, KIND_DFA), capi.Automaton(pats, 0)
    batches = [[gen.gen_textlike([0, 7, 64, 255][(i + k) % 4], 50 + 8 * k + i, pats).tobytes() for i in range(5 + 7 * k)] for k in range(8)]
    per = [[o.find_raw(h, overlapping=True) for h in hays] for hays in batches]
    want = [(np.concatenate(p), [len(r) for r in p]) for p in per]
    c, keep = device_batch(a, batches[3], 0, overlapping=True)
    c.free()
    c, keep2 = device_batch(a, batches[3], 0, overlapping=True)
    check_device_columns(c, *want[3])
    made = [device_batch(a, hays, 0, overlapping=True) for hays in batches]
    for k in (7, 6, 5, 4):
        made[k][0].free()
    c, keep3 = device_batch(a, batches[6], 0, overlapping=True)
    check_device_columns(c, *want[6])
    for k in (3, 2, 1, 0):
        check_device_columns(made[k][0], *want[k])
    for d in [*keep, *keep2, *keep3] + [d for _, ks in made for d in ks]:
        d.free()
    a.close()


def test_empty_batches_and_no_match_at_all():
    import ahocorasick_rs as ar
    b, s = ar.BytesAhoCorasick(PATS), ar.AhoCorasick(["ab", "é"])
    a = capi.Automaton(PATS, 0)
    none = np.zeros((0, 3), np.uint64)
    # an empty batch, a batch of empty haystacks, a batch without a match
    for obj, hays in ((b, []), (b, [b"", b"", b""]), (b, [b"0123", b"", b"4567" * 500]), (s, []), (s, ["", ""]), (s, ["xyz", "ü"])):
        c = obj.find_matches_as_columns_batch(hays)
        assert len(c) == 0 and c.tolist() == [[] for _ in hays]
        check_host_columns(c, none, [0] * len(hays))
    for hays in ([], [b"", b""], [b"0123", b"", b"4567" * 500]):
        dc, keep = device_batch(a, hays, 0)
        check_device_columns(dc, none, [0] * len(hays))
        for k in keep:
            k.free()
    # one haystack without a match: host, and device (empty and not)
    for obj, hay in ((b, b""), (b, b"0123" * 5000), (s, ""), (s, "nothing to see")):
        c = obj.find_matches_as_columns(hay)
        assert len(c) == 0 and c.tolist() == []
        check_host_columns(c, none)
    dev = capi.DeviceBuffer(1 << 20).upload(np.frombuffer(b"0123" * (1 << 18), dtype=np.uint8))
    for n in (0, 1, 1 << 20):
        dc = a.find_columns_device(dev.ptr, n)
        assert all(dc.data_ptr(k) for k in range(3))  # (an empty column still has an address)
        check_device_columns(dc, none)
    dev.free()
    a.close()


# ---------------------------------------------------------------------------
# a find beneath that was cut into byte ranges, and one on the dense path
# ---------------------------------------------------------------------------
def test_cut_find_and_dense_path(monkeypatch):
    pats = gen.gen_patterns(2000, 5, 12, gen.AZ, 1)
    a, o = capi.Automaton(pats, 0, capi.IMPL_DFA), Oracle(pats, 0, KIND_DFA)
    hay = gen.gen_textlike((3 << 20) + 4321, 71, pats).tobytes()
    rows = o.find_raw(hay)
    dev = capi.DeviceBuffer(len(hay) + 16).upload(np.frombuffer(b"\xa5" * 8 + hay, dtype=np.uint8))
    monkeypatch.setenv("ACX_CHUNK_BYTES", "700001")
    a.path_stats(reset=True)
    dc = a.find_columns_device(dev.ptr + 8, len(hay))
    st = a.path_stats()
    monkeypatch.delenv("ACX_CHUNK_BYTES")
    assert st["byte_ranges"] == 5, st
    check_device_columns(dc, rows)
    dev.free()
    # a pattern every 32 bytes: the dense path (or the hot pipeline) on the second call at the latest
    every = bytearray(gen.gen_uniform(8 << 20, gen.AZ, 13).tobytes())  # (the size tests/test_gpu_replace_seams.py uses)
    rng = gen.SplitMix64(77)
    for k in range(0, len(every) - 32, 32):
        p = pats[rng.next() % len(pats)]
        every[k:k + len(p)] = p
    every = bytes(every)
    rows = o.find_raw(every)
    assert len(rows) >= len(every) // 32
    dev = capi.DeviceBuffer(len(every)).upload(np.frombuffer(every, dtype=np.uint8))
    a.path_stats(reset=True)
    for _ in range(2):
        check_device_columns(a.find_columns_device(dev.ptr, len(every)), rows)
    st = a.path_stats()
    assert st["hot_calls"] + st["dense_tiles"] + st["dense_radix"] >= 2, st
    dev.free()
    a.close()


# ---------------------------------------------------------------------------
# lifetime (host columns here; device columns with torch below), threads
# ---------------------------------------------------------------------------
def test_exported_host_columns_outlive_the_result():
    import ahocorasick_rs as ar
    o, b = Oracle(PATS, 0, KIND_DFA), ar.BytesAhoCorasick(PATS)
    hay = gen.gen_textlike(200_000, 3, PATS).tobytes()
    want = cols_of(o.find_raw(hay))
    c = b.find_matches_as_columns(hay)
    arrays = [np.from_dlpack(x) for x in (c.pattern, c.start, c.end)]
    views = [memoryview(x) for x in (c.pattern, c.start, c.end)]
    unused = c.pattern.__dlpack__()  # (a capsule nobody consumes gives its reference back too)
    del c, unused
    gc.collect()
    for k in range(20):  # (other results come and go where the columns' memory would be if it had been freed)
        b.find_matches_as_columns(gen.gen_textlike(200_000, 50 + k, PATS).tobytes())
    for got, mv, w in zip(arrays, views, want):
        assert np.array_equal(got, w) and np.array_equal(np.asarray(mv), w)


def test_eight_threads_on_one_handle():
    import ahocorasick_rs as ar
    b = ar.BytesAhoCorasick(PATS)
    a = capi.Automaton(PATS, 0)
    o = Oracle(PATS, 0, KIND_DFA)
    work = []
    for t in range(8):
        hay = gen.gen_textlike(50_000 + 30_000 * t, 200 + t, PATS).tobytes()
        hays = batch_with_empties(PATS, 20 + t, 300 + t)
        per = [o.find_raw(h) for h in hays]
        work.append((hay, o.find_raw(hay), hays, np.concatenate(per), [len(r) for r in per]))
    errors = []

    def run(t):
        try:
            hay, rows, hays, brows, counts = work[t]
            dev = capi.DeviceBuffer(len(hay)).upload(np.frombuffer(hay, dtype=np.uint8))
            for _ in range(4):
                check_host_columns(b.find_matches_as_columns(hay), rows)
                check_host_columns(b.find_matches_as_columns_batch(hays), brows, counts)
                check_device_columns(a.find_columns_device(dev.ptr, len(hay)), rows)
            dev.free()
        except BaseException as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=run, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    a.close()


# ---------------------------------------------------------------------------
# a seeded random loop: pattern sets, match kinds, single or batch, host or device
# ---------------------------------------------------------------------------
def test_seeded_random_cases():
    import ahocorasick_rs as ar
    rng = random.Random(20261017)
    for case in range(48):
        mk = rng.choice([0, 0, 1, 2])
        ov = mk == 0 and rng.random() < 0.4
        alpha = rng.choice([b"ab", b"abcd", gen.AZ])
        pats = gen.gen_patterns(rng.choice([1, 3, 40, 600]), 1, rng.choice([2, 6, 12]), alpha, 1000 + case)
        text = rng.choice([alpha, alpha + b"xyz", b"0123"])
        o = Oracle(pats, mk, KIND_DFA)
        batch, device = rng.random() < 0.5, rng.random() < 0.5
        n_hay = rng.choice([1, 2, 7, 64, 65, 130]) if batch else 1
        hays = [bytes(rng.choices(text, k=rng.choice([0, 1, 9, 200, 5000]))) for _ in range(n_hay)]
        per = [o.find_raw(h, overlapping=ov) for h in hays]
        rows, counts = np.concatenate(per), [len(r) for r in per]
        what = (case, mk, ov, batch, device, n_hay)
        try:
            if device:
                a = capi.Automaton(pats, mk)
                if batch:
                    dc, keep = device_batch(a, hays, rng.randrange(16), overlapping=ov)
                    check_device_columns(dc, rows, counts)
                else:
                    off = rng.randrange(16)
                    keep = [capi.DeviceBuffer(len(hays[0]) + 32).upload(np.frombuffer(b"\xa5" * off + hays[0], dtype=np.uint8))]
                    check_device_columns(a.find_columns_device(keep[0].ptr + off, len(hays[0]), overlapping=ov), rows)
                for k in keep:
                    k.free()
                a.close()
            else:
                b = ar.BytesAhoCorasick(pats, matchkind=matchkind(ar, mk))
                if batch:
                    c = b.find_matches_as_columns_batch(hays, overlapping=ov)
                    check_host_columns(c, rows, counts)
                    assert c.tolist() == [[tuple(int(v) for v in r) for r in p] for p in per]
                else:
                    c = b.find_matches_as_columns(hays[0], overlapping=ov)
                    check_host_columns(c, rows)
                    assert c.tolist() == [tuple(int(v) for v in r) for r in rows]
        except AssertionError as e:
            raise AssertionError(f"case {what}: {e}") from e


# ---------------------------------------------------------------------------
# tensors in HBM through the Python methods, and torch as the consumer of the columns
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
pats = gen.gen_patterns(3000, 5, 12, gen.AZ, 1) + [b"ab", b"ab"]
hay = gen.gen_textlike(3 << 20, 13, pats)
t = torch.from_numpy(hay.copy()).to("cuda:0")
kinds = (ar.MatchKind.Standard, ar.MatchKind.LeftmostFirst, ar.MatchKind.LeftmostLongest)

def tensors(c):
    return [torch.from_dlpack(x) for x in (c.pattern, c.start, c.end)]

def same(ts, rows, where):
    rows = torch.from_numpy(np.ascontiguousarray(rows).view(np.int64).reshape(-1, 3))
    for k, x in enumerate(ts):
        assert x.dtype == torch.int64 and tuple(x.shape) == (len(rows),) and x.is_contiguous(), (where, k)
        assert x.device.type == ("cuda" if where == "device" else "cpu"), (where, k, x.device)
        assert torch.equal(x.cpu(), rows[:, k]), (where, k)

for mk, ov in ((0, False), (0, True), (1, False), (2, False)):
    o = Oracle(pats, mk, KIND_DFA)
    b = ar.BytesAhoCorasick(pats, matchkind=kinds[mk])
    rows = o.find_raw(hay, overlapping=ov)
    c = b.find_matches_as_columns(t, overlapping=ov)            # a tensor in HBM: the columns stay there
    assert c.device == 0 and len(c) == len(rows) and c.row_offsets is None
    for x in (c.pattern, c.start, c.end):
        assert x.__dlpack_device__() == (10, 0) and len(x) == len(rows)
        try:
            memoryview(x)
            raise SystemExit("a device column exported a host buffer")
        except BufferError:
            pass
    same(tensors(c), rows, "device")
    assert c.tolist() == o.find(hay.tobytes(), overlapping=ov) == b.find_matches_as_indexes(t, overlapping=ov)
    c = b.find_matches_as_columns(hay.tobytes(), overlapping=ov)  # host bytes: host columns, torch takes them as they are
    assert c.device is None
    same(tensors(c), rows, "host")
    c = b.find_matches_as_columns(torch.from_numpy(hay), overlapping=ov)  # host memory behind DLPack
    assert c.device is None
    same(tensors(c), rows, "host")

# an odd device address; the consumer on a stream of its own
o, b = Oracle(pats, 0, KIND_DFA), ar.BytesAhoCorasick(pats)
side = torch.cuda.Stream()
with torch.cuda.stream(side):
    ts = tensors(b.find_matches_as_columns(t[12345:]))
    total = ts[2].sum()
rows = o.find_raw(hay[12345:])
same(ts, rows, "device")
assert int(total) == int(rows[:, 2].astype(np.int64).sum())

# no match: every column has length 0 and still becomes a tensor and an array; a batch's row offsets as well
for arg in (torch.zeros(0, dtype=torch.uint8, device="cuda:0"), torch.full((1 << 20,), 48, dtype=torch.uint8, device="cuda:0"), b"", b"0000"):
    c = b.find_matches_as_columns(arg)
    assert len(c) == 0 and c.tolist() == [] and c.device == (0 if isinstance(arg, torch.Tensor) else None)
    for x in tensors(c):
        assert tuple(x.shape) == (0,) and x.dtype == torch.int64
    if c.device is None:
        assert all(np.from_dlpack(x).shape == (0,) for x in (c.pattern, c.start, c.end))
c = b.find_matches_as_columns_batch([b"", b"0000"])
assert torch.equal(torch.from_dlpack(c.row_offsets), torch.zeros(3, dtype=torch.int64))
c = b.find_matches_as_columns_batch([])
assert torch.equal(torch.from_dlpack(c.row_offsets), torch.zeros(1, dtype=torch.int64))

# lifetime: the tensors keep the result alive after the MatchColumns object is gone
rows = o.find_raw(hay)
c = b.find_matches_as_columns(t)
ts = tensors(c)
unused = c.end.__dlpack__()
del c, unused
gc.collect()
for k in range(6):  # (other results come and go where the columns would be if they had been given back)
    other = torch.from_numpy(gen.gen_textlike(3 << 20, 40 + k, pats).copy()).to("cuda:0")
    keep = tensors(b.find_matches_as_columns(other))
    del keep
gc.collect()
torch.cuda.synchronize()
same(ts, rows, "device")
del ts
gc.collect()
assert torch.equal(t.cpu(), torch.from_numpy(hay))
print("OK")
"""


def test_tensors_in_and_torch_out():
    """find_matches_as_columns on a tensor in HBM, torch.from_dlpack of host and device columns, empty columns, lifetime.  In
    a process of its own: torch has to be the first to load the HIP runtime."""
    pytest.importorskip("torch")
    p = subprocess.run([sys.executable, "-c", _TENSOR_SCRIPT, ROOT, os.path.join(ROOT, "tests")], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout + p.stderr
