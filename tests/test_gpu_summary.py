"""The summaries on the device (acx_summarize / acx_summarize_device; is_match, find_first, count_matches, count_by_pattern and
their batch forms): both routes on the same inputs, every match kind, overlapping counts, code points, case-insensitive
handles, batches with empty haystacks, the device forms at odd and even pointer residues, both histogram forms, every path a
find can take in front of the reduction, one run at 1 GiB, threads on one handle, and a slice of tools/gpu_fuzz.py's summary
mode.  Expected values: the oracle's matches reduced in Python (at 1 GiB: the library's own records, which
tests/test_gpu_batch.py::test_baseline_size_1gib_bit_exact pins to the oracle)."""
import os
import sys
import threading

import numpy as np
import pytest

import gen
from oracle_lib import KIND_DFA, Oracle

pytestmark = pytest.mark.gpu
capi = pytest.importorskip("ahocorasick_rs_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOLD = bytes.maketrans(bytes(range(65, 91)), bytes(range(97, 123)))
LDS_BINS = 8192  # csrc/summary.hpp: SUMMARY_LDS_BINS


def reduce_rows(per_haystack, n_patterns):
    """per_haystack: one (n, 3) array of the oracle per haystack -> total, counts, any, first, by_pattern"""
    rows = np.concatenate([r.reshape(-1, 3) for r in per_haystack]) if per_haystack else np.zeros((0, 3), np.uint64)
    return {"total": len(rows), "counts": [len(r) for r in per_haystack], "any": [len(r) > 0 for r in per_haystack],
            "first": [tuple(int(v) for v in r[0]) if len(r) else None for r in per_haystack],
            "hist": np.bincount(rows[:, 0].astype(np.int64), minlength=n_patterns).astype(np.uint64)}


def check(s, want, on_device, what=3):
    assert s.on_device == on_device
    assert s.total == want["total"]
    assert [int(v) for v in s.counts()] == want["counts"]
    if what & 1:
        assert [bool(v) for v in s.any()] == want["any"]
        got = [None if int(r["pattern"]) == capi.NO_MATCH else (int(r["pattern"]), int(r["start"]), int(r["end"])) for r in s.first()]
        assert got == want["first"]
    else:
        for part in (s.any, s.first):
            with pytest.raises(ValueError):
                part()
    if what & 2:
        assert np.array_equal(s.by_pattern(), want["hist"])
    else:
        with pytest.raises(ValueError):
            s.by_pattern()
    s.free()


def batch_with_empties(pats, n_hay, seed):
    """n_hay haystacks of 0 .. 3000 bytes: empty ones in front, in the middle (two in a row) and at the end, some without a match"""
    rng = gen.SplitMix64(seed)
    hays = []
    for i in range(n_hay):
        n = [0, 17, 300, 3000, 64][rng.next() % 5]
        h = gen.gen_textlike(n, seed + i, pats).tobytes() if i % 3 else gen.gen_uniform(n, b"0123", seed + i).tobytes()
        hays.append(h)
    for i in (0, 1, n_hay // 2, n_hay // 2 + 1, n_hay - 1):
        hays[i] = b""
    return hays


@pytest.mark.parametrize("mk", [0, 1, 2])
def test_both_routes_on_the_same_inputs(monkeypatch, mk):
    pats = gen.gen_patterns(500, 3, 9, gen.AZ, 5) + [b"ab", b"abab", b"bab"]
    a = capi.Automaton(pats, mk)
    o = Oracle(pats, mk, KIND_DFA)
    # 64 * 4 + 64 + 3 haystacks: across the 64-lane boundary and across a workgroup boundary (256) of the gather
    for n_hay in (1, 63, 64, 65, 323):
        hays = batch_with_empties(pats, n_hay, 100 + n_hay) if n_hay > 4 else [gen.gen_textlike(5000, 9, pats).tobytes()]
        for ov in ([False, True] if mk == 0 else [False]):
            want = reduce_rows([o.find_raw(h, overlapping=ov) for h in hays], len(pats))
            for route, limit in (("host", str(1 << 40)), ("device", "0")):
                monkeypatch.setenv("ACX_SUMMARY_HOST_MAX", limit)
                for what in (3, 0, 1, 2):
                    check(a.summarize_batch(hays, what, overlapping=ov), want, route == "device", what)
            single = hays[len(hays) // 3]
            one = reduce_rows([o.find_raw(single, overlapping=ov)], len(pats))
            for route, limit in (("host", str(1 << 40)), ("device", "0")):
                monkeypatch.setenv("ACX_SUMMARY_HOST_MAX", limit)
                check(a.summarize(single, overlapping=ov), one, route == "device" and len(single) > 0)
    # an empty batch and a batch of empty haystacks
    monkeypatch.setenv("ACX_SUMMARY_HOST_MAX", "0")
    check(a.summarize_batch([]), reduce_rows([], len(pats)), False)
    check(a.summarize_batch([b"", b""]), reduce_rows([np.zeros((0, 3), np.uint64)] * 2, len(pats)), False)
    a.close()


@pytest.mark.parametrize("mk", [1, 2])
def test_overlapping_on_a_leftmost_handle_is_the_finds_error(monkeypatch, mk):
    a = capi.Automaton([b"ab", b"b"], mk)
    buf = capi.DeviceBuffer(64).upload(np.frombuffer(b"xxabxx", dtype=np.uint8))
    for limit in ("0", str(1 << 40)):
        monkeypatch.setenv("ACX_SUMMARY_HOST_MAX", limit)
        for call in (lambda: a.summarize(b"xxabxx", overlapping=True), lambda: a.summarize_batch([b"ab", b"b"], overlapping=True),
                     lambda: a.summarize_device(buf.ptr, 6, overlapping=True)):
            with pytest.raises(ValueError) as ei:
                call()
            assert ei.value.code == capi.EOVERLAP
    buf.free()
    a.close()
    import ahocorasick_rs as ar
    b = ar.BytesAhoCorasick([b"ab"], matchkind=ar.MatchKind.LeftmostFirst if mk == 1 else ar.MatchKind.LeftmostLongest)
    for m, arg in (("count_matches", b"ab"), ("count_by_pattern", b"ab"), ("count_matches_batch", [b"ab"]), ("count_by_pattern_batch", [b"ab"])):
        with pytest.raises(ValueError):
            getattr(b, m)(arg, overlapping=True)
        with pytest.raises(ValueError):
            b.find_matches_as_indexes(b"ab", overlapping=True)


@pytest.mark.parametrize("route", ["host", "device"])
def test_python_methods_str_code_points_and_case_insensitive(monkeypatch, route):
    import ahocorasick_rs as ar
    monkeypatch.setenv("ACX_SUMMARY_HOST_MAX", "0" if route == "device" else str(1 << 40))
    pats = ["é☃", "ab", "b🤦", "☃", "ab"]  # (a copy: the overlapping counts hold it)
    hays = ["", "ab☃é☃b🤦", "xxé☃" * 50, "🤦🤦ab", "ascii only ab ab", "nothing", "é" * 3000 + "☃", ""]
    kinds = (ar.MatchKind.Standard, ar.MatchKind.LeftmostFirst, ar.MatchKind.LeftmostLongest)
    for mk in (0, 1, 2):
        a = ar.AhoCorasick(pats, matchkind=kinds[mk])
        b = ar.BytesAhoCorasick([p.encode() for p in pats], matchkind=kinds[mk])
        o = Oracle([p.encode() for p in pats], mk, KIND_DFA)
        for ov in ([False, True] if mk == 0 else [False]):
            per = [o.find_str(h, overlapping=ov) for h in hays]
            per_b = [o.find(h.encode(), overlapping=ov) for h in hays]
            hist = [sum(m[0] == p for ms in per for m in ms) for p in range(len(pats))]
            assert a.count_matches_batch(hays, overlapping=ov) == [len(ms) for ms in per]
            assert b.count_matches_batch([h.encode() for h in hays], overlapping=ov) == [len(ms) for ms in per]
            assert a.count_by_pattern_batch(hays, overlapping=ov) == hist
            assert b.count_by_pattern_batch([h.encode() for h in hays], overlapping=ov) == hist
            for h, ms, mb in zip(hays, per, per_b):
                assert a.count_matches(h, overlapping=ov) == len(ms) == b.count_matches(h.encode(), overlapping=ov)
                want = [sum(m[0] == p for m in ms) for p in range(len(pats))]
                assert a.count_by_pattern(h, overlapping=ov) == want == b.count_by_pattern(h.encode(), overlapping=ov)
        per = [o.find_str(h) for h in hays]
        per_b = [o.find(h.encode()) for h in hays]
        assert a.is_match_batch(hays) == [bool(ms) for ms in per] == b.is_match_batch([h.encode() for h in hays])
        assert a.find_first_batch(hays) == [ms[0] if ms else None for ms in per]  # code points
        assert b.find_first_batch([h.encode() for h in hays]) == [ms[0] if ms else None for ms in per_b]  # bytes
        for h, ms, mb in zip(hays, per, per_b):
            assert a.is_match(h) is bool(ms) and b.is_match(h.encode()) is bool(ms)
            assert a.find_first(h) == (ms[0] if ms else None)
            assert b.find_first(h.encode()) == (mb[0] if mb else None)
        assert a.is_match_batch([]) == [] and a.find_first_batch([]) == [] and a.count_matches_batch([]) == []
        assert a.count_by_pattern_batch([]) == [0] * len(pats)
    # a case-insensitive handle keeps its meaning; offsets are the caller's
    cpats, chays = ["Straße", "ABC", "bcD"], ["", "xxabcd", "STRAßE strasse Straße", "ABCD" * 700, "nothing"]
    o = Oracle([p.encode().translate(FOLD) for p in cpats], 1, KIND_DFA)
    a = ar.AhoCorasick(cpats, matchkind=ar.MatchKind.LeftmostFirst, ascii_case_insensitive=True)
    per = [o.find_str(h.encode().translate(FOLD).decode()) for h in chays]
    assert a.is_match_batch(chays) == [bool(ms) for ms in per]
    assert a.find_first_batch(chays) == [ms[0] if ms else None for ms in per]
    assert a.count_matches_batch(chays) == [len(ms) for ms in per]
    assert a.count_by_pattern_batch(chays) == [sum(m[0] == p for ms in per for m in ms) for p in range(len(cpats))]
    assert [a.find_first(h) for h in chays] == [ms[0] if ms else None for ms in per]


@pytest.mark.parametrize("ci", [False, True])
@pytest.mark.parametrize("residue", [1, 8])
def test_device_forms_at_pointer_residues(residue, ci):
    pats = gen.gen_patterns(3000, 5, 12, gen.AZ, 1)
    o = Oracle(pats, 0, KIND_DFA)
    n_hay, L = 64 * 4 + 64 + 5, 1000
    hay = gen.gen_textlike(n_hay * L, 13, pats)
    hay[3 * L:5 * L] = ord("0")  # (haystacks without a match)
    host = hay.tobytes()
    if ci:
        upper = hay.copy()
        sel = (gen.stream_np(3, len(upper)) & np.uint64(1)) == 1
        upper[sel & (upper >= 97) & (upper <= 122)] -= 32
        hay = upper
    a = capi.Automaton(pats, 0, capi.IMPL_DFA, ascii_case_insensitive=ci)
    buf = capi.DeviceBuffer(n_hay * L + 64).upload(np.concatenate([np.zeros(residue, np.uint8), hay]))
    st0 = a.path_stats(reset=True)
    # uniform
    want = reduce_rows([o.find_raw(host[i * L:(i + 1) * L]) for i in range(n_hay)], len(pats))
    check(a.summarize_device(buf.ptr + residue, n_hay * L, n_hay=n_hay, uniform_len=L), want, True)
    # ragged, with empty haystacks in front, inside and at the end
    cuts = sorted([0, 0, 0, 777, 777, 777, 70_001, 200_000, 200_000, n_hay * L, n_hay * L] + list(range(1000, n_hay * L, 2113)))
    off = capi.DeviceBuffer(8 * len(cuts)).upload(np.array(cuts, dtype=np.uint64).view(np.uint8))
    want = reduce_rows([o.find_raw(host[cuts[i]:cuts[i + 1]]) for i in range(len(cuts) - 1)], len(pats))
    for ov in (False, True):
        w = want if not ov else reduce_rows([o.find_raw(host[cuts[i]:cuts[i + 1]], overlapping=True) for i in range(len(cuts) - 1)], len(pats))
        check(a.summarize_device(buf.ptr + residue, n_hay * L, n_hay=len(cuts) - 1, d_offsets=off.ptr, overlapping=ov), w, True)
    # one haystack
    check(a.summarize_device(buf.ptr + residue, n_hay * L), reduce_rows([o.find_raw(host)], len(pats)), True)
    # ... and an empty one; an empty uniform batch and an empty ragged one (n_hay == 0: no haystack, no word of the bitmap)
    check(a.summarize_device(buf.ptr + residue, 0), reduce_rows([np.zeros((0, 3), np.uint64)], len(pats)), True)
    check(a.summarize_device(buf.ptr + residue, 0, n_hay=0, uniform_len=L), reduce_rows([], len(pats)), True)
    check(a.summarize_device(buf.ptr + residue, 0, n_hay=0, d_offsets=off.ptr), reduce_rows([], len(pats)), True)
    st = a.path_stats()
    assert (st["folded_on_device"] >= 4) if ci else (st["folded_on_device"] == 0), st
    assert np.array_equal(buf.download(residue + n_hay * L)[residue:], hay)  # the caller's bytes are not written
    # the parts where they lie in HBM
    s = a.summarize_device(buf.ptr + residue, n_hay * L, n_hay=n_hay, uniform_len=L)
    for name in ("counts", "any", "first", "by_pattern"):
        assert s.device_ptr(name) != 0, name
    got = np.zeros(n_hay, dtype=np.uint64)
    capi._check(capi.lib().acx_device_download(got.ctypes.data, s.device_ptr("counts"), n_hay * 8))
    assert np.array_equal(got, s.counts())
    s.free()
    off.free(); buf.free(); a.close()


@pytest.mark.parametrize("n_pat", [3000, LDS_BINS, LDS_BINS + 1, 20000])
def test_both_histogram_forms(n_pat):
    # below, at and above the bound of the LDS form (n_patterns <= 8192), and well above it
    base = list(dict.fromkeys(gen.gen_patterns(n_pat, 4, 10, gen.AZ, 7)))
    pats = (base + gen.gen_patterns(n_pat, 11, 14, gen.AZ, 8))[:n_pat]
    assert len(pats) == n_pat
    hay = gen.gen_textlike(4 << 20, 11, pats)
    a = capi.Automaton(pats, 0)
    o = Oracle(pats, 0, KIND_DFA)
    buf = capi.DeviceBuffer(len(hay)).upload(hay)
    for ov in (False, True):
        want = reduce_rows([o.find_raw(hay, overlapping=ov)], n_pat)
        assert want["total"] > 3000 and np.count_nonzero(want["hist"]) > 1000
        check(a.summarize_device(buf.ptr, len(hay), capi.SUM_BY_PATTERN, overlapping=ov), want, True, 2)
    buf.free(); a.close()


@pytest.mark.parametrize("n_distinct", [1500, 6000])
def test_histogram_counts_every_copy_under_overlapping(n_distinct):
    # every string three times (the result of an overlapping search is expanded to the copies where it is complete):
    # 4 500 patterns for the LDS form, 18 000 for the global one
    base = list(dict.fromkeys(gen.gen_patterns(n_distinct, 4, 9, gen.AZ, 17)))
    pats = base + base[::-1] + base
    hay = gen.gen_textlike(2 << 20, 11, base)
    a = capi.Automaton(pats, 0)
    o = Oracle(pats, 0, KIND_DFA)
    buf = capi.DeviceBuffer(len(hay)).upload(hay)
    want_ov = reduce_rows([o.find_raw(hay, overlapping=True)], len(pats))
    want = reduce_rows([o.find_raw(hay)], len(pats))
    assert want_ov["total"] >= 3 * want["total"] > 0
    assert int(want["hist"][len(base):].sum()) == 0  # (a non-overlapping search reports the lowest id of a string)
    check(a.summarize_device(buf.ptr, len(hay), overlapping=True), want_ov, True)
    check(a.summarize_device(buf.ptr, len(hay)), want, True)
    # a uniform batch of it: the per-haystack counts follow the expansion
    L = 4096
    n_hay = len(hay) // L
    host = hay.tobytes()
    want_b = reduce_rows([o.find_raw(host[i * L:(i + 1) * L], overlapping=True) for i in range(n_hay)], len(pats))
    check(a.summarize_device(buf.ptr, n_hay * L, n_hay=n_hay, uniform_len=L, overlapping=True), want_b, True)
    buf.free(); a.close()


def plant(hay: np.ndarray, pats, lo: int, hi: int, every: int, seed: int) -> None:
    rng = gen.SplitMix64(seed)
    for k in range(lo, hi - 32, every):
        p = np.frombuffer(pats[rng.next() % len(pats)], dtype=np.uint8)
        hay[k:k + len(p)] = p


def test_the_paths_a_find_takes_in_front_of_the_reduction(monkeypatch):
    pats = gen.gen_patterns(10000, 5, 12, gen.AZ, 1)
    a = capi.Automaton(pats, 0, capi.IMPL_DFA)
    o = Oracle(pats, 0, KIND_DFA)
    # K0: a haystack under 16 KiB, host route
    small = gen.gen_textlike(12_000, 11, pats).tobytes()
    a.path_stats(reset=True)
    check(a.summarize(small), reduce_rows([o.find_raw(small)], len(pats)), False)
    st = a.path_stats()
    assert st["k0"] == 1 and st["sparse"] == st["hot_calls"] == st["dense_tiles"] == st["dense_radix"] == 0, st
    # ... and on the device route (K0 takes a small device haystack as well)
    monkeypatch.setenv("ACX_SUMMARY_HOST_MAX", "0")
    check(a.summarize(small), reduce_rows([o.find_raw(small)], len(pats)), True)
    # a sparse 64 MiB haystack, generated in HBM
    n = 64 << 20
    buf = capi.DeviceBuffer(n)
    a.generate(buf.ptr, n, 1, 11)
    host = buf.download()
    want = reduce_rows([o.find_raw(host)], len(pats))
    a.path_stats(reset=True)
    check(a.summarize_device(buf.ptr, n), want, True)
    st = a.path_stats()
    assert st["sparse"] == 1 and st["hot_calls"] == st["dense_tiles"] == st["dense_radix"] == st["byte_ranges"] == 0, st
    # the same from host memory: staged, device route
    a.path_stats(reset=True)
    check(a.summarize(host), want, True)
    st = a.path_stats()
    assert st["sparse"] == 1 and st["k0"] == st["in_place"] == 0, st
    buf.free()
    # a dense stretch: the hot pipeline takes its groups
    hot = gen.gen_textlike(4 << 20, 11, pats).copy()
    a0 = (len(hot) // 3) & ~(64 * 4096 - 1)
    plant(hot, pats, a0 + 8 * 4096, a0 + 8 * 4096 + (64 << 10), 32, 77)
    want = reduce_rows([o.find_raw(hot)], len(pats))
    a.path_stats(reset=True)
    check(a.summarize(hot), want, True)
    st = a.path_stats()
    assert st["hot_calls"] == 1 and st["dense_tiles"] == st["dense_radix"] == 0, st
    # the result spliced from byte ranges
    monkeypatch.setenv("ACX_CHUNK_BYTES", str(700_001))
    a.path_stats(reset=True)
    check(a.summarize(hot), want, True)
    st = a.path_stats()
    assert st["byte_ranges"] >= 2, st  # (4 MiB in pieces of 700 001 bytes)
    monkeypatch.delenv("ACX_CHUNK_BYTES")
    a.close()
    # dense everywhere: a pattern every 32 bytes (a fresh handle, as tests/test_gpu_hot.py takes one)
    a = capi.Automaton(pats, 0, capi.IMPL_DFA)
    dense = gen.gen_uniform(8 << 20, gen.AZ, 12).copy()
    plant(dense, pats, 0, len(dense), 32, 77)
    want = reduce_rows([o.find_raw(dense)], len(pats))
    a.path_stats(reset=True)
    check(a.summarize(dense), want, True)
    st = a.path_stats(reset=True)
    assert st["hot_calls"] == 1 and st["dense_tiles"] == st["dense_radix"] == 0, st
    check(a.summarize(dense), want, True)  # (the handle's next call: the dense path proper)
    st = a.path_stats()
    assert st["dense_tiles"] + st["dense_radix"] == 1 and st["hot_calls"] == 0, st
    a.close()


def test_one_run_at_1gib():
    """cfg2 at full size: the device summary equals the numpy reduction of acx_find_device's own records (which
    tests/test_gpu_batch.py::test_baseline_size_1gib_bit_exact pins to the oracle)"""
    pats = gen.gen_patterns(10000, 5, 12, gen.AZ, 1)
    n = 1 << 30
    a = capi.Automaton(pats, 0, capi.IMPL_DFA)
    buf = capi.DeviceBuffer(n)
    a.generate(buf.ptr, n, 1, 11)
    r = a.find_device(buf.ptr, n)
    m = r.matches()
    r.free()
    assert len(m) > 1_000_000
    s = a.summarize_device(buf.ptr, n)
    assert s.on_device and s.total == len(m) and [int(v) for v in s.counts()] == [len(m)]
    assert [bool(v) for v in s.any()] == [True]
    f = s.first()[0]
    assert (int(f["pattern"]), int(f["start"]), int(f["end"])) == (int(m[0]["pattern"]), int(m[0]["start"]), int(m[0]["end"]))
    assert np.array_equal(s.by_pattern(), np.bincount(m["pattern"].astype(np.int64), minlength=len(pats)).astype(np.uint64))
    s.free()
    # as a uniform batch of 8 KiB rows (cfg3's shape at this size: 131 072 haystacks)
    L = 8192
    r = a.find_device(buf.ptr, n, n_hay=n // L, uniform_len=L)
    m, counts = r.matches(), r.counts()
    r.free()
    s = a.summarize_device(buf.ptr, n, n_hay=n // L, uniform_len=L)
    assert s.total == len(m) and np.array_equal(s.counts(), counts)
    assert np.array_equal(s.any(), counts > 0)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    f = s.first()
    has = counts > 0
    assert np.array_equal(f[has], m[starts[has]])
    assert np.all(f["pattern"][~has] == np.uint64(capi.NO_MATCH)) and not f["start"][~has].any() and not f["end"][~has].any()
    assert np.array_equal(s.by_pattern(), np.bincount(m["pattern"].astype(np.int64), minlength=len(pats)).astype(np.uint64))
    s.free()
    buf.free(); a.close()


@pytest.mark.parametrize("route", ["host", "device"])
def test_eight_threads_on_one_handle(monkeypatch, route):
    import ahocorasick_rs as ar
    monkeypatch.setenv("ACX_SUMMARY_HOST_MAX", "0" if route == "device" else str(1 << 40))
    pats = gen.gen_patterns(2000, 4, 9, gen.AZ, 3)
    b = ar.BytesAhoCorasick(pats)
    o = Oracle(pats, 0, KIND_DFA)
    work = []
    for t in range(8):
        hays = batch_with_empties(pats, 100 + 31 * t, 500 + t)
        work.append((hays, [o.find(h) for h in hays]))
    errors = []

    def run(t):
        hays, want = work[t]
        try:
            for k in range(6):  # a fixed number of calls, the two kinds in turn
                if (k + t) % 2:
                    assert b.is_match_batch(hays) == [bool(w) for w in want]
                else:
                    assert b.find_matches_as_indexes_batch(hays) == want
            assert b.find_first_batch(hays) == [w[0] if w else None for w in want]
            assert b.count_matches_batch(hays) == [len(w) for w in want]
        except BaseException as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=run, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


_TENSOR_SCRIPT = r"""
import sys
import torch  # first: one process holds ONE HIP runtime, and torch must be the one to load it
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
import gen
from oracle_lib import KIND_DFA, Oracle
import ahocorasick_rs_amd as ac
pats = gen.gen_patterns(3000, 5, 12, gen.AZ, 1)
hay = gen.gen_textlike(3 << 20, 13, pats)
b = ac.BytesAhoCorasick(pats)
o = Oracle(pats, 0, KIND_DFA)
want = o.find(hay.tobytes())
t = torch.from_numpy(hay.copy()).to("cuda:0")
assert b.find_matches_as_indexes(t) == want
assert b.is_match(t) is True and b.find_first(t) == want[0] and b.count_matches(t) == len(want)
assert b.count_by_pattern(t) == np.bincount([w[0] for w in want], minlength=len(pats)).tolist()
assert b.count_matches(t, overlapping=True) == len(o.find(hay.tobytes(), overlapping=True))
assert b.find_first(t[12345:]) == o.find(hay[12345:].tobytes())[0]  # (an odd device address)
empty = torch.zeros(0, dtype=torch.uint8, device="cuda:0")
assert b.is_match(empty) is False and b.find_first(empty) is None and b.count_matches(empty) == 0
assert b.count_matches(torch.from_numpy(hay[:5000])) == len(o.find(hay[:5000].tobytes()))  # (host memory behind DLPack)
assert torch.equal(t.cpu(), torch.from_numpy(hay))
print("OK")
"""


def test_dlpack_haystack_on_the_device():
    """BytesAhoCorasick.is_match / find_first / count_* (tensor in HBM): searched and reduced where it lies.  In a process of
    its own: torch has to be the first to load the HIP runtime."""
    import subprocess
    pytest.importorskip("torch")
    p = subprocess.run([sys.executable, "-c", _TENSOR_SCRIPT, ROOT, os.path.join(ROOT, "tests")], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout + p.stderr


def test_summary_cases_seeded():
    """gpu_fuzz.SUMMARY_N cases of gpu_fuzz.SUMMARY_SEED (tests/test_summary_cpu.py checks what the plan covers)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gpu_fuzz
    n = gpu_fuzz.SUMMARY_N
    ran, failures, skipped, build_errors = gpu_fuzz.run_summary(gpu_fuzz.plan_summary(n, gpu_fuzz.SUMMARY_SEED))
    assert failures == 0, f"{failures} of {n} cases differ from the reference (the lines marked FAIL above)"
    assert build_errors == 0
    assert skipped == 0
    assert ran == n
