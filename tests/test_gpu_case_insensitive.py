"""ascii_case_insensitive on the MI355X.  The expected answer is always the oracle over folded inputs:
ci_find(H, P, kind, overlapping) == find(fold(H), fold(P), kind, overlapping) with the same pattern ids (the crate adds the
opposite-case edge to the same trie node; fold: A-Z -> a-z only).  For LeftmostFirst, Python `re` alternation with
re.IGNORECASE on bytes (ASCII-only folding) is a second, independent check.  Every route is confirmed by path_stats; the
caller's memory is checked byte for byte after the calls."""
import os
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
FOLD = bytes.maketrans(bytes(range(65, 91)), bytes(range(97, 123)))
CI = capi.BUILD_ASCII_CASE_INSENSITIVE


def fold(b) -> bytes:
    return bytes(b).translate(FOLD)


def cols(a):
    return np.stack([a["pattern"], a["start"], a["end"]], 1) if len(a) else np.zeros((0, 3), np.uint64)


def upper_some(b: bytes, seed: int) -> bytes:
    """about half of the ASCII letters upper-cased, by a seeded mask"""
    a = np.frombuffer(b, dtype=np.uint8).copy()
    z = gen.stream_np(seed, len(a))
    m = ((z & np.uint64(1)) == 1) & (a >= 97) & (a <= 122)
    a[m] -= 32
    return a.tobytes()


PATS = [upper_some(p, 100 + i) for i, p in enumerate(gen.gen_patterns(2000, 5, 12, gen.AZ, 1))]
FPATS = [fold(p) for p in PATS]


def text(n: int, seed: int) -> bytes:
    return upper_some(gen.gen_textlike(n, seed, FPATS).tobytes(), seed + 1)


@pytest.fixture(scope="module")
def automata():
    return {mk: capi.Automaton(PATS, mk, ascii_case_insensitive=True) for mk in (0, 1, 2)}


@pytest.fixture(scope="module")
def oracles():
    return {mk: Oracle(FPATS, mk, KIND_DFA) for mk in (0, 1, 2)}


# (size, the counter that says which way the call went)
ROUTES = [(75, "k0"), (16000, "k0"), (300_000, "in_place"), (1 << 20, "in_place"), ((3 << 20) + 7, "folded_on_device")]


@pytest.mark.parametrize("mk", [0, 1, 2])
def test_every_kind_and_route_bytes(automata, oracles, mk):
    a, o = automata[mk], oracles[mk]
    full = text((3 << 20) + 7, 11)
    for n, counter in ROUTES:
        hay = full[:n]
        fh = fold(hay)
        for ov in ([False, True] if mk == 0 else [False]):
            want = o.find_raw(fh, overlapping=ov)
            a.path_stats(reset=True)
            got = cols(a.find(hay, overlapping=ov))
            st = a.path_stats()
            assert got.shape == want.shape and np.array_equal(got, want), (mk, n, ov)
            assert st[counter] >= 1, (n, st)
            if counter != "folded_on_device":
                assert st["folded_on_device"] == 0, (n, st)


def test_leftmost_first_against_re_ignorecase():
    pats = PATS[:300]
    a = capi.Automaton(pats, 1, ascii_case_insensitive=True)
    rx = re.compile(b"|".join(re.escape(p) for p in pats), re.IGNORECASE)
    first = {}
    for i, p in enumerate(pats):
        first.setdefault(fold(p), i)
    for n in (2000, 200_000, (2 << 20) + 3):
        hay = upper_some(gen.gen_textlike(n, 5 + n, [fold(p) for p in pats], plant_every=256).tobytes(), n)
        want = [(first[fold(m.group())], m.start(), m.end()) for m in rx.finditer(hay)]
        assert len(want) > 0
        assert [tuple(int(v) for v in r) for r in a.find(hay)] == want, n


def test_str_api_code_points_and_strings():
    import ahocorasick_rs_amd as ac
    upats = list(dict.fromkeys(gen.gen_patterns(60, 2, 5, gen.AZ_UNI, 5)))
    upats = [p.upper() if i % 3 == 0 else p for i, p in enumerate(upats)] + ["café", "CAFÉ"]
    raw = gen.gen_unicode_textlike(30000, 8, upats)
    chars = list(raw)
    rng = gen.SplitMix64(9)
    for i in range(len(chars)):  # mixed case, non-ASCII included (É is not é for the fold)
        r = rng.next() % 4
        if r == 0:
            chars[i] = chars[i].upper()
    txt = "".join(chars) + " Café CAFÉ café cafÉ"
    fold_s = str.maketrans("ABCDEFGHIJKLMNOPQRSTUVWXYZ", "abcdefghijklmnopqrstuvwxyz")
    for mk in (0, 1, 2):
        o = Oracle([p.encode() for p in upats], mk, KIND_DFA)
        o_f = Oracle([p.translate(fold_s).encode() for p in upats], mk, KIND_DFA)
        want = o_f.find_str(txt.translate(fold_s))
        assert want != o.find_str(txt)  # (the flag changes the answer)
        for sp in (True, False):
            kind = [ac.MatchKind.Standard, ac.MatchKind.LeftmostFirst, ac.MatchKind.LeftmostLongest][mk]
            A = ac.AhoCorasick(upats, matchkind=kind, store_patterns=sp, ascii_case_insensitive=True)
            assert A._info()["ascii_case_insensitive"] is True
            idx = A.find_matches_as_indexes(txt)
            assert idx == want, (mk, sp)
            strs = A.find_matches_as_strings(txt)
            # stored patterns come back as given; otherwise the caller's own text, in its own case
            assert strs == ([upats[p] for p, _, _ in idx] if sp else [txt[s:e] for _, s, e in idx]), (mk, sp)
            if mk == 0:
                assert A.find_matches_as_indexes(txt, overlapping=True) == o_f.find_str(txt.translate(fold_s), overlapping=True)
    assert ac.AhoCorasick(["x"])._info()["ascii_case_insensitive"] is False


def test_patterns_equal_after_folding():
    pats = [b"abc", b"ABC", b"aBc", b"xyz", b"bCd", b"ab"]
    hay_small = b"xx ABCD abcd aBcD XyZ zabcabcABC"
    hay_big = upper_some(gen.gen_uniform(3 << 20, b"abcdxyz ", 4).tobytes(), 6)
    for mk in (0, 1, 2):
        a = capi.Automaton(pats, mk, ascii_case_insensitive=True)
        o = Oracle([fold(p) for p in pats], mk, KIND_DFA)
        for hay in (hay_small, hay_big):
            for ov in ([False, True] if mk == 0 else [False]):
                got = cols(a.find(hay, overlapping=ov))
                want = o.find_raw(fold(hay), overlapping=ov)
                assert got.shape == want.shape and np.array_equal(got, want), (mk, len(hay), ov)
        a.close()


def test_batch_and_callers_memory_untouched(automata, oracles):
    import ahocorasick_rs_amd as ac
    full = text(4 << 20, 21)
    sizes = [0, 100, 5000, 70000, 1, 300000, (1 << 20) + 5, 17]
    hs, at = [], 0
    for s in sizes:
        hs.append(full[at:at + s]); at += s
    a, o = automata[0], oracles[0]
    a.path_stats(reset=True)
    m, counts = a.find_batch(hs)
    assert a.path_stats()["folded_on_device"] == 1
    pos = 0
    for i, h in enumerate(hs):
        want = o.find_raw(fold(h))
        assert int(counts[i]) == len(want) and np.array_equal(cols(m[pos:pos + len(want)]), want), i
        pos += len(want)
    B = ac.BytesAhoCorasick(PATS, ascii_case_insensitive=True)
    assert B.find_matches_as_indexes_batch(hs) == [o.find(fold(h)) for h in hs]
    for n in (75, 300_000, 3 << 20):
        ba = bytearray(full[:n])
        keep = bytes(ba)
        assert B.find_matches_as_indexes(ba) == o.find(fold(keep))
        assert bytes(ba) == keep, n
        assert B.replace_all(ba, [b"#"] * len(PATS)) is not None and bytes(ba) == keep, n


def test_device_buffers_odd_offsets_and_untouched(automata, oracles):
    full = text((2 << 20) + 64, 31)
    buf = capi.DeviceBuffer(len(full)).upload(np.frombuffer(full, dtype=np.uint8))
    for mk in (0, 2):
        a, o = automata[mk], oracles[mk]
        for off, n in ((0, 2 << 20), (1, (2 << 20) - 1), (7, 5000), (13, 300_001), (3, 50)):
            a.path_stats(reset=True)
            r = a.find_device(buf.ptr + off, n)
            got = cols(r.matches())
            r.free()
            st = a.path_stats()
            assert np.array_equal(got, o.find_raw(fold(full[off:off + n]))), (mk, off, n)
            assert st["folded_on_device"] == 1, st
    # a uniform batch at an odd address
    a, o = automata[0], oracles[0]
    L, nh = 8192, 200
    r = a.find_device(buf.ptr + 5, L * nh, n_hay=nh, uniform_len=L)
    m, counts = r.matches(), r.counts()
    r.free()
    pos = 0
    for i in range(nh):
        want = o.find_raw(fold(full[5 + i * L:5 + (i + 1) * L]))
        assert int(counts[i]) == len(want) and np.array_equal(cols(m[pos:pos + len(want)]), want), i
        pos += len(want)
    assert buf.download().tobytes() == full  # the caller's device memory is never written
    buf.free()


def py_splice(hay: bytes, matches, repl) -> bytes:
    out, at = [], 0
    for p, s, e in matches:
        p, s, e = int(p), int(s), int(e)
        out.append(hay[at:s]); out.append(repl[p]); at = e
    out.append(hay[at:])
    return b"".join(out)


@pytest.mark.parametrize("route", ["host", "device"])
def test_replace_all_splices_the_original_bytes(automata, oracles, monkeypatch, route):
    monkeypatch.setenv("ACX_REPLACE_HOST_MAX", str(1 << 40) if route == "host" else "0")
    repl = [bytes([65 + i % 26]) * (i % 5) for i in range(len(PATS))]
    for mk in (0, 1, 2):
        a, o = automata[mk], oracles[mk]
        full = text((2 << 20) + 9, 41)
        for n in (75, 70_000, (2 << 20) + 9):
            hay = full[:n]
            a.path_stats(reset=True)
            got = a.replace(hay, repl)
            assert got == py_splice(hay, o.find_raw(fold(hay)), repl), (route, mk, n)
            assert a.path_stats()["replaced_on_device"] == (1 if route == "device" else 0)
    a, o = automata[0], oracles[0]
    full = text(1 << 20, 43)
    buf = capi.DeviceBuffer(len(full) + 16).upload(np.frombuffer(full + bytes(16), dtype=np.uint8))
    r = a.replace_device(buf.ptr + 3, len(full) - 3, repl)
    assert r.download() == py_splice(full[3:], o.find_raw(fold(full[3:])), repl)
    r.free()
    assert buf.download(len(full)).tobytes() == full
    buf.free()


def test_case_sensitive_handle_beside_it(automata):
    cs = capi.Automaton(PATS, 0)
    o = Oracle(PATS, 0, KIND_DFA)
    full = text(3 << 20, 51)
    buf = capi.DeviceBuffer(len(full)).upload(np.frombuffer(full, dtype=np.uint8))
    cs.path_stats(reset=True)
    for n in (75, 300_000, 3 << 20):
        assert np.array_equal(cols(cs.find(full[:n])), o.find_raw(full[:n])), n
        automata[0].find(full[:n])  # (the case-insensitive handle in between)
    r = cs.find_device(buf.ptr, len(full))
    assert np.array_equal(cols(r.matches()), o.find_raw(full))
    r.free()
    cs.find_batch([full[:1000], full[:(1 << 20) + 1]])
    st = cs.path_stats()
    assert st["folded_on_device"] == 0, st
    assert cs.info.flags == 0 and automata[0].info.flags == CI
    buf.free()
    cs.close()


def test_replicate_keeps_the_flag(automata, oracles):
    r = automata[1].replicate(0)
    assert r.info.flags == CI
    hay = text(1 << 20, 61)
    assert np.array_equal(cols(r.find(hay)), oracles[1].find_raw(fold(hay)))
    r.close()


def test_forced_paths(monkeypatch, oracles):
    # K1a (ACX_KERNEL, read per build), byte ranges (ACX_CHUNK_BYTES, read per call), the hot and dense paths on a dense
    # mixed-case input
    hay = text(3 << 20, 71)
    monkeypatch.setenv("ACX_KERNEL", "dfa_walk")
    a = capi.Automaton(PATS, 0, ascii_case_insensitive=True)
    monkeypatch.delenv("ACX_KERNEL")
    assert capi.KERNEL_NAMES[a.info.kernel] == "dfa_walk"
    for n in (5000, 300_000, 3 << 20):
        assert np.array_equal(cols(a.find(hay[:n])), oracles[0].find_raw(fold(hay[:n]))), n
    a.close()
    a = capi.Automaton(PATS, 2, ascii_case_insensitive=True)
    monkeypatch.setenv("ACX_CHUNK_BYTES", "700001")
    a.path_stats(reset=True)
    got = cols(a.find(hay))
    st = a.path_stats()
    monkeypatch.delenv("ACX_CHUNK_BYTES")
    assert st["byte_ranges"] >= 4 and np.array_equal(got, oracles[2].find_raw(fold(hay)))
    # a pattern every 32 bytes in one 64 KiB region (hot groups), then everywhere (the dense path on the next call)
    dense = bytearray(gen.gen_uniform(8 << 20, gen.AZ, 12).tobytes())
    rng = gen.SplitMix64(77)
    for k in range(1 << 20, (1 << 20) + (64 << 10), 32):
        p = PATS[rng.next() % len(PATS)]
        dense[k:k + len(p)] = p
    dense = upper_some(bytes(dense), 3)
    a0 = capi.Automaton(PATS, 0, ascii_case_insensitive=True)
    a0.path_stats(reset=True)
    assert np.array_equal(cols(a0.find(dense)), oracles[0].find_raw(fold(dense)))
    assert a0.path_stats()["hot_calls"] == 1
    every = bytearray(gen.gen_uniform(8 << 20, gen.AZ, 13).tobytes())
    for k in range(0, len(every) - 32, 32):
        p = PATS[rng.next() % len(PATS)]
        every[k:k + len(p)] = p
    every = upper_some(bytes(every), 4)
    want = oracles[0].find_raw(fold(every))
    a0.path_stats(reset=True)
    for _ in range(2):
        assert np.array_equal(cols(a0.find(every)), want)
    st = a0.path_stats()
    assert st["hot_calls"] + st["dense_tiles"] + st["dense_radix"] >= 2, st
    a0.close()
    a.close()


_CHILD = r"""
import os, sys
sys.path[:0] = [os.environ["ACX_ROOT"], os.path.join(os.environ["ACX_ROOT"], "tests")]
if sys.argv[1] == "tensor":
    import torch  # first: one process holds ONE HIP runtime
import numpy as np
import gen
import test_gpu_case_insensitive as T
from oracle_lib import KIND_DFA, Oracle
import ahocorasick_rs_amd as ac
from ahocorasick_rs_amd import capi
o = Oracle(T.FPATS, 0, KIND_DFA)
if sys.argv[1] == "tensor":
    full = T.text((2 << 20) + 32, 81)
    B = ac.BytesAhoCorasick(T.PATS, ascii_case_insensitive=True)
    t = torch.from_numpy(np.frombuffer(full, dtype=np.uint8).copy()).to("cuda:0")
    for off, n in ((0, 2 << 20), (1, (2 << 20) + 31), (12345, 70000), (3, 40)):
        assert B.find_matches_as_indexes(t[off:off + n]) == o.find(T.fold(full[off:off + n])), (off, n)
    repl = [b"<>"] * len(T.PATS)
    assert B.replace_all(t[1:], repl) == T.py_splice(full[1:], o.find_raw(T.fold(full[1:])), repl)
    assert t.cpu().numpy().tobytes() == full
else:
    a = capi.Automaton(T.PATS, 0, ascii_case_insensitive=True)
    hays = [T.text(60 + (k % 7) * 90, 200 + k) for k in range(300)] + [T.text(16000, 7)]
    a.path_stats(reset=True)
    for h in hays:
        assert np.array_equal(T.cols(a.find(h)), o.find_raw(T.fold(h)))
    st = a.path_stats()
    print("STATS", st["k0"], st["resident_launches"], st["folded_on_device"])
print("OK")
"""


@pytest.mark.parametrize("env", [{}, {"ACX_NO_RESIDENT": "1"}])
def test_k0_resident_and_launched(env):
    r = subprocess.run([sys.executable, "-c", _CHILD, "small"], env={**os.environ, **env, "ACX_ROOT": ROOT},
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    k0, launches, folded = [int(x) for x in next(l for l in r.stdout.splitlines() if l.startswith("STATS")).split()[1:]]
    assert k0 == 301 and folded == 0
    assert (launches == 0) if env else (1 <= launches < 301)


def test_device_tensor_odd_offsets():
    pytest.importorskip("torch")
    r = subprocess.run([sys.executable, "-c", _CHILD, "tensor"], env={**os.environ, "ACX_ROOT": ROOT},
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_eight_threads_one_handle(automata, oracles):
    a, o = automata[0], oracles[0]
    full = text((3 << 20) + 100, 91)
    buf = capi.DeviceBuffer(len(full)).upload(np.frombuffer(full, dtype=np.uint8))
    cases = [(0, 75), (10, 4000), (100, 300_000), (5, 900_000), (1, (3 << 20) + 50), (3, 1 << 20)]
    want = [o.find_raw(fold(full[s:s + n])) for s, n in cases]
    errors = []

    def worker(t):
        try:
            for it in range(8):
                i = (t + it) % len(cases)
                s, n = cases[i]
                if (t + it) % 3 == 0:
                    r = a.find_device(buf.ptr + s, n)
                    got = cols(r.matches())
                    r.free()
                else:
                    got = cols(a.find(full[s:s + n]))
                if not np.array_equal(got, want[i]):
                    errors.append((t, it, i))
        except Exception as e:  # pragma: no cover - reported below
            errors.append((t, repr(e)))

    th = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors[:5]
    assert buf.download().tobytes() == full
    buf.free()
