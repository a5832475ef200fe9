"""replace_all on the MI355X: both routes (host splice behind acx_find up to ACX_REPLACE_HOST_MAX, device splice beyond),
every match kind, the Python API, density edges, batches, an output beyond 2^32 bytes and threads.  The expected output
is always a plain splice of the oracle's matches (or, for str, of find_matches_as_indexes)."""
import ctypes
import threading

import numpy as np
import pytest

import gen
from oracle_lib import KIND_DFA, Oracle

pytestmark = pytest.mark.gpu

capi = pytest.importorskip("ahocorasick_rs_amd.capi")
HOST, DEVICE = str(1 << 40), "0"  # ACX_REPLACE_HOST_MAX values that force each route


def py_splice(hay: bytes, matches, repl) -> bytes:
    out, at = [], 0
    for p, s, e in matches:
        p, s, e = int(p), int(s), int(e)
        out.append(hay[at:s])
        out.append(repl[p])
        at = e
    out.append(hay[at:])
    return b"".join(out)


def mixed_repl(n: int, seed: int, lens=(0, 1, 4, 7, 12, 20, 64)):
    rng = gen.SplitMix64(seed)
    out = []
    for i in range(n):
        L = lens[rng.next() % len(lens)]
        out.append(bytes(65 + (rng.next() % 26) for _ in range(L)))
    return out


PATS = gen.gen_patterns(2000, 5, 12, gen.AZ, 1)
REPL = mixed_repl(len(PATS), 3)


@pytest.fixture(scope="module")
def automata():
    return {mk: capi.Automaton(PATS, mk, capi.IMPL_DFA) for mk in (0, 1, 2)}


@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("mk", [0, 1, 2])
def test_both_routes_every_kind(automata, monkeypatch, route, mk):
    monkeypatch.setenv("ACX_REPLACE_HOST_MAX", HOST if route == "host" else DEVICE)
    a = automata[mk]
    orc = Oracle(PATS, mk, KIND_DFA)
    full = gen.gen_textlike(16 << 20, 21, PATS).tobytes()
    for n in (0, 75, 16 << 10, (64 << 10) + 1, (1 << 20) + 1, 16 << 20):
        hay = full[:n]
        a.path_stats(reset=True)
        got = a.replace(hay, REPL)
        assert got == py_splice(hay, orc.find_raw(hay), REPL), (route, mk, n)
        if n:
            assert a.path_stats()["replaced_on_device"] == (1 if route == "device" else 0)


def test_default_route_by_size(automata, monkeypatch):
    monkeypatch.delenv("ACX_REPLACE_HOST_MAX", raising=False)
    a = automata[0]
    hay = gen.gen_textlike(2 << 20, 5, PATS).tobytes()
    for n, dev in ((1 << 20, 0), ((1 << 20) + 1, 1)):
        a.path_stats(reset=True)
        a.replace(hay[:n], REPL)
        assert a.path_stats()["replaced_on_device"] == dev, n


UPATS = list(dict.fromkeys(gen.gen_patterns(60, 2, 5, gen.AZ_UNI, 5)))


@pytest.mark.parametrize("route", ["host", "device"])
def test_str_api_utf8(monkeypatch, route):
    import ahocorasick_rs_amd as ac
    monkeypatch.setenv("ACX_REPLACE_HOST_MAX", HOST if route == "host" else DEVICE)
    text = gen.gen_unicode_textlike(40000, 8, UPATS)
    repl = ["", "é", "☃☃", "🤦x", "plain", "ü" * 9] * (len(UPATS) // 6 + 1)
    repl = repl[:len(UPATS)]
    for mk in (ac.MatchKind.Standard, ac.MatchKind.LeftmostFirst, ac.MatchKind.LeftmostLongest):
        A = ac.AhoCorasick(UPATS, matchkind=mk)
        m = A.find_matches_as_indexes(text)
        assert len(m) > 50
        out, at = [], 0
        for p, s, e in m:
            out.append(text[at:s]); out.append(repl[p]); at = e
        out.append(text[at:])
        assert A.replace_all(text, repl) == "".join(out)
        assert A.replace_all(text, iter(repl)) == "".join(out)  # any iterable, materialised once
    with pytest.raises(ValueError):
        A.replace_all(text, repl[:-1])
    with pytest.raises(TypeError):
        A.replace_all(text, [r.encode() for r in repl])


def test_bytes_api_buffers(monkeypatch):
    import ahocorasick_rs_amd as ac
    B = ac.BytesAhoCorasick(PATS)
    hay = gen.gen_textlike(3 << 20, 9, PATS).tobytes()
    want = py_splice(hay, Oracle(PATS, 0, KIND_DFA).find_raw(hay), REPL)
    for h in (hay, bytearray(hay), memoryview(hay)):
        got = B.replace_all(h, REPL)
        assert type(got) is bytes and got == want
    assert B.replace_all(b"", REPL) == b""
    nomatch = b"0123456789" * 100
    got = B.replace_all(nomatch, REPL)
    assert got == nomatch and got is not nomatch
    with pytest.raises(ValueError):
        B.replace_all(hay, REPL + [b"x"])
    with pytest.raises(ValueError, match="2001 entries.*2000 patterns"):
        capi.Automaton(PATS).replace(hay[:100], REPL + [b"x"])


_TENSOR_SCRIPT = r"""
import sys
import torch  # first: one process holds ONE HIP runtime, and torch must be the one to load it
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import gen
import test_gpu_replace as T
from oracle_lib import KIND_DFA, Oracle
import ahocorasick_rs_amd as ac
B = ac.BytesAhoCorasick(T.PATS)
hay = gen.gen_textlike(3 << 20, 9, T.PATS)
want = T.py_splice(hay.tobytes(), Oracle(T.PATS, 0, KIND_DFA).find_raw(hay), T.REPL)
t = torch.from_numpy(hay).to("cuda:0")
assert B.replace_all(t, T.REPL) == want
assert B.replace_all(t[12345:], T.REPL) == B.replace_all(hay[12345:].tobytes(), T.REPL)
assert B.replace_all(torch.from_numpy(hay[:5000]), T.REPL) == B.replace_all(hay[:5000].tobytes(), T.REPL)
print("OK")
"""


def test_bytes_api_device_tensor():
    """BytesAhoCorasick.replace_all(tensor in HBM): searched and spliced where it lies.  In a process of its own: torch
    has to be the first to load the HIP runtime."""
    import os
    import subprocess
    import sys
    pytest.importorskip("torch")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", _TENSOR_SCRIPT, root, os.path.join(root, "tests")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout + p.stderr


@pytest.mark.parametrize("rlen", [0, 1, 2, 37])
def test_density_every_byte_matched(monkeypatch, rlen):
    monkeypatch.setenv("ACX_REPLACE_HOST_MAX", DEVICE)
    a = capi.Automaton([b"ab"], 0, capi.IMPL_DFA)
    N = 600_000
    hay = b"ab" * N
    r = bytes(range(65, 65 + rlen))
    a.path_stats(reset=True)
    got = a.replace(hay, [r])
    assert a.path_stats()["replaced_on_device"] == 1
    assert got == r * N


def test_single_long_replacement_and_tile_boundaries(monkeypatch):
    monkeypatch.setenv("ACX_REPLACE_HOST_MAX", DEVICE)
    pats = [b"QQQQQQQQ", b"@"]
    a = capi.Automaton(pats, 0, capi.IMPL_DFA)
    base = gen.gen_textlike(1 << 20, 31).tobytes()
    # one 10 KiB replacement
    h = bytearray(base); h[500_001] = ord("@")
    big = bytes(gen.gen_uniform(10 << 10, gen.AZ, 4))
    assert a.replace(bytes(h), [b"", big]) == bytes(h[:500_001]) + big + bytes(h[500_002:])
    # matches straddling every 16 KiB output tile boundary (equal lengths: output offsets = input offsets), and the same
    # with a shift that moves them across the 16-byte chunks
    h = bytearray(base)
    for k in range(1, len(h) // 16384):
        h[k * 16384 - 4:k * 16384 + 4] = pats[0]
    h = bytes(h)
    m = Oracle(pats, 0, KIND_DFA).find_raw(h)
    assert len(m) == len(h) // 16384 - 1
    for repl in ([b"abcdefgh", b"#"], [b"abcdefghijk", b""], [b"xyz", b"###"]):
        assert a.replace(h, repl) == py_splice(h, m, repl)


@pytest.mark.parametrize("route", ["host", "device"])
def test_batch(monkeypatch, route):
    import ahocorasick_rs_amd as ac
    monkeypatch.setenv("ACX_REPLACE_HOST_MAX", HOST if route == "host" else DEVICE)
    full = gen.gen_textlike(2 << 20, 41, PATS).tobytes()
    sizes = [0, 100, 5000, 0, 70000, 1, 300000, 0, 1 << 20, 17]
    hs, at = [], 0
    for s in sizes:
        hs.append(full[at:at + s]); at += s
    B = ac.BytesAhoCorasick(PATS)
    orc = Oracle(PATS, 0, KIND_DFA)
    want = [py_splice(h, orc.find_raw(h), REPL) for h in hs]
    assert B.replace_all_batch(hs, REPL) == want
    assert [B.replace_all(h, REPL) for h in hs] == want
    assert capi.Automaton(PATS).replace_batch(hs, REPL) == want
    assert B.replace_all_batch([], REPL) == []
    A = ac.AhoCorasick([p.decode() for p in PATS])
    assert A.replace_all_batch([h.decode() for h in hs], [r.decode() for r in REPL]) == [w.decode() for w in want]


def expected_window(hay: np.ndarray, m: np.ndarray, repl, rlen: np.ndarray, lo: int, hi: int) -> bytes:
    """bytes [lo, hi) of the splice of `hay` by the matches m, without building the whole output"""
    p, s, e = m[:, 0].astype(np.int64), m[:, 1].astype(np.int64), m[:, 2].astype(np.int64)
    d = rlen[p] - (e - s)
    P = np.concatenate([[0], np.cumsum(d)])
    o = s + P[:-1]
    total = len(hay) + int(P[-1])
    hi = min(hi, total)
    out = []
    x = lo
    j = int(np.searchsorted(o, lo, side="right")) - 1
    n = len(o)
    while x < hi:
        nxt = int(o[j + 1]) if j + 1 < n else total
        if j >= 0 and x < int(o[j]) + int(rlen[p[j]]):
            k = x - int(o[j])
            take = min(hi, int(o[j]) + int(rlen[p[j]])) - x
            out.append(repl[int(p[j])][k:k + take])
        else:
            shift = int(P[j + 1]) if j >= 0 else 0
            end = min(hi, nxt)
            out.append(hay[x - shift:end - shift].tobytes())
            take = end - x
        x += take
        while j + 1 < n and int(o[j + 1]) <= x:
            j += 1
    return b"".join(out)


def test_output_beyond_2_32_bytes():
    pats = gen.gen_patterns(10000, 5, 12, gen.AZ, 1)
    repl = [bytes([65 + i % 26]) * 4096 for i in range(len(pats))]
    a = capi.Automaton(pats, 0, capi.IMPL_DFA)
    n = 1 << 30
    buf = capi.DeviceBuffer(n)
    a.generate(buf.ptr, n, 1, 11)
    a.path_stats(reset=True)
    r = a.replace_device(buf.ptr, n, repl)
    assert a.path_stats()["replaced_on_device"] == 1
    hay = buf.download()
    m = Oracle(pats, 0, KIND_DFA).find_raw(hay)
    rlen = np.array([len(x) for x in repl], dtype=np.int64)
    total = n + int((rlen[m[:, 0].astype(np.int64)] - (m[:, 2] - m[:, 1]).astype(np.int64)).sum())
    assert total > (1 << 32) and r.nbytes == total
    assert [int(v) for v in r.offsets()] == [0, total]
    ptr = r.device_ptr
    rng = gen.SplitMix64(99)
    windows = [(0, 64 << 20), (total - (64 << 20), total)] + [
        (w, w + (1 << 20)) for w in (int(rng.next() % (total - (1 << 20))) for _ in range(16))]
    for lo, hi in windows:
        got = bytearray(hi - lo)
        capi._check(capi.lib().acx_device_download((ctypes.c_uint8 * len(got)).from_buffer(got), ptr + lo, hi - lo))
        assert bytes(got) == expected_window(hay, m, repl, rlen, lo, hi), (lo, hi)
    r.free()
    buf.free()


def test_threads_one_handle_both_routes(monkeypatch):
    import ahocorasick_rs_amd as ac
    monkeypatch.delenv("ACX_REPLACE_HOST_MAX", raising=False)
    B = ac.BytesAhoCorasick(PATS)
    orc = Oracle(PATS, 0, KIND_DFA)
    full = gen.gen_textlike(3 << 20, 51, PATS).tobytes()
    cases = [full[k * 1000:k * 1000 + s] for k, s in enumerate((2000, 200_000, (3 << 20) - 8000, 40, 900_000, (1 << 20) + 5))]
    want = [py_splice(h, orc.find_raw(h), REPL) for h in cases]
    errors = []

    def worker(t):
        try:
            for it in range(6):
                i = (t + it) % len(cases)
                if B.replace_all(cases[i], REPL) != want[i]:
                    errors.append((t, it, i))
        except Exception as e:  # pragma: no cover - reported below
            errors.append((t, repr(e)))

    th = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors
