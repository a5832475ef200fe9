"""The device splice (csrc/replace.hip) and the device fold (csrc/fold.hip) at their seams: device batches, the scan's
second and third level, replacements longer than an output tile, tiles crowded with deletions, the 32 bytes at either
end of the haystack and of the blob at every pointer residue, a find beneath that was cut, and the fold's head / body /
tail at every pointer residue.

Every size is derived from the kernels' own constants, read out of the .hip sources, so that a retuned kernel moves its
tests with it.  The expected output is always built without the code under test: the oracle's matches (over the folded
bytes for a case-insensitive handle) spliced by plain Python / numpy, per haystack.

What enters which branch (the constants as they stand: RS_ITEMS = 2 048, RG_TILE = 16 384, RG_WIN = 1 024):
  row_begin(): uniform_len / off       test_device_batch_uniform / test_device_batch_ragged (n_hay = 200 / 13)
  k_rep_positions' search over S.first the same two, and test_counts_scan_beyond_one_level (n_hay > RS_ITEMS: the counts
                                       scan takes two levels)
  scan_level, three levels             test_three_scan_levels (the oracle's row count is asserted: RS_ITEMS^2 + 1 and beyond)
  k_rep_gather, whole tiles inside one replacement   test_long_segments (6 RG_TILE + 7 bytes anywhere; RG_TILE bytes from output byte 0)
  k_rep_gather, rounds with deletions  test_crowded_tiles_mixed_lengths (~RG_TILE segments per tile), test_deletion_runs
  load16, either side of its test      test_ends_and_alignment (16 pointer residues x 16 output residues)
  run_replace over a cut find          test_cut_find_* (byte_ranges / hot_calls / dense_* asserted)
  k_fold head / tail / n16 == 0        test_fold_* (folded_on_device asserted)"""
import os
import re

import numpy as np
import pytest

import gen
from oracle_lib import KIND_DFA, Oracle, byte_to_code_point

pytestmark = pytest.mark.gpu
capi = pytest.importorskip("ahocorasick_rs_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ahocorasick_rs_amd", "csrc")


def hip_constants(path: str, names):
    src = open(os.path.join(CSRC, path)).read()
    out = {}
    for n in names:
        m = re.search(r"\b%s\s*=\s*(\d+)\s*[,;]" % n, src)
        assert m, f"{n} is no longer a plain constant of {path}"
        out[n] = int(m.group(1))
    return out


_C = {**hip_constants("replace.hip", ("RS_THREADS", "RS_PER", "RG_TILE", "RG_WIN")),
      **hip_constants("fold.hip", ("FOLD_THREADS", "FOLD_UNROLL"))}
RS_ITEMS = _C["RS_THREADS"] * _C["RS_PER"]
RG_TILE, RG_WIN = _C["RG_TILE"], _C["RG_WIN"]
FOLD_SPAN = 16 * _C["FOLD_THREADS"] * _C["FOLD_UNROLL"]  # bytes one workgroup's unrolled pass covers
FOLD = bytes.maketrans(bytes(range(65, 91)), bytes(range(97, 123)))


def test_constants_are_what_the_sizes_below_assume():
    # (not their values: their relations -- a tile is whole 16-byte chunks, a window is smaller than a crowded tile)
    assert RS_ITEMS >= 64 and RS_ITEMS ** 2 * 2 * 1.2 <= 16 << 20, "three scan levels no longer fit a 16 MB haystack"
    assert RG_TILE % 16 == 0 and 2 * RG_WIN + 8 < RG_TILE
    assert FOLD_SPAN * 64 <= 16 << 20


# ---------------------------------------------------------------------------
# the expected value
# ---------------------------------------------------------------------------
def py_splice(hay: bytes, matches, repl) -> bytes:
    out, at = [], 0
    for p, s, e in matches:
        p, s, e = int(p), int(s), int(e)
        assert s >= at
        out.append(hay[at:s]); out.append(repl[p]); at = e
    out.append(hay[at:])
    return b"".join(out)


def np_splice(hay: np.ndarray, m: np.ndarray, repl) -> np.ndarray:
    """py_splice for millions of matches: the kept bytes and the replacement bytes keep their order, so the output is two
    masked assignments"""
    p, s, e = (m[:, k].astype(np.int64) for k in range(3))
    rlen = np.array([len(r) for r in repl], dtype=np.int64)[p]
    mlen = e - s
    assert (s[1:] >= e[:-1]).all()
    keep = np.ones(len(hay), dtype=bool)
    keep[np.repeat(s - (np.cumsum(mlen) - mlen), mlen) + np.arange(int(mlen.sum()))] = False
    o = s + (np.cumsum(rlen - mlen) - (rlen - mlen))  # where every replacement starts in the output
    total = len(hay) + int((rlen - mlen).sum())
    blob = np.frombuffer(b"".join(repl) + b"\0", dtype=np.uint8)
    roff = (np.cumsum([0] + [len(r) for r in repl])[:-1])[p]
    before = np.cumsum(rlen) - rlen
    k = np.arange(int(rlen.sum()))
    out = np.empty(total, dtype=np.uint8)
    is_rep = np.zeros(total, dtype=bool)
    pos = np.repeat(o - before, rlen) + k
    is_rep[pos] = True
    out[pos] = blob[np.repeat(roff - before, rlen) + k]
    out[~is_rep] = hay[keep]
    return out


def test_np_splice_is_the_plain_splice():
    hay = gen.gen_uniform(5000, b"abcdx", 3)
    pats, repl = [b"ab", b"cd", b"xx"], [b"", b"XYZ", b"q"]
    m = Oracle(pats, 0, KIND_DFA).find_raw(hay)
    assert len(m) > 300 and np_splice(hay, m, repl).tobytes() == py_splice(hay.tobytes(), m, repl)


def first_diff(got: bytes, want: bytes) -> str:
    a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
    n = min(len(a), len(b))
    d = np.nonzero(a[:n] != b[:n])[0]
    i = int(d[0]) if len(d) else n
    return f"got {len(a)} want {len(b)} bytes, first difference at byte {i} (tile {i // RG_TILE}, byte {i % RG_TILE} of it): " \
           f"got {got[i:i + 8]!r} want {want[i:i + 8]!r}"


def same(got: bytes, want: bytes, what=None):
    assert got == want, (what, first_diff(got, want))


def mixed_repl(n: int, seed: int, lens=(0, 1, 4, 7, 12, 20, 64)):
    rng = gen.SplitMix64(seed)
    return [bytes(65 + (rng.next() % 26) for _ in range(lens[rng.next() % len(lens)])) for _ in range(n)]


def upper_some(b: bytes, seed: int) -> bytes:
    a = np.frombuffer(b, dtype=np.uint8).copy()
    z = gen.stream_np(seed, len(a))
    sel = ((z & np.uint64(1)) == 1) & (a >= 97) & (a <= 122)
    a[sel] -= 32
    return a.tobytes()


class OnDevice:
    """`data` in HBM at a pointer that is `off` modulo 16 (hipMalloc's pointers are multiples of 16), inside a buffer
    filled with 0xA5 around it"""

    def __init__(self, data, off: int = 0):
        d = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        self.image = np.concatenate([np.full(off, 0xA5, np.uint8), d, np.full(16, 0xA5, np.uint8)])
        self.buf = capi.DeviceBuffer(len(self.image)).upload(self.image)
        assert self.buf.ptr % 16 == 0
        self.ptr, self.n = self.buf.ptr + off, len(d)

    def unchanged(self) -> bool:
        return np.array_equal(self.buf.download(), self.image)

    def free(self):
        self.buf.free()


def u64_on_device(values) -> "capi.DeviceBuffer":
    a = np.ascontiguousarray(np.asarray(values, dtype=np.uint64))
    return capi.DeviceBuffer(a.nbytes).upload(a.view(np.uint8))


def check_device_batch(a, orc, hs, repl, off, *, uniform_len=0, fold=False, what=None, stats=None):
    """replace_device over the haystacks `hs` laid behind one another at pointer residue `off`: the bytes, offsets() and
    the caller's buffer; stats: receives the call's path_stats"""
    want = [py_splice(h, orc.find_raw(h.translate(FOLD) if fold else h), repl) for h in hs]
    dev = OnDevice(b"".join(hs), off)
    d_off = None
    a.path_stats(reset=True)
    if uniform_len:
        r = a.replace_device(dev.ptr, dev.n, repl, n_hay=len(hs), uniform_len=uniform_len)
    else:
        d_off = u64_on_device(np.cumsum([0] + [len(h) for h in hs]))
        r = a.replace_device(dev.ptr, dev.n, repl, d_offsets=d_off.ptr, n_hay=len(hs))
    st = a.path_stats()
    got, bounds = r.download(), [int(v) for v in r.offsets()]
    r.free()
    assert st["replaced_on_device"] == 1, st
    if stats is not None:
        stats.update(st)
    want_bounds = [int(v) for v in np.cumsum([0] + [len(w) for w in want])]
    if bounds != want_bounds:
        i = next(k for k in range(len(bounds)) if bounds[k] != want_bounds[k])
        raise AssertionError((what, f"offsets()[{i}] is {bounds[i]}, the splice of haystacks 0 .. {i - 1} has {want_bounds[i]} bytes"))
    for i, w in enumerate(want):
        same(got[bounds[i]:bounds[i + 1]], w, (what, "haystack", i))
    assert dev.unchanged(), (what, "the caller's buffer was written")
    dev.free()
    if d_off:
        d_off.free()
    return want


# ---------------------------------------------------------------------------
# device batches
# ---------------------------------------------------------------------------
PATS = gen.gen_patterns(2000, 5, 12, gen.AZ, 1)
REPL = mixed_repl(len(PATS), 3)


@pytest.fixture(scope="module")
def automata():
    return {mk: capi.Automaton(PATS, mk, capi.IMPL_DFA) for mk in (0, 1, 2)}


@pytest.fixture(scope="module")
def oracles():
    return {mk: Oracle(PATS, mk, KIND_DFA) for mk in (0, 1, 2)}


@pytest.mark.parametrize("off", [0, 1, 5, 15])
def test_device_batch_uniform(automata, oracles, off):
    L, nh = 8192, 200
    full = gen.gen_textlike(L * nh, 61, PATS).tobytes()
    hs = [full[i * L:(i + 1) * L] for i in range(nh)]
    for mk in (0, 1, 2):
        check_device_batch(automata[mk], oracles[mk], hs, REPL, off, uniform_len=L, what=("uniform", mk, off))


def ragged_batch():
    full = gen.gen_textlike(2 << 20, 62, PATS).tobytes()
    nomatch = b"0123456789" * 500
    sizes = [0, 100, 5000, 0, 0, 70000, -300, 1, (1 << 20) + 77, 17, -4096, 33, 0]  # (negative: that many bytes without a match)
    hs, at = [], 0
    for s in sizes:
        if s < 0:
            hs.append(nomatch[:-s])
        else:
            hs.append(full[at:at + s]); at += s
    return hs


@pytest.mark.parametrize("off", [0, 1, 5, 15])
def test_device_batch_ragged(automata, oracles, monkeypatch, off):
    hs = ragged_batch()
    assert len(hs[0]) == 0 and len(hs[-1]) == 0 and max(len(h) for h in hs) > 1 << 20
    for mk in (0, 1, 2):
        want = check_device_batch(automata[mk], oracles[mk], hs, REPL, off, what=("ragged", mk, off))
        assert want[6] == hs[6] and want[10] == hs[10] and want[5] != hs[5]
        if off == 0:  # the same batch from host memory, staged and spliced on the device
            monkeypatch.setenv("ACX_REPLACE_HOST_MAX", "0")
            automata[mk].path_stats(reset=True)
            got = automata[mk].replace_batch(hs, REPL)
            assert automata[mk].path_stats()["replaced_on_device"] == 1
            monkeypatch.delenv("ACX_REPLACE_HOST_MAX")
            assert len(got) == len(want)
            for i, w in enumerate(want):
                same(got[i], w, ("replace_batch", mk, i))


def test_counts_scan_beyond_one_level(monkeypatch):
    names = gen.names_like()
    pats = [p.encode() for p in names]
    repl = mixed_repl(len(pats), 17)
    n_lines = RS_ITEMS + RS_ITEMS // 8 + 3
    hs = [b"" if i % 7 == 5 else ln.encode() for i, ln in enumerate(gen.names_lines(names, n_lines, every=3))]
    assert len(hs) > RS_ITEMS and hs[5] == b"" and sum(len(h) for h in hs) < 16 << 20
    a, orc = capi.Automaton(pats, 0), Oracle(pats, 0, KIND_DFA)
    want = check_device_batch(a, orc, hs, repl, 3, what="lines")
    assert sum(w != h for w, h in zip(want, hs)) > n_lines // 4  # (a name every third line, most of them replaced)
    monkeypatch.setenv("ACX_REPLACE_HOST_MAX", "0")
    a.path_stats(reset=True)
    got = a.replace_batch(hs, repl)
    assert a.path_stats()["replaced_on_device"] == 1
    assert got == want
    a.close()


# ---------------------------------------------------------------------------
# the scan over the matches: one, two and three levels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [RS_ITEMS, RS_ITEMS + 1, RS_ITEMS ** 2 - 1, RS_ITEMS ** 2, RS_ITEMS ** 2 + 1,
                               RS_ITEMS ** 2 * 6 // 5])
def test_three_scan_levels(n):
    # two-byte units "ab" (deleted: -2), "cd" (+1) and "xy" (no match; no pattern lies across two units), laid out by a
    # seeded draw: exactly n matches, and a partial put in the wrong place shifts everything behind it
    pats, repl = [b"ab", b"cd"], [b"", b"XYZ"]
    units = n + n // 16 + 5
    order = np.argsort(gen.stream_np(1000 + n % 997, units), kind="stable")
    kind = np.full(units, 2, dtype=np.int64)
    kind[order[:n]] = (gen.stream_np(7, n) >> np.uint64(13)).astype(np.int64) & 1
    hay = np.frombuffer(b"abcdxy", dtype=np.uint8).reshape(3, 2)[kind].reshape(-1)
    assert len(hay) <= 16 << 20
    m = Oracle(pats, 0, KIND_DFA).find_raw(hay)
    assert len(m) == n
    want = np_splice(hay, m, repl)
    a = capi.Automaton(pats, 0, capi.IMPL_DFA)
    dev = OnDevice(hay, 0)
    a.path_stats(reset=True)
    r = a.replace_device(dev.ptr, dev.n, repl)
    assert a.path_stats()["replaced_on_device"] == 1
    assert r.nbytes == len(want) and [int(v) for v in r.offsets()] == [0, len(want)]
    same(r.download(), want.tobytes(), n)
    r.free()
    dev.free()
    a.close()


# ---------------------------------------------------------------------------
# the gather: replacements longer than a tile
# ---------------------------------------------------------------------------
def filler(n: int, seed: int) -> bytes:
    return gen.gen_uniform(n, b"mnopqrstuvwxyz ", seed).tobytes()


def blob_bytes(n: int, seed: int) -> bytes:
    return gen.gen_uniform(n, gen.ALL_BYTES, seed).tobytes()  # (not periodic in 16: a chunk from the wrong offset differs)


@pytest.mark.parametrize("where", ["first", "last", "tile_end", "adjacent", "all_of_it"])
@pytest.mark.parametrize("rlen", [RG_TILE - 1, RG_TILE, RG_TILE + 1, 6 * RG_TILE + 7])
def test_long_segments(rlen, where):
    pats = [b"@", b"QQ", b"#"]
    repl = [blob_bytes(rlen, 5), b"", blob_bytes(rlen + 5, 6)]
    h = bytearray(filler(3 * RG_TILE + 11, 8))
    if where == "first":
        h[0:1] = b"@"
    elif where == "last":
        h[-1:] = b"#"
    elif where == "tile_end":  # the replacement's last byte is the last byte of an output tile
        s = RG_TILE + (-rlen) % RG_TILE
        h[s:s + 1] = b"@"
        assert (s + rlen) % RG_TILE == 0
    elif where == "adjacent":
        h[1000:1002] = b"@#"
    else:
        h = bytearray(b"@")
    h = bytes(h)
    a, orc = capi.Automaton(pats, 0), Oracle(pats, 0, KIND_DFA)
    for off in (0, 7):
        dev = OnDevice(h, off)
        r = a.replace_device(dev.ptr, dev.n, repl)
        want = py_splice(h, orc.find_raw(h), repl)
        assert len(want) >= rlen
        same(r.download(), want, (rlen, where, off))
        r.free()
        assert dev.unchanged()
        dev.free()
    a.close()


# ---------------------------------------------------------------------------
# the gather: rounds of RG_WIN segments with deletions among them
# ---------------------------------------------------------------------------
CROWD_PATS, CROWD_REPL = [b"ab", b"cd", b"ef", b"gh"], [b"", b"", b"1", b"XYZ"]


def test_crowded_tiles_mixed_lengths():
    # adjacent two-byte matches, one output byte each on average: a tile holds about RG_TILE segments, many of them
    # beginning at one output offset
    units = 6 * RG_TILE
    kind = (gen.stream_np(23, units) >> np.uint64(11)).astype(np.int64) & 3
    hay = np.frombuffer(b"abcdefgh", dtype=np.uint8).reshape(4, 2)[kind].reshape(-1)
    m = Oracle(CROWD_PATS, 0, KIND_DFA).find_raw(hay)
    assert len(m) == units
    want = np_splice(hay, m, CROWD_REPL)
    assert len(want) >= 4 * RG_TILE
    a = capi.Automaton(CROWD_PATS, 0)
    for off in (0, 9):
        dev = OnDevice(hay, off)
        r = a.replace_device(dev.ptr, dev.n, CROWD_REPL)
        same(r.download(), want.tobytes(), off)
        r.free()
        dev.free()
    a.close()


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("at", [RG_TILE - 8, RG_TILE - 1, RG_TILE, RG_TILE + 1, RG_TILE + RG_TILE // 2 + 3])
def test_deletion_runs(at, split):
    # more than 2 RG_WIN deletions in a row whose (empty) output lies at byte `at` of the output, then unmatched bytes;
    # split: one byte of output in the middle of the run, so that its halves lie on either side of byte `at`
    run = 2 * RG_WIN + 3
    dele = np.frombuffer(b"abcd", dtype=np.uint8).reshape(2, 2)[(gen.stream_np(at, run) & np.uint64(1)).astype(np.int64)]
    dele = dele.reshape(-1).tobytes()
    h = filler(at, 4) + dele + (b"ef" + dele if split else b"") + filler(2 * RG_TILE + 5, 5)
    orc = Oracle(CROWD_PATS, 0, KIND_DFA)
    m = orc.find_raw(h)
    assert len(m) == run * (2 if split else 1) + int(split)
    want = py_splice(h, m, CROWD_REPL)
    assert len(want) == at + int(split) + 2 * RG_TILE + 5
    a = capi.Automaton(CROWD_PATS, 0)
    dev = OnDevice(h, 3)
    r = a.replace_device(dev.ptr, dev.n, CROWD_REPL)
    same(r.download(), want, (at, split))
    r.free()
    dev.free()
    a.close()


# ---------------------------------------------------------------------------
# load16 and the last store: the 32 bytes at either end, every residue
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("off", range(16))
def test_ends_and_alignment(off):
    pats = [b"@@", b"##", b"$$", b"%%"]
    repl = [blob_bytes(5, 1), b"", blob_bytes(16, 2), blob_bytes(33, 3)]  # (the blob's first and last entry are both used)
    a, orc = capi.Automaton(pats, 0), Oracle(pats, 0, KIND_DFA)
    residues = set()
    for k in range(16):
        n = 2 * RG_TILE + 100 + k
        h = bytearray(filler(n, 40 + k))
        first = (off + 3 * k) % 29          # a match inside the first 32 bytes ...
        last = n - 2 - (5 * off + k) % 29   # ... and inside the last 32
        h[first:first + 2] = pats[off % 4]  # (by the residue alone: the output's length then moves with k, by one)
        h[last:last + 2] = pats[(off // 4 + off) % 4]
        h[5000:5002], h[RG_TILE + 70:RG_TILE + 72], h[9000:9004] = pats[0], pats[3], pats[1] + pats[2]
        h = bytes(h)
        want = py_splice(h, orc.find_raw(h), repl)
        residues.add(len(want) % 16)
        dev = OnDevice(h, off)
        r = a.replace_device(dev.ptr, dev.n, repl)
        assert r.nbytes == len(want)
        same(r.download(), want, (off, k))
        r.free()
        assert dev.unchanged()
        dev.free()
    assert residues == set(range(16))
    a.close()


def test_output_lengths_of_every_residue():
    # one replacement of 0 .. 47 bytes: every residue of the output's length, the last 16-byte store into the rounded buffer
    pats = [b"@@"]
    a = capi.Automaton(pats, 0)
    h = bytearray(filler(RG_TILE + 40, 9))
    h[RG_TILE + 10:RG_TILE + 12] = b"@@"
    h = bytes(h)
    dev = OnDevice(h, 11)
    for rl in range(48):
        repl = [blob_bytes(rl, 100 + rl)]
        r = a.replace_device(dev.ptr, dev.n, repl)
        same(r.download(), h[:RG_TILE + 10] + repl[0] + h[RG_TILE + 12:], rl)
        r.free()
    dev.free()
    a.close()


# ---------------------------------------------------------------------------
# a find beneath that was cut
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mk", [0, 1, 2])
def test_cut_find_byte_ranges_one_haystack(automata, oracles, monkeypatch, mk):
    hay = gen.gen_textlike((3 << 20) + 4321, 71, PATS).tobytes()
    want = py_splice(hay, oracles[mk].find_raw(hay), REPL)
    a = automata[mk]
    monkeypatch.setenv("ACX_CHUNK_BYTES", "700001")
    monkeypatch.setenv("ACX_REPLACE_HOST_MAX", "0")
    a.path_stats(reset=True)
    got = a.replace(hay, REPL)
    st = a.path_stats()
    assert st["byte_ranges"] == 5 and st["replaced_on_device"] == 1, st
    same(got, want, mk)
    dev = OnDevice(hay, 13)
    a.path_stats(reset=True)
    r = a.replace_device(dev.ptr, dev.n, REPL)
    st = a.path_stats()
    assert st["byte_ranges"] == 5 and st["replaced_on_device"] == 1, st
    same(r.download(), want, (mk, "device"))
    r.free()
    dev.free()


@pytest.mark.parametrize("mk", [0, 1, 2])
def test_cut_find_batch_over_the_occurrence_limit(monkeypatch, mk):
    # the batch of test_gpu_chunked.py: one pass may index 50 000 occurrences, the batch is cut at haystack boundaries
    import random
    pats, repl = [b"ab", b"b", b"bab"], [b"", b"12345", b"Z"]
    r = random.Random(5)
    hs = [b"ab" * r.randint(1, 60_000) + bytes(r.choice(b"abc") for _ in range(r.randint(0, 300))) for _ in range(7)] + [b"", b"abab"]
    a, orc = capi.Automaton(pats, mk), Oracle(pats, mk, KIND_DFA)
    want = [py_splice(h, orc.find_raw(h), repl) for h in hs]
    monkeypatch.setenv("ACX_MAX_OCC", "50000")
    monkeypatch.setenv("ACX_NO_BUCKET", "1")
    monkeypatch.setenv("ACX_REPLACE_HOST_MAX", "0")
    a.path_stats(reset=True)
    got = a.replace_batch(hs, repl)
    st = a.path_stats()
    assert st["byte_ranges"] >= 2 and st["replaced_on_device"] == 1, st
    for i, w in enumerate(want):
        same(got[i], w, (mk, i))
    st = {}
    check_device_batch(a, orc, hs, repl, 5, what=("max_occ", mk), stats=st)
    assert st["byte_ranges"] >= 2, st
    a.close()


CI_PATS = [upper_some(p, 100 + i) for i, p in enumerate(PATS)]  # (the sets of test_gpu_case_insensitive.py)
CI_FPATS = [p.translate(FOLD) for p in CI_PATS]


@pytest.mark.parametrize("mk", [0, 1, 2])
def test_cut_find_hot_and_dense_paths(monkeypatch, mk):
    # the inputs of test_gpu_case_insensitive.py::test_forced_paths: a pattern every 32 bytes in one 64 KiB region (hot
    # groups), then everywhere (the dense path on the next call), mixed case, replacements of mixed lengths
    monkeypatch.setenv("ACX_REPLACE_HOST_MAX", "0")
    orc = Oracle(CI_FPATS, mk, KIND_DFA)
    dense = bytearray(gen.gen_uniform(8 << 20, gen.AZ, 12).tobytes())
    rng = gen.SplitMix64(77)
    for k in range(1 << 20, (1 << 20) + (64 << 10), 32):
        p = CI_PATS[rng.next() % len(CI_PATS)]
        dense[k:k + len(p)] = p
    dense = upper_some(bytes(dense), 3)
    a = capi.Automaton(CI_PATS, mk, ascii_case_insensitive=True)
    a.path_stats(reset=True)
    got = a.replace(dense, REPL)
    st = a.path_stats()
    assert st["hot_calls"] == 1 and st["replaced_on_device"] == 1, st
    same(got, py_splice(dense, orc.find_raw(dense.translate(FOLD)), REPL), (mk, "hot"))
    every = bytearray(gen.gen_uniform(8 << 20, gen.AZ, 13).tobytes())
    for k in range(0, len(every) - 32, 32):
        p = CI_PATS[rng.next() % len(CI_PATS)]
        every[k:k + len(p)] = p
    every = upper_some(bytes(every), 4)
    m = orc.find_raw(every.translate(FOLD))
    want = np_splice(np.frombuffer(every, dtype=np.uint8), m, REPL).tobytes()
    a.path_stats(reset=True)
    for _ in range(2):
        same(a.replace(every, REPL), want, (mk, "dense"))
    st = a.path_stats()
    assert st["hot_calls"] + st["dense_tiles"] + st["dense_radix"] >= 2 and st["replaced_on_device"] == 2, st
    a.close()


# ---------------------------------------------------------------------------
# the fold
# ---------------------------------------------------------------------------
# the neighbours of both letter ranges, letters of both cases, and bytes >= 0x80 that are a letter + 0x80 (bit 5 clear / set)
FOLD_ALPHA = b"@[`{AaZzMm" + bytes([0xC1, 0xDA, 0xE1, 0xFA])
FOLD_PATS = list(dict.fromkeys(gen.gen_patterns(60, 2, 3, FOLD_ALPHA, 31)))
FOLD_FPATS = [p.translate(FOLD) for p in FOLD_PATS]


def cols(a):
    return np.stack([a["pattern"], a["start"], a["end"]], 1) if len(a) else np.zeros((0, 3), np.uint64)


def check_fold(a, orc, image: "OnDevice", full: bytes, cases):
    a.path_stats(reset=True)
    calls = 0
    for n in cases:
        hay = full[:n]
        r = a.find_device(image.ptr, n)
        got = cols(r.matches())
        r.free()
        want = orc.find_raw(hay.translate(FOLD))
        assert got.shape == want.shape and np.array_equal(got, want), (image.ptr % 16, n)
        calls += n > 0
    assert a.path_stats()["folded_on_device"] == calls
    assert image.unchanged(), "the caller's buffer was written"


@pytest.fixture(scope="module")
def fold_handle():
    assert {0x40, 0x5B, 0x60, 0x7B, 0xC1, 0xE1} <= set(FOLD_ALPHA)
    return capi.Automaton(FOLD_PATS, 0, ascii_case_insensitive=True), Oracle(FOLD_FPATS, 0, KIND_DFA)


@pytest.mark.parametrize("off", range(16))
def test_fold_short_lengths_every_residue(fold_handle, off):
    a, orc = fold_handle
    full = gen.gen_uniform(48, FOLD_ALPHA, 50 + off).tobytes()
    image = OnDevice(full, off)
    check_fold(a, orc, image, full, range(49))
    image.free()


@pytest.mark.parametrize("off", [0, 1, 8, 15])
def test_fold_unrolled_loop_hand_over(fold_handle, off):
    a, orc = fold_handle
    ks = (1, 2, 5, 64)
    full = gen.gen_uniform(FOLD_SPAN * ks[-1] + 17, FOLD_ALPHA, 70 + off).tobytes()
    image = OnDevice(full, off)
    check_fold(a, orc, image, full, [FOLD_SPAN * k + d for k in ks for d in (-17, -16, -1, 0, 1, 15, 16, 17)])
    image.free()


def test_fold_every_byte_value():
    # all 256 byte values through the fold, against a pattern per value: only A-Z may change
    pats = [bytes([0x7C, v]) for v in range(256)]
    a = capi.Automaton(pats, 1, ascii_case_insensitive=True)
    orc = Oracle([p.translate(FOLD) for p in pats], 1, KIND_DFA)
    full = b"".join(pats) * 3 + b"|"
    for off in (0, 5):
        image = OnDevice(full, off)
        check_fold(a, orc, image, full, [len(full), len(full) - 1, 515])
        image.free()
    a.close()


def test_fold_code_points_beyond_1_mib():
    import ahocorasick_rs_amd as ac
    upats = list(dict.fromkeys(gen.gen_patterns(300, 2, 6, gen.AZ_UNI, 5)))
    raw = gen.gen_unicode_textlike_bytes(1_100_000, 8, upats).tobytes()
    assert len(raw) > (1 << 20) + 1000
    hay = upper_some(raw, 9)  # (ASCII letters only: the bytes of the other characters stay as they are)
    txt = hay.decode("utf-8")
    mixed = [p.upper() if i % 3 == 0 else p for i, p in enumerate(upats)]
    bpats = [p.encode() for p in mixed]
    b2c = byte_to_code_point(hay)
    for mk in (0, 1, 2):
        m = Oracle([p.translate(FOLD) for p in bpats], mk, KIND_DFA).find_raw(hay.translate(FOLD))
        want = np.stack([m[:, 0], b2c[m[:, 1].astype(np.int64)], b2c[m[:, 2].astype(np.int64)]], 1)
        assert len(want) > 1000 and int(want[-1, 2]) < int(m[-1, 2])
        a = capi.Automaton(bpats, mk, ascii_case_insensitive=True)
        a.path_stats(reset=True)
        got = cols(a.find(hay, codepoints=True))
        assert a.path_stats()["folded_on_device"] == 1
        assert got.shape == want.shape and np.array_equal(got, want), mk
        a.close()
        kind = [ac.MatchKind.Standard, ac.MatchKind.LeftmostFirst, ac.MatchKind.LeftmostLongest][mk]
        A = ac.AhoCorasick(mixed, matchkind=kind, ascii_case_insensitive=True)
        assert A.find_matches_as_indexes(txt) == [tuple(int(v) for v in r) for r in want], mk


def test_fold_uniform_batch_at_full_size():
    a = capi.Automaton(CI_PATS, 0, ascii_case_insensitive=True)
    orc = Oracle(CI_FPATS, 0, KIND_DFA)
    L, nh = 1024, RS_ITEMS + 52
    full = upper_some(gen.gen_textlike(L * nh, 81, CI_FPATS, plant_every=256).tobytes(), 82)
    hs = [full[i * L:(i + 1) * L] for i in range(nh)]
    image = OnDevice(full, 7)
    a.path_stats(reset=True)
    r = a.find_device(image.ptr, len(full), n_hay=nh, uniform_len=L)
    m, counts = cols(r.matches()), r.counts()
    r.free()
    assert a.path_stats()["folded_on_device"] == 1
    want = [orc.find_raw(h.translate(FOLD)) for h in hs]
    assert [int(c) for c in counts] == [len(w) for w in want]
    assert np.array_equal(m, np.concatenate(want).astype(np.uint64))
    assert image.unchanged()
    image.free()
    check_device_batch(a, orc, hs, REPL, 7, uniform_len=L, fold=True, what="ci uniform")
    a.close()
