"""GPU: the code-point conversion (the str API's offsets) at its seams, on every route that has a form of it.

The forms (kernels.hip): K1b's CP variant counts lead bytes per 16 bytes while it scans; k_count_leads does it for haystacks
K1b did not count (an aligned 16-byte branch and a byte-wise one); k_block_partials -> k_block_prefix build the prefix
over 1 KiB blocks, BP_BLOCKS blocks a workgroup, the sentinel entry possibly alone in the last one; code_point_of() takes a
carried count from k_tile_main, or counts x's chunk in place -- one aligned 16-byte load, or lead_bytes_between() on an
unaligned haystack --, and sums the block's count bytes under a mask; k_tile_write adds the pattern's characters,
k_to_code_points and k_localize count the span, k_localize subtracts its haystack's first byte; K0, launched and resident,
converts by itself; a call in byte ranges converts once, over pieces that begin inside characters.

The haystacks, their plants and what they are there for come from tests/cp_seams.py, sized from the constants of the
sources; tests/test_cp_seams_cpu.py shows on the CPU that every seam is reached by a match the oracle reports.  Every test
here compares complete row arrays with the oracle's byte rows mapped through cp_seams.code_points(); nothing expected
comes from the library, and path_stats says which way a call went.  LeftmostLongest (cfg5's kind) unless stated.

Out of scope: beyond 4 GiB block_prefix() falls back to the library's device-wide scan; no haystack here is larger than
2 MiB + 5 KiB + 321 bytes (the seams lie at 16 B, 1 KiB, 4 KiB, 16 KiB, 256 KiB and 1 MiB)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cp_seams as S
from oracle_lib import KIND_DFA, Oracle

pytestmark = pytest.mark.gpu
capi = pytest.importorskip("ahocorasick_rs_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = ord("#")  # around a device haystack: LEAD bytes, so that a count that leaves its range shows
QUIET = ("hot_calls", "dense_tiles", "dense_radix", "k0", "byte_ranges", "overflow_regrown", "wide_redone")


def cols(a):
    return np.stack([a["pattern"], a["start"], a["end"]], 1).astype(np.uint64) if len(a) else np.zeros((0, 3), np.uint64)


def same_rows(got, want, what, byte_rows=None):
    """complete arrays; the message names the first wrong row and where its match starts"""
    got = np.asarray(got, dtype=np.uint64).reshape(-1, 3)
    if got.shape == want.shape and np.array_equal(got, want):
        return
    k = next((i for i in range(min(len(got), len(want))) if not np.array_equal(got[i], want[i])), min(len(got), len(want)))
    where = ""
    if byte_rows is not None and k < len(byte_rows):
        x = int(byte_rows[k][1])
        where = f"; its match starts at byte {x}: x mod 16 = {x % 16}, x mod 1024 = {x % 1024}, block {x // 1024}"
    raise AssertionError(f"{what}: {len(got)} rows, expected {len(want)}; first wrong row {k}: "
                         f"{got[k].tolist() if k < len(got) else None}, expected {want[k].tolist() if k < len(want) else None}{where}")


class Device:
    """one buffer for every haystack of the module: [guard][haystack at the residue asked for][guard]"""

    def __init__(self):
        self.buf = capi.DeviceBuffer(S.sizes().big + 64)
        assert self.buf.ptr % 16 == 0
        self.image = None

    def put(self, hay: np.ndarray, lead: int = 0) -> int:
        self.image = np.concatenate([np.full(16 + lead, GUARD, np.uint8), hay, np.full(32 - lead, GUARD, np.uint8)])
        self.buf.upload(self.image)
        return self.buf.ptr + 16 + lead

    def unchanged(self) -> bool:
        return np.array_equal(self.buf.download(len(self.image)), self.image)


@pytest.fixture(scope="module")
def dev():
    d = Device()
    yield d
    d.buf.free()


@pytest.fixture(scope="module")
def handles():
    hs = {mk: capi.Automaton(S.PATS_B, mk) for mk in (0, 1, 2)}
    for a in hs.values():
        assert a.info.kernel == capi.KERNEL_PREFILTER  # (the sparse path's scan is K1b)
    yield hs
    for a in hs.values():
        a.close()


def find_device(a, ptr, n, ov=False, **kw):
    a.path_stats(reset=True)
    r = a.find_device(ptr, n, overlapping=ov, codepoints=True, **kw)
    got, counts = cols(r.matches()), (r.counts() if r.n_hay else None)
    r.free()
    return got, counts, a.path_stats()


def sparse_only(st, what):
    assert st["sparse"] == 1 and all(st[k] == 0 for k in QUIET), f"{what}: {sorted(st.items())}"


# ---------------------------------------------------------------------------
# one haystack in HBM
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("w", S.WIDTHS)
def test_aligned_device_haystack_every_kind(dev, handles, w):
    """K1b<CP> -> the prefix on the side stream -> k_tile_write<CPW> with the carried counts"""
    for c in (c for c in S.plan() if c.width == w):
        ptr = dev.put(c.hay)
        assert ptr % 16 == 0
        for mk, ov in S.KINDS:
            got, _, st = find_device(handles[mk], ptr, len(c.hay), ov)
            same_rows(got, S.expected(c.name, mk, ov), (c.name, mk, ov), S.byte_rows(c.name, mk, ov))
            sparse_only(st, (c.name, mk, ov))


@pytest.mark.parametrize("lead", [1, 7, 8, 15])
@pytest.mark.parametrize("w", S.WIDTHS)
def test_unaligned_device_haystack(dev, handles, w, lead):
    """k_count_leads' byte branch -> block_prefix(sub = nullptr) -> k_to_code_points through lead_bytes_between()"""
    a = handles[2]
    for c in (c for c in S.plan() if c.width == w):
        ptr = dev.put(c.hay, lead)
        assert ptr % 16 == lead
        got, _, st = find_device(a, ptr, len(c.hay))
        same_rows(got, S.expected(c.name, *S.LL), (c.name, lead), S.byte_rows(c.name, *S.LL))
        sparse_only(st, (c.name, lead))
        assert dev.unchanged(), (c.name, lead)  # the caller's bytes (and what lies around them)


@pytest.mark.parametrize("w", ["w1", "w4"])
def test_the_walks_hits_carry_no_count(dev, w):
    """the DFA walk's occurrences come without a window: every start is counted in place (CP_UNKNOWN), aligned haystack"""
    a = capi.Automaton(S.PATS_B, 2, kernel=capi.KERNEL_DFA_WALK)
    assert a.info.kernel == capi.KERNEL_DFA_WALK
    for c in (c for c in S.plan() if c.width == w):
        got, _, st = find_device(a, dev.put(c.hay), len(c.hay))
        same_rows(got, S.expected(c.name, *S.LL), (c.name, "walk"), S.byte_rows(c.name, *S.LL))
        assert st["k0"] == st["byte_ranges"] == 0, st
    a.close()


# ---------------------------------------------------------------------------
# batches: k_localize
# ---------------------------------------------------------------------------
def batch_expected(h, offs):
    rows = [S.expected_of(h[a:b], *S.LL) for a, b in zip(offs[:-1], offs[1:])]
    return np.concatenate(rows).astype(np.uint64), np.array([len(r) for r in rows], dtype=np.uint64)


def test_uniform_batches(dev, handles):
    for h, ul in S.uniform_batches():
        n_hay = len(h) // ul
        want, want_counts = batch_expected(h, [k * ul for k in range(n_hay + 1)])
        got, counts, st = find_device(handles[2], dev.put(h), len(h), n_hay=n_hay, uniform_len=ul)
        same_rows(got, want, ("uniform", ul))
        assert np.array_equal(counts, want_counts), ul
        assert st["k0"] == st["byte_ranges"] == 0 and len(want) >= 16, f"{sorted(st.items())}"


@pytest.mark.parametrize("lead", [0, 5])
def test_ragged_batch_from_device_memory(dev, handles, lead):
    h, offs = S.ragged_batch()
    want, want_counts = batch_expected(h, offs)
    d_offs = capi.DeviceBuffer(8 * len(offs)).upload(np.array(offs, dtype=np.uint64))
    got, counts, st = find_device(handles[2], dev.put(h, lead), len(h), d_offsets=d_offs.ptr, n_hay=len(offs) - 1)
    d_offs.free()
    same_rows(got, want, ("ragged", lead))
    assert np.array_equal(counts, want_counts) and (want_counts == 0).sum() >= 5 and len(want) >= 30
    assert st["k0"] == st["byte_ranges"] == 0, f"{sorted(st.items())}"
    assert dev.unchanged()


def test_ragged_batch_from_host_memory(handles):
    h, offs = S.ragged_batch()
    want, want_counts = batch_expected(h, offs)
    m, counts = handles[2].find_batch([h[a:b].tobytes() for a, b in zip(offs[:-1], offs[1:])], codepoints=True)
    same_rows(cols(m), want, "ragged, host")
    assert np.array_equal(counts, want_counts)


# ---------------------------------------------------------------------------
# a call in byte ranges: the pieces begin inside characters
# ---------------------------------------------------------------------------
def test_byte_ranges_cut_inside_characters(dev, handles, monkeypatch):
    for name, h, piece in S.range_cases():
        ptr = dev.put(h)
        for mk, ov in (S.LL, (0, True)):
            want = S.expected_of(h, mk, ov)
            monkeypatch.setenv("ACX_CHUNK_BYTES", str(piece))
            got, _, st = find_device(handles[mk], ptr, len(h), ov)
            monkeypatch.delenv("ACX_CHUNK_BYTES")
            same_rows(got, want, (name, mk, ov))
            assert st["byte_ranges"] >= 3 and st["byte_ranges"] >= len(h) // piece, (name, st)
    assert "ACX_CHUNK_BYTES" not in os.environ


# ---------------------------------------------------------------------------
# hot groups and the dense path: their words carry no count
# ---------------------------------------------------------------------------
def cells(width: str, nbytes: int) -> np.ndarray:
    """a pattern every 32 bytes: cells of a short pattern, the filler's characters and pad bytes, valid on their own"""
    unit, out = S.UNITS[width], []
    for k in range(nbytes // 32):
        p = S.PATS_B[S.SHORT_IDS[k % len(S.SHORT_IDS)]] + b"z"
        p += unit * ((31 - len(p)) // len(unit))
        out.append(p + b"z" * (32 - len(p)))
    return np.frombuffer(b"".join(out), dtype=np.uint8)


@pytest.mark.parametrize("w", ["w4", "mixed"])
def test_hot_groups(w):
    z = S.sizes()
    h = np.array(S.case(f"{w}-big").hay)
    at = 6 * z.group + 8 * z.tile
    S.overwrite(h, at, cells(w, 64 << 10).tobytes())
    h.tobytes().decode("utf-8")
    want = S.expected_of(h, *S.LL)
    a = capi.Automaton(S.PATS_B, 2)
    a.path_stats(reset=True)
    got = cols(a.find(h, codepoints=True))
    st = a.path_stats()
    same_rows(got, want, ("hot", w), S.oracle(2).find_raw(h))
    assert st["hot_calls"] == 1 and st["dense_tiles"] == st["dense_radix"] == 0 and len(want) > 2000, st
    a.close()


@pytest.mark.parametrize("w", ["w3", "mixed"])
def test_dense_everywhere(w):
    h = cells(w, S.sizes().big)
    h.tobytes().decode("utf-8")
    want = S.expected_of(h, *S.LL)
    assert len(want) == len(h) // 32
    a = capi.Automaton(S.PATS_B, 2)  # (a fresh handle: its first call finds out, its second one takes the dense path)
    a.path_stats(reset=True)
    same_rows(cols(a.find(h, codepoints=True)), want, ("dense, first call", w), S.oracle(2).find_raw(h))
    st = a.path_stats(reset=True)
    assert st["hot_calls"] == 1 and st["dense_tiles"] == st["dense_radix"] == 0, st
    same_rows(cols(a.find(h, codepoints=True)), want, ("dense, second call", w), S.oracle(2).find_raw(h))
    st = a.path_stats()
    assert st["dense_tiles"] + st["dense_radix"] == 1 and st["hot_calls"] == 0, st
    a.close()


# ---------------------------------------------------------------------------
# K0, launched and resident
# ---------------------------------------------------------------------------
def k0_sets():
    """an automaton per way K0 finds its occurrences (kernels.hip small_mode): compared directly (four patterns of at most
    16 bytes: up to 1 024 bytes; the LDS table beyond), the table in LDS (every second pattern: 170 states of 32 classes
    fit K0_LT_ENTRIES), the tables in global memory (all of them: 263 states do not; the prefilter beyond 1 KiB)"""
    few = [S.PATS_B[i] for i in (0, 12, 18, 31)]
    assert all(len(p) <= 16 for p in few) and S.SPAN36 % 2 == 0 and S.LONG_TAIL[0] % 2 == 0
    return {"direct comparison": few, "table in LDS": S.PATS_B[::2], "tables in global memory": S.PATS_B}


def run_k0_loops(resident: bool) -> None:
    hays = [S.head(S.case(f"{w}-big").hay, n) for n in S.K0_CUTS for w in S.WIDTHS]
    for which, pats in k0_sets().items():
        o = Oracle(pats, 2, KIND_DFA)
        want = [S.map_rows(o.find_raw(h), S.code_points(h)) for h in hays]
        a = capi.Automaton(pats, 2)
        a.path_stats(reset=True)
        calls = 0
        for k, h in enumerate(hays):
            for _ in range(3):  # (a loop of calls: nothing between them)
                got = cols(a.find(h, codepoints=True))
                calls += 1
                same_rows(got, want[k], (which, len(h), S.WIDTHS[k % len(S.WIDTHS)], "resident" if resident else "launched"),
                          o.find_raw(h))
        st = a.path_stats()
        assert st["k0"] == calls and st["sparse"] == 0, (which, st)
        assert (st["resident_launches"] >= 1) if resident else (st["resident_launches"] == 0), (which, st)
        a.close()


def test_k0_resident_loops():
    assert "ACX_NO_RESIDENT" not in os.environ
    run_k0_loops(True)


def test_k0_launched_loops():
    """ACX_NO_RESIDENT is read once per process: the same loops in a process of their own"""
    code = ("import os, sys; sys.path[:0] = [os.environ['ACX_ROOT'], os.path.join(os.environ['ACX_ROOT'], 'tests')]; "
            "import test_gpu_cp_seams as T; T.run_k0_loops(False); print('OK')")
    r = subprocess.run([sys.executable, "-c", code], env={**os.environ, "ACX_NO_RESIDENT": "1", "ACX_ROOT": ROOT},
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


# ---------------------------------------------------------------------------
# the Python class
# ---------------------------------------------------------------------------
def test_the_python_class():
    import ahocorasick_rs_amd as ac
    a = ac.AhoCorasick(S.PATTERNS, matchkind=ac.MatchKind.LeftmostLongest)
    c = S.case("mixed-mid")
    text = c.hay.tobytes().decode("utf-8")
    want = [tuple(int(v) for v in r) for r in S.expected(c.name, *S.LL)]
    assert a.find_matches_as_indexes(text) == want
    strings = a.find_matches_as_strings(text)
    assert strings == [S.PATTERNS[p] for p, _, _ in want] and all(text[s:e] == S.PATTERNS[p] for p, s, e in want)
    col = a.find_matches_as_columns(text)
    assert len(col) == len(want)
    for k, part in enumerate((col.pattern, col.start, col.end)):
        assert np.array_equal(np.from_dlpack(part), np.array([r[k] for r in want], dtype=np.int64)), k
    # an all-ASCII str: the code points ARE the byte offsets
    h = np.array(S.case("w1-mid").hay)
    h[h >= 0x80] = S.PAD
    text = h.tobytes().decode("ascii")
    rows = S.oracle(2).find_raw(h)
    assert len(rows) >= 30 and np.array_equal(S.map_rows(rows, S.code_points(h)), rows.astype(np.uint64))
    want = [tuple(int(v) for v in r) for r in rows]
    assert a.find_matches_as_indexes(text) == want
    assert a.find_matches_as_strings(text) == [S.PATTERNS[p] for p, _, _ in want]
    assert np.array_equal(np.from_dlpack(a.find_matches_as_columns(text).end), np.array([r[2] for r in want], dtype=np.int64))
