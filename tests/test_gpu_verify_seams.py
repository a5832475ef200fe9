"""GPU: verify_candidate() -- the one place where a prefix hit becomes an occurrence -- and the packed occurrence words of
k_tile_main / k_tile_write / k_dense_main at their field limits, on every route that runs them.

verify_candidate() (kernels.hip) compares four byte ranges by four mechanisms: [0, Q2) is the prefix table's word,
[Q2, Q2 + n0) comes from the 16 haystack bytes that travel with the hit and the 12 pattern bytes of pinfo, everything behind
is compared in place, 32 bytes a round in four masked pieces, and an anchored pattern's head through a window of its own;
room / back keep an occurrence inside its haystack, length 255 in pinfo means "read plen", lists are verified two
candidates at a time.  Its callers: k_tile_main (sparse path), k_walk_hits (dense path, radix form), k_dense_verify
(dense path, tile-ordered), k_hot_verify (hot groups), K0's prefilter mode.  A wrong verify reports a match only where a
near miss lies: tests/verify_seams.py plants one at every byte of every length class, and tests/test_verify_seams_cpu.py
shows on the CPU that the oracle reports none of them and that every class is there.

Every test compares complete (pattern, start, end) arrays with the oracle's rows, the overlapping Standard search with
verify_seams.brute() too; path_stats says which way a call went.  No haystack is longer than 2 groups + 5 000 bytes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import verify_seams as V

pytestmark = pytest.mark.gpu
capi = pytest.importorskip("ahocorasick_rs_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = ord("#")
QUIET = ("hot_calls", "dense_tiles", "dense_radix", "k0", "byte_ranges", "wide_redone")
PACKED = [r.name for r in V.packed_rows()]
NARROW = [r.name for r in V.packed_rows() if V.narrow_expected(r.n, r.max_len)]


def cols(a):
    return np.stack([a["pattern"], a["start"], a["end"]], 1).astype(np.uint64) if len(a) else np.zeros((0, 3), np.uint64)


def same_rows(got, want, what):
    """complete arrays; the message names the first wrong row"""
    got = np.asarray(got, dtype=np.uint64).reshape(-1, 3)
    want = np.asarray(want, dtype=np.uint64).reshape(-1, 3)
    if got.shape == want.shape and np.array_equal(got, want):
        return
    k = next((i for i in range(min(len(got), len(want))) if not np.array_equal(got[i], want[i])), min(len(got), len(want)))
    raise AssertionError(f"{what}: {len(got)} rows, expected {len(want)}; first wrong row {k}: "
                         f"{got[k].tolist() if k < len(got) else None}, expected {want[k].tolist() if k < len(want) else None}")


class Device:
    """one buffer for every haystack of the module: [guard][haystack at the residue asked for][guard]"""

    def __init__(self):
        self.buf = capi.DeviceBuffer(V.HAY_LEN + 64)
        assert self.buf.ptr % 16 == 0

    def put(self, hay, lead: int = 0) -> int:
        hay = np.frombuffer(hay, dtype=np.uint8) if isinstance(hay, (bytes, bytearray)) else hay
        self.buf.upload(np.concatenate([np.full(16 + lead, GUARD, np.uint8), hay, np.full(32 - lead, GUARD, np.uint8)]))
        return self.buf.ptr + 16 + lead


@pytest.fixture(scope="module")
def dev():
    d = Device()
    yield d
    d.buf.free()


_HANDLES = {}


def patterns_of(name):
    return list(V.packed_patterns(name) if name.startswith("pw") else V.patterns(name))


def handle(name: str, mk: int, forced: bool = True):
    """one automaton per (set, kind, scan kernel asked for) for the whole module.  forced: K1b's prefilter whatever the
    set's size, and K0 does not take the call"""
    key = (name, mk, forced)
    if key not in _HANDLES:
        _HANDLES[key] = capi.Automaton(patterns_of(name), mk, kernel=capi.KERNEL_PREFILTER if forced else None)
    return _HANDLES[key]


@pytest.fixture(scope="module", autouse=True)
def close_handles():
    yield
    for a in _HANDLES.values():
        a.close()
    _HANDLES.clear()


def find_device(a, ptr, n, ov=False, **kw):
    a.path_stats(reset=True)
    r = a.find_device(ptr, n, overlapping=ov, **kw)
    got, counts = cols(r.matches()), (r.counts() if r.n_hay else None)
    r.free()
    return got, counts, a.path_stats()


def check_every_kind(name, ptr, hay, want_of, stats_ok, what, **kw):
    for mk, ov in V.KINDS:
        got, _, st = find_device(handle(name, mk), ptr, len(hay), ov, **kw)
        same_rows(got, want_of(mk, ov), (name, what, mk, ov))
        if (mk, ov) == (0, True) and not name.startswith("pw"):
            same_rows(got, V.brute(V.patterns(name), hay), (name, what, "brute"))
        assert stats_ok(st), (name, what, mk, ov, sorted(st.items()))


def sparse_only(st):
    return st["sparse"] == 1 and all(st[k] == 0 for k in QUIET)


# ---------------------------------------------------------------------------
# verify cases: one haystack
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", V.VERIFY_SETS)
def test_sparse_path(dev, name):
    """K1b -> k_tile_main: ONE candidate (A), a list two at a time (B, the list sets), anchored (urls)"""
    c = V.case(name)
    ptr = dev.put(c.hay)
    assert ptr % 16 == 0
    check_every_kind(name, ptr, c.hay, lambda mk, ov: V.expected(name, mk, ov), sparse_only, "aligned")


@pytest.mark.parametrize("name", V.VERIFY_SETS)
def test_sparse_path_at_residue_7(dev, name):
    c = V.case(name)
    ptr = dev.put(c.hay, 7)
    assert ptr % 16 == 7
    check_every_kind(name, ptr, c.hay, lambda mk, ov: V.expected(name, mk, ov), sparse_only, "residue 7")


@pytest.mark.parametrize("form", ["tiles", "radix"])
@pytest.mark.parametrize("name", V.VERIFY_SETS)
def test_dense_path(dev, monkeypatch, name, form):
    """ACX_NO_BUCKET=1: no sparse attempt -- k_dense_verify (tile-ordered) or, with ACX_NO_DENSE_TILES=1, the hit regions ->
    k_walk_hits -> radix sort"""
    c = V.case(name)
    ptr = dev.put(c.hay)
    monkeypatch.setenv("ACX_NO_BUCKET", "1")
    if form == "radix":
        monkeypatch.setenv("ACX_NO_DENSE_TILES", "1")

    def dense(st):
        mine, other = ("dense_tiles", "dense_radix") if form == "tiles" else ("dense_radix", "dense_tiles")
        return st["sparse"] == st["hot_calls"] == 0 and st[mine] >= 1 and st[other] == 0

    check_every_kind(name, ptr, c.hay, lambda mk, ov: V.expected(name, mk, ov), dense, form)


@pytest.mark.parametrize("name", V.VERIFY_SETS)
def test_hot_pipeline(dev, name):
    """a dense stretch in the second group: k_hot_verify verifies that group's hits, k_tile_main the first group's"""
    h = V.hot_hay(name)
    ptr = dev.put(h)
    check_every_kind(name, ptr, h, lambda mk, ov: V.rows_of(name, h, mk, ov),
                     lambda st: st["hot_calls"] >= 1 and st["dense_tiles"] == st["dense_radix"] == 0, "hot")


@pytest.mark.parametrize("name", V.VERIFY_SETS)
def test_k0(name):
    """the same copies in pieces of at most 16 384 bytes (K0's own modes) and in 40 000 bytes (its prefilter mode)"""
    pieces = V.k0_pieces(name)
    for k, h in enumerate(pieces):
        for mk, ov in V.KINDS:
            a = handle(name, mk, forced=False)
            a.path_stats(reset=True)
            a.profile_read(reset=True)
            got = cols(a.find(np.ascontiguousarray(h), overlapping=ov))
            st, small = a.path_stats(), a.profile_read().small_calls
            same_rows(got, V.rows_of(name, h, mk, ov), (name, "K0 piece", k, mk, ov))
            assert st["k0"] >= 1 or small == 1, (name, k, mk, ov, sorted(st.items()))


# ---------------------------------------------------------------------------
# verify cases: room and back -- rows as haystacks of their own, and as batches
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("forced", [True, False], ids=["pipeline", "K0"])
@pytest.mark.parametrize("name", V.VERIFY_SETS)
def test_every_row_as_a_haystack_of_its_own(dev, name, forced):
    """the haystack ends with a pattern's last byte, one byte short of it (the byte IS there, behind the end), begins with
    an anchored pattern (back < shift), begins behind its head"""
    rs = V.rows(name, False)
    offs = V.offsets_of(rs)
    ptr = dev.put(b"".join(r.data for r in rs))
    for mk, ov in V.KINDS:
        a = handle(name, mk, forced)
        want = V.row_expected(name, False, mk, ov)
        for k, r in enumerate(rs):
            got, _, st = find_device(a, ptr + offs[k], len(r.data), ov)
            same_rows(got, want[k], (name, "row", k, r.what, r.pid, r.c, mk, ov))
            assert (st["k0"] == 0 and st["sparse"] + st["hot_calls"] >= 1) if forced else st["k0"] == 1, (name, k, sorted(st.items()))


def batch_expected(name, ragged, mk, ov):
    ex = V.row_expected(name, ragged, mk, ov)
    return np.concatenate(ex), np.array([len(e) for e in ex], dtype=np.uint64)


@pytest.mark.parametrize("name", V.VERIFY_SETS)
def test_uniform_batch_from_device_memory(dev, name):
    rs = V.rows(name, False)
    blob = b"".join(r.data for r in rs)
    ptr = dev.put(blob)
    for mk, ov in V.KINDS:
        want, want_counts = batch_expected(name, False, mk, ov)
        got, counts, st = find_device(handle(name, mk), ptr, len(blob), ov, n_hay=len(rs), uniform_len=V.row_len(name))
        same_rows(got, want, (name, "uniform", mk, ov))
        assert np.array_equal(counts, want_counts) and st["k0"] == 0, (name, mk, ov, sorted(st.items()))


@pytest.mark.parametrize("lead", [0, 7])
@pytest.mark.parametrize("name", V.VERIFY_SETS)
def test_ragged_batch_from_device_memory(dev, name, lead):
    rs = V.rows(name, True)
    offs = V.offsets_of(rs)
    blob = b"".join(r.data for r in rs)
    ptr = dev.put(blob, lead)
    d_offs = capi.DeviceBuffer(8 * len(offs)).upload(np.array(offs, dtype=np.uint64))
    for mk, ov in V.KINDS:
        want, want_counts = batch_expected(name, True, mk, ov)
        got, counts, st = find_device(handle(name, mk), ptr, len(blob), ov, d_offsets=d_offs.ptr, n_hay=len(rs))
        same_rows(got, want, (name, "ragged", lead, mk, ov))
        assert np.array_equal(counts, want_counts) and st["k0"] == 0, (name, mk, ov, sorted(st.items()))
    d_offs.free()


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
@pytest.mark.parametrize("name", V.VERIFY_SETS)
def test_batch_from_host_memory(name, ragged):
    rs = V.rows(name, ragged)
    for mk, ov in V.KINDS:
        want, want_counts = batch_expected(name, ragged, mk, ov)
        m, counts = handle(name, mk).find_batch([r.data for r in rs], overlapping=ov)
        same_rows(cols(m), want, (name, "host batch", ragged, mk, ov))
        assert np.array_equal(counts, want_counts), (name, ragged, mk, ov)


# ---------------------------------------------------------------------------
# verify cases: code points (all bytes are ASCII: the byte rows ARE the code points)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["urls", "q5"])
def test_code_points(dev, name):
    """k_tile_main<CP>: the window at the START of an anchored occurrence is handed over (sw0 / sw1)"""
    c = V.case(name)
    assert int(c.hay.max()) < 0x80
    ptr = dev.put(c.hay)
    check_every_kind(name, ptr, c.hay, lambda mk, ov: V.expected(name, mk, ov), lambda st: st["sparse"] == 1 and st["k0"] == 0,
                     "code points", codepoints=True)
    rs = V.rows(name, False)
    blob = b"".join(r.data for r in rs)
    ptr = dev.put(blob)
    for mk, ov in V.KINDS:
        want, _ = batch_expected(name, False, mk, ov)
        got, _, _ = find_device(handle(name, mk), ptr, len(blob), ov, n_hay=len(rs), uniform_len=V.row_len(name), codepoints=True)
        same_rows(got, want, (name, "code points, batch", mk, ov))


# ---------------------------------------------------------------------------
# packed-word cases
# ---------------------------------------------------------------------------
def packed_want(name, hay):
    return lambda mk, ov: V.packed_oracle(name, mk).find_raw(np.ascontiguousarray(hay), overlapping=ov)


def run_packed(names, dev=None) -> None:
    """every kind on the sparse path, K1b's hits (the form: tile_words_narrow()) -- also run in processes of their own"""
    own = dev is None
    dev = dev or Device()
    for name in names:
        c = V.packed_case(name)
        ptr = dev.put(c.hay)
        check_every_kind(name, ptr, c.hay, packed_want(name, c.hay),
                         lambda st: st["sparse"] >= 1 and st["hot_calls"] == st["dense_tiles"] == st["dense_radix"] == 0, "packed")
    if own:
        for a in _HANDLES.values():
            a.close()
        _HANDLES.clear()
        dev.buf.free()


@pytest.mark.parametrize("name", PACKED)
def test_packed_words_on_the_sparse_path(dev, name):
    r = V.packed_row(name)
    assert handle(name, 2).info.max_pattern_len == r.max_len and handle(name, 2).info.n_patterns == r.n
    run_packed([name], dev)
    # the kernel the library picks by itself, host memory
    c = V.packed_case(name)
    for mk, ov in V.KINDS:
        a = handle(name, mk, forced=False)
        a.path_stats(reset=True)
        same_rows(cols(a.find(c.hay, overlapping=ov)), packed_want(name, c.hay)(mk, ov), (name, "host", mk, ov))
        st = a.path_stats()
        assert st["sparse"] >= 1 and st["hot_calls"] == st["dense_tiles"] == st["dense_radix"] == 0, (name, mk, ov, sorted(st.items()))


def in_a_process_with(env: str, names) -> None:
    code = ("import os, sys; sys.path[:0] = [os.environ['ACX_ROOT'], os.path.join(os.environ['ACX_ROOT'], 'tests')]; "
            "import test_gpu_verify_seams as T; T.run_packed(sys.argv[1:]); print('OK')")
    r = subprocess.run([sys.executable, "-c", code] + list(names), env={**os.environ, env: "1", "ACX_ROOT": ROOT},
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, (env, r.stdout[-2000:], r.stderr[-3000:])


def test_narrow_rows_with_wide_words():
    """ACX_MAIN_WIDE (read once per process) makes tile_words_narrow() say no: the rows that fit W32_FIELD are staged and
    decoded as 64-bit words [rel : 19 | tie | length].  path_stats does not show the form; verify_seams.source_constants()
    checks that the sources still read the switch by this name, in that function"""
    assert len(NARROW) == 5 and "ACX_MAIN_WIDE" not in os.environ and V.C["W32_FIELD"] == 20
    in_a_process_with("ACX_MAIN_WIDE", NARROW)


def test_every_row_with_the_wide_post_stage():
    """ACX_FORCE_WIDE (read once per process) selects the wide form of the POST STAGE for every K1b call -- GROUP_MAX_WIDE
    matches a group, 64 staged occurrences a bucket --, not the width of the words: the narrow rows still run the 32-bit
    words, in the kernel's other instantiation (its flags are 64-bit masks), the wide rows the 64-bit words.
    verify_seams.source_constants() checks that attempt_sparse() still reads the switch by this name"""
    assert len(PACKED) == 8 and "ACX_FORCE_WIDE" not in os.environ
    in_a_process_with("ACX_FORCE_WIDE", PACKED)


@pytest.mark.parametrize("name", PACKED)
def test_packed_words_on_the_dense_tile_path(dev, monkeypatch, name):
    """k_dense_main's words [rel : 12 | tie | length] on the tile-ordered dense path, and on no other: the plants lie where
    that form can certify a sync point for every group (verify_seams.dense_placements())"""
    c = V.packed_dense_case(name)
    ptr = dev.put(c.hay)
    monkeypatch.setenv("ACX_NO_BUCKET", "1")
    check_every_kind(name, ptr, c.hay, packed_want(name, c.hay),
                     lambda st: st["sparse"] == st["hot_calls"] == st["dense_radix"] == 0 and st["dense_tiles"] >= 1, "dense tiles")


@pytest.mark.parametrize("name", PACKED)
def test_packed_words_on_the_radix_path(dev, monkeypatch, name):
    """the sparse path's own haystack, every placement ("end first" of the longest pattern too), through the form that
    resolves globally: occurrence records, no packed word"""
    c = V.packed_case(name)
    ptr = dev.put(c.hay)
    monkeypatch.setenv("ACX_NO_BUCKET", "1")
    monkeypatch.setenv("ACX_NO_DENSE_TILES", "1")
    check_every_kind(name, ptr, c.hay, packed_want(name, c.hay),
                     lambda st: st["sparse"] == st["hot_calls"] == st["dense_tiles"] == 0 and st["dense_radix"] >= 1, "radix")


@pytest.mark.parametrize("name", PACKED)
def test_packed_words_in_hot_groups(dev, name):
    """the 48-bit repack of k_hot_verify and k_dense_main's words, spliced with the sparse groups' by k_tile_write"""
    h = V.packed_hot_hay(name)
    ptr = dev.put(h)
    check_every_kind(name, ptr, h, packed_want(name, h),
                     lambda st: st["hot_calls"] >= 1 and st["dense_tiles"] == st["dense_radix"] == 0, "hot")


@pytest.mark.parametrize("name", ["pw65x8191", "pw65x8192", "pw16385x31", "pw16385x32"])
def test_packed_words_with_code_points(dev, name):
    """CP_BITS above the length: always the wide form"""
    c = V.packed_case(name)
    ptr = dev.put(c.hay)
    check_every_kind(name, ptr, c.hay, packed_want(name, c.hay),
                     lambda st: st["sparse"] >= 1 and st["hot_calls"] == st["dense_tiles"] == st["dense_radix"] == 0, "code points",
                     codepoints=True)
