"""Whole-word matching on the device (acx_words_rows_device, acx_find_words / _device, acx_filter_words / _device;
find_whole_words_as_columns / _batch, filter_whole_words_batch): the stage alone on uploaded records at the seams of its
tile -- record counts around the tile, the three row cuts, all and none surviving, clusters across a tile boundary, one chain
cluster of about 5 000 records, touching matches, a misaligned haystack -- with guard words around its outputs; the full
routes from host memory and from HBM against brute force and `re`; the cross-check of the resolve against the leftmost
handles' own finds; a case-insensitive handle; the Python classes.  Expected values come from Python (str.find over the
patterns and the definition restated below), never from the library."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
capi = pytest.importorskip("ahocorasick_rs_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ahocorasick_rs_amd", "csrc")

STD, LF, LL = capi.MATCH_STANDARD, capi.MATCH_LEFTMOST_FIRST, capi.MATCH_LEFTMOST_LONGEST
MODES = [("overlapping", True, STD), ("standard", False, STD), ("first", False, LF), ("longest", False, LL)]
DEFAULT = capi.ASCII_WORD_BYTES
ALL_BYTES = bytes(range(256))
GUARD = 0xC3
T = int(re.search(r"\bWORDS_TILE\s*=\s*(\d+)\s*;", open(os.path.join(CSRC, "words.hpp")).read()).group(1))


# ---------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------
def occurrences(row: bytes, patterns):
    """every (p, s, e) with row[s:e] == patterns[p], in the overlapping find's order: end ascending, longer first, pattern"""
    occ = []
    for p, pat in enumerate(patterns):
        s = row.find(pat)
        while s >= 0:
            occ.append((p, s, s + len(pat)))
            s = row.find(pat, s + 1)
    return sorted(occ, key=lambda r: (r[2], r[1], r[0]))


KEYS = {STD: lambda r: (r[2], r[1], r[0]), LF: lambda r: (r[1], r[0]), LL: lambda r: (r[1], -r[2], r[0])}


def brute(row, occ, overlapping, kind, word_bytes):
    """the issue's definition, word for word: among the whole-word records with s >= pos the least by key"""
    W = set(DEFAULT if word_bytes is None else bytes(word_bytes))
    ww = [(p, s, e) for p, s, e in occ if (s == 0 or row[s - 1] not in W) and (e == len(row) or row[e] not in W)]
    if overlapping:
        return ww
    out, pos = [], 0
    while True:
        live = [r for r in ww if r[1] >= pos]
        if not live:
            return out
        out.append(min(live, key=KEYS[kind]))
        pos = out[-1][2]


def definition(row, occ, overlapping, kind, word_bytes):
    """the same in one walk over the records sorted by key (the least record with s >= pos is the first such one: pos only
    grows), for rows of thousands of records"""
    W = set(DEFAULT if word_bytes is None else bytes(word_bytes))
    ww = [(p, s, e) for p, s, e in occ if (s == 0 or row[s - 1] not in W) and (e == len(row) or row[e] not in W)]
    if overlapping:
        return ww
    out, pos = [], 0
    for r in sorted(ww, key=KEYS[kind]):
        if r[1] >= pos:
            out.append(r)
            pos = r[2]
    return out


def random_rows(rng, n_rows, longest=40, alphabet=b"ab_ .-", fixed=None):
    rows = []
    for _ in range(n_rows):
        k = fixed if fixed is not None else (0 if rng.random() < 0.15 else int(rng.integers(0, longest + 1)))
        rows.append(bytes(alphabet[int(i)] for i in rng.integers(0, len(alphabet), k)))
    return rows


def random_patterns(rng, alphabet=b"ab_ .-"):
    return [bytes(alphabet[int(i)] for i in rng.integers(0, len(alphabet), int(rng.integers(1, 5)))) for _ in range(int(rng.integers(1, 7)))]


def test_the_two_forms_of_the_definition_agree():
    rng = np.random.default_rng(3)
    for _ in range(200):
        rows, pats = random_rows(rng, 3), random_patterns(rng)
        for row in rows:
            occ = occurrences(row, pats)
            for _, ov, kind in MODES:
                for wb in (None, b"", b"ab"):
                    assert definition(row, occ, ov, kind, wb) == brute(row, occ, ov, kind, wb), (row, pats, kind, wb)


# ---------------------------------------------------------------------------
# the stage alone
# ---------------------------------------------------------------------------
def run_stage(rows, occ_rows, overlapping, kind, word_bytes, cut="offsets", misalign=0):
    """words_rows_device on uploaded records: the bytes at an address `misalign` beyond an aligned one, the record output
    between guard bytes -> (records, counts); the guards, the records behind the survivors and every input checked unwritten"""
    hay = b"".join(rows)
    rec = np.ascontiguousarray(np.asarray([r for o in occ_rows for r in o], dtype=np.uint64).reshape(-1, 3))
    counts = np.asarray([len(o) for o in occ_rows], dtype=np.uint64)
    n, n_hay = len(rec), len(rows)
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
    bufs = []

    def dev(arr, extra=16):
        b = capi.DeviceBuffer(arr.nbytes + extra)
        bufs.append(b)
        if arr.nbytes:
            b.upload(arr)
        return b

    try:
        h_img = np.frombuffer(b"\xAA" * misalign + hay + b"wwww", dtype=np.uint8)  # (word bytes behind the batch: never a neighbour)
        d_hay = dev(h_img)
        d_rec, d_cnt, d_off = dev(rec.reshape(-1)), dev(counts), dev(off)
        out_img = np.full(64 + 24 * n + 64, GUARD, dtype=np.uint8)
        cnt_img = np.full(64 + 8 * n_hay + 64, GUARD, dtype=np.uint8)
        d_out, d_oc = dev(out_img), dev(cnt_img)
        uniform = len(rows[0]) if cut == "uniform" else 0
        kept = capi.words_rows_device(d_hay.ptr + misalign, len(hay), d_off.ptr if cut == "offsets" else 0, n_hay if cut != "single" else 0,
                                      uniform, d_rec.ptr if n else 0, n, d_cnt.ptr, overlapping, kind, word_bytes, d_out.ptr + 64,
                                      d_oc.ptr + 64)
        got, got_c = d_out.download(len(out_img)), d_oc.download(len(cnt_img))
        assert np.array_equal(d_rec.download(24 * n), rec.reshape(-1).view(np.uint8)), "the records were written"
        assert np.array_equal(d_cnt.download(8 * n_hay).view(np.uint64), counts), "the counts were written"
        assert np.array_equal(d_hay.download(len(h_img)), h_img), "the haystack was written"
    finally:
        for b in bufs:
            b.free()
    assert 0 <= kept <= n
    assert (got[:64] == GUARD).all() and (got[64 + 24 * kept:] == GUARD).all(), "a byte outside the surviving records was written"
    assert (got_c[:64] == GUARD).all() and (got_c[64 + 8 * n_hay:] == GUARD).all(), "a guard byte of the counts was written"
    recs = got[64:64 + 24 * kept].view(np.uint64).reshape(-1, 3)
    return [tuple(int(x) for x in r) for r in recs.tolist()], got_c[64:64 + 8 * n_hay].view(np.uint64).tolist()


def check_stage(rows, occ_rows, word_bytes=None, cut="offsets", misalign=0, what=None, modes=MODES):
    for name, overlapping, kind in modes:
        want = [definition(r, o, overlapping, kind, word_bytes) for r, o in zip(rows, occ_rows)]
        got, counts = run_stage(rows, occ_rows, overlapping, kind, word_bytes, cut, misalign)
        flat = [r for w in want for r in w]
        if got != flat or counts != [len(w) for w in want]:
            bad = next((i for i, (a, b) in enumerate(zip(got, flat)) if a != b), min(len(got), len(flat)))
            raise AssertionError((what, name, cut, "records", len(got), "wanted", len(flat), "first difference at", bad,
                                  got[max(bad - 2, 0):bad + 3], flat[max(bad - 2, 0):bad + 3], counts[:8], [len(w) for w in want][:8]))


def trimmed(rows, pats, n):
    """the rows' occurrences, cut behind the first n of them (the stage takes the records as they come)"""
    occ_rows, left = [], n
    for row in rows:
        o = occurrences(row, pats)[:left]
        left -= len(o)
        occ_rows.append(o)
    assert left == 0, "the rows hold fewer occurrences than the case wants"
    return occ_rows


@pytest.mark.parametrize("n", [0, 1, T - 1, T, T + 1, 2 * T + 1])
def test_stage_record_counts_around_the_tile_in_every_cut(n):
    rng = np.random.default_rng(100 + n)
    pats = [b"a", b"ab", b"b ", b"a a", b"_"]
    rows = random_rows(rng, 30 + n // 3)
    rows[0], rows[5] = b"", b""
    check_stage(rows, trimmed(rows, pats, n), None, "offsets", what=("ragged", n))
    check_stage(rows, trimmed(rows, pats, n), b"", "offsets", what=("all survive", n))
    rows = random_rows(rng, 4 + n // 5, fixed=24)
    check_stage(rows, trimmed(rows, pats, n), None, "uniform", what=("uniform", n))
    row = [b"".join(random_rows(rng, 2 + n // 3, fixed=12))]
    check_stage(row, trimmed(row, pats, n), None, "single", what=("one row", n))
    # none survive: every byte is a word byte and no occurrence is its whole row
    rows = [b"." + r + b"." for r in random_rows(rng, 30 + n // 3)]
    got = run_stage(rows, trimmed(rows, pats, n), True, STD, ALL_BYTES)
    assert got == ([], [0] * len(rows))
    got = run_stage(rows, trimmed(rows, pats, n), False, LL, ALL_BYTES)
    assert got == ([], [0] * len(rows))


def test_stage_a_cluster_across_a_tile_boundary():
    pats = [b"x", b"a a", b"a a a"]
    for lead in (T - 11, T - 1, T):  # the chain's records begin at this record index
        rows = [b" ".join([b"x"] * lead), b" ".join([b"a"] * 20), b"x a a x"]
        occ = [occurrences(r, pats) for r in rows]
        assert len(occ[0]) == lead and len(occ[1]) == 19 + 18
        check_stage(rows, occ, None, what=("cluster at", lead))
        one = [b" ".join(rows)]
        check_stage(one, [occurrences(one[0], pats)], None, "single", what=("cluster in one row at", lead))


def test_stage_one_chain_cluster_of_five_thousand_records():
    pats = [b"a a", b"a a a"]
    row = b" ".join([b"a"] * 2502)
    occ = occurrences(row, pats)
    assert len(occ) == 2501 + 2500
    rows = [b"a a", row, b"", b"a a a a"]
    occ_rows = [occurrences(r, pats) for r in rows]
    check_stage(rows, occ_rows, None, what="chain")
    want = definition(row, occ, False, LL, None)
    assert len(want) == 834 and want[0] == (1, 0, 5) and want[1] == (1, 6, 11)  # (the greedy walks all of it)
    check_stage([row], [occ], None, "single", what="chain alone")


def test_stage_touching_matches_and_a_misaligned_haystack():
    pats = [b"ab", b"cd", b"abcd", b"b"]
    rows = [b"abcdab", b"ab cd", b"cdcd"]
    occ = [occurrences(r, pats) for r in rows]
    check_stage(rows, occ, b"", what="touching, every occurrence whole")
    assert run_stage(rows, occ, False, LF, b"")[0][:3] == [(0, 0, 2), (1, 2, 4), (0, 4, 6)]
    assert run_stage(rows, occ, False, LL, b"")[0][:2] == [(2, 0, 4), (0, 4, 6)]
    rng = np.random.default_rng(5)
    rows = random_rows(rng, 40)
    rp = random_patterns(rng)
    occ = [occurrences(r, rp) for r in rows]
    for misalign in (1, 3, 7):
        check_stage(rows, occ, None, misalign=misalign, what=("misaligned", misalign))
    big = [b"".join(rows)]
    check_stage(big, [occurrences(big[0], rp)], b"_", "single", misalign=5, what="misaligned, one row")


def test_stage_refusals():
    rows, pats = [b"a a", b"a"], [b"a"]
    occ = [occurrences(r, pats) for r in rows]
    with pytest.raises(ValueError) as e:
        run_stage(rows, occ, False, 7, None)
    assert e.value.code == capi.EINVAL
    # counts that do not sum to the records: refused before a kernel reads a record by them
    rec = np.asarray([(0, 0, 1), (0, 2, 3), (0, 0, 1)], dtype=np.uint64)
    bufs = [capi.DeviceBuffer(256).upload(x) for x in (np.frombuffer(b"a aa", dtype=np.uint8), rec.reshape(-1),
                                                      np.asarray([1, 1], dtype=np.uint64), np.asarray([0, 3, 4], dtype=np.uint64))]
    out, oc = capi.DeviceBuffer(256), capi.DeviceBuffer(256)
    try:
        with pytest.raises(ValueError) as e:
            capi.words_rows_device(bufs[0].ptr, 4, bufs[3].ptr, 2, 0, bufs[1].ptr, 3, bufs[2].ptr, False, LL, None, out.ptr, oc.ptr)
        assert e.value.code == capi.EINVAL and "sum" in str(e.value)
        with pytest.raises(ValueError) as e:  # a misaligned record pointer
            capi.words_rows_device(bufs[0].ptr, 4, bufs[3].ptr, 2, 0, bufs[1].ptr + 4, 2, bufs[2].ptr, False, LL, None, out.ptr, oc.ptr)
        assert e.value.code == capi.EINVAL
    finally:
        for x in bufs + [out, oc]:
            x.free()
    # a pattern that does not fit the leftmost kinds' key
    with pytest.raises(ValueError) as e:
        run_stage([b"a"], [[(1 << 24, 0, 1)]], False, LF, None)
    assert e.value.code == capi.ETOOBIG
    assert run_stage([b"a"], [[(1 << 24, 0, 1)]], True, STD, None) == ([(1 << 24, 0, 1)], [1])


# ---------------------------------------------------------------------------
# the full routes through the C ABI
# ---------------------------------------------------------------------------
def columns(c):
    """a DeviceColumns as (records, counts or None)"""
    recs = list(zip(c.pattern().tolist(), c.start().tolist(), c.end().tolist()))
    ro = c.row_offsets()
    return recs, (None if ro is None else np.diff(ro).tolist())


def find_words_device(a, rows, overlapping, kind, word_bytes, cut="offsets"):
    hay = np.frombuffer(b"".join(rows) + b"\0", dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
    d_hay, d_off = capi.DeviceBuffer(hay.nbytes + 16).upload(hay), capi.DeviceBuffer(off.nbytes + 16).upload(off)
    try:
        kw = {"offsets": dict(d_offsets=d_off.ptr, n_hay=len(rows)), "uniform": dict(n_hay=len(rows), uniform_len=len(rows[0])),
              "single": {}}[cut]
        c = a.find_words_device(d_hay.ptr, len(hay) - 1, overlapping=overlapping, match_kind=kind, word_bytes=word_bytes, **kw)
        assert c.on_device
        out = columns(c)
        c.free()
        return out
    finally:
        d_hay.free()
        d_off.free()


@pytest.mark.parametrize("route", ["host", "staged", "device"])
def test_routes_against_brute_force_and_re(route, monkeypatch):
    if route == "staged":
        monkeypatch.setenv("ACX_WORDS_HOST_MAX", "0")  # host haystacks, the device route
    rng = np.random.default_rng(42)
    for rep in range(6):
        rows, pats = random_rows(rng, [1, 2, 7, 64, 301, 40][rep], alphabet=b"ab_ .-9"), list(dict.fromkeys(random_patterns(rng, b"ab_ .-9")))
        a = capi.Automaton(pats, STD)
        rx = re.compile(rb"(?<!\w)(?:" + b"|".join(re.escape(p) for p in pats) + rb")(?!\w)")
        for name, overlapping, kind in MODES:
            for wb in (None, b"ab9"):
                want = [brute(r, occurrences(r, pats), overlapping, kind, wb) for r in rows]
                if route == "device":
                    got = find_words_device(a, rows, overlapping, kind, wb)
                else:
                    c = a.find_words(rows, overlapping, kind, wb)
                    assert not c.on_device
                    got = columns(c)
                    c.free()
                assert got == ([r for w in want for r in w], [len(w) for w in want]), (route, name, wb, rep, pats)
                if kind == LF and not overlapping and wb is None:
                    assert [(s, e) for _, s, e in got[0]] == [(m.start(), m.end()) for r in rows for m in rx.finditer(r)]
        # one haystack that is no batch
        row = b" ".join(rows[:5])
        want = brute(row, occurrences(row, pats), False, LL, None)
        if route == "device":
            assert find_words_device(a, [row], False, LL, None, "single") == (want, None)
        else:
            c = a.find_words(None, False, LL, None, single=row)
            assert columns(c) == (want, None)
            c.free()
        a.close()


def test_the_resolve_equals_the_leftmost_handles_own_finds():
    """W empty: every occurrence is whole, and the stage's resolve must give what a handle of that kind finds -- the
    cross-check against the oracle-tested pipeline"""
    rng = np.random.default_rng(9)
    pats = list(dict.fromkeys(random_patterns(rng) + random_patterns(rng) + [b"ab", b"abab", b"b"]))
    rows = random_rows(rng, 300, longest=60)
    std = capi.Automaton(pats, STD)
    for kind in (STD, LF, LL):
        own = capi.Automaton(pats, kind)
        c = own.find_columns_batch(rows)
        want = columns(c)
        c.free()
        own.close()
        assert find_words_device(std, rows, False, kind, b"") == want, kind
        c = std.find_words(rows, False, kind, b"")
        assert columns(c) == want, kind
        c.free()
    c = std.find_columns_batch(rows, overlapping=True)
    assert find_words_device(std, rows, True, STD, b"") == columns(c)
    c.free()
    std.close()


def test_a_case_insensitive_handle_tests_the_callers_bytes():
    a = capi.Automaton([b"cat"], STD, ascii_case_insensitive=True)
    rows = [b"xCATx XcatX", b"Xcatx xCATX cat"]
    upper, lower = bytes(range(65, 91)), bytes(range(97, 123))
    # A-Z are word bytes, a-z are not: the neighbours x bound a match, the neighbours X do not -- on the UNFOLDED bytes
    want_u = ([(0, 1, 4), (0, 12, 15)], [1, 1])
    want_l = ([(0, 7, 10), (0, 12, 15)], [1, 1])
    for find in (lambda wb: find_words_device(a, rows, False, LL, wb), lambda wb: columns(a.find_words(rows, False, LL, wb))):
        assert find(upper) == want_u
        assert find(lower) == want_l
    f = a.filter_words(rows, False, LL, upper, 1, capi.FILTER_KEEP_MATCHED)
    assert f.data().tobytes() == b"".join(rows)  # (the caller's bytes, not the folded ones)
    f.free()
    a.close()


def test_non_standard_handles_and_bad_kinds_are_refused():
    for kind in (LF, LL):
        a = capi.Automaton([b"a"], kind)
        for call in (lambda: a.find_words([b"a"]), lambda: a.filter_words([b"a"]), lambda: a.find_words_device(0, 0),
                     lambda: a.filter_words_device(0, 0)):
            with pytest.raises(ValueError) as e:
                call()
            assert e.value.code == capi.EOVERLAP
        a.close()
    a = capi.Automaton([b"a"], STD)
    for call in (lambda: a.find_words([b"a"], False, 3), lambda: a.filter_words([b"a"], False, -1), lambda: a.find_words_device(0, 0, match_kind=9)):
        with pytest.raises(ValueError) as e:
            call()
        assert e.value.code == capi.EINVAL
    a.close()


def test_filter_words_through_the_c_abi_host_and_device():
    a = capi.Automaton([b"ass"], STD)
    rows = [b"class act", b"an ass", b"ass", b"passes", b"ass ass"]
    hay = np.frombuffer(b"".join(rows) + b"\0", dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
    d_hay, d_off = capi.DeviceBuffer(hay.nbytes + 16).upload(hay), capi.DeviceBuffer(off.nbytes + 16).upload(off)
    try:
        for flags, mm, want in ((0, 1, [0, 3]), (capi.FILTER_KEEP_MATCHED, 1, [1, 2, 4]), (capi.FILTER_KEEP_MATCHED, 2, [4]), (0, 2, [0, 1, 2, 3])):
            for f in (a.filter_words(rows, False, LL, None, mm, flags),
                      a.filter_words_device(d_hay.ptr, len(hay) - 1, d_offsets=d_off.ptr, n_hay=len(rows), min_matches=mm, flags=flags)):
                assert f.rows().tolist() == want, (flags, mm)
                assert f.data().tobytes() == b"".join(rows[i] for i in want)
                f.free()
    finally:
        d_hay.free()
        d_off.free()
    a.close()


# ---------------------------------------------------------------------------
# the Python classes
# ---------------------------------------------------------------------------
def test_python_sequences_both_classes():
    import ahocorasick_rs as ar
    rows = [b"the cat", b"cat he cat", b"", b"concat cat."]
    pats = [b"he cat", b"cat"]
    b = ar.BytesAhoCorasick(pats)
    t = ar.AhoCorasick([p.decode() for p in pats])
    for name, overlapping, kind in MODES:
        mk = {STD: ar.MatchKind.Standard, LF: ar.MatchKind.LeftmostFirst, LL: ar.MatchKind.LeftmostLongest}[kind]
        want = [brute(r, occurrences(r, pats), overlapping, kind, None) for r in rows]
        assert b.find_whole_words_as_columns_batch(rows, overlapping, matchkind=mk).tolist() == want, name
        assert t.find_whole_words_as_columns_batch([r.decode() for r in rows], overlapping, matchkind=mk).tolist() == want, name
        for r, w in zip(rows, want):
            assert b.find_whole_words_as_columns(r, overlapping, matchkind=mk).tolist() == w
            assert t.find_whole_words_as_columns(r.decode(), overlapping, matchkind=mk).tolist() == w
    assert b.find_whole_words_as_columns(b"the cat").tolist() == [(1, 4, 7)]
    assert b.find_whole_words_as_columns(b"the cat", word_bytes=b"").tolist() == [(0, 1, 7)]
    assert b.find_whole_words_as_columns(b"the cat", word_bytes=bytearray(b"xx")).tolist() == [(0, 1, 7)]  # (`t` is no word byte now: he cat is whole)
    assert b.find_whole_words_as_columns(b"the cat", word_bytes=memoryview(b"tt")).tolist() == [(1, 4, 7)]
    assert b.find_whole_words_as_columns(b"the cat", word_bytes=ar.ASCII_WORD_BYTES).tolist() == [(1, 4, 7)]


def test_python_str_gives_character_indexes():
    import ahocorasick_rs as ar
    t = ar.AhoCorasick(["cat", "né", "€"])
    text = "é€ cat, ñcat cat€ né é né"
    #       0123456789...
    want = [(m.start(), m.end()) for m in re.finditer(r"(?<![0-9A-Za-z_])(?:cat|né|€)(?![0-9A-Za-z_])", text)]
    got = t.find_whole_words_as_columns(text, matchkind=ar.MatchKind.LeftmostFirst).tolist()
    # (non-ASCII bytes are no word bytes by default: `ñcat` has a whole `cat`, `é€` a whole `€`, and in `cat€` the `cat` is whole, the `€` behind a `t` is not)
    assert [(s, e) for _, s, e in got] == want and [text[s:e] for _, s, e in got] == ["€", "cat", "cat", "cat", "né", "né"]
    rows = [text, "", "cat", "ünicat €"]
    got = t.find_whole_words_as_columns_batch(rows, matchkind=ar.MatchKind.LeftmostFirst).tolist()
    assert [[(s, e) for _, s, e in r] for r in got] == \
        [[(m.start(), m.end()) for m in re.finditer(r"(?<![0-9A-Za-z_])(?:cat|né|€)(?![0-9A-Za-z_])", r)] for r in rows]
    # every byte beyond ASCII counts as a word byte: the caller's way to a wider word class
    wide = ar.ASCII_WORD_BYTES + bytes(range(128, 256))
    got = t.find_whole_words_as_columns(text, matchkind=ar.MatchKind.LeftmostFirst, word_bytes=wide).tolist()
    assert [(text[s:e], s) for _, s, e in got] == [("cat", 3), ("né", 18), ("né", 23)]


def test_python_filter_and_errors():
    import ahocorasick_rs as ar
    rows = [b"class act", b"an ass", b"ass", b"passes"]
    for cls, conv in ((ar.BytesAhoCorasick, lambda x: x), (ar.AhoCorasick, lambda x: x.decode())):
        o = cls([conv(b"ass")])
        hs = [conv(r) for r in rows]
        f = o.filter_whole_words_batch(hs)
        assert f.tolist() == [hs[0], hs[3]] and np.from_dlpack(f.rows).tolist() == [0, 3] and f.source_rows == 4
        assert bytes(memoryview(f.data)) == rows[0] + rows[3]  # (the caller's bytes)
        f = o.filter_whole_words_batch(hs, keep="matched")
        assert f.tolist() == [hs[1], hs[2]] and np.from_dlpack(f.rows).tolist() == [1, 2]
        assert o.filter_whole_words_batch(hs, keep="matched", min_matches=2).tolist() == []
        assert o.filter_whole_words_batch(hs + [conv(b"ass, ass")], True, keep="matched", min_matches=2).tolist() == [conv(b"ass, ass")]
        assert o.filter_batch(hs).tolist() == []  # (by substring every row goes)
        for bad in ("ab", 7, [1, 2]):
            with pytest.raises(TypeError):
                o.find_whole_words_as_columns(hs[0], word_bytes=bad)
            with pytest.raises(TypeError):
                o.filter_whole_words_batch(hs, word_bytes=bad)
        for bad in (0, "LeftmostFirst", None, True):
            with pytest.raises(TypeError):
                o.find_whole_words_as_columns(hs[0], matchkind=bad)
            with pytest.raises(TypeError):
                o.find_whole_words_as_columns_batch(hs, matchkind=bad)
        with pytest.raises(TypeError):
            o.find_whole_words_as_columns(hs[0], 1)
        with pytest.raises(ValueError):
            o.filter_whole_words_batch(hs, min_matches=0)
        for mk in (ar.MatchKind.LeftmostFirst, ar.MatchKind.LeftmostLongest):
            lm = cls([conv(b"ass")], matchkind=mk)
            for call in (lambda: lm.find_whole_words_as_columns(hs[0]), lambda: lm.find_whole_words_as_columns_batch(hs),
                         lambda: lm.filter_whole_words_batch(hs)):
                with pytest.raises(ValueError):
                    call()
            with pytest.raises(ValueError):
                lm.find_matches_as_indexes(hs[0], overlapping=True)  # (the same refusal)


_TENSOR_SCRIPT = r"""
import re
import sys
import torch  # first: one process holds ONE HIP runtime, and torch must be the one to load it
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
import ahocorasick_rs as ar
from test_gpu_words import brute, definition, occurrences, random_rows, STD, LF, LL

rng = np.random.default_rng(77)
pats = [b"cat", b"he cat", b"a", b"a a", b"at"]
rows = random_rows(rng, 400, longest=50, alphabet=b"cat he_.")
rows[3] = b""
L = 32
uni = random_rows(rng, 300, fixed=L, alphabet=b"cat he_.")
b = ar.BytesAhoCorasick(pats)
t = ar.AhoCorasick([p.decode() for p in pats])
kinds = {STD: ar.MatchKind.Standard, LF: ar.MatchKind.LeftmostFirst, LL: ar.MatchKind.LeftmostLongest}
dev = torch.from_numpy(np.frombuffer(b"".join(rows), dtype=np.uint8).copy()).to("cuda:0")
off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)).to("cuda:0")
udev = torch.from_numpy(np.frombuffer(b"".join(uni), dtype=np.uint8).copy()).to("cuda:0")

def as_rows(mc):
    p, s, e, ro = (torch.from_dlpack(c).cpu().tolist() for c in (mc.pattern, mc.start, mc.end, mc.row_offsets))
    return [list(zip(p[a:z], s[a:z], e[a:z])) for a, z in zip(ro, ro[1:])]

for ov, kind in ((True, STD), (False, STD), (False, LF), (False, LL)):
    for wb in (None, b"ca_"):
        want = [brute(r, occurrences(r, pats), ov, kind, wb) for r in rows]
        wantu = [brute(r, occurrences(r, pats), ov, kind, wb) for r in uni]
        for o in (b, t):  # the str class on a tensor: byte offsets local to the row
            mc = o.find_whole_words_as_columns_batch(dev, ov, matchkind=kinds[kind], word_bytes=wb, offsets=off)
            assert mc.device == 0 and as_rows(mc) == want, (ov, kind, wb)
            mc = o.find_whole_words_as_columns_batch(udev, ov, matchkind=kinds[kind], word_bytes=wb, row_length=L)
            assert mc.device == 0 and as_rows(mc) == wantu, (ov, kind, wb)
        mc = b.find_whole_words_as_columns_batch(torch.from_numpy(np.frombuffer(b"".join(uni), dtype=np.uint8).copy()), ov, matchkind=kinds[kind], word_bytes=wb, row_length=L)
        assert mc.device is None and as_rows(mc) == wantu
        one = b.find_whole_words_as_columns(dev, ov, matchkind=kinds[kind], word_bytes=wb)
        big = b"".join(rows)
        assert one.device == 0 and one.tolist() == definition(big, occurrences(big, pats), ov, kind, wb)
# multi-byte characters in front of a match: a tensor gives byte offsets
text = "é€ cat".encode()
tt = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to("cuda:0")
assert t.find_whole_words_as_columns_batch(tt, row_length=len(text)).tolist() == [[(0, 6, 9)]]
assert t.find_whole_words_as_columns(text.decode()).tolist() == [(0, 3, 6)]
# the filter on a tensor: the caller's bytes, where they lie
ass = ar.BytesAhoCorasick([b"ass"])
fr = [b"class act", b"an ass", b"ass", b"passes"]
ft = torch.from_numpy(np.frombuffer(b"".join(fr), dtype=np.uint8).copy()).to("cuda:0")
fo = torch.tensor([0, 9, 15, 18, 24], dtype=torch.int64, device="cuda:0")
for keep, mm, want in (("unmatched", 1, [0, 3]), ("matched", 1, [1, 2]), ("matched", 2, [])):
    f = ass.filter_whole_words_batch(ft, keep=keep, min_matches=mm, offsets=fo)
    assert f.device == 0 and torch.from_dlpack(f.rows).cpu().tolist() == want
    assert bytes(torch.from_dlpack(f.data).cpu().numpy()) == b"".join(fr[i] for i in want)
print("OK")
"""


def test_python_tensors_in_hbm():
    p = subprocess.run([sys.executable, "-c", _TENSOR_SCRIPT, ROOT, os.path.join(ROOT, "tests")], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
