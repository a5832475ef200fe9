"""CPU checks of the merged spans of a search's matches (acx_spans_host: the union of every row's records, two of them one
span when the later one starts at most `gap` behind the earlier one's end; and what the header, the binding, the stubs and
the extension classes declare for cover_spans / cover_spans_batch).  Expected values come from Python (the sort-and-sweep
definition restated below over synthetic records), never from the library.  tests/test_gpu_spans.py has the device side."""
import ast
import os
import re

import numpy as np
import pytest

capi = pytest.importorskip("ahocorasick_rs_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ahocorasick_rs_amd", "csrc")

NEW_EXPORTS = ("acx_spans", "acx_spans_device", "acx_spans_host", "acx_spans_rows_device", "acx_spans_count", "acx_spans_rows",
               "acx_spans_on_device", "acx_spans_data", "acx_spans_copy", "acx_free_spans")
GAP_MAX = (1 << 63) - 1


def definition(records, counts, gap):
    """sort and sweep: per row the live records (start < end) by start; a record joins the open span when its start is at
    most the span's end + gap, else it opens the next one -> (row_offsets, [(start, end)])"""
    counts = [len(records)] if counts is None else [int(c) for c in counts]
    spans, ro, at = [], [0], 0
    for c in counts:
        live = sorted((int(s), int(e)) for _, s, e in records[at:at + c] if int(s) < int(e))
        at += c
        first = len(spans)
        for s, e in live:
            if len(spans) > first and s - spans[-1][1] <= gap:
                spans[-1] = (spans[-1][0], max(spans[-1][1], e))
            else:
                spans.append((s, e))
        ro.append(len(spans))
    assert at == len(records)
    return ro, spans


def check(records, counts, gap=0, what=None):
    records = [tuple(int(x) for x in r) for r in records]
    ro, start, end = capi.spans_host(np.asarray(records, dtype=np.uint64).reshape(-1, 3), counts, gap)
    want_ro, want = definition(records, counts, gap)
    assert start.dtype == end.dtype == ro.dtype == np.int64
    got = list(zip(start.astype(np.uint64).tolist(), end.astype(np.uint64).tolist()))
    assert got == want and ro.tolist() == want_ro, (what, gap, got[:12], want[:12], ro.tolist()[:12], want_ro[:12])
    # what the issue promises of every result
    for h in range(len(want_ro) - 1):
        row = got[want_ro[h]:want_ro[h + 1]]
        assert all(s < e for s, e in row) and all(b[0] - a[1] > gap for a, b in zip(row, row[1:])), (what, h)
    return got


def random_rows(rng, counts, span=200, longest=12, empties=0.15, base=0):
    """counts[h] records per row with random starts, some of them empty (start == end) or reversed, ordered by (end, start)
    within a row as a search reports them"""
    out = []
    for k in counts:
        rec = []
        for _ in range(int(k)):
            s = base + int(rng.integers(0, span))
            e = s + int(rng.integers(1, longest + 1))
            if rng.random() < empties:
                e = s if rng.random() < 0.5 else max(s - 1, 0)
            rec.append((int(rng.integers(0, 1 << 20)), s, e))
        rec.sort(key=lambda r: (r[2], r[1]))
        out += rec
    return out


@pytest.mark.parametrize("gap", [0, 1, 2, 5, 64, GAP_MAX])
def test_spans_host_on_seeded_batches(gap):
    rng = np.random.default_rng(20261020 + gap % 1000)
    for rows in (1, 2, 7, 64, 301):
        counts = rng.choice([0, 0, 1, 2, 5, 40], size=rows)
        check(random_rows(rng, counts), counts, gap, ("ragged", rows))
        check(random_rows(rng, counts, span=4000), counts, gap, ("sparse", rows))
        check(random_rows(rng, counts, span=30, empties=0.5), counts, gap, ("dense, many empty", rows))
    one = random_rows(rng, [500], span=3000)
    check(one, None, gap, "one row, counts = NULL")
    check(one, [500], gap, "one row with its count")


def test_spans_host_empty_rows_and_nothing():
    assert check([], None) == [] and check([], []) == [] and check([], [0, 0, 0]) == []
    assert check([(0, 1, 2)], [0, 1, 0]) == [(1, 2)]
    assert check([(0, 1, 2), (0, 2, 3)], [0, 1, 0, 0, 1, 0]) == [(1, 2), (2, 3)]          # touching, but in two rows
    assert check([(0, 1, 2), (0, 2, 3)], [1, 1], GAP_MAX) == [(1, 2), (2, 3)]              # whatever the gap is
    assert check([(0, 5, 5), (0, 7, 3), (0, 0, 0)], [2, 1]) == []                          # rows whose records are all empty
    ro, s, e = capi.spans_host(np.zeros((0, 3), dtype=np.uint64), [0, 0], 0)
    assert ro.tolist() == [0, 0, 0] and len(s) == len(e) == 0


def test_spans_host_nested_identical_and_chained_records_ordered_by_end():
    nested = [(0, 4, 6), (1, 3, 7), (2, 2, 8), (3, 0, 9)]        # each one inside the next
    same = [(0, 15, 19), (1, 15, 19), (2, 15, 19)]               # copies of a pattern
    chained = [(0, 30, 34), (1, 32, 36), (2, 35, 39), (3, 39, 42), (4, 42, 43)]
    assert check(nested, None) == [(0, 9)]
    assert check(same, None) == [(15, 19)]
    assert check(chained, None) == [(30, 43)]                    # overlapping, then touching: one span
    assert check(nested + same + chained, None) == [(0, 9), (15, 19), (30, 43)]
    assert check(nested + same + chained, None, 5) == [(0, 9), (15, 19), (30, 43)]
    assert check(nested + same + chained, None, 6) == [(0, 19), (30, 43)]
    assert check(nested + same + chained, None, 11) == [(0, 43)]
    assert check(nested + same + chained, [4, 3, 5], 11) == [(0, 9), (15, 19), (30, 43)]
    # a long record that ends last reaches back over everything before it
    assert check([(0, 10, 12), (0, 20, 22), (0, 30, 32), (0, 5, 40)], None) == [(5, 40)]
    assert check([(0, 10, 12), (0, 20, 22), (0, 30, 32), (0, 21, 40)], None) == [(10, 12), (20, 40)]


def test_spans_host_empty_records_at_every_position():
    live = [(0, 2, 4), (0, 4, 6), (0, 10, 12), (0, 20, 25)]
    want = definition(live, None, 0)[1]
    for at in range(len(live) + 1):
        for dead in ((9, 3, 3), (9, 12, 12), (9, 30, 7), (9, 0, 0)):
            for k in (1, 3):
                rec = live[:at] + [dead] * k + live[at:]
                assert check(rec, None, 0, (at, dead, k)) == want
                assert check(rec, [at + k, len(live) - at], 0) == definition(live, [at, len(live) - at], 0)[1]


def test_spans_host_gaps_around_the_hole():
    rec = [(0, 10, 20), (0, 27, 30), (0, 30, 31), (0, 100, 101)]  # holes of 7 and 69
    assert check(rec, None, 0) == [(10, 20), (27, 31), (100, 101)]
    assert check(rec, None, 1) == [(10, 20), (27, 31), (100, 101)]
    assert check(rec, None, 6) == [(10, 20), (27, 31), (100, 101)]   # the hole - 1
    assert check(rec, None, 7) == [(10, 31), (100, 101)]              # the exact hole
    assert check(rec, None, 68) == [(10, 31), (100, 101)]
    assert check(rec, None, 69) == [(10, 101)]
    assert check(rec, None, GAP_MAX) == [(10, 101)]
    assert check(rec, [2, 2], GAP_MAX) == [(10, 30), (30, 101)]


def test_spans_host_values_beyond_32_bits():
    B = 1 << 40
    rec = [(0, B, B + 5), (0, B + 5, B + 9), (0, B + 10, B + 11), (0, (1 << 62), (1 << 62) + 1), (0, (1 << 63) - 2, (1 << 63) - 1)]
    assert check(rec, None, 0) == [(B, B + 9), (B + 10, B + 11), (1 << 62, (1 << 62) + 1), ((1 << 63) - 2, (1 << 63) - 1)]
    assert check(rec, None, 1) == [(B, B + 11), (1 << 62, (1 << 62) + 1), ((1 << 63) - 2, (1 << 63) - 1)]
    assert check(rec, None, GAP_MAX) == [(B, (1 << 63) - 1)]
    # words beyond 2^63 compare as unsigned: no difference wraps
    big = [(0, 5, 6), (0, (1 << 64) - 3, (1 << 64) - 2)]
    assert check(big, None, GAP_MAX) == [(5, 6), ((1 << 64) - 3, (1 << 64) - 2)]
    rng = np.random.default_rng(5)
    counts = [40, 0, 3, 200]
    check(random_rows(rng, counts, span=500, base=(1 << 33) - 250), counts, 3, "around 2^33")


def test_spans_host_refuses_bad_arguments():
    rec = [(0, 1, 2), (0, 3, 4), (0, 5, 6)]
    for counts in ([1, 1], [2, 2], [4, 0], [0, 0], [(1 << 64) - 1, 4], []):  # the counts do not sum to the records
        with pytest.raises(ValueError) as ei:
            capi.spans_host(rec, counts, 0)
        assert ei.value.code == capi.EINVAL, counts
    for gap in (1 << 63, (1 << 64) - 1):
        with pytest.raises(ValueError) as ei:
            capi.spans_host(rec, None, gap)
        assert ei.value.code == capi.EINVAL, gap
    L = capi.lib()
    m = np.asarray(rec, dtype=np.uint64)
    c = np.asarray([1, 2], dtype=np.uint64)
    ro, s, e = np.zeros(3, np.int64), np.full(4, -7, np.int64), np.full(4, -7, np.int64)
    n = capi.ctypes.c_uint64(99)
    ok = lambda *a: L.acx_spans_host(*a, capi.ctypes.byref(n))  # noqa: E731
    assert ok(m.ctypes.data, 3, c.ctypes.data, 2, 0, ro.ctypes.data, s.ctypes.data, e.ctypes.data) == capi.OK and n.value == 3
    assert s.tolist() == [1, 3, 5, -7] and e.tolist() == [2, 4, 6, -7] and ro.tolist() == [0, 1, 3]   # nothing behind the spans
    assert ok(m.ctypes.data, 3, c.ctypes.data, 2, 1, None, s.ctypes.data, e.ctypes.data) == capi.OK and n.value == 2  # no row offsets wanted
    assert ok(None, 3, c.ctypes.data, 2, 0, ro.ctypes.data, s.ctypes.data, e.ctypes.data) == capi.EINVAL        # no records
    assert ok(m.ctypes.data, 3, c.ctypes.data, 2, 0, ro.ctypes.data, None, e.ctypes.data) == capi.EINVAL        # no start
    assert ok(m.ctypes.data, 3, c.ctypes.data, 2, 0, ro.ctypes.data, s.ctypes.data, None) == capi.EINVAL        # no end
    assert ok(m.ctypes.data, 3, None, 2, 0, ro.ctypes.data, s.ctypes.data, e.ctypes.data) == capi.EINVAL        # two rows, no counts
    assert L.acx_spans_host(m.ctypes.data, 3, c.ctypes.data, 2, 0, ro.ctypes.data, s.ctypes.data, e.ctypes.data, None) == capi.EINVAL
    assert ok(None, 0, None, 0, 0, ro.ctypes.data, None, None) == capi.OK and n.value == 0 and ro.tolist()[:2] == [0, 0]


def test_header_and_binding_agree_on_the_spans_abi():
    hdr = open(os.path.join(ROOT, "include", "acx.h")).read()
    L = capi.lib()
    for name in NEW_EXPORTS:
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert decl, name
        assert hasattr(L, name), name
        n_args = len([a for a in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",") if a.strip()])
        assert len(getattr(L, name).argtypes) == n_args, (name, n_args)  # bound with its argument types, one per argument
    for k, name in enumerate(("START", "END", "ROW_OFFSETS")):
        assert int(re.search(r"#define ACX_SPAN_%s (\d+)" % name, hdr).group(1)) == getattr(capi, "SPAN_" + name) == k
    assert re.search(r"typedef struct acx_spans acx_spans_t;", hdr)
    # acx_spans* take acx_find_columns*'s arguments with `gap` in front of the result
    u64 = capi.ctypes.c_uint64
    for mine, plain in (("acx_spans", "acx_find_columns"), ("acx_spans_device", "acx_find_columns_device")):
        want = list(getattr(L, plain).argtypes)
        want.insert(len(want) - 1, u64)
        assert list(getattr(L, mine).argtypes) == want, mine
    assert list(L.acx_spans_data.argtypes) == list(L.acx_columns_data.argtypes) and L.acx_spans_data.restype is capi.ctypes.c_void_p
    assert list(L.acx_spans_copy.argtypes) == list(L.acx_columns_copy.argtypes)
    assert L.acx_spans_count.restype is u64 and L.acx_spans_rows.restype is u64 and L.acx_free_spans.restype is None
    assert list(L.acx_spans_host.argtypes) == list(L.acx_spans_rows_device.argtypes)
    assert L.acx_spans_host.argtypes[4] is u64 and L.acx_spans_host.argtypes[1] is u64 and L.acx_spans_host.argtypes[3] is u64
    # additive: the version and the path counters are the parent's
    assert L.acx_version() == capi.ABI_VERSION == int(re.search(r"#define ACX_VERSION (\d+)", hdr).group(1)) == 11
    assert len(capi.Automaton.PATH_STATS) == int(re.search(r"#define ACX_PATH_STATS (\d+)", hdr).group(1)) == 14
    for name in ("spans", "spans_device"):
        assert callable(getattr(capi.Automaton, name))
    assert callable(capi.spans_host) and callable(capi.spans_rows_device) and capi.DeviceSpans


def test_the_stage_is_in_the_build_list_and_its_sizes_are_plain_constants():
    from ahocorasick_rs_amd import _build
    assert "spans.hip" in _build.LIB_SOURCES and "spans_api.cpp" in _build.LIB_SOURCES and "spans.hpp" in _build.LIB_HEADERS
    for f in ("spans.hip", "spans_api.cpp", "spans.hpp"):
        assert os.path.exists(os.path.join(CSRC, f)), f
    hpp = open(os.path.join(CSRC, "spans.hpp")).read()
    c = {}
    for name in ("SPANS_THREADS", "SPANS_TILE"):  # plain constants: the seam tests read them
        m = re.search(r"constexpr uint32_t %s\s*=\s*(\d+)\s*;" % name, hpp)
        assert m, name
        c[name] = int(m.group(1))
    assert c["SPANS_TILE"] % c["SPANS_THREADS"] == 0 and c["SPANS_THREADS"] % 64 == 0
    hip = open(os.path.join(CSRC, "spans.hip")).read()
    assert "asm" not in hip, "plain C++ stores only"
    assert not re.findall(r"\batomic\w+\(", hip), "the stage needs no atomic"


def test_pyi_declares_the_methods_and_the_class():
    tree = ast.parse(open(os.path.join(ROOT, "ahocorasick_rs_amd", "ahocorasick_rs.pyi")).read())
    classes = {c.name: c for c in tree.body if isinstance(c, ast.ClassDef)}
    want = {
        "cover_spans": (["self", "haystack", "overlapping"], ["gap"], ["0"]),
        "cover_spans_batch": (["self", "haystacks", "overlapping"], ["gap", "offsets", "row_length"], ["0", "None", "None"]),
    }
    for cls in ("AhoCorasick", "BytesAhoCorasick"):
        for method, (pos, kwonly, kwdefaults) in want.items():
            mine = [f for f in classes[cls].body if isinstance(f, ast.FunctionDef) and f.name == method]
            assert len(mine) == 1, (cls, method)
            a = mine[0].args
            assert [x.arg for x in a.args] == pos, (cls, method)
            assert [x.arg for x in a.kwonlyargs] == kwonly, (cls, method)
            assert a.vararg is None and a.kwarg is None, (cls, method)
            assert [ast.unparse(d) for d in a.defaults] == ["False"], (cls, method)
            assert [ast.unparse(d) for d in a.kw_defaults] == kwdefaults, (cls, method)
            assert ast.unparse(mine[0].returns) == "MatchSpans", (cls, method)
            gap = [x for x in a.kwonlyargs if x.arg == "gap"][0]
            assert ast.unparse(gap.annotation) == "int"
    names = {f.name for f in classes["MatchSpans"].body if isinstance(f, ast.FunctionDef)}
    assert names == {"start", "end", "row_offsets", "device", "__len__", "tolist"}   # MatchColumns without `pattern`
    assert "__init__" not in names


def test_extension_classes_have_the_methods():
    import ahocorasick_rs
    import ahocorasick_rs_amd
    sigs = (("cover_spans", "cover_spans(haystack, overlapping=False, *, gap=0) -> MatchSpans"),
            ("cover_spans_batch", "cover_spans_batch(haystacks, overlapping=False, *, gap=0, offsets=None, row_length=None) -> MatchSpans"))
    for mod in (ahocorasick_rs, ahocorasick_rs_amd, ahocorasick_rs.ahocorasick_rs):
        for cls in (mod.AhoCorasick, mod.BytesAhoCorasick):
            for method, sig in sigs:
                assert callable(getattr(cls, method)), (cls, method)
                assert getattr(cls, method).__doc__.startswith(sig), (cls, method)
        assert isinstance(mod.MatchSpans, type) and "MatchSpans" in mod.__all__
        with pytest.raises(TypeError):
            mod.MatchSpans()  # (made by the methods only)
    assert ahocorasick_rs.MatchSpans is ahocorasick_rs_amd.MatchSpans
    assert set(ahocorasick_rs.__all__) == set(ahocorasick_rs_amd.__all__)
    for name in ("start", "end", "row_offsets", "device", "tolist", "__len__"):
        assert hasattr(ahocorasick_rs.MatchSpans, name)
    assert not hasattr(ahocorasick_rs.MatchSpans, "pattern")
    # the parent's methods keep their signatures
    assert "match_mask_batch(haystacks, overlapping=False, *, offsets=None, row_length=None)" in ahocorasick_rs.AhoCorasick.match_mask_batch.__doc__
    assert "MaskedRows" in ahocorasick_rs.__all__ and "MatchColumns" in ahocorasick_rs.__all__


def test_the_gap_argument():
    """the one check both classes' cover_spans and cover_spans_batch make of `gap` (the extension's _spans_gap: no automaton)"""
    from ahocorasick_rs_amd.ahocorasick_rs import _spans_gap
    for gap in (0, 1, 64, 1 << 32, GAP_MAX):
        assert _spans_gap(gap) == gap
    for bad in (-1, -(1 << 70), 1 << 63, 1 << 64, 1 << 70):
        with pytest.raises(ValueError):
            _spans_gap(bad)
    for bad in (True, False, 1.0, "1", None, b"1", [1], np.float64(2)):
        with pytest.raises(TypeError):
            _spans_gap(bad)
