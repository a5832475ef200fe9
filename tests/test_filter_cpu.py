"""CPU checks of the row filter (acx_filter_host: keep or drop the rows of a batch by their match counts, and what the
header, the binding, the stubs and the extension classes declare for filter_batch).  Expected values come from a plain
Python restatement of the definition, never from the library.  tests/test_gpu_filter.py has the device side."""
import ast
import os
import re

import numpy as np
import pytest

capi = pytest.importorskip("ahocorasick_rs_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

METHOD = "filter_batch"
NEW_EXPORTS = ("acx_filter", "acx_filter_device", "acx_filter_host", "acx_filter_rows_device", "acx_filtered_rows",
               "acx_filtered_bytes", "acx_filtered_on_device", "acx_filtered_data", "acx_filtered_copy", "acx_free_filtered")
GUARD = 0x5A


def definition(rows, counts, min_matches, keep):
    """the issue's definition: rows (list of bytes), counts[h] -> (kept row indexes, offsets, data)"""
    kept, offsets, data = [], [0], b""
    for h, row in enumerate(rows):
        matched = counts[h] >= min_matches
        if matched == (keep == "matched"):
            kept.append(h)
            data += row
            offsets.append(len(data))
    return np.asarray(kept, np.int64), np.asarray(offsets, np.int64), np.frombuffer(data, np.uint8)


def offsets_of(rows):
    return np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)


def check(rows, counts, min_matches, keep):
    flags = capi.FILTER_KEEP_MATCHED if keep == "matched" else 0
    hay = b"".join(rows)
    got = capi.filter_host(hay, offsets_of(rows), counts, min_matches, flags)
    want = definition(rows, counts, min_matches, keep)
    for g, w, dt in zip(got, want, (np.int64, np.int64, np.uint8)):
        assert g.dtype == dt and np.array_equal(g, w), (len(rows), min_matches, keep, g[:20], w[:20])
    assert capi.filter_host(hay, offsets_of(rows), counts, min_matches, flags, sizes_only=True) == (len(want[0]), len(want[2]))
    assert (np.diff(got[0]) > 0).all() and got[1][0] == 0
    for i, h in enumerate(got[0]):  # the kept rows are the caller's own bytes
        assert got[2][got[1][i]:got[1][i + 1]].tobytes() == rows[h]


def seeded_batch(seed, n):
    rng = np.random.default_rng(seed)
    rows = [bytes(rng.integers(0, 256, size=int(rng.choice([0, 0, 1, 2, 15, 16, 17, 100])), dtype=np.uint8)) for _ in range(n)]
    counts = [int(c) for c in rng.choice([0, 0, 1, 2, 4, 5, 9], size=n)]
    return rows, counts


@pytest.mark.parametrize("keep", ["unmatched", "matched"])
@pytest.mark.parametrize("min_matches", [1, 2, 5])
def test_filter_host_on_seeded_batches(keep, min_matches):
    for seed, n in ((1, 1), (2, 7), (3, 64), (4, 301)):
        rows, counts = seeded_batch(20261018 + seed, n)
        check(rows, counts, min_matches, keep)
    rows, counts = seeded_batch(99, 301)
    assert any(not r for r in rows) and any(c >= 5 for c in counts) and any(c == 0 for c in counts)


@pytest.mark.parametrize("rows,counts", [
    ([], []),                                             # an empty batch
    ([b"", b"", b""], [0, 3, 0]),                         # all rows empty: rows they are
    ([b"", b"ab", b"", b"", b"cde", b""], [0] * 6),       # all kept / none kept by the keep mode
    ([b"ab", b"cde", b"f"], [1, 7, 2]),                   # all matched
    ([b"ab", b"", b"cde"], [1, 0, 0]),                    # all but the first
    ([b"ab", b"", b"cde"], [0, 0, 1]),                    # all but the last
], ids=["empty-batch", "all-empty", "no-match", "all-match", "but-first", "but-last"])
@pytest.mark.parametrize("keep", ["unmatched", "matched"])
def test_filter_host_cases(rows, counts, keep):
    check(rows, counts, 1, keep)


def test_filter_host_one_row_without_offsets():
    for counts, flags, kept in (([2], capi.FILTER_KEEP_MATCHED, True), ([2], 0, False), ([1], capi.FILTER_KEEP_MATCHED, True)):
        rows, off, data = capi.filter_host(b"hello", None, counts, 1, flags)
        assert list(rows) == ([0] if kept else []) and list(off) == ([0, 5] if kept else [0])
        assert data.tobytes() == (b"hello" if kept else b"")
    assert capi.filter_host(b"hello", None, [2], 3, capi.FILTER_KEEP_MATCHED, sizes_only=True) == (0, 0)


def test_filter_host_writes_exactly_its_outputs():
    rows = [b"abc", b"", b"defgh", b"", b"i"]
    counts = np.asarray([0, 0, 2, 1, 0], dtype=np.uint64)
    hay = np.frombuffer(b"".join(rows), dtype=np.uint8)
    off = offsets_of(rows)
    wr, wo, wd = definition(rows, list(counts), 1, "unmatched")
    r = np.full(len(wr) + 2, -7, dtype=np.int64)
    o = np.full(len(wo) + 2, -7, dtype=np.int64)
    d = np.full(len(wd) + 2, GUARD, dtype=np.uint8)
    k, nb = capi.ctypes.c_uint64(), capi.ctypes.c_uint64()
    rc = capi.lib().acx_filter_host(hay.ctypes.data, len(hay), off.ctypes.data, len(rows), counts.ctypes.data, 1, 0,
                                    r[1:].ctypes.data, o[1:].ctypes.data, d[1:].ctypes.data, capi.ctypes.byref(k),
                                    capi.ctypes.byref(nb))
    assert rc == capi.OK and (k.value, nb.value) == (len(wr), len(wd))
    assert r[0] == r[-1] == -7 and np.array_equal(r[1:-1], wr)
    assert o[0] == o[-1] == -7 and np.array_equal(o[1:-1], wo)
    assert d[0] == d[-1] == GUARD and np.array_equal(d[1:-1], wd)


def test_filter_host_refuses_bad_arguments():
    rows = [b"ab", b"cd"]
    hay, off = b"".join(rows), [0, 2, 4]
    for kw in (dict(flags=2), dict(flags=3), dict(flags=1 << 31), dict(min_matches=0)):
        with pytest.raises(ValueError) as ei:
            capi.filter_host(hay, off, [0, 1], **kw)
        assert ei.value.code == capi.EINVAL, kw
    for bad in ([1, 2, 4], [0, 3, 2], [0, 2, 3], [0, 2, 5], [0, 5, 4]):  # not from 0, not rising, not to len
        with pytest.raises(ValueError) as ei:
            capi.filter_host(hay, bad, [0, 1])
        assert ei.value.code == capi.EINVAL, bad


def test_header_and_binding_agree_on_the_filter_abi():
    hdr = open(os.path.join(ROOT, "include", "acx.h")).read()
    L = capi.lib()
    for name in NEW_EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes, name  # bound with its argument types
    for k, name in enumerate(("ROWS", "OFFSETS", "DATA")):
        assert getattr(capi, "FILT_" + name) == int(re.search(r"#define ACX_FILT_%s (\d+)" % name, hdr).group(1)) == k
    assert capi.FILTER_KEEP_MATCHED == int(re.search(r"#define ACX_FILTER_KEEP_MATCHED (\d+)", hdr).group(1)) == 1
    # additive: the version and the path counters are the parent's
    assert L.acx_version() == capi.ABI_VERSION == int(re.search(r"#define ACX_VERSION (\d+)", hdr).group(1)) == 11
    assert len(capi.Automaton.PATH_STATS) == int(re.search(r"#define ACX_PATH_STATS (\d+)", hdr).group(1)) == 14
    for name in ("filter", "filter_device"):
        assert callable(getattr(capi.Automaton, name))
    assert callable(capi.filter_host) and callable(capi.filter_rows_device) and capi.DeviceFiltered


def test_the_stage_is_in_the_build_list():
    from ahocorasick_rs_amd import _build
    assert "filter.hip" in _build.LIB_SOURCES and "filter_api.cpp" in _build.LIB_SOURCES and "filter.hpp" in _build.LIB_HEADERS
    for f in ("filter.hip", "filter_api.cpp", "filter.hpp"):
        assert os.path.exists(os.path.join(ROOT, "ahocorasick_rs_amd", "csrc", f)), f
    hpp = open(os.path.join(ROOT, "ahocorasick_rs_amd", "csrc", "filter.hpp")).read()
    for name in ("FILTER_THREADS", "FILTER_TILE", "FILTER_WIN"):  # plain constants: the seam tests read them
        assert re.search(r"constexpr uint32_t %s\s*=\s*\d+\s*;" % name, hpp), name


def test_pyi_declares_the_method_and_the_class():
    tree = ast.parse(open(os.path.join(ROOT, "ahocorasick_rs_amd", "ahocorasick_rs.pyi")).read())
    classes = {c.name: c for c in tree.body if isinstance(c, ast.ClassDef)}
    for cls in ("AhoCorasick", "BytesAhoCorasick"):
        mine = [f for f in classes[cls].body if isinstance(f, ast.FunctionDef) and f.name == METHOD]
        assert len(mine) == 1, cls
        a = mine[0].args
        assert [x.arg for x in a.args] == ["self", "haystacks", "overlapping"], cls
        assert [x.arg for x in a.kwonlyargs] == ["keep", "min_matches", "offsets", "row_length"], cls
        assert a.vararg is None and a.kwarg is None, cls
        assert ast.unparse(a.defaults[0]) == "False", cls
        assert [ast.unparse(d) for d in a.kw_defaults] == ["'unmatched'", "1", "None", "None"], cls
        assert ast.unparse(mine[0].returns) == "FilteredRows"
    names = {f.name for f in classes["FilteredRows"].body if isinstance(f, ast.FunctionDef)}
    assert names >= {"rows", "offsets", "data", "device", "nbytes", "source_rows", "__len__", "tolist"}


def test_extension_classes_have_the_method():
    import ahocorasick_rs
    import ahocorasick_rs_amd
    for mod in (ahocorasick_rs, ahocorasick_rs_amd):
        for cls in (mod.AhoCorasick, mod.BytesAhoCorasick):
            assert callable(getattr(cls, METHOD)), cls
        assert isinstance(mod.FilteredRows, type) and "FilteredRows" in mod.__all__
        with pytest.raises(TypeError):
            mod.FilteredRows()  # (made by the method only)
    assert ahocorasick_rs.FilteredRows is ahocorasick_rs_amd.FilteredRows
    for name in ("rows", "offsets", "data", "device", "nbytes", "source_rows", "tolist", "__len__"):
        assert hasattr(ahocorasick_rs.FilteredRows, name)
