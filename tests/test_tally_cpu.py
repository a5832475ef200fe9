"""CPU checks of the tally (acx_tally_host: per-haystack pattern counts as a CSR matrix, and what the header, the binding,
the stubs and the extension classes declare for count_by_pattern_sparse_batch).  Expected values come from a
collections.Counter per row, never from the library.  tests/test_gpu_tally.py has the device side."""
import ast
import os
import re
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

capi = pytest.importorskip("ahocorasick_rs_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

METHOD = "count_by_pattern_sparse_batch"
NEW_EXPORTS = ("acx_tally", "acx_tally_device", "acx_tally_host", "acx_tally_rows_device", "acx_tally_nnz", "acx_tally_rows",
               "acx_tally_on_device", "acx_tally_data", "acx_tally_copy", "acx_free_tally")
GUARD = 0x5A5AA5A55A5AA5A5


def records_of(rows):
    """rows: one list of pattern ids per haystack -> (records with junk start / end words, counts)"""
    flat = [p for r in rows for p in r]
    m = np.zeros((len(flat), 3), dtype=np.uint64)
    m[:, 0] = np.asarray(flat, dtype=np.uint64)
    m[:, 1] = np.arange(len(flat), dtype=np.uint64) * np.uint64(3) + np.uint64(1 << 40)
    m[:, 2] = np.arange(len(flat), dtype=np.uint64) * np.uint64(5) + np.uint64(1 << 41)
    return m, [len(r) for r in rows]


def expected(rows):
    ro, pat, cnt = [0], [], []
    for r in rows:
        for p, c in sorted(Counter(r).items()):
            pat.append(p)
            cnt.append(c)
        ro.append(len(pat))
    return np.asarray(ro, np.int64), np.asarray(pat, np.int64), np.asarray(cnt, np.int64)


def check(rows):
    m, counts = records_of(rows)
    ro, pat, cnt = capi.tally_host(m, counts)
    want = expected(rows)
    for got, w in zip((ro, pat, cnt), want):
        assert got.dtype == np.int64 and np.array_equal(got, w), (rows if len(rows) < 20 else len(rows), got[:20], w[:20])
    assert (cnt >= 1).all()
    for h in range(len(rows)):
        assert (np.diff(pat[ro[h]:ro[h + 1]]) > 0).all(), h  # strictly ascending within a row


@pytest.mark.parametrize("rows", [
    [],                                   # zero rows
    [[], [], []],                         # all rows empty
    [[], [], [4, 4, 1], [2]],             # leading empty rows
    [[4, 4, 1], [2], [], []],             # trailing
    [[4, 4, 1], [], [], [2], [], [0]],    # interior
    [[7]],                                # one record
    [[9] * 37],                           # one pattern repeated
    [list(range(40, 0, -1))],             # all distinct, descending
    [[1, 5, 3], [3, 5, 1], [1], [1]],     # adjacent rows end and begin with the same pattern: they must not merge
    [[0, (1 << 24) - 1, 0], [(1 << 24) - 1], [0]],  # the lowest and the highest pattern id
], ids=["zero-rows", "all-empty", "leading-empty", "trailing-empty", "interior-empty", "one-record", "one-pattern",
        "descending", "no-merge-across-rows", "id-0-and-2^24-1"])
def test_tally_host_cases(rows):
    check(rows)


def test_tally_host_random_ragged_rows():
    rng = np.random.default_rng(20261017)
    left, rows = 5003, []
    while left:
        n = min(left, int(rng.choice([0, 0, 1, 2, 7, 64, 300])))
        span = int(rng.choice([1, 3, 50, 1 << 24]))
        rows.append([int(v) for v in rng.integers(0, span, size=n)])
        left -= n
    assert sum(len(r) for r in rows) == 5003 and any(not r for r in rows)
    check(rows)


def test_tally_host_writes_exactly_its_outputs():
    rows = [[3, 1, 3], [], [2, 2], [5, 4, 3, 2, 1]]
    m, counts = records_of(rows)
    c = np.asarray(counts, dtype=np.uint64)
    ro = np.full(len(rows) + 1 + 2, GUARD, dtype=np.uint64)
    pat = np.full(len(m) + 2, GUARD, dtype=np.uint64)
    cnt = np.full(len(m) + 2, GUARD, dtype=np.uint64)
    nnz = capi.ctypes.c_uint64()
    rc = capi.lib().acx_tally_host(m.ctypes.data, len(m), c.ctypes.data, len(c), ro[1:].ctypes.data, pat[1:].ctypes.data,
                                   cnt[1:].ctypes.data, capi.ctypes.byref(nnz))
    assert rc == capi.OK
    wro, wpat, wcnt = expected(rows)
    assert nnz.value == len(wpat)
    assert ro[0] == ro[-1] == GUARD and np.array_equal(ro[1:-1].view(np.int64), wro)
    for buf, w in ((pat, wpat), (cnt, wcnt)):
        assert buf[0] == GUARD and (buf[1 + len(w):] == GUARD).all() and np.array_equal(buf[1:1 + len(w)].view(np.int64), w)


def test_tally_host_refuses_counts_that_do_not_sum():
    m, _ = records_of([[1, 2, 3]])
    for counts in ([2], [4], [1, 1], [2 ** 64 - 1, 4]):
        with pytest.raises(ValueError) as ei:
            capi.tally_host(m, counts)
        assert ei.value.code == capi.EINVAL


def test_header_and_binding_agree_on_the_tally_abi():
    hdr = open(os.path.join(ROOT, "include", "acx.h")).read()
    L = capi.lib()
    for name in NEW_EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
    for k, name in enumerate(("ROW_OFFSETS", "PATTERN", "COUNT")):
        assert getattr(capi, "TALLY_" + name) == int(re.search(r"#define ACX_TALLY_%s (\d+)" % name, hdr).group(1)) == k
    # additive: the version and the path counters are the parent's
    assert L.acx_version() == capi.ABI_VERSION == int(re.search(r"#define ACX_VERSION (\d+)", hdr).group(1)) == 11
    assert len(capi.Automaton.PATH_STATS) == int(re.search(r"#define ACX_PATH_STATS (\d+)", hdr).group(1)) == 14
    for name in ("tally", "tally_device"):
        assert callable(getattr(capi.Automaton, name))
    assert callable(capi.tally_host) and callable(capi.tally_rows_device) and capi.DeviceTally


def test_the_stage_is_in_the_build_list():
    src = open(os.path.join(ROOT, "ahocorasick_rs_amd", "_build.py")).read()
    for f in ("tally.hip", "tally_api.cpp", "tally.hpp"):
        assert '"%s"' % f in src, f
        assert os.path.exists(os.path.join(ROOT, "ahocorasick_rs_amd", "csrc", f)), f


def test_pyi_declares_the_method_and_the_class():
    tree = ast.parse(open(os.path.join(ROOT, "ahocorasick_rs_amd", "ahocorasick_rs.pyi")).read())
    classes = {c.name: c for c in tree.body if isinstance(c, ast.ClassDef)}
    for cls in ("AhoCorasick", "BytesAhoCorasick"):
        mine = [f for f in classes[cls].body if isinstance(f, ast.FunctionDef) and f.name == METHOD]
        assert len(mine) == 1, cls
        a = mine[0].args
        assert [x.arg for x in a.args] == ["self", "haystacks", "overlapping"], cls
        assert [x.arg for x in a.kwonlyargs] == ["offsets", "row_length"] and a.vararg is None and a.kwarg is None, cls
        assert ast.unparse(a.defaults[0]) == "False" and [ast.unparse(d) for d in a.kw_defaults] == ["None", "None"], cls
        assert ast.unparse(mine[0].returns) == "PatternCounts"
    names = {f.name for f in classes["PatternCounts"].body if isinstance(f, ast.FunctionDef)}
    assert names >= {"row_offsets", "pattern", "count", "shape", "device", "__len__", "tolist"}


def test_extension_classes_have_the_method():
    import ahocorasick_rs
    import ahocorasick_rs_amd
    for mod in (ahocorasick_rs, ahocorasick_rs_amd):
        for cls in (mod.AhoCorasick, mod.BytesAhoCorasick):
            assert callable(getattr(cls, METHOD)), cls
        assert isinstance(mod.PatternCounts, type) and "PatternCounts" in mod.__all__
        with pytest.raises(TypeError):
            mod.PatternCounts()  # (made by the method only)
    assert ahocorasick_rs.PatternCounts is ahocorasick_rs_amd.PatternCounts
    for name in ("row_offsets", "pattern", "count", "shape", "device", "tolist", "__len__"):
        assert hasattr(ahocorasick_rs.PatternCounts, name)


def test_importing_the_package_still_needs_neither_numpy_nor_torch():
    code = ("import sys; sys.path.insert(0, %r); import ahocorasick_rs; ahocorasick_rs.PatternCounts; "
            "assert 'numpy' not in sys.modules and 'torch' not in sys.modules" % ROOT)
    subprocess.check_call([sys.executable, "-S", "-c", code])
