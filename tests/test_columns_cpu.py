"""CPU checks of the columns (acx_split_host, and what the header, the binding, the stubs and the extension classes declare
for find_matches_as_columns).  tests/test_gpu_columns.py has the device side."""
import ast
import os
import re

import numpy as np
import pytest

capi = pytest.importorskip("ahocorasick_rs_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

METHODS = ("find_matches_as_columns", "find_matches_as_columns_batch")
NEW_EXPORTS = ("acx_find_columns", "acx_find_columns_device", "acx_columns_count", "acx_columns_rows", "acx_columns_on_device",
               "acx_columns_data", "acx_columns_copy", "acx_free_columns", "acx_split_host", "acx_split_device")


def check_split(rows):
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 3)
    pattern, start, end = capi.split_host(rows)
    for got, k in ((pattern, 0), (start, 1), (end, 2)):
        assert got.dtype == np.int64 and got.shape == (len(rows),)
        assert np.array_equal(got.view(np.uint64), rows[:, k])


@pytest.mark.parametrize("n", [0, 1, 2])
def test_split_host_small(n):
    check_split([(3 * i, 3 * i + 1 + 2 ** 40, 3 * i + 2 + 2 ** 41) for i in range(n)])


def test_split_host_random_rows_beyond_32_bits():
    rng = np.random.default_rng(20261017)
    rows = rng.integers(0, 2 ** 63, size=(5003, 3), dtype=np.uint64)
    assert all((rows[:, k] >= 2 ** 32).any() for k in range(3))
    rows[7] = (2 ** 64 - 1, 2 ** 63, 2 ** 32)  # (the top bit: the int64 view of the same 64 bits)
    check_split(rows)


def test_split_host_writes_exactly_n_words():
    n = 37
    rows = np.arange(3 * n, dtype=np.uint64).reshape(n, 3)
    cols = [np.full(n + 2, 0x5A5A, dtype=np.int64) for _ in range(3)]
    rc = capi.lib().acx_split_host(rows.ctypes.data, n, *[c[1:].ctypes.data for c in cols])
    assert rc == capi.OK
    for k, c in enumerate(cols):
        assert c[0] == c[-1] == 0x5A5A and np.array_equal(c[1:-1].view(np.uint64), rows[:, k])


def test_split_of_nothing_touches_nothing():
    assert capi.lib().acx_split_host(None, 0, None, None, None) == capi.OK
    capi.split_device(0, 0, 0, 0, 0)  # (n = 0: no device is asked for)


def test_header_and_binding_agree_on_the_columns_abi():
    hdr = open(os.path.join(ROOT, "include", "acx.h")).read()
    L = capi.lib()
    for name in NEW_EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
    for k, name in enumerate(("PATTERN", "START", "END", "ROW_OFFSETS")):
        assert getattr(capi, "COL_" + name) == int(re.search(r"#define ACX_COL_%s (\d+)" % name, hdr).group(1)) == k
    # additive: the version and the path counters are the parent's
    assert L.acx_version() == capi.ABI_VERSION == int(re.search(r"#define ACX_VERSION (\d+)", hdr).group(1)) == 11
    assert len(capi.Automaton.PATH_STATS) == int(re.search(r"#define ACX_PATH_STATS (\d+)", hdr).group(1)) == 14
    for name in ("find_columns", "find_columns_batch", "find_columns_device"):
        assert callable(getattr(capi.Automaton, name))
    assert callable(capi.split_host) and callable(capi.split_device) and capi.DeviceColumns


def test_the_kernel_is_in_the_build_list():
    src = open(os.path.join(ROOT, "ahocorasick_rs_amd", "_build.py")).read()
    for f in ("columns.hip", "columns_api.cpp", "columns.hpp"):
        assert '"%s"' % f in src, f
        assert os.path.exists(os.path.join(ROOT, "ahocorasick_rs_amd", "csrc", f)), f


def test_pyi_declares_the_methods_and_the_classes():
    tree = ast.parse(open(os.path.join(ROOT, "ahocorasick_rs_amd", "ahocorasick_rs.pyi")).read())
    classes = {c.name: c for c in tree.body if isinstance(c, ast.ClassDef)}
    assert len(classes) == len([c for c in tree.body if isinstance(c, ast.ClassDef)])  # (no class twice)
    for cls in ("AhoCorasick", "BytesAhoCorasick"):
        fns = [f for f in classes[cls].body if isinstance(f, ast.FunctionDef)]
        for m in METHODS:
            mine = [f for f in fns if f.name == m]
            assert len(mine) == 1, (cls, m)
            args = [a.arg for a in mine[0].args.args]
            assert args == ["self", "haystacks" if m.endswith("_batch") else "haystack", "overlapping"], (cls, m, args)
            assert ast.unparse(mine[0].returns) == "MatchColumns"
    names = {f.name for f in classes["MatchColumns"].body if isinstance(f, ast.FunctionDef)}
    assert names >= {"pattern", "start", "end", "row_offsets", "device", "__len__", "tolist"}
    names = {f.name for f in classes["Column"].body if isinstance(f, ast.FunctionDef)}
    assert names >= {"__len__", "__dlpack__", "__dlpack_device__"}


def test_extension_classes_have_the_methods():
    import ahocorasick_rs
    import ahocorasick_rs_amd
    for mod in (ahocorasick_rs, ahocorasick_rs_amd):
        for cls in (mod.AhoCorasick, mod.BytesAhoCorasick):
            for m in METHODS:
                assert callable(getattr(cls, m)), (cls, m)
        for name in ("MatchColumns", "Column"):
            assert isinstance(getattr(mod, name), type) and name in mod.__all__
            with pytest.raises(TypeError):
                getattr(mod, name)()  # (made by the find methods only)
    assert ahocorasick_rs.MatchColumns is ahocorasick_rs_amd.MatchColumns
    assert ahocorasick_rs.Column is ahocorasick_rs_amd.Column
    for name in ("__dlpack__", "__dlpack_device__", "__len__"):
        assert hasattr(ahocorasick_rs.Column, name)
    for name in ("pattern", "start", "end", "row_offsets", "device", "tolist", "__len__"):
        assert hasattr(ahocorasick_rs.MatchColumns, name)


def test_importing_the_package_needs_neither_numpy_nor_torch():
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import ahocorasick_rs; ahocorasick_rs.MatchColumns; "
            "assert 'numpy' not in sys.modules and 'torch' not in sys.modules" % ROOT)
    subprocess.check_call([sys.executable, "-S", "-c", code])


def test_without_a_device_the_error_is_the_librarys():
    # no CPU fallback.  The methods are resolved on the CLASS first (AttributeError here means the method is missing); only
    # then is an object built and the call made: without a GPU the library's own error, with one the answer
    import ahocorasick_rs
    for cls, pat, hay in ((ahocorasick_rs.AhoCorasick, "ab", "xaby"), (ahocorasick_rs.BytesAhoCorasick, b"ab", b"xaby")):
        unbound = {m: getattr(cls, m) for m in METHODS}
        assert all(callable(f) for f in unbound.values())
        if capi.device_count() == 0:
            with pytest.raises(RuntimeError, match="no HIP device"):
                cls([pat])
            continue
        obj = cls([pat])
        for m, f in unbound.items():
            batch = m.endswith("_batch")
            got = f(obj, [hay] if batch else hay)
            assert isinstance(got, ahocorasick_rs.MatchColumns) and len(got) == 1 and got.device is None
            assert got.tolist() == ([[(0, 1, 3)]] if batch else [(0, 1, 3)]), (cls, m)
            assert [list(memoryview(c)) for c in (got.pattern, got.start, got.end)] == [[0], [1], [3]]
            assert (got.row_offsets is None) == (not batch)
            if batch:
                assert list(memoryview(got.row_offsets)) == [0, 1]
