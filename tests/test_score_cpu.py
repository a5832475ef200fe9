"""CPU checks of the row scores (acx_score_host: per-pattern weights summed over every row's matches, and what the header,
the binding, the stubs and the extension classes declare for score_batch / filter_by_score_batch).  Expected values come
from numpy (np.add.at over the rows of random records), never from the library.  tests/test_gpu_score.py has the device
side."""
import ast
import os
import re

import numpy as np
import pytest

capi = pytest.importorskip("ahocorasick_rs_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_EXPORTS = ("acx_score", "acx_score_device", "acx_score_host", "acx_score_rows_device", "acx_scores_rows",
               "acx_scores_on_device", "acx_scores_data", "acx_scores_copy", "acx_free_scores", "acx_filter_scored",
               "acx_filter_scored_device")
W_MAX = (1 << 31) - 1


def definition(pattern, counts, weights):
    """score[h] = sum of weights[pattern] over row h's records (pattern >= len(weights): nothing), modulo 2^64"""
    pattern = np.asarray(pattern, dtype=np.uint64)
    w = np.asarray(weights, dtype=np.int64)
    row = np.repeat(np.arange(len(counts)), np.asarray(counts, dtype=np.int64))
    ok = pattern < len(w)
    score = np.zeros(len(counts), dtype=np.int64)
    with np.errstate(over="ignore"):
        np.add.at(score, row[ok], w[pattern[ok].astype(np.int64)])
    return score


def records(pattern, rng):
    """records of (pattern, start, end): the sum reads the pattern alone, the rest is noise"""
    m = rng.integers(0, 1 << 40, size=(len(pattern), 3), dtype=np.uint64)
    m[:, 0] = pattern
    return m


def check(pattern, counts, weights, rng):
    got = capi.score_host(records(pattern, rng), counts, weights)
    want = definition(pattern, counts, weights)
    assert got.dtype == np.int64 and np.array_equal(got, want), (len(counts), got[:10], want[:10])


# the per-row counts a find leaves behind, by kind: Standard (many short runs), overlapping (dense rows), leftmost (sparse
# rows, many empty ones), one haystack that is a batch of one row
COUNT_SHAPES = {
    "standard": lambda rng, rows: rng.integers(0, 6, size=rows),
    "overlapping": lambda rng, rows: rng.integers(10, 60, size=rows),
    "leftmost": lambda rng, rows: rng.choice([0, 0, 0, 1, 2], size=rows),
    "one-row": lambda rng, rows: np.asarray([rows * 3]),
}


@pytest.mark.parametrize("shape", sorted(COUNT_SHAPES))
def test_score_host_on_random_records(shape):
    rng = np.random.default_rng(20261018)
    for rows, n_patterns in ((1, 1), (7, 3), (64, 17), (301, 1000)):
        counts = COUNT_SHAPES[shape](rng, rows)
        n = int(counts.sum())
        weights = rng.integers(-50, 50, size=n_patterns)
        weights[rng.integers(0, n_patterns)] = 0
        check(rng.integers(0, n_patterns, size=n), counts, weights, rng)


def test_score_host_counts_null_is_one_row():
    rng = np.random.default_rng(1)
    pattern = rng.integers(0, 5, size=100)
    weights = [3, -2, 0, 7, -11]
    got = capi.score_host(records(pattern, rng), None, weights)
    assert list(got) == [int(definition(pattern, [100], weights)[0])]
    assert list(capi.score_host(np.zeros((0, 3), np.uint64), None, weights)) == [0]


def test_score_host_empty_rows_and_zero_rows():
    rng = np.random.default_rng(2)
    check([], [], [1, 2, 3], rng)                                  # zero rows
    check([], [0, 0, 0], [1, 2, 3], rng)                           # rows without a record score 0
    check([0, 1, 2, 2], [0, 0, 3, 0, 0, 1, 0], [5, -7, 11], rng)   # empty rows at the start, between and at the end


def test_score_host_negative_and_zero_weights():
    rng = np.random.default_rng(3)
    check([0, 1, 2, 0, 1, 2], [3, 3], [-1, 0, 1], rng)
    check([1, 1, 1, 1], [4], [9, 0], rng)
    assert list(capi.score_host(records([0, 1, 0, 1], rng), [4], [-5, 5])) == [0]
    assert list(capi.score_host(records([0, 0, 0], rng), [1, 2], [-(1 << 20)])) == [-(1 << 20), -(1 << 21)]


@pytest.mark.parametrize("w", [W_MAX, -W_MAX])
def test_score_host_extreme_weights_pass_2_pow_40(w):
    rng = np.random.default_rng(4)
    n = 600                                   # 600 * (2^31 - 1) > 2^40: the sum is 64-bit
    got = capi.score_host(records(np.zeros(n, np.uint64), rng), [n, 0], [w])
    assert abs(n * w) > 1 << 40 and list(got) == [n * w, 0]
    got = capi.score_host(records(np.tile([0, 1], n), rng), [2 * n], [w, -w])
    assert list(got) == [0]


def test_score_host_ignores_patterns_beyond_the_weights():
    rng = np.random.default_rng(5)
    pattern = np.asarray([0, 3, 1, 2, 1 << 40, 2, (1 << 64) - 1, 1], dtype=np.uint64)
    check(pattern, [4, 4], [10, 100, 1000], rng)
    assert list(capi.score_host(records(pattern, rng), [4, 4], [10, 100, 1000])) == [1110, 1100]
    assert list(capi.score_host(records(pattern, rng), [8], [])) == [0]  # no pattern at all: nothing to index


def test_score_host_refuses_bad_arguments():
    rng = np.random.default_rng(6)
    m = records([0, 1, 0], rng)
    for counts in ([1, 1], [2, 2], [4], [0, 0, 0], [(1 << 64) - 1, 4]):  # the counts do not sum to the records
        with pytest.raises(ValueError) as ei:
            capi.score_host(m, counts, [1, 2])
        assert ei.value.code == capi.EINVAL, counts
    L = capi.lib()
    w = np.asarray([1, 2], dtype=np.int32)
    c = np.asarray([3], dtype=np.uint64)
    out = np.zeros(1, dtype=np.int64)
    assert L.acx_score_host(None, 3, c.ctypes.data, 1, w.ctypes.data, 2, out.ctypes.data) == capi.EINVAL     # no records
    assert L.acx_score_host(m.ctypes.data, 3, c.ctypes.data, 1, None, 2, out.ctypes.data) == capi.EINVAL     # no weights
    assert L.acx_score_host(m.ctypes.data, 3, c.ctypes.data, 1, w.ctypes.data, 2, None) == capi.EINVAL       # no output
    assert L.acx_score_host(m.ctypes.data, 3, None, 2, w.ctypes.data, 2, out.ctypes.data) == capi.EINVAL     # two rows, no counts
    for bad in ([1 << 31], [-(1 << 31)], [0, 1 << 40]):  # the binding's own check: |w| < 2^31
        with pytest.raises(ValueError):
            capi.score_host(m, [3], bad)


def test_score_host_writes_exactly_its_output():
    rng = np.random.default_rng(7)
    m = records([0, 1, 1], rng)
    c = np.asarray([1, 0, 2], dtype=np.uint64)
    w = np.asarray([4, -9], dtype=np.int32)
    out = np.full(5, -7, dtype=np.int64)
    before = m.copy()
    assert capi.lib().acx_score_host(m.ctypes.data, 3, c.ctypes.data, 3, w.ctypes.data, 2, out[1:].ctypes.data) == capi.OK
    assert list(out) == [-7, 4, 0, -18, -7] and np.array_equal(m, before)


def test_header_and_binding_agree_on_the_score_abi():
    hdr = open(os.path.join(ROOT, "include", "acx.h")).read()
    L = capi.lib()
    for name in NEW_EXPORTS:
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert decl, name
        assert hasattr(L, name), name
        n_args = len([a for a in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",") if a.strip()])
        assert len(getattr(L, name).argtypes) == n_args, (name, n_args)  # bound with its argument types, one per argument
    # acx_filter_scored* take acx_filter*'s arguments with (weights, n_weights, min_score) in place of min_matches
    for scored, plain in (("acx_filter_scored", "acx_filter"), ("acx_filter_scored_device", "acx_filter_device")):
        want = list(getattr(L, plain).argtypes)
        at = want.index(capi.ctypes.c_uint32) - 1
        want[at:at + 1] = [capi.ctypes.c_void_p, capi.ctypes.c_uint64, capi.ctypes.c_int64]
        assert list(getattr(L, scored).argtypes) == want, scored
    # additive: the version and the path counters are the parent's
    assert L.acx_version() == capi.ABI_VERSION == int(re.search(r"#define ACX_VERSION (\d+)", hdr).group(1)) == 11
    assert len(capi.Automaton.PATH_STATS) == int(re.search(r"#define ACX_PATH_STATS (\d+)", hdr).group(1)) == 14
    for name in ("score", "score_device", "filter_scored", "filter_scored_device"):
        assert callable(getattr(capi.Automaton, name))
    assert callable(capi.score_host) and callable(capi.score_rows_device) and capi.DeviceScores


def test_the_stage_is_in_the_build_list():
    from ahocorasick_rs_amd import _build
    assert "score.hip" in _build.LIB_SOURCES and "score_api.cpp" in _build.LIB_SOURCES and "score.hpp" in _build.LIB_HEADERS
    for f in ("score.hip", "score_api.cpp", "score.hpp"):
        assert os.path.exists(os.path.join(ROOT, "ahocorasick_rs_amd", "csrc", f)), f
    hpp = open(os.path.join(ROOT, "ahocorasick_rs_amd", "csrc", "score.hpp")).read()
    for name in ("SCORE_THREADS", "SCORE_TILE"):  # plain constants: the seam tests read them
        assert re.search(r"constexpr uint32_t %s\s*=\s*\d+\s*;" % name, hpp), name


def test_pyi_declares_the_methods_and_the_class():
    tree = ast.parse(open(os.path.join(ROOT, "ahocorasick_rs_amd", "ahocorasick_rs.pyi")).read())
    classes = {c.name: c for c in tree.body if isinstance(c, ast.ClassDef)}
    want = {
        "score_batch": (["offsets", "row_length"], ["None", "None"], "RowScores"),
        "filter_by_score_batch": (["keep", "min_score", "offsets", "row_length"], ["'unmatched'", "1", "None", "None"], "FilteredRows"),
    }
    for cls in ("AhoCorasick", "BytesAhoCorasick"):
        for method, (kwonly, kw_defaults, returns) in want.items():
            mine = [f for f in classes[cls].body if isinstance(f, ast.FunctionDef) and f.name == method]
            assert len(mine) == 1, (cls, method)
            a = mine[0].args
            assert [x.arg for x in a.args] == ["self", "haystacks", "weights", "overlapping"], (cls, method)
            assert [x.arg for x in a.kwonlyargs] == kwonly, (cls, method)
            assert a.vararg is None and a.kwarg is None, (cls, method)
            assert [ast.unparse(d) for d in a.defaults] == ["False"], (cls, method)
            assert [ast.unparse(d) for d in a.kw_defaults] == kw_defaults, (cls, method)
            assert ast.unparse(mine[0].returns) == returns
    names = {f.name for f in classes["RowScores"].body if isinstance(f, ast.FunctionDef)}
    assert names >= {"score", "device", "__len__", "tolist"}


def test_extension_classes_have_the_methods():
    import ahocorasick_rs
    import ahocorasick_rs_amd
    for mod in (ahocorasick_rs, ahocorasick_rs_amd, ahocorasick_rs.ahocorasick_rs):
        for cls in (mod.AhoCorasick, mod.BytesAhoCorasick):
            for method in ("score_batch", "filter_by_score_batch"):
                assert callable(getattr(cls, method)), (cls, method)
                assert method + "(haystacks, weights, overlapping=False, *" in getattr(cls, method).__doc__
        assert isinstance(mod.RowScores, type) and "RowScores" in mod.__all__
        with pytest.raises(TypeError):
            mod.RowScores()  # (made by the method only)
    assert ahocorasick_rs.RowScores is ahocorasick_rs_amd.RowScores
    for name in ("score", "device", "tolist", "__len__"):
        assert hasattr(ahocorasick_rs.RowScores, name)
    # the parent's method keeps its signature
    assert "filter_batch(haystacks, overlapping=False, *, keep='unmatched', min_matches=1" in ahocorasick_rs.AhoCorasick.filter_batch.__doc__
