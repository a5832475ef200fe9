"""CPU checks of the summaries (acx_summarize_host, the host route of acx_summarize): the oracle's matches reduced in plain
Python are the definition it must meet; what the header, the binding, the stubs and the extension classes declare; and what
the summary mode of tools/gpu_fuzz.py plans (tests/test_gpu_summary.py runs a slice of it on a GPU)."""
import ast
import os
import random
import re
import sys

import numpy as np
import pytest

import gen
from oracle_lib import KIND_DFA, Oracle

capi = pytest.importorskip("ahocorasick_rs_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gpu_fuzz  # noqa: E402

METHODS = ("is_match", "find_first", "count_matches", "count_by_pattern", "is_match_batch", "find_first_batch",
           "count_matches_batch", "count_by_pattern_batch")
NEW_EXPORTS = ("acx_summarize", "acx_summarize_device", "acx_summary_total", "acx_summary_on_device", "acx_summary_counts",
               "acx_summary_any", "acx_summary_first", "acx_summary_by_pattern", "acx_summary_device_counts",
               "acx_summary_device_any", "acx_summary_device_first", "acx_summary_device_by_pattern", "acx_free_summary",
               "acx_summarize_host")


def py_reduce(per_haystack, n_patterns):
    """per_haystack: one list of (pattern, start, end) per haystack -> (any, first, by_pattern)"""
    hist = [0] * n_patterns
    for ms in per_haystack:
        for p, _, _ in ms:
            hist[p] += 1
    return [len(ms) > 0 for ms in per_haystack], [ms[0] if ms else None for ms in per_haystack], hist


def check(per_haystack, n_patterns, one=False):
    rows = [m for ms in per_haystack for m in ms]
    counts = None if one else [len(ms) for ms in per_haystack]
    any_, first, hist = capi.summarize_host(rows, counts, n_patterns)
    want_any, want_first, want_hist = py_reduce(per_haystack, n_patterns)
    assert [bool(v) for v in any_] == want_any
    got_first = [None if int(r["pattern"]) == capi.NO_MATCH else (int(r["pattern"]), int(r["start"]), int(r["end"])) for r in first]
    assert got_first == want_first
    for r in first:
        if int(r["pattern"]) == capi.NO_MATCH:
            assert int(r["start"]) == 0 and int(r["end"]) == 0
    assert [int(v) for v in hist] == want_hist
    # the parts on their own
    a1, f1, h1 = capi.summarize_host(rows, counts, n_patterns, capi.SUM_FIRST)
    assert h1 is None and np.array_equal(a1, any_) and np.array_equal(f1, first)
    a2, f2, h2 = capi.summarize_host(rows, counts, n_patterns, capi.SUM_BY_PATTERN)
    assert a2 is None and f2 is None and np.array_equal(h2, hist)
    assert capi.summarize_host(rows, counts, n_patterns, 0) == (None, None, None)


@pytest.mark.parametrize("mk", [0, 1, 2])
@pytest.mark.parametrize("seed", range(40))
def test_summarize_host_equals_the_reduced_oracle(mk, seed):
    # 3 x 40 x (1 or 2 searches) seeded cases: batches of 0 .. 200 haystacks with empty ones among them, sets with patterns
    # that never match (the letters q .. z occur in no haystack), haystacks without any match
    rng = random.Random(1000 * mk + seed)
    pats = gen.gen_patterns(rng.choice([1, 3, 40, 300]), 1, 6, b"abcd", seed) + \
        gen.gen_patterns(rng.choice([1, 20]), 2, 5, b"qrstuvwxyz", seed + 1)
    rng.shuffle(pats)
    o = Oracle(pats, mk, KIND_DFA)
    n_hay = rng.choice([0, 1, 2, 63, 64, 65, 128, 200])
    alpha = rng.choice([b"abcde", b"efgh", b"abcdefghijklmnop"])  # (efgh: no match at all)
    hays = [bytes(rng.choice(alpha) for _ in range(rng.choice([0, 0, 1, 5, 40, 300]))) for _ in range(n_hay)]
    for ov in ([False, True] if mk == 0 else [False]):
        check([o.find(h, overlapping=ov) for h in hays], len(pats))
    if hays:
        check([o.find(hays[-1])], len(pats), one=True)


@pytest.mark.parametrize("n_hay", [0, 1, 63, 64, 65])
@pytest.mark.parametrize("fill", ["none", "all", "last", "alternate"])
def test_summarize_host_bitmap_words(n_hay, fill):
    has = {"none": lambda h: False, "all": lambda h: True, "last": lambda h: h == n_hay - 1, "alternate": lambda h: h % 2 == 1}[fill]
    per = [[(h % 3, h, h + 2), (2, h + 5, h + 6)] if has(h) else [] for h in range(n_hay)]
    check(per, 3)
    rows = [m for ms in per for m in ms]
    bits = np.zeros((n_hay + 63) // 64 + 1, dtype=np.uint64)
    bits[-1] = 0xABCD  # (a guard word behind the bitmap: exactly (n_hay + 63) / 64 words are written)
    first = np.zeros(n_hay + 1, dtype=capi.MATCH_DTYPE)
    counts = np.array([len(ms) for ms in per] + [0], dtype=np.uint64)
    m = np.array(rows, dtype=np.uint64).reshape(-1, 3)
    rc = capi.lib().acx_summarize_host(m.ctypes.data if len(m) else None, len(m), counts.ctypes.data, n_hay, 3, capi.SUM_FIRST,
                                       bits.ctypes.data, first.ctypes.data, None)
    assert rc == capi.OK and int(bits[-1]) == 0xABCD
    for h in range(n_hay):
        assert bool((int(bits[h >> 6]) >> (h & 63)) & 1) == has(h), h  # LSB first within a word


def test_summarize_host_utf8_rows():
    # code-point rows (Oracle.find_str) reduce like any others: the reduction never looks at the offsets
    pats = ["é☃", "ab", "b🤦", "☃"]
    o = Oracle([p.encode() for p in pats], 0, KIND_DFA)
    hays = ["", "ab☃é☃b🤦", "xxé☃" * 50, "🤦🤦ab", "nothing here"]
    check([o.find_str(h) for h in hays], len(pats))
    check([o.find_str(h, overlapping=True) for h in hays], len(pats))


def test_summarize_host_rejects_counts_that_do_not_sum():
    rows = [(0, 0, 1), (1, 2, 3), (0, 4, 5)]
    for counts in ([1, 1], [2, 2], [4], [0, 0, 0], [2 ** 63, 2 ** 63 + 3]):
        with pytest.raises(ValueError) as ei:
            capi.summarize_host(rows, counts, 2)
        assert ei.value.code == capi.EINVAL
    with pytest.raises(ValueError):
        capi.summarize_host([], [1], 2)


def test_summarize_host_rejects_a_pattern_beyond_the_set():
    for rows, n_pat in (([(2, 0, 1)], 2), ([(0, 0, 1), (7, 1, 2)], 3), ([(0, 0, 1)], 0), ([(capi.NO_MATCH, 0, 0)], 5)):
        with pytest.raises(ValueError) as ei:
            capi.summarize_host(rows, [len(rows)], n_pat)
        assert ei.value.code == capi.EINVAL
    with pytest.raises(ValueError) as ei:  # (bits of `what` that do not exist)
        capi.summarize_host([(0, 0, 1)], [1], 1, what=4)
    assert ei.value.code == capi.EINVAL


def test_header_and_binding_agree_on_the_summary_abi():
    hdr = open(os.path.join(ROOT, "include", "acx.h")).read()
    L = capi.lib()
    for name in NEW_EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
    assert capi.SUM_FIRST == int(re.search(r"#define ACX_SUM_FIRST (\d+)", hdr).group(1)) == 1
    assert capi.SUM_BY_PATTERN == int(re.search(r"#define ACX_SUM_BY_PATTERN (\d+)", hdr).group(1)) == 2
    # additive: the version and the path counters are the parent's
    assert L.acx_version() == capi.ABI_VERSION == int(re.search(r"#define ACX_VERSION (\d+)", hdr).group(1))
    assert len(capi.Automaton.PATH_STATS) == int(re.search(r"#define ACX_PATH_STATS (\d+)", hdr).group(1))
    for name in ("summarize", "summarize_batch", "summarize_device"):
        assert callable(getattr(capi.Automaton, name))
    assert callable(capi.summarize_host) and capi.DeviceSummary


def test_no_forbidden_mnemonic_in_the_new_sources():
    for f in ("summary.hip", "summary.hpp", "summary_api.cpp"):
        src = open(os.path.join(ROOT, "ahocorasick_rs_amd", "csrc", f)).read().lower()
        for word in ("s_" + "store", "s_buffer_" + "store", "s_scratch_" + "store", "s_" + "atomic", "s_buffer_" + "atomic",
                     "s_dcache_" + "wb", "s_dcache_" + "discard", "asm"):
            assert word not in src, (f, word)


def test_pyi_declares_the_summary_methods():
    tree = ast.parse(open(os.path.join(ROOT, "ahocorasick_rs_amd", "ahocorasick_rs.pyi")).read())
    classes = {c.name: c for c in tree.body if isinstance(c, ast.ClassDef)}
    for cls in ("AhoCorasick", "BytesAhoCorasick"):
        fns = {f.name: f for f in classes[cls].body if isinstance(f, ast.FunctionDef)}
        for m in METHODS:
            assert m in fns, (cls, m)
            args = [a.arg for a in fns[m].args.args]
            assert args[1] == ("haystacks" if m.endswith("_batch") else "haystack"), (cls, m, args)
            assert ("overlapping" in args) == m.startswith("count_"), (cls, m, args)


def test_extension_classes_have_the_summary_methods():
    import ahocorasick_rs
    import ahocorasick_rs_amd
    for mod in (ahocorasick_rs, ahocorasick_rs_amd):
        for cls in (mod.AhoCorasick, mod.BytesAhoCorasick):
            for m in METHODS:
                assert callable(getattr(cls, m)), (cls, m)


def test_without_a_device_the_error_is_the_librarys():
    # no CPU fallback.  The methods are resolved on the CLASS first (AttributeError here means the method is missing); only
    # then is an object built and the call made: without a GPU the library's own error, with one the answer
    import ahocorasick_rs
    want = {"is_match": True, "find_first": (0, 1, 3), "count_matches": 1, "count_by_pattern": [1]}
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
            one = want[m[:-len("_batch")] if batch else m]
            assert got == ([one] if batch and m != "count_by_pattern_batch" else one), (cls, m)


# ---- the plan of the summary mode of tools/gpu_fuzz.py
@pytest.fixture(scope="module")
def plan():
    return gpu_fuzz.plan_summary(gpu_fuzz.SUMMARY_N, gpu_fuzz.SUMMARY_SEED)


def test_summary_plan_is_deterministic(plan):
    again = gpu_fuzz.plan_summary(gpu_fuzz.SUMMARY_N, gpu_fuzz.SUMMARY_SEED)
    assert len(plan) == len(again) == gpu_fuzz.SUMMARY_N
    for a, b in zip(plan, again):
        assert a == b, a["i"]
    assert gpu_fuzz.plan_digest(plan) == gpu_fuzz.plan_digest(again)
    assert gpu_fuzz.plan_digest(plan[:7]) != gpu_fuzz.plan_digest(gpu_fuzz.plan_summary(7, gpu_fuzz.SUMMARY_SEED + 1))


def test_summary_plan_leaves_the_fuzz_sequence_alone():
    gpu_fuzz.rng, gpu_fuzz.MAX_SIZE_LOG2 = random.Random(5), 12.0
    first = gpu_fuzz.make_case()
    gpu_fuzz.rng = random.Random(5)
    gpu_fuzz.plan_summary(3, 1)
    assert gpu_fuzz.MAX_SIZE_LOG2 == 12.0 and gpu_fuzz.make_case() == first
    # and the surface plan is what it was: the new mode touches neither its ops nor its size and seed
    assert len(gpu_fuzz.OPS) == 11 and (gpu_fuzz.SURFACE_N, gpu_fuzz.SURFACE_SEED) == (176, 20261016)


def test_summary_plan_covers_the_entry_points(plan):
    assert {c["op"] for c in plan} == set(gpu_fuzz.SUMMARY_OPS) and len(gpu_fuzz.SUMMARY_OPS) == 6
    for op in gpu_fuzz.SUMMARY_OPS:
        cs = [c for c in plan if c["op"] == op]
        assert len(cs) >= 12, op
        for ci in (False, True):
            assert sum(c["ci"] == ci for c in cs) >= 4, (op, ci)
        for mk in (0, 1, 2):
            assert sum(c["mk"] == mk for c in cs) >= 2, (op, mk)
        if op.startswith("summarize_device_") and op != "summarize_device_route":  # odd and even pointer residues
            assert any(c["off"] % 2 for c in cs) and any(c["off"] % 2 == 0 for c in cs), op
    assert {c["route"] for c in plan if c["op"] == "summarize_batch"} == {"host", "device"}
    assert {c["what"] for c in plan} == {0, 1, 2, 3}
    assert sum(c["ov"] for c in plan) >= 3 and sum(c["cp"] for c in plan) >= 3
    assert sum(c["ov"] and bool(c["what"] & 2) for c in plan) >= 1  # overlapping counts per pattern
    assert sum(c["cp"] and bool(c["what"] & 1) for c in plan) >= 1  # a code-point first match
    batches = [c for c in plan if c["op"] in ("summarize_batch", "summarize_device_ragged", "summarize_device_uniform")]
    assert sum(any(len(h) == 0 for h in c["hays"]) for c in batches) >= 5
    assert sum(len(c["hays"]) > 64 for c in batches) >= 3  # more than one word of the bitmap


def test_no_summary_case_can_be_skipped(plan):
    for c in plan:
        ref = gpu_fuzz.reference(c)
        assert len(ref["rows"]) == c["rows"] <= gpu_fuzz.SURFACE_ROWS <= gpu_fuzz.ROW_LIMIT, c["i"]
        assert sum(ref["counts"]) == len(ref["rows"]) and len(ref["counts"]) == len(c["hays"])
        if c["ov"]:
            assert c["mk"] == 0
        # the reference, reduced by the fuzz tool, is what acx_summarize_host makes of the same rows
        want = gpu_fuzz.reduce_reference(ref, len(c["pats"]))
        any_, first, hist = capi.summarize_host(ref["rows"], ref["counts"], len(c["pats"]))
        assert [bool(v) for v in any_] == want["any"], c["i"]
        assert np.array_equal(hist, want["hist"]), c["i"]
        got = [None if int(r["pattern"]) == capi.NO_MATCH else (int(r["pattern"]), int(r["start"]), int(r["end"])) for r in first]
        assert got == want["first"], c["i"]
