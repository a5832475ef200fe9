"""What the surface slice of tools/gpu_fuzz.py (tests/test_gpu_fuzz_surface.py) covers, checked without a GPU: the plan is
deterministic, holds every entry point often enough under either build flag and every match kind, holds batches with
empty haystacks and zero-length replacements that a match really uses, and no case is large enough to be skipped."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gpu_fuzz  # noqa: E402


@pytest.fixture(scope="module")
def plan():
    return gpu_fuzz.plan_surface(gpu_fuzz.SURFACE_N, gpu_fuzz.SURFACE_SEED)


def test_plan_is_deterministic(plan):
    again = gpu_fuzz.plan_surface(gpu_fuzz.SURFACE_N, gpu_fuzz.SURFACE_SEED)
    assert len(plan) == len(again) == gpu_fuzz.SURFACE_N
    for a, b in zip(plan, again):
        assert a == b, a["i"]
    assert gpu_fuzz.plan_digest(plan) == gpu_fuzz.plan_digest(again)
    assert gpu_fuzz.plan_digest(plan) != gpu_fuzz.plan_digest(gpu_fuzz.plan_surface(11, gpu_fuzz.SURFACE_SEED + 1))


def test_plan_leaves_the_fuzz_sequence_alone(plan):
    # plan_surface borrows make_case()'s generator and puts it back
    import random
    gpu_fuzz.rng, gpu_fuzz.MAX_SIZE_LOG2 = random.Random(5), 12.0
    first = gpu_fuzz.make_case()
    gpu_fuzz.rng = random.Random(5)
    gpu_fuzz.plan_surface(3, 1)
    assert gpu_fuzz.MAX_SIZE_LOG2 == 12.0 and gpu_fuzz.make_case() == first


def test_plan_covers_the_call_surface(plan):
    assert {c["op"] for c in plan} == set(gpu_fuzz.OPS) and len(gpu_fuzz.OPS) == 11
    for op in gpu_fuzz.OPS:
        cs = [c for c in plan if c["op"] == op]
        assert len(cs) >= 8, op
        for ci in (False, True):
            assert sum(c["ci"] == ci for c in cs) >= 3, (op, ci)
        for mk in (0, 1, 2):
            assert sum(c["mk"] == mk for c in cs) >= 1, (op, mk)
    batches = [c for c in plan if len(c["hays"]) != 1 or c["op"] in gpu_fuzz.BATCH_OPS or c["op"].endswith("_uniform")]
    assert sum(any(len(h) == 0 for h in c["hays"]) for c in batches) >= 5
    assert {c["off"] for c in plan} >= set(range(1, 16, 2))  # (odd and even device pointer residues)
    assert any(c["ov"] for c in plan) and any(c["cp"] for c in plan)
    assert {len(r) for c in plan if c["repl"] for r in c["repl"]} >= {0, 1, 4, 7, 20, 64}


def test_zero_length_replacements_are_used(plan):
    # recomputed here from the reference, not taken from the plan's own flag
    used = 0
    for c in plan:
        if c["repl"] is None:
            continue
        rows = gpu_fuzz.reference(c)["rows"]
        hit = len(rows) and any(len(c["repl"][int(p)]) == 0 for p in set(rows[:, 0].tolist()))
        assert bool(hit) == c["zero_used"], c["i"]
        used += bool(hit)
    assert used >= 5


def test_no_case_can_be_skipped(plan):
    for c in plan:
        ref = gpu_fuzz.reference(c)
        assert len(ref["rows"]) == c["rows"] <= gpu_fuzz.ROW_LIMIT, c["i"]
        assert len(ref["rows"]) <= 20_000_000
        assert sum(ref["counts"]) == len(ref["rows"]) and len(ref["counts"]) == len(c["hays"])
        assert sum(len(x) for x in ref["outs"]) == c["out_bytes"]
        if c["cp"] or c["ov"]:
            assert c["op"].startswith("find")
        if c["ov"]:
            assert c["mk"] == 0
