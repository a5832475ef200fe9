"""What the walk slice of tools/gpu_fuzz.py (plan_walk / run_walk; tests/test_gpu_fuzz_walk.py) covers, checked without a GPU,
and whether its reference can be trusted.

The reference (gpu_fuzz.reference_walk: the oracle's overlapping rows and a few lines of numpy) is held against the three
restated definitions -- test_gpu_at.definition, test_gpu_seg.definition and wp_definition.definition, the per-pattern brute
forces -- on 84 small drawn cases, every op under every (kind, flag) deal, and the host forms (acx_match_at_host,
acx_segment_host, acx_wordpiece_host) against it on those and on the whole plan: all must agree exactly.

The plan is deterministic, leaves the fuzz sequence alone, holds every op often enough under either build flag and every match
kind, and no case can be skipped.  What it reaches inside the walkers is RECOMPUTED here -- from the patterns by a plain
Python trie (dicts), or from the reference's result -- never read from a flag the plan set itself: nodes below the root with
more than AT_PROBE children that a walk really searches, roots with 256 children, the node of C with more than AT_PROBE
children, identical patterns in the result, and the seams of every feature (walk_coverage_table prints the counts with -s).

Measured on the CPU of the build box: building the plan of WALK_N = 140 cases takes 3.8 s, its references and host forms
2.3 s more; the whole file 25 s (the plan twice, the statistics, and 7 s for the digests of the two older plans)."""
import os
import sys

import numpy as np
import pytest

import wp_definition as wpd

capi = pytest.importorskip("ahocorasick_rs_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gpu_fuzz  # noqa: E402
import test_gpu_at as tat  # noqa: E402  (the restated definitions and hip_constants; their tests stay theirs)
import test_gpu_seg as tseg  # noqa: E402

FEATURES = ("match_at", "segment", "wordpiece")
PROBE, AT_TILE = tat.PROBE, tat.TILE
SEG_TILE, SEG_FAN = tseg.TILE, tseg.FAN
WP_TILE = tat.hip_constants("wp.hpp", ("WP_TILE",))["WP_TILE"]
WALKS_LOOKED_AT = 3000  # walks per case the trie statistics follow (evenly spread over the case's walks)


@pytest.fixture(scope="module")
def plan():
    return gpu_fuzz.plan_walk(gpu_fuzz.WALK_N, gpu_fuzz.WALK_SEED)


# ---------------------------------------------------------------------------
# the reference against the restated definitions, and the host forms against the reference
# ---------------------------------------------------------------------------
def brute_force(c, ctx):
    """what the per-pattern definitions of the three GPU test files give for the case"""
    feature, whole, bounds = gpu_fuzz.walk_feature(c["op"]), ctx["whole"], ctx["bounds"]
    offsets = None if c["shape"] == "find" or c["shape"].endswith("_one") else bounds
    if feature == "match_at":
        anchors = tat.anchors_of(len(whole), c["positions"], offsets)
        got = tat.definition(c["pats"], whole, anchors, c["mk"], overlapping=c["ov"], full=c["full"], fold=c["ci"], local=c["positions"] is None)
        return dict(zip(("pattern", "end", "row_offsets"), got if c["ov"] else got[:2]))
    if feature == "segment":
        return dict(zip(gpu_fuzz.WALK_COLUMNS[feature], tseg.definition(c["pats"], whole, c["mk"], offsets=offsets, utf8=c["utf8"], fold=c["ci"])))
    return dict(zip(gpu_fuzz.WALK_COLUMNS[feature], wpd.definition(c["pats"], whole, c["mk"], c["cls"], prefix=c["prefix"], M=c["max_word"],
                                                                   unk=c["unk_id"], offsets=offsets, fold=c["ci"])))


def test_the_reference_agrees_with_the_restated_definitions_and_the_host_forms():
    small = gpu_fuzz.plan_walk(6 * len(gpu_fuzz.WALK_OPS), 7, size_log2=11.0, pat_log10=2.0)
    seen = set()
    for c in small:
        ctx = gpu_fuzz._walk_ctx(c, 1 << 62)
        ref = gpu_fuzz.reference_walk(c, ctx=ctx)
        feature = gpu_fuzz.walk_feature(c["op"])
        diff = gpu_fuzz.walk_difference(feature, ref, brute_force(c, ctx))
        assert diff is None, ("the reference against the definition", c["i"], gpu_fuzz._walk_tag(c), diff)
        diff = gpu_fuzz.walk_host_form(c, ctx, ref)
        assert diff is None, ("the host form against the reference", c["i"], gpu_fuzz._walk_tag(c), diff)
        seen.add((c["op"], c["mk"], c["ci"]))
        seen.add((feature, c["shape"]))
        seen |= {(feature, k, c[k]) for k in ("ov", "full", "utf8", "row_starts") if k in c}
    assert len({x for x in seen if x[0] in gpu_fuzz.WALK_OPS}) == 6 * len(gpu_fuzz.WALK_OPS)  # every op under all six deals
    for feature in FEATURES:
        assert {x[1] for x in seen if x[0] == feature and len(x) == 2} >= {"find", "find_batch", "find_device_one", "find_device_uniform",
                                                                            "find_device_ragged"}, feature
    assert {x[1:] for x in seen if x[0] == "match_at" and len(x) == 3} == {(k, v) for k in ("ov", "full", "row_starts") for v in (False, True)}
    assert {x[2] for x in seen if x[:2] == ("segment", "utf8")} == {False, True}
    assert {c["prefix"] for c in small if "prefix" in c} >= {b"##", b"", b"@"} and {c["max_word"] for c in small if "prefix" in c} == {1, 7, 100, 1024}


def test_the_host_forms_agree_with_the_reference_on_the_whole_plan(plan):
    for c in plan:
        ctx = gpu_fuzz._walk_ctx(c, 1 << 62)
        diff = gpu_fuzz.walk_host_form(c, ctx, gpu_fuzz.reference_walk(c, ctx=ctx))
        assert diff is None, (c["i"], gpu_fuzz._walk_tag(c), diff)


# ---------------------------------------------------------------------------
# the plan as such
# ---------------------------------------------------------------------------
def test_plan_is_deterministic(plan):
    again = gpu_fuzz.plan_walk(gpu_fuzz.WALK_N, gpu_fuzz.WALK_SEED)
    assert len(plan) == len(again) == gpu_fuzz.WALK_N
    assert gpu_fuzz.walk_digest(plan) == gpu_fuzz.walk_digest(again)
    assert gpu_fuzz.walk_digest(plan[:11]) != gpu_fuzz.walk_digest(gpu_fuzz.plan_walk(11, gpu_fuzz.WALK_SEED + 1))


def test_plan_leaves_the_fuzz_sequence_and_the_other_plans_alone():
    import random
    gpu_fuzz.rng, gpu_fuzz.MAX_SIZE_LOG2 = random.Random(5), 12.0
    first = gpu_fuzz.make_case()
    gpu_fuzz.rng = random.Random(5)
    gpu_fuzz.plan_walk(3, 1)
    assert gpu_fuzz.MAX_SIZE_LOG2 == 12.0 and gpu_fuzz.make_case() == first
    # the two older plans are byte for byte what they were before the walk plan was added
    assert gpu_fuzz.plan_digest(gpu_fuzz.plan_summary(gpu_fuzz.SUMMARY_N, gpu_fuzz.SUMMARY_SEED)) == \
        "2ea28ef9b95ba17c7af2da52a8184b7e82ed04675dbe1402f80b43e70ef8d550"
    assert gpu_fuzz.plan_digest(gpu_fuzz.plan_surface(gpu_fuzz.SURFACE_N, gpu_fuzz.SURFACE_SEED)) == \
        "dd069e379a1ffcdae944fdf6d9917306c52e0004f3f280816e923d9365632dac"


def test_plan_covers_every_way_in(plan):
    assert {c["op"] for c in plan} == set(gpu_fuzz.WALK_OPS) and len(gpu_fuzz.WALK_OPS) == 14
    for op in gpu_fuzz.WALK_OPS:
        cs = [c for c in plan if c["op"] == op]
        assert len(cs) >= 8, op
        for ci in (False, True):
            assert sum(c["ci"] == ci for c in cs) >= 3, (op, ci)
        assert {c["mk"] for c in cs} == {0, 1, 2}, op
        assert {c["kernel"] for c in plan if gpu_fuzz.walk_feature(c["op"]) == gpu_fuzz.walk_feature(op)} == {None, 1, 2}
    device = [c for c in plan if not c["op"].endswith("_host")]
    assert {c["off"] for c in device} == set(range(16))  # (odd and even device pointer residues)
    assert sum(len(c["hays"]) > 1 and any(len(h) == 0 for h in c["hays"]) for c in plan) >= 10
    for feature in FEATURES:
        cs = [c for c in plan if gpu_fuzz.walk_feature(c["op"]) == feature]
        assert sum(len(c["hays"]) > 1 and any(len(h) == 0 for h in c["hays"]) for c in cs) >= 2, feature
        assert sum(c["raw"] for c in cs) >= 1 and sum(c["compressed"] for c in cs) >= 1, feature
        assert {c["shape"] for c in cs} == {"find", "find_batch", "find_device_one", "find_device_uniform", "find_device_ragged"}
    blocks = [plan[k:k + 14] for k in range(0, len(plan) - 13, 14)]
    assert all({c["op"] for c in b} == set(gpu_fuzz.WALK_OPS) and sum(c["raw"] for c in b) == 1 for b in blocks)
    at = [c for c in plan if gpu_fuzz.walk_feature(c["op"]) == "match_at"]
    assert all(c["mk"] == 0 for c in at if c["ov"]) and all(c["row_starts"] for c in at if c["full"]) and not any(c["ov"] and c["raw"] for c in at)
    wp = [c for c in plan if gpu_fuzz.walk_feature(c["op"]) == "wordpiece"]
    assert {c["max_word"] for c in wp} == {1, 7, 100, capi.WP_MAX_WORD} and {c["prefix"] for c in wp} >= {b"##", b"", b"@"}
    for c in wp:
        assert c["cls"][32] == c["cls"][10] == wpd.SPACE and (c["cls"] == wpd.ALONE).sum() in (1, 2) and (c["cls"] == wpd.SPACE).sum() in (2, 3, 4)
    assert any(c["utf8"] for c in plan if c["op"].startswith("segment") and c["name"] == "utf8")
    assert any(c["utf8"] for c in plan if c["op"].startswith("segment") and c["name"] == "bytes")


def test_no_case_can_be_skipped(plan):
    for c in plan:
        ctx = gpu_fuzz._walk_ctx(c, 1 << 62)
        assert ctx["rows"] == c["rows"] <= gpu_fuzz.SURFACE_ROWS <= gpu_fuzz.ROW_LIMIT, c["i"]
        assert ctx["n"] <= 2 ** gpu_fuzz.WALK_SIZE_LOG2 + 600 and gpu_fuzz.WALK_SIZE_LOG2 <= gpu_fuzz.SURFACE_SIZE_LOG2
        assert max(len(p) for p in c["pats"]) <= tseg.MAX_STEP  # (the segmenter takes every pattern set of the plan)


# ---------------------------------------------------------------------------
# what the plan reaches inside the walkers, recomputed
# ---------------------------------------------------------------------------
def trie_of(patterns):
    root = {}
    for p in patterns:
        node = root
        for b in p:
            node = node.setdefault(b, {})
    return root


def spread(items, n=WALKS_LOOKED_AT):
    return items if len(items) <= n else [items[k * len(items) // n] for k in range(n)]


def searches_a_wide_node(node, data, p, limit):
    """does the walk from `node` over data[p .. limit) look for a child in a node BEHIND its first one that has more than
    AT_PROBE children (the first step goes through a 256-entry table in all three kernels, the later ones through at_child)"""
    first = True
    while p < limit:
        if not first and len(node) > PROBE:
            return True
        node = node.get(data[p])
        if node is None:
            return False
        first = False
        p += 1
    return False


def statistics(c):
    """-> dict of what the case reaches, from its patterns, its inputs and the reference's result alone"""
    feature = gpu_fuzz.walk_feature(c["op"])
    fold = (lambda b: b.translate(gpu_fuzz.FOLD)) if c["ci"] else (lambda b: b)
    ctx = gpu_fuzz._walk_ctx(c, 1 << 62)
    ref = gpu_fuzz.reference_walk(dict(c, unk_id=-1), ctx=ctx)
    n, bounds, data, raw = ctx["n"], ctx["bounds"], fold(ctx["whole"]), ctx["whole"]
    folded = [fold(p) for p in c["pats"]]
    root = trie_of(folded)
    twins = {}
    for i, p in enumerate(folded):
        twins.setdefault(p, []).append(i)
    twin = np.zeros(len(folded) + 1, dtype=bool)
    twin[[i for v in twins.values() if len(v) > 1 for i in v]] = True
    s = {"feature": feature, "root_256": len(root) == 256}
    row_end = lambda p: int(bounds[np.searchsorted(bounds, p, side="right")])
    if feature == "match_at":
        pos, ids = c["positions"], ref["pattern"]
        if pos is None:
            walks = [(int(a), int(b)) for a, b in zip(bounds[:-1], bounds[1:]) if b > a]
            lens = np.diff(bounds)
            s.update(last_byte=bool((lens == 1).any()), empty_row=bool((lens == 0).any()), outside=False, tiles=len(lens) > AT_TILE)
        else:
            inside = pos[(pos >= 0) & (pos < n)]
            walks = [(int(p), row_end(p)) for p in spread(inside.tolist())]
            lens = np.diff(bounds)
            s.update(last_byte=bool(np.isin(inside, bounds[1:][lens > 0] - 1).any()), empty_row=bool(np.isin(pos, bounds[:-1][lens == 0]).any()),
                     outside=bool(((pos < 0) | (pos >= n)).any()), tiles=len(pos) > AT_TILE)
        if c["ov"]:
            k = np.diff(ref["row_offsets"])
            s.update(ov_0=bool((k == 0).any()), ov_1=bool((k == 1).any()), ov_2=bool((k >= 2).any()))
            listed = set(ids.tolist())
            s["twins_listed"] = any(len(v) > 1 and set(v) <= listed for v in twins.values())
        if c["full"]:
            s.update(full_hit=bool((ids >= 0).any()), full_miss=bool((ids < 0).any()))
        s["wide"] = any(searches_a_wide_node(root, data, p, L) for p, L in walks)
    elif feature == "segment":
        ids, off = ref["pattern"], ref["offsets"]
        walks = [(int(p), row_end(p)) for p in spread(off[:-1].tolist())]
        s["wide"] = any(searches_a_wide_node(root, data, p, L) for p, L in walks)
        size = np.diff(off)
        s.update(matched=bool((ids >= 0).any()), unknown=bool((ids < 0).any()), crosses=bool((off[:-1] // SEG_TILE != (off[1:] - 1) // SEG_TILE).any()),
                 entries=len(tseg.entries_taken(off, n)) if n > SEG_TILE else 0, two_levels=n > SEG_FAN * SEG_TILE)
        if c["utf8"]:
            lead = np.frombuffer(raw, dtype=np.uint8)[off[:-1]]
            want = np.where((lead >= 0xC0) & (lead <= 0xDF), 2, np.where((lead >= 0xE0) & (lead <= 0xEF), 3, np.where((lead >= 0xF0) & (lead <= 0xF7), 4, 1)))
            unk = ids < 0
            s.update({f"unit_{u}": bool((unk & (size == u) & (want == u)).any()) for u in (2, 3, 4)}, truncated=bool((unk & (size < want)).any()))
    else:
        ids, start, end, first = ref["id"], ref["start"], ref["end"], ref["first"]
        C = fold(c["prefix"])
        node = root
        for b in C:
            node = node.get(b) if node is not None else None
        word = np.cumsum(first.astype(np.int64)) - 1                                   # the word of every piece
        we = np.zeros(int(first.sum()), dtype=np.int64)
        we[word] = end                                                # (the last piece of a word writes last)
        starts = [(root if f else node, int(p), int(we[w])) for f, p, w in zip(first.tolist(), start.tolist(), word.tolist())]
        s["wide"] = any(searches_a_wide_node(at, data, p, L) for at, p, L in spread(starts) if at is not None)
        s["c_wide"] = node is not None and len(node) > PROBE and bool((first == 0).any())
        s.update(zip(("multi", "by_step", "by_length"), wpd.fuzz_shows_all_three({"M": c["max_word"]}, tuple(ref.values()))))
        ws = start[first == 1]
        s.update(crosses=bool((ws // WP_TILE != (we - 1) // WP_TILE).any()), no_node=node is None, empty_c=len(C) == 0,
                 c_is_met=bool(len(C) and C in twins and (first == 1)[np.isin(ids, twins[C])].any()))
    s["twin"] = bool(twin[ids[ids >= 0]].any())
    return s


def count(stats, key, feature=None):
    return sum(bool(s.get(key)) for s in stats if feature is None or s["feature"] == feature)


def walk_coverage_table(stats) -> str:
    lines = [f"{'':28s} " + " ".join(f"{f:>10s}" for f in FEATURES)]
    for key, what in (("wide", f"a node of > {PROBE} children searched"), ("root_256", "a root with 256 children"), ("twin", "a twin in the result")):
        lines.append(f"{what:28s} " + " ".join(f"{count(stats, key, f):10d}" for f in FEATURES))
    rest = {"match_at": ("twins_listed", "ov_0", "ov_1", "ov_2", "full_hit", "full_miss", "last_byte", "empty_row", "outside", "tiles"),
            "segment": ("matched", "unknown", "unit_2", "unit_3", "unit_4", "truncated", "crosses", "two_levels"),
            "wordpiece": ("c_wide", "multi", "by_step", "by_length", "crosses", "no_node", "empty_c", "c_is_met")}
    for f in FEATURES:
        lines.append(f"{f}: " + ", ".join(f"{k} {count(stats, k, f)}" for k in rest[f]))
    lines.append("segment: most distinct tile entries in one case %d" % max(s.get("entries", 0) for s in stats))
    lines.append("wordpiece: cases with all three of fuzz_shows_all_three %d" % sum(s["feature"] == "wordpiece" and s["multi"] and s["by_step"] and s["by_length"] for s in stats))
    return "\n".join(lines)


@pytest.fixture(scope="module")
def stats(plan):
    out = [statistics(c) for c in plan]
    print()
    print(gpu_fuzz.walk_coverage_table(plan))
    print(walk_coverage_table(out))
    return out


def test_the_trie_and_identical_patterns(stats):
    for f in FEATURES:
        assert count(stats, "wide", f) >= 3, f    # at_child's binary search behind the first step
        assert count(stats, "root_256", f) >= 1, f
        assert count(stats, "twin", f) >= 2, f
    assert count(stats, "c_wide", "wordpiece") >= 3  # cont_next is filled by the search
    assert count(stats, "twins_listed", "match_at") >= 1  # overlapping: both twins are listed


def test_match_at_seams(stats):
    for key in ("ov_0", "ov_1", "ov_2", "full_hit", "full_miss", "last_byte", "empty_row", "outside", "tiles"):
        assert count(stats, key, "match_at") >= 1, key
    assert any(s.get("ov_0") and s.get("ov_1") and s.get("ov_2") for s in stats)
    assert any(s.get("full_hit") and s.get("full_miss") for s in stats)


def test_segment_seams(stats):
    assert sum(bool(s.get("matched") and s.get("unknown")) for s in stats) >= 3
    for key in ("unit_2", "unit_3", "unit_4", "truncated", "crosses", "two_levels"):
        assert count(stats, key, "segment") >= 1, key
    assert max(s.get("entries", 0) for s in stats) >= 3


def test_wordpiece_seams(stats):
    wp = [s for s in stats if s["feature"] == "wordpiece"]
    assert sum(s["multi"] and s["by_step"] and s["by_length"] for s in wp) >= 5
    for key in ("multi", "by_step", "by_length", "crosses", "no_node", "empty_c", "c_is_met"):
        assert count(stats, key, "wordpiece") >= 1, key
