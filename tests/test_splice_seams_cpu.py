"""The plan of tests/splice_seams.py, checked without a GPU: the model of run_chunked over the oracle IS the oracle on every
case of (a) to (d), and the model of run_batch_split cuts every batch of (g) where the sources say; every case hits the seam
it names (a record exactly at each planted position, the skip counts, prefixes of exactly 0 / 1 / 255 / 256 / 257 / n
records, out[1] on either side of hi, ranges of 0 records, copies on the first and the last record, a run across record
256) -- a condition: a case that misses its seam fails HERE, it is not dropped --; the model and
distributed.simulate_single_sharded, the rule's second statement, agree rank by rank; and the sources still hold the lines
the model restates."""
import importlib.util
import os

import numpy as np
import pytest

import k1b_seams as K
import splice_seams as P

CUT = P.cut_cases()


def _distributed():
    # (by path: the package's __init__ imports the extension module, which needs the HIP runtime's library, not a GPU)
    spec = importlib.util.spec_from_file_location("acx_distributed", os.path.join(P.ROOT, "ahocorasick_rs_amd", "distributed.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_sources_still_say_what_the_model_restates():
    P.source_constants.cache_clear()
    c = P.source_constants()
    assert (c["FLOOR_MUL"], c["FLOOR_ADD"], c["MAX_DEPTH"]) == (2, 16, 40)
    assert c["SMALL_MAX_LEN"] == 16384 and c["SMALL_PF_MAX_LEN"] == 65536 and c["SMALL_MAX_OCC"] == 1024
    assert [P.floor_of(m) for m in (1, 7, 39, 519)] == [18, 30, 94, 1054]
    # the plan's sizes against them
    assert P.G_LIMIT > c["SMALL_MAX_OCC"] < P.F_LIMIT and 5 * P.HOST_PIECE > c["SMALL_PF_MAX_LEN"] and P.HOST_PIECE + 8 <= c["SMALL_MAX_LEN"] and P.F_BYTES <= 256 << 10
    assert all(c_.piece > P.floor_of(P.max_len(c_.set) - 1) for c_ in CUT)
    assert all(len(c_.hay) <= P.SMALL_MAX_LEN for c_ in CUT)  # (through find_device: a host call this small never reaches run_find)


def test_a_pinned_line_that_changes_fails():
    """the pins are not vacuous: sources that hold one of the issue's mutants, or lack the skip, are refused"""
    for old, new in (("lo + 1, cut, st)", "lo, cut, st)"), ("if (a0 >= hi) { lo = hi; continue; }", ""), ("w % 3 ? shift : 0", "shift"),
                     ("if (nx < limit) return;", "if (nx <= limit) return;"), ("std::min(len, hi + m)", "std::min(len, hi + m - 1)"),
                     ("a0 = lo > m ? lo - m : 0", "a0 = lo > m ? lo - m + 1 : 0"), ("std::max(std::max(carry, hi), last_end)", "std::max(carry, hi)"),
                     ("upper_bound_u64(G.offsets, G.n_hay + 1, s) - 1; base", "upper_bound_u64(G.offsets, G.n_hay + 1, s); base"),
                     ("const uint64_t half = n / 2;", "const uint64_t half = (n + 1) / 2;"), ("n_later * 4 >=", "n_later * 4 >")):
        assert any(old in P.read_source(f) for f in ("find_pipeline.cpp", "kernels.hip", "build_upload.cpp")), old
        with pytest.raises(AssertionError):
            P.check_sources(lambda name: P.read_source(name).replace(old, new))
    # (a constant that changes moves the plan with it)
    assert P.check_sources(lambda name: P.read_source(name).replace("piece <= 2 * m + 16", "piece <= 2 * m + 20"))["FLOOR_ADD"] == 20


def test_the_sets_are_what_the_classes_need():
    for s in ("s8", "s40"):
        pats = P.patterns(s)
        L = pats[0]
        assert len(L) == P.max_len(s) and all(p in L for p in pats[1:4])
        assert L.startswith(pats[1]) and L.endswith(pats[3]) and 0 < L.find(pats[2]) < len(L) - len(pats[2])
        assert b"x" in pats and pats.index(b"pq") < pats.index(b"pqrs")
        # leftmost-first and leftmost-longest disagree; the chain's occurrences each begin inside the one before
        assert P.expected(s, b"-pqrs-", 1, False).tolist() != P.expected(s, b"-pqrs-", 2, False).tolist()
        chain = P.expected(s, b"kzkzkzkzk", 0, True)
        assert len(chain) >= 6 and all(int(b[1]) < int(a[2]) for a, b in zip(chain, chain[1:]))
    assert sorted(len(p) for p in P.LADDER) == list(range(1, 9)) and P.max_len("lad") == 8
    assert P.max_len("s40") - 1 > 20  # (cases_a("s40", 95, 3, 20): max_len - 1 exceeds the last range)
    for s in ("s8", "s40", "lad", "c", "u", "cp_at", "cp_below", "cp_run"):
        assert all(K.CLEAN not in p for p in P.patterns(s)), s
    assert P.n_later("cp_at") * 4 == len(P.patterns("cp_at")) and P.n_later("cp_below") * 4 == len(P.patterns("cp_below")) - 1
    assert max(P.copies_of("cp_run").values()) == 300
    capi = pytest.importorskip("ahocorasick_rs_amd.capi")
    for s in ("s8", "s40", "lad", "c", "cp_run"):  # the forced prefilter exists for every set that runs under it
        assert int(capi.HostAutomaton(list(P.patterns(s)), 0).t.filter_q) != 0, s


@pytest.mark.parametrize("cls", "abcd")
def test_the_model_over_the_oracle_is_the_oracle_and_every_case_hits_its_seam(cls):
    cases = [c for c in CUT + P.host_haystacks() + P.copy_range_cases() if c.cls == cls or (cls == "d" and c.cls == "i")]
    assert len(cases) >= 2 and len({c.name for c in cases}) == len(cases)
    bad, kinds_seen, claims_seen = [], set(), {}
    for c in cases:
        assert c.claims, c.name
        for mk, ov in c.kinds:
            got = P.model_of(c, mk, ov)
            want = P.expected(c.set, c.hay, mk, ov)
            if not (got.rows.shape == want.shape and np.array_equal(got.rows, want)):
                bad.append("%s kind %d overlapping %s: the model's rows are not the oracle's" % (c.name, mk, ov))
            if got.searched + got.skipped != -(-len(c.hay) // c.piece) or len(got.ranges) < 2:
                bad.append("%s: %d + %d ranges" % (c.name, got.searched, got.skipped))
            bad += P.check_claims(c, mk, ov, got)
            kinds_seen.add((mk, ov))
        for cl in c.claims:
            assert set(cl.kinds) <= set(c.kinds), (c.name, cl)
            claims_seen[cl.what] = claims_seen.get(cl.what, 0) + 1
    assert not bad, (len(bad), bad[:40])
    assert kinds_seen == (set(P.NOV) if cls == "b" else set(P.KINDS))
    need = {"a": {"row", "start"}, "b": {"row", "absent", "restart", "differs", "skips"}, "c": {"records", "prefix", "out1", "row"},
            "d": {"kept"}}[cls]
    assert need <= set(claims_seen), (cls, claims_seen)


def test_the_second_reference_agrees_for_standard():
    for c in CUT:
        for ov in (True, False):
            if (0, ov) in c.kinds:
                ref = (K.brute if ov else K.brute_iter)(P.patterns(c.set), c.hay)
                assert np.array_equal(ref, P.expected(c.set, c.hay, 0, ov)), (c.name, ov)


def test_class_a_plants_at_every_border_in_both_modes():
    for args in (("s8", 31, 4), ("s8", 31, 4, 11), ("s40", 95, 3), ("s40", 95, 3, 20)):
        cases = P.cases_a(*args)
        n = len(cases[0].hay)
        borders = list(range(args[1], n, args[1]))
        assert len(borders) == args[2] - 1
        names = {c.name.split("/", 3)[3] for c in cases}
        for B in borders:
            for what in ("Lend-1", "Lend", "Lend+1", "Lstart-1", "Lstart", "Lstart-m-1", "x-1", "x", "nested"):
                assert "B%d/%s" % (B, what) in names or (B == borders[-1] and len(args) == 4), (args, B, what)
        assert {"first", "last", "every"} <= names
        # nested: the front one ends before the border, the end one behind it, under the overlapping kind
        for B in borders[:-1]:
            c = next(c for c in cases if c.name.endswith("B%d/nested" % B))
            ends = sorted(int(r[2]) for r in P.expected(c.set, c.hay, 0, True) if abs(int(r[2]) - B) < P.max_len(c.set))
            assert ends[0] < B < ends[-1] and len(ends) == 4, (c.name, ends)


def test_class_c_holds_every_size_in_both_modes():
    for mode, kinds, ridx in (("ov", P.OV, 1), ("nov", P.NOV, 0)):
        seen = set()
        for c in P.cases_c():
            if not c.name.startswith(mode + "/n"):
                continue
            for mk, ov in kinds:
                r = P.model_of(c, mk, ov).ranges[ridx]
                seen.add((r.n, r.cut[0]))
                # the thread that writes: the prefix's last one -- of block 0 or 1 (2: 513 records), the last thread when all are kept
                assert r.cut[0] == 0 or r.cut[0] <= r.n
        for n in (1, 255, 256, 257, 513):
            for k in (0, 1, 255, 256, 257, n):
                assert k > n or (n, k) in seen, (mode, n, k)
    sides = {cl.args[1] for c in P.cases_c() for cl in c.claims if cl.what == "out1"}
    assert sides == {"beyond", "before"}


def test_class_d_ranges_straddle_256_words_and_one_is_empty():
    c = P.cases_d()[0]
    for mk, ov in c.kinds:
        kept = [len(r.kept) for r in P.model_of(c, mk, ov).ranges]
        assert kept[:4] == [85, 86, 0, 171] and kept[4] > 170, kept
        assert 3 * 85 < 256 < 3 * 86 and 3 * 170 < 512 < 3 * 171
        want = P.expected(c.set, c.hay, mk, ov)
        assert {int(p) for p in want[:, 0]} >= {P.pid("s8", b"x")} and int(want[-1, 1]) > 0  # (a shift would show in every id)
    z = P.cases_d()[1]
    assert all(len(P.expected(z.set, z.hay, mk, ov)) == 0 and P.model_of(z, mk, ov).searched == 4 for mk, ov in z.kinds)


def test_the_batch_model_cuts_where_the_sources_say():
    """half = n / 2, a part of one haystack is a call of its own; every batch's rows are its haystacks' own"""
    split_sizes, heavy_alone = set(), 0
    for b in P.batches_g():
        off = P.batch_offsets(b)
        assert not b.uniform or len({len(h) for h in b.hays}) == 1, b.name
        for mk, ov in P.KINDS:
            cuts, t = P.batch_tree(b, mk, ov, P.G_LIMIT)
            rows = [len(r) for r in P.batch_expected(b, mk, ov)]
            assert (t.splits > 0) == (sum(rows) >= P.G_LIMIT), b.name
            for lo, half in cuts:
                assert 0 <= lo < half < len(b.hays)
            if cuts:
                assert cuts[0] == (0, len(b.hays) // 2)
                split_sizes.add(len(b.hays))
            if b.name.startswith("heavy"):
                h = b.hays.index(P.HEAVY)
                assert rows[h] >= P.G_LIMIT > sum(rows) - rows[h] and t.ranges >= t.splits + 2, (b.name, t.ranges, t.splits)
                assert len(b.hays) == 1 or off[h] % 16 != 0, (b.name, off[h])
                heavy_alone += 1
            elif b.name != "all_empty/n5" and len(b.hays) > 1:
                assert t.splits >= 1, b.name
    assert split_sizes == {2, 3, 4, 5, 9} and heavy_alone == 6 * 2 * 4
    names = {b.name for b in P.batches_g()}
    for n in (3, 4, 5, 9):
        assert {"empty@%d/n%d" % (at, n) for at in (n // 2 - 1, n // 2, n // 2 + 1) if at < n} <= names
    assert {"empties_front_end/n9", "all_empty/n5"} <= names


def test_class_h_names_what_it_holds():
    by = {b.name: b for b in P.batches_h()}
    for b in by.values():
        assert not b.uniform or len({len(h) for h in b.hays}) == 1, b.name
    b = by["first_and_last_byte"]
    rows = P.batch_expected(b, 0, True)
    assert [0, 0, 8] in rows[0].tolist() and [0, 8, 16] in rows[2].tolist() and len(rows[4]) == 1
    b = by["split_across_two"]
    rows = P.batch_expected(b, 0, True)
    assert [len(r) for r in rows] == [1, 1, 0, 0, 1] and not any(0 in r[:, 0] for r in rows if len(r))  # ("abc" | "fgh" | "x")
    # (the stream as ONE haystack does hold the longest pattern, and "abc" across the third border)
    assert sorted(P.expected("s8", b"".join(b.hays), 0, True)[:, 0].tolist()) == [0, 1, 1, 2, 3, 4]
    b = by["empties_around"]
    assert [len(r) for r in P.batch_expected(b, 0, True)] == [0, 0, 4, 0, 1, 0, 0, 1, 0]
    assert [len(h) for h in by["uniform1"].hays] == [1] * 7 and len(by["uniform_max_len"].hays[0]) == P.max_len("s8")
    assert len(by["uniform13"].hays[0]) % 16 == 13
    for name in ("behind_2_3_4_bytes", "behind_2_3_4_bytes_uniform"):
        b = by[name]
        widths = {len(h.decode()[-1].encode()) for h in b.hays[:-1]}
        assert {2, 3, 4} <= widths and b.codepoints, (name, widths)
        assert all(len(r) for r in P.batch_expected(b, 0, True)), name


def test_the_copies_are_where_the_cases_say():
    seen = set()
    for c in P.copy_cases():
        pats = P.patterns(c.set)
        many = {p for p in pats if pats.count(p) > 1}
        rows = P.expected(c.set, c.hay, 0, True).tolist()
        occ = sorted({(e, -(e - s), pats[i]) for i, s, e in rows})  # the unexpanded result: one record per string and place
        assert len(rows) == sum(pats.count(p) for _, _, p in occ)
        for cl in c.claims:
            if cl == "first":
                ok = pats[rows[0][0]] in many
            elif cl == "last":
                ok = pats[rows[-1][0]] in many
            elif cl == "run300":
                run = [k for k, (_, _, p) in enumerate(occ) if pats.count(p) == 301]
                at = sum(pats.count(p) for _, _, p in occ[:run[0]])  # the run's first record: it must cross record 256
                ok = bool(run) and at < 256 < at + 301
            elif cl == "n1":
                ok = len(occ) == 1 and len(rows) > 1
            elif cl == "none":
                ok = len(rows) == len(occ) > 0
            elif cl == "zero_next_to_many":
                ok = any(a[2] not in many and pats.count(b[2]) >= 3 for a, b in zip(occ, occ[1:]))
            assert ok, (c.name, cl)
            seen.add(cl)
    assert seen == {"first", "last", "run300", "n1", "none", "zero_next_to_many"}
    for b in P.copy_batches():
        n = [len(r) for r in P.batch_expected(b, 0, True)]
        pats = P.patterns(b.set)
        # haystacks without an occurrence, and empty ones, between haystacks whose occurrences carry copies
        k = [i for i, x in enumerate(n) if x == 0]
        assert any(0 < i < len(n) - 1 and not b.hays[i] for i in k) and any(b.hays[i] for i in k) or b.uniform, b.name
        assert any(pats.count(pats[int(r[0])]) > 1 for r in np.concatenate(P.batch_expected(b, 0, True))), b.name
    for c in P.copy_range_cases():
        got = P.model_of(c, 0, True)
        assert not P.check_claims(c, 0, True, got)
        for r in got.ranges:  # a run lies whole in one range
            ids = [int(x[0]) for x in r.kept if P.patterns(c.set)[int(x[0])] == b"ab"]
            assert len(ids) in (0, 301), (c.name, len(ids))


@pytest.mark.parametrize("world", [2, 3, 4, 5])
def test_the_model_and_the_sharded_simulation_state_one_rule(world):
    D = _distributed()

    class Adapter:  # capi.Automaton's find() and max_pattern_len, from the oracle
        def __init__(self, set_name, mk):
            self.o, self.max_pattern_len = P.oracle(set_name, mk), P.max_len(set_name)

        def find(self, hay, overlapping=False, codepoints=False):
            raw = self.o.find_raw(bytes(hay), overlapping)
            out = np.empty(len(raw), dtype=[("pattern", "<u8"), ("start", "<u8"), ("end", "<u8")])
            out["pattern"], out["start"], out["end"] = raw[:, 0], raw[:, 1], raw[:, 2]
            return out

    cases = [c for c, w in P.sharded_cases() if w == world]
    assert len(cases) >= 9
    adapters = {}
    for c in cases:
        n = len(c.hay)
        # shard_range's borders are the planted ones: the multiples of the case's piece
        assert [D.shard_range(n, r, world) for r in range(world)] == [(r * c.piece, (r + 1) * c.piece) for r in range(world)], c.name
        for mk, ov in c.kinds:
            a = adapters.setdefault((c.set, mk), Adapter(c.set, mk))
            sim = D.simulate_single_sharded(a, c.hay, world, ov)
            got = P.model_of(c, mk, ov)
            assert len(sim) == len(got.ranges) == world
            for rank, (s, r) in enumerate(zip(sim, got.ranges)):
                assert np.array_equal(K.cols(s).reshape(-1, 3), r.kept), (c.name, mk, ov, rank)
            assert not P.check_claims(c, mk, ov, got), c.name
    if world == 5:  # the occurrence that covers two borders
        two = next(c for c in cases if c.name == "two_borders")
        r = next(r for r in P.expected(two.set, two.hay, 0, True).tolist() if r[0] == 0)
        assert len([B for B in range(two.piece, len(two.hay), two.piece) if r[1] < B < r[2]]) == 2


def test_the_lower_bound_of_the_real_trigger():
    """the dense input's tree: 256 KiB in two halves; a half's window is max_len - 1 bytes longer than the half when it is
    scanned beyond its end (not overlapping: the first) or from before its start (overlapping: the second), so ITS halves
    leave a third range of a few bytes: 2 + 3 + 2 ranges"""
    pats, hay = P.dense_input()
    o = P.Oracle(list(pats), 0, P.KIND_DFA)
    find = lambda a, b, ov: o.find_raw(hay[a:b], overlapping=ov)  # noqa: E731
    m = max(len(p) for p in pats) - 1
    for ov in (False, True):
        whole = len(find(0, len(hay), ov))
        assert whole >= 2 * P.F_LIMIT and whole // 4 < P.F_LIMIT, whole
        assert P.least_ranges(find, len(hay), m, ov, P.F_LIMIT) == 7
    # a forced walk with the limit at 10: every piece down to the floor holds 10 rows or more -- ACX_ETOOBIG, no result
    t = P.Tree(P.finder("s8", b"x" * 4096, 0), 7, lambda rows: rows >= 10)
    with pytest.raises(P.TooBig):
        t.single(0, 4096, False)
