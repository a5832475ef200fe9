"""The plan of tests/post_seams.py, checked without a GPU.  The plan is a fixed list (one digest on two builds of it); the
reference is pinned twice -- the oracle's rows against bytes.find in a loop (k1b_seams.brute() / brute_iter(),
post_seams.brute_leftmost()) on every case, for all four (kind, overlapping) pairs --; and every class's geometry is
recomputed from those rows, the pointer residue and the constants, not taken from the plan's bookkeeping: the fill of every
bucket as each group stages it, per key mode; the reported matches per group; the prefix hits per tile (Q2 and the anchor
shift from capi.HostAutomaton's tables, which need no device); for the chains, which links the kernel's rule certifies; for
the batches, the match each haystack border falls behind.  A class without a case fails HERE."""
import numpy as np
import pytest

import k1b_seams as K
import post_seams as P

capi = pytest.importorskip("ahocorasick_rs_amd.capi")
CASES = P.all_cases()
MIN_SLOTS = min(f.slots for f in P.FORMS)


def test_the_sources_still_say_what_the_plan_restates():
    P.source_constants.cache_clear()
    c = P.source_constants()
    assert c["STAGE_SLOTS_W32"] <= 32 and c["STAGE_SLOTS"] <= c["STAGE_SLOTS_W32"] < c["STAGE_SLOTS_WIDE"] == c["HIT_SLOTS"] == 64
    assert c["GROUP_MAX"] == 16 * c["GROUP_TILES"] and c["STAGE_SLOTS_WIDE"] * c["GROUP_TILES"] == c["GROUP_MAX_WIDE"]
    assert c["WRITE_CHUNK"] == 256 and c["GROUP_MAX"] == 4 * c["WRITE_CHUNK"] and c["SUPER"] == 64
    assert [P.longest_for(k) for k in (1, 2, 3, 4)] == [2049, 6145, 10241, 14337]
    assert [P.tile_lookback(n) for n in (1, 2049, 2050, 14337, 14338)] == [1, 1, 2, 4, 5]


def test_the_plan_is_deterministic():
    first = P.digest()
    for f in (P.patterns, P.cases_a, P.cases_b, P.cases_c, P.cases_d, P.cases_e, P.cases_h, P.cases_f, P.cases_g, P.all_cases, P.batches, P.sequence_inputs, P.ladder_inputs):
        f.cache_clear()
    assert P.digest() == first


def test_no_class_and_no_form_is_empty():
    for f in P.FORMS:
        for cls in P.CLASSES:
            # (h: k_dense_main has one form of words; f: one stream of 33 MiB a form; d: one a lookback; g: the ACX_NO_WIDE leg's)
            least = {"f": 1, "d": 2, "g": 0}.get(cls, 4)
            assert len(P.cases_of(f.name, cls)) >= least or (cls == "h" and f.env), (f.name, cls)
    assert len(P.cases_of("nowide", "g")) == 2 and len(P.cases_of("full", "h")) == 34 and not P.cases_of("nospec", "a")
    assert len({c.name for c in CASES}) == len(CASES)
    assert len(P.batches()) == 2 and len(P.sequence_order()) == 21
    for c in CASES:
        assert set(c.stats) == set(c.kinds), c.name
        # at most 4 groups + a partial tile but (f) and the 17-hot-group shape of (g); the 10^6 rows: test_case
        assert c.lead + len(c.hay) <= 4 * P.GROUP + P.TILE or c.cls in ("f", "g"), c.name
    # every path the plan can name is named by some case of every form
    for f in P.FORMS:
        seen = {st for c in CASES if f.name in c.forms for st in c.stats.values()}
        assert {P.SPARSE, P.HOT1, P.HOT2, P.DENSE} <= seen, (f.name, seen)


@pytest.mark.parametrize("set_name", sorted({c.set for c in CASES}))
def test_each_set_has_the_tables_its_cases_assume(set_name):
    """Q2, no anchors (a hit lies at the start of its occurrence), the lookback, narrow words by itself"""
    pats = list(P.patterns(set_name))
    h = capi.HostAutomaton(pats, 0)
    assert int(h.t.filter_q2) == P.q2_of(set_name) == {"big": 8, "urls": 6}.get(set_name, 5)
    assert (int(h.t.max_shift) != 0) == (set_name == "urls")  # ANCH
    rank_bits = max(1, (len(pats) - 1).bit_length())
    assert (rank_bits + P.max_len(set_name).bit_length() <= P.C["W32_FIELD"]) == (set_name != "w4")  # tile_words_narrow()
    assert int(max(h.rank)).bit_length() <= rank_bits and (set_name != "w4" or int(max(h.rank)).bit_length() == rank_bits)
    h.close()
    lb = P.tile_lookback(P.max_len(set_name))
    assert (lb <= P.C["MAX_LOOKBACK"]) == (set_name != "L%d" % (P.longest_for(P.C["MAX_LOOKBACK"]) + 1))


def rows_of(c, mk, ov):
    """the oracle's rows in BYTES (a code-point case: of the same stream)"""
    return P.expected(c._replace(name=c.name + "/bytes", cp=False), mk, ov)


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_case(c):
    pats = P.patterns(c.set)
    occ = K.brute(pats, c.hay)
    # ---- the oracle, pinned
    assert np.array_equal(rows_of(c, 0, True), occ)
    assert np.array_equal(rows_of(c, 0, False), K.brute_iter(pats, c.hay))
    assert np.array_equal(rows_of(c, 1, False), P.brute_leftmost(pats, c.hay, False))
    assert np.array_equal(rows_of(c, 2, False), P.brute_leftmost(pats, c.hay, True))
    assert 0 < len(occ) <= 10 ** 6
    if c.cp:  # valid UTF-8, two-byte characters in front of the first plant: code points and bytes differ from the first row on
        c.hay.tobytes().decode("utf-8")
        assert (P.expected(c, 0, True)[:, 1] < occ[:, 1]).all() and len(P.expected(c, 0, True)) == len(occ)
    # ---- one cause: no tile above its hit slots (h: the dense path has none; its tail cases are hot BY their tiles' hits)
    hits = P.hits_per_tile(c.set, c.hay, c.lead)
    assert c.cls == "h" or max(hits.values()) <= P.HIT_SLOTS, (c.name, max(hits.values()))
    if c.cls == "h":
        check_dense(c, occ, hits)
    G = c.geo
    ng = P.n_groups(c.lead, len(c.hay))
    for fname in c.forms:
        f = P.FORM[fname]
        for mk, ov in c.kinds:
            km = P.key_mode(mk, ov)
            rep = rows_of(c, mk, ov)
            want = c.stats[(mk, ov)]
            if c.cls in ("a", "b", "d", "e", "f", "g") or "pairs" in G or "long" in G:
                hot = P.predicted_hot_groups(c, f, occ, rep, km)
                assert (want[2] == hot) and (want == P.SPARSE) == (hot == 0), (c.name, fname, mk, ov, hot, want)
            if c.cls == "a":
                g = min(G["bucket"] // P.GT, ng - 1)
                b = P.staged_buckets(occ, km, c.lead, g, P.max_len(c.set))
                sl = P.slots_of(c, f)
                assert b[G["bucket"]] == G["fill"] and G["fill"] in (sl - 1, sl, sl + 1)
                assert all(n < MIN_SLOTS for t, n in b.items() if t != G["bucket"])
                if G["how"] == "inside":  # the bucket's first and last key, to the byte
                    k = np.sort(P.keys_of(occ, km, c.lead))
                    k = k[k >> P.C["TILE_BITS"] == G["bucket"]]
                    first = G["bucket"] * P.TILE + P.FIRST + (len(P.S) if km == 0 else 0)
                    assert (k[0], k[-1]) == (first, first + (G["fill"] - 1) * (P.PITCH_WIDE if f.slots > 32 else P.PITCH))
                if G["how"] == "straddle":
                    assert hits[G["bucket"]] == G["fill"] - 1 and hits[G["bucket"] - 1] == 1
                if G["how"] == "anch_ahead":  # 65 keys, 64 hits in the tile, the last plant's in the look-ahead tile
                    assert hits[G["bucket"]] == G["fill"] - 1 and hits[G["bucket"] + 1] == 1 and (G["bucket"] + 1) % P.GT == 0
                    last = int(occ[:, 1].max())
                    assert last == (G["bucket"] + 1) * P.TILE - 2 and last + G["shift"] >= (G["bucket"] + 1) * P.TILE
                if G["how"] == "anch":
                    assert hits[G["bucket"]] == G["fill"] and G["shift"] >= 2
                if G["how"] == "pairs":
                    assert hits[G["bucket"]] == (G["fill"] + 1) // 2
            if c.cls in ("b", "e"):
                k = P.keys_of(rep, km, c.lead) // P.GROUP
                if G["reported"] is not None:
                    assert int(np.count_nonzero(k == G["group"])) == G["reported"]
                else:  # the full house: every bucket and every tile of the group at its slots, one bucket one above
                    b = P.staged_buckets(occ, km, c.lead, G["group"], P.max_len(c.set))
                    own = [b.get(t, 0) for t in range(G["group"] * P.GT, (G["group"] + 1) * P.GT)]
                    assert sum(own) == G["staged"] and sorted(own)[:-1] == [f.slots] * (P.GT - 1) and max(own) - f.slots == G["staged"] - P.GROUP_MAX_WIDE
                    # (the tile whose bucket takes one more by two occurrences a hit has fewer hits)
                    assert sum(hits[t] == P.HIT_SLOTS for t in range(G["group"] * P.GT, (G["group"] + 1) * P.GT)) >= P.GT - 1
                if c.cls == "e":
                    assert [int(np.count_nonzero(k == g)) for g in (0, 2)] == [P.E_FRONT, P.E_BEHIND]
    if c.cls == "f":
        check_super(c, occ)
    if c.cls == "d":
        check_prefix(c, occ, hits)
    if c.cls == "g":
        check_room(c)
    if "pairs" in G:
        check_pairs(c, occ)
    if "links" in G:
        check_chain(c, occ)
    if "long" in G:
        check_long(c, occ)


def dense_words(occ, km, g, lb=1):
    """occurrences dense group g stages: the keys in its DT_GROUP tiles and the lookback tiles in front"""
    k = P.keys_of(occ, km, 0) >> P.C["TILE_BITS"]
    return int(np.count_nonzero((k >= g * P.DT - lb) & (k < (g + 1) * P.DT)))


def check_dense(c, occ, hits):
    G = c.geo
    lb = P.tile_lookback(P.max_len(c.set))
    assert lb == (P.C["MAX_LOOKBACK"] if G.get("where") == "context" else 1) and P.n_groups(0, len(c.hay)) == 1
    for mk, ov in c.kinds:
        km = P.key_mode(mk, ov)
        tiles, n = np.unique(P.keys_of(occ, km, 0) >> P.C["TILE_BITS"], return_counts=True)
        fill = dict(zip(tiles.tolist(), n.tolist()))
        if "bucket" in G:
            assert fill == {G["bucket"]: G["fill"]}
            # first: a dense group's first tile; last: its last, context to the next group; context (lookback 4): in the middle
            # of group 1 and context to group 2
            assert {"first": G["bucket"] % P.DT == 0, "last": G["bucket"] % P.DT == P.DT - 1,
                    "context": 0 < G["bucket"] % P.DT < P.DT - 1 and (G["bucket"] // P.DT + 1) * P.DT - G["bucket"] <= lb}[G["where"]]
            assert (c.radix) == (G["fill"] > P.C["DT_SLOTS"]) and c.tiles == (bool(c.env) and not c.radix)
        if "words" in G:
            assert dense_words(occ, km, G["dense_group"]) == G["words"] and max(fill.values()) <= P.C["DT_SLOTS"]
            assert all(dense_words(occ, km, g) <= G["words"] for g in range(6))
        else:
            assert all(dense_words(occ, km, g, lb) <= P.C["DT_COMPACT_WORDS"] for g in range(6)) or c.radix
        if "dense_pair" in G:
            (s1, s2), L, bd = G["dense_pair"], G["len"], G["border"]
            k1, k2 = (s1 + L, s2 + L) if km == 0 else (s1, s2)
            assert {(s1, s1 + L), (s2, s2 + L)} <= {(int(x), int(e)) for _, x, e in occ.tolist()}
            assert bd % (P.DT * P.TILE) == 0 and bd % P.GROUP and k1 < bd == k2 and (s1 + L) - s2 in (0, 1)
            # a dense group whose first own occurrence has nothing in front of it: its first sync point lies AT out0
            lone = 4 * P.DT
            assert fill[lone] == 1 and lone - 1 not in fill
            assert c.env or max(fill.values()) > P.FORMS[0].slots  # the tail leg: a full bucket behind the pair
        if "big" in G:
            s, e = G["big"]
            inside = occ[(occ[:, 1] >= s) & (occ[:, 2] <= e) & (occ[:, 0] == 0)]
            assert len(inside) == 250 and s // (P.DT * P.TILE) + 1 == e // (P.DT * P.TILE)
            assert len(P.expected(c, 2, False)) == 1  # LeftmostLongest: the long one covers them all
    if not c.env and "bucket" in G:  # the hot pipeline's tail: hot by the tile's hits or by the bucket's fill
        assert hits[G["bucket"]] > P.HIT_SLOTS or G["fill"] > P.FORMS[0].slots


def check_prefix(c, occ, hits):
    """every whole tile of groups 0 and 1 holds d_hits() hits: 1 .. 64 over the first 64 staged tiles of group 1, the seam
    63 | 64 between the waves' halves at 64 | 1, on from there for the lanes that add tail_base; the occurrences are the
    tiles' LAST hits"""
    lb = c.geo["lookback"]
    assert P.tile_lookback(P.max_len(c.set)) == lb and lb in (1, P.C["MAX_LOOKBACK"])
    first = P.GT - lb
    staged = [hits[first + t] for t in range(P.GT + lb)]
    assert staged[:64] == list(range(1, 65)) and staged[64:] == list(range(1, lb + 1)) and len(staged) == 64 + lb
    assert all(hits[t] == P.d_hits(t, lb) for t in range(2 * P.GT))  # (group 0, lb = 0: its own 64 tiles, another rotation)
    assert len(set(np.cumsum(staged).tolist())) == len(staged)
    last = {}
    a = c.hay.tobytes()
    for _, x, e in occ.tolist():
        assert e - x == len(P.S) and a.find(b"-" * 8, int(e), int(e) + 8) == int(e)  # nothing behind it in its tile
        last[int(x) >> P.C["TILE_BITS"]] = int(x)
    assert {first + 62, first + 63, first + 64, 2 * P.GT - 1, P.GT - 1, P.GT} <= set(last) and len(last) == len(occ) >= 20
    assert all((x & (P.TILE - 1)) == 8 + (hits[t] - 1) * P.D_PITCH for t, x in last.items())


def check_room(c):
    n_hot, groups = c.geo["hot"], c.geo["groups"]
    cap, bound = P.room_for_hot(groups, n_hot)
    assert ng_of(c) == groups >= 4 * n_hot + 1 and groups >= 32 and n_hot * 32 > groups  # not held dense; WOULD be redone wide
    assert (bound > cap) == (n_hot > P.C["HOT_INLINE"])  # HOT_INLINE + 1: hot_totals and the exact-size buffer


def check_super(c, occ):
    """group g reports g % 7 + 1 matches but the two hot ones, which straddle the border of supergroups 0 and 1; no two
    groups start at the same place of the output"""
    S_ = P.C["SUPER"]
    assert ng_of(c) == 2 * S_ + 3 and c.geo["hot"] == (S_ - 1, S_) and (S_ - 1) // S_ != S_ // S_
    for mk, ov in c.kinds:
        rep = P.expected(c, mk, ov)
        per = np.bincount(P.keys_of(rep, P.key_mode(mk, ov), 0) // P.GROUP, minlength=ng_of(c))
        assert all(per[g] == g % 7 + 1 for g in range(ng_of(c)) if g not in c.geo["hot"])
        assert all(per[g] > 7 for g in c.geo["hot"]) and len(set(np.cumsum(per).tolist())) == ng_of(c)


def ng_of(c):
    return P.n_groups(c.lead, len(c.hay))


def check_pairs(c, occ):
    """o1's key is the last of its bucket, o2's key the first of the next one, at each of the three borders; they touch or
    overlap by one byte; at the tight variant one of the two keys sits ON the border's byte"""
    G, km = c.geo, c.km
    spans = {(int(x), int(e)) for _, x, e in occ.tolist()}
    keys = np.sort(P.keys_of(occ, km, 0))
    assert P.tile_lookback(P.max_len(c.set)) == G["lookback"]
    assert sorted(G["borders"].values()) == [(P.GT - G["lookback"]) * P.TILE, P.GT * P.TILE, (P.GT + 6) * P.TILE]
    for name, (s1, s2) in G["pairs"].items():
        bd, L = G["borders"][name], G["len"]
        assert (s1, s1 + L) in spans and (s2, s2 + L) in spans and (s1 + L) - s2 in (0, 1)
        k1, k2 = (s1 + L, s2 + L) if km == 0 else (s1, s2)
        assert k1 < bd <= k2 and (k2 == bd or k1 == bd - 1), (c.name, name, k1, k2, bd)
        b = keys[(keys >> P.C["TILE_BITS"]) == bd >> P.C["TILE_BITS"]]
        assert b[0] == k2  # the bucket's first: its chain starts here if it is certified
        rep = {(int(x), int(e)) for _, x, e in P.expected(c, c.kinds[0][0], False).tolist()}
        assert ((s2, s2 + L) in rep) == ((s1 + L) == s2)  # the overlapping second one is not reported


def check_chain(c, occ):
    """group 1's staged links by the kernel's rule: some link certified iff the plan says so; the shadowed first link is
    not reported"""
    G = c.geo
    first_idx, margin = G["first_idx"], G["margin"]
    assert first_idx == (P.GT - P.tile_lookback(P.max_len(c.set))) * P.TILE and margin == P.max_len(c.set) - 1
    LL = G["link_len"]
    links = [(s, s + LL) for s in G["links"]]
    assert {(int(x), int(e)) for _, x, e in occ.tolist()} == set(links)
    assert all(b[0] == a[1] - 1 for a, b in zip(links, links[1:]))  # each overlaps the next by one byte
    for km in (0, 1):
        complete = first_idx + (margin if km == 0 else 0)
        staged = sorted((s, e) for s, e in links if complete <= (e if km == 0 else s) < 2 * P.GROUP)
        cert = P.certified(staged, first_idx, margin)
        assert any(cert) == G["certifiable"], (c.name, km)
        if G["certifiable"]:
            assert cert[0] and staged[0][0] == first_idx + margin
        else:
            assert (first_idx + margin - 1, first_idx + margin - 1 + LL) in staged
        # the links reach the group's output, a bucket holds fewer than any form's slots
        assert max(e for _, e in staged) > P.GROUP + P.TILE and len(staged) >= 3
        assert max(P.staged_buckets(occ, km, 0, 1, P.max_len(c.set)).values()) < MIN_SLOTS
    if c.name.endswith("shadowed"):
        for mk in (0, 1, 2):
            rep = [int(x) for _, x, _ in P.expected(c, mk, False).tolist()]
            assert rep[:2] == [first_idx - 1, first_idx + margin - 1 + LL - 1]


def check_long(c, occ):
    G, km = c.geo, c.km
    (s1, e1), (s2, e2) = G["long"], G["short"]
    spans = {(int(x), int(e)) for _, x, e in occ.tolist()}
    assert spans == {(s1, e1), (s2, e2)} and e1 - s1 == P.longest_for(G["lookback"]) == P.max_len(c.set)
    assert ((e1 if km == 0 else s1) + 1) % P.TILE == 0 and e1 - s2 in (0, 1)
    assert s1 // P.GROUP == 1 and e2 // P.GROUP == 1
    if km == 1:  # the buckets between the two keys are empty
        assert (s2 >> P.C["TILE_BITS"]) - (s1 >> P.C["TILE_BITS"]) == G["lookback"]
    for mk, ov in c.kinds:
        assert len(P.expected(c, mk, ov)) == (2 if ov or e1 == s2 else 1)


@pytest.mark.parametrize("b", P.batches(), ids=lambda b: b.name)
def test_batch(b):
    bd = P.batch_bounds(b)
    assert bd[0] == 0 and bd[-1] == len(b.hay) and (np.diff(bd) >= 0).all()
    whole = P.oracle("p", 0).find_raw(b.hay, overlapping=True).astype(np.int64)
    assert np.array_equal(whole, K.brute(P.patterns("p"), b.hay).astype(np.int64))
    assert max(P.hits_per_tile("p", b.hay, 0).values()) < MIN_SLOTS
    # no haystack border cuts an occurrence: the haystacks' rows together are the stream's
    hs = np.searchsorted(bd, whole[:, 1], side="right") - 1
    assert (whole[:, 2] <= bd[hs + 1]).all()
    for mk, ov in K.KINDS:
        rows, counts = P.batch_expected(b, mk, ov)
        assert len(rows) == len(whole) == counts.sum() and len(counts) == len(bd) - 1
        assert np.array_equal(counts, np.bincount(hs, minlength=len(bd) - 1).astype(np.uint64))
    g1 = whole[whole[:, 1] // P.GROUP == 1]
    if b.offsets:
        # the borders inside group 1's stretch, by the match they fall behind
        inside = sorted({int(np.count_nonzero(g1[:, 1] < o)) for o in bd if g1[0, 1] < o <= g1[-1, 1]})
        assert tuple(inside) == b.geo["behind"] and {P.CHUNK - 1, P.CHUNK, P.CHUNK + 1, 2 * P.CHUNK} <= set(inside)
        assert len(g1) == 2 * P.CHUNK + 1
        # a run of one haystack's matches that the chunk border cuts, and empty haystacks at a border
        i = int(np.flatnonzero(bd == bd[np.searchsorted(bd, g1[250, 1], side="right") - 1])[0])
        assert np.count_nonzero(g1[:, 1] < bd[i]) == 250 and np.count_nonzero(g1[:, 1] < bd[i + 1]) == 255
        empty = np.flatnonzero(np.diff(bd) == 0)
        assert len(empty) == 2 and np.count_nonzero(g1[:, 1] < bd[empty[0]]) == b.geo["empty_at"] == P.CHUNK
        # ... and one whose run IS cut: matches 250 .. 254 lie in chunk 0, a run that crosses 255 | 256 does not exist
        # (a border lies there) -- the cut run is 260 .. 511 | 512: the long haystack's
        j = int(np.searchsorted(bd, g1[300, 1], side="right") - 1)
        assert np.count_nonzero(g1[:, 1] < bd[j]) == 260 and np.count_nonzero(g1[:, 1] < bd[j + 1]) == 2 * P.CHUNK
    else:
        per = np.bincount(hs, minlength=len(bd) - 1)
        rows_g1 = np.unique(g1[:, 1] // b.row_length)
        assert len(g1) == len(rows_g1) == b.geo["rows_in_group_1"] > P.CHUNK and per.max() == 1
        assert rows_g1[-1] - rows_g1[0] == len(rows_g1) - 1  # one after the other: a chunk of 256 runs of one


@pytest.mark.parametrize("form", P.FORMS, ids=lambda f: f.name)
def test_grow_and_redo(form):
    """small -> large -> small: the large stream has more than SUPER groups (sg_cap 3 > n_super 1 behind it), two small calls
    follow it (one of either parity); the redone call: 32 groups, two hot ones by the form's own slots"""
    grow = P.named_sequence(form.name, "grow")
    sizes = [P.n_groups(0, len(h)) for _, h, _, _ in grow]
    assert sizes[:4] == [1, P.F_GROUPS, 1, 1] and P.F_GROUPS > 2 * P.C["SUPER"]
    if form.gmax == P.GROUP_MAX:
        for name, hay, path, more in P.named_sequence(form.name, "redo"):
            occ = K.brute(P.patterns("p"), hay)
            c = P.Case(name, "g", "p", (form.name,), None, 0, hay, {}, {})
            ng = P.n_groups(0, len(hay))
            for mk, ov in K.KINDS:
                rep = P.oracle("p", mk).find_raw(hay, overlapping=ov).astype(np.uint64)
                hot = P.predicted_hot_groups(c, form, occ, rep, P.key_mode(mk, ov))
                assert (more["wide_redone"] == 1) == (ng >= 32 and hot * 32 > ng), (name, hot, ng)
                if more["wide_redone"]:  # nothing hot in the wide form, and few enough occurrences to leave it again
                    assert P.predicted_hot_groups(c, P.FORM["wide"], occ, rep, P.key_mode(mk, ov)) == 0 and path == P.SPARSE
                    assert len(occ) * 5 < ng * P.GROUP_MAX * 2
                else:
                    assert hot == path[2]


@pytest.mark.parametrize("form", P.FORMS, ids=lambda f: f.name)
def test_sequence(form):
    ins = P.sequence_inputs(form.name)
    assert sorted(P.sequence_order()) == sorted(list(range(len(ins))) * 3)
    paths = [p for _, _, p in ins]
    assert paths.count(P.HOT1) == 3 and paths.count(P.SPARSE) == 4
    seq = P.named_sequence(form.name, "seq")
    assert [m["overflow_regrown"] for n, _, _, m in seq if n == "regrow"] == [1, 0, 0] and sum(m["overflow_regrown"] for *_, m in seq) == 1
    sizes = [len(h) for _, h, _ in ins]
    assert sizes[0] < P.GROUP < max(sizes) and sizes[-1] < max(sizes)  # the workspace grows, then serves smaller streams
    for name, hay, path in ins:
        occ = K.brute(P.patterns("p"), hay)
        top = max(P.hits_per_tile("p", hay, 0).values(), default=0)
        assert top <= P.HIT_SLOTS or (name == "regrow" and P.HIT_SLOTS + 64 < top == P.REGROW_HITS < P.C["DT_SLOTS"])
        c = P.Case(name, "g", "p", (form.name,), None, 0, hay, {}, {})
        for mk, ov in K.KINDS:
            rep = P.oracle("p", mk).find_raw(hay, overlapping=ov).astype(np.uint64)
            assert P.predicted_hot_groups(c, form, occ, rep, P.key_mode(mk, ov)) == path[2], (name, mk, ov)


@pytest.mark.parametrize("form", P.FORMS, ids=lambda f: f.name)
def test_ladder(form):
    """1 hot group, as many as the bound attempt_sparse computes behind it, the bound behind THAT + 1, none, 1"""
    ins = P.ladder_inputs(form.name)
    groups = P.n_groups(0, P.LADDER_LEN)
    assert groups == 5 and groups < 8
    hot = [p[2] for _, p in ins]
    assert hot == [1, P.spec_bound(hot[0], groups), P.spec_bound(hot[1], groups) + 1, 0, 1] == [1, 2, 5, 0, 1]
    for hay, path in ins:
        occ = K.brute(P.patterns("p"), hay)
        assert max(P.hits_per_tile("p", hay, 0).values()) <= P.HIT_SLOTS
        c = P.Case("ladder", "g", "p", (form.name,), None, 0, hay, {}, {})
        for mk, ov in K.KINDS:
            rep = P.oracle("p", mk).find_raw(hay, overlapping=ov).astype(np.uint64)
            assert P.predicted_hot_groups(c, form, occ, rep, P.key_mode(mk, ov)) == path[2], (mk, ov)


def test_every_plant_lies_where_it_was_recorded():
    """the occurrences of every stream against tests/golden/post_seams_rows.json (post_seams.write_golden() records them)"""
    import json
    want = json.load(open(P.GOLDEN))
    got = P.rows_digests()
    assert sorted(got) == sorted(want)
    assert [k for k in got if got[k] != want[k]] == []
