"""The plan of tests/verify_seams.py, checked without a GPU.  Two duties: the reference is pinned -- the oracle's
overlapping Standard rows against brute(), bytes.find in a loop, on every verify haystack and every batch row --, and the
plan is shown to reach every class it is there for, counted from the oracle's matches and the host compiler's own tables
(capi.HostAutomaton needs no device): a class without a case fails HERE, nothing is skipped on the device."""
import numpy as np
import pytest

import verify_seams as V

C = V.C


def reported(name, mk=0, ov=True):
    return set(map(tuple, V.expected(name, mk, ov).tolist()))


def span(name, p):
    return (p.pid, p.x, p.x + len(V.patterns(name)[p.pid]))


def test_the_plan_is_a_fixed_list():
    assert V.plan() == ("q3", "q4", "q5", "q6", "q7", "q8", "sentinel", "lists", "urls", "pw64x14337", "pw65x8191", "pw65x8192",
                        "pw128x8191", "pw16384x63", "pw16384x64", "pw16385x31", "pw16385x32")
    assert len(V.plan()) == 17 and len(V.VERIFY_SETS) == 9 and len(V.packed_rows()) == 8
    for n in V.VERIFY_SETS:
        assert len(V.case(n).plants) >= 40 and len(V.rows(n, False)) >= 40 and len(V.rows(n, True)) >= 40, n
    for r in V.packed_rows():
        assert len(V.packed_case(r.name).plants) >= 40 and len(V.packed_dense_case(r.name).plants) >= 10, r.name


def test_constants_are_what_the_plan_assumes():
    assert V.TILE == 4096 and V.HAY_LEN == 2 * C["GROUP_TILES"] * 4096 + 5000 <= 1 << 20
    assert C["FILTER2_MAX_Q"] == 8 and C["SHIFT_MAX"] == 12 and max(V.REQUIRED_SHIFTS) == C["SHIFT_MAX"]
    assert [V.d_of(q) for q in (3, 4, 5, 6, 7, 8)] == [15, 16, 16, 16, 16, 16]
    assert C["REL_BITS"] >= C["TILE_BITS"] + V.bits_for(C["GROUP_TILES"] + C["MAX_LOOKBACK"] - 1)
    assert V.longest_sparse() == 14337 and V.bits_for(V.longest_sparse()) == 14
    # the longest haystack of any route
    assert max(len(V.hot_hay(n)) for n in V.VERIFY_SETS) == 2 * V.GROUP < V.HAY_LEN <= 1 << 20
    assert max(r.n for r in V.packed_rows()) == 16385


@pytest.mark.parametrize("name", V.VERIFY_SETS)
def test_the_oracle_is_brute_force(name):
    pats, c = V.patterns(name), V.case(name)
    assert np.array_equal(V.expected(name, 0, True), V.brute(pats, c.hay))
    for ragged in (False, True):
        for r, want in zip(V.rows(name, ragged), V.row_expected(name, ragged, 0, True)):
            assert np.array_equal(want, V.brute(pats, r.data)), (name, ragged, r.pid, r.what)
    for h in (V.hot_hay(name),) + tuple(V.k0_pieces(name)[-3:]):
        assert np.array_equal(V.rows_of(name, h, 0, True), V.brute(pats, h)), name
    # no byte of the filler or of a near miss in a pattern; the four searches differ
    assert not {V.FILL, V.MISS} & set(b"".join(pats))
    assert len({V.expected(name, mk, ov).tobytes() for mk, ov in V.KINDS}) == 4, name


@pytest.mark.parametrize("name", V.VERIFY_SETS)
def test_every_true_copy_is_reported_and_no_near_miss(name):
    rep, c = reported(name), V.case(name)
    true = [p for p in c.plants if p.k < 0]
    miss = [p for p in c.plants if p.k >= 0]
    assert true and all(span(name, p) in rep for p in true)
    assert miss and not any(span(name, p) in rep for p in miss)
    q = V.q2_of(name)
    for p in miss:  # a near miss IS one: the bytes the prefix table is keyed on are whole, one byte behind them is not
        data = bytes(c.hay[p.x:p.x + len(V.patterns(name)[p.pid])])
        want = V.patterns(name)[p.pid]
        assert [k for k in range(len(want)) if data[k] != want[k]] == [p.k] and data[p.k] == V.MISS, (name, p)
        assert p.k >= q or name == "urls", (name, p)
    # sparse: no tile near the 24 occurrences a bucket of k_tile_main stages or the 64 hits it has slots for
    occ = V.expected(name, 0, True)
    for col in (1, 2):
        assert np.unique(occ[:, col] // V.TILE, return_counts=True)[1].max() <= 16, name
    assert np.unique(np.array([p.x for p in c.plants]) // V.TILE, return_counts=True)[1].max() <= 48, name
    # the last byte of the longest pattern is the haystack's last; a copy across the group boundary; one that ends with a
    # tile and one that begins the next; copies across tile boundaries
    last = V.expected(name, *V.LL)[-1]
    assert last[2] == V.HAY_LEN and last[2] - last[1] == max(len(p) for p in V.patterns(name))
    assert {p.what for p in c.plants} == {"true", "miss", "group", "before", "after", "end"}
    rows = V.expected(name, 0, True)
    assert ((rows[:, 1] < V.GROUP) & (rows[:, 2] > V.GROUP)).any()
    assert (rows[:, 2] == V.GROUP + 8 * V.TILE).any() and (rows[:, 1] == V.GROUP + 8 * V.TILE).any()
    ends = np.array([p.x + len(V.patterns(name)[p.pid]) - 1 for p in c.plants])
    assert ((np.array([p.x for p in c.plants]) // V.TILE) != (ends // V.TILE)).sum() >= (3 if len(c.plants) > 200 else 1)


@pytest.mark.parametrize("q", [3, 4, 5, 6, 7, 8])
def test_q2_sets(q):
    name = f"q{q}"
    q2, max_shift, shifts, lists, _, singles, _ = V.host_tables(name)
    tg = V.tagged(name)
    assert q2 == q == V.q2_of(name) == min(len(p.data) for p in tg) and max_shift == 0 and set(shifts) == {0}
    d = V.d_of(q)
    lengths = V.lengths_of(q)
    assert {L - d for L in lengths} >= set(V.OFFSETS) and set(lengths) >= {q + 1, q + 11, q + 12, q + 13, 15, 16, 17}
    # A<L>: one candidate each; B<L> and the shortest pattern: ONE list
    assert singles == len(lengths) and lists == (len(lengths) + 1,)
    rep, c = reported(name), V.case(name)
    for kind in "AB":
        for L in lengths:
            (pid,) = [i for i, p in enumerate(tg) if p.tag == (kind, L)]
            assert len(tg[pid].data) == L
            mine = [p for p in c.plants if p.pid == pid]
            assert sum(p.k < 0 and span(name, p) in rep for p in mine) >= 1, (name, kind, L)
            got = {p.k for p in mine if p.k >= 0}
            want = set(range(q, L)) if L <= 64 else \
                set(range(q, d + 40)) | set(range(L - 9, L)) | {k for k in range(q, L) if (k - d) % 8 in (0, 7)}
            assert got == want == set(V.miss_bytes(q, L)), (name, kind, L, sorted(want - got))
    # every piece of two in-place rounds has a near miss in its first and in its last byte
    L = d + 65
    for k in range(8):
        assert {d + 8 * k, d + 8 * k + 7} <= set(V.miss_bytes(q, L))
    assert L - 1 == d + 2 * V.ROUND and L - 1 in V.miss_bytes(q, L)  # (a third round for ONE byte)


def test_sentinel_set():
    tg, name = V.tagged("sentinel"), "sentinel"
    assert sorted(len(p.data) for p in tg) == [254, 254, 255, 255, 256, 256, 257] and V.host_tables(name)[0] == 8
    assert V.SENTINEL == 255 and V.host_tables(name)[3] == (4,)  # (the four nested ones: one list)
    x = tg[1].data
    assert [tg[i].data for i in (0, 2, 3)] == [x[:255], x[:254], x[:256]]
    rep, c = reported(name), V.case(name)
    for i, p in enumerate(tg):
        L = len(p.data)
        mine = [pl for pl in c.plants if pl.pid == i]
        assert any(pl.k < 0 and span(name, pl) in rep for pl in mine)
        assert {pl.k for pl in mine if pl.k >= 0} >= {L - 1} | ({254} if L > 254 else set()), (i, L)
    # a wrong length changes the winner: the leftmost kinds pick different members where the longest one lies
    first = {tuple(r) for r in V.expected(name, 1, False).tolist()}
    longest = {tuple(r) for r in V.expected(name, 2, False).tolist()}
    at = next(pl.x for pl in c.plants if pl.pid == 1 and pl.k < 0)
    assert (0, at, at + 255) in first and (1, at, at + 257) in longest


def test_candidate_lists():
    name = "lists"
    q2, max_shift, _, lists, _, singles, redirects = V.host_tables(name)
    assert q2 == V.LIST_Q == 5 and max_shift == 0
    # a list of 1 is a plain code in the table: the shortest pattern's and the one of ("list", 1, 0), looked up by its key
    assert set(lists) == {2, 3, 4, 5} and singles == 2 and redirects == 1
    from ahocorasick_rs_amd import capi
    tg = V.tagged(name)
    (one,) = [i for i, p in enumerate(tg) if p.tag == ("list", 1, 0)]
    h = capi.HostAutomaton(list(V.patterns(name)))
    key = int.from_bytes(tg[one].data[:8], "little")
    mine = [e for e in np.array(h.prefix_table).tolist() if e[2] != 0xFFFFFFFF and (e[1] << 32 | e[0]) == key]
    h.close()
    assert len(mine) == 1 and mine[0][2] & 15 == 8 and (mine[0][2] >> 4) & 15 == 0 and mine[0][3] == one, mine
    # n = 2 .. 5, the second copy of a member of n = 3 is filed with it; the redirect group's keys "fgh", "fga" (2) and "cde" (3)
    assert sorted(lists) == [2, 2, 2, 3, 4, 4, 5]
    tg = V.tagged(name)
    rep, c = reported(name), V.case(name)
    for n in range(1, 6):
        members = [i for i, p in enumerate(tg) if p.tag[:2] == ("list", n)]
        assert len(members) == n and len({tg[i].data[:8] for i in members}) == 1 and len({tg[i].data[8] for i in members}) == n
        for i in members:
            mine = [p for p in c.plants if p.pid == i]
            assert any(p.k < 0 and span(name, p) in rep for p in mine) and any(p.k >= 0 for p in mine), (n, i)
    red = [i for i, p in enumerate(tg) if p.tag[0] == "redirect"]
    assert len({tg[i].data[:5] for i in red}) == 1 and len({tg[i].data[:8] for i in red}) == 3 and len({len(tg[i].data) for i in red}) >= 4
    for i in red:
        assert any(p.pid == i and p.k < 0 and span(name, p) in rep for p in c.plants), i
    # the copy: both ids by the overlapping search, the lower one by the others
    (cp,) = [i for i, p in enumerate(tg) if p.tag[0] == "copy"]
    orig = next(i for i, p in enumerate(tg) if p.data == tg[cp].data)
    assert orig < cp
    at = next(p.x for p in c.plants if p.pid == cp and p.k < 0)
    assert {(orig, at, at + len(tg[cp].data)), (cp, at, at + len(tg[cp].data))} <= rep
    for mk in (1, 2):
        r = V.expected(name, mk, False)
        assert orig in r[r[:, 1] == at][:, 0] and cp not in r[:, 0]


def test_anchored_set():
    name = "urls"
    q2, max_shift, shifts, _, _, _, _ = V.host_tables(name)
    reached = sorted(set(shifts) - {0})
    assert set(reached) >= set(V.REQUIRED_SHIFTS) and max_shift == C["SHIFT_MAX"], reached
    assert reached == list(range(1, 13))  # what the set reaches: every shift there is
    rep, c = reported(name), V.case(name)
    pats = V.patterns(name)
    for s in reached:
        ids = [i for i in V.row_patterns(name) if shifts[i] == s]
        assert ids, s
        ks = {p.k for p in c.plants if p.pid in ids and p.k >= 0}
        L = {len(pats[i]) for i in ids}
        assert ks >= set(range(s)) | {s} and any(l - 1 in ks for l in L), (s, sorted(ks))
        for ragged in (False, True):
            rs, ex = V.rows(name, ragged), V.row_expected(name, ragged, 0, True)
            first = [(r, e) for r, e in zip(rs, ex) if r.pid in ids and r.what == "first"]
            assert first and all(any(row[0] == r.pid and row[1] == 0 for row in e.tolist()) for r, e in first), s  # back < shift
            cut = [(r, e) for r, e in zip(rs, ex) if r.pid in ids and r.what == "cut-b" and r.c in (1, s)]
            assert {r.c for r, _ in cut} == {1, s} and not any(row[0] == r.pid for r, e in cut for row in e.tolist()), s


@pytest.mark.parametrize("name", V.VERIFY_SETS)
def test_rows(name):
    pats = V.patterns(name)
    for ragged in (False, True):
        rs, ex = V.rows(name, ragged), V.row_expected(name, ragged, 0, True)
        offs = V.offsets_of(rs)
        blob = b"".join(r.data for r in rs)
        if ragged:
            assert {o % 16 for o in offs} == set(range(16)) and sum(1 for r in rs if not r.data) >= 2
        else:
            assert {len(r.data) for r in rs} == {V.row_len(name)}
        for i in V.row_patterns(name):
            mine = [(k, r, e) for k, (r, e) in enumerate(zip(rs, ex)) if r.pid == i]
            L = len(pats[i])
            flush = [(r, e) for _, r, e in mine if r.what == "flush"]
            assert len(flush) == 1 and [i, len(flush[0][0].data) - L, len(flush[0][0].data)] in flush[0][1].tolist()
            short = [(k, r, e) for k, r, e in mine if r.what == "short"]
            assert len(short) == 1 and short[0][1].data.endswith(pats[i][:-1])
            for k, r, e in mine:
                if r.what in ("short", "cut-a"):  # contiguous in the blob, a match in neither row
                    assert rs[k + 1].what == "cut-b" and blob[offs[k + 1] - r.c:offs[k + 1] - r.c + L] == pats[i]
                    assert i not in e[:, 0] or all(row[2] - row[1] != L or row[0] != i for row in e.tolist())
                    assert not any(row[0] == i and row[1] < L for row in ex[k + 1].tolist())
            assert len([1 for _, r, _ in mine if r.what in ("short", "cut-a")]) >= (2 if L > 2 and len(V.cuts_of(name, i)) > 1 else 1)


def test_the_other_routes_haystacks():
    for name in V.VERIFY_SETS:
        c = V.case(name)
        h = V.hot_hay(name)
        piece, pitch = V.hot_piece(name)
        assert V.TILE // pitch > 64  # more hits to a tile than slots
        g = V.GROUP
        assert len(h) == 2 * g and bytes(h[g + 8 * V.TILE:g + 8 * V.TILE + len(piece)]) == piece
        miss = np.array([p.x for p in c.plants if p.k >= 0])
        assert (miss < 8 * V.TILE - 300).sum() >= 5 and (miss < g - 300).sum() >= 20  # in the hot group; in the one in front
        assert np.array_equal(h[:g], c.hay[:g]) and np.array_equal(h[g:g + 8 * V.TILE], c.hay[:8 * V.TILE])
        ks = V.k0_pieces(name)
        assert V.K0_PIECE == 16384 and V.K0_PF == 40000 and max(len(k) for k in ks) == 40000
        assert sum(len(k) for k in ks) == 2 * V.HAY_LEN and sum(len(k) for k in ks if len(k) <= 16384) >= V.HAY_LEN


@pytest.mark.parametrize("row", V.packed_rows(), ids=lambda r: r.name)
def test_packed_rows(row):
    table = {"pw64x14337": (6, True), "pw65x8191": (7, True), "pw65x8192": (7, False), "pw128x8191": (7, True),
             "pw16384x63": (14, True), "pw16384x64": (14, False), "pw16385x31": (15, True), "pw16385x32": (15, False)}
    rb, narrow = table[row.name]
    assert V.rank_bits_of(row.n) == rb and V.narrow_expected(row.n, row.max_len) == narrow
    assert not V.narrow_expected(row.n, row.max_len, codepoints=True)
    lb = V.bits_for(row.max_len)
    assert (rb + lb == C["W32_FIELD"]) if narrow else (rb + lb == C["W32_FIELD"] + 1)  # both sides of the boundary
    assert 64 - C["REL_BITS"] - rb - C["CP_BITS"] >= lb  # (the wide form holds it, the carried count above it)
    pats, named = V.packed_patterns(row.name), V.packed_named(row.name)
    assert len(pats) == row.n and max(len(p) for p in pats) == row.max_len == len(pats[named["longest"]])
    assert sum(len(p) == row.max_len for p in pats) == 1 and set(b"".join(pats)) <= set(range(97, 123))
    long_p = pats[named["longest"]]
    assert long_p.startswith(pats[1]) and long_p.endswith(pats[2]) and pats[1].startswith(pats[4]) and len(pats[4]) < len(pats[1]) < row.max_len
    if row.n & (row.n - 1) == 0 and (row.max_len + 1) & row.max_len == 0:  # tie + length: a field with all bits set
        assert named["longest"] == row.n - 1 and ((row.n - 1) << lb | row.max_len) == (1 << (rb + lb)) - 1
    assert row.name != "pw128x8191" or (rb + lb == C["W32_FIELD"] and named["longest"] == 127)
    # the highest tie value: the last id (LeftmostFirst), the last rank (the kinds that rank)
    from ahocorasick_rs_amd import capi
    for mk in (0, 2):
        h = capi.HostAutomaton(list(pats), mk)
        top = int(np.argmax(h.rank))
        h.close()
        assert top in named.values(), (row.name, mk, top, named)
    c = V.packed_case(row.name)
    for who in set(named.values()):
        L = len(pats[who])
        mine = {w: x for x, i, w in c.plants if i == who}
        assert mine["start first"] % V.TILE == 0 and mine["start last"] % V.TILE == V.TILE - 1
        assert (mine["end first"] + L) % V.TILE == 0 and (mine["end last"] + L) % V.TILE == V.TILE - 1
        assert mine["tile"] // V.TILE != (mine["tile"] + L - 1) // V.TILE
    x = next(x for x, i, w in c.plants if w == "group")
    assert x < V.GROUP < x + row.max_len
    assert sum(w == "spread" for _, _, w in c.plants) == 30 and len(c.hay) == 2 * V.GROUP
    # every plant is an occurrence, and nothing else is: the filler matches nothing
    occ = V.packed_oracle(row.name, 0).find_raw(c.hay, overlapping=True)
    got = {tuple(r) for r in occ.tolist()}
    assert all((i, x, x + len(pats[i])) in got for x, i, _ in c.plants)
    assert np.array_equal(occ, V.brute(pats, c.hay)) if row.n <= 128 else len(occ) >= len(c.plants)
    results = {V.packed_oracle(row.name, mk).find_raw(c.hay).tobytes() for mk in (0, 1, 2)}
    assert len(results) == 3  # a length or a tie that loses a bit changes a result
    for col in (1, 2):
        assert np.unique(occ[:, col] // V.TILE, return_counts=True)[1].max() <= 16
    hot = V.packed_hot_hay(row.name)
    assert len(hot) == len(c.hay) and (hot != c.hay).sum() >= 4 * 2048


@pytest.mark.parametrize("row", V.packed_rows(), ids=lambda r: r.name)
def test_packed_rows_on_the_dense_tile_path(row):
    """the plants of the tile-ordered dense leg lie where k_dense_main can certify a sync point for every group: inside one
    dense group, or starting in the last 2 KiB in front of one"""
    assert V.DGROUP == C["DT_GROUP"] * V.TILE == 16384 and V.GROUP % V.DGROUP == 0
    for L in (4, 12, 31, 32, 63, 64, 8191, 8192, V.longest_sparse()):
        slack = ((L - 1 + 2048 + V.TILE - 1) // V.TILE) * V.TILE - (L - 1)  # tile_lookback(L) tiles less the longest reach
        assert slack >= V.DENSE_SLACK
    pats, named = V.packed_patterns(row.name), V.packed_named(row.name)
    c = V.packed_dense_case(row.name)
    occ = {tuple(r) for r in V.packed_oracle(row.name, 0).find_raw(c.hay, overlapping=True).tolist()}
    for who in set(named.values()):
        L = len(pats[who])
        mine = {w: x for x, i, w in c.plants if i == who}
        want = {"start first", "start last", "end last", "tile", "group"} | ({"end first"} if L + 1 <= V.DGROUP - V.TILE else set())
        assert set(mine) == want and ("end first" in mine or (L == V.longest_sparse() and row.name == "pw64x14337"))
        for w, x in mine.items():
            assert (who, x, x + L) in occ
            o = x % V.DGROUP
            assert o + L < V.DGROUP or o >= V.DGROUP - V.DENSE_SLACK, (row.name, who, w, o)
        assert mine["start first"] % V.TILE == 0 and mine["start last"] % V.TILE == V.TILE - 1
        assert (mine["end last"] + L) % V.TILE == V.TILE - 1 and ("end first" not in mine or (mine["end first"] + L) % V.TILE == 0)
        assert mine["tile"] // V.TILE != (mine["tile"] + L - 1) // V.TILE
        assert mine["group"] // V.DGROUP != (mine["group"] + L - 1) // V.DGROUP
    x = next(x for x, i, w in c.plants if w == "group" and i == named["longest"])
    assert x < V.GROUP < x + row.max_len
    assert len({V.packed_oracle(row.name, mk).find_raw(c.hay).tobytes() for mk in (0, 1, 2)}) == 3
