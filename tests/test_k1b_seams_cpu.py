"""The plan of tests/k1b_seams.py, checked without a GPU.  The plan is a fixed list (one digest on two builds of it); the
reference is pinned twice -- the oracle's rows against brute() / brute_iter(), bytes.find in a loop, on every case below
1 MiB and for both semantics --; and no class is empty: for every class the plan names, the ORACLE reports a match with the
start and the end the class is named for (the geometry is recomputed here from the reported row and the pointer residue,
not taken from the plan's bookkeeping), every "one byte short" and NUL-tail plant is reported nowhere, each of the kernel's
four tile bounds takes both of its values, every sweep holds exactly k matches of P in its tile.  Nothing is skipped on the
device: the cap on cases left out is 0."""
import collections

import numpy as np
import pytest

import k1b_seams as K

capi = pytest.importorskip("ahocorasick_rs_amd.capi")
C, TILE, ROW = K.C, K.TILE, K.ROW
MAX_ROWS, MAX_CALLS, LEFT_OUT = 10 ** 6, 3000, 0


def reported(set_name, c):
    return set(map(tuple, K.expected(set_name, c.hay, 0, True).tolist()))


def hits_of(set_name, cls=None, prefix=None):
    """(case, mark, index, length) of every plant of a class that the oracle reports where it was planted"""
    out = []
    for c in K.position_cases(set_name):
        marks = [m for m in c.marks if m.hit and (m.cls == cls if cls else m.cls.startswith(prefix))]
        if not marks:
            continue
        rep = reported(set_name, c)
        for m in marks:
            L = len(K.patterns(set_name)[m.pid])
            if (m.pid, m.start, m.start + L) in rep:
                out.append((c, m, c.lead + m.start, L))
    return out


def test_the_constants_and_the_forms():
    assert TILE == 4096 and ROW == 1024 and C["K1B_STAGE_BYTES"] == ROW + 16 and C["STAGE_ROW"] == ROW
    assert K.HB < K.Q1CAP == 64 == K.HIT_SLOTS and K.HB_BIG < K.HB and C["OVF_LISTS"] >= 1
    assert [(f.q, f.bigv, f.sh) for f in K.FORMS] == [(q, b, s) for q, b in ((3, 0), (4, 0), (5, 0), (5, 1), (5, 2)) for s in (False, True)]
    assert len(K.FORMS) == 10 and len(K.SINKS) == 4 and len({f.name for f in K.FORMS}) == 10
    assert len({(f.name, s) for f in K.FORMS for s in K.SINKS}) == 40
    # ACX_FILTER_BIG is only read for Q = 5, and the forced forms run the sets of the Q = 5 forms
    assert all(f.q == 5 and f.set == K.FORM["q5sh" if f.sh else "q5"].set for f in K.FORMS if f.bigv)
    assert set(K.SWEEP_K) == set(range(K.HIT_SLOTS - 4, K.HIT_SLOTS + 5)) and len(K.SWEEP_TILES) == 4


def test_the_plan_is_deterministic():
    first = K.digest()
    for f in (K.patterns, K.position_cases, K.oracle):
        f.cache_clear()
    assert K.digest() == first


@pytest.mark.parametrize("form", K.FORMS, ids=lambda f: f.name)
def test_each_form_has_the_tables_its_row_claims(form):
    h = capi.HostAutomaton(list(K.patterns(form.set)))
    assert h.t.filter_q == form.q and h.t.long_min_len == form.q == K.min_len(form.set)
    assert (h.t.n_short == len(K.SHORTS)) if form.sh else (h.t.n_short == 0)
    assert h.t.filter_density < 0.2  # left alone the set takes BIGV = 0: 1 and 2 are forced
    h.close()


@pytest.mark.parametrize("set_name", K.SET_NAMES)
def test_the_oracle_is_brute_force(set_name):
    pats = K.patterns(set_name)
    assert K.CLEAN not in set(b"".join(pats))
    cases = list(K.position_cases(set_name))
    cases += [K.sweep_case(set_name, w, k, pair) for w in K.SWEEP_TILES for k in K.SWEEP_K
              for pair in ((False, True) if set_name.endswith("sh") else (False,))]
    for c in cases:
        assert len(c.hay) < 1 << 20 and len(c.front) < 16
        assert np.array_equal(K.expected(set_name, c.hay, 0, True), K.brute(pats, c.hay)), c.name
        assert np.array_equal(K.expected(set_name, c.hay, 0, False), K.brute_iter(pats, c.hay)), c.name
        assert len(K.expected(set_name, c.hay, 0, True)) <= MAX_ROWS
    # the two-batch burst shape (16 CUs + 2 tiles; below 1 MiB at 2 CUs)
    hay = K.turn_hay(set_name, K.turn_tiles(2)["w+2"], 2, bursts=True)
    assert len(hay) < 1 << 20
    assert np.array_equal(K.expected(set_name, hay, 0, True), K.brute(pats, hay))
    assert np.array_equal(K.expected(set_name, hay, 0, False), K.brute_iter(pats, hay))


def test_the_oracle_is_brute_force_on_the_region_cases():
    pats = K.region_set()
    o = K.Oracle(list(pats), 0, K.KIND_DFA)
    for name, hay, hits in K.region_cases(K.CPU_CUS):
        rows = o.find_raw(hay, overlapping=True)
        assert np.array_equal(rows, K.brute(pats, hay)) and np.array_equal(o.find_raw(hay), K.brute_iter(pats, hay))
        assert len(rows) == hits and K.n_tiles(0, len(hay)) == 1, name  # every match a prefix hit of the one wave
    cap = K.hit_region_records(TILE, 1, K.CPU_CUS)
    assert cap == 4096 and [h for _, _, h in K.region_cases(K.CPU_CUS)][:3] == [cap - 1, cap, cap + 1]
    assert K.region_cases(K.CPU_CUS)[3][2] > cap + cap // 2  # the whole tile: nearly two hits a byte


@pytest.mark.parametrize("set_name", K.SET_NAMES)
def test_no_position_class_is_empty(set_name):
    geometry = {
        "lane15": lambda c, i, L: i % 16 == 15,
        "lane0": lambda c, i, L: i % 16 == 0,
        "rowflush": lambda c, i, L: (i + L) % ROW == 0 and L >= 8,
        "rowend": lambda c, i, L: i % ROW == ROW - 3,
        "rowcross": lambda c, i, L: i % ROW >= ROW - 16 and (i + L - 1) // ROW == i // ROW + 1 and i // TILE == (i + L - 1) // TILE,
        "lane63": lambda c, i, L: i % ROW == ROW - 16,
        "tilecross": lambda c, i, L: (i + L - 1) // TILE == i // TILE + 1,
        "wgcross": lambda c, i, L: (i + L - 1) // TILE == i // TILE + 1 and ((i + L - 1) // TILE) % K.WAVES == 0,
        "groupcross": lambda c, i, L: c.lead == 0 and i < K.GROUP < i + L,
        "last_start": lambda c, i, L: L == K.min_len(set_name) and i + L == c.lead + len(c.hay),
        "ends_in_last16": lambda c, i, L: 0 < c.lead + len(c.hay) - (i + L) < 16,
    }
    for cls, ok in geometry.items():
        got = hits_of(set_name, cls)
        assert got and all(ok(c, i, L) for c, _, i, L in got), cls
    # the seams around tiles of other waves and, 16 and 17, of the second workgroup; at every residue
    seams = collections.defaultdict(set)
    for c, m, i, L in hits_of(set_name, "lane15") + hits_of(set_name, "tilecross") + hits_of(set_name, "wgcross"):
        if c.name.startswith("seams_t"):
            seams[int(c.name.split("_")[1][1:])].add(c.lead)
    assert set(seams) == {0, 1, 2, 15, 16, 17} and all(v == {0, 1, 15} for v in seams.values())
    assert K.scan_grid(K.n_tiles(0, 19 * TILE + 21), K.CPU_CUS) == 2
    # the end of the stream: every length the set holds flush with the last byte, and one byte short of it
    lens = K.flush_lengths(set_name)
    assert lens == ([1, 2] if set_name.endswith("sh") else []) + list(range(K.min_len(set_name), 18))
    for Lw in lens:
        got = hits_of(set_name, "flush%d" % Lw)
        assert got and all(L == Lw and m.start + L == len(c.hay) for c, m, i, L in got), Lw
    assert any(L <= 8 for *_, L in hits_of(set_name, prefix="flush")) and any(8 < L <= 16 for *_, L in hits_of(set_name, prefix="flush"))
    misses, cuts_mid = 0, []
    for c in K.position_cases(set_name):
        rep = K.expected(set_name, c.hay, 0, True)
        for m in c.marks:
            if m.hit:
                continue
            p = K.patterns(set_name)[m.pid]
            if m.cls == "cutprefix":  # mid-stream: CUT_KEPT bytes of a pattern that would end in the next tile, then other bytes
                i, kept = c.lead + m.start, K.CUT_KEPT
                cuts_mid.append(c)
                assert c.hay[m.start:m.start + kept] == p[:kept] and c.hay[m.start:m.start + len(p)] != p and len(p) == K.MAX_FLUSH > kept
                assert (i + kept) % TILE == TILE - 2 and (i + len(p) - 1) // TILE == i // TILE + 1
                assert c.hay[m.start + kept] != K.CLEAN  # the border plant lies directly behind it
                assert not ((rep[:, 0] == m.pid) & (rep[:, 1] == m.start)).any(), (c.name, m)
                continue
            misses += 1
            cut = len(c.hay) - m.start
            assert 0 < cut < len(p) and c.hay[m.start:] == p[:cut] and (m.cls.startswith("short") or p[cut:] == b"\0" * (len(p) - cut))
            assert not ((rep[:, 0] == m.pid) & (rep[:, 1] == m.start)).any(), (c.name, m)
    assert misses == len([L for L in lens if L > 1]) + 2 * len(K.NUL_STEMS) + 3
    # the cut prefix: in front of a border of every seam tile, at every residue, on both fillers, and of the group's border
    assert {c.name for c in cuts_mid} >= {f"seams_t{t}_r{r}_clean" for t in (0, 1, 2, 15, 16, 17) for r in (0, 1, 15)} | \
        {"seams_t0_r0_az", "seams_t16_r15_az", "seams_group"}
    # ... and the NUL cut begins behind the last start (only the boundary mask answers for it), pad bytes behind it in its block
    cuts = [(c, m) for c in K.position_cases(set_name) for m in c.marks if m.cls == "nulcut"]
    mlen = K.min_len(set_name)
    assert len(cuts) == 3 and all(m.start == len(c.hay) - (mlen - 1) > len(c.hay) - mlen for c, m in cuts)
    assert {(-len(c.hay)) % 16 >= 2 for c, m in cuts} == {True} and len(K.nul_cut(mlen)) == mlen + 1
    # STAGED: a survivor at bytes ROW - 8 .. ROW - 1 of each of a tile's four rows, and of the stream's last row
    assert K.BEHIND == 8
    for k in range(1, K.BEHIND + 1):
        got = hits_of(set_name, "stage%d" % k)
        assert {(i // ROW) % 4 for c, m, i, L in got if i % ROW == ROW - k} == {0, 1, 2, 3}, k
        assert all(i % ROW + 8 >= ROW for c, m, i, L in got)
    last = hits_of(set_name, prefix="stage_last")
    assert {ROW - i % ROW for c, m, i, L in last} == {k for k in range(1, K.BEHIND + 1) if any(L <= k for L in lens)}
    assert all(i // ROW == (len(c.hay) - 1) // ROW and len(c.hay) % ROW == 0 for c, m, i, L in last)
    # more survivors than Q1 holds: in one row; in a tile's four rows together and in none of them alone
    row = collections.Counter(i // ROW for c, m, i, L in hits_of(set_name, "q1row"))
    assert len(row) == 1 and max(row.values()) > K.Q1CAP
    tile = hits_of(set_name, "q1tile")
    assert len({i // TILE for *_, i, L in tile}) == 1 and len(tile) > K.Q1CAP
    assert max(collections.Counter(i // ROW for *_, i, L in tile).values()) <= K.Q1CAP
    # bursts: n hits in n lanes of one tile
    for n in (K.HB - 1, K.HB, K.HB + 1, 64):
        got = hits_of(set_name, "burst%d" % n)
        assert len(got) == n == len({(i % ROW) // 16 for *_, i, L in got}) and len({i // TILE for *_, i, L in got}) == 1
        c = got[0][0]
        assert len(reported(set_name, c)) == n  # nothing else in the haystack: one batch, one push


@pytest.mark.parametrize("set_name", K.SET_NAMES)
def test_every_tile_bound_takes_both_values(set_name):
    m = K.min_len(set_name)
    seen = collections.defaultdict(set)
    want_d = {0, 1, 15, 16, 17, m - 1, m, m + 1, TILE - 1}
    totals = collections.defaultdict(set)
    for c in K.position_cases(set_name):
        if not c.name.startswith("total_"):
            continue
        b = K.tile_bounds(c.lead, len(c.hay), m)
        total = c.lead + len(c.hay)
        totals[total // TILE].add((total % TILE, c.lead))
        seen["t_int_lo"].add(b["t_int_lo"])
        for name in ("t_int_hi", "t_full", "t_inside"):
            seen[name].add(b[name] - b["last"])
    assert set(totals) == {1, 2, 16} and all(v == {(d, r) for d in want_d for r in (0, 1, 8, 15)} for v in totals.values())
    assert seen["t_int_lo"] == {0, 1}
    for name in ("t_int_hi", "t_inside"):
        assert seen[name] == {0, -1}, (name, seen[name])  # the last tile's index, and the one before
    # t_full has ONE value: total16 - 16 and total - 1 lie in the same 16-byte block, so it IS the last tile's index at
    # every total -- every tile but the last takes the scalar-base loads, the last one the clamped ones
    assert seen["t_full"] == {0}


@pytest.mark.parametrize("set_name", K.SET_NAMES)
def test_every_sweep_holds_k_matches_in_its_tile(set_name):
    pats = K.patterns(set_name)
    for where in K.SWEEP_TILES:
        for pair in ((False, True) if set_name.endswith("sh") else (False,)):
            tiles = set()
            for k in K.SWEEP_K:
                c = K.sweep_case(set_name, where, k, pair)
                rows = K.expected(set_name, c.hay, 0, True)
                P = c.marks[0].pid
                t = (rows[:, 1] + c.lead) // TILE
                assert len(set(t.tolist())) == 1 and len(rows) == k  # one tile; a match per prefix hit, k in all
                if pair:
                    ab, a = K.pid_of(set_name, b"ab"), K.pid_of(set_name, b"a")
                    assert (rows[:, 0] == P).sum() == k - 2 * K.PAIR_FIXED and (rows[:, 0] == ab).sum() == (rows[:, 0] == a).sum() == K.PAIR_FIXED
                    assert b"a" not in pats[P]
                else:
                    assert (rows[:, 0] == P).all()
                tiles.add(int(t[0]))
                assert c.lead == (15 if where == "first_lead15" else 0)
                cut = K.nul_cut(K.min_len(set_name))
                assert (where == "last_partial") == c.hay.endswith(cut[:-2]) and cut in pats
            last = K.n_tiles(c.lead, len(c.hay)) - 1
            assert tiles == {{"first_lead15": 0, "interior": 2, "last_partial": last, "group_last": C["GROUP_TILES"] - 1}[where]}
            assert where != "last_partial" or (c.lead + len(c.hay)) % TILE
            assert where != "group_last" or last == C["GROUP_TILES"]


def test_the_staircase_check_itself():
    assert K.staircase([0, 0, 0, 0, 0, 1, 2, 3, 4], [0] * 5 + [1] * 4) is None
    assert K.staircase([0, 0, 0, 1, 2, 3, 4, 5, 6], [1] * 9)       # a stray hit: the crossing moved
    assert K.staircase([0, 0, 0, 0, 0, 2, 3, 4, 5], [1] * 9)       # never 1
    assert K.staircase([0, 0, 0, 0, 0, 1, 2, 2, 4], [1] * 9)       # a step missed
    assert K.staircase([1, 2, 3, 4, 5, 6, 7, 8, 9], [1] * 9)       # not 0 at the smallest k
    assert K.staircase([0, 0, 0, 0, 0, 1, 2, 3, 4], [0] * 9)       # no hot group


def test_wave_turns_at_256_compute_units():
    t = K.turn_tiles(K.CPU_CUS)
    w = 16 * K.CPU_CUS
    assert (t["w-1"], t["w"], t["w+1"], t["w+2"]) == (w - 1, w, w + 1, w + 2) and t["counts"] == 16 * w + w // 2 + 1
    # below 16 tiles a wave no count leaves in a full batch, and no epilogue stores behind one: the branch is dead
    for name in ("w-1", "w", "w+1", "w+2"):
        b = K.count_batches(t[name], K.CPU_CUS)
        assert b["full"] == 0 and b["epilogue_behind_batch"] == 0 and b["max"] == (1 if name in ("w-1", "w") else 2)
    b = K.count_batches(t["counts"], K.CPU_CUS)
    assert b == {"full": w, "epilogue_behind_batch": w // 2 + 1, "remainders": [0, 1], "max": 17}
    assert K.count_batches(t["counts"] - w // 2 - 1, K.CPU_CUS)["epilogue_behind_batch"] == 0  # 16 tiles a wave: none
    # the two-batch bursts: one wave, consecutive turns, HB and HB + 1 hits together
    cus = 2
    hay = K.turn_hay("s5", K.turn_tiles(cus)["w+2"], cus, bursts=True)
    rows = K.expected("s5", hay, 0, True)
    per = collections.Counter((rows[:, 1] // TILE).tolist())
    w2 = 16 * cus
    assert per[0] + per[w2] == K.HB and per[1] + per[w2 + 1] == K.HB + 1 and min(per[0], per[w2], per[1], per[w2 + 1]) >= 2
    assert np.array_equal(rows, K.brute(K.patterns("s5"), hay))


def test_the_counts_shape_has_a_plant_in_every_tile():
    tiles = K.turn_tiles(K.CPU_CUS)["counts"]
    hay = K.turn_hay("s5", tiles, K.CPU_CUS, multibyte=True)
    assert 264 << 20 <= len(hay) < 265 << 20 and len(hay) % TILE and K.n_tiles(0, len(hay)) == tiles
    rows = K.expected("s5", hay, 0, False)
    assert tiles - 1 <= len(rows) <= MAX_ROWS
    assert len(np.unique(rows[:, 1] // TILE)) >= tiles - 1  # (the last, partial tile may be too short for its plant)
    cross = rows[(rows[:, 1] // TILE) != ((rows[:, 2] - 1) // TILE)]
    assert len(cross) == (len(hay) - 16) // (16 * TILE) and ((cross[:, 2] - 1) // TILE % 16 == 0).all()
    # the offsets walk through the tile: every row of a tile, most lanes
    off = rows[:, 1] % TILE
    assert len(np.unique(off // ROW)) == 4 and len(np.unique(off % ROW // 16)) == 64
    cp = K.code_points_at(hay, rows[:, 1])
    assert (cp < rows[:, 1]).any() and cp[0] == rows[0, 1] - np.count_nonzero((hay[:int(rows[0, 1])] & 0xC0) == 0x80)
    bytes(hay[:1 << 16]).decode("utf-8")


def test_nothing_is_left_out_and_every_leg_is_a_few_thousand_calls():
    assert LEFT_OUT == 0
    for f in K.FORMS:
        for s in K.SINKS:
            assert 400 <= K.leg_calls(f.set, s) <= MAX_CALLS
    assert len(K.SWEEP_K) * 2 <= MAX_CALLS
    assert {L for s in K.SET_NAMES for L in K.flush_lengths(s)} == set(range(1, 18))
