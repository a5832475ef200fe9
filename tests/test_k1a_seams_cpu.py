"""CPU: the plan of tests/k1a_seams.py holds what it claims -- no GPU.  The oracle is pinned against brute(), brute_iter() and
brute_leftmost() on every case below 1 MiB; every class's geometry is recomputed from the oracle's rows, the pointer residue
and the host tables (a plant moved by one byte at a limit fails here); form_of() is held against every set and every case;
the failureless cases are enumerated by the Python twin of test_host_cpu.py (imported, not copied), whose trace counts the
survivors, items and stage-G hits (k1a_seams.scan_trace()); no class is empty; the CU-dependent shapes are built at 2 and 256
CUs; class (g)'s plants are the oracle's rows at 2 CUs.  The file's 32 tests take 18 .. 21 s."""
import numpy as np
import pytest

import k1a_seams as K
from k1b_seams import brute, brute_iter
from post_seams import brute_leftmost

capi = pytest.importorskip("ahocorasick_rs_amd.capi")
CUS = (2, 256)


def all_cases(cus=256):
    return K.plan(cus) + K.plan(cus, True)


def ov_rows(c):
    return K.expected(c, 0, True)


def test_constants_and_restated_lines():
    assert K.TILE == 4096 and K.C["K1A_T3B_WORDS"] == len(K.host("fl31").walk_t3b)
    assert K.warm16(17) == 16 and K.warm16(18) == 32 and K.warm16(33) == 32 and K.warm16(34) == 48
    # the chunk moves from its floor to warm * 8 between max_len 33 and 34; the walk length is an odd multiple of 16 at 17
    assert [K.walk16_chunk(m, 10000, 256) for m in (17, 18, 33, 34)] == [K.C["W16_MIN"]] * 3 + [48 * K.C["W16_WARMX"]]
    assert (K.warm16(17) + K.walk16_chunk(17, 10000, 256)) // 16 % 2 == 1
    assert K.pick_chunk(12) == K.C["CH_MIN"] and K.pick_chunk(34) == (33 * K.C["CH_WARMX"] + 63) & ~63


def test_the_grid_stride_loop_of_walk16_takes_a_second_turn_beyond_cus_mib():
    """the grid-stride loop of k1a_walk16 by the restated arithmetic.  Up to cus MiB (the chunk at its floor of 256 bytes:
    cus * 1024 lanes of four chains) it takes ONE turn.  Beyond, walk16_chunk() rounds total / (cus * 4096) DOWN before it
    rounds up to 16: wherever that quotient is a multiple of 16 and the division leaves a remainder, the chunks of one turn
    do not hold the stream and lane 0 takes a second turn for the rest -- first at cus MiB + 1 byte (256 MiB + 1 on 256
    CUs), NOT only from 2^40 bytes on.  k1a_seams.second_turn_case() is that shape."""
    for cus in CUS:
        for total in [1, 4096, 1 << 20, (cus << 20) - 1, cus << 20]:
            for ml in (1, 12, 34, 4000):
                assert K.walk16_turns(total, ml, cus) == 1
        assert K.walk16_turns((cus << 20) + 1, 12, cus) == 2 and K.walk16_turns((cus << 20) + 1, 34, cus) == 1
        assert K.walk16_turns((cus << 20) + 16 * cus * 4096, 12, cus) == 1  # (the quotient is 272: the chunks hold it again)
        c = K.second_turn_case(cus)
        total = len(c.hay)
        chunk = K.walk16_chunk(K.max_len(c.set), total, cus)
        assert K.walk16_turns(total, K.max_len(c.set), cus) == 2 and chunk * K.CHAINS * 1024 * cus < total
        tail = c.hay[chunk * K.CHAINS * 1024 * cus - 64:]
        rows = brute(K.patterns(c.set), tail)   # the plants around the second turn's first byte, and in it
        assert (rows[:, 2] == 64).any() and (rows[:, 1] == 64).any() and (rows[:, 2] == 64 + chunk + 1).any() and (rows[:, 2] == len(tail)).any()


@pytest.mark.parametrize("name", K.SETS)
def test_form_of_every_set(name):
    h = K.host(name)
    for mk in (1, 2):  # the kinds share the trie: the same form under every kind
        g = K.host(name, mk)
        assert (g.n_states, g.n_classes, g.dense, len(g.walk_t3b) > 0) == (h.n_states, h.n_classes, h.dense, len(h.walk_t3b) > 0)
    want = {"w16over": ("chunked", "chunked"), "chnfa": ("chunked_nfa", "chunked_nfa")}.get(
        name, ("failureless", "failureless") if name.startswith("fl") and name != "fl32" else ("walk16", "chunked"))
    assert (K.form_of(h, False), K.form_of(h, True)) == want
    assert K.form_of(h, False, chunked_again=True) != "failureless" and K.form_of(h, True, no_pfac=True) in ("chunked", "chunked_nfa")


def test_the_sets_straddle_their_limits():
    assert K.host("fl31").n_classes == 32 and K.host("fl32").n_classes == 33
    assert K.host("w16max").n_states == 0xFFFF and K.host("w16over").n_states == 0x10000
    h = K.host("w16")
    assert h.n_classes > 32 and K.rows16(h.n_states, h.n_classes) < h.n_states <= 0xFFFF
    assert K.host("ch3fff").n_states > K.C["HOT_MAX"] and K.host("ch3fff").dense and not K.host("chnfa").dense
    g = K.host("fltail").walk_grec
    tails = {(int(r[1]) >> 24) & 15 for r in g if int(r[1]) & 0x40000000}
    assert tails == set(range(9)), tails  # GREC_TAIL records of 0 .. 8 bytes, none of 9
    s = K.host("flshort")
    assert (s.walk_t3r[:, 1] >> 31).any() and (s.walk_t3b == 0xFFFFFFFF).any() and not (K.host("fl31").walk_t3r[:, 1] >> 31).any()
    assert 0xFFFFFFFE in K.host("flmany").walk_grec[:, 2]  # OWN1_MANY
    # flalias: a near miss passes level 1 (one symbol) and dies at the class triple
    a = K.host("flalias")
    tr = K.scan_trace("flalias", b"---AAb!x---aAb!x---")
    assert tr["survivors"][3] and not tr["items"][3] and not tr["hits"][3] and (tr["items"][11] or tr["hits"][11]) and a.n_classes <= 32


def test_every_case_has_the_form_it_is_meant_for():
    for nopfac in (False, True):
        for c in K.plan(256, nopfac):
            assert c.form == K.form_of(K.host(c.set), bool(c.cuts), no_pfac=nopfac), (c.set, c.cls, c.name)
            if c.cuts:
                assert c.cuts[0] == 0 and c.cuts[-1] == len(c.hay) and list(c.cuts) == sorted(c.cuts)
                assert not c.uniform or all(b - a == c.uniform for a, b in zip(c.cuts, c.cuts[1:]))


def test_no_class_is_empty_and_the_shapes_build_at_2_and_256_cus():
    for cus in CUS:
        # (the GPU file parametrises over the two constants: collecting it builds no plan)
        assert tuple(K.legs(cus)) == K.LEGS and tuple(K.legs(cus, True)) == K.NOPFAC_LEGS
        assert {cl for cl, _ in K.LEGS} | {"g"} == set(K.CLASSES) and K.G_SHAPES == tuple(K.turn_tiles(cus))
        for s in K.NOPFAC_SETS:  # every failureless set, every class of the child, the workgroup border of walk16 among them
            mine = {(c.cls, c.name.split("_")[0]) for c in K.plan(cus, True) if c.set == s}
            assert {("a", "len"), ("b", "lanes"), ("b", "waves"), ("b", "groups"), ("b", "chunks"), ("d", "ragged"), ("d", "uniform")} <= mine, s
        for c in K.plan(cus) + K.plan(cus, True):
            lim = 10 ** 6
            assert sum(len(r) for r in ov_rows(c)) <= lim and c.residues, c.name
            for kind, *v in c.claim:
                if kind == "chunk" and c.form == "walk16":
                    assert v[0] == K.walk16_chunk(K.max_len(c.set), c.residues[0] + len(c.hay), cus)
    assert any(("odd_walk", 1) in c.claim for c in K.plan(256)) and any(("odd_walk", 0) in c.claim for c in K.plan(256))


def test_no_bucket_of_a_sparse_call_holds_more_than_the_post_stage_stages():
    """a call the plan expects on the sparse path: at most STAGE_SLOTS occurrences a bucket of the post stage (4 KiB of the
    index space), counted by start (the leftmost kinds) and by end (Standard), at every residue of the case; one it expects
    to leave for its hits: more than STAGE_SLOTS_W32 in one bucket under either key"""
    for c in all_cases():
        if c.leaves:
            if c.cls == "e":
                rows = ov_rows(c)[0].astype(np.int64)
                assert min(np.bincount(rows[:, col] >> K.C["TILE_BITS"]).max() for col in (1, 2)) > K.BUCKET_W32, c.name
            continue
        base = np.repeat(np.asarray(c.cuts[:-1] if c.cuts else (0,), np.int64), [len(r) for r in ov_rows(c)])
        rows = np.concatenate(ov_rows(c)).astype(np.int64)
        for lead in c.residues:
            for col in (1, 2):
                if len(rows):
                    assert np.bincount((rows[:, col] + base + lead) >> K.C["TILE_BITS"]).max() <= K.BUCKET, (c.set, c.cls, c.name)


def test_the_oracle_against_the_brute_searches():
    seen = set()
    for c in all_cases():
        if len(c.hay) >= 1 << 20 or (c.set, c.hay, c.cuts) in seen:
            continue
        seen.add((c.set, c.hay, c.cuts))
        pats = K.patterns(c.set)
        for k, row in enumerate(K.rows_of(c)):
            if not row:
                continue
            b = brute(pats, row)
            assert np.array_equal(K.expected(c, 0, True)[k], b), (c.set, c.name, k)
            assert np.array_equal(K.expected(c, 0, False)[k], brute_iter(pats, row)), (c.set, c.name, k)
            assert np.array_equal(K.expected(c, 1, False)[k], brute_leftmost(pats, row, False)), (c.set, c.name, k)
            assert np.array_equal(K.expected(c, 2, False)[k], brute_leftmost(pats, row, True)), (c.set, c.name, k)


def test_the_twin_of_the_failureless_form_enumerates_every_case():
    from test_host_cpu import failureless_walk_occurrences
    n = 0
    for c in K.plan(256):
        if c.form != "failureless" or c.cuts or len(c.hay) > 20000:
            continue
        got = sorted(failureless_walk_occurrences(K.host(c.set), c.hay))
        assert got == sorted(tuple(int(v) for v in r) for r in ov_rows(c)[0]), (c.set, c.name)
        # ... and scan_trace(): every occurrence starts at a position that stage G settles or hands to the walk
        tr = K.scan_trace(c.set, c.hay)
        starts = np.unique(ov_rows(c)[0][:, 1].astype(np.int64))
        assert (tr["items"][starts] | tr["hits"][starts]).all() and not (tr["items"] & tr["hits"]).any(), (c.set, c.name)
        n += 1
    assert n > 150


def test_class_a_ends_of_the_stream():
    forced = 0
    for c in all_cases():
        if c.cls != "a":
            continue
        rows, n = ov_rows(c)[0], len(c.hay)
        assert c.residues == K.RES4
        for kind, *v in c.claim:
            if kind == "ends_at":
                assert len(rows) and rows[:, 2].max() == v[0] == n, (c.set, c.name)
            elif kind == "starts_at":
                assert ((rows[:, 1] == v[0]) & (rows[:, 2] == len(K.longest(c.set)))).any()
            elif kind == "n":
                assert len(rows) == v[0]
            elif kind == "cut":  # one byte more (a NUL pattern: its NULs) would complete it: it is not reported
                p = v[0]
                if len(p) == 1:
                    continue
                k = next(k for k in range(len(p) - 1, 0, -1) if c.hay.endswith(p[:k]))
                assert k >= len(p.rstrip(b"\0")) - (0 if p.endswith(b"\0") else 1) and not ((rows[:, 1] == n - k) & (rows[:, 0] == K.patterns(c.set).index(p))).any(), (c.set, c.name)
        if c.form == "failureless":  # the last three positions: forced through level 1, kept up to last_start, walked from the root
            tr, mn = K.scan_trace(c.set, c.hay), K.min_len(c.set)
            for p in range(max(0, n - 3), n):
                keep = n >= mn and p <= n - mn
                assert tr["survivors"][p] == keep and tr["items"][p] == keep and not tr["hits"][p], (c.set, c.name, p)
                forced += keep
            if n < mn:
                assert not tr["survivors"].any()  # any_start
    assert forced > 50  # (flshort: min_len 1, all three positions; the sets without short patterns: none behind last_start)


def test_class_b_chunk_seams():
    n16 = nch = 0
    ends16 = {}
    for c in all_cases():
        if c.cls != "b":
            continue
        rows = np.concatenate(ov_rows(c))
        lead = c.residues[0] if c.form == "walk16" else 0
        chunk = dict((k[0], k[1]) for k in c.claim if k[0] == "chunk")["chunk"]
        ml = K.max_len(c.set)
        for kind, *v in c.claim:
            if kind == "ends_at_index":  # a chunk's last byte is index c * chunk - 1: an end at c * chunk; its first: c * chunk + 1
                assert v[0] % chunk in (0, 1) and (rows[:, 2] + lead == v[0]).any(), (c.set, c.name, v)
                n16 += 1
                ends16.setdefault((c.set, c.name.split("_")[0]), set()).add((v[0] // chunk, v[0] % chunk))
            elif kind == "ends_at":
                assert v[0] % chunk in (0, 1) and (rows[:, 2] == v[0]).any(), (c.set, c.name, v)
                nch += 1
            elif kind == "starts_at":    # the warm-up's first byte, and the byte in front of it
                assert (v[0] + ml - 1) % chunk in (0, chunk - 1) and ((rows[:, 1] == v[0]) & (rows[:, 2] == v[0] + ml)).any(), (c.set, c.name, v)
                nch += 1
        if c.form == "walk16":
            assert len(c.residues) == 1
            total = lead + len(c.hay)
            chunks = (total + chunk - 1) // chunk
            assert total % chunk and chunks % K.CHAINS, "the last group straddles total"
            if c.name.startswith("lanes") and ml % 16 == 1:  # the longest pattern's start is the warm-up's first byte
                assert any((rows[:, 1] + lead == k * chunk - K.warm16(ml)).any() for k in range(1, 9))
            if c.name.startswith("waves"):
                assert (rows[:, 2] + lead == 256 * chunk).any() or (rows[:, 2] + lead == 256 * chunk + 1).any()
            if c.name.startswith("groups"):
                assert (rows[:, 2] + lead == 4096 * chunk).any() or (rows[:, 2] + lead == 4096 * chunk + 1).any()
        else:
            assert c.residues == tuple(range(16))
    assert n16 > 100 and nch > 40
    for (name, label), got in ends16.items():  # both sides of the borders chain | chain, lane | lane, wave | wave, workgroup | workgroup
        for border in (1, 4) + ((256,) if label == "waves" else ()) + ((4096,) if label == "groups" else ()):
            assert {(border, 0), (border, 1)} <= got, (name, label, border)


def test_class_c_table_seams():
    seen = set()
    for c in K.plan(256):
        if c.cls != "c":
            continue
        h = K.host(c.set)
        es = K.visited(c.set, c.hay)
        ids = [0] + [e & K.ID_MASK for e in es]
        of, bfs, plain = K.walk_order(c.set) if c.form == "walk16" else (None, None, None)
        hr = K.hot_rows(h.n_states, h.stride)
        for kind, *v in c.claim:
            seen.add(kind)
            if kind == "walk_state":
                assert int(bfs[v[0]]) in ids, (c.set, v)
            elif kind == "rows16":
                assert v[0] == K.rows16(h.n_states, h.n_classes)
                w = [int(of[i]) for i in ids]  # from LDS to table16 and back
                assert v[0] == h.n_states or any(a < v[0] <= b for a, b in zip(w, w[1:])) and any(b < v[0] <= a for a, b in zip(w, w[1:]))
            elif kind == "bfs_state":
                assert v[0] in ids
            elif kind == "hot_rows":
                assert v[0] == hr < h.n_states
            elif kind == "hot_ffff":  # a hot row's entry whose target cannot be stored: 0xFFFF, read from HBM
                assert any(s < hr and (e & K.ID_MASK) >= K.C["HOT_MAX"] for s, e in zip(ids, es))
            elif kind == "hot_flag":
                assert any(s < hr and (e & K.ID_MASK) < K.C["HOT_MAX"] and (e >> v[0]) & 1 for s, e in zip(ids, es))
        if c.form == "walk16":  # the first reporting state is walked into, and it alone reports there
            rows = ov_rows(c)[0]
            p = K.pattern_through(c.set, int(bfs[plain]))
            x = c.hay.index(p)
            assert ((rows[:, 1] >= x) & (rows[:, 2] <= x + len(p))).sum() == 1
    assert seen >= {"walk_state", "rows16", "bfs_state", "hot_rows", "hot_ffff", "hot_flag"}


def test_class_d_haystack_borders():
    kinds = set()
    for c in all_cases():
        if c.cls != "d":
            continue
        cuts, rows = set(c.cuts), ov_rows(c)
        ml = K.max_len(c.set)
        assert c.host_too and len(c.residues) == 2
        at = {}
        for k in c.cuts:  # empty haystacks at one border: the offsets that repeat it
            at[k] = at.get(k, -1) + 1
        sizes = {b - a for a, b in zip(c.cuts, c.cuts[1:])}

        def straddled(p):  # p stands in the stream with a border inside it: no haystack reports it there
            x = c.hay.find(p)
            while x >= 0:
                if any(x < k < x + len(p) for k in cuts):
                    return True
                x = c.hay.find(p, x + 1)
            return False

        def flush(p):      # p ends exactly at a border, inside ONE haystack
            return any(k >= len(p) and c.hay[k - len(p):k] == p and not any(k - len(p) < j < k for j in cuts) for k in cuts)
        for kind, *v in c.claim:
            kinds.add(kind)
            if kind == "border_in_warmup":
                assert any(v[0] - (ml - 1) < k < v[0] for k in cuts)
            elif kind == "border_at":
                assert v[0] in cuts
            elif kind == "empty_run":  # exactly that many empty haystacks side by side, haystacks with bytes on both sides
                assert any(r == v[0] and 0 < k < len(c.hay) for k, r in at.items()), (c.set, c.name, v)
            elif kind == "empty_run_at_chunk_border":
                assert any(r == v[0] and k and k % K.pick_chunk(ml) == 0 for k, r in at.items()), (c.set, c.name, v)
            elif kind == "cut":
                assert straddled(v[0]) and flush(v[0])
            elif kind in ("room4", "tail_flush"):
                assert flush(v[0]) and straddled(v[0]) and (len(v[0]) == 4) == (kind == "room4")
            elif kind == "d_over_room":  # its first three bytes end a haystack: the scan's depth 4 reaches beyond it
                assert flush(v[0]) and any(c.hay[k - 3:k + len(v[0]) - 3] == v[0] for k in cuts if k >= 3)
            elif kind == "short_at_row_end":
                assert flush(v[0]) and len(v[0]) <= 3
            elif kind == "rows":
                assert len(c.cuts) - 1 == v[0] and c.uniform
        if c.name == "ragged":
            assert {1, 2, 3, 4, 5} <= sizes or c.form == "failureless"
        total = sum(len(r) for r in rows)
        assert total >= 3 or c.uniform < K.min_len(c.set), (c.set, c.name)
    assert kinds >= {"border_in_warmup", "border_at", "empty_run", "empty_run_at_chunk_border", "cut", "room4", "tail_flush", "d_over_room", "short_at_row_end", "rows"}


def test_class_e_stage_g_and_the_walk():
    paths = set()
    for c in K.plan(256):
        if c.cls != "e":
            continue
        rows = ov_rows(c)[0]
        tr = K.scan_trace(c.set, c.hay)
        if c.name == "near_misses":
            pats = K.patterns(c.set)
            exact = [p for p in K.TAILS + (K.OWN4_LONG, K.OWN4)]
            for p in exact:
                x = c.hay.index(p)
                assert ((rows[:, 1] == x) & (rows[:, 0] == pats.index(p))).any()
                for q in K.near_misses(p):  # planted, a survivor of level 1 up to depth 4, and not reported
                    y = c.hay.index(q)
                    assert tr["survivors"][y] and not ((rows[:, 1] == y) & (rows[:, 2] == y + len(p))).any()
            assert sum(len(K.near_misses(p)) for p in exact) == sum(K.TAIL_REST) + 2
        elif c.name == "copies":
            pats = K.patterns(c.set)
            for p in (b"manyx", b"duplicate", b"four"):
                x = c.hay.index(p)
                ids = sorted(int(r[0]) for r in rows if r[1] == x and r[2] == x + len(p))
                assert ids == [i for i, q in enumerate(pats) if q == p] and len(ids) == 3
        else:
            (_, tile, ng, nw), = c.claim
            lo, hi = tile * K.TILE, (tile + 1) * K.TILE
            in_tile = (rows[:, 1] >= lo) & (rows[:, 1] < hi)
            assert tr["hits"][lo:hi].sum() == ng and in_tile.sum() == ng + nw and c.fresh
            assert tr["items"][lo:hi].sum() >= nw and c.leaves
            assert c.name.startswith("tile-1") == (len(c.hay) % K.TILE != 0 and hi > len(c.hay))
            paths.add((ng, nw))
    assert paths == {(63, 0), (64, 0), (65, 0), (60, 3), (60, 4), (60, 5)}


def test_class_f_region_capacity():
    for cus in CUS:
        cases = [c for c in K.plan(cus) if c.cls == "f"]
        assert len(cases) == 7
        left = set()
        for c in cases:
            n = len(c.hay)
            assert n <= K.TILE and K.pfac_scan_grid(0, n, cus) == 1  # ONE tile: one wave, one region
            (_, items), (_, cs, cd) = c.claim
            assert (cs, cd) == (K.pfac_region_cap(n, 1, False), K.pfac_region_cap(n, 1, True))
            tr = K.scan_trace(c.set, c.hay)
            assert tr["items"].sum() == items and tr["hits"].sum() == 0 and c.fresh and c.leaves == (items > cs)
            assert K.scan_trace(c.set, c.hay, slots=False)["items"].sum() == items
            assert len(ov_rows(c)[0]) == 1  # the stretch of 'a' holds no occurrence: the one at the end is the answer
            left.add((items - cs, items - cd))
        assert {d for d, _ in left} >= {-1, 0, 1} and {d for _, d in left} >= {-1, 0, 1} and any(c.claim[0][1] > 256 for c in cases)


def test_class_g_wave_turns():
    """the plants of turn_case() ARE the oracle's rows under every kind on the same layout at 2 CUs (all four shapes), and
    at 256 CUs for the three small shapes; the counts shape stores one full batch of 16 counts in every wave, with an epilogue
    of one count behind it in W / 2 + 1 of them; stage G's hits and k1a_walk's items both occur in every shape"""
    from k1b_seams import count_batches
    o = {mk: K.oracle(K.G_SET, mk) for mk in (0, 1, 2)}
    for cus, shapes in ((2, K.G_SHAPES), (256, K.G_SHAPES[:1])):
        for name in shapes:
            tiles = K.turn_tiles(cus)[name]
            hay, want = K.turn_case(tiles)
            assert len(hay) == (tiles - 1) * K.TILE + 1234 and K.pfac_scan_grid(0, len(hay), cus) == min(cus, (tiles + 15) // 16)
            for mk, ov in K.KINDS:
                assert np.array_equal(o[mk].find_raw(hay, overlapping=ov).astype(np.uint64), want), (cus, name, mk, ov)
            primer, pwant = K.turn_case(tiles, K.PRIMER_SHIFT)  # the haystack every handle sees first: other positions, a plant in every tile
            assert len(primer) == len(hay) and np.array_equal(pwant[:, 1:], want[:, 1:] + K.PRIMER_SHIFT)
            assert len(np.unique(pwant[:, 1].astype(np.int64) >> 12)) == tiles and not set(pwant[:, 1].tolist()) & set(want[:, 1].tolist())
            for mk, ov in K.KINDS[:2] if name == "counts" else K.KINDS:
                assert np.array_equal(o[mk].find_raw(primer, overlapping=ov).astype(np.uint64), pwant), (cus, name, mk, ov)
            starts = want[:, 1].astype(np.int64)
            assert len(np.unique(starts >> K.C["TILE_BITS"])) == tiles  # a plant starts in every tile
            ends = want[:, 2].astype(np.int64)
            crossing = (starts >> K.C["TILE_BITS"]) != ((ends - 1) >> K.C["TILE_BITS"])
            assert crossing.sum() == (tiles - 1) // 16 and (ends[crossing] // K.TILE % 16 == 0).all()
            lens = ends - starts
            assert (lens <= 12).any() and (lens >= 13).any()
            if cus == 2 and name != "counts":  # stage G settles the short ones, the long ones leave as items
                tr = K.scan_trace(K.G_SET, hay.tobytes())
                assert tr["hits"][starts[lens <= 12]].all() and tr["items"][starts[lens >= 13]].all()
    for cus in CUS:
        t = K.turn_tiles(cus)
        assert (t["w-1"], t["w"], t["w+1"]) == (16 * cus - 1, 16 * cus, 16 * cus + 1)
        b = count_batches(t["counts"], cus)
        assert b["full"] == 16 * cus and b["epilogue_behind_batch"] == 8 * cus + 1 and b["remainders"] == [0, 1]
        assert count_batches(t["w+1"], cus)["max"] == 2 and count_batches(t["w"], cus)["max"] == 1
