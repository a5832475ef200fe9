"""The plan of tests/cp_seams.py, checked without a GPU.  Two duties: the reference is pinned -- code_points() against
Python's own decoder at every character boundary of every planned haystack, the mapped oracle rows against the oracle's
own str search --, and the plan is shown to reach every seam it is there for, with the oracle's matches (LeftmostLongest,
cfg5's kind) and not with the plants it asked for: a class without a reported match fails HERE, nothing is skipped on the
device."""
import numpy as np
import pytest

import cp_seams as S

PLAN = S.plan()
C, Z = S.source_constants(), S.sizes()


def starts_of(c):
    return set(S.byte_rows(c.name, *S.LL)[:, 1].tolist())


def reported(c):
    """the plants the oracle reports a match AT (LeftmostLongest)"""
    st = starts_of(c)
    return [p for p in c.plants if p.x in st]


def boundaries_by_decoder(hay: np.ndarray) -> np.ndarray:
    """the byte offset of every character boundary, from the decoded string (not from the lead-byte rule)"""
    u = np.frombuffer(hay.tobytes().decode("utf-8").encode("utf-32-le"), dtype=np.uint32)
    width = 1 + (u >= 0x80).astype(np.int64) + (u >= 0x800) + (u >= 0x10000)
    return np.concatenate([[0], np.cumsum(width)])


def test_constants_are_what_the_plan_assumes():
    assert C["CP_UNKNOWN"] == (1 << C["CP_BITS"]) - 1 and C["CP_UNKNOWN"] > S.CHUNK  # (a carried count of 16 fits)
    assert C["BP_BLOCKS"] % C["BP_THREADS"] == 0 and Z.wg == C["BP_BLOCKS"] * S.BLOCK
    assert Z.tile % S.BLOCK == 0 and Z.dgroup < Z.group < Z.wg and Z.wg % Z.group == 0
    assert Z.big == 2 * C["BP_BLOCKS"] * 1024 + 5 * 1024 + 321 and max(len(c.hay) for c in PLAN) == Z.big
    assert Z.big <= (2 << 20) + (8 << 10)
    for inst in S.boundaries().values():  # (no instance of a smaller boundary is one of a larger one: the layouts stay apart)
        assert all(b + 64 < Z.big for b in inst)
    assert all(b % Z.group for b in S.boundaries()["tile"] + S.boundaries()["dgroup"])
    assert all(b % Z.dgroup for b in S.boundaries()["tile"]) and all(b % Z.wg for b in S.boundaries()["group"])


def test_patterns_are_what_the_issue_asks_for():
    P = S.PATTERNS
    assert 36 <= len(P) <= 48 and all(3 <= len(p) <= 12 for p in P)
    assert set("".join(P)) <= set("abcdefgh") | {"é", "☃", "🤦"}
    assert len(S.ASCII_IDS) >= 5 and len(S.FOUR_FIRST) >= 4 and len(S.FOUR_LAST) >= 4
    assert len(P) - len(set(P)) == 1  # one pair of copies
    assert len(S.LONG_TAIL) == 2 and S.PLEN[S.SPAN36] > 32
    assert all(len(P[i]) != S.PLEN[i] for i in S.LONG_TAIL + [S.SPAN36])  # (pchars is not the byte length)
    # nested: the three kinds (and the overlapping search) give four different results on the same haystack
    rows = [S.byte_rows("mixed-big", mk, ov).tobytes() for mk, ov in S.KINDS]
    assert len(set(rows)) == 4


def test_no_filler_holds_what_a_pattern_is_filed_under():
    k = S.KEY_BYTES
    assert k >= 5
    for w, unit in S.UNITS.items():
        f = unit * 8
        for p in S.PATS_B:
            assert not any(p[i:i + k] in f for i in range(len(p) - k + 1)), (w, p.decode())
    assert not set(b"abcdefgh") & set(b"".join(S.UNITS.values()) + bytes([S.PAD]))


def test_the_reference_is_the_decoders_count_at_every_character_boundary():
    for c in PLAN:
        cp = S.code_points(c.hay)
        b = boundaries_by_decoder(c.hay)  # (raises where a haystack is not valid UTF-8)
        assert b[-1] == len(c.hay) and np.array_equal(cp[b], np.arange(len(b), dtype=np.uint64)), c.name
        assert cp.dtype == np.uint64 and len(cp) == len(c.hay) + 1
        for x in (c.plants[0].x, c.plants[-1].x, len(c.hay)):  # (and literally, at a few of them)
            assert len(c.hay[:x].tobytes().decode("utf-8")) == cp[x], (c.name, x)
    # fillers of one width: the widths the plan is about
    for w, width in (("w1", 1), ("w2", 2), ("w3", 3), ("w4", 4)):
        h = S.case(f"{w}-big").hay
        assert abs(len(h) / float(S.code_points(h)[-1]) - width) < 0.2, w  # (but for the two stretches of another width)


def test_mapped_oracle_rows_are_the_oracles_str_search():
    for c in PLAN:
        text = c.hay.tobytes().decode("utf-8")
        for mk, ov in (S.KINDS if c.name.endswith("-big") else [S.LL]):
            want = S.oracle(mk).find_str(text, overlapping=ov)
            got = S.expected(c.name, mk, ov)
            assert len(got) == len(want) > 0 and [tuple(int(v) for v in r) for r in got] == want, (c.name, mk, ov)


def test_every_plant_is_a_match_where_it_was_put():
    for c in PLAN:
        rep = reported(c)
        assert len(rep) == len(c.plants) >= 100, (c.name, len(rep), len(c.plants))
        # sparse: no 4 KiB tile near k_tile_main's 24 staged occurrences (every occurrence counts, by its start or its end)
        occ = S.byte_rows(c.name, 0, True)
        for col in (1, 2):
            assert np.unique(occ[:, col] // Z.tile, return_counts=True)[1].max() <= 20, c.name


@pytest.mark.parametrize("w", S.WIDTHS)
def test_residues_and_carried_counts(w):
    ascii_r, ascii_c, four_r, four_c = set(), set(), set(), set()
    for c in (c for c in PLAN if c.width == w):
        for p in reported(c):
            if p.tag[0] == "res1":
                chunk = c.hay[p.x & ~15:(p.x | 15) + 1]
                assert p.x % 16 == p.tag[1] and (chunk < 0x80).all() and S.PATTERNS[p.pid].isascii()
                ascii_r.add(p.x % 16)
                ascii_c.add(S.carried_at(c.hay, p.x))
            if p.tag[0] == "res4":
                assert p.x % 16 == p.tag[1]
                # a stretch of 4-byte characters on both sides
                assert bytes(c.hay[p.x - 16:p.x - 8]).count(S.UNITS["w4"]) >= 1 and bytes(c.hay[p.x + 40:p.x + 56]).count(S.UNITS["w4"]) >= 3
                four_r.add(p.x % 16)
                four_c.add(S.carried_at(c.hay, p.x))
    assert ascii_r == set(range(16)) and ascii_c == set(range(1, 17)), (ascii_r, ascii_c)
    assert four_r == set(range(16)) and four_c >= {1, 2, 3, 4}, (four_r, four_c)
    assert max(four_c) < C["CP_UNKNOWN"]


@pytest.mark.parametrize("w", S.WIDTHS)
def test_blocks_boundaries_and_lengths(w):
    cases = [c for c in PLAN if c.width == w]
    offs, first_blocks = set(), set()
    before, after, across = {}, {}, {}
    two_rounds = inside_four = at_wg = 0
    for c in cases:
        rows = S.byte_rows(c.name, *S.LL)
        st = set(rows[:, 1].tolist())
        for p in reported(c):
            if p.tag[0] == "blk":
                offs.add(p.x % S.BLOCK)
            if p.x // S.BLOCK in (C["BP_BLOCKS"], 2 * C["BP_BLOCKS"]):
                first_blocks.add((p.x // S.BLOCK, (p.x % S.BLOCK) // S.CHUNK))
        for kind, inst in S.boundaries().items():
            for B in inst:
                if B + 64 > len(c.hay):
                    continue
                before[kind] = before.get(kind, 0) + sum(1 for x in range(B - 17, B) if x in st)
                after[kind] = after.get(kind, 0) + sum(1 for x in range(B, B + 18) if x in st)
                sp = rows[(rows[:, 1] < B) & (rows[:, 2] > B)]
                across[kind] = across.get(kind, 0) + len(sp)
                for _, s, e in sp.tolist():
                    two_rounds += e - (s & ~7) > 32  # lead_bytes_between(): 32 bytes a round, from the aligned word of s
                    inside_four += c.hay[s] >= 0xF0 and s + 4 > B
                at_wg += kind in ("wg1", "wg2") and B in st
    assert offs == set(S.BLOCK_OFFSETS) == {0, 1, 15, 16, 1007, 1008, 1023}, offs
    for kind in ("tile", "dgroup", "group", "wg1", "wg2"):
        assert before[kind] >= 2 and after[kind] >= 2 and across[kind] >= 1, (kind, before, after, across)
    assert two_rounds >= 3 and inside_four >= 3 and at_wg >= 2
    # starts in the first block of the second and of the third prefix workgroup: its first chunk, a middle one, the last
    for blk in (C["BP_BLOCKS"], 2 * C["BP_BLOCKS"]):
        assert {ch for b, ch in first_blocks if b == blk} >= {0, 1, 32, 62}, first_blocks
    # the lengths: the prefix's entries and the sentinel among them, the residues, a match in the last 16 bytes
    want = S.sentinel_lengths()
    assert {e for e, _ in want} == {C["BP_BLOCKS"] - 1, C["BP_BLOCKS"], C["BP_BLOCKS"] + 1, 2 * C["BP_BLOCKS"] + 1}
    assert {n % 16 for _, n in want} == {0, 1, 15} and {n % 1024 for _, n in want} >= {0, 1}
    for entries, n in want:
        c = S.case(f"{w}-len{n}")
        assert len(c.hay) == n and (n + S.BLOCK - 1) // S.BLOCK + 1 == entries
        last = S.byte_rows(c.name, *S.LL)[-1]
        assert last[2] == n and last[1] >= n - 16, (c.name, last)
    for c in cases:  # (every case ends with one)
        last = S.byte_rows(c.name, *S.LL)[-1]
        assert last[2] == len(c.hay) and last[1] >= len(c.hay) - 16, (c.name, last)
    # every pattern is reported, both copies by the overlapping search
    seen = set()
    for c in cases:
        seen |= set(S.byte_rows(c.name, 0, True)[:, 0].tolist())
    assert seen == set(range(len(S.PATTERNS)))


def test_batches():
    h, offs = S.ragged_batch()
    assert offs[0] == offs[1] == 0 < offs[2] and offs[-3] < offs[-1] == offs[-2] == len(h)  # empty in front and at the end
    lens = np.diff(offs)
    assert (lens >= 0).all() and any(lens[i] == 0 and lens[i + 1] == 0 for i in range(1, len(lens) - 2))  # two in a row inside
    assert {o % 16 for o in offs} == set(range(16))
    assert {o % 1024 for o in offs} >= {0, 1, 1023, 1007}
    with_match = 0
    for a, b in zip(offs[:-1], offs[1:]):
        h[a:b].tobytes().decode("utf-8")  # every boundary is a character boundary
        with_match += len(S.oracle(2).find_raw(np.ascontiguousarray(h[a:b]))) > 0
    assert with_match == sum(1 for n in lens if n >= 40) >= 20 and S.code_points(h)[-1] < len(h)
    (u4, l4), (u1k, l1k) = S.uniform_batches()
    assert l4 % 4 == 0 and l4 % 16 and l1k == 1024
    for u, ul in ((u4, l4), (u1k, l1k)):
        assert len(u) % ul == 0 and len(u) // ul >= 32
        hit = rows = 0
        for k in range(len(u) // ul):
            piece = u[k * ul:(k + 1) * ul]
            piece.tobytes().decode("utf-8")
            n = len(S.oracle(2).find_raw(np.ascontiguousarray(piece)))
            hit, rows = hit + (n > 0), rows + n
        assert hit >= 8 and rows >= 16 and len(u) / float(S.code_points(u)[-1]) > 3.5  # (4-byte filler)


def test_byte_ranges_cut_inside_characters():
    names = set()
    for name, h, piece in S.range_cases():
        h.tobytes().decode("utf-8")
        cuts = list(range(piece, len(h), piece))
        assert len(cuts) + 1 >= 3 and piece > 2 * (max(S.PLEN) - 1) + 16, name
        width = 3 if "w3" in name else 4
        assert piece % width == int(name.split()[2]), name
        for c in cuts:
            assert (h[c] & 0xC0) == 0x80, (name, c)  # inside a character ...
            k = c
            while (h[k] & 0xC0) == 0x80:
                k -= 1
            assert h[k] >= (0xF0 if width == 4 else 0xE0), (name, c)  # ... of the filler's width
        assert len(S.oracle(2).find_raw(np.ascontiguousarray(h))) >= 100
        names.add(name)
    assert names == {"w4 piece 1 mod 4", "w4 piece 2 mod 4", "w4 piece 3 mod 4", "w3 piece 1 mod 3"}


def test_k0_cuts_hold_matches_at_their_ends():
    assert S.K0_CUTS == (1008, 1024, 1025, 16384)
    for w in S.WIDTHS:
        for n in S.K0_CUTS:
            h = S.head(S.case(f"{w}-big").hay, n)
            h.tobytes().decode("utf-8")
            rows = S.oracle(2).find_raw(h)
            assert len(h) == n and len(rows) >= 4, (w, n)
            if n != 1025:
                assert rows[-1][2] == n, (w, n, rows[-1])  # flush with the end
            assert S.code_points(h)[-1] <= n
