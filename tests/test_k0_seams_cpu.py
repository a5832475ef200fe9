"""CPU: the K0 seam plan (tests/k0_seams.py) against references that share nothing with the oracle -- bytes.find-based
searches for all four kinds -- and every claim of a class recomputed from those rows: the occurrence count n, the match
count per kind and where each match travels, the mode of every call, the parity of the last legal start, the poll's covered
and width along every sequence.  A plant moved by one byte at a limit fails here (DESIGN section 8 lists the moves tried)."""
import numpy as np
import pytest

import k0_seams as P
from k1b_seams import KINDS, brute, brute_iter
from post_seams import brute_leftmost

C = P.C
_brute = {}


def searches(g, k):
    """{kind: rows} of call k from bytes.find alone"""
    c = g.calls[k]
    h = c.hay.lower() if g.ci else c.hay
    key = (g.set, g.ci, h)
    if key not in _brute:
        pats = [p.lower() if g.ci else p for p in P.patterns(g.set)]
        _brute[key] = {(0, True): brute(pats, h), (0, False): brute_iter(pats, h), (1, False): brute_leftmost(pats, h, False),
                       (2, False): brute_leftmost(pats, h, True)}
    return _brute[key]


def occurrences(g, k) -> int:
    """n as K0 counts it: overlapping rows, one per string where the set holds copies"""
    rows = searches(g, k)[(0, True)]
    pats = P.patterns(g.set)
    return len({(pats[int(i)], int(x), int(e)) for i, x, e in rows})


GROUPS = P.plan()
IDS = [f"{g.cls}-{g.set}-{g.name}" for g in GROUPS]


def test_constants_and_lines():
    """relations between the constants that the plan relies on (their values are the sources': a changed one moves the cases)"""
    assert P.INLINE == 16 * 63 and C["K0_MAILBOX_HAY"] == 16  # 63 lanes x 16 bytes beside the word's lane
    assert P.WAVE == 64 and P.TINY == 16 * P.WAVE            # a wavefront; one 16-byte slice a lane
    assert P.TINY < P.STRIDE < P.MAX_LEN < P.PF_MAX_LEN == 1 << 16  # a packed match carries 16-bit offsets
    assert P.LINE0 + 3 == 8 and P.MORE + 2 == 8 and P.IN_LINES == P.LINE0 + (P.LINES - 1) * P.MORE  # 64-byte lines of 8 words
    # where a match travels: the last of a line and the first of the next, the last in a line and the first in out[]
    assert P.line_and_slot(0) == (0, 2) and P.line_and_slot(P.LINE0 - 1) == (0, 6) and P.line_and_slot(P.LINE0) == (1, 1)
    for L in range(1, P.LINES):
        last = P.LINE0 + L * P.MORE - 1
        assert P.line_and_slot(last) == (L, 6) and P.line_and_slot(last + 1) == ((L + 1, 1) if L + 1 < P.LINES else (-1, 0))
    assert P.line_and_slot(P.IN_LINES + 1) == (-1, 1) and P.line_and_slot(P.WAVE) == (-1, P.WAVE - P.IN_LINES)
    for k in range(70):  # kernels.hpp, k0_result_lines()
        mm = min(k, P.IN_LINES)
        lines = 1 if mm <= P.LINE0 else 1 + (mm - P.LINE0 + P.MORE - 1) // P.MORE
        assert lines == 1 + max((P.line_and_slot(i)[0] for i in range(mm)), default=0)
    # every line's last match and the next one, the first two of out[], wave 0's limit and one more
    assert set(P.B_COUNTS) == {0, 1, P.WAVE, P.WAVE + 1, P.IN_LINES + 2} | {P.LINE0 + L * P.MORE + d for L in range(P.LINES) for d in (0, 1)}


def test_a_failure_under_any_kind_reaches_a_test():
    """run_group() tags a failure with the mode of the call UNDER ITS KIND; an overlapping call on the set with copies is MODE 1
    where the non-overlapping call on the same bytes is MODE 2: tests_of() and verdict() count both, so no tag is dropped"""
    for route in P.ROUTES:
        groups = P.route_groups(route)
        pairs = set(P.tests_of(route))
        for g in groups:
            for c in g.calls:
                for mk, ov in KINDS:
                    md = P.call_mode(g, c, route, ov)
                    assert (g.cls, md) in pairs, (route, g.set, g.name, c.name, ov)
                    # a faked record: this one failure, and nothing else anywhere
                    if g.set == "copies" or c is g.calls[0]:
                        records = [{"fails": [[md, "faked"]] if h is g else []} for h in groups]
                        assert P.verdict(records, groups, route, g.cls, md) == (1, ["faked"]), (route, g.set, g.name, c.name, ov)
    g = P.group("e", "copies", "copies")
    assert P.group_modes(g, "resident") == {1, 2} and {c.mode for c in g.calls} == {2}
    assert any(b"abc" in c.hay for c in g.calls)


def test_sets_are_at_their_limits():
    f = lambda s: P.facts(s, 0)
    assert f("dc64").n_patterns == C["K0_DC_PATTERNS"] and f("dc64").max_len == 16 and sorted({len(p) for p in P.patterns("dc64")}) == list(P.DC_LENS)
    n = C["K0_DC_WORK"] // C["K0_DC_PATTERNS"]
    assert [P.m(s, n) for s in ("dc64", "dc65", "dc17")] == [2, 0, 0] and f("dc65").n_patterns == 65 and f("dc17").max_len == 17
    assert P.m("dc64", n + 1) == 0
    assert (P.m("one16", C["K0_DC_WORK"]), P.m("one16", C["K0_DC_WORK"] + 1)) == (2, 1)
    assert (P.m("dc4", 1024), P.m("dc4", 1025), P.m("dc8", 512), P.m("dc8", 513), P.m("dc2", 2048), P.m("dc2", 2049)) == (2, 1, 2, 1, 2, 1)
    # LT: 255 bytes and 256; the largest set of a 32-class row and of a 4-class row, and one pattern more
    assert (f("lt255").max_len, P.m("lt255", 1024), f("lt256").max_len, P.m("lt256", 1024)) == (255, 1, 256, 0)
    assert P.lt_reasons(f("lt256")) == ["max_len"]
    assert P.m("ltmax", 64) == 1 and P.m("ltover", 64) == 0 and P.lt_reasons(f("ltover")) == ["K0_LT_ENTRIES"]
    assert f("ltmax").n_states * f("ltmax").stride == C["K0_LT_ENTRIES"]
    assert P.m("ltids", 64) == 1 and P.m("ltidsover", 64) == 0 and P.lt_reasons(f("ltidsover")) == ["K0_LT_ENTRIES", "K0_LT_IDS states"]
    assert f("ltids").n_states == C["K0_LT_IDS"] and f("ltids").n_states * f("ltids").stride == C["K0_LT_ENTRIES"]
    # (K0_LT_IDS patterns: n_states > n_patterns for distinct strings -- the states' limit comes first; not covered)
    assert f("ltids").n_patterns == C["K0_LT_IDS"] - 1
    # MODE 0 at every length up to 16 KiB, not K0 beyond; the same compressed
    for s in ("m0", "m0c"):
        assert {P.m(s, n) for n in (1, 1024, 1025, P.MAX_LEN)} == {0} and P.m(s, P.MAX_LEN + 1) == -1 and f(s).short_min_len == 1
    assert f("m0").dense and not f("m0c").dense
    # MODE 3 from 1 025 bytes to 64 KiB
    for s in ("m3", "urls3", "long2k", "lt256"):
        assert [P.m(s, n) for n in (1024, 1025, P.MAX_LEN, P.MAX_LEN + 1, P.PF_MAX_LEN, P.PF_MAX_LEN + 1)] == [0, 3, 3, 3, 3, -1], s
        assert P.mode_of(f(s), 1025, False, prefilter=False) == 0 and P.mode_of(f(s), P.MAX_LEN + 1, False, prefilter=False) == -1
    assert min(len(p) for p in P.patterns("m3")) == 3 and f("m3").long_min_len == 3 and f("urls3").max_shift != 0
    assert all(nul in P.patterns("m3") for nul in P.NULS) and [len(p) - len(p.rstrip(b"\0")) for p in P.NULS] == [1, 2, 8]
    assert f("long2k").long_min_len == len(P.LONG_A) == 2000
    # copies: an overlapping call is not MODE 2
    assert f("copies").copies == 2 and (P.mode_of(f("copies"), 64, False), P.mode_of(f("copies"), 64, True)) == (2, 1)
    assert P.facts("copies", 1).copies == 0  # (the leftmost kinds have no view of their own)
    for s in P.SETS:  # no pattern occurs in a filler
        assert not any(P.FILL in p or P.FILL2 in p for p in P.patterns(s)), s


def test_every_class_runs_the_modes_it_claims():
    want = {"a": {0, 1, 2, 3}, "b": {0, 1, 2}, "c": {0, 1, 2, 3}, "d": {-1, 0, 1, 2, 3}, "e": {0, 1, 2}, "f": {0, 1, 2}, "g": {0, 1, 2, 3},
            "i": {0, 1, 3}}
    for cls in P.CLASSES:
        assert {c.mode for g in GROUPS if g.cls == cls for c in g.calls} == want[cls], cls
    assert dict.fromkeys(c for c, _ in P.tests_of("resident")) == dict.fromkeys(P.CLASSES)
    # without the prefilter the large automata walk beyond 1 KiB, and beyond 16 KiB nothing is K0's
    nopf = [(g, c, P.call_mode(g, c, "nopf")) for g in GROUPS for c in g.calls]
    assert not any(md == 3 for _, _, md in nopf)
    assert all(md == -1 for g, c, md in nopf if len(c.hay) > P.MAX_LEN)
    assert sum(1 for g, c, md in nopf if c.mode == 3 and md == 0 and 1024 < len(c.hay) <= P.MAX_LEN and g.set == "m3") > 50


@pytest.mark.parametrize("g", GROUPS, ids=IDS)
def test_modes_oracle_and_claims(g):
    f = P.facts(g.set, 0)
    assert len(g.calls) > 0
    for k, c in enumerate(g.calls):
        assert 0 < len(c.hay) <= P.PF_MAX_LEN + 1
        assert P.mode_of(f, len(c.hay), False) == c.mode, (c.name, c.mode)
        rows = searches(g, k)
        for mk, ov in KINDS:
            assert np.array_equal(P.byte_rows(g, k, mk, ov), rows[(mk, ov)]), (c.name, mk, ov)
        n = occurrences(g, k)
        assert c.dense == (n > P.MAX_OCC or c.mode < 0), (c.name, n)
        ends = {int(e) for e in rows[(0, True)][:, 2]}
        for what, *v in c.claim:
            if what == "n":
                assert n == v[0], (c.name, n, v)
            elif what == "more_than":
                assert v[0] < n <= P.MAX_OCC, (c.name, n)
            elif what in ("ends_at", "last_end"):
                assert v[0] == len(c.hay) and max(ends) == v[0], (c.name, v)
            elif what == "cut":  # the byte that is missing would complete an occurrence of the plant, and it is not there
                whole = brute([v[0]], c.hay + v[0][-1:])
                assert len(c.hay) + 1 in {int(e) for e in whole[:, 2]} and c.hay.endswith(v[0][:-1]), c.name
            elif what == "taken":
                assert [len(rows[kd]) for kd in ((1, False), (2, False))] == [v[0]] * 2, (c.name, v)
            elif what == "leftmost":
                assert [len(rows[kd]) for kd in ((1, False), (2, False))] == [v[0]] * 2, (c.name, v)
            elif what == "leftmost_starts":  # match i begins at v[0] + v[1] * i
                for kd in ((1, False), (2, False)):
                    assert rows[kd][:, 1].astype(int).tolist() == [v[0] + v[1] * i for i in range(len(rows[kd]))], (c.name, kd)
            elif what == "has_starts":
                assert {int(x) for x in rows[(0, True)][:, 1]} >= {v[0] + v[1] * i for i in range(v[2])}, c.name
            else:
                raise AssertionError(what)


def test_a_wave0_limits():
    for g in (g for g in GROUPS if g.cls == "a"):
        by = {c.name: (c, k) for k, c in enumerate(g.calls)}
        for n in (P.TINY, P.TINY + 1):
            for cnt in (P.WAVE - 1, P.WAVE, P.WAVE + 1):
                c, k = by[f"units{cnt}_{n}"]
                cm, km = by[f"units{cnt}_{n}_mirror"]
                s, sm = searches(g, k)[(0, True)][:, 1].astype(int), searches(g, km)[(0, True)][:, 1].astype(int)
                assert len(s) == cnt and s[0] == 0 and s[-1] + len(P.U) == n == len(c.hay)
                assert sorted(n - len(P.U) - sm) == sorted(s) and list(s) != list(sm)  # the same positions from the other end
            if P.info(g.set).chain:
                c, k = by[f"chain{P.WAVE}_{n}"]
                r = searches(g, k)
                assert len(r[(0, True)]) == P.WAVE and [len(r[kd]) for kd in KINDS if not kd[1]] == [P.WAVE // 2] * 3
                assert int(searches(g, by[f"chain{P.WAVE}_{n}_mirror"][1])[(0, True)][-1, 2]) == n
            if P.info(g.set).cover:
                r = searches(g, by[f"cover_{n}"][1])
                assert len(r[(0, True)]) == P.WAVE and len(r[(1, False)]) == len(r[(2, False)]) == 1 and len(r[(0, False)]) > 1


def test_b_counts_lines_and_alternation():
    for g in (g for g in GROUPS if g.cls == "b"):
        names = [c.name for c in g.calls]
        seen = {}
        for fam in ("unit", "fam"):
            for cnt in P.B_COUNTS:
                ka, kb = names.index(f"{fam}{cnt}_A0"), names.index(f"{fam}{cnt}_B0")
                assert (kb, names.index(f"{fam}{cnt}_A1"), names.index(f"{fam}{cnt}_B1")) == (ka + 1, ka + 2, ka + 3)  # A B A B
                ra, rb = searches(g, ka), searches(g, kb)
                for kd in ((1, False), (2, False)):
                    a, b = ra[kd].astype(int), rb[kd].astype(int)
                    assert len(a) == len(b) == cnt, (g.set, fam, cnt, kd)
                    # the two haystacks' matches differ in every position and pattern id
                    assert not set(a[:, 0]) & set(b[:, 0]) and not set(a[:, 1]) & set(b[:, 1]) and not set(a[:, 2]) & set(b[:, 2])
                    # ... and match i of either travels in the same word of the same line
                    assert all(a[i, 1] != b[i, 1] and a[i, 2] != b[i, 2] and a[i, 0] != b[i, 0] for i in range(cnt))
                n, nb = occurrences(g, ka), occurrences(g, kb)
                assert (n == nb == cnt) if fam == "unit" else (n > cnt and nb > cnt) or cnt == 0, (g.set, fam, cnt, n, nb)
                seen.setdefault(fam, []).append((cnt, n))
                assert all(x != y for x, y in zip(g.calls[ka].hay, g.calls[kb].hay))  # every byte differs
        # the family's calls cross wave 0's limit in n while the matches are at the lines
        assert any(n > P.WAVE >= cnt for cnt, n in seen["fam"]) and any(cnt < n <= P.WAVE for cnt, n in seen["fam"])


def test_c_the_dense_cut():
    assert sorted({(g.set, c.mode) for g in GROUPS if g.cls == "c" for c in g.calls}) == [("dc2", 2), ("few", 1), ("m0", 0), ("m0c", 0), ("m3", 3)]
    for g in (g for g in GROUPS if g.cls == "c"):
        assert [occurrences(g, k) for k in range(3)] == [P.MAX_OCC - 1, P.MAX_OCC, P.MAX_OCC + 1]
        assert [c.dense for c in g.calls] == [False, False, True]
        assert all(len(c.hay) == (P.MAX_LEN if g.set == "m3" else len(g.calls[0].hay)) >= 2048 for c in g.calls)


def test_d_lengths_and_the_last_legal_start():
    assert set(P.D_LENS) >= {1, 2, 15, 16, 17, 47, 48, 49, 63, 64, 65, 1007, 1008, 1009, 1023, 1024, 1025, 8191, 8192, 8193, 16383, 16384, 16385,
                             65535, 65536, 65537}
    for g in (g for g in GROUPS if g.cls == "d" and g.name == "lengths"):
        f = P.facts(g.set, 0)
        lens = {len(c.hay) for c in g.calls}
        assert lens >= {n for n in P.D_LENS if P.m(g.set, n) >= 0 or P.m(g.set, n - 1) >= 0} >= {n for n in P.D_LENS if n <= P.MAX_LEN + 1}, g.set
        parity = set()
        for k, c in enumerate(g.calls):
            if c.mode == 3 and c.name.startswith("flush_"):
                last = len(c.hay) - f.long_min_len
                starts = searches(g, k)[(0, True)][:, 1].astype(int)
                if last in starts:
                    parity.add(last & 1)
                assert 0 in starts and max(searches(g, k)[(0, True)][:, 2].astype(int)) == len(c.hay), c.name
        if any(c.mode == 3 for c in g.calls):
            assert lens == set(P.D_LENS), g.set
            if g.set in ("m3", "urls3"):
                assert parity == {0, 1}, (g.set, parity)  # a pattern begins at the last legal start, even and odd
        if g.set == "m3":
            names = [c.name for c in g.calls]
            for n in (P.MAX_LEN, P.PF_MAX_LEN):
                for x in range(P.STRIDE - 2, P.STRIDE + 2):
                    st = searches(g, names.index(f"stride_{n}_{x}"))[(0, True)][:, 1].astype(int)
                    assert x in st, (n, x)
            for n in (1025, P.MAX_LEN, P.PF_MAX_LEN):  # the letters end at the last byte, the NULs would lie behind it
                c = g.calls[names.index(f"nul_stems_{n}")]
                assert c.hay.endswith(P.NULS[0][:-1]) and occurrences(g, names.index(f"nul_stems_{n}")) == 0
                c = g.calls[names.index(f"nul_short_{n}")]
                assert c.hay.endswith(P.NULS[2][:-1]) and occurrences(g, names.index(f"nul_short_{n}")) == 0
    g = P.group("d", "long2k", "min_len")
    assert [len(c.hay) - P.facts("long2k", 0).long_min_len for c in g.calls[:4]] == [-1, 0, 1, 1]


def test_e_windows():
    g = P.group("e", "dc64", "windows")
    seen = set()
    for k, c in enumerate(g.calls):
        if c.name.startswith("len") and "_at" in c.name:
            r = searches(g, k)[(0, True)].astype(int)
            seen.add((int(r[0, 2] - r[0, 1]), int(r[0, 1]) & 7))
        if c.name.startswith("near"):
            assert occurrences(g, k) == 0
            j = int(c.name[4:])
            p = P.patterns("dc64")[5]
            assert c.hay[9:25] == p[:j] + b"Z" + p[j + 1:]
    assert seen == {(L, r) for L in P.DC_LENS for r in range(8)}
    w = P.group("e", "one16", "work")
    assert len(w.calls) == 40 and [len(c.hay) for c in w.calls[:2]] == [C["K0_DC_WORK"], C["K0_DC_WORK"] + 1]
    assert [c.mode for c in w.calls] == [2, 1] * 20
    lo, hi = (searches(w, k)[(0, True)].astype(int) for k in (0, 1))
    assert len(lo) == len(hi) == 3 and not set(lo[:, 1]) & set(hi[:, 1]) and lo[-1, 2] == len(w.calls[0].hay) and hi[-1, 2] == len(w.calls[1].hay)


def test_f_sequences_and_the_poll():
    assert P.F_LENS == (16, 1008, 16, 1009, 48, 49, 1024, 1)
    for name, steps in P.sequences().items():
        lens = [n for n, _, _ in steps]
        tr = P.poll_trace(lens)
        for (cov, width, inline), n in zip(tr, lens):
            assert cov == (min(n, P.INLINE) + 15) // 16 * 16 if n < P.INLINE else cov == P.INLINE
            assert width == min(64, (1 + cov // 16 + 3) // 4 * 4) and width % 4 == 0
        # a call wider than the last one's width is read behind the fence; some are, some are not
        # (descending: every call fits the width the longer call before it left behind)
        assert {i for _, _, i in tr} == ({True} if name == "descending" else {False, True}), name
        assert {cp for _, _, cp in steps} == {False, True}
        assert sorted(set(lens)) == sorted(set(P.F_LENS))
    assert [i for _, _, i in P.poll_trace([16, 1008, 16, 1009, 48, 49, 1024, 1])] == [True, False, True, False, True, False, False, True]
    for g in (g for g in GROUPS if g.cls == "f"):
        for a, b in zip(g.calls, g.calls[1:]):
            n = min(len(a.hay), len(b.hay))
            assert all(x != y for x, y in zip(a.hay[:n], b.hay[:n])), (g.name, a.name)
        if g.name.startswith("full_then_empty"):
            cnt = [occurrences(g, k) for k in range(len(g.calls))]
            assert cnt[0] > P.WAVE and cnt[1] == 0 and cnt[3] == 0 and cnt[2] > P.WAVE, cnt
        if g.ci:
            assert any(c.hay != c.hay.lower() for c in g.calls)


def test_g_code_points():
    for g in (g for g in GROUPS if g.cls == "g"):
        names = [c.name for c in g.calls]
        for k, c in enumerate(g.calls):
            c.hay.decode()  # whole characters only
        for n in (P.TINY, P.TINY + 1, P.MAX_LEN):
            k = names.index(f"mixed_{n}")
            r = searches(g, k)[(0, True)].astype(int)
            assert {int(e) & 15 for e in r[:, 2]} == set(range(16)) and {int(s) & 15 for s in r[:, 1]} == set(range(16)), (g.set, n)
            assert 0 in r[:, 1] and n in r[:, 2] and len(r) <= P.WAVE < occurrences(g, names.index(f"mixed_{n}_many"))
            assert sum(1 for b in g.calls[k].hay if b & 0xC0 == 0x80) > n // 3
        assert sorted({len(c.hay) for c in g.calls}) == [n for n in (1024, 1025, 16384, 16385, 65536) if P.m(g.set, n) >= 0]
    m3 = P.group("g", "m3", "code_points")
    k = [c.name for c in m3.calls].index(f"ascii_{P.PF_MAX_LEN}")
    assert int(searches(m3, k)[(0, True)][-1, 2]) - 1 == 0xFFFF


def test_i_chains():
    for g in (g for g in GROUPS if g.cls == "i"):
        names = [c.name for c in g.calls]
        L = P.facts(g.set, 0).max_len
        for links in (70, 200):
            r = searches(g, names.index(f"links{links}_at0"))
            assert len(r[(0, True)]) == links and len(r[(1, False)]) == (links + 1) // 2
        for n in (P.TINY, P.TINY + 1):
            r = searches(g, names.index(f"touching_{n}"))[(0, True)].astype(int)
            long_row = r[(r[:, 2] - r[:, 1]) == L][0]
            assert long_row[1] + L in r[:, 1]  # an occurrence begins exactly max_len behind the longest one's start
            r = searches(g, names.index(f"over_last_byte_{n}"))[(0, True)].astype(int)
            long_row = r[(r[:, 2] - r[:, 1]) == L][0]
            assert long_row[1] + L - 1 in r[r[:, 0] != long_row[0]][:, 1]  # ... and max_len - 1 behind it: over its last byte
            lm = searches(g, names.index(f"over_last_byte_{n}"))[(1, False)].astype(int)
            assert long_row[1] + L - 1 not in lm[:, 1]
            # two occurrences at one start max_len - 1 in front of X, the longest one the FIRST in either leftmost order: the scan
            # back from X must pass the short one (start + max_len == X's start + 1) to meet the one that covers X's first byte
            k = names.index(f"two_at_one_start_{n}")
            r = searches(g, k)[(0, True)].astype(int)
            at3 = r[r[:, 1] == 3]
            assert sorted((at3[:, 2] - at3[:, 1]).tolist()) == [4, L] and at3[at3[:, 2] - 3 == L][0, 0] < at3[at3[:, 2] - 3 == 4][0, 0]
            assert 3 + L - 1 in r[:, 1] and occurrences(g, k) > P.WAVE
            for kd in ((1, False), (2, False)):
                lm = searches(g, k)[kd].astype(int)
                assert lm[0].tolist()[1:] == [3, 3 + L] and 3 + L - 1 not in lm[:, 1]


def test_the_resident_tests_sets_have_the_modes_their_comments_claim():
    """tests/test_gpu_resident.py sets(): the third set holds b"b" -- short_min_len != 0, no prefilter: MODE 0 at every length;
    the fourth set, without patterns under 3 bytes, is the one that runs MODE 3 beyond 1 KiB"""
    import test_gpu_resident as T
    s = T.sets()
    assert list(s) == ["direct comparison", "table in LDS", "tables in global memory", "prefilter beyond 1 KiB"]
    modes = {name: [P.mode_of(P.facts_of(tuple(p), 0), n, False) for n in (75, 1024, 1025, 5000)] for name, p in s.items()}
    assert modes == {"direct comparison": [2, 1, 1, 1], "table in LDS": [1, 1, 1, 1], "tables in global memory": [0, 0, 0, 0],
                     "prefilter beyond 1 KiB": [0, 0, 3, 3]}, modes
