"""GPU: one result spliced from pieces, at the seams -- run_chunked (k_cut_point, k_copy_shifted), run_batch_split
(k_rebase_offsets), expand_copies / expand_copies_host (k_copy_counts, k_expand_copies, k_expand_counts) and k_localize,
element-wise against the oracle: every row's pattern, start and end, the per-haystack counts, path_stats()["byte_ranges"]
against the model's count and the error codes.

The plan (sets, haystacks, the model, what every case claims) is tests/splice_seams.py, checked on the CPU by
tests/test_splice_seams_cpu.py.  A class is ONE test per engine or route: its cases share the handles and the oracle's rows,
and a failure names up to 40 of them.  Engines of a piece: "k0" (the default for pieces this small: k0 == the ranges
searched), "walk" and "prefilter" (a forced kernel turns K0 off in-process: k0 == 0).  A forced one-haystack call of at most
SMALL_MAX_LEN bytes from HOST memory never reaches run_find's forcing (acx_find hands it to K0 first): the small cases run
through find_device, the host routes on haystacks beyond K0's reach.  byte_ranges is what proves that a case was cut at all.

ACX_CHUNK_BYTES and ACX_MAX_OCC are read per call, ACX_EXPAND_COPIES when an automaton is built: set around the call with
with_env.  No call here is the uncut call of an input whose cut call follows on the same handle (a buffer from the pool can
hold the right records of the call before: DESIGN section 8), and the overlapping kind runs first."""
import numpy as np
import pytest

import splice_seams as P
from k1b_seams import KINDS, cols, with_env

pytestmark = pytest.mark.gpu
capi = pytest.importorskip("ahocorasick_rs_amd.capi")
SWITCHES = ("ACX_CHUNK_BYTES", "ACX_MAX_OCC", "ACX_NO_BUCKET", "ACX_NO_DENSE_TILES", "ACX_EXPAND_COPIES", "ACX_KERNEL", "ACX_NO_SMALL")
CUT = P.cut_cases()


@pytest.fixture(autouse=True)
def no_switch(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def told(fails):
    assert not fails, (len(fails), fails[:40])


def too_big(call) -> str:
    """the call must end in ACX_ETOOBIG, "more than 2^32 occurrences"; what is wrong otherwise"""
    try:
        call()
    except ValueError as e:
        if getattr(e, "code", None) != capi.ETOOBIG or "more than 2^32 occurrences" not in str(e):
            return "the wrong error: %s %s" % (getattr(e, "code", None), e)
        return ""
    return "no error"


# ---------------------------------------------------------------------------
# (a) .. (d): one haystack in byte ranges, resident on the device
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("engine", P.ENGINES)
@pytest.mark.parametrize("cls", "abcd")
def test_a_haystack_in_byte_ranges(cls, engine):
    """(a) the cut of a range at every border, (b) the carry, (c) k_cut_point's blocks and its two words, (d) the copy: every
    case at pointer residues 0, 1 and 15, every kind of its own; rows, byte_ranges == the model's, k0 == the engine's"""
    cases = [c for c in CUT if c.cls == cls]
    calls, fails = P.run_cut_cases(cases, engine)
    assert calls == sum(len(c.kinds) for c in cases) * len(P.RESIDUES)
    told(fails)


@pytest.mark.parametrize("engine", P.ENGINES)
def test_copies_in_byte_ranges(engine):
    """(i) a run of 301 ids that ends at lo is the range in front's, one that ends at lo + 1 this range's, whole either way"""
    calls, fails = P.run_cut_cases(P.copy_range_cases(), engine)
    assert calls == 2 * len(P.RESIDUES)
    told(fails)


# ---------------------------------------------------------------------------
# the host routes: find(), the Python classes, the sharded simulation
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("engine", P.ENGINES)
def test_host_memory_in_byte_ranges(engine):
    """(a), (b) from host memory: 65 555 bytes are beyond K0, their five (six) ranges within it"""
    H = P.Handles(engine)
    fails = []
    for c in P.host_haystacks():
        for mk, ov in P.ordered(c.kinds):
            model = P.model_of(c, mk, ov)
            a = H.get(c.set, mk)
            with with_env({"ACX_CHUNK_BYTES": str(c.piece)}):
                a.path_stats(reset=True)
                got = cols(a.find(c.hay, overlapping=ov))
                st = a.path_stats(reset=True)
            why = P.diff(got, P.expected(c.set, c.hay, mk, ov))
            if why is None and (st["byte_ranges"], st["k0"]) != (model.searched, model.searched if engine == "k0" else 0):
                why = "byte_ranges %d, k0 %d against the model's %d ranges" % (st["byte_ranges"], st["k0"], model.searched)
            if why:
                fails.append("%s kind %d overlapping %s: %s" % (c.name, mk, ov, why))
    H.close()
    told(fails)


@pytest.mark.parametrize("cls", "ab")
def test_the_python_classes_in_byte_ranges(cls):
    """BytesAhoCorasick on bytes (byte offsets), AhoCorasick on str (code points; the sets are ASCII: the same numbers)"""
    import ahocorasick_rs_amd as ac
    kinds = {0: ac.MatchKind.Standard, 1: ac.MatchKind.LeftmostFirst, 2: ac.MatchKind.LeftmostLongest}
    fails = []
    for c in [c for c in P.host_haystacks() if c.cls == cls]:
        pats = list(P.patterns(c.set))
        for mk, ov in P.ordered(c.kinds):
            want = [tuple(int(v) for v in r) for r in P.expected(c.set, c.hay, mk, ov)]
            b = ac.BytesAhoCorasick(pats, matchkind=kinds[mk])
            t = ac.AhoCorasick([p.decode() for p in pats], matchkind=kinds[mk])
            with with_env({"ACX_CHUNK_BYTES": str(c.piece)}):
                if b.find_matches_as_indexes(c.hay, overlapping=ov) != want:
                    fails.append("%s kind %d overlapping %s: BytesAhoCorasick" % (c.name, mk, ov))
                if t.find_matches_as_indexes(c.hay.decode(), overlapping=ov) != want:
                    fails.append("%s kind %d overlapping %s: AhoCorasick" % (c.name, mk, ov))
    told(fails)


@pytest.mark.parametrize("route", ["host", "device"])
def test_the_ranks_of_a_sharded_haystack(route):
    """simulate_single_sharded over the real automaton: rank by rank what the model's ranges keep, world 2 .. 5 at lengths
    whose borders are the planted ones, and the occurrence that covers two borders"""
    from ahocorasick_rs_amd import distributed as D
    H = P.Handles("k0")
    fails = []
    for c, world in P.sharded_cases():
        buf = P.on_device(0, c.hay) if route == "device" else None
        hay = D.DeviceHaystack(buf.ptr, len(c.hay)) if buf else c.hay
        for mk, ov in P.ordered(c.kinds):
            model = P.model_of(c, mk, ov)
            sim = D.simulate_single_sharded(H.get(c.set, mk), hay, world, ov)
            why = None if len(sim) == world else "%d ranks" % len(sim)
            for rank in range(world if why is None else 0):
                why = why or P.diff(cols(sim[rank]).reshape(-1, 3), model.ranges[rank].kept)
            why = why or P.diff(np.concatenate([cols(s).reshape(-1, 3) for s in sim]), P.expected(c.set, c.hay, mk, ov))
            if why:
                fails.append("%s world %d kind %d overlapping %s: %s" % (c.name, world, mk, ov, why))
        if buf:
            buf.free()
    H.close()
    told(fails)


# ---------------------------------------------------------------------------
# (e) the floor and forcing
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("engine", P.ENGINES)
def test_the_floor_of_a_piece_and_what_is_cut_at_all(engine):
    H = P.Handles(engine)
    fails = []
    for set_name, hay in P.floor_cases():
        floor = P.floor_of(P.max_len(set_name) - 1)
        buf = P.on_device(0, hay)
        for mk, ov in P.ordered(KINDS):
            a = H.get(set_name, mk)
            want = P.expected(set_name, hay, mk, ov)
            tag = "%s kind %d overlapping %s: " % (set_name, mk, ov)

            def run(piece, n=len(hay)):
                return P.cut_call(a, buf.ptr, n, ov, piece)
            # at the floor: ACX_ETOOBIG, and the handle answers the next call
            why = too_big(lambda: run(floor))
            if why:
                fails.append(tag + "a piece of the floor's %d bytes: %s" % (floor, why))
            got, st = run(floor + 1)
            model = P.model_chunked(P.finder(set_name, hay, mk), len(hay), floor + 1, P.max_len(set_name) - 1, ov)
            why = P.diff(got, want) or (None if st["byte_ranges"] == model.searched else "byte_ranges %d" % st["byte_ranges"])
            if why:
                fails.append(tag + "right after the error, a piece of %d bytes: %s" % (floor + 1, why))
            # a haystack of one byte more than a piece is cut in two, one of exactly a piece is not cut (in this order: the
            # cut call does not follow the uncut one of nearly the same input)
            piece = 2 * floor + 5
            for n, ranges in ((piece + 1, 2), (piece, 0)):
                got, st = run(piece, n)
                why = P.diff(got, P.expected(set_name, hay[:n], mk, ov))
                if why is None and st["byte_ranges"] != ranges:
                    why = "byte_ranges %d, not %d" % (st["byte_ranges"], ranges)
                if why:
                    fails.append(tag + "%d bytes at a piece of %d: %s" % (n, piece, why))
        buf.free()
    H.close()
    told(fails)


# ---------------------------------------------------------------------------
# (f) halving by the real trigger
# ---------------------------------------------------------------------------
WAYS = {"dense_tiles": {"ACX_NO_BUCKET": "1"}, "dense_radix": {"ACX_NO_BUCKET": "1", "ACX_NO_DENSE_TILES": "1"}, "unforced": {}}


@pytest.mark.parametrize("way", list(WAYS))
def test_a_pass_over_its_limit_is_halved_until_the_pieces_fit(way):
    """256 KiB with a pattern every 32 bytes under ACX_MAX_OCC = 3 000: halves, then quarters.  byte_ranges is held to the
    model's LOWER bound (splice_seams.least_ranges() says why it cannot be an equality).  "unforced": the way this input
    goes by itself -- through the hit slots and the hot pipeline, which reads the limit only where it sizes an output for
    more than HOT_INLINE hot groups: two groups are answered in one pass, whatever the limit (splice_seams.HOT_GROUPS_MIN;
    the hot pipeline's own trigger needs 4.25 MiB and stays with test_gpu_chunked.py)"""
    pats, hay = P.dense_input()
    m = max(len(p) for p in pats) - 1
    fails = []
    for mk, ov in ((0, True), (0, False), (2, False)):
        o = P.Oracle(list(pats), mk, P.KIND_DFA)
        find = lambda a, b, v: o.find_raw(hay[a:b], overlapping=v)  # noqa: E731
        least = P.least_ranges(find, len(hay), m, ov, P.F_LIMIT)
        a = capi.Automaton(list(pats), mk, capi.IMPL_DFA)
        with with_env({"ACX_MAX_OCC": str(P.F_LIMIT), **WAYS[way]}):
            a.path_stats(reset=True)
            got = cols(a.find(hay, overlapping=ov))
            st = a.path_stats(reset=True)
        a.close()
        why = P.diff(got, find(0, len(hay), ov).astype(np.uint64))
        dense = st["dense_tiles"] + st["dense_radix"]  # (the tile-ordered form may hand a piece to the radix form, never the reverse)
        took = {"unforced": True, "dense_tiles": dense >= 4 and st["dense_tiles"] >= 1, "dense_radix": st["dense_radix"] >= 4 and st["dense_tiles"] == 0}
        if way == "unforced" and st["dense_tiles"] + st["dense_radix"] == 0:
            least = 0 if len(hay) < P.HOT_GROUPS_MIN * P.GROUP else least
        if why is None and not ((st["byte_ranges"] >= least >= 6 or st["byte_ranges"] == least == 0) and took[way]):
            why = "byte_ranges %d against at least %d: %s" % (st["byte_ranges"], least, st)
        if why:
            fails.append("kind %d overlapping %s: %s" % (mk, ov, why))
    told(fails)


def test_halving_ends_in_k0_or_at_the_floor():
    """32 736 bytes of 1 637 rows under a limit of 1 500: two halves whose windows (max_len - 1 bytes more) are within K0's
    reach, and their rows within its room -- and a forced walk under a
    limit every piece exceeds: halved down to the floor, ACX_ETOOBIG, and the handle answers the next call"""
    fails = []
    n = 2 * (P.SMALL_MAX_LEN - 16)
    hay = P.plant(n, [(k, P.LADDER[7]) for k in range(4, n - 8, 20)])  # (one occurrence a plant under every kind)
    for mk, ov in P.ordered(KINDS):
        want = P.expected("lad", hay, mk, ov)
        a = P.automaton("lad", mk)
        with with_env({"ACX_MAX_OCC": "1500", "ACX_NO_BUCKET": "1"}):
            a.path_stats(reset=True)
            got = cols(a.find(hay, overlapping=ov))
            st = a.path_stats(reset=True)
        a.close()
        least = P.least_ranges(P.finder("lad", hay, mk), len(hay), 7, ov, 1500)
        why = P.diff(got, want)
        if why is None and not (len(want) == 1637 and st["byte_ranges"] == least == 2 and st["k0"] == 2):
            why = "byte_ranges %d (at least %d), k0 %d" % (st["byte_ranges"], least, st["k0"])
        if why:
            fails.append("k0 kind %d overlapping %s: %s" % (mk, ov, why))
    dense = b"x" * 4096
    buf = P.on_device(0, dense)
    for mk, ov in ((0, True), (0, False), (2, False)):
        a = P.automaton("s8", mk, "walk")
        with with_env({"ACX_MAX_OCC": "10", "ACX_NO_BUCKET": "1"}):
            a.path_stats(reset=True)
            why = too_big(lambda: a.find_device(buf.ptr, len(dense), overlapping=ov))
            st = a.path_stats(reset=True)
        if not why and not (st["k0"] == 0 and st["byte_ranges"] >= 7):  # (4 096 -> 2 048 -> .. -> 32: seven levels, then 16 <= 30)
            why = "no error, but %s" % st
        if why:
            fails.append("floor kind %d overlapping %s: %s" % (mk, ov, why))
        r = a.find_device(buf.ptr, len(dense), overlapping=ov)
        why = P.diff(cols(r.matches()), P.expected("s8", dense, mk, ov))
        r.free()
        a.close()
        if why:
            fails.append("floor kind %d overlapping %s, the call after the error: %s" % (mk, ov, why))
    buf.free()
    told(fails)


# ---------------------------------------------------------------------------
# (g) a batch in two parts, (h) k_localize, (i) copies in a batch
# ---------------------------------------------------------------------------
ROUTES = ("find_batch", "d_offsets", "uniform_len")


def run_batches(batches, route: str, kinds, handles: P.Handles, env, least_of=None):
    """every batch the route takes under every kind: rows and counts per haystack, byte_ranges >= least_of(batch, kind)"""
    fails, ran = [], 0
    for b in batches:
        if (route == "uniform_len") != b.uniform and route != "find_batch":
            continue
        blob, off = b"".join(b.hays), P.batch_offsets(b)
        if route == "uniform_len" and not blob:
            continue
        bufs = []
        if route != "find_batch":
            bufs.append(P.on_device(0, blob))
            if route == "d_offsets":
                bufs.append(capi.DeviceBuffer(8 * len(off)).upload(np.array(off, dtype=np.uint64)))
        for mk, ov in P.ordered(kinds):
            a = handles.get(b.set, mk)
            per = P.batch_expected(b, mk, ov)
            with with_env(env):
                a.path_stats(reset=True)
                if route == "find_batch":
                    m, counts = a.find_batch(list(b.hays), overlapping=ov, codepoints=b.codepoints)
                else:
                    r = a.find_device(bufs[0].ptr, len(blob), n_hay=len(b.hays), overlapping=ov, codepoints=b.codepoints,
                                      **({"uniform_len": len(b.hays[0])} if route == "uniform_len" else {"d_offsets": bufs[1].ptr}))
                    m, counts = r.matches(), r.counts()
                    r.free()
                st = a.path_stats(reset=True)
            ran += 1
            why = None if [int(c) for c in counts] == [len(x) for x in per] else "counts %s against %s" % (list(counts), [len(x) for x in per])
            why = why or P.diff(cols(m), np.concatenate([x.reshape(-1, 3) for x in per]).astype(np.uint64))
            least = least_of(b, mk, ov) if least_of else None
            if why is None and least is not None and not (st["byte_ranges"] >= least if least else st["byte_ranges"] == 0):
                why = "byte_ranges %d against at least %d" % (st["byte_ranges"], least)
            if why:
                fails.append("%s kind %d overlapping %s: %s" % (b.name, mk, ov, why))
        for x in bufs:
            x.free()
    return ran, fails


@pytest.mark.parametrize("route", ROUTES)
def test_a_batch_over_the_limit_in_two_parts(route):
    """ACX_MAX_OCC = 2 000 with ACX_NO_BUCKET: n_hay 1, 2, 3, 4, 5 and 9, ragged and uniform, empty haystacks around the
    cut, one heavy haystack that ends alone in a part and goes on in byte ranges (also as code points, from a byte offset that
    is no multiple of 16), all empty.  byte_ranges: at least the model's splits and ranges; 0 where the model never splits"""
    H = P.Handles("k0")
    ran, fails = run_batches(P.batches_g(), route, KINDS, H, {"ACX_MAX_OCC": str(P.G_LIMIT), "ACX_NO_BUCKET": "1"},
                             lambda b, mk, ov: P.batch_tree(b, mk, ov, P.G_LIMIT)[1].ranges)
    H.close()
    assert ran >= 4 * 6
    told(fails)


@pytest.mark.parametrize("route", ROUTES)
def test_local_offsets_and_counts_of_a_batch(route):
    """(h) no limit lowered: matches on a haystack's first and up to its last byte, a pattern split across two haystacks,
    empty haystacks around matching ones, uniform lengths 1, max_len and 13, haystacks that begin behind characters of 2, 3
    and 4 bytes as code points"""
    H = P.Handles("k0")
    ran, fails = run_batches(P.batches_h(), route, KINDS, H, {}, lambda b, mk, ov: 0)
    H.close()
    assert ran >= 4 * 3
    told(fails)


# ---------------------------------------------------------------------------
# (i) copies of a string
# ---------------------------------------------------------------------------
def copy_handles():
    """set -> [(name, automaton, expanded)]: ACX_EXPAND_COPIES forced on and off, and left to n_later * 4 >= n_patterns"""
    out = {}
    for s in ("cp_at", "cp_below", "cp_run"):
        out[s] = []
        for name, env in (("on", {"ACX_EXPAND_COPIES": "1"}), ("off", {"ACX_EXPAND_COPIES": "0"}), ("itself", {})):
            with with_env(env):
                out[s].append((name, P.automaton(s, 0)))
    return out


def test_copies_expanded_or_not_give_the_oracles_rows():
    """forced on, forced off, just below and at n_later * 4 == n_patterns; 0 copies next to many, copies on the first and the
    last record, a run of 300 across a block, n = 1, no string with copies occurs; K0's host expansion against the device's"""
    H = copy_handles()
    fails = []
    for c in P.copy_cases():
        want = P.expected(c.set, c.hay, 0, True)
        buf = P.on_device(0, c.hay)
        big = c.hay + b"-" * P.SMALL_PF_MAX_LEN  # (beyond K0: the pipeline and the device's expansion from host memory too)
        for name, a in H[c.set]:
            a.path_stats(reset=True)
            host = cols(a.find(c.hay, overlapping=True))  # K0 on the host's own memory: expand_copies_host
            k0 = a.path_stats(reset=True)["k0"]
            r = a.find_device(buf.ptr, len(c.hay), overlapping=True)  # K0 launched: expand_copies
            dev = cols(r.matches())
            r.free()
            for what, got in (("host", host), ("device", dev), ("pipeline", cols(a.find(big, overlapping=True)))):
                why = P.diff(got, want)
                if why:
                    fails.append("%s expansion %s, %s: %s" % (c.name, name, what, why))
            if k0 != 1:
                fails.append("%s expansion %s: the host call was not K0's" % (c.name, name))
        buf.free()
    for hs in H.values():
        for _, a in hs:
            a.close()
    told(fails)


@pytest.mark.parametrize("route", ROUTES)
def test_copies_in_a_batch(route):
    """haystacks without an occurrence, and empty ones, between haystacks whose occurrences carry copies"""
    H = copy_handles()
    fails = []
    for k, name in enumerate(("on", "off", "itself")):
        class One:
            def get(self, set_name, mk):
                return H[set_name][k][1]
        fails += ["expansion %s: %s" % (name, f) for f in run_batches(P.copy_batches(), route, P.STD, One(), {})[1]]
    for hs in H.values():
        for _, a in hs:
            a.close()
    told(fails)
