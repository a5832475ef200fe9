"""The stage between verification and the output -- k_tile_main (order, sync points, match kind), k_tile_write (the groups'
places, the batch's per-haystack runs) -- at its limits: the constants, the pattern sets, the haystacks and the plan that
tests/test_post_seams_cpu.py checks on the CPU and tests/test_gpu_post_seams.py runs on the device.  Needs no GPU (run_case()
and what it calls import the library when called).

Expected rows are the oracle's (tests/oracle_lib.py); k1b_seams.brute() / brute_iter() are the second reference.  Sizes are
read from the kernels' sources (source_constants()): a changed constant moves the cases with it, a renamed one, or a line of
arithmetic the plan restates that no longer stands in the sources, fails on the CPU.

key_mode = overlapping ? 0 : match_kind.  Standard and every overlapping call are keyed on the END of an occurrence (a
bucket is the 4 KiB tile of end + lead), the two leftmost kinds on its START.  Every position class is built per key mode
(km 0: the end, km 1: the start), by INDEX (index = lead + stream position), and runs under the kinds of its key mode.

Three forms of k_tile_main are the plan's first axis: "narrow" (32-bit staged words, STAGE_SLOTS_W32 slots: what these tiny
sets get by themselves), "words64" (the same sets under ACX_MAIN_WIDE: 64-bit words, STAGE_SLOTS slots) and "wide"
(ACX_FORCE_WIDE: STAGE_SLOTS_WIDE slots, 64-bit flag masks, GROUP_MAX_WIDE matches a group).  The two switches are read once
per process: child_main() runs every case of a form in ONE child.

One prefix hit per START of a pattern on the filler '-' (no pattern holds it): patterns that share their first Q2 bytes
("qwert", "qwertyu") share the hit.  Every case keeps every tile at or below HIT_SLOTS hits, so that the path it expects has
one cause; test_post_seams_cpu.py recomputes that.

Every call that asserts a path runs on a FRESH handle: a call that gave up holds its handle on the dense path for eight
calls, a call with hot groups changes what the next one queues.  Class (g) alone keeps a handle, and states its order.

Classes: (a) bucket staircase (also as code points and with an anchored pattern), (b) group staircase, (c) sync points and
chains under lookback 1 and 4, (d) the hits' prefix, (e) the write kernel's chunks and the batch's runs (also as code points),
(f) supergroups, (g) sequences on one handle, the hot pipeline queued ahead at its bound, the workspace small -> large -> small,
a call redone wide, the output's room, (h) k_dense_main as the dense path proper, in its full form and as the hot pipeline's
tail.  Further legs in children of their own: LEGS.  Not planted here (DESIGN section 8 says so too): the anchored and the
code-point leg of the other classes."""
from __future__ import annotations

import functools
import hashlib
import json
import os
import re
import sys
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

from k1b_seams import CLEAN, KINDS, code_points_at, cols, with_env
from oracle_lib import KIND_DFA, Oracle
from verify_seams import body

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ahocorasick_rs_amd", "csrc")


# ---------------------------------------------------------------------------
# the constants of the sources, and what the plan believes of them
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def source_constants() -> Dict[str, int]:
    kern = open(os.path.join(CSRC, "kernels.hip")).read()
    types = open(os.path.join(CSRC, "device_types.hpp")).read()
    attempts = open(os.path.join(CSRC, "find_attempts.cpp")).read()
    space = open(os.path.join(CSRC, "workspace.cpp")).read()
    auto = open(os.path.join(CSRC, "automaton.hpp")).read()
    out: Dict[str, int] = {}

    def plain(name, src, where):
        m = re.search(r"\b%s\s*=\s*(\d+)\s*[,;]" % name, src)
        assert m, f"{name} is no longer a plain constant of {where}"
        out[name] = int(m.group(1))

    def defined(name, macro, src, where):
        assert re.search(r"\b%s\s*=\s*%s\s*;" % (name, macro), src), f"{name} is no longer {macro}"
        m = re.search(r"#define\s+%s\s+(\d+)\s*(?://.*)?$" % macro, src, re.M)
        assert m, f"{macro} is no longer a plain constant of {where}"
        out[name] = int(m.group(1))

    defined("STAGE_SLOTS", "ACX_STAGE_SLOTS", kern, "kernels.hip")
    for n in ("STAGE_SLOTS_W32", "STAGE_SLOTS_WIDE", "SUPER", "WRITE_CHUNK", "DT_COMPACT_WORDS", "W32_FIELD", "REL_BITS"):
        plain(n, kern, "kernels.hip")
    for n in ("TILE_BITS", "HIT_SLOTS", "MAX_LOOKBACK", "DT_SLOTS"):
        plain(n, types, "device_types.hpp")
    defined("GROUP_TILES", "ACX_GROUP_TILES", types, "device_types.hpp")
    defined("GROUP_MAX", "ACX_GROUP_MAX", types, "device_types.hpp")
    defined("DT_GROUP", "ACX_DT_GROUP", types, "device_types.hpp")
    m = re.search(r"\bGROUP_MAX_WIDE\s*=\s*(\d+)\s*\*\s*GROUP_MAX\s*;", types)
    assert m, "GROUP_MAX_WIDE is no longer a multiple of GROUP_MAX"
    out["GROUP_MAX_WIDE"] = int(m.group(1)) * out["GROUP_MAX"]
    assert re.search(r"\bDT_GMAX\s*=\s*DT_GROUP\s*\*\s*DT_SLOTS\s*;", types), "DT_GMAX is no longer DT_GROUP * DT_SLOTS"
    out["DT_GMAX"] = out["DT_GROUP"] * out["DT_SLOTS"]
    assert re.search(r"\bHOT_SUB\s*=\s*GROUP_TILES\s*/\s*DT_GROUP\s*;", types), "HOT_SUB is no longer GROUP_TILES / DT_GROUP"
    out["HOT_SUB"] = out["GROUP_TILES"] // out["DT_GROUP"]
    m = re.search(r"\bHOT_INLINE\s*=\s*(\d+)\s*,\s*HOT_INLINE_MAX\s*=\s*(\d+)\s*;", attempts)
    assert m, "HOT_INLINE / HOT_INLINE_MAX are no longer plain constants of find_attempts.cpp"
    out["HOT_INLINE"], out["HOT_INLINE_MAX"] = int(m.group(1)), int(m.group(2))
    plain("FILTER2_MAX_Q", auto, "automaton.hpp")
    # ---- what the plan's own arithmetic restates
    for pat, src, what in (
            # tile_lookback(): the context is longer than the longest pattern by at least 2 KiB
            (r"need\s*=\s*\(uint64_t\)\(max_len\s*\?\s*max_len\s*-\s*1\s*:\s*0\)\s*\+\s*2048\s*;", kern, "tile_lookback()'s slack"),
            (r"return\s*\(uint32_t\)\(\(need\s*\+\s*\(1u\s*<<\s*TILE_BITS\)\s*-\s*1\)\s*>>\s*TILE_BITS\)\s*;", kern, "tile_lookback()'s rounding"),
            (r"a->sparse_ok\s*=\s*tile_lookback\(a->host\.max_len\)\s*<=\s*MAX_LOOKBACK\s*;",
             open(os.path.join(CSRC, "build_upload.cpp")).read(), "sparse_ok"),
            # complete and wlow: first_idx + (max_len - 1)
            (r"margin\s*=\s*A\.max_len\s*\?\s*A\.max_len\s*-\s*1\s*:\s*0\s*;", kern, "margin"),
            (r"complete\s*=\s*first\s*==\s*0\s*\?\s*0\s*:\s*first_idx\s*\+\s*\(key_mode\s*==\s*0\s*\?\s*margin\s*:\s*0\)\s*;", kern, "complete"),
            (r"wlow\s*=\s*first\s*==\s*0\s*\?\s*0\s*:\s*\(int32_t\)margin\s*;", kern, "wlow"),
            (r"first\s*=\s*tile0\s*>=\s*lookback\s*\?\s*tile0\s*-\s*lookback\s*:\s*0\s*;", kern, "the first staged tile"),
            (r"kidx\s*=\s*\(key_mode\s*==\s*0\s*\?\s*ps\s*\+\s*L\s*:\s*ps\)\s*\+\s*lead\s*;", kern, "the key index"),
            (r"if\s*\(kidx\s*<\s*complete\s*\|\|\s*kidx\s*>=\s*idx_hi\)\s*return\s*;", kern, "what a group stages"),
            # the limits themselves
            (r"if\s*\(r\s*<\s*SLOTS\)", kern, "r < SLOTS"),
            (r"if\s*\(total\s*>\s*T\.gmax\)", kern, "total > T.gmax"),
            (r"accepted\s*=\s*cnt\s*>=\s*8\s*\*\s*sizeof\(MK\)\s*\?\s*~\(MK\)0\s*:", kern, "the accept mask"),
            (r"if\s*\(s\s*>=\s*wlow\s*&&\s*m\s*<=\s*s\)", kern, "the certification"),
            (r"overfull\s*=\s*c\s*>\s*HIT_SLOTS\s*;", kern, "an overfull tile"),
            (r"sum\s*=\s*t\s*<\s*gq\s*\?\s*\(T\.btot\[sg\s*\*\s*SUPER\s*\+\s*t\]\s*&\s*~HOT_BIT\)\s*:\s*0\s*;", kern, "t < gq"),
            (r"for\s*\(uint32_t\s+k\s*=\s*t\s*;\s*k\s*<\s*sg\s*;\s*k\s*\+=\s*64\)", kern, "k < sg"),
            (r"if\s*\(c\s*>\s*0\s*&&\s*hs\[c\s*-\s*1\]\s*==\s*h\)\s*continue\s*;", kern, "the run-head test"),
            (r"if\s*\(L\.first_sync\s*>\s*out0\)", kern, "L.first_sync > out0"),
            (r"if\s*\(t\s*==\s*63\)\s*tail_base\s*=\s*incl\s*;", kern, "tail_base"),
            (r"if\s*\(t\s*>=\s*64\s*&&\s*t\s*<\s*128\)\s*incl\s*\+=\s*tail_base\s*;", kern, "incl += tail_base"),
            # the three forms: (W32, threads, slots)
            (r"ACX_TILE_MAIN_W\(AN,\s*false,\s*true,\s*ACX_MAIN_THREADS_W32,\s*STAGE_SLOTS_W32\)", kern, "the narrow form"),
            (r"else\s+ACX_TILE_MAIN_W\(AN,\s*false,\s*false,\s*MAIN_THREADS,\s*STAGE_SLOTS\)", kern, "the 64-bit-word form"),
            (r"ACX_TILE_MAIN_W\(AN,\s*false,\s*false,\s*MAIN_THREADS,\s*STAGE_SLOTS_WIDE\)", kern, "the wide form"),
            (r"#define\s+ACX_MAIN_THREADS_W32\s+128\b", kern, "the narrow form's 128 threads"),
            (r"#define\s+ACX_MAIN_THREADS\s+256\b", kern, "the 256 threads"),
            (r"wide\s*=\s*T\.gmax\s*>\s*GROUP_MAX\s*;", kern, "how tile_post() knows the wide form"),
            (r"gmax\s*=\s*wide\s*\?\s*GROUP_MAX_WIDE\s*:\s*GROUP_MAX\s*;", attempts, "gmax"),
            # n_groups = ceil((tiles + 1) / GROUP_TILES)
            (r"groups\s*=\s*\(tiles\s*\+\s*1\s*\+\s*GROUP_TILES\s*-\s*1\)\s*/\s*GROUP_TILES\s*;", space, "n_groups"),
            # a handle is held on the dense path, or redone wide, only from these sizes on
            (r"n_hot\s*\*\s*4\s*>\s*T\.n_groups\s*&&\s*T\.n_groups\s*>=\s*8", attempts, "dense_hold after many hot groups"),
            (r"T\.n_groups\s*>=\s*32\s*&&\s*n_hot\s*\*\s*32\s*>\s*T\.n_groups", attempts, "the wide redo")):
        assert re.search(pat, src), f"the sources no longer define {what} as the plan restates it"
    # sort_bucket<1|2|4|8>: 64 / 128 / 256
    for n, k in ((64, 1), (128, 2), (256, 4)):
        assert re.search(r"n\s*<=\s*%d\)\s*sort_bucket<%d>" % (n, k), kern), f"sort_bucket<{k}> is no longer taken up to {n}"
    assert re.search(r"else\s+sort_bucket<8>", kern), "sort_bucket<8> no longer takes the rest"
    # the switches, read by these names where the plan believes they are
    for name, src, pat in (
            ("ACX_MAIN_WIDE", kern, r"static\s+const\s+bool\s+wide_env\s*=\s*std::getenv\(\"ACX_MAIN_WIDE\"\)"),
            ("ACX_FORCE_WIDE", attempts, r"static\s+const\s+bool\s+force_wide\s*=\s*std::getenv\(\"ACX_FORCE_WIDE\"\)"),
            ("ACX_NO_WIDE", attempts, r"static\s+const\s+bool\s+no_wide\s*=\s*std::getenv\(\"ACX_NO_WIDE\"\)"),
            ("ACX_NO_BUCKET", attempts, r"no_sparse_env\s*=\s*std::getenv\(\"ACX_NO_BUCKET\"\)"),
            ("ACX_NO_DENSE_COMPACT", attempts, r"static\s+const\s+bool\s+no_compact\s*=\s*std::getenv\(\"ACX_NO_DENSE_COMPACT\"\)"),
            ("ACX_NO_DENSE_TILES", attempts, r"no_tiles_env\s*=\s*std::getenv\(\"ACX_NO_DENSE_TILES\"\)"),
            ("ACX_NO_SPEC_HOT", attempts, r"static\s+const\s+bool\s+no_spec\s*=\s*std::getenv\(\"ACX_NO_SPEC_HOT\"\)")):
        assert re.search(pat, src), f"{name} is no longer read where the plan believes it is"
    return out


C = source_constants()
TILE = 1 << C["TILE_BITS"]
GT = C["GROUP_TILES"]
GROUP = GT * TILE
HIT_SLOTS, GROUP_MAX, GROUP_MAX_WIDE, CHUNK = C["HIT_SLOTS"], C["GROUP_MAX"], C["GROUP_MAX_WIDE"], C["WRITE_CHUNK"]


class Form(NamedTuple):
    name: str
    env: Optional[str]  # the switch its child runs under
    slots: int
    gmax: int
    narrow: bool


FORMS = (Form("narrow", None, C["STAGE_SLOTS_W32"], GROUP_MAX, True),
         Form("words64", "ACX_MAIN_WIDE", C["STAGE_SLOTS"], GROUP_MAX, False),
         Form("wide", "ACX_FORCE_WIDE", C["STAGE_SLOTS_WIDE"], GROUP_MAX_WIDE, True))
# further legs, each a switch read once per process (one child each): k_dense_main's full form for every dense call, no hot
# pipeline queued ahead, no redo in the wide form.  k_tile_main runs in its narrow form in them.
LEGS = (Form("full", "ACX_NO_DENSE_COMPACT", C["STAGE_SLOTS_W32"], GROUP_MAX, True),
        Form("nospec", "ACX_NO_SPEC_HOT", C["STAGE_SLOTS_W32"], GROUP_MAX, True),
        Form("nowide", "ACX_NO_WIDE", C["STAGE_SLOTS_W32"], GROUP_MAX, True))
FORM = {f.name: f for f in FORMS + LEGS}
KM_KINDS = {0: ((0, False), (0, True)), 1: ((1, False), (2, False))}  # the kinds of a key mode


def key_mode(mk: int, ov: bool) -> int:
    return 0 if ov else mk


def tile_lookback(max_len: int) -> int:
    need = (max_len - 1 if max_len else 0) + 2048
    return (need + TILE - 1) >> C["TILE_BITS"]


def longest_for(lookback: int) -> int:
    """the longest pattern that `lookback` context tiles admit"""
    return lookback * TILE - 2048 + 1


def n_groups(lead: int, n: int) -> int:
    tiles = (lead + n + TILE - 1) // TILE
    return (tiles + 1 + GT - 1) // GT


# ---------------------------------------------------------------------------
# pattern sets
# ---------------------------------------------------------------------------
S = b"qwert"      # the staircases' plant: no border of its own, one hit
N = b"qwertyu"    # ... and a second occurrence at the same start, on the same hit (a list of two)
X = b"xyzwx"      # overlaps itself by one byte
LINK_LEN = 201    # a chain's link: <= 21 links to a bucket, below every form's slots
LINK = b"k" + body(4100, LINK_LEN - 2) + b"k"  # ... overlaps itself by one byte


LINK4_LEN = 4 * (1 << 12) - 2048 + 1  # the longest link lookback 4 admits
LINK4 = b"k" + body(4400, LINK4_LEN - 2) + b"k"
BIG = b"B" + b"".join(b"z" + body(6000 + i, 7) for i in range(250))[:1999]  # 2 000 bytes that hold 250 occurrences of "z"


def long_pattern(n: int) -> bytes:
    """n bytes that end in X's first byte: an X can overlap its last byte"""
    return b"L" + body(5000 + n, n - 2) + X[:1]


@functools.lru_cache(maxsize=None)
def patterns(set_name: str) -> Tuple[bytes, ...]:
    """"p": the short ones; "chain": + LINK; "L<n>": + one pattern of n bytes"""
    if set_name == "p":
        return (S, X, N)
    if set_name == "chain":
        return (S, X, N, LINK)
    if set_name == "big":
        return (b"z", BIG)
    if set_name == "urls":  # ANCH (max_shift != 0): verify_seams' URL-like set
        import verify_seams
        return verify_seams.patterns("urls")
    if set_name == "w4":
        # lookback MAX_LOOKBACK and, with 104 patterns, a tie field of 7 bits beside 14 bits of length: tile_words_narrow()
        # refuses the set -- 64-bit staged words BY ITSELF (STAGE_SLOTS slots, 256 threads; under ACX_FORCE_WIDE the third
        # instantiation of the wide form).  The hundred further patterns occur nowhere.
        return (S, X, N, LINK4) + tuple(b"Z" + body(7000 + i, 6) for i in range(100))
    assert set_name[0] == "L"
    return (S, X, N, long_pattern(int(set_name[1:])))


def max_len(set_name: str) -> int:
    return max(len(p) for p in patterns(set_name))


def q2_of(set_name: str) -> int:
    return min(C["FILTER2_MAX_Q"], min(len(p) for p in patterns(set_name) if len(p) > 2))


@functools.lru_cache(maxsize=None)
def oracle(set_name: str, mk: int) -> Oracle:
    return Oracle(list(patterns(set_name)), mk, KIND_DFA)


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
SPARSE = (1, 0, 0, 0)       # (sparse, hot_calls, hot_groups, dense_tiles + dense_radix)
HOT1, HOT2 = (0, 1, 1, 0), (0, 1, 2, 0)
DENSE = (0, 0, 0, 1)


class Case(NamedTuple):
    name: str
    cls: str                 # a | b | c | e
    set: str
    forms: Tuple[str, ...]
    km: Optional[int]        # the key mode it is built for (None: for all four kinds)
    lead: int
    hay: np.ndarray
    stats: Dict[Tuple[int, bool], tuple]  # per (kind, overlapping): what path_stats must say
    geo: Dict                # what test_post_seams_cpu.py recomputes from the oracle's rows
    radix: bool = False      # DENSE: by the radix form (dense_radix == 1)
    tiles: bool = False      # DENSE: by the tile-ordered form (dense_tiles == 1)
    env: Tuple[str, ...] = ()  # switches read per call that the case runs under
    cp: bool = False         # codepoints=True: k_tile_main<CP> carries the start chunk's lead-byte count into k_tile_write<CPW>

    @property
    def kinds(self):
        return KINDS if self.km is None else KM_KINDS[self.km]


class Hay:
    """a stream of n filler bytes at pointer residue `lead`; plants by INDEX"""

    def __init__(self, n: int, lead: int = 0):
        self.n, self.lead = n, lead
        self.buf = np.full(n, CLEAN, dtype=np.uint8)
        self.used = np.zeros(n, dtype=bool)

    def put(self, idx: int, data: bytes, over: int = 0):
        """`data` starts at index idx; over: its first `over` bytes may lie on a plant (and must agree with it)"""
        p = idx - self.lead
        assert 0 <= p and p + len(data) <= self.n, (idx, len(data))
        d = np.frombuffer(data, dtype=np.uint8)
        assert not self.used[p + over:p + len(d)].any() and np.array_equal(self.buf[p:p + over], d[:over]), idx
        self.buf[p:p + len(d)] = d
        self.used[p:p + len(d)] = True

    def put_key(self, key_idx: int, data: bytes, km: int):
        """... so that its KEY (km 0: the end, km 1: the start) has index key_idx"""
        self.put(key_idx - len(data) if km == 0 else key_idx, data)


PITCH = 40   # between the plants of a bucket (up to 29 of them)
PITCH_WIDE = 28  # ... of the wide form's (up to 65 of them in the 1 900 bytes of a partial tile)
FIRST = 16   # a bucket's first key offset: behind what a straddling plant takes of the tile


def fill_bucket(h: Hay, tile: int, k: int, km: Optional[int], form: Form, how: str = "inside"):
    """k occurrences whose keys lie in bucket `tile`, no tile above HIT_SLOTS hits.  inside: k plants of S in the tile.
    straddle (km 0): the first one, X, starts two bytes in front of the tile and ends in it -- its hit is the tile's in
    front.  pairs (km 1): S and N at one start, two occurrences on ONE hit (k odd: and a lone S)."""
    pitch = PITCH_WIDE if form.slots > 32 else PITCH
    base = tile * TILE + FIRST
    if how == "straddle":
        assert km == 0
        h.put(tile * TILE - 2, X)
        k -= 1
    if how == "pairs":
        assert km == 1
        for i in range(k // 2):
            h.put(base + i * pitch, N)
        if k % 2:
            h.put(base + (k // 2) * pitch, S)
        return
    for i in range(k):  # (wholly inside the tile: start and end, the key of either mode, are the tile's)
        h.put(base + i * pitch, S)


def spread(n: int, buckets: int) -> List[int]:
    return [n // buckets + (1 if i < n % buckets else 0) for i in range(buckets)]


def fill_group(h: Hay, tiles: List[int], n: int, km: Optional[int], form: Form):
    """n occurrences of S, their keys spread evenly over the buckets `tiles`"""
    for t, k in zip(tiles, spread(n, len(tiles))):
        fill_bucket(h, t, k, km, form)


DENSE_PITCH = 7  # up to 585 plants of S to a tile (dense_fill)
STAIR_LEN = 2 * GROUP + 6 * TILE + 1900  # groups 0 and 1 whole, the last tile partial


def stair_buckets() -> Dict[str, Tuple[int, int]]:
    """bucket staircase: name -> (tile, hot groups at SLOTS + 1)"""
    last = (STAIR_LEN - 1) // TILE
    return {"g0_first": (0, 1), "g1_first": (GT, 1), "g1_b5": (GT + 5, 1), "last_partial": (last, 1),
            # the last context tile of group 1 (lookback 1): group 0 reports it, group 1 stages it too -- both give up
            "context": (GT - 1, 2),
            # bucket 63 of group 1, the last key before the next group's idx_hi: group 2's context as well
            "g1_last": (2 * GT - 1, 2)}


@functools.lru_cache(maxsize=None)
def cases_a() -> Tuple[Case, ...]:
    out = []
    for f in FORMS:
        for where, (tile, hot) in stair_buckets().items():
            # the wide form: SLOTS + 1 starts in one tile would be HIT_SLOTS + 1 hits there -- a straddling first plant
            # (km 0) or two occurrences a hit (km 1) fill the bucket and leave the tiles at or below their slots
            for km, how in ((None, "inside"), (0, "straddle"), (1, "pairs")):
                if how == "straddle" and tile == 0:
                    continue  # (nothing in front of the stream)
                for k in (f.slots - 1, f.slots, f.slots + 1):
                    if how == "inside" and k > HIT_SLOTS:
                        continue
                    h = Hay(STAIR_LEN)
                    fill_bucket(h, tile, k, km, f, how)
                    # (the straddling plant ends 3 bytes into the context tile, in front of `complete` = first_idx + max_len
                    # - 1: group 1 does not stage it, its copy of the bucket stays at SLOTS and only group 0 gives up)
                    n_hot = 1 if how == "straddle" and where in ("context", "g1_last") else hot
                    st = SPARSE if k <= f.slots else (HOT1 if n_hot == 1 else HOT2)
                    kinds = KINDS if km is None else KM_KINDS[km]
                    out.append(Case(f"a_{f.name}_{where}_{how}_k{k}", "a", "p", (f.name,), km, 0, h.buf,
                                    {kd: st for kd in kinds}, {"bucket": tile, "fill": k, "slots": f.slots, "how": how}))
        # ... and ANCH (k_tile_main<true, ..>): an anchored pattern's hit lies behind its start.  "anch": the staircase inside the
        # bucket; "anch_ahead" (key mode 1, bucket 63 of group 1): the last plant starts in the group's last two bytes -- its
        # hit lies in the NEXT group's first tile, the look-ahead tile group 1 reads for it (and the wide form reaches 65 keys
        # with 64 hits in the tile)
        U, shift = anchored_plant()
        for where, km, how in (("g1_first", None, "anch"), ("g1_last", None, "anch"), ("g1_last", 1, "anch_ahead")):
            tile, hot = stair_buckets()[where]
            for k in (f.slots - 1, f.slots, f.slots + 1):
                if how == "anch" and k > HIT_SLOTS:
                    continue
                h = Hay(STAIR_LEN)
                for i in range(k - (how == "anch_ahead")):
                    h.put(tile * TILE + FIRST + i * (PITCH_WIDE if f.slots > 32 else PITCH), U)
                if how == "anch_ahead":
                    h.put((tile + 1) * TILE - 2, U)
                st = SPARSE if k <= f.slots else (HOT1 if hot == 1 else HOT2)
                out.append(Case(f"a_{f.name}_{where}_{how}_k{k}", "a", "urls", (f.name,), km, 0, h.buf,
                                {kd: st for kd in (KINDS if km is None else KM_KINDS[km])},
                                {"bucket": tile, "fill": k, "slots": f.slots, "how": how, "shift": shift}))
        if f.name == "words64":
            # ... and as code points over two-byte characters: k_tile_main<CP> (STAGE_SLOTS slots, 128 threads), whatever the
            # words the set would get -- the default process
            for where in ("g1_first", "g1_last"):
                tile, hot = stair_buckets()[where]
                for k in (f.slots - 1, f.slots, f.slots + 1):
                    h = Hay(STAIR_LEN)
                    fill_bucket(h, tile, k, None, f)
                    st = SPARSE if k <= f.slots else (HOT1 if hot == 1 else HOT2)
                    out.append(Case(f"a_cp_{where}_k{k}", "a", "p", ("narrow",), None, 0, two_byte_filler(h.buf), {kd: st for kd in KINDS},
                                    {"bucket": tile, "fill": k, "slots": f.slots, "how": "inside"}, cp=True))
        if f.slots < HIT_SLOTS:  # ... and at a pointer residue: the bucket is the tile of key + lead
            for k in (f.slots, f.slots + 1):
                h = Hay(STAIR_LEN, 9)
                fill_bucket(h, GT + 5, k, None, f)
                out.append(Case(f"a_{f.name}_lead9_k{k}", "a", "p", (f.name,), None, 9, h.buf,
                                {kd: SPARSE if k <= f.slots else HOT1 for kd in KINDS},
                                {"bucket": GT + 5, "fill": k, "slots": f.slots, "how": "inside"}))
    return tuple(out)


B_LEN = 2 * GROUP + (GT - 2) * TILE + 1000  # three groups; the last one's last tile is partial


@functools.lru_cache(maxsize=None)
def cases_b() -> Tuple[Case, ...]:
    """group staircase: GROUP_MAX - 1, GROUP_MAX, GROUP_MAX + 1 reported matches in one group, 16 or 17 to a bucket.  The wide
    form cannot reach total > gmax (GROUP_MAX_WIDE + 1 accepted would need a bucket of STAGE_SLOTS_WIDE + 1): its case is
    the full house, STAGE_SLOTS_WIDE occurrences in each bucket and HIT_SLOTS hits in each tile of one group, and one more."""
    out = []
    assert n_groups(0, B_LEN) == 3
    whole = (B_LEN - 1) // TILE  # (the partial tile takes none)
    for g in (0, 1, 2):
        tiles = [t for t in range(g * GT, (g + 1) * GT) if t < whole]
        for n in (GROUP_MAX - 1, GROUP_MAX, GROUP_MAX + 1):
            h = Hay(B_LEN)
            fill_group(h, tiles, n, None, FORMS[0])
            st = SPARSE if n <= GROUP_MAX else HOT1
            out.append(Case(f"b_g{g}_n{n}", "b", "p", ("narrow", "words64"), None, 0, h.buf,
                            {kd: st for kd in KINDS}, {"group": g, "reported": n, "slots": C["STAGE_SLOTS"]}))
    f = FORM["wide"]
    assert f.slots * GT == GROUP_MAX_WIDE and f.slots == HIT_SLOTS
    tiles = list(range(GT, 2 * GT))
    for km in (0, 1):
        for more in (0, 1):
            h = Hay(B_LEN)
            if more and km == 0:  # the group's first bucket gets 65 keys, its tile 64 hits: the straddling plant's is group 0's
                fill_bucket(h, GT, f.slots + 1, 0, f, "straddle")
            elif more:            # an N in the place of one S: one occurrence more on the same hit
                fill_bucket(h, GT, f.slots + 1, 1, f, "pairs")
            for t in tiles:
                if not (more and t == GT):
                    fill_bucket(h, t, f.slots, None, f)
            out.append(Case(f"b_wide_full_house_km{km}_plus{more}", "b", "p", ("wide",), km, 0, h.buf,
                            {kd: HOT1 if more else SPARSE for kd in KM_KINDS[km]},
                            {"group": 1, "reported": None, "staged": GROUP_MAX_WIDE + more, "slots": f.slots}))
    return tuple(out)


C_LEN = 2 * GROUP + 3 * TILE + 700  # (a lookback-4 link that starts in tile GT + 8 ends in tile GT + 12)
ALL = tuple(f.name for f in FORMS)


def certified(spans: List[Tuple[int, int]], first_idx: int, margin: int) -> List[bool]:
    """the kernel's rule, restated: sorted by key, occurrence i of a group whose first staged index is first_idx is a
    certified sync point iff it starts at or behind wlow (0 in group 0, else first_idx + margin) and no staged occurrence
    in front of it ends behind its start"""
    wlow = first_idx + margin if first_idx else 0
    out, m = [], 0
    for s, e in spans:
        out.append(s >= wlow and m <= s)
        m = max(m, e)
    return out


@functools.lru_cache(maxsize=None)
def cases_c() -> Tuple[Case, ...]:
    out = []
    # ---- pairs: o1 and o2 touch (S S) or overlap by one byte (X X); o1's key in the bucket in front of a border, o2's key the
    # FIRST of the bucket behind it -- the chain of that bucket starts at o2 if o2 is certified.  Three borders in one stream:
    # a bucket border of group 1, the first tile of group 1's context, the border between context and output (the groups')
    # ... under lookback 1 (set "p", all three forms) and lookback 4 (set "w4": wide words by itself)
    for set_name, lb, forms, sfx in (("p", 1, ALL, ""), ("w4", C["MAX_LOOKBACK"], ("narrow", "wide"), "_lb4")):
      borders = {"bucket": (GT + 6) * TILE, "context": (GT - lb) * TILE, "group": GT * TILE}
      for pair, p, step in (("touch", S, len(S)), ("overlap", X, len(X) - 1)):
        for km in (0, 1):
            # km 1: o2 starts at the border + d, o1 `step` in front of it; km 0: o2 ENDS at the border + d
            for d, tag in ((0, "o2_first"), (step - 1, "o1_last")):
                h = Hay(C_LEN)
                at = {}
                for name, bd in borders.items():
                    s2 = bd + d if km == 1 else bd + d - len(p)
                    h.put(s2 - step, p)
                    h.put(s2, p, over=len(p) - step)
                    at[name] = (s2 - step, s2)
                out.append(Case(f"c_{pair}_km{km}_{tag}{sfx}", "c", set_name, forms, km, 0, h.buf, {kd: SPARSE for kd in KM_KINDS[km]},
                                {"pairs": at, "len": len(p), "borders": borders, "lookback": lb}))
    # ---- chains of LINKs, each overlapping the next by one byte, from group 1's context into its output.  first_idx + margin:
    # the first link is certified, every bucket's walk back ends there, the group stays sparse.  One byte earlier it is not
    # (s < wlow), and no link behind it is (each starts in front of the end of the one before): the walk leaves the stage,
    # group 1 gives up; the hot pipeline's dense group (DT_GROUP tiles from the same tile on, the same context) has no
    # certified sync point at or in front of its own first occurrence either (L.first_sync > out0), nor has the dense path's
    # tile-ordered form: the call ends on the radix form.  "shadowed": a link that starts one byte in front of the context and
    # covers the uncertifiable one's first byte -- that one is NOT reported, so an early certificate is a wrong answer, not
    # only a wrong path.  Overlapping calls have no sync points: always sparse.
    for set_name, lb, link, forms, sfx, reach in (("chain", 1, LINK, ALL, "", 2), ("w4", C["MAX_LOOKBACK"], LINK4, ("narrow", "wide"), "_lb4", 9)):
      first_idx = (GT - lb) * TILE
      margin = max_len(set_name) - 1
      assert tile_lookback(max_len(set_name)) == lb and len(link) == margin + 1
      for tag, start, shadow in (("certifiable", first_idx + margin, False), ("uncertifiable", first_idx + margin - 1, False),
                                 ("shadowed", first_idx + margin - 1, True)):
        h = Hay(C_LEN)
        links = []
        if shadow:
            h.put(first_idx - 1, link)
            links.append(first_idx - 1)
        x = start
        while x < (GT + reach) * TILE:
            h.put(x, link, over=1 if links and links[-1] + len(link) - 1 == x else 0)
            links.append(x)
            x += len(link) - 1
        st = {(0, True): SPARSE}
        for kd in ((0, False), (1, False), (2, False)):
            st[kd] = SPARSE if tag == "certifiable" else DENSE
        out.append(Case(f"c_chain_{tag}{sfx}", "c", set_name, forms, None, 0, h.buf, st,
                        {"links": tuple(links), "first_idx": first_idx, "margin": margin, "certifiable": tag == "certifiable",
                         "link_len": len(link)}, radix=tag != "certifiable"))
    # ---- the longest pattern each lookback admits, from a bucket's last byte on; a short occurrence at its end - 1 (overlaps
    # it by one byte) or at its end (touches it): the short one's walk back to the long one -- its only company -- crosses
    # the empty buckets in between
    for lb in range(1, C["MAX_LOOKBACK"] + 1):
        L = longest_for(lb)
        name = "L%d" % L
        assert tile_lookback(L) == lb and tile_lookback(L + 1) == lb + 1
        for km in (0, 1):
            for tag, p, d in (("overlap", X, -1), ("touch", S, 0)):
                h = Hay(C_LEN)
                s1 = (GT + 9) * TILE - 1 if km == 1 else (GT + 9) * TILE - 1 - L  # (km 0: its END is a bucket's last byte)
                h.put(s1, long_pattern(L))
                s2 = s1 + L + d
                h.put(s2, p, over=-d)
                out.append(Case(f"c_long_lb{lb}_km{km}_{tag}", "c", name, ALL, km, 0, h.buf, {kd: SPARSE for kd in KM_KINDS[km]},
                                {"long": (s1, s1 + L), "short": (s2, s2 + len(p)), "lookback": lb}))
    # ---- one byte beyond MAX_LOOKBACK's reach: never the sparse kernels
    L = longest_for(C["MAX_LOOKBACK"]) + 1
    h = Hay(C_LEN)
    h.put((GT + 9) * TILE - 1, long_pattern(L))
    h.put(5 * TILE, S)
    out.append(Case("c_beyond_reach", "c", "L%d" % L, ("narrow",), None, 0, h.buf, {kd: DENSE for kd in KINDS},
                    {"lookback": C["MAX_LOOKBACK"] + 1}))
    return tuple(out)


E_LEN = 2 * GROUP + 5 * TILE + 300
E_N = (1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1, GROUP_MAX)
E_N_WIDE = (GROUP_MAX + 1, GROUP_MAX_WIDE)
E_FRONT, E_BEHIND = 3, 2  # matches of group 0 and group 2: the stretch of group 1 begins behind the first


def write_hay(n: int, form: Form) -> np.ndarray:
    h = Hay(E_LEN)
    fill_bucket(h, 3, E_FRONT, None, form)
    fill_group(h, list(range(GT, 2 * GT)), n, None, form)
    fill_bucket(h, 2 * GT + 1, E_BEHIND, None, form)
    return h.buf


def two_byte_filler(hay: np.ndarray) -> np.ndarray:
    """every run of filler bytes as two-byte characters (and one '-' where the run is odd): the same offsets, valid UTF-8,
    code points and bytes part ways"""
    out = hay.copy()
    f = np.flatnonzero(np.diff(np.concatenate([[0], (hay == CLEAN).astype(np.int8), [0]])))
    for lo, hi in zip(f[::2].tolist(), f[1::2].tolist()):
        even = lo + (hi - lo) // 2 * 2
        out[lo:even:2], out[lo + 1:even:2] = 0xC3, 0xA9
    return out


@functools.lru_cache(maxsize=None)
def cases_e() -> Tuple[Case, ...]:
    """group 1 reports n matches: the write kernel's chunks of WRITE_CHUNK end in front of, at and behind the stretch's end"""
    out = []
    for n in E_N + E_N_WIDE:
        forms = ALL if n <= GROUP_MAX else ("wide",)
        hay = write_hay(n, FORM["wide"] if n > GROUP_MAX else FORMS[0])
        out.append(Case(f"e_n{n}", "e", "p", forms, None, 0, hay, {kd: SPARSE for kd in KINDS}, {"group": 1, "reported": n}))
        if n <= GROUP_MAX:  # ... and as code points, over a filler of two-byte characters (the CP form stages 64-bit words)
            out.append(Case(f"e_n{n}_cp", "e", "p", forms, None, 0, two_byte_filler(hay), {kd: SPARSE for kd in KINDS},
                            {"group": 1, "reported": n}, cp=True))
    return tuple(out)


class Batch(NamedTuple):
    name: str
    hay: np.ndarray
    offsets: Optional[Tuple[int, ...]]  # ragged: n_hay + 1 of them
    row_length: int                     # uniform: the haystacks' length
    geo: Dict


def match_starts(hay: np.ndarray) -> np.ndarray:
    """starts of the S plants (the batches hold nothing else)"""
    a = hay.tobytes()
    out, x = [], a.find(S)
    while x >= 0:
        out.append(x)
        x = a.find(S, x + 1)
    return np.array(out, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def batches() -> Tuple[Batch, ...]:
    """the same streams as batches (km 1 plants; every kind runs them -- a haystack border cuts no plant).  ragged: haystack
    borders behind matches 255 and 256 of group 1's stretch (chunk 0 ends between them), a run of one haystack's matches
    that the chunk border cuts (250 .. 259), two EMPTY haystacks at the border behind match 256, and a long haystack
    over the rest.  uniform: rows of 256 bytes, 300 one-match haystacks inside group 1 (a chunk of 256 runs of one, then 44),
    every other row empty."""
    out = []
    hay = write_hay(2 * CHUNK + 1, FORMS[0])
    st = match_starts(hay)
    g1 = st[E_FRONT:]  # group 1's stretch, in output order
    assert (g1[:2 * CHUNK + 1] // GROUP == 1).all()
    cut = lambda i: int(g1[i]) - 3  # a border in front of match i of the stretch
    offs = [0, 100, int(st[1]) - 1, cut(0), cut(250), cut(255), cut(256), cut(256), cut(256), cut(257), cut(260), cut(2 * CHUNK), len(hay)]
    assert offs == sorted(offs)
    out.append(Batch("ragged", hay, tuple(offs), 0, {"behind": (250, 255, 256, 257, 260, 2 * CHUNK), "empty_at": 256}))
    row = 256
    h = Hay(E_LEN - E_LEN % row)
    for r in range(300):
        h.put(GROUP + 16 * TILE + r * row + 100, S)
    h.put(5 * row + 7, S)
    h.put(2 * GROUP + 3 * row, S)
    out.append(Batch("uniform", h.buf, None, row, {"rows_in_group_1": 300}))
    return tuple(out)


def batch_bounds(b: Batch) -> np.ndarray:
    return np.array(b.offsets if b.offsets else range(0, len(b.hay) + 1, b.row_length), dtype=np.int64)


def batch_expected(b: Batch, mk: int, ov: bool) -> Tuple[np.ndarray, np.ndarray]:
    """(rows with offsets local to their haystack, matches per haystack): the oracle on every haystack by itself"""
    bd = batch_bounds(b)
    o = oracle("p", mk)
    rows, counts = [], np.zeros(len(bd) - 1, dtype=np.uint64)
    whole = o.find_raw(b.hay, overlapping=ov).astype(np.uint64)
    hs = np.searchsorted(bd, whole[:, 1].astype(np.int64), side="right") - 1
    for i in np.unique(hs):  # (only the haystacks that hold something: the others are filler)
        r = o.find_raw(np.ascontiguousarray(b.hay[bd[i]:bd[i + 1]]), overlapping=ov).astype(np.uint64)
        rows.append(r)
        counts[i] = len(r)
    return (np.concatenate(rows) if rows else np.zeros((0, 3), np.uint64)), counts


# ---- (g) sequences on one handle: six inputs, twice in a row and then in reverse -- every call under both parities of the
# call's sequence number (the two sets of supergroup words, the two control blocks) and behind a sparse call, a hot one (which
# makes the next call queue the hot pipeline ahead), and one of another size.  Order and paths: SEQ_PATHS.  None gives up, so
# the handle is never held on the dense path.
@functools.lru_cache(maxsize=None)
def sequence_inputs(form: str) -> Tuple[Tuple[str, np.ndarray, tuple], ...]:
    """(plants with two occurrences a hit: the streams suit all four kinds and leave the wide form's tiles at their slots)"""
    f = FORM[form]
    out = []
    for name, tile, k in (("sparse_small", 2, 3), ("hot_bucket", GT + 5, f.slots + 1), ("sparse_b", GT + 5, f.slots)):
        h = Hay(STAIR_LEN if name != "sparse_small" else 3 * TILE + 5)
        fill_bucket(h, tile, k, 1, f, "pairs")
        out.append((name, h.buf, SPARSE if k <= f.slots else HOT1))
    out.append(("groups", write_hay(CHUNK + 1, f), SPARSE))
    h = Hay(B_LEN)
    if f.gmax == GROUP_MAX:  # a group of GROUP_MAX + 1; the wide form: the full house and one more
        fill_group(h, list(range(GT, 2 * GT)), GROUP_MAX + 1, None, f)
    else:
        for t in range(GT, 2 * GT):
            fill_bucket(h, t, f.slots + (1 if t == GT + 7 else 0), 1, f, "pairs" if t == GT + 7 else "inside")
    out.append(("hot_group", h.buf, HOT1))
    out.append(("empty", np.full(GROUP + 77, CLEAN, dtype=np.uint8), SPARSE))
    # one tile of REGROW_HITS hits: REGROW_HITS - HIT_SLOTS of them go to the tile's overflow list, which holds OVF_PER_TILE
    # records a tile of the workspace shared among OVF_LISTS lists -- a handful here: the lists are regrown and the call made
    # again (overflow_regrown == 1 the first time, 0 on the same handle afterwards: SEQ_REGROWN); the bucket stays below DT_SLOTS
    h = Hay(STAIR_LEN)
    dense_fill(h, GT + 9, REGROW_HITS)
    out.append(("regrow", h.buf, HOT1))
    return tuple(out)


REGROW_HITS = 200


# ---- the hot pipeline queued AHEAD (attempt_sparse): behind a call with n hot groups the next call launches it for
# bound = min(2 n, HOT_INLINE_MAX, the context's hot_inline = HOT_INLINE, n_groups below 32 groups) hot groups and reads their
# number on the device.  One handle, five groups: 1 hot group (nothing queued ahead: the first call) -> bound 2: 2 hot groups, as
# many as the bound (the queued pipeline is the call's) -> bound 4: 5 hot groups, bound + 1 (its kernels return, the host runs the
# pipeline) -> none (they return, sparse) -> 1 again.  Fewer than 8 groups: no call holds the handle on the dense path.
LADDER_LEN = 4 * GROUP + 2000
LADDER = ((1,), (1, 2), (0, 1, 2, 3, 4), (), (3,))


def spec_bound(n_hot_before: int, groups: int) -> int:
    return min(2 * n_hot_before, C["HOT_INLINE_MAX"], C["HOT_INLINE"], groups // 32 if groups >= 32 else groups)


@functools.lru_cache(maxsize=None)
def ladder_inputs(form: str) -> Tuple[Tuple[np.ndarray, tuple], ...]:
    f = FORM[form]
    out = []
    for hot in LADDER:
        h = Hay(LADDER_LEN)
        for g in range(5):
            fill_bucket(h, g * GT, f.slots + 1 if g in hot else 2, 1, f, "pairs")
        out.append((h.buf, (0, 1, len(hot), 0) if hot else SPARSE))
    return tuple(out)


# ---- (d) the hits' prefix (hoff): every staged tile of group 1 holds another number of hits, 1 .. 64 and on from 1 -- staged
# tiles 63 | 64 are the seam between wave 0's and wave 1's halves of the prefix (tail_base) --, in group 0 (lb = 0) and in group 1
# with lookback 1 (nb = 65) and 4 (nb = 68: lanes 64 .. 67 add tail_base).  The hits are the first Q2 bytes of the set's long
# pattern on the filler: a hit that verifies to nothing; every 8th tile, and the tiles on either side of the group border and
# of the seam, end in an S -- the tile's LAST hit: h - hoff[tile] is then the largest the tile has.
D_LEN = 2 * GROUP + 3 * TILE + 500
D_PITCH = 8


def d_hits(tile: int, lb: int) -> int:
    return (tile - (GT - lb)) % 64 + 1


def d_has_s(tile: int, lb: int) -> bool:
    return tile % 8 == 0 or GT - lb - 1 <= tile <= GT or tile >= 2 * GT - 3 - lb


@functools.lru_cache(maxsize=None)
def cases_d() -> Tuple[Case, ...]:
    out = []
    for set_name, lb in (("chain", 1), ("L%d" % longest_for(C["MAX_LOOKBACK"]), C["MAX_LOOKBACK"])):
        assert tile_lookback(max_len(set_name)) == lb
        pre = patterns(set_name)[-1][:q2_of(set_name)]
        h = Hay(D_LEN)
        for tile in range(D_LEN // TILE):
            n = d_hits(tile, lb)
            for i in range(n):
                h.put(tile * TILE + 8 + i * D_PITCH, S if i == n - 1 and d_has_s(tile, lb) else pre)
        out.append(Case(f"d_lb{lb}", "d", set_name, ALL, None, 0, h.buf, {kd: SPARSE for kd in KINDS}, {"lookback": lb}))
    return tuple(out)


# ---- (g) hot groups against the output's room (run_hot): a device result's buffer has room for HOT_INLINE hot groups' worth of
# dense records; HOT_INLINE + 1 hot groups take the hot_totals branch and a buffer of the exact size.  n_groups >= 4 n_hot + 1:
# the handle is not held on the dense path; n_hot * 32 > n_groups: the call would be redone wide -- the ACX_NO_WIDE leg.
@functools.lru_cache(maxsize=None)
def cases_g() -> Tuple[Case, ...]:
    out = []
    f = FORM["nowide"]
    groups = 4 * (C["HOT_INLINE"] + 1) + 1
    for n_hot in (C["HOT_INLINE"], C["HOT_INLINE"] + 1):
        h = Hay((groups - 1) * GROUP + 3 * TILE)
        assert n_groups(0, h.n) == groups and n_hot * 32 > groups
        for g in range(groups):
            fill_bucket(h, g * GT + 2, f.slots + 1 if 1 <= g <= n_hot else 2, 1, f, "pairs")
        out.append(Case(f"g_hot_inline_{n_hot}", "g", "p", ("nowide",), None, 0, h.buf, {kd: (0, 1, n_hot, 0) for kd in KINDS},
                        {"hot": n_hot, "groups": groups}))
    return tuple(out)


def room_for_hot(groups: int, n_hot: int) -> Tuple[int, int]:
    """(records the output buffer of a fresh context holds, the bound run_hot computes for n_hot hot groups)"""
    cap = groups * GROUP_MAX + min(groups, C["HOT_INLINE"]) * C["HOT_SUB"] * C["DT_GMAX"]
    return cap, (groups - n_hot) * GROUP_MAX + n_hot * C["HOT_SUB"] * C["DT_GMAX"]


# ---- (g) a workspace that grows small -> large -> small: behind the 131-group stream of (f) sg_cap is larger than n_super, and
# the two small calls behind it (one of either seq parity) find both sets of supergroup words clear.  And a call that is REDONE
# in the wide form (32 groups, two hot: n_hot * 32 > n_groups) between hot calls of the narrow form: the redone call ends
# sparse with wide_redone == 1 and, with nothing hot left and few occurrences, hands the context back to the narrow form.
@functools.lru_cache(maxsize=None)
def named_sequence(form: str, which: str):
    """[(name, stream, path, further exact counters)]"""
    f = FORM[form]
    if which == "ladder":
        return tuple(("ladder%d" % i, h, p, {}) for i, (h, p) in enumerate(ladder_inputs(form)))
    if which == "seq":
        ins = sequence_inputs(form)
        out, seen = [], False
        for i in sequence_order():
            out.append(ins[i] + ({"overflow_regrown": int(ins[i][0] == "regrow" and not seen)},))
            seen = seen or ins[i][0] == "regrow"
        return tuple(out)
    small = sequence_inputs(form)[0]
    hot = sequence_inputs(form)[1]
    if which == "grow":
        big = next(c for c in cases_f() if form in c.forms)
        return (small + ({},), ("large", big.hay, HOT2, {}), small + ({},), small + ({},), hot + ({},), small + ({},))
    assert which == "redo" and f.gmax == GROUP_MAX
    h = Hay(31 * GROUP + 3 * TILE)
    assert n_groups(0, h.n) == 32
    for g in range(32):
        fill_bucket(h, g * GT + 2, f.slots + 1 if g in (7, 20) else 2, 1, f, "pairs")
    redo = ("redone_wide", h.buf, SPARSE, {"wide_redone": 1})
    return (hot + ({"wide_redone": 0},), redo, hot + ({"wide_redone": 0},), redo, small + ({"wide_redone": 0},))


def sequence_order() -> List[int]:
    n = len(sequence_inputs("narrow"))
    return [i for i in range(n) for _ in (0, 1)] + list(range(n - 1, -1, -1))


# ---- (h) k_dense_main, reached as the dense path proper (ACX_NO_BUCKET, read per call) and as the hot pipeline's tail (no
# switch: a tile of more than HIT_SLOTS hits, or a bucket above the form's slots, makes its group hot)
DT = C["DT_GROUP"]
H_LEN = 6 * DT * TILE + 900
H_FILLS = (64, 65, 128, 129, 256, 257, C["DT_SLOTS"] - 1, C["DT_SLOTS"], C["DT_SLOTS"] + 1)


def dense_fill(h: Hay, tile: int, k: int):
    for i in range(k):
        h.put(tile * TILE + i * DENSE_PITCH, S)


@functools.lru_cache(maxsize=None)
def cases_h() -> Tuple[Case, ...]:
    """bucket fills around sort_bucket's thresholds and DT_SLOTS, the bucket a dense group's first tile and its last (the
    next group's context); DT_COMPACT_WORDS and one more staged words in one dense group (compact -> full: path_stats has no
    word for it -- the plan's arithmetic and the right answer are the proof, as for K1b's second region pass); a first
    certified sync point exactly at the group's first own occurrence (nothing in front: first_sync == out0) and one element
    in front of it (a pair across the dense group's border); one 2 000-byte occurrence over 250 one-byte ones."""
    out = []
    proper = ("ACX_NO_BUCKET",)

    def both(name, set_name, hay, geo, lost=False):
        # dense path proper: the tile-ordered form, or (a bucket above DT_SLOTS) the radix form; default process: the hot
        # pipeline finishes the one hot group, or loses it and the call ends on the radix form
        out.append(Case("h_proper_" + name, "h", set_name, ("narrow", "full"), None, 0, hay, {kd: DENSE for kd in KINDS}, geo,
                        radix=lost, tiles=not lost, env=proper))
        out.append(Case("h_tail_" + name, "h", set_name, ("narrow",), None, 0, hay, {kd: DENSE if lost else HOT1 for kd in KINDS},
                        geo, radix=lost))

    # (context: under the set with lookback MAX_LOOKBACK a tile in the middle of dense group 1 is context to group 2 and the
    # first or last tile of no group)
    for where, tile, set_name in (("first", 2 * DT, "p"), ("last", 3 * DT - 1, "p"), ("context", 2 * DT - 2, "L%d" % longest_for(C["MAX_LOOKBACK"]))):
        for k in H_FILLS:
            h = Hay(H_LEN)
            dense_fill(h, tile, k)
            both(f"fill_{where}_k{k}", set_name, h.buf, {"bucket": tile, "fill": k, "where": where}, lost=k > C["DT_SLOTS"])
    for extra in (0, 1):  # DT_COMPACT_WORDS staged words in dense group 2, and one more
        h = Hay(H_LEN)
        for t in range(2 * DT, 2 * DT + C["DT_COMPACT_WORDS"] // C["DT_SLOTS"]):
            dense_fill(h, t, C["DT_SLOTS"])
        if extra:
            h.put((3 * DT - 1) * TILE + 9, S)
        both(f"words_{C['DT_COMPACT_WORDS'] + extra}", "p", h.buf, {"dense_group": 2, "words": C["DT_COMPACT_WORDS"] + extra})
    bd = 2 * DT * TILE  # the border in front of dense group 2 (not a group border of the sparse path)
    for pair, p, step in (("touch", S, len(S)), ("overlap", X, len(X) - 1)):
        for km in (0, 1):
            h = Hay(H_LEN)
            s2 = bd if km == 1 else bd - len(p)
            h.put(s2 - step, p)
            h.put(s2, p, over=len(p) - step)
            h.put(4 * DT * TILE, S)  # ... and a dense group whose first own occurrence is its first sync point
            geo = {"dense_pair": (s2 - step, s2), "len": len(p), "border": bd}
            out.append(Case(f"h_proper_{pair}_km{km}", "h", "p", ("narrow", "full"), km, 0, h.buf, {kd: DENSE for kd in KM_KINDS[km]},
                            geo, tiles=True, env=proper))
            # ... and as the hot pipeline's tail: a full bucket in the tile behind the pair makes the group hot
            h2 = Hay(H_LEN)
            h2.buf[:] = h.buf
            h2.used[:] = h.buf != CLEAN
            fill_bucket(h2, 2 * DT + 1, FORMS[0].slots + 1, 1, FORMS[0], "pairs")
            out.append(Case(f"h_tail_{pair}_km{km}", "h", "p", ("narrow",), km, 0, h2.buf, {kd: HOT1 for kd in KM_KINDS[km]}, geo))
    h = Hay(H_LEN)
    h.put(3 * DT * TILE - 700, BIG)
    both("big_over_250", "big", h.buf, {"big": (3 * DT * TILE - 700, 3 * DT * TILE - 700 + len(BIG))})
    return tuple(out)


# ---- (f) supergroups: 2 SUPER + 3 groups (33 MiB); group g reports g % 7 + 1 matches, so that no two prefixes of the counts
# coincide; the last group of supergroup 0 and the first of supergroup 1 are hot (a bucket of SLOTS + 1): their counts enter the
# places of the groups behind them through btot & ~HOT_BIT, the supergroup words and the hot write.  n_hot * 32 <= n_groups:
# the context does not switch to the wide form; n_hot * 4 <= n_groups: nor is it held on the dense path.
F_GROUPS = 2 * C["SUPER"] + 3
F_HOT = (C["SUPER"] - 1, C["SUPER"])


@functools.lru_cache(maxsize=None)
def cases_f() -> Tuple[Case, ...]:
    out = []
    n = (F_GROUPS - 1) * GROUP + 5 * TILE + 321
    assert n_groups(0, n) == F_GROUPS and len(F_HOT) * 32 <= F_GROUPS
    for f in FORMS:
        h = Hay(n)
        for g in range(F_GROUPS):
            if g in F_HOT:
                fill_bucket(h, g * GT + 3, f.slots + 1, 1, f, "pairs")
            else:
                fill_bucket(h, g * GT + 3, g % 7 + 1, None, f)
        out.append(Case(f"f_{f.name}", "f", "p", (f.name,), None, 0, h.buf, {kd: HOT2 for kd in KINDS},
                        {"hot": F_HOT, "slots": f.slots}))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def all_cases() -> Tuple[Case, ...]:
    return cases_a() + cases_b() + cases_c() + cases_d() + cases_e() + cases_h() + cases_f() + cases_g()


def cases_of(form: str, cls: str) -> List[Case]:
    return [c for c in all_cases() if form in c.forms and c.cls == cls]


CLASSES = ("a", "b", "c", "d", "e", "f", "g", "h")
_want: Dict[tuple, np.ndarray] = {}


def expected(c: Case, mk: int, ov: bool) -> np.ndarray:
    key = (c.name, mk, ov)
    if key not in _want:
        r = oracle(c.set, mk).find_raw(c.hay, overlapping=ov).astype(np.uint64)
        if c.cp and len(r):
            r = np.stack([r[:, 0], code_points_at(c.hay, r[:, 1]), code_points_at(c.hay, r[:, 2])], 1)
        r.setflags(write=False)
        _want[key] = r
    return _want[key]


def digest() -> str:
    h = hashlib.sha256()
    for c in all_cases():
        h.update(c.name.encode() + b"\0".join(patterns(c.set)) + c.hay.tobytes() + repr((sorted(c.stats.items()), c.radix, c.tiles, c.env, c.cp)).encode())
    for b in batches():
        h.update(b.name.encode() + b.hay.tobytes() + repr(b.offsets).encode() + str(b.row_length).encode())
    for f in FORMS:
        for name, hay, st in sequence_inputs(f.name):
            h.update(name.encode() + hay.tobytes() + repr(st).encode())
        for hay, st in ladder_inputs(f.name):
            h.update(hay.tobytes() + repr(st).encode())
    return h.hexdigest()


GOLDEN = os.path.join(ROOT, "tests", "golden", "post_seams_rows.json")


def rows_digests() -> Dict[str, str]:
    """name -> a digest of where every occurrence of the stream lies (the oracle's overlapping rows), its length and its
    pointer residue: tests/golden/post_seams_rows.json holds them as recorded, so that a plant moved by one byte INSIDE its
    bucket -- which no class's geometry sees -- fails on the CPU too.  A changed constant of the sources moves the plants with
    it: write_golden() records them again."""
    def d(set_name, hay, lead):
        r = oracle(set_name, 0).find_raw(hay, overlapping=True).astype(np.uint64)
        return hashlib.sha256(r.tobytes() + b"%d %d" % (len(hay), lead)).hexdigest()[:16]
    out = {c.name: d(c.set, c.hay, c.lead) for c in all_cases()}
    out.update({"batch_" + b.name: d("p", b.hay, 0) for b in batches()})
    for f in FORMS:
        out.update({f"seq_{f.name}_{name}": d("p", hay, 0) for name, hay, _ in sequence_inputs(f.name)})
        out.update({f"ladder_{f.name}_{i}": d("p", hay, 0) for i, (hay, _) in enumerate(ladder_inputs(f.name))})
    return out


def write_golden():
    with open(GOLDEN, "w") as f:
        json.dump(rows_digests(), f, indent=0, sort_keys=True)
        f.write("\n")


# ---------------------------------------------------------------------------
# the geometry, restated from the kernel's rules (test_post_seams_cpu.py holds every case against it)
# ---------------------------------------------------------------------------
def brute_leftmost(pats, hay, longest: bool) -> np.ndarray:
    """the two leftmost searches from bytes.find alone: the occurrence that starts first at or behind the end of the one
    before; at one start the lowest id (LeftmostFirst) or the longest, then the lowest id (LeftmostLongest)"""
    from k1b_seams import brute
    occ = sorted(((x, -(e - x) if longest else 0, i, e) for i, x, e in brute(pats, hay).tolist()))
    out, at = [], 0
    for x, _, i, e in occ:
        if x >= at:
            out.append((i, x, e))
            at = e
    return np.array(out, dtype=np.uint64).reshape(-1, 3)


def keys_of(rows: np.ndarray, km: int, lead: int) -> np.ndarray:
    return (rows[:, 2] if km == 0 else rows[:, 1]).astype(np.int64) + lead


def staged_buckets(occ: np.ndarray, km: int, lead: int, g: int, mlen: int) -> Dict[int, int]:
    """occurrences per bucket (tile of the key index) as group g stages them: complete <= key index < the group's end"""
    first = max(g * GT - tile_lookback(mlen), 0)
    complete = 0 if first == 0 else first * TILE + (mlen - 1 if km == 0 else 0)
    k = keys_of(occ, km, lead)
    k = k[(k >= complete) & (k < (g + 1) * GROUP)]
    t, n = np.unique(k >> C["TILE_BITS"], return_counts=True)
    return dict(zip(t.tolist(), n.tolist()))


def anchored_plant() -> Tuple[bytes, int]:
    """(the first URL pattern that is filed at least two bytes behind its beginning and is ONE occurrence where it stands
    alone, its shift): its hit lies `shift` bytes behind its start"""
    import verify_seams
    from k1b_seams import brute
    pats, shifts = patterns("urls"), verify_seams.host_tables("urls")[2]
    for p, sh in zip(pats, shifts):
        if sh >= 2 and p[:4] in (b"www.", b"ftp:") and len(brute(pats, b"--" + p + b"--")) == 1:
            return p, sh
    raise AssertionError("the URL set has no such pattern any more")


def hits_per_tile(set_name: str, hay: np.ndarray, lead: int) -> Dict[int, int]:
    """prefix hits: the positions at which the Q2 bytes a pattern is filed under stand -- its first ones, or (an anchored
    set) those `shift` bytes behind its beginning -- one hit however many patterns share them, by tile of the index"""
    q2, a = q2_of(set_name), hay.tobytes()
    pos = set()
    shifts = [0] * len(patterns(set_name))
    if set_name == "urls":
        import verify_seams
        shifts = verify_seams.host_tables("urls")[2]
    for pre in {p[sh:sh + q2] for p, sh in zip(patterns(set_name), shifts)}:
        x = a.find(pre)
        while x >= 0:
            pos.add(x)
            x = a.find(pre, x + 1)
    t, n = np.unique((np.array(sorted(pos), dtype=np.int64) + lead) >> C["TILE_BITS"], return_counts=True)
    return dict(zip(t.tolist(), n.tolist()))


def slots_of(c: Case, form: Form) -> int:
    """the slots of the instantiation the case runs in: the code-point form and a set that tile_words_narrow() refuses stage
    64-bit words -- STAGE_SLOTS where the set by itself would get STAGE_SLOTS_W32"""
    return C["STAGE_SLOTS"] if (c.cp or c.set == "w4") and form.gmax == GROUP_MAX else form.slots


def predicted_hot_groups(c: Case, form: Form, occ: np.ndarray, reported: np.ndarray, km: int) -> int:
    """groups that cannot finish by the limits alone: a staged bucket above the form's slots, or more reported matches than
    the form's stretch holds (chains are class (c)'s own business)"""
    hot = 0
    rk = keys_of(reported, km, c.lead)
    for g in range(n_groups(c.lead, len(c.hay))):
        b = staged_buckets(occ, km, c.lead, g, max_len(c.set))
        n = int(np.count_nonzero((rk >= g * GROUP) & (rk < (g + 1) * GROUP)))
        hot += int(max(b.values(), default=0) > slots_of(c, form) or n > form.gmax)
    return hot


# ---------------------------------------------------------------------------
# the device side (imports the library when called)
# ---------------------------------------------------------------------------
def path_of(st: Dict[str, int]) -> tuple:
    return (st["sparse"], st["hot_calls"], st["hot_groups"], st["dense_tiles"] + st["dense_radix"])


def run_case(c: Case) -> List[str]:
    """the case under each of its kinds, every call on a FRESH handle: element-wise against the oracle, path_stats against
    the plan"""
    from ahocorasick_rs_amd import capi
    fails = []
    dev = capi.DeviceBuffer(c.lead + len(c.hay) + 16)
    dev.upload(np.concatenate([np.full(c.lead, CLEAN, np.uint8), c.hay, np.zeros(16, np.uint8)]))
    assert dev.ptr % 16 == 0
    # (the overlapping call first: the buffers a fresh handle gets may be the ones the call before gave back, and behind the
    # non-overlapping call on the same stream they would hold that call's records at the same places)
    for mk, ov in sorted(c.kinds, key=lambda kd: not kd[1]):
        a = capi.Automaton(list(patterns(c.set)), mk, kernel=capi.KERNEL_PREFILTER)
        with with_env({k: "1" for k in c.env}):
            r = a.find_device(dev.ptr + c.lead, len(c.hay), overlapping=ov, codepoints=c.cp)
        got = cols(r.matches())
        r.free()
        st = a.path_stats()
        a.close()
        want = expected(c, mk, ov)
        if not np.array_equal(got, want):
            bad = next((i for i in range(min(len(got), len(want))) if not np.array_equal(got[i], want[i])), min(len(got), len(want)))
            fails.append(f"{c.name} kind {mk} overlapping {ov}: {len(got)} rows against {len(want)}, first difference at row {bad}")
        dense = c.stats[(mk, ov)] == DENSE
        if st["k0"] or path_of(st) != c.stats[(mk, ov)] or (dense and c.radix and st["dense_radix"] != 1) or (dense and c.tiles and st["dense_tiles"] != 1):
            fails.append(f"{c.name} kind {mk} overlapping {ov}: path {path_of(st)} k0 {st['k0']} radix {st['dense_radix']}, "
                         f"the plan says {c.stats[(mk, ov)]}{' by the radix form' if c.radix else ' by the tile-ordered form' if c.tiles else ''}")
    dev.free()
    return fails


def run_class(form: str, cls: str) -> Dict:
    fails, calls = [], 0
    for c in cases_of(form, cls):
        fails += run_case(c)
        calls += len(c.kinds)
    return {"form": form, "cls": cls, "calls": calls, "fails": fails[:40], "n_fails": len(fails)}


def run_batch(b: Batch, how: str) -> List[str]:
    """how: device (find_device with d_offsets / uniform_len) or host (find_batch); a fresh handle per call; rows and the
    counts per haystack element-wise"""
    from ahocorasick_rs_amd import capi
    fails = []
    bd = batch_bounds(b)
    for mk, ov in KINDS:
        a = capi.Automaton(list(patterns("p")), mk, kernel=capi.KERNEL_PREFILTER)
        want, want_counts = batch_expected(b, mk, ov)
        if how == "device":
            dev = capi.DeviceBuffer(len(b.hay) + 16)
            dev.upload(np.concatenate([b.hay, np.zeros(16, np.uint8)]))
            doff = None
            if b.offsets:
                doff = capi.DeviceBuffer(8 * len(bd))
                doff.upload(bd.astype(np.uint64).view(np.uint8))
            r = a.find_device(dev.ptr, len(b.hay), d_offsets=doff.ptr if doff else 0, n_hay=len(bd) - 1,
                              uniform_len=b.row_length if not b.offsets else 0, overlapping=ov)
            got, counts = cols(r.matches()), np.asarray(r.counts(), dtype=np.uint64)
            r.free()
            dev.free()
            if doff:
                doff.free()
        else:
            m, counts = a.find_batch([b.hay[bd[i]:bd[i + 1]].tobytes() for i in range(len(bd) - 1)], overlapping=ov)
            got = cols(m)
        st = a.path_stats()
        a.close()
        if not np.array_equal(got, want):
            fails.append(f"{b.name} {how} kind {mk} overlapping {ov}: {len(got)} rows against {len(want)}")
        if not np.array_equal(counts, want_counts):
            i = int(np.flatnonzero(counts != want_counts)[0]) if len(counts) == len(want_counts) else -1
            fails.append(f"{b.name} {how} kind {mk} overlapping {ov}: counts differ, first at haystack {i}: "
                         f"{counts[i] if i >= 0 else len(counts)} against {want_counts[i] if i >= 0 else len(want_counts)}")
        if st["k0"] or path_of(st) != SPARSE:
            fails.append(f"{b.name} {how} kind {mk} overlapping {ov}: path {path_of(st)} k0 {st['k0']}")
    return fails


def run_sequence(form: str, mk: int, ov: bool, which: str = "seq") -> List[str]:
    from ahocorasick_rs_amd import capi
    ins = named_sequence(form if FORM[form] in FORMS else "narrow", which)
    a = capi.Automaton(list(patterns("p")), mk, kernel=capi.KERNEL_PREFILTER)
    o = oracle("p", mk)
    fails = []
    for step, (name, hay, path, more) in enumerate(ins):
        dev = capi.DeviceBuffer(len(hay) + 16)
        dev.upload(np.concatenate([hay, np.zeros(16, np.uint8)]))
        a.path_stats(reset=True)
        r = a.find_device(dev.ptr, len(hay), overlapping=ov)
        got = cols(r.matches())
        r.free()
        dev.free()
        st = a.path_stats()
        if not np.array_equal(got, o.find_raw(hay, overlapping=ov).astype(np.uint64)):
            fails.append(f"step {step} ({name}) kind {mk} overlapping {ov}: wrong rows ({len(got)})")
        if st["k0"] or path_of(st) != path or any(st[k] != v for k, v in more.items()):
            fails.append(f"step {step} ({name}) kind {mk} overlapping {ov}: path {path_of(st)} {[st[k] for k in more]}, the plan says {path} {more}")
    a.close()
    return fails


SEQUENCES = ("seq", "ladder", "grow", "redo")


def child_main(form: str):
    """every class of one form, its batches and its sequences: one JSON line each"""
    f = FORM[form]
    assert f.env and os.environ.get(f.env), f.env
    for cls in CLASSES:
        if cases_of(form, cls):
            print("CLASS " + json.dumps(run_class(form, cls)), flush=True)
    if f in LEGS:
        if form == "nospec":  # the ladder with nothing queued ahead: the same rows and the same hot_groups, step by step
            for mk, ov in KINDS:
                print("SEQ " + json.dumps({"form": form, "cls": f"ladder_{mk}_{int(ov)}", "fails": run_sequence(form, mk, ov, "ladder")}), flush=True)
        print("DONE", flush=True)
        return
    for b in batches():
        for how in ("device", "host"):
            print("BATCH " + json.dumps({"form": form, "cls": b.name + "_" + how, "fails": run_batch(b, how)}), flush=True)
    for mk, ov in KINDS:
        print("SEQ " + json.dumps({"form": form, "cls": f"seq_{mk}_{int(ov)}", "fails": run_sequence(form, mk, ov)}), flush=True)
        for which in SEQUENCES[1:]:
            if which != "redo" or f.gmax == GROUP_MAX:
                print("SEQ " + json.dumps({"form": form, "cls": f"{which}_{mk}_{int(ov)}", "fails": run_sequence(form, mk, ov, which)}), flush=True)
    print("DONE", flush=True)


if __name__ == "__main__":
    child_main(sys.argv[1])
