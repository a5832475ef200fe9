"""K1b (k1b_prefilter<Q, SLOTS, CP, BIGV, SH>, csrc/kernels.hip) at its seams: the constants, the ten scan forms with a pattern
set each, the four sinks, the haystacks and the plan that tests/test_k1b_seams_cpu.py checks on the CPU and
tests/test_gpu_k1b_seams.py runs on the device.  Needs no GPU (run_leg() and what it calls import the library when called).

Expected rows are the oracle's (tests/oracle_lib.py); brute() / brute_iter() are a second, independent reference: bytes.find
in a loop.  Nothing expected comes from the library.  Sizes are read from the kernels' sources (source_constants()): a
changed constant moves the cases with it, a renamed one fails loudly.

The kernel works on the index space of the 16-byte aligned address below the haystack pointer: index = lead + stream
position; a lane owns 16 indexes, a row 1 KiB, a tile 4 KiB, a wave every (16 * workgroups)-th tile.  Every plant below is
placed by INDEX.  Two fillers: CLEAN, one byte ('-') that no pattern holds -- whatever is reported lies where something was
planted --, and the a-z + space alphabet of the first seam test, whose level 1 has false survivors to queue."""
from __future__ import annotations

import functools
import hashlib
import json
import os
import re
import sys
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

import gen
from oracle_lib import KIND_DFA, Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ahocorasick_rs_amd", "csrc")
CLEAN = ord("-")
ALPHABET = np.frombuffer(gen.AZ + b"      ", dtype=np.uint8)  # a-z, a space at one position in six
KINDS = [(0, False), (0, True), (1, False), (2, False)]  # (match kind, overlapping)
CPU_CUS = 256  # the CU count the plan is checked at on the CPU


# ---------------------------------------------------------------------------
# the constants of the sources
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def source_constants() -> Dict[str, int]:
    kern = open(os.path.join(CSRC, "kernels.hip")).read()
    types = open(os.path.join(CSRC, "device_types.hpp")).read()
    upload = open(os.path.join(CSRC, "build_upload.cpp")).read()
    attempts = open(os.path.join(CSRC, "find_attempts.cpp")).read()
    out = {}

    def plain(name, src, where):
        m = re.search(r"\b%s\s*=\s*(\d+)\s*[,;]" % name, src)
        assert m, f"{name} is no longer a plain constant of {where}"
        out[name] = int(m.group(1))

    for n in ("K1B_ROWS", "K1B_HB", "K1B_HB_BIG", "K1B_Q1CAP"):
        plain(n, kern, "kernels.hip")
    for n in ("TILE_BITS", "HIT_SLOTS", "OVF_LISTS"):
        plain(n, types, "device_types.hpp")
    m = re.search(r"\bK1B_STAGE_BYTES\s*=\s*(\d+)\s*\+\s*(\d+)\s*;", kern)
    assert m, "K1B_STAGE_BYTES is no longer a row + the bytes behind it"
    out["K1B_STAGE_BYTES"], out["STAGE_ROW"] = int(m.group(1)) + int(m.group(2)), int(m.group(1))
    # the bytes staged behind the row: ONE uint2 store at the row's end (two dwords), within the padding
    m = re.search(r"\*\(uint2 \*\)\(stg \+ (\d+)\) = make_uint2\(rx_, ry_\);", kern)
    assert m and int(m.group(1)) == out["STAGE_ROW"], "K1B_STAGE_ROW no longer stages a uint2 behind the row"
    out["STAGE_BEHIND"] = 2 * 4
    assert out["STAGE_ROW"] + out["STAGE_BEHIND"] <= out["K1B_STAGE_BYTES"]
    assert re.search(r"\bGROUP_TILES\s*=\s*ACX_GROUP_TILES\s*;", types), "GROUP_TILES is no longer ACX_GROUP_TILES"
    m = re.search(r"#define\s+ACX_GROUP_TILES\s+(\d+)\s*$", types, re.M)
    assert m, "ACX_GROUP_TILES is no longer a plain constant of device_types.hpp"
    out["GROUP_TILES"] = int(m.group(1))
    # what the plan's own arithmetic restates: the four tile bounds, the grid, the counts' batches, the regions' room
    for pat, what in (
            (r"t_int_lo\s*=\s*lead\s*\?\s*1u\s*:\s*0u\s*;", "t_int_lo"),
            (r"t_int_hi\s*=\s*\(uint32_t\)\(last_start\s*>>\s*TILE_BITS\)\s*;", "t_int_hi"),
            (r"t_full\s*=\s*\(uint32_t\)\(last_block\s*>>\s*TILE_BITS\)\s*;", "t_full"),
            (r"t_inside\s*=\s*total\s*>=\s*16\s*\?\s*\(uint32_t\)\(\(total\s*-\s*16\)\s*>>\s*TILE_BITS\)\s*:\s*0u\s*;", "t_inside"),
            (r"last_start\s*=\s*total\s*>=\s*A\.min_len\s*\?\s*total\s*-\s*A\.min_len\s*:\s*0\s*;", "last_start"),
            (r"last_block\s*=\s*total16\s*-\s*16\s*;", "last_block"),
            (r"blocks\s*=\s*\(ntiles\s*\+\s*15\)\s*/\s*16\s*;", "prefilter_grid()"),
            (r"\(kC\s*&\s*15\)\s*==\s*15", "the counts' batch of 16"),
            (r"\(kC\s*&\s*~15u\)\s*\+\s*lane", "the counts' epilogue")):
        assert re.search(pat, kern), f"kernels.hip no longer defines {what} as the plan restates it"
    # BIGV is forced by a switch that path_stats cannot show: read by this name, once, inside upload_tables()
    body = upload[upload.index("int upload_tables("):]
    assert re.search(r"static\s+const\s+char\s*\*big_env\s*=\s*std::getenv\(\"ACX_FILTER_BIG\"\)\s*;", body) and \
        re.search(r"D\.filter_big\s*=\s*big_env\s*\?\s*\(uint32_t\)std::atoi\(big_env\)", body), \
        "upload_tables() no longer reads ACX_FILTER_BIG"
    assert re.search(r"if\s*\(A\.filter_big\s*>=\s*2\)\s*\{\s*ACX_K1B_SH\(5,\s*2\)", kern), "launch_prefilter() no longer launches STAGED on filter_big >= 2"
    # the region switches, read per call; the first size of the hit regions
    assert re.search(r"no_sparse_env\s*=\s*std::getenv\(\"ACX_NO_BUCKET\"\)\s*!=\s*nullptr", attempts) and \
        re.search(r"const\s+bool\s+no_tiles_env\s*=\s*std::getenv\(\"ACX_NO_DENSE_TILES\"\)\s*!=\s*nullptr", attempts), \
        "the dense forms' switches are no longer read per call under these names"
    m = re.findall(r"ensure_hits\(x,\s*std::max<uint64_t>\(1u\s*<<\s*(\d+),\s*c\.len\s*/\s*(\d+)\)\)", attempts)
    assert len(m) == 2 and len(set(m)) == 1, "attempt_dense() / attempt_dense_tiles() no longer size the hit regions alike"
    out["HIT_RECORDS_MIN"], out["HIT_RECORDS_DIV"] = 1 << int(m[0][0]), int(m[0][1])
    assert len(re.findall(r"hit_cap\s*=\s*(?:c\.pre\s*\?\s*)?w\.hit_total\(\)\s*/\s*hit_grid", attempts)) == 2
    return out


C = source_constants()
TILE = 1 << C["TILE_BITS"]
ROW = TILE // C["K1B_ROWS"]
HIT_SLOTS, HB, HB_BIG, Q1CAP = C["HIT_SLOTS"], C["K1B_HB"], C["K1B_HB_BIG"], C["K1B_Q1CAP"]
BEHIND = C["STAGE_BEHIND"]  # a survivor's window, and what STAGED keeps of the bytes behind a row
GROUP = C["GROUP_TILES"] * TILE
WAVES = 16  # of a workgroup


def tile_bounds(lead: int, n: int, m: int) -> Dict[str, int]:
    """the kernel's four wave-uniform tile bounds for a stream of n bytes at pointer residue `lead`, shortest pattern m, and
    the index of the last tile -- from their definitions in the comment above them"""
    total = lead + n
    total16 = (total + 15) & ~15
    last_start = total - m if total >= m else 0
    return {"t_int_lo": 1 if lead else 0, "t_int_hi": last_start >> C["TILE_BITS"],
            "t_full": (total16 - 16) >> C["TILE_BITS"], "t_inside": ((total - 16) >> C["TILE_BITS"]) if total >= 16 else 0,
            "last": (total - 1) >> C["TILE_BITS"]}


def n_tiles(lead: int, n: int) -> int:
    return (lead + n + TILE - 1) // TILE


def scan_grid(tiles: int, cus: int) -> int:
    return max(1, min((tiles + WAVES - 1) // WAVES, cus))


def hit_region_records(n: int, tiles: int, cus: int) -> int:
    """records a wave's region holds on a handle's first dense call (attempt_dense / attempt_dense_tiles)"""
    return max(C["HIT_RECORDS_MIN"], n // C["HIT_RECORDS_DIV"]) // (WAVES * scan_grid(tiles, cus))


# ---------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------
def brute(pats, hay) -> np.ndarray:
    """every (pattern, start, end) with hay[start:end] == pattern, in the order of the oracle's overlapping Standard search:
    by end; at one end the longer pattern first, copies of a pattern by id"""
    h = bytes(hay)
    rows = []
    for i, p in enumerate(pats):
        p = bytes(p)
        x = h.find(p)
        while x >= 0:
            rows.append((x + len(p), -len(p), i, x))
            x = h.find(p, x + 1)
    rows.sort()
    return np.array([(i, x, e) for e, _, i, x in rows], dtype=np.uint64).reshape(-1, 3)


def brute_iter(pats, hay) -> np.ndarray:
    """the Standard search that does not overlap: the occurrence that ends first among those that begin at or behind the end
    of the one before (at one end the longest, then the lowest id)"""
    out, at = [], 0
    for i, x, e in brute(pats, hay).tolist():
        if x >= at:
            out.append((i, x, e))
            at = e
    return np.array(out, dtype=np.uint64).reshape(-1, 3)


# ---------------------------------------------------------------------------
# the ten scan forms and their pattern sets
# ---------------------------------------------------------------------------
def pattern_sets():
    """the five sets of test_level1_seams_at_every_length_and_residue: (patterns, filter_q, code points)"""
    q5 = list(dict.fromkeys(gen.gen_patterns(300, 5, 12, gen.AZ, 71)))
    q4 = list(dict.fromkeys(gen.gen_patterns(300, 4, 9, gen.AZ, 72)))
    q3 = list(dict.fromkeys(gen.gen_patterns(300, 3, 8, gen.AZ, 73)))
    sh = list(dict.fromkeys(gen.gen_patterns(250, 5, 10, gen.AZ, 74) + [b"q", b"zx", b"jq", b"kz"]))
    return {"q5": (q5, 5, False), "q4": (q4, 4, False), "q3": (q3, 3, False), "sh": (sh, 5, False),
            "cp": (q5, 5, True)}


def build_case(pats, n, lead, seed, tail_fits, multibyte):
    """(bytes in front of the pointer, the stream): `lead` bytes + n bytes of filler with patterns planted at
    the seams of the index space (index = lead + stream position)."""
    rng = np.random.default_rng(seed)
    buf = ALPHABET[rng.integers(0, len(ALPHABET), lead + n)].copy()
    used = np.zeros(lead + n, dtype=bool)
    by_len = sorted(pats, key=len)
    shortest, longest = by_len[0], by_len[-1]
    pick = lambda k: pats[(seed + 7 * k) % len(pats)]

    def plant(idx, p):  # at an index of the kernel's index space; only where it lies wholly inside the stream
        if idx >= lead and idx + len(p) <= lead + n:
            buf[idx:idx + len(p)] = np.frombuffer(p, dtype=np.uint8)
            used[idx:idx + len(p)] = True

    plant(16 * 3 + 15, pick(1))                 # starts at byte 15 of a lane
    plant(16 * 6, pick(2))                      # ... at byte 0 of the next kind of lane (16 of the one before)
    plant(1024 - len(longest), longest)         # bytes .. 1023 of a row: ends flush with the row
    plant(2048 - 3, pick(3))                    # lane 63 reads its look-ahead from the next row
    plant(2048 + 1008, shortest)                # the first byte of lane 63
    plant(4096 - 12, by_len[len(by_len) // 2][:12])  # inside the last 12 bytes of a tile (a prefix may match too)
    plant(4096 - 2, pick(4))                    # across the tile border
    plant(8192 - 1, pick(5))                    # ... and the next one
    # the end of the stream: a pattern flush with the last byte, or the shortest pattern one byte too late to fit
    tail = pick(6) if tail_fits else shortest[:-1]
    if len(tail) and len(tail) <= n:
        buf[lead + n - len(tail):] = np.frombuffer(tail, dtype=np.uint8)
        used[lead + n - len(tail):] = True
    # the lead bytes: a pattern that begins in front of the pointer and runs into the stream -- no match there
    if lead:
        p = pick(8)
        at = max(0, lead + 2 - len(p))
        m = min(len(p), lead + n - at)
        buf[at:at + m] = np.frombuffer(p[:m], dtype=np.uint8)
        used[at:at + m] = True
    if multibyte:  # str API: two-byte characters in the filler, so that code points and bytes part ways
        for at in range(lead + 3, lead + n - 1, 37):
            if not used[at] and not used[at + 1]:
                buf[at], buf[at + 1] = 0xC3, 0xA9
                used[at:at + 2] = True
    return buf[:lead].tobytes(), buf[lead:].tobytes()


def byte_to_code_point(hay: bytes) -> np.ndarray:
    a = np.frombuffer(hay, dtype=np.uint8)
    out = np.zeros(len(a) + 1, dtype=np.uint64)
    np.cumsum((a & 0xC0) != 0x80, out=out[1:])
    return out


def letters(seed: int, n: int) -> bytes:
    """n letters b .. z of a fixed sequence (a 31-bit LCG: the same bytes on every interpreter); never 'a'"""
    out, x = bytearray(), (seed * 2654435761 + 12345) & 0x7FFFFFFF
    for _ in range(n):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out.append(98 + (x >> 16) % 25)
    return bytes(out)


SHORTS = [b"a", b"ab", b"zx", b"kz"]  # SH: 1- and 2-byte patterns; "a" + "ab": two hits at one position
NUL_STEMS = ((b"nulone", 1), (b"nultwo", 2), (b"nuloct", 8))  # stem + that many NUL bytes is a pattern, the stem is none
MAX_FLUSH = 17
CUT_KEPT = 12  # bytes of the MAX_FLUSH-byte pattern that plant_seams() leaves in front of a tile's border plant


def nul_cut(q: int) -> bytes:
    """a pattern of q + 1 bytes whose last two are NUL: the q - 1 letters in front of them, flush with the end of a stream,
    begin BEHIND the last index a pattern can start at -- only the boundary mask keeps the zero fill from completing its key"""
    return letters(7700 + q, q - 1) + b"\0\0"


class Form(NamedTuple):
    name: str
    q: int
    bigv: int
    sh: bool
    set: str  # the pattern set


FORMS = tuple(Form(("q%d" % q if not b else "big%d" % b) + ("sh" if sh else ""), q, b, sh, "s%d%s" % (q, "sh" if sh else ""))
              for q, b in ((3, 0), (4, 0), (5, 0), (5, 1), (5, 2)) for sh in (False, True))
FORM = {f.name: f for f in FORMS}
SET_NAMES = tuple(dict.fromkeys(f.set for f in FORMS))
SINKS = ("slots", "slots_cp", "regions_tiles", "regions_radix")
SINK_ENV = {"slots": {}, "slots_cp": {}, "regions_tiles": {"ACX_NO_BUCKET": "1"},
            "regions_radix": {"ACX_NO_BUCKET": "1", "ACX_NO_DENSE_TILES": "1"}}


@functools.lru_cache(maxsize=None)
def patterns(set_name: str) -> Tuple[bytes, ...]:
    """today's recipe per Q (SH: + the short ones), a ladder with one pattern of every length Q .. 17, the NUL tails"""
    q, sh = int(set_name[1]), set_name.endswith("sh")
    hi = {5: 12, 4: 9, 3: 8}[q]
    base = gen.gen_patterns(250 if sh else 300, q, hi if not sh or q != 5 else 10, gen.AZ, {5: 71, 4: 72, 3: 73}[q] + (3 if sh else 0))
    ladder = [letters(1000 * q + L + (500 if sh else 0), L) for L in range(q, MAX_FLUSH + 1)]
    nul = [stem + b"\0" * k for stem, k in NUL_STEMS] + [nul_cut(q)]
    return tuple(dict.fromkeys(base + ladder + nul + (SHORTS if sh else [])))


def min_len(set_name: str) -> int:
    return int(set_name[1])  # k1b_min_len: the shortest pattern in the level-1 / level-2 tables


def pid_of(set_name: str, p: bytes) -> int:
    return patterns(set_name).index(p)


def ladder_pid(set_name: str, L: int) -> int:
    """the lowest id among the patterns of L bytes (the one an occurrence is reported under: all patterns differ)"""
    sh = set_name.endswith("sh")
    if L <= 2:
        return pid_of(set_name, SHORTS[L - 1])
    return pid_of(set_name, letters(1000 * min_len(set_name) + L + (500 if sh else 0), L))


def flush_lengths(set_name: str) -> List[int]:
    return ([1, 2] if set_name.endswith("sh") else []) + list(range(min_len(set_name), MAX_FLUSH + 1))


@functools.lru_cache(maxsize=None)
def oracle(set_name: str, mk: int) -> Oracle:
    return Oracle(list(patterns(set_name)), mk, KIND_DFA)


# ---------------------------------------------------------------------------
# haystacks
# ---------------------------------------------------------------------------
class Mark(NamedTuple):
    cls: str     # the class the plant is there for
    pid: int
    start: int   # stream position
    hit: bool    # True: an occurrence of pid begins here; False: none may be reported here


class Case(NamedTuple):
    name: str
    group: str   # position | sweep | burst
    front: bytes  # the bytes in front of the pointer (len = the pointer's residue)
    hay: bytes
    marks: Tuple[Mark, ...]

    @property
    def lead(self) -> int:
        return len(self.front)


class Builder:
    def __init__(self, set_name: str, total: int, lead: int, filler: str, seed: int):
        self.set, self.pats, self.lead, self.total = set_name, patterns(set_name), lead, total
        if filler == "clean":
            self.buf = np.full(total, CLEAN, dtype=np.uint8)
        else:
            self.buf = ALPHABET[np.random.default_rng(seed).integers(0, len(ALPHABET), total)].copy()
        self.used = np.zeros(total, dtype=bool)
        self.marks: List[Mark] = []
        self.seed = seed
        by_len = sorted(range(len(self.pats)), key=lambda i: (len(self.pats[i]), i))
        # (the pool the plants are drawn from: no NUL tail, and nothing a short pattern occurs in -- one match a plant)
        long_ = [i for i in by_len if len(self.pats[i]) >= 3 and b"\0" not in self.pats[i] and not any(x in self.pats[i] for x in SHORTS)]
        self.shortest, self.longest = long_[0], long_[-1]
        self.pool = long_

    def pick(self, k: int) -> int:
        return self.pool[(self.seed + 7 * k) % len(self.pool)]

    def plant(self, idx: int, pid: int, cls: str, data: Optional[bytes] = None, hit: bool = True, touch: bool = False) -> bool:
        """pattern pid (or `data`, a part of it) at INDEX idx, where it lies wholly inside the stream on untouched bytes
        (touch: a plant may lie directly in front of it or behind it)"""
        d = self.pats[pid] if data is None else data
        if idx < self.lead or idx + len(d) > self.total or self.used[max(idx - (0 if touch else 1), 0):idx + len(d) + (0 if touch else 1)].any():
            return False
        self.buf[idx:idx + len(d)] = np.frombuffer(d, dtype=np.uint8)
        self.used[idx:idx + len(d)] = True
        self.marks.append(Mark(cls, pid, idx - self.lead, hit))
        return True

    def case(self, name: str, group: str = "position") -> Case:
        # two-byte characters in the untouched filler, so that code points and bytes part ways (no pattern holds their bytes)
        for at in range(self.lead + 3, self.total - 2, 37):
            if not self.used[at - 1:at + 3].any():
                self.buf[at], self.buf[at + 1] = 0xC3, 0xA9
        return Case(name, group, self.buf[:self.lead].tobytes(), self.buf[self.lead:].tobytes(), tuple(self.marks))


def plant_seams(b: Builder, t: int, tag: str = ""):
    """what build_case() of the first seam test plants, around tile t"""
    o = t * TILE
    border = lambda x: "groupcross" if x % GROUP == 0 else "wgcross" if x % (WAVES * TILE) == 0 else "tilecross"
    b.plant(o + 16 * 3 + 15, b.pick(1), "lane15" + tag)                      # starts at byte 15 of a lane
    b.plant(o + 16 * 6, b.pick(2), "lane0" + tag)                            # ... at byte 0
    b.plant(o + ROW - len(b.pats[b.longest]), b.longest, "rowflush" + tag)   # ends flush with the row
    b.plant(o + 2 * ROW - 3, b.pick(3), "rowend" + tag)                      # lane 63 reads its look-ahead from the next row
    b.plant(o + 3 * ROW - 2, b.pick(7), "rowcross" + tag)                    # ... whatever the pattern's length
    b.plant(o + 2 * ROW + ROW - 16, b.shortest, "lane63" + tag)              # the first byte of lane 63
    b.plant(o + TILE - 2, b.pick(4), border(o + TILE) + tag)                 # across the tile border
    # the first CUT_KEPT bytes of a longer pattern in the tile's last bytes, the border plant directly behind them (as
    # build_case() leaves them: its border plant overwrites the cut's end): a level-1 survivor and a prefix hit whose
    # pattern would end in the next tile -- the post stage must reject it across the border
    cut = ladder_pid(b.set, MAX_FLUSH)
    b.plant(o + TILE - 2 - CUT_KEPT, cut, "cutprefix" + tag, data=b.pats[cut][:CUT_KEPT], hit=False, touch=True)
    b.plant(o + 2 * TILE - 1, b.pick(5), border(o + 2 * TILE) + tag)         # ... and the next one
    if o:
        b.plant(o - 1, b.pick(6), border(o) + tag)                           # ... and the one in front


def plant_stage(b: Builder, t: int):
    """a survivor at byte ROW - k of each of the four rows of tile t + k - 1, k = 1 .. BEHIND: its window of BEHIND bytes ends
    at, or runs into, the BEHIND bytes behind the staged row (row 3: the next tile's first bytes, another wave's tile)"""
    for k in range(1, BEHIND + 1):
        for r in range(C["K1B_ROWS"]):
            assert b.plant((t + k - 1) * TILE + r * ROW + ROW - k, b.pick(10 * r + k), "stage%d" % k)


def burst_positions(n: int) -> List[int]:
    """n tile offsets in n different lanes (one survivor a lane: ONE compaction round, one batch), the rows taking turns"""
    return [(i % C["K1B_ROWS"]) * ROW + i * 16 + 3 for i in range(n)]


@functools.lru_cache(maxsize=None)
def position_cases(set_name: str) -> Tuple[Case, ...]:
    m = min_len(set_name)
    out: List[Case] = []
    # -- the seams of the first test, around tiles owned by other waves and (16, 17) by the second workgroup
    for t in (0, 1, 2, 15, 16, 17):
        for lead in (0, 1, 15):
            for filler in ("clean", "az"):
                if filler == "az" and not (lead in (0, 15) and t in (0, 16)):
                    continue
                b = Builder(set_name, lead + (t + 2) * TILE + 21, lead, filler, 100 * t + lead)
                plant_seams(b, t)
                if lead:  # a pattern that begins in front of the pointer and runs into the stream: no match there
                    p = b.pick(8)
                    at = max(0, lead + 2 - len(b.pats[p]))
                    d = b.pats[p][:lead + 2 - at] if at == 0 else b.pats[p]
                    b.buf[at:at + len(d)] = np.frombuffer(d, dtype=np.uint8)
                    b.used[at:at + len(d)] = True
                out.append(b.case(f"seams_t{t}_r{lead}_{filler}"))
    # -- across the border of a group of the post stage
    b = Builder(set_name, GROUP + TILE + 21, 0, "clean", 5)
    plant_seams(b, C["GROUP_TILES"] - 1)
    out.append(b.case("seams_group"))
    # -- totals 4096 k + d at four residues: the four tile bounds flip between the last tile and the one before
    for k in (1, 2, 16):
        for d in sorted({0, 1, 15, 16, 17, m - 1, m, m + 1, TILE - 1}):
            for lead in (0, 1, 8, 15):
                total = TILE * k + d
                b = Builder(set_name, total, lead, "clean", 31 * k + d + lead)
                b.plant(total - m, b.shortest, "last_start")                    # the last index a pattern can start at
                b.plant(total - 16 - len(b.pats[b.pick(1)]) + 3, b.pick(1), "ends_in_last16")
                b.plant(TILE * k - 2, b.pick(2), "tilecross")
                b.plant(TILE * (k - 1) + 16 * 9 + 15, b.pick(3), "lane15")
                if d >= 40:
                    b.plant(TILE * k + 3, b.pick(4), "tail_tile")
                out.append(b.case(f"total_k{k}_d{d}_r{lead}"))
    # -- the end of the stream: a pattern of every length flush with the last byte, and the same one byte short
    for L in flush_lengths(set_name):
        pid = ladder_pid(set_name, L)
        for short in (0, 1):
            lead = (3 * L) % 16
            total = lead + 200 + 7 * L + (TILE if L % 4 == 1 else 0)
            b = Builder(set_name, total, lead, "clean", L)
            if short and L > 1:
                b.plant(total - (L - 1), pid, "short%d" % L, data=b.pats[pid][:L - 1], hit=False)
            elif not short:
                b.plant(total - L, pid, "flush%d" % L)
            b.plant(lead + 40, b.pick(L), "body")
            out.append(b.case(f"end_L{L}_{'short' if short else 'flush'}"))
    # -- patterns that end in NUL bytes, the stream stops just in front of them: the zero fill must not complete them
    for stem, k in NUL_STEMS:
        for total in (300, TILE + len(stem)):
            b = Builder(set_name, total, 0, "clean", k)
            b.plant(total - len(stem), pid_of(set_name, stem + b"\0" * k), "nultail%d" % k, data=stem, hit=False)
            b.plant(60, pid_of(set_name, stem + b"\0" * k), "nulbody%d" % k)
            out.append(b.case(f"nul{k}_n{total}"))
    cut = nul_cut(m)
    for total in (300, 2 * TILE + 9, 2 * TILE + 2):
        b = Builder(set_name, total, 0, "clean", total)
        b.plant(total - (m - 1), pid_of(set_name, cut), "nulcut", data=cut[:m - 1], hit=False)
        b.plant(70, pid_of(set_name, cut), "nulcutbody")
        out.append(b.case(f"nulcut_n{total}"))
    # -- STAGED's row ends (planted for every form)
    b = Builder(set_name, (BEHIND + 2) * TILE + 100, 0, "clean", 9)
    plant_stage(b, 1)
    out.append(b.case("stage_rows"))
    for k in range(1, BEHIND + 1):  # ... at the stream's last row: the shortest pattern that still fits behind byte ROW - k
        Ls = [L for L in flush_lengths(set_name) if L <= k]
        if Ls:
            total = 2 * TILE + 3 * ROW
            b = Builder(set_name, total, 0, "clean", k)
            b.plant(total - k, ladder_pid(set_name, Ls[-1]), "stage_last%d" % k)
            out.append(b.case(f"stage_last_k{k}"))
    # -- more level-1 survivors than Q1 holds, in one row and in a tile's four rows together (back to back)
    L = len(patterns(set_name)[Builder(set_name, 16, 0, "clean", 0).shortest])
    b = Builder(set_name, 5 * TILE + 33, 7, "clean", 11)
    for i in range(Q1CAP + 9):
        b.plant(TILE + ROW + 5 + i * (L + 2), b.shortest, "q1row")
    for r in range(C["K1B_ROWS"]):
        for i in range(Q1CAP // 4 + 3):
            b.plant(3 * TILE + r * ROW + 11 + i * (L + 2), b.shortest, "q1tile")
    out.append(b.case("q1cap"))
    # -- bursts: one push of HB - 1, HB, HB + 1 and 64 hits (np <= HB, np = HB + 1 straight to HBM, a full batch)
    for n in (HB - 1, HB, HB + 1, 64):
        b = Builder(set_name, 4 * TILE + 50, 0, "clean", n)
        for i, off in enumerate(burst_positions(n)):
            b.plant(2 * TILE + off, b.shortest if L <= 8 else b.pick(i), "burst%d" % n)
        out.append(b.case(f"burst_{n}", "burst"))
    return tuple(out)


SWEEP_TILES = ("first_lead15", "interior", "last_partial", "group_last")
SWEEP_K = tuple(range(HIT_SLOTS - 4, HIT_SLOTS + 5))
PAIR_FIXED = 16  # the "ab" pairs of the pair sweep: 32 hits behind the k long ones


def sweep_case(set_name: str, where: str, k: int, pair: bool) -> Case:
    """P planted k times in one otherwise clean tile; pair: k - 2 * PAIR_FIXED times, and "ab" PAIR_FIXED times -- the side
    test's survivors are queued behind the tile's long ones, so the pair's two hits take slots k', k' + 1, k' + 2 ..."""
    lead, tiles, t, extra = {"first_lead15": (15, 2, 0, 77), "interior": (0, 4, 2, 0), "last_partial": (0, 4, 3, 1900 - TILE),
                             "group_last": (0, C["GROUP_TILES"] + 1, C["GROUP_TILES"] - 1, 123 - TILE)}[where]
    b = Builder(set_name, tiles * TILE + extra, lead, "clean", k)
    base = t * TILE + (lead + 1 if t == 0 else 5)
    n_long = k - 2 * PAIR_FIXED if pair else k
    for i in range(n_long):
        assert b.plant(base + 24 * i, b.shortest, "sweep")
    if pair:
        for i in range(PAIR_FIXED):
            assert b.plant(base + 24 * n_long + 4 * i, pid_of(set_name, b"ab"), "pair")
    if where == "last_partial":  # ... and no hit behind the last start: the mask's upper clamp (nul_cut)
        m = min_len(set_name)
        assert b.plant(b.total - (m - 1), pid_of(set_name, nul_cut(m)), "nulcut", data=nul_cut(m)[:m - 1], hit=False)
    return b.case(f"sweep_{where}_{'pair_' if pair else ''}k{k}", "sweep")


def region_set() -> Tuple[bytes, ...]:
    return tuple(patterns("s5")) + (b"a", b"aa")


def region_cases(cus: int) -> List[Tuple[str, bytes, int]]:
    """(name, one tile's stream, prefix hits): runs of 'a' under "a" + "aa" -- a run of r bytes is 2 r - 1 hits of ONE wave --
    sized to the region's records minus one, the records, one more, and the whole tile"""
    cap = hit_region_records(TILE, 1, cus)
    out = []
    for name, hits in (("below", cap - 1), ("exact", cap), ("above", cap + 1), ("tile", 2 * (TILE - 16) - 1)):
        r, lone = (hits + 1) // 2, hits % 2 == 0  # an even number: a lone 'a' more
        buf = np.full(TILE - 5, CLEAN, dtype=np.uint8)
        buf[3:3 + r] = ord("a")
        if lone:
            buf[3 + r + 1] = ord("a")
        assert 3 + r + 2 <= len(buf)
        out.append((name, buf.tobytes(), 2 * r - 1 + (1 if lone else 0)))
    return out


# ---------------------------------------------------------------------------
# wave turns
# ---------------------------------------------------------------------------
def turn_tiles(cus: int) -> Dict[str, int]:
    w = WAVES * cus
    return {"w-1": w - 1, "w": w, "w+1": w + 1, "w+2": w + 2, "counts": 16 * w + w // 2 + 1}


def turn_hay(set_name: str, tiles: int, cus: int, bursts: bool = False, multibyte: bool = False) -> np.ndarray:
    """`tiles` tiles of the clean filler, the last one partial: one plant per tile at an offset that walks through the tile,
    one across every 16th tile border.  bursts: two consecutive batches of ONE wave (its tiles t and t + 16 * CUs) whose
    sizes sum to HB (tiles 0 and W) and to HB + 1 (tiles 1 and W + 1)"""
    pats = patterns(set_name)
    pool = [i for i, p in enumerate(pats) if 3 <= len(p) <= 12 and b"\0" not in p][:64]
    n = tiles * TILE - 100 if bursts else (tiles - 1) * TILE + 1234
    hay = np.full(n, CLEAN, dtype=np.uint8)
    t = np.arange(tiles, dtype=np.int64)
    off = 64 + (t * 37) % (TILE - 160)
    pos = t * TILE + off
    pos = pos[pos + 16 <= n]
    w = WAVES * cus
    skip = {0, 1, w, w + 1} if bursts else set()
    for j, pid in enumerate(pool):
        p = np.frombuffer(pats[pid], dtype=np.uint8)
        at = pos[j::len(pool)]
        at = at[~np.isin(at // TILE, list(skip))] if skip else at
        for x in range(len(p)):
            hay[at + x] = p[x]
    for i, bd in enumerate(range(16 * TILE, n - 16, 16 * TILE)):
        p = pats[pool[i % len(pool)]]
        s = bd - 1 - i % (len(p) - 1)
        hay[s:s + len(p)] = np.frombuffer(p, dtype=np.uint8)
    if bursts:
        assert tiles >= w + 2
        short = min((pats[i] for i in pool), key=len)
        for tile, cnt in ((0, HB // 2), (w, HB - HB // 2), (1, HB // 2), (w + 1, HB + 1 - HB // 2)):
            for o in burst_positions(cnt):
                hay[tile * TILE + 32 + o:tile * TILE + 32 + o + len(short)] = np.frombuffer(short, dtype=np.uint8)
    if multibyte:  # two-byte characters in the filler, so that code points and bytes part ways
        at = np.arange(7, n - 2, 4099)
        at = at[(hay[at] == CLEAN) & (hay[at + 1] == CLEAN)]
        hay[at], hay[at + 1] = 0xC3, 0xA9
    return hay


def code_points_at(hay: np.ndarray, x: np.ndarray) -> np.ndarray:
    """code points in front of the byte offsets x: offsets minus the continuation bytes in front of them"""
    cont = np.flatnonzero((hay & 0xC0) == 0x80)
    return (x.astype(np.int64) - np.searchsorted(cont, x.astype(np.int64), side="left")).astype(np.uint64)


def count_batches(tiles: int, cus: int) -> Dict[str, int]:
    """how the tile counts of a scan leave its waves: waves that store at least one full batch of 16, waves whose epilogue
    stores behind a full batch (kC > 16 with a remainder), the remainders that occur"""
    nw = WAVES * scan_grid(tiles, cus)
    per = [len(range(wv, tiles, nw)) for wv in range(nw)]
    return {"full": sum(1 for k in per if k >= 16), "epilogue_behind_batch": sum(1 for k in per if k > 16 and k % 16),
            "remainders": sorted({k % 16 for k in per}), "max": max(per)}


# ---------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------
def expected(set_name: str, hay, mk: int, ov: bool) -> np.ndarray:
    return oracle(set_name, mk).find_raw(np.frombuffer(hay, dtype=np.uint8) if isinstance(hay, bytes) else hay,
                                         overlapping=ov).astype(np.uint64)


def leg_calls(set_name: str, sink: str) -> int:
    """device calls a (form, sink) leg makes on the position classes"""
    return len(KINDS) * len(position_cases(set_name))


def digest() -> str:
    h = hashlib.sha256()
    for s in SET_NAMES:
        h.update(b"\0".join(patterns(s)))
        for c in position_cases(s):
            h.update(c.name.encode() + c.front + c.hay + repr(c.marks).encode())
        for where in SWEEP_TILES:
            for k in SWEEP_K:
                for pair in ((False, True) if s.endswith("sh") else (False,)):
                    c = sweep_case(s, where, k, pair)
                    h.update(c.name.encode() + c.front + c.hay)
    for name, hay, hits in region_cases(CPU_CUS):
        h.update(name.encode() + hay + str(hits).encode())
    h.update(turn_hay("s5", turn_tiles(4)["w+2"], 4, bursts=True, multibyte=True).tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------------
# the device side (imports the library when called; the BIGV forms run it in a child process: ACX_FILTER_BIG is read once)
# ---------------------------------------------------------------------------
def cols(a):
    return np.stack([a["pattern"], a["start"], a["end"]], 1) if len(a) else np.zeros((0, 3), np.uint64)


class Device:
    """a form's automatons (one per match kind) and the calls of a leg against the oracle"""

    def __init__(self, form: Form, pats=None, set_name=None):
        from ahocorasick_rs_amd import capi
        self.capi, self.form = capi, form
        self.set = set_name or form.set
        self.pats = list(pats if pats is not None else patterns(self.set))
        self.autos = {}
        self.fails: List[str] = []

    def auto(self, mk: int):
        if mk not in self.autos:
            a = self.capi.Automaton(self.pats, mk, kernel=self.capi.KERNEL_PREFILTER)
            assert a.info.kernel == self.capi.KERNEL_PREFILTER and a.info.filter_q == self.form.q, (a.info.kernel, a.info.filter_q)
            self.autos[mk] = a
        return self.autos[mk]

    def reset(self):
        for a in self.autos.values():
            a.path_stats(reset=True)

    def stats(self) -> Dict[str, int]:
        out: Dict[str, int] = {}
        for a in self.autos.values():
            for k, v in a.path_stats(reset=True).items():
                out[k] = out.get(k, 0) + v
        return out

    def close(self):
        for a in self.autos.values():
            a.close()
        self.autos = {}

    def run(self, name: str, front: bytes, hay, kinds, codepoints: bool, want_of) -> int:
        """the stream at pointer residue len(front) under every kind of `kinds`; want_of(mk, ov) -> the expected rows"""
        capi = self.capi
        lead = len(front)
        arr = np.frombuffer(hay, dtype=np.uint8) if isinstance(hay, bytes) else hay
        dev = capi.DeviceBuffer(lead + len(arr) + 16)
        # (16 zero bytes behind the stream: what the kernel's last, clamped loads see beyond the end is defined)
        dev.upload(np.concatenate([np.frombuffer(front, dtype=np.uint8), arr, np.zeros(16, dtype=np.uint8)]))
        assert dev.ptr % 16 == 0
        for mk, ov in kinds:
            want = want_of(mk, ov)
            r = self.auto(mk).find_device(dev.ptr + lead, len(arr), overlapping=ov, codepoints=codepoints)
            got = cols(r.matches())
            r.free()
            if not np.array_equal(got, want) and len(self.fails) < 5:
                self.fails.append(f"{name} kind {mk} overlapping {ov} residue {lead} n {len(arr)}: {len(got)} rows against {len(want)}")
        dev.free()
        return len(kinds)


_want_cache: Dict[tuple, np.ndarray] = {}


def case_expected(set_name: str, c: Case, mk: int, ov: bool, codepoints: bool = False) -> np.ndarray:
    key = (set_name, c.name, mk, ov, codepoints)
    if key not in _want_cache:
        w = expected(set_name, c.hay, mk, ov)
        if codepoints and len(w):
            a = np.frombuffer(c.hay, dtype=np.uint8)
            w = np.stack([w[:, 0], code_points_at(a, w[:, 1]), code_points_at(a, w[:, 2])], 1)
        _want_cache[key] = w
    return _want_cache[key]


def pipeline_calls(st) -> int:
    return st["sparse"] + st["hot_calls"] + st["dense_tiles"] + st["dense_radix"]


def sink_proof(sink: str, st: Dict[str, int], calls: int) -> Optional[str]:
    """what path_stats must say of a leg's calls (None: it does)"""
    if st["k0"] != 0 or pipeline_calls(st) != calls:
        return f"k0 or a call outside the scan's pipeline: {st} for {calls} calls"
    if sink in ("slots", "slots_cp") and st["sparse"] + st["hot_calls"] != calls:
        return f"not every call left through the hit slots: {st}"
    # (ACX_NO_BUCKET sends EVERY call to attempt_dense(): none through the hit slots, all by the form asked for)
    if sink == "regions_tiles" and not (st["sparse"] + st["hot_calls"] == 0 and st["dense_tiles"] == calls and st["dense_radix"] == 0):
        return f"not every call by the tile-ordered dense form: {st}"
    if sink == "regions_radix" and not (st["sparse"] + st["hot_calls"] == 0 and st["dense_radix"] == calls and st["dense_tiles"] == 0):
        return f"not every call by the radix form: {st}"
    return None


def with_env(env: Dict[str, str]):
    class _E:
        def __enter__(self):
            self.old = {k: os.environ.get(k) for k in env}
            os.environ.update(env)

        def __exit__(self, *a):
            for k, v in self.old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    return _E()


def run_leg(form: Form, sink: str) -> Dict:
    """the position classes of one (form, sink): every case under all four kinds, element-wise against the oracle.  The
    cases on the clean filler first, the a-z filler behind them (a 1-byte pattern overfills its tiles' slots: the overflow
    lists and the hot pipeline take those calls, still through the hit slots), each part with the sink's proof."""
    d = Device(form)
    cp = sink == "slots_cp"
    out = {"form": form.name, "sink": sink, "calls": 0}
    with with_env(SINK_ENV[sink]):
        for part in ("clean", "az"):
            for mk, _ in KINDS:
                d.auto(mk)
            d.reset()
            calls = 0
            for c in position_cases(form.set):
                if c.name.endswith("_az") != (part == "az"):
                    continue
                # CP needs pointer residue 0; at the others the plain kernel runs beside k_count_leads: that leg stays in
                calls += d.run(c.name, c.front, c.hay, KINDS, cp, lambda mk, ov, c=c: case_expected(form.set, c, mk, ov, cp))
            st = d.stats()
            out["calls"] += calls
            out["stats_" + part] = st
            why = sink_proof(sink, st, calls)
            if why:
                d.fails.append(why)
    d.close()
    out["fails"] = d.fails
    return out


def run_sweep(form: Form, where: str, pair: bool) -> Dict:
    """HIT_SLOTS - 4 .. + 4 hits in one tile on the hit-slot sink: equal to the oracle at every k, and overflow_hits --
    the hits beyond the tile's slots, as the hot pipeline counts them -- 0 first, then 1, 2, ... one per added plant"""
    d = Device(form)
    ovf, hot = [], []
    kinds = [(0, False), (0, True)]
    for k in SWEEP_K:
        c = sweep_case(form.set, where, k, pair)
        d.auto(0)
        d.reset()
        d.run(c.name, c.front, c.hay, kinds, False, lambda mk, ov, c=c: expected(form.set, c.hay, mk, ov))
        st = d.stats()
        if st["k0"] or st["sparse"] + st["hot_calls"] != len(kinds):
            d.fails.append(f"{c.name}: not through the hit slots: {st}")
        ovf.append(st["overflow_hits"] // len(kinds) if st["overflow_hits"] % len(kinds) == 0 else -1)
        hot.append(st["hot_groups"])
    d.close()
    why = staircase(ovf, hot)
    if why:
        d.fails.append(why)
    return {"form": form.name, "where": where, "pair": pair, "overflow_hits": ovf, "hot_groups": hot, "fails": d.fails}


def staircase(ovf: List[int], hot: List[int]) -> Optional[str]:
    """overflow_hits over the sweep: 0 up to HIT_SLOTS plants, then 1 (the 65-hit tile; the step before it is the 64-hit
    tile), 2, ... -- one more per added plant.  Exactly max(0, k - HIT_SLOTS): on the clean filler level 1 has no survivor
    but the plants, and level 2 is exact, so a plant is ONE prefix hit (measured on all ten forms); a hit more -- a position
    behind the last start that the boundary mask let through -- moves the crossing and fails here.  The hot pipeline takes
    the overfull group from the first overflow on."""
    if ovf != [max(0, k - HIT_SLOTS) for k in SWEEP_K]:
        return f"overflow_hits {ovf}: not max(0, k - {HIT_SLOTS}) for k = {SWEEP_K[0]} .. {SWEEP_K[-1]}"
    first = next(i for i, v in enumerate(ovf) if v)
    if any(h < 1 for h in hot[first:]):
        return f"hot_groups {hot}: the overfull group did not go to the hot pipeline"
    return None


def run_turn_bursts(form: Form, cus: int) -> Dict:
    """two consecutive batches of one wave (W + 2 tiles) that sum to HB and to HB + 1, on the hit-slot sink"""
    d = Device(form)
    hay = turn_hay(form.set, turn_tiles(cus)["w+2"], cus, bursts=True)
    d.auto(0)
    d.reset()
    d.run("turn_bursts", b"", hay, [(0, False)], False, lambda mk, ov: expected(form.set, hay, mk, ov))
    st = d.stats()
    if st["k0"] or st["sparse"] + st["hot_calls"] != 1:
        d.fails.append(f"turn_bursts: not through the hit slots: {st}")
    d.close()
    return {"form": form.name, "turn_bursts": True, "fails": d.fails}


def child_main(bigv: int, cus: int):
    """every (SH, sink) leg of one BIGV, its sweeps and its two-batch bursts: one JSON line per leg"""
    assert os.environ.get("ACX_FILTER_BIG") == str(bigv)
    for f in FORMS:
        if f.bigv != bigv:
            continue
        for sink in SINKS:
            print("LEG " + json.dumps(run_leg(f, sink)), flush=True)
        for where in SWEEP_TILES:
            for pair in ((False, True) if f.sh else (False,)):
                print("SWEEP " + json.dumps(run_sweep(f, where, pair)), flush=True)
        print("TURN " + json.dumps(run_turn_bursts(f, cus)), flush=True)
    print("DONE", flush=True)


if __name__ == "__main__":
    child_main(int(sys.argv[1]), int(sys.argv[2]))
