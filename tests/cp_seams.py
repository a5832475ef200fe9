"""The code-point conversion at its seams: the reference, the constants, the haystacks and the plan that
tests/test_cp_seams_cpu.py checks on the CPU and tests/test_gpu_cp_seams.py runs on the device.  Needs no GPU.

The reference is code_points(): cp[x] = bytes b of hay[:x] with (b & 0xC0) != 0x80, a uint64 cumsum.  Expected rows are
the oracle's byte rows (tests/oracle_lib.py, pinned by tests/test_oracle_golden.py) mapped through that table; nothing
expected comes from the library.  The sizes are derived from the constants of the kernels' sources (source_constants()).

Haystacks are valid UTF-8 written from fillers of ONE width -- 1 (letters i .. y, which no pattern holds), 2 (é), 3 (☃),
4 (🤦) -- or a mixed filler; a pattern is planted at an exact byte offset whatever the filler's width: the character the
offset cuts is replaced by one to three ASCII pad bytes ('z') -- the whole character in front where none is cut, so that it
cannot begin another pattern together with the plant's first letters --, and so is the one the plant's end cuts.  Patterns hold the
letters a .. h and the three characters; none of them holds a stretch of five bytes that a filler holds (the prefix table
of the prefilter is keyed on the first bytes of a pattern: a key that the filler holds would be a hit at every character,
and the call would leave the sparse path the tests want to see)."""
from __future__ import annotations

import functools
import os
import re
from typing import Dict, List, NamedTuple, Tuple

import numpy as np

from oracle_lib import KIND_DFA, Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ahocorasick_rs_amd", "csrc")
BLOCK, CHUNK = 1024, 16  # code_point_of(): blk = x >> 10, chunk = (x & 1023) >> 4 (checked by source_constants)
PAD = ord("z")


# ---------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------
def code_points(hay: np.ndarray) -> np.ndarray:
    """cp[x] = lead (non-continuation) bytes in hay[:x], x = 0 .. len"""
    hay = np.asarray(hay, dtype=np.uint8)
    out = np.zeros(len(hay) + 1, dtype=np.uint64)
    np.cumsum((hay & 0xC0) != 0x80, dtype=np.uint64, out=out[1:])
    return out


def map_rows(rows: np.ndarray, cp: np.ndarray) -> np.ndarray:
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 3)
    return np.stack([rows[:, 0], cp[rows[:, 1]], cp[rows[:, 2]]], 1).astype(np.uint64)


# ---------------------------------------------------------------------------
# the constants of the sources
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def source_constants() -> Dict[str, int]:
    kern = open(os.path.join(CSRC, "kernels.hip")).read()
    types = open(os.path.join(CSRC, "device_types.hpp")).read()  # (kernels.hip includes it: the tile geometry)
    out = {}

    def plain(name, src, where):
        m = re.search(r"\b%s\s*=\s*(\d+)\s*[,;]" % name, src)
        assert m, f"{name} is no longer a plain constant of {where}"
        out[name] = int(m.group(1))

    for n in ("BP_BLOCKS", "BP_THREADS", "CP_BITS", "CP_UNKNOWN"):
        plain(n, kern, "kernels.hip")
    plain("TILE_BITS", types, "device_types.hpp")
    for n in ("DT_GROUP", "GROUP_TILES"):  # constexpr uint32_t DT_GROUP = ACX_DT_GROUP;  #define ACX_DT_GROUP 4
        assert re.search(r"\b%s\s*=\s*ACX_%s\s*;" % (n, n), types), f"{n} is no longer ACX_{n} in device_types.hpp"
        m = re.search(r"#define\s+ACX_%s\s+(\d+)\s*$" % n, types, re.M)
        assert m, f"ACX_{n} is no longer a plain constant of device_types.hpp"
        out[n] = int(m.group(1))
    # the block and the chunk of code_point_of() are written as shifts
    assert re.search(r"blk\s*=\s*x\s*>>\s*10\s*;", kern) and re.search(r"\(x\s*&\s*1023\)\s*>>\s*4\s*;", kern), \
        "code_point_of() no longer works on 1 KiB blocks of 16-byte chunks"
    return out


class Sizes(NamedTuple):
    tile: int      # bytes of a tile of k_tile_main
    dgroup: int    # DT_GROUP tiles: a group of the dense (and the hot) pipeline
    group: int     # GROUP_TILES tiles: a group of k_tile_main / k_tile_write
    wg: int        # bytes whose blocks ONE workgroup of k_block_partials / k_block_prefix takes
    big: int       # the largest haystack


def sizes() -> Sizes:
    c = source_constants()
    tile = 1 << c["TILE_BITS"]
    wg = c["BP_BLOCKS"] * BLOCK
    return Sizes(tile, c["DT_GROUP"] * tile, c["GROUP_TILES"] * tile, wg, 2 * wg + 5 * BLOCK + 321)


# ---------------------------------------------------------------------------
# patterns
# ---------------------------------------------------------------------------
PATTERNS: List[str] = [
    # all ASCII; nested, so that the three match kinds differ
    "abcde", "abcdefgh", "bcdef", "cdefgha", "habcd", "fghab", "gabcdefghabc", "defgh", "hgfed", "fedcba",
    # a pair of copies
    "a☃bcd", "a☃bcd",
    # begin with a 4-byte character
    "🤦abc", "🤦a☃", "🤦héb", "🤦bcdefg", "🤦☃🤦☃a", "🤦éa",
    # end with one
    "abc🤦", "é☃a🤦", "cd🤦", "hgf🤦",
    # both
    "🤦ab🤦",
    # begin with a 2- or 3-byte character
    "éabcd", "éa☃b", "☃abc", "☃éa🤦", "☃cd", "éh☃",
    # characters of every width inside; nested
    "a🤦b☃c", "ab☃éc", "b☃c", "b☃cd", "ab☃c", "hé☃", "c🤦d", "c🤦dé", "d☃é🤦e", "gé🤦", "fé☃éf",
    # 17 - 24 bytes: the long-tail verification; the code points are not the bytes
    "ab☃🤦é☃cd🤦", "🤦a☃b🤦c☃d",
    # 36 bytes in 12 characters: a span that lead_bytes_between() counts in two rounds
    "🤦a🤦☃🤦b🤦☃🤦c🤦☃",
]
PATS_B: List[bytes] = [p.encode("utf-8") for p in PATTERNS]
PLEN = [len(p) for p in PATS_B]
LONG_TAIL = [i for i, n in enumerate(PLEN) if 17 <= n <= 24]
SPAN36 = PLEN.index(36)
ASCII_IDS = [i for i, p in enumerate(PATTERNS) if p.isascii()]
FOUR_FIRST = [i for i, p in enumerate(PATTERNS) if p[0] == "🤦" and i != SPAN36]
FOUR_LAST = [i for i, p in enumerate(PATTERNS) if p[-1] == "🤦"]
SHORT_IDS = [i for i, n in enumerate(PLEN) if n <= 8]
KEY_BYTES = min(PLEN)  # what the prefix table is keyed on is at least this long (automaton.cpp: Q2 = min(8, shortest))

UNITS: Dict[str, bytes] = {
    "w1": b"ijklmnopqrstuvwxy",  # 17 letters: every letter meets every residue mod 16
    "w2": "é".encode(),
    "w3": "☃".encode(),
    "w4": "🤦".encode(),
    "mixed": "kémn☃o🤦".encode(),  # 13 bytes, 7 characters
}
WIDTHS = list(UNITS)


# ---------------------------------------------------------------------------
# the haystack builder
# ---------------------------------------------------------------------------
def _cont(b) -> bool:
    return (int(b) & 0xC0) == 0x80


def _seal_tail(h: np.ndarray) -> None:
    """the last character, when the end cuts it, becomes pad bytes"""
    n = len(h)
    if not n:
        return
    k = n - 1
    while k > 0 and _cont(h[k]):
        k -= 1
    b = int(h[k])
    width = 1 if b < 0x80 else 2 if b < 0xE0 else 3 if b < 0xF0 else 4
    if k + width > n or _cont(b):
        h[k:] = PAD


def fill(n: int, unit: bytes) -> np.ndarray:
    h = np.resize(np.frombuffer(unit, dtype=np.uint8), n).copy()
    _seal_tail(h)
    return h


def overwrite(h: np.ndarray, a: int, data) -> Tuple[int, int]:
    """h[a : a + len(data)] = data; the characters the two ends cut become pad bytes -> the bytes touched, [s, t)"""
    data = np.frombuffer(bytes(data), dtype=np.uint8)
    n, b = len(h), a + len(data)
    assert 0 <= a and b <= n
    s = a
    while s > 0 and s < n and _cont(h[s]):
        s -= 1
    assert a - s <= 3
    h[s:a] = PAD
    h[a:b] = data
    t = b
    while t < n and _cont(h[t]):
        h[t] = PAD
        t += 1
    assert t - b <= 3
    return s, t


def force_boundary(h: np.ndarray, b: int) -> None:
    """a character boundary at byte b: the character that lies across it becomes pad bytes"""
    if 0 < b < len(h) and _cont(h[b]):
        overwrite(h, b, b"")


def head(hay: np.ndarray, n: int) -> np.ndarray:
    """the first n bytes as a haystack of their own"""
    h = np.array(hay[:n], dtype=np.uint8)
    _seal_tail(h)
    return h


class Plant(NamedTuple):
    x: int
    pid: int
    tag: tuple  # what it is there for: ("res1", r) ("res4", r) ("blk", off) ("bound", name, B) ("tail",) ("any",)


class Case(NamedTuple):
    name: str
    width: str
    hay: np.ndarray
    plants: Tuple[Plant, ...]
    targets: str


class Builder:
    def __init__(self, n: int, width: str):
        self.n, self.width = n, width
        self.h = fill(n, UNITS[width])
        self.taken: List[Tuple[int, int]] = []
        self.plants: List[Plant] = []

    def region(self, a: int, length: int, unit: bytes) -> None:
        if a + length <= self.n:
            overwrite(self.h, a, fill(length, unit).tobytes())

    def free(self, lo: int, hi: int) -> bool:
        return all(hi + 1 <= s or t + 1 <= lo for s, t in self.taken)

    def plant(self, x: int, pid: int, tag: tuple) -> bool:
        p = PATS_B[pid]
        if x < 0 or x + len(p) > self.n or not self.free(x - 4, x + len(p) + 3):
            return False
        s, t = overwrite(self.h, x, p)
        if s == x and x > 0 and self.h[x - 1] >= 0x80:
            # a filler character right in front would begin another pattern with the plant's first letters ("🤦abc"):
            # the match would start there, not at x
            while _cont(self.h[s - 1]):
                s -= 1
            s -= 1
            self.h[s:x] = PAD
        self.taken.append((s, t))
        self.plants.append(Plant(x, pid, tag))
        return True

    def carried_if(self, x: int, pid: int) -> int:
        """lead bytes of x's 16-byte chunk at or behind x, were the pattern planted there"""
        lo, hi = max(0, x - 16), min(self.n, x + 64)
        loc = self.h[lo:hi].copy()
        overwrite(loc, x - lo, PATS_B[pid])
        return carried_at(loc, x - lo, base=lo)


def carried_at(h: np.ndarray, x: int, base: int = 0) -> int:
    """what k_tile_main packs beside an occurrence that starts at x: lead bytes in [x, the end of x's 16-byte chunk)"""
    end = min(len(h), ((x + base) | 15) + 1 - base)
    return int(np.count_nonzero((h[x:end] & 0xC0) != 0x80))


# layouts of the plants around a boundary B: (offset from B, what)
#   "s" a short pattern   "x4" one that begins with a 4-byte character (at -2: the boundary lies inside the character)
#   "xl" a long-tail pattern (17 - 24 bytes)   "x36" the 36-byte one
LAYOUTS = [
    [(-17, "s"), (-2, "x4"), (16, "s")],
    [(-16, "s"), (0, "s"), (17, "s")],
    [(-15, "s"), (-1, "xl")],
    [(-20, "x36")],
]
BLOCK_OFFSETS = [0, 1, 15, 16, 1007, 1008, 1023]  # x mod 1024: chunk 0 and chunk 63 of a block


def boundaries() -> Dict[str, List[int]]:
    """every kind of boundary and its instances, one layout each (by position in the list, modulo the layouts)"""
    z = sizes()
    return {
        "tile": [z.tile * k for k in (17, 19, 21, 23)],
        "dgroup": [z.dgroup * k for k in (7, 9, 10, 11)],
        "group": [z.group * k for k in (1, 2, 3, 5)],
        "wg1": [z.wg],
        "wg2": [2 * z.wg],
    }


def build_case(name: str, width: str, n: int, wg_layouts: Tuple[int, int], tail_pid: int, targets: str) -> Case:
    z = sizes()
    b = Builder(n, width)
    rot = [0]

    def nxt(ids):
        rot[0] += 1
        return ids[rot[0] % len(ids)]

    # the head: what the K0 cuts (1 008, 1 024, 1 025, 16 384 bytes) hold -- matches flush with and across those marks
    for x, ids in ((37, SHORT_IDS), (200, FOUR_FIRST), (463, LONG_TAIL), (700, [SPAN36]), (1500, FOUR_LAST), (4090, LONG_TAIL),
                   (9001, SHORT_IDS), (12345, FOUR_FIRST)):
        b.plant(x, nxt(ids), ("any",))
    for mark in (1008, 1024, 16384):
        pid = nxt(SHORT_IDS)
        b.plant(mark - PLEN[pid], pid, ("any",))
    b.plant(1020 + 32, nxt(SHORT_IDS), ("any",))
    # every residue mod 16 inside an all-ASCII stretch (carried 16 .. 1) and inside a 4-byte stretch (carried 1 .. 4)
    # (four plants to a tile: k_tile_main stages 24 occurrences per 4 KiB, nested ones included, before its group goes hot)
    a0, f0, step = 300 * BLOCK, 320 * BLOCK, 65 * CHUNK
    b.region(a0, 18 * step, UNITS["w1"])
    b.region(f0, 24 * step, UNITS["w4"])
    for r in range(16):
        b.plant(a0 + 16 + step * r + r, ASCII_IDS[r % len(ASCII_IDS)], ("res1", r))
    need = {1, 2, 3, 4}
    slot = 0
    for r in list(range(16)) + [12, 14, 10, 6, 2, 9, 5]:  # (a second visit where the first left a count out)
        x = f0 + 16 + step * slot + r
        if x + 64 > n or (slot >= 16 and not need):
            break
        got = {b.carried_if(x, pid): pid for pid in reversed(range(len(PATS_B)))}
        hit = [c for c in sorted(need) if c in got]
        if slot >= 16 and not hit:
            continue
        pid = got[hit[0]] if hit else FOUR_FIRST[r % len(FOUR_FIRST)]
        if b.plant(x, pid, ("res4", r)) and hit:
            need.discard(hit[0])
        slot += 1
    # chunk 0 and chunk 63 of a block
    for j, off in enumerate(BLOCK_OFFSETS):
        b.plant(48 * BLOCK + 2 * BLOCK * j + off, nxt(range(len(PATS_B))), ("blk", off))
    # both sides of every boundary, and across it
    for kind, inst in boundaries().items():
        for k, B in enumerate(inst):
            lay = LAYOUTS[wg_layouts[0] if kind == "wg1" else wg_layouts[1] if kind == "wg2" else k % len(LAYOUTS)]
            for off, what in lay:
                ids = {"s": SHORT_IDS, "x4": FOUR_FIRST, "xl": LONG_TAIL, "x36": [SPAN36]}[what]
                b.plant(B + off, nxt(ids), ("bound", kind, B))
            if kind in ("wg1", "wg2"):  # further starts in the first block of the second and the third workgroup
                for off in (517, 1007):
                    b.plant(B + off, nxt(range(len(PATS_B))), ("blk1", kind, off))
    # a match within the last 16 bytes
    b.plant(n - PLEN[tail_pid], tail_pid, ("tail",))
    # every pattern now and then
    for i, x in enumerate(range(17 * BLOCK + 5, n - 64, 23 * BLOCK + 37)):
        b.plant(x, i % len(PATS_B), ("any",))
    h = b.h
    h.setflags(write=False)
    return Case(name, width, h, tuple(b.plants), targets)


def sentinel_lengths() -> List[Tuple[int, int]]:
    """(blocks + 1, length): the entries of the prefix, its sentinel included, one short of a workgroup, a whole one, one
    more -- the sentinel alone in the second workgroup -- and two and one; lengths that are 0, 1 and 15 mod 16, 0 and 1
    mod 1024"""
    bp = source_constants()["BP_BLOCKS"]
    out = []
    for entries in (bp - 1, bp, bp + 1, 2 * bp + 1):
        nb = entries - 1
        out += [(entries, nb * BLOCK), (entries, (nb - 1) * BLOCK + 1), (entries, nb * BLOCK - 1)]
    return out


TAIL_IDS = [i for i, n in enumerate(PLEN) if n <= 16]


@functools.lru_cache(maxsize=None)
def plan() -> Tuple[Case, ...]:
    z = sizes()
    cases = []
    for w in WIDTHS:
        k = WIDTHS.index(w)
        cases.append(build_case(f"{w}-big", w, z.big, (0, 0), TAIL_IDS[k], "every class; three prefix workgroups"))
        cases.append(build_case(f"{w}-mid", w, z.wg + 2 * BLOCK + 7, (1, 1), TAIL_IDS[k + 5], "a start at the second workgroup's first byte"))
        cases.append(build_case(f"{w}-top", w, 2 * z.wg + BLOCK + 5, (2, 1), TAIL_IDS[k + 10], "a start at the third workgroup's first byte"))
        for j, (entries, n) in enumerate(sentinel_lengths()):
            cases.append(build_case(f"{w}-len{n}", w, n, (3, 3), TAIL_IDS[(3 * k + j) % len(TAIL_IDS)],
                                    f"{entries} prefix entries, the last one the sentinel; a match in the last 16 bytes"))
    return tuple(cases)


def case(name: str) -> Case:
    return next(c for c in plan() if c.name == name)


# ---------------------------------------------------------------------------
# expected rows
# ---------------------------------------------------------------------------
KINDS = [(0, False), (0, True), (1, False), (2, False)]  # (match kind, overlapping)
LL = (2, False)  # LeftmostLongest: cfg5's


@functools.lru_cache(maxsize=None)
def oracle(mk: int, extra: tuple = ()) -> Oracle:
    return Oracle(PATS_B + list(extra), mk, KIND_DFA)


def expected_of(hay: np.ndarray, mk: int, ov: bool, extra: tuple = ()) -> np.ndarray:
    """the oracle's rows of one haystack in code points"""
    hay = np.ascontiguousarray(hay)
    return map_rows(oracle(mk, extra).find_raw(hay, overlapping=ov), code_points(hay))


@functools.lru_cache(maxsize=None)
def byte_rows(name: str, mk: int, ov: bool) -> np.ndarray:
    r = oracle(mk).find_raw(np.ascontiguousarray(case(name).hay), overlapping=ov).astype(np.uint64)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def expected(name: str, mk: int, ov: bool) -> np.ndarray:
    r = map_rows(byte_rows(name, mk, ov), code_points(case(name).hay))
    r.setflags(write=False)
    return r


# ---------------------------------------------------------------------------
# batches, byte ranges, K0 cuts
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ragged_batch() -> Tuple[np.ndarray, Tuple[int, ...]]:
    """(bytes, offsets): boundaries at character boundaries that take every residue mod 16, some at k * 1024 and
    k * 1024 +- 1; empty haystacks in front, in the middle (two in a row) and at the end"""
    h = np.array(case("mixed-big").hay[:64 * BLOCK + 77])
    _seal_tail(h)
    cuts = sorted({2 * BLOCK * i + 100 + i for i in range(16)} | {BLOCK * k + d for k in (33, 35, 37) for d in (-1, 0, 1)}
                  | {41 * BLOCK, 48 * BLOCK + 1007, 48 * BLOCK + 1023})
    for c in cuts:
        force_boundary(h, c)
    for k, (a, b) in enumerate(zip([0] + cuts, cuts + [len(h)])):  # a match in every haystack that has the room, some at its first byte
        if b - a >= 40:
            overwrite(h, a + (0 if k % 3 == 0 else 5 + k % 7), PATS_B[(5 * k) % len(PATS_B)])
    mid = cuts[len(cuts) // 2]
    offs = [0, 0] + cuts[:len(cuts) // 2] + [mid, mid, mid] + cuts[len(cuts) // 2 + 1:] + [len(h), len(h)]
    h.setflags(write=False)
    return h, tuple(offs)


@functools.lru_cache(maxsize=None)
def uniform_batches() -> Tuple[Tuple[np.ndarray, int], ...]:
    """(bytes, uniform_len): 4-byte filler and a length that is a multiple of 4; 1 024"""
    out = []
    for ul in (4 * 251, BLOCK):
        n_hay = 60
        h = np.array(case("w4-big").hay[320 * BLOCK:320 * BLOCK + n_hay * ul])  # (the 4-byte stretch and its sixteen residues)
        for k in range(1, n_hay):
            force_boundary(h, k * ul)
        _seal_tail(h)
        h.setflags(write=False)
        out.append((h, ul))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def range_cases() -> Tuple[Tuple[str, np.ndarray, int], ...]:
    """(name, haystack, ACX_CHUNK_BYTES): every cut k * piece lies inside a character"""
    h4, h3 = case("w4-mid").hay, case("w3-mid").hay
    shifted = np.concatenate([np.array([PAD], dtype=np.uint8), h4])  # (characters at 1 mod 4: cuts at 2 and 0 are inside)
    return (("w4 piece 1 mod 4", h4, 349_529), ("w4 piece 3 mod 4", h4, 350_003), ("w4 piece 2 mod 4", shifted, 400_002),
            ("w3 piece 1 mod 3", h3, 400_000))


K0_CUTS = (1008, 1024, 1025, 16384)  # the poll's reach, wave 0's limit, one more, the largest K0 call
