"""verify_candidate() and the packed occurrence words at their field limits: the references, the constants, the pattern
sets, the haystacks and the plan that tests/test_verify_seams_cpu.py checks on the CPU and tests/test_gpu_verify_seams.py
runs on the device.  Needs no GPU.

Expected rows are the oracle's (tests/oracle_lib.py, pinned by tests/test_oracle_golden.py); brute() is a second,
independent reference for the verify cases: bytes.find in a loop.  Nothing expected comes from the library.  The sizes
and the field widths are read from the kernels' sources (source_constants()).

Verify cases.  The filler is ONE byte (a blank) that no pattern holds, a near miss is a copy of a pattern with ONE byte
replaced by '#', which no pattern holds either: whatever is reported lies where something was planted.  The first byte of
every pattern of the Q2 sets is an upper-case letter, the bytes behind the beginning are a .. h: no
prefix-table key begins inside a copy.  Every length class of a Q2 set comes twice: A<L> under a beginning of its own
(ONE candidate; the key holds min(L, 8) bytes, the prefix table answers for them), B<L> under the beginning it shares with
the set's shortest pattern (a candidate LIST; the key holds Q2 bytes, verify_candidate answers for all the others).

Packed-word cases.  n patterns over a .. z, the longest of exactly max_len bytes, on two groups of filler."""
from __future__ import annotations

import functools
import os
import re
from typing import Dict, List, NamedTuple, Tuple

import numpy as np

from oracle_lib import KIND_DFA, Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ahocorasick_rs_amd", "csrc")
FILL, MISS = ord(" "), ord("#")
BODY = b"abcdefgh"
KINDS = [(0, False), (0, True), (1, False), (2, False)]  # (match kind, overlapping)
LL = (2, False)


# ---------------------------------------------------------------------------
# the constants of the sources
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def source_constants() -> Dict[str, int]:
    kern = open(os.path.join(CSRC, "kernels.hip")).read()
    types = open(os.path.join(CSRC, "device_types.hpp")).read()
    auto = open(os.path.join(CSRC, "automaton.hpp")).read()
    out = {}

    def plain(name, src, where):
        m = re.search(r"\b%s\s*=\s*(\d+)\s*[,;]" % name, src)
        assert m, f"{name} is no longer a plain constant of {where}"
        out[name] = int(m.group(1))

    for n in ("W32_FIELD", "REL_BITS", "CP_BITS"):
        plain(n, kern, "kernels.hip")
    for n in ("TILE_BITS", "MAX_LOOKBACK"):
        plain(n, types, "device_types.hpp")
    for n in ("SHIFT_MAX", "FILTER2_MAX_Q"):
        plain(n, auto, "automaton.hpp")
    assert re.search(r"\bGROUP_TILES\s*=\s*ACX_GROUP_TILES\s*;", types), "GROUP_TILES is no longer ACX_GROUP_TILES"
    m = re.search(r"#define\s+ACX_GROUP_TILES\s+(\d+)\s*$", types, re.M)
    assert m, "ACX_GROUP_TILES is no longer a plain constant of device_types.hpp"
    out["GROUP_TILES"] = int(m.group(1))
    assert re.search(r"\bDT_GROUP\s*=\s*ACX_DT_GROUP\s*;", types), "DT_GROUP is no longer ACX_DT_GROUP"
    m = re.search(r"#define\s+ACX_DT_GROUP\s+(\d+)\s*$", types, re.M)
    assert m, "ACX_DT_GROUP is no longer a plain constant of device_types.hpp"
    out["DT_GROUP"] = int(m.group(1))
    # the two switches the packed rows are run under in processes of their own: read where the tests believe they are
    attempts = open(os.path.join(CSRC, "find_attempts.cpp")).read()
    assert re.search(r"wide_env\s*=\s*std::getenv\(\"ACX_MAIN_WIDE\"\)\s*!=\s*nullptr", kern) and \
        re.search(r"return\s*!codepoints\s*&&\s*!wide_env\s*&&", kern), "tile_words_narrow() no longer reads ACX_MAIN_WIDE"
    assert re.search(r"force_wide\s*=\s*std::getenv\(\"ACX_FORCE_WIDE\"\)\s*!=\s*nullptr", attempts) and \
        re.search(r"wide\s*=\s*\(x->wide\s*\|\|\s*force_wide\)", attempts), "attempt_sparse() no longer reads ACX_FORCE_WIDE"
    # the carried window and pinfo, as verify_candidate() writes them: 16 haystack bytes, 12 pattern bytes, rounds of 32
    assert re.search(r"have\s*=\s*16\s*-\s*q\s*;", kern) and re.search(r"L\s*-\s*q\s*<\s*12\s*\?\s*L\s*-\s*q\s*:\s*12\s*;", kern) \
        and re.search(r"d\s*<\s*L\s*;\s*d\s*\+=\s*32\s*\)", kern), "verify_candidate() no longer compares 16 / 12 / 32 bytes"
    assert re.search(r"if\s*\(Lw\s*==\s*255\)\s*Lw\s*=\s*A\.plen\[pid\]\s*;", kern), "the length sentinel is no longer 255"
    return out


C = source_constants()
TILE = 1 << C["TILE_BITS"]
GROUP = C["GROUP_TILES"] * TILE
DGROUP = C["DT_GROUP"] * TILE  # a group of k_dense_main
HAY_LEN = 2 * GROUP + 5000
WINDOW, PINFO, ROUND, SENTINEL = 16, 12, 32, 255


def bits_for(x: int) -> int:
    return int(x).bit_length()


def d_of(q: int) -> int:
    """where the in-place comparison begins for a pattern that reaches it"""
    return q + min(PINFO, WINDOW - q)


# ---------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------
def brute(pats, hay) -> np.ndarray:
    """every (pattern, start, end) with hay[start:end] == pattern, in the order of the oracle's overlapping Standard
    search: by end; at one end the longer pattern first, copies of a pattern by id"""
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


@functools.lru_cache(maxsize=None)
def oracle(name: str, mk: int) -> Oracle:
    return Oracle(list(patterns(name)), mk, KIND_DFA)


def rows_of(name: str, hay, mk: int, ov: bool) -> np.ndarray:
    return oracle(name, mk).find_raw(np.ascontiguousarray(hay), overlapping=ov).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def expected(name: str, mk: int, ov: bool) -> np.ndarray:
    r = rows_of(name, case(name).hay, mk, ov)
    r.setflags(write=False)
    return r


# ---------------------------------------------------------------------------
# pattern sets of the verify cases
# ---------------------------------------------------------------------------
def body(seed: int, n: int) -> bytes:
    """n letters a .. h of a fixed sequence (a 31-bit LCG: the same bytes on every interpreter)"""
    out, x = bytearray(), (seed * 2654435761 + 12345) & 0x7FFFFFFF
    for _ in range(n):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out.append(BODY[(x >> 16) & 7])
    return bytes(out)


OFFSETS = (-1, 0, 1, 7, 8, 9, 16, 17, 24, 25, 31, 32, 33, 40, 63, 64, 65)  # L - d


def lengths_of(q: int) -> List[int]:
    d = d_of(q)
    return sorted({d + x for x in OFFSETS} | {q + 1, q + 11, q + 12, q + 13, 15, 16, 17})


def miss_bytes(q: int, L: int) -> List[int]:
    """the bytes of a pattern of L bytes that get a near miss each"""
    if L <= 64:
        return list(range(q, L))
    d = d_of(q)
    return sorted(set(range(q, d + 40)) | set(range(L - 9, L)) | {k for k in range(q, L) if (k - d) % 8 in (0, 7)})


class Pat(NamedTuple):
    data: bytes
    tag: tuple  # ("short",) ("A", L) ("B", L) ("list", n, m) ("redirect", key, m) ("copy", n, m) ("sent", L) ("alone", L)
                #  ("url", bytes of the beginning, number) ("bare", L)


def q2_set(q: int) -> List[Pat]:
    g = b"Z" + body(900 + q, q - 1)
    pats = []
    for j, L in enumerate(lengths_of(q)):
        pats.append(Pat(bytes([ord("A") + j]) + body(100 * q + j, L - 1), ("A", L)))
        pats.append(Pat(g + body(100 * q + 50 + j, L - q), ("B", L)))
    pats.insert(len(pats) // 2, Pat(g, ("short",)))  # (a prefix of every B: LeftmostFirst prefers it to the B's behind it only)
    return pats


def sentinel_set() -> List[Pat]:
    x = b"X" + body(7001, 256)
    return [Pat(x[:255], ("sent", 255)), Pat(x, ("sent", 257)), Pat(x[:254], ("sent", 254)), Pat(x[:256], ("sent", 256)),
            Pat(b"Y" + body(7002, 254), ("alone", 255)), Pat(b"W" + body(7003, 255), ("alone", 256)),
            Pat(b"U" + body(7004, 253), ("alone", 254))]


LIST_Q = 5


def list_set() -> List[Pat]:
    pats = [Pat(b"V" + body(8000, LIST_Q - 1), ("short",))]
    for n in range(1, 6):
        key = bytes([ord("A") + n]) + body(8000 + n, 7)
        for m in range(n):
            pats.append(Pat(key + BODY[m:m + 1] + body(8100 + 10 * n + m, 3 + 5 * m), ("list", n, m)))
    r = b"R" + body(8200, LIST_Q - 1)
    pats += [Pat(r + b"fgh", ("redirect", "fgh", 0)), Pat(r + b"fghab" + body(8201, 3), ("redirect", "fgh", 1)),
             Pat(r + b"fga" + body(8202, 3) + body(8203, 9), ("redirect", "fga", 0)),  # (the longer one has the lower id)
             Pat(r + b"fga" + body(8202, 3), ("redirect", "fga", 1))]
    pats += [Pat(r + b"cde" + BODY[m:m + 1] + body(8210 + m, 2 + m), ("redirect", "cde", m)) for m in range(3)]
    pats.append(Pat(next(p.data for p in pats if p.tag == ("list", 3, 1)), ("copy", 3, 1)))  # the lowest id wins
    return pats


URL_PREFIXES = (b"/", b"//", b"www.", b"http:", b"ftp://", b"http://", b"https://", b"http://m.", b"http://ww2.",
                b"http://www.", b"https://www.")
HOST = b"abcdegijklnoqruvxyz"  # (letters no prefix holds)
REQUIRED_SHIFTS = (1, 4, 7, 8, 9, 12)


def url_set() -> List[Pat]:
    """hosts behind common beginnings of 1 .. 12 bytes, the endings of url_like_patterns (tests/test_gpu_round4.py); the
    beginnings on their own, so that an occurrence holds a shorter one"""
    rng = np.random.default_rng(3)
    pats = [Pat(b"http://", ("bare", 7))]  # (the lowest id and the highest: the three kinds differ)
    for pre in URL_PREFIXES:
        for i in range(24):
            host = bytes(HOST[int(v)] for v in rng.integers(0, len(HOST), int(rng.integers(6, 10))))
            pats.append(Pat(pre + host + [b".com", b".org/x", b".net/index", b""][i % 4], ("url", len(pre), i)))
    return pats + [Pat(b"https:", ("bare", 6))]


@functools.lru_cache(maxsize=None)
def url_picks() -> Tuple[int, ...]:
    """the first two patterns of every shift the host compiler gives the URL set, and two that stay at their beginning"""
    shifts = host_tables("urls")[2]
    tg = tagged("urls")
    return tuple(sorted(i for s in set(shifts) for i in [k for k, v in enumerate(shifts) if v == s and tg[k].tag[0] == "url"][:2]))


VERIFY_SETS = ["q3", "q4", "q5", "q6", "q7", "q8", "sentinel", "lists", "urls"]


@functools.lru_cache(maxsize=None)
def tagged(name: str) -> Tuple[Pat, ...]:
    if name[0] == "q" and name[1:].isdigit():
        return tuple(q2_set(int(name[1:])))
    return tuple({"sentinel": sentinel_set, "lists": list_set, "urls": url_set}[name]())


def patterns(name: str) -> Tuple[bytes, ...]:
    return tuple(p.data for p in tagged(name))


def q2_of(name: str) -> int:
    """Q2 = min(FILTER2_MAX_Q, the shortest pattern longer than 2 bytes) (automaton.cpp)"""
    return min(C["FILTER2_MAX_Q"], min(len(p) for p in patterns(name) if len(p) > 2))


@functools.lru_cache(maxsize=None)
def host_tables(name: str, mk: int = 0):
    """(filter_q2, max_shift, shifts, list lengths, ranks, keys with ONE candidate, redirect entries) of the library's own
    host compiler"""
    from ahocorasick_rs_amd import capi
    h = capi.HostAutomaton(list(patterns(name)), mk)
    q2, max_shift = int(h.t.filter_q2), int(h.t.max_shift)
    shifts = tuple(int(v) for v in h.pattern_shift)
    ranks = tuple(int(v) for v in h.rank)
    bl, lists, k = [int(v) for v in h.prefix_lists], [], 0
    while k < len(bl):  # {n, n codes} one after the other
        lists.append(bl[k])
        k += 1 + bl[k]
    assert k == len(bl)
    tab = np.array(h.prefix_table)
    final = tab[(tab[:, 2] != 0xFFFFFFFF) & (((tab[:, 2] >> 4) & 15) == 0)]
    singles = int(np.count_nonzero((final[:, 3] & 0x80000000) == 0))
    redirects = int(np.count_nonzero((tab[:, 2] != 0xFFFFFFFF) & (((tab[:, 2] >> 4) & 15) != 0)))
    h.close()
    return q2, max_shift, shifts, tuple(lists), ranks, singles, redirects


# ---------------------------------------------------------------------------
# haystacks of the verify cases
# ---------------------------------------------------------------------------
class Plant(NamedTuple):
    x: int     # where the copy starts
    pid: int
    k: int     # the byte that was replaced; -1: a true occurrence
    what: str  # "true" "miss" "group" "before" "after" "end" (flush with the haystack's end)


class Case(NamedTuple):
    name: str
    hay: np.ndarray
    plants: Tuple[Plant, ...]


def near(p: bytes, k: int) -> bytes:
    assert 0 <= k < len(p) and p[k] != MISS
    return p[:k] + bytes([MISS]) + p[k + 1:]


def copies_of(name: str) -> List[Tuple[int, int]]:
    """(pattern, replaced byte or -1) for every copy the main haystack of a set holds, in the order they are laid out"""
    tg, out = tagged(name), []
    q = q2_of(name)
    for i, p in enumerate(tg):
        L = len(p.data)
        out.append((i, -1))
        if p.tag[0] in ("A", "B"):
            ks = miss_bytes(q, L)
        elif p.tag[0] in ("sent", "alone"):
            ks = sorted({L - 1, 254} & set(range(L))) + ([8, 19, 20, 21, 52, 53, 251] if p.tag[0] == "alone" else [])
        elif p.tag[0] in ("list", "redirect", "copy"):
            ks = sorted({8, L - 1, 5, 7} & set(range(LIST_Q, L)))
        elif p.tag[0] == "url":
            s = host_tables(name)[2][i]
            ks = sorted(set(range(s)) | {s, L - 1}) if i in url_picks() else []
        else:
            ks = []
        out += [(i, k) for k in ks]
    if name[0] != "q":
        return out
    # A and B copies in turn: the shortest pattern occurs in every B copy, and a bucket of k_tile_main holds 24 occurrences
    a = [c for c in out if tg[c[0]].tag[0] != "B"]
    b = [c for c in out if tg[c[0]].tag[0] == "B"]
    both = [c for pair in zip(a, b) for c in pair]
    return both + a[len(b):] + b[len(a):]


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    pats = patterns(name)
    cp = copies_of(name)
    longest = max(len(p) for p in pats)
    # kept free for the copies at the boundaries: around the group boundary, around a tile boundary, the haystack's end
    zones = [(GROUP - 2 * longest - 16, GROUP + 2 * longest + 16), (GROUP + 8 * TILE - 2 * longest - 16, GROUP + 8 * TILE + 2 * longest + 16),
             (HAY_LEN - 2 * longest - 200, HAY_LEN)]
    pitch = min((HAY_LEN - 3000 - 12 * longest) // len(cp), 1200) | 1  # (a small set's copies: all in the first tiles)
    assert pitch >= longest + 24 and pitch >= 96, (name, pitch)  # (at most 43 copies, and as many hits, to a tile)
    h = np.full(HAY_LEN, FILL, dtype=np.uint8)
    plants = []
    x = 100
    for i, k in cp:
        data = pats[i] if k < 0 else near(pats[i], k)
        for lo, hi in zones:
            if x < hi and x + len(data) > lo:
                x = hi
        h[x:x + len(data)] = np.frombuffer(data, dtype=np.uint8)
        plants.append(Plant(x, i, k, "true" if k < 0 else "miss"))
        x += pitch
    assert x < zones[-1][0], name

    def put(x, i, what):
        assert any(lo <= x - 8 and x + len(pats[i]) + 8 <= hi + 8 for lo, hi in zones)
        h[x:x + len(pats[i])] = np.frombuffer(pats[i], dtype=np.uint8)
        plants.append(Plant(x, i, -1, what))

    big = max(range(len(pats)), key=lambda v: len(pats[v]))
    put(GROUP - longest // 2, big, "group")                 # across the group boundary
    put(GROUP + 8 * TILE - len(pats[1]), 1, "before")      # its last byte is a tile's last
    put(GROUP + 8 * TILE, 2, "after")                      # (no gap between the two)
    put(HAY_LEN - longest, big, "end")                     # its last byte is the haystack's last
    h.setflags(write=False)
    return Case(name, h, tuple(sorted(plants)))


# ---------------------------------------------------------------------------
# rows: a pattern at the end of its haystack, one byte short of it, across the cut between two rows, at a row's first byte
# ---------------------------------------------------------------------------
class Row(NamedTuple):
    data: bytes
    pid: int
    what: str  # "flush" "short" (the cut lies in front of the last byte) "cut-a" / "cut-b" (the two sides) "first" "pad"
    c: int     # bytes of the pattern in front of the cut


def cuts_of(name: str, i: int) -> List[int]:
    L, q = len(patterns(name)[i]), q2_of(name)
    cs = {L - 1, q if i % 2 == 0 else 1}
    if name == "urls":
        s = host_tables(name)[2][i]
        cs |= {s, 1} if s else set()
    return sorted(c for c in cs if 0 < c < L)


def row_patterns(name: str) -> List[int]:
    tg = tagged(name)
    if name == "urls":
        return [i for i, p in enumerate(tg) if p.tag[0] == "bare" or i in url_picks()]
    return list(range(len(tg)))


@functools.lru_cache(maxsize=None)
def rows(name: str, ragged: bool) -> Tuple[Row, ...]:
    """uniform: every row has row_len(name) bytes.  ragged: rows of every length mod 16, empty ones among them"""
    pats = patterns(name)
    U = row_len(name)
    out = []

    def pad(j, used):
        return bytes([FILL]) * ((U - used) if not ragged else 20 + (7 * j + len(out)) % 37)

    for j, i in enumerate(row_patterns(name)):
        p = pats[i]
        out.append(Row(pad(j, len(p)) + p, i, "flush", len(p)))
        for c in cuts_of(name, i):
            what = "short" if c == len(p) - 1 else "cut-a"
            out.append(Row(pad(j, c) + p[:c], i, what, c))
            out.append(Row(p[c:] + pad(j, len(p) - c), i, "cut-b", c))
        out.append(Row(p + pad(j, len(p)), i, "first", 0))
        if ragged and j % 5 == 0:
            out.append(Row(b"", i, "pad", 0))
    return tuple(out)


def row_len(name: str) -> int:
    longest = max(len(p) for p in patterns(name))
    return 192 if longest <= 128 else 640


def offsets_of(rs) -> List[int]:
    return [0] + np.cumsum([len(r.data) for r in rs]).tolist()


@functools.lru_cache(maxsize=None)
def row_expected(name: str, ragged: bool, mk: int, ov: bool) -> Tuple[np.ndarray, ...]:
    o = oracle(name, mk)
    return tuple(o.find_raw(r.data, overlapping=ov).astype(np.uint64).reshape(-1, 3) for r in rows(name, ragged))


# ---------------------------------------------------------------------------
# the other routes' haystacks
# ---------------------------------------------------------------------------
def hot_piece(name: str) -> Tuple[bytes, int]:
    """(bytes, pitch) of a dense stretch: more prefix hits to a tile than k_tile_main has slots for (64)"""
    pats = patterns(name)
    short = min(pats, key=len)
    return (short, 32) if len(short) <= 24 else (short[:40], 48)  # (the sentinel set: hits that fail at byte 40)


@functools.lru_cache(maxsize=None)
def hot_hay(name: str) -> np.ndarray:
    """the main haystack's first group, and a hot one behind it: 32 KiB of the first group's copies, 64 KiB of the dense
    stretch (as tests/test_gpu_hot.py lays one out: 8 tiles into its group), 100 KiB of copies again -- near misses in the
    hot group and in the group in front of it"""
    main = case(name).hay
    g = np.full(GROUP, FILL, dtype=np.uint8)
    g[:8 * TILE] = main[:8 * TILE]
    piece, pitch = hot_piece(name)
    for x in range(8 * TILE, 8 * TILE + (64 << 10), pitch):
        g[x:x + len(piece)] = np.frombuffer(piece, dtype=np.uint8)
    g[24 * TILE + 64:24 * TILE + 64 + 100_000] = main[8 * TILE:8 * TILE + 100_000]
    h = np.concatenate([main[:GROUP], g])
    h.setflags(write=False)
    return h


K0_PIECE, K0_PF = 16384, 40000


def k0_pieces(name: str) -> List[np.ndarray]:
    """the whole haystack twice: in pieces of 16 384 bytes (K0's own modes), in pieces of 40 000 (its prefilter mode, the one
    that calls verify_candidate())"""
    h = case(name).hay
    return [h[a:a + K0_PIECE] for a in range(0, len(h), K0_PIECE)] + [h[a:a + K0_PF] for a in range(0, len(h), K0_PF)]


# ---------------------------------------------------------------------------
# packed-word cases
# ---------------------------------------------------------------------------
class PackedRow(NamedTuple):
    name: str
    n: int
    max_len: int
    last_longest: bool


def longest_sparse() -> int:
    """the longest pattern whose context fits MAX_LOOKBACK tiles: tile_lookback() asks for max_len - 1 + 2 048 bytes"""
    return C["MAX_LOOKBACK"] * TILE - 2047


def packed_rows() -> Tuple[PackedRow, ...]:
    def row(n, max_len, last=False):
        both = n & (n - 1) == 0 and (max_len + 1) & max_len == 0
        return PackedRow(f"pw{n}x{max_len}", n, max_len, last or both)

    return (row(64, longest_sparse()), row(65, 8191), row(65, 8192), row(128, 8191, True), row(16384, 63), row(16384, 64),
            row(16385, 31), row(16385, 32))


def packed_row(name: str) -> PackedRow:
    return next(r for r in packed_rows() if r.name == name)


def rank_bits_of(n: int) -> int:
    return max(1, bits_for(n - 1))


def narrow_expected(n: int, max_len: int, codepoints: bool = False) -> bool:
    """the form k_tile_main stages in: tie + length in W32_FIELD bits, byte offsets"""
    return not codepoints and rank_bits_of(n) + bits_for(max_len) <= C["W32_FIELD"]


@functools.lru_cache(maxsize=None)
def packed_patterns(name: str) -> Tuple[bytes, ...]:
    """random patterns of 5 .. 12 letters; the longest, a prefix and a suffix of it, ONE pattern of 4 letters (the last rank
    of the kinds that rank by length) with the highest id a shortest pattern can have; the last id: the longest pattern
    where the row says so, else a pattern of 12"""
    r = packed_row(name)
    rng = np.random.default_rng(r.n * 7 + r.max_len)
    lens = rng.integers(5, 13, r.n)
    blob = rng.integers(97, 123, int(lens.sum()), dtype=np.uint8).tobytes()
    offs = np.concatenate([[0], np.cumsum(lens)])
    pats = [blob[offs[i]:offs[i + 1]] for i in range(r.n)]
    long_p = rng.integers(97, 123, r.max_len, dtype=np.uint8).tobytes()
    half = max(6, r.max_len // 2)
    pats[r.n - 1 if r.last_longest else 3] = long_p
    pats[1], pats[2], pats[4] = long_p[:half], long_p[-half:], long_p[:half - 2]  # (LeftmostFirst: 1; Standard: 4; longest: all of it)
    pats[r.n - 2] = rng.integers(97, 123, 4, dtype=np.uint8).tobytes()
    if not r.last_longest:
        pats[r.n - 1] = rng.integers(97, 123, 12, dtype=np.uint8).tobytes()
    return tuple(pats)


def packed_named(name: str) -> Dict[str, int]:
    r = packed_row(name)
    return {"longest": r.n - 1 if r.last_longest else 3, "last id": r.n - 1, "shortest": r.n - 2}


class PackedCase(NamedTuple):
    name: str
    hay: np.ndarray
    plants: Tuple[Tuple[int, int, str], ...]  # (start, pattern, what)


@functools.lru_cache(maxsize=None)
def packed_case(name: str) -> PackedCase:
    pats, named = packed_patterns(name), packed_named(name)
    n = 2 * GROUP
    h = np.full(n, FILL, dtype=np.uint8)
    taken, plants = [], []

    def put(x, i, what):
        L = len(pats[i])
        assert 0 <= x and x + L <= n and all(x + L + 2 <= a or b + 2 <= x for a, b in taken), (name, x, i, what)
        h[x:x + L] = np.frombuffer(pats[i], dtype=np.uint8)
        taken.append((x, x + L))
        plants.append((x, i, what))

    # the one group boundary there is goes to the longest pattern; its prefix and suffix lie in it.  It starts in the last
    # 1 KiB of the first group: the second group's context reaches max_len + 2 KiB back, and an occurrence that starts in its
    # last 2 KiB can be the sync point of the chains that enter the group (one that starts further back cannot: k_tile_main
    # then hands the call to the dense path, and the words under test are not the ones that run)
    who = named["longest"]
    put(GROUP - min(len(pats[who]) // 2, 1024), who, "group")
    cur = 1  # the next free tile
    for who in dict.fromkeys(named.values()):
        L = len(pats[who])
        for what in ("start first", "start last", "end first", "end last", "tile"):
            while True:
                T = (cur + (L + TILE - 1) // TILE) * TILE
                x = {"start first": T, "start last": T + TILE - 1, "end first": T - L, "end last": T + TILE - 1 - L,
                     "tile": T - (L + 1) // 2}[what]
                if all(x + L + 2 <= a or b + 2 <= x for a, b in taken):
                    break
                cur += 1
            put(x, who, what)
            cur = (x + L) // TILE + 2
    # 30 more positions
    shorts = [i for i in dict.fromkeys(named.values()) if len(pats[i]) <= 64] or [1]
    spread = [x for x in range(777, n - 100, (n - 900) // 45 | 1) if all(x + 70 <= a or b + 6 <= x for a, b in taken)][:30]
    assert len(spread) == 30, (name, len(spread))
    for k, x in enumerate(spread):
        put(x, shorts[k % len(shorts)], "spread")
    h.setflags(write=False)
    return PackedCase(name, h, tuple(sorted(plants)))


DENSE_SLACK = 2048  # tile_lookback(): the context is longer than the longest pattern by at least this


def dense_placements(L: int) -> Dict[str, int]:
    """where a pattern of L bytes may start, relative to a boundary between two groups of k_dense_main, so that the
    tile-ordered dense form can resolve the call (kernels.hip, k_dense_main: the first occurrence of a group's own tiles
    needs a certified sync point at or in front of it -- an occurrence nothing earlier reaches into, which starts in the
    group's own tiles or in the last DENSE_SLACK bytes in front of them).  So a plant lies inside ONE dense group, or
    starts less than DENSE_SLACK bytes in front of one and its nested occurrences find it in their context.  A pattern
    longer than three tiles cannot end at a tile's first byte under that rule: no "end first" for it here -- the radix
    form, which resolves globally, takes that placement (and every other one) from packed_case()."""
    out = {"start first": 0, "start last": -1, "end last": DGROUP - 1 - L, "group": -min(L // 2 + 1, DENSE_SLACK // 2)}
    if L + 1 <= DGROUP - TILE:
        out["end first"] = DGROUP - TILE - L
    out["tile"] = TILE - (L + 1) // 2 if L // 2 < TILE else -1
    return out


@functools.lru_cache(maxsize=None)
def packed_dense_case(name: str) -> PackedCase:
    """the packed row's named patterns at the placements dense_placements() allows, one dense-group boundary each; the
    longest pattern's "group" copy lies across the boundary of two groups of k_tile_main as well"""
    pats, named = packed_patterns(name), packed_named(name)
    n = 2 * GROUP
    h = np.full(n, FILL, dtype=np.uint8)
    plants = []
    b = 2  # the next dense-group boundary to plant at: a long pattern has two dense groups to itself, a short one's copies
    #        inside one group share it
    for who in dict.fromkeys(named.values()):
        L = len(pats[who])
        last_b = None
        for what, off in dense_placements(L).items():
            if what == "group" and who == named["longest"]:
                B = GROUP
            elif L <= 64 and off >= 0 and last_b is not None:
                B = last_b
            else:
                while abs(b * DGROUP - GROUP) < 3 * DGROUP:  # (the group boundary's neighbourhood is the longest pattern's)
                    b += 1
                B = b * DGROUP
                b += 2
                last_b = B if off >= 0 else last_b
            x = B + off
            assert off >= -DENSE_SLACK and (off < 0 or off + L < DGROUP) and x + L < n, (name, what, off)
            h[x:x + L] = np.frombuffer(pats[who], dtype=np.uint8)
            plants.append((x, who, what))
    xs = sorted((x, x + len(pats[i])) for x, i, _ in plants)
    assert all(a2 >= b1 + 64 for (_, b1), (a2, _) in zip(xs, xs[1:])), name
    h.setflags(write=False)
    return PackedCase(name, h, tuple(sorted(plants)))


@functools.lru_cache(maxsize=None)
def packed_hot_hay(name: str) -> np.ndarray:
    """a dense stretch (the shortest pattern every 32 bytes, 64 KiB) where the case holds nothing"""
    c = packed_case(name)
    h = np.array(c.hay)
    pats = packed_patterns(name)
    p = np.frombuffer(pats[packed_named(name)["shortest"]], dtype=np.uint8)
    spans = [(x, x + len(pats[i])) for x, i, _ in c.plants]
    free = [T for T in range(TILE, 2 * GROUP - (65 << 10), TILE) if all(b + 64 <= T or T + (64 << 10) + 64 <= a for a, b in spans)]
    assert free, name
    for x in range(free[0], free[0] + (64 << 10), 32):
        h[x:x + len(p)] = p
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def packed_oracle(name: str, mk: int) -> Oracle:
    return Oracle(list(packed_patterns(name)), mk, KIND_DFA)


# ---------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------
def plan() -> Tuple[str, ...]:
    """the names of all cases: nine verify sets, eight packed-word rows"""
    return tuple(VERIFY_SETS) + tuple(r.name for r in packed_rows())
