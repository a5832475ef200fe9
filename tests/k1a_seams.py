"""K1a -- the DFA-walk scan (kernels.hip; reached by acx_set_kernel / kernel=capi.KERNEL_DFA_WALK / ACX_KERNEL=dfa_walk) -- at
its seams in all three forms: the constants, the pattern sets, the haystacks and the plan that tests/test_k1a_seams_cpu.py
checks on the CPU and tests/test_gpu_k1a_seams.py runs on the device.  Needs no GPU (run_leg() and what it calls import the
library when called).

The forms (form_of() restates launch_k1a() / launch_dfa_walk()):
  failureless  k1a_scan + k1a_walk over walk_t3b / walk_t3r / walk_grec: automata of at most 32 byte classes;
  walk16       k1a_walk16: a dense table of at most 65 535 states, ONE haystack, four chains a lane;
  chunked      k1a_dfa_walk over walk_span() / dfa_step(): batches, and dense tables of more states;
  chunked_nfa  ... over nfa_step(): no dense table (built under ACX_DENSE_LIMIT=0).
ACX_NO_PFAC (read once per process: ONE child) puts the failureless sets on walk16 / chunked.

Expected rows are the oracle's (tests/oracle_lib.py); k1b_seams.brute() / brute_iter() and post_seams.brute_leftmost() are the
second reference.  Nothing expected comes from the device.  Sizes are read from the sources (source_constants()): a changed
constant moves the cases with it, a renamed one, or a line the plan restates that no longer stands, fails on the CPU.

Every plant is placed on a filler ('-') that no pattern holds.  walk16 works on the index space of the 16-byte aligned
address below the pointer (index = lead + stream position): its chunk seams are planted by INDEX.  The chunked walk works on
stream positions.  The failureless form works like K1b: tiles of 4 KiB of the index space, 16 waves a workgroup.

Classes: (a) the ends of the stream, (b) chunk seams, (c) table seams (LDS rows, walk_plain, 0x3FFF / 0xFFFF), (d) haystack
borders, (e) stage G and the walk of the failureless form (tails, the 64th hit slot), (f) the region capacity of k1a_scan.
(g) the wave turns of the failureless form at 16 x CUs tiles and the counts' batches of 16 (turn_case(): expected rows from the
plants, hit-slot sink only)."""
from __future__ import annotations

import functools
import json
import os
import re
import sys
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

import gen
from k0_seams import hay_of
from k1b_seams import NUL_STEMS, brute, code_points_at, cols, letters, with_env
from oracle_lib import KIND_DFA, Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ahocorasick_rs_amd", "csrc")
KINDS = [(0, True), (0, False), (1, False), (2, False)]  # (match kind, overlapping): the overlapping kind first, on a fresh handle
FILL = ord("-")
MAX_LDS = 160 * 1024  # what build_upload.cpp clamps a->max_lds to, and what the MI355X has
ID_MASK = 0x3FFFFFFF


# ---------------------------------------------------------------------------
# the constants of the sources, and the lines the plan restates
# ---------------------------------------------------------------------------
def _pin(text: str) -> str:
    """a source line as a pattern: its tokens, whatever the white space between them"""
    return r"\s*".join(re.escape(t) for t in re.findall(r"\w+|[^\w\s]", text))


PINNED = (  # (file, the line): each of its own line
    ("kernels.hip", "const bool emit = i >= warm;"),
    ("kernels.hip", "if (lo >= (int64_t)lead && hi <= (int64_t)total) {"),
    ("kernels.hip", "if (emit && t_ >= plain)"),
    ("kernels.hip", "uint64_t pos = c0 > warm ? c0 - warm : 0;"),
    ("kernels.hip", "bool emit = pos >= c0;"),
    ("kernels.hip", "while (nb == pos);"),
    ("kernels.hip", "if (s < W.hot_rows) {"),
    ("kernels.hip", "if (v != 0xFFFFu) return (v & 0x3FFFu) | ((v & 0xC000u) << 16);"),
    ("kernels.hip", "const bool interior = tbase >= lead && tbase + tile_bytes + 4 <= last_start;"),
    ("kernels.hip", "if (p0_ + j + 4 > total) force_ |= 1u << j;"),
    ("kernels.hip", "if (any_start && p0_ + j >= lead && p0_ + j <= last_start) keep_ |= 1u << j;"),
    ("kernels.hip", "rootG = (eT.y & T3R_SHORT) != 0 || posT + 5 > len;"),
    ("kernels.hip", "if (hit) hit = 4 + tn <= segment_end(G, len, posG) - posG;"),
    ("kernels.hip", "bool same = d + tn <= room;"),
    ("kernels.hip", "if (d >= room) break;"),
    ("kernels.hip", "if (d > room) continue;"),
    ("kernels.hip", "if (d - wd >= 8) { w = load_window(stream, len, pos + d); wd = d; }"),
    ("kernels.hip", "if (slot < HIT_SLOTS)"),
    ("kernels.hip", "if (go && slot < dcap) {"),
    ("kernels.hip", "if (n > D.cap) {"),
    ("kernels.hip", "if ((kG & 15) == 15) {"),
    ("kernels.hip", "const uint64_t last_start = total >= min_len ? total - min_len : 0;"),
    ("kernels.hip", "const bool any_start = total >= lead + min_len;"),
    ("kernels.hip", "if (A.table16 && !segmented) {"),
    ("kernels.hip", "const uint32_t warm = ((A.max_len ? A.max_len - 1 : 0) + 15u) & ~15u;"),
    ("kernels.hip", "const uint64_t warm = A.max_len ? A.max_len - 1 : 0;"),
    ("kernels.hip", "uint32_t rows16 = (uint32_t)std::min<size_t>(budget / ((size_t)2 * NC), A.n_states);"),
    ("kernels.hip", "if (A.table16) return (uint32_t)n_cus;"),
    ("kernels.hip", "bool pfac_available(const DevAutomaton &A, size_t max_lds) { return A.t3b != nullptr && max_lds >= sizeof(K1aLds); }"),
    ("find_attempts.cpp", "const bool pfac = !c.pre && pfac_available(a->dev, a->max_lds) && !no_pfac_on() && !c.chunked_walk;"),
    ("find_attempts.cpp", 'bool no_pfac_on() { static const bool no_pfac = std::getenv("ACX_NO_PFAC") != nullptr; return no_pfac; }'),
    ("find_attempts.cpp", 'bool no_bucket_now() { const bool no_sparse_env = std::getenv("ACX_NO_BUCKET") != nullptr; return no_sparse_env; }'),
    ("automaton.cpp", 'const char *env = std::getenv("ACX_DENSE_LIMIT");'),
    ("automaton.cpp", "if (A.n_classes > 32 || A.n_patterns == 0) return;"),
    ("automaton.cpp", "else if (nc == 1 && !own && tl[c0] < 8) {"),
    ("build_upload.cpp", "hot16[i] = id < 0x3FFFu ? (uint16_t)(id | ((en >> 30) << 14)) : (uint16_t)0xFFFF;"),
    ("build_upload.cpp", "if (H.dense && H.n_states <= 0xFFFF && H.n_patterns > 0) {"),
    ("build_upload.cpp", "if (a->max_lds > 160 * 1024) a->max_lds = 160 * 1024;"),
)


def _function(src: str, head: str) -> str:
    at = src.index(head)
    return src[at:src.index("\n}\n", at)]


@functools.lru_cache(maxsize=None)
def source_constants() -> Dict[str, int]:
    src = {f: open(os.path.join(CSRC, f)).read() for f in ("kernels.hip", "automaton.hpp", "automaton.cpp", "device_types.hpp",
                                                           "build_upload.cpp", "find_attempts.cpp")}
    kern = src["kernels.hip"]
    out: Dict[str, int] = {}

    def plain(name, f):
        m = re.search(r"\b%s\s*=\s*(\d+)\s*[,;]" % name, src[f])
        assert m, f"{name} is no longer a plain constant of {f}"
        out[name] = int(m.group(1))

    plain("K1A_CHAINS", "kernels.hip")
    plain("K1A_LDS_HEADER", "kernels.hip")
    plain("HIT_SLOTS", "device_types.hpp")
    plain("TILE_BITS", "device_types.hpp")
    m = re.search(r"#define\s+ACX_STAGE_SLOTS\s+(\d+)\s*$", kern, re.M)
    assert m and re.search(r"\bSTAGE_SLOTS\s*=\s*ACX_STAGE_SLOTS\s*;", kern), "STAGE_SLOTS is no longer ACX_STAGE_SLOTS"
    out["STAGE_SLOTS"] = int(m.group(1))
    plain("STAGE_SLOTS_W32", "kernels.hip")
    m = re.search(r"\bK1A_T3B_WORDS\s*=\s*(\d+)\s*\*\s*(\d+)\s*;", src["automaton.hpp"])
    assert m, "K1A_T3B_WORDS is no longer 1024 * 33"
    out["K1A_T3B_WORDS"] = int(m.group(1)) * int(m.group(2))
    for f, line in PINNED:
        assert re.search(_pin(line), src[f]), f"{f} no longer holds the line the plan restates: {line}"

    def lits(head, pattern, names):
        m = re.search(pattern, re.sub(r"\s+", " ", _function(kern, head)))
        assert m, f"{head.split('(')[0].split()[-1]}() is no longer what the plan restates"
        for n, v in zip(names, m.groups()):
            out[n] = int(v, 0)

    lits("static uint32_t walk16_chunk(",
         r"uint64_t c = total / \(\(uint64_t\)n_cus \* (\d+) \* K1A_CHAINS\); c = \(c \+ 15\) & ~15ull; if \(c < (\d+)\) c = \2; "
         r"if \(c < \(uint64_t\)warm \* (\d+)\) c = \(uint64_t\)warm \* \3; if \(c > \(1u << (\d+)\)\) c = 1u << \4; return",
         ("W16_THREADS", "W16_MIN", "W16_WARMX", "W16_MAXLOG"))
    lits("static uint32_t pick_chunk(",
         r"uint64_t c = (\d+); uint64_t need = \(uint64_t\)\(max_len \? max_len - 1 : 0\) \* (\d+); if \(c < need\) c = \(need \+ (\d+)\) & ~\3ull;",
         ("CH_MIN", "CH_WARMX", "CH_ROUND"))
    lits("uint32_t dfa_walk_hot_rows(",
         r"size_t budget = max_lds > (\d+) \+ K1A_LDS_HEADER \? max_lds - \1 - K1A_LDS_HEADER : 0; size_t rows = budget / \(\(size_t\)2 << stride2\); "
         r"if \(rows > n_states\) rows = n_states; if \(rows > (0x[0-9A-Fa-f]+)\) rows = \2;", ("LDS_SPARE", "HOT_MAX"))
    lits("static uint64_t pfac_region_cap(",
         r"return len / \(dense \? (\d+) : (\d+)\) / \(\(uint64_t\)scan_grid \* 16\) \+ (\d+);", ("CAP_DENSE_DIV", "CAP_DIV", "CAP_BASE"))
    lits("uint32_t pfac_scan_grid(",
         r"const uint64_t total = \(\(uintptr_t\)d_hay & 15\) \+ len; uint64_t blocks = \(\(total \+ (\d+)\) / (\d+) \+ 15\) / 16; "
         r"if \(blocks > \(uint64_t\)n_cus\) blocks = n_cus; return blocks \? \(uint32_t\)blocks : 1;", ("GRID_ROUND", "GRID_TILE"))
    assert out["GRID_TILE"] == 1 << out["TILE_BITS"] and out["GRID_ROUND"] == out["GRID_TILE"] - 1
    assert out["HOT_MAX"] == 0x3FFF
    return out


C = source_constants()
TILE = 1 << C["TILE_BITS"]
HIT_SLOTS, CHAINS = C["HIT_SLOTS"], C["K1A_CHAINS"]
# k_tile_main stages at most STAGE_SLOTS occurrences a bucket (4 KiB of key positions: ends under Standard, starts under the
# leftmost kinds; STAGE_SLOTS_W32 in its narrow-word form).  K1a's hits have no hot pipeline behind them (hot_ok == 0): a
# fuller bucket raises the abort flag and the call is redone on the dense path -- BEFORE a tile's 64 hit slots can overflow
# (the occurrences of one tile's starts end in at most two buckets).  A case the plan expects on the sparse path holds at most
# STAGE_SLOTS a bucket; one it expects to leave holds more than STAGE_SLOTS_W32.
BUCKET, BUCKET_W32 = C["STAGE_SLOTS"], C["STAGE_SLOTS_W32"]


def warm16(max_len: int) -> int:
    return ((max_len - 1 if max_len else 0) + 15) & ~15


def walk16_chunk(max_len: int, total: int, cus: int) -> int:
    c = total // (cus * C["W16_THREADS"] * CHAINS)
    c = max((c + 15) & ~15, C["W16_MIN"], warm16(max_len) * C["W16_WARMX"])
    return min(c, 1 << C["W16_MAXLOG"])


def pick_chunk(max_len: int) -> int:
    need = (max_len - 1 if max_len else 0) * C["CH_WARMX"]
    return C["CH_MIN"] if C["CH_MIN"] >= need else (need + C["CH_ROUND"]) & ~C["CH_ROUND"]


def lds_budget(max_lds: int = MAX_LDS) -> int:
    return max(max_lds - C["LDS_SPARE"] - C["K1A_LDS_HEADER"], 0)


def hot_rows(n_states: int, stride: int, max_lds: int = MAX_LDS) -> int:
    return min(lds_budget(max_lds) // (2 * stride), n_states, C["HOT_MAX"])


def rows16(n_states: int, n_classes: int, max_lds: int = MAX_LDS) -> int:
    return min(lds_budget(max_lds) // (2 * n_classes), n_states)


def pfac_scan_grid(lead: int, n: int, cus: int) -> int:
    return max(1, min(((lead + n + TILE - 1) // TILE + 15) // 16, cus))


def pfac_region_cap(n: int, grid: int, dense: bool) -> int:
    return n // (C["CAP_DENSE_DIV"] if dense else C["CAP_DIV"]) // (grid * 16) + C["CAP_BASE"]


def walk16_turns(total: int, max_len: int, cus: int) -> int:
    """turns of k1a_walk16's grid-stride loop: groups of K1A_CHAINS chunks over cus * 1024 lanes"""
    chunk = walk16_chunk(max_len, total, cus)
    groups = ((total + chunk - 1) // chunk + CHAINS - 1) // CHAINS
    return (groups + cus * 1024 - 1) // (cus * 1024)


# ---------------------------------------------------------------------------
# pattern sets
# ---------------------------------------------------------------------------
ALPHA40 = bytes(range(97, 123)) + bytes(range(65, 79))  # a-z, A-N: 41 byte classes
# the byte classes are the used bytes and the runs of unused ones between them: a .. ~ is 30 used bytes and two runs, 32
# classes; one used byte more (0x7F) is 33.  (The sets keep the names of their class counts' neighbours, 31 | 32 used bytes.)
BASE31 = (b"qwert", b"yuiop", b"asdfgh", b"jklzxcvbnm", b"{|}~", b"bnm{|")  # nothing under 4 bytes
TAIL_REST = (0, 1, 7, 8, 9, 12, 13, 16, 17)  # bytes below depth 4: lengths 4, 5, 11, 12, 13 (GREC_TAIL at 8, walked at 9), 16, 17, 20, 21
NULS = tuple(stem + b"\0" * k for stem, k in NUL_STEMS)
CAP_PAT = b"a" * 17 + b"b"


def tail_pattern(k: int) -> bytes:
    """the pattern with TAIL_REST[k] bytes below its depth-4 node; its first byte is its own, so its chain is alone"""
    return bytes([ord("b") + k]) + letters(900 + k, 3 + TAIL_REST[k])


TAILS = tuple(tail_pattern(k) for k in range(len(TAIL_REST)))
OWN4, OWN4_LONG = b"wxyz", b"wxyzuv"  # a pattern that ends at a depth-4 node with children: GREC_OWN, the walk goes on


def long_pattern(L: int) -> bytes:
    return b"N" + bytes(ALPHA40[(7 * i + L) % 40] for i in range(L - 2)) + b"M"


@functools.lru_cache(maxsize=None)
def below_65535() -> Tuple[Tuple[bytes, ...], int]:
    """(the most patterns of a pool that leave room for one more of at least 5 bytes below 65 535 states, that room): ONE
    search over HostAutomaton for w16max and its twin (about 15 builds, 0.5 s)"""
    pool = tuple(dict.fromkeys(gen.gen_patterns(11000, 5, 12, ALPHA40, 172)))
    from ahocorasick_rs_amd import capi

    def states(k):
        h = capi.HostAutomaton(list(pool[:k]))
        n = h.n_states
        h.close()
        return n
    lo, hi = 1, len(pool)
    assert states(lo) <= 0xFFFF - 5 < states(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if states(mid) <= 0xFFFF - 5 else (lo, mid)
    room = 0xFFFF - states(lo)
    assert 5 <= room <= 17, room
    return pool[:lo], room


@functools.lru_cache(maxsize=None)
def patterns(name: str) -> Tuple[bytes, ...]:
    w16 = tuple(dict.fromkeys(gen.gen_patterns(1500, 5, 12, ALPHA40, 171)))
    if name == "fl31":
        return BASE31
    if name == "fl32":      # one used byte more: 33 classes, no failureless tables
        return BASE31 + (b"\x7fqwe\x7f",)
    if name == "flshort":   # T3R_SHORT, ITEM_ROOT, the all-ones t3b entries
        return BASE31 + (b"q", b"as", b"jkl")
    if name == "flalias":   # a / A / !: one symbol (low five bits), three classes: t3b passes, t3r rejects
        return (b"aAb!x", b"Aab!!", b"!aAbq", b"abab", b"qwert")
    if name == "fltail":
        return TAILS + (OWN4, OWN4_LONG)
    if name == "flmany":    # OWN1_MANY: at a depth-4 node, at the leaf of a chain (the chain is NOT a tail), below depth 4
        return (b"manyx",) * 3 + (b"duplicate",) * 3 + (b"four",) * 3 + (b"qwert",)
    if name == "flnul":
        return NULS + (b"qwert", b"nulo")
    if name == "flcap":
        return (CAP_PAT,)
    if name == "w16":
        return w16
    if name.startswith("w16len"):
        return w16 + (long_pattern(int(name[6:])),)
    if name in ("w16max", "w16over"):  # exactly 65 535 states, and its twin of 65 536: no table16
        base, room = below_65535()
        return base + (b"0" + b"1" * (room - 1 + (name == "w16over")),)  # (a fresh first byte: one state a byte)
    if name == "ch3fff":    # the first 16 000 three-byte strings over 33 letters, and one pattern through the first depth-3 node
        a = ALPHA40[:33]
        three = tuple(bytes([a[i // 1089], a[i // 33 % 33], a[i % 33]]) for i in range(16000))
        return three + (three[0] + b"bcdefgh",)
    if name == "chnfa":     # built under ACX_DENSE_LIMIT=0
        return w16
    raise KeyError(name)


FL_SETS = ("fl31", "flshort", "flalias", "fltail", "flmany", "flnul")
W16_SETS = ("fl32", "w16", "w16len17", "w16len18", "w16len33", "w16len34", "w16max")
SETS = FL_SETS + ("flcap",) + W16_SETS + ("w16over", "ch3fff", "chnfa")


def dense_limit0(name: str) -> bool:
    return name == "chnfa"


_hosts: Dict[tuple, object] = {}


def host(name: str, mk: int = 0):
    """the set's HostAutomaton (kept: its arrays are views)"""
    if (name, mk) not in _hosts:
        from ahocorasick_rs_amd import capi
        with with_env({"ACX_DENSE_LIMIT": "0"} if dense_limit0(name) else {}):
            _hosts[(name, mk)] = capi.HostAutomaton(list(patterns(name)), mk)
    return _hosts[(name, mk)]


def form_of(h, segmented: bool, no_pfac: bool = False, chunked_again: bool = False) -> str:
    """launch_k1a() and launch_dfa_walk(): which of K1a's kernels a call of kernel=KERNEL_DFA_WALK runs"""
    assert (len(h.walk_t3b) > 0) == (h.n_classes <= 32)
    if len(h.walk_t3b) and not no_pfac and not chunked_again:
        return "failureless"
    if h.dense and h.n_states <= 0xFFFF and not segmented:
        return "walk16"
    return "chunked" if h.dense else "chunked_nfa"


def max_len(name: str) -> int:
    return max(len(p) for p in patterns(name))


def min_len(name: str) -> int:
    return min(len(p) for p in patterns(name))


def longest(name: str) -> bytes:
    return max(patterns(name), key=len)


def unit(name: str) -> bytes:
    """the set's plant: one occurrence of itself"""
    return {"flalias": b"aAb!x", "fltail": TAILS[1], "flmany": b"qwert", "flnul": b"qwert", "flcap": CAP_PAT,
            "ch3fff": patterns("ch3fff")[5000]}.get(name, patterns(name)[0])  # (ch3fff: three bytes -- its long pattern holds eight more)


# ---------------------------------------------------------------------------
# the host tables, walked
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def walk_order(name: str) -> Tuple[np.ndarray, np.ndarray, int]:
    """(walk id of a BFS id, BFS id of a walk id, walk_plain) as upload_tables() numbers table16's rows: the states no
    transition reports first, in BFS order, the reporting ones behind them"""
    h = host(name)
    t = h.table
    rep = np.zeros(h.n_states, bool)
    rep[(t & ID_MASK)[(t >> 31) == 1]] = True
    bfs = np.concatenate([np.flatnonzero(~rep), np.flatnonzero(rep)])
    of = np.empty(h.n_states, np.int64)
    of[bfs] = np.arange(h.n_states)
    return of, bfs, int((~rep).sum())


def visited(name: str, hay: bytes) -> List[int]:
    """the dense table's entry (id | flags) behind every byte of `hay`, walked from the root"""
    h = host(name)
    cls, t, s, out = h.classes, h.table, 0, []
    for b in hay:
        e = int(t[s, cls[b]])
        out.append(e)
        s = e & ID_MASK
    return out


@functools.lru_cache(maxsize=None)
def parents(name: str) -> np.ndarray:
    h = host(name)
    fc = h.first_child.astype(np.int64)
    par = np.zeros(h.n_states, np.int64)
    for s in range(h.n_states):
        par[fc[s]:fc[s + 1]] = s
    return par


def string_of(name: str, s: int) -> bytes:
    """the bytes on the trie path to state s"""
    h, par, out = host(name), parents(name), bytearray()
    while s:
        out.append(int(h.in_byte[s]))
        s = int(par[s])
    return bytes(reversed(out))


def pattern_through(name: str, s: int) -> bytes:
    """a pattern whose trie path passes state s: down the first children to a state that ends one"""
    h = host(name)
    while not (int(h.state_flags[s]) & 1):
        assert h.first_child[s] < h.first_child[s + 1]
        s = int(h.first_child[s])
    return string_of(name, s)


@functools.lru_cache(maxsize=4096)
def scan_trace(name: str, hay: bytes, slots: bool = True) -> Dict[str, np.ndarray]:
    """per stream position of ONE haystack at pointer residue 0: the survivors of level 1, the items k1a_scan leaves for
    k1a_walk, the hits stage G writes itself -- counted by the Python twin of the failureless form (test_host_cpu.py,
    imported: ONE restatement of the walk tables' decode).  The twin walks every position; the kernel keeps a position only
    up to last_start and where any_start holds (the keep_ line, PINNED above): that mask is applied here.  slots = False
    (the occurrence regions): stage G's hits leave as items too"""
    from test_host_cpu import failureless_walk_occurrences
    tr = {"survivors": [], "items": [], "hits": []}
    failureless_walk_occurrences(host(name), hay, trace=tr)
    n, mn = len(hay), min_len(name)
    keep = np.arange(n) <= n - mn if n >= mn else np.zeros(n, bool)
    out = {}
    for k, v in tr.items():
        out[k] = np.zeros(n, bool)
        out[k][np.asarray(v, np.int64)] = True
        out[k] &= keep
    if not slots:
        out["items"], out["hits"] = out["items"] | out["hits"], np.zeros(n, bool)
    return out


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------
class Case(NamedTuple):
    cls: str
    set: str
    name: str
    form: str                       # the form the call is meant for (checked against form_of() on the CPU)
    hay: bytes
    cuts: Tuple[int, ...] = ()      # a batch: the offsets of its haystacks (n + 1 of them); (): one haystack
    uniform: int = 0                # ... passed as uniform_len (the cuts are its multiples)
    residues: Tuple[int, ...] = (0,)
    leaves: bool = False            # on the hit-slot sink the call leaves the sparse path (a fresh handle either way)
    fresh: bool = False             # a path-asserting call: on a handle of its own
    host_too: bool = False          # a batch: from host memory as well (find_batch)
    claim: tuple = ()               # what the class says of the call, recomputed on the CPU


RES4 = (0, 1, 8, 15)
A_LENS = (1, 2, 3, 4, 5, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 8192 + 21)


def single_form(name: str, nopfac: bool = False) -> str:
    return form_of(host(name), False, no_pfac=nopfac)


def batch_form(name: str, nopfac: bool = False) -> str:
    return form_of(host(name), True, no_pfac=nopfac)


def fits(name: str, room: int, k: int = 0) -> bytes:
    """the k-th longest pattern of at most `room` bytes (b"": none)"""
    ps = sorted({p for p in patterns(name) if len(p) <= room}, key=lambda p: (-len(p), p))
    return ps[k % len(ps)] if ps else b""


def cases_a(name: str, nopfac: bool = False) -> List[Case]:
    """the ends of the stream: every length with the longest pattern that fits from byte 0 and one flush with the last byte;
    every pattern length flush with the last byte and one byte short; the NUL patterns with the stream cut in front of the
    NULs.  Failureless form: the last three positions leave level 1 by force_ (bytes behind the end took part in the
    test), are kept by keep_ up to last_start, and walk from the root (posT + 5 > len); below min_len any_start is false"""
    form, out = single_form(name, nopfac), []
    for n in A_LENS:
        e = fits(name, n)
        first = fits(name, n - len(e), 1)
        plants = ([(0, first)] if first else []) + ([(n - len(e), e)] if e else [])
        out.append(Case("a", name, f"len_{n}", form, hay_of(n, plants), residues=RES4, claim=(("ends_at", n),) if e else (("n", 0),)))
    big = longest(name)
    out.append(Case("a", name, "longest_from_0", form, hay_of(len(big) + 40, [(0, big)]), residues=RES4, claim=(("starts_at", 0),)))
    for L in sorted({len(p) for p in patterns(name)})[:24]:
        p = next(q for q in patterns(name) if len(q) == L)
        n = 200 + 3 * L
        out.append(Case("a", name, f"flush_L{L}", form, hay_of(n, [(20, unit(name)), (n - L, p)]), residues=RES4, claim=(("ends_at", n),)))
        out.append(Case("a", name, f"short_L{L}", form, hay_of(n + 1, [(20, unit(name)), (n + 1 - L, p)])[:n], residues=RES4,
                        claim=(("cut", p),)))
    if name == "flnul":
        for stem, k in NUL_STEMS:
            for n in (300, TILE + len(stem)):
                out.append(Case("a", name, f"nul{k}_cut_{n}", form, hay_of(n, [(60, stem + b"\0" * k), (n - len(stem), stem)]),
                                residues=RES4, claim=(("cut", stem + b"\0" * k),)))
                out.append(Case("a", name, f"nul{k}_flush_{n}", form, hay_of(n, [(n - len(stem) - k, stem + b"\0" * k)]),
                                residues=RES4, claim=(("ends_at", n),)))
    return out


def cases_b_walk16(name: str, cus: int, nopfac: bool = False) -> List[Case]:
    """walk16's chunk seams, by INDEX: an occurrence ending at a chunk's last byte and at the next chunk's first byte, the
    longest pattern ending at a chunk's first byte (its start is the warm-up's first byte when max_len - 1 is a multiple of
    16), at the borders chain 0 | 1, lane | lane (chain 3 | chain 0), wave | wave, workgroup | workgroup; the first and the
    last group (checked steps), interior groups (K1A_STEP4), a group that straddles `total`"""
    form, ml, u, big, out = single_form(name, nopfac), max_len(name), unit(name), longest(name), []
    assert form == "walk16"
    for label, chains, leads in (("lanes", 4 * 6 + 2, RES4), ("waves", 4 * 64 * 2 + 3, (0, 15)), ("groups", 4 * 1024 + 4 * 5 + 1, (8, 1))):
        for li, lead in enumerate(leads):
            chunk = walk16_chunk(ml, lead + chains * C["W16_MIN"], cus)
            total = chains * chunk - (chunk // 2 + 5)          # the last chunk is partial; the last group straddles `total`
            assert walk16_chunk(ml, total, cus) == chunk and walk16_turns(total, ml, cus) == 1
            borders = sorted({1, 2, 4, 8, 12, chains - 1} | ({256, 512} if chains > 512 else set()) | ({4096} if chains > 4097 else set()))
            plants, claim = [], []
            for k, c in enumerate(borders):
                x = c * chunk                                   # index of the chunk's first byte
                p = (u, big, fits(name, 64, k))[k % 3]
                plants.append((x - len(p) - 60, p, x - 60))     # inside the chunk before
                if (c + li) % 2:
                    plants.append((x - len(p), p, x))           # ends at the chunk's last byte
                else:
                    plants.append((x + 1 - len(big), big, x + 1))  # the longest pattern ends at the chunk's first byte
                claim += [("ends_at_index", x + 1 - (c + li) % 2)]
            keep, taken = [], []
            for s, p, e in sorted(plants):
                if s >= lead and e <= total and all(s > t + 1 for t in taken):
                    keep.append((s - lead, p))
                    taken.append(e)
            claim = [c for c in claim if any(s + lead + len(p) == c[1] for s, p in keep)]
            assert claim
            out.append(Case("b", name, f"{label}_r{lead}", form, hay_of(total - lead, keep), residues=(lead,),
                            claim=tuple(claim) + (("chunk", chunk), ("odd_walk", (warm16(ml) + chunk) // 16 % 2))))
    return out


def second_turn_case(cus: int) -> Case:
    """cus MiB + three chunks and a bit under w16: walk16_chunk() leaves the chunk at 256 bytes, cus * 1024 lanes of four
    chains hold cus MiB, and lane 0 of workgroup 0 takes a SECOND turn of the grid-stride loop for the rest (a partial group).
    Plants: an occurrence ending at the first turn's last byte, one starting at the second turn's first byte, the longest
    pattern ending at the first byte of the second turn's chain 1, one flush with the end; one every MiB in front"""
    u, big = unit("w16"), longest("w16")
    chunk = C["W16_MIN"]
    x = chunk * CHAINS * 1024 * cus
    n = x + 3 * chunk + 77
    assert walk16_chunk(max_len("w16"), n, cus) == chunk and walk16_turns(n, max_len("w16"), cus) == 2
    plants = [(k << 20 | 33, u) for k in range(cus)] + [(x - len(u), u), (x, u), (x + chunk + 1 - len(big), big), (n - len(u), u)]
    return Case("b", "w16", "second_turn", "walk16", hay_of(n, plants), claim=(("chunk", chunk), ("turns", 2)))


def cases_b_chunked(name: str, nopfac: bool = False) -> List[Case]:
    """the chunked walk's seams, by stream position: occurrences ending at c0 (the chunk before emits them) and at c0 + 1
    (the chunk's first emitted byte), the longest pattern starting at c0 - warm (the warm-up's first byte) and at
    c0 - warm - 1, at every pointer residue (walk_span()'s alignment loop).  A set with a table16 reaches the chunked walk
    as a batch of ONE haystack"""
    ml, u, big, out = max_len(name), unit(name), longest(name), []
    one = form_of(host(name), False, no_pfac=nopfac) in ("chunked", "chunked_nfa")
    form = single_form(name, nopfac) if one else batch_form(name, nopfac)
    assert form in ("chunked", "chunked_nfa")
    chunk, warm = pick_chunk(ml), ml - 1
    n = 6 * chunk + chunk // 3
    plants, claim = [], []
    for c in ((1, 2, 3, 4, 5) if len(brute(patterns(name), big)) <= 2 else (1, 2)):  # (few enough for a bucket of the post stage)
        c0 = c * chunk
        plants += [((c0 - len(u), u) if c % 2 else (c0 + 1 - len(u), u)), (c0 - warm - (c % 2), big)]
        claim += [("ends_at", c0 if c % 2 else c0 + 1), ("starts_at", c0 - warm - (c % 2))]
    plants = [(s, p) for s, p in plants if s >= 0]
    plants.sort()
    kept = [plants[0]]
    for s, p in plants[1:]:
        if s > kept[-1][0] + len(kept[-1][1]):
            kept.append((s, p))
    claim = [c for c in claim if any((s + len(p) if c[0] == "ends_at" else s) == c[1] for s, p in kept)]
    assert len(claim) >= 3, claim
    out.append(Case("b", name, "chunks", form, hay_of(n, kept), cuts=() if one else (0, n), uniform=0 if one else n,
                    residues=tuple(range(16)), claim=tuple(claim) + (("chunk", chunk),)))
    return out


def cases_c(name: str) -> List[Case]:
    """table seams.  walk16: plants whose walks pass walk-order states rows16 - 1 and rows16 (the LDS rows' edge), a plant
    whose only reporting state is walk_plain (the first reporting one) and one whose walk passes walk_plain - 1 (the last
    that reports nothing).  chunked: BFS states hot_rows - 1 | hot_rows; ch3fff: a hot-row entry stored as 0xFFFF (a target
    >= 0x3FFF) and hot-row entries with OUT and OWN set"""
    h, out = host(name), []
    if single_form(name) == "walk16":
        of, bfs, plain = walk_order(name)
        r16 = rows16(h.n_states, h.n_classes)
        want = [("walk_state", plain), ("walk_state", plain - 1)] + ([("walk_state", r16 - 1), ("walk_state", r16)] if r16 < h.n_states else [])
        plants = [pattern_through(name, int(bfs[w])) for _, w in want]
        x, ps = 30, []
        for p in plants:
            ps.append((x, p))
            x += len(p) + 40
        out.append(Case("c", name, "rows16_plain", "walk16", hay_of(x + 300, ps), residues=(0, 15), claim=tuple(want) + (("rows16", r16),)))
    if h.dense and h.n_states > hot_rows(h.n_states, h.stride):
        hr = hot_rows(h.n_states, h.stride)
        want = [("bfs_state", hr - 1), ("bfs_state", hr)]
        plants = [pattern_through(name, hr - 1), pattern_through(name, hr)]
        if name == "ch3fff":
            want += [("hot_ffff",), ("hot_flag", 31), ("hot_flag", 30)]
            plants.append(patterns(name)[-1])
        x, ps = 30, []
        for p in plants:
            ps.append((x, p))
            x += len(p) + 40
        n = x + 300
        one = single_form(name) == "chunked"
        out.append(Case("c", name, "hot_rows", "chunked", hay_of(n, ps), cuts=() if one else (0, n), uniform=0 if one else n,
                        residues=(0, 15), claim=tuple(want) + (("hot_rows", hr),)))
    return out


def batch_of(rows: List[bytes]) -> Tuple[bytes, Tuple[int, ...]]:
    cuts = [0]
    for r in rows:
        cuts.append(cuts[-1] + len(r))
    return b"".join(rows), tuple(cuts)


def cases_d(name: str, nopfac: bool = False) -> List[Case]:
    """haystack borders.  Chunked walk (the batches of a set with a dense table): a border inside a chunk's warm-up, at c0 and
    at c0 + 1; two and three empty haystacks at one border and at a chunk border; an occurrence cut by a border (not
    reported), one flush with it; rows of 1 .. 5 bytes -- ragged and uniform, from device and from host memory.
    Failureless form (it takes batches itself): a 4-byte pattern with room 4 and 3, a tail flush with the border and one
    byte over it, an item with d > room, a short pattern with fewer than 4 bytes left in its ROW while the stream goes on"""
    form, ml, u, big, out = batch_form(name, nopfac), max_len(name), unit(name), longest(name), []
    chunk, warm = pick_chunk(ml), ml - 1
    fill = lambda k: bytes([FILL]) * k
    if form != "failureless":
        rows: List[bytes] = []
        size = lambda: sum(len(r) for r in rows)
        pad_to = lambda x: rows.append(hay_of(x - size(), [(3, u)]) if x - size() >= len(u) + 6 else fill(x - size()))
        pad_to(chunk - warm // 2 - 1)                   # a border inside the warm-up of chunk 1 ...
        rows.append(big[:warm // 2 + 1] + fill(7) + u)  # ... the longest pattern's first bytes in front of c0: cut by nothing, no match
        pad_to(2 * chunk)                               # a border exactly at c0
        rows += [u + fill(3), b"", b"", u]              # two empty haystacks at one border
        pad_to(3 * chunk + 1)                           # a border at c0 + 1
        rows.append(fill(5) + big)                      # flush with the border behind it
        rows += [fill(3) + big[:len(big) // 2], big[len(big) // 2:] + fill(4)]  # an occurrence cut by a border: no match
        pad_to((TILE // chunk + 2) * chunk)             # (in the next bucket of the post stage)
        rows += [b"", b"", b""]                         # three empty haystacks at a chunk border
        rows += [(u + fill(5))[:k] for k in range(1, 6)]  # rows of 1 .. 5 bytes
        rows += [u, fill(2) + u + fill(chunk)]
        hay, cuts = batch_of(rows)
        out.append(Case("d", name, "ragged", form, hay, cuts=cuts, residues=(0, 5), host_too=True,
                        claim=(("border_in_warmup", chunk), ("border_at", 2 * chunk), ("border_at", 3 * chunk + 1), ("empty_run", 2), ("empty_run_at_chunk_border", 3),
                               ("cut", big))))
        for L in (chunk, chunk + 1, chunk // 2 + 1, 5):  # uniform rows: borders at c0, drifting through the chunks, inside the warm-up
            k = max(6, 3 * chunk // L)
            us = fits(name, L)
            every = max(3, k // 6)  # (few enough for a bucket of the post stage)
            rs = [hay_of(L, ([(0, us)] if i % every == 0 and us else []) + ([(L - len(big), big)] if i % every == 1 and len(big) + len(us) <= L else []))
                  for i in range(k)]
            if len(big) <= 2 * L - 2:                    # cut by a border
                half = len(big) // 2
                rs[-2] = rs[-2][:L - half] + big[:half]
                rs[-1] = big[half:][:L] + rs[-1][len(big) - half:]
            hay, cuts = batch_of(rs)
            out.append(Case("d", name, f"uniform_{L}", form, hay, cuts=cuts, uniform=L, residues=(0, 9), host_too=True, claim=(("rows", k),)))
        return out
    # ---- the failureless form
    uniq = tuple(dict.fromkeys(patterns(name)))
    short = [p for p in uniq if len(p) <= 3]
    four = [p for p in uniq if len(p) == 4]
    tails = [p for p in uniq if 5 <= len(p) <= 12]
    longs = [p for p in uniq if len(p) >= 14]
    rows = [fill(40) + u + fill(9)]
    claim = []
    for p in four:
        rows += [fill(11) + p, fill(11) + p[:3], p[3:] + fill(6)]  # room 4: reported; room 3: its last byte is the next row's
        claim.append(("room4", p))
    for p in tails:
        rows += [fill(9) + p, fill(9) + p[:-1], p[-1:] + fill(5)]  # a tail flush with the border, and one byte over it
        claim.append(("tail_flush", p))
    for p in longs:
        rows += [fill(3) + p, fill(3) + p[:-1], p[-1:] + fill(5), fill(2) + p[:3], p[3:] + fill(2)]  # ... the last: d = 4 > room = 3
        claim.append(("d_over_room", p))
    for p in short:
        rows += [fill(6) + p, fill(6) + p[:-1] if len(p) > 1 else fill(6), fill(4) + p + fill(len(p) % 3)]  # fewer than 4 bytes left in the ROW
        claim.append(("short_at_row_end", p))
    rows += [b"", b"", u, b"", b"", b"", u[:2], u[2:], fill(TILE) + u]  # two and three empty haystacks at one border
    hay, cuts = batch_of(rows)
    out.append(Case("d", name, "ragged", form, hay, cuts=cuts, residues=(0, 5), host_too=True, claim=tuple(claim) + (("empty_run", 2), ("empty_run", 3))))
    for L in (3, 4, 5, 16, 21):
        k = 5000 // L
        p = (four + tails + [u])[0]
        every = max(4, 1200 // L)  # (few enough for a bucket of the post stage, copies counted)
        rs = [hay_of(L, [(L - len(p), p)] if i % every == 1 and len(p) <= L else [(0, short[0])] if short and i % every == 2 else [])
              for i in range(k)]
        if len(p) <= 2 * L - 2:
            rs[-2] = rs[-2][:L - 2] + p[:2]
            rs[-1] = (p[2:] + fill(L))[:L]
        hay, cuts = batch_of(rs)
        out.append(Case("d", name, f"uniform_{L}", form, hay, cuts=cuts, uniform=L, residues=(0, 9), host_too=True, claim=(("rows", k),)))
    return out


E_TILES = (0, 1, 15, 16, 17)


def near_misses(p: bytes) -> List[bytes]:
    """p with one byte below depth 4 replaced by its neighbour in the alphabet (a used byte: its class is its own)"""
    return [p[:k] + bytes([p[k] - 1 if p[k] == ord("z") else p[k] + 1]) + p[k + 1:] for k in range(4, len(p))]


def cases_e() -> List[Case]:
    """stage G and the walk of the failureless form: every pattern of fltail with a near miss in each byte below depth 4;
    63, 64, 65 stage-G hits in one tile, 60 stage-G hits and 3, 4, 5 that k1a_walk appends with atomics, in tiles 0, 1, 15, 16,
    17 and the stream's partial last tile; flmany's copies.  EVERY one of the tile cases leaves the sparse path, the 63-hit
    one too: their occurrences lie in ONE bucket of the post stage, which stages BUCKET of them (above) -- the scan's
    `slot < HIT_SLOTS` keeps the 65th hit inside the tile's slots, and the dense path gives the answer"""
    out = []
    plants, x = [], 7
    for p in TAILS + (OWN4_LONG, OWN4):
        for q in [p] + near_misses(p):
            plants.append((x, q))
            x += len(q) + 3
    out.append(Case("e", "fltail", "near_misses", "failureless", hay_of(x + 50, plants), residues=(0, 7),
                    claim=(("occurrences", len(TAILS) + 3), ("hits_max", HIT_SLOTS))))
    g, w = TAILS[1], TAILS[7]  # 5 bytes: settled by stage G; 20 bytes: an item, k1a_walk's hit
    for t in E_TILES + (-1,):
        tiles = (t if t >= 0 else 3) + 2
        n = tiles * TILE - (0 if t >= 0 else TILE - 700)
        base = (t if t >= 0 else tiles - 1) * TILE + 9
        for ng, nw in ((63, 0), (64, 0), (65, 0), (60, 3), (60, 4), (60, 5)):
            ps = [(base + 8 * i, g) for i in range(ng)] + [(base + 8 * ng + 24 * i, w) for i in range(nw)]
            assert ps[-1][0] + len(ps[-1][1]) <= min(n, (base // TILE + 1) * TILE)
            out.append(Case("e", "fltail", f"tile{t}_{ng}+{nw}", "failureless", hay_of(n, ps + ([(n - 30, OWN4_LONG)] if t >= 0 else [])), fresh=True,
                            leaves=True, claim=(("tile_hits", base // TILE, ng, nw),)))
    plants, x = [], 5
    for p in (b"manyx", b"duplicate", b"four", b"manyx"[:4], b"duplicat", b"fourfour", b"qwert"):
        plants.append((x, p))
        x += len(p) + 2
    out.append(Case("e", "flmany", "copies", "failureless", hay_of(x + 20, plants), residues=(0, 3), claim=(("occurrences", 13),)))
    return out


def cases_f(cus: int) -> List[Case]:
    """the region capacity of k1a_scan: a stretch of r bytes 'a' under ('a' * 17 + 'b') leaves r - 4 items and no hit (the
    pattern itself, 20 bytes in front of the end, three more: the positions up to last_start), all
    of ONE wave's region in a one-tile haystack: cap - 1, cap, cap + 1 items for the sparse capacity (the third leaves the
    sparse path) and for the dense one (cap + 1: the dense attempt gives up too and the chunked walk answers), and 300 items
    (more than a workgroup of k1a_walk: i += blockDim.x)"""
    n = TILE - 40
    cs, cd = pfac_region_cap(n, pfac_scan_grid(0, n, cus), False), pfac_region_cap(n, pfac_scan_grid(0, n, cus), True)
    assert 256 < cs < cd and cd + 1 + 4 + 30 <= n
    out = []
    for items in (300, cs - 1, cs, cs + 1, cd - 1, cd, cd + 1):
        hay = hay_of(n, [(10, b"a" * (items - 3 + 4)), (n - 20, CAP_PAT)])
        out.append(Case("f", "flcap", f"items_{items}", "failureless", hay, fresh=True, leaves=items > cs,
                        claim=(("items", items), ("cap", cs, cd))))
    return out


# ---------------------------------------------------------------------------
# (g) wave turns of the failureless form
# ---------------------------------------------------------------------------
G_SET = "fltail"
G_SHAPES = ("w-1", "w", "w+1", "counts")


def turn_tiles(cus: int) -> Dict[str, int]:
    """W = 16 * CUs waves: one tile fewer than waves, a tile a wave, the first wave's second turn; 16 W + W / 2 + 1: the
    smallest shape at which a wave stores a full batch of 16 tile counts ((kG & 15) == 15) with an epilogue behind it"""
    w = 16 * cus
    return {"w-1": w - 1, "w": w, "w+1": w + 1, "counts": 16 * w + w // 2 + 1}


PRIMER_SHIFT = 40


def turn_case(tiles: int, shift: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """(`tiles` tiles of the filler, the last one partial; the expected rows): one plant per tile at an offset that walks
    through the tile and one across every 16th tile border, TAILS in turn -- lengths 4 .. 12 are stage G's hits, 13 .. 21
    items of k1a_walk.  The plants are disjoint and hold no other pattern, so the rows are the plants under every kind,
    by position (test_k1a_seams_cpu.py pins them against the oracle at 2 CUs).  shift = PRIMER_SHIFT: every plant that many
    bytes further on -- the haystack run_turn() searches FIRST on every handle, so that the hit slots and counts the scan
    does not write this time hold another call's valid records, not fresh memory's zeroes"""
    n = (tiles - 1) * TILE + 1234
    hay = np.full(n, FILL, dtype=np.uint8)
    t = np.arange(tiles, dtype=np.int64)
    start = t * TILE + 64 + (t * 37) % np.where(t == tiles - 1, 1100, TILE - 160)  # (the last tile: 1 234 bytes)
    pid = t % len(TAILS)
    bd = np.arange(16 * TILE, n - 32, 16 * TILE, dtype=np.int64)
    k = np.arange(len(bd), dtype=np.int64)
    bpid = (k + 3) % len(TAILS)
    lens = np.array([len(p) for p in TAILS], np.int64)
    start = np.concatenate([start, bd - 1 - k % (lens[bpid] - 1)]) + shift
    pid = np.concatenate([pid, bpid])
    ok = start + lens[pid] <= n
    start, pid = start[ok], pid[ok]
    for j, p in enumerate(TAILS):
        at = start[pid == j]
        for x, b in enumerate(p):
            hay[at + x] = b
    order = np.argsort(start, kind="stable")
    rows = np.stack([pid[order], start[order], start[order] + lens[pid[order]]], 1).astype(np.uint64)
    assert (rows[1:, 1] > rows[:-1, 2]).all()
    return hay, rows


def run_turn(tiles: int, kinds=None) -> Dict:
    """the (g) shape on the hit-slot sink, device memory, element-wise against the plants; sparse == the calls"""
    from ahocorasick_rs_amd import capi
    fails, calls, autos = [], 0, {}
    for shift in (PRIMER_SHIFT, 0):  # (the primer on every handle first: docstring of turn_case())
        hay, want = turn_case(tiles, shift)
        dev = capi.DeviceBuffer(len(hay) + 16)
        dev.upload(np.concatenate([hay, np.zeros(16, np.uint8)]))
        for mk, ov in (kinds or KINDS):
            if mk not in autos:
                autos[mk] = automaton(G_SET, mk)
            r = autos[mk].find_device(dev.ptr, len(hay), overlapping=ov)
            got = cols(r.matches())
            r.free()
            calls += 1
            if not np.array_equal(got, want):
                k = next((j for j in range(min(len(got), len(want))) if not np.array_equal(got[j], want[j])), min(len(got), len(want)))
                fails.append(f"{tiles} tiles shift {shift} kind {mk} overlapping {ov}: {len(got)} rows against {len(want)}, first difference at row {k}")
        dev.free()
    for mk, a in autos.items():
        why = check_stats(a.path_stats(), "slots", 2 * sum(1 for m, _ in (kinds or KINDS) if m == mk), 0)
        a.close()
        if why:
            fails.append(f"{tiles} tiles kind {mk}: {why}")
    return {"cls": "g", "form": "failureless", "sink": "slots", "calls": calls, "n_fails": len(fails), "fails": fails[:40]}


A_SETS = FL_SETS + ("fl32", "w16", "w16len17", "w16len34", "w16max", "w16over", "ch3fff", "chnfa")
B16_SETS = ("fl32", "w16", "w16len17", "w16len18", "w16len33", "w16len34")
BCH_SETS = ("w16", "w16len17", "w16len34", "w16over", "ch3fff", "chnfa")
C_SETS = ("w16", "w16max", "w16over", "ch3fff")
D_SETS = ("w16", "w16len34", "w16over", "chnfa", "fltail", "flshort", "flmany")
NOPFAC_SETS = FL_SETS  # the failureless sets' classes (a), (b), (d) on walk16 / chunked
CLASSES = ("a", "b", "c", "d", "e", "f", "g")
# (class, form) pairs that have cases -- one test each per sink; the CPU file holds legs() against them on every CU count,
# so that collecting the GPU file builds no plan
LEGS = (("a", "chunked"), ("a", "chunked_nfa"), ("a", "failureless"), ("a", "walk16"), ("b", "chunked"), ("b", "chunked_nfa"),
        ("b", "walk16"), ("c", "chunked"), ("c", "walk16"), ("d", "chunked"), ("d", "chunked_nfa"), ("d", "failureless"),
        ("e", "failureless"), ("f", "failureless"))
NOPFAC_LEGS = (("a", "walk16"), ("b", "chunked"), ("b", "walk16"), ("d", "chunked"))


@functools.lru_cache(maxsize=None)
def plan(cus: int, nopfac: bool = False) -> Tuple[Case, ...]:
    out: List[Case] = []
    if nopfac:
        for s in NOPFAC_SETS:
            out += cases_a(s, True) + cases_b_walk16(s, cus, True) + cases_b_chunked(s, True) + cases_d(s, True)
        return tuple(out)
    for s in A_SETS:
        out += cases_a(s)
    for s in B16_SETS:
        out += cases_b_walk16(s, cus)
    for s in BCH_SETS:
        out += cases_b_chunked(s)
    for s in C_SETS:
        out += cases_c(s)
    for s in D_SETS:
        out += cases_d(s)
    return tuple(out + cases_e() + cases_f(cus))


def legs(cus: int, nopfac: bool = False) -> List[Tuple[str, str]]:
    """(class, form) pairs that have cases: one test each per sink"""
    return sorted({(c.cls, c.form) for c in plan(cus, nopfac)})


# ---------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle(name: str, mk: int) -> Oracle:
    return Oracle(list(patterns(name)), mk, KIND_DFA)


_want: Dict[tuple, List[np.ndarray]] = {}


def rows_of(c: Case) -> List[bytes]:
    return [c.hay[a:b] for a, b in zip(c.cuts, c.cuts[1:])] if c.cuts else [c.hay]


def expected(c: Case, mk: int, ov: bool) -> List[np.ndarray]:
    """the oracle's rows per haystack of the case (offsets local to the haystack)"""
    key = (c.cls, c.set, c.name, c.form, mk, ov)
    if key not in _want:
        o = oracle(c.set, mk)
        _want[key] = [o.find_raw(np.frombuffer(r, dtype=np.uint8), overlapping=ov).astype(np.uint64).reshape(-1, 3) if r
                      else np.zeros((0, 3), np.uint64) for r in rows_of(c)]
    return _want[key]


# ---------------------------------------------------------------------------
# the device side (imports the library when called)
# ---------------------------------------------------------------------------
GUARD = 0xC3
SINKS = ("slots", "regions")
SINK_ENV = {"slots": {}, "regions": {"ACX_NO_BUCKET": "1"}}


def automaton(name: str, mk: int):
    from ahocorasick_rs_amd import capi
    with with_env({"ACX_DENSE_LIMIT": "0"} if dense_limit0(name) else {}):
        a = capi.Automaton(list(patterns(name)), mk, kernel=capi.KERNEL_DFA_WALK)
    assert a.info.kernel == capi.KERNEL_DFA_WALK
    a.path_stats(reset=True)
    return a


def check_stats(st: Dict[str, int], sink: str, sparse: int, dense: int) -> Optional[str]:
    want = {"k0": 0, "sparse": sparse if sink == "slots" else 0, "hot_calls": 0, "dense_tiles": 0,
            "dense_radix": dense if sink == "slots" else sparse + dense}
    got = {k: st[k] for k in want}
    return None if got == want else f"path_stats {got}, the plan says {want}"


def run_case(a, c: Case, mk: int, ov: bool, codepoints: bool = False) -> Tuple[int, List[str]]:
    """the case at every residue of its pointer between guard bytes (a batch: by uniform_len or by device offsets, and from
    host memory), element-wise against the oracle, counts per haystack.  Returns (device calls, what differed)"""
    from ahocorasick_rs_amd import capi
    want = expected(c, mk, ov)
    arr = np.frombuffer(c.hay, dtype=np.uint8)
    if codepoints:
        want = [np.stack([w[:, 0], code_points_at(arr, w[:, 1]), code_points_at(arr, w[:, 2])], 1) if len(w) else w for w in want]
    flat = np.concatenate(want) if len(want) > 1 else want[0]
    counts = np.array([len(w) for w in want], np.uint64)
    n, calls, bad = len(arr), 0, []
    tag = f"{c.set}/{c.cls}/{c.name} kind {mk} overlapping {ov}"
    for res in c.residues:
        buf = np.full(16 + res + n + 48, GUARD, np.uint8)
        buf[16 + res:16 + res + n] = arr
        dev = capi.DeviceBuffer(len(buf))
        dev.upload(buf)
        assert dev.ptr % 16 == 0
        forms = [("uniform" if c.uniform else "offsets")] + (["offsets"] if c.uniform else []) if c.cuts else ["one"]
        for how in forms:
            off = None
            if how == "one":
                r = a.find_device(dev.ptr + 16 + res, n, overlapping=ov, codepoints=codepoints)
            elif how == "uniform":
                r = a.find_device(dev.ptr + 16 + res, n, n_hay=len(c.cuts) - 1, uniform_len=c.uniform, overlapping=ov)
            else:
                off = capi.DeviceBuffer(8 * len(c.cuts))
                off.upload(np.array(c.cuts, np.uint64).view(np.uint8))
                r = a.find_device(dev.ptr + 16 + res, n, d_offsets=off.ptr, n_hay=len(c.cuts) - 1, overlapping=ov)
            got = cols(r.matches())
            gc = r.counts() if c.cuts else counts
            r.free()
            if off is not None:
                off.free()
            calls += 1
            if not np.array_equal(got, flat) or not np.array_equal(np.asarray(gc, np.uint64), counts):
                k = next((j for j in range(min(len(got), len(flat))) if not np.array_equal(got[j], flat[j])), min(len(got), len(flat)))
                bad.append(f"{tag} residue {res} {how}: {len(got)} rows against {len(flat)}, first difference at row {k}")
        if not np.array_equal(dev.download(), buf):
            bad.append(f"{tag} residue {res}: the buffer was written to")
        dev.free()
    if c.host_too:
        m, gc = a.find_batch(rows_of(c), overlapping=ov)
        calls += 1
        if not np.array_equal(cols(m), flat) or not np.array_equal(np.asarray(gc, np.uint64), counts):
            bad.append(f"{tag} from host memory: {len(m)} rows against {len(flat)}")
    elif not c.cuts and not c.fresh and c.residues == RES4 and c.name.startswith("len_"):
        got = cols(a.find(c.hay, overlapping=ov, codepoints=codepoints))  # the host route of a single haystack
        calls += 1
        if not np.array_equal(got, flat):
            bad.append(f"{tag} from host memory: {len(got)} rows against {len(flat)}")
    return calls, bad


def run_leg(cases: Tuple[Case, ...], cls: str, form: str, sink: str) -> Dict:
    """every case of (class, form) under all four kinds on one sink: ONE handle per set and match kind (the overlapping
    calls first), a handle of its own for every path-asserting call; path_stats exact per handle"""
    mine = [c for c in cases if (c.cls, c.form) == (cls, form)]
    fails: List[str] = []
    calls = 0
    with with_env(SINK_ENV[sink]):
        for name in dict.fromkeys(c.set for c in mine):
            for mk in (0, 1, 2):
                a, made = automaton(name, mk), 0
                for ov in ((True, False) if mk == 0 else (False,)):
                    for c in mine:
                        if c.set != name:
                            continue
                        if c.fresh:
                            b = automaton(name, mk)
                            k, bad = run_case(b, c, mk, ov)
                            why = check_stats(b.path_stats(), sink, 0 if c.leaves else k, k if c.leaves else 0)
                            b.close()
                            fails += bad + ([f"{name}/{cls}/{c.name} kind {mk} overlapping {ov}: {why}"] if why else [])
                        else:
                            k, bad = run_case(a, c, mk, ov)
                            made += k
                            fails += bad
                        calls += k
                why = check_stats(a.path_stats(), sink, made, 0)
                a.close()
                if why:
                    fails.append(f"{name}/{cls} kind {mk}: {why}")
    return {"cls": cls, "form": form, "sink": sink, "calls": calls, "n_fails": len(fails), "fails": fails[:40]}


def run_codepoints(cases: Tuple[Case, ...], name: str) -> List[str]:
    """class (a) of one set with codepoints=True at residues 0 and 7 (the guard byte is a lead byte: counted wherever it is read)"""
    fails = []
    for mk, ov in KINDS:
        a = automaton(name, mk)
        for c in cases:
            if (c.cls, c.set) == ("a", name) and c.name.startswith(("len_", "flush_")):
                fails += run_case(a, c._replace(residues=(0, 7)), mk, ov, codepoints=True)[1]
        a.close()
    return fails[:40]


def run_python_classes(cases: Tuple[Case, ...], name: str) -> List[str]:
    """class (a) of one set through BytesAhoCorasick and AhoCorasick built under ACX_KERNEL=dfa_walk"""
    import ahocorasick_rs_amd as ac
    kinds = {0: ac.MatchKind.Standard, 1: ac.MatchKind.LeftmostFirst, 2: ac.MatchKind.LeftmostLongest}
    fails = []
    for mk, ov in KINDS:
        with with_env({"ACX_KERNEL": "dfa_walk"}):
            b = ac.BytesAhoCorasick(list(patterns(name)), matchkind=kinds[mk])
            t = ac.AhoCorasick([p.decode() for p in patterns(name)], matchkind=kinds[mk])
        for c in cases:
            if (c.cls, c.set) != ("a", name) or not c.name.startswith(("len_", "flush_")):
                continue
            rows = [tuple(int(v) for v in r) for r in expected(c, mk, ov)[0]]
            if b.find_matches_as_indexes(c.hay, overlapping=ov) != rows:
                fails.append(f"{name}/{c.name} kind {mk} overlapping {ov}: BytesAhoCorasick")
            if t.find_matches_as_indexes(c.hay.decode(), overlapping=ov) != rows:  # (ASCII: code points are bytes)
                fails.append(f"{name}/{c.name} kind {mk} overlapping {ov}: AhoCorasick")
    return fails[:40]


def child_main(cus: int):
    """the ACX_NO_PFAC child: the failureless sets' classes (a), (b), (d) on walk16 / chunked, both sinks: a line per leg"""
    assert os.environ.get("ACX_NO_PFAC")
    cases = plan(cus, True)
    for cls, form in legs(cus, True):
        for sink in SINKS:
            print("LEG " + json.dumps(run_leg(cases, cls, form, sink)), flush=True)
    print("DONE", flush=True)


if __name__ == "__main__":
    child_main(int(sys.argv[1]))
