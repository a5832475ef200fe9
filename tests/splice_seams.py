"""The layer that makes ONE result of several runs of the pipeline -- run_chunked (a haystack in byte ranges: k_cut_point,
k_copy_shifted), run_batch_split (a batch in two parts: k_rebase_offsets), expand_copies / expand_copies_host (k_copy_counts,
k_expand_copies, k_expand_counts) and k_localize -- at its seams: the constants and the pinned lines of the sources, a Python
model of the two loops over any find(), the pattern sets, the haystacks and the claims that tests/test_splice_seams_cpu.py
checks on the CPU and tests/test_gpu_splice_seams.py runs on the device.  Needs no GPU (what runs a case imports the library
when called).

Expected rows are the oracle's (tests/oracle_lib.py) over the WHOLE haystack; k1b_seams.brute() / brute_iter() are the second
reference for Standard.  The model restates run_chunked line by line (source_constants() pins every line it restates: a
changed line fails on the CPU, it does not silently move the plan) and gives what the oracle cannot: how many ranges are
searched (path_stats()["byte_ranges"]), which are skipped, and for every range the records of its window, the size of the
cut prefix and the two words k_cut_point leaves.

The cut of a range is by END for an overlapping search and by START for the three kinds that do not overlap: every case
states its kinds, every claim the kinds it holds for.  A case is tiny: max_len 8 admits pieces of 31 bytes.  The filler '-'
is in no pattern.

Classes: (a) the cut of a range -- plants at every border of a haystack in 4 (3) ranges, full and with a short last range;
(b) the carry -- a match of every length from hi - 1 with an occurrence it shadows, chains across a border, the skip;
(c) k_cut_point's own seams -- 1 / 255 / 256 / 257 / 513 records, a prefix of 0 / 1 / 255 / 256 / 257 / all, out[1] on either
side of hi; (d) the copy -- ranges of 85 / 86 / 0 / 171 records, a total of 0; (e) the floor and forcing; (f) halving by
the real trigger; (g) a batch in two parts; (h) k_localize; (i) copies of a string.  No single occurrence covers two borders
of run_chunked (piece > 2 * (max_len - 1) + 16 > max_len): that case exists for the ranks of a sharded haystack only, whose
ranges may be shorter than a pattern, and runs there (sharded_cases())."""
from __future__ import annotations

import functools
import os
import re
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from k1b_seams import CLEAN, GROUP, KINDS, cols, with_env
from oracle_lib import KIND_DFA, Oracle, byte_to_code_point

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ahocorasick_rs_amd", "csrc")
NOV = tuple(k for k in KINDS if not k[1])  # the kinds that do not overlap: cut by START
OV = tuple(k for k in KINDS if k[1])       # cut by END
STD = ((0, False), (0, True))              # copies of a string exist for Standard alone


# ---------------------------------------------------------------------------
# the constants of the sources, and the lines the model restates
# ---------------------------------------------------------------------------
def _lit(line: str) -> str:
    """a line of source as a pattern: the same tokens, any white space"""
    return r"\s*".join(re.escape(t) for t in re.findall(r"[A-Za-z_0-9]+|[^\sA-Za-z_0-9]", line))


def read_source(name: str) -> str:
    return open(os.path.join(CSRC, name)).read()


@functools.lru_cache(maxsize=None)
def source_constants() -> Dict[str, int]:
    return check_sources(read_source)


def check_sources(src: Callable[[str], str]) -> Dict[str, int]:
    """the constants, from sources in which every line the model restates still stands (src: file name -> text)"""
    kern, khpp, pipe, small, common, upload = (src(n) for n in ("kernels.hip", "kernels.hpp", "find_pipeline.cpp", "small_calls.cpp",
                                                                "host_common.hpp", "build_upload.cpp"))
    out: Dict[str, int] = {}
    m = re.search(r"constexpr\s+uint32_t\s+SMALL_MAX_LEN\s*=\s*(\d+)\s*,\s*SMALL_MAX_OCC\s*=\s*(\d+)\s*;", khpp)
    assert m, "SMALL_MAX_LEN / SMALL_MAX_OCC are no longer plain constants of kernels.hpp"
    out["SMALL_MAX_LEN"], out["SMALL_MAX_OCC"] = int(m.group(1)), int(m.group(2))
    m = re.search(r"constexpr\s+uint32_t\s+SMALL_PF_MAX_LEN\s*=\s*(\d+)\s*;", khpp)
    assert m, "SMALL_PF_MAX_LEN is no longer a plain constant of kernels.hpp"
    out["SMALL_PF_MAX_LEN"] = int(m.group(1))
    m = re.search(r"if\s*\(segmented\s*\|\|\s*depth\s*>=\s*(\d+)\s*\|\|\s*piece\s*<=\s*(\d+)\s*\*\s*m\s*\+\s*(\d+)\)\s*"
                  r"return\s+fail\(ACX_ETOOBIG,\s*\"more than 2\^32 occurrences\"\);", pipe)
    assert m, "the floor of a piece is no longer `piece <= 2 * m + 16` with its message"
    out["MAX_DEPTH"], out["FLOOR_MUL"], out["FLOOR_ADD"] = (int(g) for g in m.groups())

    def body_of(text, head, tail, what):
        a = text.find(head)
        b = text.find(tail, a + 1)
        assert 0 <= a < b, f"{what} is no longer where the plan looks for it"
        return text[a:b]

    chunked = body_of(pipe, "int run_chunked(acx_automaton *a, Ctx *x, const uint8_t *d_hay, uint64_t len, int overlapping, int codepoints,\n"
                            "                acx_result **out, uint64_t piece, int depth) {", "\n} // namespace", "run_chunked")
    split = body_of(pipe, "int run_batch_split(acx_automaton *a, Ctx *x, const uint8_t *d_hay, uint64_t len, const Segments &G, int overlapping,\n"
                          "                    int codepoints, acx_result **out, int depth) {", "// One haystack in byte ranges", "run_batch_split")
    find = body_of(pipe, "int run_find(acx_automaton *a, Ctx *x,", "namespace {\n\n// A batch", "run_find")
    cutk = body_of(kern, "__global__ void k_cut_point(", "hipError_t cut_point(", "k_cut_point")
    localize = body_of(kern, "__global__ void k_localize(", "hipError_t localize(", "k_localize")
    limit = body_of(common, "inline uint64_t occ_limit() {", "inline int fail_occ()", "occ_limit")
    for line, text, what in (
            # ---- run_chunked
            ("const uint64_t m = a->host.max_len ? a->host.max_len - 1 : 0;", chunked, "m"),
            ("for (uint64_t lo = 0; lo < len;) {", chunked, "the loop over the ranges"),
            ("const uint64_t hi = std::min(len, lo + piece);", chunked, "hi"),
            ("const bool last = hi == len;", chunked, "last"),
            ("if (overlapping) { a0 = lo > m ? lo - m : 0; a1 = hi; }", chunked, "the overlapping window"),
            ("else { carry = std::max(carry, lo); a0 = carry; a1 = last ? len : std::min(len, hi + m); }", chunked, "the window that does not overlap"),
            ("if (a0 >= hi) { lo = hi; continue; }", chunked, "the skip"),
            ("a->path[8]++;", chunked, "byte_ranges"),
            ("run_find(a, x, d_hay + a0, a1 - a0, Segments{nullptr, 1, 0}, overlapping, 0, &r, piece_opts);", chunked, "a piece's call"),
            ("uint64_t first = 0, n = r->n, last_end = 0;", chunked, "first / n / last_end"),
            ("if (n && ((overlapping && lo > 0) || (!overlapping && !last))) {", chunked, "when a piece is cut"),
            ("hipError_t e = overlapping ? cut_point(r->d_matches, n, true, a0, lo + 1, cut, st)", chunked, "the overlapping cut"),
            (": cut_point(r->d_matches, n, false, a0, hi, cut, st);", chunked, "the cut that does not overlap"),
            ("if (overlapping) first = w.h_pinned[PIN_RANGE_CUT];", chunked, "first"),
            ("else { n = w.h_pinned[PIN_RANGE_CUT]; last_end = w.h_pinned[PIN_RANGE_CUT + 1]; }", chunked, "n / last_end"),
            ("} else if (n && !overlapping) {", chunked, "the last range"),
            ("last_end = len;", chunked, "the last range's last_end"),
            ("if (n > first) {", chunked, "a piece with records"),
            ("pieces.push_back(Piece{r->d_matches, first, n - first, a0});", chunked, "a piece"),
            ("if (!overlapping) carry = std::max(std::max(carry, hi), last_end);", chunked, "the carry update"),
            ("copy_shifted(r->d_matches + at, p.buf + p.first, p.n, p.shift, st)", chunked, "the copy"),
            ("if (!total) return ACX_OK;", chunked, "a total of 0"),
            # ---- run_find
            ("const char *cb = depth == 0 && !segmented ? std::getenv(\"ACX_CHUNK_BYTES\") : nullptr;", find, "depth == 0 && !segmented"),
            ("int rc = forced && len > forced ? TOO_MANY_OCC : body();", find, "forced && len > forced"),
            ("const uint64_t piece = forced && len > forced ? forced : len / 2;", find, "the piece"),
            ("if (segmented && depth < 40) return run_batch_split(a, x, d_hay, len, G, overlapping, codepoints, out, depth + 1);", find, "a batch goes on in two parts"),
            ("return run_chunked(a, x, d_hay, len, overlapping, codepoints, out, piece, depth + 1);", find, "a haystack goes on in ranges"),
            ("if (allow_small && !segmented && small_ok(a, len)) {", find, "K0 first"),
            # ---- run_batch_split
            ("a->path[8]++;", split, "byte_ranges of a split"),
            ("if (n <= 1) return one_haystack(d_hay, len, out);", split, "a batch of one"),
            ("const uint64_t half = n / 2;", split, "half = n / 2"),
            ("cut = half * G.uniform_len;", split, "the uniform cut"),
            ("rebase_offsets(reb, G.offsets + half, n - half + 1, cut, st);", split, "the rebased offsets"),
            ("if (k == 1) return one_haystack(h, hl, r);", split, "k == 1"),
            ("int rc = part(d_hay, cut, G.offsets, half, &ra);", split, "the first part"),
            ("if (rc == ACX_OK) rc = part(d_hay + cut, len - cut, reb, n - half, &rb);", split, "the second part"),
            # ---- the kernels
            ("if (i >= n) return;", cutk, "k_cut_point's first condition"),
            ("const uint64_t v = (by_end ? m[i].end : m[i].start) + shift;", cutk, "k_cut_point's value"),
            ("if (v >= limit) return;", cutk, "k_cut_point's second condition"),
            ("if (i + 1 < n) {", cutk, "k_cut_point's last element"),
            ("if (nx < limit) return;", cutk, "k_cut_point's third condition"),
            ("out[0] = i + 1;", cutk, "out[0]"),
            ("out[1] = m[i].end + shift;", cutk, "out[1]"),
            ("hipError_t e = hipMemsetAsync(out, 0, 16, st);", kern, "the two words' zeros"),
            ("dst[w] = src[w] + (w % 3 ? shift : 0);", kern, "k_copy_shifted"),
            ("if (i < n) dst[i] = src[i] - base;", kern, "k_rebase_offsets"),
            ("k[i] = i < n ? 1 + (uint64_t)xcnt[m[i].pattern] : 0;", kern, "k_copy_counts"),
            ("if (r) o.pattern = xids[xoff[v.pattern] + (r - 1)];", kern, "k_expand_copies"),
            ("counts[h] = offs[incl[h]] - offs[h ? incl[h - 1] : 0];", kern, "k_expand_counts"),
            ("else { h = upper_bound_u64(G.offsets, G.n_hay + 1, s) - 1; base = G.offsets[h]; }", localize, "k_localize's haystack"),
            ("if (G.uniform_len) { h = s / G.uniform_len; base = h * G.uniform_len; }", localize, "k_localize's uniform haystack"),
            # ---- the expansion, the switches, who takes a small call
            ("if (total == n) return done(ACX_OK);", pipe, "expand_copies' early return"),
            ("for (uint64_t i = 0; i < *n; i++) total += 1 + a->x_cnt[src[i].pattern];", pipe, "expand_copies_host"),
            ("a->expand_ov = xe ? std::atoi(xe) != 0 : n_later * 4 >= (uint64_t)H.n_patterns;", upload, "n_later * 4 >= n_patterns"),
            ("const char *xe = std::getenv(\"ACX_EXPAND_COPIES\");", upload, "ACX_EXPAND_COPIES, read at build"),
            ("const char *e = std::getenv(\"ACX_MAX_OCC\");", limit, "ACX_MAX_OCC, read per call"),
            ("return !off && !a->kernel_forced && len > 0 && a->host.n_patterns > 0 &&", small, "a forced kernel turns K0 off")):
        assert re.search(_lit(line), text), f"the sources no longer define {what} as the plan restates it: {line}"
    assert "static" not in limit, "ACX_MAX_OCC is no longer read per call"
    # the hot pipeline reads the limit only where it sizes an output the context's buffer has no room for: more hot groups
    # than HOT_INLINE
    attempts = src("find_attempts.cpp")
    m = re.search(r"constexpr\s+uint64_t\s+HOT_INLINE\s*=\s*(\d+)\s*,", attempts)
    assert m and re.search(_lit("if (bound > w.final_cap && c.out == w.final) {"), attempts) and \
        re.search(r"uint64_t\s+hot_inline\s*=\s*%s\s*;" % m.group(1), src("workspace.hpp")), "the hot pipeline's limit is no longer read where the plan believes"
    out["HOT_INLINE"] = int(m.group(1))
    return out


C = source_constants()
SMALL_MAX_LEN, SMALL_PF_MAX_LEN, SMALL_MAX_OCC = C["SMALL_MAX_LEN"], C["SMALL_PF_MAX_LEN"], C["SMALL_MAX_OCC"]


def floor_of(m: int) -> int:
    """the longest piece run_find refuses"""
    return C["FLOOR_MUL"] * m + C["FLOOR_ADD"]


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
class TooBig(Exception):
    """ACX_ETOOBIG: a piece at the floor, or the depth"""


class Range(NamedTuple):
    lo: int
    hi: int
    a0: int
    a1: int
    skipped: bool
    n: int                    # the records of the window (0 when skipped)
    cut: Optional[Tuple[int, int]]  # what k_cut_point left in its two words; None: it did not run
    kept: np.ndarray          # the rows this range contributes, global offsets
    dropped: np.ndarray       # the rows of the window cut away, global offsets


class Chunked(NamedTuple):
    rows: np.ndarray
    searched: int             # byte_ranges of this level
    skipped: int
    ranges: Tuple[Range, ...]


def cut_point(rows: np.ndarray, by_end: bool, shift: int, limit: int) -> Tuple[int, int]:
    """k_cut_point: every element whose value is below the limit and whose successor's is not (or that is the last)
    writes {index + 1, its end + shift}; nobody else does.  One writer is the kernel's premise: two are the model's error."""
    v = (rows[:, 2] if by_end else rows[:, 1]).astype(np.int64) + shift
    writers = [i for i in range(len(v)) if v[i] < limit and (i + 1 == len(v) or v[i + 1] >= limit)]
    assert len(writers) <= 1, "the records are not ordered by the field they are cut by"
    if not writers:
        return 0, 0
    i = writers[0]
    return i + 1, int(rows[i, 2]) + shift


def shifted(rows: np.ndarray, by: int) -> np.ndarray:
    out = rows.astype(np.uint64).reshape(-1, 3).copy()
    out[:, 1:] += np.uint64(by)
    return out


def model_chunked(find: Callable[[int, int, bool], np.ndarray], n: int, piece: int, m: int, ov: bool) -> Chunked:
    """run_chunked over find(a, b, overlapping) -> the rows of hay[a:b], offsets local to a"""
    ranges: List[Range] = []
    none = np.zeros((0, 3), np.uint64)
    carry = lo = searched = skipped = 0
    while lo < n:
        hi = min(n, lo + piece)
        last = hi == n
        if ov:
            a0, a1 = (lo - m if lo > m else 0), hi
        else:
            carry = max(carry, lo)
            a0, a1 = carry, (n if last else min(n, hi + m))
        if a0 >= hi:
            ranges.append(Range(lo, hi, a0, a1, True, 0, None, none, none))
            skipped += 1
            lo = hi
            continue
        searched += 1
        rows = find(a0, a1, ov).astype(np.uint64).reshape(-1, 3)
        first, k, last_end, cut = 0, len(rows), 0, None
        if k and ((ov and lo > 0) or (not ov and not last)):
            cut = cut_point(rows, True, a0, lo + 1) if ov else cut_point(rows, False, a0, hi)
            if ov:
                first = cut[0]
            else:
                k, last_end = cut
        elif k and not ov:
            last_end = n
        ranges.append(Range(lo, hi, a0, a1, False, len(rows), cut, shifted(rows[first:k], a0),
                            shifted(np.concatenate([rows[:first], rows[k:]]), a0)))
        if not ov:
            carry = max(carry, hi, last_end)
        lo = hi
    kept = [r.kept for r in ranges]
    return Chunked(np.concatenate(kept) if kept else none, searched, skipped, tuple(ranges))


class Tree:
    """run_find's recursion when a pass answers TOO_MANY_OCC: `too_many(rows)` says when.  ranges: what byte_ranges counts."""

    def __init__(self, find, m: int, too_many: Callable[[int], bool]):
        self.find, self.m, self.too_many = find, m, too_many
        self.ranges = self.splits = 0

    def single(self, a: int, b: int, ov: bool, depth: int = 0, forced: int = 0) -> np.ndarray:
        """one haystack hay[a:b]: its rows, local to a"""
        n = b - a
        cut = bool(forced) and depth == 0 and n > forced
        if not cut:
            rows = self.find(a, b, ov)
            if not self.too_many(len(rows)):
                return rows
        piece = forced if cut else n // 2
        if depth >= C["MAX_DEPTH"] or piece <= floor_of(self.m):
            raise TooBig()
        got = model_chunked(lambda x, y, o: self.counted(a + x, a + y, o, depth + 1), n, piece, self.m, ov)
        return got.rows

    def counted(self, a, b, ov, depth):
        self.ranges += 1
        return self.single(a, b, ov, depth)

    def batch(self, offsets: Sequence[int], ov: bool, depth: int = 0) -> List[Tuple[int, int]]:
        """a batch (offsets of its haystacks, the last one its end): the cuts run_batch_split makes, as (first haystack,
        haystack the cut falls in front of); the rows are the haystacks' own"""
        cuts: List[Tuple[int, int]] = []

        def one(h, depth):
            self.single(offsets[h], offsets[h + 1], ov, depth)

        def part(lo, hi, depth):  # haystacks [lo, hi) as a batch of their own
            total = sum(len(self.find(offsets[h], offsets[h + 1], ov)) for h in range(lo, hi))
            if not self.too_many(total):
                return
            if depth >= C["MAX_DEPTH"]:
                raise TooBig()
            depth += 1
            self.ranges += 1
            self.splits += 1
            if hi - lo <= 1:
                return one(lo, depth)
            half = lo + (hi - lo) // 2
            cuts.append((lo, half))
            for x, y in ((lo, half), (half, hi)):
                if y - x == 1:
                    one(x, depth)
                else:
                    part(x, y, depth)
        part(0, len(offsets) - 1, depth)
        return cuts


# ---------------------------------------------------------------------------
# pattern sets
# ---------------------------------------------------------------------------
L8 = b"abcdefgh"
L40 = b"ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789!@#$"
LONG = bytes(ord("A") + (i * i + 3 * i + i // 7) % 23 for i in range(520))  # letters A .. W: no 'x', no filler
PIECE_C = floor_of(len(LONG) - 1) + 1   # class (c): 1 055 bytes, a prefix of 257 records fits max_len - 1 = 519 bytes
LADDER = (b"1", b"2b", b"3cc", b"4ddd", b"5eeee", b"6fffff", b"7gggggg", b"8hhhhhhh")
SHADOWS = (b"bw", b"cw", b"dw", b"ew", b"fw", b"gw", b"hw")  # each begins on the last byte of a ladder pattern + 'w'


@functools.lru_cache(maxsize=None)
def patterns(set_name: str) -> Tuple[bytes, ...]:
    if set_name == "s8":
        # the longest; nested in it at its front, middle and end; one byte; leftmost-first takes "pq", leftmost-longest
        # "pqrs"; "kzk" / "zkzk": every occurrence begins inside the one before
        return (L8, b"abc", b"def", b"fgh", b"x", b"pq", b"pqrs", b"kzk", b"zkzk")
    if set_name == "s40":  # max_len - 1 = 39 exceeds a short last range
        return (L40, b"ABC", b"STU", b"@#$", b"x", b"pq", b"pqrs", b"kzk", b"zkzk")
    if set_name == "lad":  # a pattern of every length 1 .. 8, and what each must shadow
        return LADDER + SHADOWS
    if set_name == "c":
        return (LONG, b"x")
    if set_name == "u":  # code points: characters of 2, 3 and 4 bytes
        return (b"x", "é☃".encode(), "☃".encode(), L8, "😀a".encode())
    if set_name.startswith("cp"):  # copies: see copy_set()
        return copy_set(set_name)
    raise KeyError(set_name)


def copy_set(name: str) -> Tuple[bytes, ...]:
    """"cp_at": 8 patterns, 2 later copies (n_later * 4 == n_patterns: expanded by itself); "cp_below": 9 patterns, 2 later
    copies (not expanded by itself); "cp_run": "ab" 301 times (a run of 300 copies crosses a block of 256 threads), "cd" twice,
    "zz" and "x" once"""
    if name == "cp_at":
        return (b"ab", b"cd", b"ab", b"zz", b"x", b"ab", b"abcd", b"q")
    if name == "cp_below":
        return (b"ab", b"cd", b"ab", b"zz", b"x", b"ab", b"abcd", b"q", b"r")
    if name == "cp_run":
        return (b"zz", b"ab", b"x", b"cd") + (b"ab",) * 300 + (b"cd",)
    raise KeyError(name)


def max_len(set_name: str) -> int:
    return max(len(p) for p in patterns(set_name))


def pid(set_name: str, p: bytes) -> int:
    return patterns(set_name).index(p)


@functools.lru_cache(maxsize=None)
def oracle(set_name: str, mk: int) -> Oracle:
    return Oracle(list(patterns(set_name)), mk, KIND_DFA)


@functools.lru_cache(maxsize=None)
def expected(set_name: str, hay: bytes, mk: int, ov: bool) -> np.ndarray:
    w = oracle(set_name, mk).find_raw(hay, overlapping=ov).astype(np.uint64).reshape(-1, 3)
    w.setflags(write=False)
    return w


def finder(set_name: str, hay: bytes, mk: int) -> Callable[[int, int, bool], np.ndarray]:
    o = oracle(set_name, mk)
    return lambda a, b, ov: o.find_raw(hay[a:b], overlapping=ov)


def as_code_points(hay: bytes, rows: np.ndarray) -> np.ndarray:
    if not len(rows):
        return rows
    b2c = byte_to_code_point(hay)
    return np.stack([rows[:, 0], b2c[rows[:, 1]], b2c[rows[:, 2]]], 1).astype(np.uint64)


# ---------------------------------------------------------------------------
# cases of one haystack in byte ranges: (a) .. (d)
# ---------------------------------------------------------------------------
class Claim(NamedTuple):
    what: str      # "row" | "start" | "absent" | "skips" | "records" | "prefix" | "out1" | "kept" | "differs" | "restart"
    kinds: tuple   # the kinds it holds for
    args: tuple


class Case(NamedTuple):
    cls: str
    name: str
    set: str
    hay: bytes
    piece: int
    kinds: tuple
    claims: Tuple[Claim, ...]


def plant(n: int, plants: Sequence[Tuple[int, bytes]]) -> bytes:
    a = bytearray([CLEAN]) * n
    for pos, p in plants:
        assert 0 <= pos and pos + len(p) <= n, (pos, len(p), n)
        assert all(c == CLEAN for c in a[pos:pos + len(p)]), ("two plants on one byte", pos)
        a[pos:pos + len(p)] = p
    return bytes(a)


def occ_claims(set_name: str, pos: int, p: bytes) -> Tuple[Claim, ...]:
    """an occurrence of p planted at pos on the filler: the overlapping search reports it as it is, every other kind a
    match that STARTS there (Standard the first of the nested ones to end)"""
    return (Claim("row", OV, (pid(set_name, p), pos, pos + len(p))), Claim("start", NOV, (pos,)))


def border_plants(set_name: str, B: int) -> List[Tuple[str, int, bytes]]:
    """what class (a) plants at a border B, one case each"""
    L = patterns(set_name)[0]
    ll, m = len(L), len(L) - 1
    out = [("Lend-1", B - 1 - ll, L), ("Lend", B - ll, L), ("Lend+1", B + 1 - ll, L),
           ("Lstart-1", B - 1, L), ("Lstart", B, L), ("Lstart-m-1", B - m - 1, L),
           ("x-1", B - 1, b"x"), ("x", B, b"x"),
           # nested: the front one ends before B, the middle one lies across it, the end one behind it
           ("nested", B - (4 if ll == 8 else ll // 2), L)]
    assert B + 1 - ll == B - m  # (the longest pattern starting at B - m IS the one ending at B + 1)
    return out


@functools.lru_cache(maxsize=None)
def cases_a(set_name: str, piece: int, n_ranges: int, tail: int = 0) -> Tuple[Case, ...]:
    """tail: the bytes of a short last range (0: every range is a full piece)"""
    L = patterns(set_name)[0]
    n = piece * n_ranges if not tail else piece * (n_ranges - 1) + tail
    borders = [piece * k for k in range(1, n_ranges)]
    tag = "%s/p%d/r%d%s" % (set_name, piece, n_ranges, "t%d" % tail if tail else "")
    out = []

    def case(name, plants):
        edge = [(0, b"x"), (n - 1, b"x")]  # the first and the last range are never empty
        plants = list(plants) + [e for e in edge if all(e[0] + 1 <= q or q + len(p) <= e[0] for q, p in plants)]
        claims = tuple(c for q, p in plants for c in occ_claims(set_name, q, p))
        out.append(Case("a", "%s/%s" % (tag, name), set_name, plant(n, plants), piece, KINDS, claims))

    for B in borders:
        for name, pos, p in border_plants(set_name, B):
            if pos + len(p) <= n:
                case("B%d/%s" % (B, name), [(pos, p)])
    # lo == 0 and `last` take other branches: the longest pattern on the first byte and up to the last one
    case("first", [(0, L)])
    case("last", [(n - len(L), L)])
    # every border at once, a different plant at each
    every = [border_plants(set_name, B)[(3 * k + 1) % 9] for k, B in enumerate(borders)]
    case("every", [(pos, p) for _, pos, p in every if pos + len(p) <= n])
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cases_b() -> Tuple[Case, ...]:
    out = []
    P, m = 31, 7
    n = 3 * P
    for B in (P, 2 * P):
        for k in range(1, 9):
            lad = LADDER[k - 1]
            if k == 1:  # nothing to shadow: the next range's first byte holds a match that must be reported
                hay = plant(n, [(B - 1, lad), (B, LADDER[1])])
                claims = (Claim("row", NOV, (0, B - 1, B)), Claim("row", NOV, (1, B, B + 2)))
            else:
                hay = plant(n, [(B - 1, lad + b"w")])
                s = B - 1 + k - 1  # where the shadowed occurrence begins: inside the match, at or behind the border
                claims = (Claim("row", NOV, (k - 1, B - 1, B - 1 + k)), Claim("absent", NOV, (s,)), Claim("restart", NOV, (B, s)))
            out.append(Case("b", "lad/B%d/len%d" % (B, k), "lad", hay, P, NOV, claims))
    # chains across a border: what the truncated window shows behind hi is not what is there
    for B in (P, 2 * P):
        for phase in CHAIN_PHASES:
            chain = b"kz" * 14 + b"k"
            hay = plant(n, [(B - 9 + phase, chain)])
            out.append(Case("b", "chain/B%d/ph%d" % (B, phase), "s8", hay, P, NOV, (Claim("differs", NOV, (B // P - 1,)),)))
    # the skip: a last range shorter than the carried match's tail -- and one byte more, which is searched
    out.append(Case("b", "skip/lad", "lad", b"-" * 30 + LADDER[7], P, NOV, (Claim("skips", NOV, (1,)),)))
    out.append(Case("b", "noskip/lad", "lad", b"-" * 30 + LADDER[7] + b"1", P, NOV, (Claim("skips", NOV, (0,)), Claim("row", NOV, (0, 38, 39)))))
    # (Standard reports "abc", "def": its carry is 36, the leftmost kinds' 38)
    left = ((1, False), (2, False))
    out.append(Case("b", "skip/s8", "s8", b"-" * 30 + L8, P, NOV, (Claim("skips", left, (1,)), Claim("skips", ((0, False),), (0,)))))
    out.append(Case("b", "noskip/s8", "s8", b"-" * 30 + L8 + b"x", P, NOV, (Claim("skips", NOV, (0,)), Claim("row", NOV, (4, 38, 39)))))
    # (a match from a range in front never covers a whole range behind it: piece > max_len.  The carry beyond a short last
    # range's end is the only skip there is.)  A carried match that ends INSIDE the next range: searched from there
    out.append(Case("b", "carry_inside/lad", "lad", plant(n, [(P - 1, LADDER[7] + b"w"), (P + 8, LADDER[0])]), P, NOV,
                    (Claim("row", NOV, (7, P - 1, P + 7)), Claim("row", NOV, (0, P + 8, P + 9)), Claim("absent", NOV, (P + 6,)),
                     Claim("restart", NOV, (P, P + 6)))))
    return tuple(out)


# where the chain begins, from B - 9: at these the truncated window ends inside a link under every kind (at 1 and 5 it ends
# where a link ends and shows the truth; the CPU file recomputes the claim)
CHAIN_PHASES = (0, 2, 3, 4)


@functools.lru_cache(maxsize=None)
def cases_c() -> Tuple[Case, ...]:
    """k_cut_point: n records, of which k before the limit.  Overlapping: the window of range 1, [lo - m, len): k 'x' end at
    or before lo (the prefix is CUT AWAY).  Not overlapping: the window of range 0, [0, hi + m): k 'x' start before hi (the
    prefix is KEPT)."""
    out = []
    P, m = PIECE_C, len(LONG) - 1
    n_hay = P + 600
    for n in (1, 255, 256, 257, 513):
        for k in sorted({0, 1, 255, 256, 257, n}):
            if k > n:
                continue
            hay = plant(n_hay, [(P - k, b"x" * k), (P, b"x" * (n - k))])
            for mode, kinds, ridx in (("ov", OV, 1), ("nov", NOV, 0)):
                claims = (Claim("records", kinds, (ridx, n)), Claim("prefix", kinds, (ridx, k)))
                out.append(Case("c", "%s/n%d/k%d" % (mode, n, k), "c", hay, P, kinds, claims))
    # out[1], the end of the last kept match, is what the carry reads: beyond hi (the longest pattern from hi - 1, 'x'
    # behind its end: range 1 is searched from there) and before hi (the last kept 'x' ends at hi - 4, 'x' behind hi dropped)
    hay = plant(n_hay, [(100, b"x" * 7), (P - 1, LONG), (P - 1 + len(LONG), b"xx"), (n_hay - 9, b"x")])
    out.append(Case("c", "nov/out1_beyond", "c", hay, P, NOV, (Claim("out1", NOV, (0, "beyond")), Claim("row", NOV, (0, P - 1, P - 1 + len(LONG))))))
    hay = plant(n_hay, [(100, b"x" * 7), (P - 5, b"x"), (P + 3, b"xxx"), (n_hay - 9, b"x")])
    out.append(Case("c", "nov/out1_before", "c", hay, P, NOV, (Claim("out1", NOV, (0, "before")), Claim("prefix", NOV, (0, 8)))))
    # ... and the longest pattern across the overlapping cut: ending at lo (the range in front's: it begins one byte before
    # this range's window) and at lo + 1 (this one's: it begins on the window's first byte); nothing is cut away in either
    for d in (0, 1):
        hay = plant(n_hay, [(P + d - len(LONG), LONG), (P + 40, b"x")])
        out.append(Case("c", "ov/long_end_lo+%d" % d, "c", hay, P, OV, (Claim("prefix", OV, (1, 0)), Claim("row", OV, (0, P + d - len(LONG), P + d)))))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cases_d() -> Tuple[Case, ...]:
    """the copy: 3 * n words on either side of 256 and 512 (n = 85 | 86, 170 | 171), a range without records between two
    with some, pattern ids that a shift would change (every row is compared in full), a total of 0"""
    P = 200
    per = (85, 86, 0, 171, 170)
    plants = []
    for r, k in enumerate(per):
        plants.append((r * P + 12, b"x" * k))  # (12 bytes from the border: in no other range's window)
    plants.append((4 * P + 185, L8))
    hay = plant(5 * P, plants)
    # Standard that does not overlap reports "abc", "def" of the longest pattern; every other kind one row
    # the last range: 170 'x' and the longest pattern -- with its three nested ones when overlapping, as "abc", "def" under
    # Standard that does not overlap, as one row under the leftmost kinds
    claims = tuple(Claim("kept", kinds, (per[:4] + (170 + k,),))
                   for kinds, k in ((((0, True),), 4), (((0, False),), 2), (((1, False), (2, False)), 1)))
    return (Case("d", "words", "s8", hay, P, KINDS, claims),
            Case("d", "total0", "s8", b"-" * 100, 31, KINDS, (Claim("kept", KINDS, ((0, 0, 0, 0),)),)))


def cut_cases() -> Tuple[Case, ...]:
    """classes (a) to (d) as run_chunked sees them"""
    return (cases_a("s8", 31, 4) + cases_a("s8", 31, 4, 11) + cases_a("s40", 95, 3) + cases_a("s40", 95, 3, 20) +
            cases_b() + cases_c() + cases_d())


def sharded_cases() -> Tuple[Tuple[Case, int], ...]:
    """(case, world): the (a) and (b) haystacks at lengths whose shard_range borders are the planted ones -- world ranges of
    one piece each -- and the occurrence that covers two borders (40 bytes over ranks of 20)"""
    out = [(c, w) for w in (2, 3, 4, 5) for c in cases_a("s8", 31, w)]
    out += [(c, 3) for c in cases_b() if len(c.hay) == 93]
    two = Case("a", "two_borders", "s40", plant(100, [(15, L40), (70, b"x")]), 20, KINDS, occ_claims("s40", 15, L40))
    return tuple(out) + ((two, 5),)


def model_of(c: Case, mk: int, ov: bool) -> Chunked:
    return model_chunked(finder(c.set, c.hay, mk), len(c.hay), c.piece, max_len(c.set) - 1, ov)


def check_claims(c: Case, mk: int, ov: bool, got: Optional[Chunked] = None) -> List[str]:
    """what of the case's claims does not hold under this kind (computed with the oracle and the model)"""
    got = got or model_of(c, mk, ov)
    want = expected(c.set, c.hay, mk, ov)
    rows = {tuple(int(v) for v in r) for r in want}
    bad = []
    for cl in c.claims:
        if (mk, ov) not in cl.kinds:
            continue
        a = cl.args
        if cl.what == "row":
            ok = tuple(a) in rows
        elif cl.what == "start":
            ok = any(r[1] == a[0] for r in rows)
        elif cl.what == "absent":
            ok = not any(r[1] == a[0] for r in rows)
        elif cl.what == "restart":  # a search that resumes at the border, not at the carry, reports what the match shadows
            ok = any(int(r[1]) + a[0] == a[1] for r in finder(c.set, c.hay, mk)(a[0], len(c.hay), ov))
        elif cl.what == "skips":
            ok = (got.skipped > 0) == bool(a[0]) and got.searched + got.skipped == len(got.ranges)
        elif cl.what == "records":
            ok = got.ranges[a[0]].n == a[1] and got.ranges[a[0]].cut is not None
        elif cl.what == "prefix":
            r = got.ranges[a[0]]
            ok = r.cut is not None and r.cut[0] == a[1] and (a[1] > 0 or r.cut == (0, 0))
        elif cl.what == "out1":
            r = got.ranges[a[0]]
            ok = r.cut is not None and r.cut[0] > 0 and (r.cut[1] > r.hi if a[1] == "beyond" else r.cut[1] < r.hi)
        elif cl.what == "kept":
            ok = tuple(len(r.kept) for r in got.ranges) == tuple(a[0])
        elif cl.what == "differs":
            r = got.ranges[a[0]]
            there = {x for x in rows if r.hi <= x[1] < r.a1}
            ok = len(r.dropped) > 0 and {tuple(int(v) for v in x) for x in r.dropped} != there
        else:
            raise KeyError(cl.what)
        if not ok:
            bad.append("%s kind %d overlapping %s: %s%s does not hold" % (c.name, mk, ov, cl.what, a))
    return bad


# ---------------------------------------------------------------------------
# (e) the floor and forcing
# ---------------------------------------------------------------------------
def floor_cases() -> Tuple[Tuple[str, bytes], ...]:
    """(set, haystack): cut at floor + 1 it gives the oracle's rows, at the floor ACX_ETOOBIG"""
    return (("s8", cases_a("s8", 31, 4)[-1].hay), ("s40", cases_a("s40", 95, 3)[-1].hay))


# ---------------------------------------------------------------------------
# (f) halving by the real trigger
# ---------------------------------------------------------------------------
HOT_GROUPS_MIN = C["HOT_INLINE"] + 1  # hot groups (of GROUP bytes) from which the hot pipeline reads the limit at all
F_LIMIT = 3000        # ACX_MAX_OCC: above SMALL_MAX_OCC, so that a pass K0 answers is never one the limit would have refused
F_BYTES = 256 << 10
F_STRIDE = 32


@functools.lru_cache(maxsize=None)
def dense_input() -> Tuple[Tuple[bytes, ...], bytes]:
    """a pattern every 32 bytes of 256 KiB: 8 192 occurrences, halved twice until the pieces stay under F_LIMIT"""
    import gen
    pats = tuple(gen.gen_patterns(2000, 5, 12, gen.AZ, 1))
    hay = gen.gen_uniform(F_BYTES, gen.AZ, 12).copy()
    rng = gen.SplitMix64(77)
    for k in range(0, len(hay) - F_STRIDE, F_STRIDE):
        p = np.frombuffer(pats[rng.next() % len(pats)], dtype=np.uint8)
        hay[k:k + len(p)] = p
    return pats, hay.tobytes()


def least_ranges(find, n: int, m: int, ov: bool, limit: int) -> int:
    """a LOWER bound of byte_ranges on the dense path: a pass that would report `limit` rows or more cannot be one dense pass
    (both forms count every occurrence, reported or not), so every range the model cuts the library cuts too.  The library
    may cut more: the occurrences a leftmost kind drops, and the prefix hits, count as well.  (The hit slots have no limit
    of their own, and the hot pipeline reads it from HOT_GROUPS_MIN hot groups on.)"""
    t = Tree(find, m, lambda rows: rows >= limit)
    t.single(0, n, ov)
    return t.ranges


# ---------------------------------------------------------------------------
# (g) a batch in two parts, (h) k_localize
# ---------------------------------------------------------------------------
G_LIMIT = 2000  # above SMALL_MAX_OCC
HEAVY = ("x☃é☃-" * 800).encode()          # 2 400 rows (3 200 overlapping) in 8 000 bytes: alone in a part it goes on in byte ranges
MID = b"x" * 1090 + b"-abcdefgh-" + b"x" * 5  # 1 096 rows: one stays under the limit, two do not
LIGHT = ("x-é☃" * 3).encode()


class Batch(NamedTuple):
    cls: str
    name: str
    set: str
    hays: Tuple[bytes, ...]
    uniform: bool
    codepoints: bool


@functools.lru_cache(maxsize=None)
def batches_g() -> Tuple[Batch, ...]:
    out = []
    e = b""
    for n in (1, 2, 3, 4, 5, 9):
        half = n // 2
        out.append(Batch("g", "uniform/n%d" % n, "u", (MID,) * n, True, False))
        ragged = [MID + b"x" * (7 * h) for h in range(n)]
        out.append(Batch("g", "ragged/n%d" % n, "u", tuple(ragged), False, False))
        # one heavy haystack among light ones: alone in a part, at a byte offset that is no multiple of 16
        heavy = [LIGHT + b"-" * h for h in range(n)]
        heavy[min(n - 1, half)] = HEAVY
        out.append(Batch("g", "heavy/n%d" % n, "u", tuple(heavy), False, False))
        out.append(Batch("g", "heavy_cp/n%d" % n, "u", tuple(heavy), False, True))
        if n >= 3:
            for at in sorted({half - 1, half, half + 1}):
                if 0 <= at < n:
                    hs = list(ragged)
                    hs[at] = e
                    out.append(Batch("g", "empty@%d/n%d" % (at, n), "u", tuple(hs), False, False))
    out.append(Batch("g", "empties_front_end/n9", "u", (e, e, e) + (MID,) * 3 + (e, e, e), False, False))
    out.append(Batch("g", "all_empty/n5", "u", (e,) * 5, False, False))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def batches_h() -> Tuple[Batch, ...]:
    """no limit is lowered: one pass, k_localize alone"""
    e = b""
    u = lambda s: s.encode()  # noqa: E731
    return (
        Batch("h", "first_and_last_byte", "s8", (L8, b"x", L8 + L8, b"x-x", b"abc"), False, False),
        Batch("h", "split_across_two", "s8", (b"--abcd", b"efgh--", b"ab", b"c", b"x"), False, False),
        Batch("h", "empties_around", "s8", (e, e, L8, e, b"x", e, e, b"-abc", e), False, False),
        Batch("h", "uniform1", "s8", (b"x", b"-", b"x", b"a", b"b", b"c", b"x"), True, False),
        Batch("h", "uniform_max_len", "s8", (L8, b"-bcdefgh", L8, b"abcdefg-", b"xxxxxxxx"), True, False),
        Batch("h", "uniform13", "s8", (b"abcdefgh--x--", b"-----abcdefgh", b"x-----------x", b"fghabcdefghab", b"efgh---abcdef"), True, False),
        Batch("h", "behind_2_3_4_bytes", "u", (u("xé"), u("x-é☃"), u("☃"), u("x"), u("x😀"), u("x-😀a"), u("é☃x")), False, True),
        Batch("h", "behind_2_3_4_bytes_uniform", "u", (u("xx--é"), u("xé☃"), u("--x☃"), u("x-x-x-"), u("xx😀"), u("xabcd-")), True, True))


def batch_offsets(b: Batch) -> List[int]:
    off = [0]
    for h in b.hays:
        off.append(off[-1] + len(h))
    return off


def batch_expected(b: Batch, mk: int, ov: bool) -> List[np.ndarray]:
    per = [expected(b.set, h, mk, ov) for h in b.hays]
    return [as_code_points(h, r) for h, r in zip(b.hays, per)] if b.codepoints else per


def batch_tree(b: Batch, mk: int, ov: bool, limit: int) -> Tuple[List[Tuple[int, int]], Tree]:
    blob = b"".join(b.hays)
    t = Tree(finder(b.set, blob, mk), max_len(b.set) - 1, lambda rows: rows >= limit)
    return t.batch(batch_offsets(b), ov), t


# ---------------------------------------------------------------------------
# (i) copies of a string (Standard, overlapping)
# ---------------------------------------------------------------------------
class CopyCase(NamedTuple):
    name: str
    set: str
    hay: bytes
    claims: tuple  # "first", "last": the result's first / last record carries copies; "run300"; "n1"; "none"; "zero_next_to_many"


@functools.lru_cache(maxsize=None)
def copy_cases() -> Tuple[CopyCase, ...]:
    out = []
    for s in ("cp_at", "cp_below"):
        out.append(CopyCase(s + "/mixed", s, b"ab-zz-abcd-q-cd-x-ab", ("first", "last", "zero_next_to_many")))
        out.append(CopyCase(s + "/n1", s, b"----ab----", ("n1", "first", "last")))
        out.append(CopyCase(s + "/none", s, b"zz-x-q-zz--x", ("none",)))
    out.append(CopyCase("cp_run/run300", "cp_run", b"zz-ab-x-zzab-cd", ("run300", "zero_next_to_many", "last")))
    out.append(CopyCase("cp_run/first", "cp_run", b"ab-x", ("run300", "first")))
    out.append(CopyCase("cp_run/none", "cp_run", b"zz-x-zz", ("none",)))
    return tuple(out)


def copy_batches() -> Tuple[Batch, ...]:
    e = b""
    return (Batch("i", "cp_at/between", "cp_at", (b"ab", e, b"----", b"zz-ab-cd", e, e, b"x", b"abcd"), False, False),
            Batch("i", "cp_run/between", "cp_run", (e, b"ab-ab", b"---", e, b"zz", b"cd-ab", e), False, False),
            Batch("i", "cp_at/uniform", "cp_at", (b"ab--", b"----", b"zzab", b"abcd", b"-x--"), True, False))


def copy_range_cases() -> Tuple[Case, ...]:
    """in byte ranges: a run of copies that ends at lo (the range in front's, whole) and one that ends at lo + 1 (this
    range's, whole); cp_run: max_len 2, pieces from 19 bytes"""
    P = floor_of(max_len("cp_run") - 1) + 1
    n = 3 * P
    out = []
    for d in (0, 1):
        hay = plant(n, [(P + d - 2, b"ab"), (2 * P + d - 2, b"cd"), (3, b"x")])
        out.append(Case("i", "ranges/end_lo+%d" % d, "cp_run", hay, P, ((0, True),),
                        (Claim("kept", ((0, True),), ((1 + 301 * (1 - d), 301 * d + 2 * (1 - d), 2 * d),)),)))
    return tuple(out)


def copies_of(set_name: str) -> Dict[int, int]:
    """lowest id of a string -> its later copies"""
    seen: Dict[bytes, int] = {}
    out: Dict[int, int] = {}
    for i, p in enumerate(patterns(set_name)):
        if p in seen:
            out[seen[p]] = out.get(seen[p], 0) + 1
        else:
            seen[p] = i
    return out


def n_later(set_name: str) -> int:
    return sum(copies_of(set_name).values())


# ---------------------------------------------------------------------------
# the device side (imports the library when called)
# ---------------------------------------------------------------------------
ENGINES = ("k0", "walk", "prefilter")
RESIDUES = (0, 1, 15)
HOST_PIECE = 13111  # the host route: five ranges of a haystack beyond K0's reach (SMALL_PF_MAX_LEN), each within it


def automaton(set_name: str, mk: int, engine: str = "k0", pats=None):
    from ahocorasick_rs_amd import capi
    kernel = {"k0": None, "walk": capi.KERNEL_DFA_WALK, "prefilter": capi.KERNEL_PREFILTER}[engine]
    return capi.Automaton(list(pats if pats is not None else patterns(set_name)), mk, kernel=kernel)


class Handles:
    """one automaton per (set, kind) of an engine"""

    def __init__(self, engine: str = "k0"):
        self.engine, self.autos = engine, {}

    def get(self, set_name: str, mk: int):
        if (set_name, mk) not in self.autos:
            self.autos[(set_name, mk)] = automaton(set_name, mk, self.engine)
        return self.autos[(set_name, mk)]

    def close(self):
        for a in self.autos.values():
            a.close()
        self.autos = {}


def on_device(front: int, hay: bytes):
    """hay at pointer residue `front`, 16 zero bytes behind it"""
    from ahocorasick_rs_amd import capi
    buf = capi.DeviceBuffer(front + len(hay) + 16)
    buf.upload(np.frombuffer(b"\xff" * front + hay + b"\0" * 16, dtype=np.uint8))
    assert buf.ptr % 16 == 0
    return buf


def ordered(kinds) -> list:
    """the overlapping kind first"""
    return sorted(kinds, key=lambda k: (not k[1], k[0]))


def cut_call(a, ptr: int, n: int, ov: bool, piece: int, codepoints: bool = False):
    """one find_device under ACX_CHUNK_BYTES: (rows, path_stats)"""
    with with_env({"ACX_CHUNK_BYTES": str(piece)}):
        a.path_stats(reset=True)
        r = a.find_device(ptr, n, overlapping=ov, codepoints=codepoints)
        got = cols(r.matches())
        r.free()
        return got, a.path_stats(reset=True)


def diff(got: np.ndarray, want: np.ndarray) -> Optional[str]:
    if got.shape == want.shape and np.array_equal(got, want):
        return None
    k = next((i for i in range(min(len(got), len(want))) if not np.array_equal(got[i], want[i])), min(len(got), len(want)))
    return "%d rows against %d, first difference at row %d: %s against %s" % (
        len(got), len(want), k, got[k].tolist() if k < len(got) else None, want[k].tolist() if k < len(want) else None)


def run_cut_cases(cases: Sequence[Case], engine: str, residues=RESIDUES) -> Tuple[int, List[str]]:
    """every case under every kind of its own at every residue: rows, byte_ranges and the engine, element-wise"""
    H = Handles(engine)
    fails: List[str] = []
    calls = 0
    try:
        for c in cases:
            for front in residues:
                buf = on_device(front, c.hay)
                for mk, ov in ordered(c.kinds):
                    model = model_of(c, mk, ov)
                    got, st = cut_call(H.get(c.set, mk), buf.ptr + front, len(c.hay), ov, c.piece)
                    calls += 1
                    why = diff(got, expected(c.set, c.hay, mk, ov))
                    if why is None and st["byte_ranges"] != model.searched:
                        why = "byte_ranges %d against the model's %d" % (st["byte_ranges"], model.searched)
                    if why is None and st["k0"] != (model.searched if engine == "k0" else 0):
                        why = "k0 %d of %d ranges on engine %s" % (st["k0"], model.searched, engine)
                    if why:
                        fails.append("%s kind %d overlapping %s residue %d: %s" % (c.name, mk, ov, front, why))
                buf.free()
    finally:
        H.close()
    return calls, fails


def host_haystacks() -> Tuple[Case, ...]:
    """classes (a) and (b) on the host route: 5 ranges of HOST_PIECE bytes -- a haystack beyond K0's reach whose pieces are
    K0's --, a different plant at every border"""
    P = HOST_PIECE
    n = 5 * P
    borders = (P, 2 * P, 3 * P, 4 * P)
    assert n > SMALL_PF_MAX_LEN and P + 8 <= SMALL_MAX_LEN
    out = []
    for k in range(3):
        plants, claims = [(0, b"x"), (n - 1, b"x")], []
        for j, B in enumerate(borders):
            _, pos, p = border_plants("s8", B)[(3 * j + k) % 9]
            plants.append((pos, p))
            claims += occ_claims("s8", pos, p)
        out.append(Case("a", "host/a%d" % k, "s8", plant(n, plants), P, KINDS, tuple(claims)))
    for k in range(3):
        plants, claims = [], []
        for j, B in enumerate(borders):
            ln = 2 + (3 * k + j) % 7  # 2 .. 8
            plants.append((B - 1, LADDER[ln - 1] + b"w"))
            claims += [Claim("row", NOV, (ln - 1, B - 1, B - 1 + ln)), Claim("absent", NOV, (B - 1 + ln - 1,)),
                       Claim("restart", NOV, (B, B - 1 + ln - 1))]
        out.append(Case("b", "host/b%d" % k, "lad", plant(n, plants), P, NOV, tuple(claims)))
    chain = b"kz" * 14 + b"k"
    out.append(Case("b", "host/chain", "s8", plant(n, [(B - 9 + ph, chain) for B, ph in zip(borders, CHAIN_PHASES)]), P, NOV,
                    tuple(Claim("differs", NOV, (r,)) for r in range(4))))
    # the skip: a sixth range of 7 bytes, all of them the tail of the match that starts on the fifth range's last byte
    out.append(Case("b", "host/skip", "lad", b"-" * (n - 1) + LADDER[7], P, NOV, (Claim("skips", NOV, (1,)),)))
    return tuple(out)
