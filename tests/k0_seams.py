"""K0 -- a whole small call in one workgroup (kernels.hip k0_call<MODE>, launched as k0_small, fed through the mailbox as
k0_resident; the host side is small_calls.cpp) -- at its seams: the constants, the pattern sets, the haystacks and the plan
that tests/test_k0_seams_cpu.py checks on the CPU and tests/test_gpu_k0_seams.py runs on the device.  Needs no GPU
(run_group() and what it calls import the library when called).

Expected rows are the oracle's (tests/oracle_lib.py); k1b_seams.brute() / brute_iter() and post_seams.brute_leftmost() are
the second reference.  Sizes are read from the kernels' sources (source_constants()): a changed constant moves the cases
with it, a renamed one, or a line the plan restates that no longer stands in the sources, fails on the CPU.

mode_of() restates small_mode(): 0 the walk over the tables in global memory (dense table or trie_child), 1 the tables in
LDS (LT), 2 direct comparison (DC), 3 the prefilter, -1 not K0.  Every call of the plan records the mode it is meant for.

A GROUP is an ordered list of calls that run on ONE handle per kind, in that order, nothing between them: the resident
kernel keeps the LDS images of the call before (tables = false) and the bytes of a longer haystack lie behind a shorter
one, so the order is part of the plan.  Every plant is placed by index on a filler no pattern occurs in.

Classes: (a) 63 / 64 / 65 occurrences at wave 0's limit, (b) match counts at the result lines, two haystacks alternating,
(c) the dense cut at SMALL_MAX_OCC, (d) lengths, (e) MODE 2's windows and the DC work limit, (f) sequences of lengths for
the poll, (g) code points, (i) chains in the general finish.  (h), the device-memory form, is a ROUTE: classes a, b, c, d
again through find_device (seq == 0, unpacked records) at pointer residues 0, 1, 8, 15 between guard bytes.

Routes: "resident" (this process, ACX_NO_RESIDENT unset), "device" (this process, find_device), "launched" (ONE child under
ACX_NO_RESIDENT=1), "nopf" (ONE child under ACX_K0_NO_PREFILTER=1: the walk modes on large automata beyond 1 KiB; beyond
SMALL_MAX_LEN the pipeline answers)."""
from __future__ import annotations

import functools
import json
import os
import re
import sys
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

import gen
from k1b_seams import KINDS, NUL_STEMS, code_points_at, cols, with_env
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
    hpp = open(os.path.join(CSRC, "kernels.hpp")).read()
    small = open(os.path.join(CSRC, "small_calls.cpp")).read()
    auto = open(os.path.join(CSRC, "automaton.cpp")).read()
    out: Dict[str, int] = {}

    def plain(name, src, where):
        m = re.search(r"\b%s\s*=\s*(\d+)\s*[,;]" % name, src)
        assert m, f"{name} is no longer a plain constant of {where}"
        out[name] = int(m.group(1))

    for n in ("SMALL_MAX_LEN", "SMALL_MAX_OCC", "SMALL_PF_MAX_LEN", "K0_RESULT_LINES", "K0_MORE_MATCHES", "K0_MAILBOX_INLINE",
              "K0_MAILBOX_HAY"):
        plain(n, hpp, "kernels.hpp")
    for n in ("K0_LT_ENTRIES", "K0_LT_IDS", "K0_DC_PATTERNS", "K0_DC_WORK", "PPS"):
        plain(n, kern, "kernels.hip")
    m = re.search(r"#define\s+ACX_K0_LINE_MATCHES\s+(\d+)\s*$", hpp, re.M)
    assert m, "ACX_K0_LINE_MATCHES is no longer a plain constant of kernels.hpp"
    out["ACX_K0_LINE_MATCHES"] = int(m.group(1))
    assert re.search(r"K0_LINES_MATCHES\s*=\s*ACX_K0_LINE_MATCHES\s*\+\s*\(K0_RESULT_LINES\s*-\s*1\)\s*\*\s*K0_MORE_MATCHES\s*;", hpp), \
        "K0_LINES_MATCHES is no longer the first line's matches and K0_MORE_MATCHES for every further line"
    out["K0_LINES_MATCHES"] = out["ACX_K0_LINE_MATCHES"] + (out["K0_RESULT_LINES"] - 1) * out["K0_MORE_MATCHES"]
    m = re.search(r"const\s+bool\s+tiny\s*=\s*len\s*<=\s*(\d+)\s*;", kern)
    assert m, "tiny is no longer len <= a literal"
    out["TINY"] = int(m.group(1))
    m = re.search(r"if\s*\(seq\s*&&\s*tiny\s*&&\s*n\s*<=\s*(\d+)\)", kern)
    assert m, "wave 0's finish is no longer taken under seq && tiny && n <= 64"
    out["WAVE"] = int(m.group(1))
    for pat, src, what in (
            # small_mode(), whole
            (r"const\s+bool\s+lt\s*=\s*A\.table\s*&&\s*\(\(uint64_t\)A\.n_states\s*<<\s*A\.stride2\)\s*<=\s*K0_LT_ENTRIES\s*&&\s*"
             r"A\.n_states\s*<=\s*K0_LT_IDS\s*&&\s*A\.n_patterns\s*<=\s*K0_LT_IDS\s*&&\s*A\.max_len\s*<\s*256\s*;", kern, "small_mode(): lt"),
            (r"const\s+bool\s+dc\s*=\s*A\.n_patterns\s*<=\s*K0_DC_PATTERNS\s*&&\s*A\.min_len\s*>=\s*1\s*&&\s*A\.max_len\s*<=\s*16\s*&&\s*"
             r"A\.pat_blob\s*&&\s*A\.pat_off\s*&&\s*\(uint64_t\)len\s*\*\s*A\.n_patterns\s*<=\s*K0_DC_WORK\s*&&\s*direct_ok\s*;", kern,
             "small_mode(): dc"),
            (r"const\s+bool\s+pf\s*=\s*small_prefilter_ok\(A\)\s*&&\s*\(len\s*>\s*SMALL_MAX_LEN\s*\|\|\s*\(!dc\s*&&\s*!lt\s*&&\s*len\s*>\s*1024u\)\)\s*;",
             kern, "small_mode(): pf"),
            (r"if\s*\(len\s*>\s*SMALL_MAX_LEN\s*&&\s*!pf\)\s*return\s*-1\s*;\s*return\s*pf\s*\?\s*3\s*:\s*dc\s*\?\s*2\s*:\s*lt\s*\?\s*1\s*:\s*0\s*;",
             kern, "small_mode(): the result"),
            (r"return\s*!off\s*&&\s*A\.filter_q\s*>=\s*3\s*&&\s*A\.short_min_len\s*==\s*0\s*&&\s*A\.filterA\s*&&\s*A\.ptab\s*&&\s*A\.pinfo\s*&&\s*"
             r"A\.max_len\s*<\s*\(1u\s*<<\s*15\)\s*;", kern, "small_prefilter_ok()"),
            (r"llevel\[LT\s*\?\s*258\s*:\s*1\]", kern, "llevel[258]"),
            (r"if\s*\(t\s*<\s*A\.max_len\s*\+\s*2\)\s*llevel\[t\]\s*=\s*A\.level_start\[t\]\s*;", kern, "t < A.max_len + 2"),
            # the finishes
            (r"if\s*\(n\s*>\s*SMALL_MAX_OCC\)", kern, "n > SMALL_MAX_OCC"),
            (r"if\s*\(tot\s*>\s*K0_LINES_MATCHES\)", kern, "tot > K0_LINES_MATCHES"),
            (r"taken\s*=\s*n\s*==\s*64\s*\?\s*~0ull\s*:\s*\(1ull\s*<<\s*n\)\s*-\s*1\s*;", kern, "taken"),
            (r"to\s*=\s*\(t\s*<\s*n\s*\?\s*r\s*:\s*63u\)\s*<<\s*2\s*;", kern, "the permute's target"),
            (r"\(\(e\s*>>\s*4\)\s*<\s*64\s*\?\s*be\s*:\s*all\)", kern, "(e >> 4) < 64 ? be : all"),
            (r"if\s*\(sj\s*>=\s*pos\)\s*\{\s*taken\s*\|=", kern, "sj >= pos"),
            (r"if\s*\(key_mode\s*==\s*0\s*\|\|\s*sj\s*\+\s*A\.max_len\s*<=\s*s\)\s*break\s*;", kern, "sj + A.max_len <= s"),
            (r"if\s*\(n\s*<=\s*64\)\s*\{\s*//\s*\(mine\s*!=\s*0\s*only\s*in\s*wave\s*0\)", kern, "the general finish's n <= 64"),
            (r"if\s*\(n\s*<=\s*64\s*\?\s*t\s*==\s*63\s*:\s*t\s*==\s*1023\)\s*s_total\s*=\s*total\s*;", kern, "the total's lane"),
            (r"if\s*\(codepoints\s*&&\s*PF\s*&&\s*len\s*>\s*16384\)", kern, "the SPT path"),
            # MODE 3
            (r"const\s+bool\s+any\s*=\s*len\s*>=\s*A\.k1b_min_len\s*;", kern, "any"),
            (r"last\s*=\s*any\s*\?\s*len\s*-\s*A\.k1b_min_len\s*:\s*0\s*;", kern, "last"),
            (r"j0\s*=\s*2\s*\*\s*PPS\s*\*\s*t\s*;\s*any\s*&&\s*j0\s*<=\s*last\s*;\s*j0\s*\+=\s*2\s*\*\s*PPS\s*\*\s*1024\)", kern, "2 * PPS * 1024"),
            (r"&&\s*j\s*\+\s*1\s*<=\s*last\s*;", kern, "j + 1 <= last"),
            (r"if\s*\(PF\s*&&\s*t\s*<\s*32\)\s*sh\[len\s*\+\s*t\]\s*=\s*0\s*;", kern, "the 32 zero bytes"),
            (r"sh\[MAXLEN\s*\+\s*32\]", kern, "sh[MAXLEN + 32]"),
            # MODE 2
            (r"m0\s*=\s*L\s*>=\s*8\s*\?\s*~0ull\s*:\s*\(1ull\s*<<\s*\(8\s*\*\s*L\)\)\s*-\s*1\s*;", kern, "m0"),
            (r"m1\s*=\s*L\s*>\s*8\s*\?\s*\(L\s*>=\s*16\s*\?\s*~0ull\s*:\s*\(1ull\s*<<\s*\(8\s*\*\s*\(L\s*-\s*8\)\)\)\s*-\s*1\)\s*:\s*0\s*;", kern, "m1"),
            (r"c\s*=\s*sh64\[q\s*\+\s*2\]\s*;", kern, "sh64[q + 2]"),
            # the poll
            (r"covered\s*=\s*len\s*<\s*K0_MAILBOX_INLINE\s*\?\s*\(len\s*\+\s*15\)\s*&\s*~15u\s*:\s*K0_MAILBOX_INLINE\s*;", kern, "covered"),
            (r"if\s*\(covered\s*<=\s*16\s*\*\s*\(width\s*-\s*1\)\)", kern, "covered <= 16 * (width - 1)"),
            (r"width\s*=\s*min\(64u,\s*\(1\s*\+\s*covered\s*/\s*16\s*\+\s*3\)\s*&\s*~3u\)\s*;", kern, "width"),
            # the host
            (r"return\s*!off\s*&&\s*!a->kernel_forced\s*&&\s*len\s*>\s*0\s*&&\s*a->host\.n_patterns\s*>\s*0\s*&&\s*"
             r"\(len\s*<=\s*SMALL_MAX_LEN\s*\|\|\s*\(len\s*<=\s*SMALL_PF_MAX_LEN\s*&&\s*small_prefilter_ok\(a->dev\)\)\)\s*;", small, "small_ok()"),
            (r"if\s*\(mode\s*<\s*0\s*\|\|\s*len\s*>\s*SMALL_MAX_LEN\)\s*\{\s*stop_resident\(c\)\s*;\s*return\s*ACX_OK\s*;\s*\}", small,
             "the resident kernel's length limit"),
            (r"if\s*\(\+\+R\.switches\s*>=\s*4\)\s*\{\s*R\.switches\s*=\s*0\s*;\s*R\.calls\s*=\s*0\s*;\s*R\.off\s*=\s*256\s*;", small, "R.off after four changes"),
            (r"a->expand_ov\s*=\s*xe\s*\?\s*std::atoi\(xe\)\s*!=\s*0\s*:\s*n_later\s*\*\s*4\s*>=\s*\(uint64_t\)H\.n_patterns\s*;",
             open(os.path.join(CSRC, "build_upload.cpp")).read(), "expand_ov")):
        assert re.search(pat, src), f"the sources no longer define {what} as the plan restates it"
    for name, src, pat in (
            ("ACX_NO_RESIDENT", small, r"static\s+const\s+bool\s+off\s*=\s*std::getenv\(\"ACX_NO_RESIDENT\"\)"),
            ("ACX_NO_SMALL", small, r"static\s+const\s+bool\s+off\s*=\s*std::getenv\(\"ACX_NO_SMALL\"\)"),
            ("ACX_K0_NO_PREFILTER", kern, r"static\s+const\s+bool\s+off\s*=\s*std::getenv\(\"ACX_K0_NO_PREFILTER\"\)"),
            ("ACX_DENSE_LIMIT", auto, r"const\s+char\s*\*env\s*=\s*std::getenv\(\"ACX_DENSE_LIMIT\"\)")):
        assert re.search(pat, src), f"{name} is no longer read where the plan believes it is"
    return out


C = source_constants()
TINY, WAVE, MAX_OCC = C["TINY"], C["WAVE"], C["SMALL_MAX_OCC"]
MAX_LEN, PF_MAX_LEN, INLINE = C["SMALL_MAX_LEN"], C["SMALL_PF_MAX_LEN"], C["K0_MAILBOX_INLINE"]
LINE0, MORE, LINES, IN_LINES = C["ACX_K0_LINE_MATCHES"], C["K0_MORE_MATCHES"], C["K0_RESULT_LINES"], C["K0_LINES_MATCHES"]
STRIDE = 2 * C["PPS"] * 1024  # positions between a thread's steps in MODE 3


def line_and_slot(i: int) -> Tuple[int, int]:
    """where match i of a polled call travels: (line, word) for the first K0_LINES_MATCHES, (-1, index in out[]) beyond"""
    if i < LINE0:
        return 0, 2 + i
    if i < IN_LINES:
        return 1 + (i - LINE0) // MORE, 1 + (i - LINE0) % MORE
    return -1, i - IN_LINES


def covered_of(n: int) -> int:
    return (n + 15) & ~15 if n < INLINE else INLINE


def poll_trace(lens: List[int]) -> List[Tuple[int, int, bool]]:
    """(covered, the width the poll leaves behind, the bytes came with the poll) per call of a kernel that takes `lens` in
    turn; the kernel's first poll is 64 lanes wide"""
    out, width = [], 64
    for n in lens:
        cov = covered_of(n)
        inline = cov <= 16 * (width - 1)
        width = min(64, (1 + cov // 16 + 3) & ~3)
        out.append((cov, width, inline))
    return out


# ---------------------------------------------------------------------------
# pattern sets: each on the filler '-' (and '+'), which no pattern holds
# ---------------------------------------------------------------------------
FILL, FILL2 = ord("-"), ord("+")
U, U2, X = b"qwert", b"yuiop", b"xyzwx"  # two units (one occurrence a plant); X overlaps itself by one byte
L17 = b"L" + body(17, 16)
COVER = b"W" + b"cd" * 31 + b"dx"       # holds 31 "cd" and 32 "d": 64 occurrences, one leftmost match; X can begin at its last byte
COVER3 = b"W" + b"cde" * 63 + b"x"      # ... without patterns under 3 bytes: 63 "cde" and itself
# as long as the cover (the set's max_len), and its own first bytes as a LATER pattern: two occurrences at one start, the longest first
VLONG, VLONG3 = b"V" + body(65, len(COVER) - 2) + b"x", b"V" + body(191, len(COVER3) - 2) + b"x"
PRE = b"ijklmnopqrstuvwxyz"             # (letters body() does not use)
DC_LENS = (1, 7, 8, 9, 15, 16)
NULS = tuple(stem + b"\0" * k for stem, k in NUL_STEMS)
LONG_A, LONG_B = b"A" + body(2000, 1999), b"B" + body(2100, 2099)


def dc_pattern(i: int, L: int) -> bytes:
    return bytes([ord("A") + i // 6]) if L == 1 else (bytes([PRE[i // 18], PRE[i % 18]]) + body(100 + i, L - 2))


def shortlex(k: int) -> Tuple[bytes, ...]:
    """the first k strings over {a, b} by length, then by value: every state a pattern's"""
    out, L = [], 1
    while len(out) < k:
        for v in range(1 << L):
            out.append(bytes(ord("a") + ((v >> (L - 1 - j)) & 1) for j in range(L)))
            if len(out) == k:
                break
        L += 1
    return tuple(out)


class SetInfo(NamedTuple):
    pats: Tuple[bytes, ...]
    fam: Tuple[bytes, ...] = ()    # a word and its suffixes: len(fam) occurrences a plant, one leftmost match
    fam2: Tuple[bytes, ...] = ()
    cover: Optional[bytes] = None
    chain: bool = False            # X is in the set
    dense_limit0: bool = False     # built under ACX_DENSE_LIMIT=0: the compressed automaton (trie_child)
    one: Optional[bytes] = None    # a 1-byte pattern


FAM, FAM2 = (b"abcd", b"bcd", b"cd"), (b"ghij", b"hij", b"ij")
FAM_3, FAM2_3 = (b"abcde", b"bcde", b"cde"), (b"ghijk", b"hijk", b"ijk")
FEW = (U, U2) + FAM + FAM2 + (b"d", X, L17, COVER, VLONG, VLONG[:4])
BIG3 = (U, U2) + FAM_3 + FAM2_3 + (X, COVER3) + NULS + (VLONG3, VLONG3[:4])


@functools.lru_cache(maxsize=None)
def info(name: str) -> SetInfo:
    many = tuple(gen.gen_patterns(3000, 4, 12, gen.AZ, 3))
    if name == "dc4":    # MODE 2 up to 1 024 bytes
        return SetInfo((U, U2, b"abcd", b"bcd"), fam=(b"abcd", b"bcd"))
    if name == "dc8":    # MODE 2 up to 512 bytes
        return SetInfo((U, U2) + FAM + FAM2, fam=FAM, fam2=FAM2)
    if name == "dc2":    # MODE 2 up to 2 048 bytes
        return SetInfo((U, b"d"), one=b"d")
    if name == "one16":  # MODE 2 up to 4 096 bytes, MODE 1 beyond
        return SetInfo((dc_pattern(5, 16),))
    if name in ("dc64", "dc65", "dc17"):
        pats = [dc_pattern(i, DC_LENS[i % 6]) for i in range(65 if name == "dc65" else 64)]
        if name == "dc17":
            pats[63] = dc_pattern(63, 17)
        return SetInfo(tuple(pats))
    if name == "few":    # MODE 1 at every length
        return SetInfo(FEW, fam=FAM, fam2=FAM2, cover=COVER, chain=True, one=b"d")
    if name in ("lt255", "lt256"):  # one pattern of 255 bytes (LT's deepest walk, llevel[257]) and its twin of 256 (not LT)
        return SetInfo((b"M" + body(255, int(name[2:]) - 1),))
    if name in ("ltmax", "ltover"):  # the largest set LT takes beside U and U2 (a row of 32 classes), and one pattern more
        return SetInfo((U, U2) + shortlex(lt_limit((U, U2))[0] + (name == "ltover")))
    if name in ("ltids", "ltidsover"):  # ... over {a, b} alone (a row of 4 classes)
        return SetInfo(shortlex(lt_limit(())[0] + (name == "ltidsover")))
    if name in ("m0", "m0c"):  # MODE 0 at every length: too large for the LDS, a 1-byte pattern keeps the prefilter away
        return SetInfo(FEW + many, fam=FAM, fam2=FAM2, cover=COVER, chain=True, dense_limit0=name == "m0c", one=b"d")
    if name == "m3":     # MODE 0 up to 1 KiB, MODE 3 beyond
        return SetInfo(BIG3 + many, fam=FAM_3, fam2=FAM2_3, cover=COVER3, chain=True)
    if name == "urls3":  # anchored (max_shift != 0): verify_seams' URL set without its 1- and 2-byte beginnings
        import verify_seams
        return SetInfo((U, U2) + FAM_3 + tuple(p for p in verify_seams.patterns("urls") if len(p) >= 3), fam=FAM_3)
    if name == "long2k":  # k1b_min_len = 2 000: MODE 3 on haystacks shorter than every pattern
        return SetInfo((LONG_A, LONG_B))
    if name == "copies":  # copies of a string: expand_ov, an overlapping call is not MODE 2
        return SetInfo((b"abc", b"abc", U, U, b"zq"))
    raise KeyError(name)


SETS = ("dc4", "dc8", "dc2", "one16", "dc64", "dc65", "dc17", "few", "lt255", "lt256", "ltmax", "ltover", "ltids", "ltidsover", "m0", "m0c", "m3", "urls3",
        "long2k", "copies")


def patterns(name: str) -> Tuple[bytes, ...]:
    return info(name).pats


class Facts(NamedTuple):
    """what small_mode() reads of an automaton"""
    dense: bool
    n_states: int
    stride: int
    n_patterns: int
    min_len: int
    max_len: int
    filter_q: int
    short_min_len: int
    long_min_len: int
    max_shift: int
    copies: int   # ids that are a later copy of a string (Standard only)


@functools.lru_cache(maxsize=None)
def facts_of(pats: Tuple[bytes, ...], mk: int, dense_limit0: bool = False) -> Facts:
    from ahocorasick_rs_amd import capi
    with with_env({"ACX_DENSE_LIMIT": "0"} if dense_limit0 else {}):
        h = capi.HostAutomaton(list(pats), mk)
    t = h.t
    own = np.diff(h.own_off.astype(np.int64))
    f = Facts(bool(t.dense), int(t.n_states), int(t.stride), int(t.n_patterns), int(t.min_pattern_len), int(t.max_pattern_len),
              int(t.filter_q), int(t.short_min_len) if t.n_short else 0, int(t.long_min_len), int(t.max_shift),
              int(np.sum(own[own > 1] - 1)) if mk == 0 else 0)
    h.close()
    return f


def facts(name: str, mk: int) -> Facts:
    return facts_of(patterns(name), mk, info(name).dense_limit0)


def lt_reasons(f: Facts) -> List[str]:
    """the limits of LT that the automaton is beyond"""
    return [w for w, bad in (("K0_LT_ENTRIES", f.n_states * f.stride > C["K0_LT_ENTRIES"]), ("K0_LT_IDS states", f.n_states > C["K0_LT_IDS"]),
                             ("K0_LT_IDS patterns", f.n_patterns > C["K0_LT_IDS"]), ("max_len", f.max_len >= 256),
                             ("no dense table", not f.dense)) if bad]


def mode_of(f: Facts, n: int, overlapping: bool, prefilter: bool = True) -> int:
    """small_mode(view of the call, n, !(overlapping && expand_ov)) behind small_ok(); prefilter = False: ACX_K0_NO_PREFILTER"""
    if n == 0 or f.n_patterns == 0:
        return -1
    expand_ov = f.copies > 0 and f.copies * 4 >= f.n_patterns
    direct_ok = not (overlapping and expand_ov)
    lt = not lt_reasons(f)
    dc = f.n_patterns <= C["K0_DC_PATTERNS"] and f.min_len >= 1 and f.max_len <= 16 and n * f.n_patterns <= C["K0_DC_WORK"] and direct_ok
    pf_ok = prefilter and f.filter_q >= 3 and f.short_min_len == 0 and f.max_len < (1 << 15)
    pf = pf_ok and (n > MAX_LEN or (not dc and not lt and n > 1024))
    if n > MAX_LEN and not (pf and n <= PF_MAX_LEN):
        return -1
    return 3 if pf else 2 if dc else 1 if lt else 0


@functools.lru_cache(maxsize=None)
def lt_limit(base: Tuple[bytes, ...]) -> Tuple[int, List[str]]:
    """(k, the limits the set of k + 1 is beyond): `base` and the first k strings over {a, b} are the largest such set LT takes"""
    def ok(k):
        return not lt_reasons(facts_of(base + shortlex(k), 0))
    lo, hi = 1, 4096
    assert ok(lo) and not ok(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return lo, lt_reasons(facts_of(base + shortlex(lo + 1), 0))


# ---------------------------------------------------------------------------
# haystacks
# ---------------------------------------------------------------------------
def hay_of(n: int, plants, fill: int = FILL) -> bytes:
    """n filler bytes with (position, bytes) plants; a plant must lie inside"""
    h = bytearray([fill]) * n
    for x, p in plants:
        assert 0 <= x and x + len(p) <= n, (x, len(p), n)
        h[x:x + len(p)] = p
    return bytes(h)


class Call(NamedTuple):
    name: str
    hay: bytes
    mode: int                # the mode the call is meant for (checked against mode_of() on the CPU; "nopf": mode_of(prefilter=False))
    cp: bool = False
    dense: bool = False      # more than SMALL_MAX_OCC occurrences: K0 gives up, the pipeline answers
    claim: tuple = ()        # what the class says of the call, recomputed on the CPU: ("n", 64), ("matches", kind index, 23), ...


class Group(NamedTuple):
    cls: str
    set: str
    name: str
    calls: Tuple[Call, ...]
    ci: bool = False         # an ascii_case_insensitive handle
    device: bool = False     # runs on the "device" route too (class h)


def spread(n: int, k: int, width: int, mirror: bool) -> List[int]:
    """k starts of `width`-byte plants in n bytes: the first at 0, the last flush with the end, evenly between; mirrored:
    the same positions counted from the end"""
    if k == 0:
        return []
    if k == 1:
        return [0 if mirror else n - width]
    pitch = (n - width) // (k - 1)
    assert pitch >= width + 1, (n, k, width)
    xs = [i * pitch for i in range(k - 1)] + [n - width]
    return sorted(n - width - x for x in xs) if mirror else xs


def m(name: str, n: int, ov: bool = False) -> int:
    return mode_of(facts(name, 0), n, ov)


@functools.lru_cache(maxsize=None)
def per_plant(name: str, word: bytes) -> int:
    """occurrences of the set's patterns in one plant of `word`"""
    return sum(word.count(p) for p in patterns(name))


A_SETS = ("dc4", "few", "m0", "m0c", "m3")


def groups_a() -> List[Group]:
    """63, 64, 65 occurrences in 1 024 and 1 025 bytes, the last one ending at the last byte, planted forwards and mirrored;
    64 links of X (every second one taken), COVER (one taken)"""
    out = []
    for s in A_SETS:
        i, calls = info(s), []
        for n in (TINY, TINY + 1):
            for k in (WAVE - 1, WAVE, WAVE + 1):
                for mir in (False, True):
                    calls.append(Call(f"units{k}_{n}{'_mirror' if mir else ''}", hay_of(n, [(x, U) for x in spread(n, k, len(U), mir)]), m(s, n),
                                      claim=(("n", k), ("last_end", n))))
            if i.chain:
                for mir in (False, True):
                    at = n - (4 * WAVE + 1) if mir else 0
                    calls.append(Call(f"chain{WAVE}_{n}{'_mirror' if mir else ''}", hay_of(n, [(at + 4 * j, X) for j in range(WAVE)]), m(s, n),
                                      claim=(("n", WAVE), ("taken", WAVE // 2))))
            if i.cover:
                for mir in (False, True):
                    calls.append(Call(f"cover_{n}{'_mirror' if mir else ''}", hay_of(n, [(n - len(i.cover) if mir else 0, i.cover)]), m(s, n),
                                      claim=(("n", WAVE), ("taken", 1))))
        out.append(Group("a", s, "wave0", tuple(calls), device=True))
    return out


B_COUNTS = (0, 1, LINE0, LINE0 + 1, LINE0 + MORE, LINE0 + MORE + 1, LINE0 + 2 * MORE, LINE0 + 2 * MORE + 1, IN_LINES, IN_LINES + 1,
            IN_LINES + 2, WAVE, WAVE + 1)
B_LEN = 512
B_SETS = ("dc8", "few", "m0", "m0c", "m3")


def groups_b() -> List[Group]:
    """k matches, k at every line's limit: haystack A (U, or the first family, from byte 0 on) and haystack B (U2, or the second
    family, from byte 3 on, on the other filler) alternate on one handle -- they differ in every match's position and id"""
    out = []
    for s in B_SETS:
        i, calls = info(s), []
        for fam in (False, True):
            for k in B_COUNTS:
                pa, pb = ((i.fam[0], i.fam2[0]) if fam else (U, U2))
                a = hay_of(B_LEN, [(7 * j, pa) for j in range(k)])
                b = hay_of(B_LEN, [(3 + 7 * j, pb) for j in range(k)], FILL2)
                for rep in range(2):
                    calls.append(Call(f"{'fam' if fam else 'unit'}{k}_A{rep}", a, m(s, B_LEN), claim=(("n", k * per_plant(s, pa)), ("leftmost", k), ("leftmost_starts", 0, 7))))
                    calls.append(Call(f"{'fam' if fam else 'unit'}{k}_B{rep}", b, m(s, B_LEN), claim=(("n", k * per_plant(s, pb)), ("leftmost", k), ("leftmost_starts", 3, 7))))
        out.append(Group("b", s, "lines", tuple(calls), device=True))
    return out


def groups_c() -> List[Group]:
    """SMALL_MAX_OCC - 1, SMALL_MAX_OCC and one more occurrence: the last call is the pipeline's"""
    out = []
    for s, n, p, pitch in (("dc2", 2048, b"d", 2), ("few", 2100, b"d", 2), ("m0", 2100, b"d", 2), ("m0c", 2100, b"d", 2), ("m3", MAX_LEN, U, 16)):
        slots = list(range(0, n - len(p) + 1, pitch)) + [pitch // 2]  # (the last one between the first two)
        assert len(slots) >= MAX_OCC + 1
        calls = []
        for k in (MAX_OCC - 1, MAX_OCC, MAX_OCC + 1):
            xs = slots[:k] if k <= MAX_OCC else slots[:MAX_OCC] + slots[-1:]
            calls.append(Call(f"occ{k}", hay_of(n, [(x, p) for x in xs]), m(s, n), dense=k > MAX_OCC,
                              claim=(("n", k), ("has_starts", 0, pitch, min(k, MAX_OCC)))))
        out.append(Group("c", s, "cut", tuple(calls), device=True))
    return out


D_LENS = (1, 2, 15, 16, 17, 47, 48, 49, 63, 64, 65, INLINE - 1, INLINE, INLINE + 1, TINY - 1, TINY, TINY + 1, STRIDE - 1, STRIDE, STRIDE + 1,
          MAX_LEN - 1, MAX_LEN, MAX_LEN + 1, PF_MAX_LEN - 1, PF_MAX_LEN, PF_MAX_LEN + 1)
D_SETS = ("dc4", "dc2", "few", "lt255", "lt256", "ltmax", "ltover", "ltids", "ltidsover", "m0", "m0c", "m3", "urls3", "copies")


def end_plant(i: SetInfo, n: int) -> bytes:
    """what stands flush with the last byte: the family's word (its shortest suffix begins at the last legal start), else U,
    else the longest pattern that fits"""
    for p in [p for p in i.fam[:1] + (U,) if p in i.pats] + sorted(i.pats, key=len, reverse=True):
        if len(p) <= n:
            return p
    return b""


def front_plant(i: SetInfo, room: int) -> bytes:
    """what stands at byte 0: the longest pattern that fits the room (the deepest walk the set has)"""
    return next((p for p in sorted(i.pats, key=len, reverse=True) if len(p) <= room), b"")


def groups_d() -> List[Group]:
    """every length: a match flush with byte 0 and one flush with the last byte (flush), the same with the last plant cut one
    byte short by the end (cut), MODE 3: the letters of the NUL patterns at the very end, their NULs in the zero fill (nul),
    plants around a thread's stride"""
    out = []
    for s in D_SETS:
        i, calls = info(s), []
        for n in D_LENS:
            md = m(s, n)
            if md < 0 and m(s, n - 1) < 0:
                continue  # (the first length beyond K0's reach is enough)
            e = end_plant(i, n)
            first = front_plant(i, n - len(e))
            plants = ([(0, first)] if first else []) + ([(n - len(e), e)] if e else [])
            calls.append(Call(f"flush_{n}", hay_of(n, plants), md, dense=md < 0, claim=(("ends_at", n),) if e else ()))
            e1 = end_plant(i, n + 1)
            if e1:  # the plant's last byte is beyond the end
                first = front_plant(i, n + 1 - len(e1))
                cut = hay_of(n + 1, ([(0, first)] if first else []) + [(n + 1 - len(e1), e1)])[:n]
                calls.append(Call(f"cut_{n}", cut, md, dense=md < 0, claim=(("cut", e1),)))
            if md == 3 and NULS[0] in i.pats:
                stems = [(n - 40, NULS[2][:-8]), (n - 20, NULS[1][:-2]), (n - len(NULS[0]) + 1, NULS[0][:-1])]
                calls.append(Call(f"nul_stems_{n}", hay_of(n, stems), md, claim=(("n", 0),)))
                calls.append(Call(f"nul_short_{n}", hay_of(n, [(n - 40, NULS[1][:-1]), (n - len(NULS[2]) + 1, NULS[2][:-1])]), md, claim=(("n", 0),)))
                calls.append(Call(f"nul_flush_{n}", hay_of(n, [(0, NULS[1]), (n - len(NULS[2]), NULS[2])]), md, claim=(("n", 2), ("ends_at", n))))
        if m(s, STRIDE + 8) == 3:  # starts around the stride of a thread's steps, in 16 KiB and in 64 KiB
            for n in (MAX_LEN, PF_MAX_LEN):
                if m(s, n) == 3:
                    w = i.fam[0] if i.fam else max(i.pats, key=len)
                    w2 = U if U in i.pats else w
                    for x in range(STRIDE - 2, STRIDE + 2):
                        calls.append(Call(f"stride_{n}_{x}", hay_of(n, [(x, w), (min(x + STRIDE, n - len(w2)), w2)]), 3,
                                          claim=(("n", per_plant(s, w) + per_plant(s, w2)),)))
        out.append(Group("d", s, "lengths", tuple(calls), device=True))
    # MODE 3 on haystacks shorter than, and as long as, the shortest pattern (any = false; last = 0)
    k = len(LONG_A)
    calls = [Call("short_by_one", LONG_A[:k - 1], 3, claim=(("n", 0),)), Call("exact", LONG_A, 3, claim=(("n", 1), ("ends_at", k))),
             Call("one_more_odd", b"-" + LONG_A, 3, claim=(("n", 1), ("ends_at", k + 1))), Call("one_more_even", LONG_A + b"-", 3, claim=(("n", 1),)),
             Call("second_exact", LONG_B, 3, claim=(("n", 1),)), Call("both", LONG_A + LONG_B, 3, claim=(("n", 2), ("ends_at", 2 * k + 100)))]
    out.append(Group("d", "long2k", "min_len", tuple(calls), device=True))
    return out


def near(p: bytes, k: int) -> bytes:
    """p with byte k replaced by a letter no pattern of the DC sets holds"""
    return p[:k] + b"Z" + p[k + 1:]


def groups_e() -> List[Group]:
    """MODE 2: a pattern of every length at every pos & 7 and at the haystack's last bytes, a near miss in every byte of the
    16-byte pattern, the twins of 65 patterns and of a 17-byte pattern; len * n_patterns = K0_DC_WORK and one more, as a loop
    of 40 calls on one handle"""
    out = []
    n = C["K0_DC_WORK"] // C["K0_DC_PATTERNS"]
    for s in ("dc64", "dc65", "dc17"):
        pats, calls = patterns(s), []
        for k, L in enumerate(DC_LENS):
            p = pats[6 + k] if len(pats[6 + k]) == L else pats[k]
            assert len(p) == L
            for x in range(8, 16):
                calls.append(Call(f"len{L}_at{x}", hay_of(n, [(x, p), (x + 24, pats[12 + k])]), m(s, n), claim=(("n", 2),)))
            calls.append(Call(f"len{L}_last", hay_of(n, [(n - L, p)]), m(s, n), claim=(("n", 1), ("ends_at", n))))
            calls.append(Call(f"len{L}_last_cut", hay_of(n + 1, [(n - L + 1, p)])[:n], m(s, n), claim=(("n", 0),)))
        p16 = pats[5]
        for k in range(16):
            calls.append(Call(f"near{k}", hay_of(n, [(9, near(p16, k)), (40, near(p16, k))]), m(s, n), claim=(("n", 0),)))
        longest = max(pats, key=len)
        calls.append(Call("longest", hay_of(n, [(3, longest), (n - len(longest), longest)]), m(s, n), claim=(("n", 2),)))
        out.append(Group("e", s, "windows", tuple(calls)))
    p, w = patterns("one16")[0], C["K0_DC_WORK"]
    lo = hay_of(w, [(0, p), (1001, p), (w - 16, p)])
    hi = hay_of(w + 1, [(1, p), (1000, p), (w + 1 - 16, p)], FILL2)
    calls = []
    for k in range(20):
        calls += [Call(f"work_{w}_{k}", lo, m("one16", w), claim=(("n", 3),)), Call(f"work_{w + 1}_{k}", hi, m("one16", w + 1), claim=(("n", 3),))]
    out.append(Group("e", "one16", "work", tuple(calls)))
    # a set with copies: not MODE 2 for an overlapping call (the plan's modes are the non-overlapping call's; call_mode() names the other)
    calls = [Call(f"copies_{k}", hay_of(64, [(k, b"abc"), (k + 20, U), (61, b"abc")]), m("copies", 64), claim=(("n", 3),)) for k in range(8)]
    out.append(Group("e", "copies", "copies", tuple(calls)))
    return out


F_LENS = (16, INLINE, 16, INLINE + 1, 48, 49, TINY, 1)
F_SETS = ("dc4", "few", "m0")


def seq_hay(n: int, step: int, full: Optional[bool]) -> bytes:
    """call `step` of a sequence: even steps on '-' with U from byte 0 on, odd steps on '+' with U2 from byte 3 on -- every
    byte differs from the step before; full: plants back to back, None: filler alone, else one at the front and one flush
    with the end"""
    p, off, fill = (U, 0, FILL) if step % 2 == 0 else (U2, 3, FILL2)
    if n < off + len(p) or full is None:
        return bytes([fill]) * n
    xs = list(range(off, n - len(p) + 1, 10)) if full else sorted({off, n - len(p)} if n - len(p) >= off + len(p) else {n - len(p)})
    return hay_of(n, [(x, p) for x in xs], fill)


def sequences() -> Dict[str, List[Tuple[int, bool, bool]]]:
    """name -> (length, full of matches, code points) per call"""
    asc, alt = sorted(F_LENS), list(F_LENS)
    out = {"as_listed": [(n, False, k % 2 == 1) for k, n in enumerate(alt)],
           "ascending": [(n, False, k % 2 == 0) for k, n in enumerate(asc)],
           "descending": [(n, False, k % 2 == 1) for k, n in enumerate(reversed(asc))],
           # a long haystack full of matches, then a short one of filler, and the reverse
           "full_then_empty": [(TINY, True, False), (16, None, False), (INLINE, True, True), (1, None, False), (48, True, False),
                               (INLINE + 1, True, False), (49, None, True), (TINY, True, True)]}
    return out


def groups_f() -> List[Group]:
    out = []
    for s in F_SETS:
        for ci in (False, True):
            if ci and s != "few":
                continue
            for name, steps in sequences().items():
                calls = []
                for k, (n, full, cp) in enumerate(steps):
                    h = seq_hay(n, k, full)
                    calls.append(Call(f"{name}_{k}_{n}", h.upper() if ci and k % 3 else h, m(s, n), cp=cp))
                out.append(Group("f", s, name + ("_ci" if ci else ""), tuple(calls), ci=ci))
    return out


UNITS = {"w1": ["-"], "w2": ["é"], "w3": ["☃"], "w4": ["🤦"], "mixed": ["-", "é", "☃", "🤦", "é", "-", "-", "🤦"]}
G_SETS = ("dc4", "few", "m0", "m3")


def cp_hay(n: int, width: str, plants) -> bytes:
    """n bytes of whole characters of the filler, '-' where a whole one does not fit, with the plants at their byte offsets"""
    units, out, k = [u.encode() for u in UNITS[width]], bytearray(), 0
    for x, p in sorted(plants) + [(n, b"")]:
        assert x >= len(out), (x, len(out))
        while len(out) + len(units[k % len(units)]) <= x:
            out += units[k % len(units)]
            k += 1
        out += b"-" * (x - len(out)) + p
    assert len(out) == n
    return bytes(out)


def groups_g() -> List[Group]:
    """fillers of every character width: matches from byte 0, ends at every x & 15 around slice borders, a match that ends at
    the last byte -- 1 024 bytes (cpre[64], and wave 0's shuffles), 1 025 and 16 384 (cpre[1024]), 16 385 and 65 536 (SPT)"""
    out = []
    for s in G_SETS:
        calls = []
        for n in (TINY, TINY + 1, MAX_LEN, MAX_LEN + 1, PF_MAX_LEN):
            md = m(s, n)
            if md < 0:
                continue
            for w in UNITS:
                base = 0 if n <= TINY + 1 else n - 1024  # (the last KiB of a long haystack: every slice in front counts)
                ends = [base + 48 * (k + 2) + k for k in range(16)]
                few_plants = [(0, U)] + [(e - len(U), U2 if k % 2 else U) for k, e in enumerate(ends)][:3 if w != "mixed" else 16]
                plants = few_plants + [(n - len(U), U)]
                calls.append(Call(f"{w}_{n}", cp_hay(n, w, plants), md, cp=True, claim=(("ends_at", n),)))
                if w == "mixed":  # every x & 15, and few enough occurrences for wave 0 (1 024 bytes); then more than 64
                    many = [(x, U) for x in range(base + 8, base + 48 * 17 + 15, 11) if all(abs(x - y) >= 6 for y, _ in plants)]
                    calls.append(Call(f"{w}_{n}_many", cp_hay(n, w, plants + many), md, cp=True, claim=(("more_than", WAVE),)))
                    calls.append(Call(f"{w}_{n}_bytes", cp_hay(n, w, plants), md, cp=False))
            if n == PF_MAX_LEN:  # end - 1 = 65 535 in the packed word's 16 bits
                calls.append(Call(f"ascii_{n}", hay_of(n, [(0, U), (n - len(U), U)]), md, cp=True, claim=(("ends_at", n),)))
        out.append(Group("g", s, "code_points", tuple(calls)))
    return out


def groups_i() -> List[Group]:
    """the general finish's sync points: 70 and 200 links of X, each overlapping the next by one byte; the longest pattern
    with the next occurrence max_len bytes behind its start (the scan stops there) and max_len - 1 (X over its last byte)"""
    out = []
    for s in ("few", "m0", "m0c", "m3"):
        i, calls = info(s), []
        f = facts(s, 0)
        assert len(i.cover) <= f.max_len
        for links in (70, 200):
            n = 4 * links + 1 + 40
            for at in (0, 39):
                calls.append(Call(f"links{links}_at{at}", hay_of(n, [(at + 4 * j, X) for j in range(links)]), m(s, n),
                                  claim=(("n", links), ("taken", (links + 1) // 2))))
        longest = max(i.pats, key=len)
        L = len(longest)
        for n in (TINY, TINY + 1):
            units = [(x, U) for x in range(2 * L + 40, 2 * L + 40 + 12 * 10, 10)]
            calls.append(Call(f"touching_{n}", hay_of(n, [(3, longest), (3 + L, U)] + units), m(s, n), claim=(("more_than", WAVE),)))
            calls.append(Call(f"over_last_byte_{n}", hay_of(n, [(3, longest), (3 + L - 1, X)] + units), m(s, n), claim=(("more_than", WAVE),)))
            v = VLONG if VLONG in i.pats else VLONG3
            assert len(v) == L
            units = [(x, U) for x in range(L + 40, L + 40 + 70 * 6, 6)]
            calls.append(Call(f"two_at_one_start_{n}", hay_of(n, [(3, v), (3 + L - 1, X)] + units), m(s, n), claim=(("more_than", WAVE),)))
            calls.append(Call(f"two_longest_{n}", hay_of(n, [(3, longest), (3 + L - 1, X), (3 + L + 3, X), (3 + L + 8, longest)]), m(s, n),
                              claim=(("more_than", WAVE),)))
        out.append(Group("i", s, "chains", tuple(calls)))
    return out


CLASSES = ("a", "b", "c", "d", "e", "f", "g", "i")


@functools.lru_cache(maxsize=None)
def plan() -> Tuple[Group, ...]:
    return tuple(groups_a() + groups_b() + groups_c() + groups_d() + groups_e() + groups_f() + groups_g() + groups_i())


def group(cls: str, set_name: str, name: str) -> Group:
    return next(g for g in plan() if (g.cls, g.set, g.name) == (cls, set_name, name))


RESIDUES = (0, 1, 8, 15)
ROUTES = ("resident", "device", "launched", "nopf")
ROUTE_ENV = {"launched": "ACX_NO_RESIDENT", "nopf": "ACX_K0_NO_PREFILTER"}


def route_groups(route: str) -> List[Group]:
    return [g for g in plan() if route != "device" or g.device]


def call_mode(g: Group, c: Call, route: str, ov: bool = False) -> int:
    """the mode of the call on a route: the plan's, or what is left without the prefilter / for an overlapping call on copies"""
    if route == "nopf" or (ov and g.set == "copies"):
        return mode_of(facts(g.set, 0), len(c.hay), ov, prefilter=route != "nopf")
    return c.mode


def group_modes(g: Group, route: str) -> set:
    """the modes the group's calls have on a route under ANY kind (an overlapping call on copies has another mode than the
    non-overlapping call on the same bytes): what run_group() can tag a failure with"""
    return {call_mode(g, c, route, ov) for c in g.calls for ov in (False, True)}


def tests_of(route: str) -> List[Tuple[str, int]]:
    """(class, mode) pairs that have calls on a route: one test each"""
    return sorted({(g.cls, md) for g in route_groups(route) for md in group_modes(g, route)})


# ---------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle(set_name: str, mk: int, ci: bool = False) -> Oracle:
    return Oracle([p.lower() if ci else p for p in patterns(set_name)], mk, KIND_DFA)


_want: Dict[tuple, np.ndarray] = {}


def byte_rows(g: Group, k: int, mk: int, ov: bool) -> np.ndarray:
    key = (g.cls, g.set, g.name, k, mk, ov)
    if key not in _want:
        h = g.calls[k].hay
        _want[key] = oracle(g.set, mk, g.ci).find_raw(np.frombuffer(h.lower() if g.ci else h, dtype=np.uint8), overlapping=ov).astype(np.uint64)
    return _want[key]


def expected(g: Group, k: int, mk: int, ov: bool) -> np.ndarray:
    w, c = byte_rows(g, k, mk, ov), g.calls[k]
    if c.cp and len(w):
        a = np.frombuffer(c.hay, dtype=np.uint8)
        w = np.stack([w[:, 0], code_points_at(a, w[:, 1]), code_points_at(a, w[:, 2])], 1)
    return w


# ---------------------------------------------------------------------------
# the device side (imports the library when called)
# ---------------------------------------------------------------------------
GUARD = 0xC3  # a lead byte: counted as a code point wherever it is read as part of the haystack


def pipeline_calls(st) -> int:
    return st["sparse"] + st["hot_calls"] + st["dense_tiles"] + st["dense_radix"]


def run_group(g: Group, route: str) -> Dict:
    """the group's calls in their order on ONE handle per kind, element-wise against the oracle; path_stats over the group.
    "device": every call at every pointer residue between guard bytes, which stay as they were"""
    from ahocorasick_rs_amd import capi
    fails: List[Tuple[int, str]] = []
    calls = 0
    for mk, ov in KINDS:
        with with_env({"ACX_DENSE_LIMIT": "0"} if info(g.set).dense_limit0 else {}):
            a = capi.Automaton(list(patterns(g.set)), mk, ascii_case_insensitive=g.ci)
        a.path_stats(reset=True)
        want_k0 = made = 0
        for k, c in enumerate(g.calls):
            md = call_mode(g, c, route, ov)
            want = expected(g, k, mk, ov)
            for res in (RESIDUES if route == "device" else (None,)):
                if res is None:
                    try:
                        got = cols(a.find(c.hay, overlapping=ov, codepoints=c.cp))
                    except capi.AcxError as e:  # (an answer that did not arrive is a wrong answer of that call, not the end of the group)
                        got = np.full((1, 3), 2 ** 63, np.uint64)
                        fails.append((md, f"{g.set}/{g.name}/{c.name} kind {mk} overlapping {ov}: {e}"))
                    same = True
                else:
                    n = len(c.hay)
                    buf = np.full(16 + res + n + 48, GUARD, np.uint8)
                    buf[16 + res:16 + res + n] = np.frombuffer(c.hay, dtype=np.uint8)
                    dev = capi.DeviceBuffer(len(buf))
                    dev.upload(buf)
                    assert dev.ptr % 16 == 0
                    r = a.find_device(dev.ptr + 16 + res, n, overlapping=ov, codepoints=c.cp)
                    got = cols(r.matches())
                    r.free()
                    same = np.array_equal(dev.download(), buf)
                    dev.free()
                made += 1
                want_k0 += int(md >= 0 and not c.dense)
                if not np.array_equal(got, want) or not same:
                    bad = next((j for j in range(min(len(got), len(want))) if not np.array_equal(got[j], want[j])), min(len(got), len(want)))
                    fails.append((md, f"{g.set}/{g.name}/{c.name} kind {mk} overlapping {ov}{'' if res is None else ' residue %d' % res}: "
                                      f"{len(got)} rows against {len(want)}, first difference at row {bad}"
                                      f"{'' if same else '; the buffer was written to'}"))
        st = a.path_stats()
        a.close()
        calls += made
        if st["k0"] != want_k0 or pipeline_calls(st) != made - want_k0:
            fails.append((-2, f"{g.set}/{g.name} kind {mk} overlapping {ov}: k0 {st['k0']} and {pipeline_calls(st)} pipeline calls, the plan says "
                              f"{want_k0} and {made - want_k0} ({st})"))
        if route == "resident" and want_k0 and st["resident_launches"] < 1 and any(len(c.hay) <= MAX_LEN for c in g.calls):
            fails.append((-2, f"{g.set}/{g.name} kind {mk} overlapping {ov}: no resident kernel was launched ({st})"))
        if route in ("launched", "device") and st["resident_launches"] != 0:
            fails.append((-2, f"{g.set}/{g.name} kind {mk} overlapping {ov}: {st['resident_launches']} resident launches on the {route} route"))
    return {"cls": g.cls, "set": g.set, "name": g.name, "calls": calls, "fails": fails}


def run_group_py(g: Group) -> List[str]:
    """the group through the Python classes: BytesAhoCorasick (byte offsets) and AhoCorasick (str: code points, always)"""
    import ahocorasick_rs_amd as ac
    kinds = {0: ac.MatchKind.Standard, 1: ac.MatchKind.LeftmostFirst, 2: ac.MatchKind.LeftmostLongest}
    fails = []
    for mk, ov in KINDS:
        with with_env({"ACX_DENSE_LIMIT": "0"} if info(g.set).dense_limit0 else {}):
            b = ac.BytesAhoCorasick(list(patterns(g.set)), matchkind=kinds[mk])
            t = ac.AhoCorasick([p.decode() for p in patterns(g.set)], matchkind=kinds[mk])
        for k, c in enumerate(g.calls):
            rows = byte_rows(g, k, mk, ov)
            a = np.frombuffer(c.hay, dtype=np.uint8)
            cp = np.stack([rows[:, 0], code_points_at(a, rows[:, 1]), code_points_at(a, rows[:, 2])], 1) if len(rows) else rows
            if b.find_matches_as_indexes(c.hay, overlapping=ov) != [tuple(int(v) for v in r) for r in rows]:
                fails.append(f"{g.set}/{g.name}/{c.name} kind {mk} overlapping {ov}: BytesAhoCorasick")
            if t.find_matches_as_indexes(c.hay.decode(), overlapping=ov) != [tuple(int(v) for v in r) for r in cp]:
                fails.append(f"{g.set}/{g.name}/{c.name} kind {mk} overlapping {ov}: AhoCorasick")
    return fails


_ran: Dict[tuple, Dict] = {}


def ran(g: Group, route: str) -> Dict:
    key = (route, g.cls, g.set, g.name)
    if key not in _ran:
        _ran[key] = run_group(g, route)
    return _ran[key]


def verdict(records: List[Dict], groups: List[Group], route: str, cls: str, mode: int) -> Tuple[int, List[str]]:
    """(the fails of class `cls` on calls meant for `mode`, plus the path_stats fails of the groups that hold such calls)"""
    out = []
    for g, rec in zip(groups, records):
        if g.cls == cls and mode in group_modes(g, route):
            out += [t for md, t in rec["fails"] if md == mode or md == -2]
    return len(out), out[:40]


def child_main(route: str):
    assert os.environ.get(ROUTE_ENV[route]), ROUTE_ENV[route]
    for g in route_groups(route):
        print("GROUP " + json.dumps(run_group(g, route)), flush=True)
    print("DONE", flush=True)


if __name__ == "__main__":
    child_main(sys.argv[1])
