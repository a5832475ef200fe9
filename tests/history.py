"""A handle's history: what a context (Ctx, csrc/workspace.hpp) carries from one find call to the next, as a model, the
inputs that drive it and the plan of call sequences that tests/test_history_cpu.py checks on the CPU and
tests/test_gpu_history.py runs on the device.  Needs no GPU (run_sequence() and what it calls import the library when called).

* source_constants(): the limits the decisions compare against, read from the sources, and the five places whose wording the
  model restates (a changed constant moves the plan with it, a reworded line fails loudly).
* Context: a Python restatement of the policy state of a Ctx.  step(facts) composes the functions of csrc/find_policy.hpp in
  the order csrc/find_attempts.cpp calls them and returns the deltas of the observable acx_path_stats counters.  The CPU test
  steps the header's own functions through the same sequences (its DRIVER) and compares state and deltas after every call.
* the input classes: built on gen.gen_textlike / gen.gen_uniform with plants, each with Facts computed from the ORACLE's rows
  alone (occurrences per tile, per group, per overflow list).  A claim -- "no hot group", "these groups are hot", "the
  overflow lists are too small" -- holds only where its quantity lies a MARGIN (2, four stated exceptions) on the claimed
  side of its threshold; between the two sides a call is UNPREDICTED, and the plan may hold no such call.
* PLAN: the sequences A .. K of calls on one handle.  Nothing expected comes from the library.

What the occurrence counts stand for.  The device decides on prefix HITS per tile (a hit per position whose prefix passes the
filter: at least one per distinct start of an occurrence, false survivors on top) and on the VIEW's occurrences per bucket and
group (all occurrences for Standard; a leftmost view may hold fewer).  "At least" claims use lower bounds that are exact
(distinct starts, the kind's own reported rows); "at most" claims use all occurrences and leave the margin to the false
survivors."""
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
KINDS = [(0, False), (0, True), (1, False), (2, False)]  # Standard, Standard overlapping, LeftmostFirst, LeftmostLongest
KIND_NAMES = ["standard", "overlapping", "leftmost_first", "leftmost_longest"]
EXACT = ("sparse", "hot_calls", "dense_tiles", "dense_radix", "wide_redone", "overflow_regrown", "in_place", "k0", "byte_ranges")
MARGIN = 2


def _read(*path) -> str:
    with open(os.path.join(*path)) as f:
        return f.read()


# ---------------------------------------------------------------------------
# the constants and the wording of the sources
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def source_constants() -> Dict[str, int]:
    policy, attempts = _read(CSRC, "find_policy.hpp"), _read(CSRC, "find_attempts.cpp")
    types, work = _read(CSRC, "device_types.hpp"), _read(CSRC, "workspace.cpp")
    kern, kern_h, api = _read(CSRC, "kernels.hip"), _read(CSRC, "kernels.hpp"), _read(ROOT, "include", "acx.h")
    out = {}

    def plain(name, src, where, rx=r"\b%s\s*=\s*(\d+)\s*[,;]"):
        m = re.search(rx % name, src)
        assert m, f"{name} is no longer a plain constant of {where}"
        out[name] = int(m.group(1))

    for n in ("HOLD_CALLS", "DENSE_FULL_CALLS", "MAX_ATTEMPTS"):
        plain(n, policy, "find_policy.hpp", r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;")
    m = re.search(r"constexpr\s+uint64_t\s+HOT_INLINE\s*=\s*(\d+)\s*,\s*HOT_INLINE_MAX\s*=\s*(\d+)\s*;", attempts)
    assert m, "HOT_INLINE / HOT_INLINE_MAX are no longer plain constants of find_attempts.cpp"
    out["HOT_INLINE"], out["HOT_INLINE_MAX"] = int(m.group(1)), int(m.group(2))
    m = re.search(r"constexpr\s+uint64_t\s+PIN_FINAL_MAX\s*=\s*(\d+)ull\s*<<\s*(\d+)\s*;", attempts)
    assert m, "PIN_FINAL_MAX is no longer a shifted constant of find_attempts.cpp"
    out["PIN_FINAL_MAX"] = int(m.group(1)) << int(m.group(2))
    for n in ("TILE_BITS", "HIT_SLOTS", "OVF_LISTS", "DT_SLOTS"):
        plain(n, types, "device_types.hpp")
    for n, d in (("GROUP_TILES", "ACX_GROUP_TILES"), ("GROUP_MAX", "ACX_GROUP_MAX"), ("DT_GROUP", "ACX_DT_GROUP")):
        assert re.search(r"\b%s\s*=\s*%s\s*;" % (n, d), types), f"{n} is no longer {d}"
        m = re.search(r"#define\s+%s\s+(\d+)\s*$" % d, types, re.M)
        assert m, f"{d} is no longer a plain constant of device_types.hpp"
        out[n] = int(m.group(1))
    m = re.search(r"\bGROUP_MAX_WIDE\s*=\s*(\d+)\s*\*\s*GROUP_MAX\s*;", types)
    assert m, "GROUP_MAX_WIDE is no longer a multiple of GROUP_MAX"
    out["GROUP_MAX_WIDE"] = int(m.group(1)) * out["GROUP_MAX"]
    assert re.search(r"\bDT_GMAX\s*=\s*DT_GROUP\s*\*\s*DT_SLOTS\s*;", types) and re.search(r"\bHOT_SUB\s*=\s*GROUP_TILES\s*/\s*DT_GROUP\s*;", types)
    out["DT_GMAX"], out["HOT_SUB"] = out["DT_GROUP"] * out["DT_SLOTS"], out["GROUP_TILES"] // out["DT_GROUP"]
    m = re.search(r"inplace_max\s*=\s*std::getenv\(\"ACX_INPLACE_MAX\"\)\s*\?[^\n;]*:\s*\(1ull\s*<<\s*(\d+)\)\s*;", work)
    assert m, "place_host_haystack() no longer has its in-place limit as 1ull << N"
    out["INPLACE_MAX"] = 1 << int(m.group(1))
    plain("OVF_PER_TILE", work, "workspace.cpp")
    plain("SMALL_MAX_LEN", kern_h, "kernels.hpp")
    plain("STAGE_SLOTS_W32", kern, "kernels.hip")
    plain("STAGE_SLOTS_WIDE", kern, "kernels.hip")
    m = re.search(r"#define\s+ACX_STAGE_SLOTS\s+(\d+)\s*$", kern, re.M)
    assert m, "ACX_STAGE_SLOTS is no longer a plain constant of kernels.hip"
    out["STAGE_SLOTS"] = int(m.group(1))
    m = re.search(r"typedef struct acx_match \{(.*?)\}\s*acx_match_t;", api, re.S)
    assert m and re.findall(r"\b(\w+)\s+\w+\s*;", m.group(1)) == ["uint64_t"] * 3, "acx_match_t is no longer three uint64_t"
    out["MATCH_BYTES"] = 24
    assert re.search(r"constexpr\s+pol::Limits\s+LIM\{HIT_SLOTS,\s*OVF_LISTS,\s*GROUP_MAX,\s*GROUP_MAX_WIDE,\s*HOT_SUB,\s*DT_GMAX,\s*"
                     r"sizeof\(acx_match_t\),\s*HOT_INLINE,\s*HOT_INLINE_MAX,\s*PIN_FINAL_MAX\}", attempts), "find_attempts.cpp fills LIM otherwise"
    return out


def source_wording() -> None:
    """the lines the model restates, where find_attempts.cpp, workspace.cpp and kernels.hip have them"""
    attempts, work, kern = _read(CSRC, "find_attempts.cpp"), _read(CSRC, "workspace.cpp"), _read(CSRC, "kernels.hip")
    # (1) a give-up sets the hold, the dense form of THE SAME call counts it down: run_pipeline() goes on with the dense attempt
    sparse_body = attempts[attempts.index("struct SparseAttempt"):attempts.index("struct DenseAttempt")]
    dense_body = attempts[attempts.index("struct DenseAttempt"):attempts.index("int zero_counts(")]
    gave_up = sparse_body.index("set_hold(pol::hold_gave_up());")
    assert sparse_body.index("*what = Attempt::GoDense;") > gave_up, "the give-up no longer sets its hold before it hands the call over"
    assert re.search(r"if\s*\(what\s*==\s*Attempt::GoDense\)\s*sparse\s*=\s*false;\s*if\s*\(what\s*==\s*Attempt::Done\)\s*break;", attempts)
    assert re.search(r"void hold_after\(uint64_t n_raw\)\s*\{\s*set_hold\(pol::hold_after_dense\(pol::Hold\{x->dense_hold,\s*"
                     r"x->hold_dense_input\},\s*n_raw,\s*c\.tiles\)\);\s*\}", dense_body), "hold_after() no longer counts the context's hold"
    assert dense_body.count("hold_after(n_raw);") == 2, "the two dense forms no longer both count the hold"
    # (2) the wide form is the context's from the call that took it
    assert "x->wide = c.wide_tried = true;" in sparse_body
    assert re.search(r"if\s*\(pol::leave_wide\(LIM,\s*wide,\s*t\.n_hot,\s*c\.n_raw,\s*T\.n_groups\)\)\s*x->wide\s*=\s*false;", sparse_body)
    # (3) the in-place condition
    assert re.search(r"if\s*\(len\s*<=\s*inplace_max\s*&&\s*a->kernel\s*==\s*ACX_KERNEL_PREFILTER\s*&&\s*a->sparse_ok\s*&&\s*"
                     r"c->dense_hold\s*==\s*0\s*&&\s*!c->wide\s*&&\s*c->spec_hot\s*==\s*0\)", work), "place_host_haystack() decides otherwise"
    # (4) a pinned result is not regrown
    assert "if (bound > c.out_cap && c.out != w.final) return ACX_OK;" in sparse_body
    # (5) one thread's calls stay on one context: the lease takes the context that was given back last
    assert re.search(r"if\s*\(!a->idle\.empty\(\)\)\s*\{\s*Ctx\s*\*c\s*=\s*a->idle\.back\(\);\s*a->idle\.pop_back\(\);\s*return c;\s*\}", work) and \
        "a->idle.push_back(c);" in work, "take_ctx() no longer takes idle.back()"
    # what the facts restate: the overflow list of a tile, the groups of a call, the lists' first size, the buckets' room
    assert re.search(r"list\s*=\s*\(uint32_t\)tile\s*&\s*\(OVF_LISTS\s*-\s*1\)", kern)
    assert re.search(r"groups\s*=\s*\(tiles\s*\+\s*1\s*\+\s*GROUP_TILES\s*-\s*1\)\s*/\s*GROUP_TILES\s*;", work)
    assert re.search(r"cap_tiles\s*=\s*tiles\s*>\s*w\.tile_cap\s*\?\s*tiles\s*\+\s*tiles\s*/\s*8\s*\+\s*GROUP_TILES\s*:\s*w\.tile_cap\s*;", work)
    assert re.search(r"set_overflow_room\(c,\s*\(cap_tiles\s*\*\s*OVF_PER_TILE\s*\+\s*OVF_LISTS\s*-\s*1\)\s*/\s*OVF_LISTS\)", work)
    assert re.search(r"want\s*=\s*std::min<uint64_t>\(std::max<uint64_t>\(want,\s*64\)", work)
    assert re.search(r"cap\s*=\s*key_tiles\s*\+\s*key_tiles\s*/\s*8\s*\+\s*DT_GROUP\s*;", work)
    assert re.search(r"hot_counts\s*=\s*c\.pre\s*&&\s*w\.dt\.counts\s*&&\s*c\.tiles\s*\+\s*1\s*<=\s*w\.dt_cap\s*\?", sparse_body)


C = source_constants()
TILE = 1 << C["TILE_BITS"]
GROUP = C["GROUP_TILES"] * TILE
STAGE_NARROW_MIN, STAGE_NARROW_MAX = min(C["STAGE_SLOTS"], C["STAGE_SLOTS_W32"]), max(C["STAGE_SLOTS"], C["STAGE_SLOTS_W32"])


def tiles_of(n: int) -> int:
    return (n + TILE - 1) // TILE  # (every haystack of the plan lies at a 16-byte aligned address: no lead bytes)


def groups_of(n: int) -> int:
    return (tiles_of(n) + 1 + C["GROUP_TILES"] - 1) // C["GROUP_TILES"]


# ---------------------------------------------------------------------------
# find_policy.hpp, restated
# ---------------------------------------------------------------------------
def cap_for(n_groups, gmax, pre, hot_room):
    return n_groups * gmax + (min(n_groups, hot_room) * C["HOT_SUB"] * C["DT_GMAX"] if pre else 0)


def pin_result(host_result, segmented, expands, n_groups, gmax, pre):
    return bool(host_result and not segmented and cap_for(n_groups, gmax, pre, C["HOT_INLINE_MAX"]) * C["MATCH_BYTES"] <= C["PIN_FINAL_MAX"]
                and not expands)


def hot_bound(n_groups, gmax, n_hot):
    return (n_groups - n_hot) * gmax + n_hot * C["HOT_SUB"] * C["DT_GMAX"]


def spec_bound(spec_hot, pinned, hot_inline, n_groups):
    if not spec_hot:
        return 0
    b = min(2 * spec_hot, C["HOT_INLINE_MAX"])
    b = min(b, C["HOT_INLINE_MAX"] if pinned else hot_inline)
    b = min(b, n_groups // 32 if n_groups >= 32 else n_groups)
    return b if b >= spec_hot else 0


def regrow_overflow(why, ovf_max, ovf_grown, tiles):
    return why == 2 and not ovf_grown and ovf_max * C["OVF_LISTS"] <= 3 * tiles * C["HIT_SLOTS"] + (C["OVF_LISTS"] << 12)


def overflow_room(ovf_max):
    return ovf_max + ovf_max // 4 + 64


def pinned_groups_max(gmax: int) -> int:
    """the most groups of a K1b call whose records still go to the context's pinned buffer"""
    g = 1
    while pin_result(True, False, False, g + 1, gmax, True):
        g += 1
    return g


class Facts(NamedTuple):
    """what the model may know of a call: its geometry, and what the oracle's rows say of its input"""
    n: int                  # bytes
    host: bool              # acx_find (host haystack, host result) -- or acx_find_device (both on the device)
    pre: bool               # K1b (the prefilter kernel) -- or K1a, which has no hot pipeline
    batch: bool             # a ragged batch of the same bytes (acx_find_batch: staged, segmented)
    small: bool             # K0 takes the call
    n_raw: int              # occurrences
    hot_narrow: Tuple[int, int]  # hot groups, at least and at most: the narrow form
    hot_wide: Tuple[int, int]    # ... the wide form
    ovf_need: int           # hits beyond their tiles' slots in the fullest overflow list (estimate: occurrences for hits)
    n_ovf: int              # ... in all lists
    hits: int               # prefix hits, at least (distinct starts)
    crowded: Optional[bool]  # a group of the tile-ordered dense form does not fit its compact stage
    hot_bytes: int          # bytes of the tiles that may send hits to the overflow lists


class Context:
    """what a Ctx remembers between two calls, as far as it decides a path"""

    def __init__(self, no_spec: bool = False):
        self.dense_hold, self.hold_input = 0, False
        self.spec_hot, self.spec_ovf = 0, 0
        self.hot_inline = C["HOT_INLINE"]
        self.dense_full = 0
        self.wide = False
        self.flag_idx = 0          # the control block the next sparse attempt takes
        self.tile_cap = 0          # tiles the tile buffers hold
        self.trecs_gmax = 0        # records per group the record buffer holds
        self.ovf_cap = 0           # records per overflow list (regrown: an estimate)
        self.ovf_regrown = False   # ... sized by regrow_overflow, not by ensure_tiles
        self.dt_cap = 0            # key tiles the hot pipeline's buckets hold
        self.no_spec = no_spec
        self.spec_queued = False   # (the last call queued the hot pipeline ahead: no counter shows it)
        self.last_hot = None       # the last call's hot groups entered the state (observe_hot)

    def state(self) -> Tuple:
        return (self.dense_hold, int(self.hold_input), self.spec_hot, self.hot_inline, self.dense_full, int(self.wide), self.flag_idx,
                self.tile_cap, self.trecs_gmax, self.dt_cap, int(self.spec_queued))

    def _ensure_dense_tiles(self, tiles):
        if tiles + 1 > self.dt_cap:
            self.dt_cap = (tiles + 1) + (tiles + 1) // 8 + C["DT_GROUP"]

    def step(self, f: Facts, use_hi: bool = False) -> Dict[str, int]:
        """one call.  use_hi: the upper bound of the hot groups where the facts leave a range (the plan demands the same deltas)"""
        d = dict.fromkeys(EXACT, 0)
        self.last_hot, self.spec_queued = None, False
        if f.small:
            d["k0"] = 1
            return d
        if f.host and not f.batch and f.n <= C["INPLACE_MAX"] and f.pre and self.dense_hold == 0 and not self.wide and self.spec_hot == 0:
            d["in_place"] = 1
        tiles, n_groups = tiles_of(f.n), groups_of(f.n)
        sparse = self.dense_hold == 0 and tiles < (1 << 26)  # start_sparse
        ovf_grown = wide_tried = no_dense_tiles = False
        for attempt in range(C["MAX_ATTEMPTS"] + 1):
            assert attempt < C["MAX_ATTEMPTS"], "the model ran out of attempts: no valid call does"
            if not sparse:
                if f.pre and not no_dense_tiles:  # dense_in_tiles
                    self._ensure_dense_tiles(tiles)
                    compact = self.dense_full == 0  # dense_form
                    self.dense_full = max(self.dense_full - 1, 0)
                    if compact and f.crowded:
                        self.dense_full = C["DENSE_FULL_CALLS"]
                    d["dense_tiles"] += 1
                else:
                    d["dense_radix"] += 1
                if f.n_raw > 8 * tiles:  # hold_after_dense
                    self.dense_hold, self.hold_input = C["HOLD_CALLS"], True
                elif self.dense_hold > 0:
                    self.dense_hold = 0 if self.hold_input else self.dense_hold - 1
                return d
            wide = self.wide and f.pre
            gmax = C["GROUP_MAX_WIDE"] if wide else C["GROUP_MAX"]
            if tiles > self.tile_cap or gmax > self.trecs_gmax:  # ensure_tiles
                if tiles > self.tile_cap:
                    self.tile_cap = tiles + tiles // 8 + C["GROUP_TILES"]
                self.trecs_gmax = max(gmax, self.trecs_gmax)
                first = max((self.tile_cap * C["OVF_PER_TILE"] + C["OVF_LISTS"] - 1) // C["OVF_LISTS"], 64)
                if first > self.ovf_cap:
                    self.ovf_cap, self.ovf_regrown = first, False
            pin = pin_result(f.host and not f.batch, f.batch, False, n_groups, gmax, f.pre)  # (the plan's sets have no copies: expand_ov is off)
            out_cap = cap_for(n_groups, gmax, f.pre, C["HOT_INLINE_MAX"] if pin else self.hot_inline)
            self.flag_idx ^= 1  # take_control_block
            bound = 0
            if f.pre and self.dt_cap and tiles + 1 <= self.dt_cap and not self.no_spec:
                bound = spec_bound(self.spec_hot, pin, self.hot_inline, n_groups)
                if bound:
                    self._ensure_dense_tiles(tiles)
            self.spec_queued = bound > 0
            # ---- pass 0's line
            lo, hi = f.hot_wide if wide else f.hot_narrow
            n_hot = hi if use_hi else lo
            why, ovf_max = 0, 0
            if f.pre and f.ovf_need > self.ovf_cap:
                why, ovf_max = 2, f.ovf_need
            elif not f.pre and n_hot:
                why = 1  # (K1a: nothing takes the groups its tile kernels cannot finish)
            if regrow_overflow(why, ovf_max, ovf_grown, tiles):
                self.ovf_cap, self.ovf_regrown = max(self.ovf_cap, overflow_room(ovf_max)), True
                ovf_grown = True
                continue
            self.spec_hot = n_hot if (not why and 0 < n_hot <= C["HOT_INLINE_MAX"]) else 0  # next_speculation
            self.spec_ovf = ovf_max
            spec_done = bool(bound and not why and 0 < n_hot <= bound)  # spec_is_ours
            act = "dense"
            if not why and f.pre and not wide and not wide_tried and n_groups >= 32 and n_hot * 32 > n_groups and f.n_ovf * 8 <= f.hits:
                act = "redo_wide"
            elif not why and not spec_done:
                act = "run_hot" if n_hot else "sparse"
            elif not why:
                act = "spec_done"
            if spec_done:
                d["hot_calls"] += 1
                self.last_hot = (lo, hi)
            if ovf_grown and why != 2:
                d["overflow_regrown"] += 1
            if act == "redo_wide":
                self.wide = wide_tried = True
                d["wide_redone"] += 1
                continue
            if act == "run_hot":
                self._ensure_dense_tiles(tiles)
                if pin and hot_bound(n_groups, gmax, n_hot) > out_cap:
                    act, no_dense_tiles = "dense", False  # (the pinned buffer is not regrown; pinned_room_always_holds(): never)
                else:
                    if n_hot * 4 > n_groups and n_groups >= 8:  # dense_everywhere
                        self.dense_hold, self.hold_input = C["HOLD_CALLS"], True
                    d["hot_calls"] += 1
                    self.last_hot = (lo, hi)
                    if n_hot > self.hot_inline:  # grown_hot_inline
                        self.hot_inline = min(C["HOT_INLINE_MAX"], 2 * n_hot)
            elif act == "sparse":
                d["sparse"] += 1
            if act == "dense":
                self.dense_hold, self.hold_input = C["HOLD_CALLS"], False  # hold_gave_up
                sparse = False
                continue
            if wide and n_hot == 0 and f.n_raw * 5 < n_groups * C["GROUP_MAX"] * 2:  # leave_wide
                self.wide = False
            return d
        raise AssertionError("unreachable")

    def observe_hot(self, n_hot: int) -> None:
        """the hot groups the device counted for the last call, within the facts' bounds: what the NEXT call's prediction may
        take from an earlier call (spec_hot, hot_inline) -- never anything of the call being predicted"""
        if self.last_hot is None:
            return
        lo, hi = self.last_hot
        assert lo <= n_hot <= hi
        if self.spec_hot:
            self.spec_hot = n_hot if n_hot <= C["HOT_INLINE_MAX"] else 0
        if n_hot > self.hot_inline:
            self.hot_inline = min(C["HOT_INLINE_MAX"], 2 * n_hot)


def pinned_room_always_holds() -> bool:
    """run_hot() hands a call to the dense path when the hot pipeline's bound exceeds a PINNED buffer.  The pinned buffer has
    room for HOT_INLINE_MAX hot groups and is taken by at most pinned_groups_max() groups: while that is no more than
    HOT_INLINE_MAX every group may be hot and the bound is the room.  The line cannot fire; no input of the plan can reach it."""
    for gmax in (C["GROUP_MAX"], C["GROUP_MAX_WIDE"]):
        top = pinned_groups_max(gmax)
        if top > C["HOT_INLINE_MAX"]:
            return False
        for g in range(1, top + 1):
            if any(hot_bound(g, gmax, h) > cap_for(g, gmax, True, C["HOT_INLINE_MAX"]) for h in range(g + 1)):
                return False
    return True


# ---------------------------------------------------------------------------
# pattern sets and inputs
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def patterns(name: str) -> Tuple[bytes, ...]:
    if name == "head":    # the headline's set, without copies (copies would switch on expand_ov, which keeps results off the pinned buffer)
        return tuple(dict.fromkeys(gen.gen_patterns(10000, 5, 12, gen.AZ, 1)))
    if name == "short":   # test_gpu_round6.py's set for the dense forms
        return tuple(dict.fromkeys(gen.gen_patterns(3000, 5, 9, gen.AZ, 2)))
    if name == "head_cp":  # ... and two patterns of more than one byte a character: code points differ from byte offsets behind them
        return patterns("head") + CP_PATTERNS
    if name == "pair":    # test_gpu_sparse_path.py's: both patterns' occurrences are staged whatever the call reports
        return (b"abcde", b"cde")
    raise KeyError(name)


CP_PATTERNS = (b"caf\xc3\xa9", b"\xf0\x9f\xa4\xa6x")
SET_PRE = {"head": True, "head_cp": True, "short": True, "pair": False}  # "pair" runs on K1a (KERNEL_DFA_WALK), which gives up where K1b has hot groups


def _plant(hay: np.ndarray, pats, lo: int, hi: int, every: int, seed: int) -> None:
    rng = gen.SplitMix64(seed)
    for k in range(lo, hi - 32, every):
        p = np.frombuffer(pats[rng.next() % len(pats)], dtype=np.uint8)
        hay[k:k + len(p)] = p


REGION_BYTES, REGION_STEP, REGION_AT = 48 << 10, 48, 8 * TILE


class Input(NamedTuple):
    """an input of a class: cls, the set, bytes, a step or a count of regions, the seed"""
    cls: str
    set: str
    n: int
    arg: int = 0
    seed: int = 1

    @property
    def key(self) -> str:
        return "%s/%s/%d/%d/%d" % self


def region_groups(n: int, k: int) -> List[int]:
    full = n // GROUP  # whole groups of the haystack
    assert 1 <= k <= full, (n, k)
    step = full // k
    step -= step > 1 and step % 2 == 0  # (an odd stride: the stretches' tiles then spread over the overflow lists, tile mod OVF_LISTS)
    return [i * step for i in range(k)]


def _plant_characters(hay: np.ndarray, n: int) -> None:
    """the two multibyte patterns in turn, one every ~3 KiB outside the stretches: the text stays valid UTF-8 (ASCII around whole
    characters), and every code-point offset behind the first differs from its byte offset"""
    for i, at in enumerate(range(1000, n - 16, 3001)):
        if REGION_AT - 64 <= at % GROUP < REGION_AT + REGION_BYTES + 64:
            continue
        c = np.frombuffer(CP_PATTERNS[i % 2], dtype=np.uint8)
        hay[at:at + len(c)] = c


@functools.lru_cache(maxsize=64)
def build(inp: Input) -> bytes:
    if inp.set == "head_cp":
        hay = np.frombuffer(build(inp._replace(set="head")), dtype=np.uint8).copy()
        _plant_characters(hay, inp.n)
        return hay.tobytes()
    pats = patterns(inp.set)
    if inp.cls == "CLEAN":      # text, a pattern every 4 KiB ("pair": none -- the text's own letters hold a few); four in a shorter one
        return gen.gen_textlike(inp.n, inp.seed, pats if inp.set != "pair" else (), plant_every=min(4096, max(inp.n // 4, 64))).tobytes()
    if inp.cls == "STEP":       # text with a pattern every KiB, and one every `arg` bytes on top: D256, D128, MID, STEP64, CROWDED
        hay = gen.gen_textlike(inp.n, 11, pats).copy()
        _plant(hay, pats, 0, inp.n, inp.arg, inp.seed)
        return hay.tobytes()
    if inp.cls == "UNIFORM":    # letters with a pattern every `arg` bytes: EVERYWHERE, OVF (bench.py --dist D's shape)
        hay = gen.gen_uniform(inp.n, gen.AZ, 12).copy()
        _plant(hay, pats, 0, inp.n, inp.arg, inp.seed)
        return hay.tobytes()
    if inp.cls == "REGIONS":    # CLEAN with `arg` stretches of 48 KiB, a pattern every 48 bytes, each inside one group
        hay = gen.gen_textlike(inp.n, inp.seed, pats, plant_every=4096).copy()
        for i, g in enumerate(region_groups(inp.n, inp.arg)):
            at = g * GROUP + REGION_AT
            _plant(hay, pats, at, at + REGION_BYTES, REGION_STEP, 1000 * inp.seed + i)
        return hay.tobytes()
    if inp.cls == "GIVEUP":     # one 4 KiB bucket with 40 plants of "abcde" (80 staged occurrences) in an empty stream
        hay = bytearray(b"." * inp.n)
        hay[50000:50000 + 5 * 40] = b"abcde" * 40
        return bytes(hay)
    raise KeyError(inp.cls)


_oracles: Dict[Tuple[str, int], Oracle] = {}
_rows: Dict[Tuple[str, int], np.ndarray] = {}


def oracle(set_name: str, mk: int) -> Oracle:
    if (set_name, mk) not in _oracles:
        _oracles[(set_name, mk)] = Oracle(list(patterns(set_name)), mk, KIND_DFA)
    return _oracles[(set_name, mk)]


def rows(inp: Input, kind: int) -> np.ndarray:
    """the oracle's rows of an input under KINDS[kind]: computed once a session, never changed"""
    if (inp.key, kind) not in _rows:
        mk, ov = KINDS[kind]
        r = oracle(inp.set, mk).find_raw(build(inp), overlapping=ov)
        r.setflags(write=False)
        _rows[(inp.key, kind)] = r
    return _rows[(inp.key, kind)]


class Census(NamedTuple):
    tile_occ: np.ndarray     # all occurrences by the tile of their start
    tile_starts: np.ndarray  # distinct starts: a lower bound of the tile's prefix hits
    n_raw: int


@functools.lru_cache(maxsize=256)
def census(inp: Input) -> Census:
    all_occ = rows(inp, 1)  # Standard, overlapping: every occurrence
    t = tiles_of(inp.n) + 1
    starts = all_occ[:, 1].astype(np.int64) if len(all_occ) else np.zeros(0, np.int64)
    return Census(np.bincount(starts >> C["TILE_BITS"], minlength=t), np.bincount(np.unique(starts) >> C["TILE_BITS"], minlength=t),
                  len(all_occ))


# the margins below 2, and why: GROUP_MAX and GROUP_MAX_WIDE are a factor 4 apart; a density that overfills the narrow groups
# (D256) below one that the wide groups still hold (D128) cannot keep a factor 2 from both.  The narrow side needs none: a
# group reports at most gmax matches, so a group with more ROWS than that is hot whatever else holds.
MARGIN_ROWS_OVER_GMAX = 1    # rows of the kind itself in a group > gmax: exact
MARGIN_D128_WIDE = 1.5       # D128 in the wide form: ~36 occurrences a bucket of 64, ~2 350 a group of 4 096
# an overflow list regrown for an input holds 1.25 x its fullest list + 64; the next input's need is compared with that
# ESTIMATE (both are counted in occurrences, the false survivors inflate both alike): a margin of 1.25 on the estimate
MARGIN_REGROWN = 1.25


def hot_range(inp: Input, kind: int, wide: bool, margin: float = MARGIN) -> Tuple[int, int]:
    """(at least, at most) hot groups.  Hot for certain: a tile with more distinct starts than HIT_SLOTS, a bucket with `margin`
    times the occurrences the stage holds, a group with more rows of this kind than gmax.  Cool for certain: every tile and
    bucket `margin` below its limit, the group's occurrences `margin` below gmax.  A hot stretch may cost the group behind it
    too (its last tiles are that group's context): at most twice the certain ones, plus every group that is neither."""
    cen, n_groups = census(inp), groups_of(inp.n)
    gmax = C["GROUP_MAX_WIDE"] if wide else C["GROUP_MAX"]
    stage_lo, stage_hi = (C["STAGE_SLOTS_WIDE"],) * 2 if wide else (STAGE_NARROW_MIN, STAGE_NARROW_MAX)
    gt = C["GROUP_TILES"]
    pad = lambda a: np.concatenate([a, np.zeros(n_groups * gt - len(a), np.int64)])[:n_groups * gt].reshape(n_groups, gt)
    occ, starts = pad(cen.tile_occ), pad(cen.tile_starts)
    grows = np.zeros(n_groups, np.int64)
    if occ.sum(1).max() > gmax * MARGIN_ROWS_OVER_GMAX:  # (a kind's rows are among the occurrences: no group with fewer can have more rows)
        r = rows(inp, kind)
        grows = np.bincount(r[:, 1].astype(np.int64) // GROUP, minlength=n_groups)[:n_groups] if len(r) else grows
    hot = (starts.max(1) > C["HIT_SLOTS"]) | (occ.max(1) >= margin * stage_hi) | (grows > gmax * MARGIN_ROWS_OVER_GMAX)
    cool = (occ.max(1) * margin <= min(stage_lo, C["HIT_SLOTS"])) & (occ.sum(1) * margin <= gmax)
    lo, unsure = int(hot.sum()), int((~hot & ~cool).sum())
    return lo, min(n_groups, max(2 * lo, lo + unsure) if lo or unsure else 0)


def overflow_need(inp: Input) -> Tuple[int, int, int]:
    """(the fullest overflow list, all lists, bytes of the tiles that feed them): a tile's hits beyond HIT_SLOTS go to list
    tile mod OVF_LISTS -- in occurrences (hits are at least the distinct starts; the margin is the callers')"""
    over = np.maximum(census(inp).tile_occ - C["HIT_SLOTS"], 0)
    lists = np.bincount(np.arange(len(over)) % C["OVF_LISTS"], weights=over, minlength=C["OVF_LISTS"])
    may = int((census(inp).tile_occ * MARGIN > C["HIT_SLOTS"]).sum())
    return int(lists.max()), int(over.sum()), may * TILE


def crowded(inp: Input) -> Optional[bool]:
    """a group of the tile-ordered dense form stages DT_GROUP tiles and the context tile in front: more than the compact stage's
    GROUP_MAX words -- True where the distinct STARTS of five tiles in a row are more than that (every view stages at least one
    occurrence per start: exact, no margin; a pattern every 16 bytes gives 1 280, and DT_SLOTS words a bucket leave no room for
    twice as many), False where the occurrences are MARGIN below it, None in between"""
    cen = census(inp)
    if len(cen.tile_occ) < 8:
        return None
    five = np.ones(C["DT_GROUP"] + 1, np.int64)
    if np.median(np.convolve(cen.tile_starts[:-1], five, "valid")) > C["GROUP_MAX"]:
        return True
    if np.convolve(cen.tile_occ, five, "valid").max() * MARGIN <= C["GROUP_MAX"]:
        return False
    return None


class Call(NamedTuple):
    inp: Input
    host: bool = True
    batch: bool = False
    codepoints: bool = False
    flip_overlapping: bool = False   # sequence I: Standard runs this call overlapping (and the overlapping leg runs it plain)
    wide_margin: float = MARGIN


@functools.lru_cache(maxsize=None)
def facts(call: Call, kind: int) -> Facts:
    inp, kind = call.inp, call_kind(call, kind)
    pre = SET_PRE[inp.set]
    small = pre and not call.batch and inp.n <= C["SMALL_MAX_LEN"]  # (K1a is a FORCED kernel: small_ok() refuses those)
    assert not C["SMALL_MAX_LEN"] < inp.n <= 4 * C["SMALL_MAX_LEN"], "K0's prefilter mode may take this length: the model does not say"
    cen = census(inp)
    need, n_ovf, hot_bytes = overflow_need(inp)
    return Facts(inp.n, call.host, pre, call.batch, small, cen.n_raw, hot_range(inp, kind, False), hot_range(inp, kind, True, call.wide_margin),
                 need, n_ovf, int(cen.tile_starts.sum()), crowded(inp), hot_bytes)


# ---------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------
MiB = 1 << 20


def CLEAN(n, seed=12, set_="head"):
    return Call(Input("CLEAN", set_, n, 0, seed))


def STEP(n, step, set_="head", **kw):
    return Call(Input("STEP", set_, n, step, step), **kw)


def REGIONS(n, k, seed, **kw):
    return Call(Input("REGIONS", "head", n, k, seed), **kw)


def call_kind(call: "Call", kind: int) -> int:
    """the kind a call runs under: sequence I runs every other call of a Standard handle the other way"""
    return 1 - kind if call.flip_overlapping and kind < 2 else kind


def EVERYWHERE(n):
    return Call(Input("UNIFORM", "head", n, 32, 77))


MID_STEP = 384  # 8 MiB: ~30 000 occurrences against leave_wide's 13 517, ~15 a bucket, ~940 a group


def D256(n): return STEP(n, 256)
def D128(n): return STEP(n, 128, wide_margin=MARGIN_D128_WIDE)
def MID(n): return STEP(n, MID_STEP)
def STEP64(n): return STEP(n, 64, "short")
def CROWDED(n): return STEP(n, 16, "short")
def GIVEUP(): return Call(Input("GIVEUP", "pair", MiB))
def SMALL(seed): return Call(Input("CLEAN", "head", 300, 0, seed))


def on_device(calls):
    return [c._replace(host=False) for c in calls]


def _plan() -> Dict[str, List[Call]]:
    W, D, E1 = 8 * MiB, 2 * MiB, MiB  # RedoWide needs 32 groups; dense_everywhere 8; the in-place haystack at most 1 MiB
    full = C["DENSE_FULL_CALLS"]
    p: Dict[str, List[Call]] = {}
    # A: the wide form taken, kept, left (leave_wide has no counter: the LAST call's wide_redone pins it), and its twin
    p["A_wide_left"] = [D256(W), D256(W), D128(W), CLEAN(W), D256(W)]
    p["A_wide_kept"] = [D256(W), D256(W), D128(W), MID(W), D256(W)]
    # ... the tile buffers regrow while the record buffer has its wide size
    p["A_regrow"] = [D256(W), CLEAN(W), CLEAN(2 * W, 13), D256(2 * W)]
    # B: the hold after a give-up, until the model says sparse again (+ one)
    p["B_gave_up"] = [GIVEUP()] + [CLEAN(MiB, 30 + i, "pair") for i in range(C["HOLD_CALLS"] + 1)]
    # C: the hold after a dense input
    p["C_dense_input"] = [EVERYWHERE(D), EVERYWHERE(D), CLEAN(D), CLEAN(D, 13)]
    # D: the full form's countdown.  The first CROWDED call is a hot call that sets the hold; the second meets the compact stage
    p["D_countdown"] = [CROWDED(D), CROWDED(D)] + [STEP64(D)] * (full + 2)
    p["D_rearmed_at_the_end"] = [CROWDED(D), CROWDED(D)] + [STEP64(D)] * full + [CROWDED(D), STEP64(D)]
    p["D_crowded_one_before"] = [CROWDED(D), CROWDED(D)] + [STEP64(D)] * (full - 1) + [CROWDED(D), STEP64(D), STEP64(D)]
    # E: speculation and the in-place haystack
    e = [CLEAN(E1, 41), REGIONS(E1, 1, 42), CLEAN(E1, 43), CLEAN(E1, 44), REGIONS(E1, 1, 45), REGIONS(E1, 1, 46), REGIONS(E1, 3, 47)]
    p["E_host"] = e
    p["E_device"] = on_device(e)
    # G: the overflow lists regrown, then reused
    p["G_overflow"] = [EVERYWHERE(W), EVERYWHERE(W), CLEAN(W), EVERYWHERE(2 * W)]
    # H: the pinned result's boundary
    top = pinned_groups_max(C["GROUP_MAX"])
    at, over = pin_lengths()
    assert groups_of(at) == top and groups_of(over) == top + 1
    p["H_pinned"] = [CLEAN(at, 51), CLEAN(over, 53), CLEAN(at, 51), CLEAN(over, 53)]
    # (hot groups at that boundary: 42 groups redo a call with 2 hot groups in the wide form, and one region may cost two groups.
    # In a context that IS wide no call is redone: the boundary of the wide form's groups, each side with two regions)
    at_w, over_w = pin_lengths(C["GROUP_MAX_WIDE"])
    p["H_pinned_wide"] = [D256(W), REGIONS(at_w, 2, 52), REGIONS(over_w, 2, 54), REGIONS(at_w, 2, 55)]
    p["H_pinned_wide_device"] = on_device(p["H_pinned_wide"])
    # F: hot_inline grows.  More than HOT_INLINE hot groups in a call that is neither dense everywhere (at most a quarter of the
    # groups hot, with twice the regions) nor redone wide (a context that IS wide): the smallest such shape, again, and a larger one
    k = C["HOT_INLINE"] + 1
    n_f = (4 * 2 * k - 1) * GROUP
    assert groups_of(n_f) == 8 * k
    p["F_hot_inline_grows"] = on_device([D256(W), REGIONS(n_f, k, 81), REGIONS(n_f, k, 82), REGIONS(n_f + 64 * GROUP, k, 83)])
    # I: sizes and kinds in turn on one handle: overlapping and not, byte and code-point results, one haystack and a ragged batch
    # of the same bytes, host and device memory; a REGIONS(1) call at the second and at the fifth position
    sizes = [TILE, GROUP - 1, GROUP + 1, 32 * GROUP, 3 * TILE, 64 * GROUP, 2 * GROUP]
    assert [groups_of(x) for x in sizes[3::2]] == [33, 65]
    i_calls = [Call(Input("CLEAN", "head_cp", n, 0, 90 + j)) for j, n in enumerate(sizes)]
    i_calls.insert(1, Call(Input("REGIONS", "head_cp", MiB, 1, 98)))
    i_calls.insert(4, Call(Input("REGIONS", "head_cp", MiB, 1, 99)))
    p["I_in_turn"] = [c._replace(flip_overlapping=bool(j & 1), codepoints=bool(j & 2), batch=bool(j % 3 == 2), host=bool((j // 2) & 1) or j == 0)
                      for j, c in enumerate(i_calls)]
    # J: A, B, C and G behind one CLEAN call: every restart() then falls on the other control block and abort flag
    for name in ("A_wide_left", "A_wide_kept", "B_gave_up", "C_dense_input", "G_overflow"):
        first = p[name][0].inp
        p["J_" + name] = [CLEAN(first.n, 61, first.set)] + p[name]
    # K: small calls between large ones
    k: List[Call] = []
    for i, c in enumerate(e):
        k += [c, SMALL(70 + i)]
    p["K_small_between"] = k
    return p


def pin_lengths(gmax: int = 0) -> Tuple[int, int]:
    """the last length whose K1b host call is pinned, the first whose is not -- from the constants"""
    top = pinned_groups_max(gmax or C["GROUP_MAX"])
    last_tiles = top * C["GROUP_TILES"] - 1  # groups = (tiles + 1 + GROUP_TILES - 1) / GROUP_TILES
    return last_tiles * TILE, last_tiles * TILE + 1


PLAN = _plan()
NO_SPEC_SEQUENCES = ("E_host", "E_device", "K_small_between")


def plan_digest() -> str:
    text = json.dumps({k: [(c.inp.key, c.host, c.batch, c.codepoints, c.flip_overlapping) for c in v] for k, v in sorted(PLAN.items())})
    return hashlib.sha256(text.encode()).hexdigest()[:16]


def crowded_decided() -> bool:
    """every call of the D sequences is crowded or not by its margin: the countdown of the full form is the model's to state"""
    return all(crowded(c.inp) is not None for name, calls in PLAN.items() if name.startswith("D_") for c in calls)


class Predicted(NamedTuple):
    exact: Dict[str, int]
    hot_groups: Tuple[int, int]
    overflow_hits: Tuple[int, int]
    state: Tuple


def unpredicted(f: Facts, ctx: Context) -> List[str]:
    """the reasons a call has no single prediction: a range of hot groups that straddles a decision is found by stepping both
    ends (predict()); here, the quantities that must keep their margin from what the context holds"""
    out = []
    if f.small:
        return out
    if ctx.dense_hold:  # (whether the compact stage holds the groups shows in no counter: sequence D's inputs are decided, crowded_decided())
        return out
    cap = ctx.ovf_cap
    first = max(((tiles_of(f.n) + tiles_of(f.n) // 8 + C["GROUP_TILES"]) * C["OVF_PER_TILE"] + C["OVF_LISTS"] - 1) // C["OVF_LISTS"], 64)
    if tiles_of(f.n) > ctx.tile_cap and first > cap:
        cap, regrown = first, False
    else:
        regrown = ctx.ovf_regrown
    m = MARGIN_REGROWN if regrown else MARGIN
    if f.pre and not (f.ovf_need * m <= cap or f.ovf_need >= m * cap):
        out.append("overflow need %d against lists of %d" % (f.ovf_need, cap))
    return out


def predict(name: str, kind: int, no_spec: bool = False, observed: Optional[List[int]] = None) -> List[Predicted]:
    """every call's deltas.  observed: the hot_groups deltas of the calls run so far -- call i is predicted from those of calls
    < i only.  Raises where a call has no single prediction."""
    lo_ctx, hi_ctx = Context(no_spec), Context(no_spec)
    out = []
    mk, ov = KINDS[kind]
    for i, call in enumerate(PLAN[name]):
        f = facts(call, kind)
        why = unpredicted(f, lo_ctx)
        d_lo = lo_ctx.step(f)
        d_hi = hi_ctx.step(f, use_hi=True)
        if d_lo != d_hi or lo_ctx.state()[:2] + lo_ctx.state()[4:10] != hi_ctx.state()[:2] + hi_ctx.state()[4:10]:  # (but spec_hot, hot_inline)
            why.append("the hot groups' range straddles a decision: %s / %s" % (d_lo, d_hi))
        assert not why, (name, KIND_NAMES[kind], i, call.inp.key, why)
        hot = lo_ctx.last_hot or (0, 0)
        out.append(Predicted(d_lo, hot, (0, f.hot_bytes if d_lo["hot_calls"] else 0), lo_ctx.state()))
        if observed is not None and i < len(observed) and lo_ctx.last_hot is not None:
            lo_ctx.observe_hot(observed[i])
            hi_ctx.last_hot = lo_ctx.last_hot
            hi_ctx.observe_hot(observed[i])
    return out


# ---------------------------------------------------------------------------
# on the device
# ---------------------------------------------------------------------------
def cols(a) -> np.ndarray:
    return np.stack([a["pattern"], a["start"], a["end"]], 1) if len(a) else np.zeros((0, 3), np.uint64)


def pieces_of(hay: bytes, seed: int) -> List[int]:
    """the offsets of a ragged batch over the bytes: 2 .. 24 pieces of unequal lengths, cut between characters, an empty one
    among them"""
    rng, n = gen.SplitMix64(seed), len(hay)
    cuts = set()
    for _ in range(2 + rng.next() % 22):
        c = rng.next() % (n + 1)
        while c < n and (hay[c] & 0xC0) == 0x80:
            c += 1
        cuts.add(c)
    cuts = sorted(cuts)
    return [0] + cuts + [cuts[-1], n]


def expected(call: Call, kind: int):
    """the oracle's rows of a call as the entry point lays them out: (rows, counts or None)"""
    from oracle_lib import byte_to_code_point
    kind = call_kind(call, kind)
    mk, ov = KINDS[kind]
    hay = build(call.inp)
    if not call.batch:
        want = rows(call.inp, kind)
        if call.codepoints and len(want):
            b2c = byte_to_code_point(hay)
            want = np.stack([want[:, 0], b2c[want[:, 1]], b2c[want[:, 2]]], 1)
        return want, None
    off = pieces_of(hay, call.inp.seed)
    out, counts = [], []
    for lo, hi in zip(off, off[1:]):
        r = oracle(call.inp.set, mk).find_raw(hay[lo:hi], overlapping=ov)
        if call.codepoints and len(r):
            b2c = byte_to_code_point(hay[lo:hi])
            r = np.stack([r[:, 0], b2c[r[:, 1]], b2c[r[:, 2]]], 1)
        out.append(r)
        counts.append(len(r))
    return np.concatenate(out) if out else np.zeros((0, 3), np.uint64), np.array(counts, dtype=np.uint64)


def run_call(a, call: Call, kind: int, bufs: Dict):
    """(rows, counts or None) of one call through the C ABI"""
    from ahocorasick_rs_amd import capi
    mk, ov = KINDS[call_kind(call, kind)]
    hay = build(call.inp)
    off = pieces_of(hay, call.inp.seed) if call.batch else None
    if call.host:
        if call.batch:
            m, counts = a.find_batch([hay[lo:hi] for lo, hi in zip(off, off[1:])], overlapping=ov, codepoints=call.codepoints)
            return cols(m), counts
        return cols(a.find(hay, overlapping=ov, codepoints=call.codepoints)), None
    if call.inp.key not in bufs:
        bufs[call.inp.key] = capi.DeviceBuffer(len(hay) + 16).upload(np.frombuffer(hay, dtype=np.uint8))
    dev = bufs[call.inp.key]
    assert dev.ptr % 16 == 0
    if call.batch:
        d_off = capi.DeviceBuffer(8 * len(off)).upload(np.array(off, dtype=np.uint64).view(np.uint8))
        try:
            r = a.find_device(dev.ptr, len(hay), d_offsets=d_off.ptr, n_hay=len(off) - 1, overlapping=ov, codepoints=call.codepoints)
            got, counts = cols(r.matches()), r.counts()
            r.free()
        finally:
            d_off.free()
        return got, counts
    r = a.find_device(dev.ptr, len(hay), overlapping=ov, codepoints=call.codepoints)
    got = cols(r.matches())
    r.free()
    return got, None


def run_sequence(name: str, kind: int, no_spec: bool = False) -> Dict:
    """one handle, the sequence's calls in turn, path_stats(reset=True) in front of every call: rows against the oracle
    element-wise, counter deltas against the model.  {"calls": n, "fails": [...], "log": [per-call deltas]}"""
    from ahocorasick_rs_amd import capi
    calls = PLAN[name]
    mk, _ = KINDS[kind]
    set_name = calls[0].inp.set
    pre = SET_PRE[set_name]
    a = capi.Automaton(list(patterns(set_name)), mk, capi.IMPL_DFA, kernel=None if pre else capi.KERNEL_DFA_WALK)
    fails, log, observed = [], [], []
    if pre and a.info.kernel != capi.KERNEL_PREFILTER:
        fails.append("the set does not run on the prefilter kernel")
    bufs = {}
    try:
        for i, call in enumerate(calls):
            assert call.inp.set == set_name
            want_p = predict(name, kind, no_spec, observed)[i]
            want, want_counts = expected(call, kind)
            a.path_stats(reset=True)
            got, counts = run_call(a, call, kind, bufs)
            st = a.path_stats(reset=True)
            log.append({k: st[k] for k in EXACT + ("hot_groups", "overflow_hits") if st[k]})
            where = "%s call %d (%s)" % (name, i, call.inp.key)
            if got.shape != want.shape or not np.array_equal(got, want):
                fails.append("%s: %d rows, the oracle has %d" % (where, len(got), len(want)))
            if want_counts is not None and not np.array_equal(np.asarray(counts, dtype=np.uint64), want_counts):
                fails.append("%s: the batch's counts differ from the oracle's" % where)
            bad = {k: (st[k], want_p.exact[k]) for k in EXACT if st[k] != want_p.exact[k]}
            if bad:
                fails.append("%s: counters (device, model) %s" % (where, bad))
            for k, (lo, hi) in (("hot_groups", want_p.hot_groups), ("overflow_hits", want_p.overflow_hits)):
                if not lo <= st[k] <= hi:
                    fails.append("%s: %s %d outside [%d, %d]" % (where, k, st[k], lo, hi))
            ok_hot = want_p.hot_groups[0] <= st["hot_groups"] <= want_p.hot_groups[1]
            observed.append(st["hot_groups"] if ok_hot else want_p.hot_groups[0])
    finally:
        for b in bufs.values():
            b.free()
        a.close()
    return {"name": name, "kind": kind, "calls": len(calls), "fails": fails, "log": log}


def main(argv: List[str]) -> int:
    """the child of test_gpu_history.py: ACX_NO_SPEC_HOT is read once per process, so the sequences that queue the hot pipeline
    ahead run here once more without it, one line per (sequence, kind), DONE at the end"""
    assert os.environ.get("ACX_NO_SPEC_HOT"), "the child runs with ACX_NO_SPEC_HOT set"
    for name in NO_SPEC_SEQUENCES:
        for kind in range(len(KINDS)):
            print("SEQ " + json.dumps(run_sequence(name, kind, no_spec=True)), flush=True)
    print("DONE", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
