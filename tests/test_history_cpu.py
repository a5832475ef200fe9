"""A handle's history on the CPU (tests/history.py): the model pinned against csrc/find_policy.hpp, the inputs' classes proved
from the oracle's rows, the plan pinned.

* DRIVER: a stand-alone C++ program includes find_policy.hpp -- a host compiler alone builds it -- and keeps a context of its
  own: it steps the header's OWN functions, in the order find_attempts.cpp calls them, through every sequence of the plan,
  and prints state and counter deltas after every call.  history.Context must say the same, call by call, at both ends of
  every range of hot groups.  A changed comparison or constant of the header moves the driver and not the model.
* every input class is what it claims, with its margin, from the oracle's rows alone.
* every call of the plan has exactly ONE predicted delta vector (history.predict raises otherwise): the cap is 0.
No GPU."""
import os
import shutil
import subprocess

import pytest

import history as H
from history import C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ahocorasick_rs_amd", "csrc")

DRIVER = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "find_policy.hpp"

using namespace acx_policy;
typedef unsigned long long ull;

static Limits L;
static ull GROUP_TILES, TILE_BITS, OVF_PER_TILE, DT_GROUP, INPLACE_MAX;

struct Ctx {  // what workspace.hpp's Ctx and Workspace remember, as far as it decides a path
    int dense_hold = 0; bool hold_input = false;
    uint32_t spec_hot = 0, spec_ovf = 0;
    ull hot_inline = 0;
    int dense_full = 0;
    bool wide = false;
    int flag_idx = 0;
    ull tile_cap = 0, trecs_gmax = 0, ovf_cap = 0, dt_cap = 0;
    bool spec_queued = false;
};
struct Facts { ull n, host, pre, batch, small, n_raw, hot_narrow, hot_wide, ovf_need, n_ovf, hits, crowded; };
enum { SPARSE, HOT_CALLS, DENSE_TILES, DENSE_RADIX, WIDE_REDONE, OVF_REGROWN, IN_PLACE, K0, BYTE_RANGES, N_DELTA };

static void ensure_dense_tiles(Ctx &x, ull tiles) {
    if (tiles + 1 > x.dt_cap) x.dt_cap = (tiles + 1) + (tiles + 1) / 8 + DT_GROUP;
}

static void step(Ctx &x, const Facts &f, bool no_spec, ull d[N_DELTA]) {
    for (int i = 0; i < N_DELTA; i++) d[i] = 0;
    x.spec_queued = false;
    if (f.small) { d[K0] = 1; return; }
    // place_host_haystack()
    if (f.host && !f.batch && f.n <= INPLACE_MAX && f.pre && x.dense_hold == 0 && !x.wide && x.spec_hot == 0) d[IN_PLACE] = 1;
    const ull tiles = (f.n + (1ull << TILE_BITS) - 1) >> TILE_BITS, n_groups = (tiles + 1 + GROUP_TILES - 1) / GROUP_TILES;
    bool sparse = start_sparse(true, x.dense_hold, false, tiles);
    bool ovf_grown = false, wide_tried = false, no_dense_tiles = false;
    for (int attempt = 0;; attempt++) {
        if (attempt == MAX_ATTEMPTS) { std::printf("the driver ran out of attempts\n"); std::exit(2); }
        if (!sparse) {  // DenseAttempt
            if (dense_in_tiles(f.pre, true, no_dense_tiles, false, tiles)) {
                ensure_dense_tiles(x, tiles);
                const DenseForm form = dense_form(x.dense_full, false);
                x.dense_full = form.dense_full;
                if (form.compact && f.crowded) x.dense_full = DENSE_FULL_CALLS;
                d[DENSE_TILES]++;
            } else
                d[DENSE_RADIX]++;
            const Hold h = hold_after_dense(Hold{x.dense_hold, x.hold_input}, f.n_raw, tiles);
            x.dense_hold = h.calls; x.hold_input = h.input;
            return;
        }
        // SparseAttempt::run
        const bool wide = x.wide && f.pre;
        const ull gmax = wide ? L.group_max_wide : L.group_max;
        if (tiles > x.tile_cap || gmax > x.trecs_gmax) {  // ensure_tiles
            if (tiles > x.tile_cap) x.tile_cap = tiles + tiles / 8 + GROUP_TILES;
            if (gmax > x.trecs_gmax) x.trecs_gmax = gmax;
            ull want = (x.tile_cap * OVF_PER_TILE + L.ovf_lists - 1) / L.ovf_lists;
            if (want < 64) want = 64;
            if (want > x.ovf_cap) x.ovf_cap = want;
        }
        const bool pin = pin_result(L, f.host && !f.batch, f.batch, false, n_groups, gmax, f.pre);
        const ull out_cap = cap_for(L, n_groups, gmax, f.pre, pin ? L.hot_inline_max : x.hot_inline);
        x.flag_idx ^= 1;  // take_control_block
        uint32_t bound = 0;
        if (f.pre && x.dt_cap && tiles + 1 <= x.dt_cap && !no_spec) {  // launch_post_stage
            bound = spec_bound(L, x.spec_hot, pin, x.hot_inline, n_groups);
            if (bound) ensure_dense_tiles(x, tiles);
        }
        x.spec_queued = bound > 0;
        // pass 0's line, as k_tile_write publishes it
        const ull n_hot = wide ? f.hot_wide : f.hot_narrow;
        ull why = 0, ovf_max = 0;
        if (f.pre && f.ovf_need > x.ovf_cap) { why = 2; ovf_max = f.ovf_need; }
        else if (!f.pre && n_hot) why = 1;
        const uint64_t line[8] = {0, 0, f.n_raw, f.hits, why | (n_hot << 8), f.n_ovf | (ovf_max << 32), 0, 0};
        const TotalsLine t = decode_totals(line);
        // act_on_totals
        if (regrow_overflow(L, t, ovf_grown, tiles)) {
            const ull room = overflow_room(t);
            if (room > x.ovf_cap) x.ovf_cap = room;
            ovf_grown = true;
            continue;
        }
        const Speculation next = next_speculation(L, t);
        x.spec_hot = next.hot; x.spec_ovf = next.ovf;
        const bool spec_done = spec_is_ours(bound, t);
        const SparseCall me{(bool)f.pre, wide, wide_tried, false, ovf_grown, n_groups};
        Verdict v = verdict(me, t, spec_done, false, t.prefix_hits);
        if (v.count_hot) d[HOT_CALLS]++;
        if (v.count_regrown) d[OVF_REGROWN]++;
        if (v.act == Act::RedoWide) { x.wide = wide_tried = true; d[WIDE_REDONE]++; continue; }
        if (v.act == Act::RunHot) {  // run_hot
            ensure_dense_tiles(x, tiles);
            if (hot_bound(L, n_groups, gmax, (uint32_t)t.n_hot) > out_cap && pin) v.act = Act::Dense;
            else {
                if (dense_everywhere((uint32_t)t.n_hot, n_groups)) { const Hold h = hold_dense_input(); x.dense_hold = h.calls; x.hold_input = h.input; }
                d[HOT_CALLS]++;
                x.hot_inline = grown_hot_inline(L, t.n_hot, x.hot_inline);
            }
        } else if (v.act == Act::Sparse) d[SPARSE]++;
        if (v.act == Act::Dense) {
            const Hold h = hold_gave_up(); x.dense_hold = h.calls; x.hold_input = h.input;
            sparse = false;
            continue;
        }
        if (leave_wide(L, wide, t.n_hot, t.occurrences, n_groups)) x.wide = false;
        return;
    }
}

int main(int argc, char **argv) {
    if (argc != 16) return 3;
    ull a[16];
    for (int i = 1; i < 16; i++) a[i] = std::strtoull(argv[i], nullptr, 10);
    L = Limits{a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10]};
    GROUP_TILES = a[11]; TILE_BITS = a[12]; OVF_PER_TILE = a[13]; DT_GROUP = a[14]; INPLACE_MAX = a[15];
    Ctx x;
    ull no_spec = 0;
    char tag[16];
    while (std::scanf("%15s", tag) == 1) {
        if (tag[0] == 'S') {  // SEQ no_spec: a fresh context
            if (std::scanf("%llu", &no_spec) != 1) return 4;
            x = Ctx();
            x.hot_inline = L.hot_inline;
            continue;
        }
        Facts f;
        if (std::scanf("%llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu", &f.n, &f.host, &f.pre, &f.batch, &f.small, &f.n_raw,
                       &f.hot_narrow, &f.hot_wide, &f.ovf_need, &f.n_ovf, &f.hits, &f.crowded) != 12) return 4;
        ull d[N_DELTA];
        step(x, f, no_spec != 0, d);
        for (int i = 0; i < N_DELTA; i++) std::printf("%llu ", d[i]);
        std::printf("| %d %d %u %llu %d %d %d %llu %llu %llu %d\n", x.dense_hold, (int)x.hold_input, x.spec_hot, x.hot_inline, x.dense_full,
                    (int)x.wide, x.flag_idx, x.tile_cap, x.trecs_gmax, x.dt_cap, (int)x.spec_queued);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler: the model cannot be pinned against the header")
    d = tmp_path_factory.mktemp("history")
    src = d / "history_driver.cpp"
    src.write_text(DRIVER)
    exe = d / "history_driver"
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-o", str(exe), str(src)])
    args = [C[k] for k in ("HIT_SLOTS", "OVF_LISTS", "GROUP_MAX", "GROUP_MAX_WIDE", "HOT_SUB", "DT_GMAX", "MATCH_BYTES", "HOT_INLINE",
                           "HOT_INLINE_MAX", "PIN_FINAL_MAX", "GROUP_TILES", "TILE_BITS", "OVF_PER_TILE", "DT_GROUP", "INPLACE_MAX")]

    def run(text: str):
        r = subprocess.run([str(exe)] + [str(v) for v in args], input=text, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout.splitlines()
    return run


def test_the_sources_say_what_the_model_restates():
    H.source_wording()
    assert C["HOLD_CALLS"] >= 2 and C["DENSE_FULL_CALLS"] >= 2 and C["MAX_ATTEMPTS"] >= 4
    assert C["INPLACE_MAX"] == 1 << 20 and C["MATCH_BYTES"] == 24
    assert H.pinned_room_always_holds()  # (the line of run_hot() that sends a pinned call to the dense path cannot fire)


@pytest.mark.parametrize("no_spec", [False, True], ids=["spec", "no_spec"])
def test_the_model_and_the_header_agree_on_every_step(driver, no_spec):
    """every sequence, every kind, the lower and the upper end of every range of hot groups: the driver's deltas and state
    against Context's after every call"""
    text, want = [], []
    for name, calls in H.PLAN.items():
        if no_spec and name not in H.NO_SPEC_SEQUENCES:
            continue
        for kind in range(len(H.KINDS)):
            for hi in (0, 1):
                ctx = H.Context(no_spec)
                text.append("SEQ %d" % no_spec)
                for i, call in enumerate(calls):
                    f = H.facts(call, kind)
                    d = ctx.step(f, use_hi=bool(hi))
                    want.append(((name, kind, hi, i), [d[k] for k in H.EXACT], list(ctx.state())))
                    text.append("CALL %d %d %d %d %d %d %d %d %d %d %d %d" % (
                        f.n, f.host, f.pre, f.batch, f.small, f.n_raw, f.hot_narrow[hi], f.hot_wide[hi], f.ovf_need, f.n_ovf, f.hits,
                        bool(f.crowded)))
    lines = driver("\n".join(text) + "\n")
    assert len(lines) == len(want)
    for ln, (where, deltas, state) in zip(lines, want):
        got_d, got_s = ln.split("|")
        assert [int(v) for v in got_d.split()] == deltas and [int(v) for v in got_s.split()] == state, (where, ln, deltas, state)
    assert len(want) >= (40 if no_spec else 400)


@pytest.mark.parametrize("name", list(H.PLAN))
def test_every_call_has_exactly_one_prediction(name):
    """history.predict() raises where a call's facts straddle a decision: the cap on unpredicted calls is 0"""
    for kind in range(len(H.KINDS)):
        p = H.predict(name, kind)
        assert len(p) == len(H.PLAN[name])
        for q in p:
            assert sum(q.exact[k] for k in ("sparse", "hot_calls", "dense_tiles", "dense_radix", "k0")) == 1 and q.exact["byte_ranges"] == 0


def test_the_plan_says_what_the_issue_asks_for():
    """the transitions themselves, as the model states them: what the GPU run must then show call by call"""
    def col(name, key, kind=0):
        return [q.exact[key] for q in H.predict(name, kind)]
    for kind in range(len(H.KINDS)):
        assert col("A_wide_left", "wide_redone", kind) == [1, 0, 0, 0, 1] and col("A_wide_left", "sparse", kind) == [1] * 5
        assert col("A_wide_kept", "wide_redone", kind) == [1, 0, 0, 0, 0]  # (the twin: MID keeps the form)
        assert col("A_regrow", "wide_redone", kind) == [1, 0, 0, 1]
        # B: the give-up's own dense attempt counts the hold down once: HOLD_CALLS - 1 held calls follow it
        held = C["HOLD_CALLS"] - 1
        assert held == 7 and C["DENSE_FULL_CALLS"] == 8  # (as DESIGN.md section 4 states them: a changed constant changes that table too)
        assert col("B_gave_up", "dense_radix", kind) == [1] + [1] * held + [0, 0] and col("B_gave_up", "sparse", kind) == [0] * (held + 1) + [1, 1]
        assert [sum(x) for x in zip(col("C_dense_input", "hot_calls", kind), col("C_dense_input", "dense_tiles", kind),
                                    col("C_dense_input", "sparse", kind))] == [1] * 4
        assert col("C_dense_input", "hot_calls", kind) == [1, 0, 0, 0] and col("C_dense_input", "dense_tiles", kind) == [0, 1, 1, 0]
        for name in ("D_countdown", "D_rearmed_at_the_end", "D_crowded_one_before"):
            assert col(name, "dense_tiles", kind) == [0] + [1] * (len(H.PLAN[name]) - 1)
        assert col("E_host", "in_place", kind) == [1, 1, 0, 1, 1, 0, 0] and col("E_host", "hot_calls", kind) == [0, 1, 0, 0, 1, 1, 1]
        assert col("E_device", "in_place", kind) == [0] * 7 and col("E_device", "hot_calls", kind) == col("E_host", "hot_calls", kind)
        assert col("F_hot_inline_grows", "hot_calls", kind) == [0, 1, 1, 1] and col("F_hot_inline_grows", "wide_redone", kind) == [1, 0, 0, 0]
        assert col("G_overflow", "overflow_regrown", kind) == [1, 0, 0, 1]
        assert col("I_in_turn", "k0", kind) == [1, 0, 0, 0, 0, 0, 1, 0, 0] and col("I_in_turn", "hot_calls", kind) == [0, 1, 0, 0, 1, 0, 0, 0, 0]
        assert col("K_small_between", "k0", kind) == [0, 1] * 7
        assert [v for v in col("K_small_between", "in_place", kind)[::2]] == col("E_host", "in_place", kind)
    assert H.crowded_decided()
    # F: the context's room for hot groups grows with the first call that has more than HOT_INLINE of them, and stays
    ctx, room = H.Context(), []
    for call in H.PLAN["F_hot_inline_grows"]:
        ctx.step(H.facts(call, 0))
        room.append(ctx.hot_inline)
    k = C["HOT_INLINE"] + 1
    assert room == [C["HOT_INLINE"]] + [min(C["HOT_INLINE_MAX"], 2 * k)] * 3
    f = [H.facts(c, 0) for c in H.PLAN["F_hot_inline_grows"][1:]]
    assert all(x.hot_wide == (k, 2 * k) and 2 * k * 4 <= H.groups_of(x.n) for x in f) and H.groups_of(f[0].n) == 8 * k  # the smallest
    # I: every pair of the four alternations occurs, at sizes on both sides of a group and of 32 and 64 groups
    i_calls = H.PLAN["I_in_turn"]
    assert {(c.flip_overlapping, c.codepoints) for c in i_calls} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {(c.batch, c.host) for c in i_calls} == {(a, b) for a in (False, True) for b in (False, True)}
    assert [c.inp.cls for c in i_calls] == ["CLEAN", "REGIONS", "CLEAN", "CLEAN", "REGIONS", "CLEAN", "CLEAN", "CLEAN", "CLEAN"]
    # D: where the compact form is back -- DENSE_FULL_CALLS calls after the one that armed the full form
    ctx, full = H.Context(), []
    for call in H.PLAN["D_countdown"]:
        ctx.step(H.facts(call, 0))
        full.append(ctx.dense_full)
    assert full == [0, C["DENSE_FULL_CALLS"]] + list(range(C["DENSE_FULL_CALLS"] - 1, -1, -1)) + [0, 0]
    ctx, full = H.Context(), []
    for call in H.PLAN["D_rearmed_at_the_end"]:
        ctx.step(H.facts(call, 0))
        full.append(ctx.dense_full)
    assert full[-3:] == [0, C["DENSE_FULL_CALLS"], C["DENSE_FULL_CALLS"] - 1]  # the compact form was back, and met a crowded call
    ctx, full = H.Context(), []
    for call in H.PLAN["D_crowded_one_before"]:
        ctx.step(H.facts(call, 0))
        full.append(ctx.dense_full)
    assert full[-4:] == [1, 0, 0, 0]  # the crowded call ran in the full form that was still in force: nothing re-armed


def test_the_pinned_boundary_from_the_constants():
    at, over = H.pin_lengths()
    top = H.pinned_groups_max(C["GROUP_MAX"])
    per_group = (C["GROUP_MAX"] + C["HOT_SUB"] * C["DT_GMAX"]) * C["MATCH_BYTES"]
    assert top * per_group <= C["PIN_FINAL_MAX"] < (top + 1) * per_group and top <= C["HOT_INLINE_MAX"]
    assert over == at + 1 and H.groups_of(at) == top and H.groups_of(over) == top + 1
    assert H.pin_result(True, False, False, H.groups_of(at), C["GROUP_MAX"], True) and \
        not H.pin_result(True, False, False, H.groups_of(over), C["GROUP_MAX"], True)
    at_w, over_w = H.pin_lengths(C["GROUP_MAX_WIDE"])
    assert H.pin_result(True, False, False, H.groups_of(at_w), C["GROUP_MAX_WIDE"], True) and \
        not H.pin_result(True, False, False, H.groups_of(over_w), C["GROUP_MAX_WIDE"], True) and over_w == at_w + 1


def _inputs():
    seen = {}
    for calls in H.PLAN.values():
        for c in calls:
            seen.setdefault(c.inp.key, c)
    return seen


@pytest.mark.parametrize("key", sorted(_inputs()))
def test_every_input_is_of_its_class(key):
    """from the oracle's rows: the class's defining quantity on the claimed side of its threshold, by its margin"""
    call = _inputs()[key]
    inp = call.inp
    cen = H.census(inp)
    groups, tiles = H.groups_of(inp.n), H.tiles_of(inp.n)
    whole = inp.n // H.GROUP
    need, _, _ = H.overflow_need(inp)
    first_lists = max(((tiles + tiles // 8 + C["GROUP_TILES"]) * C["OVF_PER_TILE"] + C["OVF_LISTS"] - 1) // C["OVF_LISTS"], 64)
    for kind in range(len(H.KINDS)):
        narrow, wide = H.hot_range(inp, kind, False), H.hot_range(inp, kind, True, call.wide_margin)
        if inp.cls == "CLEAN":
            assert narrow == (0, 0) and wide == (0, 0)
            if inp.n > C["SMALL_MAX_LEN"]:
                assert cen.tile_occ.max() * H.MARGIN <= min(H.STAGE_NARROW_MIN, C["HIT_SLOTS"]) and need == 0
                assert cen.n_raw * 5 * H.MARGIN < groups * C["GROUP_MAX"] * 2   # leave_wide fires
                assert cen.n_raw * H.MARGIN <= 8 * tiles                       # not a dense input
        elif inp.cls == "REGIONS":
            assert narrow[0] == inp.arg and wide[0] == inp.arg and narrow[1] <= 2 * inp.arg
            assert need * H.MARGIN <= first_lists
        elif inp.cls == "STEP" and inp.set == "head":
            assert wide == (0, 0) and need == 0                                # the wide form holds every group
            if inp.arg in (256, 128):
                assert narrow[0] >= whole and narrow[0] * 32 > groups * H.MARGIN  # the narrow stage gives up in every whole group
            if inp.arg == H.MID_STEP:
                assert cen.n_raw * 5 >= H.MARGIN * groups * C["GROUP_MAX"] * 2  # leave_wide does not fire
        elif inp.cls == "STEP":  # STEP64, CROWDED: dense inputs
            assert cen.n_raw >= H.MARGIN * 8 * tiles
            assert H.crowded(inp) is (inp.arg == 16)
            assert cen.tile_occ.max() * 1.9 <= C["DT_SLOTS"]                   # a bucket of the dense form holds its tile (1.9: 261 of 512)
            if inp.arg == 16:
                assert narrow[0] >= whole and need >= H.MARGIN * first_lists
        elif inp.cls == "UNIFORM":
            assert narrow[0] >= whole and narrow[0] * 4 > groups * H.MARGIN     # dense_everywhere
            assert need >= H.MARGIN * first_lists                               # the first lists are too small
            assert cen.n_raw >= H.MARGIN * 8 * tiles
            assert H.overflow_need(inp)[1] * 8 >= H.MARGIN * cen.tile_starts.sum()  # ... and too many overflow hits for the wide form
        elif inp.cls == "GIVEUP":
            assert narrow[0] == 1 and cen.tile_occ.max() >= H.MARGIN * H.STAGE_NARROW_MAX and cen.n_raw * H.MARGIN <= 8 * tiles
        else:
            raise AssertionError(inp.cls)


def test_the_plan_is_pinned():
    assert sorted(H.PLAN) == sorted(["A_wide_left", "A_wide_kept", "A_regrow", "B_gave_up", "C_dense_input", "D_countdown",
                                     "D_rearmed_at_the_end", "D_crowded_one_before", "E_host", "E_device", "F_hot_inline_grows", "G_overflow",
                                     "H_pinned", "I_in_turn",
                                     "H_pinned_wide", "H_pinned_wide_device", "J_A_wide_left", "J_A_wide_kept", "J_B_gave_up",
                                     "J_C_dense_input", "J_G_overflow", "K_small_between"])
    assert H.plan_digest() == "5051dfca6e2e347b", H.plan_digest()
