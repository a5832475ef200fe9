"""The path policy of a find call (csrc/find_policy.hpp) at the boundary of every comparison it makes.

A stand-alone C++ program with its own main includes the header -- a host compiler alone builds it: no HIP, no context, no
environment -- and compares every decision with a literal expectation, worked out by hand from the comparisons
find_attempts.cpp made before the policy had a header of its own.  The limits are the real ones (HIT_SLOTS 64, OVF_LISTS
256, GROUP_MAX 1024, GROUP_MAX_WIDE 4096, HOT_SUB 16, DT_GMAX 2048, 24-byte records, HOT_INLINE 16 .. 128, 32 MiB of pinned
records), passed in as numbers; test_post_seams_cpu.py keeps them equal to the sources'.  No GPU.
"""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ahocorasick_rs_amd", "csrc")

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include "find_policy.hpp"

using namespace acx_policy;
typedef unsigned long long ull;

static unsigned cases = 0, bad = 0;
static void check(int line, ull got, ull want) {
    cases++;
    if (got != want && bad++ < 20) std::printf("line %d: got %llu, want %llu\n", line, got, want);
}
#define IS(expr, want) check(__LINE__, (ull)(expr), (ull)(want))

static const Limits L{64, 256, 1024, 4096, 16, 2048, 24, 16, 128, 32ull << 20};

// the line as k_tile_write publishes it: [4] why | hot groups << 8, [5] overflow hits | the fullest list << 32
static TotalsLine line_of(ull why, ull n_hot, ull n_ovf, ull ovf_max, ull hits = 0) {
    const uint64_t w[8] = {7, 11, 22, hits, why | (n_hot << 8), n_ovf | (ovf_max << 32), 0, 0};
    return decode_totals(w);
}
static ull act(const SparseCall &s, const TotalsLine &t, bool spec_done, bool spec_lost, ull hits) {
    return (ull)verdict(s, t, spec_done, spec_lost, hits).act;
}
static const ull REDO = (ull)Act::RedoWide, HOT = (ull)Act::RunHot, SPARSE = (ull)Act::Sparse, SPEC = (ull)Act::SpecDone,
                 DENSE = (ull)Act::Dense;

int main() {
    // ---- rule 1: the line's fields at their full widths, none bleeding into another
    {
        const uint64_t full[8] = {1, ~0ull, ~0ull - 1, ~0ull - 2, ~0ull, ~0ull, 0, 0};
        TotalsLine t = decode_totals(full);
        IS(t.matches, ~0ull); IS(t.occurrences, ~0ull - 1); IS(t.prefix_hits, ~0ull - 2);
        IS(t.why, 255); IS(t.n_hot, (1ull << 56) - 1); IS(t.n_ovf, 0xFFFFFFFFull); IS(t.ovf_max, 0xFFFFFFFFull);
        t = line_of(2, (1ull << 56) - 1, 0, 0xFFFFFFFFull);
        IS(t.why, 2); IS(t.n_hot, (1ull << 56) - 1); IS(t.n_ovf, 0); IS(t.ovf_max, 0xFFFFFFFFull);
        t = line_of(255, 0, 0xFFFFFFFFull, 0, 5);
        IS(t.why, 255); IS(t.n_hot, 0); IS(t.n_ovf, 0xFFFFFFFFull); IS(t.ovf_max, 0);
        IS(t.matches, 11); IS(t.occurrences, 22); IS(t.prefix_hits, 5);
    }
    // ---- rule 2: output room.  A hot group reports up to HOT_SUB * DT_GMAX = 32 768 records
    IS(cap_for(L, 100, 1024, true, 128), 100 * 1024 + 100 * 32768);  // fewer groups than the room for hot ones
    IS(cap_for(L, 200, 1024, true, 128), 200 * 1024 + 128 * 32768);  // more
    IS(cap_for(L, 16, 1024, true, 16), 16 * 1024 + 16 * 32768);
    IS(cap_for(L, 17, 1024, true, 16), 17 * 1024 + 16 * 32768);
    IS(cap_for(L, 200, 1024, false, 128), 200 * 1024);               // K1a: no hot pipeline
    IS(cap_for(L, 10, 4096, true, 16), 10 * 4096 + 10 * 32768);      // the wide form
    // the pin test: 32 MiB hold 1 398 101 records; K1b, narrow: 33 792 a group
    IS(pin_result(L, true, false, false, 41, 1024, true), 1);        // 1 385 472 records
    IS(pin_result(L, true, false, false, 42, 1024, true), 0);        // 1 419 264
    IS(pin_result(L, true, false, false, 1365, 1024, false), 1);     // K1a: 1 397 760
    IS(pin_result(L, true, false, false, 1366, 1024, false), 0);     // 1 398 784
    {
        Limits X = L; // (a limit the records fill exactly: 41 groups' 1 385 472 records of 24 bytes)
        X.pin_final_max = 1385472ull * 24;
        IS(pin_result(X, true, false, false, 41, 1024, true), 1);
        X.pin_final_max = 1385472ull * 24 - 24; // one record over
        IS(pin_result(X, true, false, false, 41, 1024, true), 0);
        X.pin_final_max = 1385472ull * 24 - 1;  // one byte over
        IS(pin_result(X, true, false, false, 41, 1024, true), 0);
    }
    IS(pin_result(L, false, false, false, 41, 1024, true), 0);       // a device result
    IS(pin_result(L, true, true, false, 41, 1024, true), 0);         // veto: a batch
    IS(pin_result(L, true, false, true, 41, 1024, true), 0);         // veto: overlapping, copies expanded afterwards
    IS(hot_bound(L, 96, 1024, 3), 93 * 1024 + 3 * 32768);
    IS(hot_bound(L, 96, 1024, 0), 96 * 1024);
    IS(hot_bound(L, 96, 1024, 96), 96 * 32768);
    IS(hot_bound(L, 10, 4096, 1), 9 * 4096 + 32768);
    // ---- rule 3: hit counters
    IS(hit_counters(true, false, 256, 0, 1000).nw, 4096);  IS(hit_counters(true, false, 256, 0, 1000).iters, 1);
    IS(hit_counters(true, false, 256, 0, 4096).iters, 1);  IS(hit_counters(true, false, 256, 0, 4097).iters, 2);
    IS(hit_counters(false, true, 256, 2, 96).nw, 32);      IS(hit_counters(false, true, 256, 2, 96).iters, 3);
    IS(hit_counters(false, true, 256, 2, 97).iters, 4);
    IS(hit_counters(false, false, 256, 0, 100).nw, 1);     IS(hit_counters(false, false, 256, 0, 100).iters, 100);
    IS(hit_counters(true, true, 3, 2, 100).nw, 48);        // (K1b wins: pfac is K1a's)
    // ---- rule 4: the speculative bound = min(2 * spec_hot, 128, room, n_groups >= 32 ? n_groups / 32 : n_groups), taken when >= spec_hot
    IS(spec_bound(L, 0, false, 16, 96), 0);
    IS(spec_bound(L, 1, false, 16, 96), 2);
    IS(spec_bound(L, 64, true, 16, 4096), 128);
    IS(spec_bound(L, 65, true, 16, 8192), 128);   // 130 -> HOT_INLINE_MAX
    IS(spec_bound(L, 128, true, 16, 8192), 128);
    IS(spec_bound(L, 129, true, 16, 8192), 0);
    IS(spec_bound(L, 1, false, 16, 31), 2);       // fewer than 32 groups: all of them
    IS(spec_bound(L, 1, false, 16, 32), 1);       // 32 / 32
    IS(spec_bound(L, 1, false, 16, 63), 1);
    IS(spec_bound(L, 1, false, 16, 64), 2);
    IS(spec_bound(L, 2, false, 16, 31), 4);
    IS(spec_bound(L, 2, false, 16, 32), 0);       // 1 < 2
    IS(spec_bound(L, 2, false, 16, 63), 0);
    IS(spec_bound(L, 2, false, 16, 64), 2);
    IS(spec_bound(L, 9, false, 16, 4096), 16);    // the context's room: 16 >= 9
    IS(spec_bound(L, 17, false, 16, 4096), 0);    // 16 < 17
    IS(spec_bound(L, 9, true, 16, 4096), 18);     // pinned: the full room
    IS(spec_bound(L, 17, true, 16, 4096), 34);
    // ---- rule 5a: regrow when why == 2, not grown yet, ovf_max * 256 <= 3 * tiles * 64 + (256 << 12)
    IS(regrow_overflow(L, line_of(2, 0, 0, 4096), false, 1), 1);    // 1 048 576 <= 1 048 768
    IS(regrow_overflow(L, line_of(2, 0, 0, 4097), false, 1), 0);    // 1 048 832
    IS(regrow_overflow(L, line_of(2, 0, 0, 4099), false, 4), 1);    // 1 049 344 == 1 049 344
    IS(regrow_overflow(L, line_of(2, 0, 0, 4100), false, 4), 0);    // one list entry above
    IS(regrow_overflow(L, line_of(2, 0, 0, 4864), false, 1024), 1); // 1 245 184 == 1 245 184
    IS(regrow_overflow(L, line_of(2, 0, 0, 4865), false, 1024), 0);
    IS(regrow_overflow(L, line_of(2, 0, 0, 10), true, 1024), 0);    // grown once already
    IS(regrow_overflow(L, line_of(1, 0, 0, 10), false, 1024), 0);   // aborted for another reason
    IS(regrow_overflow(L, line_of(0, 0, 0, 10), false, 1024), 0);
    IS(overflow_room(line_of(2, 0, 0, 4099)), 4099 + 1024 + 64);
    IS(overflow_room(line_of(2, 0, 0, 0)), 64);
    // ---- rule 5b: what the next call speculates on
    IS(next_speculation(L, line_of(0, 3, 0, 7)).hot, 3);   IS(next_speculation(L, line_of(0, 3, 0, 7)).ovf, 7);
    IS(next_speculation(L, line_of(0, 128, 0, 7)).hot, 128);
    IS(next_speculation(L, line_of(0, 129, 0, 7)).hot, 0);
    IS(next_speculation(L, line_of(0, 0, 0, 7)).hot, 0);
    IS(next_speculation(L, line_of(1, 3, 0, 7)).hot, 0);   IS(next_speculation(L, line_of(1, 3, 0, 7)).ovf, 7);
    IS(next_speculation(L, line_of(2, 3, 0, 9)).hot, 0);   IS(next_speculation(L, line_of(2, 3, 0, 9)).ovf, 9);
    // ---- rule 5c: the speculative pipeline is this call's
    IS(spec_is_ours(4, line_of(0, 4, 0, 0)), 1);
    IS(spec_is_ours(4, line_of(0, 5, 0, 0)), 0);
    IS(spec_is_ours(4, line_of(0, 0, 0, 0)), 0);
    IS(spec_is_ours(0, line_of(0, 1, 0, 0)), 0);
    IS(spec_is_ours(4, line_of(1, 2, 0, 0)), 0);
    // ---- rule 5e (and f, g, h): redo wide when !why, K1b, narrow, not tried, not switched off, n_groups >= 32,
    // n_hot * 32 > n_groups, n_ovf * 8 <= hits
    {
        const SparseCall s32{true, false, false, false, false, 32}, s31{true, false, false, false, false, 31},
                         s63{true, false, false, false, false, 63}, s64{true, false, false, false, false, 64};
        const TotalsLine t = line_of(0, 2, 10, 0);
        IS(act(s32, t, false, false, 80), REDO);    // 64 > 32, 80 <= 80
        IS(act(s31, t, false, false, 80), HOT);     // 31 groups
        IS(act(s64, t, false, false, 80), HOT);     // 64 > 64 fails
        IS(act(s63, t, false, false, 80), REDO);    // 64 > 63
        IS(act(s32, t, false, false, 79), HOT);     // 80 <= 79 fails
        IS(act(s32, t, false, false, 81), REDO);
        IS(act(SparseCall{true, true, false, false, false, 32}, t, false, false, 80), HOT);  // wide already
        IS(act(SparseCall{true, false, true, false, false, 32}, t, false, false, 80), HOT);  // tried in this call
        IS(act(SparseCall{true, false, false, true, false, 32}, t, false, false, 80), HOT);  // ACX_NO_WIDE
        IS(act(SparseCall{false, false, false, false, false, 32}, t, false, false, 80), HOT); // K1a
        // the order: the speculative pipeline is counted as a hot call, THEN the call is redone wide
        Verdict v = verdict(s32, t, true, false, 80);
        IS(v.count_hot, 1); IS((ull)v.act, REDO); IS(v.count_regrown, 0);
        v = verdict(s64, t, true, false, 80);       // ... and where the wide form is not due: done
        IS(v.count_hot, 1); IS((ull)v.act, SPEC);
        v = verdict(s32, t, true, true, 80);        // the speculative pipeline gave up: why becomes 1
        IS(v.count_hot, 0); IS((ull)v.act, DENSE);
        v = verdict(s64, t, false, false, 80);
        IS(v.count_hot, 0); IS((ull)v.act, HOT);
        IS(act(s64, line_of(0, 0, 0, 0), false, false, 80), SPARSE);
        IS(act(s64, line_of(1, 0, 0, 0), false, false, 80), DENSE);
        IS(act(s32, line_of(1, 2, 10, 0), false, false, 80), DENSE); // aborted: no wide form either
        IS(act(s32, line_of(2, 2, 10, 0), false, false, 80), DENSE); // the lists could not be regrown
    }
    // ---- rule 5d: overflow_regrown = ovf_grown && why != 2, behind a speculative pipeline that gave up
    {
        const SparseCall g{true, false, false, false, true, 64}, n{true, false, false, false, false, 64};
        Verdict v = verdict(g, line_of(0, 0, 0, 0), false, false, 0);
        IS(v.count_regrown, 1); IS((ull)v.act, SPARSE);
        v = verdict(g, line_of(1, 0, 0, 0), false, false, 0);
        IS(v.count_regrown, 1); IS((ull)v.act, DENSE);
        v = verdict(g, line_of(2, 0, 0, 9), false, false, 0); // too small again: the dense path, not counted
        IS(v.count_regrown, 0); IS((ull)v.act, DENSE);
        v = verdict(g, line_of(0, 2, 0, 0), true, true, 0);
        IS(v.count_regrown, 1); IS(v.count_hot, 0); IS((ull)v.act, DENSE);
        v = verdict(g, line_of(0, 2, 0, 0), true, false, 0);
        IS(v.count_regrown, 1); IS(v.count_hot, 1); IS((ull)v.act, SPEC);
        IS(verdict(n, line_of(0, 0, 0, 0), false, false, 0).count_regrown, 0);
        IS(verdict(n, line_of(1, 0, 0, 0), false, false, 0).count_regrown, 0);
    }
    // ---- rule 6
    IS(grown_hot_inline(L, 16, 16), 16);
    IS(grown_hot_inline(L, 17, 16), 34);
    IS(grown_hot_inline(L, 64, 16), 128);
    IS(grown_hot_inline(L, 65, 16), 128);  // 130 -> 128
    IS(grown_hot_inline(L, 128, 128), 128);
    IS(grown_hot_inline(L, 129, 128), 128);
    IS(dense_everywhere(2, 8), 0);         // 8 > 8 fails
    IS(dense_everywhere(3, 8), 1);
    IS(dense_everywhere(2, 7), 0);         // 8 > 7, but 7 groups
    IS(dense_everywhere(7, 7), 0);
    IS(dense_everywhere(2, 9), 0);
    IS(dense_everywhere(3, 9), 1);
    IS(leave_wide(L, true, 0, 2048, 5), 0); // 10 240 < 10 240 fails
    IS(leave_wide(L, true, 0, 2047, 5), 1);
    IS(leave_wide(L, false, 0, 2047, 5), 0);
    IS(leave_wide(L, true, 1, 2047, 5), 0);
    // ---- rule 7: the density hold
    {
        Hold h = hold_after_dense(Hold{0, false}, 800, 100);   // 800 > 800 fails
        IS(h.calls, 0); IS(h.input, 0);
        h = hold_after_dense(Hold{0, false}, 801, 100);
        IS(h.calls, 8); IS(h.input, 1);
        h = hold_after_dense(hold_dense_input(), 800, 100);    // the input's hold ends with one input that is not dense
        IS(h.calls, 0);
        h = hold_after_dense(hold_gave_up(), 800, 100);        // a give-up's is counted down
        IS(h.calls, 7); IS(h.input, 0);
        h = hold_after_dense(Hold{1, false}, 0, 100);
        IS(h.calls, 0); IS(h.input, 0);
        h = hold_after_dense(hold_gave_up(), 801, 100);        // ... unless the dense path finds the input dense
        IS(h.calls, 8); IS(h.input, 1);
        h = hold_after_dense(Hold{3, true}, 801, 100);
        IS(h.calls, 8); IS(h.input, 1);
        IS(hold_dense_input().calls, 8); IS(hold_dense_input().input, 1);
        IS(hold_gave_up().calls, 8);     IS(hold_gave_up().input, 0);
        IS(dense_form(0, false).compact, 1); IS(dense_form(0, false).dense_full, 0);
        IS(dense_form(1, false).compact, 0); IS(dense_form(1, false).dense_full, 0);
        IS(dense_form(8, false).compact, 0); IS(dense_form(8, false).dense_full, 7);
        IS(dense_form(0, true).compact, 0);  IS(dense_form(0, true).dense_full, 0);
        IS(DENSE_FULL_CALLS, 8);
    }
    // ---- rule 8: the first attempt, the dense form, the attempts
    IS(start_sparse(true, 0, false, 100), 1);
    IS(start_sparse(true, 1, false, 100), 0);
    IS(start_sparse(true, 0, true, 100), 0);
    IS(start_sparse(false, 0, false, 100), 0);
    IS(start_sparse(true, 0, false, (1ull << 26) - 1), 1);
    IS(start_sparse(true, 0, false, 1ull << 26), 0);
    IS(dense_in_tiles(true, true, false, false, 100), 1);
    IS(dense_in_tiles(false, true, false, false, 100), 0);
    IS(dense_in_tiles(true, false, false, false, 100), 0);
    IS(dense_in_tiles(true, true, true, false, 100), 0);
    IS(dense_in_tiles(true, true, false, true, 100), 0);
    IS(dense_in_tiles(true, true, false, false, (1ull << 26) - 1), 1);
    IS(dense_in_tiles(true, true, false, false, 1ull << 26), 0);
    IS(MAX_ATTEMPTS, 6);
    std::printf("cases %u bad %u\n", cases, bad);
    return bad ? 1 : 0;
}
"""


def test_find_policy_at_its_boundaries(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler: the policy cannot be checked")
    src = tmp_path / "find_policy_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "find_policy_check"
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-o", str(exe), str(src)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "cases" and int(last[1]) == 184 and int(last[3]) == 0  # (184: every IS() above, each reached once)
