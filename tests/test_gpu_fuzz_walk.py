"""A fixed number of seeded cases of tools/gpu_fuzz.py's walk plan run under -m gpu: the three entry points that walk the trie
from an anchor and never take a failure link -- match_at (host input; positions over one haystack, a uniform and a ragged
cut; row starts over a uniform and a ragged cut; overlapping; FULL), segment and wordpiece (host input; one haystack, a
uniform and a ragged cut; SEG_UTF8; continuation prefixes that are "##", empty, one byte, of the alphabet, in no entry and an
entry themselves; four word limits; classes drawn from the alphabet) -- on make_case()'s dictionaries: tries of 10^3 to 10^4
states over 2 letters to all 256 byte values to UTF-8, patterns of up to 68 bytes, identical and nested patterns, x match kind
x ascii_case_insensitive x forced kernel x device pointer residue x cuts with empty rows, one raw *_into_device call between
guard bytes and one handle kept in compressed form only per block.  Every case is held against gpu_fuzz.reference_walk (the
oracle's overlapping rows and numpy; no library code), and so is the host form over the same inputs: when the two differ, that
shows which side is wrong.  tests/test_fuzz_walk_plan_cpu.py checks (without a GPU) the reference against the per-pattern
definitions and what the plan reaches inside the walkers.

Measured on an MI355X: WALK_N = 140 cases (seed 20261025) take 5.7 s, plan included -- 0 failures, 0 build errors, 0 skipped."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_walk_cases_seeded():
    """gpu_fuzz.WALK_N = 140 cases of gpu_fuzz.WALK_SEED = 20261025: 5.7 s on the MI355X it was measured on"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gpu_fuzz
    n = gpu_fuzz.WALK_N
    ran, failures, skipped, build_errors = gpu_fuzz.run_walk(gpu_fuzz.plan_walk(n, gpu_fuzz.WALK_SEED))
    assert failures == 0, f"{failures} of {n} cases differ from the reference (the lines marked FAIL above, each with its first difference)"
    assert build_errors == 0
    assert skipped == 0
    assert ran == n
