"""A fixed number of seeded cases of tools/gpu_fuzz.py's surface run under -m gpu: every entry point (find, find_batch,
find_device with one haystack / a uniform / a ragged batch, replace on either route, replace_batch, replace_device in its
three forms) x match kind x ascii_case_insensitive x device pointer residue x batch cuts with empty haystacks x
replacement lengths, against the oracle and a plain splice.  The same SURFACE_N cases on every box: a case count, not a
time budget; tests/test_fuzz_plan_cpu.py checks (without a GPU) what the plan covers and that no case can be skipped.

Measured on an MI355X: SURFACE_N = 176 cases (seed 20261016) take 8.1 s, plan included -- 0 failures, 0 build errors,
0 skipped; the time-budgeted slice beside it (tests/test_gpu_fuzz.py) is given 60 s."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_surface_cases_seeded():
    """gpu_fuzz.SURFACE_N = 176 cases of gpu_fuzz.SURFACE_SEED = 20261016: 8.1 s on the MI355X it was measured on"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gpu_fuzz
    n = gpu_fuzz.SURFACE_N
    ran, failures, skipped, build_errors = gpu_fuzz.run_surface(gpu_fuzz.plan_surface(n, gpu_fuzz.SURFACE_SEED))
    assert failures == 0, f"{failures} of {n} cases differ from the reference (the lines marked FAIL above)"
    assert build_errors == 0
    assert skipped == 0
    assert ran == n
