"""keep_mask16 (csrc/k1b_bounds.hpp), the boundary mask of K1b's level 1, against its definition.

A stand-alone C++ program with its own main includes the header and compares the helper with the
16-iteration loop it replaced in the kernel -- bit j iff lo <= p0 + j <= hi -- exhaustively over
p0 = 0 .. 8192 step 16, lo = 0 .. 15 and the hi values at which a tile, a row or the stream ends,
hi < lo (empty) among them.  No GPU.
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
#include "k1b_bounds.hpp"

static uint32_t by_definition(uint64_t p0, uint64_t lo, uint64_t hi) {
    uint32_t keep = 0;
    for (int j = 0; j < 16; j++)
        if (p0 + j >= lo && p0 + j <= hi) keep |= 1u << j;
    return keep;
}

int main() {
    const uint64_t his[] = {0, 1, 15, 16, 17, 4095, 4096, 4097, 8191, ~0ull - 16};
    unsigned long long cases = 0, empty = 0, bad = 0;
    for (uint64_t p0 = 0; p0 <= 8192; p0 += 16)
        for (uint64_t lo = 0; lo <= 15; lo++)
            for (uint64_t hi : his) {
                const uint32_t want = by_definition(p0, lo, hi), got = acx::keep_mask16(p0, lo, hi);
                cases++;
                if (hi < lo) {
                    empty++;
                    if (want != 0) { std::printf("the definition is not empty for hi < lo\n"); return 2; }
                }
                if (got != want && bad++ < 10)
                    std::printf("p0=%llu lo=%llu hi=%llu: got %04x, want %04x\n", (unsigned long long)p0,
                                (unsigned long long)lo, (unsigned long long)hi, got, want);
            }
    std::printf("cases %llu empty %llu bad %llu\n", cases, empty, bad);
    return bad ? 1 : 0;
}
"""


def test_keep_mask16_matches_its_definition(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler: the helper cannot be checked")
    src = tmp_path / "k1b_bounds_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "k1b_bounds_check"
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-o", str(exe), str(src)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    last = r.stdout.strip().splitlines()[-1].split()
    # 513 values of p0 x 16 of lo x 10 of hi; hi < lo occurs (hi = 0, 1 against lo up to 15)
    assert int(last[1]) == 513 * 16 * 10 and int(last[3]) > 0 and int(last[5]) == 0
