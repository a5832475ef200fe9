"""GPU: K0 (kernels.hip k0_call<MODE>: a whole small call in one workgroup) at its seams -- wave 0's finish at 63 / 64 / 65
occurrences, the result lines at 5 | 6, 11 | 12, 17 | 18, 23 | 24 | 25 matches with two haystacks alternating on one handle,
the dense cut at SMALL_MAX_OCC, every length at which the code takes another path, MODE 2's windows and work limit, the
poll's widths along sequences of lengths, code points over fillers of every width, chains in the general finish --
element-wise against the oracle, in every mode and on every route.

The plan (sets, haystacks, the mode every call is meant for, the routes) is tests/k0_seams.py, checked on the CPU by
tests/test_k0_seams_cpu.py.  Routes: "resident" (this process: the mailbox and k0_resident), "device" (this process:
find_device, seq == 0, unpacked records, pointer residues 0, 1, 8, 15 between guard bytes), "launched" (ONE child under
ACX_NO_RESIDENT=1: k0_small for every call) and "nopf" (ONE child under ACX_K0_NO_PREFILTER=1: the walk modes on large
automata beyond 1 KiB; beyond SMALL_MAX_LEN the pipeline answers, k0 == 0).  Both switches are read once per process.

A class is ONE test per mode and route: its groups run once (each an ordered list of calls on one handle per kind) and the
test reads the fails of the calls meant for its mode, and what path_stats said of their groups: k0 == the calls K0 is to
answer, the pipeline's calls == the others (the dense cut's last call, the lengths beyond K0's reach), resident_launches
>= 1 here and == 0 in the ACX_NO_RESIDENT child and on the device route.  path_stats has no word for the mode: DESIGN section 8
shows by mutants of one mode each that the classes run the mode they claim."""
import json
import os
import subprocess
import sys

import pytest

import k0_seams as P

pytestmark = pytest.mark.gpu
capi = pytest.importorskip("ahocorasick_rs_amd.capi")
HERE = os.path.dirname(os.path.abspath(__file__))
SWITCHES = ("ACX_NO_RESIDENT", "ACX_K0_NO_PREFILTER", "ACX_NO_SMALL", "ACX_DENSE_LIMIT", "ACX_RESIDENT_LIFE_US", "ACX_RESIDENT_IDLE_US",
            "ACX_EXPAND_COPIES", "ACX_KERNEL")

# the two switches are per-process statics of the library: what counts is what the SESSION was started with -- read here, at
# import, before the fixture below takes them out of os.environ
AT_START = {k: os.environ.get(k) for k in ("ACX_NO_RESIDENT", "ACX_K0_NO_PREFILTER", "ACX_NO_SMALL")}

_children = {}  # route -> the child's records, or the text of its failure: a child is started ONCE a session, whatever it does
FAULT_WORDS = ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR", "hipErrorIllegalAddress", "hipErrorLaunchFailure",
               "Segmentation fault", "core dumped")
CHILD_LIMIT_S = 240  # (measured: see DESIGN section 8)


def child(route: str):
    """every group of one route, run once in a process of its own: the records in the plan's order.  A child that hangs,
    dies of a signal or names a device fault ends the session: nothing more is started on the device.  Any other failure is
    stored, and every test of that route fails on the stored text without starting the child again."""
    if route not in _children:
        _children[route] = "the child was started and did not return"  # (whatever is raised below: not a second time)
        env = {**os.environ, "PYTHONPATH": os.pathsep.join([os.path.dirname(HERE), HERE])}
        for k in SWITCHES:
            env.pop(k, None)
        env[P.ROUTE_ENV[route]] = "1"
        try:
            r = subprocess.run([sys.executable, os.path.join(HERE, "k0_seams.py"), route], env=env, capture_output=True, text=True,
                               timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired as e:  # (subprocess.run has killed it)
            _children[route] = "the %s child did not end within %d s and was killed" % (route, CHILD_LIMIT_S)
            pytest.exit(_children[route] + ":\n" + str(e.stderr or "")[-4000:], returncode=3)
        text = r.stdout[-2000:] + r.stderr[-4000:]
        if r.returncode < 0 or r.returncode in (134, 139) or any(w in r.stdout or w in r.stderr for w in FAULT_WORDS):
            _children[route] = "the %s child ended with %d on a device fault or a signal" % (route, r.returncode)
            pytest.exit(_children[route] + ":\n" + text, returncode=3)
        lines = r.stdout.splitlines()
        if r.returncode != 0 or not lines or lines[-1] != "DONE" or len(lines) - 1 != len(P.route_groups(route)):
            _children[route] = "the %s child ended with %d:\n%s" % (route, r.returncode, text)
        else:
            _children[route] = [json.loads(ln.split(" ", 1)[1]) for ln in lines[:-1]]
    assert isinstance(_children[route], list), _children[route]
    return _children[route]


@pytest.fixture(autouse=True)
def no_switch(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("route,cls,mode", [(r, c, md) for r in P.ROUTES for c, md in P.tests_of(r)],
                         ids=lambda v: v if isinstance(v, str) else "mode%d" % v if v >= 0 else "not_k0")
def test_class_in_every_mode_on_every_route(route, cls, mode):
    """(a) 63, 64, 65 occurrences in 1 024 and 1 025 bytes, planted forwards and mirrored, 64 chained and 64 covered ones;
    (b) 0 .. 65 matches at the lines' limits, haystacks A B A B; (c) SMALL_MAX_OCC - 1, SMALL_MAX_OCC, one more (the pipeline's);
    (d) every length of the plan: flush with both ends, cut by the end, NULs in the zero fill, a thread's stride, shorter than
    every pattern; (e) every pattern length at every pos & 7, near misses, the work limit as a loop of 40 calls; (f) sequences
    of lengths, code points on and off, a case-insensitive handle; (g) code points; (i) chains and the sync scan's stop"""
    groups = P.route_groups(route)
    if route in P.ROUTE_ENV:
        records = child(route)
    else:
        assert all(v is None for v in AT_START.values()), f"this process was started with {AT_START}: its routes are not the plan's"
        records = [P.ran(g, route) if mode in P.group_modes(g, route) and g.cls == cls else None for g in groups]
        groups, records = [g for g, r in zip(groups, records) if r], [r for r in records if r]
    assert [(r["cls"], r["set"], r["name"]) for r in records] == [(g.cls, g.set, g.name) for g in groups]
    per = len(P.RESIDUES) if route == "device" else 1
    assert all(r["calls"] == len(P.KINDS) * per * len(g.calls) for g, r in zip(groups, records))
    n, fails = P.verdict(records, groups, route, cls, mode)
    assert not n, (n, fails)


@pytest.mark.parametrize("g", [g for g in P.plan() if g.cls in ("b", "g")], ids=lambda g: f"{g.cls}-{g.set}")
def test_lines_and_code_points_through_the_python_classes(g):
    """classes (b) and (g), every set of theirs (MODE 2, 1, 0 dense and compressed, 3), through BytesAhoCorasick and AhoCorasick
    (str: code-point indexes), every kind"""
    fails = P.run_group_py(g)
    assert not fails, (len(fails), fails[:40])
