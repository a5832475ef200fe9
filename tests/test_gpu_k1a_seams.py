"""GPU: the seams of K1a (kernel=KERNEL_DFA_WALK) in its three forms -- the failureless walk (k1a_scan + k1a_walk), the compact
walk (k1a_walk16) and the chunked walk (k1a_dfa_walk over the dense table, the hot rows in LDS, or the compressed automaton)
-- element-wise against the oracle, on both sinks: the hit slots (path_stats: sparse == the calls, k0 == 0) and the occurrence
regions (ACX_NO_BUCKET, read per call: dense_radix == the calls, dense_tiles == 0 -- K1a has no tile-ordered dense form).

The plan (the sets, the cases, their references, form_of() and what every class claims) is tests/k1a_seams.py, checked on the
CPU by tests/test_k1a_seams_cpu.py.  A class is ONE test per form and sink, with up to 40 failing cases named in the message.
path_stats has no word for the form: the per-form mutants of DESIGN section 8 are the evidence for form_of().  Every
path-asserting call (the 64th hit slot, the region capacity) runs on a handle of its own: a call that gave up holds its handle
for HOLD_CALLS.  The overlapping kind runs first on a fresh handle (tests/test_gpu_post_seams.py explains why).

ACX_NO_PFAC is read once per process: ONE child runs the failureless sets' classes (a), (b), (d) on walk16 / chunked, started
and judged as the K1b children are: a hang, a signal or a device fault in it ends the session, any other failure is stored and
fails its tests without a second start.

The region-capacity cases: an input over the dense capacity as well goes on to the chunked walk; path_stats has no word for
that second attempt (dense_radix counts the call once): the plan's arithmetic and the right answer are the proof.

The second turn of k1a_walk16's grid-stride loop is reachable (test_k1a_seams_cpu.py shows the arithmetic): CUs MiB + 845
bytes, on the hit-slot sink only.  That and class (g)'s 16 W + W / 2 + 1 tiles are the file's only inputs above 64 MiB.

The 64th hit slot: k_tile_main stages STAGE_SLOTS = 24 occurrences a bucket and K1a's hits have no hot pipeline behind them,
so the 63 / 64 / 65-hit tiles of class (e) ALL leave the sparse path (dense_radix == 1 on a fresh handle); the plan holds every
other case to 24 a bucket (k1a_seams.BUCKET).

Measured on the MI355X (256 CUs): the file's 46 tests take 18 .. 20 s alone (the K1b file's 25 s is the yardstick): 2.8 .. 3.6 s
class (a) on the chunked form (w16over's 65 536 states, a handle a kind), 2.4 .. 2.6 s the first test of the ACX_NO_PFAC
child (it pays for all eight), 1.5 .. 1.7 s class (e) (36 fresh handles a kind), 1.0 s the second turn (256 MiB + 845 bytes),
nothing else above 0.9 s; class (g)'s 264 MiB shape well below a second (its rows are the plants: no oracle runs over it).
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import k1a_seams as K

pytestmark = pytest.mark.gpu
capi = pytest.importorskip("ahocorasick_rs_amd.capi")
HERE = os.path.dirname(os.path.abspath(__file__))
SWITCHES = ("ACX_NO_PFAC", "ACX_NO_BUCKET", "ACX_NO_DENSE_TILES", "ACX_DENSE_LIMIT", "ACX_KERNEL", "ACX_NO_SMALL", "ACX_WALK_STATS")
LEGS, NOPFAC_LEGS = K.LEGS, K.NOPFAC_LEGS  # (class, form): constants, held against the plan on the CPU -- no plan at collection


@functools.lru_cache(maxsize=None)
def compute_units() -> int:
    """asked in a process of its own: one process holds ONE HIP runtime, and here the library has loaded it already"""
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return int(r.stdout.split()[-1])


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


_child = {}
FAULT_WORDS = ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR", "hipErrorIllegalAddress", "hipErrorLaunchFailure",
               "Segmentation fault", "core dumped")
CHILD_LIMIT_S = 240


def child():
    """the ACX_NO_PFAC legs, run once in a process of its own: {(class, form, sink): the line's record}"""
    if "r" not in _child:
        _child["r"] = "the child was started and did not return"
        env = {**os.environ, "ACX_NO_PFAC": "1", "PYTHONPATH": os.pathsep.join([os.path.dirname(HERE), HERE])}
        for k in SWITCHES[1:]:
            env.pop(k, None)
        cus = compute_units()
        try:
            r = subprocess.run([sys.executable, os.path.join(HERE, "k1a_seams.py"), str(cus)], env=env, capture_output=True, text=True,
                               timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired as e:
            _child["r"] = "the ACX_NO_PFAC child did not end within %d s and was killed" % CHILD_LIMIT_S
            pytest.exit(_child["r"] + ":\n" + str(e.stderr or "")[-4000:], returncode=3)
        text = r.stdout[-2000:] + r.stderr[-4000:]
        if r.returncode < 0 or r.returncode in (134, 139) or any(w in r.stdout or w in r.stderr for w in FAULT_WORDS):
            _child["r"] = "the ACX_NO_PFAC child ended with %d on a device fault or a signal" % r.returncode
            pytest.exit(_child["r"] + ":\n" + text, returncode=3)
        lines = r.stdout.splitlines()
        if r.returncode != 0 or not lines or lines[-1] != "DONE":
            _child["r"] = "the ACX_NO_PFAC child ended with %d:\n%s" % (r.returncode, text)
        else:
            out = {}
            for ln in lines[:-1]:
                rec = json.loads(ln.split(" ", 1)[1])
                out[(rec["cls"], rec["form"], rec["sink"])] = rec
            _child["r"] = out
    assert isinstance(_child["r"], dict), _child["r"]
    return _child["r"]


def in_process(fn, *args):
    """a leg in this process: an error of the device ends the session (nothing more is started on it), as a child's does"""
    try:
        return fn(*args)
    except capi.AcxError as e:
        pytest.exit("a call failed on the device, the session ends: %s" % e, returncode=3)


def judge(rec):
    print(json.dumps({k: v for k, v in rec.items() if k != "fails"}))
    assert rec["calls"] > 0 and rec["n_fails"] == 0, "%d failing cases, the first:\n%s" % (rec["n_fails"], "\n".join(rec["fails"]))


@pytest.mark.parametrize("sink", K.SINKS)
@pytest.mark.parametrize("cls,form", LEGS, ids=["%s-%s" % p for p in LEGS])
def test_class_on_every_form_and_sink(cls, form, sink):
    """every case of the class meant for the form, all four kinds, element-wise; path_stats exact per handle (run_leg())"""
    judge(in_process(K.run_leg, K.plan(compute_units()), cls, form, sink))


@pytest.mark.parametrize("sink", K.SINKS)
@pytest.mark.parametrize("cls,form", NOPFAC_LEGS, ids=["%s-%s" % p for p in NOPFAC_LEGS])
def test_failureless_sets_on_the_other_forms(cls, form, sink):
    """ACX_NO_PFAC: sets of at most 32 classes on walk16 (one haystack) and on the chunked walk (batches)"""
    judge(child()[(cls, form, sink)])


@pytest.mark.parametrize("name", ["flshort", "w16", "w16over"])
def test_ends_of_the_stream_in_code_points(name):
    """class (a) with codepoints=True at pointer residues 0 and 7, one set a form"""
    fails = in_process(K.run_codepoints, K.plan(compute_units()), name)
    assert not fails, fails


@pytest.mark.parametrize("name", ["fl31", "w16"])
def test_ends_of_the_stream_through_the_python_classes(name):
    """class (a) through BytesAhoCorasick and AhoCorasick, built under ACX_KERNEL=dfa_walk"""
    fails = in_process(K.run_python_classes, K.plan(compute_units()), name)
    assert not fails, fails


def test_the_second_turn_of_walk16():
    """CUs MiB + 845 bytes: the chunks of one turn do not hold the stream, lane 0 walks the rest in a second turn"""
    cus = compute_units()
    c = K.second_turn_case(cus)
    a = K.automaton(c.set, 0)
    fails = []
    for ov in (True, False):
        want = K.expected(c, 0, ov)[0]
        assert len(want) >= cus + 4
        fails += in_process(K.run_case, a, c, 0, ov)[1]
    why = K.check_stats(a.path_stats(), "slots", 2, 0)
    a.close()
    assert not fails and not why, (fails, why)


@pytest.mark.parametrize("shape", K.G_SHAPES)
def test_wave_turns_of_the_failureless_form(shape):
    """class (g), hit-slot sink: 16 x CUs - 1 tiles, that many, one more (the first wave's second turn), and 16 W + W / 2 + 1
    (264 MiB on 256 CUs: every wave stores a full batch of 16 tile counts, W / 2 + 1 of them an epilogue behind it): a plant
    in every tile and across every 16th border, against the plants, under all four kinds"""
    judge(in_process(K.run_turn, K.turn_tiles(compute_units())[shape]))
