"""GPU: the seams of K1b -- the lane, row and tile borders of its index space, the ends of the stream, the lead bytes in
front of a misaligned device pointer, the edges of its output stage and the turns of its waves -- element-wise against the
oracle, in all thirty instantiations launch_prefilter() can launch: the ten scan forms (Q, BIGV, SH) of tests/k1b_seams.py on
the four sinks (hit slots; hit slots + CP; regions, tile-ordered dense form; regions, radix form).

The kernel works on the 16-byte aligned address below the haystack pointer: index = lead + stream position, a lane owns 16
indexes, a row 1 KiB, a tile 4 KiB.  Interior tiles skip the boundary mask; the first tile (lead > 0) and the tiles the
stream ends in apply it (k1b_bounds.hpp).  Every haystack here is device-resident at a chosen residue of its pointer, the
prefilter kernel is forced (K0 never takes a call: acx_path_stats says so).

The plan (the cases, their references, the forms and how each is forced) is tests/k1b_seams.py, checked on the CPU by
tests/test_k1b_seams_cpu.py.  (Q, SH) are proven by info.filter_q and the host tables' n_short there; BIGV 1 and 2 are forced
by ACX_FILTER_BIG, read once per process: ONE child process per value runs all of its (SH, sink) legs, its sweeps and its
bursts and prints a line per leg, the parent asserts on the lines.  The region sinks are forced by ACX_NO_BUCKET (+
ACX_NO_DENSE_TILES), read per call; path_stats names the form every call left by.

The region-capacity cases (test_a_wave_fills_its_region): nothing in path_stats counts the second pass that a full hit
region costs -- dense_tiles / dense_radix count the call once, whichever pass finished it --, so the proof that it ran is
the plan's arithmetic (the hits of the one wave against hit_region_records()) and the right answer.

Measured on the MI355X (256 CUs): the file's 106 tests take 25 s alone -- 5 to 13 s the BIGV = 1 child (its first leg pays
for all of its legs, sweeps and bursts, and for the first start of a process with the library), 2 s the BIGV = 2 child,
0.1 - 0.3 s a (form, sink) leg of 692 - 740 calls, 0.7 s and 0.9 s the 264 MiB shape on the hit-slot sink and with CP (so
the CP leg stays at that shape), everything else below 0.3 s.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import k1b_seams as K
from k1b_seams import ALPHABET, build_case, byte_to_code_point, cols, pattern_sets, pipeline_calls
from oracle_lib import KIND_DFA, Oracle

pytestmark = pytest.mark.gpu
capi = pytest.importorskip("ahocorasick_rs_amd.capi")
HERE = os.path.dirname(os.path.abspath(__file__))

LENGTHS = [1, 4, 5, 16, 1023, 1024, 1025, 4095, 4096, 4097, 8192 + 21]
RESIDUES = [0, 1, 15]
SETS = pattern_sets()


def run(a, o, front, hay, codepoints):
    """the stream at device pointer residue len(front), both match semantics, against the oracle"""
    lead = len(front)
    dev = capi.DeviceBuffer(lead + len(hay) + 16)
    dev.upload(np.frombuffer(front + hay, dtype=np.uint8))
    assert dev.ptr % 16 == 0
    b2c = byte_to_code_point(hay) if codepoints else None
    for ov in (False, True):
        want = o.find_raw(hay, overlapping=ov)
        if codepoints:
            want = np.stack([want[:, 0], b2c[want[:, 1]], b2c[want[:, 2]]], 1) if len(want) else want
        r = a.find_device(dev.ptr + lead, len(hay), overlapping=ov, codepoints=codepoints)
        got = cols(r.matches())
        r.free()
        assert np.array_equal(got, want), (lead, len(hay), ov, len(got), len(want))
    dev.free()


@pytest.mark.parametrize("name", list(SETS))
def test_level1_seams_at_every_length_and_residue(name):
    pats, q, codepoints = SETS[name]
    a = capi.Automaton(pats, 0, kernel=capi.KERNEL_PREFILTER)
    assert a.info.kernel == capi.KERNEL_PREFILTER and a.info.filter_q == q
    o = Oracle(pats, 0, KIND_DFA)
    a.path_stats(reset=True)
    calls = 0
    for n in LENGTHS:
        for lead in RESIDUES:
            for tail_fits in (True, False):
                front, hay = build_case(pats, n, lead, 1000 * n + 10 * lead + tail_fits, tail_fits, codepoints)
                if codepoints:
                    hay.decode("utf-8")
                run(a, o, front, hay, codepoints)
                calls += 2
    st = a.path_stats()
    assert st["k0"] == 0 and pipeline_calls(st) >= calls, st
    a.close()


def test_every_wave_scans_an_interior_tile():
    # 16 MiB + 4 KiB + 7 bytes: 4096 whole tiles for the 4096 waves of a full grid, one more whole tile and a
    # partial one for a second turn; a pattern in every KiB and one across every 4 KiB multiple (the 16 MiB one
    # among them)
    pats, q, _ = SETS["q5"]
    n = (16 << 20) + 4096 + 7
    rng = np.random.default_rng(16)
    buf = ALPHABET[rng.integers(0, len(ALPHABET), n)].copy()
    for k, at in enumerate(range(100, n - 16, 1024)):
        p = pats[k % len(pats)]
        buf[at:at + len(p)] = np.frombuffer(p, dtype=np.uint8)
    for k, at in enumerate(range(4096, n, 4096)):
        p = pats[(5 * k + 1) % len(pats)]
        s = at - 1 - k % (len(p) - 1)  # 1 .. len - 1 bytes in front of the border
        if s + len(p) <= n:
            buf[s:s + len(p)] = np.frombuffer(p, dtype=np.uint8)
    hay = buf.tobytes()
    a = capi.Automaton(pats, 0, kernel=capi.KERNEL_PREFILTER)
    assert a.info.kernel == capi.KERNEL_PREFILTER and a.info.filter_q == q
    o = Oracle(pats, 0, KIND_DFA)
    a.path_stats(reset=True)
    run(a, o, b"", hay, False)
    st = a.path_stats()
    assert st["k0"] == 0 and pipeline_calls(st) >= 2, st
    want = o.find_raw(hay)
    assert len(want) >= (n // 1024) and np.any((want[:, 1] < (16 << 20)) & (want[:, 2] > (16 << 20)))
    a.close()


# ---------------------------------------------------------------------------
# the plan of tests/k1b_seams.py
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def compute_units() -> int:
    """torch.cuda.get_device_properties, asked in a process of its own: one process holds ONE HIP runtime, and here the
    library has loaded it already"""
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return int(r.stdout.split()[-1])


_children = {}  # BIGV -> the child's records, or the text of its failure: a child is started ONCE a session, whatever it does
FAULT_WORDS = ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR", "hipErrorIllegalAddress", "hipErrorLaunchFailure",
               "Segmentation fault", "core dumped")
CHILD_LIMIT_S = 300  # (measured: 2 - 13 s)


def child(bigv: int):
    """every leg of one BIGV, run once in a process of its own: {("LEG" | "SWEEP" | "TURN", key): the line's record}.  A
    child that hangs, dies of a signal or names a device fault ends the session: nothing more is started on the device.
    Any other failure is stored, and every test of that BIGV fails on the stored text without starting the child again."""
    if bigv not in _children:
        _children[bigv] = "the child was started and did not return"  # (whatever is raised below: not a second time)
        env = {**os.environ, "ACX_FILTER_BIG": str(bigv), "PYTHONPATH": os.pathsep.join([os.path.dirname(HERE), HERE])}
        for k in ("ACX_NO_BUCKET", "ACX_NO_DENSE_TILES"):
            env.pop(k, None)
        cus = compute_units()
        try:
            r = subprocess.run([sys.executable, os.path.join(HERE, "k1b_seams.py"), str(bigv), str(cus)], env=env,
                               capture_output=True, text=True, timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired as e:  # (subprocess.run has killed it)
            _children[bigv] = "the ACX_FILTER_BIG=%d child did not end within %d s and was killed" % (bigv, CHILD_LIMIT_S)
            pytest.exit(_children[bigv] + ":\n" + str(e.stderr or "")[-4000:], returncode=3)
        text = r.stdout[-2000:] + r.stderr[-4000:]
        if r.returncode < 0 or r.returncode in (134, 139) or any(w in r.stdout or w in r.stderr for w in FAULT_WORDS):
            _children[bigv] = "the ACX_FILTER_BIG=%d child ended with %d on a device fault or a signal" % (bigv, r.returncode)
            pytest.exit(_children[bigv] + ":\n" + text, returncode=3)
        lines = r.stdout.splitlines()
        if r.returncode != 0 or not lines or lines[-1] != "DONE":
            _children[bigv] = "the ACX_FILTER_BIG=%d child ended with %d:\n%s" % (bigv, r.returncode, text)
        else:
            out = {}
            for ln in lines[:-1]:
                kind, rec = ln.split(" ", 1)
                rec = json.loads(rec)
                out[(kind, rec["form"], rec.get("sink"), rec.get("where"), rec.get("pair"))] = rec
            _children[bigv] = out
    assert isinstance(_children[bigv], dict), _children[bigv]
    return _children[bigv]


@pytest.mark.parametrize("sink", K.SINKS)
@pytest.mark.parametrize("form", K.FORMS, ids=lambda f: f.name)
def test_position_classes_on_every_form_and_sink(form, sink, monkeypatch):
    """all four kinds on every position class; k0 == 0 and the sink's proof from path_stats inside run_leg()"""
    if form.bigv:
        rec = child(form.bigv)[("LEG", form.name, sink, None, None)]
    else:
        for k in ("ACX_NO_BUCKET", "ACX_NO_DENSE_TILES"):
            monkeypatch.delenv(k, raising=False)
        rec = K.run_leg(form, sink)
    print(json.dumps({k: v for k, v in rec.items() if k != "fails"}))
    assert rec["calls"] == K.leg_calls(form.set, sink) and not rec["fails"], rec["fails"]


@pytest.mark.parametrize("where", K.SWEEP_TILES)
@pytest.mark.parametrize("form", K.FORMS, ids=lambda f: f.name)
def test_overflow_staircase_around_the_hit_slots(form, where):
    """HIT_SLOTS - 4 .. HIT_SLOTS + 4 hits in the first tile behind 15 lead bytes, an interior tile, the stream's last, partial
    tile and a group's last tile: equal to the oracle at every k; overflow_hits 0, ..., 0, 1, 2, ... (K.staircase).  SH forms:
    also with the pair "a" + "ab", whose two hits straddle the last slot at every other k."""
    for pair in ((False, True) if form.sh else (False,)):
        rec = child(form.bigv)[("SWEEP", form.name, None, where, pair)] if form.bigv else K.run_sweep(form, where, pair)
        print(json.dumps({k: v for k, v in rec.items() if k != "fails"}))
        assert not rec["fails"], rec["fails"]
        assert rec["overflow_hits"][0] == 0 and 1 in rec["overflow_hits"]


@pytest.mark.parametrize("form", K.FORMS, ids=lambda f: f.name)
def test_two_batches_of_one_wave_fill_the_burst_buffer(form):
    """16 * CUs + 2 tiles: the first two waves take a second turn, and their two batches hold HB and HB + 1 hits together"""
    rec = child(form.bigv)[("TURN", form.name, None, None, None)] if form.bigv else K.run_turn_bursts(form, compute_units())
    assert not rec["fails"], rec["fails"]


@pytest.mark.parametrize("sink", ["regions_tiles", "regions_radix"])
def test_a_wave_fills_its_region(sink, monkeypatch):
    """one tile of 'a' under "a" + "aa": ONE wave pushes the region's records minus one, the records, one more, and nearly
    two per byte of the tile (hit_region_records(): max(65 536, n / 64) records over 16 regions = 4 096 on a handle's first
    dense call).  A fresh handle per case, so that the regions have their first size.  path_stats has no word for the
    second pass (module docstring): the answer is the proof.  The tile-ordered form may hand a call of this density (two
    occurrences a byte) to the radix form: either may finish it, K0 and the hit slots may not."""
    cus = compute_units()
    for k, v in K.SINK_ENV[sink].items():
        monkeypatch.setenv(k, v)
    pats = list(K.region_set())
    o = Oracle(pats, 0, KIND_DFA)
    for name, hay, hits in K.region_cases(cus):
        assert K.hit_region_records(len(hay), 1, cus) == 4096
        d = K.Device(K.FORM["q5sh"], pats=pats, set_name="region")
        d.auto(0)
        d.reset()
        calls = d.run(name, b"", hay, [(0, False), (0, True)], False, lambda mk, ov: o.find_raw(hay, overlapping=ov))
        st = d.stats()
        d.close()
        print(name, hits, st)
        assert not d.fails, d.fails
        assert st["k0"] == 0 and st["sparse"] + st["hot_calls"] == 0 and st["dense_tiles"] + st["dense_radix"] == calls, st
        if sink == "regions_radix":
            assert st["dense_tiles"] == 0, st


def turn_run(set_name, hay, codepoints):
    a = capi.Automaton(list(K.patterns(set_name)), 0, kernel=capi.KERNEL_PREFILTER)
    assert a.info.kernel == capi.KERNEL_PREFILTER and a.info.filter_q == 5
    want = K.expected(set_name, hay, 0, False)
    if codepoints:
        want = np.stack([want[:, 0], K.code_points_at(hay, want[:, 1]), K.code_points_at(hay, want[:, 2])], 1)
    dev = capi.DeviceBuffer(len(hay) + 16)
    dev.upload(hay)
    a.path_stats(reset=True)
    r = a.find_device(dev.ptr, len(hay), codepoints=codepoints)
    got = cols(r.matches())
    r.free()
    dev.free()
    st = a.path_stats()
    a.close()
    assert st["k0"] == 0 and st["sparse"] + st["hot_calls"] == 1, st
    assert np.array_equal(got, want), (len(got), len(want))
    return want


@pytest.mark.parametrize("tiles", ["w-1", "w", "w+1"])
@pytest.mark.parametrize("codepoints", [False, True], ids=["slots", "cp"])
def test_the_grid_stops_growing(tiles, codepoints):
    """16 * CUs - 1, that many, one more tile: every wave one tile; the first wave a second turn"""
    cus = compute_units()
    hay = K.turn_hay("s5", K.turn_tiles(cus)[tiles], cus, multibyte=codepoints)
    want = turn_run("s5", hay, codepoints)
    assert len(want) >= K.turn_tiles(cus)[tiles] - 1


@pytest.mark.parametrize("codepoints", [False, True], ids=["slots", "cp"])
def test_the_counts_leave_sixteen_at_a_time(codepoints):
    """16 W + W / 2 + 1 tiles (W = 16 * CUs waves; 264 MiB on 256 CUs): every wave stores one full batch of 16 tile counts,
    W / 2 + 1 of them an epilogue of one count behind it, the others none; the last tile is partial.  The smallest shape at
    which the batch store and an epilogue behind a batch run at all.  A lost or misplaced count drops a tile's hits: one
    plant in every tile, one across every 16th border, element-wise."""
    cus = compute_units()
    tiles = K.turn_tiles(cus)["counts"]
    b = K.count_batches(tiles, cus)
    assert b["full"] == 16 * cus and b["epilogue_behind_batch"] == 8 * cus + 1 and b["remainders"] == [0, 1]
    hay = K.turn_hay("s5", tiles, cus, multibyte=codepoints)
    want = turn_run("s5", hay, codepoints)
    assert len(want) >= tiles - 1
