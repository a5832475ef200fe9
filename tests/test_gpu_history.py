"""GPU: a handle's history -- every path transition of a context, call by call (tests/history.py).

Every other GPU test treats a call as if it were its handle's first.  Here one handle runs a SEQUENCE of calls under each match
kind; acx_path_stats is reset in front of every call, and after it the rows are compared element-wise with the oracle and the
counters' deltas with the model of tests/history.py (Context: csrc/find_policy.hpp composed in the order csrc/find_attempts.cpp
calls it; tests/test_history_cpu.py pins that model against the header's own functions and proves the inputs' classes from
the oracle's rows).  The sequences: A the wide form taken, kept and left (and the buffers regrown behind it), B the hold after
a give-up counted out, C the hold after a dense input, D the full dense form's countdown, E what the next call queues ahead
and when a host haystack is read in place, G the overflow lists regrown and reused, H the pinned result's boundary, J the
same behind one more call (the other control block), K small calls between large ones.

ACX_NO_SPEC_HOT is read once per process: ONE child runs E and K again without the hot pipeline queued ahead, and the parent
asserts on its lines.  A child that hangs, dies of a signal or names a device fault ends the session; any other failure is
stored and fails its tests without a second start.
"""
import json
import os
import subprocess
import sys

import pytest

import history as H

pytestmark = pytest.mark.gpu
capi = pytest.importorskip("ahocorasick_rs_amd.capi")
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("kind", range(len(H.KINDS)), ids=H.KIND_NAMES)
@pytest.mark.parametrize("name", list(H.PLAN))
def test_a_sequence_on_one_handle_call_by_call(name, kind):
    rec = H.run_sequence(name, kind)
    print(json.dumps(rec["log"]))
    assert rec["calls"] == len(H.PLAN[name]) and not rec["fails"], rec["fails"]


_child = None  # the child's records, or the text of its failure: started ONCE a session, whatever it does
FAULT_WORDS = ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR", "hipErrorIllegalAddress", "hipErrorLaunchFailure",
               "Segmentation fault", "core dumped")
CHILD_LIMIT_S = 300


def child():
    global _child
    if _child is None:
        _child = "the child was started and did not return"
        env = {**os.environ, "ACX_NO_SPEC_HOT": "1", "PYTHONPATH": os.pathsep.join([os.path.dirname(HERE), HERE])}
        try:
            r = subprocess.run([sys.executable, os.path.join(HERE, "history.py")], env=env, capture_output=True, text=True,
                               timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired as e:  # (subprocess.run has killed it)
            _child = "the ACX_NO_SPEC_HOT child did not end within %d s and was killed" % CHILD_LIMIT_S
            pytest.exit(_child + ":\n" + str(e.stderr or "")[-4000:], returncode=3)
        text = r.stdout[-2000:] + r.stderr[-4000:]
        if r.returncode < 0 or r.returncode in (134, 139) or any(w in r.stdout or w in r.stderr for w in FAULT_WORDS):
            _child = "the ACX_NO_SPEC_HOT child ended with %d on a device fault or a signal" % r.returncode
            pytest.exit(_child + ":\n" + text, returncode=3)
        lines = r.stdout.splitlines()
        if r.returncode != 0 or not lines or lines[-1] != "DONE":
            _child = "the ACX_NO_SPEC_HOT child ended with %d:\n%s" % (r.returncode, text)
        else:
            recs = [json.loads(ln.split(" ", 1)[1]) for ln in lines[:-1] if ln.startswith("SEQ ")]
            _child = {(rec["name"], rec["kind"]): rec for rec in recs}
    assert isinstance(_child, dict), _child
    return _child


@pytest.mark.parametrize("kind", range(len(H.KINDS)), ids=H.KIND_NAMES)
@pytest.mark.parametrize("name", H.NO_SPEC_SEQUENCES)
def test_the_same_without_the_hot_pipeline_queued_ahead(name, kind):
    rec = child()[(name, kind)]
    print(json.dumps(rec["log"]))
    assert rec["calls"] == len(H.PLAN[name]) and not rec["fails"], rec["fails"]
