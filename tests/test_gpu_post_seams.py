"""GPU: the order and match-kind stage at its limits -- k_tile_main's bucket slots, group stretches, accept masks, certified
sync points and chains; k_tile_write's chunks, places and per-haystack runs -- element-wise against the oracle and against
the path the plan names (path_stats), in the three forms of k_tile_main that tile_post() launches for byte offsets: narrow
words (STAGE_SLOTS_W32 slots, 128 threads), 64-bit words (STAGE_SLOTS slots, 256 threads) and the wide form
(STAGE_SLOTS_WIDE slots, 64-bit flag masks, GROUP_MAX_WIDE matches a group).

The plan (cases, references, expected paths, and how each form is forced) is tests/post_seams.py, checked on the CPU by
tests/test_post_seams_cpu.py.  The narrow form is what the plan's tiny sets get by themselves and runs in this process;
ACX_MAIN_WIDE and ACX_FORCE_WIDE are read once per process: ONE child per switch runs all of its classes, batches and
sequences and prints a line each, the parent asserts on the lines.  Every call that asserts a path runs on a fresh handle
(post_seams.run_case()); the sequences keep one handle and state their order.

Three further children, one switch each (post_seams.LEGS): ACX_NO_DENSE_COMPACT (k_dense_main's full form for the dense-path
cases of class h), ACX_NO_SPEC_HOT (the ladder with nothing queued ahead) and ACX_NO_WIDE (HOT_INLINE and HOT_INLINE + 1 hot
groups against the output's room).  A class is ONE test a form: its calls share the child and the oracle's rows.

path_stats does not name the form: post_seams.source_constants() pins where tile_post() chooses it, and the staircases
themselves tell the forms apart -- 28 keys to a bucket are sparse in the narrow form and hot in the 64-bit-word one, 29 are hot
in both and sparse in the wide one.
"""
import json
import os
import subprocess
import sys

import pytest

import k1b_seams as K
import post_seams as P

pytestmark = pytest.mark.gpu
capi = pytest.importorskip("ahocorasick_rs_amd.capi")
HERE = os.path.dirname(os.path.abspath(__file__))
SWITCHES = ("ACX_MAIN_WIDE", "ACX_FORCE_WIDE", "ACX_NO_WIDE", "ACX_NO_BUCKET", "ACX_NO_DENSE_COMPACT", "ACX_NO_DENSE_TILES", "ACX_NO_SPEC_HOT")

_children = {}  # form -> the child's records, or the text of its failure: a child is started ONCE a session, whatever it does
FAULT_WORDS = ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR", "hipErrorIllegalAddress", "hipErrorLaunchFailure",
               "Segmentation fault", "core dumped")
CHILD_LIMIT_S = 240  # (measured: see DESIGN section 8)


def child(form: str):
    """every class, batch and sequence of one form, run once in a process of its own: {class: the line's record}.  A child
    that hangs, dies of a signal or names a device fault ends the session: nothing more is started on the device.  Any
    other failure is stored, and every test of that form fails on the stored text without starting the child again."""
    if form not in _children:
        _children[form] = "the child was started and did not return"  # (whatever is raised below: not a second time)
        env = {**os.environ, "PYTHONPATH": os.pathsep.join([os.path.dirname(HERE), HERE])}
        for k in SWITCHES:
            env.pop(k, None)
        env[P.FORM[form].env] = "1"
        try:
            r = subprocess.run([sys.executable, os.path.join(HERE, "post_seams.py"), form], env=env, capture_output=True, text=True,
                               timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired as e:  # (subprocess.run has killed it)
            _children[form] = "the %s child did not end within %d s and was killed" % (form, CHILD_LIMIT_S)
            pytest.exit(_children[form] + ":\n" + str(e.stderr or "")[-4000:], returncode=3)
        text = r.stdout[-2000:] + r.stderr[-4000:]
        if r.returncode < 0 or r.returncode in (134, 139) or any(w in r.stdout or w in r.stderr for w in FAULT_WORDS):
            _children[form] = "the %s child ended with %d on a device fault or a signal" % (form, r.returncode)
            pytest.exit(_children[form] + ":\n" + text, returncode=3)
        lines = r.stdout.splitlines()
        if r.returncode != 0 or not lines or lines[-1] != "DONE":
            _children[form] = "the %s child ended with %d:\n%s" % (form, r.returncode, text)
        else:
            _children[form] = {json.loads(ln.split(" ", 1)[1])["cls"]: json.loads(ln.split(" ", 1)[1]) for ln in lines[:-1]}
    assert isinstance(_children[form], dict), _children[form]
    return _children[form]


@pytest.fixture(autouse=True)
def no_switch(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("form,cls", [(f, cls) for f in P.FORMS + P.LEGS for cls in P.CLASSES if P.cases_of(f.name, cls)],
                         ids=lambda v: v if isinstance(v, str) else v.name)
def test_class_in_every_form(form, cls):
    """(a) SLOTS - 1, SLOTS, SLOTS + 1 keys in one bucket: hot_groups 0, 0, 1 (2 where the next group stages the bucket too);
    (b) GROUP_MAX - 1, GROUP_MAX, GROUP_MAX + 1 matches in one group, the wide form's full house and one more; (c) touching and
    overlapping pairs over the borders, chains from the first certifiable byte and the one in front, the longest pattern of
    every lookback, one beyond; (e) groups of 1 .. GROUP_MAX (the wide form: GROUP_MAX_WIDE) matches around the write kernel's
    chunks, and the same as code points; (d) another number of hits in every staged tile, lookback 1 and 4: the prefix across
    the waves' halves; (g, the ACX_NO_WIDE child) HOT_INLINE and HOT_INLINE + 1 hot groups of 69: the output's room; (f) 131 groups, the two at the border of supergroups 0 and 1 hot; (h, k_dense_main has one form of words: this process only) bucket fills around sort_bucket's thresholds and DT_SLOTS,
    DT_COMPACT_WORDS staged words and one more, pairs over a dense group's border, a long occurrence over 250 short ones -- as
    the dense path proper (ACX_NO_BUCKET; again in the ACX_NO_DENSE_COMPACT child: the full form) and as the hot pipeline's tail"""
    rec = child(form.name)[cls] if form.env else P.run_class(form.name, cls)
    print(json.dumps({k: v for k, v in rec.items() if k != "fails"}))
    assert rec["calls"] == sum(len(c.kinds) for c in P.cases_of(form.name, cls)) and not rec["fails"], (rec["n_fails"], rec["fails"])


@pytest.mark.parametrize("how", ["device", "host"])
@pytest.mark.parametrize("b", P.batches(), ids=lambda b: b.name)
@pytest.mark.parametrize("form", P.FORMS, ids=lambda f: f.name)
def test_batch_counts_per_haystack(form, b, how):
    """haystack borders behind matches 250, 255, 256, 257, 260 and 512 of a group's stretch, two empty haystacks at the chunk
    border, a run the chunk border cuts; 300 one-match haystacks in one group: rows local to their haystack and the counts
    per haystack, element-wise, from device memory (offsets / row length) and from host memory"""
    fails = child(form.name)[b.name + "_" + how]["fails"] if form.env else P.run_batch(b, how)
    assert not fails, fails


@pytest.mark.parametrize("kind", K.KINDS, ids=lambda k: "kind%d_ov%d" % (k[0], int(k[1])))
@pytest.mark.parametrize("form", P.FORMS, ids=lambda f: f.name)
def test_sequence_on_one_handle(form, kind):
    """six streams, each twice in a row, then all in reverse, on ONE handle: both parities of the call's sequence number
    behind a sparse call, a hot one (the next call queues the hot pipeline ahead) and one of another size"""
    mk, ov = kind
    fails = child(form.name)[f"seq_{mk}_{int(ov)}"]["fails"] if form.env else P.run_sequence(form.name, mk, ov)
    assert not fails, fails


@pytest.mark.parametrize("kind", K.KINDS, ids=lambda k: "kind%d_ov%d" % (k[0], int(k[1])))
@pytest.mark.parametrize("form", P.FORMS, ids=lambda f: f.name)
def test_hot_pipeline_queued_ahead_at_its_bound(form, kind):
    """one handle, five groups: 1 hot group, then 2 (the bound the call behind 1 computes: the queued pipeline is the call's),
    then 5 (the bound behind 2, + 1: its kernels return and the host runs the pipeline), then none, then 1; hot_groups exact"""
    mk, ov = kind
    fails = child(form.name)[f"ladder_{mk}_{int(ov)}"]["fails"] if form.env else P.run_sequence(form.name, mk, ov, "ladder")
    assert not fails, fails
    if not form.env:  # ... and with nothing queued ahead (the ACX_NO_SPEC_HOT child): the same rows and counts at every step
        fails = child("nospec")[f"ladder_{mk}_{int(ov)}"]["fails"]
        assert not fails, fails


@pytest.mark.parametrize("kind", K.KINDS, ids=lambda k: "kind%d_ov%d" % (k[0], int(k[1])))
@pytest.mark.parametrize("form,which", [(f, w) for f in P.FORMS for w in ("grow", "redo") if w == "grow" or f.gmax == P.GROUP_MAX],
                         ids=lambda v: v if isinstance(v, str) else v.name)
def test_workspace_and_wide_redo_on_one_handle(form, which, kind):
    """grow: a 3-tile stream, the 131-group stream of (f), the small one twice (either parity of the call's number finds its
    set of supergroup words clear although sg_cap is now larger than n_super), a hot call, the small one.  redo (the two
    forms of GROUP_MAX): a hot call, a 32-group stream with two hot groups -- redone in the wide form, wide_redone == 1,
    sparse there, and the context goes back to the narrow form --, the hot call again, both again (under ACX_FORCE_WIDE no
    call is REdone wide: no such sequence for that form)"""
    mk, ov = kind
    fails = child(form.name)[f"{which}_{mk}_{int(ov)}"]["fails"] if form.env else P.run_sequence(form.name, mk, ov, which)
    assert not fails, fails
