"""GPU: what a plain bench.py run prints and what --dump-outputs writes (the last timed step's result, the same as
the library returns for the same seeded input), and that --full still takes the measurements beside the headline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gen

pytestmark = pytest.mark.gpu
capi = pytest.importorskip("ahocorasick_rs_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NBYTES = 64 << 20


def run_bench(*argv, timeout=600):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def load(d, name):
    a = np.load(os.path.join(d, name + ".npy"))
    assert a.dtype == np.float64
    return a


def test_plain_run_dumps_the_last_step(tmp_path):
    d = str(tmp_path / "out")
    out = run_bench("--gpus", "1", "--steps", "4", "--warmup", "1", "--bytes", str(NBYTES), "--dump-outputs", d)
    assert out["steps"] == 4 and out["ms_per_step"] > 0 and out["unit"] == "GB/s" and out["dtype"] == "u8"
    c = out["config"]
    assert "cpu_baseline" not in out and "secondary" not in c and "target_8gib" not in c and c["value_no_settle"] is None
    a = capi.Automaton(gen.gen_patterns(10000, 5, 12, gen.AZ, 1), capi.MATCH_STANDARD, capi.IMPL_DFA)
    buf = capi.DeviceBuffer(NBYTES)
    a.generate(buf.ptr, NBYTES, 1, 11)
    r = a.find_device(buf.ptr, NBYTES)
    want = r.matches()
    r.free()
    assert load(d, "count").tolist() == [len(want)] == [c["matches_per_gpu_step"]] and len(want) > 0
    for k in ("pattern", "start", "end"):
        assert np.array_equal(load(d, k).astype(np.uint64), want[k]), k
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 * 10 ** 6
    a.close()


def test_batch_dump_has_per_haystack_counts(tmp_path):
    d = str(tmp_path / "out")
    out = run_bench("--config", "cfg3", "--steps", "2", "--warmup", "1", "--bytes", str(NBYTES), "--dump-outputs", d)
    counts = load(d, "counts")
    assert len(counts) == NBYTES // 8192 and counts.sum() == load(d, "count")[0] == out["config"]["matches_per_gpu_step"]
    assert len(load(d, "start")) == counts.sum()


def test_full_run_keeps_the_side_measurements():
    out = run_bench("--full", "--steps", "3", "--warmup", "1", "--bytes", str(NBYTES), "--cpu-sample-bytes", str(16 << 20))
    assert out["config"]["value_no_settle"] > 0
    b = out["cpu_baseline"]
    assert b["value"] > 0 and b["sha256_equal_gpu"] is True and b["matches"] == out["config"]["matches_per_gpu_step"]
