"""ascii_case_insensitive benchmark: case-sensitive against case-insensitive handles of the same patterns, same box,
alternated, medians.

  python tools/bench_case.py [--steps K] [--warmup W] [--bytes N]

One JSON line:
  device   cfg2 (10 000 patterns a-z, seed 1), a text-like 1 GiB haystack in HBM: acx_find_device waited for, cs_ms / ci_ms,
           their difference (what the fold pass costs the call) and d2d_ms, a device-to-device copy of the same bytes
  host     the same haystack in host memory (acx_find: staged, folded in place on the device): cs_ms / ci_ms
  short    the reference's short loop (10 patterns, 10 000 haystacks of ~75 characters; find_matches_as_indexes per
           haystack): us per call, cs / ci
The kernel time of the fold itself comes from a rocprofv3 --kernel-trace --stats run of this script (k_fold against the
runtime's copy kernel).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def pair_ms(fa, fb, steps, warmup):
    """fa and fb alternated call by call: the medians of both (ms)"""
    for _ in range(warmup):
        fa(); fb()
    ta, tb = [], []
    for _ in range(steps):
        for f, t in ((fa, ta), (fb, tb)):
            t0 = time.perf_counter()
            f()
            t.append(time.perf_counter() - t0)
    return 1e3 * median(ta), 1e3 * median(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bytes", type=int, default=1 << 30)
    args = ap.parse_args()
    import torch
    import gen
    import ahocorasick_rs_amd as ac
    from ahocorasick_rs_amd import capi

    pats = gen.gen_patterns(10000, 5, 12, gen.AZ, 1)
    cs = capi.Automaton(pats, 0, capi.IMPL_DFA)
    ci = capi.Automaton(pats, 0, capi.IMPL_DFA, ascii_case_insensitive=True)
    n = args.bytes
    hay = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    cs.generate(hay.data_ptr(), n, 1, 11)
    torch.cuda.synchronize()

    def find(a):
        def f():
            r = a.find_device(hay.data_ptr(), n)
            r.device_ptr  # (waits for the records)
            r.free()
        return f

    r1, r2 = cs.find_device(hay.data_ptr(), n), ci.find_device(hay.data_ptr(), n)
    assert r1.count == r2.count  # (a-z haystack and patterns: the fold changes nothing)
    matches = r1.count
    r1.free(); r2.free()
    cs_ms, ci_ms = pair_ms(find(cs), find(ci), args.steps, args.warmup)
    dst = torch.empty_like(hay)

    def d2d():
        dst.copy_(hay)
        torch.cuda.synchronize()

    d2d_ms = pair_ms(d2d, d2d, args.steps, args.warmup)[0]
    del dst
    res = {"what": "cs vs ascii_case_insensitive, cfg2 10k patterns, text-like seed 11", "bytes": n, "matches": matches,
           "steps": args.steps,
           "device": {"cs_ms": round(cs_ms, 4), "ci_ms": round(ci_ms, 4), "fold_cost_ms": round(ci_ms - cs_ms, 4),
                      "d2d_ms": round(d2d_ms, 4), "ci_over_cs": round(ci_ms / cs_ms, 4)}}
    host = hay.cpu().numpy()
    hs = max(3, args.steps // 4)
    hcs, hci = pair_ms(lambda: cs.find(host), lambda: ci.find(host), hs, 1)
    res["host"] = {"cs_ms": round(hcs, 3), "ci_ms": round(hci, 3), "ci_over_cs": round(hci / hcs, 4), "steps": hs}
    del host, hay
    short_p = ["abc", "hello", "world", "aardvark", "fish", "what", "arbitrarymonkey", "birds", "host7", "host76"]
    short_h = ["arbitrarymonkey says hello to fish host76, 0.123 my friend, but why??? {}".format(i) for i in range(10_000)]
    A, B = ac.AhoCorasick(short_p), ac.AhoCorasick(short_p, ascii_case_insensitive=True)
    sub = short_h[:2000]
    assert [A.find_matches_as_indexes(h) for h in sub[:50]] == [B.find_matches_as_indexes(h) for h in sub[:50]]
    import gc
    rounds = {"cs": [], "ci": []}
    for _ in range(5):
        for name, X in (("cs", A), ("ci", B)):
            X.find_matches_as_indexes(sub[0])
            gc.collect(); gc.disable()
            t0 = time.perf_counter()
            for h in sub:
                X.find_matches_as_indexes(h)
            rounds[name].append((time.perf_counter() - t0) / len(sub) * 1e6)
            gc.enable()
    res["short"] = {"cs_us": round(median(rounds["cs"]), 2), "ci_us": round(median(rounds["ci"]), 2),
                    "rounds_cs": [round(x, 2) for x in rounds["cs"]], "rounds_ci": [round(x, 2) for x in rounds["ci"]]}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
