"""Replacement benchmark (acx_replace_device vs acx_find_device on the same device haystack, same box).

  python tools/bench_replace.py [--steps K] [--warmup W] [--every 0|64|32] [--bytes N] [--routes]

One JSON line: the median wall time per call of
  find_ms      acx_find_device, waited for (the records complete), freed
  replace_ms   acx_replace_device, waited for (the output complete), freed
  splice_ms    their difference: what the replacement adds to the find
  d2d_ms       a torch device-to-device copy of as many bytes as the output has (the copy roofline of the box)
on cfg2's 10 000 patterns over a text-like 1 GiB haystack (seed 11; --every N: plus a planted pattern every N bytes),
replacements of mixed lengths 0 .. 24 (seeded).  --routes adds host-memory calls of 256 KiB, 1 MiB and 4 MiB on either
route (ACX_REPLACE_HOST_MAX forced), the per-call medians.
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


def mixed_repl(n, seed=3, lens=(0, 0, 1, 3, 5, 8, 12, 24)):
    import gen
    rng = gen.SplitMix64(seed)
    return [bytes(65 + rng.next() % 26 for _ in range(lens[rng.next() % len(lens)])) for _ in range(n)]


def median_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return 1e3 * ts[len(ts) // 2]


def plant(hay, pats, every, torch, period=1 << 20, seed=77):
    """a pattern of `pats` at every multiple of `every` bytes, on top of the haystack (device-side select)"""
    import numpy as np
    import gen
    val = np.zeros(period, dtype=np.uint8)
    msk = np.zeros(period, dtype=np.bool_)
    rng = gen.SplitMix64(seed)
    for k in range(0, period - 32, every):
        p = np.frombuffer(pats[rng.next() % len(pats)], dtype=np.uint8)
        val[k:k + len(p)] = p
        msk[k:k + len(p)] = True
    v = torch.from_numpy(val).to(hay.device)
    m = torch.from_numpy(msk).to(hay.device)
    h2 = hay.view(-1, period)
    h2.copy_(torch.where(m, v, h2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--every", type=int, default=0)
    ap.add_argument("--routes", action="store_true")
    args = ap.parse_args()
    import torch
    import gen
    from ahocorasick_rs_amd import capi

    pats = gen.gen_patterns(10000, 5, 12, gen.AZ, 1)
    repl = mixed_repl(len(pats))
    a = capi.Automaton(pats, 0, capi.IMPL_DFA)
    n = args.bytes
    hay = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    a.generate(hay.data_ptr(), n, 1, 11)
    if args.every:
        plant(hay, pats, args.every, torch)
    torch.cuda.synchronize()

    def find():
        r = a.find_device(hay.data_ptr(), n)
        r.device_ptr  # (waits for the records)
        count = r.count
        r.free()
        return count

    out_len = [0]

    def replace():
        r = a.replace_device(hay.data_ptr(), n, repl)
        r.device_ptr  # (waits for the output)
        out_len[0] = r.nbytes
        r.free()

    matches = find()
    find_ms = median_ms(find, args.steps, args.warmup)
    replace_ms = median_ms(replace, args.steps, args.warmup)
    src = torch.empty(out_len[0], dtype=torch.uint8, device="cuda:0")
    dst = torch.empty_like(src)

    def d2d():
        dst.copy_(src)
        torch.cuda.synchronize()

    d2d_ms = median_ms(d2d, args.steps, args.warmup)
    res = {"what": "replace_device vs find_device, cfg2 10k patterns, text-like seed 11" +
                   (f" + a planted pattern every {args.every} B" if args.every else ""),
           "bytes": n, "matches": matches, "output_bytes": out_len[0], "steps": args.steps,
           "find_ms": round(find_ms, 4), "replace_ms": round(replace_ms, 4),
           "splice_ms": round(replace_ms - find_ms, 4), "d2d_ms": round(d2d_ms, 4),
           "splice_over_d2d": round((replace_ms - find_ms) / d2d_ms, 3)}
    del src, dst
    if args.routes:
        host = gen.gen_textlike(4 << 20, 21, pats).tobytes()
        routes = {}
        for size in (256 << 10, 1 << 20, 4 << 20):
            h = host[:size]
            for name, env in (("host", str(1 << 40)), ("device", "0")):
                os.environ["ACX_REPLACE_HOST_MAX"] = env
                routes[f"{size >> 10}KiB_{name}_ms"] = round(median_ms(lambda: a.replace(h, repl), args.steps, args.warmup), 4)
        os.environ.pop("ACX_REPLACE_HOST_MAX", None)
        res["routes"] = routes
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
