"""Columns benchmark (find_matches_as_columns and the split kernel against what they replace; same box, same session,
interleaved).

  python tools/bench_columns.py [--steps K] [--warmup W] [--settle-ms MS] [--bytes N] [--parts call,kernel,pair | trace]
                                [--out profiles/r10/columns_bench.jsonl]

One JSON line per part, appended to --out and printed.  Every figure is the median wall time per call over K rounds; a round
runs every variant of the part once, in rotation, so that the variants see the same clocks (paired, interleaved); every part
starts with an untimed settle phase of --settle-ms.  Needs torch (the haystack and the consumer of the columns are torch's).

  call     cfg2 (10 000 patterns, text-like seed 11) as a uint8 tensor in HBM, --bytes (1 GiB), BytesAhoCorasick:
             floor_a, floor_b  acx_find_device, waited for, freed -- twice per round: their spread is the A/A spread of the
                               session ("aa_spread_pct")
             columns           find_matches_as_columns(tensor) + torch.from_dlpack of the three columns + a synchronise
             tuples            find_matches_as_indexes(tensor): the tuple list (the parent commit's code)
  kernel   a dense result -- cfg2's text with a pattern planted every 32 bytes, --bytes, searched once: tens of millions of
           records in HBM -- and on it, in rotation:
             split_a, split_b  acx_split_device (synchronous), twice per round: the A/A spread
             copy              a device-to-device copy of the same 24 n bytes (torch) + a synchronise
           "split_minus_copy_ms": the median of the per-round differences
  pair     tools/ubench_split.hip (built to build/ubench_split if it is not there) on as many records as `kernel` had:
           the LDS-staged kernel of the library, the thread-per-record form and a copy, timed with events
  trace    no timing: ten rounds of `kernel`'s split and copy, for a kernel trace made in a run of its own:
             rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_columns.py --parts trace
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def paired(variants, steps, warmup, settle_ms):
    """variants: {name: fn} -> {name: [seconds per round]}: settle, warm up, then `steps` rounds of every variant in rotation"""
    names = list(variants)
    t_end = time.perf_counter() + settle_ms * 1e-3
    variants[names[0]]()
    while time.perf_counter() < t_end:
        variants[names[0]]()
    for _ in range(warmup):
        for n in names:
            variants[n]()
    ts = {n: [] for n in names}
    for k in range(steps):
        for j in range(len(names)):
            n = names[(j + k) % len(names)]
            t0 = time.perf_counter()
            variants[n]()
            ts[n].append(time.perf_counter() - t0)
    return ts


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def ms(ts):
    return {n: round(1e3 * med(v), 4) for n, v in ts.items()}


def spread(a, b):
    aa = [abs(x - y) / x for x, y in zip(a, b)]
    return {"median": round(100 * med(aa), 3), "max": round(100 * max(aa), 3)}


def cfg2(capi, gen, torch, nbytes):
    pats = gen.gen_patterns(10000, 5, 12, gen.AZ, 1)
    a = capi.Automaton(pats, 0, capi.IMPL_DFA)
    hay = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    a.generate(hay.data_ptr(), nbytes, 1, 11)
    return pats, a, hay


def part_call(args, capi, gen, torch):
    import ahocorasick_rs as ar
    pats, a, hay = cfg2(capi, gen, torch, args.bytes)
    b = ar.BytesAhoCorasick(pats)
    info = {}

    def floor():
        r = a.find_device(hay.data_ptr(), args.bytes)
        r.device_ptr  # (waits for the records)
        info["matches"] = r.count
        r.free()

    def columns():
        c = b.find_matches_as_columns(hay)
        t = [torch.from_dlpack(x) for x in (c.pattern, c.start, c.end)]
        torch.cuda.synchronize()
        info["columns"] = len(t[0])

    def tuples():
        info["tuples"] = len(b.find_matches_as_indexes(hay))

    ts = paired({"floor_a": floor, "columns": columns, "tuples": tuples, "floor_b": floor}, args.steps, args.warmup,
                args.settle_ms)
    assert info["matches"] == info["columns"] == info["tuples"], info
    res = {"part": "call", "what": "cfg2 10k patterns, text-like seed 11, a uint8 tensor in HBM", "bytes": args.bytes,
           "matches": info["matches"], "steps": args.steps, "ms": ms(ts), "aa_spread_pct": spread(ts["floor_a"], ts["floor_b"]),
           "columns_minus_floor_ms": round(1e3 * med([c - f for c, f in zip(ts["columns"], ts["floor_a"])]), 4),
           "tuples_over_columns": round(med(ts["tuples"]) / med(ts["columns"]), 1)}
    a.close()
    return res


def dense_result(args, capi, gen, torch):
    """cfg2's text with a pattern planted every 32 bytes, searched: (automaton, result, n records, its device address)"""
    import numpy as np
    pats, a, hay = cfg2(capi, gen, torch, args.bytes)
    rng = gen.SplitMix64(77)
    period = 1 << 20
    val, msk = np.zeros(period, dtype=np.uint8), np.zeros(period, dtype=bool)
    for k in range(0, period - 32, 32):
        p = np.frombuffer(pats[rng.next() % len(pats)], dtype=np.uint8)
        val[k:k + len(p)] = p
        msk[k:k + len(p)] = True
    idx = torch.from_numpy(np.flatnonzero(msk)).cuda()
    hay[:args.bytes // period * period].view(-1, period)[:, idx] = torch.from_numpy(val[msk]).cuda()
    torch.cuda.synchronize()
    r = a.find_device(hay.data_ptr(), args.bytes)
    return a, r, r.count, r.device_ptr


def part_kernel(args, capi, gen, torch, trace=False):
    a, r, n, d_m = dense_result(args, capi, gen, torch)
    cols = torch.empty(3 * n, dtype=torch.int64, device="cuda")
    # (the copy's source: a tensor as large as the records, which are the library's allocation and no tensor)
    rec = torch.zeros(3 * n, dtype=torch.int64, device="cuda")
    p = [cols.data_ptr() + 8 * n * k for k in range(3)]

    def split():
        capi.split_device(d_m, n, p[0], p[1], p[2])

    def copy():
        cols.copy_(rec)
        torch.cuda.synchronize()

    if trace:
        for _ in range(10):
            split(); copy()
        res = {"part": "trace", "records": n}
    else:
        ts = paired({"split_a": split, "copy": copy, "split_b": split}, args.steps, args.warmup, args.settle_ms)
        res = {"part": "kernel", "what": "cfg2's text, a pattern planted every 32 bytes: acx_split_device vs a device copy of 24 n bytes",
               "bytes": args.bytes, "records": n, "steps": args.steps, "ms": ms(ts),
               "aa_spread_pct": spread(ts["split_a"], ts["split_b"]),
               "split_minus_copy_ms": round(1e3 * med([s - c for s, c in zip(ts["split_a"], ts["copy"])]), 4),
               "gb_per_s": {k: round(48e-9 * n / med(ts[k]), 1) for k in ("split_a", "copy")}}
    r.free(); a.close()
    return res


def part_pair(args, records):
    exe, src = os.path.join(ROOT, "build", "ubench_split"), os.path.join(ROOT, "tools", "ubench_split.hip")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                               "-o", exe, src])
    out = subprocess.run([exe, str(records), str(max(args.steps, 20))], check=True, stdout=subprocess.PIPE, text=True).stdout
    return [json.loads(line) for line in out.splitlines() if line.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=500.0)
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--parts", default="call,kernel,pair")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "columns_bench.jsonl"))
    args = ap.parse_args()
    import torch  # first: one process holds one HIP runtime (ahocorasick_rs_amd/__init__.py)
    import gen
    from ahocorasick_rs_amd import capi
    if capi.device_count() < 1:
        raise SystemExit("bench_columns: no HIP device (there is nothing to measure without one)")
    stamp = {"date": time.strftime("%Y-%m-%d"), "gpu": torch.cuda.get_device_name(0)}
    results, records = [], None
    for part in args.parts.split(","):
        if part == "call":
            results.append(part_call(args, capi, gen, torch))
        elif part in ("kernel", "trace"):
            results.append(part_kernel(args, capi, gen, torch, trace=part == "trace"))
            records = results[-1]["records"]
        elif part == "pair":
            results.extend(part_pair(args, records or args.bytes // 32))
        else:
            raise SystemExit("unknown part " + part)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for res in results:
            res.update(stamp)
            line = json.dumps(res)
            print(line, flush=True)
            if res["part"] != "trace":
                f.write(line + "\n")


if __name__ == "__main__":
    main()
