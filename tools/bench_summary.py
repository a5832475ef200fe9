"""Summary benchmark (acx_summarize* against the find it replaces, same box, same session, interleaved).

  python tools/bench_summary.py [--steps K] [--warmup W] [--settle-ms MS] [--bytes N] [--rows R] [--parts device,host,routes,hist | trace]
                                [--out profiles/r09/summary_bench.jsonl]

One JSON line per part, appended to --out and printed, and a short table (markdown) at the end.  Every figure is the median
wall time per call over K rounds; a round runs every variant of the part once, in rotation, so that the variants see the
same clocks (paired, interleaved); every part starts with the settle phase bench.py uses (untimed calls for --settle-ms).

  device   cfg2 (10 000 patterns, text-like seed 11) resident in HBM, --bytes (1 GiB):
             find_a, find_b   acx_find_device, waited for, freed -- twice per round: their spread is the A/A spread of the
                              session ("aa_spread_pct": the median of |a - b| / a over the rounds, and the largest)
             find_copy        acx_find_device + acx_result_copy (the records on the host)
             sum_0 .. sum_3   acx_summarize_device with what = 0, 1, 2, 3, every requested part copied to the host
           "added_ms": sum_k - find_a per round, the median; "condition": sum_1 <= find_copy read against the A/A spread
  host     cfg3's shape, --rows (131 072) x 8 KiB of host memory, text-like (sparse) and with a pattern planted every 256 B:
             C ABI    acx_find_batch against acx_summarize (what = 1) on the device route
             Python   [bool(x) for x in find_matches_as_indexes_batch(rows)] against is_match_batch(rows)
  routes   the ACX_SUMMARY_HOST_MAX crossover: acx_summarize (what = 1) from host memory with either route forced, on one
           haystack and on a batch of 8 KiB rows of 64 KiB .. 16 MiB in all (text-like over cfg2's patterns)
  hist     the histogram forms at their own sizes: 3 000 patterns (LDS form), 8 192 (the LDS form at its bound),
           20 000 (global atomics), over 256 MiB with a pattern planted every 256 B: sum_2 - sum_0
  trace    no timing: ten rounds of the device part's calls, for a kernel trace made in a run of its own, without counters:
             rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_summary.py --parts trace
           (the per-kernel times are in <dir>/.../*_kernel_stats.csv: k_sum_gather, k_sum_hist_lds / k_sum_hist_global,
           k_rep_prefix of the counts' scan, beside the find's own kernels)
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


def plant_host(hay, pats, every, seed=77):
    import numpy as np
    import gen
    rng = gen.SplitMix64(seed)
    period = 1 << 20
    val, msk = np.zeros(period, dtype=np.uint8), np.zeros(period, dtype=bool)
    for k in range(0, period - 32, every):
        p = np.frombuffer(pats[rng.next() % len(pats)], dtype=np.uint8)
        val[k:k + len(p)] = p
        msk[k:k + len(p)] = True
    h2 = hay[:len(hay) // period * period].reshape(-1, period)
    h2[:, msk] = val[msk]


def part_device(args, capi, gen, np):
    pats = gen.gen_patterns(10000, 5, 12, gen.AZ, 1)
    a = capi.Automaton(pats, 0, capi.IMPL_DFA)
    n = args.bytes
    buf = capi.DeviceBuffer(n)
    a.generate(buf.ptr, n, 1, 11)
    info = {}

    def find():
        r = a.find_device(buf.ptr, n)
        r.device_ptr  # (waits for the records)
        info["matches"] = r.count
        r.free()

    def find_copy():
        r = a.find_device(buf.ptr, n)
        r.matches()
        r.free()

    def summarize(what):
        def fn():
            s = a.summarize_device(buf.ptr, n, what)
            s.counts()
            if what & 1:
                s.any_bits(); s.first()
            if what & 2:
                s.by_pattern()
            s.free()
        return fn

    v = {"find_a": find, "find_copy": find_copy, "sum_0": summarize(0), "sum_1": summarize(1), "find_b": find,
         "sum_2": summarize(2), "sum_3": summarize(3)}
    ts = paired(v, args.steps, args.warmup, args.settle_ms)
    aa = [abs(x - y) / x for x, y in zip(ts["find_a"], ts["find_b"])]
    m = ms(ts)
    added = {f"sum_{k}": round(1e3 * med([s - f for s, f in zip(ts[f"sum_{k}"], ts["find_a"])]), 4) for k in range(4)}
    diff = 1e3 * med([s - f for s, f in zip(ts["sum_1"], ts["find_copy"])])
    res = {"part": "device", "what": "cfg2 10k patterns, text-like seed 11, resident in HBM", "bytes": n, "matches": info["matches"],
           "steps": args.steps, "ms": m, "added_ms": added,
           "aa_spread_pct": {"median": round(100 * med(aa), 3), "max": round(100 * max(aa), 3)},
           "sum_1_minus_find_copy_ms": round(diff, 4),
           "condition_sum_1_not_longer_than_find_copy": bool(diff <= max(aa) * m["find_a"])}
    buf.free(); a.close()
    return res


def part_host(args, capi, gen, np):
    import ahocorasick_rs as ar
    pats = gen.gen_patterns(10000, 5, 12, gen.AZ, 1)
    L, rows = 8192, args.rows
    a = capi.Automaton(pats, 0, capi.IMPL_DFA)
    b = ar.BytesAhoCorasick(pats)
    out = []
    for density in ("sparse", "every_256"):
        hay = gen.gen_textlike(rows * L, 13, pats).copy()
        if density == "every_256":
            plant_host(hay, pats, 256)
        off = (np.arange(rows + 1, dtype=np.uint64) * np.uint64(L))
        lib, ct = capi.lib(), __import__("ctypes")
        info = {}

        def find_batch():
            m, n = ct.c_void_p(), ct.c_uint64()
            counts = np.zeros(rows, dtype=np.uint64)
            capi._check(lib.acx_find_batch(a._h, hay.ctypes.data, off.ctypes.data, rows, 0, 0, ct.byref(m), ct.byref(n), counts.ctypes.data))
            info["matches"] = int(n.value)
            lib.acx_free_matches(m)

        def summarize():
            s = ct.c_void_p()
            capi._check(lib.acx_summarize(a._h, hay.ctypes.data, rows * L, off.ctypes.data, rows, 0, 0, capi.SUM_FIRST, ct.byref(s)))
            d = capi.DeviceSummary(s.value, rows, len(pats))
            info["on_device"] = d.on_device
            d.any_bits()
            d.free()

        ts = paired({"find_batch": find_batch, "summarize_what_1": summarize}, args.steps, args.warmup, args.settle_ms)
        res = {"part": "host", "density": density, "rows": rows, "row_bytes": L, "c_abi_ms": ms(ts), "matches": info["matches"],
               "summarize_on_device": info["on_device"], "steps": args.steps}
        hb = hay.tobytes()
        hs = [hb[i * L:(i + 1) * L] for i in range(rows)]
        del hb
        py_steps = max(2, args.steps // 4)
        ts = paired({"bool_of_find_batch": lambda: [bool(x) for x in b.find_matches_as_indexes_batch(hs)],
                     "is_match_batch": lambda: b.is_match_batch(hs)}, py_steps, 1, 0)
        res["python_ms"], res["python_steps"] = ms(ts), py_steps
        out.append(res)
        del hs
    a.close()
    return out


def part_routes(args, capi, gen, np):
    pats = gen.gen_patterns(10000, 5, 12, gen.AZ, 1)
    a = capi.Automaton(pats, 0, capi.IMPL_DFA)
    L = 8192
    host = gen.gen_textlike(16 << 20, 21, pats).tobytes()
    out = []
    saved = os.environ.get("ACX_SUMMARY_HOST_MAX")
    for size in (64 << 10, 256 << 10, 1 << 20, 4 << 20, 16 << 20):
        h = host[:size]
        rows = [h[i * L:(i + 1) * L] for i in range(size // L)]

        def call(limit, batch):
            def fn():
                os.environ["ACX_SUMMARY_HOST_MAX"] = limit
                s = a.summarize_batch(rows, capi.SUM_FIRST) if batch else a.summarize(h, capi.SUM_FIRST)
                s.any_bits()
                s.free()
            return fn

        ts = paired({"one_host": call(str(1 << 40), False), "one_device": call("0", False),
                     "batch_host": call(str(1 << 40), True), "batch_device": call("0", True)}, args.steps, args.warmup, args.settle_ms)
        out.append({"part": "routes", "bytes": size, "rows": len(rows), "ms": ms(ts), "steps": args.steps})
    if saved is None:
        os.environ.pop("ACX_SUMMARY_HOST_MAX", None)
    else:
        os.environ["ACX_SUMMARY_HOST_MAX"] = saved
    a.close()
    return out


def part_trace(args, capi, gen, np):
    pats = gen.gen_patterns(10000, 5, 12, gen.AZ, 1)
    a = capi.Automaton(pats, 0, capi.IMPL_DFA)
    n = args.bytes
    buf = capi.DeviceBuffer(n)
    a.generate(buf.ptr, n, 1, 11)
    L = 8192
    for _ in range(10):
        r = a.find_device(buf.ptr, n)
        r.matches()
        r.free()
        for what in (0, 1, 2, 3):
            for seg in ({}, {"n_hay": n // L, "uniform_len": L}):
                s = a.summarize_device(buf.ptr, n, what, **seg)
                s.counts()
                s.free()
    buf.free(); a.close()
    return []


def part_hist(args, capi, gen, np):
    out = []
    n = 256 << 20
    for n_pat in (3000, 8192, 20000):
        base = list(dict.fromkeys(gen.gen_patterns(n_pat, 5, 12, gen.AZ, 7)))
        pats = (base + gen.gen_patterns(n_pat, 13, 15, gen.AZ, 8))[:n_pat]
        a = capi.Automaton(pats, 0, capi.IMPL_DFA)
        hay = gen.gen_textlike(n, 11, pats).copy()
        plant_host(hay, pats, 256)
        buf = capi.DeviceBuffer(n).upload(hay)
        info = {}

        def summarize(what):
            def fn():
                s = a.summarize_device(buf.ptr, n, what)
                info["matches"] = s.total
                if what & 2:
                    s.by_pattern()
                else:
                    s.counts()
                s.free()
            return fn

        ts = paired({"sum_0": summarize(0), "sum_2": summarize(2)}, args.steps, args.warmup, args.settle_ms)
        out.append({"part": "hist", "n_patterns": n_pat, "form": "lds" if n_pat <= 8192 else "global", "bytes": n,
                    "matches": info["matches"], "ms": ms(ts),
                    "hist_added_ms": round(1e3 * med([x - y for x, y in zip(ts["sum_2"], ts["sum_0"])]), 4), "steps": args.steps})
        buf.free(); a.close()
    return out


def table(lines):
    t = ["| part | case | variant | ms |", "|---|---|---|---|"]
    for r in lines:
        if r["part"] == "device":
            for k, v in r["ms"].items():
                t.append(f"| device | 1 GiB cfg2, {r['matches']} matches | {k} | {v} |")
            for k, v in r["added_ms"].items():
                t.append(f"| device | added over find_a | {k} | {v} |")
            t.append(f"| device | A/A spread of find (median / max) | % | {r['aa_spread_pct']['median']} / {r['aa_spread_pct']['max']} |")
        elif r["part"] == "routes":
            for k, v in r["ms"].items():
                t.append(f"| routes | {r['bytes'] >> 10} KiB ({r['rows']} rows) | {k} | {v} |")
        elif r["part"] == "host":
            for k, v in list(r["c_abi_ms"].items()) + list(r["python_ms"].items()):
                t.append(f"| host | {r['rows']} x {r['row_bytes']} B, {r['density']}, {r['matches']} matches | {k} | {v} |")
        else:
            t.append(f"| hist | {r['n_patterns']} patterns ({r['form']}), {r['matches']} matches | sum_2 - sum_0 | {r['hist_added_ms']} |")
    return "\n".join(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=50.0)
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--parts", default="device,host,routes,hist")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "summary_bench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import gen
    from ahocorasick_rs_amd import capi

    os.environ.pop("ACX_SUMMARY_HOST_MAX", None)
    lines = []
    for part in args.parts.split(","):
        r = {"device": part_device, "host": part_host, "routes": part_routes, "hist": part_hist, "trace": part_trace}[part](args, capi, gen, np)
        for x in (r if isinstance(r, list) else [r]):
            lines.append(x)
            print(json.dumps(x), flush=True)
    if not lines:
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for x in lines:
            f.write(json.dumps(x) + "\n")
    print(table(lines), flush=True)


if __name__ == "__main__":
    main()
