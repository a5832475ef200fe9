"""Filter benchmark (acx_filter_device against the find beneath it, a device-to-device copy of the kept bytes and what a torch
user does today; same box, same session, interleaved).

  python tools/bench_filter.py [--steps K] [--warmup W] [--settle-ms MS] [--rows R] [--parts keep1,keep50,keep99 | trace]
                               [--out profiles/r12/filter_bench.jsonl]

One JSON line per shape, appended to --out and printed, and the row of DESIGN.md section 16's table for it.  Every figure is
the median wall time per call over K rounds (at least 20); a round runs every variant once, in rotation, so that the
variants see the same clocks (paired, interleaved); every shape starts with the settle phase bench.py uses (untimed calls
for --settle-ms).

  shapes    cfg2's batch shape in HBM: --rows (131 072) x 8 KiB = 1 GiB as ONE uint8 tensor, digits (no pattern of cfg2's
            10 000 lower-case ones occurs in them) with one pattern planted in 99 %, 50 % and 1 % of the rows, so that
            keep="unmatched" keeps about 1 %, 50 % and 99 % of the rows: keep1, keep50, keep99
  variants  find_a, find_b     acx_find_device on the uniform batch, waited for, freed -- twice per round: the floor, and their
                               spread is the A/A spread of the session
            filter             acx_filter_device (keep the unmatched rows), waited for
            d2d_copy           a device-to-device copy of as many bytes as the filter kept (torch, synchronised): what the
                               gather is judged against
            torch_index        what a torch user does today: the per-row counts of acx_summarize_device, then mask, diff /
                               cumsum over the offsets, a repeat_interleave + arange index of 8 bytes per kept byte and
                               index_select, synchronised
  "gather_ms" = filter - find_a per round (median): the stage's cost; "gather_vs_copy" = gather_ms / d2d_copy.
  trace     no timing: ten rounds of the keep50 shape's filter calls, for a kernel trace made in a run of its own, without
            counters:
              rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_filter.py --parts trace
            (k_filter_flags, k_filter_index, k_filter_tiles, k_filter_gather, the scans' k_rep_prefix / k_rep_partials;
            beside the find's own kernels)
"""
import argparse
import json
import os
import platform
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

L = 8192
PLANTED = {"keep1": 0.99, "keep50": 0.5, "keep99": 0.01}


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


def make_shape(args, capi, gen, np, torch, fraction):
    pats = gen.gen_patterns(10000, 5, 12, gen.AZ, 1)
    a = capi.Automaton(pats, 0, capi.IMPL_DFA)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(13)
    t = torch.randint(48, 58, (args.rows * L,), dtype=torch.uint8, device="cuda:0", generator=g)
    planted = torch.rand(args.rows, device="cuda:0", generator=g) < fraction
    p = torch.from_numpy(np.frombuffer(pats[7], dtype=np.uint8).copy()).to("cuda:0")
    rows = torch.nonzero(planted).flatten()
    at = rows * L + (rows * 37) % (L - 64)  # (the pattern somewhere inside its row, another place in every row)
    for j in range(len(p)):
        t[at + j] = p[j]
    torch.cuda.synchronize()
    return a, t, int(planted.sum())


def variants_of(args, capi, torch, a, t):
    n, rows, info = t.numel(), args.rows, {}

    def find():
        r = a.find_device(t.data_ptr(), n, n_hay=rows, uniform_len=L)
        r.device_ptr  # (waits for the records)
        info["matches"] = r.count
        r.free()

    def filt():
        f = a.filter_device(t.data_ptr(), n, n_hay=rows, uniform_len=L)
        f.data_ptr(capi.FILT_DATA)  # (waits for the stage)
        info["kept_rows"], info["kept_bytes"] = f.n_rows, f.nbytes
        f.free()

    filt()
    kept_bytes = info["kept_bytes"]
    dst = torch.empty(max(kept_bytes, 1), dtype=torch.uint8, device="cuda:0")

    def d2d_copy():
        dst[:kept_bytes].copy_(t[:kept_bytes])
        torch.cuda.synchronize()

    class DeviceWords:  # u64 words of the C ABI as torch sees them (int64), without a copy
        def __init__(self, ptr, words):
            self.__cuda_array_interface__ = {"shape": (words,), "typestr": "<i8", "data": (ptr, False), "version": 2}

    offsets = torch.arange(rows + 1, dtype=torch.int64, device="cuda:0") * L

    def torch_index():
        s = a.summarize_device(t.data_ptr(), n, 0, n_hay=rows, uniform_len=L)
        counts = torch.as_tensor(DeviceWords(s.device_ptr("counts"), rows), device="cuda:0")
        keep = counts < 1
        lens = torch.diff(offsets)[keep]
        starts = offsets[:-1][keep]
        out_off = torch.cumsum(lens, 0)
        total = int(out_off[-1]) if out_off.numel() else 0
        if total:
            idx = torch.repeat_interleave(starts - (out_off - lens), lens) + torch.arange(total, device="cuda:0")
            out = torch.index_select(t, 0, idx)
            info["torch_bytes"] = int(out.numel())
            del idx, out
        torch.cuda.synchronize()
        del counts
        s.free()

    return {"find_a": find, "filter": filt, "d2d_copy": d2d_copy, "find_b": find, "torch_index": torch_index}, info


def part_shape(args, capi, gen, np, torch, part):
    a, t, planted = make_shape(args, capi, gen, np, torch, PLANTED[part])
    v, info = variants_of(args, capi, torch, a, t)
    ts = paired(v, args.steps, args.warmup, args.settle_ms)
    aa = [abs(x - y) for x, y in zip(ts["find_a"], ts["find_b"])]
    m = {n: round(1e3 * med(x), 4) for n, x in ts.items()}
    gather = 1e3 * med([f - s for f, s in zip(ts["filter"], ts["find_a"])])
    res = {"part": part, "rows": args.rows, "row_bytes": L, "planted_rows": planted, "matches": info.get("matches"),
           "kept_rows": info.get("kept_rows"), "kept_bytes": info.get("kept_bytes"), "torch_bytes": info.get("torch_bytes"),
           "steps": args.steps, "ms": m, "aa_spread_ms": {"median": round(1e3 * med(aa), 4), "max": round(1e3 * max(aa), 4)},
           "gather_ms": round(gather, 4), "gather_vs_copy": round(gather / m["d2d_copy"], 3) if m["d2d_copy"] else None,
           "box": platform.node(), "date": time.strftime("%Y-%m-%d")}
    a.close()
    del t
    torch.cuda.empty_cache()
    return res


def part_trace(args, capi, gen, np, torch):
    a, t, _ = make_shape(args, capi, gen, np, torch, PLANTED["keep50"])
    v, _ = variants_of(args, capi, torch, a, t)
    for _ in range(10):
        v["filter"]()
    a.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=50.0)
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--parts", default="keep1,keep50,keep99")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "filter_bench.jsonl"))
    args = ap.parse_args()
    import torch  # first: one process holds one HIP runtime (ahocorasick_rs_amd/__init__.py)
    import numpy as np
    import gen
    from ahocorasick_rs_amd import capi
    if args.parts == "trace":
        part_trace(args, capi, gen, np, torch)
        return
    if args.steps < 20:
        print("note: medians of fewer than 20 rounds are not what DESIGN.md section 16 asks for", file=sys.stderr)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    rows = []
    for part in args.parts.split(","):
        res = part_shape(args, capi, gen, np, torch, part)
        line = json.dumps(res)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        m = res["ms"]
        rows.append("| %s | %s | %s | %s | %s | %s | %s | %s |" % (res["part"], res["kept_bytes"], m["find_a"], m["find_b"], m["filter"],
                                                                   res["gather_ms"], m["d2d_copy"], m["torch_index"]))
    print("| shape | kept bytes | find (A) | find (A') | filter | filter - find | D2D copy | torch index_select |")
    print("|---|---|---|---|---|---|---|---|")
    print("\n".join(rows))


if __name__ == "__main__":
    main()
