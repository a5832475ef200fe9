"""Tally benchmark (acx_tally_device against the find beneath it, the columns and what a torch user does today; same box, same
session, interleaved).

  python tools/bench_tally.py [--steps K] [--warmup W] [--settle-ms MS] [--rows R] [--parts sparse,planted | trace]
                              [--out profiles/r11/tally_bench.jsonl]

One JSON line per shape, appended to --out and printed, and the row of DESIGN.md section 15's table for it.  Every figure is
the median wall time per call over K rounds (at least 20); a round runs every variant once, in rotation, so that the
variants see the same clocks (paired, interleaved); every shape starts with the settle phase bench.py uses (untimed calls
for --settle-ms).

  sparse    cfg3's shape: --rows (131 072) x 8 KiB as ONE uint8 tensor in HBM, text-like (seed 13) over cfg2's 10 000 patterns
  planted   the same with a pattern planted every 256 bytes
  variants  find_a, find_b     acx_find_device on the uniform batch, waited for, freed -- twice per round: the floor, and their
                               spread is the A/A spread of the session
            columns            acx_find_columns_device, waited for
            tally              acx_tally_device as shipped, waited for
            tally_radix        acx_tally_device with ACX_TALLY_ROW_MAX=0: rocPRIM's radix sort for every row
            torch_unique       what a torch user does today: the columns, torch.searchsorted for every match's row,
                               torch.unique(row << 24 | pattern, return_counts=True), synchronised
  "tile_beats_radix": whether tally_radix - tally is larger than the A/A spread (the largest |a - b| of the session).
  trace     no timing: ten rounds of the planted shape's tally calls (both forms), for a kernel trace made in a run of its own,
            without counters:
              rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_tally.py --parts trace
            (k_tally_tiles, k_tally_compact, the scans' k_rep_prefix; k_tally_long_keys, rocPRIM's sort kernels and
            k_tally_rle for the radix form; beside the find's own kernels)
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


def make_shape(args, capi, gen, np, torch, planted):
    pats = gen.gen_patterns(10000, 5, 12, gen.AZ, 1)
    a = capi.Automaton(pats, 0, capi.IMPL_DFA)
    hay = gen.gen_textlike(args.rows * L, 13, pats).copy()
    if planted:
        rng = gen.SplitMix64(77)
        period = 1 << 20
        val, msk = np.zeros(period, dtype=np.uint8), np.zeros(period, dtype=bool)
        for k in range(0, period - 32, 256):
            p = np.frombuffer(pats[rng.next() % len(pats)], dtype=np.uint8)
            val[k:k + len(p)] = p
            msk[k:k + len(p)] = True
        h2 = hay[:len(hay) // period * period].reshape(-1, period)
        h2[:, msk] = val[msk]
    t = torch.from_numpy(hay).to("cuda:0")
    torch.cuda.synchronize()
    return a, t


def variants_of(args, capi, torch, a, t):
    n, rows, info = t.numel(), args.rows, {}

    def find():
        r = a.find_device(t.data_ptr(), n, n_hay=rows, uniform_len=L)
        r.device_ptr  # (waits for the records)
        info["matches"] = r.count
        r.free()

    def columns():
        c = a.find_columns_device(t.data_ptr(), n, n_hay=rows, uniform_len=L)
        c.data_ptr(capi.COL_ROW_OFFSETS)  # (waits for the split and the scan)
        c.free()

    def tally(row_max):
        def fn():
            if row_max is None:
                os.environ.pop("ACX_TALLY_ROW_MAX", None)
            else:
                os.environ["ACX_TALLY_ROW_MAX"] = row_max
            x = a.tally_device(t.data_ptr(), n, n_hay=rows, uniform_len=L)
            x.data_ptr(capi.TALLY_COUNT)  # (waits for the stage)
            info["nnz"] = x.nnz
            x.free()
            os.environ.pop("ACX_TALLY_ROW_MAX", None)
        return fn

    class DeviceWords:  # an int64 column of the C ABI as torch sees it, without a copy
        def __init__(self, ptr, words):
            self.__cuda_array_interface__ = {"shape": (words,), "typestr": "<i8", "data": (ptr, False), "version": 2}

    def torch_unique():
        c = a.find_columns_device(t.data_ptr(), n, n_hay=rows, uniform_len=L)
        cnt = c.count
        if cnt:
            pat = torch.as_tensor(DeviceWords(c.data_ptr(capi.COL_PATTERN), cnt), device="cuda:0")
            ro = torch.as_tensor(DeviceWords(c.data_ptr(capi.COL_ROW_OFFSETS), rows + 1), device="cuda:0")
            row = torch.searchsorted(ro, torch.arange(cnt, device="cuda:0"), right=True) - 1
            keys, counts = torch.unique((row << 24) | pat, return_counts=True)
            info["unique"] = int(keys.numel())
            del pat, ro
        torch.cuda.synchronize()
        c.free()

    return {"find_a": find, "columns": columns, "tally": tally(None), "find_b": find, "tally_radix": tally("0"),
            "torch_unique": torch_unique}, info


def part_shape(args, capi, gen, np, torch, planted):
    a, t = make_shape(args, capi, gen, np, torch, planted)
    v, info = variants_of(args, capi, torch, a, t)
    ts = paired(v, args.steps, args.warmup, args.settle_ms)
    aa = [abs(x - y) for x, y in zip(ts["find_a"], ts["find_b"])]
    m = {n: round(1e3 * med(x), 4) for n, x in ts.items()}
    gain = 1e3 * med([r - s for r, s in zip(ts["tally_radix"], ts["tally"])])
    res = {"part": "planted" if planted else "sparse", "rows": args.rows, "row_bytes": L, "matches": info.get("matches"),
           "nnz": info.get("nnz"), "torch_unique_entries": info.get("unique"), "steps": args.steps, "ms": m,
           "aa_spread_ms": {"median": round(1e3 * med(aa), 4), "max": round(1e3 * max(aa), 4)},
           "tally_radix_minus_tally_ms": round(gain, 4), "tile_beats_radix": bool(gain > 1e3 * max(aa)),
           "box": platform.node(), "date": time.strftime("%Y-%m-%d")}
    a.close()
    return res


def part_trace(args, capi, gen, np, torch):
    a, t = make_shape(args, capi, gen, np, torch, True)
    v, _ = variants_of(args, capi, torch, a, t)
    for _ in range(10):
        v["tally"]()
        v["tally_radix"]()
    a.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=50.0)
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--parts", default="sparse,planted")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "tally_bench.jsonl"))
    args = ap.parse_args()
    import torch  # first: one process holds one HIP runtime (ahocorasick_rs_amd/__init__.py)
    import numpy as np
    import gen
    from ahocorasick_rs_amd import capi
    if args.parts == "trace":
        part_trace(args, capi, gen, np, torch)
        return
    if args.steps < 20:
        print("note: medians of fewer than 20 rounds are not what DESIGN.md section 15 asks for", file=sys.stderr)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    rows = []
    for part in args.parts.split(","):
        res = part_shape(args, capi, gen, np, torch, part == "planted")
        line = json.dumps(res)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        m = res["ms"]
        rows.append("| %s | %s | %s | %s | %s | %s | %s |" % (res["part"], m["find_a"], m["find_b"], m["columns"], m["tally"],
                                                              m["tally_radix"], m["torch_unique"]))
    print("| shape | find (A) | find (A') | columns | tally | tally, ROW_MAX=0 | torch on columns |")
    print("|---|---|---|---|---|---|---|")
    print("\n".join(rows))


if __name__ == "__main__":
    main()
