"""Row-cut benchmark (acx_split_rows_device against a device-to-device copy of the input, what a torch user does today and
the find the cut is made for; same box, same session, interleaved).

  python tools/bench_rows.py [--steps K] [--warmup W] [--settle-ms MS] [--bytes N] [--parts line16,line80,line1024 | trace]
                             [--out profiles/r15/rows_bench.jsonl]

One JSON line per shape, appended to --out and printed, and the row of DESIGN.md section 19's table for it.  Every figure is
the median wall time per call over K rounds (at least 20); a round runs every variant once, in rotation, so that the
variants see the same clocks (paired, interleaved); every shape starts with the settle phase bench.py uses (untimed calls
for --settle-ms).

  shapes    --bytes (1 GiB) as ONE uint8 tensor in HBM: digits (no pattern of cfg2's 10 000 lower-case ones occurs in them)
            with a newline at every byte with probability 1 / 16, 1 / 80 and 1 / 1 024 -- mean line lengths of 16, 80 and
            1 024 bytes: line16, line80, line1024.  The last byte is no newline, so the last row is unterminated.
  variants  split_a, split_b   acx_split_rows_device, waited for (acx_rows_offsets), freed -- twice per round: their spread is
                               the A/A spread of the session
            d2d_copy           a device-to-device copy of the input (torch, synchronised): the bandwidth yardstick -- the
                               stage reads the input twice and writes 8 bytes per row
            torch_cat          torch.cat([zero, torch.nonzero(t == 10).flatten() + 1, end]), synchronised: what a caller
                               writes today (a bool byte per input byte, a compaction, a concatenation)
            find               acx_find_device with cfg2's automaton over the same tensor as one haystack, waited for, freed:
                               what the cut is the first step of
  The offsets of split_rows and of the torch expression are compared once per shape before anything is timed.
  trace     no timing: ten split calls on the line80 shape, for a kernel trace made in a run of its own, without counters:
              rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_rows.py --parts trace
            (k_rows_count, k_rows_write, the scan's k_rep_prefix / k_rep_partials)
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

MEAN = {"line16": 16, "line80": 80, "line1024": 1024}


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


def make_shape(args, torch, mean):
    g = torch.Generator(device="cuda:0")
    g.manual_seed(13 + mean)
    n = args.bytes
    t = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    step = 1 << 28  # (the random floats of a piece: 1 GiB, not 4)
    for lo in range(0, n, step):
        piece = t[lo:lo + step]
        piece.copy_(torch.randint(48, 58, (piece.numel(),), dtype=torch.uint8, device="cuda:0", generator=g))
        piece[torch.rand(piece.numel(), device="cuda:0", generator=g) < 1.0 / mean] = 10
    t[-1] = 48
    torch.cuda.synchronize()
    return t


def variants_of(args, capi, torch, a, t):
    n, info = t.numel(), {}

    def split():
        r = capi.split_rows_device(t.data_ptr(), n, 10)
        info["rows"] = r.rows
        r.offsets_ptr()  # (waits for the stage)
        r.free()

    dst = torch.empty_like(t)

    def d2d_copy():
        dst.copy_(t)
        torch.cuda.synchronize()

    zero = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    end = torch.full((1,), n, dtype=torch.int64, device="cuda:0")

    def torch_cat():
        off = torch.cat([zero, torch.nonzero(t == 10).flatten() + 1, end])
        torch.cuda.synchronize()
        info["torch_rows"] = off.numel() - 1
        return off

    def find():
        r = a.find_device(t.data_ptr(), n)
        r.device_ptr  # (waits for the records)
        info["matches"] = r.count
        r.free()

    class DeviceWords:  # int64 words of the C ABI as torch sees them, without a copy
        def __init__(self, ptr, words):
            self.__cuda_array_interface__ = {"shape": (words,), "typestr": "<i8", "data": (ptr, False), "version": 2}

    r = capi.split_rows_device(t.data_ptr(), n, 10)
    mine = torch.as_tensor(DeviceWords(r.offsets_ptr(), r.rows + 1), device="cuda:0")
    assert torch.equal(mine, torch_cat()), "split_rows and the torch expression disagree"
    del mine
    r.free()
    return {"split_a": split, "d2d_copy": d2d_copy, "torch_cat": torch_cat, "split_b": split, "find": find}, info


def part_shape(args, capi, torch, a, part):
    t = make_shape(args, torch, MEAN[part])
    v, info = variants_of(args, capi, torch, a, t)
    ts = paired(v, args.steps, args.warmup, args.settle_ms)
    aa = [abs(x - y) for x, y in zip(ts["split_a"], ts["split_b"])]
    m = {n: round(1e3 * med(x), 4) for n, x in ts.items()}
    res = {"part": part, "bytes": args.bytes, "mean_line": MEAN[part], "rows": info.get("rows"), "torch_rows": info.get("torch_rows"),
           "matches": info.get("matches"), "steps": args.steps, "ms": m,
           "aa_spread_ms": {"median": round(1e3 * med(aa), 4), "max": round(1e3 * max(aa), 4)},
           "split_vs_copy": round(m["split_a"] / m["d2d_copy"], 3) if m["d2d_copy"] else None,
           "torch_vs_split": round(m["torch_cat"] / m["split_a"], 3) if m["split_a"] else None,
           "box": platform.node(), "date": time.strftime("%Y-%m-%d")}
    del t
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=50.0)
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--parts", default="line16,line80,line1024")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "rows_bench.jsonl"))
    args = ap.parse_args()
    import torch  # first: one process holds one HIP runtime (ahocorasick_rs_amd/__init__.py)
    import gen
    from ahocorasick_rs_amd import capi
    if args.parts == "trace":
        t = make_shape(args, torch, MEAN["line80"])
        for _ in range(10):
            r = capi.split_rows_device(t.data_ptr(), t.numel(), 10)
            r.offsets_ptr()
            r.free()
        return
    if args.steps < 20:
        print("note: medians of fewer than 20 rounds are not what DESIGN.md section 19 asks for", file=sys.stderr)
    a = capi.Automaton(gen.gen_patterns(10000, 5, 12, gen.AZ, 1), 0, capi.IMPL_DFA)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    rows = []
    for part in args.parts.split(","):
        res = part_shape(args, capi, torch, a, part)
        line = json.dumps(res)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        m = res["ms"]
        rows.append("| %s | %s | %s | %s | %s | %s | %s |" % (res["part"], res["rows"], m["split_a"], m["split_b"], m["d2d_copy"],
                                                             m["torch_cat"], m["find"]))
    a.close()
    print("| shape | rows | split_rows (A) | split_rows (A') | D2D copy of the input | torch expression | cfg2 find |")
    print("|---|---|---|---|---|---|---|")
    print("\n".join(rows))


if __name__ == "__main__":
    main()
