"""Mask benchmark (acx_mask_device against the find beneath it, a device-to-device copy of the haystack, replace_all with
same-length replacements -- the only way to do this before -- and the torch form of the mask from the columns; same box, same
session, interleaved).

  python tools/bench_mask.py [--steps K] [--warmup W] [--settle-ms MS] [--rows R] [--every B [B ...]] [--parts mask | trace]
                             [--out profiles/r14/mask_bench.jsonl]

One JSON line per shape, appended to --out and printed, and the row of DESIGN.md section 18's table for it.  Every figure is
the median wall time per call over K rounds (at least 20); a round runs every variant once, in rotation, so that the
variants see the same clocks (paired, interleaved); the shape starts with the settle phase bench.py uses (untimed calls
for --settle-ms).

  shape     cfg2's batch shape in HBM: --rows (131 072) x 8 KiB = 1 GiB as ONE uint8 tensor of digits (no pattern of cfg2's
            10 000 lower-case ones occurs in them) with one of eight patterns planted every --every bytes: 256 (about 4 M
            records), and the dense end of the curve, 64 and 32 (--every 256 64 32 runs the three one after the other).
  variants  find_a, find_b     acx_find_device on the uniform batch, waited for, freed -- twice per round: the floor, and their
                               spread is the A/A spread of the session
            mask_all           acx_mask_device (fill '*'), waited for
            match_mask         acx_mask_device (ACX_MASK_ZERO, fill 1), waited for
            d2d_hay            a device-to-device copy of the haystack (torch, synchronised): what the stage's copy and its
                               one pass over the records are judged against
            replace_same_len   acx_replace_device with '*' * len(pattern) for every pattern: what a caller did before
            torch_mask         find_columns_device, then index_add_ of +1 / -1 at every start / end and a cumsum over the
                               haystack's length (int32: 4 bytes per haystack byte and more), synchronised
  "mask_ms" = mask_all - find_a per round (median): the stage's cost; "mask_vs_copy" = mask_ms / d2d_hay;
  "splice_ms" = replace_same_len - find_a per round (median): replace_all's splice on the same input; "mask_vs_splice" =
  mask_ms / splice_ms -- below 1 the stage is faster than the splice it replaces.
  trace     no timing: ten rounds of mask_all and match_mask, for a kernel trace made in a run of its own, without counters:
              rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_mask.py --parts trace
            (k_mask_tiles, k_mask_paint, k_mask_offsets, the scan's k_rep_prefix / k_rep_partials, the copy; beside the find's
            own kernels)
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


def make_shape(args, every, capi, gen, np, torch):
    pats = gen.gen_patterns(10000, 5, 12, gen.AZ, 1)
    a = capi.Automaton(pats, 0, capi.IMPL_DFA)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(13)
    n = args.rows * L
    t = torch.randint(48, 58, (n,), dtype=torch.uint8, device="cuda:0", generator=g)
    at = torch.arange(0, n - 64, every, device="cuda:0")
    for k in range(8):  # (eight patterns in turn; every one inside its `every` bytes, so inside its row)
        p = torch.from_numpy(np.frombuffer(pats[7 + 1000 * k][:every - 1], dtype=np.uint8).copy()).to("cuda:0")
        mine = at[k::8]
        for j in range(len(p)):
            t[mine + j] = p[j]
    torch.cuda.synchronize()
    return a, t, [b"*" * len(p) for p in pats]


class DeviceWords:  # int64 words of the C ABI as torch sees them, without a copy
    def __init__(self, ptr, words):
        self.__cuda_array_interface__ = {"shape": (words,), "typestr": "<i8", "data": (ptr, False), "version": 2}


def variants_of(args, capi, torch, a, t, same_len):
    n, rows, info = t.numel(), args.rows, {}

    def find():
        r = a.find_device(t.data_ptr(), n, n_hay=rows, uniform_len=L)
        r.device_ptr  # (waits for the records)
        info["matches"] = r.count
        r.free()

    def mask(fill, flags):
        def run():
            m = a.mask_device(t.data_ptr(), n, fill, n_hay=rows, uniform_len=L, flags=flags)
            m.data_ptr()  # (waits for the stage)
            m.free()
        return run

    dst = torch.empty_like(t)

    def d2d_hay():
        dst.copy_(t)
        torch.cuda.synchronize()

    def replace_same_len():
        r = a.replace_device(t.data_ptr(), n, same_len, n_hay=rows, uniform_len=L)
        r.device_ptr  # (waits for the splice)
        info["replaced_bytes"] = r.nbytes
        r.free()

    def torch_mask():
        c = a.find_columns_device(t.data_ptr(), n, n_hay=rows, uniform_len=L)
        k = c.count
        st, en, ro = (torch.as_tensor(DeviceWords(c.data_ptr(w), max(words, 1)), device="cuda:0")[:words]
                      for w, words in ((capi.COL_START, k), (capi.COL_END, k), (capi.COL_ROW_OFFSETS, rows + 1)))
        row = torch.repeat_interleave(torch.arange(rows, device="cuda:0"), ro[1:] - ro[:-1])
        edge = torch.zeros(n + 1, dtype=torch.int32, device="cuda:0")
        one = torch.ones(k, dtype=torch.int32, device="cuda:0")
        edge.index_add_(0, row * L + st, one)
        edge.index_add_(0, row * L + en, -one)
        out = (edge.cumsum(0, dtype=torch.int32)[:-1] > 0).to(torch.uint8)
        info["torch_mask_bytes"] = int(out.sum())
        torch.cuda.synchronize()
        del st, en, ro, row, edge, one, out
        c.free()

    return {"find_a": find, "mask_all": mask(42, 0), "d2d_hay": d2d_hay, "match_mask": mask(1, capi.MASK_ZERO), "find_b": find,
            "replace_same_len": replace_same_len, "torch_mask": torch_mask}, info


def part_mask(args, every, capi, gen, np, torch):
    a, t, same_len = make_shape(args, every, capi, gen, np, torch)
    v, info = variants_of(args, capi, torch, a, t, same_len)
    ts = paired(v, args.steps, args.warmup, args.settle_ms)
    aa = [abs(x - y) for x, y in zip(ts["find_a"], ts["find_b"])]
    m = {n: round(1e3 * med(x), 4) for n, x in ts.items()}
    stage = 1e3 * med([s - f for s, f in zip(ts["mask_all"], ts["find_a"])])
    stage01 = 1e3 * med([s - f for s, f in zip(ts["match_mask"], ts["find_a"])])
    splice = 1e3 * med([s - f for s, f in zip(ts["replace_same_len"], ts["find_a"])])
    res = {"part": "mask", "rows": args.rows, "row_bytes": L, "planted_every": every, "matches": info.get("matches"),
           "replaced_bytes": info.get("replaced_bytes"), "covered_bytes": info.get("torch_mask_bytes"), "steps": args.steps, "ms": m,
           "aa_spread_ms": {"median": round(1e3 * med(aa), 4), "max": round(1e3 * max(aa), 4)},
           "mask_ms": round(stage, 4), "match_mask_ms": round(stage01, 4), "splice_ms": round(splice, 4),
           "mask_vs_copy": round(stage / m["d2d_hay"], 3) if m["d2d_hay"] else None,
           "mask_vs_splice": round(stage / splice, 3) if splice > 0 else None, "box": platform.node(), "date": time.strftime("%Y-%m-%d")}
    a.close()
    return res


def part_trace(args, every, capi, gen, np, torch):
    a, t, same_len = make_shape(args, every, capi, gen, np, torch)
    v, _ = variants_of(args, capi, torch, a, t, same_len)
    for _ in range(10):
        v["mask_all"]()
        v["match_mask"]()
    a.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=50.0)
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--every", type=int, nargs="+", default=[256])
    ap.add_argument("--parts", default="mask")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "mask_bench.jsonl"))
    args = ap.parse_args()
    import torch  # first: one process holds one HIP runtime (ahocorasick_rs_amd/__init__.py)
    import numpy as np
    import gen
    from ahocorasick_rs_amd import capi
    if args.parts == "trace":
        part_trace(args, args.every[0], capi, gen, np, torch)
        return
    if args.steps < 20:
        print("note: medians of fewer than 20 rounds are not what DESIGN.md section 18 asks for", file=sys.stderr)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    rows = []
    for every in args.every:
        res = part_mask(args, every, capi, gen, np, torch)
        line = json.dumps(res)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        rows.append(res)
    print("| shape | records | find (A) | find (A') | mask_all | mask - find | match_mask - find | D2D copy of the haystack | replace_all, same length | splice = replace - find | torch mask |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for res in rows:
        m = res["ms"]
        print("| %d x %d, a pattern every %d bytes | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s |" % (
            res["rows"], L, res["planted_every"], res["matches"], m["find_a"], m["find_b"], m["mask_all"], res["mask_ms"], res["match_mask_ms"],
            m["d2d_hay"], m["replace_same_len"], res["splice_ms"], m["torch_mask"]))


if __name__ == "__main__":
    main()
