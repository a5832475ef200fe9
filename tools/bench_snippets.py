"""Snippet benchmark (acx_snippets_device against the find beneath it, the split into columns, a copy of the output's bytes
and the torch index form over the columns -- the only way to cut snippets before; same box, same session, interleaved).

  python tools/bench_snippets.py [--steps K] [--warmup W] [--settle-ms MS] [--rows R] [--every B [B ...]]
                                 [--context C [C ...]] [--torch-max-bytes N] [--parts snippets | trace]
                                 [--out profiles/r17/snippets_bench.jsonl]

One JSON line per shape, appended to --out and printed, and the row of DESIGN.md section 21's table for it.  Every figure is
the median wall time per call over K rounds (at least 20); a round runs every variant once, in rotation, so that the
variants see the same clocks (paired, interleaved); the shape starts with the settle phase bench.py uses (untimed calls
for --settle-ms).  Before anything is timed the snippets are compared with the torch index form, byte by byte.

  shape     cfg2's batch shape in HBM: --rows (131 072) x 8 KiB = 1 GiB as ONE uint8 tensor of digits (no pattern of cfg2's
            10 000 lower-case ones occurs in them) with one of eight patterns planted every --every bytes (256, 64, 32) and a
            --context of 0, 32 and 128 bytes: nine shapes (the default runs them one after the other).
  variants  find_a, find_b   acx_find_device on the uniform batch, waited for, freed -- twice per round: the floor, and their
                             spread is the A/A spread of the session
            columns          acx_find_columns_device, waited for
            snippets         acx_snippets_device, waited for (the gather included)
            copy             a device-to-device copy of the output's bytes
            torch_index      find_columns_device, then repeat_interleave + arange + index in torch, synchronised: an 8-byte
                             index per output byte.  Skipped (null) where the output exceeds --torch-max-bytes (2 GiB): the
                             indexes alone would be 8 times that.
  "snippets_ms" = snippets - find_a per round (median): the stage's cost; "split_ms" = columns - find_a per round (median).
  The gather alone against filter_gather fed the same offsets and sources is tools/ubench_snippets.hip's figure.
  trace     no timing: ten rounds of snippets, for a kernel trace made in a run of its own, without counters:
              rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_snippets.py --parts trace
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
    return a, t


class DeviceArray:  # a part of the C ABI's result as torch sees it, without a copy
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


def words_of(torch, r, which, words):
    return torch.as_tensor(DeviceArray(r.data_ptr(which), max(words, 1), "<i8"), device="cuda:0")[:words]


def bytes_of(torch, r, which, n):
    return torch.as_tensor(DeviceArray(r.data_ptr(which), max(n, 1), "|u1"), device="cuda:0")[:n]


def torch_index(args, capi, torch, a, t, context):
    """the snippets from the columns, in torch: the definition on the columns, then one index per output byte"""
    n, rows = t.numel(), args.rows
    c = a.find_columns_device(t.data_ptr(), n, n_hay=rows, uniform_len=L)
    k = c.count
    st, en, ro = (words_of(torch, c, w, words) for w, words in ((capi.COL_START, k), (capi.COL_END, k), (capi.COL_ROW_OFFSETS, rows + 1)))
    row = torch.repeat_interleave(torch.arange(rows, device="cuda:0"), ro[1:] - ro[:-1])
    lo = st - torch.clamp(st, max=context)
    hi = en + torch.clamp(L - en, max=context)
    seg = hi - lo
    offs = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda:0"), seg.cumsum(0)])
    idx = torch.repeat_interleave(row * L + lo - offs[:-1], seg) + torch.arange(int(offs[-1]), device="cuda:0")
    out = t[idx], offs, st - lo
    torch.cuda.synchronize()
    c.free()
    return out


def variants_of(args, capi, torch, a, t, context, with_torch):
    n, rows, info = t.numel(), args.rows, {}

    def find():
        r = a.find_device(t.data_ptr(), n, n_hay=rows, uniform_len=L)
        r.device_ptr  # (waits for the records)
        info["matches"] = r.count
        r.free()

    def snippets():
        s = a.snippets_device(t.data_ptr(), n, n_hay=rows, uniform_len=L, context=context)
        s.data_ptr(capi.SNIP_DATA)  # (waits for the gather)
        info["output_bytes"] = s.nbytes
        s.free()

    def columns():
        c = a.find_columns_device(t.data_ptr(), n, n_hay=rows, uniform_len=L)
        c.data_ptr(capi.COL_ROW_OFFSETS)  # (waits for the split and the scan)
        c.free()

    snippets()
    src = torch.empty(info["output_bytes"], dtype=torch.uint8, device="cuda:0")
    dst = torch.empty_like(src)

    def copy():
        dst.copy_(src)
        torch.cuda.synchronize()

    def index():
        out = torch_index(args, capi, torch, a, t, context)
        del out

    v = {"find_a": find, "snippets": snippets, "columns": columns, "copy": copy, "find_b": find}
    if with_torch:
        v["torch_index"] = index
    return v, info


def check_against_torch(args, capi, torch, a, t, context):
    """the stage's snippets and the torch index form, byte by byte: no figure of a wrong result is taken"""
    n, rows = t.numel(), args.rows
    s = a.snippets_device(t.data_ptr(), n, n_hay=rows, uniform_len=L, context=context)
    k = s.count
    want_data, want_offs, want_lead = torch_index(args, capi, torch, a, t, context)
    got = (bytes_of(torch, s, capi.SNIP_DATA, s.nbytes), words_of(torch, s, capi.SNIP_OFFSETS, k + 1), words_of(torch, s, capi.SNIP_LEAD, k))
    for name, g, w in zip(("data", "offsets", "lead"), got, (want_data, want_offs, want_lead)):
        if g.shape != w.shape or not torch.equal(g, w):
            raise SystemExit("context %d: the stage's %s differ from the torch index form (%d against %d entries)" % (context, name, len(g), len(w)))
    del got, want_data, want_offs, want_lead
    s.free()


def part_snippets(args, a, t, every, context, capi, torch):
    probe = a.snippets_device(t.data_ptr(), t.numel(), n_hay=args.rows, uniform_len=L, context=context)
    out_bytes = probe.nbytes
    probe.free()
    with_torch = out_bytes <= args.torch_max_bytes
    if with_torch:
        check_against_torch(args, capi, torch, a, t, context)
    v, info = variants_of(args, capi, torch, a, t, context, with_torch)
    ts = paired(v, args.steps, args.warmup, args.settle_ms)
    aa = [abs(x - y) for x, y in zip(ts["find_a"], ts["find_b"])]
    m = {n: round(1e3 * med(x), 4) for n, x in ts.items()}
    m.setdefault("torch_index", None)
    stage = 1e3 * med([s - f for s, f in zip(ts["snippets"], ts["find_a"])])
    split = 1e3 * med([s - f for s, f in zip(ts["columns"], ts["find_a"])])
    return {"part": "snippets", "rows": args.rows, "row_bytes": L, "planted_every": every, "context": context, "matches": info.get("matches"),
            "output_bytes": info.get("output_bytes"), "steps": args.steps, "ms": m,
            "aa_spread_ms": {"median": round(1e3 * med(aa), 4), "max": round(1e3 * max(aa), 4)},
            "snippets_ms": round(stage, 4), "split_ms": round(split, 4), "checked_against_torch": with_torch, "box": platform.node(),
            "date": time.strftime("%Y-%m-%d")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=50.0)
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--every", type=int, nargs="+", default=[256, 64, 32])
    ap.add_argument("--context", type=int, nargs="+", default=[0, 32, 128])
    ap.add_argument("--torch-max-bytes", type=int, default=2 << 30)
    ap.add_argument("--parts", default="snippets")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17", "snippets_bench.jsonl"))
    args = ap.parse_args()
    import torch  # first: one process holds one HIP runtime (ahocorasick_rs_amd/__init__.py)
    import numpy as np
    import gen
    from ahocorasick_rs_amd import capi
    if args.parts == "trace":
        a, t = make_shape(args, args.every[0], capi, gen, np, torch)
        for _ in range(10):
            s = a.snippets_device(t.data_ptr(), t.numel(), n_hay=args.rows, uniform_len=L, context=args.context[-1])
            s.data_ptr(capi.SNIP_DATA)
            s.free()
        a.close()
        return
    if args.steps < 20:
        print("note: medians of fewer than 20 rounds are not what DESIGN.md section 21 asks for", file=sys.stderr)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    rows = []
    for every in args.every:
        a, t = make_shape(args, every, capi, gen, np, torch)
        for context in args.context:
            res = part_snippets(args, a, t, every, context, capi, torch)
            line = json.dumps(res)
            print(line, flush=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
            rows.append(res)
        a.close()
        del t
        torch.cuda.empty_cache()
    print("| shape | context | records | output bytes | snippets | find (A) | find (A') | A/A spread (median) | snippets - find | columns - find | copy | torch index |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for res in rows:
        m = res["ms"]
        print("| %d x %d, a pattern every %d bytes | %d | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s |" % (
            res["rows"], L, res["planted_every"], res["context"], res["matches"], res["output_bytes"], m["snippets"], m["find_a"], m["find_b"],
            res["aa_spread_ms"]["median"], res["snippets_ms"], res["split_ms"], m["copy"], m["torch_index"]))


if __name__ == "__main__":
    main()
