"""Span benchmark (acx_spans_device against the find beneath it, the split into columns, the 0 / 1 mask and the torch merge
over the columns -- the only way to get merged spans before; same box, same session, interleaved).

  python tools/bench_spans.py [--steps K] [--warmup W] [--settle-ms MS] [--rows R] [--every B [B ...]] [--parts spans | trace]
                              [--out profiles/r16/spans_bench.jsonl]

One JSON line per shape, appended to --out and printed, and the row of DESIGN.md section 20's table for it.  Every figure is
the median wall time per call over K rounds (at least 20); a round runs every variant once, in rotation, so that the
variants see the same clocks (paired, interleaved); the shape starts with the settle phase bench.py uses (untimed calls
for --settle-ms).  Before anything is timed the spans of both gaps are compared with the torch merge, entry by entry.

  shape     cfg2's batch shape in HBM: --rows (131 072) x 8 KiB = 1 GiB as ONE uint8 tensor of digits (no pattern of cfg2's
            10 000 lower-case ones occurs in them) with one of eight patterns planted every --every bytes: 256 (about 4 M
            records), and the dense end of the curve, 64 and 32 (--every 256 64 32 runs the three one after the other).
  variants  find_a, find_b     acx_find_device on the uniform batch, waited for, freed -- twice per round: the floor, and their
                               spread is the A/A spread of the session
            spans_gap0         acx_spans_device with gap 0, waited for
            spans_gap64        acx_spans_device with gap 64, waited for
            columns            acx_find_columns_device, waited for: the split of the same records, 24 bytes read and 24
                               written per match -- what the stage's two reads of 16 bytes are judged against
            match_mask         acx_mask_device (ACX_MASK_ZERO, fill 1), waited for: the full-length form of the same cover
            torch_merge        find_columns_device, then a stable sort by (row, start), a running maximum of the ends and a
                               compare in torch (gap 0), synchronised
  "spans_ms" = spans_gap0 - find_a per round (median): the stage's cost; "split_ms" = columns - find_a per round (median);
  "spans_vs_split" = spans_ms / split_ms; "over_split_ms" = spans_ms - split_ms, to be held against the A/A spread.
  trace     no timing: ten rounds of spans_gap0 and spans_gap64, for a kernel trace made in a run of its own, without counters:
              rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_spans.py --parts trace
            (k_span_tiles, k_span_carry, k_span_count, k_span_emit, the scan's k_rep_prefix / k_rep_partials; beside the
            find's own kernels)
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


class DeviceWords:  # int64 words of the C ABI as torch sees them, without a copy
    def __init__(self, ptr, words):
        self.__cuda_array_interface__ = {"shape": (words,), "typestr": "<i8", "data": (ptr, False), "version": 2}


def words_of(torch, r, which, words):
    return torch.as_tensor(DeviceWords(r.data_ptr(which), max(words, 1)), device="cuda:0")[:words]


def torch_merge(args, capi, torch, a, t, gap):
    """the merged spans from the columns, in torch -> (start, end, row_offsets); the rows are moved 2 L apart, so that no
    gap below L joins two of them"""
    n, rows = t.numel(), args.rows
    c = a.find_columns_device(t.data_ptr(), n, n_hay=rows, uniform_len=L)
    k = c.count
    st, en, ro = (words_of(torch, c, w, words) for w, words in ((capi.COL_START, k), (capi.COL_END, k), (capi.COL_ROW_OFFSETS, rows + 1)))
    row = torch.repeat_interleave(torch.arange(rows, device="cuda:0"), ro[1:] - ro[:-1])
    live = st < en
    row, ks, ke = row[live], (row * (2 * L) + st)[live], (row * (2 * L) + en)[live]
    order = torch.argsort(ks, stable=True)
    row, ks, ke = row[order], ks[order], ke[order]
    reach = torch.cummax(ke, 0).values
    opens = torch.ones(len(ks), dtype=torch.bool, device="cuda:0")
    opens[1:] = ks[1:] - reach[:-1] > gap
    closes = torch.cat([opens[1:], torch.ones(1, dtype=torch.bool, device="cuda:0")])
    shift = row * (2 * L)
    out = (ks - shift)[opens], (reach - shift)[closes], torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda:0"),
                                                                   torch.bincount(row[opens], minlength=rows).cumsum(0)])
    torch.cuda.synchronize()
    c.free()
    return out


def variants_of(args, capi, torch, a, t):
    n, rows, info = t.numel(), args.rows, {}

    def find():
        r = a.find_device(t.data_ptr(), n, n_hay=rows, uniform_len=L)
        r.device_ptr  # (waits for the records)
        info["matches"] = r.count
        r.free()

    def spans(gap):
        def run():
            s = a.spans_device(t.data_ptr(), n, n_hay=rows, uniform_len=L, gap=gap)
            s.data_ptr(capi.SPAN_ROW_OFFSETS)  # (waits for the stage)
            info["spans_gap%d" % gap] = s.count
            s.free()
        return run

    def columns():
        c = a.find_columns_device(t.data_ptr(), n, n_hay=rows, uniform_len=L)
        c.data_ptr(capi.COL_ROW_OFFSETS)  # (waits for the split and the scan)
        c.free()

    def match_mask():
        m = a.mask_device(t.data_ptr(), n, 1, n_hay=rows, uniform_len=L, flags=capi.MASK_ZERO)
        m.data_ptr()  # (waits for the stage)
        m.free()

    def merge():
        out = torch_merge(args, capi, torch, a, t, 0)
        del out

    return {"find_a": find, "spans_gap0": spans(0), "columns": columns, "spans_gap64": spans(64), "find_b": find, "match_mask": match_mask,
            "torch_merge": merge}, info


def check_against_torch(args, capi, torch, a, t):
    """the stage's spans and the torch merge, entry by entry, for both gaps: no figure of a wrong result is taken"""
    n, rows = t.numel(), args.rows
    for gap in (0, 64):
        s = a.spans_device(t.data_ptr(), n, n_hay=rows, uniform_len=L, gap=gap)
        k = s.count
        got = [words_of(torch, s, w, words) for w, words in ((capi.SPAN_START, k), (capi.SPAN_END, k), (capi.SPAN_ROW_OFFSETS, rows + 1))]
        want = torch_merge(args, capi, torch, a, t, gap)
        for name, g, w in zip(("start", "end", "row_offsets"), got, want):
            if g.shape != w.shape or not torch.equal(g, w):
                raise SystemExit("gap %d: the stage's %s differ from the torch merge (%d against %d entries)" % (gap, name, len(g), len(w)))
        del got, want
        s.free()


def part_spans(args, every, capi, gen, np, torch):
    a, t = make_shape(args, every, capi, gen, np, torch)
    check_against_torch(args, capi, torch, a, t)
    v, info = variants_of(args, capi, torch, a, t)
    ts = paired(v, args.steps, args.warmup, args.settle_ms)
    aa = [abs(x - y) for x, y in zip(ts["find_a"], ts["find_b"])]
    m = {n: round(1e3 * med(x), 4) for n, x in ts.items()}
    stage = 1e3 * med([s - f for s, f in zip(ts["spans_gap0"], ts["find_a"])])
    stage64 = 1e3 * med([s - f for s, f in zip(ts["spans_gap64"], ts["find_a"])])
    split = 1e3 * med([s - f for s, f in zip(ts["columns"], ts["find_a"])])
    mask = 1e3 * med([s - f for s, f in zip(ts["match_mask"], ts["find_a"])])
    over = 1e3 * med([(s - f) - (c - f) for s, c, f in zip(ts["spans_gap0"], ts["columns"], ts["find_a"])])
    res = {"part": "spans", "rows": args.rows, "row_bytes": L, "planted_every": every, "matches": info.get("matches"),
           "spans_gap0": info.get("spans_gap0"), "spans_gap64": info.get("spans_gap64"), "steps": args.steps, "ms": m,
           "aa_spread_ms": {"median": round(1e3 * med(aa), 4), "max": round(1e3 * max(aa), 4)},
           "spans_ms": round(stage, 4), "spans_gap64_ms": round(stage64, 4), "split_ms": round(split, 4), "match_mask_ms": round(mask, 4),
           "over_split_ms": round(over, 4), "spans_vs_split": round(stage / split, 3) if split > 0 else None,
           "checked_against_torch": True, "box": platform.node(), "date": time.strftime("%Y-%m-%d")}
    a.close()
    return res


def part_trace(args, every, capi, gen, np, torch):
    a, t = make_shape(args, every, capi, gen, np, torch)
    v, _ = variants_of(args, capi, torch, a, t)
    for _ in range(10):
        v["spans_gap0"]()
        v["spans_gap64"]()
    a.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=50.0)
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--every", type=int, nargs="+", default=[256])
    ap.add_argument("--parts", default="spans")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "spans_bench.jsonl"))
    args = ap.parse_args()
    import torch  # first: one process holds one HIP runtime (ahocorasick_rs_amd/__init__.py)
    import numpy as np
    import gen
    from ahocorasick_rs_amd import capi
    if args.parts == "trace":
        part_trace(args, args.every[0], capi, gen, np, torch)
        return
    if args.steps < 20:
        print("note: medians of fewer than 20 rounds are not what DESIGN.md section 20 asks for", file=sys.stderr)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    rows = []
    for every in args.every:
        res = part_spans(args, every, capi, gen, np, torch)
        line = json.dumps(res)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        rows.append(res)
    print("| shape | records | spans, gap 0 | spans, gap 64 | find (A) | find (A') | A/A spread (median) | spans - find, gap 0 | spans - find, gap 64 | columns - find | "
          "(spans - find) - (columns - find) | match_mask - find | torch merge |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for res in rows:
        m = res["ms"]
        print("| %d x %d, a pattern every %d bytes | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s |" % (
            res["rows"], L, res["planted_every"], res["matches"], res["spans_gap0"], res["spans_gap64"], m["find_a"], m["find_b"],
            res["aa_spread_ms"]["median"], res["spans_ms"], res["spans_gap64_ms"], res["split_ms"], res["over_split_ms"], res["match_mask_ms"],
            m["torch_merge"]))


if __name__ == "__main__":
    main()
