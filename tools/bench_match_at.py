"""Match-at benchmark (acx_match_at_device in its prefix form and on free positions, against the find alone on the same data,
a device-to-device copy of the stage's own columns and the only way before: an overlapping find plus a torch filter on the
starts -- same box, same session, interleaved).

  python tools/bench_match_at.py [--steps K] [--warmup W] [--settle-ms MS] [--rows R] [--every B [B ...]] [--parts at | trace]
                                 [--out profiles/r20/match_at_bench.jsonl]

One JSON line per shape, appended to --out and printed, and the row of DESIGN.md section 24's table for it.  Every figure is
the median wall time per call over K rounds (at least 20); a round runs every variant once, in rotation, so that the
variants see the same clocks (paired, interleaved); the shape starts with the settle phase bench.py uses (untimed calls
for --settle-ms).  Before anything is timed the new results are compared with the old way's, entry by entry.

  shape     cfg2's batch shape in HBM: --rows (131 072) x 8 KiB = 1 GiB as ONE uint8 tensor of digits (no pattern of cfg2's
            10 000 lower-case ones occurs in them).  Positions: one per --every bytes (4, 16, 64), each at a seeded place
            inside its --every bytes, ONE ascending int64 tensor in HBM; one of eight patterns is planted at every 64th of
            them and at the start of every fourth row.  The share of anchors at which a pattern begins is counted, not
            assumed ("positions_with_a_pattern", "rows_with_a_prefix").  No 8 KiB row IS a pattern: the full form's walks
            all run to the end of their pattern and report nothing.
  variants  find_a, find_b     acx_find_device on the uniform batch, waited for, freed -- twice per round: the find alone on
                               the same data, and their spread is the A/A spread of the session
            prefix             acx_match_at_device, ACX_AT_ROW_STARTS, uniform rows, waited for
            prefix_full        ... with ACX_AT_FULL
            match_at           acx_match_at_device on the positions, uniform rows, waited for
            copy               the stage's own columns moved by torch, device to device: the positions in, two columns of as
                               many words out (A words read, 2 A written), synchronised: its traffic floor
            old_way            find_columns_device(overlapping) plus torch.isin(row * 8192 + start, positions), synchronised
            old_prefix         find_columns_device(overlapping) plus start == 0, synchronised
  trace     no timing: ten rounds of prefix and match_at, for a kernel trace made in a run of its own, without counters:
              rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_match_at.py --parts trace
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
SHARE = 64  # a pattern at every SHARE-th position


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


class DeviceWords:  # words of the C ABI as torch sees them, without a copy
    def __init__(self, ptr, words, typestr="<i8"):
        self.__cuda_array_interface__ = {"shape": (words,), "typestr": typestr, "data": (ptr, False), "version": 2}


def words_at(torch, ptr, words):
    return torch.as_tensor(DeviceWords(ptr, max(words, 1)), device="cuda:0")[:words]


def make_shape(args, every, capi, gen, np, torch):
    pats = gen.gen_patterns(10000, 5, 12, gen.AZ, 1)
    a = capi.Automaton(pats, 0, capi.IMPL_DFA)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(13)
    n = args.rows * L
    t = torch.randint(48, 58, (n,), dtype=torch.uint8, device="cuda:0", generator=g)
    slots = n // every
    pos = (torch.arange(slots, dtype=torch.int64, device="cuda:0") * every +
           torch.randint(0, every, (slots,), dtype=torch.int64, device="cuda:0", generator=g)).contiguous()
    planted = [torch.from_numpy(np.frombuffer(pats[7 + 1000 * k], dtype=np.uint8).copy()).to("cuda:0") for k in range(8)]
    for k, p in enumerate(planted):  # (a pattern inside the tensor and inside its row)
        mine = pos[SHARE * k + 7::8 * SHARE]
        mine = mine[(mine % L) + len(p) <= L]
        for j in range(len(p)):
            t[mine + j] = p[j]
    starts = torch.arange(0, args.rows, 4, dtype=torch.int64, device="cuda:0") * L
    for k, p in enumerate(planted):
        mine = starts[k::8]
        for j in range(len(p)):
            t[mine + j] = p[j]
    torch.cuda.synchronize()
    return a, t, pos


def prefix(a, t, rows, flags):
    return a.match_at_device(t.data_ptr(), t.numel(), 0, 0, flags, n_hay=rows, uniform_len=L)


def at(a, t, pos, rows, flags=0):
    return a.match_at_device(t.data_ptr(), t.numel(), pos.data_ptr(), pos.numel(), flags, n_hay=rows, uniform_len=L)


def old_way(args, capi, torch, a, t, pos, row_starts):
    """the overlapping find's columns filtered in torch -> (start, end, pattern) of the records that begin at a position
    (row_starts: at the start of their row), global, sorted by (start, end, pattern)"""
    n, rows = t.numel(), args.rows
    c = a.find_columns_device(t.data_ptr(), n, n_hay=rows, uniform_len=L, overlapping=True)
    k = c.count
    pt, st, en = (words_at(torch, c.data_ptr(w), k) for w in (capi.COL_PATTERN, capi.COL_START, capi.COL_END))
    ro = words_at(torch, c.data_ptr(capi.COL_ROW_OFFSETS), rows + 1)
    row = torch.repeat_interleave(torch.arange(rows, device="cuda:0"), ro[1:] - ro[:-1])
    gs = row * L + st
    keep = (st == 0) if row_starts else torch.isin(gs, pos)
    out = (gs[keep], (row * L + en)[keep], pt[keep].clone())
    torch.cuda.synchronize()
    c.free()
    return out


def check_against_old(args, capi, torch, a, t, pos):
    """the new results and the old way's, entry by entry: no figure of a wrong result is taken"""
    rows = args.rows
    for row_starts in (False, True):
        gs, ge, pt = old_way(args, capi, torch, a, t, pos, row_starts)
        order = torch.argsort(pt, stable=True)
        order = order[torch.argsort(ge[order], stable=True)]
        order = order[torch.argsort(gs[order], stable=True)]
        gs, ge, pt = gs[order], ge[order], pt[order]
        r = prefix(a, t, rows, capi.AT_OVERLAPPING | capi.AT_ROW_STARTS) if row_starts else at(a, t, pos, rows, capi.AT_OVERLAPPING)
        A, E = r.count, r.entries
        if E != gs.numel():
            raise SystemExit("match_at reports %d entries, the old way %d (row_starts=%s)" % (E, gs.numel(), row_starts))
        ro = words_at(torch, r.row_offsets_ptr(), A + 1)
        anchors = torch.arange(rows, device="cuda:0") * L if row_starts else pos
        start = torch.repeat_interleave(anchors, ro[1:] - ro[:-1])
        end = words_at(torch, r.end_ptr(), E) + (start if row_starts else 0)
        pattern = words_at(torch, r.pattern_ptr(), E)
        if not (torch.equal(start, gs) and torch.equal(end, ge) and torch.equal(pattern, pt)):
            raise SystemExit("match_at differs from the old way (row_starts=%s)" % row_starts)
        # ... and the form that is timed: per anchor the first entry (Standard: the smallest end, then the lowest index)
        r1 = prefix(a, t, rows, capi.AT_ROW_STARTS) if row_starts else at(a, t, pos, rows)
        first = torch.full((A,), -1, dtype=torch.int64, device="cuda:0")
        has = ro[1:] > ro[:-1]
        first[has] = pattern[ro[:-1][has]]
        if not torch.equal(words_at(torch, r1.pattern_ptr(), A), first):
            raise SystemExit("the non-overlapping form differs from the first entry of the overlapping one")
        hits = int(has.sum())
        r.free()
        r1.free()
        if not row_starts:
            at_hits = hits
    return at_hits, hits


def variants_of(args, capi, torch, a, t, pos):
    n, rows, info = t.numel(), args.rows, {}
    out_p, out_e = torch.empty_like(pos), torch.empty_like(pos)

    def find():
        r = a.find_device(t.data_ptr(), n, n_hay=rows, uniform_len=L)
        r.device_ptr  # (waits for the records)
        info["matches"] = r.count
        r.free()

    def run(make):
        def f():
            r = make()
            r.end_ptr()  # (waits for the walk)
            r.free()
        return f

    def copy():
        out_p.copy_(pos)
        out_e.copy_(pos)
        torch.cuda.synchronize()

    def old(row_starts):
        def f():
            out = old_way(args, capi, torch, a, t, pos, row_starts)
            del out
        return f

    return {"find_a": find, "prefix": run(lambda: prefix(a, t, rows, capi.AT_ROW_STARTS)),
            "prefix_full": run(lambda: prefix(a, t, rows, capi.AT_ROW_STARTS | capi.AT_FULL)),
            "match_at": run(lambda: at(a, t, pos, rows)), "copy": copy, "old_way": old(False), "old_prefix": old(True),
            "find_b": find}, info


def part_at(args, every, capi, gen, np, torch):
    a, t, pos = make_shape(args, every, capi, gen, np, torch)
    at_hits, prefix_hits = check_against_old(args, capi, torch, a, t, pos)
    v, info = variants_of(args, capi, torch, a, t, pos)
    ts = paired(v, args.steps, args.warmup, args.settle_ms)
    aa = [abs(x - y) for x, y in zip(ts["find_a"], ts["find_b"])]
    m = {n: round(1e3 * med(x), 4) for n, x in ts.items()}
    res = {"part": "at", "rows": args.rows, "row_bytes": L, "position_every": every, "positions": pos.numel(),
           "positions_with_a_pattern": at_hits, "rows_with_a_prefix": prefix_hits, "find_matches": info.get("matches"),
           "steps": args.steps, "ms": m, "aa_spread_ms": {"median": round(1e3 * med(aa), 4), "max": round(1e3 * max(aa), 4)},
           "prefix_vs_find": round(m["prefix"] / m["find_a"], 4) if m["find_a"] else None,
           "match_at_vs_copy": round(m["match_at"] / m["copy"], 3) if m["copy"] else None,
           "old_way_vs_match_at": round(m["old_way"] / m["match_at"], 2) if m["match_at"] else None,
           "old_prefix_vs_prefix": round(m["old_prefix"] / m["prefix"], 2) if m["prefix"] else None,
           "checked_against_old_way": True, "box": platform.node(), "date": time.strftime("%Y-%m-%d")}
    a.close()
    return res


def part_trace(args, every, capi, gen, np, torch):
    a, t, pos = make_shape(args, every, capi, gen, np, torch)
    v, _ = variants_of(args, capi, torch, a, t, pos)
    for _ in range(10):
        v["prefix"]()
        v["match_at"]()
    a.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=50.0)
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--every", type=int, nargs="+", default=[64, 16, 4])
    ap.add_argument("--parts", default="at")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20", "match_at_bench.jsonl"))
    args = ap.parse_args()
    import torch  # first: one process holds one HIP runtime (ahocorasick_rs_amd/__init__.py)
    import numpy as np
    import gen
    from ahocorasick_rs_amd import capi
    if args.parts == "trace":
        part_trace(args, args.every[0], capi, gen, np, torch)
        return
    if args.steps < 20:
        print("note: medians of fewer than 20 rounds are not what DESIGN.md section 24 asks for", file=sys.stderr)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    rows = []
    for every in args.every:
        res = part_at(args, every, capi, gen, np, torch)
        line = json.dumps(res)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        rows.append(res)
    print("| a position every | positions (with a pattern) | find (A) | find (A') | A/A spread (median) | prefix | prefix, full | match_at | copy of its columns | old way | old way, prefix |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for res in rows:
        m = res["ms"]
        print("| %d bytes | %s (%s) | %s | %s | %s | %s | %s | %s | %s | %s | %s |" % (
            res["position_every"], res["positions"], res["positions_with_a_pattern"], m["find_a"], m["find_b"],
            res["aa_spread_ms"]["median"], m["prefix"], m["prefix_full"], m["match_at"], m["copy"], m["old_way"], m["old_prefix"]))


if __name__ == "__main__":
    main()
