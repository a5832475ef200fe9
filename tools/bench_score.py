"""Score benchmark (acx_score_device against the find beneath it, a device-to-device copy of the find's records and what a
caller does today through the tally; acx_filter_scored_device beside acx_filter_device; same box, same session, interleaved).

  python tools/bench_score.py [--steps K] [--warmup W] [--settle-ms MS] [--rows R] [--every B] [--parts score | trace]
                              [--out profiles/r13/score_bench.jsonl]

One JSON line per shape, appended to --out and printed, and the row of DESIGN.md section 17's table for it.  Every figure is
the median wall time per call over K rounds (at least 20); a round runs every variant once, in rotation, so that the
variants see the same clocks (paired, interleaved); the shape starts with the settle phase bench.py uses (untimed calls
for --settle-ms).

  shape     cfg2's batch shape in HBM: --rows (131 072) x 8 KiB = 1 GiB as ONE uint8 tensor of digits (no pattern of cfg2's
            10 000 lower-case ones occurs in them) with one of eight patterns planted every --every (256) bytes: about 4 M
            records, 96 MiB of them.  Weights: seeded, -9 .. 9.
  variants  find_a, find_b     acx_find_device on the uniform batch, waited for, freed -- twice per round: the floor, and their
                               spread is the A/A spread of the session
            score              acx_score_device, waited for
            d2d_records        a device-to-device copy of as many bytes as the find's records hold (24 per match; torch,
                               synchronised): what the score's one pass over the records is judged against
            tally_spmv         what a caller does today: acx_tally_device (a segmented sort of every record), then
                               torch.sparse_csr_tensor(...) @ w (float64: exact below 2^53, and torch has no integer sparse
                               product on the device), synchronised
            filter             acx_filter_device (min_matches = 1, keep the unmatched rows), waited for
            filter_scored      acx_filter_scored_device (min_score = 1, keep the unmatched rows), waited for
  "score_ms" = score - find_a per round (median): the stage's cost; "score_vs_copy" = score_ms / d2d_records;
  "scored_extra_ms" = filter_scored - filter per round (median): what the verdict by score adds to the filter.
  trace     no timing: ten rounds of score and filter_scored, for a kernel trace made in a run of its own, without counters:
              rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_score.py --parts trace
            (k_score_tiles, k_score, k_score_flags, the scan's k_rep_prefix / k_rep_partials; beside the find's own kernels)
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


def make_shape(args, capi, gen, np, torch):
    pats = gen.gen_patterns(10000, 5, 12, gen.AZ, 1)
    a = capi.Automaton(pats, 0, capi.IMPL_DFA)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(13)
    n = args.rows * L
    t = torch.randint(48, 58, (n,), dtype=torch.uint8, device="cuda:0", generator=g)
    at = torch.arange(0, n - 64, args.every, device="cuda:0")
    for k in range(8):  # (eight patterns in turn; every one inside its 256 bytes, so inside its row)
        p = torch.from_numpy(np.frombuffer(pats[7 + 1000 * k], dtype=np.uint8).copy()).to("cuda:0")
        mine = at[k::8]
        for j in range(len(p)):
            t[mine + j] = p[j]
    torch.cuda.synchronize()
    w = np.random.default_rng(13).integers(-9, 10, size=len(pats)).astype(np.int64)
    return a, t, w, len(pats)


class DeviceWords:  # int64 words of the C ABI as torch sees them, without a copy
    def __init__(self, ptr, words):
        self.__cuda_array_interface__ = {"shape": (words,), "typestr": "<i8", "data": (ptr, False), "version": 2}


def variants_of(args, capi, torch, a, t, w, n_patterns):
    n, rows, info = t.numel(), args.rows, {}

    def find():
        r = a.find_device(t.data_ptr(), n, n_hay=rows, uniform_len=L)
        r.device_ptr  # (waits for the records)
        info["matches"] = r.count
        r.free()

    def score():
        s = a.score_device(t.data_ptr(), n, w, n_hay=rows, uniform_len=L)
        s.data_ptr()  # (waits for the stage)
        s.free()

    find()
    record_bytes = 24 * info["matches"]
    src = torch.zeros(max(record_bytes, 1), dtype=torch.uint8, device="cuda:0")
    dst = torch.empty_like(src)

    def d2d_records():
        dst.copy_(src)
        torch.cuda.synchronize()

    w_dev = torch.from_numpy(w).to("cuda:0").to(torch.float64).unsqueeze(1)

    def tally_spmv():
        c = a.tally_device(t.data_ptr(), n, n_hay=rows, uniform_len=L)
        nnz = c.nnz
        parts = [torch.as_tensor(DeviceWords(c.data_ptr(k), max(words, 1)), device="cuda:0")[:words]
                 for k, words in ((capi.TALLY_ROW_OFFSETS, rows + 1), (capi.TALLY_PATTERN, nnz), (capi.TALLY_COUNT, nnz))]
        csr = torch.sparse_csr_tensor(parts[0], parts[1], parts[2].to(torch.float64), size=(rows, n_patterns))
        out = csr @ w_dev
        info["spmv_sum"] = float(out.sum())
        torch.cuda.synchronize()
        del csr, out, parts
        c.free()

    def filt():
        f = a.filter_device(t.data_ptr(), n, n_hay=rows, uniform_len=L)
        f.data_ptr(capi.FILT_DATA)  # (waits for the stage)
        info["kept_rows"] = f.n_rows
        f.free()

    def filt_scored():
        f = a.filter_scored_device(t.data_ptr(), n, w, n_hay=rows, uniform_len=L)
        f.data_ptr(capi.FILT_DATA)
        info["kept_rows_scored"] = f.n_rows
        f.free()

    return {"find_a": find, "score": score, "d2d_records": d2d_records, "tally_spmv": tally_spmv, "find_b": find,
            "filter": filt, "filter_scored": filt_scored}, info


def part_score(args, capi, gen, np, torch):
    a, t, w, n_patterns = make_shape(args, capi, gen, np, torch)
    v, info = variants_of(args, capi, torch, a, t, w, n_patterns)
    ts = paired(v, args.steps, args.warmup, args.settle_ms)
    aa = [abs(x - y) for x, y in zip(ts["find_a"], ts["find_b"])]
    m = {n: round(1e3 * med(x), 4) for n, x in ts.items()}
    stage = 1e3 * med([s - f for s, f in zip(ts["score"], ts["find_a"])])
    extra = 1e3 * med([s - f for s, f in zip(ts["filter_scored"], ts["filter"])])
    res = {"part": "score", "rows": args.rows, "row_bytes": L, "planted_every": args.every, "matches": info.get("matches"),
           "record_bytes": 24 * info.get("matches", 0), "kept_rows": info.get("kept_rows"),
           "kept_rows_scored": info.get("kept_rows_scored"), "steps": args.steps, "ms": m,
           "aa_spread_ms": {"median": round(1e3 * med(aa), 4), "max": round(1e3 * max(aa), 4)},
           "score_ms": round(stage, 4), "score_vs_copy": round(stage / m["d2d_records"], 3) if m["d2d_records"] else None,
           "scored_extra_ms": round(extra, 4), "box": platform.node(), "date": time.strftime("%Y-%m-%d")}
    a.close()
    return res


def part_trace(args, capi, gen, np, torch):
    a, t, w, n_patterns = make_shape(args, capi, gen, np, torch)
    v, _ = variants_of(args, capi, torch, a, t, w, n_patterns)
    for _ in range(10):
        v["score"]()
        v["filter_scored"]()
    a.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=50.0)
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--every", type=int, default=256)
    ap.add_argument("--parts", default="score")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "score_bench.jsonl"))
    args = ap.parse_args()
    import torch  # first: one process holds one HIP runtime (ahocorasick_rs_amd/__init__.py)
    import numpy as np
    import gen
    from ahocorasick_rs_amd import capi
    if args.parts == "trace":
        part_trace(args, capi, gen, np, torch)
        return
    if args.steps < 20:
        print("note: medians of fewer than 20 rounds are not what DESIGN.md section 17 asks for", file=sys.stderr)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    res = part_score(args, capi, gen, np, torch)
    line = json.dumps(res)
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    m = res["ms"]
    print("| shape | records | find (A) | find (A') | score | score - find | D2D copy of the records | tally + spmv | filter | filter_scored |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    print("| %d x %d | %s | %s | %s | %s | %s | %s | %s | %s | %s |" % (res["rows"], L, res["matches"], m["find_a"], m["find_b"], m["score"],
                                                                       res["score_ms"], m["d2d_records"], m["tally_spmv"], m["filter"],
                                                                       m["filter_scored"]))


if __name__ == "__main__":
    main()
