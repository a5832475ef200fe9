"""Segment benchmark (acx_segment_device on cfg2's batch shape and on the same bytes as ONE row, against the find alone on the
same data, a device-to-device copy of the stage's own columns, match_at at EVERY byte position -- what any other route to the
chain needs before its chase can even start -- and a one-core re.finditer of the alternation on a slice; same box, same
session, interleaved).

  python tools/bench_segment.py [--steps K] [--warmup W] [--settle-ms MS] [--rows R] [--cover C [C ...]] [--re-mib M]
                                [--re-seconds S] [--out profiles/r21/segment_bench.jsonl]

One JSON line per coverage, appended to --out and printed, and the row of DESIGN.md section 25's table for it.  Every figure
is the median wall time per call over K rounds (at least 20); a round runs every variant once, in rotation, so that the
variants see the same clocks (paired, interleaved); the shape starts with the settle phase bench.py uses (untimed calls for
--settle-ms).  Before anything is timed the device result of a slice is compared with acx_segment_host, entry by entry.

  shape     cfg2's batch shape in HBM: --rows (131 072) x 8 KiB = 1 GiB as ONE uint8 tensor.  A 4 MiB paragraph -- words of
            cfg2's 10 000 lower-case patterns (a LeftmostLongest handle: MaxMatch) between runs of digits, which no pattern
            holds -- repeated to the size; --cover (0.5, 0.95) steers the share of bytes the dictionary covers, and the share
            that IS covered is counted from the result, with T ("pieces", "covered").
  variants  find_a, find_b     acx_find_device on the uniform batch, waited for, freed -- twice per round: the find alone, and
                               their spread is the A/A spread of the session
            segment_batch      acx_segment_device, uniform rows, waited for
            segment_one        ... the same bytes as ONE row
            count_only         acx_segment_into_device with cap = 0: k_seg<COUNT> and the tree, no emit -- the split of the
                               call from outside, without a profiler
            copy               the stage's own columns moved by torch, device to device: T, T + 1 and rows + 1 words,
                               synchronised: its traffic floor
            match_at_all       acx_match_at_device on EVERY byte position (an int64 per byte in, two out), uniform rows
  re        once, untimed by the rounds: re.finditer of P_0|P_1|...|(?s:.) with the words longest first, on the first
            --re-mib (64) MiB, one core; it is stopped after --re-seconds and says how far it got
"""
import argparse
import json
import os
import platform
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

L = 8192
PARAGRAPH = 4 << 20


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


def paragraph(pats, cover, np):
    """PARAGRAPH bytes: a word, then digits, so that about `cover` of the bytes are words"""
    rng = np.random.default_rng(int(cover * 1000))
    out, size = [], 0
    while size < PARAGRAPH + 64:
        w = pats[int(rng.integers(0, len(pats)))]
        gap = int(rng.poisson(len(w) * (1 - cover) / cover)) if cover < 1 else 0
        out.append(w)
        out.append(bytes(rng.integers(48, 58, size=gap, dtype=np.uint8)))
        size += len(w) + gap
    return b"".join(out)[:PARAGRAPH]


def make_shape(args, cover, capi, gen, np, torch):
    pats = gen.gen_patterns(10000, 5, 12, gen.AZ, 1)
    a = capi.Automaton(pats, capi.MATCH_LEFTMOST_LONGEST)
    para = paragraph(pats, cover, np)
    n = args.rows * L
    t = torch.from_numpy(np.frombuffer(para, dtype=np.uint8).copy()).to("cuda:0").repeat((n + PARAGRAPH - 1) // PARAGRAPH)[:n].contiguous()
    torch.cuda.synchronize()
    return a, t, pats, para


def check_against_host(args, capi, np, torch, a, t, pats, para):
    """the device result of the first paragraph, cut into rows, against acx_segment_host, entry by entry"""
    n = min(PARAGRAPH, t.numel())
    rows = n // L
    r = a.segment_device(t.data_ptr(), n, n_hay=rows, uniform_len=L)
    h = capi.HostAutomaton(pats, capi.MATCH_LEFTMOST_LONGEST)
    want = capi.segment_host(h, para[:n], offsets=np.arange(0, n + 1, L), match_kind=capi.MATCH_LEFTMOST_LONGEST)
    h.close()
    got = (r.pattern(), r.offsets(), r.row_offsets())
    for g, w, name in zip(got, want, ("pattern", "offsets", "row_offsets")):
        if not np.array_equal(g, w):
            raise SystemExit("segment_device differs from acx_segment_host in %s" % name)
    r.free()


def variants_of(args, capi, torch, a, t):
    n, rows, info = t.numel(), args.rows, {}
    r = a.segment_device(t.data_ptr(), n, n_hay=rows, uniform_len=L)
    T = r.count
    pat, off = words_at(torch, r.pattern_ptr(), T), words_at(torch, r.offsets_ptr(), T + 1)
    info["pieces"] = T
    info["covered"] = round(float(((off[1:] - off[:-1]) * (pat >= 0)).sum()) / n, 4)
    r1 = a.segment_device(t.data_ptr(), n)
    info["pieces_one_row"] = r1.count
    r1.free()
    src = [torch.empty(k, dtype=torch.int64, device="cuda:0") for k in (T, T + 1, rows + 1)]
    dst = [torch.empty_like(x) for x in src]
    r.free()
    sink = torch.empty(16, dtype=torch.int64, device="cuda:0")
    pos = torch.arange(n, dtype=torch.int64, device="cuda:0") if args.match_at_all else None

    def find():
        f = a.find_device(t.data_ptr(), n, n_hay=rows, uniform_len=L)
        f.device_ptr  # (waits for the records)
        info["matches"] = f.count
        f.free()

    def seg(batch):
        def f():
            s = a.segment_device(t.data_ptr(), n, n_hay=rows if batch else 0, uniform_len=L if batch else 0)
            s.offsets_ptr()  # (waits for the last kernel)
            s.free()
        return f

    def count_only():
        a.segment_into_device(t.data_ptr(), n, 0, 0, sink.data_ptr(), sink.data_ptr())

    def copy():
        for d, s in zip(dst, src):
            d.copy_(s)
        torch.cuda.synchronize()

    def at_all():
        m = a.match_at_device(t.data_ptr(), n, pos.data_ptr(), n, 0, n_hay=rows, uniform_len=L)
        m.end_ptr()
        m.free()

    v = {"find_a": find, "segment_batch": seg(True), "segment_one": seg(False), "count_only": count_only, "copy": copy}
    if pos is not None:
        v["match_at_all"] = at_all
    v["find_b"] = find
    return v, info


def re_finditer(args, pats, para, t):
    """one core: re.finditer of the alternation (longest first: MaxMatch) on a slice; stopped after --re-seconds"""
    n = min(args.re_mib << 20, t.numel())
    data = (para * ((n + len(para) - 1) // len(para)))[:n]
    rx = re.compile(b"|".join(re.escape(p) for p in sorted(pats, key=len, reverse=True)) + b"|(?s:.)")
    t0, done, pieces = time.perf_counter(), 0, 0
    for m in rx.finditer(data):
        pieces += 1
        done = m.end()
        if not pieces & 0xFFF and time.perf_counter() - t0 > args.re_seconds:
            break
    dt = time.perf_counter() - t0
    return {"slice_bytes": n, "bytes_done": done, "pieces": pieces, "seconds": round(dt, 3),
            "mb_per_s": round(done / dt / 1e6, 3) if dt else None, "finished": done == n}


def part(args, cover, capi, gen, np, torch):
    a, t, pats, para = make_shape(args, cover, capi, gen, np, torch)
    check_against_host(args, capi, np, torch, a, t, pats, para)
    v, info = variants_of(args, capi, torch, a, t)
    ts = paired(v, args.steps, args.warmup, args.settle_ms)
    aa = [abs(x - y) for x, y in zip(ts["find_a"], ts["find_b"])]
    m = {n: round(1e3 * med(x), 4) for n, x in ts.items()}
    res = {"part": "segment", "rows": args.rows, "row_bytes": L, "cover_asked": cover, **info, "steps": args.steps, "ms": m,
           "aa_spread_ms": {"median": round(1e3 * med(aa), 4), "max": round(1e3 * max(aa), 4)},
           "segment_vs_copy": round(m["segment_batch"] / m["copy"], 2) if m["copy"] else None,
           "segment_vs_find": round(m["segment_batch"] / m["find_a"], 2) if m["find_a"] else None,
           "emit_share": round(1 - m["count_only"] / m["segment_one"], 3) if m["segment_one"] else None,
           "re_finditer": re_finditer(args, pats, para, t) if args.re_seconds > 0 else None,
           "checked_against_segment_host": True, "box": platform.node(), "date": time.strftime("%Y-%m-%d")}
    a.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=50.0)
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--cover", type=float, nargs="+", default=[0.5, 0.95])
    ap.add_argument("--no-match-at-all", dest="match_at_all", action="store_false")
    ap.add_argument("--re-mib", type=int, default=64)
    ap.add_argument("--re-seconds", type=float, default=30.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "segment_bench.jsonl"))
    args = ap.parse_args()
    import torch  # first: one process holds one HIP runtime (ahocorasick_rs_amd/__init__.py)
    import numpy as np
    import gen
    from ahocorasick_rs_amd import capi
    if args.steps < 20:
        print("note: medians of fewer than 20 rounds are not what DESIGN.md section 25 asks for", file=sys.stderr)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    rows = []
    for cover in args.cover:
        res = part(args, cover, capi, gen, np, torch)
        line = json.dumps(res)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        rows.append(res)
    print("| covered | pieces T | find (A) | find (A') | A/A spread (median) | segment_batch | as ONE row | count only | copy of its columns | match_at at every byte | re.finditer, one core |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for res in rows:
        m, rx = res["ms"], res["re_finditer"] or {}
        print("| %s | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s MB/s |" % (
            res["covered"], res["pieces"], m["find_a"], m["find_b"], res["aa_spread_ms"]["median"], m["segment_batch"],
            m["segment_one"], m["count_only"], m["copy"], m.get("match_at_all"), rx.get("mb_per_s")))


if __name__ == "__main__":
    main()
