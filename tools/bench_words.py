"""Whole-word benchmark (acx_find_words_device / acx_filter_words_device against the overlapping find beneath them and the
torch form over the columns -- a gather of the neighbour bytes and a mask, the only way before; same box, same session,
interleaved).

  python tools/bench_words.py [--steps K] [--warmup W] [--settle-ms MS] [--rows R] [--every B [B ...]] [--parts words | trace]
                              [--out profiles/r18/words_bench.jsonl]

One JSON line per shape, appended to --out and printed, and the row of DESIGN.md section 22's table for it.  Every figure is
the median wall time per call over K rounds (at least 20); a round runs every variant once, in rotation, so that the
variants see the same clocks (paired, interleaved); the shape starts with the settle phase bench.py uses (untimed calls
for --settle-ms).  Before anything is timed the overlapping form is compared with the torch form, entry by entry.

  shape     cfg2's batch shape in HBM: --rows (131 072) x 8 KiB = 1 GiB as ONE uint8 tensor of filler -- four digits and
            twelve bytes that are no word bytes, drawn evenly, so that about 9 of 16 planted patterns are whole words -- with
            one of eight of cfg2's 10 000 lower-case patterns planted every --every bytes: 256, 64 and 32.
  variants  find_a, find_b     acx_find_device, overlapping, on the uniform batch, waited for, freed -- twice per round: the
                               floor, and their spread is the A/A spread of the session
            words_all          acx_find_words_device, overlapping = 1: the test and one compaction
            words_standard / words_first / words_longest   overlapping = 0 with each kind: the resolve and a second compaction
            filter_words       acx_filter_words_device (LeftmostLongest, keep unmatched)
            torch_form         find_columns_device(overlapping), then the neighbour bytes gathered and masked in torch,
                               synchronised (what overlapping = 1 computes)
  "<variant>_stage_ms" = variant - find_a per round (median): the stage's cost beside the find's.
  trace     no timing: ten rounds of words_all and words_longest, for a kernel trace made in a run of its own, without counters
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
FILLER = b"0123 .,;:-!?()[]"


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
    table = torch.from_numpy(np.frombuffer(FILLER, dtype=np.uint8).copy()).to("cuda:0")
    t = table[torch.randint(0, len(FILLER), (n,), device="cuda:0", generator=g)]
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


def torch_form(args, capi, np, torch, a, t):
    """every whole-word occurrence from the overlapping columns, in torch -> (pattern, start, end, row_offsets)"""
    n, rows = t.numel(), args.rows
    c = a.find_columns_device(t.data_ptr(), n, n_hay=rows, uniform_len=L, overlapping=True)
    k = c.count
    pa, st, en, ro = (words_of(torch, c, w, words) for w, words in ((capi.COL_PATTERN, k), (capi.COL_START, k), (capi.COL_END, k),
                                                                    (capi.COL_ROW_OFFSETS, rows + 1)))
    is_word = torch.zeros(256, dtype=torch.bool, device="cuda:0")
    is_word[torch.from_numpy(np.frombuffer(capi.ASCII_WORD_BYTES, dtype=np.uint8).astype(np.int64)).to("cuda:0")] = True
    row = torch.repeat_interleave(torch.arange(rows, device="cuda:0"), ro[1:] - ro[:-1])
    base = row * L
    left = (st == 0) | ~is_word[t[(base + st - 1).clamp(min=0)].long()]
    right = (en == L) | ~is_word[t[(base + en).clamp(max=n - 1)].long()]
    keep = left & right
    out = pa[keep], st[keep], en[keep], torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda:0"),
                                                   torch.bincount(row[keep], minlength=rows).cumsum(0)])
    torch.cuda.synchronize()
    c.free()
    return out


def variants_of(args, capi, np, torch, a, t):
    n, rows, info = t.numel(), args.rows, {}

    def find():
        r = a.find_device(t.data_ptr(), n, n_hay=rows, uniform_len=L, overlapping=True)
        r.device_ptr  # (waits for the records)
        info["occurrences"] = r.count
        r.free()

    def words(name, overlapping, kind):
        def run():
            c = a.find_words_device(t.data_ptr(), n, n_hay=rows, uniform_len=L, overlapping=overlapping, match_kind=kind)
            c.data_ptr(capi.COL_ROW_OFFSETS)  # (waits for the stage)
            info[name] = c.count
            c.free()
        return run

    def filter_words():
        f = a.filter_words_device(t.data_ptr(), n, n_hay=rows, uniform_len=L, match_kind=capi.MATCH_LEFTMOST_LONGEST)
        f.data_ptr(capi.FILT_DATA)  # (waits for the gather)
        info["kept_rows"] = f.n_rows
        f.free()

    def form():
        out = torch_form(args, capi, np, torch, a, t)
        del out

    return {"find_a": find, "words_all": words("words_all", True, capi.MATCH_STANDARD),
            "words_standard": words("words_standard", False, capi.MATCH_STANDARD),
            "words_first": words("words_first", False, capi.MATCH_LEFTMOST_FIRST), "find_b": find,
            "words_longest": words("words_longest", False, capi.MATCH_LEFTMOST_LONGEST), "filter_words": filter_words,
            "torch_form": form}, info


def check_against_torch(args, capi, np, torch, a, t):
    """the stage's overlapping form and the torch form, entry by entry: no figure of a wrong result is taken"""
    n, rows = t.numel(), args.rows
    c = a.find_words_device(t.data_ptr(), n, n_hay=rows, uniform_len=L, overlapping=True)
    k = c.count
    got = [words_of(torch, c, w, words) for w, words in ((capi.COL_PATTERN, k), (capi.COL_START, k), (capi.COL_END, k),
                                                         (capi.COL_ROW_OFFSETS, rows + 1))]
    want = torch_form(args, capi, np, torch, a, t)
    for name, g, w in zip(("pattern", "start", "end", "row_offsets"), got, want):
        if g.shape != w.shape or not torch.equal(g, w):
            raise SystemExit("the stage's %s differ from the torch form (%d against %d entries)" % (name, len(g), len(w)))
    del got, want
    c.free()


STAGES = ("words_all", "words_standard", "words_first", "words_longest", "filter_words", "torch_form")


def part_words(args, every, capi, gen, np, torch):
    a, t = make_shape(args, every, capi, gen, np, torch)
    check_against_torch(args, capi, np, torch, a, t)
    v, info = variants_of(args, capi, np, torch, a, t)
    ts = paired(v, args.steps, args.warmup, args.settle_ms)
    aa = [abs(x - y) for x, y in zip(ts["find_a"], ts["find_b"])]
    res = {"part": "words", "rows": args.rows, "row_bytes": L, "planted_every": every, "steps": args.steps, **info,
           "ms": {n: round(1e3 * med(x), 4) for n, x in ts.items()},
           "aa_spread_ms": {"median": round(1e3 * med(aa), 4), "max": round(1e3 * max(aa), 4)},
           "checked_against_torch": True, "box": platform.node(), "date": time.strftime("%Y-%m-%d")}
    for name in STAGES:
        res[name + "_stage_ms"] = round(1e3 * med([s - f for s, f in zip(ts[name], ts["find_a"])]), 4)
    a.close()
    return res


def part_trace(args, every, capi, gen, np, torch):
    a, t = make_shape(args, every, capi, gen, np, torch)
    v, _ = variants_of(args, capi, np, torch, a, t)
    for _ in range(10):
        v["words_all"]()
        v["words_longest"]()
    a.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=50.0)
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--every", type=int, nargs="+", default=[256, 64, 32])
    ap.add_argument("--parts", default="words")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "words_bench.jsonl"))
    args = ap.parse_args()
    import torch  # first: one process holds one HIP runtime (ahocorasick_rs_amd/__init__.py)
    import numpy as np
    import gen
    from ahocorasick_rs_amd import capi
    if args.parts == "trace":
        part_trace(args, args.every[0], capi, gen, np, torch)
        return
    if args.steps < 20:
        print("note: medians of fewer than 20 rounds are not what DESIGN.md section 22 asks for", file=sys.stderr)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    rows = []
    for every in args.every:
        res = part_words(args, every, capi, gen, np, torch)
        line = json.dumps(res)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        rows.append(res)
    print("| shape | occurrences | whole words | find (A) | find (A') | A/A spread (median) | all - find | Standard - find | LeftmostFirst - find | "
          "LeftmostLongest - find | filter - find | torch form - find |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for res in rows:
        m = res["ms"]
        print("| %d x %d, a pattern every %d bytes | %s | %s | %s | %s | %s | %s |" % (
            res["rows"], L, res["planted_every"], res.get("occurrences"), res.get("words_all"), m["find_a"], m["find_b"],
            res["aa_spread_ms"]["median"], " | ".join(str(res[n + "_stage_ms"]) for n in STAGES)))


if __name__ == "__main__":
    main()
