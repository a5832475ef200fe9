"""Token-label benchmark (acx_tokens_device against the find beneath it, a device clear of its outputs and the torch form over
the columns -- the only way to get token labels before; same box, same session, interleaved).

  python tools/bench_tokens.py [--steps K] [--warmup W] [--settle-ms MS] [--rows R] [--every B [B ...]] [--parts tokens | trace]
                               [--out profiles/r19/tokens_bench.jsonl]

One JSON line per shape, appended to --out and printed, and the row of DESIGN.md section 23's table for it.  Every figure is
the median wall time per call over K rounds (at least 20); a round runs every variant once, in rotation, so that the
variants see the same clocks (paired, interleaved); the shape starts with the settle phase bench.py uses (untimed calls
for --settle-ms).  Before anything is timed the stage's pattern column is compared with the torch form, entry by entry, and
the begin column with the one derived from the torch form's owners.

  shape     cfg2's batch shape in HBM: --rows (131 072) x 8 KiB = 1 GiB as ONE uint8 tensor of digits (no pattern of cfg2's
            10 000 lower-case ones occurs in them) with one of eight patterns planted every --every bytes: 256 (about 4 M
            records), and the dense end of the curve, 64 and 32.  Tokens: a partition of the whole tensor into tokens of
            seeded lengths 1 .. 8 bytes (mean 4.5; about 240 M tokens), ONE int64 tensor of T + 1 boundaries in HBM.
  variants  find_a, find_b     acx_find_device on the uniform batch, waited for, freed -- twice per round: the floor, and their
                               spread is the A/A spread of the session
            label_tokens       acx_tokens_device, waited for
            clear              the stage's two outputs filled by torch (T int64 words with -1, T bytes with 0), synchronised:
                               what writing the result alone costs
            torch_form         find_columns_device, then searchsorted x 2, repeat_interleave, scatter_reduce(amin) and a gather
                               in torch, synchronised; skipped (null) where its index tensor would pass 2 GiB
  "tokens_ms" = label_tokens - find_a per round (median): the stage's cost, to be read beside find_a and clear.
  trace     no timing: ten rounds of label_tokens, for a kernel trace made in a run of its own, without counters:
              rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_tokens.py --parts trace
            (k_tok_tiles, k_tok_own, k_tok_label, the scan's k_rep_prefix / k_rep_partials; beside the find's own kernels)
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
    # the tokens: seeded lengths 1 .. 8, cut where they pass the tensor's end
    cuts = torch.cumsum(torch.randint(1, 9, (n // 4 + 8,), dtype=torch.int64, device="cuda:0", generator=g), 0)
    keep = int((cuts < n).sum())
    tok = torch.cat([cuts.new_zeros(1), cuts[:keep], cuts.new_full((1,), n)]).contiguous()
    del cuts
    torch.cuda.synchronize()
    return a, t, tok


class DeviceWords:  # words of the C ABI as torch sees them, without a copy
    def __init__(self, ptr, words, typestr="<i8"):
        self.__cuda_array_interface__ = {"shape": (words,), "typestr": typestr, "data": (ptr, False), "version": 2}


def column_of(torch, r, which, words):
    return torch.as_tensor(DeviceWords(r.data_ptr(which), max(words, 1)), device="cuda:0")[:words]


def torch_form(args, capi, torch, a, t, tok, limit=1 << 31):
    """the owners and their patterns from the columns, in torch -> (pattern, owner), or None where the index tensor of the
    repeat_interleave would pass `limit` bytes"""
    n, rows, T = t.numel(), args.rows, tok.numel() - 1
    c = a.find_columns_device(t.data_ptr(), n, n_hay=rows, uniform_len=L)
    k = c.count
    pt, st, en, ro = (column_of(torch, c, w, words) for w, words in ((capi.COL_PATTERN, k), (capi.COL_START, k), (capi.COL_END, k),
                                                                      (capi.COL_ROW_OFFSETS, rows + 1)))
    row = torch.repeat_interleave(torch.arange(rows, device="cuda:0"), ro[1:] - ro[:-1])
    gs, ge = row * L + st, row * L + en
    first = torch.searchsorted(tok[1:], gs, right=True)    # the tokens that end at or before the start
    stop = torch.searchsorted(tok[:-1], ge, right=False)   # the tokens that begin before the end
    cnt = (stop - first).clamp(min=0)
    total = int(cnt.sum())
    if 8 * total > limit:
        c.free()
        return None
    idx = torch.repeat_interleave(torch.arange(k, device="cuda:0"), cnt)
    tokens = first[idx] + torch.arange(total, device="cuda:0") - torch.repeat_interleave(torch.cumsum(cnt, 0) - cnt, cnt)
    owner = torch.full((T,), k, dtype=torch.int64, device="cuda:0").scatter_reduce(0, tokens, idx, "amin")
    pattern = torch.where(owner < k, torch.cat([pt, pt.new_zeros(1)])[owner], -1)
    torch.cuda.synchronize()
    c.free()
    return pattern, owner


def label(a, t, tok, rows):
    T = tok.numel() - 1
    return a.tokens_device(t.data_ptr(), t.numel(), tok.data_ptr(), tok.data_ptr() + 8, T, n_hay=rows, uniform_len=L)


def variants_of(args, capi, torch, a, t, tok, with_torch):
    n, rows, T, info = t.numel(), args.rows, tok.numel() - 1, {}
    out_p = torch.empty(T, dtype=torch.int64, device="cuda:0")
    out_b = torch.empty(T, dtype=torch.uint8, device="cuda:0")

    def find():
        r = a.find_device(t.data_ptr(), n, n_hay=rows, uniform_len=L)
        r.device_ptr  # (waits for the records)
        info["matches"] = r.count
        r.free()

    def label_tokens():
        l = label(a, t, tok, rows)
        l.begin_ptr()  # (waits for the stage)
        l.free()

    def clear():
        out_p.fill_(-1)
        out_b.zero_()
        torch.cuda.synchronize()

    def form():
        out = torch_form(args, capi, torch, a, t, tok)
        del out

    v = {"find_a": find, "label_tokens": label_tokens, "clear": clear, "find_b": find}
    if with_torch:
        v["torch_form"] = form
    return v, info


def check_against_torch(args, capi, torch, a, t, tok):
    """the stage's columns and the torch form, entry by entry: no figure of a wrong result is taken.  False: the torch form
    does not fit and nothing was compared."""
    want = torch_form(args, capi, torch, a, t, tok)
    if want is None:
        return False
    T = tok.numel() - 1
    l = label(a, t, tok, args.rows)
    got_p = torch.as_tensor(DeviceWords(l.pattern_ptr(), T), device="cuda:0")
    got_b = torch.as_tensor(DeviceWords(l.begin_ptr(), T, "|u1"), device="cuda:0")
    pattern, owner = want
    prev = torch.cat([owner.new_full((1,), -1), owner[:-1]])
    begin = ((pattern >= 0) & (owner != prev)).to(torch.uint8)  # (a token without an owner carries the record count)
    if not torch.equal(got_p, pattern):
        raise SystemExit("the stage's pattern column differs from the torch form at token %d" % int((got_p != pattern).nonzero()[0]))
    if not torch.equal(got_b, begin):
        raise SystemExit("the stage's begin column differs from the torch form at token %d" % int((got_b != begin).nonzero()[0]))
    del got_p, got_b, want
    l.free()
    return True


def part_tokens(args, every, capi, gen, np, torch):
    a, t, tok = make_shape(args, every, capi, gen, np, torch)
    checked = check_against_torch(args, capi, torch, a, t, tok)
    v, info = variants_of(args, capi, torch, a, t, tok, checked)
    ts = paired(v, args.steps, args.warmup, args.settle_ms)
    aa = [abs(x - y) for x, y in zip(ts["find_a"], ts["find_b"])]
    m = {n: round(1e3 * med(x), 4) for n, x in ts.items()}
    m.setdefault("torch_form", None)
    stage = 1e3 * med([s - f for s, f in zip(ts["label_tokens"], ts["find_a"])])
    res = {"part": "tokens", "rows": args.rows, "row_bytes": L, "planted_every": every, "matches": info.get("matches"),
           "tokens": tok.numel() - 1, "steps": args.steps, "ms": m,
           "aa_spread_ms": {"median": round(1e3 * med(aa), 4), "max": round(1e3 * max(aa), 4)}, "tokens_ms": round(stage, 4),
           "tokens_vs_find": round(stage / m["find_a"], 3) if m["find_a"] else None,
           "torch_vs_label": round(m["torch_form"] / m["label_tokens"], 2) if m["torch_form"] else None,
           "checked_against_torch": checked, "box": platform.node(), "date": time.strftime("%Y-%m-%d")}
    a.close()
    return res


def part_trace(args, every, capi, gen, np, torch):
    a, t, tok = make_shape(args, every, capi, gen, np, torch)
    v, _ = variants_of(args, capi, torch, a, t, tok, False)
    for _ in range(10):
        v["label_tokens"]()
    a.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=50.0)
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--every", type=int, nargs="+", default=[256, 64, 32])
    ap.add_argument("--parts", default="tokens")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "tokens_bench.jsonl"))
    args = ap.parse_args()
    import torch  # first: one process holds one HIP runtime (ahocorasick_rs_amd/__init__.py)
    import numpy as np
    import gen
    from ahocorasick_rs_amd import capi
    if args.parts == "trace":
        part_trace(args, args.every[0], capi, gen, np, torch)
        return
    if args.steps < 20:
        print("note: medians of fewer than 20 rounds are not what DESIGN.md section 23 asks for", file=sys.stderr)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    rows = []
    for every in args.every:
        res = part_tokens(args, every, capi, gen, np, torch)
        line = json.dumps(res)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        rows.append(res)
    print("| shape | records | tokens | find (A) | find (A') | A/A spread (median) | label_tokens | label_tokens - find | clear of the outputs | torch form |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for res in rows:
        m = res["ms"]
        print("| %d x %d, a pattern every %d bytes | %s | %s | %s | %s | %s | %s | %s | %s | %s |" % (
            res["rows"], L, res["planted_every"], res["matches"], res["tokens"], m["find_a"], m["find_b"], res["aa_spread_ms"]["median"],
            m["label_tokens"], res["tokens_ms"], m["clear"], m["torch_form"] if m["torch_form"] is not None else "skipped"))


if __name__ == "__main__":
    main()
