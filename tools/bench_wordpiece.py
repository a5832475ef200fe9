"""WordPiece benchmark (acx_wordpiece_device on cfg2's batch shape, against the find alone on the same data, the count pass
alone, a device-to-device copy of the input plus the stage's own columns, and a one-core Python WordPiece loop on a slice;
same box, same session, interleaved).

  python tools/bench_wordpiece.py [--steps K] [--warmup W] [--settle-ms MS] [--rows R] [--cover C [C ...]] [--py-mib M]
                                  [--py-seconds S] [--out profiles/r22/wordpiece_bench.jsonl]

One JSON line per coverage, appended to --out and printed, and the row of DESIGN.md section 26's table for it.  Every figure
is the median wall time per call over K rounds (at least 20); a round runs every variant once, in rotation, so that the
variants see the same clocks (paired, interleaved); the shape starts with the settle phase bench.py uses (untimed calls for
--settle-ms).  Before anything is timed the device result of a slice is compared with acx_wordpiece_host, entry by entry.

  shape     cfg2's batch shape in HBM: --rows (131 072) x 8 KiB = 1 GiB as ONE uint8 tensor.  A 4 MiB paragraph -- cfg2's
            10 000 lower-case words, one space between two -- repeated to the size.  The vocabulary (a LeftmostLongest handle)
            holds --cover (0.5, 0.95) of the words: three in four as whole entries, every fourth as a first half and a
            "##" second half.  The share of the words that are known and T are counted from the result ("known", "pieces").
  variants  find_a, find_b     acx_find_device on the uniform batch, waited for, freed -- twice per round: the find alone, and
                               their spread is the A/A spread of the session
            wordpiece_batch    acx_wordpiece_device, uniform rows, waited for: the call
            count_only         acx_wordpiece_into_device with cap = 0: k_wp<COUNT>, the scan and the carry, no emit
            copy               the input's bytes and the stage's own columns moved by torch, device to device: n bytes, three
                               times T words, T bytes and rows + 1 words, synchronised: its traffic floor
  python    once, untimed by the rounds: the WordPiece loop of BERT's tokenizer in plain Python (a dict, longest match first)
            over the first --py-mib (16) MiB, one core; it is stopped after --py-seconds and says how far it got
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
PARAGRAPH = 4 << 20
PREFIX = b"##"
MAX_WORD = 100


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


def words_at(torch, ptr, words, typestr="<i8"):
    return torch.as_tensor(DeviceWords(ptr, max(words, 1), typestr), device="cuda:0")[:words]


def vocabulary(words, cover):
    """`cover` of the words: three in four as whole entries, every fourth as a first half and a continuation"""
    vocab = []
    for k, w in enumerate(words[:int(len(words) * cover)]):
        if k % 4 == 3:
            vocab += [w[:len(w) // 2], PREFIX + w[len(w) // 2:]]
        else:
            vocab.append(w)
    return sorted(set(vocab))


def paragraph(words, np):
    rng = np.random.default_rng(26)
    out, size = [], 0
    while size < PARAGRAPH + 64:
        w = words[int(rng.integers(0, len(words)))]
        out.append(w)
        size += len(w) + 1
    return b" ".join(out)[:PARAGRAPH]


def make_shape(args, cover, capi, gen, np, torch):
    words = gen.gen_patterns(10000, 5, 12, gen.AZ, 1)
    vocab = vocabulary(words, cover)
    a = capi.Automaton(vocab, capi.MATCH_LEFTMOST_LONGEST)
    para = paragraph(words, np)
    n = args.rows * L
    t = torch.from_numpy(np.frombuffer(para, dtype=np.uint8).copy()).to("cuda:0").repeat((n + PARAGRAPH - 1) // PARAGRAPH)[:n].contiguous()
    torch.cuda.synchronize()
    return a, t, vocab, para


def check_against_host(args, capi, np, torch, a, t, vocab, para, cls):
    """the device result of the first paragraph, cut into rows, against acx_wordpiece_host, entry by entry"""
    n = min(PARAGRAPH, t.numel())
    rows = n // L
    r = a.wordpiece_device(t.data_ptr(), n, cls, prefix=PREFIX, max_word=MAX_WORD, n_hay=rows, uniform_len=L)
    h = capi.HostAutomaton(vocab, capi.MATCH_LEFTMOST_LONGEST)
    want = capi.wordpiece_host(h, para[:n], cls, prefix=PREFIX, max_word=MAX_WORD, offsets=np.arange(0, n + 1, L),
                               match_kind=capi.MATCH_LEFTMOST_LONGEST)
    h.close()
    got = (r.id(), r.start(), r.end(), r.first(), r.row_offsets())
    for g, w, name in zip(got, want, ("id", "start", "end", "first", "row_offsets")):
        if not np.array_equal(g, w):
            raise SystemExit("wordpiece_device differs from acx_wordpiece_host in %s" % name)
    r.free()


def variants_of(args, capi, torch, a, t, cls):
    n, rows, info = t.numel(), args.rows, {}
    r = a.wordpiece_device(t.data_ptr(), n, cls, prefix=PREFIX, max_word=MAX_WORD, n_hay=rows, uniform_len=L)
    T = r.count
    ids, first = words_at(torch, r.id_ptr(), T), words_at(torch, r.first_ptr(), T, "|u1")
    n_words = int((first == 1).sum())
    info["pieces"] = T
    info["words"] = n_words
    info["known"] = round(float(((first == 1) & (ids >= 0)).sum()) / max(n_words, 1), 4)
    r.free()
    src = [torch.empty(n, dtype=torch.uint8, device="cuda:0")] + [torch.empty(T, dtype=torch.int64, device="cuda:0") for _ in range(3)] + \
          [torch.empty(T, dtype=torch.uint8, device="cuda:0"), torch.empty(rows + 1, dtype=torch.int64, device="cuda:0")]
    dst = [torch.empty_like(x) for x in src]

    def find():
        f = a.find_device(t.data_ptr(), n, n_hay=rows, uniform_len=L)
        f.device_ptr  # (waits for the records)
        info["matches"] = f.count
        f.free()

    def call():
        s = a.wordpiece_device(t.data_ptr(), n, cls, prefix=PREFIX, max_word=MAX_WORD, n_hay=rows, uniform_len=L)
        s.start_ptr()  # (waits for the last kernel)
        s.free()

    def count_only():
        a.wordpiece_into_device(t.data_ptr(), n, cls, 0, 0, 0, 0, 0, 0, prefix=PREFIX, max_word=MAX_WORD, n_hay=rows, uniform_len=L)

    def copy():
        for d, s in zip(dst, src):
            d.copy_(s)
        torch.cuda.synchronize()

    return {"find_a": find, "wordpiece_batch": call, "count_only": count_only, "copy": copy, "find_b": find}, info


def python_loop(args, vocab, para, t):
    """one core: BERT's WordpieceTokenizer loop over text.split() with a dict, on a slice; stopped after --py-seconds"""
    n = min(args.py_mib << 20, t.numel())
    data = (para * ((n + len(para) - 1) // len(para)))[:n]
    index = {v: i for i, v in enumerate(vocab)}
    t0, done, pieces = time.perf_counter(), 0, 0
    for k, w in enumerate(data.split()):
        done += len(w) + 1
        if len(w) > MAX_WORD:
            pieces += 1
            continue
        p, out = 0, 0
        while p < len(w):
            e = len(w)
            while e > p and ((w[p:e] if p == 0 else PREFIX + w[p:e]) not in index):
                e -= 1
            if e == p:
                out = 1
                break
            out += 1
            p = e
        pieces += out
        if not k & 0xFFF and time.perf_counter() - t0 > args.py_seconds:
            break
    dt = time.perf_counter() - t0
    done = min(done, n)
    return {"slice_bytes": n, "bytes_done": done, "pieces": pieces, "seconds": round(dt, 3),
            "mb_per_s": round(done / dt / 1e6, 3) if dt else None, "finished": done >= n}


def part(args, cover, capi, gen, np, torch):
    cls = capi.wp_classes()
    a, t, vocab, para = make_shape(args, cover, capi, gen, np, torch)
    check_against_host(args, capi, np, torch, a, t, vocab, para, cls)
    v, info = variants_of(args, capi, torch, a, t, cls)
    ts = paired(v, args.steps, args.warmup, args.settle_ms)
    aa = [abs(x - y) for x, y in zip(ts["find_a"], ts["find_b"])]
    m = {n: round(1e3 * med(x), 4) for n, x in ts.items()}
    res = {"part": "wordpiece", "rows": args.rows, "row_bytes": L, "cover_asked": cover, "vocabulary": len(vocab), **info,
           "steps": args.steps, "ms": m, "aa_spread_ms": {"median": round(1e3 * med(aa), 4), "max": round(1e3 * max(aa), 4)},
           "call_vs_copy": round(m["wordpiece_batch"] / m["copy"], 2) if m["copy"] else None,
           "call_vs_find": round(m["wordpiece_batch"] / m["find_a"], 2) if m["find_a"] else None,
           "emit_share": round(1 - m["count_only"] / m["wordpiece_batch"], 3) if m["wordpiece_batch"] else None,
           "python_loop": python_loop(args, vocab, para, t) if args.py_seconds > 0 else None,
           "checked_against_wordpiece_host": True, "box": platform.node(), "date": time.strftime("%Y-%m-%d")}
    a.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=50.0)
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--cover", type=float, nargs="+", default=[0.5, 0.95])
    ap.add_argument("--py-mib", type=int, default=16)
    ap.add_argument("--py-seconds", type=float, default=20.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22", "wordpiece_bench.jsonl"))
    args = ap.parse_args()
    import torch  # first: one process holds one HIP runtime (ahocorasick_rs_amd/__init__.py)
    import numpy as np
    import gen
    from ahocorasick_rs_amd import capi
    if args.steps < 20:
        print("note: medians of fewer than 20 rounds are not what DESIGN.md section 26 asks for", file=sys.stderr)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    rows = []
    for cover in args.cover:
        res = part(args, cover, capi, gen, np, torch)
        line = json.dumps(res)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        rows.append(res)
    print("| words known | pieces T | find (A) | find (A') | A/A spread (median) | wordpiece_batch | count only | copy of input and columns | call / copy | call / find | Python loop, one core |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for res in rows:
        m, py = res["ms"], res["python_loop"] or {}
        print("| %s | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s MB/s |" % (
            res["known"], res["pieces"], m["find_a"], m["find_b"], res["aa_spread_ms"]["median"], m["wordpiece_batch"],
            m["count_only"], m["copy"], res["call_vs_copy"], res["call_vs_find"], py.get("mb_per_s")))


if __name__ == "__main__":
    main()
