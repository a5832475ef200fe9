#!/usr/bin/env python3
"""Randomised parity run on a GPU box: HIP path (C ABI) vs the oracle on random pattern sets
(alphabets from 2 letters to all bytes to UTF-8 with 2/3/4-byte characters, 1 .. 30 000
patterns, duplicates, nested patterns) and haystacks of 0 .. 48 MiB (text-like, uniform, dense,
planted), all match kinds, overlapping, byte offsets and code points, both scan kernels.
usage: gpu_fuzz.py [seconds] [seed]   -- prints one line per case, exits non-zero on a mismatch.
       gpu_fuzz.py surface [n] [seed] [--plan-only]   -- the whole call surface (plan_surface / run_surface below): batches,
       find_device, replace*, the case-insensitive build flag, device pointer residues; --plan-only prints the coverage
       table of the plan with the oracle alone (no GPU).
       gpu_fuzz.py summary [n] [seed] [--plan-only]   -- the summaries (plan_summary / run_summary below): acx_summarize on the
       host and the device route, batches, acx_summarize_device in its three forms at odd and even pointer residues, both
       build flags, every match kind, overlapping counts, code points; each against the oracle's matches reduced in Python.
       gpu_fuzz.py walk [n] [seed] [--plan-only]   -- the anchored walkers (plan_walk / run_walk below): match_at, segment and
       wordpiece through every way in (host input, one haystack, a uniform and a ragged cut in HBM, row starts, the raw
       *_into_device forms), every match kind, both build flags, forced kernels, compressed-only handles, pointer residues;
       each against reference_walk -- the oracle's overlapping rows and numpy -- and so is the host form over the same inputs.
tests/test_gpu_fuzz.py runs a bounded, seeded slice of it (fuzz(budget, seed, max_size_log2)) under -m gpu,
tests/test_gpu_fuzz_surface.py a fixed number of surface cases; tests/test_fuzz_plan_cpu.py checks what that plan covers;
tests/test_gpu_summary.py a slice of the summary cases, tests/test_summary_cpu.py what their plan covers;
tests/test_gpu_fuzz_walk.py runs the walk plan, tests/test_fuzz_walk_plan_cpu.py checks its reference and what it covers.
UTF-8 cases only ever hold patterns made of whole characters (a str pattern cannot end inside one:
the precondition of codepoints = 1, include/acx.h)."""
import os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
import numpy as np
import gen
from oracle_lib import KIND_DFA, Oracle, byte_to_code_point
try:  # (the plan of the surface cases needs the oracle alone)
    from ahocorasick_rs_amd import capi
except ImportError:
    capi = None

rng = random.Random(20260927)
MAX_SIZE_LOG2 = 25.5
ALPHAS = [("ab", b"ab"), ("abc", b"abc"), ("a-h", b"abcdefgh"), ("a-z", gen.AZ), ("a-z+sp", gen.AZ + b" "),
          ("bytes", bytes(range(256))), ("utf8", None)]
UNI = "abcdefghijklmnopqrstuvwxyz" + "é☃\U0001F926"


def cols(a):
    return np.stack([a["pattern"], a["start"], a["end"]], 1) if len(a) else np.zeros((0, 3), np.uint64)


def make_case(max_pat_log10: float = 4.5):
    name, alpha = ALPHAS[rng.randrange(len(ALPHAS))]
    n_pat = int(10 ** rng.uniform(0, max_pat_log10))
    lo = rng.choice([1, 2, 3, 5, 5, 5, 8])
    hi = lo + rng.choice([0, 3, 7, 20, 60])
    if alpha is None:
        pats = ["".join(rng.choice(UNI) for _ in range(rng.randint(lo, hi))).encode() for _ in range(n_pat)]
    else:
        pats = [bytes(rng.choice(alpha) for _ in range(rng.randint(lo, hi))) for _ in range(n_pat)]
    if rng.random() < 0.3 and n_pat > 3:  # duplicates and nested patterns
        pats += [pats[rng.randrange(n_pat)] for _ in range(n_pat // 10 + 1)]
        if alpha is None:  # (prefixes of whole characters: a str pattern cannot end inside one)
            pats += [pats[rng.randrange(n_pat)].decode()[:rng.randint(1, 4)].encode() for _ in range(n_pat // 10 + 1)]
        else:
            pats += [pats[rng.randrange(n_pat)][:rng.randint(1, 6)] for _ in range(n_pat // 10 + 1)]
    size = int(2 ** rng.uniform(0, MAX_SIZE_LOG2)) if rng.random() < 0.9 else rng.choice([0, 1, 4095, 4096, 4097, 262144, 262145])
    if alpha is not None and len(alpha) <= 8:  # small alphabets: the output is many times the input -- keep it bounded
        size = min(size, (1 << 18) if lo <= 2 else (1 << 21))
    kind = rng.choice(["uniform", "text", "planted", "dense"])
    if alpha is None:
        chars = [rng.choice(UNI) if rng.random() < 0.3 else rng.choice("abcdefgh ") for _ in range(min(size, 200000))]
        base = "".join(chars).encode()
        hay = (base * (size // max(len(base), 1) + 1))[:size]
        while hay and (hay[-1] & 0xC0) == 0x80 or (hay and hay[-1] >= 0xC0):
            hay = hay[:-1]  # cut at a character boundary
        hay = bytearray(hay)
    else:
        a = np.frombuffer(alpha, dtype=np.uint8)
        hay = bytearray(a[np.random.default_rng(rng.randrange(1 << 30)).integers(0, len(a), size)].tobytes())
    if kind in ("planted", "dense") and size > 64:
        step = rng.choice([37, 300, 5000]) if kind == "planted" else rng.choice([3, 9, 17])
        p = 0
        while p < size - 70 and (kind == "planted" or p < 400000):
            x = pats[rng.randrange(len(pats))]
            if alpha is not None and p + len(x) <= size:
                hay[p:p + len(x)] = x
            p += step + rng.randrange(step)
    return name, kind, pats, bytes(hay)



def fuzz(budget: float, seed: int, max_size_log2: float = 25.5, save_failures: bool = True):
    """-> (cases, failures); deterministic in (seed, max_size_log2) up to where the time budget cuts it.  A pattern set the
    library refuses to build counts as a failure."""
    global rng, MAX_SIZE_LOG2
    rng = random.Random(seed)
    MAX_SIZE_LOG2 = max_size_log2
    t_end = time.time() + budget
    cases = fails = 0
    while time.time() < t_end:
        name, kind, pats, hay = make_case()
        mk = rng.randrange(3)
        kernel = rng.choice([None, capi.KERNEL_DFA_WALK, capi.KERNEL_PREFILTER])
        ov = mk == 0 and rng.random() < 0.4
        cp = name == "utf8" and rng.random() < 0.7
        if os.environ.get("FUZZ_ONLY") and os.environ["FUZZ_ONLY"] != name:
            continue
        # hundreds of copies of every pattern on text where every position matches (seed 40404, case 23: 22 264 patterns over
        # {a, b} of 1-4 bytes = 30 distinct strings, 256 KiB of a/b).  The device reports one occurrence per STRING and the
        # copies are expanded where the result is complete ("copies of a pattern"; tests/test_gpu_copies.py),
        # so such a case costs its OUTPUT only -- which for an overlapping search is the occurrences x the copies: skipped
        # when that is beyond the 2 * 10^7 rows the rule below allows (decided here, before the oracle builds them; the rng
        # stream is not disturbed)
        copies = len(pats) / max(len(set(pats)), 1)
        if ov and copies > 50 and len(hay) * copies > 2e7:
            print(f"skip {name:7s} {kind:8s} pats {len(pats):6d} hay {len(hay):9d}: overlapping, {copies:.0f} copies of every pattern", flush=True)
            continue
        try:
            a = capi.Automaton(pats, mk, kernel=kernel)
        except (capi.AcxError, ValueError, MemoryError) as e:
            print("build error", name, kind, len(pats), mk, kernel, e, flush=True)
            fails += 1; continue
        o = Oracle(pats, mk, KIND_DFA)
        want = o.find_raw(hay, overlapping=ov)
        if cp and len(want):
            b2c = byte_to_code_point(hay)
            want = np.stack([want[:, 0], b2c[want[:, 1].astype(np.int64)], b2c[want[:, 2].astype(np.int64)]], 1)
        if len(want) > 20_000_000:
            a.close(); continue
        try:
            got = cols(a.find(hay, overlapping=ov, codepoints=cp))
        except (capi.AcxError, ValueError, MemoryError) as e:
            print("find error", name, kind, len(pats), len(hay), mk, ov, cp, kernel, len(want), e, flush=True)
            fails += 1; a.close(); continue
        ok = np.array_equal(got, want)
        # the same bytes at an unaligned device address, and again (buffers of the previous call in flight)
        got2 = cols(a.find(np.frombuffer(b"x" * 3 + hay, dtype=np.uint8)[3:], overlapping=ov, codepoints=cp))
        ok = ok and np.array_equal(got2, want)
        cases += 1
        if not ok:
            for tag, g in (("aligned", got), ("unaligned", got2)):
                if np.array_equal(g, want):
                    continue
                m = min(len(g), len(want))
                d = np.nonzero((g[:m] != want[:m]).any(1))[0]
                i = int(d[0]) if len(d) else m
                print(f"  {tag}: got {len(g)} want {len(want)} rows, first difference at row {i}: got "
                      f"{g[i].tolist() if i < len(g) else None} want {want[i].tolist() if i < len(want) else None}", flush=True)
        print(f"{'ok  ' if ok else 'FAIL'} {name:7s} {kind:8s} pats {len(pats):6d} hay {len(hay):9d} mk {mk} ov {int(ov)} cp {int(cp)} "
              f"kernel {kernel} matches {len(want)}", flush=True)
        if not ok:
            fails += 1
            if save_failures:
                np.save(f"/root/repo/gpurun_out/fuzz_fail_{cases}_hay.npy", np.frombuffer(hay, dtype=np.uint8))
                open(f"/root/repo/gpurun_out/fuzz_fail_{cases}_pats.txt", "w").write(repr((pats, mk, ov, cp, kernel)))
        a.close()
    return cases, fails


# ---------------------------------------------------------------------------
# the rest of the call surface: a PLAN of cases (no GPU), and its run
# ---------------------------------------------------------------------------
OPS = ("find", "find_batch", "find_device_one", "find_device_uniform", "find_device_ragged", "replace_host", "replace_device_route",
       "replace_batch", "replace_device_one", "replace_device_uniform", "replace_device_ragged")
BATCH_OPS = ("find_batch", "find_device_ragged", "replace_batch", "replace_device_ragged")
REPL_LENS = (0, 1, 4, 7, 20, 64, 5000)
ROW_LIMIT = 20_000_000            # what fuzz() allows a case
SURFACE_ROWS, SURFACE_OUT_BYTES = 1_000_000, 48 << 20  # what a surface case is cut down to: it stays in the low seconds
SURFACE_SIZE_LOG2, SURFACE_PAT_LOG10 = 20.0, 3.3
FOLD = bytes.maketrans(bytes(range(65, 91)), bytes(range(97, 123)))


def _upper_some(b: bytes, seed: int) -> bytes:
    """about half of the ASCII lower-case letters upper-cased, by a seeded mask"""
    a = np.frombuffer(b, dtype=np.uint8).copy()
    sel = ((gen.stream_np(seed, len(a)) & np.uint64(1)) == 1) & (a >= 97) & (a <= 122)
    a[sel] -= 32
    return a.tobytes()


def _char_start(hay: bytes, p: int) -> int:
    while 0 < p < len(hay) and (hay[p] & 0xC0) == 0x80:
        p -= 1
    return p


def _splice(hay: bytes, rows, repl) -> bytes:
    out, at = [], 0
    for p, s, e in rows.tolist():
        out.append(hay[at:s]); out.append(repl[p]); at = e
    out.append(hay[at:])
    return b"".join(out)


def reference(c: dict) -> dict:
    """what the case must give, from the oracle alone (over folded inputs for a case-insensitive handle) and a plain splice:
    rows (all haystacks' matches behind one another), counts per haystack, outs (the replaced haystacks) for a replace op"""
    fold = (lambda b: b.translate(FOLD)) if c["ci"] else (lambda b: b)
    o = Oracle([fold(p) for p in c["pats"]], c["mk"], KIND_DFA)
    rows, counts, outs = [], [], []
    for h in c["hays"]:
        w = o.find_raw(fold(h), overlapping=c["ov"])
        if c["repl"] is not None:
            outs.append(_splice(h, w, c["repl"]))
        if c["cp"] and len(w):
            b2c = byte_to_code_point(h)
            w = np.stack([w[:, 0], b2c[w[:, 1].astype(np.int64)], b2c[w[:, 2].astype(np.int64)]], 1)
        rows.append(w.reshape(-1, 3).astype(np.uint64)); counts.append(len(w))
    return {"rows": np.concatenate(rows) if rows else np.zeros((0, 3), np.uint64), "counts": counts, "outs": outs}


def _cut(hay: bytes, utf8: bool, op: str):
    """the haystacks of the case: the whole of it, pieces of one length, or ragged pieces with empty ones among them"""
    if op.endswith("_uniform"):
        L = min(rng.choice([1, 7, 64, 1000, 4096, 8192]), max(len(hay), 1))
        n = len(hay) // L
        return [hay[i * L:(i + 1) * L] for i in range(n)], L
    if op not in BATCH_OPS:
        return [hay], 0
    cuts = sorted(rng.randrange(len(hay) + 1) for _ in range(rng.randint(0, 12)))
    if utf8:
        cuts = sorted(_char_start(hay, p) for p in cuts)
    if rng.random() < 0.6:  # empty haystacks: in front, at the end, twice in a row inside
        cuts += [rng.choice([0, len(hay)] + cuts) for _ in range(rng.randint(1, 3))]
    cuts = [0] + sorted(cuts) + [len(hay)]
    return [hay[cuts[i]:cuts[i + 1]] for i in range(len(cuts) - 1)], 0


def plan_surface(n_cases: int, seed: int):
    """-> n_cases cases (dicts) over the whole call surface; deterministic in (n_cases, seed); no GPU and no capi.Automaton.
    Pattern sets and haystacks: make_case()'s shapes with smaller caps.  The op, the match kind and the build flag are dealt
    from a deck, not drawn one by one: every block of len(OPS) cases holds every op once (in a drawn order), and an op's
    (kind, flag) pair moves to the next of the six with every block -- so 8 blocks hold every op 8 times, with either flag at
    least 3 times and with every kind.  Everything else is drawn.  A case whose reference would have more than SURFACE_ROWS
    rows or SURFACE_OUT_BYTES of output has its haystack halved (its 5000-byte replacements shortened first) until it has
    not: no case ever needs to be skipped."""
    global rng, MAX_SIZE_LOG2
    saved = (rng, MAX_SIZE_LOG2)
    rng, MAX_SIZE_LOG2 = random.Random(seed), SURFACE_SIZE_LOG2
    cases = []
    try:
        order = []
        while len(cases) < n_cases:
            i = len(cases)
            if i % len(OPS) == 0:
                order = list(range(len(OPS)))
                rng.shuffle(order)
            j = order[i % len(OPS)]
            deal = (i // len(OPS) + j) % 6
            op, mk, ci = OPS[j], deal % 3, deal >= 3
            name, kind, pats, hay = make_case(SURFACE_PAT_LOG10)
            utf8, is_find = name == "utf8", op.startswith("find")
            c = {"i": i, "op": op, "name": name, "kind": kind, "mk": mk, "ci": ci,
                 "kernel": rng.choice([None, 1, 2]),  # (capi.KERNEL_DFA_WALK, capi.KERNEL_PREFILTER)
                 "ov": is_find and mk == 0 and rng.random() < 0.4,
                 "cp": is_find and utf8 and not op.endswith("_uniform") and rng.random() < 0.7,
                 "off": rng.randrange(16), "route": rng.choice(["host", "device"]) if op == "replace_batch" else None}
            if ci:
                pats = [_upper_some(p, rng.randrange(1 << 30)) for p in pats]
                hay = _upper_some(hay, rng.randrange(1 << 30))
            c["pats"] = pats
            repl = None
            if not is_find:
                pool = np.random.default_rng(rng.randrange(1 << 30)).integers(0, 256, 8192, dtype=np.uint8).tobytes()
                repl = []
                for _ in pats:
                    L, at = rng.choice(REPL_LENS), rng.randrange(3000)
                    repl.append(pool[at:at + L])
            c["repl"] = repl
            cut_state = rng.getstate()  # (the same cuts, in proportion, when the haystack has to shrink)
            while True:
                rng.setstate(cut_state)
                c["hays"], c["uniform_len"] = _cut(hay, utf8, op)
                ref = reference(c)
                out_bytes = sum(len(x) for x in ref["outs"])
                if len(ref["rows"]) <= SURFACE_ROWS and out_bytes <= SURFACE_OUT_BYTES:
                    break
                if out_bytes > SURFACE_OUT_BYTES and any(len(r) > 64 for r in repl):
                    c["repl"] = repl = [r[:64] for r in repl]
                    continue
                hay = hay[:_char_start(hay, len(hay) // 2)] if utf8 else hay[:len(hay) // 2]
            c["rows"], c["out_bytes"] = len(ref["rows"]), out_bytes
            c["zero_used"] = bool(repl is not None and len(ref["rows"]) and
                                  any(len(repl[p]) == 0 for p in np.unique(ref["rows"][:, 0]).tolist()))
            cases.append(c)
    finally:
        rng, MAX_SIZE_LOG2 = saved
    return cases


def plan_digest(cases) -> str:
    import hashlib
    h = hashlib.sha256()
    for c in cases:
        h.update(repr([(k, c[k]) for k in sorted(c) if k not in ("pats", "hays", "repl")]).encode())
        for part in (c["pats"], c["hays"], c["repl"] or []):
            h.update(repr([len(x) for x in part]).encode())
            h.update(b"".join(part))
    return h.hexdigest()


def coverage_table(cases) -> str:
    lines = [f"{len(cases)} cases; most rows {max(c['rows'] for c in cases)} (limit {ROW_LIMIT}), most output bytes "
             f"{max(c['out_bytes'] for c in cases)}",
             f"{'op':24s} {'n':>3s}  ci=0 ci=1   mk0 mk1 mk2   ov  cp  empty-hay  zero-repl-used"]
    for op in OPS:
        cs = [c for c in cases if c["op"] == op]
        lines.append(f"{op:24s} {len(cs):3d}  {sum(not c['ci'] for c in cs):4d} {sum(c['ci'] for c in cs):4d}   "
                     + " ".join(f"{sum(c['mk'] == k for c in cs):3d}" for k in range(3))
                     + f"  {sum(c['ov'] for c in cs):3d} {sum(c['cp'] for c in cs):3d}  {sum(any(len(h) == 0 for h in c['hays']) for c in cs):9d}"
                     + f"  {sum(c['zero_used'] for c in cs):14d}")
    for c in cases:
        lines.append(f"  case {c['i']:3d} {c['op']:24s} {c['name']:7s} {c['kind']:8s} pats {len(c['pats']):5d} hays {len(c['hays']):5d} "
                     f"bytes {sum(len(h) for h in c['hays']):8d} rows {c['rows']:8d} out {c['out_bytes']:9d}")
    return "\n".join(lines)


def _on_device(data: bytes, off: int):
    buf = capi.DeviceBuffer(off + len(data) + 16)
    buf.upload(np.frombuffer(bytes(off) + data, dtype=np.uint8))
    return buf


def _run_case(a, c: dict, ref: dict):
    """-> None, or the first difference as text"""
    hays, off, L = c["hays"], c["off"], c["uniform_len"]
    whole = b"".join(hays)
    bounds = np.cumsum([0] + [len(h) for h in hays]).astype(np.uint64)
    op, kw = c["op"], {"overlapping": c["ov"], "codepoints": c["cp"]}
    bufs, counts, outs, rows = [], None, None, None
    try:
        if op.endswith(("_one", "_uniform", "_ragged")):
            bufs.append(_on_device(whole, off))
            seg = {}
            if op.endswith("_uniform"):
                seg = {"n_hay": len(hays), "uniform_len": L}
            elif op.endswith("_ragged"):
                bufs.append(capi.DeviceBuffer(bounds.nbytes).upload(bounds.view(np.uint8)))
                seg = {"n_hay": len(hays), "d_offsets": bufs[1].ptr}
            if op.startswith("find"):
                r = a.find_device(bufs[0].ptr + off, len(whole), **seg, **kw)
                rows = cols(r.matches())
                counts = [int(v) for v in r.counts()] if seg else None
                r.free()
            else:
                r = a.replace_device(bufs[0].ptr + off, len(whole), c["repl"], **seg)
                got, ob = r.download(), [int(v) for v in r.offsets()][:len(hays) + 1]
                r.free()
                if len(ob) != len(hays) + 1 or ob[0] != 0 or ob[-1] != len(got) or any(ob[k] > ob[k + 1] for k in range(len(hays))):
                    return f"offsets() {ob[:8]}... do not delimit {len(hays)} outputs of {len(got)} bytes"
                outs = [got[ob[k]:ob[k + 1]] for k in range(len(hays))]
            if not np.array_equal(bufs[0].download(off + len(whole)), np.frombuffer(bytes(off) + whole, dtype=np.uint8)):
                return "the caller's device buffer was written"
        elif op == "find":
            rows = cols(a.find(np.frombuffer(b"x" * off + whole, dtype=np.uint8)[off:], **kw))
        elif op == "find_batch":
            m, cnt = a.find_batch(hays, **kw)
            rows, counts = cols(m), [int(v) for v in cnt]
        else:
            os.environ["ACX_REPLACE_HOST_MAX"] = "0" if (op == "replace_device_route" or c["route"] == "device") else str(1 << 40)
            try:
                outs = a.replace_batch(hays, c["repl"]) if op == "replace_batch" else [a.replace(whole, c["repl"])]
            finally:
                del os.environ["ACX_REPLACE_HOST_MAX"]
    finally:
        for b in bufs:
            b.free()
    if outs is not None:
        if len(outs) != len(ref["outs"]):
            return f"{len(outs)} outputs for {len(hays)} haystacks"
        for k, (g, w) in enumerate(zip(outs, ref["outs"])):
            if g != w:
                n = min(len(g), len(w))
                d = np.nonzero(np.frombuffer(g[:n], dtype=np.uint8) != np.frombuffer(w[:n], dtype=np.uint8))[0]
                i = int(d[0]) if len(d) else n
                return f"haystack {k} ({len(hays[k])} bytes): got {len(g)} want {len(w)} bytes, first difference at byte {i}: got {g[i:i + 8]!r} want {w[i:i + 8]!r}"
        return None
    want = ref["rows"]
    if counts is not None and counts != ref["counts"]:
        k = next(i for i in range(len(counts)) if counts[i] != ref["counts"][i])
        return f"haystack {k} ({len(hays[k])} bytes): {counts[k]} matches, the reference has {ref['counts'][k]}"
    if not np.array_equal(rows, want):
        n = min(len(rows), len(want))
        d = np.nonzero((rows[:n] != want[:n]).any(1))[0]
        i = int(d[0]) if len(d) else n
        k = int(np.searchsorted(np.cumsum(ref["counts"]), i, side="right"))
        return (f"got {len(rows)} want {len(want)} rows, first difference at row {i} (haystack {k}): got "
                f"{rows[i].tolist() if i < len(rows) else None} want {want[i].tolist() if i < len(want) else None}")
    return None


def run_surface(cases):
    """-> (ran, failures, skipped, build_errors): every case through the C ABI against reference(case); one line per case,
    the first difference of a case that fails.  A pattern set that does not build is a failure."""
    ran = fails = skipped = build_errors = 0
    for c in cases:
        tag = (f"{c['i']:3d} {c['op']:22s} {c['name']:7s} {c['kind']:8s} pats {len(c['pats']):5d} hays {len(c['hays']):5d} bytes "
               f"{sum(len(h) for h in c['hays']):8d} mk {c['mk']} ci {int(c['ci'])} ov {int(c['ov'])} cp {int(c['cp'])} off {c['off']:2d} "
               f"kernel {c['kernel']} rows {c['rows']}")
        if c["rows"] > ROW_LIMIT:
            print("skip", tag, flush=True)
            skipped += 1
            continue
        try:
            a = capi.Automaton(c["pats"], c["mk"], kernel=c["kernel"], ascii_case_insensitive=c["ci"])
        except (capi.AcxError, ValueError, MemoryError) as e:
            print("FAIL", tag, "build error:", e, flush=True)
            build_errors += 1; fails += 1
            continue
        t0 = time.time()
        try:
            diff = _run_case(a, c, reference(c))
        except (capi.AcxError, ValueError, MemoryError) as e:
            diff = f"error: {e}"
        a.close()
        ran += 1
        print(f"{'FAIL' if diff else 'ok  '} {tag} {time.time() - t0:.2f} s", flush=True)
        if diff:
            print("    ", diff, flush=True)
            fails += 1
    return ran, fails, skipped, build_errors


SURFACE_N, SURFACE_SEED = 176, 20261016  # what tests/test_gpu_fuzz_surface.py runs and tests/test_fuzz_plan_cpu.py checks


# ---------------------------------------------------------------------------
# the summaries (acx_summarize*): a plan of their own, reduced from the same reference
# ---------------------------------------------------------------------------
SUMMARY_OPS = ("summarize_host", "summarize_device_route", "summarize_batch", "summarize_device_one", "summarize_device_uniform",
               "summarize_device_ragged")
_SUMMARY_SHAPE = {"summarize_host": "find", "summarize_device_route": "find", "summarize_batch": "find_batch",  # (_cut's names)
                  "summarize_device_one": "find_device_one", "summarize_device_uniform": "find_device_uniform",
                  "summarize_device_ragged": "find_device_ragged"}
SUMMARY_WHATS = (3, 3, 1, 2, 0)  # ACX_SUM_FIRST | ACX_SUM_BY_PATTERN


def plan_summary(n_cases: int, seed: int):
    """-> n_cases cases over the summary entry points; deterministic in (n_cases, seed); no GPU and no capi.Automaton.  Built as
    plan_surface builds its cases -- make_case()'s shapes with the surface's caps, the op, the match kind and the build flag
    dealt from a deck (every block of len(SUMMARY_OPS) cases holds every op once, an op's (kind, flag) pair moves on with every
    block), a haystack halved until its reference has at most SURFACE_ROWS rows -- with make_case()'s generator borrowed and
    put back.  The pointer residue of a device case alternates between odd and even with the blocks."""
    global rng, MAX_SIZE_LOG2
    saved = (rng, MAX_SIZE_LOG2)
    rng, MAX_SIZE_LOG2 = random.Random(seed), SURFACE_SIZE_LOG2
    cases = []
    try:
        order = []
        while len(cases) < n_cases:
            i, k = len(cases), len(SUMMARY_OPS)
            if i % k == 0:
                order = list(range(k))
                rng.shuffle(order)
            j = order[i % k]
            deal = (i // k + j) % 6
            op, mk, ci = SUMMARY_OPS[j], deal % 3, deal >= 3
            name, kind, pats, hay = make_case(SURFACE_PAT_LOG10)
            utf8 = name == "utf8"
            c = {"i": i, "op": op, "name": name, "kind": kind, "mk": mk, "ci": ci, "kernel": rng.choice([None, 1, 2]),
                 "ov": mk == 0 and rng.random() < 0.4,
                 "cp": utf8 and not op.endswith("_uniform") and rng.random() < 0.7,
                 "off": 2 * rng.randrange(8) + (i // k + j) % 2,
                 "route": rng.choice(["host", "device"]) if op == "summarize_batch" else None,
                 "what": rng.choice(SUMMARY_WHATS), "repl": None}
            if ci:
                pats = [_upper_some(p, rng.randrange(1 << 30)) for p in pats]
                hay = _upper_some(hay, rng.randrange(1 << 30))
            c["pats"] = pats
            cut_state = rng.getstate()
            while True:
                rng.setstate(cut_state)
                c["hays"], c["uniform_len"] = _cut(hay, utf8, _SUMMARY_SHAPE[op])
                ref = reference(c)
                if len(ref["rows"]) <= SURFACE_ROWS:
                    break
                hay = hay[:_char_start(hay, len(hay) // 2)] if utf8 else hay[:len(hay) // 2]
            c["rows"], c["out_bytes"], c["zero_used"] = len(ref["rows"]), 0, False
            cases.append(c)
    finally:
        rng, MAX_SIZE_LOG2 = saved
    return cases


def summary_coverage_table(cases) -> str:
    lines = [f"{len(cases)} cases; most rows {max(c['rows'] for c in cases)} (limit {ROW_LIMIT})",
             f"{'op':26s} {'n':>3s}  ci=0 ci=1   mk0 mk1 mk2   ov  cp  odd even  empty-hay  what 0/1/2/3"]
    for op in SUMMARY_OPS:
        cs = [c for c in cases if c["op"] == op]
        lines.append(f"{op:26s} {len(cs):3d}  {sum(not c['ci'] for c in cs):4d} {sum(c['ci'] for c in cs):4d}   "
                     + " ".join(f"{sum(c['mk'] == k for c in cs):3d}" for k in range(3))
                     + f"  {sum(c['ov'] for c in cs):3d} {sum(c['cp'] for c in cs):3d}  {sum(c['off'] % 2 for c in cs):3d} "
                     + f"{sum(1 - c['off'] % 2 for c in cs):4d}  {sum(any(len(h) == 0 for h in c['hays']) for c in cs):9d}  "
                     + "/".join(str(sum(c['what'] == w for c in cs)) for w in range(4)))
    for c in cases:
        lines.append(f"  case {c['i']:3d} {c['op']:26s} {c['name']:7s} {c['kind']:8s} pats {len(c['pats']):5d} hays {len(c['hays']):5d} "
                     f"bytes {sum(len(h) for h in c['hays']):8d} rows {c['rows']:8d}")
    return "\n".join(lines)


def reduce_reference(ref: dict, n_patterns: int) -> dict:
    """the summaries of reference(case), reduced here: any / first per haystack (None: no match), the per-pattern totals"""
    rows, counts = ref["rows"], ref["counts"]
    at = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return {"total": len(rows), "counts": counts, "any": [n > 0 for n in counts],
            "first": [tuple(int(v) for v in rows[at[h]]) if counts[h] else None for h in range(len(counts))],
            "hist": np.bincount(rows[:, 0].astype(np.int64), minlength=n_patterns).astype(np.uint64)}


def _run_summary_case(a, c: dict, ref: dict):
    """-> None, or the first difference as text"""
    hays, off, L, what = c["hays"], c["off"], c["uniform_len"], c["what"]
    whole = b"".join(hays)
    bounds = np.cumsum([0] + [len(h) for h in hays]).astype(np.uint64)
    op, kw = c["op"], {"overlapping": c["ov"], "codepoints": c["cp"]}
    want = reduce_reference(ref, len(c["pats"]))
    bufs, s = [], None
    try:
        if op.startswith("summarize_device_") and op != "summarize_device_route":
            bufs.append(_on_device(whole, off))
            seg = {}
            if op.endswith("_uniform"):
                seg = {"n_hay": len(hays), "uniform_len": L}
            elif op.endswith("_ragged"):
                bufs.append(capi.DeviceBuffer(bounds.nbytes).upload(bounds.view(np.uint8)))
                seg = {"n_hay": len(hays), "d_offsets": bufs[1].ptr}
            s = a.summarize_device(bufs[0].ptr + off, len(whole), what, **seg, **kw)
            device = True
        else:
            to_device = op == "summarize_device_route" or c["route"] == "device"
            before = os.environ.get("ACX_SUMMARY_HOST_MAX")
            os.environ["ACX_SUMMARY_HOST_MAX"] = "0" if to_device else str(1 << 40)
            try:
                if op == "summarize_batch":
                    s = a.summarize_batch(hays, what, **kw)
                else:
                    s = a.summarize(np.frombuffer(b"x" * off + whole, dtype=np.uint8)[off:], what, **kw)
            finally:  # (the caller's own setting comes back)
                if before is None:
                    del os.environ["ACX_SUMMARY_HOST_MAX"]
                else:
                    os.environ["ACX_SUMMARY_HOST_MAX"] = before
            device = to_device and len(whole) > 0  # (nothing is beyond a limit of 0 bytes but a non-empty input)
        if s.on_device != device:
            return f"on_device is {s.on_device}, the call should have been reduced {'in HBM' if device else 'on the host'}"
        if s.total != want["total"]:
            return f"total {s.total}, the reference has {want['total']} matches"
        counts = [int(v) for v in s.counts()]
        if counts != want["counts"]:
            k = next((i for i in range(min(len(counts), len(want["counts"]))) if counts[i] != want["counts"][i]), -1)
            return f"{len(counts)} counts for {len(want['counts'])} haystacks; haystack {k}: {counts[k]} matches, the reference has {want['counts'][k]}"
        for part, bit in (("any", 1), ("first", 1), ("by_pattern", 2)):
            if not what & bit:
                try:
                    getattr(s, part)()
                except ValueError:
                    continue
                return f"{part}() of a summary made with what = {what} did not fail"
        if what & 1:
            got_any = [bool(v) for v in s.any()]
            if got_any != want["any"]:
                k = next(i for i in range(len(got_any)) if got_any[i] != want["any"][i])
                return f"any[{k}] is {got_any[k]}, haystack {k} ({len(hays[k])} bytes) has {want['counts'][k]} matches"
            f = s.first()
            got_first = [None if int(r["pattern"]) == capi.NO_MATCH else (int(r["pattern"]), int(r["start"]), int(r["end"])) for r in f]
            if got_first != want["first"]:
                k = next(i for i in range(len(got_first)) if got_first[i] != want["first"][i])
                return f"first[{k}] is {got_first[k]}, the reference has {want['first'][k]}"
        if what & 2:
            h = s.by_pattern()
            if not np.array_equal(h, want["hist"]):
                p = int(np.nonzero(h != want["hist"])[0][0]) if len(h) == len(want["hist"]) else -1
                return f"by_pattern[{p}] is {int(h[p])}, the reference has {int(want['hist'][p])} ({len(h)} entries for {len(want['hist'])} patterns)"
        if bufs and not np.array_equal(bufs[0].download(off + len(whole)), np.frombuffer(bytes(off) + whole, dtype=np.uint8)):
            return "the caller's device buffer was written"
    finally:
        if s is not None:
            s.free()
        for b in bufs:
            b.free()
    return None


def run_summary(cases):
    """-> (ran, failures, skipped, build_errors), as run_surface: every case through the C ABI against the reduced reference"""
    ran = fails = skipped = build_errors = 0
    for c in cases:
        tag = (f"{c['i']:3d} {c['op']:24s} {c['name']:7s} {c['kind']:8s} pats {len(c['pats']):5d} hays {len(c['hays']):5d} bytes "
               f"{sum(len(h) for h in c['hays']):8d} mk {c['mk']} ci {int(c['ci'])} ov {int(c['ov'])} cp {int(c['cp'])} off {c['off']:2d} "
               f"what {c['what']} kernel {c['kernel']} rows {c['rows']}")
        if c["rows"] > ROW_LIMIT:
            print("skip", tag, flush=True)
            skipped += 1
            continue
        try:
            a = capi.Automaton(c["pats"], c["mk"], kernel=c["kernel"], ascii_case_insensitive=c["ci"])
        except (capi.AcxError, ValueError, MemoryError) as e:
            print("FAIL", tag, "build error:", e, flush=True)
            build_errors += 1; fails += 1
            continue
        t0 = time.time()
        try:
            diff = _run_summary_case(a, c, reference(c))
        except (capi.AcxError, ValueError, MemoryError) as e:
            diff = f"error: {e}"
        a.close()
        ran += 1
        print(f"{'FAIL' if diff else 'ok  '} {tag} {time.time() - t0:.2f} s", flush=True)
        if diff:
            print("    ", diff, flush=True)
            fails += 1
    return ran, fails, skipped, build_errors


SUMMARY_N, SUMMARY_SEED = 72, 20261017  # what tests/test_gpu_summary.py runs a slice of and tests/test_summary_cpu.py checks


# ---------------------------------------------------------------------------
# the anchored walkers (match_at, segment, wordpiece): a plan of their own, and a reference from the oracle's overlapping rows
# ---------------------------------------------------------------------------
WALK_OPS = ("match_at_host", "match_at_device_one", "match_at_device_uniform", "match_at_device_ragged", "match_at_rows_uniform",
            "match_at_rows_ragged", "segment_host", "segment_device_one", "segment_device_uniform", "segment_device_ragged",
            "wordpiece_host", "wordpiece_device_one", "wordpiece_device_uniform", "wordpiece_device_ragged")
WALK_SIZE_LOG2 = SURFACE_SIZE_LOG2  # the data of a walk case: at most 2^20 bytes
WALK_MAX_WORDS = (1, 7, 100, 1024)  # (the last one is WP_MAX_WORD, wp.hpp)
WP_WORD, WP_SPACE, WP_ALONE = 0, 1, 2
WALK_COLUMNS = {"match_at": ("pattern", "end", "row_offsets"), "segment": ("pattern", "offsets", "row_offsets"),
                "wordpiece": ("id", "start", "end", "first", "row_offsets")}


def walk_feature(op: str) -> str:
    return "match_at" if op.startswith("match_at") else op.split("_")[0]


def _walk_shape(op: str, host_rows: bool) -> str:
    """_cut()'s name for the rows of the case"""
    if op.endswith("_host"):
        return "find_batch" if host_rows else "find"
    return "find_device_" + op.rsplit("_", 1)[1]


class _Cands:
    """candidates (pattern, start, end) of every start at once, ordered by (start, end, pattern); lo[p] .. lo[p + 1]: those of p"""

    def __init__(self, pid, s, e, n):
        o = np.lexsort((pid, e, s))
        self.pid, self.s, self.e, self.n = pid[o], s[o], e[o], n
        self.lo = np.searchsorted(self.s, np.arange(n + 2))

    def keep(self, mask):
        return _Cands(self.pid[mask], self.s[mask], self.e[mask], self.n)

    def pick(self, kind):
        """the candidate the kind keeps of every start -> (pattern, end) over 0 .. n, -1 where there is none: one lexsort and
        the first of every group of one start"""
        pid, s, e = self.pid, self.s, self.e
        o = np.lexsort({0: (pid, e, s), 1: (pid, s), 2: (pid, -e, s), "lowest": (pid, s)}[kind])
        first = np.ones(len(o), dtype=bool)
        first[1:] = s[o][1:] != s[o][:-1]
        o = o[first]
        bp, be = np.full(self.n + 1, -1, np.int64), np.full(self.n + 1, -1, np.int64)
        bp[s[o]], be[s[o]] = pid[o], e[o]
        return bp, be

    def stepper(self, kind):
        """-> step(p, limit): the candidate of start p among those that end at or before limit, or None -- for the chains,
        whose limit (a word's end) differs from start to start; plain lists and one bisection per step"""
        from bisect import bisect_right
        lo, E, PID, m = self.lo.tolist(), self.e.tolist(), self.pid.tolist(), len(self.pid)
        at = None
        if kind == 2 and m:  # the largest end: the first of the last (start, end) group
            new = np.ones(m, dtype=bool)
            new[1:] = (self.s[1:] != self.s[:-1]) | (self.e[1:] != self.e[:-1])
            at = np.maximum.accumulate(np.where(new, np.arange(m), 0)).tolist()
        elif kind == 1 and m:  # the smallest pattern so far within the start: a running minimum that starts again per start
            new = np.ones(m, dtype=bool)
            new[1:] = self.s[1:] != self.s[:-1]
            down = (int(new.sum()) - np.cumsum(new)) * (int(self.pid.max()) + 1)  # (later starts lie lower: no minimum carries over)
            at = (np.minimum.accumulate((self.pid + down) * (m + 1) + np.arange(m)) % (m + 1)).tolist()

        def step(p, limit):
            a, b = lo[p], lo[p + 1]
            if a == b or E[a] > limit:
                return None
            k = a if at is None else at[bisect_right(E, limit, a, b) - 1]
            return PID[k], E[k]
        return step


def _walk_ctx(c: dict, limit: int = SURFACE_ROWS):
    """the data of the case, its row bounds and the candidate sets C(p, L) of at.hpp's definition -- or None when the oracle
    would give more than `limit` rows"""
    fold = (lambda b: b.translate(FOLD)) if c["ci"] else (lambda b: b)
    whole = b"".join(c["hays"])
    n = len(whole)
    bounds = np.cumsum([0] + [len(h) for h in c["hays"]]).astype(np.int64)
    data, rows = fold(whole), 0

    def cands(pats, index=None):
        nonlocal rows
        if not pats or rows > limit:
            return _Cands(*(np.zeros(0, np.int64),) * 3, n)
        o = Oracle([fold(p) for p in pats], 0, KIND_DFA)
        rows += o.count(data, overlapping=True)
        if rows > limit:
            return _Cands(*(np.zeros(0, np.int64),) * 3, n)
        w = o.find_raw(data, overlapping=True).astype(np.int64).reshape(-1, 3)
        pid, s, e = w[:, 0], w[:, 1], w[:, 2]
        if index is not None:
            pid = np.asarray(index, dtype=np.int64)[pid]
        keep = e <= bounds[np.searchsorted(bounds, s, side="right")]  # (the row of s is the LAST one that begins at or before it)
        return _Cands(pid[keep], s[keep], e[keep], n)

    ctx = {"whole": whole, "n": n, "bounds": bounds, "all": cands(c["pats"])}
    if walk_feature(c["op"]) == "wordpiece":
        C = fold(c["prefix"])
        index = [i for i, p in enumerate(c["pats"]) if fold(p).startswith(C) and len(p) > len(C)]
        ctx["cont"] = cands([c["pats"][i][len(C):] for i in index], index)
    ctx["rows"] = rows
    return None if rows > limit else ctx


def _utf8_units(raw, limit):
    """seg.hpp's unknown unit of every position, from the raw bytes: the length the lead byte announces, shortened to the
    continuation bytes that follow inside the row (limit: the row end of every position)"""
    n = len(raw)
    want = np.where((raw >= 0xC0) & (raw <= 0xDF), 2, np.where((raw >= 0xE0) & (raw <= 0xEF), 3, np.where((raw >= 0xF0) & (raw <= 0xF7), 4, 1)))
    cont = np.concatenate([(raw >= 0x80) & (raw <= 0xBF), np.zeros(4, dtype=bool)])
    p = np.arange(n)
    u, run = np.ones(n, np.int64), np.ones(n, dtype=bool)
    for k in (1, 2, 3):
        run = run & cont[p + k] & (p + k < limit) & (want > k)
        u += run
    return u


def reference_walk(c: dict, positions="own", ctx=None) -> dict:
    """What a walk case must give -- the columns of WALK_COLUMNS[feature] -- without capi and without a GPU.

    The candidate sets C(p, L) of at.hpp come from ONE Standard oracle over the (folded) patterns: its overlapping rows over
    the (folded) data, grouped by start, and restricted to those that end inside the row of their start.  The overlapping
    search reports, at a match state, EVERY pattern of the state's list in index order (ac_oracle.c, aco_find_overlapping_iter;
    add_match appends at the tail) -- so of identical patterns each one has a row of its own, with its own index, (start, end)
    equal.  Nothing needs to be added for them: the overlapping form lists them all by (end, index), and the picks order by
    index last, so the lowest index of identical patterns wins.
      match_at   the pick of the kind per start (a lexsort and the first of each start's group), read at the anchors; a
                 position outside the data, or an empty row, has none; FULL keeps end == L first.  Row starts: end is a length.
      segment    the same pick per start gives every position its step -- the match length, or seg.hpp's unknown unit from the
                 RAW bytes -- and the chain is a plain loop, one step per piece.
      wordpiece  the words from cls as wp.hpp states them (vectorised); at a word's start the candidates of the whole
                 vocabulary, behind it those of a second oracle over the entries that begin with C and are longer, C stripped,
                 mapped back to their index (an empty C: every entry), both restricted to the word's end; a word longer than M
                 or with a step without a candidate is ONE unknown piece.
    positions: the case's own, or another array (the host form refuses those outside the data)."""
    ctx = ctx or _walk_ctx(c, 1 << 62)
    n, bounds, cd, feature = ctx["n"], ctx["bounds"], ctx["all"], walk_feature(c["op"])
    if feature == "match_at":
        pos = c["positions"] if isinstance(positions, str) else positions
        if pos is None:  # the rows are the anchors
            p, L = bounds[:-1], bounds[1:]
            valid, local = L > p, p
        else:
            pos = np.asarray(pos, dtype=np.int64)
            valid = (pos >= 0) & (pos < n)
            p = np.where(valid, pos, n)
            local = 0
        if c["full"]:
            cd = cd.keep(cd.e == bounds[np.searchsorted(bounds, cd.s, side="right")])
        if not c["ov"]:
            bp, be = cd.pick("lowest" if c["full"] else c["mk"])
            pat = np.where(valid, bp[p], -1)
            return {"pattern": pat, "end": np.where(pat >= 0, be[p] - local, -1)}
        k = np.where(valid, cd.lo[p + 1] - cd.lo[p], 0)
        ro = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
        at = np.repeat(cd.lo[p], k) + np.arange(ro[-1]) - np.repeat(ro[:-1], k)
        return {"pattern": cd.pid[at], "end": cd.e[at] - (np.repeat(local, k) if pos is None else 0), "row_offsets": ro}
    raw = np.frombuffer(ctx["whole"], dtype=np.uint8)
    if feature == "segment":
        bp, be = cd.pick(c["mk"])
        at = np.arange(n)
        limit = bounds[np.searchsorted(bounds, at, side="right")] if n else at
        unit = _utf8_units(raw, limit) if c["utf8"] else np.ones(n, np.int64)
        step = np.where(bp[:n] >= 0, be[:n] - at, unit).tolist()
        starts, p = [], 0
        while p < n:
            starts.append(p)
            p += step[p]
        starts = np.asarray(starts, dtype=np.int64).reshape(-1)
        return {"pattern": bp[starts], "offsets": np.concatenate([starts, [n]]).astype(np.int64),
                "row_offsets": np.searchsorted(starts, bounds, side="left").astype(np.int64)}
    cls, M, unk = np.asarray(c["cls"], dtype=np.uint8), c["max_word"], c["unk_id"]
    k = cls[raw]
    row_start = np.zeros(n + 1, dtype=bool)
    row_start[bounds] = True
    row_start = row_start[:n]
    start = (k != WP_SPACE) & (row_start | (k == WP_ALONE) | ~np.concatenate([[False], k[:-1] == WP_WORD]))
    nextb = np.concatenate([np.minimum.accumulate(np.where((k != WP_WORD) | row_start, np.arange(n), n)[::-1])[::-1], [n]])
    ws = np.flatnonzero(start)
    we = np.where(k[ws] == WP_ALONE, ws + 1, nextb[ws + 1])
    first_step, next_step = cd.stepper(c["mk"]), ctx["cont"].stepper(c["mk"])
    out = []
    for a, b in zip(ws.tolist(), we.tolist()):
        pieces, p = [], a
        if b - a <= M:
            r = first_step(a, b)
            while r is not None:
                pieces.append((r[0], p, r[1], int(p == a)))
                p = r[1]
                if p == b:
                    break
                r = next_step(p, b)
        out += pieces if p == b else [(unk, a, b, 1)]
    col = lambda j, t: np.asarray([x[j] for x in out], dtype=t).reshape(-1)
    ref = {"id": col(0, np.int64), "start": col(1, np.int64), "end": col(2, np.int64), "first": col(3, np.uint8)}
    ref["row_offsets"] = np.searchsorted(ref["start"], bounds, side="left").astype(np.int64)
    return ref


def _wp_vocabulary(pats, alpha: bytes, utf8: bool):
    """-> (the vocabulary, C, whether C is an entry): make_case()'s patterns with the drawn prefix in front of a drawn half"""
    how = rng.choice(["##", "", "@", "own", "none"])
    if how == "own":
        C = rng.choice(["é", "☃", "a☃"]).encode() if utf8 else bytes(rng.choice(alpha) for _ in range(2))
    elif how == "none":
        C = next(x for x in (b"\x01\x02", b"~^", b"\x7f\x00\x7f", b"\x02\x01\x7f\x01") if not any(p.translate(FOLD).startswith(x) for p in pats))
    else:
        C = how.encode()
    vocab = [C + p if how != "none" and rng.random() < 0.5 else p for p in pats]
    own = bool(C) and how != "none" and rng.random() < 0.35
    if own:
        vocab.append(C)
    return vocab, C, own


def _wp_classes(alpha: bytes):
    """one or two byte values of the alphabet are SPACE beside 32 and 10, one or two ALONE (a comma where the alphabet is too small)"""
    values = sorted(set(alpha) - {32, 10})
    special = rng.sample(values, min(rng.randint(2, 4), len(values) // 4 * 2))
    cls = np.zeros(256, dtype=np.uint8)
    cls[[32, 10] + special[:len(special) // 2]] = WP_SPACE
    cls[special[len(special) // 2:] or [44]] = WP_ALONE
    return cls


def _wp_text(hay: bytes, vocab, C: bytes, own: bool, cls, M: int) -> bytes:
    """separators written into the haystack at drawn distances -- mostly 1 to 12 bytes, now and then more than M (the stretch
    cleared of separators), now and then two in a row -- and words made of entries behind some of them"""
    a = np.frombuffer(hay, dtype=np.uint8).copy()
    n = len(a)
    seps = [int(b) for b in np.flatnonzero(cls != WP_WORD)]
    spaces = [int(b) for b in np.flatnonzero(cls == WP_SPACE)]
    word_byte = next(b for b in list(hay[:64]) + list(range(97, 123)) if cls[b] == WP_WORD)
    cont = [x[len(C):] for x in vocab if x.startswith(C) and len(x) > len(C)]
    p = 0
    while p < n:
        r = rng.random()
        gap = rng.randint(1, 12) if r < 0.93 else 0 if r < 0.985 else M + rng.randint(1, 40)
        if gap > M:
            part = a[p:p + gap]
            part[cls[part] != WP_WORD] = word_byte
        elif gap and rng.random() < 0.4:
            word = C if own and rng.random() < 0.2 else rng.choice(vocab)
            for _ in range(rng.choice([0, 0, 1, 2, 3]) if cont else 0):
                word = word + rng.choice(cont)
            word = np.frombuffer(word, dtype=np.uint8)[:n - p]
            a[p:p + len(word)] = word
            gap = len(word)
        p += gap
        if p < n:
            a[p] = rng.choice(spaces if rng.random() < 0.8 else seps)
            p += 1
    return a.tobytes()


def plan_walk(n_cases: int, seed: int, size_log2: float = WALK_SIZE_LOG2, pat_log10: float = SURFACE_PAT_LOG10):
    """-> n_cases cases over the three anchored walkers, every way in (WALK_OPS); deterministic in (n_cases, seed); no GPU and
    no capi.Automaton.  Built as plan_summary builds its cases -- make_case()'s shapes with the surface's caps (the data at most
    2^WALK_SIZE_LOG2 bytes), the op, the match kind and the build flag dealt from a deck, the generator borrowed and put back, a
    haystack halved until the oracle gives at most SURFACE_ROWS overlapping rows over it.  One device op of every block calls
    the raw *_into_device form, one op of every block runs on a handle kept in compressed form only.  A pattern set over all
    byte values also gets an entry per first byte: a root with 256 children.  size_log2, pat_log10: smaller caps, for the
    cross-check of the reference against the per-pattern brute forces (tests/test_fuzz_walk_plan_cpu.py)."""
    global rng, MAX_SIZE_LOG2
    saved = (rng, MAX_SIZE_LOG2)
    rng, MAX_SIZE_LOG2 = random.Random(seed), size_log2
    cases, k = [], len(WALK_OPS)
    try:
        order, raw_j, compressed_j = [], 0, 0
        while len(cases) < n_cases:
            i = len(cases)
            if i % k == 0:
                order = list(range(k))
                rng.shuffle(order)
                raw_j = rng.choice([j for j in range(k) if not WALK_OPS[j].endswith("_host")])
                compressed_j = rng.randrange(k)
            j = order[i % k]
            deal = (i // k + j) % 6
            op, mk, ci = WALK_OPS[j], deal % 3, deal >= 3
            feature = walk_feature(op)
            name, kind, pats, hay = make_case(pat_log10)
            utf8 = name == "utf8"
            alpha = dict(ALPHAS)[name] or UNI.encode()
            c = {"i": i, "op": op, "name": name, "kind": kind, "mk": mk, "ci": ci, "kernel": rng.choice([None, 1, 2]),
                 "off": rng.randrange(16), "raw": j == raw_j, "compressed": j == compressed_j,
                 "shape": _walk_shape(op, rng.random() < 0.6)}
            fan = [bytes([b]) + bytes(rng.choice(alpha) for _ in range(rng.randint(0, 3))) for b in range(256)] if name == "bytes" else []
            if feature != "wordpiece":
                pats = pats + fan
            if ci:
                pats = [_upper_some(p, rng.randrange(1 << 30)) for p in pats]
                hay = _upper_some(hay, rng.randrange(1 << 30))
            if feature == "match_at":
                c["row_starts"] = "_rows_" in op or (c["shape"] == "find_batch" and rng.random() < 0.3)
                c["ov"] = mk == 0 and not c["raw"] and rng.random() < 0.5
                c["full"] = c["row_starts"] and rng.random() < 0.5
            elif feature == "segment":
                c["utf8"] = rng.random() < (0.7 if utf8 else 0.5 if name == "bytes" else 0.2)
            else:
                pats, c["prefix"], c["prefix_is_entry"] = _wp_vocabulary(pats, alpha, utf8)
                pats = pats + fan  # (behind the prefixes: the root keeps all 256)
                c["max_word"], c["unk_id"] = rng.choice(WALK_MAX_WORDS), rng.choice([-1, -1, 0, 1 << 40])
                c["cls"] = _wp_classes(alpha)
                hay = _wp_text(hay, pats, c["prefix"], c["prefix_is_entry"], c["cls"], c["max_word"])
            c["pats"] = pats
            cut_state = rng.getstate()
            while True:
                rng.setstate(cut_state)
                c["hays"], c["uniform_len"] = _cut(hay, utf8, c["shape"])
                if feature == "match_at" and c["full"]:  # rows that ARE a pattern, and one that is a byte longer
                    if c["uniform_len"]:
                        fits = [p for p in pats if len(p) == c["uniform_len"]]
                        for r in range(0, len(c["hays"]), 5):
                            if fits:
                                c["hays"][r] = rng.choice(fits)
                    else:
                        for x in [rng.choice(pats) for _ in range(3)] + [rng.choice(pats) + rng.choice(pats)[:1]]:
                            c["hays"].insert(rng.randrange(len(c["hays"]) + 1), x)
                ctx = _walk_ctx(c)
                if ctx is not None:
                    break
                hay = hay[:_char_start(hay, len(hay) // 2)] if utf8 else hay[:len(hay) // 2]
            c["rows"] = ctx["rows"]
            if feature == "match_at":
                c["positions"] = None if c["row_starts"] else _walk_positions(c, ctx)
            c["pieces"] = len(next(iter(reference_walk(c, ctx=ctx).values())))
            cases.append(c)
    finally:
        rng, MAX_SIZE_LOG2 = saved
    return cases


def _walk_positions(c: dict, ctx: dict):
    """about one anchor per 4 to 64 bytes, unsorted and with repeats, half of them where candidates begin; the last byte of
    rows, the start of empty rows, len -- and for device inputs a few beyond len and negative"""
    n, bounds = ctx["n"], ctx["bounds"]
    g = np.random.default_rng(rng.randrange(1 << 30))
    count = int(n / 2 ** rng.uniform(2, 6)) + rng.randint(0, 3)
    pos = g.integers(0, max(n, 1), size=count)
    begins, many = np.unique(ctx["all"].s), np.flatnonzero(np.diff(ctx["all"].lo) >= 2)
    if len(begins):
        pos[:count // 2] = g.choice(begins, size=count // 2)
    if len(many):  # (... a part of them where several do)
        pos[:count // 6 + 1] = g.choice(many, size=count // 6 + 1)
    pos[count - count // 8:] = pos[:count // 8]
    lens = np.diff(bounds)
    ends, empty = bounds[1:][lens > 0] - 1, bounds[:-1][lens == 0]
    extra = [g.choice(x, size=min(k, len(x))) if len(x) else [] for x, k in ((ends, 8), (empty, 4))] + [[n, n]]
    if not c["op"].endswith("_host"):
        extra.append([n + 1, n + 5, -1, -(1 << 62), 1 << 62, -n - 1])
    pos = np.concatenate([pos] + [np.asarray(x, dtype=np.int64) for x in extra]).astype(np.int64)
    return pos[g.permutation(len(pos))]


def walk_digest(cases) -> str:
    import hashlib
    h = hashlib.sha256()
    for c in cases:
        h.update(repr([(k, c[k] if not isinstance(c[k], np.ndarray) else c[k].tolist()) for k in sorted(c) if k not in ("pats", "hays")]).encode())
        for part in (c["pats"], c["hays"]):
            h.update(repr([len(x) for x in part]).encode())
            h.update(b"".join(part))
    return h.hexdigest()


def walk_coverage_table(cases) -> str:
    lines = [f"{len(cases)} cases; most oracle rows {max(c['rows'] for c in cases)} (limit {SURFACE_ROWS}), most data bytes "
             f"{max(sum(len(h) for h in c['hays']) for c in cases)}",
             f"{'op':26s} {'n':>3s}  ci=0 ci=1   mk0 mk1 mk2  odd even  empty-row  raw compressed"]
    for op in WALK_OPS:
        cs = [c for c in cases if c["op"] == op]
        lines.append(f"{op:26s} {len(cs):3d}  {sum(not c['ci'] for c in cs):4d} {sum(c['ci'] for c in cs):4d}   "
                     + " ".join(f"{sum(c['mk'] == k for c in cs):3d}" for k in range(3))
                     + f"  {sum(c['off'] % 2 for c in cs):3d} {sum(1 - c['off'] % 2 for c in cs):4d}  "
                     + f"{sum(any(len(h) == 0 for h in c['hays']) for c in cs):9d}  {sum(c['raw'] for c in cs):3d} {sum(c['compressed'] for c in cs):10d}")
    for c in cases:
        lines.append(f"  case {c['i']:3d} {_walk_tag(c)}")
    return "\n".join(lines)


def _walk_tag(c: dict) -> str:
    what = {"match_at": lambda: f"ov {int(c['ov'])} full {int(c['full'])} anchors {len(c['hays']) if c['positions'] is None else len(c['positions'])}",
            "segment": lambda: f"utf8 {int(c['utf8'])}",
            "wordpiece": lambda: f"C {c['prefix']!r}{'*' if c['prefix_is_entry'] else ''} M {c['max_word']}"}[walk_feature(c["op"])]()
    return (f"{c['op']:24s} {c['name']:7s} {c['kind']:8s} pats {len(c['pats']):5d} hays {len(c['hays']):6d} bytes "
            f"{sum(len(h) for h in c['hays']):7d} mk {c['mk']} ci {int(c['ci'])} off {c['off']:2d} kernel {c['kernel']} "
            f"{'raw ' if c['raw'] else ''}{'compressed ' if c['compressed'] else ''}{what} rows {c['rows']} out {c['pieces']}")


def walk_difference(feature: str, got: dict, want: dict):
    """-> None, or the first difference as text: feature, column, index, got and want"""
    for name in WALK_COLUMNS[feature]:
        g, w = got.get(name), want.get(name)
        if g is None and w is None:
            continue
        if g is None or w is None:
            return f"{feature} {name}: {'missing' if g is None else 'present'}, the reference has {'none' if w is None else len(w)}"
        g, w = np.asarray(g), np.asarray(w)
        m = min(len(g), len(w))
        bad = np.flatnonzero(g[:m].astype(np.int64) != w[:m].astype(np.int64))
        if len(bad) or len(g) != len(w):
            i = int(bad[0]) if len(bad) else m
            return (f"{feature} {name}[{i}]: got {int(g[i]) if i < len(g) else None} want {int(w[i]) if i < len(w) else None} "
                    f"({len(g)} entries, the reference has {len(w)})")
    return None


def walk_host_form(c: dict, ctx: dict, ref: dict):
    """the host form (acx_match_at_host / acx_segment_host / acx_wordpiece_host: the definition walked over the compiled
    tables, no device) over the same inputs -> None, or its first difference from the reference"""
    feature, whole = walk_feature(c["op"]), ctx["whole"]
    offsets = None if c["shape"] == "find" or c["shape"].endswith("_one") else ctx["bounds"]
    h = capi.HostAutomaton(c["pats"], c["mk"], capi.BUILD_ASCII_CASE_INSENSITIVE if c["ci"] else 0)
    try:
        if feature == "match_at":
            pos = c["positions"]
            if pos is not None:  # (it refuses a position outside the data)
                pos = pos[(pos >= 0) & (pos <= len(whole))]
                ref = reference_walk(c, pos, ctx)
            flags = (capi.AT_OVERLAPPING if c["ov"] else 0) | (capi.AT_FULL if c["full"] else 0) | (capi.AT_ROW_STARTS if pos is None else 0)
            got = capi.match_at_host(h, whole, pos, offsets=offsets, flags=flags, match_kind=c["mk"])
        elif feature == "segment":
            got = capi.segment_host(h, whole, offsets=offsets, flags=capi.SEG_UTF8 if c["utf8"] else 0, match_kind=c["mk"])
        else:
            got = capi.wordpiece_host(h, whole, c["cls"], prefix=c["prefix"], max_word=c["max_word"], unk_id=c["unk_id"],
                                      offsets=offsets, match_kind=c["mk"])
    finally:
        h.close()
    return walk_difference(feature, dict(zip(WALK_COLUMNS[feature], got)), ref)


def _run_walk_case(a, c: dict, ctx: dict, ref: dict):
    """-> None, or the first difference as text"""
    feature, whole, bounds, off, L = walk_feature(c["op"]), ctx["whole"], ctx["bounds"], c["off"], c["uniform_len"]
    names, rows = WALK_COLUMNS[feature], len(c["hays"])
    ragged = c["shape"] in BATCH_OPS
    if feature == "match_at":
        pos = c["positions"]
        flags = (capi.AT_OVERLAPPING if c["ov"] else 0) | (capi.AT_FULL if c["full"] else 0) | (capi.AT_ROW_STARTS if pos is None else 0)
    elif feature == "segment":
        flags = capi.SEG_UTF8 if c["utf8"] else 0
    else:
        kw = {"prefix": c["prefix"], "max_word": c["max_word"], "unk_id": c["unk_id"]}
    if c["op"].endswith("_host"):  # host input: a sequence of rows, or one haystack that is no batch
        hay = (c["hays"], None) if c["shape"] == "find_batch" else (None, whole)
        if feature == "match_at":
            r = a.match_at(hay[0], pos, flags, single=hay[1])
        elif feature == "segment":
            r = a.segment(hay[0], flags, single=hay[1])
        else:
            r = a.wordpiece(hay[0], c["cls"], single=hay[1], **kw)
        try:
            if r.on_device:
                return "a host input gave a result on the device"
            return walk_difference(feature, {name: getattr(r, name)() for name in names}, ref)
        finally:
            r.free()
    if c["raw"]:  # the *_into_device form, its outputs between guard bytes (the feature's own test file has the frame)
        cut = {"offsets": bounds if ragged else None, "uniform": L}
        if feature == "match_at":
            from test_gpu_at import run_raw
            got = run_raw(a, whole, pos, flags=flags & capi.AT_FULL, base_res=off, out_res=off & 1, **cut)
            return walk_difference(feature, dict(zip(names, got)), ref)
        T = len(ref[names[0]])
        if feature == "segment":
            from test_gpu_seg import run_raw
            got_T, out = run_raw(a, whole, T, flags=flags, base_res=off, **cut)
            if got_T != T:
                return f"segment: {got_T} pieces, the reference has {T}"
            return walk_difference(feature, dict(zip(names, [o.view(np.int64) for o in out])), ref)
        from test_gpu_wp import GUARD, run_raw
        got_T, got, sizes = run_raw(a, whole, c["cls"], max(T, 1), prefix=c["prefix"], M=c["max_word"], unk=c["unk_id"], base_res=off, **cut)
        if got_T != T:
            return f"wordpiece: {got_T} pieces, the reference has {T}"
        out = {}
        for g, size, name in zip(got, sizes, names):
            used = ref[name].nbytes
            if not ((g[:64] == GUARD).all() and (g[64 + used:] == GUARD).all()):
                return f"wordpiece {name}: a byte around its {used} bytes was written"
            out[name] = g[64:64 + used].copy().view(ref[name].dtype)
        return walk_difference(feature, out, ref)
    bufs, r = [], None
    try:
        bufs.append(_on_device(whole, off))
        seg = {}
        if L:
            seg = {"n_hay": rows, "uniform_len": L}
        elif ragged:
            bufs.append(capi.DeviceBuffer(bounds.nbytes).upload(bounds.astype(np.uint64).view(np.uint8)))
            seg = {"n_hay": rows, "d_offsets": bufs[-1].ptr}
        if feature == "match_at":
            d_pos, n_pos = 0, 0
            if pos is not None:
                bufs.append(capi.DeviceBuffer(8 * len(pos) + 16))
                if len(pos):
                    bufs[-1].upload(pos.view(np.uint8))
                d_pos, n_pos, at_pos = bufs[-1].ptr, len(pos), bufs[-1]
            r = a.match_at_device(bufs[0].ptr + off, len(whole), d_pos, n_pos, flags, **seg)
        elif feature == "segment":
            r = a.segment_device(bufs[0].ptr + off, len(whole), flags, **seg)
        else:
            r = a.wordpiece_device(bufs[0].ptr + off, len(whole), c["cls"], **seg, **kw)
        if not r.on_device:
            return "a device input gave a result on the host"
        got = {name: getattr(r, name)() for name in names}
        if not np.array_equal(bufs[0].download(off + len(whole)), np.frombuffer(bytes(off) + whole, dtype=np.uint8)):
            return "the caller's device buffer was written"
        if ragged and not L and not np.array_equal(bufs[1].download(bounds.nbytes).view(np.uint64), bounds.astype(np.uint64)):
            return "the caller's offsets were written"
        if feature == "match_at" and pos is not None and len(pos) and not np.array_equal(at_pos.download(8 * len(pos)).view(np.int64), pos):
            return "the caller's positions were written"
        return walk_difference(feature, got, ref)
    finally:
        if r is not None:
            r.free()
        for b in bufs:
            b.free()


def run_walk(cases):
    """-> (ran, failures, skipped, build_errors), as run_surface: every case through the C ABI against reference_walk(case), and
    the host form over the same inputs against it too -- when the two differ, that shows which side is wrong.  One line per
    case, the first difference (feature, column, index, got, want) of a case that fails."""
    ran = fails = skipped = build_errors = 0
    for c in cases:
        tag = f"{c['i']:3d} {_walk_tag(c)}"
        if c["rows"] > ROW_LIMIT:
            print("skip", tag, flush=True)
            skipped += 1
            continue
        before = os.environ.get("ACX_DENSE_LIMIT")
        if c["compressed"]:
            os.environ["ACX_DENSE_LIMIT"] = "0"
        try:
            a = capi.Automaton(c["pats"], c["mk"], kernel=c["kernel"], ascii_case_insensitive=c["ci"])
        except (capi.AcxError, ValueError, MemoryError) as e:
            print("FAIL", tag, "build error:", e, flush=True)
            build_errors += 1; fails += 1
            continue
        finally:
            if c["compressed"]:
                os.environ.pop("ACX_DENSE_LIMIT")
                if before is not None:
                    os.environ["ACX_DENSE_LIMIT"] = before
        t0 = time.time()
        ctx = _walk_ctx(c, 1 << 62)
        ref = reference_walk(c, ctx=ctx)
        diffs = []
        if c["compressed"] and a.info.table_bytes != 0:
            diffs.append("the handle was to be kept in compressed form only and has a dense table")
        for leg, run in (("the library", lambda: _run_walk_case(a, c, ctx, ref)), ("the host form", lambda: walk_host_form(c, ctx, ref))):
            try:
                d = run()
            except (capi.AcxError, ValueError, MemoryError, AssertionError) as e:
                d = f"error: {e}"
            if d:
                diffs.append(f"{leg}: {d}")
        a.close()
        ran += 1
        print(f"{'FAIL' if diffs else 'ok  '} {tag} {time.time() - t0:.2f} s", flush=True)
        for d in diffs:
            print("    ", d, flush=True)
        fails += bool(diffs)
    return ran, fails, skipped, build_errors


WALK_N, WALK_SEED = 140, 20261025  # what tests/test_gpu_fuzz_walk.py runs and tests/test_fuzz_walk_plan_cpu.py checks


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "walk":
        args = [x for x in sys.argv[2:] if x != "--plan-only"]
        plan = plan_walk(int(args[0]) if args else WALK_N, int(args[1]) if len(args) > 1 else WALK_SEED)
        print(walk_coverage_table(plan), flush=True)
        if "--plan-only" in sys.argv:
            sys.exit(0)
        ran, n_fails, skipped, build_errors = run_walk(plan)
        print(f"{ran} cases ran, {n_fails} failures, {skipped} skipped, {build_errors} build errors")
        sys.exit(1 if n_fails or skipped else 0)
    if len(sys.argv) > 1 and sys.argv[1] == "summary":
        args = [x for x in sys.argv[2:] if x != "--plan-only"]
        plan = plan_summary(int(args[0]) if args else SUMMARY_N, int(args[1]) if len(args) > 1 else SUMMARY_SEED)
        print(summary_coverage_table(plan), flush=True)
        if "--plan-only" in sys.argv:
            sys.exit(0)
        ran, n_fails, skipped, build_errors = run_summary(plan)
        print(f"{ran} cases ran, {n_fails} failures, {skipped} skipped, {build_errors} build errors")
        sys.exit(1 if n_fails or skipped else 0)
    if len(sys.argv) > 1 and sys.argv[1] == "surface":
        args = [x for x in sys.argv[2:] if x != "--plan-only"]
        plan = plan_surface(int(args[0]) if args else SURFACE_N, int(args[1]) if len(args) > 1 else SURFACE_SEED)
        print(coverage_table(plan), flush=True)
        if "--plan-only" in sys.argv:
            sys.exit(0)
        ran, n_fails, skipped, build_errors = run_surface(plan)
        print(f"{ran} cases ran, {n_fails} failures, {skipped} skipped, {build_errors} build errors")
        sys.exit(1 if n_fails or skipped else 0)

    n_cases, n_fails = fuzz(float(sys.argv[1]) if len(sys.argv) > 1 else 120.0,
                            int(sys.argv[2]) if len(sys.argv) > 2 else 20260927)
    print(f"{n_cases} cases, {n_fails} failures")
    sys.exit(1 if n_fails else 0)
