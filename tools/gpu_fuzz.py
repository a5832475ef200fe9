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
tests/test_gpu_fuzz.py runs a bounded, seeded slice of it (fuzz(budget, seed, max_size_log2)) under -m gpu,
tests/test_gpu_fuzz_surface.py a fixed number of surface cases; tests/test_fuzz_plan_cpu.py checks what that plan covers;
tests/test_gpu_summary.py a slice of the summary cases, tests/test_summary_cpu.py what their plan covers.
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


if __name__ == "__main__":
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
