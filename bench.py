#!/usr/bin/env python3
"""bench.py -- haystack GB/s of the MI355X-native Aho-Corasick hot path.

Metric (BASELINE.json): haystack GB/s (+ % of the HBM roofline), 10k-pattern DFA.

  N = 1   cfg2: 10 000 patterns (a-z, len 5-12, SplitMix64 seed 1), Implementation.DFA,
          ONE 1 GiB text-like synthetic haystack (seed 11, one pattern planted per KiB),
          MatchKind.Standard, non-overlapping, byte offsets (BytesAhoCorasick path).
  N > 1   cfg3: the same automaton on every GPU; a batch of 8 KiB haystacks cut from one
          global SplitMix64 stream (seed 13, offset by rank), 131 072 haystacks (1 GiB) per GPU
          (weak scaling); no data-path collective; RCCL all-gather of the per-shard match
          counts only.  `python bench.py --gpus N` launches its own N ranks (one per GPU,
          torch.distributed.run, rendezvous on 127.0.0.1) when it is not already running under
          a launcher (RANK unset); under `python -m torch.distributed.run ... bench.py --gpus N`
          it is one of the ranks.  Fewer than N devices: non-zero exit, no line.
  --config cfg2|cfg3|cfg4|cfg4b|cfg5 selects another BASELINE.json configuration at N = 1 (same JSON
          shape, `config.workload` names it): cfg4 = 100 000 patterns a-z, overlapping, uniform
          haystack; cfg4b = the byte-alphabet variant; cfg5 = 10 000 patterns over a-z + 2/3/4-byte
          characters, LeftmostLongest, UTF-8 haystack, code-point indexes (the str API's path).
  --host  the host-memory entry point (acx_find: host bytes in -> host match array out, the
          only shape the reference's API has): a separate, labelled metric, never `value` of
          the device-resident metric.

A "step" is one complete pass of the hot path over the rank's resident batch: scan kernel ->
verification / ordering / match-kind resolution -> final (pattern, start, end) u64 triples in
HBM, their count on the host (+ the count all-gather for N > 1).  Inputs are resident in HBM
before the timed region; nothing is cached between steps.

One JSON line on rank 0; `roofline` is for the dominant kernel (K1) from HIP events recorded on
the library's stream inside the timed region.  A plain run sets up, settles, warms up, times the
K steps and prints the line; everything else it can measure runs only with --full:
  --full  the cold number (config.value_no_settle: the same W + K steps without the settle phase),
          config.secondary (K1a, word-shaped text, names over prose, dense stretches, the density sweep),
          config.target_8gib, and `cpu_baseline`: the reference's algorithm on the host cores of this
          box (rank 0, N = 1): a genuine `ahocorasick_rs` wheel if one is importable, else the oracle's
          C restatement -- 1 core and all cores, 3 warm-ups, median of 7.  The --no-* switches below
          turn single parts of it off.
  --dump-outputs DIR  after the timed steps, what the last timed step returned to its caller, as
          float64 .npy files (exact for offsets and ids below 2^53): count.npy (matches of the step),
          pattern.npy / start.npy / end.npy (the match triples; at most 64 MB in all -- beyond that a
          fixed, seeded sample of the rows, whose row numbers are in match_index.npy), counts.npy
          (matches per haystack, batch configurations).  Ranks other than 0 of a multi-GPU run
          prefix their files with rank<r>_.  The inputs depend on the arguments only.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_GBPS = 8000.0  # MI355X spec, /opt/skills/guides/MI355X_MICROARCH.md
GIB = 1 << 30


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bytes", type=int, default=GIB, help="haystack bytes per GPU")
    ap.add_argument("--callers", type=int, default=1,
                    help="information only: issue the K timed steps from this many host threads at once "
                         "(concurrent calls on one handle); the metric says so")
    ap.add_argument("--settle-ms", type=float, default=50.0,
                    help="untimed steps for this many ms before the W warm-up steps (GPU power-state transient "
                         "after a cold start; 0: none); reported as config.settle_ms")
    ap.add_argument("--ablate", default="", help="measurement only: override the configuration's match kind / "
                    "index kind / overlapping, e.g. mk=standard,cp=0,ov=1 (the line says so in config.workload)")
    ap.add_argument("--config", choices=["auto", "cfg2", "cfg3", "cfg4", "cfg4b", "cfg5", "large", "mixed", "mixedx", "mixedb", "cfg2b"], default="auto",
                    help="auto: cfg2 at N=1, cfg3 at N>1")
    ap.add_argument("--dist", choices=["T", "U", "Z", "D", "H1", "H100"] + ["P%d" % n for n in DENSITIES], default="T",
                    help="cfg2 haystack: T text-like (headline), U iid-uniform a-z, Z all zero bytes "
                         "(calibration of the PMC traffic counters only: the scan reads, nothing else happens), "
                         "D dense: one pattern planted every 32 bytes (>= 1 occurrence per 32 B: the region path)")
    ap.add_argument("--no-target-size", action="store_true",
                    help="skip the in-process run at north_star's target size (8 GiB) that fills config.target_8gib")
    ap.add_argument("--no-secondary", action="store_true",
                    help="skip the secondary lines of the default run (config.secondary: the DFA-walk kernel on the same "
                         "input, word-shaped text, the reference benchmark's names-over-prose shape)")
    ap.add_argument("--no-cold", action="store_true",
                    help="skip the second timed region without the settle phase (config.value_no_settle)")
    ap.add_argument("--kernel", choices=["auto", "dfa_walk", "prefilter"], default="auto")
    ap.add_argument("--workload", choices=["auto", "single", "batch"], default="auto",
                    help="(kept for round-1 scripts) batch == --config cfg3")
    ap.add_argument("--host", action="store_true",
                    help="time the host-memory entry point (acx_find) instead: separate metric")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-sample-bytes", type=int, default=256 << 20,
                    help="prefix of the haystack the 1-core CPU leg scans per run")
    ap.add_argument("--dry-run", action="store_true",
                    help="launcher / collective plumbing only: gloo on CPU, no device work (tests)")
    ap.add_argument("--full", action="store_true",
                    help="also the measurements beside the headline: the cold number, the secondary lines, the 8 GiB "
                         "run and the CPU baseline (each still subject to its --no-* switch)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (float64 .npy, at most 64 MB) into DIR")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.warmup < 0:
        ap.error("--warmup must not be negative")
    if args.dump_outputs and args.callers > 1:
        ap.error("--dump-outputs needs --callers 1 (concurrent callers have no single last step)")
    return args


# ---------------------------------------------------------------------------
# launcher: `python bench.py --gpus N` spawns its own ranks
# ---------------------------------------------------------------------------
def free_port() -> int:
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def self_launch(args) -> int:
    if not args.dry_run:
        import torch
        have = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if have < args.gpus:
            print(f"bench.py: --gpus {args.gpus} but only {have} HIP device(s) are visible", file=sys.stderr)
            return 2
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on this driver (RCCL needs it)
    env["ACX_BENCH_SELF_LAUNCHED"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


# ---------------------------------------------------------------------------
# workloads
# ---------------------------------------------------------------------------
def resolve_config(args, world: int) -> str:
    if args.config != "auto":
        return args.config
    if args.workload == "batch":
        return "cfg3"
    if args.workload == "single":
        return "cfg2"
    return "cfg3" if world > 1 else "cfg2"


def build_workload(cfg: str, args, rank: int, capi, gen, torch, dev):
    import numpy as np
    """-> dict(ac, hay (device tensor), nbytes, find kwargs, description, patterns, match_kind,
    overlapping)."""
    nbytes = args.bytes
    kern = {"auto": None, "dfa_walk": capi.KERNEL_DFA_WALK, "prefilter": capi.KERNEL_PREFILTER}[args.kernel]
    w = {"cfg": cfg, "overlapping": False, "codepoints": False, "n_hay": 0, "uniform_len": 0}
    if cfg in ("cfg2", "cfg3"):
        pats = gen.gen_patterns(10000, 5, 12, gen.AZ, 1)
        w["mk"], impl = capi.MATCH_STANDARD, capi.IMPL_DFA
    elif cfg == "cfg2b":
        # SURVEY 8(d)'s stress variant (B) of cfg2: 10 000 patterns over all byte values (seed 2: 74 579 states,
        # a 72.8 MiB dense table with Implementation.DFA) over iid-uniform bytes
        pats = gen.gen_patterns(10000, 5, 12, gen.ALL_BYTES, 2)
        w["mk"], impl = capi.MATCH_STANDARD, capi.IMPL_DFA
    elif cfg in ("mixed", "mixedx"):
        # cfg2's set plus a 2-byte and a 1-byte pattern (mixed lengths: K1b cannot take the set).  mixed: the
        # short patterns are rare in the haystack (b"qz": 1 per 676 letter pairs, b"~": never); mixedx: the
        # round-2 VERDICT's example b"ab" + b"x" -- one occurrence per ~22 bytes of a-z text: dense output
        pats = gen.gen_patterns(10000, 5, 12, gen.AZ, 1) + ([b"qz", b"~"] if cfg == "mixed" else [b"ab", b"x"])
        w["mk"], impl = capi.MATCH_STANDARD, capi.IMPL_DFA
    elif cfg in ("cfg4", "cfg4b"):
        pats = gen.gen_patterns(100000, 5, 12, gen.AZ if cfg == "cfg4" else gen.ALL_BYTES, 3 if cfg == "cfg4" else 4)
        w["mk"], impl, w["overlapping"] = capi.MATCH_STANDARD, capi.IMPL_AUTO, True
    elif cfg == "large":
        # construction at scale (not a BASELINE.json configuration): 1 M patterns, an automaton of
        # ~4.9 M states that is kept in its compressed form (no dense table)
        pats = gen.gen_patterns(1000000, 8, 16, gen.AZ, 9)
        w["mk"], impl = capi.MATCH_LEFTMOST_LONGEST, capi.IMPL_AUTO
    else:  # cfg5 / mixedb
        spats = list(dict.fromkeys(gen.gen_patterns(10000, 5, 12, gen.AZ_UNI, 5)))
        pats = [p.encode() for p in spats]
        if cfg == "mixedb":
            # round 3's cliff: cfg5's set (> 32 byte classes) + 1-character patterns of 1 and 2 bytes that are rare
            # in the haystack ("Q": its low five bits are q's -- the side test's aliasing is part of the number)
            pats += ["ß".encode(), b"Q"]
        w["mk"], impl, w["codepoints"] = capi.MATCH_LEFTMOST_LONGEST, capi.IMPL_AUTO, True
    t0 = time.perf_counter()
    for kv in filter(None, (args.ablate or "").split(",")):  # measurement switches, never the judged line
        k, v = kv.split("=")
        if k == "mk":
            w["mk"] = {"standard": capi.MATCH_STANDARD, "lf": capi.MATCH_LEFTMOST_FIRST, "ll": capi.MATCH_LEFTMOST_LONGEST}[v]
        elif k == "cp":
            w["codepoints"] = bool(int(v))
        elif k == "ov":
            w["overlapping"] = bool(int(v))
        else:
            raise SystemExit(f"--ablate: unknown switch {k}")
    ac = capi.Automaton(pats, w["mk"], impl, kernel=kern)
    w.update(ac=ac, patterns=pats, build_s=time.perf_counter() - t0)
    if cfg in ("cfg5", "mixedb"):
        # ~1.13 bytes per character at 5 % non-ASCII: generate enough characters, cut at a
        # character boundary at or below --bytes
        host = gen.gen_unicode_textlike_bytes(int(nbytes / 1.12) + 1024, 56, spats,
                                              threads=min(32, os.cpu_count() or 1))
        cut = min(nbytes, len(host))
        while cut < len(host) and (host[cut] & 0xC0) == 0x80:
            cut -= 1
        nbytes = cut
        hay = torch.from_numpy(host[:cut]).to(dev)
        w["desc"] = (f"cfg5: 10k patterns over a-z + e-acute/snowman/facepalm (2/3/4-byte), seed 5, MatchKind."
                     f"LeftmostLongest, {nbytes / GIB:.3f} GiB UTF-8 text-like str haystack (~5 % non-ASCII, "
                     "seed 56), code-point indexes (AhoCorasick str path)")
        if cfg == "mixedb":
            w["desc"] = "mixedb (not a BASELINE configuration): cfg5's set + the 1-character patterns sharp-s (2 bytes) and Q; " + w["desc"][6:]
    else:
        hay = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        if cfg in ("cfg2", "mixed", "mixedx"):
            if args.dist == "Z":
                hay.zero_()
                torch.cuda.synchronize()
            elif args.dist == "D":
                # dense output: uniform a-z with a pattern planted at every multiple of 32 bytes (chunks built
                # on the host from one 16 MiB period: the content repeats, the scan does not care)
                per = gen.gen_uniform(PERIOD_BYTES, gen.AZ, 12)  # (not 16 MiB: tile_to_device)
                rng = gen.SplitMix64(77)
                for k in range(0, len(per) - 32, 32):
                    p = np.frombuffer(pats[rng.next() % len(pats)], dtype=np.uint8)
                    per[k:k + len(p)] = p
                dper = torch.from_numpy(per).to(dev)
                for off in range(0, nbytes, len(per)):
                    n_ = min(len(per), nbytes - off)
                    hay[off:off + n_] = dper[:n_]
                torch.cuda.synchronize()
            elif args.dist in ("H1", "H100") or args.dist.startswith("P"):
                # the headline's text with dense stretches / a denser plant on top (the hot pipeline: DESIGN.md)
                ac.generate(hay.data_ptr(), nbytes, 1, 11)
                torch.cuda.synchronize()
                if args.dist.startswith("P"):
                    overlay_planted(hay, pats, int(args.dist[1:]), None, torch, dev)
                else:
                    overlay_planted(hay, pats, 32, hot_regions(args.dist, nbytes), torch, dev)
            else:
                kind, seed = (1, 11) if args.dist == "T" else (0, 12)
                ac.generate(hay.data_ptr(), nbytes, kind, seed)
            what = {"H1": "text-like T (seed 11) with ONE 64 KiB region that holds a pattern every 32 bytes (not the headline)",
                    "H100": "text-like T (seed 11) with every 100th 256 KiB group holding a pattern every 32 bytes -- 1 % of the groups (not the headline)",
                    **{"P%d" % n: "text-like T (seed 11) + a pattern planted every %d bytes everywhere (density sweep, not the headline)" % n
                       for n in DENSITIES},
                    "T": "text-like (T, seed 11: iid a-z letters, a space with probability 43/256 at every "
                         "position -- geometric word lengths, not a natural-language word model -- one pattern planted per KiB)", "U": "uniform a-z (U, seed 12)",
                    "Z": "ALL-ZERO (calibration only, not a benchmark)",
                    "D": "DENSE (uniform a-z, one pattern planted every 32 bytes, period 4093 x 4 KiB: the dense path, "
                         "not the headline)"}[args.dist]
            w["desc"] = ("cfg2: 10k patterns a-z len 5-12 (seed 1), Implementation.DFA, one "
                         f"{nbytes / GIB:g} GiB {what} bytes haystack, MatchKind.Standard, non-overlapping")
            if cfg != "cfg2":
                w["desc"] = (f"{cfg} (not a BASELINE configuration): cfg2's set + " +
                             ("b'qz' + b'~' (short patterns that are rare in the haystack)" if cfg == "mixed"
                              else "b'ab' + b'x' (one occurrence per ~22 bytes: dense output)") + "; " + w["desc"][6:])
        elif cfg == "cfg3":
            if nbytes % 8192:
                raise SystemExit("--bytes must be a multiple of 8192 for cfg3")
            ac.generate(hay.data_ptr(), nbytes, 1, 13, stream_offset=rank * nbytes)
            w["uniform_len"], w["n_hay"] = 8192, nbytes // 8192
            w["desc"] = ("cfg3: 10k patterns a-z len 5-12 (seed 1), Implementation.DFA, batch of "
                         f"{nbytes // 8192} x 8 KiB haystacks per GPU from one SplitMix64 stream (seed 13, "
                         "offset by rank), MatchKind.Standard, sharded by haystack, RCCL all-gather of match counts")
        elif cfg == "large":
            ac.generate(hay.data_ptr(), nbytes, 1, 11)
            w["desc"] = (f"large: 1M patterns a-z len 8-16 (seed 9), implementation=None, MatchKind.LeftmostLongest, "
                         f"one {nbytes / GIB:g} GiB text-like (T, seed 11) haystack")
        elif cfg == "cfg4":
            ac.generate(hay.data_ptr(), nbytes, 0, 12)
            w["desc"] = (f"cfg4: 100k patterns a-z len 5-12 (seed 3), implementation=None, overlapping=True, one "
                         f"{nbytes / GIB:g} GiB uniform a-z haystack (seed 12)")
        elif cfg == "cfg2b":
            host = gen.gen_uniform(nbytes, gen.ALL_BYTES, 12)
            hay = torch.from_numpy(host).to(dev)
            w["desc"] = (f"cfg2b (stress variant B of cfg2): 10k patterns over all byte values len 5-12 (seed 2), "
                         f"Implementation.DFA, MatchKind.Standard, one {nbytes / GIB:g} GiB uniform-bytes haystack (seed 12)")
        else:
            host = gen.gen_uniform(nbytes, gen.ALL_BYTES, 12)
            hay = torch.from_numpy(host).to(dev)
            w["desc"] = (f"cfg4b: 100k patterns over all byte values len 5-12 (seed 4), implementation=None, "
                         f"overlapping=True, one {nbytes / GIB:g} GiB uniform-bytes haystack (seed 12)")
    if args.ablate:
        w["desc"] += f" [ABLATION {args.ablate}: not the configuration's own settings]"
    w.update(hay=hay, nbytes=nbytes)
    return w


# ---------------------------------------------------------------------------
def run(args) -> None:
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")

    import numpy as np
    import torch
    dist = None
    if args.dry_run:
        dev = torch.device("cpu")
        if "RANK" in os.environ:
            import torch.distributed as dist
            dist.init_process_group(backend="gloo")
        w = {"cfg": resolve_config(args, world), "nbytes": args.bytes, "desc": "dry run: no device work"}
    else:
        import gen
        from ahocorasick_rs_amd import capi
        if not torch.cuda.is_available() or capi.device_count() < 1:
            raise SystemExit("bench.py needs a HIP device (there is no CPU fallback)")
        if torch.cuda.device_count() < world:
            raise SystemExit(f"{world} ranks but only {torch.cuda.device_count()} HIP device(s)")
        torch.cuda.set_device(local_rank)
        capi.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
        if world > 1 or "RANK" in os.environ:  # one rank per GPU over RCCL
            import torch.distributed as dist
            dist.init_process_group(backend="nccl", device_id=dev)
        w = build_workload(resolve_config(args, world), args, rank, capi, gen, torch, dev)
    world_observed = dist.get_world_size() if dist is not None else 1
    cfg, nbytes = w["cfg"], w["nbytes"]

    # The count all-gather of a step overlaps the next step's scan: a helper thread issues it (the host
    # side of a torch collective -- filling the 8-byte tensor, enqueueing, waiting -- is ~80 us of Python
    # and launch overhead, a fifth of a step, and the main thread is inside the library with the GIL
    # released meanwhile); two buffers are used in turn, the last gather is waited for inside the timed
    # region.  Nothing on the data path depends on it.
    counts_local = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(2)]
    counts_all = [torch.zeros(world, dtype=torch.int64, device=dev) for _ in range(2)]
    pending = [None, 0]  # [unused, steps issued]
    gather_q = None
    if dist is not None:
        import queue
        import threading
        gather_q = queue.Queue()

        def gather_worker():
            if not args.dry_run:
                torch.cuda.set_device(dev)
            while True:
                item = gather_q.get()
                if item is None:
                    gather_q.task_done()
                    return
                k, n = item
                counts_local[k].fill_(n)
                dist.all_gather_into_tensor(counts_all[k], counts_local[k])
                gather_q.task_done()

        threading.Thread(target=gather_worker, daemon=True).start()
    last = {}

    def hot(hold: bool = False) -> int:
        """one pass of the hot path over this rank's batch (no collective); hold: keep the device result
        (last["held"]) instead of freeing it"""
        if args.dry_run:
            n = 1000 + rank
        elif args.host:
            m = w["ac"].find(w["host_hay"], overlapping=w["overlapping"], codepoints=w["codepoints"])
            n = len(m)
            last["matches"] = m
        elif last.get("keep"):
            r = w["ac"].find_device(w["hay"].data_ptr(), nbytes, n_hay=w["n_hay"], uniform_len=w["uniform_len"],
                                    overlapping=w["overlapping"], codepoints=w["codepoints"])
            n = r.count
            last["matches"] = r.matches()
            r.free()
        else:
            # the same three C-ABI calls as capi.Automaton.find_device + DeviceResult.count / free, without the Python
            # objects in between (a step is ~350 us: ten microseconds of interpreter per step are three percent)
            n = fast_step(hold)
        return n

    fast_step = None
    if not args.dry_run and not args.host:
        import ctypes
        L_ = capi.lib()
        h_, out_ = w["ac"]._h, ctypes.c_void_p()
        ptr_, ref_ = w["hay"].data_ptr(), ctypes.byref(out_)
        nh_, ul_, ov_, cp_ = w["n_hay"], w["uniform_len"], int(w["overlapping"]), int(w["codepoints"])

        def fast_step(hold: bool = False) -> int:
            rc = L_.acx_find_device(h_, ptr_, nbytes, None, nh_, ul_, ov_, cp_, ref_)
            if rc:
                capi._check(rc)
            n_ = L_.acx_result_count(out_)
            if hold:  # (--dump-outputs: the last timed step's result is read after the timed region)
                last["held"] = capi.DeviceResult(out_.value, nh_ if ul_ else 0)
            else:
                L_.acx_free_result(out_)
            return n_

    def gather_wait() -> None:
        if gather_q is not None:
            gather_q.join()

    def step(hold: bool = False) -> int:
        n = hot(hold)
        if dist is not None:  # C1: per-shard match counts -> global output offsets
            k = pending[1] & 1
            pending[1] += 1
            gather_q.put((k, n))
        return n

    if args.host and not args.dry_run:
        w["host_hay"] = w["hay"].cpu().numpy()  # pageable host memory, what a Python caller holds

    def sync():
        if not args.dry_run:
            torch.cuda.synchronize()

    n_matches = 0
    n_gathers = [0]
    _step = step

    def step(hold: bool = False) -> int:  # (counts the collectives: config.collective says what ran)
        if dist is not None:
            n_gathers[0] += 1
        return _step(hold)

    def timed_region(steps: int, warmup: int, profile: bool, hold_last: bool = False):
        """W untimed warm-up steps, then exactly K steps between barrier + synchronize on both sides
        (hold_last: the K-th step keeps its result for --dump-outputs)"""
        n = 0
        for _ in range(warmup):
            n = step()
        gather_wait()  # (the helper thread is idle whenever this thread talks to the communicator)
        if profile and not args.dry_run:
            # the kernel time is measured live in the timed region, on every 4th step (the event pair
            # costs the dispatch it rides on ~6 us; roofline.kernel_ms_samples says how many were taken)
            w["ac"].profile_enable(4 if steps >= 8 else 1)
            w["ac"].profile_read(reset=True)
        if dist is not None:
            dist.barrier()
        sync()
        t0 = time.perf_counter()
        if args.callers > 1 and dist is None and not args.dry_run:
            # (information only, never the default: K steps issued by several host threads at once -- the
            # reference releases the GIL around a search, src/lib.rs:238, and a handle here serves up to
            # ACX_MAX_CONCURRENCY calls side by side, each on its own stream)
            import threading
            per = [steps // args.callers + (1 if i < steps % args.callers else 0) for i in range(args.callers)]
            ths = [threading.Thread(target=lambda k=k: [hot() for _ in range(k)]) for k in per]
            for th in ths:
                th.start()
            for th in ths:
                th.join()
        else:
            for _ in range(steps - 1 if hold_last else steps):
                n = step()
            if hold_last:
                n = step(True)
        gather_wait()
        sync()
        if dist is not None:
            dist.barrier()
        dt = time.perf_counter() - t0
        pr = None
        if profile and not args.dry_run:
            pr = w["ac"].profile_read(reset=True)
            w["ac"].profile_enable(False)
        return dt, n, pr

    # ---- (1) the cold number, on the record next to the settled one (config.value_no_settle): the very
    # same W warm-up + K timed steps WITHOUT the settle phase, from an idle GPU (2 s of idleness put the
    # power controller back into its start-up transient: profiles/r02/step_times_cold_start.txt); --full only
    cold = None
    if args.full and not args.dry_run and not args.no_cold and args.settle_ms > 0:
        n_matches = hot()  # the first call allocates the workspaces: tens of ms, part of neither region
        sync()
        time.sleep(2.0)
        dt, n_matches, _ = timed_region(args.steps, args.warmup, False)
        cold = dt
        time.sleep(0.5)
    # ---- (2) settle (untimed, before the W warm-up steps, disclosed in config.settle_ms): from a cold
    # start the GPU's power controller goes through a transient of ~15 ms -- boost clocks for the first
    # few steps, a dip while it finds the power limit, then the sustained state.  W = 5 warm-up steps
    # end in the middle of it; a throughput metric is about the sustained state.
    settled = 0
    if args.settle_ms > 0 and not args.dry_run:
        # (the hot path only: the ranks settle by time, each for itself -- no collective in here)
        n_matches = hot()
        settled += 1
        sync()
        t_end = time.perf_counter() + args.settle_ms * 1e-3
        while time.perf_counter() < t_end:
            n_matches = hot()
            settled += 1
    elapsed, n_matches, prof = timed_region(args.steps, args.warmup, True, hold_last=bool(args.dump_outputs))
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, last, n_matches, "" if rank == 0 else f"rank{rank}_", DUMP_LIMIT // world)

    total_matches = n_matches
    per_rank = [nbytes * args.steps / elapsed / 1e9]
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        every = torch.zeros(world, dtype=torch.float64, device=dev)
        dist.all_gather_into_tensor(every, t)
        per_rank = [nbytes * args.steps / float(x) / 1e9 for x in every.cpu().tolist()]
        elapsed = float(every.max().item())  # MAX over ranks
        total_matches = int(counts_all[(pending[1] - 1) & 1].sum().item())
        if cold is not None:
            t = torch.tensor([cold], dtype=torch.float64, device=dev)
            dist.all_gather_into_tensor(every, t)
            cold = float(every.max().item())

    if rank == 0:
        ms_per_step = elapsed / args.steps * 1e3
        value = world * nbytes * args.steps / elapsed / 1e9
        out = {
            "metric": "haystack GB/s, 10k-pattern DFA",
            "value": round(value, 2),
            "unit": "GB/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u8",
            "data": "synthetic",
            "config": {"workload": w["desc"], "bytes_per_gpu": nbytes,
                       "world_size_observed": world_observed,
                       "launcher": "self (torch.distributed.run)" if os.environ.get("ACX_BENCH_SELF_LAUNCHED")
                       else ("torch.distributed.run" if "RANK" in os.environ else "none"),
                       "per_rank_gbps": [round(x, 2) for x in per_rank],
                       "settle_ms": 0 if args.dry_run else args.settle_ms, "settle_steps": settled,
                       "value_no_settle": None if cold is None else round(world * nbytes * args.steps / cold / 1e9, 2),
                       "ms_per_step_no_settle": None if cold is None else round(cold / args.steps * 1e3, 4),
                       "collective": {"backend": dist.get_backend() if dist is not None else None,
                                      "all_gathers": n_gathers[0], "what": "per-rank match counts (8 B per rank)"},
                       "matches_per_gpu_step": int(n_matches), "matches_total": int(total_matches)},
        }
        if cfg not in ("cfg2", "cfg3"):
            out["metric"] = f"haystack GB/s, {cfg} (not the headline metric)"
        if args.host:
            out["metric"] = ("host-memory entry point GB/s (acx_find: pageable host bytes in -> host match array "
                             f"out, PCIe-inclusive), {cfg}")
        if args.callers > 1:
            out["metric"] += f" ({args.callers} concurrent callers on one handle: not the headline)"
            out["config"]["callers"] = args.callers
        if args.dry_run:
            out["metric"] = "dry run (launcher / collective plumbing only)"
            out["data"] = "none"
        else:
            info = w["ac"].info
            scan_ms = prof.scan_ms / max(prof.scan_launches, 1)
            algo_bytes = nbytes + 24 * n_matches  # 1 B read / haystack byte + 24 B / match
            achieved = algo_bytes / (scan_ms * 1e-3) / 1e9 if scan_ms > 0 else 0.0
            # (the scan stage: K1b, or K1a = k1a_scan + k1a_walk -- automata of more than 32 byte classes, and the
            # dense path, walk in chunks: k1a_walk16 / k1a_dfa_walk)
            kname = "k1b_prefilter" if info.kernel == capi.KERNEL_PREFILTER else (
                "k1a_walk16 (chunked)" if os.environ.get("ACX_NO_PFAC") else "k1a_scan+k1a_walk")
            traffic, traffic_src = measured_traffic(kname, nbytes, args.dist, cfg)
            out["config"].update({
                "n_patterns": len(w["patterns"]), "n_states": int(info.n_states),
                "dfa_table_bytes": int(info.table_bytes), "build_s": round(w["build_s"], 3), "scan_kernel": capi.KERNEL_NAMES[info.kernel],
                "raw_occurrences_per_step": int(prof.raw_occurrences // max(prof.scan_launches, 1)),
                "prefix_hits_per_step": int(prof.prefix_hits // max(prof.scan_launches, 1)),
                "percent_of_hbm_roofline": round(100.0 * value / (HBM_PEAK_GBPS * world), 2),
            })
            out["roofline"] = {
                "bound": "hbm", "kernel": kname, "achieved": round(achieved, 2), "peak": HBM_PEAK_GBPS,
                "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBPS, 4), "traffic": traffic,
                "traffic_source": traffic_src, "kernel_ms": round(scan_ms, 4),
                "kernel_ms_samples": int(prof.scan_launches),
                "algorithmic_bytes": int(algo_bytes),
            }
            if (args.full and world == 1 and cfg == "cfg2" and args.dist == "T" and nbytes == GIB and not args.no_secondary
                    and not args.host and args.callers == 1 and not args.ablate and args.kernel == "auto"):
                # (before the 8 GiB run: the lines that sit next to the headline are taken in the headline's own state)
                out["config"]["secondary"] = secondary_runs(w, capi, gen, torch, dev)
            if (args.full and world == 1 and cfg == "cfg2" and args.dist == "T" and nbytes == GIB and not args.no_target_size
                    and not args.host and args.callers == 1 and not args.ablate and args.kernel == "auto"):
                out["config"]["target_8gib"] = target_size_run(w, torch, dev)
            if args.full and world == 1 and not args.no_cpu_baseline:
                last["keep"] = True
                step()  # one more pass, keeping the match stream for the SHA-256 comparison
                out["cpu_baseline"] = cpu_baseline(w, last.get("matches"), args.cpu_sample_bytes)
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def timed_steps(ac, ptr, nbytes, torch, steps=10, warmup=4, **kw):
    """W warm-up + K timed steps of find_device behind the settled state of the main run
    -> (ms per step, matches, ms of the scan stage from the event pair on every 4th step)"""
    n = 0
    t_end = time.perf_counter() + 0.03  # (untimed: the same settle phase as the headline's, scaled down: another kernel
    k = 0                               # mix goes through its own power transient)
    while k < warmup or time.perf_counter() < t_end:
        r = ac.find_device(ptr, nbytes, **kw)
        n = r.count
        r.free()
        k += 1
    ac.profile_enable(4)
    ac.profile_read(reset=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        r = ac.find_device(ptr, nbytes, **kw)
        n = r.count
        r.free()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps * 1e3
    pr = ac.profile_read(reset=True)
    ac.profile_enable(False)
    return dt, int(n), round(pr.scan_ms / max(pr.scan_launches, 1), 4)


PERIOD_BYTES = 4093 * 4096  # (see tile_to_device)


def overlay_planted(hay, pats, every: int, regions, torch, dev, seed: int = 77):
    """plant a pattern of `pats` at every multiple of `every` bytes (>= 32) inside the byte ranges `regions` of the device
    haystack `hay` (None: everywhere), on top of what is there: the planted bytes of one period are built on the host
    (values + mask), the overlay itself is a device-side select.  -> planted slots"""
    import numpy as np
    import gen
    span = PERIOD_BYTES if regions is None else min(PERIOD_BYTES, max(b - a for a, b in regions))
    val = np.zeros(span, dtype=np.uint8)
    msk = np.zeros(span, dtype=np.bool_)
    rng = gen.SplitMix64(seed)
    for k in range(0, span - 32, every):
        p_ = np.frombuffer(pats[rng.next() % len(pats)], dtype=np.uint8)
        val[k:k + len(p_)] = p_
        msk[k:k + len(p_)] = True
    dval, dmsk = torch.from_numpy(val).to(dev), torch.from_numpy(msk).to(dev)
    nbytes = hay.numel()
    slots = 0
    for a, b in (regions if regions is not None else [(0, nbytes)]):
        for off in range(a, b, span):
            n_ = min(span, b - off)
            seg = hay[off:off + n_]
            seg.copy_(torch.where(dmsk[:n_], dval[:n_], seg))
            slots += n_ // every
    torch.cuda.synchronize()
    return slots


DENSITIES = (1024, 512, 256, 128, 64, 32)  # --dist P<n>: T + a pattern planted every n bytes, everywhere
GROUP_BYTES = 64 * 4096                    # the sparse path's group: 64 tiles of 4 KiB


def hot_regions(dist: str, nbytes: int):
    """H1: ONE 64 KiB region (a third of the way in) holds a pattern every 32 bytes; H100: every 100th 256 KiB group does,
    whole (1 % of the groups, scattered: none is another's neighbour)"""
    if dist == "H1":
        a = (nbytes // 3) & ~(GROUP_BYTES - 1)
        return [(a + 8 * 4096, a + 8 * 4096 + (64 << 10))] if nbytes >= a + GROUP_BYTES else [(0, min(nbytes, 64 << 10))]
    groups = nbytes // GROUP_BYTES
    return [(g * GROUP_BYTES, (g + 1) * GROUP_BYTES) for g in range(50, groups, 100)] or [(0, min(nbytes, GROUP_BYTES))]


def tile_to_device(period, nbytes, torch, dev):
    """a device haystack of nbytes made of copies of `period` (host numpy bytes): a 1 GiB host array would cost
    more time than the measurement.  The period is 4093 tiles of 4 KiB -- NOT the 16 MiB it was at first: a K1b
    wave scans the tiles gw, gw + 4096, gw + 8192, ...; with a period of 4096 tiles every one of them had the
    SAME content, a wave with an expensive tile kept it for the whole launch, and the kernel ran at the pace of
    the unluckiest wave (measured: 333 us against 284 us on the same text unrepeated)."""
    hay = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dper = torch.from_numpy(period).to(dev)
    for off in range(0, nbytes, len(period)):
        n_ = min(len(period), nbytes - off)
        hay[off:off + n_] = dper[:n_]
    torch.cuda.synchronize()
    return hay


def secondary_runs(w, capi, gen, torch, dev, nbytes: int = GIB):
    """Lines that belong next to the headline, same process, same settled GPU:
      k1a      the kernel north_star describes (the DFA walk, failureless form) on the headline's very input
      T_words  the headline's set over SURVEY 8d's T as worded: a-z words of 1-10 letters, single spaces
      prose    the reference benchmark's "long" shape (benchmarks/test_comparison.py:16-53): 4 244 names-like patterns
               (5 % duplicates) over ~600-byte prose lines, a name in every third line; with the fraction of the
               positions that survive level 1 of the prefilter (CPU simulation of the kernel's test on the
               product's own table over the 16 MiB period)
    Each: {gbps, frac (of 8 TB/s), ms_per_step, matches}.  Device-resident, 10 timed steps."""
    import numpy as np
    out = {}

    def roof(kms, n):  # the scan stage's roofline, as the headline's: algorithmic bytes / its event-pair time
        ach = (nbytes + 24 * n) / (kms * 1e-3) / 1e9 if kms > 0 else 0.0
        return {"bound": "hbm", "achieved": round(ach, 2), "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBPS, 4),
                "kernel_ms": kms, "algorithmic_bytes": int(nbytes + 24 * n)}
    try:
        k1a = capi.Automaton(w["patterns"], w["mk"], capi.IMPL_DFA, kernel=capi.KERNEL_DFA_WALK)
        ms, n, kms = timed_steps(k1a, w["hay"].data_ptr(), nbytes, torch)
        out["k1a"] = {"kernel": "k1a_scan+k1a_walk", "gbps": round(nbytes / ms / 1e6, 2), "frac": round(nbytes / ms / 1e6 / HBM_PEAK_GBPS, 4),
                      "ms_per_step": round(ms, 4), "scan_ms": kms, "matches": n, "roofline": roof(kms, n)}
        k1a.close()
    except Exception as e:
        out["k1a"] = {"skipped": repr(e)}
    try:
        per = gen.gen_words(16 << 20, 11, w["patterns"])[:PERIOD_BYTES]
        hay = tile_to_device(per, nbytes, torch, dev)
        ms, n, kms = timed_steps(w["ac"], hay.data_ptr(), nbytes, torch)
        out["T_words"] = {"what": "cfg2's set over a-z words of 1-10 letters, single spaces, one pattern planted per KiB "
                                  "(period: 4093 tiles of 4 KiB)", "gbps": round(nbytes / ms / 1e6, 2),
                          "frac": round(nbytes / ms / 1e6 / HBM_PEAK_GBPS, 4), "ms_per_step": round(ms, 4), "scan_ms": kms, "matches": n,
                          "roofline": roof(kms, n)}
        del hay
    except Exception as e:
        out["T_words"] = {"skipped": repr(e)}
    try:
        names = [p.encode() for p in gen.names_like(4244, 6)]
        per = np.frombuffer(gen.names_haystack([p.decode() for p in names], PERIOD_BYTES, every=3), dtype=np.uint8).copy()
        ac = capi.Automaton(names, capi.MATCH_STANDARD, capi.IMPL_AUTO)
        hay = tile_to_device(per, nbytes, torch, dev)
        ms, n, kms = timed_steps(ac, hay.data_ptr(), nbytes, torch)
        surv = None
        try:
            h = capi.HostAutomaton(names, capi.MATCH_STANDARD)
            surv = round(100.0 * gen.level1_survivor_rate(np.asarray(h.filter_xy), int(h.t.filter_q), per[: 4 << 20]), 3)
            h.close()
        except Exception:
            pass
        out["prose"] = {"what": "4 244 names-like patterns (5-12 letters, ~5 % duplicates) over prose lines, a name in every "
                                "third line (tests/gen.py names_haystack, period: 4093 tiles of 4 KiB): the reference benchmark's long shape",
                        "kernel": capi.KERNEL_NAMES[ac.info.kernel], "gbps": round(nbytes / ms / 1e6, 2),
                        "frac": round(nbytes / ms / 1e6 / HBM_PEAK_GBPS, 4), "ms_per_step": round(ms, 4), "scan_ms": kms, "matches": n,
                        "level1_survivor_pct": surv, "roofline": roof(kms, n)}
        ac.close()
        del hay
    except Exception as e:
        out["prose"] = {"skipped": repr(e)}
    # where the matches are must not decide what a byte costs (the reference's loop: src/lib.rs:59): the headline's text
    # with dense stretches (the hot pipeline takes the groups they lie in), and the whole curve from sparse to dense
    try:
        hay = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        hot, dens = {}, {}
        for name in ("H1", "H100"):
            w["ac"].generate(hay.data_ptr(), nbytes, 1, 11)
            torch.cuda.synchronize()
            overlay_planted(hay, w["patterns"], 32, hot_regions(name, nbytes), torch, dev)
            ms, n, kms = timed_steps(w["ac"], hay.data_ptr(), nbytes, torch, steps=8, warmup=3)
            hot[name] = {"gbps": round(nbytes / ms / 1e6, 2), "frac": round(nbytes / ms / 1e6 / HBM_PEAK_GBPS, 4),
                         "ms_per_step": round(ms, 4), "scan_ms": kms, "matches": n, "roofline": roof(kms, n)}
        hot["what"] = ("the headline's text T with a pattern planted every 32 bytes in ONE 64 KiB region (H1) / in every 100th 256 KiB "
                       "group, whole: 1 % of the groups (H100)")
        out["hot"] = hot
        for every in DENSITIES:
            w["ac"].generate(hay.data_ptr(), nbytes, 1, 11)
            torch.cuda.synchronize()
            overlay_planted(hay, w["patterns"], every, None, torch, dev)
            ms, n, kms = timed_steps(w["ac"], hay.data_ptr(), nbytes, torch, steps=6, warmup=3)
            dens[str(every)] = {"gbps": round(nbytes / ms / 1e6, 2), "ms_per_step": round(ms, 4), "scan_ms": kms, "matches": n}
        dens["what"] = ("the headline's text T + a pattern planted every N bytes everywhere: N -> GB/s (whole step, 1 GiB); round 6: "
                        "from one match per 256 bytes on the context takes the wide form of the post stage, from one per 64 bytes on "
                        "the dense path")
        g = [dens[str(e)]["gbps"] for e in DENSITIES]
        dens["largest_step_between_neighbours"] = round(max(a / b for a, b in zip(g, g[1:])), 2)
        out["density"] = dens
        # (the handle as the headline left it: the dense inputs above hold a context on the dense path until it sees an input
        # that is not dense -- one call -- and on the wide form of the post stage until a call of it sees a sparse input -- one more)
        w["ac"].generate(hay.data_ptr(), nbytes, 1, 11)
        torch.cuda.synchronize()
        for _ in range(3):
            r = w["ac"].find_device(hay.data_ptr(), nbytes)
            r.free()
        torch.cuda.synchronize()
        del hay
    except Exception as e:
        out["density"] = {"skipped": repr(e)}
    return out


def target_size_run(w, torch, dev, nbytes: int = 8 * GIB, steps: int = 5, warmup: int = 2):
    """north_star's target size in the same process: the same automaton over ONE 8 GiB text-like haystack
    (same generator, seed 11; match offsets beyond 2^32), W warm-up + K timed steps behind the settled
    state of the main run.  -> {bytes, steps, ms_per_step, gbps, frac (of 8 TB/s), matches}"""
    try:
        free, _ = torch.cuda.mem_get_info()
        if free < nbytes * 2:
            return {"skipped": f"only {free >> 30} GiB of HBM free"}
        ac = w["ac"]
        hay = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ac.generate(hay.data_ptr(), nbytes, 1, 11)
        n = 0
        for _ in range(warmup + 1):  # (+1: the first call at this size grows the workspaces)
            r = ac.find_device(hay.data_ptr(), nbytes)
            n = r.count
            r.free()
        torch.cuda.synchronize()
        ac.path_stats(reset=True)
        t0 = time.perf_counter()
        for _ in range(steps):
            r = ac.find_device(hay.data_ptr(), nbytes)
            n = r.count
            r.free()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        del hay
        gbps = nbytes / dt / 1e9
        paths = {k: v for k, v in ac.path_stats().items() if v}  # (which way the timed calls went: acx_path_stats)
        return {"bytes": nbytes, "steps": steps, "warmup": warmup, "ms_per_step": round(dt * 1e3, 4),
                "gbps": round(gbps, 2), "frac": round(gbps / HBM_PEAK_GBPS, 4), "matches": int(n), "paths": paths}
    except Exception as e:  # never take the headline down
        return {"skipped": f"failed: {e!r}"}


DUMP_LIMIT = 64 * 10 ** 6  # --dump-outputs: bytes written at most, all ranks together


def dump_outputs(d: str, last: dict, n: int, prefix: str, limit: int) -> None:
    """--dump-outputs: what the last timed step returned to its caller, as float64 .npy files (exact below 2^53):
    count, for a batch the matches per haystack (counts), and the match triples (pattern / start / end).  An array that
    would not fit in `limit` is replaced by a fixed, seeded sample of its rows, whose row numbers go into
    <name>_index (match_index for the triples)."""
    import numpy as np
    r = last.pop("held", None)  # (device path: the held result; host path: the last step's host array)
    try:
        matches = last.get("matches") if r is None else r.matches()
        counts = r.counts() if r is not None and r.n_hay else None
    finally:
        if r is not None:
            r.free()
    out = {"count": np.array([n], dtype=np.float64)}

    def fit(a, width: int, share: int, name: str):
        """-> (the rows of `a` -- `width` float64 columns each -- that fit in `share` bytes: all, or a seeded sample whose
        row numbers go into <name>_index; bytes used)"""
        if len(a) * width * 8 <= share:
            return a, len(a) * width * 8
        keep = share // ((width + 1) * 8)
        idx = np.sort(np.random.default_rng(1).choice(len(a), keep, replace=False))
        out[name + "_index"] = idx.astype(np.float64)
        return a[idx], keep * (width + 1) * 8

    room = limit - 8 - 4096  # (the count, the .npy headers)
    if counts is not None:  # (the per-haystack counts take at most half, the triples the rest)
        counts, used = fit(counts, 1, room // 2, "counts")
        room -= used
        out["counts"] = counts.astype(np.float64)
    if matches is not None:
        matches, _ = fit(matches, 3, room, "match")
        for c in ("pattern", "start", "end"):
            out[c] = np.ascontiguousarray(matches[c]).astype(np.float64)
    os.makedirs(d, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(d, prefix + name + ".npy"), a)


def measured_traffic(kernel: str, nbytes: int, dist_name: str, cfg: str):
    """HBM bytes per launch of the dominant kernel from the PMC passes of the SAME command
    (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, gfx950 correction; produced by
    tools/collect_profiles.sh and committed under profiles/).  NOT measured in this run: the
    second value names the file the number comes from; (None, None) when no measurement of this
    exact configuration is on file -- or when the file's counters were read from other device code than
    this tree's (kernel_source_sha256, tools/kernel_hash.py): a figure goes stale the moment a kernel changes."""
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from kernel_hash import kernel_source_sha256
        now = kernel_source_sha256()
        best = (None, None)
        for d in sorted(os.listdir(os.path.join(ROOT, "profiles"))):
            f = os.path.join(ROOT, "profiles", d, "pmc_traffic.json")
            if os.path.exists(f):
                t = json.load(open(f))
                for e in (t if isinstance(t, list) else [t]):  # (round 3: one entry per measured configuration)
                    if (e.get("kernel") == kernel and e.get("workload_bytes") == nbytes
                            and e.get("dist") == dist_name and e.get("config", "cfg2") == cfg):
                        if e.get("kernel_source_sha256") == now:  # counters of THIS device code only
                            best = (int(e["traffic_bytes"]), os.path.relpath(f, ROOT))
                        elif best[0] is None:
                            best = (None, f"{os.path.relpath(f, ROOT)} is of other device code "
                                          f"({str(e.get('kernel_source_sha256'))[:12]} != {now[:12]}): stale, not reported")
        return best
    except Exception:
        return (None, None)


# ---------------------------------------------------------------------------
# CPU baseline
# ---------------------------------------------------------------------------
def probe_genuine_wheel():
    """A genuine `ahocorasick_rs` (the Rust wheel) importable from OUTSIDE this repository?
    The repository ships its own package of that name (marked __acx_amd__): search with the
    repository's directories off sys.path and refuse anything that carries the marker."""
    import importlib
    import importlib.util
    saved_path, saved_mods = list(sys.path), {k: v for k, v in sys.modules.items() if k.startswith("ahocorasick_rs")}
    try:
        sys.path[:] = [p for p in sys.path if p not in ("", ".") and os.path.abspath(p) != ROOT
                       and not os.path.abspath(p).startswith(ROOT + os.sep)]
        for k in list(saved_mods):
            if not k.startswith("ahocorasick_rs_amd"):
                sys.modules.pop(k, None)
        spec = importlib.util.find_spec("ahocorasick_rs")
        if spec is None or (spec.origin and os.path.abspath(spec.origin).startswith(ROOT + os.sep)):
            return None
        mod = importlib.import_module("ahocorasick_rs")
        return None if getattr(mod, "__acx_amd__", False) else mod
    except Exception:
        return None
    finally:
        sys.path[:] = saved_path
        for k in [k for k in sys.modules if k.startswith("ahocorasick_rs") and not k.startswith("ahocorasick_rs_amd")]:
            sys.modules.pop(k, None)
        sys.modules.update(saved_mods)


def sha256_stream(arr) -> str:
    """SHA-256 of the canonical (pattern:u64, start:u64, end:u64) little-endian stream."""
    import numpy as np
    a = np.ascontiguousarray(arr, dtype="<u8").reshape(-1, 3)
    return hashlib.sha256(a.tobytes()).hexdigest()


def median_time(fn, warm=3, runs=7):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), ts


def oracle_all_cores(o, host, max_len, threads, overlapping):
    """The whole stream, exactly, with `threads` host threads (ctypes releases the GIL): ranges
    of the haystack with max_len - 1 bytes of overlap.  Overlapping searches: a range reports
    the occurrences that end in it.  Non-overlapping: a range reports the matches that start in
    it, scanned speculatively from its own start; a sequential pass then follows the carry (the
    end of the previous range's last match) and rescans the rare range whose carry differs."""
    import numpy as np
    from concurrent.futures import ThreadPoolExecutor
    n, m = len(host), max(max_len - 1, 0)
    cuts = [n * i // threads for i in range(threads + 1)]

    def pin(i):
        try:
            cpus = sorted(os.sched_getaffinity(0))
            os.sched_setaffinity(0, {cpus[i % len(cpus)]})
        except Exception:
            pass

    def scan(i, carry=None):
        lo, hi = cuts[i], cuts[i + 1]
        pin(i)
        if overlapping:
            w0 = max(0, lo - m)
            r = o.find_raw(host[w0:hi], overlapping=True)
            r[:, 1:] += w0
            return r[r[:, 2] > lo] if lo > 0 else r
        c = lo if carry is None else carry
        if c >= hi and i < threads - 1:
            return np.zeros((0, 3), np.uint64)
        r = o.find_raw(host[c:n if i == threads - 1 else min(n, hi + m)])
        r[:, 1:] += c
        return r if i == threads - 1 else r[r[:, 1] < hi]

    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(scan, range(threads)))
    if not overlapping:
        carry = 0
        for i in range(threads):
            lo, hi = cuts[i], cuts[i + 1]
            want = max(carry, lo)
            if want != lo:
                parts[i] = scan(i, want)
            carry = max(hi, want, int(parts[i][-1, 2]) if len(parts[i]) else 0)
    return np.concatenate(parts) if parts else np.zeros((0, 3), np.uint64)


def cpu_baseline(w, gpu_matches, sample_bytes):
    """The reference's algorithm on this box's host cores, on the very same haystack bytes.
    Ladder: a genuine `ahocorasick_rs` wheel if importable; else the oracle's C
    restatement (class map, one dependent u32 load per byte, special-state range check).
    1 core on a bounded prefix and all cores on the whole haystack; 3 warm-ups, median of 7;
    SHA-256 of the (u64,u64,u64) stream compared with the GPU's."""
    import numpy as np
    try:
        host = w["hay"].cpu().numpy()
        nbytes = len(host)
        mk, ov = w["mk"], w["overlapping"]
        ncpu = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
        sample = host[: min(sample_bytes, nbytes)]
        gpu_sha = None
        if gpu_matches is not None and not w["codepoints"]:
            gpu_sha = sha256_stream(np.stack([gpu_matches["pattern"], gpu_matches["start"], gpu_matches["end"]], 1))
        wheel = probe_genuine_wheel()
        if wheel is not None:
            kinds = [wheel.MatchKind.Standard, wheel.MatchKind.LeftmostFirst, wheel.MatchKind.LeftmostLongest]
            a = wheel.BytesAhoCorasick(w["patterns"], matchkind=kinds[mk],
                                       implementation=wheel.Implementation.DFA if w["cfg"] in ("cfg2", "cfg3") else None)
            buf = sample.tobytes()
            med, ts = median_time(lambda: a.find_matches_as_indexes(buf, overlapping=ov))
            full = a.find_matches_as_indexes(host.tobytes(), overlapping=ov)
            sha = sha256_stream(np.array(full, dtype=np.uint64).reshape(-1, 3))
            return {"value": round(len(sample) / med / 1e9, 4), "unit": "GB/s", "cores": 1, "kind": "reference",
                    "sample": f"genuine ahocorasick_rs wheel, first {len(sample) / GIB:g} GiB of the same haystack, "
                              f"3 warm-ups, median of 7 ({min(ts):.3f}-{max(ts):.3f} s)",
                    "host_cores_available": ncpu, "sha256_equal_gpu": None if gpu_sha is None else sha == gpu_sha}
        from oracle_lib import KIND_DFA, Oracle
        o = Oracle(w["patterns"], mk, KIND_DFA)
        max_len = max(len(p) for p in w["patterns"])
        one = (lambda: o.find_raw(sample, overlapping=True)) if ov else (lambda: o.count(sample))
        med1, ts1 = median_time(one)
        # (64 threads: measured on the 256-core box of round 3 -- 64 / 128 / 256 threads: 1.80 / 1.96 / 1.85 GB/s,
        # the leg does not scale beyond that on this host; ACX_CPU_BASELINE_THREADS overrides)
        threads = max(1, min(ncpu, int(os.environ.get("ACX_CPU_BASELINE_THREADS", "64"))))
        medn, tsn = median_time(lambda: oracle_all_cores(o, host, max_len, threads, ov), warm=1, runs=3)
        full = oracle_all_cores(o, host, max_len, threads, ov)
        res = {"value": round(len(sample) / med1 / 1e9, 4), "unit": "GB/s", "cores": 1, "kind": "port",
               "sample": f"CPU restatement of the reference algorithm (not the Rust binary): oracle DFA loop, first "
                         f"{len(sample) / GIB:g} GiB of the same haystack, 3 warm-ups, median of 7 "
                         f"({min(ts1):.3f}-{max(ts1):.3f} s)",
               "all_cores": {"value": round(nbytes / medn / 1e9, 4), "unit": "GB/s", "cores": threads,
                             "sample": f"whole {nbytes / GIB:g} GiB haystack in {threads} ranges with "
                                       f"{max_len - 1} bytes of overlap, threads pinned, 1 warm-up, median of 3 "
                                       f"({min(tsn):.3f}-{max(tsn):.3f} s)"},
               "host_cores_available": ncpu, "matches": int(len(full))}
        if gpu_sha is not None:
            res["sha256_equal_gpu"] = sha256_stream(full) == gpu_sha
        return res
    except Exception as e:  # the baseline must never take the GPU number down with it
        return {"value": None, "unit": "GB/s", "cores": 1, "kind": "port", "sample": f"failed: {e!r}"}


def main() -> None:
    args = parse_args()
    if args.gpus > 1 and "RANK" not in os.environ:
        sys.exit(self_launch(args))
    run(args)


if __name__ == "__main__":
    main()
