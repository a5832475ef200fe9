#!/usr/bin/env python3
"""Static instruction accounting of one k1b_prefilter instantiation (no GPU needed).

Cross-compiles ahocorasick_rs_amd/csrc/kernels.hip to gfx950 assembly with the library's own flags
(ahocorasick_rs_amd/_build.py), isolates one instantiation and prints

  * its .vgpr_count, .sgpr_count, spill counts and scratch size (the code object's metadata),
  * its instruction totals by opcode class (v_*, s_*, ds_*, global_*, other),
  * the same totals for the INTERIOR PATH of the tile loop.

The interior path is defined on the control-flow graph, not by looking for particular instructions:
the tile loop is the loop that contains the most level-1 blocks (the blocks with eight or more LDS
instructions, a row's table reads: by opcode class, no particular instruction is looked for; of two
such loops the larger); inner loops run their header once (back edges are cut); of
all paths from the loop header through every level-1 block to the back edge, the path with the
fewest vector-ALU instructions is taken (ties: fewest instructions).  That is the iteration of a
wave whose tile is interior (the boundary masking is a wave-uniform branch with more work behind it,
so the cheapest path is the one taken when `interior` is true), whose level-1 masks are empty after
the first compaction round and whose level-2 stages hold nothing: everything every tile pays.  What
survivors add (level 2, per batch) is not on it.  Where the compiler guards a block with a flag it set
in an earlier block instead of branching twice, the cheapest path may pass the guard on the cheap side
of both (the tile prefetch's address arithmetic, half a dozen instructions, is such a block): the
figure is a lower bound, and the same one on both sides of a comparison.  It is NOT the per-tile-wave
instruction count a counter run gives (485 VALU on the parent), which includes level 2.

usage: tools/k1b_isa_count.py [--q 5] [--slots 1] [--cp 0] [--big 0] [--sh 0] [--all]
                              [--source kernels.hip] [--asm kernels.s] [--blocks]
"""
from __future__ import annotations

import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "ahocorasick_rs_amd", "csrc", "kernels.hip")
CLASSES = ("v_", "s_", "ds_", "global_", "other")
# the instantiations launch_prefilter picks for: the headline (bytes API, sparse mode), the str API, a set with
# 1- and 2-byte patterns, a saturated level-1 table, a table that passes nearly every position
NAMED = [("headline", (5, 1, 0, 0, 0)), ("CP", (5, 1, 1, 0, 0)), ("SH", (5, 1, 0, 0, 1)),
         ("BIG", (5, 1, 0, 1, 0)), ("STAGED", (5, 1, 0, 2, 0)),
         # ... and for shorter shortest patterns, with and without the side test; region mode (the dense path)
         ("Q4", (4, 1, 0, 0, 0)), ("Q3", (3, 1, 0, 0, 0)), ("Q4 SH", (4, 1, 0, 0, 1)), ("Q3 SH", (3, 1, 0, 0, 1)),
         ("region", (5, 0, 0, 0, 0))]


def compile_asm(source: str, out: str) -> None:
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.dirname(SOURCE), "-o", out, source]
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    if r.returncode:
        sys.stderr.write(r.stderr)
        raise SystemExit("the compile failed: " + " ".join(cmd))


def opclass(mn: str) -> str:
    for c in CLASSES[:-1]:
        if mn.startswith(c):
            return c
    return "other"


def symbol_of(q, slots, cp, big, sh) -> str:
    return "k1b_prefilterILi%dELb%dELb%dELi%dELb%dEE" % (q, slots, cp, big, sh)


def function_lines(asm: list[str], key: str) -> tuple[str, list[str]]:
    start = None
    for i, ln in enumerate(asm):
        if start is None:
            if ln.startswith("_Z") and key in ln.split(":")[0] and ln.rstrip().split(";")[0].rstrip().endswith(":"):
                start, name = i, ln.split(":")[0]
        elif ln.startswith(".Lfunc_end"):
            return name, asm[start + 1:i]
    raise SystemExit("no function with %s in the assembly" % key)


def metadata(asm: list[str], name: str) -> dict:
    # one entry per kernel, its keys in alphabetical order: .args first, .group_segment_fixed_size before .name
    out, cur, mine = {}, {}, False
    for ln in asm:
        s = ln.strip()
        if s.startswith("- .args:") or s.startswith("- .agpr_count:"):
            if mine:
                break
            cur = {}
        elif s.startswith(".name:"):
            mine = s.split(":", 1)[1].strip() == name
        else:
            m = re.match(r"\.(private_segment_fixed_size|sgpr_count|sgpr_spill_count|vgpr_count|vgpr_spill_count"
                         r"|group_segment_fixed_size):\s+(\d+)", s)
            if m:
                cur[m.group(1)] = int(m.group(2))
        if mine:
            out = cur
    return out


class Block:
    def __init__(self, label):
        self.label, self.ops, self.succ = label, [], []

    def count(self) -> Counter:
        return Counter(opclass(m) for m in self.ops)


def build_cfg(lines: list[str]) -> list[Block]:
    blocks, cur, targets = [Block("entry")], None, []
    cur = blocks[0]
    fall = True
    for ln in lines:
        code = ln.split(";")[0].rstrip()
        if not code.strip():
            continue
        if not code[0].isspace():  # a label
            m = re.match(r"(\.?\w+):", code)
            if not m:
                continue
            nb = Block(m.group(1))
            if fall:
                cur.succ.append(nb.label)
            blocks.append(nb)
            cur, fall = nb, True
            continue
        tok = code.split()
        mn = tok[0]
        if mn.startswith("."):
            continue
        if not fall:  # code behind an unconditional branch without a label: its own (unreachable) block
            cur = Block("anon%d" % len(blocks))
            blocks.append(cur)
            fall = True
        cur.ops.append(mn)
        if mn == "s_branch":
            cur.succ.append(tok[1])
            fall = False
        elif mn.startswith("s_cbranch"):
            nb = Block("ft%d" % len(blocks))
            cur.succ += [tok[1], nb.label]
            blocks.append(nb)
            cur = nb
        elif mn in ("s_endpgm", "s_setpc_b64"):
            fall = False
    return blocks


def interior_path(blocks: list[Block]):
    by = {b.label: b for b in blocks}
    order = {b.label: i for i, b in enumerate(blocks)}
    # back edges by an iterative depth-first search from the entry
    state, back, stack = {}, set(), [(blocks[0].label, 0)]
    state[blocks[0].label] = 1
    while stack:
        lab, i = stack.pop()
        succ = by[lab].succ
        if i < len(succ):
            stack.append((lab, i + 1))
            t = succ[i]
            if state.get(t, 0) == 1:
                back.add((lab, t))
            elif state.get(t, 0) == 0:
                state[t] = 1
                stack.append((t, 0))
        else:
            state[lab] = 2
    level1 = [b.label for b in blocks if b.count()["ds_"] >= 8]
    if not level1:
        raise SystemExit("no level-1 block found")
    pred = {b.label: [] for b in blocks}
    for b in blocks:
        for t in b.succ:
            pred[t].append(b.label)

    def natural_loop(header, latches):
        body, work = {header}, [l for l in latches]
        while work:
            n = work.pop()
            if n in body:
                continue
            body.add(n)
            work += pred[n]
        return body

    best = None
    for h in {t for _, t in back}:
        latches = [s for s, t in back if t == h]
        body = natural_loop(h, latches)
        inside = sum(1 for l in level1 if l in body)  # (the copy of the table into LDS is such a block too, in a loop of its own)
        if inside and (best is None or (inside, len(body)) > (best[3], len(best[1]))):
            best = (h, body, latches, inside)
    if best is None:
        raise SystemExit("no loop holds a level-1 block")
    header, body, latches, _ = best
    level1 = [l for l in level1 if l in body]
    # the loop as a DAG (back edges cut), in topological order
    succ = {n: [t for t in by[n].succ if t in body and (n, t) not in back] for n in body}
    indeg = Counter(t for n in body for t in succ[n])
    topo, ready = [], [n for n in body if indeg[n] == 0]
    while ready:
        ready.sort(key=lambda n: order[n])
        n = ready.pop(0)
        topo.append(n)
        for t in succ[n]:
            indeg[t] -= 1
            if indeg[t] == 0:
                ready.append(t)
    pos = {n: i for i, n in enumerate(topo)}
    cost = {n: (by[n].count()["v_"], len(by[n].ops)) for n in body}
    stops = [header] + sorted(set(level1) - {header}, key=lambda n: pos[n])
    INF = (10 ** 9, 10 ** 9)

    def cheapest(src, dsts):
        dist, via = {src: (0, 0)}, {}
        for n in topo[pos[src]:]:
            if n not in dist:
                continue
            for t in succ[n]:
                d = (dist[n][0] + cost[t][0], dist[n][1] + cost[t][1])
                if d < dist.get(t, INF):
                    dist[t], via[t] = d, n
        d = min(dsts, key=lambda n: dist.get(n, INF))
        if d not in dist:
            raise SystemExit("no path from %s to %s" % (src, dsts))
        path = [d]
        while path[-1] != src:
            path.append(via[path[-1]])
        return path[::-1]

    path = [header]
    for a, b in zip(stops, stops[1:]):
        path += cheapest(a, [b])[1:]
    if path[-1] not in latches:
        path += cheapest(path[-1], latches)[1:]
    return header, len(body), [by[n] for n in path], level1


def fmt(c: Counter) -> str:
    return "  ".join("%s %5d" % (k.rstrip("_") if k != "other" else k, c[k]) for k in CLASSES) + "   total %5d" % sum(c.values())


def report(asm: list[str], tag: str, inst, show_blocks: bool) -> None:
    name, lines = function_lines(asm, symbol_of(*inst))
    md = metadata(asm, name)
    blocks = build_cfg(lines)
    total = Counter()
    for b in blocks:
        total += b.count()
    header, nbody, path, level1 = interior_path(blocks)
    inner = Counter()
    for b in path:
        inner += b.count()
    print("%s: k1b_prefilter<Q=%d, SLOTS=%d, CP=%d, BIGV=%d, SH=%d>" % ((tag,) + tuple(inst)))
    print("  vgpr_count %d  sgpr_count %d  vgpr_spill %d  sgpr_spill %d  scratch %d B  lds %d B" % (
        md.get("vgpr_count", -1), md.get("sgpr_count", -1), md.get("vgpr_spill_count", -1),
        md.get("sgpr_spill_count", -1), md.get("private_segment_fixed_size", -1), md.get("group_segment_fixed_size", -1)))
    print("  kernel         %s" % fmt(total))
    print("  interior path  %s   (%d of the loop's %d blocks, %d level-1 blocks, header %s)" % (
        fmt(inner), len(path), nbody, len(level1), header))
    if show_blocks:
        for b in path:
            print("    %-12s %s" % (b.label, fmt(b.count())))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--q", type=int, default=5)
    ap.add_argument("--slots", type=int, default=1)
    ap.add_argument("--cp", type=int, default=0)
    ap.add_argument("--big", type=int, default=0)
    ap.add_argument("--sh", type=int, default=0)
    ap.add_argument("--all", action="store_true", help="the ten instantiations of NAMED: headline, CP, SH, BIG, STAGED, Q4, Q3, Q4 SH, Q3 SH, region")
    ap.add_argument("--source", default=SOURCE, help="the kernel source to compile (default: the tree's)")
    ap.add_argument("--asm", help="an assembly file compiled earlier (skips the compile)")
    ap.add_argument("--blocks", action="store_true", help="list the blocks of the interior path")
    a = ap.parse_args()
    if a.asm:
        asm = open(a.asm).read().split("\n")
    else:
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, "kernels.s")
            compile_asm(a.source, out)
            asm = open(out).read().split("\n")
    insts = NAMED if a.all else [("selected", (a.q, a.slots, a.cp, a.big, a.sh))]
    for tag, inst in insts:
        report(asm, tag, inst, a.blocks)


if __name__ == "__main__":
    sys.exit(main())
