#!/usr/bin/env python
"""Static instruction counts of the gfx950 code of one csrc file, per kernel symbol and basic block.

    python tools/isa_counts.py conv3x3_ring.hip [--match ring16_kernel] [--blocks] [--asm FILE.s] [-D NAME=V ...]

Compiles the file for gfx950 with the flags of flairhip/build.py (device side only, to assembly; nothing is run) and
classifies every instruction as MFMA, other vector ALU, scalar (ALU and scalar loads), LDS, vector memory, or wait /
barrier (s_waitcnt, s_barrier, s_nop, s_sleep).  Per kernel it prints the resource lines of the metadata and three
regions found from the branch structure of the laid-out code:

    chunk loop   the innermost loop(s) that hold MFMAs (one pass = one 64-byte channel chunk of a ring kernel), and a
                 pass the compiler peeled off it: the MFMA column tells how many copies of the pass were counted
    tile loop    the outermost loop that holds MFMAs, without the chunk loop: what a block pays per tile --
                 tile bookkeeping and epilogue, every conditional block counted as taken
    outside      prologue and exit

and, with --blocks, every basic block.  It also lists the stores of the tile region in code order with the waits
between them (an epilogue that waits for memory between two stores of a tile shows here).  The counts are static:
a block that a launch never enters (an epilogue form's flag not set) still counts, so they bound the dynamic
counters of profiles/ from above for the tile region and match them in the chunk loop."""
from __future__ import annotations

import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flair-for-aigle_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc"]  # flairhip/build.py
CLASSES = ["mfma", "valu", "salu", "lds", "vmem", "wait"]
HEAD = {"mfma": "MFMA", "valu": "VALU", "salu": "SALU", "lds": "LDS", "vmem": "vec mem", "wait": "wait/bar"}


def classify(op: str) -> str | None:
    if op.startswith(("v_mfma", "v_smfmac")):
        return "mfma"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith(("s_waitcnt", "s_barrier", "s_nop", "s_sleep")):
        return "wait"
    if op.startswith("s_"):
        return "salu"
    return None


def is_store(op: str) -> bool:
    return op.startswith(("global_store", "buffer_store", "flat_store", "global_atomic", "buffer_atomic"))


class Block:
    def __init__(self, label: str):
        self.label = label
        self.n = collections.Counter()
        self.ops: list[tuple[str, str]] = []  # (opcode, operands)
        self.targets: list[str] = []


def parse(asm: str) -> dict[str, tuple[list[Block], dict[str, str]]]:
    """-> {symbol: (blocks in layout order, metadata)}"""
    kernels: dict[str, tuple[list[Block], dict[str, str]]] = {}
    cur: list[Block] | None = None
    name = None
    globl = set(re.findall(r"^\s*\.(?:globl|weak)\s+(\S+)", asm, re.M))
    for line in asm.splitlines():
        s = line.split(";")[0].strip()
        if not s:
            continue
        m = re.match(r"^([A-Za-z_.$][\w.$]*):$", s)
        if m:
            lab = m.group(1)
            if lab in globl and not lab.endswith(".kd"):
                name, cur = lab, [Block("entry")]
                kernels[name] = (cur, {})
            elif cur is not None and lab.startswith(".LBB"):
                cur.append(Block(lab))
            elif lab.startswith(".Lfunc_end"):
                cur = None
            continue
        if cur is None or s.startswith("."):
            continue
        parts = s.split(None, 1)
        op, rest = parts[0], (parts[1] if len(parts) > 1 else "")
        c = classify(op)
        if c is None:
            continue
        b = cur[-1]
        b.n[c] += 1
        b.ops.append((op, rest))
        if op.startswith(("s_cbranch", "s_branch")):
            b.targets.append(rest.strip())
    # metadata (YAML in the note section): the few resource lines
    for m in re.finditer(r"\.name:\s+(\S+)\n((?:\s+\.\w+:.*\n)+)", asm):
        if m.group(1) in kernels:
            kernels[m.group(1)][1].update(re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_count|sgpr_spill_count|"
                                                     r"group_segment_fixed_size|private_segment_fixed_size):\s+(\S+)",
                                                     m.group(2)))
    return kernels


def loops(blocks: list[Block]) -> list[tuple[int, int]]:
    """Back edges of the laid-out code as closed block intervals [head, latch]."""
    pos = {b.label: i for i, b in enumerate(blocks)}
    out = set()
    for i, b in enumerate(blocks):
        for t in b.targets:
            if t in pos and pos[t] <= i:
                out.add((pos[t], i))
    # merge the latches of one head
    by_head: dict[int, int] = {}
    for h, l in out:
        by_head[h] = max(l, by_head.get(h, l))
    return sorted(by_head.items())


def regions(blocks: list[Block]) -> tuple[set[int], set[int]]:
    """-> (blocks of the chunk loops, blocks of the tile loop without them)"""
    mf = [i for i, b in enumerate(blocks) if b.n["mfma"]]
    if not mf:
        return set(), set()
    with_mfma = [(h, l) for h, l in loops(blocks) if any(h <= i <= l for i in mf)]
    if not with_mfma:
        return set(mf), set()
    inner = [(h, l) for h, l in with_mfma
             if not any((h2, l2) != (h, l) and h <= h2 and l2 <= l for h2, l2 in with_mfma)]
    outer = min(h for h, _ in with_mfma), max(l for _, l in with_mfma)
    chunk = {i for h, l in inner for i in range(h, l + 1)}
    # a chunk pass the compiler peeled off the loop (the tile's last chunk): the span from its first to its last
    # MFMA block, laid out between the loop and the epilogue
    peeled = [i for i in mf if i not in chunk and outer[0] <= i <= outer[1]]
    if inner != [outer] and peeled:
        chunk |= set(range(min(peeled), max(peeled) + 1))
    tile = set(range(outer[0], outer[1] + 1)) - chunk
    return chunk, tile


def total(blocks: list[Block], idx) -> collections.Counter:
    n = collections.Counter()
    for i in idx:
        n.update(blocks[i].n)
    return n


def row(label: str, n: collections.Counter) -> str:
    return f"  {label:<34s}" + "".join(f"{n[c]:>9d}" for c in CLASSES)


def demangle(names: list[str]) -> dict[str, str]:
    for tool in ("c++filt", "llvm-cxxfilt"):
        try:
            out = subprocess.run([tool] + names, capture_output=True, text=True, check=True)
            return dict(zip(names, out.stdout.splitlines()))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}  # no demangler: --match then takes mangled text


def store_chain(blocks: list[Block], idx) -> tuple[int, int, list[str]]:
    """Vector stores and loads of a region in layout order with the vmcnt waits among them: (16-byte stores, vmcnt
    waits that stand between the first and the last 16-byte store, the chain as text).  Layout order is execution
    order for an epilogue whose conditional blocks only skip forward."""
    chain: list[tuple[str, str]] = []
    for i in sorted(idx):
        for op, rest in blocks[i].ops:
            if is_store(op):
                chain.append(("store16" if op.endswith("dwordx4") else "store", f"{blocks[i].label}: {op}"))
            elif op.startswith(("global_load", "buffer_load", "flat_load")):
                chain.append(("load", f"{blocks[i].label}:   {op}"))
            elif op == "s_waitcnt" and "vmcnt" in rest:
                chain.append(("wait", f"{blocks[i].label}:     s_waitcnt {rest}"))
    at = [k for k, (kind, _) in enumerate(chain) if kind == "store16"]
    waits_between = sum(1 for k, (kind, _) in enumerate(chain) if kind == "wait" and at and at[0] < k < at[-1])
    first = at[0] if at else len(chain)
    lead = [c for c in chain[:first] if c[0] != "load" or "_lds_" not in c[1]]
    return len(at), waits_between, [t for _, t in lead[-12:] + chain[first:]]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("source", help="file under csrc/ (or a path)")
    ap.add_argument("--match", default="", help="only kernels whose demangled name contains this")
    ap.add_argument("--blocks", action="store_true", help="print every basic block")
    ap.add_argument("--stores", action="store_true", help="print the store / wait chain of the tile region")
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("-D", action="append", default=[], metavar="NAME=V")
    args = ap.parse_args()

    if args.asm:
        asm = open(args.asm).read()
    else:
        src = args.source if os.path.exists(args.source) else os.path.join(CSRC, args.source)
        hipcc = os.environ.get("HIPCC") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc")
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "k.s")
            cmd = [hipcc] + FLAGS + [f"-D{d}" for d in args.D] + ["--cuda-device-only", "-S", src, "-o", out]
            proc = subprocess.run(cmd, capture_output=True, text=True)
            if proc.returncode != 0:
                sys.stderr.write(proc.stderr)
                return 1
            asm = open(out).read()

    kernels = parse(asm)
    pretty = demangle(list(kernels))
    for sym, (blocks, meta) in kernels.items():
        if args.match not in pretty[sym]:
            continue
        chunk, tile = regions(blocks)
        rest = set(range(len(blocks))) - chunk - tile
        nc, nt, nr = total(blocks, chunk), total(blocks, tile), total(blocks, rest)
        print(pretty[sym].replace("void ", "").split("(")[0])
        print("  " + "  ".join(f"{k} {v}" for k, v in sorted(meta.items())))
        print(f"  {'region':<34s}" + "".join(f"{HEAD[c]:>9s}" for c in CLASSES))
        print(row(f"chunk loop ({len(chunk)} blocks)", nc))
        print(row(f"tile loop, rest ({len(tile)} blocks)", nt))
        print(row(f"outside ({len(rest)} blocks)", nr))
        if nc["mfma"]:
            print(f"  chunk loop per MFMA: VALU {nc['valu'] / nc['mfma']:.2f}  SALU {nc['salu'] / nc['mfma']:.2f}  "
                  f"LDS {nc['lds'] / nc['mfma']:.2f}  wait/bar {nc['wait'] / nc['mfma']:.2f}")
        ns, nw, chain = store_chain(blocks, tile)
        print(f"  tile region: {ns} 16-byte stores, {nw} vmcnt waits between the first and the last of them")
        if args.stores:
            for c in chain:
                print("      " + c)
        if args.blocks:
            for i, b in enumerate(blocks):
                where = "chunk" if i in chunk else ("tile" if i in tile else "")
                print(row(f"  {b.label} {where}", b.n))
        print()
    return 0


if __name__ == "__main__":
    sys.exit(main())
