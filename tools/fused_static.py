#!/usr/bin/env python3
"""Static evidence for the fused launches of the split learner (csrc/fsplit.hip: forward_kernel, backward_kernel), CPU only.

usage: tools/fused_static.py [TREE] > profiles/r15_fused_launches_static.txt

fsplit.hip of TREE (default: this checkout) is compiled with the Makefile's flags plus `--cuda-device-only -S` (tools/isa_diff.py's
command). Printed: per kernel the VGPR count, scratch and LDS bytes of its descriptor and the number of flat_ instructions (an LDS
pointer that lost its address space would show as flat loads); then, for each fused kernel, its loops in program order beside the loops
of the stand-alone kernels whose bodies it runs, in the same order: instructions and MFMAs per loop, and which mnemonics occur a
different number of times once waits, s_nop and register moves are left out (none: the tile loop holds the same instructions). A tile
loop is a top-level loop with MFMAs in it."""
import collections
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_diff import FLAGS, HIPCC, PER_FILE  # noqa: E402
from startup_static import demangle  # noqa: E402

NAME = "fsplit.hip"
SKIP = re.compile(r"^(s_waitcnt|s_nop|v_mov_b32|v_mov_b64|s_mov_b32|s_mov_b64|v_accvgpr_\w+|v_pk_mov_b32)$")
PHASES = {
    "forward_kernel<{S}>": ["head_kernel<{S}, ActorS, 0, false>", "head_kernel<{S}, CriticS, 1, false>", "head_kernel<{S}, ActorS, 6, false>",
                            "head_kernel<{S}, CriticS, 5, false>", "actor_seed_kernel"],
    "backward_kernel<{S}>": ["dw_kernel<{S}, CriticS>", "dx_kernel<{S}, CriticS>", "dxa_kernel<{S}>", "dw_kernel<{S}, ActorS>", "dx_kernel<{S}, ActorS>"],
}


def kernels(tree):
    out = os.path.join(tempfile.mkdtemp(prefix="fused_static_"), "fsplit.s")
    cmd = [HIPCC, *FLAGS, *PER_FILE[NAME], "--cuda-device-only", "-S", "-x", "hip", NAME, "-o", out]
    r = subprocess.run(cmd, cwd=os.path.join(tree, "avddpg_amd", "csrc"), capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stderr)
    text = open(out).read()
    bodies, meta, cur = {}, {}, None
    for l in text.split("\n"):
        m = re.match(r"^(_Z\w+):", l)
        if m:
            cur = m.group(1)
            bodies[cur] = []
        elif l.startswith("\t.end_amdhsa_kernel") or l.startswith(".Lfunc_end"):
            cur = None if l.startswith(".Lfunc_end") else cur
        elif cur is not None:
            bodies[cur].append(l)
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)", text, re.S):
        meta[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgpr=int(m.group(4)))
    names = demangle([n for n in bodies if n in meta])
    return {names[n]: (bodies[n], meta[n]) for n in names}


def loops(body):
    """Top-level loops in program order (the blocks the assembler marks as inside them): [Counter of mnemonics]."""
    out = []
    for i, l in enumerate(body):
        m = re.match(r"^\.L(BB\d+_\d+):.*This (Inner )?Loop Header: Depth=1", l)
        if not m:
            continue
        end = i + 1  # the loop's blocks: up to the first label that is not marked as inside this loop
        while end < len(body) and not (re.match(r"^\.LBB\d+_\d+:", body[end]) and f"Header={m.group(1)} " not in body[end]):
            end += 1
        ins = [x.split()[0] for x in body[i + 1:end] if re.match(r"^\s+[a-z]", x) and not x.lstrip().startswith((".", ";"))]
        out.append(collections.Counter(ins))
    return out


def main():
    tree = sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ks = kernels(tree)
    print("kernel                                              vgpr scratch     lds  flat_")
    for n, (body, m) in sorted(ks.items()):
        if "front" in n or "prep" in n:
            continue
        flat = sum(1 for l in body if re.match(r"\s+flat_", l))
        print(f"{n[:50]:50s} {m['vgpr']:5d} {m['scratch']:7d} {m['lds']:7d} {flat:6d}")
    core = lambda c: collections.Counter({k: v for k, v in c.items() if not SKIP.match(k)})
    mf = lambda c: sum(v for k, v in c.items() if k.startswith("v_mfma"))
    for S in ("4", "3"):
        for fused, parts in PHASES.items():
            fused = fused.format(S=S)
            mine = [c for c in loops(ks[fused][0]) if mf(c)]  # the tile loops: those with MFMAs (the seed's and the start-up loops have none)
            ref = [(p.format(S=S), c) for p in parts for c in loops(ks[p.format(S=S)][0]) if mf(c)]
            print(f"\n{fused}: {len(mine)} tile loops; its phases' stand-alone kernels: {len(ref)} tile loops")
            print(f"  LDS {ks[fused][1]['lds']} B = largest phase {max(ks[p.format(S=S)][1]['lds'] for p in parts)} B")
            for i in range(max(len(mine), len(ref))):
                a = mine[i] if i < len(mine) else None
                who, b = ref[i] if i < len(ref) else ("-", None)
                if a is None or b is None:
                    print(f"  loop {i}: {who}: no counterpart")
                    continue
                d = {k: (core(a)[k], core(b)[k]) for k in set(core(a)) | set(core(b)) if core(a)[k] != core(b)[k]}
                print(f"  loop {i} {who[:38]:38s} fused {sum(a.values()):5d} instr {mf(a):4d} MFMA | stand-alone {sum(b.values()):5d} instr {mf(b):4d} MFMA | "
                      f"{'same mnemonic counts (waits, s_nop, moves aside)' if not d else 'DIFFERENT (fused, stand-alone): ' + str(dict(sorted(d.items())))}")


if __name__ == "__main__":
    main()
