#!/usr/bin/env python3
"""Static evidence for the start-up of the split learner's kernels (csrc/fsplit.hip), two source trees side by side (CPU only).

usage: tools/startup_static.py TREE_A TREE_B > profiles/r14_startup_static.txt

Each TREE holds avddpg_amd/csrc and include/ (a checkout, or `git archive <commit> avddpg_amd/csrc include | tar -x -C DIR`). fsplit.hip
is compiled in both with the Makefile's flags plus `--cuda-device-only -S` (tools/isa_diff.py's command), and per kernel this prints
  * the VGPR count and the scratch bytes of the kernel descriptor (.vgpr_count, .private_segment_fixed_size);
  * how many vector-memory loads are issued before the first `s_waitcnt vmcnt` (what is in flight together at the first wait), and how
    many loads and `vmcnt` waits stand in front of the first `s_barrier`;
  * the part from the first MFMA on -- the tile loop and what follows it: whether its mnemonic sequence is the same in both trees
    (operands are not compared: the prologue change renumbers registers), and if not, how many instructions stand at another place
    and which mnemonics occur a different number of times (none: the scheduler ordered one set of instructions differently).
Only load, wait, barrier and MFMA mnemonics are looked at by name."""
import collections
import difflib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_diff import FLAGS, HIPCC, PER_FILE  # noqa: E402

NAME = "fsplit.hip"
LOAD = re.compile(r"^(global|buffer|flat)_load")


def demangle(names):
    for tool in ("/opt/rocm/lib/llvm/bin/llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool, *names], capture_output=True, text=True, check=True).stdout.split("\n")
            return {n: re.sub(r"^void |avd::fsplit::|\(.*", "", d) for n, d in zip(names, out)}
        except Exception:
            pass
    return {n: n for n in names}


def kernels(tree, out):
    cmd = [HIPCC, *FLAGS, *PER_FILE[NAME], "--cuda-device-only", "-S", "-x", "hip", NAME, "-o", out]
    r = subprocess.run(cmd, cwd=os.path.join(os.path.abspath(tree), "avddpg_amd", "csrc"), capture_output=True, text=True)
    if r.returncode:
        sys.exit(f"{tree}: {' '.join(cmd)} failed\n{r.stderr}")
    ops, meta, cur, mname = {}, {}, None, None
    for l in open(out):
        m = re.match(r"^(_Z\w+):", l)
        if m:
            cur = m.group(1)
            ops[cur] = []
            continue
        m = re.match(r"\s*\.name:\s+(_Z\w+)", l)
        if m:
            mname = m.group(1)
        m = re.match(r"\s*\.(vgpr_count|private_segment_fixed_size):\s+(\d+)", l)
        if m and mname:
            meta.setdefault(mname, {})[m.group(1)] = int(m.group(2))
        if cur is None or not l.startswith("\t") or l.lstrip().startswith((";", ".")):
            if cur is not None and re.match(r"^\.Lfunc_end", l):
                cur = None
            continue
        ops[cur].append(l.split()[0] + (" vmcnt" if l.split()[0] == "s_waitcnt" and "vmcnt" in l else ""))
    return {k: v for k, v in ops.items() if k in meta}, meta


def start_up(seq):
    first_wait = next((i for i, o in enumerate(seq) if o == "s_waitcnt vmcnt"), len(seq))
    barrier = next((i for i, o in enumerate(seq) if o == "s_barrier"), len(seq))
    n = lambda lo, hi, f: sum(1 for o in seq[lo:hi] if f(o))
    return (n(0, first_wait, lambda o: LOAD.match(o)), n(0, barrier, lambda o: LOAD.match(o)), n(0, barrier, lambda o: o == "s_waitcnt vmcnt"))


def body(seq):
    first = next((i for i, o in enumerate(seq) if o.startswith("v_mfma")), len(seq))
    return seq[first:]


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    tmp = tempfile.mkdtemp(prefix="startup_static_")
    (oa, ma), (ob, mb) = kernels(sys.argv[1], os.path.join(tmp, "a.s")), kernels(sys.argv[2], os.path.join(tmp, "b.s"))
    names = demangle(sorted(oa))
    print("# kernel: vgpr a -> b, scratch a -> b | loads in flight at the first vmcnt wait a -> b | loads / vmcnt waits before the first "
          "s_barrier a -> b | from the first MFMA on")
    for k in sorted(oa, key=lambda k: names[k]):
        if k not in ob:
            continue
        a, b = oa[k], ob[k]
        sa, sb = start_up(a), start_up(b)
        ba, bb = body(a), body(b)
        if not ba:
            tail = "no MFMA; whole sequence " + ("identical" if a == b else "differs")
        elif ba == bb:
            tail = f"{len(ba)} instructions, {sum(o.startswith('v_mfma') for o in ba)} MFMA: mnemonic sequence identical"
        else:
            moved = sum(max(i2 - i1, j2 - j1) for t, i1, i2, j1, j2 in difflib.SequenceMatcher(None, ba, bb, autojunk=False).get_opcodes() if t != "equal")
            ca, cb = collections.Counter(ba), collections.Counter(bb)
            diff = ", ".join(f"{m} {ca[m]} -> {cb[m]}" for m in sorted(set(ca) | set(cb)) if ca[m] != cb[m])
            tail = (f"{len(ba)} -> {len(bb)} instructions, {sum(o.startswith('v_mfma') for o in ba)} -> {sum(o.startswith('v_mfma') for o in bb)} MFMA: "
                    f"{moved} at another place; counts that differ: {diff or 'none (one set of instructions, ordered differently)'}")
        print(f"{names[k]:44s} vgpr {ma[k]['vgpr_count']:3d} -> {mb[k]['vgpr_count']:3d}  scratch {ma[k]['private_segment_fixed_size']} -> "
              f"{mb[k]['private_segment_fixed_size']} | first wait {sa[0]:2d} -> {sb[0]:2d} | before barrier {sa[1]:2d} loads / {sa[2]:2d} waits -> "
              f"{sb[1]:2d} / {sb[2]:2d} | {tail}")


if __name__ == "__main__":
    main()
