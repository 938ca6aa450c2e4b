#!/usr/bin/env python3
"""gfx950 assembly of csrc files in two source trees, compared text for text (CPU only: no GPU is needed).

usage: tools/isa_diff.py [-j N] [--keep DIR] [--common] TREE_A TREE_B file.hip [file.hip ...]

Each TREE holds avddpg_amd/csrc and include/ (a checkout, or `git archive <commit> avddpg_amd/csrc include | tar -x -C DIR`).
Every file is compiled in both trees with the Makefile's flags plus `--cuda-device-only -S`, once plain and once with -DAVD_DIAG.
Comment lines, `.file` / `.loc` / `.ident` and the per-compilation `__hip_cuid_*` symbol are dropped; what remains -- every
instruction, every kernel descriptor and the metadata with each kernel's .vgpr_count / .sgpr_count / .private_segment_fixed_size /
.group_segment_fixed_size -- must be byte-identical. Prints one line per (file, build) with the kernel count and the largest
register / scratch / LDS figures, a unified diff where the trees differ, and exits non-zero on any difference: identical text is
the same bits and the same speed, so a refactor that passes needs no timing run for these kernels.

--common: for a change that ADDS kernels to a file. The text is compared kernel by kernel over the kernels both trees have -- each
kernel's instructions from its label to the end of its descriptor, and its metadata entry (registers, scratch, LDS, arguments) --
with the function numbers in local labels (.LBB<n>_, .Lfunc_end<n>) dropped, since a kernel emitted in front shifts them. Kernels
that only one tree has are listed with their resource figures and are not a difference."""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = "-O3 -fPIC -fvisibility=hidden --offload-arch=gfx950 -std=c++17 -Wall -Wno-unused-function".split()
PER_FILE = {"wide.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form"], "fset.hip": ["-fno-honor-nans"],
            "fsplit.hip": ["-fno-honor-nans", "-fno-slp-vectorize"]}  # (csrc/Makefile's per-file FLAGS)
DROP = re.compile(r"^\s*(;|\.file\b|\.loc\b|\.ident\b)|__hip_cuid_")


def assembly(tree, name, diag, out):
    cmd = [HIPCC, *FLAGS, *PER_FILE.get(name, []), *(["-DAVD_DIAG"] if diag else []), "--cuda-device-only", "-S", "-x", "hip", name, "-o", out]
    r = subprocess.run(cmd, cwd=os.path.join(tree, "avddpg_amd", "csrc"), capture_output=True, text=True)
    if r.returncode:
        sys.exit(f"{tree}: {' '.join(cmd)} failed\n{r.stderr}")
    with open(out) as f:
        return [l for l in f if l.strip() and not DROP.search(l)]


def kernels(lines):
    """{kernel name: its text (label .. .end_amdhsa_kernel) + its metadata entry}, local labels without their function number"""
    norm = lambda l: re.sub(r"\.(LBB|Lfunc_end|Lfunc_begin|Ltmp)\d+", r".\1", re.sub(r"\s*;.*$", "", l))  # (and trailing comments)
    names = [l.split()[1] for l in lines if l.lstrip().startswith(".amdhsa_kernel ")]
    out = {}
    for n in names:
        i = next(k for k, l in enumerate(lines) if l.startswith(n + ":"))
        j = next(k for k in range(i, len(lines)) if lines[k].lstrip().startswith(".end_amdhsa_kernel"))
        out[n] = [norm(l) for l in lines[i:j + 1]]
    entry = None
    for l in lines[next((k for k, l in enumerate(lines) if l.startswith("amdhsa.kernels:")), len(lines)) + 1:]:
        if l.startswith("  - "):
            entry = []
        elif not l.startswith("    "):
            break
        entry.append(l)
        m = re.match(r"\s+\.name:\s+(\S+)", l)
        if m and m.group(1) in out:
            out[m.group(1)].append(entry)
    return {n: [x for part in v for x in (part if isinstance(part, list) else [part])] for n, v in out.items()}


def summary(lines):
    top = lambda key: max([int(m.group(1)) for l in lines for m in [re.match(rf"\s*\.{key}:\s+(\d+)", l)] if m], default=0)
    return (f"{sum(1 for l in lines if l.lstrip().startswith('.amdhsa_kernel '))} kernels, max vgpr {top('vgpr_count')} sgpr {top('sgpr_count')} "
            f"scratch {top('private_segment_fixed_size')} lds {top('group_segment_fixed_size')}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-j", type=int, default=8, help="compilations in flight")
    ap.add_argument("--keep", help="leave the raw .s files in this directory")
    ap.add_argument("--common", action="store_true", help="compare kernel by kernel over the kernels both trees have")
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("files", nargs="+")
    a = ap.parse_args()
    tmp = a.keep or tempfile.mkdtemp(prefix="isa_diff_")
    os.makedirs(tmp, exist_ok=True)
    jobs = [(f, d) for f in a.files for d in (False, True)]
    with ThreadPoolExecutor(a.j) as ex:
        fut = {(f, d, side): ex.submit(assembly, os.path.abspath(tree), f, d, os.path.join(tmp, f"{side}_{f}{'_diag' if d else ''}.s"))
               for f, d in jobs for side, tree in (("a", a.tree_a), ("b", a.tree_b))}
    bad = 0
    for f, d in jobs:
        la, lb = fut[f, d, "a"].result(), fut[f, d, "b"].result()
        if a.common:
            ka, kb = kernels(la), kernels(lb)
            for n in sorted(set(ka) ^ set(kb)):
                print(f"{f:12s} {'-DAVD_DIAG' if d else 'plain':10s} only in {'a' if n in ka else 'b'}: {n}  {summary((ka.get(n) or kb[n]))}")
            both = sorted(set(ka) & set(kb))
            la, lb = [l for n in both for l in ka[n]], [l for n in both for l in kb[n]]
        same = la == lb
        bad += not same
        print(f"{f:12s} {'-DAVD_DIAG' if d else 'plain':10s} {'IDENTICAL' if same else 'DIFFERENT'}  {len(la)} / {len(lb)} lines  a: {summary(la)}"
              + ("" if same else f"  b: {summary(lb)}"))
        if not same:
            sys.stdout.writelines(difflib.unified_diff(la, lb, f"a/{f}", f"b/{f}", n=2))
    print(f"{len(jobs) - bad} of {len(jobs)} identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
