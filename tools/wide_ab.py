#!/usr/bin/env python3
"""A/B of the shared-set learner's HOST code (csrc/wide.hip) between two builds of the library: same launches, same values.

usage: tools/wide_ab.py PARENT_LIB_DIR [--out FILE] [--repeats 8] [--no-trace]

PARENT_LIB_DIR holds libavddpg_hip.so and libavddpg_hip_diag.so of the tree to compare against (`git archive <commit> avddpg_amd/csrc
include | tar -x -C DIR`, `make -C DIR/avddpg_amd/csrc all diag`, then DIR/avddpg_amd/lib); this tree's two libraries are the other
side. Every (case, side) runs in a fresh child process that loads its library through AVDDPG_HIP_LIB, under `rocprofv3 --kernel-trace`:
one warm-up call, a marker kernel, then `repeats` calls on the same inputs.
 * launch sequence: the ordered (kernel name, grid, workgroup, LDS bytes) list of the first call after the marker, memset / copy
   kernels of the runtime included where the trace shows them, must be identical on both sides;
 * values: the learner accumulates with f32 atomics, so two builds cannot be compared bit for bit. The yardstick is the parent's own
   repeat-to-repeat spread (max |delta| per slab over the slab's max, as tools/determinism_c5.py); this tree against the parent,
   measured the same way, must be zero or at most twice that spread (both are maxima of a few draws of the same summation-order
   noise). avd_actor_forward_shared_bf16 has no atomics: bit equality.
Prints the report (and writes it to --out); exit status 1 on any difference."""
import argparse
import csv
import glob
import hashlib
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W1024 = dict(actor_layer1_size=1024, actor_layer2_size=1024, critic_layer1_size=1024, critic_layer2_size=1024)
# (name, Config widths, rows per set (learn) or agents per set (act), library, environment): two weight sets, S = 4
CASES = [
    ("learn 256/128/48, 384 rows", {}, 384, "product", {}),
    ("learn 1024/1024/48, 192 rows", W1024, 192, "product", {}),
    ("learn 1024/1024/48, 768 rows", W1024, 768, "product", {}),
    ("learn 1024/1024/48, 960 rows", W1024, 960, "product", {}),
    ("learn 1024/1024/48, 768 rows, AVD_WIDE_DUAL=0", W1024, 768, "diagnostic", {"AVD_WIDE_DUAL": "0"}),
    ("learn 1024/1024/48, 768 rows, AVD_WIDE_FUSED_DELTA=0", W1024, 768, "diagnostic", {"AVD_WIDE_FUSED_DELTA": "0"}),
    ("learn 1024/1024/48, 768 rows, AVD_WIDE_FUSED_FWD=0", W1024, 768, "diagnostic", {"AVD_WIDE_FUSED_FWD": "0"}),
    ("act 1024/1024/48, 12 agents per set", W1024, 12, "product", {}),
]
LIB = {"product": "libavddpg_hip.so", "diagnostic": "libavddpg_hip_diag.so"}
MARKER, LAST = "sin_kernel", {"learn": "losses_kernel", "act": "tanh_rows_kernel"}


def child(index, out, repeats):
    """One side of one case, in this process: [repeats][values] -> out (.npy), path flags on stdout where the library has the query."""
    import ctypes

    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from avddpg_amd import _hip
    from tests.gpu_util import t
    from tests.test_gpu_mlp import _perturbed_group

    name, widths, rows, _, _ = CASES[index]
    n_sets, S = 2, 4
    conf, grp = _perturbed_group(n_sets, S=S, seed=91, **widths)
    rs = np.random.RandomState(92)
    marker = lambda: (torch.cuda.synchronize(), torch.zeros(4096, device="cuda").sin_(), torch.cuda.synchronize())
    if name.startswith("act"):
        x = t(rs.normal(0, 1.5, size=(n_sets, rows, S)).astype(np.float32))
        run = lambda: grp.actor_shared(x, n_sets * rows).clone().reshape(-1)
    else:
        s, s2 = (t(rs.normal(0, 1.5, size=(n_sets, rows, S)).astype(np.float32)) for _ in range(2))
        a = t(rs.uniform(-2.5, 2.5, size=(n_sets, rows, 1)).astype(np.float32))
        r = t(-np.abs(rs.normal(0, 0.3, size=(n_sets, rows))).astype(np.float32))
        losses = torch.zeros(n_sets, 2, device="cuda")
        run = lambda: torch.cat([grp.learn_shared(s, a, r, s2, n_sets * rows // 64, losses=losses).reshape(-1), losses.reshape(-1)]).clone()
        if getattr(_hip.lib(), "avd_learn_shared_path", None) is not None:
            flags = ctypes.c_uint(0)
            _hip.call("avd_learn_shared_path", grp._layp, n_sets * rows // 64, n_sets, ctypes.byref(flags))
            print("path_flags", flags.value)
    run()
    marker()
    vals = torch.stack([run() for _ in range(repeats)])
    torch.cuda.synchronize()
    np.save(out, vals.cpu().numpy())
    print("sizes", grp.lay.actor_size, grp.lay.theta_size)


def launches(trace_dir, kind):
    """The recorded call's launches out of a rocprofv3 kernel trace: after the marker kernel, up to the call's last kernel."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        sys.exit(f"{trace_dir}: expected one kernel trace, found {files}")
    with open(files[0], newline="") as f:
        rows = list(csv.DictReader(f))
    col = {k.lower(): k for k in rows[0]}
    pick = lambda r, *names: tuple(int(r[col[n]]) for n in names)
    rows.sort(key=lambda r: int(r[col["dispatch_id"]]))
    names = [r[col["kernel_name"]] for r in rows]
    marks = [i for i, n in enumerate(names) if MARKER in n]
    if not marks:
        sys.exit(f"{files[0]}: no marker kernel ({MARKER}) among {sorted(set(names))}")
    start = end = marks[-1] + 1
    while LAST[kind] not in names[end]:
        end += 1
    while end + 1 < len(names) and LAST[kind] in names[end + 1]:  # (acting: one tanh launch per set)
        end += 1
    return [(names[i], pick(rows[i], "grid_size_x", "grid_size_y", "grid_size_z"), pick(rows[i], "workgroup_size_x", "workgroup_size_y", "workgroup_size_z"),
             int(rows[i][col["lds_block_size"]])) for i in range(start, end + 1)]


def run_side(index, lib_path, env_extra, repeats, trace, tmp, tag):
    import numpy as np

    out = os.path.join(tmp, f"{tag}_{index}.npy")
    env = {k: v for k, v in os.environ.items() if not k.startswith("AVD_")}
    env.update(env_extra, AVDDPG_HIP_LIB=lib_path)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(index), out, str(repeats)]
    tdir = os.path.join(tmp, f"trace_{tag}_{index}")
    if trace:  # (tracing only: no counters; the program goes after `--`)
        cmd = ["rocprofv3", "--kernel-trace", "-f", "csv", "-d", tdir, "-o", "t", "--"] + cmd
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if p.returncode:
        sys.exit(f"{CASES[index][0]} ({tag}): exit status {p.returncode}; nothing more is started\n{p.stdout[-1500:]}\n{p.stderr[-3000:]}")
    word = lambda key: next((l.split()[1:] for l in p.stdout.splitlines() if l.startswith(key)), None)
    kind = "act" if CASES[index][0].startswith("act") else "learn"
    return np.load(out), (launches(tdir, kind) if trace else None), word("path_flags"), [int(x) for x in word("sizes")]


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(int(sys.argv[2]), sys.argv[3], int(sys.argv[4]))
    import numpy as np

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent_lib_dir")
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=8)
    ap.add_argument("--no-trace", action="store_true", help="values only (no rocprofv3)")
    a = ap.parse_args()
    lines, bad = [], 0

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/wide_ab.py: parent = {a.parent_lib_dir}, this tree = avddpg_amd/lib; {a.repeats} repeats per side; two weight sets, S = 4")
    bits = ("fused_fwd", "fused_delta", "r1", "dual", "act_in_dx")
    tmp = tempfile.mkdtemp(prefix="wide_ab_")
    seen_runtime_kernels = set()
    for i, (name, _, _, kind, env) in enumerate(CASES):
        old, lo, _, sizes = run_side(i, os.path.join(os.path.abspath(a.parent_lib_dir), LIB[kind]), env, a.repeats, not a.no_trace, tmp, "parent")
        new, ln, flags, _ = run_side(i, os.path.join(ROOT, "avddpg_amd", "lib", LIB[kind]), env, a.repeats, not a.no_trace, tmp, "new")
        say(f"\n== {name} ({kind} library)" + (f"; path: {', '.join(b for k, b in enumerate(bits) if int(flags[0]) >> k & 1) or 'none (layer-wise)'}" if flags else ""))
        if lo is not None:
            h = lambda l: hashlib.sha256(repr(l).encode()).hexdigest()[:16]
            same = lo == ln
            bad += not same
            say(f"launch sequence: parent {len(lo)} launches sha256 {h(lo)}, this tree {len(ln)} launches sha256 {h(ln)}: {'IDENTICAL' if same else 'DIFFERENT'}")
            for k in range(max(len(lo), len(ln))):
                x, y = (lo[k] if k < len(lo) else None), (ln[k] if k < len(ln) else None)
                short = lambda nm: nm.replace("(anonymous namespace)::", "").split("(")[0][:90]
                fmt = lambda e: "-" if e is None else f"{short(e[0])} grid {e[1]} wg {e[2]} lds {e[3]}"
                say(f"  {k:2d} {fmt(y)}" if x == y else f"  {k:2d} parent: {fmt(x)}\n     new:    {fmt(y)}")
                seen_runtime_kernels |= {short(e[0]) for e in (x, y) if e and "rocclr" in e[0]}
        if name.startswith("act"):
            equal = np.array_equal(old, new) and np.array_equal(old[0], old[-1])
            bad += not equal
            say(f"values: {old.shape[1]} outputs x {a.repeats} repeats, parent vs this tree bit for bit: {'EQUAL' if equal else 'DIFFERENT'}")
            continue
        asz, tsz = sizes
        n = old.shape[1] - 4
        slabs = [("actor", [slice(s * tsz, s * tsz + asz) for s in range(n // tsz)]), ("critic", [slice(s * tsz + asz, (s + 1) * tsz) for s in range(n // tsz)]),
                 ("losses", [slice(n, n + 4)])]
        for slab, sl in slabs:
            cat = lambda v: np.concatenate([v[..., s] for s in sl], axis=-1)
            ref = cat(old[0])
            scale = np.abs(ref).max()
            spread = max(np.abs(cat(old[k]) - ref).max() for k in range(1, a.repeats)) / scale
            dev = max(np.abs(cat(new[k]) - ref).max() for k in range(a.repeats)) / scale
            ok = dev == 0 or dev <= 2 * spread
            bad += not ok
            say(f"values, {slab:6s}: parent repeat-to-repeat spread {spread:.3e}, this tree vs parent {dev:.3e} of the slab's max {scale:.3e}: "
                f"{'OK' if ok else 'OUTSIDE'} (zero, or <= 2 x the parent's spread)")
    if not a.no_trace:
        say("\nruntime kernels (hipMemsetAsync / hipMemcpy2DAsync) seen in the kernel traces: " + (", ".join(sorted(seen_runtime_kernels)) or "none"))
    say(f"\nverdict: {'every launch sequence identical, every value within the bound' if not bad else f'{bad} check(s) failed'}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
