#!/usr/bin/env python3
"""A/B of the per-agent learner's HOST code (csrc/mlp.hip, lean.hip, cen.hip) between two builds of the library: same launches, same bits.

usage: tools/learn_ab.py PARENT_LIB_DIR [--out FILE] [--no-trace]

PARENT_LIB_DIR holds libavddpg_hip.so and libavddpg_hip_diag.so of the tree to compare against (`git archive <commit> avddpg_amd/csrc
include | tar -x -C DIR`, `make -C DIR/avddpg_amd/csrc all diag`, then DIR/avddpg_amd/lib); this tree's two libraries are the other
side. Every (group, side) runs in a fresh child process that loads its library through AVDDPG_HIP_LIB, under `rocprofv3 --kernel-trace`;
the children run one after another and the first that fails ends the run. A group is one library with one setting of the diagnostic
switches; inside it every case calls the learn entry points it has (avd_learn_f32, avd_learn_update_f32, avd_learn_update_act_f32 and
at the reference widths their three HP twins) on the same inputs, each from freshly uploaded slabs.
 * values: these kernels use no atomics, every sum has a fixed order. Every output slab -- grads, losses, theta_out, theta_t, stats_t,
   m, v, next actions -- must be EQUAL BIT FOR BIT on both sides.
 * launch sequence: the ordered (kernel name, grid, workgroup, LDS bytes) list of the whole child (the uploads' and the runtime's
   kernels included) must be identical on both sides.
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
REF3, REF4, GEN, CEN3, CEN5 = (3, 1, 256, 128, 48), (4, 1, 256, 128, 48), (5, 2, 128, 64, 32), (12, 3, 320, 160, 64), (20, 5, 320, 160, 64)
SCALAR, HP = ("learn", "update", "update_act"), ("learn_hp", "update_hp", "update_act_hp")
REFERENCE = [(dims, n, set_mod) for dims in (REF3, REF4) for n, set_mod in ((3, 0), (6, 3))]
own = lambda entries, set_mod: tuple(e for e in entries if set_mod == 0 or e.startswith("learn"))  # (shared sets: the gradient calls only)
# (group, library, environment, [(dims, agents, set_mod, entries)])
GROUPS = [
    ("product library", "product", {},
     [(d, n, sm, own(SCALAR + HP, sm)) for d, n, sm in REFERENCE] + [(GEN, 3, 0, SCALAR), (CEN3, 3, 0, SCALAR), (CEN5, 3, 0, SCALAR)]),
    ("diagnostic library, AVD_LEARN_KERNEL=fast", "diagnostic", {"AVD_LEARN_KERNEL": "fast"}, [(d, n, sm, own(SCALAR, sm)) for d, n, sm in REFERENCE]),
    ("diagnostic library, AVD_LEARN_GENERAL=1", "diagnostic", {"AVD_LEARN_GENERAL": "1"}, [(d, n, sm, own(SCALAR, sm)) for d, n, sm in REFERENCE]),
    ("diagnostic library, AVD_CEN_CHUNK=2 (the side-stream pipeline at 5 agents)", "diagnostic", {"AVD_CEN_CHUNK": "2"},
     [(CEN3, 5, 0, ("update", "update_act")), (CEN5, 5, 0, ("update", "update_act"))]),
]
LIB = {"product": "libavddpg_hip.so", "diagnostic": "libavddpg_hip_diag.so"}
KERNEL_NAMES = ("lean", "fast", "cen", "general")


def child(index, out):
    """One side of one group, in this process: every output slab of every (case, entry) -> out (.npz)."""
    import ctypes

    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from avddpg_amd import _hip, params

    dev = torch.device("cuda")
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    results = {}
    for ci, (dims, n, set_mod, entries) in enumerate(GROUPS[index][3]):
        S, A = dims[:2]
        lay = _hip.make_layout(*dims, 64)
        layp, T, St = ctypes.byref(lay), lay.theta_size, lay.stats_size
        rs = np.random.RandomState(100 + ci)
        n_sets = set_mod or n
        th0, st0 = params.init_weights(lay, rs)
        spread = lambda base, scale: (base[None] * (1 + scale * rs.standard_normal((n_sets, base.size)))).astype(np.float32)
        h = dict(theta=spread(th0, 0.05), theta_t=spread(th0, 0.05),
                 stats=(st0[None] + 0.2 * np.abs(rs.standard_normal((n_sets, St)))).astype(np.float32),
                 stats_t=(st0[None] + 0.2 * np.abs(rs.standard_normal((n_sets, St)))).astype(np.float32),
                 m=(1e-3 * rs.standard_normal((n, T))).astype(np.float32), v=(1e-6 * rs.standard_normal((n, T)) ** 2).astype(np.float32),
                 step=np.arange(3, 3 + n, dtype=np.int32),
                 s=rs.normal(0, 1.5, (n, 64, S)).astype(np.float32), a=rs.uniform(-2.5, 2.5, (n, 64, A)).astype(np.float32),
                 r=(-np.abs(rs.normal(0, 0.3, (n, 64)))).astype(np.float32), s2=rs.normal(0, 1.5, (n, 64, S)).astype(np.float32),
                 x=rs.normal(0, 1.5, (n, S + 2)).astype(np.float32))  # next states, row stride S + 2
        # (actor_lr, critic_lr, tau, 1 - tau, gamma, ou_theta, ou_scale, reserved) per experiment; agent j: row j % 3
        table = np.array([[1e-4 * (e + 1), 1e-3 / (e + 1), 0.005 * (e + 1), 1 - 0.005 * (e + 1), 0.99 - 0.02 * e, 0, 0, 0] for e in range(3)], np.float32)
        kern = ""
        if getattr(_hip.lib(), "avd_learn_kernel", None) is not None:
            k = ctypes.c_int(-1)
            _hip.call("avd_learn_kernel", layp, 0, ctypes.byref(k))
            kern = KERNEL_NAMES[k.value]
        print(f"case {ci} kernel {kern or '?'}")
        for entry in entries:
            d = {k: up(v) for k, v in h.items()}  # fresh slabs for every call
            d.update(theta_out=torch.zeros(n, T, device=dev), grads=torch.zeros(n, T, device=dev), losses=torch.zeros(n, 2, device=dev),
                     next=torch.zeros(n, A, device=dev), hp=up(table))
            p = {k: _hip.ptr(v) for k, v in d.items()}
            sweep, tail = entry.endswith("_hp"), ()
            if sweep:
                tail = (p["hp"], 3, 1)
            if entry.startswith("learn"):
                scal = (2.5,) if sweep else (0.99, 2.5)
                _hip.call("avd_learn_hp_f32" if sweep else "avd_learn_f32", layp, n, set_mod, p["theta"], p["stats"], p["theta_t"], p["stats_t"],
                          p["s"], p["a"], p["r"], p["s2"], *scal, p["grads"], p["losses"], *tail, None)
                outs = ("grads", "losses")
            else:
                act = "_act" in entry
                scal = (2.5,) if sweep else (0.99, 2.5, 1e-4, 1e-3, 0.005)
                name = "avd_learn_update" + ("_act" if act else "") + ("_hp" if sweep else "") + "_f32"
                _hip.call(name, layp, n, p["theta"], p["stats"], p["theta_out"], p["theta_t"], p["stats_t"], p["m"], p["v"], p["step"], p["s"],
                          p["a"], p["r"], p["s2"], *scal, p["grads"], p["losses"], *((p["x"], S + 2, p["next"]) if act else ()), *tail, None)
                outs = ("grads", "losses", "theta_out", "theta_t", "stats_t", "m", "v") + (("next",) if act else ())
            torch.cuda.synchronize()
            for k in outs:
                results[f"{ci}/{entry}/{k}"] = d[k].cpu().numpy()
    np.savez(out, **results)


def launches(trace_dir):
    """Every launch of a rocprofv3 kernel trace, in dispatch order."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        sys.exit(f"{trace_dir}: expected one kernel trace, found {files}")
    with open(files[0], newline="") as f:
        rows = list(csv.DictReader(f))
    col = {k.lower(): k for k in rows[0]}
    pick = lambda r, *names: tuple(int(r[col[n]]) for n in names)
    rows.sort(key=lambda r: int(r[col["dispatch_id"]]))
    return [(r[col["kernel_name"]], pick(r, "grid_size_x", "grid_size_y", "grid_size_z"), pick(r, "workgroup_size_x", "workgroup_size_y", "workgroup_size_z"),
             int(r[col["lds_block_size"]])) for r in rows]


def run_side(index, lib_path, trace, tmp, tag):
    import numpy as np

    out = os.path.join(tmp, f"{tag}_{index}.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("AVD_")}
    env.update(GROUPS[index][2], AVDDPG_HIP_LIB=lib_path)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(index), out]
    tdir = os.path.join(tmp, f"trace_{tag}_{index}")
    if trace:  # (tracing only: no counters; the program goes after `--`)
        cmd = ["rocprofv3", "--kernel-trace", "-f", "csv", "-d", tdir, "-o", "t", "--"] + cmd
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if p.returncode:
        sys.exit(f"{GROUPS[index][0]} ({tag}): exit status {p.returncode}; nothing more is started\n{p.stdout[-1500:]}\n{p.stderr[-3000:]}")
    kernels = [l.split()[3] for l in p.stdout.splitlines() if l.startswith("case ")]
    return dict(np.load(out)), (launches(tdir) if trace else None), kernels


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(int(sys.argv[2]), sys.argv[3])
    import numpy as np

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent_lib_dir")
    ap.add_argument("--out")
    ap.add_argument("--no-trace", action="store_true", help="values only (no rocprofv3)")
    a = ap.parse_args()
    lines, bad = [], 0

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/learn_ab.py: parent = {a.parent_lib_dir}, this tree = avddpg_amd/lib; batches of 64 rows; every slab compared bit for bit")
    tmp = tempfile.mkdtemp(prefix="learn_ab_")
    short = lambda nm: nm.replace("(anonymous namespace)::", "").split("(")[0][:100]
    for i, (group, kind, _, cases) in enumerate(GROUPS):
        old, lo, _ = run_side(i, os.path.join(os.path.abspath(a.parent_lib_dir), LIB[kind]), not a.no_trace, tmp, "parent")
        new, ln, kernels = run_side(i, os.path.join(ROOT, "avddpg_amd", "lib", LIB[kind]), not a.no_trace, tmp, "new")
        say(f"\n== {group}")
        if sorted(old) != sorted(new):
            bad += 1
            say(f"  DIFFERENT sets of outputs: {sorted(set(old) ^ set(new))}")
        for ci, (dims, n, set_mod, entries) in enumerate(cases):
            say(f"  S={dims[0]} A={dims[1]} {dims[2]}/{dims[3]}/{dims[4]}, {n} agents, set_mod={set_mod} -> {kernels[ci] if ci < len(kernels) else '?'}")
            for entry in entries:
                keys = sorted(k for k in old if k.startswith(f"{ci}/{entry}/"))
                same = {k.split("/")[2]: k in new and old[k].shape == new[k].shape and old[k].tobytes() == new[k].tobytes() for k in keys}
                finite = all(np.isfinite(old[k]).all() for k in keys)
                ok = bool(keys) and all(same.values())
                bad += not ok
                say(f"    {entry:14s} {sum(old[k].size for k in keys):9d} values in {', '.join(same)}: "
                    f"{'EQUAL bit for bit' if ok else 'DIFFERENT: ' + ', '.join(k for k, v in same.items() if not v)}{'' if finite else ' (non-finite values present)'}")
        if lo is not None:
            h = lambda l: hashlib.sha256(repr(l).encode()).hexdigest()[:16]
            same = lo == ln
            bad += not same
            say(f"  launch sequence of the whole child: parent {len(lo)} launches sha256 {h(lo)}, this tree {len(ln)} launches sha256 {h(ln)}: "
                f"{'IDENTICAL' if same else 'DIFFERENT'}")
            fmt = lambda e: "-" if e is None else f"{short(e[0])} grid {e[1]} wg {e[2]} lds {e[3]}"
            for k in range(max(len(lo), len(ln))):
                x, y = (lo[k] if k < len(lo) else None), (ln[k] if k < len(ln) else None)
                if x != y:
                    say(f"    {k:3d} parent: {fmt(x)}\n        new:    {fmt(y)}")
            mine = [e for e in ln if "avd" in e[0]]
            say(f"  the library's {len(mine)} launches, in order (runs of one launch folded):")
            k = 0
            while k < len(mine):
                j = k
                while j + 1 < len(mine) and mine[j + 1] == mine[k]:
                    j += 1
                say(f"    {j - k + 1:2d} x {fmt(mine[k])}")
                k = j + 1
    say(f"\nverdict: {'every slab equal bit for bit' + ('' if a.no_trace else ', every launch sequence identical') if not bad else f'{bad} check(s) failed'}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
