"""Population-based training (`tr --pbt`): what an exploit and a generation cost.

  * avd_copy_experiment_sets_f32 alone on random slabs at the reference layout, timed with device events over --reps calls after a
    warm-up: nofrl 64 x 3 (E = 64 experiments of one platoon of three vehicles, 16 pairs), fused3 4 x 16 x 5 (E = 4 experiments of
    five shared sets, one pair) and a gigabyte case (E = 16 experiments of 256 platoons x 3, four pairs). Bytes moved = 2 x (pairs x
    sets per experiment x (4 theta_size + 2 stats_size + 1) x 4 B) -- read once, written once.
  * a generation of the CLI example (`tr --sweep actor_lr=5e-5,1e-4,2e-4 --sweep critic_lr=1e-3,2e-3 --seeds 1-2 --pbt 20000`, nofrl, the
    Config's platoon shape): scoring (one evaluator launch), plan, exploit and set_hparams, timed with a host clock between device
    synchronisations, against the time of one interval of training steps estimated from --steps timed steps.

Prints one JSON line per case. Run it under `rocprofv3 --kernel-trace --stats` for the kernel's own time.

  python tools/pbt_time.py [--reps 50] [--steps 2000] [--only copy|generation]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from avddpg_amd import _hip, config, pbt, trainer  # noqa: E402
from avddpg_amd._hip import call, ptr, stream_handle  # noqa: E402


def copy_case(case, E, sets_per_exp, M, pairs, reps):
    lay = _hip.make_layout(4, 1, 256, 128, 48, 64)
    n = E * sets_per_exp
    T, S = lay.theta_size, lay.stats_size
    sl = [torch.zeros(n, w, dtype=torch.float32, device="cuda") for w in (T, S, T, S, T, T)]
    step = torch.zeros(n, dtype=torch.int32, device="cuda")
    flat = [x for pr in pairs for x in pr]
    arr = (ctypes.c_int32 * len(flat))(*flat)
    args = (ctypes.byref(lay), n, E, M, arr, len(pairs), *[ptr(t) for t in sl], ptr(step))
    for _ in range(5):
        call("avd_copy_experiment_sets_f32", *args, stream_handle())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        call("avd_copy_experiment_sets_f32", *args, stream_handle())
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    nbytes = 2 * len(pairs) * sets_per_exp * (4 * T + 2 * S + 1) * 4
    out = dict(case=case, E=E, sets_per_experiment=sets_per_exp, pairs=len(pairs), bytes=nbytes, ms=round(ms, 4),
               GB_per_s=round(nbytes / ms / 1e6, 1))
    print(json.dumps(out), flush=True)
    del sl, step
    torch.cuda.empty_cache()


def generation_case(steps):
    conf = config.Config()
    grid = [(a, c) for a in (5e-5, 1e-4, 2e-4) for c in (1e-3, 2e-3)]
    seeds = [k for _ in grid for k in (1, 2)]
    hps = [dict(actor_lr=a, critic_lr=c) for a, c in grid for _ in (1, 2)]
    vt = trainer.VecTrainer(conf, rng="device", auto_reset="platoon", fused_update=True, seeds=seeds, hparams=hps)
    vt.reset_episode()
    for _ in range(conf.batch_size + 100):
        vt.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        vt.step()
    torch.cuda.synchronize()
    step_s = (time.perf_counter() - t0) / steps
    gens = []
    for g in range(1, 4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit = np.mean(vt.evaluator_scores().astype(np.float64), axis=1)
        pairs, rows = pbt.plan(fit, vt.hp_rows, ["actor_lr", "critic_lr"], g, vt.seeds, 0.25, (0.8, 1.2))
        vt.exploit(pairs)
        vt.set_hparams(rows)
        torch.cuda.synchronize()
        gens.append(time.perf_counter() - t0)
    interval = 20000
    out = dict(case="cli_example_generation", E=vt.E, platoons_per_experiment=vt.P_exp, L=vt.L, step_ms=round(1e3 * step_s, 4),
               generation_s=[round(x, 4) for x in gens], interval_steps=interval, interval_s=round(interval * step_s, 2),
               generation_share_of_interval=round(min(gens) / (interval * step_s), 5))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--only", choices=["copy", "generation"], default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    if args.only in (None, "copy"):
        copy_case("nofrl_64x3_E64", 64, 3, 3, [(e, 63 - e) for e in range(16)], args.reps)
        copy_case("fused3_4x16x5", 4, 5, 5, [(0, 3)], args.reps)
        copy_case("nofrl_256x3_E16_gigabyte", 16, 768, 3, [(e, 15 - e) for e in range(4)], args.reps)
    if args.only in (None, "generation"):
        generation_case(args.steps)


if __name__ == "__main__":
    main()
