"""Seed batches (VecTrainer(seeds=...)): training steps per second per experiment against one experiment per process.

  * config #1's shape, nofrl 1 x 3 (one platoon of three vehicles per experiment): E = 1 (a plain VecTrainer, what `tr --seed k` runs)
    and seed batches of E = 8 and 64;
  * interfrl 4096 x 5 as one experiment against a batch of E = 4 experiments of 1024 x 5 (shared sets, --engine, default fused3).

Every run uses per-platoon episodes on the device (`--episodes platoon`) and is timed after a warm-up that passes the replay gate
(so every timed step learns), with a device synchronisation at both ends. Prints one JSON line per run:
{"case", "E", "platoons_per_experiment", "L", "steps", "s", "batch_steps_per_s", "experiment_steps_per_s"}.
--solo-only times the E = 1 runs only (they reach only the scalar-seed kernels: runs against an older build of the library,
AVDDPG_HIP_LIB=..., for a before / after kernel-trace pair).

  python tools/seed_batch_time.py [--steps 2000] [--warmup 200] [--engine fused3] [--buffer-size 10000] [--solo-only]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from avddpg_amd import config, trainer  # noqa: E402


def run(case, fed_method, P, L, E, steps, warmup, buffer_size, engine=None):
    conf = config.Config(num_platoons=P, pl_size=L, fed_method=fed_method, buffer_size=buffer_size, weighted_average_enabled=False)
    kw = dict(rng="device", auto_reset="platoon", fused_update=fed_method == conf.nofrl, shared_engine=engine)
    vt = trainer.VecTrainer(conf, seed=1, **kw) if E == 1 else trainer.VecTrainer(conf, seeds=list(range(1, E + 1)), **kw)
    vt.reset_episode()
    for _ in range(max(warmup, conf.batch_size + 1)):
        vt.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        vt.step()
    torch.cuda.synchronize()
    s = time.perf_counter() - t0
    out = dict(case=case, E=E, platoons_per_experiment=P, L=L, engine=vt.shared_engine if vt.shared else None, steps=steps,
               s=round(s, 4), batch_steps_per_s=round(steps / s, 1), experiment_steps_per_s=round(E * steps / s, 1))
    print(json.dumps(out), flush=True)
    del vt
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--engine", choices=["per_agent", "batched", "fused", "fused3"], default="fused3")
    ap.add_argument("--buffer-size", type=int, default=10000, help="replay capacity per agent (the reference's 100000 at 4096 x 5 is 82 GB)")
    ap.add_argument("--solo-only", action="store_true")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    st, wu, bs = args.steps, args.warmup, args.buffer_size
    for E in ((1,) if args.solo_only else (1, 8, 64)):
        run("nofrl_config1_1x3", "normal", 1, 3, E, st, wu, bs)
    run("interfrl_4096x5", "interfrl", 4096, 5, 1, st, wu, bs, args.engine)
    if not args.solo_only:
        run("interfrl_4x1024x5", "interfrl", 1024, 5, 4, st, wu, bs, args.engine)


if __name__ == "__main__":
    main()
