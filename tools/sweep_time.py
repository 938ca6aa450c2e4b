"""Hyperparameter sweeps (VecTrainer(seeds=..., hparams=...)): training steps per second per experiment against one experiment per process.

  * config #1's shape, nofrl 1 x 3 (one platoon of three vehicles per experiment): E = 1 (a plain VecTrainer, what `tr --seed k` runs)
    and sweeps of E = 8 (actor_lr x critic_lr 2 x 2, 2 seeds) and E = 64 (actor_lr x critic_lr x gamma 4 x 4 x 2, 2 seeds);
  * interfrl 64 x 5 as one experiment against a sweep of E = 4 experiments of 16 x 5 (actor_lr 2 x tau 2, one seed), both on the
    fused3 engine (the split-operand set learner; --engine per_agent for the exact-f32 one).

Every run uses per-platoon episodes on the device (`--episodes platoon`) and is timed after a warm-up that passes the replay gate
(so every timed step learns), with a device synchronisation at both ends. Prints one JSON line per run:
{"case", "E", "platoons_per_experiment", "L", "steps", "s", "batch_steps_per_s", "experiment_steps_per_s"}.

  python tools/sweep_time.py [--steps 2000] [--warmup 200] [--buffer-size 10000] [--engine fused3]
"""
import argparse
import itertools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from avddpg_amd import config, trainer  # noqa: E402


def grid(seeds, **lists):
    """The experiments of a grid x seeds (seeds innermost) -> (seeds, hparams) as VecTrainer takes them."""
    names = list(lists)
    exps = [(dict(zip(names, combo)), k) for combo in itertools.product(*lists.values()) for k in seeds]
    return [k for _, k in exps], [h for h, _ in exps]


def run(case, fed_method, P, L, steps, warmup, buffer_size, sweep=None, engine=None):
    conf = config.Config(num_platoons=P, pl_size=L, fed_method=fed_method, buffer_size=buffer_size, weighted_average_enabled=False)
    kw = dict(rng="device", auto_reset="platoon", fused_update=fed_method == conf.nofrl, shared_engine=engine)
    if sweep is None:
        vt, E = trainer.VecTrainer(conf, seed=1, **kw), 1
    else:
        seeds, hps = sweep
        vt, E = trainer.VecTrainer(conf, seeds=seeds, hparams=hps, **kw), len(seeds)
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
    ap.add_argument("--buffer-size", type=int, default=10000)
    ap.add_argument("--engine", choices=["per_agent", "fused3"], default="fused3")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    st, wu, bs = args.steps, args.warmup, args.buffer_size
    lr_a, lr_c = [2.5e-5, 5e-5, 1e-4, 2e-4], [2.5e-4, 5e-4, 1e-3, 2e-3]
    run("nofrl_config1_1x3", "normal", 1, 3, st, wu, bs)
    run("nofrl_config1_1x3", "normal", 1, 3, st, wu, bs, grid((1, 2), actor_lr=lr_a[1:3], critic_lr=lr_c[1:3]))
    run("nofrl_config1_1x3", "normal", 1, 3, st, wu, bs, grid((1, 2), actor_lr=lr_a, critic_lr=lr_c, gamma=[0.95, 0.99]))
    run("interfrl_64x5", "interfrl", 64, 5, st, wu, bs, engine=args.engine)
    run("interfrl_4x16x5", "interfrl", 16, 5, st, wu, bs, grid((1,), actor_lr=lr_a[1:3], tau=[1e-3, 5e-3]), engine=args.engine)


if __name__ == "__main__":
    main()
