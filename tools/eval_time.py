#!/usr/bin/env python3
"""Time the evaluator rollout kernel (avd_eval_rollout_f32, csrc/eval.hip) with HIP events, one warm-up launch first, and the
per-platoon loop it replaces (evaluator.run, ~10 launches per step) on 16 platoons, extrapolated. One JSON line per shape:
  (a) per_agent: P platoons x L vehicles, one actor per (platoon, vehicle), T steps (default 4096 x 5, T = 600);
  (b) shared   : L shared actors (interfrl) from `seeds` evaluation seeds, T steps (default 5 x 1024 seeds).
Bytes streamed = rollouts x T x M x (actor weights + BN statistics read by one forward). usage: eval_time.py [P] [L] [seeds] [reps]"""
import copy
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # the repository root
import torch

from avddpg_amd import config, evaluator, vec

P = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
L = int(sys.argv[2]) if len(sys.argv) > 2 else 5
NSEED = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
REPS = int(sys.argv[4]) if len(sys.argv) > 4 else 3
T = 600


def actors(conf, n_sets, seed):
    """n_sets different actors at the reference widths, theta / stats slabs only."""
    small = vec.AgentGroup(1, 4, 1, conf, seed=seed)
    lay = small.lay
    g = copy.copy(small)
    g.theta = small.theta.expand(n_sets, lay.theta_size).contiguous()
    g.stats = small.stats.expand(n_sets, lay.stats_size).contiguous()
    gen = torch.Generator(device="cuda").manual_seed(seed)
    for lo in range(0, n_sets, 2048):
        blk = g.theta[lo:lo + 2048, :lay.actor_size]
        blk.mul_(1.0 + 0.2 * torch.randn(blk.shape, device="cuda", generator=gen))
    g.theta[:, lay.aW3:lay.aW3 + lay.H2] *= 40
    g.theta_t, g.stats_t, g.n_sets = g.theta, g.stats, n_sets
    return g


def forward_bytes(lay):
    H1, H2, S, A = lay.H1, lay.H2, lay.S, lay.A
    return 4 * (S * H1 + 3 * H1 + H1 * H2 + 3 * H2 + H2 * A + A + 2 * H1 + 2 * H2)


def time_kernel(b):
    b.launch()  # warm-up
    torch.cuda.synchronize()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2 * REPS)]
    for i in range(REPS):
        e[2 * i].record()
        b.launch()
        e[2 * i + 1].record()
    torch.cuda.synchronize()
    return sorted(e[2 * i].elapsed_time(e[2 * i + 1]) for i in range(REPS))


conf = config.Config(pl_size=L, num_platoons=P)
grp = actors(conf, P * L, 81)
shapes = [("per_agent", dict(platoons=range(P)), P, "%d platoons x %d vehicles, one actor each" % (P, L)),
          ("shared", dict(platoons=[0], set_mod=L, seeds=range(NSEED)), NSEED, "%d shared actors x %d seeds" % (L, NSEED))]
for name, kw, R, what in shapes:
    b = evaluator.prepare_many(conf, grp, manual_timestep_override=T, **kw)
    ms = time_kernel(b)
    nbytes = R * T * L * forward_bytes(grp.lay)
    print(json.dumps(dict(shape=name, what=what, rollouts=R, T=T, ms_min=round(ms[0], 2), ms_median=round(ms[len(ms) // 2], 2),
                          weight_bytes_streamed=nbytes, GBps=round(nbytes / (ms[0] * 1e-3) / 1e9, 1))), flush=True)

# the per-platoon loop it replaces: evaluator.run on 16 platoons, extrapolated to P
n = 16


def sub(p):  # platoon p's sets as a group of their own (views): what evaluator.run addresses
    v = copy.copy(grp)
    v.theta, v.stats, v.n_sets = grp.theta[p * L:(p + 1) * L], grp.stats[p * L:(p + 1) * L], L
    return v


evaluator.run(conf=conf, actors=sub(0), pl_idx=1, manual_timestep_override=T)  # warm-up
torch.cuda.synchronize()
t0 = time.perf_counter()
for p in range(n):
    evaluator.run(conf=conf, actors=sub(p), pl_idx=p + 1, manual_timestep_override=T)
torch.cuda.synchronize()
per = (time.perf_counter() - t0) / n
print(json.dumps(dict(shape="evaluator.run loop", platoons_timed=n, T=T, s_per_platoon=round(per, 4),
                      extrapolated_s_for_P=round(per * P, 1), P=P)), flush=True)
