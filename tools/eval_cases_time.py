#!/usr/bin/env python3
"""Time the scenario evaluator (avd_eval_cases_f32, csrc/evalx.hip) against the rollout kernel it shares its arithmetic with
(avd_eval_rollout_f32, csrc/eval.hip) on the same cases, in one process: HIP events, one warm-up launch of each form first, then the
two forms ALTERNATED for `reps` repeats.
  (a) run_many(seeds=range(K))                : one workgroup per (platoon, seed), every workgroup streams its platoon's actors;
  (b) run_cases(("gaussian",), seeds=range(K)): one workgroup per (platoon, block of cases), the actors streamed once per block.
Shapes: P x L per-agent actors (default 4096 x 5), T = 600, K in {1, 4, 16}; L shared actors x K = 1024. The two forms' scores must be
identical before a time is printed. One JSON line per shape: min / median ms of both forms, the spread (max - min) over the alternated
repeats, the weight bytes each form streams COUNTED from the shapes (as tools/eval_time.py counts them; not a counter value), the ratio
a / b of the medians, and (b)'s f32 FMA rate as a share of the 157.3 TFLOP/s vector FP32 peak. usage: eval_cases_time.py [P] [L] [reps]"""
import copy
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # the repository root
import numpy as np
import torch

from avddpg_amd import config, evaluator, vec

P = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
L = int(sys.argv[2]) if len(sys.argv) > 2 else 5
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
T = 600
PEAK_FP32_VECTOR = 157.3e12  # FLOP/s, MI355X vector FP32


def actors(conf, n_sets, seed):
    """n_sets different actors at the reference widths, theta / stats slabs only (as tools/eval_time.py makes them)."""
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


def forward_fma(lay):
    return lay.S * lay.H1 + lay.H1 * lay.H2 + lay.H2 * lay.A + lay.H1 + lay.H2  # the three layers and the two BN applications


def alternate(a, b):
    """-> (sorted ms of a, sorted ms of b) over REPS alternated launches after one warm-up of each."""
    a.launch(), b.launch()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4 * REPS)]
    for i in range(REPS):
        for j, form in enumerate((a, b)):
            ev[4 * i + 2 * j].record()
            form.launch()
            ev[4 * i + 2 * j + 1].record()
    torch.cuda.synchronize()
    ms = lambda j: sorted(ev[4 * i + 2 * j].elapsed_time(ev[4 * i + 2 * j + 1]) for i in range(REPS))
    return ms(0), ms(1)


def main():
    conf = config.Config(pl_size=L, num_platoons=P)
    grp = actors(conf, P * L, 81)
    lay = grp.lay
    shapes = [(f"per_agent K={K}", dict(platoons=range(P)), P, K) for K in (1, 4, 16)] + [("shared K=1024", dict(platoons=[0], set_mod=L), 1, 1024)]
    for name, kw, G, K in shapes:
        seeds = list(range(K))
        a = evaluator.prepare_many(conf, grp, seeds=seeds, manual_timestep_override=T, **kw)
        b = evaluator.prepare_cases(conf, grp, scenarios=("gaussian",), seeds=seeds, manual_timestep_override=T, **kw)
        ms_a, ms_b = alternate(a, b)
        sa, sb = a.results()[0], b.results().scores[:, 0]
        assert sa.shape == sb.shape and np.array_equal(sa, sb), f"{name}: the two forms' scores differ"
        blocks = G * ((K + b.block - 1) // b.block)
        fma = G * K * T * L * forward_fma(lay)
        med = lambda v: v[len(v) // 2]
        spread = max(ms_a[-1] - ms_a[0], ms_b[-1] - ms_b[0])
        print(json.dumps(dict(shape=name, groups=G, K=K, T=T, L=L, block=b.block, reps=REPS,
                              rollout_ms_min=round(ms_a[0], 2), rollout_ms_median=round(med(ms_a), 2),
                              cases_ms_min=round(ms_b[0], 2), cases_ms_median=round(med(ms_b), 2), spread_ms=round(spread, 2),
                              ratio_rollout_over_cases=round(med(ms_a) / med(ms_b), 2),
                              rollout_weight_bytes=G * K * T * L * forward_bytes(lay), cases_weight_bytes=blocks * T * L * forward_bytes(lay),
                              cases_fma=fma, cases_share_of_fp32_vector_peak=round(2 * fma / (ms_b[0] * 1e-3) / PEAK_FP32_VECTOR, 4))), flush=True)


if __name__ == "__main__":
    main()
