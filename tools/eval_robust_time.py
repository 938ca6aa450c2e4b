#!/usr/bin/env python3
"""Time the disturbed scenario evaluator (avd_eval_cases_dist_f32) against the nominal kernel of the same build (avd_eval_cases_f32,
both csrc/evalx.hip) on the same number of cases, in one process: HIP events, one warm-up launch of each form first, then the two forms
ALTERNATED for `reps` repeats.
  (a) run_cases(scenarios, seeds)                          : K = scenarios x seeds cases, blocks of avd_eval_cases_block;
  (b) run_disturbed(scenarios', [nominal, *levels], seeds) : the same K = scenarios' x levels x seeds, blocks of avd_eval_cases_dist_block.
Shape: P x L per-agent actors (default 4096 x 5), T = 600, 16 seeds: K = 16 (one scenario; (b): one seed-sharing pair of levels x 8
seeds) and the robustness matrix K = 96 (6 scenarios x 16 seeds against 1 scenario x 6 levels x 16 seeds). Before a time is printed,
(b)'s nominal level must equal run_cases on its scenarios bit for bit. One JSON line per shape: min / median ms of both forms, the
spread (max - min) over the alternated repeats, the weight bytes each form streams COUNTED from the shapes (not a counter value), the
ratio b / a of the medians. No threshold: the numbers are the result. usage: eval_robust_time.py [P] [L] [reps] [out.json]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # the repository root
import numpy as np
import torch

from avddpg_amd import config, evaluator
from avddpg_amd.scenarios import Disturbance
from tools import eval_cases_time as ect

P = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
L = int(sys.argv[2]) if len(sys.argv) > 2 else 5
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
OUT = sys.argv[4] if len(sys.argv) > 4 else None
T = 600

LEVELS = [Disturbance("radar", noise_ep=0.05, noise_ev=0.05, noise_a=0.02), Disturbance("lag3", v2v_delay=3), Disturbance("loss20", v2v_drop=0.2),
          Disturbance("slow", dyn_coeff=0.15),
          Disturbance("all", noise_ep=0.05, noise_ev=0.05, noise_a=0.02, v2v_delay=3, v2v_drop=0.2, dyn_coeff=0.15)]


def main():
    assert torch.cuda.is_available(), "a timing needs the GPU"
    ect.REPS = REPS
    conf = config.Config(pl_size=L, num_platoons=P)
    grp = ect.actors(conf, P * L, 81)
    lay = grp.lay
    kw = dict(platoons=range(P), manual_timestep_override=T)
    shapes = [("K=16: 1 scenario x 16 seeds | x (nominal, all) x 8 seeds", ["step"], list(range(16)), ["step"], LEVELS[4:], list(range(8))),
              ("K=96: 6 scenarios x 16 seeds | 1 scenario x (nominal + 5 levels) x 16 seeds", ["zero", "step", "ramp", "brake", "sine", "gaussian"],
               list(range(16)), ["step"], LEVELS, list(range(16)))]
    lines = []
    for name, a_names, a_seeds, b_names, levels, b_seeds in shapes:
        a = evaluator.prepare_cases(conf, grp, scenarios=a_names, seeds=a_seeds, **kw)
        b = evaluator.prepare_disturbed(conf, grp, scenarios=b_names, disturbances=levels, seeds=b_seeds, **kw)
        assert a.K == b.K, (a.K, b.K)
        ms_a, ms_b = ect.alternate(a, b)
        rb = b.results()
        ref = evaluator.run_cases(conf, grp, scenarios=b_names, seeds=b_seeds, **kw)
        assert np.array_equal(rb.nominal().counters, ref.counters), f"{name}: the nominal level differs from run_cases"
        differ = [not np.array_equal(rb.counters[:, :, d], rb.counters[:, :, 0]) for d in range(1, len(levels) + 1)]
        assert all(differ), (name, differ)
        med = lambda v: v[len(v) // 2]
        blocks = lambda batch: P * ((batch.K + batch.block - 1) // batch.block)
        lines.append(dict(shape=name, platoons=P, L=L, K=a.K, T=T, reps=REPS, nominal_block=a.block, disturbed_block=b.block,
                          nominal_ms_min=round(ms_a[0], 2), nominal_ms_median=round(med(ms_a), 2),
                          disturbed_ms_min=round(ms_b[0], 2), disturbed_ms_median=round(med(ms_b), 2),
                          spread_ms=round(max(ms_a[-1] - ms_a[0], ms_b[-1] - ms_b[0]), 2),
                          ratio_disturbed_over_nominal=round(med(ms_b) / med(ms_a), 3),
                          nominal_weight_bytes=blocks(a) * T * L * ect.forward_bytes(lay),
                          disturbed_weight_bytes=blocks(b) * T * L * ect.forward_bytes(lay),
                          rollout_kernel_weight_bytes=P * a.K * T * L * ect.forward_bytes(lay)))
        print(json.dumps(lines[-1]), flush=True)
    if OUT:
        with open(OUT, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), note="same build, same process, forms alternated; bytes counted from shapes",
                           shapes=lines), f, indent=1)


if __name__ == "__main__":
    main()
