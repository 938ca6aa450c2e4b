#!/usr/bin/env python3
"""Time the linear scenario evaluator (avd_eval_linear_f32, avd_linear_fitness_f32, csrc/lin.hip) beside the yardstick that exists
today, the scenario evaluator on one platoon's actors (avd_eval_cases_f32, csrc/evalx.hip), on the same 12 cases, in one process: HIP
events around `inner` back-to-back launches of one form, one warm-up launch of every form first, then the forms ALTERNATED for `reps`
repeats. L = 5, T = 600.
  linear_1        : the rollout launch at G = 1, K = 12 (6 scenarios x 2 seeds), nominal;
  linear_grid     : the rollout launch at G = `G` (default 4096), the same K = 12, nominal, metrics not requested (tune_linear's launch);
  linear_grid_dist: the same G over K = 12 disturbed cases (1 scenario x (nominal + 5 levels) x 2 seeds);
  fitness         : the fitness launch over linear_grid's counters;
  actors_cases    : avd_eval_cases_f32, one platoon's 5 actors (reference widths) over linear_1's 12 cases.
Before a time is printed the grid's first candidate must equal linear_1's counters bit for bit (the same gains on the same cases) and the
device fitness the NumPy float32 loop. One JSON object: per form min / median ms per launch and the spread (max - min) over the repeats,
plus rollouts and vehicle-steps per second of the grid forms COUNTED from the shapes. No threshold: the numbers are the result.
usage: eval_linear_time.py [G] [reps] [inner] [out.json]   (out.json default: profiles/eval_linear_time.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)  # the repository root
import numpy as np
import torch

from avddpg_amd import config, evaluator, scenarios
from avddpg_amd.scenarios import Disturbance
from tools import eval_cases_time as ect

G = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
INNER = int(sys.argv[3]) if len(sys.argv) > 3 else 10
OUT = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "eval_linear_time.json")
L, T = 5, 600
NAMES, SEEDS = ["zero", "step", "ramp", "brake", "sine", "gaussian"], [6, 7]
LEVELS = [Disturbance("radar", noise_ep=0.05, noise_ev=0.05, noise_a=0.02), Disturbance("lag3", v2v_delay=3), Disturbance("loss20", v2v_drop=0.2),
          Disturbance("slow", dyn_coeff=0.15),
          Disturbance("all", noise_ep=0.05, noise_ev=0.05, noise_a=0.02, v2v_delay=3, v2v_drop=0.2, dyn_coeff=0.15)]


class Fitness:
    """The fitness launch over a batch's counters, as a form with launch()."""

    def __init__(self, batch):
        self.b = batch
        self.out = torch.empty(batch.G, dtype=torch.float32, device=batch.counters.device)

    def launch(self):
        from avddpg_amd._hip import call, ptr, stream_handle

        call("avd_linear_fitness_f32", self.b.G, self.b.K, self.b.L, ptr(self.b.counters), ptr(self.out), stream_handle())


def alternate(forms):
    """{name: sorted ms per launch} over REPS alternated windows of INNER launches each, after one warm-up launch of every form."""
    for f in forms.values():
        f.launch()
    torch.cuda.synchronize()
    ev = {n: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)] for n in forms}
    for i in range(REPS):
        for n, f in forms.items():
            ev[n][i][0].record()
            for _ in range(INNER):
                f.launch()
            ev[n][i][1].record()
    torch.cuda.synchronize()
    return {n: sorted(a.elapsed_time(b) / INNER for a, b in ev[n]) for n in forms}


def main():
    assert torch.cuda.is_available(), "a timing needs the GPU"
    conf = config.Config(pl_size=L)
    grid = np.zeros((G, 4), dtype=np.float32)  # candidate 0 is linear_1's law; the rest spread around it
    rng = np.random.RandomState(3)
    grid[:, 0], grid[:, 1] = 0.5 + 1.5 * rng.rand(G), 1.0 + 3.0 * rng.rand(G)
    grid[0] = (0.5, 1.0, 0.0, 0.0)
    gains = np.repeat(grid[:, None, :], L, axis=1)
    mk = lambda g, names, levels, metrics: evaluator.LinearBatch(conf, g, names, levels, SEEDS, None, 10.0, T, metrics=metrics)
    one = mk(gains[:1], NAMES, [], True)
    big = mk(gains, NAMES, [], False)
    dist = mk(gains, ["step"], LEVELS, False)
    assert one.K == big.K == dist.K == 12
    actors = evaluator.prepare_cases(conf, ect.actors(conf, L, 81), [0], NAMES, seeds=SEEDS, manual_timestep_override=T)
    assert actors.K == 12 and actors.G == 1
    forms = dict(linear_1=one, linear_grid=big, linear_grid_dist=dist, fitness=Fitness(big), actors_cases=actors)
    ms = alternate(forms)
    c1, cg = one.counters.cpu().numpy(), big.counters.cpu().numpy()
    assert np.array_equal(c1[0], cg[0]), "the grid's first candidate differs from the single launch of the same law"
    fit = forms["fitness"].out.cpu().numpy()
    assert np.array_equal(fit, scenarios.fitness_of(cg)), "the device fitness differs from the NumPy float32 loop"
    assert np.isfinite(dist.counters.cpu().numpy()).all()
    med = lambda v: v[len(v) // 2]
    out = dict(device=torch.cuda.get_device_name(0), note="same build, same process, forms alternated; rates counted from shapes",
               G=G, K=12, L=L, T=T, reps=REPS, launches_per_window=INNER)
    for n, v in ms.items():
        out[n] = dict(ms_min=round(v[0], 4), ms_median=round(med(v), 4), spread_ms=round(v[-1] - v[0], 4))
    for n in ("linear_grid", "linear_grid_dist"):
        sec = med(ms[n]) * 1e-3
        out[n].update(rollouts_per_s=round(G * 12 / sec), vehicle_steps_per_s=round(G * 12 * L * T / sec))
    out["ratio_linear_1_over_actors_cases"] = round(med(ms["linear_1"]) / med(ms["actors_cases"]), 4)
    out["best_of_grid"] = dict(index=int(scenarios.first_argmax(fit)), fitness=float(fit[scenarios.first_argmax(fit)]),
                               gains=[float(x) for x in grid[scenarios.first_argmax(fit)]])
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
