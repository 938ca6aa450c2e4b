#!/usr/bin/env python3
"""What the gain search finds on the README's grid case (docs/TRAINING_EVIDENCE.md): 5 vehicles, Model B, euler, T = 600, the six
scenarios x evaluation seeds 6, 7. The grid `kp=0:2:9,kv=0:4:9,ka=-0.5:0:3` first (evaluator.tune_linear), then searches of pop 1024 x 30
generations (evaluator.search_linear), tied and per vehicle: inside the grid's box from the midpoint and from the grid's pick, and in the
wider box `kp=0:3,kv=0:4,ka=-1:0,kf=0:1`. Per search the best table, its fitness and generation, the best-so-far history and the final
std; then every law's score on the standard case (gaussian, seed 6) and its mean score over the 12 cases, undisturbed and under a V2V
delay of 3 steps (evaluator.run_linear). One JSON object, printed and written.
usage: search_evidence.py [out.json]   (default: profiles/search_evidence.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)  # the repository root
import numpy as np

from avddpg_amd import config, evaluator, scenarios
from avddpg_amd.scenarios import LinearLaw, SearchSpace

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "search_evidence.json")
NAMES, SEEDS = ["gaussian", "step", "ramp", "brake", "sine", "zero"], [6, 7]
BOX = dict(kp=(0, 2), kv=(0, 4), ka=(-0.5, 0))
WIDE = dict(kp=(0, 3), kv=(0, 4), ka=(-1, 0), kf=(0, 1))


def main():
    conf = config.Config(pl_size=5)
    kw = dict(scenarios=NAMES, seeds=SEEDS)
    grid = scenarios.parse_gain_grid("kp=0:2:9,kv=0:4:9,ka=-0.5:0:3")
    best, fit = evaluator.tune_linear(conf, grid, **kw)
    pick = grid[best][None]
    out = dict(grid=dict(gains=grid[best].tolist(), fitness=float(fit[best])))
    laws = [LinearLaw("grid", *[float(x) for x in grid[best]])]
    for tag, bounds, per_vehicle, init in (("tied", BOX, False, None), ("per_vehicle", BOX, True, None), ("tied_from_grid", BOX, False, pick),
                                           ("per_vehicle_from_grid", BOX, True, pick), ("wide_tied", WIDE, False, None),
                                           ("wide_per_vehicle", WIDE, True, None)):
        space = SearchSpace(bounds, pop=1024, gens=30, elite=0.125, per_vehicle=per_vehicle, init=init)
        r = evaluator.search_linear(conf, space, **kw)
        out[tag] = dict(fitness=r.fitness, generation=r.generation, table=np.asarray(r.law.table, dtype=np.float64).round(5).tolist(),
                        history_best=[round(float(x), 6) for x in r.history[:, 2]], final_std=r.std.astype(np.float64).round(5).tolist())
        laws.append(LinearLaw(tag, table=r.law.table))
    res = evaluator.run_linear(conf, laws, ["gaussian"], seeds=[6])
    out["gaussian_seed6_scores"] = {b.name: float(res.scores[i, 0, 0]) for i, b in enumerate(laws)}
    res = evaluator.run_linear(conf, laws, NAMES, [scenarios.Disturbance("lag", v2v_delay=3)], seeds=SEEDS)
    out["mean_score_nominal"] = {b.name: float(np.mean(res.scores[i, :, 0])) for i, b in enumerate(laws)}
    out["mean_score_lag3"] = {b.name: float(np.mean(res.scores[i, :, 1])) for i, b in enumerate(laws)}
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
