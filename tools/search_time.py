#!/usr/bin/env python3
"""Time one generation of the gain search (evaluator.search_linear: avd_search_sample_f32 -> avd_eval_linear_f32 ->
avd_linear_fitness_f32 -> avd_search_refit_f32; csrc/search.hip, csrc/lin.hip) launch by launch, beside the grid's single rollout launch
of the same G (tune_linear's code path: a LinearBatch of fixed gains), in one process: HIP events around `inner` back-to-back launches of
one form, one warm-up launch of every form first, then the forms ALTERNATED for `reps` repeats. pop = `G` (default 4096), L = 5, T =
600, 12 cases (6 scenarios x 2 seeds), one gain row per vehicle (R = 5), floor(G / 8) elites.
  sample      : avd_search_sample_f32 into the search batch's gains;
  rollout     : avd_eval_linear_f32 over those candidates, metrics not requested;
  fitness     : avd_linear_fitness_f32 over its counters;
  refit       : avd_search_refit_f32 (rank + refit kernels) on a copy of the distribution, so the sampled candidates stay spread;
  generation  : the four launches back to back, on a distribution of its own that the refit moves (what search_linear enqueues);
  grid_rollout: avd_eval_linear_f32 over G homogeneous laws spread over the same bounds (the grid search's one rollout launch).
Before a time is printed the sample's candidate 0 must equal the mean bit for bit, the device fitness the NumPy float32 loop, and the
refit's best-ever fitness the maximum of that fitness. One JSON object: per form min / median ms per launch (per generation) and the
spread (max - min) over the repeats. No threshold: the numbers are the result.
usage: search_time.py [G] [reps] [inner] [out.json]   (out.json default: profiles/search_time.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)  # the repository root
import numpy as np
import torch

from avddpg_amd import config, evaluator, scenarios
from avddpg_amd._hip import call, ptr, stream_handle

G = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
INNER = int(sys.argv[3]) if len(sys.argv) > 3 else 10
OUT = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "search_time.json")
L, T, SEED = 5, 600, 6
NAMES, SEEDS = ["zero", "step", "ramp", "brake", "sine", "gaussian"], [6, 7]
BOUNDS = dict(kp=(0, 2), kv=(0, 4), ka=(-0.5, 0))


class Form:
    def __init__(self, fn):
        self.launch = fn


class Search:
    """The device state of one search over a LinearBatch, and its four launches."""

    def __init__(self, conf, space, batch):
        dev = batch.counters.device
        up = lambda x: torch.from_numpy(x).to(dev)
        self.b, self.R, self.n_elite, self.alpha = batch, space.rows(L), space.n_elite(), float(space.alpha)
        self.lo, self.hi, self.mean, self.std, self.min_std = (up(x) for x in space.tables(L))
        self.best_gains = torch.zeros(self.R, 4, device=dev)
        self.best_fit = torch.full((1,), -np.inf, device=dev)
        self.best_gen = torch.full((1,), -1, dtype=torch.int32, device=dev)
        self.fit = torch.empty(batch.G, device=dev)
        self.elite = torch.zeros(self.n_elite, dtype=torch.int32, device=dev)
        self.hist = torch.zeros(4, device=dev)
        self.gen = 0

    def sample(self):
        call("avd_search_sample_f32", self.b.G, L, self.R, ptr(self.mean), ptr(self.std), ptr(self.lo), ptr(self.hi), SEED, self.gen,
             ptr(self.b.gains), stream_handle())

    def fitness(self):
        self.b.enqueue_fitness(self.fit)

    def refit(self, mean=None, std=None):
        call("avd_search_refit_f32", self.b.G, L, self.R, self.n_elite, self.alpha, ptr(self.b.gains), ptr(self.fit), ptr(self.min_std),
             ptr(self.mean if mean is None else mean), ptr(self.std if std is None else std), ptr(self.best_gains), ptr(self.best_fit),
             ptr(self.best_gen), self.gen, ptr(self.elite), ptr(self.hist), stream_handle())

    def generation(self):
        self.sample(), self.b.launch(), self.fitness(), self.refit()
        self.gen += 1


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
    space = scenarios.check_search(scenarios.SearchSpace(BOUNDS, pop=G, gens=1, elite=0.125, seed=SEED), conf)
    mk = lambda g: evaluator.LinearBatch(conf, g, NAMES, [], SEEDS, None, 10.0, T, metrics=False)
    parts, whole = Search(conf, space, mk(np.zeros((G, L, 4), dtype=np.float32))), Search(conf, space, mk(np.zeros((G, L, 4), dtype=np.float32)))
    rng = np.random.RandomState(3)
    grid = np.zeros((G, 4), dtype=np.float32)
    for c, k in enumerate(scenarios.GAIN_KEYS[:3]):
        grid[:, c] = BOUNDS[k][0] + (BOUNDS[k][1] - BOUNDS[k][0]) * rng.rand(G)
    fixed = mk(np.repeat(grid[:, None, :], L, axis=1))
    assert parts.b.K == fixed.K == 12
    mean0, std0 = parts.mean.clone(), parts.std.clone()
    scratch = (parts.mean.clone(), parts.std.clone())

    def refit_on_copies():  # (the sample form's distribution stays where it started)
        parts.refit(*scratch)

    # the checks, on one pass of the four launches
    parts.sample(), parts.b.launch(), parts.fitness(), refit_on_copies()
    gains, fit = parts.b.gains.cpu().numpy(), parts.fit.cpu().numpy()
    assert np.array_equal(gains[0], mean0.cpu().numpy()), "candidate 0 is not the mean"
    assert np.array_equal(fit, scenarios.fitness_of(parts.b.counters.cpu().numpy())), "the device fitness differs from the NumPy float32 loop"
    assert float(parts.best_fit.cpu()[0]) == float(np.nanmax(fit)) and float(parts.hist.cpu()[3]) == space.n_elite()
    forms = dict(sample=Form(parts.sample), rollout=Form(parts.b.launch), fitness=Form(parts.fitness), refit=Form(refit_on_copies),
                 generation=Form(whole.generation), grid_rollout=Form(fixed.launch))
    ms = alternate(forms)
    med = lambda v: v[len(v) // 2]
    out = dict(device=torch.cuda.get_device_name(0), note="same build, same process, forms alternated; refit = the rank and refit kernels of one "
               "entry point", pop=G, K=12, L=L, T=T, rows=space.rows(L), n_elite=space.n_elite(),
               reps=REPS, launches_per_window=INNER)
    for n, v in ms.items():
        out[n] = dict(ms_min=round(v[0], 4), ms_median=round(med(v), 4), spread_ms=round(v[-1] - v[0], 4))
    parts_sum = sum(med(ms[n]) for n in ("sample", "rollout", "fitness", "refit"))
    out["sum_of_parts_ms"] = round(parts_sum, 4)
    out["generation_over_grid_rollout"] = round(med(ms["generation"]) / med(ms["grid_rollout"]), 4)
    out["generations_run"] = whole.gen
    out["best_after_those"] = dict(fitness=float(whole.best_fit.cpu()[0]), generation=int(whole.best_gen.cpu()[0]),
                                   table=whole.best_gains.cpu().numpy().astype(np.float64).round(6).tolist())
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
