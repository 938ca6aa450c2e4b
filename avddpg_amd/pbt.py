"""Population-based training over a hyperparameter sweep (`tr --pbt`, VecTrainer.exploit / set_hparams).

Every ``interval`` steps a generation ranks the experiments by fitness (the mean evaluator score of their platoons), replaces the
bottom ``k = floor(fraction * E)`` by copies of members of the top k -- the whole learner moves, the environment, OU state, replay
ring and seed stay -- and gives each replaced experiment its parent's values with every swept one multiplied by a factor drawn from
``perturb``. This module is the host side only: the refusals (check_pbt) and the plan of one generation (plan), both pure."""
import math

import numpy as np

from .vec import HP_KEYS

CLAMP_TO_ONE = ("tau", "gamma")  # (vec.hparams_rows: tau in (0, 1], gamma in [0, 1])


def check_pbt(interval, fraction, perturb, n_experiments, swept):
    """Why population-based training cannot run with these settings, raised as a ValueError -- or (interval, fraction, perturb tuple,
    k). Called before anything is allocated or launched. swept: the swept names (empty or None: not a sweep)."""
    if not swept:
        raise ValueError("population-based training needs a hyperparameter sweep (--sweep): it perturbs the swept values")
    bad = sorted(set(swept) - set(HP_KEYS))
    if bad:
        raise ValueError(f"population-based training perturbs {list(HP_KEYS)} only, got {bad}")
    if int(interval) != interval or interval < 1:
        raise ValueError(f"the generation interval must be an integer >= 1 step, got {interval}")
    fraction = float(fraction)
    if not 0 < fraction <= 0.5:
        raise ValueError(f"the exploit fraction must lie in (0, 0.5], got {fraction}")
    k = int(math.floor(fraction * n_experiments))
    if k == 0:
        raise ValueError(f"fraction {fraction} of {n_experiments} experiments replaces none (floor(fraction * E) == 0)")
    perturb = tuple(float(f) for f in perturb)
    if not perturb:
        raise ValueError("the perturbation factors are empty")
    for f in perturb:
        if not math.isfinite(f) or f <= 0:
            raise ValueError(f"perturbation factor {f} must be finite and > 0")
    return int(interval), fraction, perturb, k


def ranking(fitness):
    """Experiment indices from best to worst: fitness descending, NaN last, ties to the lower index."""
    f = [float(x) for x in fitness]
    return sorted(range(len(f)), key=lambda e: (math.isnan(f[e]), 0.0 if math.isnan(f[e]) else -f[e], e))


def rng_for(key, generation):
    """The generator of one generation: keyed by the batch's seeds and the generation number (never the global np.random stream)."""
    return np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(k) for k in key] + [int(generation)])))


def plan(fitness, rows, keys, generation, key, fraction, perturb):
    """One generation -> (pairs, new_rows). fitness [E]; rows: the E full rows in force (dicts of vec.HP_KEYS); keys: the swept names;
    key: the batch's seeds. The bottom k = floor(fraction * E) experiments of ranking(fitness), worst first, each get a parent drawn
    uniformly from the top k; pairs = [(parent, dst)]. new_rows[dst] = the parent's row with each swept key times a factor drawn from
    perturb (tau and gamma clamped to at most 1); every other row is unchanged."""
    E = len(rows)
    if len(fitness) != E:
        raise ValueError(f"{len(fitness)} fitness values for {E} experiments")
    k = int(math.floor(float(fraction) * E))
    order = ranking(fitness)
    top, bottom = order[:k], order[E - k:][::-1]
    rng = rng_for(key, generation)
    perturb = [float(f) for f in perturb]
    pairs, new_rows = [], [dict(r) for r in rows]
    for dst in bottom:
        parent = top[int(rng.integers(k))]
        row = dict(rows[parent])
        for name in keys:
            row[name] = row[name] * perturb[int(rng.integers(len(perturb)))]
            if name in CLAMP_TO_ONE:
                row[name] = min(row[name], 1.0)
        pairs.append((parent, dst))
        new_rows[dst] = row
    return pairs, new_rows
