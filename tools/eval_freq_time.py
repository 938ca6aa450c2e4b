#!/usr/bin/env python3
"""Time the frequency variants of the scenario evaluators (avd_eval_cases_freq_f32, csrc/evalx.hip; avd_eval_linear_freq_f32,
csrc/lin.hip) beside their non-frequency twins -- the kernels the parent commit had -- on the SAME cases, in one process: HIP events
around `inner` back-to-back launches of one form, one warm-up launch of every form first, then the forms ALTERNATED for `reps` repeats.
The cases are a frequency sweep's (fmin=0.02,fmax=2,n=16: 13 snapped frequencies, T = 600, one seed), L = 5:
  actors / actors_freq            : `P` platoons' actors (default 256, reference widths) x 13 cases, nominal (blocks of 16 rows);
  actors_dist / actors_dist_freq  : the same platoons x 26 cases (nominal + lag3 with sensor noise; blocks of 8 rows);
  linear / linear_freq            : `G` laws (default 4096) x 13 cases, nominal;
  linear_dist / linear_dist_freq  : the same laws x 26 disturbed cases.
Before a time is printed every frequency form's counters and metrics must equal its twin's bit for bit. One JSON object: per form min /
median ms per launch and the spread (max - min) over the repeats, and per pair the surcharge (the medians' ratio - 1). No threshold: the
numbers are the result.
usage: eval_freq_time.py [P] [G] [reps] [inner] [out.json]   (out.json default: profiles/eval_freq_time.json)"""
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
from tools import eval_linear_time as elt

P = int(sys.argv[1]) if len(sys.argv) > 1 else 256
G = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
elt.REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
elt.INNER = int(sys.argv[4]) if len(sys.argv) > 4 else 5
OUT = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "eval_freq_time.json")
L = 5
SPEC = "fmin=0.02,fmax=2,n=16"
LEVELS = [Disturbance("lag3", v2v_delay=3, noise_ep=0.05)]


def main():
    assert torch.cuda.is_available(), "a timing needs the GPU"
    conf = config.Config(pl_size=L)
    spec = scenarios.parse_frequency(SPEC)
    grp = ect.actors(conf, P * L, 81)
    rng = np.random.RandomState(3)
    gains = np.zeros((G, L, 4), dtype=np.float32)
    gains[:, :, 0], gains[:, :, 1] = (0.5 + 1.5 * rng.rand(G))[:, None], (1.0 + 3.0 * rng.rand(G))[:, None]
    forms, pairs = {}, []
    for tag, levels in (("", []), ("_dist", LEVELS)):
        f = evaluator.prepare_frequency(conf, grp, range(P), spec, levels)
        names, rows = [f"f{int(c)}" for c in f.cycles], f.leader_h.reshape(f.NC, -1, f.T)[:, 0]
        t = evaluator.CaseBatch(conf, grp, range(P), names, None, None, 10.0, None, None, None, None, f.levels, rows)
        lf = evaluator.LinearFrequencyBatch(conf, gains, spec, levels, None)
        lt = evaluator.LinearBatch(conf, gains, names, levels, None, None, 10.0, None, True, rows)
        assert torch.equal(t.leader, f.leader) and torch.equal(lt.leader, lf.leader) and f.K == t.K == lf.K == lt.K == 13 * (1 + len(levels))
        forms.update({f"actors{tag}": t, f"actors{tag}_freq": f, f"linear{tag}": lt, f"linear{tag}_freq": lf})
        pairs += [(f"actors{tag}", f"actors{tag}_freq"), (f"linear{tag}", f"linear{tag}_freq")]
    ms = elt.alternate(forms)
    for a, b in pairs:
        for n in ("counters", "metrics"):
            assert torch.equal(getattr(forms[a], n), getattr(forms[b], n)), f"{b}: {n} differ from {a}'s"
        assert torch.isfinite(forms[b].spectrum).all()
    med = lambda v: v[len(v) // 2]
    out = dict(device=torch.cuda.get_device_name(0), note="same build, same process, forms alternated; each pair runs the same cases",
               spec=SPEC, cycles=[int(c) for c in forms["actors_freq"].cycles], P=P, G=G, L=L, T=int(forms["actors_freq"].T),
               K=dict(nominal=13, disturbed=26), reps=elt.REPS, launches_per_window=elt.INNER)
    for n, v in ms.items():
        out[n] = dict(ms_min=round(v[0], 4), ms_median=round(med(v), 4), spread_ms=round(v[-1] - v[0], 4))
    out["surcharge"] = {b: round(med(ms[b]) / med(ms[a]) - 1, 4) for a, b in pairs}
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
