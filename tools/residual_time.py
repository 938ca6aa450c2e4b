#!/usr/bin/env python3
"""Time the residual policy's launches (avd_step_fused_res_f32, csrc/env.hip; avd_eval_cases_res_f32, csrc/evalx.hip) against the
launches of the same build without a law, on the same state, in one process.
Step forms, timed as tools/train_leader_time.py times its forms (a window is `inner` launches timed with HIP events in chunks of 25
back-to-back launches, the per-platoon episode end untimed between chunks, every window from freshly reset states; one warm-up window
of each form, then the forms ALTERNATED for `reps` repeats), at P x L (default 4096 x 5), Model B, the replay add included:
  (a) nominal                        : avd_step_fused_f32, the launch the parent commit has;
  (b) residual, zero law, scale 1    : avd_step_fused_res_f32 computing what (a) computes;
  (c) residual, kp=2 kv=1            : the law acting;
  (d) levels x manoeuvres            : avd_step_fused_dist_lead_f32, the parent's launch;
  (e) levels x manoeuvres, residual  : the same levels and manoeuvres through avd_step_fused_res_f32, kp=2 kv=1 kf=0.5.
Evaluator forms (one warm-up launch each, then `reps` alternated windows of 10 launches): the scenario evaluator on 5 shared actors x 12
cases (6 scenarios x 2 seeds, T = 600) without a law (avd_eval_cases_f32) and with one (avd_eval_cases_res_f32).
Before a time is printed, (b)'s state after the timed windows must equal (a)'s bit for bit and finite, and the evaluator with the zero
law must return the counters of the evaluator without one. One JSON line per form: min / median per launch (us for the step, ms for the
evaluator), the spread (max - min) over the alternated repeats and the ratio of the medians to the form without a law. The residual
step reads 16 B of gains (L rows, shared by every platoon) and writes 4 B (`applied`) more per vehicle; under levels it reads the
observation it would otherwise read only for the replay row. No threshold: the numbers are the result.
usage: residual_time.py [P] [L] [reps] [inner] [out.json]   (out.json default: profiles/residual_time.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)  # the repository root
import numpy as np
import torch

from avddpg_amd import config, evaluator, trainer, vec
from avddpg_amd.scenarios import Disturbance, Manoeuvre, ResidualLaw

P = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
L = int(sys.argv[2]) if len(sys.argv) > 2 else 5
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
INNER = int(sys.argv[4]) if len(sys.argv) > 4 else 200
OUT = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "residual_time.json")
CAP = 1024
CHUNK = 25  # launches per event pair
EVAL_INNER = 10

LEVELS = lambda: [Disturbance("clean"), Disturbance("radar", noise_ep=0.05, noise_ev=0.05, noise_a=0.02), Disturbance("link", v2v_delay=3, v2v_drop=0.2)]
MIXED = lambda: [Manoeuvre("step", profile="step"), Manoeuvre("brake", profile="brake", amp=0.5),
                 Manoeuvre("sine", profile="sine", amp=0.3, noise=0.05), Manoeuvre("clean")]
# (name, levels, manoeuvres, law, index of the form it is compared with)
FORMS = [("nominal", None, None, None, 0),
         ("residual, zero law, scale 1", None, None, lambda: ResidualLaw(0, 0), 0),
         ("residual, kp=2 kv=1", None, None, lambda: ResidualLaw(2, 1), 0),
         ("levels x manoeuvres", LEVELS, MIXED, None, 3),
         ("levels x manoeuvres, residual kp=2 kv=1 kf=0.5", LEVELS, MIXED, lambda: ResidualLaw(2, 1, 0, 0.5), 3)]


def main():
    assert torch.cuda.is_available(), "a timing needs the GPU"
    conf = config.Config(pl_size=L, num_platoons=P, buffer_size=CAP)
    ring = None
    vts = []
    for _, levels, ms, law, _ in FORMS:  # (one replay ring shared by the forms: they are timed one after the other)
        vt = trainer.VecTrainer(conf, rng="device", auto_reset="platoon", seed=7, init_seed=7, replay_ring=ring,
                                train_disturb=levels() if levels else None, train_leader=ms() if ms else None, residual=law() if law else None)
        ring = vt.replay.ring
        vt.reset_episode()
        vt.actor_out.uniform_(-1.0, 1.0, generator=torch.Generator(device="cuda").manual_seed(3))
        vts.append(vt)

    def window(vt):
        vt.reset_episode()
        pairs, left = [], INNER
        while left > 0:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(min(CHUNK, left)):
                vt._step_fused()
            e1.record()
            pairs.append((e0, e1))
            left -= CHUNK
            vt.env.episode_end(vt.ep_reward, vt.M, conf.steps_per_episode, any_reset=vt.env.any_done)  # untimed: resets what left the bounds
        torch.cuda.synchronize()
        return sum(a.elapsed_time(b) for a, b in pairs) * 1000.0 / INNER  # us per launch

    for vt in vts:
        window(vt)  # warm-up
    us = [[] for _ in FORMS]
    for _ in range(REPS):
        for k, vt in enumerate(vts):
            us[k].append(window(vt))
    a, b = vts[0], vts[1]
    for n in ("x", "prev_a", "reward", "done"):
        assert torch.equal(getattr(a.env, n).view(torch.uint8), getattr(b.env, n).view(torch.uint8)), f"zero law: {n} differs from the nominal launch"
    assert torch.equal(a.actions.view(torch.int32), b.actions.view(torch.int32)) and torch.equal(a.leader_exog.view(torch.int32), b.leader_exog.view(torch.int32))
    assert bool((b.applied.view(-1) == b.actions.view(-1)).all())
    for vt in vts:
        assert bool(torch.isfinite(vt.env.x).all()) and float(vt.env.x[..., :2].abs().max()) < 10 * conf.max_ep, "degenerate states"
    med = lambda v: sorted(v)[len(v) // 2]
    lines = []
    for (name, _, _, _, base), v in zip(FORMS, us):
        lines.append(dict(form=name, platoons=P, L=L, reps=REPS, launches_per_window=INNER, us_min=round(min(v), 2), us_median=round(med(v), 2),
                          spread_us=round(max(v) - min(v), 2), compared_with=FORMS[base][0], ratio=round(med(v) / med(us[base]), 3)))
        print(json.dumps(lines[-1]), flush=True)

    # ---- the scenario evaluator: 5 shared actors x 12 cases --------------------------------------------------------------------------
    econf = config.Config(pl_size=L)
    grp = vec.AgentGroup(L, 4, 1, econf, seed=11)
    lay = grp.lay
    grp.theta[:, lay.aW3:lay.aW3 + lay.H2] *= 40.0  # unsaturated, non-zero actions
    names, seeds = ["zero", "step", "ramp", "brake", "sine", "gaussian"], [6, 7]
    mk = lambda law: evaluator.prepare_cases(econf, grp, [0], names, seeds=seeds, set_mod=L, base_law=law)
    forms = {"run_cases": mk(None), "run_cases, zero law": mk(ResidualLaw(0, 0)), "run_cases, kp=2 kv=1": mk(ResidualLaw(2, 1))}
    for f in forms.values():
        f.launch()
    torch.cuda.synchronize()
    assert np.array_equal(forms["run_cases"].results().counters, forms["run_cases, zero law"].results().counters), "zero law: counters differ"
    ev = {n: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)] for n in forms}
    for i in range(REPS):
        for n, f in forms.items():
            ev[n][i][0].record()
            for _ in range(EVAL_INNER):
                f.launch()
            ev[n][i][1].record()
    torch.cuda.synchronize()
    ms = {n: sorted(x.elapsed_time(y) / EVAL_INNER for x, y in ev[n]) for n in forms}
    for n, v in ms.items():
        lines.append(dict(form=n, actors=L, cases=forms[n].K, T=forms[n].T, block=forms[n].block, reps=REPS, launches_per_window=EVAL_INNER,
                          ms_min=round(v[0], 4), ms_median=round(med(v), 4), spread_ms=round(v[-1] - v[0], 4), compared_with="run_cases",
                          ratio=round(med(v) / med(ms["run_cases"]), 3)))
        print(json.dumps(lines[-1]), flush=True)
    with open(OUT, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), note="same build, same process, forms alternated", forms=lines), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
