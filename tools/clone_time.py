#!/usr/bin/env python3
"""Time the warm start's launches (avd_clone_sample_f32, csrc/clone.hip; avd_actor_clone_f32, csrc/mlp.hip; the avd_adam_polyak_f32 of
a fit step) beside avd_learn_f32 on the same set counts, in one process, and the whole default fit (2000 steps) by the wall clock.
Set counts: 5 (one platoon's vehicles, what `tr --warm_start` fits) and 64 x 5. Reference widths, Model B.
A window is `inner` back-to-back launches of one form between two HIP events; one warm-up window per form, then the forms ALTERNATED
for `reps` repeats. One JSON line per (set count, form): min / median us per launch and the spread (max - min) over the repeats; for the
clone launch also the ratio of its median to avd_learn_f32's (the clone does one forward and one backward where the learner does five
and two). The fit: AgentGroup.clone_fit with the default WarmStart, from launch to the losses on the host, median of 3, and the last
step's mean loss. No threshold: the numbers are the result.
usage: clone_time.py [reps] [inner] [out.json]   (out.json default: profiles/clone_time.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)  # the repository root
import numpy as np
import torch

from avddpg_amd import _hip, config, vec
from avddpg_amd._hip import call, ptr, stream_handle
from avddpg_amd.scenarios import WarmStart

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
INNER = int(sys.argv[2]) if len(sys.argv) > 2 else 200
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "clone_time.json")
L = 5


def forms_of(n_sets):
    conf = config.Config(pl_size=L)
    grp = vec.AgentGroup(n_sets, 4, 1, conf, seed=11)
    lay, f32 = grp.lay, dict(dtype=torch.float32, device="cuda")
    spec = WarmStart(kp=2, kv=1)
    gains, box = torch.from_numpy(spec.gains(L)).cuda(), torch.from_numpy(spec.box(conf)).cuda()
    s, u = torch.empty(n_sets, 64, 4, **f32), torch.empty(n_sets, 64, 1, **f32)
    grads, losses = torch.zeros(n_sets, lay.theta_size, **f32), torch.zeros(n_sets, 2, **f32)
    gen = torch.Generator(device="cuda").manual_seed(3)
    a, r, s2 = (torch.empty(n_sets, 64, 1, **f32).uniform_(-2.5, 2.5, generator=gen), -torch.rand(n_sets, 64, generator=gen, **f32),
                torch.empty(n_sets, 64, 4, **f32).uniform_(-1.5, 1.5, generator=gen))
    one = torch.ones(n_sets, dtype=torch.int32, device="cuda")
    st = stream_handle()
    common = (ptr(grp.theta), ptr(grp.stats))

    def sample():
        call("avd_clone_sample_f32", n_sets, 4, L, ptr(gains), ptr(box), -2.5, 2.5, 0, 1, 0, None, 1, ptr(s), ptr(u), st)

    def clone():
        call("avd_actor_clone_f32", grp._layp, n_sets, *common, ptr(s), ptr(u), 2.5, ptr(grads), ptr(losses), st)

    def adam():  # (step 1 every time, lr as small as it gets: the weights stay where the other forms can use them)
        call("avd_adam_polyak_f32", grp._layp, n_sets, *common, ptr(grp.theta_t), ptr(grp.stats_t), ptr(grp.m), ptr(grp.v), ptr(grads), ptr(one),
             1e-12, 1e-12, 1.0, st)

    def learn():
        call("avd_learn_f32", grp._layp, n_sets, 0, *common, ptr(grp.theta_t), ptr(grp.stats_t), ptr(s), ptr(a), ptr(r), ptr(s2), 0.99, 2.5,
             ptr(grads), ptr(losses), st)

    sample()
    keep = (grp, gains, box, s, u, grads, losses, a, r, s2, one)  # (alive as long as the closures run)
    return [("avd_clone_sample_f32", sample), ("avd_actor_clone_f32", clone), ("avd_adam_polyak_f32 (tau = 1)", adam),
            ("avd_learn_f32", learn)], keep


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(INNER):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / INNER  # us per launch


def main():
    assert torch.cuda.is_available(), "a timing needs the GPU"
    med = lambda v: sorted(v)[len(v) // 2]
    lines = []
    for n_sets in (L, 64 * L):
        forms, keep = forms_of(n_sets)
        for _, fn in forms:
            window(fn)  # warm-up
        us = {name: [] for name, _ in forms}
        for _ in range(REPS):
            for name, fn in forms:
                us[name].append(window(fn))
        assert bool(torch.isfinite(keep[5]).all()), "non-finite gradients"
        for name, _ in forms:
            v = us[name]
            line = dict(form=name, n_sets=n_sets, reps=REPS, launches_per_window=INNER, us_min=round(min(v), 2), us_median=round(med(v), 2),
                        spread_us=round(max(v) - min(v), 2))
            if name == "avd_actor_clone_f32":
                line["ratio_to_avd_learn_f32"] = round(med(v) / med(us["avd_learn_f32"]), 3)
            lines.append(line)
            print(json.dumps(line), flush=True)
    # the whole default fit, wall clock (launch to the losses on the host)
    conf = config.Config(pl_size=L)
    spec = WarmStart(kp=2, kv=1)
    walls, last = [], None
    for _ in range(3):
        grp = vec.AgentGroup(L, 4, 1, conf, seed=1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last = grp.clone_fit(spec, M=L, seed=1)
        walls.append(time.perf_counter() - t0)
    line = dict(form="AgentGroup.clone_fit, default WarmStart", n_sets=L, steps=spec.steps, launches=3 * spec.steps, wall_s_median=round(med(walls), 4),
                wall_s_min=round(min(walls), 4), wall_s_max=round(max(walls), 4), us_per_step=round(1e6 * med(walls) / spec.steps, 1),
                final_loss_mean=float(np.mean(last)))
    lines.append(line)
    print(json.dumps(line), flush=True)
    with open(OUT, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), note="same build, same process, forms alternated", forms=lines), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
