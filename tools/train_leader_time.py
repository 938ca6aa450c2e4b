#!/usr/bin/env python3
"""Time the step launch under leader manoeuvres (avd_step_fused_lead_f32, avd_step_fused_dist_lead_f32) against the launches of the
same build without them (avd_step_fused_f32, avd_step_fused_dist_f32; all csrc/env.hip) on the same state, in one process: a window is
`inner` launches timed with HIP events in chunks of 25 back-to-back launches, with the per-platoon episode end (untimed) between chunks,
so that every launch runs on states inside the terminal bounds and the platoons' episode steps spread as in training; every window
starts from freshly reset states. One warm-up window of each form first, then the forms ALTERNATED for `reps` repeats.
  (a) nominal                      : VecTrainer._step_fused of a plain trainer -- the launch the parent commit has;
  (b) one gaussian manoeuvre       : the manoeuvre twin computing what (a) computes (what the extra arguments and the branch cost);
  (c) step / brake / noisy sine / clean : a table read on three quarters of the leaders, an extra multiply-add on one quarter;
  (d) levels                       : clean / noisy / lagged + lossy disturbance levels, no manoeuvres -- the parent's disturbed launch;
  (e) levels x manoeuvres          : (d)'s levels crossed with (c)'s manoeuvres in one instantiation.
Shape: P x L (default 4096 x 5), Model B, the replay add included (ring of `cap` rows per agent). Before a time is printed, (b)'s state
after the timed windows must equal (a)'s bit for bit and finite. One JSON line per form: min / median us per launch, the spread (max -
min) over the alternated repeats and the ratio of the medians to the form without manoeuvres ((a) for (b), (c); (d) for (e)). The
manoeuvre forms read 4 B more per PLATOON (one table entry or none; the episode step), nothing more per vehicle. No threshold: the
numbers are the result.
usage: train_leader_time.py [P] [L] [reps] [inner] [out.json]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # the repository root
import torch

from avddpg_amd import config, trainer
from avddpg_amd.scenarios import Disturbance, Manoeuvre

P = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
L = int(sys.argv[2]) if len(sys.argv) > 2 else 5
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
INNER = int(sys.argv[4]) if len(sys.argv) > 4 else 200
OUT = sys.argv[5] if len(sys.argv) > 5 else None
CAP = 1024
CHUNK = 25  # launches per event pair

LEVELS = lambda: [Disturbance("clean"), Disturbance("radar", noise_ep=0.05, noise_ev=0.05, noise_a=0.02), Disturbance("link", v2v_delay=3, v2v_drop=0.2)]
MIXED = lambda: [Manoeuvre("step", profile="step"), Manoeuvre("brake", profile="brake", amp=0.5),
                 Manoeuvre("sine", profile="sine", amp=0.3, noise=0.05), Manoeuvre("clean")]
# (name, levels, manoeuvres, index of the form it is compared with)
FORMS = [("nominal", None, None, 0),
         ("one gaussian manoeuvre", None, lambda: [Manoeuvre("clean")], 0),
         ("step / brake / noisy sine / clean", None, MIXED, 0),
         ("levels: clean / noisy / lagged+lossy", LEVELS, None, 3),
         ("levels x manoeuvres", LEVELS, MIXED, 3)]


def main():
    assert torch.cuda.is_available(), "a timing needs the GPU"
    conf = config.Config(pl_size=L, num_platoons=P, buffer_size=CAP)
    ring = None
    vts = []
    for _, levels, ms, _ in FORMS:  # (one replay ring shared by the forms: they are timed one after the other)
        vt = trainer.VecTrainer(conf, rng="device", auto_reset="platoon", seed=7, init_seed=7, replay_ring=ring,
                                train_disturb=levels() if levels else None, train_leader=ms() if ms else None)
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
    a, b = vts[0].env, vts[1].env
    for n in ("x", "prev_a", "reward", "done"):
        assert torch.equal(getattr(a, n).view(torch.uint8), getattr(b, n).view(torch.uint8)), f"one gaussian manoeuvre: {n} differs from the nominal launch"
    assert torch.equal(vts[0].leader_exog.view(torch.int32), vts[1].leader_exog.view(torch.int32))
    for vt in vts:
        assert bool(torch.isfinite(vt.env.x).all()) and float(vt.env.x[..., :2].abs().max()) < 10 * conf.max_ep, "degenerate states"
    med = lambda v: sorted(v)[len(v) // 2]
    lines = []
    for (name, _, _, base), v in zip(FORMS, us):
        lines.append(dict(form=name, platoons=P, L=L, reps=REPS, launches_per_window=INNER, us_min=round(min(v), 2), us_median=round(med(v), 2),
                          spread_us=round(max(v) - min(v), 2), compared_with=FORMS[base][0], ratio=round(med(v) / med(us[base]), 3)))
        print(json.dumps(lines[-1]), flush=True)
    if OUT:
        with open(OUT, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), note="same build, same process, forms alternated", forms=lines), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
