#!/usr/bin/env python3
"""Time the disturbed step launch (avd_step_fused_dist_f32) against the nominal one of the same build (avd_step_fused_f32, both
csrc/env.hip) on the same state, in one process: a window is `inner` launches timed with HIP events in chunks of 25 back-to-back
launches, with the per-platoon episode end (untimed) between chunks, so that every launch runs on states inside the terminal bounds --
a platoon that leaves them is reset as in training; every window starts from freshly reset states. One warm-up window of each form
first, then the forms ALTERNATED for `reps` repeats.
  (a) nominal                         : VecTrainer._step_fused of a plain trainer;
  (b) null x 3                        : three null levels, no link state (what the observation buffer and the staged tables cost);
  (c) clean / noisy / lagged + lossy  : sensor noise on a third of the platoons, the V2V ring and a loss draw on another third;
  (d) all three axes on every platoon : the most one launch can do.
Shape: P x L (default 4096 x 5), Model B, the replay add included (ring of `cap` rows per agent). Before a time is printed, (b)'s true
state after the timed windows must equal (a)'s bit for bit and finite. One JSON line per form: min / median us per launch, the spread
(max - min) over the alternated repeats, the ratio to (a) of the medians, and the bytes per vehicle-step each form moves COUNTED from
the shapes (not a counter value). No threshold: the numbers are the result.
usage: train_disturb_time.py [P] [L] [reps] [inner] [out.json]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # the repository root
import torch

from avddpg_amd import config, trainer
from avddpg_amd.scenarios import Disturbance

P = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
L = int(sys.argv[2]) if len(sys.argv) > 2 else 5
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
INNER = int(sys.argv[4]) if len(sys.argv) > 4 else 200
OUT = sys.argv[5] if len(sys.argv) > 5 else None
CAP = 1024
CHUNK = 25  # launches per event pair

NOISE = dict(noise_ep=0.05, noise_ev=0.05, noise_a=0.02)
FORMS = [("nominal", None),
         ("null x 3", [Disturbance("a"), Disturbance("b"), Disturbance("c")]),
         ("clean / noisy / lagged+lossy", [Disturbance("clean"), Disturbance("radar", **NOISE), Disturbance("link", v2v_delay=3, v2v_drop=0.2)]),
         ("all axes, every platoon", [Disturbance("all", v2v_delay=3, v2v_drop=0.2, dyn_coeff=0.15, **NOISE)])]


def step_bytes(levels, S=4):
    """Bytes per vehicle-step, counted from the shapes (the per-platoon leader input and done flag, 5 B per platoon, come on top of
    every form). Nominal: reads x 16, prev_a 4, actor_out 4, ou_state 4, ep_reward 4; writes x 16, prev_a 4, ou_state 4, action 4,
    reward 4, term 1, ep_reward 4, the replay row 4 (2 S + 2). Disturbed: + obs_in 16 read (the row's s) + obs_out 16 written; a vehicle
    whose level uses the link + one ring slot written (4), one read (4), and the held value read (dropped) or written (not): 4."""
    nominal = 32 + 37 + 4 * (2 * S + 2)
    if levels is None:
        return nominal
    link = sum(d.uses_v2v for d in levels) / len(levels)
    return nominal + 32 + 12 * link


def main():
    assert torch.cuda.is_available(), "a timing needs the GPU"
    conf = config.Config(pl_size=L, num_platoons=P, buffer_size=CAP)
    ring = None
    vts = []
    for _, levels in FORMS:  # (one replay ring shared by the forms: they are timed one after the other)
        vt = trainer.VecTrainer(conf, rng="device", auto_reset="platoon", seed=7, init_seed=7, replay_ring=ring, train_disturb=levels)
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
        assert torch.equal(getattr(a, n).view(torch.uint8), getattr(b, n).view(torch.uint8)), f"null levels: {n} differs from the nominal launch"
    assert torch.equal(b.obs.view(torch.int32), b.x.view(torch.int32))
    for vt in vts:
        assert bool(torch.isfinite(vt.env.x).all()) and float(vt.env.x[..., :2].abs().max()) < 10 * conf.max_ep, "degenerate states"
    med = lambda v: sorted(v)[len(v) // 2]
    lines = []
    for (name, levels), v in zip(FORMS, us):
        lines.append(dict(form=name, platoons=P, L=L, reps=REPS, launches_per_window=INNER, us_min=round(min(v), 2), us_median=round(med(v), 2),
                          spread_us=round(max(v) - min(v), 2), ratio_to_nominal=round(med(v) / med(us[0]), 3),
                          counted_bytes_per_vehicle_step=step_bytes(levels),
                          counted_gbytes_per_s=round((step_bytes(levels) * P * L + 5 * P) / med(v) / 1e3, 1)))
        print(json.dumps(lines[-1]), flush=True)
    if OUT:
        with open(OUT, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0),
                           note="same build, same process, forms alternated; bytes counted from shapes, not read from counters", forms=lines),
                      f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
