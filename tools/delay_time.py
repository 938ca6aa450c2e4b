#!/usr/bin/env python3
"""Time the two calls of a delayed-policy run beside the calls they stand in for, in one process, at 4096 platoons x 5 vehicles (the
headline shape): reference widths, Model B.
  learn : the TD-only call (avd_learn_set_split_td_f16x3, un-smoothed), the critic phase alone (avd_learn_set_split_critic) and the
          full call (avd_learn_set_split_f16x3), on the same inputs;
  update: avd_adam_polyak_delayed_f32 with policy 0 and 1 (AgentGroup.apply_delayed) and avd_adam_polyak_guarded_f32
          (AgentGroup.apply(guarded=True)), on a second group with the gradients of one learn call.
A window is `inner` back-to-back calls of one form between two HIP events (the updates: `inner` x 4, a call of a few microseconds
needs more of them between two events); one warm-up window per form, then the forms ALTERNATED for `reps` repeats. One JSON line per
form: min / median us per call and the spread (max - min) over the repeats. The TD-only call does strictly less work than the critic
phase, so it has to be faster by more than the larger of the two spreads: `td_faster_than_critic_phase` records whether it is, and
`ratio_to_full` stands beside the counted share of the matrix work (avd_learn_set_split_mfma_count's 3296 per tile against the TD
call's 2096).
usage: delay_time.py [reps] [inner] [out.json]   (out.json default: profiles/delay_time.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)  # the repository root
import torch

from avddpg_amd import config, vec

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
INNER = int(sys.argv[2]) if len(sys.argv) > 2 else 50
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "delay_time.json")
P, L = 4096, 5
TD, CRITIC, FULL = "avd_learn_set_split_td_f16x3", "avd_learn_set_split_critic", "avd_learn_set_split_f16x3"
SKIP, POLICY, GUARDED = "avd_adam_polyak_delayed_f32(policy=0)", "avd_adam_polyak_delayed_f32(policy=1)", "avd_adam_polyak_guarded_f32"
MFMA_FULL, MFMA_TD = 3296, 2096  # per tile (csrc/fsplit.hip MFMA_PER_TILE, MFMA_PER_TILE_TD)


def forms():
    conf = config.Config(pl_size=L, num_platoons=P, fed_method="interfrl")
    grp, upd = vec.AgentGroup(L, 4, 1, conf, seed=11), vec.AgentGroup(L, 4, 1, conf, seed=11)
    f32 = dict(dtype=torch.float32, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(3)
    rn = lambda *sh: torch.randn(*sh, generator=gen, **f32)
    n = P * L
    s, a, r, s2 = 1.5 * rn(n, 64, 4), 2.5 * (2 * torch.rand(n, 64, 1, generator=gen, **f32) - 1), -0.3 * rn(n, 64).abs(), 1.5 * rn(n, 64, 4)
    grads, losses = torch.zeros(L, grp.lay.theta_size, **f32), torch.zeros(L, 2, **f32)
    fixed = grp.learn_set_split(s, a, r, s2, n).clone()  # the updates' gradients

    def td():
        grp.learn_set_split_td(s, a, r, s2, n, grads=grads, losses=losses)

    def critic():
        grp.learn_set_fused(s, a, r, s2, n, grads=grads, losses=losses, split=True, phase="critic")

    def full():
        grp.learn_set_split(s, a, r, s2, n, grads=grads, losses=losses)

    return [(TD, td, 1), (CRITIC, critic, 1), (FULL, full, 1), (SKIP, lambda: upd.apply_delayed(fixed, False), 4),
            (POLICY, lambda: upd.apply_delayed(fixed, True), 4), (GUARDED, lambda: upd.apply(fixed, guarded=True), 4)], grads, upd


def window(fn, count):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(count):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / count  # us per call


def main():
    assert torch.cuda.is_available(), "a timing needs the GPU"
    med = lambda v: sorted(v)[len(v) // 2]
    fs, grads, upd = forms()
    for _, fn, k in fs:
        window(fn, INNER * k)  # warm-up
    us = {name: [] for name, _, _ in fs}
    for _ in range(REPS):
        for name, fn, k in fs:
            us[name].append(window(fn, INNER * k))
    assert bool(torch.isfinite(grads).all()), "non-finite gradients"
    assert int(upd.nonfinite_skipped.item()) == 0, "a guarded update skipped a set"
    spread = lambda name: max(us[name]) - min(us[name])
    lines = []
    for name, _, k in fs:
        v = us[name]
        line = dict(form=name, platoons=P, vehicles=L, reps=REPS, calls_per_window=INNER * k, us_min=round(min(v), 2), us_median=round(med(v), 2),
                    spread_us=round(spread(name), 2))
        if name == TD:
            line["median_minus_critic_phase_us"] = round(med(v) - med(us[CRITIC]), 2)
            line["td_faster_than_critic_phase"] = bool(med(us[CRITIC]) - med(v) > max(spread(TD), spread(CRITIC)))
            line["ratio_to_critic_phase"] = round(med(v) / med(us[CRITIC]), 5)
            line["ratio_to_full"] = round(med(v) / med(us[FULL]), 5)
            line["counted_mfma_ratio_to_full"] = round(MFMA_TD / MFMA_FULL, 5)
            d2 = (med(v) + med(us[SKIP]) + med(us[FULL]) + med(us[POLICY])) / (2 * (med(us[FULL]) + med(us[GUARDED])))
            line["learn_plus_update_at_delay_2_to_plain"] = round(d2, 5)
        if name in (SKIP, POLICY):
            line["ratio_to_guarded"] = round(med(v) / med(us[GUARDED]), 5)
        lines.append(line)
        print(json.dumps(line), flush=True)
    with open(OUT, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), note="same build, same process, forms alternated", forms=lines), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
