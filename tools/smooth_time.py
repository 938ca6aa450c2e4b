#!/usr/bin/env python3
"""Time the smoothed learn call (avd_learn_set_split_smooth_f16x3 at sigma > 0: csrc/smooth.hip's launch in the chain of
csrc/fsplit.hip) beside avd_learn_set_split_f16x3 on the same inputs, and the smoothing launch on its own (avd_target_smooth_f32 on a
[n_agents, 64] buffer), in one process, at 4096 platoons x 5 vehicles (the headline shape): reference widths, Model B, sigma 0.2,
clip 0.5.
A window is `inner` back-to-back calls of one form between two HIP events; one warm-up window per form, then the forms ALTERNATED for
`reps` repeats. One JSON line per form: min / median us per call and the spread (max - min) over the repeats; for the smoothed call also
the difference of the medians -- what the one extra launch costs inside the chain. The stand-alone launch is timed in windows of
`inner` x 4 launches (a launch of a few microseconds needs more of them between two events). No threshold: the yardstick is the
un-smoothed call of the same process.
usage: smooth_time.py [reps] [inner] [out.json]   (out.json default: profiles/smooth_time.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)  # the repository root
import torch

from avddpg_amd import config, vec
from avddpg_amd.trainer import TargetNoise

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
INNER = int(sys.argv[2]) if len(sys.argv) > 2 else 50
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "smooth_time.json")
P, L = 4096, 5
PLAIN, SMOOTH, ALONE = "avd_learn_set_split_f16x3", "avd_learn_set_split_smooth_f16x3", "avd_target_smooth_f32"


def forms():
    conf = config.Config(pl_size=L, num_platoons=P, fed_method="interfrl")
    grp = vec.AgentGroup(L, 4, 1, conf, seed=11)
    f32 = dict(dtype=torch.float32, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(3)
    rn = lambda *sh: torch.randn(*sh, generator=gen, **f32)
    n = P * L
    s, a, r, s2 = 1.5 * rn(n, 64, 4), 2.5 * (2 * torch.rand(n, 64, 1, generator=gen, **f32) - 1), -0.3 * rn(n, 64).abs(), 1.5 * rn(n, 64, 4)
    tn = TargetNoise(0.2)
    grads, losses = torch.zeros(L, grp.lay.theta_size, **f32), torch.zeros(L, 2, **f32)
    a2 = 2.5 * torch.tanh(rn(n, 64))
    calls = [0]

    def plain():
        grp.learn_set_split(s, a, r, s2, n, grads=grads, losses=losses)

    def smoothed():
        grp.learn_set_split_smooth(s, a, r, s2, n, tn, calls[0], grads=grads, losses=losses, M=L, seed=7)
        calls[0] += 1

    def alone():
        grp.target_smooth(a2, tn, calls[0], M=L, seed=7)
        calls[0] += 1

    return [(PLAIN, plain, 1), (SMOOTH, smoothed, 1), (ALONE, alone, 4)], grads, n


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
    fs, grads, n = forms()
    for _, fn, k in fs:
        window(fn, INNER * k)  # warm-up
    us = {name: [] for name, _, _ in fs}
    for _ in range(REPS):
        for name, fn, k in fs:
            us[name].append(window(fn, INNER * k))
    assert bool(torch.isfinite(grads).all()), "non-finite gradients"
    lines = []
    for name, _, k in fs:
        v = us[name]
        line = dict(form=name, platoons=P, vehicles=L, reps=REPS, calls_per_window=INNER * k, us_min=round(min(v), 2), us_median=round(med(v), 2),
                    spread_us=round(max(v) - min(v), 2))
        if name == SMOOTH:
            base = med(us[PLAIN])
            line["median_minus_unsmoothed_us"] = round(med(v) - base, 2)
            line["ratio_to_unsmoothed"] = round(med(v) / base, 5)
        if name == ALONE:
            line["bytes_moved"] = 2 * 4 * 64 * n  # one 16-byte load and store per four rows
            line["gb_per_s_at_median"] = round(line["bytes_moved"] / med(v) / 1e3, 1)
        lines.append(line)
        print(json.dumps(line), flush=True)
    with open(OUT, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), note="same build, same process, forms alternated", forms=lines), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
