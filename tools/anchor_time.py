#!/usr/bin/env python3
"""Time the anchored learn call (avd_learn_set_split_anchor_f16x3: csrc/anchor.hip's seed and reducer in the chain of csrc/fsplit.hip)
beside avd_learn_set_split_f16x3 on the same inputs, in one process, at 4096 platoons x 5 vehicles (the headline shape): reference
widths, Model B, a per-vehicle gain table, weight 1.
A window is `inner` back-to-back calls of one form between two HIP events; one warm-up window per form, then the forms ALTERNATED for
`reps` repeats. One JSON line per form: min / median us per call and the spread (max - min) over the repeats; for the anchored call also
the difference of the medians -- what the anchored seed (20 more bytes read per row than actor_seed_kernel) and the reducer's launch
cost together. The two launches are not timed apart: the chain has no entry point that runs one kernel alone. No threshold: the
yardstick is the un-anchored call of the same process.
usage: anchor_time.py [reps] [inner] [out.json]   (out.json default: profiles/anchor_time.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)  # the repository root
import torch

from avddpg_amd import config, vec
from avddpg_amd.scenarios import Anchor

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
INNER = int(sys.argv[2]) if len(sys.argv) > 2 else 50
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "anchor_time.json")
P, L = 4096, 5


def forms():
    conf = config.Config(pl_size=L, num_platoons=P, fed_method="interfrl")
    grp = vec.AgentGroup(L, 4, 1, conf, seed=11)
    f32 = dict(dtype=torch.float32, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(3)
    rn = lambda *sh: torch.randn(*sh, generator=gen, **f32)
    n = P * L
    s, a, r, s2 = 1.5 * rn(n, 64, 4), 2.5 * (2 * torch.rand(n, 64, 1, generator=gen, **f32) - 1), -0.3 * rn(n, 64).abs(), 1.5 * rn(n, 64, 4)
    table = [[2.0 + 0.1 * m, 1.0, 0.0, 0.2] for m in range(L)]
    gains = torch.from_numpy(Anchor(table=table).gains(L)).cuda()
    grads, losses, al = torch.zeros(L, grp.lay.theta_size, **f32), torch.zeros(L, 2, **f32), torch.zeros(L, **f32)

    def plain():
        grp.learn_set_split(s, a, r, s2, n, grads=grads, losses=losses)

    def anchored():
        grp.learn_set_split_anchor(s, a, r, s2, n, gains, 1.0, al, grads=grads, losses=losses)

    return [("avd_learn_set_split_f16x3", plain), ("avd_learn_set_split_anchor_f16x3", anchored)], (grads, al)


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(INNER):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / INNER  # us per call


def main():
    assert torch.cuda.is_available(), "a timing needs the GPU"
    med = lambda v: sorted(v)[len(v) // 2]
    fs, (grads, al) = forms()
    for _, fn in fs:
        window(fn)  # warm-up
    us = {name: [] for name, _ in fs}
    for _ in range(REPS):
        for name, fn in fs:
            us[name].append(window(fn))
    assert bool(torch.isfinite(grads).all()) and bool((al > 0).all()), "non-finite gradients or no anchor loss"
    lines = []
    for name, _ in fs:
        v = us[name]
        line = dict(form=name, platoons=P, vehicles=L, reps=REPS, calls_per_window=INNER, us_min=round(min(v), 2), us_median=round(med(v), 2),
                    spread_us=round(max(v) - min(v), 2))
        if "anchor" in name:
            base = med(us["avd_learn_set_split_f16x3"])
            line["median_minus_unanchored_us"] = round(med(v) - base, 2)
            line["ratio_to_unanchored"] = round(med(v) / base, 5)
        lines.append(line)
        print(json.dumps(line), flush=True)
    with open(OUT, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), note="same build, same process, forms alternated", forms=lines), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
