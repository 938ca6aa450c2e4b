"""Keeping the best actors seen (`tr --keep_best`): what the keep launches, a whole evaluation and the flag on a headline run cost.

Alternated rounds in one process, device events around each call after a warm-up:
  * keep_alone: avd_keep_best_f32 alone at 4096 x 5 per-agent sets (4096 units of M = 5 sets, 20 480 sets, the reference layout)
    with EVERY unit improving (best scores reset to -inf before the call) and with NONE improving (reset to +inf). Bytes moved
    when all improve = 2 x units x M x (actor_size + cmms) x 4 B, read once and written once; none when none does.
  * evaluation: VecTrainer.keep_best_update (the rollout launch + the keep launches) at 4096 x 5 nofrl per-agent sets -- 4096 rollouts --
    and at 4096 x 5 interfrl shared sets -- one rollout --, again with every unit and with no unit improving.
  * headline: 4096 x 5 interfrl, the fused3 engine, --steps steps per round with an evaluation at the round's first and last step
    (`--keep_best STEPS` on a run of STEPS steps) against the same steps without: one trainer, the rounds alternate, host clock between
    device synchronisations. The rounds without are what the run does without the flag.

Writes --out (default profiles/keep_best_time.json) and prints the same JSON.

  python tools/keep_best_time.py [--reps 20] [--steps 10000] [--rounds 2] [--only keep|evaluation|headline] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from avddpg_amd import _hip, config, trainer  # noqa: E402
from avddpg_amd._hip import call, ptr, stream_handle  # noqa: E402

INF = float("inf")


def _stats(ms):
    ms = sorted(ms)
    return dict(median_ms=round(ms[len(ms) // 2], 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4), n=len(ms))


def _alternate(arms, reps, warmup=3):
    """arms: {name: (prepare, run)}; each round runs every arm once, prepare outside the event bracket. -> {name: [ms]}"""
    out = {n: [] for n in arms}
    for r in range(warmup + reps):
        for name, (prepare, run) in arms.items():
            prepare()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            if r >= warmup:
                out[name].append(e0.elapsed_time(e1))
    return out


def keep_alone(reps, P=4096, M=5, NS=1):
    lay = _hip.make_layout(4, 1, 256, 128, 48, 64)
    n_sets, f32 = P * M, dict(dtype=torch.float32, device="cuda")
    theta, stats = torch.randn(n_sets, lay.theta_size, **f32), torch.randn(n_sets, lay.stats_size, **f32)
    best_theta, best_stats = torch.zeros(n_sets, lay.actor_size, **f32), torch.zeros(n_sets, lay.cmms, **f32)
    score = torch.zeros(P, **f32)
    step, improved = torch.zeros(P, dtype=torch.int64, device="cuda"), torch.zeros(P, dtype=torch.int32, device="cuda")
    base = [u * M for u in range(P)]
    h_base, d_base = (ctypes.c_int32 * P)(*base), torch.tensor(base, dtype=torch.int32, device="cuda")
    counters = -torch.rand(P * NS, M, **f32)
    run = lambda: call("avd_keep_best_f32", ctypes.byref(lay), P, M, NS, n_sets, ptr(d_base), h_base, ptr(counters), ptr(theta), ptr(stats),
                       7, ptr(best_theta), ptr(best_stats), ptr(score), ptr(step), ptr(improved), stream_handle())
    ms = _alternate(dict(all_improve=(lambda: score.fill_(-INF), run), none_improves=(lambda: score.fill_(INF), run)), reps)
    nbytes = 2 * n_sets * (lay.actor_size + lay.cmms) * 4
    out = dict(units=P, M=M, NS=NS, bytes_when_all_improve=nbytes, all_improve=_stats(ms["all_improve"]), none_improves=_stats(ms["none_improves"]))
    out["all_improve"]["GB_per_s"] = round(nbytes / out["all_improve"]["median_ms"] / 1e6, 1)
    return out


def _headline_trainer(mode, P=4096, L=5):
    conf = config.Config(num_platoons=P, pl_size=L, buffer_size=1000, fed_method="interfrl" if mode == "interfrl" else "normal",
                         weighted_average_enabled=False, random_seed=1)
    vt = trainer.VecTrainer(conf, rng="device", auto_reset=True, seed=1, fused_update=mode == "nofrl",
                            shared_engine="fused3" if mode == "interfrl" else None)
    vt.reset_episode()
    return vt


def evaluation(reps, mode):
    vt = _headline_trainer(mode)
    vt.enable_keep_best()
    k = vt._keep
    run = lambda: vt.keep_best_update(1)
    ms = _alternate(dict(all_improve=(lambda: k["score"].fill_(-INF), run), none_improves=(lambda: k["score"].fill_(INF), run),
                         rollout_alone=(lambda: None, k["batch"].launch)), reps)
    return dict(mode=mode, units=k["n_units"], M=vt.M, NS=k["NS"], rollouts=k["batch"].n_roll, T=k["batch"].T,
                **{n: _stats(v) for n, v in ms.items()})


def headline(steps, rounds, warm=200):
    vt = _headline_trainer("interfrl")
    vt.enable_keep_best()
    for _ in range(warm):
        vt.step()
    vt.keep_best_update(0)
    torch.cuda.synchronize()
    res = dict(with_keep_best=[], without=[])
    for _ in range(rounds):
        for arm in ("without", "with_keep_best"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if arm == "with_keep_best":
                vt.keep_best_update(0)
            for _ in range(steps):
                vt.step()
            if arm == "with_keep_best":
                vt.keep_best_update(steps)
            torch.cuda.synchronize()
            res[arm].append(time.perf_counter() - t0)
    a, b = float(np.median(res["with_keep_best"])), float(np.median(res["without"]))
    return dict(workload="4096 x 5 interfrl fused3", steps_per_round=steps, rounds=rounds, evaluations_per_round=2,
                seconds_with=[round(x, 4) for x in res["with_keep_best"]], seconds_without=[round(x, 4) for x in res["without"]],
                step_ms_without=round(1e3 * b / steps, 4), extra_seconds_per_round=round(a - b, 4), relative_cost=round((a - b) / b, 6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--only", choices=["keep", "evaluation", "headline"], default=None)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "keep_best_time.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "keep_best_time.py measures on the GPU"
    torch.cuda.set_device(0)
    out = dict(device=torch.cuda.get_device_name(0))
    if args.only in (None, "keep"):
        out["keep_alone"] = keep_alone(args.reps)
        torch.cuda.empty_cache()
    if args.only in (None, "evaluation"):
        out["evaluation"] = [evaluation(args.reps, "nofrl"), evaluation(args.reps, "interfrl")]
        torch.cuda.empty_cache()
    if args.only in (None, "headline"):
        out["headline"] = headline(args.steps, args.rounds)
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
