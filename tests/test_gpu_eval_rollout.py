"""The evaluator rollout of many platoons' actors in one launch (avd_eval_rollout_f32, csrc/eval.hip; evaluator.run_many) against
the per-step launches of evaluator.run -- itself pinned to the reference goldens G8 / G9 and to the oracle
(tests/test_gpu_trainer.py) -- compared with ==: scores, float32 counters and every trace array. Then the end-of-training
simulation rewards of `tr` (workers/trainer.py:277-280, 537-550) and the --eval_platoons curve columns."""
import copy
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from avddpg_amd import config, evaluator, trainer, vec
from tests.gpu_util import need_gpu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _group(conf, n_sets, S, A, seed, hidd_mult=1, last_scale=40.0, spread=0.2):
    """n_sets visibly different actors: every actor weight scaled by its own (1 + spread * N(0, 1)) (zero padding stays
    zero), the last layer by last_scale as in tests/test_gpu_trainer.py:242 -- unsaturated, non-zero actions."""
    grp = vec.AgentGroup(n_sets, S, A, conf, seed=seed, hidd_mult=hidd_mult)
    lay = grp.lay
    g = torch.Generator(device="cuda").manual_seed(seed)
    act = grp.theta[:, :lay.actor_size]
    act.mul_(1.0 + spread * torch.randn(act.shape, device="cuda", generator=g))
    grp.theta[:, lay.aW3:lay.aW3 + lay.H2 * A] *= last_scale
    return grp


def _sets(grp, lo, n):
    """Weight sets lo .. lo + n as a group of their own (views): what evaluator.run addresses as a platoon's actors."""
    v = copy.copy(grp)
    v.theta, v.stats, v.theta_t, v.stats_t = (x[lo:lo + n] for x in (grp.theta, grp.stats, grp.theta_t, grp.stats_t))
    v.n_sets = n
    return v


def _with_seed(conf, seed):
    c = copy.copy(conf)
    c.evaluation_seed = seed
    return c


def _same(got, ref, what):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    bad = np.argwhere(got != ref)
    assert bad.size == 0, (what, bad[:4], got[tuple(bad[0])], ref[tuple(bad[0])])


def _check_per_agent(conf, grp, platoons, T, traced=(), seeds=None):
    """run_many on per-agent sets against evaluator.run platoon by platoon (and seed by seed): bit for bit."""
    M = 1 if conf.framework == conf.cntrl else conf.pl_size
    seeds = [conf.evaluation_seed] if seeds is None else list(seeds)
    trace = [(i, k) for i in traced for k in range(len(seeds))]
    sc, cnt, tr = evaluator.run_many(conf, grp, platoons, seeds=seeds, manual_timestep_override=T, trace=trace)
    assert sc.dtype == np.float32 and sc.shape == (len(platoons), len(seeds)) and cnt.shape == (len(platoons), len(seeds), M)
    for i, p in enumerate(platoons):
        for k, sd in enumerate(seeds):
            r, t = evaluator.run(conf=_with_seed(conf, sd), actors=_sets(grp, p * M, M), pl_idx=p + 1, manual_timestep_override=T)
            assert sc[i, k] == r, (p, sd, sc[i, k], r)
            _same(cnt[i, k], t["counters"], ("counters", p, sd))
            if (i, k) in tr:
                for key in ("states", "inputs", "jerks", "leader", "counters"):
                    _same(tr[(i, k)][key], t[key], (key, p, sd))
    return sc, cnt, tr


def test_per_agent_sets_bitwise_equal_to_the_evaluator_at_full_episode_length():
    """24 platoons x 5 vehicles, 120 different actors, the full 600-step episode: scores and counters of every platoon, the
    whole traces of the first, a middle and the last platoon."""
    need_gpu()
    P, L = 24, 5
    conf = config.Config(pl_size=L, num_platoons=P)
    grp = _group(conf, P * L, 4, 1, seed=11)
    sc, cnt, tr = _check_per_agent(conf, grp, range(P), conf.steps_per_episode, traced=(0, P // 2, P - 1))
    u = np.abs(tr[(0, 0)]["inputs"])
    assert np.any((u > 0.05) & (u < conf.action_high))  # non-zero, unsaturated actions
    assert len(set(sc[:, 0].tolist())) > 1  # the platoons' actors really differ


@pytest.mark.parametrize("model", ["ModelA", "ModelB"])
@pytest.mark.parametrize("method", ["euler", "exact"])
@pytest.mark.parametrize("L", [1, 3, 16])
def test_configuration_matrix_bitwise(model, method, L):
    need_gpu()
    conf = config.Config(pl_size=L, model=model, method=method)
    S = 3 if model == "ModelA" else 4
    grp = _group(conf, 3 * L, S, 1, seed=20 + L)
    _check_per_agent(conf, grp, [0, 1, 2], 300, traced=(1,))


def test_uniform_leader_inputs_and_centralized_bitwise():
    need_gpu()
    conf = config.Config(pl_size=3, rand_gen="uniform")
    _check_per_agent(conf, _group(conf, 9, 4, 1, seed=31), [0, 1, 2], 300, traced=(2,))
    L = 3
    conf = config.Config(pl_size=L, framework="centralized")
    grp = _group(conf, 3, 4 * L, L, seed=32, hidd_mult=conf.centrl_hidd_mult)
    assert (grp.lay.H1, grp.lay.H2) == (320, 160)
    _, _, tr = _check_per_agent(conf, grp, [0, 1, 2], 300, traced=(0, 2))
    assert tr[(0, 0)]["states"].shape == (300, L, 4) and np.abs(tr[(0, 0)]["inputs"]).max() > 0.05


def test_terminal_reward_branch_bitwise():
    """Actors pushed to a near-constant full-scale action drive the followers past max_ep / max_ev: the terminal reward is used
    (the rollout does not stop), and can_terminate=False gives a different result -- both bit for bit."""
    need_gpu()
    L = 3
    out = {}
    for can in (True, False):
        conf = config.Config(pl_size=L, can_terminate=can)
        grp = _group(conf, 2 * L, 4, 1, seed=41)
        lay = grp.lay
        grp.theta[:, lay.aW3:lay.aW3 + lay.H2] = 0.0
        grp.theta[:, lay.ab3] = 3.0  # tanh(3) * 2.5: every vehicle accelerates whatever the state
        sc, cnt, tr = _check_per_agent(conf, grp, [0, 1], 600, traced=(0,))
        st = tr[(0, 0)]["states"]
        assert (np.abs(st[..., 0]) > conf.max_ep).any() or (np.abs(st[..., 1]) > conf.max_ev).any()
        out[can] = (sc, cnt)
    assert not np.array_equal(out[True][1], out[False][1])


def test_shared_sets_of_an_interfrl_trainer():
    """interfrl + gradients with every step federated keeps ONE set per vehicle index (VecTrainer.shared): with set_mod = M
    every platoon's result equals evaluator.run(set_mod=M) on the trained actors; run_simulations divides by re_scalar."""
    need_gpu()
    conf = config.Config(num_platoons=6, pl_size=3, buffer_size=128, fed_method="interfrl", weighted_average_enabled=False,
                         re_scalar=2.0)
    vt = trainer.VecTrainer(conf, rng="device", auto_reset=True)
    assert vt.shared
    vt.reset_episode()
    for _ in range(80):
        vt.step()
    torch.cuda.synchronize()
    sc, cnt, tr = evaluator.run_many(conf, vt.agents, range(vt.P), set_mod=vt.M, trace=[0, vt.P - 1])
    r, t = evaluator.run(conf=conf, actors=vt.agents, pl_idx=1, set_mod=vt.M)
    assert sc.shape == (vt.P, 1) and np.all(sc == r)
    for p in range(vt.P):
        _same(cnt[p, 0], t["counters"], ("counters", p))
    for key in ("states", "inputs", "jerks"):
        _same(tr[(vt.P - 1, 0)][key], t[key], key)
    assert vt.run_simulations() == [float(r / conf.re_scalar)] * vt.P


def test_seeds_bitwise_and_global_rng_restored():
    need_gpu()
    L = 4
    conf = config.Config(pl_size=L)
    grp = _group(conf, 3 * L, 4, 1, seed=51)
    np.random.seed(1234)
    np.random.normal()
    before = np.random.get_state()
    seeds = [6, 0, 1, 2, 99, 12345, 7, 2 ** 31 - 1]
    sc, _, _ = evaluator.run_many(conf, grp, [0, 1, 2], seeds=seeds, manual_timestep_override=200, trace=[(1, 3)])
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert len(set(sc[0].tolist())) > 1  # the seeds give different start states / leader inputs
    _check_per_agent(conf, grp, [0, 1, 2], 200, traced=(1,), seeds=seeds)


def test_two_platoons_against_the_oracle_rollout():
    """The same tolerances as tests/test_gpu_trainer.py:246-248."""
    need_gpu()
    from oracle import evaluator as oeval
    from oracle import platoon as oplatoon

    L = 3
    conf = config.Config(pl_size=L)
    grp = _group(conf, 2 * L, 4, 1, seed=61)
    sc, _, tr = evaluator.run_many(conf, grp, [0, 1], manual_timestep_override=100, trace=[0, 1])
    for p in range(2):
        actors = [[w.astype(np.float64) for w in grp.get_weights(p * L + m, "actor")] for m in range(L)]
        o_rew, o_tr = oeval.run(oplatoon.EnvParams(), L, actors, 100)
        got = tr[(p, 0)]
        assert abs(sc[p, 0] - o_rew) <= 2e-3 and np.abs(o_tr["inputs"]).max() > 0.05
        assert np.allclose(got["inputs"], o_tr["inputs"], atol=5e-5)
        assert np.allclose(got["states"], o_tr["states"], atol=2e-4, rtol=1e-4)
        assert np.allclose(got["jerks"], o_tr["jerks"], atol=5e-3)


def _big_group(conf, n_sets, S, A, seed):
    """n_sets perturbed actors in theta / stats slabs only (no target / Adam slabs: 4 x less memory than an AgentGroup)."""
    small = _group(conf, 1, S, A, seed=seed, spread=0.0)
    g = copy.copy(small)
    lay = small.lay
    g.theta = small.theta[0:1].expand(n_sets, lay.theta_size).contiguous()
    g.stats = small.stats[0:1].expand(n_sets, lay.stats_size).contiguous()
    gen = torch.Generator(device="cuda").manual_seed(seed)
    for lo in range(0, n_sets, 2048):
        blk = g.theta[lo:lo + 2048, :lay.actor_size]
        blk.mul_(1.0 + 0.2 * torch.randn(blk.shape, device="cuda", generator=gen))
    g.theta_t, g.stats_t, g.n_sets = g.theta, g.stats, n_sets
    return g


def test_at_size_4096_platoons_of_5_in_one_launch():
    """4096 x 5 per-agent actors at the reference widths, 600 steps, one launch: 8 sampled platoons bit for bit, the kernel
    <= 1.0 s (events, after one warm-up); then hidden-1024 shared actors (BASELINE config 5 widths) over 16 seeds."""
    need_gpu()
    P, L, T = 4096, 5, 600
    conf = config.Config(pl_size=L, num_platoons=P)
    grp = _big_group(conf, P * L, 4, 1, seed=71)
    b = evaluator.prepare_many(conf, grp, range(P), manual_timestep_override=T)
    b.launch()  # warm-up
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    b.launch()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    sc, cnt, _ = b.results()
    assert np.isfinite(cnt).all()
    print(f"eval rollout 4096 x 5, T = 600: {ms:.1f} ms")
    for p in (0, 1, 777, 1500, 2048, 3001, 4000, P - 1):
        r, t = evaluator.run(conf=conf, actors=_sets(grp, p * L, L), pl_idx=p + 1, manual_timestep_override=T)
        assert sc[p, 0] == r, (p, sc[p, 0], r)
        _same(cnt[p, 0], t["counters"], ("counters", p))
    assert ms <= 1000.0, f"{ms:.1f} ms"
    del grp, b
    torch.cuda.empty_cache()
    conf = config.Config(pl_size=L, actor_layer1_size=1024, actor_layer2_size=1024, critic_layer1_size=1024, critic_layer2_size=1024)
    wide = _group(conf, L, 4, 1, seed=72, last_scale=20.0)
    assert (wide.lay.H1, wide.lay.H2) == (1024, 1024)
    seeds = list(range(100, 116))
    sc, cnt, tr = evaluator.run_many(conf, wide, range(3), set_mod=L, seeds=seeds, trace=[(2, 15)])
    for k, sd in enumerate(seeds):
        r, t = evaluator.run(conf=_with_seed(conf, sd), actors=wide, pl_idx=1, set_mod=L)
        assert np.all(sc[:, k] == r), (sd, sc[:, k], r)
        for i in range(3):
            _same(cnt[i, k], t["counters"], ("counters", i, sd))
        if k == 15:
            for key in ("states", "inputs", "jerks"):
                _same(tr[(2, 15)][key], t[key], key)


def _tr(tmp_path, *extra):
    cmd = [sys.executable, "-m", "avddpg_amd", "tr", "--pl_num", "3", "--pl_size", "2", "--buffer_size", "500", "--out", str(tmp_path),
           *extra]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout.strip().splitlines()[-1]


def test_cli_writes_the_simulation_rewards_and_the_curve_columns(tmp_path):
    """`tr` ends as the reference's Trainer.run: conf.json carries pl_rews_for_simulations (one evaluator score / re_scalar per
    platoon, here recomputed from the saved actors with evaluator.run) and pl_rew_for_simulation (their average).
    --episodes platoon --eval_platoons all appends evaluator_mean,evaluator_min,evaluator_max to curve.csv; without the flag the
    header is unchanged."""
    need_gpu()
    from avddpg_amd import artifacts
    from avddpg_amd.config import Config

    base = _tr(tmp_path / "ref", "--total_time_steps", "1200")
    js = json.load(open(os.path.join(base, "conf.json")))
    sims = js["pl_rews_for_simulations"]
    assert len(sims) == 3 and js["pl_rew_for_simulation"] == float(np.average(sims))
    conf = artifacts.config_loader(os.path.join(base, "conf.json"), Config)
    for p in range(1, 4):
        grp = vec.AgentGroup(2, 4, 1, conf)
        for m in range(2):
            grp.set_weights(m, "actor", artifacts.load_actor_weights(base, p, m + 1))
        r, _ = evaluator.run(conf=conf, actors=grp, pl_idx=p)
        assert sims[p - 1] == float(r / conf.re_scalar), (p, sims, r)
    assert len(set(sims)) > 1

    dev = ("--total_time_steps", "200", "--rng", "device", "--episodes", "platoon", "--report_every", "100")
    base = _tr(tmp_path / "curve", *dev, "--eval_platoons", "all")
    rows = list(csv.reader(open(os.path.join(base, "curve.csv"))))
    assert rows[0] == ["step", "episodes_closed", "mean_episodic_reward", "mean_episode_length", "evaluator_score", "evaluator_mean",
                       "evaluator_min", "evaluator_max"]
    assert len(rows) == 1 + 3 and all(len(r) == 8 for r in rows)
    for r in rows[1:]:
        lo, mean, hi = float(r[6]), float(r[5]), float(r[7])
        assert lo <= mean <= hi < 0
    js = json.load(open(os.path.join(base, "conf.json")))
    assert len(js["pl_rews_for_simulations"]) == 3 and "pl_rew_for_simulation" in js
    base = _tr(tmp_path / "plain", *dev)
    assert open(os.path.join(base, "curve.csv")).readline() == \
        "step,episodes_closed,mean_episodic_reward,mean_episode_length,evaluator_score\n"
