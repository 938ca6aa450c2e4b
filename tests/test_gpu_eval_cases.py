"""The scenario evaluator (avd_eval_cases_f32, csrc/evalx.hip; evaluator.run_cases): every platoon's actors over leader scenarios x
evaluation seeds in one launch, each weight element read once per block of cases. The yardstick is the existing rollout kernel
(avd_eval_rollout_f32 through a RolloutBatch, whose public `leader` tensor is overwritten with the scenario's profile before the
launch): counters compared with ==, metrics with == against scenarios.metrics_from_traces on the yardstick's traces. Then the float64
restatement written from the oracle (tests/scenario_oracle.py), VecTrainer.evaluate_scenarios and the CLI."""
import copy
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from avddpg_amd import _hip, config, evaluator, scenarios, trainer
from tests import scenario_oracle as so
from tests.gpu_util import need_gpu
from tests.test_gpu_eval_rollout import _big_group, _group, _same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _blocks(L):
    """Every block size the host can pick at this L."""
    blk = _hip.lib().avd_eval_cases_block
    return sorted({blk(K, L) for K in range(1, 200)})


def _yardstick(conf, grp, platoons, names, seeds, T=None, amp=None, period_s=10.0, **kw):
    """The existing kernel on the same cases: per scenario one RolloutBatch over platoons x seeds with every rollout traced and, for
    the other scenarios than gaussian, its leader rows overwritten with the profile. -> counters [NP, scen, seed, M], metrics
    {name: [NP, scen, seed, L]} from metrics_from_traces, traces {(i, c, k): dict}."""
    NP, NS = len(platoons), len(seeds)
    cnts, mets, traces = [], [], {}
    for c, name in enumerate(names):
        b = evaluator.prepare_many(conf, grp, platoons, seeds=seeds, manual_timestep_override=T,
                                   trace=[(i, k) for i in range(NP) for k in range(NS)], **kw)
        if name != "gaussian":
            row = torch.from_numpy(scenarios.leader_profile(name, b.T, conf, amp, period_s)).to(b.leader.device)
            b.leader.copy_(row.expand_as(b.leader))
        b.launch()
        _, cnt, tr = b.results()
        x0 = b.x0.cpu().numpy()
        cnts.append(cnt)
        m = [[scenarios.metrics_from_traces(tr[(i, k)], x0[k], conf) for k in range(NS)] for i in range(NP)]
        mets.append({n: np.array([[m[i][k][n] for k in range(NS)] for i in range(NP)]) for n in scenarios.METRICS})
        for (i, k), t in tr.items():
            traces[(i, c, k)] = t
    return np.stack(cnts, axis=1), {n: np.stack([m[n] for m in mets], axis=1) for n in scenarios.METRICS}, traces


def _check_gaussian(conf, grp, platoons, seeds, T, **kw):
    """run_cases(("gaussian",), seeds) against run_many(seeds=seeds): scores and counters bit for bit."""
    sc, cnt, _ = evaluator.run_many(conf, grp, platoons, seeds=seeds, manual_timestep_override=T, **kw)
    r = evaluator.run_cases(conf, grp, platoons, ("gaussian",), seeds=seeds, manual_timestep_override=T, **kw)
    assert r.scores.shape == (len(platoons), 1, len(seeds)) and r.scenarios == ["gaussian"] and r.seeds == list(seeds)
    _same(r.scores[:, 0], sc, "scores")
    _same(r.counters[:, 0], cnt, "counters")
    assert np.isfinite(cnt).all() and all(np.isfinite(v).all() for v in r.metrics.values())
    return r


@pytest.mark.parametrize("L", [1, 3, 5, 16])
def test_gaussian_cases_equal_run_many_at_every_block_size_and_tail(L):
    """K in {1, RB - 1, RB, RB + 1, 3 RB + 2} for every block size RB the host can pick at this L (per-agent sets)."""
    need_gpu()
    conf = config.Config(pl_size=L)
    grp = _group(conf, 3 * L, 4, 1, seed=100 + L)
    sizes = _blocks(L)
    assert len(sizes) >= 3 and all(rb * L <= 256 for rb in sizes)
    Ks = sorted({K for rb in sizes for K in (1, rb - 1, rb, rb + 1, 3 * rb + 2) if K >= 1})
    used = set()
    for K in Ks:
        b = evaluator.prepare_cases(conf, grp, [0, 1, 2], ("gaussian",), seeds=range(50, 50 + K), manual_timestep_override=40)
        assert b.block == _hip.lib().avd_eval_cases_block(K, L) and b.K == K
        used.add(b.block)
        r = _check_gaussian(conf, grp, [0, 1, 2], list(range(50, 50 + K)), 40)
        assert len({tuple(x) for x in r.counters[:, 0, :, 0].T.tolist()}) == K or K == 1  # the seeds' cases differ
    assert used == set(sizes)


@pytest.mark.parametrize("model", ["ModelA", "ModelB"])
@pytest.mark.parametrize("method", ["euler", "exact"])
@pytest.mark.parametrize("L", [1, 3, 16])
def test_configuration_matrix_bitwise(model, method, L):
    need_gpu()
    conf = config.Config(pl_size=L, model=model, method=method)
    S = 3 if model == "ModelA" else 4
    grp = _group(conf, 3 * L, S, 1, seed=20 + L)
    _check_gaussian(conf, grp, [2, 0, 1], [6, 0, 1, 2, 99, 12345], 200)  # K = 6: a block of 8 with a tail
    names = ["step", "sine"]
    r = evaluator.run_cases(conf, grp, [0, 1, 2], names, seeds=[6, 7], manual_timestep_override=120)
    cnt, met, _ = _yardstick(conf, grp, [0, 1, 2], names, [6, 7], T=120)
    _same(r.counters, cnt, "counters")
    for n in scenarios.METRICS:
        _same(r.metrics[n], met[n], n)


def test_shared_sets_set_bases_centralized_and_uniform_inputs():
    need_gpu()
    L = 5
    conf = config.Config(pl_size=L, rand_gen="uniform")
    grp = _group(conf, 3 * L, 4, 1, seed=31)
    seeds = [6, 7, 8, 9, 10]
    r = _check_gaussian(conf, grp, range(4), seeds, 150, set_mod=L)  # shared sets: ONE group, repeated per platoon
    assert all(np.array_equal(r.counters[0], r.counters[p]) for p in range(4))
    r = _check_gaussian(conf, grp, range(3), seeds, 150, set_mod=L, set_bases=[2 * L, 0, L])
    assert not np.array_equal(r.counters[0], r.counters[1])
    per = _check_gaussian(conf, grp, [2, 0, 1], seeds, 150)
    _same(per.counters, r.counters, "set_bases against per-agent sets")
    L = 3
    conf = config.Config(pl_size=L, framework="centralized", rand_gen="uniform")
    cen = _group(conf, 3, 4 * L, L, seed=32, hidd_mult=conf.centrl_hidd_mult)
    assert (cen.lay.H1, cen.lay.H2) == (320, 160)
    r = _check_gaussian(conf, cen, [0, 1, 2], seeds, 150)
    assert r.counters.shape == (3, 1, 5, 1) and r.metrics["sum_u2"].shape == (3, 1, 5, L)
    names = ["brake", "ramp"]
    r = evaluator.run_cases(conf, cen, [0, 1, 2], names, seeds=[6, 7], manual_timestep_override=120)
    cnt, met, _ = _yardstick(conf, cen, [0, 1, 2], names, [6, 7], T=120)
    _same(r.counters, cnt, "centralized counters")
    for n in scenarios.METRICS:
        _same(r.metrics[n], met[n], n)


def test_six_scenarios_two_seeds_eight_platoons_against_the_rollout_kernel():
    """All six scenarios x 2 seeds on 8 platoons x 5, the full episode: counters equal the overwritten-leader RolloutBatch, metrics equal
    metrics_from_traces on its traces; the gaussian profile is _start's own draws; the caller's RNG state is restored."""
    need_gpu()
    P, L = 8, 5
    conf = config.Config(pl_size=L, num_platoons=P)
    grp = _group(conf, P * L, 4, 1, seed=11)
    names, seeds = ["zero", "step", "ramp", "brake", "sine", "gaussian"], [6, 41]
    np.random.seed(1234)
    before = np.random.get_state()
    r = evaluator.run_cases(conf, grp, range(P), names, seeds=seeds)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    T = conf.steps_per_episode
    assert r.T == T and r.scores.shape == (P, 6, 2) and r.scores.dtype == np.float32 and r.counters.shape == (P, 6, 2, L)
    cnt, met, tr = _yardstick(conf, grp, range(P), names, seeds)
    _same(r.counters, cnt, "counters")
    for n in scenarios.METRICS:
        assert r.metrics[n].shape == (P, 6, 2, L)
        _same(r.metrics[n], met[n], n)
    for i in range(P):
        for c in range(6):
            for k in range(2):
                assert r.scores[i, c, k] == round(np.average(cnt[i, c, k]), 3)
    for k, sd in enumerate(seeds):
        _same(scenarios.leader_profile("gaussian", T, conf, seed=sd), evaluator._start(conf, True, None, evaluation_seed=sd)[1], "gaussian")
        _same(tr[(0, 5, k)]["leader"], scenarios.leader_profile("gaussian", T, conf, seed=sd), "leader")
    # the scenarios do different things to the platoon, the seeds only to the gaussian one (same start state otherwise)
    assert len({r.counters[0, c, 0].tobytes() for c in range(6)}) == 6
    assert np.array_equal(r.counters[:, :5, 0], r.counters[:, :5, 1]) and not np.array_equal(r.counters[:, 5, 0], r.counters[:, 5, 1])
    u = np.abs(tr[(0, 1, 0)]["inputs"])
    assert np.any((u > 0.05) & (u < conf.action_high))
    s = r.summary()
    assert s["ss_ratio"].shape == (P, 6, 2, L) and s["string_stable"].shape == (P, 6, 2) and np.isnan(s["ss_ratio"][..., 0]).all()
    assert np.array_equal(s["rms_u"], np.sqrt(r.metrics["sum_u2"] / np.float32(T)))


def test_terminal_branch_metrics():
    """The recipe of test_terminal_reward_branch_bitwise: actors pushed to a near-constant full-scale action drive the followers past
    max_ep / max_ev. term_steps > 0 with the first terminal step where the yardstick's own traces first cross a bound; none with
    can_terminate = False."""
    need_gpu()
    L = 3
    names, seeds = ["gaussian", "step"], [6]
    out = {}
    for can in (True, False):
        conf = config.Config(pl_size=L, can_terminate=can)
        grp = _group(conf, 2 * L, 4, 1, seed=41)
        lay = grp.lay
        grp.theta[:, lay.aW3:lay.aW3 + lay.H2] = 0.0
        grp.theta[:, lay.ab3] = 3.0  # tanh(3) * 2.5: every vehicle accelerates whatever the state
        r = evaluator.run_cases(conf, grp, [0, 1], names, seeds=seeds)
        cnt, met, tr = _yardstick(conf, grp, [0, 1], names, seeds)
        _same(r.counters, cnt, "counters")
        for n in scenarios.METRICS:
            _same(r.metrics[n], met[n], n)
        st = tr[(0, 0, 0)]["states"]  # the yardstick's own traces cross a bound: the case cannot pass vacuously
        cross = (np.abs(st[..., 0]) > conf.max_ep) | (np.abs(st[..., 1]) > conf.max_ev)  # [T, L] on POST-step states
        assert cross[:-1].any()
        if can:
            assert (r.metrics["term_steps"][0, 0, 0] > 0).any()
            for v in range(L):
                hit = np.flatnonzero(cross[:-1, v])  # crossing after step t makes step t + 1's pre-step test fire
                assert r.metrics["first_term"][0, 0, 0, v] == (hit[0] + 1 if hit.size else -1)
                assert r.metrics["term_steps"][0, 0, 0, v] == hit.size
        else:
            assert (r.metrics["term_steps"] == 0).all() and (r.metrics["first_term"] == -1).all()
        out[can] = r.counters
    assert not np.array_equal(out[True], out[False])


def test_two_platoons_against_the_float64_restatement():
    """step and brake on two platoons against the float64 loop written from the oracle, at the tolerances
    tests/test_gpu_eval_rollout.py:182-184 holds the traces to (tests/scenario_oracle.check_against)."""
    need_gpu()
    L, T = 3, 100
    conf = config.Config(pl_size=L)
    grp = _group(conf, 2 * L, 4, 1, seed=61)
    names = ["step", "brake"]
    r = evaluator.run_cases(conf, grp, [0, 1], names, manual_timestep_override=T)
    for p in range(2):
        actors = [[w.astype(np.float64) for w in grp.get_weights(p * L + m, "actor")] for m in range(L)]
        for c, name in enumerate(names):
            ref, _, tr = so.rollout(so.env_params(conf), L, actors, scenarios.leader_profile(name, T, conf), conf.evaluation_seed)
            assert np.abs(tr["inputs"]).max() > 0.05
            so.check_against({n: r.metrics[n][p, c, 0] for n in scenarios.METRICS}, ref, T)


def test_at_size_4096_platoons_of_5_times_16_seeds_in_one_launch():
    """4096 x 5 per-agent actors x K = 16 (gaussian x 16 seeds, T = 600): one launch, equal to run_many(seeds=range(16)) bit for bit.
    Each side runs once."""
    need_gpu()
    P, L, T = 4096, 5, 600
    conf = config.Config(pl_size=L, num_platoons=P)
    grp = _big_group(conf, P * L, 4, 1, seed=71)
    seeds = list(range(16))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    b = evaluator.prepare_cases(conf, grp, range(P), ("gaussian",), seeds=seeds, manual_timestep_override=T)
    assert (b.G, b.K, b.block) == (P, 16, 16)
    ev[0].record()
    b.launch()
    ev[1].record()
    a = evaluator.prepare_many(conf, grp, range(P), seeds=seeds, manual_timestep_override=T)
    ev[2].record()
    a.launch()
    ev[3].record()
    torch.cuda.synchronize()
    print(f"4096 x 5 x 16 seeds, T = 600 (first launches, no warm-up): cases {ev[0].elapsed_time(ev[1]):.1f} ms, "
          f"rollout kernel {ev[2].elapsed_time(ev[3]):.1f} ms")
    r = b.results()
    sc, cnt, _ = a.results()
    assert np.isfinite(cnt).all()
    _same(r.counters[:, 0], cnt, "counters")
    _same(r.scores[:, 0], sc, "scores")
    assert len(set(sc[:, 0].tolist())) > 1 and all(np.isfinite(v).all() for v in r.metrics.values())


def test_set_base_out_of_range_gives_nan_for_that_group_only():
    need_gpu()
    L = 5
    conf = config.Config(pl_size=L)
    grp = _group(conf, 4 * L, 4, 1, seed=81)
    kw = dict(scenarios=("zero", "step"), seeds=[6, 7, 8], manual_timestep_override=50)  # K = 6: a block with a tail
    good = evaluator.run_cases(conf, grp, range(4), **kw)
    for bad_base in (4 * L - L + 1, -1, 4 * L):
        b = evaluator.prepare_cases(conf, grp, range(4), **kw)
        b.set_base[2] = bad_base
        b.launch()
        r = b.results()
        assert np.isnan(r.counters[2]).all() and all(np.isnan(v[2]).all() for v in r.metrics.values()) and np.isnan(r.scores[2]).all()
        for p in (0, 1, 3):
            _same(r.counters[p], good.counters[p], ("counters", p))
            for n in scenarios.METRICS:
                _same(r.metrics[n][p], good.metrics[n][p], (n, p))


@pytest.mark.parametrize("fed", ["normal", "interfrl"])
def test_vec_trainer_evaluate_scenarios_on_a_seed_batch(fed):
    """Axis order [E, P, scen, seed, ...]; each experiment's slice equals run_cases on experiment_agents(e). nofrl: per-agent sets;
    interfrl with every step federated: shared sets."""
    need_gpu()
    P, L, E = 3, 2, 2
    conf = config.Config(num_platoons=P, pl_size=L, buffer_size=128, fed_method=fed, weighted_average_enabled=False)
    vt = trainer.VecTrainer(conf, rng="device", auto_reset="platoon", seeds=[3, 4])
    assert vt.shared == (fed == "interfrl")
    vt.reset_episode()
    for _ in range(80):
        vt.step()
    torch.cuda.synchronize()
    names, seeds = ["zero", "step", "gaussian"], [6, 9]
    r = vt.evaluate_scenarios(names, seeds=seeds)
    assert r.scores.shape == (E, P, 3, 2) and r.counters.shape == (E, P, 3, 2, L) and r.metrics["max_abs_ep"].shape == (E, P, 3, 2, L)
    for e in range(E):
        solo = evaluator.run_cases(vt.conf, vt.experiment_agents(e), range(P), names, seeds=seeds, set_mod=vt.M if vt.shared else None)
        _same(r.scores[e], solo.scores, ("scores", e))
        _same(r.counters[e], solo.counters, ("counters", e))
        for n in scenarios.METRICS:
            _same(r.metrics[n][e], solo.metrics[n], (n, e))
    assert not np.array_equal(r.counters[0], r.counters[1])
    _same(r.scores[:, :, 2, 0], vt.evaluator_scores(), "the gaussian scenario at the default seed is evaluator_scores")
    sub = vt.evaluate_scenarios(["step"], seeds=[9], platoons=[2, 0])
    _same(sub.counters[:, :, 0, 0], r.counters[:, [2, 0], 1, 1], "platoons")


def _run(*argv):
    out = subprocess.run([sys.executable, "-m", "avddpg_amd", *argv], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout.strip().splitlines()


def test_cli_tr_and_esim_write_the_same_scenarios_csv(tmp_path):
    """`tr --scenarios zero,step` then `esim <dir> --scenarios zero,step` (a fresh process each): both write scenarios.csv, with
    identical rows for the saved platoons; conf.json records the suite. Without the flag `tr` writes the files and conf.json keys it
    wrote before."""
    need_gpu()
    tr = ("tr", "--pl_num", "3", "--pl_size", "2", "--buffer_size", "500", "--total_time_steps", "200", "--rng", "device", "--episodes",
          "platoon", "--report_every", "100", "--save_platoons", "2")
    base = _run(*tr, "--out", str(tmp_path / "with"), "--scenarios", "zero,step", "--eval_seeds", "6-7")[-1]
    path = os.path.join(base, "scenarios.csv")
    rows = list(csv.reader(open(path)))
    assert rows[0] == scenarios.CSV_HEADER and len(rows) == 1 + 3 * 2 * 2 * 2 and all(len(r) == 16 for r in rows)
    assert [r[:4] for r in rows[1:5]] == [["1", "zero", "6", "1"], ["1", "zero", "6", "2"], ["1", "zero", "7", "1"], ["1", "zero", "7", "2"]]
    assert all(float(r[15]) < 0 and float(r[4]) > 0 and r[14] == ("" if r[3] == "1" else r[14]) for r in rows[1:])
    js = json.load(open(os.path.join(base, "conf.json")))
    assert js["scenario_suite"] == [["names", ["zero", "step"]], ["seeds", [6, 7]], ["amp", 0.1], ["period_s", 10.0]]
    os.rename(path, path + ".tr")
    lines = _run("esim", base, "--scenarios", "zero,step", "--eval_seeds", "6-7")
    assert len(lines) == 2 * 2 and lines[0].startswith("platoon 1 zero: score ") and "string_stable" in lines[0]
    again = list(csv.reader(open(path)))
    assert again[0] == rows[0] and again[1:] == [r for r in rows[1:] if int(r[0]) <= 2]  # the two saved platoons
    plain = _run(*tr, "--out", str(tmp_path / "plain"))[-1]
    agents = {f"{stem}{p}_{m}.npz" for stem in ("actor", "critic", "target_actor", "target_critic") for p in (1, 2) for m in (1, 2)}
    assert set(os.listdir(plain)) == {"curve.csv", "conf.json"} | agents
    assert set(os.listdir(base)) == set(os.listdir(plain)) | {"scenarios.csv", "scenarios.csv.tr"}
    assert set(json.load(open(os.path.join(plain, "conf.json")))) == set(js) - {"scenario_suite"}
    lines = _run("esim", plain, "--n_timesteps", "50")
    assert len(lines) == 2 and lines[0].startswith("platoon 1: cumulative platoon reward ") and not os.path.exists(os.path.join(plain, "scenarios.csv"))


def test_cli_seed_batch_writes_scenarios_into_every_experiment(tmp_path):
    need_gpu()
    base = _run("tr", "--pl_num", "2", "--pl_size", "2", "--buffer_size", "500", "--total_time_steps", "100", "--rng", "device",
                "--episodes", "platoon", "--report_every", "100", "--seeds", "1,2", "--scenarios", "brake", "--out", str(tmp_path))[-1]
    tables = []
    for k in (1, 2):
        d = os.path.join(base, f"seed{k}")
        rows = list(csv.reader(open(os.path.join(d, "scenarios.csv"))))
        assert rows[0] == scenarios.CSV_HEADER and len(rows) == 1 + 2 * 1 * 1 * 2 and {r[1] for r in rows[1:]} == {"brake"}
        assert json.load(open(os.path.join(d, "conf.json")))["scenario_suite"][0] == ["names", ["brake"]]
        tables.append(rows)
    assert tables[0] != tables[1]
