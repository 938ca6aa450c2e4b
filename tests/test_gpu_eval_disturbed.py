"""The disturbed scenario evaluator (avd_eval_cases_dist_f32, csrc/evalx.hip; evaluator.run_disturbed): sensor noise, V2V delay and
loss, plant mismatch per case. Yardsticks: the nominal kernel (run_cases) with == wherever an axis sits at its zero, run_cases on the
other configuration for the plant, the two link extremes against each other, then the float64 restatement (tests/disturbed_oracle.py)
at the tolerances of tests/scenario_oracle.check_against; VecTrainer.evaluate_robustness and the CLI."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from avddpg_amd import _hip, config, evaluator, scenarios, trainer
from avddpg_amd.scenarios import Disturbance
from tests import disturbed_oracle as do
from tests import scenario_oracle as so
from tests.gpu_util import need_gpu
from tests.test_gpu_eval_rollout import _group, _same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _blocks(L):
    """Every block size the disturbed picker can return at this L."""
    blk = _hip.lib().avd_eval_cases_dist_block
    return sorted({blk(K, L) for K in range(1, 200)})


def _same_level(r, d, ref, what):
    """Level d of a DisturbedResults against a CaseResults: counters and all eight metrics with ==."""
    _same(r.counters[:, :, d], ref.counters, (what, "counters"))
    _same(r.scores[:, :, d], ref.scores, (what, "scores"))
    for n in scenarios.METRICS:
        _same(r.metrics[n][:, :, d], ref.metrics[n], (what, n))


def _differs(r, d, ref):
    return not np.array_equal(r.counters[:, :, d], ref.counters)


@pytest.mark.parametrize("sets", ["per_agent", "shared"])
@pytest.mark.parametrize("framework", ["decentralized", "centralized"])
@pytest.mark.parametrize("method", ["euler", "exact"])
@pytest.mark.parametrize("model", ["ModelA", "ModelB"])
@pytest.mark.parametrize("L", [1, 3, 16])
def test_null_disturbance_is_the_nominal_kernel_bit_for_bit(L, model, method, framework, sets):
    """K in {1, RB - 1, RB, RB + 1, 3 RB + 2} for every block size RB the disturbed picker returns at this L: the nominal level alone
    (K cases) and beside an all-zero named level (2 K cases) equal run_cases on the same cases."""
    need_gpu()
    conf = config.Config(pl_size=L, model=model, method=method, framework=framework)
    cen = framework == "centralized"
    S = 3 if model == "ModelA" else 4
    M = 1 if cen else L
    grp = _group(conf, 2 * M, S * L if cen else S, L if cen else 1, seed=300 + L, hidd_mult=conf.centrl_hidd_mult if cen else 1)
    kw = dict(set_mod=M, set_bases=[M, 0]) if sets == "shared" else {}
    sizes = _blocks(L)
    assert sizes == [1, 4, 8] and all(rb * L <= 256 for rb in sizes)
    used = set()
    for K in sorted({K for rb in sizes for K in (1, rb - 1, rb, rb + 1, 3 * rb + 2) if K >= 1}):
        seeds = list(range(50, 50 + K))
        ref = evaluator.run_cases(conf, grp, [0, 1], ("step",), seeds=seeds, manual_timestep_override=40, **kw)
        b = evaluator.prepare_disturbed(conf, grp, [0, 1], ("step",), (), seeds=seeds, manual_timestep_override=40, **kw)
        assert b.K == K and b.block == _hip.lib().avd_eval_cases_dist_block(K, L) and b.abc is None
        used.add(b.block)
        b.launch()
        r = b.results()
        assert r.disturbances == ["nominal"] and r.scores.shape == (2, 1, 1, K) and r.counters.shape == (2, 1, 1, K, M)
        assert r.metrics["sum_u2"].shape == (2, 1, 1, K, L) and np.isfinite(r.counters).all()
        _same_level(r, 0, ref, ("nominal alone", K))
        nom = r.nominal()
        _same(nom.counters, ref.counters, "nominal()")
        assert nom.scenarios == ref.scenarios and nom.seeds == ref.seeds and nom.T == ref.T
        r = evaluator.run_disturbed(conf, grp, [0, 1], ("step",), [Disturbance("zero")], seeds=seeds, manual_timestep_override=40, **kw)
        assert r.disturbances == ["nominal", "zero"] and r.scores.shape == (2, 1, 2, K)
        for d in (0, 1):
            _same_level(r, d, ref, ("with a zero level", K, d))
        assert not np.array_equal(ref.counters[0], ref.counters[1])
    assert used == set(sizes)


def test_each_axis_is_identity_at_its_zero():
    need_gpu()
    L = 3
    conf = config.Config(pl_size=L)
    grp = _group(conf, 2 * L, 4, 1, seed=311)
    names, seeds = ["step", "sine"], [6, 7, 8]
    ref = evaluator.run_cases(conf, grp, [0, 1], names, seeds=seeds, manual_timestep_override=40)
    zeros = [Disturbance("delay0", v2v_delay=0), Disturbance("drop0", v2v_drop=0.0), Disturbance("sigma0", noise_ep=0.0, noise_ev=0, noise_a=0.0),
             Disturbance("plant0", dyn_coeff=conf.dyn_coeff),
             Disturbance("all0", noise_ep=0, noise_ev=0, noise_a=0, v2v_delay=0, v2v_drop=0.0, dyn_coeff=conf.dyn_coeff)]
    for levels in ([z] for z in zeros):  # alone
        b = evaluator.prepare_disturbed(conf, grp, [0, 1], names, levels, seeds=seeds, manual_timestep_override=40)
        assert (b.abc is not None) == (levels[0].dyn_coeff is not None)  # the plant's zero goes through an explicit table
        b.launch()
        r = b.results()
        for d in range(2):
            _same_level(r, d, ref, (levels[0].name, d))
    # in combination, beside a level that is NOT at its zero (the launch's other rows do not leak into these)
    r = evaluator.run_disturbed(conf, grp, [0, 1], names, zeros + [Disturbance("real", noise_ep=0.05, v2v_delay=2, dyn_coeff=0.15)],
                                seeds=seeds, manual_timestep_override=40)
    assert r.scores.shape == (2, 2, 7, 3)
    for d in range(6):
        _same_level(r, d, ref, ("combined", d))
    assert _differs(r, 6, ref)


@pytest.mark.parametrize("method", ["euler", "exact"])
@pytest.mark.parametrize("L", [1, 5])
def test_plant_mismatch_equals_the_nominal_kernel_on_the_other_configuration(L, method):
    need_gpu()
    conf = config.Config(pl_size=L, method=method)
    other = config.Config(pl_size=L, method=method, dyn_coeff=0.15)
    assert conf.dyn_coeff != 0.15
    grp = _group(conf, 2 * L, 4, 1, seed=320 + L)
    names, seeds = ["step", "gaussian"], [6, 7, 8]
    for sd in seeds:  # the two configurations start alike; the disturbed path uses the nominal one's regardless
        a, b = evaluator._start(conf, True, 40, evaluation_seed=sd), evaluator._start(other, True, 40, evaluation_seed=sd)
        assert torch.equal(a[0].x, b[0].x) and torch.equal(a[0].prev_a, b[0].prev_a) and np.array_equal(a[1], b[1])
    ref = evaluator.run_cases(other, grp, [0, 1], names, seeds=seeds, manual_timestep_override=40)
    nominal = evaluator.run_cases(conf, grp, [0, 1], names, seeds=seeds, manual_timestep_override=40)
    r = evaluator.run_disturbed(conf, grp, [0, 1], names, [Disturbance("slow", dyn_coeff=0.15)], seeds=seeds, manual_timestep_override=40)
    _same_level(r, 0, nominal, "nominal")
    _same_level(r, 1, ref, "dyn_coeff=0.15")
    assert _differs(r, 1, nominal)


def test_link_extremes_hold_the_start_value_and_agree():
    """T = 12 < 16: with every sample lost, and with a delay of 15 steps, the actors see x0's 4th state throughout."""
    need_gpu()
    L = 3
    conf = config.Config(pl_size=L)
    grp = _group(conf, 2 * L, 4, 1, seed=331)
    r = evaluator.run_disturbed(conf, grp, [0, 1], ["step", "gaussian"], [Disturbance("lost", v2v_drop=1.0), Disturbance("late", v2v_delay=15)],
                                seeds=[6, 7], manual_timestep_override=12)
    _same(r.counters[:, :, 1], r.counters[:, :, 2], "counters")
    for n in scenarios.METRICS:
        _same(r.metrics[n][:, :, 1], r.metrics[n][:, :, 2], n)
    assert not np.array_equal(r.counters[:, :, 1], r.counters[:, :, 0])
    assert not np.array_equal(r.metrics["sum_u2"][:, :, 1], r.metrics["sum_u2"][:, :, 0])


AXES = [Disturbance("noise", noise_ep=0.05, noise_ev=0.05, noise_a=0.02), Disturbance("delay", v2v_delay=3), Disturbance("drop", v2v_drop=0.3),
        Disturbance("plant", dyn_coeff=0.15),
        Disturbance("all", noise_ep=0.05, noise_ev=0.05, noise_a=0.02, v2v_delay=3, v2v_drop=0.3, dyn_coeff=0.15)]


def _oracle_check(conf, L, levels, names, seeds, T, actor_seed):
    """-> the DisturbedResults. The oracle's own margins first: no |ep|, |ev| within 1e-2 of its bound, so equal terminal counts hide
    nothing. The actors are scenario_oracle.random_actors (numpy, no device) with the last layer scaled by 10: the actor seeds were
    picked on the CPU, with tests/disturbed_oracle.py alone, for rollouts that stay inside the bounds under every level (random actors
    at the scale of 40 drive most platoons far past them), with actions above 0.05."""
    S = 3 if conf.model == conf.modelA else 4
    grp = _group(conf, L, S, 1, seed=340 + L)
    for m, w in enumerate(so.random_actors(conf, L, actor_seed, last_scale=10.0)):
        grp.set_weights(m, "actor", [x.astype(np.float32) for x in w])
    r = evaluator.run_disturbed(conf, grp, [0], names, levels, seeds=seeds, manual_timestep_override=T)
    actors = [[w.astype(np.float64) for w in grp.get_weights(m, "actor")] for m in range(L)]
    ep = so.env_params(conf)
    worst = {}
    for c, name in enumerate(names):
        for d, lv in enumerate([scenarios.NOMINAL] + levels):
            for k, sd in enumerate(seeds):
                leader = scenarios.leader_profile(name, T, conf, seed=sd)
                ref, x0, tr = do.rollout(ep, L, actors, leader, evaluation_seed=sd, sigma=lv.sigma, v2v_delay=lv.v2v_delay,
                                         v2v_drop=lv.v2v_drop, dyn_coeff=lv.dyn_coeff)
                st = np.concatenate([x0[None, :, :2], tr["states"][:, :, :2]])
                for c2, bound in ((0, conf.max_ep), (1, conf.max_ev)):
                    assert np.all(np.abs(np.abs(st[..., c2]) - bound) > 1e-2), (name, lv.name, sd)
                assert np.abs(tr["inputs"]).max() > 0.05
                got = {n: r.metrics[n][0, c, d, k] for n in scenarios.METRICS}
                for n in ("max_abs_ep", "max_abs_ev", "max_abs_a", "final_abs_ep"):
                    worst[n] = max(worst.get(n, 0.0), float(np.max(np.abs(got[n] - ref[n]))))
                for n, s in (("rms_u", "sum_u2"), ("rms_jerk", "sum_jerk2")):
                    worst[n] = max(worst.get(n, 0.0), float(np.max(np.abs(np.sqrt(got[s].astype(np.float64) / T) - np.sqrt(ref[s] / T)))))
                print(conf.model, L, name, lv.name, sd)
                so.check_against(got, ref, T)
    print("worst deviations", conf.model, "L =", L, {k: f"{v:.3g}" for k, v in worst.items()})
    return r


@pytest.mark.parametrize("L", [3, 5])
def test_against_the_float64_oracle_one_axis_at_a_time_and_all_together(L):
    """Noise 0.05 / 0.05 / 0.02, delay 3, drop 0.3, dyn_coeff 0.15, each alone and all together, step and sine, 2 seeds, T = 120, at the
    tolerances of scenario_oracle.check_against (imported). The worst deviation per metric is printed; no run on a device has been
    recorded yet ("not measured")."""
    need_gpu()
    conf = config.Config(pl_size=L)
    r = _oracle_check(conf, L, AXES, ["step", "sine"], [6, 7], 120, actor_seed=407)
    assert len({r.counters[0, 0, d].tobytes() for d in range(6)}) == 6  # every axis acts


def test_model_a_against_the_float64_oracle_with_noise_and_plant():
    need_gpu()
    L = 3
    conf = config.Config(pl_size=L, model="ModelA")
    levels = [Disturbance("noise", noise_ep=0.05, noise_ev=0.05, noise_a=0.02), Disturbance("plant", dyn_coeff=0.15),
              Disturbance("both", noise_ep=0.05, noise_ev=0.05, noise_a=0.02, dyn_coeff=0.15)]
    _oracle_check(conf, L, levels, ["step"], [6], 120, actor_seed=420)
    grp = _group(conf, L, 3, 1, seed=351)
    with pytest.raises(ValueError, match="need Model B"):
        evaluator.run_disturbed(conf, grp, [0], ["step"], [Disturbance("lag", v2v_delay=1)], manual_timestep_override=40)


def test_vec_trainer_evaluate_robustness_on_a_seed_batch():
    """Axis order [E, P, scen, dist, seed, ...]; each experiment's slice equals run_disturbed on experiment_agents(e)."""
    need_gpu()
    P, L, E = 3, 2, 2
    conf = config.Config(num_platoons=P, pl_size=L, buffer_size=128, fed_method="normal")
    vt = trainer.VecTrainer(conf, rng="device", auto_reset="platoon", seeds=[3, 4])
    vt.reset_episode()
    for _ in range(40):
        vt.step()
    torch.cuda.synchronize()
    names, seeds, levels = ["zero", "step"], [6, 9], [Disturbance("lag", v2v_delay=2), Disturbance("radar", noise_ep=0.05, dyn_coeff=0.12)]
    r = vt.evaluate_robustness(names, levels, seeds=seeds)
    assert r.disturbances == ["nominal", "lag", "radar"]
    assert r.scores.shape == (E, P, 2, 3, 2) and r.counters.shape == (E, P, 2, 3, 2, L) and r.metrics["max_abs_ep"].shape == (E, P, 2, 3, 2, L)
    for e in range(E):
        solo = evaluator.run_disturbed(vt.conf, vt.experiment_agents(e), range(P), names, levels, seeds=seeds)
        _same(r.scores[e], solo.scores, ("scores", e))
        _same(r.counters[e], solo.counters, ("counters", e))
        for n in scenarios.METRICS:
            _same(r.metrics[n][e], solo.metrics[n], (n, e))
    assert not np.array_equal(r.counters[0], r.counters[1])
    plain = vt.evaluate_scenarios(names, seeds=seeds)
    _same(r.counters[:, :, :, 0], plain.counters, "the nominal level is evaluate_scenarios")
    sub = vt.evaluate_robustness(["step"], levels[:1], seeds=[9], platoons=[2, 0])
    _same(sub.counters[:, :, 0, 1, 0], r.counters[:, [2, 0], 1, 1, 1], "platoons")


def _run(*argv):
    out = subprocess.run([sys.executable, "-m", "avddpg_amd", *argv], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout.strip().splitlines()


def test_cli_tr_and_esim_write_robustness_csv_and_the_same_scenarios_csv(tmp_path):
    """`tr --seeds 1,2 --scenarios step --disturb lag:v2v_delay=2`: every experiment directory gets robustness.csv with the documented
    header and a scenarios.csv byte-identical to the run without --disturb; `esim` on a directory reproduces both files."""
    need_gpu()
    tr = ("tr", "--pl_num", "3", "--pl_size", "2", "--buffer_size", "500", "--total_time_steps", "60", "--rng", "device", "--episodes",
          "platoon", "--report_every", "60", "--seeds", "1,2", "--scenarios", "step", "--eval_seeds", "6-7")
    plain = _run(*tr, "--out", str(tmp_path / "plain"))[-1]
    base = _run(*tr, "--disturb", "lag:v2v_delay=2", "--out", str(tmp_path / "with"))[-1]
    tables = []
    for k in (1, 2):
        d = os.path.join(base, f"seed{k}")
        assert open(os.path.join(d, "scenarios.csv"), "rb").read() == open(os.path.join(plain, f"seed{k}", "scenarios.csv"), "rb").read()
        rows = list(csv.reader(open(os.path.join(d, "robustness.csv"))))
        assert rows[0] == scenarios.ROBUSTNESS_HEADER == ["platoon", "scenario", "disturbance", "seed", "vehicle", *scenarios.METRICS, "rms_u",
                                                          "rms_jerk", "ss_ratio", "score", "score_delta"]
        assert len(rows) == 1 + 3 * 1 * 2 * 2 * 2 and all(len(x) == 18 for x in rows)
        assert [x[:5] for x in rows[1:6]] == [["1", "step", "nominal", "6", "1"], ["1", "step", "nominal", "6", "2"],
                                              ["1", "step", "nominal", "7", "1"], ["1", "step", "nominal", "7", "2"], ["1", "step", "lag", "6", "1"]]
        nominal = [x[:2] + x[3:-1] for x in rows[1:] if x[2] == "nominal"]
        assert nominal == list(csv.reader(open(os.path.join(d, "scenarios.csv"))))[1:]
        assert all(float(x[-1]) == 0 for x in rows[1:] if x[2] == "nominal")
        lag = [x[:2] + x[3:-1] for x in rows[1:] if x[2] == "lag"]
        assert [x[:4] for x in lag] == [x[:4] for x in nominal] and [x[4:12] for x in lag] != [x[4:12] for x in nominal]  # the delay acts
        score = {(x[0], x[3]): np.float32(x[-2]) for x in rows[1:] if x[2] == "nominal"}
        assert all(np.float32(x[-1]) == np.float32(x[-2]) - score[(x[0], x[3])] for x in rows[1:])
        js = json.load(open(os.path.join(d, "conf.json")))
        assert js["robustness_suite"] == [["lag", [["noise_ep", 0], ["noise_ev", 0], ["noise_a", 0], ["v2v_delay", 2], ["v2v_drop", 0.0],
                                                   ["dyn_coeff", None]]]]
        assert js["scenario_suite"] == json.load(open(os.path.join(plain, f"seed{k}", "conf.json")))["scenario_suite"]
        assert set(os.listdir(d)) == set(os.listdir(os.path.join(plain, f"seed{k}"))) | {"robustness.csv"}
        tables.append(rows)
    assert tables[0] != tables[1]
    d = os.path.join(base, "seed1")
    for f in ("scenarios.csv", "robustness.csv"):
        os.rename(os.path.join(d, f), os.path.join(d, f + ".tr"))
    lines = _run("esim", d, "--scenarios", "step", "--eval_seeds", "6-7", "--disturb", "lag:v2v_delay=2")
    assert len(lines) == 3 and lines[0].startswith("platoon 1 step: score ")
    for f in ("scenarios.csv", "robustness.csv"):  # the batch saved its three platoons: esim's files are the trainer's
        assert open(os.path.join(d, f), "rb").read() == open(os.path.join(d, f + ".tr"), "rb").read(), f
