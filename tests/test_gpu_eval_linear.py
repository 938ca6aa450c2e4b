"""The linear scenario evaluator (avd_eval_linear_f32 / avd_linear_fitness_f32, csrc/lin.hip; evaluator.run_linear / tune_linear).
Yardsticks: the disturbed scenario evaluator with == at zero gains (actors whose last layer is zero), the float64 restatement
(tests/linear_oracle.py) at the tolerances of tests/scenario_oracle.check_against, single-rollout launches with == for the packing of
rollouts into waves, the NumPy float32 loop with == for the fitness, and the CLI's files."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from avddpg_amd import _hip, config, evaluator, scenarios
from avddpg_amd._hip import ptr
from avddpg_amd.scenarios import Disturbance, LinearLaw
from tests import linear_oracle as lo
from tests import scenario_oracle as so
from tests.gpu_util import need_gpu
from tests.test_gpu_eval_disturbed import AXES
from tests.test_gpu_eval_rollout import _group, _same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE, PLANT, ALL = AXES[0], AXES[3], AXES[4]


def _same_results(got, ref, what):
    """Two results of the same shape: counters, scores and all eight metrics with ==."""
    _same(got.counters, ref.counters, (what, "counters"))
    _same(got.scores, ref.scores, (what, "scores"))
    for n in scenarios.METRICS:
        _same(got.metrics[n], ref.metrics[n], (what, n))


# ---- 1. bit for bit against the existing kernel ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model,method,L", [("ModelB", m, L) for m in ("euler", "exact") for L in (1, 3, 5, 16)] + [("ModelA", "euler", 3)])
def test_zero_gains_equal_the_disturbed_evaluator_on_actors_with_a_zero_last_layer(model, method, L):
    """tanhf(0) * high = 0 = the zero law's action: step, reward, metrics, case indexing and the plant table are evalx.hip's. (The
    observation path does not reach a zero law's action: the oracle tests pin it.)"""
    need_gpu()
    conf = config.Config(pl_size=L, model=model, method=method)
    S = 3 if model == "ModelA" else 4
    levels = AXES if model == "ModelB" else [NOISE, PLANT]
    grp = _group(conf, L, S, 1, seed=500 + L)
    lay = grp.lay
    grp.theta[:, lay.aW3:lay.aW3 + lay.H2] = 0.0
    grp.theta[:, lay.ab3] = 0.0
    names, seeds, T = ["step", "sine", "gaussian"], [6, 7], 100
    ref = evaluator.run_disturbed(conf, grp, [0], names, levels, seeds=seeds, manual_timestep_override=T)
    zero = [LinearLaw("zero")]
    got = evaluator.run_linear(conf, zero, names, levels, seeds=seeds, manual_timestep_override=T)
    assert got.disturbances == ref.disturbances == ["nominal"] + [d.name for d in levels]
    assert got.counters.shape == (1, 3, len(levels) + 1, 2, L) and got.metrics["sum_u2"].shape == (1, 3, len(levels) + 1, 2, L)
    _same_results(got, ref, "disturbed")
    assert np.all(got.metrics["sum_u2"] == 0) and np.isfinite(got.counters).all() and np.all(got.counters < 0)
    assert len({got.counters[0, 0, d].tobytes() for d in (0, len(levels) - (model == "ModelB"))}) == 2  # the plant level acts
    # the nominal instantiation (null tables): run_cases' cases
    plain = evaluator.run_linear(conf, zero, names, seeds=seeds, manual_timestep_override=T)
    assert isinstance(plain, evaluator.CaseResults) and plain.counters.shape == (1, 3, 2, L)
    _same_results(plain, ref.nominal(), "nominal")


def test_every_batch_class_builds_the_same_case_tables_and_outputs_of_its_own_size():
    """One suite, T = 40 past the 16-slot ring, one level with every axis on: LinearBatch, DisturbedBatch and CaseBatch hold the same
    tables case for case, and each allocates counters and metrics for its own K. No rollout is launched."""
    need_gpu()
    L, names, seeds, T = 3, ("gaussian", "step"), (1, 2), 40
    conf = config.Config(pl_size=L)
    full = Disturbance("full", noise_ep=0.05, noise_ev=0.04, noise_a=0.02, v2v_delay=15, v2v_drop=0.3, dyn_coeff=0.15)
    grp = _group(conf, 2 * L, 4, 1, seed=77)
    gains = np.zeros((5, L, 4), dtype=np.float32)
    cases = evaluator.prepare_cases(conf, grp, [0, 1], names, seeds=seeds, manual_timestep_override=T)
    dist = evaluator.prepare_disturbed(conf, grp, [0, 1], names, [full], seeds=seeds, manual_timestep_override=T)
    lin = evaluator.LinearBatch(conf, gains, names, [full], seeds, None, 10.0, T)
    plain = evaluator.LinearBatch(conf, gains, names, [], seeds, None, 10.0, T)
    tables = ("x0", "pa0", "leader", "sigma", "delay", "drop_q", "noise_seed", "abc")
    assert (cases.K, dist.K, lin.K, plain.K) == (4, 8, 8, 4) and (dist.ND, lin.ND) == (2, 2)
    for n in tables:
        assert torch.equal(getattr(lin, n), getattr(dist, n)), n
    assert np.array_equal(lin.leader_h, dist.leader_h) and np.array_equal(plain.leader_h, cases.leader_h)
    assert float(dist.sigma.min()) == 0.0 < float(dist.sigma.max()) and int(dist.delay.max()) == 15 and dist.abc.shape == (8, L, 24)
    assert 0 < int(dist.drop_q.max()) < 1 << 24
    for n in tables[:3]:
        assert torch.equal(getattr(plain, n), getattr(cases, n)), n
        wide = getattr(dist, n).reshape(2, 2, 2, *getattr(dist, n).shape[1:])  # [scenario, level, seed, ...]
        assert torch.equal(wide[:, 0].reshape(getattr(cases, n).shape), getattr(cases, n)), n
    for n in tables[3:]:
        assert getattr(plain, n) is None, n
    for b in (cases, dist, lin, plain):  # (decentralized: one counter per vehicle)
        assert tuple(b.counters.shape) == (b.G, b.K, L) and tuple(b.metrics.shape) == (b.G, b.K, L, _hip.AVD_EVAL_NMETRIC)
    assert (cases.G, dist.G, lin.G, plain.G) == (2, 2, 5, 5)


# ---- 2. the float64 oracle ---------------------------------------------------------------------------------------------------------------

def _table(kind, L):
    if kind == "graded":
        return [[0.5 + 0.05 * v, 1.0 + 0.1 * v, -0.1, 0.3] for v in range(L)]
    return [[4.0, 4.0, 0.0, 0.0]] * L  # stiff


def _oracle_check(conf, L, table, levels, names, seeds, T, min_margin=1e-2, score=True, raw=False):
    """-> (the results, the number of clipped samples of the oracle, its terminal vehicle-steps). The oracle's own margins first: no
    |ep|, |ev| sample within 1e-2 of its bound, so equal terminal counts hide nothing; actions above 0.05. raw: the table goes to a
    LinearBatch as it is (run_linear refuses a 4th gain under Model A)."""
    if raw:
        b = evaluator.LinearBatch(conf, np.asarray([table], dtype=np.float32), names, levels, seeds, None, 10.0, T)
        b.launch()
        r = b.results()
    else:
        r = evaluator.run_linear(conf, [LinearLaw("law", table=table)], names, levels, seeds=seeds, manual_timestep_override=T)
    ep = so.env_params(conf)
    worst, clipped, terminal = {}, 0, 0
    for c, name in enumerate(names):
        for d, lv in enumerate([scenarios.NOMINAL] + list(levels)):
            for k, sd in enumerate(seeds):
                leader = scenarios.leader_profile(name, T, conf, seed=sd)
                ref, x0, tr = lo.rollout(ep, L, table, leader, evaluation_seed=sd, sigma=lv.sigma, v2v_delay=lv.v2v_delay,
                                         v2v_drop=lv.v2v_drop, dyn_coeff=lv.dyn_coeff)
                st = np.concatenate([x0[None, :, :2], tr["states"][:, :, :2]])
                for c2, bound in ((0, conf.max_ep), (1, conf.max_ev)):
                    assert np.all(np.abs(np.abs(st[..., c2]) - bound) > min_margin), (name, lv.name, sd)
                assert np.abs(tr["inputs"]).max() > 0.05
                clipped += int(np.sum(np.abs(tr["inputs"]) == conf.action_high))
                terminal += int(ref["term_steps"].sum())
                at = (0, c, d, k) if levels else (0, c, k)
                got = {n: r.metrics[n][at] for n in scenarios.METRICS}
                for n in ("max_abs_ep", "max_abs_ev", "max_abs_a", "final_abs_ep"):
                    worst[n] = max(worst.get(n, 0.0), float(np.max(np.abs(got[n] - ref[n]))))
                for n, s in (("rms_u", "sum_u2"), ("rms_jerk", "sum_jerk2")):
                    worst[n] = max(worst.get(n, 0.0), float(np.max(np.abs(np.sqrt(got[s].astype(np.float64) / T) - np.sqrt(ref[s] / T)))))
                o_score = round(np.average(tr["counters"].astype(np.float32)), 3)
                worst["score"] = max(worst.get("score", 0.0), abs(float(r.scores[at]) - float(o_score)))
                print(conf.model, L, name, lv.name, sd, "score", r.scores[at], o_score)
                so.check_against(got, ref, T)
                if score:
                    assert abs(float(r.scores[at]) - float(o_score)) <= 2e-3, (name, lv.name, sd, r.scores[at], o_score)
    print("worst deviations", conf.model, "L =", L, {k: f"{v:.3g}" for k, v in worst.items()}, "clipped", clipped, "terminal", terminal)
    return r, clipped, terminal


@pytest.mark.parametrize("kind", ["graded", "stiff"])
@pytest.mark.parametrize("L", [3, 5])
def test_against_the_float64_oracle_one_axis_at_a_time_and_all_together(L, kind):
    """Per-vehicle rows (graded) and a law that lives on the clip (stiff), nominal and the five AXES, step and sine, 2 seeds, T = 120, at
    the tolerances of scenario_oracle.check_against; the score within 2e-3 of the oracle's. Recorded on an MI355X (the test prints
    them): maxima and final |ep| within 3.5e-7, rms_u 4.6e-7, rms_jerk 3.4e-6, every rounded score equal."""
    need_gpu()
    conf = config.Config(pl_size=L)
    r, clipped, terminal = _oracle_check(conf, L, _table(kind, L), AXES, ["step", "sine"], [6, 7], 120)
    assert terminal == 0 and (clipped > 0 or (kind, L) == ("graded", 3))  # the clip is exercised
    distinct = len({r.counters[0, 0, d].tobytes() for d in range(6)})
    if kind == "graded":
        assert distinct == 6  # every axis acts
    else:  # a zero 4th gain: the link's delay and loss do not reach the action, bit for bit; noise, plant and both do
        assert distinct == 4
        _same(r.counters[:, :, 2], r.counters[:, :, 0], "delay")
        _same(r.counters[:, :, 3], r.counters[:, :, 0], "drop")


@pytest.mark.parametrize("kind", ["graded", "stiff"])
def test_model_a_against_the_float64_oracle_with_noise_and_plant(kind):
    """Model A reads three observations: the graded table's 4th gain (0.3) is in the launch and is not read -- the oracle applies the
    first num_obs gains. The raw batch takes such a table; run_linear refuses it."""
    need_gpu()
    L = 3
    conf = config.Config(pl_size=L, model="ModelA")
    _oracle_check(conf, L, _table(kind, L), [NOISE, PLANT], ["step", "sine"], [6, 7], 120, raw=True)
    with pytest.raises(ValueError, match="kf needs Model B"):
        evaluator.run_linear(conf, [LinearLaw("ff", kf=0.3)], ["step"], manual_timestep_override=40)
    with pytest.raises(ValueError, match="need Model B"):
        evaluator.run_linear(conf, [LinearLaw("x", kp=1)], ["step"], [Disturbance("lag", v2v_delay=1)], manual_timestep_override=40)
    with pytest.raises(ValueError, match="not available for the centralized framework"):
        evaluator.run_linear(config.Config(pl_size=L, framework="centralized"), [LinearLaw("x", kp=1)], ["step"], manual_timestep_override=40)


# ---- 3. terminal accounting --------------------------------------------------------------------------------------------------------------

def test_terminal_steps_and_the_first_of_them_equal_the_oracle():
    """Positive feedback (-0.5, -1, 0, 0) drives every follower past its bounds: term_steps and first_term equal the oracle's (whose
    margin to a bound is 0.027 > 1e-2 here), the other metrics at check_against's tolerances, nominal and under the `all` level."""
    need_gpu()
    L = 3
    conf = config.Config(pl_size=L)
    r, _, terminal = _oracle_check(conf, L, [[-0.5, -1.0, 0.0, 0.0]] * L, [ALL], ["step", "sine"], [6, 7], 200, score=False)
    assert terminal > 1000 and r.metrics["term_steps"].sum() == terminal and (r.metrics["first_term"] >= 0).any()


# ---- 4. packing independence -------------------------------------------------------------------------------------------------------------

def _solo(b, g, k):
    """A G = 1, K = 1 launch of gain set g and case k of a LinearBatch, on its own device inputs: (counters [L], metrics [L, 8])."""
    one = lambda x: None if x is None else x[k:k + 1].contiguous()
    f32 = dict(dtype=torch.float32, device=b.counters.device)
    cnt, met = torch.full((b.L,), np.nan, **f32), torch.full((b.L, _hip.AVD_EVAL_NMETRIC), np.nan, **f32)
    c = b.conf
    _hip.call("avd_eval_linear_f32", ptr(b.env.d_consts), 1, 1, b.L, b.T, ptr(b.gains[g:g + 1].contiguous()), ptr(one(b.x0)), ptr(one(b.pa0)),
              ptr(one(b.leader)), c.action_low, c.action_high, c.sample_rate, ptr(one(b.sigma)), ptr(one(b.delay)), ptr(one(b.drop_q)),
              ptr(one(b.noise_seed)), ptr(one(b.abc)), ptr(cnt), ptr(met), _hip.stream_handle())
    return cnt.cpu().numpy(), met.cpu().numpy()


@pytest.mark.parametrize("G,L,disturbed", [(37, 5, False), (7, 3, True)])
def test_every_rollout_is_independent_of_how_the_launch_packs_it(G, L, disturbed):
    """37 x 6 rollouts of 5 lanes (12 per wave, 19 workgroups, the last one partly filled) on the nominal kernel; 7 x 5 of 3 lanes (21 per
    wave) on the disturbed one, whose ring column is per lane: a (g, k) slice equals a launch of that pair alone. Neighbouring gain sets
    and vehicles differ."""
    need_gpu()
    conf = config.Config(pl_size=L)
    gains = np.array([[[0.3 + 0.02 * g + 0.05 * v, 0.8 + 0.03 * g + 0.1 * v, -0.1 - 0.01 * g, 0.2 + 0.01 * g] for v in range(L)] for g in range(G)],
                     dtype=np.float32)
    if disturbed:
        names, seeds, levels = ["sine"], [6], [AXES[0], AXES[1], AXES[2], ALL]
    else:
        names, seeds, levels = ["step", "sine", "gaussian"], [6, 7], []
    b = evaluator.LinearBatch(conf, gains, names, levels, seeds, None, 10.0, 120)
    K, per_wave = b.K, 64 // L
    assert (b.G, K) == ((37, 6) if not disturbed else (7, 5)) and (G * K) % per_wave != 0 and G * K > per_wave
    b.counters.fill_(float("nan")), b.metrics.fill_(float("nan"))
    b.launch()
    cnt, met = b.counters.cpu().numpy(), b.metrics.cpu().numpy()
    assert np.isfinite(cnt).all() and np.isfinite(met).all()
    rolls = {0, G * K - 1, per_wave - 1, per_wave, 2 * per_wave - 1, 2 * per_wave} | {int(r) for r in np.random.RandomState(G).randint(0, G * K, 8)}
    rolls = sorted(r for r in rolls if r < G * K)
    assert len(rolls) >= 10
    for r in rolls:
        g, k = divmod(r, K)
        c1, m1 = _solo(b, g, k)
        _same(cnt[g, k], c1, ("counters", g, k))
        _same(met[g, k], m1, ("metrics", g, k))
    for g in range(G - 1):  # a lane that read its neighbour's row would not pass
        assert not np.array_equal(cnt[g], cnt[g + 1])
    assert all(not np.array_equal(cnt[:, :, v], cnt[:, :, v + 1]) for v in range(L - 1))


# ---- 5. tuning ---------------------------------------------------------------------------------------------------------------------------

def test_tune_linear_fitness_is_the_numpy_loop_and_the_best_is_the_first_argmax():
    need_gpu()
    L = 5
    conf = config.Config(pl_size=L)
    grid = scenarios.parse_gain_grid("kp=0:2:5,kv=0:4:5")
    kw = dict(scenarios=["step", "sine"], seeds=[6, 7], manual_timestep_override=120)
    best, fit = evaluator.tune_linear(conf, grid, **kw)
    assert fit.dtype == np.float32 and fit.shape == (25,) and np.isfinite(fit).all()
    ref = np.zeros(25, dtype=np.float32)
    for g in range(25):
        solo = evaluator.run_linear(conf, [LinearLaw("c", *[float(x) for x in grid[g]])], **kw)
        assert solo.counters.shape == (1, 2, 2, L)
        ref[g] = scenarios.fitness_of(solo.counters.reshape(1, 4, L))[0]
    _same(fit, ref, "fitness")
    assert best == scenarios.first_argmax(ref) == int(np.argmax(ref)) and np.array_equal(grid[0], np.zeros(4, dtype=np.float32))
    assert fit[best] > fit[0]  # better than no control at all
    print("tuned", grid[best], "fitness", fit[best], "zero gains", fit[0])


# ---- 6. the CLI --------------------------------------------------------------------------------------------------------------------------

def _run(*argv):
    out = subprocess.run([sys.executable, "-m", "avddpg_amd", *argv], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout.strip().splitlines()


_TR = ("tr", "--pl_num", "3", "--pl_size", "2", "--buffer_size", "500", "--total_time_steps", "60", "--rng", "device", "--episodes", "platoon",
       "--report_every", "60", "--scenarios", "step,sine", "--eval_seeds", "6-7", "--disturb", "lag:v2v_delay=2")
_BASE = ("--baseline", "cacc:kp=0.5,kv=1", "--baseline_tune", "kp=0:1:3,kv=0:2:3")
_HEADER = ["controller", "scenario", "disturbance", "seed", "vehicle", *scenarios.METRICS, "rms_u", "rms_jerk", "ss_ratio", "score", "score_delta",
           "actors_score"]


def _check_baseline_csv(d):
    rows = list(csv.reader(open(os.path.join(d, "baseline.csv"))))
    assert rows[0] == scenarios.BASELINE_ROBUSTNESS_HEADER == _HEADER
    assert len(rows) == 1 + 2 * 2 * 2 * 2 * 2 and all(len(x) == 19 for x in rows)  # laws x scenarios x levels x seeds x vehicles
    assert [x[:5] for x in rows[1:6]] == [["cacc", "step", "nominal", "6", "1"], ["cacc", "step", "nominal", "6", "2"],
                                          ["cacc", "step", "nominal", "7", "1"], ["cacc", "step", "nominal", "7", "2"],
                                          ["cacc", "step", "lag", "6", "1"]]
    assert [x[0] for x in rows[1:]] == ["cacc"] * 16 + ["tuned"] * 16
    assert all(float(x[-2]) == 0 for x in rows[1:] if x[2] == "nominal")
    score = {(x[0], x[1], x[3]): np.float32(x[-3]) for x in rows[1:] if x[2] == "nominal"}
    assert all(np.float32(x[-2]) == np.float32(x[-3]) - score[(x[0], x[1], x[3])] for x in rows[1:])
    # actors_score: the mean over the platoons of robustness.csv's score for the same (scenario, disturbance, seed)
    rob = list(csv.reader(open(os.path.join(d, "robustness.csv"))))[1:]
    per = {}
    for x in rob:
        if x[4] == "1":
            per.setdefault((x[1], x[2], x[3]), []).append(np.float32(x[-2]))
    for x in rows[1:]:
        want = np.mean(np.array(per[(x[1], x[2], x[3])], dtype=np.float32), dtype=np.float32)
        assert len(per[(x[1], x[2], x[3])]) == 3 and x[-1] == repr(float(want)), (x[:5], x[-1], want)
    return rows


def test_cli_tr_and_esim_write_baseline_csv_and_leave_the_other_files_alone(tmp_path):
    need_gpu()
    plain = _run(*_TR, "--out", str(tmp_path / "plain"))[-1]
    base = _run(*_TR, *_BASE, "--out", str(tmp_path / "with"))[-1]
    for f in ("scenarios.csv", "robustness.csv"):
        assert open(os.path.join(base, f), "rb").read() == open(os.path.join(plain, f), "rb").read(), f
    assert set(os.listdir(base)) == set(os.listdir(plain)) | {"baseline.csv"}
    rows = _check_baseline_csv(base)
    js, js0 = json.load(open(os.path.join(base, "conf.json"))), json.load(open(os.path.join(plain, "conf.json")))
    assert "baseline_suite" not in js0 and "baseline_tune" not in js0
    assert js["baseline_suite"][0] == ["cacc", [["kp", 0.5], ["kv", 1.0], ["ka", 0], ["kf", 0]]]
    name, tuned = js["baseline_suite"][1]
    grid = scenarios.parse_gain_grid("kp=0:1:3,kv=0:2:3")
    tune = dict(js["baseline_tune"])
    assert name == "tuned" and tune["grid"] == "kp=0:1:3,kv=0:2:3" and tune["candidates"] == 9 and tune["gains"] == tuned
    assert [v for _, v in tuned] == [float(x) for x in grid[tune["best_index"]]]
    assert {k: v for k, v in js.items() if not k.startswith("baseline_")}.keys() == js0.keys()
    for f in ("scenarios.csv", "robustness.csv", "baseline.csv"):
        os.rename(os.path.join(base, f), os.path.join(base, f + ".tr"))
    lines = _run("esim", base, "--scenarios", "step,sine", "--eval_seeds", "6-7", "--disturb", "lag:v2v_delay=2", *_BASE)
    assert len(lines) == 3 * 2 + 2 * 2 and lines[0].startswith("platoon 1 step: score ")
    assert lines[6].startswith("baseline cacc step: score ") and lines[9].startswith("baseline tuned sine: score ")
    for f in ("scenarios.csv", "robustness.csv", "baseline.csv"):  # the run saved its three platoons: esim's files are the trainer's
        assert open(os.path.join(base, f), "rb").read() == open(os.path.join(base, f + ".tr"), "rb").read(), f
    assert rows == list(csv.reader(open(os.path.join(base, "baseline.csv"))))


def test_cli_seed_batch_writes_the_baseline_into_every_experiment_directory(tmp_path):
    """`tr --seeds 1,2`: the baseline is computed once; the directories' files differ in actors_score alone."""
    need_gpu()
    base = _run(*_TR, *_BASE, "--seeds", "1,2", "--out", str(tmp_path / "batch"))[-1]
    tables = [_check_baseline_csv(os.path.join(base, f"seed{k}")) for k in (1, 2)]
    assert [x[:-1] for x in tables[0]] == [x[:-1] for x in tables[1]] and tables[0] != tables[1]
    for k in (1, 2):
        js = json.load(open(os.path.join(base, f"seed{k}", "conf.json")))
        assert [n for n, _ in js["baseline_suite"]] == ["cacc", "tuned"] and dict(js["baseline_tune"])["grid"] == "kp=0:1:3,kv=0:2:3"
