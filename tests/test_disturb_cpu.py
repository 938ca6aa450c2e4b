"""The disturbed scenario evaluator's host side, no device: scenarios.Disturbance / parse_disturbance / check_disturbances, the drop
threshold and the plant table, robustness.csv from a synthetic results object, the argument checks of the avd_eval_cases_dist_* entry
points (each fails before any HIP call), the CLI's --disturb flag, and tests/disturbed_oracle.py against tests/scenario_oracle.py."""
import ctypes as C
import math

import numpy as np
import pytest

from avddpg_amd import __main__ as cli
from avddpg_amd import _hip, config, dynamics, evaluator, scenarios
from avddpg_amd.scenarios import Disturbance
from tests import disturbed_oracle as do
from tests import scenario_oracle as so

AVD_E_INVALID, AVD_E_UNSUPPORTED = -1, -3
FAKE = C.c_void_p(0x1000)  # non-null, never dereferenced: every refusal below comes before the first HIP call


# ---- 1. Disturbance, the parser, the checks ---------------------------------------------------------------------------------------

def test_parse_disturbance_and_defaults():
    d = scenarios.parse_disturbance("lag3:v2v_delay=3,v2v_drop=0.1")
    assert (d.name, d.v2v_delay, d.v2v_drop, d.sigma, d.dyn_coeff) == ("lag3", 3, 0.1, (0.0, 0.0, 0.0), None)
    assert isinstance(d.v2v_delay, int) and d.uses_v2v
    d = scenarios.parse_disturbance(" radar : noise_ep = 0.05 , noise_ev=0.05,noise_a=0.02, dyn_coeff=0.15 ")
    assert (d.name, d.sigma, d.dyn_coeff, d.uses_v2v) == ("radar", (0.05, 0.05, 0.02), 0.15, False)
    assert d.items() == [["noise_ep", 0.05], ["noise_ev", 0.05], ["noise_a", 0.02], ["v2v_delay", 0], ["v2v_drop", 0.0], ["dyn_coeff", 0.15]]
    z = scenarios.parse_disturbance("same")
    assert z.items() == Disturbance("same").items() == [[k, v] for k, v in zip(scenarios.DISTURBANCE_KEYS, (0, 0, 0, 0, 0.0, None))]
    n = scenarios.NOMINAL
    assert n.name == "nominal" and n.sigma == (0.0, 0.0, 0.0) and not n.uses_v2v and n.dyn_coeff is None
    assert scenarios.check_disturbances([d, z]) == [d, z] and scenarios.check_disturbances([]) == []
    assert scenarios.MAX_DELAY == _hip.AVD_EVAL_MAX_DELAY == 15


@pytest.mark.parametrize("text,match", [
    ("x:gain=2", "unknown key 'gain'"),
    ("x:v2v_delay", "unknown key 'v2v_delay'"),      # no value
    ("x:noise_ep=0.1,noise_ep=0.2", "noise_ep given twice"),
    ("x:noise_ep=abc", "noise_ep='abc' is not a number"),
    ("x:v2v_delay=2.5", "v2v_delay='2.5' is not an integer"),
    (":v2v_delay=2", "no name"),
])
def test_parser_refusals(text, match):
    with pytest.raises(ValueError, match=match):
        scenarios.parse_disturbance(text)


@pytest.mark.parametrize("kw,match", [
    (dict(noise_ep=float("nan")), "noise_ep=nan must be a finite number >= 0"),
    (dict(noise_ev=float("inf")), "noise_ev=inf must be a finite"),
    (dict(noise_a=-0.1), "noise_a=-0.1 must be a finite number >= 0"),
    (dict(noise_a="0.1"), "noise_a='0.1' must be"),
    (dict(v2v_delay=-1), "v2v_delay=-1 must be"),
    (dict(v2v_delay=16), "v2v_delay=16 must be an integer in 0..15"),
    (dict(v2v_delay=2.5), "v2v_delay=2.5 must be an integer in 0..15"),
    (dict(v2v_drop=1.01), r"v2v_drop=1.01 must be in \[0, 1\]"),
    (dict(v2v_drop=-0.2), "v2v_drop=-0.2 must be a finite number >= 0"),
    (dict(v2v_drop=float("nan")), "v2v_drop=nan"),
    (dict(dyn_coeff=0.0), "dyn_coeff=0.0 must be > 0"),
    (dict(dyn_coeff=-0.1), "dyn_coeff=-0.1 must be"),
    (dict(dyn_coeff=float("inf")), "dyn_coeff=inf must be"),
])
def test_check_disturbances_refuses_bad_values(kw, match):
    with pytest.raises(ValueError, match=match):
        scenarios.check_disturbances([Disturbance("x", **kw)])


def test_check_disturbances_refuses_names_and_model_a_links():
    with pytest.raises(ValueError, match="listed more than once"):
        scenarios.check_disturbances([Disturbance("a", noise_ep=0.1), Disturbance("a")])
    with pytest.raises(ValueError, match="'nominal' is reserved"):
        scenarios.check_disturbances([Disturbance("nominal", noise_ep=0.1)])
    with pytest.raises(ValueError, match="not a scenarios.Disturbance"):
        scenarios.check_disturbances(["lag:v2v_delay=2"])
    a, b = config.Config(model="ModelA"), config.Config(model="ModelB")
    for kw in (dict(v2v_delay=1), dict(v2v_drop=0.5)):
        with pytest.raises(ValueError, match="need Model B"):
            scenarios.check_disturbances([Disturbance("x", **kw)], a)
        assert len(scenarios.check_disturbances([Disturbance("x", **kw)], b)) == 1
        assert len(scenarios.check_disturbances([Disturbance("x", **kw)])) == 1  # no configuration: the launch's check decides
    assert len(scenarios.check_disturbances([Disturbance("x", noise_a=0.1, dyn_coeff=0.2, v2v_delay=0, v2v_drop=0.0)], a)) == 1
    # the extremes are allowed
    scenarios.check_disturbances([Disturbance("x", v2v_delay=15, v2v_drop=1.0), Disturbance("y", v2v_delay=np.int32(3), noise_ep=np.float32(0.5))], b)


def test_drop_threshold_rounding():
    """drop_q = round(p * 2^24): 0 never drops ((word >> 8) < 0 is false), 2^24 always ((word >> 8) <= 2^24 - 1)."""
    assert scenarios.drop_threshold(0) == scenarios.drop_threshold(0.0) == 0
    assert scenarios.drop_threshold(1) == scenarios.drop_threshold(1.0) == 1 << 24
    assert 0.3 * (1 << 24) == 5033164.8 and scenarios.drop_threshold(0.3) == 5033165
    assert scenarios.drop_threshold(2.0 ** -25) == 0 and scenarios.drop_threshold(3 * 2.0 ** -25) == 2  # (ties to even; below one step)
    assert all(isinstance(scenarios.drop_threshold(p), int) for p in (0, 0.3, 1))


@pytest.mark.parametrize("method", ["euler", "exact"])
@pytest.mark.parametrize("model", ["ModelA", "ModelB"])
def test_plant_table_is_env_consts_at_the_nominal_value_and_the_other_configurations_elsewhere(method, model):
    L = 5
    conf = config.Config(pl_size=L, method=method, model=model, dyn_coeff=0.25, pl_leader_tau=0.15, timegap=0.8)
    for value, other in ((None, conf), (0.25, conf), (0.15, config.Config(pl_size=L, method=method, model=model, dyn_coeff=0.15,
                                                                           pl_leader_tau=0.15, timegap=0.8))):
        t = scenarios.plant_table(conf, L, value)
        c = dynamics.env_consts(other, L)
        assert t.shape == (L, 24) and t.dtype == np.float32
        for i in range(L):
            ref = np.array(list(c.A[i]) + list(c.B[i]) + list(c.C[i]), dtype=np.float32)
            assert np.array_equal(t[i], ref), (value, i)
    assert not np.array_equal(scenarios.plant_table(conf, L, 0.15), scenarios.plant_table(conf, L))
    # the leader's lag is not the plant's: vehicle 0 keeps pl_leader_tau in its last row / C, vehicles >= 1 chain the new value
    t = scenarios.plant_table(conf, L, 0.2)
    assert not np.array_equal(t[0], t[1]) and np.array_equal(t[1], t[4])


# ---- 2. robustness.csv ------------------------------------------------------------------------------------------------------------

def _synthetic(P=2, NC=2, ND=3, NS=2, L=2):
    rng = np.random.RandomState(3)
    metrics = {n: rng.rand(P, NC, ND, NS, L).astype(np.float32) + np.float32(0.5) for n in scenarios.METRICS}
    scores = -rng.rand(P, NC, ND, NS).astype(np.float32)
    counters = rng.rand(P, NC, ND, NS, L).astype(np.float32)
    return evaluator.DisturbedResults(["zero", "step"], ["nominal", "lag", "radar"], [6, 9], 50, scores, counters, metrics)


def test_robustness_rows_and_score_delta(tmp_path):
    import csv

    r = _synthetic()
    assert scenarios.ROBUSTNESS_HEADER == ["platoon", "scenario", "disturbance", "seed", "vehicle", *scenarios.METRICS, "rms_u", "rms_jerk",
                                           "ss_ratio", "score", "score_delta"]
    assert [c for c in scenarios.ROBUSTNESS_HEADER if c not in ("disturbance", "score_delta")] == scenarios.CSV_HEADER
    rows = scenarios.robustness_rows(r, [1, 2])
    assert len(rows) == 2 * 2 * 3 * 2 * 2 and all(len(x) == len(scenarios.ROBUSTNESS_HEADER) for x in rows)
    assert [x[:5] for x in rows[:5]] == [[1, "zero", "nominal", 6, 1], [1, "zero", "nominal", 6, 2], [1, "zero", "nominal", 9, 1],
                                         [1, "zero", "nominal", 9, 2], [1, "zero", "lag", 6, 1]]
    it = iter(rows)
    for i in range(2):
        for c in range(2):
            for d in range(3):
                for k in range(2):
                    for v in range(2):
                        row = next(it)
                        assert row[-2] == repr(float(r.scores[i, c, d, k]))
                        assert row[-1] == repr(float(r.scores[i, c, d, k] - r.scores[i, c, 0, k]))
                        assert row[5] == repr(float(r.metrics["max_abs_ep"][i, c, d, k, v]))
                        if d == 0:
                            assert row[-1] == "0.0"
    # the nominal level's rows are scenarios.csv's rows with the two columns taken out
    nominal = r.nominal()
    assert nominal.scores.shape == (2, 2, 2) and nominal.metrics["sum_u2"].shape == (2, 2, 2, 2) and nominal.T == 50
    assert [x[:2] + x[3:-1] for x in rows if x[2] == "nominal"] == scenarios.csv_rows(nominal, [1, 2])
    scenarios.write_robustness_csv(tmp_path / "robustness.csv", r, [1, 2])
    back = list(csv.reader(open(tmp_path / "robustness.csv")))
    assert back[0] == scenarios.ROBUSTNESS_HEADER and back[1:] == [[str(x) for x in row] for row in rows]
    s = r.summary()
    assert s["ss_ratio"].shape == (2, 2, 3, 2, 2) and s["string_stable"].shape == (2, 2, 3, 2)


# ---- 3. the entry points' refusals --------------------------------------------------------------------------------------------------

def _args(**kw):
    """Valid arguments of a decentralized L = 5 launch (reference widths), with `kw` overriding some."""
    a = dict(lay=C.byref(_hip.make_layout(4, 1, 256, 128, 48, 64)), consts=FAKE, G=8, K=12, L=5, M=5, T=600, theta=FAKE, stats=FAKE,
             n_sets=40, set_base=FAKE, x0=FAKE, prev_a0=FAKE, leader=FAKE, high=2.5, lo=-2.5, hi=2.5, sample_rate=0.1, sigma=FAKE,
             delay=FAKE, drop_q=FAKE, noise_seed=FAKE, abc=None, counters=FAKE, metrics=None, stream=None)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("kw,match", [
    (dict(lay=None), "null layout or constants"),
    (dict(theta=None), "null pointer"),
    (dict(counters=None), "null pointer"),
    (dict(sigma=None), "null disturbance table"),
    (dict(delay=None), "null disturbance table"),
    (dict(drop_q=None), "null disturbance table"),
    (dict(noise_seed=None), "null disturbance table"),
    (dict(L=17, M=17), "L=17 (L must be 1..16)"),
    (dict(M=2), "M=2 (M must be L=5"),
    (dict(K=0), "G=8 K=0 T=600"),
    (dict(sample_rate=0.0), "sample_rate=0"),
])
def test_bad_arguments_are_refused_before_any_hip_call(kw, match):
    lib = _hip.lib()
    rc = lib.avd_eval_cases_dist_f32(*_args(**kw))
    msg = lib.avd_last_error().decode()
    assert rc == AVD_E_INVALID and msg.startswith("avd_eval_cases_dist_f32: ") and match in msg, (rc, msg)


def test_disturbed_lds_limit_and_block_size():
    """The disturbed kernel's blocks: the smallest of 1, 4, 8 that holds all K cases, else 8 (more LDS per case than the nominal kernel's,
    whose choice stays as it was); its own 160 KiB check."""
    lib = _hip.lib()
    blk, nom = lib.avd_eval_cases_dist_block, lib.avd_eval_cases_block
    for L in (1, 5, 16):
        assert [blk(K, L) for K in (1, 2, 4, 5, 8, 9, 16, 100)] == [1, 4, 4, 8, 8, 8, 8, 8]
        assert [nom(K, L) for K in (1, 2, 4, 5, 8, 9, 16, 100)] == [1, 4, 4, 8, 8, 16, 16, 16]
    assert blk(0, 5) == AVD_E_INVALID and "avd_eval_cases_dist_block: K=0" in lib.avd_last_error().decode()
    assert blk(4, 17) == AVD_E_INVALID and "L=17" in lib.avd_last_error().decode()
    wide = C.byref(_hip.make_layout(4, 1, 2048, 1024, 48, 64))  # 8 rows of 3072 hidden floats + 1216 more: 137 KiB; 2048 / 2048: 169 KiB
    huge = C.byref(_hip.make_layout(4, 1, 2048, 2048, 48, 64))
    rc = lib.avd_eval_cases_dist_f32(*_args(lay=huge, K=16))
    assert rc == AVD_E_UNSUPPORTED and "of LDS for blocks of 8 cases (> 160 KiB)" in lib.avd_last_error().decode()
    rc = lib.avd_eval_cases_dist_f32(*_args(lay=wide, K=16, sigma=None))  # past the LDS check
    assert rc == AVD_E_INVALID and "null disturbance table" in lib.avd_last_error().decode()


def test_host_check_of_the_disturbance_tables():
    lib = _hip.lib()

    def check(sigma, delay, drop_q):
        s, d, q = np.asarray(sigma, dtype=np.float32).reshape(-1, 3), np.asarray(delay, dtype=np.int32), np.asarray(drop_q, dtype=np.uint32)
        rc = lib.avd_eval_cases_dist_check(len(d), s.ctypes.data, d.ctypes.data, q.ctypes.data)
        return rc, lib.avd_last_error().decode()

    z = [0.0, 0.0, 0.0]
    assert check([z, [0.05, 0.05, 0.02]], [0, 15], [0, 1 << 24])[0] == 0
    for bad, match in ((float("nan"), "sigma[1][2]=nan"), (float("inf"), "sigma[1][2]=inf"), (-0.5, "sigma[1][2]=-0.5")):
        rc, msg = check([z, [0.0, 0.0, bad]], [0, 0], [0, 0])
        assert rc == AVD_E_INVALID and match in msg and "finite and >= 0" in msg, msg
    rc, msg = check([z, z], [0, 16], [0, 0])
    assert rc == AVD_E_INVALID and "delay[1]=16 (must be 0..15)" in msg
    rc, msg = check([z, z], [-1, 0], [0, 0])
    assert rc == AVD_E_INVALID and "delay[0]=-1" in msg
    rc, msg = check([z], [0], [(1 << 24) + 1])
    assert rc == AVD_E_INVALID and "drop_q[0]=16777217 (must be <= 2^24" in msg
    assert lib.avd_eval_cases_dist_check(0, FAKE, FAKE, FAKE) == AVD_E_INVALID and "K=0" in lib.avd_last_error().decode()
    assert lib.avd_eval_cases_dist_check(1, None, FAKE, FAKE) == AVD_E_INVALID and "null pointer" in lib.avd_last_error().decode()


# ---- 4. the CLI ---------------------------------------------------------------------------------------------------------------------

def _parse(*argv):
    return cli.get_cmdl_args(list(argv), config.Config())


@pytest.mark.parametrize("argv,match", [
    (["tr", "--disturb", "lag:v2v_delay=2"], "--disturb needs --scenarios"),
    (["esim", "d", "--disturb", "lag:v2v_delay=2"], "--disturb needs --scenarios"),
    (["tr", "--scenarios", "step", "--disturb", "lag:v2v_lag=2"], "--disturb: disturbance 'lag': unknown key 'v2v_lag'"),
    (["tr", "--scenarios", "step", "--disturb", "lag:v2v_delay=16"], "--disturb: disturbance 'lag': v2v_delay=16"),
    (["esim", "d", "--scenarios", "step", "--disturb", "lag:v2v_drop=1.5"], "v2v_drop=1.5 must be in [0, 1]"),
    (["tr", "--scenarios", "step", "--disturb", "a:noise_ep=0.1", "--disturb", "a:noise_ev=0.1"], "listed more than once"),
    (["tr", "--scenarios", "step", "--disturb", "nominal:noise_ep=0.1"], "reserved"),
    (["tr", "--scenarios", "step", "--disturb", "x:dyn_coeff=0"], "dyn_coeff=0.0 must be > 0"),
    (["tr", "--scenarios", "step", "--disturb", "x:noise_a=-1"], "noise_a=-1.0 must be a finite number >= 0"),
])
def test_cli_refusals(argv, match, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(*argv)
    assert e.value.code == 2 and match in capsys.readouterr().err


def test_cli_parses_repeated_flags_and_is_refused_under_several_ranks(monkeypatch, capsys):
    args, _ = _parse("tr", "--scenarios", "step,sine", "--disturb", "lag:v2v_delay=2", "--disturb", "slow:dyn_coeff=0.15,noise_a=0.02")
    assert [d.name for d in args.disturb] == ["lag", "slow"] and args.disturb[0].v2v_delay == 2 and args.disturb[1].dyn_coeff == 0.15
    assert cli._disturb(_parse("tr", "--scenarios", "step")[0]) is None and cli._disturb(_parse("esim", "d")[0]) is None
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        _parse("tr", "--scenarios", "step", "--disturb", "lag:v2v_delay=2")
    assert "more than one rank" in capsys.readouterr().err
    assert len(_parse("esim", "d", "--scenarios", "step", "--disturb", "lag:v2v_delay=2")[0].disturb) == 1  # esim runs in one process


# ---- 5. the float64 oracle of the GPU tests ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", ["ModelA", "ModelB"])
def test_disturbed_oracle_with_the_null_disturbance_is_the_scenario_oracle(model):
    L, T = 3, 30
    conf = config.Config(pl_size=L, model=model)
    ep = so.env_params(conf)
    actors = so.random_actors(conf, L, seed=5)
    leader = scenarios.leader_profile("sine", T, conf)
    ref = so.rollout(ep, L, actors, leader, evaluation_seed=7)
    for kw in (dict(), dict(dyn_coeff=conf.dyn_coeff), dict(sigma=(0.0, 0.0, 0.0), v2v_delay=0, v2v_drop=0.0, noise_seed=99)):
        got = do.rollout(ep, L, actors, leader, evaluation_seed=7, **kw)
        assert np.array_equal(got[1], ref[1])
        for n in scenarios.METRICS:
            assert np.array_equal(got[0][n], ref[0][n]), n
        for n in ("states", "inputs", "jerks"):
            assert np.array_equal(got[2][n], ref[2][n]), n
    assert np.abs(ref[2]["inputs"]).max() > 0.01


def test_disturbed_oracle_axes_act_and_the_link_extremes_agree():
    L, T = 3, 12
    conf = config.Config(pl_size=L)
    ep = so.env_params(conf)
    actors = so.random_actors(conf, L, seed=5)
    leader = scenarios.leader_profile("step", T, conf)
    run = lambda **kw: do.rollout(ep, L, actors, leader, evaluation_seed=6, **kw)[2]["inputs"]
    base = run()
    held = run(v2v_drop=1.0)
    assert np.array_equal(held, run(v2v_delay=15)) and not np.array_equal(held, base)  # both hold x0's value for all 12 steps
    for kw in (dict(sigma=(0.05, 0.0, 0.0)), dict(sigma=(0.0, 0.0, 0.02)), dict(v2v_delay=3), dict(v2v_drop=0.3), dict(dyn_coeff=0.15)):
        assert not np.array_equal(run(**kw), base), kw
    assert np.array_equal(run(sigma=(0.05, 0.05, 0.02)), run(sigma=(0.05, 0.05, 0.02)))
    assert not np.array_equal(run(sigma=(0.05, 0.05, 0.02)), run(sigma=(0.05, 0.05, 0.02), noise_seed=7))
    assert math.isfinite(float(np.abs(base).max()))
