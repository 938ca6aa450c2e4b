"""The linear baseline of the scenario evaluator, the parts that need no GPU: scenarios.LinearLaw and its parsers, the gain grid, the
fitness and arg-max rules, the CLI's refusals, what avd_eval_linear_f32 / avd_linear_fitness_f32 refuse on the host before any HIP call,
and tests/linear_oracle.py against tests/scenario_oracle.py at zero gains."""
import ctypes
import math

import numpy as np
import pytest

from avddpg_amd import __main__ as cli
from avddpg_amd import _hip, config, scenarios
from avddpg_amd.scenarios import LinearLaw
from tests import linear_oracle as lo
from tests import scenario_oracle as so


# ---- 1. laws and parsers ----------------------------------------------------------------------------------------------------------------

def test_linear_law_items_gains_and_table():
    b = LinearLaw("cacc", kp=0.5, kv=1)
    assert b.items() == [["kp", 0.5], ["kv", 1], ["ka", 0], ["kf", 0]] and "cacc" in repr(b)
    g = b.gains(3)
    assert g.dtype == np.float32 and g.shape == (3, 4) and np.array_equal(g, np.tile(np.float32([0.5, 1, 0, 0]), (3, 1)))
    table = [[0.5 + 0.05 * v, 1.0 + 0.1 * v, -0.1, 0.3] for v in range(3)]
    t = LinearLaw("graded", kp=9, table=table)  # the table overrides the scalars
    assert np.array_equal(t.gains(3), np.asarray(table, dtype=np.float32)) and t.items()[-1][0] == "table"
    with pytest.raises(ValueError, match=r"gain table of shape \(3, 4\) for a platoon of 5"):
        t.gains(5)


def test_parse_baseline():
    b = scenarios.parse_baseline("cacc:kp=0.5,kv=1")
    assert (b.name, b.kp, b.kv, b.ka, b.kf, b.table) == ("cacc", 0.5, 1.0, 0, 0, None)
    assert scenarios.parse_baseline(" still ").items() == [["kp", 0], ["kv", 0], ["ka", 0], ["kf", 0]]
    assert scenarios.parse_baseline("x: ka = -0.5 , kf=1e0").items() == [["kp", 0], ["kv", 0], ["ka", -0.5], ["kf", 1.0]]
    for text, msg in ((":kp=1", "no name before ':'"), ("x:kq=1", "unknown key 'kq'"), ("x:kp", "unknown key 'kp'"),
                      ("x:kp=1,kp=2", "kp given twice"), ("x:kv=fast", "kv='fast' is not a number")):
        with pytest.raises(ValueError, match=msg):
            scenarios.parse_baseline(text)


def test_check_baselines_refusals():
    ok = [LinearLaw("a", kp=1), LinearLaw("b", kf=0.5)]
    assert scenarios.check_baselines(ok) == ok and scenarios.check_baselines(ok, config.Config()) == ok
    assert scenarios.check_baselines([]) == []
    many = [LinearLaw(f"l{i}") for i in range(17)]
    assert len(scenarios.check_baselines(many[:16])) == 16
    for laws, conf, msg in (
            (many, None, "17 baselines listed: at most 16"),
            ([LinearLaw("a"), LinearLaw("a")], None, r"baseline\(s\) \['a'\] listed more than once"),
            ([LinearLaw("tuned", kp=1)], None, "'tuned' is reserved"),
            ([LinearLaw("x", kp=math.nan)], None, "kp=nan must be a finite number"),
            ([LinearLaw("x", kv=math.inf)], None, "kv=inf must be a finite number"),
            ([LinearLaw("x", ka="1")], None, "ka='1' must be a finite number"),
            ([LinearLaw("x", kp=True)], None, "kp=True must be a finite number"),
            (["cacc:kp=1"], None, "is not a scenarios.LinearLaw"),
            ([LinearLaw("x", table=[[1, 2, 3]])], None, "table must be a finite"),
            ([LinearLaw("x", table=[[1, 2, 3, math.nan]])], None, "table must be a finite"),
            ([LinearLaw("x", table=np.zeros((3, 4)))], config.Config(pl_size=5), "a gain table of 3 rows for pl_size=5"),
            ([LinearLaw("x", kf=0.1)], config.Config(model="ModelA"), "kf needs Model B"),
            ([LinearLaw("x", table=[[0, 0, 0, 1.0]] * 3)], config.Config(model="ModelA", pl_size=3), "kf needs Model B"),
            ([LinearLaw("x", kp=1)], config.Config(framework="centralized"), "not available for the centralized framework")):
        with pytest.raises(ValueError, match=msg):
            scenarios.check_baselines(laws, conf)
    assert scenarios.check_baselines([LinearLaw("x", kp=1, ka=-1)], config.Config(model="ModelA"))  # kf = 0 is fine under Model A
    assert scenarios.check_baselines([LinearLaw("tuned")], reserved=())  # (what the tuner itself appends)


def test_parse_gain_grid():
    g = scenarios.parse_gain_grid("kp=0:2:9,kv=0:4:9,ka=-0.5:0:3")
    assert g.dtype == np.float32 and g.shape == (9 * 9 * 3, 4) and g.flags["C_CONTIGUOUS"]
    kp, kv, ka = np.linspace(0, 2, 9), np.linspace(0, 4, 9), np.linspace(-0.5, 0, 3)
    ref = np.array([[a, b, c, 0.0] for a in kp for b in kv for c in ka]).astype(np.float32)  # the last key varies fastest
    assert np.array_equal(g, ref)
    assert np.array_equal(scenarios.parse_gain_grid("kf=1:2:2"), np.float32([[0, 0, 0, 1], [0, 0, 0, 2]]))
    assert np.array_equal(scenarios.parse_gain_grid("kv=3,kp=0.5:9:1"), np.float32([[0.5, 3, 0, 0]]))  # n = 1: lo; a single value
    assert np.array_equal(scenarios.parse_gain_grid("kp=0.1:0.3:3")[:, 0], np.linspace(0.1, 0.3, 3).astype(np.float32))
    assert scenarios.parse_gain_grid("kp=0:1:256,kv=0:1:256").shape == (65536, 4)
    for text, msg in (("kp=0:1:0", r"kp has n=0 points \(n must be >= 1\)"), ("kp=0:1:-2", "n=-2"), ("kp=0:inf:3", "non-finite bound"),
                      ("kp=nan:1:3", "non-finite bound"), ("kp=0:1:257,kv=0:1:256", r"65792 candidates \(at most 65536\)"),
                      ("kq=0:1:3", "unknown key 'kq'"), ("kp=0:1:3,kp=0:1:3", "kp given twice"), ("kp=0:1", "is not lo:hi:n"),
                      ("kp=0:1:2.5", "is not lo:hi:n"), ("kp=a:1:3", "is not lo:hi:n"), ("", "no axis given"), ("kp", "unknown key 'kp'")):
        with pytest.raises(ValueError, match=msg):
            scenarios.parse_gain_grid(text)


# ---- 2. the fitness and arg-max rules ----------------------------------------------------------------------------------------------------

def test_fitness_is_the_sequential_float32_sum_and_argmax_takes_the_first_and_never_a_nan():
    rng = np.random.RandomState(5)
    c = (rng.standard_normal((7, 6, 5)) * 1e3).astype(np.float32)
    c[3] = c[1]          # a tie
    c[5, 2, 1] = np.nan  # a candidate that blew up
    fit = scenarios.fitness_of(c)
    assert fit.dtype == np.float32 and fit.shape == (7,)
    for g in range(7):
        s = np.float32(0)
        for k in range(6):
            for v in range(5):
                s = np.float32(s + c[g, k, v])
        want = np.float32(s / np.float32(30))
        assert (np.isnan(want) and np.isnan(fit[g])) or fit[g] == want
    assert fit[3] == fit[1] and np.isnan(fit[5])
    # (a pairwise or float64 sum differs from the sequential one on these magnitudes: the rule is not vacuous)
    assert any(fit[g] != np.float32(c[g].astype(np.float64).sum() / 30) for g in (0, 1, 2, 4, 6))
    arg = scenarios.first_argmax
    assert arg(np.float32([1, 3, 3, 2])) == 1 and arg(np.float32([np.nan, 1, 5, np.nan, 5])) == 2
    assert arg(np.float32([2, np.nan])) == 0 and arg(np.float32([np.nan, np.nan])) == 0 and arg(np.float32([-4])) == 0
    assert arg(np.float32([np.nan, -np.inf])) == 1 and arg(np.float32([-1, -1, -0.5, -0.5])) == 2
    f = fit.copy()
    best = arg(f)
    assert not np.isnan(f[best]) and f[best] == np.nanmax(f) and best == int(np.flatnonzero(f == np.nanmax(f))[0])


# ---- 3. the CLI --------------------------------------------------------------------------------------------------------------------------

def _parse(*argv, conf=None):
    return cli.get_cmdl_args(list(argv), config.Config() if conf is None else conf)


@pytest.mark.parametrize("argv,match", [
    (["tr", "--baseline", "cacc:kp=1"], "--baseline needs --scenarios"),
    (["esim", "d", "--baseline", "cacc:kp=1"], "--baseline needs --scenarios"),
    (["tr", "--baseline_tune", "kp=0:1:3"], "--baseline_tune needs --scenarios"),
    (["esim", "d", "--baseline_tune", "kp=0:1:3"], "--baseline_tune needs --scenarios"),
    (["tr", "--scenarios", "step", "--baseline", "x:kq=1"], "--baseline: baseline 'x': unknown key 'kq'"),
    (["tr", "--scenarios", "step", "--baseline", "x:kp=nan"], "kp=nan must be a finite number"),
    (["esim", "d", "--scenarios", "step", "--baseline", "x:kp=inf"], "kp=inf must be a finite number"),
    (["tr", "--scenarios", "step", "--baseline", "a:kp=1", "--baseline", "a:kp=2"], "listed more than once"),
    (["tr", "--scenarios", "step", "--baseline", "tuned:kp=1"], "'tuned' is reserved"),
    (["tr", "--scenarios", "step"] + [x for i in range(17) for x in ("--baseline", f"l{i}")], "17 baselines listed: at most 16"),
    (["tr", "--scenarios", "step", "--baseline_tune", "kp=0:1:3"] + [x for i in range(16) for x in ("--baseline", f"l{i}")], "at most 16 in all"),
    (["tr", "--scenarios", "step", "--baseline_tune", "kp=0:1:0"], "--baseline_tune: gain grid: kp has n=0 points"),
    (["tr", "--scenarios", "step", "--baseline_tune", "kp=0:inf:3"], "non-finite bound"),
    (["esim", "d", "--scenarios", "step", "--baseline_tune", "kp=0:1:300,kv=0:1:300"], "90000 candidates"),
])
def test_cli_refusals(argv, match, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(*argv)
    assert e.value.code == 2 and match in capsys.readouterr().err


def test_cli_refuses_what_needs_the_configuration_and_a_process_group(monkeypatch, capsys):
    for conf, argv, match in ((config.Config(model="ModelA"), ["--baseline", "ff:kf=1"], "kf needs Model B"),
                              (config.Config(model="ModelA"), ["--baseline_tune", "kp=0:1:2,kf=0:1:2"], "a grid over kf needs Model B"),
                              (config.Config(framework="centralized"), ["--baseline", "cacc:kp=1"], "not available for the centralized framework")):
        with pytest.raises(SystemExit) as e:
            _parse("tr", "--scenarios", "step", *argv, conf=conf)
        assert e.value.code == 2 and match in capsys.readouterr().err
    args, _ = _parse("tr", "--scenarios", "step,sine", "--baseline", "cacc:kp=0.5,kv=1", "--baseline", "ff:kf=1", "--baseline_tune", "kp=0:1:3,kv=0:2:3")
    assert [b.name for b in args.baseline] == ["cacc", "ff"] and args.baseline[0].kv == 1.0
    text, grid = args.baseline_tune
    assert text == "kp=0:1:3,kv=0:2:3" and grid.shape == (9, 4)
    laws, tune = cli._baseline_flags(args)
    assert len(laws) == 2 and tune[0] == text
    assert cli._baseline_flags(_parse("tr", "--scenarios", "step")[0]) is None and cli._baseline_flags(_parse("esim", "d")[0]) is None
    only_tune = cli._baseline_flags(_parse("esim", "d", "--scenarios", "step", "--baseline_tune", "kp=1")[0])
    assert only_tune[0] == [] and only_tune[1][1].shape == (1, 4)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        _parse("tr", "--scenarios", "step", "--baseline", "cacc:kp=1")
    assert "--scenarios is not available under a process group of more than one rank" in capsys.readouterr().err
    assert len(_parse("esim", "d", "--scenarios", "step", "--baseline", "cacc:kp=1")[0].baseline) == 1  # esim runs in one process


# ---- 4. the entry points' host checks ----------------------------------------------------------------------------------------------------

_BOGUS = 0x1000  # non-null "device pointers" that nothing reads: every call below is refused on the host
_PTRS = ("d_consts", "gains", "x0", "prev_a0", "leader", "sigma", "delay", "drop_q", "noise_seed", "abc", "counters", "metrics")
_TABLES = ("sigma", "delay", "drop_q", "noise_seed", "abc")


def _linear_call(G=2, K=3, L=5, T=10, sample_rate=0.1, **ptrs):
    p = {k: ctypes.c_void_p(_BOGUS * (i + 1)) for i, k in enumerate(_PTRS)}
    p.update(ptrs)
    _hip.call("avd_eval_linear_f32", p["d_consts"], G, K, L, T, p["gains"], p["x0"], p["prev_a0"], p["leader"], -2.5, 2.5, sample_rate,
              p["sigma"], p["delay"], p["drop_q"], p["noise_seed"], p["abc"], p["counters"], p["metrics"], None)


def test_linear_entry_points_refuse_on_the_host_before_any_hip_call():
    """One fault per call, with status and message (no GPU here: a call that got past its checks would fail with a HIP error instead)."""
    refuse = lambda code, msg: pytest.raises(_hip.AvdError, match=rf"failed \({code}\): {msg}")
    who = "avd_eval_linear_f32"
    for name in ("d_consts", "gains", "x0", "prev_a0", "leader", "counters"):
        with refuse(-1, f"{who}: null pointer"):
            _linear_call(**{name: None})
    for L in (0, -1, 17):
        with refuse(-1, rf"{who}: L={L} \(L must be 1..16\)"):
            _linear_call(L=L)
    for kw, got in ((dict(G=0), "G=0 K=3 T=10"), (dict(K=0), "G=2 K=0 T=10"), (dict(T=0), "G=2 K=3 T=0"), (dict(G=-4), "G=-4 K=3 T=10")):
        with refuse(-1, rf"{who}: {got} \(all must be >= 1\)"):
            _linear_call(**kw)
    for rate in (0.0, -0.1, math.nan):
        with refuse(-1, f"{who}: sample_rate="):
            _linear_call(sample_rate=rate)
    # the five tables: all null (nominal) or all but abc; any other mix is refused
    for missing in ([t] for t in _TABLES[:4]):
        with refuse(-1, f"{who}: null disturbance table"):
            _linear_call(**{t: None for t in missing})
    for present in _TABLES:
        with refuse(-1, f"{who}: null disturbance table"):
            _linear_call(**{t: None for t in _TABLES if t != present})
    with refuse(-1, f"{who}: null disturbance table"):
        _linear_call(sigma=None, delay=None, abc=None)
    # a grid that cannot hold G x K rollouts, with the numbers
    big = 2 ** 31 - 1
    with refuse(-3, rf"{who}: G={big} x K={big} = {big * big} rollouts, 12 per workgroup at L=5, need {(big * big + 11) // 12} workgroups"):
        _linear_call(G=big, K=big)
    with refuse(-3, rf"{who}: G={big} x K=17 = {big * 17} rollouts, 4 per workgroup at L=16"):
        _linear_call(G=big, K=17, L=16)
    # the fitness entry point
    who = "avd_linear_fitness_f32"
    fit = lambda G=4, K=3, L=5, counters=ctypes.c_void_p(_BOGUS), fitness=ctypes.c_void_p(2 * _BOGUS): \
        _hip.call(who, G, K, L, counters, fitness, None)
    for kw in (dict(counters=None), dict(fitness=None)):
        with refuse(-1, f"{who}: null pointer"):
            fit(**kw)
    for L in (0, 17):
        with refuse(-1, rf"{who}: L={L} \(L must be 1..16\)"):
            fit(L=L)
    for kw, got in ((dict(G=0), "G=0 K=3"), (dict(K=-1), "G=4 K=-1")):
        with refuse(-1, rf"{who}: {got} \(both must be >= 1\)"):
            fit(**kw)


# ---- 5. the oracle -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", ["ModelA", "ModelB"])
def test_linear_oracle_at_zero_gains_is_the_scenario_oracle_on_actors_with_a_zero_last_layer(model):
    L, T = 3, 40
    conf = config.Config(pl_size=L, model=model)
    ep = so.env_params(conf)
    actors = so.random_actors(conf, L, seed=17)
    for w in actors:
        w[12], w[13] = np.zeros_like(w[12]), np.zeros_like(w[13])
    for name, sd in (("step", 6), ("sine", 7)):
        leader = scenarios.leader_profile(name, T, conf, seed=sd)
        ref_m, ref_x0, ref_tr = so.rollout(ep, L, actors, leader, evaluation_seed=sd)
        got_m, got_x0, got_tr = lo.rollout(ep, L, np.zeros((L, 4)), leader, evaluation_seed=sd)
        assert np.array_equal(got_x0, ref_x0) and set(got_m) == set(ref_m) == set(scenarios.METRICS)
        for k in ref_m:
            assert np.array_equal(got_m[k], ref_m[k]), k
        for k in ref_tr:
            assert np.array_equal(got_tr[k], ref_tr[k]), k
        assert np.all(got_tr["inputs"] == 0) and got_tr["counters"].shape == (L,) and np.all(got_tr["counters"] < 0)
    # and the law itself: the gain row on the first num_obs observations, clipped
    assert lo.law([1.0, 2.0, 3.0, 4.0], [0.1, 0.2, 0.3], -2.5, 2.5) == (0.1 + 0.4) + 0.9
    assert lo.law([1.0, 2.0, 3.0, 4.0], [0.1, 0.2, 0.3, 0.4], -2.5, 2.5) == 2.5
    m, _, tr = lo.rollout(ep, L, [[4, 4, 0, 0]] * L, scenarios.leader_profile("step", T, conf), evaluation_seed=6)
    assert np.abs(tr["inputs"]).max() == 2.5 and m["sum_u2"].min() > 0
