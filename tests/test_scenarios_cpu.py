"""CPU checks of the scenario evaluator: the leader profiles (scenarios.leader_profile), the definition of the control metrics
(scenarios.metrics_from_traces) against a float64 restatement of the rollout written from the oracle (tests/scenario_oracle.py), the
argument checks of avd_eval_cases_f32 (csrc/evalx.hip; each fails before any HIP call) and the CLI's scenario flags."""
import copy
import ctypes as C

import numpy as np
import pytest

from avddpg_amd import __main__ as cli
from avddpg_amd import _hip, config, scenarios
from tests import scenario_oracle as so

AVD_E_INVALID, AVD_E_UNSUPPORTED = -1, -3
FAKE = C.c_void_p(0x1000)  # a non-null "device pointer": the checks only test it for NULL, nothing dereferences it on the host


# ---- 1. profiles --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [600, 101])
def test_deterministic_profiles_exact_values(T):
    conf = config.Config()
    q, amp = T // 4, 0.25
    at = [q - 1, q, 2 * q - 1, 2 * q, T - 1]
    f32 = lambda v: np.array(v, dtype=np.float64).astype(np.float32)
    want = dict(zero=[0, 0, 0, 0, 0], step=[0, amp, amp, amp, amp], brake=[0, -amp, -amp, 0, 0],
                ramp=[0, 0, amp * (q - 1) / q, amp, amp],
                sine=[amp * np.sin(2 * np.pi * k * conf.sample_rate / 7.0) for k in at])
    for name, vals in want.items():
        u = scenarios.leader_profile(name, T, conf, amp=amp, period_s=7.0)
        assert u.dtype == np.float32 and u.shape == (T,), name
        assert np.array_equal(u[at], f32(vals)), (name, u[at], vals)
    assert np.array_equal(scenarios.leader_profile("step", T, conf)[[q - 1, q]], f32([0, conf.reset_max_u]))  # amp defaults to reset_max_u
    k = np.arange(T)
    assert np.array_equal(scenarios.leader_profile("ramp", T, conf, amp=amp), (amp * np.clip((k - q) / q, 0, 1)).astype(np.float32))


@pytest.mark.parametrize("rand_gen", ["normal", "uniform"])
def test_gaussian_profile_is_the_evaluators_draws_and_restores_the_rng(rand_gen):
    """evaluator._start's draw order written out: seed, the evaluator platoon's two constructor draws (front_accel, front_u), then the
    T leader inputs (tests/test_gpu_eval_cases.py compares with _start itself, which needs the device)."""
    conf = config.Config(rand_gen=rand_gen)
    draw = (lambda s: np.random.uniform(-s, s)) if rand_gen == "uniform" else (lambda s: np.random.normal(0, s))
    for seed in (None, 0, 99):
        np.random.seed(conf.evaluation_seed if seed is None else seed)
        draw(conf.pl_leader_reset_a), draw(conf.reset_max_u)
        want = np.array([draw(conf.reset_max_u) for _ in range(50)], dtype=np.float32)
        np.random.seed(4321)
        before = np.random.get_state()
        got = scenarios.leader_profile("gaussian", 50, conf, seed=seed)
        after = np.random.get_state()
        assert got.dtype == np.float32 and np.array_equal(got, want)
        assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert not np.array_equal(scenarios.leader_profile("gaussian", 50, conf, seed=1), scenarios.leader_profile("gaussian", 50, conf, seed=2))


@pytest.mark.parametrize("kw,match", [
    (dict(name="chirp"), "unknown scenario 'chirp'"),
    (dict(amp=float("nan")), "amp=nan is not finite"),
    (dict(amp=float("inf")), "not finite"),
    (dict(period_s=float("nan")), "period_s"),
    (dict(period_s=float("inf")), "period_s"),
    (dict(period_s=0.0), "must be finite and > 0"),
    (dict(period_s=-1.0), "must be finite and > 0"),
    (dict(T=3), "T=3"),
])
def test_profile_refusals(kw, match):
    a = dict(name="sine", T=600, amp=None, period_s=10.0)
    a.update(kw)
    with pytest.raises(ValueError, match=match):
        scenarios.leader_profile(a["name"], a["T"], config.Config(), amp=a["amp"], period_s=a["period_s"])


def test_scenario_lists_refuse_unknown_and_repeated_names():
    assert scenarios.check_names(("zero", "step")) == ["zero", "step"]
    with pytest.raises(ValueError, match="listed more than once"):
        scenarios.check_names(["step", "zero", "step"])
    with pytest.raises(ValueError, match="unknown scenario"):
        scenarios.check_names(["step", "Step"])
    with pytest.raises(ValueError, match="no scenario"):
        scenarios.check_names([])


# ---- 2. the metrics' definition against the float64 restatement ------------------------------------------------------------------

@pytest.mark.parametrize("model", ["ModelA", "ModelB"])
@pytest.mark.parametrize("L", [3, 5])
@pytest.mark.parametrize("name", ["step", "brake"])
def test_metrics_from_traces_against_the_float64_restatement(name, L, model):
    """Both sides from the oracle's own float64 rollout: the restatement forms the metrics inside its loop, metrics_from_traces from
    the traces cast to float32. This checks the definitions, not the GPU."""
    conf = config.Config(pl_size=L, model=model)
    T = 120
    leader = scenarios.leader_profile(name, T, conf)
    ref, x0, tr = so.rollout(so.env_params(conf), L, so.random_actors(conf, L, seed=7 + L), leader)
    assert np.abs(tr["inputs"]).max() > 0.05 and np.abs(tr["inputs"]).max() < conf.action_high
    tr32 = {k: v.astype(np.float32) for k, v in tr.items()}
    got = scenarios.metrics_from_traces(tr32, x0.astype(np.float32), conf)
    assert list(got) == list(scenarios.METRICS) and all(v.dtype == np.float32 and v.shape == (L,) for v in got.values())
    so.check_against(got, ref, T)


def test_terminal_steps_and_summary():
    """A hand-made trace: the terminal test reads the PRE-step state (x0, then the previous post-step state)."""
    conf = config.Config(pl_size=2)
    st = np.zeros((4, 2, 4), dtype=np.float32)
    st[:, 0, 0] = [1, 25, 2, 30]   # vehicle 1: |ep| > 20 after steps 1 and 3 -> terminal on step 2 only (step 4 does not exist)
    st[:, 1, 1] = [0, 0, -21, 0]   # vehicle 2: |ev| > 20 after step 2 -> terminal on step 3
    tr = dict(states=st, inputs=np.full((4, 2), 0.5, np.float32), jerks=np.tile(np.float32([1, -2]), (4, 1)))
    x0 = np.zeros((2, 4), dtype=np.float32)
    x0[1, 0] = -20.5              # vehicle 2 starts out of bounds -> terminal on step 0
    m = scenarios.metrics_from_traces(tr, x0, conf)
    assert m["term_steps"].tolist() == [1, 2] and m["first_term"].tolist() == [2, 0]
    assert m["max_abs_ep"].tolist() == [30, 0] and m["max_abs_ev"].tolist() == [0, 21] and m["final_abs_ep"].tolist() == [30, 0]
    assert m["sum_u2"].tolist() == [1, 1] and m["sum_jerk2"].tolist() == [4, 16]
    off = scenarios.metrics_from_traces(tr, x0, config.Config(pl_size=2, can_terminate=False))
    assert off["term_steps"].tolist() == [0, 0] and off["first_term"].tolist() == [-1, -1]
    s = scenarios.summarise(m, 4)
    assert s["rms_u"].tolist() == [0.5, 0.5] and s["rms_jerk"].tolist() == [1, 2]
    assert np.isnan(s["ss_ratio"][0]) and s["ss_ratio"][1] == 0 and bool(s["string_stable"]) is True
    grow = scenarios.summarise(dict(m, max_abs_ep=np.float32([[1, 2, 1], [2, 1, 1]])), 4)
    assert grow["string_stable"].tolist() == [False, True] and grow["ss_ratio"][0, 1:].tolist() == [2, 0.5]


# ---- 3. the entry point's refusals --------------------------------------------------------------------------------------------------

def _args(**kw):
    """Valid arguments of a decentralized L = 5 launch (reference widths), with `kw` overriding some."""
    a = dict(lay=C.byref(_hip.make_layout(4, 1, 256, 128, 48, 64)), consts=FAKE, G=8, K=12, L=5, M=5, T=600, theta=FAKE, stats=FAKE,
             n_sets=40, set_base=FAKE, x0=FAKE, prev_a0=FAKE, leader=FAKE, high=2.5, lo=-2.5, hi=2.5, sample_rate=0.1, counters=FAKE,
             metrics=None, stream=None)
    a.update(kw)
    return list(a.values())


def _rc_and_message(**kw):
    lib = _hip.lib()
    rc = lib.avd_eval_cases_f32(*_args(**kw))
    return rc, lib.avd_last_error().decode()


@pytest.mark.parametrize("kw,match", [
    (dict(lay=None), "null layout or constants"),
    (dict(consts=None), "null layout or constants"),
    (dict(theta=None), "null pointer"),
    (dict(stats=None), "null pointer"),
    (dict(set_base=None), "null pointer"),
    (dict(x0=None), "null pointer"),
    (dict(prev_a0=None), "null pointer"),
    (dict(leader=None), "null pointer"),
    (dict(counters=None), "null pointer"),
    (dict(L=0, M=0), "L=0 (L must be 1..16)"),
    (dict(L=17, M=17), "L=17 (L must be 1..16)"),
    (dict(M=2), "M=2 (M must be L=5"),
    (dict(M=0), "M=0 (M must be L=5"),
    (dict(G=0), "G=0 K=12 T=600 (all must be >= 1)"),
    (dict(K=0), "G=8 K=0 T=600"),
    (dict(K=-2), "K=-2"),
    (dict(T=0), "T=0 (all must be >= 1)"),
    (dict(n_sets=4), "n_sets=4 (need n_sets >= M=5)"),
    (dict(sample_rate=0.0), "sample_rate=0"),
    (dict(sample_rate=-0.1), "sample_rate=-0.1"),
    (dict(M=1), "does not fit L=5 M=1"),
])
def test_bad_arguments_are_refused_before_any_hip_call(kw, match):
    rc, msg = _rc_and_message(**kw)
    assert rc == AVD_E_INVALID and msg.startswith("avd_eval_cases_f32: ") and match in msg, (rc, msg)


def test_layout_and_lds_limits():
    cen = C.byref(_hip.make_layout(12, 3, 320, 160, 64, 64))
    rc, msg = _rc_and_message(lay=cen, L=3, M=3)
    assert rc == AVD_E_INVALID and "layout S=12 A=3 does not fit L=3 M=3" in msg
    huge = C.byref(_hip.make_layout(4, 1, 2048, 2048, 48, 64))  # 16 rows of 4096 hidden floats: 256 KiB
    rc, msg = _rc_and_message(lay=huge, K=16)
    assert rc == AVD_E_UNSUPPORTED and "of LDS for blocks of 16 cases (> 160 KiB)" in msg
    with pytest.raises(_hip.AvdError, match=r"avd_eval_cases_f32 failed \(-1\): .*L=99"):
        _hip.call("avd_eval_cases_f32", *_args(L=99, M=99))


def test_block_size_is_named_by_the_host():
    """avd_eval_cases_block: the smallest instantiated block that holds all K cases, else the largest; RB * L <= 256."""
    blk = _hip.lib().avd_eval_cases_block
    sizes = sorted({blk(K, L) for K in range(1, 80) for L in (1, 5, 16)})
    assert sizes[0] == 1 and all(rb * 16 <= 256 for rb in sizes) and len(sizes) >= 3
    for L in (1, 5, 16):
        assert blk(1, L) == 1
        for rb in sizes:
            assert blk(rb, L) == rb and blk(3 * sizes[-1] + 2, L) == sizes[-1]
        for K in range(1, 80):
            rb = blk(K, L)
            assert rb >= min(K, sizes[-1]) and not any(s >= K and s < rb for s in sizes)
    assert blk(0, 5) == AVD_E_INVALID and "K=0" in _hip.lib().avd_last_error().decode()
    assert blk(4, 17) == AVD_E_INVALID and "L=17" in _hip.lib().avd_last_error().decode()


# ---- 4. the parser -----------------------------------------------------------------------------------------------------------------

def _parse(*argv):
    return cli.get_cmdl_args(list(argv), config.Config())


@pytest.mark.parametrize("argv,match", [
    (["tr", "--eval_seeds", "6"], "--eval_seeds needs --scenarios"),
    (["tr", "--scenario_amp", "0.2"], "--scenario_amp needs --scenarios"),
    (["tr", "--scenario_period", "5"], "--scenario_period needs --scenarios"),
    (["esim", "d", "--eval_seeds", "6"], "--eval_seeds needs --scenarios"),
    (["esim", "d", "--scenario_amp", "0.2"], "--scenario_amp needs --scenarios"),
    (["esim", "d", "--scenario_period", "5"], "--scenario_period needs --scenarios"),
    (["tr", "--scenarios", "zero,chirp"], "unknown scenario 'chirp'"),
    (["esim", "d", "--scenarios", "step,step"], "listed more than once"),
    (["tr", "--scenarios", ""], "unknown scenario ''"),
    (["tr", "--scenarios", "zero", "--eval_seeds", "3,3"], "--eval_seeds: seed"),
    (["tr", "--scenarios", "zero", "--eval_seeds", "9-7"], "runs backwards"),
    (["esim", "d", "--scenarios", "zero", "--eval_seeds", "x"], "--eval_seeds: 'x'"),
    (["tr", "--scenarios", "sine", "--scenario_period", "0"], "--scenario_period must be finite and > 0"),
    (["tr", "--scenarios", "sine", "--scenario_amp", "nan"], "--scenario_amp must be finite"),
])
def test_parser_refusals(argv, match, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(*argv)
    assert e.value.code == 2 and match in capsys.readouterr().err


def test_tr_scenarios_is_refused_under_several_ranks(monkeypatch, capsys):
    """The choice the issue leaves open: refused (scenarios.csv is not gathered across ranks), not one file per rank."""
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        _parse("tr", "--scenarios", "zero")
    assert "more than one rank" in capsys.readouterr().err
    args, _ = _parse("esim", "d", "--scenarios", "zero")  # esim runs in one process
    assert args.scenarios == ["zero"]
    monkeypatch.setenv("WORLD_SIZE", "1")
    assert _parse("tr", "--scenarios", "zero")[0].scenarios == ["zero"]


def test_parsed_flags_and_unchanged_defaults():
    args, conf = _parse("tr", "--scenarios", "zero,step,ramp,brake,sine,gaussian", "--eval_seeds", "6,7-9", "--scenario_amp", "0.3",
                        "--scenario_period", "4")
    assert args.scenarios == ["zero", "step", "ramp", "brake", "sine", "gaussian"] and args.eval_seeds == [6, 7, 8, 9]
    assert (args.scenario_amp, args.scenario_period) == (0.3, 4.0)
    assert cli._suite(args) == dict(scenarios=args.scenarios, seeds=[6, 7, 8, 9], amp=0.3, period_s=4.0)
    new = {"scenarios", "eval_seeds", "scenario_amp", "scenario_period"}
    for argv in (["tr", "--pl_num", "3"], ["esim", "some/dir", "--n_timesteps", "50"]):
        plain, pconf = _parse(*argv)
        with_flag, fconf = _parse(*argv, "--scenarios", "zero")
        assert all(getattr(plain, k) is None for k in new)
        # without the flag nothing else in the namespace or the Config differs from a run with it, and neither carries a suite
        assert {k: v for k, v in vars(plain).items() if k not in new} == {k: v for k, v in vars(with_flag).items() if k not in new}
        assert pconf.__dict__ == fconf.__dict__ == cli.set_args_to_config(copy.copy(plain), config.Config()).__dict__
        assert not hasattr(pconf, "scenario_suite")
    assert set(vars(_parse("esim", "d")[0])) == {"mode", "exp_path", "n_timesteps"} | new
