"""Residual policies without a GPU: the parser and check_residual's refusals, trainer.check_residual, conf.json's residual_law round
trip, the float64 oracle against the linear oracle, the float32 law at zero gains, what the three new entry points refuse on the host,
the ABI's three places and the CLI's argument errors."""
import ctypes
import fnmatch
import json
import os
import re

import numpy as np
import pytest

from avddpg_amd import __main__ as cli
from avddpg_amd import _hip, artifacts, config, scenarios, trainer
from avddpg_amd.scenarios import ResidualLaw, check_residual, parse_residual
from tests import linear_oracle, residual_oracle, scenario_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["avd_step_fused_res_f32", "avd_eval_rollout_res_f32", "avd_eval_cases_res_f32"]


def test_parse_residual():
    law = parse_residual("kp=2,kv=1")
    assert isinstance(law, ResidualLaw) and (law.kp, law.kv, law.ka, law.kf, law.scale, law.source) == (2.0, 1.0, 0, 0, 1.0, "given")
    law = parse_residual(" kp=0.5, kv=1 ,ka=-0.25,kf=0.75,scale=0.5 ")
    assert (law.kp, law.kv, law.ka, law.kf, law.scale) == (0.5, 1.0, -0.25, 0.75, 0.5)
    assert parse_residual("tuned") == scenarios.TUNED == parse_residual(" tuned ")
    assert np.array_equal(law.gains(3), np.tile(np.float32([0.5, 1, -0.25, 0.75]), (3, 1)))
    assert check_residual(law, config.Config()) is law


@pytest.mark.parametrize("text,msg", [
    ("", "no gain given"),
    ("kp=2,gain=1", "unknown key 'gain'"),
    ("kp", "unknown key 'kp'"),
    ("kp=1,kp=2", "kp given twice"),
    ("kp=1,scale=0.5,scale=1", "scale given twice"),
    ("kp=big", "kp='big' is not a number"),
    ("best", "unknown key 'best'"),
])
def test_parse_residual_refusals(text, msg):
    with pytest.raises(ValueError, match=msg):
        parse_residual(text)


def test_check_residual_refusals():
    modelA = config.Config(model="ModelA")
    assert modelA.model == modelA.modelA
    with pytest.raises(ValueError, match="is not a scenarios.ResidualLaw"):
        check_residual(scenarios.LinearLaw("x", 1, 1))
    with pytest.raises(ValueError, match="kp=nan must be a finite number"):
        check_residual(ResidualLaw(kp=float("nan")))
    with pytest.raises(ValueError, match="kv=inf must be a finite number"):
        check_residual(ResidualLaw(kv=float("inf")))
    with pytest.raises(ValueError, match="kf needs Model B"):
        check_residual(ResidualLaw(1, 1, 0, 0.5), modelA)
    assert check_residual(ResidualLaw(1, 1, 0.5, 0), modelA).ka == 0.5
    with pytest.raises(ValueError, match=r"table must be a finite \[L, 4\] array"):
        check_residual(ResidualLaw(table=np.zeros((5, 3))))
    with pytest.raises(ValueError, match=r"table must be a finite \[L, 4\] array"):
        check_residual(ResidualLaw(table=np.full((5, 4), np.nan)))
    with pytest.raises(ValueError, match="a gain table of 4 rows for pl_size=5"):
        check_residual(ResidualLaw(table=np.zeros((4, 4))), config.Config(pl_size=5))
    tab = np.zeros((5, 4))
    tab[2, 3] = 0.1
    with pytest.raises(ValueError, match="kf needs Model B"):
        check_residual(ResidualLaw(table=tab), config.Config(model="ModelA", pl_size=5))
    with pytest.raises(ValueError, match="not available for the centralized framework"):
        check_residual(ResidualLaw(1, 1), config.Config(framework="centralized"))
    for sc in (0, -0.5, 1.5, float("nan"), float("inf"), "1", True):
        with pytest.raises(ValueError, match=r"scale=.* must be a number in \(0, 1\]"):
            check_residual(ResidualLaw(1, 1, scale=sc))
    assert check_residual(ResidualLaw(1, 1, scale=1)).scale == 1 and check_residual(ResidualLaw(1, 1, scale=1e-3)).scale == 1e-3


def test_trainer_check_residual_refusals():
    law = ResidualLaw(2, 1)
    ok = lambda **kw: trainer.check_residual(kw.pop("conf", config.Config()), kw.pop("law", law), kw.pop("rng", "device"), **kw)
    assert ok() is law and ok(fused_step=True) is law and ok(world_size=1) is law
    with pytest.raises(ValueError, match="a residual policy needs the decentralized framework"):
        ok(conf=config.Config(framework="centralized"))
    with pytest.raises(ValueError, match="a residual policy needs rng='device'"):
        ok(rng="host")
    with pytest.raises(ValueError, match=r"a residual policy needs the fused step \(fused_step=False"):
        ok(fused_step=False)
    with pytest.raises(ValueError, match="does not combine with a hyperparameter sweep or PBT"):
        ok(hparams=[dict(actor_lr=1e-4)])
    with pytest.raises(ValueError, match="runs on one rank: no process group of more than one rank"):
        ok(world_size=2)
    with pytest.raises(ValueError, match=r"scale=2 must be a number in \(0, 1\]"):
        ok(law=ResidualLaw(1, 1, scale=2))
    # the trainer refuses before it allocates: no GPU here, so anything past the check would fail differently
    small = lambda **kw: config.Config(num_platoons=2, pl_size=2, **kw)
    with pytest.raises(ValueError, match="a residual policy needs rng='device'"):
        trainer.VecTrainer(small(), rng="host", residual=law)
    with pytest.raises(ValueError, match="a residual policy needs the fused step"):
        trainer.VecTrainer(small(), rng="device", fused_step=False, residual=law)
    with pytest.raises(ValueError, match="a residual policy needs the decentralized framework"):
        trainer.VecTrainer(small(framework="centralized"), rng="device", residual=law)
    with pytest.raises(ValueError, match="does not combine with a hyperparameter sweep or PBT"):
        trainer.VecTrainer(small(), rng="device", auto_reset="platoon", seeds=[1, 2], hparams=[dict(actor_lr=1e-4), dict(actor_lr=2e-4)],
                           residual=law)


def test_conf_json_round_trip(tmp_path):
    tab = np.arange(20, dtype=np.float64).reshape(5, 4) / 8
    for law in (ResidualLaw(2, 1), ResidualLaw(0.5, 1, -0.25, 0.75, scale=0.25, source="tuned"), ResidualLaw(table=tab, scale=0.5)):
        conf = config.Config(pl_size=5)
        conf.residual_law = law.record()
        path = str(tmp_path / "conf.json")
        artifacts.config_writer(path, conf)
        rec = json.load(open(path))["residual_law"]
        assert [k for k, _ in rec][:5] == ["kp", "kv", "ka", "kf", "scale"] and rec[-1][0] == "source"
        back = ResidualLaw.from_record(rec)
        assert (back.kp, back.kv, back.ka, back.kf, back.scale, back.source) == (law.kp, law.kv, law.ka, law.kf, law.scale, law.source)
        assert np.array_equal(back.gains(5), law.gains(5)) and (back.table is None) == (law.table is None)
        assert back.record() == rec and check_residual(back, conf) is back
        assert artifacts.config_loader(path, config.Config).pl_size == conf.pl_size  # (the loader passes over the new field)
    assert ResidualLaw.from_record(None) is None
    with pytest.raises(ValueError, match="unknown or repeated key"):
        ResidualLaw.from_record([["kp", 1], ["gain", 2]])


@pytest.mark.parametrize("dist", [{}, dict(v2v_delay=2, v2v_drop=0.1, sigma=(0.05, 0.0, 0.02))])
def test_oracle_with_zero_actors_is_the_linear_oracle(dist):
    conf = config.Config(pl_size=3)
    ep, L, T = scenario_oracle.env_params(conf), 3, 25
    actors = scenario_oracle.random_actors(conf, L, 11, last_scale=0.0)
    for w in actors:
        w[13] = np.zeros_like(w[13])  # the last layer's bias
    gains = np.array([[1.0, 2.0, -0.5, 1.0], [0.5, 1.0, 0.0, 0.25], [2.0, 0.5, -1.0, 0.0]])
    leader = scenarios.leader_profile("brake", T, conf)
    m, x0, tr = residual_oracle.rollout(ep, L, actors, gains, 0.5, leader, **dist)
    rm, rx0, rtr = linear_oracle.rollout(ep, L, gains, leader, **dist)
    assert not tr["residual"].any() and np.array_equal(x0, rx0)
    for k in rm:
        assert np.array_equal(m[k], rm[k]), k
    for k in ("states", "inputs", "jerks", "counters"):
        assert np.array_equal(tr[k], rtr[k]), k
    assert np.abs(tr["inputs"]).max() > 0.1  # (the law acts)


@pytest.mark.parametrize("delay", [0, 3])
def test_float32_loop_stays_inside_half_the_oracle_tolerances_on_the_gpu_tests_inputs(delay):
    """What tests/test_gpu_residual.py's oracle test rests on: for ITS actors and law, float32 arithmetic alone (the CPU loop) keeps every
    metric inside half of scenario_oracle.check_against's tolerances against the float64 oracle."""
    conf = config.Config(pl_size=5)
    ep, L, T = scenario_oracle.env_params(conf), 5, conf.steps_per_episode
    actors = scenario_oracle.random_actors(conf, L, 31, last_scale=400.0)
    gains = np.tile([0.5, 1.0, 0.0, 0.3], (L, 1))
    leader = scenarios.leader_profile("gaussian", T, conf, seed=6)
    m64, x0, tr = residual_oracle.rollout(ep, L, actors, gains, 0.5, leader, v2v_delay=delay)
    m32, _ = residual_oracle.rollout32(ep, L, actors, gains, 0.5, leader, x0, conf, v2v_delay=delay)
    for k in ("max_abs_ep", "max_abs_ev", "max_abs_a", "final_abs_ep"):
        assert np.all(np.abs(m32[k] - m64[k]) <= 0.5 * (2e-4 + 1e-4 * np.abs(m64[k]))), k
    for s, atol in (("sum_u2", 5e-5), ("sum_jerk2", 5e-3)):
        assert np.all(np.abs(np.sqrt(m32[s].astype(np.float64) / T) - np.sqrt(m64[s] / T)) <= 0.5 * atol), s
    assert not m64["term_steps"].any() and np.array_equal(m32["term_steps"], m64["term_steps"])
    assert np.sqrt(np.mean(tr["residual"] ** 2)) > 0.05 and np.any(np.abs(tr["inputs"]) == 2.5)


@pytest.mark.parametrize("model_a", [False, True])
def test_law_with_zero_gains_is_the_clip(model_a):
    rs = np.random.RandomState(5)
    r = np.concatenate([rs.uniform(-4, 4, 4000), [0.0, -0.0, 2.5, -2.5, 1e-30, -1e-30, 3.0, -3.0]]).astype(np.float32)
    ob = rs.normal(0, 2, (r.size, 4)).astype(np.float32)
    for zero in (0.0, -0.0):
        u = residual_oracle.law(np.full(4, zero, np.float32), ob, 1.0, r, -2.5, 2.5, model_a)
        assert u.dtype == np.float32 and np.array_equal(u, np.clip(r, np.float32(-2.5), np.float32(2.5)))  # (as values: -0 == +0)
    # and with gains it is the formula, each operation rounded to float32
    g = np.float32([1.0, 2.0, -0.5, 1.0])
    f = np.float32
    z = f(f(f(g[0] * ob[:, 0]) + f(g[1] * ob[:, 1])) + f(g[2] * ob[:, 2]))
    z = z if model_a else f(z + f(g[3] * ob[:, 3]))
    want = np.clip(f(z + f(f(0.25) * r)), f(-2.5), f(2.5))
    assert np.array_equal(residual_oracle.law(g, ob, 0.25, r, -2.5, 2.5, model_a), want)


def test_abi_names_in_header_export_map_and_binding():
    header = open(_hip.HEADER_PATH).read()
    globs = re.findall(r"global:\s*([^;]+);", open(os.path.join(ROOT, "avddpg_amd", "csrc", "exports.map")).read())
    patterns = [p.strip() for g in globs for p in g.split(",")]
    for name in NEW:
        assert re.search(rf"\bint {name}\(", header), name
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), name
        assert name in _hip._PROTOS
        assert getattr(_hip.lib(), name) is not None


# ---- the entry points' host checks ------------------------------------------------------------------------------------------------
_B = lambda k: ctypes.c_void_p(0x1000 * (k + 1))  # non-null, 16-byte aligned "device pointers" nothing reads: every call is refused on the host


def _step_call(gains=_B(50), scale=0.5, n_levels=0, n_man=0, seeds=None, n_groups=2, consts=_B(0), obs_in=_B(22), table=_B(40)):
    head = [consts, 8, 2, 4, _B(1), _B(2), _B(3), None, _B(4), None, _B(5), None, None, _B(6), _B(7), _B(8), _B(9), 0.15, 0.0, 0.1, 0.2,
            -2.5, 2.5, 0.1, 0, 7, 3, 4, None, 8, 0, None]
    levels = (_hip.TrainLevel * max(1, min(n_levels, 16)))()
    dist = [n_levels, levels, _B(20), _B(21), obs_in, _B(23), None, None, 1]
    lead = [n_man, 12, table, _B(41), _B(42), _B(43), 0]
    _hip.call("avd_step_fused_res_f32", *head, seeds, n_groups, *dist, *lead, gains, scale, None, None)


def test_step_entry_point_refuses_on_the_host_before_any_hip_call():
    refuse = lambda msg: pytest.raises(_hip.AvdError, match=rf"failed \(-1\): avd_step_fused_res_f32: {msg}")
    with refuse(r"gains=.* \(must be a non-null, 16-byte aligned \[L\]\[4\] table\)"):
        _step_call(gains=None)
    with refuse(r"gains=.* \(must be a non-null, 16-byte aligned"):
        _step_call(gains=ctypes.c_void_p(0x1004))
    for sc in (0.0, -1.0, 1.5, float("nan")):
        with refuse(r"scale=.* \(must be in \(0, 1\]\)"):
            _step_call(scale=sc)
    with refuse(r"n_levels=-1 n_manoeuvres=0 \(0: none\)"):
        _step_call(n_levels=-1)
    with refuse(r"n_levels=17 \(must be 1..16\)"):
        _step_call(n_levels=17)
    with refuse(r"obs_in=.* \(must be 16-byte aligned\)"):
        _step_call(n_levels=1, obs_in=ctypes.c_void_p(0x2008))
    with refuse(r"n_manoeuvres=17 \(must be 1..16\)"):
        _step_call(n_man=17)
    with refuse("null manoeuvre table, noise table or gaussian flags"):
        _step_call(n_man=2, table=None)
    with refuse(r"d_seeds=.* n_groups=3 P=8 \(P must be a multiple of n_groups\)"):
        _step_call(seeds=_B(10), n_groups=3)
    # past its own checks the step's apply, with or without levels, manoeuvres and a seed table: a null constants block
    for kw in (dict(), dict(n_levels=2), dict(n_man=2), dict(n_levels=2, n_man=2), dict(seeds=_B(10), n_levels=1, n_man=1)):
        with refuse("null pointer"):
            _step_call(consts=None, **kw)


def _eval_call(entry, M=5, gains=_B(50), scale=1.0, lay=None):
    lay = _hip.make_layout(4, 1, 256, 128, 48, 64) if lay is None else lay
    L = 5
    if entry == "avd_eval_rollout_res_f32":
        _hip.call(entry, ctypes.byref(lay), _B(0), 2, L, M, 10, _B(1), _B(2), 8, _B(3), _B(4), _B(5), _B(6), 1, _B(7), 2.5, -2.5, 2.5, 0.1,
                  _B(8), 0, None, None, None, None, gains, scale, None)
    else:
        _hip.call(entry, ctypes.byref(lay), _B(0), 1, 2, L, M, 10, _B(1), _B(2), 8, _B(3), _B(4), _B(5), _B(6), 2.5, -2.5, 2.5, 0.1,
                  None, None, None, None, None, gains, scale, _B(8), _B(9), None)


@pytest.mark.parametrize("entry", NEW[1:])
def test_evaluator_entry_points_refuse_on_the_host_before_any_hip_call(entry):
    with pytest.raises(_hip.AvdError, match=rf"failed \(-1\): {entry}: gains=.* \(must be a non-null, 16-byte aligned"):
        _eval_call(entry, gains=None)
    with pytest.raises(_hip.AvdError, match=rf"failed \(-1\): {entry}: gains=.* \(must be a non-null, 16-byte aligned"):
        _eval_call(entry, gains=ctypes.c_void_p(0x1008))
    for sc in (0.0, 1.25, float("nan")):
        with pytest.raises(_hip.AvdError, match=rf"failed \(-1\): {entry}: scale=.* \(must be in \(0, 1\]\)"):
            _eval_call(entry, scale=sc)
    cen = _hip.make_layout(20, 5, 307, 153, 57, 64)
    with pytest.raises(_hip.AvdError, match=rf"failed \(-3\): {entry}: M=1 L=5 \(a residual on a per-vehicle law needs decentralized agents"):
        _eval_call(entry, M=1, lay=cen)


def test_cases_entry_point_refuses_a_partial_disturbance_table():
    lay = _hip.make_layout(4, 1, 256, 128, 48, 64)
    with pytest.raises(_hip.AvdError, match=r"avd_eval_cases_res_f32: null disturbance table \(all five null"):
        _hip.call("avd_eval_cases_res_f32", ctypes.byref(lay), _B(0), 1, 2, 5, 5, 10, _B(1), _B(2), 8, _B(3), _B(4), _B(5), _B(6), 2.5, -2.5,
                  2.5, 0.1, _B(10), None, _B(12), _B(13), None, _B(50), 1.0, _B(8), _B(9), None)


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv,msg", [
    (["--rng", "host", "--residual", "kp=2,kv=1"], "--residual needs --rng device"),
    (["--residual", "kp=2,kv=1"], "--residual needs --rng device"),
    (["--rng", "device", "--episodes", "platoon", "--sweep", "actor_lr=1e-4,2e-4", "--residual", "kp=2,kv=1"],
     "--residual does not combine with --sweep / --pbt"),
    (["--rng", "device", "--residual", "kp=2,gain=1"], "--residual: residual: unknown key 'gain'"),
    (["--rng", "device", "--residual", "kp=nan"], "--residual: baseline 'residual': kp=nan must be a finite number"),
    (["--rng", "device", "--residual", "kp=2,scale=0"], r"--residual: residual: scale=0.0 must be a number in \(0, 1\]"),
    (["--rng", "device", "--residual", "tuned"], "--residual tuned needs --scenarios and --baseline_tune"),
    (["--rng", "device", "--residual", "tuned", "--scenarios", "gaussian"], "--residual tuned needs --scenarios and --baseline_tune"),
])
def test_cli_argument_errors(argv, msg, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        cli.get_cmdl_args(["tr", *argv], config.Config())
    assert e.value.code == 2 and re.search(msg, capsys.readouterr().err)


def test_cli_refuses_more_than_one_rank_and_what_needs_the_configuration(capsys, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        cli.get_cmdl_args(["tr", "--rng", "device", "--residual", "kp=2,kv=1"], config.Config())
    assert e.value.code == 2 and "--residual is not available under a process group of more than one rank" in capsys.readouterr().err
    monkeypatch.delenv("WORLD_SIZE")
    args, conf = cli.get_cmdl_args(["tr", "--rng", "device", "--residual", "kp=2,kv=1,kf=0.5,scale=0.5"], config.Config())
    assert isinstance(args.residual, ResidualLaw) and (args.residual.kf, args.residual.scale) == (0.5, 0.5)
    with pytest.raises(SystemExit, match="--residual: baseline 'residual': kf needs Model B"):
        cli._resolve_residual(args, config.Config(model="ModelA"), "platoon")
    with pytest.raises(SystemExit, match="--residual: a residual policy needs the decentralized framework"):
        cli._resolve_residual(args, config.Config(framework="centralized"), "platoon")
    cli._resolve_residual(args, conf, "platoon")
    c2 = config.Config()
    cli._record_residual(c2, args)
    assert c2.residual_law == args.residual.record() and dict(c2.residual_law)["source"] == "given"
    args, _ = cli.get_cmdl_args(["tr", "--rng", "device"], config.Config())
    assert args.residual is None and cli._residual_kw(args) == {}
    cli._record_residual(c2 := config.Config(), args)
    assert not hasattr(c2, "residual_law")
