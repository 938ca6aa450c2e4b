"""Delayed policy updates without a device (tr --policy_delay, trainer.check_policy_delay, the host checks of
avd_adam_polyak_delayed_f32 and avd_learn_set_split_td_f16x3, tests/delay_oracle.py): the policy-call schedule, every refusal of
check_policy_delay, of the trainer, of the CLI and of the two entry points, conf.json's field, and the oracle's own properties -- a
policy call with equal counts is the guarded update, a skipped call moves the critic's weights and moments and nothing else."""
import ctypes
import json
import math

import numpy as np
import pytest

from avddpg_amd import __main__ as cli
from avddpg_amd import _hip, artifacts, config, trainer
from avddpg_amd.trainer import TargetNoise
from tests import delay_oracle as do

FUSED3 = ["--fed_method", "interfrl", "--engine", "fused3", "--rng", "device"]
ACTOR_LR, CRITIC_LR, TAU = 1e-4, 1e-3, 0.005


def _interfrl(**kw):
    return config.Config(fed_method="interfrl", **kw)


# ---- the schedule ----

def test_policy_call_schedule():
    assert do.schedule(7, 3) == [False, False, True, False, False, True, False]
    assert do.schedule(4, 1) == [True] * 4 and do.schedule(5, 2) == [False, True, False, True, False]
    for d in (1, 2, 3, 7):
        assert [trainer.is_policy_call(k, d) for k in range(30)] == do.schedule(30, d)
        assert sum(do.schedule(30, d)) == 30 // d
    assert all(trainer.is_policy_call(k, None) for k in range(5))  # no delay: every call


# ---- the oracle's own properties ----

def _state(n_sets=5, T=64, S=8, A=24, seed=3, **kw):
    h, scale, rs = do.host_state(n_sets, T, S, seed, **kw)
    return h, do.gradients(scale, rs), A


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def test_oracle_policy_call_with_equal_counts_is_the_guarded_update():
    h, g, A = _state(step=5, actor_step=5)
    g[3, 0] = np.nan  # a guarded set on both sides
    twin = {k: x.copy() for k, x in h.items()}
    for _ in range(3):
        assert do.delayed_call(h, g, True, A, ACTOR_LR, CRITIC_LR, TAU) == 1
        assert do.guarded_call(twin, g, A, ACTOR_LR, CRITIC_LR, TAU) == 1
    for k in ("theta", "theta_t", "m", "v", "stats_t", "step"):
        assert np.array_equal(_bits(h[k]), _bits(twin[k])), k
    assert np.array_equal(h["actor_step"], h["step"]) and h["step"].tolist() == [8, 8, 8, 5, 8]


def test_oracle_skipped_call_moves_the_critics_weights_and_moments_only():
    h, g, A = _state()
    g[:, :A] = np.nan  # the actor block of the gradients may hold anything
    before = {k: x.copy() for k, x in h.items()}
    assert do.delayed_call(h, g, False, A, ACTOR_LR, CRITIC_LR, TAU) == 0
    for k in ("theta", "m", "v"):
        assert np.array_equal(_bits(h[k][:, :A]), _bits(before[k][:, :A])), k
        assert not np.array_equal(_bits(h[k][:, A:]), _bits(before[k][:, A:])), k
    for k in ("theta_t", "stats_t", "stats", "actor_step"):
        assert np.array_equal(_bits(h[k]), _bits(before[k])), k
    assert np.array_equal(h["step"], before["step"] + 1)
    # the critic's step is Adam's at iteration step, by the oracle's own functions
    from oracle import mlp as omlp
    w, m, v = (before[k][0, A:].copy() for k in ("theta", "m", "v"))
    omlp.adam_update(w, m, v, g[0, A:], omlp.adam_alpha(CRITIC_LR, 6))
    assert np.array_equal(_bits(w), _bits(h["theta"][0, A:]))


def test_oracle_guard_by_call_kind():
    h, g, A = _state()
    g[1, A] = np.inf  # the critic's head: guarded on both kinds
    g[2, 0] = np.nan  # the actor's head: guarded on a policy call only
    before = {k: x.copy() for k, x in h.items()}
    assert do.delayed_call(h, g, False, A, ACTOR_LR, CRITIC_LR, TAU) == 1
    assert h["step"].tolist() == [6, 5, 6, 6, 6] and h["actor_step"].tolist() == [2] * 5
    assert np.array_equal(_bits(h["theta"][1]), _bits(before["theta"][1])) and not np.array_equal(_bits(h["theta"][2]), _bits(before["theta"][2]))
    assert do.delayed_call(h, g, True, A, ACTOR_LR, CRITIC_LR, TAU) == 2
    assert h["step"].tolist() == [7, 5, 6, 7, 7] and h["actor_step"].tolist() == [3, 2, 2, 3, 3]
    assert np.array_equal(_bits(h["theta_t"][[1, 2]]), _bits(before["theta_t"][[1, 2]]))


# ---- trainer and CLI ----

def test_check_policy_delay_refusals():
    ok = _interfrl()
    assert trainer.check_policy_delay(2, ok, "fused3") == 2 and trainer.check_policy_delay(1) == 1
    assert trainer.check_policy_delay(np.int64(3), ok, "fused3", steps=67) == 3  # 67 steps: 3 learner calls past the 64-row gate
    assert trainer.check_policy_delay(3, steps=4) == 3  # (without a configuration the gate is not known)
    for d, steps in ((4, 67), (50, 100), (37, 100), (2, 65), (1, 64)):
        with pytest.raises(ValueError, match=rf"policy_delay={d} is above the {steps - 64} learner calls"):
            trainer.check_policy_delay(d, ok, "fused3", steps=steps)
    assert trainer.check_policy_delay(36, ok, "fused3", steps=100) == 36
    for d in (0, -1, 2.0, 2.5, "2", True, None, math.nan):
        with pytest.raises(ValueError, match="policy delay: policy_delay="):
            trainer.check_policy_delay(d, ok, "fused3")
    for steps in (2, 1):
        with pytest.raises(ValueError, match="is not below the run's"):
            trainer.check_policy_delay(2, ok, "fused3", steps=steps)
    for engine in (None, "per_agent", "batched", "fused"):
        with pytest.raises(ValueError, match="policy delay needs shared_engine='fused3'"):
            trainer.check_policy_delay(2, ok, engine)
    with pytest.raises(ValueError, match="policy delay needs rng='device'"):
        trainer.check_policy_delay(2, ok, "fused3", rng="host")
    with pytest.raises(ValueError, match="hyperparameter sweep or PBT"):
        trainer.check_policy_delay(2, ok, "fused3", hparams=[{}])
    with pytest.raises(ValueError, match="overlap_allreduce"):
        trainer.check_policy_delay(2, ok, "fused3", overlap_allreduce=True)
    with pytest.raises(ValueError, match="policy delay runs on one rank"):
        trainer.check_policy_delay(2, ok, "fused3", world_size=2)
    with pytest.raises(ValueError, match="policy delay needs the decentralized framework"):
        trainer.check_policy_delay(2, _interfrl(framework="centralized"), "fused3")
    for conf in (config.Config(fed_method="intrafrl"), config.Config()):
        with pytest.raises(ValueError, match="policy delay needs shared weight sets"):
            trainer.check_policy_delay(2, conf, "fused3")
    with pytest.raises(ValueError, match="policy delay needs shared weight sets"):
        trainer.check_policy_delay(2, ok, "fused3", shared_sets=False)


def test_the_trainer_refuses_before_anything_is_allocated(monkeypatch):
    from avddpg_amd import vec

    def boom(*a, **k):
        raise AssertionError("something was allocated")

    for name in ("VecPlatoon", "AgentGroup", "VecReplay", "VecOUNoise"):
        monkeypatch.setattr(vec, name, boom)
    for kw, msg in ((dict(shared_engine="fused"), "needs shared_engine='fused3'"), (dict(shared_engine="fused3", rng="host"), "needs rng='device'"),
                    (dict(shared_engine="fused3", overlap_allreduce=True), "overlap_allreduce"),
                    (dict(shared_engine="fused3", seeds=(1, 2), hparams=[{}, {}]), "hyperparameter sweep or PBT"),
                    (dict(shared_engine="fused3", policy_delay=0), "must be >= 1"), (dict(shared_engine="fused3", policy_delay=1.5), "whole number")):
        with pytest.raises(ValueError, match=msg):
            trainer.VecTrainer(_interfrl(), **{**dict(rng="device", policy_delay=2), **kw})
    with pytest.raises(ValueError, match="needs the decentralized framework"):
        trainer.VecTrainer(_interfrl(framework="centralized"), rng="device", shared_engine="fused3", policy_delay=2)


@pytest.mark.parametrize("argv,msg", [
    (["--policy_delay", "2", "--rng", "device", "--fed_method", "interfrl"], "--policy_delay needs --engine fused3"),
    (["--policy_delay", "2", "--rng", "device", "--fed_method", "interfrl", "--engine", "per_agent"], "--policy_delay needs --engine fused3"),
    (["--policy_delay", "2", "--rng", "device", "--fed_method", "interfrl", "--engine", "batched"], "--policy_delay needs --engine fused3"),
    (["--policy_delay", "2", "--rng", "device", "--fed_method", "interfrl", "--engine", "fused"], "--policy_delay needs --engine fused3"),
    (["--policy_delay", "2", "--fed_method", "interfrl", "--engine", "fused3", "--rng", "host"], "--policy_delay needs --rng device"),
    (["--policy_delay", "2", "--fed_method", "interfrl", "--engine", "fused3"], "--policy_delay needs --rng device"),
    ([*FUSED3, "--policy_delay", "2", "--episodes", "platoon", "--seeds", "1,2", "--sweep", "actor_lr=1e-4,1e-3"],
     "--policy_delay does not combine with --sweep / --pbt"),
    ([*FUSED3, "--policy_delay", "2", "--episodes", "platoon", "--seeds", "1,2", "--sweep", "actor_lr=1e-4,1e-3", "--pbt", "100"],
     "--policy_delay does not combine with --sweep / --pbt"),
    ([*FUSED3, "--policy_delay", "0"], "--policy_delay: policy delay: policy_delay=0 must be >= 1"),
    ([*FUSED3, "--policy_delay", "-3"], "--policy_delay: policy delay: policy_delay=-3 must be >= 1"),
    ([*FUSED3, "--policy_delay", "2.5"], "--policy_delay: policy delay: D='2.5' must be a whole number >= 1"),
    ([*FUSED3, "--policy_delay", "two"], "--policy_delay: policy delay: D='two' must be a whole number >= 1"),
    ([*FUSED3, "--policy_delay", "100", "--total_time_steps", "100"], "--policy_delay: policy delay: policy_delay=100 is not below the run's 100 steps"),
    ([*FUSED3, "--policy_delay", "500", "--total_time_steps", "100"], "is not below the run's 100 steps"),
    ([*FUSED3, "--policy_delay", "50", "--total_time_steps", "100"],
     "--policy_delay: policy delay: policy_delay=50 is above the 36 learner calls that 100 steps make past the replay gate"),
    (["--rng", "device", "--engine", "fused3", "--policy_delay", "2"], "--policy_delay: policy delay needs shared weight sets"),
    (["--rng", "device", "--engine", "fused3", "--fed_method", "intrafrl", "--policy_delay", "2"],
     "--policy_delay: policy delay needs shared weight sets"),
])
def test_cli_argument_errors(argv, msg, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        cli.get_cmdl_args(["tr", *argv], config.Config())
    assert e.value.code == 2 and msg in capsys.readouterr().err


def test_cli_refuses_more_than_one_rank_and_the_centralized_framework_and_composes(capsys, monkeypatch, tmp_path):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cli.get_cmdl_args(["tr", *FUSED3, "--policy_delay", "2"], config.Config())
    assert "--policy_delay is not available under a process group of more than one rank" in capsys.readouterr().err
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(SystemExit):
        cli.get_cmdl_args(["tr", *FUSED3, "--policy_delay", "2"], config.Config(framework="centralized"))
    assert "policy delay needs the decentralized framework" in capsys.readouterr().err
    args, conf = cli.get_cmdl_args(["tr", *FUSED3, "--policy_delay", "3", "--target_noise", "sigma=0.2,clip=0.4", "--anchor", "kp=2,kv=1,weight=10",
                                    "--warm_start", "kp=2,kv=1", "--actor_hold", "10", "--total_time_steps", "100"], config.Config())
    assert args.policy_delay == 3 and isinstance(args.policy_delay, int)
    assert cli._delay_kw(args) == dict(policy_delay=3) and cli._noise_kw(args) == dict(target_noise=TargetNoise(0.2, 0.4))
    # conf.json's field: an int beside the others, read back by json and ignored by the loader esim uses
    cli._record_noise(conf, args)
    cli._record_delay(conf, args)
    assert conf.policy_delay == 3 and conf.target_noise == [["sigma", 0.2], ["clip", 0.4]]
    path = tmp_path / "conf.json"
    artifacts.config_writer(str(path), conf)
    assert json.load(open(path))["policy_delay"] == 3
    loaded = artifacts.config_loader(str(path), config.Config)
    assert not hasattr(loaded, "policy_delay") and loaded.fed_method == conf.fed_method
    args, conf = cli.get_cmdl_args(["tr", *FUSED3, "--policy_delay", "2", "--residual", "kp=2,kv=1", "--episodes", "platoon", "--seeds", "1,2"],
                                   config.Config())
    assert args.policy_delay == 2 and args.residual.kp == 2 and cli._delay_kw(args) == dict(policy_delay=2) and cli._noise_kw(args) == {}
    # without the flag: nothing is handed to the trainer, nothing recorded
    args, conf = cli.get_cmdl_args(["tr", *FUSED3], config.Config())
    assert args.policy_delay is None and cli._delay_kw(args) == {}
    cli._record_delay(conf, args)
    assert not hasattr(conf, "policy_delay")


# ---- the entry points' host checks (no GPU here: a call that got past its checks would fail with a HIP error instead) ----

_BOGUS = 0x1000


def _update(lay, n_sets=3, policy=0, actor_lr=1e-4, critic_lr=1e-3, tau=0.005, skipped=True, **null):
    names = ("theta", "stats", "theta_t", "stats_t", "m", "v", "grads", "step", "actor_step")
    p = [None if k in null else ctypes.c_void_p(_BOGUS * (i + 1)) for i, k in enumerate(names)]
    _hip.call("avd_adam_polyak_delayed_f32", None if lay is None else ctypes.byref(lay), n_sets, *p, policy, actor_lr, critic_lr, tau,
              ctypes.c_void_p(_BOGUS * 20) if skipped else None, None)


@pytest.mark.parametrize("policy", [0, 1])
def test_update_entry_point_refuses_on_the_host_before_any_launch(policy):
    who = "avd_adam_polyak_delayed_f32"
    ref = _hip.make_layout(4, 1, 256, 128, 48, 64)
    refuse = lambda msg: pytest.raises(_hip.AvdError, match=rf"failed \(-1\): {who}: {msg}")
    with refuse("n_sets=3"):  # (a null layout)
        _update(None, policy=policy)
    for n in (0, -2, 65536):
        with refuse(f"n_sets={n}"):
            _update(ref, n_sets=n, policy=policy)
    for name in ("theta", "stats", "theta_t", "stats_t", "m", "v", "grads", "step", "actor_step"):
        with refuse("null pointer"):
            _update(ref, policy=policy, **{name: 1})
    odd = _hip.make_layout(4, 1, 256, 128, 48, 64)
    odd.actor_size += 2
    with refuse("layout not 4-float aligned"):
        _update(odd, policy=policy)
    none = _hip.make_layout(4, 1, 256, 128, 48, 64)
    none.actor_size = none.theta_size
    with refuse("layout without an actor or a critic block"):
        _update(none, policy=policy)
    for kw in (dict(actor_lr=-1e-4), dict(critic_lr=-1e-3), dict(actor_lr=math.inf), dict(critic_lr=math.nan), dict(actor_lr=math.nan)):
        with refuse(r"actor_lr=\S+ critic_lr=\S+ \(must be finite and >= 0\)"):
            _update(ref, policy=policy, **kw)
    for tau in (0.0, -0.005, 1.5, math.nan, math.inf):
        with refuse(r"tau=\S+ \(must be in \(0, 1\]\)"):
            _update(ref, policy=policy, tau=tau)


def _td(lay, n_agents=12, n_sets=6, M=3, E=1, lo=-2.5, hi=2.5, sigma=0.2, clip=0.5, seeds=None, ws=_BOGUS * 16, **null):
    names = ("theta", "stats", "theta_t", "stats_t", "s", "a", "r", "s2", "grads", "losses")
    p = {k: (None if k in null else ctypes.c_void_p(_BOGUS * (i + 1))) for i, k in enumerate(names)}
    _hip.call("avd_learn_set_split_td_f16x3", None if lay is None else ctypes.byref(lay), n_agents, n_sets, p["theta"], p["stats"], p["theta_t"],
              p["stats_t"], p["s"], p["a"], p["r"], p["s2"], None, 0.99, 2.5, p["grads"], p["losses"], None if ws is None else ctypes.c_void_p(ws),
              0, sigma, clip, lo, hi, 1, 0, None if seeds is None else ctypes.c_void_p(seeds), E, M, None)


def test_td_entry_point_refuses_on_the_host_before_any_hip_call():
    """avd_learn_set_split_critic's refusals and check_smooth's, one fault per call; what passes them all gets as far as the workspace
    size, the last host check."""
    who = "avd_learn_set_split_td_f16x3"
    ref = _hip.make_layout(4, 1, 256, 128, 48, 64)
    refuse = lambda code, msg: pytest.raises(_hip.AvdError, match=rf"failed \({code}\): {who}: {msg}")
    size = r"workspace 0 B < \d+ B"
    with refuse(-1, "null layout"):
        _td(None)
    with refuse(-3, "serves the reference widths only"):
        _td(_hip.make_layout(4, 1, 320, 160, 48, 64))
    for kw, msg in ((dict(n_agents=13), "n_agents=13 n_sets=6"), (dict(n_agents=0), "n_agents=0 n_sets=6"),
                    (dict(n_agents=130, n_sets=65, M=1), "n_agents=130 n_sets=65"),
                    (dict(M=0), "M=0 E=1"), (dict(E=0), "M=3 E=0"), (dict(E=-1), "M=3 E=-1"),
                    (dict(M=4), r"n_sets=6 M=4 E=1 \(n_sets must be a multiple of E x M\)"), (dict(E=4, seeds=_BOGUS), "n_sets=6 M=3 E=4"),
                    (dict(E=2), "E=2 without a seed table"), (dict(sigma=-0.1), r"sigma=-0.1 \(must be finite and >= 0\)"),
                    (dict(sigma=float("inf")), "sigma=inf"), (dict(sigma=float("nan")), "sigma=-?nan"), (dict(clip=0.0), r"noise_clip=0 \(must be > 0"),
                    (dict(clip=-0.5), "noise_clip=-0.5"), (dict(clip=float("nan")), "noise_clip=-?nan"), (dict(lo=1.0, hi=-1.0), "lo=1 > hi=-1"),
                    (dict(ws=_BOGUS + 8), "the workspace must be 16-byte aligned"),
                    (dict(theta=1), "null pointer"), (dict(theta_t=1), "null pointer"), (dict(stats_t=1), "null pointer"), (dict(a=1), "null pointer"),
                    (dict(r=1), "null pointer"), (dict(s2=1), "null pointer"), (dict(grads=1), "null pointer"), (dict(ws=None), "null pointer"),
                    # accepted as far as the workspace size: sigma 0 (no launch), no noise clip, a seed table, null losses
                    (dict(), size), (dict(sigma=0.0), size), (dict(clip=float("inf")), size), (dict(E=2, seeds=_BOGUS), size),
                    (dict(M=1, E=6, seeds=_BOGUS), size), (dict(losses=1), size)):
        with refuse(-1, msg):
            _td(ref, **kw)
    assert _hip._PROTOS[who][:18] == _hip._PROTOS["avd_learn_set_split_critic"][:18]  # the critic phase's arguments first
