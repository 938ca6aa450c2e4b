"""Target policy smoothing without a device (tr --target_noise, trainer.TargetNoise, the host checks of avd_target_smooth_f32 and
avd_learn_set_split_smooth_f16x3, tests/smooth_oracle.py): TargetNoise's defaults and parsing, every refusal of check_target_noise, of
the CLI and of the two entry points, and the oracle's own properties -- the index mapping against a hand-written table, a seed batch's
experiment equal to its solo draw, oracle.mlp.learn at zero noise, only the critic's side depending on the noise."""
import ctypes
import math

import numpy as np
import pytest

from avddpg_amd import __main__ as cli
from avddpg_amd import _hip, config, trainer
from avddpg_amd.trainer import TargetNoise
from oracle import mlp as omlp
from oracle import philox
from tests import smooth_oracle

FUSED3 = ["--fed_method", "interfrl", "--engine", "fused3", "--rng", "device"]


def _interfrl(**kw):
    return config.Config(fed_method="interfrl", **kw)


def test_target_noise_defaults_and_parsing():
    tn = TargetNoise()
    assert (tn.sigma, tn.clip) == (0.2, 0.5)  # TD3's pair
    assert TargetNoise(0.4).clip == 1.0 and TargetNoise(sigma=1.5).clip == 3.75
    assert TargetNoise(0.2, 0.3).clip == 0.3 and TargetNoise(0.2, clip=math.inf).clip == math.inf
    assert TargetNoise(0.0).clip > 0  # sigma 0: the launch is skipped, any positive clip does
    assert TargetNoise(0.2) == TargetNoise(0.2, 0.5) and hash(TargetNoise(0.2)) == hash(TargetNoise(0.2, 0.5))
    assert TargetNoise(0.2) != TargetNoise(0.2, 0.4)
    with pytest.raises(AttributeError, match="frozen"):
        tn.sigma = 1.0
    with pytest.raises(AttributeError, match="frozen"):
        del tn.clip
    assert tn.record() == [["sigma", 0.2], ["clip", 0.5]]
    assert TargetNoise.parse("sigma=0.2") == TargetNoise(0.2, 0.5)
    assert TargetNoise.parse(" sigma=0.3 , clip=0.5 ") == TargetNoise(0.3, 0.5)
    assert TargetNoise.parse("clip=inf,sigma=1") == TargetNoise(1.0, math.inf)
    assert repr(TargetNoise(0.2)) == "TargetNoise(sigma=0.2, clip=0.5)"


@pytest.mark.parametrize("text,msg", [("", "no sigma given"), ("clip=0.5", "no sigma given"), ("sigma=0.2,sigma=0.3", "sigma given twice"),
                                      ("sigma=0.2,clip=1,clip=2", "clip given twice"), ("sigma=0.2,decay=3", "unknown key 'decay'"),
                                      ("0.2", "unknown key '0.2'"), ("sigma=abc", "sigma='abc' is not a number"),
                                      ("sigma=0.2,clip=", "clip='' is not a number")])
def test_parse_refusals(text, msg):
    with pytest.raises(ValueError, match=msg):
        TargetNoise.parse(text)


def test_check_target_noise_refusals():
    ok, tn = _interfrl(), TargetNoise(0.2)
    assert trainer.check_target_noise(tn, ok, "fused3") is tn
    assert trainer.check_target_noise(tn) is tn  # the values alone
    assert trainer.check_target_noise(TargetNoise(0.0), ok, "fused3").sigma == 0.0
    assert trainer.check_target_noise(TargetNoise(0.2, math.inf), ok, "fused3").clip == math.inf
    with pytest.raises(ValueError, match="is not a trainer.TargetNoise"):
        trainer.check_target_noise(0.2, ok, "fused3")
    for sigma in (-0.1, math.inf, -math.inf, math.nan, "0.2", True, 1e39):
        with pytest.raises(ValueError, match="target noise: sigma="):
            trainer.check_target_noise(TargetNoise(sigma, 0.5), ok, "fused3")
    for clip in (0.0, -0.5, math.nan, -math.inf, "0.5", False, 1e-50):
        with pytest.raises(ValueError, match="target noise: clip="):
            trainer.check_target_noise(TargetNoise(0.2, clip), ok, "fused3")
    for engine in (None, "per_agent", "batched", "fused"):
        with pytest.raises(ValueError, match="target noise needs shared_engine='fused3'"):
            trainer.check_target_noise(tn, ok, engine)
    with pytest.raises(ValueError, match="target noise needs rng='device'"):
        trainer.check_target_noise(tn, ok, "fused3", rng="host")
    with pytest.raises(ValueError, match="hyperparameter sweep or PBT"):
        trainer.check_target_noise(tn, ok, "fused3", hparams=[{}])
    with pytest.raises(ValueError, match="overlap_allreduce"):
        trainer.check_target_noise(tn, ok, "fused3", overlap_allreduce=True)
    with pytest.raises(ValueError, match="target noise runs on one rank"):
        trainer.check_target_noise(tn, ok, "fused3", world_size=2)
    with pytest.raises(ValueError, match="target noise needs the decentralized framework"):
        trainer.check_target_noise(tn, _interfrl(framework="centralized"), "fused3")
    with pytest.raises(ValueError, match="target noise needs shared weight sets"):
        trainer.check_target_noise(tn, config.Config(fed_method="intrafrl"), "fused3")
    with pytest.raises(ValueError, match="target noise needs shared weight sets"):
        trainer.check_target_noise(tn, config.Config(), "fused3")  # no federation
    with pytest.raises(ValueError, match="target noise needs shared weight sets"):
        trainer.check_target_noise(tn, ok, "fused3", shared_sets=False)


def test_the_trainer_refuses_before_anything_is_allocated(monkeypatch):
    """VecTrainer(target_noise=...) raises from its first lines: no environment, no agents, no library call."""
    from avddpg_amd import vec

    def boom(*a, **k):
        raise AssertionError("something was allocated")

    for name in ("VecPlatoon", "AgentGroup", "VecReplay", "VecOUNoise"):
        monkeypatch.setattr(vec, name, boom)
    tn = TargetNoise(0.2)
    for kw, msg in ((dict(shared_engine="fused"), "needs shared_engine='fused3'"), (dict(shared_engine="fused3", rng="host"), "needs rng='device'"),
                    (dict(shared_engine="fused3", overlap_allreduce=True), "overlap_allreduce"),
                    (dict(shared_engine="fused3", seeds=(1, 2), hparams=[{}, {}]), "hyperparameter sweep or PBT"),
                    (dict(shared_engine="fused3", target_noise=TargetNoise(-1.0)), "sigma=-1.0")):
        with pytest.raises(ValueError, match=msg):
            trainer.VecTrainer(_interfrl(), **{**dict(rng="device", target_noise=tn), **kw})
    with pytest.raises(ValueError, match="needs the decentralized framework"):
        trainer.VecTrainer(_interfrl(framework="centralized"), rng="device", shared_engine="fused3", target_noise=tn)


@pytest.mark.parametrize("argv,msg", [
    (["--target_noise", "sigma=0.2", "--rng", "device", "--fed_method", "interfrl"], "--target_noise needs --engine fused3"),
    (["--target_noise", "sigma=0.2", "--rng", "device", "--fed_method", "interfrl", "--engine", "per_agent"], "--target_noise needs --engine fused3"),
    (["--target_noise", "sigma=0.2", "--rng", "device", "--fed_method", "interfrl", "--engine", "batched"], "--target_noise needs --engine fused3"),
    (["--target_noise", "sigma=0.2", "--rng", "device", "--fed_method", "interfrl", "--engine", "fused"], "--target_noise needs --engine fused3"),
    (["--target_noise", "sigma=0.2", "--fed_method", "interfrl", "--engine", "fused3", "--rng", "host"], "--target_noise needs --rng device"),
    (["--target_noise", "sigma=0.2", "--fed_method", "interfrl", "--engine", "fused3"], "--target_noise needs --rng device"),
    ([*FUSED3, "--target_noise", "sigma=0.2", "--episodes", "platoon", "--seeds", "1,2", "--sweep", "actor_lr=1e-4,1e-3"],
     "--target_noise does not combine with --sweep / --pbt"),
    ([*FUSED3, "--target_noise", "sigma=0.2", "--episodes", "platoon", "--seeds", "1,2", "--sweep", "actor_lr=1e-4,1e-3", "--pbt", "100"],
     "--target_noise does not combine with --sweep / --pbt"),
    ([*FUSED3, "--target_noise", "sigma=-0.2"], "--target_noise: target noise: sigma=-0.2 must be a finite number >= 0"),
    ([*FUSED3, "--target_noise", "sigma=inf"], "--target_noise: target noise: sigma=inf must be a finite number >= 0"),
    ([*FUSED3, "--target_noise", "sigma=nan"], "--target_noise: target noise: sigma=nan must be a finite number >= 0"),
    ([*FUSED3, "--target_noise", "sigma=0.2,clip=0"], "--target_noise: target noise: clip=0.0 must be a number > 0"),
    ([*FUSED3, "--target_noise", "sigma=0.2,clip=-1"], "--target_noise: target noise: clip=-1.0 must be a number > 0"),
    ([*FUSED3, "--target_noise", "sigma=0.2,clip=nan"], "--target_noise: target noise: clip=nan must be a number > 0"),
    ([*FUSED3, "--target_noise", "sigma=0.2,weight=3"], "--target_noise: target noise: unknown key 'weight'"),
    ([*FUSED3, "--target_noise", "sigma=0.2,sigma=0.3"], "--target_noise: target noise: sigma given twice"),
    ([*FUSED3, "--target_noise", "clip=0.3"], "no sigma given"),
    (["--rng", "device", "--engine", "fused3", "--target_noise", "sigma=0.2"], "--target_noise: target noise needs shared weight sets"),
    (["--rng", "device", "--engine", "fused3", "--fed_method", "intrafrl", "--target_noise", "sigma=0.2"],
     "--target_noise: target noise needs shared weight sets"),
])
def test_cli_argument_errors(argv, msg, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        cli.get_cmdl_args(["tr", *argv], config.Config())
    assert e.value.code == 2 and msg in capsys.readouterr().err


def test_cli_refuses_more_than_one_rank_and_the_centralized_framework_and_composes(capsys, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cli.get_cmdl_args(["tr", *FUSED3, "--target_noise", "sigma=0.2"], config.Config())
    assert "--target_noise is not available under a process group of more than one rank" in capsys.readouterr().err
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(SystemExit):
        cli.get_cmdl_args(["tr", *FUSED3, "--target_noise", "sigma=0.2"], config.Config(framework="centralized"))
    assert "target noise needs the decentralized framework" in capsys.readouterr().err
    args, conf = cli.get_cmdl_args(["tr", *FUSED3, "--target_noise", "sigma=0.2,clip=0.4", "--anchor", "kp=2,kv=1,weight=10", "--warm_start",
                                    "kp=2,kv=1", "--actor_hold", "10", "--total_time_steps", "100"], config.Config())
    assert args.target_noise == TargetNoise(0.2, 0.4) and cli._noise_kw(args) == dict(target_noise=args.target_noise)
    assert cli._anchor_kw(args) == dict(anchor=args.anchor)
    cli._record_noise(conf, args)
    assert conf.target_noise == [["sigma", 0.2], ["clip", 0.4]]
    args, conf = cli.get_cmdl_args(["tr", *FUSED3, "--target_noise", "sigma=0.2", "--residual", "kp=2,kv=1"], config.Config())
    assert args.target_noise.clip == 0.5 and args.residual.kp == 2
    # without the flag: nothing is handed to the trainer, nothing recorded
    args, conf = cli.get_cmdl_args(["tr", *FUSED3], config.Config())
    assert args.target_noise is None and cli._noise_kw(args) == {}
    cli._record_noise(conf, args)
    assert not hasattr(conf, "target_noise")


# ---- the entry points' host checks (no GPU here: a call that got past its checks would fail with a HIP error instead) ----

_BOGUS = 0x1000


def test_target_smooth_refuses_on_the_host_before_any_hip_call():
    who = "avd_target_smooth_f32"
    refuse = lambda msg: pytest.raises(_hip.AvdError, match=rf"failed \(-1\): {who}: {msg}")

    def go(n_agents=12, M=3, E=1, a2=_BOGUS, sigma=0.2, clip=0.5, lo=-2.5, hi=2.5, seeds=None):
        _hip.call(who, n_agents, M, E, None if a2 is None else ctypes.c_void_p(a2), sigma, clip, lo, hi, 1, 0,
                  None if seeds is None else ctypes.c_void_p(seeds), None)

    for kw, msg in ((dict(a2=None), "null a2"), (dict(a2=_BOGUS + 4), "a2 must be 16-byte aligned"), (dict(n_agents=0), "n_agents=0"),
                    (dict(n_agents=-3), "n_agents=-3"), (dict(n_agents=(1 << 24) + 1), "n_agents=16777217"), (dict(M=0), "M=0 E=1"),
                    (dict(M=-1), "M=-1 E=1"), (dict(E=0), "M=3 E=0"), (dict(M=5), r"n_agents=12 M=5 E=1 \(n_agents must be a multiple of E x M\)"),
                    (dict(E=5, seeds=_BOGUS), "n_agents=12 M=3 E=5"), (dict(E=2), "E=2 without a seed table"),
                    (dict(sigma=-0.1), r"sigma=-0.1 \(must be finite and >= 0\)"), (dict(sigma=float("inf")), "sigma=inf"),
                    (dict(sigma=float("nan")), "sigma=-?nan"), (dict(clip=0.0), r"noise_clip=0 \(must be > 0"),
                    (dict(clip=-0.5), "noise_clip=-0.5"), (dict(clip=float("nan")), "noise_clip=-?nan"),
                    (dict(clip=float("-inf")), "noise_clip=-inf"), (dict(lo=1.0, hi=-1.0), "lo=1 > hi=-1")):
        with refuse(msg):
            go(**kw)


def _entry(lay, n_agents=12, n_sets=6, M=3, E=1, lo=-2.5, hi=2.5, weight=1.0, sigma=0.2, clip=0.5, seeds=None, ws=_BOGUS * 16, **null):
    """avd_learn_set_split_smooth_f16x3 with non-null pointers nothing reads, everywhere but where `null` names an argument."""
    names = ("theta", "stats", "theta_t", "stats_t", "s", "a", "r", "s2", "grads", "losses", "gains", "anchor_loss")
    p = {k: (None if k in null else ctypes.c_void_p(_BOGUS * (i + 1))) for i, k in enumerate(names)}
    _hip.call("avd_learn_set_split_smooth_f16x3", None if lay is None else ctypes.byref(lay), n_agents, n_sets, p["theta"], p["stats"],
              p["theta_t"], p["stats_t"], p["s"], p["a"], p["r"], p["s2"], None, 0.99, 2.5, p["grads"], p["losses"],
              None if ws is None else ctypes.c_void_p(ws), 0, p["gains"], M, 0, lo, hi, weight, p["anchor_loss"], sigma, clip, 1, 0,
              None if seeds is None else ctypes.c_void_p(seeds), E, None)


def test_learner_entry_point_refuses_on_the_host_before_any_hip_call():
    """One fault per call, with status and text; the cases that pass every check of the smoothing and the anchor get as far as the
    workspace size, the last host check."""
    who = "avd_learn_set_split_smooth_f16x3"
    ref = _hip.make_layout(4, 1, 256, 128, 48, 64)
    refuse = lambda code, msg: pytest.raises(_hip.AvdError, match=rf"failed \({code}\): {who}: {msg}")
    size = r"workspace 0 B < \d+ B"
    with refuse(-1, "null layout"):
        _entry(None)
    with refuse(-3, "serves the reference widths only"):
        _entry(_hip.make_layout(4, 1, 320, 160, 48, 64))
    for kw, msg in ((dict(n_agents=13), "n_agents=13 n_sets=6"), (dict(n_agents=0), "n_agents=0 n_sets=6"),
                    (dict(n_agents=130, n_sets=65, M=1), "n_agents=130 n_sets=65"),
                    # the anchor's, with gains
                    (dict(anchor_loss=1), "null gains / anchor_loss"), (dict(M=4), "n_sets=6 M=4"), (dict(M=0), "n_sets=6 M=0"),
                    (dict(weight=-1e-3), r"weight=-0.001 \(must be finite and >= 0\)"), (dict(weight=float("nan")), "weight=-?nan"),
                    (dict(lo=1.0, hi=-1.0), "lo=1 > hi=-1"),
                    # the smoothing's own, without gains and with
                    (dict(gains=1, M=0), "M=0 E=1"), (dict(gains=1, E=0), "M=3 E=0"), (dict(E=-1), "M=3 E=-1"),
                    (dict(gains=1, M=4), r"n_sets=6 M=4 E=1 \(n_sets must be a multiple of E x M\)"),
                    (dict(E=4, seeds=_BOGUS), "n_sets=6 M=3 E=4"), (dict(E=2), "E=2 without a seed table"),
                    (dict(gains=1, E=2), "E=2 without a seed table"), (dict(sigma=-0.1), r"sigma=-0.1 \(must be finite and >= 0\)"),
                    (dict(sigma=float("inf")), "sigma=inf"), (dict(gains=1, sigma=float("nan")), "sigma=-?nan"),
                    (dict(clip=0.0), r"noise_clip=0 \(must be > 0"), (dict(clip=-0.5), "noise_clip=-0.5"),
                    (dict(gains=1, clip=float("nan")), "noise_clip=-?nan"), (dict(gains=1, lo=1.0, hi=-1.0), "lo=1 > hi=-1"),
                    (dict(ws=_BOGUS + 8), "the workspace must be 16-byte aligned"),
                    (dict(theta=1), "null pointer"), (dict(s2=1), "null pointer"), (dict(grads=1), "null pointer"), (dict(ws=None), "null pointer"),
                    # accepted as far as the workspace size: no anchor (anchor_loss may be null, weight unread), sigma 0, no noise clip, a table
                    (dict(), size), (dict(gains=1, anchor_loss=1, weight=float("nan")), size), (dict(sigma=0.0), size), (dict(sigma=-0.0), size),
                    (dict(clip=float("inf")), size), (dict(E=2, seeds=_BOGUS), size), (dict(M=1, E=6, seeds=_BOGUS, gains=1), size),
                    (dict(lo=2.5, hi=2.5), size)):
        with refuse(-1, msg):
            _entry(ref, **kw)
    assert _hip._PROTOS[who][:25] == _hip._PROTOS["avd_learn_set_split_anchor_f16x3"][:25]  # the anchored call's arguments first


# ---- the oracle's own properties ----

def test_the_index_mapping_against_a_hand_written_table():
    """E = 2 experiments of M = 3 vehicles, P = 2 platoons: agent v = (p E + e) M + m, solo index p M + m."""
    table = [  # v: (e, p, m, vs)
        (0, 0, 0, 0), (0, 0, 1, 1), (0, 0, 2, 2), (1, 0, 0, 0), (1, 0, 1, 1), (1, 0, 2, 2),
        (0, 1, 0, 3), (0, 1, 1, 4), (0, 1, 2, 5), (1, 1, 0, 3), (1, 1, 1, 4), (1, 1, 2, 5)]
    e, p, m, vs = smooth_oracle.keys(12, 3, 2)
    assert [tuple(int(x) for x in row) for row in zip(e, p, m, vs)] == table
    assert smooth_oracle.STREAM_SMOOTH == 12 and smooth_oracle.STREAM_SMOOTH not in (
        philox.STREAM_RESET_A, philox.STREAM_RESET_B, philox.STREAM_OU, philox.STREAM_NORMAL, philox.STREAM_REPLAY)
    # the row layout: thread q's block gives rows 4q .. 4q + 3, straight from oracle.philox
    n = smooth_oracle.normals(12, 3, 2, counter=7, seeds=(11, 22))
    w = philox.philox_at(22, 7, np.array([4 * 16 + 5]), 12)  # agent 10 = (e 1, p 1, m 1): vs 4, thread 5
    n0, n1 = philox.box_muller(w[0], w[1])
    n2, n3 = philox.box_muller(w[2], w[3])
    assert np.array_equal(n[10, 20:24], np.array([n0[0], n1[0], n2[0], n3[0]], np.float32))


def test_a_seed_batch_experiment_draws_what_its_solo_run_draws():
    E, M, P = 2, 3, 4
    seeds = (5, 9)
    big = smooth_oracle.noise(P * E * M, M, E, 0.2, 0.5, counter=3, seeds=seeds)
    e, _, _, _ = smooth_oracle.keys(P * E * M, M, E)
    for k, key in enumerate(seeds):
        solo = smooth_oracle.noise(P * M, M, 1, 0.2, 0.5, counter=3, seed=key)
        assert np.array_equal(big[e == k], solo), k
    assert not np.array_equal(big[e == 0], big[e == 1])
    assert not np.array_equal(big, smooth_oracle.noise(P * E * M, M, E, 0.2, 0.5, counter=4, seeds=seeds))
    assert np.abs(big).max() == np.float32(0.5)  # the clip binds somewhere in 1536 draws at 2.5 sigma, exactly
    wide = smooth_oracle.noise(P * E * M, M, E, 0.2, math.inf, counter=3, seeds=seeds)
    assert np.abs(wide).max() > 0.5 and np.array_equal(np.clip(wide, -0.5, 0.5), big)


def _small_nets(rs, S=4, dtype=np.float64):
    """The four weight lists at the reference widths, Keras order, with moving statistics away from (0, 1)."""
    def actor():
        w = []
        for i, o in ((S, 256), (256, 128)):
            w += [rs.randn(i, o) / np.sqrt(i), 0.1 * rs.randn(o), 1 + 0.1 * rs.randn(o), 0.1 * rs.randn(o), 0.1 * rs.randn(o), 0.5 + rs.rand(o)]
        return [x.astype(dtype) for x in w + [0.1 * rs.randn(128, 1), 0.1 * rs.randn(1)]]

    def critic():
        w = [rs.randn(S, 256) / np.sqrt(S), 0.1 * rs.randn(256), rs.randn(1, 48), 0.1 * rs.randn(48)]
        for o in (256, 48):
            w += [1 + 0.1 * rs.randn(o), 0.1 * rs.randn(o), 0.1 * rs.randn(o), 0.5 + rs.rand(o)]
        w += [rs.randn(304, 128) / np.sqrt(304), 0.1 * rs.randn(128), 1 + 0.1 * rs.randn(128), 0.1 * rs.randn(128), 0.1 * rs.randn(128),
              0.5 + rs.rand(128), 0.1 * rs.randn(128, 1), 0.1 * rs.randn(1)]
        return [x.astype(dtype) for x in w]

    return [actor(), critic(), actor(), critic()]


def test_the_oracle_is_learn_at_zero_noise_and_only_the_critic_side_sees_the_noise():
    rs = np.random.RandomState(3)
    P, S = 3, 4
    nets = _small_nets(rs)
    s, a, r, s2 = rs.randn(P, 64, S), rs.uniform(-2.5, 2.5, (P, 64, 1)), -rs.rand(P, 64), rs.randn(P, 64, S)
    rows = lambda x: x.reshape(P * 64, *x.shape[2:])
    cg0, ag0, aux0 = omlp.learn((rows(s), rows(a), rows(r)[:, None], rows(s2)), *nets)
    zero = smooth_oracle.parts((s, a, r, s2), nets, np.zeros((P, 64), np.float32), -2.5, 2.5)
    for x, y in zip(zero["cg"] + zero["ag"], list(cg0) + list(ag0)):
        assert np.allclose(x, y, rtol=0, atol=1e-6 * np.abs(y).max())  # (ta passes through float32 once: 6e-8 of it)
    assert abs(zero["critic_loss"] - aux0["critic_loss"]) <= 1e-6 * aux0["critic_loss"] and zero["action_clipped"] == 0.0
    eps = smooth_oracle.noise(P, 1, 1, 1.5, 3.75, counter=0, seed=1)
    noisy = smooth_oracle.parts((s, a, r, s2), nets, eps, -2.5, 2.5)
    for x, y in zip(noisy["ag"], zero["ag"]):
        assert np.array_equal(x, y)  # the actor's gradients do not depend on y
    assert noisy["actor_loss"] == zero["actor_loss"]
    assert any(not np.allclose(x, y, rtol=1e-3, atol=0) for x, y in zip(noisy["cg"], zero["cg"]))
    assert noisy["critic_loss"] != zero["critic_loss"]
    # agent weights all 1: the weighted sum of per-agent terms is the concatenated batch's
    ones = smooth_oracle.parts((s, a, r, s2), nets, eps, -2.5, 2.5, agent_weight=np.ones(P))
    for x, y in zip(ones["cg"] + ones["ag"], noisy["cg"] + noisy["ag"]):
        assert np.allclose(x, y, rtol=0, atol=1e-12 * max(1.0, np.abs(y).max()))
    # with a gain row the anchor's summand comes on top, through anchor_oracle.combine
    both = smooth_oracle.parts((s, a, r, s2), nets, eps, -2.5, 2.5, gain_row=[2.0, 1.0, -0.3, 0.4])
    cg, ag = smooth_oracle.combine(both, 10.0)
    assert all(np.array_equal(x, y) for x, y in zip(cg, noisy["cg"])) and both["anchor_loss"] > 0
    assert all(np.allclose(x, y + 10.0 * b, rtol=0, atol=1e-12 * max(1.0, np.abs(x).max())) for x, y, b in zip(ag, noisy["ag"], both["bc"]))
