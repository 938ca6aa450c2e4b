"""Warm start (tr --warm_start / --actor_hold), what needs no GPU: the flag text and every refusal, the conf.json record's round trip,
the test oracles of the two new entry points (tests/clone_oracle.py) against independent restatements, the entry points' host-side
argument checks, and a float64 oracle fit under the conditions the end-to-end GPU test puts on its reference."""
import ctypes
import re

import numpy as np
import pytest

from avddpg_amd import __main__ as cli
from avddpg_amd import _hip, config, scenarios, trainer
from oracle import mlp as omlp
from oracle import philox
from tests import clone_oracle


def test_parse_defaults_and_every_key():
    w = scenarios.parse_warm_start("kp=2,kv=1")
    assert isinstance(w, scenarios.WarmStart) and isinstance(w, scenarios.LinearLaw)
    assert (w.kp, w.kv, w.ka, w.kf, w.steps, w.lr, w.ep, w.ev, w.a, w.source) == (2.0, 1.0, 0, 0, 2000, 1e-3, None, None, None, "given")
    conf = config.Config()
    assert np.array_equal(w.box(conf), np.array([conf.reset_ep_max, conf.reset_max_ev, 1.0, 1.0], np.float32))
    w = scenarios.parse_warm_start(" kp=1.5, kv=0.5,ka=-0.1,kf=0.3,steps=300,lr=2e-3,ep=2,ev=3,a=0.5 ")
    assert (w.kp, w.kv, w.ka, w.kf, w.steps, w.lr, w.ep, w.ev, w.a) == (1.5, 0.5, -0.1, 0.3, 300, 2e-3, 2.0, 3.0, 0.5)
    assert isinstance(w.steps, int)
    assert np.array_equal(w.box(conf), np.array([2, 3, 0.5, 0.5], np.float32))  # a bounds a_pred too
    assert scenarios.check_warm_start(w, conf) is w
    assert scenarios.parse_warm_start("tuned") == scenarios.TUNED and scenarios.parse_warm_start(" searched ") == scenarios.SEARCHED
    assert np.array_equal(w.gains(3), np.tile(np.array([1.5, 0.5, -0.1, 0.3], np.float32), (3, 1)))


@pytest.mark.parametrize("text,msg", [
    ("", "no gain given"),
    ("kp=2,kq=1", "unknown key 'kq'"),
    ("kp=2,scale=0.5", "unknown key 'scale'"),
    ("kp", "unknown key 'kp'"),
    ("kp=2,kp=3", "kp given twice"),
    ("kp=2,steps=10,steps=20", "steps given twice"),
    ("kp=two", "kp='two' is not a number"),
    ("kp=2,steps=1.5", "steps=1.5 is not a whole number"),
    ("kp=2,steps=nan", "is not a whole number"),
])
def test_parse_refusals(text, msg):
    with pytest.raises(ValueError, match=re.escape(msg)):
        scenarios.parse_warm_start(text)


@pytest.mark.parametrize("kw,msg", [
    (dict(kp=float("nan")), "kp=nan must be a finite number"),
    (dict(kp=2, kv=float("inf")), "kv=inf must be a finite number"),
    (dict(kp=2, steps=0), "steps=0 must be a whole number in 1 .. 100000"),
    (dict(kp=2, steps=100001), "steps=100001 must be a whole number in 1 .. 100000"),
    (dict(kp=2, steps=2.0), "steps=2.0 must be a whole number"),
    (dict(kp=2, lr=0.0), "lr=0.0 must be a finite number > 0"),
    (dict(kp=2, lr=-1e-3), "lr=-0.001 must be a finite number > 0"),
    (dict(kp=2, lr=float("inf")), "lr=inf must be a finite number > 0"),
    (dict(kp=2, ep=0.0), "ep=0.0 must be a finite number > 0"),
    (dict(kp=2, ev=-1.0), "ev=-1.0 must be a finite number > 0"),
    (dict(kp=2, a=float("nan")), "a=nan must be a finite number > 0"),
    (dict(table=np.ones((3, 3))), "table must be a finite [L, 4] array"),
])
def test_check_refuses_bad_values(kw, msg):
    with pytest.raises(ValueError, match=re.escape(msg)):
        scenarios.check_warm_start(scenarios.WarmStart(**kw))
    assert scenarios.check_warm_start(scenarios.WarmStart(kp=2, steps=1)).steps == 1
    assert scenarios.check_warm_start(scenarios.WarmStart(kp=2, steps=100000)).steps == 100000


def test_check_refusals_that_need_the_configuration():
    conf = config.Config(pl_size=3)
    with pytest.raises(ValueError, match="not a scenarios.WarmStart"):
        scenarios.check_warm_start(scenarios.ResidualLaw(kp=2), conf)
    with pytest.raises(ValueError, match="a gain table of 5 rows for pl_size=3"):
        scenarios.check_warm_start(scenarios.WarmStart(table=np.ones((5, 4))), conf)
    assert scenarios.check_warm_start(scenarios.WarmStart(table=np.ones((3, 4))), conf).gains(3).shape == (3, 4)
    conf_a = config.Config(pl_size=3, model="ModelA")
    assert conf_a.model == conf_a.modelA
    with pytest.raises(ValueError, match="kf needs Model B"):
        scenarios.check_warm_start(scenarios.WarmStart(kp=2, kf=0.5), conf_a)
    ok = scenarios.WarmStart(kp=2, kv=1)
    # trainer.check_warm_start: the run around the spec
    assert trainer.check_warm_start(conf, ok, "device") is ok
    with pytest.raises(ValueError, match="needs rng='device'"):
        trainer.check_warm_start(conf, ok, "host")
    with pytest.raises(ValueError, match="needs the decentralized framework"):
        trainer.check_warm_start(config.Config(pl_size=3, framework="centralized"), ok, "device")
    with pytest.raises(ValueError, match="residual policy: the law would act twice"):
        trainer.check_warm_start(conf, ok, "device", residual=scenarios.ResidualLaw(kp=2))
    with pytest.raises(ValueError, match="hyperparameter sweep or PBT"):
        trainer.check_warm_start(conf, ok, "device", hparams=[{}])
    with pytest.raises(ValueError, match="runs on one rank"):
        trainer.check_warm_start(conf, ok, "device", world_size=2)
    # actor_hold
    assert trainer.check_actor_hold(0) == 0 and trainer.check_actor_hold(7) == 7
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="actor_hold"):
            trainer.check_actor_hold(bad)
    with pytest.raises(ValueError, match="sweep's update reads its step sizes from its table"):
        trainer.check_actor_hold(3, hparams=[{}])
    assert trainer.check_actor_hold(0, hparams=[{}]) == 0


def test_record_round_trip():
    for w in (scenarios.WarmStart(kp=2, kv=1), scenarios.WarmStart(1.5, 0.5, -0.1, 0.3, steps=300, lr=2e-3, ep=2, ev=3, a=0.5, source="tuned"),
              scenarios.WarmStart(table=np.arange(12.0).reshape(3, 4), steps=7, source="searched")):
        rec = w.record()
        assert all(isinstance(p, list) and len(p) == 2 for p in rec)  # pairs, like ResidualLaw.record
        import json
        back = scenarios.WarmStart.from_record(json.loads(json.dumps(rec)))
        assert back.record() == rec
        for k in ("kp", "kv", "ka", "kf", "steps", "lr", "ep", "ev", "a", "source"):
            assert getattr(back, k) == getattr(w, k), k
        assert (back.table is None) == (w.table is None) and (w.table is None or np.array_equal(back.table, w.table))
    assert scenarios.WarmStart.from_record(None) is None
    with pytest.raises(ValueError, match="unknown or repeated"):
        scenarios.WarmStart.from_record([["kp", 1.0], ["scale", 1.0]])
    with pytest.raises(ValueError, match="unknown or repeated"):
        scenarios.WarmStart.from_record([["kp", 1.0], ["kp", 2.0]])


DEV = ["--rng", "device"]


@pytest.mark.parametrize("argv,msg", [
    (["--warm_start", "kp=2,kv=1"], "--warm_start needs --rng device"),
    (DEV + ["--warm_start", "kp=2,kv=1", "--residual", "kp=2,kv=1"], "--warm_start does not combine with --residual"),
    (DEV + ["--episodes", "platoon", "--warm_start", "kp=2", "--seeds", "1,2", "--sweep", "actor_lr=1e-3,1e-4"],
     "--warm_start does not combine with --sweep / --pbt"),
    (DEV + ["--warm_start", "kp=2,kx=1"], "--warm_start: warm_start: unknown key 'kx'"),
    (DEV + ["--warm_start", "kp=2,kp=1"], "--warm_start: warm_start: kp given twice"),
    (DEV + ["--warm_start", "kp=nan"], "--warm_start: baseline 'warm_start': kp=nan must be a finite number"),
    (DEV + ["--warm_start", "kp=2,steps=0"], "steps=0 must be a whole number in 1 .. 100000"),
    (DEV + ["--warm_start", "kp=2,steps=100001"], "steps=100001 must be a whole number in 1 .. 100000"),
    (DEV + ["--warm_start", "kp=2,lr=0"], "lr=0.0 must be a finite number > 0"),
    (DEV + ["--warm_start", "kp=2,ep=0"], "ep=0.0 must be a finite number > 0"),
    (DEV + ["--warm_start", "kp=2,ev=-1"], "ev=-1.0 must be a finite number > 0"),
    (DEV + ["--warm_start", "kp=2,a=inf"], "a=inf must be a finite number > 0"),
    (DEV + ["--warm_start", "tuned"], "--warm_start tuned needs --scenarios and --baseline_tune"),
    (DEV + ["--warm_start", "searched"], "--warm_start searched needs --scenarios and --baseline_search"),
    (["--actor_hold", "0"], "--actor_hold: N=0 must be >= 1"),
    (["--actor_hold", "-3"], "--actor_hold: N=-3 must be >= 1"),
    (["--actor_hold", "50", "--total_time_steps", "50"], "--actor_hold: N=50 must be below the run's 50 steps"),
    (DEV + ["--episodes", "platoon", "--actor_hold", "5", "--seeds", "1,2", "--sweep", "actor_lr=1e-3,1e-4"],
     "--actor_hold does not combine with --sweep / --pbt"),
])
def test_cli_argument_errors(argv, msg, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        cli.get_cmdl_args(["tr", *argv], config.Config())
    assert e.value.code == 2 and msg in capsys.readouterr().err


def test_cli_refuses_more_than_one_rank_and_what_needs_the_configuration(capsys, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cli.get_cmdl_args(["tr", *DEV, "--warm_start", "kp=2,kv=1"], config.Config())
    assert "--warm_start is not available under a process group of more than one rank" in capsys.readouterr().err
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(SystemExit):
        cli.get_cmdl_args(["tr", *DEV, "--warm_start", "kp=2,kf=0.5"], config.Config(model="ModelA"))
    assert "kf needs Model B" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.get_cmdl_args(["tr", *DEV, "--warm_start", "kp=2"], config.Config(framework="centralized"))
    assert "a warm start needs the decentralized framework" in capsys.readouterr().err
    args, conf = cli.get_cmdl_args(["tr", *DEV, "--warm_start", "kp=2,kv=1,steps=50", "--actor_hold", "10", "--total_time_steps", "100"],
                                   config.Config())
    assert isinstance(args.warm_start, scenarios.WarmStart) and args.warm_start.steps == 50 and args.actor_hold == 10
    assert cli._warm_kw(args) == dict(warm_start=args.warm_start, actor_hold=10)
    # without the flags: nothing is handed to the trainer, nothing recorded
    args, conf = cli.get_cmdl_args(["tr", *DEV], config.Config())
    assert args.warm_start is None and args.actor_hold is None and cli._warm_kw(args) == {}
    cli._record_warm(conf, args)
    assert not hasattr(conf, "warm_start") and not hasattr(conf, "actor_hold")


def test_sample_oracle_against_a_scalar_restatement():
    """clone_oracle.sample: every word from oracle.philox's block of (key, counter, m * 64 + b, stream 11); the law in float32, the
    terms added in order; kf skipped under Model A; sets of one (experiment, vehicle) draw the same rows whatever the set count."""
    gains = np.array([[2, 1, 0.25, 0.5], [1, 0.5, -0.1, 0.3], [3, 2, 0, 0]], np.float32)
    box = np.array([1.5, 1.5, 1.0, 1.0], np.float32)
    s, u = clone_oracle.sample(6, 4, 3, gains, box, -2.5, 2.5, False, 9, 4, seeds=(7, 8))
    assert s.shape == (6, 64, 4) and u.shape == (6, 64, 1) and s.dtype == u.dtype == np.float32
    f = np.float32
    for j, b in ((0, 0), (1, 63), (4, 17), (5, 1)):
        m, e = j % 3, j // 3
        w = philox.philox4x32_10(m * 64 + b, 11, 4, 0, (7, 8)[e], 0)
        x = [f(f(int(w[c]) >> 8) * f(2.0 / 16777216.0) - f(1.0)) * box[c] for c in range(4)]
        assert [float(v) for v in x] == [float(v) for v in s[j, b]]
        z = f(f(f(gains[m, 0] * x[0]) + f(gains[m, 1] * x[1])) + f(gains[m, 2] * x[2]))
        z4 = f(z + f(gains[m, 3] * x[3]))
        assert float(u[j, b, 0]) == float(min(max(z4, f(-2.5)), f(2.5)))
    assert np.all(np.abs(s) <= box) and np.all(np.abs(u) <= 2.5)
    # Model A (S = 3): three components, kf ignored
    s3, u3 = clone_oracle.sample(3, 3, 3, gains, box, -2.5, 2.5, True, 7, 4)
    assert np.array_equal(s3, s[:3, :, :3])  # experiment 0 of the batch drew what the solo key 7 draws
    g0 = gains.copy()
    g0[:, 3] = 0
    assert np.array_equal(u3, clone_oracle.sample(3, 4, 3, g0, box, -2.5, 2.5, False, 7, 4)[1])
    # a second platoon's sets repeat the first's rows; another counter draws other rows
    s2, u2 = clone_oracle.sample(12, 4, 3, gains, box, -2.5, 2.5, False, 0, 4, seeds=(7, 8))
    assert np.array_equal(s2[:6], s) and np.array_equal(s2[6:], s) and np.array_equal(u2[6:], u)
    assert not np.array_equal(clone_oracle.sample(3, 4, 3, gains, box, -2.5, 2.5, False, 7, 5)[0], s[:3])
    # the clip binds on some rows and not on others for the un-tuned law (2, 1, 0, 0) in the default box
    _, uc = clone_oracle.sample(3, 4, 3, np.tile(f([2, 1, 0, 0]), (3, 1)), box, -2.5, 2.5, False, 1, 0)
    assert 0.1 <= np.mean(np.abs(uc) == 2.5) <= 0.9


def test_grads_oracle_is_the_gradient_of_the_loss():
    """clone_oracle.grads: omlp.actor_forward / actor_backward with dout = 2 (out - u) / out.size, against central differences of the
    loss in float64 (A = 2, small widths)."""
    rs = np.random.RandomState(3)
    S, A = 5, 2
    w = omlp.init_actor(rs, S, A, H1=16, H2=32, dtype=np.float64)
    for i in (1, 2, 3, 4, 7, 8, 9, 10, 13):
        w[i] = w[i] + rs.uniform(-0.3, 0.3, w[i].shape)
    w[5], w[11] = np.abs(w[5]) + 0.5, np.abs(w[11]) + 0.5
    w[12] = w[12] * 30
    s, u = rs.normal(0, 1, (64, S)), rs.uniform(-2.5, 2.5, (64, A))
    g, loss, _ = clone_oracle.grads(w, s, u, 2.5)
    out = omlp.actor_forward(w, s, 2.5)
    assert np.isclose(loss, np.mean((out - u) ** 2)) and loss > 0.1
    assert [x.shape for x in g] == [w[i].shape for i in omlp.ACTOR_TRAINABLE]
    for gi, i in zip(g, omlp.ACTOR_TRAINABLE):
        idx = np.unravel_index(np.argmax(np.abs(gi)), gi.shape)
        h = 1e-6
        keep = w[i][idx]
        w[i][idx] = keep + h
        lp = np.mean((omlp.actor_forward(w, s, 2.5) - u) ** 2)
        w[i][idx] = keep - h
        lm = np.mean((omlp.actor_forward(w, s, 2.5) - u) ** 2)
        w[i][idx] = keep
        assert abs((lp - lm) / (2 * h) - gi[idx]) <= 1e-5 * max(1.0, abs(gi[idx])), (i, idx)


def _lay(S=4, A=1, H1=256, H2=128, Ha=48, B=64):
    return _hip.make_layout(S, A, H1, H2, Ha, B)


def test_clone_entry_points_refuse_on_the_host_before_any_hip_call():
    """Null pointers, B = 32 and a shape outside the learner's domain: status and message, no launch (this machine has no GPU: a
    launch would fail differently)."""
    one = ctypes.c_void_p(16)  # (never dereferenced: every refusal comes first)
    lay = _lay()
    with pytest.raises(_hip.AvdError, match=r"avd_actor_clone_f32 failed \(-?\d+\): avd_actor_clone_f32: null pointer"):
        _hip.call("avd_actor_clone_f32", ctypes.byref(lay), 1, None, one, one, one, 2.5, one, None, None)
    with pytest.raises(_hip.AvdError, match="avd_actor_clone_f32: null pointer"):
        _hip.call("avd_actor_clone_f32", ctypes.byref(lay), 1, one, one, one, one, 2.5, None, None, None)
    with pytest.raises(_hip.AvdError, match="avd_actor_clone_f32: null layout"):
        _hip.call("avd_actor_clone_f32", None, 1, one, one, one, one, 2.5, one, None, None)
    with pytest.raises(_hip.AvdError, match="avd_actor_clone_f32: n_sets=0"):
        _hip.call("avd_actor_clone_f32", ctypes.byref(lay), 0, one, one, one, one, 2.5, one, None, None)
    lay32 = _lay(B=32)
    with pytest.raises(_hip.AvdError, match=r"avd_actor_clone_f32: batch_size=32; the tile kernels implement B == 64"):
        _hip.call("avd_actor_clone_f32", ctypes.byref(lay32), 1, one, one, one, one, 2.5, one, None, None)
    for bad, msg in ((_lay(H2=48), "H2 a multiple of 32"), (_lay(H1=100), "H1 and Ha multiples of 16"), (_lay(S=65), "need S <= 64"),
                     (_lay(H2=288), "<= 256")):
        with pytest.raises(_hip.AvdError, match="avd_actor_clone_f32: need S <= 64, A <= 16") as e:
            _hip.call("avd_actor_clone_f32", ctypes.byref(bad), 1, one, one, one, one, 2.5, one, None, None)
        assert msg in str(e.value)
        with pytest.raises(_hip.AvdError) as ref:  # the learner's own refusal of the same shape: same status, same text after the name
            _hip.call("avd_learn_check_shape", ctypes.byref(bad))
        tail = lambda x: str(x.value).split(": ", 2)[2]
        status = lambda x: re.search(r"failed \((-?\d+)\)", str(x.value)).group(1)
        assert tail(e) == tail(ref) and status(e) == status(ref)
    # the sampler
    ok = (5, 4, 5, one, one, -2.5, 2.5, 0, 1, 0, None, 1, one, one, None)
    for i, val, msg in ((1, 5, "S=5"), (1, 2, "S=2"), (2, 0, "M=0"), (0, 7, "n_sets=7"), (0, 0, "n_sets=0"), (11, 2, "E=2"),
                        (3, None, "null pointer"), (4, None, "null pointer"), (12, None, "null pointer"), (13, None, "null pointer"),
                        (5, 3.0, "lo=3 > hi=2.5")):
        a = list(ok)
        a[i] = val
        with pytest.raises(_hip.AvdError, match="avd_clone_sample_f32: ") as e:
            _hip.call("avd_clone_sample_f32", *a)
        assert msg in str(e.value), (i, val, str(e.value))


def test_float64_oracle_fit_meets_the_conditions_of_the_end_to_end_test():
    """L = 3, 500 steps, Philox draws (key 1), default box, gains (2, 1, 0, 0), float64. Measured: first-step losses 2.79 / 3.04 / 2.71,
    mean loss of the last 50 steps 0.00411 (per actor 0.00383 .. 0.00425), evaluator score -3.142, the law's own -2.952 (gap 0.19);
    the float32 fit on the same draws: 0.00411 (differs by 2e-5 relative), the same score.
    The conditions are those tests/test_gpu_clone.py puts on its float32 reference."""
    r = clone_oracle.standard_fit("float64")
    losses = r["losses"]
    first, last = float(np.mean(losses[:, 0])), float(np.mean(losses[:, -50:]))
    print(f"WARM oracle f64: first {first:.4g} last50 {last:.4g} score {r['score']:.3f} law {r['law_score']:.3f}")
    assert last <= 0.01 and last * 100 <= first
    assert abs(r["score"] - r["law_score"]) <= 0.25
    r32 = clone_oracle.standard_fit("float32")
    last32 = float(np.mean(r32["losses"][:, -50:]))
    print(f"WARM oracle f32: last50 {last32:.4g} score {r32['score']:.3f}")
    assert last32 <= 0.01 and abs(r32["score"] - r32["law_score"]) <= 0.25  # (the GPU test's reference meets them too)
