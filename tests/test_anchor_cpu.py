"""The anchor without a device (tr --anchor, scenarios.Anchor, avd_learn_set_split_anchor_f16x3's host checks, tests/anchor_oracle.py):
the spec's parsing, checking and record round trip, weight_at's rounding and decay, every refusal of the trainer, the CLI and the entry
point, and the oracle's own properties -- linear in the weight, oracle.mlp.learn at weight 0, the law in linear_law's order."""
import ctypes

import numpy as np
import pytest

from avddpg_amd import __main__ as cli
from avddpg_amd import _hip, config, params, scenarios, trainer
from oracle import mlp as omlp
from tests import anchor_oracle, linear_oracle

FUSED3 = ["--fed_method", "interfrl", "--engine", "fused3", "--rng", "device"]


def _interfrl(**kw):
    return config.Config(fed_method="interfrl", **kw)


def test_parse_check_and_record_round_trip():
    a = scenarios.parse_anchor("kp=2, kv=1,kf=0.25,weight=0.5,decay=5000")
    assert isinstance(a, scenarios.Anchor) and isinstance(a, scenarios.LinearLaw)
    assert (a.kp, a.kv, a.ka, a.kf, a.weight, a.decay, a.source, a.pending, a.name) == (2.0, 1.0, 0, 0.25, 0.5, 5000, "given", False, "anchor")
    assert isinstance(a.decay, int)
    assert scenarios.check_anchor(a) is a
    d = scenarios.parse_anchor("kp=2,kv=1")
    assert (d.weight, d.decay) == (1.0, 0)
    rec = a.record()
    assert rec == [["kp", 2.0], ["kv", 1.0], ["ka", 0.0], ["kf", 0.25], ["weight", 0.5], ["decay", 5000], ["source", "given"]]
    b = scenarios.Anchor.from_record(rec)
    assert b.record() == rec and scenarios.Anchor.from_record(None) is None
    tab = scenarios.Anchor(table=[[2, 1, 0, 0], [1.5, 1, 0, 0.1]], weight=3, source="searched")
    back = scenarios.Anchor.from_record(tab.record())
    assert np.array_equal(back.gains(2), tab.gains(2)) and back.source == "searched" and back.weight == 3.0
    with pytest.raises(ValueError, match="unknown or repeated"):
        scenarios.Anchor.from_record(rec + [["scale", 1.0]])
    # the words stand in place of the gains, followed by the other keys
    for word in ("tuned", "searched"):
        w = scenarios.parse_anchor(f"{word},weight=10,decay=100")
        assert w.pending and w.source == word and (w.weight, w.decay) == (10.0, 100)
        law = scenarios.LinearLaw(word, 1.5, 0.5, 0, 0.2)
        got = w.with_gains(law, source=word)
        assert not got.pending and (got.kp, got.kv, got.kf, got.weight, got.decay, got.source) == (1.5, 0.5, 0.2, 10.0, 100, word)
    assert scenarios.parse_anchor("tuned").pending


@pytest.mark.parametrize("text,msg", [
    ("", "no gain given"), ("kp", "unknown key 'kp'"), ("scale=1", "unknown key 'scale'"), ("kp=2,kp=3", "kp given twice"),
    ("kp=two", "kp='two' is not a number"), ("kp=2,decay=1.5", "decay=1.5 is not a whole number"), ("kp=2,decay=inf", "is not a whole number"),
    ("tuned,kp=2", "kp given beside the word 'tuned'"), ("kp=2,tuned", "unknown key 'tuned'"),
])
def test_parse_refusals(text, msg):
    with pytest.raises(ValueError, match=msg):
        scenarios.parse_anchor(text)


def test_check_refusals():
    A = scenarios.Anchor
    for spec, msg in ((A(kp=float("nan")), "kp=nan must be a finite number"), (A(kp=2, weight=-1), "weight=-1 must be a finite number >= 0"),
                      (A(kp=2, weight=float("inf")), "weight=inf must be a finite"), (A(kp=2, weight=float("nan")), "weight=nan must be"),
                      (A(kp=2, weight=True), "weight=True"), (A(kp=2, weight=1e39), "does not fit float32"),
                      (A(kp=2, decay=-1), "decay=-1 must be a whole number"), (A(kp=2, decay=2.0), "decay=2.0 must be a whole number"),
                      (A(table=[[1, 2, 3]]), r"table must be a finite \[L, 4\]")):
        with pytest.raises(ValueError, match=msg):
            scenarios.check_anchor(spec)
    with pytest.raises(ValueError, match="is not a scenarios.Anchor"):
        scenarios.check_anchor(scenarios.WarmStart(kp=2))
    with pytest.raises(ValueError, match="kf needs Model B"):
        scenarios.check_anchor(A(kp=2, kf=0.5), _interfrl(model="ModelA"))
    with pytest.raises(ValueError, match="a gain table of 2 rows for pl_size=3"):
        scenarios.check_anchor(A(table=[[2, 1, 0, 0]] * 2), _interfrl(pl_size=3))
    assert scenarios.check_anchor(A(kp=2, weight=0)).weight == 0  # weight 0 is a spec: the anchor loss stays a diagnostic


def test_weight_at_rounds_once_and_decays_linearly():
    a = scenarios.Anchor(kp=2, weight=0.1)
    assert a.weight_at(0) == a.weight_at(10 ** 6) == float(np.float32(0.1)) != 0.1
    d = scenarios.Anchor(kp=2, weight=0.3, decay=7)
    for call in range(0, 12):
        want = np.float32(np.float64(0.3) * max(0.0, 1.0 - call / 7.0))  # float64, rounded once
        assert d.weight_at(call) == float(want), call
    assert d.weight_at(0) == float(np.float32(0.3)) and d.weight_at(7) == 0.0 and d.weight_at(8) == 0.0
    # (not the product of the rounded factors)
    assert any(d.weight_at(c) != float(np.float32(0.3) * np.float32(1.0 - c / 7.0)) for c in range(1, 7))
    assert scenarios.Anchor(kp=2, weight=2.0, decay=4).weight_at(2) == 1.0


def test_trainer_refusals_before_anything_is_allocated():
    ok, spec = _interfrl(), scenarios.Anchor(kp=2, kv=1)
    assert trainer.check_anchor(ok, spec, "fused3") is spec
    for engine in (None, "per_agent", "batched", "fused"):
        with pytest.raises(ValueError, match="an anchor needs shared_engine='fused3'"):
            trainer.check_anchor(ok, spec, engine)
    with pytest.raises(ValueError, match="an anchor needs shared weight sets"):
        trainer.check_anchor(config.Config(fed_method="intrafrl"), spec, "fused3")
    with pytest.raises(ValueError, match="an anchor needs shared weight sets"):
        trainer.check_anchor(config.Config(), spec, "fused3")  # no federation
    with pytest.raises(ValueError, match="an anchor needs shared weight sets"):
        trainer.check_anchor(ok, spec, "fused3", shared_sets=False)
    with pytest.raises(ValueError, match="hyperparameter sweep or PBT"):
        trainer.check_anchor(ok, spec, "fused3", hparams=[{}])
    with pytest.raises(ValueError, match="overlap_allreduce"):
        trainer.check_anchor(ok, spec, "fused3", overlap_allreduce=True)
    with pytest.raises(ValueError, match="an anchor runs on one rank"):
        trainer.check_anchor(ok, spec, "fused3", world_size=2)
    with pytest.raises(ValueError, match="an anchor needs the decentralized framework"):
        trainer.check_anchor(_interfrl(framework="centralized"), spec, "fused3")
    with pytest.raises(ValueError, match="kf needs Model B"):
        trainer.check_anchor(_interfrl(model="ModelA"), scenarios.Anchor(kp=2, kf=1), "fused3")
    with pytest.raises(ValueError, match="have not been filled in"):
        trainer.check_anchor(ok, scenarios.parse_anchor("tuned"), "fused3")
    with pytest.raises(ValueError, match="weight=-2"):
        trainer.check_anchor(ok, scenarios.Anchor(kp=2, weight=-2), "fused3")


@pytest.mark.parametrize("argv,msg", [
    (["--anchor", "kp=2,kv=1", "--rng", "device", "--fed_method", "interfrl"], "--anchor needs --engine fused3"),
    (["--anchor", "kp=2,kv=1", "--rng", "device", "--fed_method", "interfrl", "--engine", "per_agent"], "--anchor needs --engine fused3"),
    (["--anchor", "kp=2,kv=1", "--rng", "device", "--fed_method", "interfrl", "--engine", "fused"], "--anchor needs --engine fused3"),
    ([*FUSED3, "--anchor", "kp=2,kv=1", "--episodes", "platoon", "--seeds", "1,2", "--sweep", "actor_lr=1e-4,1e-3"], "--anchor does not combine with --sweep / --pbt"),
    ([*FUSED3, "--anchor", "kp=2,weight=-1"], "--anchor: anchor: weight=-1.0 must be a finite number >= 0"),
    ([*FUSED3, "--anchor", "kp=2,decay=-5"], "--anchor: anchor: decay=-5 must be a whole number"),
    ([*FUSED3, "--anchor", "kx=2"], "--anchor: anchor: unknown key 'kx'"),
    ([*FUSED3, "--anchor", "tuned,weight=2"], "--anchor tuned needs --scenarios and --baseline_tune"),
    ([*FUSED3, "--anchor", "searched"], "--anchor searched needs --scenarios and --baseline_search"),
    (["--rng", "device", "--engine", "fused3", "--anchor", "kp=2"], "--anchor: an anchor needs shared weight sets"),
    (["--rng", "device", "--engine", "fused3", "--fed_method", "intrafrl", "--anchor", "kp=2"], "--anchor: an anchor needs shared weight sets"),
])
def test_cli_argument_errors(argv, msg, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        cli.get_cmdl_args(["tr", *argv], config.Config())
    assert e.value.code == 2 and msg in capsys.readouterr().err


def test_cli_refuses_more_than_one_rank_and_what_needs_the_configuration(capsys, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cli.get_cmdl_args(["tr", *FUSED3, "--anchor", "kp=2,kv=1"], config.Config())
    assert "--anchor is not available under a process group of more than one rank" in capsys.readouterr().err
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(SystemExit):
        cli.get_cmdl_args(["tr", *FUSED3, "--anchor", "kp=2,kf=0.5"], config.Config(model="ModelA"))
    assert "kf needs Model B" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.get_cmdl_args(["tr", *FUSED3, "--anchor", "kp=2"], config.Config(framework="centralized"))
    assert "an anchor needs the decentralized framework" in capsys.readouterr().err
    args, conf = cli.get_cmdl_args(["tr", *FUSED3, "--anchor", "kp=2,kv=1,weight=10,decay=50", "--warm_start", "kp=2,kv=1", "--actor_hold", "10",
                                    "--total_time_steps", "100"], config.Config())
    assert isinstance(args.anchor, scenarios.Anchor) and (args.anchor.weight, args.anchor.decay) == (10.0, 50)
    assert cli._anchor_kw(args) == dict(anchor=args.anchor)
    # with a residual policy: the law is the target of the correction
    args, conf = cli.get_cmdl_args(["tr", *FUSED3, "--anchor", "kp=0", "--residual", "kp=2,kv=1"], config.Config())
    assert args.anchor.kp == 0 and args.residual.kp == 2
    # without the flag: nothing is handed to the trainer, nothing recorded
    args, conf = cli.get_cmdl_args(["tr", *FUSED3], config.Config())
    assert args.anchor is None and cli._anchor_kw(args) == {}
    cli._record_anchor(conf, args, None)
    assert not hasattr(conf, "anchor")


_BOGUS = 0x1000


def _entry(lay, n_agents=6, n_sets=2, M=2, lo=-2.5, hi=2.5, weight=1.0, **null):
    """avd_learn_set_split_anchor_f16x3 with non-null pointers nothing reads, everywhere but where `null` names an argument."""
    names = ("theta", "stats", "theta_t", "stats_t", "s", "a", "r", "s2", "grads", "losses", "workspace", "gains", "anchor_loss")
    p = {k: (None if k in null else ctypes.c_void_p(_BOGUS * (i + 1))) for i, k in enumerate(names)}
    _hip.call("avd_learn_set_split_anchor_f16x3", None if lay is None else ctypes.byref(lay), n_agents, n_sets, p["theta"], p["stats"],
              p["theta_t"], p["stats_t"], p["s"], p["a"], p["r"], p["s2"], None, 0.99, 2.5, p["grads"], p["losses"], p["workspace"], 0,
              p["gains"], M, 0, lo, hi, weight, p["anchor_loss"], None)


def test_entry_point_refuses_on_the_host_before_any_hip_call():
    """One fault per call, with status and text (no GPU here: a call that got past its checks would fail with a HIP error instead; the
    last case gets as far as the workspace size, the last host check)."""
    who = "avd_learn_set_split_anchor_f16x3"
    ref = _hip.make_layout(4, 1, 256, 128, 48, 64)
    refuse = lambda code, msg: pytest.raises(_hip.AvdError, match=rf"failed \({code}\): {who}: {msg}")
    with refuse(-1, "null layout"):
        _entry(None)
    with refuse(-3, "serves the reference widths only"):
        _entry(_hip.make_layout(4, 1, 320, 160, 48, 64))
    with refuse(-3, "serves the reference widths only"):
        _entry(_hip.make_layout(4, 1, 256, 128, 48, 32))
    for kw, msg in ((dict(n_agents=5), "n_agents=5 n_sets=2"), (dict(n_agents=0), "n_agents=0 n_sets=2"), (dict(n_sets=0), "n_agents=6 n_sets=0"),
                    (dict(n_agents=130, n_sets=65, M=1), "n_agents=130 n_sets=65"),
                    (dict(gains=1), "null gains / anchor_loss"), (dict(anchor_loss=1), "null gains / anchor_loss"),
                    (dict(M=0), r"n_sets=2 M=0 \(n_sets must be a multiple of M >= 1\)"), (dict(M=-2), "n_sets=2 M=-2"),
                    (dict(n_agents=12, n_sets=6, M=4), "n_sets=6 M=4"),
                    (dict(weight=-1e-3), r"weight=-0.001 \(must be finite and >= 0\)"), (dict(weight=float("inf")), "weight=inf"),
                    (dict(weight=float("-inf")), "weight=-inf"), (dict(weight=float("nan")), "weight=-?nan"),
                    (dict(lo=1.0, hi=-1.0), "lo=1 > hi=-1"),
                    (dict(theta=1), "null pointer"), (dict(s=1), "null pointer"), (dict(s2=1), "null pointer"), (dict(grads=1), "null pointer"),
                    (dict(workspace=1), "null pointer"), (dict(), r"workspace 0 B < \d+ B"), (dict(weight=0.0), r"workspace 0 B < \d+ B"),
                    (dict(weight=-0.0), r"workspace 0 B < \d+ B"), (dict(lo=2.5, hi=2.5), r"workspace 0 B < \d+ B")):
        with refuse(-1, msg):
            _entry(ref, **kw)
    assert _hip._PROTOS[who][:19] == _hip._PROTOS["avd_learn_set_split_f16x3"][:19]  # the un-anchored call's arguments first


def _small_nets(rs, S=4, dtype=np.float64):
    """Four weight lists at the reference widths from the package's initialiser, the scalars off their initial values."""
    lay = _hip.make_layout(S, 1, 256, 128, 48, 64)
    nets = []
    for _ in range(2):
        th, st = params.init_weights(lay, rs)
        for which in ("actor", "critic"):
            w = params.unpack(lay, th, st, which)
            for x in w:
                if x.ndim == 1:
                    x += rs.uniform(-0.2, 0.2, x.shape).astype(np.float32)
            for i in ((5, 11) if which == "actor" else (7, 11, 17)):
                w[i][:] = np.abs(w[i]) + 0.5
            nets.append([x.astype(dtype) for x in w])
    return nets  # actor, critic, target actor, target critic


def test_the_oracle_is_linear_in_the_weight_and_learn_at_zero():
    rs = np.random.RandomState(5)
    P, S = 3, 4
    nets = _small_nets(rs, S)
    s = rs.normal(0, 1.5, size=(P, 64, S)).astype(np.float32)
    a = rs.uniform(-2.5, 2.5, size=(P, 64, 1)).astype(np.float32)
    r = -np.abs(rs.normal(0, 0.3, size=(P, 64))).astype(np.float32)
    s2 = rs.normal(0, 1.5, size=(P, 64, S)).astype(np.float32)
    row = np.array([2.0, 1.0, -0.3, 0.4], np.float32)
    cat = lambda x: x.reshape(P * 64, *x.shape[2:])
    cg, ag, aux = omlp.learn((cat(s), cat(a), cat(r)[:, None], cat(s2)), *nets)
    cg0, ag0, aux0 = anchor_oracle.learn((s, a, r, s2), nets, row, 0.0, -2.5, 2.5, False)
    for x, y in zip(list(cg) + list(ag), list(cg0) + list(ag0)):
        assert np.array_equal(x, y)
    assert aux0["critic_loss"] == float(aux["critic_loss"]) and aux0["actor_loss"] == float(aux["actor_loss"]) and aux0["anchor_loss"] > 0
    g1 = anchor_oracle.learn((s, a, r, s2), nets, row, 1.0, -2.5, 2.5, False)
    g3 = anchor_oracle.learn((s, a, r, s2), nets, row, 3.0, -2.5, 2.5, False)
    for x0, x1, x3, c1, c3 in zip(ag0, g1[1], g3[1], g1[0], g3[0]):
        assert np.allclose(x3 - x0, 3.0 * (x1 - x0), rtol=1e-12, atol=1e-18) and np.abs(x1 - x0).max() > 0
        assert np.array_equal(c1, c3)  # the critic's gradients do not see the anchor
    assert g1[2] == g3[2] == aux0  # nor do the losses; the anchor loss does not carry the weight
    # the behaviour-cloning summand is the gradient of weight * mean((mu - u*)^2): a finite difference on the output bias
    act = [x.copy() for x in nets[0]]
    u = anchor_oracle.law_rows(row, cat(s), -2.5, 2.5, False).astype(np.float64)
    loss = lambda w: float(np.mean((omlp.actor_forward(w, cat(s).astype(np.float64), 2.5)[:, 0] - u) ** 2))
    h = 1e-6
    act[13][0] += h
    up = loss(act)
    act[13][0] -= 2 * h
    fd = (up - loss(act)) / (2 * h)
    bc = anchor_oracle.parts((s, a, r, s2), nets, row, -2.5, 2.5, False)["bc"]
    assert abs(float(bc[-1][0]) - fd) <= 1e-6 * abs(fd)
    # agent weights: uniform factors give the concatenated batch's terms; the weighted anchor loss is the weighted mean
    ones = anchor_oracle.learn((s, a, r, s2), nets, row, 3.0, -2.5, 2.5, False, agent_weight=np.ones(P))
    for x, y in zip(g3[1], ones[1]):
        assert np.allclose(x, y, rtol=1e-11, atol=1e-16)
    aw = np.array([0.5, 1.0, 1.5])
    wl = anchor_oracle.learn((s, a, r, s2), nets, row, 3.0, -2.5, 2.5, False, agent_weight=aw)[2]["anchor_loss"]
    per = [anchor_oracle.learn((s[p:p + 1], a[p:p + 1], r[p:p + 1], s2[p:p + 1]), nets, row, 0.0, -2.5, 2.5, False)[2]["anchor_loss"] for p in range(P)]
    assert abs(wl - float(np.dot(aw, per)) / P) <= 1e-12 * wl


def test_the_oracles_law_is_linear_law_in_float32():
    rs = np.random.RandomState(9)
    s = rs.normal(0, 1.5, size=(200, 4)).astype(np.float32)
    row = np.array([2.3, 1.1, -0.3, 0.45], np.float32)
    for model_a in (False, True):
        got = anchor_oracle.law_rows(row, s, -2.5, 2.5, model_a)
        assert got.dtype == np.float32
        for b in range(len(s)):
            want = np.float32(linear_oracle.law(row, s[b, :3 if model_a else 4], np.float32(-2.5), np.float32(2.5)))
            assert got[b] == want, (model_a, b)
    assert np.array_equal(anchor_oracle.law_rows(row, s[:, :3], -2.5, 2.5, True), anchor_oracle.law_rows(row, s, -2.5, 2.5, True))
    big = anchor_oracle.law_rows(8 * row, s, -2.5, 2.5, False)
    assert np.mean(np.abs(big) == 2.5) > 0.5
