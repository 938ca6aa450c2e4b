"""VecTrainer(target_noise=...) and `tr --target_noise SPEC` on the GPU, 8 platoons x 3 vehicles on the fused3 engine: the trainer hands
the sampled batch, the noise, its seed (or its seed table) and the 0-based learner-call count to avd_learn_set_split_smooth_f16x3; sigma
0 trains what the run without the keyword trains, bit for bit; a seed batch's experiment draws its solo run's noise; an anchor's loss
buffers still fill; and the CLI end to end, with its refusals."""
import json
import os

import numpy as np
import pytest
import torch

from avddpg_amd import __main__ as cli
from avddpg_amd import config, scenarios, trainer, vec
from avddpg_amd.trainer import TargetNoise
from tests.gpu_util import need_gpu
from tests.test_gpu_residual import _esim_rewards, _files, _run

pytestmark = pytest.mark.gpu

P, L = 8, 3
GATE = 65  # the replay gate: the first learner call is step 65's (strictly more than batch_size rows)


def _conf(**kw):
    return config.Config(**{**dict(num_platoons=P, pl_size=L, buffer_size=200, fed_method="interfrl"), **kw})


def _vt(noise=None, seed=5, **kw):
    if "seeds" not in kw:
        kw["seed"] = seed
    vt = trainer.VecTrainer(_conf(), rng="device", auto_reset="platoon", shared_engine="fused3", target_noise=noise, **kw)
    vt.reset_episode()
    return vt


def _steps(vt, n):
    for _ in range(n):
        vt.step()
    torch.cuda.synchronize()
    return vt


def _spy(monkeypatch, vt, seen):
    real = vt.agents.learn_set_split_smooth

    def spy(s, a, r, s2, n, noise, counter, **kw):
        seen.update(batch=[x.clone() for x in (s, a, r, s2)], n=n, noise=noise, counter=counter, kw=dict(kw),
                    aw=None if kw.get("agent_weight") is None else kw["agent_weight"].clone(),
                    theta=[x.clone() for x in (vt.agents.theta, vt.agents.stats, vt.agents.theta_t, vt.agents.stats_t)])
        return real(s, a, r, s2, n, noise, counter, **kw)

    monkeypatch.setattr(vt.agents, "learn_set_split_smooth", spy)


def test_a_step_hands_the_sampled_batch_the_noise_and_the_call_count_to_the_entry_point(monkeypatch):
    need_gpu()
    tn = TargetNoise(0.2)
    vt = _steps(_vt(tn, seed=5), GATE + 1)  # two learner calls done
    assert vt.learner_calls == 2 and vt.target_noise is tn
    seen = {}
    _spy(monkeypatch, vt, seen)
    vt.step()
    torch.cuda.synchronize()
    assert vt.learner_calls == 3 and seen["n"] == P * L and seen["noise"] is tn and seen["counter"] == 2
    assert seen["kw"]["seed"] == 5 and seen["kw"]["d_seeds"] is None and seen["kw"]["M"] == L and seen["kw"]["anchor"] is None
    # a direct call on the same batch from the same weights, counter = learner_calls - 1
    grp = vec.AgentGroup(L, 4, 1, _conf())
    for dst, src in zip((grp.theta, grp.stats, grp.theta_t, grp.stats_t), seen["theta"]):
        dst.copy_(src)
    g = grp.learn_set_split_smooth(*seen["batch"], P * L, tn, vt.learner_calls - 1, agent_weight=seen["aw"], M=L, seed=5)
    torch.cuda.synchronize()
    assert torch.equal(g, vt.set_grads)
    other = grp.learn_set_split_smooth(*seen["batch"], P * L, tn, vt.learner_calls, agent_weight=seen["aw"], M=L, seed=5)
    torch.cuda.synchronize()
    assert not torch.equal(other, vt.set_grads)  # (the counter is part of the key)


def test_sigma_zero_trains_what_the_run_without_the_keyword_trains():
    need_gpu()
    plain = _steps(_vt(None), GATE + 100)
    zero = _steps(_vt(TargetNoise(0.0)), GATE + 100)
    assert plain.target_noise is None and zero.target_noise.sigma == 0.0
    assert plain.learner_calls == zero.learner_calls == 101
    for name in ("theta", "theta_t", "stats", "stats_t", "m", "v"):
        assert torch.equal(getattr(plain.agents, name), getattr(zero.agents, name)), name
    assert torch.equal(plain.env.x, zero.env.x)
    noisy = _steps(_vt(TargetNoise(0.2)), GATE + 100)
    assert not torch.equal(noisy.agents.theta, plain.agents.theta) and bool(torch.isfinite(noisy.agents.theta).all())


def test_a_seed_batch_passes_its_table_and_each_experiment_draws_its_solo_noise(monkeypatch):
    need_gpu()
    seeds = (4, 8)
    tn = TargetNoise(0.2)
    batch = _steps(_vt(tn, seeds=seeds), GATE - 1)
    seen = {}
    _spy(monkeypatch, batch, seen)
    batch.step()
    torch.cuda.synchronize()
    E = len(seeds)
    assert batch.learner_calls == 1 and seen["counter"] == 0 and seen["n"] == P * E * L and seen["kw"]["M"] == L
    assert seen["kw"]["seed"] is None and seen["kw"]["d_seeds"] is batch.env.d_seeds
    assert seen["kw"]["d_seeds"].cpu().tolist() == list(seeds)
    assert bool(torch.isfinite(batch.set_grads).all())
    # the noise of that call, through target_smooth on a zero action: experiment e's agents get the solo run's draws
    n = P * E * L
    big = batch.agents.target_smooth(torch.zeros(n, 64, device="cuda"), tn, 0, M=L, d_seeds=batch.env.d_seeds)
    v = np.arange(n)
    for e, k in enumerate(seeds):
        solo = _steps(_vt(tn, seed=k, init_seed=k), GATE - 1)
        got = {}
        _spy(monkeypatch, solo, got)
        solo.step()
        torch.cuda.synchronize()
        assert got["kw"]["seed"] == k and got["kw"]["d_seeds"] is None and got["counter"] == 0
        mine = solo.agents.target_smooth(torch.zeros(P * L, 64, device="cuda"), tn, 0, M=L, seed=got["kw"]["seed"])
        sel = torch.from_numpy(v[(v // L) % E == e]).cuda()
        assert torch.equal(big[sel], mine), e
        assert bool((mine != 0).any())
    assert not torch.equal(big[torch.from_numpy(v[(v // L) % E == 0]).cuda()], big[torch.from_numpy(v[(v // L) % E == 1]).cuda()])


def test_with_an_anchor_the_anchor_loss_buffers_still_fill(monkeypatch):
    need_gpu()
    spec = scenarios.Anchor(table=[[2, 1, 0, 0], [1.5, 1.2, -0.1, 0.3], [2.5, 0.8, 0, 0.5]], weight=4.0, decay=10)
    tn = TargetNoise(0.2)
    vt = _steps(_vt(tn, anchor=spec), GATE - 1)
    assert vt.learner_calls == 0 and bool((vt.anchor_losses() == 0).all()) and vt.anchor_loss_first is None
    seen = {}
    _spy(monkeypatch, vt, seen)
    called = []
    monkeypatch.setattr(vt.agents, "learn_set_split_anchor", lambda *a, **k: called.append(1))
    _steps(vt, 2)
    assert vt.learner_calls == 2 and not called  # one call carries both
    gains, weight, al = seen["kw"]["anchor"]
    assert np.array_equal(gains.cpu().numpy(), spec.gains(L)) and weight == spec.weight_at(1) == vt.anchor_weight and al is vt.anchor_loss
    assert bool((vt.anchor_losses() > 0).all()) and bool((vt.anchor_loss_first > 0).all())
    assert not torch.equal(vt.anchor_loss_first, vt.anchor_losses())
    # the anchor's side of the first call is the anchored run's without noise: same seed, same first batch
    ref = _steps(_vt(None, anchor=spec), GATE)
    assert torch.equal(ref.anchor_loss_first, vt.anchor_loss_first)


TR = ("tr", "--pl_num", str(P), "--pl_size", str(L), "--buffer_size", "500", "--total_time_steps", "200", "--rng", "device", "--episodes",
      "platoon", "--report_every", "100", "--fed_method", "interfrl", "--engine", "fused3", "--seed", "3")


def test_cli_end_to_end(tmp_path, capsys):
    """conf.json's target_noise record in the run's directory and in best/, `esim` on both (it ignores the record), a seed batch's
    per-experiment record beside an anchor's; a run with sigma 0 writes the files of the run without the flag, byte for byte, and that
    run records nothing."""
    need_gpu()
    cj = lambda d: json.load(open(os.path.join(d, "conf.json")))
    run = _run(capsys, *TR, "--target_noise", "sigma=0.2,clip=0.4", "--keep_best", "100", "--out", str(tmp_path / "a"))[-1]
    j = cj(run)
    assert j["target_noise"] == [["sigma", 0.2], ["clip", 0.4]]
    bj = cj(os.path.join(run, "best"))
    assert bj["target_noise"] == j["target_noise"]
    assert len(_esim_rewards(capsys, run, j)) == j["saved_platoons"]
    assert len(_esim_rewards(capsys, os.path.join(run, "best"), bj)) == bj["saved_platoons"]
    batch = _run(capsys, *TR[:-2], "--target_noise", "sigma=0.2", "--anchor", "kp=2,kv=1", "--seeds", "3,4", "--out", str(tmp_path / "b"))[-1]
    for k in (3, 4):
        rec = cj(os.path.join(batch, f"seed{k}"))
        assert rec["target_noise"] == [["sigma", 0.2], ["clip", 0.5]] and len(dict(rec["anchor"])["anchor_loss_last"]) == L
    plain = _run(capsys, *TR, "--out", str(tmp_path / "p"))[-1]
    assert "target_noise" not in cj(plain)
    zero = _run(capsys, *TR, "--target_noise", "sigma=0", "--out", str(tmp_path / "z"))[-1]
    a, b = _files(plain), _files(zero)
    assert set(a) == set(b) and "curve.csv" in a
    for f in a:
        assert a[f] == b[f], f
    assert _files(run)["curve.csv"] != a["curve.csv"]


@pytest.mark.parametrize("argv,msg", [
    (("--engine", "fused"), "--target_noise needs --engine fused3"),
    (("--engine", "per_agent"), "--target_noise needs --engine fused3"),
    (("--engine", "fused3", "--rng", "host"), "--target_noise needs --rng device"),
    (("--engine", "fused3", "--seeds", "1,2", "--sweep", "actor_lr=1e-4,1e-3"), "--target_noise does not combine with --sweep / --pbt"),
    (("--engine", "fused3", "--seeds", "1,2", "--sweep", "actor_lr=1e-4,1e-3", "--pbt", "100"), "--target_noise does not combine with --sweep / --pbt"),
    (("--engine", "fused3", "centralized"), "target noise needs the decentralized framework"),
])
def test_cli_refusals_exit_before_anything_is_allocated(argv, msg, tmp_path, capsys, monkeypatch):
    need_gpu()
    monkeypatch.setattr(trainer, "VecTrainer", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a trainer was built")))
    base = ["tr", "--pl_num", str(P), "--pl_size", str(L), "--total_time_steps", "200", "--episodes", "platoon", "--fed_method", "interfrl",
            "--out", str(tmp_path / "r"), "--target_noise", "sigma=0.2"]
    if "--rng" not in argv:
        base += ["--rng", "device"]
    conf = config.Config(framework="centralized") if argv[-1] == "centralized" else None  # (the framework is not a flag of the CLI)
    with pytest.raises(SystemExit) as e:
        cli.main(base + [x for x in argv if x != "centralized"], conf)
    assert e.value.code == 2 and msg in capsys.readouterr().err
    assert not os.path.exists(tmp_path / "r")


def test_the_trainer_refuses_more_than_one_rank_and_the_overlapped_exchange():
    need_gpu()
    for kw, msg in ((dict(overlap_allreduce=True), "overlap_allreduce"), (dict(rng="host"), "needs rng='device'"),
                    (dict(shared_engine="fused"), "needs shared_engine='fused3'")):
        with pytest.raises(ValueError, match=msg):
            trainer.VecTrainer(_conf(), **{**dict(rng="device", auto_reset="platoon", shared_engine="fused3", target_noise=TargetNoise(0.2)), **kw})
    with pytest.raises(ValueError, match="runs on one rank"):
        trainer.check_target_noise(TargetNoise(0.2), _conf(), "fused3", world_size=2)
