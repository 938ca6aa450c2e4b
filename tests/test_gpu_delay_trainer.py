"""VecTrainer(policy_delay=...) and `tr --policy_delay D` on the GPU, 8 platoons x 3 vehicles on the fused3 engine with the device's
generator: on a d = 3 schedule the actors and every target move on calls 3, 6, 9, 12 only while the critics move on every call and
the two Adam counts run apart; d = 1 trains what the run without the keyword trains, bit for bit, through the new update entry; the
keyword composes with target_noise, anchor and a seed batch; and the CLI end to end."""
import json
import os

import pytest
import torch

from avddpg_amd import config, scenarios, trainer
from avddpg_amd.trainer import TargetNoise
from tests.gpu_util import need_gpu
from tests.test_gpu_residual import _esim_rewards, _files, _run

pytestmark = pytest.mark.gpu

P, L = 8, 3
GATE = 65  # the replay gate: the first learner call is step 65's (strictly more than batch_size rows)
STATE = ("theta", "theta_t", "stats", "stats_t", "m", "v", "step")


def _conf(**kw):
    return config.Config(**{**dict(num_platoons=P, pl_size=L, buffer_size=200, fed_method="interfrl"), **kw})


def _vt(delay=None, seed=5, **kw):
    if "seeds" not in kw:
        kw["seed"] = seed
    vt = trainer.VecTrainer(_conf(), rng="device", auto_reset="platoon", shared_engine="fused3", policy_delay=delay, **kw)
    vt.reset_episode()
    return vt


def _steps(vt, n):
    for _ in range(n):
        vt.step()
    torch.cuda.synchronize()
    return vt


def _bits(x):
    return x.contiguous().view(torch.int32)


def test_actors_and_targets_move_on_policy_calls_only_and_the_counts_run_apart():
    need_gpu()
    vt = _steps(_vt(3), GATE - 1)
    ag, A = vt.agents, vt.agents.lay.actor_size
    assert vt.learner_calls == 0 and vt.policy_delay == 3 and ag.actor_step is not None and int(ag.actor_step.abs().sum()) == 0
    ag.stats_t.add_(0.25)  # off their nets' statistics: every soft update then moves them, whether or not training moves stats
    snap = lambda: {k: getattr(ag, k).clone() for k in ("theta", "theta_t", "stats_t", "m", "v")}
    for call in range(1, 13):
        before = snap()
        _steps(vt, 1)
        now = snap()
        policy = call % 3 == 0
        assert vt.learner_calls == call and vt.policy_call is policy
        same = lambda k, sl=slice(None): torch.equal(_bits(before[k][:, sl]), _bits(now[k][:, sl]))
        every_set = lambda k, sl: bool((_bits(before[k][:, sl]) != _bits(now[k][:, sl])).any(dim=1).all())
        for k in ("theta", "m", "v"):
            assert every_set(k, slice(A, None)), (call, k, "the critic block moves on every call")
            assert every_set(k, slice(0, A)) if policy else same(k, slice(0, A)), (call, k, "actor block")
        assert every_set("theta_t", slice(None)) if policy else same("theta_t"), (call, "theta_t")
        assert every_set("stats_t", slice(None)) if policy else same("stats_t"), (call, "stats_t")
        assert ag.step.tolist() == [call] * L and ag.actor_step.tolist() == [call // 3] * L, call
        if not policy:  # the TD-only call's slab: zeros where the actor's gradients would be
            assert bool((_bits(vt.set_grads[:, :A]) == 0).all()) and bool((vt.set_losses[:, 1] == 0).all())
        else:
            assert bool((vt.set_grads[:, :A] != 0).any())
    assert vt.nonfinite_updates() == 0
    assert bool(torch.isfinite(ag.theta).all())


def test_delay_one_trains_what_the_run_without_the_keyword_trains():
    need_gpu()
    plain = _steps(_vt(None), GATE + 9)
    one = _steps(_vt(1), GATE + 9)
    assert plain.policy_delay is None and plain.agents.actor_step is None and one.policy_delay == 1
    assert plain.learner_calls == one.learner_calls == 10
    for name in STATE:
        assert torch.equal(_bits(getattr(plain.agents, name)), _bits(getattr(one.agents, name))), name
    assert torch.equal(one.agents.actor_step, one.agents.step) and one.agents.step.tolist() == [10] * L
    assert torch.equal(plain.env.x, one.env.x)
    two = _steps(_vt(2), GATE + 9)
    assert not torch.equal(two.agents.theta, plain.agents.theta) and bool(torch.isfinite(two.agents.theta).all())


def test_composes_with_target_noise_an_anchor_and_a_seed_batch():
    """Learner call 0 of a d = 3 run is a skipped call: experiment 0's critic block of the batch's slab equals its solo run's within the
    engine's tolerance for a changed set count (2e-5 of the slab's max: tests/test_gpu_seed_batch.py). The anchor's first loss is the
    first policy call's."""
    need_gpu()
    spec = scenarios.Anchor(table=[[2, 1, 0, 0], [1.5, 1.2, -0.1, 0.3], [2.5, 0.8, 0, 0.5]], weight=4.0, decay=10)
    tn = TargetNoise(0.2)
    batch = _steps(_vt(3, seeds=[1, 2], target_noise=tn, anchor=spec), GATE)
    solo = _steps(_vt(3, seed=1, init_seed=1, target_noise=tn, anchor=spec), GATE)
    A = batch.agents.lay.actor_size
    assert batch.learner_calls == solo.learner_calls == 1 and not batch.policy_call and not solo.policy_call
    mine, ref = batch.set_grads[:L], solo.set_grads
    assert bool((batch.set_grads[:, :A] == 0).all()) and bool((ref[:, :A] == 0).all())
    scale = ref[:, A:].abs().max().item()
    err = (mine[:, A:] - ref[:, A:]).abs().max().item()
    print(f"experiment 0 against its solo run: {err / scale:.2e} of the slab's max")
    assert scale > 0 and err <= 2e-5 * scale
    assert (batch.set_grads[L:, A:] - ref[:, A:]).abs().max().item() > 1e-3 * scale  # (the other experiment trains something else)
    assert batch.anchor_loss_first is None
    _steps(batch, 2)
    assert batch.learner_calls == 3 and batch.policy_call and bool((batch.anchor_loss_first > 0).all())
    assert batch.agents.step.tolist() == [3] * (2 * L) and batch.agents.actor_step.tolist() == [1] * (2 * L)
    assert bool(torch.isfinite(batch.agents.theta).all()) and batch.nonfinite_updates() == 0


TR = ("tr", "--pl_num", str(P), "--pl_size", str(L), "--buffer_size", "500", "--total_time_steps", "200", "--rng", "device", "--episodes",
      "platoon", "--report_every", "100", "--fed_method", "interfrl", "--engine", "fused3", "--seed", "3")


def test_cli_end_to_end(tmp_path, capsys):
    """conf.json's policy_delay in the run's directory and in best/, `esim` on both (it ignores the field); a run with D = 1 writes the
    files of the run without the flag, byte for byte, and that run records nothing."""
    need_gpu()
    cj = lambda d: json.load(open(os.path.join(d, "conf.json")))
    run = _run(capsys, *TR, "--policy_delay", "2", "--target_noise", "sigma=0.2", "--keep_best", "100", "--out", str(tmp_path / "a"))[-1]
    j = cj(run)
    assert j["policy_delay"] == 2
    bj = cj(os.path.join(run, "best"))
    assert bj["policy_delay"] == 2
    assert len(_esim_rewards(capsys, run, j)) == j["saved_platoons"]
    assert len(_esim_rewards(capsys, os.path.join(run, "best"), bj)) == bj["saved_platoons"]
    plain = _run(capsys, *TR, "--out", str(tmp_path / "p"))[-1]
    assert "policy_delay" not in cj(plain)
    one = _run(capsys, *TR, "--policy_delay", "1", "--out", str(tmp_path / "o"))[-1]
    assert cj(one)["policy_delay"] == 1
    a, b = _files(plain), _files(one)
    assert set(a) == set(b) and "curve.csv" in a
    for f in a:
        assert a[f] == b[f], f
    batch = _run(capsys, *TR[:-2], "--policy_delay", "2", "--seeds", "3,4", "--out", str(tmp_path / "b"))[-1]
    for k in (3, 4):
        assert cj(os.path.join(batch, f"seed{k}"))["policy_delay"] == 2
