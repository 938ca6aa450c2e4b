"""VecTrainer(anchor=...) and `tr --anchor SPEC` on the GPU, 8 platoons x 3 vehicles on the fused3 engine: the trainer hands the sampled
batch, the gain table and weight_at(call) to avd_learn_set_split_anchor_f16x3; weight 0 trains what the run without the flag trains,
bit for bit; a decay reaches the entry point as weight_at says; a seed batch's experiment is its solo run within the engine's tolerance;
the anchor pulls the actors towards the law (two runs compared, no threshold); and the CLI end to end."""
import json
import os

import numpy as np
import pytest
import torch

from avddpg_amd import config, scenarios, trainer, vec
from tests.gpu_util import need_gpu
from tests.test_gpu_residual import _esim_rewards, _files, _run

pytestmark = pytest.mark.gpu

P, L = 8, 3
GATE = 65  # the replay gate: the first learner call is step 65's (strictly more than batch_size rows)


def _conf(**kw):
    return config.Config(**{**dict(num_platoons=P, pl_size=L, buffer_size=200, fed_method="interfrl"), **kw})


def _vt(anchor=None, seed=5, **kw):
    if "seeds" not in kw:
        kw["seed"] = seed
    vt = trainer.VecTrainer(_conf(), rng="device", auto_reset="platoon", shared_engine="fused3", anchor=anchor, **kw)
    vt.reset_episode()
    return vt


def _steps(vt, n):
    for _ in range(n):
        vt.step()
    torch.cuda.synchronize()
    return vt


def test_a_step_hands_the_sampled_batch_the_table_and_the_weight_to_the_entry_point(monkeypatch):
    need_gpu()
    spec = scenarios.Anchor(table=[[2, 1, 0, 0], [1.5, 1.2, -0.1, 0.3], [2.5, 0.8, 0, 0.5]], weight=4.0)
    vt = _steps(_vt(spec), GATE - 1)
    assert vt.learner_calls == 0 and bool((vt.anchor_losses() == 0).all()) and vt.anchor_loss_first is None
    seen = {}
    real = vt.agents.learn_set_split_anchor

    def spy(s, a, r, s2, n, gains, weight, anchor_loss, **kw):
        seen.update(batch=[x.clone() for x in (s, a, r, s2)], n=n, gains=gains.clone(), weight=weight,
                    aw=None if kw.get("agent_weight") is None else kw["agent_weight"].clone(),
                    theta=[x.clone() for x in (vt.agents.theta, vt.agents.stats, vt.agents.theta_t, vt.agents.stats_t)])
        return real(s, a, r, s2, n, gains, weight, anchor_loss, **kw)

    monkeypatch.setattr(vt.agents, "learn_set_split_anchor", spy)
    vt.step()
    torch.cuda.synchronize()
    assert vt.learner_calls == 1 and seen["n"] == P * L and seen["weight"] == 4.0 == vt.anchor_weight
    assert np.array_equal(seen["gains"].cpu().numpy(), spec.gains(L))
    # a direct call on the same batch from the same weights
    grp = vec.AgentGroup(L, 4, 1, _conf())
    for dst, src in zip((grp.theta, grp.stats, grp.theta_t, grp.stats_t), seen["theta"]):
        dst.copy_(src)
    al = torch.zeros(L, device="cuda")
    g = grp.learn_set_split_anchor(*seen["batch"], P * L, seen["gains"], 4.0, al, agent_weight=seen["aw"])
    torch.cuda.synchronize()
    assert torch.equal(g, vt.set_grads) and torch.equal(al, vt.anchor_losses()) and bool((al > 0).all())
    assert torch.equal(vt.anchor_loss_first, al)


def test_weight_zero_trains_what_the_run_without_an_anchor_trains():
    need_gpu()
    plain = _steps(_vt(None), GATE + 100)
    zero = _steps(_vt(scenarios.Anchor(kp=2, kv=1, weight=0.0)), GATE + 100)
    assert plain.anchor is None and plain.anchor_loss is None and plain.anchor_gains is None
    assert plain.learner_calls == zero.learner_calls == 101
    for name in ("theta", "theta_t", "stats", "stats_t", "m", "v"):
        assert torch.equal(getattr(plain.agents, name), getattr(zero.agents, name)), name
    assert torch.equal(plain.env.x, zero.env.x)
    assert bool((zero.anchor_losses() > 0).all())  # still a diagnostic
    with pytest.raises(ValueError, match="anchor_losses needs"):
        plain.anchor_losses()


def test_a_decay_reaches_the_entry_point_as_weight_at_says(monkeypatch):
    need_gpu()
    N = 20
    spec = scenarios.Anchor(kp=2, kv=1, weight=0.3, decay=N)
    vt = _steps(_vt(spec), GATE - 1)
    handed = []
    real = vec.call
    monkeypatch.setattr(vec, "call", lambda name, *a: (handed.append(a[23]) if name == "avd_learn_set_split_anchor_f16x3" else None,
                                                        real(name, *a))[1])
    _steps(vt, N + 2)
    assert len(handed) == N + 2
    for call in (0, N // 2, N, N + 1):
        assert handed[call] == spec.weight_at(call), call
    assert handed[0] == float(np.float32(0.3)) and handed[N // 2] == float(np.float32(0.15)) and handed[N] == 0.0
    assert bool((vt.anchor_losses() > 0).all())  # the entry point is still called at weight 0


def test_a_seed_batch_experiment_equals_its_solo_run():
    """Up to the first learner call bit for bit; the first anchored learn within the fused3 engine's tolerance of the solo call's
    (2e-5 of the slab's max: tests/test_gpu_seed_batch.py -- its reduction tree depends on the set count)."""
    need_gpu()
    seeds = (4, 8)
    spec = scenarios.Anchor(table=[[2, 1, 0, 0], [1.5, 1.2, -0.1, 0.3], [2.5, 0.8, 0, 0.5]], weight=4.0)
    batch = _steps(_vt(spec, seeds=seeds), GATE)
    assert batch.learner_calls == 1 and batch.anchor_losses().shape == (len(seeds) * L,)
    for e, k in enumerate(seeds):
        solo = _steps(_vt(spec, seed=k, init_seed=k), GATE)
        mine, ref = batch.set_grads[e * L:(e + 1) * L], solo.set_grads
        assert (mine - ref).abs().max().item() <= 2e-5 * ref.abs().max().item(), e
        al, rl = batch.anchor_losses()[e * L:(e + 1) * L], solo.anchor_losses()
        assert (al - rl).abs().max().item() <= 1e-5 * rl.abs().max().item(), e
    assert not torch.equal(batch.anchor_losses()[:L], batch.anchor_losses()[L:])


def test_the_anchor_pulls_the_actors_towards_the_law():
    """The same seed, 200 learner calls, weight 10 against weight 0: the anchored run ends with the smaller mean anchor loss."""
    need_gpu()
    runs = {w: _steps(_vt(scenarios.Anchor(kp=2, kv=1, weight=w)), GATE + 199) for w in (10.0, 0.0)}
    assert runs[10.0].learner_calls == runs[0.0].learner_calls == 200
    first = {w: float(vt.anchor_loss_first.mean()) for w, vt in runs.items()}
    last = {w: float(vt.anchor_losses().mean()) for w, vt in runs.items()}
    print("mean anchor loss, first -> last:", {w: (first[w], last[w]) for w in runs})
    assert first[10.0] == first[0.0]  # the same start
    assert last[10.0] < last[0.0]


TR = ("tr", "--pl_num", str(P), "--pl_size", str(L), "--buffer_size", "500", "--total_time_steps", "200", "--rng", "device", "--episodes",
      "platoon", "--report_every", "100", "--fed_method", "interfrl", "--engine", "fused3", "--seed", "3")


def test_cli_end_to_end(tmp_path, capsys):
    """conf.json's anchor record in the run's directory and in best/, `esim` on both, a seed batch's per-experiment record; a run with
    weight 0 writes the files of the run without the flag, byte for byte, and that run records nothing."""
    need_gpu()
    cj = lambda d: json.load(open(os.path.join(d, "conf.json")))
    run = _run(capsys, *TR, "--anchor", "kp=2,kv=1,weight=10,decay=100", "--keep_best", "100", "--out", str(tmp_path / "a"))[-1]
    j = cj(run)
    rec = dict(j["anchor"])
    assert list(rec) == ["law", "anchor_loss_first", "anchor_loss_last"]
    law = scenarios.Anchor.from_record(rec["law"])
    assert (law.kp, law.kv, law.weight, law.decay, law.source) == (2.0, 1.0, 10.0, 100, "given")
    assert len(rec["anchor_loss_first"]) == len(rec["anchor_loss_last"]) == L
    assert all(np.isfinite(x) and x > 0 for x in rec["anchor_loss_first"] + rec["anchor_loss_last"])
    assert rec["anchor_loss_first"] != rec["anchor_loss_last"]
    bj = cj(os.path.join(run, "best"))
    assert bj["anchor"] == j["anchor"]
    assert len(_esim_rewards(capsys, run, j)) == j["saved_platoons"]
    assert len(_esim_rewards(capsys, os.path.join(run, "best"), bj)) == bj["saved_platoons"]
    # a seed batch: each experiment's own sets in its own conf.json
    batch = _run(capsys, *TR[:-2], "--anchor", "kp=2,kv=1", "--seeds", "3,4", "--out", str(tmp_path / "b"))[-1]
    recs = [dict(cj(os.path.join(batch, f"seed{k}"))["anchor"]) for k in (3, 4)]
    assert all(len(r["anchor_loss_last"]) == L for r in recs) and recs[0]["anchor_loss_last"] != recs[1]["anchor_loss_last"]
    # without the flag: no record; weight 0 writes the same files
    plain = _run(capsys, *TR, "--out", str(tmp_path / "p"))[-1]
    assert "anchor" not in cj(plain)
    zero = _run(capsys, *TR, "--anchor", "kp=2,kv=1,weight=0", "--out", str(tmp_path / "z"))[-1]
    a, b = _files(plain), _files(zero)
    assert set(a) == set(b) and "curve.csv" in a
    for f in a:
        assert a[f] == b[f], f
    assert _files(run)["curve.csv"] != a["curve.csv"]
