"""VecTrainer(actor_hold=N): for the first N learner calls the actor's step size handed to the update is 0 -- the actor's bits stay, its
Adam moments and the critic move -- and the configuration's afterwards; without the argument (and without a warm start) the trainer
calls neither entry point of the fit and hands every update the configuration's step size."""
import pytest
import torch

from avddpg_amd import config, scenarios, trainer, vec
from tests.gpu_util import need_gpu

pytestmark = pytest.mark.gpu

GATE = 64  # steps before the first learner call: the replay gate opens after the 65th add (batch_size 64)
# the position of the actor's step size among an update entry point's arguments
LR_ARG = {"avd_adam_polyak_f32": 10, "avd_adam_polyak_guarded_f32": 10, "avd_adam_polyak_intra_f32": 13, "avd_learn_update_f32": 16,
          "avd_learn_update_act_f32": 16}


def _trainer(engine, **kw):
    if engine == "per_agent_fused":  # nofrl: learn + Adam + Polyak in one kernel (avd_learn_update_act_f32), theta ping-pong
        conf = config.Config(num_platoons=2, pl_size=3, buffer_size=128)
        return trainer.VecTrainer(conf, rng="device", auto_reset="platoon", fused_update=True, seed=4, **kw)
    conf = config.Config(num_platoons=8, pl_size=3, buffer_size=128, fed_method="interfrl", weighted_average_enabled=False)
    return trainer.VecTrainer(conf, rng="device", auto_reset=True, seed=5, shared_engine="fused3", **kw)


@pytest.mark.parametrize("engine", ["per_agent_fused", "fused3"])
def test_actor_block_is_bitwise_constant_under_the_hold_and_moves_after_it(engine):
    need_gpu()
    vt = _trainer(engine, actor_hold=3)
    vt.reset_episode()
    for _ in range(GATE):
        vt.step()
    assert vt.learner_calls == 0 and not vt.agents.step.any()
    A = vt.agents.lay.actor_size
    snap = lambda: (vt.agents.theta[:, :A].clone(), vt.agents.theta[:, A:].clone(), vt.agents.m[:, :A].clone())
    actor0, critic, m_actor = snap()
    for call_no in (1, 2, 3):
        vt.step()
        a, c, m = snap()
        assert vt.learner_calls == call_no and vt.agents.actor_lr == 0.0
        assert torch.equal(a, actor0), call_no  # w - 0 * x = w
        assert not torch.equal(c, critic) and not torch.equal(m, m_actor), call_no  # the critic learns; the actor's moments accumulate
        critic, m_actor = c, m
    assert int(vt.agents.step.max()) == 3 and torch.isfinite(vt.agents.theta).all()
    vt.step()  # the fourth learner call: the configuration's step size again
    torch.cuda.synchronize()
    assert vt.agents.actor_lr == vt.conf.actor_lr
    assert not torch.equal(vt.agents.theta[:, :A], actor0)


@pytest.mark.parametrize("engine", ["per_agent_fused", "fused3"])
def test_without_the_arguments_nothing_new_is_called_and_the_configured_step_size_is_passed(engine, monkeypatch):
    need_gpu()
    seen = []
    real = vec.call

    def recorder(name, *args):
        seen.append((name, args))
        return real(name, *args)

    monkeypatch.setattr(vec, "call", recorder)
    monkeypatch.setattr(trainer, "call", recorder)
    vt = _trainer(engine)
    assert vt.warm_start is None and vt.actor_hold == 0
    vt.reset_episode()
    for _ in range(GATE + 3):
        vt.step()
    torch.cuda.synchronize()
    names = [n for n, _ in seen]
    assert "avd_actor_clone_f32" not in names and "avd_clone_sample_f32" not in names
    updates = [(n, a) for n, a in seen if n in LR_ARG]
    assert len(updates) == 3 and vt.learner_calls == 3
    for n, a in updates:
        assert a[LR_ARG[n]] == vt.conf.actor_lr, (n, a[LR_ARG[n]])
    assert vt.agents._actor_lr is None  # nothing was set: the property reads the configuration


def test_warm_start_runs_once_before_the_first_update_and_composes_with_the_hold():
    """VecTrainer(warm_start=..., actor_hold=...): the first step runs the fit (every platoon's actors the fitted ones, Adam state zero);
    a second fit, or one after an update, is refused; under the hold the fitted actors stay."""
    need_gpu()
    spec = scenarios.WarmStart(kp=2, kv=1, steps=10)
    vt = _trainer("per_agent_fused", warm_start=spec, actor_hold=2)
    vt.reset_episode()
    th0 = vt.agents.theta.clone()
    A, M = vt.agents.lay.actor_size, vt.M
    vt.step()
    assert vt.warm_start_losses is not None and vt.warm_start_losses.shape == (M,)
    fitted = vt.agents.theta.clone()
    assert not torch.equal(fitted[:, :A], th0[:, :A]) and torch.equal(fitted[:, A:], th0[:, A:])
    assert torch.equal(fitted[:M], fitted[M:]) and torch.equal(vt.agents.theta_t, fitted)
    with pytest.raises(ValueError, match="already been fitted"):
        vt.fit_warm_start()
    for _ in range(GATE + 1):
        vt.step()
    assert vt.learner_calls == 2 and torch.equal(vt.agents.theta[:, :A], fitted[:, :A])
    late = _trainer("per_agent_fused", warm_start=spec)
    late.reset_episode()
    late.warm_start_losses = ()  # (as if fitted: run to the first update without the fit)
    for _ in range(GATE + 1):
        late.step()
    late.warm_start_losses = None
    with pytest.raises(ValueError, match="before the first update"):
        late.fit_warm_start()
