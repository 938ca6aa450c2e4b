"""The warm start's two kernels and the fit around them on the GPU: avd_actor_clone_f32 (csrc/mlp.hip: gen::actor_clone_kernel) against
the float64 oracle over the shapes of tests/test_gpu_general_shapes.py that reach distinct code, avd_clone_sample_f32 (csrc/clone.hip)
bit for bit against tests/clone_oracle.sample, AgentGroup.clone_fit's mechanics, and a whole 500-step fit beside the float32 oracle
fit on the same draws.

Tolerances are tests/test_gpu_mlp.py's: GRAD_TOL = 1e-4 of each tensor's max (or 4 x the float32 oracle's own error where that is
larger), FWD_TOL = 2e-5 on the loss. Every comparison stands on conditions on its inputs taken from the oracle alone."""
import numpy as np
import pytest
import torch

from avddpg_amd import _hip, config, evaluator, scenarios, vec
from tests import clone_oracle
from tests.gpu_util import need_gpu, t
from tests.test_gpu_general_shapes import SHAPES, _group, _logical_mask, _x_scale
from tests.test_gpu_mlp import FWD_TOL, GRAD_TOL, _nets, _relerr

pytestmark = pytest.mark.gpu

_BY_ID = {p.id: p.values[0] for p in SHAPES}
CLONE_SHAPES = [pytest.param(_BY_ID[i], id=i) for i in (
    "ref-4x1-general", "ref-3x1-general",  # the reference widths, Model B and Model A
    "min-1x1-16.32.16",                    # every minimum
    "ragged-5x2-48.32.16",                 # K not a multiple of 4, A = 2
    "padded-3x1-100.50.20",                # padded to 112/64/32
    "st16lo-21x3-128.256.32")]             # H2 at its maximum, A = 3, l1_fwd_t<16>
HIGH = 2.5


def _clone(grp, s, u, grads, losses):
    n = s.shape[0]
    _hip.call("avd_actor_clone_f32", grp._layp, n, _hip.ptr(grp.theta), _hip.ptr(grp.stats), _hip.ptr(s), _hip.ptr(u), HIGH, _hip.ptr(grads),
              _hip.ptr(losses), _hip.stream_handle())
    torch.cuda.synchronize()


@pytest.mark.parametrize("sh", CLONE_SHAPES)
def test_gradients_match_the_float64_oracle(sh):
    """Three sets per shape: all ten actor gradient tensors and the loss against the float64 oracle; the critic block and every slab
    element outside the logical actor tensors exactly 0; theta and stats untouched; permuting the sets permutes the rows bit for bit."""
    need_gpu()
    n = 3
    conf, grp = _group(sh, n, seed=301)
    lay = grp.lay
    rs = np.random.RandomState(302)
    s = (rs.normal(0, 1.5, size=(n, 64, sh.S)) * _x_scale(sh.S)).astype(np.float32)
    u = rs.uniform(-HIGH, HIGH, size=(n, 64, sh.A)).astype(np.float32)
    th0, st0 = grp.theta.clone(), grp.stats.clone()
    grads = torch.full((n, lay.theta_size), 7.0, device="cuda")
    losses = torch.full((n,), 7.0, device="cuda")
    _clone(grp, t(s), t(u), grads, losses)
    assert torch.equal(grp.theta, th0) and torch.equal(grp.stats, st0)
    assert torch.isfinite(grads).all()
    worst, worst_loss = 0.0, 0.0
    for v in range(n):
        a64, a32 = _nets(grp, v, np.float64)[0], _nets(grp, v, np.float32)[0]
        ref, loss, (_, p1, _, p2, _, th) = clone_oracle.grads(a64, s[v], u[v], HIGH)
        r32, _, _ = clone_oracle.grads(a32, s[v], u[v], HIGH)
        # the inputs bite (oracle alone)
        for name, p in (("hidden 1", p1), ("hidden 2", p2)):
            frac = float(np.mean(p > 0))
            assert 0.2 <= frac <= 0.8, (v, name, frac)
        assert float(np.mean(np.all(np.abs(th) < 0.99, axis=1))) >= 0.5, v
        assert float(np.mean(np.abs(th * HIGH - u[v]))) > 0.1 * HIGH, v
        got = grp.grads_as_lists(grads[v])[1]
        assert [g.shape for g in got] == [r.shape for r in ref]
        for i, (g, r, r3) in enumerate(zip(got, ref, r32)):
            assert np.max(np.abs(r)) > 1e-8, (v, i, "a gradient tensor of the oracle is trivial")
            e, e32 = _relerr(g, r), _relerr(r3, r)
            worst = max(worst, e)
            assert e <= max(GRAD_TOL, 4 * e32), (v, i, e, e32)
        el = abs(float(losses[v]) - loss) / max(1.0, abs(loss))
        worst_loss = max(worst_loss, el)
        assert el <= FWD_TOL, (v, float(losses[v]), loss)
    print(f"CLONE grads S={sh.S} A={sh.A} {sh.padded}: worst relerr {worst:.3g}, loss {worst_loss:.3g}")
    g = grads.cpu().numpy()
    mask = _logical_mask(grp)
    assert np.all(g[:, lay.actor_size:] == 0.0)  # the critic block: zeros, so the slab goes straight into Adam
    assert np.all(g[:, :lay.actor_size][:, ~mask[:lay.actor_size]] == 0.0)  # padded units and alignment gaps
    assert np.mean(g[:, :lay.actor_size][:, mask[:lay.actor_size]] != 0.0) > 0.3
    # sets do not read each other's rows
    perm = [2, 0, 1]
    grp.theta.copy_(th0[perm]), grp.stats.copy_(st0[perm])
    g2 = torch.full_like(grads, 7.0)
    l2 = torch.full_like(losses, 7.0)
    _clone(grp, t(s[perm]), t(u[perm]), g2, l2)
    assert torch.equal(g2, grads[perm]) and torch.equal(l2, losses[perm])
    # losses = NULL is accepted and changes nothing
    g3 = torch.full_like(grads, 7.0)
    sp, up = t(s[perm]), t(u[perm])
    _hip.call("avd_actor_clone_f32", grp._layp, n, _hip.ptr(grp.theta), _hip.ptr(grp.stats), _hip.ptr(sp), _hip.ptr(up), HIGH, _hip.ptr(g3), None,
              _hip.stream_handle())
    torch.cuda.synchronize()
    assert torch.equal(g3, g2)


def _sample(n_sets, S, M, gains, box, model_a, key, counter, seeds=None):
    s = torch.full((n_sets, 64, S), 7.0, device="cuda")
    u = torch.full((n_sets, 64, 1), 7.0, device="cuda")
    d_seeds = None if seeds is None else vec.seed_table(seeds, "cuda")[1]
    d_gains, d_box = t(gains), t(box)  # (held until the launch has run)
    _hip.call("avd_clone_sample_f32", n_sets, S, M, _hip.ptr(d_gains), _hip.ptr(d_box), -HIGH, HIGH, int(model_a), int(key), int(counter),
              _hip.ptr(d_seeds), 1 if seeds is None else len(seeds), _hip.ptr(s), _hip.ptr(u), _hip.stream_handle())
    torch.cuda.synchronize()
    return s.cpu().numpy(), u.cpu().numpy()


TABLE = np.array([[2, 1, 0.25, 0.5], [1, 0.5, -0.1, 0.3], [3, 2, 0, 0]], np.float32)  # one row per vehicle, M = 3
BOX = np.array([1.5, 1.5, 1.0, 1.0], np.float32)


@pytest.mark.parametrize("S,model_a,counter,seeds,n_sets", [
    (4, False, 0, None, 6),      # two platoons of per-agent sets
    (4, False, 5, None, 3),      # another fit step
    (3, True, 0, None, 6),       # Model A: three components, kf ignored
    (3, True, 5, None, 3),
    (4, False, 2, (3, 5), 12),   # a seed batch: two platoons x two experiments x three vehicles
    (3, True, 2, (3, 5), 6),
])
def test_sampler_is_bitwise_the_oracle(S, model_a, counter, seeds, n_sets):
    need_gpu()
    key = 9
    s, u = _sample(n_sets, S, 3, TABLE, BOX, model_a, key, counter, seeds)
    rs, ru = clone_oracle.sample(n_sets, S, 3, TABLE, BOX, -HIGH, HIGH, model_a, key, counter, seeds)
    assert np.array_equal(s, rs) and np.array_equal(u, ru)
    assert len(np.unique(s[:3])) > 0.9 * s[:3].size  # (draws, not a constant)
    if seeds is not None:  # experiment e of the batch draws what its solo run draws
        for e, k in enumerate(seeds):
            solo = _sample(3, S, 3, TABLE, BOX, model_a, k, counter)
            assert np.array_equal(s[3 * e:3 * e + 3], solo[0]) and np.array_equal(u[3 * e:3 * e + 3], solo[1])


def test_sampler_clip_binds_on_part_of_the_rows_for_the_untuned_law():
    """Gains (2, 1, 0, 0) in the default box: between 10 % and 90 % of the targets sit on the clip (on the oracle's draws), and the
    device agrees with them bit for bit."""
    need_gpu()
    g = np.tile(np.float32([2, 1, 0, 0]), (3, 1))
    rs, ru = clone_oracle.sample(3, 4, 3, g, BOX, -HIGH, HIGH, False, 1, 0)
    frac = float(np.mean(np.abs(ru) == HIGH))
    assert 0.1 <= frac <= 0.9, frac
    s, u = _sample(3, 4, 3, g, BOX, False, 1, 0)
    assert np.array_equal(s, rs) and np.array_equal(u, ru)


def _fit_group(n_sets, conf, **kw):
    grp = vec.AgentGroup(n_sets, 4, 1, conf, **kw)
    # statistics off their initial values (the same for every set count), so that "unchanged" says something
    grp.stats.add_(0.125)
    grp.stats_t.copy_(grp.stats)
    return grp


def test_fit_mechanics():
    """AgentGroup.clone_fit, 20 steps, M = 3, two platoons of per-agent sets: the critics, the statistics and the critics' targets keep
    their bits; every target equals its online net; the Adam state is zero; both platoons hold the same sets (the ping-pong slab too);
    and a seed batch (3, 5) is the two solo fits, bit for bit."""
    need_gpu()
    M, P = 3, 2
    conf = config.Config(pl_size=M, num_platoons=P)
    spec = scenarios.WarmStart(kp=2, kv=1, steps=20)
    solo = {}
    for k in (3, 5):
        grp = _fit_group(P * M, conf, seed=k)
        grp.theta_alt = grp.theta.clone()
        A = grp.lay.actor_size
        th0, tht0, st0, stt0 = grp.theta.clone(), grp.theta_t.clone(), grp.stats.clone(), grp.stats_t.clone()
        log = torch.zeros(20, M, device="cuda")
        losses = grp.clone_fit(spec, M=M, seed=k, loss_log=log)
        torch.cuda.synchronize()
        assert losses.shape == (M,) and np.array_equal(losses, log[-1].cpu().numpy())
        assert float(log[-1].mean()) < float(log[0].mean())  # 20 steps of size 1e-3: it has begun to learn
        assert torch.equal(grp.theta[:, A:], th0[:, A:]) and torch.equal(grp.theta_t[:, A:], tht0[:, A:])
        assert torch.equal(grp.stats, st0) and torch.equal(grp.stats_t, stt0)
        assert not torch.equal(grp.theta[:, :A], th0[:, :A])
        assert torch.equal(grp.theta_t, grp.theta) and torch.equal(grp.theta_alt, grp.theta)
        assert not grp.m.any() and not grp.v.any() and not grp.step.any()
        assert torch.equal(grp.theta[:M], grp.theta[M:]) and torch.equal(grp.theta_t[:M], grp.theta_t[M:])
        assert not torch.equal(grp.theta[0, :A], grp.theta[1, :A])  # (each vehicle index draws its own rows)
        solo[k] = grp
    batch = _fit_group(P * 2 * M, conf, seeds=(3, 5), seed_block=M)
    T = batch.lay.theta_size
    for e, k in enumerate((3, 5)):  # (the same start as the solo groups: statistics included)
        assert torch.equal(batch.stats.view(P, 2, M, -1)[:, e], solo[k].stats.view(P, M, -1))
    losses = batch.clone_fit(spec, seeds=(3, 5), M=M)
    torch.cuda.synchronize()
    assert losses.shape == (2 * M,)
    for e, k in enumerate((3, 5)):
        for name in ("theta", "theta_t"):
            assert torch.equal(getattr(batch, name).view(P, 2, M, T)[:, e], getattr(solo[k], name).view(P, M, T)), (k, name)
    assert not batch.m.any() and not batch.v.any() and not batch.step.any()
    # shared sets: n_sets == E * M, nothing to copy
    shared = _fit_group(M, conf, seed=3)
    shared.clone_fit(spec, M=M, seed=3)
    assert torch.equal(shared.theta, solo[3].theta[:M]) and torch.equal(shared.theta_t, shared.theta)


def test_fit_end_to_end_beside_the_float32_oracle():
    """500 steps, L = 3, reference widths, gains (2, 1, 0, 0), draw seed clone_oracle.STANDARD_SEED = 1, beside the float32 oracle fit on
    the same draws. Measured on the oracle (CPU): first-step loss 2.85 (mean of the three actors), mean loss of the last 50 steps
    0.0041077, evaluator score -3.142, the law's own -2.952 (run_linear: -2.952; gap 0.19). Measured on the MI355X: first-step loss
    2.8458 (oracle 2.8458), mean loss of the last 50 steps 0.0041077 (oracle 0.0041077: five equal digits), score -3.142 (oracle
    -3.142). The test prints the line."""
    need_gpu()
    r = clone_oracle.standard_fit("float32")
    conf, spec, L = r["conf"], r["spec"], 3
    ref_first, ref_last = float(np.mean(r["losses"][:, 0])), float(np.mean(r["losses"][:, -50:]))
    law = float(evaluator.run_linear(conf, [scenarios.LinearLaw("law", kp=2, kv=1)]).scores[0, 0, 0])
    # conditions on the oracle alone
    assert ref_last <= 0.01 and 100 * ref_last <= ref_first
    assert abs(r["score"] - law) <= 0.25, (r["score"], law)
    grp = vec.AgentGroup(L, 4, 1, conf, seed=clone_oracle.STANDARD_SEED)
    log = torch.zeros(spec.steps, L, device="cuda")
    grp.clone_fit(spec, M=L, seed=clone_oracle.STANDARD_SEED, loss_log=log)
    got = log.cpu().numpy().T  # [L, steps]
    got_last = float(np.mean(got[:, -50:]))
    score = float(evaluator.run_many(conf, grp, [0])[0][0, 0])
    print(f"CLONE fit: first loss gpu {float(np.mean(got[:, 0])):.5g} oracle {ref_first:.5g}; last-50 loss gpu {got_last:.5g} oracle "
          f"{ref_last:.5g}; score gpu {score:.3f} oracle {r['score']:.3f} law {law:.3f}")
    assert abs(float(np.mean(got[:, 0])) - ref_first) <= FWD_TOL * ref_first * 10  # (step 1: the same weights, the same rows)
    assert abs(got_last - ref_last) <= 0.10 * ref_last
    assert abs(score - r["score"]) <= 0.05
