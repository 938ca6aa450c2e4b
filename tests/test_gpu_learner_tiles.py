"""The per-agent exact-f32 learn kernels -- cen::learn_kernel_c (csrc/cen.hip, the shipped path of the centralized shapes) and
lean::learn_kernel_l (csrc/lean.hip, the shipped path at the reference widths) -- tile by tile against the float64 oracle.

tests/test_gpu_mlp.py and tests/test_gpu_general_shapes.py hold these kernels to GRAD_TOL = 1e-4 of a whole tensor's max, some 100 x
their real error, and a work item whose values are small passes that however wrong it is. Here every tile of the kernel's own plan
(cen: gemm_dw's 32 x 32 items, l1_grads' 16 x 16 tiles, out_bwd's and gemm_dx_bn's 16-wide tiles, labelled with the wave that made
them) has a limit of its own, 4 x what float32 evaluations of the oracle in four summation orders miss the float64 oracle by in that
tile (tests/tile_oracle.py; tests/test_learner_tiles_cpu.py checks the rule itself; tile_oracle.FALLBACK: the one-element b3 gradients
at A = 1, where that is one scalar's luck, keep GRAD_TOL). Cases cen3, cen5, lean4, lean3 x {plain, ladder:
tile scales spread over 1 : 50 and more, hp: gamma 0.9 and action_high 1.5} x {5 agents on per-agent sets, 7 agents on 3 shared sets}; the
gradient slab is prefilled with NaN, every element outside the logical tensors has to come back exactly 0.
The same cases run on gen::learn_kernel_g (the diagnostic build's AVD_LEARN_GENERAL) under the same rule: the control that tells a
wrong kernel from ill-conditioned inputs. cen only: the STATS instantiation (learn_update) leaves the same gradient bits, and an
agent's row does not depend on where it sits in the launch (the scratch parked in the gradient row and the critic's snapshot stay
inside their workgroup). The TILE lines (-s) give, per tensor, the worst error / limit with its tile's label, the float32 evaluations'
worst error and the kernel's, both of the tensor's max. Measured figures: docs/learner_tile_parity.md."""
import numpy as np
import pytest
import torch

from tests import tile_oracle as to
from tests.gpu_util import need_gpu, t
from tests.test_gpu_general_shapes import _logical_mask
from tests.test_gpu_mlp import _perturbed_group

pytestmark = pytest.mark.gpu

CASE_VARIANTS = [pytest.param(c.name, v, id=f"{c.name}-{v}") for c in to.CASES for v in to.VARIANTS]
CEN_VARIANTS = [pytest.param(c.name, v, id=f"{c.name}-{v}") for c in to.CASES if c.kernel == "cen" for v in to.VARIANTS]


def _setup(name, variant, set_mod):
    """(group, conditioned batch on the device); the group's four slabs are the host tables of tests/tile_oracle.py bit for bit --
    plain and hp straight from _perturbed_group (the host half restates its draws), the ladder written through set_weights."""
    c = to.CASE[name]
    _, hconf, th, st, tht, stt = to.slabs(name, variant, set_mod)
    conf, grp = _perturbed_group(len(th), S=c.S, seed=to.group_seed(name, set_mod), A=c.A, hidd_mult=c.hidd_mult, **to.conf_kw(name, variant))
    assert (conf.gamma, conf.action_high, grp.high) == (hconf.gamma, hconf.action_high, hconf.action_high)
    if variant == "ladder":
        for k in range(len(th)):
            an, cn, tan, tcn = to.nets(name, variant, set_mod, k, np.float32)
            grp.set_weights(k, "actor", an), grp.set_weights(k, "critic", cn)
            grp.set_weights(k, "actor", tan, target=True), grp.set_weights(k, "critic", tcn, target=True)
    for dev, host in ((grp.theta, th), (grp.stats, st), (grp.theta_t, tht), (grp.stats_t, stt)):
        assert np.array_equal(dev.cpu().numpy(), host), (name, variant, set_mod)
    return grp, tuple(t(x.copy()) for x in to.batch(name, variant, set_mod))  # (the cached batch is read-only)


def _learn(grp, dev, set_mod):
    n = dev[0].shape[0]
    grads = torch.full((n, grp.lay.theta_size), float("nan"), device="cuda")
    losses = torch.full((n, 2), float("nan"), device="cuda")
    grp.learn(*dev, set_mod, grads=grads, losses=losses)
    torch.cuda.synchronize()
    return grads, losses


def _check(name, variant, set_mod, grp, grads, losses, worst, kernel):
    """The requirements on one launch's slab; returns what missed them."""
    g, lo = grads.cpu().numpy(), losses.cpu().numpy().astype(np.float64)
    mask = _logical_mask(grp)
    assert np.array_equal(np.flatnonzero(mask), to.plan(name).logical)
    bad = []
    if not np.isfinite(g).all():
        bad.append((set_mod, "non-finite slab elements", int((~np.isfinite(g)).sum())))
    if not np.all(g[:, ~mask] == 0.0):
        bad.append((set_mod, "non-zero outside the logical tensors", np.argwhere(g[:, ~mask] != 0.0)[:4].tolist()))
    for v in range(len(g)):
        ref = to.reference(name, variant, set_mod, v)  # (agent v against its set v % set_mod: the reference is of that set)
        to.report(name, g[v], ref, worst)
        bad += [(set_mod, v) + x for x in to.violations(name, g[v], ref, kernel)]
        if not np.all(np.abs(lo[v] - ref.losses) <= ref.loss_tol):
            bad.append((set_mod, v, "losses", lo[v].tolist(), ref.losses.tolist(), ref.loss_tol.tolist()))
    return bad


def _print(name, variant, kernel, worst):
    for n_, m in to.GROUPS:
        print(f"NUDGED {name} {variant} set_mod={m}: rows per agent {to.nudged_rows(name, variant, m).sum(axis=1).tolist()}")
    for tensor in to.NAMES:
        ratio, label, e32, err = worst[tensor]
        fb = " FALLBACK" if (kernel, tensor) in to.FALLBACK and to.CASE[name].A == 1 else ""
        print(f"TILE {name} {variant} {kernel} {tensor}: err/limit {ratio:.3f} at [{label}] e32 {e32:.3e} kernel {err:.3e} (of the tensor's max){fb}")


def _run(name, variant, kernel):
    worst, bad, slabs = {}, [], []
    for _, set_mod in to.GROUPS:
        grp, dev = _setup(name, variant, set_mod)
        grads, losses = _learn(grp, dev, set_mod)
        bad += _check(name, variant, set_mod, grp, grads, losses, worst, kernel)
        slabs.append(grads)
    _print(name, variant, kernel, worst)
    assert bad == [], (len(bad), bad[:12])
    return slabs


@pytest.mark.parametrize("name,variant", CASE_VARIANTS)
def test_shipped_learn_kernel_meets_the_tile_rule(name, variant):
    """grp.learn of the shipped library (cen::learn_kernel_c / lean::learn_kernel_l), 5 agents on per-agent sets and 7 agents on 3
    shared sets, the gradient slab prefilled with NaN: the whole slab finite, every tile of every agent within its limit, every element
    outside the logical tensors exactly 0, both losses within 1e-6 relative (or 4 x the float32 evaluations' own loss error)."""
    need_gpu()
    _run(name, variant, to.CASE[name].kernel)


@pytest.mark.parametrize("name,variant", CASE_VARIANTS)
def test_general_kernel_meets_the_same_rule_on_the_same_cases(name, variant, diag_lib, monkeypatch):
    """The control: gen::learn_kernel_g (csrc/mlp.hip) through the diagnostic build's AVD_LEARN_GENERAL, same cases, same rule. It did
    run: its slab differs from the shipped kernel's in some bits."""
    need_gpu()
    monkeypatch.setenv("AVD_LEARN_GENERAL", "1")
    general = _run(name, variant, "general")
    monkeypatch.delenv("AVD_LEARN_GENERAL")
    grp, dev = _setup(name, variant, 0)
    shipped, _ = _learn(grp, dev, 0)
    assert not torch.equal(shipped, general[0]) and torch.isfinite(shipped).all()


@pytest.mark.parametrize("name,variant", CEN_VARIANTS)
def test_cen_stats_instantiation_leaves_the_gradient_bits_of_learn(name, variant):
    """learn_kernel_c<S, A, true> (the learn half of learn_update) from the same state, its gradient scratch prefilled with NaN: the
    scratch equals learn's slab bit for bit (so it meets the tile rule), losses too; padding exactly 0."""
    need_gpu()
    grp, dev = _setup(name, variant, 0)
    grads, losses = _learn(grp, dev, 0)
    scratch = torch.full_like(grads, float("nan"))
    losses_u = torch.full_like(losses, float("nan"))
    theta0 = grp.theta.clone()
    grp.learn_update(*dev, scratch, losses=losses_u)
    torch.cuda.synchronize()
    assert torch.isfinite(scratch).all() and torch.equal(scratch, grads) and torch.equal(losses_u, losses)
    mask = torch.from_numpy(_logical_mask(grp)).cuda()
    assert bool((scratch[:, ~mask] == 0).all()) and not torch.equal(grp.theta, theta0)
    assert torch.equal(grp.theta[:, ~mask], theta0[:, ~mask])


@pytest.mark.parametrize("name,variant", CEN_VARIANTS)
def test_cen_agent_row_does_not_depend_on_its_position(name, variant):
    """Agent 0's batch and weights copied to agent 4: bit-identical slab rows in one launch, and a launch of agent 0 alone gives the same
    bits -- the activations parked in the gradient row and the critic's layer-2 snapshot do not leak between workgroups."""
    need_gpu()
    grp, dev = _setup(name, variant, 0)
    for x in (grp.theta, grp.stats, grp.theta_t, grp.stats_t) + tuple(dev):
        x[4].copy_(x[0])
    grads, losses = _learn(grp, dev, 0)
    assert torch.isfinite(grads).all() and torch.equal(grads[4], grads[0]) and torch.equal(losses[4], losses[0])
    assert not torch.equal(grads[1], grads[0])
    alone, losses1 = _learn(grp, tuple(x[0:1].contiguous() for x in dev), 0)
    assert torch.equal(alone[0], grads[0]) and torch.equal(losses1[0], losses[0])
    assert to.violations(name, grads[0].cpu().numpy(), to.reference(name, variant, 0, 0), "cen") == []
