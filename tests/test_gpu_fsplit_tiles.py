"""The split set learner (csrc/fsplit.hip, avd_learn_set_split_f16x3, the product library) agent by agent against the float64 oracle.

Every multi-tile test of tests/test_gpu_fsplit*.py compares the mean over a set's P platoons, in which one agent's 64-row tile is 1 / P:
at P ~ 1100 a tile may be 2 % wrong and still meet 2e-5. ``agent_weight`` multiplies an agent's two loss seeds (head_kernel, HEAD_BOTH),
so with weight 1 on the agents of one platoon p0 and 0 elsewhere ONE call returns, for every set at once, 1 / P x learn(that agent's
rows): compared here tensor by tensor with the float64 oracle of those 64 rows under the rule of tests/split_oracle.py --
max(SPLIT_TOL_SMALL, 4 x the float32 NumPy oracle's own error on the same rows); the whole-set mask and general weights at SPLIT_TOL.
The cases give a workgroup 32-33 tiles and mask every ordinal of whole workgroups: both periods of the heads' 5 : 5 : 3 : 3 deal, every
slot and buffer phase of dx, dw and dxa, the tile finished after the loop at odd and even counts (tests/test_split_tiles_cpu.py checks
that, the cap on the rule and that the rule rejects a dropped, a shifted and a once-rounded tile). The mask label names the workgroup,
the ordinal, the head wave pair and position, ordinal % 3 and ordinal & 1. Measured figures: docs/fsplit_tile_parity.md."""
import numpy as np
import pytest
import torch

from tests import bf16_oracle as bo
from tests import split_oracle as so
from tests.gpu_util import need_gpu, t
from tests.test_gpu_mlp import _nets, _perturbed_group

pytestmark = pytest.mark.gpu


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _setup(name):
    """(case, J, P, group, conditioned agent-major host batch, the same on the device); the group's weights are the host tables' bit
    for bit."""
    case = so.case(name, _cus())
    J, P, _ = so.plan(name, _cus())
    conf, grp = _perturbed_group(case.n_sets, S=case.S, seed=case.seed, **bo.case_conf_kw(case))
    for k in case.check:  # the CPU-side references and the tie conditioning are of THESE weights
        for host, devw in zip(bo.case_nets(case, k), _nets(grp, k, np.float64)):
            assert all(np.array_equal(x, y) for x, y in zip(host, devw)), k
    batch = so.batch(name, _cus())
    return case, J, P, grp, batch, tuple(t(x) for x in batch)


def _learn(grp, case, dev, agent_weight):
    g = grp.learn_set_split(*dev, case.n_sets * case.rows // so.B, agent_weight=agent_weight)
    torch.cuda.synchronize()
    return g.clone()


def _platoon_mask(case, P, platoons):
    w = np.zeros((P, case.n_sets), np.float32)  # agent v = p * n_sets + m
    w[list(platoons)] = 1.0
    return w.reshape(-1)


def _named(grp, row):
    cg, ag = grp.grads_as_lists(row)
    return dict(zip(so.NAMES, cg + ag))


def _compare(grp, g, checks, tsz, worst, label):
    """checks: {set: (ref, table)}. -> the rule's violations of one result; keeps per (tile size, tensor) the comparison with the largest
    error / limit."""
    bad = []
    for k, (ref, table) in checks.items():
        got = _named(grp, g[k])
        for tensor in so.NAMES:
            e32, limit = table[tensor]
            err = so.relerr(got[tensor], ref[tensor])
            if err / limit > worst.get((tsz, tensor), (-1.0,))[0]:
                worst[(tsz, tensor)] = (err / limit, e32, err, limit, f"set{k}:{label}")
        bad += [(k, label) + v for v in so.violations(got, ref, table)]
    return bad


def _report(name, worst):
    for (tsz, tensor), (_, e32, err, limit, label) in sorted(worst.items(), key=lambda kv: (str(kv[0][0]), so.NAMES.index(kv[0][1]))):
        print(f"TILE {name} t={tsz} {tensor}: e32 {e32:.3e} kernel {err:.3e} ({label}) ratio {err / max(e32, 1e-300):.2f} tol {limit:.3e}")


@pytest.mark.parametrize("name", so.SPLIT_NAMES)
def test_every_agent_mask_matches_the_float64_oracle_at_the_f32_tolerance(name):
    """One learn_set_split call per mask (the masked platoons one by one, then all ones), the other agents ordinary data; every checked
    set's slab against the float64 oracle of the masked agent of THAT set, every tensor under its own limit, finite results. The TILE
    lines give, per tile size and tensor, the comparison closest to (or furthest beyond) its limit over the sets and masks.
    The whole-set mask is also agent_weight = 1 == agent_weight = None: x * 1.0f is exact and the partials are summed in a fixed
    order, so the two slabs are bit-identical."""
    need_gpu()
    case, J, P, grp, batch, dev = _setup(name)
    ms, per = so.reference(name, _cus())
    worst, bad, ones = {}, [], None
    for i, (label, tsz, lo, hi) in enumerate(ms):
        g = _learn(grp, case, dev, t(_platoon_mask(case, P, range(P) if tsz == "whole" else [lo // so.B])))
        if not torch.isfinite(g).all():
            bad.append((label, "non-finite slab"))
        bad += _compare(grp, g, {k: items[i] for k, items in per.items() if items[i] is not None}, tsz, worst, label)
        if tsz == "whole":
            ones = g
    print(f"PLAN {name}: CUs {_cus()} J {J} P {P} sets {case.n_sets} checked {case.check} whole-set mask on {so.SPLIT_SPEC[name].whole} "
          f"masks {len(ms)} tiles per workgroup {sorted({so.tiles_of(j0, J, P) for j0 in range(J)})} nudged rows {so.nudges(name, _cus())}")
    _report(name, worst)
    assert bad == [], bad
    assert ones is not None and torch.equal(ones, _learn(grp, case, dev, None))


def test_general_agent_weights_match_the_row_scaled_oracle():
    """64 sets x (32 J + 1) platoons, factors w_p * P / sum(w) that differ per platoon and per set (0.2 ... 3.0, +-20 % jitter): against
    the float64 oracle with the same factors on both loss seeds of every row, within max(SPLIT_TOL, 4 x its float32 twin's error)."""
    need_gpu()
    name = "split_64sets_deep"
    case, J, P, grp, batch, dev = _setup(name)
    w, per = so.weighted_reference(name, _cus())
    g = _learn(grp, case, dev, t(w.reshape(-1)))
    assert torch.isfinite(g).all()
    worst = {}
    bad = _compare(grp, g, per, "weighted", worst, "weighted")
    _report(name, worst)
    assert bad == [], bad


@pytest.mark.parametrize("name", ["split_64sets_deep", "fset_modelA_ragged"])
def test_zero_weight_agents_add_nothing(name):
    """Weight 1 on two platoons that share a workgroup (p0 and p0 + J), 0 elsewhere; the other agents once with the case's data, once
    with an independent draw of the same distributions (not x 100: the fp16 overflow watch would rightly answer with NaN). A zero-weight
    row has exactly zero loss seeds, hence zero terms in every sum, and the partials are reduced in a fixed order: the two slabs are
    bit-identical. A tile index that reads a neighbour's rows, or a sum that takes in another agent's, shows up."""
    need_gpu()
    case, J, P, grp, (s, a, r, s2), _ = _setup(name)
    p0 = 1  # ordinals 0 and 1 of workgroup 1 % J
    assert p0 + J < P
    w = _platoon_mask(case, P, [p0, p0 + J])
    inside = w > 0  # [n_agents]
    o = so.other_draw(name, _cus())
    assert all(x.shape == y.shape and not np.array_equal(x, y) for x, y in zip((s, a, r, s2), o))
    mix = lambda x, y: np.where(inside.reshape((-1,) + (1,) * (x.ndim - 1)), x, y).astype(np.float32)
    g0 = _learn(grp, case, (t(s), t(a), t(r), t(s2)), t(w))
    g1 = _learn(grp, case, tuple(t(mix(x, y)) for x, y in zip((s, a, r, s2), o)), t(w))
    assert torch.isfinite(g0).all() and torch.isfinite(g1).all() and g0.abs().max() > 0
    if not torch.equal(g0, g1):
        d = (g0 - g1).abs()
        lay = grp.lay
        leak = {blk: (d[:, lo:hi].max() / g0[:, lo:hi].abs().max()).item() for blk, lo, hi in (("actor", 0, lay.actor_size), ("critic", lay.actor_size, lay.theta_size))}
        raise AssertionError(f"{name}: zero-weight agents leak, largest difference / block max {leak}, sets {torch.nonzero(d.amax(dim=1)).flatten().tolist()}")
