"""The fused bf16 set learner (csrc/fset.hip, the product library) agent by agent against the float64 oracle.

A whole-set comparison cannot see one agent's 64-row tile: at 70 platoons it carries 1.4 % of a set's gradient, less than the 2e-2 that
tests/test_gpu_fset.py allows, and no shape of that file gives a workgroup more than two tiles. ``agent_weight`` multiplies the two
loss seeds of an agent's rows (head_kernel), so with weight 1 on the agents of one platoon p0 and 0 elsewhere ONE call returns, for
every set at once, 1 / P x learn(that agent's 64 rows): compared here tensor by tensor under the rule of tests/bf16_oracle.py --
max(1e-4, 4 x the error of the bf16-operand oracle, pooled over one set's masks of one tile size), derived from the reference alone and
held under the cap of 0.5 by tests/test_bf16_oracle_cpu.py. The mask label names the platoon, hence the workgroup p0 % J, the tile
ordinal p0 // J and the wave pair. Cases (bf16_oracle.FSET): 64 sets x 27 platoons (7 tiles per workgroup: the prefetch, a wave
pair's second tile, dxa's parities, the widest set stride), 5 sets x 70 (ragged, Model A), 1 set x 300. Measured figures:
docs/fset_tile_parity.md."""
import numpy as np
import pytest
import torch

from tests import bf16_oracle as bo
from tests.gpu_util import need_gpu, t
from tests.test_gpu_mlp import _nets, _perturbed_group

pytestmark = pytest.mark.gpu

FSET_NAMES = [c.name for c in bo.FSET]


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _setup(name):
    """(case, J, P, group, agent-major host batch, the same on the device); the group's weights are the host tables' bit for bit."""
    case = bo.fset_case(name, _cus())
    J, P, _ = bo.fset_plan(name, _cus())
    conf, grp = _perturbed_group(case.n_sets, S=case.S, seed=case.seed, **bo.case_conf_kw(case))
    for k in case.check:  # the CPU-side tables are of THESE weights
        for host, devw in zip(bo.case_nets(case, k), _nets(grp, k, np.float64)):
            assert all(np.array_equal(x, y) for x, y in zip(host, devw)), k
    batch = bo.fset_batch(case)
    return case, J, P, grp, batch, tuple(t(x) for x in batch)


def _learn(grp, case, dev, agent_weight, split=False):
    n_agents = case.n_sets * case.rows // bo.FSET_B
    fn = grp.learn_set_split if split else grp.learn_set_fused
    g = fn(*dev, n_agents, agent_weight=agent_weight)
    torch.cuda.synchronize()
    return g.clone()


def _platoon_mask(case, P, platoons):
    w = np.zeros((P, case.n_sets), np.float32)  # agent v = p * n_sets + m
    w[list(platoons)] = 1.0
    return w.reshape(-1)


def _named(grp, row):
    cg, ag = grp.grads_as_lists(row)
    return dict(zip(bo.NAMES, cg + ag))


def _compare(name, grp, g, checks, worst, label):
    """checks: {set: (ref, table)}. -> the rule's violations of one result; keeps the worst error / e_bf16 per (tile size, tensor)."""
    bad = []
    for k, (ref, tsz, table) in checks.items():
        got = _named(grp, g[k])
        for tensor in bo.NAMES:
            scale, e, limit = table[tensor]
            err = float(np.max(np.abs(got[tensor].astype(np.float64) - ref[tensor])) / scale)
            ratio = err / max(e, 1e-300)
            if ratio > worst.get((tsz, tensor), (-1.0,))[0]:
                worst[(tsz, tensor)] = (ratio, e, err, limit, f"set{k}:{label}")
        bad += [(k, label) + v for v in bo.violations(got, ref, table)]
    return bad


def _report(name, worst):
    for (tsz, tensor), (ratio, e, err, limit, label) in sorted(worst.items(), key=lambda kv: (str(kv[0][0]), bo.NAMES.index(kv[0][1]))):
        print(f"TILE {name} t={tsz} {tensor}: e_bf16 {e:.3e} kernel {err:.3e} ({label}) ratio {ratio:.2f} tol {limit:.3e}")


@pytest.mark.parametrize("name", FSET_NAMES)
def test_every_agent_mask_matches_the_oracle_within_four_times_the_bf16_oracle_error(name):
    """One learn_set_fused call per mask (the masked platoons one by one, then all ones), the other agents ordinary data; every checked
    set's slab against the float64 oracle of the masked agent of THAT set, every tensor under the set's pooled rule, finite results.
    The TILE lines give, per tile size and tensor, the comparison with the largest error / e_bf16 over the sets and masks.
    The whole-set mask is also agent_weight = 1 == agent_weight = None: x * 1.0f is exact and the partials are summed in a fixed
    order, so the two slabs are bit-identical."""
    need_gpu()
    case, J, P, grp, batch, dev = _setup(name)
    ms, per = bo.fset_reference(name, _cus())
    worst, bad = {}, []
    ones = None
    for i, (label, tsz, lo, hi) in enumerate(ms):
        mask = _platoon_mask(case, P, range(P) if tsz == "whole" else [lo // bo.FSET_B])
        g = _learn(grp, case, dev, t(mask))
        assert torch.isfinite(g).all(), label
        where = label if tsz == "whole" else f"{label}(wg{(lo // bo.FSET_B) % J},tile{(lo // bo.FSET_B) // J})"
        bad += _compare(name, grp, g, {k: (refs[i], tsz, tol[tsz]) for k, (refs, _, tol) in per.items()}, worst, where)
        if tsz == "whole":
            ones = g
    print(f"PLAN {name}: CUs {_cus()} J {J} P {P} sets {case.n_sets} checked {case.check} masks {len(ms)}")
    _report(name, worst)
    assert bad == [], bad
    assert ones is not None and torch.equal(ones, _learn(grp, case, dev, None))


def test_general_agent_weights_match_the_row_scaled_oracle():
    """64 sets x 27 platoons, factors w_p * P / sum(w) that differ per platoon and per set (0.2 ... 3.0, +-20 % jitter): against the
    oracle with the same factors on both loss seeds of every row, under the same rule (its own one-mask table per checked set)."""
    need_gpu()
    name = "fset_64sets"
    case, J, P, grp, batch, dev = _setup(name)
    w, per = bo.fset_weighted_reference(name, _cus())
    g = _learn(grp, case, dev, t(w.reshape(-1)))
    assert torch.isfinite(g).all()
    worst = {}
    bad = _compare(name, grp, g, {k: (ref, "weighted", tol) for k, (ref, _, tol) in per.items()}, worst, "weighted")
    _report(name, worst)
    assert bad == [], bad


@pytest.mark.parametrize("name", ["fset_64sets", "fset_modelA_ragged"])
def test_zero_weight_agents_add_nothing(name):
    """Weight 1 on two platoons that share a workgroup (p0 and p0 + J), 0 elsewhere; the other agents once with ordinary data, once
    with s, s' and r x 100 (finite: bf16 has f32's exponent range, so pack_x_kernel's non-finite watch stays quiet). A zero-weight row
    has exactly zero loss seeds, hence zero dZ2 and zero terms in every sum, and the sums are taken in a fixed order: the two slabs are
    bit-identical. A tile index that reads a neighbour's rows shows up a hundredfold."""
    need_gpu()
    case, J, P, grp, (s, a, r, s2), _ = _setup(name)
    p0 = 1
    assert p0 + J < P
    w = _platoon_mask(case, P, [p0, p0 + J])
    inside = w > 0  # [n_agents]
    big = lambda x: np.where(inside.reshape((-1,) + (1,) * (x.ndim - 1)), x, 100.0 * x).astype(np.float32)
    g0 = _learn(grp, case, (t(s), t(a), t(r), t(s2)), t(w))
    g1 = _learn(grp, case, (t(big(s)), t(a), t(big(r)), t(big(s2))), t(w))
    assert torch.isfinite(g0).all() and torch.isfinite(g1).all() and g0.abs().max() > 0
    if not torch.equal(g0, g1):
        d = (g0 - g1).abs()
        lay = grp.lay
        leak = {blk: (d[:, lo:hi].max() / g0[:, lo:hi].abs().max()).item() for blk, lo, hi in (("actor", 0, lay.actor_size), ("critic", lay.actor_size, lay.theta_size))}
        raise AssertionError(f"{name}: zero-weight agents leak, largest difference / block max {leak}, sets {torch.nonzero(d.amax(dim=1)).flatten().tolist()}")


def test_split_engine_at_64_sets_matches_the_oracle():
    """The f32-class sibling (csrc/fsplit.hip: same plan, same finalize) on the 64-set batch, whole set, sets 0 / 37 / 63: every tensor
    within max(SPLIT_TOL, 4 x the float32 oracle's own error) of the float64 oracle -- tests/test_gpu_fsplit.py's rule and constants."""
    from tests.test_gpu_fsplit import _errors_vs_oracle

    need_gpu()
    case, J, P, grp, (s, a, r, s2), dev = _setup("fset_64sets")
    g = _learn(grp, case, dev, None, split=True)
    assert torch.isfinite(g).all()
    errs, worst = _errors_vs_oracle(grp, g, s, a, r, s2, P, case.n_sets, case.check)
    print(f"SPLIT fset_64sets sets {case.check}: worst error / tensor max {worst:.3e}")
    assert not errs, errs
