"""The shared-set bf16 learner (csrc/wide.hip, the product library) tile by tile against the float64 oracle.

A whole-set comparison cannot see a 32-row tile of wrong gradients (4096 rows average it to under the bf16 rounding noise: the fault
fw::fwd_gen_kernel<true, 4> once had met every tensor-level tolerance). ``row_weight`` multiplies each row's two loss seeds
(rows_kernel), so with weight 1 on one tile and 0 elsewhere learn_shared returns that tile's contribution / Ns: compared here with
Nt / Ns x oracle.learn(rows of the tile), tensor by tensor, under the rule of tests/bf16_oracle.py -- max(1e-4, 4 x the error of the
bf16-operand oracle, pooled over the masks of the case and tile size), derived from the reference alone and asserted under the cap
of 0.5 by tests/test_bf16_oracle_cpu.py. The cases (bf16_oracle.CASES) come from the path conditions of avd_learn_shared_bf16.
The emulation places two roundings
where the kernels document them (bf16_oracle.learn placement=): generic rounding alone left the one-element ab3 of two whole-set masks
at 4.4 x its own error. Measured figures and that finding: docs/wide_tile_parity.md."""
import numpy as np
import pytest
import torch

from tests import bf16_oracle as bo
from tests.gpu_util import need_gpu, t
from tests.test_gpu_mlp import _nets, _perturbed_group

pytestmark = pytest.mark.gpu


def _group_and_batch(case):
    conf, grp = _perturbed_group(case.n_sets, S=case.S, seed=case.seed, **bo.case_conf_kw(case))
    return grp, bo.case_batch(case)


def _learn(grp, case, dev, row_weight):
    n_agents = case.n_sets * case.rows // 64
    g = grp.learn_shared(*dev, n_agents, row_weight=row_weight)
    torch.cuda.synchronize()
    return g.clone()


def _weights(case, lo, hi):
    w = np.zeros((case.n_sets, case.rows), np.float32)
    w[:, lo:hi] = 1.0
    return t(w)


def _named(grp, row):
    cg, ag = grp.grads_as_lists(row)
    return dict(zip(bo.NAMES, cg + ag))


@pytest.mark.parametrize("name", [c.name for c in bo.CASES])
def test_every_tile_mask_matches_the_oracle_within_four_times_the_bf16_oracle_error(name):
    """One learn_shared call per mask (all 256-row tiles, 32-row sub-tiles, the whole set), two weight sets, the other rows ordinary
    data; the second set's slab against the float64 oracle of the masked rows, every tensor of every mask under the pooled rule.
    The whole-set mask (all ones) under the same rule also shows row_weight = 1 == row_weight = None."""
    need_gpu()
    case = bo.CASE[name]
    grp, batch = _group_and_batch(case)
    k = case.check[0]
    for host, devw in zip(bo.case_nets(case, k), _nets(grp, k, np.float64)):  # the CPU-side tables are of THESE weights
        assert all(np.array_equal(x, y) for x, y in zip(host, devw))
    ms, refs, _, tol = bo.case_reference(name)
    s, a, r, s2 = batch
    dev = (t(s), t(a), t(r), t(s2))
    worst, bad = {}, []
    for (label, tsz, lo, hi), ref in zip(ms, refs):
        g = _learn(grp, case, dev, _weights(case, lo, hi))
        assert torch.isfinite(g).all(), label
        got = _named(grp, g[k])
        skip = bo.skipped(case, tsz)
        for tensor in bo.NAMES:
            scale, e, limit = tol[tsz][tensor]
            err = float(np.max(np.abs(got[tensor].astype(np.float64) - ref[tensor])) / scale)
            if err > worst.get((tsz, tensor), (-1.0,))[0]:
                worst[(tsz, tensor)] = (err, label)
        bad += [(label,) + v for v in bo.violations(got, ref, tol[tsz], skip)]
    for (tsz, tensor), (err, label) in sorted(worst.items()):  # the figures of docs/wide_tile_parity.md
        _, e, limit = tol[tsz][tensor]
        print(f"TILE {name} t={tsz} {tensor}: e_bf16 {e:.3e} kernel {err:.3e} ({label}) ratio {err / max(e, 1e-300):.2f} tol {limit:.3e}")
    assert bad == [], bad
    # row_weight = None is row_weight = 1: the same seeds (x 1.0f is exact), only the order of the f32 atomics differs -- 1e-4 of each
    # block's max, the repeat-to-repeat bound of test_config5_hidden1024_repeats_of_a_learn_agree
    ones = _learn(grp, case, dev, _weights(case, 0, case.rows))
    plain = _learn(grp, case, dev, None)
    lay = grp.lay
    for lo, hi in ((0, lay.actor_size), (lay.actor_size, lay.theta_size)):
        d = (ones[:, lo:hi] - plain[:, lo:hi]).abs().max().item()
        assert d <= 1e-4 * plain[:, lo:hi].abs().max().item(), (lo, d)


@pytest.mark.parametrize("name", ["h1024", "h512"])
@pytest.mark.parametrize("lo,hi", [(512, 768), (256 + 96, 256 + 128)])
def test_zero_weight_rows_add_nothing(name, lo, hi):
    """The rows outside the mask once with ordinary data, once with states and rewards x 100 (finite; bf16 has f32's range): their
    seeds are exact zeros either way, so the two slabs may differ by the order of the f32 atomics alone -- 1e-4 of each block's max
    (the bound test_config5_hidden1024_repeats_of_a_learn_agree holds repeats to). A row index that reads a neighbouring tile shows
    up a hundredfold."""
    need_gpu()
    case = bo.CASE[name]
    grp, (s, a, r, s2) = _group_and_batch(case)
    w = _weights(case, lo, hi)
    inside = np.zeros(case.rows, bool)
    inside[lo:hi] = True
    big = lambda x: np.where(inside.reshape((1, -1) + (1,) * (x.ndim - 2)), x, 100.0 * x).astype(np.float32)
    g0 = _learn(grp, case, (t(s), t(a), t(r), t(s2)), w)
    g1 = _learn(grp, case, (t(big(s)), t(a), t(big(r)), t(big(s2))), w)
    assert torch.isfinite(g0).all() and torch.isfinite(g1).all()
    lay = grp.lay
    for b0, b1 in ((0, lay.actor_size), (lay.actor_size, lay.theta_size)):
        scale = g0[:, b0:b1].abs().max().item()
        d = (g0[:, b0:b1] - g1[:, b0:b1]).abs().max().item()
        print(f"LEAK {name} rows [{lo}, {hi}) block [{b0}, {b1}): {d / scale:.3e} of the block's max")
        assert scale > 0 and d <= 1e-4 * scale, (name, b0, d / scale)
