"""The split set learner's start-up (csrc/fsplit.hip: what a workgroup of head_kernel, dw_kernel, dx_kernel, dxa_kernel does in front of
its first tile) at the shapes where a change there can go wrong. Since r14 every load of that part -- the whole LDS weight image, the
tables, the resident fragments, the first one or two tiles' operands -- is requested before the first of them is waited for, and the
row factor's scale (set_gscale: loads, a reduction, a barrier) runs behind those requests, not in front of them.

Shapes, per S in {3, 4} and n_sets in {1, 2, 5}, with J = CUs // n_sets workgroups per set (make_plan):
    P = J - 1   fewer platoons than compute units: make_plan then gives the set P workgroups of ONE tile each (no tile prefetched in the
                loop, dxa's waves of parity 1 and the second register sets of dw / dx idle) -- the grid no longer fills the device;
    P = J       one tile per workgroup on every CU;
    P = J + 1   ONE workgroup with two tiles: the second tile is the one whose fetch dw / dx issue in the prologue;
    P = 2 J + 1 three tiles in one workgroup, two in the others: dx's third slot, dw's first reuse of a register set.
Any critic gradient covers the critic's last k-steps (K = 304: the 16-feature tile) and the action tiles.

Inputs, references and the rule are those of tests/test_gpu_fsplit_tiles.py (tests/split_oracle.py, tests/bf16_oracle.py): host weight
tables equal to the device group's bit for bit, the batch conditioned against relu ties on the host, the float64 oracle of every set's
64 P rows, and per tensor max |got - ref| / max |ref| <= max(SPLIT_TOL, 4 x the float32 NumPy oracle's own error) -- the whole-set
floor of split_oracle.table. Both losses within 1e-4 (tests/test_gpu_fsplit.py::_errors_vs_oracle). Every case runs its call twice, each
time on a workspace, a slab and a loss buffer filled with NaN: the two results must be the same bits, and finite."""
import functools

import numpy as np
import pytest
import torch

from avddpg_amd import vec
from oracle import mlp as omlp
from tests import bf16_oracle as bo
from tests import split_oracle as so
from tests.gpu_util import need_gpu, t
from tests.test_gpu_fset import _batch
from tests.test_gpu_fsplit import SPLIT_TOL
from tests.test_gpu_mlp import _nets, _perturbed_group

pytestmark = pytest.mark.gpu

LOSS_TOL = 1e-4
SHAPES = {"below_J": lambda J: max(1, J - 1), "J": lambda J: J, "J_plus_1": lambda J: J + 1, "2J_plus_1": lambda J: 2 * J + 1}


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _case(S, n_sets, shape, cus):
    J = max(1, cus // n_sets)
    P = SHAPES[shape](J)
    seed = 1400 + 100 * S + 10 * n_sets + list(SHAPES).index(shape)
    return J, P, bo.Case(f"startup_S{S}_M{n_sets}_{shape}", bo.FSET_WIDTHS, S, P * so.B, seed, "start-up shapes", (), "generic", n_sets,
                         tuple(range(n_sets)))


@functools.lru_cache(maxsize=2)
def _conditioned(S, n_sets, shape, cus):
    """(case, agent-major batch, nudged rows): drawn as bo.fset_batch draws it, every row conditioned as split_oracle._batch does for a
    set with a whole-set mask (each set's layer maxima over its own rows)."""
    _, P, c = _case(S, n_sets, shape, cus)
    s, a, r, s2 = bo.fset_batch(c)
    nudged = 0
    for _ in range(8):
        bad = np.zeros(s.shape[:2], bool)
        for k in range(n_sets):
            an, cn, _, _ = bo.case_nets(c, k)
            sel = np.arange(P) * n_sets + k
            bad[sel] = so.tie_rows(an, cn, s[sel].reshape(-1, S).astype(np.float64), a[sel].reshape(-1, 1).astype(np.float64)).reshape(P, -1)
        if not bad.any():
            break
        nudged += int(bad.sum())
        s[bad] += so.NUDGE_S
        a[bad] = np.clip(a[bad] + so.NUDGE_A, -so.HIGH, so.HIGH)
    else:
        raise AssertionError(f"{c.name}: could not condition the batch")
    return c, (s, a, r, s2), nudged


def _nan_call(grp, dev, n):
    """One learn_set_split call on a workspace, a gradient slab and a loss buffer that hold nothing but NaN -> (grads, losses)."""
    ws = grp._workspace("_fsplit_ws", "avd_learn_set_split_workspace", n)
    assert ws.numel() % 4 == 0
    ws.view(torch.float32).fill_(float("nan"))
    grads = torch.full((grp.n_sets, grp.lay.theta_size), float("nan"), device="cuda")
    losses = torch.full((grp.n_sets, 2), float("nan"), device="cuda")
    ptr0 = ws.data_ptr()
    g = grp.learn_set_split(*dev, n, grads=grads, losses=losses)
    torch.cuda.synchronize()
    assert grp._fsplit_ws.data_ptr() == ptr0 and g.data_ptr() == grads.data_ptr()
    return g.clone(), losses.clone()


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("n_sets", [1, 2, 5])
@pytest.mark.parametrize("S", [3, 4])
def test_start_up_shapes_match_the_float64_oracle_and_repeat_bit_for_bit_on_nan_filled_memory(S, n_sets, shape):
    need_gpu()
    cus = _cus()
    J, P, _ = _case(S, n_sets, shape, cus)
    c, batch, nudged = _conditioned(S, n_sets, shape, cus)
    conf, grp = _perturbed_group(n_sets, S=S, seed=c.seed, **bo.case_conf_kw(c))
    for k in range(n_sets):  # the references and the tie conditioning are of THESE weights
        for host, devw in zip(bo.case_nets(c, k), _nets(grp, k, np.float64)):
            assert all(np.array_equal(x, y) for x, y in zip(host, devw)), k
    dev = tuple(t(x) for x in batch)
    n = P * n_sets
    g1, l1 = _nan_call(grp, dev, n)
    g2, l2 = _nan_call(grp, dev, n)
    assert torch.isfinite(g1).all() and torch.isfinite(l1).all() and g1.abs().max() > 0
    assert torch.equal(g1.view(torch.int32), g2.view(torch.int32)) and torch.equal(l1.view(torch.int32), l2.view(torch.int32))
    sm = bo.set_major(batch, n_sets)
    s, a, r, s2 = sm
    bad = []
    print(f"PLAN {c.name}: CUs {cus} J {min(J, P)} P {P} sets {n_sets} tiles per workgroup "
          f"{sorted({so.tiles_of(j0, min(J, P), P) for j0 in range(min(J, P))})} nudged rows {nudged}")
    for k in range(n_sets):
        nets = bo.case_nets(c, k)
        rows = (s[k], a[k], r[k][:, None], s2[k])
        cg64, ag64, aux = bo.learn(rows, *nets, rnd=bo.identity)  # (= bo.tile_learn over the whole set, and its losses)
        ref = dict(zip(so.NAMES, cg64 + ag64))
        cg32, ag32, _ = omlp.learn(rows, *so._nets32(nets))
        e32 = {name: so.relerr(g.astype(np.float64), ref[name]) for name, g in zip(so.NAMES, cg32 + ag32)}
        table = so.table("whole", e32)
        assert all(limit >= SPLIT_TOL for _, limit in table.values())
        cg, ag = grp.grads_as_lists(g1[k])
        got = dict(zip(so.NAMES, cg + ag))
        for name in so.NAMES:
            print(f"STARTUP {c.name} set {k} {name}: e32 {e32[name]:.3e} kernel {so.relerr(got[name], ref[name]):.3e} tol {table[name][1]:.3e}")
        bad += [(k,) + v for v in so.violations(got, ref, table)]
        lo = l1[k].cpu().numpy()
        print(f"STARTUP {c.name} set {k} losses: critic {lo[0]:.6e} / {aux['critic_loss']:.6e} actor {lo[1]:.6e} / {aux['actor_loss']:.6e}")
        if not abs(lo[0] - aux["critic_loss"]) <= LOSS_TOL * abs(aux["critic_loss"]):
            bad.append((k, "critic_loss", float(lo[0]), float(aux["critic_loss"])))
        if not abs(lo[1] - aux["actor_loss"]) <= LOSS_TOL * max(1e-2, abs(aux["actor_loss"])):
            bad.append((k, "actor_loss", float(lo[1]), float(aux["actor_loss"])))
    assert bad == [], bad


def test_an_fp16_overflow_still_turns_the_slab_to_nan_with_two_tiles_in_one_workgroup():
    """tests/test_gpu_fsplit.py::test_split_set_learner_turns_an_fp16_overflow_into_nan_gradients (its critic action layer case: HEAD_BOTH,
    branch A) at P = J + 1: the `bad` flag's path -- watch, atomicOr, finalize -- behind the new prologue. Just below the threshold the
    result is finite and the exact engine's."""
    need_gpu()
    M, S = 2, 4
    P = max(1, _cus() // M) + 1
    conf, grp = _perturbed_group(M, S=S, seed=83)
    lay = grp.lay
    s, a, r, s2 = (t(x) for x in _batch(np.random.RandomState(84), P * M, S))
    s[:, :, 0] = 1.5
    s2[:, :, 0] = 1.5
    a[:] = 2.5
    grp.theta[0, lay.actor_size + lay.cWa + 5] = 240.0  # za = 2.5 * 240 = 600 < 1023.75
    g = grp.learn_set_split(s, a, r, s2, P * M).clone()
    assert torch.isfinite(g).all()
    exact = vec.fed_mean(grp.learn(s, a, r, s2, M), P, M, method=conf.interfrl)
    for lo, hi in ((0, lay.actor_size), (lay.actor_size, lay.theta_size)):
        assert (g[:, lo:hi] - exact[:, lo:hi]).abs().max().item() <= SPLIT_TOL * exact[:, lo:hi].abs().max().item()
    grp.theta[0, lay.actor_size + lay.cWa + 5] = 480.0  # za = 1200: S1 relu(za) overflows fp16
    g = grp.learn_set_split(s, a, r, s2, P * M)
    for lo, hi in ((lay.aW2, lay.aW2 + 256 * 128), (lay.actor_size + lay.cW2, lay.actor_size + lay.cW2 + 304 * 128)):
        assert torch.isnan(g[:, lo:hi]).all()
