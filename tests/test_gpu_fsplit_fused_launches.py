"""The split learner's plain single call runs its ten persistent kernels and the actor's seed as two launches (csrc/fsplit.hip:
forward_kernel, backward_kernel: the bodies of the stand-alone kernels back to back, a workgroup barrier between two of them). The
two-phase form of the same call (phase="critic" then phase="actor") keeps launching the stand-alone kernels, one per body: it is the
yardstick here, and the single call must give its bits -- slab and losses -- whatever the tile count per workgroup is, whatever the
workspace held before, call after call; and an fp16 overflow inside a fused phase must still turn the slab to NaN.

J = CUs // n_sets workgroups serve a set, each tiles j0, j0 + J, ..; a head deals its tiles to the wave pairs FAST : SLOW = 5 : 3 in
periods of 16. The shapes: P = 1 (all workgroups but one per set without a tile), J + 1 (one workgroup with two tiles), 17 J + 3 (a
full period of 16 plus a remainder, uneven counts), 4 J - 1 at three sets (another J, one workgroup short) and J + 5 at one set."""
import numpy as np
import pytest
import torch

from tests.gpu_util import need_gpu, t
from tests.test_gpu_fset import _batch
from tests.test_gpu_fsplit_glue import _bits, _dirty, _workspace
from tests.test_gpu_mlp import _perturbed_group

pytestmark = pytest.mark.gpu


def _J(n_sets):
    return torch.cuda.get_device_properties(0).multi_processor_count // n_sets


# (n_sets, P as a function of J, S, weighted)
CASES = [
    pytest.param(5, lambda J: 1, 4, False, id="5sets-P1-S4"),
    pytest.param(5, lambda J: J + 1, 4, False, id="5sets-J+1-S4"),
    pytest.param(5, lambda J: J + 1, 3, False, id="5sets-J+1-S3"),
    pytest.param(5, lambda J: 17 * J + 3, 4, False, id="5sets-17J+3-S4"),
    pytest.param(5, lambda J: 17 * J + 3, 3, False, id="5sets-17J+3-S3"),
    pytest.param(3, lambda J: 4 * J - 1, 4, False, id="3sets-4J-1-S4"),
    pytest.param(1, lambda J: J + 5, 4, False, id="1set-J+5-S4"),
    pytest.param(5, lambda J: J + 1, 4, True, id="5sets-J+1-S4-weighted"),
]


def _setup(n_sets, P, S, seed, weighted=False):
    conf, grp = _perturbed_group(n_sets, S=S, seed=seed)
    n = P * n_sets
    rs = np.random.RandomState(seed + 1)
    batch = tuple(t(x) for x in _batch(rs, n, S))
    kw = {}
    if weighted:
        kw["agent_weight"] = t(rs.uniform(0.25, 1.75, size=n).astype(np.float32))
    return grp, batch, n, kw


def _single(grp, batch, n, kw, grads=None):
    losses = torch.full((grp.n_sets, 2), 7.0, device="cuda")
    g = grp.learn_set_fused(*batch, n, grads=grads, losses=losses, split=True, **kw)
    torch.cuda.synchronize()
    return g.clone(), losses.clone()


def _pair(grp, batch, n, kw):
    losses = torch.full((grp.n_sets, 2), 7.0, device="cuda")
    g = grp.learn_set_fused(*batch, n, losses=losses, split=True, phase="critic", **kw)
    g = grp.learn_set_fused(*batch, n, grads=g, split=True, phase="actor")
    torch.cuda.synchronize()
    return g.clone(), losses.clone()


def _same(x, y):
    return torch.equal(_bits(x[0]), _bits(y[0])) and torch.equal(_bits(x[1]), _bits(y[1]))


@pytest.mark.parametrize("n_sets,p_of_j,S,weighted", CASES)
def test_the_single_call_gives_the_bits_of_the_two_phase_pair(n_sets, p_of_j, S, weighted):
    need_gpu()
    J = _J(n_sets)
    P = p_of_j(J)
    assert J >= 2 and P >= 1
    grp, batch, n, kw = _setup(n_sets, P, S, 301, weighted)
    ref = _pair(grp, batch, n, kw)
    assert torch.isfinite(ref[0]).all() and torch.isfinite(ref[1]).all() and ref[0].abs().max() > 0
    assert not bool((ref[1] == 7.0).any())  # (both losses of every set were written)
    got = _single(grp, batch, n, kw)
    assert _same(got, ref)
    if weighted:  # the weights bite: the unweighted call gives other bits
        assert not torch.equal(_bits(_single(grp, batch, n, {})[0]), _bits(ref[0]))


def test_a_poisoned_workspace_and_slab_give_the_same_bits_and_so_does_a_second_call():
    """17 J + 3 tiles per set. Every word of the workspace and of the slab a NaN bit pattern (then 0xFF bytes) before the single call:
    the fused launches read nothing that this call has not written. And the call made twice in a row gives the same bits twice."""
    need_gpu()
    n_sets, S = 5, 4
    P = 17 * _J(n_sets) + 3
    grp, batch, n, kw = _setup(n_sets, P, S, 303)
    ref = _pair(grp, batch, n, kw)
    assert torch.isfinite(ref[0]).all() and ref[0].abs().max() > 0
    for how in ("nan", "ff"):
        ws = _dirty(_workspace(grp, n), how)
        ptr0 = ws.data_ptr()
        slab = torch.full((n_sets, grp.lay.theta_size), float("nan"), device="cuda")
        got = _single(grp, batch, n, kw, grads=slab)
        assert grp._fsplit_ws.data_ptr() == ptr0, "the call replaced the workspace: the poisoned one was not used"
        assert torch.equal(_bits(slab), _bits(got[0]))  # (the call wrote into the slab it was given)
        assert _same(got, ref), how
    first = _single(grp, batch, n, kw)
    second = _single(grp, batch, n, kw)
    assert _same(first, ref) and _same(second, ref)


def test_an_fp16_overflow_in_a_fused_phase_still_turns_the_slab_to_nan():
    """tests/test_gpu_fsplit.py's recipe at the critic's action layer (HEAD_BOTH, branch A: the fourth phase of the forward launch): za =
    2.5 x 480 = 1200 >= 1023.75 overflows the fp16 activation -> NaN over the slab; at half the weight (600) the call is finite and
    still the two-phase pair's bits."""
    need_gpu()
    P, M, S = 5, 2, 4
    conf, grp = _perturbed_group(M, S=S, seed=83)
    lay = grp.lay
    n = P * M
    s, a, r, s2 = (t(x) for x in _batch(np.random.RandomState(84), n, S))
    s[:, :, 0] = 1.5
    s2[:, :, 0] = 1.5
    a[:] = 2.5
    at = lay.actor_size + lay.cWa + 5
    grp.theta[0, at] = 240.0
    ref = _pair(grp, (s, a, r, s2), n, {})
    got = _single(grp, (s, a, r, s2), n, {})
    assert torch.isfinite(got[0]).all() and _same(got, ref)
    grp.theta[0, at] = 480.0
    g, _ = _single(grp, (s, a, r, s2), n, {})
    for lo, hi in ((lay.aW2, lay.aW2 + 256 * 128), (lay.actor_size + lay.cW2, lay.actor_size + lay.cW2 + 304 * 128)):
        assert torch.isnan(g[:, lo:hi]).all()
    grp.theta[0, at] = 240.0  # and the flag does not stick
    assert _same(_single(grp, (s, a, r, s2), n, {}), ref)
