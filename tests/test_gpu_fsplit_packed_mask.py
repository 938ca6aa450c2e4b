"""The split learner's relu masks travel from the heads to dw / dx / dxa as one bit per element (csrc/fsplit.hip, HeadArgs::sm).
Tensor tolerances over thousands of rows cannot see one wrong mask bit, so these tests make ONE agent's 64 rows the whole
gradient of its set: one-hot agent weights (the agent_weight path: every other agent's loss seeds are zero) with the weight P,
which turns the set's mean over P agents into that agent's own 64-row batch gradient. Each set is then compared with the float64
oracle on that batch at GRAD_TOL (far below what one wrong bit costs), for agents at the first and the last tile of a workgroup and at several residues of J (the
workgroups per set), S = 3 and 4, L = 5 and 10. Every picked batch holds rows with both signs of the critic's seed q - y, and one
row whose second-layer pre-activations are <= 0 in every column, in the actor and in critic(s, a) (its mask words are zero)."""
import numpy as np
import pytest
import torch

from oracle import mlp as omlp
from tests.gpu_util import need_gpu, t
from tests.test_gpu_fset import NAMES, _batch
from tests.test_gpu_fsplit import _untie
from tests.test_gpu_mlp import GRAD_TOL, _nets, _perturbed_group, _relerr

pytestmark = pytest.mark.gpu

DEAD_ROW = 7  # the row of every picked agent whose z2 is made <= 0 everywhere


def _z2(grp, k, S, x, act):
    """float64 second-layer pre-activations of set k: actor(x) and critic(x, act) [rows, 128]."""
    an, cn, _, _ = _nets(grp, k, np.float64)
    W1, b1, W2, b2 = an[0], an[1], an[6], an[7]
    y1 = np.maximum(x @ W1 + b1, 0) * omlp._bn_coeffs(*an[2:6])[0] + omlp._bn_coeffs(*an[2:6])[1]
    Ws, bs, Wa, ba, CW2, cb2 = cn[0], cn[1], cn[2], cn[3], cn[12], cn[13]
    ys = np.maximum(x @ Ws + bs, 0) * omlp._bn_coeffs(*cn[4:8])[0] + omlp._bn_coeffs(*cn[4:8])[1]
    ya = np.maximum(act @ Wa + ba, 0) * omlp._bn_coeffs(*cn[8:12])[0] + omlp._bn_coeffs(*cn[8:12])[1]
    return y1 @ W2 + b2, np.concatenate([ys, ya], axis=1) @ CW2 + cb2


def _kill_row(grp, k, S, x, act):
    """Lower the second-layer biases of set k (actor and critic) so that row DEAD_ROW of x sits at -0.3 x the batch's typical
    |z2| in every column; the other rows keep a mix of active and inactive columns."""
    lay = grp.lay
    za, zc = _z2(grp, k, S, x, act)
    for z, off in ((za, lay.ab2), (zc, lay.actor_size + lay.cb2)):
        shift = z[DEAD_ROW] + 0.3 * np.abs(z).mean()
        grp.theta[k, off:off + 128] -= torch.tensor(shift, dtype=torch.float32, device=grp.theta.device)


def _run(S, M, P, picks, seed):
    """picks[k]: the platoon whose agent p * M + k is set k's whole gradient."""
    need_gpu()
    conf, grp = _perturbed_group(M, S=S, seed=seed)
    n = P * M
    s, a, r, s2 = _batch(np.random.RandomState(seed + 1), n, S)
    for k in range(M):
        v = picks[k] * M + k
        _kill_row(grp, k, S, s[v].astype(np.float64), a[v].astype(np.float64))
    _untie(grp, M, S, s, a)
    for k in range(M):  # centre the picked batch's TD errors: rows with both signs of g3 (r enters nothing but y)
        v = picks[k] * M + k
        _, _, aux = omlp.learn((s[v], a[v], r[v][:, None], s2[v]), *_nets(grp, k, np.float64))
        r[v] += np.float32(np.median((aux["q"] - aux["y"]).ravel()))
    w = np.zeros(n, np.float32)
    for k in range(M):
        w[picks[k] * M + k] = P  # (the set's mean over P agents -> this agent's mean over its 64 rows)
    g = grp.learn_set_split(t(s), t(a), t(r), t(s2), n, agent_weight=t(w)).clone()
    g2 = grp.learn_set_split(t(s), t(a), t(r), t(s2), n, agent_weight=t(w)).clone()
    torch.cuda.synchronize()
    assert torch.equal(g, g2), "two identical calls differ"
    assert torch.isfinite(g).all()
    for k in range(M):
        v = picks[k] * M + k
        x, act = s[v].astype(np.float64), a[v].astype(np.float64)
        za, zc = _z2(grp, k, S, x, act)
        assert (za[DEAD_ROW] <= 0).all() and (zc[DEAD_ROW] <= 0).all(), "the dead row came back to life"
        live = np.delete(np.stack([za, zc]), DEAD_ROW, axis=1) > 0
        assert 0.02 < live.mean() < 0.98, live.mean()  # the other rows: mixed masks
        batch = (s[v], a[v], r[v][:, None], s2[v])
        cg, ag, aux = omlp.learn(batch, *_nets(grp, k, np.float64))
        dq = (aux["q"] - aux["y"]).ravel()
        assert (dq > 0).any() and (dq < 0).any(), "the critic's seed has one sign only"
        cg32, ag32, _ = omlp.learn(batch, *_nets(grp, k, np.float32))
        gcg, gag = grp.grads_as_lists(g[k])
        # One wrong mask bit moves a 64-row sum by ~1/64 of its scale: held at the exact-f32 kernels' GRAD_TOL (or 4 x the float32
        # oracle's own error). The learner's precision at SPLIT_TOL is tests/test_gpu_fsplit.py's; over ONE agent's rows the
        # sums of g3-weighted terms (output layers: ab3, cW3, cg3, ..., with the TD errors centred above) cancel far below their
        # terms, and there the fp16-pair operands measure up to 5e-5 of the sum.
        bad = {name: (_relerr(got, ref), _relerr(r32, ref)) for name, got, ref, r32 in zip(NAMES, gcg + gag, cg + ag, cg32 + ag32)
               if _relerr(got, ref) > max(GRAD_TOL, 4 * _relerr(r32, ref))}
        assert not bad, (S, M, P, k, picks[k], bad)


def _J(M):
    """Workgroups per set: one per CU (fsplit.hip make_plan)."""
    return max(1, torch.cuda.get_device_properties(0).multi_processor_count // M)


@pytest.mark.parametrize("S,M", [(4, 5), (3, 5), (4, 10), (3, 10)])
def test_one_agent_per_set_matches_oracle_through_the_packed_masks(S, M):
    need_gpu()
    J = _J(M)
    P = 3 * J + 7  # three full rounds of tiles per workgroup and a ragged fourth
    # per set: first tile of workgroup 0 / of the last workgroup, the last tile of a workgroup, and residues 1, 2, J // 2 + 3 of J
    cands = [0, J - 1, P - 1, P - J, J + 1, 2 * J + 2, J // 2 + 3, 2 * J + J // 2]
    for rot in range(2):  # every candidate is some set's pick in one of the two calls
        picks = [cands[(k + rot * M) % len(cands)] for k in range(M)]
        _run(S, M, P, picks, seed=301 + 10 * S + M + rot)
