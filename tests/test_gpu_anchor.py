"""The anchored split set learner on the GPU (avd_learn_set_split_anchor_f16x3: csrc/anchor.hip's seed in the chain of csrc/fsplit.hip)
against tests/anchor_oracle.py: oracle.mlp.learn's gradients plus weight x the behaviour-cloning gradients of tests/clone_oracle.py, in
float64, over the shapes of tests/test_gpu_fsplit.py that reach distinct code of the seed kernel. The rule is
test_gpu_fsplit._errors_vs_oracle's: every gradient tensor within max(SPLIT_TOL, 4 x the float32 oracle's own error) of the float64
reference; both losses and the anchor loss within 1e-4. Then what the call promises bit for bit: weight 0 is learn_set_split, the
critic block and the losses never change, two calls agree, the workspace and the slab may hold anything, a seed batch's set uses its
vehicle's row; and what it refuses on the host.

Measured on one MI355X, worst over every parity case below (the six shapes, both weights, the clipped table): the actor tensors
aW1 4.4e-7, ab1 1.1e-6, ag1 1.2e-6, abe1 1.2e-6, aW2 1.2e-6, ab2 1.3e-6, ag2 1.2e-6, abe2 1.8e-6, aW3 1.3e-6, ab3 1.8e-6 of the tensor's
max (the un-anchored learner measures 3e-7 ... 5e-7 at these sizes; the difference mu - u* of two float32 numbers cancels where the
actor is near the law, and the kernel's mu carries the forward pass's own error into it); the critic tensors, which the anchor does not
touch, <= 6.2e-7. Every tensor is inside SPLIT_TOL = 2e-5 without the float32-oracle clause; losses and anchor loss agree to 7 digits."""
import ctypes

import numpy as np
import pytest
import torch

from avddpg_amd import _hip
from tests import anchor_oracle
from tests.gpu_util import need_gpu, t
from tests.test_gpu_fset import NAMES, _batch
from tests.test_gpu_fsplit import SPLIT_TOL, _untie
from tests.test_gpu_mlp import _nets, _perturbed_group, _relerr

pytestmark = pytest.mark.gpu

LO, HI = -2.5, 2.5
LOSS_TOL = 1e-4


def _table(M, scale=1.0, seed=7):
    """float32 [M, 4]: distinct rows around (kp, kv, ka, kf) = (2, 1, -0.3, 0.4)."""
    rs = np.random.RandomState(seed)
    return (scale * (np.array([2.0, 1.0, -0.3, 0.4]) + rs.uniform(-0.5, 0.5, size=(M, 4)))).astype(np.float32)


def _anchored(grp, batch, n, gains, weight, aw=None, grads=None):
    """One anchored call -> (grads, losses, anchor_loss), clones."""
    losses = torch.full((grp.n_sets, 2), 7.0, device="cuda")
    al = torch.full((grp.n_sets,), 7.0, device="cuda")
    g = grp.learn_set_split_anchor(*batch, n, t(gains), weight, al, grads=grads, losses=losses, agent_weight=None if aw is None else t(aw))
    torch.cuda.synchronize()
    return g.clone(), losses.clone(), al.clone()


def _check_sets(grp, got, s, a, r, s2, P, M, sets, gains, weights, aw=None, table_rows=None):
    """Every set of `sets` against the oracle at every weight of `weights` (got: {weight: (grads, losses, anchor_loss)}); the oracle's
    two summands are computed once per set and dtype. -> ({(weight, set, tensor): (error, float32 oracle's error)} of the misses,
    {tensor: worst error}, the smallest share of clipped targets)."""
    S = grp.lay.S
    rows = len(gains) if table_rows is None else table_rows
    errs, worst, clipped = {}, {}, 1.0
    for k in sets:
        sel = np.arange(P) * M + k
        batch = (s[sel], a[sel], r[sel], s2[sel])
        awk = None if aw is None else aw[sel]
        p64 = anchor_oracle.parts(batch, _nets(grp, k, np.float64), gains[k % rows], LO, HI, S == 3, agent_weight=awk)
        p32 = anchor_oracle.parts(batch, _nets(grp, k, np.float32), gains[k % rows], LO, HI, S == 3, agent_weight=awk)
        clipped = min(clipped, p64["clipped"])
        for w in weights:
            g, losses, al = got[w]
            (cg, ag), (cg32, ag32) = anchor_oracle.combine(p64, w), anchor_oracle.combine(p32, w)
            gcg, gag = grp.grads_as_lists(g[k])
            for name, x, ref, r32 in zip(NAMES, gcg + gag, list(cg) + ag, list(cg32) + ag32):
                e, e32 = _relerr(x, ref), _relerr(r32, ref)
                worst[name] = max(worst.get(name, 0.0), e)
                if e > max(SPLIT_TOL, 4 * e32):
                    errs[(w, k, name)] = (e, e32)
            lo = losses[k].cpu().numpy()
            print(f"weight {w} set {k}: losses {lo} oracle {p64['critic_loss']:.8g} {p64['actor_loss']:.8g}; anchor_loss {float(al[k]):.8g} "
                  f"oracle {p64['anchor_loss']:.8g}; clipped {p64['clipped']:.3f}")
            assert abs(lo[0] - p64["critic_loss"]) <= LOSS_TOL * abs(p64["critic_loss"])
            assert abs(lo[1] - p64["actor_loss"]) <= LOSS_TOL * max(1e-2, abs(p64["actor_loss"]))
            assert abs(float(al[k]) - p64["anchor_loss"]) <= LOSS_TOL * abs(p64["anchor_loss"])
    print("worst error per tensor:", {n_: f"{e:.1e}" for n_, e in worst.items()})
    return errs, worst, clipped


def _case(S, P, M, seed, weighted=False):
    conf, grp = _perturbed_group(M, S=S, seed=seed)
    rs = np.random.RandomState(seed + 1)
    n = P * M
    s, a, r, s2 = _batch(rs, n, S)
    _untie(grp, M, S, s, a)
    aw = None
    if weighted:  # the factors of a weighted federated mean: w_p P / sum_p w_p per set, agent-major
        w = (np.linspace(0.2, 3.0, P)[:, None].repeat(M, axis=1) * rs.uniform(0.8, 1.2, size=(P, M))).astype(np.float32)
        aw = (w * (P / w.sum(axis=0))).reshape(-1).astype(np.float32)
    return grp, n, (s, a, r, s2), aw


@pytest.mark.parametrize("S,P,M,weighted", [(4, 6, 2, False), (3, 5, 3, False), (4, 1, 1, False), (4, 70, 5, True), (4, 300, 1, False)])
def test_anchored_learner_matches_the_oracle(S, P, M, weighted):
    """(3, 5, 3): Model A; (4, 70, 5): ragged tile counts, non-uniform agent weights; (4, 300, 1): every workgroup on one set, so most
    waves of the seed kernel have no tile. A per-vehicle table with distinct rows, weights 0.5 and 10."""
    need_gpu()
    grp, n, (s, a, r, s2), aw = _case(S, P, M, 301, weighted)
    gains = _table(M)
    if S == 3:
        gains[:, 3] = 0.0
    batch = tuple(t(x) for x in (s, a, r, s2))
    got = {w: _anchored(grp, batch, n, gains, w, aw) for w in (0.5, 10.0)}
    for g, _, _ in got.values():
        assert torch.isfinite(g).all()
    errs, _, _ = _check_sets(grp, got, s, a, r, s2, P, M, range(M), gains, (0.5, 10.0), aw)
    assert not errs, errs


def test_anchored_learner_where_a_wave_walks_more_than_one_tile():
    """64 sets leave J = CUs // 64 = 4 workgroups per set; with P = 40 > 8 J a wave of the seed kernel takes a second tile. Table of 4
    rows: set j uses row j % 4. Sets 0, 5 and 63 against the oracle."""
    need_gpu()
    S, P, M = 4, 40, 64
    grp, n, (s, a, r, s2), _ = _case(S, P, M, 311)
    gains = _table(4)
    batch = tuple(t(x) for x in (s, a, r, s2))
    got = {10.0: _anchored(grp, batch, n, gains, 10.0)}
    errs, _, _ = _check_sets(grp, got, s, a, r, s2, P, M, (0, 5, 63), gains, (10.0,))
    assert not errs, errs


def test_a_clipped_target():
    """Gains large enough that most targets sit at an action bound: the clip is part of the target, not of the gradient."""
    need_gpu()
    S, P, M = 4, 6, 2
    grp, n, (s, a, r, s2), _ = _case(S, P, M, 321)
    gains = _table(M, scale=8.0)
    batch = tuple(t(x) for x in (s, a, r, s2))
    got = {w: _anchored(grp, batch, n, gains, w) for w in (0.5, 10.0)}
    errs, _, clipped = _check_sets(grp, got, s, a, r, s2, P, M, range(M), gains, (0.5, 10.0))
    assert clipped > 0.5, clipped
    assert not errs, errs


def test_weight_zero_is_the_unanchored_call_and_the_critic_block_never_changes():
    """weight 0: grads and losses torch.equal to learn_set_split on the same inputs, the anchor loss still the oracle's. Any weight:
    the critic block and both losses torch.equal to the un-anchored call's; two calls give the same bits in every output."""
    need_gpu()
    S, P, M = 4, 40, 5
    grp, n, (s, a, r, s2), aw = _case(S, P, M, 331, weighted=True)
    gains = _table(M)
    batch = tuple(t(x) for x in (s, a, r, s2))
    l0 = torch.zeros(M, 2, device="cuda")
    g0 = grp.learn_set_split(*batch, n, losses=l0, agent_weight=t(aw)).clone()
    A = grp.lay.actor_size
    zero = _anchored(grp, batch, n, gains, 0.0, aw)
    assert torch.equal(zero[0], g0) and torch.equal(zero[1], l0)
    _check_sets(grp, {0.0: zero}, s, a, r, s2, P, M, range(M), gains, (0.0,), aw)
    for w in (0.5, 10.0):
        g, lo, al = _anchored(grp, batch, n, gains, w, aw)
        assert torch.equal(g[:, A:], g0[:, A:]) and torch.equal(lo, l0), w
        assert not torch.equal(g[:, :A], g0[:, :A]), w  # (the anchor acts)
        assert torch.equal(al, zero[2]), w  # the anchor loss does not carry the weight
        g2, lo2, al2 = _anchored(grp, batch, n, gains, w, aw)
        for x, y in ((g, g2), (lo, lo2), (al, al2)):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), w


@pytest.mark.parametrize("how", ["ff", "nan"])
def test_a_dirty_workspace_and_slab_change_nothing(how):
    """As tests/test_gpu_fsplit_glue.py: the call on a workspace full of 0xFF bytes or NaNs, into a slab and an anchor loss full of
    NaNs, is bit for bit the call on zeroed memory."""
    need_gpu()
    from tests.test_gpu_fsplit_glue import _dirty, _workspace

    S, P, M = 4, 7, 3
    grp, n, (s, a, r, s2), _ = _case(S, P, M, 341)
    gains = _table(M)
    batch = tuple(t(x) for x in (s, a, r, s2))
    ws = _dirty(_workspace(grp, n), "zero")
    clean = _anchored(grp, batch, n, gains, 10.0, grads=torch.zeros(M, grp.lay.theta_size, device="cuda"))
    assert torch.isfinite(clean[0]).all() and torch.isfinite(clean[2]).all()
    _dirty(ws, how)
    ptr0 = ws.data_ptr()
    dirty = _anchored(grp, batch, n, gains, 10.0, grads=torch.full((M, grp.lay.theta_size), float("nan"), device="cuda"))
    assert grp._fsplit_ws.data_ptr() == ptr0
    for x, y in zip(clean, dirty):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), how


def test_a_seed_batch_set_uses_its_vehicles_row():
    """n_sets = 6, M = 3 (two experiments of three vehicles): set 4 = (experiment 1, vehicle 1) uses row 1. Its actor block and anchor
    loss equal those of a solo call on experiment 1's sets and agents whose table agrees in row 1 only. P = 5 <= J in both calls, so
    both reduce in the same order."""
    need_gpu()
    S, P, E, M = 4, 5, 2, 3
    grp, n, (s, a, r, s2), _ = _case(S, P, E * M, 351)
    gains = _table(M)
    big = _anchored(grp, tuple(t(x) for x in (s, a, r, s2)), n, gains, 10.0)
    conf, solo = _perturbed_group(M, S=S, seed=352)
    for dst, src in ((solo.theta, grp.theta), (solo.stats, grp.stats), (solo.theta_t, grp.theta_t), (solo.stats_t, grp.stats_t)):
        dst.copy_(src[M:2 * M])
    sel = (np.arange(P)[:, None] * (E * M) + M + np.arange(M)[None, :]).reshape(-1)  # experiment 1's agents, agent-major
    other = _table(M, seed=99)
    other[1] = gains[1]
    got = _anchored(solo, tuple(t(np.ascontiguousarray(x[sel])) for x in (s, a, r, s2)), P * M, other, 10.0)
    A = grp.lay.actor_size
    assert torch.equal(big[0][4, :A], got[0][1, :A]) and torch.equal(big[2][4], got[2][1])
    assert not torch.equal(big[0][3, :A], got[0][0, :A])  # (row 0 differs: the table matters)


def test_host_refusals_leave_every_output_untouched():
    """Everything the entry point refuses before its first HIP call, with the status and the text, on real device buffers: grads, losses
    and anchor_loss keep their sentinel."""
    need_gpu()
    S, P, M = 4, 3, 2
    grp, n, batch, _ = _case(S, P, M, 361)
    s, a, r, s2 = (t(x) for x in batch)
    gains = t(_table(M))
    need = ctypes.c_size_t(0)
    _hip.call("avd_learn_set_split_workspace", grp._layp, n, M, ctypes.byref(need))
    ws = torch.zeros(need.value, dtype=torch.uint8, device="cuda")
    grads = torch.full((M, grp.lay.theta_size), 3.0, device="cuda")
    losses, al = torch.full((M, 2), 3.0, device="cuda"), torch.full((M,), 3.0, device="cuda")
    p = _hip.ptr

    def go(lay=grp._layp, n_agents=n, n_sets=M, gains_=gains, Mt=M, lo=LO, hi=HI, weight=1.0, al_=al, theta=grp.theta, wsb=None):
        _hip.call("avd_learn_set_split_anchor_f16x3", lay, n_agents, n_sets, p(theta), p(grp.stats), p(grp.theta_t), p(grp.stats_t), p(s), p(a),
                  p(r), p(s2), None, 0.99, 2.5, p(grads), p(losses), p(ws), ws.numel() if wsb is None else wsb, p(gains_), Mt, 0, lo, hi,
                  weight, p(al_), _hip.stream_handle())

    who = "avd_learn_set_split_anchor_f16x3"
    refuse = lambda code, msg: pytest.raises(_hip.AvdError, match=rf"failed \({code}\): {who}: {msg}")
    wide = _hip.make_layout(4, 1, 320, 160, 48, 64)
    for code, msg, kw in ((-1, "null gains / anchor_loss", dict(gains_=None)), (-1, "null gains / anchor_loss", dict(al_=None)),
                          (-1, "n_sets=2 M=0", dict(Mt=0)), (-1, "n_sets=2 M=-1", dict(Mt=-1)), (-1, "n_sets=2 M=3", dict(Mt=3)),
                          (-1, "weight=-0.5", dict(weight=-0.5)), (-1, "weight=inf", dict(weight=float("inf"))),
                          (-1, "weight=-?nan", dict(weight=float("nan"))), (-1, r"lo=2.5 > hi=-2.5", dict(lo=HI, hi=LO)),
                          (-1, "null layout", dict(lay=None)), (-1, "n_agents=5 n_sets=2", dict(n_agents=5)),
                          (-1, "n_agents=6 n_sets=65", dict(n_sets=65, Mt=1)), (-3, "serves the reference widths only", dict(lay=ctypes.byref(wide))),
                          (-1, "null pointer", dict(theta=None)), (-1, "workspace 16 B <", dict(wsb=16))):
        with refuse(code, msg):
            go(**kw)
    torch.cuda.synchronize()
    assert bool((grads == 3.0).all()) and bool((losses == 3.0).all()) and bool((al == 3.0).all())
    go()  # and the same buffers are accepted when nothing is wrong
    torch.cuda.synchronize()
    assert torch.isfinite(grads).all() and bool((al != 3.0).all())
