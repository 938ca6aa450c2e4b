"""The TD-only learn call of the split set learner (avd_learn_set_split_td_f16x3, AgentGroup.learn_set_split_td) against the calls it
is cut from, BIT FOR BIT: its critic block and critic loss are avd_learn_set_split_critic's (un-smoothed) and
avd_learn_set_split_smooth_f16x3's (smoothed, same key and counter) on the same inputs; its actor block is all zero and its actor loss
0. No tolerance of its own: those two calls are the yardsticks, and they are tested against the float64 oracle in
tests/test_gpu_fsplit.py and tests/test_gpu_smooth.py. Then: a workspace and a slab that hold anything, non-finite inputs, and what the
entry point refuses on the host.

Shapes (S, P, M, weighted): tests/test_gpu_smooth.py's -- (3, 5, 3): Model A; (4, 1, 1): one tile; (4, 70, 5): ragged tile counts,
non-uniform agent weights."""
import ctypes
import math

import pytest
import torch

from avddpg_amd import _hip
from avddpg_amd.trainer import TargetNoise
from avddpg_amd.vec import seed_table
from tests.gpu_util import need_gpu, t
from tests.test_gpu_anchor import _case

pytestmark = pytest.mark.gpu

LO, HI = -2.5, 2.5
SHAPES = [(4, 6, 2, False), (3, 5, 3, False), (4, 1, 1, False), (4, 70, 5, True)]


def _bits(x):
    return x.contiguous().view(torch.int32)


def _td(grp, batch, n, aw=None, noise=None, counter=0, grads=None, seed=3, M=None, d_seeds=None):
    """One TD-only call -> (grads, losses), clones; the losses start from a sentinel."""
    losses = torch.full((grp.n_sets, 2), 7.0, device="cuda")
    g = grp.learn_set_split_td(*batch, n, noise=noise, counter=counter, grads=grads, losses=losses, agent_weight=None if aw is None else t(aw),
                               M=M, seed=seed, d_seeds=d_seeds)
    torch.cuda.synchronize()
    return g.clone(), losses.clone()


def _assert_td_of(td, ref, A, what):
    """td (grads, losses) of the TD-only call against ref (grads, losses) of a full or critic-phase call"""
    g, lo = td
    assert torch.isfinite(ref[0]).all(), what
    assert torch.equal(_bits(g[:, A:]), _bits(ref[0][:, A:])), (what, "critic block")
    assert torch.equal(_bits(lo[:, 0]), _bits(ref[1][:, 0])), (what, "critic loss")
    assert bool((_bits(g[:, :A]) == 0).all()), (what, "actor block")  # +0.0, every bit: the front launch's zeros
    assert bool((lo[:, 1] == 0).all()), (what, "actor loss")
    assert bool((g[:, A:] != 0).any(dim=1).all()), what


@pytest.mark.parametrize("S,P,M,weighted", SHAPES)
def test_td_call_is_the_critic_phase_bit_for_bit(S, P, M, weighted):
    need_gpu()
    grp, n, (s, a, r, s2), aw = _case(S, P, M, 501, weighted)
    batch = tuple(t(x) for x in (s, a, r, s2))
    A = grp.lay.actor_size
    lc = torch.full((M, 2), 7.0, device="cuda")
    gc = grp.learn_set_fused(*batch, n, losses=lc, agent_weight=None if aw is None else t(aw), split=True, phase="critic").clone()
    torch.cuda.synchronize()
    td = _td(grp, batch, n, aw)
    _assert_td_of(td, (gc, lc), A, "critic phase")
    # sigma 0 with a noise object: no smoothing launch, the same bits; and two calls agree
    for other in (_td(grp, batch, n, aw, noise=TargetNoise(0.0), counter=9), _td(grp, batch, n, aw)):
        assert torch.equal(_bits(other[0]), _bits(td[0])) and torch.equal(_bits(other[1]), _bits(td[1]))


@pytest.mark.parametrize("S,P,M,weighted", SHAPES)
def test_smoothed_td_call_is_the_smoothed_calls_critic_block_bit_for_bit(S, P, M, weighted):
    need_gpu()
    grp, n, (s, a, r, s2), aw = _case(S, P, M, 511, weighted)
    batch = tuple(t(x) for x in (s, a, r, s2))
    A = grp.lay.actor_size
    tn = TargetNoise(0.2, 0.5)
    ls = torch.full((M, 2), 7.0, device="cuda")
    gs = grp.learn_set_split_smooth(*batch, n, tn, 6, losses=ls, agent_weight=None if aw is None else t(aw), seed=3).clone()
    torch.cuda.synchronize()
    td = _td(grp, batch, n, aw, noise=tn, counter=6, seed=3)
    _assert_td_of(td, (gs, ls), A, "smoothed call")
    plain = _td(grp, batch, n, aw)
    assert not torch.equal(plain[0][:, A:], td[0][:, A:])  # (the noise acts)
    assert not torch.equal(_td(grp, batch, n, aw, noise=tn, counter=7, seed=3)[0][:, A:], td[0][:, A:])  # (and the counter keys it)


def test_a_seed_table_keys_the_td_call_like_the_smoothed_call():
    """n_sets = 6 = 2 experiments x 3 vehicles with a seed table: still the smoothed call's critic block, bit for bit."""
    need_gpu()
    S, P, E, M = 4, 5, 2, 3
    grp, n, (s, a, r, s2), _ = _case(S, P, E * M, 521)
    batch = tuple(t(x) for x in (s, a, r, s2))
    tn, tab = TargetNoise(1.5, 3.0), seed_table((61, 62), "cuda")[1]
    ls = torch.zeros(E * M, 2, device="cuda")
    gs = grp.learn_set_split_smooth(*batch, n, tn, 3, losses=ls, M=M, d_seeds=tab).clone()
    torch.cuda.synchronize()
    _assert_td_of(_td(grp, batch, n, noise=tn, counter=3, M=M, d_seeds=tab), (gs, ls), grp.lay.actor_size, "seed batch")


@pytest.mark.parametrize("how", ["ff", "nan"])
def test_a_dirty_workspace_and_slab_change_nothing(how):
    need_gpu()
    from tests.test_gpu_fsplit_glue import _dirty, _workspace

    S, P, M = 4, 7, 3
    grp, n, (s, a, r, s2), _ = _case(S, P, M, 531)
    batch = tuple(t(x) for x in (s, a, r, s2))
    tn = TargetNoise(1.5, 3.0)
    ws = _dirty(_workspace(grp, n), "zero")
    clean = _td(grp, batch, n, noise=tn, counter=1, grads=torch.zeros(M, grp.lay.theta_size, device="cuda"))
    assert torch.isfinite(clean[0]).all()
    _dirty(ws, how)
    ptr0 = ws.data_ptr()
    dirty = _td(grp, batch, n, noise=tn, counter=1, grads=torch.full((M, grp.lay.theta_size), float("nan"), device="cuda"))
    assert grp._fsplit_ws.data_ptr() == ptr0
    for x, y in zip(clean, dirty):
        assert torch.equal(_bits(x), _bits(y)), how


@pytest.mark.parametrize("where", ["s2", "theta_t", "s"])
def test_a_non_finite_input_still_gives_a_non_finite_critic_head(where):
    """What the guarded update looks at: element 0 of every set's critic block (the whole block and the critic loss are NaN)."""
    need_gpu()
    S, P, M = 4, 5, 2
    grp, n, (s, a, r, s2), _ = _case(S, P, M, 541)
    batch = [t(x) for x in (s, a, r, s2)]
    tn = TargetNoise(0.2)
    assert torch.isfinite(_td(grp, batch, n, noise=tn)[0]).all()
    if where == "theta_t":
        grp.theta_t[1, grp.lay.aW2 + 777] = float("nan")
    else:
        batch[{"s": 0, "s2": 3}[where]].view(-1)[321] = float("nan")
    g, lo = _td(grp, batch, n, noise=tn)
    A = grp.lay.actor_size
    assert not torch.isfinite(g[:, A]).any() and torch.isnan(g[:, A + grp.lay.cW2:A + grp.lay.cW2 + 304 * 128]).all()
    assert torch.isnan(lo[:, 0]).all()


def test_host_refusals_leave_every_output_untouched():
    need_gpu()
    p = _hip.ptr
    S, P, M = 4, 3, 2
    grp, n, batch, _ = _case(S, P, M, 551)
    s, a, r, s2 = (t(x) for x in batch)
    seeds = seed_table((1, 2), "cuda")[1]
    need = ctypes.c_size_t(0)
    _hip.call("avd_learn_set_split_workspace", grp._layp, n, M, ctypes.byref(need))
    ws = torch.zeros(need.value, dtype=torch.uint8, device="cuda")
    grads = torch.full((M, grp.lay.theta_size), 3.0, device="cuda")
    losses = torch.full((M, 2), 3.0, device="cuda")

    def go(lay=grp._layp, n_agents=n, n_sets=M, Mt=M, lo=LO, hi=HI, theta=grp.theta, s2_=s2, wsb=None, sigma=0.2, clip=0.5, tab=None, E=1):
        _hip.call("avd_learn_set_split_td_f16x3", lay, n_agents, n_sets, p(theta), p(grp.stats), p(grp.theta_t), p(grp.stats_t), p(s), p(a), p(r),
                  p(s2_), None, 0.99, 2.5, p(grads), p(losses), p(ws), ws.numel() if wsb is None else wsb, sigma, clip, lo, hi, 1, 0, p(tab), E,
                  Mt, _hip.stream_handle())

    who = "avd_learn_set_split_td_f16x3"
    refuse = lambda code, msg: pytest.raises(_hip.AvdError, match=rf"failed \({code}\): {who}: {msg}")
    wide = _hip.make_layout(4, 1, 320, 160, 48, 64)
    for code, msg, kw in ((-1, "M=0 E=1", dict(Mt=0)), (-1, "M=2 E=0", dict(E=0)), (-1, "n_sets=2 M=2 E=2", dict(E=2, tab=seeds)),
                          (-1, "E=2 without a seed table", dict(E=2, Mt=1)), (-1, "sigma=-0.2", dict(sigma=-0.2)),
                          (-1, "sigma=inf", dict(sigma=math.inf)), (-1, "sigma=-?nan", dict(sigma=math.nan)), (-1, "noise_clip=0 ", dict(clip=0.0)),
                          (-1, "noise_clip=-?nan", dict(clip=math.nan)), (-1, "lo=2.5 > hi=-2.5", dict(lo=HI, hi=LO)),
                          (-1, "null layout", dict(lay=None)), (-1, "n_agents=5 n_sets=2", dict(n_agents=5)),
                          (-3, "serves the reference widths only", dict(lay=ctypes.byref(wide))), (-1, "null pointer", dict(theta=None)),
                          (-1, "null pointer", dict(s2_=None)), (-1, "workspace 16 B <", dict(wsb=16))):
        with refuse(code, msg):
            go(**kw)
    torch.cuda.synchronize()
    assert bool((grads == 3.0).all()) and bool((losses == 3.0).all())
    go(E=2, Mt=1, tab=seeds)  # accepted: a table and a seed batch's layout
    torch.cuda.synchronize()
    A = grp.lay.actor_size
    assert torch.isfinite(grads).all() and bool((grads[:, :A] == 0).all()) and bool((losses[:, 1] == 0).all()) and bool((losses[:, 0] != 3.0).all())
