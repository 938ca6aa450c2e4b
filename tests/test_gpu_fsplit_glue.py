"""The split learner's glue (csrc/fsplit.hip: front_kernel, prep_kernel; csrc/fset.hip: finalize) asks nothing of the state its
workspace and its gradient slab are in when a learn call begins. Until r09 two memsets per call hid that: one zeroed the slab (finalize
never writes the padding between its tensors), one zeroed the `bad` flag and the words the scale step took its maxima into with
atomicMax. Now the front launch writes every word a later kernel reads -- per-slice maxima with plain stores, one flag word per wave
of the roles that test inputs, `bad` cleared by one designated block, the slab zeroed by blocks of its own -- and these tests hold
it to that: a call on a workspace full of 0xFF bytes or NaNs, into a slab full of garbage, after a call with other weights, is bit
for bit the call on fresh zeroed memory; and the conditions that used to set `bad` from the fused roles still turn the slab to NaN.
Every case checks on its own inputs that it runs the path it is about (the workspace really is the dirty one, the slab really has
padding, the poisoned value really sits where the pack / prep1 role reads it)."""
import ctypes

import numpy as np
import pytest
import torch

from avddpg_amd import params
from avddpg_amd._hip import call
from tests.gpu_util import need_gpu, t
from tests.test_gpu_fset import _batch
from tests.test_gpu_mlp import _perturbed_group

pytestmark = pytest.mark.gpu

P, M, S = 7, 3, 4  # 21 agents: an odd count, so the last pack block of each input is half empty (its flag words are still written)


def _bits(x):
    return x.contiguous().view(torch.int32)


def _workspace(grp, n_agents):
    """The group's split-learner workspace, allocated at exactly the size the library reports (so that learn_set_fused keeps it)."""
    need = ctypes.c_size_t(0)
    call("avd_learn_set_split_workspace", grp._layp, n_agents, grp.n_sets, ctypes.byref(need))
    ws = getattr(grp, "_fsplit_ws", None)
    if ws is None or ws.numel() < need.value:
        ws = grp._fsplit_ws = torch.zeros(need.value, dtype=torch.uint8, device="cuda")
    assert ws.numel() % 4 == 0
    return ws


def _dirty(ws, how):
    if how == "zero":
        ws.zero_()
    elif how == "ff":
        ws.fill_(0xFF)  # every flag word non-zero, every float a negative quiet NaN, every stored maximum 0xffffffff
    elif how == "nan":
        ws.view(torch.float32).fill_(float("nan"))  # 0x7fc00000: as a maximum's bits it beats any finite float
    else:  # a huge finite float: as a stale maximum it would scale every weight to zero
        ws.view(torch.float32).fill_(3.0e38)
    return ws


def _learn(grp, batch, n, how, two_phase=False, grads=None, **kw):
    """One learn call (or the critic / actor pair) on the group's workspace brought into state `how` first; asserts that the call
    ran on that very buffer. Returns (grads, losses) as clones."""
    ws = _dirty(_workspace(grp, n), how)
    ptr0 = ws.data_ptr()
    if how == "ff":
        assert bool((ws == 0xFF).all())
    losses = torch.full((grp.n_sets, 2), 7.0, device="cuda")
    if two_phase:
        g = grp.learn_set_fused(*batch, n, grads=grads, losses=losses, split=True, phase="critic", **kw)
        g = grp.learn_set_fused(*batch, n, grads=g, split=True, phase="actor")
    else:
        g = grp.learn_set_split(*batch, n, grads=grads, losses=losses, **kw)
    torch.cuda.synchronize()
    assert grp._fsplit_ws.data_ptr() == ptr0, "the call replaced the workspace: the dirty one was not used"
    return g.clone(), losses.clone()


def _padding_mask(lay):
    """[theta_size] bool: the floats of a weight set's slab that belong to no trainable tensor (every tensor starts on a 4-float
    boundary: include/avddpg_hip.h)."""
    pad = np.ones(lay.theta_size, bool)
    p = params.logical_dims(lay)
    for name, kind, shp in params.ACTOR_WEIGHTS + params.CRITIC_WEIGHTS:
        if kind == "t":
            off = params._offset(lay, name, kind)
            pad[off:off + int(np.prod(shp(p)))] = False
    return pad


@pytest.mark.parametrize("two_phase", [False, True])
@pytest.mark.parametrize("how", ["ff", "nan", "huge"])
def test_a_dirty_workspace_gives_the_bits_of_a_zeroed_one(how, two_phase):
    need_gpu()
    conf, grp = _perturbed_group(M, S=S, seed=201)
    n = P * M
    batch = tuple(t(x) for x in _batch(np.random.RandomState(202), n, S))
    g0, l0 = _learn(grp, batch, n, "zero", two_phase)
    assert torch.isfinite(g0).all() and torch.isfinite(l0).all() and g0.abs().max() > 0
    g1, l1 = _learn(grp, batch, n, how, two_phase)
    assert torch.equal(_bits(g0), _bits(g1)), how
    assert torch.equal(_bits(l0), _bits(l1)), how


@pytest.mark.parametrize("S_", [4, 3])
@pytest.mark.parametrize("two_phase", [False, True])
def test_a_garbage_slab_comes_back_with_exactly_zero_padding(two_phase, S_):
    need_gpu()
    conf, grp = _perturbed_group(M, S=S_, seed=203)
    lay = grp.lay
    n = P * M
    batch = tuple(t(x) for x in _batch(np.random.RandomState(204), n, S_))
    pad = torch.from_numpy(_padding_mask(lay)).cuda()
    assert int(pad.sum()) >= 6, "this layout has no padding: the case tests nothing"  # (b3 of both nets alone leaves 2 x 3 floats)
    clean, _ = _learn(grp, batch, n, "zero", two_phase, grads=torch.zeros(M, lay.theta_size, device="cuda"))
    for fill in (float("nan"), 3.0e38, -1.0):
        slab = torch.full((M, lay.theta_size), fill, device="cuda")
        got, _ = _learn(grp, batch, n, "ff", two_phase, grads=slab)
        assert got.data_ptr() != slab.data_ptr() and torch.equal(_bits(slab), _bits(got))  # (the call wrote into the slab it was given)
        assert bool((_bits(got)[:, pad] == 0).all()), fill  # +0.0, bit for bit
        assert torch.equal(_bits(got), _bits(clean)), fill


@pytest.mark.parametrize("two_phase", [False, True])
@pytest.mark.parametrize("where", ["s", "s2", "a", "r", "s_last_row", "b1"])
def test_the_front_roles_flags_still_turn_the_slab_to_nan(where, two_phase):
    """What pack_x and prep1 used to report with atomicOr(bad) now travels through their waves' flag words and prep_kernel: a
    non-finite input, an input (or a first-layer bias times 64) beyond fp16's range -> NaN over the slab; the same value just below
    the limit -> finite gradients. The workspace is dirty before every call, so a flag word can only be zero if its wave wrote it."""
    need_gpu()
    conf, grp = _perturbed_group(M, S=S, seed=205)
    lay = grp.lay
    n = P * M
    s, a, r, s2 = (t(x) for x in _batch(np.random.RandomState(206), n, S))
    big = [(lay.aW2, lay.aW2 + 256 * 128), (lay.actor_size + lay.cW2, lay.actor_size + lay.cW2 + 304 * 128)]

    if where == "b1":  # feature 200 of the target actor's first layer sees no input: its activation is the bias itself
        for k in range(S):
            grp.theta_t[M - 1, lay.aW1 + k * 256 + 200] = 0.0

    def poke(v):
        if where == "b1":  # prep1's role: S1 b = 64 b against 65520
            grp.theta_t[M - 1, lay.ab1 + 200] = v / 64.0
        elif where == "s_last_row":  # the last row of the batch: the half-empty last pack block of input 0
            s.view(-1)[-1] = v
        else:
            {"s": s, "s2": s2, "a": a, "r": r}[where].view(-1)[4 * 333 + 2] = v

    assert (2 * n * 64) % 256 != 0  # (the last pack block of each input is half empty)
    overflow = where != "r"  # r is only tested for finiteness: it never becomes an fp16 operand
    if where in ("r", "b1"):
        # the control: 64 b = 65000 is just below F16_OVERFLOW = 65520 (the largest finite fp16 is 65504); a large finite reward.
        # (A state or an action of 65000 overflows an ACTIVATION further on, which the heads catch; their control is
        #  test_just_below_the_fp16_limit_an_input_stays_finite.)
        poke(65000.0 if overflow else 1.0e6)
        g, lo = _learn(grp, (s, a, r, s2), n, "ff", two_phase)
        assert torch.isfinite(g).all(), where
    poisons = [70000.0, float("inf"), float("nan")] if overflow else [float("inf"), float("nan")]
    for v in poisons:
        poke(v)
        g, lo = _learn(grp, (s, a, r, s2), n, "ff", two_phase)
        for lo_, hi_ in big:
            assert torch.isnan(g[:, lo_:hi_]).all(), (where, v)
    # and the flag does not stick: the same workspace, clean inputs again
    poke(0.25)
    g, lo = _learn(grp, (s, a, r, s2), n, "ff", two_phase)
    assert torch.isfinite(g).all(), where


def test_just_below_the_fp16_limit_an_input_stays_finite():
    """The control of the overflow cases on a path where nothing downstream can overflow either: the poked state feeds weights that
    are zero for that input column, so 65000 reaches pack's test (< 65520: passes) and no activation grows from it; 65520 fails."""
    need_gpu()
    conf, grp = _perturbed_group(M, S=S, seed=207)
    lay = grp.lay
    n = P * M
    s, a, r, s2 = (t(x) for x in _batch(np.random.RandomState(208), n, S))
    for th in (grp.theta, grp.theta_t):  # input column 3 of both first layers, online and target: unused
        th[:, lay.aW1 + 3 * 256:lay.aW1 + 4 * 256] = 0.0
        th[:, lay.actor_size + lay.cWs + 3 * 256:lay.actor_size + lay.cWs + 4 * 256] = 0.0
    ref, _ = _learn(grp, (s, a, r, s2), n, "ff")
    assert torch.isfinite(ref).all()
    for x in (s, s2):
        x[5, 17, 3] = 65000.0
    g, _ = _learn(grp, (s, a, r, s2), n, "ff")
    assert torch.isfinite(g).all()
    s[5, 17, 3] = 65520.0
    g, _ = _learn(grp, (s, a, r, s2), n, "ff")
    assert torch.isnan(g[:, lay.aW2:lay.aW2 + 256 * 128]).all()


@pytest.mark.parametrize("two_phase", [False, True])
def test_two_calls_on_one_workspace_each_give_the_result_of_a_fresh_one(two_phase):
    """Stale per-slice maxima: the second call's second-layer weights are 1/64 of the first's (then 4096 x), so a maximum left over
    from the other call would move SW / SWC by six (twelve) binary orders -- out of fp16's range on one side, into its subnormals
    on the other."""
    need_gpu()
    n = P * M
    batch = tuple(t(x) for x in _batch(np.random.RandomState(210), n, S))
    conf, grp = _perturbed_group(M, S=S, seed=209)
    lay = grp.lay
    w2 = [(lay.aW2, lay.aW2 + 256 * 128), (lay.actor_size + lay.cW2, lay.actor_size + lay.cW2 + 304 * 128)]
    theta0, theta_t0 = grp.theta.clone(), grp.theta_t.clone()

    def set_scale(k):
        grp.theta.copy_(theta0), grp.theta_t.copy_(theta_t0)
        for th in (grp.theta, grp.theta_t):
            for lo, hi in w2:
                th[:, lo:hi] *= k

    fresh = {}
    for k in (1.0, 1.0 / 64, 64.0):
        set_scale(k)
        fresh[k] = _learn(grp, batch, n, "zero", two_phase)
        assert torch.isfinite(fresh[k][0]).all()
    assert not torch.equal(fresh[1.0][0], fresh[1.0 / 64][0]) and not torch.equal(fresh[1.0][0], fresh[64.0][0])
    ws = _workspace(grp, n)
    for k in (1.0, 1.0 / 64, 64.0, 1.0):  # back to back, the workspace left as the call before left it
        set_scale(k)
        ptr0 = ws.data_ptr()
        losses = torch.zeros(M, 2, device="cuda")
        if two_phase:
            g = grp.learn_set_fused(*batch, n, losses=losses, split=True, phase="critic")
            g = grp.learn_set_fused(*batch, n, grads=g, split=True, phase="actor")
        else:
            g = grp.learn_set_split(*batch, n, losses=losses)
        torch.cuda.synchronize()
        assert grp._fsplit_ws.data_ptr() == ptr0
        assert torch.equal(_bits(g), _bits(fresh[k][0])) and torch.equal(_bits(losses), _bits(fresh[k][1])), k
