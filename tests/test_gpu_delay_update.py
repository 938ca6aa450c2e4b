"""The delayed update (avd_adam_polyak_delayed_f32, csrc/optim.hip) against tests/delay_oracle.py, BIT FOR BIT, from a run in progress
(step 5, actor_step 2, non-zero moments, targets that differ from their nets): a d = 3 schedule of seven calls, policy calls against
avd_adam_polyak_guarded_f32 on a twin, a skipped call whose actor gradients are NaN, and the guard of either kind of call.

Layouts: the reference widths at S = 4 (what the trainer runs) and the small layout of tests/test_gpu_optim_kernels.py, whose
actor_size / 4 = 2053 is no multiple of 256 -- a skipped call's first workgroup then starts inside a 256-group block of the slab.
n_sets 1, 3 and 257: the last takes the capped grid (eight workgroups per set striding over the block)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from avddpg_amd import _hip
from avddpg_amd._hip import call, ptr, stream_handle
from tests import delay_oracle as do
from tests.gpu_util import need_gpu

pytestmark = pytest.mark.gpu
ACTOR_LR, CRITIC_LR, TAU = 1e-4, 1e-3, 0.005  # (different step sizes: an actor / critic mix-up at the boundary shows)
ARRAYS = ("theta", "theta_t", "m", "v", "stats_t", "stats", "step", "actor_step")


@functools.lru_cache(None)
def _layout(name):
    if name == "reference":
        return _hip.make_layout(4, 1, 256, 128, 48, 64)
    lay = _hip.make_layout(4, 1, 112, 64, 16, 64)
    assert (lay.actor_size // 4) % 256 and lay.actor_size % 4 == 0 and (lay.theta_size - lay.actor_size) // 4 > 8 * 256
    return lay


CASES = [(name, n) for name in ("reference", "small") for n in (1, 3, 257)]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


class _Dev:
    """device copies of a host state"""

    def __init__(self, h):
        for k, x in h.items():
            setattr(self, k, torch.from_numpy(np.ascontiguousarray(x)).cuda())
        self.skipped = torch.zeros(1, dtype=torch.int32, device="cuda")

    def delayed(self, lay, grads, policy):
        """AgentGroup.apply_delayed: the caller advances the counts a call uses"""
        self.step += 1
        if policy:
            self.actor_step += 1
        self.g = torch.from_numpy(grads).cuda()
        call("avd_adam_polyak_delayed_f32", C.byref(lay), self.theta.shape[0], ptr(self.theta), ptr(self.stats), ptr(self.theta_t),
             ptr(self.stats_t), ptr(self.m), ptr(self.v), ptr(self.g), ptr(self.step), ptr(self.actor_step), 1 if policy else 0, ACTOR_LR,
             CRITIC_LR, TAU, ptr(self.skipped), stream_handle())

    def guarded(self, lay, grads):
        self.step += 1
        self.g = torch.from_numpy(grads).cuda()
        call("avd_adam_polyak_guarded_f32", C.byref(lay), self.theta.shape[0], ptr(self.theta), ptr(self.stats), ptr(self.theta_t),
             ptr(self.stats_t), ptr(self.m), ptr(self.v), ptr(self.g), ptr(self.step), ACTOR_LR, CRITIC_LR, TAU, ptr(self.skipped),
             stream_handle())

    def host(self):
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy() for k in ARRAYS}


def _start(name, n_sets, seed, **kw):
    lay = _layout(name)
    h, scale, rs = do.host_state(n_sets, lay.theta_size, lay.stats_size, seed, **kw)
    return lay, h, scale, rs


def _assert_same(got, want, what):
    for k in ARRAYS:
        diff = (_bits(got[k]) != _bits(want[k])).reshape(got[k].shape[0], -1)
        assert not diff.any(), (what, k, "sets", np.nonzero(diff.any(axis=1))[0][:8], "first element", int(np.argmax(diff.any(axis=0))))


@pytest.mark.parametrize("name,n_sets", CASES)
def test_seven_calls_at_delay_three_match_the_oracle_bit_for_bit(name, n_sets):
    """Calls 3 and 6 are policy calls. After every call: theta, theta_t, m, v, stats_t and both counts against the oracle."""
    need_gpu()
    lay, h, scale, rs = _start(name, n_sets, seed=21 + n_sets)
    d = _Dev(h)
    for k, policy in enumerate(do.schedule(7, 3)):
        g = do.gradients(scale, rs)
        d.delayed(lay, g, policy)
        assert do.delayed_call(h, g, policy, lay.actor_size, ACTOR_LR, CRITIC_LR, TAU) == 0
        _assert_same(d.host(), h, f"call {k} policy={policy}")
    assert h["step"].tolist() == [12] * n_sets and h["actor_step"].tolist() == [4] * n_sets and int(d.skipped.item()) == 0


@pytest.mark.parametrize("name,n_sets", CASES)
def test_policy_calls_with_equal_counts_are_the_guarded_update_bit_for_bit(name, n_sets):
    """Six policy calls with actor_step == step against avd_adam_polyak_guarded_f32 on a twin: the same element step, the same step
    sizes."""
    need_gpu()
    lay, h, scale, rs = _start(name, n_sets, seed=31 + n_sets, step=5, actor_step=5)
    d, twin = _Dev(h), _Dev(h)
    for k in range(6):
        g = do.gradients(scale, rs)
        d.delayed(lay, g, True)
        twin.guarded(lay, g)
        got, want = d.host(), twin.host()
        want["actor_step"] = want["step"]
        _assert_same(got, want, f"call {k}")
    assert not np.array_equal(_bits(got["theta"]), _bits(h["theta"])) and got["step"].tolist() == [11] * n_sets


@pytest.mark.parametrize("name,n_sets", CASES)
def test_a_skipped_call_never_looks_at_the_actor_block(name, n_sets):
    """The actor block of the gradients is all NaN: the update proceeds (nothing is guarded), and every actor-side array, every target
    and stats_t keep their bits; the critic block is the oracle's."""
    need_gpu()
    lay, h, scale, rs = _start(name, n_sets, seed=41 + n_sets)
    A = lay.actor_size
    g = do.gradients(scale, rs)
    g[:, :A] = np.nan
    before = {k: x.copy() for k, x in h.items()}
    d = _Dev(h)
    d.delayed(lay, g, False)
    got = d.host()
    assert do.delayed_call(h, g, False, A, ACTOR_LR, CRITIC_LR, TAU) == 0 and int(d.skipped.item()) == 0
    _assert_same(got, h, "skipped call")
    for k in ("theta", "m", "v"):
        assert np.array_equal(_bits(got[k][:, :A]), _bits(before[k][:, :A])), k
        assert (_bits(got[k][:, A:]) != _bits(before[k][:, A:])).any(axis=1).all(), k  # every set's critic stepped
    for k in ("theta_t", "stats_t", "stats", "actor_step"):
        assert np.array_equal(_bits(got[k]), _bits(before[k])), k
    assert np.array_equal(got["step"], before["step"] + 1)


@pytest.mark.parametrize("name,n_sets", [c for c in CASES if c[1] > 1])
def test_a_non_finite_critic_head_on_a_skipped_call_guards_that_set_alone(name, n_sets):
    """The set is untouched, step put back, actor_step untouched, skipped == 1; the other sets match the oracle. A NaN at the ACTOR
    block's head of another set is not looked at."""
    need_gpu()
    lay, h, scale, rs = _start(name, n_sets, seed=51 + n_sets)
    A = lay.actor_size
    g = do.gradients(scale, rs)
    bad, other = n_sets - 1, 0
    g[bad, A] = np.nan
    g[other, 0] = np.nan
    before = {k: x.copy() for k, x in h.items()}
    d = _Dev(h)
    d.delayed(lay, g, False)
    got = d.host()
    assert do.delayed_call(h, g, False, A, ACTOR_LR, CRITIC_LR, TAU) == 1 and int(d.skipped.item()) == 1
    _assert_same(got, h, "guarded skipped call")
    for k in ARRAYS:
        assert np.array_equal(_bits(got[k][bad]), _bits(before[k][bad])), k
    assert got["step"][bad] == 5 and got["step"][other] == 6 and got["actor_step"].tolist() == [2] * n_sets


@pytest.mark.parametrize("name,n_sets", [c for c in CASES if c[1] > 1])
def test_a_non_finite_actor_head_on_a_policy_call_puts_both_counts_back(name, n_sets):
    need_gpu()
    lay, h, scale, rs = _start(name, n_sets, seed=61 + n_sets)
    A = lay.actor_size
    g = do.gradients(scale, rs)
    bad_a, bad_c = 1, n_sets - 1
    g[bad_a, 0] = -np.inf
    g[bad_c, A] = np.nan
    before = {k: x.copy() for k, x in h.items()}
    d = _Dev(h)
    d.delayed(lay, g, True)
    got = d.host()
    assert do.delayed_call(h, g, True, A, ACTOR_LR, CRITIC_LR, TAU) == 2 and int(d.skipped.item()) == 2
    _assert_same(got, h, "guarded policy call")
    for s in (bad_a, bad_c):
        for k in ARRAYS:
            assert np.array_equal(_bits(got[k][s]), _bits(before[k][s])), (s, k)
        assert got["step"][s] == 5 and got["actor_step"][s] == 2
    assert got["step"][0] == 6 and got["actor_step"][0] == 3
