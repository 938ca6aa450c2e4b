"""Every form of the split set learner through the public AgentGroup methods, on one set of inputs and weights: which C entry point each
form reaches, the bit-for-bit equalities the methods' docstrings promise between the forms, and that what the workspace and the gradient
slab held before a call changes nothing.

The shape is the smallest the learner accepts that still has one tile per workgroup, more than one workgroup per set and more than one
set: two weight sets, four agents per set (n_agents = 8, B = 64; J = min(CUs // 2, 4) = 4 workgroups per set), at S = 3 and S = 4. The
sweep's table is the smallest with more than one row: two experiments of one set each, conf's values in both rows.

The forms:
  1 plain single call            learn_set_split                              avd_learn_set_split_f16x3
  2 critic phase, actor phase    learn_set_fused(split=True, phase=...)       avd_learn_set_split_critic, avd_learn_set_split_actor
  3 smoothed, sigma 0            learn_set_split_smooth                       avd_learn_set_split_smooth_f16x3
  4 smoothed, sigma > 0          learn_set_split_smooth                       avd_learn_set_split_smooth_f16x3
  5 anchored                     learn_set_split_anchor                       avd_learn_set_split_anchor_f16x3
  6 smoothed and anchored        learn_set_split_smooth(anchor=...)           avd_learn_set_split_smooth_f16x3
  7 TD-only                      learn_set_split_td                           avd_learn_set_split_td_f16x3
  8 TD-only with noise           learn_set_split_td(noise=...)                avd_learn_set_split_td_f16x3
  9 sweep, conf's gamma per row  learn_set_split after set_hparams            avd_learn_set_split_hp_f16x3
Every form runs twice, once on a zeroed workspace and slab and once on both filled with NaN bytes. Nothing is timed."""
import copy
import functools

import numpy as np
import pytest
import torch

from avddpg_amd import vec
from avddpg_amd.trainer import TargetNoise
from tests.gpu_util import need_gpu, t
from tests.test_gpu_anchor import _table
from tests.test_gpu_fset import _batch
from tests.test_gpu_fsplit_glue import _bits, _dirty, _workspace
from tests.test_gpu_mlp import _perturbed_group

pytestmark = pytest.mark.gpu

N_SETS, P = 2, 4
N = N_SETS * P
ENTRIES = {1: ["avd_learn_set_split_f16x3"], 2: ["avd_learn_set_split_critic", "avd_learn_set_split_actor"],
           3: ["avd_learn_set_split_smooth_f16x3"], 4: ["avd_learn_set_split_smooth_f16x3"], 5: ["avd_learn_set_split_anchor_f16x3"],
           6: ["avd_learn_set_split_smooth_f16x3"], 7: ["avd_learn_set_split_td_f16x3"], 8: ["avd_learn_set_split_td_f16x3"],
           9: ["avd_learn_set_split_hp_f16x3"]}
NOT_LEARN = ("avd_learn_set_split_workspace", "avd_learn_set_split_mfma_count")


@functools.lru_cache(maxsize=None)
def _forms(S):
    """{(form, how): (grads, losses, the C entries reached)} for how in ("zero", "nan"), every form computed once per S."""
    conf, grp = _perturbed_group(N_SETS, S=S, seed=701)
    batch = tuple(t(x) for x in _batch(np.random.RandomState(702), N, S))
    gains = t(_table(N_SETS))
    noise, quiet = TargetNoise(0.2, 0.5), TargetNoise(0.0)
    swept = copy.copy(grp)  # the same weights under a sweep table whose rows are conf's
    swept.set_hparams(vec.hparams_table(vec.hparams_rows(conf, [{}, {}]), conf.ou_dt, "cuda"), 2, 1)
    assert grp.hp is None and swept.hp is not None

    def pair(grads, losses):
        g = grp.learn_set_fused(*batch, N, grads=grads, losses=losses, split=True, phase="critic")
        return grp.learn_set_fused(*batch, N, grads=g, split=True, phase="actor")

    anchor = lambda: (gains, 10.0, torch.full((N_SETS,), 7.0, device="cuda"))
    forms = {
        1: lambda g, lo: grp.learn_set_split(*batch, N, grads=g, losses=lo),
        2: pair,
        3: lambda g, lo: grp.learn_set_split_smooth(*batch, N, quiet, 6, grads=g, losses=lo, seed=3),
        4: lambda g, lo: grp.learn_set_split_smooth(*batch, N, noise, 6, grads=g, losses=lo, seed=3),
        5: lambda g, lo: grp.learn_set_split_anchor(*batch, N, *anchor(), grads=g, losses=lo),
        6: lambda g, lo: grp.learn_set_split_smooth(*batch, N, noise, 6, anchor=anchor(), grads=g, losses=lo, seed=3),
        7: lambda g, lo: grp.learn_set_split_td(*batch, N, grads=g, losses=lo),
        8: lambda g, lo: grp.learn_set_split_td(*batch, N, noise=noise, counter=6, grads=g, losses=lo, seed=3),
        9: lambda g, lo: swept.learn_set_split(*batch, N, grads=g, losses=lo),
    }
    reached = []
    real = vec.call

    def spy(name, *args):  # wraps the module's call: every call still goes to the library
        reached.append(name)
        return real(name, *args)

    out = {}
    vec.call = spy
    try:
        for how in ("zero", "nan"):
            for k, run in forms.items():
                ws = _dirty(_workspace(grp, N), how)
                swept._fsplit_ws = ws
                slab = torch.zeros(N_SETS, grp.lay.theta_size, device="cuda")
                if how == "nan":
                    slab.fill_(float("nan"))
                losses = torch.full((N_SETS, 2), 7.0, device="cuda")
                del reached[:]
                g = run(slab, losses)
                torch.cuda.synchronize()
                assert g.data_ptr() == slab.data_ptr() and grp._fsplit_ws.data_ptr() == ws.data_ptr(), (k, how)
                out[k, how] = (g.clone(), losses.clone(), [n for n in reached if n.startswith("avd_learn_set_split") and n not in NOT_LEARN])
    finally:
        vec.call = real
    return out, grp.lay.actor_size


def _eq(x, y):
    return torch.equal(_bits(x), _bits(y))


@pytest.mark.parametrize("S", [3, 4])
def test_each_form_reaches_the_entry_point_its_docstring_names(S):
    need_gpu()
    out, _ = _forms(S)
    for (k, how), (_, _, reached) in out.items():
        assert reached == ENTRIES[k], (k, how, reached)


@pytest.mark.parametrize("S", [3, 4])
def test_the_forms_agree_bit_for_bit_where_their_docstrings_say_so(S):
    need_gpu()
    out, A = _forms(S)
    g, lo = {k: out[k, "nan"][0] for k in ENTRIES}, {k: out[k, "nan"][1] for k in ENTRIES}
    for k in ENTRIES:
        assert torch.isfinite(g[k]).all() and torch.isfinite(lo[k]).all() and not bool((lo[k] == 7.0).any()), k
        assert bool((g[k][:, A:] != 0).any(dim=1).all()), k
    for k in (2, 3, 9):  # the whole slab and both losses
        assert _eq(g[k], g[1]) and _eq(lo[k], lo[1]), k
    for k, ref in ((5, 1), (6, 4), (7, 1), (8, 4)):  # the critic block and the critic loss
        assert _eq(g[k][:, A:], g[ref][:, A:]) and _eq(lo[k][:, 0], lo[ref][:, 0]), (k, ref)
    for k in (7, 8):  # nothing of the actor's half: +0.0 in every bit of its block, loss 0
        assert bool((_bits(g[k][:, :A]) == 0).all()) and bool((lo[k][:, 1] == 0).all()), k
    # and the variants act: the noise moves the critic block and leaves the actor's alone, the anchor moves the actor block
    assert not _eq(g[4][:, A:], g[1][:, A:]) and _eq(g[4][:, :A], g[1][:, :A]) and _eq(lo[4][:, 1], lo[1][:, 1])
    assert not _eq(g[5][:, :A], g[1][:, :A]) and not _eq(g[6][:, :A], g[4][:, :A]) and _eq(g[6][:, :A], g[5][:, :A])


@pytest.mark.parametrize("S", [3, 4])
def test_a_dirty_workspace_and_slab_change_nothing(S):
    need_gpu()
    out, _ = _forms(S)
    for k in ENTRIES:
        assert _eq(out[k, "nan"][0], out[k, "zero"][0]) and _eq(out[k, "nan"][1], out[k, "zero"][1]), k
