"""The general learner and the batch-1 forward kernels (csrc/mlp.hip: gen::learn_kernel_g<false / true>, adam_polyak_ranges_kernel,
mlp_rows_kernel, actor_rows_shared_kernel) over the shape domain the header promises -- S <= 64, A <= 16, H1 and Ha multiples of
16, H2 a multiple of 32 and <= 256, a 64-row tile within 160 KiB of LDS -- against the float64 oracle (oracle/mlp.py, itself pinned to
torch float64 autograd at these shapes in tests/test_oracle_mlp.py).

The shapes (SHAPES below; "floats" = gen::lds_floats of the padded layout, limit 40960) are chosen by what they reach in the code:

  S   A  logical H1/H2/Ha   padded       floats  reaches
  4   1  307/153/57 (x1.2)  320/160/64   37672   centralized pl_size 1: a real configuration on the general kernel
  8   2  307/153/57 (x1.2)  320/160/64   38376   centralized pl_size 2; K = 8: l1_fwd_t<2>'s upper edge, two full steps
 16   4  307/153/57 (x1.2)  320/160/64   39784   centralized pl_size 4; K = 16 in l1_fwd_t<5>
 20   5  307/153/57 (x1.2)  320/160/64   40488   (added) centralized pl_size 5, the LARGEST centralized shape that fits, on the
                                                 general kernel (diagnostic switch; the shipped library runs cen.hip here)
  1   1  16/32/16           same          5416   every minimum; ONE column tile for four waves in every first layer; H2 = 32
  5   2  48/32/16           same          8232   K = 5 (not a multiple of 4) in <2>; three column tiles in a state branch
  9   1  128/64/32          same         16584   <5>'s lower edge: the j < K clamp inside the third step
 21   3  128/256/32         same         31496   <16>'s lower edge (six steps, clamp in the sixth); H2 = 256 = 16 * DX_NB
 64  16  128/64/32          same         26824   both documented maxima: <16> with all 16 steps, every [64][A] array at its largest
 40  10  208/96/48          same         31144   the centralized pl_size 10 interface at a width that fits; <16> with ten steps
  4   1  448/32/16          same         34120   the widest first layer (28 column tiles) beside the narrowest second
  3   1  100/50/20          112/64/32    15144   padding in all three widths; Model A's S = 3
  4   1  256/128/48         same         30184   the reference widths forced onto the general kernel (diagnostic switch)
  3   1  256/128/48         same         30120   the same at Model A's S = 3 (new)

(S = 21, 40 and 64 are the l1_fwd_t<16> range 21 <= K <= 64; A = 10 and 16 put the critic's action branch into <5>.)

Every comparison is against the float64 oracle at the tolerances of tests/test_gpu_mlp.py (FWD_TOL = 2e-5, GRAD_TOL = 1e-4 of the
tensor's max, or 4 x the float32 oracle's own error where that is larger); the fused update and the shared-row actor are compared
bit for bit with the unfused / one-agent-per-workgroup paths. No test can pass on degenerate inputs: _assert_inputs_bite holds for
every case (conditions on the inputs, from the oracle alone). States are drawn with std 1.5 * min(1, 2 / sqrt(S)): the perturbed
actor head (x 30, tuned at S = 4 in _perturbed_group) saturates tanh on wider inputs otherwise.

Worst measured relative errors per shape (of the tensor's max; all agents, per-agent and shared sets), MI355X, measured with this
file on top of commit 7d5a213 (the tests print them: run with -s):

  S   A  padded       forward   critic grads  actor grads
  4   1  320/160/64   6.8e-08   3.5e-06       6.3e-07
  8   2  320/160/64   7.7e-08   7.0e-07       6.6e-07
 16   4  320/160/64   1.2e-07   6.1e-07       5.4e-07
 20   5  320/160/64   1.1e-07   4.5e-07       5.9e-07
  1   1  16/32/16     1.4e-08   4.0e-07       3.8e-07
  5   2  48/32/16     3.3e-08   3.5e-07       5.2e-07
  9   1  128/64/32    3.2e-08   5.6e-07       7.3e-06
 21   3  128/256/32   7.0e-08   6.4e-07       8.3e-07
 64  16  128/64/32    7.6e-08   3.5e-07       4.3e-07
 40  10  208/96/48    7.2e-08   4.5e-07       4.0e-07
  4   1  448/32/16    6.6e-08   1.1e-06       2.4e-06
  3   1  112/64/32    2.5e-08   4.8e-07       1.7e-05  (actor db2 / dgamma2 of one agent; the float32 oracle is 1.65e-05 off there too)
  4   1  256/128/48   5.3e-08   1.5e-06       2.0e-06
  3   1  256/128/48   4.6e-08   3.9e-07       5.9e-07

No shape needed the "4 x the float32 oracle" escape; no kernel defect was found.
"""
import collections

import numpy as np
import pytest
import torch

from avddpg_amd import _hip, config, params, trainer, vec
from oracle import mlp as omlp
from tests.gpu_util import need_gpu, t
from tests.test_gpu_mlp import FWD_TOL, GRAD_TOL, _central_batches, _nets, _perturbed_group, _relerr

pytestmark = pytest.mark.gpu

LDS_LIMIT_FLOATS = 160 * 1024 // 4
Shape = collections.namedtuple("Shape", "S A widths hidd_mult padded floats general")
REF = (256, 128, 48)
SHAPES = [
    pytest.param(Shape(4, 1, REF, 1.2, (320, 160, 64), 37672, False), id="cen1-4x1-320.160.64"),
    pytest.param(Shape(8, 2, REF, 1.2, (320, 160, 64), 38376, False), id="cen2-8x2-320.160.64"),
    pytest.param(Shape(16, 4, REF, 1.2, (320, 160, 64), 39784, False), id="cen4-16x4-320.160.64"),
    pytest.param(Shape(20, 5, REF, 1.2, (320, 160, 64), 40488, True), id="cen5-20x5-320.160.64-general"),
    pytest.param(Shape(1, 1, (16, 32, 16), 1, (16, 32, 16), 5416, False), id="min-1x1-16.32.16"),
    pytest.param(Shape(5, 2, (48, 32, 16), 1, (48, 32, 16), 8232, False), id="ragged-5x2-48.32.16"),
    pytest.param(Shape(9, 1, (128, 64, 32), 1, (128, 64, 32), 16584, False), id="st5lo-9x1-128.64.32"),
    pytest.param(Shape(21, 3, (128, 256, 32), 1, (128, 256, 32), 31496, False), id="st16lo-21x3-128.256.32"),
    pytest.param(Shape(64, 16, (128, 64, 32), 1, (128, 64, 32), 26824, False), id="max-64x16-128.64.32"),
    pytest.param(Shape(40, 10, (208, 96, 48), 1, (208, 96, 48), 31144, False), id="cen10-40x10-208.96.48"),
    pytest.param(Shape(4, 1, (448, 32, 16), 1, (448, 32, 16), 34120, False), id="wide1-4x1-448.32.16"),
    pytest.param(Shape(3, 1, (100, 50, 20), 1, (112, 64, 32), 15144, False), id="padded-3x1-100.50.20"),
    pytest.param(Shape(4, 1, REF, 1, REF, 30184, True), id="ref-4x1-general"),
    pytest.param(Shape(3, 1, REF, 1, REF, 30120, True), id="ref-3x1-general"),
]
AT_SIZE = Shape(21, 3, (128, 256, 32), 1, (128, 256, 32), 31496, False)


def _lds_floats(lay):
    """gen::lds_floats (csrc/mlp.hip), restated: the general kernel's 64-row tile in floats."""
    ld = lambda k: k if (k >> 2) & 1 else k + 4
    return (64 * ld(lay.H1 + lay.Ha) + 64 * ld(lay.H2) + 2 * (lay.H1 + lay.Ha) + 5 * lay.H2 + 64 * lay.S + 64 + 7 * 64 * lay.A + 8)


def _x_scale(S):
    return min(1.0, 2.0 / np.sqrt(S))


def _width_kw(widths):
    H1, H2, Ha = widths
    return dict(actor_layer1_size=H1, actor_layer2_size=H2, critic_layer1_size=H1, critic_layer2_size=H2, critic_act_layer_size=Ha)


def _group(sh, n_sets, seed):
    conf, grp = _perturbed_group(n_sets, S=sh.S, seed=seed, A=sh.A, hidd_mult=sh.hidd_mult, **_width_kw(sh.widths))
    lay = grp.lay
    assert (lay.S, lay.A, lay.H1, lay.H2, lay.Ha) == (sh.S, sh.A) + tuple(sh.padded)
    assert tuple(grp.dims)[2:] == tuple(int(w * sh.hidd_mult) for w in sh.widths)
    assert _lds_floats(lay) == sh.floats <= LDS_LIMIT_FLOATS  # (the table above, and the kernel's bound)
    return conf, grp


def _batches(sh, n_agents, seed):
    s, a, r, s2 = _central_batches(n_agents, sh.S, sh.A, seed)
    xs = float(_x_scale(sh.S))
    return (s * xs).contiguous(), a, r, (s2 * xs).contiguous()


def _states(sh, n_agents, seed):
    rs = np.random.RandomState(seed)
    return (rs.normal(0, 1.5, size=(n_agents, sh.S)) * _x_scale(sh.S)).astype(np.float32)


def _route(sh, request, monkeypatch):
    """Rows whose shape has a kernel of its own reach the general one through the diagnostic build's switch."""
    if sh.general:
        request.getfixturevalue("diag_lib")
        monkeypatch.setenv("AVD_LEARN_GENERAL", "1")


def _assert_inputs_bite(nets64, s, a, where):
    """Conditions on the INPUTS (float64 oracle alone) without which a comparison could pass vacuously: in every hidden layer of
    the online actor and critic between 20 % and 80 % of the units are active (relu > 0), averaged over the rows; at least half of
    the rows leave the online actor's tanh unsaturated (|tanh| < 0.99)."""
    aw, cw = nets64[0], nets64[1]
    _, (_, p1, _, p2, _, th) = omlp.actor_forward(aw, s, 2.5, cache=True)
    _, (_, _, ps, pa, _, pc2, _) = omlp.critic_forward(cw, s, a, cache=True)
    for name, p in (("actor 1", p1), ("actor 2", p2), ("critic s", ps), ("critic a", pa), ("critic 2", pc2)):
        frac = float(np.mean(p > 0))
        assert 0.2 <= frac <= 0.8, (where, name, frac)
    unsat = float(np.mean(np.all(np.abs(th) < 0.99, axis=1)))
    assert unsat >= 0.5, (where, "tanh rows unsaturated", unsat)


def _logical_mask(grp):
    """Boolean [theta_size]: True on the elements of the logical tensors, False on padded units' rows / columns / entries and on
    the alignment gaps -- from params.pack alone: the slab elements that differ between packing all-ones and all-zeros tensors
    (the neutral padding value, 0 or 1, is the same in both)."""
    lay, d = grp.lay, params.logical_dims(grp.lay, grp.dims)
    slabs = []
    for fill in (1.0, 0.0):
        th, st = np.zeros(lay.theta_size, np.float32), np.zeros(lay.stats_size, np.float32)
        for which, spec in (("actor", params.ACTOR_WEIGHTS), ("critic", params.CRITIC_WEIGHTS)):
            params.pack(lay, [np.full(shp(d), fill, np.float32) for _, _, shp in spec], th, st, which, dims=grp.dims)
        slabs.append(th)
    mask = slabs[0] != slabs[1]
    n_logical = sum(int(np.prod(shp(d))) for _, k, shp in params.ACTOR_WEIGHTS + params.CRITIC_WEIGHTS if k == "t")
    assert int(mask.sum()) == n_logical
    return mask


def _check_learn_against_oracle(grp, conf, batches, grads, losses, agents, set_mod, where):
    """Every gradient tensor, both losses and the shapes of `agents` against the float64 oracle; returns the worst (critic, actor)
    relative errors."""
    s, a, r, s2 = (x.cpu().numpy() for x in batches)
    worst = [0.0, 0.0]
    for v in agents:
        k = v % set_mod if set_mod else v
        batch = (s[v], a[v], r[v][:, None], s2[v])
        nets64 = _nets(grp, k, np.float64)
        _assert_inputs_bite(nets64, s[v], a[v], (where, v))
        cg, ag, aux = omlp.learn(batch, *nets64, gamma=conf.gamma, high=2.5)
        cg32, ag32, _ = omlp.learn(batch, *_nets(grp, k, np.float32), gamma=conf.gamma, high=2.5)
        for ref in cg + ag:
            assert np.max(np.abs(ref)) > 1e-8, (where, v, "a gradient tensor of the oracle is trivial")
        gcg, gag = grp.grads_as_lists(grads[v])
        assert [w.shape for w in gcg] == [w.shape for w in cg] and [w.shape for w in gag] == [w.shape for w in ag]
        lo = losses[v].cpu().numpy()
        assert abs(lo[0] - aux["critic_loss"]) <= 1e-4 * max(1.0, abs(aux["critic_loss"])), (where, v)
        assert abs(lo[1] - aux["actor_loss"]) <= 1e-4 * max(1.0, abs(aux["actor_loss"])), (where, v)
        for net, (got_l, ref_l, r32_l) in enumerate(((gcg, cg, cg32), (gag, ag, ag32))):
            for i, (got, ref, r32) in enumerate(zip(got_l, ref_l, r32_l)):
                e, e32 = _relerr(got, ref), _relerr(r32, ref)
                worst[net] = max(worst[net], e)
                if e > GRAD_TOL / 10:
                    print(f"  {where} agent {v} {'critic actor'.split()[net]}[{i}]: relerr {e:.3g} (f32 oracle {e32:.3g})")
                assert e <= max(GRAD_TOL, 4 * e32), (where, v, "critic actor".split()[net], i, e, e32)
    return worst


@pytest.mark.parametrize("sh", SHAPES)
def test_forward_matches_oracle(sh):
    """mlp_rows_kernel, one agent per workgroup (set_mod = 0): every actor and critic output element, online and target nets."""
    need_gpu()
    n = 8
    conf, grp = _group(sh, n, seed=201)
    x = _states(sh, n, 202)
    act = np.random.RandomState(203).uniform(-2.5, 2.5, size=(n, sh.A)).astype(np.float32)
    worst, active, unsat, qmax = 0.0, [], 0, 0.0
    for target in (False, True):
        out = grp.actor(t(x), set_mod=0, target=target).cpu().numpy().reshape(n, sh.A)
        q = grp.critic(t(x), t(act), set_mod=0, target=target).cpu().numpy().reshape(n, sh.A)
        for v in range(n):
            nets = _nets(grp, v, np.float64)
            aw, cw = (nets[2], nets[3]) if target else (nets[0], nets[1])
            ref, (_, p1, _, p2, _, th) = omlp.actor_forward(aw, x[v:v + 1], 2.5, cache=True)
            refq, (_, _, ps, pa, _, pc2, _) = omlp.critic_forward(cw, x[v:v + 1], act[v:v + 1], cache=True)
            active.append([np.mean(p > 0) for p in (p1, p2, ps, pa, pc2)])
            unsat += bool(np.all(np.abs(th) < 0.99))
            qmax = max(qmax, float(np.max(np.abs(refq))))
            e_a = np.max(np.abs(out[v] - ref[0])) / 2.5
            e_q = np.max(np.abs(q[v] - refq[0])) / max(1.0, np.max(np.abs(refq)))
            worst = max(worst, e_a, e_q)
            assert e_a <= FWD_TOL and e_q <= FWD_TOL, (target, v, e_a, e_q)
    # the inputs bite: hidden layers neither dead nor all-on (averaged over the 16 evaluations), tanh mostly unsaturated
    frac = np.mean(np.array(active), axis=0)
    assert np.all(frac >= 0.2) and np.all(frac <= 0.8), frac
    assert unsat >= n and qmax > 0.05, (unsat, qmax)
    print(f"GENSHAPE forward S={sh.S} A={sh.A} {sh.padded}: worst relerr {worst:.3g}")


@pytest.mark.parametrize("sh", SHAPES)
def test_learn_matches_oracle_and_padding_is_exact(sh, request, monkeypatch):
    """gen::learn_kernel_g<false>: all 24 gradient tensors and both losses of 5 agents with per-agent sets and of 7 agents sharing 3
    sets (n_agents % set_mod != 0), against the float64 oracle; every slab element outside the logical tensors is exactly 0."""
    need_gpu()
    _route(sh, request, monkeypatch)
    worst = [0.0, 0.0]
    for n_agents, set_mod, seed in ((5, 0, 211), (7, 3, 215)):
        conf, grp = _group(sh, set_mod or n_agents, seed=seed)
        b = _batches(sh, n_agents, seed + 1)
        losses = torch.zeros(n_agents, 2, device="cuda")
        grads = torch.full((n_agents, grp.lay.theta_size), 7.0, device="cuda")
        grp.learn(*b, set_mod, grads=grads, losses=losses)
        torch.cuda.synchronize()
        assert torch.isfinite(grads).all()
        w = _check_learn_against_oracle(grp, conf, b, grads, losses, range(n_agents), set_mod, f"learn set_mod={set_mod}")
        worst = [max(x, y) for x, y in zip(worst, w)]
        mask = _logical_mask(grp)
        g = grads.cpu().numpy()
        assert np.all(g[:, ~mask] == 0.0), np.argwhere(g[:, ~mask] != 0.0)[:8]
        assert np.mean(g[:, mask] != 0.0) > 0.3
        if tuple(sh.padded) != tuple(grp.dims)[2:]:  # padded units exist beyond the 4-float alignment gaps
            assert int((~mask).sum()) > 64
    print(f"GENSHAPE learn S={sh.S} A={sh.A} {sh.padded}: worst relerr critic {worst[0]:.3g} actor {worst[1]:.3g}")


@pytest.mark.parametrize("sh", SHAPES)
def test_fused_update_is_bitwise_learn_then_apply(sh, request, monkeypatch):
    """gen::learn_kernel_g<true> + adam_polyak_ranges_kernel (avd_learn_update_f32; with next states avd_learn_update_act_f32, whose
    Python entry serves A = 1) against avd_learn_f32 + avd_adam_polyak_f32 + avd_actor_forward_f32: three steps in a row (theta
    ping-pong; steps 1 and 3 with next states where A = 1), every state tensor, the losses and the next actions bit for bit; the
    two skip ranges [aW2, aW2 + H1 H2) and [cW2, cW2 + (H1 + Ha) H2) move with the widths. Padding never moves."""
    need_gpu()
    _route(sh, request, monkeypatch)
    n = 5
    (conf, ga), (_, gb) = _group(sh, n, seed=221), _group(sh, n, seed=221)
    assert torch.equal(ga.theta, gb.theta) and torch.equal(ga.theta_t, gb.theta_t)
    start = [x.clone() for x in (ga.theta, ga.m, ga.v)]
    mask = torch.from_numpy(_logical_mask(ga)).cuda()
    scratch = torch.zeros(n, ga.lay.theta_size, device="cuda")
    la, lb = torch.zeros(n, 2, device="cuda"), torch.zeros(n, 2, device="cuda")
    for k in range(3):
        b = _batches(sh, n, 222 + k)
        nxt = t(_states(sh, n, 226 + k))
        s_, a_ = b[0].cpu().numpy(), b[1].cpu().numpy()
        for v in range(n):
            _assert_inputs_bite(_nets(ga, v, np.float64), s_[v], a_[v], ("fused", k, v))
        with_next = sh.A == 1 and k != 1
        if with_next:
            out = torch.full((n,), 7.0, device="cuda")
            ga.learn_update(*b, scratch, losses=la, next_states=nxt, next_actions=out)
        else:
            ga.learn_update(*b, scratch, losses=la)
            out = ga.actor(nxt, 0)
        gb.apply(gb.learn(*b, 0, losses=lb))
        want = gb.actor(nxt, 0)
        torch.cuda.synchronize()
        for name in ("theta", "theta_t", "stats_t", "m", "v", "step"):
            x, y = getattr(ga, name), getattr(gb, name)
            assert torch.equal(x, y), (k, name, int((x != y).sum()), torch.nonzero(x != y)[:4].tolist())
        assert torch.equal(la, lb) and torch.equal(out, want), k
        assert torch.isfinite(ga.theta).all() and float(want.abs().max()) > 0.05
    assert ga.step.tolist() == [3] * n
    for x, x0 in zip((ga.theta, ga.m, ga.v), start):
        assert torch.equal(x[:, ~mask], x0[:, ~mask])  # padded entries: exactly their initial values
    assert float((ga.theta[:, mask] != start[0][:, mask]).float().mean()) > 0.5 and float((ga.v[:, mask] > 0).float().mean()) > 0.3


def test_lane_independence_and_determinism_at_size_2048_agents():
    """The pattern of test_full_size_learn_properties_20480_agents at a non-reference shape (S = 21, A = 3, 128/256/32): an agent's
    gradient depends on its own batch and weights only, wherever it sits in the grid; two launches agree bit for bit; three agents
    against the float64 oracle."""
    need_gpu()
    sh, n, n_src = AT_SIZE, 2048, 8
    conf, src = _group(sh, n_src, seed=231)
    grp = vec.AgentGroup(n, sh.S, sh.A, conf, hidd_mult=sh.hidd_mult)
    for name in ("theta", "stats", "theta_t", "stats_t"):
        getattr(grp, name).copy_(getattr(src, name).repeat(n // n_src, 1))
    g = torch.Generator(device="cuda").manual_seed(232)
    xs = float(_x_scale(sh.S))
    s = torch.randn(n, 64, sh.S, device="cuda", generator=g) * (1.5 * xs)
    a = torch.rand(n, 64, sh.A, device="cuda", generator=g) * 5 - 2.5
    r = -torch.rand(n, 64, device="cuda", generator=g)
    s2 = torch.randn(n, 64, sh.S, device="cuda", generator=g) * (1.5 * xs)
    for dst in (8, 1025, n - 1):
        for x in (grp.theta, grp.theta_t, grp.stats, grp.stats_t, s, a, r, s2):
            x[dst].copy_(x[7])
    losses = torch.zeros(n, 2, device="cuda")
    g1 = grp.learn(s, a, r, s2, 0, losses=losses)
    g2 = grp.learn(s, a, r, s2, 0)
    assert torch.equal(g1, g2) and torch.isfinite(g1).all()
    for dst in (8, 1025, n - 1):
        assert torch.equal(g1[dst], g1[7])
    assert not torch.equal(g1[7], g1[9]) and not torch.equal(g1[7], g1[15])  # (other weights; the same weights, another batch)
    _check_learn_against_oracle(grp, conf, (s, a, r, s2), g1, losses, (7, 1234, n - 2), 0, "at size")


WIDE = (1024, 1024, 48)
ACTOR_CASES = [  # S, A, widths, n_agents, set_mod, whether avd_actor_forward_f32 takes actor_rows_shared_kernel
    pytest.param(9, 1, (128, 64, 32), 8, 1, True, id="narrow-8x1-shared"),
    pytest.param(9, 1, (128, 64, 32), 39, 3, True, id="narrow-13x3-shared-ragged-group"),
    pytest.param(5, 2, (48, 32, 16), 20, 2, True, id="narrow-A2-10x2-shared"),
    pytest.param(9, 1, (128, 64, 32), 14, 2, False, id="narrow-7x2-fewer-than-8-per-set"),
    pytest.param(9, 1, (128, 64, 32), 23, 3, False, id="narrow-23-agents-not-a-multiple-of-3"),
    pytest.param(4, 1, WIDE, 18, 2, False, id="hidden1024-9x2-over-64KiB"),
]


@pytest.mark.parametrize("S,A,widths,n_agents,M,shared_rows", ACTOR_CASES)
def test_actor_with_shared_sets_across_the_shared_row_switch(S, A, widths, n_agents, M, shared_rows):
    """avd_actor_forward_f32 with set_mod = M runs actor_rows_shared_kernel (8 agents of a set per workgroup) when every set has the
    same number >= 8 of agents and 8 (H1 + H2 + 256 + 64) floats fit 64 KiB, and mlp_rows_kernel otherwise: on either side of
    each condition the actions are, bit for bit, those of the same agents evaluated one per launch (set_mod = 0) on a one-set copy
    of their weights, and within FWD_TOL of the float64 oracle."""
    need_gpu()
    conf, grp = _perturbed_group(M, S=S, A=A, seed=241, **_width_kw(widths))
    lay = grp.lay
    fits = 8 * (lay.H1 + lay.H2 + 256 + 64) * 4 <= 64 * 1024
    assert (n_agents % M == 0 and n_agents // M >= 8 and fits) == shared_rows  # (launch_rows' rule, restated)
    x = (np.random.RandomState(242).normal(0, 1.5, size=(n_agents, S)) * (0.25 if widths == WIDE else _x_scale(S))).astype(np.float32)
    got = grp.actor(t(x), set_mod=M)
    one = vec.AgentGroup(1, S, A, conf)
    ref = torch.empty_like(got)
    for v in range(n_agents):
        one.theta.copy_(grp.theta[v % M:v % M + 1]), one.stats.copy_(grp.stats[v % M:v % M + 1])
        ref[v] = one.actor(t(x[v:v + 1]), set_mod=0)[0]
    assert torch.equal(got, ref), torch.nonzero(got != ref)[:4].tolist()
    got = got.cpu().numpy().reshape(n_agents, A)
    unsat = 0
    for v in range(n_agents):
        aw = [w.astype(np.float64) for w in grp.get_weights(v % M, "actor")]
        want = omlp.actor_forward(aw, x[v:v + 1], 2.5)[0]
        unsat += bool(np.all(np.abs(want) < 0.99 * 2.5))
        assert np.max(np.abs(got[v] - want)) <= FWD_TOL * 2.5, (v, got[v], want)
    assert unsat >= n_agents / 2 and np.abs(got).max() > 0.05


def _sentinel_state(grp, n):
    T = grp.lay.theta_size
    grp.theta_alt = torch.full((n, T), 7.0, device="cuda")
    grp.m.fill_(7.0), grp.v.fill_(7.0)
    return torch.full((n, T), 7.0, device="cuda")


@pytest.mark.parametrize("S,A,widths,hidd_mult,message", [
    # 36968 + 64 * 24 + 448 * 6 = 41192 floats > 40960
    pytest.param(24, 6, REF, 1.2, r"need 164768 B of LDS per 64-row tile \(> 160 KiB\)", id="centralized-pl_size-6"),
    pytest.param(4, 1, (256, 288, 48), 1, r"H2 a multiple of 32 and <= 256 \(got S=4 A=1 H1=256 H2=288 Ha=48\)", id="H2-288"),
])
def test_shapes_outside_the_domain_are_refused_before_any_launch(S, A, widths, hidd_mult, message):
    """The first centralized shape that does not fit the LDS (pl_size 6, against pl_size 5 with 472 floats to spare, which
    SHAPES runs) and H2 > 16 * DX_NB: learn and learn_update raise with the limit named, and write nothing."""
    need_gpu()
    n = 2
    conf = config.Config(**_width_kw(widths))
    grp = vec.AgentGroup(n, S, A, conf, hidd_mult=hidd_mult)
    with pytest.raises(_hip.AvdError, match=message):
        _hip.call("avd_learn_check_shape", grp._layp)
    z = lambda *shape: torch.zeros(*shape, device="cuda")
    b = (z(n, 64, S), z(n, 64, A), z(n, 64), z(n, 64, S))
    grads = _sentinel_state(grp, n)
    theta0, theta_t0 = grp.theta.clone(), grp.theta_t.clone()
    with pytest.raises(_hip.AvdError, match="avd_learn_f32.*" + message):
        grp.learn(*b, 0, grads=grads)
    with pytest.raises(_hip.AvdError, match="avd_learn_update_f32.*" + message):
        grp.learn_update(*b, grads)
    torch.cuda.synchronize()
    for x in (grads, grp.theta_alt, grp.m, grp.v):
        assert bool((x == 7.0).all())
    assert torch.equal(grp.theta, theta0) and torch.equal(grp.theta_t, theta_t0)


def test_trainer_refuses_centralized_pl_size_6_at_construction():
    """centralized pl_size 5 is the largest platoon the per-agent learner serves; pl_size 6 is refused when the trainer is built,
    with the learner's own message, not at the first learn step."""
    need_gpu()
    vt = trainer.VecTrainer(config.Config(num_platoons=2, pl_size=5, buffer_size=128, framework="centralized"), rng="device")
    assert (vt.S, vt.A) == (20, 5) and _lds_floats(vt.agents.lay) == LDS_LIMIT_FLOATS - 472
    with pytest.raises(_hip.AvdError, match=r"S=24 A=6 H1=320 H2=160 Ha=64 need 164768 B of LDS per 64-row tile \(> 160 KiB\)"):
        trainer.VecTrainer(config.Config(num_platoons=2, pl_size=6, buffer_size=128, framework="centralized"), rng="device")
