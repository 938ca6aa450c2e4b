"""Target policy smoothing on the GPU: csrc/smooth.hip's kernel alone (avd_target_smooth_f32) against tests/smooth_oracle.py's restatement
of its draws, and the smoothed split set learner (avd_learn_set_split_smooth_f16x3) against the float64 oracle -- oracle.mlp.learn with
the target action replaced by the smoothed, clipped one. The learner's rule is test_gpu_anchor's: every gradient tensor within
max(SPLIT_TOL, 4 x the float32 oracle's own error) of the float64 reference, the losses within 1e-4. Then what the call promises bit for
bit: sigma 0 is the un-smoothed call (plain and anchored), the actor block and the actor loss never depend on the noise, two calls agree,
the workspace and the slab may hold anything, a non-finite input still turns the slab to NaN; and what both entry points refuse on the
host.

The kernel's allowance is 2e-5 sigma absolute per element: tests/test_gpu_replay.py's device-vs-libm allowance for a normal draw (2e-6 at
sigma 0.1), scaled. The moments are those of the CLIPPED noise clip(sigma n, -c, c) -- the normal with its tails moved onto +-c, which is
what min / max produce: variance sigma^2 (1 - 2 Q(k) - 2 k phi(k) + 2 k^2 Q(k)) at k = c / sigma. (The renormalised truncated normal,
without the two atoms, has the standard deviation 0.9546 sigma at k = 2.5 where the clipped noise has 0.9887 sigma: 3.5 % apart, so only
the clipped law can be met to 3 %.)

Measured figures: see the docstring of test_smoothed_learner_matches_the_oracle."""
import ctypes
import math

import numpy as np
import pytest
import torch

from avddpg_amd import _hip
from avddpg_amd.trainer import TargetNoise
from avddpg_amd.vec import seed_table
from tests import smooth_oracle
from tests.gpu_util import need_gpu, t
from tests.test_gpu_anchor import _case, _table
from tests.test_gpu_fset import NAMES
from tests.test_gpu_fsplit import SPLIT_TOL
from tests.test_gpu_mlp import _nets, _perturbed_group, _relerr

pytestmark = pytest.mark.gpu

LO, HI = -2.5, 2.5
LOSS_TOL = 1e-4
DRAW_TOL = 2e-5  # x sigma, absolute


def _smooth(a2, M, E, sigma, clip, counter, seed=0, seeds=None, lo=LO, hi=HI):
    """avd_target_smooth_f32 on a copy of float32 [n, 64] -> numpy."""
    x = t(np.ascontiguousarray(a2, dtype=np.float32)).clone()
    d_seeds = None if seeds is None else seed_table(seeds, "cuda")[1]
    _hip.call("avd_target_smooth_f32", x.shape[0], M, E, _hip.ptr(x), sigma, clip, lo, hi, seed, counter, _hip.ptr(d_seeds), _hip.stream_handle())
    torch.cuda.synchronize()
    return x.cpu().numpy()


def _actions(rs, n):
    """float32 [n, 64] in [LO, HI], with values at and next to both bounds and at 0."""
    a = rs.uniform(LO, HI, size=(n, 64)).astype(np.float32)
    lo, hi = np.float32(LO), np.float32(HI)
    flat = a.reshape(-1)
    special = [lo, hi, np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(0)), np.float32(0), np.float32(-0.0), hi - np.float32(1e-3),
               lo + np.float32(1e-3)]
    for i, v in enumerate(special * 4):
        flat[(i * 7) % flat.size] = v
    return a


@pytest.mark.parametrize("n,M,E", [(1, 1, 1), (37, 1, 1), (18, 3, 2), (16 * 9 + 5, 1, 1), (16, 1, 1)])
@pytest.mark.parametrize("sigma,clip", [(0.2, 0.5), (0.2, math.inf), (1.5, 0.5), (1.5, math.inf)])
def test_kernel_matches_the_oracle(n, M, E, sigma, clip):
    """(1): one agent, 16 live threads of a workgroup; (37), (149): agent counts that are no multiple of the workgroup's 16 -- the tail
    workgroup; (16): exactly one full workgroup; (18, 3, 2): a seed table."""
    need_gpu()
    rs = np.random.RandomState(1000 + n)
    a2 = _actions(rs, n)
    seeds = None if E == 1 else (21, 22)
    out = _smooth(a2, M, E, sigma, clip, counter=5, seed=17, seeds=seeds)
    tol = DRAW_TOL * sigma
    raw = np.float32(sigma) * smooth_oracle.normals(n, M, E, 5, 17, seeds)  # before the noise clip
    eps = smooth_oracle.noise(n, M, E, sigma, clip, 5, 17, seeds)
    ref = smooth_oracle.smooth(a2, eps, LO, HI)
    lo, hi, c = np.float32(LO), np.float32(HI), np.float32(clip)
    print(f"n={n} sigma={sigma} clip={clip}: worst |out - oracle| {np.abs(out - ref).max():.3g} (allowed {tol:.3g}); noise clip binds on "
          f"{np.mean(np.abs(eps) == c):.3f}, action clip on {np.mean((ref == lo) | (ref == hi)):.3f} of the rows")
    assert out.dtype == np.float32 and np.all(out >= lo) and np.all(out <= hi)
    assert np.abs(out - ref).max() <= tol
    # both clips inactive, for the oracle and the device alike: the applied noise is the oracle's eps
    free = (np.abs(eps) < c) & (ref > lo) & (ref < hi) & (out > lo) & (out < hi) & (np.abs(out - a2) < c)
    assert free.mean() > 0.1
    assert np.abs((out - a2) - eps)[free].max() <= tol + np.spacing(np.float32(HI))  # (out - a2 carries the sum's own rounding)
    # the noise clip active beyond the draw's allowance: |eps| == c exactly, so the output is the float32 sum with +-c, clipped
    hard = np.abs(raw) > c + np.float32(tol)
    if np.isfinite(clip):
        assert hard.mean() > (0.5 if sigma > 1 else 0.005)
        want = smooth_oracle.smooth(a2, np.sign(raw) * c, LO, HI)
        assert np.array_equal(out[hard], want[hard])
    else:
        assert not hard.any()
    # values that start on a bound stay within it, and those pushed outwards stay on it
    assert np.all(out[(a2 == hi) & (raw > tol)] == hi) and np.all(out[(a2 == lo) & (raw < -tol)] == lo)


@pytest.mark.parametrize("sigma,clip", [(0.2, 0.5), (1.5, 0.5), (0.2, math.inf)])
def test_moments_of_the_clipped_noise(sigma, clip):
    """64 x 1024 rows from a zero action between infinite bounds: the output IS the noise. Mean within 0.03 sigma of 0, standard
    deviation within 3 % of the clipped normal's (the module's docstring), the share of rows on +-c within 3 % of 2 Q(k) + 0.005."""
    need_gpu()
    n = 1024
    out = _smooth(np.zeros((n, 64), np.float32), 1, 1, sigma, clip, counter=9, seed=4, lo=-math.inf, hi=math.inf).astype(np.float64)
    k = clip / sigma
    Q = 0.5 * math.erfc(k / math.sqrt(2)) if math.isfinite(k) else 0.0
    phi = math.exp(-0.5 * k * k) / math.sqrt(2 * math.pi) if math.isfinite(k) else 0.0
    var = 1 - 2 * Q - 2 * k * phi + 2 * k * k * Q if math.isfinite(k) else 1.0
    std = sigma * math.sqrt(var)
    print(f"sigma={sigma} clip={clip}: mean {out.mean():.5f}, std {out.std():.5f} (clipped normal {std:.5f}), on the clip "
          f"{np.mean(np.abs(out) == np.float32(clip)):.4f} (2 Q = {2 * Q:.4f})")
    assert abs(out.mean()) < 0.03 * sigma
    assert abs(out.std() / std - 1) < 0.03
    assert np.abs(out).max() <= np.float32(clip)
    assert abs(np.mean(np.abs(out) == np.float32(clip)) - 2 * Q) <= 0.03 * 2 * Q + (0.005 if Q else 0.0)


def test_keys_a_seed_table_gives_the_solo_calls_bits_and_the_counter_matters():
    need_gpu()
    E, M, P = 2, 3, 7
    n = P * E * M
    a2 = _actions(np.random.RandomState(5), n)
    seeds = (31, 47)
    big = _smooth(a2, M, E, 0.2, 0.5, counter=12, seeds=seeds)
    e, _, _, _ = smooth_oracle.keys(n, M, E)
    for k, key in enumerate(seeds):
        solo = _smooth(a2[e == k], M, 1, 0.2, 0.5, counter=12, seed=key)
        assert np.array_equal(big[e == k].view(np.int32), solo.view(np.int32)), k
    again = _smooth(a2, M, E, 0.2, 0.5, counter=12, seeds=seeds)
    assert np.array_equal(big.view(np.int32), again.view(np.int32))
    other = _smooth(a2, M, E, 0.2, 0.5, counter=13, seeds=seeds)
    assert np.mean(big != other) > 0.9
    high = _smooth(a2, M, E, 0.2, 0.5, counter=12 + (1 << 32), seeds=seeds)  # the counter's high word is part of the key
    assert np.mean(big != high) > 0.9
    assert np.mean(big != _smooth(a2, M, E, 0.2, 0.5, counter=12, seeds=(31, 48))[:]) > 0.4  # experiment 1 alone changes
    assert np.array_equal(big[e == 0], _smooth(a2, M, E, 0.2, 0.5, counter=12, seeds=(31, 48))[e == 0])


# ---- the learner ----

def _smoothed(grp, batch, n, tn, counter, aw=None, anchor=None, grads=None, seed=3, M=None, d_seeds=None):
    """One smoothed call -> (grads, losses, anchor_loss or None), clones. anchor: (gains numpy, weight)."""
    losses = torch.full((grp.n_sets, 2), 7.0, device="cuda")
    al = an = None
    if anchor is not None:
        al = torch.full((grp.n_sets,), 7.0, device="cuda")
        an = (t(anchor[0]), anchor[1], al)
    g = grp.learn_set_split_smooth(*batch, n, tn, counter, anchor=an, grads=grads, losses=losses, agent_weight=None if aw is None else t(aw),
                                   M=M, seed=seed, d_seeds=d_seeds)
    torch.cuda.synchronize()
    return g.clone(), losses.clone(), None if al is None else al.clone()


def _check_sets(grp, got, s, a, r, s2, P, M, eps, aw=None, gains=None, weight=0.0):
    """Every set of one call against the oracle. -> ({(set, tensor): (error, float32 oracle's error)} of the misses, {tensor: worst
    error}, the share of rows whose target action the action clip moved)."""
    S = grp.lay.S
    g, losses, al = got
    errs, worst, moved = {}, {}, 0.0
    for k in range(M):
        sel = np.arange(P) * M + k
        batch = (s[sel], a[sel], r[sel], s2[sel])
        kw = dict(agent_weight=None if aw is None else aw[sel], gain_row=None if gains is None else gains[k % len(gains)], model_a=S == 3)
        p64 = smooth_oracle.parts(batch, _nets(grp, k, np.float64), eps[sel], LO, HI, **kw)
        p32 = smooth_oracle.parts(batch, _nets(grp, k, np.float32), eps[sel], LO, HI, **kw)
        moved += p64["action_clipped"] / M
        (cg, ag), (cg32, ag32) = smooth_oracle.combine(p64, weight), smooth_oracle.combine(p32, weight)
        gcg, gag = grp.grads_as_lists(g[k])
        for name, x, ref, r32 in zip(NAMES, gcg + gag, list(cg) + list(ag), list(cg32) + list(ag32)):
            e, e32 = _relerr(x, ref), _relerr(r32, ref)
            worst[name] = max(worst.get(name, 0.0), e)
            if e > max(SPLIT_TOL, 4 * e32):
                errs[(k, name)] = (e, e32)
        lo = losses[k].cpu().numpy()
        print(f"set {k}: losses {lo} oracle {p64['critic_loss']:.8g} {p64['actor_loss']:.8g}; action clip moved {p64['action_clipped']:.3f}")
        assert abs(lo[0] - p64["critic_loss"]) <= LOSS_TOL * abs(p64["critic_loss"])
        assert abs(lo[1] - p64["actor_loss"]) <= LOSS_TOL * max(1e-2, abs(p64["actor_loss"]))
        if gains is not None:
            assert abs(float(al[k]) - p64["anchor_loss"]) <= LOSS_TOL * abs(p64["anchor_loss"])
    print("worst error per tensor:", {n_: f"{e:.1e}" for n_, e in worst.items()})
    return errs, worst, moved


@pytest.mark.parametrize("sigma,clip", [(0.2, 0.5), (1.5, 3.0)])
@pytest.mark.parametrize("S,P,M,weighted", [(4, 6, 2, False), (3, 5, 3, False), (4, 1, 1, False), (4, 70, 5, True)])
def test_smoothed_learner_matches_the_oracle(S, P, M, weighted, sigma, clip):
    """(3, 5, 3): Model A; (4, 1, 1): one tile; (4, 70, 5): ragged tile counts, non-uniform agent weights. sigma 1.5 with the noise clip
    at 2 sigma = 3.0: the noise clip binds on 2 Q(2) = 4.6 % of the rows and, the target actions lying in [-2.5, 2.5], the action clip
    moves at least the P(|1.5 n| > 2.5 + 2.5) share and about P(|1.5 n| > 2.5) = 9.6 % for actions near 0 -- both asserted from the
    oracle wherever the call has 700 rows or more (2 % each: three standard errors below the smaller expectation at 768 rows).

    Measured on one MI355X, worst over these eight cases and the anchored one below: the critic tensors <= 3.6e-7 (cW3), the actor tensors
    <= 1.5e-6 (ab1, aW3) of the tensor's max; every tensor is inside SPLIT_TOL = 2e-5 without the float32-oracle clause; at sigma 1.5 the
    noise clip binds on 4.7 % of the rows and the action clip moves 9 - 18 % per set. The kernel alone: worst |out - oracle| 2.4e-7 at
    sigma 0.2 (allowed 4e-6) and 4.8e-7 at sigma 1.5 (allowed 3e-5)."""
    need_gpu()
    grp, n, (s, a, r, s2), aw = _case(S, P, M, 401, weighted)
    tn = TargetNoise(sigma, clip)
    batch = tuple(t(x) for x in (s, a, r, s2))
    got = _smoothed(grp, batch, n, tn, counter=6, aw=aw, seed=3)
    assert torch.isfinite(got[0]).all()
    eps = smooth_oracle.noise(n, M, 1, sigma, clip, 6, seed=3)
    errs, _, moved = _check_sets(grp, got, s, a, r, s2, P, M, eps, aw)
    if sigma > 1 and n * 64 >= 700:
        bound = float(np.mean(np.abs(eps) == np.float32(clip)))
        print(f"noise clip binds on {bound:.3f}, action clip moves {moved:.3f} of the rows")
        assert bound > 0.02 and moved > 0.02
    assert not errs, errs


def test_anchor_and_smoothing_together_match_the_combined_oracle():
    need_gpu()
    S, P, M = 4, 6, 2
    grp, n, (s, a, r, s2), _ = _case(S, P, M, 411)
    gains = _table(M)
    batch = tuple(t(x) for x in (s, a, r, s2))
    got = _smoothed(grp, batch, n, TargetNoise(0.2), counter=2, anchor=(gains, 10.0), seed=8)
    eps = smooth_oracle.noise(n, M, 1, 0.2, 0.5, 2, seed=8)
    errs, _, _ = _check_sets(grp, got, s, a, r, s2, P, M, eps, gains=gains, weight=10.0)
    assert not errs, errs
    # the anchor's side is the anchored call's bit for bit: the actor block, the actor loss and the anchor loss
    al = torch.zeros(M, device="cuda")
    lo = torch.zeros(M, 2, device="cuda")
    g = grp.learn_set_split_anchor(*batch, n, t(gains), 10.0, al, losses=lo)
    torch.cuda.synchronize()
    A = grp.lay.actor_size
    assert torch.equal(got[0][:, :A], g[:, :A]) and torch.equal(got[1][:, 1], lo[:, 1]) and torch.equal(got[2], al)
    assert not torch.equal(got[0][:, A:], g[:, A:]) and not torch.equal(got[1][:, 0], lo[:, 0])


def test_sigma_zero_is_the_unsmoothed_call_and_the_actor_side_never_sees_the_noise():
    """sigma 0: grads and losses torch.equal to learn_set_split (no gains) and to learn_set_split_anchor (gains). sigma > 0: the actor
    block of the slab and losses[:, 1] torch.equal to the un-smoothed call's -- they do not depend on y --, the critic block and
    losses[:, 0] differ; two calls give the same bits, another counter other bits."""
    need_gpu()
    S, P, M = 4, 40, 5
    grp, n, (s, a, r, s2), aw = _case(S, P, M, 421, weighted=True)
    gains = _table(M)
    batch = tuple(t(x) for x in (s, a, r, s2))
    A = grp.lay.actor_size
    l0 = torch.zeros(M, 2, device="cuda")
    g0 = grp.learn_set_split(*batch, n, losses=l0, agent_weight=t(aw)).clone()
    zero = _smoothed(grp, batch, n, TargetNoise(0.0), 4, aw)
    assert torch.equal(zero[0], g0) and torch.equal(zero[1], l0)
    la, al = torch.zeros(M, 2, device="cuda"), torch.zeros(M, device="cuda")
    ga = grp.learn_set_split_anchor(*batch, n, t(gains), 10.0, al, losses=la, agent_weight=t(aw)).clone()
    zero_a = _smoothed(grp, batch, n, TargetNoise(0.0), 4, aw, anchor=(gains, 10.0))
    assert torch.equal(zero_a[0], ga) and torch.equal(zero_a[1], la) and torch.equal(zero_a[2], al)
    for sigma, clip in ((0.2, 0.5), (1.5, 3.0)):
        g, lo, _ = _smoothed(grp, batch, n, TargetNoise(sigma, clip), 4, aw)
        assert torch.equal(g[:, :A], g0[:, :A]) and torch.equal(lo[:, 1], l0[:, 1]), sigma
        assert not torch.equal(g[:, A:], g0[:, A:]) and not torch.equal(lo[:, 0], l0[:, 0]), sigma  # (the noise acts)
        g2, lo2, _ = _smoothed(grp, batch, n, TargetNoise(sigma, clip), 4, aw)
        assert torch.equal(g.view(torch.int32), g2.view(torch.int32)) and torch.equal(lo.view(torch.int32), lo2.view(torch.int32)), sigma
        g3, _, _ = _smoothed(grp, batch, n, TargetNoise(sigma, clip), 5, aw)
        assert not torch.equal(g3[:, A:], g[:, A:]) and torch.equal(g3[:, :A], g[:, :A]), sigma


@pytest.mark.parametrize("how", ["ff", "nan"])
def test_a_dirty_workspace_and_slab_change_nothing(how):
    """As tests/test_gpu_fsplit_glue.py: the call on a workspace full of 0xFF bytes or NaNs, into a slab full of NaNs, is bit for bit the
    call on zeroed memory (the workspace's target actions are written by the target actor's head before the smoothing reads them)."""
    need_gpu()
    from tests.test_gpu_fsplit_glue import _dirty, _workspace

    S, P, M = 4, 7, 3
    grp, n, (s, a, r, s2), _ = _case(S, P, M, 431)
    batch = tuple(t(x) for x in (s, a, r, s2))
    tn = TargetNoise(1.5, 3.0)
    ws = _dirty(_workspace(grp, n), "zero")
    clean = _smoothed(grp, batch, n, tn, 1, grads=torch.zeros(M, grp.lay.theta_size, device="cuda"))
    assert torch.isfinite(clean[0]).all()
    _dirty(ws, how)
    ptr0 = ws.data_ptr()
    dirty = _smoothed(grp, batch, n, tn, 1, grads=torch.full((M, grp.lay.theta_size), float("nan"), device="cuda"))
    assert grp._fsplit_ws.data_ptr() == ptr0
    for x, y in zip(clean[:2], dirty[:2]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), how


@pytest.mark.parametrize("where", ["s2", "theta_t", "s"])
def test_a_non_finite_input_still_turns_the_slab_to_nan(where):
    """A NaN in s2 or in the target actor's weights reaches the target actions themselves. The heads raise the chain's flag from their
    own accumulators before the smoothing runs, so finalize writes NaN into the whole slab and both losses whatever the smoothing
    launch does to a NaN action."""
    need_gpu()
    S, P, M = 4, 5, 2
    grp, n, (s, a, r, s2), _ = _case(S, P, M, 441)
    batch = [t(x) for x in (s, a, r, s2)]
    tn = TargetNoise(0.2)
    assert torch.isfinite(_smoothed(grp, batch, n, tn, 0)[0]).all()
    if where == "theta_t":
        grp.theta_t[1, grp.lay.aW2 + 777] = float("nan")
    else:
        batch[{"s": 0, "s2": 3}[where]].view(-1)[321] = float("nan")
    g, lo, _ = _smoothed(grp, batch, n, tn, 0)
    lay = grp.lay
    for a0, a1 in ((lay.aW2, lay.aW2 + 256 * 128), (lay.actor_size + lay.cW2, lay.actor_size + lay.cW2 + 304 * 128)):
        assert torch.isnan(g[:, a0:a1]).all()
    assert torch.isnan(lo).all()


def test_a_seed_batch_set_draws_its_experiments_noise():
    """n_sets = 6 = 2 experiments x 3 vehicles: the critic block of experiment 1's sets equals, within the engine's tolerance for a
    changed set count (2e-5 of the slab's max: tests/test_gpu_seed_batch.py), that of a solo call on experiment 1's sets and agents
    with its seed; with the other experiment's seed it does not."""
    need_gpu()
    S, P, E, M = 4, 5, 2, 3
    grp, n, (s, a, r, s2), _ = _case(S, P, E * M, 451)
    seeds = (61, 62)
    tn = TargetNoise(1.5, 3.0)
    big = _smoothed(grp, tuple(t(x) for x in (s, a, r, s2)), n, tn, 3, M=M, d_seeds=seed_table(seeds, "cuda")[1])
    conf, solo = _perturbed_group(M, S=S, seed=452)
    for dst, src in ((solo.theta, grp.theta), (solo.stats, grp.stats), (solo.theta_t, grp.theta_t), (solo.stats_t, grp.stats_t)):
        dst.copy_(src[M:2 * M])
    sel = (np.arange(P)[:, None] * (E * M) + M + np.arange(M)[None, :]).reshape(-1)  # experiment 1's agents, agent-major
    sub = tuple(t(np.ascontiguousarray(x[sel])) for x in (s, a, r, s2))
    mine = big[0][M:2 * M]
    ref = _smoothed(solo, sub, P * M, tn, 3, seed=seeds[1])[0]
    wrong = _smoothed(solo, sub, P * M, tn, 3, seed=seeds[0])[0]
    scale = ref.abs().max().item()
    assert (mine - ref).abs().max().item() <= 2e-5 * scale
    assert (mine - wrong).abs().max().item() > 1e-3 * scale  # (fifty times the tolerance: the seed matters)


def test_host_refusals_leave_every_output_untouched():
    """What the two entry points refuse before their first HIP call, on real device buffers: the target actions, grads, losses and the
    anchor loss keep their sentinel; then the same buffers are accepted when nothing is wrong."""
    need_gpu()
    p = _hip.ptr
    a2 = torch.full((12, 64), 1.0, device="cuda")
    seeds = seed_table((1, 2), "cuda")[1]

    def alone(n=12, M=3, E=1, buf=a2, sigma=0.2, clip=0.5, lo=LO, hi=HI, tab=None):
        _hip.call("avd_target_smooth_f32", n, M, E, p(buf), sigma, clip, lo, hi, 1, 0, p(tab), _hip.stream_handle())

    who = "avd_target_smooth_f32"
    refuse = lambda name, code, msg: pytest.raises(_hip.AvdError, match=rf"failed \({code}\): {name}: {msg}")
    for msg, kw in (("null a2", dict(buf=None)), ("n_agents=0", dict(n=0)), ("M=0 E=1", dict(M=0)), ("M=3 E=0", dict(E=0)),
                    ("n_agents=12 M=5 E=1", dict(M=5)), ("E=2 without a seed table", dict(E=2)), ("sigma=-0.2", dict(sigma=-0.2)),
                    ("sigma=inf", dict(sigma=math.inf)), ("sigma=-?nan", dict(sigma=math.nan)), ("noise_clip=0 ", dict(clip=0.0)),
                    ("noise_clip=-?nan", dict(clip=math.nan)), ("lo=2.5 > hi=-2.5", dict(lo=HI, hi=LO))):
        with refuse(who, -1, msg):
            alone(**kw)
    torch.cuda.synchronize()
    assert bool((a2 == 1.0).all())
    alone(E=2, tab=seeds)
    torch.cuda.synchronize()
    assert bool((a2 != 1.0).all()) and bool((a2 > 1.0 - 0.5 - 1e-6).all()) and bool((a2 < 1.0 + 0.5 + 1e-6).all())

    S, P, M = 4, 3, 2
    grp, n, batch, _ = _case(S, P, M, 461)
    s, a, r, s2 = (t(x) for x in batch)
    gains = t(_table(M))
    need = ctypes.c_size_t(0)
    _hip.call("avd_learn_set_split_workspace", grp._layp, n, M, ctypes.byref(need))
    ws = torch.zeros(need.value, dtype=torch.uint8, device="cuda")
    grads = torch.full((M, grp.lay.theta_size), 3.0, device="cuda")
    losses, al = torch.full((M, 2), 3.0, device="cuda"), torch.full((M,), 3.0, device="cuda")

    def go(lay=grp._layp, n_agents=n, n_sets=M, gains_=gains, Mt=M, lo=LO, hi=HI, weight=1.0, al_=al, theta=grp.theta, wsb=None, sigma=0.2,
           clip=0.5, tab=None, E=1):
        _hip.call("avd_learn_set_split_smooth_f16x3", lay, n_agents, n_sets, p(theta), p(grp.stats), p(grp.theta_t), p(grp.stats_t), p(s), p(a),
                  p(r), p(s2), None, 0.99, 2.5, p(grads), p(losses), p(ws), ws.numel() if wsb is None else wsb, p(gains_), Mt, 0, lo, hi,
                  weight, p(al_), sigma, clip, 1, 0, p(tab), E, _hip.stream_handle())

    who = "avd_learn_set_split_smooth_f16x3"
    wide = _hip.make_layout(4, 1, 320, 160, 48, 64)
    for code, msg, kw in ((-1, "null gains / anchor_loss", dict(al_=None)), (-1, "n_sets=2 M=3", dict(Mt=3)), (-1, "weight=-0.5", dict(weight=-0.5)),
                          (-1, "M=0 E=1", dict(gains_=None, Mt=0)), (-1, "M=2 E=0", dict(E=0)), (-1, "n_sets=2 M=2 E=2", dict(E=2, tab=seeds)),
                          (-1, "E=2 without a seed table", dict(E=2, Mt=1)), (-1, "sigma=-0.2", dict(sigma=-0.2)),
                          (-1, "sigma=inf", dict(sigma=math.inf)), (-1, "sigma=-?nan", dict(sigma=math.nan)), (-1, "noise_clip=0 ", dict(clip=0.0)),
                          (-1, "noise_clip=-1", dict(clip=-1.0)), (-1, "noise_clip=-?nan", dict(clip=math.nan)),
                          (-1, r"lo=2.5 > hi=-2.5", dict(lo=HI, hi=LO)), (-1, "null layout", dict(lay=None)),
                          (-1, "n_agents=5 n_sets=2", dict(n_agents=5)), (-3, "serves the reference widths only", dict(lay=ctypes.byref(wide))),
                          (-1, "null pointer", dict(theta=None)), (-1, "workspace 16 B <", dict(wsb=16))):
        with refuse(who, code, msg):
            go(**kw)
    torch.cuda.synchronize()
    assert bool((grads == 3.0).all()) and bool((losses == 3.0).all()) and bool((al == 3.0).all())
    go(gains_=None, al_=None, weight=math.nan)  # no anchor: anchor_loss may be null, weight is unread
    torch.cuda.synchronize()
    assert torch.isfinite(grads).all() and bool((al == 3.0).all())
    go(E=2, Mt=1, tab=seeds)  # and with a table and a seed batch's layout
    torch.cuda.synchronize()
    assert torch.isfinite(grads).all() and bool((al != 3.0).all())
