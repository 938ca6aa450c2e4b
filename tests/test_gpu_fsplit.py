"""GPU parity of the split-operand fused set learner (csrc/fsplit.hip, avd_learn_set_split_f16x3): Trainer.learn
(workers/trainer.py:472-508) + federated mean (src/server/federated.py:47-63, 99-118) for agents that share their networks,
with every GEMM operand an exact 16-bit pair hi + lo. The reference multiplies float32 by float32 (agent/model.py:26-36, 63-83;
workers/trainer.py:472-508), so the bar is float32's own, enforced here rather than quoted from a profile:

  SPLIT_TOL = 2e-5 of each gradient tensor's max against the float64 oracle (or 4 x the float32 ORACLE's own error on the same
  batch where that is larger) -- 5 x tighter than the 1e-4 the exact-f32 kernels are held to (tests/test_gpu_mlp.py GRAD_TOL).
  Measured (tools/r04_precision_probe.py @ tag r06-pre-prune, profiles/r04_precision_probe.txt): <= 5e-7 at 64 ... 4480 rows per set (asserted at
  SPLIT_TOL_SMALL = 4e-6; the float32 NumPy oracle sits at 1e-6 there, r03's bf16 pairs sat at 5.6e-6), <= 1.1e-5 per tensor at
  4096 x 5 (262 144 rows per set; one relu-tie row is worth ~1e-5 there), where the exact-f32 per-agent engine + fed_mean sits at
  <= 1.5e-5 and the float32 NumPy oracle at <= 1.8e-4.

Covered: conditioned inputs (no relu ties) AND unconditioned inputs with every out-of-tolerance tensor traced to a tie row;
the exact-f32 per-agent kernel + fed_mean; bit-identical reruns; fp16 overflow and non-finite inputs -> NaN; at 4096 x 5 the
float64 oracle on two whole sets, the f32 engine on all five and the mean-of-halves property; VecTrainer trajectories.
One agent's 64-row tile at every tile ordinal of a workgroup: tests/test_gpu_fsplit_tiles.py, docs/fsplit_tile_parity.md."""
import numpy as np
import pytest
import torch

from avddpg_amd import config, vec
from oracle import mlp as omlp
from tests.gpu_util import need_gpu, t
from tests.split_oracle import tie_rows
from tests.test_gpu_fset import NAMES, _batch
from tests.test_gpu_mlp import GRAD_TOL, _nets, _perturbed_group, _relerr

pytestmark = pytest.mark.gpu

SPLIT_TOL = 2e-5
SPLIT_TOL_SMALL = 4e-6  # conditioned inputs, <= 4480 rows per set


def _tie_mask(grp, M, S, s, a, tie=1e-6, sets=None):
    """[agents, 64] bool: batch rows with a pre-activation closer to 0 than `tie` x its layer's largest, in any layer that is
    differentiated (actor(s), critic(s, a), critic(s, mu)) -- evaluated in float64 with agent v's set v % M (only the agents of
    `sets` when given; the others stay False)."""
    bad = np.zeros(s.shape[:2], bool)
    for k in (range(M) if sets is None else sets):
        an, cn, _, _ = _nets(grp, k, np.float64)
        sel = np.arange(k, s.shape[0], M)
        x = s[sel].reshape(-1, s.shape[2])[:, :S].astype(np.float64)
        act = a[sel].reshape(-1, 1).astype(np.float64)
        t_ = tie_rows(an, cn, x, act, tie)  # (the float64 arithmetic: tests/split_oracle.py)
        bad[sel] = t_.reshape(len(sel), -1)
    return bad


def _untie(grp, M, S, s, a, tie=1e-6):
    """The relu derivative is discontinuous at 0: a row with a pre-activation within float32 resolution of 0 in a layer that is
    differentiated has no defined float32 gradient -- the same arithmetic in another order decides the sign the other way, and
    ONE such row moves the actor's first-layer gradient of a 4480-row batch by 1e-3 of its max (seen: |z2| = 1.1e-8 at scale
    0.8 in one row of 22400; tools/fsplit_both_debug.py @ tag r06-pre-prune). The CONDITIONED tests nudge such rows (in place, deterministically)
    until none is left; the unconditioned test below runs the same inputs as they are and accounts for every tie. Returns the
    number of nudges."""
    nudged = 0
    for _ in range(8):
        bad = _tie_mask(grp, M, S, s, a, tie)
        if not bad.any():
            return nudged
        nudged += int(bad.sum())
        s[bad] += np.float32(0.0173)
        a[bad] = np.clip(a[bad] + np.float32(0.0091), -2.5, 2.5)
    raise AssertionError("could not condition the batch")


def _errors_vs_oracle(grp, g, s, a, r, s2, P, M, sets, B=64, losses=None, loss_tol=1e-4):
    """{(set, tensor): (error, float32 oracle's error)} of the tensors of g [M, theta] that miss max(SPLIT_TOL, 4 x f32-oracle
    error) against the float64 oracle on each set's concatenated P x 64-row batch; also checks the losses when given."""
    errs, worst = {}, 0.0
    for k in sets:
        sel = np.arange(P) * M + k
        cat = lambda x: x[sel].reshape(P * B, *x.shape[2:])
        batch = (cat(s), cat(a), cat(r)[:, None], cat(s2))
        cg, ag, aux = omlp.learn(batch, *_nets(grp, k, np.float64))
        cg32, ag32, _ = omlp.learn(batch, *_nets(grp, k, np.float32))
        gcg, gag = grp.grads_as_lists(g[k])
        for name, got, ref, r32 in zip(NAMES, gcg + gag, cg + ag, cg32 + ag32):
            e, e32 = _relerr(got, ref), _relerr(r32, ref)
            worst = max(worst, e)
            if e > max(SPLIT_TOL, 4 * e32):
                errs[(k, name)] = (e, e32)
        if losses is not None:
            lo = losses[k].cpu().numpy()
            assert abs(lo[0] - aux["critic_loss"]) <= loss_tol * abs(aux["critic_loss"])
            assert abs(lo[1] - aux["actor_loss"]) <= loss_tol * max(1e-2, abs(aux["actor_loss"]))
    return errs, worst


@pytest.mark.parametrize("S,P,M", [(4, 6, 2), (3, 5, 3), (4, 1, 1), (4, 70, 5), (4, 300, 1)])  # (300, 1): every CU's workgroup on ONE set, 1-2 tiles each
def test_split_set_learner_matches_oracle_at_the_f32_tolerance(S, P, M):
    """The mean over a set's P agents of their 64-row batch gradients == the gradient of the P*64-row batch (inference-mode
    BN: rows are independent). Every gradient tensor within max(SPLIT_TOL = 2e-5, 4 x the float32 oracle's own error) of the
    float64 oracle (the exact-f32 learn kernels are asserted at 1e-4, tests/test_gpu_mlp.py::test_learn_gradients_match_oracle).
    Inputs conditioned against relu ties (_untie); the same inputs unconditioned: next test."""
    need_gpu()
    conf, grp = _perturbed_group(M, S=S, seed=61)
    rs = np.random.RandomState(62)
    n = P * M  # agent v = p*M + m uses set m
    s, a, r, s2 = _batch(rs, n, S)
    _untie(grp, M, S, s, a)
    losses = torch.zeros(M, 2, device="cuda")
    g = grp.learn_set_split(t(s), t(a), t(r), t(s2), n, losses=losses)
    torch.cuda.synchronize()
    assert torch.isfinite(g).all()
    errs, worst = _errors_vs_oracle(grp, g, s, a, r, s2, P, M, range(M), losses=losses)
    assert not errs, errs
    assert worst <= SPLIT_TOL_SMALL, worst  # (at these sizes the float32-oracle clause is not needed: fp16 pairs measure 3e-7 ... 5e-7)


@pytest.mark.parametrize("S,P,M", [(4, 6, 2), (3, 5, 3), (4, 1, 1), (4, 70, 5)])
def test_split_set_learner_unconditioned_inputs_every_miss_is_a_relu_tie(S, P, M):
    """the SAME cases without _untie, so that the conditioning is shown to hide nothing but relu ties. Every
    tensor that misses the tolerance on the raw inputs is traced: the platoons (64-row tiles) of that set are learned one by
    one and compared with the oracle tile by tile; each tile that misses must contain a tie row (a pre-activation within 1e-6
    of its layer's largest of 0, where the float32 derivative is undefined), and with those tiles left out of BOTH means the
    set is back inside the tolerance. The tie rows are reported. (Seed 62 at S = 4, P = 70, M = 5 holds the known case: one
    row of 22 400 with |z2| = 1.1e-8 in critic(s, mu) moves every actor tensor by 5.5e-5 ... 1.1e-3.)"""
    need_gpu()
    B = 64
    conf, grp = _perturbed_group(M, S=S, seed=61)
    n = P * M
    s, a, r, s2 = _batch(np.random.RandomState(62), n, S)
    g = grp.learn_set_split(t(s), t(a), t(r), t(s2), n).clone()
    assert torch.isfinite(g).all()
    errs, _ = _errors_vs_oracle(grp, g, s, a, r, s2, P, M, range(M))
    if not errs:
        return
    ties = _tie_mask(grp, M, S, s, a)  # [agents, 64]
    # platoon by platoon: n_agents = M, one 64-row tile per set
    tiles = [grp.learn_set_split(t(s[p * M:(p + 1) * M]), t(a[p * M:(p + 1) * M]), t(r[p * M:(p + 1) * M]), t(s2[p * M:(p + 1) * M]), M).clone()
             for p in range(P)]
    report = {}
    for k in sorted({k for k, _ in errs}):
        missing = []
        for p in range(P):
            v = p * M + k
            cg, ag, _ = omlp.learn((s[v], a[v], r[v][:, None], s2[v]), *_nets(grp, k, np.float64))
            cg32, ag32, _ = omlp.learn((s[v], a[v], r[v][:, None], s2[v]), *_nets(grp, k, np.float32))
            gcg, gag = grp.grads_as_lists(tiles[p][k])
            if any(_relerr(got, ref) > max(SPLIT_TOL, 4 * _relerr(r32, ref)) for got, ref, r32 in zip(gcg + gag, cg + ag, cg32 + ag32)):
                missing.append(p)
        assert missing, (k, "tensors miss the tolerance but no single tile does", {n_: e for (kk, n_), e in errs.items() if kk == k})
        for p in missing:
            rows = np.nonzero(ties[p * M + k])[0]
            assert len(rows) > 0, (k, p, "a tile misses the tolerance without a relu tie in it")
            report[(k, p)] = rows.tolist()
        # without the tie tiles, on both sides: inside the tolerance again
        keep = [p for p in range(P) if p not in missing]
        assert keep, "every tile of the set holds a tie"
        sel = np.array(keep) * M + k
        cat = lambda x: x[sel].reshape(len(keep) * B, *x.shape[2:])
        batch = (cat(s), cat(a), cat(r)[:, None], cat(s2))
        cg, ag, _ = omlp.learn(batch, *_nets(grp, k, np.float64))
        cg32, ag32, _ = omlp.learn(batch, *_nets(grp, k, np.float32))
        mean = torch.stack([tiles[p][k] for p in keep]).double().mean(dim=0).float()
        gcg, gag = grp.grads_as_lists(mean)
        for name, got, ref, r32 in zip(NAMES, gcg + gag, cg + ag, cg32 + ag32):
            assert _relerr(got, ref) <= max(SPLIT_TOL, 4 * _relerr(r32, ref)), (k, name, _relerr(got, ref))
        assert len(missing) <= int(ties[np.arange(P) * M + k].any(axis=1).sum())
    print(f"unconditioned S={S} P={P} M={M}: {len(errs)} tensors over tolerance, all traced to relu-tie rows (set, platoon) -> rows: {report}")


@pytest.mark.parametrize("P,M", [(8, 3), (1, 1), (70, 5)])
def test_split_set_learner_equals_per_agent_f32_kernel_plus_federated_mean(P, M):
    """avd_learn_f32 per agent (exact f32 MFMA) + fed_mean over the platoons vs the split learner on the same agent-major
    batch: SPLIT_TOL of each block's max (the bf16 learner of fset.hip: 1.7e-2 on the actor block)."""
    need_gpu()
    B, S = 64, 4
    conf, grp = _perturbed_group(M, S=S, seed=71)
    rs = np.random.RandomState(72)
    n = P * M
    s, a, r, s2 = _batch(rs, n, S)
    _untie(grp, M, S, s, a)
    per_agent = grp.learn(t(s), t(a), t(r), t(s2), M)
    avg = vec.fed_mean(per_agent, P, M, method=conf.interfrl).cpu().numpy()  # [M, theta]
    split = grp.learn_set_split(t(s), t(a), t(r), t(s2), n).cpu().numpy()
    bf16 = grp.learn_set_fused(t(s), t(a), t(r), t(s2), n).cpu().numpy()
    lay = grp.lay
    for name, lo, hi in (("actor", 0, lay.actor_size), ("critic", lay.actor_size, lay.theta_size)):
        scale = np.abs(avg[:, lo:hi]).max()
        es, eb = np.abs(avg[:, lo:hi] - split[:, lo:hi]).max() / scale, np.abs(avg[:, lo:hi] - bf16[:, lo:hi]).max() / scale
        assert es <= SPLIT_TOL, (name, es, eb)
        assert es < 0.05 * eb or eb < 1e-4, (name, es, eb)  # two orders of magnitude closer than single-rounded operands
    # padding floats of the slab stay zero (what Adam relies on)
    assert split[:, lay.actor_size - 3:lay.actor_size].max() == 0.0 or lay.actor_size % 4 == 0


def test_split_set_learner_is_deterministic():
    need_gpu()
    P, M, S = 40, 5, 4
    conf, grp = _perturbed_group(M, S=S, seed=75)
    s, a, r, s2 = (t(x) for x in _batch(np.random.RandomState(76), P * M, S))
    g1 = grp.learn_set_split(s, a, r, s2, P * M).clone()
    g2 = grp.learn_set_split(s, a, r, s2, P * M).clone()
    assert torch.equal(g1, g2)


def test_split_set_learner_weighted_mean_matches_weighted_fed_mean():
    """Server.get_weighted_avg_params (src/server/federated.py:99-118) through per-agent factors w_p * P / sum(w)."""
    need_gpu()
    P, M, B, S = 6, 2, 64, 4
    conf, grp = _perturbed_group(M, S=S, seed=101)
    rs = np.random.RandomState(102)
    n = P * M
    s, a, r, s2 = _batch(rs, n, S)
    for p in range(P):  # make the platoons' gradients differ, else any weighting gives the same mean
        r[p * M:(p + 1) * M] *= 1.0 + 4.0 * p
        s[p * M:(p + 1) * M] += 0.5 * p
    w = np.linspace(0.2, 3.0, P)[:, None].repeat(M, axis=1).astype(np.float32) * rs.uniform(0.8, 1.2, size=(P, M)).astype(np.float32)
    per_agent = grp.learn(t(s), t(a), t(r), t(s2), M)
    avg = vec.fed_mean(per_agent, P, M, weights=t(w), method=conf.interfrl).cpu().numpy()
    aw = (w * (P / w.sum(axis=0))).reshape(-1).astype(np.float32)  # agent-major [P*M]
    g = grp.learn_set_split(t(s), t(a), t(r), t(s2), n, agent_weight=t(aw)).cpu().numpy()
    unweighted = grp.learn_set_split(t(s), t(a), t(r), t(s2), n).cpu().numpy()
    lay = grp.lay
    for lo, hi in ((0, lay.actor_size), (lay.actor_size, lay.theta_size)):
        scale = np.abs(avg[:, lo:hi]).max()
        assert np.abs(avg[:, lo:hi] - g[:, lo:hi]).max() <= SPLIT_TOL * scale
        assert np.abs(avg[:, lo:hi] - unweighted[:, lo:hi]).max() > 5e-2 * scale  # the weights matter in this case


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("where", ["theta", "stats_t", "s", "a", "r"])
def test_set_learners_turn_a_non_finite_input_into_nan_gradients(split, where):
    """both set learners are built with -fno-honor-nans and their relu() turns a NaN into 0, so a diverged weight
    or a poisoned replay row would vanish instead of propagating as it does through the f32 engines. The inputs are tested
    for finiteness on the way in (bit tests) and finalize writes NaN into the whole slab."""
    need_gpu()
    P, M, S = 5, 2, 4
    conf, grp = _perturbed_group(M, S=S, seed=81)
    s, a, r, s2 = (t(x) for x in _batch(np.random.RandomState(82), P * M, S))
    fn = grp.learn_set_split if split else grp.learn_set_fused
    assert torch.isfinite(fn(s, a, r, s2, P * M)).all()
    bad = float("nan") if where != "r" else float("inf")
    if where == "theta":
        grp.theta[1, grp.lay.cW2 + grp.lay.actor_size + 777] = bad
    elif where == "stats_t":
        grp.stats_t[0, grp.lay.amv1 + 3] = bad
    else:
        {"s": s, "a": a, "r": r}[where].view(-1)[321] = bad
    g = fn(s, a, r, s2, P * M)
    lay = grp.lay
    for lo, hi in ((lay.aW2, lay.aW2 + 256 * 128), (lay.actor_size + lay.cW2, lay.actor_size + lay.cW2 + 304 * 128)):
        assert torch.isnan(g[:, lo:hi]).all()


@pytest.mark.parametrize("where", ["actor_W1", "critic_Wa", "target_critic_Ws", "target_actor_b1", "state"])
def test_split_set_learner_turns_an_fp16_overflow_into_nan_gradients(where):
    """first-layer activations travel as fp16 pairs scaled by S1 = 64, so relu(z1) >= 1023.75 converts to
    (+inf, -inf); under -fno-honor-nans the NaN accumulators that follow would be relu'd to 0 and the call would return wrong,
    finite gradients. Every such conversion is watched (one accumulator per batch row and sweep in the heads; the scaled static
    operands in the prep kernels; the inputs in pack): the whole slab must come back NaN -- and stay finite, equal to the exact
    engine's, just below the threshold."""
    need_gpu()
    P, M, S = 5, 2, 4
    conf, grp = _perturbed_group(M, S=S, seed=83)
    lay = grp.lay
    s, a, r, s2 = (t(x) for x in _batch(np.random.RandomState(84), P * M, S))
    s[:, :, 0] = 1.5  # (a known input magnitude on state 0)
    s2[:, :, 0] = 1.5
    a[:] = 2.5

    def poke(scale):
        if where == "actor_W1":        # z1 = 1.5 * 800 * scale + ...: activation overflow in OUT_TANH(actor, s); S1 w = 51 200 * scale is representable
            grp.theta[1, lay.aW1 + 0 * 256 + 7] = 800.0 * scale
        elif where == "critic_Wa":     # action layer: za = 2.5 * 480 * scale: HEAD_BOTH, branch A
            grp.theta[0, lay.actor_size + lay.cWa + 5] = 480.0 * scale
        elif where == "target_critic_Ws":  # OUT_TD on s'
            grp.theta_t[1, lay.actor_size + lay.cWs + 0 * 256 + 9] = 800.0 * scale
        elif where == "target_actor_b1":   # S1 b = 76 800: the static operand itself overflows (prep1_kernel)
            grp.theta_t[0, lay.ab1 + 3] = 1200.0 * scale
        else:                           # an input that fp16 cannot hold (pack_x_kernel); below: a large but harmless one
            s.view(-1)[4 * 77 + 1] = 70000.0 if scale == 1.0 else 300.0

    poke(0.5)  # z1 <= 600 < 1023.75 / bias 600 / state 300: finite, and still the exact engine's gradients
    g = grp.learn_set_split(s, a, r, s2, P * M).clone()
    assert torch.isfinite(g).all()
    exact = vec.fed_mean(grp.learn(s, a, r, s2, M), P, M, method=conf.interfrl)
    for lo, hi in ((0, lay.actor_size), (lay.actor_size, lay.theta_size)):
        assert (g[:, lo:hi] - exact[:, lo:hi]).abs().max().item() <= SPLIT_TOL * exact[:, lo:hi].abs().max().item()
    poke(1.0)
    g = grp.learn_set_split(s, a, r, s2, P * M)
    for lo, hi in ((lay.aW2, lay.aW2 + 256 * 128), (lay.actor_size + lay.cW2, lay.actor_size + lay.cW2 + 304 * 128)):
        assert torch.isnan(g[:, lo:hi]).all(), where


def test_full_size_split_learner_against_the_float64_oracle_the_f32_engine_and_the_mean_of_its_halves():
    """BASELINE configs[1] / configs[3]'s per-GPU shape (4096 platoons x 5 vehicle indices, 64-row batches = 262 144 rows per
    weight set), VERDICT r03 #1(c):
      * the FLOAT64 ORACLE's gradient of two whole sets (first and last; NumPy takes seconds per set): every tensor within
        SPLIT_TOL = 2e-5 of its max -- no float32-oracle clause here (that NumPy oracle is the least accurate of the three at this
        size: 1.8e-4), unconditioned inputs;
      * the exact-f32 per-agent learn kernel + federated mean on all five sets: the split learner must be at least as close to
        the oracle as that engine on the two oracle sets (2 x its error, or SPLIT_TOL), and within 5e-5 of it per block on all
        five (the comparator's own distance from the oracle is 1.5e-5 per tensor);
      * the size-independent property that the mean over all platoons is the average of the means over its two halves (same
        operand values on both sides, only the f32 summation grouping differs: 2e-5); bit-identical reruns."""
    need_gpu()
    P, M, B, S = 4096, 5, 64, 4
    conf, grp = _perturbed_group(M, S=S, seed=91)
    gen = torch.Generator(device="cuda").manual_seed(92)
    rn = lambda *sh: torch.randn(*sh, device="cuda", generator=gen)
    n = P * M
    s, a, r, s2 = 1.5 * rn(n, B, S), 2.5 * (2 * torch.rand(n, B, 1, device="cuda", generator=gen) - 1), -rn(n, B).abs() * 0.3, 1.5 * rn(n, B, S)
    full = grp.learn_set_split(s, a, r, s2, n).clone()
    again = grp.learn_set_split(s, a, r, s2, n)
    assert torch.equal(full, again) and torch.isfinite(full).all() and full.abs().max() > 0
    h = n // 2
    halves = []
    for lo in (0, h):
        sl = lambda x: x[lo:lo + h].contiguous()
        halves.append(grp.learn_set_split(sl(s), sl(a), sl(r), sl(s2), h).clone())
    avg = 0.5 * (halves[0] + halves[1])
    exact = vec.fed_mean(grp.learn(s, a, r, s2, M), P, M, method=conf.interfrl)
    lay = grp.lay
    for lo, hi in ((0, lay.actor_size), (lay.actor_size, lay.theta_size)):
        scale = exact[:, lo:hi].abs().max().item()
        assert (full[:, lo:hi] - avg[:, lo:hi]).abs().max().item() <= 2e-5 * scale, lo
        assert (full[:, lo:hi] - exact[:, lo:hi]).abs().max().item() <= 5e-5 * scale, (lo, (full[:, lo:hi] - exact[:, lo:hi]).abs().max().item() / scale)
    assert not torch.allclose(halves[0], halves[1])  # the halves are different batches
    sn, an, rn_, s2n = (x.cpu().numpy() for x in (s, a, r, s2))
    worst = {}
    for k in (0, M - 1):
        sel = np.arange(P) * M + k
        cat = lambda x: x[sel].reshape(P * B, *x.shape[2:])
        cg, ag, _ = omlp.learn((cat(sn), cat(an), cat(rn_)[:, None], cat(s2n)), *_nets(grp, k, np.float64))
        gs, ge = grp.grads_as_lists(full[k]), grp.grads_as_lists(exact[k])
        for name, got, eng, ref in zip(NAMES, gs[0] + gs[1], ge[0] + ge[1], cg + ag):
            e, ee = _relerr(got, ref), _relerr(eng, ref)
            worst[name] = max(worst.get(name, 0.0), e)
            assert e <= SPLIT_TOL, (k, name, e, ee)
            assert e <= max(SPLIT_TOL, 2 * ee), (k, name, e, ee)
    print("4096 x 5, split learner vs float64 oracle, worst per tensor:", {n_: f"{e:.1e}" for n_, e in worst.items()})


def test_trainer_split_engine_tracks_per_agent_engine_under_interfrl():
    """VecTrainer with shared weight sets: the split learner against the exact f32 per-agent kernel + fed_sum on the same
    host RNG stream (parity mode). Before the first update the two differ only by the acting kernel (f32 matrix cores for the
    set learners, csrc/act.hip, vs the rows kernel: f32 summation order, 2e-6); afterwards the gradients differ at the 1e-5 level and
    Adam normalises every step to |dw| <= lr, so what remains is bounded by the f32 kernels' own run-to-run class: actions
    within 2e-4 of the action range (the bf16 engine needs 5e-3 here, tests/test_gpu_fset.py)."""
    from avddpg_amd import trainer

    need_gpu()
    P, L, steps = 6, 3, 72
    conf = config.Config(num_platoons=P, pl_size=L, buffer_size=128, fed_method="interfrl", weighted_average_enabled=False)
    runs = []
    for engine in ("per_agent", "fused3"):
        np.random.seed(11)
        vt = trainer.VecTrainer(conf, rng="host", shared_sets=True, shared_engine=engine)
        vt.reset_episode()
        traj = []
        for i in range(steps):
            vt.step(0, i)
            traj.append((vt.actions.cpu().numpy().copy(), vt.env.x.cpu().numpy().copy()))
        runs.append((vt, traj))
    (a, ta), (b, tb) = runs
    assert b.grads is None and b.shared_engine == "fused3" and a.updates == b.updates == (steps - 64) * P * L
    for i in range(steps):
        tol = 2e-6 if i < 65 else 2e-4
        assert np.abs(ta[i][0] - tb[i][0]).max() <= tol * 2.5, i
        assert np.abs(ta[i][1] - tb[i][1]).max() <= tol * max(1.0, np.abs(ta[i][1]).max()), i
    n_upd = steps - 64
    for lr, lo, hi in ((conf.actor_lr, 0, a.agents.lay.actor_size), (conf.critic_lr, a.agents.lay.actor_size, a.agents.lay.theta_size)):
        d = (a.agents.theta[:, lo:hi] - b.agents.theta[:, lo:hi]).abs()
        assert d.max().item() <= 2 * lr * n_upd and d.mean().item() <= 0.02 * lr * n_upd
    assert torch.isfinite(b.agents.theta).all() and int(b.agents.step[0]) == n_upd


def test_trainer_split_engine_weighted_federation_runs_model_a():
    """Weighted interfrl (workers/trainer.py:385-398) + Model A (S = 3) through the split engine."""
    from avddpg_amd import trainer

    need_gpu()
    conf = config.Config(num_platoons=4, pl_size=2, buffer_size=128, fed_method="interfrl", weighted_average_enabled=True,
                         weighted_window=2, episode_sim_time=3.0, model="ModelA")  # 30-step episodes
    np.random.seed(2)
    vt = trainer.VecTrainer(conf, rng="host", shared_engine="fused3")
    assert vt.shared and vt.shared_engine == "fused3" and vt.agents.lay.S == 3
    th0 = vt.agents.theta.clone()
    vt.run(number_of_episodes=4)
    assert vt.fed_weights is not None and vt.fed_weights[0] == 3
    assert torch.isfinite(vt.agents.theta).all() and int(vt.agents.step[0]) == 4 * 30 - 64
    assert not torch.equal(vt.agents.theta, th0)


@pytest.mark.parametrize("scale_w2,scale_in", [(1e-3, 1.0), (300.0, 1.0), (1.0, 12.0), (0.0, 1.0)])
def test_split_set_learner_fp16_scaling_is_robust_to_weight_and_state_magnitudes(scale_w2, scale_in):
    """The heads carry their operands as fp16 pairs (5-bit exponent): second-layer weights are rescaled per set and net by a
    power of two (scale_kernel), first-layer weights by 2^6, and the scales are folded into f32 constants. Weights 1e-3 ... 300 x
    their usual size, states up to the env's bounds (|x| ~ 20), and an all-zero second layer (max = 0: no scale to derive) must
    give the exact engine's gradients all the same -- ten weight sets (BASELINE configs[2]'s vehicle count)."""
    need_gpu()
    P, M, S = 9, 10, 4
    conf, grp = _perturbed_group(M, S=S, seed=141)
    lay = grp.lay
    for th in (grp.theta, grp.theta_t):
        th[:, lay.aW2:lay.aW2 + 256 * 128] *= scale_w2
        th[:, lay.actor_size + lay.cW2:lay.actor_size + lay.cW2 + 304 * 128] *= scale_w2
    s, a, r, s2 = _batch(np.random.RandomState(142), P * M, S)
    s, s2 = s * scale_in, s2 * scale_in
    exact = vec.fed_mean(grp.learn(t(s), t(a), t(r), t(s2), M), P, M, method=conf.interfrl).cpu().numpy()
    got = grp.learn_set_split(t(s), t(a), t(r), t(s2), P * M).cpu().numpy()
    assert np.isfinite(got).all()
    for k in range(M):
        ce, ae = grp.grads_as_lists(torch.from_numpy(exact[k]).cuda())
        cg, ag = grp.grads_as_lists(torch.from_numpy(got[k]).cuda())
        for name, x, z in zip(NAMES, cg + ag, ce + ae):
            scale = np.abs(z).max()
            if scale > 0:
                assert np.abs(x - z).max() <= SPLIT_TOL * scale, (k, name, np.abs(x - z).max() / scale)
            else:
                assert np.abs(x).max() == 0.0, (k, name)


def test_guarded_update_skips_a_set_whose_slab_is_nan_and_is_bitwise_the_plain_update_otherwise():
    """the split engine answers an fp16 overflow / a non-finite input with an all-NaN slab; fed to Adam that would poison the
    shared weight set for good. avd_adam_polyak_guarded_f32 leaves such a set untouched (weights, moments, targets, step counter),
    counts it, and is bit-identical to avd_adam_polyak_f32 for every finite set."""
    need_gpu()
    M, P, S = 3, 4, 4
    conf, grp = _perturbed_group(M, S=S, seed=81)
    conf2, ref = _perturbed_group(M, S=S, seed=81)
    n = P * M
    s, a, r, s2 = _batch(np.random.RandomState(82), n, S)
    g = grp.learn_set_split(t(s), t(a), t(r), t(s2), n).clone()
    assert torch.isfinite(g).all()
    g_bad = g.clone()
    g_bad[1] = float("nan")  # what finalize writes for a set when the learner's `bad` flag is up
    before = [x.clone() for x in (grp.theta, grp.theta_t, grp.stats_t, grp.m, grp.v)]
    grp.apply(g_bad, guarded=True)
    ref.apply(g)
    torch.cuda.synchronize()
    assert int(grp.nonfinite_skipped.item()) == 1 and grp.step.tolist() == [1, 0, 1] and ref.step.tolist() == [1, 1, 1]
    for x, b, y in zip((grp.theta, grp.theta_t, grp.stats_t, grp.m, grp.v), before, (ref.theta, ref.theta_t, ref.stats_t, ref.m, ref.v)):
        assert torch.equal(x[1], b[1])                                        # the NaN set: untouched
        assert torch.equal(x[0], y[0]) and torch.equal(x[2], y[2])            # the others: the plain update, bit for bit
        assert torch.isfinite(x).all()
    # a NaN at the head of the CRITIC block alone is caught too (the two-phase call finalizes the blocks separately)
    g_c = g.clone()
    g_c[0, grp.lay.actor_size:] = float("nan")
    th0 = grp.theta[0].clone()
    grp.apply(g_c, guarded=True)
    assert int(grp.nonfinite_skipped.item()) == 2 and torch.equal(grp.theta[0], th0) and grp.step.tolist() == [1, 1, 2]
    # end to end: an overflowing state in one platoon's batch -> NaN slab from the learner -> the trainer's guarded update counts it
    from avddpg_amd import trainer as tr
    vt = tr.VecTrainer(config.Config(num_platoons=8, pl_size=3, buffer_size=128, fed_method="interfrl", weighted_average_enabled=False),
                       rng="device", auto_reset=True, seed=5, shared_engine="fused3")
    vt.reset_episode()
    for _ in range(66):
        vt.step()
    assert vt.nonfinite_updates() == 0 and vt.updates > 0
    vt.replay.ring[0, :, 0] = 7e4  # every stored state of agent 0 beyond fp16's range
    th = vt.agents.theta.clone()
    vt.step()
    torch.cuda.synchronize()
    assert vt.nonfinite_updates() >= 1 and torch.isfinite(vt.agents.theta).all()
    assert torch.equal(vt.agents.theta[0], th[0])  # agent 0 = vehicle 0's set: skipped


def test_guarded_update_covers_the_bf16_set_learner_and_an_infinite_head():
    """the guard's contract -- element 0 of a set's actor block and of its critic block is non-finite iff the block is
    invalid -- end to end for the OTHER 16-bit set learner too (csrc/fset.hip, shared_engine="fused": a non-finite input makes its
    finalize write NaN over the whole slab), and for an Inf at a block's head (r05's guard tested for NaN only: an Inf went into
    Adam's moments)."""
    need_gpu()
    from avddpg_amd import trainer as tr

    vt = tr.VecTrainer(config.Config(num_platoons=8, pl_size=3, buffer_size=128, fed_method="interfrl", weighted_average_enabled=False),
                       rng="device", auto_reset=True, seed=5, shared_engine="fused")
    vt.reset_episode()
    for _ in range(66):
        vt.step()
    assert vt.nonfinite_updates() == 0 and vt.updates > 0
    vt.replay.ring[0, :, 0] = float("inf")  # every stored state of agent 0 non-finite
    th, steps = vt.agents.theta.clone(), vt.agents.step.clone()
    vt.step()
    torch.cuda.synchronize()
    assert vt.nonfinite_updates() >= 1 and torch.isfinite(vt.agents.theta).all() and torch.isfinite(vt.agents.m).all()
    assert torch.equal(vt.agents.theta[0], th[0]) and int(vt.agents.step[0]) == int(steps[0])  # vehicle 0's set: skipped, count put back
    # an infinite head of either block is a skipped set like a NaN one
    M = 3
    conf, grp = _perturbed_group(M, S=4, seed=91)
    g = torch.zeros(M, grp.lay.theta_size, device="cuda")
    g[0, 0] = float("inf")
    g[2, grp.lay.actor_size] = float("-inf")
    before = grp.theta.clone()
    grp.apply(g, guarded=True)
    torch.cuda.synchronize()
    assert int(grp.nonfinite_skipped.item()) == 2 and grp.step.tolist() == [0, 1, 0]
    assert torch.equal(grp.theta[0], before[0]) and torch.equal(grp.theta[2], before[2]) and torch.isfinite(grp.m).all()
