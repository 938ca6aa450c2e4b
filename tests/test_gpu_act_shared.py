"""The kernels that produce every action of a shared-set run, row by row against the oracles:

  avd_actor_forward_shared_bf16 (csrc/wide.hip: l1_fwd_kernel<S> -> launch_gemm<EpiFwd> -> tanh_rows_kernel; AgentGroup.actor_shared)
      over the forward cases of tests/bf16_oracle.py (FWD_CASES: both GEMM kernels, ragged last row tiles, one row per set, one row past
      a tile, K = 64, S = 3, one set), EVERY row of EVERY set held to the rule of tests/bf16_oracle.py -- max and rms error against the
      float64 reference within max(FWD_TOL, 4 x the bf16-operand oracle's own), nothing measured from a kernel in it; the bounds of
      `out`; a used, a poisoned and a fresh workspace; the library's refusals;
  VecTrainer._act_wide_shared (the set-major transposition around it) agent by agent against the oracle on the agent's OWN observation;
  avd_actor_forward_set_f32 (csrc/act.hip; AgentGroup.actor_set) every row against the float64 oracle at FWD_TOL and the rows kernel
      at 2e-6, at P = 1, 31, 32, 33 and 65 agents per set, 1, 3 and 64 sets, x_stride 7 with NaN in the columns it must not read.

tests/test_bf16_oracle_cpu.py checks the cases without a GPU (cap 2e-2, inputs bite, the rule rejects planted defects).

Measured errors of the bf16 chain, relative to high = 2.5, beside the oracle's (MI355X; the tests print them: run with -s):

  case             measured max  rms        oracle e_max  e_rms      tolerance max  rms
  t256_ragged      3.51e-03      7.23e-04   4.02e-03      9.19e-04   1.61e-02       3.67e-03
  t128_511         2.66e-03      5.84e-04   3.52e-03      1.22e-03   1.41e-02       4.90e-03
  one_row          1.43e-03      8.53e-04   9.86e-04      7.41e-04   3.94e-03       2.96e-03
  past_tile        2.99e-03      9.18e-04   3.64e-03      1.28e-03   1.45e-02       5.11e-03
  modelA           3.03e-03      6.91e-04   3.93e-03      1.01e-03   1.57e-02       4.04e-03
  k64_t256         4.16e-03      6.87e-04   3.95e-03      8.49e-04   1.58e-02       3.40e-03
  k64_t128         2.30e-03      6.66e-04   3.41e-03      1.15e-03   1.36e-02       4.60e-03
  trainer_modelB   1.62e-03      7.09e-04   3.25e-03      9.70e-04   1.30e-02       3.88e-03
  trainer_modelA   2.90e-03      7.26e-04   3.57e-03      1.29e-03   1.43e-02       5.17e-03

Measured with this file on top of commit ee6e30f. The chain sits AT the bf16-operand oracle's own distance from float64 (0.6 .. 1.5 x
its e_max, 0.5 .. 1.2 x its e_rms), nowhere near the 2e-2 budget of tests/test_gpu_wide.py; no measured error exceeds half its
tolerance (largest share: one_row, 0.36 of the maximum's), the used, the poisoned and the fresh workspace gave the same figures to all
printed digits, and no kernel defect was found. actor_set: 2.2e-08 .. 1.0e-07 of high from the float64 oracle (allowed 2e-05), at most
9.5e-08 from the rows kernel (allowed 2e-06), at every shape.

The states are drawn with std 12 .. 32, not the 1.5 of the other tests: at 1.5 the outputs of a set's rows differ by about a
hundredth of high and a row holding its neighbour's output would pass (the case table in tests/bf16_oracle.py says which case takes
what, and why).
"""
import functools

import numpy as np
import pytest
import torch

from avddpg_amd import _hip, config, trainer, vec
from oracle import mlp as omlp
from tests import bf16_oracle as bo
from tests.gpu_util import need_gpu, t
from tests.test_gpu_mlp import FWD_TOL, _perturbed_group

pytestmark = pytest.mark.gpu
HIGH = bo.HIGH
SENTINEL = 0x7FA5C3A5  # a NaN bit pattern no kernel produces
FWD_NAMES = [c.name for c in bo.FWD_CASES]
assert FWD_TOL == bo.FWD_TOL


@functools.lru_cache(maxsize=None)
def _slabs(name):
    """(theta, stats) of the case's perturbed sets on the host (tests/bf16_oracle.py perturbed_slabs: the slabs its oracles unpack)."""
    case = bo.FWD_CASE[name]
    _, th, st, _, _ = bo.perturbed_slabs(case.n_sets, case.S, case.seed, **bo.fwd_conf_kw(case))
    return torch.from_numpy(th.copy()), torch.from_numpy(st.copy())


def _load(grp, name):
    th, st = _slabs(name)
    assert grp.theta.shape == th.shape and grp.stats.shape == st.shape
    grp.theta.copy_(th), grp.stats.copy_(st)
    return grp


def _group(name):
    """A fresh AgentGroup (no workspace yet) with the case's weights."""
    case = bo.FWD_CASE[name]
    grp = vec.AgentGroup(case.n_sets, case.S, 1, config.Config(**bo.fwd_conf_kw(case)), seed=case.seed)
    assert grp.high == HIGH
    return _load(grp, name)


def _framed(rows, cols, pad=300):
    """(buffer of SENTINEL bits, its [rows, cols] block in the middle as a contiguous view)."""
    buf = torch.full((2 * pad + rows * cols,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    return buf, buf[pad:pad + rows * cols].view(rows, cols)


def _assert_frame(buf, rows, cols, pad=300, written=True):
    bits = buf.view(torch.int32)
    assert bool((bits[:pad] == SENTINEL).all()) and bool((bits[pad + rows * cols:] == SENTINEL).all()), "written outside out"
    inside = bits[pad:pad + rows * cols] == SENTINEL
    assert bool((~inside).all() if written else inside.all()), ("element(s) of out not written" if written else "out written")


def _check(name, got, what=""):
    fr = bo.fwd_reference(name)
    e_max, e_rms = bo.fwd_errors(got, fr.ref)
    print(f"{name}{what}: measured max {e_max:.3e} rms {e_rms:.3e} | oracle e_max {fr.e_max:.3e} e_rms {fr.e_rms:.3e} | "
          f"tolerance max {fr.tol_max:.3e} rms {fr.tol_rms:.3e}")
    assert got.shape == fr.ref.shape and bo.fwd_violations(got, fr.ref, fr.tol_max, fr.tol_rms) == [], (name, what, e_max, e_rms)


@pytest.mark.parametrize("name", FWD_NAMES)
def test_actor_shared_holds_every_row_of_every_set_to_the_rule_and_stays_inside_out(name):
    """actor_shared on the set-major states into a framed `out`: every row of every set within the rule; the frame on both sides of the
    [sets, Ns] block bit-identical (padding rows Ns .. Np never reach `out`), every element of the block written."""
    need_gpu()
    case, fr = bo.FWD_CASE[name], bo.fwd_reference(name)
    grp = _group(name)
    buf, out = _framed(case.n_sets, case.P)
    ret = grp.actor_shared(t(fr.x.copy()), case.n_sets * case.P, out=out)
    torch.cuda.synchronize()
    assert ret is out
    _assert_frame(buf, case.n_sets, case.P)
    _check(name, out.cpu().numpy())
    plain = grp.actor_shared(t(fr.x.copy()), case.n_sets * case.P)  # (the allocating form; f32 atomics in another order)
    assert plain.shape == (case.n_sets, case.P) and float((plain - out).abs().max()) <= FWD_TOL * HIGH


def test_actor_shared_in_a_used_a_poisoned_and_a_fresh_workspace():
    """t256_ragged and t128_511 (same widths, other weights and row counts) three ways: (1) on ONE group, t128_511 after t256_ragged, in
    the first call's larger, used workspace (it only ever grows); (2) in a workspace of 0xFF bytes (NaN in every format) half as large
    again as needed; (3) each on a fresh group. All meet the rule and agree within FWD_TOL x high (not bit for bit: the head sums are
    f32 atomics)."""
    need_gpu()
    a, b = "t256_ragged", "t128_511"
    x = {n: t(bo.fwd_reference(n).x.copy()) for n in (a, b)}
    n_agents = {n: bo.FWD_CASE[n].n_sets * bo.FWD_CASE[n].P for n in (a, b)}
    got = {n: {} for n in (a, b)}
    grp = _group(a)
    got[a]["used"] = grp.actor_shared(x[a], n_agents[a]).cpu().numpy()
    big = grp._wide_act_ws
    got[b]["used"] = _load(grp, b).actor_shared(x[b], n_agents[b]).cpu().numpy()
    assert grp._wide_act_ws is big  # the second call ran in the first one's workspace
    small = _group(b)
    got[b]["fresh"] = small.actor_shared(x[b], n_agents[b]).cpu().numpy()
    assert small._wide_act_ws.numel() < big.numel()
    got[a]["fresh"] = _group(a).actor_shared(x[a], n_agents[a]).cpu().numpy()
    for n in (a, b):
        grp = _group(n)
        grp._wide_act_ws = poisoned = torch.full((big.numel() * 3 // 2,), 0xFF, dtype=torch.uint8, device="cuda")
        got[n]["poisoned"] = grp.actor_shared(x[n], n_agents[n]).cpu().numpy()
        assert grp._wide_act_ws is poisoned
    for n in (a, b):
        for how, g in got[n].items():
            _check(n, g, f" ({how} workspace)")
            d = np.abs(g - got[n]["fresh"]).max()
            assert d <= FWD_TOL * HIGH, (n, how, d)


def test_actor_shared_refusals_stay_refusals_and_leave_out_untouched():
    need_gpu()
    conf = config.Config(actor_layer1_size=96, critic_layer1_size=96)
    grp = vec.AgentGroup(2, 4, 1, conf)
    assert grp.lay.H1 == 96
    buf, out = _framed(2, 8)
    with pytest.raises(_hip.AvdError, match="multiples of 64"):
        grp.actor_shared(torch.zeros(2, 8, 4, device="cuda"), 16, out=out)
    grp = _group("past_tile")  # 3 sets
    buf2, out2 = _framed(3, 3)
    with pytest.raises(_hip.AvdError, match="must be a multiple of n_sets=3"):
        grp.actor_shared(torch.zeros(3, 3, 4, device="cuda"), 10, out=out2)
    torch.cuda.synchronize()
    _assert_frame(buf, 2, 8, written=False), _assert_frame(buf2, 3, 3, written=False)
    assert getattr(grp, "_wide_act_ws", None) is None  # (refused before a workspace was made)


@pytest.mark.parametrize("name", [c.name for c in bo.TRAINER_CASES])
def test_trainer_acts_for_every_agent_on_its_own_observation_with_its_own_set(name):
    """VecTrainer at 8 platoons x 5 vehicles, 1024/1024, interfrl (the batched engine, acting through _act_wide_shared exactly as a step
    does): actor_out[p * M + m] against the float64 oracle's actor of set m on agent (p, m)'s observation, taken from a copy of
    env.agent_states() made before; the rule of tests/bf16_oracle.py on these 40 rows. Model A: the fourth float of every agent is NaN
    -- a run that reads four floats, or strides by three, fails. The expected outputs with P and M swapped miss the rule."""
    need_gpu()
    case, fr = bo.FWD_CASE[name], bo.fwd_reference(name)
    P, M, S = case.P, case.n_sets, case.S
    H1, H2, _ = case.widths
    conf = config.Config(num_platoons=P, pl_size=M, buffer_size=128, fed_method="interfrl", weighted_average_enabled=False,
                         model="ModelA" if S == 3 else "ModelB", actor_layer1_size=H1, actor_layer2_size=H2, critic_layer1_size=H1,
                         critic_layer2_size=H2)
    vt = trainer.VecTrainer(conf, rng="device", auto_reset=True)
    assert vt.shared and vt.shared_engine == "batched" and vt.agents.lay.H2 > 256 and (vt.S, vt.M, vt.P, vt.agents.n_sets) == (S, M, P, M)
    _load(vt.agents, name)
    vt.reset_episode()
    vt.env.agent_states().copy_(t(bo.trainer_env_states(case, np.nan if S == 3 else 0.0)))
    seen = vt.env.agent_states().clone().cpu().numpy()  # [P, M, 4]
    vt.actor_out.fill_(float("nan"))
    vt._act_wide_shared(vt.env.agent_states())
    got = vt.actor_out.cpu().numpy().reshape(P, M)
    want = np.empty((P, M))
    for m in range(M):
        w = bo.fwd_actor(case, m)
        for p in range(P):
            want[p, m] = omlp.actor_forward(w, seen[p, m, :S].astype(np.float64)[None], HIGH)[0, 0]
    assert np.max(np.abs(want.T - fr.ref)) <= 1e-9 * HIGH  # the rule's reference is this very expectation, set-major
    assert fr.tol_max <= bo.FWD_CAP
    bo.fwd_inputs_bite(want.T, fr.active1, fr.active2)
    _check(name, got.T)
    assert np.isfinite(got).all() and len(np.unique(got)) == P * M  # distinct sets and distinct platoons: distinct actions
    assert len(bo.fwd_violations(got.T, want.reshape(M, P), fr.tol_max, fr.tol_rms)) == 2  # the planted axis swap fails
    # ... and a whole step runs the same method: same actor outputs (up to the order of the head's atomics), then it moves on
    vt.actor_out.fill_(float("nan"))
    if S == 3:
        vt.env.agent_states()[..., 3] = 0.0  # (the plant reads the fourth float)
    vt.step()
    assert float((vt.actor_out.view(P, M) - t(got)).abs().max()) <= FWD_TOL * HIGH and vt.env_steps == P


@pytest.mark.parametrize("S,P,M", [(4, 1, 1), (4, 31, 3), (4, 32, 3), (3, 33, 64), (4, 65, 1)])
def test_actor_set_every_row_against_the_oracle_at_the_workgroup_edges(S, P, M):
    """csrc/act.hip: a workgroup takes 32 platoons of a set, rows beyond P are redirected to agent 0. Every agent against the float64
    oracle (FWD_TOL) and the rows kernel (2e-6), `out` framed; the same states at x_stride = 7 with NaN in every column from S on:
    finite and bit-identical; with run_if_nonzero reading 0 nothing is written."""
    need_gpu()
    n = P * M
    conf, grp = _perturbed_group(M, S=S, seed=141 + P)
    rs = np.random.RandomState(142 + P)
    x = rs.normal(0, 1.5, size=(n, 4)).astype(np.float32)  # env layout: 4 floats per agent, the first S are the observation
    want = np.empty(n)
    for m in range(M):
        w = [v.astype(np.float64) for v in grp.get_weights(m, "actor")]
        want[m::M] = omlp.actor_forward(w, x[m::M, :S].astype(np.float64), HIGH)[:, 0]
    # the comparison can fail: the agents' outputs differ by far more than the tolerance
    assert np.abs(want).max() > 0.05 and (n == 1 or np.ptp(want) >= 100 * FWD_TOL * HIGH) and np.mean(np.abs(want) < 0.99 * HIGH) >= 0.5
    buf, out = _framed(1, n)
    grp.actor_set(t(x), n, x_stride=4, out=out.view(-1))
    torch.cuda.synchronize()
    _assert_frame(buf, 1, n)
    got = out.view(-1).cpu().numpy()
    rows = grp.actor(t(x), set_mod=M, x_stride=4).cpu().numpy()
    e_or, e_rows = np.abs(got - want).max() / HIGH, np.abs(got - rows).max() / HIGH
    print(f"actor_set S={S} P={P} M={M}: vs float64 oracle {e_or:.2e} (allowed {FWD_TOL:.0e}), vs rows kernel {e_rows:.2e} (allowed 2e-06)")
    assert e_or <= FWD_TOL and e_rows <= 2e-6
    x7 = np.full((n, 7), np.nan, np.float32)
    x7[:, :S] = x[:, :S]
    buf7, out7 = _framed(1, n)
    grp.actor_set(t(x7), n, x_stride=7, out=out7.view(-1))
    torch.cuda.synchronize()
    _assert_frame(buf7, 1, n)
    assert bool(torch.isfinite(out7).all()) and torch.equal(out7, out)
    buf0, out0 = _framed(1, n)
    grp.actor_set(t(x), n, x_stride=4, out=out0.view(-1), run_if_nonzero=torch.zeros(1, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    _assert_frame(buf0, 1, n, written=False)
