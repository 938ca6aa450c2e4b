"""The optimiser / target-network / federation kernels of csrc/optim.hip against plain references (tests/optim_oracle.py), at the
launch geometries the workload reaches and the toy-sized tests do not: capped grids that stride with a ragged tail, the actor / critic
boundary inside a block, Adam iteration counts far past 3, more than one block of platoons, every closing rule of the reward ring.

Adam + Polyak is compared BIT FOR BIT with the float32 oracle (oracle/mlp.py, whose bias-correction powers are the exact powers
rounded once: tests/test_optim_oracle_cpu.py); the float32 sums with float64 under bounds that count the kernels' roundings.
Each test prints its worst error / bound ratio before it asserts."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from avddpg_amd import _hip, vec
from avddpg_amd._hip import call, ptr, stream_handle
from oracle import mlp as omlp
from tests import optim_oracle as oo
from tests.gpu_util import need_gpu, t

pytestmark = pytest.mark.gpu
F, U = np.float32, oo.U
ACTOR_LR, CRITIC_LR, TAU = 1e-4, 1e-3, 0.005  # (different step sizes: an actor / critic mix-up at the boundary shows)
# the Adam iteration counts every update test covers: the first few, the first counts at which a float32 power that is not correctly
# rounded gives another step size at lr = 1e-3 (4, 9, 20, 45, 58, 61), the counts around which 1 - beta^t becomes 1 (165, 17 321),
# beta^t subnormal and zero (829, 986/987; 87 294, 103 921/103 922), and what a long run reaches
STEP_COUNTS = [1, 2, 3, 4, 9, 20, 45, 58, 61, 100, 164, 165, 829, 986, 987, 1000, 12345, 17320, 17321, 87294, 10**5, 103921, 103922,
               10**6, 2**31 - 1]


@functools.lru_cache(None)
def _layout():
    """The smallest layout that reaches the launchers' branches: more than 2 x 8 x 256 float4 groups per set (a grid capped at 8 blocks
    makes three strides, the last one ragged), the actor / critic boundary inside a block of 256 groups."""
    lay = _hip.make_layout(4, 1, 112, 64, 16, 64)
    n4 = lay.theta_size // 4
    assert 2 * 8 * 256 < n4 < 3 * 8 * 256 and n4 % 256 and lay.actor_size % 1024 and lay.actor_size % 4 == 0
    assert (lay.theta_size, lay.actor_size, lay.stats_size) == (17512, 8212, 736)
    return lay


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _same_bits(got, want):
    return np.array_equal(_bits(got), _bits(want))


def _bad_sets(got, want):
    """rows whose bits differ (for the assertion message)"""
    return np.nonzero((_bits(got) != _bits(want)).reshape(got.shape[0], -1).any(axis=1))[0]


def _steps(rs, n):
    """n Adam iteration counts: STEP_COUNTS, then a spread over five decades, shuffled over the sets"""
    rest = np.concatenate([rs.randint(1, 200, n), rs.randint(200, 20000, n), rs.randint(20000, 2 * 10**6, n)])
    s = np.concatenate([STEP_COUNTS, rs.permutation(rest)[:max(0, n - len(STEP_COUNTS))]]).astype(np.int64)[:n]
    return rs.permutation(s).astype(np.int32)


def _host_state(n_sets, seed):
    """weights, targets, moments (a run in progress: non-zero), statistics, gradients spanning 1e-6 .. 1"""
    lay, rs = _layout(), np.random.RandomState(seed)
    T, S = lay.theta_size, lay.stats_size
    n = lambda *sh: rs.standard_normal(sh).astype(F)
    scale = rs.choice([1e-6, 1e-3, 1.0], size=(n_sets, T)).astype(F)
    h = dict(theta=0.1 * n(n_sets, T), theta_t=0.1 * n(n_sets, T), m=0.3 * scale * n(n_sets, T),
             v=(scale * scale * rs.uniform(0.0, 1.5, (n_sets, T))).astype(F), stats=n(n_sets, S), stats_t=n(n_sets, S),
             grads=scale * n(n_sets, T), step=_steps(rs, n_sets))
    h["v"][:, ::97] = 0  # (fresh elements)
    return h


class _Dev:
    """device copies of a host state"""

    def __init__(self, h):
        for k, x in h.items():
            setattr(self, k, torch.from_numpy(np.ascontiguousarray(x)).cuda())

    def slabs(self):
        return (ptr(self.theta), ptr(self.stats), ptr(self.theta_t), ptr(self.stats_t), ptr(self.m), ptr(self.v), ptr(self.grads),
                ptr(self.step))

    def host(self):
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy() for k in ("theta", "theta_t", "m", "v", "stats", "stats_t", "grads", "step")}


HP_ROWS = [(1e-4, 1e-3, 0.005), (3e-4, 2e-4, 0.01), (5e-5, 2e-3, 0.001)]  # (actor_lr, critic_lr, tau)
HP_BLOCK = 4  # set j takes row (j // 4) % 3


def _hp_table():
    arr = (_hip.HParams * len(HP_ROWS))()
    for row, (alr, clr, tau) in zip(arr, HP_ROWS):
        row.actor_lr, row.critic_lr = alr, clr
        row.tau, row.one_minus_tau = oo.tau_pair(tau)
        row.gamma, row.ou_theta, row.ou_scale = 0.99, 0.15, 0.02
    return torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy()).cuda()


def _per_set_hparams(n_sets, hp):
    """(actor_lr, critic_lr, tau_f, omt_f) of every set as float32 vectors: the scalars, or its row of the sweep table"""
    if not hp:
        tf, of = oo.tau_pair(TAU)
        return np.full(n_sets, ACTOR_LR, F), np.full(n_sets, CRITIC_LR, F), np.full(n_sets, tf, F), np.full(n_sets, of, F)
    rows = [HP_ROWS[(j // HP_BLOCK) % len(HP_ROWS)] for j in range(n_sets)]
    return (np.array([r[0] for r in rows], F), np.array([r[1] for r in rows], F), np.array([oo.tau_pair(r[2])[0] for r in rows], F),
            np.array([oo.tau_pair(r[2])[1] for r in rows], F))


def _oracle_update(h, hp, sets=None):
    """the float32 oracle's Adam + Polyak step of the sets (default: all) of host state h at their iteration counts -> new state"""
    lay = _layout()
    o = {k: x.copy() for k, x in h.items()}
    alr, clr, tf, of = _per_set_hparams(h["theta"].shape[0], hp)
    for k in (range(h["theta"].shape[0]) if sets is None else sets):
        oo.adam_polyak_set(o["theta"][k], o["theta_t"][k], o["m"][k], o["v"][k], o["stats_t"][k], o["stats"][k], h["grads"][k],
                           h["step"][k], lay.actor_size, alr[k], clr[k], tf[k], of[k])
    return o


def _launch_update(d, n_sets, hp, guarded, skipped=None):
    lay = _layout()
    if hp:
        tbl = _hp_table()
        if guarded:
            call("avd_adam_polyak_guarded_hp_f32", C.byref(lay), n_sets, *d.slabs(), ptr(skipped), ptr(tbl), len(HP_ROWS), HP_BLOCK,
                 stream_handle())
        else:
            call("avd_adam_polyak_hp_f32", C.byref(lay), n_sets, *d.slabs(), ptr(tbl), len(HP_ROWS), HP_BLOCK, stream_handle())
    elif guarded:
        call("avd_adam_polyak_guarded_f32", C.byref(lay), n_sets, *d.slabs(), ACTOR_LR, CRITIC_LR, TAU, ptr(skipped), stream_handle())
    else:
        call("avd_adam_polyak_f32", C.byref(lay), n_sets, *d.slabs(), ACTOR_LR, CRITIC_LR, TAU, stream_handle())
    return d.host()


N_SETS = 264  # >= 256: the launcher caps the grid at 8 blocks per set; a multiple of 3 rows x 4 sets of the sweep table


@pytest.mark.parametrize("hp", [False, True], ids=["scalar", "hp"])
def test_adam_polyak_bit_exact_at_real_step_counts(hp):
    """avd_adam_polyak_f32 / avd_adam_polyak_hp_f32, one launch of 264 sets (grid capped: three strides per thread, the last ragged;
    the actor / critic boundary inside block 0's second stride) whose Adam iteration counts are STEP_COUNTS and a spread up to 2e6:
    theta, theta_t, m, v, stats_t bit-equal to the float32 oracle, stats and step unmoved. The hp form: every set against the oracle
    with its own row's step sizes, tau and 1 - tau.
    A mismatch names the sets and their iteration counts: the side that is not the correctly rounded power is then found by copying
    the device's step size out through a one-set, one-step run (m = v = 0, g = 1: theta moves by alpha / (sqrt(0.001...) + eps))."""
    need_gpu()
    h = _host_state(N_SETS, seed=11)
    assert set(STEP_COUNTS) <= set(h["step"].tolist())
    got = _launch_update(_Dev(h), N_SETS, hp, guarded=False)
    want = _oracle_update(h, hp)
    for name in ("theta", "m", "v", "theta_t", "stats_t"):
        bad = _bad_sets(got[name], want[name])
        assert bad.size == 0, (name, "sets", bad[:8], "step counts", sorted(set(h["step"][bad].tolist()))[:16])
    assert _same_bits(got["stats"], h["stats"]) and _same_bits(got["grads"], h["grads"]) and np.array_equal(got["step"], h["step"])
    assert not _same_bits(got["theta"], h["theta"]) and not _same_bits(got["stats_t"], h["stats_t"])


@pytest.mark.parametrize("hp", [False, True], ids=["scalar", "hp"])
def test_adam_polyak_guarded_skips_exactly_the_sets_with_a_nonfinite_head(hp):
    """avd_adam_polyak_guarded_f32 / _guarded_hp_f32 on 264 sets: NaN at the actor head of one, Inf at the critic head of another, NaN
    at both of a third -- untouched bit for bit (theta, theta_t, m, v, stats_t), their iteration count put back, skipped == 3. The
    contract is the two heads only: a set with NaN elsewhere steps (and gets NaN exactly where the oracle does). Every other set is
    bit-equal to the unguarded oracle."""
    need_gpu()
    lay = _layout()
    h = _host_state(N_SETS, seed=12)
    A = lay.actor_size
    poisoned, elsewhere = [5, 130, 263], 77
    h["grads"][5, 0] = np.nan
    h["grads"][130, A] = -np.inf
    h["grads"][263, 0] = h["grads"][263, A] = np.nan
    h["grads"][elsewhere, [1, A - 1, A + 1, lay.theta_size - 1]] = np.nan
    d = _Dev(h)
    skipped = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = _launch_update(d, N_SETS, hp, guarded=True, skipped=skipped)
    stepping = [k for k in range(N_SETS) if k not in poisoned]
    with np.errstate(invalid="ignore"):
        want = _oracle_update(h, hp, sets=stepping)
    assert int(skipped.item()) == 3
    want_step = h["step"].copy()
    want_step[poisoned] -= 1
    assert np.array_equal(got["step"], want_step)
    for name in ("theta", "m", "v", "theta_t", "stats_t"):
        assert _same_bits(got[name][poisoned], h[name][poisoned]), name  # untouched
        g, w = got[name].copy(), want[name].copy()
        nan_g, nan_w = np.isnan(g[elsewhere]), np.isnan(w[elsewhere])
        assert np.array_equal(nan_g, nan_w), name  # NaN where the oracle has it (the payload is not compared)
        if name != "stats_t":
            assert nan_w[[1, A - 1, A + 1, lay.theta_size - 1]].all() and nan_w.sum() == 4
        g[elsewhere][nan_g] = w[elsewhere][nan_w] = 0
        bad = _bad_sets(g, w)
        assert bad.size == 0, (name, bad[:8], h["step"][bad][:8])
    assert _same_bits(got["stats"], h["stats"])
    assert not _same_bits(got["theta"][elsewhere], h["theta"][elsewhere])  # that set did step


# ---- avd_adam_polyak_intra_f32 -----------------------------------------------------------------------------------------------------

@functools.lru_cache(2)
def _intra_state(P, M):
    h = _host_state(P * M, seed=100 + P + M)
    rs = np.random.RandomState(P * 31 + M)
    # different iteration counts inside every platoon, the interesting ones first
    st = np.concatenate([STEP_COUNTS, rs.randint(1, 30000, P * M)])[:P * M].astype(np.int32)
    h["step"] = st
    if M > 1:
        assert all(len(set(row)) > 1 for row in st.reshape(P, M).tolist())
    h["grads"] = rs.standard_normal(h["grads"].shape).astype(F) * rs.choice([1e-3, 1.0], size=(P * M, 1)).astype(F)  # members O(1) apart
    h["weights"] = rs.uniform(0.5, 6.0, P * M).astype(F)
    return h


def _check_intra_against_float64(h, got, dev_mean, P, M, w_host, stepping):
    """(a) of the test below: `got` (the state after the intrafrl update) and dev_mean (the float32 platoon means) against the float64
    mean rounded to float32 and fed to the float32 Adam oracle; returns the worst error / bound ratio."""
    lay = _layout()
    T, A = lay.theta_size, lay.actor_size
    tf, of = oo.tau_pair(TAU)
    st = {k: x for k, x in h.items() if k != "weights"}
    s64, abs64, ws64 = oo.fed_sum64(h["grads"], w_host, *oo.strides("intrafrl", P, M))
    mean64 = s64 / ws64[:, None]
    g_ref = mean64.astype(F)  # [P, T]
    dg = oo.fed_sum_bound(M, abs64, ws64) + U * np.abs(mean64)
    assert np.all(np.abs(dev_mean - mean64) <= dg)
    print(f"intra P={P} M={M} weighted={w_host is not None}: mean error/bound {np.max(np.abs(dev_mean - mean64) / np.maximum(dg, 1e-300)):.3f}")
    ref_in = dict(st, grads=np.repeat(g_ref, M, axis=0))
    ref = _oracle_update(ref_in, hp=False, sets=np.nonzero(stepping)[0])
    alpha = {lr: np.array([omlp.adam_alpha(lr, int(s)) for s in h["step"]], np.float64) for lr in (ACTOR_LR, CRITIC_LR)}
    worst = 0.0
    for p in range(P):  # platoon by platoon: the bound's float64 temporaries stay small
        rows = np.arange(p * M, (p + 1) * M)[stepping[p * M:(p + 1) * M]]
        if rows.size == 0:
            continue
        for lo, hi, lr in ((0, A, ACTOR_LR), (A, T, CRITIC_LR)):
            sl = (rows[:, None], np.arange(lo, hi)[None, :])
            bm, bv, bw, bt = oo.adam_polyak_perturbation_bound(h["theta"][sl], h["theta_t"][sl], h["m"][sl], h["v"][sl], g_ref[p, lo:hi][None, :],
                                                               dg[p, lo:hi][None, :], alpha[lr][rows][:, None], tf, of)
            for name, b in (("m", bm), ("v", bv), ("theta", bw), ("theta_t", bt)):
                err = np.abs(got[name][sl].astype(np.float64) - ref[name][sl])
                r = float(np.max(err / np.maximum(b, 1e-300)))
                worst = max(worst, r)
                assert r <= 1.0, (name, p, r)
    return worst


INTRA_CASES = [(P, M, w, ls) for P, M in ((64, 5), (70, 1), (65, 3), (64, 16), (3, 7)) for w in (False, True)
               for ls in ((0, 1) if M > 1 else (0,))]


@pytest.mark.parametrize("P,M,weighted,lead_skip", INTRA_CASES)
def test_adam_polyak_intra_against_float64_mean_and_four_kernel_path(P, M, weighted, lead_skip):
    """avd_adam_polyak_intra_f32: every agent of a platoon steps with the (weighted) mean of the platoon's M gradient rows. P >= 64
    caps the grid at 8 blocks per platoon (three strides); M = 1, M no multiple of 4 and M = 16 (the kernel's limit) all run.
    (a) Reference: the float64 mean rounded to float32, fed to the float32 Adam oracle at each agent's own iteration count. The
        device's float32 mean is within fed_sum's bound of it (+ the reference's own rounding), so m, v, theta, theta_t are within
        what one Adam + Polyak step does to a gradient perturbed by that much (optim_oracle.adam_polyak_perturbation_bound).
    (b) Bit-equal to fed_mean + fed_scatter + avd_adam_polyak_f32 on copies (same summation order and scaling).
    (c) lead_skip: vehicle 0 of every platoon untouched bit for bit, stats_t included; its gradient still enters the mean.
        stats_t of everyone else: the float32 soft update, bit for bit."""
    need_gpu()
    lay = _layout()
    h = _intra_state(P, M)
    n_sets, T, A = P * M, lay.theta_size, lay.actor_size
    w_host = h["weights"] if weighted else None
    st = {k: x for k, x in h.items() if k != "weights"}
    d = _Dev(st)
    wd = t(w_host) if weighted else None
    call("avd_adam_polyak_intra_f32", C.byref(lay), P, M, lead_skip, *d.slabs(), ptr(wd), ACTOR_LR, CRITIC_LR, TAU, stream_handle())
    got = d.host()
    stepping = np.ones((P, M), bool)
    stepping[:, 0] = not lead_skip
    stepping = stepping.reshape(-1)
    assert np.array_equal(got["step"], h["step"]) and _same_bits(got["grads"], h["grads"]) and _same_bits(got["stats"], h["stats"])

    # (c) the lead vehicles, and the statistics' targets
    tf, of = oo.tau_pair(TAU)
    for name in ("theta", "theta_t", "m", "v", "stats_t"):
        assert _same_bits(got[name][~stepping], h[name][~stepping]), name
    want_stt = h["stats_t"].copy()
    want_stt[stepping] = h["stats"][stepping] * tf + h["stats_t"][stepping] * of
    assert _same_bits(got["stats_t"], want_stt)  # polyak_intra's stats_t obeys lead_skip

    # (b) the four-kernel path on copies
    d2 = _Dev(st)
    avg = vec.fed_mean(d2.grads, P, M, weights=wd, method="intrafrl")
    vec.fed_scatter(avg, d2.grads, P, M, "intrafrl")
    call("avd_adam_polyak_f32", C.byref(lay), n_sets, *d2.slabs(), ACTOR_LR, CRITIC_LR, TAU, stream_handle())
    four = d2.host()
    for name in ("theta", "theta_t", "m", "v"):
        assert _same_bits(got[name][stepping], four[name][stepping]), name

    # (a) the float64 mean
    worst = _check_intra_against_float64(h, got, avg.cpu().numpy(), P, M, w_host, stepping)
    print(f"intra P={P} M={M} weighted={weighted} lead_skip={lead_skip}: worst Adam error/bound {worst:.3f}")


def test_adam_polyak_intra_refuses_more_than_16_vehicles():
    """M = 17 > INTRA_MAX_M: refused before any launch (the kernel's shared arrays hold 16 agents)."""
    need_gpu()
    lay = _layout()
    with pytest.raises(_hip.AvdError, match=r"avd_adam_polyak_intra_f32: P=3 M=17 \(M <= 16\)"):
        call("avd_adam_polyak_intra_f32", C.byref(lay), 3, 17, 0, *([None] * 9), ACTOR_LR, CRITIC_LR, TAU, None)


# ---- fed_sum / fed_finalize / fed_scatter ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("method", ["interfrl", "intrafrl"])
def test_fed_sum_finalize_against_float64(method, weighted):
    """avd_fed_sum_f32 + avd_fed_finalize_f32 for n_in around the four phases and the unroll of 8 per phase (1 .. 5, 31 .. 37, 65),
    n / 4 just below, at and above the 64-column block and over three blocks, both stride patterns, plain and weighted (weights in
    [0.5, 6], one of them zero). Per element |mean - float64 mean| <= (ceil(n_in / 4) + 8) 2^-24 sum|w g| / sum w; wsum within
    n_in 2^-24 relative. The members are O(1) and distinct: a dropped or doubled member misses the bound by orders of magnitude."""
    need_gpu()
    rs = np.random.RandomState(21 + weighted)
    worst = worst_w = 0.0
    for n_in in (1, 2, 3, 4, 5, 31, 32, 33, 36, 37, 65):
        for n_out in (1, 3):
            P, M = (n_in, n_out) if method == "interfrl" else (n_out, n_in)
            geo = oo.strides(method, P, M)
            assert geo[:2] == (n_out, n_in)
            for n in (4, 252, 256, 260, 4 * 64 * 3 + 4):
                g = (rs.standard_normal((P * M, n)) + rs.uniform(-2, 2, (P * M, 1))).astype(F)
                w = None
                if weighted:
                    w = rs.uniform(0.5, 6.0, P * M).astype(F)
                    if n_in > 1:
                        w[rs.randint(P * M)] = 0
                gd, wdv = t(g), (t(w) if weighted else None)
                out = torch.full((n_out, n), 7.0, device="cuda")
                wsum = torch.full((n_out,), -1.0, device="cuda") if weighted else None
                call("avd_fed_sum_f32", *geo, n, ptr(gd), ptr(wdv), ptr(out), ptr(wsum), stream_handle())
                call("avd_fed_finalize_f32", n_out, n, ptr(out), float(n_in), ptr(wsum), stream_handle())
                s64, abs64, ws64 = oo.fed_sum64(g, w, *geo)
                err = np.abs(out.cpu().numpy().astype(np.float64) - s64 / ws64[:, None])
                r = float(np.max(err / oo.fed_sum_bound(n_in, abs64, ws64)))
                worst = max(worst, r)
                assert r <= 1.0, (n_in, n_out, n, r)
                if weighted:
                    rw = float(np.max(np.abs(wsum.cpu().numpy().astype(np.float64) - ws64) / (n_in * U * ws64)))
                    worst_w = max(worst_w, rw)
                    assert rw <= 1.0, (n_in, n_out, n, rw)
    print(f"fed_sum + fed_finalize {method} weighted={weighted}: worst error/bound {worst:.3f}, wsum {worst_w:.3f}")


@pytest.mark.parametrize("n_out,n", [(3, 260), (1, 4), (3, 2048 * 256 // 3 + 1001)])
def test_fed_finalize_alone_bit_exact(n_out, n):
    """avd_fed_finalize_f32 on a given float32 sum: (1 / wsum) * out and out / count as numpy float32 forms them, bit for bit; the last
    shape has more than 2048 x 256 elements, so the capped grid strides."""
    need_gpu()
    rs = np.random.RandomState(n)
    assert n < 10**5 or n_out * n > 2048 * 256
    x = (rs.standard_normal((n_out, n)) * rs.choice([1e-5, 1.0, 300.0], (n_out, n))).astype(F)
    wsum = rs.uniform(0.5, 4000.0, n_out).astype(F)
    a, b = t(x), t(x)
    call("avd_fed_finalize_f32", n_out, n, ptr(a), 0.0, ptr(t(wsum)), stream_handle())
    call("avd_fed_finalize_f32", n_out, n, ptr(b), 37.0, None, stream_handle())
    assert _same_bits(a.cpu().numpy(), (F(1) / wsum)[:, None] * x)
    assert _same_bits(b.cpu().numpy(), x / F(37))


@pytest.mark.parametrize("method", ["interfrl", "intrafrl"])
def test_fed_scatter_writes_the_targeted_rows_and_nothing_else(method):
    """avd_fed_scatter_f32 into a sentinel-filled destination: i_begin 0, 1 and n_in - 1; n / 4 = 1, around the 16-block grid cap
    (4095, 4096, 4097) and two strides past it (8200). Every targeted row equals its source row, every other element keeps the
    sentinel."""
    need_gpu()
    P, M = 3, 4
    n_out, n_in, so, si = oo.strides(method, P, M)
    rows = oo.fed_rows(n_out, n_in, so, si)
    rs = np.random.RandomState(31)
    for n4 in (1, 4095, 4096, 4097, 8200):
        n = 4 * n4
        src = rs.standard_normal((n_out, n)).astype(F)
        sd = t(src)
        for i_begin in (0, 1, n_in - 1):
            dst = torch.full((P * M, n), -12345.0, device="cuda")
            vec.fed_scatter(sd, dst, P, M, method, i_begin=i_begin)
            want = np.full((P * M, n), -12345.0, F)
            for o in range(n_out):
                want[rows[o, i_begin:]] = src[o]
            assert _same_bits(dst.cpu().numpy(), want), (n4, i_begin)


# ---- the reward ring and the federated weights -------------------------------------------------------------------------------------

@pytest.mark.parametrize("zero_after", [0, 1])
@pytest.mark.parametrize("mode", ["force", "cond", "done"])
def test_fed_history_push_follows_the_host_shadow(mode, zero_after):
    """avd_fed_history_push_f32 over one block, the block edge and several blocks of platoons (1, 255, 256, 257, 1000), 3 W + 2 pushes so
    every slot wraps: after EVERY push the ring (slot hist_cnt % W), hist_cnt and ep_reward equal the host shadow exactly, rows of
    platoons that did not close included. force: the caller's step limit, on alternate pushes (the others: a cond flag that reads 0);
    cond: a device flag toggled between pushes; done: per-platoon flags and ep_len + 1 >= limit, other platoons on every push
    (ep_len absent on every third push: the flags alone)."""
    need_gpu()
    rs = np.random.RandomState(41 + zero_after)
    limit = 7
    for P in (1, 255, 256, 257, 1000):
        for M in (1, 5):
            for W in (1, 3):
                ring0 = rs.uniform(-900, -800, (P * M, W)).astype(F)  # (recognisable: a row nobody wrote keeps these)
                cnt0 = rs.randint(0, 2 * W + 1, P).astype(np.int32)  # platoons at different slots
                sh = oo.HistoryShadow(P, M, W, ring0, cnt0)
                ring, cnt = t(ring0), torch.from_numpy(cnt0).cuda()
                ep = rs.uniform(-50, -1, P * M).astype(F)
                epd = t(ep)
                flag = torch.zeros(1, dtype=torch.int32, device="cuda")
                closed_some = closed_all = False
                for k in range(3 * W + 2):
                    inc = rs.uniform(-9, -0.1, P * M).astype(F)
                    ep = ep + inc
                    epd += t(inc)
                    done = ep_len = cond = None
                    force = 0
                    if mode == "force":
                        force, cond = k % 2, flag
                        close = np.full(P, bool(force))
                    elif mode == "cond":
                        on = int(k % 3 != 1)
                        flag.fill_(on)
                        cond, close = flag, np.full(P, bool(on))
                    else:
                        dn = (rs.uniform(size=P) < 0.3).astype(np.uint8)
                        close = dn != 0
                        done = torch.from_numpy(dn).cuda()
                        if k % 3 != 2:
                            el = rs.randint(0, limit + 2, P).astype(np.int32)
                            ep_len = torch.from_numpy(el).cuda()
                            close = close | (el + 1 >= limit)
                    call("avd_fed_history_push_f32", P, M, W, ptr(epd), ptr(done), ptr(ep_len), limit, ptr(cond), force, zero_after,
                         ptr(ring), ptr(cnt), stream_handle())
                    sh.push(ep, close, zero_after)
                    closed_some |= bool(close.any()) and not bool(close.all())
                    closed_all |= bool(close.all())
                    assert _same_bits(ring.cpu().numpy(), sh.ring), (P, M, W, k)
                    assert np.array_equal(cnt.cpu().numpy(), sh.cnt), (P, M, W, k)
                    assert _same_bits(epd.cpu().numpy(), ep), (P, M, W, k)
                assert closed_all if mode != "done" else (closed_some or P == 1)
                assert (sh.cnt - cnt0).max() > W or mode == "done"  # the ring wrapped


FW_CASES = ["on", "off", "auto_on", "auto_one_short_low", "auto_one_short_high"]


@pytest.mark.parametrize("case", FW_CASES)
def test_fed_weights_against_float64(case):
    """avd_fed_weights_f32 for P below, at and above the block of 1024 threads (1, 6, 1023, 1024, 1025, 4096, 5000): negative ring rows
    (this environment's rewards) and one positive row. host_enabled 1 / 0; -1 with every count >= W; -1 with exactly one platoon at
    W - 1, once below index 1024 and once above (where P allows) -- then all ones and wsum == P, exactly.
    Relative bounds against float64 in units of 2^-24, by counting roundings: w: W + 2 (W - 1 additions of one sign, / W, 1 / x);
    wsum: that + ceil(P / 1024) + 10 (a thread's serial additions, the tree of ten levels); agent_weight: the two + 2 (P / wsum, the
    product). sum_p agent_weight[p, m] = P within P 2^-24 x that bound. Two launches on the same inputs give the same bits."""
    need_gpu()
    rs = np.random.RandomState(51)
    worst = [0.0, 0.0, 0.0]
    for P in (1, 6, 1023, 1024, 1025, 4096, 5000):
        if case == "auto_one_short_high" and P <= 1024:
            continue
        for M in (1, 5):
            for W in (1, 3):
                ring = rs.uniform(-300, -5, (P * M, W)).astype(F)
                ring[rs.randint(P * M)] = rs.uniform(5, 300, W).astype(F)  # fabsf
                cnt = rs.randint(W, W + 5, P).astype(np.int32)
                if case.startswith("auto_one_short"):
                    cnt[rs.randint(min(P, 1024)) if case.endswith("low") else rs.randint(1024, P)] = W - 1
                host_enabled = {"on": 1, "off": 0}.get(case, -1)
                if case == "off":
                    cnt[:] = W + 1  # (the counts do not matter)
                rd, cd = t(ring), torch.from_numpy(cnt).cuda()
                outs = []
                for _ in range(2):
                    w_raw, aw, wsum = (torch.full((P * M,), -3.0, device="cuda"), torch.full((P * M,), -3.0, device="cuda"),
                                       torch.full((M,), -3.0, device="cuda"))
                    call("avd_fed_weights_f32", P, M, W, ptr(rd), ptr(cd), host_enabled, ptr(w_raw), ptr(aw), ptr(wsum), stream_handle())
                    outs.append([x.cpu().numpy() for x in (w_raw, aw, wsum)])
                assert all(_same_bits(a, b) for a, b in zip(*outs)), (P, M, W)
                w_raw, aw, wsum = outs[0]
                enabled, w64, aw64, ws64 = oo.fed_weights64(ring, cnt, P, M, W, host_enabled)
                assert enabled == (case in ("on", "auto_on"))
                if not enabled:
                    assert np.all(w_raw == 1) and np.all(aw == 1) and np.all(wsum == F(P)), (P, M, W)
                    continue
                b_w = W + 2
                b_ws = b_w + -(-P // 1024) + 10
                b_aw = b_w + b_ws + 2
                rel = lambda got, ref: float(np.max(np.abs(got.astype(np.float64) - ref) / np.abs(ref))) / U
                r = [rel(w_raw.reshape(P, M), w64) / b_w, rel(wsum, ws64) / b_ws, rel(aw.reshape(P, M), aw64) / b_aw]
                worst = [max(a, b) for a, b in zip(worst, r)]
                assert max(r) <= 1.0, (P, M, W, r)
                assert np.all(np.abs(aw.reshape(P, M).astype(np.float64).sum(axis=0) - P) <= P * U * b_aw), (P, M, W)
                assert np.all(w_raw > 0) and np.all(aw > 0)
    print(f"fed_weights {case}: worst error/bound w {worst[0]:.3f}, wsum {worst[1]:.3f}, agent_weight {worst[2]:.3f}")


def test_polyak_strided_bit_exact():
    """avd_polyak_f32 with more than 2048 x 256 elements (the capped grid strides, ragged tail): w tau + t (1 - tau) as numpy float32
    forms it, bit for bit."""
    need_gpu()
    n = 2048 * 256 + 1003
    rs = np.random.RandomState(61)
    w, tt = rs.standard_normal(n).astype(F), rs.standard_normal(n).astype(F)
    wd, td = t(w), t(tt)
    call("avd_polyak_f32", n, ptr(wd), ptr(td), TAU, stream_handle())
    tf, of = oo.tau_pair(TAU)
    assert _same_bits(td.cpu().numpy(), w * tf + tt * of) and _same_bits(wd.cpu().numpy(), w)
