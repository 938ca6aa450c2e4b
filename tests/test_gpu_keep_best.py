"""Keeping the best actors seen in training, on the GPU: avd_keep_best_f32 (csrc/best.hip) against tests/keep_best_oracle.py, bit for
bit, over three layouts and a case with more work items than blocks; then VecTrainer.enable_keep_best / keep_best_update / best_scores /
best_agents against a host shadow that replays the rule on evaluator.run_many's counters, the closed loop through best_agents(), the
proof that retention leaves the training state alone, and the CLI's directories.

Kernel case: 7 units x M = 3 sets x NS = 2 seeds over 30 online sets (set_base permuted, with gaps and unused sets at both ends), snapshot slabs
pre-filled with a sentinel, four consecutive calls whose crafted counters give each unit its own history (improve, tie, worse, NaN,
-inf, +inf, improve again). Trainer cases: pl_size 3, 4 platoons, episodes of 60 steps, 160 steps of training, an evaluation every 32."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from avddpg_amd import _hip, config, evaluator, params, trainer, vec
from avddpg_amd._hip import ptr, stream_handle
from tests import keep_best_oracle as kbo
from tests.gpu_util import need_gpu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = {"reference": (4, 1, 256, 128, 48), "hidden1024": (4, 1, *params.padded_widths(1024, 1024, 48)), "small": (3, 1, 64, 32, 16)}
INF, NAN = float("inf"), float("nan")
# level of unit u at call c: counters = level + a small per-unit pattern, so equal levels give equal bits and a higher level a higher score
LEVELS = [[-5, -5, -6, -4],       # improve, tie, worse, improve again
          [-5, NAN, -4, -4],      # improve, NaN, improve again, tie
          [NAN, -7, -8, NAN],     # NaN at the -inf start, first improvement at the second call, worse, NaN
          [-INF, -3, -3, -2],     # -inf does not beat the -inf start
          [-5, -4, -3, -2],       # improves every time
          [-1, -2, -3, -4],       # improves the first time only
          [-5, INF, INF, -1]]     # +inf improves, ties with itself, and is never beaten
EXPECT = [[1, 0, 0, 1], [1, 0, 1, 0], [0, 1, 0, 0], [0, 1, 0, 1], [1, 1, 1, 1], [1, 0, 0, 0], [1, 1, 0, 0]]
SET_BASE = [25, 1, 17, 9, 21, 5, 13]  # permuted, M = 3 sets each at a stride of 4: gaps; sets 28, 29 and 0 belong to nobody
N_UNITS, M, NS, N_SETS = 7, 3, 2, 30


def _bits(t):
    t = torch.as_tensor(t).detach().cpu().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    return t


def _eq(a, b, what):
    a, b = _bits(a), _bits(torch.from_numpy(np.ascontiguousarray(b)) if isinstance(b, np.ndarray) else b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert torch.equal(a, b), f"{what}: {(a != b).sum().item()} of {a.numel()} differ"


class Case:
    """Device arrays of one kernel case and the oracle beside them."""

    def __init__(self, dims, n_units, m, ns, n_sets, set_base, seed=0):
        need_gpu()
        self.lay = _hip.make_layout(*dims, 64)
        self.n_units, self.M, self.NS, self.n_sets = n_units, m, ns, n_sets
        self.g = torch.Generator(device="cuda").manual_seed(seed)
        lay, f32 = self.lay, dict(dtype=torch.float32, device="cuda")
        self.h_base = (ctypes.c_int32 * n_units)(*set_base)
        self.d_base = torch.tensor(list(set_base), dtype=torch.int32, device="cuda")
        rows = n_units * m
        # the sentinel: a finite ramp no weight takes
        self.best_theta = (torch.arange(rows * lay.actor_size, **f32) * 0.5 + 1e6).view(rows, lay.actor_size)
        self.best_stats = (torch.arange(rows * lay.cmms, **f32) * 0.25 - 3e6).view(rows, lay.cmms)
        self.best_score = torch.full((n_units,), -INF, **f32)
        self.best_step = torch.full((n_units,), -1, dtype=torch.int64, device="cuda")
        self.improved = torch.full((n_units,), 7, dtype=torch.int32, device="cuda")
        self.oracle = kbo.KeepBest(n_units, m, self.best_theta.cpu().numpy(), self.best_stats.cpu().numpy())
        self.new_weights()

    def new_weights(self):
        lay = self.lay
        self.theta = torch.randn(self.n_sets, lay.theta_size, generator=self.g, device="cuda")
        self.stats = torch.randn(self.n_sets, lay.stats_size, generator=self.g, device="cuda")

    def snapshot(self):
        return [t.clone() for t in (self.best_theta, self.best_stats, self.best_score, self.best_step, self.improved)]

    def call(self, d_counters, step_now, **over):
        a = dict(lay=ctypes.byref(self.lay), n_units=self.n_units, M=self.M, NS=self.NS, n_sets=self.n_sets, d_base=ptr(self.d_base),
                 h_base=self.h_base, counters=ptr(d_counters), theta=ptr(self.theta), stats=ptr(self.stats), step=step_now,
                 best_theta=ptr(self.best_theta), best_stats=ptr(self.best_stats), best_score=ptr(self.best_score),
                 best_step=ptr(self.best_step), improved=ptr(self.improved))
        a.update(over)
        _hip.call("avd_keep_best_f32", *a.values(), stream_handle())

    def check(self, what):
        o = self.oracle
        _eq(self.improved, o.improved, f"{what}: improved")
        _eq(self.best_score, o.best_score, f"{what}: best_score")
        _eq(self.best_step, o.best_step, f"{what}: best_step")
        _eq(self.best_theta, o.best_theta, f"{what}: best_theta")
        _eq(self.best_stats, o.best_stats, f"{what}: best_stats")


def _counters(levels, pattern):
    """[n_units, NS, M] float32: unit u's level plus its pattern (a NaN / infinite level: in one counter, the others finite)."""
    c = np.array(pattern, dtype=np.float32, copy=True)
    for u, lv in enumerate(levels):
        if np.isfinite(lv):
            c[u] += np.float32(lv)
        else:
            c[u].reshape(-1)[(u + 2) % c[u].size] = lv
    return c


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_kernel_against_the_oracle_over_four_calls(name):
    k = Case(LAYOUTS[name], N_UNITS, M, NS, N_SETS, SET_BASE)
    lay = k.lay
    assert max(SET_BASE) + M <= N_SETS and len(set(SET_BASE)) == N_UNITS and sorted(SET_BASE) != SET_BASE
    assert (lay.actor_size // 4 > _hip.KEEP_CHUNK4) == (name != "small")  # a row takes several work items but for the small layout
    pattern = np.random.RandomState(4).uniform(-0.25, 0.25, (N_UNITS, NS, M)).astype(np.float32)
    sent_t, sent_s = k.best_theta.clone(), k.best_stats.clone()
    for c in range(4):
        if c:
            k.new_weights()  # every call sees other online weights: a copy that should not have happened shows
        cnt = _counters([LEVELS[u][c] for u in range(N_UNITS)], pattern)
        d_cnt = torch.from_numpy(cnt).cuda()
        th0, st0, cnt0, before = k.theta.clone(), k.stats.clone(), d_cnt.clone(), k.snapshot()
        step = 1000 * c + (2 ** 40 if c == 3 else 0)  # (an int64 step)
        k.call(d_cnt, step)
        torch.cuda.synchronize()
        imp = k.oracle.update(cnt, th0.cpu().numpy(), st0.cpu().numpy(), SET_BASE, step)
        assert imp.tolist() == [EXPECT[u][c] for u in range(N_UNITS)], (c, imp.tolist())  # the oracle's decisions, by hand
        k.check(f"{name} call {c}")
        # the online slabs and the counters are only read
        _eq(k.theta, th0, "theta"), _eq(k.stats, st0, "stats"), _eq(d_cnt, cnt0, "counters")
        # a unit that did not improve keeps, bit for bit, what it had: the earlier snapshot, or the sentinel
        for u in range(N_UNITS):
            if not imp[u]:
                r = slice(u * M, (u + 1) * M)
                _eq(k.best_theta[r], before[0][r], f"unit {u} rows"), _eq(k.best_stats[r], before[1][r], f"unit {u} stats rows")
                _eq(k.best_score[u], before[2][u], "score"), _eq(k.best_step[u], before[3][u], "step")
    assert k.best_step.tolist() == [3000 + 2 ** 40, 2000, 1000, 3000 + 2 ** 40, 3000 + 2 ** 40, 0, 1000]
    assert k.best_score[6].item() == INF and not torch.isnan(k.best_score).any()
    assert not torch.equal(k.best_theta, sent_t) and not torch.equal(k.best_stats, sent_s)


def test_more_work_items_than_blocks():
    """The small layout's rows are one work item each: 2800 units x 3 sets are 8400 work items for the 8192 blocks of the capped grid, so
    the stride loop runs twice in 208 blocks. Units share the 50 online sets (a base anywhere in [0, n_sets - M])."""
    n_units, n_sets = 2800, 50
    rng = np.random.RandomState(11)
    base = rng.randint(0, n_sets - M + 1, n_units)
    base[:3] = (n_sets - M, 0, n_sets - M)  # the last admissible base
    k = Case(LAYOUTS["small"], n_units, M, NS, n_sets, base.tolist(), seed=2)
    n_chunks = -(-max(k.lay.actor_size, k.lay.cmms) // 4 // _hip.KEEP_CHUNK4)
    assert n_chunks == 1 and _hip.KEEP_MAX_BLOCKS < n_units * M * n_chunks < 2 * _hip.KEEP_MAX_BLOCKS
    # every third unit holds a best it cannot beat, one unit in 7 scores NaN
    k.best_score[::3] = 100.0
    k.best_step[::3] = 5
    k.oracle.best_score[::3], k.oracle.best_step[::3] = 100.0, 5
    cnt = rng.uniform(-30, -1, (n_units, NS, M)).astype(np.float32)
    cnt[::7, 1, 2] = NAN
    d_cnt = torch.from_numpy(cnt).cuda()
    th0, st0 = k.theta.clone(), k.stats.clone()
    k.call(d_cnt, 77)
    torch.cuda.synchronize()
    imp = k.oracle.update(cnt, th0.cpu().numpy(), st0.cpu().numpy(), base, 77)
    assert 0 < imp.sum() < n_units and imp[-1] + imp[-2] + imp[-3] > 0  # (units past the first stride improved too)
    k.check("capped grid")
    _eq(k.theta, th0, "theta"), _eq(k.stats, st0, "stats")


def test_refused_calls_leave_every_array_unchanged():
    k = Case(LAYOUTS["small"], N_UNITS, M, NS, N_SETS, SET_BASE)
    cnt = torch.full((N_UNITS, NS, M), -1.0, device="cuda")  # (every unit would improve)
    before, th0, st0 = k.snapshot(), k.theta.clone(), k.stats.clone()
    bad = lambda *b: (ctypes.c_int32 * N_UNITS)(*b)
    off = lambda t: ctypes.c_void_p(t.data_ptr() + 4)
    faults = [(dict(lay=None), "null or empty layout"), (dict(n_units=0), "each must be >= 1"), (dict(M=0), "each must be >= 1"),
              (dict(NS=0), "each must be >= 1"), (dict(h_base=bad(25, 1, 17, 9, 21, 5, 28)), r"set_base\[6\]=28 is outside \[0, n_sets - M = 27\]"),
              (dict(h_base=bad(25, -1, 17, 9, 21, 5, 13)), r"set_base\[1\]=-1 is outside"), (dict(n_sets=27), r"set_base\[0\]=25 is outside"),
              (dict(counters=None), "null pointer"), (dict(improved=None), "null pointer"), (dict(best_step=None), "null pointer"),
              (dict(theta=off(k.theta)), "not 16-byte aligned"), (dict(best_theta=off(k.best_theta)), "not 16-byte aligned"),
              (dict(stats=off(k.stats)), "not 16-byte aligned"), (dict(best_stats=off(k.best_stats)), "not 16-byte aligned")]
    for over, msg in faults:
        with pytest.raises(_hip.AvdError, match=rf"failed \(-1\): avd_keep_best_f32: .*{msg}"):
            k.call(cnt, 9, **over)
    torch.cuda.synchronize()
    for got, want, what in zip(k.snapshot(), before, ("best_theta", "best_stats", "best_score", "best_step", "improved")):
        _eq(got, want, what)
    _eq(k.theta, th0, "theta"), _eq(k.stats, st0, "stats")
    k.call(cnt, 9)  # and the same arrays are taken when nothing is wrong
    torch.cuda.synchronize()
    assert k.improved.tolist() == [1] * N_UNITS and k.best_step.tolist() == [9] * N_UNITS


# ---- the trainer ---------------------------------------------------------------------------------------------------------------------
STEPS, EVERY = 160, 32
ARRANGEMENTS = {
    # name: (Config overrides, VecTrainer keywords, evaluation seeds of the retention score)
    "nofrl_fused": (dict(fed_method="normal"), dict(fused_update=True, seed=3, init_seed=3), None),
    "interfrl_shared": (dict(fed_method="interfrl", weighted_average_enabled=False), dict(shared_engine="per_agent", seed=3, init_seed=3), (6, 9)),
    "seed_batch": (dict(fed_method="normal"), dict(fused_update=True, seeds=(3, 8)), (6, 9)),
}


def _trainer(name):
    ckw, tkw, seeds = ARRANGEMENTS[name]
    conf = config.Config(pl_size=3, num_platoons=4, buffer_size=300, episode_sim_time=6.05, **ckw)
    assert conf.steps_per_episode == 60
    vt = trainer.VecTrainer(conf, rng="device", auto_reset="platoon", **tkw)
    vt.reset_episode()
    return vt, seeds


def _addressing(vt):
    """(platoons, run_many keywords, set bases) of the units: the groups evaluator_scores() scores."""
    E, Mv = vt.E, vt.M
    if vt.seeds is not None and vt.shared:
        return list(range(E)), dict(set_mod=Mv, set_bases=[e * Mv for e in range(E)]), [e * Mv for e in range(E)]
    if vt.seeds is not None:
        glob = [vec.batch_platoon(e, p, E) for e in range(E) for p in range(vt.P_exp)]
        return glob, {}, [g * Mv for g in glob]
    if vt.shared:
        return [0], dict(set_mod=Mv), [0]
    return list(range(vt.P)), {}, [p * Mv for p in range(vt.P)]


class Shadow:
    """The retention rule replayed on the host: at each evaluation the online slabs are cloned, the counters come from
    evaluator.run_many on the same weights, and the oracle decides."""

    def __init__(self, vt, seeds):
        self.vt, self.seeds = vt, seeds
        self.platoons, self.kw, self.bases = _addressing(vt)
        lay, ag = vt.agents.lay, vt.agents
        rows = np.concatenate([np.arange(b, b + vt.M) for b in self.bases])
        self.oracle = kbo.KeepBest(len(self.bases), vt.M, ag.theta.cpu().numpy()[rows, :lay.actor_size], ag.stats.cpu().numpy()[rows, :lay.cmms])
        self.history = []

    def evaluate(self, step):
        vt = self.vt
        th, st = vt.agents.theta.cpu().numpy().copy(), vt.agents.stats.cpu().numpy().copy()
        cnt = evaluator.run_many(vt.conf, vt.agents, self.platoons, seeds=self.seeds, **self.kw)[1]
        self.history.append(self.oracle.update(cnt, th, st, self.bases, step))


def _train_with_retention(name, shadow=True):
    vt, seeds = _trainer(name)
    vt.enable_keep_best(seeds)
    sh = Shadow(vt, seeds) if shadow else None
    for k in range(0, STEPS + 1):
        if k:
            vt.step()
        if k % EVERY == 0 or k == STEPS:
            vt.keep_best_update(k)
            if sh:
                sh.evaluate(k)
    torch.cuda.synchronize()
    return vt, sh


@pytest.mark.parametrize("name", list(ARRANGEMENTS))
def test_trainer_retention_equals_the_host_shadow(name):
    need_gpu()
    vt, sh = _train_with_retention(name)
    o, k = sh.oracle, vt._keep
    n_units = {"nofrl_fused": 4, "interfrl_shared": 1, "seed_batch": 8}[name]
    assert k["n_units"] == n_units == o.n_units and k["evaluations"] == len(sh.history) == STEPS // EVERY + 1
    hist = np.array(sh.history)
    print(f"{name}: improved per evaluation\n{hist}\nbest_step {o.best_step.tolist()} best_score {o.best_score.tolist()}")
    # the test shows something only if the snapshot moved after step 0 and also stayed where a later evaluation was no better
    assert hist[0].all(), "every unit improves on the -inf start"
    assert hist[1:].any(), "no unit improved after step 0: pick other seeds or more steps"
    assert not hist[1:].all(), "every evaluation improved every unit: the rule's other branch is not exercised"
    score, step = vt.best_scores()
    _eq(torch.from_numpy(score), o.best_score, "best_score"), _eq(torch.from_numpy(step), o.best_step, "best_step")
    assert score.dtype == np.float32 and step.dtype == np.int64
    _eq(k["theta"], o.best_theta, "snapshot theta"), _eq(k["stats"], o.best_stats, "snapshot stats")
    _eq(k["improved"], sh.history[-1], "improved of the last evaluation")
    # closed loop: the rollout counters of best_agents() reduce by the oracle's formula to exactly best_score
    best = vt.best_agents()
    cnt = evaluator.run_many(vt.conf, best, sh.platoons, seeds=sh.seeds, **sh.kw)[1]
    for u in range(n_units):
        assert kbo.score(cnt[u]).view(np.int32) == score[u].view(np.int32), (u, kbo.score(cnt[u]), score[u])
    # best_agents(): the retained actor blocks at full stride, everything else the final slabs
    lay, ag = vt.agents.lay, vt.agents
    rows = np.concatenate([np.arange(b, b + vt.M) for b in sh.bases])
    assert best.theta.shape == ag.theta.shape and best.stats.shape == ag.stats.shape and best.n_sets == ag.n_sets
    _eq(best.theta[rows, :lay.actor_size], o.best_theta, "best_agents actor blocks")
    _eq(best.stats[rows, :lay.cmms], o.best_stats, "best_agents actor statistics")
    _eq(best.theta[:, lay.actor_size:], ag.theta[:, lay.actor_size:], "best_agents critic blocks")
    _eq(best.stats[:, lay.cmms:], ag.stats[:, lay.cmms:], "best_agents critic statistics")
    _eq(best.theta_t, ag.theta_t, "targets"), _eq(best.stats_t, ag.stats_t, "target statistics")
    # the final actors' score (the last evaluation's counters)
    final = evaluator.run_many(vt.conf, vt.agents, sh.platoons, seeds=sh.seeds, **sh.kw)[1]
    _eq(torch.from_numpy(vt.last_scores()), np.array([kbo.score(final[u]) for u in range(n_units)], dtype=np.float32), "last_scores")
    # the simulation rewards of the retained actors come through the usual call
    sims = vt.run_simulations(agents=best)
    assert np.shape(sims) == np.shape(vt.run_simulations())


def _state(vt):
    ag, env, rp = vt.agents, vt.env, vt.replay
    out = {n: getattr(ag, n) for n in ("theta", "theta_t", "stats", "stats_t", "m", "v", "step")}
    out.update({f"env.{n}": getattr(env, n) for n in ("x", "x_prev", "prev_a", "cum_accel", "reward", "term", "done", "ep_len")})
    out.update({f"ep_stats.{n}": t for n, t in env.ep_stats.items()})
    out.update(ou=vt.ou.state, ring=rp.ring, ep_reward=vt.ep_reward, actor_out=vt.actor_out, actions=vt.actions, leader_exog=vt.leader_exog)
    out = {n: t for n, t in out.items() if t is not None}  # (cum_accel exists only with track_aux)
    host = dict(buffer_counter=rp.buffer_counter, samples=rp.samples, ou_calls=vt.ou.calls, exog_calls=vt.exog_calls, step_count=env.step_count,
                steps_total=vt.steps_total, updates=vt.updates, env_steps=vt.env_steps, episode=vt.episode)
    return out, host


@pytest.mark.parametrize("name", ["nofrl_fused", "interfrl_shared"])
def test_retention_does_not_perturb_training(name):
    need_gpu()
    np.random.seed(12345)
    with_keep, _ = _train_with_retention(name, shadow=False)
    rng_after = np.random.get_state()
    np.random.seed(12345)
    plain, _ = _trainer(name)
    for _ in range(STEPS):
        plain.step()
    torch.cuda.synchronize()
    assert plain._keep is None
    a, ha = _state(with_keep)
    b, hb = _state(plain)
    assert ha == hb and ha["steps_total"] == STEPS and ha["samples"] == STEPS - 64
    for n in a:
        _eq(a[n], b[n], n)
    for x, y in zip(rng_after, np.random.get_state()):  # the caller's global NumPy stream is where it was
        assert np.array_equal(x, y)


# ---- the CLI -------------------------------------------------------------------------------------------------------------------------
def _cli(*args):
    r = subprocess.run([sys.executable, "-m", "avddpg_amd", *args], cwd=ROOT, capture_output=True, text=True, timeout=600,
                       env={**os.environ, "PYTHONPATH": ROOT})
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout.strip().splitlines()


@pytest.mark.parametrize("seeds", [None, "1,2"])
def test_cli_writes_best_and_leaves_every_other_output_alone(tmp_path, seeds):
    need_gpu()
    common = ["tr", "--rng", "device", "--episodes", "platoon", "--total_time_steps", "120"] + ([] if seeds is None else ["--seeds", seeds])
    kept = _cli(*common, "--keep_best", "40", "--out", str(tmp_path / "kept"))[-1]
    plain = _cli(*common, "--out", str(tmp_path / "plain"))[-1]
    subs = [""] if seeds is None else ["seed1", "seed2"]
    for i, sub in enumerate(subs):
        d, p = os.path.join(kept, sub), os.path.join(plain, sub)
        cj, pj = json.load(open(os.path.join(d, "conf.json"))), json.load(open(os.path.join(p, "conf.json")))
        # without the flag: no best/, no best.csv, no keep_best key -- and nothing else differs
        assert not os.path.exists(os.path.join(p, "best")) and not os.path.exists(os.path.join(p, "best.csv")) and "keep_best" not in pj
        assert {k: v for k, v in cj.items() if k not in ("keep_best", "timestamp")} == {k: v for k, v in pj.items() if k != "timestamp"}
        assert open(os.path.join(d, "curve.csv"), "rb").read() == open(os.path.join(p, "curve.csv"), "rb").read()
        files = sorted(f for f in os.listdir(p) if f.endswith(".npz"))
        assert files and files == sorted(f for f in os.listdir(d) if f.endswith(".npz"))
        for f in files:
            x, y = np.load(os.path.join(p, f)), np.load(os.path.join(d, f))
            assert x.files == y.files and all(x[n].tobytes() == y[n].tobytes() for n in x.files), f
        # with it: best/, best.csv, conf.json's keep_best
        kb = dict(cj["keep_best"])
        assert kb["interval"] == 40 and kb["seeds"] == [cj["evaluation_seed"]]
        bd = os.path.join(d, "best")
        bj = json.load(open(os.path.join(bd, "conf.json")))
        assert dict(bj["keep_best"]) == dict(interval=40, seeds=[cj["evaluation_seed"]], evaluations=4)  # steps 0, 40, 80, 120
        assert bj["saved_platoons"] == cj["saved_platoons"] == 1 and len(bj["pl_rews_for_simulations"]) == 1
        assert kb["best_pl_rew_for_simulation"] == bj["pl_rew_for_simulation"] == float(np.average(bj["pl_rews_for_simulations"]))
        assert sorted(f for f in os.listdir(bd) if f.endswith(".npz")) == files
        rows = [r.split(",") for r in open(os.path.join(d, "best.csv")).read().strip().splitlines()]
        assert rows[0] == ["unit", "best_step", "best_score", "final_score"] and len(rows) == 2 and rows[1][0] == "0"
        assert int(rows[1][1]) in (0, 40, 80, 120) and float(rows[1][2]) >= float(rows[1][3])
        assert rows[1][2] == "%.9g" % np.float32(rows[1][2])
        # the retained actors' reward is their rounded best score (one unit, one seed, re_scalar 1); the final actors' the final score
        assert np.float32(bj["pl_rews_for_simulations"][0]) == np.float32(round(np.float32(rows[1][2]), 3))
        assert np.float32(cj["pl_rews_for_simulations"][0]) == np.float32(round(np.float32(rows[1][3]), 3))
        if i == 0:  # esim on best/ as it stands today: its printed reward is best/conf.json's
            out = _cli("esim", bd, "--n_timesteps", str(bj["steps_per_episode"]))
            line = [x for x in out if x.startswith("platoon 1:")][0]
            assert np.float32(line.split()[-1]) == np.float32(bj["pl_rews_for_simulations"][0])


def _best_csv(d):
    rows = [r.split(",") for r in open(os.path.join(d, "best.csv")).read().strip().splitlines()]
    assert rows[0] == ["unit", "best_step", "best_score", "final_score"] and [r[0] for r in rows[1:]] == [str(i) for i in range(len(rows) - 1)]
    return [(int(r[1]), np.float32(r[2]), np.float32(r[3])) for r in rows[1:]]


def test_cli_reference_episodes_with_scenarios(tmp_path, capsys):
    """`tr --keep_best` under the host episode loop (--episodes reference, host RNG), with --scenarios: evaluations at step 0, every 64
    steps and the last step; best/ holds both platoons' retained actors and the suite's files from them."""
    need_gpu()
    from avddpg_amd import __main__ as cli

    conf = config.Config(episode_sim_time=3.05)
    cli.main(["tr", "--pl_num", "2", "--pl_size", "2", "--total_time_steps", "200", "--buffer_size", "300", "--keep_best", "64",
              "--keep_best_seeds", "6-7", "--scenarios", "step", "--out", str(tmp_path)], conf=conf)
    base = capsys.readouterr().out.strip().splitlines()[-1]
    cj, bj = json.load(open(os.path.join(base, "conf.json"))), json.load(open(os.path.join(base, "best", "conf.json")))
    units = _best_csv(base)
    assert len(units) == 2 and all(b >= f and s >= 0 for s, b, f in units)  # per-agent sets: one unit per platoon
    kb, bk = dict(cj["keep_best"]), dict(bj["keep_best"])
    assert kb["interval"] == bk["interval"] == 64 and kb["seeds"] == bk["seeds"] == [6, 7] and bk["evaluations"] >= 2
    # 6 episodes of at most 30 steps: the evaluations are step 0, the multiples of 64 and the last step
    assert all(s % 64 == 0 or s == max(u[0] for u in units) for s, _, _ in units) and max(u[0] for u in units) <= 180
    assert bj["saved_platoons"] == cj["saved_platoons"] == 2 and len(bj["pl_rews_for_simulations"]) == 2
    for f in ("actor1_1.npz", "actor2_2.npz", "critic2_1.npz", "target_actor1_2.npz", "scenarios.csv"):
        assert os.path.exists(os.path.join(base, "best", f)) and os.path.exists(os.path.join(base, f)), f
    assert bj["scenario_suite"] == cj["scenario_suite"]
    # a platoon whose retained actors are the final ones has the final reward
    for p in range(2):
        pairs = [(np.load(os.path.join(base, f"actor{p + 1}_{m}.npz")), np.load(os.path.join(base, "best", f"actor{p + 1}_{m}.npz"))) for m in (1, 2)]
        if all(np.array_equal(x[n], y[n]) for x, y in pairs for n in x.files):
            assert bj["pl_rews_for_simulations"][p] == cj["pl_rews_for_simulations"][p]
        assert bj["pl_rews_for_simulations"][p] >= cj["pl_rews_for_simulations"][p] or kb["seeds"] != [cj["evaluation_seed"]]


def test_cli_sweep_with_pbt(tmp_path, capsys):
    """`tr --sweep --pbt --keep_best`: every experiment directory gains best/ and best.csv, sweep.csv one column; the snapshot stays with
    the experiment."""
    need_gpu()
    import csv

    from avddpg_amd import __main__ as cli

    cli.main(["tr", "--rng", "device", "--episodes", "platoon", "--pl_num", "2", "--pl_size", "3", "--buffer_size", "400", "--sweep",
              "actor_lr=5e-5,1e-4", "--seeds", "4-5", "--pbt", "50", "--keep_best", "40", "--total_time_steps", "120", "--out", str(tmp_path)])
    base = capsys.readouterr().out.strip().splitlines()[-1]
    rows = list(csv.DictReader(open(os.path.join(base, "sweep.csv"))))
    assert len(rows) == 4 and list(rows[0])[-1] == "best_pl_rew_for_simulation"
    assert os.path.exists(os.path.join(base, "pbt.csv"))
    for r in rows:
        d = os.path.join(base, r["label"], f"seed{r['seed']}")
        cj, bj = json.load(open(os.path.join(d, "conf.json"))), json.load(open(os.path.join(d, "best", "conf.json")))
        units = _best_csv(d)
        assert len(units) == 2 and all(s in (0, 40, 80, 120) and b >= f for s, b, f in units)
        assert dict(bj["keep_best"])["evaluations"] == 4 and bj["random_seed"] == int(r["seed"]) and dict(bj["pbt"])["interval"] == 50
        assert float(r["best_pl_rew_for_simulation"]) == dict(cj["keep_best"])["best_pl_rew_for_simulation"] == bj["pl_rew_for_simulation"]
        # (each platoon's best score is at least its final one, rounding to 3 digits is monotone, and the score's seed is the reward's)
        assert all(x >= y for x, y in zip(bj["pl_rews_for_simulations"], cj["pl_rews_for_simulations"]))
        assert os.path.exists(os.path.join(d, "best", "actor2_3.npz"))
