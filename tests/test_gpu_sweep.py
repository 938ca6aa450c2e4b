"""Hyperparameter sweeps (VecTrainer(seeds=..., hparams=...), `tr --sweep`): E experiments with their own actor_lr, critic_lr, tau, gamma
and OU noise in one launch chain, each the run its own Config gives alone.

The *_hp_* entry points against the scalar ones called with each row's values on the same full-size batch (bitwise, per experiment
slice); whole runs against solo runs; each table value read where it should be; the guard rails; the CLI's directories."""
import copy
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from avddpg_amd import _hip, config, trainer, vec
from avddpg_amd._hip import call, ptr, stream_handle

from tests.gpu_util import need_gpu
from tests.test_gpu_seed_batch import _compare_runs, _conf, _deint, _eq, _run, _stats_and_sims

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS3 = [dict(actor_lr=1e-4, critic_lr=2e-3, tau=0.01, gamma=0.9, std_dev=0.05, theta=0.3),
         dict(actor_lr=3e-5, critic_lr=5e-4, tau=0.003, gamma=0.99, std_dev=0.2, theta=0.05),
         dict(actor_lr=5e-4, critic_lr=1e-4, tau=0.1, gamma=0.5, std_dev=0.0, theta=0.15)]


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _table(conf, rows):
    return vec.hparams_table(vec.hparams_rows(conf, rows), conf.ou_dt, "cuda")


# ---- 1. the entry points ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [3, 5])
def test_step_fused_hp_equals_seeds_entry_per_row(L):
    need_gpu()
    E, Pe, S = 3, 7, 4
    P = E * Pe
    seeds = (5, 17, 2 ** 40 + 3)
    conf = config.Config(pl_size=L, num_platoons=P)
    env = vec.VecPlatoon(P, L, conf, rng="device", seeds=seeds)
    tbl = _table(conf, ROWS3)
    g = _gen(11)
    f32 = dict(dtype=torch.float32, device="cuda")
    rn = lambda *sh: torch.randn(*sh, generator=g, device="cuda")
    cap = 16
    inp = dict(x=0.3 * rn(P, L, 4), pa=0.1 * rn(P, L), act=rn(P, L), ou=0.2 * rn(P, L), ring=rn(P * L, cap, 2 * S + 2), er=rn(P, L))

    def step(row):
        o = dict(x=torch.empty(P, L, 4, **f32), pa=inp["pa"].clone(), rew=torch.empty(P, L, **f32), done=torch.empty(P, dtype=torch.uint8,
                 device="cuda"), flag=torch.zeros(2, dtype=torch.int32, device="cuda"), ou=inp["ou"].clone(), action=torch.empty(P, L, **f32),
                 exog=torch.empty(P, **f32), ring=inp["ring"].clone(), er=inp["er"].clone())
        head = (ptr(env.d_consts), P, L, S, ptr(inp["x"]), ptr(o["x"]), ptr(o["pa"]), None, ptr(o["rew"]), None, ptr(o["done"]),
                ptr(o["flag"][0:1]), ptr(o["flag"][1:2]), ptr(inp["act"]), ptr(o["ou"]), ptr(o["action"]), ptr(o["exog"]))
        tail = (9, 13, ptr(o["ring"]), cap, 1000 * cap + 5, ptr(o["er"]), stream_handle())
        if row is None:
            call("avd_step_fused_hp_f32", *head, 0.0, conf.ou_dt, conf.action_low, conf.action_high, conf.reset_max_u, 0, ptr(env.d_seeds),
                 ptr(tbl), E, *tail)
        else:
            call("avd_step_fused_seeds_f32", *head, row["theta"], 0.0, conf.ou_dt, row["std_dev"], conf.action_low, conf.action_high,
                 conf.reset_max_u, 0, ptr(env.d_seeds), E, *tail)
        return o

    got = step(None)
    for e, row in enumerate(ROWS3):
        ref = step(row)
        for n in ("x", "pa", "rew", "done", "ou", "action", "exog", "er"):
            _eq(_deint(got[n], E, e), _deint(ref[n], E, e), f"step {n} e={e}")
        _eq(_deint(got["ring"], E, e, L), _deint(ref["ring"], E, e, L), f"step ring e={e}")


def _group(E, M, k, S=4, conf=None):
    conf = conf or config.Config(pl_size=M)
    grp = vec.AgentGroup(E * M * k, S, 1, conf, seeds=(5, 17, 2 ** 31 + 3)[:E], seed_block=M)
    g = _gen(7)
    for t in (grp.m, grp.v):
        t.copy_(1e-3 * torch.randn(t.shape, generator=g, device="cuda").abs())
    grp.step.fill_(4)
    return grp


def _clone(grp, row=None):
    c = copy.copy(grp)
    for n in ("theta", "stats", "theta_t", "stats_t", "m", "v", "step"):
        setattr(c, n, getattr(grp, n).clone())
    c.theta_alt = None
    if row is not None:
        c.config = config.Config(**{**{k: getattr(grp.config, k) for k in ("pl_size",)}, **row})
        c.hp = None
    return c


def _batch(n, S, seed=3):
    g = _gen(seed)
    rn = lambda *sh: torch.randn(*sh, generator=g, device="cuda")
    return 1.5 * rn(n, 64, S), 2.0 * rn(n, 64, 1).clamp(-1.25, 1.25), -0.3 * rn(n, 64).abs(), 1.5 * rn(n, 64, S)


_STATE = ("theta", "stats", "theta_t", "stats_t", "m", "v", "step")


@pytest.mark.parametrize("S", [3, 4])
@pytest.mark.parametrize("act", [False, True])
def test_learn_update_hp_equals_scalar_per_row(S, act):
    need_gpu()
    E, M, k = 3, 3, 2
    grp = _group(E, M, k, S)
    n = grp.n_sets
    s, a, r, s2 = _batch(n, S)
    nx = torch.randn(n, 4, generator=_gen(9), device="cuda")
    f32 = dict(dtype=torch.float32, device="cuda")

    def run(g):
        out = torch.zeros(n, **f32)
        g.learn_update(s, a, r, s2, torch.zeros(n, g.lay.theta_size, **f32), losses=torch.zeros(n, 2, **f32),
                       next_states=nx if act else None, x_stride=4, next_actions=out if act else None)
        return out

    hp = _clone(grp)
    hp.set_hparams(_table(grp.config, ROWS3), E, M)
    out = run(hp)
    for e, row in enumerate(ROWS3):
        ref = _clone(grp, row)
        ro = run(ref)
        for nm in _STATE:
            _eq(_deint(getattr(hp, nm), E, e, M), _deint(getattr(ref, nm), E, e, M), f"{nm} e={e}")
        if act:
            _eq(_deint(out, E, e, M), _deint(ro, E, e, M), f"next actions e={e}")


@pytest.mark.parametrize("S", [3, 4])
def test_learn_and_adam_hp_equal_scalar_per_row_on_shared_sets(S):
    """per_agent interfrl: learn with set_mod = E*M over the agents, then Adam + Polyak of the E*M sets."""
    need_gpu()
    E, M, Pn = 3, 3, 4
    grp = _group(E, M, 1, S)
    n = Pn * E * M
    s, a, r, s2 = _batch(n, S, 5)
    f32 = dict(dtype=torch.float32, device="cuda")

    def run(g):
        grads = g.learn(s, a, r, s2, E * M, losses=torch.zeros(n, 2, **f32))
        avg = vec.fed_mean(grads, Pn, E * M)
        g.apply(avg)
        return grads

    hp = _clone(grp)
    hp.set_hparams(_table(grp.config, ROWS3), E, M)
    gh = run(hp)
    for e, row in enumerate(ROWS3):
        ref = _clone(grp, row)
        gr = run(ref)
        _eq(_deint(gh, E, e, M), _deint(gr, E, e, M), f"grads e={e}")
        for nm in _STATE:
            _eq(getattr(hp, nm).view(E, M, -1)[e], getattr(ref, nm).view(E, M, -1)[e], f"{nm} e={e}")


def test_guarded_adam_hp_skips_the_nan_set_as_the_scalar_form():
    need_gpu()
    E, M = 3, 2
    grp = _group(E, M, 2)
    grads = 1e-2 * torch.randn(grp.n_sets, grp.lay.theta_size, generator=_gen(4), device="cuda")
    grads[7].fill_(float("nan"))
    hp = _clone(grp)
    hp.set_hparams(_table(grp.config, ROWS3), E, M)
    hp.apply(grads, guarded=True)
    for e, row in enumerate(ROWS3):
        ref = _clone(grp, row)
        ref.nonfinite_skipped = None
        ref.apply(grads, guarded=True)
        for nm in _STATE:
            _eq(_deint(getattr(hp, nm), E, e, M), _deint(getattr(ref, nm), E, e, M), f"{nm} e={e}")
    assert int(hp.nonfinite_skipped.item()) == 1
    _eq(hp.theta[7], grp.theta[7], "the NaN set's weights are untouched")
    assert int(hp.step[7]) == int(grp.step[7])


def test_rows_equal_to_conf_give_the_non_hp_path_bitwise():
    need_gpu()
    E, M, S = 2, 3, 4
    grp = _group(E, M, 2, S)
    n = grp.n_sets
    s, a, r, s2 = _batch(n, S, 8)
    f32 = dict(dtype=torch.float32, device="cuda")
    outs = []
    for use_hp in (False, True):
        g = _clone(grp)
        if use_hp:
            g.set_hparams(_table(grp.config, [{}] * E), E, M)
        g.learn_update(s, a, r, s2, torch.zeros(n, g.lay.theta_size, **f32))
        gr = g.learn(s, a, r, s2, 0)
        g.apply(gr)
        outs.append(g)
    for nm in _STATE:
        _eq(getattr(outs[0], nm), getattr(outs[1], nm), nm)


# ---- 2. whole runs against solo runs ------------------------------------------------------------------------------------------
H2 = [dict(actor_lr=1e-4, gamma=0.95, std_dev=0.05), dict(critic_lr=2e-3, tau=0.01, theta=0.3)]


@pytest.mark.parametrize("fused_update", [True, False])
def test_nofrl_sweep_is_bitwise_its_solo_runs(fused_update):
    need_gpu()
    seeds, P, L, steps = (3, 9), 8, 3, 400
    exps = [(h, k) for h in H2 for k in seeds]
    batch = trainer.VecTrainer(_conf("normal", P, L), rng="device", auto_reset="platoon", fused_update=fused_update,
                               seeds=[k for _, k in exps], hparams=[h for h, _ in exps])
    _run(batch, steps)
    solos = []
    for h, k in exps:
        s = trainer.VecTrainer(_conf("normal", P, L, **h), rng="device", auto_reset="platoon", fused_update=fused_update, seed=k, init_seed=k)
        _run(s, steps)
        solos.append(s)
    _compare_runs(batch, solos, shared=False)
    _stats_and_sims(batch, solos)
    ce = batch.experiment_conf(2)
    assert ce.random_seed == 3 and ce.critic_lr == 2e-3 and ce.actor_lr == config.Config().actor_lr


@pytest.mark.parametrize("weighted", [False, True])
def test_interfrl_per_agent_sweep_is_bitwise_its_solo_runs(weighted):
    need_gpu()
    seeds, P, L, steps = (2, 7, 2), 8, 3, 240
    hps = [H2[0], H2[0], H2[1]]
    kw = dict(weighted_average_enabled=weighted, weighted_window=2)
    batch = trainer.VecTrainer(_conf("interfrl", P, L, **kw), rng="device", auto_reset="platoon", seeds=seeds, hparams=hps)
    assert batch.shared and batch.shared_engine == "per_agent"
    _run(batch, steps)
    solos = []
    for h, k in zip(hps, seeds):
        s = trainer.VecTrainer(_conf("interfrl", P, L, **kw, **h), rng="device", auto_reset="platoon", seed=k, init_seed=k)
        _run(s, steps)
        solos.append(s)
    _compare_runs(batch, solos, shared=True)
    _stats_and_sims(batch, solos)


@pytest.mark.parametrize("name,value", [("actor_lr", 3e-4), ("critic_lr", 3e-3), ("tau", 0.2), ("gamma", 0.5), ("std_dev", 0.3),
                                        ("theta", 0.9)])
def test_each_value_is_read_where_it_should_be(name, value):
    """Same seed twice, one value changed: compared at the first update (after step 65)."""
    need_gpu()
    P, L = 2, 3
    vt = trainer.VecTrainer(_conf("normal", P, L), rng="device", auto_reset="platoon", fused_update=True, seeds=(4, 4),
                            hparams=[{}, {name: value}])
    E, M = 2, L
    if name in ("std_dev", "theta"):
        vt.reset_episode()
        vt.step()
        vt.step()  # (theta first acts on a non-zero OU state)
        a0, a1 = _deint(vt.ou.state, E, 0, M), _deint(vt.ou.state, E, 1, M)
        assert not torch.equal(a0, a1)
        return
    _run(vt, 65)
    assert vt.replay.samples == 1
    ag, A = vt.agents, vt.agents.lay.actor_size
    pick = lambda t, e: _deint(t, E, e, M)
    same = lambda t, sl: torch.equal(pick(t, 0)[:, sl], pick(t, 1)[:, sl])
    act, cri = slice(0, A), slice(A, None)
    if name == "actor_lr":
        assert same(ag.theta, cri) and not same(ag.theta, act) and same(ag.m, slice(None))
    elif name == "critic_lr":
        assert same(ag.theta, act) and not same(ag.theta, cri) and same(ag.m, slice(None))
    elif name == "tau":
        assert same(ag.theta, slice(None)) and same(ag.m, slice(None)) and same(ag.v, slice(None))
        assert not same(ag.theta_t, act) and not same(ag.theta_t, cri)
    else:  # gamma: the critic's TD target; the actor's gradient takes the pre-update critic
        assert not same(ag.theta, cri) and same(ag.theta, act) and same(ag.m, act)


def test_rejected_sweeps_raise_before_any_launch(monkeypatch):
    need_gpu()
    calls = []
    real = _hip.call
    monkeypatch.setattr(trainer, "call", lambda name, *a: (calls.append(name), real(name, *a)))
    monkeypatch.setattr(vec, "call", lambda name, *a: (calls.append(name), real(name, *a)))
    ok = dict(rng="device", auto_reset="platoon", seeds=(1, 2))
    cases = [
        (dict(fed_method="normal"), dict(ok, hparams=[{"lr": 1}, {}]), "unknown key"),
        (dict(fed_method="normal"), dict(ok, hparams=[{"tau": float("inf")}, {}]), "not finite"),
        (dict(fed_method="normal"), dict(ok, hparams=[{"actor_lr": 0}, {}]), "> 0"),
        (dict(fed_method="normal"), dict(ok, hparams=[{"tau": 2}, {}]), r"\(0, 1\]"),
        (dict(fed_method="normal"), dict(ok, hparams=[{"gamma": -0.1}, {}]), r"\[0, 1\]"),
        (dict(fed_method="normal"), dict(ok, hparams=[{"std_dev": -1}, {}]), ">= 0"),
        (dict(fed_method="interfrl"), dict(ok, hparams=[{}, {"tau": 0.1}], shared_engine="fused"), "per_agent"),
        (dict(fed_method="interfrl"), dict(ok, hparams=[{}, {"tau": 0.1}], shared_engine="batched"), "per_agent"),
        (dict(fed_method="normal", actor_layer1_size=128, critic_layer1_size=128), dict(ok, hparams=[{}, {"tau": 0.1}]), "widths"),
        (dict(fed_method="normal"), dict(ok, hparams=[{}, {"tau": 0.1}], pipeline_chunks=2), "pipeline"),
        (dict(fed_method="normal"), dict(ok, seeds=(1, 1), hparams=[{"tau": 0.1}, {"tau": 0.1}]), "twice"),
        (dict(fed_method="normal"), dict(rng="device", auto_reset="platoon", hparams=[{}]), "needs seeds"),
        (dict(fed_method="normal"), dict(ok, hparams=[{}]), "rows for"),
        (dict(fed_method="intrafrl"), dict(ok, hparams=[{}, {"tau": 0.1}]), "intrafrl"),
        (dict(fed_method="normal"), dict(ok, rng="host", hparams=[{}, {"tau": 0.1}]), "rng='device'"),
    ]
    for ckw, tkw, msg in cases:
        conf = config.Config(num_platoons=2, **{"pl_size": 3, **ckw})
        with pytest.raises(ValueError, match=msg):
            trainer.VecTrainer(conf, **tkw)
    assert all(n == "avd_mlp_layout_init" for n in calls), calls
    # the entry points validate the table arguments before any launch
    vt = trainer.VecTrainer(config.Config(num_platoons=2, pl_size=3), rng="device", auto_reset="platoon", seeds=(1, 1),
                            hparams=[{}, {"tau": 0.1}])
    ag = vt.agents
    with pytest.raises(_hip.AvdError, match="multiple"):
        call("avd_adam_polyak_hp_f32", ag._layp, 5, ptr(ag.theta), ptr(ag.stats), ptr(ag.theta_t), ptr(ag.stats_t), ptr(ag.m), ptr(ag.v),
             ptr(ag.theta), ptr(ag.step), ptr(vt.d_hp), 2, 3, stream_handle())
    with pytest.raises(_hip.AvdError, match="d_hp"):
        call("avd_adam_polyak_hp_f32", ag._layp, 6, ptr(ag.theta), ptr(ag.stats), ptr(ag.theta_t), ptr(ag.stats_t), ptr(ag.m), ptr(ag.v),
             ptr(ag.theta), ptr(ag.step), None, 2, 3, stream_handle())


# ---- 3. the CLI ---------------------------------------------------------------------------------------------------------------
def _cli(args):
    r = subprocess.run([sys.executable, "-m", "avddpg_amd", "tr", *args], cwd=ROOT, capture_output=True, text=True, timeout=600,
                       env={**os.environ, "PYTHONPATH": ROOT})
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout.strip().splitlines()[-1]


def test_cli_sweep_writes_one_directory_per_experiment_equal_to_its_solo_run(tmp_path):
    need_gpu()
    common = ["--rng", "device", "--episodes", "platoon", "--pl_num", "3", "--pl_size", "3", "--total_time_steps", "150",
              "--buffer_size", "400", "--report_every", "50"]
    base = _cli(common + ["--sweep", "actor_lr=5e-5,1e-4", "--sweep", "critic_lr=5e-4,1e-3", "--seeds", "3-4", "--out", str(tmp_path / "b")])
    solo = _cli(common + ["--seed", "4", "--actor_lr", "1e-4", "--critic_lr", "5e-4", "--out", str(tmp_path / "s")])
    rows = list(csv.DictReader(open(os.path.join(base, "sweep.csv"))))
    assert len(rows) == 8
    dirs = [os.path.join(base, r["label"], f"seed{r['seed']}") for r in rows]
    assert len(set(dirs)) == 8
    for r, d in zip(rows, dirs):
        cj = json.load(open(os.path.join(d, "conf.json")))
        assert cj["random_seed"] == int(r["seed"]) and cj["seed_batch"] == [3, 4]
        assert cj["actor_lr"] == float(r["actor_lr"]) and cj["critic_lr"] == float(r["critic_lr"])
        assert cj["sweep"] == [["actor_lr", [5e-5, 1e-4]], ["critic_lr", [5e-4, 1e-3]]]
        assert float(r["pl_rew_for_simulation"]) == cj["pl_rew_for_simulation"]
        last = open(os.path.join(d, "curve.csv")).read().strip().splitlines()[-1].split(",")
        assert r["final_evaluator_score"] == last[4]
    assert [(float(r["actor_lr"]), float(r["critic_lr"]), int(r["seed"])) for r in rows[:3]] == [(5e-5, 5e-4, 3), (5e-5, 5e-4, 4),
                                                                                                  (5e-5, 1e-3, 3)]
    d = os.path.join(base, "actor_lr=0.0001_critic_lr=0.0005", "seed4")
    assert open(os.path.join(d, "curve.csv")).read() == open(os.path.join(solo, "curve.csv")).read()
    cs, cb = json.load(open(os.path.join(solo, "conf.json"))), json.load(open(os.path.join(d, "conf.json")))
    assert cb["pl_rews_for_simulations"] == cs["pl_rews_for_simulations"]
    for f in os.listdir(solo):
        if f.endswith(".npz"):
            a, b = np.load(os.path.join(solo, f)), np.load(os.path.join(d, f))
            assert all(np.array_equal(a[n], b[n]) for n in a.files), f
    # esim on the directory reproduces its last curve score of platoon 1
    last = open(os.path.join(d, "curve.csv")).read().strip().splitlines()[-1].split(",")
    r = subprocess.run([sys.executable, "-m", "avddpg_amd", "esim", d, "--n_timesteps", str(cb["steps_per_episode"])], cwd=ROOT,
                       capture_output=True, text=True, timeout=600, env={**os.environ, "PYTHONPATH": ROOT})
    assert r.returncode == 0, r.stderr[-3000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("platoon 1:")][0]
    assert np.float32(line.split()[-1]) == np.float32(last[4])


# ---- 4. the split-operand set learner (fused3) ------------------------------------------------------------------------------------
def test_learn_set_split_hp_equals_scalar_per_row():
    """One avd_learn_set_split_hp_f16x3 call at E = 3, P = 64, L = 5 against E calls of avd_learn_set_split_f16x3 on the same full-size
    batch, each with row e's gamma: the set count, and with it every reduction tree, is the same -- experiment e's sets bitwise."""
    need_gpu()
    E, P, L = 3, 64, 5
    conf = config.Config(pl_size=L, num_platoons=P, fed_method="interfrl")
    big = vec.AgentGroup(E * L, 4, 1, conf, seeds=(5, 17, 2 ** 31 + 3), seed_block=L)
    g = _gen(3)
    rn = lambda *sh: torch.randn(*sh, generator=g, device="cuda")
    n = P * E * L
    s, a, r, s2 = 1.5 * rn(n, 64, 4), 2.0 * rn(n, 64, 1).clamp(-1.25, 1.25), -0.3 * rn(n, 64).abs(), 1.5 * rn(n, 64, 4)
    f32 = dict(dtype=torch.float32, device="cuda")
    hp = _clone(big)
    hp.set_hparams(_table(conf, ROWS3), E, L)
    lh = torch.zeros(E * L, 2, **f32)
    gh = hp.learn_set_split(s, a, r, s2, n, losses=lh).clone()
    for e, row in enumerate(ROWS3):
        ref = _clone(big, row)
        lr_ = torch.zeros(E * L, 2, **f32)
        gr = ref.learn_set_split(s, a, r, s2, n, losses=lr_).clone()
        _eq(gh.view(E, L, -1)[e], gr.view(E, L, -1)[e], f"grads e={e}")
        _eq(lh.view(E, L, 2)[e], lr_.view(E, L, 2)[e], f"losses e={e}")


def test_fused3_sweep_equals_seed_batches_with_each_rows_conf():
    """The fused3 engine's experiments depend on the set count (its reduction tree), so the yardstick is the seed batch of the same seeds
    whose conf holds row e's values: experiment e's slice of everything bitwise equal (learn via the split learner's HP twin, update via
    the guarded Adam's)."""
    need_gpu()
    seeds, P, L, steps = (4, 8, 15), 8, 5, 150
    mk = lambda conf, **kw: trainer.VecTrainer(conf, rng="device", auto_reset="platoon", shared_engine="fused3", **kw)
    batch = mk(_conf("interfrl", P, L), seeds=seeds, hparams=ROWS3)
    _run(batch, steps)
    assert batch.replay.samples == steps - 64 and batch.nonfinite_updates() == 0
    E, M = 3, L
    for e, row in enumerate(ROWS3):
        sb = mk(_conf("interfrl", P, L, **row), seeds=seeds)
        _run(sb, steps)
        for nm in _STATE:
            t, u = getattr(batch.agents, nm), getattr(sb.agents, nm)
            _eq(t.view(E, M, *t.shape[1:])[e], u.view(E, M, *u.shape[1:])[e], f"{nm} e={e}")
        _eq(_deint(batch.replay.ring, E, e, M), _deint(sb.replay.ring, E, e, M), f"replay ring e={e}")
        _eq(_deint(batch.ou.state, E, e, M), _deint(sb.ou.state, E, e, M), f"ou e={e}")
        for nm in ("x", "prev_a", "ep_len", "done"):
            _eq(_deint(getattr(batch.env, nm), E, e), _deint(getattr(sb.env, nm), E, e), f"env.{nm} e={e}")
        del sb
