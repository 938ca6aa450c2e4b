"""Seed batches (VecTrainer(seeds=...), `tr --seeds`): E experiments in one launch chain, each the run its own seed gives alone.

The draw kernels' *_seeds_* entry points against the scalar ones per experiment; whole training runs against solo runs, bitwise
where no kernel reduces over platoons; the set learners within their own tolerances; the guard rails; the CLI's directories."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from avddpg_amd import _hip, config, trainer, vec
from avddpg_amd._hip import call, ptr, stream_handle
from oracle import philox as ophilox

from tests.gpu_util import need_gpu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS3 = (5, 17, 2 ** 40 + 3)


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _deint(t, E, e, per=1):
    """Experiment e's slice of a batch tensor whose leading dim is (platoon g = p*E + e) x per."""
    return t.reshape(-1, E, per, *t.shape[1:])[:, e].reshape(-1, *t.shape[1:])


def _eq(a, b, what):
    a, b = a.cpu(), b.cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype.is_floating_point:
        a, b = a.view(torch.int32), b.view(torch.int32)  # bitwise, NaN-safe
    assert torch.equal(a, b), f"{what}: {(a != b).sum().item()} of {a.numel()} differ"


# ---- 1. the draw kernels ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [3, 5])
@pytest.mark.parametrize("uniform", [False, True])
def test_grouped_draw_kernels_equal_scalar_kernels_per_experiment(L, uniform):
    need_gpu()
    E, Pe, S = len(SEEDS3), 7, 4
    P = E * Pe
    conf = config.Config(pl_size=L, num_platoons=P, rand_gen="uniform" if uniform else "normal")
    env = vec.VecPlatoon(P, L, conf, rng="device", seeds=SEEDS3)
    d_seeds, cst = env.d_seeds, env.d_consts
    g = _gen(11)
    f32 = dict(dtype=torch.float32, device="cuda")
    rn = lambda *sh: torch.randn(*sh, generator=g, device="cuda")
    cap, slot = 16, 5

    def step_inputs(n):
        return dict(x=0.3 * rn(n, L, 4), pa=0.1 * rn(n, L), act=rn(n, L), ou=0.2 * rn(n, L), ring=rn(n * L, cap, 2 * S + 2),
                    er=rn(n, L))

    def step(inp, n, key, grouped):
        o = dict(x=torch.empty(n, L, 4, **f32), pa=inp["pa"].clone(), rew=torch.empty(n, L, **f32),
                 term=torch.empty(n, L, dtype=torch.uint8, device="cuda"), done=torch.empty(n, dtype=torch.uint8, device="cuda"),
                 flag=torch.zeros(2, dtype=torch.int32, device="cuda"), ou=inp["ou"].clone(), action=torch.empty(n, L, **f32),
                 exog=torch.empty(n, **f32), ring=inp["ring"].clone(), er=inp["er"].clone())
        fn = "avd_step_fused_seeds_f32" if grouped else "avd_step_fused_f32"
        call(fn, ptr(cst), n, L, S, ptr(inp["x"]), ptr(o["x"]), ptr(o["pa"]), None, ptr(o["rew"]), ptr(o["term"]), ptr(o["done"]),
             ptr(o["flag"][0:1]), ptr(o["flag"][1:2]), ptr(inp["act"]), ptr(o["ou"]), ptr(o["action"]), ptr(o["exog"]), conf.theta, 0.0,
             conf.ou_dt, conf.std_dev, conf.action_low, conf.action_high, conf.reset_max_u, 1 if uniform else 0, *key, 9, 13,
             ptr(o["ring"]), cap, 1000 * cap + slot, ptr(o["er"]), stream_handle())
        return o

    inp = step_inputs(P)
    got = step(inp, P, (ptr(d_seeds), E), True)
    flag_any = 0
    for e, k in enumerate(SEEDS3):
        sub = {n: (_deint(t, E, e, L) if n == "ring" else _deint(t, E, e)).contiguous() for n, t in inp.items()}
        ref = step(sub, Pe, (k,), False)
        for n in ("x", "pa", "rew", "term", "done", "ou", "action", "exog", "er"):
            _eq(_deint(got[n], E, e), ref[n], f"step_fused {n} e={e}")
        _eq(_deint(got["ring"], E, e, L), ref["ring"], f"step_fused ring e={e}")
        flag_any |= int(ref["flag"][0])
        # OU normals against the oracle's Philox at (seed_e, counter 9, the solo vehicle index)
        w = ophilox.philox_at(k, 9, np.arange(Pe * L), ophilox.STREAM_OU)
        nrm = ophilox.box_muller(w[0], w[1])[0]
        st = sub["ou"].cpu().numpy().reshape(-1)
        want = (st + (np.float32(conf.theta) * (np.float32(0) - st)) * np.float32(conf.ou_dt)) + \
            np.float32(conf.std_dev) * np.float32(np.sqrt(conf.ou_dt)) * nrm
        assert np.allclose(_deint(got["ou"], E, e).cpu().numpy().reshape(-1), want, rtol=0, atol=2e-6)
    assert int(got["flag"][0]) == flag_any

    # reset: the grouped reset against scalar resets per experiment and against the oracle's draws
    def reset(n, key, grouped, counter=4):
        x, pa = torch.full((n, L, 4), 7.0, **f32), torch.full((n, L), 7.0, **f32)
        if grouped:
            call("avd_env_reset_seeds_f32", ptr(cst), n, L, ptr(x), ptr(pa), None, 0, ptr(d_seeds), E, counter, None, stream_handle())
        else:
            call("avd_env_reset_f32", ptr(cst), n, L, ptr(x), ptr(pa), None, None, None, 0, key, counter, None, stream_handle())
        return x, pa

    gx, gpa = reset(P, None, True)
    for e, k in enumerate(SEEDS3):
        rx, rpa = reset(Pe, k, False)
        _eq(_deint(gx, E, e), rx, f"reset x e={e}")
        _eq(_deint(gpa, E, e), rpa, f"reset prev_a e={e}")
        v = np.arange(Pe * L)
        ra, rb = ophilox.philox_at(k, 4, v, ophilox.STREAM_RESET_A), ophilox.philox_at(k, 4, v, ophilox.STREAM_RESET_B)
        h = env.h_consts
        if uniform:
            d0 = ophilox.uniform_pm1(ra[0]) * np.float32(h.reset_ep_max)
            d2 = ophilox.uniform_pm1(rb[0]) * np.float32(h.reset_max_a)
            tol = 0.0
        else:
            d0 = ophilox.box_muller(ra[0], ra[1])[0] * np.float32(h.reset_ep_max)
            d2 = ophilox.box_muller(rb[0], rb[1])[0] * np.float32(h.reset_max_a)
            tol = 2e-6 * max(1.0, float(h.reset_ep_max), float(h.reset_max_a)) * 4
        gxe = _deint(gx, E, e).cpu().numpy().reshape(-1, 4)
        assert np.abs(gxe[:, 0] - d0).max() <= tol and np.abs(gxe[:, 2] - d2).max() <= tol

    # episode end: random closes
    M = L
    done = (torch.rand(P, generator=g, device="cuda") < 0.4).to(torch.uint8)
    ep_len = torch.randint(0, 30, (P,), generator=g, device="cuda", dtype=torch.int32)
    x0, pa0, er0 = 0.3 * rn(P, L, 4), 0.1 * rn(P, L), rn(P, M)

    def ep_end(sel, n, key, grouped):
        x, pa, er, ln = x0[sel].clone(), pa0[sel].clone(), er0[sel].clone(), ep_len[sel].clone()
        rs, ls, cnt = torch.zeros(n, **f32), torch.zeros(n, **f32), torch.zeros(n, dtype=torch.int32, device="cuda")
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        if grouped:
            call("avd_episode_end_seeds_f32", ptr(cst), n, L, M, ptr(x), ptr(pa), None, ptr(done[sel].contiguous()), ptr(ln), ptr(er), 25,
                 ptr(rs), ptr(ls), ptr(cnt), ptr(flag), 0, ptr(d_seeds), E, 6, stream_handle())
        else:
            call("avd_episode_end_f32", ptr(cst), n, L, M, ptr(x), ptr(pa), None, ptr(done[sel].contiguous()), ptr(ln), ptr(er), 25,
                 ptr(rs), ptr(ls), ptr(cnt), ptr(flag), 0, key, 6, stream_handle())
        return dict(x=x, pa=pa, er=er, ln=ln, rs=rs, ls=ls, cnt=cnt)

    allp = torch.arange(P, device="cuda")
    got = ep_end(allp, P, None, True)
    for e, k in enumerate(SEEDS3):
        ref = ep_end(allp.view(Pe, E)[:, e].contiguous(), Pe, k, False)
        for n in ref:
            _eq(_deint(got[n], E, e), ref[n], f"episode_end {n} e={e}")

    # replay sample: agents (p*E + e)*M + m, B = 64
    B, cap, rng_range = 64, 50, 37
    ring = rn(P * M, cap, 2 * S + 2)

    def sample(rg, n, key, grouped):
        o = [torch.empty(n, B, dtype=torch.int32, device="cuda"), torch.empty(n, B, S, **f32), torch.empty(n, B, 1, **f32),
             torch.empty(n, B, **f32), torch.empty(n, B, S, **f32)]
        if grouped:
            call("avd_replay_sample_seeds_f32", n, cap, S, 1, B, ptr(rg), rng_range, ptr(d_seeds), E, M, 3, *map(ptr, o), stream_handle())
        else:
            call("avd_replay_sample_f32", n, cap, S, 1, B, ptr(rg), rng_range, key, 3, *map(ptr, o), stream_handle())
        return o

    got = sample(ring, P * M, None, True)
    for e, k in enumerate(SEEDS3):
        ref = sample(_deint(ring, E, e, M).contiguous(), Pe * M, k, False)
        for n, a, b in zip(("idx", "s", "a", "r", "s2"), got, ref):
            _eq(_deint(a, E, e, M), b, f"replay {n} e={e}")
        assert np.array_equal(ref[0].cpu().numpy(), ophilox.replay_indices(Pe * M, B, rng_range, k, 3))


@pytest.mark.parametrize("L", [3, 5])
def test_one_group_equals_the_scalar_entry_points(L):
    """n_groups = 1 with the same seed: every *_seeds_* entry point gives the scalar one's bits."""
    need_gpu()
    P, S, k = 9, 4, 2 ** 40 + 3
    conf = config.Config(pl_size=L, num_platoons=P)
    env = vec.VecPlatoon(P, L, conf, rng="device", seeds=[k])
    f32 = dict(dtype=torch.float32, device="cuda")
    g = _gen(5)
    x_in, act, ou0 = 0.3 * torch.randn(P, L, 4, generator=g, device="cuda"), torch.randn(P, L, generator=g, device="cuda"), \
        torch.zeros(P, L, **f32)
    outs = []
    for grouped in (False, True):
        x, pa, ou = torch.empty(P, L, 4, **f32), torch.zeros(P, L, **f32), ou0.clone()
        rew, act_o, ex = torch.empty(P, L, **f32), torch.empty(P, L, **f32), torch.empty(P, **f32)
        done, flag = torch.empty(P, dtype=torch.uint8, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
        key = (ptr(env.d_seeds), 1) if grouped else (k,)
        call("avd_step_fused_seeds_f32" if grouped else "avd_step_fused_f32", ptr(env.d_consts), P, L, S, ptr(x_in), ptr(x), ptr(pa), None,
             ptr(rew), None, ptr(done), ptr(flag[0:1]), None, ptr(act), ptr(ou), ptr(act_o), ptr(ex), conf.theta, 0.0, conf.ou_dt,
             conf.std_dev, -2.5, 2.5, conf.reset_max_u, 0, *key, 3, 4, None, 0, 0, None, stream_handle())
        rx, rpa = torch.empty(P, L, 4, **f32), torch.empty(P, L, **f32)
        if grouped:
            call("avd_env_reset_seeds_f32", ptr(env.d_consts), P, L, ptr(rx), ptr(rpa), None, 0, ptr(env.d_seeds), 1, 2, None,
                 stream_handle())
        else:
            call("avd_env_reset_f32", ptr(env.d_consts), P, L, ptr(rx), ptr(rpa), None, None, None, 0, k, 2, None, stream_handle())
        outs.append((x, pa, ou, rew, act_o, ex, done, rx, rpa))
    for i, (a, b) in enumerate(zip(*outs)):
        _eq(a, b, f"output {i}")


# ---- 2. / 3. whole runs against solo runs -------------------------------------------------------------------------------------
def _conf(fed_method, P, L, **kw):
    c = dict(pl_size=L, num_platoons=P, buffer_size=300, episode_sim_time=3.0, fed_method=fed_method)
    c.update(kw)
    return config.Config(**c)


def _run(vt, steps):
    vt.reset_episode()
    for _ in range(steps):
        vt.step()
    torch.cuda.synchronize()


def _compare_runs(batch, solos, shared, exact_weights=True):
    E, M = batch.E, batch.M
    ag = batch.agents
    for e, solo in enumerate(solos):
        sa = solo.agents
        if exact_weights:
            for n in ("theta", "theta_t", "stats", "stats_t", "m", "v", "step"):
                t = getattr(ag, n)
                mine = t.view(E, M, *t.shape[1:])[e] if shared else _deint(t, E, e, M)
                _eq(mine, getattr(sa, n), f"{n} e={e}")
        env, senv = batch.env, solo.env
        _eq(_deint(batch.replay.ring, E, e, M), solo.replay.ring, f"replay ring e={e}")
        for n in ("x", "prev_a", "ep_len", "done"):
            _eq(_deint(getattr(env, n), E, e), getattr(senv, n), f"env.{n} e={e}")
        _eq(_deint(batch.ou.state, E, e, M), solo.ou.state, f"ou e={e}")
        _eq(_deint(batch.ep_reward, E, e), solo.ep_reward, f"ep_reward e={e}")
        for n in ("ret_sum", "len_sum", "count"):
            _eq(_deint(env.ep_stats[n], E, e), senv.ep_stats[n], f"ep_stats.{n} e={e}")


def _stats_and_sims(batch, solos):
    per = batch.env.pop_episode_stats(per_experiment=True)
    sims = batch.run_simulations()
    for e, solo in enumerate(solos):
        r, ln, n = solo.env.pop_episode_stats()
        assert n > 0 and n == per[2][e]
        assert r == per[0][e] and ln == per[1][e]
        assert sims[e] == solo.run_simulations()


def test_nofrl_seed_batch_is_bitwise_its_solo_runs():
    """E = 4 x P = 8 x L = 3, 400 steps (episodes of 30 steps close; learning from step 65): every experiment's weights, Adam state,
    replay ring, env, episode sums and simulation scores equal VecTrainer(seed=k, init_seed=k) at P = 8."""
    need_gpu()
    seeds, P, L, steps = (3, 9, 2 ** 31 + 1, 40), 8, 3, 400
    batch = trainer.VecTrainer(_conf("normal", P, L), rng="device", auto_reset="platoon", fused_update=True, seeds=seeds)
    _run(batch, steps)
    solos = []
    for k in seeds:
        s = trainer.VecTrainer(_conf("normal", P, L), rng="device", auto_reset="platoon", fused_update=True, seed=k, init_seed=k)
        _run(s, steps)
        solos.append(s)
    assert batch.replay.samples == steps - 64 and batch.E == 4 and batch.P == 32
    _compare_runs(batch, solos, shared=False)
    _stats_and_sims(batch, solos)


@pytest.mark.parametrize("weighted", [False, True])
def test_interfrl_per_agent_seed_batch_is_bitwise_its_solo_runs(weighted):
    """The per_agent engine sums each set over the platoons in a fixed order: its federated view [P, E*M] sums exactly one
    experiment's platoons, in the solo order -- bitwise end to end, unweighted and with device weights."""
    need_gpu()
    seeds, P, L, steps = (2, 7, 1001), 8, 3, 240
    kw = dict(weighted_average_enabled=weighted, weighted_window=2)
    batch = trainer.VecTrainer(_conf("interfrl", P, L, **kw), rng="device", auto_reset="platoon", seeds=seeds)
    assert batch.shared and batch.shared_engine == "per_agent" and batch.agents.n_sets == 3 * L
    _run(batch, steps)
    solos = []
    for k in seeds:
        s = trainer.VecTrainer(_conf("interfrl", P, L, **kw), rng="device", auto_reset="platoon", seed=k, init_seed=k)
        _run(s, steps)
        solos.append(s)
    _compare_runs(batch, solos, shared=True)
    if weighted:
        _eq(batch._wsum.view(3, L)[1], solos[1]._wsum, "weight sums")
    _stats_and_sims(batch, solos)


@pytest.mark.parametrize("engine", ["fused3", "batched"])
def test_set_learner_seed_batch(engine):
    """(a) one learn call on E = 3, P = 64, L = 5 against E solo calls on the same inputs, within the engine's tolerance (the set
    learners' reduction tree depends on the set count); (b) up to the first learn step, env, noise and replay bitwise equal to the
    solo runs; (c) avd_fed_weights_f32 on [P, E*M] bitwise equal to per-experiment [P, M] calls."""
    need_gpu()
    E, P, L = 3, 64, 5
    conf = config.Config(pl_size=L, num_platoons=P, fed_method="interfrl")
    wseeds = (5, 17, 2 ** 31 + 3)  # (initial weights: np.random.RandomState takes seeds below 2**32)
    big = vec.AgentGroup(E * L, 4, 1, conf, seeds=wseeds, seed_block=L)
    g = _gen(3)
    rn = lambda *sh: torch.randn(*sh, generator=g, device="cuda")
    n = P * E * L
    s, a, r, s2 = 1.5 * rn(n, 64, 4), 2.0 * rn(n, 64, 1).clamp(-1.25, 1.25), -0.3 * rn(n, 64).abs(), 1.5 * rn(n, 64, 4)

    def learn(grp, s, a, r, s2, n_agents):
        if engine == "fused3":
            return grp.learn_set_split(s, a, r, s2, n_agents).clone()
        Ms = grp.n_sets
        sm = lambda x: x.view(n_agents // Ms, Ms, *x.shape[1:]).transpose(0, 1).reshape(Ms, -1, *x.shape[2:]).contiguous()
        return grp.learn_shared(sm(s), sm(a), sm(r), sm(s2), n_agents).clone()

    gb = learn(big, s, a, r, s2, n)
    tol = 2e-5 if engine == "fused3" else 2e-2
    for e, k in enumerate(wseeds):
        solo = vec.AgentGroup(L, 4, 1, conf, seed=k)
        _eq(big.theta.view(E, L, -1)[e], solo.theta, f"initial weights e={e}")
        sl = [_deint(x, E, e, L).contiguous() for x in (s, a, r, s2)]
        gs = learn(solo, *sl, P * L)
        mine = gb.view(E, L, -1)[e]
        scale = gs.abs().max().item()
        assert (mine - gs).abs().max().item() <= tol * scale, (e, (mine - gs).abs().max().item() / scale)

    # (b) the trainer, up to the first learn step
    seeds, Pt = (4, 8, 15), 8
    mk = lambda **kw: trainer.VecTrainer(config.Config(pl_size=L, num_platoons=Pt, fed_method="interfrl", buffer_size=200),
                                         rng="device", auto_reset="platoon", shared_engine=engine, **kw)
    batch = mk(seeds=seeds)
    _run(batch, 64)
    solos = []
    for k in seeds:
        so = mk(seed=k, init_seed=k)
        _run(so, 64)
        solos.append(so)
    assert batch.replay.samples == 0
    _compare_runs(batch, solos, shared=True)

    # (c) the device federated weights on the federated view
    W = 3
    ring = rn(Pt * E * L, W).abs() + 0.1
    cnt = torch.full((Pt * E,), W, dtype=torch.int32, device="cuda")
    f32 = dict(dtype=torch.float32, device="cuda")

    def weights(rg, Pv, Mv):
        w, aw, ws = torch.empty(Pv * Mv, **f32), torch.empty(Pv * Mv, **f32), torch.empty(Mv, **f32)
        call("avd_fed_weights_f32", Pv, Mv, W, ptr(rg), ptr(cnt), 1, ptr(w), ptr(aw), ptr(ws), stream_handle())
        return w, aw, ws

    wb, awb, wsb = weights(ring, Pt, E * L)
    for e in range(E):
        w, aw, ws = weights(_deint(ring, E, e, L).contiguous(), Pt, L)
        _eq(_deint(wb, E, e, L), w, "w")
        _eq(_deint(awb, E, e, L), aw, "agent weights")
        _eq(wsb.view(E, L)[e], ws, "weight sums")


# ---- 4. guard rails ---------------------------------------------------------------------------------------------------------
def test_rejected_batches_raise_before_any_launch(monkeypatch):
    need_gpu()
    calls = []
    real = _hip.call
    monkeypatch.setattr(trainer, "call", lambda name, *a: (calls.append(name), real(name, *a)))
    monkeypatch.setattr(vec, "call", lambda name, *a: (calls.append(name), real(name, *a)))
    ok = dict(rng="device", auto_reset="platoon", seeds=(1, 2))
    cases = [
        (dict(fed_method="normal"), dict(ok, rng="host"), "rng='device'"),
        (dict(fed_method="normal"), dict(ok, auto_reset=True), "per-platoon episodes"),
        (dict(fed_method="normal", framework="centralized", pl_size=1), ok, "decentralized"),
        (dict(fed_method="intrafrl"), ok, "intrafrl"),
        (dict(fed_method="interfrl", aggregation_method="weights"), ok, "gradient aggregation"),
        (dict(fed_method="normal"), dict(ok, fused_step=False), "fused step"),
        (dict(fed_method="normal"), dict(ok, seed=3), "mutually exclusive"),
        (dict(fed_method="normal"), dict(ok, seeds=(1, 1)), "duplicate"),
        (dict(fed_method="interfrl", pl_size=5), dict(ok, seeds=tuple(range(13)), shared_engine="fused3"), "at most 64"),
        (dict(fed_method="interfrl", pl_size=5), dict(ok, seeds=tuple(range(13)), shared_engine="fused"), "at most 64"),
    ]
    for ckw, tkw, msg in cases:
        conf = config.Config(num_platoons=2, **{"pl_size": 3, **ckw})
        with pytest.raises(ValueError, match=msg):
            trainer.VecTrainer(conf, **tkw)
    assert all(n == "avd_mlp_layout_init" for n in calls), calls
    # a batch's objects refuse the scalar draw paths
    conf = config.Config(num_platoons=2, pl_size=3)
    vt = trainer.VecTrainer(conf, rng="device", auto_reset="platoon", seeds=(1, 2))
    with pytest.raises(_hip.AvdError, match="seeds"):
        vt.ou()
    with pytest.raises(_hip.AvdError, match="seeds"):
        vt.replay.draw_indices()
    with pytest.raises(_hip.AvdError, match="not a multiple|n_groups"):
        call("avd_env_reset_seeds_f32", ptr(vt.env.d_consts), 5, 3, ptr(vt.env.x), ptr(vt.env.prev_a), None, 0, ptr(vt.env.d_seeds), 2,
             0, None, stream_handle())


# ---- 5. the CLI's directories -----------------------------------------------------------------------------------------------
def _cli(args, cwd):
    r = subprocess.run([sys.executable, "-m", "avddpg_amd", "tr", *args], cwd=ROOT, capture_output=True, text=True, timeout=600,
                       env={**os.environ, "PYTHONPATH": ROOT})
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout.strip().splitlines()[-1]


def test_cli_seeds_writes_one_directory_per_seed_equal_to_its_solo_run(tmp_path):
    need_gpu()
    common = ["--rng", "device", "--episodes", "platoon", "--pl_num", "3", "--pl_size", "3", "--total_time_steps", "150",
              "--buffer_size", "400", "--report_every", "50", "--eval_platoons", "all"]
    base = _cli(common + ["--seeds", "3-4", "--out", str(tmp_path / "batch")], tmp_path)
    solo = _cli(common + ["--seed", "4", "--out", str(tmp_path / "solo")], tmp_path)
    for k in (3, 4):
        d = os.path.join(base, f"seed{k}")
        assert os.path.exists(os.path.join(d, "curve.csv")) and os.path.exists(os.path.join(d, "actor1_1.npz"))
        cj = json.load(open(os.path.join(d, "conf.json")))
        assert cj["random_seed"] == k and cj["seed_batch"] == [3, 4] and len(cj["pl_rews_for_simulations"]) == 3
        # esim on the directory reproduces the experiment's final rollout score of platoon 1 (the last curve point)
        last = open(os.path.join(d, "curve.csv")).read().strip().splitlines()[-1].split(",")
        r = subprocess.run([sys.executable, "-m", "avddpg_amd", "esim", d, "--n_timesteps", str(cj["steps_per_episode"])], cwd=ROOT,
                           capture_output=True, text=True, timeout=600, env={**os.environ, "PYTHONPATH": ROOT})
        assert r.returncode == 0, r.stderr[-3000:]
        line = [x for x in r.stdout.splitlines() if x.startswith("platoon 1:")][0]
        assert np.float32(line.split()[-1]) == np.float32(last[4])  # (esim prints the float32 score, curve.csv with 3 decimals)
    # nofrl: experiment 4 of the batch is the solo `tr --seed 4`, curve and simulation scores alike
    assert open(os.path.join(base, "seed4", "curve.csv")).read() == open(os.path.join(solo, "curve.csv")).read()
    cs, cb = json.load(open(os.path.join(solo, "conf.json"))), json.load(open(os.path.join(base, "seed4", "conf.json")))
    assert cb["pl_rews_for_simulations"] == cs["pl_rews_for_simulations"]
    for f in os.listdir(solo):
        if f.endswith(".npz"):
            a, b = np.load(os.path.join(solo, f)), np.load(os.path.join(base, "seed4", f))
            assert all(np.array_equal(a[n], b[n]) for n in a.files), f
