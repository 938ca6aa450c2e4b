"""Training under disturbances on the GPU: avd_step_fused_dist_f32 / avd_observe_f32 (csrc/env.hip) against avd_step_fused_f32 with ==
wherever a level sits at its zero, against the other configuration's constants for the plant, against tests/train_disturb_oracle.py
for the link (exact) and the noise; then VecTrainer(train_disturb=...), the seed batch and the CLI.

Shapes (L, P), three levels each so that P % n_levels != 0: (5, 13) 12 platoons per wave -- a second wave with idle lanes; (1, 70);
(16, 5) 4 per wave; (3, 90) a second workgroup (84 platoons per block)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from avddpg_amd import _hip, config, scenarios, trainer, vec
from avddpg_amd._hip import call, ptr, stream_handle
from avddpg_amd.scenarios import Disturbance
from tests import train_disturb_oracle as tdo
from tests.gpu_util import need_gpu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 13), (1, 70), (16, 5), (3, 90)]
CAP, SLOT, OU_C, EXOG_C, SEED = 8, 3, 9, 13, 21
TRUE_OUT = ("x", "pa", "cum", "rew", "term", "done", "flag", "ou", "action", "exog", "er")  # what comes from the true state


def _eq(a, b, what):
    a, b = a.cpu(), b.cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype.is_floating_point:
        a, b = a.view(torch.int32), b.view(torch.int32)  # bitwise, NaN-safe
    assert torch.equal(a, b), f"{what}: {(a != b).sum().item()} of {a.numel()} differ"


def _differs(a, b):
    return not torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


def _inputs(P, L, S, seed=5):
    """A state well inside the terminal bounds (|ep|, |ev| < 20: no comparison hinges on a flag), random everything else."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *sh: torch.randn(*sh, generator=g, device="cuda")
    return dict(x=0.5 * rn(P, L, 4), pa=0.1 * rn(P, L), cum=rn(P, L), act=rn(P, L), ou=0.2 * rn(P, L), ring=rn(P * L, CAP, 2 * S + 2),
                er=rn(P, L), obs=0.5 * rn(P, L, 4))


class Tables:
    """The device tables of a level list, as VecPlatoon(train_disturb=...) makes them."""

    def __init__(self, levels, conf, L):
        self.levels = scenarios.check_disturbances(levels, conf)
        self.n = len(self.levels)
        self.h, self.d = vec.train_level_table(self.levels, "cuda")
        self.plant = torch.from_numpy(np.stack([scenarios.plant_table(conf, L, d.dyn_coeff) for d in self.levels])).cuda()


def _consts(conf, L):
    return vec.VecPlatoon(1, L, conf, rng="device").d_consts  # (device RNG: the constructor launches nothing)


def _step(conf, P, L, inp, tab=None, link=None, counter=1, key=(SEED,), cst=None, ring=True):
    """One launch of avd_step_fused_f32 (tab None) or avd_step_fused_dist_f32 from the state ``inp``; nothing of ``inp`` is written.
    link: (hist, recv) tensors, updated in place, or None (NULL pointers). key: (seed,) or (d_seeds, E)."""
    S = 3 if conf.model == conf.modelA else 4
    f32 = dict(dtype=torch.float32, device="cuda")
    cst = _consts(conf, L) if cst is None else cst
    o = dict(x=torch.empty(P, L, 4, **f32), pa=inp["pa"].clone(), cum=inp["cum"].clone(), rew=torch.empty(P, L, **f32),
             term=torch.empty(P, L, dtype=torch.uint8, device="cuda"), done=torch.empty(P, dtype=torch.uint8, device="cuda"),
             flag=torch.tensor([0, 7], dtype=torch.int32, device="cuda"), ou=inp["ou"].clone(), action=torch.empty(P, L, **f32),
             exog=torch.empty(P, **f32), ring=inp["ring"].clone(), er=inp["er"].clone(), obs=torch.full((P, L, 4), 9.0, **f32))
    grouped = len(key) == 2
    head = (ptr(cst), P, L, S, ptr(inp["x"]), ptr(o["x"]), ptr(o["pa"]), ptr(o["cum"]), ptr(o["rew"]), ptr(o["term"]), ptr(o["done"]),
            ptr(o["flag"][0:1]), ptr(o["flag"][1:2]), ptr(inp["act"]), ptr(o["ou"]), ptr(o["action"]), ptr(o["exog"]), conf.theta, 0.0,
            conf.ou_dt, conf.std_dev, conf.action_low, conf.action_high, conf.reset_max_u, 0, *key, OU_C, EXOG_C,
            ptr(o["ring"]) if ring else None, CAP, 1000 * CAP + SLOT, ptr(o["er"]))
    if tab is None:
        call("avd_step_fused_seeds_f32" if grouped else "avd_step_fused_f32", *head, stream_handle())
    else:
        hist, recv = link if link is not None else (None, None)
        call("avd_step_fused_dist_seeds_f32" if grouped else "avd_step_fused_dist_f32", *head, tab.n, tab.h, ptr(tab.d), ptr(tab.plant),
             ptr(inp["obs"]), ptr(o["obs"]), ptr(hist), ptr(recv), counter, stream_handle())
    return o


def _observe(P, L, x, obs, tab, link=None, counter=0, key=(SEED,), only_where_zero=None, run_if_nonzero=None):
    hist, recv = link if link is not None else (None, None)
    call("avd_observe_seeds_f32" if len(key) == 2 else "avd_observe_f32", P, L, ptr(x), ptr(obs), tab.n, ptr(tab.d), ptr(hist), ptr(recv),
         *key, counter, ptr(only_where_zero), ptr(run_if_nonzero), stream_handle())


def _new_link(P, L, fill=-3.0):
    return torch.full((P, L, 16), fill, device="cuda"), torch.full((P, L), fill, device="cuda")


# ---- 1. null levels are today's launch ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["ModelB", "ModelA"])
@pytest.mark.parametrize("L,P", SHAPES)
def test_null_levels_are_the_nominal_launch_bit_for_bit(L, P, model):
    need_gpu()
    conf = config.Config(pl_size=L, model=model)
    S = 3 if model == "ModelA" else 4
    inp = _inputs(P, L, S)
    inp["obs"] = inp["x"].clone()  # what a null level observes of x_in
    ref = _step(conf, P, L, inp)
    null3 = [Disturbance("a"), Disturbance("b"), Disturbance("c")]
    same_plant = [Disturbance(n, dyn_coeff=conf.dyn_coeff) for n in "abc"]
    for what, levels in (("null", null3), ("explicit dyn_coeff", same_plant)):
        got = _step(conf, P, L, inp, Tables(levels, conf, L))
        for n in TRUE_OUT + ("ring",):
            _eq(got[n], ref[n], (what, n))
        _eq(got["obs"], got["x"], (what, "obs_out has x_out's bits"))
    assert int(ref["flag"][1]) == 0 and int(ref["flag"][0]) == 0  # (the other flag cleared; no terminal state in these inputs)
    # with a link buffer present, null levels leave it alone
    link = _new_link(P, L)
    got = _step(conf, P, L, inp, Tables(null3, conf, L), link=link)
    _eq(got["obs"], ref["x"], "obs with an unused link")
    assert bool((link[0] == -3.0).all()) and bool((link[1] == -3.0).all())
    # the observe kernel under null levels copies x
    obs = torch.full((P, L, 4), 9.0, device="cuda")
    _observe(P, L, inp["x"], obs, Tables(null3, conf, L))
    _eq(obs, inp["x"], "observe, null levels")


# ---- 2. a plant level is the other configuration ---------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["ModelB", "ModelA"])
@pytest.mark.parametrize("L,P", SHAPES)
def test_plant_level_equals_the_other_configuration(L, P, model):
    need_gpu()
    conf = config.Config(pl_size=L, model=model)
    assert conf.dyn_coeff != 0.15
    S = 3 if model == "ModelA" else 4
    inp = _inputs(P, L, S, seed=6)
    inp["obs"] = inp["x"].clone()  # (no level here changes the observation)
    other = lambda tau: _step(config.Config(pl_size=L, model=model, dyn_coeff=tau), P, L, inp)
    ref = other(0.15)
    got = _step(conf, P, L, inp, Tables([Disturbance(n, dyn_coeff=0.15) for n in "abc"], conf, L))
    assert _differs(ref["x"], _step(conf, P, L, inp)["x"])
    for n in TRUE_OUT + ("ring",):
        _eq(got[n], ref[n], n)
    _eq(got["obs"], ref["x"], "obs")
    # mixed: each platoon matches the run of its own level
    taus = [None, 0.15, 0.25]
    got = _step(conf, P, L, inp, Tables([Disturbance(n, dyn_coeff=t) for n, t in zip("abc", taus)], conf, L))
    flag = 0
    for k, tau in enumerate(taus):
        ref = other(conf.dyn_coeff if tau is None else tau)
        sel = torch.arange(k, P, 3, device="cuda")
        for n in TRUE_OUT:
            if n != "flag":
                _eq(got[n][sel], ref[n][sel], (n, k))
        _eq(got["ring"].view(P, L, CAP, -1)[sel], ref["ring"].view(P, L, CAP, -1)[sel], ("ring", k))
        flag |= int(ref["done"][sel].any())
    assert int(got["flag"][0]) == flag


# ---- 3. the link, exact -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", [0, 1, 2])
@pytest.mark.parametrize("L,P", SHAPES)
def test_link_delay_loss_and_the_fresh_link_after_a_gated_observe(L, P, rot):
    """20 steps under (delay 3 | always dropped | delay 1, loss 0.4), the level list rotated by ``rot`` so that at every shape each level
    also sits on the platoons of the second wave / second workgroup ((5, 13): platoon 12; (16, 5): platoon 4; (1, 70): 64..69; (3, 90):
    84..89). Every vehicle's observed w against the recorded true w / the helper's integer compare, bit for bit."""
    need_gpu()
    T = 20
    conf = config.Config(pl_size=L)
    base = [Disturbance("lag", v2v_delay=3), Disturbance("dead", v2v_drop=1), Disturbance("lossy", v2v_delay=1, v2v_drop=0.4)]
    tab = Tables(base[rot:] + base[:rot], conf, L)
    kind = np.array([(tdo.level_of(p, 3) + rot) % 3 for p in range(P)])  # 0 lag, 1 dead, 2 lossy
    lag, dead = kind == 0, kind == 1
    lossy = np.where(kind == 2)[0]
    assert lag.any() and dead.any() and len(lossy) and {int(kind[P - 1]) for _ in [0]} <= {0, 1, 2}
    inp = _inputs(P, L, 4, seed=7)
    link = _new_link(P, L)
    obs0 = torch.full((P, L, 4), 9.0, device="cuda")
    _observe(P, L, inp["x"], obs0, tab, link=link, counter=0)
    _eq(obs0, inp["x"], "fresh observation (no noise level)")
    _eq(link[0], inp["x"][..., 3:4].expand(P, L, 16).contiguous(), "fresh ring")
    _eq(link[1], inp["x"][..., 3].contiguous(), "fresh held value")
    w = [inp["x"][..., 3].cpu().numpy().copy()]  # w[c]: the true x.w of the state observed with counter c
    index = (lossy[:, None] * L + np.arange(L)[None]).reshape(-1)  # the Philox index: the vehicle p * L + i
    model = tdo.Link(w[0][lossy].reshape(-1), 1, scenarios.drop_threshold(0.4), SEED, index)
    held = updated = 0
    bits = lambda a: np.ascontiguousarray(a).view(np.int32)
    for t in range(T):
        out = _step(conf, P, L, inp, tab, link=link, counter=t + 1, ring=False)
        w.append(out["x"][..., 3].cpu().numpy().copy())
        ow = out["obs"][..., 3].cpu().numpy()
        assert np.array_equal(bits(out["obs"][..., :3].cpu().numpy()), bits(out["x"][..., :3].cpu().numpy()))
        assert np.array_equal(bits(ow[lag]), bits(w[max(t + 1 - 3, 0)][lag])), ("delay 3", t)
        assert np.array_equal(bits(ow[dead]), bits(w[0][dead])), ("drop 1", t)
        want, lost = model.push(w[t + 1][lossy].reshape(-1), t + 1)
        assert np.array_equal(bits(ow[lossy].reshape(-1)), bits(want)), ("drop 0.4", t)
        held, updated = held + int(lost.sum()), updated + int((~lost).sum())
        inp = dict(inp, x=out["x"], pa=out["pa"], ou=out["ou"], obs=out["obs"], cum=out["cum"], er=out["er"])
    n = len(index) * T  # (P(held) = 0.4: at the smallest count, 320 samples, 0.25 n and 0.45 n lie 5.5 standard deviations out)
    assert n >= 320 and held > 0.25 * n and updated > 0.45 * n
    _eq(link[1][torch.from_numpy(lossy).cuda()].reshape(-1), torch.from_numpy(model.recv), "held value")
    # the ring itself: a lagged vehicle's 16 slots hold the true w of the last 16 counters, each at counter & 15
    ring_want = np.stack([w[c] for c in range(T - 15, T + 1)], axis=-1)[..., np.argsort([c & 15 for c in range(T - 15, T + 1)])]
    assert np.array_equal(bits(link[0].cpu().numpy()[lag]), bits(ring_want[lag])), "ring slots"
    # a gated observe refills exactly the masked platoons
    # (from a state whose w is the last one's + 1: at L = 1 the leader's w does not move, a refill with it would show nothing)
    x2 = inp["x"].clone()
    x2[..., 3] += 1.0
    before = (link[0].clone(), link[1].clone(), inp["obs"].clone())
    ep_len = torch.tensor([0 if p in (1, P // 2, P - 1) else 4 for p in range(P)], dtype=torch.int32, device="cuda")
    obs = inp["obs"].clone()
    zero, one = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.ones(1, dtype=torch.int32, device="cuda")
    _observe(P, L, x2, obs, tab, link=link, counter=T, only_where_zero=ep_len, run_if_nonzero=zero)
    for got, ref, nm in zip((link[0], link[1], obs), before, ("ring", "held", "obs")):
        _eq(got, ref, ("run_if_nonzero reads 0: nothing changes", nm))
    _observe(P, L, x2, obs, tab, link=link, counter=T, only_where_zero=ep_len, run_if_nonzero=one)
    m = ep_len.cpu() == 0
    _eq(link[0][m], x2[m][..., 3:4].expand(-1, L, 16).contiguous(), "refilled ring")
    _eq(link[1][m], x2[m][..., 3].contiguous(), "refilled held value")
    _eq(obs[m], x2[m], "fresh observation")
    for got, ref, nm in zip((link[0], link[1], obs), before, ("ring", "held", "obs")):
        _eq(got[~m], ref[~m], ("unmasked platoons unchanged", nm))
    assert _differs(link[0][m], before[0][m])


# ---- 4. the noise -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["ModelB", "ModelA"])
@pytest.mark.parametrize("L,P", SHAPES)
def test_sensor_noise_against_the_philox_restatement(L, P, model):
    """obs - x against sigma * n of tests/train_disturb_oracle.py at the state tolerance tests/scenario_oracle.check_against holds the
    disturbed evaluator to against tests/disturbed_oracle.py (atol 2e-4, rtol 1e-4), for the step's obs_out and the observe kernel."""
    need_gpu()
    conf = config.Config(pl_size=L, model=model)
    S = 3 if model == "ModelA" else 4
    sig = [(0.05, 0.05, 0.02), (0.0, 0.3, 0.0), (0.0, 0.0, 0.0)]
    tab = Tables([Disturbance(n, noise_ep=s[0], noise_ev=s[1], noise_a=s[2]) for n, s in zip("abc", sig)], conf, L)
    inp = _inputs(P, L, S, seed=8)
    a, b, c = (_step(conf, P, L, inp, tab, counter=k) for k in (4, 4, 5))
    nominal = _step(conf, P, L, inp)
    for n in TRUE_OUT:
        _eq(a[n], nominal[n], ("the true state ignores the noise", n))
    _eq(a["obs"], b["obs"], "same (seed, counter): same bits")
    sigma = np.array([sig[tdo.level_of(p, 3)] for p in range(P)], dtype=np.float64)[:, None, :].repeat(L, axis=1)  # [P, L, 3]
    noisy = torch.from_numpy(sigma != 0)
    assert _differs(a["obs"].cpu()[..., :3][noisy], c["obs"].cpu()[..., :3][noisy])
    obs_k = torch.full((P, L, 4), 9.0, device="cuda")
    _observe(P, L, a["x"], obs_k, tab, counter=4)
    _eq(obs_k, a["obs"], "the observe kernel makes the step's observation of the same state")
    x, ob = a["x"].cpu(), a["obs"].cpu()
    _eq(ob[..., 3], x[..., 3], "component 3 without a link level")
    _eq(ob[..., :3][~noisy], x[..., :3][~noisy], "sigma == 0 keeps x's bits")
    assert bool((ob[..., :3][noisy] != x[..., :3][noisy]).all())
    want = sigma * tdo.normals(SEED, 4, np.arange(P * L)).reshape(P, L, 3)
    got = ob[..., :3].numpy().astype(np.float64) - x[..., :3].numpy().astype(np.float64)
    print("max |(obs - x) - sigma n|", np.max(np.abs(got - want)))
    assert np.allclose(got, want, atol=2e-4, rtol=1e-4)
    # Beside the issue's bound, one from the number formats: the float32 add rounds by at most half an ulp of the result (2^-24 |obs|);
    # the float32 product by 2^-24 |sigma n|, and sigma itself is rounded to float32 (another 2^-24); n differs from numpy's float32
    # Box-Muller by the device's logf / sqrtf / sinf / cosf, a few ulp each: 16 ulp (2^-23 each) of max(|n|, 1) allowed.
    n64 = np.abs(tdo.normals(SEED, 4, np.arange(P * L)).reshape(P, L, 3))
    tight = 2.0 ** -24 * np.abs(ob[..., :3].numpy().astype(np.float64)) + sigma * (2.0 ** -23 * np.abs(n64) + 16 * 2.0 ** -23 * np.maximum(n64, 1.0))
    ratio = np.abs(got - want)[sigma != 0] / tight[sigma != 0]
    print("worst deviation over the format bound", ratio.max())
    assert ratio.max() <= 1.0
    # a seed batch draws with (seeds[e], the counter, the vehicle index of the solo run), under the solo run's level
    E = 2 if P % 2 == 0 else (5 if P % 5 == 0 else 13)
    seeds, d_seeds = vec.seed_table(range(40, 40 + E), "cuda")
    g = _step(conf, P, L, inp, tab, counter=4, key=(ptr(d_seeds), E))
    for e, k in enumerate(seeds):
        sub = {n: t.view(P // E, E, *t.shape[1:])[:, e].contiguous() for n, t in inp.items() if n != "ring"}
        sub["ring"] = inp["ring"].view(P // E, E, L, CAP, -1)[:, e].reshape(-1, CAP, 2 * S + 2).contiguous()
        solo = _step(conf, P // E, L, sub, tab, counter=4, key=(k,))
        for n in ("x", "obs", "ou", "rew", "exog"):
            _eq(g[n].view(P // E, E, *g[n].shape[1:])[:, e], solo[n], ("seed batch", n, e))
        _eq(g["ring"].view(P // E, E, L, CAP, -1)[:, e].reshape(-1, CAP, 2 * S + 2), solo["ring"], ("seed batch ring", e))


# ---- 5. the replay holds observations ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,P", SHAPES)
def test_replay_row_holds_what_the_agent_saw(L, P):
    need_gpu()
    conf = config.Config(pl_size=L)
    S = 4
    tab = Tables([Disturbance(n, noise_ep=0.1, noise_ev=0.1, noise_a=0.05, v2v_delay=2) for n in "abc"], conf, L)
    inp = _inputs(P, L, S, seed=9)
    # every ring slot its own value, 1000 v + slot: the slot a vehicle reads is identifiable
    fill = (1000.0 * torch.arange(P * L, device="cuda").view(P, L, 1) + torch.arange(16, device="cuda").view(1, 1, 16)).float()
    link = (fill.clone(), torch.full((P, L), -3.0, device="cuda"))
    counter, delay = 19, 2
    got, ref = _step(conf, P, L, inp, tab, link=link, counter=counter), _step(conf, P, L, inp)
    row, nom = got["ring"][:, SLOT], ref["ring"][:, SLOT]
    _eq(row[:, :S], inp["obs"].view(-1, 4)[:, :S], "s is obs_in")
    _eq(row[:, S + 2:], got["obs"].view(-1, 4)[:, :S], "s' is obs_out")
    _eq(row[:, S:S + 2], nom[:, S:S + 2], "u and -r are the nominal launch's")
    _eq(got["x"], ref["x"], "the true state")
    assert bool((row[:, :S] != inp["x"].view(-1, 4)[:, :S]).any(dim=1).all()) and bool((row[:, S + 2:] != got["x"].view(-1, 4)).any(dim=1).all())
    _eq(got["obs"][..., 3], fill[..., (counter - delay) & 15].contiguous(), "the lagged component is the vehicle's own slot (c - delay) & 15")
    _eq(link[1], got["obs"][..., 3].contiguous(), "the held value")
    want = fill.clone()
    want[..., counter & 15] = got["x"][..., 3]
    _eq(link[0], want, "one slot written: the vehicle's own, counter & 15")
    other = torch.ones(CAP, dtype=torch.bool)
    other[SLOT] = False
    _eq(got["ring"][:, other], inp["ring"][:, other], "the other slots")


# ---- 6. the trainer ---------------------------------------------------------------------------------------------------------
def _conf(**kw):
    return config.Config(num_platoons=6, pl_size=3, episode_sim_time=0.8, buffer_size=256, **kw)


REGIMES = {"nofrl per_agent": (dict(), dict()), "nofrl fused_update": (dict(), dict(fused_update=True)),
           "interfrl fused3": (dict(fed_method="interfrl"), dict(shared_engine="fused3"))}


def _train(conf_kw, kw, auto_reset, levels, steps=80, **more):
    conf = _conf(**conf_kw)
    assert conf.steps_per_episode == 8
    vt = trainer.VecTrainer(conf, rng="device", auto_reset=auto_reset, train_disturb=levels, **kw, **more)
    if auto_reset is False:
        vt.run(number_of_episodes=steps // conf.steps_per_episode)  # the host episode loop (reset_episode per episode)
    else:
        vt.reset_episode()
        for _ in range(steps):
            vt.step()
    torch.cuda.synchronize()
    return vt


def _state(vt):
    ag = vt.agents
    out = dict(theta=ag.theta, theta_t=ag.theta_t, stats=ag.stats, stats_t=ag.stats_t, m=ag.m, v=ag.v, adam_step=ag.step, ring=vt.replay.ring,
               x=vt.env.x, ep_reward=vt.ep_reward, ou=vt.ou.state)
    if vt.env.ep_stats is not None:
        out.update({"ep_" + k: t for k, t in vt.env.ep_stats.items()})
    return out


@pytest.mark.parametrize("auto_reset", ["platoon", True, False])
@pytest.mark.parametrize("regime", list(REGIMES))
def test_trainer_with_null_levels_is_the_plain_trainer_bit_for_bit(regime, auto_reset):
    """80 steps of 8-step episodes: every reset path re-observes (a platoon left with a stale observation would act from, and store, its
    pre-reset state) and the disturbed launch chain under null levels computes what the plain one does. It does NOT show which buffer a
    consumer reads -- obs equals x here; test_actors_act_from_the_observation does."""
    need_gpu()
    conf_kw, kw = REGIMES[regime]
    plain = _state(_train(conf_kw, kw, auto_reset, None))
    vt = _train(conf_kw, kw, auto_reset, [Disturbance("a"), Disturbance("b")])
    assert vt.env.link_hist is None and vt.env.obs_counter == 80 and vt.replay.buffer_counter == 80
    got = _state(vt)
    assert int(got["adam_step"].min()) >= 80 - 65
    for n, t in plain.items():
        _eq(got[n], t, (regime, auto_reset, n))
    _eq(vt.env.obs, vt.env.x, "obs")
    if auto_reset == "platoon":
        assert int(vt.env.ep_stats["count"].sum()) >= 6 * 9


def _actor_of(vt, states):
    """The actors' outputs on ``states`` [P, L, 4] by the kernel the trainer's plain path takes for this regime."""
    st = states.view(vt.P * vt.M, vt.x_stride)
    if vt.act_mfma:
        return vt.agents.actor_set(st, vt.P * vt.M, x_stride=vt.x_stride)
    return vt.agents.actor(st, vt.set_mod, x_stride=vt.x_stride).view(-1)


NOISY = lambda: [Disturbance("rough", noise_ep=0.2, noise_ev=0.2, noise_a=0.1, v2v_delay=2)]


@pytest.mark.parametrize("regime", list(REGIMES))
def test_actors_act_from_the_observation(regime):
    """Every platoon under a noisy, lagged level. Plain _act path, before the replay gate opens (no update: the weights are those the
    step acted with): after a step, actor_out is actor(the observation the step acted from) and not actor(the true state); the same
    right after the all-platoons reset at the episode's step limit, which re-observed the fresh states."""
    need_gpu()
    conf_kw, kw = REGIMES[regime]
    vt = trainer.VecTrainer(_conf(**conf_kw), rng="device", auto_reset=True, train_disturb=NOISY(), **kw)
    vt.reset_episode()
    for k in range(1, 9):
        vt.step()
        if k in (1, 5):
            assert not vt._act_ready
            _eq(vt.actor_out.view(-1), _actor_of(vt, vt.env.obs_prev), ("acted from o_t", k))
            assert _differs(vt.actor_out.view(-1), _actor_of(vt, vt.env.x_prev))
    assert vt.ep_step == 0 and vt.episode == 1  # the 8th step closed the episode: fresh states, re-observed
    fresh_x, fresh_obs = vt.env.x.clone(), vt.env.obs.clone()
    assert _differs(fresh_obs[..., :3], fresh_x[..., :3])
    _eq(fresh_obs[..., 3], fresh_x[..., 3], "a fresh link holds the start value")
    vt._act()
    _eq(vt.env.obs_prev, fresh_obs, "the buffers swapped")
    _eq(vt.actor_out.view(-1), _actor_of(vt, fresh_obs), "acted from the fresh observation")
    assert _differs(vt.actor_out.view(-1), _actor_of(vt, fresh_x))


def test_fused_update_epilogue_and_its_gated_recompute_read_the_observation():
    """nofrl fused_update, per-platoon episodes of 8 steps. Step 67 (no episode closes): the update's next-action epilogue left
    actor(updated weights, env.obs) in actor_out, not actor(env.x). Step 72 closes every platoon's episode: the next _act recomputes,
    gated on the flag, from the re-observed fresh states."""
    need_gpu()
    vt = trainer.VecTrainer(_conf(), rng="device", auto_reset="platoon", train_disturb=NOISY(), fused_update=True)
    vt.reset_episode()
    for _ in range(67):
        vt.step()
    assert vt._act_ready and vt.updates > 0 and int(vt.env.ep_len.min()) == 67 % 8
    _eq(vt.actor_out.view(-1), _actor_of(vt, vt.env.obs), "the epilogue read o_{t+1}")
    assert _differs(vt.actor_out.view(-1), _actor_of(vt, vt.env.x))
    for _ in range(5):
        vt.step()
    assert vt._act_ready and int(vt.env.ep_len.max()) == 0 and int(vt.env.any_done) != 0  # all reset, flag set
    stale, fresh_x, fresh_obs = vt.actor_out.clone(), vt.env.x.clone(), vt.env.obs.clone()
    assert _differs(stale.view(-1), _actor_of(vt, fresh_obs))
    vt._act()
    _eq(vt.actor_out.view(-1), _actor_of(vt, fresh_obs), "the gated recompute read the fresh observation")
    assert _differs(vt.actor_out.view(-1), _actor_of(vt, fresh_x)) and _differs(vt.actor_out, stale)


@pytest.mark.parametrize("regime", list(REGIMES))
def test_trainer_with_a_real_level_trains_on_other_data_and_stays_finite(regime):
    need_gpu()
    conf_kw, kw = REGIMES[regime]
    plain = _state(_train(conf_kw, kw, "platoon", None))
    levels = [Disturbance("clean"), Disturbance("rough", noise_ep=0.1, noise_ev=0.1, v2v_delay=2, v2v_drop=0.2, dyn_coeff=0.15)]
    vt = _train(conf_kw, kw, "platoon", levels)
    got = _state(vt)
    assert vt.env.link_hist is not None
    assert _differs(got["theta"], plain["theta"]) and _differs(got["ring"], plain["ring"])
    for n in ("theta", "theta_t", "m", "v", "ring", "x"):
        assert bool(torch.isfinite(got[n]).all()), n
    assert _differs(vt.env.obs, vt.env.x)
    # the clean share of platoons (even ones) observes the truth
    _eq(vt.env.obs[0::2], vt.env.x[0::2], "clean platoons")


# ---- 7. the seed batch ------------------------------------------------------------------------------------------------------
def test_seed_batch_experiment_is_its_solo_run_bit_for_bit():
    need_gpu()
    levels = lambda: [Disturbance("clean"), Disturbance("rough", noise_ep=0.1, noise_a=0.05, v2v_delay=2, v2v_drop=0.2, dyn_coeff=0.15),
                      Disturbance("lag", v2v_delay=5)]
    seeds = [3, 4]
    batch = _train({}, {}, "platoon", levels(), seeds=seeds)
    E, M, P = 2, 3, 6
    for e, k in enumerate(seeds):
        solo = _train({}, {}, "platoon", levels(), seed=k, init_seed=k)
        per_agent = lambda t: t.view(P, E, M, *t.shape[1:])[:, e].reshape(P * M, *t.shape[1:])
        per_platoon = lambda t: t.view(P, E, *t.shape[1:])[:, e]
        ag, sg = batch.agents, solo.agents
        for n in ("theta", "theta_t", "stats", "stats_t", "m", "v", "step"):
            _eq(per_agent(getattr(ag, n)), getattr(sg, n), (n, e))
        _eq(per_agent(batch.replay.ring), solo.replay.ring, ("ring", e))
        for n in ("x", "obs", "link_hist", "link_recv"):
            _eq(per_platoon(getattr(batch.env, n)), getattr(solo.env, n), (n, e))
        for n, t in batch.env.ep_stats.items():
            _eq(per_platoon(t), solo.env.ep_stats[n], ("ep_stats", n, e))
    assert _differs(batch.env.obs, batch.env.x)


# ---- 8. the CLI -------------------------------------------------------------------------------------------------------------
def _run(*argv):
    out = subprocess.run([sys.executable, "-m", "avddpg_amd", *argv], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout.strip().splitlines()[-1]


def _files(d):
    """The run's files but conf.json: the CSVs as bytes, the checkpoints as their arrays' bytes (an .npz carries its write time)."""
    out = {}
    for f in sorted(os.listdir(d)):
        if f.endswith(".npz"):
            z = np.load(os.path.join(d, f))
            out[f] = [z[k].tobytes() for k in z.files]
        elif f != "conf.json":
            out[f] = open(os.path.join(d, f), "rb").read()
    return out


def test_cli_trains_under_levels_and_without_the_flag_nothing_changes(tmp_path):
    """`tr ... --train_disturb clean --train_disturb rough:... --scenarios step --disturb lag:...` records the levels and writes
    robustness.csv. Without the flag the run takes the entry points it always took and conf.json has no train_disturbances; its every
    other file is byte-identical to the run under one null level, which the trainer tests above tie to the plain trainer bit for bit."""
    need_gpu()
    tr = ("tr", "--pl_num", "3", "--pl_size", "2", "--buffer_size", "500", "--total_time_steps", "70", "--rng", "device", "--episodes", "platoon",
          "--report_every", "70", "--scenarios", "step", "--disturb", "lag:v2v_delay=2")
    plain = _run(*tr, "--out", str(tmp_path / "plain"))
    null = _run(*tr, "--train_disturb", "clean", "--out", str(tmp_path / "null"))
    base = _run(*tr, "--train_disturb", "clean", "--train_disturb", "rough:noise_ep=0.1,v2v_delay=2", "--out", str(tmp_path / "with"))
    conf = json.load(open(os.path.join(base, "conf.json")))
    assert conf["train_disturbances"] == [["clean", Disturbance("clean").items()], ["rough", Disturbance("rough", noise_ep=0.1, v2v_delay=2).items()]]
    assert conf["robustness_suite"] == [["lag", Disturbance("lag", v2v_delay=2).items()]]
    for f in ("robustness.csv", "scenarios.csv", "curve.csv"):
        assert os.path.getsize(os.path.join(base, f)) > 0, f
    assert "train_disturbances" not in json.load(open(os.path.join(plain, "conf.json")))
    assert json.load(open(os.path.join(null, "conf.json")))["train_disturbances"] == [["clean", Disturbance("clean").items()]]
    a, b, c = _files(plain), _files(null), _files(base)
    assert set(a) == set(b) == set(c) and "robustness.csv" in a and any(f.endswith(".npz") for f in a)
    for f in a:
        assert a[f] == b[f], f
    assert a["robustness.csv"] != c["robustness.csv"]  # (other actors: trained on what the rough platoons observed)
