"""Training under leader manoeuvres on the GPU: avd_step_fused_lead_f32 and its three twins (csrc/env.hip) against the nominal and the
disturbed launch where every manoeuvre is the clean gaussian one, against tests/train_leader_oracle.py and avd_env_step_f32 where
they are not; then VecTrainer(train_leader=...), the seed batch and the CLI. Every comparison is exact: each value is a table entry or
made by arithmetic an existing kernel already performs.

Shapes (L, P), those of tests/test_gpu_train_disturb.py: (5, 13) 12 platoons per wave -- a second wave with idle lanes; (1, 70);
(16, 5) 4 per wave; (3, 90) a second workgroup (84 platoons per block). Episodes of T = 12 steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from avddpg_amd import config, scenarios, trainer, vec
from avddpg_amd._hip import call, ptr, stream_handle
from avddpg_amd.scenarios import Disturbance, Manoeuvre
from tests import train_leader_oracle as tlo
from tests.gpu_util import need_gpu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 13), (1, 70), (16, 5), (3, 90)]
T = 12
CAP, SLOT, OU_C, EXOG_C, SEED = 8, 3, 9, 13, 21
OUT = ("x", "pa", "cum", "rew", "term", "done", "flag", "ou", "action", "exog", "er", "ring")


def _eq(a, b, what):
    a, b = (torch.as_tensor(t).cpu() for t in (a, b))
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype.is_floating_point:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)  # bitwise, NaN-safe
    assert torch.equal(a, b), f"{what}: {(a != b).sum().item()} of {a.numel()} differ"


def _differs(a, b):
    return not torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))


def _conf(L, model="ModelB", **kw):
    conf = config.Config(pl_size=L, model=model, episode_sim_time=1.25, **kw)
    assert conf.steps_per_episode == T
    return conf


def _inputs(P, L, S, seed=5):
    """A state well inside the terminal bounds, random everything else."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *sh: torch.randn(*sh, generator=g, device="cuda")
    return dict(x=0.5 * rn(P, L, 4), pa=0.1 * rn(P, L), cum=rn(P, L), act=rn(P, L), ou=0.2 * rn(P, L), ring=rn(P * L, CAP, 2 * S + 2),
                er=rn(P, L), obs=0.5 * rn(P, L, 4))


class Levels:
    """The device tables of a level list, as VecPlatoon(train_disturb=...) makes them."""

    def __init__(self, levels, conf, L):
        self.levels = scenarios.check_disturbances(levels, conf)
        self.n = len(self.levels)
        self.h, self.d = vec.train_level_table(self.levels, "cuda")
        self.plant = torch.from_numpy(np.stack([scenarios.plant_table(conf, L, d.dyn_coeff) for d in self.levels])).cuda()


class Lead:
    """The device tables of a manoeuvre list, as VecTrainer(train_leader=...) makes them."""

    def __init__(self, manoeuvres, conf):
        self.ms = scenarios.check_manoeuvres(manoeuvres)
        table, noise, gauss = scenarios.manoeuvre_table(conf, self.ms)
        self.n, self.T = table.shape
        self.table, self.noise, self.gauss = torch.from_numpy(table).cuda(), torch.from_numpy(noise).cuda(), torch.from_numpy(gauss.astype(np.uint8)).cuda()


def _step(conf, P, L, inp, lead=None, tab=None, key=(SEED,), ep_len=None, ep_step=0, link=None, counter=1):
    """One launch from the state ``inp`` (nothing of it is written): the nominal / disturbed step (lead None) or its manoeuvre twin.
    key: (seed,) or (d_seeds, E). ep_len: int32 [P] device tensor or None (then ep_step)."""
    S = 3 if conf.model == conf.modelA else 4
    f32 = dict(dtype=torch.float32, device="cuda")
    cst = vec.VecPlatoon(1, L, conf, rng="device").d_consts  # (device RNG: the constructor launches nothing)
    o = dict(x=torch.empty(P, L, 4, **f32), pa=inp["pa"].clone(), cum=inp["cum"].clone(), rew=torch.empty(P, L, **f32),
             term=torch.empty(P, L, dtype=torch.uint8, device="cuda"), done=torch.empty(P, dtype=torch.uint8, device="cuda"),
             flag=torch.tensor([0, 7], dtype=torch.int32, device="cuda"), ou=inp["ou"].clone(), action=torch.empty(P, L, **f32),
             exog=torch.empty(P, **f32), ring=inp["ring"].clone(), er=inp["er"].clone(), obs=torch.full((P, L, 4), 9.0, **f32))
    head = (ptr(cst), P, L, S, ptr(inp["x"]), ptr(o["x"]), ptr(o["pa"]), ptr(o["cum"]), ptr(o["rew"]), ptr(o["term"]), ptr(o["done"]),
            ptr(o["flag"][0:1]), ptr(o["flag"][1:2]), ptr(inp["act"]), ptr(o["ou"]), ptr(o["action"]), ptr(o["exog"]), conf.theta, 0.0,
            conf.ou_dt, conf.std_dev, conf.action_low, conf.action_high, conf.reset_max_u, 1 if conf.rand_gen == conf.uniform else 0, *key,
            OU_C, EXOG_C, ptr(o["ring"]), CAP, 1000 * CAP + SLOT, ptr(o["er"]))
    name = "avd_step_fused" + ("_dist" if tab is not None else "") + ("_lead" if lead is not None else "") + ("_seeds" if len(key) == 2 else "") + "_f32"
    dist, ld = (), ()
    if tab is not None:
        hist, recv = link if link is not None else (None, None)
        dist = (tab.n, tab.h, ptr(tab.d), ptr(tab.plant), ptr(inp["obs"]), ptr(o["obs"]), ptr(hist), ptr(recv), counter)
    if lead is not None:
        ld = (lead.n, lead.T, ptr(lead.table), ptr(lead.noise), ptr(lead.gauss), ptr(ep_len), ep_step) + (() if tab is not None else (1,))
    call(name, *head, *dist, *ld, stream_handle())
    return o


def _ep_len(P, clamp_at=1):
    """Steps of the platoons' own episodes: spread over 0 .. T - 1 (platoon 4 sits at T - 1), platoon ``clamp_at`` past the episode's end
    (a defined input: the kernel clamps it to T - 1)."""
    k = (np.arange(P) * 5 + 3) % T
    assert k[4] == T - 1 and len(set(k.tolist())) == min(P, T)
    k[clamp_at] = T + 7
    return k, torch.from_numpy(k.astype(np.int32)).cuda()


LEVELS = lambda: [Disturbance("clean"), Disturbance("rough", noise_ep=0.1, noise_a=0.05, dyn_coeff=0.15), Disturbance("lag", noise_ev=0.2)]
MIXED = lambda: [Manoeuvre("step", profile="step"), Manoeuvre("brake", profile="brake", amp=0.5), Manoeuvre("sine", profile="sine", amp=0.3, period=0.7, noise=0.05),
                 Manoeuvre("clean")]


# ---- 1. all-gaussian manoeuvres are today's launches ----------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["ModelB", "ModelA"])
@pytest.mark.parametrize("L,P", SHAPES)
def test_gaussian_manoeuvres_are_the_nominal_and_the_disturbed_launch_bit_for_bit(L, P, model):
    need_gpu()
    conf = _conf(L, model)
    S = 3 if model == "ModelA" else 4
    inp = _inputs(P, L, S)
    lead = Lead([Manoeuvre("a"), Manoeuvre("b", noise=conf.reset_max_u), Manoeuvre("c")], conf)
    _, ep_len = _ep_len(P)
    ref = _step(conf, P, L, inp)
    for what, kw in (("ep_len", dict(ep_len=ep_len)), ("ep_step", dict(ep_step=T - 1))):
        got = _step(conf, P, L, inp, lead, **kw)
        for n in OUT:
            _eq(got[n], ref[n], (what, n))
    assert int(ref["flag"][1]) == 0
    tab = Levels(LEVELS(), conf, L)
    ref = _step(conf, P, L, inp, tab=tab, counter=4)
    got = _step(conf, P, L, inp, lead, tab=tab, counter=4, ep_len=ep_len)
    for n in OUT + ("obs",):
        _eq(got[n], ref[n], ("with levels", n))
    assert _differs(ref["obs"], ref["x"])


# ---- 2. mixed manoeuvres: the exog from the oracle, the state from avd_env_step_f32 on it, the rest untouched ----------------------
def _check_mixed(conf, P, L, inp, got, want_exog, nominal):
    S = 3 if conf.model == conf.modelA else 4
    _eq(got["exog"], torch.from_numpy(want_exog), "leader_exog")
    f32 = dict(dtype=torch.float32, device="cuda")
    e = dict(x=torch.empty(P, L, 4, **f32), pa=inp["pa"].clone(), cum=inp["cum"].clone(), rew=torch.empty(P, L, **f32),
             term=torch.empty(P, L, dtype=torch.uint8, device="cuda"), done=torch.empty(P, dtype=torch.uint8, device="cuda"))
    cst = vec.VecPlatoon(1, L, conf, rng="device").d_consts
    call("avd_env_step_f32", ptr(cst), P, L, ptr(inp["x"]), ptr(e["x"]), ptr(e["pa"]), ptr(e["cum"]), ptr(got["action"]), ptr(got["exog"]),
         ptr(e["rew"]), ptr(e["term"]), ptr(e["done"]), None, None, stream_handle())
    for n in e:
        _eq(got[n], e[n], ("avd_env_step_f32 on the launch's action and exog", n))
    for n in ("ou", "action", "er", "flag"):
        _eq(got[n], nominal[n], ("untouched by the manoeuvre", n))
    _eq(got["ring"][:, :, :S + 2], nominal["ring"][:, :, :S + 2], "the replay row's s, a, r")
    _eq(got["ring"][:, SLOT, S + 2:], got["x"].view(-1, 4)[:, :S], "the replay row's s'")


@pytest.mark.parametrize("rand_gen", ["normal", "uniform"])
@pytest.mark.parametrize("model", ["ModelB", "ModelA"])
@pytest.mark.parametrize("L,P", SHAPES)
def test_mixed_manoeuvres_at_the_platoons_own_episode_steps(L, P, model, rand_gen):
    need_gpu()
    conf = _conf(L, model, rand_gen=rand_gen)
    S = 3 if model == "ModelA" else 4
    inp = _inputs(P, L, S, seed=6)
    lead = Lead(MIXED(), conf)
    k, ep_len = _ep_len(P)
    got, nominal = _step(conf, P, L, inp, lead, ep_len=ep_len), _step(conf, P, L, inp)
    want = tlo.expected_exog(conf, lead.ms, P, k, [SEED], EXOG_C)
    _check_mixed(conf, P, L, inp, got, want, nominal)
    # what the oracle says, said once more by hand for the platoons whose value is a bare table entry, the clamped one among them
    table = lead.table.cpu().numpy()
    exog = got["exog"].cpu().numpy()
    for p in range(P):
        m = p % 4
        if m in (0, 1):
            assert exog[p].view(np.int32) == table[m, min(k[p], T - 1)].view(np.int32), p
    assert k[1] > T - 1 and exog[1] == np.float32(0.0)  # (the brake row's last entry; unclamped, the index would land in the sine row)
    gauss = np.arange(P) % 4 == 3
    _eq(got["exog"].cpu()[gauss], nominal["exog"].cpu()[gauss], "the gaussian share draws what the nominal launch draws")
    assert _differs(got["x"], nominal["x"])
    # the noisy sine: the table entry plus the scaled draw, not the entry alone
    sine = np.arange(P) % 4 == 2
    assert sine.any() and np.all(exog[sine] != table[2, np.minimum(k, T - 1)][sine])


# ---- 3. the host-step form ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ep_step", [0, T // 4, T - 1])
@pytest.mark.parametrize("L,P", SHAPES)
def test_host_step_form_reads_one_step_for_every_platoon(L, P, ep_step):
    need_gpu()
    conf = _conf(L)
    inp = _inputs(P, L, 4, seed=7)
    lead = Lead(MIXED(), conf)
    got, nominal = _step(conf, P, L, inp, lead, ep_len=None, ep_step=ep_step), _step(conf, P, L, inp)
    _check_mixed(conf, P, L, inp, got, tlo.expected_exog(conf, lead.ms, P, ep_step, [SEED], EXOG_C), nominal)
    want = {0: 0.0 if ep_step < T // 4 else conf.reset_max_u, 1: -0.5 if T // 4 <= ep_step < T // 2 else 0.0}
    for m, v in want.items():
        assert bool((got["exog"][m::4] == float(np.float32(v))).all()), (m, ep_step)


# ---- 4. the seed-batch form ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_levels", [False, True])
@pytest.mark.parametrize("L,P", SHAPES)
def test_seed_batch_launch_equals_the_solo_launches(L, P, with_levels):
    """E = 3 experiments of P platoons each: experiment e's slice of the batch launch equals its solo launch bit for bit, the manoeuvre
    (and the level) assigned by the solo run's platoon index."""
    need_gpu()
    E = 3
    conf = _conf(L)
    inp = _inputs(P * E, L, 4, seed=8)
    lead = Lead(MIXED(), conf)
    tab = Levels(LEVELS(), conf, L) if with_levels else None
    seeds, d_seeds = vec.seed_table(range(40, 40 + E), "cuda")
    k = (np.arange(P * E) * 7 + 2) % T
    ep_len = torch.from_numpy(k.astype(np.int32)).cuda()
    g = _step(conf, P * E, L, inp, lead, tab=tab, key=(ptr(d_seeds), E), ep_len=ep_len, counter=4)
    n_levels = tab.n if with_levels else 1
    _eq(g["exog"], torch.from_numpy(tlo.expected_exog(conf, lead.ms, P * E, k, list(seeds), EXOG_C, n_levels=n_levels)), "batch exog")
    for e, sd in enumerate(seeds):
        sub = {n: t.view(P, E, *t.shape[1:])[:, e].contiguous() for n, t in inp.items() if n != "ring"}
        sub["ring"] = inp["ring"].view(P, E, L, CAP, -1)[:, e].reshape(-1, CAP, 10).contiguous()
        solo = _step(conf, P, L, sub, lead, tab=tab, key=(sd,), ep_len=ep_len.view(P, E)[:, e].contiguous(), counter=4)
        for n in ("x", "pa", "cum", "rew", "term", "done", "ou", "action", "exog", "er", "obs"):
            _eq(g[n].view(P, E, *g[n].shape[1:])[:, e], solo[n], ("seed batch", n, e))
        _eq(g["ring"].view(P, E, L, CAP, -1)[:, e].reshape(-1, CAP, 10), solo["ring"], ("seed batch ring", e))


# ---- 5. the trainer ---------------------------------------------------------------------------------------------------------
def _tconf(**kw):
    conf = config.Config(num_platoons=6, pl_size=3, episode_sim_time=1.25, buffer_size=256, **kw)
    assert conf.steps_per_episode == T
    return conf


REGIMES = {"nofrl per_agent": dict(), "interfrl per_agent": dict(fed_method="interfrl")}


def _train(conf_kw, auto_reset, manoeuvres, steps=80, **more):
    """``steps`` training steps; -> (trainer, per-step leader_exog [steps, P], per-step k [steps, P]: the step of each platoon's own
    episode at the launch, replayed on the host from the done flags / the host loop's counter)."""
    conf = _tconf(**conf_kw)
    vt = trainer.VecTrainer(conf, rng="device", auto_reset=auto_reset, shared_engine="per_agent", train_leader=manoeuvres, **more)
    exog, ks = [], []
    if auto_reset is False:  # the host episode loop (VecTrainer.run's, with the trace taken per step)
        ep = 0
        while len(exog) < steps:
            vt.episode = ep
            vt.reset_episode()
            for i in range(conf.steps_per_episode):
                ks.append(np.full(vt.P, i))
                flag = vt.step(ep, i)
                exog.append(vt.leader_exog.cpu().numpy().copy())
                if flag or len(exog) == steps:
                    break
            ep += 1
    else:
        vt.reset_episode()
        k = np.zeros(vt.P, dtype=np.int64)
        for _ in range(steps):
            ks.append(k.copy())
            vt.step()
            exog.append(vt.leader_exog.cpu().numpy().copy())
            done = vt.env.done.cpu().numpy() != 0
            k = np.where(done | (k + 1 >= conf.steps_per_episode), 0, k + 1)  # episode_end's rule
        assert np.array_equal(vt.env.ep_len.cpu().numpy(), k)
    torch.cuda.synchronize()
    return vt, np.stack(exog), np.stack(ks)


def _state(vt):
    ag = vt.agents
    out = dict(theta=ag.theta, theta_t=ag.theta_t, stats=ag.stats, stats_t=ag.stats_t, m=ag.m, v=ag.v, adam_step=ag.step, ring=vt.replay.ring,
               x=vt.env.x, prev_a=vt.env.prev_a, ep_reward=vt.ep_reward, ou=vt.ou.state, exog=vt.leader_exog)
    if vt.env.ep_stats is not None:
        out.update({"ep_" + k: t for k, t in vt.env.ep_stats.items()})
    return out


@pytest.mark.parametrize("auto_reset", ["platoon", False])
@pytest.mark.parametrize("regime", list(REGIMES))
def test_trainer_under_manoeuvres(regime, auto_reset):
    """80 steps of 12-step episodes. [gaussian] is the plain trainer bit for bit. Under [clean, brake amp 0.5] the even platoons keep the
    plain run's leader inputs and the odd ones follow the brake row at the step of their own episode, across several episode ends."""
    need_gpu()
    conf_kw = REGIMES[regime]
    plain, plain_exog, _ = _train(conf_kw, auto_reset, None)
    assert plain.lead is None and (auto_reset is False or plain.env.ep_len is not None)
    vt, exog, _ = _train(conf_kw, auto_reset, [Manoeuvre("gaussian")])
    assert vt.lead is not None and vt.replay.buffer_counter == 80 and int(vt.agents.step.min()) >= 80 - 65
    for n, t in _state(plain).items():
        _eq(_state(vt)[n], t, (regime, auto_reset, n))
    _eq(exog, plain_exog, "the trace of leader inputs")
    vt, exog, ks = _train(conf_kw, auto_reset, [Manoeuvre("clean"), Manoeuvre("brake", profile="brake", amp=0.5)])
    _eq(exog[:, 0::2], plain_exog[:, 0::2], "the gaussian share keeps the plain run's leader inputs")
    row = scenarios.leader_profile("brake", T, vt.conf, 0.5)
    _eq(exog[:, 1::2], row[ks[:, 1::2]], "the brake share follows the table at the step of its own episode")
    assert (ks == 0).sum(axis=0).min() >= 80 // T and ks.max() >= T // 2  # several episodes each, some through the brake window
    assert {float(v) for v in exog[:, 1::2].ravel()} == {0.0, -0.5}
    got = _state(vt)
    assert _differs(got["theta"], _state(plain)["theta"]) and _differs(got["ring"], _state(plain)["ring"])
    for n in ("theta", "theta_t", "m", "v", "ring", "x", "ou", "ep_reward"):
        assert bool(torch.isfinite(got[n]).all()), n


# ---- 6. a seed batch with manoeuvres and levels together -------------------------------------------------------------------------
def test_seed_batch_with_manoeuvres_and_levels_is_its_solo_runs_bit_for_bit():
    need_gpu()
    levels = lambda: [Disturbance("clean"), Disturbance("rough", noise_ep=0.1, noise_a=0.05, v2v_delay=2, v2v_drop=0.2, dyn_coeff=0.15)]
    ms = lambda: [Manoeuvre("clean"), Manoeuvre("brake", profile="brake", amp=0.5), Manoeuvre("sine", profile="sine", period=0.6, noise=0.02)]
    seeds = [3, 4]
    batch, bexog, _ = _train({}, "platoon", ms(), seeds=seeds, train_disturb=levels())
    E, M, P = 2, 3, 6
    for e, k in enumerate(seeds):
        solo, sexog, ks = _train({}, "platoon", ms(), seed=k, init_seed=k, train_disturb=levels())
        per_agent = lambda t: t.view(P, E, M, *t.shape[1:])[:, e].reshape(P * M, *t.shape[1:])
        per_platoon = lambda t: t.view(P, E, *t.shape[1:])[:, e]
        for n in ("theta", "theta_t", "stats", "stats_t", "m", "v", "step"):
            _eq(per_agent(getattr(batch.agents, n)), getattr(solo.agents, n), (n, e))
        _eq(per_agent(batch.replay.ring), solo.replay.ring, ("ring", e))
        for n in ("x", "obs", "link_hist", "link_recv", "ep_len"):
            _eq(per_platoon(getattr(batch.env, n)), getattr(solo.env, n), (n, e))
        _eq(bexog[:, e::E], sexog, ("the trace of leader inputs", e))
        # levels and manoeuvres cross: platoon q of the solo run is under level q % 2 and manoeuvre (q // 2) % 3
        brake = [q for q in range(P) if tlo.manoeuvre_of(q, 3, n_levels=2) == 1]
        assert brake == [2, 3]
        _eq(sexog[:, brake], scenarios.leader_profile("brake", T, solo.conf, 0.5)[ks[:, brake]], ("brake share", e))
    assert _differs(batch.env.obs, batch.env.x)


# ---- 7. the CLI -------------------------------------------------------------------------------------------------------------
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


def test_cli_trains_under_manoeuvres_and_without_the_flag_nothing_changes(tmp_path):
    """`tr ... --train_leader clean --train_leader brake:amp=0.5 --scenarios brake` records the manoeuvres and writes scenarios.csv.
    Without the flag conf.json has no train_leader and every other file is byte-identical to the run under the one gaussian
    manoeuvre, which the trainer test above ties to the plain trainer bit for bit."""
    need_gpu()
    tr = ("tr", "--pl_num", "4", "--pl_size", "2", "--buffer_size", "500", "--total_time_steps", "70", "--rng", "device", "--episodes", "platoon",
          "--report_every", "70", "--scenarios", "brake")
    plain = _run(*tr, "--out", str(tmp_path / "plain"))
    null = _run(*tr, "--train_leader", "clean", "--out", str(tmp_path / "null"))
    base = _run(*tr, "--train_leader", "clean", "--train_leader", "brake:amp=0.5", "--out", str(tmp_path / "with"))
    conf = json.load(open(os.path.join(base, "conf.json")))
    assert conf["train_leader"] == [["clean", [["profile", "gaussian"], ["amp", None], ["period", 10.0], ["noise", None]]],
                                    ["brake", [["profile", "brake"], ["amp", 0.5], ["period", 10.0], ["noise", None]]]]
    assert conf["scenario_suite"][0] == ["names", ["brake"]]
    for f in ("scenarios.csv", "curve.csv"):
        assert os.path.getsize(os.path.join(base, f)) > 0, f
    pconf = json.load(open(os.path.join(plain, "conf.json")))
    assert "train_leader" not in pconf and "train_disturbances" not in pconf
    nconf = json.load(open(os.path.join(null, "conf.json")))
    assert nconf.pop("train_leader") == [["clean", Manoeuvre("clean").items()]]
    assert set(nconf) == set(pconf) and nconf["pl_rews_for_simulations"] == pconf["pl_rews_for_simulations"]
    a, b, c = _files(plain), _files(null), _files(base)
    assert set(a) == set(b) == set(c) and "scenarios.csv" in a and any(f.endswith(".npz") for f in a)
    for f in a:
        assert a[f] == b[f], f
    assert a["scenarios.csv"] != c["scenarios.csv"]  # (other actors: half the platoons trained behind a braking leader)
