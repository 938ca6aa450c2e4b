"""Residual policies on the GPU (tr --residual): avd_step_fused_res_f32 (csrc/env.hip) built from pieces that exist -- the nominal
launch's action and leader input, the float32 law of tests/residual_oracle.py, avd_env_step_f32 -- and against its twins at zero gains;
avd_eval_cases_res_f32 / avd_eval_rollout_res_f32 (csrc/evalx.hip, csrc/eval.hip) against the linear evaluator with actors whose last
layer is zero, against their twins at zero gains, against each other and against the float64 oracle; then the trainer and the CLI. Every
comparison is exact unless a tolerance is named."""
import json
import os

import numpy as np
import pytest
import torch

from avddpg_amd import __main__ as cli
from avddpg_amd import config, evaluator, scenarios, vec
from avddpg_amd._hip import call, ptr, stream_handle
from avddpg_amd.scenarios import Disturbance, LinearLaw, Manoeuvre, ResidualLaw, parse_disturbance
from tests import residual_oracle as ro
from tests import scenario_oracle as so
from tests.gpu_util import need_gpu
from tests.test_gpu_train_leader import CAP, SEED, Lead, Levels, _conf, _differs, _eq, _inputs

pytestmark = pytest.mark.gpu

OUT = ("x", "pa", "cum", "rew", "term", "done", "flag", "ou", "action", "exog", "er", "ring")
LINK = 16  # slots of a vehicle's V2V ring (csrc/env.hip)


def _launch(conf, P, L, inp, res=None, tab=None, lead=None, key=(SEED,), ep_len=None, counter=1, ou_c=9, exog_c=13, slot=3):
    """One fused-step launch from the state ``inp`` (nothing of it is written). res None: the existing entry point the other arguments
    name; res = (gains [L, 4] device tensor, scale): avd_step_fused_res_f32 with the same arguments, and ``applied`` among the outputs."""
    S = 3 if conf.model == conf.modelA else 4
    f32 = dict(dtype=torch.float32, device="cuda")
    cst = vec.VecPlatoon(1, L, conf, rng="device").d_consts  # (device RNG: the constructor launches nothing)
    o = dict(x=torch.empty(P, L, 4, **f32), pa=inp["pa"].clone(), cum=inp["cum"].clone(), rew=torch.empty(P, L, **f32),
             term=torch.empty(P, L, dtype=torch.uint8, device="cuda"), done=torch.empty(P, dtype=torch.uint8, device="cuda"),
             flag=torch.tensor([0, 7], dtype=torch.int32, device="cuda"), ou=inp["ou"].clone(), action=torch.empty(P, L, **f32),
             exog=torch.empty(P, **f32), ring=inp["ring"].clone(), er=inp["er"].clone(), obs=torch.full((P, L, 4), 9.0, **f32),
             hist=inp["hist"].clone(), recv=inp["recv"].clone(), applied=torch.full((P, L), 77.0, **f32))
    head = (ptr(cst), P, L, S, ptr(inp["x"]), ptr(o["x"]), ptr(o["pa"]), ptr(o["cum"]), ptr(o["rew"]), ptr(o["term"]), ptr(o["done"]),
            ptr(o["flag"][0:1]), ptr(o["flag"][1:2]), ptr(inp["act"]), ptr(o["ou"]), ptr(o["action"]), ptr(o["exog"]), conf.theta, 0.0,
            conf.ou_dt, conf.std_dev, conf.action_low, conf.action_high, conf.reset_max_u, 1 if conf.rand_gen == conf.uniform else 0)
    tail = (ou_c, exog_c, ptr(o["ring"]), CAP, 1000 * CAP + slot, ptr(o["er"]))
    dist = (tab.n, tab.h, ptr(tab.d), ptr(tab.plant), ptr(inp["obs"]), ptr(o["obs"]), ptr(o["hist"]), ptr(o["recv"]), counter) if tab is not None else ()
    ld = (lead.n, lead.T, ptr(lead.table), ptr(lead.noise), ptr(lead.gauss), ptr(ep_len), 0) if lead is not None else ()
    if res is None:
        name = "avd_step_fused" + ("_dist" if tab is not None else "") + ("_lead" if lead is not None else "") + ("_seeds" if len(key) == 2 else "") + "_f32"
        call(name, *head, *key, *tail, *dist, *ld, *((1,) if lead is not None and tab is None else ()), stream_handle())
    else:
        gains, scale = res
        seed, grp = ((key[0],), (None, 1)) if len(key) == 1 else ((0,), key)
        call("avd_step_fused_res_f32", *head, *seed, *tail, *grp, *(dist or (0, None, None, None, None, None, None, None, 0)),
             *(ld or (0, 0, None, None, None, None, 0)), ptr(gains), scale, ptr(o["applied"]), stream_handle())
    return o


def _state(P, L, S, seed):
    inp = _inputs(P, L, S, seed)
    g = torch.Generator(device="cuda").manual_seed(seed + 100)
    inp["hist"] = 0.3 * torch.randn(P * L, LINK, generator=g, device="cuda")
    inp["recv"] = 0.3 * torch.randn(P * L, generator=g, device="cuda")
    return inp


def _table(L, model_a=False):
    """Distinct gain rows per vehicle (a wrong vehicle index shows); under Model A the kernel does not read the 4th."""
    v = np.arange(L, dtype=np.float32)
    return np.stack([0.5 + 0.125 * v, 1.0 + 0.25 * v, -0.1 - 0.05 * v, (7.0 if model_a else 0.3) + 0.1 * v], axis=1).astype(np.float32)


# ---- 1. the step, built from pieces that exist -----------------------------------------------------------------------------------
@pytest.mark.parametrize("model,L,P", [("ModelB", 5, 13), ("ModelA", 3, 22), ("ModelB", 16, 5)])
def test_step_is_the_nominal_action_through_the_law_into_env_step(model, L, P):
    need_gpu()
    conf = _conf(L, model)
    S, model_a = (3, True) if model == "ModelA" else (4, False)
    inp = _state(P, L, S, seed=5)
    gains, scale, slot = _table(L, model_a), 0.25, 3
    nominal = _launch(conf, P, L, inp)  # the same draws: r and the leader input are its action and leader_exog
    r, exog = nominal["action"], nominal["exog"]
    u = ro.law(gains[None], inp["x"].cpu().numpy(), scale, r.cpu().numpy(), conf.action_low, conf.action_high, model_a)
    assert u.shape == (P, L) and np.any(u != r.cpu().numpy()) and np.abs(u).max() <= conf.action_high
    d_u = torch.from_numpy(u).cuda()
    f32 = dict(dtype=torch.float32, device="cuda")
    e = dict(x=torch.empty(P, L, 4, **f32), pa=inp["pa"].clone(), cum=inp["cum"].clone(), rew=torch.empty(P, L, **f32),
             term=torch.empty(P, L, dtype=torch.uint8, device="cuda"), done=torch.empty(P, dtype=torch.uint8, device="cuda"))
    cst = vec.VecPlatoon(1, L, conf, rng="device").d_consts
    call("avd_env_step_f32", ptr(cst), P, L, ptr(inp["x"]), ptr(e["x"]), ptr(e["pa"]), ptr(e["cum"]), ptr(d_u), ptr(exog), ptr(e["rew"]),
         ptr(e["term"]), ptr(e["done"]), None, None, stream_handle())
    got = _launch(conf, P, L, inp, res=(torch.from_numpy(gains).cuda(), scale))
    for n in e:
        _eq(got[n], e[n], ("avd_env_step_f32 on u and the nominal leader input", n))
    _eq(got["action"], r, "action is the agent's r")
    _eq(got["applied"], d_u, "applied is u")
    for n in ("ou", "exog", "flag"):
        _eq(got[n], nominal[n], ("untouched by the law", n))
    _eq(got["er"], inp["er"] + got["rew"], "the episodic reward counters")
    row = torch.cat([inp["x"].view(-1, 4)[:, :S], r.view(-1, 1), got["rew"].view(-1, 1), got["x"].view(-1, 4)[:, :S]], dim=1)
    _eq(got["ring"][:, slot], row, "the replay row [x_in, r, reward, x_out]")
    keep = [k for k in range(CAP) if k != slot]
    _eq(got["ring"][:, keep], inp["ring"][:, keep], "the other replay rows")
    assert _differs(got["x"], nominal["x"]) and _differs(got["rew"], nominal["rew"])


# ---- 2. zero gains, scale 1: every existing twin, bit for bit, over two consecutive steps -------------------------------------------
def _next(inp, o):
    """The state after a launch as the next launch's input (the actors' outputs stay: any value serves)."""
    return dict(x=o["x"], pa=o["pa"], cum=o["cum"], act=inp["act"], ou=o["ou"], ring=o["ring"], er=o["er"], obs=o["obs"], hist=o["hist"],
                recv=o["recv"])


@pytest.mark.parametrize("form", ["plain", "seeds", "levels and manoeuvres"])
def test_zero_gains_are_the_existing_twin_bit_for_bit(form):
    need_gpu()
    L = 5
    conf = _conf(L)
    zero = (torch.zeros(L, 4, device="cuda"), 1.0)
    kw, P, outs = {}, 13, OUT
    if form == "seeds":
        P = 12
        d_seeds = vec.seed_table([40, 41], "cuda")[1]  # (kept alive to the end of the test: the launches read it)
        kw = dict(key=(ptr(d_seeds), 2))
    elif form == "levels and manoeuvres":
        kw = dict(tab=Levels([Disturbance("clean"), Disturbance("rough", noise_ep=0.1, v2v_delay=2, v2v_drop=0.1)], conf, L),
                  lead=Lead([Manoeuvre("brake", profile="brake", amp=0.5), Manoeuvre("clean")], conf),
                  ep_len=torch.from_numpy(((np.arange(P) * 5 + 3) % 12).astype(np.int32)).cuda())
        outs = OUT + ("obs", "hist", "recv")
    a = b = _state(P, L, 4, seed=9)
    for step in range(2):
        c = dict(counter=4 + step, ou_c=9 + step, exog_c=13 + step, slot=3 + step)
        ref, got = _launch(conf, P, L, a, **kw, **c), _launch(conf, P, L, b, res=zero, **kw, **c)
        for n in outs:
            _eq(got[n], ref[n], (form, step, n))
        _eq(got["applied"], ref["action"], (form, step, "applied is the clipped action"))
        a, b = _next(a, ref), _next(b, got)
    if form == "levels and manoeuvres":
        assert _differs(ref["obs"], ref["x"]) and _differs(ref["hist"], _state(P, L, 4, seed=9)["hist"])
        assert {float(v) for v in ref["exog"][0::4].cpu()} <= {0.0, -0.5}  # (platoons 0, 4, 8, 12: level 0, the brake row)


# ---- 3. under levels the law reads the observation --------------------------------------------------------------------------------
def test_under_levels_the_law_reads_what_the_agent_observed():
    need_gpu()
    L, P = 5, 13
    conf = _conf(L)
    inp = _state(P, L, 4, seed=11)
    tab = Levels([Disturbance("clean"), Disturbance("lag", v2v_delay=2)], conf, L)
    gains = np.tile(np.float32([1.0, 0.5, -0.25, 0.5]), (L, 1))
    twin = _launch(conf, P, L, inp, tab=tab, counter=4)
    got = _launch(conf, P, L, inp, res=(torch.from_numpy(gains).cuda(), 0.5), tab=tab, counter=4)
    r = twin["action"].cpu().numpy()
    on_obs = ro.law(gains[None], inp["obs"].cpu().numpy(), 0.5, r, conf.action_low, conf.action_high, False)
    on_x = ro.law(gains[None], inp["x"].cpu().numpy(), 0.5, r, conf.action_low, conf.action_high, False)
    assert np.all(on_obs != on_x)  # (the observation buffer is drawn independently of the state: the two laws differ everywhere)
    _eq(got["applied"], torch.from_numpy(on_obs), "applied is the law on obs_in")
    _eq(got["action"], twin["action"], "action is the agent's r")
    _eq(got["ring"][:, 3, :4], inp["obs"].view(-1, 4), "the replay row's s is the observation")
    _eq(got["ring"][:, 3, 4], twin["action"].view(-1), "the replay row's a is r")
    _eq(got["ring"][:, 3, 6:], got["obs"].view(-1, 4), "the replay row's s' is the new observation")
    # the plant is the level's: avd_env_step_f32 knows one plant only, so the nominal-plant platoons (level 0: the even ones) are checked
    f32 = dict(dtype=torch.float32, device="cuda")
    e = dict(x=torch.empty(P, L, 4, **f32), pa=inp["pa"].clone(), cum=inp["cum"].clone(), rew=torch.empty(P, L, **f32),
             term=torch.empty(P, L, dtype=torch.uint8, device="cuda"), done=torch.empty(P, dtype=torch.uint8, device="cuda"))
    cst = vec.VecPlatoon(1, L, conf, rng="device").d_consts
    call("avd_env_step_f32", ptr(cst), P, L, ptr(inp["x"]), ptr(e["x"]), ptr(e["pa"]), ptr(e["cum"]), ptr(got["applied"]), ptr(got["exog"]),
         ptr(e["rew"]), ptr(e["term"]), ptr(e["done"]), None, None, stream_handle())
    for n in e:  # (neither level changes the plant)
        _eq(got[n], e[n], ("avd_env_step_f32 on applied", n))


# ---- 4. the evaluators against the linear evaluator ---------------------------------------------------------------------------------
def _load(conf, actors):
    """Keras-ordered float64 weight lists (scenario_oracle.random_actors) as an AgentGroup's actors."""
    S = 3 if conf.model == conf.modelA else 4
    grp = vec.AgentGroup(len(actors), S, 1, conf, seed=1)
    for m, w in enumerate(actors):
        grp.set_weights(m, "actor", [np.asarray(t, dtype=np.float32) for t in w])
    return grp


def _zero_actors(conf, L, n_sets=None):
    n_sets = L if n_sets is None else n_sets
    grp = vec.AgentGroup(n_sets, 4, 1, conf, seed=3)
    lay = grp.lay
    grp.theta[:, lay.aW3:lay.aW3 + lay.H2] = 0.0
    grp.theta[:, lay.ab3] = 0.0
    return grp


def _same_results(got, ref, what):
    assert got.counters.shape == ref.counters.shape, (what, got.counters.shape, ref.counters.shape)
    for n, a, b in [("counters", got.counters, ref.counters), ("scores", got.scores, ref.scores)] + \
            [(n, got.metrics[n], ref.metrics[n]) for n in scenarios.METRICS]:
        assert a.dtype == b.dtype and np.array_equal(a, b), (what, n, np.argwhere(a != b)[:4])


CASES = {"K = 12": (["zero", "step", "ramp", "brake", "sine", "gaussian"], [6, 7]), "K = 1": (["brake"], [6]),
         "K = 5": (["zero", "step", "brake", "sine", "gaussian"], [7])}


@pytest.mark.parametrize("shape", list(CASES))
def test_zero_actors_are_the_linear_evaluator(shape):
    need_gpu()
    L, T = 5, 40
    conf = config.Config(pl_size=L)
    names, seeds = CASES[shape]
    grp = _zero_actors(conf, L)
    law, lin = ResidualLaw(1, 2, -0.5, 1, scale=0.5), [LinearLaw("law", 1, 2, -0.5, 1)]
    kw = dict(seeds=seeds, manual_timestep_override=T)
    got = evaluator.run_cases(conf, grp, [0], names, base_law=law, **kw)
    ref = evaluator.run_linear(conf, lin, names, **kw)
    assert got.counters.shape == (1, len(names), len(seeds), L) and np.all(got.metrics["sum_u2"] > 0)
    _same_results(got, ref, "run_cases")
    levels = [parse_disturbance("lag:v2v_delay=3,v2v_drop=0.1"), parse_disturbance("noisy:noise_ep=0.05")]
    got = evaluator.run_disturbed(conf, grp, [0], names, levels, base_law=law, **kw)
    ref = evaluator.run_linear(conf, lin, names, levels, **kw)
    assert got.counters.shape == (1, len(names), 3, len(seeds), L)
    _same_results(got, ref, "run_disturbed")
    assert len({got.counters[0, 0, d].tobytes() for d in range(3)}) == 3  # (both levels reach the law: it reads the observation)


# ---- 5. zero gains: today's evaluators ---------------------------------------------------------------------------------------------
def test_zero_gains_are_the_evaluators_without_a_law():
    need_gpu()
    L, T = 5, 40
    conf = config.Config(pl_size=L)
    grp = _load(conf, so.random_actors(conf, L, 21))
    zero = ResidualLaw(0, 0)
    names, seeds = ["step", "gaussian", "brake"], [6, 7]
    kw = dict(seeds=seeds, manual_timestep_override=T)
    _same_results(evaluator.run_cases(conf, grp, [0], names, base_law=zero, **kw), evaluator.run_cases(conf, grp, [0], names, **kw), "run_cases")
    levels = [Disturbance("lag", v2v_delay=3, v2v_drop=0.1), Disturbance("noisy", noise_ep=0.05)]
    _same_results(evaluator.run_disturbed(conf, grp, [0], names, levels, base_law=zero, **kw),
                  evaluator.run_disturbed(conf, grp, [0], names, levels, **kw), "run_disturbed")
    trace = [(0, 0), (0, 1)]
    sc, cnt, tr = evaluator.run_many(conf, grp, [0], trace=trace, base_law=zero, **kw)
    rsc, rcnt, rtr = evaluator.run_many(conf, grp, [0], trace=trace, **kw)
    assert np.array_equal(sc, rsc) and np.array_equal(cnt, rcnt) and np.abs(rtr[(0, 0)]["inputs"]).max() > 0.05
    for k in trace:
        for n in ("states", "inputs", "jerks", "counters"):
            assert np.array_equal(tr[k][n], rtr[k][n]), (k, n)


# ---- 6. the rollout kernel against the cases kernel -------------------------------------------------------------------------------
@pytest.mark.parametrize("sets", ["per_agent", "shared"])
def test_rollout_with_the_law_is_the_cases_kernel_with_the_law(sets):
    need_gpu()
    L, T = 5, 40
    conf = config.Config(pl_size=L)
    law = ResidualLaw(0.5, 1, 0, 0, scale=0.5)
    seeds = [6, 7]
    if sets == "shared":
        grp, platoons, kw = _load(conf, so.random_actors(conf, L, 23)), [0], dict(set_mod=L)
    else:
        grp, platoons, kw = _load(conf, so.random_actors(conf, 2 * L, 23)), [0, 1], {}
    trace = [(i, k) for i in range(len(platoons)) for k in range(2)]
    b = evaluator.prepare_many(conf, grp, platoons, seeds=seeds, manual_timestep_override=T, trace=trace, base_law=law, **kw)
    b.launch()
    sc, cnt, tr = b.results()
    cases = evaluator.run_cases(conf, grp, platoons, ["gaussian"], seeds=seeds, manual_timestep_override=T, base_law=law, **kw)
    assert np.array_equal(cnt, cases.counters[:, 0]) and np.array_equal(sc, cases.scores[:, 0])
    x0 = b.x0.cpu().numpy()
    for i, k in trace:
        m = scenarios.metrics_from_traces(tr[(i, k)], x0[k], conf)
        for n in scenarios.METRICS:
            assert np.array_equal(m[n], cases.metrics[n][i, 0, k]), (i, k, n)
    plain = evaluator.run_many(conf, grp, platoons, seeds=seeds, manual_timestep_override=T, **kw)[1]
    assert not np.array_equal(plain, cnt)  # (the law acts)
    if sets == "per_agent":
        assert not np.array_equal(cnt[0], cnt[1])


# ---- 7. against the float64 oracle -------------------------------------------------------------------------------------------------
ORACLE = dict(law=(0.5, 1.0, 0.0, 0.3), scale=0.5, actors_seed=31, last_scale=400.0)


@pytest.mark.parametrize("delay", [0, 3])
def test_against_the_float64_oracle(delay):
    """The standard case (Gaussian leader input, seed 6, T = 600, L = 5, Model B) with random actors and the law (0.5, 1, 0, 0.3) at
    scale 0.5, nominal and under a V2V delay of 3 steps, held to scenario_oracle.check_against's tolerances (set for actors alone).
    The inputs were kept because the same loop in float32 on the CPU (residual_oracle.rollout32; tests/test_residual_cpu.py asserts it)
    stays far inside HALF of each tolerance against the float64 oracle -- as fractions of the tolerance, nominal / delayed: max_abs_ep
    < 1e-4 / < 1e-4, max_abs_ev 3e-4 / 2e-4, max_abs_a 5e-4 / 2e-4, final_abs_ep < 1e-4 / < 1e-4, rms_u 2.4e-3 / 2.1e-3, rms_jerk 2e-4 /
    1e-4; no terminal step, |ep| and |ev| never within 17 of their bounds, the residual's rms 0.15 beside the plant input's 0.28, the
    clip reached on 8 / 5 samples."""
    need_gpu()
    L = 5
    conf = config.Config(pl_size=L)
    T = conf.steps_per_episode
    assert T == 600
    actors = so.random_actors(conf, L, ORACLE["actors_seed"], last_scale=ORACLE["last_scale"])
    law = ResidualLaw(*ORACLE["law"], scale=ORACLE["scale"])
    grp = _load(conf, actors)
    if delay:
        r = evaluator.run_disturbed(conf, grp, [0], ["gaussian"], [Disturbance("lag", v2v_delay=delay)], set_mod=L, base_law=law)
        got = {n: r.metrics[n][0, 0, 1, 0] for n in scenarios.METRICS}
    else:
        r = evaluator.run_cases(conf, grp, [0], ["gaussian"], set_mod=L, base_law=law)
        got = {n: r.metrics[n][0, 0, 0] for n in scenarios.METRICS}
    leader = scenarios.leader_profile("gaussian", T, conf, seed=6)
    ref, x0, tr = ro.rollout(so.env_params(conf), L, actors, law.gains(L), law.scale, leader, v2v_delay=delay)
    assert np.sqrt(np.mean(tr["residual"] ** 2)) > 0.05 and np.abs(tr["inputs"]).max() > 0.05  # both parts of the policy act
    so.check_against(got, ref, T)


# ---- 8. end to end -------------------------------------------------------------------------------------------------------------------
TR = ("tr", "--pl_num", "2", "--pl_size", "3", "--buffer_size", "500", "--total_time_steps", "80", "--rng", "device", "--episodes", "platoon",
      "--report_every", "40")


def _run(capsys, *argv):
    cli.main(list(argv))
    return capsys.readouterr().out.strip().splitlines()


def _files(d):
    """The run's files but conf.json: the CSVs as bytes, the checkpoints as their arrays' bytes (an .npz carries its write time)."""
    out = {}
    for f in sorted(os.listdir(d)):
        p = os.path.join(d, f)
        if f.endswith(".npz"):
            z = np.load(p)
            out[f] = [z[k].tobytes() for k in z.files]
        elif f != "conf.json" and os.path.isfile(p):
            out[f] = open(p, "rb").read()
    return out


def _esim_rewards(capsys, d, conf_json):
    lines = _run(capsys, "esim", d, "--n_timesteps", str(conf_json["steps_per_episode"]))
    return [np.float32(x.split()[-1]) for x in lines if x.startswith("platoon ")]


def test_cli_trains_a_residual_and_esim_applies_the_law(tmp_path, capsys):
    """`tr --residual kp=0.5,kv=1`: conf.json holds residual_law and esim reproduces the simulation rewards (which the actors alone do
    not give); with --seeds 1,2 on the per_agent engine experiment k is the solo run --seed k byte for byte."""
    need_gpu()
    res = ("--residual", "kp=0.5,kv=1", "--fed_method", "interfrl", "--engine", "per_agent")
    solo = {k: _run(capsys, *TR, *res, "--seed", str(k), "--out", str(tmp_path / f"solo{k}"))[-1] for k in (1, 2)}
    cj = json.load(open(os.path.join(solo[1], "conf.json")))
    assert cj["residual_law"] == [["kp", 0.5], ["kv", 1.0], ["ka", 0.0], ["kf", 0.0], ["scale", 1.0], ["source", "given"]]
    rews = _esim_rewards(capsys, solo[1], cj)
    assert len(rews) == cj["saved_platoons"] == 2
    assert [np.float32(r / cj["re_scalar"]) for r in rews] == [np.float32(r) for r in cj["pl_rews_for_simulations"]]
    # the saved actors alone are not the policy: without the record esim scores something else
    bare = dict(cj)
    del bare["residual_law"]
    json.dump(bare, open(os.path.join(solo[1], "conf.json"), "w"))
    assert _esim_rewards(capsys, solo[1], cj) != rews
    json.dump(cj, open(os.path.join(solo[1], "conf.json"), "w"))
    batch = _run(capsys, *TR, *res, "--seeds", "1,2", "--out", str(tmp_path / "batch"))[-1]
    for k in (1, 2):
        a, b = _files(solo[k]), _files(os.path.join(batch, f"seed{k}"))
        assert set(a) == set(b) and "curve.csv" in a and sum(f.endswith(".npz") for f in a) >= 4 * 2 * 3
        for f in a:
            assert a[f] == b[f], (k, f)
        bj = json.load(open(os.path.join(batch, f"seed{k}", "conf.json")))
        assert bj["residual_law"] == cj["residual_law"]
        assert bj["pl_rews_for_simulations"] == json.load(open(os.path.join(solo[k], "conf.json")))["pl_rews_for_simulations"]
    assert _files(solo[1])["curve.csv"] != _files(solo[2])["curve.csv"]


def test_cli_zero_law_changes_no_file_and_keep_best_runs(tmp_path, capsys):
    """`tr --residual kp=0,kv=0` writes what a run without the flag writes, apart from conf.json's new field; with a law the files
    differ; `--keep_best 10` runs under a law and `esim <dir>/best` reproduces best/conf.json's rewards."""
    need_gpu()
    suite = ("--scenarios", "brake,gaussian", "--disturb", "lag:v2v_delay=2")
    plain = _run(capsys, *TR, *suite, "--out", str(tmp_path / "plain"))[-1]
    zero = _run(capsys, *TR, *suite, "--residual", "kp=0,kv=0", "--out", str(tmp_path / "zero"))[-1]
    kept = _run(capsys, *TR, *suite, "--residual", "kp=0.5,kv=1,scale=0.5", "--keep_best", "10", "--out", str(tmp_path / "kept"))[-1]
    a, b, c = _files(plain), _files(zero), _files(kept)
    assert set(a) == set(b) and {"curve.csv", "scenarios.csv", "robustness.csv"} <= set(a) and any(f.endswith(".npz") for f in a)
    for f in a:
        assert a[f] == b[f], f
    pj, zj = json.load(open(os.path.join(plain, "conf.json"))), json.load(open(os.path.join(zero, "conf.json")))
    assert "residual_law" not in pj and dict(zj.pop("residual_law")) == dict(kp=0.0, kv=0.0, ka=0.0, kf=0.0, scale=1.0, source="given")
    assert {k: v for k, v in zj.items() if k != "timestamp"} == {k: v for k, v in pj.items() if k != "timestamp"}
    assert a["curve.csv"] != c["curve.csv"] and a["scenarios.csv"] != c["scenarios.csv"]
    kj, bj = json.load(open(os.path.join(kept, "conf.json"))), json.load(open(os.path.join(kept, "best", "conf.json")))
    assert dict(kj["residual_law"])["scale"] == 0.5 and bj["residual_law"] == kj["residual_law"]
    assert dict(bj["keep_best"])["evaluations"] == 9  # steps 0, 10, ..., 80
    rews = _esim_rewards(capsys, os.path.join(kept, "best"), bj)
    assert [np.float32(r / bj["re_scalar"]) for r in rews] == [np.float32(r) for r in bj["pl_rews_for_simulations"]]
    assert os.path.getsize(os.path.join(kept, "best", "scenarios.csv")) > 0


def test_cli_residual_tuned_trains_on_the_law_the_grid_picks_and_searches_once(tmp_path, capsys, monkeypatch):
    """`tr --residual tuned --scenarios ... --baseline_tune GRID`: the law is the grid's best on the suite, searched before training and
    once (the baseline section reuses the result); conf.json records it with source `tuned`."""
    need_gpu()
    calls = []
    real = evaluator.tune_linear
    monkeypatch.setattr(evaluator, "tune_linear", lambda *a, **k: calls.append(1) or real(*a, **k))
    base = _run(capsys, *TR, "--residual", "tuned", "--scenarios", "gaussian,brake", "--baseline_tune", "kp=0:2:3,kv=0:2:3",
                "--out", str(tmp_path))[-1]
    cj = json.load(open(os.path.join(base, "conf.json")))
    law, tune = dict(cj["residual_law"]), dict(cj["baseline_tune"])
    assert len(calls) == 1 and law["source"] == "tuned" and law["scale"] == 1.0
    assert [[k, law[k]] for k in scenarios.GAIN_KEYS] == tune["gains"] and tune["candidates"] == 9
    assert (law["kp"], law["kv"]) != (0.0, 0.0)  # (the zero law is the grid's first candidate and not its best)
    assert [n for n, _ in cj["baseline_suite"]] == ["tuned"] and os.path.getsize(os.path.join(base, "baseline.csv")) > 0
    rews = _esim_rewards(capsys, base, cj)
    assert [np.float32(r / cj["re_scalar"]) for r in rews] == [np.float32(r) for r in cj["pl_rews_for_simulations"]]
