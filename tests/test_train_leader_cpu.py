"""Training under leader manoeuvres without a GPU: the parser and its refusals, scenarios.manoeuvre_table against leader_profile, the
platoon -> manoeuvre assignment, trainer.check_train_leader, what the four new entry points refuse on the host, and the CLI's argument
errors."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from avddpg_amd import _hip, config, scenarios, trainer
from avddpg_amd.scenarios import Manoeuvre, check_manoeuvres, manoeuvre_table, parse_manoeuvre
from tests import train_leader_oracle as tlo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parse_manoeuvre():
    m = parse_manoeuvre("hard:profile=brake,amp=0.5,period=4,noise=0.05")
    assert (m.name, m.profile, m.amp, m.period, m.noise) == ("hard", "brake", 0.5, 4.0, 0.05)
    assert m.items() == [["profile", "brake"], ["amp", 0.5], ["period", 4.0], ["noise", 0.05]]
    for name in scenarios.SCENARIOS:  # a bare profile name is that profile with defaults
        m = parse_manoeuvre(name)
        assert (m.name, m.profile, m.amp, m.period, m.noise) == (name, name, None, 10.0, None)
    m = parse_manoeuvre("brake:amp=0.5")
    assert (m.name, m.profile, m.amp) == ("brake", "brake", 0.5)
    m = parse_manoeuvre(" clean ")
    assert (m.name, m.profile, m.noise) == ("clean", "gaussian", None)
    assert parse_manoeuvre("clean:noise=0.2").noise == 0.2
    assert parse_manoeuvre("sine:profile=step").profile == "step"  # the key wins over the name


@pytest.mark.parametrize("text,msg", [
    (":amp=1", "no name before ':'"),
    ("a:speed=1", "unknown key 'speed'"),
    ("a:amp", "unknown key 'amp'"),
    ("a:profile=step,amp=1,amp=2", "amp given twice"),
    ("a:profile=step,profile=ramp", "profile given twice"),
    ("a:profile=step,amp=fast", "amp='fast' is not a number"),
    ("clean:amp=1", "the gaussian profile takes neither amp nor period"),
    ("a:profile=gaussian,period=5", "the gaussian profile takes neither amp nor period"),
])
def test_parse_manoeuvre_refusals(text, msg):
    with pytest.raises(ValueError, match=msg):
        parse_manoeuvre(text)


@pytest.mark.parametrize("ms,msg", [
    ([], "0 manoeuvres listed: 1 to 16"),
    ([Manoeuvre(f"m{k}") for k in range(17)], "17 manoeuvres listed: 1 to 16"),
    (["brake"], "is not a scenarios.Manoeuvre"),
    ([Manoeuvre("a", profile="swerve")], "unknown profile 'swerve'"),
    ([Manoeuvre("a", profile="step", amp=float("nan"))], "amp=nan must be a finite number"),
    ([Manoeuvre("a", profile="sine", period=float("inf"))], "period=inf must be a finite number"),
    ([Manoeuvre("a", noise=float("inf"))], "noise=inf must be a finite number"),
    ([Manoeuvre("a", profile="sine", period=0.0)], r"period=0.0 must be > 0"),
    ([Manoeuvre("a", profile="sine", period=-2.0)], r"period=-2.0 must be > 0"),
    ([Manoeuvre("a", profile="step", noise=-0.1)], r"noise=-0.1 must be >= 0"),
    ([Manoeuvre("a", amp=0.3)], "the gaussian profile takes neither amp nor period"),
    ([Manoeuvre("a", period=5.0)], "the gaussian profile takes neither amp nor period"),
    ([Manoeuvre("a"), Manoeuvre("b", profile="step"), Manoeuvre("a", profile="brake")], r"manoeuvre\(s\) \['a'\] listed more than once"),
])
def test_check_manoeuvres_refusals(ms, msg):
    with pytest.raises(ValueError, match=msg):
        check_manoeuvres(ms)


def test_check_manoeuvres_accepts_sixteen():
    ms = [Manoeuvre(f"m{k}", profile="sine", period=1.0 + k) for k in range(16)]
    assert check_manoeuvres(ms) == ms


@pytest.mark.parametrize("T", [600, 4])
def test_manoeuvre_table_rows_are_leader_profile_rows(T):
    conf = config.Config(episode_sim_time=T * 0.1 + 0.05)
    assert conf.steps_per_episode == T
    ms = [Manoeuvre("zero", profile="zero"), Manoeuvre("step", profile="step"), Manoeuvre("ramp", profile="ramp", amp=0.3),
          Manoeuvre("brake", profile="brake", amp=0.5, noise=0.05), Manoeuvre("sine", profile="sine", amp=0.2, period=3.0),
          Manoeuvre("clean"), Manoeuvre("loud", noise=0.25)]
    table, noise, gauss = manoeuvre_table(conf, ms)
    assert table.dtype == np.float32 and table.shape == (7, T) and noise.dtype == np.float32 and noise.shape == (7,)
    assert gauss.dtype == np.bool_ and gauss.tolist() == [False] * 5 + [True, True]
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.int32)
    for k, (name, amp, period) in enumerate([("zero", None, 10.0), ("step", None, 10.0), ("ramp", 0.3, 10.0), ("brake", 0.5, 10.0),
                                             ("sine", 0.2, 3.0)]):
        assert np.array_equal(bits(table[k]), bits(scenarios.leader_profile(name, T, conf, amp, period))), name
    assert np.array_equal(bits(table), bits(tlo.profile_rows(conf, ms)))
    assert np.array_equal(bits(noise), bits([0, 0, 0, 0.05, 0, conf.reset_max_u, 0.25]))
    assert not table[5:].any()  # gaussian rows are unread
    assert table[1, T // 4] == np.float32(conf.reset_max_u) and table[3, T // 4] == np.float32(-0.5) and table[1, 0] == 0


def test_manoeuvre_table_refuses_a_short_episode():
    conf = config.Config(episode_sim_time=0.35)
    assert conf.steps_per_episode == 3
    with pytest.raises(ValueError, match="T=3: a scenario needs at least 4 steps"):
        manoeuvre_table(conf, [Manoeuvre("clean")])
    with pytest.raises(ValueError, match="T=3: a scenario needs at least 4 steps"):
        trainer.check_train_leader(conf, [Manoeuvre("clean")], "device", None, "platoon")


def test_assignment_crosses_levels_and_manoeuvres():
    for n_levels in (1, 3):
        for E in (1, 2):
            for n in (1, 2, 4):
                P = 2 * n * n_levels * E
                got = tlo.assignment(P, n, n_levels, E)
                for p, (lv, m) in enumerate(got):
                    q = p // E  # the solo run's platoon index
                    assert lv == q % n_levels and m == (q // n_levels) % n == scenarios.manoeuvre_of(q, n, n_levels)
                # every (level, manoeuvre) pair occurs, equally often, in each experiment
                for e in range(E):
                    mine = got[e::E]
                    assert {mine.count(pair) for pair in set(mine)} == {2} and len(set(mine)) == n * n_levels
    assert [m for _, m in tlo.assignment(8, 2, 1, 1)] == [0, 1, 0, 1, 0, 1, 0, 1]
    assert [m for _, m in tlo.assignment(8, 2, 3, 1)] == [0, 0, 0, 1, 1, 1, 0, 0]
    assert [m for _, m in tlo.assignment(8, 2, 1, 2)] == [0, 0, 1, 1, 0, 0, 1, 1]
    assert [m for _, m in tlo.assignment(14, 2, 3, 2)] == [0] * 6 + [1] * 6 + [0, 0]


def test_check_train_leader_refusals():
    ms = [Manoeuvre("clean"), Manoeuvre("brake", profile="brake", amp=0.5)]
    ok = lambda **kw: trainer.check_train_leader(kw.pop("conf", config.Config()), ms, kw.pop("rng", "device"), kw.pop("group", None),
                                                 kw.pop("auto_reset", "platoon"), **kw)
    assert ok() == ms and ok(auto_reset=False) == ms and ok(fused_step=True) == ms
    with pytest.raises(ValueError, match="leader manoeuvres needs the decentralized framework"):
        ok(conf=config.Config(framework="centralized"))
    with pytest.raises(ValueError, match="leader manoeuvres needs rng='device'"):
        ok(rng="host")
    with pytest.raises(ValueError, match=r"leader manoeuvres needs the fused step \(fused_step=False"):
        ok(fused_step=False)
    with pytest.raises(ValueError, match="does not combine with a hyperparameter sweep or PBT"):
        ok(hparams=[dict(actor_lr=1e-4)])
    with pytest.raises(ValueError, match="runs on one GPU: no process group"):
        ok(group=object())
    with pytest.raises(ValueError, match="auto_reset=True the conditional reset happens on the device"):
        ok(auto_reset=True)
    with pytest.raises(ValueError, match="0 manoeuvres listed"):
        trainer.check_train_leader(config.Config(), [], "device", None, "platoon")
    # the trainer refuses before it allocates: no GPU here, so anything past the check would fail differently
    with pytest.raises(ValueError, match="leader manoeuvres needs rng='device'"):
        trainer.VecTrainer(config.Config(num_platoons=2, pl_size=2), rng="host", train_leader=ms)
    with pytest.raises(ValueError, match="auto_reset=True the conditional reset"):
        trainer.VecTrainer(config.Config(num_platoons=2, pl_size=2), rng="device", auto_reset=True, train_leader=ms)


# ---- the entry points' host checks ------------------------------------------------------------------------------------------------
_B = lambda k: ctypes.c_void_p(0x1000 * (k + 1))  # non-null "device pointers" nothing reads: every call below is refused on the host
ENTRIES = ["avd_step_fused_lead_f32", "avd_step_fused_lead_seeds_f32", "avd_step_fused_dist_lead_f32", "avd_step_fused_dist_lead_seeds_f32"]


def _lead_call(entry, n=2, T=12, table=_B(40), noise=_B(41), gauss=_B(42), ep_len=_B(43), ep_step=0, n_levels=1, consts=_B(0)):
    head = [consts, 8, 2, 4, _B(1), _B(2), _B(3), None, _B(4), None, _B(5), None, None, _B(6), _B(7), _B(8), _B(9), 0.15, 0.0, 0.1, 0.2,
            -2.5, 2.5, 0.1, 0]
    key = [_B(10), 2] if "seeds" in entry else [7]
    tail = [3, 4, None, 8, 0, None]  # counters, no ring, no episodic reward counters
    dist = []
    if "dist" in entry:
        levels = (_hip.TrainLevel * n_levels)() if 1 <= n_levels <= 16 else (_hip.TrainLevel * 1)()
        dist = [n_levels, levels, _B(20), _B(21), _B(22), _B(23), None, None, 1]
    lead = [n, T, table, noise, gauss, ep_len, ep_step] + ([] if "dist" in entry else [n_levels])
    _hip.call(entry, *head, *key, *tail, *dist, *lead, None)


@pytest.mark.parametrize("entry", ENTRIES)
def test_lead_entry_points_refuse_on_the_host_before_any_hip_call(entry):
    refuse = lambda msg: pytest.raises(_hip.AvdError, match=rf"failed \(-1\): {entry}: {msg}")
    for arg in ("table", "noise", "gauss"):
        with refuse("null manoeuvre table, noise table or gaussian flags"):
            _lead_call(entry, **{arg: None})
    for n in (0, 17):
        with refuse(rf"n_manoeuvres={n} \(must be 1..16\)"):
            _lead_call(entry, n=n)
    with refuse(r"T=3 \(a manoeuvre needs at least 4 steps\)"):
        _lead_call(entry, T=3)
    for step in (12, -1):
        with refuse(rf"ep_step={step} with a null ep_len \(must be in \[0, T=12\)\)"):
            _lead_call(entry, ep_len=None, ep_step=step)
    with refuse(r"n_levels=0 \(must be (>= 1|1..16)\)"):
        _lead_call(entry, n_levels=0)
    # past the manoeuvre checks the step's own apply: a null constants block
    with refuse("null pointer"):
        _lead_call(entry, consts=None)
    with refuse("null pointer"):
        _lead_call(entry, ep_len=None, ep_step=11, consts=None)
    assert _hip.AVD_TRAIN_MAX_MANOEUVRES == scenarios.MAX_MANOEUVRES == 16
    assert "#define AVD_TRAIN_MAX_MANOEUVRES 16" in open(_hip.HEADER_PATH).read()


# every entry point of the fused step, by the parts of its argument list: (seed table, sweep table, levels, manoeuvres, residual law)
STEP_ENTRIES = {
    "avd_step_fused_f32": "", "avd_step_fused_seeds_f32": "s", "avd_step_fused_hp_f32": "sh", "avd_step_fused_dist_f32": "d",
    "avd_step_fused_dist_seeds_f32": "sd", "avd_step_fused_lead_f32": "l", "avd_step_fused_lead_seeds_f32": "sl",
    "avd_step_fused_dist_lead_f32": "dl", "avd_step_fused_dist_lead_seeds_f32": "sdl", "avd_step_fused_res_f32": "r"}


def test_step_entries_are_all_of_the_abi():
    assert sorted(STEP_ENTRIES) == sorted(n for n in _hip._PROTOS if n.startswith("avd_step_fused"))


@pytest.mark.parametrize("entry", STEP_ENTRIES)
def test_every_step_entry_point_reaches_the_common_check_under_its_own_name(entry):
    """Valid arguments of the entry point's own (so every check of its variant passes) and a platoon of 17: the step's own first check
    refuses it on the host, with the name of the entry point that was called."""
    parts = STEP_ENTRIES[entry]
    head = [_B(0), 8, 17, 4, _B(1), _B(2), _B(3), None, _B(4), None, _B(5), None, None, _B(6), _B(7), _B(8), _B(9)]
    head += [0.0, 0.1, -2.5, 2.5, 0.1, 0] if "h" in parts else [0.15, 0.0, 0.1, 0.2, -2.5, 2.5, 0.1, 0]
    key = [_B(10), _B(11), 2] if "h" in parts else [_B(10), 2] if "s" in parts else [7]
    mid = [3, 4, None, 8, 0, None]  # counters, no ring, no episodic reward counters
    levels = (_hip.TrainLevel * 2)()  # (host memory the level checks read: zeros, a perfect observation and no link)
    dist = [2, levels, _B(20), _B(21), _B(22), _B(23), None, None, 1]
    lead = [2, 12, _B(40), _B(41), _B(42), _B(43), 0]
    tail = (dist if "d" in parts else []) + (lead + ([] if "d" in parts else [1]) if "l" in parts else [])
    if "r" in parts:  # the one residual entry point, in its fullest form: seed table, levels, manoeuvres
        tail = [_B(10), 2] + dist + lead + [_B(50), 0.5, None]
    with pytest.raises(_hip.AvdError, match=rf"failed \(-1\): {entry}: P=8 L=17 S=4$"):
        _hip.call(entry, *head, *key, *mid, *tail, None)


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv,msg", [
    (["--rng", "host", "--train_leader", "brake"], "--train_leader needs --rng device"),
    (["--train_leader", "brake"], "--train_leader needs --rng device"),
    (["--rng", "device", "--episodes", "platoon", "--sweep", "actor_lr=1e-4,2e-4", "--train_leader", "brake"],
     "--train_leader does not combine with --sweep / --pbt"),
    (["--rng", "device", "--train_leader", "brake:speed=3"], "--train_leader: manoeuvre 'brake': unknown key 'speed'"),
    (["--rng", "device", "--train_leader", "clean:amp=1"], "--train_leader: manoeuvre 'clean': the gaussian profile takes neither amp nor period"),
    (["--rng", "device", "--train_leader", "a:profile=sine,period=0"], "--train_leader: manoeuvre 'a': period=0.0 must be > 0"),
    (["--rng", "device", "--train_leader", "brake", "--train_leader", "brake:amp=1"], r"--train_leader: manoeuvre\(s\) \['brake'\] listed more than once"),
    (["--rng", "device"] + [a for k in range(17) for a in ("--train_leader", f"m{k}")], "--train_leader: 17 manoeuvres listed: 1 to 16"),
])
def test_cli_argument_errors(argv, msg):
    import re

    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, "-m", "avddpg_amd", "tr", *argv], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and re.search(msg, out.stderr), out.stderr[-2000:]


def test_cli_refuses_more_than_one_rank(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), WORLD_SIZE="2")
    out = subprocess.run([sys.executable, "-m", "avddpg_amd", "tr", "--rng", "device", "--train_leader", "brake", "--out", str(tmp_path)],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--train_leader is not available under a process group of more than one rank" in out.stderr, out.stderr[-2000:]
