"""Training under disturbances, the parts that need no GPU: the CLI flag, the refusals (before anything is allocated), the level
assignment, the level table's bytes, the entry points' argument checks, and that train_disturb=None makes nothing new."""
import ctypes as C

import numpy as np
import pytest

from avddpg_amd import __main__ as cli
from avddpg_amd import _hip, config, scenarios, trainer, vec
from avddpg_amd.scenarios import Disturbance
from tests import train_disturb_oracle as tdo


def _args(*extra):
    return cli.get_cmdl_args(["tr", "--rng", "device", "--episodes", "platoon", *extra], config.Config())[0]


def test_cli_parses_repeated_levels_and_a_bare_name_is_the_null_level():
    a = _args("--train_disturb", "clean", "--train_disturb", "rough:noise_ep=0.1,v2v_delay=2")
    assert [d.name for d in a.train_disturb] == ["clean", "rough"]
    clean, rough = a.train_disturb
    assert clean.sigma == (0.0, 0.0, 0.0) and not clean.uses_v2v and clean.dyn_coeff is None
    assert rough.noise_ep == 0.1 and rough.v2v_delay == 2 and rough.uses_v2v
    assert _args().train_disturb is None
    # composes with --seeds, --scenarios and --disturb
    a = _args("--train_disturb", "clean", "--seeds", "1,2", "--scenarios", "step", "--disturb", "lag:v2v_delay=2")
    assert a.seeds == [1, 2] and a.scenarios == ["step"] and [d.name for d in a.disturb] == ["lag"] and len(a.train_disturb) == 1
    conf = config.Config()
    cli._record_train_levels(conf, _args("--train_disturb", "clean", "--train_disturb", "rough:noise_ep=0.1,v2v_delay=2"))
    assert conf.train_disturbances == [["clean", Disturbance("clean").items()], ["rough", Disturbance("rough", noise_ep=0.1, v2v_delay=2).items()]]
    assert conf.train_disturbances[1][1][3] == ["v2v_delay", 2]  # (the shape of robustness_suite)
    plain = config.Config()
    cli._record_train_levels(plain, _args())
    assert not hasattr(plain, "train_disturbances")


@pytest.mark.parametrize("argv,msg", [
    (("--train_disturb", "nominal"), "--train_disturb: the disturbance name 'nominal' is reserved"),
    (("--train_disturb", "a:v2v_delay=16"), "--train_disturb: disturbance 'a': v2v_delay=16 must be an integer in 0..15"),
    (("--train_disturb", "a:bogus=1"), "--train_disturb: disturbance 'a': unknown key 'bogus'"),
    (("--train_disturb", "a", "--train_disturb", "a"), "--train_disturb: disturbance(s) ['a'] listed more than once"),
    (("--train_disturb", "a:v2v_drop=1.5"), "--train_disturb: disturbance 'a': v2v_drop=1.5 must be in [0, 1]"),
    (("--train_disturb", "a:noise_ep=-1"), "--train_disturb: disturbance 'a': noise_ep=-1.0 must be a finite number >= 0"),
    (("--train_disturb", "a", "--sweep", "tau=0.01,0.02"), "--train_disturb does not combine with --sweep / --pbt")])
def test_cli_refuses(argv, msg, capsys):
    with pytest.raises(SystemExit):
        _args(*argv)
    assert msg in capsys.readouterr().err


def test_cli_needs_the_device_rng(capsys):
    with pytest.raises(SystemExit):
        cli.get_cmdl_args(["tr", "--train_disturb", "a"], config.Config())
    assert "--train_disturb needs --rng device" in capsys.readouterr().err


def test_refusals_come_before_anything_is_allocated():
    """Every refusal is a ValueError of check_train_disturb; VecTrainer raises it first (no GPU on this path: nothing was allocated)."""
    lv = [Disturbance("a", noise_ep=0.1)]
    ok = dict(rng="device", group=None)
    assert [d.name for d in trainer.check_train_disturb(config.Config(), lv, **ok)] == ["a"]
    with pytest.raises(ValueError, match="decentralized"):
        trainer.check_train_disturb(config.Config(framework="centralized"), lv, **ok)
    with pytest.raises(ValueError, match="rng='device'"):
        trainer.check_train_disturb(config.Config(), lv, rng="host", group=None)
    with pytest.raises(ValueError, match="fused step"):
        trainer.check_train_disturb(config.Config(), lv, fused_step=False, **ok)
    with pytest.raises(ValueError, match="sweep"):
        trainer.check_train_disturb(config.Config(), lv, hparams=[{}], **ok)
    with pytest.raises(ValueError, match="process group"):
        trainer.check_train_disturb(config.Config(), lv, rng="device", group=object())
    with pytest.raises(ValueError, match="17 levels"):
        trainer.check_train_disturb(config.Config(), [Disturbance(f"l{k}") for k in range(17)], **ok)
    with pytest.raises(ValueError, match="0 levels"):
        trainer.check_train_disturb(config.Config(), [], **ok)
    assert len(trainer.check_train_disturb(config.Config(), [Disturbance(f"l{k}") for k in range(16)], **ok)) == 16
    with pytest.raises(ValueError, match="Model B"):  # check_disturbances applies unchanged
        trainer.check_train_disturb(config.Config(model="ModelA"), [Disturbance("lag", v2v_delay=1)], **ok)
    with pytest.raises(ValueError, match="reserved"):
        trainer.check_train_disturb(config.Config(), [Disturbance("nominal")], **ok)
    with pytest.raises(ValueError, match="more than once"):
        trainer.check_train_disturb(config.Config(), [Disturbance("a"), Disturbance("a")], **ok)
    for kw in (dict(rng="host"), dict(fused_step=False), dict(seeds=[1, 2], hparams=[{}, {}], auto_reset="platoon")):
        with pytest.raises(ValueError, match="training under disturbances"):
            trainer.VecTrainer(config.Config(num_platoons=2, pl_size=2), device="cpu", train_disturb=lv, **kw)
    with pytest.raises(ValueError, match="decentralized"):
        trainer.VecTrainer(config.Config(framework="centralized"), device="cpu", train_disturb=lv)


def test_level_assignment_rule_of_the_oracle_helper():
    """The rule the GPU tests hold the kernels to (tests/test_gpu_train_disturb.py: the mixed plant levels per platoon, the link levels,
    the seed batch against its solo runs): platoon p trains under level p % n_levels; in a batch of E interleaved experiments platoon
    g = p * E + e under its solo run's, p % n_levels."""
    assert [tdo.level_of(p, 3) for p in range(7)] == [0, 1, 2, 0, 1, 2, 0]
    E, n = 2, 3
    for g in range(12):
        e, p = vec.lane_of(g, E)
        assert tdo.level_of(g, n, E) == p % n and vec.batch_platoon(e, p, E) == g


def test_train_disturb_none_constructs_nothing_new():
    env = vec.VecPlatoon(4, 3, config.Config(pl_size=3), device="cpu", rng="device")
    assert env.levels is None
    for name in ("obs", "obs_prev", "link_hist", "link_recv", "d_levels", "h_levels", "d_plant", "obs_counter"):
        assert not hasattr(env, name), name
    assert env.agent_states() is env.x


def test_level_table_bytes_and_constants():
    assert C.sizeof(_hip.TrainLevel) == 32 and _hip.AVD_TRAIN_MAX_LEVELS == 16
    text = open(_hip.HEADER_PATH).read()
    assert "#define AVD_TRAIN_MAX_LEVELS 16" in text
    src = open(_hip.HEADER_PATH.replace("include/avddpg_hip.h", "avddpg_amd/csrc/common.h")).read()
    assert f"STREAM_TRAIN_OBS = {tdo.STREAM_TRAIN_OBS}," in src and f"STREAM_TRAIN_LINK = {tdo.STREAM_TRAIN_LINK}," in src
    lv = [Disturbance("clean"), Disturbance("r", noise_ep=0.1, noise_a=0.25, v2v_delay=3, v2v_drop=0.4)]
    arr, dev = vec.train_level_table(lv, "cpu")
    words = dev.numpy().view(np.uint32).reshape(2, 8)
    assert not words[0].any()
    assert np.array_equal(words[1, :3].view(np.float32), np.array([0.1, 0.0, 0.25], dtype=np.float32))
    assert words[1, 3] == 3 and words[1, 4] == scenarios.drop_threshold(0.4) == round(0.4 * 2 ** 24) and not words[1, 5:].any()
    assert bytes(arr) == dev.numpy().tobytes()


def _step_dist(n_levels, rows, link=True, P=4, L=3, S=4):
    """avd_step_fused_dist_f32 with a HOST level table and placeholder device pointers: every call here is refused by an argument check,
    ahead of any launch."""
    arr = (_hip.TrainLevel * max(1, len(rows)))()
    for r, (sg, delay, dq) in zip(arr, rows):
        r.sigma[0], r.delay, r.drop_q = sg, delay, dq
    fake = C.c_void_p(64)
    lk = fake if link else None
    _hip.call("avd_step_fused_dist_f32", fake, P, L, S, *([fake] * 13), 0.15, 0.0, 0.01, 0.02, -2.5, 2.5, 0.5, 0, 1, 0, 0, None, 0, 0, None,
              n_levels, arr, fake, fake, fake, fake, lk, lk, 1, None)


def test_entry_point_checks_its_arguments_without_a_launch():
    null = (0.0, 0, 0)
    for n, rows, msg in ((0, [null], r"n_levels=0 \(must be 1..16\)"), (17, [null], r"n_levels=17"),
                         (2, [null, (0.0, 16, 0)], r"level 1 delay=16 \(must be 0..15\)"), (1, [(0.0, -1, 0)], r"delay=-1"),
                         (1, [(0.0, 0, 2 ** 24 + 1)], r"drop_q=16777217 \(must be <= 2\^24"), (1, [(-0.5, 0, 0)], r"sigma\[0\]=-0.5"),
                         (1, [(float("inf"), 0, 0)], r"sigma\[0\]=inf"), (1, [(float("nan"), 0, 0)], r"sigma\[0\]=nan")):
        with pytest.raises(_hip.AvdError, match="avd_step_fused_dist_f32: .*" + msg):
            _step_dist(n, rows)
    with pytest.raises(_hip.AvdError, match="uses the V2V link .* but link_hist is null"):
        _step_dist(1, [(0.0, 2, 0)], link=False)
    with pytest.raises(_hip.AvdError, match=r"avd_step_fused_dist_f32: P=4 L=17 S=4"):  # the step's own checks follow
        _step_dist(1, [null], L=17)
    with pytest.raises(_hip.AvdError, match=r"S=5"):
        _step_dist(1, [null], S=5)
    fake = C.c_void_p(64)
    with pytest.raises(_hip.AvdError, match=r"avd_observe_f32: n_levels=17"):
        _hip.call("avd_observe_f32", 4, 3, fake, fake, 17, fake, None, None, 1, 0, None, None, None)
    with pytest.raises(_hip.AvdError, match=r"avd_observe_f32: P=4 L=17"):
        _hip.call("avd_observe_f32", 4, 17, fake, fake, 1, fake, None, None, 1, 0, None, None, None)
    with pytest.raises(_hip.AvdError, match=r"both be given or both be null"):
        _hip.call("avd_observe_f32", 4, 3, fake, fake, 1, fake, fake, None, 1, 0, None, None, None)
    with pytest.raises(_hip.AvdError, match=r"avd_observe_seeds_f32: d_seeds"):
        _hip.call("avd_observe_seeds_f32", 4, 3, fake, fake, 1, fake, None, None, None, 2, 0, None, None, None)
