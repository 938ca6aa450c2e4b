"""Keeping the best actors seen, without a GPU: the oracle's own rules (tests/keep_best_oracle.py), the host copy of the score formula,
the mirrored launch constants, the CLI's and enable_keep_best's refusals, and everything avd_keep_best_f32 refuses on the host."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from avddpg_amd import _hip, config, params, trainer
from avddpg_amd import __main__ as cli
from tests import keep_best_oracle as kbo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---- the oracle's own rules ------------------------------------------------------------------------------------------------------
def test_score_is_the_sequential_float32_sum_from_the_first_element():
    # 1e8 swallows every +1 added to it one at a time; a pairwise sum (np.sum from 8 elements on) would keep some of them
    c = np.array([1e8] + [1.0] * 15, dtype=np.float32)
    assert kbo.score(c) == np.float32(np.float32(1e8) / np.float32(16))
    assert np.float32(np.sum(c)) != np.float32(1e8)
    # the order matters, and it is the memory order of [NS, M]
    c = np.array([[1.0, 1e8, -1e8], [3.0, 0.0, 0.0]], dtype=np.float32)
    assert kbo.score(c) == np.float32(3.0) / np.float32(6)
    assert kbo.score(c[::-1]) == np.float32(0.0)  # 3, 3, 3, 4, 1e8, 0
    assert kbo.score(np.float32([7.5])) == np.float32(7.5)
    rng = np.random.RandomState(3)
    for n in (2, 6, 15, 64):
        c = (rng.randn(n) * 100).astype(np.float32)
        s = np.float32(0) + c[0]
        for v in c[1:]:
            s = np.float32(s + v)
        assert bits(kbo.score(c)) == bits(np.float32(s / np.float32(n)))
        assert bits(trainer.sequential_mean_f32(c)) == bits(kbo.score(c))  # the package's host copy of the formula


def test_tie_nan_and_infinities():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    assert kbo.improves(-5.0, -inf) and not kbo.improves(-inf, -inf)  # the -inf start: any finite score improves, -inf does not
    assert not kbo.improves(-5.0, -5.0) and kbo.improves(np.nextafter(np.float32(-5), np.float32(0)), -5.0)  # strict
    assert not kbo.improves(nan, -inf) and not kbo.improves(nan, 3.0)  # NaN never improves
    assert kbo.improves(inf, 1e30) and not kbo.improves(inf, inf) and not kbo.improves(1e30, inf)
    assert np.isnan(kbo.score(np.float32([1, nan, 2]))) and kbo.score(np.float32([1, inf])) == inf
    assert np.isnan(kbo.score(np.float32([inf, -inf])))


def test_state_machine_keeps_the_older_snapshot_and_touches_nothing_else():
    M, A, C = 2, 8, 4
    rng = np.random.RandomState(0)
    theta = lambda: rng.randn(7, A + 5).astype(np.float32)
    stats = lambda: rng.randn(7, C + 3).astype(np.float32)
    sent_t, sent_s = np.full((3 * M, A), 7.0, np.float32), np.full((3 * M, C), 9.0, np.float32)
    kb = kbo.KeepBest(3, M, sent_t, sent_s)
    assert np.all(kb.best_score == -np.inf) and np.all(kb.best_step == -1) and kb.best_step.dtype == np.int64
    base = np.array([5, 0, 2])
    lvl = lambda *v: np.stack([np.full((2, M), x, np.float32) for x in v])
    th0, st0 = theta(), stats()
    assert kb.update(lvl(-5, np.nan, -np.inf), th0, st0, base, 10).tolist() == [1, 0, 0]
    assert np.array_equal(kb.best_theta[0:2], th0[5:7, :A]) and np.array_equal(kb.best_stats[0:2], st0[5:7, :C])
    assert np.all(kb.best_theta[2:] == 7.0) and np.all(kb.best_stats[2:] == 9.0)  # NaN and -inf: the sentinel stays
    assert kb.best_step.tolist() == [10, -1, -1] and kb.best_score[0] == -5 and np.all(kb.best_score[1:] == -np.inf)
    th1, st1 = theta(), stats()
    assert kb.update(lvl(-5, -3, np.inf), th1, st1, base, 20).tolist() == [0, 1, 1]  # tie: the older snapshot
    assert np.array_equal(kb.best_theta[0:2], th0[5:7, :A]) and np.array_equal(kb.best_theta[2:4], th1[0:2, :A])
    assert np.array_equal(kb.best_theta[4:6], th1[2:4, :A]) and kb.best_step.tolist() == [10, 20, 20]
    th2, st2 = theta(), stats()
    assert kb.update(lvl(-6, -2, np.inf), th2, st2, base, 30).tolist() == [0, 1, 0]  # worse; improve again; a tie at +inf
    assert kb.best_step.tolist() == [10, 30, 20] and np.array_equal(kb.best_stats[2:4], st2[0:2, :C])
    assert np.array_equal(sent_t, np.full((3 * M, A), 7.0, np.float32))  # the machine works on clones


# ---- the mirrored launch constants -----------------------------------------------------------------------------------------------
def test_launch_constants_mirror_the_kernel_source():
    src = open(os.path.join(ROOT, "avddpg_amd", "csrc", "best.hip")).read()
    num = lambda name: int(re.search(rf"constexpr \w+ {name} = (\d+);", src).group(1))
    assert (num("KEEP_THREADS"), num("KEEP_UNR"), num("KEEP_MAX_BLOCKS")) == (_hip.KEEP_THREADS, _hip.KEEP_UNR, _hip.KEEP_MAX_BLOCKS)
    assert "KEEP_CHUNK4 = KEEP_THREADS * KEEP_UNR;" in src and _hip.KEEP_CHUNK4 == _hip.KEEP_THREADS * _hip.KEEP_UNR
    assert "best.hip" in open(os.path.join(ROOT, "avddpg_amd", "csrc", "Makefile")).read()


# ---- the CLI's refusals ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv,msg", [
    (["--keep_best", "0"], "--keep_best: STEPS=0 must be >= 1"),
    (["--keep_best", "-40"], "--keep_best: STEPS=-40 must be >= 1"),
    (["--keep_best_seeds", "6"], "--keep_best_seeds needs --keep_best"),
    (["--keep_best", "40", "--keep_best_seeds", "6,6"], r"--keep_best_seeds: seed\(s\) \[6\] listed more than once"),
    (["--keep_best", "40", "--keep_best_seeds", "9-7"], "--keep_best_seeds: the range '9-7' runs backwards"),
    (["--keep_best", "forty"], "invalid int value"),
])
def test_cli_argument_errors(argv, msg, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        cli.get_cmdl_args(["tr", *argv], config.Config())
    assert e.value.code == 2 and re.search(msg, capsys.readouterr().err)


def test_cli_refuses_more_than_one_rank(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), WORLD_SIZE="2")
    out = subprocess.run([sys.executable, "-m", "avddpg_amd", "tr", "--keep_best", "40", "--out", str(tmp_path)], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--keep_best is not available under a process group of more than one rank" in out.stderr, out.stderr[-2000:]
    assert not os.listdir(tmp_path)


def test_parsed_flags_and_unchanged_defaults(monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    args, _ = cli.get_cmdl_args(["tr", "--keep_best", "40", "--keep_best_seeds", "6,8-9"], config.Config())
    assert args.keep_best == 40 and args.keep_best_seeds == [6, 8, 9]
    plain, pconf = cli.get_cmdl_args(["tr", "--pl_num", "3"], config.Config())
    flagged, fconf = cli.get_cmdl_args(["tr", "--pl_num", "3", "--keep_best", "40"], config.Config())
    assert plain.keep_best is None and plain.keep_best_seeds is None and flagged.keep_best_seeds is None
    assert {k: v for k, v in vars(plain).items() if k != "keep_best"} == {k: v for k, v in vars(flagged).items() if k != "keep_best"}
    assert pconf.__dict__ == fconf.__dict__ and not hasattr(fconf, "keep_best")


# ---- enable_keep_best's refusal ----------------------------------------------------------------------------------------------------
def test_enable_keep_best_refuses_a_process_group_of_more_than_one_rank():
    trainer.check_keep_best(1)
    with pytest.raises(ValueError, match="more than one rank"):
        trainer.check_keep_best(2)
    vt = object.__new__(trainer.VecTrainer)  # no GPU here: the refusal comes before anything is allocated or launched
    vt.world_size, vt._keep = 2, None
    with pytest.raises(ValueError, match="keeping the best actors runs on one rank"):
        vt.enable_keep_best()
    assert vt._keep is None
    for method in (lambda: vt.keep_best_update(0), vt.best_scores, vt.best_agents, vt.last_scores):
        with pytest.raises(ValueError, match="first"):
            method()


# ---- the entry point's host checks -------------------------------------------------------------------------------------------------
_B = lambda k: ctypes.c_void_p(0x1000 * (k + 1))  # non-null "device pointers" nothing reads: every call below is refused on the host
_PTRS = ("d_set_base", "counters", "theta", "stats", "best_theta", "best_stats", "best_score", "best_step", "improved")


def _keep_call(lay, n_units=3, M=2, NS=2, n_sets=8, h_base=(0, 6, 3), step=5, **ptrs):
    p = {k: _B(i) for i, k in enumerate(_PTRS)}
    h = None if h_base is None else (ctypes.c_int32 * max(1, len(h_base)))(*h_base)
    p.update(ptrs)
    _hip.call("avd_keep_best_f32", None if lay is None else ctypes.byref(lay), n_units, M, NS, n_sets, p["d_set_base"], h, p["counters"],
              p["theta"], p["stats"], step, p["best_theta"], p["best_stats"], p["best_score"], p["best_step"], p["improved"], None)


def test_entry_point_refuses_on_the_host_before_any_hip_call():
    """One fault per call, with status and message. No GPU here: a call that got past its checks would fail with a HIP error instead."""
    refuse = lambda msg: pytest.raises(_hip.AvdError, match=rf"failed \(-1\): avd_keep_best_f32: {msg}")
    lay = _hip.make_layout(4, 1, 256, 128, 48, 64)
    with refuse("null or empty layout"):
        _keep_call(None)
    with refuse("null or empty layout"):
        _keep_call(_hip.MlpLayout())
    for name in _PTRS:
        with refuse("null pointer"):
            _keep_call(lay, **{name: None})
    with refuse("null pointer"):
        _keep_call(lay, h_base=None)
    for name in ("theta", "stats", "best_theta", "best_stats"):
        for off in (4, 8, 12):
            with refuse("a slab pointer is not 16-byte aligned"):
                _keep_call(lay, **{name: ctypes.c_void_p(0x1000 + off)})
    for kw, got in ((dict(n_units=0), "n_units=0 M=2 NS=2"), (dict(n_units=-1), "n_units=-1 M=2 NS=2"), (dict(M=0), "n_units=3 M=0 NS=2"),
                    (dict(NS=0), "n_units=3 M=2 NS=0"), (dict(NS=-2), "n_units=3 M=2 NS=-2")):
        with refuse(rf"{got} \(each must be >= 1\)"):
            _keep_call(lay, **kw)
    with refuse("n_sets=1 holds no unit of M=2 sets"):
        _keep_call(lay, n_sets=1)
    for h, u, b in (((0, 7, 3), 1, 7), ((-1, 6, 3), 0, -1), ((0, 6, 2 ** 31 - 1), 2, 2 ** 31 - 1)):
        with refuse(rf"set_base\[{u}\]={b} is outside \[0, n_sets - M = 6\]"):
            _keep_call(lay, h_base=h)


def test_layout_spans_the_copy_relies_on():
    """The actor span and the actor's statistics are leading, 4-float aligned spans of a set's rows in every layout the tests use."""
    for dims in ((4, 1, 256, 128, 48), (4, 1, *params.padded_widths(1024, 1024, 48)), (3, 1, 64, 32, 16)):
        lay = _hip.make_layout(*dims, 64)
        assert lay.aW1 == 0 and lay.amm1 == 0 and 0 < lay.actor_size < lay.theta_size and 0 < lay.cmms < lay.stats_size
        assert lay.actor_size % 4 == 0 and lay.cmms % 4 == 0 and lay.theta_size % 4 == 0 and lay.stats_size % 4 == 0
        assert lay.cmms == 2 * (lay.H1 + lay.H2)  # moving mean and variance of the actor's two BN layers
