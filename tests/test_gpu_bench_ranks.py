"""bench.py as the driver starts it for N > 1: self-spawned ranks, one all-reduce(sum) of the set gradients per step
(`workers/trainer.py:400-431` averaged over the platoon shards). On a one-GPU box the two ranks share the device over gloo
(RCCL refuses two ranks per device) and RCCL runs one rank; with two or more GPUs visible the same command runs over RCCL ("nccl")."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests.gpu_util import need_gpu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _bench(extra, gpus=2):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--mode", "interfrl", "--platoons", "256", "--buffer-size",
           "4096", "--steps", "6", "--warmup", "2", "--no-cpu-baseline"] + extra
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    env.pop("WORLD_SIZE", None), env.pop("RANK", None), env.pop("LOCAL_RANK", None), env.pop("MASTER_PORT", None)
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]  # rank 0 prints ONE line
    return json.loads(lines[0])


def test_two_ranks_on_one_gpu_over_gloo():
    need_gpu()
    out = _bench(["--backend", "gloo", "--single-device"])
    assert out["n_gpus"] == 2 and out["value"] > 0 and out["scaling"] == "weak" and out["config"]["platoons_per_gpu"] == 256
    assert out["collective_backend"] == "gloo" and "all-reduce" in out["config"]["parallelism"]


def test_two_ranks_over_rccl_when_two_gpus_are_visible():
    """The same command over RCCL. With two or more GPUs visible: two ranks, one per GPU. With one GPU, where RCCL refuses two ranks per
    device ("Duplicate GPU detected"), its one rank runs through a real RCCL communicator (--one-rank-rccl): every collective of the
    N > 1 interfrl path goes through RCCL on the device, timed in both of its forms with --full (the two-rank data path: over gloo
    above and in tests/test_dist_cpu.py)."""
    need_gpu()
    if torch.cuda.device_count() >= 2:
        out = _bench(["--backend", "nccl"])
        assert out["n_gpus"] == 2 and out["value"] > 0 and out["rccl_ranks"] == 2 and out["collective_backend"] == "nccl"
        return
    out = _bench(["--full", "--one-rank-rccl", "--master-port", str(_free_port())], gpus=1)
    assert out["n_gpus"] == 1 and out["value"] > 0 and out["rccl_ranks"] == 1 and out["collective_backend"] == "nccl"
    col = out["collective"]
    assert col["per_step_ms"] > 0 and out["stages_ms"]["allreduce"] == col["per_step_ms"] and col["overlapped"] is False
    assert set(col["forms"]) == {"single", "overlapped"} and all(f["stages_ms"]["allreduce"] > 0 for f in col["forms"].values())


@pytest.mark.parametrize("mode", ["interfrl", "nofrl"])
def test_dumped_outputs_of_the_last_timed_step_repeat_bit_for_bit(tmp_path, mode):
    """--dump-outputs DIR: what the last timed step of the primary workload computed, as float32 .npy files of at most 64 MB in all,
    the same bits in two runs of the same arguments although the wall-clock prewarm runs a different number of steps in each (the
    timed steps start on a new trainer). nofrl's per-agent slabs are over their share and written as a seeded sample."""
    need_gpu()
    import numpy as np

    outs = []
    for run in ("a", "b"):
        d = tmp_path / run
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--mode", mode, "--platoons", "256", "--buffer-size", "4096",
               "--steps", "7", "--warmup", "3", "--prewarm-seconds", "0.3", "--no-cpu-baseline", "--dump-outputs", str(d)]
        env = dict(os.environ)
        for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
            env.pop(k, None)
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, p.stdout[-2000:]
        out = json.loads(lines[0])
        assert out["steps"] == 7 and out["ms_per_step"] > 0 and out["prewarm"]["steps"] > 0
        arrays = out["dump_outputs"]["arrays"]
        files = sorted(os.listdir(d))
        assert files == sorted(f"{k}.npy" for k in arrays)
        assert {"actions", "states", "rewards", "losses", "theta", "theta_target"} | ({"grads"} if mode == "interfrl" else set()) <= set(arrays)
        assert sum(os.path.getsize(d / f) for f in files) <= 64e6
        got = {f: np.load(d / f) for f in files}
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
        assert np.abs(got["losses.npy"]).max() > 0 and (mode == "nofrl" or np.abs(got["grads.npy"]).max() > 0)
        if mode == "nofrl":
            assert arrays["theta"]["elements"] < np.prod(arrays["theta"]["shape"])
        outs.append(got)
    assert all(np.array_equal(outs[0][f], outs[1][f]) for f in outs[0]), [f for f in outs[0] if not np.array_equal(outs[0][f], outs[1][f])]


def test_plain_one_gpu_run_times_the_primary_workload_only():
    """A plain run (`python bench.py --gpus 1 --steps K --warmup W`, no --full) does only what its headline figure needs: the primary
    workload, no second workload, no CPU baseline, no other configs -- and its line still says what the headline is."""
    need_gpu()
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--platoons", "256", "--buffer-size", "4096", "--steps", "4",
           "--warmup", "2", "--prewarm-seconds", "0.2"]
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["primary_mode"] == "interfrl" and out["n_gpus"] == 1 and out["steps"] == 4 and out["warmup"] == 2
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["higher_is_better"] is True and out["unit"] == "env-steps/s"
    assert abs(out["value"] - 256 * 1e3 / out["ms_per_step"]) < 1e-6 * out["value"]
    assert "also_measured" not in out and "cpu_baseline" not in out


def test_default_one_gpu_run_carries_every_single_gpu_baseline_config():
    """The driver's command with --full (`python bench.py --gpus 1 --steps K --warmup W --full`) times configs[1] in both federated modes AND
    configs[2] (4096 x 10, both modes, replay capacity 100000) AND configs[4] (hidden 1024) in ONE line: `value` stays
    configs[1] interfrl, the others sit under also_measured with their own roofline. Full sizes (82 + 164 GB rings): about a minute."""
    need_gpu()
    if torch.cuda.get_device_properties(0).total_memory < 250 * 2**30:
        pytest.skip("needs the 288 GB of an MI355X (4096 x 10 at replay capacity 100000)")
    sys.path.insert(0, ROOT)
    import bench

    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--prewarm-seconds", "0.2",
           "--no-cpu-baseline", "--full"]
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["primary_mode"] == "interfrl" and out["config"]["pl_size"] == 5 and out["value"] > 0 and out["n_gpus"] == 1
    also = out["also_measured"]
    assert set(also) == {"nofrl"} | set(bench.EXTRA_CONFIGS)
    for k, name in bench.EXTRA_CONFIGS.items():
        r = also[k]
        assert r["value"] > 0 and r["steps"] == 4 and r["config"]["baseline_config"] == name
        assert r["roofline"]["bound"] in ("hbm", "mfma") and 0 < r["roofline"]["frac"] < 1
    assert also["config3_interfrl"]["config"]["pl_size"] == 10 and also["config3_nofrl"]["config"]["mode"] == "nofrl"
    assert "hidden=1024" in also["config5"]["config"]["workload"] and also["config5"]["roofline"]["unit"] == "TFLOP/s"
