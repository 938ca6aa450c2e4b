"""World-size-2 gloo tests (CPU) of the multi-GPU host logic: platoon sharding, the interfrl gradient
exchange (all-reduce of per-vehicle-index partial sums) against the oracle's federated mean over ALL platoons,
and the any-terminal flag. The same code runs over RCCL on GPUs (backend "nccl")."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from avddpg_amd import dist as adist
from oracle import federated as ofed


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_shard_platoons_partitions_exactly():
    for total, world in ((32768, 8), (4096, 1), (10, 3), (7, 8)):
        spans = [adist.shard_platoons(total, world, r) for r in range(world)]
        assert spans[0][0] == 0 and spans[-1][1] == total
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        sizes = [hi - lo for lo, hi in spans]
        assert max(sizes) - min(sizes) <= 1
    assert adist.shard_platoons(32768, 8, 3) == (12288, 16384)
    with pytest.raises(ValueError):
        adist.shard_platoons(8, 2, 2)


def _worker(rank, world, port, P_total, M, n, weighted, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        rs = np.random.RandomState(0)  # every rank generates the full problem, uses its shard
        g = rs.normal(size=(P_total, M, n)).astype(np.float32)
        w = rs.uniform(0.5, 6.0, size=(P_total, M)).astype(np.float32)
        lo, hi = adist.shard_platoons(P_total, world, rank)
        gl, wl = g[lo:hi], w[lo:hi]
        # local partial sums (what avd_fed_sum_f32 produces on each GPU), fixed platoon order
        if weighted:
            out = torch.from_numpy((gl * wl[..., None]).sum(axis=0, dtype=np.float32))
            ws = torch.from_numpy(wl.sum(axis=0, dtype=np.float32))
        else:
            out, ws = torch.from_numpy(gl.sum(axis=0, dtype=np.float32)), None
        total = adist.total_platoons(hi - lo, dist.group.WORLD)  # reduced once (trainer construction)
        out0, ws0 = out.clone(), (None if ws is None else ws.clone())
        count = adist.exchange_fed_sums(out, ws, hi - lo, dist.group.WORLD, total=total)  # one collective, no host sync
        # the uncached form (count reduced inside) gives the same sums and count
        assert adist.exchange_fed_sums(out0, ws0, hi - lo, dist.group.WORLD) == count and torch.equal(out0, out)
        assert ws is None or torch.equal(ws0, ws)
        avg = (out * (1.0 / ws)[:, None]) if weighted else out / count  # avd_fed_finalize_f32
        flag = torch.tensor([1 if rank == 1 else 0], dtype=torch.int32)
        q.put((rank, count, avg.numpy(), adist.any_terminal(flag, dist.group.WORLD),
               adist.any_terminal(torch.zeros(1, dtype=torch.int32), dist.group.WORLD)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("weighted,world,P_total,M,n", [(False, 2, 7, 3, 1000), (True, 2, 7, 3, 1000),  # 7 platoons -> shards of 4 and 3: unequal on purpose
                                                        (False, 8, 32768, 5, 48), (True, 8, 32768, 5, 48)])  # BASELINE configs[3]: 32768 platoons x 5 over 8 ranks
def test_interfrl_exchange_matches_oracle_mean_over_all_platoons(weighted, world, P_total, M, n):
    """World 2 (unequal shards) and world 8 with configs[3]'s split -- shard_platoons(32768, 8): 4096 platoons x 5 vehicle indices
    per rank (VERDICT r03 #4c; `n` columns of the [M, theta] slab stand for all of them: the exchange is elementwise)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, P_total, M, n, weighted, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    if world == 8:
        assert [adist.shard_platoons(P_total, world, r) for r in range(world)] == [(4096 * r, 4096 * (r + 1)) for r in range(8)]
    rs = np.random.RandomState(0)
    g = rs.normal(size=(P_total, M, n)).astype(np.float32)
    w = rs.uniform(0.5, 6.0, size=(P_total, M)).astype(np.float32)
    if weighted:
        ref = ofed.get_weighted_avg_params([[[w[p, m] * g[p, m]] for p in range(P_total)] for m in range(M)],
                                           [float(w[:, m].sum()) for m in range(M)])
    else:
        ref = ofed.get_avg_params([[[g[p, m]] for p in range(P_total)] for m in range(M)])
    for rank, count, avg, any1, any0 in res:
        assert count == P_total and any1 is True and any0 is False
        for m in range(M):
            assert np.allclose(avg[m], ref[m][0], rtol=1e-5, atol=(1e-6 if world == 2 else 2e-5))  # (f32 sums of 32768 terms)
    for other in res[1:]:
        assert np.array_equal(res[0][2], other[2])  # every rank ends with the identical average (bit-equal weights)


class _Sets:
    def __init__(self, rank):
        g = torch.Generator().manual_seed(100 + rank)  # every rank starts from DIFFERENT values
        self.theta = torch.randn(5, 40, generator=g)[0:1].repeat(5, 1)
        self.stats = torch.randn(5, 8, generator=g)[0:1].repeat(5, 1)
        self.theta_t, self.stats_t = self.theta.clone(), self.stats.clone()


def _bcast_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        s = _Sets(rank)
        adist.broadcast_agents(s, dist.group.WORLD)
        q.put((rank, s.theta.numpy(), s.stats.numpy(), s.theta_t.numpy()))
    finally:
        dist.destroy_process_group()


def test_broadcast_agents_world2_gives_every_rank_rank0_weight_sets():
    """ranks must not keep rank-specific initial weights -- after broadcast_agents every set on every rank is
    rank 0's set 0 (the reference starts all agents from agent (0,0)'s weights, workers/trainer.py:121-131)."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_bcast_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in range(world)], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = _Sets(0)
    for rank, th, st, tht in res:
        assert np.array_equal(th, want.theta.numpy()) and np.array_equal(st, want.stats.numpy())
        assert np.array_equal(tht, want.theta_t.numpy())
    assert not np.array_equal(_Sets(1).theta.numpy(), want.theta.numpy())  # they did differ before


def test_bench_self_spawns_its_ranks_as_children_without_a_launcher():
    """`python bench.py --gpus N` with WORLD_SIZE unset must start the N ranks itself, as child processes of a parent
    that never touches the GPU (VERDICT r2 #1b). Probe mode: every child reports its rendezvous environment and exits
    before importing torch; a failing rank's exit code is the parent's."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env["AVD_BENCH_SPAWN_PROBE"] = "1"
    for n in (4, 8):  # 8: BASELINE configs[3]'s rank count
        p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(n)], env=env, capture_output=True, text=True,
                           timeout=120)
        assert p.returncode == 0, p.stderr
        lines = [l for l in p.stdout.splitlines() if l.strip()]
        assert len(lines) == 1  # rank 0 only
        got = json.loads(lines[0])
        assert got["RANK"] == "0" and got["LOCAL_RANK"] == "0" and got["WORLD_SIZE"] == str(n) and got["MASTER_ADDR"] == "127.0.0.1"
        assert int(got["MASTER_PORT"]) > 0
    env["AVD_BENCH_SPAWN_PROBE"] = "fail1"
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2"], env=env, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 3
    # self-certification: any AVD_* / AVDDPG_HIP_LIB override makes the bench refuse, before anything is spawned
    # or imported, unless --allow-diagnostics
    env2 = {k: v for k, v in env.items() if k != "AVD_BENCH_SPAWN_PROBE"}
    for var in ("AVD_FSPLIT_ONLY", "AVDDPG_HIP_LIB", "AVD_BENCH_ORDER"):
        p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "1"], env=dict(env2, **{var: "x"}),
                           capture_output=True, text=True, timeout=60)
        assert p.returncode != 0 and var in p.stderr and "allow-diagnostics" in p.stderr and not p.stdout.strip()
    # the parent must decide to spawn before importing torch (a process that initialised the GPU may not start ranks)
    src = open(os.path.join(root, "bench.py")).read()
    main_src = src[src.index("def main():"):]
    assert main_src.index("spawn_ranks(args)") < main_src.index("import torch")


def _two_phase_worker(rank, world, port, weighted, q):
    """exchange_two_phase on CPU tensors over gloo with dist.all_reduce wrapped by a recorder: the 'fake process group that records
    calls' of VERDICT r04 #3c is the real gloo group seen through the recorder, so the data path is exercised as well."""
    import time

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        M, A, T, P = 5, 24, 56, 3 + rank  # unequal shards
        g = torch.Generator().manual_seed(7 + rank)
        slab = torch.randn(M, T, generator=g)
        w = torch.rand(P, M, generator=g) + 0.5 if weighted else None
        wsum = w.sum(dim=0) if weighted else None
        scale = float(P) if wsum is None else wsum.view(M, 1)
        total = adist.total_platoons(P, dist.group.WORLD)
        # the single-collective form on a copy (exchange_fed_sums) = what the two-phase form must reproduce bit for bit
        one = slab.clone()
        ws1 = None if wsum is None else wsum.clone()
        one.mul_(scale if wsum is None else ws1.view(M, 1))
        tot = adist.exchange_fed_sums(one, ws1, P, dist.group.WORLD, total=total)
        one.div_(tot if ws1 is None else ws1.view(M, 1))
        calls, real = [], dist.all_reduce

        def recorder(t, *a, **kw):
            calls.append((int(t.numel()), bool(kw.get("async_op", False)), time.monotonic()))
            return real(t, *a, **kw)

        two = slab.clone()
        bufs = dict(crit=torch.empty(M, T - A), act=torch.empty(M * A + M))
        actor_started = []

        def actor_phase():  # ranks take DIFFERENT time between the two collectives: the order of issue must not depend on it
            actor_started.append(time.monotonic())
            time.sleep(0.4 * rank)

        dist.all_reduce = recorder
        try:
            adist.exchange_two_phase(two, A, scale, None if wsum is None else wsum.clone(), total, dist.group.WORLD, bufs, actor_phase)
        finally:
            dist.all_reduce = real
        q.put((rank, [(n, a) for n, a, _ in calls], calls[0][2] <= actor_started[0] <= calls[1][2], torch.equal(one, two), two.numpy()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("weighted", [False, True])
def test_two_phase_exchange_issues_its_collectives_in_the_same_order_on_every_rank(weighted):
    """VERDICT r04 #3c: the overlapped exchange (avddpg_amd/dist.py exchange_two_phase; workers/trainer.py:400-431 over platoon
    shards) issues critic block, then actor block (+ the [M] weight sums), both async, on EVERY rank and independently of how long
    a rank's actor phase takes -- what a NCCL / RCCL communicator needs -- and gives the bits of the single-collective form."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_two_phase_worker, args=(r, world, port, weighted, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in range(world)], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    M, A, T = 5, 24, 56
    want = [(M * (T - A), True), (M * A + (M if weighted else 0), True)]
    for rank, calls, crit_before_actor, same_bits, _ in res:
        assert calls == want, (rank, calls)
        assert crit_before_actor  # the critic block's collective is in flight before the actor phase starts
        assert same_bits
    assert np.array_equal(res[0][4], res[1][4])  # every rank ends with the identical average


def _slab_worker(rank, world, port, P_total, M, T, weighted, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        rs = np.random.RandomState(5)
        g = rs.normal(size=(P_total, M, T)).astype(np.float32)
        w = rs.uniform(0.5, 6.0, size=(P_total, M)).astype(np.float32)
        lo, hi = adist.shard_platoons(P_total, world, rank)
        gl, wl = g[lo:hi], w[lo:hi]
        total = adist.total_platoons(hi - lo, dist.group.WORLD)
        equal = abs(total - (hi - lo) * world) < 0.5
        buf, slab = adist.set_exchange_buffer(M, T, "cpu")
        assert slab.data_ptr() == buf.data_ptr() and buf.numel() == M * T + 1 + M
        out = []
        for step in range(3):  # the flag is this rank's any-terminal flag of the step: held by rank 1 only, at step 1 only
            if weighted:  # what the set learners leave: the LOCAL weighted mean per set
                ws = torch.from_numpy(wl.sum(axis=0, dtype=np.float32))
                slab.copy_(torch.from_numpy((gl * wl[..., None]).sum(axis=0, dtype=np.float32)) / ws[:, None])
            else:
                ws = None
                slab.copy_(torch.from_numpy(gl.mean(axis=0, dtype=np.float32)))
            flag = torch.tensor([1 if (rank == 1 and step == 1) else 0], dtype=torch.int32)
            adist.exchange_set_slab(buf, M, T, ws, hi - lo, total, dist.group.WORLD, flag=flag, equal_shards=equal)
            out.append((int(flag.item()), slab.clone().numpy(), None if ws is None else ws.numpy()))
        q.put((rank, equal, out))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("weighted,P_total", [(False, 8), (False, 7), (True, 7)])
def test_set_slab_exchange_carries_the_any_terminal_flag_to_every_rank(weighted, P_total):
    """the reference ends the episode of ALL platoons when any platoon is terminal (workers/trainer.py:268-269). In
    the throughput mode the rank's flag rides in the ONE gradient all-reduce of the step (dist.exchange_set_slab: slab | flag |
    weight sums) and comes back non-zero on every rank -- here only rank 1 holds a terminal platoon, at step 1 only, and BOTH ranks
    see the flag at that step and at no other; the slab comes back as the (weighted) mean over all platoons (equal shards: one
    scaling after the collective; unequal: mean -> sum -> mean), identical bits on both ranks."""
    world, M, T = 2, 3, 257
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_slab_worker, args=(r, world, port, P_total, M, T, weighted, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in range(world)], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    rs = np.random.RandomState(5)
    g = rs.normal(size=(P_total, M, T)).astype(np.float32)
    w = rs.uniform(0.5, 6.0, size=(P_total, M)).astype(np.float32)
    ref = ((g * w[..., None]).sum(axis=0) / w.sum(axis=0)[:, None]) if weighted else g.mean(axis=0)
    for rank, equal, out in res:
        assert equal == (P_total % world == 0)
        assert [f for f, _, _ in out] == [0, 1, 0]  # both ranks end the episode at step 1 -- and only there
        for _, slab, ws in out:
            assert np.allclose(slab, ref, rtol=1e-5, atol=1e-6)
            assert ws is None or np.allclose(ws, w.sum(axis=0), rtol=1e-6)
    for a, b in zip(res[0][2], res[1][2]):
        assert np.array_equal(a[1], b[1])  # identical bits on both ranks: the weight sets stay bit-identical
