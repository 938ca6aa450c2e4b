"""Population-based training (VecTrainer.exploit / set_hparams, `tr --pbt`): one experiment's learner copied onto another's inside a
batch of interleaved experiments.

The entry point against a torch copy through views (both set arrangements, two layouts) and its refusals; whole runs with one forced
exploit against the plain sweep (every experiment that was not replaced) and against the same transfer done by hand; the CLI's
artefacts."""
import csv
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from avddpg_amd import _hip, params, pbt, trainer, vec
from avddpg_amd._hip import call, ptr, stream_handle

from tests.gpu_util import need_gpu
from tests.test_gpu_seed_batch import _conf, _deint, _eq

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SLABS = ("theta", "stats", "theta_t", "stats_t", "m", "v", "step")


# ---- 1. the entry point -------------------------------------------------------------------------------------------------------
def _slabs(lay, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    T, S = lay.theta_size, lay.stats_size
    rn = lambda w: torch.randn(n, w, generator=g, device="cuda")
    out = dict(theta=rn(T), stats=rn(S), theta_t=rn(T), stats_t=rn(S), m=rn(T), v=rn(T))
    out["step"] = torch.randint(0, 1 << 30, (n,), generator=g, device="cuda", dtype=torch.int32)
    return out


def _copy(lay, sl, n_groups, set_block, pairs, n_sets=None, **override):
    flat = [x for pr in pairs for x in pr]
    arr = (ctypes.c_int32 * max(1, len(flat)))(*flat)
    p = {k: ptr(t) for k, t in sl.items()}
    p.update(override)
    n_sets = sl["theta"].shape[0] if n_sets is None else n_sets
    call("avd_copy_experiment_sets_f32", ctypes.byref(lay), n_sets, n_groups, set_block, arr, len(pairs), p["theta"], p["stats"],
         p["theta_t"], p["stats_t"], p["m"], p["v"], p["step"], stream_handle())


def _reference(sl, n_groups, set_block, pairs):
    ref = {k: t.clone() for k, t in sl.items()}
    for s, d in pairs:
        for k, t in ref.items():
            view = t.view(-1, n_groups, set_block, *t.shape[1:])
            view[:, d] = sl[k].view(-1, n_groups, set_block, *t.shape[1:])[:, s]
    return ref


def _layouts():
    ref = _hip.make_layout(4, 1, 256, 128, 48, 64)
    wide = _hip.make_layout(4, 1, *params.padded_widths(1024, 1024, 48), 64)
    return [("reference", ref), ("hidden1024", wide)]


@pytest.mark.parametrize("arrangement", ["per_agent", "shared"])
def test_copy_experiment_sets_equals_torch_copy(arrangement):
    need_gpu()
    for name, lay in _layouts():
        E, M = (5, 3) if name == "reference" else (4, 2)
        blocks = 1 if arrangement == "shared" else 3  # per-agent sets: P platoons x E experiments x M vehicles
        n = blocks * E * M
        sl = _slabs(lay, n, 11)
        keep = {k: t.clone() for k, t in sl.items()}
        pairs = [(1, 0), (1, 3), (4, 2)] if E == 5 else [(2, 0), (3, 1)]
        want = _reference(keep, E, M, pairs)
        _copy(lay, sl, E, M, pairs)
        torch.cuda.synchronize()
        for k in _SLABS:
            _eq(sl[k], want[k], f"{name} {arrangement} {k}")
        dsts = {d for _, d in pairs}
        for k in _SLABS:  # every other set, and the step of every non-destination, bitwise unchanged
            for e in range(E):
                if e not in dsts:
                    _eq(_deint(sl[k], E, e, M), _deint(keep[k], E, e, M), f"{name} untouched {k} e={e}")
        del sl, keep, want
        torch.cuda.empty_cache()


def test_copy_experiment_sets_more_pairs_than_one_launch_holds():
    need_gpu()
    lay = _hip.make_layout(3, 1, 64, 32, 16, 64)
    E = 700
    sl = _slabs(lay, 2 * E, 5)
    keep = {k: t.clone() for k, t in sl.items()}
    pairs = [(e, e + 350) for e in range(300)]  # > 256 pairs: two launches
    _copy(lay, sl, E, 1, pairs)
    want = _reference(keep, E, 1, pairs)
    for k in _SLABS:
        _eq(sl[k], want[k], k)


def test_copy_experiment_sets_refusals_leave_every_slab_unchanged():
    need_gpu()
    lay = _hip.make_layout(4, 1, 256, 128, 48, 64)
    E, M = 4, 3
    sl = _slabs(lay, 2 * E * M, 3)
    keep = {k: t.clone() for k, t in sl.items()}
    cases = [
        (dict(pairs=[(0, 4)]), "outside"),
        (dict(pairs=[(-1, 2)]), "outside"),
        (dict(pairs=[(2, 2)]), "onto itself"),
        (dict(pairs=[(0, 1), (2, 1)]), "two pairs"),
        (dict(pairs=[(0, 1), (1, 2)]), "both a source and a destination"),
        (dict(pairs=[(1, 2), (0, 1)]), "both a source and a destination"),
        (dict(pairs=[(0, 1)], n_sets=2 * E * M - 1), "multiple"),
        (dict(pairs=[(0, 1)], n_groups=5), "multiple"),
        (dict(pairs=[(0, 1)], m=None), "null"),
        (dict(pairs=[(0, 1)], step=None), "null"),
        (dict(pairs=[(0, 1)], v=ctypes.c_void_p(sl["v"].data_ptr() + 4)), "aligned"),
    ]
    for kw, msg in cases:
        kw = dict(kw)
        pairs, n_groups = kw.pop("pairs"), kw.pop("n_groups", E)
        with pytest.raises(_hip.AvdError, match=msg):
            _copy(lay, sl, n_groups, M, pairs, **kw)
        torch.cuda.synchronize()
        for k in _SLABS:
            _eq(sl[k], keep[k], f"refused {pairs}: {k}")
    _copy(lay, sl, E, M, [])  # no pairs: nothing to do
    for k in _SLABS:
        _eq(sl[k], keep[k], f"no pairs: {k}")


# ---- 2. whole runs: one exploit mid-run -------------------------------------------------------------------------------------------
HPS = [dict(actor_lr=1e-4, critic_lr=2e-3), dict(actor_lr=3e-4, critic_lr=1e-3)]
SEEDS = (3, 9)
PAIRS = [(0, 3), (1, 2)]
EXPLOIT_AT, STEPS = 100, 180


def _exp(t, E, e, M):
    """Experiment e's slice of a tensor indexed by weight set or agent (set / agent j belongs to experiment (j // M) % E)."""
    return t.reshape(-1, E, M, *t.shape[1:])[:, e]


def _make(engine):
    fed, kw = ("normal", dict(fused_update=engine == "fused_update")) if engine in ("fused_update", "nofrl") else ("interfrl", {})
    if engine == "fused3":
        kw["shared_engine"] = "fused3"
    seeds = [k for _ in HPS for k in SEEDS]
    hps = [h for h in HPS for _ in SEEDS]
    return trainer.VecTrainer(_conf(fed, 8, 3), rng="device", auto_reset="platoon", seeds=seeds, hparams=hps, **kw)


def _losses(vt):
    return vt.set_losses if getattr(vt, "set_losses", None) is not None else vt.losses


def _same_experiment(a, b, e, what, ea=None):
    """Experiment e of trainer b against experiment ea (default e) of trainer a: learner, environment, noise, replay, counters."""
    ea = e if ea is None else ea
    E, M = a.E, a.M
    for n in _SLABS:
        _eq(_exp(getattr(a.agents, n), E, ea, M), _exp(getattr(b.agents, n), E, e, M), f"{what} {n} e={e}")
    if ea != e:
        return
    _eq(_exp(_losses(a), E, e, M), _exp(_losses(b), E, e, M), f"{what} losses e={e}")
    _eq(_deint(a.replay.ring, E, e, M), _deint(b.replay.ring, E, e, M), f"{what} replay e={e}")
    _eq(_deint(a.ou.state, E, e, M), _deint(b.ou.state, E, e, M), f"{what} ou e={e}")
    _eq(_deint(a.ep_reward, E, e), _deint(b.ep_reward, E, e), f"{what} ep_reward e={e}")
    for n in ("x", "prev_a", "ep_len", "done"):
        _eq(_deint(getattr(a.env, n), E, e), _deint(getattr(b.env, n), E, e), f"{what} env.{n} e={e}")
    for n in ("ret_sum", "len_sum", "count"):
        _eq(_deint(a.env.ep_stats[n], E, e), _deint(b.env.ep_stats[n], E, e), f"{what} ep_stats.{n} e={e}")


def _steps(vt, n):
    for _ in range(n):
        vt.step()


@pytest.mark.parametrize("engine", ["fused_update", "nofrl", "per_agent", "fused3"])
def test_exploit_continuation(engine):
    need_gpu()
    plain, auto, hand = _make(engine), _make(engine), _make(engine)
    E, M = plain.E, plain.M
    new_rows = [dict(r) for r in plain.hp_rows]
    for s, d in PAIRS:
        new_rows[d] = dict(plain.hp_rows[s], actor_lr=plain.hp_rows[s]["actor_lr"] * 1.2, critic_lr=plain.hp_rows[s]["critic_lr"] * 0.8)
    for vt in (plain, auto, hand):
        vt.reset_episode()
        _steps(vt, EXPLOIT_AT)
    assert plain.replay.samples > 0  # (the replay gate is open: every experiment has learned)
    auto.exploit(PAIRS)
    torch.cuda.synchronize()
    for s, d in PAIRS:  # right after the exploit the destination's learner is its source's
        _same_experiment(auto, auto, d, "just after the exploit", ea=s)
    auto.set_hparams(new_rows)
    # the same transfer by hand: a torch copy through views, the new values, and the next actions recomputed (the prefetch of a fused
    # update came from the old weights)
    ag = hand.agents
    for s, d in PAIRS:
        for n in _SLABS:
            t = getattr(ag, n)
            _exp(t, E, d, M).copy_(_exp(t, E, s, M).clone())
    hand._act_ready = False
    hand.set_hparams(new_rows)
    assert auto.experiment_conf(3).actor_lr == new_rows[3]["actor_lr"]
    for vt in (plain, auto, hand):
        _steps(vt, STEPS - EXPLOIT_AT)
    torch.cuda.synchronize()
    dsts = {d for _, d in PAIRS}
    for e in range(E):
        _same_experiment(auto, hand, e, "exploit vs by hand")
        if e not in dsts:
            _same_experiment(plain, auto, e, "not replaced vs plain sweep")
    per = [vt.env.pop_episode_stats(per_experiment=True) for vt in (plain, auto, hand)]
    sims = [vt.run_simulations() for vt in (plain, auto, hand)]
    for e in range(E):
        assert [p[0][e] for p in per[1:]] == [per[1][0][e]] * 2 and sims[1][e] == sims[2][e]
        if e not in dsts:
            assert per[0][0][e] == per[1][0][e] and per[0][2][e] == per[1][2][e] and sims[0][e] == sims[1][e]


def test_exploit_and_set_hparams_refusals():
    need_gpu()
    vt = trainer.VecTrainer(_conf("normal", 2, 3), rng="device", auto_reset="platoon", seeds=(1, 2))
    with pytest.raises(ValueError, match="sweep"):
        vt.set_hparams([{}, {}])
    solo = trainer.VecTrainer(_conf("normal", 2, 3), rng="device", auto_reset="platoon")
    with pytest.raises(ValueError, match="seed batch"):
        solo.exploit([(0, 1)])
    sw = _make("nofrl")
    before = sw.d_hp.clone()
    with pytest.raises(ValueError, match="tau"):
        sw.set_hparams([{}, {}, {"tau": 2.0}, {}])
    with pytest.raises(ValueError, match="rows for"):
        sw.set_hparams([{}])
    _eq(sw.d_hp, before, "refused set_hparams leaves the table")
    ptr_before = sw.d_hp.data_ptr()
    sw.set_hparams([dict(r) for r in sw.hp_rows])
    assert sw.d_hp.data_ptr() == ptr_before and sw.agents.hp[0] is sw.d_hp  # rewritten in place
    _eq(sw.d_hp, before, "the same values give the same table")
    keep = {n: getattr(sw.agents, n).clone() for n in _SLABS}
    with pytest.raises(_hip.AvdError, match="both a source"):
        sw.exploit([(0, 1), (1, 2)])
    for n in _SLABS:
        _eq(getattr(sw.agents, n), keep[n], f"refused exploit: {n}")


# ---- 3. the CLI ---------------------------------------------------------------------------------------------------------------
def _cli(args):
    r = subprocess.run([sys.executable, "-m", "avddpg_amd", "tr", *args], cwd=ROOT, capture_output=True, text=True, timeout=600,
                       env={**os.environ, "PYTHONPATH": ROOT})
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout.strip().splitlines()[-1]


COMMON = ["--rng", "device", "--episodes", "platoon", "--pl_num", "2", "--pl_size", "3", "--buffer_size", "400", "--report_every", "50",
          "--sweep", "actor_lr=5e-5,1e-4", "--sweep", "critic_lr=1e-3,2e-3", "--seeds", "4"]


def test_cli_pbt_without_a_generation_is_the_plain_sweep(tmp_path):
    need_gpu()
    a = _cli(COMMON + ["--total_time_steps", "150", "--out", str(tmp_path / "a")])
    b = _cli(COMMON + ["--total_time_steps", "150", "--pbt", "1000", "--out", str(tmp_path / "b")])
    assert open(os.path.join(a, "sweep.csv")).read() == open(os.path.join(b, "sweep.csv")).read()
    assert len(open(os.path.join(b, "pbt.csv")).read().strip().splitlines()) == 1  # the header only
    for label in os.listdir(a):
        d = os.path.join(a, label, "seed4")
        if not os.path.isdir(d):
            continue
        e = os.path.join(b, label, "seed4")
        for f in os.listdir(d):
            if f.endswith(".npz"):
                x, y = np.load(os.path.join(d, f)), np.load(os.path.join(e, f))
                assert all(np.array_equal(x[n], y[n]) for n in x.files), f
            elif f == "conf.json":
                cx, cy = json.load(open(os.path.join(d, f))), json.load(open(os.path.join(e, f)))
                assert dict(cy.pop("pbt"))["lineage"] == [] and cx == cy
            else:
                assert open(os.path.join(d, f)).read() == open(os.path.join(e, f)).read(), f


def test_cli_pbt_writes_a_consistent_lineage(tmp_path):
    need_gpu()
    base = _cli(COMMON + ["--total_time_steps", "400", "--pbt", "100", "--pbt_perturb", "0.5,2", "--out", str(tmp_path / "p")])
    rows = list(csv.DictReader(open(os.path.join(base, "pbt.csv"))))
    E, k = 4, 1
    assert [int(r["generation"]) for r in rows] == [g for g in (1, 2, 3) for _ in range(E)]
    assert [int(r["step"]) for r in rows[::E]] == [100, 200, 300]
    swept = ("actor_lr", "critic_lr")
    prev = {}
    for g in (1, 2, 3):
        gen = rows[(g - 1) * E:g * E]
        assert sorted(int(r["rank"]) for r in gen) == [1, 2, 3, 4]
        fit = [float(r["fitness"]) for r in gen]
        assert [int(r["rank"]) for r in gen] == [pbt.ranking(fit).index(e) + 1 for e in range(E)]
        kids = [r for r in gen if r["parent"] != ""]
        assert len(kids) == k
        for r in kids:
            par = gen[int(r["parent"])]
            assert int(par["rank"]) <= k and int(r["rank"]) > E - k
            for n in vec.HP_KEYS:
                if n in swept:
                    assert float(r[n]) in (float(par[n]) * 0.5, float(par[n]) * 2.0), (n, r[n], par[n])
                else:
                    assert float(r[n]) == float(par[n])
        for r in gen:  # the experiments that were not replaced keep their values
            if r["parent"] == "" and prev:
                assert all(float(r[n]) == prev[r["experiment"]][n] for n in vec.HP_KEYS)
        prev = {r["experiment"]: {n: float(r[n]) for n in vec.HP_KEYS} for r in gen}
    sweep = list(csv.DictReader(open(os.path.join(base, "sweep.csv"))))
    last = rows[2 * E:]
    for e, (s, r) in enumerate(zip(sweep, last)):
        assert s["label"] == r["label"] and int(s["seed"]) == int(r["seed"]) == 4
        assert all(float(s[n]) == float(r[n]) for n in vec.HP_KEYS)
        cj = json.load(open(os.path.join(base, r["label"], "seed4", "conf.json")))
        assert all(cj[n] == float(r[n]) for n in vec.HP_KEYS)
        p = dict(cj["pbt"])
        assert p["interval"] == 100 and p["fraction"] == 0.25 and p["perturb"] == [0.5, 2.0]
        lin = p["lineage"]
        assert [x["step"] for x in lin] == [100, 200, 300]
        for x, row in zip(lin, rows[e::E]):
            assert x["parent"] == (None if row["parent"] == "" else int(row["parent"]))
            assert all(x["values"][n] == float(row[n]) for n in vec.HP_KEYS)
