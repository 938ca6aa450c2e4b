"""The gain search on the device (avd_search_sample_f32 / avd_search_refit_f32, csrc/search.hip; evaluator.search_linear;
--baseline_search, --residual searched). Yardsticks: tests/search_oracle.py -- the sample within the project's device-vs-libm Box-Muller
allowance (2e-5 of the dimension's std; == where no normal enters), the refit with == on every output --, scenarios.fitness_of on a plain
linear-evaluator launch with == for the traced fitness, evaluator.tune_linear for the grid's pick, and the CLI's files."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from avddpg_amd import __main__ as cli
from avddpg_amd import _hip, config, evaluator, scenarios
from avddpg_amd._hip import ptr
from avddpg_amd.scenarios import Disturbance, SearchSpace
from tests import search_oracle as so
from tests.gpu_util import need_gpu

pytestmark = pytest.mark.gpu

F = np.float32
SEED = 2 ** 32 + 6   # (the high word of a 64-bit seed reaches the key)
TOL = 2e-5           # x the dimension's std: tests/test_gpu_replay.py's Box-Muller allowance, 2e-6 at scale 0.1
SENTINEL = -777.25
NAMES, SEEDS, T = ["step", "sine"], [6, 7], 40
SUITE = dict(scenarios=NAMES, seeds=SEEDS, manual_timestep_override=T)


def _dev(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x)).to(device="cuda", dtype=dtype).contiguous()


def _same(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    assert np.array_equal(got, ref, equal_nan=True), (what, got, ref)


def _check_sample(got, G, L, R, mean, std, lo, hi, seed, gen, what):
    """got [G, L, 4] against the oracle's sample from (mean, std): == for candidate 0, frozen dimensions and entries the oracle clips by
    more than the tolerance; every other entry within TOL * std[d]. -> the number of entries compared with a tolerance."""
    x, raw = so.sample(G, L, R, mean, std, lo, hi, seed, gen)
    rows = lambda t: np.repeat(np.asarray(t, dtype=F).reshape(R, 4), L, axis=0) if R == 1 else np.asarray(t, dtype=F).reshape(R, 4)
    sd, l, h = rows(std)[None], rows(lo)[None], rows(hi)[None]
    tol = (TOL * sd).astype(F)
    exact = (np.arange(G)[:, None, None] == 0) | (sd == 0) | (raw < l - tol) | (raw > h + tol)
    exact = np.broadcast_to(exact, x.shape)
    assert got.shape == x.shape and got.dtype == F
    assert np.array_equal(got[exact], x[exact]), (what, "exact entries")
    err = np.abs(got.astype(np.float64) - x)
    assert np.all(err <= np.broadcast_to(tol, x.shape)), (what, float((err / np.maximum(np.broadcast_to(sd, x.shape), 1e-30)).max()))
    assert np.all(got >= l) and np.all(got <= h)
    if R == 1:
        for v in range(1, L):
            assert np.array_equal(got[:, v], got[:, 0]), (what, "tied rows")
    return int((~exact).sum())


# ---- 1. the sample kernel ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [1, 3, 5])
def test_sample_kernel_against_the_oracle(L):
    need_gpu()
    rng = np.random.RandomState(L)
    toleranced = 0
    for R in sorted({1, L}):
        lo = np.tile(F([0.0, 0.0, -1.0, 0.0]), (R, 1))
        hi = np.tile(F([3.0, 4.0, 0.0, 1.0]), (R, 1))
        mean = (lo + (hi - lo) * rng.uniform(0.2, 0.8, (R, 4))).astype(F)
        std = ((hi - lo) / 2 * rng.uniform(0.5, 1.0, (R, 4))).astype(F)  # wide: the clip binds on many entries
        std[0, 3] = 0.0                                                   # a frozen dimension (its mean is no bound)
        d = [_dev(t) for t in (mean, std, lo, hi)]
        for G in (1, 37, 257):
            for gen in (0, 3):
                n = G * L * 4
                out = torch.full((n + 64,), SENTINEL, dtype=torch.float32, device="cuda")
                _hip.call("avd_search_sample_f32", G, L, R, *[ptr(t) for t in d], SEED, gen, ptr(out), _hip.stream_handle())
                got = out.cpu().numpy()
                assert np.all(got[n:] == F(SENTINEL)), "written past [G][L][4]"
                got = got[:n].reshape(G, L, 4)
                _same(got[0], np.repeat(mean, L, axis=0) if R == 1 and L > 1 else mean, "candidate 0 is the mean")
                assert np.all(got[:, :, 3].reshape(G, L)[:, 0] == mean[0, 3])
                toleranced += _check_sample(got, G, L, R, mean, std, lo, hi, SEED, gen, (G, L, R, gen))
        # the generation and both seed words select the draw
        a, b, c = (torch.empty(37 * L * 4, dtype=torch.float32, device="cuda") for _ in range(3))
        for out, seed, gen in ((a, SEED, 0), (b, SEED, 1), (c, 6, 0)):
            _hip.call("avd_search_sample_f32", 37, L, R, *[ptr(t) for t in d], seed, gen, ptr(out), _hip.stream_handle())
        assert not torch.equal(a, b) and not torch.equal(a, c)
    assert toleranced > 1000  # (most entries carry a normal: the comparison is not all candidate 0 and clips)


# ---- 2. the refit ------------------------------------------------------------------------------------------------------------------------

def _refit_dev(G, L, R, n_elite, alpha, gains, f, min_std, mean, std, best_gains, best_fitness, best_gen, generation):
    """One avd_search_refit_f32 call on copies of the inputs -> the oracle's dict of outputs."""
    t = dict(gains=_dev(gains), f=_dev(f), min_std=_dev(min_std), mean=_dev(mean), std=_dev(std), best_gains=_dev(best_gains),
             best_fitness=_dev(F([best_fitness])), best_gen=_dev(np.int32([best_gen]), torch.int32),
             elite=torch.full((n_elite + 16,), -5, dtype=torch.int32, device="cuda"),
             hist=torch.full((4 + 16,), SENTINEL, dtype=torch.float32, device="cuda"))
    _hip.call("avd_search_refit_f32", G, L, R, n_elite, float(alpha), ptr(t["gains"]), ptr(t["f"]), ptr(t["min_std"]), ptr(t["mean"]),
              ptr(t["std"]), ptr(t["best_gains"]), ptr(t["best_fitness"]), ptr(t["best_gen"]), generation, ptr(t["elite"]), ptr(t["hist"]),
              _hip.stream_handle())
    elite, hist = t["elite"].cpu().numpy(), t["hist"].cpu().numpy()
    assert np.all(elite[n_elite:] == -5) and np.all(hist[4:] == F(SENTINEL)), "written past elite_idx / history_row"
    assert np.array_equal(t["gains"].cpu().numpy(), np.asarray(gains, dtype=F)) and np.array_equal(t["f"].cpu().numpy(), f, equal_nan=True)
    return dict(mean=t["mean"].cpu().numpy(), std=t["std"].cpu().numpy(), best_gains=t["best_gains"].cpu().numpy(),
                best_fitness=t["best_fitness"].cpu().numpy()[0], best_gen=int(t["best_gen"].cpu()[0]), elite_idx=elite[:n_elite],
                history_row=hist[:4])


def _same_refit(got, ref, what):
    for k in ("mean", "std", "best_gains", "elite_idx", "history_row"):
        _same(got[k], ref[k], (what, k))
    assert got["best_gen"] == ref["best_gen"], (what, "best_gen", got["best_gen"], ref["best_gen"])
    _same(F(got["best_fitness"]), F(ref["best_fitness"]), (what, "best_fitness"))


def _fitness(kind, G, rng):
    f = (-5 + rng.standard_normal(G)).astype(F)
    if kind == "ties":  # blocks of exact ties, the best value among them
        f = np.round(f).astype(F)
        f[rng.permutation(G)[:max(2, G // 3)]] = f.max()
    elif kind == "nans":
        f[rng.permutation(G)[:max(1, G // 4)]] = np.nan
    elif kind == "few_valid":  # fewer valid candidates than any n_elite > 1
        keep = rng.permutation(G)[0]
        v = f[keep]
        f[:] = np.nan
        f[keep] = v
    elif kind == "all_nan":
        f[:] = np.nan
    return f


@pytest.mark.parametrize("kind", ["distinct", "ties", "nans", "few_valid", "all_nan"])
@pytest.mark.parametrize("G", [2, 257, 1000])
def test_refit_is_bit_identical_to_the_oracle(G, kind):
    """Every output with ==: sqrtf and the divisions are correctly rounded under the build's flags (HIP's default), so the oracle's
    float32 statement is the device's, bit for bit."""
    need_gpu()
    rng = np.random.RandomState(G * 7 + len(kind))
    for L, R in ((5, 5), (3, 1)):
        gains = (rng.standard_normal((G, L, 4)) * [1.5, 2.0, 0.5, 0.5] + [1.5, 2.0, -0.5, 0.5]).astype(F)
        mean, std = rng.uniform(-1, 2, (R, 4)).astype(F), rng.uniform(0.1, 1, (R, 4)).astype(F)
        std[0, 3] = 0.0        # a frozen dimension
        min_std = np.full((R, 4), 1e-3, F)
        min_std[0, 0] = 5.0    # a floor that binds
        f = _fitness(kind, G, rng)
        for n_elite in sorted({1, 2, G}):
            for alpha in (1.0, 0.7):
                what = (kind, G, L, R, n_elite, alpha)
                start = (np.zeros((R, 4), F), F(-np.inf), -1)
                ref = so.refit(G, L, R, n_elite, alpha, gains, f, min_std, mean, std, *start, 3)
                got = _refit_dev(G, L, R, n_elite, alpha, gains, f, min_std, mean, std, *start, 3)
                _same_refit(got, ref, what)
                if kind == "all_nan":
                    assert ref["E"] == 0 and got["best_gen"] == -1 and got["history_row"][3] == 0 and np.isnan(got["history_row"][0])
                    _same(got["mean"], mean, (what, "mean stays")), _same(got["std"], std, (what, "std stays"))
                    continue
                assert got["best_gen"] == 3 and got["history_row"][3] == ref["E"] == min(n_elite, int((~np.isnan(f)).sum()))
                assert got["std"][0, 3] == 0 and got["mean"][0, 3] == mean[0, 3] and got["std"][0, 0] == 5.0
                if kind == "ties":  # the tied best candidates enter in index order
                    top = np.flatnonzero(f == f.max())
                    assert got["elite_idx"][:min(n_elite, top.size)].tolist() == top[:n_elite].tolist()
                # a second generation on the state the first left: a lower best and an equal best leave the record alone, a higher one takes it
                state = (got["mean"], got["std"], got["best_gains"], got["best_fitness"], got["best_gen"])
                best = np.nanmax(f)
                for delta, moved in ((-0.5, False), (0.0, False), (0.25, True)):
                    f2 = np.where(np.isnan(f), f, np.minimum(f, best - 1)).astype(F)
                    f2[G - 1] = best + F(delta)
                    ref2 = so.refit(G, L, R, n_elite, alpha, gains, f2, min_std, *state, 4)
                    got2 = _refit_dev(G, L, R, n_elite, alpha, gains, f2, min_std, *state, 4)
                    _same_refit(got2, ref2, (what, "second", delta))
                    assert (got2["best_gen"] == 4) == moved and got2["history_row"][2] == (f2[G - 1] if moved else best)
                    if not moved:
                        _same(got2["best_gains"], got["best_gains"], (what, "best_gains stay", delta))


# ---- 3. end to end -----------------------------------------------------------------------------------------------------------------------

def _space(model, per_vehicle, **kw):
    bounds = dict(kp=(0, 3), kv=(0, 4), ka=(-1, 0))
    if model == "ModelB":
        bounds["kf"] = (0, 1)
    return SearchSpace(bounds, pop=64, gens=4, elite=0.125, seed=SEED, per_vehicle=per_vehicle, **kw)


def _fitness_of_plain_launch(conf, gains, levels=()):
    b = evaluator.LinearBatch(conf, gains, NAMES, list(levels), SEEDS, None, 10.0, T, metrics=False)
    b.launch()
    return scenarios.fitness_of(b.counters.cpu().numpy())


def _check_trace(conf, space, res, levels=()):
    """Every generation of a traced search against the oracle and a plain launch; the best-ever record against the trace."""
    L, G, gens, n_elite = conf.pl_size, space.pop, space.gens, space.n_elite()
    R = space.rows(L)
    lo, hi, mean0, std0, min_std = space.tables(L)
    tr = res.trace
    assert tr["gains"].shape == (gens, G, L, 4) and tr["fitness"].shape == (gens, G) and tr["elite_idx"].shape == (gens, n_elite)
    assert tr["mean"].shape == tr["std"].shape == (gens, R, 4) and res.history.shape == (gens, 4) and res.history.dtype == F
    _same(tr["mean"][0], mean0, "start mean"), _same(tr["std"][0], std0, "start std")
    best = (np.zeros((R, 4), F), F(-np.inf), -1)
    for g in range(gens):
        _check_sample(tr["gains"][g], G, L, R, tr["mean"][g], tr["std"][g], lo, hi, space.seed, g, ("generation", g))
        _same(tr["fitness"][g], _fitness_of_plain_launch(conf, tr["gains"][g], levels), ("fitness", g))
        ref = so.refit(G, L, R, n_elite, space.alpha, tr["gains"][g], tr["fitness"][g], min_std, tr["mean"][g], tr["std"][g], *best, g)
        _same(tr["elite_idx"][g], ref["elite_idx"], ("elite_idx", g))
        _same(res.history[g], ref["history_row"], ("history", g))
        nxt = (tr["mean"][g + 1], tr["std"][g + 1]) if g + 1 < gens else (res.mean, res.std)
        _same(nxt[0], ref["mean"], ("mean after", g)), _same(nxt[1], ref["std"], ("std after", g))
        best = (ref["best_gains"], ref["best_fitness"], ref["best_gen"])
    assert np.isfinite(tr["fitness"]).all()
    # the returned law: the first arg-max over all generations, in generation-then-index order
    at = scenarios.first_argmax(tr["fitness"].reshape(-1))
    gen, i = divmod(at, G)
    assert at == int(np.argmax(tr["fitness"].reshape(-1))) and res.generation == gen == best[2]
    _same(F(res.fitness), tr["fitness"][gen, i], "best fitness")
    table = res.law.gains(L)
    _same(table, tr["gains"][gen, i], "best table"), _same(res.best_gains, tr["gains"][gen, i, :R], "best rows")
    assert res.law.name == "searched" and np.all(np.diff(res.history[:, 2]) >= 0) and res.history[-1, 2] == F(res.fitness)
    assert np.all(res.history[:, 3] == n_elite)
    _same(_fitness_of_plain_launch(conf, table[None], levels)[0], F(res.fitness), "a fresh batch on the returned table")
    return tr


@pytest.mark.parametrize("per_vehicle", [True, False])
@pytest.mark.parametrize("model,L", [("ModelA", 3), ("ModelB", 5)])
def test_search_end_to_end_every_generation_against_the_oracle(model, L, per_vehicle):
    need_gpu()
    conf = config.Config(pl_size=L, model=model)
    space = _space(model, per_vehicle)
    res = evaluator.search_linear(conf, space, trace=True, **SUITE)
    assert (res.pop, res.gens, res.n_elite, res.K) == (64, 4, 8, 4)
    tr = _check_trace(conf, space, res)
    if model == "ModelA":
        assert np.all(tr["gains"][..., 3] == 0) and np.all(res.std[:, 3] == 0)  # kf frozen at 0
    if not per_vehicle:
        assert res.mean.shape == (1, 4) and all(np.array_equal(res.law.table[v], res.law.table[0]) for v in range(L))
    else:
        assert len({tr["gains"][1, 5, v].tobytes() for v in range(L)}) == L  # every vehicle draws its own row
    assert res.history[-1, 2] >= tr["fitness"][0, 0]  # never below the midpoint it starts from (candidate 0 of generation 0)
    # the same search without the trace: the same result
    plain = evaluator.search_linear(conf, space, **SUITE)
    assert plain.trace is None and plain.fitness == res.fitness and plain.generation == res.generation
    _same(plain.history, res.history, "history"), _same(plain.law.table, res.law.table, "table")


def test_search_from_the_grids_pick_is_never_below_it():
    """Candidate 0 of generation 0 is the start mean, here the grid's best law: a guarantee, not a measurement."""
    need_gpu()
    conf = config.Config(pl_size=5)
    grid = scenarios.parse_gain_grid("kp=0:2:3,kv=0:4:3,ka=-0.5:0:2")
    best, fit = evaluator.tune_linear(conf, grid, **SUITE)
    for per_vehicle in (True, False):
        space = SearchSpace(dict(kp=(0, 2), kv=(0, 4), ka=(-0.5, 0)), pop=64, gens=4, seed=SEED, per_vehicle=per_vehicle, init=grid[best][None])
        res = evaluator.search_linear(conf, space, trace=True, **SUITE)
        _same(res.trace["gains"][0, 0], np.tile(grid[best], (5, 1)), "candidate 0 is the grid's pick")
        _same(res.trace["fitness"][0, 0], fit[best], "and scores what the grid scored")
        assert res.fitness >= fit[best] and np.all(res.history[:, 2] >= fit[best])
        print("grid", fit[best], "search", res.fitness, "per_vehicle", per_vehicle)


def test_over_all_searches_on_the_disturbance_levels_too():
    need_gpu()
    conf = config.Config(pl_size=5)
    lag = [Disturbance("lag", v2v_delay=3, noise_ep=0.05)]
    nom = evaluator.search_linear(conf, _space("ModelB", True), disturbances=lag, trace=True, **SUITE)
    space = _space("ModelB", True, over="all")
    both = evaluator.search_linear(conf, space, disturbances=lag, trace=True, **SUITE)
    assert (nom.K, both.K) == (4, 8) and (nom.pop, nom.gens, nom.n_elite) == (both.pop, both.gens, both.n_elite)
    _same(both.trace["gains"][0], nom.trace["gains"][0], "generation 0 draws the same candidates")
    assert not np.array_equal(both.trace["fitness"][0], nom.trace["fitness"][0])
    _check_trace(conf, space, both, lag)
    # over = nominal ignores the levels: the search without any
    none = evaluator.search_linear(conf, _space("ModelB", True), trace=True, **SUITE)
    _same(none.trace["fitness"], nom.trace["fitness"], "nominal")


def test_search_is_deterministic_and_the_seed_matters():
    need_gpu()
    conf = config.Config(pl_size=3)
    a = evaluator.search_linear(conf, _space("ModelB", True), trace=True, **SUITE)
    b = evaluator.search_linear(conf, _space("ModelB", True), trace=True, **SUITE)
    for k in a.trace:
        _same(a.trace[k], b.trace[k], k)
    _same(a.history, b.history, "history"), _same(a.mean, b.mean, "mean"), _same(a.std, b.std, "std")
    assert a.fitness == b.fitness and a.generation == b.generation and np.array_equal(a.law.table, b.law.table)
    other = SearchSpace(_space("ModelB", True).bounds, pop=64, gens=4, seed=SEED + 1)
    c = evaluator.search_linear(conf, other, trace=True, **SUITE)
    _same(c.trace["gains"][0, 0], a.trace["gains"][0, 0], "candidate 0 is the midpoint under any seed")
    assert not np.array_equal(c.trace["gains"][0], a.trace["gains"][0]) and not np.array_equal(c.history, a.history)
    # the default seed is the configuration's evaluation seed
    d = evaluator.search_linear(conf, SearchSpace(other.bounds, pop=64, gens=1), trace=True, **SUITE)
    e = evaluator.search_linear(conf, SearchSpace(other.bounds, pop=64, gens=1, seed=conf.evaluation_seed), trace=True, **SUITE)
    _same(d.trace["gains"], e.trace["gains"], "default seed")


# ---- 4. the CLI --------------------------------------------------------------------------------------------------------------------------

TR = ("tr", "--pl_num", "2", "--pl_size", "3", "--buffer_size", "500", "--total_time_steps", "80", "--rng", "device", "--episodes", "platoon",
      "--report_every", "40")
FLAGS = ("--scenarios", "step,sine", "--eval_seeds", "6-7", "--disturb", "lag:v2v_delay=2")
SPEC = "kp=0:2,kv=0:4,pop=64,gens=3"


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


def test_cli_tr_and_esim_write_the_searched_law_and_leave_the_other_files_alone(tmp_path, capsys):
    need_gpu()
    import csv

    plain = _run(capsys, *TR, *FLAGS, "--out", str(tmp_path / "plain"))[-1]
    base = _run(capsys, *TR, *FLAGS, "--baseline_search", SPEC, "--out", str(tmp_path / "with"))[-1]
    a, b = _files(plain), _files(base)
    assert set(b) == set(a) | {"baseline.csv"} and {"curve.csv", "scenarios.csv", "robustness.csv"} <= set(a)
    for f in a:
        assert a[f] == b[f], f
    pj, bj = json.load(open(os.path.join(plain, "conf.json"))), json.load(open(os.path.join(base, "conf.json")))
    rest = {k: v for k, v in bj.items() if k not in ("baseline_suite", "baseline_search", "timestamp")}
    assert "baseline_search" not in pj and rest == {k: v for k, v in pj.items() if k != "timestamp"}
    rec = dict(bj["baseline_search"])
    assert (rec["spec"], rec["pop"], rec["gens"], rec["n_elite"], rec["cases"]) == (SPEC, 64, 3, 8, 4)
    assert np.asarray(rec["table"]).shape == (3, 4) and np.asarray(rec["history"]).shape == (3, 4) and 0 <= rec["generation"] < 3
    assert rec["history"][-1][2] == rec["fitness"] and rec["history"][-1][3] == 8
    (name, items), = bj["baseline_suite"]
    assert name == "searched" and dict(items)["table"] == rec["table"]
    rows = list(csv.reader(open(os.path.join(base, "baseline.csv"))))
    assert rows[0] == scenarios.BASELINE_ROBUSTNESS_HEADER and len(rows) == 1 + 2 * 2 * 2 * 3 and {x[0] for x in rows[1:]} == {"searched"}
    # esim: the same search, the same file; one report line of the search; from the grid's pick it is never below the grid
    os.rename(os.path.join(base, "baseline.csv"), os.path.join(base, "baseline.csv.tr"))
    lines = _run(capsys, "esim", base, *FLAGS, "--baseline_search", SPEC)
    assert open(os.path.join(base, "baseline.csv"), "rb").read() == open(os.path.join(base, "baseline.csv.tr"), "rb").read()
    found = [x for x in lines if x.startswith("baseline searched search: fitness ")]
    assert len(found) == 1 and f"at generation {rec['generation']} of 3 (pop 64, 8 elites, 4 cases, 3 searched row(s))" in found[0]
    assert sum(x.startswith("baseline searched s") and ": score " in x for x in lines) == 2
    lines = _run(capsys, "esim", base, *FLAGS, "--baseline_tune", "kp=0:2:3,kv=0:4:3", "--baseline_search", SPEC + ",per_vehicle=0")
    rows = list(csv.reader(open(os.path.join(base, "baseline.csv"))))
    assert [x[0] for x in rows[1::24]] == ["tuned", "searched"]
    conf = config.Config(pl_size=3)
    grid = scenarios.parse_gain_grid("kp=0:2:3,kv=0:4:3")
    best, fit = evaluator.tune_linear(conf, grid, scenarios=["step", "sine"], seeds=[6, 7])
    found = [x for x in lines if x.startswith("baseline searched search: fitness ")]
    assert len(found) == 1 and float(found[0].split()[4]) >= float(f"{fit[best]:.6f}") and "1 searched row(s)" in found[0]


def test_cli_residual_searched_trains_on_the_table_the_search_finds_and_searches_once(tmp_path, capsys, monkeypatch):
    need_gpu()
    calls = []
    real = evaluator.search_linear
    monkeypatch.setattr(evaluator, "search_linear", lambda *a, **k: calls.append(1) or real(*a, **k))
    base = _run(capsys, *TR, "--residual", "searched", "--scenarios", "gaussian,brake", "--baseline_search", SPEC, "--out", str(tmp_path))[-1]
    cj = json.load(open(os.path.join(base, "conf.json")))
    law, rec = dict(cj["residual_law"]), dict(cj["baseline_search"])
    assert len(calls) == 1 and law["source"] == "searched" and law["scale"] == 1.0 and law["table"] == rec["table"]
    assert np.asarray(law["table"]).shape == (3, 4) and np.any(np.asarray(law["table"])[:, :2] != 0)
    assert [n for n, _ in cj["baseline_suite"]] == ["searched"] and os.path.getsize(os.path.join(base, "baseline.csv")) > 0
    lines = _run(capsys, "esim", base, "--n_timesteps", str(cj["steps_per_episode"]))
    rews = [np.float32(x.split()[-1]) for x in lines if x.startswith("platoon ")]
    assert [np.float32(r / cj["re_scalar"]) for r in rews] == [np.float32(r) for r in cj["pl_rews_for_simulations"]]
    # the saved actors alone are not the policy: without the record esim scores something else
    bare = dict(cj)
    del bare["residual_law"]
    json.dump(bare, open(os.path.join(base, "conf.json"), "w"))
    lines = _run(capsys, "esim", base, "--n_timesteps", str(cj["steps_per_episode"]))
    assert [np.float32(x.split()[-1]) for x in lines if x.startswith("platoon ")] != rews
