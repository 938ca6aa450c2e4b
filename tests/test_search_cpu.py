"""The gain search (evaluator.search_linear; avd_search_sample_f32 / avd_search_refit_f32, csrc/search.hip), the parts that need no GPU:
scenarios.SearchSpace with its parser and checks, tests/search_oracle.py's ranking and refit on hand-made arrays, the C ABI's three
statements of the two entry points, what they refuse on the host before any HIP call, and the CLI's refusals."""
import ctypes
import fnmatch
import math
import os
import re
import subprocess

import numpy as np
import pytest

from avddpg_amd import __main__ as cli
from avddpg_amd import _hip, config, scenarios
from avddpg_amd.scenarios import SearchSpace
from tests import search_oracle as so

F = np.float32
CSRC = os.path.join(os.path.dirname(_hip.HEADER_PATH), "..", "avddpg_amd", "csrc")


# ---- 1. the space, its parser and its checks -----------------------------------------------------------------------------------------------

def test_parse_search_and_tables():
    sp = scenarios.parse_search("kp=0:3,kv=0:4,ka=-1:0,kf=0:1,pop=1024,gens=30,elite=0.125")
    assert sp.bounds == dict(kp=(0.0, 3.0), kv=(0.0, 4.0), ka=(-1.0, 0.0), kf=(0.0, 1.0))
    assert (sp.pop, sp.gens, sp.elite, sp.alpha, sp.min_std, sp.seed, sp.per_vehicle, sp.over, sp.init) == \
        (1024, 30, 0.125, 0.7, 0.01, None, True, "nominal", None)
    assert sp.n_elite() == 128 and sp.rows(5) == 5 and scenarios.check_search(sp, config.Config(pl_size=5)) is sp
    lo, hi, mean, std, mn = sp.tables(5)
    for t in (lo, hi, mean, std, mn):
        assert t.dtype == F and t.shape == (5, 4) and t.flags["C_CONTIGUOUS"]
    assert np.array_equal(lo[2], F([0, 0, -1, 0])) and np.array_equal(hi[4], F([3, 4, 0, 1]))
    assert np.array_equal(mean[0], F([1.5, 2, -0.5, 0.5])) and np.array_equal(std[1], F([1.5, 2, 0.5, 0.5]))
    assert np.array_equal(mn[3], (0.01 * np.array([3.0, 4.0, 1.0, 1.0])).astype(F))
    # a missing key is frozen at 0, a single value (or lo == hi) frozen there; the other knobs
    sp = scenarios.parse_search(" kp = 0.5:2 , kv=1.5, per_vehicle=0, over=all, seed=4294967303, alpha=1, min_std=0, pop=16, gens=2, elite=0.5")
    assert sp.bounds == dict(kp=(0.5, 2.0), kv=(1.5, 1.5)) and (sp.per_vehicle, sp.over, sp.seed, sp.alpha, sp.min_std) == (False, "all", 4294967303, 1.0, 0.0)
    assert scenarios.check_search(sp) is sp and sp.rows(5) == 1 and sp.n_elite() == 8
    lo, hi, mean, std, mn = sp.tables(5)
    assert lo.shape == (1, 4) and np.array_equal(mean, F([[1.25, 1.5, 0, 0]])) and np.array_equal(std, F([[0.75, 0, 0, 0]])) and not mn.any()
    # init: one row (repeated) or one per searched row
    one = sp.with_init([[1.0, 1.5, 0, 0]])
    assert scenarios.check_search(one, config.Config(pl_size=5)) is one and np.array_equal(one.tables(5)[2], F([[1, 1.5, 0, 0]]))
    per = SearchSpace(dict(kp=(0, 2)), pop=8, elite=0.25, init=[[0.1 * v, 0, 0, 0] for v in range(3)])
    assert np.array_equal(scenarios.check_search(per, config.Config(pl_size=3)).tables(3)[2][:, 0], F([0, 0.1, 0.2]))
    spread = SearchSpace(dict(kp=(0, 2)), pop=8, elite=0.25, init=[[0.5, 0, 0, 0]])
    assert np.array_equal(spread.tables(3)[2], np.tile(F([0.5, 0, 0, 0]), (3, 1)))
    # a float32 grid value that sits on a bound stays inside it
    edge = SearchSpace(dict(kp=(0.1, 0.3)), pop=8, elite=0.25, init=np.float32([[0.3, 0, 0, 0]]))
    assert scenarios.check_search(edge) is edge


@pytest.mark.parametrize("text,msg", [
    ("", "no bound given"), ("kq=0:1", "unknown key 'kq'"), ("kp", "unknown key 'kp'"), ("kp=0:1,kp=0:2", "kp given twice"),
    ("kp=0:1,pop=8,pop=9", "pop given twice"), ("kp=0:1:3", "kp='0:1:3' is not lo:hi"), ("kp=a:1", "kp='a:1' is not lo:hi"),
    ("kp=0:1,pop=1e3", "pop='1e3' is not an integer"), ("kp=0:1,elite=big", "elite='big' is not a number"),
    ("kp=0:1,per_vehicle=2", "per_vehicle='2' is not 0 or 1"), ("kp=0:1,gens=2.5", "gens='2.5' is not an integer"),
])
def test_parse_search_refusals(text, msg):
    with pytest.raises(ValueError, match=re.escape(msg)):
        scenarios.parse_search(text)


def test_check_search_refusals():
    ok = dict(kp=(0, 2), kv=(0, 4))
    B = config.Config(pl_size=3)
    for sp, conf, msg in (
            ("kp=0:1", None, "is not a scenarios.SearchSpace"),
            (SearchSpace(dict(kq=(0, 1))), None, "unknown gain key(s) ['kq']"),
            (SearchSpace(dict(kp=(0, math.inf))), None, "kp=0:inf has a non-finite bound"),
            (SearchSpace(dict(kp=(math.nan, 1))), None, "kp=nan:1 has a non-finite bound"),
            (SearchSpace(dict(kp=(2, 1))), None, "kp has lo=2 > hi=1"),
            (SearchSpace(ok, pop=1), None, "pop=1 must be an integer in [2, 65536]"),
            (SearchSpace(ok, pop=65537), None, "pop=65537 must be an integer in [2, 65536]"),
            (SearchSpace(ok, pop=64.0), None, "pop=64.0 must be an integer"),
            (SearchSpace(ok, gens=0), None, "gens=0 must be an integer in [1, 10000]"),
            (SearchSpace(ok, gens=10001), None, "gens=10001 must be an integer in [1, 10000]"),
            (SearchSpace(ok, pop=15, elite=0.125), None, "elite=0.125 with pop=15 (need elite <= 0.5 and floor(elite * pop) >= 2)"),
            (SearchSpace(ok, elite=0.51), None, "elite=0.51 with pop=1024"),
            (SearchSpace(ok, elite=math.nan), None, "elite=nan"),
            (SearchSpace(ok, alpha=0), None, "alpha=0 must be a number in (0, 1]"),
            (SearchSpace(ok, alpha=1.01), None, "alpha=1.01 must be a number in (0, 1]"),
            (SearchSpace(ok, alpha=math.nan), None, "alpha=nan"),
            (SearchSpace(ok, min_std=-0.01), None, "min_std=-0.01 must be a finite number >= 0"),
            (SearchSpace(ok, over="some"), None, "over='some' (one of nominal, all)"),
            (SearchSpace(ok, seed=-1), None, "seed=-1 must be an integer in [0, 2^64)"),
            (SearchSpace({}), None, "no searched dimension"),
            (SearchSpace(dict(kp=(1, 1), kv=2.0)), None, "no searched dimension"),
            (SearchSpace(ok, init=[[1, 1, 0]]), None, "init must be a finite [L or 1, 4] array (got shape (1, 3))"),
            (SearchSpace(ok, init=[1, 1, 0, 0]), None, "init must be a finite [L or 1, 4] array (got shape (4,))"),
            (SearchSpace(ok, init=[[1, math.nan, 0, 0]]), None, "init must be a finite"),
            (SearchSpace(ok, init=[[2.5, 1, 0, 0]]), None, "lies outside the bounds"),
            (SearchSpace(ok, init=[[1, 1, 0, 0.1]]), None, "lies outside the bounds"),  # kf is frozen at 0
            (SearchSpace(ok, init=[[1, 1, 0, 0]] * 2), B, "init of 2 rows for 3 searched row(s) (pl_size=3, per_vehicle=True)"),
            (SearchSpace(ok, init=[[1, 1, 0, 0]] * 3, per_vehicle=False), B, "init of 3 rows for 1 searched row(s)"),
            (SearchSpace(dict(kp=(0, 1), kf=(0, 1))), config.Config(model="ModelA"), "a search over kf needs Model B"),
            (SearchSpace(dict(kp=(0, 1), kf=0.5)), config.Config(model="ModelA"), "a search over kf needs Model B"),
            (SearchSpace(ok), config.Config(framework="centralized"), "not available for the centralized framework")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            scenarios.check_search(sp, conf)
    assert scenarios.check_search(SearchSpace(dict(kp=(0, 1), kf=(0, 0))), config.Config(model="ModelA"))  # kf frozen at 0 is fine
    assert scenarios.check_search(SearchSpace(ok, pop=4, elite=0.5, gens=10000, alpha=1, min_std=0, seed=2 ** 64 - 1))
    assert scenarios.parse_residual("searched") == scenarios.SEARCHED == "searched"
    # the name is reserved only for a caller that says so
    assert scenarios.check_baselines([scenarios.LinearLaw("searched", kp=1)])
    with pytest.raises(ValueError, match="'searched' is reserved for the law --baseline_search finds"):
        scenarios.check_baselines([scenarios.LinearLaw("searched", kp=1)], reserved=(scenarios.TUNED, scenarios.SEARCHED))


# ---- 2. the oracle's ranking ----------------------------------------------------------------------------------------------------------------

def test_oracle_ranking_on_hand_made_arrays():
    nan = np.nan
    for f, order, n_valid in (
            ([1.0, 3.0, 2.0], [1, 2, 0], 3),
            ([-4.0], [0], 1),
            ([2.0, 5.0, 5.0, 2.0, 5.0], [1, 2, 4, 0, 3], 5),              # ties: the lower index first
            ([0.0, -0.0, 1.0], [2, 0, 1], 3),                             # -0 == 0: a tie
            ([nan, 1.0, nan, 3.0, 1.0], [3, 1, 4, 0, 2], 3),              # NaNs last, by index
            ([nan, nan, nan], [0, 1, 2], 0),                              # all NaN
            ([nan, -np.inf, np.inf], [2, 1, 0], 2),                       # -inf still beats a NaN
            ([-1.0, nan, -1.0, nan, -0.5], [4, 0, 2, 1, 3], 3)):
        got, nv = so.rank(F(f))
        assert got.dtype == np.int32 and got.tolist() == order and nv == n_valid, f
        # the pairwise statement of the rule agrees, entry by entry
        for a in range(len(f)):
            for b in range(len(f)):
                if a != b:
                    ra, rb = order.index(a), order.index(b)
                    assert so.precedes(F(f[a]), a, F(f[b]), b) == (ra < rb), (f, a, b)
    # n_valid < n_elite: E is the valid count, elite_idx still holds n_elite entries (the NaNs fill the tail)
    G, L, R = 5, 2, 2
    gains = np.arange(G * L * 4, dtype=F).reshape(G, L, 4)
    f = F([nan, 7.0, nan, 9.0, nan])
    out = so.refit(G, L, R, 4, 1.0, gains, f, np.zeros((R, 4)), np.zeros((R, 4)), np.ones((R, 4)), np.zeros((R, 4)), -np.inf, -1, 3)
    assert out["E"] == 2 and out["elite_idx"].tolist() == [3, 1, 0, 2]
    assert np.array_equal(out["history_row"], F([9.0, 8.0, 9.0, 2.0])) and out["best_gen"] == 3 and out["best_fitness"] == 9.0
    assert np.array_equal(out["best_gains"], gains[3]) and np.array_equal(out["mean"], (gains[3] + gains[1]) / 2)
    # all NaN: nothing moves, E = 0
    mean, std, best = np.full((R, 4), 0.5, F), np.full((R, 4), 0.25, F), np.full((R, 4), 3.0, F)
    out = so.refit(G, L, R, 2, 0.7, gains, np.full(G, nan, F), np.zeros((R, 4)), mean, std, best, -2.0, 1, 5)
    assert out["E"] == 0 and np.array_equal(out["mean"], mean) and np.array_equal(out["std"], std) and np.array_equal(out["best_gains"], best)
    assert (out["best_fitness"], out["best_gen"]) == (-2.0, 1) and out["elite_idx"].tolist() == [0, 1]
    h = out["history_row"]
    assert np.isnan(h[0]) and np.isnan(h[1]) and h[2] == -2.0 and h[3] == 0


def test_oracle_best_record_is_strict_and_tied_rows_take_row_zero():
    G, L = 4, 3
    gains = np.random.RandomState(2).standard_normal((G, L, 4)).astype(F)
    f = F([1.0, 4.0, 4.0, 0.0])
    args = (np.zeros((1, 4)), np.zeros((1, 4)), np.ones((1, 4)))
    first = so.refit(G, L, 1, 2, 0.7, gains, f, *args, np.zeros((1, 4)), -np.inf, -1, 0)
    assert first["best_gen"] == 0 and first["best_fitness"] == 4.0 and np.array_equal(first["best_gains"], gains[1, :1])
    for later in (F([4.0, 1.0, 0.0, 0.0]), F([3.0, 1.0, 0.0, 0.0])):  # an equal best, a lower best: the record stays
        out = so.refit(G, L, 1, 2, 0.7, gains, later, *args, first["best_gains"], first["best_fitness"], first["best_gen"], 1)
        assert out["best_gen"] == 0 and out["best_fitness"] == 4.0 and np.array_equal(out["best_gains"], gains[1, :1])
        assert out["history_row"][0] == later[0] and out["history_row"][2] == 4.0
    out = so.refit(G, L, 1, 2, 0.7, gains, F([0, 0, 0, 4.5]), *args, first["best_gains"], first["best_fitness"], first["best_gen"], 2)
    assert out["best_gen"] == 2 and out["best_fitness"] == 4.5 and np.array_equal(out["best_gains"], gains[3, :1])


# ---- 3. the oracle's refit against float64 ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G,L,R,n_elite,alpha", [(2, 1, 1, 2, 1.0), (257, 5, 5, 32, 0.7), (1000, 3, 1, 125, 0.7), (64, 5, 5, 64, 1.0)])
def test_oracle_refit_matches_a_float64_computation(G, L, R, n_elite, alpha):
    rng = np.random.RandomState(G + L)
    # (positive gains and means: no update cancels, so a bound relative to the result is one relative to the operands)
    gains = rng.uniform(0.5, 3.5, (G, L, 4)).astype(F)
    f = (-5 + rng.standard_normal(G)).astype(F)
    mean, std = rng.uniform(0.5, 2, (R, 4)).astype(F), rng.uniform(0.1, 1, (R, 4)).astype(F)
    std[0, 3] = 0          # a frozen dimension
    min_std = np.full((R, 4), 1e-3, F)
    min_std[0, 0] = 5.0    # a floor that binds
    out = so.refit(G, L, R, n_elite, alpha, gains, f, min_std, mean, std, np.zeros((R, 4)), -np.inf, -1, 0)
    order = sorted(range(G), key=lambda i: (-float(f[i]), i))[:n_elite]
    assert out["elite_idx"].tolist() == order and out["E"] == n_elite
    x = gains[order][:, :R, :].reshape(n_elite, R * 4)
    m64, s64 = so.refit_f64(n_elite, x, float(F(alpha)), mean.reshape(-1), std.reshape(-1), min_std.reshape(-1))
    assert np.allclose(out["mean"].reshape(-1), m64, rtol=1e-6, atol=0) and np.allclose(out["std"].reshape(-1), s64, rtol=1e-6, atol=0)
    assert out["mean"][0, 3] == mean[0, 3] and out["std"][0, 3] == 0 and out["std"][0, 0] == 5.0
    assert out["mean"][0, 0] != mean[0, 0]  # (the bound dimension's mean still moves)
    h = out["history_row"]
    assert h[0] == f[order[0]] and h[3] == n_elite and abs(float(h[1]) - f[order].astype(np.float64).mean()) <= 1e-6 * abs(float(h[1]))


def test_oracle_sample_rules():
    G, L, R = 37, 3, 3
    mean, std = np.tile(F([1.0, 2.0, -0.5, 0.25]), (R, 1)), np.tile(F([1.0, 0.0, 0.5, 0.25]), (R, 1))
    lo, hi = np.tile(F([0.5, 0, -1, 0]), (R, 1)), np.tile(F([1.5, 4, 0, 0.5]), (R, 1))
    x, raw = so.sample(G, L, R, mean, std, lo, hi, 2 ** 32 + 7, 3)
    assert x.shape == raw.shape == (G, L, 4) and x.dtype == F
    assert np.array_equal(x[0], mean) and np.all(x[:, :, 1] == 2.0)                       # candidate 0; a frozen dimension
    assert np.all(x >= lo) and np.all(x <= hi) and (raw < lo).any() and (raw > hi).any()  # the clip binds on some entries
    assert np.array_equal(x, np.clip(raw, lo, hi)) and len(np.unique(x[1:, :, 0])) > 10   # rows and candidates draw their own normals
    again, _ = so.sample(G, L, R, mean, std, lo, hi, 2 ** 32 + 7, 3)
    assert np.array_equal(again, x)
    for other in (so.sample(G, L, R, mean, std, lo, hi, 7, 3)[0], so.sample(G, L, R, mean, std, lo, hi, 2 ** 32 + 7, 4)[0]):
        assert not np.array_equal(other, x)  # the high seed word and the generation both matter
    tied, _ = so.sample(G, L, 1, mean[:1], std[:1], lo[:1], hi[:1], 9, 0)
    assert tied.shape == (G, L, 4) and np.array_equal(tied[:, 0], tied[:, 1]) and np.array_equal(tied[:, 0], tied[:, 2])
    n = (so.sample(4096, 1, 1, np.zeros((1, 4)), np.ones((1, 4)), np.full((1, 4), -9), np.full((1, 4), 9), 1, 0)[0])[1:]
    assert abs(float(n.mean())) < 0.05 and abs(float(n.std()) - 1) < 0.05  # unit normals, all four columns


# ---- 4. the C ABI -----------------------------------------------------------------------------------------------------------------------------

NEW = {"avd_search_sample_f32": ["int", "int", "int", "const float*", "const float*", "const float*", "const float*", "uint64_t",
                                 "uint64_t", "float*", "void*"],
       "avd_search_refit_f32": ["int", "int", "int", "int", "float", "const float*", "const float*", "const float*", "float*", "float*",
                                "float*", "float*", "int32_t*", "int", "int32_t*", "float*", "void*"]}
_CTYPE = {"int": ctypes.c_int, "float": ctypes.c_float, "uint64_t": ctypes.c_uint64}


def test_header_exports_map_and_binding_agree_on_the_new_entry_points():
    header = re.sub(r"/\*.*?\*/", "", open(_hip.HEADER_PATH).read(), flags=re.S)
    patterns = re.findall(r"global:\s*([^;]+);", re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "exports.map")).read(), flags=re.S))
    nm = subprocess.run(["nm", "-D", "--defined-only", _hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name, types in NEW.items():
        m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in the header"
        declared = [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*") for a in m.group(1).split(",")]
        assert declared == types, (name, declared)
        assert any(fnmatch.fnmatchcase(name, p.strip()) for p in patterns), f"{name} matches no global pattern of exports.map"
        assert name in exported and hasattr(_hip.lib(), name)
        want = [_CTYPE.get(t, ctypes.c_void_p) for t in types]
        assert _hip._PROTOS[name] == want, name
    assert re.search(r"^SRCS\s*:=.*\bsearch\.hip\b", open(os.path.join(CSRC, "Makefile")).read(), flags=re.M)


def test_stream_search_is_stream_ten():
    text = open(os.path.join(CSRC, "common.h")).read()
    assert "STREAM_SEARCH = 10," in text
    ids = [int(v) for v in re.findall(r"STREAM_[A-Z_]+ = (\d+),", text)]
    assert len(ids) == len(set(ids)) and so.STREAM_SEARCH == 10  # no stream id is used twice


_BOGUS = 0x1000  # non-null "device pointers" that nothing reads: every call below is refused on the host


def _sample_call(G=8, L=5, R=5, **ptrs):
    p = {k: ctypes.c_void_p(_BOGUS * (i + 1)) for i, k in enumerate(("mean", "std", "lo", "hi", "gains"))}
    p.update(ptrs)
    _hip.call("avd_search_sample_f32", G, L, R, p["mean"], p["std"], p["lo"], p["hi"], 2 ** 32 + 6, 0, p["gains"], None)


_REFIT_PTRS = ("gains", "fitness", "min_std", "mean", "std", "best_gains", "best_fitness", "best_gen", "elite_idx", "history_row")


def _refit_call(G=8, L=5, R=5, n_elite=2, alpha=0.7, generation=0, **ptrs):
    p = {k: ctypes.c_void_p(_BOGUS * (i + 1)) for i, k in enumerate(_REFIT_PTRS)}
    p.update(ptrs)
    _hip.call("avd_search_refit_f32", G, L, R, n_elite, alpha, p["gains"], p["fitness"], p["min_std"], p["mean"], p["std"], p["best_gains"],
              p["best_fitness"], p["best_gen"], generation, p["elite_idx"], p["history_row"], None)


def test_search_entry_points_refuse_on_the_host_before_any_hip_call():
    """One fault per call, with status and message (no GPU here: a call that got past its checks would fail with a HIP error instead)."""
    refuse = lambda msg: pytest.raises(_hip.AvdError, match=rf"failed \(-1\): {msg}")
    who = "avd_search_sample_f32"
    for name in ("mean", "std", "lo", "hi", "gains"):
        with refuse(f"{who}: null pointer"):
            _sample_call(**{name: None})
    for G in (0, -3):
        with refuse(rf"{who}: G={G} \(G must be >= 1\)"):
            _sample_call(G=G)
    for L in (0, -1, 17):
        with refuse(rf"{who}: L={L} \(L must be 1..16\)"):
            _sample_call(L=L, R=1)
    for R in (0, 2, 4, 6):
        with refuse(rf"{who}: R={R} \(R must be 1, tied rows, or L=5, one row per vehicle\)"):
            _sample_call(R=R)
    who = "avd_search_refit_f32"
    for name in _REFIT_PTRS:
        with refuse(f"{who}: null pointer"):
            _refit_call(**{name: None})
    for G in (0, 65537):
        with refuse(rf"{who}: G={G} \(G must be 1..65536\)"):
            _refit_call(G=G)
    with refuse(rf"{who}: L=17 \(L must be 1..16\)"):
        _refit_call(L=17, R=1)
    with refuse(rf"{who}: R=3 \(R must be 1, tied rows, or L=5"):
        _refit_call(R=3)
    for n in (0, 9, -1):
        with refuse(rf"{who}: n_elite={n} \(n_elite must be 1..G=8\)"):
            _refit_call(n_elite=n)
    for alpha in (0.0, -0.5, 1.5, math.nan):
        with refuse(rf"{who}: alpha="):
            _refit_call(alpha=alpha)
    with refuse(rf"{who}: generation=-1"):
        _refit_call(generation=-1)


# ---- 5. the CLI -------------------------------------------------------------------------------------------------------------------------------

def _parse(*argv, conf=None):
    return cli.get_cmdl_args(list(argv), config.Config() if conf is None else conf)


SPEC = "kp=0:2,kv=0:4,pop=64,gens=3"


@pytest.mark.parametrize("argv,match", [
    (["tr", "--baseline_search", SPEC], "--baseline_search needs --scenarios"),
    (["esim", "d", "--baseline_search", SPEC], "--baseline_search needs --scenarios"),
    (["tr", "--scenarios", "step", "--baseline_search", "kq=0:1"], "--baseline_search: search: unknown key 'kq'"),
    (["tr", "--scenarios", "step", "--baseline_search", "kp=0:1,kp=0:1"], "kp given twice"),
    (["tr", "--scenarios", "step", "--baseline_search", "kp=0:inf"], "non-finite bound"),
    (["tr", "--scenarios", "step", "--baseline_search", "kp=2:1"], "kp has lo=2.0 > hi=1.0"),
    (["esim", "d", "--scenarios", "step", "--baseline_search", "kp=0:1,pop=1"], "pop=1 must be an integer in [2, 65536]"),
    (["esim", "d", "--scenarios", "step", "--baseline_search", "kp=0:1,pop=70000"], "pop=70000 must be an integer"),
    (["tr", "--scenarios", "step", "--baseline_search", "kp=0:1,gens=0"], "gens=0 must be an integer in [1, 10000]"),
    (["tr", "--scenarios", "step", "--baseline_search", "kp=0:1,pop=8,elite=0.125"], "floor(elite * pop) >= 2"),
    (["tr", "--scenarios", "step", "--baseline_search", "kp=0:1,elite=0.6"], "elite=0.6"),
    (["tr", "--scenarios", "step", "--baseline_search", "kp=0:1,alpha=0"], "alpha=0.0 must be a number in (0, 1]"),
    (["tr", "--scenarios", "step", "--baseline_search", "kp=0:1,min_std=-1"], "min_std=-1.0 must be a finite number >= 0"),
    (["tr", "--scenarios", "step", "--baseline_search", "kp=1,kv=2"], "no searched dimension"),
    (["tr", "--scenarios", "step", "--baseline_search", SPEC, "--baseline", "searched:kp=1"], "'searched' is reserved"),
    (["tr", "--scenarios", "step", "--baseline_search", SPEC] + [x for i in range(16) for x in ("--baseline", f"l{i}")],
     "16 laws beside --baseline_search's `searched`: at most 16 in all"),
    (["tr", "--scenarios", "step", "--baseline_search", SPEC, "--baseline_tune", "kp=0:1:3"] + [x for i in range(15) for x in ("--baseline", f"l{i}")],
     "15 laws beside --baseline_search's `searched` and --baseline_tune's `tuned`: at most 16 in all"),
    (["tr", "--rng", "device", "--residual", "searched"], "--residual searched needs --scenarios and --baseline_search"),
    (["tr", "--rng", "device", "--scenarios", "step", "--residual", "searched"], "--residual searched needs --scenarios and --baseline_search"),
    (["tr", "--rng", "device", "--scenarios", "step", "--baseline_tune", "kp=0:1:3", "--residual", "searched"],
     "--residual searched needs --scenarios and --baseline_search"),
])
def test_cli_refusals(argv, match, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(*argv)
    assert e.value.code == 2 and match in capsys.readouterr().err


def test_cli_refuses_what_needs_the_configuration_and_a_process_group_and_reserves_the_name_only_under_the_flag(monkeypatch, capsys):
    for conf, spec, match in ((config.Config(model="ModelA"), "kp=0:1,kf=0:1", "--baseline_search: a search over kf needs Model B"),
                              (config.Config(framework="centralized"), SPEC, "not available for the centralized framework")):
        with pytest.raises(SystemExit) as e:
            _parse("tr", "--scenarios", "step", "--baseline_search", spec, conf=conf)
        assert e.value.code == 2 and match in capsys.readouterr().err
    args, _ = _parse("tr", "--scenarios", "step,sine", "--baseline", "cacc:kp=0.5,kv=1", "--baseline_search", SPEC)
    sp = cli._search_flag(args)
    assert isinstance(sp, SearchSpace) and (sp.pop, sp.gens, sp.text) == (64, 3, SPEC) and sp.bounds == dict(kp=(0.0, 2.0), kv=(0.0, 4.0))
    laws, tune = cli._baseline_flags(args)
    assert [b.name for b in laws] == ["cacc"] and tune is None
    only = _parse("esim", "d", "--scenarios", "step", "--baseline_search", SPEC)[0]
    assert cli._baseline_flags(only) == ([], None) and cli._search_flag(only).pop == 64
    assert cli._search_flag(_parse("tr", "--scenarios", "step")[0]) is None and cli._baseline_flags(_parse("tr", "--scenarios", "step")[0]) is None
    # without the flag a law of that name stays legal
    assert [b.name for b in _parse("tr", "--scenarios", "step", "--baseline", "searched:kp=1")[0].baseline] == ["searched"]
    res = _parse("tr", "--rng", "device", "--scenarios", "step", "--baseline_search", SPEC, "--residual", "searched")[0]
    assert res.residual == scenarios.SEARCHED
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        _parse("tr", "--scenarios", "step", "--baseline_search", SPEC)
    assert "--scenarios is not available under a process group of more than one rank" in capsys.readouterr().err
    assert cli._search_flag(_parse("esim", "d", "--scenarios", "step", "--baseline_search", SPEC)[0]) is not None  # esim runs in one process
