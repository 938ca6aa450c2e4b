"""The frequency-response evaluator (avd_eval_cases_freq_f32, csrc/evalx.hip; avd_eval_linear_freq_f32, csrc/lin.hip;
evaluator.run_frequency / run_linear_frequency): a sweep of sinusoidal leader inputs as cases, the single-bin Fourier sums reduced in
the rollout loop. 1. counters and metrics are the twin entry points' on the same cases; 2. the spectrum equals
scenarios.spectrum_from_traces on the rollout kernel's traces (a RolloutBatch whose public `leader` rows are overwritten with the
sinusoids, as tests/test_gpu_eval_cases.py builds its yardstick) bit for bit; 3. the linear kernel against the actors' kernel; 4. both
against the float64 oracles; 5. VecTrainer.evaluate_frequency and the CLI."""
import csv
import json
import os

import numpy as np
import pytest
import torch

from avddpg_amd import __main__ as cli
from avddpg_amd import _hip, config, evaluator, scenarios, trainer
from avddpg_amd.scenarios import Disturbance, FrequencySpec, LinearLaw, ResidualLaw
from tests import disturbed_oracle as do
from tests import linear_oracle as lo
from tests import scenario_oracle as so
from tests.gpu_util import need_gpu
from tests.test_gpu_eval_rollout import _group, _same
from tests.test_gpu_residual import _load, _zero_actors

pytestmark = pytest.mark.gpu

T64, CYCLES = 64, (1, 4, 15)  # settle = 0.5: a window of 32 steps; 15 = ceil(32 / 2) - 1, the highest bin kept
LEVELS = [Disturbance("lag", v2v_delay=3, v2v_drop=0.1), Disturbance("noisy", noise_ep=0.05, dyn_coeff=0.15)]


def _spec(conf, cycles, T=T64, settle=0.5, amp=None):
    """The sweep whose snapped cycle counts are exactly ``cycles`` (one, or three log-spaced whose middle snaps to the middle one)."""
    W = T - int(np.floor(settle * T))
    f = [c / (W * conf.sample_rate) for c in cycles]
    spec = FrequencySpec(f[0], f[-1], len(cycles), amp=amp, settle=settle, steps=T)
    assert spec.cycles(conf).tolist() == list(cycles) and spec.window(conf) == (T, T - W, W)
    return spec


# K = F x NS: 1, 3, 7 and 17 cases -- blocks of 1, 4, 8 and 16 rows, the last with a one-row tail
SHAPES = {1: ((4,), [6]), 3: (CYCLES, [6]), 7: ((15,), list(range(6, 13))), 17: ((1,), list(range(6, 23)))}


def _same_results(got, ref, what):
    _same(got.counters.reshape(ref.counters.shape), ref.counters, (what, "counters"))
    _same(got.scores.reshape(ref.scores.shape), ref.scores, (what, "scores"))
    for n in scenarios.METRICS:
        _same(got.metrics[n].reshape(ref.metrics[n].shape), ref.metrics[n], (what, n))


def _twin(b):
    """The non-frequency batch on a FrequencyBatch's cases: same leader rows, levels, seeds, sets and law."""
    names = [f"f{int(c)}" for c in b.cycles]
    rows = b.leader_h.reshape(b.NC, -1, b.T)[:, 0]
    return names, rows


# ---- 1. pure addition --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["nominal", "disturbed", "residual", "disturbed residual"])
def test_counters_and_metrics_are_the_twin_entry_points(form):
    need_gpu()
    L = 5
    conf = config.Config(pl_size=L)
    grp = _group(conf, 2 * L, 4, 1, seed=301)
    levels = LEVELS if "disturbed" in form else []
    law = ResidualLaw(0.5, 1, 0, 0.3, scale=0.5) if "residual" in form else None
    seeds = [6, 7]
    b = evaluator.prepare_frequency(conf, grp, [0, 1], _spec(conf, CYCLES), levels, seeds, base_law=law)
    b.launch()
    got = b.results()
    names, rows = _twin(b)
    twin = evaluator.CaseBatch(conf, grp, [0, 1], names, seeds, None, 10.0, None, None, None, law, b.levels, rows)
    assert torch.equal(twin.leader, b.leader) and torch.equal(twin.x0, b.x0) and twin.K == b.K == 3 * (1 + len(levels)) * 2
    twin.launch()  # avd_eval_cases_f32 / _dist_f32 / _res_f32
    ref = twin.results()
    _same_results(got, ref, form)
    assert got.spectrum.shape == (2, 3, 1 + len(levels), 2, L, 10) and np.isfinite(got.spectrum).all()
    assert np.abs(got.metrics["sum_u2"]).min() > 0 and not np.array_equal(got.counters[0], got.counters[1])
    if levels:
        assert len({got.spectrum[0, 0, d].tobytes() for d in range(3)}) == 3  # every level reaches the response


@pytest.mark.parametrize("disturbed", [False, True])
def test_linear_counters_and_metrics_are_the_twin_entry_point(disturbed):
    need_gpu()
    L = 5
    conf = config.Config(pl_size=L)
    laws = [LinearLaw("cacc", 2, 1), LinearLaw("ff", 1, 2, -0.5, 1), LinearLaw("zero")]
    levels = LEVELS if disturbed else []
    b = evaluator.prepare_linear_frequency(conf, laws, _spec(conf, CYCLES), levels, [6, 7])
    b.launch()
    got = b.results()
    names, rows = _twin(b)
    twin = evaluator.LinearBatch(conf, b.gains_h, names, levels, [6, 7], None, 10.0, None, True, rows)
    assert torch.equal(twin.leader, b.leader)
    twin.launch()
    _same_results(got, twin.results(), "linear")
    assert got.spectrum.shape == (3, 3, 1 + len(levels), 2, L, 10) and np.all(got.spectrum[2, ..., 8:] == 0)  # the zero law: u = 0


# ---- 2. the spectrum, bit for bit ----------------------------------------------------------------------------------------------------------

def _yardstick_spectrum(conf, grp, platoons, spec, seeds, **kw):
    """Per frequency one traced RolloutBatch whose leader rows are the sinusoid: spectrum_from_traces of every trace ->
    (float32 [NP, F, NS, L, 10], counters [NP, F, NS, M])."""
    leader, basis = scenarios.frequency_leader(spec, conf), scenarios.frequency_basis(spec, conf)
    NP, NS = len(platoons), len(seeds)
    out, cnts = [], []
    for q in range(leader.shape[0]):
        b = evaluator.prepare_many(conf, grp, platoons, seeds=seeds, manual_timestep_override=leader.shape[1],
                                   trace=[(i, k) for i in range(NP) for k in range(NS)], **kw)
        b.leader.copy_(torch.from_numpy(leader[q]).to(b.leader.device).expand_as(b.leader))
        b.launch()
        _, cnt, tr = b.results()
        out.append(np.array([[scenarios.spectrum_from_traces(tr[(i, k)], basis[q]) for k in range(NS)] for i in range(NP)]))
        cnts.append(cnt)
    return np.stack(out, axis=1), np.stack(cnts, axis=1)


def _check_spectrum(conf, grp, platoons, cycles, seeds, **kw):
    spec = _spec(conf, cycles)
    r = evaluator.run_frequency(conf, grp, platoons, spec, seeds=seeds, **kw)
    ref, cnt = _yardstick_spectrum(conf, grp, platoons, spec, seeds, **kw)
    got = r.spectrum[:, :, 0]
    assert got.dtype == np.float32 and np.isfinite(got[..., :6]).all() and np.abs(got[..., :6]).max() > 0
    w = not np.isnan(ref[..., 6:8]).any()  # (decentralized Model A's traces hide w: the host definition leaves its pair NaN)
    assert w == (conf.model == conf.modelB or conf.framework == conf.cntrl) and np.isfinite(got[..., 6:8]).all()
    cols = list(range(10)) if w else [0, 1, 2, 3, 4, 5, 8, 9]
    _same(got[..., cols], ref[..., cols], ("spectrum", cycles, len(seeds)))
    _same(r.counters[:, :, 0], cnt, "counters")
    return r


@pytest.mark.parametrize("L", [1, 3, 5, 16])
def test_spectrum_is_the_host_definition_on_the_rollout_kernels_traces(L):
    """Nominal and residual, Model B, decentralized, per-agent sets, at K = 1, 3, 7, 17: every block size, 17 with a one-row tail."""
    need_gpu()
    conf = config.Config(pl_size=L)
    grp = _group(conf, 2 * L, 4, 1, seed=310 + L)
    used = set()
    for K, (cycles, seeds) in SHAPES.items():
        b = evaluator.prepare_frequency(conf, grp, [0, 1], _spec(conf, cycles), seeds=seeds)
        assert b.K == K
        used.add(b.block)
        _check_spectrum(conf, grp, [1, 0], cycles, seeds)
        if K in (3, 17):
            r = _check_spectrum(conf, grp, [0, 1], cycles, seeds, base_law=ResidualLaw(0.5, 1, 0, 0.3, scale=0.5))
            assert np.abs(r.spectrum[..., 8:]).max() > 0
    assert used == {1, 4, 8, 16}


@pytest.mark.parametrize("model,framework", [("ModelA", "decentralized"), ("ModelB", "centralized"), ("ModelA", "centralized")])
def test_spectrum_model_a_and_centralized(model, framework):
    need_gpu()
    L = 3
    conf = config.Config(pl_size=L, model=model, framework=framework)
    S = 3 if model == "ModelA" else 4
    if framework == "centralized":
        grp = _group(conf, 2, S * L, L, seed=331, hidd_mult=conf.centrl_hidd_mult)
    else:
        grp = _group(conf, 2 * L, S, 1, seed=332)
    for K in (3, 17):
        _check_spectrum(conf, grp, [0, 1], *SHAPES[K])
    if framework == "decentralized":
        _check_spectrum(conf, grp, [0, 1], *SHAPES[7], base_law=ResidualLaw(0.5, 1, -0.1, 0, scale=0.5))


def test_invalid_set_base_fills_the_spectrum_with_nan_and_shared_sets_repeat():
    need_gpu()
    L = 5
    conf = config.Config(pl_size=L)
    grp = _group(conf, 3 * L, 4, 1, seed=341)
    spec = _spec(conf, CYCLES)
    good = evaluator.run_frequency(conf, grp, range(3), spec, seeds=[6, 7])
    b = evaluator.prepare_frequency(conf, grp, range(3), spec, seeds=[6, 7])
    b.set_base[1] = 3 * L
    b.launch()
    r = b.results()
    assert np.isnan(r.spectrum[1]).all() and np.isnan(r.counters[1]).all()
    _same(r.spectrum[[0, 2]], good.spectrum[[0, 2]], "the other groups")
    sh = evaluator.run_frequency(conf, grp, range(3), spec, seeds=[6, 7], set_mod=L, set_bases=[L, 0, L])
    _same(sh.spectrum, good.spectrum[[1, 0, 1]], "set_bases")
    np.random.seed(77)
    before = np.random.get_state()
    evaluator.run_frequency(conf, grp, [0], spec)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]


# ---- 3. the linear kernel ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [3, 5, 16])
def test_linear_spectrum_is_the_actors_kernels(L):
    """Zero gains against actors whose last layer is zero, and a law against the same law as a residual policy's base under zero actors
    (u = clip(law + 0)): L = 3 leaves one idle lane per wave, 5 leaves four, 16 fills it; G x K is no multiple of the rollouts per wave;
    G = 1; disturbed with the plant table null (a link level alone) and non-null."""
    need_gpu()
    conf = config.Config(pl_size=L)
    zero = _zero_actors(conf, L)
    spec = _spec(conf, CYCLES)
    seeds = [6, 7, 8]
    law = (1, 2, -0.5, 1)
    for levels in ([], LEVELS[:1], LEVELS):
        act0 = evaluator.run_frequency(conf, zero, [0], spec, levels, seeds, set_mod=L)
        act1 = evaluator.run_frequency(conf, zero, [0], spec, levels, seeds, set_mod=L, base_law=ResidualLaw(*law, scale=0.5))
        b = evaluator.prepare_linear_frequency(conf, [LinearLaw("zero"), LinearLaw("law", *law), LinearLaw("cacc", 2, 1)], spec, levels, seeds)
        assert (b.abc is None) == (len(levels) < 2) and (b.G * b.K) % (64 // L) != 0
        b.launch()
        lin = b.results()
        _same(lin.spectrum[0], act0.spectrum[0], ("zero gains", len(levels)))
        _same(lin.spectrum[1], act1.spectrum[0], ("law", len(levels)))
        _same(lin.counters[1], act1.counters[0], ("law counters", len(levels)))
        assert np.all(lin.spectrum[0, ..., 8:] == 0) and np.abs(lin.spectrum[1, ..., 8:]).max() > 0
        solo = evaluator.run_linear_frequency(conf, [LinearLaw("law", *law)], spec, levels, seeds)  # G = 1
        _same(solo.spectrum[0], lin.spectrum[1], ("G = 1", len(levels)))


# ---- 4. against float64 ----------------------------------------------------------------------------------------------------------------------

STATE_TOL, INPUT_TOL = (2e-4, 1e-4), (5e-5, 0.0)  # tests/scenario_oracle.check_against's trace tolerances (atol, rtol)


def _oracle_amplitudes(traces, basis_row, W):
    """float64 complex amplitudes [L, 5] of an oracle rollout's traces, and max |signal| [L, 5] inside the window."""
    sig = np.concatenate([traces["states"][:, :, :4], traces["inputs"][:, :, None]], axis=-1)  # [T, L, 5]
    b = np.asarray(basis_row, dtype=np.float64)
    X = (2.0 / W) * (np.einsum("tls,t->ls", sig, b[:, 0]) - 1j * np.einsum("tls,t->ls", sig, b[:, 1]))
    return X, np.abs(sig[np.abs(b).sum(axis=1) > 0]).max(axis=0)


def _bound(X, peak, W):
    """Per scaled amplitude [L, 5]: twice the trace tolerance of its signal, plus W * 2^-23 * max |signal| for the float32 sum."""
    tol = np.empty(X.shape)
    tol[:, :4] = 2 * (STATE_TOL[0] + STATE_TOL[1] * np.abs(X[:, :4]))
    tol[:, 4] = 2 * INPUT_TOL[0]
    return tol + W * 2.0 ** -23 * peak


def _check_against_oracle(what, spectrum, refs, W):
    """spectrum [F, L, 10] against per-frequency oracle (X, peak): every scaled amplitude inside its bound, gain_a and gain_ep inside
    the bound those propagate to: dg / g <= dA_i / |A_i| + dA_{i-1} / |A_{i-1}|."""
    got = scenarios.frequency_summary(spectrum, W)
    X = np.stack([x for x, _ in refs])
    tol = np.stack([_bound(x, p, W) for x, p in refs])
    err = np.abs(got["amp"] - np.abs(X))
    print(what, "amplitude error / bound, worst per signal:", np.max(err / tol, axis=(0, 1)))
    assert np.all(err <= tol), (what, np.argwhere(err > tol)[:4])
    ga, gep, _ = scenarios._gains_of(X)
    rel = tol / np.abs(X)
    ba = np.concatenate([rel[..., :1, 2] + rel[..., :1, 3], rel[..., 1:, 2] + rel[..., :-1, 2]], axis=-1)
    bep = rel[..., 1:, 0] + rel[..., :-1, 0]
    ea, eep = np.abs(got["gain_a"] / ga - 1), np.abs(got["gain_ep"][..., 1:] / gep[..., 1:] - 1)
    print(what, "gain_a relative error", ea.max(), "of bound", (ea / ba).max(), "gain_ep", eep.max(), "of bound", (eep / bep).max())
    assert np.all(ea <= ba) and np.all(eep <= bep), what


def test_against_the_float64_oracles():
    """Random actors and the law (0.5, 1, 0, 0.3), nominal and under v2v_delay = 3 with noise_ep = 0.05, T = 120 (a window of 60),
    cycles 1, 4, 20: the oracles' own traces, reduced in float64, against the device's float32 sums."""
    need_gpu()
    L, T = 3, 120
    conf = config.Config(pl_size=L)
    spec = _spec(conf, (1, 4, 20), T=T)
    W = spec.window(conf)[2]
    level = Disturbance("lag", v2v_delay=3, noise_ep=0.05)
    actors = so.random_actors(conf, L, 61)
    table = [[0.5, 1.0, 0.0, 0.3]] * L
    ra = evaluator.run_frequency(conf, _load(conf, actors), [0], spec, [level], set_mod=L)
    rl = evaluator.run_linear_frequency(conf, [LinearLaw("law", table=table)], spec, [level])
    leader, basis = scenarios.frequency_leader(spec, conf), scenarios.frequency_basis(spec, conf)
    ep = so.env_params(conf)
    for d, lv in enumerate([scenarios.NOMINAL, level]):
        kw = dict(sigma=lv.sigma, v2v_delay=lv.v2v_delay, v2v_drop=lv.v2v_drop, dyn_coeff=lv.dyn_coeff)
        ref_a, ref_l = [], []
        for q in range(3):
            tr = do.rollout(ep, L, actors, leader[q], **kw)[2]
            assert np.abs(tr["inputs"]).max() > 0.02
            ref_a.append(_oracle_amplitudes(tr, basis[q], W))
            ref_l.append(_oracle_amplitudes(lo.rollout(ep, L, table, leader[q], **kw)[2], basis[q], W))
        _check_against_oracle(f"actors {lv.name}", ra.spectrum[0, :, d, 0], ref_a, W)
        _check_against_oracle(f"law {lv.name}", rl.spectrum[0, :, d, 0], ref_l, W)


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------------------

def _same_frequency(got, ref, what):
    _same(got.spectrum, ref.spectrum, (what, "spectrum"))
    _same(got.scores, ref.scores, (what, "scores"))
    _same(got.counters, ref.counters, (what, "counters"))
    for n in scenarios.METRICS:
        _same(got.metrics[n], ref.metrics[n], (what, n))
    assert np.array_equal(got.cycles, ref.cycles) and got.disturbances == ref.disturbances and got.seeds == ref.seeds and got.W == ref.W


@pytest.mark.parametrize("fed", ["normal", "interfrl"])
def test_vec_trainer_evaluate_frequency_on_a_two_platoon_trainer(fed):
    """Per-agent sets (nofrl) and shared sets (interfrl with every step federated), alone and as a two-seed batch: the trainer's result
    is run_frequency on the same agents, axis order [(E,) P, F, dist, seed, ...]."""
    need_gpu()
    P, L = 2, 2
    conf = config.Config(num_platoons=P, pl_size=L, buffer_size=128, fed_method=fed, weighted_average_enabled=False)
    spec = _spec(conf, CYCLES)
    levels, seeds = LEVELS[:1], [6, 9]
    for batch in (None, [3, 4]):
        vt = trainer.VecTrainer(conf, rng="device", auto_reset="platoon", seeds=batch)
        assert vt.shared == (fed == "interfrl")
        vt.reset_episode()
        for _ in range(40):
            vt.step()
        torch.cuda.synchronize()
        r = vt.evaluate_frequency(spec, levels, seeds=seeds)
        kw = dict(set_mod=vt.M) if vt.shared else {}
        if batch is None:
            assert r.spectrum.shape == (P, 3, 2, 2, L, 10) and r.scores.shape == (P, 3, 2, 2)
            _same_frequency(r, evaluator.run_frequency(vt.conf, vt.agents, range(P), spec, levels, seeds, **kw), "solo")
            sub = vt.evaluate_frequency(spec, levels, seeds=[9], platoons=[1])
            _same(sub.spectrum[:, :, :, 0], r.spectrum[[1], :, :, 1], "platoons")
            assert r.summary()["gain_a"].shape == (P, 3, 2, 2, L)
        else:
            assert r.spectrum.shape == (2, P, 3, 2, 2, L, 10) and r.counters.shape == (2, P, 3, 2, 2, L)
            for e in range(2):
                solo = evaluator.run_frequency(vt.conf, vt.experiment_agents(e), range(P), spec, levels, seeds, **kw)
                _same_frequency(cli._freq_slice(r, e), solo, ("experiment", e))
            assert not np.array_equal(r.spectrum[0], r.spectrum[1])
            sm = r.summary()
            assert sm["gain_a"].shape == (2, P, 3, 2, 2, L) and sm["peak_gain_a"].shape == (2, P, 2, 2, L) and sm["string_stable"].shape == (2, P, 2, 2)
        if vt.shared:
            idx = (slice(None), 0) if batch else (0,)
            jdx = (slice(None), 1) if batch else (1,)
            _same(r.spectrum[idx], r.spectrum[jdx], "shared sets: every platoon's response is the same")


TR = ("tr", "--pl_num", "2", "--pl_size", "3", "--buffer_size", "500", "--total_time_steps", "80", "--rng", "device", "--episodes", "platoon",
      "--report_every", "40")
FREQ = ("--freq_response", "fmin=0.03,fmax=1,n=3", "--disturb", "lag:v2v_delay=3", "--baseline", "law:kp=2,kv=1")


def _run(capsys, *argv):
    cli.main(list(argv))
    return capsys.readouterr().out.strip().splitlines()


def _files(d):
    """A directory's files but conf.json and frequency.csv: the CSVs as bytes, the checkpoints as their arrays' bytes."""
    out = {}
    for f in sorted(os.listdir(d)):
        p = os.path.join(d, f)
        if f.endswith(".npz"):
            z = np.load(p)
            out[f] = [z[k].tobytes() for k in z.files]
        elif f not in ("conf.json", "frequency.csv") and os.path.isfile(p):
            out[f] = open(p, "rb").read()
    return out


def test_cli_tr_and_esim_write_frequency_csv_and_leave_every_other_file_alone(tmp_path, capsys):
    """`tr --freq_response ... --disturb ... --baseline law:kp=2,kv=1 --keep_best 40` against the same run without the flag: the other files
    are byte-identical and conf.json gains frequency_suite alone; `esim <dir>` with the flags on the plain directory writes the same
    frequency.csv and adds the same record; the law's measured gain_a agrees with its gain_a_theory column inside the bound of
    test_against_the_float64_oracles (T = 600, a window of 300 steps, cycles 1, 5, 30: the inputs the theory's residue is negligible on)."""
    need_gpu()
    keep = ("--keep_best", "40")
    plain = _run(capsys, *TR, *keep, "--out", str(tmp_path / "plain"))[-1]
    with_f = _run(capsys, *TR, *keep, *FREQ, "--out", str(tmp_path / "freq"))[-1]
    for sub in ("", "best"):
        a, b = _files(os.path.join(plain, sub)), _files(os.path.join(with_f, sub))
        assert set(a) == set(b) and any(f.endswith(".npz") for f in a) and "frequency.csv" not in os.listdir(os.path.join(plain, sub))
        for f in a:
            assert a[f] == b[f], (sub, f)
        pj, fj = json.load(open(os.path.join(plain, sub, "conf.json"))), json.load(open(os.path.join(with_f, sub, "conf.json")))
        suite = dict(fj.pop("frequency_suite"))
        drop = lambda j: {k: v for k, v in j.items() if k not in ("timestamp",)}
        assert drop(fj) == drop(pj) and "frequency_suite" not in pj
        assert suite["cycles"] == [1, 5, 30] and suite["window"] == 300 and suite["disturbances"] == ["nominal", "lag"] and suite["seeds"] == [6]
        assert dict(suite["spec"])["fmin"] == 0.03 and np.allclose(suite["freqs_hz"], np.array([1, 5, 30]) / 30.0)
        peaks = suite["peaks"]
        assert peaks[0] == ["controller", "disturbance", "peak_gain_a", "freq_hz", "vehicle", "string_stable"]
        assert [p[:2] for p in peaks[1:]] == [[c, d] for c in ("1", "2", "law") for d in ("nominal", "lag")]
        assert all(isinstance(p[5], bool) and p[2] > 0 and p[3] in suite["freqs_hz"] and 1 <= p[4] <= 3 for p in peaks[1:])
    rows = list(csv.reader(open(os.path.join(with_f, "frequency.csv"))))
    assert rows[0] == scenarios.FREQUENCY_HEADER and len(rows) == 1 + 3 * 2 * 1 * 3 * 3
    col = {n: i for i, n in enumerate(rows[0])}
    assert [r[0] for r in rows[1::18]] == ["1", "2", "law"] and all(r[col["gain_a_theory"]] == "" for r in rows[1:37])
    assert list(csv.reader(open(os.path.join(with_f, "best", "frequency.csv"))))[37:] == rows[37:]  # (the laws do not depend on the actors)
    law = [r for r in rows[1:] if r[0] == "law"]
    W, worst = 300, 0.0
    delta = lambda a: 2 * (2e-4 + 1e-4 * a) + W * 2.0 ** -23 * a  # a steady sinusoid's peak is its amplitude
    for r in law:
        v = int(r[col["vehicle"]])
        a, prev = float(r[col["amp_a"]]), float(r[col["amp_w"]])
        if v > 1:
            prev = float(next(x for x in law if x[1:5] == r[1:5] and int(x[col["vehicle"]]) == v - 1)[col["amp_a"]])
        g, th = float(r[col["gain_a"]]), float(r[col["gain_a_theory"]])
        bound = delta(a) / a + delta(prev) / prev
        worst = max(worst, abs(g / th - 1) / bound)
        assert abs(g / th - 1) <= bound, (r[:6], g, th, bound)
    nominal, lag = [r for r in law if r[1] == "nominal"], [r for r in law if r[1] == "lag"]
    assert [r[6:] for r in nominal] == [r[6:] for r in lag]  # (kf = 0: the link's delay does not reach this law, bit for bit)
    # esim on the plain directory: the same frequency.csv, frequency_suite added to its conf.json, nothing else touched
    before, pj = _files(plain), json.load(open(os.path.join(plain, "conf.json")))
    lines = _run(capsys, "esim", plain, *FREQ)
    assert len(lines) == 3 * 2 and lines[0].startswith("platoon 1 nominal: peak gain_a ") and lines[4].startswith("baseline law nominal: peak gain_a ")
    assert _files(plain) == before and open(os.path.join(plain, "frequency.csv"), "rb").read() == open(os.path.join(with_f, "frequency.csv"), "rb").read()
    ej = json.load(open(os.path.join(plain, "conf.json")))
    assert dict(ej.pop("frequency_suite")) == dict(json.load(open(os.path.join(with_f, "conf.json")))["frequency_suite"]) and ej == pj
    lines = _run(capsys, "esim", plain, "--n_timesteps", "20")  # without the flag: the rollouts it printed before
    assert len(lines) == 2 and lines[0].startswith("platoon 1: cumulative platoon reward ")
    print("law gain_a against its theory: worst error / bound", worst)


def test_cli_seed_batch_writes_the_frequency_response_into_every_experiment_directory(tmp_path, capsys):
    need_gpu()
    base = _run(capsys, *TR, "--seeds", "1,2", *FREQ, "--out", str(tmp_path))[-1]
    tables = []
    for k in (1, 2):
        d = os.path.join(base, f"seed{k}")
        rows = list(csv.reader(open(os.path.join(d, "frequency.csv"))))
        assert rows[0] == scenarios.FREQUENCY_HEADER and len(rows) == 1 + 3 * 2 * 1 * 3 * 3 and [r[0] for r in rows[1::18]] == ["1", "2", "law"]
        suite = dict(json.load(open(os.path.join(d, "conf.json")))["frequency_suite"])
        assert suite["cycles"] == [1, 5, 30] and len(suite["peaks"]) == 1 + 3 * 2
        tables.append(rows)
    assert tables[0][1:37] != tables[1][1:37] and tables[0][37:] == tables[1][37:]  # each experiment's own actors, the same law
