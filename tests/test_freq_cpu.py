"""The frequency-response evaluator, the parts that need no GPU: scenarios.FrequencySpec and its parser, the snapped frequencies, the
leader and basis tables, the host definition of the single-bin sums, frequency_summary's rules, the float64 theory of a linear law
against the float64 oracle, frequency.csv, the CLI's refusals, and what avd_eval_cases_freq_f32 / avd_eval_linear_freq_f32 refuse on the
host before any HIP call."""
import csv
import ctypes
import math

import numpy as np
import pytest

from avddpg_amd import __main__ as cli
from avddpg_amd import _hip, config, scenarios
from avddpg_amd.evaluator import FrequencyResults
from avddpg_amd.scenarios import FrequencySpec
from tests import linear_oracle as lo
from tests import scenario_oracle as so


# ---- 1. the spec ---------------------------------------------------------------------------------------------------------------------------

def test_parse_frequency_and_its_refusals():
    s = scenarios.parse_frequency("fmin=0.02, fmax=2 ,n=16")
    assert (s.fmin, s.fmax, s.n, s.amp, s.settle, s.steps) == (0.02, 2.0, 16, None, 0.5, None) and s.text == "fmin=0.02, fmax=2 ,n=16"
    s = scenarios.parse_frequency("fmin=0.1,fmax=0.1,n=1,amp=0.05,settle=0,steps=64")
    assert (s.amp, s.settle, s.steps) == (0.05, 0.0, 64) and s.items()[0] == ["fmin", 0.1] and "FrequencySpec(fmin=0.1" in repr(s)
    for text, msg in (("fmin=1,fmax=2,n=3,q=1", "unknown key 'q'"), ("fmin=1,fmax=2,n", "unknown key 'n'"),
                      ("fmin=1,fmin=1,fmax=2,n=3", "fmin given twice"), ("fmin=1,fmax=2", "n missing"), ("", "fmin, fmax, n missing"),
                      ("fmin=a,fmax=2,n=3", "fmin='a' is not a number"), ("fmin=1,fmax=2,n=2.5", "n='2.5' is not an integer"),
                      ("fmin=nan,fmax=2,n=3", "fmin=nan must be a finite number"), ("fmin=1,fmax=inf,n=3", "fmax=inf must be a finite number"),
                      ("fmin=0,fmax=2,n=3", "need 0 < fmin <= fmax"), ("fmin=-1,fmax=2,n=3", "need 0 < fmin <= fmax"),
                      ("fmin=3,fmax=2,n=3", "need 0 < fmin <= fmax"), ("fmin=1,fmax=2,n=0", "n=0 must be an integer in 1..256"),
                      ("fmin=1,fmax=2,n=257", "n=257 must be an integer in 1..256"), ("fmin=1,fmax=2,n=3,settle=1", r"settle=1.0 must be in \[0, 1\)"),
                      ("fmin=1,fmax=2,n=3,settle=-0.1", r"settle=-0.1 must be in \[0, 1\)"), ("fmin=1,fmax=2,n=3,settle=nan", "settle=nan must be a finite"),
                      ("fmin=1,fmax=2,n=3,amp=inf", "amp=inf must be a finite number"), ("fmin=1,fmax=2,n=3,amp=nan", "amp=nan must be a finite number"),
                      ("fmin=1,fmax=2,n=3,steps=0", "steps=0 must be an integer >= 1"),
                      ("fmin=1,fmax=2,n=3,steps=14", r"a window of W=7 steps \(T=14, settle=0.5\): need W >= 8"),
                      ("fmin=1,fmax=2,n=3,steps=30,settle=0.75", "a window of W=8 steps|^$")):
        if msg.endswith("|^$"):  # W = 30 - floor(22.5) = 8: the smallest window, accepted
            assert scenarios.parse_frequency(text).window(config.Config()) == (30, 22, 8)
            continue
        with pytest.raises(ValueError, match=msg):
            scenarios.parse_frequency(text)
    conf = config.Config()
    conf.steps_per_episode = 15  # (the default window is the configuration's episode)
    with pytest.raises(ValueError, match=r"a window of W=8 steps|W=7"):
        FrequencySpec(1, 2, 3, settle=0.55).window(conf)
    for bad, msg in ((FrequencySpec(1, 2, True), "n=True must be an integer"), (FrequencySpec("1", 2, 3), "fmin='1' must be a finite number"),
                     ("fmin=1", "is not a scenarios.FrequencySpec")):
        with pytest.raises(ValueError, match=msg):
            scenarios.check_frequency(bad)


def test_frequencies_snap_to_whole_cycles_and_duplicates_drop():
    conf = config.Config()
    assert (conf.steps_per_episode, conf.sample_rate) == (600, 0.1)
    s = scenarios.parse_frequency("fmin=0.02,fmax=2,n=16")
    assert s.window(conf) == (600, 300, 300)
    cyc = s.cycles(conf)
    # 0.02 Hz is 0.6 cycles in the 30 s window: kept at 1; 16 log-spaced points give 13 distinct bins
    assert cyc.tolist() == [1, 2, 3, 4, 5, 7, 10, 13, 18, 24, 32, 44, 60] and cyc.dtype == np.int64
    assert np.array_equal(s.freqs_hz(conf), cyc / 30.0)
    # the top of the range: bins stay below W / 2
    assert FrequencySpec(0.01, 100, 4, steps=64).cycles(conf).tolist() == [1, 15] and FrequencySpec(9, 9, 1, steps=66).cycles(conf).tolist() == [16]
    assert FrequencySpec(0.01, 100, 4, steps=66).cycles(conf).tolist()[-1] == math.ceil(33 / 2) - 1
    assert FrequencySpec(1, 1, 1, steps=64).cycles(conf).tolist() == [3]  # rint(3.2)
    assert FrequencySpec(0.3, 0.31, 200, steps=64).cycles(conf).tolist() == [1]  # 200 points, one bin
    assert FrequencySpec(1, 1, 1, settle=0.25, steps=100).window(conf) == (100, 25, 75)


def test_leader_and_basis_tables():
    conf = config.Config()
    s = FrequencySpec(0.3, 4.7, 3, steps=64)
    cyc = s.cycles(conf)
    assert cyc.tolist() == [1, 4, 15]
    lead, basis = scenarios.frequency_leader(s, conf), scenarios.frequency_basis(s, conf)
    assert lead.dtype == basis.dtype == np.float32 and lead.shape == (3, 64) and basis.shape == (3, 64, 2)
    assert lead.flags["C_CONTIGUOUS"] and basis.flags["C_CONTIGUOUS"]
    k = np.arange(64, dtype=np.float64)
    for q, c in enumerate(cyc):
        ang = 2.0 * np.pi * float(c) * (k - 32) / 32
        assert np.array_equal(lead[q], (conf.reset_max_u * np.sin(ang)).astype(np.float32))  # float64, rounded once; runs before t0 too
        assert np.all(basis[q, :32] == 0) and np.array_equal(basis[q, 32:, 0], np.cos(ang[32:]).astype(np.float32))
        assert np.array_equal(basis[q, 32:, 1], np.sin(ang[32:]).astype(np.float32)) and basis[q, 32].tolist() == [1.0, 0.0]
        assert np.abs(lead[q, :32]).max() > 0.05
    # (a float32 angle would differ: the rule is not vacuous)
    assert not np.array_equal(lead[2], (np.float32(conf.reset_max_u) * np.sin(ang.astype(np.float32))).astype(np.float32))
    assert np.array_equal(scenarios.frequency_leader(FrequencySpec(0.3, 4.7, 3, amp=0.25, steps=64), conf), (0.25 * np.sin(
        2.0 * np.pi * cyc[:, None].astype(np.float64) * (k[None] - 32) / 32)).astype(np.float32))
    # whole cycles: the basis is orthogonal over the window, so the single-bin sum of the leader itself is amp * W / 2 on sin alone
    re = np.einsum("qt,qt->q", lead.astype(np.float64), basis[..., 0]), np.einsum("qt,qt->q", lead.astype(np.float64), basis[..., 1])
    assert np.allclose(re[0], 0, atol=1e-6) and np.allclose(re[1], 0.1 * 16, rtol=1e-6)


# ---- 2. the host definition of the sums ----------------------------------------------------------------------------------------------------

def test_spectrum_from_traces_is_the_sequential_float32_sum():
    rng = np.random.RandomState(5)
    T, L = 37, 3
    st = rng.randn(T, L, 4).astype(np.float32) * np.float32([30, 3, 1, 1])
    u = rng.randn(T, L).astype(np.float32)
    b = rng.randn(T, 2).astype(np.float32)
    b[:9] = 0
    got = scenarios.spectrum_from_traces(dict(states=st, inputs=u), b)
    assert got.dtype == np.float32 and got.shape == (L, 10) and scenarios.NSPEC == 10 == _hip.AVD_EVAL_NSPEC
    sig = [st[..., 0], st[..., 1], st[..., 2], st[..., 3], u]
    for v in range(L):
        for i, x in enumerate(sig):
            re = im = np.float32(0)
            for t in range(T):
                re = np.float32(re + np.float32(x[t, v] * b[t, 0]))
                im = np.float32(im + np.float32(x[t, v] * b[t, 1]))
            assert got[v, 2 * i] == re and got[v, 2 * i + 1] == im
    # (a float64 sum or a fused multiply-add differs on these magnitudes)
    f64 = np.einsum("tl,t->l", st[..., 0].astype(np.float64), b[:, 0].astype(np.float64))
    assert np.any(got[:, 0] != f64.astype(np.float32))
    # the settling steps (zero basis rows) do not count
    st2 = st.copy()
    st2[:9] = 1e6
    assert np.array_equal(scenarios.spectrum_from_traces(dict(states=st2, inputs=u), b), got)
    # Model A's traces hide w: its pair stays NaN
    a = scenarios.spectrum_from_traces(dict(states=st[..., :3], inputs=u), b)
    assert np.isnan(a[:, 6:8]).all() and np.array_equal(a[:, :6], got[:, :6]) and np.array_equal(a[:, 8:], got[:, 8:])
    with pytest.raises(ValueError, match="need"):
        scenarios.spectrum_from_traces(dict(states=st, inputs=u), b[:-1])


def _sums(X, W):
    """Raw sums [..., L, 10] whose scaled amplitudes are X [..., L, 5]: X = (2 / W) (re - j im)."""
    out = np.zeros(X.shape[:-1] + (10,))
    out[..., 0::2], out[..., 1::2] = X.real * W / 2, -X.imag * W / 2
    return out


def test_frequency_summary_ratios_nan_rules_and_peaks():
    W = 40
    X = np.zeros((3, 4, 5), dtype=np.complex128)  # [F, L, signals]
    X[..., 3] = 1.0                                # w of every vehicle: the leader's acceleration as vehicle 0's model holds it
    X[0, :, 2] = [0.5, 0.25, 0.5j, 0.0]            # a: gains 0.5, 0.5, 2 (a quarter turn), 0
    X[1, :, 2] = [2.0, 1.0, 0.0, 3.0]              # a: 2, 0.5, 0, undefined (a zero denominator)
    X[2, :, 2] = [1.0, 1.0, -1.0, 1.0]
    X[..., 0] = [4.0, 2.0, 0.0, 1.0]               # ep: -, 0.5, 0, undefined
    X[..., 4] = 0.3 - 0.4j
    s = scenarios.frequency_summary(_sums(X, W), W, freqs_hz=[0.1, 0.2, 0.4], axis=0)
    assert np.allclose(s["amp"], np.abs(X)) and np.allclose(s["phase"], np.angle(X)) and np.allclose(s["amp"][..., 4], 0.5)
    assert np.allclose(s["gain_a"][0], [0.5, 0.5, 2.0, 0.0]) and np.allclose(s["gain_a"][1, :3], [2.0, 0.5, 0.0]) and np.isnan(s["gain_a"][1, 3])
    assert np.allclose(s["gain_a"][2], 1.0) and np.allclose(s["phase_a"][0, 2], np.pi / 2) and np.allclose(abs(s["phase_a"][2, 2]), np.pi)
    assert np.isnan(s["gain_ep"][:, 0]).all() and np.allclose(s["gain_ep"][:, 1:3], [[0.5, 0.0]] * 3) and np.isnan(s["gain_ep"][:, 3]).all()
    assert np.allclose(s["peak_gain_a"], [2.0, 1.0, 2.0, 1.0]) and s["peak_index"].tolist() == [1, 2, 0, 2]
    assert np.allclose(s["peak_freq_hz"], [0.2, 0.4, 0.1, 0.4]) and s["string_stable"].shape == () and not s["string_stable"]
    # stable: every defined peak <= 1 (1 itself is); an undefined vehicle does not count
    X[..., 2] = [1.0, 0.5, 0.5, 0.0]
    X[:, 3, 3] = 0.0
    s = scenarios.frequency_summary(_sums(X, W), W, axis=0)
    assert np.allclose(s["peak_gain_a"][:3], [1.0, 0.5, 1.0]) and s["peak_gain_a"][3] == 0 and bool(s["string_stable"]) and "peak_freq_hz" not in s
    X[:, 0, 3] = 0.0  # vehicle 0's own w at zero: its gain is undefined at every frequency
    s = scenarios.frequency_summary(_sums(X, W), W, axis=0)
    assert np.isnan(s["peak_gain_a"][0]) and s["peak_index"][0] == -1 and bool(s["string_stable"])
    # a batch: [G, F, ND, NS, L, 10] with the frequency axis at 1, as FrequencyResults.summary() calls it
    big = np.broadcast_to(_sums(X, W)[None, :, None, None], (2, 3, 2, 2, 4, 10))
    sb = scenarios.frequency_summary(big, W, [0.1, 0.2, 0.4], axis=1)
    assert sb["gain_a"].shape == (2, 3, 2, 2, 4) and sb["peak_gain_a"].shape == (2, 2, 2, 4) and sb["string_stable"].shape == (2, 2, 2)
    with pytest.raises(ValueError, match="the last axis holds the 10 sums"):
        scenarios.frequency_summary(np.zeros((3, 4, 8)), W)


# ---- 3. the theory against the float64 oracle ----------------------------------------------------------------------------------------------

def _oracle_gains(conf, table, cycles, T=600, settle=0.5, amp=0.1):
    """The float64 single-bin gains of tests/linear_oracle.rollout's traces: float64 [F, L] gain_a, gain_ep."""
    L = conf.pl_size
    t0 = int(math.floor(settle * T))
    W = T - t0
    k = np.arange(T, dtype=np.float64)
    ga, gep = [], []
    for c in cycles:
        ang = 2.0 * np.pi * c * (k - t0) / W
        _, _, tr = lo.rollout(so.env_params(conf), L, table, amp * np.sin(ang))
        # inside the window nothing is clipped (the start state's first steps are: the transient the settling half absorbs); no terminal step
        assert np.abs(tr["inputs"][t0:]).max() < 0.5 * conf.action_high and np.abs(tr["states"][..., 0]).max() < conf.max_ep
        sig = np.concatenate([tr["states"][:, :, :4], tr["inputs"][:, :, None]], axis=-1)[t0:]
        X = (2.0 / W) * (np.einsum("tls,t->ls", sig, np.cos(ang[t0:])) - 1j * np.einsum("tls,t->ls", sig, np.sin(ang[t0:])))
        a, e, _ = scenarios._gains_of(X[None])
        ga.append(a[0]), gep.append(e[0])
    return np.array(ga), np.array(gep), W


def test_linear_theory_matches_the_float64_oracle_to_1e_6():
    """Law (2, 1, 0, 0) on all five vehicles, Model B, euler, T = 600, settle 0.5, amp 0.1, cycles 1, 3, 10, 30: nothing saturates inside the
    window, nothing terminates, and the transient's residue in the window stays below the bound (measured: <= 2.3e-7). The bound is a
    condition on these inputs: at 100 cycles the residue already gives 1.5e-4 for this law."""
    conf = config.Config(pl_size=5)
    assert (conf.model, conf.method, conf.steps_per_episode) == (conf.modelB, "euler", 600)
    table = np.tile(np.float64([2, 1, 0, 0]), (5, 1))
    cycles = [1, 3, 10, 30]
    ga, gep, W = _oracle_gains(conf, table, cycles)
    th = scenarios.linear_frequency_response(conf, table, cycles, W)
    ea, eep = np.abs(ga / th["gain_a"] - 1), np.abs(gep[:, 1:] / th["gain_ep"][:, 1:] - 1)
    print("theory against the oracle: gain_a", ea.max(), "gain_ep", eep.max())
    assert th["gain_a"].shape == (4, 5) and ea.max() <= 1e-6 and eep.max() <= 1e-6
    assert np.isnan(th["gain_ep"][:, 0]).all() and th["X"].shape == (4, 5, 5)


def test_the_readme_law_1_2_m05_1_is_string_unstable_at_high_frequency():
    conf = config.Config(pl_size=5)
    th = scenarios.linear_frequency_response(conf, np.tile(np.float64([1, 2, -0.5, 1]), (5, 1)), [1, 100], 300)
    assert np.all(th["gain_a"][0] < 1) and np.all(th["gain_a"][1] > 1) and not th["string_stable"]
    assert np.allclose(th["gain_a"][:, 1], [0.9288, 1.1345], atol=1e-4)
    ok = scenarios.linear_frequency_response(conf, np.tile(np.float64([2, 1, 0, 0]), (5, 1)), [1, 3, 10, 30, 100], 300)
    assert ok["string_stable"] == bool(np.all(ok["peak_gain_a"] <= 1))
    # Model A: the law reads three states, the chained value is the predecessor's acceleration; a per-level engine lag moves the response
    ca = config.Config(pl_size=3, model="ModelA")
    a = scenarios.linear_frequency_response(ca, [[2, 1, 0, 9]] * 3, [3], 300)
    b = scenarios.linear_frequency_response(ca, [[2, 1, 0, 0]] * 3, [3], 300)
    assert np.array_equal(a["gain_a"], b["gain_a"]) and np.isfinite(a["gain_a"]).all()
    assert not np.allclose(scenarios.linear_frequency_response(conf, [[2, 1, 0, 0]] * 5, [3], 300, dyn_coeff=0.3)["gain_a"], ok["gain_a"][1])
    with pytest.raises(ValueError, match=r"gains of shape \(3, 4\): need \[5, 4\]"):
        scenarios.linear_frequency_response(conf, np.zeros((3, 4)), [1], 300)


# ---- 4. frequency.csv ------------------------------------------------------------------------------------------------------------------------

def _synthetic(G=2, F=3, ND=2, NS=2, L=3, W=32):
    rng = np.random.RandomState(11)
    sp = rng.randn(G, F, ND, NS, L, 10).astype(np.float32) * 10
    sp[0, 1, 0, 0, 0, 6:8] = 0  # vehicle 0's w at zero: an undefined gain_a, an empty field
    z = np.zeros((G, F, ND, NS), dtype=np.float32)
    return FrequencyResults([0.3125, 1.25, 4.6875], [1, 4, 15], W, 64, ["nominal", "lag"], [6, 7], sp, z, z[..., None], {})


def test_frequency_csv_rows(tmp_path):
    r = _synthetic()
    theory = np.arange(2 * 2 * 3 * 3, dtype=np.float64).reshape(2, 2, 3, 3) / 7
    path = tmp_path / "frequency.csv"
    scenarios.write_frequency_csv(path, [(r, ["1", "2"], None), (r, ["cacc", "ff"], theory)])
    rows = list(csv.reader(open(path)))
    assert rows[0] == scenarios.FREQUENCY_HEADER and len(rows[0]) == 6 + 5 + 5 + 4 and len(rows) == 1 + 2 * (2 * 2 * 2 * 3 * 3)
    assert rows[0][:6] == ["controller", "disturbance", "seed", "freq_hz", "cycles", "vehicle"] and rows[0][-4:] == ["gain_a", "gain_ep", "phase_a", "gain_a_theory"]
    # the order: controller, disturbance, seed, frequency, vehicle
    assert [x[:6] for x in rows[1:5]] == [["1", "nominal", "6", "0.3125", "1", "1"], ["1", "nominal", "6", "0.3125", "1", "2"],
                                           ["1", "nominal", "6", "0.3125", "1", "3"], ["1", "nominal", "6", "1.25", "4", "1"]]
    assert rows[1 + 9][:3] == ["1", "nominal", "7"] and rows[1 + 18][:3] == ["1", "lag", "6"] and rows[1 + 36][0] == "2" and rows[1 + 72][0] == "cacc"
    s = r.summary()
    for n, row in enumerate(rows[1:]):
        g, rem = divmod(n % 72, 36)
        d, rem = divmod(rem, 18)
        k, rem = divmod(rem, 9)
        q, v = divmod(rem, 3)
        at = (g, q, d, k, v)
        assert [float(x) for x in row[6:11]] == [float(x) for x in s["amp"][at]] and row[6] == repr(float(s["amp"][at][0]))
        assert [float(x) for x in row[11:16]] == [float(x) for x in s["phase"][at]]
        assert row[17] == ("" if v == 0 else repr(float(s["gain_ep"][at])))
        assert row[19] == ("" if n < 72 else repr(float(theory[g, d, q, v])))
        if at == (0, 1, 0, 0, 0):
            assert row[16] == "" and row[18] == ""  # the undefined ratio
        else:
            assert row[16] == repr(float(s["gain_a"][at])) and row[18] == repr(float(s["phase_a"][at]))
    peaks = scenarios.frequency_peaks(r, ["1", "2"])
    assert [p[:2] for p in peaks] == [["1", "nominal"], ["1", "lag"], ["2", "nominal"], ["2", "lag"]]
    g = np.nanmean(s["gain_a"], axis=3)
    for (tag, level, pk, hz, v, ok), (i, d) in zip(peaks, [(0, 0), (0, 1), (1, 0), (1, 1)]):
        assert pk == float(np.nanmax(g[i, :, d])) and hz in r.freqs_hz and 1 <= v <= 3 and ok == bool(np.all(np.nanmax(g[i, :, d], axis=0) <= 1))
    lines = scenarios.frequency_report_lines(r, ["1", "2"])
    assert len(lines) == 4 and lines[0].startswith("platoon 1 nominal: peak gain_a ") and "string_stable" in lines[0]


# ---- 5. the CLI ------------------------------------------------------------------------------------------------------------------------------

def _parse(*argv, conf=None):
    return cli.get_cmdl_args(list(argv), config.Config() if conf is None else conf)


@pytest.mark.parametrize("argv,match", [
    (["tr", "--freq_response", "fmin=1,fmax=2"], "--freq_response: frequency 'fmin=1,fmax=2': n missing"),
    (["esim", "d", "--freq_response", "fmin=0,fmax=2,n=3"], "--freq_response: frequency: fmin=0.0 fmax=2.0 (need 0 < fmin <= fmax)"),
    (["tr", "--freq_response", "fmin=1,fmax=2,n=3,settle=1"], "settle=1.0 must be in [0, 1)"),
    (["tr", "--freq_response", "fmin=1,fmax=2,n=3,steps=10"], "a window of W=5 steps"),
    (["tr", "--freq_response", "fmin=1,fmax=2,n=3,settle=0.99"], "a window of W=6 steps (T=600"),
    (["tr", "--freq_response", "fmin=1,fmax=2,n=3", "--scenario_amp", "0.2"], "--scenario_amp needs --scenarios"),
    (["tr", "--freq_response", "fmin=1,fmax=2,n=3", "--baseline_tune", "kp=0:1:3"], "--baseline_tune needs --scenarios"),
    (["esim", "d", "--freq_response", "fmin=1,fmax=2,n=3", "--baseline_search", "kp=0:1"], "--baseline_search needs --scenarios"),
    (["tr", "--freq_response", "fmin=1,fmax=2,n=3", "--disturb", "x:noise_ep=-1"], "--disturb: disturbance 'x': noise_ep=-1.0 must be a finite number >= 0"),
    (["tr", "--freq_response", "fmin=1,fmax=2,n=3", "--baseline", "x:kq=1"], "--baseline: baseline 'x': unknown key 'kq'"),
    (["tr", "--freq_response", "fmin=1,fmax=2,n=3", "--eval_seeds", "a"], "--eval_seeds"),
    # the present refusals without either flag stay
    (["tr", "--disturb", "lag:v2v_delay=3"], "--disturb needs --scenarios"),
    (["tr", "--baseline", "cacc:kp=1"], "--baseline needs --scenarios"),
    (["esim", "d", "--eval_seeds", "6,7"], "--eval_seeds needs --scenarios"),
])
def test_cli_refusals(argv, match, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(*argv)
    assert e.value.code == 2 and match in capsys.readouterr().err


def test_cli_accepts_the_shared_flags_without_scenarios_and_refuses_what_needs_the_configuration(monkeypatch, capsys):
    args, _ = _parse("tr", "--freq_response", "fmin=0.02,fmax=2,n=16", "--disturb", "lag:v2v_delay=3", "--baseline", "cacc:kp=2,kv=1",
                     "--eval_seeds", "6-7")
    assert isinstance(cli._freq(args), FrequencySpec) and cli._freq(args).n == 16 and args.scenarios is None
    assert [d.name for d in cli._disturb(args)] == ["lag"] and [b.name for b in args.baseline] == ["cacc"] and args.eval_seeds == [6, 7]
    assert cli._baseline_flags(args)[0][0].kp == 2.0
    args, _ = _parse("esim", "d", "--freq_response", "fmin=1,fmax=2,n=2", "--scenarios", "step", "--baseline_tune", "kp=0:1:3")
    assert cli._freq(args).n == 2 and args.scenarios == ["step"]
    assert cli._freq(_parse("tr")[0]) is None and cli._freq(_parse("esim", "d", "--scenarios", "step")[0]) is None
    for conf, argv, match in ((config.Config(framework="centralized"), ["--baseline", "cacc:kp=1"], "not available for the centralized framework"),
                              (config.Config(model="ModelA"), ["--baseline", "ff:kf=1"], "kf needs Model B"),
                              (config.Config(model="ModelA"), ["--disturb", "lag:v2v_delay=3"], "--freq_response: disturbance 'lag': v2v_delay / v2v_drop need Model B")):
        with pytest.raises(SystemExit) as e:
            _parse("tr", "--freq_response", "fmin=1,fmax=2,n=3", *argv, conf=conf)
        assert e.value.code == 2 and match in capsys.readouterr().err
    _parse("tr", "--freq_response", "fmin=1,fmax=2,n=3", conf=config.Config(framework="centralized"))  # the actors' kernel works for M = 1
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        _parse("tr", "--freq_response", "fmin=1,fmax=2,n=3")
    assert "--freq_response is not available under a process group of more than one rank" in capsys.readouterr().err
    assert cli._freq(_parse("esim", "d", "--freq_response", "fmin=1,fmax=2,n=3")[0]).n == 3  # esim runs in one process


# ---- 6. the entry points' host checks --------------------------------------------------------------------------------------------------------

_BOGUS = 0x1000  # non-null "device pointers" that nothing reads: every call below is refused on the host


def _ptrs(names, over):
    p = {k: ctypes.c_void_p(_BOGUS * (i + 1)) for i, k in enumerate(names)}
    p.update(over)
    return p


_LIN = ("d_consts", "gains", "x0", "prev_a0", "leader", "sigma", "delay", "drop_q", "noise_seed", "abc", "counters", "metrics", "basis", "spectrum")
_TABLES = ("sigma", "delay", "drop_q", "noise_seed", "abc")


def _linear_call(G=2, K=3, L=5, T=10, sample_rate=0.1, **ptrs):
    p = _ptrs(_LIN, ptrs)
    _hip.call("avd_eval_linear_freq_f32", p["d_consts"], G, K, L, T, p["gains"], p["x0"], p["prev_a0"], p["leader"], -2.5, 2.5, sample_rate,
              p["sigma"], p["delay"], p["drop_q"], p["noise_seed"], p["abc"], p["counters"], p["metrics"], p["basis"], p["spectrum"], None)


_CAS = ("d_consts", "theta", "stats", "set_base", "x0", "prev_a0", "leader", "sigma", "delay", "drop_q", "noise_seed", "abc", "gains",
        "counters", "metrics", "basis", "spectrum")


def _cases_call(lay=None, G=2, K=3, L=5, M=5, T=10, n_sets=10, sample_rate=0.1, scale=0.5, **ptrs):
    p = _ptrs(_CAS, ptrs)
    lay = _hip.make_layout(4, 1, 256, 128, 48, 64) if lay is None else lay
    _hip.call("avd_eval_cases_freq_f32", ctypes.byref(lay), p["d_consts"], G, K, L, M, T, p["theta"], p["stats"], n_sets, p["set_base"],
              p["x0"], p["prev_a0"], p["leader"], 2.5, -2.5, 2.5, sample_rate, p["sigma"], p["delay"], p["drop_q"], p["noise_seed"], p["abc"],
              p["gains"], scale, p["counters"], p["metrics"], p["basis"], p["spectrum"], None)


def test_frequency_entry_points_refuse_on_the_host_before_any_hip_call():
    """One fault per call, with status and message (no GPU here: a call that got past its checks would fail with a HIP error instead)."""
    refuse = lambda code, msg: pytest.raises(_hip.AvdError, match=rf"failed \({code}\): {msg}")
    nominal = {t: None for t in _TABLES}
    who = "avd_eval_linear_freq_f32"
    for kw in ({}, nominal):  # disturbed and nominal alike
        with refuse(-1, rf"{who}: basis=\(nil\) \(must be a non-null, 8-byte aligned"):
            _linear_call(basis=None, **kw)
        with refuse(-1, rf"{who}: basis=0x1004 \(must be a non-null, 8-byte aligned"):
            _linear_call(basis=ctypes.c_void_p(0x1004), **kw)
        with refuse(-1, f"{who}: null spectrum"):
            _linear_call(spectrum=None, **kw)
    # everything the twin refuses, under the new name
    for name in ("d_consts", "gains", "x0", "prev_a0", "leader", "counters"):
        with refuse(-1, f"{who}: null pointer"):
            _linear_call(**{name: None})
    for L in (0, 17):
        with refuse(-1, rf"{who}: L={L} \(L must be 1..16\)"):
            _linear_call(L=L)
    with refuse(-1, rf"{who}: G=2 K=3 T=0 \(all must be >= 1\)"):
        _linear_call(T=0)
    with refuse(-1, f"{who}: sample_rate="):
        _linear_call(sample_rate=0.0)
    with refuse(-1, f"{who}: null disturbance table"):
        _linear_call(delay=None)
    with refuse(-1, f"{who}: null disturbance table"):
        _linear_call(sigma=None, delay=None, drop_q=None, noise_seed=None)
    big = 2 ** 31 - 1
    with refuse(-3, rf"{who}: G={big} x K={big} = {big * big} rollouts"):
        _linear_call(G=big, K=big)
    who = "avd_eval_cases_freq_f32"
    for kw in ({}, nominal, dict(gains=None), dict(gains=None, **nominal)):  # disturbed / nominal, with and without a residual law
        with refuse(-1, rf"{who}: basis=\(nil\) \(must be a non-null, 8-byte aligned"):
            _cases_call(basis=None, **kw)
        with refuse(-1, rf"{who}: basis=0x1004 \(must be"):
            _cases_call(basis=ctypes.c_void_p(0x1004), **kw)
        with refuse(-1, f"{who}: null spectrum"):
            _cases_call(spectrum=None, **kw)
    for name in ("d_consts", "theta", "stats", "set_base", "x0", "prev_a0", "leader", "counters"):
        with refuse(-1, f"{who}: null"):
            _cases_call(**{name: None})
    with refuse(-1, rf"{who}: L=17 \(L must be 1..16\)"):
        _cases_call(L=17, M=17)
    with refuse(-1, rf"{who}: M=2 \(M must be L=5"):
        _cases_call(M=2)
    with refuse(-1, rf"{who}: G=2 K=0 T=10"):
        _cases_call(K=0)
    with refuse(-1, f"{who}: null disturbance table"):
        _cases_call(noise_seed=None)
    with refuse(-1, rf"{who}: gains=0x[0-9a-f]*8 \(must be a non-null, 16-byte aligned"):
        _cases_call(gains=ctypes.c_void_p(0x2008))
    with refuse(-1, rf"{who}: scale=1.5 \(must be in \(0, 1\]\)"):
        _cases_call(scale=1.5)
    cen = _hip.make_layout(20, 5, 320, 160, 64, 64)
    with refuse(-3, rf"{who}: M=1 L=5 \(a residual on a per-vehicle law needs decentralized agents"):
        _cases_call(lay=cen, M=1)
    with refuse(-1, rf"{who}: basis=\(nil\)"):  # without a law the centralized form passes the law's checks (scale unread) and reaches the sweep's
        _cases_call(lay=cen, M=1, gains=None, scale=7.0, basis=None)
    with refuse(-3, rf"{who}: hidden sizes need \d+ B of LDS for blocks of \d+ cases"):
        _cases_call(lay=_hip.make_layout(4, 1, 8192, 4096, 48, 64), K=16, **nominal)
