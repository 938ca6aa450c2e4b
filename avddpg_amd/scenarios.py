"""Leader-input scenarios and per-vehicle control metrics of the scenario evaluator (host only: numpy, no device).

The reference's evaluator loops over an ``input_opts`` dict "for a variety of input responses" (workers/evaluator.py:55-70) and its
Config names ``zerofig_name``, ``stepfig_name``, ``rampfig_name`` beside ``guasfig_name``; only the Gaussian entry was filled in.
``leader_profile`` fills in the rest; ``metrics_from_traces`` defines, in float32 numpy, the metrics avd_eval_cases_f32
(csrc/evalx.hip) reduces on the device -- from a trace dict as ``evaluator.run`` / ``run_many`` return it, bit for bit."""
import math

import numpy as np

SCENARIOS = ("gaussian", "zero", "step", "ramp", "brake", "sine")
METRICS = ("max_abs_ep", "max_abs_ev", "max_abs_a", "sum_u2", "sum_jerk2", "term_steps", "first_term", "final_abs_ep")  # AVD_EVAL_NMETRIC


def check_names(names):
    """The scenario names as a list; an unknown name, a name listed twice or an empty list is a ValueError."""
    names = [str(n) for n in ([names] if isinstance(names, str) else names)]
    if not names:
        raise ValueError("no scenario named")
    for n in names:
        if n not in SCENARIOS:
            raise ValueError(f"unknown scenario {n!r}: one of {', '.join(SCENARIOS)}")
    dup = sorted({n for n in names if names.count(n) > 1})
    if dup:
        raise ValueError(f"scenario(s) {dup} listed more than once")
    return names


def check_knobs(T, amp, period_s):
    """amp (None: the caller's default) and period_s as floats; non-finite values, period_s <= 0 or T < 4 are a ValueError."""
    if int(T) < 4:
        raise ValueError(f"T={T}: a scenario needs at least 4 steps (the profiles switch at T // 4)")
    if amp is not None and not math.isfinite(float(amp)):
        raise ValueError(f"amp={amp} is not finite")
    period_s = float(period_s)
    if not math.isfinite(period_s) or period_s <= 0:
        raise ValueError(f"period_s={period_s} must be finite and > 0")
    return (None if amp is None else float(amp)), period_s


def leader_profile(name, T, conf, amp=None, period_s=10.0, seed=None):
    """The leader's input over T steps, float32 [T], computed in float64 and rounded once. With k the step and q = T // 4:
    zero: 0; step: amp for k >= q; ramp: amp * clip((k - q) / q, 0, 1); brake: -amp for q <= k < 2q; sine: amp * sin(2 pi k
    sample_rate / period_s); gaussian: the reference's draws for evaluation seed ``seed`` (default conf.evaluation_seed), exactly as
    evaluator._start makes them (the only profile that depends on the seed; the caller's np.random state is restored).
    amp defaults to conf.reset_max_u, the scale of leader input the actors are trained on (workers/trainer.py:291-295)."""
    (name,) = check_names([name])
    T = int(T)
    amp, period_s = check_knobs(T, amp, period_s)
    amp = float(conf.reset_max_u) if amp is None else amp
    if name == "gaussian":
        # evaluator._start's draws, restated on the host alone: seed the legacy RNG, the evaluator platoon's two constructor draws
        # (front_accel, front_u: an evaluator platoon draws no states), then the T leader inputs (workers/evaluator.py:47, 55-56)
        rand = (lambda s: np.random.uniform(-s, s)) if conf.rand_gen == conf.uniform else (lambda s: np.random.normal(0, s))
        saved = np.random.get_state()
        try:
            np.random.seed(conf.evaluation_seed if seed is None else seed)
            rand(conf.pl_leader_reset_a), rand(conf.reset_max_u)
            return np.array([rand(conf.reset_max_u) for _ in range(T)], dtype=np.float32)
        finally:
            np.random.set_state(saved)
    k = np.arange(T, dtype=np.float64)
    q = T // 4
    if name == "zero":
        u = np.zeros(T)
    elif name == "step":
        u = np.where(k >= q, amp, 0.0)
    elif name == "ramp":
        u = amp * np.clip((k - q) / q, 0.0, 1.0)
    elif name == "brake":
        u = np.where((k >= q) & (k < 2 * q), -amp, 0.0)
    else:
        u = amp * np.sin(2.0 * np.pi * k * float(conf.sample_rate) / period_s)
    return u.astype(np.float32)


def metrics_from_traces(traces, x0, conf):
    """The eight metrics per vehicle, {name: float32 [L]}, from one rollout's trace dict (``states`` [T, L, >= 3] post-step
    observations, ``inputs`` [T, L] clipped actions, ``jerks`` [T, L]) and its start state x0 [L, >= 2]. float32 throughout; the sums
    are sequential adds in step order with the product rounded first (s = s + u * u, no fused multiply-add), so a device loop without
    contraction reproduces them bit for bit. The terminal test is on the PRE-step state (x0, then the previous step's post-step state),
    as the environment forms it; the evaluator does not stop on it. Maxima ignore NaN (fmax), as the device's do."""
    st = np.asarray(traces["states"], dtype=np.float32)
    u = np.asarray(traces["inputs"], dtype=np.float32)
    jk = np.asarray(traces["jerks"], dtype=np.float32)
    T, L = u.shape
    if st.shape[2] < 3:
        raise ValueError(f"states of width {st.shape[2]}: the metrics need ep, ev and a")
    x0 = np.asarray(x0, dtype=np.float32).reshape(L, -1)
    zero = np.zeros(L, dtype=np.float32)
    ab = np.abs(st)
    mx = [np.fmax.reduce(np.concatenate([zero[None], ab[:, :, c]]), axis=0) for c in range(3)]
    su2, sj2 = zero.copy(), zero.copy()
    for t in range(T):
        su2 = su2 + u[t] * u[t]
        sj2 = sj2 + jk[t] * jk[t]
    pre = np.concatenate([x0[None, :, :2], st[:-1, :, :2]])  # [T, L, 2] pre-step ep, ev
    term = ((np.abs(pre[..., 0]) > np.float32(conf.max_ep)) | (np.abs(pre[..., 1]) > np.float32(conf.max_ev))) & bool(conf.can_terminate)
    first = np.where(term.any(axis=0), term.argmax(axis=0), -1).astype(np.float32)
    out = dict(max_abs_ep=mx[0], max_abs_ev=mx[1], max_abs_a=mx[2], sum_u2=su2, sum_jerk2=sj2,
               term_steps=term.sum(axis=0).astype(np.float32), first_term=first, final_abs_ep=ab[-1, :, 0].copy())
    return {k: np.asarray(out[k], dtype=np.float32) for k in METRICS}


def summarise(metrics, T):
    """Derived values from a metrics dict whose arrays end in the vehicle axis [..., L]: rms_u = sqrt(sum_u2 / T), rms_jerk =
    sqrt(sum_jerk2 / T), ss_ratio [..., L] = max_abs_ep[i] / max_abs_ep[i - 1] for i >= 1 (NaN for the first vehicle, and where
    the predecessor's peak is 0), string_stable [...] = every defined ratio <= 1."""
    ep = np.asarray(metrics["max_abs_ep"], dtype=np.float32)
    ratio = np.full(ep.shape, np.nan, dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio[..., 1:] = np.where(ep[..., :-1] > 0, ep[..., 1:] / ep[..., :-1], np.float32(np.nan))
        defined = ~np.isnan(ratio)
        stable = np.all(~defined | (ratio <= 1), axis=-1)
    return dict(rms_u=np.sqrt(np.asarray(metrics["sum_u2"], dtype=np.float32) / np.float32(T)),
                rms_jerk=np.sqrt(np.asarray(metrics["sum_jerk2"], dtype=np.float32) / np.float32(T)),
                ss_ratio=ratio, string_stable=stable)


CSV_HEADER = ["platoon", "scenario", "seed", "vehicle", *METRICS, "rms_u", "rms_jerk", "ss_ratio", "score"]


def csv_rows(results, platoon_tags):
    """One row per (platoon, scenario, seed, vehicle) of a CaseResults ([P, scen, seed, ...] arrays): the eight metrics, rms_u, rms_jerk,
    ss_ratio (empty for the first vehicle) and the case's score, numbers written with repr(float) so that equal values give equal
    text. platoon_tags: the first column's value per platoon (1-based platoon numbers in the CLI)."""
    s = results.summary()
    f = lambda x: "" if np.isnan(x) else repr(float(x))
    rows = []
    for i, tag in enumerate(platoon_tags):
        for c, name in enumerate(results.scenarios):
            for k, seed in enumerate(results.seeds):
                for v in range(results.metrics[METRICS[0]].shape[-1]):
                    at = (i, c, k, v)
                    rows.append([tag, name, seed, v + 1, *[f(results.metrics[m][at]) for m in METRICS], f(s["rms_u"][at]),
                                 f(s["rms_jerk"][at]), f(s["ss_ratio"][at]), f(results.scores[i, c, k])])
    return rows


def write_csv(path, results, platoon_tags):
    import csv

    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(CSV_HEADER)
        w.writerows(csv_rows(results, platoon_tags))


# ---- frequency response: what the frequency entry points (avd_eval_cases_freq_f32, avd_eval_linear_freq_f32) reduce -----------------

NSPEC = 10  # AVD_EVAL_NSPEC
SIGNALS = ("ep", "ev", "a", "w", "u")  # a vehicle's (re, im) pairs, in this order
FREQUENCY_KEYS = ("fmin", "fmax", "n", "amp", "settle", "steps")
MAX_FREQUENCIES = 256
MIN_WINDOW = 8


class FrequencySpec:
    """A frequency sweep: ``n`` log-spaced frequencies from ``fmin`` to ``fmax`` (Hz), each a sinusoidal leader input of amplitude ``amp``
    (None: conf.reset_max_u) over ``steps`` steps (None: conf.steps_per_episode), measured over the last ``1 - settle`` of the rollout.
    With T = steps, t0 = floor(settle * T) and W = T - t0, a frequency is snapped to a whole number of cycles in the window (cycles =
    round(f * W * sample_rate), kept in 1 .. ceil(W / 2) - 1, duplicates dropped), so that the single-bin sum has no leakage; the
    frequency reported is cycles / (W * sample_rate)."""

    def __init__(self, fmin, fmax, n, amp=None, settle=0.5, steps=None, text=None):
        self.fmin, self.fmax, self.n, self.amp, self.settle, self.steps, self.text = fmin, fmax, n, amp, settle, steps, text

    def window(self, conf):
        """-> (T, t0, W), checked."""
        check_frequency(self, conf)
        T = int(conf.steps_per_episode if self.steps is None else self.steps)
        t0 = int(math.floor(float(self.settle) * T))
        return T, t0, T - t0

    def cycles(self, conf):
        """int64 [F]: the snapped cycle counts, ascending, without duplicates."""
        _, _, W = self.window(conf)
        f = np.geomspace(float(self.fmin), float(self.fmax), int(self.n)) if int(self.n) > 1 else np.array([float(self.fmin)])
        c = np.clip(np.rint(f * W * float(conf.sample_rate)), 1, -(-W // 2) - 1).astype(np.int64)
        return np.unique(c)

    def freqs_hz(self, conf):
        """float64 [F]: the frequencies actually driven, cycles / (W * sample_rate)."""
        _, _, W = self.window(conf)
        return self.cycles(conf) / (W * float(conf.sample_rate))

    def items(self):
        return [[k, getattr(self, k)] for k in FREQUENCY_KEYS]

    def __repr__(self):
        return "FrequencySpec(" + ", ".join(f"{k}={v!r}" for k, v in self.items()) + ")"


def check_frequency(spec, conf=None):
    """The spec, checked. A ValueError for: not a FrequencySpec; a non-finite value; fmin <= 0 or fmin > fmax; n no integer in 1 ..
    MAX_FREQUENCIES; settle outside [0, 1); steps no integer >= 1; a window W = T - floor(settle * T) < MIN_WINDOW (with ``conf``, or
    with steps given)."""
    if not isinstance(spec, FrequencySpec):
        raise ValueError(f"{spec!r} is not a scenarios.FrequencySpec")
    num = lambda v: not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and math.isfinite(v)
    whole = lambda v: not isinstance(v, bool) and isinstance(v, (int, np.integer))
    for k in ("fmin", "fmax", "settle"):
        if not num(getattr(spec, k)):
            raise ValueError(f"frequency: {k}={getattr(spec, k)!r} must be a finite number")
    if spec.amp is not None and not num(spec.amp):
        raise ValueError(f"frequency: amp={spec.amp!r} must be a finite number")
    if spec.fmin <= 0 or spec.fmin > spec.fmax:
        raise ValueError(f"frequency: fmin={spec.fmin!r} fmax={spec.fmax!r} (need 0 < fmin <= fmax)")
    if not whole(spec.n) or not 1 <= spec.n <= MAX_FREQUENCIES:
        raise ValueError(f"frequency: n={spec.n!r} must be an integer in 1..{MAX_FREQUENCIES}")
    if not 0 <= spec.settle < 1:
        raise ValueError(f"frequency: settle={spec.settle!r} must be in [0, 1)")
    if spec.steps is not None and (not whole(spec.steps) or spec.steps < 1):
        raise ValueError(f"frequency: steps={spec.steps!r} must be an integer >= 1")
    T = spec.steps if spec.steps is not None else (None if conf is None else int(conf.steps_per_episode))
    if T is not None:
        W = int(T) - int(math.floor(float(spec.settle) * int(T)))
        if W < MIN_WINDOW:
            raise ValueError(f"frequency: a window of W={W} steps (T={T}, settle={spec.settle!r}): need W >= {MIN_WINDOW}")
    return spec


def parse_frequency(text):
    """``fmin=0.02,fmax=2,n=16[,amp=A,settle=0.5,steps=N]`` -> FrequencySpec, checked by check_frequency. An unknown key, a key given
    twice, a missing fmin / fmax / n or a value that is no number is a ValueError."""
    kw = {}
    for part in [q.strip() for q in str(text).split(",") if q.strip()]:
        key, eq, val = part.partition("=")
        key, val = key.strip(), val.strip()
        if not eq or key not in FREQUENCY_KEYS:
            raise ValueError(f"frequency: unknown key {key!r} (one of {', '.join(FREQUENCY_KEYS)}, as key=value)")
        if key in kw:
            raise ValueError(f"frequency: {key} given twice")
        try:
            kw[key] = int(val) if key in ("n", "steps") else float(val)
        except ValueError:
            raise ValueError(f"frequency: {key}={val!r} is not {'an integer' if key in ('n', 'steps') else 'a number'}") from None
    missing = [k for k in ("fmin", "fmax", "n") if k not in kw]
    if missing:
        raise ValueError(f"frequency {text!r}: {', '.join(missing)} missing (fmin=..,fmax=..,n=..[,amp=..,settle=..,steps=..])")
    return check_frequency(FrequencySpec(text=str(text).strip(), **kw))


def _frequency_angle(spec, conf):
    """float64 [F, T]: 2 pi cycles (k - t0) / W, and t0."""
    T, t0, W = spec.window(conf)
    k = np.arange(T, dtype=np.float64)
    return 2.0 * np.pi * spec.cycles(conf)[:, None].astype(np.float64) * (k[None, :] - t0) / W, t0


def frequency_leader(spec, conf):
    """float32 [F, T]: the leader's input per frequency, amp * sin(2 pi cycles (k - t0) / W) for every step k (the sinusoid runs through
    the settling steps too), computed in float64 and rounded once, as leader_profile does. amp defaults to conf.reset_max_u."""
    ang, _ = _frequency_angle(spec, conf)
    amp = float(conf.reset_max_u if spec.amp is None else spec.amp)
    return np.ascontiguousarray((amp * np.sin(ang)).astype(np.float32))


def frequency_basis(spec, conf):
    """float32 [F, T, 2]: (cos, sin) of the leader's angle for the steps k >= t0 of the window and (0, 0) before: the window is in the
    table, the device loop has no branch on t0. float64, rounded once."""
    ang, t0 = _frequency_angle(spec, conf)
    out = np.stack([np.cos(ang), np.sin(ang)], axis=-1)
    out[:, :t0] = 0.0
    return np.ascontiguousarray(out.astype(np.float32))


def spectrum_from_traces(traces, basis_row):
    """The ten single-bin Fourier sums per vehicle, float32 [L, NSPEC] -- (re, im) of ep, ev, a, w, u -- from one rollout's trace dict as
    ``evaluator.run_many`` returns it (``states`` [T, L, >= 3] post-step states, ``inputs`` [T, L] plant inputs) and the case's basis
    row [T, 2]: per step, re = re + x * c and im = im + x * s in float32, the product rounded first, sequential adds in step order -- what
    the frequency entry points accumulate, bit for bit. Traces of width 3 (Model A's hide w) leave the w pair NaN."""
    st = np.asarray(traces["states"], dtype=np.float32)
    u = np.asarray(traces["inputs"], dtype=np.float32)
    b = np.asarray(basis_row, dtype=np.float32)
    T, L = u.shape
    if b.shape != (T, 2) or st.shape[:2] != (T, L) or st.shape[2] < 3:
        raise ValueError(f"states {st.shape}, inputs {u.shape}, basis {b.shape}: need [T, L, >= 3], [T, L], [T, 2]")
    sig = [st[:, :, c] for c in range(min(4, st.shape[2]))]
    if len(sig) < 4:
        sig.append(None)
    sig.append(u)
    out = np.zeros((L, NSPEC), dtype=np.float32)
    for i, x in enumerate(sig):
        if x is None:
            out[:, 2 * i:2 * i + 2] = np.nan
            continue
        re, im = np.zeros(L, dtype=np.float32), np.zeros(L, dtype=np.float32)
        for t in range(T):
            re = re + x[t] * b[t, 0]
            im = im + x[t] * b[t, 1]
        out[:, 2 * i], out[:, 2 * i + 1] = re, im
    return out


def _ratio(num, den):
    """num / den (complex), NaN where den is 0 or either is NaN."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((np.abs(den) > 0) & ~np.isnan(num), num / np.where(den == 0, 1, den), np.nan + 0j)


def _gains_of(X):
    """complex [..., L, 5] -> (gain_a, gain_ep, phase_a) float64 [..., L] by the rules of frequency_summary."""
    a, w, ep = X[..., 2], X[..., 3], X[..., 0]
    ra = np.concatenate([_ratio(a[..., :1], w[..., :1]), _ratio(a[..., 1:], a[..., :-1])], axis=-1)
    rep = np.concatenate([np.full_like(ep[..., :1], np.nan), _ratio(ep[..., 1:], ep[..., :-1])], axis=-1)
    return np.abs(ra), np.abs(rep), np.angle(ra)


def _peaks(gain_a, freqs_hz, axis):
    """Per vehicle the largest defined gain_a over the frequency axis, its index (-1: none defined) and frequency, and string_stable."""
    g = np.moveaxis(np.asarray(gain_a, dtype=np.float64), axis, 0)
    defined = ~np.isnan(g)
    filled = np.where(defined, g, -np.inf)
    idx = np.where(defined.any(axis=0), filled.argmax(axis=0), -1)
    peak = np.where(idx >= 0, np.take_along_axis(filled, np.maximum(idx, 0)[None], axis=0)[0], np.nan)
    out = dict(peak_gain_a=peak, peak_index=idx, string_stable=np.all(np.isnan(peak) | (peak <= 1), axis=-1))
    if freqs_hz is not None:
        out["peak_freq_hz"] = np.where(idx >= 0, np.asarray(freqs_hz, dtype=np.float64)[np.maximum(idx, 0)], np.nan)
    return out


def frequency_summary(spectrum, W, freqs_hz=None, axis=0):
    """Derived values from raw sums [..., L, NSPEC] whose axis ``axis`` is the frequency axis, in float64: the complex amplitudes X =
    (2 / W) (re - j im) as ``amp`` and ``phase`` [..., L, 5] (SIGNALS order); gain_a[i] = |A_i| / |A_{i-1}|, vehicle 0 against its own w
    (the leader's acceleration as its model holds it); gain_ep[i] = |EP_i| / |EP_{i-1}|, NaN for vehicle 0; phase_a the angle of
    gain_a's ratio; a ratio is NaN where its denominator is 0. Per vehicle, peak_gain_a over the frequency axis, its peak_index and
    (with ``freqs_hz``) peak_freq_hz; string_stable [...] is True when every defined peak is <= 1.
    The states are sampled post-step and u pre-step, against the angle of the step: every state carries one step's phase lead over u.
    The magnitudes, and the ratios between states, do not depend on it."""
    sp = np.asarray(spectrum, dtype=np.float64)
    if sp.shape[-1] != NSPEC:
        raise ValueError(f"spectrum of shape {sp.shape}: the last axis holds the {NSPEC} sums")
    X = (2.0 / float(W)) * (sp[..., 0::2] - 1j * sp[..., 1::2])
    ga, gep, pa = _gains_of(X)
    out = dict(amp=np.abs(X), phase=np.angle(X), gain_a=ga, gain_ep=gep, phase_a=pa)
    out.update(_peaks(ga, freqs_hz, axis))
    return out


def linear_frequency_response(conf, gains, cycles, W, dyn_coeff=None):
    """The float64 THEORY of an unclipped linear law on the nominal observation: per frequency z = exp(2 pi j cycles / W) and vehicle i,
    X_i = (z I - A_i - B_i g_i^T)^-1 C_i exog_i with exog_0 = 1 (the leader's input), and for i >= 1 exog_i = g_{i-1}^T X_{i-1} under
    Model B (the predecessor's plant input) or the predecessor's post-step acceleration z X_{i-1}[2] under Model A (whose law reads the
    first three states only). gains [L, 4]; the matrices are dynamics.system_matrices with env_consts' tau chaining and every follower's
    engine lag ``dyn_coeff`` (None: conf.dyn_coeff). -> dict(X complex [F, L, 5] (SIGNALS order, per unit leader input), gain_a, gain_ep,
    phase_a [F, L], and frequency_summary's peaks over the frequency axis)."""
    from . import dynamics

    g = np.asarray(gains, dtype=np.float64)
    L = int(conf.pl_size)
    if g.shape != (L, 4):
        raise ValueError(f"gains of shape {g.shape}: need [{L}, 4]")
    model_a = conf.model == conf.modelA
    if model_a:
        g = g * np.array([1.0, 1.0, 1.0, 0.0])
    tau = float(conf.dyn_coeff if dyn_coeff is None else dyn_coeff)
    cyc = np.atleast_1d(np.asarray(cycles, dtype=np.float64))
    X = np.zeros((cyc.shape[0], L, 5), dtype=np.complex128)
    for f, c in enumerate(cyc):
        z = np.exp(2j * np.pi * c / float(W))
        exog = 1.0 + 0j
        for i in range(L):
            A, B, Cm = dynamics.system_matrices(conf.method, conf.sample_rate, tau, conf.pl_leader_tau if i == 0 else tau, conf.timegap)
            x = np.linalg.solve(z * np.eye(4) - A - np.outer(B, g[i]), Cm * exog)
            u = g[i] @ x
            X[f, i, :4], X[f, i, 4] = x, u
            exog = z * x[2] if model_a else u
    ga, gep, pa = _gains_of(X)
    out = dict(X=X, gain_a=ga, gain_ep=gep, phase_a=pa)
    out.update(_peaks(ga, None, 0))
    return out


FREQUENCY_HEADER = ["controller", "disturbance", "seed", "freq_hz", "cycles", "vehicle", *[f"amp_{n}" for n in SIGNALS],
                    *[f"phase_{n}" for n in SIGNALS], "gain_a", "gain_ep", "phase_a", "gain_a_theory"]


def frequency_rows(results, tags, theory=None):
    """One row per (controller, disturbance, seed, frequency, vehicle) of a FrequencyResults (spectrum [G, F, ND, NS, L, NSPEC]): the
    frequency driven and its cycle count, the five amplitudes and phases, gain_a, gain_ep, phase_a and gain_a_theory -- ``theory``
    float64 [G, ND, F, L] for laws (linear_frequency_response with each level's dyn_coeff), None for actors: the column stays empty.
    Numbers are written with repr(float); a NaN is an empty field. tags: the first column's value per controller."""
    s = results.summary()
    f = lambda x: "" if np.isnan(x) else repr(float(x))
    rows = []
    for i, tag in enumerate(tags):
        for d, level in enumerate(results.disturbances):
            for k, seed in enumerate(results.seeds):
                for q, hz in enumerate(results.freqs_hz):
                    for v in range(results.spectrum.shape[-2]):
                        at = (i, q, d, k, v)
                        rows.append([tag, level, seed, repr(float(hz)), int(results.cycles[q]), v + 1, *[f(x) for x in s["amp"][at]],
                                     *[f(x) for x in s["phase"][at]], f(s["gain_a"][at]), f(s["gain_ep"][at]), f(s["phase_a"][at]),
                                     "" if theory is None else f(theory[i, d, q, v])])
    return rows


def write_frequency_csv(path, entries):
    """frequency.csv: entries is a list of (results, tags, theory) as frequency_rows takes them (the actors', then the laws')."""
    import csv

    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(FREQUENCY_HEADER)
        for results, tags, theory in entries:
            w.writerows(frequency_rows(results, tags, theory))


def frequency_peaks(results, tags):
    """[[controller, level, peak gain_a, its frequency (Hz), its vehicle (1-based), string_stable]] per controller and level: gain_a is
    averaged over the seeds first, then the peak is taken over frequencies and vehicles."""
    ga = results.summary()["gain_a"]
    n = np.sum(~np.isnan(ga), axis=3)
    g = np.where(n > 0, np.nansum(ga, axis=3) / np.maximum(n, 1), np.nan)  # [G, F, ND, L]: the mean of the defined seeds
    out = []
    for i, tag in enumerate(tags):
        for d, level in enumerate(results.disturbances):
            p = _peaks(g[i, :, d], results.freqs_hz, 0)
            if np.all(np.isnan(p["peak_gain_a"])):
                out.append([tag, level, None, None, None, bool(p["string_stable"])])
                continue
            v = int(np.nanargmax(p["peak_gain_a"]))
            out.append([tag, level, float(p["peak_gain_a"][v]), float(p["peak_freq_hz"][v]), v + 1, bool(p["string_stable"])])
    return out


def frequency_report_lines(results, tags, what="platoon"):
    """One line per controller and level: the peak gain_a, where it is and whether the string is stable."""
    return [f"{what} {tag} {level}: peak gain_a " + ("undefined" if pk is None else f"{pk:.4f} at {hz:.4f} Hz (vehicle {v})") +
            f" string_stable {ok}" for tag, level, pk, hz, v, ok in frequency_peaks(results, tags)]


# ---- disturbances: what the disturbed scenario evaluator (avd_eval_cases_dist_f32) applies per case ---------------------------------

MAX_DELAY = 15  # AVD_EVAL_MAX_DELAY
DISTURBANCE_KEYS = ("noise_ep", "noise_ev", "noise_a", "v2v_delay", "v2v_drop", "dyn_coeff")


class Disturbance:
    """One robustness level: sensor-noise standard deviations on the observed ep, ev and a; a delay (steps) and a loss probability on the
    V2V link that carries the predecessor's acceleration (the 4th Model-B observation); the TRUE plant's engine lag ``dyn_coeff`` (None:
    the configuration's) while the actors stay those trained on the configuration's. Rewards and metrics come from the true state."""

    def __init__(self, name, noise_ep=0, noise_ev=0, noise_a=0, v2v_delay=0, v2v_drop=0.0, dyn_coeff=None):
        self.name = str(name)
        self.noise_ep, self.noise_ev, self.noise_a = noise_ep, noise_ev, noise_a
        self.v2v_delay, self.v2v_drop, self.dyn_coeff = v2v_delay, v2v_drop, dyn_coeff

    @property
    def sigma(self):
        return (float(self.noise_ep), float(self.noise_ev), float(self.noise_a))

    @property
    def uses_v2v(self):
        return self.v2v_delay != 0 or self.v2v_drop != 0

    def items(self):
        """[(key, value)] in DISTURBANCE_KEYS order (conf.json's robustness_suite)."""
        return [[k, getattr(self, k)] for k in DISTURBANCE_KEYS]

    def __repr__(self):
        return "Disturbance(" + ", ".join([repr(self.name)] + [f"{k}={v!r}" for k, v in self.items()]) + ")"


NOMINAL = Disturbance("nominal")


def parse_disturbance(text):
    """``NAME:key=val,...`` (keys of DISTURBANCE_KEYS) -> Disturbance; ``NAME`` alone is the null disturbance under that name. An unknown
    key, a key given twice or a value that is no number is a ValueError; the values are checked by check_disturbances."""
    name, _, spec = str(text).partition(":")
    name = name.strip()
    if not name:
        raise ValueError(f"disturbance {text!r}: no name before ':'")
    kw = {}
    for part in [q.strip() for q in spec.split(",") if q.strip()]:
        key, eq, val = part.partition("=")
        key, val = key.strip(), val.strip()
        if not eq or key not in DISTURBANCE_KEYS:
            raise ValueError(f"disturbance {name!r}: unknown key {key!r} (one of {', '.join(DISTURBANCE_KEYS)}, as key=value)")
        if key in kw:
            raise ValueError(f"disturbance {name!r}: {key} given twice")
        try:
            kw[key] = int(val) if key == "v2v_delay" else float(val)
        except ValueError:
            raise ValueError(f"disturbance {name!r}: {key}={val!r} is not {'an integer' if key == 'v2v_delay' else 'a number'}") from None
    return Disturbance(name, **kw)


def check_disturbances(disturbances, conf=None):
    """The disturbances as a list. A ValueError for: a non-finite or negative value; a delay outside 0..MAX_DELAY or not an integer; a
    drop outside [0, 1]; dyn_coeff <= 0; a name listed twice; the reserved name ``nominal``; with ``conf``, a V2V axis under Model A
    (its 3-state observation has no communicated component)."""
    out = list(disturbances)
    for d in out:
        if not isinstance(d, Disturbance):
            raise ValueError(f"{d!r} is not a scenarios.Disturbance")
        if d.name == NOMINAL.name:
            raise ValueError(f"the disturbance name {NOMINAL.name!r} is reserved for the undisturbed level")
        for k, v in d.items():
            if k == "dyn_coeff" and v is None:
                continue
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or v < 0:
                raise ValueError(f"disturbance {d.name!r}: {k}={v!r} must be a finite number >= 0")
        if d.v2v_delay != int(d.v2v_delay) or not 0 <= d.v2v_delay <= MAX_DELAY:
            raise ValueError(f"disturbance {d.name!r}: v2v_delay={d.v2v_delay!r} must be an integer in 0..{MAX_DELAY}")
        if d.v2v_drop > 1:
            raise ValueError(f"disturbance {d.name!r}: v2v_drop={d.v2v_drop!r} must be in [0, 1]")
        if d.dyn_coeff is not None and d.dyn_coeff <= 0:
            raise ValueError(f"disturbance {d.name!r}: dyn_coeff={d.dyn_coeff!r} must be > 0")
        if conf is not None and conf.model == conf.modelA and d.uses_v2v:
            raise ValueError(f"disturbance {d.name!r}: v2v_delay / v2v_drop need Model B (Model A observes no communicated state)")
    names = [d.name for d in out]
    dup = sorted({n for n in names if names.count(n) > 1})
    if dup:
        raise ValueError(f"disturbance(s) {dup} listed more than once")
    return out


def drop_threshold(v2v_drop):
    """drop_q = round(v2v_drop * 2^24): the device drops a V2V sample iff (philox word >> 8) < drop_q, an integer compare (0: never,
    2^24: always)."""
    return int(round(float(v2v_drop) * (1 << 24)))


def plant_table(conf, L, dyn_coeff=None):
    """float32 [L, 24] -- A (16, row-major), B (4), C (4) per vehicle -- of a platoon whose followers all have engine lag ``dyn_coeff``
    (default conf.dyn_coeff): dynamics.system_matrices in float64 with the tau chaining of dynamics.env_consts (vehicle 0 follows
    pl_leader_tau, vehicle i >= 1 its predecessor's lag), rounded to float32 once as env_consts rounds."""
    from . import dynamics

    tau = float(conf.dyn_coeff if dyn_coeff is None else dyn_coeff)
    out = np.zeros((L, 24), dtype=np.float32)
    for i in range(L):
        A, B, Cm = dynamics.system_matrices(conf.method, conf.sample_rate, tau, conf.pl_leader_tau if i == 0 else tau, conf.timegap)
        if conf.model == conf.modelA and Cm[2] != 0.0:
            raise ValueError("Model A chain needs C[2] == 0 (acceleration row independent of the exogenous input)")
        out[i] = np.concatenate([A.ravel(), B, Cm]).astype(np.float32)
    return out


# ---- linear baselines: what the linear scenario evaluator (avd_eval_linear_f32) runs in place of the actors --------------------------

MAX_BASELINES = 16
MAX_GRID = 65536
GAIN_KEYS = ("kp", "kv", "ka", "kf")
TUNED = "tuned"  # the name --baseline_tune gives the grid's best law


class LinearLaw:
    """One static feedback law per vehicle, u = clip(kp * ep + kv * ev + ka * a + kf * a_pred, action_low, action_high) on the observed
    state: the constant-time-headway controller of the platooning literature (ep already holds the headway term), with the
    predecessor's communicated acceleration as feed-forward under Model B. ``table`` ([L][4], one (kp, kv, ka, kf) row per vehicle)
    overrides the four scalars."""

    def __init__(self, name, kp=0, kv=0, ka=0, kf=0, table=None):
        self.name = str(name)
        self.kp, self.kv, self.ka, self.kf = kp, kv, ka, kf
        self.table = None if table is None else np.asarray(table)

    def items(self):
        """[(key, value)] in GAIN_KEYS order (conf.json's baseline_suite), then the table when there is one."""
        out = [[k, getattr(self, k)] for k in GAIN_KEYS]
        return out if self.table is None else out + [["table", np.asarray(self.table, dtype=np.float64).tolist()]]

    def gains(self, L):
        """float32 [L, 4]: the table, or the scalars repeated for every vehicle."""
        if self.table is not None:
            t = np.asarray(self.table, dtype=np.float32)
            if t.shape != (int(L), 4):
                raise ValueError(f"baseline {self.name!r}: a gain table of shape {t.shape} for a platoon of {L} (need [{L}, 4])")
            return np.ascontiguousarray(t)
        return np.ascontiguousarray(np.tile(np.array([self.kp, self.kv, self.ka, self.kf], dtype=np.float32), (int(L), 1)))

    def __repr__(self):
        return "LinearLaw(" + ", ".join([repr(self.name)] + [f"{k}={v!r}" for k, v in self.items()]) + ")"


def parse_baseline(text):
    """``NAME[:key=val,...]`` (keys of GAIN_KEYS) -> LinearLaw; ``NAME`` alone is the zero law under that name. An unknown key, a key
    given twice or a value that is no number is a ValueError; the values are checked by check_baselines."""
    name, _, spec = str(text).partition(":")
    name = name.strip()
    if not name:
        raise ValueError(f"baseline {text!r}: no name before ':'")
    kw = {}
    for part in [q.strip() for q in spec.split(",") if q.strip()]:
        key, eq, val = part.partition("=")
        key, val = key.strip(), val.strip()
        if not eq or key not in GAIN_KEYS:
            raise ValueError(f"baseline {name!r}: unknown key {key!r} (one of {', '.join(GAIN_KEYS)}, as key=value)")
        if key in kw:
            raise ValueError(f"baseline {name!r}: {key} given twice")
        try:
            kw[key] = float(val)
        except ValueError:
            raise ValueError(f"baseline {name!r}: {key}={val!r} is not a number") from None
    return LinearLaw(name, **kw)


def check_baselines(laws, conf=None, reserved=(TUNED,)):
    """The laws as a list. A ValueError for: more than MAX_BASELINES; a non-finite gain or a gain that is no number; a table that is
    not [*, 4]; a name listed twice; the reserved name ``tuned``; with ``conf``, a non-zero kf under Model A (its 3-state observation
    has no communicated component), a table whose row count is not conf.pl_size, and the centralized framework (a linear law is per
    vehicle)."""
    out = list(laws)
    if len(out) > MAX_BASELINES:
        raise ValueError(f"{len(out)} baselines listed: at most {MAX_BASELINES}")
    if conf is not None and conf.framework == conf.cntrl:
        raise ValueError("a linear baseline is a per-vehicle law: not available for the centralized framework")
    for b in out:
        if not isinstance(b, LinearLaw):
            raise ValueError(f"{b!r} is not a scenarios.LinearLaw")
        if b.name in reserved:
            flag = "--baseline_search finds" if b.name == "searched" else "--baseline_tune picks"
            raise ValueError(f"the baseline name {b.name!r} is reserved for the law {flag}")
        for k in GAIN_KEYS:
            v = getattr(b, k)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
                raise ValueError(f"baseline {b.name!r}: {k}={v!r} must be a finite number")
        uses_kf = b.kf != 0
        if b.table is not None:
            t = np.asarray(b.table)
            if t.ndim != 2 or t.shape[1] != 4 or t.shape[0] < 1 or not np.issubdtype(t.dtype, np.number) or not np.isfinite(t).all():
                raise ValueError(f"baseline {b.name!r}: table must be a finite [L, 4] array (got shape {t.shape})")
            if conf is not None and t.shape[0] != conf.pl_size:
                raise ValueError(f"baseline {b.name!r}: a gain table of {t.shape[0]} rows for pl_size={conf.pl_size}")
            uses_kf = bool(np.any(t[:, 3] != 0))
        if conf is not None and conf.model == conf.modelA and uses_kf:
            raise ValueError(f"baseline {b.name!r}: kf needs Model B (Model A observes no communicated state)")
    names = [b.name for b in out]
    dup = sorted({n for n in names if names.count(n) > 1})
    if dup:
        raise ValueError(f"baseline(s) {dup} listed more than once")
    return out


# ---- residual policies: the actors correct a linear law (tr --residual; avd_step_fused_res_f32, avd_eval_*_res_f32) ------------------

RESIDUAL_NAME = "residual"


class ResidualLaw(LinearLaw):
    """A LinearLaw the actors are trained as a correction to: the plant receives u = clip(law(observed state) + scale * r, action_low,
    action_high) with r the agent's action. ``scale`` in (0, 1] is the residual's authority (1: the correction can span the whole
    action range). ``source`` records where the gains came from (conf.json's residual_law): "given" or "tuned"."""

    def __init__(self, kp=0, kv=0, ka=0, kf=0, table=None, scale=1.0, name=RESIDUAL_NAME, source="given"):
        super().__init__(name, kp, kv, ka, kf, table)
        self.scale, self.source = scale, str(source)

    def record(self):
        """conf.json's residual_law entry, a list of pairs (conf.json keeps lists, not dicts): the gains in GAIN_KEYS order, the scale,
        the table when there is one, the source."""
        out = [[k, float(getattr(self, k))] for k in GAIN_KEYS] + [["scale", float(self.scale)]]
        if self.table is not None:
            out.append(["table", np.asarray(self.table, dtype=np.float64).tolist()])
        return out + [["source", self.source]]

    @classmethod
    def from_record(cls, pairs):
        """The law of a conf.json's residual_law entry (None stays None); an unknown or repeated key is a ValueError."""
        if pairs is None:
            return None
        keys = [k for k, _ in pairs]
        bad = sorted({k for k in keys if k not in GAIN_KEYS + ("scale", "table", "source") or keys.count(k) > 1})
        if bad:
            raise ValueError(f"residual_law: unknown or repeated key(s) {bad}")
        d = dict(pairs)
        return cls(*(d.get(k, 0) for k in GAIN_KEYS), table=d.get("table"), scale=d.get("scale", 1.0), source=d.get("source", "given"))

    def __repr__(self):
        return "ResidualLaw(" + ", ".join([f"{k}={v!r}" for k, v in self.items()] + [f"scale={self.scale!r}"]) + ")"


def parse_residual(text):
    """``kp=2,kv=1[,ka=..,kf=..,scale=..]`` -> ResidualLaw, or the word ``tuned`` -> TUNED (the caller searches the gains). An unknown
    key, a key given twice, a value that is no number or an empty text is a ValueError; the values are checked by check_residual."""
    text = str(text).strip()
    if text == TUNED:
        return TUNED
    if text == SEARCHED:
        return SEARCHED
    keys = GAIN_KEYS + ("scale",)
    kw = {}
    parts = [q.strip() for q in text.split(",") if q.strip()]
    if not parts:
        raise ValueError(f"residual {text!r}: no gain given (kp=..,kv=..[,ka=..,kf=..,scale=..], or the word {TUNED!r})")
    for part in parts:
        key, eq, val = part.partition("=")
        key, val = key.strip(), val.strip()
        if not eq or key not in keys:
            raise ValueError(f"residual: unknown key {key!r} (one of {', '.join(keys)}, as key=value, or the word {TUNED!r})")
        if key in kw:
            raise ValueError(f"residual: {key} given twice")
        try:
            kw[key] = float(val)
        except ValueError:
            raise ValueError(f"residual: {key}={val!r} is not a number") from None
    return ResidualLaw(**kw)


def check_residual(law, conf=None):
    """The law, checked. A ValueError for: not a ResidualLaw; check_baselines' rules (a non-finite gain, a table that is not [*, 4];
    with ``conf`` a non-zero kf under Model A, a table whose row count is not conf.pl_size, the centralized framework); a scale that is
    no number in (0, 1]."""
    if not isinstance(law, ResidualLaw):
        raise ValueError(f"{law!r} is not a scenarios.ResidualLaw")
    check_baselines([law], conf, reserved=())
    sc = law.scale
    if isinstance(sc, bool) or not isinstance(sc, (int, float, np.integer, np.floating)) or not (0 < sc <= 1):
        raise ValueError(f"residual: scale={sc!r} must be a number in (0, 1]")
    return law


# ---- warm start: the actors are fitted to a linear law before training (tr --warm_start; avd_clone_sample_f32, avd_actor_clone_f32) ----

WARM_START_NAME = "warm_start"
WARM_START_MAX_STEPS = 100000
_WARM_KEYS = GAIN_KEYS + ("steps", "lr", "ep", "ev", "a")


class WarmStart(LinearLaw):
    """A LinearLaw the actors are fitted to before the first training step (imitation pre-training): ``steps`` Adam steps of size
    ``lr`` on batches of 64 states drawn uniformly in the box (ep, ev, a, a_pred) = +-(ep, ev, a, a), the target the law's clipped
    action. ``ep`` / ``ev`` / ``a`` left None take conf.reset_ep_max, conf.reset_max_ev and 1.0 (``a`` also bounds a_pred). ``source``
    records where the gains came from: "given", "tuned" or "searched"."""

    def __init__(self, kp=0, kv=0, ka=0, kf=0, table=None, steps=2000, lr=1e-3, ep=None, ev=None, a=None, name=WARM_START_NAME,
                 source="given"):
        super().__init__(name, kp, kv, ka, kf, table)
        self.steps, self.lr, self.ep, self.ev, self.a, self.source = steps, lr, ep, ev, a, str(source)

    def box(self, conf):
        """float32 [4]: the half-widths of (ep, ev, a, a_pred), the defaults filled in from ``conf``."""
        ep = conf.reset_ep_max if self.ep is None else self.ep
        ev = conf.reset_max_ev if self.ev is None else self.ev
        a = 1.0 if self.a is None else self.a
        return np.array([ep, ev, a, a], dtype=np.float32)

    def record(self):
        """conf.json's warm_start law, a list of pairs like ResidualLaw.record: the gains, steps, lr, the box half-widths that were
        given (a default is left out and comes back as None), the table when there is one, the source."""
        out = [[k, float(getattr(self, k))] for k in GAIN_KEYS] + [["steps", int(self.steps)], ["lr", float(self.lr)]]
        out += [[k, float(getattr(self, k))] for k in ("ep", "ev", "a") if getattr(self, k) is not None]
        if self.table is not None:
            out.append(["table", np.asarray(self.table, dtype=np.float64).tolist()])
        return out + [["source", self.source]]

    @classmethod
    def from_record(cls, pairs):
        """The spec of a conf.json's warm_start law (None stays None); an unknown or repeated key is a ValueError."""
        if pairs is None:
            return None
        keys = [k for k, _ in pairs]
        bad = sorted({k for k in keys if k not in _WARM_KEYS + ("table", "source") or keys.count(k) > 1})
        if bad:
            raise ValueError(f"warm_start: unknown or repeated key(s) {bad}")
        d = dict(pairs)
        return cls(*(d.get(k, 0) for k in GAIN_KEYS), table=d.get("table"), steps=d.get("steps", 2000), lr=d.get("lr", 1e-3),
                   ep=d.get("ep"), ev=d.get("ev"), a=d.get("a"), source=d.get("source", "given"))

    def with_gains(self, law, source):
        """This spec's fit settings around another law's gains (the tuned / searched law)."""
        return WarmStart(law.kp, law.kv, law.ka, law.kf, table=law.table, steps=self.steps, lr=self.lr, ep=self.ep, ev=self.ev, a=self.a,
                         source=source)

    def __repr__(self):
        return "WarmStart(" + ", ".join([f"{k}={v!r}" for k, v in self.items()] + [f"steps={self.steps!r}", f"lr={self.lr!r}"]) + ")"


def parse_warm_start(text):
    """``kp=2,kv=1[,ka=..,kf=..,steps=..,lr=..,ep=..,ev=..,a=..]`` -> WarmStart, or the words ``tuned`` / ``searched`` -> TUNED /
    SEARCHED (the caller takes the gains --baseline_tune / --baseline_search find), as parse_residual. An unknown key, a key given
    twice, a value that is no number or an empty text is a ValueError; the values are checked by check_warm_start."""
    text = str(text).strip()
    if text == TUNED:
        return TUNED
    if text == SEARCHED:
        return SEARCHED
    kw = {}
    parts = [q.strip() for q in text.split(",") if q.strip()]
    if not parts:
        raise ValueError(f"warm_start {text!r}: no gain given (kp=..,kv=..[,ka=..,kf=..,steps=..,lr=..,ep=..,ev=..,a=..], or the word "
                         f"{TUNED!r} / {SEARCHED!r})")
    for part in parts:
        key, eq, val = part.partition("=")
        key, val = key.strip(), val.strip()
        if not eq or key not in _WARM_KEYS:
            raise ValueError(f"warm_start: unknown key {key!r} (one of {', '.join(_WARM_KEYS)}, as key=value, or the word {TUNED!r} / "
                             f"{SEARCHED!r})")
        if key in kw:
            raise ValueError(f"warm_start: {key} given twice")
        try:
            kw[key] = float(val)
        except ValueError:
            raise ValueError(f"warm_start: {key}={val!r} is not a number") from None
    if "steps" in kw:
        if not math.isfinite(kw["steps"]) or kw["steps"] != int(kw["steps"]):
            raise ValueError(f"warm_start: steps={kw['steps']!r} is not a whole number")
        kw["steps"] = int(kw["steps"])
    return WarmStart(**kw)


def check_warm_start(spec, conf=None):
    """The spec, checked. A ValueError for: not a WarmStart; check_baselines' rules (a non-finite gain, a table that is not [*, 4];
    with ``conf`` a non-zero kf under Model A, a table whose row count is not conf.pl_size, the centralized framework); steps that is
    no whole number in 1 .. WARM_START_MAX_STEPS; an lr that is not a finite number > 0; a box half-width that is given and is not a
    finite number > 0."""
    if not isinstance(spec, WarmStart):
        raise ValueError(f"{spec!r} is not a scenarios.WarmStart")
    check_baselines([spec], conf, reserved=())
    st = spec.steps
    if isinstance(st, bool) or not isinstance(st, (int, np.integer)) or not (1 <= st <= WARM_START_MAX_STEPS):
        raise ValueError(f"warm_start: steps={st!r} must be a whole number in 1 .. {WARM_START_MAX_STEPS}")
    number = lambda v: not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and math.isfinite(v)
    if not number(spec.lr) or not spec.lr > 0:
        raise ValueError(f"warm_start: lr={spec.lr!r} must be a finite number > 0")
    for k in ("ep", "ev", "a"):
        v = getattr(spec, k)
        if v is not None and (not number(v) or not v > 0):
            raise ValueError(f"warm_start: {k}={v!r} must be a finite number > 0")
    if conf is not None:
        for k, v in zip(("ep", "ev", "a"), spec.box(conf)[:3]):
            if not (math.isfinite(float(v)) and v > 0):
                raise ValueError(f"warm_start: the box half-width {k}={float(v)!r} must be a finite number > 0")
    return spec


# ---- anchor: a behaviour-cloning term ties the actors to a linear law while they train (tr --anchor; avd_learn_set_split_anchor_f16x3) ----

ANCHOR_NAME = "anchor"
_ANCHOR_KEYS = GAIN_KEYS + ("weight", "decay")


class Anchor(LinearLaw):
    """A LinearLaw the actor loss is anchored to (TD3+BC's term): the actors minimise -q(s, mu(s)) + weight * (mu(s) - u*(s))^2 with u*
    the law's clipped action on the sampled state. ``decay`` (a whole number of learner calls, 0 = constant) ramps the weight linearly
    to 0 at that call. ``source`` records where the gains came from: "given", "tuned" or "searched"; ``pending`` is True for a spec
    parsed from the word ``tuned`` / ``searched`` whose gains the caller has yet to fill in (with_gains)."""

    def __init__(self, kp=0, kv=0, ka=0, kf=0, table=None, weight=1.0, decay=0, name=ANCHOR_NAME, source="given", pending=False):
        super().__init__(name, kp, kv, ka, kf, table)
        self.weight, self.decay, self.source, self.pending = weight, decay, str(source), bool(pending)

    def weight_at(self, call):
        """The float32 weight of learner call ``call`` (0-based): ``weight``, or with a decay weight * max(0, 1 - call / decay) --
        computed in float64 and rounded once."""
        w = float(self.weight)
        if self.decay:
            w = w * max(0.0, 1.0 - float(int(call)) / float(int(self.decay)))
        return float(np.float32(w))

    def record(self):
        """conf.json's anchor law, a list of pairs like ResidualLaw.record: the gains, the weight, the decay, the table when there is one,
        the source."""
        out = [[k, float(getattr(self, k))] for k in GAIN_KEYS] + [["weight", float(self.weight)], ["decay", int(self.decay)]]
        if self.table is not None:
            out.append(["table", np.asarray(self.table, dtype=np.float64).tolist()])
        return out + [["source", self.source]]

    @classmethod
    def from_record(cls, pairs):
        """The spec of a conf.json's anchor law (None stays None); an unknown or repeated key is a ValueError."""
        if pairs is None:
            return None
        keys = [k for k, _ in pairs]
        bad = sorted({k for k in keys if k not in _ANCHOR_KEYS + ("table", "source") or keys.count(k) > 1})
        if bad:
            raise ValueError(f"anchor: unknown or repeated key(s) {bad}")
        d = dict(pairs)
        return cls(*(d.get(k, 0) for k in GAIN_KEYS), table=d.get("table"), weight=d.get("weight", 1.0), decay=d.get("decay", 0),
                   source=d.get("source", "given"))

    def with_gains(self, law, source):
        """This spec's weight and decay around another law's gains (the tuned / searched law)."""
        return Anchor(law.kp, law.kv, law.ka, law.kf, table=law.table, weight=self.weight, decay=self.decay, source=source)

    def __repr__(self):
        return "Anchor(" + ", ".join([f"{k}={v!r}" for k, v in self.items()] + [f"weight={self.weight!r}", f"decay={self.decay!r}"]) + ")"


def parse_anchor(text):
    """``kp=2,kv=1[,ka=..,kf=..,weight=..,decay=..]`` -> Anchor. The word ``tuned`` / ``searched`` may stand in place of the gains,
    followed by the other keys (``tuned,weight=10``): the Anchor then has ``pending`` set and ``source`` that word, and the caller takes
    the gains --baseline_tune / --baseline_search find (with_gains). An unknown key, a key given twice, a gain beside the word, a value
    that is no number or an empty text is a ValueError; the values are checked by check_anchor."""
    text = str(text).strip()
    kw, word = {}, None
    parts = [q.strip() for q in text.split(",") if q.strip()]
    if not parts:
        raise ValueError(f"anchor {text!r}: no gain given (kp=..,kv=..[,ka=..,kf=..,weight=..,decay=..], or the word {TUNED!r} / "
                         f"{SEARCHED!r} in place of the gains)")
    if parts[0] in (TUNED, SEARCHED):
        word, parts = parts[0], parts[1:]
    for part in parts:
        key, eq, val = part.partition("=")
        key, val = key.strip(), val.strip()
        if not eq or key not in _ANCHOR_KEYS:
            raise ValueError(f"anchor: unknown key {key!r} (one of {', '.join(_ANCHOR_KEYS)}, as key=value; the word {TUNED!r} / "
                             f"{SEARCHED!r} may stand first, in place of the gains)")
        if word is not None and key in GAIN_KEYS:
            raise ValueError(f"anchor: {key} given beside the word {word!r} (the word stands in place of the gains)")
        if key in kw:
            raise ValueError(f"anchor: {key} given twice")
        try:
            kw[key] = float(val)
        except ValueError:
            raise ValueError(f"anchor: {key}={val!r} is not a number") from None
    if "decay" in kw:
        if not math.isfinite(kw["decay"]) or kw["decay"] != int(kw["decay"]):
            raise ValueError(f"anchor: decay={kw['decay']!r} is not a whole number")
        kw["decay"] = int(kw["decay"])
    if word is not None:
        return Anchor(source=word, pending=True, **kw)
    return Anchor(**kw)


def check_anchor(spec, conf=None):
    """The spec, checked. A ValueError for: not an Anchor; check_baselines' rules (a non-finite gain, a table that is not [*, 4]; with
    ``conf`` a non-zero kf under Model A, a table whose row count is not conf.pl_size, the centralized framework); a weight that is not
    a finite number >= 0; a decay that is no whole number >= 0."""
    if not isinstance(spec, Anchor):
        raise ValueError(f"{spec!r} is not a scenarios.Anchor")
    check_baselines([spec], conf, reserved=())
    w = spec.weight
    if isinstance(w, bool) or not isinstance(w, (int, float, np.integer, np.floating)) or not math.isfinite(w) or not w >= 0:
        raise ValueError(f"anchor: weight={w!r} must be a finite number >= 0")
    if float(w) > float(np.finfo(np.float32).max):
        raise ValueError(f"anchor: weight={w!r} does not fit float32")
    d = spec.decay
    if isinstance(d, bool) or not isinstance(d, (int, np.integer)) or d < 0:
        raise ValueError(f"anchor: decay={d!r} must be a whole number of learner calls >= 0")
    return spec


def parse_gain_grid(text):
    """``kp=lo:hi:n,kv=...`` (keys of GAIN_KEYS; ``key=value`` is the single value) -> float32 [G, 4]: per key np.linspace(lo, hi, n) in
    float64, then cast; a missing key is the single value 0; the product in kp, kv, ka, kf order, the last varying fastest. A
    ValueError for an unknown key, a key given twice, n < 1 or no integer, a non-finite bound, an empty grid text and G > MAX_GRID."""
    axes = {}
    parts = [q.strip() for q in str(text).split(",") if q.strip()]
    if not parts:
        raise ValueError(f"gain grid {text!r}: no axis given (kp=lo:hi:n,...)")
    for part in parts:
        key, eq, val = part.partition("=")
        key, val = key.strip(), val.strip()
        if not eq or key not in GAIN_KEYS:
            raise ValueError(f"gain grid: unknown key {key!r} (one of {', '.join(GAIN_KEYS)}, as key=lo:hi:n)")
        if key in axes:
            raise ValueError(f"gain grid: {key} given twice")
        f = [x.strip() for x in val.split(":")]
        try:
            if len(f) == 1:
                lo = hi = float(f[0])
                n = 1
            elif len(f) == 3:
                lo, hi, n = float(f[0]), float(f[1]), int(f[2])
            else:
                raise ValueError
        except ValueError:
            raise ValueError(f"gain grid: {key}={val!r} is not lo:hi:n (two numbers and an integer) or a single number") from None
        if n < 1:
            raise ValueError(f"gain grid: {key} has n={n} points (n must be >= 1)")
        if not (math.isfinite(lo) and math.isfinite(hi)):
            raise ValueError(f"gain grid: {key}={val!r} has a non-finite bound")
        axes[key] = (lo, hi, n)
    G = 1
    for _, _, n in axes.values():
        G *= n
    if G > MAX_GRID:
        raise ValueError(f"gain grid: {G} candidates (at most {MAX_GRID})")
    cols = [np.linspace(*axes[k]) if k in axes else np.zeros(1) for k in GAIN_KEYS]
    mesh = np.meshgrid(*cols, indexing="ij")
    return np.ascontiguousarray(np.stack([m.ravel() for m in mesh], axis=1).astype(np.float32))


def first_argmax(fitness):
    """The index of the largest value of a 1-d array: the first among equals; a NaN never wins (all NaN: index 0)."""
    f = np.asarray(fitness)
    best = 0
    for i in range(1, f.shape[0]):
        if not np.isnan(f[i]) and (np.isnan(f[best]) or f[i] > f[best]):
            best = i
    return best


def fitness_of(counters):
    """float32 [G] from counters [G, K, L]: per gain set the sequential float32 sum in (k, v) order divided by float32(K * L) -- the
    loop avd_linear_fitness_f32 runs on the device, bit for bit."""
    c = np.asarray(counters, dtype=np.float32)
    c = c.reshape(c.shape[0], -1)
    out = np.zeros(c.shape[0], dtype=np.float32)
    for g in range(c.shape[0]):
        s = np.float32(0.0)
        for x in c[g]:
            s = np.float32(s + x)
        out[g] = s / np.float32(c.shape[1])
    return out


# ---- gain search: a cross-entropy search over gain tables (evaluator.search_linear; avd_search_sample_f32, avd_search_refit_f32) -----

SEARCHED = "searched"  # the name --baseline_search gives the search's best law
MAX_POP, MAX_GENS = 65536, 10000
SEARCH_OVER = ("nominal", "all")
SEARCH_KEYS = GAIN_KEYS + ("pop", "gens", "elite", "alpha", "min_std", "seed", "per_vehicle", "over")


class SearchSpace:
    """What evaluator.search_linear searches: ``bounds`` {key of GAIN_KEYS: (lo, hi)} -- a missing key is frozen at 0, lo == hi frozen at
    that value -- and the search's knobs: ``pop`` candidates per generation, ``gens`` generations, ``elite`` the fraction refitted to
    (floor(elite * pop) candidates), ``alpha`` the refit's step, ``min_std`` the floor of a dimension's standard deviation as a fraction
    of hi - lo, ``seed`` (None: the Config's evaluation_seed), ``per_vehicle`` (one gain row per vehicle; False: one row for all),
    ``over`` ("nominal": the fitness is over the undisturbed cases; "all": over the disturbance levels too) and ``init``, an optional
    [L or 1][4] start mean (default: the midpoint of the bounds). The start std is (hi - lo) / 2."""

    def __init__(self, bounds, pop=1024, gens=30, elite=0.125, alpha=0.7, min_std=0.01, seed=None, per_vehicle=True, over="nominal",
                 init=None, text=None):
        self.bounds = {k: (v if isinstance(v, (tuple, list)) else (v, v)) for k, v in dict(bounds).items()}
        self.pop, self.gens, self.elite, self.alpha, self.min_std = pop, gens, elite, alpha, min_std
        self.seed, self.per_vehicle, self.over, self.text = seed, per_vehicle, over, text
        self.init = None if init is None else np.asarray(init)

    def n_elite(self):
        return int(math.floor(self.elite * self.pop))

    def rows(self, L):
        """R: the searched rows of a platoon of L."""
        return int(L) if self.per_vehicle else 1

    def tables(self, L):
        """float32 [R, 4] each: (lo, hi, mean, std, min_std) of a checked space, formed in float64 and rounded once."""
        R = self.rows(L)
        lo = np.array([self.bounds.get(k, (0.0, 0.0))[0] for k in GAIN_KEYS], dtype=np.float64)
        hi = np.array([self.bounds.get(k, (0.0, 0.0))[1] for k in GAIN_KEYS], dtype=np.float64)
        mean = np.tile((lo + hi) / 2, (R, 1))
        if self.init is not None:
            init = np.asarray(self.init, dtype=np.float64)
            mean = np.tile(init, (R, 1)) if init.shape[0] == 1 else init.copy()
            if mean.shape != (R, 4):
                raise ValueError(f"search: init of shape {init.shape} for {R} searched row(s) (need [{R}, 4] or [1, 4])")
        f = lambda x: np.ascontiguousarray(np.tile(x, (R, 1)).astype(np.float32))
        return f(lo), f(hi), np.ascontiguousarray(mean.astype(np.float32)), f((hi - lo) / 2), f(float(self.min_std) * (hi - lo))

    def with_init(self, init):
        """The same space starting from ``init`` ([L or 1][4])."""
        return SearchSpace(self.bounds, self.pop, self.gens, self.elite, self.alpha, self.min_std, self.seed, self.per_vehicle, self.over,
                           init, self.text)

    def __repr__(self):
        return (f"SearchSpace({self.bounds!r}, pop={self.pop!r}, gens={self.gens!r}, elite={self.elite!r}, alpha={self.alpha!r}, "
                f"min_std={self.min_std!r}, seed={self.seed!r}, per_vehicle={self.per_vehicle!r}, over={self.over!r})")


def parse_search(text):
    """``kp=0:3,kv=0:4,ka=-1:0,kf=0:1,pop=1024,gens=30,elite=0.125,alpha=0.7,min_std=0.01,seed=6,per_vehicle=1,over=nominal`` ->
    SearchSpace: a gain key takes ``lo:hi`` (or a single value: frozen there), the other keys of SEARCH_KEYS one value. An unknown key, a
    key given twice, a value that is no number or an empty text is a ValueError; the values are checked by check_search."""
    parts = [q.strip() for q in str(text).split(",") if q.strip()]
    if not parts:
        raise ValueError(f"search {text!r}: no bound given (kp=lo:hi,...[,pop=..,gens=..,elite=..])")
    bounds, kw = {}, {}
    for part in parts:
        key, eq, val = part.partition("=")
        key, val = key.strip(), val.strip()
        if not eq or key not in SEARCH_KEYS:
            raise ValueError(f"search: unknown key {key!r} (one of {', '.join(SEARCH_KEYS)}, as key=value)")
        if key in bounds or key in kw:
            raise ValueError(f"search: {key} given twice")
        try:
            if key in GAIN_KEYS:
                f = [float(x) for x in val.split(":")]
                if len(f) not in (1, 2):
                    raise ValueError
                bounds[key] = (f[0], f[-1])
            elif key in ("pop", "gens", "seed"):
                kw[key] = int(val)
            elif key == "per_vehicle":
                if val.lower() not in ("0", "1", "true", "false"):
                    raise ValueError
                kw[key] = val.lower() in ("1", "true")
            elif key == "over":
                kw[key] = val
            else:
                kw[key] = float(val)
        except ValueError:
            what = "lo:hi (two numbers) or a single number" if key in GAIN_KEYS else \
                "an integer" if key in ("pop", "gens", "seed") else "0 or 1" if key == "per_vehicle" else "a number"
            raise ValueError(f"search: {key}={val!r} is not {what}") from None
    return SearchSpace(bounds, text=str(text).strip(), **kw)


def check_search(space, conf=None):
    """The space, checked. A ValueError for: not a SearchSpace; an unknown gain key; a non-finite bound; lo > hi; pop outside [2,
    MAX_POP]; gens outside [1, MAX_GENS]; elite > 0.5 or floor(elite * pop) < 2; alpha outside (0, 1]; a negative min_std; an unknown
    ``over``; a negative seed; no searched dimension at all; an init that is not finite [*, 4] or lies outside the bounds; with ``conf``,
    a non-zero kf bound under Model A, the centralized framework and an init whose row count is neither 1 nor the searched rows."""
    if not isinstance(space, SearchSpace):
        raise ValueError(f"{space!r} is not a scenarios.SearchSpace")
    num = lambda v: not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))
    whole = lambda v: not isinstance(v, bool) and isinstance(v, (int, np.integer))
    bad = sorted(k for k in space.bounds if k not in GAIN_KEYS)
    if bad:
        raise ValueError(f"search: unknown gain key(s) {bad} (one of {', '.join(GAIN_KEYS)})")
    for k, (lo, hi) in space.bounds.items():
        if not (num(lo) and num(hi) and math.isfinite(lo) and math.isfinite(hi)):
            raise ValueError(f"search: {k}={lo!r}:{hi!r} has a non-finite bound")
        if lo > hi:
            raise ValueError(f"search: {k} has lo={lo!r} > hi={hi!r}")
    if not whole(space.pop) or not 2 <= space.pop <= MAX_POP:
        raise ValueError(f"search: pop={space.pop!r} must be an integer in [2, {MAX_POP}]")
    if not whole(space.gens) or not 1 <= space.gens <= MAX_GENS:
        raise ValueError(f"search: gens={space.gens!r} must be an integer in [1, {MAX_GENS}]")
    if not num(space.elite) or not space.elite <= 0.5 or space.n_elite() < 2:
        raise ValueError(f"search: elite={space.elite!r} with pop={space.pop} (need elite <= 0.5 and floor(elite * pop) >= 2)")
    if not num(space.alpha) or not 0 < space.alpha <= 1:
        raise ValueError(f"search: alpha={space.alpha!r} must be a number in (0, 1]")
    if not num(space.min_std) or not (space.min_std >= 0 and math.isfinite(space.min_std)):
        raise ValueError(f"search: min_std={space.min_std!r} must be a finite number >= 0")
    if space.over not in SEARCH_OVER:
        raise ValueError(f"search: over={space.over!r} (one of {', '.join(SEARCH_OVER)})")
    if space.seed is not None and (not whole(space.seed) or not 0 <= space.seed < 2 ** 64):
        raise ValueError(f"search: seed={space.seed!r} must be an integer in [0, 2^64)")
    if not any(lo < hi for lo, hi in space.bounds.values()):
        raise ValueError("search: no searched dimension (every gain is frozen: give at least one key lo:hi with lo < hi)")
    lo = np.array([space.bounds.get(k, (0.0, 0.0))[0] for k in GAIN_KEYS], dtype=np.float64)
    hi = np.array([space.bounds.get(k, (0.0, 0.0))[1] for k in GAIN_KEYS], dtype=np.float64)
    if space.init is not None:
        t = np.asarray(space.init)
        if t.ndim != 2 or t.shape[1] != 4 or t.shape[0] < 1 or not np.issubdtype(t.dtype, np.number) or not np.isfinite(t).all():
            raise ValueError(f"search: init must be a finite [L or 1, 4] array (got shape {t.shape})")
        t32 = t.astype(np.float32)  # (as the device sees them: a float32 grid value on a bound stays on it)
        if np.any(t32 < lo.astype(np.float32)) or np.any(t32 > hi.astype(np.float32)):
            raise ValueError(f"search: init {t.tolist()} lies outside the bounds lo={lo.tolist()} hi={hi.tolist()}")
    if conf is not None:
        if conf.framework == conf.cntrl:
            raise ValueError("a linear baseline is a per-vehicle law: not available for the centralized framework")
        if conf.model == conf.modelA and (lo[3] != 0 or hi[3] != 0):
            raise ValueError("a search over kf needs Model B (Model A observes no communicated state)")
        if space.init is not None and space.init.shape[0] not in (1, space.rows(conf.pl_size)):
            raise ValueError(f"search: init of {space.init.shape[0]} rows for {space.rows(conf.pl_size)} searched row(s) "
                             f"(pl_size={conf.pl_size}, per_vehicle={bool(space.per_vehicle)})")
    return space


# ---- training manoeuvres: what the fused step's leader follows during training (avd_step_fused_lead_f32) -----------------------------

MAX_MANOEUVRES = 16  # AVD_TRAIN_MAX_MANOEUVRES
MANOEUVRE_KEYS = ("profile", "amp", "period", "noise")
DEFAULT_PERIOD = 10.0


class Manoeuvre:
    """One training manoeuvre: the leader's input over a platoon's own episode is ``leader_profile(profile, steps_per_episode, conf, amp,
    period)`` -- the array the scenario evaluator feeds its cases -- plus ``noise`` times the step's unit draw (default 0: the profile
    alone). ``profile='gaussian'`` is the reference's training input, the unit draw times ``noise`` (default conf.reset_max_u): the clean
    share of a run; it takes neither amp nor period."""

    def __init__(self, name, profile="gaussian", amp=None, period=DEFAULT_PERIOD, noise=None):
        self.name, self.profile = str(name), profile
        self.amp, self.period, self.noise = amp, period, noise

    def items(self):
        """[(key, value)] in MANOEUVRE_KEYS order (conf.json's train_leader)."""
        return [[k, getattr(self, k)] for k in MANOEUVRE_KEYS]

    def __repr__(self):
        return "Manoeuvre(" + ", ".join([repr(self.name)] + [f"{k}={v!r}" for k, v in self.items()]) + ")"


def parse_manoeuvre(text):
    """``NAME[:key=val,...]`` (keys of MANOEUVRE_KEYS) -> Manoeuvre. Without a profile key a NAME that is itself a profile name means
    that profile, any other NAME the gaussian one. An unknown key, a key given twice, a value that is no number or amp / period beside
    the gaussian profile is a ValueError; the values are checked by check_manoeuvres."""
    name, _, spec = str(text).partition(":")
    name = name.strip()
    if not name:
        raise ValueError(f"manoeuvre {text!r}: no name before ':'")
    kw = {}
    for part in [q.strip() for q in spec.split(",") if q.strip()]:
        key, eq, val = part.partition("=")
        key, val = key.strip(), val.strip()
        if not eq or key not in MANOEUVRE_KEYS:
            raise ValueError(f"manoeuvre {name!r}: unknown key {key!r} (one of {', '.join(MANOEUVRE_KEYS)}, as key=value)")
        if key in kw:
            raise ValueError(f"manoeuvre {name!r}: {key} given twice")
        if key == "profile":
            kw[key] = val
            continue
        try:
            kw[key] = float(val)
        except ValueError:
            raise ValueError(f"manoeuvre {name!r}: {key}={val!r} is not a number") from None
    kw.setdefault("profile", name if name in SCENARIOS else "gaussian")
    if kw["profile"] == "gaussian" and ("amp" in kw or "period" in kw):
        raise ValueError(f"manoeuvre {name!r}: the gaussian profile takes neither amp nor period (its scale is noise)")
    return Manoeuvre(name, **kw)


def check_manoeuvres(manoeuvres):
    """The manoeuvres as a list. A ValueError for: none or more than MAX_MANOEUVRES; an unknown profile; a non-finite value; period <=
    0; noise < 0; amp or period beside the gaussian profile; a name listed twice."""
    out = list(manoeuvres)
    if not 1 <= len(out) <= MAX_MANOEUVRES:
        raise ValueError(f"{len(out)} manoeuvres listed: 1 to {MAX_MANOEUVRES} (platoon p trains under manoeuvre (p // n_levels) % n_manoeuvres)")
    for m in out:
        if not isinstance(m, Manoeuvre):
            raise ValueError(f"{m!r} is not a scenarios.Manoeuvre")
        if m.profile not in SCENARIOS:
            raise ValueError(f"manoeuvre {m.name!r}: unknown profile {m.profile!r}: one of {', '.join(SCENARIOS)}")
        for k in ("amp", "period", "noise"):
            v = getattr(m, k)
            if v is None and k != "period":
                continue
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
                raise ValueError(f"manoeuvre {m.name!r}: {k}={v!r} must be a finite number")
        if m.period <= 0:
            raise ValueError(f"manoeuvre {m.name!r}: period={m.period!r} must be > 0")
        if m.noise is not None and m.noise < 0:
            raise ValueError(f"manoeuvre {m.name!r}: noise={m.noise!r} must be >= 0")
        if m.profile == "gaussian" and (m.amp is not None or m.period != DEFAULT_PERIOD):
            raise ValueError(f"manoeuvre {m.name!r}: the gaussian profile takes neither amp nor period (its scale is noise)")
    names = [m.name for m in out]
    dup = sorted({n for n in names if names.count(n) > 1})
    if dup:
        raise ValueError(f"manoeuvre(s) {dup} listed more than once")
    return out


def manoeuvre_table(conf, manoeuvres):
    """Checked manoeuvres -> (float32 [n, T] leader inputs, float32 [n] noise scales, bool [n] gaussian flags) with T =
    conf.steps_per_episode: row m is leader_profile(profile, T, conf, amp, period) -- float64, rounded once; the array evaluator.CaseBatch
    feeds avd_eval_cases_f32 -- and noise 0 by default; a gaussian manoeuvre's row is unread (zeros), its noise conf.reset_max_u by
    default."""
    ms = check_manoeuvres(manoeuvres)
    T = int(conf.steps_per_episode)
    check_knobs(T, None, DEFAULT_PERIOD)
    table = np.zeros((len(ms), T), dtype=np.float32)
    noise = np.zeros(len(ms), dtype=np.float32)
    gauss = np.zeros(len(ms), dtype=bool)
    for k, m in enumerate(ms):
        gauss[k] = m.profile == "gaussian"
        if gauss[k]:
            noise[k] = np.float32(conf.reset_max_u if m.noise is None else m.noise)
        else:
            table[k] = leader_profile(m.profile, T, conf, m.amp, m.period)
            noise[k] = np.float32(0.0 if m.noise is None else m.noise)
    return table, noise, gauss


def manoeuvre_of(q, n_manoeuvres, n_levels=1):
    """The manoeuvre index of the platoon whose solo-run index is q: levels (q % n_levels) and manoeuvres cross."""
    return (int(q) // int(n_levels)) % int(n_manoeuvres)


ROBUSTNESS_HEADER = [*CSV_HEADER[:2], "disturbance", *CSV_HEADER[2:], "score_delta"]


def robustness_rows(results, platoon_tags):
    """csv_rows for a DisturbedResults ([P, scen, dist, seed, ...] arrays): one row per (platoon, scenario, disturbance, seed, vehicle),
    the nominal level first, with the columns of scenarios.csv, the level's name after the scenario's and, last, score_delta = the
    case's score minus the nominal score of the same platoon, scenario and seed (float32)."""
    s = results.summary()
    f = lambda x: "" if np.isnan(x) else repr(float(x))
    rows = []
    for i, tag in enumerate(platoon_tags):
        for c, name in enumerate(results.scenarios):
            for d, level in enumerate(results.disturbances):
                for k, seed in enumerate(results.seeds):
                    for v in range(results.metrics[METRICS[0]].shape[-1]):
                        at = (i, c, d, k, v)
                        rows.append([tag, name, level, seed, v + 1, *[f(results.metrics[m][at]) for m in METRICS], f(s["rms_u"][at]),
                                     f(s["rms_jerk"][at]), f(s["ss_ratio"][at]), f(results.scores[i, c, d, k]),
                                     f(results.scores[i, c, d, k] - results.scores[i, c, 0, k])])
    return rows


def write_robustness_csv(path, results, platoon_tags):
    import csv

    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(ROBUSTNESS_HEADER)
        w.writerows(robustness_rows(results, platoon_tags))


BASELINE_HEADER = ["controller", *CSV_HEADER[1:], "actors_score"]
BASELINE_ROBUSTNESS_HEADER = ["controller", *ROBUSTNESS_HEADER[1:], "actors_score"]


def actors_mean_score(actors):
    """float32 [scen, (dist,) seed]: the mean over the platoon axis of the actors' scores (a CaseResults or DisturbedResults)."""
    return np.mean(np.asarray(actors.scores, dtype=np.float32), axis=0, dtype=np.float32)


def baseline_rows(results, laws, actors):
    """csv_rows / robustness_rows for a run_linear result (first axis: the laws) with the law's name in the first column and, last,
    actors_score: the mean over the run's platoons of the actors' score for the same (scenario, disturbance, seed)."""
    f = lambda x: "" if np.isnan(x) else repr(float(x))
    mean = actors_mean_score(actors)
    disturbed = hasattr(results, "disturbances")
    rows = robustness_rows(results, laws) if disturbed else csv_rows(results, laws)
    nv = results.metrics[METRICS[0]].shape[-1]
    per_law = len(rows) // max(1, len(laws))
    flat = np.repeat(mean.reshape(-1), nv)  # (scenario, (disturbance,) seed, vehicle) order, as the rows of one law
    return [r + [f(flat[i % per_law])] for i, r in enumerate(rows)]


def write_baseline_csv(path, results, laws, actors):
    import csv

    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(BASELINE_ROBUSTNESS_HEADER if hasattr(results, "disturbances") else BASELINE_HEADER)
        w.writerows(baseline_rows(results, laws, actors))


def baseline_report_lines(results, laws):
    """One line per law and scenario, as report_lines words a platoon's (nominal level of a disturbed result)."""
    nominal = results.nominal() if hasattr(results, "disturbances") else results
    return [ln.replace("platoon ", "baseline ", 1) for ln in report_lines(nominal, laws)]


def report_lines(results, platoon_tags):
    """One line per platoon and scenario: the mean score over the seeds, the worst max_abs_ep over seeds and vehicles, and whether
    every seed's rollout was string stable."""
    s = results.summary()
    out = []
    for i, tag in enumerate(platoon_tags):
        for c, name in enumerate(results.scenarios):
            out.append(f"platoon {tag} {name}: score {float(np.mean(results.scores[i, c])):.3f} worst max_abs_ep "
                       f"{float(np.max(results.metrics['max_abs_ep'][i, c])):.5f} string_stable {bool(np.all(s['string_stable'][i, c]))}")
    return out
