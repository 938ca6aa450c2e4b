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
