"""`python -m avddpg_amd {tr,esim}` -- the two modes of the reference CLI that touch the hot path, with the
reference's flag names and override quirks (``src/cmd/api.py:5-50, 59-88``): ``--fed_weight_enabled`` defaults to
False and always overrides the Config default (True); ``--intra_directional_averaging`` defaults to True; the
``type=bool`` flags treat any non-empty string as True. Reporting modes (accumr/accums/lsim/lmany/pid) are out of scope."""
import argparse
import datetime
import os
import sys

from .config import Config


def parse_seeds(text):
    """``--seeds`` value -> list of seeds: comma-separated non-negative integers and inclusive ranges ``a-b`` (``1,2,5-8`` ->
    [1, 2, 5, 6, 7, 8]), in the order given; an empty item, a reversed range or a seed listed twice is a ValueError."""
    out = []
    for item in str(text).split(","):
        item = item.strip()
        lo, sep, hi = item.partition("-")
        if not lo.isdigit() or (sep and not hi.isdigit()):
            raise ValueError(f"--seeds: {item!r} is neither a seed nor a range a-b of non-negative integers")
        a, b = int(lo), int(hi) if sep else int(lo)
        if b < a:
            raise ValueError(f"--seeds: the range {item!r} runs backwards")
        out.extend(range(a, b + 1))
    dup = sorted({k for k in out if out.count(k) > 1})
    if dup:
        raise ValueError(f"--seeds: seed(s) {dup} listed more than once")
    if any(k >= 2 ** 32 for k in out):
        raise ValueError("--seeds: seeds must be below 2**32 (the global np.random seed and the initial weights' RandomState take them)")
    return out


SWEEP_NAMES = ("actor_lr", "critic_lr", "tau", "gamma", "std_dev", "theta")  # (vec.HP_KEYS)


def parse_sweep(items):
    """``--sweep NAME=V1,V2,...`` values (in flag order) -> [(name, [values])]; an unknown or repeated name, an empty list, a value
    listed twice or one that is not a number is a ValueError."""
    out, seen = [], set()
    for item in items:
        name, sep, vals = str(item).partition("=")
        name = name.strip()
        if not sep or name not in SWEEP_NAMES:
            raise ValueError(f"--sweep: {item!r} is not NAME=V1,V2,... with NAME one of {', '.join(SWEEP_NAMES)}")
        if name in seen:
            raise ValueError(f"--sweep: {name} is swept twice")
        seen.add(name)
        parts = [v.strip() for v in vals.split(",")]
        if not vals.strip() or any(not v for v in parts):
            raise ValueError(f"--sweep {name}: empty value list or item")
        try:
            nums = [float(v) for v in parts]
        except ValueError:
            raise ValueError(f"--sweep {name}: {vals!r} holds a value that is not a number") from None
        if len(set(nums)) != len(nums):
            raise ValueError(f"--sweep {name}: a value is listed twice in {vals!r}")
        out.append((name, nums))
    return out


def sweep_experiments(sweep, seeds):
    """The experiments of a sweep: the product of its value lists in flag order (the last flag varying fastest), times the seeds
    (innermost) -> [(label, {name: value}, seed)]. The label names every swept value: ``actor_lr=0.0001_gamma=0.95``."""
    import itertools

    names = [n for n, _ in sweep]
    out = []
    for combo in itertools.product(*[v for _, v in sweep]):
        h = dict(zip(names, combo))
        label = "_".join(f"{n}={v!r}" for n, v in h.items())
        out.extend((label, h, int(k)) for k in seeds)
    return out


def _scenario_flags(p, where):
    p.add_argument("--scenarios", type=str, default=None, metavar="LIST",
                   help=f"{where} evaluate every platoon's actors over these leader scenarios (comma-separated, of zero, step, ramp, brake, "
                        "sine, gaussian) x --eval_seeds in ONE launch of the scenario evaluator and write scenarios.csv: one row per "
                        "(platoon, scenario, seed, vehicle) with the control metrics (peak errors, control effort, jerk, terminal steps, "
                        "string-stability ratio) and the case's score (not in the reference CLI)")
    p.add_argument("--eval_seeds", type=str, default=None, metavar="LIST",
                   help="--scenarios: the evaluation seeds (e.g. 6,7-9; default: the configuration's evaluation_seed); a seed fixes the "
                        "start state and the gaussian scenario's leader inputs")
    p.add_argument("--scenario_amp", type=float, default=None,
                   help="--scenarios: the amplitude of step, ramp, brake and sine (default: reset_max_u, the scale of leader input the "
                        "actors are trained on)")
    p.add_argument("--scenario_period", type=float, default=None, help="--scenarios: the sine's period in seconds (default 10)")
    # (absent from the namespace unless given: _disturb(args) reads it)
    p.add_argument("--disturb", action="append", default=argparse.SUPPRESS, metavar="NAME:key=val,...",
                   help="--scenarios: also run every scenario x seed under this disturbance (repeat the flag for more levels), all in the "
                        "same ONE launch, and write robustness.csv: scenarios.csv's columns plus `disturbance` and `score_delta` (score "
                        "minus the undisturbed score of the same platoon, scenario and seed). Keys: noise_ep, noise_ev, noise_a (sensor "
                        "noise, standard deviations), v2v_delay (steps, 0..15) and v2v_drop (loss probability) on the communicated "
                        "predecessor acceleration (Model B), dyn_coeff (the true plant's engine lag; the actors stay as trained), e.g. "
                        "lag3:v2v_delay=3,v2v_drop=0.1 (not in the reference CLI)")
    # (both absent from the namespace unless given: _baseline_flags(args) reads them)
    p.add_argument("--baseline", action="append", default=argparse.SUPPRESS, metavar="NAME[:key=val,...]",
                   help="--scenarios: also run this linear law u = clip(kp ep + kv ev + ka a + kf a_pred) in place of the actors over the "
                        "same scenarios x seeds x --disturb levels (repeat the flag for more laws, at most 16; ONE launch of the linear "
                        "scenario evaluator for all of them) and write baseline.csv: scenarios.csv's columns (robustness.csv's with "
                        "--disturb) with `controller` in place of `platoon` and a trailing `actors_score`, the mean over the run's "
                        "platoons of the actors' score for the same scenario, disturbance and seed. Keys: kp, kv, ka, kf (kf: Model B), "
                        "e.g. cacc:kp=0.5,kv=1. Decentralized platoons only (not in the reference CLI)")
    p.add_argument("--baseline_tune", type=str, default=argparse.SUPPRESS, metavar="GRID",
                   help="--scenarios: add the law `tuned`: the best of a gain grid by mean counter over the suite's undisturbed cases, "
                        "searched on the device (one rollout launch over grid x cases, one fitness launch), then evaluated like any "
                        "--baseline law. GRID: key=lo:hi:n per gain (np.linspace; a missing key is 0), at most 65536 candidates, e.g. "
                        "kp=0:2:9,kv=0:4:9,ka=-0.5:0:3 (not in the reference CLI)")
    p.add_argument("--baseline_search", type=str, default=argparse.SUPPRESS, metavar="SPEC",
                   help="--scenarios: add the law `searched`: the best gain table of a cross-entropy search that stays on the device (per "
                        "generation: sample, roll out, fitness, refit; nothing is read back until the last), one gain row per vehicle "
                        "(per_vehicle=0: one row for all), then evaluated like any --baseline law. SPEC: key=lo:hi per gain (a missing key "
                        "is frozen at 0, a single value frozen there) and pop (2..65536), gens, elite (a fraction <= 0.5), alpha, min_std, "
                        "seed, per_vehicle, over (nominal: the fitness is over the undisturbed cases; all: over the --disturb levels "
                        "too), e.g. kp=0:3,kv=0:4,ka=-1:0,kf=0:1,pop=1024,gens=30. With --baseline_tune the search starts from the "
                        "grid's pick (not in the reference CLI)")
    p.add_argument("--freq_response", type=str, default=argparse.SUPPRESS, metavar="SPEC",
                   help="the frequency response of every platoon's actors: sinusoidal leader inputs at n log-spaced frequencies (Hz, snapped "
                        "to whole cycles in the measuring window) x --eval_seeds x every --disturb level in ONE launch, the single-bin "
                        "Fourier sums reduced on the device, and the same for every --baseline / tuned / searched law; writes "
                        "frequency.csv -- one row per (controller, disturbance, seed, frequency, vehicle) with the amplitudes and phases of "
                        "ep, ev, a, w, u, the vehicle-to-vehicle gains gain_a and gain_ep, and for laws the float64 theory's gain_a -- and "
                        "conf.json's frequency_suite with the peak gain per controller and level (string stable: every peak <= 1). "
                        "Independent of --scenarios (--eval_seeds, --disturb and --baseline are then accepted without it). SPEC: "
                        "fmin=0.02,fmax=2,n=16[,amp=A,settle=0.5,steps=N] (not in the reference CLI)")


def _check_scenario_flags(ap, args):
    """The scenario flags of a parsed namespace, validated in place (scenarios -> list of names, eval_seeds -> list of seeds or None)."""
    import math

    from .scenarios import check_names

    if _freq(args) is not None:
        from .scenarios import parse_frequency

        try:  # (the window's length needs the run's configuration unless steps is given: _check_freq_conf)
            args.freq_response = parse_frequency(args.freq_response)
        except ValueError as e:
            ap.error(f"--freq_response: {e}")
    if args.scenarios is None:
        shared = ("eval_seeds", "disturb", "baseline") if _freq(args) is not None else ()  # what --freq_response uses too
        for flag in ("eval_seeds", "scenario_amp", "scenario_period", "disturb", "baseline", "baseline_tune", "baseline_search"):
            if getattr(args, flag, None) is not None and flag not in shared:
                ap.error(f"--{flag} needs --scenarios")
        if _freq(args) is None:
            return
    else:
        try:
            args.scenarios = check_names([n.strip() for n in args.scenarios.split(",")])
        except ValueError as e:
            ap.error(f"--scenarios: {e}")
    if args.eval_seeds is not None:
        try:
            args.eval_seeds = parse_seeds(args.eval_seeds)
        except ValueError as e:
            ap.error(str(e).replace("--seeds", "--eval_seeds"))
    if args.scenario_amp is not None and not math.isfinite(args.scenario_amp):
        ap.error("--scenario_amp must be finite")
    if args.scenario_period is not None and not (math.isfinite(args.scenario_period) and args.scenario_period > 0):
        ap.error("--scenario_period must be finite and > 0")
    if _disturb(args) is not None:
        from .scenarios import check_disturbances, parse_disturbance

        try:  # (the Model A refusal needs the run's configuration: evaluator.prepare_disturbed makes it)
            args.disturb = check_disturbances([parse_disturbance(d) for d in args.disturb])
        except ValueError as e:
            ap.error(f"--disturb: {e}")
    if any(getattr(args, f, None) is not None for f in ("baseline", "baseline_tune", "baseline_search")):
        from . import scenarios as _sc

        search = getattr(args, "baseline_search", None)
        try:  # (what needs the run's configuration -- Model A, the centralized framework -- is checked once it is known)
            args.baseline = _sc.check_baselines([_sc.parse_baseline(b) for b in getattr(args, "baseline", None) or []],
                                                reserved=(_sc.TUNED,) if search is None else (_sc.TUNED, _sc.SEARCHED))
        except ValueError as e:
            ap.error(f"--baseline: {e}")
        if search is not None:
            extra = 1 + (getattr(args, "baseline_tune", None) is not None)
            if len(args.baseline) + extra > _sc.MAX_BASELINES:
                also = " and --baseline_tune's `tuned`" if extra == 2 else ""
                ap.error(f"--baseline: {len(args.baseline)} laws beside --baseline_search's `searched`{also}: at most {_sc.MAX_BASELINES} in all")
            try:
                args.baseline_search = _sc.check_search(_sc.parse_search(search))
            except ValueError as e:
                ap.error(f"--baseline_search: {e}")
        if getattr(args, "baseline_tune", None) is not None:
            if len(args.baseline) + 1 > _sc.MAX_BASELINES:
                ap.error(f"--baseline: {len(args.baseline)} laws beside --baseline_tune's `tuned`: at most {_sc.MAX_BASELINES} in all")
            try:
                args.baseline_tune = (args.baseline_tune, _sc.parse_gain_grid(args.baseline_tune))
            except ValueError as e:
                ap.error(f"--baseline_tune: {e}")
    if args.mode == "tr" and int(os.environ.get("WORLD_SIZE", "1") or 1) > 1:
        # (one of the two choices: refused, rather than every rank writing a scenarios.csv of its own platoons)
        if args.scenarios is None:
            ap.error("--freq_response is not available under a process group of more than one rank (frequency.csv is not gathered across ranks)")
        ap.error("--scenarios is not available under a process group of more than one rank (scenarios.csv is not gathered across ranks)")


def _disturb(args):
    """The --disturb levels (checked Disturbances), or None without the flag."""
    return getattr(args, "disturb", None)


def _freq(args):
    """--freq_response's FrequencySpec (its text before _check_scenario_flags), or None without the flag."""
    return getattr(args, "freq_response", None)


def _exit(msg):
    raise SystemExit(msg)


def _baseline_flags(args):
    """(the --baseline laws, --baseline_tune's (text, grid) or None), or None without any of --baseline, --baseline_tune and
    --baseline_search (whose SearchSpace _search_flag returns)."""
    laws, tune = getattr(args, "baseline", None), getattr(args, "baseline_tune", None)
    return None if laws is None and tune is None and _search_flag(args) is None else (list(laws or []), tune)


def _search_flag(args):
    """--baseline_search's checked SearchSpace, or None without the flag."""
    return getattr(args, "baseline_search", None)


def _check_baseline_conf(args, conf, refuse):
    """The --baseline / --baseline_tune refusals that need the run's configuration (Model A with kf, the centralized framework)."""
    flags = _baseline_flags(args)
    if flags is None:
        return
    from . import scenarios as _sc

    laws, tune = flags
    try:
        _sc.check_baselines(laws, conf)
        if tune is not None and conf.model == conf.modelA and (tune[1][:, 3] != 0).any():
            raise ValueError("a grid over kf needs Model B (Model A observes no communicated state)")
    except ValueError as e:
        refuse(f"--baseline: {e}")
    if _search_flag(args) is not None:
        try:
            _sc.check_search(_search_flag(args), conf)
        except ValueError as e:
            refuse(f"--baseline_search: {e}")


def _check_freq_conf(args, conf, refuse):
    """The --freq_response refusals that need the run's configuration: the window's length, a V2V level under Model A."""
    if _freq(args) is None:
        return
    from . import scenarios as _sc

    try:
        _sc.check_frequency(_freq(args), conf)
        _sc.check_disturbances(_disturb(args) or [], conf)
    except ValueError as e:
        refuse(f"--freq_response: {e}")


class _Frequency:
    """What --freq_response computes beside the actors' response, once per run: the laws' (--baseline, and with --scenarios the `tuned`
    and `searched` laws) in one launch of the linear frequency evaluator, with the float64 theory of each law and level.
    ``write(d, conf, actors, tags)`` puts frequency.csv into a directory and frequency_suite into its Config."""

    def __init__(self, conf, args, baselines=None):
        import numpy as np

        from . import evaluator
        from . import scenarios as _sc

        self.spec, self.levels, self.seeds = _freq(args), _disturb(args) or [], args.eval_seeds
        laws = baselines.laws if baselines is not None else (_baseline_flags(args) or ([], None))[0]
        self.laws = None
        if laws:
            try:
                res = evaluator.run_linear_frequency(conf, laws, self.spec, self.levels, self.seeds)
            except ValueError as e:
                raise SystemExit(f"--freq_response: {e}")
            theory = np.stack([np.stack([_sc.linear_frequency_response(conf, b.gains(conf.pl_size), res.cycles, res.W, lv.dyn_coeff)["gain_a"]
                                         for lv in [_sc.NOMINAL] + list(self.levels)]) for b in laws])  # [G, ND, F, L]
            self.laws = (res, [b.name for b in laws], theory)

    def actors(self, vt, agents=None):
        """The trainer's actors over the same sweep, one launch ([P, ...]; a seed batch or sweep: [E, P, ...])."""
        try:
            return vt.evaluate_frequency(self.spec, self.levels, self.seeds, agents=agents)
        except ValueError as e:
            raise SystemExit(f"--freq_response: {e}")

    def entries(self, actors, tags):
        return [(actors, [str(t) for t in tags], None)] + ([self.laws] if self.laws is not None else [])

    def record(self, actors, tags):
        """conf.json's frequency_suite, a list of pairs (conf.json keeps lists, not dicts)."""
        from . import scenarios as _sc

        peaks = [row for res, names, _ in self.entries(actors, tags) for row in _sc.frequency_peaks(res, names)]
        return [["spec", self.spec.items()], ["freqs_hz", [float(f) for f in actors.freqs_hz]], ["cycles", [int(c) for c in actors.cycles]],
                ["window", int(actors.W)], ["seeds", [int(k) for k in actors.seeds]], ["disturbances", list(actors.disturbances)],
                ["peaks", [["controller", "disturbance", "peak_gain_a", "freq_hz", "vehicle", "string_stable"]] + peaks]]

    def write(self, d, conf, actors, tags):
        from . import scenarios as _sc

        _sc.write_frequency_csv(os.path.join(d, "frequency.csv"), self.entries(actors, tags))
        conf.frequency_suite = self.record(actors, tags)

    def report(self, actors, tags):
        from . import scenarios as _sc

        lines = _sc.frequency_report_lines(actors, [str(t) for t in tags])
        return lines if self.laws is None else lines + _sc.frequency_report_lines(self.laws[0], self.laws[1], "baseline")


def _frequency(conf, args):
    """The run's frequency section (None without the flag), computed once; the laws are the baseline section's when --scenarios made one."""
    if _freq(args) is None:
        return None
    if getattr(args, "frequency", None) is None:
        args.frequency = _Frequency(conf, args, _baselines(conf, args) if args.scenarios is not None and _baseline_flags(args) is not None else None)
    return args.frequency


def _freq_slice(res, e):
    """Experiment e's FrequencyResults of a batch's ([E, P, ...] arrays)."""
    from .evaluator import FrequencyResults

    return FrequencyResults(res.freqs_hz, res.cycles, res.W, res.T, res.disturbances, res.seeds, res.spectrum[e], res.scores[e],
                            res.counters[e], {k: v[e] for k, v in res.metrics.items()})


class _Baselines:
    """What --baseline / --baseline_tune compute, once per run: the laws (the grid's best appended as `tuned`) over the suite's cases in
    one linear-evaluator launch. ``write(d, conf, actors)`` puts baseline.csv into a directory and the record into its Config."""

    def __init__(self, conf, args):
        from . import evaluator
        from . import scenarios as _sc

        import numpy as np

        laws, tune = _baseline_flags(args)
        self.tune = self.search = self.found = None
        try:
            if tune is not None:  # the search runs over the nominal cases only
                text, grid = tune
                best, fit = evaluator.tune_linear(conf, grid, **_suite(args))
                gains = [float(x) for x in grid[best]]
                laws = laws + [_sc.LinearLaw(_sc.TUNED, *gains)]
                self.tune = [["grid", text], ["candidates", int(grid.shape[0])], ["best_index", int(best)],
                             ["gains", [[k, v] for k, v in zip(_sc.GAIN_KEYS, gains)]], ["fitness", float(fit[best])]]
            space = _search_flag(args)
            if space is not None:  # from the grid's pick when there is one: candidate 0 of generation 0 is then that law
                if tune is not None:
                    space = _sc.check_search(space.with_init(np.asarray(grid[best], dtype=np.float32)[None, :]), conf)
                self.found = evaluator.search_linear(conf, space, disturbances=_disturb(args) or (), **_suite(args))
                laws = laws + [self.found.law]
                self.search = self.found.record(space.text)
            self.laws = laws
            self.results = evaluator.run_linear(conf, laws, disturbances=_disturb(args) or (), **_suite(args))
        except ValueError as e:
            raise SystemExit(f"--baseline: {e}")
        self.names = [b.name for b in laws]

    def write(self, d, conf, actors):
        from . import scenarios as _sc

        _sc.write_baseline_csv(os.path.join(d, "baseline.csv"), self.results, self.names, actors)
        conf.baseline_suite = [[b.name, b.items()] for b in self.laws]
        if self.tune is not None:
            conf.baseline_tune = self.tune
        if self.search is not None:
            conf.baseline_search = self.search

    def report(self):
        from . import scenarios as _sc

        lines = _sc.baseline_report_lines(self.results, self.names)
        if self.found is not None:
            f = self.found
            lines.append(f"baseline {_sc.SEARCHED} search: fitness {f.fitness:.6f} at generation {f.generation} of {f.gens} "
                         f"(pop {f.pop}, {f.n_elite} elites, {f.K} cases, {f.best_gains.shape[0]} searched row(s))")
        return lines


def _record_train_levels(conf, args):
    """conf.json's train_disturbances: the --train_disturb levels in the shape of robustness_suite ([name, [[key, value], ...]] pairs)."""
    if getattr(args, "train_disturb", None) is not None:
        conf.train_disturbances = [[x.name, x.items()] for x in args.train_disturb]


def _record_train_leader(conf, args):
    """conf.json's train_leader: the --train_leader manoeuvres as [name, [[key, value], ...]] pairs."""
    if getattr(args, "train_leader", None) is not None:
        conf.train_leader = [[x.name, x.items()] for x in args.train_leader]


def _lead_kw(args):
    """VecTrainer's train_leader keyword, only where the flag was given."""
    return {} if getattr(args, "train_leader", None) is None else dict(train_leader=args.train_leader)


def _check_train_leader(args, conf, auto_reset, hparams=None):
    """The --train_leader refusals that need the run's configuration, under the flag's own name, before anything is allocated."""
    if getattr(args, "train_leader", None) is not None:
        from . import trainer

        try:
            trainer.check_train_leader(conf, args.train_leader, args.rng, None, auto_reset, hparams=hparams)
        except ValueError as e:
            raise SystemExit(f"--train_leader: {e}")


def _residual_kw(args):
    """VecTrainer's residual keyword, only where the flag was given (a `tuned` law has been searched by then: _resolve_residual)."""
    return {} if getattr(args, "residual", None) is None else dict(residual=args.residual)


def _resolve_residual(args, conf, auto_reset, hparams=None):
    """--residual before anything is allocated: the word `tuned` becomes the law --baseline_tune's grid picks on the suite's nominal cases
    (evaluator.tune_linear, run once: the baseline section reuses the result), then the refusals that need the run's configuration,
    under the flag's own name."""
    law = getattr(args, "residual", None)
    if law is None:
        return
    from . import scenarios as _sc
    from . import trainer

    try:
        if law == _sc.TUNED:
            args.baselines = _Baselines(conf, args)
            args.residual = law = _sc.ResidualLaw(*[v for _, v in dict(args.baselines.tune)["gains"]], source="tuned")
        elif law == _sc.SEARCHED:
            args.baselines = _Baselines(conf, args)
            args.residual = law = _sc.ResidualLaw(table=args.baselines.found.law.table, source="searched")
        trainer.check_residual(conf, law, args.rng, int(os.environ.get("WORLD_SIZE", "1") or 1), hparams=hparams)
    except ValueError as e:
        raise SystemExit(f"--residual: {e}")


def _record_residual(conf, args):
    """conf.json's residual_law: the law the saved actors correct (esim applies it: the actors alone are not the policy)."""
    if getattr(args, "residual", None) is not None:
        conf.residual_law = args.residual.record()


def _warm_kw(args):
    """VecTrainer's warm_start / actor_hold keywords, only where a flag was given (`tuned` / `searched` resolved: _resolve_warm_start)."""
    kw = {} if getattr(args, "warm_start", None) is None else dict(warm_start=args.warm_start)
    return kw if getattr(args, "actor_hold", None) is None else dict(kw, actor_hold=args.actor_hold)


def _resolve_warm_start(args, conf, hparams=None):
    """--warm_start / --actor_hold before anything is allocated: the words `tuned` / `searched` become the law --baseline_tune /
    --baseline_search find (computed once: the baseline section reuses it), then the refusals that need the run's configuration, under
    the flag's own name."""
    from . import scenarios as _sc
    from . import trainer

    hold = getattr(args, "actor_hold", None)
    if hold is not None:
        if hold >= conf.total_time_steps:
            raise SystemExit(f"--actor_hold: N={hold} must be below the run's {conf.total_time_steps} steps")
        try:
            trainer.check_actor_hold(hold, hparams)
        except ValueError as e:
            raise SystemExit(f"--actor_hold: {e}")
    spec = getattr(args, "warm_start", None)
    if spec is None:
        return
    try:
        if spec in (_sc.TUNED, _sc.SEARCHED):
            args.baselines = _baselines(conf, args)
            fit = _sc.WarmStart()  # (the flag's other keys do not exist beside the word: the default fit)
            if spec == _sc.TUNED:
                law = _sc.LinearLaw(_sc.TUNED, *[v for _, v in dict(args.baselines.tune)["gains"]])
            else:
                law = _sc.LinearLaw(_sc.SEARCHED, table=args.baselines.found.law.table)
            args.warm_start = spec = fit.with_gains(law, source=spec)
        trainer.check_warm_start(conf, spec, args.rng, int(os.environ.get("WORLD_SIZE", "1") or 1), hparams=hparams,
                                 residual=getattr(args, "residual", None))
    except ValueError as e:
        raise SystemExit(f"--warm_start: {e}")


def _warm_fit(vt, args):
    """--warm_start: the fit, before the step-0 evaluations (--keep_best's first snapshot is the fitted actors), then the fitted actors'
    evaluator score from one rollout launch. Leaves (mean final fit loss, score) per experiment in args.warm_result. Without the
    flag: nothing."""
    if getattr(args, "warm_start", None) is None:
        return
    import numpy as np

    loss = np.asarray(vt.fit_warm_start(), dtype=np.float64).reshape(vt.E, vt.M).mean(axis=1)
    sc = np.asarray(vt.evaluator_scores([0]), dtype=np.float64).reshape(vt.E, -1)[:, 0]
    args.warm_result = [(float(loss[e]), float(sc[e])) for e in range(vt.E)]


def _record_warm(conf, args, e=0):
    """conf.json's warm_start (a list of pairs: the law's record, the mean final fit loss, the fitted actors' evaluator score) and
    actor_hold, only where the flags were given."""
    if getattr(args, "warm_start", None) is not None:
        loss, score = args.warm_result[e]
        conf.warm_start = [["law", args.warm_start.record()], ["fit_loss", loss], ["evaluator_score", score]]
    if getattr(args, "actor_hold", None) is not None:
        conf.actor_hold = int(args.actor_hold)


def _anchor_kw(args):
    """VecTrainer's anchor keyword, only where the flag was given (`tuned` / `searched` resolved: _resolve_anchor)."""
    return {} if getattr(args, "anchor", None) is None else dict(anchor=args.anchor)


def _resolve_anchor(args, conf, hparams=None):
    """--anchor before anything is allocated: the words `tuned` / `searched` become the law --baseline_tune / --baseline_search find
    (computed once: the baseline section reuses it) around the flag's weight and decay, then the refusals that need the run's
    configuration, under the flag's own name."""
    from . import scenarios as _sc
    from . import trainer

    spec = getattr(args, "anchor", None)
    if spec is None:
        return
    try:
        if spec.pending:
            args.baselines = _baselines(conf, args)
            if spec.source == _sc.TUNED:
                law = _sc.LinearLaw(_sc.TUNED, *[v for _, v in dict(args.baselines.tune)["gains"]])
            else:
                law = _sc.LinearLaw(_sc.SEARCHED, table=args.baselines.found.law.table)
            args.anchor = spec = spec.with_gains(law, source=spec.source)
        trainer.check_anchor(conf, spec, args.engine, int(os.environ.get("WORLD_SIZE", "1") or 1), hparams=hparams)
    except ValueError as e:
        raise SystemExit(f"--anchor: {e}")


def _record_anchor(conf, args, vt, e=0):
    """conf.json's anchor (a list of pairs: the law's record, the anchor loss per weight set of experiment e at the first learner call
    and at the last), only where the flag was given. The two device tensors are read here, after training."""
    if getattr(args, "anchor", None) is None:
        return
    if getattr(args, "anchor_result", None) is None:
        first = vt.anchor_loss_first if vt.anchor_loss_first is not None else vt.anchor_losses()
        args.anchor_result = (first.cpu().tolist(), vt.anchor_losses().cpu().tolist())
    first, last = ([float(x) for x in v[e * vt.M:(e + 1) * vt.M]] for v in args.anchor_result)
    conf.anchor = [["law", args.anchor.record()], ["anchor_loss_first", first], ["anchor_loss_last", last]]


def _noise_kw(args):
    """VecTrainer's target_noise keyword, only where the flag was given."""
    return {} if getattr(args, "target_noise", None) is None else dict(target_noise=args.target_noise)


def _record_noise(conf, args):
    """conf.json's target_noise (a list of pairs: sigma, clip), only where the flag was given."""
    if getattr(args, "target_noise", None) is not None:
        conf.target_noise = args.target_noise.record()


def _delay_kw(args):
    """VecTrainer's policy_delay keyword, only where the flag was given."""
    return {} if getattr(args, "policy_delay", None) is None else dict(policy_delay=args.policy_delay)


def _record_delay(conf, args):
    """conf.json's policy_delay (the delay, an int), only where the flag was given."""
    if getattr(args, "policy_delay", None) is not None:
        conf.policy_delay = int(args.policy_delay)


def _baselines(conf, args):
    """The run's baseline section, computed once (--residual tuned has already searched the grid)."""
    if getattr(args, "baselines", None) is None:
        args.baselines = _Baselines(conf, args)
    return args.baselines


def _saved_residual(exp_path):
    """The residual law an experiment directory's conf.json records, or None."""
    import json

    from . import scenarios as _sc

    with open(os.path.join(exp_path, "conf.json")) as f:
        return _sc.ResidualLaw.from_record(json.load(f).get("residual_law"))


def _suite(args):
    """run_cases' keyword arguments from the scenario flags."""
    return dict(scenarios=args.scenarios, seeds=args.eval_seeds, amp=args.scenario_amp,
                period_s=10.0 if args.scenario_period is None else args.scenario_period)


def _record_suite(conf, res, args):
    """conf.json's scenario_suite: names, seeds, amp, period (a list of pairs: conf.json keeps lists, not dicts)."""
    conf.scenario_suite = [["names", list(res.scenarios)], ["seeds", list(res.seeds)],
                           ["amp", float(conf.reset_max_u if args.scenario_amp is None else args.scenario_amp)],
                           ["period_s", 10.0 if args.scenario_period is None else float(args.scenario_period)]]


def _slice(res, e):
    """Experiment e's CaseResults (DisturbedResults) of a batch's ([E, P, ...] arrays)."""
    from .evaluator import CaseResults, DisturbedResults

    rest = (res.seeds, res.T, res.scores[e], res.counters[e], {k: v[e] for k, v in res.metrics.items()})
    return DisturbedResults(res.scenarios, res.disturbances, *rest) if isinstance(res, DisturbedResults) else CaseResults(res.scenarios, *rest)


def _write_suite(d, conf, res, tags, args):
    """scenarios.csv and conf.json's scenario_suite from a CaseResults; from a DisturbedResults (--disturb) the same from its nominal
    slice, plus robustness.csv and conf.json's robustness_suite (a list of [name, [[key, value], ...]] pairs). -> the nominal results."""
    from . import scenarios as _sc
    from .evaluator import DisturbedResults

    nominal = res
    if isinstance(res, DisturbedResults):
        nominal = res.nominal()
        _sc.write_robustness_csv(os.path.join(d, "robustness.csv"), res, tags)
        conf.robustness_suite = [[x.name, x.items()] for x in _disturb(args)]
    _sc.write_csv(os.path.join(d, "scenarios.csv"), nominal, tags)
    _record_suite(conf, nominal, args)
    return nominal


def _keep_start(vt, args):
    """--keep_best: the snapshot slabs and the rollout batch, then the evaluation at step 0. Without the flag: nothing."""
    if getattr(args, "keep_best", None) is not None:
        vt.enable_keep_best(args.keep_best_seeds)
        vt.keep_best_update(0)


def _keep_tick(vt, args, k, total):
    """--keep_best: the evaluation after step k, at every multiple of the interval and at the last step."""
    if getattr(args, "keep_best", None) is not None and (k % args.keep_best == 0 or k == total):
        vt.keep_best_update(k)


class _KeepResults:
    """What a --keep_best run writes, read once after training: the retained actors (VecTrainer.best_agents), their simulation rewards
    (run_simulations on them) and suite (--scenarios), the units' best score and step and the final actors' score."""

    def __init__(self, vt, args):
        self.vt, self.args = vt, args
        self.agents = vt.best_agents()
        self.sims = vt.run_simulations(agents=self.agents)
        self.score, self.step = vt.best_scores()
        self.final = vt.last_scores()
        self.record = [["interval", int(args.keep_best)], ["seeds", list(vt._keep["seeds"])], ["evaluations", int(vt._keep["evaluations"])]]
        self.suite = None
        if args.scenarios is not None:
            kw = dict(agents=self.agents, **_suite(args))
            self.suite = vt.evaluate_scenarios(**kw) if _disturb(args) is None else vt.evaluate_robustness(disturbances=_disturb(args), **kw)
        self.freq = None if _freq(args) is None else _frequency(vt.conf, args).actors(vt, self.agents)

    def write(self, d, conf, n_save, e=None):
        """<d>/best/ and <d>/best.csv of a run (e None) or of experiment e of a batch, and conf.keep_best. conf: the directory's Config as
        its conf.json is about to be written."""
        import copy

        import numpy as np

        from . import artifacts

        vt, args = self.vt, self.args
        if e is None:
            units, sims, agents, suite, freq, P = range(len(self.score)), self.sims, self.agents, self.suite, self.freq, vt.P
        else:
            units = [e] if vt.shared else range(e * vt.P_exp, (e + 1) * vt.P_exp)
            sims, agents, P = self.sims[e], self.agents.experiment_view(e, vt.E, vt.M, vt.shared), vt.P_exp
            suite = None if self.suite is None else _slice(self.suite, e)
            freq = None if self.freq is None else _freq_slice(self.freq, e)
        with open(os.path.join(d, "best.csv"), "w") as f:
            f.write("unit,best_step,best_score,final_score\n")
            for i, u in enumerate(units):
                f.write(f"{i},{int(self.step[u])},{'%.9g' % float(self.score[u])},{'%.9g' % float(self.final[u])}\n")
        bd = os.path.join(d, "best")
        os.makedirs(bd, exist_ok=True)
        artifacts.save_agents(bd, agents, n_save, vt.M, shared=vt.shared)
        cb = copy.copy(conf)
        cb.pl_rews_for_simulations = list(sims)
        cb.pl_rew_for_simulation = float(np.average(sims))
        cb.saved_platoons = int(n_save)
        cb.keep_best = self.record
        if suite is not None:
            _write_suite(bd, cb, suite, range(1, P + 1), args)
        if freq is not None:
            _frequency(vt.conf, args).write(bd, cb, freq, range(1, P + 1))
        artifacts.config_writer(os.path.join(bd, "conf.json"), cb)
        conf.keep_best = self.record[:2] + [["best_pl_rew_for_simulation", cb.pl_rew_for_simulation]]


def get_cmdl_args(argv, conf):
    ap = argparse.ArgumentParser(prog="python -m avddpg_amd", description="avddpg hot path on MI355X")
    sub = ap.add_subparsers(dest="mode")
    tr = sub.add_parser("tr", help="run in training mode")
    tr.add_argument("--seed", type=int, default=conf.random_seed)
    tr.add_argument("--method", choices=[conf.exact, conf.euler])
    tr.add_argument("--rand_states", type=bool)
    tr.add_argument("--total_time_steps", type=int)
    tr.add_argument("--pl_num", type=int)
    tr.add_argument("--pl_size", type=int)
    tr.add_argument("--buffer_size", type=int)
    tr.add_argument("--actor_lr", type=float)
    tr.add_argument("--critic_lr", type=float)
    tr.add_argument("--fed_method", choices=[conf.interfrl, conf.intrafrl, conf.nofrl])
    tr.add_argument("--fed_update_count", type=int)
    tr.add_argument("--fed_cutoff_ratio", type=float)
    tr.add_argument("--fed_update_delay", type=float)
    tr.add_argument("--fed_weight_enabled", type=bool, default=False)
    tr.add_argument("--fed_weight_window", type=int)
    tr.add_argument("--fed_agg_method", type=str, choices=["gradients", "weights"])
    tr.add_argument("--intra_directional_averaging", type=bool, default=True)
    tr.add_argument("--rng", choices=["host", "device"], default="host",
                    help="host: reference RNG stream (fixed-seed parity); device: Philox in the kernels (throughput)")
    tr.add_argument("--engine", choices=["per_agent", "batched", "fused", "fused3"], default=None,
                    help="interfrl with every step federated (shared weight sets): per_agent = exact f32 kernel per agent + federated "
                         "sum (default); fused3 = split-operand set learner, f32-class results, ~4x faster; fused / batched = bf16 "
                         "operands (not in the reference CLI)")
    tr.add_argument("--episodes", choices=["reference", "platoon"], default="reference",
                    help="reference: the episode loop of workers/trainer.py:232-273 on the host (any terminal platoon ends the episode of "
                         "all; per-episode reward CSVs in the reference's schema). platoon: THROUGHPUT mode (needs --rng device): "
                         "total_time_steps steps with every platoon running its own episodes on the device (avd_episode_end_f32), no "
                         "host synchronisation per step; writes curve.csv (episodes closed, mean episodic reward and length per "
                         "reporting window, evaluator score) instead of the per-episode CSVs (not in the reference CLI). The schedule "
                         "flags keep their meaning on an episode-EQUIVALENT clock (step // steps_per_episode: --fed_update_count, "
                         "--fed_cutoff_ratio); --fed_weight_enabled weights every agent by |1 / mean of its last fed_weight_window closed "
                         "episodes' rewards| from a device-side history, from step fed_weight_window x steps_per_episode on; conf.json "
                         "records the rule (episodes_mode, episode_clock)")
    tr.add_argument("--report_every", type=int, default=10000, help="--episodes platoon: steps per curve point")
    tr.add_argument("--eval_platoons", type=str, default=None, metavar="N|all",
                    help="--episodes platoon: also score the actors of the first N platoons (or all) at every curve point with one "
                         "launch of the evaluator rollout kernel; adds the columns evaluator_mean,evaluator_min,evaluator_max to "
                         "curve.csv (not in the reference CLI)")
    tr.add_argument("--save_platoons", type=int, default=None,
                    help="checkpoint the agents of the first N platoons only (default: all with --episodes reference, 4 with platoon)")
    tr.add_argument("--seeds", type=str, default=None, metavar="LIST",
                    help="--rng device --episodes platoon: train one independent experiment per seed (e.g. 1,2,5-8) in ONE process and "
                         "launch chain; experiment k is bit-for-bit what `tr --seed k` trains alone wherever no set learner reduces over "
                         "platoons (nofrl; interfrl --engine per_agent). Writes <out>/<timestamp>/seed<k>/ per seed (curve.csv, the "
                         "actors, conf.json). Not with --seed, intrafrl, weights aggregation or the centralized framework (not in the "
                         "reference CLI)")
    tr.add_argument("--sweep", action="append", default=None, metavar="NAME=V1,V2,...",
                    help="--rng device --episodes platoon: a hyperparameter sweep in ONE process and launch chain over actor_lr, critic_lr, "
                         "tau, gamma, std_dev or theta (repeat the flag for a grid; the last flag varies fastest), times --seeds (or "
                         "--seed). Experiment (values, k) is bit-for-bit what `tr --seed k` with those values trains alone (nofrl; "
                         "interfrl --engine per_agent; --engine fused3: what `tr --seeds` with those values trains). Writes <out>/<timestamp>/<label>/seed<k>/ per experiment and sweep.csv (not in "
                         "the reference CLI)")
    tr.add_argument("--pbt", type=int, default=None, metavar="STEPS",
                    help="with --sweep: population-based training -- every STEPS steps (not at the last) rank the experiments by the mean "
                         "evaluator score of their platoons, copy the learners (weights, targets, BN statistics, Adam state) of members of "
                         "the top fraction onto the bottom fraction and give those their parent's values times factors drawn from "
                         "--pbt_perturb; environments, OU noise, replay and seeds stay. Writes <out>/<timestamp>/pbt.csv (not in the "
                         "reference CLI)")
    tr.add_argument("--pbt_fraction", type=float, default=None, help="--pbt: the share of experiments replaced per generation, in (0, 0.5] "
                                                                        "(default 0.25)")
    tr.add_argument("--pbt_perturb", type=str, default=None, metavar="F1,F2,...",
                    help="--pbt: the factors a replaced experiment's swept values are multiplied by, one drawn per value (default 0.8,1.2)")
    tr.add_argument("--train_disturb", action="append", default=None, metavar="NAME[:key=val,...]",
                    help="--rng device: TRAIN under disturbance levels (domain randomisation; repeat the flag for more levels, at most 16): "
                         "platoon p trains under level p %% n_levels for the whole run. The keys are --disturb's (noise_ep, noise_ev, noise_a, "
                         "v2v_delay, v2v_drop, dyn_coeff); a bare NAME is the undisturbed level, a clean share of platoons. The replay holds "
                         "what the agents observed; rewards and episodes come from the true state. conf.json records the levels as "
                         "train_disturbances. Composes with --seeds, --scenarios and --disturb; not with --sweep / --pbt, the centralized "
                         "framework or a process group (not in the reference CLI)")
    tr.add_argument("--train_leader", action="append", default=None, metavar="NAME[:key=val,...]",
                    help="--rng device: TRAIN under leader manoeuvres (repeat the flag for more, at most 16): platoon p's leader follows "
                         "manoeuvre (p // n_levels) %% n_manoeuvres for the whole run (n_levels: the --train_disturb level count, 1 without). "
                         "Keys: profile (one of --scenarios' names; default: NAME if it is one, else gaussian), amp, period (as "
                         "--scenario_amp / --scenario_period) and noise (times the step's unit draw, on top of the profile; default 0). The "
                         "input at step k of the platoon's own episode is the array --scenarios evaluates with. The gaussian profile is the "
                         "reference's training input, a clean share (noise: its scale, default reset_max_u; no amp or period). conf.json "
                         "records the manoeuvres as train_leader. Composes with --seeds, --train_disturb, --scenarios and --disturb; not with "
                         "--sweep / --pbt, --rng host, the centralized framework or a process group (not in the reference CLI)")
    tr.add_argument("--residual", type=str, default=None, metavar="SPEC",
                    help="--rng device: train the actors as a RESIDUAL on a static linear law, kp=..,kv=..[,ka=..,kf=..,scale=..] (scale in "
                         "(0, 1], default 1: the correction's authority), or the word `tuned`: the law --baseline_tune's grid picks on the "
                         "--scenarios suite, searched before training. The plant receives clip(law(observation) + scale * action); the "
                         "replay and the learners keep the action. conf.json records residual_law, and `esim <dir>` applies it in every "
                         "mode. Composes with --seeds, --train_disturb, --train_leader, --keep_best, --scenarios, --disturb, --baseline "
                         "and every --engine; not with --sweep / --pbt, --rng host, the centralized framework or a process group of "
                         "more than one rank (not in the reference CLI)")
    tr.add_argument("--warm_start", type=str, default=None, metavar="SPEC",
                    help="--rng device: before training, FIT the actors to a static linear law on the device (imitation pre-training): "
                         "kp=..,kv=..[,ka=..,kf=..,steps=..,lr=..,ep=..,ev=..,a=..], or the word `tuned` / `searched` (the law "
                         "--baseline_tune / --baseline_search finds on the --scenarios suite). steps (default 2000) Adam steps of size lr "
                         "(1e-3) on batches of 64 states uniform in the box +-(ep, ev, a, a) (defaults reset_ep_max, reset_max_ev, 1), the "
                         "target the law's clipped action; critics, targets' relation to their nets and every Adam state stay as "
                         "constructed. conf.json records warm_start (the law, the mean final fit loss, the fitted actors' evaluator score); "
                         "with --keep_best the step-0 snapshot is the fitted actors. Composes with --seeds, --train_disturb, --train_leader, "
                         "--keep_best and every --engine; not with --residual, --sweep / --pbt, --rng host, the centralized framework or a "
                         "process group of more than one rank (not in the reference CLI)")
    tr.add_argument("--anchor", type=str, default=None, metavar="SPEC",
                    help="anchor the actors to a linear CACC law WHILE they train (TD3+BC's behaviour-cloning term): kp=2,kv=1[,ka=..,kf=..,"
                         "weight=..,decay=..]; the word tuned / searched may stand in place of the gains (the law --baseline_tune / "
                         "--baseline_search finds), followed by the other keys. The actor loss becomes -q(s, mu(s)) + weight * (mu(s) - "
                         "u*(s))^2, u* the law's clipped action on the sampled state, added to the critic's action gradient in the split set "
                         "learner's seed launch; weight >= 0 (default 1), decay = N ramps it linearly to 0 over the first N learner calls "
                         "(0: constant). conf.json records anchor (the law, and the mean (mu - u*)^2 per weight set at the first and the "
                         "last learner call). Needs --engine fused3 (shared-set interfrl); combines with --seeds, --warm_start, "
                         "--actor_hold, --train_disturb, --train_leader, --keep_best and --residual (the target is then a law for the "
                         "correction); not with --sweep / --pbt, a process group of more than one rank or the centralized framework "
                         "(not in the reference CLI)")
    tr.add_argument("--target_noise", type=str, default=None, metavar="SPEC",
                    help="target policy smoothing (TD3's): sigma=0.2[,clip=0.5]; the critic's targets evaluate the target critic at "
                         "clip(mu'(s') + clip(sigma n, -clip, clip), action bounds), n ~ N(0, 1) per sampled row drawn on the device, in one "
                         "small launch of the split set learner's chain; clip defaults to 2.5 sigma (inf: no noise clip), sigma 0 trains what "
                         "the run without the flag trains. conf.json records target_noise (sigma, clip). Needs --engine fused3 (shared-set "
                         "interfrl) and --rng device; combines with --seeds, --anchor, --warm_start, --actor_hold, --residual, "
                         "--train_disturb, --train_leader and --keep_best; not with --sweep / --pbt, a process group of more than one rank "
                         "or the centralized framework (not in the reference CLI)")
    tr.add_argument("--policy_delay", type=str, default=None, metavar="D",
                    help="delayed policy updates (TD3's): the actors and every target network move on every D-th learner call only (call "
                         "k, 0-based, iff (k + 1) %% D == 0); on the others the critic alone takes its Adam step, from a TD-only learn call "
                         "that computes nothing of the actor's half of the chain, and the actors keep an Adam count of their own. D = 1 "
                         "trains what the run without the flag trains. conf.json records policy_delay. Needs --engine fused3 (shared-set "
                         "interfrl) and --rng device; combines with --seeds, --anchor (acts on policy calls), --target_noise, --warm_start, "
                         "--actor_hold, --residual, --train_disturb, --train_leader and --keep_best; not with --sweep / --pbt, a process "
                         "group of more than one rank or the centralized framework (not in the reference CLI)")
    tr.add_argument("--actor_hold", type=int, default=None, metavar="N",
                    help="hold the actors still for the first N learner calls (the steps past the replay gate): the actor's step size "
                         "handed to the update is 0 for them, so the critic learns to evaluate the policy it was handed (a --warm_start fit, "
                         "or a --residual law) before the actors move; the configuration's step size afterwards. conf.json records "
                         "actor_hold. N from 1 to below the run's step count; not with --sweep / --pbt (not in the reference CLI)")
    tr.add_argument("--keep_best", type=int, default=None, metavar="STEPS",
                    help="keep the best actors seen in training, on the device: at step 0, at every multiple of STEPS and at the last step "
                         "one evaluator rollout launch scores every rollout group (a platoon's actors; the shared sets; each experiment's of "
                         "--seeds / --sweep / --pbt) on the undisturbed evaluator, and a group whose mean score beats its best so far has its "
                         "actors copied into a snapshot, without a host round trip. Writes <dir>/best/ (the retained actors of the saved "
                         "platoons under the usual file names, with a conf.json: `esim <dir>/best` works) and <dir>/best.csv (unit, "
                         "best_step, best_score, final_score); conf.json gains keep_best, sweep.csv the column best_pl_rew_for_simulation. "
                         "The saved final actors and every other output stay what they are without the flag. Not under a process group of "
                         "more than one rank (not in the reference CLI)")
    tr.add_argument("--keep_best_seeds", type=str, default=None, metavar="LIST",
                    help="--keep_best: the evaluation seeds the retention score averages over (e.g. 6,7-9; default: the configuration's "
                         "evaluation_seed)")
    _scenario_flags(tr, "after training, beside the simulation rewards:")
    tr.add_argument("--out", type=str, default=".outputs")
    es = sub.add_parser("esim", help="run in evaluation/simulator mode")
    es.add_argument("exp_path", type=str)
    es.add_argument("--n_timesteps", type=int, default=100)
    _scenario_flags(es, "instead of the per-platoon rollouts of --n_timesteps steps (the scenarios run the full episode length):")
    args = ap.parse_args(argv)
    if args.mode in ("tr", "esim"):
        _check_scenario_flags(ap, args)
    if getattr(args, "save_platoons", None) is not None and args.save_platoons < 1:
        ap.error("--save_platoons must be >= 1 (esim reloads platoon 1's actors)")
    if getattr(args, "seeds", None) is not None:
        if args.rng != "device" or args.episodes != "platoon":
            ap.error("--seeds needs --rng device --episodes platoon")
        if any(a == "--seed" or a.startswith("--seed=") for a in argv):
            ap.error("--seeds and --seed are mutually exclusive")
        try:
            args.seeds = parse_seeds(args.seeds)
        except ValueError as e:
            ap.error(str(e))
    if getattr(args, "sweep", None) is not None:
        if args.rng != "device" or args.episodes != "platoon":
            ap.error("--sweep needs --rng device --episodes platoon")
        try:
            args.sweep = parse_sweep(args.sweep)
        except ValueError as e:
            ap.error(str(e))
        for name, _ in args.sweep:  # (the parsed values: argparse also takes abbreviations such as --actor)
            if getattr(args, name, None) is not None:
                ap.error(f"--sweep {name} and --{name} are mutually exclusive")
    if getattr(args, "train_disturb", None) is not None:
        from .scenarios import check_disturbances, parse_disturbance

        if args.rng != "device":
            ap.error("--train_disturb needs --rng device")
        if args.sweep is not None:
            ap.error("--train_disturb does not combine with --sweep / --pbt")
        if int(os.environ.get("WORLD_SIZE", "1") or 1) > 1:
            ap.error("--train_disturb is not available under a process group of more than one rank")
        try:  # (the Model A refusal and the level cap need the run's configuration: trainer.check_train_disturb applies them)
            args.train_disturb = check_disturbances([parse_disturbance(d) for d in args.train_disturb])
        except ValueError as e:
            ap.error(f"--train_disturb: {e}")
    if getattr(args, "train_leader", None) is not None:
        from .scenarios import check_manoeuvres, parse_manoeuvre

        if args.rng != "device":
            ap.error("--train_leader needs --rng device")
        if args.sweep is not None or args.pbt is not None:
            ap.error("--train_leader does not combine with --sweep / --pbt")
        if int(os.environ.get("WORLD_SIZE", "1") or 1) > 1:
            ap.error("--train_leader is not available under a process group of more than one rank")
        try:  # (what needs the run's configuration: trainer.check_train_leader applies it)
            args.train_leader = check_manoeuvres([parse_manoeuvre(m) for m in args.train_leader])
        except ValueError as e:
            ap.error(f"--train_leader: {e}")
    if getattr(args, "residual", None) is not None:
        from . import scenarios as _sc

        if args.rng != "device":
            ap.error("--residual needs --rng device")
        if args.sweep is not None or args.pbt is not None:
            ap.error("--residual does not combine with --sweep / --pbt")
        if int(os.environ.get("WORLD_SIZE", "1") or 1) > 1:
            ap.error("--residual is not available under a process group of more than one rank")
        try:  # (what needs the run's configuration: trainer.check_residual applies it)
            args.residual = _sc.parse_residual(args.residual)
            if args.residual not in (_sc.TUNED, _sc.SEARCHED):
                _sc.check_residual(args.residual)
        except ValueError as e:
            ap.error(f"--residual: {e}")
        if args.residual == _sc.TUNED and (args.scenarios is None or getattr(args, "baseline_tune", None) is None):
            ap.error("--residual tuned needs --scenarios and --baseline_tune (the grid the law is searched on)")
        if args.residual == _sc.SEARCHED and (args.scenarios is None or getattr(args, "baseline_search", None) is None):
            ap.error("--residual searched needs --scenarios and --baseline_search (the space the law is searched in)")
    if getattr(args, "warm_start", None) is not None:
        from . import scenarios as _sc

        if args.rng != "device":
            ap.error("--warm_start needs --rng device")
        if args.sweep is not None or args.pbt is not None:
            ap.error("--warm_start does not combine with --sweep / --pbt")
        if getattr(args, "residual", None) is not None:
            ap.error("--warm_start does not combine with --residual (the law would act twice)")
        if int(os.environ.get("WORLD_SIZE", "1") or 1) > 1:
            ap.error("--warm_start is not available under a process group of more than one rank")
        try:  # (what needs the run's configuration: trainer.check_warm_start applies it)
            args.warm_start = _sc.parse_warm_start(args.warm_start)
            if args.warm_start not in (_sc.TUNED, _sc.SEARCHED):
                _sc.check_warm_start(args.warm_start)
        except ValueError as e:
            ap.error(f"--warm_start: {e}")
        if args.warm_start == _sc.TUNED and (args.scenarios is None or getattr(args, "baseline_tune", None) is None):
            ap.error("--warm_start tuned needs --scenarios and --baseline_tune (the grid the law is searched on)")
        if args.warm_start == _sc.SEARCHED and (args.scenarios is None or getattr(args, "baseline_search", None) is None):
            ap.error("--warm_start searched needs --scenarios and --baseline_search (the space the law is searched in)")
    if getattr(args, "anchor", None) is not None:
        from . import scenarios as _sc

        if args.sweep is not None or args.pbt is not None:
            ap.error("--anchor does not combine with --sweep / --pbt (the table-driven learn call has no anchored form)")
        if args.engine != "fused3":
            ap.error(f"--anchor needs --engine fused3 (the split set learner holds the anchored seed), got --engine {args.engine}")
        if int(os.environ.get("WORLD_SIZE", "1") or 1) > 1:
            ap.error("--anchor is not available under a process group of more than one rank")
        try:  # (what needs the run's configuration: trainer.check_anchor applies it)
            args.anchor = _sc.parse_anchor(args.anchor)
            _sc.check_anchor(args.anchor)
        except ValueError as e:
            ap.error(f"--anchor: {e}")
        if args.anchor.pending and args.anchor.source == _sc.TUNED and (args.scenarios is None or getattr(args, "baseline_tune", None) is None):
            ap.error("--anchor tuned needs --scenarios and --baseline_tune (the grid the law is searched on)")
        if args.anchor.pending and args.anchor.source == _sc.SEARCHED and (args.scenarios is None or getattr(args, "baseline_search", None) is None):
            ap.error("--anchor searched needs --scenarios and --baseline_search (the space the law is searched in)")
    if getattr(args, "target_noise", None) is not None:
        from . import trainer as _tr

        if args.sweep is not None or args.pbt is not None:
            ap.error("--target_noise does not combine with --sweep / --pbt (the table-driven learn call has no smoothed form)")
        if args.engine != "fused3":
            ap.error(f"--target_noise needs --engine fused3 (the split set learner holds the smoothing launch), got --engine {args.engine}")
        if args.rng != "device":
            ap.error("--target_noise needs --rng device (the noise is drawn by the device's generator)")
        if int(os.environ.get("WORLD_SIZE", "1") or 1) > 1:
            ap.error("--target_noise is not available under a process group of more than one rank")
        try:  # (what needs the run's configuration is checked below, once it exists)
            args.target_noise = _tr.check_target_noise(_tr.TargetNoise.parse(args.target_noise))
        except ValueError as e:
            ap.error(f"--target_noise: {e}")
    if getattr(args, "policy_delay", None) is not None:
        from . import trainer as _tr

        if args.sweep is not None or args.pbt is not None:
            ap.error("--policy_delay does not combine with --sweep / --pbt (the experiment copy and the table-driven update know one Adam "
                     "count per weight set)")
        if args.engine != "fused3":
            ap.error(f"--policy_delay needs --engine fused3 (the split set learner holds the TD-only call), got --engine {args.engine}")
        if args.rng != "device":
            ap.error("--policy_delay needs --rng device (the fused3 engine's device-side run)")
        if int(os.environ.get("WORLD_SIZE", "1") or 1) > 1:
            ap.error("--policy_delay is not available under a process group of more than one rank")
        try:  # (what needs the run's configuration is checked below, once it exists)
            try:
                d = int(args.policy_delay)
            except ValueError:
                raise ValueError(f"policy delay: D={args.policy_delay!r} must be a whole number >= 1") from None
            args.policy_delay = _tr.check_policy_delay(d)
        except ValueError as e:
            ap.error(f"--policy_delay: {e}")
    if getattr(args, "actor_hold", None) is not None:
        if args.actor_hold < 1:
            ap.error(f"--actor_hold: N={args.actor_hold} must be >= 1")
        if args.sweep is not None or args.pbt is not None:
            ap.error("--actor_hold does not combine with --sweep / --pbt")
    if getattr(args, "pbt", None) is not None or getattr(args, "pbt_fraction", None) is not None or getattr(args, "pbt_perturb", None) is not None:
        if args.pbt is None:
            ap.error("--pbt_fraction / --pbt_perturb need --pbt")
        from .pbt import check_pbt

        try:
            perturb = [float(f) for f in (args.pbt_perturb if args.pbt_perturb is not None else "0.8,1.2").split(",")]
        except ValueError:
            ap.error(f"--pbt_perturb: {args.pbt_perturb!r} is not a comma-separated list of numbers")
        fraction = 0.25 if args.pbt_fraction is None else args.pbt_fraction
        swept = [n for n, _ in args.sweep] if args.sweep is not None else None
        n_exp = len(sweep_experiments(args.sweep, args.seeds if args.seeds is not None else [args.seed])) if swept else 0
        try:
            args.pbt, args.pbt_fraction, args.pbt_perturb, _ = check_pbt(args.pbt, fraction, perturb, n_exp, swept)
        except ValueError as e:
            ap.error(f"--pbt: {e}")
    if getattr(args, "keep_best_seeds", None) is not None and args.keep_best is None:
        ap.error("--keep_best_seeds needs --keep_best")
    if getattr(args, "keep_best", None) is not None:
        if args.keep_best < 1:
            ap.error(f"--keep_best: STEPS={args.keep_best} must be >= 1")
        if int(os.environ.get("WORLD_SIZE", "1") or 1) > 1:
            ap.error("--keep_best is not available under a process group of more than one rank (the snapshot is not gathered across ranks)")
        if args.keep_best_seeds is not None:
            try:
                args.keep_best_seeds = parse_seeds(args.keep_best_seeds)
            except ValueError as e:
                ap.error(str(e).replace("--seeds", "--keep_best_seeds"))
    ev = getattr(args, "eval_platoons", None)
    if ev is not None:
        if args.episodes != "platoon":
            ap.error("--eval_platoons needs --episodes platoon")
        if ev != "all" and not (ev.isdigit() and int(ev) >= 1):
            ap.error("--eval_platoons takes a platoon count >= 1 or 'all'")
    conf = set_args_to_config(args, conf)
    if args.mode == "tr":  # (esim checks against the configuration it loads)
        _check_baseline_conf(args, conf, ap.error)
        _check_freq_conf(args, conf, ap.error)
        if getattr(args, "actor_hold", None) is not None and args.actor_hold >= conf.total_time_steps:
            ap.error(f"--actor_hold: N={args.actor_hold} must be below the run's {conf.total_time_steps} steps")
        ws = getattr(args, "warm_start", None)
        if ws is not None and not isinstance(ws, str):  # (`tuned` / `searched`: checked once the law exists, _resolve_warm_start)
            from . import trainer as _tr

            try:
                _tr.check_warm_start(conf, ws, args.rng, 1, residual=getattr(args, "residual", None))
            except ValueError as e:
                ap.error(f"--warm_start: {e}")
        an = getattr(args, "anchor", None)
        if an is not None and not an.pending:  # (`tuned` / `searched`: checked once the law exists, _resolve_anchor)
            from . import trainer as _tr

            try:
                _tr.check_anchor(conf, an, args.engine, 1)
            except ValueError as e:
                ap.error(f"--anchor: {e}")
        if getattr(args, "target_noise", None) is not None:
            from . import trainer as _tr

            try:
                _tr.check_target_noise(args.target_noise, conf, args.engine, args.rng, 1)
            except ValueError as e:
                ap.error(f"--target_noise: {e}")
        if getattr(args, "policy_delay", None) is not None:
            from . import trainer as _tr

            try:
                _tr.check_policy_delay(args.policy_delay, conf, args.engine, args.rng, 1, steps=conf.total_time_steps)
            except ValueError as e:
                ap.error(f"--policy_delay: {e}")
    return args, conf


def set_args_to_config(args, conf):
    """src/cmd/api.py:5-50."""
    g = lambda n: getattr(args, n, None)
    if g("seed") is not None:
        conf.random_seed = args.seed
    for flag, field in (("method", "method"), ("rand_states", "rand_states"), ("total_time_steps", "total_time_steps"),
                        ("pl_num", "num_platoons"), ("pl_size", "pl_size"), ("buffer_size", "buffer_size"),
                        ("actor_lr", "actor_lr"), ("critic_lr", "critic_lr"), ("fed_method", "fed_method"),
                        ("fed_update_count", "fed_update_count"), ("fed_cutoff_ratio", "fed_cutoff_ratio"),
                        ("intra_directional_averaging", "intra_directional_averaging"),
                        ("fed_update_delay", "fed_update_delay"), ("fed_weight_enabled", "weighted_average_enabled"),
                        ("fed_weight_window", "weighted_window"), ("fed_agg_method", "aggregation_method")):
        if g(flag) is not None:
            setattr(conf, field, getattr(args, flag))
    return conf.refresh()


def main(argv=None, conf=None):
    """conf: the Config the flags override (the reference edits src/config.py for anything the CLI has no flag for,
    e.g. ``framework``); default Config()."""
    conf = Config() if conf is None else conf
    args, conf = get_cmdl_args(sys.argv[1:] if argv is None else argv, conf)
    if args.mode == "tr":
        import numpy as np

        from . import artifacts, trainer
        np.random.seed(conf.random_seed)  # rand.set_global_seed (src/rand.py:6-15)
        base = os.path.join(args.out, datetime.datetime.now().strftime("%y%m%d_%H%M%S"))
        os.makedirs(base, exist_ok=True)
        if args.sweep is not None:
            train_sweep(args, conf, base)
            print(base)
            return
        if args.seeds is not None:
            train_seed_batch(args, conf, base)
            print(base)
            return
        if args.episodes == "platoon":
            if args.rng != "device":
                raise SystemExit("--episodes platoon needs --rng device")
            from . import evaluator
            nofrl = conf.fed_method == conf.nofrl
            _check_train_leader(args, conf, "platoon")
            _resolve_residual(args, conf, "platoon")
            _resolve_warm_start(args, conf)
            _resolve_anchor(args, conf)
            try:
                vt = trainer.VecTrainer(conf, rng="device", auto_reset="platoon", shared_engine=args.engine, fused_update=nofrl,
                                        train_disturb=args.train_disturb, **_lead_kw(args), **_residual_kw(args), **_warm_kw(args), **_anchor_kw(args), **_noise_kw(args), **_delay_kw(args))
            except ValueError as e:
                if args.train_disturb is None:
                    raise
                raise SystemExit(f"--train_disturb: {e}")
            vt.reset_episode()
            _warm_fit(vt, args)
            _keep_start(vt, args)
            rng_state = np.random.get_state()

            def score():  # workers/evaluator.py:145 on platoon 1's actors (the evaluator reseeds the global legacy RNG: put it back)
                grp = vt.agents
                if not vt.shared:
                    import copy
                    grp = copy.copy(vt.agents)
                    grp.theta, grp.stats, grp.n_sets = vt.agents.theta[:vt.M], vt.agents.stats[:vt.M], vt.M
                if vt.residual is not None:  # the residual policy's score: the rollout kernel with the law (the same value a batch writes)
                    # (no set_state here as below: run_many restores the global np.random state itself -- with the zero law this line
                    # must leave every later draw, and so every output file, what the path below leaves)
                    return float(evaluator.run_many(conf, grp, [0], set_mod=vt.M if vt.shared else 0, base_law=vt.residual)[0][0, 0])
                r = evaluator.run(conf=conf, actors=grp, pl_idx=1, set_mod=vt.M if vt.shared else 0)[0]
                np.random.set_state(rng_state)
                return float(r)

            n_eval = None if args.eval_platoons is None else (vt.P if args.eval_platoons == "all" else min(vt.P, int(args.eval_platoons)))

            def many():  # the first n_eval platoons' scores from one rollout launch: mean, min, max (evaluator.run_many)
                if n_eval is None:
                    return ""
                sc = vt.evaluator_scores(range(n_eval))
                return f",{float(np.mean(sc)):.3f},{float(np.min(sc)):.3f},{float(np.max(sc)):.3f}"

            with open(os.path.join(base, "curve.csv"), "w") as f:
                extra = "" if n_eval is None else ",evaluator_mean,evaluator_min,evaluator_max"
                f.write(f"step,episodes_closed,mean_episodic_reward,mean_episode_length,evaluator_score{extra}\n")
                f.write(f"0,0,,,{score():.3f}{many()}\n")
                for k in range(1, conf.total_time_steps + 1):
                    vt.step()
                    _keep_tick(vt, args, k, conf.total_time_steps)
                    if k % args.report_every == 0 or k == conf.total_time_steps:
                        r, ln, n = vt.env.pop_episode_stats()
                        f.write(f"{k},{n},{r:.5f},{ln:.2f},{score():.3f}{many()}\n")
                        f.flush()
            if vt.nonfinite_updates():
                print(f"warning: {vt.nonfinite_updates()} weight-set updates were skipped for non-finite gradients", file=sys.stderr)
        else:
            _check_train_leader(args, conf, False)
            _resolve_residual(args, conf, False)
            _resolve_warm_start(args, conf)
            _resolve_anchor(args, conf)
            try:
                vt = trainer.VecTrainer(conf, rng=args.rng, auto_reset=False, shared_engine=args.engine, train_disturb=args.train_disturb,
                                        **_lead_kw(args), **_residual_kw(args), **_warm_kw(args), **_anchor_kw(args), **_noise_kw(args), **_delay_kw(args))
            except ValueError as e:
                if args.train_disturb is None:
                    raise
                raise SystemExit(f"--train_disturb: {e}")
            _warm_fit(vt, args)
            _keep_start(vt, args)
            ep, avg = vt.run(keep_best_every=args.keep_best)
            if args.keep_best is not None and vt.steps_total % args.keep_best:  # the last step
                vt.keep_best_update(vt.steps_total)
            artifacts.generate_csvs(base, conf, ep, avg)
        # Trainer.run / run_simulations (workers/trainer.py:277-280, 537-550): every platoon's evaluator score / re_scalar and their
        # average, written into conf.json (the evaluator reseeds the global legacy RNG; run_many puts it back)
        conf.pl_rews_for_simulations = vt.run_simulations()
        conf.pl_rew_for_simulation = float(np.average(conf.pl_rews_for_simulations))
        if args.scenarios is not None:  # every local platoon over scenarios (x disturbances) x seeds, one launch
            res = vt.evaluate_scenarios(**_suite(args)) if _disturb(args) is None else vt.evaluate_robustness(disturbances=_disturb(args), **_suite(args))
            _write_suite(base, conf, res, range(1, vt.P + 1), args)
            if _baseline_flags(args) is not None:
                _baselines(conf, args).write(base, conf, res)
        if _freq(args) is not None:  # the same platoons and laws over the frequency sweep, one launch each
            _frequency(conf, args).write(base, conf, _frequency(conf, args).actors(vt), range(1, vt.P + 1))
        n_save = vt.P if args.save_platoons is None and args.episodes == "reference" else min(vt.P, 4 if args.save_platoons is None else args.save_platoons)
        artifacts.save_agents(base, vt.agents, n_save, vt.M, shared=vt.shared)
        # what ran, beside the reference's fields: how many platoons' agents the directory holds (esim loops over exactly these),
        # which episode rule applied and what the schedule predicates' `training_episode` was
        conf.saved_platoons = int(n_save)
        conf.episodes_mode = args.episodes
        conf.episode_clock = ("workers/trainer.py:232-273: one episode loop for all platoons, any terminal platoon ends it" if args.episodes == "reference"
                              else "per-platoon episodes on the device; schedule predicates on step // steps_per_episode; weighted averaging "
                                   "(if enabled) from step weighted_window x steps_per_episode on, weights from each agent's last "
                                   "weighted_window closed episodes")
        _record_train_levels(conf, args)
        _record_train_leader(conf, args)
        _record_residual(conf, args)
        _record_warm(conf, args)
        _record_anchor(conf, args, vt)
        _record_noise(conf, args)
        _record_delay(conf, args)
        if args.keep_best is not None:
            _KeepResults(vt, args).write(base, conf, n_save)
        artifacts.config_writer(os.path.join(base, "conf.json"), conf)
        print(base)
    elif args.mode == "esim":
        from . import artifacts, evaluator, vec
        conf = artifacts.config_loader(os.path.join(args.exp_path, "conf.json"), Config)
        # model count and shapes as the trainer derives them (workers/evaluator.py:48-66): L models of S states / 1 action
        # decentralized, ONE model of 4L states / L actions and widths x1.2 centralized (src/environment.py:35-52)
        shape = vec.VecPlatoon(1, conf.pl_size, conf, rng="device")  # device RNG: consumes no np.random draws
        M = shape.num_models
        # a run saved with --save_platoons N holds the first N platoons' agents: conf.json says how many (older directories: all)
        import json
        saved = json.load(open(os.path.join(args.exp_path, "conf.json"))).get("saved_platoons", conf.num_platoons)
        law = _saved_residual(args.exp_path)  # (None: the actors alone, today's entry points; read once for every mode below)
        if args.scenarios is not None or _freq(args) is not None:  # ALL saved platoons' actors in one group, one launch
            from . import scenarios as _sc
            saved = int(saved)
            grp = vec.AgentGroup(saved * M, shape.num_states, shape.num_actions, conf, hidd_mult=shape.hidden_multiplier)
            for p in range(1, saved + 1):
                if not os.path.exists(os.path.join(args.exp_path, artifacts.FNAME["actor"] % (p, 1) + ".npz")):
                    raise FileNotFoundError(f"{args.exp_path}: no checkpoint of platoon {p}'s actors (conf.json records {saved} saved platoons)")
                for m in range(M):
                    grp.set_weights((p - 1) * M + m, "actor", artifacts.load_actor_weights(args.exp_path, p, m + 1))
            _check_baseline_conf(args, conf, _exit)
            _check_freq_conf(args, conf, _exit)
            base = None
            if args.scenarios is not None:
                base = _esim_suite(args, conf, grp, saved, law)
            if _freq(args) is not None:  # frequency.csv, and frequency_suite added to the directory's conf.json (nothing else in it changes)
                fq = _Frequency(conf, args, base)
                try:
                    res = evaluator.run_frequency(conf, grp, range(saved), fq.spec, fq.levels, fq.seeds, base_law=law)
                except ValueError as e:
                    raise SystemExit(f"--freq_response: {e}")
                _sc.write_frequency_csv(os.path.join(args.exp_path, "frequency.csv"), fq.entries(res, range(1, saved + 1)))
                path = os.path.join(args.exp_path, "conf.json")
                js = json.load(open(path))
                js["frequency_suite"] = fq.record(res, range(1, saved + 1))
                with open(path, "w") as f:
                    json.dump(js, f)
                print("\n".join(fq.report(res, range(1, saved + 1))))
            return
        for p in range(1, int(saved) + 1):
            if not os.path.exists(os.path.join(args.exp_path, artifacts.FNAME["actor"] % (p, 1) + ".npz")):
                raise FileNotFoundError(f"{args.exp_path}: no checkpoint of platoon {p}'s actors (conf.json records {saved} saved platoons)")
            grp = vec.AgentGroup(M, shape.num_states, shape.num_actions, conf, hidd_mult=shape.hidden_multiplier)
            for m in range(M):
                grp.set_weights(m, "actor", artifacts.load_actor_weights(args.exp_path, p, m + 1))
            if law is not None:  # a residual policy: the rollout kernel with the law in front of the plant
                rew = evaluator.run_many(conf, grp, [0], manual_timestep_override=args.n_timesteps, base_law=law)[0][0, 0]
            else:
                rew, _ = evaluator.run(conf=conf, actors=grp, pl_idx=p, manual_timestep_override=args.n_timesteps)
            print(f"platoon {p}: cumulative platoon reward {rew}")
    else:
        raise SystemExit("modes: tr, esim")


def _esim_suite(args, conf, grp, saved, law):
    """esim --scenarios: the saved platoons over the suite, scenarios.csv (robustness.csv, baseline.csv) and the report lines. -> the
    baseline section, or None without its flags."""
    from . import evaluator
    from . import scenarios as _sc

    full = evaluator.run_cases(conf, grp, range(saved), base_law=law, **_suite(args)) if _disturb(args) is None else \
        evaluator.run_disturbed(conf, grp, range(saved), disturbances=_disturb(args), base_law=law, **_suite(args))
    res = _write_suite(args.exp_path, conf, full, range(1, saved + 1), args)  # (conf.json itself is not rewritten)
    print("\n".join(_sc.report_lines(res, range(1, saved + 1))))
    if _baseline_flags(args) is not None:
        base = _Baselines(conf, args)
        base.write(args.exp_path, conf, full)
        print("\n".join(base.report()))
        return base
    return None


def train_sweep(args, conf, base):
    """`tr --sweep`: one VecTrainer(seeds=..., hparams=...) over the grid x seeds (sweep_experiments), experiment (label, k) written to
    <base>/<label>/seed<k>/ as `tr --seed k` with those values writes its own directory (conf.json holds the values in the reference's
    fields, the grid as `sweep`), and <base>/sweep.csv: one row per experiment with its values, seed, pl_rew_for_simulation and the
    last curve point's evaluator score. With --pbt the values are the final ones and <base>/pbt.csv holds every generation."""
    seeds = list(args.seeds) if args.seeds is not None else [int(conf.random_seed)]
    exps = sweep_experiments(args.sweep, seeds)
    rows = train_seed_batch(args, conf, base, experiments=exps)
    import csv

    with open(os.path.join(base, "sweep.csv"), "w", newline="") as f:
        w = csv.writer(f)
        keep = args.keep_best is not None  # one more column, only under the flag
        w.writerow(["label", *SWEEP_NAMES, "seed", "pl_rew_for_simulation", "final_evaluator_score"] + (["best_pl_rew_for_simulation"] if keep else []))
        for (label, _, k), (ce, last) in zip(exps, rows):
            w.writerow([label, *[repr(float(getattr(ce, n))) for n in SWEEP_NAMES], k, repr(ce.pl_rew_for_simulation), last] +
                       ([repr(dict(ce.keep_best)["best_pl_rew_for_simulation"])] if keep else []))


def train_seed_batch(args, conf, base, experiments=None):
    """`tr --seeds`: the experiments of one VecTrainer(seeds=...) batch, each written to <base>/seed<k>/ exactly as `tr --seed k
    --episodes platoon` writes its own directory (curve.csv, the saved agents, conf.json), plus conf.json's `seed_batch`. The curve
    points' evaluator scores of all experiments come from ONE evaluator rollout launch (VecTrainer.evaluator_scores).
    experiments (`tr --sweep`): [(label, hparams dict, seed)] -> <base>/<label>/seed<k>/, conf.json with the experiment's values and
    `sweep`; returns [(experiment Config, last curve point's evaluator score)]."""
    import csv

    import numpy as np

    from . import artifacts, trainer
    from . import pbt as _pbt
    from .vec import HP_KEYS

    if experiments is None:
        seeds, hps, flag = list(args.seeds), None, "--seeds"
        dirs = [os.path.join(base, f"seed{k}") for k in seeds]
    else:
        seeds, hps, flag = [k for _, _, k in experiments], [h for _, h, _ in experiments], "--sweep"
        dirs = [os.path.join(base, label, f"seed{k}") for label, _, k in experiments]
    E = len(seeds)
    if getattr(args, "train_disturb", None) is not None:  # (its own refusals under its own flag's name)
        try:
            trainer.check_train_disturb(conf, args.train_disturb, "device", None, hparams=hps)
        except ValueError as e:
            raise SystemExit(f"--train_disturb: {e}")
    _check_train_leader(args, conf, "platoon", hparams=hps)
    _resolve_residual(args, conf, "platoon", hparams=hps)
    _resolve_warm_start(args, conf, hparams=hps)
    _resolve_anchor(args, conf, hparams=hps)
    try:
        vt = trainer.VecTrainer(conf, rng="device", auto_reset="platoon", shared_engine=args.engine,
                                fused_update=conf.fed_method == conf.nofrl, seeds=seeds, hparams=hps,
                                train_disturb=getattr(args, "train_disturb", None), **_lead_kw(args), **_residual_kw(args), **_warm_kw(args), **_anchor_kw(args), **_noise_kw(args), **_delay_kw(args))
    except ValueError as e:
        raise SystemExit(f"{flag}: {e}")
    vt.reset_episode()
    _warm_fit(vt, args)
    _keep_start(vt, args)
    P = vt.P_exp
    n_eval = None if args.eval_platoons is None else (P if args.eval_platoons == "all" else min(P, int(args.eval_platoons)))
    last = [None] * E
    for d in dirs:
        os.makedirs(d, exist_ok=True)

    def points():  # per experiment: ",<platoon 1's score>[,mean,min,max of the first n_eval platoons]" from one rollout launch
        sc = vt.evaluator_scores(range(max(1, n_eval or 1)))
        out = []
        for e in range(E):
            line = last[e] = f"{float(sc[e, 0]):.3f}"
            if n_eval is not None:
                row = sc[e, :n_eval]
                line += f",{float(np.mean(row)):.3f},{float(np.min(row)):.3f},{float(np.max(row)):.3f}"
            out.append(line)
        return out

    use_pbt = experiments is not None and getattr(args, "pbt", None) is not None
    lineage = [[] for _ in range(E)]
    pbt_file = open(os.path.join(base, "pbt.csv"), "w", newline="") if use_pbt else None
    if use_pbt:
        pbt_csv = csv.writer(pbt_file)
        pbt_csv.writerow(["generation", "step", "experiment", "label", "seed", "fitness", "rank", "parent", *HP_KEYS])
    swept = [n for n, _ in args.sweep] if experiments is not None else []

    def generation(g, step):  # score (one rollout launch), plan, exploit, set the new values; one pbt.csv row per experiment
        fit = np.mean(vt.evaluator_scores().astype(np.float64), axis=1)
        pairs, new_rows = _pbt.plan(fit, vt.hp_rows, swept, g, vt.seeds, args.pbt_fraction, args.pbt_perturb)
        vt.exploit(pairs)
        vt.set_hparams(new_rows)
        rank = {e: r + 1 for r, e in enumerate(_pbt.ranking(fit))}
        parent = {dst: src for src, dst in pairs}
        for e, (label, _, k) in enumerate(experiments):
            vals = [vt.hp_rows[e][n] for n in HP_KEYS]
            pbt_csv.writerow([g, step, e, label, k, repr(float(fit[e])), rank[e], parent.get(e, ""), *[repr(float(x)) for x in vals]])
            lineage[e].append(dict(generation=g, step=step, parent=parent.get(e), values=dict(zip(HP_KEYS, map(float, vals)))))
        pbt_file.flush()

    files = [open(os.path.join(d, "curve.csv"), "w") for d in dirs]
    try:
        extra = "" if n_eval is None else ",evaluator_mean,evaluator_min,evaluator_max"
        for f, pt in zip(files, points()):
            f.write(f"step,episodes_closed,mean_episodic_reward,mean_episode_length,evaluator_score{extra}\n")
            f.write(f"0,0,,,{pt}\n")
        for k in range(1, conf.total_time_steps + 1):
            vt.step()
            _keep_tick(vt, args, k, conf.total_time_steps)  # (before a PBT generation at the same step: the experiment's own actors)
            if k % args.report_every == 0 or k == conf.total_time_steps:
                r, ln, n = vt.env.pop_episode_stats(per_experiment=True)
                for e, (f, pt) in enumerate(zip(files, points())):
                    f.write(f"{k},{int(n[e])},{float(r[e]):.5f},{float(ln[e]):.2f},{pt}\n")
                    f.flush()
            if use_pbt and k % args.pbt == 0 and k != conf.total_time_steps:
                generation(k // args.pbt, k)
    finally:
        for f in files:
            f.close()
        if pbt_file is not None:
            pbt_file.close()
    if vt.nonfinite_updates():
        print(f"warning: {vt.nonfinite_updates()} weight-set updates were skipped for non-finite gradients", file=sys.stderr)
    sims = vt.run_simulations()  # [E][P], one rollout launch
    suite = None  # [E, P, scen, (dist,) seed, ...], one launch
    if args.scenarios is not None:
        suite = vt.evaluate_scenarios(**_suite(args)) if _disturb(args) is None else vt.evaluate_robustness(disturbances=_disturb(args), **_suite(args))
    baselines = _baselines(conf, args) if suite is not None and _baseline_flags(args) is not None else None  # computed once
    freq = None if _freq(args) is None else _frequency(conf, args).actors(vt)  # [E, P, F, dist, seed, ...], one launch
    n_save = min(P, 4 if args.save_platoons is None else args.save_platoons)
    kept = _KeepResults(vt, args) if getattr(args, "keep_best", None) is not None else None
    done = []
    for e, (k, d) in enumerate(zip(seeds, dirs)):
        artifacts.save_agents(d, vt.experiment_agents(e), n_save, vt.M, shared=vt.shared)
        ce = vt.experiment_conf(e)  # (its seed; in a sweep also its values, in the reference's fields)
        ce.pl_rews_for_simulations = sims[e]
        ce.pl_rew_for_simulation = float(np.average(sims[e]))
        ce.saved_platoons = int(n_save)
        ce.episodes_mode = "platoon"
        ce.episode_clock = ("per-platoon episodes on the device; schedule predicates on step // steps_per_episode; weighted averaging "
                            "(if enabled) from step weighted_window x steps_per_episode on, weights from each agent's last "
                            "weighted_window closed episodes")
        if experiments is None:
            ce.seed_batch = seeds
        else:
            ce.seed_batch = list(dict.fromkeys(seeds))
            ce.sweep = [[n, list(v)] for n, v in args.sweep]  # the grid in flag order (a list: conf.json keeps lists, not dicts)
            if use_pbt:  # (lists of pairs, as `sweep`: conf.json keeps lists, not dicts, at the top level)
                ce.pbt = [["interval", args.pbt], ["fraction", args.pbt_fraction], ["perturb", list(args.pbt_perturb)],
                          ["lineage", lineage[e]]]
        _record_train_levels(ce, args)
        _record_train_leader(ce, args)
        _record_residual(ce, args)
        _record_warm(ce, args, e)
        _record_anchor(ce, args, vt, e)
        _record_noise(ce, args)
        _record_delay(ce, args)
        if suite is not None:
            _write_suite(d, ce, _slice(suite, e), range(1, P + 1), args)
            if baselines is not None:
                baselines.write(d, ce, _slice(suite, e))
        if freq is not None:
            _frequency(conf, args).write(d, ce, _freq_slice(freq, e), range(1, P + 1))
        if kept is not None:  # (after everything else the directory's conf.json records: best/conf.json carries it too)
            kept.write(d, ce, n_save, e)
        artifacts.config_writer(os.path.join(d, "conf.json"), ce)
        done.append((ce, last[e]))
    return done


if __name__ == "__main__":
    main()
