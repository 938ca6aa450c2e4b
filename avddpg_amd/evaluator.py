"""Evaluator rollout over the HIP kernels: the compute part of reference ``workers/evaluator.py:16-158``
(deterministic-start, noise-free rollout of trained actors; returns the mean episodic reward rounded to 3
digits, :145, :158). Figures / LaTeX are out of scope of the hot path; the traces they were drawn from are returned."""
import ctypes as C

import numpy as np
import torch

from . import vec
from ._hip import call, ptr, stream_handle


def get_number_of_timesteps_for_plot(conf, manual_timestep_override=None):
    return conf.steps_per_episode if manual_timestep_override is None else manual_timestep_override


def _start(conf, seed=True, manual_timestep_override=None, evaluation_seed=None):
    """The rollout's prelude (:44-60): seed the global legacy RNG with ``conf.evaluation_seed`` (or ``evaluation_seed``), the
    evaluator platoon's constructor draws, the T leader-input draws, then reset(). Returns (env, float32 inputs [T], T);
    env.x / env.prev_a hold the start state."""
    if seed:
        np.random.seed(conf.evaluation_seed if evaluation_seed is None else evaluation_seed)  # rand.set_global_seed (src/rand.py:10)
    env = vec.VecPlatoon(1, conf.pl_size, conf, evaluator_states_enabled=True, rng="host", track_aux=True)  # evaluator.py:47
    steps = get_number_of_timesteps_for_plot(conf, manual_timestep_override)
    rand = (lambda: np.random.uniform(-conf.reset_max_u, conf.reset_max_u)) if conf.rand_gen == conf.uniform else \
        (lambda: np.random.normal(0, conf.reset_max_u))
    inputs = np.array([rand() for _ in range(steps)], dtype=np.float32)  # :55-56
    env.reset()
    return env, inputs, steps


def run(conf=None, actors=None, pl_idx=None, seed=True, manual_timestep_override=None, set_mod=None, **_ignored):
    """actors: an ``AgentGroup`` whose first ``pl_size`` weight sets are the platoon's vehicle actors (or whose
    sets are addressed with ``set_mod``). Host-RNG parity mode: the global legacy RNG is seeded with
    ``conf.evaluation_seed`` and consumed in the reference's order. Returns (pl_rew, traces)."""
    env, inputs, steps = _start(conf, seed, manual_timestep_override)
    L = conf.pl_size
    d_inputs = torch.from_numpy(inputs).to(env.device)
    M, A = env.num_models, env.num_actions  # centralized: one model with L actions and a 4L-wide observation (:48, :58)
    xs = 4 * L // M
    counters = torch.zeros(M, dtype=torch.float32, device=env.device)  # float32 counters (:67)
    act = torch.zeros(1, L, dtype=torch.float32, device=env.device)
    raw = torch.zeros(M * A, dtype=torch.float32, device=env.device)
    sm = M if set_mod is None else set_mod
    states = torch.zeros(steps, L, env.obs_width, device=env.device)
    ctrl = torch.zeros(steps, L, device=env.device)
    jerks = torch.zeros(steps, L, device=env.device)
    for i in range(steps):
        actors.actor(env.x.view(M, xs), sm, x_stride=xs, out=raw)
        call("avd_policy_f32", L, ptr(raw), None, conf.action_low, conf.action_high, ptr(act), stream_handle())  # no noise
        pa_before = env.prev_a.clone()
        env.step(act, d_inputs[i:i + 1])
        counters += env.reward[0] if M == L else env.reward_mean
        states[i] = env.observations()[0]
        ctrl[i] = act[0]
        jerks[i] = env.get_jerk_from(env.x_prev, pa_before)[0]
    pl_rew = round(np.average(counters.cpu().numpy()), 3)  # np.float32 rounded in float32, as the reference (:145)
    return pl_rew, dict(states=states.cpu().numpy(), inputs=ctrl.cpu().numpy(), jerks=jerks.cpu().numpy(),
                        counters=counters.cpu().numpy(), leader=inputs)


def _base_gains(base_law, conf, dev):
    """A residual policy's law (scenarios.ResidualLaw) checked and on the device: (gains float32 [L, 4], scale) -- or (None, None)."""
    if base_law is None:
        return None, None
    from . import scenarios as _sc

    _sc.check_residual(base_law, conf)
    return torch.from_numpy(base_law.gains(conf.pl_size)).to(dev), float(base_law.scale)


def _starts(conf, seeds, manual_timestep_override):
    """``_start`` for every evaluation seed, the caller's global ``np.random`` state restored."""
    saved = np.random.get_state()
    try:
        return [_start(conf, True, manual_timestep_override, evaluation_seed=sd) for sd in seeds]
    finally:
        np.random.set_state(saved)


def _address_sets(who, actors, env, platoons, set_mod, set_bases):
    """The weight sets ``platoons`` / ``set_mod`` / ``set_bases`` address in ``actors`` (run_many's docstring), checked. -> (shared,
    per_entry, bases): shared sets or per-agent ones; one result per entry of ``platoons`` (per-agent sets, or shared sets with
    set_bases) or ONE for all of them (shared sets: every platoon's result is the same); the first set of each result."""
    M, lay = env.num_models, actors.lay
    if (lay.S, lay.A) != (env.num_states, env.num_actions):
        raise ValueError(f"actors have S={lay.S} A={lay.A}, the platoon needs S={env.num_states} A={env.num_actions}")
    shared = set_mod is not None and set_mod != 0
    if shared and set_mod != M:
        raise ValueError(f"set_mod={set_mod}: {who} addresses per-agent sets (None / 0) or shared sets (set_mod = M = {M})")
    if not shared and min(platoons) < 0:
        raise ValueError("negative platoon index")
    if set_bases is not None:
        set_bases = [int(b) for b in set_bases]
        if not shared or len(set_bases) != len(platoons) or min(set_bases) < 0:
            raise ValueError(f"set_bases={set_bases}: shared sets only (set_mod = M), one non-negative base per platoon entry")
    need = (M + (max(set_bases) if set_bases else 0)) if shared else (max(platoons) + 1) * M
    if need > actors.n_sets:
        raise ValueError(f"platoons {platoons} need {need} weight sets, the group holds {actors.n_sets}")
    per_entry = not shared or set_bases is not None
    return shared, per_entry, [0] if not per_entry else (set_bases if shared else [p * M for p in platoons])


class RolloutBatch:
    """The device inputs of one avd_eval_rollout_f32 launch (prepare_many); ``launch()`` enqueues it on the current stream,
    ``results()`` reads the counters and traces back. run_many = prepare_many + launch + results."""

    def __init__(self, conf, actors, platoons, set_mod, seeds, manual_timestep_override, trace, set_bases=None, base_law=None):
        platoons = [int(p) for p in platoons]
        seeds = [int(conf.evaluation_seed)] if seeds is None else [int(s) for s in seeds]
        if not platoons or not seeds:
            raise ValueError("run_many needs at least one platoon and one seed")
        NP, NS = len(platoons), len(seeds)
        starts = _starts(conf, seeds, manual_timestep_override)
        env, _, T = starts[0]
        L, M = conf.pl_size, env.num_models
        # rollouts: one per (result, seed)
        _, per_entry, bases = _address_sets("run_many", actors, env, platoons, set_mod, set_bases)
        self.roll = (lambda i, k: i * NS + k) if per_entry else (lambda i, k: k)
        self.n_roll = NP * NS if per_entry else NS
        want = []
        for t in trace:
            i, k = (int(t), 0) if np.isscalar(t) else (int(t[0]), int(t[1]))
            if not (0 <= i < NP and 0 <= k < NS):
                raise IndexError(f"trace entry {t} outside the [{NP}, {NS}] result")
            want.append((i, k))
        self.want, self.tr_roll = want, sorted({self.roll(i, k) for i, k in want})
        dev, nt = env.device, len(self.tr_roll)
        i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
        self.conf, self.actors, self.env, self.T, self.L, self.M, self.NP, self.NS = conf, actors, env, T, L, M, NP, NS
        self.leader_h = [inp for _, inp, _ in starts]
        self.x0 = torch.stack([e.x.reshape(L, 4) for e, _, _ in starts]).contiguous()
        self.pa0 = torch.stack([e.prev_a.reshape(L) for e, _, _ in starts]).contiguous()
        self.leader = torch.from_numpy(np.stack(self.leader_h)).to(dev)
        self.set_base = torch.tensor([b for b in bases for _ in seeds], **i32)
        self.start_idx = torch.tensor(list(range(NS)) * (NP if per_entry else 1), **i32)
        if self.set_base.numel() != self.n_roll or self.start_idx.numel() != self.n_roll:  # (the kernel reads both per rollout)
            raise AssertionError(f"rollout tables of {self.set_base.numel()} / {self.start_idx.numel()} entries for {self.n_roll} rollouts")
        self.counters = torch.empty(self.n_roll, M, **f32)
        self.tr_idx = torch.tensor(self.tr_roll, **i32) if nt else None
        self.tr_s = torch.empty(nt, T, L, env.obs_width, **f32) if nt else None
        self.tr_a = torch.empty(nt, T, L, **f32) if nt else None
        self.tr_j = torch.empty(nt, T, L, **f32) if nt else None
        self.gains, self.res_scale = _base_gains(base_law, conf, dev)

    def launch(self):
        a, c = self.actors, self.conf
        res = () if self.gains is None else (ptr(self.gains), self.res_scale)  # a residual policy: the law in front of the plant
        call("avd_eval_rollout_res_f32" if res else "avd_eval_rollout_f32", a._layp, ptr(self.env.d_consts), self.n_roll, self.L, self.M,
             self.T, ptr(a.theta), ptr(a.stats), a.n_sets, ptr(self.set_base), ptr(self.x0), ptr(self.pa0), ptr(self.leader), self.NS,
             ptr(self.start_idx), a.high, c.action_low, c.action_high, c.sample_rate, ptr(self.counters), len(self.tr_roll),
             ptr(self.tr_idx), ptr(self.tr_s), ptr(self.tr_a), ptr(self.tr_j), *res, stream_handle())

    def results(self):
        c = self.counters.cpu().numpy()
        rows = np.array([round(np.average(c[j]), 3) for j in range(self.n_roll)], dtype=np.float32)  # row by row, as run (:145)
        sel = np.array([[self.roll(i, k) for k in range(self.NS)] for i in range(self.NP)])
        scores, cnt = rows[sel], c[sel]
        traces = {}
        if self.tr_roll:
            hs, ha, hj = self.tr_s.cpu().numpy(), self.tr_a.cpu().numpy(), self.tr_j.cpu().numpy()
            for i, k in self.want:
                j = self.tr_roll.index(self.roll(i, k))
                traces[(i, k)] = dict(states=hs[j], inputs=ha[j], jerks=hj[j], counters=cnt[i, k].copy(), leader=self.leader_h[k])
        return scores, cnt, traces


def prepare_many(conf, actors, platoons, set_mod=None, seeds=None, manual_timestep_override=None, trace=(), set_bases=None, base_law=None):
    """run_many's host part (start states and leader inputs drawn, device inputs uploaded) as a RolloutBatch."""
    return RolloutBatch(conf, actors, platoons, set_mod, seeds, manual_timestep_override, trace, set_bases, base_law)


def run_many(conf, actors, platoons, set_mod=None, seeds=None, manual_timestep_override=None, trace=(), set_bases=None, base_law=None):
    """The rollout of ``run`` for many platoons' actors and evaluation seeds at once: ONE launch of the evaluator rollout
    kernel (avd_eval_rollout_f32, csrc/eval.hip), one workgroup per (platoon, seed). What Trainer.run_simulations
    (workers/trainer.py:537-550) and esim (run.py:60-70) do platoon by platoon.

    actors: an ``AgentGroup``. set_mod None (or 0): per-agent sets -- platoon p's M models are sets p*M .. p*M+M-1;
    set_mod = M: shared sets -- every platoon uses sets 0 .. M-1 (its rollouts are then computed once per seed); with
    set_bases (one per entry of ``platoons``) entry i uses sets set_bases[i] .. set_bases[i]+M-1 instead -- e.g. experiment e's sets
    e*M .. of a seed batch (trainer.VecTrainer(seeds=...)).
    seeds: evaluation seeds (default ``(conf.evaluation_seed,)``); each one's start state and leader inputs are drawn on the
    host exactly as ``run`` draws them, and the caller's global ``np.random`` state is restored on return.
    trace: (i, k) index pairs into the result (or plain i for k = 0) whose per-step traces are returned.
    base_law: a scenarios.ResidualLaw the actors correct (avd_eval_rollout_res_f32): the plant input, and the ``inputs`` trace, is
    clip(law(state) + scale * the actors' action). None: the actors alone, today's entry point with today's arguments.

    Returns (scores, counters, traces): scores float32 [len(platoons), len(seeds)] (round(mean(counters), 3), :145),
    counters float32 [len(platoons), len(seeds), M], traces {(i, k): dict like run's}. Entry [i, k] is bit-identical to
    ``run`` with ``evaluation_seed = seeds[k]`` on platoon ``platoons[i]``'s sets."""
    b = prepare_many(conf, actors, platoons, set_mod, seeds, manual_timestep_override, trace, set_bases, base_law)
    b.launch()
    return b.results()


class CaseResults:
    """What run_cases returns: ``scores`` float32 [NP, n_scen, n_seed] (round(mean(counters), 3), :145), ``counters`` float32
    [NP, n_scen, n_seed, M], ``metrics`` {name: float32 [NP, n_scen, n_seed, L]} (scenarios.METRICS), ``summary()`` the derived
    values (scenarios.summarise); ``scenarios`` / ``seeds`` name the two case axes, ``T`` is the rollout length."""

    def __init__(self, scenarios, seeds, T, scores, counters, metrics):
        self.scenarios, self.seeds, self.T = list(scenarios), list(seeds), int(T)
        self.scores, self.counters, self.metrics = scores, counters, metrics

    def summary(self):
        from . import scenarios as _sc

        return _sc.summarise(self.metrics, self.T)


def _level_tables(conf, levels, seeds, NC, L):
    """The per-case disturbance tables of scenarios x levels x seeds (seeds innermost) on the host: (sigma float32 [K, 3], delay int32
    [K], drop_q uint32 [K], noise_seed uint64 [K], abc float32 [K, L, 24] or None when no level changes the plant), checked by
    avd_eval_cases_dist_check. The noise seed is the case's evaluation seed: every level of a seed shares its draws."""
    from . import _hip
    from . import scenarios as _sc

    ND, NS = len(levels), len(seeds)
    lvl = np.tile(np.repeat(np.arange(ND), NS), NC)  # a case's level
    sigma = np.array([d.sigma for d in levels], dtype=np.float32)[lvl]
    delay = np.array([int(d.v2v_delay) for d in levels], dtype=np.int32)[lvl]
    drop_q = np.array([_sc.drop_threshold(d.v2v_drop) for d in levels], dtype=np.uint32)[lvl]
    noise_seed = np.tile(np.array(seeds, dtype=np.uint64), NC * ND)
    _hip.call("avd_eval_cases_dist_check", NC * ND * NS, sigma.ctypes.data, delay.ctypes.data, drop_q.ctypes.data)
    abc = None
    if any(d.dyn_coeff is not None for d in levels):
        abc = np.stack([_sc.plant_table(conf, L, d.dyn_coeff) for d in levels])[lvl]  # [K, L, 24]
    return sigma, delay, drop_q, noise_seed, abc


def _upload(a, dev, as_type=None):
    """A host table on the device (torch holds signed integers: unsigned tables go up as their signed views)."""
    return torch.from_numpy(a if as_type is None else a.view(as_type)).to(dev)


class _Suite:
    """The cases of a scenario suite, built once for whichever batch runs them: scenarios x seeds -- with ``levels`` (Disturbances,
    scenarios.NOMINAL first) scenarios x levels x seeds -- seeds innermost. A case's start state is its seed's, drawn as ``run`` draws
    it and always the nominal configuration's; its leader row is its scenario's (gaussian: its seed's). Fields: ``scenarios``,
    ``seeds``, ``levels`` (or None), the counts ``NC``, ``ND`` (None without levels), ``NS``, ``K`` cases, ``T`` steps, ``L``, ``env``;
    ``leader_h`` float32 [K, T] on the host; on the device ``leader``, ``x0`` [K, L, 4], ``pa0`` [K, L] and the level tables ``sigma``,
    ``delay``, ``drop_q``, ``noise_seed``, ``abc`` of _level_tables (all None without levels; abc None when no level changes the plant: the
    constants block's matrices for every case), ``sigma_h`` ... their host copies."""

    def __init__(self, conf, scenarios, levels, seeds, amp, period_s, manual_timestep_override, no_seed, rows=None):
        from . import scenarios as _sc

        if rows is not None:  # explicit leader rows float32 [NC, T] named by ``scenarios`` (a frequency sweep's): T is theirs
            rows = np.ascontiguousarray(np.asarray(rows, dtype=np.float32))
            names = [str(n) for n in scenarios]
            if rows.ndim != 2 or rows.shape[0] != len(names) or not names or not np.isfinite(rows).all():
                raise ValueError(f"leader rows of shape {rows.shape} for {len(names)} names: need finite [NC >= 1, T]")
            manual_timestep_override = rows.shape[1]
        else:
            names = _sc.check_names(scenarios)
        seeds = [int(conf.evaluation_seed)] if seeds is None else [int(s) for s in seeds]
        if not seeds:
            raise ValueError(no_seed)
        if len(set(seeds)) != len(seeds):
            raise ValueError(f"seeds {seeds}: a seed is listed more than once")
        T = get_number_of_timesteps_for_plot(conf, manual_timestep_override)
        amp, period_s = _sc.check_knobs(T, amp, period_s)
        starts = _starts(conf, seeds, manual_timestep_override)
        env = starts[0][0]
        dev, L, NC, NS = env.device, conf.pl_size, len(names), len(seeds)
        rep = 1 if levels is None else len(levels)  # a (scenario, seed)'s cases
        self.scenarios, self.seeds, self.levels, self.env = names, seeds, levels, env
        self.L, self.T, self.NC, self.ND, self.NS, self.K = L, T, NC, (None if levels is None else rep), NS, NC * rep * NS
        if rows is not None:
            self.leader_h = np.repeat(rows, rep * NS, axis=0)
        else:
            prof = {n: _sc.leader_profile(n, T, conf, amp, period_s) for n in names if n != "gaussian"}
            self.leader_h = np.stack([starts[k][1] if n == "gaussian" else prof[n] for n in names for _ in range(rep) for k in range(NS)])
        self.leader = torch.from_numpy(self.leader_h).to(dev)
        self.x0 = torch.stack([e.x.reshape(L, 4) for e, _, _ in starts]).repeat(NC * rep, 1, 1).contiguous()
        self.pa0 = torch.stack([e.prev_a.reshape(L) for e, _, _ in starts]).repeat(NC * rep, 1).contiguous()
        self.sigma_h = self.delay_h = self.drop_q_h = self.noise_seed_h = self.abc_h = None
        self.sigma = self.delay = self.drop_q = self.noise_seed = self.abc = None
        if levels is not None:  # host-checked: the kernels read them from device memory
            self.sigma_h, self.delay_h, self.drop_q_h, self.noise_seed_h, self.abc_h = _level_tables(conf, levels, seeds, NC, L)
            self.sigma, self.delay = _upload(self.sigma_h, dev), _upload(self.delay_h, dev)
            self.drop_q, self.noise_seed = _upload(self.drop_q_h, dev, np.int32), _upload(self.noise_seed_h, dev, np.int64)
            self.abc = None if self.abc_h is None else _upload(self.abc_h, dev)

    def outputs(self, G, width, metrics=True):
        """-> (counters [G, K, width], metrics [G, K, L, AVD_EVAL_NMETRIC] or None) for G groups, uninitialised, on the device."""
        from . import _hip

        f32 = dict(dtype=torch.float32, device=self.env.device)
        return torch.empty(G, self.K, width, **f32), (torch.empty(G, self.K, self.L, _hip.AVD_EVAL_NMETRIC, **f32) if metrics else None)


def _case_results(b, sel=slice(None)):
    """A launched case batch's read-back: counters -> scores rounded row by row, as run (:145) -> the groups ``sel`` -> the metric dict
    -> a CaseResults, or with levels a DisturbedResults."""
    from . import scenarios as _sc

    W = b.counters.shape[-1]
    c = b.counters.cpu().numpy().reshape(b.G * b.K, W)
    rows = np.array([round(np.average(r), 3) for r in c], dtype=np.float32)
    shape = (b.G, b.NC, b.NS) if b.levels is None else (b.G, b.NC, b.ND, b.NS)
    m = b.metrics.cpu().numpy().reshape(*shape, b.L, -1)[sel]
    metrics = {n: np.ascontiguousarray(m[..., j]) for j, n in enumerate(_sc.METRICS)}
    scores, cnt = rows.reshape(shape)[sel], c.reshape(*shape, W)[sel]
    if b.levels is None:
        return CaseResults(b.scenarios, b.seeds, b.T, scores, cnt, metrics)
    return DisturbedResults(b.scenarios, [d.name for d in b.levels], b.seeds, b.T, scores, cnt, metrics)


class CaseBatch:
    """The device inputs of one avd_eval_cases_f32 launch (prepare_cases); ``launch()`` enqueues it on the current stream,
    ``results()`` reads counters and metrics back. run_cases = prepare_cases + launch + results. ``block`` is the number of cases per
    workgroup the kernel uses for this batch (avd_eval_cases_block; with ``levels``, DisturbedBatch's, avd_eval_cases_dist_block). The
    cases and their tables are a _Suite's fields."""

    def __init__(self, conf, actors, platoons, scenarios, seeds, amp, period_s, set_mod, set_bases, manual_timestep_override, base_law=None,
                 levels=None, rows=None):
        from . import _hip

        platoons = [int(p) for p in platoons]
        no_entry = "run_cases needs at least one platoon and one seed"
        if not platoons:
            raise ValueError(no_entry)
        suite = _Suite(conf, scenarios, levels, seeds, amp, period_s, manual_timestep_override, no_entry, rows)
        vars(self).update(vars(suite))
        # groups: ONE result for all platoons, or one per entry (_address_sets)
        _, per_entry, bases = _address_sets("run_cases", actors, self.env, platoons, set_mod, set_bases)
        self.group = (lambda i: i) if per_entry else (lambda i: 0)
        self.conf, self.actors, self.M, self.NP, self.G = conf, actors, self.env.num_models, len(platoons), len(bases)
        self.set_base = torch.tensor(bases, dtype=torch.int32, device=self.env.device)
        self.counters, self.metrics = suite.outputs(self.G, self.M)
        self.block = int((_hip.lib().avd_eval_cases_block if levels is None else _hip.lib().avd_eval_cases_dist_block)(self.K, self.L))
        self.gains, self.res_scale = _base_gains(base_law, conf, self.env.device)

    def _args(self):
        """-> (common, tables, out): the argument groups every cases entry point shares."""
        a, c = self.actors, self.conf
        common = (a._layp, ptr(self.env.d_consts), self.G, self.K, self.L, self.M, self.T, ptr(a.theta), ptr(a.stats), a.n_sets,
                  ptr(self.set_base), ptr(self.x0), ptr(self.pa0), ptr(self.leader), a.high, c.action_low, c.action_high, c.sample_rate)
        tables = (ptr(self.sigma), ptr(self.delay), ptr(self.drop_q), ptr(self.noise_seed), ptr(self.abc))  # null without levels
        return common, tables, (ptr(self.counters), ptr(self.metrics), stream_handle())

    def launch(self):
        common, tables, out = self._args()
        if self.gains is not None:  # a residual policy: the law acts on what the vehicle observes
            call("avd_eval_cases_res_f32", *common, *tables, ptr(self.gains), self.res_scale, *out)
        elif self.levels is not None:
            call("avd_eval_cases_dist_f32", *common, *tables, *out)
        else:
            call("avd_eval_cases_f32", *common, *out)

    def results(self):
        return _case_results(self, [self.group(i) for i in range(self.NP)])




def prepare_cases(conf, actors, platoons, scenarios=("gaussian",), seeds=None, amp=None, period_s=10.0, set_mod=None, set_bases=None,
                  manual_timestep_override=None, base_law=None):
    """run_cases' host part (start states drawn, leader profiles made, device inputs uploaded) as a CaseBatch."""
    return CaseBatch(conf, actors, platoons, scenarios, seeds, amp, period_s, set_mod, set_bases, manual_timestep_override, base_law)


def run_cases(conf, actors, platoons, scenarios=("gaussian",), seeds=None, amp=None, period_s=10.0, set_mod=None, set_bases=None,
              manual_timestep_override=None, base_law=None):
    """Every platoon's actors over a library of leader scenarios x evaluation seeds in ONE launch of the scenario evaluator
    (avd_eval_cases_f32, csrc/evalx.hip): one workgroup per (platoon, block of cases), each weight element read once per block, the
    per-vehicle control metrics reduced on the device. The reference's evaluator names these input responses and fills in only the
    Gaussian one (workers/evaluator.py:55-70).

    scenarios: names of scenarios.SCENARIOS (leader_profile; amp defaults to conf.reset_max_u, period_s is the sine's period).
    seeds: evaluation seeds (default ``(conf.evaluation_seed,)``). Cases are scenarios x seeds, seeds innermost; a case's start state
    is drawn as ``run`` draws it for its seed, and only the gaussian scenario's leader inputs depend on the seed. The caller's global
    ``np.random`` state is restored on return. actors / platoons / set_mod / set_bases address weight sets as in ``run_many``.
    base_law: a scenarios.ResidualLaw the actors correct (avd_eval_cases_res_f32), as in ``run_many``; sum_u2 is then the plant input's.

    Returns a CaseResults. Entry [i, s, k] of its counters is bit-identical to the rollout kernel's (run_many) on the same start state
    and leader row -- for the gaussian scenario, to ``run_many(seeds=seeds)[1][i, k]`` -- and its metrics to
    scenarios.metrics_from_traces on that rollout's traces."""
    b = prepare_cases(conf, actors, platoons, scenarios, seeds, amp, period_s, set_mod, set_bases, manual_timestep_override, base_law)
    b.launch()
    return b.results()


class DisturbedResults:
    """What run_disturbed returns: CaseResults' fields with a disturbance axis after the scenario axis -- ``scores`` float32 [NP, n_scen,
    n_dist + 1, n_seed], ``counters`` [..., M], ``metrics`` {name: [..., L]}, ``summary()`` -- and ``disturbances``, the levels' names
    with "nominal" first. ``nominal()`` is the undisturbed level as a plain CaseResults."""

    def __init__(self, scenarios, disturbances, seeds, T, scores, counters, metrics):
        self.scenarios, self.disturbances, self.seeds, self.T = list(scenarios), list(disturbances), list(seeds), int(T)
        self.scores, self.counters, self.metrics = scores, counters, metrics

    def summary(self):
        from . import scenarios as _sc

        return _sc.summarise(self.metrics, self.T)

    def nominal(self):
        return CaseResults(self.scenarios, self.seeds, self.T, self.scores[:, :, 0], self.counters[:, :, 0],
                           {k: v[:, :, 0] for k, v in self.metrics.items()})


class DisturbedBatch(CaseBatch):
    """The device inputs of one avd_eval_cases_dist_f32 launch (prepare_disturbed): CaseBatch with ``levels`` -- a disturbance axis
    between scenario and seed, and the per-case disturbance tables. ``levels`` are the Disturbances, scenarios.NOMINAL first."""

    def __init__(self, conf, actors, platoons, scenarios, disturbances, seeds, amp, period_s, set_mod, set_bases, manual_timestep_override,
                 base_law=None):
        from . import scenarios as _sc

        levels = [_sc.NOMINAL] + _sc.check_disturbances(disturbances, conf)
        super().__init__(conf, actors, platoons, scenarios, seeds, amp, period_s, set_mod, set_bases, manual_timestep_override, base_law, levels)


def prepare_disturbed(conf, actors, platoons, scenarios=("gaussian",), disturbances=(), seeds=None, amp=None, period_s=10.0, set_mod=None,
                      set_bases=None, manual_timestep_override=None, base_law=None):
    """run_disturbed's host part (run_cases' plus the per-case disturbance tables, checked and uploaded) as a DisturbedBatch."""
    return DisturbedBatch(conf, actors, platoons, scenarios, disturbances, seeds, amp, period_s, set_mod, set_bases, manual_timestep_override,
                          base_law)


def run_disturbed(conf, actors, platoons, scenarios=("gaussian",), disturbances=(), seeds=None, amp=None, period_s=10.0, set_mod=None,
                  set_bases=None, manual_timestep_override=None, base_law=None):
    """run_cases under disturbances: every platoon's actors over scenarios x [nominal, *disturbances] x seeds (seeds innermost) in ONE
    launch of the disturbed scenario evaluator (avd_eval_cases_dist_f32, csrc/evalx.hip). A scenarios.Disturbance acts on what the
    actors observe (sensor noise on ep, ev, a; delay and loss on the communicated 4th state) and on the plant (its engine lag); counters
    and metrics come from the true state, and start states are always the nominal configuration's. The noise seed of a case is its
    evaluation seed. Everything else is as in run_cases; with base_law the law reads the vehicle's OBSERVATION.

    Returns a DisturbedResults; its ``nominal()`` slice, and every level whose axes are all at their zero, is bit-identical to
    run_cases on the same scenarios and seeds."""
    b = prepare_disturbed(conf, actors, platoons, scenarios, disturbances, seeds, amp, period_s, set_mod, set_bases, manual_timestep_override,
                          base_law)
    b.launch()
    return b.results()


class LinearBatch:
    """The device inputs of one avd_eval_linear_f32 launch (prepare_linear, tune_linear): G gain sets ``gains`` float32 [G, L, 4] over the
    cases of CaseBatch (no disturbances) or DisturbedBatch: the same _Suite. ``launch()`` enqueues it on the current stream, ``results()`` reads counters and metrics back (first axis: the gain
    sets). ``metrics=False`` passes the kernel a null metrics pointer. The raw form: under Model A the kernel does not read a row's 4th
    gain (prepare_linear and tune_linear refuse a non-zero one)."""

    def __init__(self, conf, gains, scenarios, disturbances, seeds, amp, period_s, manual_timestep_override, metrics=True, rows=None):
        from . import scenarios as _sc

        if conf.framework == conf.cntrl:
            raise ValueError("a linear baseline is a per-vehicle law: not available for the centralized framework")
        disturbances = list(disturbances)
        levels = [_sc.NOMINAL] + _sc.check_disturbances(disturbances, conf) if disturbances else None
        gains = np.ascontiguousarray(np.asarray(gains, dtype=np.float32))
        if gains.ndim != 3 or gains.shape[0] < 1 or gains.shape[1:] != (conf.pl_size, 4) or not np.isfinite(gains).all():
            raise ValueError(f"gains of shape {gains.shape}: need finite [G >= 1, L = {conf.pl_size}, 4]")
        suite = _Suite(conf, scenarios, levels, seeds, amp, period_s, manual_timestep_override, "run_linear needs at least one seed", rows)
        vars(self).update(vars(suite))
        self.conf, self.G = conf, gains.shape[0]
        self.gains_h, self.gains = gains, torch.from_numpy(gains).to(self.env.device)
        self.counters, self.metrics = suite.outputs(self.G, self.L, metrics)

    def _args(self):
        c = self.conf
        return (ptr(self.env.d_consts), self.G, self.K, self.L, self.T, ptr(self.gains), ptr(self.x0), ptr(self.pa0), ptr(self.leader),
                c.action_low, c.action_high, c.sample_rate, ptr(self.sigma), ptr(self.delay), ptr(self.drop_q), ptr(self.noise_seed),
                ptr(self.abc), ptr(self.counters), ptr(self.metrics))

    def launch(self):
        call("avd_eval_linear_f32", *self._args(), stream_handle())

    def enqueue_fitness(self, out=None):
        """One avd_linear_fitness_f32 launch over the counters of ``launch()`` on the current stream, into ``out`` (float32 [G] on the
        device; allocated when None). Nothing is read back."""
        if out is None:
            out = torch.empty(self.G, dtype=torch.float32, device=self.counters.device)
        call("avd_linear_fitness_f32", self.G, self.K, self.L, ptr(self.counters), ptr(out), stream_handle())
        return out

    def fitness(self):
        """One avd_linear_fitness_f32 launch over the counters of ``launch()``: float32 [G] on the host (the only read-back)."""
        return self.enqueue_fitness().cpu().numpy()

    def results(self):
        if self.metrics is None:
            raise ValueError("this batch was prepared without metrics (tune_linear): read fitness()")
        return _case_results(self)


def prepare_linear(conf, laws, scenarios=("gaussian",), disturbances=(), seeds=None, amp=None, period_s=10.0, manual_timestep_override=None):
    """run_linear's host part (laws checked, cases built as run_cases / run_disturbed build them, device inputs uploaded) as a
    LinearBatch."""
    from . import scenarios as _sc

    laws = _sc.check_baselines(laws, conf, reserved=())
    if not laws:
        raise ValueError("run_linear needs at least one law")
    gains = np.stack([b.gains(conf.pl_size) for b in laws])
    b = LinearBatch(conf, gains, scenarios, disturbances, seeds, amp, period_s, manual_timestep_override)
    b.laws = laws
    return b


def run_linear(conf, laws, scenarios=("gaussian",), disturbances=(), seeds=None, amp=None, period_s=10.0, manual_timestep_override=None):
    """Linear baselines over the scenario suite: every scenarios.LinearLaw of ``laws`` over scenarios x [nominal, *disturbances] x seeds
    in ONE launch of the linear scenario evaluator (avd_eval_linear_f32, csrc/lin.hip), one lane per (law, case, vehicle). The cases,
    the observation model, the platoon step, the reward and the metrics are run_cases' / run_disturbed's; only the controller differs: u
    = clip(kp ep + kv ev + ka a + kf a_pred) on the observed state. Decentralized platoons only.

    Returns a CaseResults (no disturbances) or a DisturbedResults whose first axis is the law axis instead of the platoon axis."""
    b = prepare_linear(conf, laws, scenarios, disturbances, seeds, amp, period_s, manual_timestep_override)
    b.launch()
    return b.results()


def tune_linear(conf, grid, scenarios=("gaussian",), disturbances=(), seeds=None, amp=None, period_s=10.0, manual_timestep_override=None):
    """A gain search on the device: every row (kp, kv, ka, kf) of ``grid`` float32 [G, 4] (scenarios.parse_gain_grid) as a homogeneous
    law -- the same row for every vehicle -- over the suite's cases in ONE rollout launch without metrics, then ONE fitness launch
    (avd_linear_fitness_f32: a candidate's mean counter over cases and vehicles, a sequential float32 sum) and a read-back of G floats.
    -> (best_index, fitness float32 [G]): the host's arg-max, the first index among equals, a NaN never wins."""
    from . import scenarios as _sc

    grid = np.asarray(grid, dtype=np.float32)
    if grid.ndim != 2 or grid.shape[1] != 4 or not 1 <= grid.shape[0] <= _sc.MAX_GRID:
        raise ValueError(f"grid of shape {grid.shape}: need [1 .. {_sc.MAX_GRID}, 4]")
    if conf.model == conf.modelA and np.any(grid[:, 3] != 0):
        raise ValueError("a grid over kf needs Model B (Model A observes no communicated state)")
    gains = np.repeat(grid[:, None, :], conf.pl_size, axis=1)
    b = LinearBatch(conf, gains, scenarios, disturbances, seeds, amp, period_s, manual_timestep_override, metrics=False)
    b.launch()
    fit = b.fitness()
    return _sc.first_argmax(fit), fit


class SearchResult:
    """What search_linear returns: ``law`` the best-ever table as a scenarios.LinearLaw (a tied search's row repeated over the vehicles),
    ``fitness`` and ``generation`` of that table, ``history`` float32 [gens, 4] (per generation: the best fitness, the elites' mean
    fitness, the best-ever fitness so far, the number of valid elites), the final ``mean`` / ``std`` float32 [R, 4], ``best_gains``
    float32 [R, 4], the counts ``pop``, ``gens``, ``n_elite``, ``K`` (cases per candidate) and ``trace`` (None, or with trace=True a dict
    of per-generation arrays: gains [gens, G, L, 4], fitness [gens, G], elite_idx [gens, n_elite], mean / std [gens, R, 4] BEFORE the
    generation's refit)."""

    def __init__(self, law, fitness, generation, history, mean, std, best_gains, pop, gens, n_elite, K, trace):
        self.law, self.fitness, self.generation, self.history = law, float(fitness), int(generation), history
        self.mean, self.std, self.best_gains, self.trace = mean, std, best_gains, trace
        self.pop, self.gens, self.n_elite, self.K = int(pop), int(gens), int(n_elite), int(K)

    def record(self, text=None):
        """conf.json's baseline_search entry, a list of pairs (conf.json keeps lists, not dicts)."""
        return [["spec", text], ["pop", self.pop], ["gens", self.gens], ["n_elite", self.n_elite], ["cases", self.K],
                ["table", np.asarray(self.law.table, dtype=np.float64).tolist()], ["fitness", self.fitness], ["generation", self.generation],
                ["history", np.asarray(self.history, dtype=np.float64).tolist()]]


def search_linear(conf, space, scenarios=("gaussian",), disturbances=(), seeds=None, amp=None, period_s=10.0, manual_timestep_override=None,
                  trace=False, name=None):
    """A cross-entropy search over gain tables, resident on the device: ``space`` (scenarios.SearchSpace) gives the bounds per gain, the
    population, the generations and whether every vehicle has its own row (R = L searched rows) or all share one (R = 1). ONE
    LinearBatch of ``pop`` gain sets without metrics is built; per generation four launches are enqueued on the current stream --
    avd_search_sample_f32 writes the batch's gains (candidate 0 is the current mean), avd_eval_linear_f32 rolls them out,
    avd_linear_fitness_f32 reduces the counters, avd_search_refit_f32 ranks the candidates, refits mean and std to the elites and keeps
    the best-ever table -- with the generation number passed by value, and nothing is read back until the last generation is enqueued.
    The fitness is tune_linear's: a candidate's mean counter over the suite's undisturbed cases (``space.over == "nominal"``) or over
    scenarios x [nominal, *disturbances] x seeds (``"all"``). -> a SearchResult; with ``trace`` every generation's candidates, fitness,
    elites and pre-refit distribution are kept (device-to-device copies into slabs, read back at the end)."""
    from . import scenarios as _sc

    space = _sc.check_search(space, conf)
    L, G, gens, n_elite = conf.pl_size, int(space.pop), int(space.gens), space.n_elite()
    R = space.rows(L)
    lo_h, hi_h, mean_h, std_h, min_h = space.tables(L)
    levels = list(disturbances) if space.over == "all" else []
    b = LinearBatch(conf, np.zeros((G, L, 4), dtype=np.float32), scenarios, levels, seeds, amp, period_s, manual_timestep_override,
                    metrics=False)
    dev = b.counters.device
    up = lambda x: torch.from_numpy(x).to(dev)
    lo, hi, mean, std, min_std = up(lo_h), up(hi_h), up(mean_h), up(std_h), up(min_h)
    f32 = dict(dtype=torch.float32, device=dev)
    best_gains, best_fit = torch.zeros(R, 4, **f32), torch.full((1,), -np.inf, **f32)
    best_gen = torch.full((1,), -1, dtype=torch.int32, device=dev)
    fit, history = torch.empty(G, **f32), torch.zeros(gens, 4, **f32)
    elite = torch.zeros(gens if trace else 1, n_elite, dtype=torch.int32, device=dev)
    slab = None
    if trace:
        slab = dict(gains=torch.empty(gens, G, L, 4, **f32), fitness=torch.empty(gens, G, **f32), mean=torch.empty(gens, R, 4, **f32),
                    std=torch.empty(gens, R, 4, **f32))
    seed = int(conf.evaluation_seed if space.seed is None else space.seed)
    row = lambda t, i: C.c_void_p(t.data_ptr() + i * t.stride(0) * t.element_size())
    for gen in range(gens):
        call("avd_search_sample_f32", G, L, R, ptr(mean), ptr(std), ptr(lo), ptr(hi), seed, gen, ptr(b.gains), stream_handle())
        b.launch()
        b.enqueue_fitness(fit)
        if trace:
            slab["gains"][gen].copy_(b.gains), slab["fitness"][gen].copy_(fit), slab["mean"][gen].copy_(mean), slab["std"][gen].copy_(std)
        call("avd_search_refit_f32", G, L, R, n_elite, float(space.alpha), ptr(b.gains), ptr(fit), ptr(min_std), ptr(mean), ptr(std),
             ptr(best_gains), ptr(best_fit), ptr(best_gen), gen, row(elite, gen if trace else 0), row(history, gen), stream_handle())
    at = int(best_gen.cpu()[0])
    if at < 0:
        raise ValueError("search: no candidate of any generation had a finite fitness")
    bg = best_gains.cpu().numpy()
    table = np.ascontiguousarray(np.repeat(bg, L, axis=0) if R == 1 else bg)
    tr = None
    if trace:
        tr = {k: v.cpu().numpy() for k, v in slab.items()}
        tr["elite_idx"] = elite.cpu().numpy()
    return SearchResult(_sc.LinearLaw(_sc.SEARCHED if name is None else name, table=table), best_fit.cpu().numpy()[0], at,
                        history.cpu().numpy(), mean.cpu().numpy(), std.cpu().numpy(), bg, G, gens, n_elite, b.K, tr)


# ---- frequency response: a sweep of sinusoidal leader inputs as cases, a single-bin Fourier sum per vehicle and signal on the device ----

class FrequencyResults:
    """What run_frequency / run_linear_frequency return: ``freqs_hz`` float64 [F] (the frequencies driven) and their ``cycles`` in the
    window of ``W`` steps (of ``T``), ``disturbances`` (the levels' names, "nominal" first), ``seeds``; ``spectrum`` float32 [G, F, ND,
    NS, L, 10] the raw sums (scenarios.SIGNALS), ``summary()`` scenarios.frequency_summary of it, and the usual
    ``scores`` [G, F, ND, NS], ``counters`` [..., M], ``metrics`` {name: [..., L]}. G: the platoon entries, or the laws."""

    def __init__(self, freqs_hz, cycles, W, T, disturbances, seeds, spectrum, scores, counters, metrics):
        self.freqs_hz, self.cycles, self.W, self.T = np.asarray(freqs_hz, dtype=np.float64), np.asarray(cycles), int(W), int(T)
        self.disturbances, self.seeds = list(disturbances), list(seeds)
        self.spectrum, self.scores, self.counters, self.metrics = spectrum, scores, counters, metrics

    def summary(self):
        from . import scenarios as _sc

        return _sc.frequency_summary(self.spectrum, self.W, self.freqs_hz, axis=self.spectrum.ndim - 5)  # [..., F, ND, NS, L, 10]


class _FrequencyMixin:
    """What the two frequency batches share: the sweep's tables before the base class builds its suite, the spectrum output after, and
    the read-back."""

    def _sweep(self, spec, conf, disturbances):
        from . import scenarios as _sc

        spec = _sc.check_frequency(spec, conf)
        self.spec, (_, self.t0, self.W) = spec, spec.window(conf)
        self.cycles, self.freqs_hz = spec.cycles(conf), spec.freqs_hz(conf)
        self._basis_f = _sc.frequency_basis(spec, conf)
        disturbances = list(disturbances)
        levels = [_sc.NOMINAL] + _sc.check_disturbances(disturbances, conf) if disturbances else None
        return [f"f{int(c)}" for c in self.cycles], _sc.frequency_leader(spec, conf), levels

    def _outputs(self):
        from . import _hip

        per = self.K // self.NC  # a frequency's cases: levels x seeds
        self.basis_h = np.repeat(self._basis_f, per, axis=0)  # [K, T, 2]
        self.basis = torch.from_numpy(self.basis_h).to(self.env.device)
        self.spectrum = torch.empty(self.G, self.K, self.L, _hip.AVD_EVAL_NSPEC, dtype=torch.float32, device=self.env.device)

    def _frequency_results(self, sel=slice(None)):
        r = super().results()
        ND = 1 if self.levels is None else self.ND
        G = r.scores.shape[0]
        shape = (G, self.NC, ND, self.NS)
        sp = self.spectrum.cpu().numpy().reshape(self.G, self.NC, ND, self.NS, self.L, -1)[sel]
        names = ["nominal"] if self.levels is None else [d.name for d in self.levels]
        return FrequencyResults(self.freqs_hz, self.cycles, self.W, self.T, names, self.seeds, np.ascontiguousarray(sp),
                                r.scores.reshape(shape), r.counters.reshape(*shape, -1),
                                {k: v.reshape(*shape, self.L) for k, v in r.metrics.items()})


class FrequencyBatch(_FrequencyMixin, CaseBatch):
    """The device inputs of one avd_eval_cases_freq_f32 launch (prepare_frequency): CaseBatch's, the cases a frequency sweep's -- frequencies x
    [nominal, *disturbances] x seeds, seeds innermost -- plus ``basis`` [K, T, 2] and ``spectrum`` [G, K, L, 10]."""

    def __init__(self, conf, actors, platoons, spec, disturbances, seeds, set_mod, set_bases, base_law):
        names, rows, levels = self._sweep(spec, conf, disturbances)
        super().__init__(conf, actors, platoons, names, seeds, None, 10.0, set_mod, set_bases, None, base_law, levels, rows)
        self._outputs()

    def launch(self):
        common, tables, out = self._args()
        call("avd_eval_cases_freq_f32", *common, *tables, ptr(self.gains), self.res_scale if self.gains is not None else 1.0, *out[:2],
             ptr(self.basis), ptr(self.spectrum), out[2])

    def results(self):
        return self._frequency_results([self.group(i) for i in range(self.NP)])


class LinearFrequencyBatch(_FrequencyMixin, LinearBatch):
    """The device inputs of one avd_eval_linear_freq_f32 launch (prepare_linear_frequency): LinearBatch's over a frequency sweep's cases."""

    def __init__(self, conf, gains, spec, disturbances, seeds):
        names, rows, _ = self._sweep(spec, conf, disturbances)
        super().__init__(conf, gains, names, disturbances, seeds, None, 10.0, None, True, rows)
        self._outputs()

    def launch(self):
        call("avd_eval_linear_freq_f32", *self._args(), ptr(self.basis), ptr(self.spectrum), stream_handle())

    def results(self):
        return self._frequency_results()


def prepare_frequency(conf, actors, platoons, spec, disturbances=(), seeds=None, set_mod=None, set_bases=None, base_law=None):
    """run_frequency's host part (the sweep's leader rows and basis table made, start states drawn, device inputs uploaded) as a
    FrequencyBatch."""
    return FrequencyBatch(conf, actors, platoons, spec, disturbances, seeds, set_mod, set_bases, base_law)


def run_frequency(conf, actors, platoons, spec, disturbances=(), seeds=None, set_mod=None, set_bases=None, base_law=None):
    """The frequency response of every platoon's actors in ONE launch of avd_eval_cases_freq_f32 (csrc/evalx.hip): ``spec`` (a
    scenarios.FrequencySpec) gives the sinusoidal leader inputs, one per snapped frequency; the cases are frequencies x [nominal,
    *disturbances] x seeds, seeds innermost, with run_cases' start states; per vehicle the kernel accumulates the single-bin Fourier
    sums of the post-step state and the plant input over the spec's window beside the usual counters and metrics (which are bit-identical
    to run_cases' / run_disturbed's on the same cases). actors / platoons / set_mod / set_bases / base_law as in run_cases. The caller's
    global ``np.random`` state is restored. -> a FrequencyResults; its spectrum is bit-identical to scenarios.spectrum_from_traces on
    the rollout's traces."""
    b = prepare_frequency(conf, actors, platoons, spec, disturbances, seeds, set_mod, set_bases, base_law)
    b.launch()
    return b.results()


def prepare_linear_frequency(conf, laws, spec, disturbances=(), seeds=None):
    """run_linear_frequency's host part as a LinearFrequencyBatch."""
    from . import scenarios as _sc

    laws = _sc.check_baselines(laws, conf, reserved=())
    if not laws:
        raise ValueError("run_linear_frequency needs at least one law")
    b = LinearFrequencyBatch(conf, np.stack([w.gains(conf.pl_size) for w in laws]), spec, disturbances, seeds)
    b.laws = laws
    return b


def run_linear_frequency(conf, laws, spec, disturbances=(), seeds=None):
    """run_frequency for linear laws (scenarios.LinearLaw) in ONE launch of avd_eval_linear_freq_f32 (csrc/lin.hip): the first axis of
    the FrequencyResults is the law axis. Decentralized platoons only. scenarios.linear_frequency_response is the float64 theory an
    unclipped law's gain_a is compared with."""
    b = prepare_linear_frequency(conf, laws, spec, disturbances, seeds)
    b.launch()
    return b.results()
