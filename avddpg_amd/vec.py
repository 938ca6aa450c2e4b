"""Batched, device-resident host API over the C ABI (include/avddpg_hip.h).

One instance of each class holds the state of P platoons x L vehicles in HBM and drives the
gfx950 kernels; Python never touches per-platoon data in the loop.  The scalar classes that
mirror the reference's object API (``environment.Platoon`` ...) are thin P = 1 views of these.

Random numbers come from one of two sources:
  * ``rng="host"``   -- the global legacy ``np.random`` stream, consumed in exactly the
                        reference's order, uploaded to the kernels (fixed-seed parity mode);
  * ``rng="device"`` -- counter-based Philox inside the kernels (throughput mode; same
                        distributions, different stream).
"""
import ctypes as C

import numpy as np
import torch

from . import _hip, dynamics, params
from ._hip import call, ptr, stream_handle


def _dev(device):
    return torch.device(device if device is not None else "cuda")


def seed_table(seeds, device, distinct=True):
    """An experiment batch's seeds -> (tuple of ints, int64 device tensor with the uint64 bit patterns the *_seeds_* kernels read).
    distinct=False: a seed may repeat (a hyperparameter sweep, whose experiments also differ in their hparams rows)."""
    seeds = tuple(int(k) for k in seeds)
    if not seeds:
        raise ValueError("an experiment batch needs at least one seed")
    if distinct and len(set(seeds)) != len(seeds):
        raise ValueError(f"duplicate seeds in {list(seeds)}: the experiments would be identical")
    if any(k < 0 or k >= 2 ** 64 for k in seeds):
        raise ValueError(f"seeds must lie in [0, 2**64): {list(seeds)}")
    bits = np.array(seeds, dtype=np.uint64).view(np.int64)
    return seeds, torch.from_numpy(bits.copy()).to(device)


# the Config fields a hyperparameter sweep may set per experiment (every one reaches the kernels as a scalar only)
HP_KEYS = ("actor_lr", "critic_lr", "tau", "gamma", "std_dev", "theta")


def hparams_rows(conf, hparams):
    """One dict per experiment (keys a subset of HP_KEYS) -> the full rows, conf's value for every missing key. Raises ValueError
    for an unknown key or a value outside what the update rules take (lr > 0, tau in (0, 1], gamma in [0, 1], std_dev, theta >= 0)."""
    import math

    rows = []
    for e, h in enumerate(hparams):
        if not isinstance(h, dict):
            raise ValueError(f"hparams[{e}] must be a dict, got {type(h).__name__}")
        bad = sorted(set(h) - set(HP_KEYS))
        if bad:
            raise ValueError(f"hparams[{e}]: unknown key(s) {bad}; a sweep sets {list(HP_KEYS)}")
        row = {k: float(h[k]) if k in h else float(getattr(conf, k)) for k in HP_KEYS}
        for k, v in row.items():
            if not math.isfinite(v):
                raise ValueError(f"hparams[{e}]: {k}={v} is not finite")
        for k in ("actor_lr", "critic_lr"):
            if row[k] <= 0:
                raise ValueError(f"hparams[{e}]: {k}={row[k]} must be > 0")
        if not 0 < row["tau"] <= 1:
            raise ValueError(f"hparams[{e}]: tau={row['tau']} must lie in (0, 1]")
        if not 0 <= row["gamma"] <= 1:
            raise ValueError(f"hparams[{e}]: gamma={row['gamma']} must lie in [0, 1]")
        for k in ("std_dev", "theta"):
            if row[k] < 0:
                raise ValueError(f"hparams[{e}]: {k}={row[k]} must be >= 0")
        rows.append(row)
    return rows


def hparams_struct(row, ou_dt):
    """One full row -> _hip.HParams with every value rounded as the scalar entry points round it: the float arguments (ctypes
    double -> float), tau / 1 - tau of the double tau (avd_adam_polyak_f32), ou_scale = f32(std_dev) * f32(sqrt(double(f32(ou_dt))))
    as a float product (avd_step_fused_f32 takes ou_dt as a float)."""
    import math

    f32 = np.float32
    h = _hip.HParams()
    h.actor_lr, h.critic_lr = f32(row["actor_lr"]), f32(row["critic_lr"])
    h.tau, h.one_minus_tau = f32(row["tau"]), f32(1.0 - row["tau"])
    h.gamma, h.ou_theta = f32(row["gamma"]), f32(row["theta"])
    h.ou_scale = f32(f32(row["std_dev"]) * f32(math.sqrt(float(f32(ou_dt)))))
    h.reserved = 0.0
    return h


def hparams_table(rows, ou_dt, device):
    """Full rows -> the avd_hparams device table (uint8 tensor, 32 bytes per experiment) the *_hp_* entry points read."""
    arr = (_hip.HParams * len(rows))(*[hparams_struct(r, ou_dt) for r in rows])
    raw = np.frombuffer(bytes(arr), dtype=np.uint8).copy()
    return torch.from_numpy(raw).to(device)


def lane_of(g, E):
    """Platoon g of a batch of E interleaved experiments -> (experiment, its platoon index in that experiment's solo run)."""
    return g % E, g // E


def batch_platoon(e, p, E):
    """Experiment e's platoon p -> its platoon index in the batch (the inverse of lane_of)."""
    return p * E + e


def train_level_table(levels, device):
    """Checked scenarios.Disturbance levels -> (the avd_train_level table as a ctypes array: the HOST copy avd_step_fused_dist_f32
    validates on every call, the same bytes as a uint8 device tensor the kernels read)."""
    from .scenarios import drop_threshold

    arr = (_hip.TrainLevel * len(levels))()
    for row, d in zip(arr, levels):
        row.sigma[0], row.sigma[1], row.sigma[2] = d.sigma
        row.delay, row.drop_q = int(d.v2v_delay), drop_threshold(d.v2v_drop)
    return arr, torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy()).to(device)


def _no_scalar_draw(what):
    raise _hip.AvdError(f"{what}: an experiment batch (seeds=...) draws only through the *_seeds_* kernels; this path would "
                        "draw with one scalar seed for every experiment")


class VecPlatoon:
    """P platoons of L vehicles. Batched ``Platoon`` (reference src/environment.py:8-301)."""

    def __init__(self, num_platoons, length, config, device=None, rand_states=True, evaluator_states_enabled=False,
                 rng="host", seed=1, track_aux=False, seeds=None, distinct_seeds=True, train_disturb=None):
        """seeds: an experiment batch -- len(seeds) experiments of num_platoons / len(seeds) platoons each, interleaved (experiment e's
        platoon p is platoon p * E + e), each drawing exactly what a solo VecPlatoon with seed=seeds[e] draws (device RNG only).
        train_disturb: scenarios.Disturbance levels to TRAIN under (already checked: trainer.check_train_disturb; device RNG): platoon p
        runs under level p % n_levels (a batch: the level of its solo run's platoon index) for good. ``self.obs`` / ``self.obs_prev``
        then hold what the agents observe of ``self.x`` / ``self.x_prev`` (sensor noise, V2V delay and loss; the level's plant drives
        x) and are swapped where x and x_prev are; every reset re-observes the fresh states (observe). None: none of this exists."""
        self.P, self.L, self.config = int(num_platoons), int(length), config
        self.length = self.L
        self.device = _dev(device)
        self.rng, self.seed = rng, int(seed)
        self.seeds = self.d_seeds = None
        self.n_groups = 1
        if seeds is not None:
            if rng != "device":
                raise ValueError("an experiment batch (seeds=...) needs rng='device'")
            self.seeds, self.d_seeds = seed_table(seeds, self.device, distinct_seeds)
            self.n_groups = len(self.seeds)
            if self.P % self.n_groups:
                raise ValueError(f"num_platoons={self.P} is not a multiple of the {self.n_groups} experiments")
        self.rand_states, self.evaluator_states_enabled = rand_states, evaluator_states_enabled
        centralized = config.framework == config.cntrl
        # attributes read by callers (environment.py:35-54)
        self.multiplier = self.L if centralized else 1
        self.hidden_multiplier = config.centrl_hidd_mult if centralized else 1
        self.num_models = 1 if centralized else self.L
        self.def_num_actions = 1
        self.num_actions = self.def_num_actions * self.multiplier
        self.def_num_states = 3 if config.model == config.modelA else 4
        self.num_states = self.def_num_states * self.multiplier
        self.number_of_reward_components = 4
        self.state_lbs = {0: "$e_{pi,k}$", 1: "$e_{vi,k}$", 2: "$a_{i,k}$", 3: "$a_{i-1,k}$"}
        self.jerk_lb, self.exog_lbl = "jerk", "$u_{i,k}$"
        self.obs_width = min(4, self.num_states)  # Vehicle.step returns x[0:num_states] (:518)

        self.h_consts = dynamics.env_consts(config, self.L)
        raw = np.frombuffer(bytes(self.h_consts), dtype=np.uint8).copy()
        self.d_consts = torch.from_numpy(raw).to(self.device)
        f32 = dict(dtype=torch.float32, device=self.device)
        P, L = self.P, self.L
        self.x = torch.zeros(P, L, 4, **f32)
        self.x_prev = torch.zeros(P, L, 4, **f32)  # state before the last step (= prev_states of the trainer)
        self.prev_a = torch.zeros(P, L, **f32)
        self.cum_accel = torch.zeros(P, L, **f32) if track_aux else None
        self.reward = torch.zeros(P, L, **f32)
        self.reward_mean = torch.zeros(P, **f32) if centralized else None
        self.term = torch.zeros(P, L, dtype=torch.uint8, device=self.device)
        self.done = torch.zeros(P, dtype=torch.uint8, device=self.device)
        # two any-terminal flag words used alternately by the fused step (avd_step_fused_f32 clears the other one); the
        # separate-kernel path keeps using word 0 and clears it with a fill
        self._any_flags = torch.zeros(2, dtype=torch.int32, device=self.device)
        self.any_done = self._any_flags[0:1]
        self.reset_count = 0
        self.step_count = 0
        self.ep_len = self.ep_stats = None  # per-platoon episodes (episode_end), made on first use
        self.levels = None
        if train_disturb is not None:
            from . import scenarios

            self.levels = list(train_disturb)
            self.h_levels, self.d_levels = train_level_table(self.levels, self.device)
            self.d_plant = torch.from_numpy(np.stack([scenarios.plant_table(config, L, d.dyn_coeff) for d in self.levels])).to(self.device)
            self.obs = torch.zeros(P, L, 4, **f32)
            self.obs_prev = torch.zeros(P, L, 4, **f32)
            self.link_hist = self.link_recv = None
            if any(d.uses_v2v for d in self.levels):  # the V2V ring and the held value, only where a level uses the link
                self.link_hist = torch.zeros(P, L, 16, **f32)
                self.link_recv = torch.zeros(P, L, **f32)
            self.obs_counter = 0  # Philox call counter of the observation in self.obs (the host owns it: step t makes t + 1)
            self.observe()
        if rng == "host":
            # constructor draws of P reference Platoon objects: 2 + 3L each (environment.py:24,32,385)
            self._host_ctor_draws()

    # -- host RNG helpers: consume np.random exactly like the reference objects --------------
    def _rand(self, val):
        c = self.config
        if c.rand_gen == c.uniform:
            return np.random.uniform(-1 * val, val)
        return np.random.normal(0, val)

    def _mode(self):
        if self.evaluator_states_enabled:
            return 1 if self.rand_states else 2
        return 0 if self.rand_states else 2

    def _host_ctor_draws(self):
        """Platoon.__init__ (:24, :32) then Vehicle.__init__ -> reset (:385): front_accel, front_u, 3 per vehicle."""
        c, P, L = self.config, self.P, self.L
        self.front_accel = np.zeros(P)
        self.front_u = np.zeros(P)
        draws = np.zeros((P, L, 3), dtype=np.float64)
        for p in range(P):
            self.front_accel[p] = self._rand(c.pl_leader_reset_a)
            self.front_u[p] = self._rand(c.reset_max_u)
            if self._mode() == 0:
                for i in range(L):
                    draws[p, i, 0] = self._rand(c.reset_ep_max)
                    draws[p, i, 1] = self._rand(c.reset_max_ev)
                    draws[p, i, 2] = self._rand(c.reset_max_a)
        self._upload_reset(draws, self.front_accel)

    def _upload_reset(self, draws, fa, cond=None):
        if self.seeds is not None:  # (a seed batch draws on the device: no host draws to upload)
            fn, key = "avd_env_reset_seeds_f32", (self._mode(), ptr(self.d_seeds), self.n_groups)
        else:
            d = torch.from_numpy(draws.astype(np.float32)).to(self.device) if draws is not None else None
            f = torch.from_numpy(np.asarray(fa, dtype=np.float32)).to(self.device) if fa is not None else None
            fn, key = "avd_env_reset_f32", (ptr(d), ptr(f), self._mode(), self.seed)
        call(fn, ptr(self.d_consts), self.P, self.L, ptr(self.x), ptr(self.prev_a), ptr(self.cum_accel), *key, self.reset_count, ptr(cond),
             stream_handle())

    def _host_reset_draws(self):
        c, P, L = self.config, self.P, self.L
        draws = np.zeros((P, L, 3), dtype=np.float64)
        fa = np.zeros(P, dtype=np.float64)
        train = self._mode() == 0
        for p in range(P):  # Platoon.reset (:284-301): front_accel, then per vehicle front_u (+3 state draws)
            fa[p] = self._rand(c.pl_leader_reset_a)
            for i in range(L):
                self.front_u[p] = self._rand(c.reset_max_u)  # kept: Platoon.step(leader_exog=None) falls back to it
                if train:
                    draws[p, i, 0] = self._rand(c.reset_ep_max)
                    draws[p, i, 1] = self._rand(c.reset_max_ev)
                    draws[p, i, 2] = self._rand(c.reset_max_a)
        self.front_accel = fa.copy()
        return draws, fa

    def observe(self, only_where_zero=None, run_if_nonzero=None):
        """(Re)observe fresh states (avd_observe_f32): self.obs from self.x with the sensor noise of the current observation counter and a
        fresh V2V link. only_where_zero: int32 [P], only platoons with a 0 entry (episode_end's ep_len); run_if_nonzero: int32 [1] device
        flag, nothing happens when it reads 0. Both None: every platoon."""
        key = (self.seed,) if self.seeds is None else (ptr(self.d_seeds), self.n_groups)
        call("avd_observe_f32" if self.seeds is None else "avd_observe_seeds_f32", self.P, self.L, ptr(self.x), ptr(self.obs),
             len(self.levels), ptr(self.d_levels), ptr(self.link_hist), ptr(self.link_recv), *key, self.obs_counter, ptr(only_where_zero),
             ptr(run_if_nonzero), stream_handle())

    def agent_states(self):
        """What the agents see of x: the observation buffer when training under disturbances, else the state itself."""
        return self.x if self.levels is None else self.obs

    # -- API ------------------------------------------------------------------------------------
    def observations(self, x=None):
        """[P, L, obs_width] view (decentralized) -- Model A hides x[3] (:518)."""
        x = self.x if x is None else x
        return x[..., : self.obs_width]

    def reset(self, cond=None):
        """All platoons reset together (workers/trainer.py:246-249). ``cond``: device int32 flag --
        reset only if non-zero (device-RNG mode only)."""
        draws = fa = None
        if self.rng == "host":
            if cond is not None:
                raise ValueError("conditional reset needs rng='device'")
            draws, fa = self._host_reset_draws()
        self._upload_reset(draws, fa, cond)
        self.reset_count += 1
        if self.levels is not None:
            self.observe(run_if_nonzero=cond)
        return self.observations()

    def episode_end(self, ep_reward, M, limit, any_reset=None):
        """Per-platoon episode end (avd_episode_end_f32; device-RNG mode): call once after every step. Platoons whose step was
        terminal or whose episode reached ``limit`` steps are closed -- their ``ep_reward`` counters [P, M] go into
        ``self.ep_stats`` (running sums over closed episodes: platoon-mean episodic reward, length, count), and they restart
        from fresh reset states. ``any_reset`` (int32[1]) is set when any platoon was closed."""
        if self.rng != "device":
            raise ValueError("per-platoon episode ends need rng='device'")
        self.ensure_episode_state()
        st = self.ep_stats
        key = (self.seed,) if self.seeds is None else (ptr(self.d_seeds), self.n_groups)
        call("avd_episode_end_f32" if self.seeds is None else "avd_episode_end_seeds_f32", ptr(self.d_consts), self.P, self.L, M,
             ptr(self.x), ptr(self.prev_a), ptr(self.cum_accel), ptr(self.done), ptr(self.ep_len), ptr(ep_reward), int(limit),
             ptr(st["ret_sum"]), ptr(st["len_sum"]), ptr(st["count"]), ptr(any_reset), self._mode(), *key, self.reset_count, stream_handle())
        self.reset_count += 1
        if self.levels is not None:  # (ep_len[p] == 0 exactly on the platoons just reset)
            self.observe(only_where_zero=self.ep_len)

    def ensure_episode_state(self):
        """The per-platoon episode counters of episode_end (made on first use)."""
        if self.ep_len is None:
            z = lambda dt: torch.zeros(self.P, dtype=dt, device=self.device)
            self.ep_len = z(torch.int32)
            self.ep_stats = dict(ret_sum=z(torch.float32), len_sum=z(torch.float32), count=z(torch.int32))

    def pop_episode_stats(self, per_experiment=False):
        """(mean platoon-mean episodic reward, mean episode length, episodes closed) since the last call; clears the sums.
        Host synchronisation: call it at reporting points, not per step.
        per_experiment (experiment batch): the three as float64 / float64 / int64 arrays [E], entry e computed from experiment e's
        platoons with the same reductions as a solo run's call (so bit-identical to it)."""
        st = self.ep_stats
        if per_experiment:
            E = self.n_groups
            parts = [{k: t.view(-1, E)[:, e].contiguous() for k, t in st.items()} for e in range(E)]
            n = np.array([int(q["count"].sum()) for q in parts], dtype=np.int64)
            ret = np.array([float(q["ret_sum"].double().sum()) for q in parts])
            ln = np.array([float(q["len_sum"].double().sum()) for q in parts])
            for t in st.values():
                t.zero_()
            with np.errstate(invalid="ignore", divide="ignore"):
                return np.where(n > 0, ret / np.maximum(n, 1), np.nan), np.where(n > 0, ln / np.maximum(n, 1), np.nan), n
        n = int(st["count"].sum())
        ret, ln = float(st["ret_sum"].double().sum()), float(st["len_sum"].double().sum())
        for t in st.values():
            t.zero_()
        return (ret / n if n else float("nan")), (ln / n if n else float("nan")), n

    def step(self, actions, leader_exog):
        """actions [P, L] float32 (device), leader_exog [P]. Returns (obs, reward, done) device tensors;
        ``self.x_prev`` then holds the pre-step state, ``self.any_done`` the any-terminal flag."""
        if self.levels is not None:
            raise _hip.AvdError("VecPlatoon.step: training under disturbances runs the fused step only (avd_step_fused_dist_f32)")
        self.x, self.x_prev = self.x_prev, self.x
        call("avd_env_step_f32", ptr(self.d_consts), self.P, self.L, ptr(self.x_prev), ptr(self.x), ptr(self.prev_a),
             ptr(self.cum_accel), ptr(actions), ptr(leader_exog), ptr(self.reward), ptr(self.term), ptr(self.done),
             ptr(self.reward_mean), ptr(self.any_done), stream_handle())
        self.step_count += 1
        return self.observations(), self.reward, self.done

    def get_jerk_from(self, x_before, prev_a_before):
        """jerk of the step that consumed (x_before, prev_a_before) (environment.py:477)."""
        return (x_before[..., 2] - prev_a_before) / self.config.sample_rate


class VecOUNoise:
    """n independent scalar OU processes (reference src/noise.py)."""

    def __init__(self, n, config, device=None, rng="host", seed=1, mean=0.0, seeds=None, distinct_seeds=True):
        """seeds: an experiment batch's seed table (its draws happen inside avd_step_fused_seeds_f32, which advances ``calls``;
        calling this object then raises)."""
        self.n, self.config, self.device = int(n), config, _dev(device)
        self.rng, self.seed, self.calls = rng, int(seed), 0
        self.seeds = None if seeds is None else seed_table(seeds, "cpu", distinct_seeds)[0]
        if self.seeds is not None and rng != "device":
            raise ValueError("an experiment batch (seeds=...) needs rng='device'")
        self.mean = float(mean)  # the level every process reverts to (src/noise.py:7, 17; the reference trainer passes zeros)
        self.state = torch.zeros(self.n, dtype=torch.float32, device=self.device)  # x_prev = 0 (noise.py:29)

    def reset(self):
        self.state.zero_()

    def __call__(self, normals=None):
        """Advance all processes; ``normals`` [n] host array of N(0,1) draws (host-RNG mode)."""
        if self.seeds is not None:
            _no_scalar_draw("VecOUNoise()")
        c = self.config
        d_n = None
        if self.rng == "host":
            if normals is None:
                normals = np.random.normal(0, 1.0, size=self.n)
            d_n = torch.from_numpy(np.asarray(normals, dtype=np.float32).reshape(self.n)).to(self.device)
        call("avd_ou_step_f32", self.n, ptr(self.state), ptr(d_n), c.theta, self.mean, c.ou_dt, c.std_dev, self.seed,
             self.calls, stream_handle())
        self.calls += 1
        return self.state


class VecReplay:
    """One ring buffer per agent: ring[n_agents][cap][2S+A+1] float32 (reference src/replaybuffer.py)."""

    def __init__(self, n_agents, buffer_capacity, batch_size, num_states, num_actions, device=None, rng="host",
                 seed=1, ring=None, seeds=None, agents_per_platoon=1, distinct_seeds=True):
        """ring: an existing [n_agents, capacity, 2S+A+1] float32 device tensor to use instead of allocating one (two trainers
        of the same shape measured in one process share the 82 GB ring of BASELINE configs[1]).
        seeds: an experiment batch (agent v = (p*E + e) * agents_per_platoon + m belongs to experiment e): sample() draws through
        avd_replay_sample_seeds_f32, each experiment's indices those of a solo VecReplay with seed=seeds[e]."""
        self.n, self.cap, self.B = int(n_agents), int(buffer_capacity), int(batch_size)
        self.S, self.A = int(num_states), int(num_actions)
        self.row = 2 * self.S + self.A + 1
        self.device, self.rng, self.seed = _dev(device), rng, int(seed)
        self.seeds = self.d_seeds = None
        self.agents_per_platoon = int(agents_per_platoon)
        if seeds is not None:
            if rng != "device":
                raise ValueError("an experiment batch (seeds=...) needs rng='device'")
            self.seeds, self.d_seeds = seed_table(seeds, self.device, distinct_seeds)
            if self.n % (len(self.seeds) * self.agents_per_platoon):
                raise ValueError(f"n_agents={self.n} is not a multiple of {len(self.seeds)} experiments x {self.agents_per_platoon} agents")
        if ring is not None:
            if tuple(ring.shape) != (self.n, self.cap, self.row) or ring.dtype != torch.float32 or not ring.is_contiguous():
                raise _hip.AvdError(f"replay ring must be contiguous float32 {(self.n, self.cap, self.row)}, got {tuple(ring.shape)}")
            self.ring = ring
        else:
            self.ring = torch.zeros(self.n, self.cap, self.row, dtype=torch.float32, device=self.device)
        self.buffer_counter = 0  # identical for all agents: they are written in lock step
        self.samples = 0
        f32 = dict(dtype=torch.float32, device=self.device)
        self.idx = torch.zeros(self.n, self.B, dtype=torch.int32, device=self.device)
        self.s = torch.zeros(self.n, self.B, self.S, **f32)
        self.a = torch.zeros(self.n, self.B, self.A, **f32)
        self.r = torch.zeros(self.n, self.B, **f32)
        self.s2 = torch.zeros(self.n, self.B, self.S, **f32)

    def add(self, s_prev, action, reward, s_next, x_stride):
        """s_prev / s_next: [n_agents, x_stride] device tensors (first S columns used)."""
        call("avd_replay_add_f32", self.n, self.cap, self.S, self.A, ptr(self.ring), self.buffer_counter, ptr(s_prev),
             ptr(s_next), x_stride, ptr(action), ptr(reward), stream_handle())
        self.buffer_counter += 1

    def sample_range(self):
        return min(self.buffer_counter, self.cap)  # replaybuffer.py:52

    def draw_indices(self, host_idx=None):
        """host mode: np.random.choice(range, B) per agent in agent order (replaybuffer.py:54)."""
        if self.seeds is not None:
            _no_scalar_draw("VecReplay.draw_indices")
        if self.rng == "host":
            if host_idx is None:
                rr = self.sample_range()
                host_idx = np.stack([np.random.choice(rr, self.B) for _ in range(self.n)])
            self.idx.copy_(torch.from_numpy(np.asarray(host_idx).astype(np.int32)))
        else:
            call("avd_replay_indices", self.n, self.B, self.sample_range(), self.seed, self.samples, ptr(self.idx),
                 stream_handle())
        self.samples += 1
        return self.idx

    def gather(self):
        call("avd_replay_gather_f32", self.n, self.cap, self.S, self.A, self.B, ptr(self.ring), ptr(self.idx),
             ptr(self.s), ptr(self.a), ptr(self.r), ptr(self.s2), stream_handle())
        return self.s, self.a, self.r, self.s2

    def sample(self, host_idx=None):
        """ReplayBuffer.sample (src/replaybuffer.py:49-63). Device-RNG mode: index draw + row gather in ONE launch
        (avd_replay_sample_f32: the same Philox draws as draw_indices(), bit for bit, rows moved whole)."""
        if self.seeds is not None:
            if host_idx is not None or not (self.A == 1 and self.S in (3, 4) and self.B % 4 == 0):
                _no_scalar_draw("VecReplay.sample (host indices, or a shape avd_replay_sample_seeds_f32 does not serve)")
            call("avd_replay_sample_seeds_f32", self.n, self.cap, self.S, self.A, self.B, ptr(self.ring), self.sample_range(),
                 ptr(self.d_seeds), len(self.seeds), self.agents_per_platoon, self.samples, ptr(self.idx), ptr(self.s), ptr(self.a),
                 ptr(self.r), ptr(self.s2), stream_handle())
            self.samples += 1
            return self.s, self.a, self.r, self.s2
        if self.rng != "host" and host_idx is None and self.A == 1 and self.S in (3, 4) and self.B % 4 == 0:
            call("avd_replay_sample_f32", self.n, self.cap, self.S, self.A, self.B, ptr(self.ring), self.sample_range(), self.seed,
                 self.samples, ptr(self.idx), ptr(self.s), ptr(self.a), ptr(self.r), ptr(self.s2), stream_handle())
            self.samples += 1
            return self.s, self.a, self.r, self.s2
        self.draw_indices(host_idx)
        return self.gather()


class AgentGroup:
    """n_sets actor/critic/target/Adam weight sets in flat slabs (reference agent/model.py,
    workers/trainer.py:100-139).  ``set_mod`` maps agent v to its weight set: 0 -> set v
    (one per agent, reference nofrl), M -> set v % M (shared per vehicle index)."""

    def __init__(self, n_sets, num_states, num_actions, config, device=None, hidd_mult=1, seed=None, high_bound=None, seeds=None,
                 seed_block=1):
        """seeds (an experiment batch; exclusive with seed): set j belongs to experiment (j // seed_block) % len(seeds) and starts from
        the weights a group built with seed=seeds[e] starts from (seed_block = M: the interleaved layout of VecPlatoon(seeds=...) for
        per-agent sets and for shared sets alike)."""
        c = config
        self.config, self.device, self.n_sets = c, _dev(device), int(n_sets)
        if (c.critic_layer1_size, c.critic_layer2_size) != (c.actor_layer1_size, c.actor_layer2_size):
            raise _hip.AvdError("actor and critic layer1/layer2 sizes must match (reference defaults do)")
        # logical widths (agent/model.py:27,30,65,70: int(size * hidd_mult)); the slabs use zero-padded widths
        self.dims = params.Dims(num_states, num_actions, int(c.actor_layer1_size * hidd_mult),
                                int(c.actor_layer2_size * hidd_mult), int(c.critic_act_layer_size * hidd_mult))
        H1p, H2p, Hap = params.padded_widths(self.dims.H1, self.dims.H2, self.dims.Ha)
        self.lay = _hip.make_layout(num_states, num_actions, H1p, H2p, Hap, c.batch_size)
        self.high = float(c.action_high if high_bound is None else high_bound)
        f32 = dict(dtype=torch.float32, device=self.device)
        n, T, S = self.n_sets, self.lay.theta_size, self.lay.stats_size
        self.theta = torch.zeros(n, T, **f32)
        self.stats = torch.zeros(n, S, **f32)
        self.theta_t = torch.zeros(n, T, **f32)
        self.stats_t = torch.zeros(n, S, **f32)
        self.m = torch.zeros(n, T, **f32)
        self.v = torch.zeros(n, T, **f32)
        self.step = torch.zeros(n, dtype=torch.int32, device=self.device)
        self._layp = C.byref(self.lay)
        if seeds is not None and seed is not None:
            raise ValueError("AgentGroup: seed and seeds are mutually exclusive")
        init = lambda k: params.init_weights(self.lay, np.random.RandomState(k), nominal=(c.actor_layer1_size, c.actor_layer2_size),
                                             dims=self.dims)
        if seeds is None:
            th, st = init(c.random_seed if seed is None else seed)
            # every agent starts from agent (0,0)'s weights; targets copy their online nets (trainer.py:121-131)
            self.theta.copy_(torch.from_numpy(th).to(self.device).expand(n, T))
            self.stats.copy_(torch.from_numpy(st).to(self.device).expand(n, S))
        else:
            E, blk = len(seeds), int(seed_block)
            if n % (E * blk):
                raise ValueError(f"AgentGroup: {n} sets are not a multiple of {E} experiments x {blk}")
            for e, k in enumerate(seeds):  # each experiment's sets from its own seed, as its solo run
                th, st = init(int(k))
                self.theta.view(-1, E, blk, T)[:, e].copy_(torch.from_numpy(th).to(self.device).expand(n // (E * blk), blk, T))
                self.stats.view(-1, E, blk, S)[:, e].copy_(torch.from_numpy(st).to(self.device).expand(n // (E * blk), blk, S))
        self.theta_t.copy_(self.theta)
        self.stats_t.copy_(self.stats)
        # a hyperparameter sweep: (avd_hparams device table, n_groups, set_block) -- set / agent j takes row (j // set_block) % n_groups;
        # learn / apply / learn_update then go through the *_hp_* entry points (set_hparams)
        self.hp = None
        # the actor's step size every update call passes by value: None = the configuration's (see actor_lr)
        self._actor_lr = None

    @property
    def actor_lr(self):
        """The actor's Adam step size handed to the update kernels (apply, apply_intra, learn_update, learn_apply): the
        configuration's, unless one has been set. Setting 0 holds the actors still (VecTrainer(actor_hold=N)): w - 0 * x = w keeps
        every actor weight's bits, while the actor's Adam moments and iteration count keep accumulating; None gives the
        configuration's back. A hyperparameter sweep reads its step sizes from its table, not from here."""
        return self.config.actor_lr if self._actor_lr is None else self._actor_lr

    @actor_lr.setter
    def actor_lr(self, value):
        self._actor_lr = None if value is None else float(value)

    def clone_fit(self, spec, seeds=None, M=None, seed=None, loss_log=None):
        """Imitation warm start: fit the actors to the linear law ``spec`` (scenarios.WarmStart) by spec.steps Adam steps of size spec.lr
        on fresh batches of 64 states drawn uniformly in spec.box(config), the target the law's clipped action.
        The E * M sets of platoon 0 are fitted (E = len(seeds) experiments, or 1; M vehicle indices; set j is experiment (j // M) % E,
        vehicle j % M -- the layout of AgentGroup(seeds=..., seed_block=M)), each step three launches: avd_clone_sample_f32 (Philox
        key = seeds[e], or ``seed`` / config.random_seed; counter = the fit step), avd_actor_clone_f32, avd_adam_polyak_f32 with
        actor_lr = spec.lr and tau = 1. The gradient slab's critic block is zero and so are the moments, so the critic keeps its bits;
        tau = 1 leaves every target equal to its online net. Afterwards m, v and step of the fitted sets are zero again (DDPG's Adam
        starts as in a cold run) and the fitted rows of theta, theta_t (and learn_update's ping-pong slab, if it exists) are copied
        to the same (experiment, vehicle) set of every other platoon: per-agent sets stay identical across platoons, as after the
        reference's initialisation. With n_sets == E * M (shared sets) nothing is copied. Refused once any update has been made.
        Returns the last step's losses [E * M] on the host; the one synchronisation is that read. loss_log (optional, a device
        tensor [steps, E * M]) receives every step's losses."""
        from . import scenarios
        scenarios.check_warm_start(spec, self.config)
        self._no_hp("clone_fit")
        c, lay = self.config, self.lay
        if lay.A != 1 or lay.S not in (3, 4):
            raise _hip.AvdError(f"clone_fit: a linear law is per vehicle (S in (3, 4), A = 1), got S={lay.S} A={lay.A}")
        if M is None:
            M = c.pl_size
        M = int(M)
        E = 1 if seeds is None else len(seeds)
        n_fit = E * M
        if M < 1 or self.n_sets % n_fit:
            raise ValueError(f"clone_fit: {self.n_sets} sets are not a multiple of {E} experiments x {M} vehicles")
        d_seeds = None if seeds is None else seed_table(seeds, self.device, distinct=False)[1]
        key = int(c.random_seed if seed is None else seed) if seeds is None else 0
        f32 = dict(dtype=torch.float32, device=self.device)
        gains = torch.from_numpy(spec.gains(M)).to(self.device)
        box = torch.from_numpy(spec.box(c)).to(self.device)
        s = torch.empty(n_fit, lay.B, lay.S, **f32)
        u = torch.empty(n_fit, lay.B, 1, **f32)
        grads = torch.empty(n_fit, lay.theta_size, **f32)
        losses = torch.zeros(n_fit, **f32)
        model_a = 1 if c.model == c.modelA else 0
        sl = slice(0, n_fit)
        th, st, tht, stt, m, v = (x[sl] for x in (self.theta, self.stats, self.theta_t, self.stats_t, self.m, self.v))
        # Adam's iteration count of every fit step, laid out once: no launch of its own between the three of a step
        counts = torch.arange(1, int(spec.steps) + 1, dtype=torch.int32, device=self.device).repeat_interleave(n_fit).view(-1, n_fit)
        stream = stream_handle()
        for k in range(int(spec.steps)):
            out = losses if loss_log is None else loss_log[k]
            call("avd_clone_sample_f32", n_fit, lay.S, M, ptr(gains), ptr(box), float(c.action_low), float(c.action_high), model_a, key, k,
                 ptr(d_seeds), E, ptr(s), ptr(u), stream)
            call("avd_actor_clone_f32", self._layp, n_fit, ptr(th), ptr(st), ptr(s), ptr(u), self.high, ptr(grads), ptr(out), stream)
            call("avd_adam_polyak_f32", self._layp, n_fit, ptr(th), ptr(st), ptr(tht), ptr(stt), ptr(m), ptr(v), ptr(grads), ptr(counts[k]),
                 float(spec.lr), c.critic_lr, 1.0, stream)
        m.zero_(), v.zero_(), self.step[sl].zero_()
        if self.n_sets > n_fit:  # every other platoon's set of the same (experiment, vehicle)
            T, reps = lay.theta_size, self.n_sets // n_fit - 1
            for slab in (self.theta, self.theta_t):
                slab.view(-1, n_fit, T)[1:].copy_(slab.view(-1, n_fit, T)[:1].expand(reps, n_fit, T))
        if getattr(self, "theta_alt", None) is not None:
            self.theta_alt.copy_(self.theta)
        if loss_log is not None:
            losses = loss_log[int(spec.steps) - 1]
        return losses.cpu().numpy()

    def set_hparams(self, table, n_groups, set_block):
        """Route learn / apply / learn_update through the *_hp_* entry points with this avd_hparams table (vec.hparams_table)."""
        if self.n_sets % (int(n_groups) * int(set_block)):
            raise ValueError(f"AgentGroup: {self.n_sets} sets are not a multiple of {n_groups} experiments x {set_block}")
        self.hp = (table, int(n_groups), int(set_block))

    def copy_experiments(self, pairs, n_groups, set_block):
        """Population-based training: for every (src, dst) experiment pair, the k-th weight set of dst becomes a bitwise copy of the k-th
        set of src -- theta, theta_t, m, v, stats, stats_t and step; set j belongs to experiment (j // set_block) % n_groups
        (avd_copy_experiment_sets_f32: destinations distinct and never a source, or nothing is written). One launch on the current
        stream, no host synchronisation. theta_alt (learn_update's ping-pong slab) is rewritten whole by the next step and is not copied."""
        flat = [int(x) for pr in pairs for x in pr]
        if len(flat) != 2 * len(pairs):
            raise ValueError(f"pairs must be (src, dst) experiment pairs, got {pairs!r}")
        arr = (C.c_int32 * max(1, len(flat)))(*flat)
        call("avd_copy_experiment_sets_f32", self._layp, self.n_sets, int(n_groups), int(set_block), arr, len(pairs), ptr(self.theta),
             ptr(self.stats), ptr(self.theta_t), ptr(self.stats_t), ptr(self.m), ptr(self.v), ptr(self.step), stream_handle())

    def keep_best(self, d_set_base, h_set_base, M, NS, counters, step, best_theta, best_stats, best_score, best_step, improved):
        """Retention of the best actors seen (avd_keep_best_f32, csrc/best.hip) on slabs the caller holds: unit u owns this group's sets
        d_set_base[u] .. +M-1 (int32 device table; h_set_base its host copy, a ctypes int32 array the entry checks) and the NS x M
        rollout counters counters[u]; where its score -- their sequential float32 mean -- beats best_score[u], its actor spans and actor
        BN statistics go to rows u*M .. of best_theta [n_units*M, actor_size] / best_stats [n_units*M, cmms], best_score[u] and
        best_step[u] (int64) are set and improved[u] (int32) is 1, else 0 and nothing is written. Two launches on the current stream, no
        host synchronisation. theta and stats are taken at call time: the fused update swaps theta with its ping-pong slab every step."""
        call("avd_keep_best_f32", self._layp, len(h_set_base), int(M), int(NS), self.n_sets, ptr(d_set_base), h_set_base, ptr(counters),
             ptr(self.theta), ptr(self.stats), int(step), ptr(best_theta), ptr(best_stats), ptr(best_score), ptr(best_step), ptr(improved),
             stream_handle())

    def _no_hp(self, what):
        if self.hp is not None:
            raise _hip.AvdError(f"{what}: a hyperparameter sweep (set_hparams) has no per-experiment form of this path")

    # -- forward ----------------------------------------------------------------------------------
    def actor(self, states, set_mod, x_stride=None, out=None, target=False, run_if_nonzero=None):
        """states [n_agents, x_stride] -> tanh(.)*high [n_agents] ([n_agents, A] when A > 1) (agent/model.py:26-36).
        run_if_nonzero: int32[1] device flag; the launch is a no-op when it reads 0 (`out` then keeps what a fused update
        left there, see learn_update)."""
        n_agents = states.shape[0]
        x_stride = states.shape[-1] if x_stride is None else x_stride
        shape = (n_agents,) if self.lay.A == 1 else (n_agents, self.lay.A)
        out = torch.empty(*shape, dtype=torch.float32, device=self.device) if out is None else out
        th, st = (self.theta_t, self.stats_t) if target else (self.theta, self.stats)
        if run_if_nonzero is not None:
            call("avd_actor_forward_cond_f32", self._layp, n_agents, set_mod, ptr(th), ptr(st), ptr(states), x_stride,
                 self.high, ptr(out), ptr(run_if_nonzero), stream_handle())
        else:
            call("avd_actor_forward_f32", self._layp, n_agents, set_mod, ptr(th), ptr(st), ptr(states), x_stride,
                 self.high, ptr(out), stream_handle())
        return out

    def actor_set(self, states, n_agents, x_stride=None, out=None, run_if_nonzero=None):
        """actor(state) for n_agents agents that SHARE this group's weight sets (agent v uses set v % n_sets) on the f32
        matrix cores (csrc/act.hip; reference widths). states [n_agents, x_stride] -> [n_agents]; same values as
        actor(states, set_mod=n_sets) up to the f32 summation order."""
        x_stride = states.shape[-1] if x_stride is None else x_stride
        out = torch.empty(n_agents, dtype=torch.float32, device=self.device) if out is None else out
        call("avd_actor_forward_set_f32", self._layp, n_agents, self.n_sets, ptr(self.theta), ptr(self.stats), ptr(states), x_stride,
             self.high, ptr(out), ptr(run_if_nonzero), stream_handle())
        return out

    def critic(self, states, actions, set_mod, x_stride=None, out=None, target=False):
        n_agents = states.shape[0]
        x_stride = states.shape[-1] if x_stride is None else x_stride
        shape = (n_agents,) if self.lay.A == 1 else (n_agents, self.lay.A)
        out = torch.empty(*shape, dtype=torch.float32, device=self.device) if out is None else out
        th, st = (self.theta_t, self.stats_t) if target else (self.theta, self.stats)
        call("avd_critic_forward_f32", self._layp, n_agents, set_mod, ptr(th), ptr(st), ptr(states), x_stride,
             ptr(actions), ptr(out), stream_handle())
        return out

    # -- learn / apply ----------------------------------------------------------------------------
    def learn(self, s, a, r, s2, set_mod, grads=None, losses=None):
        """Trainer.learn (workers/trainer.py:472-508) for n_agents batches -> grads [n_agents, theta_size]."""
        n_agents = s.shape[0]
        if grads is None:
            grads = torch.empty(n_agents, self.lay.theta_size, dtype=torch.float32, device=self.device)
        args = (self._layp, n_agents, set_mod, ptr(self.theta), ptr(self.stats), ptr(self.theta_t), ptr(self.stats_t), ptr(s), ptr(a), ptr(r),
                ptr(s2))
        if self.hp is not None:  # each agent's gamma from the sweep table
            tbl, E, blk = self.hp
            call("avd_learn_hp_f32", *args, self.high, ptr(grads), ptr(losses), ptr(tbl), E, blk, stream_handle())
        else:
            call("avd_learn_f32", *args, self.config.gamma, self.high, ptr(grads), ptr(losses), stream_handle())
        return grads

    def _workspace(self, attr, size_fn, n_agents):
        """The scratch buffer of a library call: `size_fn` says how many bytes (n_agents, n_sets) takes; one uint8 tensor per `attr`,
        which only ever grows."""
        need = C.c_size_t(0)
        call(size_fn, self._layp, n_agents, self.n_sets, C.byref(need))
        ws = getattr(self, attr, None)
        if ws is None or ws.numel() < need.value:
            ws = torch.empty(need.value, dtype=torch.uint8, device=self.device)
            setattr(self, attr, ws)
        return ws

    def learn_shared(self, s, a, r, s2, n_agents, grads=None, losses=None, row_weight=None):
        """Trainer.learn + federated mean for agents that SHARE this group's ``n_sets`` weight sets (interfrl with every
        step federated), as layer-wise bf16 GEMMs over all rows of a set (csrc/wide.hip). Batches are SET-MAJOR:
        s, s2 [n_sets, rows, S], a [n_sets, rows, 1], r [n_sets, rows] with rows = n_agents / n_sets * batch_size.
        row_weight [n_sets, rows] (optional): w_p * P / sum(w) on platoon p's rows = the weighted federated mean.
        Returns the mean gradient per set [n_sets, theta_size]."""
        if grads is None:
            grads = torch.empty(self.n_sets, self.lay.theta_size, dtype=torch.float32, device=self.device)
        ws = self._workspace("_wide_ws", "avd_learn_shared_workspace", n_agents)
        call("avd_learn_shared_bf16", self._layp, n_agents, self.n_sets, ptr(self.theta), ptr(self.stats),
             ptr(self.theta_t), ptr(self.stats_t), ptr(s), ptr(a), ptr(r), ptr(s2), ptr(row_weight), self.config.gamma,
             self.high, ptr(grads), ptr(losses), ptr(ws), ws.numel(), stream_handle())
        return grads

    def learn_set_fused(self, s, a, r, s2, n_agents, grads=None, losses=None, agent_weight=None, split=False, phase=None):
        """Trainer.learn + federated mean for agents that SHARE this group's ``n_sets`` weight sets, at the reference
        widths, as persistent resident-weight kernels. Batches are AGENT-MAJOR as sampled (agent v = p*n_sets + m uses set
        m): s, s2 [n_agents, B, S], a [n_agents, B(, 1)], r [n_agents, B].
        agent_weight [n_agents] (optional): w_p * P / sum(w) per agent = the weighted federated mean.
        split=False: bf16 GEMM operands (csrc/fset.hip, avd_learn_set_fused_bf16);
        split=True: every operand an fp16 hi + lo pair, f32-class results (csrc/fsplit.hip, avd_learn_set_split_f16x3).
        phase (split only): None = the whole call; "critic" / "actor" = its two halves over the same workspace
        (avd_learn_set_split_critic / _actor: the critic block of ``grads`` is final after the first, the actor block after the
        second; same stream, same ``grads``, nothing else in between -- VecTrainer(overlap_allreduce=True) puts the critic block's
        all-reduce between them on a side stream).
        Returns the mean gradient per set [n_sets, theta_size]."""
        if self.hp is not None and not (split and phase is None):
            self._no_hp("learn_set_fused (bf16 operands, or a phase of the split call)")
        if split:
            if phase not in (None, "critic", "actor"):
                raise _hip.AvdError(f"phase={phase!r}")
            entry, tail = "avd_learn_set_split_" + (phase or "f16x3"), tuple
            if self.hp is not None:  # a sweep: each set's gamma from the table (avd_learn_set_split_hp_f16x3)
                tbl, E, blk = self.hp
                entry, tail = "avd_learn_set_split_hp_f16x3", lambda: (ptr(tbl), E, blk)
            return self._split_learn(entry, (s, a, r, s2, n_agents, agent_weight), grads, losses, tail=tail)
        self._check_agent_major(s, a, r, s2, n_agents, agent_weight)
        if grads is None:
            grads = torch.empty(self.n_sets, self.lay.theta_size, dtype=torch.float32, device=self.device)
        ws = self._workspace("_fset_ws", "avd_learn_set_fused_workspace", n_agents)
        if phase is not None:
            raise _hip.AvdError("phase= needs split=True (csrc/fsplit.hip)")
        call("avd_learn_set_fused_bf16", self._layp, n_agents, self.n_sets, ptr(self.theta), ptr(self.stats), ptr(self.theta_t),
             ptr(self.stats_t), ptr(s), ptr(a), ptr(r), ptr(s2), ptr(agent_weight), self.config.gamma, self.high, ptr(grads), ptr(losses),
             ptr(ws), ws.numel(), stream_handle())
        return grads

    def _split_learn(self, entry, batch, grads, losses, what=None, tail=tuple):
        """What every method of the split set learner (csrc/fsplit.hip) does around its library call. ``batch``: (s, a, r, s2, n_agents,
        agent_weight). ``what``: the method's name where a sweep has no form of it. ``tail``: makes the entry's own arguments behind the
        common ones, raising for those it refuses (the anchor's buffers, the seed table), once the batch has passed. Returns ``grads``."""
        s, a, r, s2, n_agents, agent_weight = batch
        if what is not None:
            self._no_hp(what)
        self._check_agent_major(s, a, r, s2, n_agents, agent_weight)
        tail = tail()
        if grads is None:
            grads = torch.empty(self.n_sets, self.lay.theta_size, dtype=torch.float32, device=self.device)
        ws = self._workspace("_fsplit_ws", "avd_learn_set_split_workspace", n_agents)
        if entry.endswith("_actor"):  # the actor phase reads the states alone, and what the critic phase left in `ws`
            args = (ptr(s), self.high, ptr(grads))
        else:
            gamma = () if entry.endswith("_hp_f16x3") else (self.config.gamma,)  # (a sweep reads each set's from its table)
            args = (ptr(self.theta_t), ptr(self.stats_t), ptr(s), ptr(a), ptr(r), ptr(s2), ptr(agent_weight), *gamma, self.high, ptr(grads),
                    ptr(losses))
        call(entry, self._layp, n_agents, self.n_sets, ptr(self.theta), ptr(self.stats), *args, ptr(ws), ws.numel(), *tail, stream_handle())
        return grads

    def learn_set_split(self, s, a, r, s2, n_agents, grads=None, losses=None, agent_weight=None):
        """learn_set_fused with f32-class results (split operands, csrc/fsplit.hip)."""
        return self.learn_set_fused(s, a, r, s2, n_agents, grads=grads, losses=losses, agent_weight=agent_weight, split=True)

    def learn_set_split_anchor(self, s, a, r, s2, n_agents, gains, weight, anchor_loss, grads=None, losses=None, agent_weight=None):
        """learn_set_split with a behaviour-cloning term in the actor loss (avd_learn_set_split_anchor_f16x3): the actors minimise
        -mean(w q(s, mu)) + weight * mean(w (mu - u*)^2), u* the clipped linear law of ``gains`` [M, 4] (float32, on the device; set j uses
        row j % M, the seed-batch layout) on the sampled state. ``anchor_loss`` [n_sets] receives mean(w (mu - u*)^2) per set -- not times
        ``weight``, and for weight 0 too. The critic block and ``losses`` are learn_set_split's bit for bit."""
        def tail():
            self._check_anchor_buffers(gains, anchor_loss)
            c = self.config
            return (ptr(gains), int(gains.shape[0]), int(c.model == c.modelA), float(c.action_low), float(c.action_high), float(weight),
                    ptr(anchor_loss))
        return self._split_learn("avd_learn_set_split_anchor_f16x3", (s, a, r, s2, n_agents, agent_weight), grads, losses,
                                 "learn_set_split_anchor", tail)

    def _check_anchor_buffers(self, gains, anchor_loss):
        """The anchored calls take raw pointers to the gain table [M, 4] and the per-set anchor loss [n_sets]."""
        if (gains.dim() != 2 or gains.shape[1] != 4 or gains.dtype != torch.float32 or not gains.is_contiguous() or gains.shape[0] < 1
                or self.n_sets % gains.shape[0]):
            raise _hip.AvdError(f"anchor: gains must be contiguous float32 [M, 4] with n_sets={self.n_sets} a multiple of M, got "
                                f"{tuple(gains.shape)} {gains.dtype}")
        if anchor_loss.numel() != self.n_sets or anchor_loss.dtype != torch.float32 or not anchor_loss.is_contiguous():
            raise _hip.AvdError(f"anchor: anchor_loss must be contiguous float32 [{self.n_sets}], got {tuple(anchor_loss.shape)} "
                                f"{anchor_loss.dtype}")

    def _smooth_key(self, noise, seed, d_seeds, what):
        """(sigma, clip, seed, d_seeds pointer, E) of a smoothing call: ``noise`` anything with .sigma and .clip; ``d_seeds`` the int64
        device tensor of vec.seed_table (an experiment batch) or None."""
        if d_seeds is not None and (d_seeds.dtype != torch.int64 or d_seeds.dim() != 1 or not d_seeds.is_contiguous() or not d_seeds.is_cuda):
            raise _hip.AvdError(f"{what}: d_seeds must be vec.seed_table's contiguous int64 device tensor, got {tuple(d_seeds.shape)} "
                                f"{d_seeds.dtype}")
        E = 1 if d_seeds is None else int(d_seeds.numel())
        key = int(self.config.random_seed if seed is None else seed) if d_seeds is None else 0
        return float(noise.sigma), float(noise.clip), key, ptr(d_seeds), E

    def target_smooth(self, a2, noise, counter, M=None, seed=None, d_seeds=None):
        """Target policy smoothing alone (avd_target_smooth_f32), in place on ``a2`` [n_agents, 64] float32 (agent-major, agent v of weight
        set v % (E * M)): a2 <- clip(a2 + clip(sigma n, -clip, clip), action_low, action_high) with the normals keyed by (seed or
        d_seeds[e], counter, the agent's index in its experiment's solo run). ``noise``: a trainer.TargetNoise (anything with .sigma and
        .clip); M: vehicles per platoon (default n_sets // E). What learn_set_split_smooth applies to its target actions. Returns a2."""
        if a2.dim() != 2 or a2.shape[1] != 64 or a2.dtype != torch.float32 or not a2.is_contiguous() or not a2.is_cuda:
            raise _hip.AvdError(f"target_smooth: a2 must be a contiguous float32 [n_agents, 64] device tensor, got {tuple(a2.shape)} {a2.dtype}")
        sigma, clip, key, seeds, E = self._smooth_key(noise, seed, d_seeds, "target_smooth")
        c = self.config
        call("avd_target_smooth_f32", int(a2.shape[0]), int(self.n_sets // E if M is None else M), E, ptr(a2), sigma, clip,
             float(c.action_low), float(c.action_high), key, int(counter), seeds, stream_handle())
        return a2

    def learn_set_split_smooth(self, s, a, r, s2, n_agents, noise, counter, anchor=None, grads=None, losses=None, agent_weight=None, M=None,
                               seed=None, d_seeds=None):
        """learn_set_split with target policy smoothing (avd_learn_set_split_smooth_f16x3): the critic's targets are
        r + gamma Q'(s2, clip(mu'(s2) + clip(sigma n, -clip, clip), action_low, action_high)), the noise target_smooth's for this
        ``counter`` (the caller's learner-call count), ``seed`` (default: the configuration's) or ``d_seeds`` (vec.seed_table's device
        tensor: E experiments, set j of experiment (j // M) % E) and M (vehicles per platoon, default n_sets // E). ``noise``: a
        trainer.TargetNoise; sigma 0 is the un-smoothed call bit for bit. ``anchor``: None, or (gains [M, 4], weight, anchor_loss [n_sets])
        as learn_set_split_anchor takes them -- the anchored seed then runs in the same call. The actor block of the gradients and
        losses[:, 1] do not depend on the noise."""
        def tail():
            sigma, clip, key, seeds, E = self._smooth_key(noise, seed, d_seeds, "learn_set_split_smooth")
            gains = weight = anchor_loss = None
            m = M
            if anchor is not None:
                gains, weight, anchor_loss = anchor
                self._check_anchor_buffers(gains, anchor_loss)
                if m is None:
                    m = int(gains.shape[0])
                elif int(m) != int(gains.shape[0]):
                    raise _hip.AvdError(f"learn_set_split_smooth: M={m} but the anchor's table has {gains.shape[0]} rows (one M serves both)")
            if m is None:
                m = self.n_sets // E
            c = self.config
            return (ptr(gains), int(m), int(c.model == c.modelA), float(c.action_low), float(c.action_high),
                    0.0 if weight is None else float(weight), ptr(anchor_loss), sigma, clip, key, int(counter), seeds, E)
        return self._split_learn("avd_learn_set_split_smooth_f16x3", (s, a, r, s2, n_agents, agent_weight), grads, losses,
                                 "learn_set_split_smooth", tail)

    def _check_agent_major(self, s, a, r, s2, n_agents, agent_weight):
        """The set learners of csrc/fset.hip / fsplit.hip take raw pointers to tightly packed AGENT-major f32 batches
        [n_agents, B, S]: a set-major or strided view (what learn_shared wants) would silently give wrong gradients."""
        lay = self.lay
        want = {"s": (n_agents, lay.B, lay.S), "s2": (n_agents, lay.B, lay.S), "r": (n_agents, lay.B)}
        for name, x in (("s", s), ("s2", s2), ("r", r)):
            if tuple(x.shape) != want[name] or x.dtype != torch.float32 or not x.is_contiguous():
                raise _hip.AvdError(f"set learner: {name} must be contiguous float32 {want[name]} (agent-major), got "
                                    f"{tuple(x.shape)} {x.dtype} contiguous={x.is_contiguous()}")
        if a.numel() != n_agents * lay.B * lay.A or a.dtype != torch.float32 or not a.is_contiguous() or a.shape[0] != n_agents:
            raise _hip.AvdError(f"set learner: a must be contiguous float32 [{n_agents}, {lay.B}(, {lay.A})], got {tuple(a.shape)} {a.dtype}")
        if n_agents <= 0 or n_agents % self.n_sets:
            raise _hip.AvdError(f"set learner: n_agents={n_agents} is not a multiple of n_sets={self.n_sets}")
        if agent_weight is not None and (agent_weight.numel() != n_agents or agent_weight.dtype != torch.float32
                                         or not agent_weight.is_contiguous()):
            raise _hip.AvdError(f"set learner: agent_weight must be contiguous float32 [{n_agents}]")

    def actor_shared(self, states_set_major, n_agents, out=None):
        """actor(state) for agents sharing this group's weight sets as one bf16 GEMM chain per set (csrc/wide.hip):
        states [n_sets, rows, S] set-major, tightly packed -> [n_sets, rows]."""
        rows = n_agents // self.n_sets
        if out is None:
            out = torch.empty(self.n_sets, rows, dtype=torch.float32, device=self.device)
        ws = self._workspace("_wide_act_ws", "avd_actor_forward_shared_workspace", n_agents)
        call("avd_actor_forward_shared_bf16", self._layp, n_agents, self.n_sets, ptr(self.theta), ptr(self.stats),
             ptr(states_set_major), self.high, ptr(out), ptr(ws), ws.numel(), stream_handle())
        return out

    def apply(self, grads, guarded=False):
        """critic Adam, actor Adam, then Polyak (workers/trainer.py:348-356) for every weight set. guarded: a set whose gradient
        slab is NaN (what the 16-bit set learners write for a non-finite input or an fp16 overflow) takes no step at all and is
        counted in ``self.nonfinite_skipped`` (device int32; no host synchronisation) -- avd_adam_polyak_guarded_f32."""
        c = self.config
        self.step += 1
        args = (self._layp, self.n_sets, ptr(self.theta), ptr(self.stats), ptr(self.theta_t), ptr(self.stats_t), ptr(self.m), ptr(self.v),
                ptr(grads), ptr(self.step))
        skipped = ()
        if guarded:
            if getattr(self, "nonfinite_skipped", None) is None:
                self.nonfinite_skipped = torch.zeros(1, dtype=torch.int32, device=self.device)
            skipped = (ptr(self.nonfinite_skipped),)
        if self.hp is not None:  # each set's step sizes and tau from the sweep table
            tbl, E, blk = self.hp
            call("avd_adam_polyak_guarded_hp_f32" if guarded else "avd_adam_polyak_hp_f32", *args, *skipped, ptr(tbl), E, blk, stream_handle())
        else:
            call("avd_adam_polyak_guarded_f32" if guarded else "avd_adam_polyak_f32", *args, self.actor_lr, c.critic_lr, float(c.tau), *skipped,
                 stream_handle())

    actor_step = None  # int32 [n_sets], the actor block's own Adam count: only a delayed-policy run has one (enable_policy_delay)

    def enable_policy_delay(self):
        """Give the group the actor block's own Adam count (``actor_step``, int32 [n_sets], zeros): what apply_delayed steps the actors
        by while ``step`` goes on counting the critic's updates. Nothing else allocates it."""
        self._no_hp("enable_policy_delay")
        if self.actor_step is None:
            self.actor_step = torch.zeros(self.n_sets, dtype=torch.int32, device=self.device)
        return self.actor_step

    def apply_delayed(self, grads, policy):
        """apply(guarded=True) under TD3's delayed policy updates (avd_adam_polyak_delayed_f32). policy false, a skipped call: the
        critic block takes its Adam step and ``step`` advances; no target moves (theta_t, stats_t) and nothing of the actor block is
        read or written -- its part of ``grads`` may hold anything. policy true: both blocks step, the critic at ``step``, the actor
        at ``actor_step`` (both advance), then the soft update of everything. A set with a non-finite gradient block takes no step,
        has its counts put back and is counted in ``self.nonfinite_skipped``."""
        self._no_hp("apply_delayed")
        self.enable_policy_delay()
        c = self.config
        self.step += 1
        if policy:
            self.actor_step += 1
        if getattr(self, "nonfinite_skipped", None) is None:
            self.nonfinite_skipped = torch.zeros(1, dtype=torch.int32, device=self.device)
        call("avd_adam_polyak_delayed_f32", self._layp, self.n_sets, ptr(self.theta), ptr(self.stats), ptr(self.theta_t), ptr(self.stats_t),
             ptr(self.m), ptr(self.v), ptr(grads), ptr(self.step), ptr(self.actor_step), 1 if policy else 0, self.actor_lr, c.critic_lr,
             float(c.tau), ptr(self.nonfinite_skipped), stream_handle())

    def learn_set_split_td(self, s, a, r, s2, n_agents, noise=None, counter=0, grads=None, losses=None, agent_weight=None, M=None, seed=None,
                           d_seeds=None):
        """The TD-only call of the split set learner (avd_learn_set_split_td_f16x3), for the calls on which the actors do not move: the
        critic block of the gradients and losses[:, 0] are learn_set_split's bit for bit -- with ``noise`` (a trainer.TargetNoise), the
        smoothed call's for the same ``counter``, ``seed`` / ``d_seeds`` and M -- while nothing of the actor's half of the chain runs:
        the actor block is all zero and losses[:, 1] is 0."""
        def tail():
            sigma, clip, key, seeds, E = 0.0, float("inf"), 0, None, 1
            if noise is not None:
                sigma, clip, key, seeds, E = self._smooth_key(noise, seed, d_seeds, "learn_set_split_td")
            c = self.config
            return (sigma, clip, float(c.action_low), float(c.action_high), key, int(counter), seeds, E, int(self.n_sets // E if M is None else M))
        return self._split_learn("avd_learn_set_split_td_f16x3", (s, a, r, s2, n_agents, agent_weight), grads, losses, "learn_set_split_td",
                                 tail)

    def apply_intra(self, grads, P, M, weights=None, lead_skip=False, lo=0, hi=None, stream=None, advance=True):
        """intrafrl + gradients (workers/trainer.py:417-431) for platoons [lo, hi): every agent of a platoon steps with the (weighted)
        mean of the platoon's M gradient rows, averaged where it is consumed (avd_adam_polyak_intra_f32: one pass over the slab;
        same values as fed_mean + fed_scatter + apply). lead_skip: intra_directional_averaging -- vehicle 0 of every platoon takes
        no step at all (:417-418). weights [P, M] or None."""
        self._no_hp("apply_intra")
        c = self.config
        hi = P if hi is None else hi
        if self.n_sets != P * M:
            raise _hip.AvdError("apply_intra needs one weight set per agent (P * M sets)")
        if advance:  # the Adam iteration counts of the agents that step (advance=False: the caller has done it for all platoons)
            if stream is None:
                self.step.view(P, M)[lo:hi, (1 if lead_skip else 0):] += 1
            else:  # (on the stream the kernel runs on: it reads the counts)
                with torch.cuda.stream(stream):
                    self.step.view(P, M)[lo:hi, (1 if lead_skip else 0):] += 1
        a, b = lo * M, hi * M
        call("avd_adam_polyak_intra_f32", self._layp, hi - lo, M, 1 if lead_skip else 0, ptr(self.theta[a:b]), ptr(self.stats[a:b]),
             ptr(self.theta_t[a:b]), ptr(self.stats_t[a:b]), ptr(self.m[a:b]), ptr(self.v[a:b]), ptr(grads[a:b]), ptr(self.step[a:b]),
             ptr(None if weights is None else weights.reshape(-1)[a:b]), self.actor_lr, c.critic_lr, float(c.tau),
             stream_handle() if stream is None else _hip.C.c_void_p(stream.cuda_stream))

    def learn_apply_intra(self, s, a, r, s2, grads, P, M, losses=None, chunks=8, weights=None, lead_skip=False, timers=None):
        """intrafrl + gradients as a two-stream pipeline over PLATOON chunks (platoons are the unit of independence: the mean never
        leaves a platoon): chunk c's learn kernel (matrix-core bound, gradients to the slab) runs on the caller's stream, its
        mean + Adam + Polyak pass (an HBM stream, apply_intra) on a side stream under chunk c + 1's learn kernel. Same results as
        learn() followed by apply_intra()."""
        chunks = max(1, min(chunks, P))
        # the iteration counts of every stepping agent, ONCE, on the caller's stream: each chunk's pass on the side stream waits for an
        # event recorded after this (one small launch per step instead of one per chunk)
        self.step.view(P, M)[:, (1 if lead_skip else 0):] += 1
        self._chunk_pipeline([(P * i) // chunks for i in range(chunks + 1)],
                             lambda lo, hi, stream: self._learn_slice(s, a, r, s2, grads, losses, lo * M, hi * M, stream),
                             lambda lo, hi, stream: self.apply_intra(grads, P, M, weights=weights, lead_skip=lead_skip, lo=lo, hi=hi,
                                                                     stream=stream, advance=False), timers)

    def learn_update(self, s, a, r, s2, grads, losses=None, next_states=None, x_stride=None, next_actions=None):
        """Fused Trainer.learn + Adam x2 + update_target for per-agent weight sets (reference nofrl,
        workers/trainer.py:325-356) in ONE kernel: every gradient is consumed where it is produced, the updated
        weights go to the alternate slab (theta ping-pong: all forward/backward passes of the step read the
        pre-update weights, trainer.py:492-506). Same result as learn() followed by apply().
        next_states [n, x_stride] + next_actions [n]: also leaves actor(next_states) of the UPDATED weights in next_actions
        (bit-identical to actor() called afterwards; saves that launch's re-read of every actor from HBM)."""
        n = self.n_sets
        if s.shape[0] != n:
            raise _hip.AvdError("learn_update needs one weight set per agent (set_mod == 0)")
        if getattr(self, "theta_alt", None) is None:
            self.theta_alt = self.theta.clone()  # alignment padding stays zero in both slabs
        c = self.config
        self.step += 1
        hp = self.hp is not None  # each agent's gamma, step sizes and tau from the sweep table
        args = (self._layp, n, ptr(self.theta), ptr(self.stats), ptr(self.theta_alt), ptr(self.theta_t), ptr(self.stats_t), ptr(self.m),
                ptr(self.v), ptr(self.step), ptr(s), ptr(a), ptr(r), ptr(s2))
        args += (self.high,) if hp else (c.gamma, self.high, self.actor_lr, c.critic_lr, float(c.tau))
        args += (ptr(grads), ptr(losses))
        fn = "avd_learn_update_hp_f32" if hp else "avd_learn_update_f32"
        if next_actions is not None:
            # + the agents' next actions actor(next_states) with the updated weights, from the workgroup that wrote them
            if self.lay.A != 1:
                raise _hip.AvdError("next-action epilogue: A == 1 only")
            xs = next_states.shape[-1] if x_stride is None else x_stride
            args += (ptr(next_states), xs, ptr(next_actions))
            fn = "avd_learn_update_act_hp_f32" if hp else "avd_learn_update_act_f32"
        if hp:
            tbl, E, blk = self.hp
            args += (ptr(tbl), E, blk)
        call(fn, *args, stream_handle())
        self.theta, self.theta_alt = self.theta_alt, self.theta

    def learn_apply(self, s, a, r, s2, grads, losses=None, chunks=4, timers=None):
        """learn + local update for per-agent weight sets (reference nofrl, workers/trainer.py:325-356).
        Agents are independent, so they are processed in `chunks` slices: the Adam/Polyak kernel of slice c
        (an HBM stream) runs on a side HIP stream underneath the learn kernel of slice c+1 (matrix-core
        bound, ~1/5 of HBM bandwidth). Results are identical to learn() followed by apply().
        timers: optional dict of lists collecting (start, end) event pairs per kernel ("learn", "update")."""
        self._no_hp("learn_apply")
        n = self.n_sets
        if s.shape[0] != n:
            raise _hip.AvdError("learn_apply needs one weight set per agent (set_mod == 0)")
        c = self.config
        self.step += 1
        chunks = max(1, min(chunks, n))

        def update(lo, hi, stream):
            call("avd_adam_polyak_f32", self._layp, hi - lo, ptr(self.theta[lo:hi]), ptr(self.stats[lo:hi]), ptr(self.theta_t[lo:hi]),
                 ptr(self.stats_t[lo:hi]), ptr(self.m[lo:hi]), ptr(self.v[lo:hi]), ptr(grads[lo:hi]), ptr(self.step[lo:hi]), self.actor_lr,
                 c.critic_lr, float(c.tau), _hip.C.c_void_p(stream.cuda_stream))

        self._chunk_pipeline([(n * i) // chunks for i in range(chunks + 1)],
                             lambda lo, hi, stream: self._learn_slice(s, a, r, s2, grads, losses, lo, hi, stream), update, timers)

    def _learn_slice(self, s, a, r, s2, grads, losses, lo, hi, stream):
        """avd_learn_f32 of the agents [lo, hi), each with its own weight set, on `stream`."""
        call("avd_learn_f32", self._layp, hi - lo, 0, ptr(self.theta[lo:hi]), ptr(self.stats[lo:hi]), ptr(self.theta_t[lo:hi]),
             ptr(self.stats_t[lo:hi]), ptr(s[lo:hi]), ptr(a[lo:hi]), ptr(r[lo:hi]), ptr(s2[lo:hi]), self.config.gamma, self.high,
             ptr(grads[lo:hi]), ptr(losses[lo:hi]) if losses is not None else None, _hip.C.c_void_p(stream.cuda_stream))

    def _chunk_pipeline(self, bounds, learn, update, timers):
        """The two-stream pipeline of learn_apply / learn_apply_intra over the slices [bounds[i], bounds[i + 1]): learn(lo, hi, stream) on
        the caller's stream, update(lo, hi, stream) on the side stream once that slice's learn has finished -- under the next slice's
        learn -- and the caller's stream joined to the side stream at the end.
        timers: optional dict of lists collecting (start, end) event pairs per kernel ("learn", "update")."""
        main = torch.cuda.current_stream()
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream(device=self.device)
        side = self._side
        T = lambda: torch.cuda.Event(enable_timing=timers is not None)
        for lo, hi in zip(bounds, bounds[1:]):
            if hi == lo:
                continue
            t0, t1 = T(), T()
            if timers is not None:
                t0.record(main)
            learn(lo, hi, main)
            t1.record(main)
            side.wait_event(t1)
            u0, u1 = T(), T()
            if timers is not None:
                u0.record(side)
            update(lo, hi, side)
            if timers is not None:
                u1.record(side)
                timers.setdefault("learn", []).append((t0, t1))
                timers.setdefault("update", []).append((u0, u1))
        done = torch.cuda.Event()
        done.record(side)
        main.wait_event(done)

    def experiment_view(self, e, E, M, shared):
        """Experiment e's weight sets of a batch of E interleaved experiments as an AgentGroup laid out like its solo run's: per-agent
        sets -> the sets of its platoons in solo order (platoon p = sets p*M .. p*M+M-1; copied, they are strided in the batch), shared
        sets -> its M sets (a view). For saving and the evaluator; the optimiser state is not carried over."""
        import copy
        g = copy.copy(self)
        T, S = self.lay.theta_size, self.lay.stats_size
        pick = (lambda x, w: x.view(E, M, w)[e]) if shared else (lambda x, w: x.view(-1, E, M, w)[:, e].reshape(-1, w).contiguous())
        for name, w in (("theta", T), ("stats", S), ("theta_t", T), ("stats_t", S)):
            setattr(g, name, pick(getattr(self, name), w))
        g.n_sets = g.theta.shape[0]
        for name in ("m", "v", "step", "theta_alt", "hp"):  # optimiser state (and a sweep's table) stays with the batch
            setattr(g, name, None)
        return g

    # -- Keras-style weight access (host copies) ---------------------------------------------------
    def get_weights(self, set_idx, which, target=False, trainable_only=False):
        th, st = (self.theta_t, self.stats_t) if target else (self.theta, self.stats)
        return params.unpack(self.lay, th[set_idx].cpu().numpy(), st[set_idx].cpu().numpy(), which, trainable_only,
                             dims=self.dims)

    def set_weights(self, set_idx, which, weights, target=False):
        th, st = (self.theta_t, self.stats_t) if target else (self.theta, self.stats)
        h_th, h_st = th[set_idx].cpu().numpy(), st[set_idx].cpu().numpy()
        params.pack(self.lay, weights, h_th, h_st, which, dims=self.dims)
        th[set_idx].copy_(torch.from_numpy(h_th))
        st[set_idx].copy_(torch.from_numpy(h_st))

    def grads_as_lists(self, grads_row):
        """One row of a grads slab -> (critic_grad[14], actor_grad[10]) in trainable_variables order."""
        g = grads_row.cpu().numpy()
        dummy = np.zeros(self.lay.stats_size, dtype=np.float32)
        return (params.unpack(self.lay, g, dummy, "critic", trainable_only=True, dims=self.dims),
                params.unpack(self.lay, g, dummy, "actor", trainable_only=True, dims=self.dims))


def fed_mean(grads, P, M, weights=None, group=None, method="interfrl", total=None):
    """Federated average of per-agent rows grads[P*M, n] (agent id v = p*M + m)
    (reference src/server/federated.py:47-63 / :99-118).
      interfrl: mean over platoons  -> [M, n];  intrafrl: mean over a platoon's vehicles -> [P, n].
    With a torch.distributed ``group`` whose ranks each hold P platoons, interfrl's local sums are
    all-reduced (RCCL over xGMI) before the division; intrafrl never leaves the GPU."""
    n = grads.shape[-1]
    if method == "interfrl":
        n_out, n_in, so, si = M, P, 1, M
    elif method == "intrafrl":
        n_out, n_in, so, si = P, M, M, 1
    else:
        raise ValueError(method)
    out = torch.empty(n_out, n, dtype=torch.float32, device=grads.device)
    wsum = torch.empty(n_out, dtype=torch.float32, device=grads.device) if weights is not None else None
    call("avd_fed_sum_f32", n_out, n_in, so, si, n, ptr(grads), ptr(weights), ptr(out), ptr(wsum), stream_handle())
    count = float(n_in)
    if group is not None and method == "interfrl":
        from .dist import exchange_fed_sums
        count = exchange_fed_sums(out, wsum, n_in, group, total=total)  # total: cached platoon count over all ranks
    call("avd_fed_finalize_f32", n_out, n, ptr(out), count, ptr(wsum), stream_handle())
    return out


def fed_scatter(avg, dst, P, M, method="interfrl", i_begin=0):
    """Write each group's average back to its member agents' rows of dst[P*M, n]."""
    n = avg.shape[-1]
    n_out, n_in, so, si = (M, P, 1, M) if method == "interfrl" else (P, M, M, 1)
    call("avd_fed_scatter_f32", n_out, n_in, so, si, i_begin, n, ptr(avg), ptr(dst), stream_handle())
    return dst
