"""Training loop over the HIP kernels: counterpart of reference ``workers/trainer.py``.

``VecTrainer`` reproduces the control flow of ``Trainer.run`` (:223-280), ``advance_environment``
(:282-302), ``train_all_models`` (:304-359) and the federated branches (:400-456) for P platoons at
once: all state lives in HBM, one kernel launch per stage per step, no per-platoon Python.

``Trainer`` keeps the reference's constructor / ``initialize()`` / ``run()`` / ``learn()`` names on top of
it (reporting -- CSV, plots, model files -- is out of scope of this hot path).

Weight-set regimes (the reference always holds P x M separate agents):
  * per-agent  : one weight set per (platoon, vehicle)  -- nofrl, intrafrl, and any interfrl schedule
                 in which agents can diverge between federated steps;
  * shared     : one weight set per vehicle index -- interfrl + gradients when EVERY update is a
                 federated one (fed_update_delay_steps == 1, fed_update_count == 1, no cutoff): the
                 reference's P copies then stay bit-identical (same init :121-128, same averaged
                 gradients through identical Adam states :415-425), so a single copy is exact.
"""
import logging
import math

import numpy as np
import torch

from . import vec
from ._hip import call, ptr, stream_handle

log = logging.getLogger(__name__)


# ---- schedule predicates, same names and semantics as workers/trainer.py:631-695 ------------------
def is_fed_enabled(conf):
    return (conf.fed_method == conf.interfrl or conf.fed_method == conf.intrafrl) and (conf.framework == conf.dcntrl)


def is_gradient_updates_enabled(conf):
    return conf.aggregation_method == conf.gradients


def can_share_sets(conf):
    """Whether the agents of a run may share one weight set per vehicle slot: interfrl + gradients with every step federated -- the
    only regime in which every platoon's agent m holds the same weights after every step (the set learners' regime)."""
    return (is_fed_enabled(conf) and conf.fed_method == conf.interfrl and is_gradient_updates_enabled(conf)
            and conf.fed_update_delay_steps == 1 and conf.fed_update_count == 1 and conf.fed_cutoff_ratio >= 1.0)


def is_model_weight_updates_enabled(conf):
    return conf.aggregation_method == conf.weights


def is_weighted_fed_enabled(conf, training_episode):
    return conf.weighted_average_enabled and training_episode >= conf.weighted_window


def is_valid_update_episode(conf, training_episode):
    return conf.fed_enabled and (training_episode % conf.fed_update_count) == 0 and \
        training_episode <= conf.fed_cutoff_episode


def is_valid_update_step(conf, training_step):
    return (training_step % conf.fed_update_delay_steps) == 0


def is_valid_step_for_federated_training_with_gradients(conf, training_episode, training_step):
    return is_fed_enabled(conf) and is_valid_update_episode(conf, training_episode) and \
        is_valid_update_step(conf, training_step) and is_gradient_updates_enabled(conf)


def is_valid_step_for_federated_training_with_weights(conf, training_episode, training_step):
    return is_fed_enabled(conf) and is_valid_update_episode(conf, training_episode) and \
        is_valid_update_step(conf, training_step) and is_model_weight_updates_enabled(conf)


def check_seed_batch(conf, rng, auto_reset, group, fused_step=None):
    """Why a batch of experiments (VecTrainer(seeds=...)) cannot run with these settings, raised as a ValueError -- or None. Called
    before anything is allocated or launched. A batch needs every draw keyed per experiment and nothing that couples experiments."""
    if rng != "device":
        raise ValueError("a seed batch needs rng='device': the host-RNG parity mode consumes one global np.random stream")
    if auto_reset != "platoon":
        raise ValueError("a seed batch needs per-platoon episodes (auto_reset='platoon', --episodes platoon): the reference rule "
                         "(any terminal platoon ends the episode of all) would couple the experiments")
    if conf.framework == conf.cntrl:
        raise ValueError("a seed batch needs the decentralized framework: the centralized one has no fused step and its draw "
                         "kernels have no seed table")
    if conf.fed_method == conf.intrafrl:
        raise ValueError("a seed batch covers nofrl and interfrl; intrafrl is not supported")
    if is_fed_enabled(conf) and is_model_weight_updates_enabled(conf):
        raise ValueError("a seed batch covers gradient aggregation only: weights aggregation writes one group's average into every "
                         "agent (workers/trainer.py:442-446)")
    if group is not None:
        raise ValueError("a seed batch runs on one GPU: no process group")
    if fused_step is not None and not fused_step:
        raise ValueError("a seed batch needs the fused step (its draws are keyed per experiment; the separate draw kernels are not)")


def check_sweep(conf, seeds, hparams, shared_engine=None, pipeline_chunks=1):
    """Why a hyperparameter sweep (VecTrainer(seeds=..., hparams=...)) cannot run, raised as a ValueError -- or its full rows (one dict of
    vec.HP_KEYS per experiment). Called before anything is allocated or launched; a sweep is a seed batch (check_seed_batch) whose
    learners take their scalars from a per-experiment table: the exact-f32 kernels or the split-operand set learner (fused3) at the
    reference widths."""
    from .vec import hparams_rows

    hparams = list(hparams)
    if len(hparams) != len(seeds):
        raise ValueError(f"hparams has {len(hparams)} rows for {len(seeds)} seeds: one dict per experiment")
    rows = hparams_rows(conf, hparams)
    pairs = [(int(k), tuple(r[n] for n in sorted(r))) for k, r in zip(seeds, rows)]
    if len(set(pairs)) != len(pairs):
        raise ValueError("a hyperparameter sweep lists the same (seed, hparams) experiment twice: the experiments would be identical")
    if shared_engine not in (None, "per_agent", "fused3"):
        raise ValueError(f"a hyperparameter sweep runs the per_agent and fused3 engines only; shared_engine={shared_engine!r} has no "
                         "per-experiment table")
    widths = (conf.actor_layer1_size, conf.actor_layer2_size, conf.critic_layer1_size, conf.critic_layer2_size,
              conf.critic_act_layer_size, conf.batch_size)
    if widths != (256, 128, 256, 128, 48, 64):
        raise ValueError(f"a hyperparameter sweep runs the reference widths 256/128/48 with batch 64 only, got layers {widths[:5]} and "
                         f"batch {widths[5]}")
    if int(pipeline_chunks) > 1:
        raise ValueError("a hyperparameter sweep does not run the chunked learn || update pipeline (pipeline_chunks > 1)")
    return rows


def check_train_disturb(conf, train_disturb, rng, group, fused_step=None, hparams=None):
    """Why a run cannot TRAIN under these disturbance levels (VecTrainer(train_disturb=...)), raised as a ValueError -- or the checked
    list of scenarios.Disturbance. Called before anything is allocated or launched. The observation model lives in the fused step
    (avd_step_fused_dist_f32): device RNG, decentralized agents, one GPU, no sweep."""
    from . import _hip, scenarios

    if conf.framework == conf.cntrl:
        raise ValueError("training under disturbances needs the decentralized framework: the centralized one has no fused step")
    if rng != "device":
        raise ValueError("training under disturbances needs rng='device': the observation model lives in the fused step's launch")
    if fused_step is not None and not fused_step:
        raise ValueError("training under disturbances needs the fused step (fused_step=False has no observation model)")
    if hparams is not None:
        raise ValueError("training under disturbances does not combine with a hyperparameter sweep or PBT (hparams=...)")
    if group is not None:
        raise ValueError("training under disturbances runs on one GPU: no process group")
    levels = list(train_disturb)
    if not 1 <= len(levels) <= _hip.AVD_TRAIN_MAX_LEVELS:
        raise ValueError(f"train_disturb lists {len(levels)} levels: 1 to {_hip.AVD_TRAIN_MAX_LEVELS} (platoon p trains under level p % n_levels)")
    return scenarios.check_disturbances(levels, conf)


def check_train_leader(conf, train_leader, rng, group, auto_reset, fused_step=None, hparams=None):
    """Why a run cannot TRAIN under these leader manoeuvres (VecTrainer(train_leader=...)), raised as a ValueError -- or the checked list
    of scenarios.Manoeuvre. Called before anything is allocated or launched. The manoeuvre is read in the fused step's launch
    (avd_step_fused_lead_f32) at the step of the platoon's own episode: device RNG, decentralized agents, one GPU, no sweep, and an
    episode rule under which the host or the device holds that step."""
    from . import scenarios

    if conf.framework == conf.cntrl:
        raise ValueError("training under leader manoeuvres needs the decentralized framework: the centralized one has no fused step")
    if rng != "device":
        raise ValueError("training under leader manoeuvres needs rng='device': the manoeuvre is read in the fused step's launch")
    if fused_step is not None and not fused_step:
        raise ValueError("training under leader manoeuvres needs the fused step (fused_step=False draws the leader input in a kernel of its own)")
    if hparams is not None:
        raise ValueError("training under leader manoeuvres does not combine with a hyperparameter sweep or PBT (hparams=...)")
    if group is not None:
        raise ValueError("training under leader manoeuvres runs on one GPU: no process group")
    if auto_reset is True:
        raise ValueError("training under leader manoeuvres needs auto_reset='platoon' or False: with auto_reset=True the conditional reset "
                         "happens on the device, so neither side holds the episode's step")
    out = scenarios.check_manoeuvres(train_leader)
    scenarios.check_knobs(conf.steps_per_episode, None, scenarios.DEFAULT_PERIOD)
    return out


def check_residual(conf, residual, rng, world_size=1, fused_step=None, hparams=None):
    """Why a run cannot train its actors as a RESIDUAL on this linear law (VecTrainer(residual=...)), raised as a ValueError -- or the
    checked scenarios.ResidualLaw. Called before anything is allocated or launched. The law sits in the fused step's launch
    (avd_step_fused_res_f32): device RNG, decentralized agents, one rank, no sweep."""
    from . import scenarios

    if conf.framework == conf.cntrl:
        raise ValueError("a residual policy needs the decentralized framework: a linear law is per vehicle and the centralized framework "
                         "has no fused step")
    if rng != "device":
        raise ValueError("a residual policy needs rng='device': the law is applied in the fused step's launch")
    if fused_step is not None and not fused_step:
        raise ValueError("a residual policy needs the fused step (fused_step=False has no law in front of the plant)")
    if hparams is not None:
        raise ValueError("a residual policy does not combine with a hyperparameter sweep or PBT (hparams=...): the sweep's step has no "
                         "residual twin")
    if int(world_size) > 1:
        raise ValueError("a residual policy runs on one rank: no process group of more than one rank")
    return scenarios.check_residual(residual, conf)


def check_warm_start(conf, warm_start, rng, world_size=1, hparams=None, residual=None):
    """Why a run cannot start its actors from a fit to this linear law (VecTrainer(warm_start=...)), raised as a ValueError -- or the
    checked scenarios.WarmStart. Called before anything is allocated or launched. The fit draws on the device (avd_clone_sample_f32),
    fits one actor per vehicle, on one rank, outside any sweep; with a residual policy the law would act twice."""
    from . import scenarios

    if conf.framework == conf.cntrl:
        raise ValueError("a warm start needs the decentralized framework: a linear law is per vehicle")
    if rng != "device":
        raise ValueError("a warm start needs rng='device': the fit's states are drawn on the device")
    if residual is not None:
        raise ValueError("a warm start does not combine with a residual policy: the law would act twice")
    if hparams is not None:
        raise ValueError("a warm start does not combine with a hyperparameter sweep or PBT (hparams=...)")
    if int(world_size) > 1:
        raise ValueError("a warm start runs on one rank: no process group of more than one rank")
    return scenarios.check_warm_start(warm_start, conf)


def check_anchor(conf, anchor, shared_engine=None, world_size=1, hparams=None, overlap_allreduce=None, shared_sets=None):
    """Why a run cannot anchor its actors to this linear law while it trains (VecTrainer(anchor=...)), raised as a ValueError -- or the
    checked scenarios.Anchor. Called before anything is allocated or launched. The behaviour-cloning term sits in the split set
    learner's seed launch (avd_learn_set_split_anchor_f16x3): shared_engine='fused3', so shared-set interfrl, on one rank, in the
    single call (no overlapped exchange), outside any sweep."""
    from . import scenarios

    if conf.framework == conf.cntrl:
        raise ValueError("an anchor needs the decentralized framework: a linear law is per vehicle")
    if shared_engine != "fused3":
        raise ValueError(f"an anchor needs shared_engine='fused3' (the split set learner holds the anchored seed; the per-agent engines "
                         f"and the bf16 set learners have none), got shared_engine={shared_engine!r}")
    if not can_share_sets(conf) or (shared_sets is not None and not shared_sets):
        raise ValueError("an anchor needs shared weight sets: interfrl + gradients with every step federated (the fused3 engine's regime)")
    if hparams is not None:
        raise ValueError("an anchor does not combine with a hyperparameter sweep or PBT (hparams=...): the table-driven learn call has no "
                         "anchored form")
    if overlap_allreduce:
        raise ValueError("an anchor does not combine with overlap_allreduce: the two-phase learn call has no anchored form")
    if int(world_size) > 1:
        raise ValueError("an anchor runs on one rank: no process group of more than one rank")
    if getattr(anchor, "pending", False):
        raise ValueError(f"anchor: the word {anchor.source!r} stands for gains that have not been filled in (Anchor.with_gains)")
    return scenarios.check_anchor(anchor, conf)


def check_actor_hold(actor_hold, hparams=None):
    """Why a run cannot hold its actors still for its first ``actor_hold`` learner calls, raised as a ValueError -- or the count."""
    if isinstance(actor_hold, bool) or not isinstance(actor_hold, (int, np.integer)) or actor_hold < 0:
        raise ValueError(f"actor_hold={actor_hold!r} must be a whole number >= 0")
    if actor_hold and hparams is not None:
        raise ValueError("actor_hold does not combine with a hyperparameter sweep or PBT (hparams=...): a sweep's update reads its step "
                         "sizes from its table")
    return int(actor_hold)


class TargetNoise:
    """Target policy smoothing (TD3's): the critic's targets evaluate the target critic at
    clip(mu'(s') + clip(sigma n, -clip, clip), action_low, action_high), n ~ N(0, 1) per sampled row, instead of at mu'(s') alone.
    ``clip`` defaults to 2.5 sigma, TD3's ratio (0.5 at sigma 0.2); math.inf: no noise clip. Frozen: the fields cannot be reassigned."""
    __slots__ = ("sigma", "clip")

    def __init__(self, sigma=0.2, clip=None):
        object.__setattr__(self, "sigma", sigma)
        if clip is None:  # (sigma 0: any positive clip does, the launch is skipped; an invalid sigma is check_target_noise's to report)
            ok = isinstance(sigma, (int, float, np.integer, np.floating)) and not isinstance(sigma, bool) and math.isfinite(sigma) and sigma > 0
            clip = 2.5 * float(sigma) if ok else 1.0
        object.__setattr__(self, "clip", clip)

    def __setattr__(self, name, value):
        raise AttributeError(f"TargetNoise is frozen: cannot set {name}")

    def __delattr__(self, name):
        raise AttributeError(f"TargetNoise is frozen: cannot delete {name}")

    def __eq__(self, other):
        return isinstance(other, TargetNoise) and (self.sigma, self.clip) == (other.sigma, other.clip)

    def __hash__(self):
        return hash((self.sigma, self.clip))

    def __repr__(self):
        return f"TargetNoise(sigma={self.sigma!r}, clip={self.clip!r})"

    def record(self):
        """conf.json's target_noise, a list of pairs like Anchor.record."""
        return [["sigma", float(self.sigma)], ["clip", float(self.clip)]]

    @classmethod
    def parse(cls, text):
        """``sigma=0.2[,clip=0.5]`` -> TargetNoise. An unknown key, a key given twice, a value that is no number, an empty text or a
        text without sigma is a ValueError; the values are checked by check_target_noise."""
        kw = {}
        parts = [q.strip() for q in str(text).split(",") if q.strip()]
        for part in parts:
            key, eq, val = part.partition("=")
            key, val = key.strip(), val.strip()
            if not eq or key not in cls.__slots__:
                raise ValueError(f"target noise: unknown key {key!r} (sigma=..[,clip=..], as key=value)")
            if key in kw:
                raise ValueError(f"target noise: {key} given twice")
            try:
                kw[key] = float(val)
            except ValueError:
                raise ValueError(f"target noise: {key}={val!r} is not a number") from None
        if "sigma" not in kw:
            raise ValueError(f"target noise {str(text)!r}: no sigma given (sigma=..[,clip=..])")
        return cls(**kw)


def check_target_noise(target_noise, conf=None, shared_engine="fused3", rng="device", world_size=1, hparams=None, overlap_allreduce=None,
                       shared_sets=None):
    """Why a run cannot smooth its target policy with this noise (VecTrainer(target_noise=...)), raised as a ValueError -- or the checked
    TargetNoise. Called before anything is allocated or launched. The smoothing launch sits in the split set learner's chain
    (avd_learn_set_split_smooth_f16x3): shared_engine='fused3', so shared-set interfrl, on one rank, in the single call (no overlapped
    exchange), outside any sweep, with the device's generator. Without ``conf`` the values alone are checked."""
    tn = target_noise
    if not isinstance(tn, TargetNoise):
        raise ValueError(f"{tn!r} is not a trainer.TargetNoise")
    number = lambda x: isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool)
    if not number(tn.sigma) or not math.isfinite(tn.sigma) or not tn.sigma >= 0:
        raise ValueError(f"target noise: sigma={tn.sigma!r} must be a finite number >= 0")
    if float(tn.sigma) > float(np.finfo(np.float32).max):
        raise ValueError(f"target noise: sigma={tn.sigma!r} does not fit float32")
    if not number(tn.clip) or not tn.clip > 0:  # (a NaN fails the comparison; math.inf: no noise clip)
        raise ValueError(f"target noise: clip={tn.clip!r} must be a number > 0 (inf: no clip)")
    if math.isfinite(tn.clip) and float(np.float32(tn.clip)) == 0.0:
        raise ValueError(f"target noise: clip={tn.clip!r} rounds to 0 in float32")
    if shared_engine != "fused3":
        raise ValueError(f"target noise needs shared_engine='fused3' (the split set learner holds the smoothing launch; the per-agent "
                         f"engines and the bf16 set learners have none), got shared_engine={shared_engine!r}")
    if rng != "device":
        raise ValueError(f"target noise needs rng='device' (the noise is drawn by the device's counter-based generator), got rng={rng!r}")
    if hparams is not None:
        raise ValueError("target noise does not combine with a hyperparameter sweep or PBT (hparams=...): the table-driven learn call has "
                         "no smoothed form")
    if overlap_allreduce:
        raise ValueError("target noise does not combine with overlap_allreduce: the two-phase learn call has no smoothed form")
    if int(world_size) > 1:
        raise ValueError("target noise runs on one rank: no process group of more than one rank")
    if conf is not None:
        if conf.framework == conf.cntrl:
            raise ValueError("target noise needs the decentralized framework (the split set learner's)")
        if not can_share_sets(conf) or (shared_sets is not None and not shared_sets):
            raise ValueError("target noise needs shared weight sets: interfrl + gradients with every step federated (the fused3 engine's "
                             "regime)")
    return tn


def is_policy_call(call, policy_delay):
    """Whether learner call ``call`` (0-based) of a run with this delay moves the actors and the targets: every policy_delay-th call,
    the policy_delay-th first (TD3's delayed policy updates). No delay (None): every call."""
    return policy_delay is None or (int(call) + 1) % int(policy_delay) == 0


def check_policy_delay(policy_delay, conf=None, shared_engine="fused3", rng="device", world_size=1, hparams=None, overlap_allreduce=None,
                       shared_sets=None, steps=None):
    """Why a run cannot delay its policy updates by ``policy_delay`` (VecTrainer(policy_delay=...)), raised as a ValueError -- or the
    checked delay, an int >= 1. Called before anything is allocated or launched. The skipped calls run the split set learner's TD-only
    call and the update with the actor's own Adam count (avd_learn_set_split_td_f16x3, avd_adam_polyak_delayed_f32): shared_engine=
    'fused3', so shared-set interfrl, on one rank, in the single call, outside any sweep, with the device's generator. ``steps``: the
    run's step count where the caller knows it -- a delay at or above it, or (with ``conf``) above the steps - batch_size learner calls
    the run makes past the replay gate, would never move the actors. Without ``conf`` the value
    alone is checked."""
    d = policy_delay
    if isinstance(d, bool) or not isinstance(d, (int, np.integer)):
        raise ValueError(f"policy delay: policy_delay={d!r} must be a whole number >= 1")
    if d < 1:
        raise ValueError(f"policy delay: policy_delay={d!r} must be >= 1")
    if steps is not None and d >= int(steps):
        raise ValueError(f"policy delay: policy_delay={d} is not below the run's {int(steps)} steps: the actors would never move")
    if steps is not None and conf is not None and d > int(steps) - int(conf.batch_size):
        # (the replay gate: the first learner call is the step after batch_size rows are in, so a run makes steps - batch_size calls)
        raise ValueError(f"policy delay: policy_delay={d} is above the {max(0, int(steps) - int(conf.batch_size))} learner calls that "
                         f"{int(steps)} steps make past the replay gate ({int(conf.batch_size)} rows): the actors would never move")
    if shared_engine != "fused3":
        raise ValueError(f"policy delay needs shared_engine='fused3' (the split set learner holds the TD-only call; the per-agent engines "
                         f"and the bf16 set learners have none), got shared_engine={shared_engine!r}")
    if rng != "device":
        raise ValueError(f"policy delay needs rng='device' (the fused3 engine's device-side run), got rng={rng!r}")
    if hparams is not None:
        raise ValueError("policy delay does not combine with a hyperparameter sweep or PBT (hparams=...): the experiment copy and the "
                         "table-driven update know one Adam count per weight set")
    if overlap_allreduce:
        raise ValueError("policy delay does not combine with overlap_allreduce: the two-phase learn call has no TD-only form")
    if int(world_size) > 1:
        raise ValueError("policy delay runs on one rank: no process group of more than one rank")
    if conf is not None:
        if conf.framework == conf.cntrl:
            raise ValueError("policy delay needs the decentralized framework (the split set learner's)")
        if not can_share_sets(conf) or (shared_sets is not None and not shared_sets):
            raise ValueError("policy delay needs shared weight sets: interfrl + gradients with every step federated (the fused3 engine's "
                             "regime)")
    return int(d)


def check_keep_best(world_size):
    """Why a run cannot keep the best actors seen (VecTrainer.enable_keep_best), raised as a ValueError -- or None. Called before
    anything is allocated or launched."""
    if int(world_size) > 1:
        raise ValueError("keeping the best actors runs on one rank: nothing is gathered across a process group of more than one rank")


def sequential_mean_f32(x):
    """The retention score of csrc/best.hip on the host: the float32 sum of x in memory order, from the first element, one add at a
    time, divided by float32(len(x)) (np.average / np.sum add pairwise from 8 elements on)."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    s = x[0]
    with np.errstate(all="ignore"):  # (an infinite or NaN counter is a score like any other)
        for v in x[1:]:
            s = np.float32(s + v)
        return np.float32(s / np.float32(x.size))


# The set learners' largest weight-set count (the shape checks of csrc/fset.hip and csrc/fsplit.hip); the others take any count.
SET_ENGINE_MAX_SETS = {"fused": 64, "fused3": 64}


class VecTrainer:
    def __init__(self, conf, device=None, rng="device", group=None, shared_sets=None, seed=None, auto_reset=False,
                 pipeline_chunks=1, fused_update=False, shared_engine=None, init_seed=None, fused_step=None,
                 replay_ring=None, overlap_allreduce=None, seeds=None, hparams=None, train_disturb=None, train_leader=None,
                 residual=None, warm_start=None, actor_hold=0, anchor=None, target_noise=None, policy_delay=None):
        """group: torch.distributed process group whose ranks each hold ``conf.num_platoons`` platoons
        (interfrl gradients are all-reduced over it). auto_reset: end episodes on the device (no host
        sync per step); needs rng='device'. True: the reference's rule -- any terminal platoon (or the step limit) ends
        the episode of ALL platoons (workers/trainer.py:268-269). "platoon": every platoon runs its own episodes
        (vec.VecPlatoon.episode_end: closed on its own terminal step or at its own step limit, episodic rewards kept as
        per-platoon running sums in ``env.ep_stats``) -- the vectorised-environment form for thousands of platoons, where
        the any-terminal rule cuts every episode to the first terminal among them.
        seed: this rank's env / noise / replay stream seed (give every rank its own). init_seed: seed of the initial
        weights, ``conf.random_seed`` by default -- rank-INVARIANT: every agent on every rank starts from the same
        weights (workers/trainer.py:121-131); with a group they are broadcast from rank 0 as well.
        seeds: a BATCH of len(seeds) = E independent experiments in one launch chain (exclusive with seed / init_seed): experiment e is
        what VecTrainer(seed=seeds[e], init_seed=seeds[e]) computes alone (``python -m avddpg_amd tr --seed seeds[e]``), bit for bit
        wherever no set learner reduces over platoons (nofrl, interfrl per_agent). Its conf.num_platoons platoons are interleaved with
        the others': experiment e's platoon p is platoon p * E + e of the batch (self.P = E * conf.num_platoons), agent
        (e, p, m) = (p * E + e) * M + m; shared weight sets: experiment e owns sets e*M .. e*M+M-1. check_seed_batch says what a batch
        needs (device RNG, per-platoon episodes, decentralized nofrl / interfrl with gradients, one GPU).
        hparams: a hyperparameter SWEEP (needs seeds): one dict per experiment, keys a subset of vec.HP_KEYS (actor_lr, critic_lr,
        tau, gamma, std_dev, theta; a missing key takes conf's value). Experiment e is then what VecTrainer(Config(**hparams[e]),
        seed=seeds[e], init_seed=seeds[e]) computes alone, bit for bit, wherever a seed batch is; a seed may repeat when its rows
        differ (fused3: experiment e equals a seed batch of the same seeds whose conf holds row e's values -- its reduction tree depends on
        the set count). check_sweep says what else a sweep needs (the per_agent or fused3 engine, the reference widths, no
        pipeline_chunks).
        train_disturb: a list of 1..16 scenarios.Disturbance levels to TRAIN under (domain randomisation; the evaluator's observation
        model, see evaluate_robustness): platoon p runs under level p % n_levels for the whole run (a seed batch: the level of its solo
        run's platoon index, so experiment k still equals its solo run) -- a Disturbance with a name alone is a clean share. The true state
        advances with the level's plant and gives reward, terminal flags and episodes; the actors act from, and the replay holds, what
        the agents OBSERVED (env.obs: sensor noise, V2V delay and loss). check_train_disturb says what it needs (device RNG, the fused
        step, decentralized, one GPU, no sweep). None: nothing changes -- no buffer is made, the same entry points run.
        train_leader: a list of 1..16 scenarios.Manoeuvre to TRAIN under: platoon p's leader follows manoeuvre (q // n_levels) %
        n_manoeuvres for the whole run, q its solo-run platoon index and n_levels the train_disturb level count (1 without), so levels
        and manoeuvres cross. The input at step k of the platoon's OWN episode is scenarios.manoeuvre_table's row at k -- the array the
        scenario evaluator feeds -- plus the manoeuvre's noise times the step's unit draw; a gaussian manoeuvre is the reference's input, the
        clean share. k is env.ep_len with per-platoon episodes, self.ep_step under the host episode loop (auto_reset=False).
        check_train_leader says what it needs. None: nothing changes -- no buffer is made, the same entry points run.
        residual: a scenarios.ResidualLaw the actors are trained as a correction to (residual policy learning): the plant, the reward's
        control term and the value chained to the follower take u = clip(law(what the agent observes) + scale * r), r the agent's
        noisy clipped action; self.actions and the replay keep r, so no learner changes, and self.applied holds u. The step runs
        avd_step_fused_res_f32 (with seeds, train_disturb and train_leader as given) and every evaluation this trainer makes passes
        the law. check_residual says what it needs. None: nothing changes -- no buffer is made, the same entry points run.
        warm_start: a scenarios.WarmStart the actors are fitted to before the first step (imitation pre-training; AgentGroup.clone_fit):
        fit_warm_start() runs the fit -- once; the first step() runs it if nobody has -- and is refused once an update has been made.
        check_warm_start says what it needs. None: nothing is allocated, neither entry point of the fit is called.
        actor_hold: N > 0 holds the actors still for the first N learner calls (the steps past the replay gate): the actor's step size
        handed to the update is 0 for them (AgentGroup.actor_lr), the configuration's afterwards. No kernel changes: w - 0 * x = w keeps
        the actor's bits, and the actor's Adam moments and iteration count keep accumulating under the hold. The critic learns to
        evaluate the policy it was handed; every engine and framework that does not read its step sizes from a sweep table. 0: the
        configuration's step size is passed as always.
        anchor: a scenarios.Anchor the actor loss is tied to while training (TD3+BC's behaviour-cloning term): every learner call runs
        avd_learn_set_split_anchor_f16x3 with the weight Anchor.weight_at(call) -- also once a decay has brought it to 0, so that
        anchor_losses() (the last call's mean (mu - u*)^2 per weight set, on the device) stays a diagnostic. With a seed batch every
        experiment gets the same table (set e * M + m uses row m); with a residual policy the law is the target of the correction.
        check_anchor says what it needs (shared_engine='fused3', one rank, no sweep, no overlapped exchange). None: nothing is allocated,
        the un-anchored entry point runs.
        target_noise: a TargetNoise -- target policy smoothing (TD3's): every learner call runs avd_learn_set_split_smooth_f16x3, whose
        critic targets evaluate the target critic at clip(mu'(s') + clip(sigma n, -clip, clip), action_low, action_high). The noise is
        keyed by the run's seed (under seeds= by each experiment's: experiment e draws what its solo run draws) and the 0-based
        learner-call count. With anchor= the gains, weight_at(call) and the loss buffer travel in the same call. check_target_noise says
        what it needs (shared_engine='fused3', rng='device', one rank, no sweep, no overlapped exchange). None: nothing is allocated,
        today's entry points run.
        policy_delay: d >= 1 -- TD3's delayed policy updates: learner call k (0-based) is a POLICY call iff (k + 1) % d == 0
        (is_policy_call). A policy call runs the learn call of the run (plain, anchored or smoothed) and AgentGroup.apply_delayed(policy=
        True): both nets step, every target follows. Every other call runs the TD-only call (AgentGroup.learn_set_split_td, with the
        run's target_noise) and apply_delayed(policy=False): the critic alone steps, no target moves, nothing of the actor is computed,
        read or written. The critic's Adam count is agents.step, the actors' own agents.actor_step. The smoothing counter and the
        anchor's weight ramp go on counting learner calls; the anchor acts on policy calls only; actor_hold passes step size 0 on the
        policy calls inside the hold. d = 1 trains bit for bit what None trains, through the new update entry. check_policy_delay says
        what it needs (as target_noise). None: nothing is allocated, today's entry points run."""
        conf.refresh()
        def ranks():  # of `group`; asked for where a check needs them, so that a group refused before that is never asked
            if group is None:
                return 1
            import torch.distributed as _td
            return _td.get_world_size(group)

        self.levels = self.manoeuvres = self.lead = None
        self.residual = None
        if residual is not None:
            self.residual = check_residual(conf, residual, rng, ranks(), fused_step, hparams)
        self.res_gains = self.applied = None
        self.warm_start = self.warm_start_losses = None
        if warm_start is not None:
            self.warm_start = check_warm_start(conf, warm_start, rng, ranks(), hparams, residual)
        self.actor_hold = check_actor_hold(actor_hold, hparams)
        self.anchor = self.anchor_gains = self.anchor_loss = self.anchor_loss_first = self.anchor_weight = None
        if anchor is not None:
            self.anchor = check_anchor(conf, anchor, shared_engine, ranks(), hparams, overlap_allreduce, shared_sets)
        self.target_noise = None
        if target_noise is not None:
            self.target_noise = check_target_noise(target_noise, conf, shared_engine, rng, ranks(), hparams, overlap_allreduce, shared_sets)
        self.policy_delay = None
        if policy_delay is not None:
            self.policy_delay = check_policy_delay(policy_delay, conf, shared_engine, rng, ranks(), hparams, overlap_allreduce, shared_sets)
        self.policy_call = True  # whether the last learner call moved the actors and the targets (always, without a delay)
        self.learner_calls = 0  # steps that passed the replay gate (what actor_hold counts)
        if train_disturb is not None:
            self.levels = check_train_disturb(conf, train_disturb, rng, group, fused_step, hparams)
        if train_leader is not None:
            self.manoeuvres = check_train_leader(conf, train_leader, rng, group, auto_reset, fused_step, hparams)
        self.conf, self.rng, self.group = conf, rng, group
        self.device = torch.device(device if device is not None else "cuda")
        self.seeds = self.hp_rows = None
        if hparams is not None and seeds is None:
            raise ValueError("hparams= needs seeds= (one seed per experiment of the sweep)")
        if seeds is not None:
            if seed is not None or init_seed is not None:
                raise ValueError("seeds= is mutually exclusive with seed= / init_seed=")
            self.seeds = vec.seed_table(seeds, "cpu", distinct=hparams is None)[0]
            check_seed_batch(conf, rng, auto_reset, group, fused_step)
            if hparams is not None:
                self.hp_rows = check_sweep(conf, self.seeds, hparams, shared_engine, pipeline_chunks)
        distinct = self.hp_rows is None
        self.E = 1 if self.seeds is None else len(self.seeds)
        self.P, self.L = conf.num_platoons * self.E, conf.pl_size
        self.P_exp = conf.num_platoons  # platoons per experiment
        seed = (conf.random_seed if seed is None else seed) if self.seeds is None else None
        self.env = vec.VecPlatoon(self.P, self.L, conf, self.device, rand_states=conf.rand_states, rng=rng, seed=seed or 0,
                                  seeds=self.seeds, distinct_seeds=distinct, train_disturb=self.levels)
        # models per platoon: L decentralized, 1 centralized (environment.py:35-42). The reference trainer iterates
        # conf.pl_size models (trainer.py:45) and therefore only completes a centralized step when pl_size == 1; for
        # pl_size > 1 this follows the loop shape of its evaluator (workers/evaluator.py:48-91: env.num_models).
        self.centralized = conf.framework == conf.cntrl
        self.M = self.env.num_models
        self.S, self.A = self.env.num_states, self.env.num_actions
        if self.centralized and conf.model == conf.modelA and self.L > 1:
            # every Vehicle is handed the platoon's num_states = 3L >= 4 and returns x[0:3L] = all 4 entries
            # (environment.py:55-63, 518): the 4L-wide observation does not fit the 3L-wide network input.
            raise ValueError("centralized + Model A with pl_size > 1: the reference's observation is 4L wide but its "
                             "network input 3L (src/environment.py:45-63, 518); not a runnable configuration")
        self.x_stride = 4 * self.L // self.M  # floats between consecutive agents' observations in env.x
        n_agents = self.P * self.M
        self.n_agents = n_agents
        self.ou = vec.VecOUNoise(n_agents, conf, self.device, rng=rng, seed=seed or 0, seeds=self.seeds, distinct_seeds=distinct)
        fed = is_fed_enabled(conf)
        can_share = can_share_sets(conf)
        self.shared = can_share if shared_sets is None else bool(shared_sets)
        if self.shared and not can_share:
            raise ValueError("shared weight sets are only exact for interfrl+gradients with every step federated")
        # the federated view [Pf, Mf]: (platoons, weight-set slots) of the per-set means -- with a seed batch the E experiments' M
        # slots side by side (agent (e, p, m) is row p, slot e*M + m), so every mean runs over one experiment's platoons only
        self.Pf, self.Mf = self.P_exp, self.E * self.M
        self.set_mod = self.Mf if self.shared else 0
        self.agents = vec.AgentGroup(self.Mf if self.shared else n_agents, self.S, self.A, conf, self.device,
                                     seed=None if self.seeds else (conf.random_seed if init_seed is None else init_seed),
                                     hidd_mult=self.env.hidden_multiplier, seeds=self.seeds, seed_block=self.M)
        if self.policy_delay is not None:  # the actors' own Adam count
            self.agents.enable_policy_delay()
        self.d_hp = None
        if self.hp_rows is not None:  # the sweep's table: agent / set j of the batch is experiment (j // M) % E
            self.d_hp = vec.hparams_table(self.hp_rows, conf.ou_dt, self.device)
            self.agents.set_hparams(self.d_hp, self.E, self.M)
        from . import dist as _dist
        _dist.broadcast_agents(self.agents, group)
        # platoons over all ranks: a constant, reduced once here (the federated mean's divisor)
        self.total_platoons = _dist.total_platoons(self.P, group, self.device)
        self.replay = vec.VecReplay(n_agents, conf.buffer_size, conf.batch_size, self.S, self.A, self.device, rng=rng,
                                    seed=seed or 0, ring=replay_ring, seeds=self.seeds, agents_per_platoon=self.M,
                                    distinct_seeds=distinct)
        f32 = dict(dtype=torch.float32, device=self.device)
        # Shared weight sets: "per_agent" = the f32 LDS-resident kernel per agent + fed_sum (exact f32, widths up to
        # 256); "batched" = one learn over each set's P x 64 rows as bf16 MFMA GEMMs (csrc/wide.hip; any width multiple
        # of 64, e.g. BASELINE config 5's 1024); "fused" = the same quantity at the reference widths as persistent
        # register-resident-weight kernels (csrc/fset.hip; bf16 operands, deterministic, agent-major batches); "fused3" =
        # that design with every GEMM operand an exact bf16 hi + lo pair (csrc/fsplit.hip): f32-class results.
        # Default: per_agent where it exists.
        lay = self.agents.lay
        fits = lay.H2 <= 256
        self.shared_engine = shared_engine or ("batched" if (self.shared and not fits) else "per_agent")
        if self.shared_engine not in ("per_agent", "batched", "fused", "fused3"):
            raise ValueError(f"shared_engine={shared_engine!r}")
        if self.shared_engine in ("batched", "fused", "fused3") and not self.shared:
            raise ValueError("the batched learners need shared weight sets (interfrl + gradients, every step federated)")
        if self.shared_engine in ("fused", "fused3") and (lay.H1, lay.H2, lay.Ha, lay.A, lay.B) != (256, 128, 48, 1, 64):
            raise ValueError("shared_engine='fused' / 'fused3' (csrc/fset.hip, fsplit.hip) serve the reference widths 256/128/48, A = 1, batch 64 only; "
                             f"got {lay.H1}/{lay.H2}/{lay.Ha}, A = {lay.A}, batch {lay.B}: use shared_engine='batched'")
        if self.seeds is not None and self.shared and self.Mf > SET_ENGINE_MAX_SETS.get(self.shared_engine, self.Mf):
            raise ValueError(f"a seed batch of {self.E} experiments x {self.M} weight sets needs {self.Mf} sets; shared_engine="
                             f"{self.shared_engine!r} takes at most {SET_ENGINE_MAX_SETS[self.shared_engine]}")
        if self.shared_engine == "per_agent":
            # avd_learn_f32 / avd_learn_update_f32 train these networks: a shape they do not serve (centralized pl_size >= 6: the
            # 64-row tile no longer fits the LDS; H2 > 256) is refused here with their message, not at the first learn step
            call("avd_learn_check_shape", self.agents._layp)
        self.actor_out = torch.zeros(n_agents, self.A, **f32)
        self.actions = torch.zeros(self.P, self.M, self.A, **f32)  # self.actions[p][m] (trainer.py:179)
        self.leader_exog = torch.zeros(self.P, **f32)
        batched = self.shared and self.shared_engine in ("batched", "fused", "fused3")  # no per-agent gradient slab (188 GB at hidden 1024)
        self.grads = None if batched else torch.zeros(n_agents, self.agents.lay.theta_size, **f32)
        self.losses = torch.zeros(n_agents, 2, **f32)
        self.ep_reward = torch.zeros(self.P, self.M, **f32)  # float32 accumulators (trainer.py:249, 321)
        self.all_ep_reward_lists = [[[] for _ in range(self.M)] for _ in range(self.P)]
        self.all_avg_reward_lists = [[[] for _ in range(self.M)] for _ in range(self.P)]
        self.fed_weights = None
        self.exog_calls = 0
        self.seed = seed
        if auto_reset not in (False, True, "platoon"):
            raise ValueError(f"auto_reset={auto_reset!r}: False, True (any-terminal, all platoons) or 'platoon'")
        self.auto_reset = auto_reset
        if auto_reset and rng != "device":
            raise ValueError("auto_reset needs rng='device'")
        # Weighted federated averaging with the episode bookkeeping on the device (r06): the weights |1 / mean(last
        # `weighted_window` episodic rewards)| (trainer.py:385-398) come from a device ring of closed-episode rewards
        # (avd_fed_history_push_f32, filled where episodes close) through avd_fed_weights_f32, once per step, no host synchronisation.
        # Enabled like the reference (`training_episode >= weighted_window`, :694): under the all-platoons episode rule when every
        # platoon has closed `weighted_window` episodes (all counts ARE the episode number); with per-platoon episodes from step
        # weighted_window x steps_per_episode on, when every platoon has surely closed that many (a host-known moment, the same on
        # every rank).
        self._dev_weighted = bool(auto_reset and fed and conf.weighted_average_enabled)
        if self._dev_weighted:
            W = int(conf.weighted_window)
            self._hist_ring = torch.zeros(n_agents, W, **f32)
            self._hist_cnt = torch.zeros(self.P, dtype=torch.int32, device=self.device)
            self._w_raw, self._aw = torch.ones(n_agents, **f32), torch.ones(n_agents, **f32)
            self._wsum = torch.full((self.Mf,), float(self.Pf), **f32)
        self.steps_total = 0  # training steps since construction (per-platoon episodes: the schedule's episode-equivalent clock)
        # fused_step: OU noise, policy clip, leader exog, platoon step, replay add and the reward counters in ONE launch
        # (avd_step_fused_f32; bit-identical to the separate kernels). Device-RNG mode, decentralized agents. Default: on
        # where it applies.
        can_fuse_step = rng == "device" and not self.centralized and self.A == 1 and self.S in (3, 4)
        self.fused_step = can_fuse_step if fused_step is None else bool(fused_step)
        if self.fused_step and not can_fuse_step:
            raise ValueError("fused_step needs rng='device' and the decentralized framework")
        # shared sets at the reference widths with a set learner: act on the f32 matrix cores (csrc/act.hip) instead of the
        # batch-1 rows kernel (same values up to the f32 summation order; the rows kernel stays wherever bit-equality with
        # the per-agent weight-set regime is asserted, i.e. the per_agent engine)
        self.act_mfma = (self.shared and self.shared_engine in ("fused", "fused3")
                         and (lay.H1, lay.H2, lay.A) == (256, 128, 1) and lay.S in (3, 4))
        # overlapped exchange (two-phase learn call, critic block all-reduced on a side stream under the actor phase): OPT-IN. Measured
        # on a real RCCL communicator (one rank, r05: bench.py --one-rank-rccl) the overlapped form is SLOWER -- 2.31 ms per step against
        # 2.18, its collectives 0.53 ms against 0.014: the learn call's persistent kernels hold every CU (one workgroup each, 135-160 KB of
        # LDS), so RCCL's kernel does not run beside the actor phase but between its launches, and the fork / join costs on top. The
        # single all-reduce of the slab between learn and Adam is the default on every backend; bench.py times both forms at N > 1.
        can_overlap = group is not None and self.shared and self.shared_engine == "fused3"
        self.overlap_allreduce = False if overlap_allreduce is None else bool(overlap_allreduce)
        if self.overlap_allreduce and not can_overlap:
            raise ValueError("overlap_allreduce needs a process group and shared_engine='fused3' (the two-phase learn call)")
        self._side = None  # side stream + buffers of the overlapped exchange, made on first use
        # the exchange buffer of the shared-set learners ([M, theta] slab | flag | [M] weight sums: dist.set_exchange_buffer) and whether
        # this step's any-terminal flag has already travelled with it
        self._xbuf = None
        self._flag_exchanged = False
        self.world_size = ranks()
        self._equal_shards = abs(self.total_platoons - self.P * self.world_size) < 0.5
        self._keep = None  # retention of the best actors seen (enable_keep_best); None: nothing allocated, no entry point called
        self._step_parity = 0
        self._added = False
        if self.manoeuvres is not None:  # the manoeuvre tables, uploaded once; the episode's step per platoon exists from the start
            from . import scenarios
            table, noise, gauss = scenarios.manoeuvre_table(conf, self.manoeuvres)
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
            self.lead = dict(n=len(self.manoeuvres), T=table.shape[1], table=up(table), noise=up(noise), gaussian=up(gauss.astype(np.uint8)))
            if auto_reset == "platoon":
                self.env.ensure_episode_state()
        if self.residual is not None:  # the gain table, uploaded once; what the plant received, one float per vehicle
            if not self.fused_step:
                raise ValueError("a residual policy needs the fused step (fused_step=False has no law in front of the plant)")
            self.res_gains = torch.from_numpy(self.residual.gains(self.L)).to(self.device)
            self.applied = torch.zeros(self.P, self.L, **f32)
        if self.anchor is not None:  # the gain table, uploaded once; the per-set anchor loss of the last learner call
            self.anchor_gains = torch.from_numpy(self.anchor.gains(self.L)).to(self.device)
            self.anchor_loss = torch.zeros(self.Mf, **f32)
        self.fused_update = bool(fused_update)  # nofrl (any framework / widths the learn kernels serve): avd_learn_update_f32
        # fused_update also has the learn kernel evaluate the UPDATED actor on the state the next step acts from
        # (workers/trainer.py:287-289): self.actor_out then already holds the next step's actor outputs unless the states
        # were reset in between (device flag env.any_done / a host-side reset clears _act_ready)
        self._act_ready = False
        self.pipeline_chunks = int(pipeline_chunks)  # > 1: overlap Adam/Polyak with learn across agent slices (nofrl, intrafrl + gradients)
        # intrafrl + gradients: the platoon mean formed inside the Adam pass (avd_adam_polyak_intra_f32) instead of fed_sum / finalize /
        # scatter / apply over the gradient slab (same values; False keeps the four-kernel path for cross-checks)
        self.intra_fused = True
        self.timers = None
        self.episode, self.ep_step = 0, 0
        self.updates = 0  # agent-updates (one agent's learn + Adam x2 + Polyak)
        self.env_steps = 0  # platoon-steps

    # ------------------------------------------------------------------------------------------
    def _timed(self, name, fn, *args, **kw):
        """Run fn; when self.timers is a dict, bracket it with HIP events on the launch stream."""
        if self.timers is None:
            return fn(*args, **kw)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(*args, **kw)
        e1.record()
        self.timers.setdefault(name, []).append((e0, e1))
        return out

    def reset_episode(self):
        """trainer.py:244-249"""
        self._act_ready = False  # new states: the actor outputs left by the last fused update are stale
        self.env.reset()
        self.ep_reward.zero_()
        self.ep_step = 0

    def _act_wide_shared(self, seen):
        """actor(what the agents see) -> actor_out for wide shared sets: every agent re-reading its set's megabytes of weights is the
        wrong shape; one GEMM chain per set instead (bf16 operands, like this engine's learner)."""
        P, M = self.P, self.M
        sm = seen.view(self.Pf, self.Mf, 4)[..., :self.S].transpose(0, 1).contiguous()  # set-major [M, P, S]
        o = self.agents.actor_shared(sm, P * M)
        self.actor_out.copy_(o.transpose(0, 1).reshape(P * M, 1))

    def _act(self):
        """advance_environment (trainer.py:282-302): actor -> OU noise -> clip, leader exog, env step."""
        conf, P, M = self.conf, self.P, self.M
        seen = self.env.agent_states()  # env.x, or what the agents observe of it (train_disturb)
        states = seen.view(P * M, self.x_stride)
        if self.shared and self.shared_engine == "batched" and self.agents.lay.H2 > 256:
            self._act_wide_shared(seen)
        elif self._act_ready:
            # the last fused update left actor(states) in actor_out; recompute only if the episode ended since (any platoon
            # terminal resets ALL platoons, :268-269 -- the flag of the previous step is still set at this point)
            self.agents.actor(states, self.set_mod, x_stride=self.x_stride, out=self.actor_out,
                              run_if_nonzero=self.env.any_done)
        elif self.act_mfma:
            self.agents.actor_set(states, P * M, x_stride=self.x_stride, out=self.actor_out.view(-1))
        else:
            self.agents.actor(states, self.set_mod, x_stride=self.x_stride, out=self.actor_out)
        if self.fused_step:
            self._step_fused()
            return
        if self.seeds is not None:
            vec._no_scalar_draw("VecTrainer._act (separate draw kernels)")
        if self.rng == "host":
            # reference draw order per platoon: M OU normals, then the leader exog (trainer.py:286-295)
            normals = np.empty((P, M))
            exog = np.empty(P)
            for p in range(P):
                for m in range(M):
                    normals[p, m] = np.random.normal(0, 1.0)
                exog[p] = (np.random.uniform(-conf.reset_max_u, conf.reset_max_u) if conf.rand_gen == conf.uniform
                           else np.random.normal(0, conf.reset_max_u))
            noise = self.ou(normals.reshape(-1))
            self.leader_exog.copy_(torch.from_numpy(exog.astype(np.float32)))
        else:
            noise = self.ou()
            # util.get_random_val(conf.rand_gen, reset_max_u) (trainer.py:291-295): U(-u, u) or N(0, u)
            call("avd_uniform_f32" if conf.rand_gen == conf.uniform else "avd_normal_f32", P, ptr(self.leader_exog),
                 conf.reset_max_u, self.seed, self.exog_calls, stream_handle())
            self.exog_calls += 1
        if self.A > 1:  # one scalar OU process per model, broadcast over its A actions (ddpgagent.py:22)
            noise = noise.view(-1, 1).expand(-1, self.A).contiguous()
        call("avd_policy_f32", self.n_agents * self.A, ptr(self.actor_out), ptr(noise), conf.action_low,
             conf.action_high, ptr(self.actions), stream_handle())
        self.env.any_done.zero_()
        self.env.step(self.actions.view(P, self.L), self.leader_exog)

    def _step_fused(self):
        """advance_environment (workers/trainer.py:282-302) + the replay add and reward counters of train_all_models
        (:314-321) in one launch; the host only keeps the call counters in step with the separate-kernel path."""
        conf, env, ou, rp = self.conf, self.env, self.ou, self.replay
        k = self._step_parity
        self._step_parity ^= 1
        env.any_done = env._any_flags[k:k + 1]  # this step's flag (cleared by the previous step's launch, zero at start)
        other = env._any_flags[1 - k:2 - k]
        env.x, env.x_prev = env.x_prev, env.x
        lead, tag = (), ""
        if self.lead is not None:
            # training under leader manoeuvres (the *_lead_* twins): the tables and the step of the platoon's own episode -- the device's
            # counters (per-platoon episodes), or the host loop's step for every platoon
            ld, tag = self.lead, "_lead"
            per_platoon = self.auto_reset == "platoon"
            lead = (ld["n"], ld["T"], ptr(ld["table"]), ptr(ld["noise"]), ptr(ld["gaussian"]), ptr(env.ep_len) if per_platoon else None,
                    0 if per_platoon else min(self.ep_step, ld["T"] - 1))
        dist = None
        if self.levels is not None:
            # training under disturbances (avd_step_fused_dist_f32): the level's plant, the observation of the new state with the next
            # observation counter, the replay row from the observation buffers -- which swap where x and x_prev do
            env.obs, env.obs_prev = env.obs_prev, env.obs
            env.obs_counter += 1
            dist = (len(self.levels), env.h_levels, ptr(env.d_levels), ptr(env.d_plant), ptr(env.obs_prev), ptr(env.obs),
                    ptr(env.link_hist), ptr(env.link_recv), env.obs_counter)
        # every entry point's list: head, its seed key, mid, its own tail, the stream
        head = (ptr(env.d_consts), self.P, self.L, self.S, ptr(env.x_prev), ptr(env.x), ptr(env.prev_a), ptr(env.cum_accel),
                ptr(env.reward), ptr(env.term), ptr(env.done), ptr(env.any_done), ptr(other), ptr(self.actor_out), ptr(ou.state),
                ptr(self.actions), ptr(self.leader_exog), conf.theta, ou.mean, conf.ou_dt, conf.std_dev, conf.action_low,
                conf.action_high, conf.reset_max_u, 1 if conf.rand_gen == conf.uniform else 0)
        mid = (ou.calls, self.exog_calls, ptr(rp.ring), rp.cap, rp.buffer_counter, ptr(self.ep_reward))
        grp = None if self.seeds is None else (ptr(env.d_seeds), self.E)  # a batch's seed table and its length (the *_seeds_* twins)
        key, sfx = ((self.seed,), "_f32") if grp is None else (grp, "_seeds_f32")
        if self.residual is not None:
            # a residual policy: ONE entry point for every combination (seed table or none, levels or none, manoeuvres or none)
            fn, key = "avd_step_fused_res_f32", ((self.seed,) if grp is None else (0,))
            tail = (*(grp or (None, 1)), *(dist or (0, None, None, None, None, None, None, None, 0)),
                    *(lead or (0, 0, None, None, None, None, 0)), ptr(self.res_gains), float(self.residual.scale), ptr(self.applied))
        elif dist:
            fn, tail = f"avd_step_fused_dist{tag}{sfx}", dist + lead
        elif self.d_hp is not None:  # a sweep: each platoon's OU theta and scale from its experiment's row, so no scalar theta / std_dev
            fn, tail = "avd_step_fused_hp_f32", ()
            head, key = head[:17] + (ou.mean, conf.ou_dt) + head[21:], (grp[0], ptr(self.d_hp), grp[1])
        else:  # (under manoeuvres without levels the twin also takes the level count the assignment divides by: 1)
            fn, tail = f"avd_step_fused{tag}{sfx}", (lead + (1,) if lead else ())
        call(fn, *head, *key, *mid, *tail, stream_handle())
        ou.calls += 1
        self.exog_calls += 1
        env.step_count += 1
        rp.buffer_counter += 1
        self._added = True

    def _weights_for_fed(self, ep):
        """trainer.py:385-398: w = |1 / mean(last `weighted_window` episodic rewards)| per agent."""
        w = np.empty((self.P, self.M), dtype=np.float32)
        for p in range(self.P):
            for m in range(self.M):
                hist = self.all_ep_reward_lists[p][m][-self.conf.weighted_window:]
                if not hist:
                    raise RuntimeError(f"weighted federated averaging at episode {ep} needs the episodic rewards of agent "
                                       f"({p}, {m}), but none were recorded (update_reward_list is called by run())")
                w[p, m] = abs(1 / np.mean(hist))
        if not np.all(np.isfinite(w)):
            raise FloatingPointError(f"non-finite federated weights at episode {ep} (an episodic-reward mean of 0?)")
        return torch.from_numpy(w).to(self.device)

    def _train(self, ep, i):
        """train_all_models + federated branches (trainer.py:304-359, 400-456)."""
        conf, P, M = self.conf, self.P, self.M
        env = self.env

        def replay_part():
            # centralized: the platoon reward (1/L) * sum of the vehicles' (environment.py:236, 281)
            reward = env.reward_mean.view(P, 1) if self.centralized else env.reward
            xs = self.x_stride
            if self._added:  # the fused step launch has already written the row and the reward counters
                self._added = False
            else:  # (never with train_disturb: it needs the fused step)
                self.replay.add(env.x_prev.view(P * M, xs), self.actions.view(P * M, self.A), reward.view(-1),
                                env.x.view(P * M, xs), xs)
                self.ep_reward += reward
            if not self.replay.buffer_counter > conf.batch_size:  # strict gate: first update after the 65th add (:322)
                return None
            return self.replay.sample()

        batch = self._timed("replay", replay_part)
        if batch is None:
            return
        s, a, r, s2 = batch
        fed = is_fed_enabled(conf)
        self.updates += self.n_agents
        if self.actor_hold:  # the actor's step size of this learner call: 0 under the hold, then the configuration's again
            self.agents.actor_lr = 0.0 if self.learner_calls < self.actor_hold else None
        self.learner_calls += 1
        if not fed and self.fused_update:
            # nofrl: learn + Adam x2 + Polyak of every agent in one kernel (no gradient slab round trip)
            nxt = self.A == 1 and self.auto_reset  # the episode loop's host-side resets go through reset_episode()
            self._timed("learn+update", self.agents.learn_update, s, a, r, s2, self.grads, self.losses,
                        next_states=env.agent_states().view(P * M, self.x_stride) if nxt else None, x_stride=self.x_stride,
                        next_actions=self.actor_out.view(-1) if nxt else None)
            self._act_ready = nxt
            return
        if not fed and self.pipeline_chunks > 1:
            # nofrl: every agent learns and updates locally -> software-pipeline the two kernels over agent slices
            self.agents.learn_apply(s, a, r, s2, self.grads, self.losses, chunks=self.pipeline_chunks,
                                    timers=self.timers)
            return
        if (fed and conf.fed_method == conf.intrafrl and not self.shared and self.pipeline_chunks > 1
                and is_valid_update_step(conf, i) and is_valid_step_for_federated_training_with_gradients(conf, ep, i)):
            # intrafrl + gradients, every agent stepping with its platoon's mean gradient (:417-431): learn || mean + Adam + Polyak over
            # platoon chunks on two streams (vec.AgentGroup.learn_apply_intra)
            w = self._fed_weights(ep, on_device=(P, M))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if self.timers is not None:
                e0.record()
            self.agents.learn_apply_intra(s, a, r, s2, self.grads, P, M, losses=self.losses, chunks=self.pipeline_chunks, weights=w,
                                          lead_skip=bool(conf.intra_directional_averaging), timers=self.timers)
            if self.timers is not None:
                e1.record()
                self.timers.setdefault("learn+update", []).append((e0, e1))
            return
        if self.shared and self.shared_engine in ("batched", "fused", "fused3"):
            # (on the device: self._aw / self._wsum, refreshed at the end of every step)
            self._timed("learn", self._learn_batched, s, a, r, s2, self._fed_weights(ep, on_device="device"))
            # the 16-bit set learners answer a non-finite input / an fp16 overflow with an all-NaN slab: the guarded update then
            # leaves that weight set untouched and counts the event (nonfinite_updates()) instead of poisoning it for good
            if self.policy_delay is not None:  # (fused3, checked) the critic alone on a skipped call; always guarded
                self._timed("update", self.agents.apply_delayed, self.set_grads, self.policy_call)
                return
            self._timed("update", self.agents.apply, self.set_grads, guarded=self.shared_engine in ("fused", "fused3"))
            return
        self._timed("learn", self.agents.learn, s, a, r, s2, self.set_mod, grads=self.grads, losses=self.losses)
        self._timed("update", self._update, ep, i, fed)

    def _learn_batched(self, s, a, r, s2, weights=None):
        """interfrl with every step federated, shared sets: Trainer.learn + federated mean (trainer.py:400-431) as ONE
        learn over each set's P x B rows. The sampled batch is agent-major (agent v = p*M + m); the learner wants it
        set-major. Across ranks the per-set means are combined like the per-agent path's sums (dist.exchange_fed_sums).
        (P, M) is the federated view (Pf, Mf): a seed batch's experiments are E x M sets of P_exp platoons each.)"""
        P, M, B = self.Pf, self.Mf, self.conf.batch_size
        sm = lambda x: x.view(P, M, *x.shape[1:]).transpose(0, 1).reshape(M, P * B, *x.shape[2:]).contiguous()
        if getattr(self, "set_grads", None) is None:
            from .dist import set_exchange_buffer
            self._xbuf, self.set_grads = set_exchange_buffer(M, self.agents.lay.theta_size, self.device)
            self.set_losses = torch.zeros(M, 2, dtype=torch.float32, device=self.device)
        # the reference's any-terminal rule across ranks (workers/trainer.py:268-269): with device-side episodes the rank's flag of
        # this step travels in the gradient exchange and comes back as the global one, which the conditional reset then reads
        carry = self.env.any_done if (self.group is not None and self.auto_reset is True) else None
        rw = wsum = aw_dev = None
        if isinstance(weights, str):  # device weights: the factors and the per-set sums exist already (avd_fed_weights_f32)
            aw_dev, wsum, weights = self._aw, self._wsum, None
        elif weights is not None:  # [P, M] -> factors w_p * P / sum_p w_p (federated.py:99-118)
            wsum = weights.sum(dim=0)  # [M]
        if self.shared_engine in ("fused", "fused3"):  # agent-major batches as sampled, one factor per agent
            aw = aw_dev if aw_dev is not None else (None if weights is None else (weights * (float(P) / wsum)).reshape(P * M).contiguous())
            if self.overlap_allreduce:
                self._learn_split_overlapped(s, a, r, s2, aw, wsum, carry)
                self._flag_exchanged = carry is not None
                return
            if self.anchor is not None:  # (fused3, checked) the weight of this learner call: learner_calls counts it already
                self.anchor_weight = self.anchor.weight_at(self.learner_calls - 1)
            self.policy_call = is_policy_call(self.learner_calls - 1, self.policy_delay)
            if not self.policy_call:  # (fused3, checked) a skipped call of a delayed-policy run: the critic's gradients alone
                self.agents.learn_set_split_td(s, a, r, s2, P * M, noise=self.target_noise, counter=self.learner_calls - 1,
                                               grads=self.set_grads, losses=self.set_losses, agent_weight=aw, M=self.M, seed=self.seed,
                                               d_seeds=None if self.seeds is None else self.env.d_seeds)
            elif self.target_noise is not None:  # (fused3, checked) the smoothed call; an anchor's arguments travel in it
                an = None if self.anchor is None else (self.anchor_gains, self.anchor_weight, self.anchor_loss)
                self.agents.learn_set_split_smooth(s, a, r, s2, P * M, self.target_noise, self.learner_calls - 1, anchor=an,
                                                   grads=self.set_grads, losses=self.set_losses, agent_weight=aw, M=self.M, seed=self.seed,
                                                   d_seeds=None if self.seeds is None else self.env.d_seeds)
            elif self.anchor is not None:
                self.agents.learn_set_split_anchor(s, a, r, s2, P * M, self.anchor_gains, self.anchor_weight, self.anchor_loss,
                                                   grads=self.set_grads, losses=self.set_losses, agent_weight=aw)
            else:
                self.agents.learn_set_fused(s, a, r, s2, P * M, grads=self.set_grads, losses=self.set_losses, agent_weight=aw,
                                            split=self.shared_engine == "fused3")
            if self.anchor is not None and self.learner_calls == (self.policy_delay or 1):  # the first (policy) call's, kept on the device
                self.anchor_loss_first = self.anchor_loss.clone()
        else:
            if aw_dev is not None:
                rw = aw_dev.view(P, M).transpose(0, 1).reshape(M, P, 1).expand(M, P, B).reshape(M, P * B).contiguous()
            elif weights is not None:  # per-row factors, set-major
                rw = (weights * (float(P) / wsum)).transpose(0, 1).reshape(M, P, 1).expand(M, P, B).reshape(M, P * B).contiguous()
            self.agents.learn_shared(sm(s), sm(a), sm(r), sm(s2), P * M, grads=self.set_grads, losses=self.set_losses,
                                     row_weight=rw)
        if self.group is not None:
            from .dist import exchange_set_slab
            # ONE all-reduce(sum) of [slab | flag | weight sums]; local (weighted) mean <-> sum scaling around it (one launch after it
            # when every rank holds the same number of platoons)
            self._timed("allreduce", exchange_set_slab, self._xbuf, M, self.agents.lay.theta_size, wsum, P, self.total_platoons,
                        self.group, flag=carry, equal_shards=self._equal_shards)
            self._flag_exchanged = carry is not None

    def _learn_split_overlapped(self, s, a, r, s2, aw, wsum, flag=None):
        """The split-operand learner in its two phases (avd_learn_set_split_critic / _actor) with the exchange of the critic block
        overlapped: as soon as the critic phase has written its block of the [M, theta] slab, a side stream turns it into the
        local sum and all-reduces it while the actor phase -- a third of the learn call -- still computes on the main stream; the
        actor block (with the [M] weight sums of a weighted mean riding in the same buffer) follows on the main stream, the two
        streams join, and both blocks are divided by the global platoon count / weight. The same elementwise sums as
        exchange_fed_sums on the whole slab (workers/trainer.py:400-431 averages the critic and the actor gradient lists
        independently; src/server/federated.py:47-63)."""
        from .dist import exchange_two_phase

        P, M = self.P, self.M
        lay = self.agents.lay
        A, T = lay.actor_size, lay.theta_size
        if self._side is None:
            f32 = dict(dtype=torch.float32, device=self.device)
            self._side = dict(stream=torch.cuda.Stream(device=self.device), ready=torch.cuda.Event(),
                              crit=torch.empty(M, T - A, **f32), act=torch.empty(M * A + M + 1, **f32))
        scale = float(P) if wsum is None else wsum.view(M, 1)
        learn = lambda phase: self.agents.learn_set_fused(s, a, r, s2, P * M, grads=self.set_grads, losses=self.set_losses,
                                                          agent_weight=aw, split=True, phase=phase)
        learn("critic")
        exchange_two_phase(self.set_grads, A, scale, wsum, self.total_platoons, self.group, self._side,
                           lambda: learn("actor"), timers=self.timers, flag=flag)

    def _update(self, ep, i, fed):
        conf, P, M = self.conf, self.Pf, self.Mf  # (the federated view: = P, M without a seed batch)
        if not fed or not is_valid_update_step(conf, i):
            # local update (:345-356); note the gate tests the step only, not the episode (SURVEY 8a FRL quirk)
            if self.shared:
                raise RuntimeError("local update requested in shared-set mode")
            self.agents.apply(self.grads)
            return
        weights = self._fed_weights(ep, on_device=(P, M))
        method = conf.fed_method
        if is_valid_step_for_federated_training_with_gradients(conf, ep, i):
            if method == conf.intrafrl and self.intra_fused and not self.shared:
                # the platoon's mean formed where Adam consumes it: one pass over the gradient slab (avd_adam_polyak_intra_f32)
                self.agents.apply_intra(self.grads, P, M, weights=weights, lead_skip=bool(conf.intra_directional_averaging))
                return
            avg = vec.fed_mean(self.grads, P, M, weights=weights, group=self.group, method=method,
                               total=self.total_platoons)
            if self.shared:
                self.agents.apply(avg)
            else:
                directional = method == conf.intrafrl and conf.intra_directional_averaging
                vec.fed_scatter(avg, self.grads, P, M, method)
                if directional:
                    # the lead vehicle of every platoon is skipped entirely on a federated step (:417-418): no Adam
                    # step, no soft update. Its slabs are saved and put back around the batched apply.
                    ag = self.agents
                    lead = lambda x: x.view(P, M, -1)[:, 0]
                    keep = [lead(x).clone() for x in (ag.theta, ag.theta_t, ag.stats_t, ag.m, ag.v)]
                    keep_step = ag.step.view(P, M)[:, 0].clone()
                    ag.apply(self.grads)
                    for x, k in zip((ag.theta, ag.theta_t, ag.stats_t, ag.m, ag.v), keep):
                        lead(x).copy_(k)
                    ag.step.view(P, M)[:, 0].copy_(keep_step)
                else:
                    self.agents.apply(self.grads)
        elif is_valid_step_for_federated_training_with_weights(conf, ep, i):
            # weights aggregation (:433-456): average `.weights` (trainables AND BN stats) per group, then write the
            # average of group [0] into EVERY agent's model and target (the reference indexes `[0]` of the server's
            # result, :442-446 -- for interfrl that is vehicle 0's cross-platoon average, for intrafrl platoon 0's)
            if self.shared:
                raise RuntimeError("weights aggregation needs per-agent weight sets")
            ag = self.agents
            tp = self.total_platoons
            avg_th = vec.fed_mean(ag.theta, P, M, weights=weights, group=self.group, method=method, total=tp)[0]
            avg_st = vec.fed_mean(ag.stats, P, M, weights=weights, group=self.group, method=method, total=tp)[0]
            directional = method == conf.intrafrl and conf.intra_directional_averaging
            for dst, src in ((ag.theta, avg_th), (ag.theta_t, avg_th), (ag.stats, avg_st), (ag.stats_t, avg_st)):
                view = dst.view(P, M, -1)
                (view[:, 1:] if directional else view).copy_(src.expand_as(view[:, 1:] if directional else view))
        # else: FRL on, valid step, but not a valid update episode -> no parameter update at all

    def step(self, ep=None, i=None, sync=True):
        """One iteration of the loop at trainer.py:251-271. Returns the any-terminal flag (host bool)
        when ``sync`` (parity mode); with auto_reset the episode bookkeeping stays on the device."""
        ep = self.episode if ep is None else ep
        i = self.ep_step if i is None else i
        self._flag_exchanged = False
        if self.warm_start is not None and self.warm_start_losses is None:
            self.fit_warm_start()
        self._timed("act+env", self._act)
        self._train(ep, i)
        self.env_steps += self.P
        self.ep_step += 1
        if self.group is not None and self.auto_reset is True and not self._flag_exchanged:
            # a step whose flag did not travel with a gradient exchange (the replay gate is still closed, or an engine without the
            # slab exchange): its own 1-int all-reduce(max), still without a host synchronisation
            import torch.distributed as _td
            _td.all_reduce(self.env.any_done, op=_td.ReduceOp.MAX, group=self.group)
        self.steps_total += 1
        limit = self.conf.steps_per_episode
        if self.auto_reset == "platoon":
            # per-platoon episodes: there is no global episode; the schedule predicates (fed_update_count, fed_cutoff_episode,
            # trainer.py:631-695) see the episode-EQUIVALENT clock steps / steps_per_episode -- the episode number a platoon that
            # never terminates would be in -- and the running step
            if self._dev_weighted:
                self.env.ensure_episode_state()
                self._push_history(done=self.env.done, ep_len=self.env.ep_len, limit=limit, zero_after=0)
            self.env.episode_end(self.ep_reward, self.M, limit, any_reset=self.env.any_done)
            self.episode = self.steps_total // limit
            if self._dev_weighted:
                self._refresh_weights(1 if self.steps_total >= int(self.conf.weighted_window) * limit else 0)
            return None
        if self.auto_reset:
            # any platoon terminal ends the episode for ALL platoons (:268-269); so does the step limit
            if self.ep_step >= limit:
                if self._dev_weighted:
                    self._push_history(force=1, zero_after=1)
                self.env.reset()
                self._act_ready = False
                self.ep_step = 0
                self.episode += 1
            else:
                if self._dev_weighted:
                    self._push_history(cond=self.env.any_done, zero_after=1)
                self.env.reset(cond=self.env.any_done)
            if self._dev_weighted:
                self._refresh_weights(-1)
            return None
        if not sync:
            return None
        from .dist import any_terminal
        return any_terminal(self.env.any_done, self.group)

    def _fed_weights(self, ep, on_device):
        """The federated weights [P, M] of episode ep, None for the plain mean. Kept on the device (avd_fed_weights_f32): the raw weights
        viewed as on_device = (P, M) -- all ones until the weighting is enabled: the weighted formulas then give the plain mean -- or
        on_device itself where the caller only needs to know that (a string). Otherwise the host's, computed once per episode."""
        if self._dev_weighted:
            return on_device if isinstance(on_device, str) else self._w_raw.view(*on_device)
        if is_weighted_fed_enabled(self.conf, ep):
            if self.fed_weights is None or self.fed_weights[0] != ep:
                self.fed_weights = (ep, self._weights_for_fed(ep))
            return self.fed_weights[1]
        return None

    def _push_history(self, done=None, ep_len=None, limit=0, cond=None, force=0, zero_after=0):
        """Closed-episode rewards into the device ring (avd_fed_history_push_f32), BEFORE the episode end / conditional reset."""
        call("avd_fed_history_push_f32", self.P, self.M, int(self.conf.weighted_window), ptr(self.ep_reward), ptr(done), ptr(ep_len),
             int(limit), ptr(cond), int(force), int(zero_after), ptr(self._hist_ring), ptr(self._hist_cnt), stream_handle())

    def _refresh_weights(self, host_enabled):
        """trainer.py:385-398 on the device: w, the per-set sums and the learners' per-agent factors for the NEXT step's update."""
        # the federated view [Pf, Mf] (a seed batch: each per-set sum over one experiment's platoons; hist_cnt is read only by the
        # all-platoons episode rule, host_enabled < 0, which a batch does not run)
        call("avd_fed_weights_f32", self.Pf, self.Mf, int(self.conf.weighted_window), ptr(self._hist_ring), ptr(self._hist_cnt),
             int(host_enabled), ptr(self._w_raw), ptr(self._aw), ptr(self._wsum), stream_handle())

    def nonfinite_updates(self):
        """Weight-set updates skipped because the set learner returned a NaN gradient slab (host synchronisation: call it at
        reporting points). 0 unless a state, action or reward was non-finite or beyond fp16's range."""
        n = getattr(self.agents, "nonfinite_skipped", None)
        return 0 if n is None else int(n.item())

    def update_reward_list(self, ep):
        """trainer.py:510-517 (float32 counters, trailing mean over reward_averaging_window)."""
        rew = self.ep_reward.cpu().numpy()
        for p in range(self.P):
            for m in range(self.M):
                self.all_ep_reward_lists[p][m].append(rew[p, m])
                self.all_avg_reward_lists[p][m].append(
                    np.mean(self.all_ep_reward_lists[p][m][-self.conf.reward_averaging_window:]))

    def run(self, number_of_episodes=None, keep_best_every=None):
        """trainer.py:232-273. keep_best_every (after enable_keep_best): a keep_best_update at every multiple of that many steps."""
        conf = self.conf
        every = int(keep_best_every) if keep_best_every else 0
        n = conf.number_of_episodes if number_of_episodes is None else number_of_episodes
        for ep in range(n):
            self.episode = ep
            self.reset_episode()
            for i in range(conf.steps_per_episode):
                stop = self.step(ep, i)
                if every and self.steps_total % every == 0:
                    self.keep_best_update(self.steps_total)
                if stop:
                    break
            self.update_reward_list(ep)
        return self.all_ep_reward_lists, self.all_avg_reward_lists

    def anchor_losses(self):
        """The last learner call's anchor loss per weight set -- under policy_delay the last POLICY call's: the skipped calls run no
        anchored seed --, float32 [E * M] on the device: mean over the set's sampled rows of w (mu - u*)^2, not times the weight (zeros
        before the first such call)."""
        if self.anchor is None:
            raise ValueError("anchor_losses needs VecTrainer(anchor=...)")
        return self.anchor_loss

    def fit_warm_start(self):
        """The warm start's fit (AgentGroup.clone_fit with this trainer's seed or seed table), once, before the first update: the actors
        of every platoon become the fitted ones, targets equal to them, the critics and every Adam state as constructed. Returns the
        last fit step's losses, float32 [E * M] (kept in self.warm_start_losses); one synchronisation, at the end of the fit."""
        if self.warm_start is None:
            raise ValueError("fit_warm_start needs VecTrainer(warm_start=...)")
        if self.warm_start_losses is not None:
            raise ValueError("the warm start has already been fitted: it runs once")
        if self.updates or self.learner_calls:
            raise ValueError("the warm start comes before the first update: this trainer has already made one")
        self.warm_start_losses = self.agents.clone_fit(self.warm_start, seeds=self.seeds, M=self.M, seed=self.seed)
        self._act_ready = False
        return self.warm_start_losses

    def evaluator_scores(self, platoons=None, agents=None):
        """workers/evaluator.py:145 score of the CURRENT actors of each of this rank's ``platoons`` (default: all), from one
        launch of the evaluator rollout kernel (evaluator.run_many); float32 [len(platoons)]. Shared sets: one rollout.
        A seed batch: ``platoons`` index each experiment's own platoons; float32 [E, len(platoons)], still one launch.
        agents: score this group's actors instead (laid out as self.agents: best_agents())."""
        from . import evaluator

        agents = self.agents if agents is None else agents
        if self.seeds is not None:
            E, M = self.E, self.M
            platoons = list(range(self.P_exp)) if platoons is None else list(platoons)
            if self.shared:  # one rollout per experiment, on its sets e*M .. e*M+M-1
                sc = evaluator.run_many(self.conf, agents, list(range(E)), set_mod=M, set_bases=[e * M for e in range(E)], base_law=self.residual)[0]
                return np.repeat(sc[:, :1], len(platoons), axis=1)
            glob = [vec.batch_platoon(e, p, E) for e in range(E) for p in platoons]
            return evaluator.run_many(self.conf, agents, glob, base_law=self.residual)[0][:, 0].reshape(E, len(platoons))
        platoons = list(range(self.P)) if platoons is None else list(platoons)
        if self.shared:
            sc = evaluator.run_many(self.conf, agents, [0], set_mod=self.M, base_law=self.residual)[0]
            return np.repeat(sc[:, 0], len(platoons))
        return evaluator.run_many(self.conf, agents, platoons, base_law=self.residual)[0][:, 0]

    def _evaluator_addressing(self, platoons):
        """How the scenario evaluators address this trainer's actors for ``platoons`` (default: all; a seed batch or sweep: each
        experiment's own) -> (entries, keywords, lift): the platoon entries and set_mod / set_bases keywords of evaluator.run_cases and
        its kin, and the map from a result array (first axis: the entries) to the caller's -- [P, ...], or [E, P, ...] for a seed batch
        or sweep. Shared sets: one group of rollouts (per experiment), repeated per platoon."""
        if self.seeds is not None:
            E, M = self.E, self.M
            platoons = list(range(self.P_exp)) if platoons is None else list(platoons)
            n = len(platoons)
            if self.shared:  # one group per experiment, on its sets e*M .. e*M+M-1
                return list(range(E)), dict(set_mod=M, set_bases=[e * M for e in range(E)]), lambda x: np.repeat(x[:, None], n, axis=1)
            return [vec.batch_platoon(e, p, E) for e in range(E) for p in platoons], {}, lambda x: x.reshape(E, n, *x.shape[1:])
        platoons = list(range(self.P)) if platoons is None else list(platoons)
        if self.shared:
            return [0], dict(set_mod=self.M), lambda x: np.repeat(x, len(platoons), axis=0)
        return platoons, {}, lambda x: x

    def evaluate_scenarios(self, scenarios, seeds=None, platoons=None, amp=None, period_s=10.0, agents=None):
        """The CURRENT actors of each of this rank's ``platoons`` (default: all) over leader scenarios x evaluation seeds, from one
        launch of the scenario evaluator (evaluator.run_cases): a CaseResults with scores [P, scen, seed], counters [P, scen, seed, M]
        and metrics {name: [P, scen, seed, L]}. Shared sets: one group of rollouts, repeated per platoon.
        A seed batch or sweep: ``platoons`` index each experiment's own platoons and every array gains a leading experiment axis
        ([E, P, scen, seed, ...]), still from one launch; experiment e's slice equals run_cases on experiment_agents(e)."""
        from . import evaluator

        agents = self.agents if agents is None else agents  # (or a group laid out like it: best_agents())
        entries, addr, lift = self._evaluator_addressing(platoons)
        r = evaluator.run_cases(self.conf, agents, entries, scenarios=scenarios, seeds=seeds, amp=amp, period_s=period_s,
                                base_law=self.residual, **addr)
        return evaluator.CaseResults(r.scenarios, r.seeds, r.T, lift(r.scores), lift(r.counters), {k: lift(v) for k, v in r.metrics.items()})

    def evaluate_robustness(self, scenarios, disturbances, seeds=None, platoons=None, amp=None, period_s=10.0, agents=None):
        """evaluate_scenarios under disturbances: the CURRENT actors of each of this rank's ``platoons`` over leader scenarios x
        [nominal, *disturbances] x evaluation seeds, from one launch of the disturbed scenario evaluator (evaluator.run_disturbed): a
        DisturbedResults with scores [P, scen, dist, seed], counters [P, scen, dist, seed, M] and metrics {name: [P, scen, dist, seed,
        L]}; its nominal() slice equals evaluate_scenarios. A seed batch or sweep: every array gains a leading experiment axis ([E, P,
        scen, dist, seed, ...]); experiment e's slice equals run_disturbed on experiment_agents(e)."""
        from . import evaluator

        agents = self.agents if agents is None else agents  # (or a group laid out like it: best_agents())
        entries, addr, lift = self._evaluator_addressing(platoons)
        r = evaluator.run_disturbed(self.conf, agents, entries, scenarios=scenarios, disturbances=disturbances, seeds=seeds, amp=amp,
                                    period_s=period_s, base_law=self.residual, **addr)
        return evaluator.DisturbedResults(r.scenarios, r.disturbances, r.seeds, r.T, lift(r.scores), lift(r.counters),
                                          {k: lift(v) for k, v in r.metrics.items()})

    def evaluate_frequency(self, spec, disturbances=(), seeds=None, platoons=None, agents=None):
        """The frequency response of the CURRENT actors of each of this rank's ``platoons`` (default: all): ``spec`` (a
        scenarios.FrequencySpec) over frequencies x [nominal, *disturbances] x evaluation seeds, from one launch of the frequency
        evaluator (evaluator.run_frequency; a residual policy's law in front of the plant): a FrequencyResults with spectrum [P, F,
        dist, seed, L, 10], scores [P, F, dist, seed], counters and metrics. Platoons and experiments are addressed as in
        evaluate_scenarios: a seed batch or sweep gives every array a leading experiment axis, experiment e's slice equal to
        run_frequency on experiment_agents(e)."""
        from . import evaluator

        agents = self.agents if agents is None else agents  # (or a group laid out like it: best_agents())
        entries, addr, lift = self._evaluator_addressing(platoons)
        r = evaluator.run_frequency(self.conf, agents, entries, spec, disturbances, seeds, base_law=self.residual, **addr)
        return evaluator.FrequencyResults(r.freqs_hz, r.cycles, r.W, r.T, r.disturbances, r.seeds, lift(r.spectrum), lift(r.scores),
                                          lift(r.counters), {k: lift(v) for k, v in r.metrics.items()})

    def run_simulations(self, agents=None):
        """Trainer.run_simulations (workers/trainer.py:537-550): every local platoon's evaluator score over steps_per_episode
        steps divided by re_scalar -- the values the reference appends to conf.pl_rews_for_simulations (:549). Plots and the
        second, manual_timestep_override rollout are out of scope; a multi-rank run scores its own platoons.
        A seed batch: one such list per experiment ([E][P_exp]), from one rollout launch."""
        if self.seeds is not None:
            return [[float(r / self.conf.re_scalar) for r in row] for row in self.evaluator_scores(agents=agents)]
        return [float(r / self.conf.re_scalar) for r in self.evaluator_scores(agents=agents)]

    # ---- retention of the best actors seen ---------------------------------------------------------------------------------------
    def enable_keep_best(self, seeds=None):
        """Keep, on the device, the best actors each rollout group of the evaluator has had at any keep_best_update: prepares ONE
        rollout batch over exactly the groups evaluator_scores() scores (a *unit*: a platoon's M per-agent sets -- P units; the shared M
        sets -- one unit; a seed batch: experiment e's platoon p, unit e * P_exp + p, or its M shared sets, unit e) on the evaluation
        ``seeds`` (default: conf.evaluation_seed), allocates the snapshot slabs (actor span and actor BN statistics per set, a score and
        a step per unit) and fills the snapshot with the current actors, at score -inf and step -1. The caller's global np.random state
        is restored. Refused under a process group of more than one rank (nothing is gathered across ranks)."""
        check_keep_best(getattr(self, "world_size", 1))
        import ctypes as C

        from . import evaluator

        seeds = [int(self.conf.evaluation_seed)] if seeds is None else [int(k) for k in seeds]
        ag, M, E = self.agents, self.M, self.E
        if self.seeds is not None and self.shared:
            batch = evaluator.prepare_many(self.conf, ag, list(range(E)), set_mod=M, seeds=seeds, set_bases=[e * M for e in range(E)], base_law=self.residual)
        elif self.seeds is not None:
            batch = evaluator.prepare_many(self.conf, ag, [vec.batch_platoon(e, p, E) for e in range(E) for p in range(self.P_exp)], seeds=seeds,
                                           base_law=self.residual)
        elif self.shared:
            batch = evaluator.prepare_many(self.conf, ag, [0], set_mod=M, seeds=seeds, base_law=self.residual)
        else:
            batch = evaluator.prepare_many(self.conf, ag, list(range(self.P)), seeds=seeds, base_law=self.residual)
        NS = batch.NS
        d_base = batch.set_base[::NS].contiguous()  # a rollout's base is its unit's: rollout u * NS + k
        h = [int(b) for b in d_base.cpu().tolist()]
        n_units, lay, dev = len(h), ag.lay, self.device
        rows = (d_base.long().view(-1, 1) + torch.arange(M, device=dev).view(1, -1)).reshape(-1)
        self._keep = dict(batch=batch, seeds=seeds, NS=NS, n_units=n_units, d_base=d_base, h_base=(C.c_int32 * n_units)(*h), rows=rows,
                          theta=ag.theta[rows, :lay.actor_size].contiguous(), stats=ag.stats[rows, :lay.cmms].contiguous(),
                          score=torch.full((n_units,), float("-inf"), dtype=torch.float32, device=dev),
                          step=torch.full((n_units,), -1, dtype=torch.int64, device=dev),
                          improved=torch.zeros(n_units, dtype=torch.int32, device=dev), evaluations=0)

    def keep_best_update(self, step):
        """One evaluation: the rollout launch over every unit on the CURRENT actors, then the keep launches (AgentGroup.keep_best) -- a
        unit whose score, the sequential float32 mean of its NS x M counters, is above its best so far has its actors copied into the
        snapshot and ``step`` recorded. All on the current stream, no host synchronisation; nothing of the training state is written."""
        k = self._keep
        if k is None:
            raise ValueError("keep_best_update needs enable_keep_best() first")
        k["batch"].launch()
        self.agents.keep_best(k["d_base"], k["h_base"], self.M, k["NS"], k["batch"].counters, step, k["theta"], k["stats"], k["score"],
                              k["step"], k["improved"])
        k["evaluations"] += 1

    def best_scores(self):
        """(score float32 [n_units], step int64 [n_units]) of the snapshot: each unit's best score and the step it was taken at (-inf and
        -1 before the first evaluation). Synchronises. Units as in enable_keep_best."""
        k = self._keep
        if k is None:
            raise ValueError("best_scores needs enable_keep_best() first")
        return k["score"].cpu().numpy(), k["step"].cpu().numpy()

    def last_scores(self):
        """The retention score of the LAST evaluation's actors per unit, float32 [n_units] (the same formula on the counters the last
        keep_best_update left; after an evaluation at the last step: the final actors'). Synchronises."""
        k = self._keep
        if k is None or not k["evaluations"]:
            raise ValueError("last_scores needs a keep_best_update() first")
        c = k["batch"].counters.cpu().numpy().reshape(k["n_units"], -1)
        return np.array([sequential_mean_f32(row) for row in c], dtype=np.float32)

    def best_agents(self):
        """The retained actors as an AgentGroup laid out like self.agents (a copy: what artifacts.save_agents, evaluator.run_many,
        run_cases and run_disturbed take, and experiment_view for a seed batch): its online slabs are clones of the current ones at the
        full theta_size / stats_size stride with every unit's actor blocks and actor BN statistics replaced by the snapshot's. The
        critic blocks, and the target slabs (theta_t, stats_t: the trainer's own tensors, not copies), are the FINAL ones -- critics,
        targets and optimiser state are not part of the snapshot. Built on demand, at the end of a run: it clones the online slabs."""
        import copy

        k = self._keep
        if k is None:
            raise ValueError("best_agents needs enable_keep_best() first")
        lay, g = self.agents.lay, copy.copy(self.agents)
        g.theta, g.stats = self.agents.theta.clone(), self.agents.stats.clone()
        g.theta[k["rows"], :lay.actor_size] = k["theta"]
        g.stats[k["rows"], :lay.cmms] = k["stats"]
        for name in ("m", "v", "step", "theta_alt", "hp"):  # optimiser state (and a sweep's table) stays with the trainer
            setattr(g, name, None)
        return g

    def experiment_agents(self, e):
        """Experiment e's actors / critics (a seed batch) as an AgentGroup laid out like its solo run's (vec.AgentGroup.experiment_view):
        what artifacts.save_agents and the evaluator take."""
        if self.seeds is None:
            raise ValueError("experiment_agents needs a seed batch (VecTrainer(seeds=...))")
        return self.agents.experiment_view(e, self.E, self.M, self.shared)

    def exploit(self, pairs):
        """Population-based training (a seed batch): experiment dst's learner -- every weight set's online and target weights, BN
        statistics, Adam moments and step counter -- becomes a bitwise copy of experiment src's, for every (src, dst) pair
        (AgentGroup.copy_experiments; destinations distinct and never a source). Its environment, OU state, replay ring and seed stay its
        own. The actor outputs a fused update left for the next step came from the old weights: the next step recomputes them on the
        plain actor path, which is bit-identical to that prefetch for the experiments that were not replaced."""
        if self.seeds is None:
            raise ValueError("exploit needs a seed batch (VecTrainer(seeds=...))")
        self.agents.copy_experiments(pairs, self.E, self.M)
        self._act_ready = False

    def set_hparams(self, hparams):
        """A sweep's values mid-run: one dict per experiment (keys a subset of vec.HP_KEYS, a missing key takes conf's value), validated
        by vec.hparams_rows (a repeated (seed, values) experiment is allowed here). The avd_hparams table is rewritten in place by a copy
        on the current stream, so every later launch reads the new values; experiment_conf records them."""
        if self.hp_rows is None:
            raise ValueError("set_hparams needs a hyperparameter sweep (VecTrainer(seeds=..., hparams=...))")
        hparams = list(hparams)
        if len(hparams) != self.E:
            raise ValueError(f"hparams has {len(hparams)} rows for {self.E} experiments: one dict per experiment")
        rows = vec.hparams_rows(self.conf, hparams)
        self.d_hp.copy_(vec.hparams_table(rows, self.conf.ou_dt, self.device))
        self.hp_rows = rows

    def experiment_conf(self, e):
        """Experiment e's Config (a seed batch or sweep): a copy of conf with its seed as random_seed and, in a sweep, its
        hyperparameters in the reference's own fields (actor_lr, critic_lr, tau, gamma, std_dev, theta) -- what its writers record."""
        import copy

        if self.seeds is None:
            raise ValueError("experiment_conf needs a seed batch (VecTrainer(seeds=...))")
        c = copy.copy(self.conf)
        c.random_seed = self.seeds[e]
        if self.hp_rows is not None:
            for k, v in self.hp_rows[e].items():
                setattr(c, k, v)
        return c


class Trainer:
    """Reference-shaped facade (workers/trainer.py:18-61, 223): ``Trainer(base_dir, timestamp, debug_enabled,
    conf)``, ``initialize()``, ``run()``. Host-RNG parity mode by default."""

    def __init__(self, base_dir, timestamp, debug_enabled, conf, rng="host", device=None):
        self.base_dir, self.timestamp, self.debug_enabled, self.conf = base_dir, timestamp, debug_enabled, conf
        self.rng, self.device = rng, device
        self.engine = None

    def initialize(self):
        self.conf.timestamp = str(self.timestamp)
        self.conf.fed_enabled = is_fed_enabled(self.conf)
        self.engine = VecTrainer(self.conf, device=self.device, rng=self.rng)
        self.num_models, self.num_platoons = self.engine.M, self.engine.P
        self.num_states, self.num_actions = self.engine.S, self.engine.A
        self.all_ep_reward_lists = self.engine.all_ep_reward_lists
        self.all_avg_reward_lists = self.engine.all_avg_reward_lists

    def run(self, number_of_episodes=None):
        return self.engine.run(number_of_episodes)


def learn(rbuffer, actor_model, critic_model, target_actor, target_critic, gamma=0.99):
    """``Trainer.learn`` (workers/trainer.py:472-508) on reference-shaped objects: samples ``rbuffer`` and
    returns (critic_grad[14], actor_grad[10]) as lists in ``trainable_variables`` order. Pure w.r.t. the
    model weights."""
    from . import _hip, params

    lay = actor_model.lay
    s, a, r, s2 = rbuffer.sample()
    A = lay.actor_size
    theta = torch.cat([actor_model.theta[:, :A], critic_model.theta[:, A:]], dim=1).contiguous()
    theta_t = torch.cat([target_actor.theta[:, :A], target_critic.theta[:, A:]], dim=1).contiguous()

    def stats_of(act, cri):
        st = act.stats.clone()
        st[:, lay.cmms:] = cri.stats[:, lay.cmms:]
        return st

    stats, stats_t = stats_of(actor_model, critic_model), stats_of(target_actor, target_critic)
    grads = torch.empty(1, lay.theta_size, dtype=torch.float32, device=theta.device)
    call("avd_learn_f32", _hip.C.byref(lay), 1, 1, ptr(theta), ptr(stats), ptr(theta_t), ptr(stats_t),
         ptr(s.reshape(1, lay.B, lay.S).contiguous()), ptr(a.reshape(1, lay.B, lay.A).contiguous()),
         ptr(r.reshape(1, lay.B).contiguous()), ptr(s2.reshape(1, lay.B, lay.S).contiguous()), gamma,
         actor_model.high, ptr(grads), None, stream_handle())
    g = grads[0].cpu().numpy()
    dummy = np.zeros(lay.stats_size, dtype=np.float32)
    dims = getattr(actor_model, "dims", None)
    return (params.unpack(lay, g, dummy, "critic", trainable_only=True, dims=dims),
            params.unpack(lay, g, dummy, "actor", trainable_only=True, dims=dims))


Trainer.learn = staticmethod(learn)
