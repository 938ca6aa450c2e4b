"""Test infrastructure of training under leader manoeuvres (avd_step_fused_lead_f32 and its twins): which manoeuvre a platoon trains
under, restated, and the leader input the launch must write, built from pieces that exist without it -- scenarios.leader_profile rows,
the draws of avd_normal_f32 / avd_uniform_f32 with the manoeuvre's noise as their scale (tests/test_gpu_trainer.py relies on these
kernels being bit-identical to the fused step's own draw) and one float32 add."""
import numpy as np

from avddpg_amd import scenarios


def manoeuvre_of(p, n_manoeuvres, n_levels=1, E=1):
    """The manoeuvre index of platoon p (of a batch of E interleaved experiments: of its solo run's platoon index p // E): the level is
    (p // E) % n_levels, the manoeuvre the next digit, so that levels and manoeuvres cross."""
    return ((p // E) // n_levels) % n_manoeuvres


def assignment(P, n_manoeuvres, n_levels=1, E=1):
    """[(level, manoeuvre)] of the P platoons of a batch."""
    return [((p // E) % n_levels, manoeuvre_of(p, n_manoeuvres, n_levels, E)) for p in range(P)]


def profile_rows(conf, manoeuvres):
    """float32 [n, T]: scenarios.leader_profile per deterministic manoeuvre (a gaussian one's row stays 0, unread)."""
    T = int(conf.steps_per_episode)
    rows = np.zeros((len(manoeuvres), T), dtype=np.float32)
    for k, m in enumerate(manoeuvres):
        if m.profile != "gaussian":
            rows[k] = scenarios.leader_profile(m.profile, T, conf, m.amp, m.period)
    return rows


def noise_of(conf, m):
    return float((conf.reset_max_u if m.profile == "gaussian" else 0.0) if m.noise is None else m.noise)


def draws(n, scale, seed, counter, uniform):
    """float32 [n] (numpy): what avd_normal_f32 / avd_uniform_f32 write for indices 0 .. n - 1 -- the unit draw times ``scale``, rounded."""
    import torch

    from avddpg_amd._hip import call, ptr, stream_handle

    out = torch.empty(n, dtype=torch.float32, device="cuda")
    call("avd_uniform_f32" if uniform else "avd_normal_f32", n, ptr(out), float(scale), int(seed), int(counter), stream_handle())
    return out.cpu().numpy()


def expected_exog(conf, manoeuvres, P, k, seeds, counter, n_levels=1):
    """float32 [P] (numpy): the leader input of every platoon of a batch of E = len(seeds) interleaved experiments (a solo run: one
    seed) at episode steps ``k`` (int or [P], clamped to 0 .. T - 1 as the kernel clamps) and exog counter ``counter``."""
    E, T, n = len(seeds), int(conf.steps_per_episode), len(manoeuvres)
    assert P % E == 0
    uniform = conf.rand_gen == conf.uniform
    k = np.clip(np.broadcast_to(np.asarray(k, dtype=np.int64), (P,)), 0, T - 1)
    rows = profile_rows(conf, manoeuvres)
    # per (experiment, manoeuvre that uses the draw): the scaled draws of the solo run's platoons (a gaussian manoeuvre of noise 0 too:
    # its product is a signed zero)
    scaled = {(e, j): draws(P // E, noise_of(conf, m), seeds[e], counter, uniform) for e in range(E) for j, m in enumerate(manoeuvres)
              if m.profile == "gaussian" or noise_of(conf, m) != 0.0}
    out = np.zeros(P, dtype=np.float32)
    for p in range(P):
        e, q = p % E, p // E
        j = manoeuvre_of(p, n, n_levels, E)
        m = manoeuvres[j]
        if m.profile == "gaussian":
            out[p] = scaled[(e, j)][q]
        elif (e, j) in scaled:
            out[p] = np.float32(rows[j, k[p]]) + np.float32(scaled[(e, j)][q])  # one float32 add
        else:
            out[p] = rows[j, k[p]]
    return out
