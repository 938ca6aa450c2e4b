"""Test infrastructure of the linear scenario evaluator's tests: tests/disturbed_oracle.rollout's float64 loop over oracle.platoon with
the actors replaced by a static gain row per vehicle -- u = np.clip(sum of gains[m][c] * obs[c] over the first num_obs observations, low,
high), added in observation order -- behind the same observation model (sensor noise, V2V delay and loss drawn with oracle.philox, the
true plant's engine lag). Rewards, terminal flags and metrics come from the true state; ``counters`` (the per-vehicle sum of the steps'
rewards, what avd_eval_linear_f32 accumulates) rides in the traces dict."""
import dataclasses

import numpy as np

from oracle import philox, platoon
from tests.disturbed_oracle import RING, STREAM_EVAL_LINK, STREAM_EVAL_OBS, _words


def law(gains, obs, low, high):
    """One vehicle's action: the gain row on the first len(obs) observations, then np.clip."""
    z = 0.0
    for c in range(len(obs)):
        z = gains[c] * obs[c] if c == 0 else z + gains[c] * obs[c]
    return float(np.clip(z, low, high))


def rollout(ep, L, gains, leader, evaluation_seed=6, high=2.5, low=-2.5, sigma=(0.0, 0.0, 0.0), v2v_delay=0, v2v_drop=0.0, dyn_coeff=None,
            noise_seed=None):
    """-> (metrics {name: float64 [L]}, x0 float64 [L, 4], traces) as disturbed_oracle.rollout; traces also holds ``counters`` float64
    [L]. gains: [L][4] (kp, kv, ka, kf) per vehicle. ep: the NOMINAL EnvParams (start states); dyn_coeff: the true plant's (None:
    ep's). noise_seed defaults to the evaluation seed. Decentralized platoons."""
    steps = len(leader)
    gains = np.asarray(gains, dtype=np.float64).reshape(L, 4)
    noise_seed = evaluation_seed if noise_seed is None else noise_seed
    assert 0 <= v2v_delay < RING
    drop_q = int(round(float(v2v_drop) * (1 << 24)))
    plant = ep if dyn_coeff is None else dataclasses.replace(ep, dyn_coeff=dyn_coeff)
    np.random.seed(evaluation_seed)
    env = platoon.RefPlatoon(L, plant, evaluator_states=True)
    [platoon.get_random_val(ep.rand_gen, ep.reset_max_u, std_dev=ep.reset_max_u) for _ in range(steps)]  # (the draws the profile replaces)
    env.reset()
    x0 = np.array([np.asarray(f.x, dtype=np.float64).copy() for f in env.followers])
    hist = [[x0[i, 3]] * RING for i in range(L)]  # hist[i][j & 15] = the true w at step j; x0's before the first
    recv = [x0[i, 3] for i in range(L)]
    mx = np.zeros((3, L))
    su2, sj2, nterm, first, counters = np.zeros(L), np.zeros(L), np.zeros(L), np.full(L, -1.0), np.zeros(L)
    S, U, J = [], [], []
    for k in range(steps):
        acts = np.zeros(L)
        for m, f in enumerate(env.followers):
            obs = np.asarray(f.x, dtype=np.float64).copy()
            hist[m][k % RING] = obs[3]
            delayed = hist[m][(k - v2v_delay) % RING]
            dropped = drop_q != 0 and (int(_words(noise_seed, k, m, STREAM_EVAL_LINK)[0]) >> 8) < drop_q
            if not dropped:
                recv[m] = delayed
            obs[3] = recv[m]
            if any(s != 0 for s in sigma):
                r = _words(noise_seed, k, m, STREAM_EVAL_OBS)
                n_ep, n_ev = philox.box_muller(np.array([r[0]]), np.array([r[1]]))
                n_a = philox.box_muller(np.array([r[2]]), np.array([r[3]]))[0]
                for c, n in enumerate((n_ep, n_ev, n_a)):
                    if sigma[c] != 0:
                        obs[c] = obs[c] + float(sigma[c]) * float(n[0])
            acts[m] = law(gains[m], obs[:ep.num_obs], low, high)
        states = []
        for i, f in enumerate(env.followers):  # RefPlatoon.step, keeping each vehicle's reward and terminal flag
            s, rew, term = f.step(acts[i], env.exogenous(i, float(leader[k])))
            states.append(s)
            counters[i] += rew
            if term:
                nterm[i] += 1
                if first[i] < 0:
                    first[i] = k
            su2[i] += acts[i] ** 2
            sj2[i] += f.jerk ** 2
            for c in range(3):
                mx[c, i] = max(mx[c, i], abs(f.x[c]))
        S.append(np.array([np.asarray(s) for s in states]))
        U.append(acts.copy())
        J.append(np.array([f.jerk for f in env.followers]))
    metrics = dict(max_abs_ep=mx[0], max_abs_ev=mx[1], max_abs_a=mx[2], sum_u2=su2, sum_jerk2=sj2, term_steps=nterm, first_term=first,
                   final_abs_ep=np.array([abs(f.x[0]) for f in env.followers]))
    return metrics, x0, dict(states=np.array(S), inputs=np.array(U), jerks=np.array(J), counters=counters)
