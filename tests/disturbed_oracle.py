"""Test infrastructure of the disturbed scenario evaluator's tests: tests/scenario_oracle.rollout's float64 loop over oracle.platoon and
oracle.mlp with the observation model of avd_eval_cases_dist_f32 in front of the actors -- sensor noise on ep, ev, a, delay and loss on
the communicated 4th state, drawn with oracle.philox (streams 6 and 7, counter = step, index = vehicle) -- and the true plant's engine
lag in the vehicles' matrices. Rewards, terminal flags and metrics come from the true state. With the null disturbance it IS
scenario_oracle.rollout (tests/test_disturb_cpu.py asserts equality)."""
import dataclasses

import numpy as np

from oracle import mlp, philox, platoon

STREAM_EVAL_OBS, STREAM_EVAL_LINK = 6, 7
RING = 16


def _words(seed, t, v, stream):
    return [w[0] for w in philox.philox_at(int(seed), int(t), np.array([v]), stream)]


def rollout(ep, L, actors, leader, evaluation_seed=6, high=2.5, low=-2.5, sigma=(0.0, 0.0, 0.0), v2v_delay=0, v2v_drop=0.0, dyn_coeff=None,
            noise_seed=None):
    """-> (metrics {name: float64 [L]}, x0 float64 [L, 4], traces) as scenario_oracle.rollout. ep: the NOMINAL EnvParams (start states);
    dyn_coeff: the true plant's (None: ep's). noise_seed defaults to the evaluation seed. Decentralized platoons."""
    steps = len(leader)
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
    su2, sj2, nterm, first = np.zeros(L), np.zeros(L), np.zeros(L), np.full(L, -1.0)
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
            out = mlp.actor_forward(actors[m], obs[None, :ep.num_obs], high)
            acts[m] = np.ravel(mlp.policy(out, None, low, high))[0]
        states = []
        for i, f in enumerate(env.followers):  # RefPlatoon.step, keeping each vehicle's terminal flag
            s, _, term = f.step(acts[i], env.exogenous(i, float(leader[k])))
            states.append(s)
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
    return metrics, x0, dict(states=np.array(S), inputs=np.array(U), jerks=np.array(J))
