"""Test infrastructure of the residual policy's tests (tr --residual; avd_step_fused_res_f32, avd_eval_rollout_res_f32,
avd_eval_cases_res_f32): the plant input u = clip(law(observation) + scale * r) in float32 NumPy with every product and sum rounded
separately, in the kernels' order, and tests/disturbed_oracle.rollout's float64 loop with that input in place of the actor's action.
With actors whose output is zero the loop IS tests/linear_oracle.rollout (tests/test_residual_cpu.py asserts equality)."""
import dataclasses

import numpy as np

from oracle import mlp, philox, platoon
from tests.disturbed_oracle import RING, STREAM_EVAL_LINK, STREAM_EVAL_OBS, _words

_f = np.float32


def law(gains_row, ob, scale, r, lo, hi, model_a):
    """float32: z = (kp*ob.x + kv*ob.y) + ka*ob.z; z = z + kf*ob.w (Model B only); u = fminf(fmaxf(z + scale*r, lo), hi). ``ob`` and
    ``r`` may carry leading axes ([..., 4] and [...]); ``gains_row`` is [4] or broadcasts against ob."""
    g, ob = np.asarray(gains_row, dtype=_f), np.asarray(ob, dtype=_f)
    r = np.asarray(r, dtype=_f)
    with np.errstate(all="ignore"):
        z = _f(_f(_f(g[..., 0] * ob[..., 0]) + _f(g[..., 1] * ob[..., 1])) + _f(g[..., 2] * ob[..., 2]))
        if not model_a:
            z = _f(z + _f(g[..., 3] * ob[..., 3]))
        s = _f(z + _f(_f(scale) * r))
        return np.minimum(np.maximum(s, _f(lo)), _f(hi)).astype(_f)  # (no NaN reaches the kernels' fmaxf / fminf in these tests)


def law64(gains_row, obs, scale, r, lo, hi):
    """float64, the first len(obs) observations in order (Model A: 3, Model B: 4), as tests/linear_oracle.law adds them."""
    z = 0.0
    for c in range(len(obs)):
        z = gains_row[c] * obs[c] if c == 0 else z + gains_row[c] * obs[c]
    return float(np.clip(z + scale * r, lo, hi))


def rollout(ep, L, actors, gains, scale, leader, evaluation_seed=6, high=2.5, low=-2.5, sigma=(0.0, 0.0, 0.0), v2v_delay=0, v2v_drop=0.0,
            dyn_coeff=None, noise_seed=None):
    """-> (metrics {name: float64 [L]}, x0 float64 [L, 4], traces) as tests/disturbed_oracle.rollout, the plant input being
    law64(gains[m], observation) + scale * the actor's clipped action, clipped; traces also holds ``counters`` float64 [L] and
    ``residual`` (the actors' actions). gains: [L][4]."""
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
    hist = [[x0[i, 3]] * RING for i in range(L)]
    recv = [x0[i, 3] for i in range(L)]
    mx = np.zeros((3, L))
    su2, sj2, nterm, first, counters = np.zeros(L), np.zeros(L), np.zeros(L), np.full(L, -1.0), np.zeros(L)
    S, U, J, R = [], [], [], []
    for k in range(steps):
        acts, res = np.zeros(L), np.zeros(L)
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
            res[m] = np.ravel(mlp.policy(out, None, low, high))[0]
            acts[m] = law64(gains[m], obs[:ep.num_obs], scale, res[m], low, high)
        states = []
        for i, f in enumerate(env.followers):
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
        R.append(res.copy())
        J.append(np.array([f.jerk for f in env.followers]))
    metrics = dict(max_abs_ep=mx[0], max_abs_ev=mx[1], max_abs_a=mx[2], sum_u2=su2, sum_jerk2=sj2, term_steps=nterm, first_term=first,
                   final_abs_ep=np.array([abs(f.x[0]) for f in env.followers]))
    return metrics, x0, dict(states=np.array(S), inputs=np.array(U), jerks=np.array(J), counters=counters, residual=np.array(R))


def rollout32(ep, L, actors, gains, scale, leader, x0, conf, high=2.5, low=-2.5, v2v_delay=0):
    """The same loop in float32 on the CPU (float32 weights through oracle.mlp, ``law``, oracle.platoon.batched_step in float32, the
    metrics by scenarios.metrics_from_traces), for a nominal case or a V2V delay: what float32 arithmetic alone does to the metrics,
    the kernels' summation order aside. x0: the start state [L, 4]. -> (metrics {name: float32 [L]}, traces)."""
    from avddpg_amd import scenarios

    w32 = [[np.asarray(t, dtype=_f) for t in w] for w in actors]
    g = np.asarray(gains, dtype=_f).reshape(L, 4)
    x = np.asarray(x0, dtype=_f).reshape(1, L, 4).copy()
    pa, cum = x[..., 2].copy(), np.zeros((1, L), dtype=_f)
    hist = [[x[0, i, 3]] * RING for i in range(L)]
    model_a = ep.model == platoon.MODEL_A
    S, U, J = [], [], []
    for k in range(len(leader)):
        u = np.zeros((1, L), dtype=_f)
        for m in range(L):
            ob = x[0, m].copy()
            hist[m][k % RING] = ob[3]
            ob[3] = hist[m][(k - v2v_delay) % RING]
            out = mlp.actor_forward(w32[m], ob[None, :ep.num_obs], _f(high))
            r = np.ravel(mlp.policy(out, None, _f(low), _f(high)))[0]
            u[0, m] = law(g[m], ob, scale, r, low, high, model_a)
        o = platoon.batched_step(ep, x, pa, cum, u, np.asarray([leader[k]], dtype=_f), dtype=_f)
        S.append(o["x"][0].copy()), U.append(u[0].copy()), J.append(o["jerk"][0].copy())
        x, pa, cum = o["x"], o["prev_a"], o["cum_accel"]
    tr = dict(states=np.array(S), inputs=np.array(U), jerks=np.array(J))
    return scenarios.metrics_from_traces(tr, np.asarray(x0, dtype=_f), conf), tr
