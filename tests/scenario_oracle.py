"""Test infrastructure of the scenario evaluator's tests: a float64 restatement of one evaluator rollout with the leader-input list
passed in -- the loop of oracle/evaluator.py over oracle.platoon.RefPlatoon, oracle.mlp.actor_forward and oracle.mlp.policy -- that
forms the eight control metrics inside the loop, from the float64 states, and returns its traces beside them."""
import numpy as np

from oracle import mlp, platoon


def env_params(conf):
    """The oracle's EnvParams of a Config's model and method (every other value at the reference's default on both sides)."""
    return platoon.EnvParams(model=platoon.MODEL_A if conf.model == conf.modelA else platoon.MODEL_B, method=conf.method,
                             can_terminate=bool(conf.can_terminate))


def random_actors(conf, L, seed, last_scale=40.0):
    """L seeded random actors as Keras-ordered float64 weight lists (the package's initialiser, last layer scaled so that the actions
    are neither zero nor saturated)."""
    from avddpg_amd import _hip, params

    S = 3 if conf.model == conf.modelA else 4
    lay = _hip.make_layout(S, 1, conf.actor_layer1_size, conf.actor_layer2_size, 48, 64)
    out = []
    for m in range(L):
        th, st = params.init_weights(lay, np.random.RandomState(seed + m))
        w = [x.astype(np.float64) for x in params.unpack(lay, th, st, "actor")]
        w[12] = w[12] * last_scale
        out.append(w)
    return out


def rollout(ep, L, actors, leader, evaluation_seed=6, high=2.5, low=-2.5):
    """-> (metrics {name: float64 [L]}, x0 float64 [L, 4], traces dict as oracle.evaluator.run's). Decentralized platoons."""
    steps = len(leader)
    np.random.seed(evaluation_seed)
    env = platoon.RefPlatoon(L, ep, evaluator_states=True)
    [platoon.get_random_val(ep.rand_gen, ep.reset_max_u, std_dev=ep.reset_max_u) for _ in range(steps)]  # (the draws the profile replaces)
    states = env.reset()
    x0 = np.array([np.asarray(f.x, dtype=np.float64).copy() for f in env.followers])
    mx = np.zeros((3, L))
    su2, sj2, nterm, first = np.zeros(L), np.zeros(L), np.zeros(L), np.full(L, -1.0)
    S, U, J = [], [], []
    for k in range(steps):
        acts = np.zeros(L)
        for m in range(L):
            out = mlp.actor_forward(actors[m], np.asarray(states[m])[None, :], high)
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


def check_against(got, ref, T):
    """A float32 metrics dict ([L] arrays) against the float64 restatement's, at the tolerances tests/test_gpu_eval_rollout.py:182-184
    holds traces to: states atol 2e-4 rtol 1e-4 for the maxima and final_abs_ep; inputs atol 5e-5 for rms_u and jerks atol 5e-3 for
    rms_jerk (the difference of two RMS values is bounded by the largest elementwise difference); the terminal counts equal."""
    for k in ("max_abs_ep", "max_abs_ev", "max_abs_a", "final_abs_ep"):
        print(k, np.max(np.abs(got[k] - ref[k])))
        assert np.allclose(got[k], ref[k], atol=2e-4, rtol=1e-4), (k, got[k], ref[k])
    for k, s, atol in (("rms_u", "sum_u2", 5e-5), ("rms_jerk", "sum_jerk2", 5e-3)):
        a, b = np.sqrt(got[s].astype(np.float64) / T), np.sqrt(ref[s] / T)
        print(k, np.max(np.abs(a - b)))
        assert np.allclose(a, b, atol=atol, rtol=0), (k, a, b)
    assert np.array_equal(got["term_steps"], ref["term_steps"]) and np.array_equal(got["first_term"], ref["first_term"])
