"""Test infrastructure of the warm start's tests: one fit step's batch (avd_clone_sample_f32) restated with oracle.philox and
tests/linear_oracle.law in float32, the supervised actor gradient (avd_actor_clone_f32) through oracle.mlp's actor forward / backward,
and the whole fit (AgentGroup.clone_fit) as a loop over those two and the oracle's Adam -- in the dtype of the weights it is handed."""
import functools

import numpy as np

from oracle import mlp as omlp
from oracle import philox
from tests import linear_oracle

STREAM_CLONE = 11
B = 64
STANDARD_SEED = 1  # the draw seed of standard_fit (if its conditions on the oracle fail for a seed, the seed changes, not the bounds)


def sample(n_sets, S, M, gains, box, lo, hi, model_a, key, counter, seeds=None):
    """-> (s float32 [n_sets, 64, S], u float32 [n_sets, 64, 1]). Set j: vehicle m = j % M, experiment e = (j // M) % E; row b takes the
    Philox block (key or seeds[e], counter, m * 64 + b, stream 11); component c = uniform_pm1(word c) * box[c]; the target is the law
    of gains[m] on the row -- the first three terms only under Model A -- clipped to [lo, hi], all in float32, added in order."""
    gains = np.asarray(gains, dtype=np.float32).reshape(M, 4)
    box = np.asarray(box, dtype=np.float32)
    E = 1 if seeds is None else len(seeds)
    s = np.zeros((n_sets, B, S), np.float32)
    u = np.zeros((n_sets, B, 1), np.float32)
    for j in range(n_sets):
        m, e = j % M, (j // M) % E
        k = int(key) if seeds is None else int(seeds[e])
        w = philox.philox_at(k, int(counter), m * B + np.arange(B), STREAM_CLONE)
        for c in range(S):
            s[j, :, c] = philox.uniform_pm1(w[c]) * box[c]
        n_obs = 3 if (model_a or S == 3) else 4
        for b in range(B):
            u[j, b, 0] = np.float32(linear_oracle.law(gains[m], s[j, b, :n_obs], np.float32(lo), np.float32(hi)))
    return s, u


def grads(actor, s, u, high):
    """-> (gradients in ACTOR_TRAINABLE order, loss, cache) of Lb = mean((mu(s) - u)^2) in the dtype of ``actor``."""
    dt = actor[0].dtype
    out, cache = omlp.actor_forward(actor, np.asarray(s, dtype=dt), high, cache=True)
    d = out - np.asarray(u, dtype=dt)
    dout = (dt.type(2) * d / dt.type(out.size)).astype(dt)
    return omlp.actor_backward(actor, cache, dout, high), float(np.mean(np.square(d))), cache


@functools.lru_cache(maxsize=None)
def standard_fit(dtype_name, draw_seed=STANDARD_SEED, L=3, steps=500):
    """The tests' end-to-end case, computed once per dtype and shared (read only): L actors at the reference widths from the package's
    initialiser with seed ``draw_seed`` (what AgentGroup(seed=draw_seed) starts from), fitted to gains (2, 1, 0, 0) for ``steps``
    steps of size 1e-3 on Philox draws keyed by ``draw_seed`` in the default box. -> dict: losses [L, steps], actors (float64 copies
    of the fitted weights, for the float64 evaluator), score (oracle.evaluator.run on them: Gaussian leader, evaluation seed 6, the
    configuration's episode length), law_score (the law's own mean counter on the same leader, tests/linear_oracle.rollout),
    leader."""
    from avddpg_amd import _hip, config, params, scenarios
    from oracle import evaluator as oeval
    from tests import scenario_oracle

    conf = config.Config(pl_size=L)
    dt = np.dtype(dtype_name)
    spec = scenarios.WarmStart(kp=2, kv=1, steps=steps)
    lay = _hip.make_layout(4, 1, conf.actor_layer1_size, conf.actor_layer2_size, conf.critic_act_layer_size, 64)
    th, st = params.init_weights(lay, np.random.RandomState(draw_seed), nominal=(conf.actor_layer1_size, conf.actor_layer2_size))
    gains, box = spec.gains(L), spec.box(conf)
    draws = [sample(L, 4, L, gains, box, conf.action_low, conf.action_high, False, draw_seed, k) for k in range(steps)]
    actors, losses = [], np.zeros((L, steps))
    for m in range(L):
        w = [x.astype(dt) for x in params.unpack(lay, th, st, "actor")]
        losses[m] = fit(w, steps, spec.lr, lambda k: (draws[k][0][m], draws[k][1][m]), conf.action_high)
        actors.append([x.astype(np.float64) for x in w])
    ep = scenario_oracle.env_params(conf)
    T = conf.steps_per_episode
    _, zero = oeval.run(ep, L, None, T, evaluation_seed=conf.evaluation_seed)
    leader = np.asarray(zero["leader"], dtype=np.float64)
    score, _ = oeval.run(ep, L, actors, T, evaluation_seed=conf.evaluation_seed)
    _, _, tr = linear_oracle.rollout(ep, L, np.asarray(gains, np.float64), leader, evaluation_seed=conf.evaluation_seed)
    return dict(losses=losses, actors=actors, score=float(score), law_score=float(np.mean(tr["counters"])), leader=leader, draws=draws,
                conf=conf, spec=spec)


def fit(actor, steps, lr, draw, high):
    """The fit of one actor (a Keras-ordered weight list, changed in place) with the oracle's Adam: draw(k) -> (s, u) of fit step k.
    -> the losses of every step, float64 [steps]."""
    adam = omlp.RefAdam(lr)
    losses = np.zeros(steps)
    for k in range(steps):
        s, u = draw(k)
        g, losses[k], _ = grads(actor, s, u, high)
        adam.apply_gradients(g, [actor[i] for i in omlp.ACTOR_TRAINABLE])
    return losses
