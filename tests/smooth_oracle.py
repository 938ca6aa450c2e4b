"""Test infrastructure of the target policy smoothing tests (avd_target_smooth_f32, avd_learn_set_split_smooth_f16x3, tr --target_noise).

Noise: csrc/smooth.hip's draw restated with oracle.philox. Agent v of a call with E experiments of M vehicles (weight set v % (E M)) is
vehicle m = v % M of experiment e = (v // M) % E, platoon p = v // (E M); its index in the experiment's solo run is vs = p M + m. Thread
q = 0 .. 15 of the agent takes the Philox block (key or seeds[e], counter, vs * 16 + q, stream 12); box_muller(w.x, w.y) gives the normals
of rows 4q and 4q + 1 (cos, sin branch), box_muller(w.z, w.w) those of rows 4q + 2 and 4q + 3. eps = clip(sigma n, -c, c) and
a2' = clip(a2 + eps, lo, hi), every operation rounded to float32.

Learner: oracle.mlp.learn restated from its own pieces (actor_forward, critic_forward, critic_backward, actor_backward) with the target
action ta replaced by clip(float32(ta) + eps, lo, hi) in float32 -- the kernel's target action IS a float32 number whatever the dtype
of the weights. Only y changes, and through it the critic gradients and the critic loss. With agent weights the gradients are the
aw_v / P weighted sums over the set's agents (tests/anchor_oracle.py's rule), the two losses the unweighted means the learner reports;
with an anchor the behaviour-cloning gradients of tests/anchor_oracle.py come on top (anchor_oracle.combine serves both)."""
import numpy as np

from oracle import mlp as omlp
from oracle import philox
from tests import anchor_oracle, clone_oracle

STREAM_SMOOTH = 12  # csrc/common.h PhiloxStream
B = 64
Q = 16  # threads per agent: four rows each


def keys(n_agents, M, E):
    """-> (e, p, m, vs) int arrays [n_agents]: experiment, platoon, vehicle and solo agent index of every agent of the call."""
    v = np.arange(n_agents)
    m, e, p = v % M, (v // M) % E, v // (E * M)
    return e, p, m, p * M + m


def normals(n_agents, M, E, counter, seed=0, seeds=None):
    """float32 [n_agents, 64]: the standard normals of one call, before sigma."""
    e, _, _, vs = keys(n_agents, M, E)
    out = np.zeros((n_agents, B), np.float32)
    for k in sorted(set(e.tolist())):
        sel = np.nonzero(e == k)[0]
        idx = (vs[sel][:, None] * Q + np.arange(Q)[None, :]).reshape(-1)
        w = philox.philox_at(int(seed) if seeds is None else int(seeds[k]), int(counter), idx, STREAM_SMOOTH)
        n0, n1 = philox.box_muller(w[0], w[1])
        n2, n3 = philox.box_muller(w[2], w[3])
        out[sel] = np.stack([n0, n1, n2, n3], axis=1).reshape(len(sel), B)  # thread q: rows 4q .. 4q + 3
    return out


def noise(n_agents, M, E, sigma, clip, counter, seed=0, seeds=None):
    """float32 [n_agents, 64]: eps = clip(sigma n, -clip, clip) (clip = inf: none)."""
    n = normals(n_agents, M, E, counter, seed, seeds)
    c = np.float32(clip)
    return np.minimum(np.maximum(np.float32(sigma) * n, -c), c).astype(np.float32)


def smooth(a2, eps, lo, hi):
    """float32: clip(a2 + eps, lo, hi), the sum rounded to float32."""
    x = (np.asarray(a2, dtype=np.float32) + np.asarray(eps, dtype=np.float32)).astype(np.float32)
    return np.minimum(np.maximum(x, np.float32(lo)), np.float32(hi))


def learn_rows(batch, actor, critic, t_actor, t_critic, eps, lo, hi, gamma=0.99, high=2.5):
    """oracle.mlp.learn (workers/trainer.py:472-508) line for line, except ``ta``: the float32 target action plus eps [rows], clipped,
    in float32, then in the dtype of the weights. -> (critic gradients, actor gradients, aux with ``ta`` the smoothed target action and
    ``raw`` the un-smoothed float32 one)."""
    s, a, r, s2 = batch
    dtype = actor[0].dtype
    dt = dtype.type
    s, a, s2 = (np.asarray(v, dtype=dtype) for v in (s, a, s2))
    r = np.asarray(r, dtype=dtype).reshape(len(s), -1)
    raw = omlp.actor_forward(t_actor, s2, high).astype(np.float32)
    ta = smooth(raw, np.asarray(eps, dtype=np.float32).reshape(raw.shape), lo, hi)
    y = r + dt(gamma) * omlp.critic_forward(t_critic, s2, ta.astype(dtype))
    q, cc = omlp.critic_forward(critic, s, a, cache=True)
    n = dt(q.size)
    critic_loss = np.mean(np.square(y - q))
    dq = (dt(2) * (q - y) / n).astype(dtype)
    critic_grad, _ = omlp.critic_backward(critic, cc, dq)
    a1, ac = omlp.actor_forward(actor, s, high, cache=True)
    q1, cc1 = omlp.critic_forward(critic, s, a1, cache=True)
    actor_loss = -np.mean(q1)
    dq1 = np.full_like(q1, dt(-1) / dt(q1.size))
    _, da = omlp.critic_backward(critic, cc1, dq1, need_params=False)
    actor_grad = omlp.actor_backward(actor, ac, da, high)
    return critic_grad, actor_grad, dict(critic_loss=critic_loss, actor_loss=actor_loss, y=y, ta=ta, raw=raw)


def parts(batch, nets, eps, lo, hi, high=2.5, gamma=0.99, agent_weight=None, gain_row=None, model_a=False):
    """One set's summands, as anchor_oracle.parts gives them: dict(cg, ag, bc (None without gain_row), critic_loss, actor_loss,
    anchor_loss, action_clipped: the share of rows whose smoothed target action sits at lo or hi while the un-smoothed one does not;
    the share of rows whose eps sits at +-clip is read off eps by the caller). batch = (s [P, 64, S], a [P, 64, 1], r [P, 64],
    s2 [P, 64, S]) of ONE set's agents, eps [P, 64] theirs; nets the set's four weight lists in the dtype to compute in."""
    s, a, r, s2 = batch
    P = s.shape[0]
    dt = nets[0][0].dtype
    if agent_weight is None:
        groups, factors = [np.arange(P)], [dt.type(1)]
    else:
        groups, factors = [np.array([p]) for p in range(P)], [dt.type(w) / dt.type(P) for w in np.asarray(agent_weight, dtype=dt)]
    out = dict(cg=None, ag=None, bc=None, critic_loss=0.0, actor_loss=0.0, anchor_loss=0.0, action_clipped=0.0)
    acc = lambda old, new, f: [f * x for x in new] if old is None else [o + f * x for o, x in zip(old, new)]
    for sel, f in zip(groups, factors):
        cat = lambda x: x[sel].reshape(len(sel) * B, *x.shape[2:])
        rows = cat(s)
        cg, ag, aux = learn_rows((rows, cat(a), cat(r)[:, None], cat(s2)), *nets, cat(eps), lo, hi, gamma=gamma, high=high)
        out["cg"], out["ag"] = acc(out["cg"], cg, f), acc(out["ag"], ag, f)
        out["critic_loss"] += float(aux["critic_loss"]) / len(groups)
        out["actor_loss"] += float(aux["actor_loss"]) / len(groups)
        at_bound = lambda x: (x <= np.float32(lo)) | (x >= np.float32(hi))
        out["action_clipped"] += float(np.mean(at_bound(aux["ta"]) & ~at_bound(aux["raw"]))) / len(groups)
        if gain_row is not None:
            u = anchor_oracle.law_rows(gain_row, rows, lo, hi, model_a)
            bc, loss, _ = clone_oracle.grads(nets[0], rows, u[:, None], high)
            out["bc"] = acc(out["bc"], bc, f)
            out["anchor_loss"] += float(f) * loss
    return out


def combine(p, weight=0.0):
    """-> (critic gradients, actor gradients): anchor_oracle.combine where there is an anchor, the plain gradients otherwise."""
    return anchor_oracle.combine(p, weight) if p["bc"] is not None else (p["cg"], p["ag"])
