"""Test infrastructure of the anchor's tests (avd_learn_set_split_anchor_f16x3, tr --anchor): the learner's gradients with the
behaviour-cloning term, from pieces the suite already trusts. The actor's backward pass is linear in its upstream seed, so the gradient
of La' = -mean(w q(s, mu)) + weight * mean(w (mu - u*)^2) over a set's P x 64 concatenated rows is

    oracle.mlp.learn's actor gradients  +  weight x tests.clone_oracle.grads(actor, rows, u*, high)

in the dtype of the weights it is handed; the critic gradients and both losses are oracle.mlp.learn's, unchanged. u* is the law
restated in NumPy float32 in the order of csrc/eval_common.h's linear_law -- (kp ep + kv ev) + ka a, then + kf a_pred under Model B --
and clipped; it is float32 whatever the dtype of the weights (the kernel's target IS a float32 number). With agent weights the terms
are the aw_v / P weighted sums over the set's agents of the per-agent terms (the weighted federated mean); the two losses stay the
unweighted means the learner reports."""
import numpy as np

from oracle import mlp as omlp
from tests import clone_oracle

B = 64


def law_rows(gain_row, s, lo, hi, model_a):
    """float32 [rows]: the clipped law of one gain row (kp, kv, ka, kf) on float32 rows s [rows, S], every product and sum rounded to
    float32 in linear_law's order."""
    g = np.asarray(gain_row, dtype=np.float32)
    s = np.asarray(s, dtype=np.float32)
    z = (g[0] * s[:, 0] + g[1] * s[:, 1]) + g[2] * s[:, 2]
    if not model_a:
        z = z + g[3] * (s[:, 3] if s.shape[1] > 3 else np.float32(0))
    assert z.dtype == np.float32
    return np.clip(z, np.float32(lo), np.float32(hi))


def parts(batch, nets, gain_row, lo, hi, model_a, high=2.5, gamma=0.99, agent_weight=None):
    """The two summands, computed once and shared by every weight: -> dict(cg, ag: oracle.mlp.learn's gradient lists, bc: the
    behaviour-cloning gradients in ACTOR_TRAINABLE order at weight 1, critic_loss, actor_loss, anchor_loss, clipped: the share of rows
    whose target sits at a bound). batch = (s [P, 64, S], a [P, 64, 1], r [P, 64], s2 [P, 64, S]) of ONE set's agents; nets the four
    weight lists of the set in the dtype to compute in; agent_weight [P] or None."""
    s, a, r, s2 = batch
    P = s.shape[0]
    dt = nets[0][0].dtype
    if agent_weight is None:  # the concatenated P x 64-row batch
        groups, factors = [np.arange(P)], [dt.type(1)]
    else:
        groups, factors = [np.array([p]) for p in range(P)], [dt.type(w) / dt.type(P) for w in np.asarray(agent_weight, dtype=dt)]
    out = dict(cg=None, ag=None, bc=None, critic_loss=0.0, actor_loss=0.0, anchor_loss=0.0, clipped=0.0)
    acc = lambda old, new, f: [f * x for x in new] if old is None else [o + f * x for o, x in zip(old, new)]
    for sel, f in zip(groups, factors):
        cat = lambda x: x[sel].reshape(len(sel) * B, *x.shape[2:])
        rows = cat(s)
        cg, ag, aux = omlp.learn((rows, cat(a), cat(r)[:, None], cat(s2)), *nets, gamma=gamma, high=high)
        u = law_rows(gain_row, rows, lo, hi, model_a)
        bc, loss, _ = clone_oracle.grads(nets[0], rows, u[:, None], high)
        out["cg"], out["ag"], out["bc"] = acc(out["cg"], cg, f), acc(out["ag"], ag, f), acc(out["bc"], bc, f)
        out["critic_loss"] += float(aux["critic_loss"]) / len(groups)  # the learner reports both losses unweighted
        out["actor_loss"] += float(aux["actor_loss"]) / len(groups)
        out["anchor_loss"] += float(f) * loss
        out["clipped"] += float(np.mean((u <= np.float32(lo)) | (u >= np.float32(hi)))) / len(groups)
    return out


def combine(p, weight):
    """-> (critic gradients, actor gradients) at this weight, in the dtype of the parts."""
    dt = p["ag"][0].dtype
    return p["cg"], [(g + dt.type(weight) * b).astype(dt) for g, b in zip(p["ag"], p["bc"])]


def learn(batch, nets, gain_row, weight, lo, hi, model_a, high=2.5, gamma=0.99, agent_weight=None):
    """-> (critic gradients, actor gradients, dict(critic_loss, actor_loss, anchor_loss)) of one set."""
    p = parts(batch, nets, gain_row, lo, hi, model_a, high, gamma, agent_weight)
    cg, ag = combine(p, weight)
    return cg, ag, {k: p[k] for k in ("critic_loss", "actor_loss", "anchor_loss")}
