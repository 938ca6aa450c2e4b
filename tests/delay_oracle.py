"""Plain numpy reference of the delayed update (avd_adam_polyak_delayed_f32, tr --policy_delay) for tests/test_delay_cpu.py and
tests/test_gpu_delay_update.py. No device code.

Float32, bit for bit: oracle/mlp.py's adam_alpha / adam_update and tests/optim_oracle.py's rounding of tau (tau_pair), arranged as the
two kinds of call. A set's critic block [actor_size, theta_size) counts its Adam iterations in ``step``, its actor block
[0, actor_size) in ``actor_step``; the caller advances a count before the call that uses it.

  skipped call (policy false): the critic block steps at ``step``. Nothing else changes -- no target, no BN statistics' target,
                               nothing of the actor block, whose gradients are not even looked at.
  policy call  (policy true) : the critic block steps at ``step``, the actor block at ``actor_step``; then the soft update of the whole
                               slab and of the statistics.
  guard                      : a non-finite gradient at the head of the critic block -- on a policy call also of the actor block --
                               leaves the set untouched, its counts where they were before the caller advanced them, and is counted."""
import numpy as np

from oracle import mlp as omlp
from tests import optim_oracle as oo

F = np.float32
STATE = ("theta", "theta_t", "m", "v", "stats", "stats_t", "step", "actor_step")


def schedule(n_calls, d):
    """[policy?] of learner calls 0 .. n_calls - 1 at delay d: call k is a policy call iff (k + 1) % d == 0."""
    return [(k + 1) % d == 0 for k in range(n_calls)]


def delayed_call(h, grads, policy, actor_size, actor_lr, critic_lr, tau):
    """One call on the host state h (a dict of the STATE arrays, [n_sets, ...], modified in place; ``step`` / ``actor_step`` hold the
    counts BEFORE the call: the advance is done here, as AgentGroup.apply_delayed does it). -> the number of sets the guard skipped."""
    A = actor_size
    tf, of = oo.tau_pair(tau)
    bad = ~np.isfinite(grads[:, A])
    if policy:
        bad |= ~np.isfinite(grads[:, 0])
    ok = ~bad
    h["step"][ok] += 1
    if policy:
        h["actor_step"][ok] += 1
    keep = {k: h[k][bad].copy() for k in ("theta", "theta_t", "m", "v", "stats_t")}
    alpha = lambda lr, counts: np.array([omlp.adam_alpha(lr, max(int(c), 1)) for c in counts], F)[:, None]
    with np.errstate(all="ignore"):  # (a guarded set's rows are put back below; NaN elsewhere in a block steps like any number)
        omlp.adam_update(h["theta"][:, A:], h["m"][:, A:], h["v"][:, A:], grads[:, A:], alpha(critic_lr, h["step"]))
        if policy:
            omlp.adam_update(h["theta"][:, :A], h["m"][:, :A], h["v"][:, :A], grads[:, :A], alpha(actor_lr, h["actor_step"]))
            h["theta_t"][:] = h["theta"] * tf + h["theta_t"] * of
            h["stats_t"][:] = h["stats"] * tf + h["stats_t"] * of
    for k, x in keep.items():
        h[k][bad] = x
    return int(bad.sum())


def guarded_call(h, grads, actor_size, actor_lr, critic_lr, tau):
    """avd_adam_polyak_guarded_f32 in the same shape (one count, ``step``), from tests/optim_oracle.adam_polyak_set: what a policy call
    with actor_step == step has to equal."""
    bad = ~np.isfinite(grads[:, actor_size]) | ~np.isfinite(grads[:, 0])
    tf, of = oo.tau_pair(tau)
    for k in np.nonzero(~bad)[0]:
        h["step"][k] += 1
        oo.adam_polyak_set(h["theta"][k], h["theta_t"][k], h["m"][k], h["v"][k], h["stats_t"][k], h["stats"][k], grads[k], h["step"][k],
                           actor_size, actor_lr, critic_lr, tf, of)
    return int(bad.sum())


def host_state(n_sets, theta_size, stats_size, seed, step=5, actor_step=2):
    """A run in progress: weights, targets that differ from them, non-zero moments (spanning 1e-6 .. 1 like the gradients), statistics."""
    rs = np.random.RandomState(seed)
    n = lambda *sh: rs.standard_normal(sh).astype(F)
    scale = rs.choice([1e-6, 1e-3, 1.0], size=(n_sets, theta_size)).astype(F)
    h = dict(theta=0.1 * n(n_sets, theta_size), theta_t=0.1 * n(n_sets, theta_size), m=0.3 * scale * n(n_sets, theta_size),
             v=(scale * scale * rs.uniform(0.0, 1.5, (n_sets, theta_size))).astype(F), stats=n(n_sets, stats_size),
             stats_t=n(n_sets, stats_size), step=np.full(n_sets, step, np.int32), actor_step=np.full(n_sets, actor_step, np.int32))
    h["v"][:, ::97] = 0  # (fresh elements)
    return h, scale, rs


def gradients(scale, rs):
    return (scale * rs.standard_normal(scale.shape)).astype(F)
