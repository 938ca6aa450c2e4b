"""Plain numpy references of the optimiser / federation kernels (csrc/optim.hip) for tests/test_gpu_optim_kernels.py. No device code.

* float32 Adam + Polyak of one weight set, bit for bit: oracle/mlp.py's adam_alpha / adam_update and update_target's rounding of tau;
* float64 fed_sum / fed_finalize over both stride patterns (interfrl so = 1, si = M; intrafrl so = M, si = 1);
* a host shadow of the closed-episode reward ring (fed_history_push);
* float64 fed_weights;
* the bound on what one Adam + Polyak step does to a perturbed gradient (the intrafrl form averages in float32)."""
import numpy as np

from oracle import mlp as omlp

F = np.float32
U = 2.0 ** -24  # float32 unit roundoff


def tau_pair(tau):
    """update_target (oracle/mlp.py): tau and 1 - tau are Python doubles, each rounded to float32 where it multiplies."""
    return F(tau), F(1 - tau)


def adam_polyak_set(th, tht, m, v, stt, st, g, t, actor_size, actor_lr, critic_lr, tau_f, omt_f):
    """One Adam + Polyak step of ONE weight set at Adam iteration t, in place, float32: the actor block [0, actor_size) with
    actor_lr, the critic block with critic_lr, then the soft update of the targets and of the BN statistics' targets (stt <- st)."""
    n = th.shape[0]
    for lo, hi, lr in ((0, actor_size, actor_lr), (actor_size, n, critic_lr)):
        omlp.adam_update(th[lo:hi], m[lo:hi], v[lo:hi], g[lo:hi], omlp.adam_alpha(lr, int(t)))
    tht[:] = th * tau_f + tht * omt_f
    stt[:] = st * tau_f + stt * omt_f


def strides(method, P, M):
    """(n_out, n_in, so, si): agent v = p * M + m; row(o, i) = o * so + i * si."""
    return (M, P, 1, M) if method == "interfrl" else (P, M, M, 1)


def fed_rows(n_out, n_in, so, si):
    return (np.arange(n_out)[:, None] * so + np.arange(n_in)[None, :] * si)  # [n_out, n_in] row indices


def fed_sum64(g, weights, n_out, n_in, so, si):
    """float64: (sum_i w g, sum_i |w g|, sum_i w) per output row; weights None = ones."""
    rows = fed_rows(n_out, n_in, so, si)
    x = g.astype(np.float64)[rows]  # [n_out, n_in, n]
    w = np.ones(rows.shape) if weights is None else weights.astype(np.float64).reshape(-1)[rows]
    wx = w[:, :, None] * x
    return wx.sum(axis=1), np.abs(wx).sum(axis=1), w.sum(axis=1)


def fed_sum_bound(n_in, abs_sum, wsum):
    """|float32 mean - exact mean| per element for fed_sum_kernel's order: the members go to four phases (recursive summation of
    ceil(n_in / 4) products each), the phases are combined (4 roundings counted) and the sum is scaled (2)."""
    return (-(-n_in // 4) + 8) * U * abs_sum / wsum[:, None]


class HistoryShadow:
    """Host shadow of fed_history_push_kernel: ring[P * M, W] of closed-episode rewards, hist_cnt[P]; a closing platoon writes its M
    running rewards to slot hist_cnt % W and counts."""

    def __init__(self, P, M, W, ring, cnt):
        self.P, self.M, self.W = P, M, W
        self.ring, self.cnt = ring.copy().reshape(P * M, W), cnt.copy()

    def push(self, ep_reward, close, zero_after):
        """close: bool [P]. ep_reward [P * M] is modified in place (zero_after)."""
        for p in np.nonzero(close)[0]:
            slot = int(self.cnt[p]) % self.W
            sl = slice(p * self.M, (p + 1) * self.M)
            self.ring[sl, slot] = ep_reward[sl]
            if zero_after:
                ep_reward[sl] = 0
            self.cnt[p] += 1


def fed_weights64(ring, cnt, P, M, W, host_enabled):
    """float64: w = |W / sum(ring row)|, wsum[m] = sum_p w[p, m], aw = w P / wsum[m]; enabled = host_enabled (0 / 1), or for -1
    min(hist_cnt) >= W. Disabled: ones and wsum = P. Returns (enabled, w [P, M], aw [P, M], wsum [M])."""
    enabled = bool(host_enabled) if host_enabled >= 0 else bool(cnt.min() >= W)
    if not enabled:
        return False, np.ones((P, M)), np.ones((P, M)), np.full(M, float(P))
    w = np.abs(W / ring.astype(np.float64).reshape(P * M, W).sum(axis=1)).reshape(P, M)
    wsum = w.sum(axis=0)
    return True, w, w * P / wsum[None, :], wsum


def adam_polyak_perturbation_bound(w0, wt0, m0, v0, g, dg, alpha, tau_f, omt_f):
    """Two float32 evaluations of one Adam + Polyak step from the same state, with gradients within dg of g (elementwise): bounds on
    how far apart their m, v, weight and target can be, by the formulas of adam_update in float64 plus the float32 roundings of both
    evaluations. Returns (bm, bv, bw, bt).

      m' = m + (g - m) 0.1          |dm| <= 0.1 dg                      + 3 roundings each side
      v' = v + (g^2 - v) 0.001      |dv| <= 0.001 (2 |g| dg + dg^2)     + 4 roundings each side
      s  = m' alpha / (sqrt v' + e) |ds| <= alpha (bm / d_lo + |m'| (d_hi - d_lo) / (d_hi d_lo)),  d_lo, d_hi from v' -+ bv
      w' = w - s,  t' = w' tau + t (1 - tau)"""
    f8 = lambda x: np.asarray(x, np.float64)
    w0, wt0, m0, v0, g, dg, alpha = map(f8, (w0, wt0, m0, v0, g, dg, alpha))
    c1, c2, eps = 1.0 - float(F(omlp.ADAM_B1)), 1.0 - float(F(omlp.ADAM_B2)), float(F(omlp.ADAM_EPS))
    m1 = m0 + (g - m0) * c1
    v1 = v0 + (g * g - v0) * c2
    dg2 = 2 * np.abs(g) * dg + dg * dg
    bm = c1 * dg + 6 * U * (np.abs(g) + np.abs(m0) + dg)
    bv = c2 * dg2 + 8 * U * (g * g + np.abs(v0) + dg2)
    # both evaluations' denominators fl(fl(sqrt v') + e) lie in [d_lo, d_hi]
    d_lo = (np.sqrt(np.maximum(v1 - bv, 0.0)) + eps) * (1 - 4 * U)
    d_hi = (np.sqrt(v1 + bv) + eps) * (1 + 4 * U)
    s_hi = alpha * (np.abs(m1) + bm) / d_lo
    bs = alpha * bm / d_lo + alpha * (np.abs(m1) + bm) * (d_hi - d_lo) / (d_lo * d_hi) + 8 * U * s_hi
    w1 = w0 - m1 * alpha / (np.sqrt(v1) + eps)
    bw = bs + 2 * U * (np.abs(w1) + 2 * bs)
    bt = float(tau_f) * bw + 6 * U * (np.abs(w1) * float(tau_f) + np.abs(wt0) * float(omt_f) + bw)
    return bm, bv, bw, bt
