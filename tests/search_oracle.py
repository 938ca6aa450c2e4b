"""NumPy restatement of the gain search's two entry points (avd_search_sample_f32, avd_search_refit_f32: csrc/search.hip), built on
oracle/philox.py (TEST INFRASTRUCTURE). Every operation is float32, one rounding per operation, in the order include/avddpg_hip.h
states; nothing here is shared with the code under test."""
import numpy as np

from oracle import philox

STREAM_SEARCH = 10
F = np.float32


def sample(G, L, R, mean, std, lo, hi, seed, generation):
    """-> (gains float32 [G, L, 4], raw float32 [G, L, 4]): the candidates, and their values before the clip to [lo, hi]."""
    mean, std, lo, hi = (np.asarray(x, dtype=F).reshape(R, 4) for x in (mean, std, lo, hi))
    idx = (np.arange(G, dtype=np.uint64)[:, None] * np.uint64(R) + np.arange(R, dtype=np.uint64)[None, :]).reshape(-1) & np.uint64(0xFFFFFFFF)
    w = philox.philox_at(int(seed), int(generation), idx, STREAM_SEARCH)
    n0, n1 = philox.box_muller(w[0], w[1])
    n2, n3 = philox.box_muller(w[2], w[3])
    n = np.stack([n0, n1, n2, n3], axis=1).astype(F).reshape(G, R, 4)
    moved = (std[None] * n).astype(F)
    moved = (mean[None] + moved).astype(F)
    keep = (np.arange(G)[:, None, None] == 0) | (std[None] == 0)
    raw = np.where(keep, np.broadcast_to(mean[None], moved.shape), moved).astype(F)
    x = np.fmin(np.fmax(raw, lo[None]), hi[None]).astype(F)
    if R == 1:
        x, raw = np.repeat(x, L, axis=1), np.repeat(raw, L, axis=1)
    return np.ascontiguousarray(x), np.ascontiguousarray(raw)


def precedes(fi, i, fj, j):
    """Candidate i precedes candidate j."""
    ni, nj = np.isnan(fi), np.isnan(fj)
    if ni:
        return bool(nj and i < j)
    return bool(nj or fi > fj or (fi == fj and i < j))


def rank(fitness):
    """-> (order int32 [G] with order[rank] = candidate, n_valid): a candidate's rank is the number of candidates that precede it."""
    f = np.asarray(fitness, dtype=F)
    G = f.shape[0]
    nan = np.isnan(f)
    i = np.arange(G)
    with np.errstate(invalid="ignore"):
        # pre[j, i]: j precedes i
        pre = ~nan[:, None] & (nan[None, :] | (f[:, None] > f[None, :]) | ((f[:, None] == f[None, :]) & (i[:, None] < i[None, :])))
    pre |= nan[:, None] & nan[None, :] & (i[:, None] < i[None, :])
    ranks = pre.sum(axis=0)
    assert sorted(ranks.tolist()) == list(range(G))
    order = np.empty(G, dtype=np.int32)
    order[ranks] = i
    return order, int((~nan).sum())


def refit(G, L, R, n_elite, alpha, gains, fitness, min_std, mean, std, best_gains, best_fitness, best_gen, generation):
    """-> dict(mean, std, best_gains [R, 4], best_fitness, best_gen, elite_idx int32 [n_elite], history_row float32 [4], E): the state
    after avd_search_refit_f32. Inputs are not modified."""
    gains = np.asarray(gains, dtype=F).reshape(G, L, 4)
    f = np.asarray(fitness, dtype=F)
    mean, std, min_std, best_gains = (np.array(x, dtype=F).reshape(R * 4) for x in (mean, std, min_std, best_gains))
    alpha, best_fitness, best_gen = F(alpha), F(best_fitness), int(best_gen)
    order, n_valid = rank(f)
    elite_idx = order[:n_elite].copy()
    E = min(int(n_elite), n_valid)
    if E == 0:
        hist = np.array([np.nan, np.nan, best_fitness, 0.0], dtype=F)
        return dict(mean=mean.reshape(R, 4), std=std.reshape(R, 4), best_gains=best_gains.reshape(R, 4), best_fitness=best_fitness,
                    best_gen=best_gen, elite_idx=elite_idx, history_row=hist, E=0)
    x = gains[elite_idx[:E], :R, :].reshape(E, R * 4)  # x[k][d], rank order
    s = np.zeros(R * 4, dtype=F)
    for k in range(E):
        s = (s + x[k]).astype(F)
    m = (s / F(E)).astype(F)
    q = np.zeros(R * 4, dtype=F)
    for k in range(E):
        t = (x[k] - m).astype(F)
        q = (q + (t * t).astype(F)).astype(F)
    sd = np.sqrt((q / F(E)).astype(F)).astype(F)
    live = std != 0
    new_mean = (mean + (alpha * (m - mean).astype(F)).astype(F)).astype(F)
    new_std = np.fmax((std + (alpha * (sd - std).astype(F)).astype(F)).astype(F), min_std).astype(F)
    mean_o, std_o = np.where(live, new_mean, mean).astype(F), np.where(live, new_std, std).astype(F)
    top = int(elite_idx[0])
    if best_gen < 0 or f[top] > best_fitness:
        best_gains, best_fitness, best_gen = gains[top, :R, :].reshape(R * 4).copy(), f[top], int(generation)
    fs = F(0)
    for k in range(E):
        fs = F(fs + f[elite_idx[k]])
    hist = np.array([f[top], F(fs / F(E)), best_fitness, F(E)], dtype=F)
    return dict(mean=mean_o.reshape(R, 4), std=std_o.reshape(R, 4), best_gains=best_gains.reshape(R, 4), best_fitness=F(best_fitness),
                best_gen=best_gen, elite_idx=elite_idx, history_row=hist, E=E)


def refit_f64(E, x, alpha, mean, std, min_std):
    """The refit's mean / std update in float64 from elite values x [E, D] (the yardstick of the float32 statement above)."""
    x = np.asarray(x, dtype=np.float64)
    m = x.sum(axis=0) / E
    sd = np.sqrt(((x - m) ** 2).sum(axis=0) / E)
    mean, std, min_std = (np.asarray(v, dtype=np.float64) for v in (mean, std, min_std))
    live = std != 0
    return (np.where(live, mean + alpha * (m - mean), mean), np.where(live, np.maximum(std + alpha * (sd - std), min_std), std))
