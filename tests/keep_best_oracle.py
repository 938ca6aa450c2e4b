"""Retention of the best actors seen in training (avd_keep_best_f32, csrc/best.hip) restated in NumPy: the score formula in sequential
float32 and the retention rule as a state machine over clones of the snapshot slabs. Test infrastructure: nothing here calls the
library."""
import numpy as np


def score(counters):
    """One unit's score: the float32 sum of its NS * M counters in memory order, starting from the first element, one add at a time,
    divided by float32(NS * M). (np.average / np.sum add pairwise from 8 elements on: not used.)"""
    c = np.ascontiguousarray(counters, dtype=np.float32).reshape(-1)
    s = np.float32(c[0])
    with np.errstate(all="ignore"):  # (inf and NaN are inputs like any other)
        for v in c[1:]:
            s = np.float32(s + np.float32(v))
        return np.float32(s / np.float32(c.size))


def improves(new, best):
    """Strict: a tie keeps the older snapshot; a NaN score never improves (every comparison with NaN is false)."""
    return bool(np.float32(new) > np.float32(best))


class KeepBest:
    """The snapshot of n_units units of M sets: best_theta [n_units * M, actor_size], best_stats [n_units * M, cmms] (clones of what it
    is given -- a sentinel pattern, or the actors at the start), best_score float32 [n_units] from -inf, best_step int64 [n_units] from
    -1, and `improved` int32 [n_units] of the last update."""

    def __init__(self, n_units, M, best_theta, best_stats):
        self.n_units, self.M = int(n_units), int(M)
        self.best_theta, self.best_stats = np.array(best_theta, dtype=np.float32, copy=True), np.array(best_stats, dtype=np.float32, copy=True)
        assert self.best_theta.shape[0] == self.best_stats.shape[0] == self.n_units * self.M
        self.actor_size, self.cmms = self.best_theta.shape[1], self.best_stats.shape[1]
        self.best_score = np.full(self.n_units, -np.inf, dtype=np.float32)
        self.best_step = np.full(self.n_units, -1, dtype=np.int64)
        self.improved = np.zeros(self.n_units, dtype=np.int32)

    def update(self, counters, theta, stats, set_base, step):
        """counters [n_units, NS, M] (any shape with n_units leading), theta [n_sets, >= actor_size], stats [n_sets, >= cmms] the online
        slabs (only read), set_base [n_units]. Returns `improved`."""
        counters = np.asarray(counters, dtype=np.float32).reshape(self.n_units, -1)
        M = self.M
        for u in range(self.n_units):
            sc = score(counters[u])
            better = improves(sc, self.best_score[u])
            self.improved[u] = 1 if better else 0
            if not better:
                continue
            b = int(set_base[u])
            assert 0 <= b <= theta.shape[0] - M
            self.best_theta[u * M:(u + 1) * M] = theta[b:b + M, :self.actor_size]
            self.best_stats[u * M:(u + 1) * M] = stats[b:b + M, :self.cmms]
            self.best_score[u], self.best_step[u] = sc, step
        return self.improved.copy()
