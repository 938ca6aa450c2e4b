"""Test infrastructure of training under disturbances (avd_step_fused_dist_f32, avd_observe_f32): the observation model restated in
numpy over oracle.philox -- streams 8 (sensor noise) and 9 (V2V loss), (key, counter, index) = (experiment seed, observation counter,
vehicle index of the solo run). The noise is oracle.philox's Box-Muller taken to float64, as tests/disturbed_oracle.py takes it; the
loss is an integer compare, exact."""
import numpy as np

from oracle import philox

STREAM_TRAIN_OBS, STREAM_TRAIN_LINK = 8, 9
RING = 16


def level_of(p, n_levels, E=1):
    """The level index of platoon p (of a batch of E interleaved experiments: of its solo run's platoon index)."""
    return (p // E) % n_levels


def normals(seed, counter, index):
    """float64 [n, 3]: (n_ep, n_ev, n_a) of the vehicles ``index`` -- Box-Muller pair of words x, y, then the cos branch of z, w."""
    w = philox.philox_at(int(seed), int(counter), np.asarray(index), STREAM_TRAIN_OBS)
    n_ep, n_ev = philox.box_muller(w[0], w[1])
    n_a = philox.box_muller(w[2], w[3])[0]
    return np.stack([n_ep, n_ev, n_a], axis=-1).astype(np.float64)


def dropped(seed, counter, index, drop_q):
    """bool [n]: the V2V sample of (counter, vehicle) is lost iff drop_q != 0 and (word x >> 8) < drop_q."""
    w = philox.philox_at(int(seed), int(counter), np.asarray(index), STREAM_TRAIN_LINK)[0]
    return (int(drop_q) != 0) & ((w >> np.uint64(8)) < np.uint64(drop_q))


class Link:
    """The link state of n vehicles under ONE level: a 16-slot ring and a held value each, fresh from w0 [n]."""

    def __init__(self, w0, delay, drop_q, seed, index):
        w0 = np.asarray(w0, dtype=np.float32)
        self.hist = np.repeat(w0[:, None], RING, axis=1)
        self.recv = w0.copy()
        self.delay, self.drop_q, self.seed, self.index = int(delay), int(drop_q), int(seed), np.asarray(index)

    def push(self, w, counter):
        """The true w [n] of the state observed with ``counter`` -> (observed w, dropped mask)."""
        self.hist[:, counter & (RING - 1)] = np.asarray(w, dtype=np.float32)
        delayed = self.hist[:, (counter - self.delay) & (RING - 1)]
        lost = dropped(self.seed, counter, self.index, self.drop_q)
        self.recv = np.where(lost, self.recv, delayed).astype(np.float32)
        return self.recv.copy(), lost
