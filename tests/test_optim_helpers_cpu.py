"""tests/optim_oracle.py (the numpy references of the optimiser / federation kernel tests) against hand-computed small cases and
against the oracle it restates: a reference that is wrong would make the GPU tests built on it pass or fail for the wrong reason."""
import numpy as np

from oracle import federated as ofed
from oracle import mlp as omlp
from tests import optim_oracle as oo

F = np.float32


def test_adam_polyak_set_equals_refadam_and_update_target():
    """three steps of one set from zero moments: the actor and the critic block as two RefAdam optimisers (their own step sizes), the
    targets as update_target -- bit for bit"""
    rs = np.random.RandomState(0)
    n, A, alr, clr, tau = 40, 12, 1e-4, 1e-3, 0.005
    th = rs.standard_normal(n).astype(F)
    tht, st, stt = rs.standard_normal(n).astype(F), rs.standard_normal(8).astype(F), rs.standard_normal(8).astype(F)
    m, v = np.zeros(n, F), np.zeros(n, F)
    ra, rc = [th[:A].copy()], [th[A:].copy()]
    ta, tc = [tht[:A].copy()], [tht[A:].copy()]
    oa, oc = omlp.RefAdam(alr), omlp.RefAdam(clr)
    tf, of = oo.tau_pair(tau)
    assert (tf, of) == (F(0.005), F(0.995))
    for step in (1, 2, 3):
        g = (rs.standard_normal(n) * rs.choice([1e-6, 1e-3, 1.0], n)).astype(F)
        oo.adam_polyak_set(th, tht, m, v, stt, st, g, step, A, alr, clr, tf, of)
        oa.apply_gradients([g[:A]], ra)
        oc.apply_gradients([g[A:]], rc)
        tc, ta = omlp.update_target(tau, tc, rc, ta, ra)
        assert np.array_equal(th, np.concatenate([ra[0], rc[0]])) and np.array_equal(tht, np.concatenate([ta[0], tc[0]]))
        assert np.array_equal(m, np.concatenate([oa.m[0], oc.m[0]])) and np.array_equal(v, np.concatenate([oa.v[0], oc.v[0]]))
    assert th.dtype == tht.dtype == m.dtype == v.dtype == stt.dtype == np.float32


def test_strides_and_fed_sum64_by_hand():
    P, M = 2, 3  # agent v = p * M + m; rows of g are v = 0 .. 5
    g = np.array([[1, 10], [2, 20], [3, 30], [4, 40], [5, 50], [-6, 60]], F)
    w = np.array([1, 2, 3, 4, 0, 0.5], F)
    assert oo.strides("interfrl", P, M) == (3, 2, 1, 3) and oo.strides("intrafrl", P, M) == (2, 3, 3, 1)
    assert oo.fed_rows(3, 2, 1, 3).tolist() == [[0, 3], [1, 4], [2, 5]] and oo.fed_rows(2, 3, 3, 1).tolist() == [[0, 1, 2], [3, 4, 5]]
    s, a, ws = oo.fed_sum64(g, None, 3, 2, 1, 3)  # over platoons
    assert s.tolist() == [[5, 50], [7, 70], [-3, 90]] and a.tolist() == [[5, 50], [7, 70], [9, 90]] and ws.tolist() == [2, 2, 2]
    s, a, ws = oo.fed_sum64(g, w, 2, 3, 3, 1)  # over a platoon's vehicles, weighted
    assert s.tolist() == [[14, 140], [13, 190]] and a.tolist() == [[14, 140], [19, 190]] and ws.tolist() == [6, 4.5]
    assert s.dtype == np.float64
    # the oracle's list-of-lists federated mean is the same number
    ref = ofed.get_avg_params([[[g[p * M + m_]] for p in range(P)] for m_ in range(M)])
    s, _, ws = oo.fed_sum64(g, None, 3, 2, 1, 3)
    assert all(np.allclose(ref[m_][0], s[m_] / ws[m_]) for m_ in range(M))
    # the bound: (ceil(n_in / 4) + 8) 2^-24 sum|w g| / sum w
    b = oo.fed_sum_bound(5, np.array([[8.0]]), np.array([2.0]))
    assert b.tolist() == [[(2 + 8) * 2.0 ** -24 * 4.0]]


def test_history_shadow_by_hand():
    P, M, W = 2, 2, 2
    sh = oo.HistoryShadow(P, M, W, np.full((4, 2), -9, F), np.array([0, 3], np.int32))
    ep = np.array([-1, -2, -3, -4], F)
    sh.push(ep, np.array([True, False]), zero_after=0)  # platoon 0 closes into slot 0
    assert sh.ring.tolist() == [[-1, -9], [-2, -9], [-9, -9], [-9, -9]] and sh.cnt.tolist() == [1, 3] and ep.tolist() == [-1, -2, -3, -4]
    sh.push(ep, np.array([True, True]), zero_after=1)  # platoon 0 -> slot 1, platoon 1 (count 3) -> slot 1
    assert sh.ring.tolist() == [[-1, -1], [-2, -2], [-9, -3], [-9, -4]] and sh.cnt.tolist() == [2, 4] and ep.tolist() == [0, 0, 0, 0]
    ep[:] = [-5, -6, -7, -8]
    sh.push(ep, np.array([False, True]), zero_after=1)  # wraps: platoon 1 (count 4) -> slot 0
    assert sh.ring.tolist() == [[-1, -1], [-2, -2], [-7, -3], [-8, -4]] and sh.cnt.tolist() == [2, 5] and ep.tolist() == [-5, -6, 0, 0]
    sh.push(ep, np.array([False, False]), zero_after=1)
    assert sh.cnt.tolist() == [2, 5] and ep.tolist() == [-5, -6, 0, 0]


def test_fed_weights64_by_hand():
    P, M, W = 2, 2, 2
    ring = np.array([[-1, -3], [-4, -4], [2, 6], [-8, -8]], F)  # row means -2, -4, +4, -8 -> w = 1/2, 1/4, 1/4, 1/8
    on, w, aw, ws = oo.fed_weights64(ring, np.array([2, 5], np.int32), P, M, W, 1)
    assert on and w.tolist() == [[0.5, 0.25], [0.25, 0.125]] and ws.tolist() == [0.75, 0.375]
    assert np.allclose(aw, [[4 / 3, 4 / 3], [2 / 3, 2 / 3]], rtol=1e-15) and np.allclose(aw.sum(axis=0), P, rtol=1e-15)
    assert oo.fed_weights64(ring, np.array([2, 5], np.int32), P, M, W, -1)[0]  # every platoon has W closed episodes
    for enabled, cnt in ((0, [2, 5]), (-1, [2, 1]), (-1, [1, 2])):  # switched off; one platoon one episode short
        on, w, aw, ws = oo.fed_weights64(ring, np.array(cnt, np.int32), P, M, W, enabled)
        assert not on and np.all(w == 1) and np.all(aw == 1) and ws.tolist() == [2, 2]
    # the reference trainer's rule (oracle/trainer.py): |1 / mean(last W episodic rewards)|
    assert w.shape == (P, M) and abs(1 / np.mean([-1, -3])) == 0.5


def test_perturbation_bound_holds_and_is_not_slack():
    """two float32 Adam + Polyak steps from one state whose gradients differ by up to dg: the results are within the bound (not slack:
    above half of it somewhere), and a gradient off by 1000 dg is far outside"""
    rs = np.random.RandomState(1)
    n = 100000
    sc = rs.choice([1e-6, 1e-3, 1.0], n).astype(F)
    w0, wt0 = (0.1 * rs.standard_normal(n)).astype(F), (0.1 * rs.standard_normal(n)).astype(F)
    m0, v0 = (0.3 * sc * rs.standard_normal(n)).astype(F), (sc * sc * rs.uniform(0, 1.5, n)).astype(F)
    v0[::97] = 0
    g = (rs.standard_normal(n) * rs.choice([1e-8, 1e-3, 1.0], n)).astype(F)
    tf, of = oo.tau_pair(0.005)

    def step(gg, t):
        th, tht, m, v = w0.copy(), wt0.copy(), m0.copy(), v0.copy()
        oo.adam_polyak_set(th, tht, m, v, np.zeros(4, F), np.zeros(4, F), gg, t, n, 1e-3, 1e-3, tf, of)
        return m, v, th, tht

    for t in (1, 4, 1000, 10**6):
        alpha = float(omlp.adam_alpha(1e-3, t))
        for factor, inside in ((1, True), (1000, False)):
            g2 = (g + factor * 3e-7 * np.abs(g) * rs.choice([-1, 1], n)).astype(F)
            dg = np.abs(g2.astype(np.float64) - g) / factor  # (factor 1000: the bound is told a thousandth of the truth)
            bounds = oo.adam_polyak_perturbation_bound(w0, wt0, m0, v0, g, dg, alpha, tf, of)
            ratios = [float(np.max(np.abs(a.astype(np.float64) - b) / bd)) for a, b, bd in zip(step(g, t), step(g2, t), bounds)]
            assert (max(ratios) <= 1.0) == inside, (t, factor, ratios)
            assert max(ratios) > (0.5 if inside else 10), (t, factor, ratios)
