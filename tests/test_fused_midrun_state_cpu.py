"""The state generator of tests/test_gpu_fused_update_midrun.py (midrun_moments, midrun_counts, oracle_agents), without a GPU: on every
layout the GPU test uses, the moments are what a run in progress holds (three scales in both blocks, |m| <= sqrt(v), fresh elements,
padding at zero, never v = 0 under m != 0), every agent has its own Adam iteration count with all of STEP_COUNTS among them, a kernel
that read another agent's count would take another step size, the oracle at a neighbouring count gives other bits, and the float32
oracle's own step from that state stays below 4.1 lr at every one of STEP_COUNTS -- the one derived number of the GPU test:

  m' = 0.9 m + 0.1 g, v' = 0.999 v + 0.001 g^2, |m| <= sqrt(v):
  |m'| / sqrt(v') <= 0.9 sqrt(v) / sqrt(0.999 v) + 0.1 |g| / sqrt(0.001 g^2) = 0.9 / 0.9995 + 0.1 / 0.03162 = 4.063 < 4.1,
  and alpha_t = lr sqrt(1 - b2^t) / (1 - b1^t) <= lr for every t >= 1 (tests/test_optim_oracle_cpu.py).

The float32 roundings of the step and of the weight it is subtracted from (|w| <= 2: half an ulp is 1.2e-7) are far inside the 0.9 %
between 4.063 and 4.1 at the smallest step size used, 5e-5."""
import numpy as np
import pytest

from avddpg_amd import config, params
from tests import optim_oracle as oo
from tests.test_gpu_fused_update_midrun import (BOUNDARY_COUNTS, FRESH_EVERY, HP_ROWS, INT32_MAX, LAYOUTS, MIN_STEP_SIZES, SCALES, alpha_bits,
                                                assert_counts_expose_index_defects, hparams_of, layout_of, midrun_counts, midrun_moments,
                                                oracle_agents, tensor_at, wrong_count_agents)
from tests.test_gpu_general_shapes import _logical_mask
from tests.test_gpu_optim_kernels import HP_BLOCK, STEP_COUNTS

F = np.float32
N = 27  # agents: more than STEP_COUNTS, no multiple of anything


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("key", sorted(LAYOUTS))
def test_midrun_moments_are_a_run_in_progress(key):
    ref = layout_of(key)
    lay, mask = ref.lay, _logical_mask(ref)
    T, AS = lay.theta_size, lay.actor_size
    m, v = midrun_moments(mask, N, seed=5)
    assert m.shape == v.shape == (N, T) and m.dtype == v.dtype == F and np.all(np.isfinite(m)) and np.all(np.isfinite(v))
    assert np.all(v >= 0)
    # padding and fresh elements: both moments exactly zero; v = 0 never under m != 0
    fresh = np.zeros(T, bool)
    fresh[::FRESH_EVERY] = True
    assert not m[:, ~mask].any() and not v[:, ~mask].any()
    assert not m[:, fresh].any() and not v[:, fresh].any()
    assert not m[v == 0].any()
    live = mask & ~fresh
    assert np.mean(v[:, live] > 0) > 0.9999 and np.mean(m[:, live] != 0) > 0.999
    assert int((~mask).sum()) > 0 and int((mask & fresh).sum()) >= T // FRESH_EVERY // 2
    # |m| <= sqrt(v): m is fl(c fl(sqrt v)) with |c| < 1, at most (1 + 2^-24) sqrt(v)
    m8, v8 = m.astype(np.float64), v.astype(np.float64)
    assert np.all(m8 * m8 <= v8 * (1 + 4 * oo.U))
    assert np.mean(m[:, live] < 0) > 0.4 and np.mean(m[:, live] > 0) > 0.4
    # the three scales in the actor block and in the critic block (v = scale^2 U(0, 1.5): a band per scale, the rest below it)
    for lo, hi in ((0, AS), (AS, T)):
        blk = v[:, lo:hi][:, live[lo:hi]]
        edges = [1.5 * s * s for s in SCALES]
        assert np.all(blk <= edges[2])
        for a, b in ((0.0, edges[0]), (edges[0], edges[1]), (edges[1], edges[2])):
            assert 0.3 < np.mean((blk > a) & (blk <= b)) < 0.37, (key, lo, a, b)
    # seeded; the agents differ
    m2, v2 = midrun_moments(mask, N, seed=5)
    assert np.array_equal(_bits(m), _bits(m2)) and np.array_equal(_bits(v), _bits(v2))
    m3, _ = midrun_moments(mask, N, seed=6)
    assert not np.array_equal(_bits(m), _bits(m3)) and not np.array_equal(_bits(m[0]), _bits(m[1]))


@pytest.mark.parametrize("n", [26, 32, 36, 100, 300])
def test_midrun_counts_give_every_step_count_to_an_agent(n):
    c = midrun_counts(n, seed=300 + n)
    assert c.dtype == np.int32 and c.shape == (n,) and c.min() >= 1
    c8 = c.astype(np.int64)
    assert (c8 + 1).max() <= INT32_MAX  # the second update's count is still an int32
    have = set(c8.tolist())
    assert set(STEP_COUNTS) - {INT32_MAX} <= have and INT32_MAX - 1 in have  # (2^31 - 1 is reached in the second update)
    for a in (164, 986, 17320, 103921):  # the pairs the second update crosses
        assert a in have and a + 1 in STEP_COUNTS
    assert len(have) >= 20
    assert c8[:len(STEP_COUNTS)].tolist() != [min(t, INT32_MAX - 1) for t in STEP_COUNTS]  # shuffled over the agents
    assert np.array_equal(c, midrun_counts(n, seed=300 + n))
    sel = oracle_agents(c, boundaries=[n // 2])
    assert set(np.nonzero(np.isin(c8, STEP_COUNTS))[0].tolist()) <= set(sel.tolist()) and {n // 2 - 1, n // 2} <= set(sel.tolist())
    assert int(np.nonzero(c8 == INT32_MAX - 1)[0][0]) in sel and len(sel) == len(set(sel.tolist())) >= len(STEP_COUNTS)


@pytest.mark.parametrize("n,chunk,groups", [(26, None, None), (36, None, None), (300, 256, 256), (148, 104, 104), (100, 40, 7)])
def test_counts_expose_a_wrong_index_and_differ_across_chunk_boundaries(n, chunk, groups):
    """A kernel that reads step[0], the count of the same position in the first chunk, or the count of the first row its workgroup
    walked, gets another STEP SIZE for more than half of the agents that defect touches, in both updates; the agents on either side
    of every chunk boundary hold BOUNDARY_COUNTS; at least MIN_STEP_SIZES different step sizes occur."""
    boundaries = list(range(chunk, n, chunk)) if chunk else []
    c = midrun_counts(n, seed=300 + n, boundaries=boundaries)
    have = set(c.tolist())
    assert set(STEP_COUNTS) - {INT32_MAX} <= have and INT32_MAX - 1 in have and len(have) >= 20
    for lr in (5e-5, 2e-3):
        assert assert_counts_expose_index_defects(c, lr, chunk, groups) >= MIN_STEP_SIZES
        assert assert_counts_expose_index_defects(c + 1, lr, chunk, groups) >= MIN_STEP_SIZES - 1  # (17321 joins the counts at lr itself)
    for b, pair in zip(boundaries, BOUNDARY_COUNTS):
        assert (int(c[b - 1]), int(c[b])) == pair and len(set(alpha_bits(c[b - 1:b + 1], 5e-5).tolist())) == 2
    wrong = wrong_count_agents(n, chunk, groups)
    assert not wrong["step[0]"].any()
    if chunk:
        a = np.arange(n)
        assert np.array_equal(wrong["step of the first chunk"], a % chunk)
        assert np.array_equal(wrong["step of the workgroup's first row"], a // chunk * chunk + a % chunk % groups)


def test_the_oracle_check_notices_a_step_size_one_ulp_off():
    """17320 and 17321 give step sizes one ulp apart (1 - beta2^t rounds to 1 at 17321): the oracle's step from one generated state at
    these two counts differs in the bits of hundreds of weights, in both blocks (a step of ~1e-5 on a weight of ~0.05 with an ulp of
    4e-9: the changed step crosses a rounding boundary of the weight for a few per cent of the elements) -- the comparison of the GPU
    test with the oracle at the agent's own count cannot pass on a neighbour's."""
    ref = layout_of("ref4")
    lay, mask = ref.lay, _logical_mask(ref)
    a = alpha_bits([17320, 17321], 5e-5)
    assert int(a[1]) - int(a[0]) == 1
    m0, v0 = midrun_moments(mask, 1, seed=9)
    rs = np.random.RandomState(10)
    th, st = params.init_weights(lay, rs, dims=ref.dims)
    g = (rs.standard_normal(lay.theta_size) * rs.choice(SCALES, lay.theta_size) * mask).astype(F)
    out = []
    for count in (17320, 17321):
        w, tht, m, v, stt = th.copy(), th.copy(), m0[0].copy(), v0[0].copy(), st.copy()
        oo.adam_polyak_set(w, tht, m, v, stt, st, g, count, lay.actor_size, F(5e-5), F(5e-4), *oo.tau_pair(0.001))
        out.append(w)
    diff = _bits(out[0]) != _bits(out[1])
    assert diff[:lay.actor_size].sum() > 100 and diff[lay.actor_size:].sum() > 100


def test_tensor_at_names_the_slab_tensor():
    lay = layout_of("padded3").lay
    AS = lay.actor_size
    assert [tensor_at(lay, i) for i in (0, lay.aW2, lay.aW2 - 1, AS - 1, AS, AS + lay.cW2, lay.theta_size - 1)] == \
        ["aW1", "aW2", "abe1", "ab3", "cWs", "cW2", "cb3"]


@pytest.mark.parametrize("key", sorted(LAYOUTS))
def test_the_oracles_own_step_stays_below_4p1_lr_at_every_step_count(key):
    """One float32 oracle step (optim_oracle.adam_polyak_set) from the generated moments at each of STEP_COUNTS, with gradients over
    1e-6 .. 1 (a fifth of them exactly zero, as behind a dead relu) and the scalar hyperparameters or a row of HP_ROWS in turn:
    |w' - w| <= 4.1 lr in the actor block with actor_lr and in the critic block with critic_lr, more than half of the logical weights
    move, padded entries keep their bits and their moments stay zero."""
    ref = layout_of(key)
    lay, mask = ref.lay, _logical_mask(ref)
    T, AS = lay.theta_size, lay.actor_size
    m0, v0 = midrun_moments(mask, N, seed=7)
    rs = np.random.RandomState(8)
    conf = config.Config()
    alr_s, clr_s, tf_s, of_s = hparams_of(1, False, conf)
    alr_h, clr_h, tf_h, of_h = hparams_of(len(HP_ROWS) * HP_BLOCK, True, conf)
    assert len(set(alr_h.tolist())) == len(set(clr_h.tolist())) == len(set(tf_h.tolist())) == len(HP_ROWS) and clr_h.max() <= F(2e-3)
    worst = 0.0
    for i, count in enumerate(STEP_COUNTS):
        th, st = params.init_weights(lay, rs, dims=ref.dims)
        assert np.max(np.abs(th)) <= 2.0
        tht, stt = th.copy(), st.copy()
        g = (rs.standard_normal(T) * rs.choice(SCALES, T) * (rs.uniform(size=T) > 0.2) * mask).astype(F)
        if i % 4 == 0:
            alr, clr, tf, of = alr_s[0], clr_s[0], tf_s[0], of_s[0]
        else:
            j = (i % 4 - 1) * HP_BLOCK
            alr, clr, tf, of = alr_h[j], clr_h[j], tf_h[j], of_h[j]
        w, m, v = th.copy(), m0[i % N].copy(), v0[i % N].copy()
        oo.adam_polyak_set(w, tht, m, v, stt, st, g, count, AS, alr, clr, tf, of)
        assert np.all(np.isfinite(w)) and np.all(np.isfinite(m)) and np.all(np.isfinite(v)) and np.all(np.isfinite(tht))
        d = np.abs(w.astype(np.float64) - th.astype(np.float64))
        for lo, hi, lr in ((0, AS, alr), (AS, T, clr)):
            r = float(d[lo:hi].max() / float(lr))
            worst = max(worst, r)
            assert r <= 4.1, (key, count, lo, r)
        assert np.mean(_bits(w)[mask] != _bits(th)[mask]) > 0.5, (key, count)
        assert np.array_equal(_bits(w)[~mask], _bits(th)[~mask]) and not m[~mask].any() and not v[~mask].any()
    print(f"{key}: worst |step| / lr over STEP_COUNTS {worst:.4f} (bound 4.1)")
    assert worst > 0.5  # (the steps are not trivial either)
