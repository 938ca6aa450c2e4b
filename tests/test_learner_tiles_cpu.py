"""tests/tile_oracle.py checks itself (CPU only): the tile maps partition every gradient tensor, the conditioned inputs bite, the ladder
spreads the tiles' scales, the rule is never weaker than a tenth of tests/test_gpu_mlp.py's, a held-out float32 evaluation passes it,
and it rejects a dropped row, a shifted tile, another agent's tile, a once-rounded tile, a sentinel and -- on a small ladder tile -- a
1 % error that GRAD_TOL of the tensor's max lets through."""
import numpy as np
import pytest

from avddpg_amd import params
from oracle import mlp as omlp
from tests import tile_oracle as to
from tests.test_gpu_general_shapes import _assert_inputs_bite

CASE_NAMES = [c.name for c in to.CASES]
CASE_VARIANTS = [(c.name, v) for c in to.CASES for v in to.VARIANTS]
LADDER_TENSORS = ("aW2", "cW2", "ag1", "cgs", "aW1", "cWs")  # W2, BN1 (gamma: d beta does not scale with its own layer) and first layer


def _agents():
    return [(m, v) for n, m in to.GROUPS for v in range(n)]


def _tiles_of(pl, tensor):
    return np.flatnonzero(pl.tile_tensor == [t.name for t in pl.tensors].index(tensor))


def _pos(pl, i):
    return pl.pos[pl.starts[i]:pl.starts[i + 1]]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_tile_maps_partition_every_tensor_exactly_once(name):
    """Every element of the 24 padded gradient tensors lies in exactly one tile; what is left of the slab row is the alignment gaps; the
    logical elements (from params.pack alone) lie inside; to_slab is params.pack. cen: 50 / 60 gemm_dw items, 20 / 24 gemm_dx_bn tiles,
    10 out_bwd tiles (csrc/cen.hip's header), dealt item % 8 over the waves."""
    pl = to.plan(name)
    grp = to.slabs(name, "plain", 0)[0]
    lay = grp.lay
    count = np.bincount(pl.pos, minlength=pl.theta_size)
    extent = np.zeros(pl.theta_size, int)
    for tz in pl.tensors:
        extent[tz.offset:tz.offset + int(np.prod(tz.shape))] += 1
    assert np.array_equal(count, extent) and count.max() == 1
    assert [t.name for t in pl.tensors] == to.NAMES and len(to.NAMES) == 24
    assert count[pl.logical].all() and pl.theta_size - count.sum() < 16  # (gaps: the A-wide biases end off a 4-float boundary)
    assert len(pl.labels) == len(set(pl.labels)) == len(pl.tile_tensor) == len(pl.starts) - 1
    n_tiles = {tz.name: len(_tiles_of(pl, tz.name)) for tz in pl.tensors}
    c = to.CASE[name]
    H1, H2, Ha = c.padded
    if c.kernel == "cen":
        assert (n_tiles["aW2"], n_tiles["cW2"], n_tiles["ag1"], n_tiles["cgs"] + n_tiles["cga"], n_tiles["ag2"]) == (50, 60, 20, 24, 10)
        assert n_tiles["aW3"] == n_tiles["cW3"] == n_tiles["cb2"] == n_tiles["cg3"] == 10 and n_tiles["ab3"] == n_tiles["cb3"] == 1
        jt = (c.S + 15) // 16
        assert n_tiles["aW1"] == n_tiles["cWs"] == 20 * jt and n_tiles["cWa"] == 4
        for tensor, n in (("aW2", 50), ("cW2", 60)):
            labels = [pl.labels[i] for i in _tiles_of(pl, tensor)]
            assert [lab.split(" action")[0] for lab in labels] == [f"{tensor} gemm_dw item {i} wave {i % 8}" for i in range(n)]
            # item -> (k0, n0) as the kernel computes it: n0 = (item % 5) 32, k0 = (item / 5) 32
            for item, i in enumerate(_tiles_of(pl, tensor)):
                k0, n0 = 32 * (item // 5), 32 * (item % 5)
                tz = pl.tensors[to.NAMES.index(tensor)]
                want = tz.offset + (np.arange(k0, k0 + 32)[:, None] * H2 + np.arange(n0, n0 + 32)[None, :])
                assert np.array_equal(_pos(pl, i), want.reshape(-1))
    else:
        assert (n_tiles["aW2"], n_tiles["cW2"]) == (H1 // 32 * (H2 // 32), -(-(H1 + Ha) // 32) * (H2 // 32))  # (a last block of 16 rows)
    # to_slab against params.pack on float32 values
    rs = np.random.RandomState(1)
    d = params.logical_dims(lay, grp.dims)
    lists = {w: [rs.normal(size=shp(d)).astype(np.float32) for _, k, shp in spec if k == "t"]
             for w, spec in (("critic", params.CRITIC_WEIGHTS), ("actor", params.ACTOR_WEIGHTS))}
    th, st = np.zeros(lay.theta_size, np.float32), np.zeros(lay.stats_size, np.float32)
    for w in ("critic", "actor"):
        params.pack(lay, lists[w], th, st, w, trainable_only=True, dims=grp.dims)
    mine = to.to_slab(name, lists["critic"] + lists["actor"])
    assert np.array_equal(mine[pl.logical], th[pl.logical].astype(np.float64)) and np.count_nonzero(mine) == len(pl.logical)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_relabelling_and_the_seeded_learn_are_the_same_function(name):
    """In float64 a relabelled evaluation, labelled back, is the reference to rounding (the permutations are consistent); learn_rows
    with every row kept is omlp.learn bit for bit, in both precisions."""
    for m, v in ((0, 1), (3, 5)):
        conf = to.slabs(name, "ladder", m)[1]
        b = to.agent_batch(name, "ladder", m, v)
        n64 = to.nets(name, "ladder", m, to.set_of(v, m))
        kw = dict(gamma=conf.gamma, high=conf.action_high)
        cg, ag, _ = omlp.learn(b, *n64, **kw)
        ref = to.to_slab(name, cg + ag)
        bp, np_, back = to.relabel(b, n64, 99)
        assert not np.array_equal(bp[0], b[0]) and not np.array_equal(np_[0][6], n64[0][6])
        cgp, agp, _ = omlp.learn(bp, *np_, **kw)
        got = to.to_slab(name, sum(back(cgp, agp), []))
        scale = to.tensor_max(name, to.tile_max(name, ref))[to.plan(name).tile_tensor]
        assert np.all(to.tile_max(name, got - ref) <= 1e-11 * scale)
        for dtype in (np.float64, np.float32):
            nn = to.nets(name, "ladder", m, to.set_of(v, m), dtype)
            cg, ag, _ = omlp.learn(b, *nn, **kw)
            cg2, ag2 = to.learn_rows(b, *nn, **kw)
            assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(cg + ag, cg2 + ag2))


@pytest.mark.parametrize("name,variant", CASE_VARIANTS)
def test_inputs_bite(name, variant):
    """From the float64 oracle alone, for every agent: hidden layers 20 - 80 % active and at least half of the rows unsaturated
    (_assert_inputs_bite), no oracle gradient tensor trivial, no tie row left, at most 4 of the 64 rows nudged and nothing else moved."""
    for n, m in to.GROUPS:
        s, a, r, s2 = to.batch(name, variant, m)
        assert all(not x.flags.writeable for x in (s, a, r, s2)) and s.shape == (n, to.B, to.CASE[name].S)
        assert not to.tie_mask(name, variant, m, s, a).any()
        nud = to.nudged_rows(name, variant, m)
        raw = to.raw_batch(name, variant, m)
        moved = (s != raw[0]).any(axis=2) | (a != raw[1]).any(axis=2)
        assert not (moved & ~nud).any() and np.array_equal(r, raw[2]) and np.array_equal(s2, raw[3])
        assert nud.sum(axis=1).max() <= 4, nud.sum(axis=1)
        print(f"{name} {variant} set_mod={m}: nudged rows per agent {nud.sum(axis=1).tolist()}")
        conf = to.slabs(name, variant, m)[1]
        assert (conf.gamma, conf.action_high) == ((0.9, 1.5) if variant == "hp" else (0.99, 2.5))
        for v in range(n):
            n64 = to.nets(name, variant, m, to.set_of(v, m))
            _assert_inputs_bite(n64, s[v], a[v], (name, variant, m, v))
            cg, ag, _ = omlp.learn(to.agent_batch(name, variant, m, v), *n64, gamma=conf.gamma, high=conf.action_high)
            for g in cg + ag:
                assert np.max(np.abs(g)) > 1e-8
            assert np.array_equal(to.to_slab(name, cg + ag), to.reference(name, variant, m, v).ref)
    if variant == "hp":  # plain weights, other hyperparameters
        assert all(np.array_equal(x, y) for x, y in zip(to.slabs(name, "hp", 0)[2:], to.slabs(name, "plain", 0)[2:]))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_ladder_spreads_the_tile_scales(name):
    """In the W2, BN1 gamma and first-layer weight gradients of both nets the smallest tile maximum is at most 1 / 50 of the tensor's
    in every group (and at most 1 / 25 for every single agent); printed beside the plain variant's."""
    pl = to.plan(name)
    for n, m in to.GROUPS:
        ratios = {"ladder": [], "plain": []}
        for variant in ratios:
            for v in range(n):
                tm = to.tile_max(name, to.reference(name, variant, m, v).ref)
                ratios[variant].append([(tm[_tiles_of(pl, x)] / tm[_tiles_of(pl, x)].max()).min() for x in LADDER_TENSORS])
        lad, plain = np.array(ratios["ladder"]), np.array(ratios["plain"])
        with np.printoptions(precision=2):
            print(f"{name} set_mod={m}: smallest tile max / tensor max {LADDER_TENSORS}: ladder {lad.min(axis=0)}, its worst agent "
                  f"{lad.max(axis=0)}, plain {plain.min(axis=0)}")
        assert np.all(lad.min(axis=0) <= 1 / 50) and np.all(lad <= 1 / 25)
        assert np.all(lad.min(axis=0) < plain.min(axis=0))


@pytest.mark.parametrize("name,variant", CASE_VARIANTS)
def test_the_rule_is_never_weaker_than_a_tenth_of_GRAD_TOL_and_passes_a_held_out_float32_order(name, variant):
    """For every agent and tile: limit[T] <= 0.1 x GRAD_TOL x max |ref_X| (no FALLBACK tensor is exempt from being counted: there is
    none on the CPU side of the rule), and the float32 evaluation in a fifth order, not among the N_ORD, passes in every tile; the
    loss tolerance (1e-6 relative, or 4 x the float32 evaluations' loss error) stays a tenth of the 1e-4 x max(1, |loss|) of
    tests/test_gpu_general_shapes.py at the most."""
    pl = to.plan(name)
    worst_cap, worst_self = 0.0, 0.0
    for m, v in _agents():
        ref = to.reference(name, variant, m, v)
        assert ref.evals.shape == (to.N_ORD + 1, pl.theta_size) and not np.array_equal(ref.evals[0], ref.evals[1])
        assert np.all(ref.e > 0) and np.all(ref.limit >= to.FACTOR * ref.e)
        xmax = to.tensor_max(name, to.tile_max(name, ref.ref))[pl.tile_tensor]
        cap = ref.limit / (to.GRAD_TOL * xmax)
        assert np.all(cap <= 0.1), (m, v, pl.labels[int(np.argmax(cap))], float(cap.max()))
        held = to.tile_errors(name, ref.evals[to.N_ORD], ref) / ref.limit
        assert to.violations(name, ref.evals[to.N_ORD], ref) == [], (m, v, pl.labels[int(np.argmax(held))], float(held.max()))
        assert np.all(ref.loss_tol <= 1e-5 * np.maximum(1.0, np.abs(ref.losses))), (m, v, ref.loss_tol, ref.losses)
        worst_cap, worst_self = max(worst_cap, float(cap.max())), max(worst_self, float(held.max()))
    print(f"{name} {variant}: worst limit / (GRAD_TOL x tensor max) {worst_cap:.3f}, held-out order's worst error / limit {worst_self:.2f}")


def _with_tile(ref_slab, pl, i, values):
    out = ref_slab.copy()
    out[_pos(pl, i)] = values
    return out


def _neighbour(pl, i):
    """The next tile of the same tensor and size (the right-hand neighbour in the grid order), else the previous one."""
    for j in (i + 1, i - 1):
        if 0 <= j < len(pl.tile_tensor) and pl.tile_tensor[j] == pl.tile_tensor[i] and len(_pos(pl, j)) == len(_pos(pl, i)):
            return j
    raise AssertionError(pl.labels[i])


@pytest.mark.parametrize("name,variant", CASE_VARIANTS)
def test_the_rule_rejects_a_mutation_of_one_tile(name, variant):
    """The first, a middle and the last tile of a W2 gradient, a BN1 vector and a first-layer weight gradient of each net, one agent of
    each group; the rest of the slab row is the float64 reference itself. Each of these is rejected, in that tile and no other:
    (a) one batch row's contribution dropped (both loss seeds zeroed; row 17, or the next row that gives the tile at least 1e-3 of
    its max: a row whose relus are off in all of a tile's units adds nothing to it); (b) the tile's right-hand neighbour in its place;
    (c) the same tile of the next agent; (d) the tile rounded once to bf16; (e) the sentinel left in place (7.0, and NaN)."""
    pl = to.plan(name)
    for (n, m), v in zip(to.GROUPS, (0, 4)):
        conf = to.slabs(name, variant, m)[1]
        ref = to.reference(name, variant, m, v)
        other = to.reference(name, variant, m, (v + 1) % n).ref
        without = {}

        def dropped(row):
            if row not in without:
                keep = np.ones(to.B)
                keep[row] = 0
                cg, ag = to.learn_rows(to.agent_batch(name, variant, m, v), *to.nets(name, variant, m, to.set_of(v, m)), gamma=conf.gamma,
                                       high=conf.action_high, keep=keep)
                without[row] = to.to_slab(name, cg + ag)
            return without[row]

        assert to.violations(name, ref.ref, ref) == []
        for tensor in LADDER_TENSORS:
            tiles = _tiles_of(pl, tensor)
            for i in (tiles[0], tiles[len(tiles) // 2], tiles[-1]):
                p = _pos(pl, i)
                row = next(r for r in range(17, to.B) if np.abs(dropped(r)[p] - ref.ref[p]).max() >= 1e-3 * np.abs(ref.ref[p]).max())
                muts = {"dropped row": dropped(row)[p], "neighbour": ref.ref[_pos(pl, _neighbour(pl, i))], "next agent": other[p],
                        "bf16": to.round_bf16(ref.ref[p]), "sentinel": np.full(len(p), 7.0), "nan": np.full(len(p), np.nan)}
                for what, values in muts.items():
                    bad = to.violations(name, _with_tile(ref.ref, pl, i, values), ref)
                    assert [b[0] for b in bad] == [pl.labels[i]], (m, v, what, pl.labels[i], bad)
    assert len(to.violations(name, np.full(pl.theta_size, np.nan), ref)) == len(pl.labels)  # a non-finite value never passes


@pytest.mark.parametrize("name", CASE_NAMES)
def test_a_one_percent_error_on_a_small_ladder_tile_passes_GRAD_TOL_and_fails_the_rule(name):
    """The gap the tiles close: on the ladder, the smallest tile of each W2, BN1 gamma and first-layer weight gradient whose maximum is
    at most 1 / 100 of its tensor's (1 / 50 does not suffice for GRAD_TOL = 1e-4 to accept 1 %; every group has such tiles), scaled by
    1.01: GRAD_TOL of the tensor's max accepts the slab row, the rule rejects it in exactly that tile."""
    pl = to.plan(name)
    for (n, m) in to.GROUPS:
        done = 0
        for v in range(n):
            ref = to.reference(name, "ladder", m, v)
            tm = to.tile_max(name, ref.ref)
            for tensor in LADDER_TENSORS:
                tiles = _tiles_of(pl, tensor)
                i = tiles[np.argmin(tm[tiles])]
                if tm[i] > tm[tiles].max() / 100:
                    continue
                assert tm[i] <= tm[tiles].max() / 50
                wrong = _with_tile(ref.ref, pl, i, 1.01 * ref.ref[_pos(pl, i)])
                assert to.old_rule_passes(name, wrong, ref)
                assert [b[0] for b in to.violations(name, wrong, ref)] == [pl.labels[i]], (m, v, pl.labels[i])
                done += 1
        assert done >= 4, (m, done)
    # and GRAD_TOL's rule does reject a 1 % error on the LARGEST tile
    i = int(np.argmax(tm))
    assert not to.old_rule_passes(name, _with_tile(ref.ref, pl, i, 1.01 * ref.ref[_pos(pl, i)]), ref)


def test_the_fallback_stays_within_its_cap():
    """FALLBACK: at most 2 of the 24 gradient tensors per kernel, never a W2 gradient, only tensors of ONE element (limit_for leaves
    every other tile, and every case with A > 1, at the rule's limit), and there the limit is GRAD_TOL of the value."""
    kernels = {k for k, _ in to.FALLBACK}
    assert kernels <= {"cen", "lean", "general"}
    for k in kernels:
        named = {x for kk, x in to.FALLBACK if kk == k}
        assert len(named) <= 2 and named <= set(to.NAMES) and not named & set(to.W2_NAMES)
    for name in CASE_NAMES:
        pl = to.plan(name)
        ref = to.reference(name, "plain", 0, 0)
        assert to.limit_for(name, ref) is ref.limit
        for k in ("cen", "lean", "general"):
            lim = to.limit_for(name, ref, k)
            moved = {pl.tensors[pl.tile_tensor[i]].name for i in np.flatnonzero(lim != ref.limit)}
            want = {x for kk, x in to.FALLBACK if kk == k} if to.CASE[name].A == 1 else set()
            assert moved == want, (name, k, moved)
            for x in moved:
                tz = pl.tensors[to.NAMES.index(x)]
                assert tz.shape == (1,) and lim[_tiles_of(pl, x)[0]] == to.GRAD_TOL * abs(ref.ref[tz.offset])
