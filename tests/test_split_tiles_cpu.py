"""tests/split_oracle.py checks itself (CPU only, at 256 compute units): the cases of tests/test_gpu_fsplit_tiles.py reach the tile
ordinals they are there for, the conditioned batch holds no relu-tie row where a comparison is made, the float32-oracle clause of
the rule never loosens a mask past SPLIT_TOL, the rule rejects a dropped, a shifted and a once-rounded tile, and a once-rounded tile
that the whole-set rule lets through fails under its own mask."""
import numpy as np
import pytest

from tests import bf16_oracle as bo
from tests import split_oracle as so

CUS = 256  # the plan these self-checks assume (an MI355X); the GPU test takes the device's own count


def test_split_cases_reach_the_tile_ordinals_they_are_there_for():
    """64 sets: J = 4, P = 129, workgroups of 33, 32, 32, 32 tiles, 65 masks on workgroups 0 and 3 = ordinals 0 .. 32 and 0 .. 31.
    5 sets: J = 51, P = 1657, 25 workgroups of 33 tiles and 26 of 32; workgroups 0 and 50 at every ordinal, 24 and 25 at their last two.
    Over a deep case's masks: every (wave pair, position) of both head periods (csrc/fsplit.hip:512-514, 588-594), every ordinal % 3
    and ordinal & 1, and a workgroup's final tile at an even and at an odd ordinal (odd and even tile counts)."""
    assert [so.head_deal(k) for k in (0, 4, 5, 9, 10, 12, 13, 15, 16, 25, 26, 31, 32)] == [
        (0, 0, 0), (0, 0, 4), (0, 1, 0), (0, 1, 4), (0, 2, 0), (0, 2, 2), (0, 3, 0), (0, 3, 2), (1, 0, 0), (1, 1, 4), (1, 2, 0), (1, 3, 2), (2, 0, 0)]
    # next_tile of the kernel, restated: a pair's ordinals are start, .., start + cnt - 1, then + PERIOD
    for pair, (start, cnt) in enumerate(((0, 5), (5, 5), (10, 3), (13, 3))):
        k, pos, seen = start, 0, []
        while k < 48:
            seen.append(k)
            k, pos = (k + so.HEAD_PERIOD - cnt + 1, 0) if pos + 1 == cnt else (k + 1, pos + 1)
        assert seen == [k for k in range(48) if so.head_deal(k)[1] == pair]
        assert [so.head_deal(k)[2] for k in seen] == list(range(cnt)) * 3

    J, P, pl = so.plan("split_64sets_deep", CUS)
    assert (J, P, len(pl)) == (4, 129, 65) and [so.tiles_of(j, J, P) for j in range(J)] == [33, 32, 32, 32]
    assert sorted(p // J for p in pl if p % J == 0) == list(range(33)) and sorted(p // J for p in pl if p % J == J - 1) == list(range(32))
    assert {p % J for p in pl} == {0, J - 1}
    J, P, pl = so.plan("split_5sets_deep", CUS)
    assert (J, P, len(pl)) == (51, 1657, 69) and [so.tiles_of(j, J, P) for j in range(J)] == [33] * 25 + [32] * 26
    by_wg = {j: sorted(p // J for p in pl if p % J == j) for j in {p % J for p in pl}}
    assert by_wg == {0: list(range(33)), 50: list(range(32)), 24: [31, 32], 25: [30, 31]}
    for name in ("split_64sets_deep", "split_5sets_deep"):
        J, P, pl = so.plan(name, CUS)
        w = [so.where(p, J, P) for p in pl]
        deals = {(per, pair, pos) for _, _, _, per, pair, pos, _, _, _ in w}
        assert {(per,) + so.head_deal(k)[1:] for per in (0, 1) for k in range(16)} <= deals and len(deals) == 33
        assert {(m3, m2) for *_, m3, m2, _ in w} == {(i, j) for i in range(3) for j in range(2)}
        assert {(n & 1, m2) for _, _, n, _, _, _, _, m2, last in w if last} == {(1, 0), (0, 1)}  # final tile: odd count / even ordinal, and v.v.
        assert all(lab.startswith(f"p{p}(wg{p % J},tile{p // J}/") for p, (lab, *_) in zip(pl, so.masks(name, CUS)))
    # the two cases taken over from bf16_oracle.FSET: as there
    for name in ("fset_modelA_ragged", "fset_one_set"):
        assert so.plan(name, CUS) == bo.fset_plan(name, CUS) and so.case(name, CUS).S == bo.FSET_SPEC[name].S
        assert so.SPLIT_SPEC[name].check == so.SPLIT_SPEC[name].whole == bo.FSET_SPEC[name].check
    assert so.case("fset_modelA_ragged", CUS).S == 3
    for cus in (64, 104, 256, 304):  # another part: the masks stay inside the set, the deep cases stay deep
        for name in so.SPLIT_NAMES:
            c, (J, P, pl) = so.case(name, cus), so.plan(name, cus)
            assert pl and all(0 <= p < P for p in pl) and c.rows == 64 * P and J == max(1, cus // c.n_sets)
            assert 0 in c.check and c.n_sets - 1 in c.check and set(so.SPLIT_SPEC[name].whole) <= set(c.check)
            if name.startswith("split_"):
                assert max(so.tiles_of(j, J, P) for j in range(J)) == 33 and sorted(p // J for p in pl if p % J == 0) == list(range(33))


@pytest.mark.parametrize("name", so.SPLIT_NAMES)
def test_no_tie_row_is_left_where_a_comparison_is_made(name):
    """The conditioned batch: no row of a masked tile of a checked set, and no row at all of a set with a whole-set mask, lies within
    1e-6 of its layer's largest pre-activation of a relu kink (float64, host-side weights); only such rows were moved, by _untie's
    nudge; rewards and next states are the draw's."""
    s, a, r, s2 = so.batch(name, CUS)
    c = so.case(name, CUS)
    assert not so.tie_mask(name, CUS, s, a).any()
    raw = bo.fset_batch(c)
    moved = (s != raw[0]).any(axis=(1, 2)) | (a != raw[1]).any(axis=(1, 2))
    allowed = np.zeros(len(s), bool)
    for sel in so.conditioned_agents(name, CUS).values():
        allowed[sel] = True
    assert not (moved & ~allowed).any() and np.array_equal(r, raw[2]) and np.array_equal(s2, raw[3])
    rows = int(((s != raw[0]).any(axis=2) | (a != raw[1]).any(axis=2)).sum())
    print(f"{name}: {so.nudges(name, CUS)} nudges on {rows} rows of {int(allowed.sum()) * 64} conditioned")
    assert 0 < rows <= so.nudges(name, CUS) and rows < 0.01 * allowed.sum() * 64
    assert all(not x.flags.writeable for x in (s, a, r, s2))


@pytest.mark.parametrize("name", so.SPLIT_NAMES)
def test_the_float32_clause_never_loosens_a_mask_past_SPLIT_TOL(name):
    """4 x e32 <= SPLIT_TOL for every checked set, mask and tensor (and for the general-weights reference of the 64-set case): the clause
    cannot pass what the file's documented bar would not. The one mask without the clause (split_5sets_deep's 106 k-row whole set, where
    the float32 oracle itself is past SPLIT_TOL) has limit SPLIT_TOL exactly. Every 64-row limit is SPLIT_TOL_SMALL or 4 x e32."""
    small, big = so.floors()
    spec = so.SPLIT_SPEC[name]
    ms, per = so.reference(name, CUS)
    assert sorted(per) == sorted(spec.check) and [m[1] for m in ms] == [64] * (len(ms) - 1) + ["whole"]
    worst = {}
    items = [(k, tsz, it) for k, lst in per.items() for (_, tsz, _, _), it in zip(ms, lst)]
    if name == "split_64sets_deep":
        items += [(k, "weighted", it) for k, it in so.weighted_reference(name, CUS)[1].items()]
    n_whole = 0
    for k, tsz, it in items:
        if it is None:
            assert tsz == "whole" and k not in spec.whole
            continue
        n_whole += tsz == "whole"
        ref, tab = it
        assert sorted(tab) == sorted(ref) == sorted(so.NAMES)
        for tensor, (e32, limit) in tab.items():
            assert np.max(np.abs(ref[tensor])) > 0 and np.isfinite(e32)
            worst[(str(tsz), tensor)] = max(worst.get((str(tsz), tensor), 0.0), e32)
            if tsz == "whole" and not spec.whole_clause:
                assert limit == big
                continue
            assert limit == max(small if tsz == 64 and (tsz, tensor) not in so.FLOOR_FALLBACK else big, 4 * e32)
            assert 4 * e32 <= big, (name, k, tsz, tensor, e32)
    assert n_whole == len(spec.whole)
    for (tsz, tensor), e in sorted(worst.items(), key=lambda kv: (kv[0][0], so.NAMES.index(kv[0][1]))):
        print(f"{name} t={tsz} {tensor}: worst e32 {e:.3e}")


def _first_middle_last(ms):
    tiles = [i for i, m in enumerate(ms) if m[1] == 64]
    return [tiles[0], tiles[len(tiles) // 2], tiles[-1]]


@pytest.mark.parametrize("name", so.SPLIT_NAMES)
def test_the_rule_rejects_a_dropped_a_shifted_and_a_once_rounded_tile(name):
    """The first, a middle and the last masked tile of every checked set, against that mask's reference and limits:
    (a) zeros (the tile was dropped) miss on all 24 tensors;
    (b) the reference of platoon p0 + J, the same workgroup's next tile (p0 - J for a workgroup's final tile), misses on cWs, cWa, cW3
        and cg3 -- the tensors that pair the seeds with the tile's own inputs -- and on at least 20 tensors;
    (c) the tile with every GEMM operand rounded ONCE to fp16 (the lo halves of the pairs dropped: a forgotten cross term) misses on
        at least 20 tensors."""
    J, P, _ = so.plan(name, CUS)
    ms, per = so.reference(name, CUS)
    for k, lst in per.items():
        for i in _first_middle_last(ms):
            label, _, lo, hi = ms[i]
            ref, tab = lst[i]
            gone = {n: np.zeros_like(g) for n, g in ref.items()}
            assert {v[0] for v in so.violations(gone, ref, tab)} == set(so.NAMES), (k, label)
            d = so.B * J if hi + so.B * J <= so.B * P else -so.B * J
            assert lo + d >= 0
            shifted = so.rows_reference(name, CUS, k, lo + d, hi + d)[0]
            bad = {v[0] for v in so.violations(shifted, ref, tab)}
            assert {"cWs", "cWa", "cW3", "cg3"} <= bad and len(bad) >= 20, (k, label, sorted(bad))
            bad = so.violations(so.tile_once_rounded(name, CUS, k, lo, hi), ref, tab)
            print(f"{name} set {k} {label}: once-rounded tile misses on {len(bad)} tensors, error / limit {min(e / l for _, e, l in bad):.1f} ... {max(e / l for _, e, l in bad):.0f}")
            assert len(bad) >= 20, (k, label, [n for n in so.NAMES if n not in {v[0] for v in bad}])
    nan = {n: np.full_like(g, np.nan) for n, g in ref.items()}
    assert len(so.violations(nan, ref, tab)) == 24  # a non-finite result is a violation


def _planted_in_the_mean(name, k):
    """Per masked tile of set k: (label, tensors missed under its own mask, its worst error / limit there, tensors missed by the
    whole-set reference with this ONE tile replaced by its once-rounded version, the worst error / limit there)."""
    ms, per = so.reference(name, CUS)
    whole, wtab = per[k][-1]
    assert ms[-1][1] == "whole"
    out = []
    for (label, _, lo, hi), (ref, tab) in zip(ms[:-1], per[k]):
        wrong = so.tile_once_rounded(name, CUS, k, lo, hi)
        diluted = {n: whole[n] + (wrong[n] - ref[n]) for n in so.NAMES}
        out.append((label, len(so.violations(wrong, ref, tab)), max(so.relerr(wrong[n], ref[n]) / tab[n][1] for n in so.NAMES),
                    len(so.violations(diluted, whole, wtab)), max(so.relerr(diluted[n], whole[n]) / wtab[n][1] for n in so.NAMES)))
    return out


def test_a_once_rounded_tile_passes_in_the_whole_set_mean_and_fails_under_its_own_mask():
    """The gap the masks close, on split_5sets_deep (the headline's geometry, 1657 platoons), set 0: the whole-set reference with ONE
    tile replaced by its once-rounded-to-fp16 version (defect (c)) meets the whole-set rule -- SPLIT_TOL of each tensor's max, what
    tests/test_gpu_fsplit.py::_errors_vs_oracle asks at least -- on all 24 tensors for more than half of the 69 masked tiles, the first
    tile of workgroup 0 among them; every one of those tiles misses the rule under its own mask on at least 20 tensors.
    (split_64sets_deep, 129 platoons: next test.)"""
    res = _planted_in_the_mean("split_5sets_deep", 0)
    through = [r for r in res if r[3] == 0]
    print(f"split_5sets_deep set 0: {len(through)} of {len(res)} once-rounded tiles pass in the whole-set mean; worst error / limit there "
          f"{min(r[4] for r in res):.2f} ... {max(r[4] for r in res):.2f}, under their own masks {min(r[2] for r in res):.0f} ... {max(r[2] for r in res):.0f}")
    assert 2 * len(through) > len(res) and all(r[1] >= 20 for r in res)
    assert res[0][0].startswith("p0(wg0,tile0/33") and res[0][3] == 0 and res[0][1] >= 20


def test_at_129_platoons_the_whole_set_rule_sees_a_once_rounded_tile_two_orders_of_magnitude_more_weakly_than_its_mask():
    """split_64sets_deep, every masked tile of sets 0, 37 and 63. At 1 / 129 the same defect does NOT slip through the whole-set rule: it
    misses there on 1 ... 20 tensors, by 1.1 ... 60 x the limit (measured; the dilution is 1 / 129 of the tile's gradient, but relative to
    the max of a MEAN over 129 tiles, which is several times smaller than 129 x a tile's share). Under its own mask it misses on at least
    23 tensors and by at least 100 x as large a factor of the limit: a defect a hundredth the size of this one is still caught by the
    mask and long gone from the mean."""
    for k in so.SPLIT_SPEC["split_64sets_deep"].whole:
        res = _planted_in_the_mean("split_64sets_deep", k)
        print(f"split_64sets_deep set {k}: in the mean {min(r[3] for r in res)} ... {max(r[3] for r in res)} tensors miss, error / limit "
              f"{min(r[4] for r in res):.2f} ... {max(r[4] for r in res):.1f}; under the own mask {min(r[1] for r in res)} ... 24 tensors, "
              f"{min(r[2] for r in res):.0f} ... {max(r[2] for r in res):.0f}; smallest ratio of the two factors {min(r[2] / r[4] for r in res):.0f}")
        assert all(r[1] >= 23 and r[3] < r[1] and r[2] >= 100 * r[4] for r in res)
