"""tests/bf16_oracle.py checks itself (CPU only): the restated learn() is oracle/mlp.py bit for bit when nothing is rounded, the
rounding helper is torch.bfloat16's, the acceptance rule of tests/test_gpu_wide_tiles.py CAN fail (a 32-row tile whose gradient is
missing is rejected on the head tensors), and on the chosen seeds no tolerance reaches the cap at which it would say nothing. The
same for the agent-major cases of tests/test_gpu_fset_tiles.py (csrc/fset.hip), at 256 compute units: no tolerance at the cap, no
tensor left out, and a dropped, shifted or missing agent tile is rejected by the per-agent rule where a whole-set one lets it go."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import mlp as omlp
from tests import bf16_oracle as bo
from tests.test_oracle_mlp import _rand_nets


@pytest.mark.parametrize("S,H1,H2,Ha,B", [(4, 32, 16, 16, 24), (3, 64, 48, 8, 7)])
def test_without_rounding_the_module_is_the_oracle_bit_for_bit(S, H1, H2, Ha, B):
    nets = _rand_nets(5, S=S, H1=H1, H2=H2, Ha=Ha)
    rs = np.random.RandomState(6)
    batch = (rs.normal(0, 1.5, (B, S)), rs.uniform(-2.5, 2.5, (B, 1)), -np.abs(rs.normal(0, 0.3, (B, 1))), rs.normal(0, 1.5, (B, S)))
    cg, ag, aux = omlp.learn(batch, *nets)
    cg2, ag2, aux2 = bo.learn(batch, *nets, rnd=bo.identity)
    assert len(cg2) == 14 and len(ag2) == 10
    for x, y in zip(cg + ag, cg2 + ag2):
        assert x.shape == y.shape and np.array_equal(x, y)
    for k in aux:
        assert np.array_equal(aux[k], aux2[k]), k
    # the kernel's placements restate the same function: without rounding they differ from it by float64 summation order alone
    for placement in ("dual", "delta", "fset"):
        cgp, agp, _ = bo.learn(batch, *nets, rnd=bo.identity, placement=placement)
        assert all(np.max(np.abs(x - y)) <= 1e-12 * np.max(np.abs(x)) for x, y in zip(cg + ag, cgp + agp)), placement
    # ... and the rounding is not a no-op, and the fault handles reach the gradients they are meant for (and only those)
    cg3, ag3, _ = bo.learn(batch, *nets)
    assert all(not np.array_equal(x, y) for x, y in zip(cg + ag, cg3 + ag3))
    z = np.zeros((B, 1))
    cg4, ag4, _ = bo.learn(batch, *nets, rnd=bo.identity, da_scale=z)
    assert all(np.array_equal(x, y) for x, y in zip(cg, cg4)) and all(not np.any(g) for g in ag4)
    cg5, ag5, _ = bo.learn(batch, *nets, rnd=bo.identity, dq_scale=z)
    assert all(np.array_equal(x, y) for x, y in zip(ag, ag5)) and all(not np.any(g) for g in cg5)


def test_rounding_helper_is_torch_bfloat16():
    rs = np.random.RandomState(7)
    x = np.concatenate([
        (rs.normal(0, 1, 20000) * np.exp(rs.uniform(-80, 80, 20000))).astype(np.float32),  # the whole exponent range
        np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, 3.3895314e38, 3.4028235e38], np.float32),  # (the last two round to inf)
        # exact ties between two bf16 neighbours, even and odd lower neighbour: low half-word 0x8000, and one bit either side
        (np.arange(0x3F80, 0x3F80 + 512, dtype=np.uint32)[:, None] << np.uint32(16) | np.array([0x7FFF, 0x8000, 0x8001], np.uint32)).ravel().view(np.float32),
        # subnormals of f32 and of bf16 (exponent field 0), ties among them, the smallest normal
        np.array([0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x00028000, 0x007FFFFF, 0x007F8000, 0x00800000, 0x80008000,
                  0x80018000], np.uint32).view(np.float32),
        (rs.randint(0, 0x00800000, 2000).astype(np.uint32)).view(np.float32),
    ])
    want = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    got = bo.round_bf16(x)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.isnan(bo.round_bf16(np.array([np.nan], np.float32))[0])
    x64 = x[np.isfinite(x)].astype(np.float64)  # float64 in: through float32, float64 out, idempotent
    r64 = bo.round_bf16(x64)
    assert r64.dtype == np.float64 and np.array_equal(r64, want[np.isfinite(x)].astype(np.float64)) and np.array_equal(bo.round_bf16(r64), r64)
    n = x64.size // 6 * 6
    v = bo.round_bf16(x64[:n].reshape(-1, 6)[:, ::2].T)  # a strided view rounds like its copy
    assert v.shape == (3, n // 6) and np.array_equal(v, r64[:n].reshape(-1, 6)[:, ::2].T)


@pytest.mark.parametrize("name", [c.name for c in bo.CASES])
def test_no_tolerance_reaches_the_cap_on_the_chosen_seeds(name):
    """CPU alone: FACTOR x the pooled bf16-oracle error stays under CAP for every compared tensor, at every tile size of the case;
    at most two tensors may be left out at 32 rows, never a head tensor; the critic's seed does not cancel over the set."""
    case = bo.CASE[name]
    ms, refs, emus, tol = bo.case_reference(name)
    assert len(case.drop32) <= 2 and not set(case.drop32) & set(bo.HEADS)
    assert {m[1] for m in ms} == {32, 256, case.rows}
    for t, table in tol.items():
        for tensor, (scale, e, limit) in table.items():
            print(f"{name} t={t} {tensor}: scale {scale:.3e} e_bf16 {e:.3e} tol {limit:.3e}")
            assert scale > 0 and np.isfinite(e)
            if tensor not in bo.skipped(case, t):
                assert limit == max(bo.FLOOR, bo.FACTOR * e) and limit < bo.CAP, (name, t, tensor, e)
    for ref, emu, (_, t, _, _) in zip(refs, emus, ms):  # the rule accepts the emulation it was derived from
        assert bo.violations(emu, ref, tol[t]) == []


def _tile(case, i, j=None):
    lo = 256 * i + (0 if j is None else 32 * j)
    return lo, lo + (256 if j is None else 32)


def test_the_rule_rejects_a_256_row_tile_with_one_32_row_sub_tile_missing():
    """Hidden 1024, 256-row tile 5 of the float64 reference itself with (a) the action gradient, (b) the critic's loss seed zeroed on
    ONE 32-row sub-tile -- the fault csrc/wide.hip once had (fw::fwd_gen_kernel<true, 4>: whole 32-row tiles of the action gradient
    wrong, every whole-set tolerance still met): rejected on every head tensor of the actor / of the critic."""
    case = bo.CASE["h1024"]
    ms, refs, _, tol = bo.case_reference("h1024")
    nets, batch = bo.case_nets(case), bo.case_batch(case)
    lo, hi = _tile(case, 5)
    i = [m[2:] for m in ms].index((lo, hi))
    keep = np.ones((256, 1))
    keep[96:128] = 0
    for kw, heads in ((dict(da_scale=keep), ("aW3", "ab3", "ag2", "abe2")), (dict(dq_scale=keep), ("cW3", "cb3", "cg3", "cbe3"))):
        wrong = bo.tile_learn(case, nets, batch, lo, hi, bo.identity, **kw)
        bad = {v[0]: v for v in bo.violations(wrong, refs[i], tol[256])}
        assert set(heads) <= set(bad), (heads, bad)
        others = [n for n in bo.NAMES if n[0] != heads[0][0]]  # the other network's tensors are untouched
        assert not set(others) & set(bad)


def test_the_rule_rejects_a_32_row_tile_that_is_missing():
    """Hidden 1024, one 32-row mask: a result without the tile's action gradient / without its loss seed (zeros) is rejected on the
    actor's / the critic's head tensors, on every one of the case's 32-row masks."""
    ms, refs, _, tol = bo.case_reference("h1024")
    for (label, t, lo, hi), ref in zip(ms, refs):
        if t != 32:
            continue
        for heads in (("aW3", "ab3", "ag2", "abe2"), ("cW3", "cb3", "cg3", "cbe3")):
            wrong = {n: (np.zeros_like(g) if n[0] == heads[0][0] else g) for n, g in ref.items()}
            bad = {v[0] for v in bo.violations(wrong, ref, tol[32])}
            assert set(heads) <= bad, (label, heads, bad)


# ---- the agent-major cases (csrc/fset.hip) ------------------------------------------------------------------------------------------
CUS = 256  # the plan the CPU self-checks assume (an MI355X); the GPU test takes the device's own count
FSET_NAMES = [c.name for c in bo.FSET]


def test_the_refactored_helpers_give_the_wide_cases_their_old_tolerance_table():
    """The table of h256x128_S3 (every tile size, every tensor: scale, e_bf16, tolerance) as it was before the helpers took the set count
    and the checked sets from the case -- recorded to nine digits (another BLAS may sum in another order)."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bf16_oracle_h256x128_S3_tol.json")) as f:
        want = json.load(f)
    tol = bo.case_reference("h256x128_S3")[3]
    assert sorted(want) == sorted(str(t) for t in tol)
    for t, table in tol.items():
        for tensor in bo.NAMES:
            assert np.allclose(table[tensor], want[str(t)][tensor], rtol=1e-9, atol=0), (t, tensor)
    case = bo.CASE["h256x128_S3"]
    assert (case.n_sets, case.check) == (bo.N_SETS, (bo.CHECK_SET,))


def test_fset_cases_reach_the_paths_they_are_there_for():
    """At 256 CUs: 64 sets -> J = 4, 27 platoons, workgroups of 7, 7, 7, 6 tiles (more than NW / 2 = 4 and 6: the prefetch branch and a
    wave pair's second tile; odd and even counts for dxa's parities); 5 sets -> J = 51, 70 platoons, 19 workgroups with 2 tiles and 32
    with 1; one set -> 256 workgroups, 300 platoons. Masked platoons lie inside the set; checked sets include the first and the last."""
    tiles = lambda J, P: sorted({(P - j0 + J - 1) // J for j0 in range(J)})
    J, P, pl = bo.fset_plan("fset_64sets", CUS)
    assert (J, P) == (4, 27) and tiles(J, P) == [6, 7] and pl == list(range(27))
    J, P, pl = bo.fset_plan("fset_modelA_ragged", CUS)
    assert (J, P) == (51, 70) and tiles(J, P) == [1, 2] and pl == [0, 50, 51, 69] and P - J == 19
    J, P, pl = bo.fset_plan("fset_one_set", CUS)
    assert (J, P) == (256, 300) and tiles(J, P) == [1, 2] and pl == [0, 255, 256, 299]
    for cus in (64, 104, 256, 304):  # another part: still inside the set, still 7 tiles in the 64-set case
        for name in FSET_NAMES:
            case, (J, P, pl) = bo.fset_case(name, cus), bo.fset_plan(name, cus)
            assert pl and all(0 <= p < P for p in pl) and case.rows == 64 * P
            assert 0 in case.check and case.n_sets - 1 in case.check and case.widths == (256, 128, 48)
        J, P, _ = bo.fset_plan("fset_64sets", cus)
        assert tiles(J, P) in ([6, 7], [6]) and max(tiles(J, P)) >= 6
    s, a, r, s2 = bo.fset_batch(bo.fset_case("fset_modelA_ragged", CUS))
    assert s.shape == (350, 64, 3) and a.shape == (350, 64, 1) and r.shape == (350, 64) and s2.shape == s.shape
    sm = bo.set_major((s, a, r, s2), 5)  # agent p * M + m -> rows [64 p, 64 p + 64) of set m
    assert sm[0].shape == (5, 70 * 64, 3) and np.array_equal(sm[0][4, 64 * 69:], s[69 * 5 + 4]) and np.array_equal(sm[2][2, 64:128], r[1 * 5 + 2])


@pytest.mark.parametrize("name", FSET_NAMES)
def test_no_fset_tolerance_reaches_the_cap_and_no_tensor_is_left_out(name):
    """Every tensor of every checked set at both tile sizes (64 rows = one agent, the whole set): tolerance = max(FLOOR, FACTOR x e_bf16)
    under CAP; no skip list; the rule accepts the emulation it was derived from. The same for the general-weights reference."""
    case = bo.fset_case(name, CUS)
    assert case.drop32 == () and case.placement == ("fset" if name == "fset_64sets" else "generic")
    ms, per = bo.fset_reference(name, CUS)
    assert {m[1] for m in ms} == {64, "whole"} and sorted(per) == sorted(case.check)
    tables = [(k, t, table) for k, (_, _, tol) in per.items() for t, table in tol.items()]
    if name == "fset_64sets":
        tables += [(k, "weighted", tol) for k, (_, _, tol) in bo.fset_weighted_reference(name, CUS)[1].items()]
    for k, t, table in tables:
        assert sorted(table) == sorted(bo.NAMES)
        for tensor, (scale, e, limit) in table.items():
            print(f"{name} set {k} t={t} {tensor}: scale {scale:.3e} e_bf16 {e:.3e} tol {limit:.3e}")
            assert scale > 0 and np.isfinite(e) and limit == max(bo.FLOOR, bo.FACTOR * e) and limit < bo.CAP, (name, k, t, tensor, e)
    for k, (refs, emus, tol) in per.items():
        for ref, emu, (_, t, _, _) in zip(refs, emus, ms):
            assert bo.violations(emu, ref, tol[t]) == []


@pytest.mark.parametrize("name", FSET_NAMES)
def test_the_per_agent_rule_rejects_a_dropped_and_a_shifted_agent_tile(name):
    """For every checked set and every masked platoon p0, against the float64 reference of that mask (1 / P x learn(agent p0's rows)):
    (a) a result WITHOUT the agent's contribution (zeros: the tile was skipped) misses the rule on all 24 tensors;
    (b) the contribution of the NEIGHBOURING agent p0 + 1 in its place (a tile index off by one) misses it on cWs, cWa, cW3 and cg3 and
        on at least 14 tensors in all (19 or more in the two cases with few sets). The agents' batches are independent draws of one
        distribution, so tensors that are sums of like-signed seeds (biases, BN shifts: ab3, abe2, cb2, ..) can agree between two agents
        to within the bf16 noise of a 64-row tile; the tensors that pair the seeds with the tile's own inputs and activations do not."""
    case = bo.fset_case(name, CUS)
    _, P, _ = bo.fset_plan(name, CUS)
    ms, per = bo.fset_reference(name, CUS)
    batch = bo.set_major(bo.fset_batch(case), case.n_sets)
    for k, (refs, _, tol) in per.items():
        nets = bo.case_nets(case, k)
        for (label, t, lo, hi), ref in zip(ms, refs):
            if t != 64:
                continue
            gone = {n: np.zeros_like(g) for n, g in ref.items()}
            assert {v[0] for v in bo.violations(gone, ref, tol[64])} == set(bo.NAMES), (k, label)
            if hi < case.rows:
                shifted = bo.tile_learn(case, nets, batch, lo + 64, hi + 64, bo.identity, k=k)
                bad = {v[0] for v in bo.violations(shifted, ref, tol[64])}
                assert {"cWs", "cWa", "cW3", "cg3"} <= bad and len(bad) >= (14 if name == "fset_64sets" else 19), (k, label, sorted(bad))


def test_a_whole_set_comparison_lets_a_missing_agent_through_where_the_per_agent_masks_do_not():
    """A whole-set result that lacks ONE agent's tile (whole - 1 / P x learn(agent p0)), every p0 of every checked set.
    27 platoons (fset_64sets), under the pooled whole-set rule: rejected every time on all 14 critic tensors, and on every head tensor
    in sets 0 and 37. The heads that ESCAPE: aW3, ab3, ag2 and abe2 of set 63, for all 27 agents -- that set's actor tolerance is
    0.083 (the action gradient's coherent bf16 offset, docs/fset_tile_parity.md), more than the 1 / 27 an agent carries.
    70 platoons (fset_modelA_ragged), under the 2e-2 of each tensor's max that tests/test_gpu_fset.py allows: every head tensor of the
    faulty result PASSES, for every masked agent of both sets (an agent is 1 / 70 = 1.4 % of its set).
    The per-agent mask of the same agent rejects the missing tile on all 24 tensors (the test above): that is what the masks are for."""
    ms, per = bo.fset_reference("fset_64sets", CUS)
    for k, (refs, _, tol) in per.items():
        whole = refs[-1]
        assert ms[-1][1] == "whole"
        for (label, t, _, _), ref in zip(ms[:-1], refs):
            wrong = {n: whole[n] - ref[n] for n in bo.NAMES}
            bad = {v[0] for v in bo.violations(wrong, whole, tol["whole"])}
            assert {n for n in bo.NAMES if n[0] == "c"} <= bad, (k, label, sorted(bad))
            assert set(bo.HEADS) <= bad or (k == 63 and set(bo.HEADS) - bad == {"aW3", "ab3", "ag2", "abe2"}), (k, label, sorted(bad))
    ms, per = bo.fset_reference("fset_modelA_ragged", CUS)
    for k, (refs, _, _) in per.items():
        whole = refs[-1]
        for (label, t, _, _), ref in zip(ms[:-1], refs):
            for n in bo.HEADS:
                assert np.max(np.abs(ref[n])) <= 2e-2 * np.max(np.abs(whole[n])), (k, label, n)


def test_fset_general_weights_are_normalised_and_differ_per_platoon_and_per_set():
    """The factors of the general-weights test: w_p * P / sum(w) (mean 1 per set), 0.2 ... 3.0 over the platoons with +-20 % jitter, another
    column for every set; the rule accepts the emulation of that reference. (The platoons' batches are draws of one distribution, so the
    unweighted mean lies close to any weighted one: the per-agent masks, not this case, are the sharp test of the factor itself.)"""
    w, per = bo.fset_weighted_reference("fset_64sets", CUS)
    assert w.shape == (27, 64) and w.dtype == np.float32 and np.allclose(w.mean(axis=0), 1.0, atol=1e-6)
    assert w.min() > 0.05 and (w.max(axis=0) / w.min(axis=0)).min() > 8
    assert not np.allclose(w[:, 0], w[:, 63], rtol=1e-2)
    for k, (ref, emu, tol) in per.items():
        assert bo.violations(emu, ref, tol) == []


# ---- the forward cases of tests/test_gpu_act_shared.py (csrc/wide.hip, avd_actor_forward_shared_bf16) -----------------------------
FWD_NAMES = [c.name for c in bo.FWD_CASES]


def test_forward_cases_reach_the_kernels_they_are_there_for():
    """launch_gemm's choice restated (fwd_tile): 256-row tiles from 512 rows and 512 columns upward. The table's shapes against it: the
    last row tile is ragged everywhere, one row in one_row and past_tile, K = H1 = 64 in both k64 cases, S = 3 in modelA alone."""
    want = {"t256_ragged": (256, 512, 700), "t128_511": (128, 384, 511), "one_row": (128, 0, 1), "past_tile": (128, 128, 129),
            "modelA": (256, 512, 600), "k64_t256": (256, 512, 600), "k64_t128": (128, 128, 130)}
    assert sorted(want) == sorted(FWD_NAMES)
    for c in bo.FWD_CASES:
        assert (bo.fwd_tile(c), *bo.fwd_last_tile(c)) == want[c.name], c.name
        assert (c.P - bo.fwd_last_tile(c)[0]) % bo.fwd_tile(c) != 0 and c.S == (3 if c.name == "modelA" else 4)
        x = bo.fwd_states(c)
        assert x.shape == (c.n_sets, c.P, c.S) and x.dtype == np.float32 and x.flags.c_contiguous
    assert {c.n_sets for c in bo.FWD_CASES} == {1, 2, 3} and bo.FWD_CASE["k64_t256"].widths[0] == bo.FWD_CASE["k64_t128"].widths[0] == 64


@pytest.mark.parametrize("name", FWD_NAMES)
def test_forward_case_stays_under_the_cap_and_its_inputs_bite(name):
    """From the two oracles alone: max(FWD_TOL, FACTOR x e_max) <= FWD_CAP = 2e-2 (never looser than the one-shape test in
    tests/test_gpu_wide.py), the rms tolerance below the maximum's; the inputs-bite conditions (fwd_inputs_bite); the rule accepts
    the float64 reference and the bf16 oracle it was derived from."""
    case, fr = bo.FWD_CASE[name], bo.fwd_reference(name)
    print(f"{name}: std {case.std} seed {case.seed} e_max {fr.e_max:.3e} e_rms {fr.e_rms:.3e} tol_max {fr.tol_max:.3e} tol_rms {fr.tol_rms:.3e} "
          f"spread {np.round(fr.ref.std(axis=1) / bo.HIGH, 3)} active {np.round(fr.active1, 2)} {np.round(fr.active2, 2)}")
    assert fr.ref.shape == fr.emu.shape == (case.n_sets, case.P) and np.isfinite(fr.ref).all() and np.isfinite(fr.emu).all()
    assert fr.tol_max == max(bo.FWD_TOL, bo.FACTOR * fr.e_max) and fr.tol_rms == max(bo.FWD_TOL, bo.FACTOR * fr.e_rms)
    assert 0 < fr.e_rms <= fr.e_max and bo.FWD_TOL < fr.tol_rms <= fr.tol_max <= bo.FWD_CAP, (name, fr.tol_max)
    bo.fwd_inputs_bite(fr.ref, fr.active1, fr.active2, c0=fr.c0 if case.P == 1 else None)
    assert bo.fwd_violations(fr.ref, fr.ref, fr.tol_max, fr.tol_rms) == []
    assert bo.fwd_violations(fr.emu, fr.ref, fr.tol_max, fr.tol_rms) == []
    assert len(bo.fwd_violations(np.full_like(fr.ref, np.nan), fr.ref, fr.tol_max, fr.tol_rms)) == 2  # (a non-finite result fails)
    for k in range(case.n_sets):  # the reference is oracle/mlp.py's actor (the fold is a float64 regrouping)
        plain = omlp.actor_forward(bo.fwd_actor(case, k), fr.x[k].astype(np.float64), bo.HIGH)[:, 0]
        assert np.max(np.abs(plain - fr.ref[k])) <= 1e-9 * bo.HIGH


@pytest.mark.parametrize("name", FWD_NAMES)
def test_the_forward_rule_rejects_planted_defects(name):
    """Wrong results built from the float64 reference (no kernel): every one misses the rule, in every case where it applies.
      shifted   every row holds its neighbour's output, within a set                                   (P > 1)
      swapped   the outputs of the first two sets exchanged                                             (n_sets > 1)
    and, on the rows of the LAST set's last row tile only (128 or 256 rows as the case's GEMM takes them; 1 .. 188 rows here):
      stale     left at tanh(c0) * high, the pre-filled head sum that no atomic reached
      k_block   the layer-2 product without one 64-wide K block -- EVERY block in turn, each result rejected
      other_S   the states read as l1_fwd_kernel<the other S> reads them (fwd_other_S)"""
    case, fr = bo.FWD_CASE[name], bo.fwd_reference(name)
    lo, hi = bo.fwd_last_tile(case)
    k, w = case.n_sets - 1, bo.fwd_actor(case, case.n_sets - 1)
    wrong = {}
    if case.P > 1:
        wrong["shifted"] = np.roll(fr.ref, -1, axis=1)
    if case.n_sets > 1:
        wrong["swapped"] = fr.ref[[1, 0] + list(range(2, case.n_sets))]

    def last_tile(rows):
        out = fr.ref.copy()
        out[k, lo:hi] = rows
        return out
    wrong["stale"] = last_tile(np.tanh(fr.c0[k]) * bo.HIGH)
    for j in range(case.widths[0] // 64):
        wrong[f"k_block[{j}]"] = last_tile(bo.fwd_rows(w, fr.x[k, lo:hi], drop_k=j)[0])
    wrong["other_S"] = last_tile(bo.fwd_rows(w, bo.fwd_other_S(case, lo, hi)[k])[0])
    assert len(wrong) == 4 + case.widths[0] // 64 - (case.P == 1) - (case.n_sets == 1)
    for what, got in wrong.items():
        bad = bo.fwd_violations(got, fr.ref, fr.tol_max, fr.tol_rms)
        print(f"{name} {what}: errors {bo.fwd_errors(got, fr.ref)} tolerances {(fr.tol_max, fr.tol_rms)}")
        assert bad, (name, what, bo.fwd_errors(got, fr.ref), fr.tol_max, fr.tol_rms)
    # the rms half is what catches one wrong ROW TILE whose worst row stays inside the maximum's tolerance: the last tile of the last set
    # off by 0.9 x that tolerance passes the max half; it misses the rms half where 0.9 tol_max sqrt(the tile's share of the rows) > tol_rms
    off = last_tile(fr.ref[k, lo:hi] + 0.9 * fr.tol_max * bo.HIGH)
    bad = [b[0] for b in bo.fwd_violations(off, fr.ref, fr.tol_max, fr.tol_rms)]
    caught = 0.9 * fr.tol_max * np.sqrt((hi - lo) / (case.n_sets * case.P)) > fr.tol_rms
    assert bad == (["rms"] if caught else []) and (caught or name != "t256_ragged"), (name, bad)


@pytest.mark.parametrize("name", [c.name for c in bo.TRAINER_CASES])
def test_trainer_acting_cases_stay_under_the_cap_bite_and_reject_an_axis_swap(name):
    """The 40 rows of the trainer's acting test (8 platoons x 5 vehicles, 1024/1024): cap, inputs-bite, every action distinct, and the
    expected outputs with the P and M axes swapped (the set-major block read as agent-major) miss the rule."""
    case, fr = bo.FWD_CASE[name], bo.fwd_reference(name)
    print(f"{name}: e_max {fr.e_max:.3e} e_rms {fr.e_rms:.3e} tol_max {fr.tol_max:.3e} tol_rms {fr.tol_rms:.3e} spread {np.round(fr.ref.std(axis=1) / bo.HIGH, 3)}")
    assert (case.n_sets, case.P, case.widths) == (5, 8, (1024, 1024, 48)) and bo.fwd_tile(case) == 128
    assert bo.FWD_TOL < fr.tol_rms <= fr.tol_max <= bo.FWD_CAP
    bo.fwd_inputs_bite(fr.ref, fr.active1, fr.active2)
    assert len(np.unique(fr.ref)) == 40
    assert bo.fwd_violations(fr.emu, fr.ref, fr.tol_max, fr.tol_rms) == []
    swapped = fr.ref.reshape(case.P, case.n_sets).T
    assert len(bo.fwd_violations(swapped, fr.ref, fr.tol_max, fr.tol_rms)) == 2
    x = bo.trainer_env_states(case, np.nan)
    assert x.shape == (8, 5, 4) and np.array_equal(x[3, 2, :case.S], fr.x[2, 3]) and np.isnan(x[..., case.S:]).all()
