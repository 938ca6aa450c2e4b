"""tests/bf16_oracle.py checks itself (CPU only): the restated learn() is oracle/mlp.py bit for bit when nothing is rounded, the
rounding helper is torch.bfloat16's, the acceptance rule of tests/test_gpu_wide_tiles.py CAN fail (a 32-row tile whose gradient is
missing is rejected on the head tensors), and on the chosen seeds no tolerance reaches the cap at which it would say nothing."""
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
    for placement in ("dual", "delta"):
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
