"""The agent-mask cases of the split set learner (csrc/fsplit.hip, avd_learn_set_split_f16x3), their conditioned batches, the float64
and float32 references and the acceptance rule of tests/test_gpu_fsplit_tiles.py (TEST INFRASTRUCTURE, CPU only; checked by
tests/test_split_tiles_cpu.py at 256 compute units).

``agent_weight`` multiplies an agent's two loss seeds in HEAD_BOTH, so weight 1 on the agents of platoon p0 and 0 elsewhere makes ONE
call return, for every weight set at once, 1 / P x learn(that agent's 64 rows). A workgroup of a set walks the platoons j0, j0 + J, ..
(J = max(1, CUs // n_sets) workgroups per set, make_plan), so platoon p0 is tile ordinal p0 // J of workgroup p0 % J. The cases below
put masks on whole workgroups of 32-33 tiles: both periods of head_kernel's 5 : 5 : 3 : 3 deal, every phase of dx_kernel's three LDS
slots and two mask buffers, dw_kernel's two staging register sets, dxa_kernel's two parities through its look-ahead, and the tile that
each of them finishes after its loop, at an odd and at an even tile count.

The rule, from the references alone -- per mask, checked set and tensor X:
    ref = float64 oracle of the masked rows x rows / (64 P)        (bf16_oracle.tile_learn(.., identity) == oracle/mlp.py)
    e32 = max |float32 NumPy oracle_X - ref_X| / max |ref_X|       (oracle.mlp.learn on float32 nets, the same rows)
    pass  <=>  max |got_X - ref_X| / max |ref_X| <= max(FLOOR, 4 x e32),   a non-finite result never passes
FLOOR = SPLIT_TOL_SMALL for a 64-row mask (the project's bar for conditioned inputs up to 4480 rows), SPLIT_TOL for a whole set and
for general weights: tests/test_gpu_fsplit.py's constants and its _errors_vs_oracle rule. One mask has no 4 x e32 clause: the 106 k-row
whole set of split_5sets_deep, where the float32 oracle itself is past SPLIT_TOL (SplitSpec.whole_clause). FLOOR_FALLBACK names the
(tile size, tensor) pairs that a correct kernel was measured to miss SPLIT_TOL_SMALL on; their floor is SPLIT_TOL
(docs/fsplit_tile_parity.md).

Relu ties: a row within float32 resolution of a relu kink has no defined float32 derivative (tests/test_gpu_fsplit.py::_untie) and is
1 / 64 of a tile, so the batch is conditioned on the host, deterministically, from the host-side weight tables: every row of a set
that gets a whole-set mask, every masked tile of the other checked sets. The GPU test and the CPU tables use this ONE batch."""
import functools
from collections import namedtuple

import numpy as np

from oracle import mlp as omlp
from tests import bf16_oracle as bo

NAMES, B = bo.NAMES, bo.FSET_B
FACTOR = 4.0
TIE, NUDGE_S, NUDGE_A, HIGH = 1e-6, np.float32(0.0173), np.float32(0.0091), 2.5  # as tests/test_gpu_fsplit.py::_untie
# (tile size, tensor) whose floor is SPLIT_TOL instead of SPLIT_TOL_SMALL: measured, named in docs/fsplit_tile_parity.md
FLOOR_FALLBACK = frozenset()

# head_kernel deals a workgroup's tiles to its four wave pairs FAST : FAST : SLOW : SLOW in periods of 2 (FAST + SLOW) ordinals
# (csrc/fsplit.hip:512-514 HEAD_FAST / HEAD_SLOW, :588-594 the map): restated, not parsed.
HEAD_FAST, HEAD_SLOW = 5, 3
HEAD_PERIOD = 2 * (HEAD_FAST + HEAD_SLOW)


def head_deal(k):
    """Tile ordinal k of a workgroup -> (period, wave pair, position in the pair's group): pairs 0, 1 take ordinals 0-4, 5-9 of a
    period of 16, pairs 2, 3 ordinals 10-12, 13-15."""
    per, m = divmod(k, HEAD_PERIOD)
    if m < 2 * HEAD_FAST:
        return per, m // HEAD_FAST, m % HEAD_FAST
    m -= 2 * HEAD_FAST
    return per, 2 + m // HEAD_SLOW, m % HEAD_SLOW


def floors():
    """(SPLIT_TOL_SMALL, SPLIT_TOL) of tests/test_gpu_fsplit.py (imported late: that module takes its tie arithmetic from here)."""
    from tests.test_gpu_fsplit import SPLIT_TOL, SPLIT_TOL_SMALL

    return SPLIT_TOL_SMALL, SPLIT_TOL


# ---- the cases ------------------------------------------------------------------------------------------------------------------
# P and the masked platoons are written through J; `whole`: the checked sets that also get the whole-set mask.
SplitSpec = namedtuple("SplitSpec", "name S n_sets seed P platoons check whole whole_clause why")


def _deep5_platoons(J, P):
    """Workgroups 0 and J - 1 at every ordinal; workgroups J // 2 - 1 (33 tiles) and J // 2 (32) at their last two."""
    out = set(range(0, P, J)) | set(range(J - 1, P, J))
    for j0 in {max(0, J // 2 - 1), J // 2}:
        out |= set(list(range(j0, P, J))[-2:])
    return out


def _from_fset(name, seed=None):
    f = bo.FSET_SPEC[name]
    return SplitSpec(f.name, f.S, f.n_sets, f.seed if seed is None else seed, f.P, f.platoons, f.check, f.check, True, f.why)


SPLIT = [
    SplitSpec("split_64sets_deep", 4, 64, 167, lambda J: 32 * J + 1, lambda J, P: (p for p in range(P) if p % J in (0, J - 1)),
              (0, 37, 63), (0, 37, 63), True,
              "workgroup 0 walks ordinals 0 .. 32 and the last workgroup 0 .. 31: both head periods of every wave pair, every dx slot "
              "and buffer phase with odd and even counts, dxa's parities through its look-ahead, the widest set stride"),
    # whole_clause = False: at 106 k rows the float32 NumPy oracle is itself 2.0e-5 ... 5.5e-5 off (seeds 167 ... 173, abe2 / ab2), so
    # 4 x e32 would loosen the whole-set mask past SPLIT_TOL; it is held to SPLIT_TOL flat, as the 4096 x 5 test of
    # tests/test_gpu_fsplit.py holds its 262 k rows. Seed: 170 and 172 of 167 ... 173 keep every 64-row 4 x e32 under SPLIT_TOL_SMALL.
    SplitSpec("split_5sets_deep", 4, 5, 172, lambda J: 32 * J + J // 2, _deep5_platoons, (0, 4), (0,), False,
              "the headline's geometry (J = 51 at 256 CUs): ragged counts 33 / 32, first and last set; the whole-set mask on set 0 only "
              "(a 106 k-row float64 oracle)"),
    _from_fset("fset_modelA_ragged"),  # S = 3; 1-2 tiles
    # every CU on one set. Its own seed: at 19 200 rows the float32 oracle's whole-set error is 4.2e-6 ... 9.4e-6 over seeds 60 ... 79
    # (FSET's 69: 6.2e-6, 4 x that is past SPLIT_TOL); 71 has the smallest, 4.2e-6 (cbe3), and 6.2e-7 on its 64-row masks.
    _from_fset("fset_one_set", seed=71),
]
SPLIT_SPEC = {c.name: c for c in SPLIT}
SPLIT_NAMES = [c.name for c in SPLIT]


def plan(name, cus):
    """(J, P, masked platoons) of a case on a device with `cus` compute units."""
    spec = SPLIT_SPEC[name]
    J = max(1, cus // spec.n_sets)
    P = spec.P(J)
    return J, P, sorted({p for p in spec.platoons(J, P) if 0 <= p < P})


def tiles_of(j0, J, P):
    """Tiles that workgroup j0 of a set walks (head_kernel: ntile)."""
    return (P - j0 + J - 1) // J if j0 < P else 0


def case(name, cus):
    """The bf16_oracle.Case of a spec (rows = 64 P per set): serves bo.case_nets, bo.tile_learn, bo.fset_batch, bo.fset_weights."""
    spec = SPLIT_SPEC[name]
    _, P, _ = plan(name, cus)
    return bo.Case(name, bo.FSET_WIDTHS, spec.S, P * B, spec.seed, spec.why, (), "generic", spec.n_sets, spec.check)


def where(p0, J, P):
    """What platoon p0 is to the kernels: (workgroup, ordinal, tiles of that workgroup, head period, wave pair, position, ordinal % 3,
    ordinal & 1, is the workgroup's final tile)."""
    j0, k = p0 % J, p0 // J
    n = tiles_of(j0, J, P)
    return (j0, k, n) + head_deal(k) + (k % 3, k & 1, k == n - 1)


def label(p0, J, P):
    j0, k, n, per, pair, pos, m3, m2, last = where(p0, J, P)
    return f"p{p0}(wg{j0},tile{k}/{n},head{per}:pair{pair}.{pos},slot{m3},buf{m2}{',final' if last else ''})"


def masks(name, cus):
    """[(label, tile size, lo, hi)] in set-major rows: the masked platoons (tile size 64), then the whole set ("whole")."""
    J, P, platoons = plan(name, cus)
    return [(label(p0, J, P), B, B * p0, B * p0 + B) for p0 in platoons] + [("whole", "whole", 0, B * P)]


# ---- relu ties ------------------------------------------------------------------------------------------------------------------
def tie_rows(an, cn, x, act, tie=TIE, high=HIGH):
    """[rows] bool: rows with a pre-activation closer to 0 than `tie` x its layer's largest over these rows, in any layer that is
    differentiated -- actor(s), critic(s, a), critic(s, mu) -- in float64. an, cn: actor and critic in Keras weight order; x [rows, S],
    act [rows, 1]."""
    W1, b1, _, _, _, _, W2, b2 = an[:8]
    z1 = x @ W1 + b1
    y1 = np.maximum(z1, 0) * omlp._bn_coeffs(*an[2:6])[0] + omlp._bn_coeffs(*an[2:6])[1]
    pre = [z1, y1 @ W2 + b2]
    mu = omlp.actor_forward(an, x, high)
    Ws, bs, Wa, ba = cn[:4]
    CW2, cb2 = cn[12], cn[13]
    ys = np.maximum(x @ Ws + bs, 0) * omlp._bn_coeffs(*cn[4:8])[0] + omlp._bn_coeffs(*cn[4:8])[1]
    pre.append(x @ Ws + bs)
    for u in (act, mu):
        za = u @ Wa + ba
        ya = np.maximum(za, 0) * omlp._bn_coeffs(*cn[8:12])[0] + omlp._bn_coeffs(*cn[8:12])[1]
        pre += [za, np.concatenate([ys, ya], axis=1) @ CW2 + cb2]
    t_ = np.zeros(len(x), bool)
    for z in pre:
        t_ |= (np.abs(z) < tie * np.abs(z).max()).any(axis=1)
    return t_


def conditioned_agents(name, cus):
    """{checked set k: agent indices whose rows are conditioned}: every agent of a set with a whole-set mask, the masked platoons' agents
    of the other checked sets."""
    spec = SPLIT_SPEC[name]
    _, P, platoons = plan(name, cus)
    return {k: np.asarray(range(P) if k in spec.whole else platoons) * spec.n_sets + k for k in spec.check}


def tie_mask(name, cus, s, a):
    """[n_agents, 64] bool: the tie rows among the conditioned agents of an agent-major batch (each checked set's agents together: the
    layer maxima are taken over them)."""
    c = case(name, cus)
    bad = np.zeros(s.shape[:2], bool)
    for k, sel in conditioned_agents(name, cus).items():
        an, cn, _, _ = bo.case_nets(c, k)
        t_ = tie_rows(an, cn, s[sel].reshape(-1, c.S).astype(np.float64), a[sel].reshape(-1, 1).astype(np.float64))
        bad[sel] = t_.reshape(len(sel), -1)
    return bad


@functools.lru_cache(maxsize=None)
def _batch(name, cus):
    c = case(name, cus)
    s, a, r, s2 = bo.fset_batch(c)
    nudged = 0
    for _ in range(8):
        bad = tie_mask(name, cus, s, a)
        if not bad.any():
            break
        nudged += int(bad.sum())
        s[bad] += NUDGE_S
        a[bad] = np.clip(a[bad] + NUDGE_A, -HIGH, HIGH)
    else:
        raise AssertionError(f"{name}: could not condition the batch")
    for x in (s, a, r, s2):
        x.setflags(write=False)
    return (s, a, r, s2), nudged


def batch(name, cus):
    """The case's conditioned batch (s, a, r, s2), AGENT-major float32 [n_agents, 64, ..], drawn as bo.fset_batch draws it and nudged as
    _untie nudges. Cached and read-only: the GPU test and every CPU table use this one."""
    return _batch(name, cus)[0]


def nudges(name, cus):
    return _batch(name, cus)[1]


@functools.lru_cache(maxsize=None)
def _set_major(name, cus):
    return bo.set_major(batch(name, cus), SPLIT_SPEC[name].n_sets)


def other_draw(name, cus):
    """An independent draw of the same distributions, agent-major (the zero-weight test's second filling of the unmasked agents)."""
    c = case(name, cus)
    return bo.fset_batch(c._replace(seed=c.seed + 5000))


# ---- references and the rule ------------------------------------------------------------------------------------------------------
def _nets32(nets):
    return tuple([w.astype(np.float32) for w in net] for net in nets)


def relerr(got, ref):
    """max |got - ref| / max |ref| (tests/test_gpu_mlp.py::_relerr), inf when `got` is not finite."""
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    return float(np.max(np.abs(got - ref)) / max(1e-12, np.max(np.abs(ref))))


@functools.lru_cache(maxsize=None)
def rows_reference(name, cus, k, lo, hi):
    """(ref, e32) of rows [lo, hi) of set k: {tensor: float64 oracle x (hi - lo) / rows}, {tensor: the float32 oracle's relative error}."""
    c = case(name, cus)
    s, a, r, s2 = _set_major(name, cus)
    nets = bo.case_nets(c, k)
    ref = bo.tile_learn(c, nets, (s, a, r, s2), lo, hi, bo.identity, k=k)
    cg, ag, _ = omlp.learn((s[k, lo:hi], a[k, lo:hi], r[k, lo:hi, None], s2[k, lo:hi]), *_nets32(nets))
    f = (hi - lo) / c.rows
    e32 = {n: relerr(f * g.astype(np.float64), ref[n]) for n, g in zip(NAMES, cg + ag)}
    for v in ref.values():
        v.setflags(write=False)
    return ref, e32


def table(tsz, e32, clause=True):
    """{tensor: (e32, limit)} of one mask: limit = max(FLOOR, 4 x e32); clause = False: FLOOR alone."""
    small, big = floors()
    return {n: (e32[n], max(big if tsz != B or (tsz, n) in FLOOR_FALLBACK else small, FACTOR * e32[n] if clause else 0.0)) for n in NAMES}


def violations(got, ref, tab):
    """[(tensor, error, limit)] of the tensors of one mask's result that miss the rule (a non-finite tensor always does)."""
    bad = []
    for n in NAMES:
        err = relerr(got[n], ref[n])
        if not err <= tab[n][1]:
            bad.append((n, err, tab[n][1]))
    return bad


def reference(name, cus):
    """-> (masks, {checked set k: [(ref, table) or None per mask]}); None where set k gets no whole-set mask."""
    spec, ms = SPLIT_SPEC[name], masks(name, cus)
    per = {}
    for k in spec.check:
        per[k] = []
        for _, tsz, lo, hi in ms:
            if tsz == "whole" and k not in spec.whole:
                per[k].append(None)
                continue
            ref, e32 = rows_reference(name, cus, k, lo, hi)
            per[k].append((ref, table(tsz, e32, tsz != "whole" or spec.whole_clause)))
    return ms, per


def round_f16(x):
    """x rounded once to fp16 (what a path that drops the lo halves of the operand pairs multiplies)."""
    return np.asarray(x).astype(np.float16).astype(np.asarray(x).dtype)


def tile_once_rounded(name, cus, k, lo, hi):
    """The tile's result with every GEMM operand rounded once to fp16: the planted defect (c)."""
    c = case(name, cus)
    return bo.tile_learn(c, bo.case_nets(c, k), _set_major(name, cus), lo, hi, round_f16, k=k)


@functools.lru_cache(maxsize=None)
def weighted_reference(name, cus):
    """-> (w [P, n_sets], {k: (ref, table)}): bo.fset_weights on both loss seeds of every row, float64 and its float32 twin; floor SPLIT_TOL."""
    c = case(name, cus)
    sm, w = _set_major(name, cus), bo.fset_weights(c)
    s, a, r, s2 = sm
    out = {}
    for k in c.check:
        nets = bo.case_nets(c, k)
        ref = bo.weighted_learn(c, nets, sm, k, w, bo.identity)
        f = np.repeat(w[:, k], B)[:, None].astype(np.float32)
        cg, ag, _ = bo.learn((s[k], a[k], r[k][:, None], s2[k]), *_nets32(nets), rnd=bo.identity, dq_scale=f, da_scale=f)
        assert all(g.dtype == np.float32 for g in cg + ag)
        out[k] = (ref, table("weighted", {n: relerr(g.astype(np.float64), ref[n]) for n, g in zip(NAMES, cg + ag)}))
    return w, out
