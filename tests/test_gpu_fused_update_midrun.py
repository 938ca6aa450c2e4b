"""The fused learn + update entry points (avd_learn_update[_act][_hp]_f32: learn + Adam x 2 + Polyak (+ next action) in one call) in the
MIDDLE of a run: moments in progress, a different Adam iteration count on every agent, two consecutive updates. Every other test of
these paths starts from m = v = 0, takes at most six steps and gives every agent the same count, so a kernel that reads another
agent's count, a step size that is off only where 1 - beta^t rounds to 1 or beta^t is subnormal, an actor / critic step-size mix-up at
a block boundary, or an element whose v is large against g^2 passes them. tests/test_gpu_optim_kernels.py pins csrc/adam.h's rule to
the float32 oracle at such counts, but on the kernels of the unfused entry points and on one small layout; the update arithmetic of
the fused call runs elsewhere:

  case                          kernels whose update arithmetic it reaches                    reached by
  lean S=4,3 (shipped)          lean.hip learn_kernel_l<.., FUSED>: the AdamSink epilogues    count: 36 agents, 25 of them at STEP_COUNTS,
    plain / next action          of gemm_dw_dx (both W2) and the small-tensor loop at the      the others over five decades; moment scale:
    HP twin / HP + next action   kernel's end; HP twins: step sizes and tau from the sweep     1e-6 / 1e-3 / 1 per element, so actor and
                                 table inside the kernel (rows change every 4 agents)          critic alphas act on every scale
  fast S=4,3 (diagnostic,       mlp.hip fast::learn_kernel_t<.., true>: the W2 epilogues;     count, moment scale (the small tensors'
    AVD_LEARN_KERNEL=fast)       optim.hip adam_polyak_ranges_kernel for the small tensors      compact index crosses the actor / critic
    plain / next action                                                                         boundary inside a block)
  general, reference widths     mlp.hip gen::learn_kernel_g<true>: the W2 epilogues;          count, moment scale
    (diagnostic,                 adam_polyak_ranges_kernel
    AVD_LEARN_GENERAL=1)
  general, padded 100/50/20     the same two on the SHIPPED path; the skip ranges move with   count, moment scale; padding: m = v = 0 and
    -> 112/64/32, S=3            the widths                                                     a zero gradient keep padded units' bits
    plain / next action
  general, A > 1: S=8 A=2       the same two, shipped, at 320/160/64 (ranges kernel with a    count, moment scale
    x 1.2                        grid of several blocks per agent)
  centralized L=3,5 (shipped)   cen.hip cen_launch_update: the chunk pipeline hands           chunk boundary: chunk + 44 agents (chunk from
                                 step + lo to optim.hip adam_polyak_rows_kernel (whole rows,   avd_learn_update_plan) = two chunks, the
                                 clamped look-ahead loads)                                      second ragged, counts differ across it
  centralized, strided rows     the same with AVD_CEN_CHUNK=40 AVD_CEN_GROUPS=7               stride: 7 workgroups walk 40 rows (`set +=
    L=3 (diagnostic)             (100 agents: chunks 40 / 40 / 20)                             gridDim.x` six times, the last ragged); chunk
                                                                                                boundaries at 40 and 80

The state (midrun_moments / midrun_counts below; tests/test_fused_midrun_state_cpu.py asserts its properties without a GPU): weights
and BN statistics of _perturbed_group; on the logical elements v = scale^2 U(0, 1.5) with scale in {1e-6, 1e-3, 1} per element and
m = c sqrt(v), c ~ U(-1, 1); every 97th element fresh (m = v = 0); padding m = v = 0. With |m| <= sqrt(v) one step moves a weight by
at most lr (0.9 / 0.9995 + 0.1 / sqrt(0.001)) < 4.1 lr (the bias correction never enlarges the step), so the weights stay
conditioned for the second step. Counts: STEP_COUNTS of the optimiser test and its _steps recipe, shuffled over the agents;
AgentGroup adds 1 before the launch, so step is loaded with count - 1. 2^31 - 1 is the last count an int32 holds: its agent starts at
2^31 - 2 and reaches it in the second update. The second update reads the ping-ponged slab and carries agents over 164 -> 165,
986 -> 987, 17320 -> 17321 and 103921 -> 103922. The agents on either side of a chunk boundary hold a pair of BOUNDARY_COUNTS (164 |
986 at the first). From t = 17321 on every count gives lr itself, so what has to differ between agents is the STEP SIZE: each case
asserts, from the oracle alone, that reading step[0], the count of the same position in the first chunk or the count of the
workgroup's first row would change the step size of more than half of the agents it touches (assert_counts_expose_index_defects).

For each of the two updates group A takes learn_update(...), its twin B (identical state) learn(...) then apply(...):
 1. A equals B bit for bit (uint32 views): theta, theta_t, stats_t, m, v, step, losses, and the next actions equal B.actor(next, 0);
 2. A equals the float32 oracle (tests/optim_oracle.adam_polyak_set) applied on the host to the pre-step state with B's gradient slab
    at the agent's own count and (actor_lr, critic_lr, tau, 1 - tau) -- every agent at one of STEP_COUNTS and the agents on either
    side of every chunk boundary;
 3. the test can bite: everything finite, more than half of the logical weights change per step, padded entries of theta, theta_alt,
    m and v keep their bits, stats does not move, _assert_inputs_bite for three agents per step, >= 20 distinct counts per case.
The HP twins: B holds the same sweep table (set_hparams), the oracle takes each agent's own row. No tolerance anywhere."""
import collections
import ctypes as C
import types

import numpy as np
import pytest
import torch

from avddpg_amd import _hip, params, vec
from oracle import mlp as omlp
from tests import optim_oracle as oo
from tests.gpu_util import need_gpu, t
from tests.test_gpu_general_shapes import REF, Shape, _assert_inputs_bite, _batches, _logical_mask, _width_kw, _x_scale
from tests.test_gpu_mlp import _nets, _perturbed_group
from tests.test_gpu_optim_kernels import HP_BLOCK, STEP_COUNTS, _steps

pytestmark = pytest.mark.gpu
F = np.float32
INT32_MAX = 2**31 - 1
FRESH_EVERY = 97
SCALES = (1e-6, 1e-3, 1.0)
MIN_STEP_SIZES = 18  # the 18 counts of STEP_COUNTS below 17321 give 18 different step sizes (from 17321 on: lr itself)
# the sweep table of the HP twins: agent j takes row (j // HP_BLOCK) % 3 (actor_lr, critic_lr <= 2e-3, tau and gamma all differ)
HP_ROWS = [dict(actor_lr=1e-4, critic_lr=1e-3, tau=0.005, gamma=0.99), dict(actor_lr=3e-4, critic_lr=2e-4, tau=0.01, gamma=0.9),
           dict(actor_lr=5e-5, critic_lr=2e-3, tau=0.001, gamma=0.95)]
KERNELS = ("lean", "fast", "cen", "general")  # AVD_LEARN_* of include/avddpg_hip.h, 0 upwards

# S, A, logical widths, hidd_mult -> padded widths
LAYOUTS = {
    "ref4": (4, 1, REF, 1, REF), "ref3": (3, 1, REF, 1, REF), "padded3": (3, 1, (100, 50, 20), 1, (112, 64, 32)),
    "a2": (8, 2, REF, 1.2, (320, 160, 64)), "cen3": (12, 3, REF, 1.2, (320, 160, 64)), "cen5": (20, 5, REF, 1.2, (320, 160, 64)),
}


# ---- the mid-run state: host side, numpy, seeded -----------------------------------------------------------------------------------

def layout_of(key):
    """(lay, dims, Shape) of a LAYOUTS row as AgentGroup builds them: logical widths int(w * hidd_mult), slabs at the padded widths."""
    S, A, widths, mult, padded = LAYOUTS[key]
    dims = params.Dims(S, A, *(int(w * mult) for w in widths))
    assert params.padded_widths(dims.H1, dims.H2, dims.Ha) == tuple(padded)
    lay = _hip.make_layout(S, A, *padded, 64)
    return types.SimpleNamespace(lay=lay, dims=dims, shape=Shape(S, A, widths, mult, padded, 0, False))


BOUNDARY_COUNTS = [(164, 986), (17320, 58), (103921, 9)]  # what the agents on either side of the first, second, .. chunk boundary hold


def midrun_counts(n_agents, seed, boundaries=()):
    """The Adam iteration count of every agent's FIRST update: every one of STEP_COUNTS, then _steps' spread over five decades,
    shuffled over the agents. 2^31 - 1 becomes 2^31 - 2: that agent reaches the last int32 count in the second update.
    boundaries: first agents of the chunks after the first; the agents b - 1 and b swap places with the holders of a pair of
    BOUNDARY_COUNTS, so that across every chunk boundary the counts differ by a step size far from 1 ulp and the second update
    carries one of 164 -> 165, 17320 -> 17321, 103921 -> 103922 over it."""
    assert n_agents >= len(STEP_COUNTS) and len(boundaries) <= len(BOUNDARY_COUNTS)
    c = _steps(np.random.RandomState(seed), n_agents).astype(np.int64)
    c[c == INT32_MAX] = INT32_MAX - 1
    for b, pair in zip(boundaries, BOUNDARY_COUNTS):
        for pos, val in zip((b - 1, b), pair):
            j = int(np.nonzero(c == val)[0][0])
            c[[pos, j]] = c[[j, pos]]
    return c.astype(np.int32)


def oracle_agents(counts, boundaries=()):
    """The agents checked against the oracle: those whose first or second update is at one of STEP_COUNTS, and the agents on either
    side of every chunk boundary."""
    at = np.isin(counts.astype(np.int64), STEP_COUNTS) | np.isin(counts.astype(np.int64) + 1, STEP_COUNTS)
    sides = [a for b in boundaries for a in (b - 1, b)]
    return np.unique(np.concatenate([np.nonzero(at)[0], np.array(sides, np.int64)])).astype(np.int64)


def alpha_bits(counts, lr):
    """the oracle's bias-corrected step size of every agent at its count, as bits"""
    return np.array([omlp.adam_alpha(lr, int(c)) for c in counts], F).view(np.uint32)


def wrong_count_agents(n_agents, chunk=None, groups=None):
    """Stand-ins for the index defects this state is built to expose: for every agent, the agent whose count a defective kernel
    would read instead -- step[0]; with chunks of `chunk` agents the same position of the FIRST chunk (a launcher that drops
    `step + lo`); with `groups` persistent workgroups per chunk the row its workgroup walked first (a count read once, outside
    the `set += gridDim.x` loop). {name: int64 [n_agents]}; an agent that maps to itself is not affected."""
    a = np.arange(n_agents, dtype=np.int64)
    out = {"step[0]": np.zeros(n_agents, np.int64)}
    if chunk is not None:
        lo = a // chunk * chunk
        out["step of the first chunk"] = a - lo
        out["step of the workgroup's first row"] = lo + (a - lo) % groups
    return out


def assert_counts_expose_index_defects(counts, lr, chunk=None, groups=None):
    """Each stand-in of wrong_count_agents changes the STEP SIZE (not only the count: from t = 17321 on every count gives lr itself)
    of more than half of the agents it affects. Returns the number of distinct step sizes."""
    ab = alpha_bits(counts, lr)
    for name, wrong in wrong_count_agents(len(counts), chunk, groups).items():
        hit = wrong != np.arange(len(counts))
        if hit.any():
            frac = float(np.mean(ab[hit] != ab[wrong[hit]]))
            assert frac > 0.5, (name, frac)
    return len(set(ab.tolist()))


def midrun_moments(mask, n_agents, seed):
    """(m, v) [n_agents, theta_size] of a run in progress. On the logical elements (mask): v = scale^2 U(0, 1.5) with scale drawn per
    element from SCALES, m = c sqrt(v) with c ~ U(-1, 1), so |m| <= sqrt(v) (float32: |c| < 1 and the product rounds to at most the
    float32 root). Every 97th element of a row is fresh, m = v = 0; padded entries m = v = 0. v = 0 with m != 0 never occurs."""
    rng = np.random.default_rng(seed)
    shape = (n_agents, mask.size)
    scale = np.array(SCALES, F)[rng.integers(0, len(SCALES), shape, dtype=np.uint8)]
    v = scale * scale * (F(1.5) * rng.random(shape, dtype=F))
    c = F(2) * rng.random(shape, dtype=F) - F(1)
    m = c * np.sqrt(v)
    for x in (m, v):
        x[:, ::FRESH_EVERY] = 0
        x[:, ~mask] = 0
    assert m.dtype == F and v.dtype == F
    return m, v


def hparams_of(n_agents, hp, conf):
    """(actor_lr, critic_lr, tau, 1 - tau) of every agent as float32 vectors: conf's scalars, or the agent's row of HP_ROWS"""
    rows = [HP_ROWS[(j // HP_BLOCK) % len(HP_ROWS)] if hp else dict(actor_lr=conf.actor_lr, critic_lr=conf.critic_lr, tau=conf.tau)
            for j in range(n_agents)]
    return (np.array([r["actor_lr"] for r in rows], F), np.array([r["critic_lr"] for r in rows], F),
            np.array([oo.tau_pair(r["tau"])[0] for r in rows], F), np.array([oo.tau_pair(r["tau"])[1] for r in rows], F))


def tensor_at(lay, flat):
    """name of the slab tensor a flat theta index falls in (its alignment gap included)"""
    names = ["aW1", "ab1", "ag1", "abe1", "aW2", "ab2", "ag2", "abe2", "aW3", "ab3", "cWs", "cbs", "cgs", "cbes", "cWa", "cba", "cga",
             "cbea", "cW2", "cb2", "cg3", "cbe3", "cW3", "cb3"]
    offs = sorted((getattr(lay, n) + (lay.actor_size if n.startswith("c") else 0), n) for n in names)
    return [n for o, n in offs if o <= flat][-1]


# ---- the cases ---------------------------------------------------------------------------------------------------------------------

Case = collections.namedtuple("Case", "layout kernel n diag env seed")
LEAN = [pytest.param(Case(f"ref{S}", "lean", 36, False, {}, 300 + S), hp, act, id=f"lean-S{S}-{'hp' if hp else 'scalar'}{'-act' if act else ''}")
        for S in (4, 3) for hp in (False, True) for act in (False, True)]
FAST = [pytest.param(Case(f"ref{S}", "fast", 32, True, {"AVD_LEARN_KERNEL": "fast"}, 310 + S), False, act, id=f"fast-S{S}{'-act' if act else ''}")
        for S in (4, 3) for act in (False, True)]
GENERAL = [
    pytest.param(Case("ref4", "general", 32, True, {"AVD_LEARN_GENERAL": "1"}, 321), False, False, id="general-ref-S4"),
    pytest.param(Case("padded3", "general", 32, False, {}, 322), False, False, id="general-padded-S3"),
    pytest.param(Case("padded3", "general", 32, False, {}, 323), False, True, id="general-padded-S3-act"),
    pytest.param(Case("a2", "general", 26, False, {}, 324), False, False, id="general-S8-A2"),
]
CEN_EXTRA = 44  # agents past the first chunk
CEN = [
    pytest.param(Case("cen3", "cen", None, False, {}, 333), False, False, id="cen-L3-two-chunks"),
    pytest.param(Case("cen5", "cen", None, False, {}, 335), False, False, id="cen-L5-two-chunks"),
    pytest.param(Case("cen3", "cen", 100, True, {"AVD_CEN_CHUNK": "40", "AVD_CEN_GROUPS": "7"}, 343), False, False, id="cen-L3-strided-rows"),
]


def _plan(lay, n_agents):
    ch, nch, groups = C.c_int(0), C.c_int(0), C.c_int(0)
    _hip.call("avd_learn_update_plan", C.byref(lay), n_agents, C.byref(ch), C.byref(nch), C.byref(groups))
    return ch.value, nch.value, groups.value


def _ibits(x):
    return x.view(torch.int32)


def _assert_same_bits(name, xa, xb, counts, k, lay):
    """device tensors [n_agents, ...] bit for bit; the message names the first differing agent, its Adam count and the tensor"""
    a, b = _ibits(xa).reshape(xa.shape[0], -1), _ibits(xb).reshape(xb.shape[0], -1)
    if torch.equal(a, b):
        return
    agent, flat = torch.nonzero(a != b)[0].tolist()
    where = tensor_at(lay, flat) if a.shape[1] == lay.theta_size else "-"
    pytest.fail(f"update {k}: {name} differs in {int((a != b).sum())} elements of {int((a != b).any(dim=1).sum())} agents; first: agent "
                f"{agent} (Adam count {int(counts[agent]) + k}) flat index {flat} ({where}; actor block {flat < lay.actor_size}): "
                f"{a[agent, flat].item() & 0xffffffff:#010x} against {b[agent, flat].item() & 0xffffffff:#010x}")


def _load(grp, state):
    for name, x in state.items():
        getattr(grp, name).copy_(x)


@pytest.mark.parametrize("case,hp,act", LEAN + FAST + GENERAL + CEN)
def test_fused_update_midrun_is_learn_then_apply_and_the_oracle_bit_for_bit(case, hp, act, request, monkeypatch):
    """One row of the table in the module docstring: two consecutive fused updates from the mid-run state, each compared with
    learn + apply on a twin (all agents, every state tensor, losses, next actions) and with the float32 oracle (the agents at
    STEP_COUNTS and at the chunk boundaries), bit for bit; then the conditions without which that could pass vacuously."""
    need_gpu()
    if case.diag:
        request.getfixturevalue("diag_lib")
        for key, val in case.env.items():
            monkeypatch.setenv(key, val)
    ref = layout_of(case.layout)
    sh, lay = ref.shape, ref.lay
    kern = C.c_int(-1)
    _hip.call("avd_learn_kernel", C.byref(lay), int(hp), C.byref(kern))
    assert KERNELS[kern.value] == case.kernel

    # the agents, and where the chunk pipeline cuts them
    n, boundaries = case.n, []
    if case.kernel == "cen":
        if n is None:
            n = _plan(lay, 1)[0] + CEN_EXTRA  # (the chunk is a property of the device: one learn workgroup per CU)
        chunk, n_chunks, groups = _plan(lay, n)
        if case.diag:
            assert (chunk, n_chunks, groups) == (40, 3, 7)
        else:
            assert n_chunks == 2 and n == chunk + CEN_EXTRA and CEN_EXTRA < chunk and groups >= chunk
        boundaries = list(range(chunk, n, chunk))

    # group A from _perturbed_group, the mid-run moments and counts on top; B its twin
    conf, ga = _perturbed_group(n, S=sh.S, seed=case.seed, A=sh.A, hidd_mult=sh.hidd_mult, **_width_kw(sh.widths))
    gb = vec.AgentGroup(n, sh.S, sh.A, conf, hidd_mult=sh.hidd_mult)
    assert bytes(ga.lay) == bytes(lay) == bytes(gb.lay) and tuple(ga.dims) == tuple(ref.dims)
    T, AS = lay.theta_size, lay.actor_size
    mask_h = _logical_mask(ga)
    m0, v0 = midrun_moments(mask_h, n, case.seed)
    counts = midrun_counts(n, case.seed, boundaries)
    assert len(set(counts.tolist())) >= 20 and set(STEP_COUNTS) <= set(counts.tolist()) | set((counts.astype(np.int64) + 1).tolist())
    n_alpha = assert_counts_expose_index_defects(counts, conf.actor_lr, *((chunk, groups) if boundaries else ()))
    assert n_alpha >= MIN_STEP_SIZES
    for b in boundaries:  # the counts, and the step sizes, differ across every chunk boundary
        assert counts[b - 1] != counts[b] and len(set(alpha_bits(counts[b - 1:b + 1], conf.actor_lr).tolist())) == 2
    ga.m.copy_(t(m0)), ga.v.copy_(t(v0)), ga.step.copy_(torch.from_numpy(counts - 1).cuda())
    start = {name: getattr(ga, name).clone() for name in ("theta", "stats", "theta_t", "stats_t", "m", "v", "step")}
    _load(gb, start)
    if hp:
        for g in (ga, gb):
            g.set_hparams(vec.hparams_table(vec.hparams_rows(conf, HP_ROWS), conf.ou_dt, "cuda"), len(HP_ROWS), HP_BLOCK)
    alr, clr, tau_f, omt_f = hparams_of(n, hp, conf)
    mask = torch.from_numpy(mask_h).cuda()
    pad = ~mask
    assert int(pad.sum()) > (64 if tuple(sh.padded) != tuple(ref.dims)[2:] else 0)
    sel_h = oracle_agents(counts, boundaries)
    sel = torch.from_numpy(sel_h).cuda()
    assert len(sel_h) >= len(STEP_COUNTS) and all(a in sel_h for b in boundaries for a in (b - 1, b))
    bite_agents = (0, n // 2, n - 1)

    f32 = dict(dtype=torch.float32, device="cuda")
    scratch, gbuf = torch.zeros(n, T, **f32), torch.zeros(n, T, **f32)
    la, lb = torch.zeros(n, 2, **f32), torch.zeros(n, 2, **f32)
    xs = float(_x_scale(sh.S))
    for k in range(2):
        b = _batches(sh, n, case.seed + 10 + k)
        nxt_h = np.random.RandomState(case.seed + 20 + k).normal(0, 1.5, size=(n, 4 if sh.S == 3 else sh.S)) * xs  # (S = 3: rows of 4)
        nxt = t(nxt_h.astype(F))
        s_h, a_h = b[0].cpu().numpy(), b[1].cpu().numpy()
        for agent in bite_agents:
            _assert_inputs_bite(_nets(ga, agent, np.float64), s_h[agent], a_h[agent], (case.layout, k, agent))
        pre = {name: getattr(ga, name)[sel].cpu().numpy() for name in ("theta", "theta_t", "m", "v", "stats", "stats_t")}
        theta_before = ga.theta.clone()

        if act:
            out = torch.full((n,), 7.0, **f32)
            ga.learn_update(*b, scratch, losses=la, next_states=nxt, next_actions=out)
        else:
            ga.learn_update(*b, scratch, losses=la)
        gb.learn(*b, 0, grads=gbuf, losses=lb)
        gb.apply(gbuf)
        torch.cuda.synchronize()

        # 1. A equals B, bit for bit
        for name in ("theta", "theta_t", "stats_t", "m", "v"):
            _assert_same_bits(name, getattr(ga, name), getattr(gb, name), counts, k, lay)
        want_step = torch.from_numpy(counts + k).cuda()
        assert torch.equal(ga.step, want_step) and torch.equal(gb.step, want_step), k
        _assert_same_bits("losses", la, lb, counts, k, lay)
        if act:
            want = gb.actor(nxt, 0)
            _assert_same_bits("next actions", out.reshape(n, 1), want.reshape(n, 1), counts, k, lay)
            assert bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0.05 and float(out.abs().max()) <= conf.action_high

        # 2. A equals the float32 oracle on the pre-step state with B's gradients, at each agent's own count and hyperparameters
        g_sel = gbuf[sel].cpu().numpy()
        got = {name: getattr(ga, name)[sel].cpu().numpy() for name in ("theta", "theta_t", "m", "v", "stats_t")}
        for i, agent in enumerate(sel_h):
            o = {name: pre[name][i].copy() for name in pre}
            oo.adam_polyak_set(o["theta"], o["theta_t"], o["m"], o["v"], o["stats_t"], o["stats"], g_sel[i], int(counts[agent]) + k, AS,
                               alr[agent], clr[agent], tau_f[agent], omt_f[agent])
            for name in ("theta", "m", "v", "theta_t", "stats_t"):
                bad = np.nonzero(got[name][i].view(np.uint32) != o[name].view(np.uint32))[0]
                assert bad.size == 0, (f"update {k}: {name} of agent {agent} (Adam count {int(counts[agent]) + k}) differs from the float32 "
                                       f"oracle in {bad.size} elements; first: flat index {bad[0]} "
                                       f"({tensor_at(lay, int(bad[0])) if name != 'stats_t' else '-'}): "
                                       f"{got[name][i][bad[0]]!r} against {o[name][bad[0]]!r}")

        # 3. the test can bite
        for x in (ga.theta, ga.theta_t, ga.stats_t, ga.m, ga.v, la):
            assert bool(torch.isfinite(x).all())
        changed = float((_ibits(ga.theta)[:, mask] != _ibits(theta_before)[:, mask]).float().mean())
        print(f"MIDRUN {request.node.callspec.id} update {k}: {n} agents, chunk boundaries {boundaries}, {n_alpha} step sizes, "
              f"{len(sel_h)} agents against the oracle, {changed:.3f} of the logical weights changed")
        assert changed > 0.5, (k, changed)
        for name, x in (("theta", ga.theta), ("theta_alt", ga.theta_alt), ("m", ga.m), ("v", ga.v)):
            x0 = start["theta" if name == "theta_alt" else name]
            assert torch.equal(_ibits(x)[:, pad], _ibits(x0)[:, pad]), (k, name)  # padded entries keep their bits
        assert torch.equal(_ibits(ga.stats), _ibits(start["stats"])) and torch.equal(_ibits(gb.stats), _ibits(start["stats"]))
        assert torch.equal(_ibits(ga.theta_alt), _ibits(theta_before))  # the update wrote the other slab: every pass read this one
    assert not bool((start["m"][:, pad] != 0).any()) and not bool((start["v"][:, pad] != 0).any())
