"""The per-agent exact-f32 learn kernels -- cen::learn_kernel_c (csrc/cen.hip, the centralized shapes) and lean::learn_kernel_l
(csrc/lean.hip, the reference widths) -- tile by tile against the float64 oracle: the cases, their conditioned batches, the float64 and
float32 references, the tile maps and the acceptance rule of tests/test_gpu_learner_tiles.py (TEST INFRASTRUCTURE, CPU only; checked by
tests/test_learner_tiles_cpu.py). Measured figures: docs/learner_tile_parity.md.

Cases: cen3 / cen5 (S, A = 12, 3 / 20, 5, widths 307 / 153 / 57 held as 320 / 160 / 64) and lean4 / lean3 (S = 4 / 3, A = 1, 256 / 128 /
48), each with 5 agents on per-agent sets (set_mod = 0) and 7 agents sharing 3 sets (set_mod = 3), 64 rows per agent, in three
variants: `plain` (tests/test_gpu_mlp.py::_perturbed_group as it is), `ladder` (BN variances, gammas and signs stepped per 16-unit
tile, LADDER below: the smallest tile of a tensor is 1 / 50 ... 1 / 1000 of its max) and `hp` (plain weights, gamma = 0.9, action_high = 1.5).

The rule, from the references alone -- per agent, gradient tensor X (on its PADDED slab extent) and tile T of the kernel's plan:
    ref      = oracle/mlp.py learn in float64
    e[T]     = max over T and N_ORD float32 evaluations of |f32 - ref|      (the given order and N_ORD - 1 relabellings: relabel())
    base[X]  = median over X's tiles of e[T]                               (a tile where float32 got lucky is not held to that)
    limit[T] = FACTOR x max(e[T], base[X])                                 (FACTOR = 4, tests/split_oracle.py)
    pass  <=>  max over T of |got - ref| <= limit[T];  a non-finite value never passes
A one-element tensor named in FALLBACK for the kernel that runs keeps tests/test_gpu_mlp.py's rule instead (GRAD_TOL of its value).

Relu ties: a row with a pre-activation within float32 resolution of a kink has no defined float32 derivative and is 1 / 64 of an
agent's gradient, so the batches are conditioned on the host as tests/split_oracle.py conditions its own (tie_rows, TIE, the same
nudge), per agent against that agent's weight set. The GPU tests and the CPU tables use this ONE batch per (case, variant, group)."""
import functools
from collections import namedtuple

import numpy as np

from avddpg_amd import config, params, vec
from oracle import mlp as omlp
from tests.split_oracle import FACTOR, NUDGE_A, NUDGE_S, TIE, tie_rows

B = 64
GRAD_TOL = 1e-4  # tests/test_gpu_mlp.py (restated: that module is a GPU test module)
N_ORD = 4  # float32 evaluations behind e[T]; evaluation N_ORD is the held-out one of the self-consistency check
A_MAX = 2.5  # the sampled actions' range (the environment's, whatever action_high the actor is scaled by)
# (kernel that runs, tensor) pairs held to GRAD_TOL of the tensor's max instead of the tile rule, where the tensor is ONE element (A = 1,
# the lean cases): b3's gradient is then a single cancelling sum over the 64 rows and e[T] the largest of N_ORD draws of ONE scalar's
# rounding error, with no other tile for the median to lean on. Measured on the MI355X: lean::learn_kernel_l misses cb3 for 1 agent
# of 72 (error / limit 1.43), the general kernel cb3 for 6 (up to 2.57) and ab3 for 1 (1.54), at errors of 1.4e-6 of the value at the
# most; both kernels pass the same tensors at A = 3 and 5. docs/learner_tile_parity.md has the figures.
FALLBACK = frozenset({("lean", "cb3"), ("general", "cb3"), ("general", "ab3")})

Case = namedtuple("Case", "name kernel S A widths hidd_mult padded seed")
REF_WIDTHS = (256, 128, 48)
CASES = [
    Case("cen3", "cen", 12, 3, REF_WIDTHS, 1.2, (320, 160, 64), 303),
    Case("cen5", "cen", 20, 5, REF_WIDTHS, 1.2, (320, 160, 64), 305),
    Case("lean4", "lean", 4, 1, REF_WIDTHS, 1, REF_WIDTHS, 315),
    Case("lean3", "lean", 3, 1, REF_WIDTHS, 1, REF_WIDTHS, 313),
]
CASE = {c.name: c for c in CASES}
VARIANTS = ("plain", "ladder", "hp")
GROUPS = ((5, 0), (7, 3))  # (agents, set_mod)
HP = dict(gamma=0.9, action_high=1.5)
# Which draw of its batch a (case, variant, set_mod) takes (default: the first). A draw is passed over when, for one of its agents, the
# float32 evaluations themselves are ill-conditioned -- a limit above 0.1 x GRAD_TOL of the tensor's max, typically a gradient that is
# proportional to a cancelling sum over the 64 rows, such as the actor's d beta2 = W3 sum_r dz3[r] at A = 1 -- or the held-out
# evaluation misses the rule: conditions on the inputs, from the references alone (tests/test_learner_tiles_cpu.py asserts them).
# (cen3 plain, shared sets: its first draw holds at 0.099 of the 0.1; the third has the most room of the first four, 0.084.)
DRAW = {("lean3", "plain", 0): 1, ("lean3", "hp", 0): 1, ("cen3", "plain", 3): 2}

# the ladder, per 16-unit tile t of every BN layer of all four networks: moving variance x var_base ^ (t % var_period - var_mid), gamma x
# (-1 if t % sign_period == sign_at else 1) x gamma_base ^ (t % gamma_period - gamma_mid), the actor head x head (not x 30), states with
# std state_std. At the lean shapes (16 and 8 tiles per layer, 32 x 32 tiles that pair them) variance steps of 4 leave the smallest W2
# tile at 1 / 15 of its tensor's max; steps of 8 bring it under 1 / 50 (tests/test_learner_tiles_cpu.py asserts the conditions).
Ladder = namedtuple("Ladder", "var_base var_period var_mid gamma_base gamma_period gamma_mid sign_period sign_at head state_std")
LADDER = {"cen": Ladder(4.0, 5, 2, 2.0, 4, 2, 3, 1, 5.0, 0.75), "lean": Ladder(8.0, 5, 2, 2.0, 4, 2, 3, 1, 5.0, 0.75)}
HEAD_PLAIN = 30.0  # _perturbed_group's factor on the actor head

NAMES = [n for n, k, _ in params.CRITIC_WEIGHTS + params.ACTOR_WEIGHTS if k == "t"]  # critic 14, actor 10: learn()'s order
W2_NAMES, BN1_NAMES, L1W_NAMES = ("aW2", "cW2"), ("ag1", "abe1", "cgs", "cbes", "cga", "cbea"), ("aW1", "cWs", "cWa")


def conf_kw(name, variant):
    H1, H2, Ha = CASE[name].widths
    kw = dict(actor_layer1_size=H1, actor_layer2_size=H2, critic_layer1_size=H1, critic_layer2_size=H2, critic_act_layer_size=Ha)
    if variant == "hp":
        kw.update(HP)
    return kw


def group_seed(name, set_mod):
    return CASE[name].seed + 20 * set_mod


def state_std(name, variant):
    """Plain: 1.5 x min(1, 2 / sqrt(S)), as tests/test_gpu_general_shapes.py draws (the x 30 actor head saturates tanh on wider inputs
    otherwise); ladder: LADDER.state_std."""
    return LADDER[CASE[name].kernel].state_std if variant == "ladder" else 1.5 * min(1.0, 2.0 / np.sqrt(CASE[name].S))


def ladder_factors(kernel, n):
    """(variance factor, gamma factor) [n] of a BN layer of n units."""
    t = np.arange(n) // 16
    L = LADDER[kernel]
    var = L.var_base ** ((t % L.var_period) - L.var_mid)
    gam = np.where(t % L.sign_period == L.sign_at, -1.0, 1.0) * L.gamma_base ** ((t % L.gamma_period) - L.gamma_mid)
    return var.astype(np.float32), gam.astype(np.float32)


# ---- weights ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def slabs(name, variant, set_mod):
    """The host half of tests/test_gpu_mlp.py::_perturbed_group(n_sets, S, seed, A, hidd_mult, **conf_kw) -- the same draws; the GPU
    test asserts the two agree bit for bit -- with the ladder on top: (group on the CPU device, conf, theta, stats, theta_t, stats_t)."""
    c = CASE[name]
    n_sets = set_mod or GROUPS[0][0]
    conf = config.Config(**conf_kw(name, variant))
    seed = group_seed(name, set_mod)
    grp = vec.AgentGroup(n_sets, c.S, c.A, conf, seed=seed, hidd_mult=c.hidd_mult, device="cpu")
    lay, dims = grp.lay, grp.dims
    assert (lay.H1, lay.H2, lay.Ha) == tuple(c.padded) and lay.B == B
    rs = np.random.RandomState(seed + 100)
    th = np.zeros((n_sets, lay.theta_size), np.float32)
    st = np.zeros((n_sets, lay.stats_size), np.float32)
    tht, stt = th.copy(), st.copy()
    ladder = variant == "ladder"
    for dst_th, dst_st in ((th, st), (tht, stt)):
        for k in range(n_sets):
            a, s_ = params.init_weights(lay, rs, dims=dims)
            aw = params.unpack(lay, a, s_, "actor", dims=dims)
            cw = params.unpack(lay, a, s_, "critic", dims=dims)
            for net, var_idx, gam_idx in ((aw, (5, 11), (2, 8)), (cw, (7, 11, 17), (4, 8, 14))):
                for w in net:
                    if w.ndim == 1:
                        w += rs.uniform(-0.3, 0.3, w.shape).astype(np.float32)
                for i in var_idx:
                    net[i][:] = np.abs(net[i]) + 0.5
                if ladder:
                    for i, gi in zip(var_idx, gam_idx):
                        fv, fg = ladder_factors(c.kernel, len(net[i]))
                        net[i][:] = net[i] * fv
                        net[gi][:] = net[gi] * fg
            aw[12] *= LADDER[c.kernel].head if ladder else HEAD_PLAIN
            cw[18] *= 300
            params.pack(lay, aw, dst_th[k], dst_st[k], "actor", dims=dims)
            params.pack(lay, cw, dst_th[k], dst_st[k], "critic", dims=dims)
    for x in (th, st, tht, stt):
        x.setflags(write=False)
    return grp, conf, th, st, tht, stt


def nets(name, variant, set_mod, k, dtype=np.float64):
    """(actor, critic, target actor, target critic) of set k in Keras weight order, logical shapes."""
    grp, _, th, st, tht, stt = slabs(name, variant, set_mod)
    u = lambda t_, s_, which: [w.astype(dtype) for w in params.unpack(grp.lay, t_[k], s_[k], which, dims=grp.dims)]
    return u(th, st, "actor"), u(th, st, "critic"), u(tht, stt, "actor"), u(tht, stt, "critic")


def set_of(v, set_mod):
    return v % set_mod if set_mod else v


def n_agents_of(set_mod):
    return next(n for n, m in GROUPS if m == set_mod)


# ---- conditioned batches ------------------------------------------------------------------------------------------------------------
def raw_batch(name, variant, set_mod):
    """The draw of tests/test_gpu_mlp.py::_central_batches at state_std."""
    c, n = CASE[name], n_agents_of(set_mod)
    rs = np.random.RandomState(group_seed(name, set_mod) + 1000 + VARIANTS.index(variant) + 50 * DRAW.get((name, variant, set_mod), 0))
    std = state_std(name, variant)
    s = rs.normal(0, std, size=(n, B, c.S)).astype(np.float32)
    a = rs.uniform(-A_MAX, A_MAX, size=(n, B, c.A)).astype(np.float32)
    r = -np.abs(rs.normal(0, 0.3, size=(n, B))).astype(np.float32)
    s2 = rs.normal(0, std, size=(n, B, c.S)).astype(np.float32)
    return s, a, r, s2


def tie_mask(name, variant, set_mod, s, a):
    """[n_agents, 64] bool: rows of agent v within TIE of a relu kink in a differentiated pass of its set's online nets."""
    conf = slabs(name, variant, set_mod)[1]
    bad = np.zeros(s.shape[:2], bool)
    for v in range(len(s)):
        an, cn, _, _ = nets(name, variant, set_mod, set_of(v, set_mod))
        bad[v] = tie_rows(an, cn, s[v].astype(np.float64), a[v].astype(np.float64), tie=TIE, high=conf.action_high)
    return bad


@functools.lru_cache(maxsize=None)
def _batch(name, variant, set_mod):
    s, a, r, s2 = raw_batch(name, variant, set_mod)
    nudged = np.zeros(s.shape[:2], bool)
    for _ in range(8):
        bad = tie_mask(name, variant, set_mod, s, a)
        if not bad.any():
            break
        nudged |= bad
        s[bad] += NUDGE_S
        a[bad] = np.clip(a[bad] + NUDGE_A, -A_MAX, A_MAX)
    else:
        raise AssertionError(f"{name} {variant} set_mod={set_mod}: could not condition the batch")
    for x in (s, a, r, s2):
        x.setflags(write=False)
    return (s, a, r, s2), nudged


def batch(name, variant, set_mod):
    """The conditioned batch (s [n, 64, S], a [n, 64, A], r [n, 64], s2 [n, 64, S]) float32, cached and read-only."""
    return _batch(name, variant, set_mod)[0]


def nudged_rows(name, variant, set_mod):
    """[n_agents, 64] bool: the rows that were moved."""
    return _batch(name, variant, set_mod)[1]


def agent_batch(name, variant, set_mod, v):
    s, a, r, s2 = batch(name, variant, set_mod)
    return s[v], a[v], r[v][:, None], s2[v]


# ---- tensors on the slab and the tile maps -------------------------------------------------------------------------------------------
Tensor = namedtuple("Tensor", "name offset shape")  # padded shape, offset into a theta-sized slab row
Plan = namedtuple("Plan", "tensors labels tile_tensor pos starts src logical theta_size")


def slab_tensors(lay):
    p = params.logical_dims(lay)
    spec = {n: (k, f) for n, k, f in params.ACTOR_WEIGHTS + params.CRITIC_WEIGHTS}
    return [Tensor(n, params._offset(lay, n, "t"), tuple(spec[n][1](p))) for n in NAMES]


def _grid(shape, tr, tc):
    return [(r0, min(r0 + tr, shape[0]), c0, min(c0 + tc, shape[1])) for r0 in range(0, shape[0], tr) for c0 in range(0, shape[1], tc)]


def cen_tiles(tensor):
    """[(label, r0, r1, c0, c1)] of a gradient tensor as cen::learn_kernel_c produces it (csrc/cen.hip, restated, not parsed; a vector
    is one row):
      aW2 / cW2     gemm_dw: items of 32 k-rows x 32 columns, item = 5 (k0 / 32) + n0 / 32, wave item % 8 (50 / 60 items)
      aW1 / cWs / cWa   l1_grads: 16 inputs x 16 columns, item = jtiles t + jt, wave item % 8
      aW3 / cW3     out_bwd: 16-row tiles t, wave t % 8 (waves 0, 1 take t and t + 8)
      ag1 abe1 / cgs cbes / cga cbea   gemm_dx_bn's epilogue: 16-column tiles t of its call, wave t % 8 (20 / 20 + 4 tiles)
      ab2 ag2 abe2 / cb2 cg3 cbe3      out_bwd's epilogue: tile t, wave t % 8 (10 tiles)
      ab1 / cbs / cba   l1_grads' column sums, one column per thread: 16 columns = a quarter of a wave
      ab3 / cb3     out_bwd's tail, threads 0 .. A - 1: one tile."""
    n, shp = tensor.name, tensor.shape
    out = []
    if n in W2_NAMES:
        for r0, r1, c0, c1 in _grid(shp, 32, 32):
            item = (shp[1] // 32) * (r0 // 32) + c0 // 32
            out.append((f"gemm_dw item {item} wave {item % 8}" + (" action rows" if r0 >= 320 else ""), r0, r1, c0, c1))
    elif n in L1W_NAMES:
        jtiles = (shp[0] + 15) // 16
        for r0, r1, c0, c1 in _grid(shp, 16, 16):
            item = jtiles * (c0 // 16) + r0 // 16
            out.append((f"l1_grads item {item} wave {item % 8} inputs {r0}:{r1}", r0, r1, c0, c1))
    elif n in ("aW3", "cW3"):
        for r0, r1, c0, c1 in _grid(shp, 16, shp[1]):
            out.append((f"out_bwd dW3 tile {r0 // 16} wave {(r0 // 16) % 8}", r0, r1, c0, c1))
    elif n in ("ab3", "cb3"):
        out.append(("out_bwd db3", 0, 1, 0, shp[0]))
    else:
        for c0 in range(0, shp[0], 16):
            t = c0 // 16
            if n in BN1_NAMES:
                lab = f"gemm_dx_bn tile {t} wave {t % 8}" + (" action branch" if n in ("cga", "cbea") else "")
            elif n in ("ab1", "cbs", "cba"):
                lab = f"l1_grads db threads {c0}:{c0 + 16} wave {(c0 % 512) // 64}"
            else:
                lab = f"out_bwd epilogue tile {t} wave {t % 8}"
            out.append((lab, 0, 1, c0, c0 + 16))
    return out


def lean_tiles(tensor):
    """lean::learn_kernel_l: 32 x 32 for the two W2 gradients, 16-wide elsewhere (not the kernel's own plan: the rule does not depend
    on it; the label is the position)."""
    n, shp = tensor.name, tensor.shape
    if len(shp) == 1:
        return [(f"[{c0}:{min(c0 + 16, shp[0])}]", 0, 1, c0, min(c0 + 16, shp[0])) for c0 in range(0, shp[0], 16)]
    tr, tc = (32, 32) if n in W2_NAMES else (16, 16)
    return [(f"[{r0}:{r1},{c0}:{c1}]", r0, r1, c0, c1) for r0, r1, c0, c1 in _grid(shp, tr, tc)]


@functools.lru_cache(maxsize=None)
def plan(name):
    """The tile plan of a case on a theta-sized slab row: tile i has label labels[i], belongs to tensors[tile_tensor[i]] and holds the
    slab positions pos[starts[i] : starts[i + 1]]. `logical`: the slab positions of the logical tensors' elements, `src` their index
    into the concatenation of learn()'s 24 flattened gradients -- both from params.pack alone."""
    grp = slabs(name, "plain", 0)[0]
    lay, dims = grp.lay, grp.dims
    tensors = slab_tensors(lay)
    labels, tile_tensor, pos, starts = [], [], [], [0]
    for ti, tz in enumerate(tensors):
        shp2 = tz.shape if len(tz.shape) == 2 else (1, tz.shape[0])
        idx = tz.offset + np.arange(int(np.prod(shp2))).reshape(shp2)
        for lab, r0, r1, c0, c1 in (cen_tiles if CASE[name].kernel == "cen" else lean_tiles)(tz):
            labels.append(f"{tz.name} {lab}")
            tile_tensor.append(ti)
            pos.append(idx[r0:r1, c0:c1].reshape(-1))
            starts.append(starts[-1] + pos[-1].size)
    # the logical elements: pack running indices (exact in float32) at two offsets; the padding's neutral values do not move
    d = params.logical_dims(lay, dims)
    packed = []
    for base in (2.0, 3.0):
        th, st, k0 = np.zeros(lay.theta_size, np.float32), np.zeros(lay.stats_size, np.float32), 0
        lists = {"critic": [], "actor": []}
        for which, spec in (("critic", params.CRITIC_WEIGHTS), ("actor", params.ACTOR_WEIGHTS)):
            for _, kind, shp in spec:
                if kind == "t":
                    n_el = int(np.prod(shp(d)))
                    lists[which].append((np.arange(k0, k0 + n_el, dtype=np.float64) + base).reshape(shp(d)).astype(np.float32))
                    k0 += n_el
        assert k0 + 3 < 2 ** 24
        for which in ("critic", "actor"):
            params.pack(lay, lists[which], th, st, which, trainable_only=True, dims=dims)
        packed.append(th)
    logical = np.flatnonzero(packed[0] != packed[1])
    src = packed[0][logical].astype(np.int64) - 2
    assert len(logical) == k0 and np.array_equal(np.sort(src), np.arange(k0))
    return Plan(tensors, labels, np.asarray(tile_tensor), np.concatenate(pos), np.asarray(starts), src, logical, lay.theta_size)


def to_slab(name, grads):
    """learn()'s 24 gradients (critic 14 + actor 10, logical shapes) -> a float64 theta-sized slab row, zeros in the padding."""
    pl = plan(name)
    flat = np.concatenate([np.asarray(g, np.float64).reshape(-1) for g in grads])
    out = np.zeros(pl.theta_size, np.float64)
    out[pl.logical] = flat[pl.src]
    return out


def tile_max(name, x):
    """Per-tile max |x| of slab rows x [..., theta_size] -> [..., n_tiles]; inf for a tile that holds a non-finite value."""
    pl = plan(name)
    v = np.abs(np.asarray(x, np.float64)[..., pl.pos])
    v = np.where(np.isfinite(v), v, np.inf)
    return np.maximum.reduceat(v, pl.starts[:-1], axis=-1)


def tensor_max(name, tiles):
    """Per-tile values [..., n_tiles] -> per-tensor max [..., 24]."""
    pl = plan(name)
    return np.stack([tiles[..., pl.tile_tensor == i].max(axis=-1) for i in range(len(pl.tensors))], axis=-1)


# ---- float32 evaluations in other summation orders ---------------------------------------------------------------------------------
def _perm_actor(w, p1, p2):
    W1, b1, g1, be1, mm1, mv1, W2, b2, g2, be2, mm2, mv2, W3, b3 = w
    return [W1[:, p1], b1[p1], g1[p1], be1[p1], mm1[p1], mv1[p1], W2[p1][:, p2], b2[p2], g2[p2], be2[p2], mm2[p2], mv2[p2], W3[p2], b3]


def _perm_critic(w, ps, pa, p2):
    Ws, bs, Wa, ba, gs, bes, mms, mvs, ga, bea, mma, mva, W2, b2, g3, be3, mm3, mv3, W3, b3 = w
    rows = np.concatenate([ps, len(ps) + pa])
    return [Ws[:, ps], bs[ps], Wa[:, pa], ba[pa], gs[ps], bes[ps], mms[ps], mvs[ps], ga[pa], bea[pa], mma[pa], mva[pa],
            W2[rows][:, p2], b2[p2], g3[p2], be3[p2], mm3[p2], mv3[p2], W3[p2], b3]


def _back(g, rows=None, cols=None):
    """The gradient of a relabelled tensor, labelled as the original: out[rows, cols] = g."""
    out = np.empty_like(g)
    if g.ndim == 1:
        out[rows] = g
    else:
        r = np.arange(g.shape[0]) if rows is None else rows
        c = np.arange(g.shape[1]) if cols is None else cols
        out[np.ix_(r, c)] = g
    return out


def relabel(batch4, nets4, seed):
    """The same function with other labels: a joint permutation of the 64 batch rows and a consistent permutation of each hidden
    layer's units (columns of the producing layer, its bias and BN vectors, rows of the consuming matrix; the critic's state and
    action branches separately; target nets with permutations of their own). -> (batch, nets, back) where back(critic_grad,
    actor_grad) returns the gradients with the original labels."""
    rs = np.random.RandomState(seed)
    s, a, r, s2 = batch4
    rows = rs.permutation(len(s))
    an, cn, tan, tcn = nets4
    h1, h2, ha = an[0].shape[1], an[6].shape[1], cn[2].shape[1]
    pa1, pa2, pcs, pca, pc2 = rs.permutation(h1), rs.permutation(h2), rs.permutation(h1), rs.permutation(ha), rs.permutation(h2)
    out = (_perm_actor(an, pa1, pa2), _perm_critic(cn, pcs, pca, pc2),
           _perm_actor(tan, rs.permutation(h1), rs.permutation(h2)), _perm_critic(tcn, rs.permutation(h1), rs.permutation(ha), rs.permutation(h2)))
    out = tuple([np.ascontiguousarray(w) for w in net] for net in out)

    def back(cg, ag):
        dWs, dbs, dWa, dba, dgs, dbes, dga, dbea, dW2, db2, dg3, dbe3, dW3, db3 = cg
        c = [_back(dWs, cols=pcs), _back(dbs, pcs), _back(dWa, cols=pca), _back(dba, pca), _back(dgs, pcs), _back(dbes, pcs),
             _back(dga, pca), _back(dbea, pca), _back(dW2, np.concatenate([pcs, h1 + pca]), pc2), _back(db2, pc2), _back(dg3, pc2),
             _back(dbe3, pc2), _back(dW3, rows=pc2), db3]
        dW1, db1, dg1, dbe1, aW2, ab2, dg2, dbe2, aW3, ab3 = ag
        a_ = [_back(dW1, cols=pa1), _back(db1, pa1), _back(dg1, pa1), _back(dbe1, pa1), _back(aW2, pa1, pa2), _back(ab2, pa2),
              _back(dg2, pa2), _back(dbe2, pa2), _back(aW3, rows=pa2), ab3]
        return c, a_

    return (s[rows], a[rows], r[rows], s2[rows]), out, back


def learn_rows(batch4, actor, critic, t_actor, t_critic, gamma, high, keep=None):
    """oracle/mlp.py learn with a 0 / 1 factor keep[r] on both loss seeds of row r (None: all ones, then it IS omlp.learn): a zeroed
    seed row is a dropped row, the means still over all 64."""
    s, a, r, s2 = batch4
    dtype = actor[0].dtype
    dt = dtype.type
    s, a, s2 = (np.asarray(v, dtype=dtype) for v in (s, a, s2))
    r = np.asarray(r, dtype=dtype).reshape(len(s), -1)
    keep = np.ones((len(s), 1), dtype) if keep is None else np.asarray(keep, dtype).reshape(len(s), 1)
    ta = omlp.actor_forward(t_actor, s2, high)
    y = r + dt(gamma) * omlp.critic_forward(t_critic, s2, ta)
    q, cc = omlp.critic_forward(critic, s, a, cache=True)
    dq = (dt(2) * (q - y) / dt(q.size)).astype(dtype) * keep
    critic_grad, _ = omlp.critic_backward(critic, cc, dq)
    a1, ac = omlp.actor_forward(actor, s, high, cache=True)
    q1, cc1 = omlp.critic_forward(critic, s, a1, cache=True)
    dq1 = np.full_like(q1, dt(-1) / dt(q1.size)) * keep
    _, da = omlp.critic_backward(critic, cc1, dq1, need_params=False)
    return critic_grad, omlp.actor_backward(actor, ac, da, high)


# ---- references and the rule ---------------------------------------------------------------------------------------------------------
Reference = namedtuple("Reference", "ref evals losses loss_tol e limit")


@functools.lru_cache(maxsize=None)
def reference(name, variant, set_mod, v):
    """Agent v of a group -> Reference: ref [theta_size] float64 slab row of the float64 oracle; evals [N_ORD + 1, theta_size] the
    float32 evaluations (the given order, then relabelled ones; the last is held out of the rule); losses (critic, actor) of the
    float64 oracle and loss_tol, max(1e-6 |loss|, FACTOR x the float32 evaluations' error); e, limit [n_tiles] of the rule."""
    conf = slabs(name, variant, set_mod)[1]
    k = set_of(v, set_mod)
    b = agent_batch(name, variant, set_mod, v)
    kw = dict(gamma=conf.gamma, high=conf.action_high)
    cg, ag, aux = omlp.learn(b, *nets(name, variant, set_mod, k), **kw)
    ref = to_slab(name, cg + ag)
    n32 = nets(name, variant, set_mod, k, np.float32)
    evals, loss_err = [], np.zeros(2)
    for i in range(N_ORD + 1):
        if i == 0:
            cg32, ag32, aux32 = omlp.learn(b, *n32, **kw)
        else:
            bp, np_, back = relabel(b, n32, 7000 + 10 * CASE[name].seed + i)
            cg32, ag32, aux32 = omlp.learn(bp, *np_, **kw)
            cg32, ag32 = back(cg32, ag32)
        assert all(g.dtype == np.float32 for g in cg32 + ag32)
        evals.append(to_slab(name, cg32 + ag32))
        if i < N_ORD:
            loss_err = np.maximum(loss_err, [abs(float(aux32[n]) - float(aux[n])) for n in ("critic_loss", "actor_loss")])
    evals = np.stack(evals)
    losses = np.array([float(aux["critic_loss"]), float(aux["actor_loss"])])
    e = tile_max(name, evals[:N_ORD] - ref).max(axis=0)
    limit = limits(name, e)
    for x in (ref, evals, e, limit):
        x.setflags(write=False)
    return Reference(ref, evals, losses, np.maximum(1e-6 * np.abs(losses), FACTOR * loss_err), e, limit)


def limits(name, e):
    """limit[T] = FACTOR x max(e[T], median of e over the tensor's tiles)."""
    pl = plan(name)
    out = np.empty_like(e)
    for i in range(len(pl.tensors)):
        sel = pl.tile_tensor == i
        out[sel] = FACTOR * np.maximum(e[sel], np.median(e[sel]))
    return out


def limit_for(name, ref, kernel=None):
    """The rule's limits for the kernel that runs ("cen", "lean", "general"; None: the rule alone): a one-element tensor named in
    FALLBACK for that kernel gets GRAD_TOL x |ref| instead."""
    pl = plan(name)
    out = ref.limit
    for i, tz in enumerate(pl.tensors):
        if (kernel, tz.name) in FALLBACK and int(np.prod(tz.shape)) == 1:
            out = out.copy()
            out[pl.tile_tensor == i] = GRAD_TOL * np.abs(ref.ref[tz.offset])
    return out


def tile_errors(name, got, ref):
    """[n_tiles] max |got - ref| per tile, inf where `got` is not finite."""
    return tile_max(name, np.asarray(got, np.float64) - ref.ref)


def violations(name, got, ref, kernel=None):
    """[(tile label, error, limit)] of the tiles of one agent's slab row that miss the rule (limit_for(kernel))."""
    err = tile_errors(name, got, ref)
    pl, limit = plan(name), limit_for(name, ref, kernel)
    return [(pl.labels[i], float(err[i]), float(limit[i])) for i in np.flatnonzero(~(err <= limit))]


def old_rule_passes(name, got, ref):
    """tests/test_gpu_mlp.py's rule without its float32 escape: every tensor within GRAD_TOL of its max."""
    err = tensor_max(name, tile_errors(name, got, ref))
    return bool(np.all(err <= GRAD_TOL * tensor_max(name, tile_max(name, ref.ref))))


def report(name, got, ref, worst, kernel=None):
    """Keeps in worst[tensor], over the agents it is called for, [largest error / limit, its tile's label, largest e32 / tensor max,
    largest error / tensor max]; the limit is the RULE's, also for a FALLBACK tensor (the figure the fallback is there for)."""
    err = tile_errors(name, got, ref)
    pl = plan(name)
    ratio = err / ref.limit
    xmax = tensor_max(name, tile_max(name, ref.ref))
    for i, tz in enumerate(pl.tensors):
        sel = np.flatnonzero(pl.tile_tensor == i)
        j = sel[np.argmax(ratio[sel])]
        w = worst.setdefault(tz.name, [-1.0, "", 0.0, 0.0])
        if ratio[j] > w[0]:
            w[0], w[1] = float(ratio[j]), pl.labels[j]
        w[2], w[3] = max(w[2], float(ref.e[sel].max() / xmax[i])), max(w[3], float(err[sel].max() / xmax[i]))
    return worst


def round_bf16(x):
    """x rounded once to bf16 (round to nearest even), in x's dtype."""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return u.view(np.float32).astype(np.asarray(x).dtype)
