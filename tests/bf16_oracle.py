"""A bf16-operand restatement of oracle/mlp.py's learn(), the tile-mask cases of the shared-set learner (csrc/wide.hip) and the
acceptance rule that tests/test_gpu_wide_tiles.py holds the kernels to (TEST INFRASTRUCTURE, CPU only, no GPU and no library call
beyond the layout).

learn() below is oracle/mlp.py's learn() with one change: every matrix product goes through ``mm(x, w) = rnd(x) @ rnd(w)``. With
``rnd = round_bf16`` both operands of every product are rounded to bf16 (round to nearest even) and everything else -- the
accumulation, the biases, the BN tables, relu, tanh, the column sums -- stays float64: what a correct implementation on bf16 matrix
cores with ideal accumulation computes, up to WHERE it places its roundings. With ``rnd = identity`` it is oracle/mlp.py bit for
bit (tests/test_bf16_oracle_cpu.py). ``dq_scale`` / ``da_scale`` multiply the critic's loss seed / the action gradient row by row:
the handle the self-checks use to build a wrong result (a tile whose gradient is missing).

The acceptance rule (tolerances()): for tensor X over the masks of one case and tile size,
    scale  = max over the masks of max |ref_X|                       (free of one tile's cancellation: cb3, ab3 are one element)
    e_bf16 = max over the masks of max |bf16oracle_X - ref_X| / scale
    pass  <=>  max |got_X - ref_X| / scale <= max(FLOOR, FACTOR * e_bf16)   on every mask
FLOOR = 1e-4 is the f32 accumulation-order floor (tests/test_gpu_mlp.py GRAD_TOL), FACTOR = 4 the margin for "the error a correct
lower-precision implementation makes" (tests/test_gpu_mlp.py:112) -- a different placement of the roundings, another summation
order. Nothing measured from a kernel enters it. CAP: a tolerance above 0.5 would pass a wholly wrong tile (error O(1)); the CPU
suite asserts that no compared tensor of any case reaches it.

The second half holds the agent-major cases of tests/test_gpu_fset_tiles.py (csrc/fset.hip): masks of one agent's 64-row tile through
agent_weight, every checked set with its own tables, and placement="fset" for the case that needed it (docs/fset_tile_parity.md)."""
import functools
from collections import namedtuple

import numpy as np

from oracle import mlp as omlp

NAMES = ["cWs", "cbs", "cWa", "cba", "cgs", "cbes", "cga", "cbea", "cW2", "cb2", "cg3", "cbe3", "cW3", "cb3",
         "aW1", "ab1", "ag1", "abe1", "aW2", "ab2", "ag2", "abe2", "aW3", "ab3"]
HEADS = ("aW3", "ab3", "ag2", "abe2", "cW3", "cb3", "cg3", "cbe3")
FLOOR, FACTOR, CAP = 1e-4, 4.0, 0.5


def identity(x):
    return x


def round_bf16(x):
    """x -> float32 -> bf16 (round to nearest, ties to even; subnormals kept, inf/nan kept), returned in x's dtype."""
    x = np.asarray(x)
    f = np.ascontiguousarray(x, dtype=np.float32)
    b = f.view(np.uint32)
    r = ((b + (np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xFFFF0000)).view(np.float32)
    r = np.where(np.isfinite(f), r, f)
    return r.astype(x.dtype if x.dtype.kind == "f" else np.float32)


# ---- oracle/mlp.py's forward / backward / learn with the product as a parameter -------------------------------------------------
def _layer2(p, inv, sh, W2, b2, mm, fold):
    """Second layer on the first layer's BN output p * inv + sh. fold: as csrc/wide.hip places it (prep_w2_kernel, bias2_kernel) --
    inv folded into W2 BEFORE the rounding, the relu'd p as the other operand, sh . W2 in the (unrounded) bias."""
    if fold:
        return mm(p, inv[:, None] * W2) + (b2 + sh @ W2)
    return mm(p * inv + sh, W2) + b2


def actor_forward(w, s, high, mm, fold=False, mmx=None):
    """mmx: the product of the first and the output layer (default: mm; placement "fset": exact)."""
    W1, b1, g1, be1, mm1, mv1, W2, b2, g2, be2, mm2, mv2, W3, b3 = w
    mmx = mm if mmx is None else mmx
    dt = W1.dtype.type
    s = np.asarray(s, dtype=W1.dtype)
    p1 = np.maximum(mmx(s, W1) + b1, 0)
    i1, sh1 = omlp._bn_coeffs(g1, be1, mm1, mv1)
    y1 = p1 * i1 + sh1
    p2 = np.maximum(_layer2(p1, i1, sh1, W2, b2, mm, fold), 0)
    i2, sh2 = omlp._bn_coeffs(g2, be2, mm2, mv2)
    y2 = p2 * i2 + sh2
    t = np.tanh(mmx(y2, W3) + b3)
    return t * dt(high), (s, p1, y1, p2, y2, t)


def critic_forward(w, s, a, mm, fold=False, mmx=None):
    Ws, bs, Wa, ba, gs, bes, mms, mvs, ga, bea, mma, mva, W2, b2, g3, be3, mm3, mv3, W3, b3 = w
    mmx = mm if mmx is None else mmx
    s = np.asarray(s, dtype=Ws.dtype)
    a = np.asarray(a, dtype=Ws.dtype)
    ps = np.maximum(mmx(s, Ws) + bs, 0)
    is_, shs = omlp._bn_coeffs(gs, bes, mms, mvs)
    ys = ps * is_ + shs
    pa = np.maximum(mmx(a, Wa) + ba, 0)
    ia, sha = omlp._bn_coeffs(ga, bea, mma, mva)
    ya = pa * ia + sha
    c = np.concatenate([ys, ya], axis=1)
    p2 = np.maximum(_layer2(np.concatenate([ps, pa], axis=1), np.concatenate([is_, ia]), np.concatenate([shs, sha]), W2, b2, mm, fold)
                    if fold else mm(c, W2) + b2, 0)
    i3, sh3 = omlp._bn_coeffs(g3, be3, mm3, mv3)
    y2 = p2 * i3 + sh3
    return mmx(y2, W3) + b3, (s, a, ps, pa, c, p2, y2)


def _fset_layers12_backward(x, p1, inv1, sh1, bn1, W2, dz2, fs):
    """The second and first layer's backward pass as csrc/fset.hip places its roundings (dw_kernel, dx_kernel, finalize_*): dZ2 rounded
    ONCE and used everywhere (its column sums are db2), dW2 = inv1 (.) bf16(P1)^T dZ2 + sh1 (x) db2 from the relu'd first layer rounded
    once, dC = dZ2 . bf16(W2)^T; BN sums of the first layer from the unrounded dC and P1; the masked dC rounded once before it meets
    the (exact, split) inputs: dW1 = inv1 (.) x^T bf16(dC mask). -> (dW1, db1, dg1, dbe1, dW2, db2, unrounded dz1)."""
    dz2 = fs(dz2)
    db2 = dz2.sum(axis=0)
    dW2 = inv1[:, None] * (fs(p1).T @ dz2) + sh1[:, None] * db2[None, :]
    dc = dz2 @ fs(W2).T
    dg1, dbe1, dz1 = omlp._bn_backward(dc, p1, *bn1)
    v = fs(dc * (p1 > 0))
    return inv1[None, :] * (x.T @ v), inv1 * v.sum(axis=0), dg1, dbe1, dW2, db2, dz1


def critic_backward(w, cache, dq, mm, need_params=True, fs=None):
    """fs: None, or the rounding of placement "fset" (output layer exact, the rest: _fset_layers12_backward)."""
    Ws, bs, Wa, ba, gs, bes, mms, mvs, ga, bea, mma, mva, W2, b2, g3, be3, mm3, mv3, W3, b3 = w
    s, a, ps, pa, c, p2, y2 = cache
    h1 = Ws.shape[1]
    if fs is not None:
        dW3, db3 = y2.T @ dq, dq.sum(axis=0)
        dg3, dbe3, dz2 = omlp._bn_backward(dq @ W3.T, p2, g3, mm3, mv3)
        (is_, shs), (ia, sha) = omlp._bn_coeffs(gs, bes, mms, mvs), omlp._bn_coeffs(ga, bea, mma, mva)
        dWa, dba, dga, dbea, dW2a, db2, dza = _fset_layers12_backward(a, pa, ia, sha, (ga, mma, mva), W2[h1:], dz2, fs)
        da = dza @ Wa.T  # (head_kernel's action-gradient epilogue: the masked dC and inv_a wa meet in f32)
        if not need_params:
            return None, da
        dWs, dbs, dgs, dbes, dW2s, _, _ = _fset_layers12_backward(s, ps, is_, shs, (gs, mms, mvs), W2[:h1], dz2, fs)
        return [dWs, dbs, dWa, dba, dgs, dbes, dga, dbea, np.concatenate([dW2s, dW2a], axis=0), db2, dg3, dbe3, dW3, db3], da
    dW3 = mm(y2.T, dq)
    db3 = dq.sum(axis=0)
    dy2 = mm(dq, W3.T)
    dg3, dbe3, dz2 = omlp._bn_backward(dy2, p2, g3, mm3, mv3)
    dW2 = mm(c.T, dz2)
    db2 = dz2.sum(axis=0)
    dc = mm(dz2, W2.T)
    dga, dbea, dza = omlp._bn_backward(dc[:, h1:], pa, ga, mma, mva)
    dWa = mm(a.T, dza)
    dba = dza.sum(axis=0)
    da = mm(dza, Wa.T)
    if not need_params:
        return None, da
    dgs, dbes, dzs = omlp._bn_backward(dc[:, :h1], ps, gs, mms, mvs)
    dWs = mm(s.T, dzs)
    dbs = dzs.sum(axis=0)
    return [dWs, dbs, dWa, dba, dgs, dbes, dga, dbea, dW2, db2, dg3, dbe3, dW3, db3], da


def actor_backward(w, cache, dout, high, mm, fs=None):
    W1, b1, g1, be1, mm1, mv1, W2, b2, g2, be2, mm2, mv2, W3, b3 = w
    dt = W1.dtype.type
    s, p1, y1, p2, y2, t = cache
    dz3 = dout * dt(high) * (dt(1) - t * t)
    if fs is not None:
        dW3, db3 = y2.T @ dz3, dz3.sum(axis=0)
        dg2, dbe2, dz2 = omlp._bn_backward(dz3 @ W3.T, p2, g2, mm2, mv2)
        i1, sh1 = omlp._bn_coeffs(g1, be1, mm1, mv1)
        dW1, db1, dg1, dbe1, dW2, db2, _ = _fset_layers12_backward(s, p1, i1, sh1, (g1, mm1, mv1), W2, dz2, fs)
        return [dW1, db1, dg1, dbe1, dW2, db2, dg2, dbe2, dW3, db3]
    dW3 = mm(y2.T, dz3)
    db3 = dz3.sum(axis=0)
    dy2 = mm(dz3, W3.T)
    dg2, dbe2, dz2 = omlp._bn_backward(dy2, p2, g2, mm2, mv2)
    dW2 = mm(y1.T, dz2)
    db2 = dz2.sum(axis=0)
    dy1 = mm(dz2, W2.T)
    dg1, dbe1, dz1 = omlp._bn_backward(dy1, p1, g1, mm1, mv1)
    dW1 = mm(s.T, dz1)
    db1 = dz1.sum(axis=0)
    return [dW1, db1, dg1, dbe1, dW2, db2, dg2, dbe2, dW3, db3]


def _action_gradient(critic, cache, dq1, rnd, placement):
    """d q(s, mu) / d mu as csrc/wide.hip's forward kernels form it (one action, tools/dual_emul.py): from the EXACT relu mask of the
    second layer and cf = inv3 W3, never through a rounded gradient matrix --
      dual  (fw::fwd_gen_kernel<true, 4>): E = (mask . bf16(cf)) @ bf16(inv_a W2[action rows])^T, da = d sum_f pos Wa E
      delta (fw::fwd_delta_kernel):        E = mask @ bf16(cf W2[action rows])^T,                 da = d sum_f pos (inv_a Wa) E"""
    Ws, bs, Wa, ba, gs, bes, mms, mvs, ga, bea, mma, mva, W2, b2, g3, be3, mm3, mv3, W3, b3 = critic
    s, a, ps, pa, c, p2, y2 = cache
    ia, _ = omlp._bn_coeffs(ga, bea, mma, mva)
    i3, _ = omlp._bn_coeffs(g3, be3, mm3, mv3)
    assert W3.shape[1] == 1 and Wa.shape[0] == 1
    cf, mask, pos, W2a = i3 * W3[:, 0], (p2 > 0).astype(p2.dtype), (pa > 0).astype(pa.dtype), W2[Ws.shape[1]:]
    if placement == "dual":
        E = (mask * rnd(cf)[None, :]) @ rnd(ia[:, None] * W2a).T
        return dq1 * (pos * Wa[0][None, :] * E).sum(axis=1, keepdims=True)
    E = mask @ rnd(cf[None, :] * W2a).T
    return dq1 * (pos * (ia * Wa[0])[None, :] * E).sum(axis=1, keepdims=True)


def learn(batch, actor, critic, t_actor, t_critic, gamma=0.99, high=2.5, rnd=round_bf16, dq_scale=None, da_scale=None,
          placement="generic"):
    """oracle/mlp.py learn() with mm(x, w) = rnd(x) @ rnd(w). dq_scale / da_scale [rows, 1]: factors on the critic's loss seed /
    on the action gradient the actor's backward pass starts from (None: untouched).
    placement: "generic" -- both operands of every ``@`` of oracle/mlp.py as written; "dual" / "delta" -- two roundings moved to where
    csrc/wide.hip documents them: the BN scale folded into W2 before rounding in every forward pass (_layer2), and the critic's
    action gradient in the named kernel's form (_action_gradient). Everything else stays generic.
    "fset" -- csrc/fset.hip's arithmetic: first layers exact (split operands, 2^-16) and the output layer in f32 (no rounding in
    either), the BN scale folded into W2 before rounding with the folded bias exact (a bf16 pair), the relu'd first layer and dZ2
    rounded once (_fset_layers12_backward)."""
    assert placement in ("generic", "dual", "delta", "fset")
    fold = placement != "generic"
    mm = lambda x, w: np.matmul(rnd(x), rnd(w))
    mmx, fs = (np.matmul, rnd) if placement == "fset" else (None, None)
    s, a, r, s2 = batch
    dtype = actor[0].dtype
    dt = dtype.type
    s, a, s2 = (np.asarray(v, dtype=dtype) for v in (s, a, s2))
    r = np.asarray(r, dtype=dtype).reshape(len(s), -1)
    ta, _ = actor_forward(t_actor, s2, high, mm, fold, mmx)
    y = r + dt(gamma) * critic_forward(t_critic, s2, ta, mm, fold, mmx)[0]
    q, cc = critic_forward(critic, s, a, mm, fold, mmx)
    n = dt(q.size)
    critic_loss = np.mean(np.square(y - q))
    dq = (dt(2) * (q - y) / n).astype(dtype)
    if dq_scale is not None:
        dq = dq * dq_scale
    critic_grad, _ = critic_backward(critic, cc, dq, mm, fs=fs)
    a1, ac = actor_forward(actor, s, high, mm, fold, mmx)
    q1, cc1 = critic_forward(critic, s, a1, mm, fold, mmx)
    actor_loss = -np.mean(q1)
    dq1 = np.full_like(q1, dt(-1) / dt(q1.size))
    if placement in ("dual", "delta"):
        da = _action_gradient(critic, cc1, dq1, rnd, placement)
    else:
        _, da = critic_backward(critic, cc1, dq1, mm, need_params=False, fs=fs)
    if da_scale is not None:
        da = da * da_scale
    actor_grad = actor_backward(actor, ac, da, high, mm, fs=fs)
    return critic_grad, actor_grad, dict(critic_loss=critic_loss, actor_loss=actor_loss, y=y, q=q, q1=q1, a1=a1)


# ---- the acceptance rule --------------------------------------------------------------------------------------------------------
def tolerances(refs, emus):
    """refs, emus: one {name: array} per mask of ONE case and tile size -> {name: (scale, e_bf16, tol)}."""
    out = {}
    for name in NAMES:
        scale = max(max(np.max(np.abs(r[name])) for r in refs), 1e-300)
        e = max(np.max(np.abs(m[name] - r[name])) for r, m in zip(refs, emus)) / scale
        out[name] = (scale, e, max(FLOOR, FACTOR * e))
    return out


def violations(got, ref, tol, skip=()):
    """[(name, error / scale, tolerance)] of the tensors of one mask's result that miss the rule."""
    bad = []
    for name in NAMES:
        if name in skip:
            continue
        scale, _, limit = tol[name]
        err = np.max(np.abs(np.asarray(got[name], np.float64) - ref[name])) / scale
        if not err <= limit:
            bad.append((name, float(err), float(limit)))
    return bad


# ---- the cases: shapes from the path conditions of avd_learn_shared_bf16 (csrc/wide.hip, "fused_fwd" ... "act_in_dx") -----------
N_SETS, CHECK_SET = 2, 1  # the wide cases: two weight sets (the set stride is exercised); the oracles are computed for the second
# n_sets weight sets, the oracles computed for the sets of `check` (the fset cases below bring their own)
Case = namedtuple("Case", "name widths S rows seed path drop32 placement n_sets check", defaults=(N_SETS, (CHECK_SET,)))
CASES = [
    # fused forward, rank-one backward, critic(s, a) and critic(s, mu) in one pass (dual), fw::dx_gen_kernel<true> (H1 / 256 == 4)
    Case("h1024", (1024, 1024, 48), 4, 4096, 12, "fused fwd + rank-one bwd + dual + dx_gen<true>", (), "dual"),
    # rank-one backward with fw::dx_gen_kernel<false>, two state feature blocks (H1 = 512) ...
    Case("h512", (512, 512, 48), 4, 1024, 12, "fused fwd + rank-one bwd + dual + dx_gen<false>, 2 feature blocks", (), "dual"),
    # ... and one (H1 = 256)
    Case("h256x512", (256, 512, 48), 4, 1024, 13, "fused fwd + rank-one bwd + dual + dx_gen<false>, 1 feature block", (), "dual"),
    # H1 = 128 is no multiple of 256: no rank-one chain -- fused forward (stored activations), fw::fwd_delta_kernel, backward layer-wise
    Case("h128x512", (128, 512, 32), 4, 1024, 14, "fused fwd + fwd_delta, layer-wise bwd", (), "delta"),
    # H2 = 128 is no multiple of fw::FC and S = 3: nothing fused
    Case("h256x128_S3", (256, 128, 48), 3, 1024, 15, "everything layer-wise", (), "generic"),
    # 960 rows pad to 1024: the padding rows add nothing
    Case("h1024_pad", (1024, 1024, 48), 4, 960, 20, "as h1024, Ns = 960 < Np = 1024", (), "dual"),
]
CASE = {c.name: c for c in CASES}


def masks(case):
    """[(label, tile size t, lo, hi)]: rows [lo, hi) carry weight 1, all others 0; hi is clipped to the set's rows."""
    rows, out = case.rows, []
    n256 = (rows + 255) // 256
    for i in range(n256):
        out.append((f"t256[{i}]", 256, 256 * i, min(256 * i + 256, rows)))
    if case.name == "h1024":  # the eight sub-tiles of tile 5, one in each of three others -- the first and the last rows of the set
        subs = [(5, j) for j in range(8)] + [(0, 0), (10, 3), (15, 7)]
    elif case.name == "h1024_pad":  # the last 32-row sub-tile that still holds rows
        subs = [(3, 5)]
    else:  # one sub-tile per 256-row tile, the first and the last rows of the set among them
        subs = [(0, 0), (1, 3), (2, 5), (3, 7)]
    for i, j in subs:
        lo = 256 * i + 32 * j
        out.append((f"t32[{i}.{j}]", 32, lo, lo + 32))
    assert all(0 <= lo < hi <= rows for _, _, lo, hi in out)
    out.append(("whole", rows, 0, rows))
    return out


def case_conf_kw(case):
    H1, H2, Ha = case.widths
    return dict(actor_layer1_size=H1, actor_layer2_size=H2, critic_layer1_size=H1, critic_layer2_size=H2, critic_act_layer_size=Ha)


def case_batch(case):
    """(s, a, r, s2) of the case's n_sets sets, set-major, as tests/test_gpu_wide.py draws them."""
    rs = np.random.RandomState(case.seed + 1000)
    n, rows, S = case.n_sets, case.rows, case.S
    s = rs.normal(0, 1.5, size=(n, rows, S)).astype(np.float32)
    a = rs.uniform(-2.5, 2.5, size=(n, rows, 1)).astype(np.float32)
    r = -np.abs(rs.normal(0, 0.3, size=(n, rows))).astype(np.float32)
    s2 = rs.normal(0, 1.5, size=(n, rows, S)).astype(np.float32)
    return s, a, r, s2


def perturbed_slabs(n_sets, S, seed, **confkw):
    return _perturbed_slabs(n_sets, S, seed, tuple(sorted(confkw.items())))


@functools.lru_cache(maxsize=4)
def _perturbed_slabs(n_sets, S, seed, confkw):
    """The host half of tests/test_gpu_mlp.py _perturbed_group: (group on the CPU device, theta, stats, theta_t, stats_t) with the
    same draws (the GPU tests assert that the two agree bit for bit)."""
    from avddpg_amd import config, params, vec

    conf = config.Config(**dict(confkw))
    grp = vec.AgentGroup(n_sets, S, 1, conf, seed=seed, device="cpu")
    lay, dims = grp.lay, grp.dims
    rs = np.random.RandomState(seed + 100)
    th = np.zeros((n_sets, lay.theta_size), np.float32)
    st = np.zeros((n_sets, lay.stats_size), np.float32)
    tht, stt = th.copy(), st.copy()
    for dst_th, dst_st in ((th, st), (tht, stt)):
        for k in range(n_sets):
            a, s_ = params.init_weights(lay, rs, dims=dims)
            aw = params.unpack(lay, a, s_, "actor", dims=dims)
            cw = params.unpack(lay, a, s_, "critic", dims=dims)
            for net, var_idx in ((aw, (5, 11)), (cw, (7, 11, 17))):
                for w in net:
                    if w.ndim == 1:
                        w += rs.uniform(-0.3, 0.3, w.shape).astype(np.float32)
                for i in var_idx:
                    net[i][:] = np.abs(net[i]) + 0.5
            aw[12] *= 30
            cw[18] *= 300
            params.pack(lay, aw, dst_th[k], dst_st[k], "actor", dims=dims)
            params.pack(lay, cw, dst_th[k], dst_st[k], "critic", dims=dims)
    return grp, th, st, tht, stt


def case_nets(case, k=None):
    """(actor, critic, target actor, target critic) of set k (default: the case's first checked set) in float64, Keras weight order."""
    from avddpg_amd import params

    k = case.check[0] if k is None else k
    grp, th, st, tht, stt = perturbed_slabs(case.n_sets, case.S, case.seed, **case_conf_kw(case))
    c = lambda ws: [w.astype(np.float64) for w in ws]
    return (c(params.unpack(grp.lay, th[k], st[k], "actor", dims=grp.dims)), c(params.unpack(grp.lay, th[k], st[k], "critic", dims=grp.dims)),
            c(params.unpack(grp.lay, tht[k], stt[k], "actor", dims=grp.dims)), c(params.unpack(grp.lay, tht[k], stt[k], "critic", dims=grp.dims)))


def tile_learn(case, nets, batch, lo, hi, rnd, k=None, **kw):
    """{name: Nt / Ns x learn(rows [lo, hi) of set k)} of a set-major batch (k: default the case's first checked set; nets: that
    set's): what the set learners return for weight 1 on those rows, 0 elsewhere."""
    s, a, r, s2 = batch
    k = case.check[0] if k is None else k
    cg, ag, _ = learn((s[k, lo:hi], a[k, lo:hi], r[k, lo:hi, None], s2[k, lo:hi]), *nets, rnd=rnd, **kw)
    f = (hi - lo) / case.rows
    return {name: f * g for name, g in zip(NAMES, cg + ag)}


def _reference(case, batch, ms, k):
    """(masks, refs, emus, tol) of set k of a set-major batch: per mask the float64 reference and the bf16-operand oracle, and per tile
    size the pooled tolerance table {t: {tensor: (scale, e_bf16, tol)}}."""
    nets = case_nets(case, k)
    refs = [tile_learn(case, nets, batch, lo, hi, identity, k=k) for _, _, lo, hi in ms]
    emus = [tile_learn(case, nets, batch, lo, hi, round_bf16, k=k, placement=case.placement) for _, _, lo, hi in ms]
    tol = {}
    for t in sorted({m[1] for m in ms}, key=lambda t: (isinstance(t, str), t)):
        idx = [i for i, m in enumerate(ms) if m[1] == t]
        tol[t] = tolerances([refs[i] for i in idx], [emus[i] for i in idx])
    return ms, refs, emus, tol


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """-> (masks, refs, emus, tol) of the case's first checked set (the wide cases have one). Cached: every test of a case shares one
    computation."""
    case = CASE[name]
    return _reference(case, case_batch(case), masks(case), case.check[0])


def skipped(case, t):
    """Tensors not compared at tile size t (a tolerance at the cap says nothing): listed in CASES, never a head tensor."""
    return case.drop32 if t == 32 else ()


# ---- the agent-major set learner (csrc/fset.hip, csrc/fsplit.hip): one 64-row tile per agent, masks through agent_weight ---------
# make_plan gives a set J = min(CUs / n_sets, P) workgroups; workgroup j0 walks the agents (platoons) j0, j0 + J, .. of its set, so P is
# written through J = max(1, CUs // n_sets) and the caller passes the CU count (the GPU test: the device's; the CPU self-checks: 256).
FsetSpec = namedtuple("FsetSpec", "name S n_sets seed P platoons check placement why")
FSET_WIDTHS, FSET_B = (256, 128, 48), 64  # the reference widths, the only ones the engine serves
FSET = [
    FsetSpec("fset_64sets", 4, 64, 67, lambda J: 7 * J - 1, lambda J, P: range(P), (0, 37, 63), "fset",
             "every workgroup walks 7 tiles, the last 6: head_kernel's one-ahead prefetch, a wave pair's second tile in the 4-pair and "
             "the 6-pair modes, odd and even tile counts for dxa_kernel's parities, the widest set stride"),
    FsetSpec("fset_modelA_ragged", 3, 5, 62, lambda J: 70, lambda J, P: (0, J - 1, J, J + 18, P - 1), (0, 4), "generic",
             "ragged tile counts (at 256 CUs J = 51: 19 workgroups with 2 tiles, 32 with 1), Model A input width"),
    FsetSpec("fset_one_set", 4, 1, 69, lambda J: 300, lambda J, P: (0, J - 1, J, P - 1), (0,), "generic",
             "every CU on one set, 1-2 tiles each"),
]
FSET_SPEC = {c.name: c for c in FSET}


def fset_plan(name, cus):
    """(J, P, masked platoons) of an fset case on a device with `cus` compute units."""
    spec = FSET_SPEC[name]
    J = max(1, cus // spec.n_sets)
    P = spec.P(J)
    platoons = sorted({p for p in spec.platoons(J, P) if 0 <= p < P})
    return J, P, platoons


def fset_case(name, cus):
    """The Case of an fset spec: rows = P x 64 per set, its own set count and checked sets (serves case_nets, tile_learn)."""
    spec = FSET_SPEC[name]
    _, P, _ = fset_plan(name, cus)
    return Case(name, FSET_WIDTHS, spec.S, P * FSET_B, spec.seed, spec.why, (), spec.placement, spec.n_sets, spec.check)


def fset_batch(case):
    """(s, a, r, s2) AGENT-major [n_agents, 64, ..] (agent v = p * n_sets + m uses set m), drawn as tests/test_gpu_fset.py::_batch does."""
    rs = np.random.RandomState(case.seed + 1000)
    n, B, S = case.n_sets * case.rows // FSET_B, FSET_B, case.S
    s = rs.normal(0, 1.5, size=(n, B, S)).astype(np.float32)
    a = rs.uniform(-2.5, 2.5, size=(n, B, 1)).astype(np.float32)
    r = -np.abs(rs.normal(0, 0.3, size=(n, B))).astype(np.float32)
    s2 = rs.normal(0, 1.5, size=(n, B, S)).astype(np.float32)
    return s, a, r, s2


def set_major(batch, n_sets):
    """Agent-major [P * n_sets, 64, ..] -> set-major [n_sets, P * 64, ..]: platoon p's agent of set m is rows [64 p, 64 p + 64) of m."""
    def sm(x):
        P = x.shape[0] // n_sets
        return np.ascontiguousarray(x.reshape(P, n_sets, *x.shape[1:]).swapaxes(0, 1)).reshape(n_sets, P * x.shape[1], *x.shape[2:])
    return tuple(sm(x) for x in batch)


def fset_masks(name, cus):
    """[(label, tile size, lo, hi)] in set-major rows: weight 1 on every agent of platoon p0 (tile size 64; 1 / P x learn(that agent's
    rows) for every set at once), and the whole set (tile size "whole")."""
    _, P, platoons = fset_plan(name, cus)
    return [(f"p{p0}", FSET_B, FSET_B * p0, FSET_B * p0 + FSET_B) for p0 in platoons] + [("whole", "whole", 0, FSET_B * P)]


@functools.lru_cache(maxsize=None)
def fset_reference(name, cus):
    """-> (masks, {k: (refs, emus, tol)}) for every checked set k: per mask the float64 reference and the bf16-operand oracle, and per
    tile size (64, "whole") the tolerance table pooled over that set's masks. Cached per (case, CU count)."""
    case = fset_case(name, cus)
    batch, ms = set_major(fset_batch(case), case.n_sets), fset_masks(name, cus)
    return ms, {k: _reference(case, batch, ms, k)[1:] for k in case.check}


def fset_weights(case):
    """Per-agent factors w_p * P / sum(w) [P, n_sets], different per platoon AND per set: 0.2 ... 3.0 over the platoons with the
    +-20 % jitter of tests/test_gpu_fset.py's weighted test."""
    P, M = case.rows // FSET_B, case.n_sets
    rs = np.random.RandomState(case.seed + 2000)
    w = np.linspace(0.2, 3.0, P)[:, None].repeat(M, axis=1) * rs.uniform(0.8, 1.2, size=(P, M))
    return (w * (P / w.sum(axis=0))).astype(np.float32)


def weighted_learn(case, nets, batch, k, w, rnd, **kw):
    """{name: learn(all rows of set k)} with platoon p's rows weighted by w[p, k] on both loss seeds (dq_scale / da_scale): what the set
    learners return for agent_weight = w."""
    s, a, r, s2 = batch
    f = np.repeat(w[:, k].astype(np.float64), FSET_B)[:, None]
    cg, ag, _ = learn((s[k], a[k], r[k][:, None], s2[k]), *nets, rnd=rnd, dq_scale=f, da_scale=f, **kw)
    return dict(zip(NAMES, cg + ag))


@functools.lru_cache(maxsize=None)
def fset_weighted_reference(name, cus):
    """-> (w [P, n_sets], {k: (ref, emu, tol)}): the general-weights reference of every checked set, its own one-mask tolerance table."""
    case = fset_case(name, cus)
    batch, w = set_major(fset_batch(case), case.n_sets), fset_weights(case)
    out = {}
    for k in case.check:
        nets = case_nets(case, k)
        ref = weighted_learn(case, nets, batch, k, w, identity)
        emu = weighted_learn(case, nets, batch, k, w, round_bf16, placement=case.placement)
        out[k] = (ref, emu, tolerances([ref], [emu]))
    return w, out


# ---- acting with shared sets (csrc/wide.hip, avd_actor_forward_shared_bf16): the forward cases of tests/test_gpu_act_shared.py ----
# The layer-wise chain l1_fwd_kernel<S> -> launch_gemm<EpiFwd> -> tanh_rows_kernel on every row of every set, against
# actor_forward(.., fold=True): the float64 reference (mm = identity) and the bf16-operand oracle (both operands of every product
# rounded; the kernel rounds the STORED layer-2 activation and keeps cf = inv2 * W3 unrounded -- FACTOR is the margin for that).
#
# The rule (fwd_tolerances / fwd_violations), from the two oracles alone, errors relative to `high`:
#     e_max = max  over all rows and sets of |bf16oracle - ref| / high,     e_rms = the root mean square of the same
#     pass <=> max error <= max(FWD_TOL, FACTOR * e_max)   AND   rms error <= max(FWD_TOL, FACTOR * e_rms)
# FWD_TOL = 2e-5: the f32 accumulation-order floor of tests/test_gpu_mlp.py. The rms half is what bites on ONE wrong row tile (the
# maximum is set by the worst of several hundred rows). FWD_CAP: the budget of the test this one sits beside
# (tests/test_gpu_wide.py::test_shared_actor_forward_matches_per_agent_rows_kernel) -- no case may be looser.
FWD_TOL, FWD_CAP, HIGH = 2e-5, 2e-2, 2.5
FwdCase = namedtuple("FwdCase", "name widths S n_sets P seed std reaches")
# States: normal, float32, RandomState(seed + 1000) per case. NOT the std 1.5 of the other tests: at 1.5 the perturbed actors' outputs
# spread by 0.005 .. 0.02 high over a set's rows in every case (the biases dominate the first layer), five to twenty times short of the
# 0.1 high of fwd_inputs_bite -- a row holding its neighbour's output would pass. The cap held at 1.5 (tolerances 1.7e-3 .. 1.1e-2);
# the spread did not. The spread grows with the state scale, the bf16-oracle error more slowly, so each case takes the std and the
# seed (weights and states) below, found by a search over std in {12, 16, 24, 32} and seed + 10 j on the two oracles alone:
# every set's spread >= 0.1 high AND FACTOR * e_max <= FWD_CAP -- and, for one_row and past_tile, whose last row tile is ONE row, that
# row's output moves by more than the tolerance whichever 64-wide K block of layer 2 is left out (the planted defects of
# tests/test_bf16_oracle_cpu.py, which asserts all of this and prints the numbers).
FWD_CASES = [
    FwdCase("t256_ragged", (1024, 1024, 48), 4, 2, 700, 61, 24.0, "256-tile kernel, three row tiles, the last with 188 rows; Np = 768 > Ns"),
    FwdCase("t128_511", (1024, 1024, 48), 4, 2, 511, 72, 12.0, "one row short of the 256-tile condition: 128-tile kernel, K = 1024, ragged fourth tile"),
    FwdCase("one_row", (512, 320, 48), 4, 3, 1, 83, 24.0, "a set of one row; the output offset k * Ns with Ns = 1"),
    FwdCase("past_tile", (512, 320, 48), 4, 3, 129, 34, 32.0, "one row in the second 128-row tile; H2n = 512 > H2"),
    FwdCase("modelA", (256, 512, 48), 3, 2, 600, 55, 24.0, "l1_fwd_kernel<3>, 256-tile kernel at K = 256"),
    FwdCase("k64_t256", (64, 512, 16), 4, 2, 600, 56, 24.0, "256-tile kernel with two K steps under three stages"),
    FwdCase("k64_t128", (64, 64, 16), 4, 1, 130, 37, 24.0, "128-tile kernel with a single K step; one set"),
]
# VecTrainer's acting path for wide shared sets (_act_wide_shared: the set-major transposition around actor_shared), 8 platoons of 5
# vehicles at 1024/1024: n_sets = pl_size, P = num_platoons, Model B (S = 4) and Model A (S = 3). Std and seeds found as above on these
# 40 rows; the weights are loaded into the trainer's group, the states written into the environment ([P, M, 4]: trainer_env_states).
TRAINER_CASES = [
    FwdCase("trainer_modelB", (1024, 1024, 48), 4, 5, 8, 131, 24.0, "set-major view of env.x, actor_shared, copy back; 128-tile kernel, 8 rows"),
    FwdCase("trainer_modelA", (1024, 1024, 48), 3, 5, 8, 132, 24.0, "the same reading three of an agent's four floats"),
]
FWD_CASE = {c.name: c for c in FWD_CASES + TRAINER_CASES}
FwdRef = namedtuple("FwdRef", "x ref emu e_max e_rms tol_max tol_rms c0 active1 active2")


def fwd_conf_kw(case):
    H1, H2, Ha = case.widths
    return dict(actor_layer1_size=H1, actor_layer2_size=H2, critic_layer1_size=H1, critic_layer2_size=H2, critic_act_layer_size=Ha)


def fwd_tile(case):
    """Rows per tile of the layer-2 GEMM, as launch_gemm (csrc/wide.hip) chooses: 256 from 512 rows and 512 columns upward
    (K is a multiple of 32 at every width the library takes), else 128."""
    return 256 if case.P >= 512 and case.widths[1] >= 512 else 128


def fwd_last_tile(case):
    """[lo, hi): the rows of a set's last row tile."""
    t = fwd_tile(case)
    return (case.P - 1) // t * t, case.P


def fwd_states(case):
    """[n_sets, P, S] float32, set-major and tightly packed: what AgentGroup.actor_shared takes."""
    return np.random.RandomState(case.seed + 1000).normal(0, case.std, size=(case.n_sets, case.P, case.S)).astype(np.float32)


def fwd_actor(case, k):
    """Set k's actor in float64, Keras weight order (the slabs the GPU test loads: perturbed_slabs)."""
    from avddpg_amd import params

    grp, th, st, _, _ = perturbed_slabs(case.n_sets, case.S, case.seed, **fwd_conf_kw(case))
    return [w.astype(np.float64) for w in params.unpack(grp.lay, th[k], st[k], "actor", dims=grp.dims)]


def fwd_rows(w, x, drop_k=None):
    """tanh(.) * HIGH [rows] of the float64 reference in wide.hip's placement. drop_k: the layer-2 product WITHOUT the 64-wide K
    block drop_k (the folded bias keeps its sh . W2 term: what a GEMM that skips a K step computes) -- for the planted defects."""
    mm = np.matmul
    if drop_k is not None:
        keep = np.ones(w[0].shape[1], bool)
        keep[64 * drop_k:64 * drop_k + 64] = False
        mm = lambda p, v: p[:, keep] @ v[keep]
    out, cache = actor_forward(w, x, HIGH, mm, fold=True, mmx=np.matmul)
    return out[:, 0], cache


def fwd_c0(w):
    """b3 + sh2 . W3: the constant term of the output layer, what fill_rows_kernel pre-fills the head sums with."""
    _, sh2 = omlp._bn_coeffs(*w[8:12])
    return float(w[13][0] + sh2 @ w[12][:, 0])


def fwd_tolerances(ref, emu, high=HIGH):
    """ref, emu [sets, rows] -> (e_max, e_rms, tol_max, tol_rms)."""
    d = np.abs(np.asarray(emu, np.float64) - ref) / high
    e_max, e_rms = float(d.max()), float(np.sqrt(np.mean(d * d)))
    return e_max, e_rms, max(FWD_TOL, FACTOR * e_max), max(FWD_TOL, FACTOR * e_rms)


def fwd_errors(got, ref, high=HIGH):
    """(max, rms) of |got - ref| / high over all rows and sets."""
    d = np.abs(np.asarray(got, np.float64) - ref) / high
    return float(d.max()), float(np.sqrt(np.mean(d * d)))


def fwd_violations(got, ref, tol_max, tol_rms, high=HIGH):
    """[(which, error, tolerance)] of the halves of the rule that `got` [sets, rows] misses (a non-finite result misses both)."""
    e_max, e_rms = fwd_errors(got, ref, high)
    return [(n, e, tol) for n, e, tol in (("max", e_max, tol_max), ("rms", e_rms, tol_rms)) if not e <= tol]


@functools.lru_cache(maxsize=None)
def fwd_reference(name):
    """-> FwdRef of a forward case: the states, for every set the float64 reference and the bf16-operand oracle [sets, P], the rule's
    four numbers, every set's c0 and the fraction of active units per hidden layer. Cached and shared: treat it as read-only."""
    case = FWD_CASE[name]
    x = fwd_states(case)
    mm16 = lambda p, v: np.matmul(round_bf16(p), round_bf16(v))
    ref, emu, c0, a1, a2 = [], [], [], [], []
    for k in range(case.n_sets):
        w = fwd_actor(case, k)
        out, cache = fwd_rows(w, x[k])
        ref.append(out)
        emu.append(actor_forward(w, x[k], HIGH, mm16, fold=True)[0][:, 0])
        c0.append(fwd_c0(w))
        a1.append(float(np.mean(cache[1] > 0)))
        a2.append(float(np.mean(cache[3] > 0)))
    ref, emu = np.stack(ref), np.stack(emu)
    for a in (x, ref, emu):
        a.setflags(write=False)
    return FwdRef(x, ref, emu, *fwd_tolerances(ref, emu), tuple(c0), tuple(a1), tuple(a2))


def fwd_inputs_bite(ref, active1, active2, c0=None, high=HIGH):
    """The conditions under which a forward comparison can fail at all (from the float64 reference alone): 20 .. 80 % of the units of both
    hidden layers active; at least half the rows off tanh's plateau (|tanh| < 0.99); the outputs of a set's rows spread by at least
    0.1 high -- or, for a set of ONE row (c0 given), that row at least 0.1 high away from tanh(c0) * high, the value a head sum that
    received nothing would give."""
    ref = np.asarray(ref)
    assert all(0.2 <= a <= 0.8 for a in tuple(active1) + tuple(active2)), (active1, active2)
    assert np.mean(np.abs(ref) < 0.99 * high) >= 0.5, np.mean(np.abs(ref) < 0.99 * high)
    for k in range(ref.shape[0]):
        if ref.shape[1] > 1:
            assert ref[k].std() >= 0.1 * high, (k, ref[k].std())
        else:
            assert abs(ref[k, 0] - np.tanh(c0[k]) * high) >= 0.1 * high, (k, ref[k, 0], np.tanh(c0[k]) * high)


def fwd_other_S(case, lo, hi):
    """Rows [lo, hi) of every set as l1_fwd_kernel<the other S> would read them from the packed [sets, P, S] buffer: S = 4 where the case
    has 3 -- row n of set k starts at float 4 (k P + n) (the fourth float meets no weight row); S = 3 where it has 4 -- row n starts
    at float 3 (k P + n) and the fourth input is missing. Reads past the buffer's end give 0. -> [sets, hi - lo, S]."""
    S, So = case.S, 7 - case.S
    flat = np.concatenate([fwd_states(case).ravel(), np.zeros(So * case.n_sets * case.P + 4, np.float32)])
    out = np.zeros((case.n_sets, hi - lo, S), np.float32)
    for k in range(case.n_sets):
        for n in range(lo, hi):
            o = So * (k * case.P + n)
            out[k, n - lo, :3] = flat[o:o + 3]
    return out


def trainer_env_states(case, fill):
    """fwd_states(case) as the environment holds them: [P, M, 4] float32, agent (p, m) at [p, m, :S]; `fill` in the columns from S on
    (Model A: the fourth float, which the actor must not read)."""
    x = np.full((case.P, case.n_sets, 4), fill, np.float32)
    x[:, :, :case.S] = fwd_states(case).transpose(1, 0, 2)
    return x
