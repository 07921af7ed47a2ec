"""The internal attention interface (pfotgnrec_amd/csrc/attn.hpp) stated in numpy, in float64 or float32, with the
first-order magnitude ``mag`` of its own rounding noise beside every output, and the generators of the problems the kernel
tests run (tests/test_attn_ref_cpu.py, tests/test_gpu_attn_forms.py).  No import of the package.

A problem is a dict of numpy arrays named after the fields of ``PfoAttn`` (``keep``: bool [N, H, K], the dropout decisions).
Instance n, slot j is valid iff ``nbr_ids[n, j] != 0``;
  key_j   = [ nbr_tab[row_j, :D] | edge_feat[eidx_j] | cos(fmaf(dt_j, tw, tb)) ]          row_j = nbr_row[n, j] or base + n K + j
  s_jh    = scale * qk_h . key_j        a_jh = softmax over the valid j        a'_jh = a_jh * keep_jh / (1 - p)
  ctx_h   = [ sum_j a'_jh key_j | sum_j a'_jh | 1 on head 0 | 0 .. ]           per head at stride Cp
The roundings that belong to the function stay fp32 in both dtypes: dt, and the time argument as one fp32 FMA.  Everything
else follows the dtype.

``mag`` is built from the reference's own quantities only: sum |terms| for every sum, the score noise
scale * sum_c |qk_c| |key_jc| carried through the softmax to the weights and the context, and one absolute term (1) per
cosine or sine.  A result r of a fp32 evaluation is expected within a small multiple of 2^-24 * mag of the exact one."""
import numpy as np

from oracle import tgn_oracle as T

f32, f64 = np.float32, np.float64
ATTN_MARGIN = 8.0
EPS_FLOOR = 2.0 ** -23
DET_SCALE = 2.0 ** 40
RUN_CHUNK = 4            # attn_dev.hpp: members a wavefront of the run-merged kernel walks
FORMS = ["fwd_ring", "fwd_reg", "bwd_runs", "bwd_ring_none", "bwd_ring_direct", "bwd_none", "bwd_atomic", "bwd_det", "bwd_direct"]

PERTURBATIONS = ["drop_last_key", "no_dsb", "no_keep_scale_cA", "no_scale_key_side", "time_col_off", "shift_off", "no_relu",
                 "replica_dropped", "sum_before_dropout"]


def cp_of(D, Ef):
    return (2 * D + Ef + 2 + 3) // 4 * 4


def rows_of(p):
    N, K = p["N"], p["K"]
    if p["nbr_row"] is not None:
        return np.asarray(p["nbr_row"], np.int64).reshape(N, K)
    return p["nbr_row_base"] + np.arange(N * K, dtype=np.int64).reshape(N, K)


def qk_rows(p, dtype, shift_time=0):
    """[N, H, C] the folded query-key vectors (and the raw rows for the time_col_off perturbation)."""
    N, H, D, Ef, Cp = p["N"], p["H"], p["D"], p["Ef"], p["Cp"]
    q = np.asarray(p["QK"], f32).reshape(-1, p["qk_ld"])
    qr = np.arange(N) if p["qk_row"] is None else np.asarray(p["qk_row"], np.int64)
    q = q[qr][:, :H * Cp].reshape(N, H, Cp).astype(dtype)
    DE = D + Ef
    return np.concatenate([q[:, :, :DE], q[:, :, DE + shift_time:DE + shift_time + D]], axis=2)


def keys_of(p, dtype):
    """key [N, K, C], its noise magnitude kmag, sin of the time argument [N, K, D], valid [N, K]."""
    N, K, D, Ef = p["N"], p["K"], p["D"], p["Ef"]
    rows = rows_of(p)
    tab = np.asarray(p["nbr_tab"], f32).reshape(-1, p["nbr_ld"])
    kn = tab[rows][:, :, :D].astype(dtype)
    if Ef:
        ke = np.asarray(p["edge_feat"], f32).reshape(-1, Ef)[np.asarray(p["eidx"], np.int64).reshape(N, K)].astype(dtype)
    else:
        ke = np.zeros((N, K, 0), dtype)
    arg = T.fmaf(np.asarray(p["dt"], f32).reshape(N, K, 1), np.asarray(p["tw"], f32), np.asarray(p["tb"], f32))
    kt, ks = np.cos(arg.astype(dtype)), np.sin(arg.astype(dtype))
    key = np.concatenate([kn, ke, kt], axis=2)
    kmag = np.concatenate([np.abs(kn), np.abs(ke), np.abs(kt) + 1], axis=2).astype(f64)
    valid = np.asarray(p["nbr_ids"]).reshape(N, K) != 0
    return key, kmag, ks, valid


def _drop_last(valid):
    v = valid.copy()
    for n in range(v.shape[0]):
        j = np.flatnonzero(v[n])
        if len(j):
            v[n, j[-1]] = False
    return v


def keep_scale_of(p, dtype):
    return dtype(1) / (dtype(1) - dtype(f32(p["dropout_p"]))) if p["dropout_p"] > 0 else dtype(1)


def forward(p, dtype=f64, perturb=None):
    """-> dict(ctx [N, H*Cp], attw [N, H, K], inv [N] uint8) and mags (ctx, attw) as float64."""
    N, K, D, Ef, H, Cp = (p[k] for k in ("N", "K", "D", "Ef", "H", "Cp"))
    C = 2 * D + Ef
    key, kmag, _, valid = keys_of(p, dtype)
    if perturb == "drop_last_key":
        valid = _drop_last(valid)
    qk = qk_rows(p, dtype, 1 if perturb == "time_col_off" else 0)
    scale = dtype(f32(p["scale"]))
    ks = np.where(np.asarray(p["keep"], bool), keep_scale_of(p, dtype), dtype(0)).astype(dtype)       # [N, H, K]
    ctx = np.zeros((N, H, Cp), dtype)
    attw = np.zeros((N, H, K), dtype)
    m_ctx = np.zeros((N, H, Cp), f64)
    m_attw = np.zeros((N, H, K), f64)
    inv = np.ones(N, np.uint8)
    for n in range(N):
        v = np.flatnonzero(valid[n])
        if len(v) == 0:
            continue
        inv[n] = 0
        for h in range(H):
            s = (scale * (key[n, v] @ qk[n, h])).astype(dtype)
            ms = abs(float(scale)) * (kmag[n, v] @ np.abs(qk[n, h]).astype(f64)) + np.abs(s).astype(f64)
            e = np.exp(s - s.max())
            a = (e / e.sum()).astype(dtype)
            a64 = a.astype(f64)
            ma = a64 * (2 + ms + np.sum(a64 * ms))
            ap = a * ks[n, h, v]
            map_ = ma * ks[n, h, v].astype(f64) + np.abs(ap).astype(f64)
            attw[n, h, v] = a
            m_attw[n, h, v] = ma
            ctx[n, h, :C] = ap @ key[n, v]
            m_ctx[n, h, :C] = map_ @ np.abs(key[n, v]).astype(f64) + np.abs(ap).astype(f64) @ kmag[n, v]
            ctx[n, h, C] = np.sum(a) if perturb == "sum_before_dropout" else np.sum(ap)
            m_ctx[n, h, C] = np.sum(map_)
        ctx[n, 0, C + 1] = 1
    return dict(ctx=ctx.reshape(N, H * Cp), attw=attw, inv=inv), dict(ctx=m_ctx.reshape(N, H * Cp), attw=m_attw)


def backward(p, ctx, attw, dtype=f64, perturb=None, n_rep=1):
    """The backward given the forward's ctx [N, H*Cp] and attw [N, H, K] (as the kernels get them) and p["dctx"].
    -> out, mag with
      dQK [N, H*Cp]; d_slot [N*K, D] the key-side rows of every (instance, slot) with the nbr_relu mask applied (zero rows on
      padded slots: the plain-store form writes exactly these at nbr_row_base + n K + j); d_tab [nbr_rows, D] their sums per
      table row nbr_row names (no mask; requires nbr_row); dw, db [D] the time-encoder sums."""
    N, K, D, Ef, H, Cp = (p[k] for k in ("N", "K", "D", "Ef", "H", "Cp"))
    C, DE = 2 * D + Ef, D + Ef
    key, kmag, sn, valid = keys_of(p, dtype)
    if perturb == "drop_last_key":
        valid = _drop_last(valid)
    qk = qk_rows(p, dtype, 1 if perturb == "time_col_off" else 0)
    scale = dtype(f32(p["scale"]))
    kscale = keep_scale_of(p, dtype)
    keep = np.asarray(p["keep"], bool)
    ks = np.where(keep, kscale, dtype(0)).astype(dtype)
    dctx = np.asarray(p["dctx"], f32).reshape(N, H, Cp).astype(dtype)
    cx = np.asarray(ctx).reshape(N, H, Cp).astype(dtype)
    aw = np.asarray(attw).reshape(N, H, K).astype(dtype)
    dt = np.asarray(p["dt"], f32).reshape(N, K).astype(dtype)
    rows = rows_of(p)
    tab = np.asarray(p["nbr_tab"], f32).reshape(-1, p["nbr_ld"])
    dQK = np.zeros((N, H, Cp), dtype)
    m_dQK = np.zeros((N, H, Cp), f64)
    d_slot = np.zeros((N, K, D), dtype)
    m_slot = np.zeros((N, K, D), f64)
    have_tab = p["nbr_row"] is not None
    d_tab = np.zeros((p["nbr_rows"], D), dtype) if have_tab else None
    m_tab = np.zeros((p["nbr_rows"], D), f64) if have_tab else None
    dw, db = np.zeros(D, dtype), np.zeros(D, dtype)
    m_dw, m_db = np.zeros(D, f64), np.zeros(D, f64)
    A = lambda x: np.abs(x).astype(f64)
    for n in range(N):
        v = np.flatnonzero(valid[n])
        if len(v) == 0:
            continue
        dkey = np.zeros((len(v), C), dtype)
        m_dkey = np.zeros((len(v), C), f64)
        for h in range(H):
            g, x = dctx[n, h, :C], cx[n, h, :C]
            dsb = dctx[n, h, C] if perturb != "no_dsb" else dtype(0)
            t = np.sum(g * x) + dsb * cx[n, h, C]
            m_t = np.sum(A(g) * A(x)) + abs(float(dsb)) * abs(float(cx[n, h, C]))
            gk = key[n, v] @ g
            m_gk = kmag[n, v] @ A(g)
            k_ = ks[n, h, v]
            da = (gk + dsb) * k_
            m_da = (m_gk + abs(float(dsb))) * k_.astype(f64) + A(da)
            a = aw[n, h, v]
            dscore = a * (da - t)
            m_ds = A(a) * (m_da + m_t) + A(dscore)
            cA = a * (np.where(keep[n, h, v], dtype(1), dtype(0)) if perturb == "no_keep_scale_cA" else k_)
            cB = dscore * scale
            m_cB = m_ds * abs(float(scale)) + A(cB)
            dQK[n, h, :C] = cB @ key[n, v]
            m_dQK[n, h, :C] = m_cB @ A(key[n, v]) + A(cB) @ kmag[n, v]
            cBk = dscore if perturb == "no_scale_key_side" else cB
            dkey += cA[:, None] * g[None, :] + cBk[:, None] * qk[n, h][None, :]
            m_dkey += A(cA)[:, None] * A(g)[None, :] + (m_cB + A(cB))[:, None] * A(qk[n, h])[None, :]
        relu = p["nbr_relu"] and perturb != "no_relu"
        for i, j in enumerate(v):
            on = (tab[rows[n, j], :D] > 0) if relu else np.ones(D, bool)
            d_slot[n, j] = np.where(on, dkey[i, :D], dtype(0))
            m_slot[n, j] = np.where(on, m_dkey[i, :D], 0.0)
            if have_tab and not (perturb == "replica_dropped" and n_rep > 1 and (n // 4) % n_rep == 1):
                jj = j
                if perturb == "shift_off" and n == p.get("shift_victim", -1):
                    jj = v[(i + 1) % len(v)]
                d_tab[rows[n, jj]] += dkey[i, :D]
                m_tab[rows[n, jj]] += m_dkey[i, :D] + A(dkey[i, :D])
            gsin = -sn[n, j] * dkey[i, DE:]
            m_gs = A(sn[n, j]) * m_dkey[i, DE:] + A(dkey[i, DE:]) + A(gsin)
            dw += gsin * dt[n, j]
            db += gsin
            m_dw += m_gs * abs(float(dt[n, j]))
            m_db += m_gs
    out = dict(dQK=dQK.reshape(N, H * Cp), d_slot=d_slot.reshape(N * K, D), d_tab=d_tab, dw=dw, db=db)
    mag = dict(dQK=m_dQK.reshape(N, H * Cp), d_slot=m_slot.reshape(N * K, D), d_tab=m_tab, dw=m_dw, db=m_db)
    return out, mag


# ------------------------------------------------------------------------------------------------ the run-merged layout
def grouping(idx, nodes, cap_rows, key_src):
    """pfo_seg_build_launch in numpy: seg_ptr [cap_rows + 1], members (instances on a real node, by table row, inside a row by
    (key, instance)), seg_of per member position."""
    idx, nodes = np.asarray(idx, np.int64), np.asarray(nodes)
    real = np.flatnonzero(nodes != 0)
    key = np.asarray(key_src, np.int64)[real] if key_src is not None else real
    order = real[np.lexsort((real, key, idx[real]))]
    seg_ptr = np.zeros(cap_rows + 1, np.int64)
    np.add.at(seg_ptr, idx[real] + 1, 1)
    seg_ptr = np.cumsum(seg_ptr)
    seg_of = np.repeat(np.arange(cap_rows), np.diff(seg_ptr))
    return seg_ptr.astype(np.int32), order.astype(np.int32), seg_of.astype(np.int32)


def runs_rows(dQK, members, seg_of, live):
    """The run-merged layout of dQK: [M, W] rows by member position.  A live row p holds the sum of the per-instance rows of
    the members behind the previous live position of p's group (or from the group's start) up to and including p - the kernel
    stores a run at its LAST member.  Rows that are not live are returned as NaN (the kernel leaves them untouched)."""
    M = len(members)
    out = np.full((M, dQK.shape[1]), np.nan, dQK.dtype)
    acc, g = None, -1
    for q in range(M):
        if seg_of[q] != g:
            assert acc is None or not np.any(acc), "a group ends on members whose gradient no live row holds"
            acc, g = np.zeros(dQK.shape[1], dQK.dtype), seg_of[q]
        acc = acc + dQK[members[q]]
        if live[q]:
            out[q] = acc
            acc = np.zeros(dQK.shape[1], dQK.dtype)
    assert acc is None or not np.any(acc), "the list ends on members whose gradient no live row holds"
    return out


def group_sums(dQK, members, seg_ptr, n_rows):
    out = np.zeros((n_rows, dQK.shape[1]), dQK.dtype)
    for s in range(n_rows):
        for m in range(seg_ptr[s], seg_ptr[s + 1]):
            out[s] = out[s] + dQK[members[m]]
    return out


# ------------------------------------------------------------------------------------------------ bars
def bar(ref32, ref64, mag):
    """Per element: ATTN_MARGIN * max(e32, 2^-23) * mag with e32 = max |ref32 - ref64| / mag over the output (reference side only)."""
    r32, r64, mag = np.asarray(ref32, f64), np.asarray(ref64, f64), np.asarray(mag, f64)
    nz = mag > 0
    assert np.all(r32[~nz] == r64[~nz]), "the two references differ where no rounding can occur"
    e32 = float(np.max(np.abs(r32 - r64)[nz] / mag[nz])) if nz.any() else 0.0
    return ATTN_MARGIN * max(e32, EPS_FLOOR) * mag, e32


def worst_ratio(got, ref64, b):
    """max |got - ref64| / bar (0 where both vanish; inf where the bar is 0 and got differs)."""
    d = np.abs(np.asarray(got, f64) - np.asarray(ref64, f64))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0.0, d / b)
    return float(np.max(r)) if r.size else 0.0


# ------------------------------------------------------------------------------------------------ generators
COUNTS = [0, 1, 2, 3, 4, 5, None]        # None: K


def make_case(D, Ef, H, K, N=13, seed=0, p_drop=0.0, table=False, qk_share=False, relu=0, big=False, nbr_ld=None):
    """A per-instance problem.  Valid counts cycle through 0, 1, 2, 3, 4, 5, K (left-padded lists as most-recent sampling
    writes them on even instances, scattered slots on odd ones).  ``table``: nbr_row names rows of a small shared table
    (several slots per row, rows nobody names); else direct rows at nbr_row_base + n K + j.  Padded slots as sampler.hip
    writes them: id 0, edge 0, dt = the query time, row = the table row of node 0."""
    rng = np.random.default_rng([seed, D, Ef, H, K])
    Cp, C = cp_of(D, Ef), 2 * D + Ef
    n_nodes, n_edges = 23, 17
    ids = np.zeros((N, K), np.int32)
    for n in range(N):
        c = COUNTS[n % len(COUNTS)]
        c = K if c is None else min(c, K)
        slots = np.arange(K - c, K) if n % 2 == 0 else np.sort(rng.choice(K, c, replace=False))
        ids[n, slots] = rng.integers(1, n_nodes, c)
    valid = ids != 0
    eidx = np.where(valid, rng.integers(1, n_edges + 1, (N, K)), 0).astype(np.int32)
    tq = rng.integers(1, 50, N).astype(f64)
    small = rng.integers(0, 40, (N, K)).astype(f64)
    large = np.floor(10 ** rng.uniform(5, 7, (N, K)))
    dt = np.where(rng.random((N, K)) < 0.5, small, large)
    if big:
        dt[N - 1, K - 1] = 3.0e7                                   # beyond the fp32 range reduction's 2e7 at tw[0] = 1
        if not valid[N - 1, K - 1]:
            ids[N - 1, K - 1], eidx[N - 1, K - 1] = 3, 2
            valid = ids != 0
    dt = np.where(valid, dt, tq[:, None]).astype(f32)
    nbr_ld = D if nbr_ld is None else nbr_ld
    if table:
        row_of_node = rng.integers(0, 11, n_nodes).astype(np.int32)      # 11 of 16 rows, shared between nodes
        nbr_rows = 16
        nbr_row, base = row_of_node[ids].astype(np.int32), 0
    else:
        base = 3
        nbr_rows = base + N * K + 2
        nbr_row = None
    tab = rng.standard_normal((nbr_rows, nbr_ld)).astype(f32)
    if relu:
        tab = np.maximum(tab, 0)                                   # rows of a ReLU layer below: about half the columns are off
    cand = [n for n in range(N) if valid[n].sum() >= 2 and table and len(set(nbr_row[n][valid[n]])) >= 2]
    qk_ld = H * Cp + 8 if qk_share else H * Cp
    qk_row = rng.integers(0, 5, N).astype(np.int32) if qk_share else None
    QK = rng.standard_normal((7 if qk_share else N, qk_ld)).astype(f32)
    keep = rng.random((N, H, K)) >= p_drop if p_drop > 0 else np.ones((N, H, K), bool)
    if p_drop > 0:
        _mix_keep(keep, valid)
    return dict(N=N, K=K, D=D, Ef=Ef, H=H, Cp=Cp, QK=QK, qk_row=qk_row, qk_ld=qk_ld, nbr_tab=tab, nbr_ld=nbr_ld, nbr_row=nbr_row,
                nbr_row_base=base, nbr_rows=nbr_rows, edge_rows=n_edges + 1, nbr_relu=relu, nbr_ids=ids,
                edge_feat=rng.standard_normal((n_edges + 1, Ef)).astype(f32), eidx=eidx, dt=dt,
                tw=(10.0 ** -np.linspace(0, 9, D)).astype(f32), tb=rng.standard_normal(D).astype(f32),
                scale=float(f32((C / H) ** -0.5)), dropout_p=float(p_drop), keep=keep,
                dctx=rng.standard_normal((N, H * Cp)).astype(f32), shift_victim=cand[0] if cand else -1)


def _mix_keep(keep, valid):
    """Dropout cases: the instance with the most valid keys has, on every head, its first key dropped and its second kept (so
    that no draw leaves a case without a dropped weight beside a kept one)."""
    n = int(np.argmax(valid.sum(axis=1)))
    j = np.flatnonzero(valid[n])
    if len(j) >= 2:
        keep[n, :, j[0]], keep[n, :, j[1]] = False, True


def mixed_keep(p):
    """Some (instance, head) holds a dropped and a kept weight among its valid keys."""
    v = (p["nbr_ids"] != 0)[:, None, :]
    return bool(np.any((v & p["keep"]).any(axis=2) & (v & ~p["keep"]).any(axis=2)))


# (node label, history counts of its instances); "jump" is replaced by a step larger than 64 - K
GROUPS_FULL = [("one", [3]), ("same9", [7] * 9), ("by1", [5, 6, 7, 8, 9]), ("by2", [4, 6, 8, 10]), ("jump", [6, "jump", "jump+1"]),
               ("grow", ["K-2", "K-1", "K", "K+1", "K+2"]), ("none", [0, 0, 2, 3])]
GROUPS_ONE = [("one", [3])]
GROUPS_SEVEN = [("by1", [1, 2, 3]), ("same", [4, 4]), ("none", [0, 1])]


def make_runs_case(D, Ef, H, K, groups=GROUPS_FULL, seed=0, p_drop=0.0, big=False, shifts=True, n_pad=2):
    """A layer-1 problem over a touched-node table built from per-node histories: slot j of an instance with count cnt holds
    history entry cnt - K + j of its node (left-padded when cnt < K), so the lists of one node are shifts of each other by the
    difference of counts.  ``shifts`` False: the lists are shuffled per instance (uniform sampling: no members are given).
    Table rows: row 0 = node 0, the groups' rows behind it with empty rows between; n_pad padding instances sit on node 0."""
    rng = np.random.default_rng([seed, D, Ef, H, K, len(groups)])
    Cp, C = cp_of(D, Ef), 2 * D + Ef
    n_edges = 29

    def cnt_of(c):
        if isinstance(c, str):
            c = c.replace("jump", str(6 + 64 - K + 1))
            return int(eval(c, {"K": K}))                       # "K-2" .. "K+2", "71+1"
        return c
    inst = []                                                    # (node id, table row, cnt)
    row, hist = 1, {}
    for gi, (_, cnts) in enumerate(groups):
        cnts = [max(0, cnt_of(c)) for c in cnts]
        node = 2 + gi
        L = max(cnts) + 1
        t = np.cumsum(rng.integers(1, 9, L)).astype(f64) * (1.0 if gi % 2 == 0 else 1.0e4)
        hist[node] = dict(ids=rng.integers(1, 2 + len(groups), L), e=rng.integers(1, n_edges + 1, L), t=t)
        inst += [(node, row, c) for c in cnts]
        row += 2 if gi % 2 == 0 else 1                           # an empty table row behind every other group
    n_rows = row
    inst += [(0, 0, 0)] * n_pad
    order = rng.permutation(len(inst))
    inst = [inst[i] for i in order]
    N = len(inst)
    row_of_node = np.zeros(2 + len(groups), np.int32)
    for node, r, _ in inst:
        row_of_node[node] = r
    ids, eidx = np.zeros((N, K), np.int32), np.zeros((N, K), np.int32)
    dt = np.zeros((N, K), f64)
    for n, (node, r, cnt) in enumerate(inst):
        tq = 5.0
        if node:
            h = hist[node]
            tq = (h["t"][cnt - 1] if cnt else 0.0) + 2.0
            for j in range(K):
                e = cnt - K + j
                if e >= 0:
                    ids[n, j], eidx[n, j], dt[n, j] = h["ids"][e], h["e"][e], tq - h["t"][e]
        dt[n, ids[n] == 0] = tq
        if not shifts:
            perm = rng.permutation(K)
            ids[n], eidx[n], dt[n] = ids[n, perm], eidx[n, perm], dt[n, perm]
    if big:
        n_big = next(n for n in range(N) if (ids[n] != 0).sum() >= 2)
        dt[n_big, np.flatnonzero(ids[n_big])[0]] = 3.0e7
    qk_ld = H * Cp + 4
    keep = rng.random((N, H, K)) >= p_drop if p_drop > 0 else np.ones((N, H, K), bool)
    if p_drop > 0:
        _mix_keep(keep, ids != 0)
    p = dict(N=N, K=K, D=D, Ef=Ef, H=H, Cp=Cp, QK=rng.standard_normal((n_rows, qk_ld)).astype(f32),
             qk_row=np.array([r for _, r, _ in inst], np.int32), qk_ld=qk_ld,
             nbr_tab=rng.standard_normal((n_rows, D)).astype(f32), nbr_ld=D, nbr_row=row_of_node[ids].astype(np.int32),
             nbr_row_base=0, nbr_rows=n_rows, edge_rows=n_edges + 1, nbr_relu=0, nbr_ids=ids,
             edge_feat=rng.standard_normal((n_edges + 1, Ef)).astype(f32), eidx=eidx, dt=dt.astype(f32),
             tw=(10.0 ** -np.linspace(0, 9, D)).astype(f32), tb=rng.standard_normal(D).astype(f32),
             scale=float(f32((C / H) ** -0.5)), dropout_p=float(p_drop), keep=keep,
             dctx=rng.standard_normal((N, H * Cp)).astype(f32),
             nodes=np.array([node for node, _, _ in inst], np.int32), run_cnt=np.array([c for _, _, c in inst], np.int32),
             cap_rows=n_rows + 5, n_rows=n_rows, shifts=shifts)
    cand = [n for n in range(N) if len(set(p["nbr_row"][n][ids[n] != 0])) >= 2]
    p["shift_victim"] = cand[0] if cand else -1
    return p


def check_invariants(p):
    """The generator's own output: every index in range over its whole array, padded slots as the sampler writes them, and
    (with histories) neighbour lists that are shifts by the difference of counts and members ordered by (key, instance)."""
    N, K = p["N"], p["K"]
    ids, eidx = p["nbr_ids"], p["eidx"]
    assert ids.shape == (N, K) and eidx.min() >= 0 and eidx.max() < p["edge_rows"]
    rows = rows_of(p)
    assert rows.min() >= 0 and rows.max() < p["nbr_rows"] and p["nbr_tab"].shape[0] == p["nbr_rows"]
    assert np.all(eidx[ids == 0] == 0) and np.all(np.isfinite(p["dt"]))
    if p["qk_row"] is not None:
        assert p["qk_row"].min() >= 0 and p["qk_row"].max() < p["QK"].shape[0]
    if "run_cnt" not in p:
        return
    seg_ptr, members, seg_of = grouping(p["qk_row"], p["nodes"], p["cap_rows"], p["run_cnt"])
    assert seg_ptr[p["n_rows"]] == len(members) == int((p["nodes"] != 0).sum())
    cnt = p["run_cnt"]
    for s in range(p["cap_rows"]):
        mem = members[seg_ptr[s]:seg_ptr[s + 1]]
        assert all(p["qk_row"][m] == s and p["nodes"][m] != 0 for m in mem)
        keys = [(cnt[m], m) for m in mem]
        assert keys == sorted(keys)
        for a, b in zip(mem[:-1], mem[1:]):
            d = int(cnt[b] - cnt[a])
            assert d >= 0
            if d < K and p["shifts"]:
                for arr in (ids, eidx, rows):
                    assert np.array_equal(arr[a, d:], arr[b, :K - d]), "lists of one node must be shifts by the difference of counts"


# ------------------------------------------------------------------------------------------------ the cases of the kernel tests
# (D, Ef, H), each on a rule of the launchers (attn.hip attn_fwd_ring_ok / attn_bwd_ring_ok / pfo_attn_bwd_runs_possible)
RING_SHAPES = [(4, 0, 1), (32, 4, 2), (60, 4, 4), (64, 0, 2), (124, 4, 4), (172, 12, 4), (192, 0, 4), (252, 4, 2), (256, 0, 1)]
REG_SHAPES = [(64, 4, 2), (128, 4, 4), (192, 4, 2), (172, 64, 2), (256, 4, 2), (256, 0, 4)]
ODD_SHAPE = (30, 6, 2)                   # check_common admits it, the config check never produces it
K_LIST = [1, 2, 3, 5, 20, 33, 63, 64]
K_DEFAULT = 7                            # valid counts 0..5 and K all differ
# per shape: (name, make_case keywords)
VARIANTS = [("p0_direct_relu", dict(relu=1)),
            ("p01_table", dict(p_drop=0.1, table=True)),
            ("p05_share", dict(p_drop=0.5, qk_share=True)),
            ("p0_table_share_big", dict(table=True, qk_share=True, big=True))]
RUNS_SHAPES = [(4, 4, 4, 5), (32, 4, 2, 64), (32, 4, 2, 63), (64, 4, 1, 33), (124, 4, 4, 5), (172, 4, 2, 20), (172, 64, 2, 5),
               (192, 4, 2, 5), (256, 0, 2, 5)]


def per_instance_cases():
    """[(id, shape form 'ring' | 'reg', make_case arguments)]"""
    out = []
    for form, shapes in (("ring", RING_SHAPES), ("reg", REG_SHAPES + [ODD_SHAPE])):
        for (D, Ef, H) in shapes:
            for name, kw in VARIANTS:
                out.append(("%s-%d-%d-%d-%s" % (form, D, Ef, H, name), form, dict(D=D, Ef=Ef, H=H, K=K_DEFAULT, **kw)))
    for form, (D, Ef, H) in (("ring", (32, 4, 2)), ("reg", (64, 4, 2))):
        for K in K_LIST:
            out.append(("%s-%d-%d-%d-K%d" % (form, D, Ef, H, K), form, dict(D=D, Ef=Ef, H=H, K=K, p_drop=0.1, table=(K % 2 == 1))))
    return out


def runs_cases():
    """[(id, make_runs_case arguments)]: every shape with the full set of group structures, plain and with dropout; M = 1 and
    M = 7 (not a multiple of 4) at one shape; one argument beyond 2e7."""
    out = []
    for i, (D, Ef, H, K) in enumerate(RUNS_SHAPES):
        out.append(("runs-%d-%d-%d-K%d" % (D, Ef, H, K), dict(D=D, Ef=Ef, H=H, K=K, p_drop=0.1 if i % 2 else 0.0, big=(i == 5))))
    out.append(("runs-32-4-2-K5-M1", dict(D=32, Ef=4, H=2, K=5, groups=GROUPS_ONE, n_pad=1)))
    out.append(("runs-32-4-2-K5-M7", dict(D=32, Ef=4, H=2, K=5, groups=GROUPS_SEVEN, p_drop=0.1)))
    return out


def applies(perturb, p, n_rep=1):
    """Whether a perturbation changes anything at problem p (e.g. the keep scale only exists with dropout)."""
    valid = p["nbr_ids"] != 0
    if perturb == "no_dsb":         # d(sum a') cancels in the softmax backward unless the keys of one softmax have different multipliers
        return p["dropout_p"] > 0 and mixed_keep(p)
    if perturb in ("no_keep_scale_cA", "sum_before_dropout"):
        return p["dropout_p"] > 0
    if perturb in ("no_scale_key_side", "time_col_off"):      # (a softmax over one key: no score gradient, and qk decides nothing)
        return (p["scale"] != 1.0 or perturb == "time_col_off") and bool((valid.sum(axis=1) >= 2).any())
    if perturb == "shift_off":
        return p["nbr_row"] is not None and p.get("shift_victim", -1) >= 0
    if perturb == "no_relu":
        return p["nbr_row"] is None and p["nbr_relu"] != 0
    if perturb == "replica_dropped":
        return p["nbr_row"] is not None and n_rep > 1 and bool(valid[[n for n in range(p["N"]) if (n // 4) % n_rep == 1]].any())
    return bool(valid.any())


def reference(p, perturb=None, dtype=f64, n_rep=1):
    """Forward, then the backward fed the forward's fp32-rounded ctx and attw: all outputs and mags in two dicts."""
    fo, fm = forward(p, dtype, perturb)
    bo, bm = backward(p, fo["ctx"].astype(f32), fo["attw"].astype(f32), dtype, perturb, n_rep)
    fo.update(bo)
    fm.update(bm)
    return fo, fm


OUTPUTS = ["ctx", "attw", "dQK", "d_slot", "d_tab", "dw", "db"]
