"""Plain numpy float64 models of the internal contraction interface (pfotgnrec_amd/csrc/gemm.hpp), written from the header's
comments alone, and the operand generator the contraction tests share.

A problem is a dict whose keys are the fields of the C++ struct; where the struct holds a pointer the dict holds a FLAT numpy
array (the buffer the pointer would point into) and every index is formed exactly as the header states it: element strides,
leading dimensions, gathers.  Missing keys take the struct's defaults.  Every function returns new arrays and leaves its
inputs alone.  tests/test_gemm_ref_cpu.py holds these models against independent formulations."""
import numpy as np

f64 = np.float64


def wide(rs, *shape):
    """Operands with a wide dynamic range (exponents differ along k), so that dropped low pieces of a split would show:
    randn * exp(2 * randn), the generator of the split-contraction tests."""
    return (rs.randn(*shape) * np.exp(2 * rs.randn(*shape))).astype(np.float32)


def tn_scale_floor(X, col_block, k_tile=32, floor=2.0 ** -14):
    """max(|x_kc|, floor * S(k, block(c))) with S = the largest magnitude of the operand's column block over every row up to
    the end of k's tile: an upper bound of the ONE running scale the weight-gradient tile keeps per operand, workgroup tile
    (128 columns of A, 176 of B: gemm_dev.hpp BM / BN) and K-slab (a slab starts later than row 0, so its running maximum is at
    most this one).  ``floor``: 2^-16 of the scaled top, which sits up to HX_GROW = 2 binades above the maximum."""
    K, C = X.shape
    out = np.abs(X).astype(np.float64)
    for c0 in range(0, C, col_block):
        blk = out[:, c0:c0 + col_block]
        per_tile = blk.reshape(-1, k_tile, blk.shape[1]).max((1, 2)) if K % k_tile == 0 else None
        assert per_tile is not None, "K must be a multiple of the k-tile in this test"
        run = np.maximum.accumulate(per_tile)                         # [tiles]
        out[:, c0:c0 + col_block] = np.maximum(blk, floor * np.repeat(run, k_tile)[:, None])
    return out


GEMM_DEFAULTS = dict(A=(None, None), lda=(0, 0), a_idx=(None, None), B=(None, None), ldb=(0, 0), b_idx=None, K=(0, 0), C=None, ldc=0,
                     bias=None, row_scale=None, rs_ld=1, row_zero=None, relu_src=None, relu_ld=0, add_src=None, add_ld=0,
                     add_idx=None, M=0, N=0, m_dev=None, relu=0, accumulate=0, a_kmajor=0, b_kmajor=0, batch=1, a_bs=(0, 0),
                     b_bs=(0, 0), c_bs=0, bias_bs=0, rs_bs=0)


def gemm_desc(**kw):
    d = dict(GEMM_DEFAULTS)
    for k in kw:
        assert k in d or k in ("bx_force", "b_img", "b_img2", "slabs"), k
    d.update(kw)
    return d


def _flat64(x):
    return None if x is None else np.asarray(x).reshape(-1).astype(f64)


def gemm_ref(desc, rows=None, want_written=True):
    """C[M,N] = epilogue(sum over up to two K-concatenated sources A_s op(B_s)), epilogue order
    (+= C) -> + bias[n] * row_scale[m] -> + add_src[add_idx[m]][n] -> row_zero -> relu -> * (relu_src > 0).

    Returns (out, mag, written): the flat C buffer after the call in float64 (elements the call does not write keep their
    value), the per-element magnitude sum |a||b| + |every addend that entered the element| (0 where not written) and the
    boolean mask of the written elements.  m_dev: rows at or beyond it are not written (row-major A); for a k-major A it bounds
    the extent K[0] instead.

    ``rows`` (large problems, batch 1): evaluate these output rows only and return (out [n, N], mag [n, N], written, rows) -
    the results of the evaluated rows (sorted, unique, below m_dev) in compact form; ``written`` still marks every element
    the call writes (None with ``want_written=False``: a caller that walks a large problem chunk by chunk asks for it once)."""
    d = gemm_desc(**desc)
    M, N = int(d["M"]), int(d["N"])
    C0 = np.asarray(d["C"]).reshape(-1)
    written = np.zeros(C0.shape, bool)
    K = [int(d["K"][0]), int(d["K"][1])]
    Mlim = M
    if d["m_dev"] is not None:
        md = int(np.asarray(d["m_dev"]).reshape(-1)[0])
        if d["a_kmajor"]:
            K[0] = min(K[0], md)
        else:
            Mlim = min(M, md)
    subset = rows is not None
    if subset:
        assert int(d["batch"]) == 1
        rows = np.unique(np.asarray(rows, np.int64))
        rows = rows[rows < Mlim]
        for m0 in range(0, Mlim if want_written else 0, 4096):                   # every written element, a block of rows at a time
            r_ = np.arange(m0, min(Mlim, m0 + 4096))
            written[(r_[:, None] * d["ldc"] + np.arange(N)[None, :]).astype(np.int64)] = True
    else:
        rows = np.arange(Mlim)
        out, mag = C0.astype(f64), np.zeros(C0.shape, f64)
    Mlim = len(rows)
    cols = np.arange(N)
    bias, rs, add, rsrc = _flat64(d["bias"]), _flat64(d["row_scale"]), _flat64(d["add_src"]), _flat64(d["relu_src"])
    for z in range(int(d["batch"])):
        acc = np.zeros((Mlim, N), f64)
        m_ = np.zeros((Mlim, N), f64)
        for s in range(2):
            if s == 1 and K[1] == 0:
                continue
            A, B = _flat64(d["A"][s]), _flat64(d["B"][s])
            ks = np.arange(K[s])
            if d["a_kmajor"]:
                ai = z * d["a_bs"][s] + ks[None, :] * d["lda"][s] + rows[:, None]
            else:
                ar = rows if d["a_idx"][s] is None else np.asarray(d["a_idx"][s]).reshape(-1)[rows].astype(np.int64)
                ai = z * d["a_bs"][s] + ar[:, None] * d["lda"][s] + ks[None, :]
            if d["b_kmajor"]:
                kr = ks if (d["b_idx"] is None or s == 1) else np.asarray(d["b_idx"]).reshape(-1)[ks].astype(np.int64)
                bi = z * d["b_bs"][s] + kr[:, None] * d["ldb"][s] + cols[None, :]
            else:
                bi = z * d["b_bs"][s] + cols[None, :] * d["ldb"][s] + ks[:, None]
            a, b = A[ai.astype(np.int64)], B[bi.astype(np.int64)]               # [Mlim, K], [K, N]
            acc += a @ b
            m_ += np.abs(a) @ np.abs(b)
        ci = (z * d["c_bs"] + rows[:, None] * d["ldc"] + cols[None, :]).astype(np.int64)
        if d["accumulate"]:
            acc += C0[ci].astype(f64)
            m_ += np.abs(C0[ci].astype(f64))
        if bias is not None:
            sc = np.ones(Mlim) if rs is None else rs[(z * d["rs_bs"] + rows * d["rs_ld"]).astype(np.int64)]
            t = bias[(z * d["bias_bs"] + cols).astype(np.int64)][None, :] * sc[:, None]
            acc += t
            m_ += np.abs(t)
        if add is not None:
            ar = rows if d["add_idx"] is None else np.asarray(d["add_idx"]).reshape(-1)[rows].astype(np.int64)
            t = add[(ar[:, None] * d["add_ld"] + cols[None, :]).astype(np.int64)]
            acc += t
            m_ += np.abs(t)
        if d["row_zero"] is not None:
            acc[np.asarray(d["row_zero"]).reshape(-1)[rows] != 0] = 0.0
        if d["relu"]:
            acc = np.maximum(acc, 0.0)
        if rsrc is not None:
            keep = rsrc[(rows[:, None] * d["relu_ld"] + cols[None, :]).astype(np.int64)] > 0
            acc = np.where(keep, acc, 0.0)
        if subset:
            return acc, m_, (written if want_written else None), rows
        written[ci] = True
        out[ci] = acc
        mag[ci] = m_
    return out, mag, written


TN_DEFAULTS = dict(A=None, lda=0, B=None, ldb=0, b_idx=None, M=0, N=0, C=None, ldc=0, c_accumulate=1, bias_out=None,
                   bias_accumulate=1)


def tn_group_ref(probs, K, k_dev=None, a_block=None, b_block=176):
    """dW[M,N] (+)= A[:k, :M]^T B[b_idx[:k] or :k, :N] over the first k = min(K, k_dev) rows, with the optional bias gradient
    bias_out[M] (+)= sum_k A[k][m], for every problem of a grouped launch.

    Returns one dict per problem: C / C_mag / C_written (flat, as in gemm_ref) and bias / bias_mag.  ``a_block``: None gives
    the plain magnitude sum |a||b|; a column count gives the floored magnitude of a kernel that keeps one scale per operand
    tile (tn_scale_floor over blocks of a_block columns of A and b_block columns of [B | 1]: the bias gradient is carried
    as one more column of B, a column of ones)."""
    ke = K if k_dev is None else min(K, int(np.asarray(k_dev).reshape(-1)[0]))
    res = []
    for p in probs:
        q = dict(TN_DEFAULTS)
        q.update(p)
        M, N = int(q["M"]), int(q["N"])
        ks = np.arange(ke)
        A = _flat64(q["A"])[(ks[:, None] * q["lda"] + np.arange(M)[None, :]).astype(np.int64)]          # [k, M]
        kr = ks if q["b_idx"] is None else np.asarray(q["b_idx"]).reshape(-1)[ks].astype(np.int64)
        B = _flat64(q["B"])[(kr[:, None] * q["ldb"] + np.arange(N)[None, :]).astype(np.int64)]          # [k, N]
        has_bias = q["bias_out"] is not None
        Bx = np.concatenate([B, np.ones((ke, 1))], 1) if has_bias else B
        full = A.T @ Bx
        if a_block is None:
            fmag = np.abs(A).T @ np.abs(Bx)
        else:
            pad = (-ke) % 32                                                     # zero rows change no maximum
            Ap, Bp = np.pad(A, ((0, pad), (0, 0))), np.pad(Bx, ((0, pad), (0, 0)))
            fmag = (tn_scale_floor(Ap, a_block)[:ke].T @ tn_scale_floor(Bp, b_block)[:ke]) if ke > 0 else np.zeros((M, Bx.shape[1]))
        C0 = _flat64(q["C"])
        out, mag, written = C0.copy(), np.zeros_like(C0), np.zeros(C0.shape, bool)
        ci = (np.arange(M)[:, None] * q["ldc"] + np.arange(N)[None, :]).astype(np.int64)
        out[ci] = full[:, :N] + (C0[ci] if q["c_accumulate"] else 0.0)
        mag[ci] = fmag[:, :N] + (np.abs(C0[ci]) if q["c_accumulate"] else 0.0)
        written[ci] = True
        r = dict(C=out, C_mag=mag, C_written=written, bias=None, bias_mag=None)
        if has_bias:
            b0 = _flat64(q["bias_out"])
            r["bias"], r["bias_mag"] = b0.copy(), np.zeros_like(b0)
            r["bias"][:M] = full[:, N] + (b0[:M] if q["bias_accumulate"] else 0.0)
            r["bias_mag"][:M] = fmag[:, N] + (np.abs(b0[:M]) if q["bias_accumulate"] else 0.0)
        res.append(r)
    return res


# ------------------------------------------------------------------------------------------------ the launchers' dispatch
# The rule by which pfo_gemm_launch and pfo_gemm_tn_group_launch pick a kernel, a grid and a K split, stated here a second time
# and independently of gemm.hip: tests/test_gemm_plan_cpu.py holds it to the library's own answer (pfo_debug_gemm_plan /
# pfo_debug_gemm_tn_group_plan, the function the launchers switch on) over a sweep that sits on every threshold below, so a
# change of the rule on one side alone fails there - on the CPU, without a launch.  The descriptors are the ctypes structs of
# pfotgnrec_amd/_lib.py (or anything with their fields); a pointer is an integer or None and is never followed.
BM, BN, BK = 128, 176, 32                        # the workgroup tile: rows, columns, k-rows
F32_BIG_MIN_TILES = 400                          # fp32 kernel, row-major A: 128-row tiles from this many 128 x 176 tiles on, else 32-row
BX_MIN_TILES, BX_AREG8_MIN = 400, 512            # image launches: the 128-row kernels from / their eight-wavefront form from
SK_ROWS, SK_WIDE_MIN_WGS = 32, 512               # the 32-row image kernel: 176-column workgroups from this many of them on, else 64
AS_KMAX, AS_NMIN, AS_NMAX, AS_MMIN = 6 * BK, 352, 1024, 128 * 256      # the A-stationary form's shape window
SPLIT_WGS, SPLIT_MIN_KTILES = 512, 4             # a k-major launch splits K towards this many workgroups, >= 4 k-tiles a slab
TN8_MIN_ROWS, TN_SLOTS, TN8_SLOTS = 500, 512, 256                      # grouped launches: 256-row tiles when every M >= ...; workgroup slots


class PlanRefused(Exception):
    """The launcher refuses the descriptor; str() is a word of its message."""


def cdiv(a, b):
    return -(-a // b)


def _aligned(p):
    return (p or 0) % 16 == 0


def split_k(K, want):
    """(nsplit, chunk): at most ``want`` slabs of whole k-tiles, sized evenly, none planned below SPLIT_MIN_KTILES k-tiles."""
    nsplit = max(1, min(want, cdiv(K, SPLIT_MIN_KTILES * BK)))
    chunk = cdiv(cdiv(K, nsplit), BK) * BK
    return cdiv(K, chunk), chunk


def gemm_plan_ref(g):
    """What pfo_gemm_launch does with descriptor ``g``: dict(form, vec, grid_x, grid_y, grid_z, block, nsplit, chunk, kind), form
    a name of _lib.GEMM_FORMS and kind one of _lib.PROF_KINDS - or PlanRefused."""
    K = (g.K[0], g.K[1])
    if not (g.M > 0 and g.N > 0 and K[0] > 0 and g.batch >= 1):
        raise PlanRefused("bad sizes")
    if not (g.A[0] and g.B[0] and g.C):
        raise PlanRefused("null operand")
    srcs = (0, 1) if K[1] != 0 else (0,)
    if not all(g.A[s] and g.B[s] for s in srcs):
        raise PlanRefused("source 2")
    a_vec = all(_aligned(g.A[s]) and g.lda[s] % 4 == 0 and g.a_bs[s] % 4 == 0 and (g.M if g.a_kmajor else K[s]) % 4 == 0 for s in srcs)
    b_vec = all(_aligned(g.B[s]) and g.ldb[s] % 4 == 0 and g.b_bs[s] % 4 == 0 and (g.N if g.b_kmajor else K[s]) % 4 == 0 for s in srcs)
    image = bool(not g.a_kmajor and g.b_img and (K[1] == 0 or g.b_img2) and a_vec and g.batch == 1)
    if g.b_idx and not (g.b_kmajor and not image):
        raise PlanRefused("b_idx")
    if g.a_kmajor and (g.a_idx[0] or g.a_idx[1]):
        raise PlanRefused("a_idx")
    if g.add_src and not image:
        raise PlanRefused("add_src")
    tm, tn = cdiv(g.M, BM), cdiv(g.N, BN)
    plan = dict(vec=int(a_vec and b_vec), block=256, nsplit=1, chunk=0, grid_z=1,
                kind="gemm_devm" if g.m_dev else ("gemm_tn" if g.a_kmajor else ("gemm_nn" if g.b_kmajor else "gemm_nt")))
    if g.a_kmajor:
        if K[1] != 0:
            raise PlanRefused("one source")
        nsplit, chunk = split_k(K[0], cdiv(SPLIT_WGS, tm * tn * g.batch))
        if nsplit > 1 and g.b_kmajor and g.slabs:
            if g.batch != 1:
                raise PlanRefused("split-K with batch")
            if g.bias or g.relu or g.row_zero or g.relu_src:
                raise PlanRefused("no epilogue")
            return dict(plan, form="tn_group", grid_x=0, grid_y=0, grid_z=0, block=0, nsplit=nsplit, chunk=chunk, kind=None)
        return dict(plan, form="f32_128", grid_x=tm, grid_y=tn, grid_z=g.batch)
    tiles = tm * tn * g.batch
    if not image:
        if K[1] > 0 and g.b_img2:
            raise PlanRefused("two-source")
        small = tiles < F32_BIG_MIN_TILES
        return dict(plan, form="f32_32" if small else "f32_128", grid_x=cdiv(g.M, 32 if small else BM), grid_y=tn, grid_z=g.batch)
    if g.bx_force == 2 or (g.bx_force == 0 and tiles < BX_MIN_TILES):
        rows = cdiv(g.M, SK_ROWS)
        wide = rows * tn >= SK_WIDE_MIN_WGS
        return dict(plan, form="skinny11" if wide else "skinny4", grid_x=rows, grid_y=tn if wide else cdiv(g.N, 64), kind="gemm_bx_skinny")
    plain = not (g.bias or g.relu or g.relu_src or g.add_src or g.accumulate or g.row_scale or g.row_zero)
    if (K[1] == 0 and K[0] <= AS_KMAX and g.N % 32 == 0 and AS_NMIN <= g.N <= AS_NMAX and g.ldc % 4 == 0 and _aligned(g.C) and plain
            and g.M >= AS_MMIN):
        return dict(plan, form="astat", grid_x=cdiv(g.M, 128), grid_y=1, kind="gemm_bx")
    # one column tile: (row tile, column tile) = (x, y); more: a 1-D grid in the XCD tile order, row tiles padded to eights
    grid = (tm, 1) if tn == 1 else (cdiv(tm, 8) * 8 * tn, 1)
    eight = tiles >= BX_AREG8_MIN
    return dict(plan, form="areg8" if eight else "areg", grid_x=grid[0], grid_y=grid[1], block=512 if eight else 256, kind="gemm_bx")


def tn_plan_ref(probs, K, slab_floats=None):
    """What pfo_gemm_tn_group_launch does with the problems (TnDesc-like) over the extent K: the dict of gemm_plan_ref, and
    ``need`` = the slab floats the launch asks for, ``tile_rows`` = the A columns one workgroup tile takes (128 or 256; None
    for the fp32 form, which keeps no per-tile scale), ``xcd_map``.  ``slab_floats`` below ``need``: PlanRefused."""
    n = len(probs)
    if not (1 <= n <= 16 and K > 0):
        raise PlanRefused("bad arguments")
    if not all(q.A and q.B and q.C and q.M > 0 and q.N > 0 for q in probs):
        raise PlanRefused("bad problem")
    vec = all(_aligned(q.A) and _aligned(q.B) and q.lda % 4 == 0 and q.ldb % 4 == 0 and q.M % 4 == 0 and q.N % 4 == 0 for q in probs)
    tn8 = vec and all(q.M >= TN8_MIN_ROWS for q in probs)
    cols = [q.N + (1 if q.bias_out else 0) for q in probs]                       # the bias gradient rides as one more column
    rows = 256 if tn8 else BM
    tiles = sum(cdiv(q.M, rows) * cdiv(c, BN) for q, c in zip(probs, cols))
    nsplit, chunk = split_k(K, (TN8_SLOTS if tn8 else TN_SLOTS) // max(1, tiles))
    need = sum(q.M * c for q, c in zip(probs, cols)) * nsplit
    if slab_floats is not None and slab_floats < need:
        raise PlanRefused("workspace too small")
    xcd_map = int(vec and nsplit > 1)                                            # 1-D grid: every tile of one split on one XCD
    return dict(form="tn_f32" if not vec else ("tn_bx8" if tn8 else "tn_bx"), vec=int(vec), grid_x=tiles * nsplit if xcd_map else tiles,
                grid_y=1 if xcd_map else nsplit, grid_z=1, block=512 if tn8 else 256, nsplit=nsplit, chunk=chunk,
                kind="gemm_tn" if not vec else ("gemm_tn_bx8" if tn8 else "gemm_tn_bx"), need=need, tile_rows=rows if vec else None,
                xcd_map=xcd_map)


def gru_ref(msg, h, W_ih, W_hh, b_ih, b_hh, hm, touched, node_feat, n_rows, gather):
    """The lazy GRU of pfo_gru_fused_launch in float64 for rows m < n_rows.  gather = 0: msg / h / hm are packed rows; gather =
    1: they are the per-node tables and row m is node touched[m] of them.  node_feat is always the per-node table.

    Returns dict(upd_mem [n, D] = h' (h where hm == 0), h0_tab [n, D] = upd_mem + node_feat[touched], gates [n, 4 D] =
    r | z | n | gh_n, pre [n, 4 D] = the pre-activations pr | pz | gi_n | gh_n, pre_mag [n, 4 D] = sum |x||w| + |biases| of
    each pre-activation)."""
    from oracle import tgn_oracle as T
    n = int(n_rows)
    touched = np.asarray(touched).reshape(-1)[:n].astype(np.int64)
    sel = touched if gather else np.arange(n)
    x, hh = np.asarray(msg, f64)[sel], np.asarray(h, f64)[sel]
    has = np.asarray(hm).reshape(-1)[sel] != 0
    W_ih, W_hh, b_ih, b_hh = (np.asarray(a, f64) for a in (W_ih, W_hh, b_ih, b_hh))
    D = hh.shape[1]
    hn, (_, _, r, z, nn, ghn) = T.gru_cell(x, hh, W_ih, W_hh, b_ih, b_hh, dtype=f64)
    upd = np.where(has[:, None], hn, hh)
    gi, gh = x @ W_ih.T + b_ih, hh @ W_hh.T + b_hh
    mi, mh = np.abs(x) @ np.abs(W_ih).T + np.abs(b_ih), np.abs(hh) @ np.abs(W_hh).T + np.abs(b_hh)
    pre = np.concatenate([gi[:, :2 * D] + gh[:, :2 * D], gi[:, 2 * D:], gh[:, 2 * D:]], 1)
    pre_mag = np.concatenate([mi[:, :2 * D] + mh[:, :2 * D], mi[:, 2 * D:], mh[:, 2 * D:]], 1)
    return dict(upd_mem=upd, h0_tab=upd + np.asarray(node_feat, f64)[touched], gates=np.concatenate([r, z, nn, ghn], 1), pre=pre,
                pre_mag=pre_mag, has=has, h=hh)


def rank1_ref(u, ldu, v, ldv, M, N, out, ldo, reps=1, u_rs=0, v_rs=0):
    """out[m, n] += sum_{r < reps} u[r * u_rs + m * ldu] * v[r * v_rs + n * ldv] on flat buffers; returns (out, mag, written)."""
    u, v, o0 = _flat64(u), _flat64(v), _flat64(out)
    res, mag, written = o0.copy(), np.zeros_like(o0), np.zeros(o0.shape, bool)
    oi = (np.arange(M)[:, None] * ldo + np.arange(N)[None, :]).astype(np.int64)
    acc, m_ = np.zeros((M, N)), np.abs(o0[oi])
    for r in range(reps):
        ur, vr = u[r * u_rs + np.arange(M) * ldu], v[r * v_rs + np.arange(N) * ldv]
        acc += np.outer(ur, vr)
        m_ += np.outer(np.abs(ur), np.abs(vr))
    res[oi] = o0[oi] + acc
    mag[oi] = m_
    written[oi] = True
    return res, mag, written


def sum_slabs_ref(dst, src, stride, count, n_slabs=1, accumulate=1):
    """dst[i] (+)= sum_{s < n_slabs} src[s * stride + i], i < count; returns (dst, mag, written)."""
    d0, s = _flat64(dst), _flat64(src)
    res, mag, written = d0.copy(), np.zeros_like(d0), np.zeros(d0.shape, bool)
    i = np.arange(count)
    terms = np.stack([s[sl * stride + i] for sl in range(n_slabs)])
    res[:count] = terms.sum(0) + (d0[:count] if accumulate else 0.0)
    mag[:count] = np.abs(terms).sum(0) + (np.abs(d0[:count]) if accumulate else 0.0)
    written[:count] = True
    return res, mag, written
