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
    (128 columns of A, 176 of B: gemm.hip BM / BN) and K-slab (a slab starts later than row 0, so its running maximum is at
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
