"""The float64 models of tests/gemm_ref.py against independent formulations (explicit loops, np.einsum, torch float64 addmm /
relu / GRUCell), every feature alone and all combined: a wrong reference must not be able to bless a wrong kernel."""
import itertools

import numpy as np
import pytest
import torch

import gemm_ref as G

FEATURES = ["two_sources", "a_idx0", "a_idx1", "bias", "row_scale", "add_src", "add_idx", "row_zero", "relu", "relu_src", "accumulate",
            "m_dev", "a_kmajor", "b_kmajor", "b_idx", "batch"]


def _problem(rs, on, M=5, N=7, K0=6, K1=3):
    """A tiny problem with the features of ``on``: padded leading dimensions, gather tables larger than M, strides that leave
    gaps.  Returns the descriptor."""
    on = set(on)
    akm, bkm = "a_kmajor" in on, "b_kmajor" in on
    batch = 3 if "batch" in on else 1
    two = "two_sources" in on and not akm
    R = 11                                                     # rows of a gathered operand table
    d = dict(M=M, N=N, a_kmajor=int(akm), b_kmajor=int(bkm), batch=batch)
    Ks = [K0, K1 if two else 0]
    A, B, lda, ldb, a_bs, b_bs, a_idx = [None, None], [None, None], [0, 0], [0, 0], [0, 0], [0, 0], [None, None]
    for s in range(2):
        if Ks[s] == 0:
            continue
        gathered = ("a_idx%d" % s) in on and not akm
        if akm:
            lda[s] = M + 2; a_bs[s] = Ks[s] * lda[s] + 5
            A[s] = rs.randn(batch * a_bs[s] + 8)
        else:
            lda[s] = Ks[s] + 3; a_bs[s] = 2 if batch > 1 else 0          # (overlapping batches: a column offset, as tgn.hip's dh)
            A[s] = rs.randn((R if gathered else M) * lda[s] + batch * 2 + 8)
            if gathered:
                a_idx[s] = rs.randint(0, R, size=M + 4).astype(np.int32)
                a_idx[s][1] = a_idx[s][0]                                # repeated
        rows_b = Ks[s] + (4 if ("b_idx" in on and bkm and s == 0) else 0)
        if bkm:
            ldb[s] = N + 1; b_bs[s] = rows_b * ldb[s] + 3
        else:
            ldb[s] = Ks[s] + 2; b_bs[s] = N * ldb[s] + 1
        B[s] = rs.randn(batch * b_bs[s] + 8)
    d.update(A=A, B=B, lda=lda, ldb=ldb, a_bs=a_bs, b_bs=b_bs, a_idx=a_idx, K=Ks)
    if "b_idx" in on and bkm:
        d["b_idx"] = rs.permutation(Ks[0] + 4)[:Ks[0]].astype(np.int32)
    ldc = N + 2
    d.update(ldc=ldc, c_bs=M * ldc + 4, C=rs.randn(batch * (M * ldc + 4) + ldc * 2))
    if "bias" in on or "row_scale" in on:
        d.update(bias=rs.randn(batch * (N + 1)), bias_bs=N + 1)
    if "row_scale" in on:
        d.update(row_scale=rs.randn(batch * (3 * M + 2)), rs_ld=3, rs_bs=3 * M + 2)
    if "add_src" in on or "add_idx" in on:
        d.update(add_src=rs.randn(R * (N + 3)), add_ld=N + 3)
    if "add_idx" in on:
        d["add_idx"] = rs.randint(0, R, size=M).astype(np.int32)
    if "row_zero" in on:
        d["row_zero"] = (rs.rand(M) < 0.4).astype(np.uint8)
    if "relu" in on:
        d["relu"] = 1
    if "relu_src" in on:
        m = rs.randn(M * (N + 1))
        m[::3] = 0.0; m[1::5] = -0.0
        d.update(relu_src=m, relu_ld=N + 1)
    if "accumulate" in on:
        d["accumulate"] = 1
    if "m_dev" in on:
        d["m_dev"] = np.array([K0 - 2 if akm else M - 2], np.int32)
    return d


def _loops(d):
    """The header's sentence, element by element."""
    d = G.gemm_desc(**d)
    M, N = d["M"], d["N"]
    out = np.asarray(d["C"], np.float64).copy()
    mag = np.zeros_like(out)
    wr = np.zeros(out.shape, bool)
    K0, Mlim = d["K"][0], M
    if d["m_dev"] is not None:
        if d["a_kmajor"]:
            K0 = min(K0, int(d["m_dev"][0]))
        else:
            Mlim = min(M, int(d["m_dev"][0]))
    for z in range(d["batch"]):
        for m in range(Mlim):
            for n in range(N):
                v = g = 0.0
                for s in range(2):
                    for k in range(K0 if s == 0 else d["K"][1]):
                        if d["a_kmajor"]:
                            a = d["A"][s][z * d["a_bs"][s] + k * d["lda"][s] + m]
                        else:
                            r = m if d["a_idx"][s] is None else d["a_idx"][s][m]
                            a = d["A"][s][z * d["a_bs"][s] + r * d["lda"][s] + k]
                        if d["b_kmajor"]:
                            kk = d["b_idx"][k] if (d["b_idx"] is not None and s == 0) else k
                            b = d["B"][s][z * d["b_bs"][s] + kk * d["ldb"][s] + n]
                        else:
                            b = d["B"][s][z * d["b_bs"][s] + n * d["ldb"][s] + k]
                        v += a * b
                        g += abs(a * b)
                c = z * d["c_bs"] + m * d["ldc"] + n
                if d["accumulate"]:
                    v += d["C"][c]; g += abs(d["C"][c])
                if d["bias"] is not None:
                    t = d["bias"][z * d["bias_bs"] + n] * (1.0 if d["row_scale"] is None else d["row_scale"][z * d["rs_bs"] + m * d["rs_ld"]])
                    v += t; g += abs(t)
                if d["add_src"] is not None:
                    t = d["add_src"][(m if d["add_idx"] is None else d["add_idx"][m]) * d["add_ld"] + n]
                    v += t; g += abs(t)
                if d["row_zero"] is not None and d["row_zero"][m]:
                    v = 0.0
                if d["relu"] and v < 0:
                    v = 0.0
                if d["relu_src"] is not None and not d["relu_src"][m * d["relu_ld"] + n] > 0:
                    v = 0.0
                out[c], mag[c], wr[c] = v, g, True
    return out, mag, wr


SINGLE = [(f,) for f in FEATURES] + [("a_kmajor", "b_kmajor"), ("a_kmajor", "m_dev"), ("b_kmajor", "b_idx"), ("a_kmajor", "b_kmajor", "b_idx"),
                                     ("two_sources", "a_idx0"), ("two_sources", "a_idx1"), ("two_sources", "a_idx0", "a_idx1"),
                                     ("bias", "row_scale", "batch"), ("two_sources", "b_kmajor", "b_idx")]
ALL_ROWMAJOR = tuple(f for f in FEATURES if f != "a_kmajor")
ALL_KMAJOR = tuple(f for f in FEATURES if f not in ("two_sources", "a_idx0", "a_idx1"))


@pytest.mark.parametrize("on", [()] + SINGLE + [ALL_ROWMAJOR, ALL_KMAJOR], ids=lambda o: "+".join(o) or "plain")
def test_gemm_ref_matches_explicit_loops(on):
    rs = np.random.RandomState(len(on) * 7 + sum(map(len, on)))
    d = _problem(rs, on)
    out, mag, wr = G.gemm_ref(d)
    lo, lm, lw = _loops(d)
    assert np.array_equal(wr, lw)
    assert np.array_equal(out[~wr], np.asarray(d["C"])[~wr])                 # untouched elements keep their value, bit for bit
    assert np.abs(out - lo).max() < 1e-12 * max(1.0, np.abs(lm).max())
    assert np.abs(mag - lm).max() < 1e-12 * max(1.0, np.abs(lm).max())
    if "m_dev" in on and "a_kmajor" not in on:
        assert not wr.reshape(-1)[(d["M"] - 2) * d["ldc"]:d["M"] * d["ldc"]].any()
    if "relu_src" in on or "row_zero" in on or "relu" in on:
        assert (out[wr] == 0).any()                                           # the masks bite in this problem


@pytest.mark.parametrize("on", [(), ALL_ROWMAJOR[:-1]], ids=["plain", "all"])
def test_gemm_ref_row_subset_is_the_full_result_on_those_rows(on):
    rs = np.random.RandomState(21)
    d = _problem(rs, on, M=9)
    out, mag, wr = G.gemm_ref(d)
    so, sm, sw, rows = G.gemm_ref(d, rows=[0, 3, 8, 6, 3])
    assert np.array_equal(sw, wr)
    lim = 7 if "m_dev" in on else 9
    assert list(rows) == [r for r in (0, 3, 6, 8) if r < lim] and so.shape == (len(rows), d["N"])
    ci = rows[:, None] * d["ldc"] + np.arange(d["N"])[None, :]
    assert np.array_equal(so, out[ci]) and np.array_equal(sm, mag[ci])
    so2, sm2, none, rows2 = G.gemm_ref(d, rows=[0, 3, 8, 6, 3], want_written=False)
    assert none is None and np.array_equal(so2, so) and np.array_equal(sm2, sm) and np.array_equal(rows2, rows)


def test_gemm_ref_matches_torch_addmm_relu_and_einsum():
    """Contiguous operands, medium shapes: torch float64 addmm + relu; np.einsum for the two-source gathered form."""
    rs = np.random.RandomState(3)
    M, N, K, K1 = 37, 29, 41, 13
    A, W, bias, C0 = rs.randn(M, K), rs.randn(N, K), rs.randn(N), rs.randn(M, N)
    tA, tW, tb, tC = (torch.from_numpy(x) for x in (A, W, bias, C0))
    out, mag, wr = G.gemm_ref(dict(A=(A, None), lda=(K, 0), B=(W, None), ldb=(K, 0), K=(K, 0), M=M, N=N, C=C0, ldc=N, bias=bias, relu=1))
    assert wr.all()
    ref = torch.relu(torch.addmm(tb, tA, tW.T)).numpy()
    assert np.abs(out.reshape(M, N) - ref).max() < 1e-12
    assert np.abs(mag.reshape(M, N) - (np.einsum("mk,nk->mn", np.abs(A), np.abs(W)) + np.abs(bias))).max() < 1e-12
    # accumulate + k-major B
    out, _, _ = G.gemm_ref(dict(A=(A, None), lda=(K, 0), B=(W.T.copy(), None), ldb=(N, 0), K=(K, 0), M=M, N=N, C=C0, ldc=N, b_kmajor=1,
                               accumulate=1))
    assert np.abs(out.reshape(M, N) - torch.addmm(tC, tA, tW.T).numpy()).max() < 1e-12
    # k-major A (weight gradient layout): A^T B
    X = rs.randn(K, N)
    out, _, _ = G.gemm_ref(dict(A=(A.T.copy(), None), lda=(M, 0), B=(X, None), ldb=(N, 0), K=(K, 0), M=M, N=N, C=C0, ldc=N, a_kmajor=1,
                               b_kmajor=1))
    assert np.abs(out.reshape(M, N) - (tA @ torch.from_numpy(X)).numpy()).max() < 1e-12
    # two gathered sources, each against its own weight, + a gathered addend, row scale on the bias
    T0, T1, W1 = rs.randn(50, K), rs.randn(60, K1), rs.randn(N, K1)
    i0, i1, ia = rs.randint(0, 50, M), rs.randint(0, 60, M), rs.randint(0, 20, M)
    add, sc = rs.randn(20, N), rs.randn(M)
    out, mag, _ = G.gemm_ref(dict(A=(T0, T1), lda=(K, K1), a_idx=(i0.astype(np.int32), i1.astype(np.int32)), B=(W, W1), ldb=(K, K1),
                                  K=(K, K1), M=M, N=N, C=C0, ldc=N, bias=bias, row_scale=sc, rs_ld=1, add_src=add, add_ld=N,
                                  add_idx=ia.astype(np.int32)))
    ref = np.einsum("mk,nk->mn", T0[i0], W) + np.einsum("mk,nk->mn", T1[i1], W1) + np.outer(sc, bias) + add[ia]
    assert np.abs(out.reshape(M, N) - ref).max() < 1e-12
    rmag = np.abs(T0[i0]) @ np.abs(W).T + np.abs(T1[i1]) @ np.abs(W1).T + np.abs(np.outer(sc, bias)) + np.abs(add[ia])
    assert np.abs(mag.reshape(M, N) - rmag).max() < 1e-12


def test_gemm_ref_epilogue_order_is_the_documented_one():
    """Problems on which every other order of the epilogue steps gives a different answer."""
    A, W = np.array([[1.0]]), np.array([[2.0]])
    base = dict(A=(A, None), lda=(1, 0), B=(W, None), ldb=(1, 0), K=(1, 0), M=1, N=1, ldc=1)
    one = lambda **kw: G.gemm_ref(dict(base, **kw))[0][0]
    assert one(C=np.array([-10.0]), accumulate=1, relu=1) == 0.0                       # the ReLU sees the accumulated value
    assert one(C=np.array([0.0]), bias=np.array([-5.0]), relu=1) == 0.0                 # ... and the bias
    assert one(C=np.array([0.0]), add_src=np.array([-5.0]), add_ld=1, relu=1) == 0.0    # ... and the addend
    assert one(C=np.array([7.0]), accumulate=1, bias=np.array([3.0]), add_src=np.array([4.0]), add_ld=1,
               row_zero=np.array([1], np.uint8)) == 0.0                                 # row_zero clears every addend
    assert one(C=np.array([0.0]), bias=np.array([3.0]), row_scale=np.array([-2.0])) == 2.0 - 6.0   # the scale multiplies the bias alone
    assert one(C=np.array([0.0]), relu_src=np.array([-0.0]), relu_ld=1) == 0.0          # -0 and 0 are not > 0
    assert one(C=np.array([0.0]), relu_src=np.array([1e-45]), relu_ld=1) == 2.0
    assert one(C=np.array([0.0]), bias=np.array([-5.0]), relu_src=np.array([1.0]), relu_ld=1) == -3.0   # a mask, not a ReLU


@pytest.mark.parametrize("c_acc,b_acc,with_bias,gather,k_dev", list(itertools.product([0, 1], [0, 1], [0, 1], [0, 1], [None, 0, 5, 40])))
def test_tn_group_ref_matches_einsum(c_acc, b_acc, with_bias, gather, k_dev):
    rs = np.random.RandomState(11)
    K = 13
    probs, raw = [], []
    for M, N in ((4, 6), (9, 3)):
        A, B = rs.randn(K, M + 2), rs.randn(K + 7, N + 1)
        bi = rs.permutation(K + 7)[:K].astype(np.int32) if gather else None
        C0, b0 = rs.randn(M + 1, N + 3), rs.randn(M + 2)
        probs.append(dict(A=A, lda=M + 2, B=B, ldb=N + 1, b_idx=bi, M=M, N=N, C=C0, ldc=N + 3, c_accumulate=c_acc,
                          bias_out=b0 if with_bias else None, bias_accumulate=b_acc))
        raw.append((A, B, bi, C0, b0, M, N))
    res = G.tn_group_ref(probs, K, None if k_dev is None else np.array([k_dev], np.int32))
    ke = K if k_dev is None else min(K, k_dev)
    for r, (A, B, bi, C0, b0, M, N) in zip(res, raw):
        Bg = B[bi[:ke]] if gather else B[:ke]
        ref = np.einsum("km,kn->mn", A[:ke, :M], Bg[:, :N]) + (C0[:M, :N] if c_acc else 0)
        got = r["C"].reshape(C0.shape)
        assert np.abs(got[:M, :N] - ref).max() < 1e-12
        wr = r["C_written"].reshape(C0.shape)
        assert wr[:M, :N].all() and wr.sum() == M * N and np.array_equal(got[~wr], C0[~wr])
        rmag = np.einsum("km,kn->mn", np.abs(A[:ke, :M]), np.abs(Bg[:, :N])) + (np.abs(C0[:M, :N]) if c_acc else 0)
        assert np.abs(r["C_mag"].reshape(C0.shape)[:M, :N] - rmag).max() < 1e-12
        if with_bias:
            assert np.abs(r["bias"][:M] - (A[:ke, :M].sum(0) + (b0[:M] if b_acc else 0))).max() < 1e-12
            assert np.array_equal(r["bias"][M:], b0[M:])
            assert np.abs(r["bias_mag"][:M] - (np.abs(A[:ke, :M]).sum(0) + (np.abs(b0[:M]) if b_acc else 0))).max() < 1e-12
        else:
            assert r["bias"] is None


def test_tn_group_ref_floored_magnitude_is_the_shared_helper_on_the_extended_operand():
    rs = np.random.RandomState(2)
    K, M, N = 70, 9, 5                                                  # K no multiple of the k-tile: zero rows pad it
    A, B = G.wide(rs, K, M).astype(np.float64), G.wide(rs, K, N).astype(np.float64)
    r = G.tn_group_ref([dict(A=A, lda=M, B=B, ldb=N, M=M, N=N, C=np.zeros(M * N), ldc=N, c_accumulate=0, bias_out=np.zeros(M),
                             bias_accumulate=0)], K, a_block=4, b_block=4)[0]
    Ap, Bp = np.pad(A, ((0, 26), (0, 0))), np.pad(np.concatenate([B, np.ones((K, 1))], 1), ((0, 26), (0, 0)))
    ref = G.tn_scale_floor(Ap, 4)[:K].T @ G.tn_scale_floor(Bp, 4)[:K]         # (the padding rows themselves add nothing)
    assert np.allclose(r["C_mag"].reshape(M, N), ref[:, :N], rtol=1e-13) and np.allclose(r["bias_mag"], ref[:, N], rtol=1e-13)
    plain = G.tn_group_ref([dict(A=A, lda=M, B=B, ldb=N, M=M, N=N, C=np.zeros(M * N), ldc=N, c_accumulate=0)], K)[0]
    assert (r["C_mag"] >= plain["C_mag"] - 1e-9).all() and (r["C_mag"] > plain["C_mag"]).any()      # a floor only raises


@pytest.mark.parametrize("gather", [0, 1])
def test_gru_ref_matches_torch_grucell(gather):
    rs = np.random.RandomState(5)
    D, Km, nodes, n = 8, 28, 30, 9
    cell = torch.nn.GRUCell(Km, D).double()
    W_ih, W_hh, b_ih, b_hh = (p.detach().numpy() for p in (cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh))
    touched = rs.permutation(nodes)[:n + 3].astype(np.int32)
    nf = rs.randn(nodes, D)
    rows = nodes if gather else n + 3
    msg, h = rs.randn(rows, Km), rs.randn(rows, D)
    hm = (rs.rand(rows) < 0.6).astype(np.uint8)
    r = G.gru_ref(msg, h, W_ih, W_hh, b_ih, b_hh, hm, touched, nf, n, gather)
    sel = touched[:n] if gather else np.arange(n)
    with torch.no_grad():
        hn = cell(torch.from_numpy(msg[sel]), torch.from_numpy(h[sel])).numpy()
    keep = hm[sel] == 0
    assert keep.any() and (~keep).any()
    assert np.abs(r["upd_mem"][~keep] - hn[~keep]).max() < 1e-13
    assert np.array_equal(r["upd_mem"][keep], h[sel][keep])                       # kept bit for bit
    assert np.abs(r["h0_tab"] - (r["upd_mem"] + nf[touched[:n]])).max() == 0
    assert r["upd_mem"].shape == (n, D) and r["gates"].shape == (n, 4 * D)
    # the gates layout r | z | n | gh_n rebuilds h' by the cell's own formula, and the pre-activations rebuild the gates
    g = r["gates"]
    rr, zz, nn, ghn = g[:, :D], g[:, D:2 * D], g[:, 2 * D:3 * D], g[:, 3 * D:]
    assert np.abs(((1 - zz) * nn + zz * h[sel]) - hn).max() < 1e-13
    assert np.abs(ghn - (h[sel] @ W_hh[2 * D:].T + b_hh[2 * D:])).max() < 1e-13
    p = r["pre"]
    sig = lambda x: 1 / (1 + np.exp(-x))
    assert np.abs(sig(p[:, :D]) - rr).max() < 1e-13 and np.abs(sig(p[:, D:2 * D]) - zz).max() < 1e-13
    assert np.abs(np.tanh(p[:, 2 * D:3 * D] + rr * p[:, 3 * D:]) - nn).max() < 1e-13
    gi = torch.from_numpy(msg[sel]) @ cell.weight_ih.detach().T + cell.bias_ih.detach()
    assert np.abs(p[:, 2 * D:3 * D] - gi[:, 2 * D:].numpy()).max() < 1e-13
    mi = np.abs(msg[sel]) @ np.abs(W_ih).T + np.abs(b_ih)
    mh = np.abs(h[sel]) @ np.abs(W_hh).T + np.abs(b_hh)
    assert np.abs(r["pre_mag"][:, :D] - (mi[:, :D] + mh[:, :D])).max() < 1e-12
    assert np.abs(r["pre_mag"][:, 3 * D:] - mh[:, 2 * D:]).max() < 1e-12
    assert G.gru_ref(msg, h, W_ih, W_hh, b_ih, b_hh, hm, touched, nf, 0, gather)["upd_mem"].shape == (0, D)


@pytest.mark.parametrize("reps", [1, 3])
def test_rank1_ref_matches_loops(reps):
    rs = np.random.RandomState(reps)
    M, N, ldu, ldv, ldo, u_rs, v_rs = 4, 5, 2, 3, 7, 9, 16
    u, v, out = rs.randn(reps * u_rs + M * ldu), rs.randn(reps * v_rs + N * ldv), rs.randn(M * ldo + 2)
    res, mag, wr = G.rank1_ref(u, ldu, v, ldv, M, N, out, ldo, reps, u_rs, v_rs)
    exp, emag = out.copy(), np.zeros_like(out)
    for m in range(M):
        for n in range(N):
            emag[m * ldo + n] = abs(out[m * ldo + n])
            for r in range(reps):
                t = u[r * u_rs + m * ldu] * v[r * v_rs + n * ldv]
                exp[m * ldo + n] += t
                emag[m * ldo + n] += abs(t)
    assert np.abs(res - exp).max() < 1e-13 and np.abs(mag - emag).max() < 1e-13
    assert wr.sum() == M * N and np.array_equal(res[~wr], out[~wr])


@pytest.mark.parametrize("acc", [0, 1])
def test_sum_slabs_ref_matches_loops(acc):
    rs = np.random.RandomState(4)
    count, stride, ns = 6, 8, 3
    dst, src = rs.randn(count + 3), rs.randn(ns * stride)
    res, mag, wr = G.sum_slabs_ref(dst, src, stride, count, ns, acc)
    for i in range(count):
        e = sum(src[s * stride + i] for s in range(ns)) + (dst[i] if acc else 0)
        assert abs(res[i] - e) < 1e-13
        assert abs(mag[i] - (sum(abs(src[s * stride + i]) for s in range(ns)) + (abs(dst[i]) if acc else 0))) < 1e-13
    assert np.array_equal(res[count:], dst[count:]) and wr.sum() == count


def test_wide_generator_is_the_split_contraction_tests_generator():
    a = G.wide(np.random.RandomState(9), 4, 5)
    rs = np.random.RandomState(9)
    b = (rs.randn(4, 5) * np.exp(2 * rs.randn(4, 5))).astype(np.float32)
    assert a.dtype == np.float32 and np.array_equal(a, b)
