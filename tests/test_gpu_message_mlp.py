"""The fused GRU's third input form (gather = 2): message rows PACKED per touched row - the MLP message function's output -
while memory, has_msg and node features are the per-node tables gathered through ``touched``.  Method, operands and bounds of
tests/test_gpu_gemm_forms.py::test_gru_fused: wide-range operands, canaries behind every output, the float64 cell of
tests/gemm_ref.py at gru_bounds, the profiler asserting the family that ran."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

from pfotgnrec_amd import _lib
import gemm_ref as G
import test_gpu_gemm_forms as F

f64 = np.float64


class PackedMessageGruCase(F.GruCase):
    """GruCase with a message width of its own (weight_ih is [3D, message_dimension])."""

    def __init__(self, D, K_msg, weights):
        self.D, self.K_msg = D, K_msg
        self.W = weights
        self.b = F.Bufs()
        b = self.b
        W_ih, W_hh, b_ih, b_hh = weights
        self.p_bih, self.p_bhh = b.put(b_ih, np.float32), b.put(b_hh, np.float32)
        self.img = []
        for W, K, gate in ((W_ih, K_msg, 1), (W_hh, D, 2)):
            dst = b.raw(_lib.byte_count("pfo_debug_gru_img_bytes", D, K))
            d = _lib.BimgDesc(src=b.put(W, np.float32), ld=K, N=3 * D, K=K, trans=0, dst=dst, gate=gate, gate_D=D)
            _lib.call("pfo_debug_bimg", C.byref(d), 1, _lib.stream_ptr())
            self.img.append(dst)
        self.gather = 2


@pytest.mark.parametrize("scaled", [False, True], ids=["init", "blocks_2^9_apart"])
@pytest.mark.parametrize("D,K_msg", [(8, 4), (16, 12), (32, 100), (64, 100), (172, 100)])
def test_gru_fused_with_packed_messages_and_gathered_state(D, K_msg, scaled):
    """cap_rows in {1, 129, 300}, n_rows in {0, 1, cap - 1, cap}, a non-monotonic ``touched``; rows without a pending message keep
    their memory row bit for bit whatever their (packed) message row holds - NaN here."""
    rs = np.random.RandomState(D + K_msg + scaled)
    case = PackedMessageGruCase(D, K_msg, F.gru_weights(D, K_msg, scaled, seed=D + K_msg))
    for cap in (1, 129, 300):
        make = lambda *s: 0.05 * G.wide(rs, *s)
        _, h_tab, hm_tab, touched, nf = F.gru_operands(rs, D, K_msg, cap, 1, make)
        assert cap < 3 or (np.diff(touched) < 0).any()
        msg = make(cap, K_msg)                                               # packed: row m belongs to node touched[m]
        for n_rows in sorted({0, 1, cap - 1, cap}):
            msg_dev = msg.copy()
            msg_dev[hm_tab[touched] == 0] = np.nan                           # never used: those rows keep h
            (upd, h0, gates), canaries, kinds = case.run(msg_dev, h_tab, hm_tab, touched, nf, cap, n_rows)
            assert kinds == {"gru_fused": 1}, kinds
            for got, can in zip((upd, h0, gates), canaries):
                assert np.array_equal(F.bits(got[n_rows:]), F.bits(can.reshape(got.shape)[n_rows:])), "rows >= n_rows touched"
            # the float64 cell on packed rows: state rows gathered on the host
            r = G.gru_ref(msg, h_tab[touched], *case.W, hm_tab[touched], touched, nf, n_rows, 0)
            b_h, b_h0, b_g = F.gru_bounds(r, nf.astype(f64)[touched[:n_rows]])
            has = r["has"]
            for name, got, ref, bound in (("upd_mem", upd, r["upd_mem"], b_h), ("h0_tab", h0, r["h0_tab"], b_h0)):
                diff = np.abs(got[:n_rows].astype(f64) - ref)
                assert np.isfinite(got[:n_rows]).all() and (diff <= bound).all(), (name, float((diff - bound).max()))
            diff = np.abs(gates[:n_rows].astype(f64) - r["gates"])[has]
            assert np.isfinite(gates[:n_rows][has]).all() and (diff <= b_g[has]).all(), ("gates", float((diff - b_g[has]).max()))
            keep = ~has
            assert np.array_equal(F.bits(upd[:n_rows][keep]), F.bits(h_tab[touched[:n_rows]][keep])), "a row without a message must keep h bit for bit"
            if n_rows > 1:
                assert keep.any() and has.any()


def test_gather_forms_zero_and_one_are_unchanged_by_the_third():
    """The same rows through gather = 0, 1 and 2 give bitwise the same outputs: the three forms differ in where a row is read."""
    D, K_msg, cap = 32, 100, 129
    rs = np.random.RandomState(3)
    W = F.gru_weights(D, K_msg, False, seed=1)
    make = lambda *s: 0.05 * G.wide(rs, *s)
    _, h_tab, hm_tab, touched, nf = F.gru_operands(rs, D, K_msg, cap, 1, make)
    msg = make(cap, K_msg)
    msg_tab = np.zeros((len(h_tab), K_msg), np.float32)
    msg_tab[touched] = msg
    outs = []
    for gather, (m, h, hm) in ((0, (msg, h_tab[touched], hm_tab[touched])), (1, (msg_tab, h_tab, hm_tab)), (2, (msg, h_tab, hm_tab))):
        case = PackedMessageGruCase(D, K_msg, W)
        case.gather = gather
        (upd, h0, gates), _, kinds = case.run(m, h, hm, touched, nf, cap, cap - 1)
        assert kinds == {"gru_fused": 1}
        outs.append((upd, h0, gates))
    for k in (1, 2):
        for a, b in zip(outs[0], outs[k]):
            assert np.array_equal(F.bits(a), F.bits(b)), k


# ------------------------------------------------------------------------------------------------ the fused MLP forward
TOL = F.TOL                                                                  # 4e-6 x magnitude


def _image(b, W):
    N, K = W.shape
    dst = b.raw(_lib.byte_count("pfo_debug_bimg_bytes", N, K))
    d = _lib.BimgDesc(src=b.put(W, np.float32), ld=K, N=N, K=K, trans=0, dst=dst)
    _lib.call("pfo_debug_bimg", C.byref(d), 1, _lib.stream_ptr())
    return dst


def mlp_ref(x, W1, b1, W2, b2):
    """float64 MLP of the rows ``x`` -> (hid, out, bound_hid, bound_out), the bounds per element:
    bound_hid = 4e-6 (sum |x||W1| + |b1|); bound_out = 4e-6 (sum |hid||W2| + |b2|) + sum_j |W2[n, j]| bound_hid[j] (ReLU is
    1-Lipschitz, so nothing is masked)."""
    x, W1, b1, W2, b2 = (np.asarray(a, f64) for a in (x, W1, b1, W2, b2))
    hid = np.maximum(x @ W1.T + b1, 0)
    b_hid = TOL * (np.abs(x) @ np.abs(W1).T + np.abs(b1))
    out = hid @ W2.T + b2
    b_out = TOL * (hid @ np.abs(W2).T + np.abs(b2)) + b_hid @ np.abs(W2).T
    return hid, out, b_hid, b_out


@pytest.mark.parametrize("with_hid", [True, False], ids=["hid", "no_hid"])
@pytest.mark.parametrize("gather", [True, False], ids=["gathered", "packed"])
@pytest.mark.parametrize("D,Ef,Md", [(8, 4, 4), (16, 0, 12), (32, 4, 100), (64, 8, 100), (172, 4, 100)])
def test_msg_mlp_fwd(D, Ef, Md, gather, with_hid):
    """pfo_msg_mlp_fwd_launch against float64: cap_rows in {1, 129, 300}, n_rows in {0, 1, cap - 1, cap}, a non-monotonic
    ``touched`` or packed rows, with and without the hidden output; rows with hm == 0 hold NaN and must give finite zeros; rows
    >= n_rows and the canaries behind both outputs untouched."""
    Mr = 3 * D + Ef
    Hm = Mr // 2
    rs = np.random.RandomState(D + Ef + Md + 2 * gather + with_hid)
    torch.manual_seed(D + Md)
    l1, l2 = torch.nn.Linear(Mr, Hm), torch.nn.Linear(Hm, Md)             # the module's own initialiser
    W1, b1, W2, b2 = (t.detach().numpy().copy() for t in (l1.weight, l1.bias, l2.weight, l2.bias))
    wb = F.Bufs()
    img1, img2 = _image(wb, W1), _image(wb, W2)
    p_b1, p_b2 = wb.put(b1, np.float32), wb.put(b2, np.float32)
    for cap in (1, 129, 300):
        nodes = cap + 37
        touched = np.sort(rs.permutation(nodes)[:cap]).astype(np.int32)
        rs.shuffle(touched)
        rows = nodes if gather else cap
        raw = (0.05 * G.wide(rs, rows, Mr)).astype(np.float32)
        hm = (rs.rand(rows) < 0.7).astype(np.uint8)
        hm[touched[0] if gather else 0] = 0
        raw_dev = raw.copy()
        raw_dev[hm == 0] = np.nan                                           # never read
        sel = touched if gather else np.arange(cap)
        for n_rows in sorted({0, 1, cap - 1, cap}):
            b = F.Bufs()
            c_hid, c_out = F.canary((cap + 2) * Hm), F.canary((cap + 2) * Md)
            f = _lib.MsgMlpDesc(raw=b.put(raw_dev, np.float32), ld_raw=Mr, touched=b.put(touched, np.int32) if gather else None,
                                hm=b.put(hm, np.uint8), img_w1=img1, img_w2=img2, b1=p_b1, b2=p_b2, Mr=Mr, Hm=Hm, Md=Md, cap_rows=cap,
                                n_rows=b.put(np.array([n_rows], np.int32), np.int32))
            f.msg_out = b.put(c_out, np.float32)
            t_out = b.keep[-1]
            t_hid = None
            if with_hid:
                f.hid = b.put(c_hid, np.float32)
                t_hid = b.keep[-1]
            _lib.call("pfo_debug_msg_mlp_fwd", C.byref(f), _lib.stream_ptr())
            torch.cuda.synchronize()
            out = t_out[:c_out.size].cpu().numpy().reshape(cap + 2, Md)
            assert np.array_equal(F.bits(out[n_rows:]), F.bits(c_out.reshape(cap + 2, Md)[n_rows:])), "rows >= n_rows touched"
            has = hm[sel[:n_rows]] != 0
            r_hid, r_out, b_hid, b_out = mlp_ref(np.where(has[:, None], raw[sel[:n_rows]], 0), W1, b1, W2, b2)
            assert np.isfinite(out[:n_rows]).all()
            assert (out[:n_rows][~has] == 0).all(), "a row without a message must give zeros"
            diff = np.abs(out[:n_rows].astype(f64) - r_out)[has]
            assert (diff <= b_out[has]).all(), ("msg_out", float((diff - b_out[has]).max()))
            if with_hid:
                hid = t_hid[:c_hid.size].cpu().numpy().reshape(cap + 2, Hm)
                assert np.array_equal(F.bits(hid[n_rows:]), F.bits(c_hid.reshape(cap + 2, Hm)[n_rows:])), "hidden rows >= n_rows touched"
                assert np.isfinite(hid[:n_rows]).all() and (hid[:n_rows][~has] == 0).all()
                diff = np.abs(hid[:n_rows].astype(f64) - r_hid)[has]
                assert (diff <= b_hid[has]).all(), ("hid", float((diff - b_hid[has]).max()))
            if n_rows > 1:
                assert has.any() and (~has).any()


def test_msg_mlp_fwd_refuses_bad_arguments():
    Pn = 1 << 12
    ok = dict(raw=Pn, ld_raw=28, hm=Pn, img_w1=Pn, img_w2=Pn, b1=Pn, b2=Pn, msg_out=Pn, Mr=28, Hm=14, Md=4, cap_rows=5, n_rows=Pn)
    for change, word in ((dict(msg_out=None), "null argument"), (dict(img_w2=None), "null argument"), (dict(Md=6), "bad sizes"),
                         (dict(Mr=30, ld_raw=30), "bad sizes"), (dict(cap_rows=0), "bad sizes"), (dict(raw=Pn + 4), "16-byte aligned")):
        f = _lib.MsgMlpDesc(**dict(ok, **change))
        with pytest.raises(_lib.PfoError, match=word):
            _lib.call("pfo_debug_msg_mlp_fwd", C.byref(f), _lib.stream_ptr())


# ------------------------------------------------------------------------------------------------ the composed forward chain
def _gemm(b, **kw):
    """One pfo_debug_gemm launch with the profiler on -> the contraction family that ran."""
    d = _lib.GemmDesc(batch=1, rs_ld=1)
    for k, v in kw.items():
        if k in ("A", "lda", "a_idx", "B", "ldb", "K"):
            getattr(d, k)[0] = v
        else:
            setattr(d, k, v)
    with F.profiled() as p:
        _lib.call("pfo_debug_gemm", C.byref(d), _lib.stream_ptr())
        torch.cuda.synchronize()
    assert len(p.kinds) == 1 and list(p.kinds.values()) == [1], p.kinds
    return next(iter(p.kinds))


IMAGE_KINDS = ("gemm_bx", "gemm_bx_skinny")


def _local_bound(kind, K_, mag):
    """Per-element bound of ONE contraction from its magnitude sum, by the family that ran: 4e-6 mag for the image
    kernels, (K + 4) 2^-23 mag for the fp32 kernel."""
    return TOL * mag if kind in IMAGE_KINDS else (K_ + 4) * 2.0 ** -23 * mag


@pytest.mark.parametrize("gather", [True, False], ids=["gathered", "packed"])
@pytest.mark.parametrize("D,Ef,Md", [(8, 4, 4), (16, 0, 12), (32, 4, 100), (64, 8, 100), (172, 4, 100)])
def test_composed_forward_chain(D, Ef, Md, gather):
    """The two contractions the step queues for the MLP's forward (tgn.hip message_mlp: raw rows gathered through ``touched`` or
    packed, W1 / W2 images, ReLU in the first epilogue, device-side row count), through the contraction probe with the same
    descriptors, at the per-element bounds of the fused kernel: bound_hid = 4e-6 (sum |x||W1| + |b1|), bound_out = 4e-6
    (sum |hid||W2| + |b2|) + sum |W2| bound_hid.  The family that ran is asserted: the first contraction always takes an image
    kernel, the second one too unless the hidden width is no multiple of 4 (float4 staging) - only then, and only for its own
    term, the fp32 kernel's bound stands in.  ``msg_out`` is written with ldc > N.  The chain computes EVERY row below n_rows,
    pending message or not (the GRU behind it ignores the others), so every row is compared; rows >= n_rows and the padding
    columns stay untouched."""
    Mr = 3 * D + Ef
    Hm = Mr // 2
    ldo = Md + 4
    rs = np.random.RandomState(D + Ef + Md + 2 * gather)
    torch.manual_seed(D + Md)
    l1, l2 = torch.nn.Linear(Mr, Hm), torch.nn.Linear(Hm, Md)
    W1, b1, W2, b2 = (t.detach().numpy().copy() for t in (l1.weight, l1.bias, l2.weight, l2.bias))
    wb = F.Bufs()
    img1, img2 = _image(wb, W1), _image(wb, W2)
    p_W1, p_W2 = wb.put(W1, np.float32), wb.put(W2, np.float32)
    p_b1, p_b2 = wb.put(b1, np.float32), wb.put(b2, np.float32)
    for cap in (1, 129, 300):
        nodes = cap + 37
        touched = np.sort(rs.permutation(nodes)[:cap]).astype(np.int32)
        rs.shuffle(touched)
        rows = nodes if gather else cap
        raw = (0.05 * G.wide(rs, rows, Mr)).astype(np.float32)
        sel = touched if gather else np.arange(cap)
        for n_rows in sorted({0, 1, cap - 1, cap}):
            b = F.Bufs()
            c_hid, c_out = F.canary((cap + 2) * Hm), F.canary((cap + 2) * ldo)
            p_n = b.put(np.array([n_rows], np.int32), np.int32)
            p_hid = b.put(c_hid, np.float32); t_hid = b.keep[-1]
            p_out = b.put(c_out, np.float32); t_out = b.keep[-1]
            k1 = _gemm(b, A=b.put(raw, np.float32), lda=Mr, a_idx=b.put(touched, np.int32) if gather else None, B=p_W1, ldb=Mr, K=Mr,
                       C=p_hid, ldc=Hm, M=cap, N=Hm, bias=p_b1, relu=1, m_dev=p_n, b_img=img1)
            k2 = _gemm(b, A=p_hid, lda=Hm, B=p_W2, ldb=Hm, K=Hm, C=p_out, ldc=ldo, M=cap, N=Md, bias=p_b2, m_dev=p_n, b_img=img2)
            assert k1 in IMAGE_KINDS, k1
            assert (k2 in IMAGE_KINDS) == (Hm % 4 == 0), (k2, Hm)
            hid = t_hid[:c_hid.size].cpu().numpy().reshape(cap + 2, Hm)
            out = t_out[:c_out.size].cpu().numpy().reshape(cap + 2, ldo)
            can = c_out.reshape(cap + 2, ldo)
            assert np.array_equal(F.bits(out[n_rows:]), F.bits(can[n_rows:])) and np.array_equal(F.bits(out[:, Md:]), F.bits(can[:, Md:]))
            assert np.array_equal(F.bits(hid[n_rows:]), F.bits(c_hid.reshape(cap + 2, Hm)[n_rows:]))
            out = out[:, :Md]
            r_hid, r_out, b_hid, b_out = mlp_ref(raw[sel[:n_rows]], W1, b1, W2, b2)
            assert np.isfinite(out[:n_rows]).all() and np.isfinite(hid[:n_rows]).all()
            carried = b_hid @ np.abs(W2.astype(f64)).T                     # layer 1's error through layer 2
            bo = _local_bound(k2, Hm, (b_out - carried) / TOL) + carried
            d_h, d_o = np.abs(hid[:n_rows].astype(f64) - r_hid), np.abs(out[:n_rows].astype(f64) - r_out)
            assert (d_h <= b_hid).all(), ("hid", float((d_h - b_hid).max()))
            assert (d_o <= bo).all(), ("msg_out", float((d_o - bo).max()))


# ------------------------------------------------------------------------------------------------ the backward's data path
def _image_t(b, W):
    """image of W^T (rows = columns of W): what d x = d y W reads"""
    K, N = W.shape
    dst = b.raw(_lib.byte_count("pfo_debug_bimg_bytes", N, K))
    d = _lib.BimgDesc(src=b.put(W, np.float32), ld=N, N=N, K=K, trans=1, dst=dst)
    _lib.call("pfo_debug_bimg", C.byref(d), 1, _lib.stream_ptr())
    return dst


def mlp_bwd_ref(dgi, hid, W_ih, W2):
    """float64 -> (dm, dhid, bound_dm, bound_dhid): bound_dm = 4e-6 sum |dgi||W_ih|; bound_dhid = 4e-6 sum |dm||W2| +
    sum |W2| bound_dm where hid > 0; exactly 0 where hid == 0."""
    dgi, hid, W_ih, W2 = (np.asarray(a, f64) for a in (dgi, hid, W_ih, W2))
    dm = dgi @ W_ih
    b_dm = TOL * (np.abs(dgi) @ np.abs(W_ih))
    dhid = (dm @ W2) * (hid > 0)
    b_dhid = (TOL * (np.abs(dm) @ np.abs(W2)) + b_dm @ np.abs(W2)) * (hid > 0)
    return dm, dhid, b_dm, b_dhid


@pytest.mark.parametrize("form", ["fused", "fused_no_dm", "composed"])
@pytest.mark.parametrize("D,Ef,Md", [(8, 4, 4), (16, 0, 12), (32, 4, 100), (64, 8, 100), (172, 4, 100)])
def test_msg_mlp_bwd(D, Ef, Md, form):
    """d m = dgi W_ih, d hid = (d m W2) (hid > 0) against float64, ``hid`` an input of the test (zeros, negative zeros and
    positives): pfo_msg_mlp_bwd_launch with and without the d m output, and the two contractions the step queues
    (tgn.hip backward_gru) through the contraction probe; cap_rows in {1, 129, 300}, n_rows in {0, 1, cap - 1, cap}; exactly 0.0
    where hid == 0; rows >= n_rows and the canaries untouched."""
    Mr = 3 * D + Ef
    Hm, D3 = Mr // 2, 3 * D
    rs = np.random.RandomState(D + Ef + Md + len(form))
    torch.manual_seed(D + Md + 1)
    cell, l2 = torch.nn.GRUCell(Md, D), torch.nn.Linear(Hm, Md)
    W_ih, W2 = cell.weight_ih.detach().numpy().copy(), l2.weight.detach().numpy().copy()
    wb = F.Bufs()
    imgA, imgB = _image_t(wb, W_ih), _image_t(wb, W2)
    p_Wih, p_W2 = wb.put(W_ih, np.float32), wb.put(W2, np.float32)
    for cap in (1, 129, 300):
        dgi = (0.05 * G.wide(rs, cap, D3)).astype(np.float32)
        hid = np.abs(0.05 * G.wide(rs, cap, Hm)).astype(np.float32)
        dead = rs.rand(cap, Hm) < 0.4
        hid[dead] = np.where(rs.rand(int(dead.sum())) < 0.5, 0.0, -0.0).astype(np.float32)
        for n_rows in sorted({0, 1, cap - 1, cap}):
            b = F.Bufs()
            c_dm, c_dh = F.canary((cap + 2) * Md), F.canary((cap + 2) * Hm)
            p_n = b.put(np.array([n_rows], np.int32), np.int32)
            p_hid, p_dgi = b.put(hid, np.float32), b.put(dgi, np.float32)
            p_dm = b.put(c_dm, np.float32); t_dm = b.keep[-1]
            p_dh = b.put(c_dh, np.float32); t_dh = b.keep[-1]
            if form == "composed":                                         # (both are image launches at every shape: A rows and K are multiples of 4)
                k1 = _gemm(b, A=p_dgi, lda=D3, B=p_Wih, ldb=Md, K=D3, C=p_dm, ldc=Md, M=cap, N=Md, b_kmajor=1, m_dev=p_n, b_img=imgA)
                k2 = _gemm(b, A=p_dm, lda=Md, B=p_W2, ldb=Hm, K=Md, C=p_dh, ldc=Hm, M=cap, N=Hm, b_kmajor=1, m_dev=p_n, b_img=imgB,
                           relu_src=p_hid, relu_ld=Hm)
                assert k1 in IMAGE_KINDS and k2 in IMAGE_KINDS, (k1, k2)
            else:
                f = _lib.MsgMlpBwdDesc(dgi=p_dgi, hid=p_hid, img_wihT=imgA, img_w2T=imgB, d_m=p_dm if form == "fused" else None,
                                       d_hid=p_dh, D3=D3, Hm=Hm, Md=Md, cap_rows=cap, n_rows=p_n)
                _lib.call("pfo_debug_msg_mlp_bwd", C.byref(f), _lib.stream_ptr())
            torch.cuda.synchronize()
            dm = t_dm[:c_dm.size].cpu().numpy().reshape(cap + 2, Md)
            dh = t_dh[:c_dh.size].cpu().numpy().reshape(cap + 2, Hm)
            assert np.array_equal(F.bits(dh[n_rows:]), F.bits(c_dh.reshape(cap + 2, Hm)[n_rows:])), "rows >= n_rows touched"
            assert np.array_equal(F.bits(dm[n_rows if form != "fused_no_dm" else 0:]), F.bits(c_dm.reshape(cap + 2, Md)[n_rows if form != "fused_no_dm" else 0:]))
            r_dm, r_dh, b_dm, b_dh = mlp_bwd_ref(dgi[:n_rows], hid[:n_rows], W_ih, W2)
            assert np.isfinite(dh[:n_rows]).all()
            assert (dh[:n_rows][hid[:n_rows] == 0] == 0.0).all(), "exactly zero where hid == 0"
            d = np.abs(dh[:n_rows].astype(f64) - r_dh)
            assert (d <= b_dh).all(), ("d_hid", float((d - b_dh).max()))
            if form != "fused_no_dm":
                d = np.abs(dm[:n_rows].astype(f64) - r_dm)
                assert (d <= b_dm).all(), ("d_m", float((d - b_dm).max()))


def test_msg_mlp_bwd_refuses_bad_arguments():
    Pn = 1 << 12
    ok = dict(dgi=Pn, hid=Pn, img_wihT=Pn, img_w2T=Pn, d_m=Pn, d_hid=Pn, D3=24, Hm=14, Md=4, cap_rows=5, n_rows=Pn)
    for change, word in ((dict(d_hid=None), "null argument"), (dict(hid=None), "null argument"), (dict(Md=6), "bad sizes"),
                         (dict(D3=26), "bad sizes"), (dict(cap_rows=0), "bad sizes"), (dict(Md=132), "beyond 128"),
                         (dict(d_m=Pn + 4), "16-byte aligned")):
        f = _lib.MsgMlpBwdDesc(**dict(ok, **change))
        with pytest.raises(_lib.PfoError, match=word):
            _lib.call("pfo_debug_msg_mlp_bwd", C.byref(f), _lib.stream_ptr())


def test_msg_mlp_fwd_beyond_one_column_block_of_messages():
    """msg_dim > 128: the forward kernel's second grid dimension (every column block recomputes layer 1, block 0 stores ``hid``)."""
    D, Ef, Md = 8, 4, 132
    Mr = 3 * D + Ef
    Hm = Mr // 2
    rs = np.random.RandomState(7)
    torch.manual_seed(7)
    l1, l2 = torch.nn.Linear(Mr, Hm), torch.nn.Linear(Hm, Md)
    W1, b1, W2, b2 = (t.detach().numpy().copy() for t in (l1.weight, l1.bias, l2.weight, l2.bias))
    b = F.Bufs()
    cap, n_rows = 129, 128
    raw = (0.05 * G.wide(rs, cap, Mr)).astype(np.float32)
    hm = np.ones(cap, np.uint8); hm[3] = 0
    c_hid, c_out = F.canary((cap + 2) * Hm), F.canary((cap + 2) * Md)
    f = _lib.MsgMlpDesc(raw=b.put(raw, np.float32), ld_raw=Mr, hm=b.put(hm, np.uint8), img_w1=_image(b, W1), img_w2=_image(b, W2),
                        b1=b.put(b1, np.float32), b2=b.put(b2, np.float32), Mr=Mr, Hm=Hm, Md=Md, cap_rows=cap,
                        n_rows=b.put(np.array([n_rows], np.int32), np.int32))
    f.hid = b.put(c_hid, np.float32); t_hid = b.keep[-1]
    f.msg_out = b.put(c_out, np.float32); t_out = b.keep[-1]
    _lib.call("pfo_debug_msg_mlp_fwd", C.byref(f), _lib.stream_ptr())
    torch.cuda.synchronize()
    out = t_out[:c_out.size].cpu().numpy().reshape(cap + 2, Md)
    hid = t_hid[:c_hid.size].cpu().numpy().reshape(cap + 2, Hm)
    assert np.array_equal(F.bits(out[n_rows:]), F.bits(c_out.reshape(cap + 2, Md)[n_rows:]))
    assert np.array_equal(F.bits(hid[n_rows:]), F.bits(c_hid.reshape(cap + 2, Hm)[n_rows:]))
    has = hm[:n_rows] != 0
    r_hid, r_out, b_hid, b_out = mlp_ref(np.where(has[:, None], raw[:n_rows], 0), W1, b1, W2, b2)
    assert (out[:n_rows][~has] == 0).all() and (hid[:n_rows][~has] == 0).all()
    assert (np.abs(out[:n_rows].astype(f64) - r_out)[has] <= b_out[has]).all()
    assert (np.abs(hid[:n_rows].astype(f64) - r_hid)[has] <= b_hid[has]).all()
