#!/usr/bin/env python3
"""The training step with the identity message function against the same step with the MLP message function.

On the C2 synthetic graph (L2 K20 D172 H2 Ef4, memory + GRU, batch 512, 3 negatives) two models take the same STEPS batches
from the same saved state (memory, last_update, pending messages restored in front of every repetition; parameters move with
Adam as in training):
  identity : the GRU contracts the touched rows' raw messages, K = 3D+Ef = 520;
  mlp      : Linear(520, 260) -> ReLU -> Linear(260, 100) over the touched rows (two image contractions, the hidden rows
             through HBM), the GRU with K = 100; backward d m = dgi W_ih, d hid = (d m W2) (hid > 0), and two more problems in
             the GRU's grouped weight-gradient launch.
Per touched row the MLP path adds 2 (520 260 + 260 100) = 322 kFLOP forward and 2 (516 100 + 100 260) = 155 kFLOP of data
backward + 2 (260 520 + 100 260) = 322 kFLOP of weight gradients, and writes + reads hidden (260) and message (100) rows:
2.9 KB forward; the GRU's input contraction drops from 2 516 520 = 537 kFLOP to 2 516 100 = 103 kFLOP (and its dW_ih alike).
``train`` = embed_device + bpr_loss + backward + FusedAdam.step per batch; ``forward`` = eval-mode embed_device under no_grad.
Host clock (``time.perf_counter``) around a window that starts and ends in a device synchronise; WARM warm-up windows of each,
then REPS timed windows, the two models alternating and the order swapped every repetition; median, min and max are printed,
and the touched rows per step (the MLP's row count) read back outside the timed windows.  One JSON line.
Then ``kernels()`` (alone with ``--kernels-only``): the fused forward / data-backward kernels against the composed contractions
on the same rows, through the probes; a second JSON line."""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pfotgnrec_amd as P
from pfotgnrec_amd.synthetic import CONFIGS, make_graph

WARM, REPS = 2, 7
STEPS, B, START, NEG = 40, 512, 600_000, 3
dev = torch.device("cuda:0")
P._lib.require_gpu(dev)


def stats(v, per):
    v = sorted(x / per for x in v)
    return {"median": round(1e3 * float(np.median(v)), 4), "min": round(1e3 * v[0], 4), "max": round(1e3 * v[-1], 4)}


def main():
    cfg = CONFIGS["C2"]
    g = make_graph(cfg, with_prices=False, with_portfolios=False)
    d = g.data
    K = cfg.n_neighbors
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    n = STEPS * B
    lo = START - 20 * B
    src, dst = to(d.sources[lo:START + n], np.int32), to(d.destinations[lo:START + n], np.int32)
    ts, eidx = to(d.timestamps[lo:START + n], np.float64), to(d.edge_idxs[lo:START + n], np.int32)
    neg = to(np.random.RandomState(0).randint(cfg.n_users + 1, cfg.n_users + cfg.n_items + 1, size=(20 + STEPS) * B * NEG), np.int32)
    models = {}
    for name in ("identity", "mlp"):
        torch.manual_seed(1)
        tgn = P.TGN(P.get_neighbor_finder(d, False), g.node_features, g.edge_features, dev, n_layers=cfg.n_layers, n_heads=2, dropout=0.1,
                    use_memory=True, memory_dimension=cfg.dim, message_function=name, message_dimension=100, n_neighbors=K)
        opt = P.FusedAdam(tgn, lr=1e-4)
        models[name] = (tgn, opt)

    def batch(i):                                                   # i = -20 .. STEPS - 1
        k = (20 + i) * B
        return src[k:k + B], dst[k:k + B], [neg[k * NEG:(k + B) * NEG]], [NEG], ts[k:k + B], eidx[k:k + B], K

    def train(name):
        tgn, opt = models[name]
        tgn.train()
        for i in range(STEPS):
            emb, b = tgn.embed_device(*batch(i))
            P.bpr_loss(emb, b, NEG).backward()
            opt.step()
            opt.zero_grad(set_to_none=True)

    def forward(name):
        tgn, _ = models[name]
        tgn.eval()
        with torch.no_grad():
            for i in range(STEPS):
                tgn.embed_device(*batch(i))

    saved, touched = {}, {}
    for name, (tgn, _) in models.items():                          # a populated state to start from, then saved
        tgn.eval()
        with torch.no_grad():
            for i in range(-20, 0):
                tgn.embed_device(*batch(i))
            saved[name] = tgn.memory.backup_memory()
            tgn.embed_device(*batch(0))
            touched[name] = int(tgn.debug_touched()[0].shape[0])
    out = {}
    for what, fn in (("train", train), ("forward", forward)):
        for name in models:
            for _ in range(WARM):
                models[name][0].memory.restore_memory(saved[name])
                fn(name)
        torch.cuda.synchronize()
        t = {name: [] for name in models}
        order = list(models)
        for rep in range(REPS):
            for name in (order if rep % 2 == 0 else order[::-1]):
                tgn = models[name][0]
                tgn.memory.restore_memory(saved[name])
                tgn.join()
                torch.cuda.synchronize(); t0 = time.perf_counter()
                fn(name)
                tgn.join()
                torch.cuda.synchronize(); t[name].append(time.perf_counter() - t0)
        out[what] = {name: stats(t[name], STEPS) for name in models}
        out[what]["mlp_over_identity"] = round(float(np.median(t["mlp"]) / np.median(t["identity"])), 4)
    print(json.dumps({"what": "C2 graph (L2 K20 D172 H2), batch 512, 3 negatives: ms per step, identity vs mlp message function (message_dimension 100)",
                      "clock": "host perf_counter around synchronised windows of %d steps" % STEPS, "warmup": WARM, "reps": REPS,
                      "touched_rows_first_step": touched, "ms_per_step": out}), flush=True)


def kernels():
    """(b), (c): the fused kernels against the composed contractions on the same rows, through the probes, at the C2 shapes
    (raw 520, hidden 260, message 100, dgi 516).  Device events around LOOP back-to-back launches, REPS rounds, the two forms
    alternating and the order swapped every round; us per call, median (min - max).  Outputs are compared before timing."""
    import ctypes as C
    from pfotgnrec_amd import _lib
    Mr, Hm, Md, D3 = 520, 260, 100, 516
    LOOP = 100
    rs = np.random.RandomState(0)
    keep = []

    def put(a, dt=np.float32):
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev); keep.append(t); return t

    def image(W, trans):
        N, K = (W.shape[1], W.shape[0]) if trans else W.shape
        dst = torch.zeros(_lib.byte_count("pfo_debug_bimg_bytes", N, K) + 256, dtype=torch.uint8, device=dev); keep.append(dst)
        d = _lib.BimgDesc(src=put(W).data_ptr(), ld=W.shape[1], N=N, K=K, trans=int(trans), dst=dst.data_ptr())
        _lib.call("pfo_debug_bimg", C.byref(d), 1, _lib.stream_ptr())
        return dst.data_ptr()

    def gemm(**kw):
        d = _lib.GemmDesc(batch=1, rs_ld=1)
        for k, v in kw.items():
            if k in ("A", "lda", "a_idx", "B", "ldb", "K"):
                getattr(d, k)[0] = v
            else:
                setattr(d, k, v)
        return d
    lin = lambda o, i: (rs.randn(o, i) / np.sqrt(i)).astype(np.float32)
    W1, W2, W_ih = lin(Hm, Mr), lin(Md, Hm), lin(D3, Md)
    b1, b2 = put(0.1 * rs.randn(Hm)), put(0.1 * rs.randn(Md))
    tW1, tW2, tWih = put(W1), put(W2), put(W_ih)
    i1, i2, iA, iB = image(W1, 0), image(W2, 0), image(W_ih, 1), image(W2, 1)
    out = {}
    for rows in (128, 1024, 10020):
        nodes = 5 * rows
        touched = put(rs.permutation(nodes)[:rows], np.int32)
        raw, hm = put(rs.randn(nodes, Mr)), put(np.ones(nodes), np.uint8)
        n = put(np.array([rows]), np.int32)
        hid_f, out_f, hid_c, out_c = (torch.zeros(rows, w, device=dev) for w in (Hm, Md, Hm, Md))
        dgi = put(rs.randn(rows, D3))
        dm_f, dh_f, dm_c, dh_c = (torch.zeros(rows, w, device=dev) for w in (Md, Hm, Md, Hm))
        fw = _lib.MsgMlpDesc(raw=raw.data_ptr(), ld_raw=Mr, touched=touched.data_ptr(), hm=hm.data_ptr(), img_w1=i1, img_w2=i2, b1=b1.data_ptr(),
                             b2=b2.data_ptr(), hid=hid_f.data_ptr(), msg_out=out_f.data_ptr(), Mr=Mr, Hm=Hm, Md=Md, cap_rows=rows, n_rows=n.data_ptr())
        fw0 = _lib.MsgMlpDesc.from_buffer_copy(fw); fw0.hid = None
        g1 = gemm(A=raw.data_ptr(), lda=Mr, a_idx=touched.data_ptr(), B=tW1.data_ptr(), ldb=Mr, K=Mr, C=hid_c.data_ptr(), ldc=Hm, M=rows, N=Hm,
                  bias=b1.data_ptr(), relu=1, m_dev=n.data_ptr(), b_img=i1)
        g2 = gemm(A=hid_c.data_ptr(), lda=Hm, B=tW2.data_ptr(), ldb=Hm, K=Hm, C=out_c.data_ptr(), ldc=Md, M=rows, N=Md, bias=b2.data_ptr(),
                  m_dev=n.data_ptr(), b_img=i2)
        bw = _lib.MsgMlpBwdDesc(dgi=dgi.data_ptr(), hid=hid_c.data_ptr(), img_wihT=iA, img_w2T=iB, d_m=dm_f.data_ptr(), d_hid=dh_f.data_ptr(),
                                D3=D3, Hm=Hm, Md=Md, cap_rows=rows, n_rows=n.data_ptr())
        q1 = gemm(A=dgi.data_ptr(), lda=D3, B=tWih.data_ptr(), ldb=Md, K=D3, C=dm_c.data_ptr(), ldc=Md, M=rows, N=Md, b_kmajor=1,
                  m_dev=n.data_ptr(), b_img=iA)
        q2 = gemm(A=dm_c.data_ptr(), lda=Md, B=tW2.data_ptr(), ldb=Hm, K=Md, C=dh_c.data_ptr(), ldc=Hm, M=rows, N=Hm, b_kmajor=1,
                  m_dev=n.data_ptr(), b_img=iB, relu_src=hid_c.data_ptr(), relu_ld=Hm)
        sp = _lib.stream_ptr()
        forms = {"fwd_fused": lambda: _lib.call("pfo_debug_msg_mlp_fwd", C.byref(fw), sp),
                 "fwd_fused_no_hid": lambda: _lib.call("pfo_debug_msg_mlp_fwd", C.byref(fw0), sp),
                 "fwd_composed": lambda: (_lib.call("pfo_debug_gemm", C.byref(g1), sp), _lib.call("pfo_debug_gemm", C.byref(g2), sp)),
                 "bwd_fused": lambda: _lib.call("pfo_debug_msg_mlp_bwd", C.byref(bw), sp),
                 "bwd_composed": lambda: (_lib.call("pfo_debug_gemm", C.byref(q1), sp), _lib.call("pfo_debug_gemm", C.byref(q2), sp))}
        for f in forms.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
        agree = {"msg_out": rel(out_f, out_c), "hid": rel(hid_f, hid_c), "d_m": rel(dm_f, dm_c), "d_hid": rel(dh_f, dh_c)}
        assert max(agree.values()) < 1e-5, agree
        t = {k: [] for k in forms}
        order = list(forms)
        for rep in range(REPS):
            for k in (order if rep % 2 == 0 else order[::-1]):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(LOOP):
                    forms[k]()
                e1.record(); e1.synchronize()
                t[k].append(e0.elapsed_time(e1) / LOOP)
        us = lambda v: {"median": round(1e3 * float(np.median(v)), 2), "min": round(1e3 * min(v), 2), "max": round(1e3 * max(v), 2)}
        out[rows] = dict({k: us(v) for k, v in t.items()}, fused_vs_composed_max_relative_difference=agree)
    print(json.dumps({"what": "MLP message function, C2 shapes (raw 520, hidden 260, message 100): fused kernels against the composed contractions, us per call",
                      "clock": "device events around %d back-to-back calls" % LOOP, "reps": REPS, "rows": out}), flush=True)


if __name__ == "__main__":
    if "--kernels-only" not in sys.argv:
        main()
    kernels()
