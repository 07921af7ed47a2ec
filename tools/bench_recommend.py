#!/usr/bin/env python3
"""Read-only top-k recommendation at the serving shape.

1. ``pfo_recommend_topk`` alone at U = 50 000 (the C2 user count) and U = 512: I = 500 candidates, D = 172, k = 10, one block,
   portfolios of 0..7 excluded positions.  Beside it, in the same process on the same tensors, what a caller could do without
   the kernel: ``(ue @ ie.T)``, ``masked_fill_`` of the skip mask with -inf, ``torch.topk(k)`` (the mask itself is built ahead
   of the timed window).  Device events around every call, the two alternating; median and the spread of REPS calls
   after WARM warm-up calls.
2. The whole ``TGN.recommend`` call on the C2 synthetic graph at U = 512 (host clock around a call that ends in a synchronise).

Work of the kernel: 2 U I D FLOP, U D 4 + n_t I D 4 bytes read, U k 8 bytes written."""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pfotgnrec_amd as P
from pfotgnrec_amd.synthetic import CONFIGS, make_graph

WARM, REPS = 5, 30
I, D, K_TOP = 500, 172, 10
dev = torch.device("cuda:0")
P._lib.require_gpu(dev)


def stats(v, scale=1e3, nd=1):
    v = sorted(v)
    return {"median": round(scale * float(np.median(v)), nd), "min": round(scale * v[0], nd), "max": round(scale * v[-1], nd)}


def event_timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); out = fn(); b.record()
    return a, b, out


def kernel_alone(U):
    rs = np.random.RandomState(U)
    ue = torch.from_numpy(rs.randn(U, D).astype(np.float32)).to(dev)
    ie = torch.from_numpy(rs.randn(I, D).astype(np.float32)).to(dev)
    plen = rs.randint(0, 8, size=U).astype(np.int32)
    ppos = rs.randint(0, I, size=(U, 8)).astype(np.int32)
    ppos[np.arange(8)[None, :] >= plen[:, None]] = -1
    excl_pos, excl_len = torch.from_numpy(ppos).to(dev), torch.from_numpy(plen).to(dev)
    mask = torch.zeros((U, I), dtype=torch.bool, device=dev)
    rows = torch.arange(U, device=dev)[:, None].expand(U, 8)[excl_pos >= 0]
    mask[rows, excl_pos[excl_pos >= 0].long()] = True

    def ours():
        return P.recommend_topk(ue, ie, K_TOP, None, excl_pos, excl_len)

    def composed():
        s = ue @ ie.T
        s.masked_fill_(mask, float("-inf"))
        return torch.topk(s, K_TOP)

    for _ in range(WARM):
        ours(); composed()
    ev = {"ours": [], "composed": []}
    for rep in range(REPS):
        order = (("ours", ours), ("composed", composed))
        for name, fn in (order if rep % 2 == 0 else order[::-1]):
            ev[name].append(event_timed(fn)[:2])
    torch.cuda.synchronize()
    ms = {name: [a.elapsed_time(b) for a, b in v] for name, v in ev.items()}
    pos, score, _ = ours()
    tv, ti = composed()
    same = (pos.long().sort(1).values == ti.sort(1).values).all(1).float().mean().item()
    med = float(np.median(ms["ours"])) * 1e-3
    flop = 2.0 * U * I * D
    return {"what": "pfo_recommend_topk alone vs matmul + masked_fill_ + topk", "U": U, "I": I, "D": D, "k": K_TOP, "n_t": 1,
            "portfolio": "0..7 excluded positions per user", "warmup": WARM, "reps": REPS,
            "kernel_us": stats(ms["ours"]), "torch_composition_us": stats(ms["composed"]),
            "kernel_TFLOPs": round(flop / med / 1e12, 2),
            "bytes_needed": U * D * 4 + I * D * 4 + U * K_TOP * 8,
            "users_with_the_same_id_set_as_torch": round(same, 5),
            "max_abs_score_difference": float((score - tv).abs().max())}


def whole_call(U=512):
    cfg = CONFIGS["C2"]
    g = make_graph(cfg, with_prices=False)
    d = g.data
    tgn = P.TGN(P.get_neighbor_finder(d, False), g.node_features, g.edge_features, dev, n_layers=2, n_heads=2, dropout=0.1,
                use_memory=True, memory_dimension=D, message_function="identity")
    with torch.no_grad():
        tgn.memory.msg_table.normal_(0, 0.1); tgn.memory.memory.normal_(0, 0.1); tgn.memory.has_msg.fill_(1)
    rs = np.random.RandomState(1)
    users = rs.choice(np.arange(1, cfg.n_users + 1), size=U, replace=False)
    items = np.arange(cfg.n_users + 1, cfg.n_users + cfg.n_items + 1)
    rows = rs.randint(0, len(d.sources), size=U)
    packed = np.where(g.portfolio_idx[rows] >= 0, g.portfolio_idx[rows] + cfg.n_users + 1, -1).astype(np.int32)
    lens = g.portfolio_len[rows].astype(np.int32)
    now = float(d.timestamps[900000])
    users_d, items_d = torch.from_numpy(users).to(dev), torch.from_numpy(items).to(dev)
    excl = (torch.from_numpy(packed).to(dev), torch.from_numpy(lens).to(dev))
    out = {}
    for name, args in (("numpy_arguments", (users, now, K_TOP, items, (packed, lens))),
                       ("device_arguments", (users_d, now, K_TOP, items_d, excl))):
        for _ in range(3):
            tgn.recommend(*args)
        ts = []
        for _ in range(20):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            tgn.recommend(*args)
            torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        out["ms_" + name] = stats(ts, 1e3, 3)
    return {"what": "whole TGN.recommend call, C2 graph, L2 K20 D172 H2 memory+GRU", "U": U, "I": cfg.n_items, "k": K_TOP,
            "roots_embedded": U + cfg.n_items, "warmup": 3, "reps": 20, **out}


if __name__ == "__main__":
    for U in (50000, 512):
        print(json.dumps(kernel_alone(U)), flush=True)
    if "--kernel-only" not in sys.argv:
        print(json.dumps(whole_call()), flush=True)
