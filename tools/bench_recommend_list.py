#!/usr/bin/env python3
"""The list forms of the top-k recommendation against what a caller had before them.

1. ``pfo_recommend_list_topk`` alone at U = 512 and 50 000, I = 500 and 5 000, lists of W = 8 and 64 positions, D = 172, k = 10,
   one block.  Beside it, in the same process on the same tensors, the two routes to the same answer:
     exclusion   ``pfo_recommend_topk`` with the complement of each list as the exclusion list (built ahead of the timed window);
     composed    torch: gather of the listed rows, ``bmm``, ``masked_fill_`` of the slots that do not count with -inf, ``topk``
                 (the mask - padding and repeats - is built ahead of the timed window).
   Device events around every call, the routes alternating; median and the spread of REPS calls after WARM warm-up calls (a
   route whose call takes longer than SLOW_MS gets SLOW_REPS).  Asserted: the same n_valid from the two kernels, and on
   integer embeddings (every fp32 dot product exact in any order) the same positions and scores to the bit.
2. The whole ``TGN.recommend(only="held")`` call beside ``recommend(exclude="held")`` on the C2 synthetic graph at U = 512 (host
   clock around a call that ends in a synchronise).

Work of the list kernel: 2 U W D FLOP; U D 4 + U W D 4 bytes read (the gathered rows, from L2 where they repeat),
U k 8 bytes written."""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pfotgnrec_amd as P
from pfotgnrec_amd.synthetic import CONFIGS, make_graph

WARM, REPS, SLOW_MS, SLOW_REPS = 3, 20, 20.0, 5
D, K_TOP = 172, 10
dev = torch.device("cuda:0")
P._lib.require_gpu(dev)


def stats(v, scale=1e3, nd=1):
    v = sorted(v)
    return {"median": round(scale * float(np.median(v)), nd), "min": round(scale * v[0], nd), "max": round(scale * v[-1], nd)}


def event_timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); out = fn(); b.record()
    return a, b, out


def routes(U, I, W, integer=False):
    """The tensors of one shape and the three routes over them."""
    g = torch.Generator(device=dev).manual_seed(1000 * W + I + U)
    if integer:
        ue = torch.randint(-3, 4, (U, D), generator=g, device=dev).float()
        ie = torch.randint(-3, 4, (I, D), generator=g, device=dev).float()
    else:
        ue = torch.randn((U, D), generator=g, device=dev)
        ie = torch.randn((I, D), generator=g, device=dev)
    list_pos = torch.randint(0, I, (U, W), generator=g, device=dev, dtype=torch.int32)      # repeats among them
    list_len = torch.randint(W // 2, W + 1, (U,), generator=g, device=dev, dtype=torch.int32)
    counted = torch.arange(W, device=dev)[None, :] < list_len[:, None]
    list_pos = torch.where(counted, list_pos, torch.full_like(list_pos, -1))
    # the complement as an exclusion list: the positions nobody named, in front of a row of I
    named = torch.zeros((U, I), dtype=torch.bool, device=dev)
    rows = torch.arange(U, device=dev)[:, None].expand(U, W)[counted]
    named[rows, list_pos[counted].long()] = True
    excl_pos = torch.empty((U, I), dtype=torch.int32, device=dev)
    for u0 in range(0, U, 4096):
        excl_pos[u0:u0 + 4096] = torch.argsort(named[u0:u0 + 4096].to(torch.int8), dim=1, stable=True).to(torch.int32)
    excl_len = (I - named.sum(1)).to(torch.int32)
    # the slots of a list that do not count for the composition: padding, and every repeat of an earlier slot
    lp = list_pos.long()
    repeat = ((lp[:, :, None] == lp[:, None, :]) & (torch.arange(W, device=dev)[None, :] < torch.arange(W, device=dev)[:, None])[None]).any(2)
    dead = ~counted | repeat
    safe = lp.clamp(min=0)
    kk = min(K_TOP, W)
    del named

    def listed():
        return P.recommend_list_topk(ue, ie, K_TOP, list_pos, list_len)

    def exclusion():
        return P.recommend_topk(ue, ie, K_TOP, None, excl_pos, excl_len)

    def composed():
        s = torch.bmm(ie[safe], ue[:, :, None]).squeeze(2)
        s.masked_fill_(dead, float("-inf"))
        return torch.topk(s, kk)

    return dict(listed=listed, exclusion=exclusion, composed=composed), safe


def kernel_alone(U, I, W):
    fns, safe = routes(U, I, W)
    reps = {}
    for name, fn in fns.items():
        for _ in range(WARM):
            fn()
        a, b, _ = event_timed(fn)
        torch.cuda.synchronize()
        reps[name] = SLOW_REPS if a.elapsed_time(b) > SLOW_MS else REPS
    ev = {name: [] for name in fns}
    for rep in range(REPS):
        order = list(fns.items())
        for name, fn in (order if rep % 2 == 0 else order[::-1]):
            if rep < reps[name]:
                ev[name].append(event_timed(fn)[:2])
    torch.cuda.synchronize()
    ms = {name: [a.elapsed_time(b) for a, b in v] for name, v in ev.items()}
    pos, score, n = fns["listed"]()
    xpos, xscore, xn = fns["exclusion"]()
    tv, ti = fns["composed"]()
    assert torch.equal(n, xn), "the two kernels count the same admissible candidates"
    tpos = torch.where(torch.isinf(tv), torch.full_like(ti, -1), safe.gather(1, ti))
    kk = tpos.shape[1]
    med = float(np.median(ms["listed"])) * 1e-3
    both = (pos == xpos) & (pos >= 0)
    return {"what": "pfo_recommend_list_topk alone vs pfo_recommend_topk over the complement vs gather + bmm + masked_fill_ + topk",
            "U": U, "I": I, "W": W, "D": D, "k": K_TOP, "n_t": 1, "list": "W/2..W counted entries per user, repeats among them",
            "warmup": WARM, "reps": reps, "list_kernel_us": stats(ms["listed"]), "exclusion_route_us": stats(ms["exclusion"]),
            "torch_composition_us": stats(ms["composed"]),
            "list_kernel_GFLOPs": round(2.0 * U * W * D / med / 1e9, 1), "gathered_bytes": U * W * D * 4,
            "users_with_the_exclusion_routes_positions": round((pos == xpos).all(1).float().mean().item(), 5),
            "users_with_the_compositions_id_set": round((pos[:, :kk].sort(1).values == tpos.int().sort(1).values).all(1).float().mean().item(), 5),
            "max_abs_score_difference_to_the_exclusion_route": float((score - xscore)[both].abs().max()) if both.any() else None}


def exact_agreement(U=512, I=500, W=64):
    fns, _ = routes(U, I, W, integer=True)
    a, b = fns["listed"](), fns["exclusion"]()
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "exact arithmetic: the two kernels agree to the bit"
    return {"what": "integer embeddings: list kernel == exclusion route, bit for bit", "U": U, "I": I, "W": W, "ok": True}


def whole_call(U=512, width=8):
    cfg = CONFIGS["C2"]
    g = make_graph(cfg, with_prices=False)
    d = g.data
    tgn = P.TGN(P.get_neighbor_finder(d, False), g.node_features, g.edge_features, dev, n_layers=2, n_heads=2, dropout=0.1,
                use_memory=True, memory_dimension=D, message_function="identity")
    with torch.no_grad():
        tgn.memory.msg_table.normal_(0, 0.1); tgn.memory.memory.normal_(0, 0.1); tgn.memory.has_msg.fill_(1)
    tgn.track_holdings(width, cfg.n_users)
    tgn.update_holdings(d.sources, (g.portfolio_idx[:, :width], np.minimum(g.portfolio_len, width)), d.timestamps)
    rs = np.random.RandomState(1)
    users = torch.from_numpy(rs.choice(np.unique(d.sources), size=U, replace=False)).to(dev)
    items = torch.from_numpy(np.arange(cfg.n_users + 1, cfg.n_users + cfg.n_items + 1)).to(dev)
    now = float(d.timestamps[900000])
    out = {}
    for name, kw in (("only_held", dict(only="held")), ("exclude_held", dict(exclude="held"))):
        for _ in range(3):
            tgn.recommend(users, now, K_TOP, items, **kw)
        ts = []
        for _ in range(20):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            tgn.recommend(users, now, K_TOP, items, **kw)
            torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        out["ms_" + name] = stats(ts, 1e3, 3)
    return {"what": "whole TGN.recommend call, C2 graph, L2 K20 D172 H2 memory+GRU, device arguments", "U": U, "I": cfg.n_items,
            "k": K_TOP, "ledger_width": width, "roots_embedded": U + cfg.n_items, "warmup": 3, "reps": 20, **out}


if __name__ == "__main__":
    print(json.dumps(exact_agreement()), flush=True)
    for U in (512, 50000):
        for I in (500, 5000):
            for W in (8, 64):
                print(json.dumps(kernel_alone(U, I, W)), flush=True)
                torch.cuda.empty_cache()
    if "--kernel-only" not in sys.argv:
        print(json.dumps(whole_call()), flush=True)
