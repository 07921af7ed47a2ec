#!/usr/bin/env python3
"""Basket top-k at the serving shape, whole calls: ``TGN.recommend(mv=, basket=True, k=10)`` on the C2 synthetic graph, 512 users
x 500 items, against

* the route a caller has without it: k calls of ``recommend(mv=, k=1)``, each pick appended to the user's portfolio row and
  exclusion row on the device between calls (k embedding passes, k score passes, k host round trips) - outputs asserted equal;
* ``recommend(mv=, k=10)``, the independent list: the price of the feature.

Host clock around a call that ends in a synchronise, the three alternating in one process; median [min, max] of REPS calls after
WARM warm-up calls.  Work the rounds add per user over the independent list: 2 (k - 1) I^2 comparisons less the
place count's I^2, and (k - 1) I n_ret multiply-adds."""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pfotgnrec_amd as P
from pfotgnrec_amd.synthetic import CONFIGS, make_graph

WARM, REPS = 2, 10
U, K_TOP, W = 512, 10, 8
dev = torch.device("cuda:0")
P._lib.require_gpu(dev)


def stats(v, scale=1e3, nd=3):
    v = sorted(v)
    return {"median": round(scale * float(np.median(v)), nd), "min": round(scale * v[0], nd), "max": round(scale * v[-1], nd)}


def main():
    torch.manual_seed(0)
    cfg = CONFIGS["C2"]
    g = make_graph(cfg, with_prices=True)
    d = g.data
    D = cfg.dim
    tgn = P.TGN(P.get_neighbor_finder(d, False), g.node_features, g.edge_features, dev, n_layers=2, n_heads=2, dropout=0.1,
                use_memory=True, memory_dimension=D, message_function="identity")
    with torch.no_grad():
        tgn.memory.msg_table.normal_(0, 0.1); tgn.memory.memory.normal_(0, 0.1); tgn.memory.has_msg.fill_(1)
    mv = P.MVSampler(g.prices, g.upper_u, dev, day_of=g.day_of)
    rs = np.random.RandomState(1)
    users = torch.from_numpy(rs.choice(np.arange(1, cfg.n_users + 1), size=U, replace=False)).to(dev)
    items = torch.from_numpy(np.arange(cfg.n_users + 1, cfg.n_users + cfg.n_items + 1)).to(dev)
    rows = rs.randint(0, len(d.sources), size=U)
    now = float(d.timestamps[900000])
    day = int(g.day_of(np.array([now]))[0])
    # device rows with K_TOP free slots behind the holdings: the loop appends its picks in place
    port = torch.full((U, W + K_TOP), -1, dtype=torch.int32, device=dev)
    port[:, :W] = torch.from_numpy(g.portfolio_idx[rows].astype(np.int32)).to(dev)
    plen = torch.from_numpy(g.portfolio_len[rows].astype(np.int32)).to(dev)
    held_ids = torch.where(port >= 0, port + (cfg.n_users + 1), torch.full_like(port, -1))
    ar = torch.arange(U, device=dev)

    def basket():
        return tgn.recommend(users, now, K_TOP, items, exclude=(held_ids, plen), mv=mv, portfolios=(port, plen), day_idx=day, basket=True)

    def independent():
        return tgn.recommend(users, now, K_TOP, items, exclude=(held_ids, plen), mv=mv, portfolios=(port, plen), day_idx=day)

    def loop():
        p, e, n = port.clone(), held_ids.clone(), plen.clone()
        ids = torch.full((U, K_TOP), -1, dtype=torch.int32, device=dev)
        scores = torch.full((U, K_TOP), float("-inf"), dtype=torch.float32, device=dev)
        fused = torch.full((U, K_TOP), float("-inf"), dtype=torch.float64, device=dev)
        n_valid = torch.zeros(U, dtype=torch.int32, device=dev)
        for r in range(K_TOP):
            one = tgn.recommend(users, now, 1, items, exclude=(e, n), mv=mv, portfolios=(p, n), day_idx=day)
            got = (one[2] == 1) & (n_valid == r)
            ids[:, r] = torch.where(got, one[0][:, 0], ids[:, r])
            scores[:, r] = torch.where(got, one[1][:, 0], scores[:, r])
            fused[:, r] = torch.where(got, one[3][:, 0], fused[:, r])
            n_valid += got.int()
            at = n.long().clamp(max=W + K_TOP - 1)
            p[ar, at] = torch.where(got, one[0][:, 0] - (cfg.n_users + 1), p[ar, at])
            e[ar, at] = torch.where(got, one[0][:, 0], e[ar, at])
            n += got.int()
        return ids, scores, n_valid, fused

    fns = (("basket", basket), ("loop_of_k_calls", loop), ("independent_k", independent))
    for _ in range(WARM):
        for _, fn in fns:
            fn()
    ts = {name: [] for name, _ in fns}
    for rep in range(REPS):
        for name, fn in (fns if rep % 2 == 0 else fns[::-1]):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); ts[name].append(time.perf_counter() - t0)
    a, b, c = basket(), loop(), independent()
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "the basket call and the loop of k calls disagree"
    assert torch.equal(a[0][:, 0], c[0][:, 0])
    print(json.dumps({"what": "whole TGN.recommend call, C2 graph, L2 K20 D172 H2 memory+GRU, mv", "U": U, "I": cfg.n_items, "k": K_TOP,
                      "W": W, "n_ret": int(mv.returns.shape[2]), "warmup": WARM, "reps": REPS,
                      **{"ms_" + name: stats(v) for name, v in ts.items()},
                      "loop_over_basket": round(float(np.median(ts["loop_of_k_calls"]) / np.median(ts["basket"])), 2),
                      "basket_over_independent": round(float(np.median(ts["basket"]) / np.median(ts["independent_k"])), 2),
                      "basket_equals_loop": True,
                      "users_whose_list_differs_from_independent": int((a[0] != c[0]).any(1).sum())}), flush=True)


if __name__ == "__main__":
    main()
