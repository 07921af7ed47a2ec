#!/usr/bin/env python3
"""The holdings ledger at the serving shape of DESIGN 4b's whole-call figures: the C2 synthetic graph (L2 K20 D172 H2, memory +
GRU), a model over the first 600 000 interactions whose ledger is seeded from their portfolios (width 8).

(a) the query: ``TGN.recommend(users, now, 10, items, mv=, exclude="held", portfolios="held")`` for 512 users over the 500 items,
    against the route a caller had before the ledger - the same holdings kept as per-user Python lists (item node ids for
    ``exclude``, stock indices for ``portfolios``), packed by ``recommend.validate`` and uploaded with every call; the same query
    otherwise.  One process, one model, the two alternating; host clock around calls that end in a synchronise, 20 calls of
    each after 3 warm-up calls each.  The two routes must return equal outputs: asserted.
(b) the tick: ``TGN.ingest`` of the next 512 interactions with and without ``portfolios=``, in the manner of
    tools/bench_ingest.py: 7 timed runs of each after 1 warm-up, alternating, tables / finder / state restored in between.
Whole-call host-clock figures; median, min and max are printed.  The last line is one JSON object."""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pfotgnrec_amd as P
from pfotgnrec_amd.synthetic import CONFIGS, make_graph

HISTORY, TICK, B, U, K_TOP, WIDTH = 600_000, 512, 512, 512, 10, 8
Q_WARM, Q_REPS, T_WARM, T_REPS = 3, 20, 1, 7
dev = torch.device("cuda:0")
P._lib.require_gpu(dev)


def stats(v):
    v = sorted(v)
    return {"median": round(1e3 * float(np.median(v)), 3), "min": round(1e3 * v[0], 3), "max": round(1e3 * v[-1], 3)}


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    cfg = CONFIGS["C2"]
    g = make_graph(cfg, with_prices=True)
    d = g.data
    n_all = g.node_features.shape[0]
    hist, tick = slice(0, HISTORY), slice(HISTORY, HISTORY + TICK)

    def finder(sl):
        return P.NeighborFinder.from_arrays(d.sources[sl], d.destinations[sl], d.edge_idxs[sl], d.timestamps[sl], uniform=False,
                                            max_node_idx=n_all - 1, device=dev)
    tgn = P.TGN(finder(hist), g.node_features, g.edge_features[:HISTORY + 1], dev, n_layers=2, n_heads=2, dropout=0.1, use_memory=True,
                memory_dimension=cfg.dim, message_function="identity", n_neighbors=cfg.n_neighbors)
    tgn.eval()
    tgn.observe(d.sources[HISTORY - 20 * B:HISTORY], d.destinations[HISTORY - 20 * B:HISTORY], d.timestamps[HISTORY - 20 * B:HISTORY],
                d.edge_idxs[HISTORY - 20 * B:HISTORY], batch_size=B)
    tgn.track_holdings(WIDTH, g.upper_u)
    tgn.update_holdings(d.sources[hist], (g.portfolio_idx[hist], g.portfolio_len[hist]), d.timestamps[hist])
    mv = P.MVSampler(g.prices, g.upper_u, dev, day_of=g.day_of)

    # ---- (a) the query
    rs = np.random.RandomState(1)
    users = rs.choice(np.unique(d.sources[hist]), size=U, replace=False)
    items = np.arange(cfg.n_users + 1, cfg.n_users + cfg.n_items + 1)
    now = float(d.timestamps[HISTORY])
    h_idx, h_len = (t.cpu().numpy() for t in tgn.holdings.rows(users))
    # the caller's own book-keeping before the ledger: one Python list per user, in both id spaces
    port_lists = [[int(s) for s in h_idx[q, :h_len[q]]] for q in range(U)]
    excl_lists = [[s + g.upper_u + 1 for s in row] for row in port_lists]
    routes = (("held", lambda: tgn.recommend(users, now, K_TOP, items, mv=mv, exclude="held", portfolios="held")),
              ("lists", lambda: tgn.recommend(users, now, K_TOP, items, mv=mv, exclude=excl_lists, portfolios=port_lists)))
    out = {}
    for name, fn in routes:
        for _ in range(Q_WARM):
            out[name] = fn()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out["held"], out["lists"])), "the two routes must return equal outputs"
    tq = {"held": [], "lists": []}
    for rep in range(Q_REPS):
        for name, fn in (routes if rep % 2 == 0 else routes[::-1]):
            tq[name].append(timed(fn)[0])

    # ---- (b) the tick
    saved = tgn.memory.backup_memory()
    s_t, d_t, t_t = d.sources[tick], d.destinations[tick], d.timestamps[tick]
    raw_t, ports_t = g.edge_features[d.edge_idxs[tick]], (g.portfolio_idx[tick], g.portfolio_len[tick])
    tgn.reserve(n_edges=HISTORY + 1 + 2 * (T_WARM + T_REPS + 1) * TICK)

    def restore():
        tgn._edges.trim(HISTORY + 1)
        tgn._point_edges()
        tgn.set_neighbor_finder(finder(hist))
        tgn.memory.restore_memory(saved)
    ticks = (("with_portfolios", lambda: tgn.ingest(s_t, d_t, t_t, raw_t, batch_size=B, portfolios=ports_t)),
             ("without", lambda: tgn.ingest(s_t, d_t, t_t, raw_t, batch_size=B)))
    for name, fn in ticks:
        for _ in range(T_WARM):
            restore()
            fn()
    tt = {"with_portfolios": [], "without": []}
    for rep in range(T_REPS):
        for name, fn in (ticks if rep % 2 == 0 else ticks[::-1]):
            restore()
            tt[name].append(timed(fn)[0])
    mh, ml = float(np.median(tq["held"])), float(np.median(tq["lists"]))
    mw, mo = float(np.median(tt["with_portfolios"])), float(np.median(tt["without"]))
    print(json.dumps({"what": "holdings ledger on the C2 graph (600 000 edges of history, L2 K20 D172 H2, memory + GRU), width 8: "
                              "(a) recommend(mv=, exclude='held', portfolios='held') vs per-user Python lists packed and uploaded per "
                              "call, 512 users x 500 items, k = 10; (b) ingest of 512 interactions with and without portfolios=",
                      "clock": "host perf_counter around synchronised whole calls",
                      "query": {"warmup": Q_WARM, "reps": Q_REPS, "held_ms": stats(tq["held"]), "lists_ms": stats(tq["lists"]),
                                "lists_over_held": round(ml / mh, 3), "outputs_equal": True,
                                "held_entries": int(h_len.sum())},
                      "tick": {"warmup": T_WARM, "reps": T_REPS, "with_portfolios_ms": stats(tt["with_portfolios"]),
                               "without_ms": stats(tt["without"]), "added_ms": round(1e3 * (mw - mo), 3)}}), flush=True)


if __name__ == "__main__":
    main()
