#!/usr/bin/env python3
"""What scoring the served lists costs, on the C2 synthetic graph: 512 users x 500 items, k = 10, cutoffs (1, 3, 5, 10),
portfolios of width 8, n_ret = 29, a ``PriceLedger`` as the tables (horizon 3).

* device-event time of ``pfo_list_metrics`` alone next to the ``TGN.recommend`` call it follows;
* whole-call host clock (the call ends in a synchronise) of one ``backtest`` batch against ``recommend`` + ``observe`` of the same
  batch without the scoring.

Median [min, max] of REPS calls after WARM warm-up calls, the routes alternating in one process."""
import importlib, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pfotgnrec_amd as P
from pfotgnrec_amd.synthetic import CONFIGS, make_graph

WARM, REPS = 5, 30
U, K_TOP, W, CUTS, HORIZON, FIRST = 512, 10, 8, (1, 3, 5, 10), 3, 900000
dev = torch.device("cuda:0")
P._lib.require_gpu(dev)


def stats(v, scale=1e3, nd=3):
    v = sorted(v)
    return {"median": round(scale * float(np.median(v)), nd), "min": round(scale * v[0], nd), "max": round(scale * v[-1], nd)}


def event_timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); out = fn(); b.record(); b.synchronize()
    return a.elapsed_time(b) * 1e-3, out


def host_timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    torch.manual_seed(0)
    cfg = CONFIGS["C2"]
    g = make_graph(cfg, with_prices=True)
    d = g.data
    tgn = P.TGN(P.get_neighbor_finder(d, False), g.node_features, g.edge_features, dev, n_layers=2, n_heads=2, dropout=0.1,
                use_memory=True, memory_dimension=cfg.dim, message_function="identity")
    tgn.eval()
    with torch.no_grad():
        tgn.memory.msg_table.normal_(0, 0.1); tgn.memory.memory.normal_(0, 0.1); tgn.memory.has_msg.fill_(1)
    ledger = P.PriceLedger.from_prices(np.arange(cfg.n_days), g.prices, g.upper_u, dev, key_divisor=float((1 << 24) // cfg.n_days))
    sl = slice(FIRST, FIRST + U)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    src, dst, eidx = i32(d.sources[sl]), i32(d.destinations[sl]), i32(d.edge_idxs[sl])
    ts = torch.from_numpy(d.timestamps[sl].astype(np.float64)).to(dev)
    items = np.arange(cfg.n_users + 1, cfg.n_users + cfg.n_items + 1)
    port = (i32(g.portfolio_idx[sl][:, :W]), i32(g.portfolio_len[sl]))
    bt = importlib.import_module("pfotgnrec_amd.backtest")     # (the package attribute of that name is the function)
    day_p, day_f = bt.ledger_days(ledger, ts, HORIZON, dev)

    def recommend():
        return tgn.recommend(src, ts, K_TOP, items)

    lists = recommend()

    def score():
        return P.list_metrics(lists[0], dst, CUTS, port[0], port[1], g.upper_u, ledger.returns, day_p, ledger.returns, day_f, lists[2])

    def observe():
        tgn.observe(src, dst, ts, eidx, batch_size=None)

    def plain():
        recommend(); observe()

    def backtest():
        P.backtest_rows(tgn, src, dst, ts, eidx, items, K_TOP, cutoffs=CUTS, batch_size=U, tables=ledger, horizon=HORIZON, portfolios=port)

    routes = (("ms_device_list_metrics", lambda: event_timed(score)[0]), ("ms_device_recommend", lambda: event_timed(recommend)[0]),
              ("ms_host_backtest_batch", lambda: host_timed(backtest)), ("ms_host_recommend_observe", lambda: host_timed(plain)))
    for _ in range(WARM):
        for _, fn in routes:
            fn()
    t = {name: [] for name, _ in routes}
    for rep in range(REPS):
        for name, fn in (routes if rep % 2 == 0 else routes[::-1]):
            t[name].append(fn())
    med = {k: float(np.median(v)) for k, v in t.items()}
    print(json.dumps({"what": "backtest scoring, C2 graph, L2 K20 D172 H2 memory+GRU, score order, PriceLedger tables", "U": U,
                      "I": cfg.n_items, "k": K_TOP, "cutoffs": CUTS, "W": W, "n_ret": ledger.n_ret, "warmup": WARM, "reps": REPS,
                      **{k: stats(v) for k, v in t.items()},
                      "list_metrics_over_recommend_device": round(med["ms_device_list_metrics"] / med["ms_device_recommend"], 5),
                      "backtest_over_recommend_observe_host": round(med["ms_host_backtest_batch"] / med["ms_host_recommend_observe"], 3)}),
          flush=True)


if __name__ == "__main__":
    main()
