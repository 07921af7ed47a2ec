#!/usr/bin/env python3
"""The history gather on the C2 synthetic graph (50 000 users, 500 items, 1 000 000 interactions; L2 K20 D172 H2,
memory + GRU): a model over the first 600 000 interactions, its finder built on the device.

(a) the gather alone: ``functional.history_gather`` over the finder's device CSR for U = 512 and 50 000 users (drawn with
    replacement from the sources of the history, all at the time of the next interaction), W = 8 / 64 / 256, with and without
    ``count_out``.
(b) the whole query: ``TGN.recommend(users, now, 10, items, exclude="seen")`` for 512 and for 50 000 users (distinct sources of the
    history; all of them where there are fewer) over the 500 items against the route
    it replaces, written against the surface the model had before: every user's row of the finder's HOST mirrors cut at its
    query time in numpy, de-duplicated newest first, packed and passed as ``exclude=`` - once with the mirrors already fetched
    (``lists``), once with the mirrors dropped before every call as ``NeighborFinder.append`` leaves them, so that the call
    pays the fetch (``lists_fetch``).  The three routes must return equal outputs: asserted.
Device events around every call (the host work of a call lies between its two events), 30 calls of each after 5, the routes
alternating in one process - the whole query at 50 000 users 10 calls after 2: a call of the host route takes seconds there;
median [min, max] in milliseconds.  The last line is one JSON object."""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pfotgnrec_amd as P
from pfotgnrec_amd.synthetic import CONFIGS, make_graph

HISTORY, B, K_TOP, WARM, REPS = 600_000, 512, 10, 5, 30
dev = torch.device("cuda:0")
P._lib.require_gpu(dev)


def stats(v):
    v = sorted(v)
    return {"median": round(float(np.median(v)), 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def alternate(routes, warm=WARM, reps=REPS):
    """{name: [ms] * reps} for (name, fn) routes: ``warm`` calls of each, then ``reps`` rounds in alternating order."""
    for _, fn in routes:
        for _ in range(warm):
            fn()
    t = {name: [] for name, _ in routes}
    for rep in range(reps):
        for name, fn in (routes if rep % 2 == 0 else routes[::-1]):
            t[name].append(timed(fn)[0])
    return t


def host_lists(nf, users, now):
    """What a caller did before: the finder's host mirrors, each user's row cut at its time, distinct ids newest first."""
    indptr, nbr, ts = nf.indptr, nf.nbr, nf.ts
    lists = []
    for u in users:
        b, e = int(indptr[u]), int(indptr[u + 1])
        row = nbr[b:b + int(np.searchsorted(ts[b:e], now, side="left"))][::-1]
        _, first = np.unique(row, return_index=True)
        lists.append(row[np.sort(first)].tolist())
    return lists


def main():
    cfg = CONFIGS["C2"]
    g = make_graph(cfg, with_prices=False)
    d = g.data
    n_all = g.node_features.shape[0]
    hist = slice(0, HISTORY)
    nf = P.NeighborFinder.from_arrays(d.sources[hist], d.destinations[hist], d.edge_idxs[hist], d.timestamps[hist], uniform=False,
                                      max_node_idx=n_all - 1, device=dev)
    tgn = P.TGN(nf, g.node_features, g.edge_features[:HISTORY + 1], dev, n_layers=2, n_heads=2, dropout=0.1, use_memory=True,
                memory_dimension=cfg.dim, message_function="identity", n_neighbors=cfg.n_neighbors)
    tgn.eval()
    tgn.observe(d.sources[HISTORY - 20 * B:HISTORY], d.destinations[HISTORY - 20 * B:HISTORY], d.timestamps[HISTORY - 20 * B:HISTORY],
                d.edge_idxs[HISTORY - 20 * B:HISTORY], batch_size=B)
    now = float(d.timestamps[HISTORY])
    items = np.arange(cfg.n_users + 1, cfg.n_users + cfg.n_items + 1)
    indptr, nbr, _, adj_ts = nf.device_arrays(dev)
    rs = np.random.RandomState(1)

    # ---- (a) the gather alone
    gather = {}
    for U in (512, 50_000):
        users = torch.from_numpy(rs.choice(d.sources[hist], size=U).astype(np.int32)).to(dev)
        ts = torch.full((U,), now, dtype=torch.float64, device=dev)
        routes = tuple(("W%d%s" % (W, "_counts" if c else ""),
                        (lambda W=W, c=c: P.history_gather(indptr, nbr, adj_ts, users, ts, W, want=("node", "len", "time") + (("count",) if c else ()))))
                       for W in (8, 64, 256) for c in (False, True))
        t = alternate(routes)
        lens = P.history_gather(indptr, nbr, adj_ts, users, ts, 256, want=("len",))[0]
        rows = (indptr[users.long() + 1] - indptr[users.long()]).double()
        gather["U%d" % U] = dict({k: stats(v) for k, v in t.items()}, mean_row_entries=round(float(rows.mean()), 1),
                                 max_row_entries=int(rows.max()), mean_seen=round(float(lens.double().mean()), 1))
        print("gather U=%d: %s" % (U, json.dumps(gather["U%d" % U])), flush=True)

    # ---- (b) the whole query
    pool, query = np.unique(d.sources[hist]), {}
    for U, warm, reps in ((512, WARM, REPS), (50_000, 2, 10)):
        users = rs.choice(pool, size=min(U, len(pool)), replace=False)

        def lists_route(fetch):
            if fetch:
                # exactly what ``NeighborFinder.append`` does to the mirrors (``self._host = None`` behind the device merge): the
                # next reader pays the fetch.  Keep this in step with ``append`` should it ever invalidate them another way.
                nf._host = None
            return tgn.recommend(users, now, K_TOP, items, exclude=host_lists(nf, users, now))
        routes = (("seen", lambda: tgn.recommend(users, now, K_TOP, items, exclude="seen")),
                  ("lists", lambda: lists_route(False)), ("lists_fetch", lambda: lists_route(True)))
        outs = {name: fn() for name, fn in routes}
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for o in ("lists", "lists_fetch") for a, b in zip(outs["seen"], outs[o])), "the routes must return equal outputs"
        tq = alternate(routes, warm, reps)
        med = {k: float(np.median(v)) for k, v in tq.items()}
        query["U%d" % len(users)] = dict({k: stats(v) for k, v in tq.items()}, warmup=warm, reps=reps,
                                         lists_over_seen=round(med["lists"] / med["seen"], 3),
                                         lists_fetch_over_seen=round(med["lists_fetch"] / med["seen"], 3), outputs_equal=True)
        print("query U=%d: %s" % (len(users), json.dumps(query["U%d" % len(users)])), flush=True)
    print(json.dumps({"what": "history gather on the C2 graph (600 000 edges of history, L2 K20 D172 H2, memory + GRU): (a) the gather "
                              "alone over the finder's device CSR; (b) recommend(exclude='seen') vs rows cut from the finder's host "
                              "mirrors in numpy and passed as exclude=, 500 items, k = 10",
                      "clock": "device events around whole calls, milliseconds", "warmup": WARM, "reps": REPS, "gather_ms": gather,
                      "query_ms": query}), flush=True)


if __name__ == "__main__":
    main()
