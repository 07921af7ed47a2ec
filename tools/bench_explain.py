#!/usr/bin/env python3
"""The explanation query on the C2 synthetic graph (50 000 users, 500 items, 1 000 000 interactions; L2 K20 D172 H2,
memory + GRU): a model over the first 600 000 interactions, 4096 roots (sources of the history, drawn with replacement, all at
the time of the next interaction).

(a) the launch alone: ``pfo_tgn_explain`` at hops 1 and 2 (m = 10 and 256, with and without the raw tables) over the workspace a
    forward-only pass of the 4096 roots left behind - next to (b) that pass itself (``TGN._embed_readonly``), the work the launch
    rides on.  Batches of 20 launches between two device events, per-launch time = batch / 20; 30 batches after 5.
(c) the whole query ``TGN.explain`` at hops 1 and 2: the pass, the launch and the output allocation.
Device events around every call (the host work of a call lies between its two events), 30 calls of each after 5, the routes
alternating in one process; median [min, max] in milliseconds.  The last line is one JSON object."""
import ctypes, json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pfotgnrec_amd as P
from pfotgnrec_amd import _lib
from pfotgnrec_amd.synthetic import CONFIGS, make_graph

HISTORY, B, ROOTS, WARM, REPS, PER_BATCH = 600_000, 512, 4096, 5, 30, 20
dev = torch.device("cuda:0")
_lib.require_gpu(dev)


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
    K, H = cfg.n_neighbors, 2
    rs = np.random.RandomState(1)
    roots = torch.from_numpy(rs.choice(d.sources[hist], size=ROOTS).astype(np.int32)).to(dev)
    ts = torch.full((ROOTS,), now, dtype=torch.float64, device=dev)

    # ---- (a) the launch alone, over the workspace of one pass, and (b) the pass
    tgn._embed_readonly(roots, ts, K)
    ws_cfg, ws = tgn._last_ws                                  # (back in the pool, untouched until the next forward)
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)

    def launcher(hops, m, raw):
        out = [new((ROOTS, m), torch.int32), new((ROOTS, m), torch.float64), new((ROOTS,), torch.int32), new((ROOTS, m), torch.int32),
               new((ROOTS, m), torch.float32), new((ROOTS, m), torch.int32)]
        raws = [None] * 8
        if raw:
            raws[:4] = [new((ROOTS, K), torch.int32), new((ROOTS, H, K), torch.float32), new((ROOTS, K), torch.float32), new((ROOTS, K), torch.int32)]
            if hops == 2:
                raws[4:] = [new((ROOTS, K, K), torch.int32), new((ROOTS, K, H, K), torch.float32), new((ROOTS, K, K), torch.float32),
                            new((ROOTS, K, K), torch.int32)]
        ptrs = [None if t is None else t.data_ptr() for t in out + raws]

        def run():
            for _ in range(PER_BATCH):
                _lib.call("pfo_tgn_explain", ctypes.byref(ws_cfg), ws.data_ptr(), ROOTS, K, hops, m, *ptrs, _lib.stream_ptr())
            return out, raws                                   # (kept alive across the timed window)
        return run
    routes = tuple(("hops%d_m%d%s" % (hops, m, "_raw" if raw else ""), launcher(hops, m, raw))
                   for hops in (1, 2) for m, raw in ((10, False), (256, False), (10, True)))
    t = alternate(routes)
    launch = {k: stats([x / PER_BATCH for x in v]) for k, v in t.items()}
    n_valid = launcher(2, 256, False)()[0][2]
    print("launch alone (ms per launch): %s" % json.dumps(launch), flush=True)
    t = alternate((("embed_pass", lambda: tgn._embed_readonly(roots, ts, K)),))
    embed = stats(t["embed_pass"])
    print("forward-only pass of %d roots: %s" % (ROOTS, json.dumps(embed)), flush=True)

    # ---- (c) the whole query
    routes = tuple(("explain_hops%d" % hops, (lambda hops=hops: tgn.explain(roots, ts, 10, hops=hops))) for hops in (1, 2))
    routes += (("embed_pass", lambda: tgn._embed_readonly(roots, ts, K)),)
    query = {k: stats(v) for k, v in alternate(routes).items()}
    print("whole query: %s" % json.dumps(query), flush=True)
    share = {k: round(v["median"] / embed["median"], 4) for k, v in launch.items()}
    print(json.dumps({"what": "explanation query on the C2 graph (600 000 edges of history, L2 K20 D172 H2, memory + GRU), %d roots: "
                              "(a) pfo_tgn_explain alone over the workspace of a forward-only pass, ms per launch; (b) that pass; "
                              "(c) TGN.explain whole, m = 10" % ROOTS,
                      "clock": "device events around whole calls, milliseconds", "warmup": WARM, "reps": REPS,
                      "launches_per_timed_batch": PER_BATCH, "launch_ms": launch, "embed_pass_ms": embed,
                      "launch_over_embed_pass": share, "query_ms": query,
                      "mean_n_valid_hops2_m256": round(float(n_valid.double().mean()), 1)}), flush=True)


if __name__ == "__main__":
    main()
