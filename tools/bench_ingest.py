#!/usr/bin/env python3
"""One serving tick of interactions the model has never seen: ``TGN.ingest`` against the only way there was before it.

On the C2 synthetic graph (L2 K20 D172 H2, memory + GRU) a model is built over the first 600 000 interactions and brought to a
populated state; the tick is the next 512 interactions with their RAW feature rows.  It is taken in twice, from the same saved
state (tables, finder and state restored in front of every repetition):
  ingest  : ONE ``TGN.ingest`` call - ``pfo_edge_rows_append`` (frozen statistics), ``pfo_tgn_observe``, the CSR append;
  rebuild : what the parent of this feature offers - a NEW ``TGN`` constructed over the concatenated raw edge table (which
            re-normalises EVERY row with different column statistics: the semantic defect that goes with the cost) and a new
            finder over [history ; tick], parameters copied across with ``load_state_dict``, memory and the pending-message
            tables copied across by hand, then ``observe`` of the tick on the new model.
Host clock (``time.perf_counter``) around a run that starts and ends in a device synchronise; WARM warm-up runs of each, then
REPS timed runs, the two alternating and the order swapped every repetition; median, min and max are printed.
The last line is one JSON object."""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pfotgnrec_amd as P
from pfotgnrec_amd.synthetic import CONFIGS, make_graph

WARM, REPS = 1, 7
HISTORY, TICK, B = 600_000, 512, 512
dev = torch.device("cuda:0")
P._lib.require_gpu(dev)


def stats(v):
    v = sorted(v)
    return {"median": round(1e3 * float(np.median(v)), 3), "min": round(1e3 * v[0], 3), "max": round(1e3 * v[-1], 3)}


def main():
    cfg = CONFIGS["C2"]
    g = make_graph(cfg, with_prices=False, with_portfolios=False)
    d = g.data
    kw = dict(n_layers=2, n_heads=2, dropout=0.1, use_memory=True, memory_dimension=cfg.dim, message_function="identity",
              n_neighbors=cfg.n_neighbors)
    hist = slice(0, HISTORY)
    tick = slice(HISTORY, HISTORY + TICK)
    n_all = g.node_features.shape[0]

    def finder(sl):
        return P.NeighborFinder.from_arrays(d.sources[sl], d.destinations[sl], d.edge_idxs[sl], d.timestamps[sl], uniform=False,
                                            max_node_idx=n_all - 1, device=dev)

    def served_model():
        t = P.TGN(finder(hist), g.node_features, g.edge_features[:HISTORY + 1], dev, **kw)
        t.eval()
        return t
    tgn = served_model()
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    # a populated state to start from: the 20 batches in front of the tick, then saved
    tgn.observe(d.sources[HISTORY - 20 * B:HISTORY], d.destinations[HISTORY - 20 * B:HISTORY], d.timestamps[HISTORY - 20 * B:HISTORY],
                d.edge_idxs[HISTORY - 20 * B:HISTORY], batch_size=B)
    saved = tgn.memory.backup_memory()
    params = {k: v.clone() for k, v in tgn.state_dict().items() if not k.startswith("memory.")}
    s_t, d_t, t_t = d.sources[tick], d.destinations[tick], d.timestamps[tick]
    raw_t = g.edge_features[d.edge_idxs[tick]]
    tgn.reserve(n_edges=HISTORY + 1 + (WARM + REPS + 2) * TICK)     # (the restore below only moves the row count back)
    end_state = {}

    def restore():
        """The served model as it was in front of the tick: tables, row count, finder, state."""
        tgn._edges.trim(HISTORY + 1)
        tgn._point_edges()
        tgn.set_neighbor_finder(finder(hist))
        tgn.memory.restore_memory(saved)

    def ingest_path():
        tgn.ingest(s_t, d_t, t_t, raw_t, batch_size=B)
        return tgn

    def rebuild_path():
        new = P.TGN(finder(slice(0, HISTORY + TICK)), g.node_features, g.edge_features[:HISTORY + 1 + TICK], dev, **kw)
        new.eval()
        new.load_state_dict(params, strict=False)
        new.memory.restore_memory(tgn.memory.backup_memory())
        new.observe(s_t, d_t, t_t, d.edge_idxs[tick], batch_size=B)
        return new
    paths = (("ingest", ingest_path), ("rebuild", rebuild_path))
    for name, fn in paths:
        for _ in range(WARM):
            restore()
            out = fn()
        torch.cuda.synchronize()
        end_state[name] = out.memory.memory.detach().clone()
    t = {"ingest": [], "rebuild": []}
    for rep in range(REPS):
        for name, fn in (paths if rep % 2 == 0 else paths[::-1]):
            restore()
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); t[name].append(time.perf_counter() - t0)
    # (the two end states differ BY DESIGN: the rebuilt model sees every edge feature under new column statistics)
    diff = float((end_state["ingest"] - end_state["rebuild"]).abs().max() / end_state["rebuild"].abs().max())
    mi, mr = float(np.median(t["ingest"])), float(np.median(t["rebuild"]))
    print(json.dumps({"what": "one tick of 512 unseen interactions on the C2 graph (600 000 edges of history, L2 K20 D172 H2): "
                              "TGN.ingest vs a new TGN over the concatenated arrays with parameters, memory and messages copied across",
                      "clock": "host perf_counter around synchronised runs", "warmup": WARM, "reps": REPS,
                      "ingest_ms": stats(t["ingest"]), "rebuild_ms": stats(t["rebuild"]), "rebuild_over_ingest": round(mr / mi, 1),
                      "end_memory_max_relative_difference_renormalised_rebuild": diff}), flush=True)


if __name__ == "__main__":
    main()
