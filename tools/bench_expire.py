#!/usr/bin/env python3
"""The retention window: ``TGN.expire`` against the only way back there was before it, and what it does to the serving tick.

On the C2 synthetic graph (L2 K20 D172 H2, memory + GRU) a model is built over the first 600 000 interactions and brought to a
populated state.  Two comparisons, every run from the same saved state (table rows, row count, finder and memory restored in
front of every repetition):
  expire vs rebuild : ONE ``TGN.expire`` at the timestamp of the middle interaction (half the history goes: the adjacency
            expiry, the release decision, the table compaction, the id rewrite) against what the parent of this feature
            offers - ``NeighborFinder.from_arrays`` over the filtered log with densely renumbered edge ids, a NEW ``TGN`` over
            the kept raw feature rows (which re-normalises them with different column statistics), parameters copied across
            with ``load_state_dict``, memory and the pending-message tables copied across by hand.
  tick before vs after : ONE ``TGN.ingest`` of the next 512 interactions on the full adjacency and on the expired one - the
            tick's CSR merge is linear in the adjacency size.
Host clock (``time.perf_counter``) around a run that starts and ends in a device synchronise; WARM warm-up runs of each, then
REPS timed runs, the two of a pair alternating and the order swapped every repetition; median, min and max are printed.
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


def alternate(paths, restore):
    """``paths``: two (name, prepare, run); prepare is untimed.  Returns name -> list of seconds."""
    for _, prep, run in paths:
        for _ in range(WARM):
            restore(); prep(); run()
    t = {name: [] for name, _, _ in paths}
    for rep in range(REPS):
        for name, prep, run in (paths if rep % 2 == 0 else paths[::-1]):
            restore(); prep()
            torch.cuda.synchronize(); t0 = time.perf_counter()
            run()
            torch.cuda.synchronize(); t[name].append(time.perf_counter() - t0)
    return t


def main():
    cfg = CONFIGS["C2"]
    g = make_graph(cfg, with_prices=False, with_portfolios=False)
    d = g.data
    kw = dict(n_layers=2, n_heads=2, dropout=0.1, use_memory=True, memory_dimension=cfg.dim, message_function="identity",
              n_neighbors=cfg.n_neighbors)
    hist, tick = slice(0, HISTORY), slice(HISTORY, HISTORY + TICK)
    n_all = g.node_features.shape[0]

    def finder(src, dst, eid, ts):
        return P.NeighborFinder.from_arrays(src, dst, eid, ts, uniform=False, max_node_idx=n_all - 1, device=dev)
    full_finder = lambda: finder(d.sources[hist], d.destinations[hist], d.edge_idxs[hist], d.timestamps[hist])
    tgn = P.TGN(full_finder(), g.node_features, g.edge_features[:HISTORY + 1], dev, **kw)
    tgn.eval()
    tgn.observe(d.sources[HISTORY - 20 * B:HISTORY], d.destinations[HISTORY - 20 * B:HISTORY], d.timestamps[HISTORY - 20 * B:HISTORY],
                d.edge_idxs[HISTORY - 20 * B:HISTORY], batch_size=B)
    saved = tgn.memory.backup_memory()
    params = {k: v.clone() for k, v in tgn.state_dict().items() if not k.startswith("memory.")}
    tgn.reserve(n_edges=HISTORY + 1 + 2 * TICK)
    table = tgn._edges.storage[0].clone()                              # (rows behind the live ones are zero)
    cutoff = float(d.timestamps[HISTORY // 2])
    keep = d.timestamps[hist] >= cutoff
    kept_rows = np.concatenate([[0], d.edge_idxs[hist][keep]])    # the filtered log's feature rows, padding row first
    dense = np.arange(1, int(keep.sum()) + 1)

    def restore():
        """The served model as it was: table rows, row count, finder, state."""
        tgn._edges.storage[0].copy_(table)
        tgn._edges.rows = HISTORY + 1                             # (back UP after an expiry, back down after a tick)
        tgn._point_edges()
        tgn.set_neighbor_finder(full_finder())
        tgn.memory.restore_memory(saved)
    out = {}

    def expire_path():
        out["expire"] = tgn.expire(cutoff)
        out["after"] = (int(tgn.neighbor_finder.device_arrays(dev)[1].shape[0]), int(tgn.edge_raw_features.shape[0]))   # (host-side shapes)

    def rebuild_path():
        nf = finder(d.sources[hist][keep], d.destinations[hist][keep], dense, d.timestamps[hist][keep])
        new = P.TGN(nf, g.node_features, g.edge_features[kept_rows], dev, **kw)
        new.eval()
        new.load_state_dict(params, strict=False)
        new.memory.restore_memory(tgn.memory.backup_memory())
        out["rebuild"] = new
    nothing = lambda: None
    t1 = alternate((("expire", nothing, expire_path), ("rebuild", nothing, rebuild_path)), restore)
    dropped, remap = out["expire"]
    entries_after, rows_after = out["after"]
    assert rows_after == len(kept_rows) and entries_after == 2 * int(keep.sum()), "both routes keep the same rows and entries"

    s_t, d_t, t_t = d.sources[tick], d.destinations[tick], d.timestamps[tick]
    raw_t = g.edge_features[d.edge_idxs[tick]]
    tick_run = lambda: tgn.ingest(s_t, d_t, t_t, raw_t, batch_size=B)
    t2 = alternate((("tick_before", nothing, tick_run), ("tick_after", lambda: tgn.expire(cutoff), tick_run)), restore)
    me, mr = float(np.median(t1["expire"])), float(np.median(t1["rebuild"]))
    mb, ma = float(np.median(t2["tick_before"])), float(np.median(t2["tick_after"]))
    print(json.dumps({"what": "C2 graph, 600 000 edges of history (L2 K20 D172 H2): TGN.expire dropping half the history vs a new finder "
                              "and a new TGN over the filtered log with state copied across; a 512-interaction TGN.ingest tick on the "
                              "full and on the expired adjacency",
                      "clock": "host perf_counter around synchronised runs", "warmup": WARM, "reps": REPS,
                      "entries_dropped": int(dropped), "entries_after": entries_after, "rows_before": HISTORY + 1, "rows_after": rows_after,
                      "expire_ms": stats(t1["expire"]), "rebuild_ms": stats(t1["rebuild"]), "rebuild_over_expire": round(mr / me, 1),
                      "tick_before_ms": stats(t2["tick_before"]), "tick_after_ms": stats(t2["tick_after"]),
                      "tick_before_over_after": round(mb / ma, 2)}), flush=True)


if __name__ == "__main__":
    main()
