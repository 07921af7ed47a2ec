#!/usr/bin/env python3
"""Erasure by node: ``TGN.forget`` against the only way there was before it, beside ``TGN.expire`` on the same graph.

On the C2 synthetic graph (L2 K20 D172 H2, memory + GRU) a model is built over the first 600 000 interactions and brought to a
populated state - the graph of ``tools/bench_expire.py``.  Every run starts from the same saved state (table rows, row count,
finder, memory and node features restored in front of every repetition):
  forget vs rebuild : ONE ``TGN.forget`` of 500 users and 5 items (1 % of each; an item is a hub row of about 2 400 entries) - the
            flags, the sweep of the adjacency, the node rows, the release decision, the table compaction, the id rewrite - against
            what the parent of this feature offers: ``NeighborFinder.from_arrays`` over the log without the interactions that
            touch a forgotten node, with densely renumbered edge ids, a NEW ``TGN`` over the kept raw feature rows (which
            re-normalises them with different column statistics), parameters copied across with ``load_state_dict``, memory and
            the pending-message tables copied across by hand and the forgotten rows zeroed.
  expire    : ONE ``TGN.expire`` at the timestamp of the middle interaction, as ``bench_expire.py`` times it, for the record.
Host clock (``time.perf_counter``) around a run that starts and ends in a device synchronise; WARM warm-up runs of each, then
REPS timed runs, forget and rebuild alternating and the order swapped every repetition; median, min and max are printed.
The last line is one JSON object."""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pfotgnrec_amd as P
from pfotgnrec_amd.synthetic import CONFIGS, make_graph

WARM, REPS = 1, 7
HISTORY, B = 600_000, 512
N_FORGET_USERS, N_FORGET_ITEMS = 500, 5
dev = torch.device("cuda:0")
P._lib.require_gpu(dev)


def stats(v):
    v = sorted(v)
    return {"median": round(1e3 * float(np.median(v)), 3), "min": round(1e3 * v[0], 3), "max": round(1e3 * v[-1], 3)}


def alternate(paths, restore):
    """``paths``: (name, run) pairs.  Returns name -> list of seconds."""
    for _, run in paths:
        for _ in range(WARM):
            restore(); run()
    t = {name: [] for name, _ in paths}
    for rep in range(REPS):
        for name, run in (paths if rep % 2 == 0 else paths[::-1]):
            restore()
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
    hist = slice(0, HISTORY)
    n_all = g.node_features.shape[0]
    src, dst, eid, ts = d.sources[hist], d.destinations[hist], d.edge_idxs[hist], d.timestamps[hist]

    def finder(s, t, e, when):
        return P.NeighborFinder.from_arrays(s, t, e, when, uniform=False, max_node_idx=n_all - 1, device=dev)
    full_finder = lambda: finder(src, dst, eid, ts)
    tgn = P.TGN(full_finder(), g.node_features, g.edge_features[:HISTORY + 1], dev, **kw)
    tgn.eval()
    tgn.observe(src[-20 * B:], dst[-20 * B:], ts[-20 * B:], eid[-20 * B:], batch_size=B)
    saved = tgn.memory.backup_memory()
    params = {k: v.clone() for k, v in tgn.state_dict().items() if not k.startswith("memory.")}
    table, nodes = tgn._edges.storage[0].clone(), tgn._nodes.storage[0].clone()
    rs = np.random.RandomState(0)
    ids = np.concatenate([rs.choice(np.arange(1, cfg.n_users + 1), N_FORGET_USERS, replace=False),
                          rs.choice(np.arange(cfg.n_users + 1, cfg.n_users + cfg.n_items + 1), N_FORGET_ITEMS, replace=False)])
    keep = ~(np.isin(src, ids) | np.isin(dst, ids))
    kept_rows = np.concatenate([[0], eid[keep]])                   # the filtered log's feature rows, padding row first
    dense = np.arange(1, int(keep.sum()) + 1)
    ids_dev = torch.from_numpy(ids).to(dev)
    cutoff = float(ts[HISTORY // 2])

    def restore():
        """The served model as it was: table rows, row count, node features, finder, state."""
        tgn._edges.storage[0].copy_(table)
        tgn._edges.rows = HISTORY + 1                              # (back UP after a compaction)
        tgn._point_edges()
        tgn._nodes.storage[0].copy_(nodes)
        tgn.set_neighbor_finder(full_finder())
        tgn.memory.restore_memory(saved)
    out = {}

    def forget_path():
        out["forget"] = tgn.forget(ids)
        out["after"] = (int(tgn.neighbor_finder.device_arrays(dev)[1].shape[0]), int(tgn.edge_raw_features.shape[0]))

    def rebuild_path():
        nf = finder(src[keep], dst[keep], dense, ts[keep])
        new = P.TGN(nf, g.node_features, g.edge_features[kept_rows], dev, **kw)
        new.eval()
        new.load_state_dict(params, strict=False)
        new.memory.restore_memory(tgn.memory.backup_memory())
        with torch.no_grad():
            for t in (new.memory.memory, new.memory.last_update, new.memory.msg_table, new.memory.msg_time, new.memory.has_msg,
                      new.node_raw_features):
                t.index_fill_(0, ids_dev, 0)
        out["rebuild"] = new

    def expire_path():
        out["expire"] = tgn.expire(cutoff)
    t1 = alternate([("forget", forget_path), ("rebuild", rebuild_path)], restore)
    dropped, remap = out["forget"]
    entries_after, rows_after = out["after"]
    assert rows_after == len(kept_rows) and entries_after == 2 * int(keep.sum()), "both routes keep the same rows and entries"
    t2 = alternate([("expire", expire_path)], restore)
    mf, mr = float(np.median(t1["forget"])), float(np.median(t1["rebuild"]))
    print(json.dumps({"what": "C2 graph, 600 000 edges of history (L2 K20 D172 H2): TGN.forget of 500 users and 5 items vs a new finder "
                              "and a new TGN over the filtered log with state copied across; TGN.expire of half the history on the "
                              "same graph for the record",
                      "clock": "host perf_counter around synchronised runs", "warmup": WARM, "reps": REPS,
                      "nodes_forgotten": int(len(ids)), "entries_dropped": int(dropped), "entries_after": entries_after,
                      "rows_before": HISTORY + 1, "rows_after": rows_after,
                      "forget_ms": stats(t1["forget"]), "rebuild_ms": stats(t1["rebuild"]), "rebuild_over_forget": round(mr / mf, 1),
                      "expire_ms": stats(t2["expire"]), "expire_entries_dropped": int(out["expire"][0])}), flush=True)


if __name__ == "__main__":
    main()
