"""The holdings ledger's rules in numpy - the reference every device comparison is ``np.array_equal`` against.

Tables over the node rows: ``idx`` i32[n_nodes, W] stock indices padded with -1, ``len`` i32[n_nodes] valid leading entries,
``time`` f64[n_nodes] the timestamp of the interaction that wrote the row.  A row that was never written holds (-1.., 0, -inf)."""
import numpy as np


def new_tables(n_nodes, W):
    return (np.full((n_nodes, W), -1, np.int32), np.zeros(n_nodes, np.int32), np.full(n_nodes, -np.inf, np.float64))


def store(idx, length, time, src, port_idx, port_len, ts):
    """In place, a sequential loop over the events in input order: per user the LAST event of the call wins; an empty portfolio
    overwrites; entries are stored verbatim; no comparison with the stored time; ids outside [1, n_nodes) are skipped."""
    n_nodes, W = idx.shape
    port_idx = np.asarray(port_idx, np.int32)
    stride = port_idx.shape[1] if port_idx.ndim == 2 else 0
    for e in range(len(src)):
        u = int(src[e])
        if not 1 <= u < n_nodes:
            continue
        L = min(max(int(port_len[e]), 0), min(W, stride))
        idx[u, :L] = port_idx[e, :L]
        idx[u, L:] = -1
        length[u] = L
        time[u] = ts[e]
    return idx, length, time


def gather(idx, length, users, items=None, upper_u=0):
    """-> (port_idx i32[U, W], port_len i32[U], excl_pos i32[U, W] or None without ``items``)."""
    n_nodes, W = idx.shape
    U = len(users)
    port_idx = np.full((U, W), -1, np.int32)
    port_len = np.zeros(U, np.int32)
    excl = None
    if items is not None:
        excl = np.full((U, W), -1, np.int32)
        where = {}
        for p, v in enumerate(np.asarray(items).tolist()):
            where[int(v)] = p
    for q in range(U):
        u = int(users[q])
        if not 0 <= u < n_nodes:
            continue
        port_idx[q] = idx[u]
        port_len[q] = length[u]
        if excl is not None:
            for j in range(min(max(int(length[u]), 0), W)):
                excl[q, j] = where.get(int(idx[u, j]) + int(upper_u) + 1, -1) if idx[u, j] >= 0 else -1
    return port_idx, port_len, excl


def held_node_lists(idx, length, users, upper_u):
    """What a caller of the list route passes as ``exclude``: per user the item NODE ids of its row."""
    out = []
    for u in users:
        u = int(u)
        out.append([int(s) + int(upper_u) + 1 for s in idx[u, :length[u]]] if 0 <= u < idx.shape[0] else [])
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
