"""Holdings from trades in numpy - the sequential loop every device comparison of ``pfo_holdings_apply`` is
``np.array_equal`` / ``same_bits`` against.

Tables over the node rows as in ``holdings_ref``: ``idx`` i32[n_nodes, W], ``len`` i32[n_nodes], ``time`` f64[n_nodes], and
optionally ``qty`` f64[n_nodes, W] (0.0 at and behind ``len``).  Events: ``src``, ``stock``, ``side`` (+1 buy, -1 sell), ``ts`` and
optionally ``qty_in``."""
import math

import numpy as np

COUNTS = ("valid", "overflow", "unmatched", "closes", "middle_closes", "qty_added", "qty_reduced", "appended")


def new_qty(n_nodes, W):
    return np.zeros((n_nodes, W), np.float64)


def apply(idx, length, time, src, stock, side, ts, qty=None, qty_in=None, counters=None):
    """In place, the events in input order.  ``counters``: an int64[2] array (overflow, unmatched) the call ADDS to, or None.
    Returns the per-case counts of this call as a dict (``COUNTS``)."""
    n_nodes, W = idx.shape
    c = dict.fromkeys(COUNTS, 0)
    for e in range(len(src)):
        u, s, sd = int(src[e]), int(stock[e]), int(side[e])
        if not 1 <= u < n_nodes or s < 0 or sd not in (1, -1):
            continue
        q = 1.0
        if qty is not None and qty_in is not None:
            q = float(qty_in[e])
            if not (math.isfinite(q) and q > 0):
                continue
        c["valid"] += 1
        L = min(max(int(length[u]), 0), W)
        hit = np.flatnonzero(idx[u, :L] == s)
        j = int(hit[0]) if hit.size else -1                     # the FIRST occurrence decides
        if sd == 1:
            if j >= 0:
                if qty is not None:
                    qty[u, j] = qty[u, j] + np.float64(q)
                    c["qty_added"] += 1
            elif L < W:
                idx[u, L] = s
                if qty is not None:
                    qty[u, L] = q
                length[u] = L + 1
                c["appended"] += 1
            else:
                c["overflow"] += 1
        elif j < 0:
            c["unmatched"] += 1
        else:
            rem = qty[u, j] - np.float64(q) if qty is not None else None
            if rem is not None and rem > 0:
                qty[u, j] = rem
                c["qty_reduced"] += 1
            else:
                idx[u, j:L - 1] = idx[u, j + 1:L].copy()
                idx[u, L - 1] = -1
                if qty is not None:
                    qty[u, j:L - 1] = qty[u, j + 1:L].copy()
                    qty[u, L - 1] = 0.0
                length[u] = L - 1
                c["closes"] += 1
                c["middle_closes"] += j < L - 1
        time[u] = ts[e]
    if counters is not None:
        counters[0] += c["overflow"]
        counters[1] += c["unmatched"]
    return c


def final_rows(idx, length, time, users):
    """What the snapshot writer is fed for snapshot equivalence: (src, port_idx, port_len, ts) of ``users``' present rows."""
    users = np.asarray(users, np.int32)
    return users, idx[users].copy(), length[users].copy(), time[users].copy()


def reload_events(idx, length, time, qty=None):
    """A saved ledger as trades: one buy per stored slot in slot order at the row's time -> (src, stock, side, ts, qty or None)."""
    n_nodes, W = idx.shape
    L = np.clip(length, 0, W)
    rows = np.repeat(np.arange(n_nodes), L)
    cols = np.concatenate([np.arange(k) for k in L]) if rows.size else np.zeros(0, np.int64)
    return (rows.astype(np.int32), idx[rows, cols].astype(np.int32), np.ones(rows.size, np.int32), time[rows].astype(np.float64),
            None if qty is None else qty[rows, cols].astype(np.float64))


def make_case(seed, n_nodes, W, N, users=None, quantities=False):
    """The issue's case generator -> (src, stock, side, ts, qty_in or None)."""
    rs = np.random.RandomState(seed)
    src = (rs.randint(-1, n_nodes + 1, N) if users is None else rs.choice(np.asarray(users), N)).astype(np.int32)
    stock = rs.randint(-1, 2 * W, N).astype(np.int32)
    side = rs.choice([1, 1, 1, -1, -1, 0, 2], N).astype(np.int32)
    ts = np.cumsum(rs.randint(0, 3, N)).astype(np.float64)
    qty_in = None
    if quantities:
        qty_in = rs.choice([1, 2, .5, 3, 0, -1, np.nan, np.inf], N, p=[.3, .2, .2, .1, .05, .05, .05, .05]).astype(np.float64)
    return src, stock, side, ts, qty_in


# (seed, n_nodes, W, N, users or None = all, quantities)
CASES = [(1, 70, 1, 513, None, False), (2, 70, 3, 513, None, False), (3, 70, 8, 5000, None, True), (4, 70, 64, 5000, (5,), False),
         (5, 70, 65, 5000, (5, 6), True), (6, 300, 256, 5000, (7, 299), False), (7, 70000, 8, 5000, None, True),
         (8, 70, 8, 64, None, False), (9, 70, 8, 65, (3,), True), (10, 70, 8, 1, None, False)]
