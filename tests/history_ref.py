"""The rule of ``pfo_history_gather`` (include/pfotgn.h) restated in numpy: what each user's row of a time-sorted CSR names
strictly before the user's query time - distinct neighbours, newest first - and the cases the GPU tests rest on, built here so
that the CPU tests can prove them binding from this reference alone."""
import collections

import numpy as np

I32_MAX = 2 ** 31 - 1
NAN_BITS = np.array([np.nan]).view(np.int64)[0]

Rows = collections.namedtuple("Rows", "node len time count pos stock")


def same_bits(a, b):
    """Equal shape, dtype and bytes (NaN padding and signed zeros included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def window(indptr, adj_ts, u, t, since=None, max_scan=0):
    """(lo, hi): the row entries [lo, hi) of user ``u`` a query at time ``t`` walks (row-relative); (0, 0) when empty."""
    n_nodes = len(indptr) - 1
    if not 0 <= u < n_nodes or not np.isfinite(t):
        return 0, 0
    row = adj_ts[indptr[u]:indptr[u + 1]]
    hi = int(np.searchsorted(row, t, side="left"))              # entries with ts < t (fp64, strict)
    lo = 0 if since is None or np.isnan(since) else int(np.searchsorted(row, since, side="left"))
    if max_scan > 0:
        lo = max(lo, hi - max_scan)
    return (lo, hi) if hi > lo else (0, 0)


def gather(indptr, adj_nbr, adj_ts, users, ts, W, since=None, max_scan=0, items=None, upper_u=None):
    """``Rows`` of host arrays: node i32[U, W] (-1 padding), len i32[U], time f64[U, W] (NaN padding), count i32[U, W] (0), pos
    i32[U, W] (-1; None without ``items``), stock i32[U, W] (-1; None without ``upper_u``)."""
    indptr, adj_nbr, adj_ts = np.asarray(indptr, np.int64), np.asarray(adj_nbr, np.int32), np.asarray(adj_ts, np.float64)
    users, ts = np.asarray(users, np.int64), np.asarray(ts, np.float64)
    U = len(users)
    node = np.full((U, W), -1, np.int32)
    length = np.zeros(U, np.int32)
    time = np.full((U, W), np.nan, np.float64)
    count = np.zeros((U, W), np.int32)
    where = None
    if items is not None:
        where = {int(v): i for i, v in enumerate(np.asarray(items).tolist())}
    for q in range(U):
        u = int(users[q])
        lo, hi = window(indptr, adj_ts, u, ts[q], None if since is None else since[q], max_scan)
        if hi <= lo:
            continue
        base = int(indptr[u])
        nbr = adj_nbr[base + lo:base + hi][::-1]                # newest first; among equal timestamps the later entry first
        tt = adj_ts[base + lo:base + hi][::-1]
        uniq, first, cnt = np.unique(nbr, return_index=True, return_counts=True)
        order = np.argsort(first, kind="stable")[:W]            # by first meeting; beyond W dropped, repeats and all
        k = len(order)
        node[q, :k], time[q, :k], count[q, :k], length[q] = uniq[order], tt[first[order]], cnt[order], k
    pos = stock = None
    if items is not None:
        pos = np.asarray([[where.get(int(v), -1) if v >= 0 else -1 for v in r] for r in node], np.int32).reshape(U, W)
    if upper_u is not None:
        s = node.astype(np.int64) - int(upper_u) - 1
        stock = np.where((node >= 0) & (s >= 0) & (s < 2 ** 31), s, -1).astype(np.int32)
    return Rows(node, length, time, count, pos, stock)


def gather_loop(indptr, adj_nbr, adj_ts, users, ts, W, since=None, max_scan=0):
    """The same rule as a plain loop over row entries, one compare at a time -> (node lists, time lists, count lists)."""
    out = []
    for q, u in enumerate(users):
        ids, times, counts = [], [], []
        if 0 <= u < len(indptr) - 1 and np.isfinite(ts[q]):
            b, e = int(indptr[u]), int(indptr[u + 1])
            s = None if since is None or np.isnan(since[q]) else since[q]
            inside = [i for i in range(b, e) if adj_ts[i] < ts[q]]
            hi = len(inside)
            lo = 0 if s is None else sum(1 for i in range(b, e) if adj_ts[i] < s)
            if max_scan > 0:
                lo = max(lo, hi - max_scan)
            dropped = set()
            for i in range(b + hi - 1, b + lo - 1, -1):
                v = int(adj_nbr[i])
                if v in ids:
                    counts[ids.index(v)] += 1
                elif v in dropped:
                    pass
                elif len(ids) < W:
                    ids.append(v), times.append(float(adj_ts[i])), counts.append(1)
                else:
                    dropped.add(v)
        out.append((ids, times, counts))
    return out


def node_lists(rows):
    """The kept node ids of every user as Python lists, newest first (the explicit ``exclude=`` / ``only=`` form)."""
    return [rows.node[q, :rows.len[q]].tolist() for q in range(len(rows.len))]


def csr(rows_nbr, rows_ts):
    """(indptr i64, adj_nbr i32, adj_ts f64) from per-node lists (each row's timestamps ascending)."""
    indptr = np.zeros(len(rows_nbr) + 1, np.int64)
    np.cumsum([len(r) for r in rows_nbr], out=indptr[1:])
    cat = lambda rows, dt: np.concatenate([np.asarray(r, dt) for r in rows] + [np.zeros(0, dt)])
    return indptr, cat(rows_nbr, np.int32), cat(rows_ts, np.float64)


# ---------------------------------------------------------------------------------------------- the cases of the GPU test
ROW_LENGTHS = (0, 1, 63, 64, 65, 129, 300, 5000)
WIDTHS = (1, 8, 64, 256)
USER_COUNTS = (1, 5, 67)
MAX_SCANS = (1, 64, 65)
N_NODES = 1300                  # rows 1 .. 8 have the lengths above, rows 9 .. 13 are the special ones, the rest are empty
TIED_ROW, CHUNK_ROW, CROSS_ROW, FULL_ROW, WIDE_ROW = 9, 10, 11, 12, 13
UPPER_U = 40


def world(seed=11):
    """A CSR whose rows have every length of ``ROW_LENGTHS`` (row r + 1 has length ROW_LENGTHS[r]) with repeated neighbours and
    runs of tied timestamps, and the special rows: TIED_ROW - 100 entries at one timestamp; CHUNK_ROW - 40 entries, every id
    twice inside one chunk; CROSS_ROW - 200 entries over 70 ids, each id's repeats more than 64 entries apart; FULL_ROW - 400
    entries whose 20 newest ids come back after the list is full; WIDE_ROW - 600 entries over 400 distinct ids (cut by every
    W).  Neighbour ids lie in [1, N_NODES)."""
    rs = np.random.RandomState(seed)
    nbr, ts = [[] for _ in range(N_NODES)], [[] for _ in range(N_NODES)]
    for r, n in enumerate(ROW_LENGTHS):
        nbr[r + 1] = rs.randint(1, max(2, min(N_NODES, 2 + n // 3)), size=n).tolist()       # about three entries per id
        ts[r + 1] = np.sort(rs.randint(0, max(1, n // 2) + 1, size=n).astype(np.float64) * 0.5).tolist()   # ties
    nbr[TIED_ROW], ts[TIED_ROW] = rs.randint(1, 30, size=100).tolist(), [7.0] * 100
    nbr[CHUNK_ROW], ts[CHUNK_ROW] = np.repeat(rs.permutation(np.arange(100, 120)), 2).tolist(), np.arange(40.0).tolist()
    nbr[CROSS_ROW], ts[CROSS_ROW] = (np.arange(200) % 70 + 200).tolist(), np.arange(200.0).tolist()
    late = np.arange(500, 520)
    nbr[FULL_ROW] = np.concatenate([np.tile(late, 5), rs.permutation(np.arange(600, 900)), late]).tolist()[-400:]
    ts[FULL_ROW] = (np.arange(400.0) * 0.25).tolist()
    nbr[WIDE_ROW] = np.concatenate([rs.permutation(np.arange(800, 1200)), rs.randint(800, 1200, size=200)]).tolist()
    ts[WIDE_ROW] = np.sort(rs.rand(600) * 100).tolist()
    return csr(nbr, ts)


def queries(indptr, adj_ts, U, seed):
    """(users i64[U], ts f64[U], since f64[U]) over ``world``: the users cycle through every row with entries, the empty row 1,
    an empty row behind them and the ids -1 and N_NODES; query times sit ON an entry's timestamp (strict: that entry and its
    ties are not seen), past the row's end, before its start, and at NaN / +inf / -inf; ``since`` sits ON an entry's timestamp
    (inclusive), is NaN (absent), -inf, +inf, or above the query time."""
    rs = np.random.RandomState(seed)
    pool = [2, 5, 8, TIED_ROW, WIDE_ROW, 1, -1, 3, 4, 6, 7, CHUNK_ROW, CROSS_ROW, FULL_ROW, N_NODES, 700]
    users = np.asarray([pool[(i + seed) % len(pool)] for i in range(U)], np.int64)
    ts, since = np.zeros(U), np.full(U, np.nan)
    for q, u in enumerate(users):
        row = adj_ts[indptr[u]:indptr[u + 1]] if 0 <= u < N_NODES else np.zeros(0)
        n, kind = len(row), (q + seed) % 7
        if n == 0:
            ts[q] = 5.0
            continue
        at = float(row[rs.randint(n // 2, n)])
        ts[q] = [at, float(row[-1]) + 1.0, at, float(row[-1]) + 1.0, at, at, float(row[-1]) + 1.0][kind]
        if kind in (2, 3):
            since[q] = float(row[rs.randint(0, n // 2 + 1)])        # on an entry: inclusive
        elif kind == 4:
            since[q] = ts[q] + 1.0                                  # above the query time: empty
        elif kind == 5:
            since[q] = -np.inf
    if U >= 60:
        ts[U - 1], ts[U - 2], ts[U - 3], ts[U - 4] = np.nan, np.inf, -np.inf, float(adj_ts[indptr[8]]) - 1.0
        users[U - 4:] = [8, 8, 8, 8]
        since[U - 5], users[U - 5], ts[U - 5] = np.inf, 8, 1e9
    return users, ts, since


def calls(U):
    """The (seed, max_scan) calls that make up the case of one (U, W) pair: ``queries(.., U, seed)`` at every ``max_scan`` of
    ``MAX_SCANS`` and without one.  The fewer users a call has, the more seeds it takes for the case to meet every rule."""
    seeds = range(32) if U == 1 else range(8) if U == 5 else (3,)
    return [(seed, m) for seed in seeds for m in (0,) + MAX_SCANS]


def binding(indptr, adj_nbr, adj_ts, users, ts, W, since, max_scan):
    """How many users of ONE call each rule decides: dict(cut_by_W, repeats, empty, cut_by_since, cut_by_max_scan) - counted from
    the reference: a user is cut by W when an unbounded width keeps more ids, has repeats when a count exceeds 1, is cut by
    ``since`` / ``max_scan`` when dropping that argument moves its window's lower end."""
    full = gather(indptr, adj_nbr, adj_ts, users, ts, max(ROW_LENGTHS) + 1, since, max_scan)
    got = gather(indptr, adj_nbr, adj_ts, users, ts, W, since, max_scan)
    n = dict(cut_by_W=int((full.len > got.len).sum()), repeats=int((got.count.max(axis=1) > 1).sum()), empty=0, cut_by_since=0,
             cut_by_max_scan=0)
    for q, u in enumerate(users):
        lo, hi = window(indptr, adj_ts, int(u), ts[q], None if since is None else since[q], max_scan)
        n["empty"] += hi <= lo
        n["cut_by_since"] += since is not None and (lo, hi) != window(indptr, adj_ts, int(u), ts[q], None, max_scan)
        n["cut_by_max_scan"] += max_scan > 0 and (lo, hi) != window(indptr, adj_ts, int(u), ts[q], None if since is None else since[q], 0)
    return n
