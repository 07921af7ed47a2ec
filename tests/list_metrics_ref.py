"""numpy restatement of ``pfo_list_metrics`` (include/pfotgn.h): a served list scored against what happened.

Written from the contract, not from the kernel.  Per user
    counted slots   t < clamp(n_valid, 0, L) whose id is >= 0; a skipped slot keeps its place (cutoff c = the first c SLOTS)
    rank            the first counted slot whose id equals truth (truth >= 0), else RANK_NONE
    hits, ndcg      fp32: rank < c, and 1 / log2(rank + 2) where hit, all in fp32 (numpy's log2f)
and per table (past = in-sample with day_past, future = out-of-sample with day_future, each with its own extents)
    rows(c) = log-returns of the portfolio's stocks, then those of the counted slots among the first c (a stock that occurs twice
              counts twice; stock of an item = id - upper_u - 1)
    daily   = rows.mean(axis=0);  ret = daily.mean() * 251;  sharpe = ret / (daily.std(ddof=0) * sqrt(251))
    figure  = (ret, sharpe) of rows(c) minus (ret, sharpe) of the portfolio alone - the latter 0, 0 for an empty portfolio
laid out (return@c.. | sharpe@c..) in-sample, then out-of-sample.  A day outside a table: that table's figures are NaN.  A stock
outside a table stands for a row of NaN: the series it takes part in are NaN in that table.  No rows at all (empty portfolio and
nothing counted): 0 / 0 = NaN.  The other table is never touched by either.
"""
import numpy as np

RANK_NONE = (1 << 31) - 1


def _ret_sharpe(rows, dtype):
    with np.errstate(all="ignore"):
        daily = np.asarray(rows, dtype).mean(axis=0)
        ret = daily.mean() * dtype(251)
        return ret, ret / (daily.std() * np.sqrt(dtype(251)))


def _rows_of(table, stocks, n_ret):
    """The log-return rows of ``stocks`` in one day's table [n_stocks, n_ret]; a stock outside it gives a row of NaN."""
    out = np.full((len(stocks), n_ret), np.nan)
    for i, s in enumerate(stocks):
        if 0 <= s < table.shape[0]:
            out[i] = table[s]
    return out


def list_metrics(list_item, n_valid, truth, cutoffs, port_idx, port_len, upper_u, ret_past, day_past, ret_future, day_future,
                 dtype=np.float64, parts=False):
    """(rank i32[U], hits f32[U, n_c], ndcg f32[U, n_c], invest dtype[U, 4 n_c]); ``parts=True`` adds |new| + |old| per investment
    value.  ``dtype=np.longdouble`` evaluates the same formulas on the same fp64 log-returns in extended precision.
    n_valid None: all L; port_idx None: empty portfolios."""
    list_item = np.asarray(list_item, np.int64)
    U, L = list_item.shape
    cuts = [int(c) for c in cutoffs]
    n_c = len(cuts)
    rank = np.full(U, RANK_NONE, np.int32)
    hits, ndcg = np.zeros((U, n_c), np.float32), np.zeros((U, n_c), np.float32)
    invest, scale = np.full((U, 4 * n_c), np.nan, dtype), np.full((U, 4 * n_c), np.nan, dtype)
    for u in range(U):
        nv = L if n_valid is None else min(max(int(n_valid[u]), 0), L)
        counted = [(t, int(list_item[u, t])) for t in range(nv) if list_item[u, t] >= 0]
        if truth[u] >= 0:
            at = [t for t, i in counted if i == truth[u]]
            if at:
                rank[u] = at[0]
        for i, c in enumerate(cuts):
            if rank[u] < c:
                hits[u, i] = 1
                ndcg[u, i] = np.float32(1) / np.log2(np.float32(rank[u]) + np.float32(2))
        port = []
        if port_idx is not None and np.asarray(port_idx).ndim == 2 and np.asarray(port_idx).shape[1] > 0:
            W = np.asarray(port_idx).shape[1]
            port = [int(s) for s in np.asarray(port_idx)[u, :min(max(int(port_len[u]), 0), W)]]
        for t, (tab, day) in enumerate(((ret_past, day_past), (ret_future, day_future))):
            tab = np.asarray(tab, np.float64)
            d = int(day[u])
            if not 0 <= d < tab.shape[0]:
                continue                                         # this table's figures stay NaN
            n_ret = tab.shape[2]
            prow = _rows_of(tab[d], port, n_ret)
            old = (dtype(0), dtype(0)) if not port else _ret_sharpe(prow, dtype)
            for i, c in enumerate(cuts):
                rows = np.concatenate([prow, _rows_of(tab[d], [s - upper_u - 1 for q, s in counted if q < c], n_ret)], axis=0)
                new = _ret_sharpe(rows, dtype) if rows.shape[0] else (dtype(np.nan), dtype(np.nan))
                for m in range(2):
                    with np.errstate(all="ignore"):
                        invest[u, t * 2 * n_c + m * n_c + i] = new[m] - old[m]
                        scale[u, t * 2 * n_c + m * n_c + i] = abs(new[m]) + abs(old[m])
    out = (rank, hits, ndcg, invest)
    return out + (scale,) if parts else out
