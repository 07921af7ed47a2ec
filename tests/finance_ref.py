"""numpy restatement of the investment metrics of the reference's evaluation loop, for sizes the fixtures cannot cover.

Written from the formulas, not copied: per interaction and per price table (past = in-sample, future = out-of-sample)
    rows  = log-returns of the portfolio's stocks followed by those of the top-k recommended stocks (evaluation.py:26-31:
            np.concatenate, so a stock that occurs twice counts twice), log-return = np.log(p[1:] / p[:-1]) per stock
    daily = rows.mean(axis=0)                                                        (evaluation.py:32)
    ret   = daily.mean() * 251;  sharpe = ret / (daily.std(ddof=0) * sqrt(251))     (evaluation.py:33-34)
    out   = (ret, sharpe) of portfolio + top-k  minus  (ret, sharpe) of the portfolio alone   (evaluation.py:36, 158-172),
            the latter 0, 0 for an empty portfolio (evaluation.py:153-157)
for k = 1, 3, 5.  The ranking that picks the top-k is the project's canonical order: stable ascending
argsort, reversed - score descending, the larger candidate position first among equal scores.
"""
import numpy as np

TOPK = (1, 3, 5)


def canonical_order(scores):
    """Positions of a score row [positive | negatives] in the canonical order."""
    return np.argsort(np.asarray(scores), kind="stable")[::-1]


def tie_free(scores, k):
    """No group of equal scores straddles position k of the sorted row (the top-k SET does not depend on the tie policy)."""
    s = np.sort(np.asarray(scores))[::-1]
    return k >= len(s) or s[k - 1] != s[k]


def _ret_sharpe(rows, dtype):
    rows = np.asarray(rows, dtype)
    daily = rows.mean(axis=0)
    ret = daily.mean() * dtype(251)
    return ret, ret / (daily.std() * np.sqrt(dtype(251)))


def invest_metrics(ret_past_day, ret_future_day, port, top_items, dtype=np.float64, parts=False):
    """f[12] = (return@1,3,5 | sharpe@1,3,5) in-sample, then out-of-sample, for one interaction.

    ret_*_day f64[n_items, n_ret]: the day's log-return tables; port: stock indices of the portfolio ([] = empty);
    top_items: stock indices of the recommended stocks, best first (at least 5, or all there are).
    ``dtype=np.longdouble`` evaluates the same formulas on the same fp64 log-returns in extended precision.
    ``parts=True`` also returns |new| + |old| per value (the magnitudes whose difference the value is)."""
    port = np.asarray(port, np.int64).reshape(-1)
    top = np.asarray(top_items, np.int64).reshape(-1)
    out, scale = np.zeros(12, dtype), np.zeros(12, dtype)
    for t, table in enumerate((ret_past_day, ret_future_day)):
        table = np.asarray(table, np.float64)
        old = (dtype(0), dtype(0)) if len(port) == 0 else _ret_sharpe(table[port], dtype)
        for i, k in enumerate(TOPK):
            new = _ret_sharpe(np.concatenate([table[port], table[top[:k]]], axis=0), dtype)
            for m in range(2):
                out[t * 6 + m * 3 + i] = new[m] - old[m]
                scale[t * 6 + m * 3 + i] = abs(new[m]) + abs(old[m])
    return (out, scale) if parts else out


def invest_bar(e_ref_max, scale):
    """Error bar of an fp64 implementation of ``invest_metrics`` against the extended-precision value.

    Both sides are fp64 sums of the same at most (W + 5) * n_ret terms, taken in different orders, followed by a subtraction
    that cancels.  ``e_ref_max`` is the largest error the reference's own fp64 evaluation shows in the fixture; another
    summation tree over the same terms may be that many times worse as it has levels more, bounded here by 16x.  The bar is
    floored at 8 ulp of |new| + |old| so that values the reference happens to hit exactly (new == old) do not make it zero."""
    return np.maximum(16.0 * float(e_ref_max), 8.0 * np.finfo(np.float64).eps * np.asarray(scale, np.float64))
