"""numpy reference of the position-weighted mean-variance order (``pfo_recommend_mv_topk_weighted`` and its wide and list
siblings, ``TGN.recommend(portfolio_weights=...)``): ``recommend_mv_ref`` / ``recommend_list_ref`` with one thing replaced - y,
which is main.py:268 with ``1.0 / np.sum(w) * np.sum(w * sigma_ij)`` in place of ``y_uj / n_holding * np.sum(sigma_ij)``, over the
holdings that COUNT: stock inside the table, weight finite and > 0.  The reference's own ``np.mean`` / ``np.cov`` calls stay.

On the exact return tables of ``recommend_mv_ref`` every covariance is one correctly rounded scaling of an exact sum, ``w * sigma``
is one rounded product, and with fewer than eight counted holdings both ``np.sum`` add sequentially in index order - the kernel's
order - so the cases keep to seven counted holdings at most and y agrees to the last bit.

Also here: the host model of ``pfo_holdings_gather_weights`` and the generators of the cases.  No import of the package."""
import numpy as np

import recommend_list_ref as L
import recommend_mv_ref as M

SHARES, VALUE = 0, 1


def counts(w):
    """A weight counts iff it is finite and > 0."""
    w = np.asarray(w, np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(w) & (w > 0)


def y_mv(returns, day, cand_stock, port, w, gamma=2.0):
    """``recommend_mv_ref.y_mv`` for one user holding the rows ``port`` with the weights ``w`` (both already cut down to the
    holdings that count) - main.py:243-271 line by line, :268 weighted."""
    cand_feature = returns[day][np.asarray(cand_stock, np.int64)]
    port = np.asarray(port, np.int64)
    w = np.asarray(w, np.float64)
    port_feature = returns[day][port] if len(port) else None
    y_mv_list = []
    with np.errstate(all="ignore"):
        for feature in cand_feature:
            mu_i = np.mean(feature)                                                # :243
            if port_feature is None:
                cov_i = np.cov(feature)                                            # :247
                sigma_i = cov_i
                y = (mu_i / gamma) / sigma_i                                       # :254
            else:
                cov_i = np.cov(feature, port_feature)                              # :259
                sigma_ij = cov_i[0, 1:]
                sigma_i = cov_i[0, 0]
                sum_sigma_ij = 1.0 / np.sum(w) * np.sum(w * sigma_ij)              # :268, weighted
                y = (mu_i / gamma - 0.5 * sum_sigma_ij) / sigma_i                  # :271
            y_mv_list.append(float(y))
    return np.array(y_mv_list, np.float64)


def portfolio(port_idx, port_len, port_w, u, n_stocks):
    """(stocks, weights) of the holdings of row u that count, in row order: among the first min(port_len[u], W) entries those
    with the stock in range and a weight that counts."""
    if port_idx is None or port_idx.shape[1] == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.float64)
    W = port_idx.shape[1]
    n = W if port_len is None else min(max(int(port_len[u]), 0), W)
    row, w = np.asarray(port_idx[u, :n], np.int64), np.asarray(port_w[u, :n], np.float64)
    keep = (row >= 0) & (row < n_stocks) & counts(w)
    return row[keep], w[keep]


def y_matrix(returns, day_idx, cand_stock, port_idx, port_len, port_w, gamma=2.0):
    """``recommend_mv_ref.y_matrix`` with the weighted y."""
    n_days, n_stocks, _ = returns.shape
    cand_stock = np.asarray(cand_stock, np.int64)
    U, I = len(day_idx), len(cand_stock)
    y = np.full((U, I), np.nan)
    inside = (cand_stock >= 0) & (cand_stock < n_stocks)
    uniq, inv = np.unique(cand_stock[inside], return_inverse=True)
    for u in range(U):
        d = int(day_idx[u])
        if 0 <= d < n_days and len(uniq):
            y[u, inside] = y_mv(returns, d, uniq, *portfolio(port_idx, port_len, port_w, u, n_stocks), gamma)[inv]
    return y


def weight_rows(seed, port_idx, port_len):
    """f64[U, W] beside ``port_idx``: random positive doubles; every fifth user from 5 on holds exact 1.0 rows.  The slots at
    and behind a row's length are read by nobody: NaN."""
    rs = np.random.RandomState(seed)
    U, W = port_idx.shape
    w = rs.uniform(0.01, 100.0, size=(U, W))
    w[5::5] = 1.0
    for u in range(U):
        w[u, min(max(int(port_len[u]), 0), W):] = np.nan
    return w


def weighted_side(seed, U, I, n_ret, W=8, **kw):
    """``recommend_mv_ref.mv_side`` with ``port_w`` added and two rows rewritten (W >= 8, the case not ``clean``): user 3's full
    row gets a zero, a negative, a NaN and a +inf weight among the valid ones; user 4 holds three in-range stocks none of whose
    weights counts - main.py:254.  User 2 holds one stock (``mv_side``).  At most seven holdings count anywhere."""
    c = M.mv_side(seed, U, I, n_ret, W, **kw)
    S = c["returns"].shape[1]
    rs = np.random.RandomState(seed + 1)
    if U > 4 and not kw.get("clean"):
        c["port_idx"][4, :3], c["port_len"][4] = rs.randint(1, S, size=3), 3
    w = weight_rows(seed + 2, c["port_idx"], c["port_len"])
    if not kw.get("clean"):
        if U > 3 and W >= 8:
            w[3, [2, 5, 6, 7]] = (0.0, -1.5, np.nan, np.inf)
        if U > 4:
            w[4, :3] = (0.0, np.nan, -2.0)
    c["port_w"] = w
    return c


def exact_case(seed, U, I, D, k, n_t, n_ret, W=8):
    """``recommend_mv_ref.exact_case`` with the weighted side in place of ``mv_side``."""
    import recommend_ref as R
    c = R.exact_case(seed, U, I, D, k, n_t)
    c.update(weighted_side(seed + 7, U, I, n_ret, W))
    return c


def y_of(c):
    return y_matrix(c["returns"], c["day_idx"], c["cand_stock"], c["port_idx"], c["port_len"], c["port_w"], c["gamma"])


def reference(c, lam, k, scores=None, y=None):
    """``recommend_mv_ref.reference`` over the weighted y (``y``: the ``y_raw`` of an earlier call on the same case)."""
    return M.reference(c, lam, k, scores, y_of(c) if y is None else y)


def reference_list(c, lam, k, scores=None, y=None):
    """``recommend_list_ref.reference_mv`` over the weighted y."""
    return L.reference_mv(c, lam, k, scores, y_of(c) if y is None else y)


# ---- pfo_holdings_gather_weights

def gather_weights(users, hold_idx, hold_len, hold_qty, mode, last_close=None):
    """The host model: w_out f64[U, W]."""
    n_nodes, W = hold_idx.shape
    users = np.asarray(users, np.int64)
    out = np.zeros((len(users), W), np.float64)
    ok = (users >= 0) & (users < n_nodes)
    u = np.where(ok, users, 0)
    length = np.where(ok, np.clip(hold_len[u], 0, W), 0)
    live = np.arange(W)[None, :] < length[:, None]
    qty = hold_qty[u]
    if mode == SHARES:
        out[live] = qty[live]
        return out
    stock = hold_idx[u].astype(np.int64)
    inside = (stock >= 0) & (stock < len(last_close))
    with np.errstate(invalid="ignore"):
        value = qty * np.asarray(last_close, np.float64)[np.where(inside, stock, 0)]
    out[live & inside] = value[live & inside]
    return out


def gather_case(seed, n_nodes, W, U, n_stocks):
    """A ledger with quantities and a close table: lengths beyond W and below 0, stocks outside [0, n_stocks) and negative,
    NaN closes (never quoted); users outside [0, n_nodes) among the queried ones."""
    rs = np.random.RandomState(seed)
    hold_idx = rs.randint(-2, n_stocks + 3, size=(n_nodes, W)).astype(np.int32)
    hold_len = rs.randint(-1, W + 3, size=n_nodes).astype(np.int32)
    hold_qty = rs.uniform(0.5, 500.0, size=(n_nodes, W))
    last_close = rs.uniform(1.0, 300.0, size=n_stocks)
    last_close[rs.rand(n_stocks) < 0.2] = np.nan
    users = rs.randint(0, n_nodes, size=U).astype(np.int32)
    for i, bad in enumerate((-1, n_nodes, n_nodes + 5, -2 ** 31, 2 ** 31 - 1)):
        if 3 * i + 1 < U:
            users[3 * i + 1] = bad
    return dict(users=users, hold_idx=hold_idx, hold_len=hold_len, hold_qty=hold_qty, last_close=last_close)
