"""numpy reference of the portfolio-aware top-k (``pfo_recommend_mv_topk`` / ``TGN.recommend(mv=...)``): ``recommend_ref`` for
scores, eps, the skip rules and the canonical order, the reference project's own numpy calls for y_mv (main.py:243-271:
``np.mean``, ``np.cov`` ddof=1, ``np.sum``) and ``scipy.stats.rankdata`` for the two ranks (main.py:282).

Return tables of the cases below are small integers / 64 whose rows sum to a multiple of n_ret: every mean, deviation, product
and sum of products is then exact in ANY order, so ``np.cov`` (a BLAS product, summation order unknown) and a kernel that adds
in index order agree to the last bit, as the small-integer embeddings make every fp32 score exact.  What is left are single
correctly rounded operations in a fixed order - as long as fewer than eight stocks are held: from eight on ``np.sum`` adds the
covariances pairwise, so the cases keep to seven holdings at most."""
import numpy as np
from scipy.stats import rankdata

import recommend_ref as R

# (seed, U, I, D, k) of the GPU test of 0 < lambda < 1 on random normal embeddings: chosen so that at least one user in two has
# every pair of admissible fp64 scores further apart than the two fp32 error bounds (tests/test_recommend_mv_cpu.py computes it)
BLEND_CASES = [(21, 37, 40, 32, 10), (22, 5, 40, 32, 5)]


def y_mv(returns, day, cand_stock, port, gamma=2.0):
    """y_mv of the candidates ``cand_stock`` (rows of returns[day]) for one user holding the rows ``port`` - main.py:243-271
    line by line on log-returns (what main.py:218/226-227 make of the prices).  Empty ``port``: the ``'' in stocks_p`` branch."""
    cand_feature = returns[day][np.asarray(cand_stock, np.int64)]
    port = np.asarray(port, np.int64)
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
                y_uj = 1
                n_holding = len(port)
                sum_sigma_ij = y_uj / n_holding * np.sum(sigma_ij)                 # :268
                y = (mu_i / gamma - 0.5 * sum_sigma_ij) / sigma_i                  # :271
            y_mv_list.append(float(y))
    return np.array(y_mv_list, np.float64)


def portfolio(port_idx, port_len, u, n_stocks):
    """The in-range entries among the first min(port_len[u], W) of row u (duplicates kept)."""
    if port_idx is None or port_idx.shape[1] == 0:
        return np.zeros(0, np.int64)
    W = port_idx.shape[1]
    n = W if port_len is None else min(max(int(port_len[u]), 0), W)
    row = np.asarray(port_idx[u, :n], np.int64)
    return row[(row >= 0) & (row < n_stocks)]


def y_matrix(returns, day_idx, cand_stock, port_idx, port_len, gamma=2.0):
    """y f64[U, I], NaN where nothing is defined (day or stock outside the tables).  y_mv is called once per distinct stock of
    a user (candidates that share a stock share their y)."""
    n_days, n_stocks, _ = returns.shape
    cand_stock = np.asarray(cand_stock, np.int64)
    U, I = len(day_idx), len(cand_stock)
    y = np.full((U, I), np.nan)
    inside = (cand_stock >= 0) & (cand_stock < n_stocks)
    uniq, inv = np.unique(cand_stock[inside], return_inverse=True)
    for u in range(U):
        d = int(day_idx[u])
        if 0 <= d < n_days and len(uniq):
            y[u, inside] = y_mv(returns, d, uniq, portfolio(port_idx, port_len, u, n_stocks), gamma)[inv]
    return y


def admissible(base, y):
    """A(u): the skip rules of ``recommend_ref.admissible`` minus the candidates without a y (NaN: stock or day outside the
    tables, or 0 / 0)."""
    return base & ~np.isnan(y)


def fuse(scores, y, adm, lam, k):
    """(top_pos i32[U,k], top_score f32[U,k], top_fused f64[U,k], n_valid i32[U], fused f64[U,I]) of a score matrix and a y
    matrix over the admissible sets ``adm``: main.py:282-286 with the average-tie rank of the SCORE in place of the positional
    n..1 (-0 == +0), then the canonical order of ``fused``; NaN in ``fused`` outside adm, empty slots -1 / -inf / -inf."""
    scores = np.asarray(scores)
    U, I = scores.shape
    top_pos = np.full((U, k), -1, np.int32)
    top_score = np.full((U, k), -np.inf, np.float32)
    top_fused = np.full((U, k), -np.inf, np.float64)
    n_valid = np.zeros(U, np.int32)
    fused = np.full((U, I), np.nan)
    for u in range(U):
        a = np.flatnonzero(adm[u])
        if not len(a):
            continue
        invest_rank = rankdata(y[u, a])                                            # :282
        tgn_rank = rankdata(scores[u, a])
        new_rank = np.array([r1 * lam + r2 * (1 - lam) for r1, r2 in zip(invest_rank, tgn_rank)])    # :286
        fused[u, a] = new_rank
        order = a[R.canonical_order(new_rank)][:k]
        n = len(order)
        top_pos[u, :n] = order
        top_score[u, :n] = scores[u, order].astype(np.float32) + np.float32(0.0)
        top_fused[u, :n] = fused[u, order]
        n_valid[u] = n
    return top_pos, top_score, top_fused, n_valid, fused


def separated_share(s64, eps, adm):
    """The share of users for whom no two admissible candidates have fp64 scores closer than the sum of their eps: no fp32
    rounding can then change the order of any two of their scores, so their rank of the score is the fp64 one."""
    U = s64.shape[0]
    clear = 0
    for u in range(U):
        a = np.flatnonzero(adm[u])
        gap = np.abs(s64[u, a][:, None] - s64[u, a][None, :]) - (eps[u, a][:, None] + eps[u, a][None, :])
        np.fill_diagonal(gap, np.inf)
        clear += int((gap > 0).all())
    return clear / max(U, 1)


def exact_returns(rs, n_days, n_stocks, n_ret):
    """f64[n_days, n_stocks, n_ret]: integers / 64, every row summing to a multiple of n_ret (see the module docstring); a
    quarter of the rows repeat another row of their day (y ties); stock 0 never moves (constant price: y = 0 / 0)."""
    v = rs.randint(-8, 9, size=(n_days, n_stocks, n_ret)).astype(np.int64)
    v[:, :, -1] -= v.sum(2) - n_ret * np.rint(v.sum(2) / n_ret).astype(np.int64)
    assert (v.sum(2) % n_ret == 0).all()
    for d in range(n_days):
        for _ in range(n_stocks // 4):
            i, j = rs.randint(1, n_stocks, size=2) if n_stocks > 1 else (0, 0)
            v[d, i] = v[d, j]
    v[:, 0, :] = 0
    return v.astype(np.float64) / 64.0


def mv_side(seed, U, I, n_ret, W=8, n_days=3, n_stocks=None, clean=False):
    """The mean-variance inputs of a case: dict(returns, cand_stock, day_idx, port_idx, port_len, gamma).  Unless ``clean``:
    the last candidate sits on the constant stock 0 (NaN y) and candidate 0 has cand_stock -1 (where I >= 3); user 1 holds
    nothing, user 2 one stock, user 3 a full row of W with a duplicate and an out-of-range entry, user 4 only out-of-range
    entries, the others 0..7 stocks with an out-of-range entry now and then; the last user's day is n_days, user 5's is -1.
    ``clean``: every candidate on a moving stock of its own day table, every day inside - no NaN y."""
    rs = np.random.RandomState(seed)
    S = n_stocks or min(I + 2, 300)
    returns = exact_returns(rs, n_days, S, n_ret)
    cand_stock = rs.randint(1, S, size=I).astype(np.int32)
    day_idx = rs.randint(0, n_days, size=U).astype(np.int32)
    port_idx = np.full((U, W), -1, np.int32)
    port_len = np.zeros(U, np.int32)
    for u in range(U):
        n = rs.randint(0, min(W, 8))                                # at most seven holdings
        port_idx[u, :n] = rs.randint(1 if clean else 0, S, size=n)
        port_len[u] = n
        if not clean and n and rs.rand() < 0.3:
            port_idx[u, rs.randint(0, n)] = S + rs.randint(0, 3)
    if clean:
        # a row that does not move on some day would be 0 / 0 there: give it one step up and one down (the sum stays)
        flat = np.flatnonzero((returns == returns[:, :, :1]).all(2))
        for f in flat:
            d, s = divmod(int(f), S)
            if s:
                returns[d, s, 0] += 1.0 / 64.0
                returns[d, s, 1] -= 1.0 / 64.0
    else:
        if I >= 3:
            cand_stock[0] = -1
            cand_stock[I - 1] = 0
        if I >= 5:
            cand_stock[2] = S + 1
        if U > 1:
            port_len[1] = 0
        if U > 2:
            port_idx[2, 0], port_len[2] = rs.randint(1, S), 1
        if U > 3:
            row = rs.randint(1, S, size=W)
            row[1] = row[0]
            row[W // 2] = S
            port_idx[3], port_len[3] = row, W + 2                   # (a length beyond the row is clamped to it)
        if U > 4:
            port_idx[4, :2], port_len[4] = (-1, S), 2
        if U > 5:
            day_idx[5] = -1
        if U > 6:
            day_idx[U - 1] = n_days
    return dict(returns=returns, cand_stock=cand_stock, day_idx=day_idx, port_idx=port_idx, port_len=port_len, gamma=2.0)


def exact_case(seed, U, I, D, k, n_t, n_ret, W=8):
    """``recommend_ref.exact_case`` (small-integer embeddings, ties, exclusions, item_ok, user 0 short of candidates, mixed
    blocks) with an exact ``mv_side`` merged in."""
    c = R.exact_case(seed, U, I, D, k, n_t)
    c.update(mv_side(seed + 7, U, I, n_ret, W))
    return c


def reference(c, lam, k, scores=None, y=None):
    """Everything the kernel returns for a case dict, from the inputs alone (or from the given score matrix): dict(top_pos,
    top_score, top_fused, n_valid, y, fused, adm, s64, y_raw).  ``y``: the ``y_raw`` of an earlier call on the same case
    (y does not depend on lambda or k)."""
    U, I = c["user_emb"].shape[0], len(c["cand_stock"])
    s64 = R.scores64(c["user_emb"], c["item_emb"], c["user_block"], I)
    if y is None:
        y = y_matrix(c["returns"], c["day_idx"], c["cand_stock"], c["port_idx"], c["port_len"], c["gamma"])
    adm = admissible(R.admissible(U, I, c.get("excl_pos"), c.get("excl_len"), c.get("item_ok")), y)
    pos, sc, fu, n, fused = fuse(s64 if scores is None else scores, y, adm, lam, k)
    return dict(top_pos=pos, top_score=sc, top_fused=fu, n_valid=n, y=np.where(adm, y, np.nan), fused=fused, adm=adm, s64=s64,
                y_raw=y)
