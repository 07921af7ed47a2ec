"""numpy reference of the basket top-k (``pfo_recommend_basket_topk`` / ``TGN.recommend(mv=..., basket=True)``): the list of
``recommend_mv_ref`` taken one pick at a time.  Round r ranks the admissible candidates that have not been picked against the
portfolio followed by the stocks of picks 0 .. r-1 (``recommend_mv_ref.y_mv`` / ``fuse``: the reference project's own numpy and
scipy calls), takes the first of the canonical order, and reports that pick's position, score and fused value of round r.  Only
the picked position leaves the pool; the picked stock joins the portfolio even if it is held already; a NaN y sits out its round
only; the list ends when nobody takes part.

Exactness: ``y_mv`` adds the covariances with ``np.sum``, pairwise from eight terms on, the kernel in list order.  A case
therefore either keeps holdings + k - 1 <= 7, or has n_ret - 1 a power of two: the covariances of ``exact_returns`` are then
exact dyadic numbers and their sum is exact in any order.  ``CASES`` keep to that (n_ret = 29: W = 4, which ``mv_side`` turns
into at most 3 in-range holdings, and k <= 4)."""
import numpy as np

import recommend_ref as R
import recommend_mv_ref as M

# exact_case(seed, U, I, D, k, n_t, n_ret, W); the last has k > I for every user and ends early
CASES = [(3, 20, 40, 32, 4, 1, 29, 4), (4, 37, 40, 32, 4, 3, 29, 4), (5, 20, 70, 32, 16, 1, 17, 8), (6, 17, 300, 32, 8, 3, 33, 8),
         (7, 9, 12, 32, 16, 1, 5, 8)]
LAMBDAS = (0.0, 0.5, 1.0)


def case(spec):
    seed, U, I, D, k, n_t, n_ret, W = spec
    return M.exact_case(seed, U, I, D, k, n_t, n_ret, W)


def basket(scores, base, returns, day_idx, cand_stock, port_idx, port_len, gamma, lam, k):
    """The rounds over a score matrix [U, I] and the skip-rule mask ``base`` [U, I] (``recommend_ref.admissible``):
    dict(top_pos i32[U,k], top_score f32[U,k], top_fused f64[U,k], n_valid i32[U]); empty slots -1 / -inf / -inf."""
    scores = np.asarray(scores)
    U, I = scores.shape
    n_days, n_stocks, _ = returns.shape
    cand_stock = np.asarray(cand_stock, np.int64)
    inside = (cand_stock >= 0) & (cand_stock < n_stocks)
    uniq, inv = np.unique(cand_stock[inside], return_inverse=True)      # candidates that share a stock share their y
    top_pos = np.full((U, k), -1, np.int32)
    top_score = np.full((U, k), -np.inf, np.float32)
    top_fused = np.full((U, k), -np.inf, np.float64)
    n_valid = np.zeros(U, np.int32)
    for u in range(U):
        d = int(day_idx[u])
        if not (0 <= d < n_days and len(uniq)):
            continue                                                    # a day outside the tables: an empty list
        port = [int(s) for s in M.portfolio(port_idx, port_len, u, n_stocks)]
        taken = np.zeros(I, bool)
        for r in range(k):
            y = np.full(I, np.nan)
            y[inside] = M.y_mv(returns, d, uniq, port, gamma)[inv]
            adm = M.admissible(base[u] & ~taken, y)[None]
            pos, sc, fu, n, _ = M.fuse(scores[u][None], y[None], adm, lam, 1)
            if n[0] == 0:
                break
            p = int(pos[0, 0])
            top_pos[u, r], top_score[u, r], top_fused[u, r] = p, sc[0, 0], fu[0, 0]
            n_valid[u] = r + 1
            taken[p] = True
            port.append(int(cand_stock[p]))
    return dict(top_pos=top_pos, top_score=top_score, top_fused=top_fused, n_valid=n_valid)


def reference(c, lam, k, scores=None):
    """Everything the kernel returns for a case dict (``recommend_mv_ref.exact_case`` and the like), from the inputs alone or
    from the given score matrix."""
    U, I = c["user_emb"].shape[0], len(c["cand_stock"])
    if scores is None:
        scores = R.scores64(c["user_emb"], c["item_emb"], c["user_block"], I)
    base = R.admissible(U, I, c.get("excl_pos"), c.get("excl_len"), c.get("item_ok"))
    return basket(scores, base, c["returns"], c["day_idx"], c["cand_stock"], c.get("port_idx"), c.get("port_len"), c["gamma"], lam, k)


def rows_with_picks(rows, lens, U, k):
    """(rows [U, W + k], lens [U]) with k free slots behind the entries in use: the row a caller of the k = 1 loop appends its
    picks to.  ``rows`` None: no entries; ``lens`` None: whole rows."""
    W = 0 if rows is None else rows.shape[1]
    out = np.full((U, W + k), -1, np.int32)
    n = np.zeros(U, np.int32) if rows is None else (np.full(U, W, np.int32) if lens is None else np.clip(lens, 0, W).astype(np.int32))
    for u in range(U):
        out[u, :n[u]] = rows[u, :n[u]]
    return out, n


def loop_of_single_picks(c, k, single):
    """What a caller does today: k calls of ``single(case) -> dict(top_pos, top_score, top_fused, n_valid)`` at k = 1, each
    pick appended to the user's portfolio row (its stock) and exclusion row (its position).  The same dict as ``reference``."""
    U = c["user_emb"].shape[0]
    port_idx, port_len = rows_with_picks(c.get("port_idx"), c.get("port_len"), U, k)
    excl_pos, excl_len = rows_with_picks(c.get("excl_pos"), c.get("excl_len"), U, k)
    top_pos = np.full((U, k), -1, np.int32)
    top_score = np.full((U, k), -np.inf, np.float32)
    top_fused = np.full((U, k), -np.inf, np.float64)
    n_valid = np.zeros(U, np.int32)
    live = np.ones(U, bool)
    for r in range(k):
        one = single(dict(c, port_idx=port_idx, port_len=port_len, excl_pos=excl_pos, excl_len=excl_len))
        live &= one["n_valid"] == 1                                     # a list that has ended stays ended
        for u in np.flatnonzero(live):
            p = int(one["top_pos"][u, 0])
            top_pos[u, r], top_score[u, r], top_fused[u, r] = p, one["top_score"][u, 0], one["top_fused"][u, 0]
            n_valid[u] = r + 1
            port_idx[u, port_len[u]] = c["cand_stock"][p]
            port_len[u] += 1
            excl_pos[u, excl_len[u]] = p
            excl_len[u] += 1
    return dict(top_pos=top_pos, top_score=top_score, top_fused=top_fused, n_valid=n_valid)


def same(a, b):
    """All four outputs equal (the score compared as bits: -0 and +0 differ)."""
    return (np.array_equal(a["top_pos"], b["top_pos"]) and np.array_equal(a["n_valid"], b["n_valid"])
            and np.array_equal(np.asarray(a["top_score"]).view(np.int32), np.asarray(b["top_score"]).view(np.int32))
            and np.array_equal(a["top_fused"], b["top_fused"]))
