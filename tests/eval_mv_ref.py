"""numpy reference of the evaluation row ranked in a served order (``pfo_eval_metrics_mv`` / ``eval_recommendation(order=)``),
composed from what the served orders are already held to, one interaction at a time as a one-user case:
``recommend_mv_ref.y_matrix`` (``y_mv`` / ``portfolio``) and ``fuse`` for the fused list (mode 0),
``recommend_basket_ref.basket`` with k = 5 for the basket (mode 1), ``finance_ref.invest_metrics`` for the twelve investment values
of the resulting top-5.  It takes a score matrix, as ``recommend_mv_ref.reference(..., scores=)`` does.

Exactness follows the two modules' own rules: small-integer embeddings (every fp32 score exact), ``exact_returns`` tables for
the order (every mean and covariance exact), at most 7 holdings in mode 0; in mode 1 holdings + 4 <= 7, or mv_ret - 1 a power of
two.  The investment values are NOT exact - they are held to ``finance_ref.invest_bar``."""
import warnings

import numpy as np

import finance_ref as F
import recommend_ref as R
import recommend_mv_ref as M
import recommend_basket_ref as BK

RANK_NONE = (1 << 31) - 1


def scores64(emb, B, n_neg):
    """fp64 scores [B, 1 + n_neg] of emb = [src B | dst B | neg B * n_neg]."""
    e = np.asarray(emb, np.float64)
    src, dst, neg = e[:B], e[B:2 * B], e[2 * B:].reshape(B, n_neg, -1)
    return np.concatenate([(src * dst).sum(1)[:, None], np.einsum("bd,bkd->bk", src, neg)], 1)


def dot_error_bound(emb, B, n_neg):
    """``recommend_ref.dot_error_bound`` for the rows of an evaluation batch: gamma_D * sum_d |u_d v_d|, [B, 1 + n_neg]."""
    e = np.abs(np.asarray(emb, np.float64))
    D = e.shape[1]
    gamma = D * 2.0 ** -24 / (1.0 - D * 2.0 ** -24)
    return gamma * scores64(e, B, n_neg)


def invest_port(c, b):
    """The portfolio of row b as the investment stage takes it: the first min(port_len, W) entries, or None when one of them
    lies outside the investment tables (the row's twelve values are NaN then)."""
    W = c["port_idx"].shape[1]
    n = min(int(c["port_len"][b]), W)
    row = np.asarray(c["port_idx"][b, :max(n, 0)], np.int64)
    if ((row < 0) | (row >= c["ret_past"].shape[1])).any():
        return None
    return row


def invest_rows(c, top5_item, dtype=np.float64):
    """(invest [B, 12], scale [B, 12]) of the given top-5 node ids (-1 = empty slot) - ``finance_ref.invest_metrics`` per row."""
    B = top5_item.shape[0]
    out, scale = np.full((B, 12), np.nan, dtype), np.full((B, 12), np.nan, dtype)
    for b in range(B):
        port = invest_port(c, b)
        if port is None:
            continue
        d = int(c["day_idx"][b])
        items = top5_item[b][top5_item[b] >= 0].astype(np.int64) - c["upper_u"] - 1
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)         # (no holding and no pick: the mean of no rows, NaN on both sides)
            out[b], scale[b] = F.invest_metrics(c["ret_past"][d], c["ret_future"][d], port, items, dtype=dtype, parts=True)
    return out, scale


def reference(c, lam, mode, scores):
    """Everything the kernel returns for a case dict - cand i32[B, 1+n_neg], upper_u, day_idx, port_idx, port_len, ret_past,
    ret_future, ret_mv, mv_day_idx, gamma - and a score matrix [B, 1+n_neg]: dict(rank, top5_pos, top5_item, top5_fused, n_adm,
    y, fused, adm, invest, invest_scale); y / fused NaN outside A(b), fused round 0's in mode 1."""
    scores = np.asarray(scores)
    B, n_cand = scores.shape
    ret_mv = c["ret_mv"]
    rank = np.full(B, RANK_NONE, np.int32)
    top5_pos = np.full((B, 5), -1, np.int32)
    top5_fused = np.full((B, 5), -np.inf)
    n_adm = np.zeros(B, np.int32)
    y_all, fused_all = np.full((B, n_cand), np.nan), np.full((B, n_cand), np.nan)
    for b in range(B):
        stock = np.asarray(c["cand"][b], np.int64) - c["upper_u"] - 1
        day, pi, pl = c["mv_day_idx"][b:b + 1], c["port_idx"][b:b + 1], c["port_len"][b:b + 1]
        y = M.y_matrix(ret_mv, day, stock, pi, pl, c["gamma"])
        adm = M.admissible(np.ones((1, n_cand), bool), y)
        n_adm[b] = adm.sum()
        pos, _, fu, _, fused = M.fuse(scores[b][None], y, adm, lam, 5)
        y_all[b], fused_all[b] = np.where(adm[0], y[0], np.nan), fused[0]
        if mode == 0:
            top5_pos[b], top5_fused[b] = pos[0], fu[0]
            if adm[0, 0]:
                a = np.flatnonzero(adm[0])
                rank[b] = int(np.flatnonzero(a[R.canonical_order(fused[0, a])] == 0)[0])
        else:
            r = BK.basket(scores[b][None], np.ones((1, n_cand), bool), ret_mv, day, stock, pi, pl, c["gamma"], lam, 5)
            top5_pos[b], top5_fused[b] = r["top_pos"][0], r["top_fused"][0]
            at = np.flatnonzero(top5_pos[b] == 0)
            if adm[0, 0] and len(at):
                rank[b] = int(at[0])
    top5_item = np.where(top5_pos >= 0, np.take_along_axis(np.asarray(c["cand"]), np.maximum(top5_pos, 0), 1), -1).astype(np.int32)
    invest, scale = invest_rows(c, top5_item)
    return dict(rank=rank, top5_pos=top5_pos, top5_item=top5_item, top5_fused=top5_fused, n_adm=n_adm, y=y_all, fused=fused_all,
                adm=~np.isnan(y_all), invest=invest, invest_scale=scale)


def rows(c, sel):
    """The case restricted to the interactions ``sel`` (a list of row numbers), the tables shared."""
    sel = np.asarray(sel, np.int64)
    B, n_neg = c["B"], c["n_neg"]
    emb = np.asarray(c["emb"])
    neg = emb[2 * B:].reshape(B, n_neg, -1)
    out = dict(c, B=len(sel), emb=np.concatenate([emb[sel], emb[B + sel], neg[sel].reshape(len(sel) * n_neg, -1)]))
    for k in ("cand", "day_idx", "port_idx", "port_len", "mv_day_idx"):
        out[k] = np.asarray(c[k])[sel].copy()
    return out


def loop_of_single_picks(c, lam, scores):
    """The basket as a caller of mode 0 would build it: five rounds of the fused list's first pick, the pick's stock appended
    to the portfolio row and its position taken out of the candidates (moved to a stock outside the order table).
    (top5_pos i32[B,5], top5_fused f64[B,5]) - what mode 1 returns."""
    B = c["B"]
    W = c["port_idx"].shape[1]
    port_idx = np.concatenate([c["port_idx"], np.full((B, 5), -1, np.int32)], 1)
    port_len = np.clip(c["port_len"], 0, W).astype(np.int32)
    cand = np.array(c["cand"])
    gone = c["upper_u"] + 1 + c["ret_mv"].shape[1]                  # the first stock outside the order table
    top5_pos, top5_fused = np.full((B, 5), -1, np.int32), np.full((B, 5), -np.inf)
    for b in range(B):
        for r in range(5):
            one = rows(dict(c, port_idx=port_idx, port_len=port_len, cand=cand), [b])
            one["port_idx"][0, :port_len[b]] = port_idx[b, :port_len[b]]
            ref = reference(one, lam, 0, scores[b:b + 1])
            p = int(ref["top5_pos"][0, 0])
            if p < 0:
                break
            top5_pos[b, r], top5_fused[b, r] = p, ref["top5_fused"][0, 0]
            port_idx[b, port_len[b]] = c["cand"][b, p] - c["upper_u"] - 1
            port_len[b] += 1
            cand[b, p] = gone
    return top5_pos, top5_fused


def hits_ndcg(rank):
    """(recall f32[B,3], ndcg f64[B,3]) at k = 1, 3, 5 of a rank vector; RANK_NONE is a miss at every k."""
    rank = np.asarray(rank, np.int64)
    hit = np.stack([rank < k for k in (1, 3, 5)], 1)
    with np.errstate(all="ignore"):
        return hit.astype(np.float32), np.where(hit, 1.0 / np.log2(rank[:, None] + 2.0), 0.0)


# ---- cases

def _tables(rs, n_days, S, n_ret):
    """Investment tables of S stocks: ordinary fp64 log-returns (nothing about them is exact)."""
    return rs.randn(n_days, S, n_ret) * 0.01, rs.randn(n_days, S, n_ret) * 0.01


def exact_case(seed, B, n_neg, D, mv_ret, W, n_ret=29, mv_stocks=24, special=True):
    """Small-integer embeddings (a third of an interaction's negatives repeat another: score ties) over an ``exact_returns``
    order table of ``mv_stocks`` stocks (stock 0 never moves: y = 0 / 0; a quarter of the rows repeat another: y ties) and
    investment tables of mv_stocks + 3 stocks, so a stock can lie outside the order table and inside the investment tables.
    Portfolios hold 0 .. min(W, 8) - 1 stocks.  ``special`` (B >= 14, n_neg >= 8) makes rows
      0  the positive on the constant stock          1  the positive's stock outside ret_mv
      2  mv_day_idx = -1                             3  mv_day_idx = mv_days
      4  an empty portfolio                          5  a portfolio of entries outside ret_mv only (inside the investment tables)
      6  a portfolio of -1 and an entry outside every table (the investment values are NaN)
      7  a full portfolio row with a duplicate       8  every candidate inadmissible
      9  exactly 3 admissible candidates            10  exactly 5
     11  all negatives one candidate (same embedding, same stock): y and score ties straddling position 5
     12  eight negatives of one embedding on different stocks (score ties)    13  eight on one stock (y ties)."""
    rs = np.random.RandomState(seed)
    n_cand, mv_days, n_days, S, U = 1 + n_neg, 3, 4, mv_stocks + 3, 1000
    emb = rs.randint(-3, 4, size=(B * (2 + n_neg), D)).astype(np.float32)
    neg = emb[2 * B:].reshape(B, n_neg, D)
    for b in range(B):
        for _ in range(n_neg // 3):
            i, j = rs.randint(0, n_neg, size=2)
            neg[b, i] = neg[b, j]
    stock = rs.randint(1, mv_stocks, size=(B, n_cand))
    ret_mv = M.exact_returns(rs, mv_days, mv_stocks, mv_ret)
    ret_past, ret_future = _tables(rs, n_days, S, n_ret)
    mv_day = rs.randint(0, mv_days, size=B).astype(np.int32)
    day = rs.randint(0, n_days, size=B).astype(np.int32)
    port_idx = np.full((B, W), -1, np.int32)
    port_len = np.zeros(B, np.int32)
    for b in range(B):
        n = rs.randint(0, min(W, 8))
        port_idx[b, :n] = rs.randint(0, mv_stocks, size=n)
        port_len[b] = n
    if special:
        assert B >= 14 and n_neg >= 8
        stock[0, 0] = 0
        stock[1, 0] = mv_stocks + 1
        mv_day[2], mv_day[3] = -1, mv_days
        port_len[4] = 0
        port_idx[5, :2], port_len[5] = (mv_stocks, mv_stocks + 2), 2
        port_idx[6, :2], port_len[6] = (-1, S + 2), 2
        row = rs.randint(1, mv_stocks, size=W)
        row[1] = row[0]
        port_idx[7], port_len[7] = row, W + 2                       # (a length beyond the row is clamped to it)
        stock[8] = np.where(rs.rand(n_cand) < 0.5, 0, mv_stocks + rs.randint(0, 3, size=n_cand))
        for b, n in ((9, 3), (10, 5)):
            keep = rs.permutation(n_cand)[:n]
            out = np.ones(n_cand, bool)
            out[keep] = False
            stock[b, out] = 0
        neg[11, :] = neg[11, 0]
        stock[11, 1:] = stock[11, 1]
        neg[12, :8] = neg[12, 0]
        stock[12, 1:9] = rs.permutation(np.arange(1, mv_stocks))[:8]
        stock[13, 1:9] = stock[13, 1]
        # the rows that count their admissible candidates must not lose one to a day's constant copy
        for b in (9, 10):
            mv_day[b] = 0
    cand = (stock + U + 1).astype(np.int32)
    return dict(emb=np.ascontiguousarray(emb), B=B, n_neg=n_neg, cand=cand, upper_u=U, day_idx=day, port_idx=port_idx, port_len=port_len,
                ret_past=ret_past, ret_future=ret_future, ret_mv=ret_mv, mv_day_idx=mv_day, gamma=2.0)


def clean_case(seed, B, n_neg, D, n_ret, mv_ret, normal=True):
    """Random normal (or small-integer) embeddings with a clean order side: every candidate on a moving stock of its day (no
    NaN y), every day inside, portfolios of 0..7 moving stocks; the investment tables hold the same stocks."""
    rs = np.random.RandomState(seed)
    m = M.mv_side(seed + 3, B, 1 + n_neg, mv_ret, n_stocks=40, clean=True)
    S, U = m["returns"].shape[1], 1000
    emb = rs.randn(B * (2 + n_neg), D).astype(np.float32) if normal else rs.randint(-3, 4, size=(B * (2 + n_neg), D)).astype(np.float32)
    stock = rs.randint(1, S, size=(B, 1 + n_neg))
    ret_past, ret_future = _tables(rs, 3, S, n_ret)
    return dict(emb=emb, B=B, n_neg=n_neg, cand=(stock + U + 1).astype(np.int32), upper_u=U, day_idx=rs.randint(0, 3, size=B).astype(np.int32),
                port_idx=m["port_idx"], port_len=m["port_len"], ret_past=ret_past, ret_future=ret_future, ret_mv=m["returns"],
                mv_day_idx=m["day_idx"], gamma=2.0)


# (seed, B, n_neg, D, mv_ret, W): the first carries the special rows - mv_ret - 1 a power of two, so up to eight holdings plus four
# picks stay exact; the second puts two candidates on most threads (1 + n_neg > 256) with at most 3 holdings at mv_ret = 29
EXACT_CASES = [(31, 18, 20, 32, 17, 8), (32, 4, 300, 32, 29, 4)]
# smaller ones for the host-side identities (holdings + 4 <= 7 at mv_ret = 10; mv_ret - 1 a power of two otherwise)
SMALL_CASES = [(33, 6, 9, 8, 9, 8), (34, 5, 12, 16, 10, 4), (35, 3, 40, 32, 33, 8)]
LAMBDAS = (0.0, 0.5, 1.0)


def case(spec):
    seed, B, n_neg, D, mv_ret, W = spec
    return exact_case(seed, B, n_neg, D, mv_ret, W, special=B >= 14)
