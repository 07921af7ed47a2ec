"""numpy reference of the group caps (``pfo_recommend_topk_capped`` / ``pfo_recommend_mv_topk_capped`` /
``pfo_recommend_basket_topk_capped`` / ``TGN.recommend(groups=, group_cap=)``), on top of ``recommend_ref``, ``recommend_mv_ref``
and ``recommend_basket_ref``: the canonical order of the uncapped entry, walked with a candidate skipped once its group holds
``cap`` picks.  A group id is any non-negative integer; a negative one puts the candidate in no group and it is never capped.

The walk has two exact reformulations the kernels rest on, stated here for the tests to hold against it:
  count form   a candidate survives iff fewer than ``cap`` candidates of its own group stand before it in the order; the capped
               list is the first k survivors (``survivors``);
  chunk form   the capped top-k of A u B is the capped top-k of (capped top-k of A) u B, so the order may be walked a chunk of
               candidates at a time with the list carried along and the counts started from zero in every chunk (``chunked``).
"""
import numpy as np

import recommend_ref as R
import recommend_mv_ref as M
import recommend_basket_ref as B

# exact_case(seed, U, I, D, k, n_t) of recommend_ref with (n_groups, cap): the plain cases of the GPU test, by name
PLAIN_CASES = {"A": ((3, 20, 40, 32, 4, 1), 3, 1), "B": ((4, 37, 600, 32, 16, 3), 5, 2), "C": ((5, 20, 1100, 172, 64, 1), 40, 1),
               "E": ((7, 9, 12, 32, 16, 1), 2, 2), "F": ((8, 33, 513, 64, 10, 2), 11, 1)}
# (n_groups, cap) every case of recommend_basket_ref.CASES runs at, in the mean-variance order and as a basket
MV_CAPS = ((3, 1), (8, 2))


def groups_of(seed, I, n_groups):
    """The group ids of a case: -1 (no group) and 0 .. n_groups - 1, drawn apart from the case's own stream."""
    return np.random.RandomState(seed + 1000).randint(-1, n_groups, I).astype(np.int32)


def capped_walk(order, groups, cap, k):
    """The first k positions of ``order`` taken greedily: a position is skipped when its group is >= 0 and already holds
    ``cap`` of the positions taken."""
    held, taken = {}, []
    for c in order:
        if len(taken) == k:
            break
        g = int(groups[c])
        if g >= 0:
            if held.get(g, 0) >= cap:
                continue
            held[g] = held.get(g, 0) + 1
        taken.append(int(c))
    return np.array(taken, np.int64)


def survivors(order, groups, cap):
    """The count form: the positions of ``order`` with fewer than ``cap`` members of their own group before them, in order."""
    order = np.asarray(order, np.int64)
    g = np.asarray(groups)[order]
    before = np.array([int((g[:i] == g[i]).sum()) for i in range(len(order))], np.int64)
    return order[(g < 0) | (before < cap)]


def chunked(place, positions, groups, cap, k, chunk):
    """The chunk form: ``positions`` (any order) taken ``chunk`` at a time; the list carried from the chunks before and the
    chunk's own positions are put in the canonical order (``place[c]``: the place of c in it, smaller = earlier) and walked
    with counts that start from zero."""
    carried = np.zeros(0, np.int64)
    positions = np.asarray(positions, np.int64)
    for lo in range(0, len(positions), chunk):
        pool = np.concatenate([carried, positions[lo:lo + chunk]])
        carried = capped_walk(pool[np.argsort(place[pool], kind="stable")], groups, cap, k)
    return carried


def n_valid_formula(adm_row, groups, cap, k):
    """min(k, #groupless admissible + sum over groups of min(cap, #admissible of the group))."""
    g = np.asarray(groups)[np.flatnonzero(adm_row)]
    return min(k, int((g < 0).sum()) + sum(min(cap, int((g == v).sum())) for v in np.unique(g[g >= 0])))


def topk_capped(scores, adm, groups, cap, k):
    """``recommend_ref.topk`` under the cap: (top_pos i32[U,k], top_score f32[U,k], n_valid i32[U])."""
    scores = np.asarray(scores)
    U = scores.shape[0]
    top_pos = np.full((U, k), -1, np.int32)
    top_score = np.full((U, k), -np.inf, np.float32)
    n_valid = np.zeros(U, np.int32)
    for u in range(U):
        order = R.canonical_order(scores[u])
        took = capped_walk(order[adm[u][order]], groups, cap, k)
        n = len(took)
        top_pos[u, :n] = took
        top_score[u, :n] = scores[u, took].astype(np.float32) + np.float32(0.0)
        n_valid[u] = n
    return top_pos, top_score, n_valid


def mv_capped(scores, y, adm, lam, groups, cap, k):
    """``recommend_mv_ref.fuse`` at the full depth (every rank over the whole admissible set), then the walk: dict(top_pos,
    top_score, top_fused, n_valid, fused) - ``fused`` f64[U,I] the uncapped values, NaN outside ``adm``."""
    scores = np.asarray(scores)
    U, I = scores.shape
    pos, sc, fu, n_all, fused = M.fuse(scores, y, adm, lam, I)
    out = dict(top_pos=np.full((U, k), -1, np.int32), top_score=np.full((U, k), -np.inf, np.float32),
               top_fused=np.full((U, k), -np.inf, np.float64), n_valid=np.zeros(U, np.int32), fused=fused)
    for u in range(U):
        took = capped_walk(pos[u, :n_all[u]], groups, cap, k)
        n = len(took)
        at = np.array([int(np.flatnonzero(pos[u, :n_all[u]] == c)[0]) for c in took], np.int64)
        out["top_pos"][u, :n], out["top_score"][u, :n], out["top_fused"][u, :n], out["n_valid"][u] = took, sc[u, at], fu[u, at], n
    return out


def _full_groups(picks, groups, cap):
    """bool [I]: the candidates of a group that holds ``cap`` of ``picks``."""
    groups = np.asarray(groups)
    g = groups[np.asarray(picks, np.int64)] if len(picks) else np.zeros(0, np.int64)
    full = [v for v in np.unique(g[g >= 0]) if int((g == v).sum()) >= cap]
    return np.isin(groups, full) & (groups >= 0)


def basket_capped(scores, base, returns, day_idx, cand_stock, port_idx, port_len, gamma, lam, groups, cap, k):
    """``recommend_basket_ref.basket`` with full groups leaving the pool: round r is one round of it (k = 1) over the skip-rule
    mask minus the picks minus every candidate of a full group, the picks' stocks behind the portfolio.  The dict of ``basket``."""
    scores = np.asarray(scores)
    U, I = scores.shape
    out = dict(top_pos=np.full((U, k), -1, np.int32), top_score=np.full((U, k), -np.inf, np.float32),
               top_fused=np.full((U, k), -np.inf, np.float64), n_valid=np.zeros(U, np.int32))
    ports, plen = B.rows_with_picks(port_idx, port_len, U, k)
    pool = np.array(base, bool)
    live = np.ones(U, bool)
    for r in range(k):
        one = B.basket(scores, pool, returns, day_idx, cand_stock, ports, plen, gamma, lam, 1)
        live &= one["n_valid"] == 1                                     # a list that has ended stays ended
        for u in np.flatnonzero(live):
            p = int(one["top_pos"][u, 0])
            out["top_pos"][u, r], out["top_score"][u, r], out["top_fused"][u, r] = p, one["top_score"][u, 0], one["top_fused"][u, 0]
            out["n_valid"][u] = r + 1
            ports[u, plen[u]] = cand_stock[p]
            plen[u] += 1
            pool[u, p] = False
            pool[u] &= ~_full_groups(out["top_pos"][u, :r + 1], groups, cap)
    return out


def loop_of_single_picks_capped(c, groups, cap, k, single):
    """What replaces the capped basket without it: k calls of ``single(case) -> dict(top_pos, top_score, top_fused, n_valid)``
    at k = 1 (the UNCAPPED mean-variance entry), each pick appended to the user's portfolio row and exclusion row - and, once the
    pick's group is full, every other candidate of that group appended to the exclusion row as well."""
    U, I = c["user_emb"].shape[0], len(c["cand_stock"])
    groups = np.asarray(groups)
    port_idx, port_len = B.rows_with_picks(c.get("port_idx"), c.get("port_len"), U, k)
    excl_pos, excl_len = B.rows_with_picks(c.get("excl_pos"), c.get("excl_len"), U, k + I)
    out = dict(top_pos=np.full((U, k), -1, np.int32), top_score=np.full((U, k), -np.inf, np.float32),
               top_fused=np.full((U, k), -np.inf, np.float64), n_valid=np.zeros(U, np.int32))
    live = np.ones(U, bool)
    for r in range(k):
        one = single(dict(c, port_idx=port_idx, port_len=port_len, excl_pos=excl_pos, excl_len=excl_len))
        live &= one["n_valid"] == 1
        for u in np.flatnonzero(live):
            p = int(one["top_pos"][u, 0])
            out["top_pos"][u, r], out["top_score"][u, r], out["top_fused"][u, r] = p, one["top_score"][u, 0], one["top_fused"][u, 0]
            out["n_valid"][u] = r + 1
            port_idx[u, port_len[u]] = c["cand_stock"][p]
            port_len[u] += 1
            more = [p]
            g = int(groups[p])
            if g >= 0 and int((groups[out["top_pos"][u, :r + 1]] == g).sum()) == cap:
                more += [int(j) for j in np.flatnonzero(groups == g) if j != p]
            excl_pos[u, excl_len[u]:excl_len[u] + len(more)] = more
            excl_len[u] += len(more)
    return out


# ---- whole cases

def plain_case(name):
    """(case dict, groups, cap, k, n_t) of a plain exact case."""
    spec, n_groups, cap = PLAIN_CASES[name]
    return R.exact_case(*spec), groups_of(spec[0], spec[2], n_groups), cap, spec[4], spec[5]


def reference_topk(c, groups, cap, k, scores=None):
    """dict(top_pos, top_score, n_valid, adm) of the plain capped entry for a case dict, from the inputs (or a score matrix)."""
    U, I = c["user_emb"].shape[0], len(groups)
    if scores is None:
        scores = R.scores64(c["user_emb"], c["item_emb"], c["user_block"], I)
    adm = R.admissible(U, I, c.get("excl_pos"), c.get("excl_len"), c.get("item_ok"))
    pos, sc, n = topk_capped(scores, adm, groups, cap, k)
    return dict(top_pos=pos, top_score=sc, n_valid=n, adm=adm)


def reference_mv(c, lam, groups, cap, k, scores=None, y=None):
    """``recommend_mv_ref.reference`` under the cap: dict(top_pos, top_score, top_fused, n_valid, y, fused, adm, y_raw)."""
    U, I = c["user_emb"].shape[0], len(c["cand_stock"])
    if scores is None:
        scores = R.scores64(c["user_emb"], c["item_emb"], c["user_block"], I)
    if y is None:
        y = M.y_matrix(c["returns"], c["day_idx"], c["cand_stock"], c["port_idx"], c["port_len"], c["gamma"])
    adm = M.admissible(R.admissible(U, I, c.get("excl_pos"), c.get("excl_len"), c.get("item_ok")), y)
    return dict(mv_capped(scores, y, adm, lam, groups, cap, k), y=np.where(adm, y, np.nan), adm=adm, y_raw=y)


def reference_basket(c, lam, groups, cap, k, scores=None):
    """``recommend_basket_ref.reference`` under the cap."""
    U, I = c["user_emb"].shape[0], len(c["cand_stock"])
    if scores is None:
        scores = R.scores64(c["user_emb"], c["item_emb"], c["user_block"], I)
    base = R.admissible(U, I, c.get("excl_pos"), c.get("excl_len"), c.get("item_ok"))
    return basket_capped(scores, base, c["returns"], c["day_idx"], c["cand_stock"], c.get("port_idx"), c.get("port_len"), c["gamma"],
                         lam, groups, cap, k)


def binding(c, groups, cap, k):
    """(users whose capped list differs from the uncapped one, users whose capped list ends short of min(k, #admissible)) of a
    plain case, by the reference alone."""
    U, I = c["user_emb"].shape[0], len(groups)
    s64 = R.scores64(c["user_emb"], c["item_emb"], c["user_block"], I)
    ref = reference_topk(c, groups, cap, k, s64)
    pos, _, n = R.topk(s64, ref["adm"], k)
    return int((pos != ref["top_pos"]).any(1).sum()), int((ref["n_valid"] < n).sum())
