"""numpy reference of the group caps that count holdings (``pfo_recommend_topk_capped_held`` /
``pfo_recommend_mv_topk_capped_held`` / ``pfo_recommend_basket_topk_capped_held`` / ``TGN.recommend(held_groups=)``), on top of
``recommend_capped_ref``: the walk of the capped entry with the count of a group started from h_u(g), the number of entries of
the user's held-group row (``held_group[u, :held_len[u]]``) that name g.  A negative entry is a holding in no group and counts
for nothing; an id named twice counts twice.

Both reformulations of the capped walk carry over, stated here for the tests to hold against it:
  count form   a candidate survives iff (candidates of its own group before it in the order) + h_u(g) < cap (``survivors``);
  chunk form   the capped top-k of A u B is the capped top-k of (capped top-k of A) u B with the counts started from h_u in
               every chunk (``chunked``).
"""
import numpy as np

import recommend_ref as R
import recommend_mv_ref as M
import recommend_basket_ref as B
import recommend_capped_ref as C

# the width of the held rows of each plain case of ``recommend_capped_ref.PLAIN_CASES``
HELD_WIDTHS = {"A": 3, "B": 6, "C": 24, "E": 2, "F": 8}
# ... and of every case of ``recommend_basket_ref.CASES``, by (n_groups, cap) of ``recommend_capped_ref.MV_CAPS``
MV_HELD_WIDTH = 4


def held_rows_of(seed, U, n_groups, width):
    """The held rows of a case, drawn apart from the case's own stream and from its groups: (ids i32[U, width] with -1 behind
    the length, lens i32[U])."""
    rs = np.random.RandomState(seed + 2000)
    ids = rs.randint(-1, n_groups, (U, width)).astype(np.int32)
    lens = rs.randint(0, width + 1, U).astype(np.int32)
    ids[np.arange(width)[None, :] >= lens[:, None]] = -1
    return ids, lens


def held_counts(held_group, held_len, u):
    """h_u as a dict: group id -> the number of entries of user u's row that name it (None rows: nothing is held)."""
    if held_group is None or np.asarray(held_group).shape[1] == 0:
        return {}
    held_group = np.asarray(held_group)
    n = held_group.shape[1] if held_len is None else min(max(int(held_len[u]), 0), held_group.shape[1])
    h = {}
    for g in held_group[u, :n].tolist():
        if g >= 0:
            h[g] = h.get(g, 0) + 1
    return h


def capped_walk(order, groups, cap, k, h):
    """``recommend_capped_ref.capped_walk`` with the counts started from ``h`` (a dict, not changed)."""
    held, taken = dict(h), []
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


def survivors(order, groups, cap, h):
    """The count form: the positions of ``order`` with (members of their own group before them) + h(g) < cap, in order."""
    order = np.asarray(order, np.int64)
    g = np.asarray(groups)[order]
    before = np.array([int((g[:i] == g[i]).sum()) + h.get(int(g[i]), 0) for i in range(len(order))], np.int64)
    return order[(g < 0) | (before < cap)]


def chunked(place, positions, groups, cap, k, chunk, h):
    """The chunk form: ``recommend_capped_ref.chunked`` with the counts of every chunk started from ``h``."""
    carried = np.zeros(0, np.int64)
    positions = np.asarray(positions, np.int64)
    for lo in range(0, len(positions), chunk):
        pool = np.concatenate([carried, positions[lo:lo + chunk]])
        carried = capped_walk(pool[np.argsort(place[pool], kind="stable")], groups, cap, k, h)
    return carried


def brute_force(order, groups, cap, k, h):
    """The greedy list without a running count: a position of ``order`` is taken iff, counted afresh, the positions taken so
    far of its group plus h stay below the cap."""
    taken = []
    for c in order:
        if len(taken) == k:
            break
        g = int(groups[c])
        if g >= 0 and sum(1 for t in taken if int(groups[t]) == g) + h.get(g, 0) >= cap:
            continue
        taken.append(int(c))
    return np.array(taken, np.int64)


def n_valid_formula(adm_row, groups, cap, k, h):
    """min(k, #groupless admissible + sum over groups of min(max(cap - h(g), 0), #admissible of the group))."""
    g = np.asarray(groups)[np.flatnonzero(adm_row)]
    return min(k, int((g < 0).sum()) + sum(min(max(cap - h.get(int(v), 0), 0), int((g == v).sum())) for v in np.unique(g[g >= 0])))


def topk_capped_held(scores, adm, groups, cap, k, held_group, held_len):
    """``recommend_capped_ref.topk_capped`` under holdings: (top_pos i32[U,k], top_score f32[U,k], n_valid i32[U])."""
    scores = np.asarray(scores)
    U = scores.shape[0]
    top_pos = np.full((U, k), -1, np.int32)
    top_score = np.full((U, k), -np.inf, np.float32)
    n_valid = np.zeros(U, np.int32)
    for u in range(U):
        order = R.canonical_order(scores[u])
        took = capped_walk(order[adm[u][order]], groups, cap, k, held_counts(held_group, held_len, u))
        n = len(took)
        top_pos[u, :n] = took
        top_score[u, :n] = scores[u, took].astype(np.float32) + np.float32(0.0)
        n_valid[u] = n
    return top_pos, top_score, n_valid


def mv_capped_held(scores, y, adm, lam, groups, cap, k, held_group, held_len):
    """``recommend_capped_ref.mv_capped`` under holdings: every rank over the whole admissible set, then the walk."""
    scores = np.asarray(scores)
    U, I = scores.shape
    pos, sc, fu, n_all, fused = M.fuse(scores, y, adm, lam, I)
    out = dict(top_pos=np.full((U, k), -1, np.int32), top_score=np.full((U, k), -np.inf, np.float32),
               top_fused=np.full((U, k), -np.inf, np.float64), n_valid=np.zeros(U, np.int32), fused=fused)
    for u in range(U):
        took = capped_walk(pos[u, :n_all[u]], groups, cap, k, held_counts(held_group, held_len, u))
        n = len(took)
        at = np.array([int(np.flatnonzero(pos[u, :n_all[u]] == c)[0]) for c in took], np.int64)
        out["top_pos"][u, :n], out["top_score"][u, :n], out["top_fused"][u, :n], out["n_valid"][u] = took, sc[u, at], fu[u, at], n
    return out


def full_groups(picks, groups, cap, h):
    """bool [I]: the candidates of a group with (members among ``picks``) + h(g) >= cap - with no pick, the groups closed
    from the start."""
    groups = np.asarray(groups)
    g = groups[np.asarray(picks, np.int64)] if len(picks) else np.zeros(0, np.int64)
    full = [v for v in np.unique(groups[groups >= 0]) if int((g == v).sum()) + h.get(int(v), 0) >= cap]
    return np.isin(groups, full) & (groups >= 0)


def basket_capped_held(scores, base, returns, day_idx, cand_stock, port_idx, port_len, gamma, lam, groups, cap, k, held_group, held_len):
    """``recommend_capped_ref.basket_capped`` under holdings: the pool of round r is the skip-rule mask minus the picks minus
    every candidate of a group with picks + h_u(g) >= cap - in round 0 too.  The dict of ``recommend_basket_ref.basket``."""
    scores = np.asarray(scores)
    U, I = scores.shape
    out = dict(top_pos=np.full((U, k), -1, np.int32), top_score=np.full((U, k), -np.inf, np.float32),
               top_fused=np.full((U, k), -np.inf, np.float64), n_valid=np.zeros(U, np.int32))
    ports, plen = B.rows_with_picks(port_idx, port_len, U, k)
    h = [held_counts(held_group, held_len, u) for u in range(U)]
    pool = np.array(base, bool)
    for u in range(U):
        pool[u] &= ~full_groups([], groups, cap, h[u])
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
            pool[u] &= ~full_groups(out["top_pos"][u, :r + 1], groups, cap, h[u])
    return out


def loop_of_single_picks_capped_held(c, groups, cap, k, single, held_group, held_len):
    """What replaces the basket under holdings without it: k calls of ``single(case) -> dict(top_pos, top_score, top_fused,
    n_valid)`` at k = 1 (the UNCAPPED mean-variance entry), each pick appended to the user's portfolio row and exclusion row, and
    every candidate of a closed group - closed from the start, or by the picks - appended to the exclusion row as well."""
    U, I = c["user_emb"].shape[0], len(c["cand_stock"])
    groups = np.asarray(groups)
    port_idx, port_len = B.rows_with_picks(c.get("port_idx"), c.get("port_len"), U, k)
    excl_pos, excl_len = B.rows_with_picks(c.get("excl_pos"), c.get("excl_len"), U, k + 2 * I)
    h = [held_counts(held_group, held_len, u) for u in range(U)]
    closed = np.zeros((U, I), bool)

    def close(u, picks):
        new = full_groups(picks, groups, cap, h[u]) & ~closed[u]
        more = np.flatnonzero(new)
        excl_pos[u, excl_len[u]:excl_len[u] + len(more)] = more
        excl_len[u] += len(more)
        closed[u] |= new
    for u in range(U):
        close(u, [])
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
            excl_pos[u, excl_len[u]] = p
            excl_len[u] += 1
            close(u, out["top_pos"][u, :r + 1])
    return out


# ---- whole cases

def plain_case(name):
    """(case dict, groups, cap, k, n_t, held ids, held lens) of a plain exact case."""
    c, groups, cap, k, n_t = C.plain_case(name)
    spec, n_groups, _ = C.PLAIN_CASES[name]
    ids, lens = held_rows_of(spec[0], spec[1], n_groups, HELD_WIDTHS[name])
    return c, groups, cap, k, n_t, ids, lens


def reference_topk(c, groups, cap, k, held_group, held_len, scores=None):
    """dict(top_pos, top_score, n_valid, adm) of the plain entry under holdings, from the inputs (or a score matrix)."""
    U, I = c["user_emb"].shape[0], len(groups)
    if scores is None:
        scores = R.scores64(c["user_emb"], c["item_emb"], c["user_block"], I)
    adm = R.admissible(U, I, c.get("excl_pos"), c.get("excl_len"), c.get("item_ok"))
    pos, sc, n = topk_capped_held(scores, adm, groups, cap, k, held_group, held_len)
    return dict(top_pos=pos, top_score=sc, n_valid=n, adm=adm)


def reference_mv(c, lam, groups, cap, k, held_group, held_len, scores=None, y=None):
    """``recommend_capped_ref.reference_mv`` under holdings: dict(top_pos, top_score, top_fused, n_valid, y, fused, adm, y_raw)."""
    U, I = c["user_emb"].shape[0], len(c["cand_stock"])
    if scores is None:
        scores = R.scores64(c["user_emb"], c["item_emb"], c["user_block"], I)
    if y is None:
        y = M.y_matrix(c["returns"], c["day_idx"], c["cand_stock"], c["port_idx"], c["port_len"], c["gamma"])
    adm = M.admissible(R.admissible(U, I, c.get("excl_pos"), c.get("excl_len"), c.get("item_ok")), y)
    return dict(mv_capped_held(scores, y, adm, lam, groups, cap, k, held_group, held_len), y=np.where(adm, y, np.nan), adm=adm, y_raw=y)


def reference_basket(c, lam, groups, cap, k, held_group, held_len, scores=None):
    """``recommend_capped_ref.reference_basket`` under holdings."""
    U, I = c["user_emb"].shape[0], len(c["cand_stock"])
    if scores is None:
        scores = R.scores64(c["user_emb"], c["item_emb"], c["user_block"], I)
    base = R.admissible(U, I, c.get("excl_pos"), c.get("excl_len"), c.get("item_ok"))
    return basket_capped_held(scores, base, c["returns"], c["day_idx"], c["cand_stock"], c.get("port_idx"), c.get("port_len"), c["gamma"],
                              lam, groups, cap, k, held_group, held_len)


def conditions(c, groups, cap, k, held_group, held_len):
    """What a plain case must show before it is trusted, by the reference alone: dict(differ - users whose list differs from
    the capped list without holdings, closed - users with a group closed from the start, partial - users with 0 < h_u(g) < cap
    for some group, empty - users with an empty row)."""
    U, I = c["user_emb"].shape[0], len(groups)
    s64 = R.scores64(c["user_emb"], c["item_emb"], c["user_block"], I)
    ref = reference_topk(c, groups, cap, k, held_group, held_len, s64)
    plain = C.reference_topk(c, groups, cap, k, s64)
    h = [held_counts(held_group, held_len, u) for u in range(U)]
    return dict(differ=int((plain["top_pos"] != ref["top_pos"]).any(1).sum()), closed=sum(1 for d in h if any(v >= cap for v in d.values())),
                partial=sum(1 for d in h if any(0 < v < cap for v in d.values())), empty=int((np.asarray(held_len) == 0).sum()))
