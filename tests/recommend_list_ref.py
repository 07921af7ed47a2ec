"""numpy reference of the list forms of the top-k recommendation (``pfo_recommend_list_topk`` / ``pfo_recommend_list_mv_topk`` /
``TGN.recommend(only=...)``): the admissible set of a user's OWN list, then ``recommend_ref.topk`` / ``recommend_mv_ref.fuse``
over it - the shared-list references with another admissible set, nothing else.  No import of the package."""
import numpy as np

import recommend_ref as R
import recommend_mv_ref as M


# (seed, U, I, D, W, k, n_t) of the tests on random normal embeddings (``normal_list_case``): tests/test_recommend_list_cpu.py
# computes, from the inputs alone, the share of users ``recommend_ref.check_topk`` pins for each
NORMAL_CASES = [(1, 67, 300, 32, 8, 10, 1), (2, 67, 300, 172, 64, 10, 3), (3, 130, 1000, 172, 256, 64, 1), (4, 33, 17, 256, 65, 1, 2),
                (5, 67, 300, 4, 64, 10, 1)]


def normal_list_case(seed, U, I, D, W, n_t):
    return list_case(R.normal_case(seed, U, I, D, n_t), seed, W)


def list_rows(list_pos, list_len, u):
    """The entries of row u that count: the first min(max(list_len[u], 0), list_stride)."""
    W = list_pos.shape[1]
    n = W if list_len is None else min(max(int(list_len[u]), 0), W)
    return np.asarray(list_pos[u, :n], np.int64)


def admissible_list(U, I, list_pos, list_len=None, item_ok=None):
    """bool [U, I]: position p may be offered to user u - p is among the entries of row u that count, 0 <= p < I, and
    item_ok[p] != 0.  A set: naming a position twice changes nothing."""
    adm = np.zeros((U, I), bool)
    for u in range(U):
        row = list_rows(list_pos, list_len, u)
        adm[u, row[(row >= 0) & (row < I)]] = True
    if item_ok is not None:
        adm &= (np.asarray(item_ok) != 0)[None, :]
    return adm


def complement(U, I, list_pos, list_len=None):
    """(excl_pos i32[U, I], excl_len i32[U]): every position a user's list does NOT name - the exclusion list that says the same
    to the shared-list kernels."""
    named = admissible_list(U, I, list_pos, list_len)
    excl_pos = np.full((U, max(I, 1)), -1, np.int32)
    excl_len = np.zeros(U, np.int32)
    for u in range(U):
        rest = np.flatnonzero(~named[u])
        excl_pos[u, :len(rest)] = rest
        excl_len[u] = len(rest)
    return excl_pos, excl_len


def list_case(base, seed, W):
    """A case of ``recommend_ref`` / ``recommend_mv_ref`` with per-user lists of stride W added (``list_pos`` i32[U, W] padded
    with -1, ``list_len`` i32[U]) and its exclusion lists taken out: rows of 0..W entries from [-1, I + 1] - the -1 padding and
    positions >= I among them -, the second entry a repeat of the first, and a length that may reach past the row."""
    U = base["user_emb"].shape[0]
    I = len(base["item_ok"])
    rs = np.random.RandomState(seed + 100)
    list_pos = np.full((U, W), -1, np.int32)
    list_len = np.zeros(U, np.int32)
    for u in range(U):
        n = rs.randint(0, W + 1)
        row = rs.randint(-1, I + 2, size=n)
        if n >= 2:
            row[1] = row[0]
        list_pos[u, :n] = row
        list_len[u] = n + rs.randint(0, 3)
    c = dict(base, list_pos=list_pos, list_len=list_len, I=I)
    c["excl_pos"] = c["excl_len"] = None
    return c


def first_slots(c, adm):
    """bool [U, W]: slot s of row u is the first occurrence of a position of ``adm[u]`` - where the diagnostic arrays hold a
    value (NaN everywhere else)."""
    U, W = c["list_pos"].shape
    first = np.zeros((U, W), bool)
    for u in range(U):
        seen = set()
        for s, p in enumerate(list_rows(c["list_pos"], c["list_len"], u)):
            if 0 <= p < adm.shape[1] and adm[u, p] and int(p) not in seen:
                seen.add(int(p))
                first[u, s] = True
    return first


def by_slot(c, adm, values, dtype):
    """``values`` [U, I] laid out by list slot, [U, W]: the value of the slot's position where ``first_slots``, NaN elsewhere."""
    first = first_slots(c, adm)
    out = np.full(first.shape, np.nan, dtype)
    u, s = np.nonzero(first)
    out[u, s] = values[u, c["list_pos"][u, s]]
    return out


def reference(c, k):
    """dict(top_pos, top_score, n_valid, adm, s64, score) of the score form: ``recommend_ref.topk`` over the list's set."""
    U, I = c["user_emb"].shape[0], c["I"]
    s64 = R.scores64(c["user_emb"], c["item_emb"], c["user_block"], I)
    adm = admissible_list(U, I, c["list_pos"], c["list_len"], c.get("item_ok"))
    pos, score, n = R.topk(s64, adm, k)
    return dict(top_pos=pos, top_score=score, n_valid=n, adm=adm, s64=s64, score=by_slot(c, adm, s64, np.float32))


def reference_mv(c, lam, k, scores=None, y=None):
    """What ``recommend_mv_ref.reference`` returns, over the list's set (``scores`` / ``y``: as there), and the three diagnostic
    arrays by list slot: ``score_slot``, ``y_slot``, ``fused_slot``."""
    U, I = c["user_emb"].shape[0], len(c["cand_stock"])
    s64 = R.scores64(c["user_emb"], c["item_emb"], c["user_block"], I)
    if y is None:
        y = M.y_matrix(c["returns"], c["day_idx"], c["cand_stock"], c["port_idx"], c["port_len"], c["gamma"])
    adm = M.admissible(admissible_list(U, I, c["list_pos"], c["list_len"], c.get("item_ok")), y)
    used = s64 if scores is None else scores
    pos, sc, fu, n, fused = M.fuse(used, y, adm, lam, k)
    return dict(top_pos=pos, top_score=sc, top_fused=fu, n_valid=n, y=np.where(adm, y, np.nan), fused=fused, adm=adm, s64=s64, y_raw=y,
                score_slot=by_slot(c, adm, used, np.float32), y_slot=by_slot(c, adm, y, np.float64),
                fused_slot=by_slot(c, adm, fused, np.float64))
