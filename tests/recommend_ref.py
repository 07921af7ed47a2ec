"""numpy reference of the read-only top-k recommendation (``pfo_recommend_topk`` / ``TGN.recommend``), in the style of
``finance_ref.py``: the fp64 score matrix, the skip rules, the canonical order (a stable ascending argsort,
reversed - score descending, the larger position first among equal scores) and the checker the GPU tests hold a result to.
"""
import numpy as np


def canonical_order(scores):
    """Positions of one row in the canonical order (-0 and +0 are equal scores)."""
    return np.argsort(np.asarray(scores), kind="stable")[::-1]


def item_rows(user_block, U, I):
    """[U, I] rows of item_emb that user u's candidates are: user_block[u] * I + i."""
    ub = np.zeros(U, np.int64) if user_block is None else np.asarray(user_block, np.int64)
    return ub[:, None] * I + np.arange(I)[None, :]


def scores64(user_emb, item_emb, user_block, I):
    """fp64 scores [U, I]: user_emb[u] . item_emb[user_block[u] * I + i]."""
    ue, ie = np.asarray(user_emb, np.float64), np.asarray(item_emb, np.float64)
    # (every user against every block, then each user's own block: one BLAS product instead of a [U, I, D] gather)
    return np.take_along_axis(ue @ ie.T, item_rows(user_block, ue.shape[0], I), 1)


def dot_error_bound(user_emb, item_emb, user_block, I):
    """eps [U, I] = gamma_D * sum_d |u_d * v_d|, gamma_D = D u / (1 - D u), u = 2^-24: the bound of an fp32 dot product of D
    terms evaluated in ANY order (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 3.5)."""
    ue, ie = np.abs(np.asarray(user_emb, np.float64)), np.abs(np.asarray(item_emb, np.float64))
    D = ue.shape[1]
    gamma = D * 2.0 ** -24 / (1.0 - D * 2.0 ** -24)
    return gamma * np.take_along_axis(ue @ ie.T, item_rows(user_block, ue.shape[0], I), 1)


def admissible(U, I, excl_pos=None, excl_len=None, item_ok=None):
    """bool [U, I]: candidate i may be offered to user u.  Skipped: item_ok[i] == 0, or i in excl_pos[u, :excl_len[u]]
    (entries outside [0, I) are ignored, duplicates allowed; excl_len None = the whole row, clamped to the row)."""
    adm = np.ones((U, I), bool)
    if item_ok is not None:
        adm &= (np.asarray(item_ok) != 0)[None, :]
    if excl_pos is not None:
        ep = np.asarray(excl_pos)
        W = ep.shape[1]
        for u in range(U):
            n = W if excl_len is None else min(max(int(excl_len[u]), 0), W)
            for p in ep[u, :n]:
                if 0 <= p < I:
                    adm[u, p] = False
    return adm


def topk(scores, adm, k):
    """(top_pos i32[U,k], top_score f32[U,k], n_valid i32[U]) of a score matrix: the first k admissible positions of every
    row's canonical order; empty slots -1 / -inf.  A zero score is +0."""
    scores = np.asarray(scores)
    U = scores.shape[0]
    top_pos = np.full((U, k), -1, np.int32)
    top_score = np.full((U, k), -np.inf, np.float32)
    n_valid = np.zeros(U, np.int32)
    for u in range(U):
        order = canonical_order(scores[u])
        order = order[adm[u][order]][:k]
        n = len(order)
        top_pos[u, :n] = order
        top_score[u, :n] = scores[u, order].astype(np.float32) + np.float32(0.0)
        n_valid[u] = n
    return top_pos, top_score, n_valid


def check_topk(top_pos, top_score, n_valid, s64, eps, adm, k):
    """Holds a result to the contract, against fp64 scores ``s64`` and their fp32 error bound ``eps`` (both [U, I]):
      (a) each returned score is within eps of the fp64 score of the returned item;
      (b) rows are sorted by the returned scores, the larger position first among bit-equal ones;
      (c) no skipped item, no duplicate, n_valid = min(k, #admissible), empty slots -1 / -inf;
      (d) no item left out has an fp64 score above that of the k-th returned item by more than the two items' eps.
    Users whose fp64 gap between rank k and rank k + 1 exceeds 4 x the largest eps of their row cannot have a member of the
    top k change places with an outsider (that needs a gap <= eps_i + eps_j): their id SET must be the reference's; where
    every gap down to rank k + 1 is that large, the ORDER too.  Returns the share of users of the first kind."""
    top_pos, top_score, n_valid = np.asarray(top_pos), np.asarray(top_score), np.asarray(n_valid)
    U, I = s64.shape
    assert top_pos.shape == (U, k) and top_score.shape == (U, k) and n_valid.shape == (U,)
    ref_pos, _, ref_n = topk(s64, adm, k)
    decided = 0
    for u in range(U):
        n = int(n_valid[u])
        assert n == min(k, int(adm[u].sum())) == ref_n[u], (u, n, int(adm[u].sum()))
        p, s = top_pos[u, :n].astype(np.int64), top_score[u, :n].astype(np.float64)
        assert (top_pos[u, n:] == -1).all() and np.isneginf(top_score[u, n:]).all(), u                      # (c)
        assert ((p >= 0) & (p < I)).all() and adm[u, p].all() and len(set(p.tolist())) == n, (u, p)          # (c)
        assert (np.abs(s - s64[u, p]) <= eps[u, p]).all(), (u, float(np.abs(s - s64[u, p]).max()))           # (a)
        for j in range(n - 1):                                                                              # (b)
            assert s[j] > s[j + 1] or (s[j] == s[j + 1] and p[j] > p[j + 1]), (u, j, s[j], s[j + 1], p[j], p[j + 1])
        left = adm[u].copy()
        left[p] = False
        if n == k and left.any():                                                                           # (d)
            last = p[-1]
            over = s64[u, left] - s64[u, last] - (eps[u, left] + eps[u, last])
            assert (over <= 0).all(), (u, float(over.max()))
        # users the rounding cannot touch
        order = canonical_order(s64[u])
        order = order[adm[u][order]]
        if len(order) <= k:
            gaps = -np.diff(s64[u, order])
            cut_clear = True
        else:
            gaps = -np.diff(s64[u, order[:k + 1]])
            cut_clear = gaps[-1] > 4.0 * eps[u].max()
        if cut_clear:
            decided += 1
            assert set(p.tolist()) == set(ref_pos[u, :n].tolist()), (u, p, ref_pos[u, :n])
            if (gaps > 4.0 * eps[u].max()).all():
                assert np.array_equal(p, ref_pos[u, :n]), (u, p, ref_pos[u, :n])
    return decided / max(U, 1)


def decided_share(s64, eps, adm, k):
    """The share ``check_topk`` returns, from the inputs alone (to fix seeds without a kernel)."""
    U = s64.shape[0]
    n = 0
    for u in range(U):
        order = canonical_order(s64[u])
        order = order[adm[u][order]]
        n += int(len(order) <= k or (s64[u, order[k - 1]] - s64[u, order[k]]) > 4.0 * eps[u].max())
    return n / max(U, 1)


def exact_case(seed, U, I, D, k, n_t):
    """Small-integer embeddings (every fp32 dot product exact in any order) with everything the order can trip over:
    duplicated item rows (ties), an all-zero user row (every score ties), exclusion lists with duplicates, -1 padding and
    positions >= I, an item_ok mask, user 0 with fewer than k admissible candidates, users of mixed blocks in shuffled order.
    Returns dict(user_emb, item_emb, user_block, excl_pos, excl_len, item_ok)."""
    rs = np.random.RandomState(seed)
    ue = rs.randint(-3, 4, size=(U, D)).astype(np.float32)
    ie = rs.randint(-3, 4, size=(n_t * I, D)).astype(np.float32)
    for b in range(n_t):                                        # a third of the rows repeat another row of their block
        for _ in range(I // 3):
            i, j = rs.randint(0, I, size=2)
            ie[b * I + i] = ie[b * I + j]
    ue[U // 2] = 0.0
    user_block = rs.randint(0, n_t, size=U).astype(np.int32) if n_t > 1 else None
    item_ok = (rs.rand(I) > 0.15).astype(np.uint8)
    if not item_ok.any():
        item_ok[rs.randint(0, I)] = 1
    W = I + 12
    excl_pos = np.full((U, W), -1, np.int32)
    excl_len = np.zeros(U, np.int32)
    for u in range(U):
        n = rs.randint(0, 9)
        row = rs.randint(-1, I + 3, size=n)                     # -1 and >= I among them
        if n >= 2:
            row[1] = row[0]                                     # a duplicate
        excl_pos[u, :n] = row
        excl_len[u] = n + rs.randint(0, 3)                      # the length may reach into the -1 padding
    # user 0: at most k - 2 candidates are left (none at k <= 2) -> fewer than k admissible
    keep = max(0, min(k - 1, I) - 1)
    row = rs.permutation(I)[:I - keep]
    excl_pos[0, :len(row)] = row
    excl_pos[0, len(row):len(row) + 3] = row[:1]                # duplicates behind them
    excl_len[0] = min(W, len(row) + 3)
    return dict(user_emb=ue, item_emb=ie, user_block=user_block, excl_pos=excl_pos, excl_len=excl_len, item_ok=item_ok)


def normal_case(seed, U, I, D, n_t=1):
    """Standard normal embeddings with portfolios of 0..7 excluded positions and an item_ok mask."""
    rs = np.random.RandomState(seed)
    ue = rs.randn(U, D).astype(np.float32)
    ie = rs.randn(n_t * I, D).astype(np.float32)
    user_block = rs.randint(0, n_t, size=U).astype(np.int32) if n_t > 1 else None
    excl_pos = np.full((U, 8), -1, np.int32)
    excl_len = rs.randint(0, 8, size=U).astype(np.int32)
    for u in range(U):
        excl_pos[u, :excl_len[u]] = rs.randint(0, I, size=excl_len[u])
    item_ok = (rs.rand(I) > 0.05).astype(np.uint8)
    return dict(user_emb=ue, item_emb=ie, user_block=user_block, excl_pos=excl_pos, excl_len=excl_len, item_ok=item_ok)
