"""GPU tests of the group caps: ``pfo_recommend_topk_capped`` / ``pfo_recommend_mv_topk_capped`` /
``pfo_recommend_basket_topk_capped`` against the numpy reference of ``recommend_capped_ref`` - exact arithmetic, or the device's own
score matrix, so every comparison is equality: positions, counts, score bits, fused values - against their uncapped siblings
where the cap cannot bind, the capped basket against the k = 1 loop it replaces, and ``TGN.recommend(groups=, group_cap=)`` and
``backtest`` end to end."""
import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

import pfotgnrec_amd as P
from pfotgnrec_amd import recommend as RC
from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
import recommend_ref as R
import recommend_mv_ref as M
import recommend_basket_ref as B
import recommend_capped_ref as C

DEV = "cuda:0"
NAMES = ("top_pos", "top_score", "top_fused", "n_valid")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _cap(groups, cap):
    return {} if groups is None else dict(cand_group=_dev(np.asarray(groups, np.int32)), group_cap=cap)


def _plain(c, k, n_t=1, groups=None, cap=None):
    out = P.recommend_topk(_dev(c["user_emb"]), _dev(c["item_emb"]), k, _dev(c.get("user_block")), _dev(c.get("excl_pos")),
                           _dev(c.get("excl_len")), _dev(c.get("item_ok")), n_blocks=n_t, **_cap(groups, cap))
    return {n: t.cpu().numpy() for n, t in zip(("top_pos", "top_score", "n_valid"), out)}


def _mv_args(c, lam, k):
    return (_dev(c["user_emb"]), _dev(c["item_emb"]), k, _dev(c["cand_stock"]), _dev(c["returns"]), _dev(c["day_idx"]),
            _dev(c.get("port_idx")), _dev(c.get("port_len")), c["gamma"], lam, _dev(c.get("user_block")), _dev(c.get("excl_pos")),
            _dev(c.get("excl_len")), _dev(c.get("item_ok")))


def _mv(c, lam, k, n_t=1, groups=None, cap=None, want_all=False):
    out = P.recommend_mv_topk(*_mv_args(c, lam, k), n_blocks=n_t, want_all=want_all, **_cap(groups, cap))
    return {n: t.cpu().numpy() for n, t in zip(NAMES + ("score", "y", "fused"), out)}


def _basket(c, lam, k, n_t=1, groups=None, cap=None):
    return {n: t.cpu().numpy() for n, t in zip(NAMES, P.recommend_basket_topk(*_mv_args(c, lam, k), n_blocks=n_t, **_cap(groups, cap)))}


def _same_plain(a, b):
    return (np.array_equal(a["top_pos"], b["top_pos"]) and np.array_equal(a["n_valid"], b["n_valid"])
            and np.array_equal(np.asarray(a["top_score"]).view(np.int32), np.asarray(b["top_score"]).view(np.int32)))


def _obeys(top_pos, n_valid, groups, cap):
    for u in range(top_pos.shape[0]):
        p = top_pos[u, :n_valid[u]]
        g = np.asarray(groups)[p]
        if len(set(p.tolist())) != len(p) or (top_pos[u, n_valid[u]:] != -1).any() or any(int((g == v).sum()) > cap for v in np.unique(g[g >= 0])):
            return False
    return True


# ---------------------------------------------------------------------------------------------- exact arithmetic

@pytest.mark.parametrize("name", sorted(C.PLAIN_CASES))
def test_plain_kernel_equals_the_reference(name):
    """One, two and three chunks, a one-candidate last chunk (F), a partial 16-user tile, mixed blocks, D = 172, k = 64, lists
    that end short (E).  Before the device is looked at: the cap changes the list of at least half of the users."""
    c, groups, cap, k, n_t = C.plain_case(name)
    U = c["user_emb"].shape[0]
    changed, short = C.binding(c, groups, cap, k)
    assert 2 * changed >= U, (name, changed, U)
    assert name != "E" or short == U
    ref, got = C.reference_topk(c, groups, cap, k), _plain(c, k, n_t, groups, cap)
    for n in ("top_pos", "top_score", "n_valid"):
        print("FIGURES capped plain %s %s: %d of %d entries differ" % (name, n, int((got[n] != ref[n]).sum()), ref[n].size))
    assert _same_plain(got, ref), name
    assert _obeys(got["top_pos"], got["n_valid"], groups, cap)


@pytest.mark.parametrize("spec", B.CASES, ids=lambda s: "seed%d" % s[0])
def test_mv_and_basket_kernels_equal_the_reference(spec):
    """The cases of the basket test (their exactness conditions do not depend on the cap) at 3 groups with cap 1 and at 8 groups
    with cap 2, lambda 0, 0.5 and 1: all four outputs of both forms, and the diagnostics of the mean-variance form - the
    UNCAPPED y and fused of every admissible candidate."""
    c, (seed, U, I, D, k, n_t, n_ret, W) = B.case(spec), spec
    y = None
    for n_groups, cap in C.MV_CAPS:
        groups = C.groups_of(seed, I, n_groups)
        for lam in B.LAMBDAS:
            ref = C.reference_mv(c, lam, groups, cap, k, y=y)
            y = ref["y_raw"]
            got = _mv(c, lam, k, n_t, groups, cap, want_all=True)
            assert B.same(got, ref), (spec, n_groups, cap, lam)
            assert np.array_equal(got["y"], ref["y"], equal_nan=True) and np.array_equal(got["fused"], ref["fused"], equal_nan=True)
            assert _obeys(got["top_pos"], got["n_valid"], groups, cap)
            assert B.same(_basket(c, lam, k, n_t, groups, cap), C.reference_basket(c, lam, groups, cap, k)), (spec, n_groups, cap, lam)
        if (n_groups, cap) == (3, 1) and k >= 4:
            assert (got["top_pos"] != _mv(c, lam, k, n_t)["top_pos"]).any(), "the cap must move a list"


@pytest.mark.parametrize("D", [64, 128, 256])
def test_kernels_equal_the_reference_at_the_other_row_widths(D):
    """The cases above reach the instantiations for rows of up to 32 and 176 floats (the plain ones 64 too); these reach the
    ones for 64, 128 and 256, on the exact case of the uncapped kernels' tests of the same name."""
    c = M.exact_case(9000 + D, 17, 65, D, 5, 2, 29)
    groups = C.groups_of(D, 65, 3)
    assert _same_plain(_plain(c, 5, 2, groups, 1), C.reference_topk(c, groups, 1, 5))
    assert B.same(_mv(c, 0.5, 5, 2, groups, 1), C.reference_mv(c, 0.5, groups, 1, 5))
    assert B.same(_basket(c, 0.5, 5, 2, groups, 1), C.reference_basket(c, 0.5, groups, 1, 5))


# ---------------------------------------------------------------------------------------------- normal embeddings

def _normal(seed, U, I, D, n_t, n_ret=33, W=8):
    """Random normal embeddings, exclusion lists and an item_ok mask with the untidy mean-variance side of ``mv_side``; n_ret - 1
    a power of two: every covariance sum is exact in any order (``recommend_basket_ref``)."""
    c = R.normal_case(seed, U, I, D, n_t)
    c.update(M.mv_side(seed + 1, U, I, n_ret, W))
    return c


@pytest.mark.parametrize("U,I,D,n_t,k,k_basket", [(40, 500, 172, 1, 10, 3), (20, 1100, 64, 2, 10, 3), (3, 2048, 172, 1, 5, 3)])
def test_normal_cases_over_the_devices_own_scores(U, I, D, n_t, k, k_basket):
    """The reference runs over the score matrix the device computed (``score_out`` of the mean-variance entry: all kernels
    share ``rec_score_chunk``, so the bits are the plain kernel's too) - no rounding tolerance is needed.  2048 candidates is
    the LDS bound of the mean-variance and the basket form: the launch that asks for 152 KB."""
    c = _normal(100 + U, U, I, D, n_t)
    groups, cap = C.groups_of(U, I, 6), 2
    plain_mv = _mv(c, 0.5, k, n_t, want_all=True)
    scores = plain_mv["score"]
    base = R.admissible(U, I, c["excl_pos"], c["excl_len"], c["item_ok"])
    pos, sc, n = C.topk_capped(scores, base, groups, cap, k)
    got = _plain(c, k, n_t, groups, cap)
    assert _same_plain(got, dict(top_pos=pos, top_score=sc, n_valid=n))
    assert U < 20 or not np.array_equal(got["top_pos"], _plain(c, k, n_t)["top_pos"]), "the cap must move a list"
    ref = C.reference_mv(c, 0.5, groups, cap, k, scores=scores)
    got = _mv(c, 0.5, k, n_t, groups, cap, want_all=True)
    assert B.same(got, ref)
    for n_ in ("score", "y", "fused"):                                  # the diagnostics are the uncapped entry's
        assert np.array_equal(got[n_], plain_mv[n_], equal_nan=True), n_
    assert np.array_equal(got["y"], ref["y"], equal_nan=True) and np.array_equal(got["fused"], ref["fused"], equal_nan=True)
    assert U < 20 or not np.array_equal(got["top_pos"], plain_mv["top_pos"]), "the cap must move a list"
    assert B.same(_basket(c, 0.5, k_basket, n_t, groups, 1), C.reference_basket(c, 0.5, groups, 1, k_basket, scores=scores))


# ---------------------------------------------------------------------------------------------- equivalences on the device

@pytest.mark.parametrize("U,I,D,k,n_t", [(37, 40, 32, 4, 3), (33, 600, 172, 16, 2), (5, 2048, 64, 64, 1)])
def test_a_cap_that_cannot_bind_is_the_uncapped_entry(U, I, D, k, n_t):
    """group_cap >= k, every cand_group negative, and every candidate in a group of its own with cap 1: every output of the
    uncapped entry to the bit, in all three forms (the basket at min(k, 8) rounds)."""
    c = _normal(7 * U + I, U, I, D, n_t)
    kb = min(k, 8)
    plain, mv, bk = _plain(c, k, n_t), _mv(c, 0.5, k, n_t, want_all=True), _basket(c, 0.5, kb, n_t)
    own = (np.arange(I, dtype=np.int64)[::-1] * 1048573 % (2 ** 31 - 1)).astype(np.int32)
    assert len(set(own.tolist())) == I
    for groups, cap in ((C.groups_of(U, I, 3), k), (C.groups_of(U, I, 3), 2 ** 31 - 1), (np.full(I, -1, np.int32), 1),
                        (-1 - C.groups_of(U, I, 3).clip(0), 1), (own, 1)):
        assert _same_plain(_plain(c, k, n_t, groups, cap), plain)
        got = _mv(c, 0.5, k, n_t, groups, cap, want_all=True)
        assert B.same(got, mv) and all(np.array_equal(got[n], mv[n], equal_nan=True) for n in ("score", "y", "fused"))
        assert B.same(_basket(c, 0.5, kb, n_t, groups, cap), bk)


@pytest.mark.parametrize("U,I,D,k,n_t,n_groups,cap", [(33, 257, 32, 8, 3, 4, 2), (5, 70, 32, 64, 1, 3, 1), (3, 2048, 172, 3, 1, 2, 1)])
def test_capped_basket_equals_the_loop_of_single_picks(U, I, D, k, n_t, n_groups, cap):
    """What the one launch replaces: k launches of the UNCAPPED ``pfo_recommend_mv_topk`` at k = 1, the pick appended to the
    portfolio row and the exclusion row - and, once its group is full, the rest of the group to the exclusion row too."""
    c = _normal(7 * U + I, U, I, D, n_t, 29)
    groups = C.groups_of(I, I, n_groups)
    got = _basket(c, 0.5, k, n_t, groups, cap)
    want = C.loop_of_single_picks_capped(c, groups, cap, k, lambda cc: _mv(cc, 0.5, 1, n_t))
    assert B.same(got, want) and _obeys(got["top_pos"], got["n_valid"], groups, cap)
    assert not B.same(got, _basket(c, 0.5, k, n_t)), "the cap must move a list"
    if k == 64:                                                         # three groups of one pick and the groupless: lists end short
        assert (got["n_valid"] > 3).any() and (got["n_valid"] <= 3 + int((groups < 0).sum())).all()


# ---------------------------------------------------------------------------------------------- TGN.recommend and backtest end to end
N_USERS, N_ITEMS, K_NBR, CUT, LOG, BATCH, WIDTH, N_DAYS = 30, 40, 5, 300, 32, 16, 8, 64
ITEMS = np.arange(N_USERS + 1, N_USERS + N_ITEMS + 1)
GROUPS = np.arange(N_ITEMS) % 5 - 1                                     # eight items in no group, four groups of eight
CAP = 2


class _SynTables(P.InvestTables):
    """InvestTables over the synthetic calendar: the day of a timestamp is the graph's ``day_of``."""

    def day_indices(self, timestamps):
        return ((np.asarray(timestamps).astype(np.int64) * N_DAYS) >> 24).astype(np.int32)


class _World:
    """The small served model of the other recommend tests: memory, two layers, the first CUT interactions observed."""

    def __init__(self):
        self.g = g = make_graph(SyntheticConfig("t", N_USERS, N_ITEMS, 400, 16, 2, K_NBR, 2), with_prices=True)
        d = g.data
        sl = slice(CUT, CUT + LOG)
        self.log = (d.sources[sl], d.destinations[sl], d.timestamps[sl], d.edge_idxs[sl])
        self.ports = (g.portfolio_idx[sl], g.portfolio_len[sl])
        self.mv = P.MVSampler(g.prices, g.upper_u, DEV, day_of=g.day_of)
        rs = np.random.RandomState(4)
        future = g.prices * np.exp(np.cumsum(rs.randn(*g.prices.shape) * 0.02, axis=2))
        self.tables = _SynTables.from_prices(list(range(N_DAYS)), g.prices, future, g.map_item_id, upper_u=g.upper_u)
        self.days = g.day_of(self.log[2])

    def model(self):
        torch.manual_seed(6)
        g, d = self.g, self.g.data
        nf = P.NeighborFinder.from_arrays(d.sources[:CUT], d.destinations[:CUT], d.edge_idxs[:CUT], d.timestamps[:CUT], uniform=False,
                                          max_node_idx=g.node_features.shape[0] - 1)
        t = P.TGN(nf, g.node_features, g.edge_features, DEV, n_layers=2, n_heads=2, dropout=0.0, use_memory=True,
                  memory_dimension=16, message_function="identity", n_neighbors=K_NBR)
        t.eval()
        t.observe(d.sources[:CUT], d.destinations[:CUT], d.timestamps[:CUT], d.edge_idxs[:CUT], batch_size=50)
        return t


@pytest.fixture(scope="module")
def world():
    return _World()


def _state(t):
    m = t.memory
    out = [x.detach().clone() for x in (t.flat_parameters, m.memory, m.last_update, m.msg_table, m.msg_time, m.has_msg)]
    if t._flat_grad is not None:
        out.append(t._flat_grad.clone())
    return out


def _host_flags(t):
    return (t.training, t._step, t._gru_applied_now, t.memory._any_msg, t.memory._state_version)


def test_recommend_obeys_the_cap_in_the_three_orders_and_writes_nothing(world):
    w = world
    t = w.model()
    src, _, log_ts, _ = w.log
    users, ts, k = src[:BATCH], np.full(BATCH, float(log_ts[0])), 8
    ts[::3] += 64.0                                                     # two blocks, mixed: the block sort and its inverse run
    ok = np.arange(N_ITEMS) % 7 != 0
    ports = (w.ports[0][:BATCH].astype(np.int32), w.ports[1][:BATCH].astype(np.int32))
    groups_d = _dev(GROUPS.astype(np.int32))
    for order in (dict(), dict(mv=w.mv, portfolios=ports), dict(mv=w.mv, portfolios=ports, basket=True)):
        before, flags = _state(t), _host_flags(t)
        out = t.recommend(users, ts, k, ITEMS, item_ok=ok, return_embeddings=True, groups=GROUPS, group_cap=CAP, **order)
        assert all(torch.equal(x, y) for x, y in zip(before, _state(t))) and flags == _host_flags(t)
        assert not any(x.requires_grad for x in out)
        ids, n_valid = out[0].cpu().numpy(), out[2].cpu().numpy()
        pos = np.where(ids >= 0, ids - N_USERS - 1, -1)
        assert (n_valid == k).all() and _obeys(pos, n_valid, GROUPS, CAP) and ok[pos].all()
        plain = t.recommend(users, ts, k, ITEMS, item_ok=ok, **order)
        assert not torch.equal(plain[0], out[0]), "the cap must move a list"
        assert not _obeys(np.where(plain[0].cpu().numpy() >= 0, plain[0].cpu().numpy() - N_USERS - 1, -1), n_valid, GROUPS, CAP)
        # the functional call over the embeddings the query hands back
        ue, ie, ub = out[-3:]
        n_t = int(ie.shape[0]) // N_ITEMS
        assert n_t == 2
        cap = dict(cand_group=groups_d, group_cap=CAP)
        if not order:
            f_pos, f_score, f_n = P.recommend_topk(ue, ie, k, ub, None, None, _dev(ok), n_blocks=n_t, **cap)
            f_fused = None
        else:
            returns, day = RC.mv_device_side(w.mv, DEV, w.mv.day_of(ts))
            fn = P.recommend_basket_topk if order.get("basket") else P.recommend_mv_topk
            f_pos, f_score, f_fused, f_n = fn(ue, ie, k, _dev((ITEMS - w.g.upper_u - 1).astype(np.int32)), returns, day, _dev(ports[0]),
                                             _dev(ports[1]), float(w.mv.gamma), float(w.mv.lambda_mv), ub, None, None, _dev(ok), n_blocks=n_t,
                                             **cap)
            assert torch.equal(f_fused, out[3])
        assert torch.equal(f_pos, torch.from_numpy(pos.astype(np.int32)).to(DEV)) and torch.equal(f_score, out[1]) and torch.equal(f_n, out[2])
        # groups as a list and as an int64 device tensor: the same query
        for g in (GROUPS.tolist(), torch.from_numpy(GROUPS.astype(np.int64)).to(DEV)):
            again = t.recommend(users, ts, k, ITEMS, item_ok=ok, groups=g, group_cap=CAP, **order)
            assert all(torch.equal(x, y) for x, y in zip(again, out))
        # a cap that cannot bind is the query without one
        loose = t.recommend(users, ts, k, ITEMS, item_ok=ok, groups=GROUPS, group_cap=k, **order)
        assert all(torch.equal(x, y) for x, y in zip(loose, plain))
    with pytest.raises(ValueError, match="the list forms have no capped order"):
        t.recommend(users, ts, k, ITEMS, groups=GROUPS, group_cap=CAP, only=[[int(ITEMS[0])]] * BATCH)


def test_backtest_with_groups_is_recommend_score_observe_by_hand(world):
    """``backtest_rows(groups=, group_cap=)`` on one short log against a twin model walked by hand: the capped lists of
    ``recommend``, ``list_metrics`` on them, ``observe``."""
    w = world
    src, dst, ts, eidx = w.log
    cuts = (1, 3, 6)
    kw = dict(cutoffs=cuts, batch_size=BATCH, tables=w.tables, mv=w.mv, portfolios=w.ports)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)
    rows = P.backtest_rows(w.model(), src, dst, ts, eidx, ITEMS, 6, groups=GROUPS, group_cap=1, **kw)
    out = P.backtest(w.model(), src, dst, ts, eidx, ITEMS, 6, name="cap", groups=GROUPS, group_cap=1, **kw)
    assert out["cap_recall_avg_6"] == np.mean((rows["rank"] < 6).astype(np.float64)) and out["n"] == LOG
    assert _obeys(np.where(rows["list_item"] >= 0, rows["list_item"] - N_USERS - 1, -1), rows["n_valid"], GROUPS, 1)
    assert not np.array_equal(rows["list_item"], P.backtest_rows(w.model(), src, dst, ts, eidx, ITEMS, 6, **kw)["list_item"])
    b = w.model()
    rp, rf = w.tables.device_tables(DEV)
    day = i32(w.days)
    for lo in range(0, LOG, BATCH):
        hi = lo + BATCH
        ports = (w.ports[0][lo:hi], w.ports[1][lo:hi])
        res = b.recommend(src[lo:hi], ts[lo:hi], 6, ITEMS, mv=w.mv, portfolios=ports, groups=GROUPS, group_cap=1)
        assert np.array_equal(res[0].cpu().numpy(), rows["list_item"][lo:hi]) and np.array_equal(res[2].cpu().numpy(), rows["n_valid"][lo:hi])
        hand = P.list_metrics(res[0], i32(dst[lo:hi]), cuts, i32(ports[0]), i32(ports[1]), w.g.upper_u, rp, day[lo:hi], rf, day[lo:hi], res[2])
        for name, h in zip(("rank", "recall", "ndcg", "invest"), hand):
            h = h.cpu().numpy()
            assert np.array_equal(h.view(np.uint8), rows[name][lo:hi].view(np.uint8)), (name, lo)
        b.observe(src[lo:hi], dst[lo:hi], ts[lo:hi], eidx[lo:hi], batch_size=None)
