"""GPU tests of the basket top-k: ``pfo_recommend_basket_topk`` against the numpy reference of ``recommend_basket_ref`` (exact
arithmetic, bit for bit), against ``pfo_recommend_mv_topk`` at k = 1 and against the loop of k single picks a caller runs today,
its edges, and ``TGN.recommend(mv=..., basket=True)`` end to end.  Every comparison is equality."""
import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

import pfotgnrec_amd as P
from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
import recommend_ref as R
import recommend_mv_ref as M
import recommend_basket_ref as B

DEV = "cuda:0"
NAMES = ("top_pos", "top_score", "top_fused", "n_valid")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _args(c, lam, k, n_t):
    return (_dev(c["user_emb"]), _dev(c["item_emb"]), k, _dev(c["cand_stock"]), _dev(c["returns"]), _dev(c["day_idx"]),
            _dev(c.get("port_idx")), _dev(c.get("port_len")), c["gamma"], lam, _dev(c.get("user_block")), _dev(c.get("excl_pos")),
            _dev(c.get("excl_len")), _dev(c.get("item_ok")))


def _basket(c, lam, k, n_t=1):
    return {n: t.cpu().numpy() for n, t in zip(NAMES, P.recommend_basket_topk(*_args(c, lam, k, n_t), n_blocks=n_t))}


def _mv(c, lam, k, n_t=1):
    return {n: t.cpu().numpy() for n, t in zip(NAMES, P.recommend_mv_topk(*_args(c, lam, k, n_t), n_blocks=n_t))}


def _normal(seed, U, I, D, n_t, n_ret, W=8):
    """Random normal embeddings, exclusion lists and an item_ok mask with the untidy mean-variance side of ``mv_side`` (NaN y,
    stocks and days outside the tables, portfolios with duplicates and out-of-range entries)."""
    c = R.normal_case(seed, U, I, D, n_t)
    c.update(M.mv_side(seed + 1, U, I, n_ret, W))
    return c


# ---------------------------------------------------------------------------------------------- the kernel alone

@pytest.mark.parametrize("spec", B.CASES, ids=lambda s: "seed%d" % s[0])
def test_kernel_equals_the_reference(spec):
    """Exact arithmetic (integer embeddings, return tables of ``exact_returns`` under the exactness condition of
    ``recommend_basket_ref``): positions, scores, fused values of every round and counts are the reference's to the bit."""
    c, k, n_t = B.case(spec), spec[4], spec[5]
    for lam in B.LAMBDAS:
        ref, got = B.reference(c, lam, k), _basket(c, lam, k, n_t)
        for n in NAMES:
            print("FIGURES basket %s lambda %.1f %s: %d of %d entries differ" % (spec, lam, n, int((got[n] != ref[n]).sum()), ref[n].size))
        assert B.same(got, ref), (spec, lam)
        if lam == 0.5:
            plain = _mv(c, lam, k, n_t)
            assert (got["top_pos"] != plain["top_pos"]).any(1).sum() >= 5, "the picks must move the list"
    if spec[0] == 7:
        assert (got["n_valid"] < k).all()


@pytest.mark.parametrize("D", [48, 64, 112, 128])
def test_kernel_equals_the_reference_at_the_middle_row_widths(D):
    """``B.CASES`` reach the instantiations for rows of up to 32, 176 and 256 floats; these reach the ones for 64 and 128, at
    both ends of each, on the exact case of the mean-variance kernel's test of the same name."""
    c = M.exact_case(9000 + D, 17, 65, D, 5, 2, 29)
    ref = B.reference(c, 0.5, 5)
    assert (ref["n_valid"] == 0).any() and (ref["n_valid"] == 5).any()
    assert B.same(_basket(c, 0.5, 5, 2), ref), D


@pytest.mark.parametrize("I", [1, 2, 15, 16, 17, 255, 256, 257, 2048])
def test_one_pick_is_the_mean_variance_kernel(I):
    """k = 1 against ``pfo_recommend_mv_topk``: all four outputs equal, at the edges of the 16-wide score tile, of the 256
    threads that share a user's candidates and of the 16-user tile; 2048 is the LDS bound (the launch that asks for it)."""
    seed = 0
    for U in (1, 15, 16, 17, 33):
        for D in (32, 172):
            for n_ret in (2, 29, 128):
                seed += 1
                n_t = 2 if U > 1 else 1
                c = _normal(1000 * I + seed, U, I, D, n_t, n_ret)
                assert B.same(_basket(c, 0.5, 1, n_t), _mv(c, 0.5, 1, n_t)), (U, I, D, n_ret)


@pytest.mark.parametrize("U,I,D,k,n_t,W", [(33, 257, 32, 8, 3, 8), (5, 70, 32, 64, 1, 8), (3, 2048, 172, 3, 1, 8)])
def test_kernel_equals_the_loop_of_single_picks(U, I, D, k, n_t, W):
    """What a caller does today - k launches of ``pfo_recommend_mv_topk`` with k = 1, the pick appended to the portfolio row
    and to the exclusion row in between - gives the same four outputs (holdings pass eight: both sides add in list order)."""
    c = _normal(7 * U + I, U, I, D, n_t, 29, W)
    got = _basket(c, 0.5, k, n_t)
    want = B.loop_of_single_picks(c, k, lambda cc: _mv(cc, 0.5, 1, n_t))
    assert B.same(got, want)
    if U == 33:
        held = max(len(M.portfolio(c["port_idx"], c["port_len"], u, c["returns"].shape[1])) for u in range(U))
        no_day = [5, U - 1]                                             # (``mv_side``: their day is outside the tables)
        assert held == 7 and (np.delete(got["n_valid"], no_day) == k).all() and (got["n_valid"][no_day] == 0).all()
    if k == 64:
        assert (got["n_valid"] < k).any() and (got["n_valid"] == k).any()   # some lists run out of candidates, some do not


def _pair_table():
    """The hand-built day of tests/test_recommend_basket_cpu.py: stocks 0 and 1 identical (y = 8), 2 uncorrelated (7.68), 3 (0)."""
    a = np.array([3.0, -1.0, 3.0, -1.0, 3.0, -1.0, 3.0, -1.0, 1.0]) / 64.0
    b = np.array([34.0, 34.0, 14.0, 14.0, 34.0, 34.0, 14.0, 14.0, 24.0]) / 64.0
    d = np.array([-4.0, 4.0, 4.0, -4.0, -4.0, 4.0, 4.0, -4.0, 0.0]) / 64.0
    return np.stack([a, a, b, d])[None]


def test_edges():
    c0 = B.case(B.CASES[2])                                          # (5, 20, 70, 32, 16, 1, 17, 8): any number of holdings is exact
    U, I, k = 20, 70, 16
    empty = dict(top_pos=np.full((U, k), -1, np.int32), top_score=np.full((U, k), -np.inf, np.float32),
                 top_fused=np.full((U, k), -np.inf), n_valid=np.zeros(U, np.int32))
    # every candidate excluded, by the mask and by the lists
    assert B.same(_basket(dict(c0, item_ok=np.zeros(I, np.uint8)), 0.5, k), empty)
    everything = np.tile(np.arange(I, dtype=np.int32), (U, 1))
    assert B.same(_basket(dict(c0, excl_pos=everything, excl_len=None), 0.5, k), empty)
    # every day outside the tables
    for day in (-1, c0["returns"].shape[0]):
        assert B.same(_basket(dict(c0, day_idx=np.full(U, day, np.int32)), 0.5, k), empty)
    # nobody holds anything: port_idx null
    c = dict(c0, port_idx=None, port_len=None)
    assert B.same(_basket(c, 0.5, k), B.reference(c, 0.5, k))
    # the constant stock (row 0 of every day): held, it counts as a holding with covariance 0; as a candidate it is never picked
    c = dict(c0, port_idx=c0["port_idx"].copy())
    c["port_idx"][c["port_len"] > 0, 0] = 0
    got = _basket(c, 0.5, k)
    assert c["cand_stock"][I - 1] == 0 and not (got["top_pos"] == I - 1).any()
    assert B.same(got, B.reference(c, 0.5, k))
    # two candidates on one stock: the pick takes its position out, the other stays and now carries its own variance
    pair = dict(user_emb=np.ones((1, 4), np.float32), item_emb=np.zeros((4, 4), np.float32), user_block=None, returns=_pair_table(),
                cand_stock=np.array([0, 0, 2, 3], np.int32), day_idx=np.zeros(1, np.int32), port_idx=None, port_len=None, gamma=2.0)
    got = _basket(pair, 1.0, 4)
    assert got["top_pos"].tolist() == [[1, 2, 0, 3]] and got["top_fused"].tolist() == [[3.5, 3.0, 2.0, 1.0]]
    assert B.same(got, B.reference(pair, 1.0, 4)) and _mv(pair, 1.0, 4)["top_pos"].tolist() == [[1, 0, 2, 3]]


def test_users_short_of_candidates_inside_a_tile():
    """One tile of 16 users: user 3 has two candidates left, user 7 none, user 11 one, the others all of them - the early ends
    must not disturb the rounds of the users behind them."""
    spec = (5, 16, 70, 32, 16, 1, 17, 8)
    c = B.case(spec)
    U, I, k = 16, 70, 16
    c["day_idx"] = np.zeros(U, np.int32)
    c["item_ok"] = None
    excl = np.full((U, I), -1, np.int32)
    for u, left in ((3, 2), (7, 0), (11, 1)):
        excl[u, :I - left] = np.random.RandomState(u).permutation(I)[:I - left]
    c["excl_pos"], c["excl_len"] = excl, None
    ref, got = B.reference(c, 0.5, k), _basket(c, 0.5, k)
    assert ref["n_valid"][[3, 7, 11]].tolist() == [2, 0, 1] and (np.delete(ref["n_valid"], [3, 7, 11]) == k).all()
    assert B.same(got, ref)


def test_errors_of_the_entry_point():
    from pfotgnrec_amd import _lib
    c = B.case(B.CASES[0])
    ue, ie, out = _dev(c["user_emb"]), _dev(c["item_emb"]), torch.empty(20 * 4 * 8, dtype=torch.int32, device=DEV)
    args = lambda I, k, n_ret: ("pfo_recommend_basket_topk", ue.data_ptr(), ie.data_ptr(), None, 20, I, 1, 32, None, None, 0, None,
                                _dev(c["cand_stock"]).data_ptr(), _dev(c["returns"]).data_ptr(), 3, 42, n_ret,
                                _dev(c["day_idx"]).data_ptr(), None, None, 0, 2.0, 0.5, k, out.data_ptr(), out.data_ptr(),
                                out.data_ptr(), None, _lib.stream_ptr())
    for bad, msg in ((args(2049, 4, 29), "I must be"), (args(40, 65, 29), "k must be"), (args(40, 4, 1), "n_ret must be")):
        with pytest.raises(_lib.PfoError, match=msg):
            _lib.call(*bad)


# ---------------------------------------------------------------------------------------------- TGN.recommend end to end
N_USERS, N_ITEMS, K_NBR, CUT, WIDTH = 120, 30, 5, 900, 8
ITEMS = np.arange(N_USERS + 1, N_USERS + N_ITEMS + 1)


class _World:
    """A small served model: memory and messages advanced over the first CUT interactions, their portfolios in the ledger, a
    mean-variance sampler over the synthetic prices."""

    def __init__(self):
        torch.manual_seed(6)
        self.g = g = make_graph(SyntheticConfig("t", N_USERS, N_ITEMS, 1500, 16, 1, K_NBR, 2), with_prices=True)
        d = g.data
        nf = P.NeighborFinder.from_arrays(d.sources[:CUT], d.destinations[:CUT], d.edge_idxs[:CUT], d.timestamps[:CUT], uniform=False,
                                          max_node_idx=g.node_features.shape[0] - 1)
        self.tgn = t = P.TGN(nf, g.node_features, g.edge_features[:CUT + 1], DEV, n_layers=1, n_heads=2, dropout=0.0, use_memory=True,
                             memory_dimension=16, message_function="identity", n_neighbors=K_NBR)
        t.eval()
        t.observe(d.sources[:CUT], d.destinations[:CUT], d.timestamps[:CUT], d.edge_idxs[:CUT], batch_size=50)
        t.track_holdings(WIDTH, g.upper_u)
        t.update_holdings(d.sources[:CUT], (g.portfolio_idx[:CUT], g.portfolio_len[:CUT]), d.timestamps[:CUT])
        self.mv = P.MVSampler(g.prices, g.upper_u, DEV, day_of=g.day_of)
        self.users = np.concatenate([np.unique(d.sources[CUT - 200:CUT])[:35], [3, 4]])
        self.now = float(d.timestamps[CUT - 1]) + 1.0
        idx, ln = (x.cpu().numpy() for x in t.holdings.rows(self.users))
        self.rows = (idx, ln)
        self.stocks = [[int(s) for s in idx[i, :ln[i]]] for i in range(len(self.users))]
        self.held_items = [[s + g.upper_u + 1 for s in row] for row in self.stocks]

    def state(self):
        m = self.tgn.memory
        return [x.detach().clone() for x in (self.tgn.flat_parameters, m.memory, m.last_update, m.msg_table, m.msg_time, m.has_msg,
                                             self.tgn.holdings.idx, self.tgn.holdings.len)]

    def loop(self, ts, k, stocks, excluded, **kw):
        """k calls of ``recommend(mv=, k=1)``, each pick appended to the user's portfolio and exclusion lists."""
        U = len(self.users)
        stocks, excluded = [list(r) for r in stocks], [list(r) for r in excluded]
        ids = np.full((U, k), -1, np.int32)
        scores = np.full((U, k), -np.inf, np.float32)
        fused = np.full((U, k), -np.inf)
        n_valid = np.zeros(U, np.int32)
        for r in range(k):
            one = [x.cpu().numpy() for x in self.tgn.recommend(self.users, ts, 1, ITEMS, mv=self.mv, portfolios=stocks, exclude=excluded, **kw)]
            for u in np.flatnonzero((one[2] == 1) & (n_valid == r)):
                ids[u, r], scores[u, r], fused[u, r], n_valid[u] = one[0][u, 0], one[1][u, 0], one[3][u, 0], r + 1
                stocks[u].append(int(ids[u, r]) - self.g.upper_u - 1)
                excluded[u].append(int(ids[u, r]))
        return ids, scores, n_valid, fused


@pytest.fixture(scope="module")
def world():
    return _World()


def _same_out(got, want):
    got = [x.cpu().numpy() for x in got[:4]]
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.int32), want[1].view(np.int32))
            and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]))


def test_recommend_basket_equals_the_loop_and_writes_nothing(world):
    w = world
    U, k = len(w.users), 5
    ts = np.array([w.now, w.now - 300.0, w.now + 64.0])[np.random.RandomState(2).randint(0, 3, size=U)]
    ok = np.arange(N_ITEMS) % 7 != 0
    before = w.state()
    out = w.tgn.recommend(w.users, ts, k, ITEMS, mv=w.mv, portfolios=w.stocks, exclude=w.held_items, item_ok=ok, basket=True,
                          return_embeddings=True)
    assert all(torch.equal(x, y) for x, y in zip(before, w.state())) and not w.tgn.training
    assert len(out) == 7 and out[3].dtype == torch.float64 and not any(t.requires_grad for t in out)
    ub = out[6].cpu().numpy()
    assert len(set(ub.tolist())) == 3 and (np.diff(ub) < 0).any(), "mixed blocks, not sorted: the block sort and its inverse run"
    assert _same_out(out, w.loop(ts, k, w.stocks, w.held_items, item_ok=ok))
    ids = out[0].cpu().numpy()
    assert (out[2].cpu().numpy() == k).all()
    for u in range(U):
        assert len(set(ids[u].tolist())) == k and not (set(ids[u].tolist()) & set(w.held_items[u]))
        assert not (set(ids[u].tolist()) & set(ITEMS[~ok].tolist()))
    plain = w.tgn.recommend(w.users, ts, k, ITEMS, mv=w.mv, portfolios=w.stocks, exclude=w.held_items, item_ok=ok)
    assert torch.equal(plain[0][:, 0], out[0][:, 0]) and not torch.equal(plain[0], out[0]), "the picks must move the list"
    # one timestamp for all (no block sort), and one user alone gets what it got in the crowd
    one_ts = w.tgn.recommend(w.users, w.now, k, ITEMS, mv=w.mv, portfolios=w.stocks, exclude=w.held_items, basket=True)
    assert len(one_ts) == 4 and _same_out(one_ts, w.loop(w.now, k, w.stocks, w.held_items))
    alone = w.tgn.recommend(w.users[4:5], ts[4], k, ITEMS, mv=w.mv, portfolios=w.stocks[4:5], exclude=w.held_items[4:5], item_ok=ok,
                            basket=True)
    assert all(torch.equal(alone[i][0], out[i][4]) for i in range(4))
    empty = w.tgn.recommend(w.users[:0], w.now, k, ITEMS, mv=w.mv, portfolios=[], basket=True)
    assert [tuple(t.shape) for t in empty] == [(0, k), (0, k), (0,), (0, k)]


def test_recommend_basket_reads_the_ledger(world):
    w = world
    U, k = len(w.users), 4
    ts = np.where(np.arange(U) % 2 == 0, w.now, w.now + 5.0)
    assert sum(len(r) for r in w.stocks) > 20
    want = w.tgn.recommend(w.users, ts, k, ITEMS, mv=w.mv, portfolios=w.rows, exclude=w.held_items, basket=True)
    for kw in (dict(portfolios="held", exclude="held"), dict(portfolios="held", exclude=w.held_items),
               dict(portfolios=w.stocks, exclude="held")):
        got = w.tgn.recommend(w.users, ts, k, ITEMS, mv=w.mv, basket=True, **kw)
        assert all(torch.equal(x, y) for x, y in zip(got, want)), sorted(kw.items())


def test_basket_false_is_the_call_without_the_keyword(world):
    w = world
    ts = np.where(np.arange(len(w.users)) % 2 == 0, w.now, w.now + 5.0)
    for kw in (dict(), dict(mv=w.mv, portfolios=w.stocks), dict(mv=w.mv, portfolios="held", exclude="held", return_embeddings=True)):
        a = w.tgn.recommend(w.users, ts, 5, ITEMS, **kw)
        b = w.tgn.recommend(w.users, ts, 5, ITEMS, basket=False, **kw)
        assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
