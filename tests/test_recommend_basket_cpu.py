"""Host side of the basket top-k: the three identities of the numpy reference (``recommend_basket_ref``) on the cases the GPU test
uses, a hand-built table on which the sequential list differs from the independent one the way it is meant to, the ``basket``
keyword of ``TGN.recommend`` checked without a device, and the C symbol."""
import os
import re
import types

import numpy as np
import pytest
import torch

import pfotgnrec_amd as P
from pfotgnrec_amd import _lib
from pfotgnrec_amd import recommend as RC
from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
import recommend_ref as R
import recommend_mv_ref as M
import recommend_basket_ref as B
from conftest import REPO


def _mv_single(lam):
    return lambda c: M.reference(c, lam, 1)


@pytest.mark.parametrize("spec", B.CASES, ids=lambda s: "seed%d" % s[0])
def test_reference_identities(spec):
    """k = 1 is the mean-variance list; lambda = 0 gives its positions for any k; any k is the loop of k single picks with the
    pick appended to the portfolio and exclusion rows.  And the feature shows: at lambda 0.5 several users of every case with
    room for it get a list the independent ranking does not give."""
    c, k = B.case(spec), spec[4]
    y = None
    for lam in B.LAMBDAS:
        plain = M.reference(c, lam, k, y=y)
        y = plain["y_raw"]
        got = B.reference(c, lam, k)
        assert B.same(B.reference(c, lam, 1), M.reference(c, lam, 1, y=y)), lam
        assert np.array_equal(got["top_pos"][:, 0], plain["top_pos"][:, 0]) and np.array_equal(got["n_valid"], plain["n_valid"])
        assert np.array_equal(got["top_fused"][:, 0], plain["top_fused"][:, 0])
        if lam == 0.0:
            assert np.array_equal(got["top_pos"], plain["top_pos"])
            assert np.array_equal(got["top_score"].view(np.int32), plain["top_score"].view(np.int32))
        assert B.same(got, B.loop_of_single_picks(c, k, _mv_single(lam))), lam
        # picks are distinct positions, the empty slots sit behind them
        for u in range(got["top_pos"].shape[0]):
            n = got["n_valid"][u]
            assert len(set(got["top_pos"][u, :n].tolist())) == n and (got["top_pos"][u, n:] == -1).all()
            assert np.isneginf(got["top_fused"][u, n:]).all() and np.isneginf(got["top_score"][u, n:]).all()
        if lam == 0.5:
            differs = int((got["top_pos"] != plain["top_pos"]).any(1).sum())
            print("users whose list differs from the independent one:", spec, differs)
            assert differs >= 5
    if spec[0] == 7:
        assert (got["n_valid"] < k).all(), "k > I: every list ends early"


def test_cases_keep_the_exactness_condition():
    for spec in B.CASES:
        seed, U, I, D, k, n_t, n_ret, W = spec
        c = B.case(spec)
        held = max(len(M.portfolio(c["port_idx"], c["port_len"], u, c["returns"].shape[1])) for u in range(U))
        pow2 = (n_ret - 1) & (n_ret - 2) == 0
        assert pow2 or held + k - 1 <= 7, spec


def test_a_correlated_pair_no_longer_fills_the_list():
    """Stocks 0 and 1 move together and rank highest, stock 2 is uncorrelated with them and ranks just below, stock 3 is a
    poor fourth.  lambda 1, k 2: the independent list is the pair; the basket takes stock 2 second, because with stock 1 held
    the twin's covariance weighs on its y."""
    a = np.array([3.0, -1.0, 3.0, -1.0, 3.0, -1.0, 3.0, -1.0, 1.0]) / 64.0          # y = 8 (rows sum to a multiple of n_ret = 9:
    b = np.array([34.0, 34.0, 14.0, 14.0, 34.0, 34.0, 14.0, 14.0, 24.0]) / 64.0     # y = 7.68     every mean and covariance exact)
    d = np.array([-4.0, 4.0, 4.0, -4.0, -4.0, 4.0, 4.0, -4.0, 0.0]) / 64.0          # y = 0
    returns = np.stack([a, a, b, d])[None]
    assert np.cov(a, b)[0, 1] == 0.0 and np.cov(a, d)[0, 1] == 0.0 and np.cov(b, d)[0, 1] == 0.0
    c = dict(user_emb=np.ones((1, 4), np.float32), item_emb=np.zeros((4, 4), np.float32), user_block=None, returns=returns,
             cand_stock=np.arange(4, dtype=np.int32), day_idx=np.zeros(1, np.int32), port_idx=np.zeros((1, 0), np.int32),
             port_len=np.zeros(1, np.int32), gamma=2.0)
    y = M.y_matrix(returns, c["day_idx"], c["cand_stock"], None, None)[0]
    assert y.tolist() == [8.0, 8.0, 7.68, 0.0]                      # held, the twin's y drops by 0.5 (its own variance / 2 / var)
    plain = M.reference(c, 1.0, 2)
    got = B.reference(c, 1.0, 2)
    assert plain["top_pos"].tolist() == [[1, 0]]
    assert got["top_pos"].tolist() == [[1, 2]] and got["n_valid"].tolist() == [2]
    # the fused value is the one of the pick's own round: first of four, then first of three
    assert got["top_fused"].tolist() == [[3.5, 3.0]]
    # a second candidate on the picked stock stays in the pool: four picks out of four
    assert sorted(B.reference(c, 1.0, 4)["top_pos"][0].tolist()) == [0, 1, 2, 3]


# ---- the keyword of TGN.recommend: checked on the host, before any device is asked for

@pytest.fixture(scope="module")
def cpu_model():
    g = make_graph(SyntheticConfig("t", 50, 10, 400, 8, 1, 4, 2), with_prices=False)
    nf = P.get_neighbor_finder(g.data, False)
    tgn = P.TGN(nf, g.node_features, g.edge_features, "cpu", n_layers=1, n_heads=2, use_memory=True, memory_dimension=8,
                message_function="identity")
    mv = types.SimpleNamespace(returns=torch.zeros(4, 10, 29, dtype=torch.float64), upper_u=50, gamma=2.0, lambda_mv=0.5,
                               day_of=lambda ts: np.asarray(ts, np.int64) % 4)
    return tgn, np.arange(51, 61), mv


def test_basket_is_validated_on_the_host(cpu_model):
    tgn, items, mv = cpu_model
    good = dict(users=[1, 2, 3], timestamps=5.0, k=3, items=items)
    with pytest.raises(ValueError, match="basket=True needs mv"):
        tgn.recommend(basket=True, **good)
    for bad in (1, 0, "yes", None, [True]):
        with pytest.raises(ValueError, match="basket must be"):
            tgn.recommend(mv=mv, portfolios=[[0], [], [1, 2]], basket=bad, **good)
    args = (tgn.n_nodes, tgn.n_neighbors, [1, 2, 3], 5.0, 3, items, None, None, None)
    def eq(x, y):
        if isinstance(x, np.ndarray):
            return np.array_equal(x, y)
        if isinstance(x, RC.MVQuery):
            return x.src is y.src and all(eq(p, q) for p, q in zip(x[1:], y[1:]))
        return x is y or x == y

    for kw in (dict(), dict(mv=mv, portfolios=[[0], [], [1, 2]])):
        a, b = RC.validate(*args, **kw), RC.validate(*args, basket=False, **kw)
        assert a.basket is False and a._fields == b._fields and all(eq(x, y) for x, y in zip(a, b))
    on = RC.validate(*args, mv=mv, portfolios=[[0], [], [1, 2]], basket=True)
    assert on.basket is True and all(eq(x, y) for x, y in zip(on[:-1], b[:-1]))
    if not torch.cuda.is_available():
        with pytest.raises(_lib.PfoError):                           # valid: only the device is missing - no fallback
            tgn.recommend(mv=mv, portfolios=[[0], [], [1, 2]], basket=True, **good)


def test_recommend_basket_topk_validates_then_requires_a_gpu():
    ue, ie = torch.zeros(3, 8), torch.zeros(10, 8)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    good = dict(user_emb=ue, item_emb=ie, k=3, cand_stock=i32(10), returns=torch.zeros(2, 5, 29, dtype=torch.float64),
                day_idx=i32(3), port_idx=i32(3, 4), port_len=i32(3), gamma=2.0, lambda_mv=0.5)
    for kw in (dict(k=0), dict(k=65), dict(cand_stock=i32(9)), dict(returns=torch.zeros(2, 5, 29)),
               dict(returns=torch.zeros(2, 5, 129, dtype=torch.float64)), dict(day_idx=i32(2)), dict(port_idx=i32(2, 4)),
               dict(port_idx=None), dict(user_block=i32(2)), dict(n_blocks=3), dict(excl_len=i32(3)), dict(user_emb=ue.double()),
               dict(cand_stock=i32(2049), item_emb=torch.zeros(2049, 8))):
        with pytest.raises(ValueError):
            P.recommend_basket_topk(**dict(good, **kw))
    with pytest.raises(TypeError):
        P.recommend_basket_topk(want_all=True, **good)               # no diagnostic arrays
    if not torch.cuda.is_available():
        with pytest.raises(_lib.PfoError):
            P.recommend_basket_topk(**good)


def test_header_and_ctypes_table_declare_the_symbol():
    text = open(os.path.join(REPO, "include", "pfotgn.h")).read()
    m = re.search(r"\bint\s+pfo_recommend_basket_topk\s*\(([^;]*)\)\s*;", text)
    assert m, "include/pfotgn.h does not declare pfo_recommend_basket_topk"
    params = [p.strip() for p in m.group(1).split(",")]
    mv = re.search(r"\bint\s+pfo_recommend_mv_topk\s*\(([^;]*)\)\s*;", text)
    mv_params = [p.strip() for p in mv.group(1).split(",")]
    assert params == mv_params[:27] + mv_params[30:], "pfo_recommend_mv_topk's arguments without the three diagnostic arrays"
    res, args = _lib.PROTOTYPES["pfo_recommend_basket_topk"]
    assert len(args) == len(params) == 28 and args == _lib.PROTOTYPES["pfo_recommend_mv_topk"][1][:27] + [_lib._VP]
    lib = _lib.load()
    assert hasattr(lib, "pfo_recommend_basket_topk") and lib.pfo_abi_version() == 6
