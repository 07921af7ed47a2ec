"""Host side of the portfolio-aware top-k: the numpy reference pinned to the reference project's recorded y_mv, the reference's
own behaviour on hand-made cases, every ValueError of ``TGN.recommend(mv=...)`` without a device, and the ctypes table."""
import types

import numpy as np
import pytest
import torch

import pfotgnrec_amd as P
from pfotgnrec_amd import _lib
from pfotgnrec_amd.mv_sampler import log_returns
from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
import recommend_ref as R
import recommend_mv_ref as M
from conftest import load_golden


@pytest.mark.parametrize("lam", ["lam05", "lam01"])
def test_reference_y_mv_reproduces_the_golden_of_the_reference_project(lam):
    """g3_mv.npz holds main.py's own y_mv per candidate (fp64): the reference used by the GPU tests must give those bits from
    the fixture's prices, candidates and portfolios."""
    g = load_golden("g3_mv")
    up = int(g["upper_u"])
    ret = log_returns(g["prices"])
    cand = np.concatenate([g["dst"].reshape(-1, 1), g[lam + "_neg"]], 1) - up - 1
    for b in range(cand.shape[0]):
        port = M.portfolio(g["port_idx"], g["port_len"], b, ret.shape[1])
        y = M.y_mv(ret, int(g[lam + "_day_idx"][b]), cand[b], port, float(g["gamma"]))
        assert np.array_equal(y, g[lam + "_y_mv"][b]), b
    assert (g["port_len"] == 0).any() and (g["port_len"] > 1).any()


def test_reference_fuse_on_a_hand_made_row():
    #                 pos:  0    1    2     3    4
    s = np.array([[1.0, 3.0, 3.0, -0.0, 0.0]])
    y = np.array([[5.0, 1.0, np.inf, 2.0, np.nan]])
    adm = M.admissible(np.ones((1, 5), bool), y)
    assert adm.tolist() == [[True, True, True, True, False]]
    # ranks over the four: score 2, 3.5, 3.5, 1 ; y 3, 1, 4, 2
    pos, sc, fu, n, fused = M.fuse(s, y, adm, 0.5, 3)
    assert fused[0, :4].tolist() == [2.5, 2.25, 3.75, 1.5] and np.isnan(fused[0, 4])
    assert pos.tolist() == [[2, 0, 1]] and fu.tolist() == [[3.75, 2.5, 2.25]] and n.tolist() == [3]
    assert sc.tolist() == [[3.0, 1.0, 3.0]]
    pos, _, fu, n, _ = M.fuse(s, y, adm, 0.0, 5)                  # lambda 0: the order of the scores, larger position first
    assert pos.tolist() == [[2, 1, 0, 3, -1]] and n.tolist() == [4] and np.isneginf(fu[0, 4])
    assert pos[0, :4].tolist() == R.topk(s, adm, 5)[0][0, :4].tolist()
    pos, _, _, _, _ = M.fuse(s, y, adm, 1.0, 5)                   # lambda 1: y alone
    assert pos.tolist() == [[2, 0, 3, 1, -1]]
    tie = M.fuse(np.zeros((1, 3)), np.array([[1.0, 1.0, 1.0]]), np.ones((1, 3), bool), 0.3, 3)
    assert tie[0].tolist() == [[2, 1, 0]] and len(set(tie[2][0].tolist())) == 1 and abs(tie[2][0, 0] - 2.0) < 1e-15


def test_reference_portfolio_rules_and_exact_tables():
    pi = np.array([[3, 3, -1, 9, 1, 2], [0, 1, 2, 3, 4, 5]], np.int32)
    assert M.portfolio(pi, np.array([5, 9]), 0, 9).tolist() == [3, 3, 1]           # duplicate kept, -1 and 9 dropped
    assert M.portfolio(pi, np.array([5, 9]), 1, 9).tolist() == [0, 1, 2, 3, 4, 5]  # the length is clamped to the row
    assert M.portfolio(pi, np.array([0, 0]), 0, 9).tolist() == []
    for n_ret in (2, 29):
        c = M.exact_case(3, 17, 65, 4, 5, 2, n_ret)
        v = c["returns"] * 64.0
        assert (v == np.rint(v)).all() and (np.abs(v) <= 64).all() and (v.sum(2) % n_ret == 0).all()
        y = M.y_matrix(c["returns"], c["day_idx"], c["cand_stock"], c["port_idx"], c["port_len"])
        assert np.isnan(y[:, 0]).all() and np.isnan(y[:, 64]).all()                # cand_stock -1; the constant stock: 0 / 0
        assert np.isnan(y[16]).all() and np.isnan(y[5]).all()                      # days outside the table
        ok = ~np.isnan(y[1])
        assert ok.sum() > 40 and len(np.unique(y[1][ok])) < ok.sum()               # y ties
        held = [len(M.portfolio(c["port_idx"], c["port_len"], u, c["returns"].shape[1])) for u in range(17)]
        assert held[1] == 0 and held[2] == 1 and held[3] == 7 and held[4] == 0 and max(held) <= 7
        r = M.reference(c, 0.5, 5)
        assert r["n_valid"][0] < 5 and (r["n_valid"][[5, 16]] == 0).all()


def test_seeds_of_the_gpu_test_leave_one_user_in_two_with_separated_scores():
    """Test 4 of the GPU file asserts the reference's order for this share of its users; here from the inputs alone."""
    for seed, U, I, D, k in M.BLEND_CASES:
        c = R.normal_case(seed, U, I, D)
        s, eps = R.scores64(c["user_emb"], c["item_emb"], None, I), R.dot_error_bound(c["user_emb"], c["item_emb"], None, I)
        share = M.separated_share(s, eps, R.admissible(U, I, c["excl_pos"], c["excl_len"], c["item_ok"]))
        print("separated share", (seed, U, I, D, k), share)
        assert share >= 0.5


# ---- TGN.recommend(mv=...): every ValueError fires without a device

@pytest.fixture(scope="module")
def cpu_model():
    g = make_graph(SyntheticConfig("t", 50, 10, 400, 8, 1, 4, 2), with_prices=False)
    nf = P.get_neighbor_finder(g.data, False)
    tgn = P.TGN(nf, g.node_features, g.edge_features, "cpu", n_layers=1, n_heads=2, use_memory=True, memory_dimension=8,
                message_function="identity")
    mv = types.SimpleNamespace(returns=torch.zeros(4, 10, 29, dtype=torch.float64), upper_u=50, gamma=2.0, lambda_mv=0.5,
                               day_of=lambda ts: np.asarray(ts, np.int64) % 4)
    return tgn, np.arange(51, 61), mv


GOOD = dict(users=[1, 2, 3], timestamps=5.0, k=3, portfolios=[[0], [], [1, 2]])


def _no_attr(mv, name):
    d = dict(vars(mv))
    del d[name]
    return types.SimpleNamespace(**d)


@pytest.mark.parametrize("bad", [
    dict(mv=None), dict(mv=None, portfolios=None, day_idx=1), dict(portfolios=None),
    dict(portfolios=[[0], []]), dict(portfolios=5), dict(portfolios=[[0.5], [], []]),
    dict(portfolios=(np.zeros((2, 4), np.int32), np.zeros(2, np.int32))),
    dict(portfolios=(np.zeros((3, 4), np.float32), np.zeros(3, np.int32))),
    dict(portfolios=(np.zeros((3, 4), np.int32), np.zeros(3, np.float64))),
    dict(portfolios=(torch.zeros(3, 4), torch.zeros(3, dtype=torch.int32))),
    dict(portfolios=(np.zeros((3, 4), np.int32), np.zeros((3, 1), np.int32))),
    dict(day_idx=4), dict(day_idx=-1), dict(day_idx=[0, 1]), dict(day_idx=[0, 1, 4]), dict(day_idx=1.0),
    dict(day_idx=np.zeros((3, 1), np.int64)), dict(day_idx=torch.zeros(3)),
    dict(timestamps=torch.tensor(5.0)), dict(timestamps=6.0, mv="shifted_days"),
    dict(mv="no_returns"), dict(mv="no_day_of"), dict(mv="flat_returns"),
    dict(k=0), dict(items=[51, 52, 51]),
], ids=lambda d: ",".join("%s=%s" % (k, str(v).replace("\n", "")[:18]) for k, v in d.items()))
def test_recommend_mv_rejects_bad_arguments_before_asking_for_a_gpu(cpu_model, bad):
    tgn, items, mv = cpu_model
    args = dict(GOOD, items=items, mv=mv)
    args.update(bad)
    if args["mv"] == "no_returns":
        args["mv"] = _no_attr(mv, "returns")
    elif args["mv"] == "no_day_of":
        args["mv"] = _no_attr(mv, "day_of")
    elif args["mv"] == "flat_returns":
        args["mv"] = types.SimpleNamespace(**dict(vars(mv), returns=torch.zeros(4, 290, dtype=torch.float64)))
    elif args["mv"] == "shifted_days":                      # day_of answers with a day the table does not hold
        args["mv"] = types.SimpleNamespace(**dict(vars(mv), day_of=lambda ts: np.asarray(ts, np.int64) + 10))
    with pytest.raises(ValueError):
        tgn.recommend(**args)


def test_recommend_mv_limits_the_candidate_list():
    q = dict(U=3, mv=types.SimpleNamespace(returns=np.zeros((2, 5, 3)), upper_u=0, gamma=2.0, lambda_mv=0.5, day_of=None),
             portfolios=[[], [], []], day_idx=0, ts_h=None, scalar_ts=True)
    from pfotgnrec_amd import recommend as RC
    assert _lib.RECOMMEND_MV_MAX_ITEMS == 2048
    mvq = RC.validate_mv(I=2048, **q)
    assert mvq.day_idx.tolist() == [0, 0, 0] and mvq.port_idx.shape == (3, 0)
    with pytest.raises(ValueError, match="2048"):
        RC.validate_mv(I=2049, **q)
    with pytest.raises(ValueError):
        P.recommend_mv_topk(torch.zeros(3, 8), torch.zeros(2049, 8), 3, torch.zeros(2049, dtype=torch.int32),
                            torch.zeros(2, 5, 3, dtype=torch.float64), torch.zeros(3, dtype=torch.int32), None, None, 2.0, 0.5)


@pytest.mark.parametrize("extra", [
    dict(), dict(day_idx=2), dict(day_idx=[0, 3, 1]), dict(timestamps=np.array([5.0, 6.0, 5.0])),
    dict(portfolios=(np.full((3, 2), -1, np.int32), np.zeros(3, np.int32))),
    dict(portfolios=(torch.zeros(3, 2, dtype=torch.int64), torch.zeros(3, dtype=torch.int32)), day_idx=torch.zeros(3, dtype=torch.int64)),
    dict(exclude=[[51], [], [52]], return_embeddings=True),
], ids=["plain", "one_day", "days", "per_user_ts", "packed", "tensors", "exclude"])
def test_recommend_mv_on_a_cpu_model_is_an_error_not_a_fallback(cpu_model, extra):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    tgn, items, mv = cpu_model
    args = dict(GOOD, items=items, mv=mv)
    args.update(extra)
    with pytest.raises(_lib.PfoError):
        tgn.recommend(**args)


def test_recommend_mv_topk_validates_then_requires_a_gpu():
    ue, ie = torch.zeros(3, 8), torch.zeros(10, 8)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    good = dict(user_emb=ue, item_emb=ie, k=3, cand_stock=i32(10), returns=torch.zeros(2, 5, 29, dtype=torch.float64),
                day_idx=i32(3), port_idx=i32(3, 4), port_len=i32(3), gamma=2.0, lambda_mv=0.5)
    for kw in (dict(k=0), dict(k=65), dict(cand_stock=i32(9)), dict(cand_stock=torch.zeros(10, dtype=torch.int64)),
               dict(returns=torch.zeros(2, 5, 29)), dict(returns=torch.zeros(2, 5, 1, dtype=torch.float64)),
               dict(returns=torch.zeros(2, 5, 129, dtype=torch.float64)), dict(returns=torch.zeros(10, 29, dtype=torch.float64)),
               dict(day_idx=i32(2)), dict(day_idx=torch.zeros(3, dtype=torch.int64)), dict(port_idx=i32(2, 4)),
               dict(port_len=i32(2)), dict(port_idx=None), dict(user_block=i32(2)), dict(n_blocks=3),
               dict(item_ok=torch.ones(4, dtype=torch.uint8)), dict(excl_len=i32(3)), dict(user_emb=torch.zeros(3, 6)),
               dict(user_emb=ue.double())):
        with pytest.raises(ValueError):
            P.recommend_mv_topk(**dict(good, **kw))
    if not torch.cuda.is_available():
        with pytest.raises(_lib.PfoError):
            P.recommend_mv_topk(**good)


def test_ctypes_table_and_dispatcher_op():
    assert "pfo_recommend_mv_topk" in _lib.PROTOTYPES and len(_lib.PROTOTYPES["pfo_recommend_mv_topk"][1]) == 31
    assert hasattr(_lib.load(), "pfo_recommend_mv_topk") and _lib.load().pfo_abi_version() == 6
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        out = torch.ops.pfotgn.recommend_mv_topk(torch.empty(7, 8), torch.empty(20, 8), 5, torch.empty(10, dtype=torch.int32),
                                                 torch.empty(2, 5, 29, dtype=torch.float64), torch.empty(7, dtype=torch.int32),
                                                 2.0, 0.5, 2)
    assert [(tuple(t.shape), t.dtype) for t in out] == [((7, 5), torch.int32), ((7, 5), torch.float32), ((7, 5), torch.float64),
                                                        ((7,), torch.int32)]
