"""CPU-side tests of the position-weighted mean-variance order: the reference's own identities (all-ones weights are the
unweighted y bit for bit, a power-of-two scaling changes no bit, an uncounted holding is no holding), the host model of
``pfo_holdings_gather_weights`` against a dict loop, and every ValueError of ``recommend`` / ``backtest`` /
``functional`` - raised before a device is asked for."""
import importlib
import inspect
import types

import numpy as np
import pytest
import torch

import pfotgnrec_amd as P
from pfotgnrec_amd import _lib, recommend as RC
from pfotgnrec_amd.holdings import Holdings
from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
import recommend_mv_ref as M
import recommend_mv_weighted_ref as WR

BT = importlib.import_module("pfotgnrec_amd.backtest")


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ---- the arithmetic

@pytest.mark.parametrize("seed,n_ret", [(1, 2), (2, 29), (3, 30)])
def test_all_ones_weights_are_the_unweighted_y(seed, n_ret):
    c = M.mv_side(seed, 37, 40, n_ret)
    ones = np.ones(c["port_idx"].shape)
    want = M.y_matrix(c["returns"], c["day_idx"], c["cand_stock"], c["port_idx"], c["port_len"])
    got = WR.y_matrix(c["returns"], c["day_idx"], c["cand_stock"], c["port_idx"], c["port_len"], ones)
    assert np.array_equal(got, want, equal_nan=True) and _same(got, want)
    S = c["returns"].shape[1]
    for u in range(37):
        port = M.portfolio(c["port_idx"], c["port_len"], u, S)
        d = int(c["day_idx"][u])
        if 0 <= d < 3:
            cand = np.arange(1, S)
            assert np.array_equal(WR.y_mv(c["returns"], d, cand, port, np.ones(len(port))), M.y_mv(c["returns"], d, cand, port), equal_nan=True)
    assert (c["port_len"] >= 2).sum() > 10


def test_a_power_of_two_scaling_changes_no_bit():
    c = WR.weighted_side(4, 37, 40, 29)
    base = WR.y_of(c)
    for e in (-20, -1, 1, 33):
        scale = np.ldexp(1.0, e * (1 + np.arange(37) % 3))[:, None]
        got = WR.y_of(dict(c, port_w=c["port_w"] * scale))
        assert _same(got, base), e
    other = WR.y_of(dict(c, port_w=c["port_w"] * np.linspace(1.0, 3.0, 8)[None, :]))
    assert not _same(other, base), "the weights must matter"


def test_an_uncounted_holding_equals_the_row_without_it():
    c = WR.weighted_side(5, 37, 40, 29)
    base = WR.y_of(c)
    S = c["returns"].shape[1]
    idx, ln, w = (np.full((37, 8), -1, np.int32), np.zeros(37, np.int32), np.full((37, 8), np.nan))
    dropped = 0
    for u in range(37):
        stocks, ws = WR.portfolio(c["port_idx"], c["port_len"], c["port_w"], u, S)
        dropped += min(int(c["port_len"][u]), 8) - len(stocks)
        idx[u, :len(stocks)], w[u, :len(stocks)], ln[u] = stocks, ws, len(stocks)
        assert len(stocks) <= 7
    assert dropped >= 8 and ln[4] == 0 and ln[3] == 3 and ln[2] == 1
    assert _same(WR.y_of(dict(c, port_idx=idx, port_len=ln, port_w=w)), base)
    # user 4 holds three stocks in the table and no weight that counts: main.py:254, the y of a user who holds nothing
    empty = M.y_matrix(c["returns"], c["day_idx"], c["cand_stock"], None, None)
    assert _same(base[4], empty[4]) and not _same(base[3], empty[3])
    for bad in (0.0, -0.0, -3.0, np.nan, np.inf, -np.inf):
        assert not WR.counts(bad)
    assert WR.counts(5e-324) and WR.counts(np.finfo(np.float64).max)


@pytest.mark.parametrize("W", [1, 64, 256])
def test_the_gather_model_against_a_dict_loop(W):
    n_nodes, n_stocks = 50, 40
    g = WR.gather_case(10 + W, n_nodes, W, 33, n_stocks)
    for mode in (WR.SHARES, WR.VALUE):
        got = WR.gather_weights(g["users"], g["hold_idx"], g["hold_len"], g["hold_qty"], mode, g["last_close"])
        want = {}
        for q, u in enumerate(g["users"].tolist()):
            L = min(max(int(g["hold_len"][u]), 0), W) if 0 <= u < n_nodes else 0
            for j in range(W):
                v = 0.0
                if j < L:
                    v = float(g["hold_qty"][u, j])
                    if mode == WR.VALUE:
                        s = int(g["hold_idx"][u, j])
                        v = v * float(g["last_close"][s]) if 0 <= s < n_stocks else 0.0
                want[q, j] = v
        flat = np.array([want[q, j] for q in range(33) for j in range(W)]).reshape(33, W)
        assert np.array_equal(got, flat, equal_nan=True)
        if W > 1:
            assert (got == 0).any() and (got > 0).any() and (mode == WR.SHARES or np.isnan(got).any())
    assert ((g["users"] < 0) | (g["users"] >= n_nodes)).sum() == 5


# ---- recommend / backtest: checked on the host, before any device is asked for

@pytest.fixture(scope="module")
def cpu_model():
    g = make_graph(SyntheticConfig("t", 50, 10, 400, 8, 1, 4, 2), with_prices=False)
    nf = P.get_neighbor_finder(g.data, False)
    tgn = P.TGN(nf, g.node_features, g.edge_features, "cpu", n_layers=1, n_heads=2, use_memory=True, memory_dimension=8,
                message_function="identity")
    mv = types.SimpleNamespace(returns=torch.zeros(4, 10, 29, dtype=torch.float64), upper_u=50, gamma=2.0, lambda_mv=0.5,
                               day_of=lambda ts: np.asarray(ts, np.int64) % 4)
    return tgn, np.arange(51, 61), mv


def _ledger(quantities, upper_u=50):
    return Holdings(61, 61, 4, upper_u, "cpu", quantities=quantities)


def _refusals(call, mv, rows=3):
    ports = [[0], [], [1, 2]][:rows] + [[3]] * (rows - 3)
    w_ok = [[1.0], [], [2.0, 0.5]][:rows] + [[1.0]] * (rows - 3)
    led = P.PriceLedger(29, 50, "cpu")
    for kw, msg in (
            (dict(portfolio_weights=w_ok), "needs mv"),
            (dict(portfolio_weights="shares"), "needs mv"),
            (dict(mv=mv, portfolios=ports, portfolio_weights=w_ok, basket=True), "basket=True cannot be combined"),
            (dict(mv=mv, portfolios=ports, portfolio_weights=w_ok, groups=np.zeros(10, np.int32), group_cap=2), "no weighted form"),
            (dict(mv=mv, portfolios="seen", portfolio_weights=w_ok), "never sees"),
            (dict(mv=mv, portfolios=ports, portfolio_weights="cash"), "portfolio_weights must be"),
            (dict(mv=mv, portfolios=ports, portfolio_weights="shares"), 'needs portfolios="held"'),
            (dict(mv=mv, portfolios="held", holdings=_ledger(False), portfolio_weights="shares"), "keeps quantities"),
            (dict(mv=mv, portfolios="held", holdings=_ledger(False), portfolio_weights="value"), "keeps quantities"),
            (dict(mv=mv, portfolios="held", holdings=_ledger(True), portfolio_weights="value"), "PriceLedger"),
            (dict(mv=P.PriceLedger(29, 49, "cpu"), portfolios="held", holdings=_ledger(True), portfolio_weights="value", day_idx=0),
             "number the stocks differently"),
            (dict(mv=mv, portfolios="held", holdings=_ledger(True), portfolio_weights=np.ones((rows, 4))), "explicit portfolios"),
            (dict(mv=mv, portfolios=ports, portfolio_weights=w_ok[:-1]), "portfolio_weights lists %d" % (rows - 1)),
            (dict(mv=mv, portfolios=ports, portfolio_weights=[[1.0, 2.0]] + w_ok[1:]), "2 weights for user 0"),
            (dict(mv=mv, portfolios=ports, portfolio_weights=[["a"]] + w_ok[1:]), "portfolio_weights must be"),
            (dict(mv=mv, portfolios=ports, portfolio_weights=np.ones((rows, 3))), "has shape"),
            (dict(mv=mv, portfolios=ports, portfolio_weights=torch.ones(rows + 1, 2, dtype=torch.float64)), "has shape"),
            (dict(mv=mv, portfolios=ports, portfolio_weights=np.ones(rows)), "has shape"),
            (dict(mv=mv, portfolios=ports, portfolio_weights=np.ones((rows, 2), bool)), "must be numbers"),
            (dict(mv=mv, portfolios=(torch.zeros(rows, 2, dtype=torch.int32), torch.zeros(rows, dtype=torch.int32)), portfolio_weights=w_ok),
             "pass an f64"),
    ):
        with pytest.raises(ValueError, match=msg):
            call(**kw)
    assert led.upper_u == 50


def test_recommend_validates_the_weights_on_the_host(cpu_model):
    tgn, items, mv = cpu_model

    def call(holdings=None, **kw):
        tgn.holdings = holdings
        try:
            tgn.recommend([1, 2, 3], 5.0, 3, items, **kw)
        finally:
            tgn.holdings = None
    _refusals(call, mv)
    # what is valid gets as far as asking for the device
    if not torch.cuda.is_available():
        for kw in (dict(portfolios=[[0], [], [1, 2]], portfolio_weights=[[1.0], [], [2.0, 0.5]]),
                   dict(portfolios=[[0], [], [1, 2]], portfolio_weights=np.ones((3, 2))),
                   dict(portfolios=[[0], [], [1, 2]], portfolio_weights=None)):
            with pytest.raises(_lib.PfoError):
                tgn.recommend([1, 2, 3], 5.0, 3, items, mv=mv, **kw)
        tgn.holdings = _ledger(True)
        try:
            with pytest.raises(_lib.PfoError):
                tgn.recommend([1, 2, 3], 5.0, 3, items, mv=mv, portfolios="held", portfolio_weights="shares")
        finally:
            tgn.holdings = None
    q = RC.validate(61, 4, [1, 2, 3], 5.0, 3, items, None, None, None, mv, [[0], [], [1, 2]], portfolio_weights=[[1.5], [], [2.0, 0.5]])
    assert q.weights.dtype == np.float64 and q.weights.tolist() == [[1.5, 0.0], [0.0, 0.0], [2.0, 0.5]]
    assert RC.validate(61, 4, [1, 2, 3], 5.0, 3, items, None, None, None, mv, [[0], [], [1, 2]]).weights is None


def test_backtest_makes_the_same_checks_before_any_device_work(cpu_model):
    _, _, mv = cpu_model
    tables = P.InvestTables.__new__(P.InvestTables)
    tables.upper_u = 50
    log = (np.array([1, 2, 3]), np.array([56, 57, 58]), np.array([1.0, 2.0, 3.0]), np.array([1, 2, 3]))

    def call(mv=None, portfolios=None, day_idx=None, holdings=None, **kw):
        tgn = types.SimpleNamespace(holdings=holdings, device="cpu")
        for fn in (BT.backtest_rows, BT.backtest):
            try:
                fn(tgn, *log, np.arange(51, 61), 3, cutoffs=(1, 3), batch_size=2, tables=tables, mv=mv, portfolios=portfolios, **kw)
            except ValueError as e:
                err = e
            else:
                raise AssertionError("not refused")
        raise err
    _refusals(call, mv)
    if not torch.cuda.is_available():
        tgn = types.SimpleNamespace(holdings=None, device="cpu")
        with pytest.raises(_lib.PfoError):
            BT.backtest(tgn, *log, np.arange(51, 61), 3, cutoffs=(1, 3), batch_size=2, tables=tables, mv=mv, portfolios=[[0], [], [1, 2]],
                        portfolio_weights=[[1.0], [], [2.0, 0.5]])


def test_the_keyword_goes_by_name_and_defaults_to_none():
    for fn in (P.TGN.recommend, BT.backtest, BT.backtest_rows, RC.validate):
        p = inspect.signature(fn).parameters["portfolio_weights"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    for fn in (P.recommend_mv_topk, P.recommend_mv_topk_wide, P.recommend_list_mv_topk):
        assert inspect.signature(fn).parameters["port_w"].default is None
    assert "port_w" not in inspect.signature(P.recommend_basket_topk).parameters
    assert inspect.signature(P.holdings_gather_weights).parameters["last_close"].default is None
    for name in ("pfo_recommend_mv_topk", "pfo_recommend_mv_topk_wide", "pfo_recommend_list_mv_topk"):
        plain, weighted = _lib.PROTOTYPES[name][1], _lib.PROTOTYPES[name + "_weighted"][1]
        at = 19                                                        # port_len is argument 18 of all three
        assert weighted[:at] == plain[:at] and weighted[at + 1:] == plain[at:] and weighted[at] is plain[at - 1]


# ---- functional: a mis-shaped port_w is refused without a device

def _functional_args(U=5, I=7, D=8, W=3):
    return dict(user_emb=torch.zeros(U, D), item_emb=torch.zeros(I, D), k=2, cand_stock=torch.zeros(I, dtype=torch.int32),
                returns=torch.zeros(2, 4, 5, dtype=torch.float64), day_idx=torch.zeros(U, dtype=torch.int32),
                port_idx=torch.zeros(U, W, dtype=torch.int32), port_len=torch.zeros(U, dtype=torch.int32), gamma=2.0, lambda_mv=0.5)


@pytest.mark.parametrize("form", ["bounded", "wide", "list"])
def test_functional_refuses_a_misshaped_port_w(form):
    a = _functional_args()
    fn = {"bounded": P.recommend_mv_topk, "wide": P.recommend_mv_topk_wide, "list": P.recommend_list_mv_topk}[form]
    if form == "list":
        a.update(list_pos=torch.zeros(5, 2, dtype=torch.int32), list_len=torch.zeros(5, dtype=torch.int32))
    for bad in (torch.zeros(5, 2, dtype=torch.float64), torch.zeros(4, 3, dtype=torch.float64), torch.zeros(15, dtype=torch.float64),
                torch.zeros(5, 3), torch.zeros(5, 3, dtype=torch.int32), np.zeros((5, 3))):
        with pytest.raises(ValueError, match="port_w must be float64"):
            fn(port_w=bad, **a)
    with pytest.raises(ValueError, match="port_w without port_idx"):
        fn(port_w=torch.zeros(5, 3, dtype=torch.float64), **dict(a, port_idx=None, port_len=None))
    if form == "bounded":
        with pytest.raises(ValueError, match="no weighted form"):
            fn(port_w=torch.zeros(5, 3, dtype=torch.float64), cand_group=torch.zeros(7, dtype=torch.int32), group_cap=1, **a)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.PfoError):                              # well-shaped: as far as asking for the device
            fn(port_w=torch.zeros(5, 3, dtype=torch.float64), **a)


def test_gather_weights_checks_its_arguments_on_the_host():
    idx, ln, qty = torch.zeros(6, 4, dtype=torch.int32), torch.zeros(6, dtype=torch.int32), torch.zeros(6, 4, dtype=torch.float64)
    users = torch.zeros(3, dtype=torch.int32)
    for args, msg in (((users, idx, ln, qty, "cash"), "mode must be"), ((users, idx, ln, qty, 2), "mode must be"),
                      ((users, idx, ln, None, "shares"), "quantities must be f64"), ((users, idx, ln, qty.float(), 0), "quantities must be f64"),
                      ((users, idx, ln, qty[:, :3], 0), "quantities must be f64"), ((users, idx, ln, qty, "value"), "needs last_close"),
                      ((users, idx, ln, qty, 1, torch.zeros(5)), "needs last_close"), ((users.long(), idx, ln, qty, 0), "users must be int32")):
        with pytest.raises(ValueError, match=msg):
            P.holdings_gather_weights(*args)
    with pytest.raises(ValueError, match="keeps quantities"):
        _ledger(False).gather_weights(users, "shares")
    if not torch.cuda.is_available():
        with pytest.raises(_lib.PfoError):
            _ledger(True).gather_weights(users, "shares")
