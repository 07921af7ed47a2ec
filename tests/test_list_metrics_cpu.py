"""Host side of the backtest (no GPU): the numpy restatement of ``pfo_list_metrics`` (``list_metrics_ref``) against the
reference's own values at depths its call sites never use (fixture g12, tools/make_golden.py) and at (1, 3, 5) against g9a; the
C symbol and its bounds (refused before any device pointer is looked at); every ``ValueError`` of ``backtest``; the dict builder."""
import ctypes as C
import importlib
import os
import re
import types

import numpy as np
import pytest
import torch

import pfotgnrec_amd as P
from pfotgnrec_amd import _lib
from pfotgnrec_amd.mv_sampler import log_returns
import finance_ref as F
import list_metrics_ref as LR
from conftest import REPO, load_golden

BT = importlib.import_module("pfotgnrec_amd.backtest")     # (the package attribute of that name is the function)


def check_invest(got, hi, lo, scale, ref, e_ref_max, what):
    """|got - extended-precision value| within finance_ref.invest_bar: 16x the reference's own largest fp64 error in the fixture,
    floored at 8 ulp of |new| + |old| - the project's rule, no new tolerance.  Signs (the '>0' shares) compare exactly."""
    err = np.abs((got - hi) - lo)
    bar = F.invest_bar(e_ref_max, scale)
    w = np.unravel_index((err - bar).argmax(), err.shape)
    msg = "%s: max error %.3g (the reference's own %.3g); worst value: error %.3g against its bar %.3g" % (what, err.max(), e_ref_max, err[w], bar[w])
    print(msg)
    assert np.all(err <= bar), msg
    assert np.array_equal(got > 0, ref > 0), what


def g12_arguments(g):
    rp, rf = log_returns(g["prices_past"]), log_returns(g["prices_future"])
    return (g["list_item"], None, g["truth"], tuple(int(c) for c in g["cutoffs"]), g["port_idx"], g["port_len"], int(g["upper_u"]),
            rp, g["day_idx"], rf, g["day_idx"])


# ---- the restatement against the reference

def test_restatement_against_g12():
    g = load_golden("g12_list_metrics")
    assert g["list_item"].shape == (100, 20) and g["cutoffs"].tolist() == [1, 2, 3, 5, 10, 20]
    assert np.abs((g["invest"] - g["invest_exact_hi"]) - g["invest_exact_lo"]).max() == float(g["e_ref_max"])
    rank, hits, ndcg, invest = LR.list_metrics(*g12_arguments(g))
    check_invest(invest, g["invest_exact_hi"], g["invest_exact_lo"], g["invest_scale"], g["invest"], float(g["e_ref_max"]),
                 "restatement vs g12")
    # ranking: the reference's recall_at_k / ndcg_at_k on the same lists
    assert np.array_equal(rank, g["rank"])
    assert np.array_equal(hits.astype(np.float64), g["recall"])
    assert np.allclose(ndcg, g["ndcg"], rtol=0, atol=1e-6)
    inside = g["truth"] >= 0
    where = np.array([np.flatnonzero(l == t)[0] if (l == t).any() else LR.RANK_NONE for l, t in zip(g["list_item"], g["truth"])])
    assert np.array_equal(rank[inside], where[inside]) and np.all(rank[~inside] == LR.RANK_NONE)
    assert {0, 19, LR.RANK_NONE} <= set(rank.tolist())
    one = np.arange(100) % 10 == 1                               # the portfolio is the first pick: exactly zero at cutoff 1
    assert np.all(invest[one][:, [0, 6, 12, 18]] == 0)
    # the fixture covers what the issue asks of it
    n = g["port_len"]
    assert n.min() == 0 and n.max() == 7
    dup = [len(set(r[:m])) < m for r, m in zip(g["port_idx"], n)]
    held_in_list = [bool(np.isin(r[:m] + int(g["upper_u"]) + 1, l).any()) for r, m, l in zip(g["port_idx"], n, g["list_item"])]
    assert sum(dup) >= 10 and sum(held_in_list) >= 10


def test_restatement_against_g9a_at_1_3_5():
    """Cutoffs (1, 3, 5) on the canonical top-5 of g9a's rows: the twelve values the reference computes there."""
    g = load_golden("g9a_invest_metrics")
    U = int(g["upper_u"])
    codes = [str(c) for c in g["codes"]]
    mid = {c: i for i, c in enumerate(codes)}
    rp, rf = log_returns(g["prices_past"]), log_returns(g["prices_future"])
    pfs = [[str(c) for c in g["port_codes"][r, :g["port_n"][r]]] for r in range(len(g["port_n"]))]
    pidx, _, plen = P.evaluation.eval_portfolios(pfs, mid)
    lists = np.take_along_axis(g["cand"], g["canonical"][:, :5], 1)
    rank, hits, ndcg, invest = LR.list_metrics(lists, None, g["cand"][:, 0], (1, 3, 5), pidx, plen, U, rp, g["day_idx"], rf, g["day_idx"])
    e_ref = np.abs((g["invest"] - g["invest_exact_hi"]) - g["invest_exact_lo"]).max()
    check_invest(invest, g["invest_exact_hi"], g["invest_exact_lo"], g["invest_scale"], g["invest"], e_ref, "restatement vs g9a")
    assert np.array_equal(invest, F_rows(g, rp, rf, pfs, mid, U))
    # the place in the list is the canonical rank wherever that is below 5 and the positive's id occurs once among the five
    place = np.argmax(g["canonical"] == 0, axis=1)
    once = (lists == g["cand"][:, :1]).sum(1) == 1
    assert np.array_equal(rank[(place < 5) & once], place[(place < 5) & once])


def F_rows(g, rp, rf, pfs, mid, U):
    out = np.zeros((len(pfs), 12))
    for b, pf in enumerate(pfs):
        port = [] if "" in pf else [mid[c] for c in pf]
        out[b] = F.invest_metrics(rp[g["day_idx"][b]], rf[g["day_idx"][b]], port, (g["cand"][b] - U - 1)[g["canonical"][b]][:5])
    return out


def test_restatement_nan_rule_is_per_table():
    rs = np.random.RandomState(3)
    past, future = rs.randn(2, 6, 5) / 64, rs.randn(3, 4, 5) / 64
    lists = np.array([[11, 12, 13], [11, 15, 13], [11, 12, 13], [11, 12, 13]])       # upper_u = 10: stocks 0.., 15 -> stock 4
    day_p, day_f = np.array([0, 1, 2, 0]), np.array([2, 0, 1, 3])
    r, h, n, inv = LR.list_metrics(lists, None, np.array([12, 15, -1, 99]), (1, 2, 3), np.array([[0], [1], [5], [0]]), np.ones(4, int), 10,
                                   past, day_p, future, day_f)
    assert r.tolist() == [1, 1, LR.RANK_NONE, LR.RANK_NONE]
    assert np.isfinite(inv[0]).all()
    assert np.isfinite(inv[1, :6]).all() and np.isfinite(inv[1, [6, 9]]).all() and np.isnan(inv[1, [7, 8, 10, 11]]).all()   # stock 4: past only
    assert np.isnan(inv[2, :6]).all() and np.isnan(inv[2, 6:]).all()           # day 2 outside past; portfolio stock 5 outside future
    assert np.isfinite(inv[3, :6]).all() and np.isnan(inv[3, 6:]).all()        # day 3 outside future


# ---- the C symbol

def test_header_library_ctypes_table_and_dispatcher_declare_the_symbol():
    text = open(os.path.join(REPO, "include", "pfotgn.h")).read()
    m = re.search(r"\bint\s+pfo_list_metrics\s*\(([^;]*)\)\s*;", text)
    assert m, "include/pfotgn.h does not declare pfo_list_metrics"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    res, args = _lib.PROTOTYPES["pfo_list_metrics"]
    assert res is C.c_int and len(args) == len(params) == 27
    for p, a in zip(params, args):
        want = C.c_int32 if p.startswith("int32_t ") else C.c_int64 if p.startswith("int64_t ") else None
        if want is not None:
            assert a is want, p
        elif p == "const int32_t* cutoffs":
            assert a == C.POINTER(C.c_int32)
        else:
            assert "*" in p and a is _lib._VP, p
    lib = _lib.load()
    assert hasattr(lib, "pfo_list_metrics") and lib.pfo_abi_version() == 6
    assert hasattr(torch.ops.pfotgn, "list_metrics")
    from pfotgnrec_amd import build
    assert "backtest.hip" in build.SOURCES
    for name in ("list_metrics", "list_buffers", "backtest", "backtest_rows", "backtest_result_dict"):
        assert hasattr(P, name), name


GOOD = dict(U=1, L=10, cutoffs=(1, 3, 5, 10), port_stride=2, upper_u=10, pd=2, ps=5, fd=3, fs=4, n_ret=29, out_row0=0, out_rows=1)


def _call_with_null_pointers(**kw):
    a = dict(GOOD, **kw)
    lib = _lib.load()
    cuts = a["cutoffs"]
    n_c = a.get("n_c", 0 if cuts is None else len(cuts))
    arr = None if cuts is None else (C.c_int32 * max(len(cuts), 1))(*cuts)
    rc = lib.pfo_list_metrics(None, None, None, a["U"], a["L"], arr, n_c, None, None, a["port_stride"], a["upper_u"], None, None, a["pd"],
                              a["ps"], None, None, a["fd"], a["fs"], a["n_ret"], a["out_row0"], a["out_rows"], None, None, None, None, None)
    return rc, lib.pfo_last_error().decode()


@pytest.mark.parametrize("kw, msg", [
    (dict(U=-1), "U must be"), (dict(U=1 << 31, out_rows=1 << 32), "U must be"),
    (dict(L=0), "L must be"), (dict(L=65, cutoffs=(1,)), "L must be"), (dict(L=-4), "L must be"),
    (dict(cutoffs=(), n_c=0), "n_c must be"), (dict(cutoffs=tuple(range(1, 10))), "n_c must be"), (dict(n_c=-1), "n_c must be"),
    (dict(n_ret=1), "n_ret must be"), (dict(n_ret=129), "n_ret must be"), (dict(n_ret=0), "n_ret must be"),
    (dict(pd=0), "table sizes"), (dict(ps=0), "table sizes"), (dict(fd=-1), "table sizes"), (dict(fs=0), "table sizes"),
    (dict(port_stride=-1), "table sizes"),
    (dict(out_row0=-1), "exceed the output buffers"), (dict(out_row0=1), "exceed the output buffers"),
    (dict(U=3, out_rows=2), "exceed the output buffers"),
    (dict(cutoffs=None, n_c=2), "null cutoffs"),
    (dict(cutoffs=(0, 3)), "strictly increasing"), (dict(cutoffs=(1, 11)), "strictly increasing"), (dict(cutoffs=(3, 3)), "strictly increasing"),
    (dict(cutoffs=(5, 3)), "strictly increasing"), (dict(cutoffs=(-2,)), "strictly increasing"), (dict(L=4, cutoffs=(1, 5)), "strictly increasing")])
def test_every_bound_is_refused_before_a_device_pointer_is_read(kw, msg):
    rc, err = _call_with_null_pointers(**kw)
    assert rc != 0 and "pfo_list_metrics" in err and msg in err, (rc, err)


def test_bounds_that_hold_reach_the_pointer_check_and_no_rows_is_ok():
    for kw in (dict(), dict(L=1, cutoffs=(1,)), dict(L=64, cutoffs=tuple(range(57, 65))), dict(n_ret=2), dict(n_ret=128), dict(port_stride=0),
               dict(U=5, out_row0=3, out_rows=8)):
        rc, err = _call_with_null_pointers(**kw)
        assert rc != 0 and "null input" in err, (kw, rc, err)
    assert _call_with_null_pointers(U=0, out_rows=0)[0] == 0
    assert _call_with_null_pointers(U=0, out_row0=4, out_rows=4)[0] == 0
    assert _call_with_null_pointers(U=0, cutoffs=(2, 1))[0] != 0     # the bounds come first even then


def test_functional_refuses_on_the_host():
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32)
    tab = torch.zeros((2, 5, 29), dtype=torch.float64)
    good = dict(list_item=i32(3, 10), truth=i32(3), cutoffs=(1, 3), port_idx=i32(3, 2), port_len=i32(3), upper_u=10, ret_past=tab,
                day_past=i32(3), ret_future=tab, day_future=i32(3))
    for kw, msg in ((dict(list_item=i32(3, 65)), r"L must be"), (dict(list_item=i32(3, 10).long()), "int32"), (dict(cutoffs=(3, 1)), "increasing"),
                    (dict(cutoffs=(1, 11)), r"\[1, L\]"), (dict(cutoffs=()), "between 1 and 8"), (dict(cutoffs=range(1, 10)), "between 1 and 8"),
                    (dict(truth=i32(4)), "truth"), (dict(day_future=i32(3).long()), "day_future"), (dict(n_valid=i32(2)), "n_valid"),
                    (dict(port_idx=i32(4, 2)), "port_idx"), (dict(port_len=None), "port_len"),
                    (dict(ret_future=torch.zeros((2, 5, 30), dtype=torch.float64)), "returns per stock"),
                    (dict(ret_past=tab.float()), "float64"), (dict(ret_past=torch.zeros((2, 5, 1), dtype=torch.float64),
                                                                    ret_future=torch.zeros((2, 5, 1), dtype=torch.float64)), "n_ret must be"),
                    (dict(out_row0=2), "out_row0 without out"),
                    (dict(out=(i32(3), torch.zeros(3, 2), torch.zeros(3, 2), torch.zeros(3, 8)), out_row0=0), "list_buffers"),
                    (dict(out=(i32(3), torch.zeros(3, 2), torch.zeros(3, 2), torch.zeros(3, 8, dtype=torch.float64)), out_row0=1), "exceed")):
        with pytest.raises(ValueError, match=msg):
            P.list_metrics(**dict(good, **kw))


# ---- backtest: what it refuses, before any device work

def _log(n=8):
    return dict(sources=np.arange(1, n + 1), destinations=np.arange(21, 21 + n), edge_times=20200101000000.0 + np.arange(n),
                edge_idxs=np.arange(1, n + 1))


def _tables(upper_u=20):
    p = 100.0 + np.arange(2 * 4 * 6, dtype=np.float64).reshape(2, 4, 6)
    return P.InvestTables.from_prices(["20200101", "20200102"], p, p + 1.0, {"a": 0, "b": 1, "c": 2, "d": 3}, upper_u=upper_u)


def test_backtest_refusals_need_no_device():
    tgn = types.SimpleNamespace(holdings=None, device=torch.device("cuda:0"), n_nodes=40)
    items = np.arange(21, 25)
    base = dict(items=items, k=10, cutoffs=(1, 3, 5, 10), batch_size=4, tables=_tables())
    mv = types.SimpleNamespace(returns=np.zeros((2, 4, 5)), upper_u=19, gamma=2.0, lambda_mv=0.5, day_of=lambda t: np.zeros(len(t), int))
    ledger = P.PriceLedger(5, 20, "cpu")
    for kw, msg in ((dict(cutoffs=(1, 3, 3)), "strictly increasing"), (dict(cutoffs=(3, 1)), "strictly increasing"),
                    (dict(cutoffs=(0, 1)), r"\[1, k\]"), (dict(cutoffs=(1, 11)), r"\[1, k\]"), (dict(k=65, cutoffs=(1,)), r"k must be in \[1, 64\]"),
                    (dict(k=0, cutoffs=(1,)), r"k must be"), (dict(k=2.5), "k must be an integer"),
                    (dict(destinations=np.arange(21, 28)), "same length"), (dict(edge_idxs=np.arange(3)), "same length"),
                    (dict(batch_size=0), "batch_size must be at least 1"), (dict(batch_size=-5), "batch_size"),
                    (dict(tables=None), "InvestTables or a PriceLedger"), (dict(tables=(1, 2)), "InvestTables or a PriceLedger"),
                    (dict(tables=ledger, horizon=0), "horizon must be at least 1"), (dict(tables=ledger, horizon=-3), "horizon"),
                    (dict(horizon=3), "belongs to a PriceLedger"),
                    (dict(mv=mv, portfolios=[[0]] * 8), "number the stocks differently"),
                    (dict(tables=ledger, mv=mv, portfolios=[[0]] * 8), "number the stocks differently"),
                    (dict(mv=types.SimpleNamespace(**dict(mv.__dict__, upper_u=20))), "mv needs portfolios"),
                    (dict(basket=True), "basket=True needs mv"), (dict(exclude="held"), "holdings ledger"),
                    (dict(tables=_tables(None)), "upper_u is not known"), (dict(upper_u=7), "number the stocks differently"),
                    (dict(exclude=[[21]] * 7), "exclude lists 7 interactions")):
        args = dict(_log(), **base)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            P.backtest(tgn, **args)
        with pytest.raises(ValueError, match=msg):
            P.backtest_rows(tgn, **args)


def test_ledger_days_on_the_host():
    led = P.PriceLedger(3, 20, "cpu", max_days=4)
    # a ring state written by hand (no device call in this test): days 20200103 .. 06 live, the oldest in slot 2
    led.keys, led.head, led.n_days = [20200103, 20200104, 20200105, 20200106], 2, 4
    assert led.day_cap == 4
    ts = np.array([20200103e6, 20200104e6 + 5, 20200106e6, 20200102e6, 20200109e6])
    past, future = BT.ledger_days(led, ts, 2, "cpu")
    assert past.dtype == torch.int32 and past.tolist() == [2, 3, 1, -1, -1]
    assert future.tolist() == [0, 1, -1, -1, -1]                 # two trading days later; -1 where the ring does not reach, or no day at all


# ---- the dict builder

def test_result_dict_keys_counts_and_nan_rows():
    cuts = (1, 2, 4)
    rank = np.array([0, 1, 3, LR.RANK_NONE, 2])
    inv = np.arange(5 * 12, dtype=np.float64).reshape(5, 12) - 20.0
    inv[1, 6:] = np.nan                                          # row 1 misses the future table
    inv[3, :] = np.nan                                           # row 3 misses both
    inv[4, 8] = np.nan                                           # one NaN is enough: the row leaves the out-of-sample figures
    d = P.backtest_result_dict("bt", rank, inv, cuts)
    assert (d["n"], d["n_past"], d["n_future"]) == (5, 4, 2)
    want = {"bt_%s_avg_%d" % (m, c) for m in ("recall", "ndcg") for c in cuts}
    want |= {"bt_%s_%s_%d%s" % (m, s, c, t) for m in ("return", "sharpe") for s in ("avg", "percent") for c in cuts for t in ("", "_")}
    assert set(d) == want | {"n", "n_past", "n_future"}
    assert d["bt_recall_avg_1"] == 1 / 5 and d["bt_recall_avg_2"] == 2 / 5 and d["bt_recall_avg_4"] == 4 / 5
    nd = np.where(rank < 4, 1.0 / np.log2(rank + 2.0), 0.0)
    assert d["bt_ndcg_avg_4"] == np.mean(nd) and d["bt_ndcg_avg_1"] == 1 / 5
    past_rows, future_rows = [0, 1, 2, 4], [0, 2]
    for i, c in enumerate(cuts):
        assert d["bt_return_avg_%d" % c] == np.mean(np.ascontiguousarray(inv[past_rows, i]))
        assert d["bt_sharpe_avg_%d" % c] == np.mean(np.ascontiguousarray(inv[past_rows, 3 + i]))
        assert d["bt_return_avg_%d_" % c] == np.mean(np.ascontiguousarray(inv[future_rows, 6 + i]))
        assert d["bt_sharpe_percent_%d_" % c] == (inv[future_rows, 9 + i] > 0).sum() / 2
        assert d["bt_return_percent_%d" % c] == (inv[past_rows, i] > 0).sum() / 4
    none = P.backtest_result_dict("bt", rank, np.full((5, 12), np.nan), cuts)
    assert none["n_past"] == none["n_future"] == 0 and np.isnan(none["bt_return_avg_1"]) and np.isnan(none["bt_sharpe_percent_4_"])
    assert none["bt_recall_avg_4"] == 4 / 5
    with pytest.raises(ValueError, match="empty"):
        P.backtest_result_dict("bt", np.zeros(0, int), np.zeros((0, 12)), cuts)
    with pytest.raises(ValueError, match="invest must be"):
        P.backtest_result_dict("bt", rank, inv[:, :8], cuts)
