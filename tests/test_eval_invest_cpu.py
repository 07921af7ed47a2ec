"""Host side of the native eval_recommendation (no GPU): the numpy restatement of the investment metrics against the
reference's own values (fixtures g9a / g9b, tools/make_golden.py), the canonical top-k, and the loop's host logic."""
import numpy as np
import pytest

from conftest import load_golden
import finance_ref as F

from pfotgnrec_amd import _lib
from pfotgnrec_amd.mv_sampler import log_returns
from pfotgnrec_amd import evaluation as E


def _portfolios(g, rows=None):
    pc, pn = g["port_codes"], g["port_n"]
    rows = range(len(pn)) if rows is None else rows
    return [[str(c) for c in pc[r, :pn[r]]] for r in rows]


def _restated(g, ret_past, ret_future, day, portfolio, map_item_id, top_idx):
    port = [] if "" in portfolio else [map_item_id[c] for c in portfolio]
    return F.invest_metrics(ret_past[day], ret_future[day], port, top_idx, parts=True)


def _check_invest(got, g, rows=slice(None), what=""):
    """|got - exact| within invest_bar (16x the reference's own largest fp64 error in the fixture, floored at 8 ulp of
    |new| + |old|); prints both."""
    hi, lo, scale, ref = g["invest_exact_hi"][rows], g["invest_exact_lo"][rows], g["invest_scale"][rows], g["invest"][rows]
    e_ref = np.abs((g["invest"] - g["invest_exact_hi"]) - g["invest_exact_lo"]).max()
    err = np.abs((got - hi) - lo)
    bar = F.invest_bar(e_ref, scale)
    w = np.unravel_index((err - bar).argmax(), err.shape)
    msg = "%s: max error %.3g (the reference's own %.3g); worst value: error %.3g against its bar %.3g" % (what, err.max(), e_ref, err[w], bar[w])
    print(msg)
    assert np.all(err <= bar), msg
    assert np.array_equal(got > 0, ref > 0)                      # the '>0' shares compare exactly


def test_restatement_against_g9a():
    g = load_golden("g9a_invest_metrics")
    U = int(g["upper_u"])
    codes = [str(c) for c in g["codes"]]
    mid = {c: i for i, c in enumerate(codes)}
    rp, rf = log_returns(g["prices_past"]), log_returns(g["prices_future"])
    pfs = _portfolios(g)
    B = len(pfs)
    got = np.zeros((B, 12))
    for b in range(B):
        order = F.canonical_order(g["scores"][b])
        assert np.array_equal(order, g["canonical"][b])
        assert int(np.where(order == 0)[0][0]) == g["n_greater"][b] + g["n_equal"][b]
        got[b], _ = _restated(g, rp, rf, g["day_idx"][b], pfs[b], mid, (g["cand"][b] - U - 1)[order][:5])
        for i, k in enumerate((1, 3, 5)):
            assert F.tie_free(g["scores"][b], k) == g["tie_free"][b, i]
    _check_invest(got, g, what="restatement vs g9a")
    free = g["tie_free"].all(1)
    assert free.sum() * 2 >= B and np.array_equal(g["invest"][free], g["invest_ref_ranking"][free])
    one = np.arange(B) % 9 == 1                                  # the portfolio is the top-1 stock: exactly zero at k = 1
    assert np.all(got[one][:, [0, 3, 6, 9]] == 0)


@pytest.mark.parametrize("L", [1, 2])
def test_restatement_against_g9b(L):
    g = load_golden("g9b_eval_loop_L%d" % L)
    U, first = int(g["upper_u"]), int(g["eval_first"])
    codes = [str(c) for c in g["codes"]]
    mid = {c: i for i, c in enumerate(codes)}
    tables = E.InvestTables.from_prices([str(d) for d in g["days"]], g["prices_past"], g["prices_future"], mid)
    n = g["rank"].shape[0]
    pfs = _portfolios(g, range(first, first + n))
    day = tables.day_indices(g["ts_all"][first:first + n])
    negs = g["negatives"].reshape(n, -1)
    got = np.zeros((n, 12))
    for r in range(n):
        ids = np.concatenate(([g["dst_all"][first + r]], negs[r]))
        order = F.canonical_order(g["scores"][r])
        assert np.array_equal(order, g["canonical"][r]) and np.array_equal(ids[order][:5], g["top5_item"][r])
        assert int(np.where(order == 0)[0][0]) == g["rank"][r]
        got[r], _ = _restated(g, tables.returns_past, tables.returns_future, day[r], pfs[r], mid, (ids - U - 1)[order][:5])
    _check_invest(got, g, what="restatement vs g9b L%d" % L)
    # the dict from the rows: the investment keys are the reference's, recall / NDCG the canonical ones
    d = E.eval_result_dict("val", g["rank"], g["invest"])
    assert list(d) == [str(k) for k in g["result_keys"]]
    for k, ref, canon in zip(d, g["result_values"], g["canonical_values"]):
        if "recall" in k or "ndcg" in k:
            assert d[k] == canon and d[k] <= ref                 # the positive last among its ties: never better than the reference's
        else:
            assert d[k] == ref == canon, k


def test_batches_skip_the_last_and_test_run_stops_at_two():
    assert E.eval_batches(100, 24) == [(0, 24), (24, 48), (48, 72), (72, 96)]
    assert E.eval_batches(96, 24) == [(0, 24), (24, 48), (48, 72)]          # a full last batch is skipped as well
    assert E.eval_batches(100, 24, is_test_run=True) == [(0, 24), (24, 48)]
    assert E.eval_batches(48, 24, is_test_run=True) == [(0, 24)]
    assert E.eval_batches(10, 24) == []


def test_portfolio_with_an_empty_code_counts_as_empty():
    mid = {"000001": 0, "000002": 1, "000003": 2}
    idx, draw, invest = E.eval_portfolios([[""], ["000002"], ["000003", "", "000001"], ["000001", "000002", "000003"]], mid)
    assert draw.tolist() == [0, 1, 2, 3]                          # the candidate draw drops only the '' entries (utils.py:76)
    assert invest.tolist() == [0, 1, 0, 3]                        # evaluation.py:153: '' anywhere -> the whole list is empty
    assert idx[2, :2].tolist() == [2, 0] and idx[3].tolist() == [0, 1, 2]


def test_day_keys_are_the_first_eight_characters():
    mid = {"000001": 0}
    p = np.ones((2, 1, 30))
    t = E.InvestTables.from_prices(["20200101", "20200102"], p, p * 2, mid)
    assert t.day_indices(np.array([20200102093000.0, 20200101150000.0])).tolist() == [1, 0]
    with pytest.raises(KeyError):
        t.day_indices(np.array([20200103093000.0]))
    tf = {"20200102": {"000001": np.arange(1.0, 31.0)}, "20200101": {"000001": np.arange(2.0, 32.0)}}
    t2 = E.InvestTables(tf, tf, mid)
    assert t2.days == ["20200101", "20200102"] and t2.returns_past.shape == (2, 1, 29)
    assert np.array_equal(t2.returns_past[1, 0], np.log(np.arange(2.0, 31.0) / np.arange(1.0, 30.0)))
    with pytest.raises(ValueError):
        E.InvestTables(tf, {"20200101": tf["20200101"]}, mid)


def test_tables_from_the_reference_files(tmp_path):
    """evaluation.py:41-43: the three pickles under {root}/period_{p}/."""
    import pickle
    rs = np.random.RandomState(1)
    codes = ["000001", "000002", "000003"]
    mid = {c: i for i, c in enumerate(codes)}
    past = {d: {c: 50 + rs.rand(30) for c in codes} for d in ("20200102", "20200101")}
    future = {d: {c: 50 + rs.rand(30) for c in codes} for d in ("20200101", "20200102")}
    d = tmp_path / "data" / "period_30"
    d.mkdir(parents=True)
    for name, obj in (("time_feature_past_30.pkl", past), ("time_feature_future_30.pkl", future), ("map_item_id.pkl", mid)):
        with open(d / name, "wb") as f:
            pickle.dump(obj, f)
    t = E.InvestTables.from_files(30, root=str(tmp_path / "data"))
    assert t.days == ["20200101", "20200102"] and t.map_item_id == mid and t.n_items == 3
    p = past["20200102"]["000002"]
    assert np.array_equal(t.returns_past[1, 1], np.log(p[1:] / p[:-1]))
    p = future["20200101"]["000003"]
    assert np.array_equal(t.returns_future[0, 2], np.log(p[1:] / p[:-1]))


def test_result_dict_keys_and_order():
    rs = np.random.RandomState(0)
    rank = rs.randint(0, 9, 50)
    invest = rs.randn(50, 12)
    d = E.eval_result_dict("test", rank, invest)
    want = ["test_%s_avg_%d" % (m, k) for m in ("recall", "ndcg") for k in (1, 3, 5)]
    for suffix in ("", "_"):
        for m in ("return", "sharpe"):
            want += ["test_%s_%s_%d%s" % (m, kind, k, suffix) for kind in ("avg", "percent") for k in (1, 3, 5)]
    assert list(d) == want and len(d) == 30
    assert d["test_recall_avg_3"] == np.mean((rank < 3).astype(float))
    assert d["test_ndcg_avg_5"] == np.mean([1 / np.log2(r + 2) if r < 5 else 0.0 for r in rank])
    assert d["test_sharpe_avg_3_"] == np.mean([invest[i][10] for i in range(50)])
    assert d["test_return_percent_5"] == len([i for i in invest if i[2] > 0]) / 50
    with pytest.raises(ValueError):
        E.eval_result_dict("test", rank[:0], invest[:0])


def test_injected_negatives_forms():
    a = [np.full((3, 4), 7), np.full((3, 4), 8)]
    assert E._injected(a, 1, None, None, 3, 4)[0, 0] == 8
    seen = []

    def draw(k, sources, portfolios):
        seen.append((k, len(sources), len(portfolios)))
        return np.full((3, 4), k)
    assert E._injected(draw, 2, [1, 2, 3], [[""]] * 3, 3, 4)[2, 3] == 2 and seen == [(2, 3, 3)]
    with pytest.raises(ValueError):
        E._injected(a, 0, None, None, 3, 5)


def test_eval_recommendation_without_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import pfotgnrec_amd as P
    from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
    g = make_graph(SyntheticConfig("t", 50, 10, 400, 8, 1, 4, 2, n_days=2))
    nf = P.get_neighbor_finder(g.data, False)
    tgn = P.TGN(nf, g.node_features, g.edge_features, "cpu", n_layers=1, n_heads=2, use_memory=True, memory_dimension=8,
                message_function="identity")
    tables = P.InvestTables.from_prices(["0", "1"], g.prices, g.prices, g.map_item_id)
    with pytest.raises(_lib.PfoError):
        P.eval_recommendation(tgn, g.data, g.data, 24, 4, g.upper_u, 30, False, "val", tables=tables)
    with pytest.raises(_lib.PfoError):
        P.eval_metrics(torch.zeros(8, 8), 2, 2, None, None, None, None, None, None, 0)
