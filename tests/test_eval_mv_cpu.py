"""Host side of the evaluation in a served order (``pfo_eval_metrics_mv`` / ``eval_recommendation(order=)``): the C symbol and
its bounds (refused before any pointer is looked at, so no device is needed), the identities of the numpy reference
(``eval_mv_ref``) on exact cases, a hand-built row on which the two modes differ, and every ``ValueError`` of the Python layers
on a host model."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import pfotgnrec_amd as P
from pfotgnrec_amd import _lib
from pfotgnrec_amd import evaluation as E
from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
import finance_ref as F
import recommend_mv_ref as M
import eval_mv_ref as V
from conftest import REPO


# ---- the C symbol

def test_header_library_and_ctypes_table_declare_the_symbol():
    text = open(os.path.join(REPO, "include", "pfotgn.h")).read()
    m = re.search(r"\bint\s+pfo_eval_metrics_mv\s*\(([^;]*)\)\s*;", text)
    assert m, "include/pfotgn.h does not declare pfo_eval_metrics_mv"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    base = re.search(r"\bint\s+pfo_eval_metrics\s*\(([^;]*)\)\s*;", text)
    base_params = [" ".join(p.split()) for p in base.group(1).split(",")]
    assert params[:23] == base_params[:23] and params[-1] == base_params[-1] == "void* stream"
    assert params[23:-1] == ["const double* ret_mv", "int32_t mv_days", "int32_t mv_stocks", "int32_t mv_ret", "const int32_t* mv_day_idx",
                             "double gamma", "double lambda_mv", "int32_t mode", "double* top5_fused", "int32_t* n_adm",
                             "float* score_out", "double* y_out", "double* fused_out"]
    assert re.search(r"#define\s+PFO_EVAL_RANK_NONE\s+2147483647\b", text)
    res, args = _lib.PROTOTYPES["pfo_eval_metrics_mv"]
    base_args = _lib.PROTOTYPES["pfo_eval_metrics"][1]
    assert res is C.c_int and len(args) == len(params) == 37
    assert args[:23] == base_args[:23] and args[23:] == [_lib._VP, C.c_int32, C.c_int32, C.c_int32, _lib._VP, C.c_double, C.c_double,
                                                         C.c_int32] + [_lib._VP] * 6
    assert _lib.EVAL_RANK_NONE == 2 ** 31 - 1 == V.RANK_NONE
    lib = _lib.load()
    assert hasattr(lib, "pfo_eval_metrics_mv") and lib.pfo_abi_version() == 6


GOOD = dict(B=1, D=8, n_neg=4, port_stride=2, n_days=2, n_stocks=5, n_ret=29, upper_u=10, out_row0=0, out_rows=1, mv_days=2,
            mv_stocks=5, mv_ret=29, gamma=2.0, lambda_mv=0.5, mode=0)


def _call_with_null_pointers(**kw):
    a = dict(GOOD, **kw)
    lib = _lib.load()
    rc = lib.pfo_eval_metrics_mv(None, a["B"], a["D"], a["n_neg"], None, None, None, None, a["port_stride"], None, None, a["n_days"],
                                 a["n_stocks"], a["n_ret"], a["upper_u"], a["out_row0"], a["out_rows"], None, None, None, None, None,
                                 None, None, a["mv_days"], a["mv_stocks"], a["mv_ret"], None, a["gamma"], a["lambda_mv"], a["mode"],
                                 None, None, None, None, None, None)
    return rc, lib.pfo_last_error().decode()


@pytest.mark.parametrize("kw, msg", [
    (dict(B=-1), "multiple of 4"), (dict(D=0), "multiple of 4"), (dict(D=6), "multiple of 4"), (dict(D=260), "at most 256"),
    (dict(n_neg=0), "n_neg"), (dict(n_neg=2048), "n_neg"), (dict(n_neg=-3), "n_neg"),
    (dict(n_ret=0), "n_ret must be"), (dict(n_ret=129), "n_ret must be"), (dict(mv_ret=1), "mv_ret"), (dict(mv_ret=129), "mv_ret"),
    (dict(n_days=0), "table sizes"), (dict(n_stocks=0), "table sizes"), (dict(port_stride=-1), "table sizes"),
    (dict(mv_days=0), "table sizes"), (dict(mv_stocks=-2), "table sizes"), (dict(mode=2), "mode"), (dict(mode=-1), "mode"),
    (dict(out_row0=-1), "exceed the output buffers"), (dict(out_row0=1), "exceed the output buffers"),
    (dict(B=3, out_rows=2), "exceed the output buffers")])
def test_every_bound_is_refused_before_a_pointer_is_read(kw, msg):
    rc, err = _call_with_null_pointers(**kw)
    assert rc != 0 and "pfo_eval_metrics_mv" in err and msg in err, (rc, err)


def test_bounds_that_hold_reach_the_pointer_check_and_no_rows_is_ok():
    for kw in (dict(), dict(n_neg=2047), dict(n_neg=1), dict(mv_ret=2), dict(mv_ret=128, n_ret=1), dict(mode=1), dict(D=256)):
        rc, err = _call_with_null_pointers(**kw)
        assert rc != 0 and "null input" in err, (kw, rc, err)
    assert _call_with_null_pointers(B=0, out_rows=0)[0] == 0
    assert _call_with_null_pointers(B=0, mode=3)[0] != 0          # the bounds come first even then


# ---- the reference's own identities

ALL_CASES = V.EXACT_CASES + V.SMALL_CASES


@pytest.fixture(scope="module", params=ALL_CASES, ids=lambda s: "seed%d" % s[0])
def exact(request):
    c = V.case(request.param)
    return c, V.scores64(c["emb"], c["B"], c["n_neg"])


def test_cases_keep_the_exactness_condition():
    assert len(ALL_CASES) >= 5
    for spec in ALL_CASES:
        c, mv_ret = V.case(spec), spec[4]
        held = max(len(M.portfolio(c["port_idx"], c["port_len"], b, c["ret_mv"].shape[1])) for b in range(c["B"]))
        pow2 = (mv_ret - 1) & (mv_ret - 2) == 0
        assert pow2 or held + 4 <= 7, spec


def test_lambda_zero_is_the_score_order_over_the_admissible(exact):
    """lambda = 0: fused is the rank of the score, so the order is ``finance_ref.canonical_order`` of the scores restricted to
    A(b), and the rank of an admissible positive is the number of admissible negatives scoring >= it - in both modes (the
    basket's censored at 5)."""
    c, s = exact
    r0, r1 = V.reference(c, 0.0, 0, s), V.reference(c, 0.0, 1, s)
    for b in range(c["B"]):
        adm = r0["adm"][b]
        order = F.canonical_order(s[b])
        order = order[adm[order]]
        want = np.full(5, -1)
        want[:min(5, len(order))] = order[:5]
        assert np.array_equal(r0["top5_pos"][b], want) and np.array_equal(r1["top5_pos"][b], want), b
        if adm[0]:
            rank = int((s[b, 1:][adm[1:]] >= s[b, 0]).sum())
            assert r0["rank"][b] == rank and r1["rank"][b] == (rank if rank < 5 else V.RANK_NONE), b
        else:
            assert r0["rank"][b] == r1["rank"][b] == V.RANK_NONE, b
        assert r0["n_adm"][b] == r1["n_adm"][b] == adm.sum()
    assert np.array_equal(r0["invest"], r1["invest"], equal_nan=True)


@pytest.mark.parametrize("lam", V.LAMBDAS)
def test_basket_is_five_single_picks_of_the_fused_list(exact, lam):
    c, s = exact
    got = V.reference(c, lam, 1, s)
    pos, fused = V.loop_of_single_picks(c, lam, s)
    assert np.array_equal(got["top5_pos"], pos) and np.array_equal(got["top5_fused"], fused)
    first = V.reference(c, lam, 0, s)
    assert np.array_equal(got["top5_pos"][:, 0], first["top5_pos"][:, 0]) and np.array_equal(got["fused"], first["fused"], equal_nan=True)
    for b in range(c["B"]):                                        # distinct picks, the empty slots behind them
        n = int((got["top5_pos"][b] >= 0).sum())
        assert len(set(got["top5_pos"][b, :n].tolist())) == n and (got["top5_pos"][b, n:] == -1).all()
        assert np.isneginf(got["top5_fused"][b, n:]).all()
        at = np.flatnonzero(got["top5_pos"][b] == 0)
        assert got["rank"][b] == (at[0] if len(at) and got["adm"][b, 0] else V.RANK_NONE)


def test_special_rows_are_what_they_claim():
    c = V.case(V.EXACT_CASES[0])
    s = V.scores64(c["emb"], c["B"], c["n_neg"])
    n_cand = 1 + c["n_neg"]
    for mode in (0, 1):
        r = V.reference(c, 0.5, mode, s)
        assert r["rank"][0] == r["rank"][1] == V.RANK_NONE and not r["adm"][0, 0] and not r["adm"][1, 0]
        for b in (2, 3, 8):
            assert r["n_adm"][b] == 0 and (r["top5_pos"][b] == -1).all() and r["rank"][b] == V.RANK_NONE
            assert np.isneginf(r["top5_fused"][b]).all() and np.isfinite(r["invest"][b]).all() == (len(V.invest_port(c, b)) > 0)
        assert r["n_adm"][9] == 3 and (r["top5_pos"][9] >= 0).sum() == 3 and r["n_adm"][10] == 5 and (r["top5_pos"][10] >= 0).all()
        assert np.isnan(r["invest"][6]).all() and not np.isnan(r["invest"][5]).any()
        assert r["n_adm"][11] == n_cand and len(set(r["fused"][11, 1:].tolist())) == 1       # one tie group across position 5
    hits, ndcg = V.hits_ndcg(r["rank"])
    assert not hits[0].any() and not ndcg[0].any()


def test_a_correlated_pair_fills_the_fused_list_and_not_the_basket():
    """Stocks 0 and 1 are the same series with the highest y, stock 2 is uncorrelated with them and ranks just below, stock 3 is
    a poor fourth.  lambda 1: the fused list opens with the pair; the basket takes stock 2 second, because with stock 1 held
    the twin carries its covariance."""
    a = np.array([3.0, -1.0, 3.0, -1.0, 3.0, -1.0, 3.0, -1.0, 1.0]) / 64.0
    b = np.array([34.0, 34.0, 14.0, 14.0, 34.0, 34.0, 14.0, 14.0, 24.0]) / 64.0
    d = np.array([-4.0, 4.0, 4.0, -4.0, -4.0, 4.0, 4.0, -4.0, 0.0]) / 64.0
    ret_mv = np.stack([a, a, b, d])[None]
    rs = np.random.RandomState(0)
    c = dict(B=1, n_neg=3, cand=np.arange(101, 105, dtype=np.int32)[None], upper_u=100, day_idx=np.zeros(1, np.int32),
             port_idx=np.zeros((1, 0), np.int32), port_len=np.zeros(1, np.int32), ret_past=rs.randn(1, 4, 9) * 0.01,
             ret_future=rs.randn(1, 4, 9) * 0.01, ret_mv=ret_mv, mv_day_idx=np.zeros(1, np.int32), gamma=2.0)
    s = np.zeros((1, 4))
    fused, basket = V.reference(c, 1.0, 0, s), V.reference(c, 1.0, 1, s)
    assert fused["y"][0].tolist() == [8.0, 8.0, 7.68, 0.0]
    assert fused["top5_pos"][0].tolist() == [1, 0, 2, 3, -1] and fused["rank"][0] == 1
    assert basket["top5_pos"][0, :2].tolist() == [1, 2] and sorted(basket["top5_pos"][0, :4].tolist()) == [0, 1, 2, 3]
    assert basket["top5_fused"][0, :2].tolist() == [3.5, 3.0]      # first of four, then first of three
    assert basket["rank"][0] == int(np.flatnonzero(basket["top5_pos"][0] == 0)[0]) >= 2
    assert np.array_equal(fused["invest"][0, [0, 3]], basket["invest"][0, [0, 3]])           # the same first pick


# ---- the Python layers, checked on the host before any device is asked for

def _good_args():
    B, n_neg, D = 3, 4, 8
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    tab = torch.zeros(2, 6, 29, dtype=torch.float64)
    return dict(emb=torch.zeros(B * (2 + n_neg), D), batch=B, n_neg=n_neg, cand=i32(B, 1 + n_neg), day_idx=i32(B), port_idx=i32(B, 4),
                port_len=i32(B), ret_past=tab, ret_future=tab, upper_u=10, returns_mv=torch.zeros(3, 5, 17, dtype=torch.float64),
                mv_day_idx=i32(B), gamma=2.0, lambda_mv=0.5, mode=0)


@pytest.mark.parametrize("kw", [
    dict(mode=2), dict(mode=-1), dict(mode="mv"), dict(mode=0.5),
    dict(n_neg=2048, emb=torch.zeros(3 * 2050, 8), cand=torch.zeros(3, 2049, dtype=torch.int32)), dict(n_neg=0),
    dict(returns_mv=torch.zeros(3, 5, 17)), dict(returns_mv=torch.zeros(3, 5, dtype=torch.float64)), dict(returns_mv=None),
    dict(returns_mv=torch.zeros(3, 5, 1, dtype=torch.float64)), dict(returns_mv=torch.zeros(3, 5, 129, dtype=torch.float64)),
    dict(returns_mv=torch.zeros(0, 5, 17, dtype=torch.float64)),
    dict(mv_day_idx=torch.zeros(2, dtype=torch.int32)), dict(mv_day_idx=torch.zeros(3, dtype=torch.int64)),
    dict(mv_day_idx=torch.zeros(3, 1, dtype=torch.int32)), dict(mv_day_idx=None),
    dict(ret_future=torch.zeros(2, 6, 28, dtype=torch.float64)), dict(cand=torch.zeros(3, 4, dtype=torch.int32)),
    dict(emb=torch.zeros(17, 8)), dict(emb=torch.zeros(18))], ids=lambda kw: ",".join(kw))
def test_eval_metrics_mv_validates_on_the_host(kw):
    with pytest.raises(ValueError):
        P.eval_metrics_mv(**dict(_good_args(), **kw))


def test_eval_metrics_mv_then_requires_a_gpu():
    if not torch.cuda.is_available():
        with pytest.raises(_lib.PfoError):                          # valid: only the device is missing - no fallback
            P.eval_metrics_mv(**_good_args())
        with pytest.raises(_lib.PfoError):
            P.eval_buffers_mv(4, "cpu")


@pytest.fixture(scope="module")
def cpu_model():
    g = make_graph(SyntheticConfig("t", 50, 10, 400, 8, 1, 4, 2, n_days=2))
    nf = P.get_neighbor_finder(g.data, False)
    tgn = P.TGN(nf, g.node_features, g.edge_features, "cpu", n_layers=1, n_heads=2, use_memory=True, memory_dimension=8,
                message_function="identity")
    tables = P.InvestTables.from_prices(["0", "1"], g.prices, g.prices, g.map_item_id)
    mv = types.SimpleNamespace(returns=torch.zeros(2, 10, 29, dtype=torch.float64), upper_u=g.upper_u, gamma=2.0, lambda_mv=0.5,
                               day_of=lambda ts: np.zeros(len(ts), np.int32))
    return tgn, g, tables, mv


def test_order_and_mv_are_validated_before_any_device_work(cpu_model):
    tgn, g, tables, mv = cpu_model
    run = lambda **kw: P.eval_recommendation(tgn, g.data, g.data, 24, 4, g.upper_u, 30, False, "val", tables=tables, **kw)
    for bad in ("fused", "", None, 0, "MV"):
        with pytest.raises(ValueError, match="order must be"):
            run(order=bad)
        with pytest.raises(ValueError, match="order must be"):
            run(order=bad, mv=mv)
    for order in ("mv", "basket"):
        with pytest.raises(ValueError, match="needs mv"):
            run(order=order)
        with pytest.raises(ValueError, match="upper_u"):
            run(order=order, mv=types.SimpleNamespace(**dict(vars(mv), upper_u=g.upper_u + 1)))
        with pytest.raises(ValueError, match="is missing"):
            run(order=order, mv=types.SimpleNamespace(returns=mv.returns, upper_u=g.upper_u))
        wide = types.SimpleNamespace(destinations=np.arange(2048))
        with pytest.raises(ValueError, match="at most 2047"):
            E.eval_recommendation_rows(tgn, g.data, wide, 24, 4, g.upper_u, 30, False, tables=tables, order=order, mv=mv)
        E.check_order(order, mv, g.upper_u, 2047)                   # the largest list is fine
    with pytest.raises(TypeError):
        P.eval_recommendation(tgn, g.data, g.data, 24, 4, g.upper_u, 30, False, "val", None, None, None, None, "mv")   # keyword-only
    E.check_order("score", None, g.upper_u, 10 ** 6)               # the score order knows no bound and needs no mv
    if not torch.cuda.is_available():
        for kw in (dict(), dict(order="score"), dict(order="mv", mv=mv), dict(order="basket", mv=mv)):
            with pytest.raises(_lib.PfoError):                      # valid: only the device is missing - no fallback
                run(**kw)


def test_the_day_conversion_is_written_once():
    """``recommend._assemble_mv`` and ``eval_recommendation_rows`` share ``recommend.mv_device_side``."""
    import inspect
    from pfotgnrec_amd import recommend as RC
    for fn in (RC._assemble_mv, E.eval_recommendation_rows):
        src = inspect.getsource(fn)
        assert "mv_device_side(" in src and "slots_of(" not in src
    ret, day = RC.mv_device_side(types.SimpleNamespace(returns=np.zeros((2, 3, 4))), "cpu", np.array([1, 0, 1]))
    assert ret.dtype == torch.float64 and tuple(ret.shape) == (2, 3, 4) and day.dtype == torch.int32 and day.tolist() == [1, 0, 1]
