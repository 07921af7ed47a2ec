"""GPU parity of the evaluation in a served order (``pfo_eval_metrics_mv`` / ``eval_recommendation(order=)``): against
``pfo_eval_metrics`` where the two must agree (lambda = 0), against the numpy reference ``eval_mv_ref`` on exact cases, against
the two serving kernels, on random normal embeddings with the reference fed the kernel's own scores, and end to end on the small
model of ``test_gpu_eval_invest.py``.  No tolerance beyond ``finance_ref.invest_bar`` and the fp32 dot-product bound."""
import numpy as np
import pytest
import torch

from conftest import load_golden, has_gpu
import finance_ref as F
import eval_mv_ref as V

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

import pfotgnrec_amd as P
from pfotgnrec_amd import evaluation as E
from test_gpu_eval_invest import _g9b_data, _g9b_model, _g9b_reset

DEV = "cuda:0"
NONE = V.RANK_NONE
NAMES = ("rank", "recall", "ndcg", "top5_pos", "top5_item", "invest", "top5_fused", "n_adm", "score", "y", "fused")
CANARY = -7


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)


def _inputs(c):
    return (_dev(c["emb"], np.float32), c["B"], c["n_neg"], _dev(c["cand"], np.int32), _dev(c["day_idx"], np.int32),
            _dev(c["port_idx"], np.int32), _dev(c["port_len"], np.int32), _dev(c["ret_past"], np.float64), _dev(c["ret_future"], np.float64),
            c["upper_u"])


def run_mv(c, lam, mode, row0=2, spare=3, inputs=None):
    """The kernel on a case, written at ``row0`` into canary-filled buffers of B + row0 + spare rows: dict of host arrays (the
    rows of this call), after checking that no other row was touched."""
    B = c["B"]
    out = P.eval_buffers_mv(B + row0 + spare, DEV)
    for o in out:
        o.fill_(CANARY)
    res = P.eval_metrics_mv(*(inputs or _inputs(c)), _dev(c["ret_mv"], np.float64), _dev(c["mv_day_idx"], np.int32), c["gamma"], lam,
                            mode, out=out, out_row0=row0, want_all=True)
    for o in out:
        assert bool((o[:row0] == CANARY).all()) and bool((o[row0 + B:] == CANARY).all())
    return {k: v.cpu().numpy() for k, v in zip(NAMES, res)}


def check_ranking_follows(got):
    """recall / NDCG are functions of the rank, as in pfo_eval_metrics; RANK_NONE is a miss at every k."""
    hits, ndcg = V.hits_ndcg(got["rank"])
    assert np.array_equal(got["recall"], hits)
    assert np.allclose(got["ndcg"], ndcg, rtol=0, atol=1e-6) and np.array_equal(got["ndcg"] == 0, ndcg == 0)


# ---- 1: lambda = 0 against pfo_eval_metrics

# (B, n_neg, D, n_ret, mv_ret): every B, n_neg, D and table length the kernel takes another path at, each at least once
SHAPES = [(1, 1, 4, 2, 2), (3, 4, 172, 29, 29), (3, 5, 256, 128, 128), (1, 63, 172, 29, 2), (3, 64, 4, 2, 29), (3, 65, 256, 29, 128),
          (1, 255, 172, 128, 29), (3, 256, 4, 29, 29), (3, 2047, 172, 29, 29), (1, 2047, 256, 2, 128)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-n%d-D%d-r%d-m%d" % s)
def test_lambda_zero_is_pfo_eval_metrics(shape):
    """Random normal embeddings, every candidate admissible: at lambda = 0 the fused value is the rank of the score, so rank,
    hits, NDCG, top-5 and the twelve investment values are pfo_eval_metrics's, bit for bit, in both modes - but that the
    basket's rank is censored at 5 (its contract), which changes no hit and no NDCG value."""
    B, n_neg, D, n_ret, mv_ret = shape
    c = V.clean_case(100 + n_neg + D, B, n_neg, D, n_ret, mv_ret)
    inputs = _inputs(c)
    base = [t.cpu().numpy() for t in P.eval_metrics(*inputs)]
    for mode in (0, 1):
        got = run_mv(c, 0.0, mode, inputs=inputs)
        assert (got["n_adm"] == 1 + n_neg).all()
        want_rank = base[0] if mode == 0 else np.where(base[0] < 5, base[0], NONE)
        assert np.array_equal(got["rank"], want_rank), mode
        for name, ref in zip(NAMES[1:5], base[1:5]):
            assert np.array_equal(got[name], ref), (mode, name)
        assert np.array_equal(got["invest"], base[5], equal_nan=True), mode


# ---- 2: against the reference on exact cases

@pytest.fixture(scope="module", params=V.EXACT_CASES, ids=lambda s: "seed%d" % s[0])
def exact(request):
    """(case, fp64 scores - exact in fp32 too -, the reference per (lambda, mode), the extended-precision investment values)."""
    c = V.case(request.param)
    s = V.scores64(c["emb"], c["B"], c["n_neg"])
    refs = {(lam, mode): V.reference(c, lam, mode, s) for lam in V.LAMBDAS for mode in (0, 1)}
    return c, s, refs


def check_invest(got, c, ref):
    """The existing rule of test_gpu_eval_invest.py: within ``finance_ref.invest_bar`` of the extended-precision value, the bar
    from the reference's own fp64 error over these rows; NaN in the same places."""
    exact, _ = V.invest_rows(c, ref["top5_item"], dtype=np.longdouble)
    nan = np.isnan(ref["invest"])
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(np.isnan(exact.astype(np.float64)), nan)
    ok = ~nan
    e_ref = np.abs(ref["invest"][ok] - exact[ok]).astype(np.float64).max() if ok.any() else 0.0
    err = np.abs(got[ok] - exact[ok]).astype(np.float64)
    bar = F.invest_bar(e_ref, ref["invest_scale"][ok])
    msg = "max error %.3g (the reference's own %.3g), worst against its bar: %.3g" % (err.max() if ok.any() else 0.0, e_ref,
                                                                                    (err - bar).max() if ok.any() else 0.0)
    print(msg)
    assert np.all(err <= bar), msg


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("lam", V.LAMBDAS)
def test_against_the_reference(exact, lam, mode):
    c, s, refs = exact
    ref = refs[lam, mode]
    got = run_mv(c, lam, mode)
    assert np.array_equal(got["score"].astype(np.float64), s)
    for name in ("rank", "top5_pos", "top5_item", "top5_fused", "n_adm"):
        assert np.array_equal(got[name], ref[name]), name
    assert np.array_equal(got["y"], ref["y"], equal_nan=True) and np.array_equal(got["fused"], ref["fused"], equal_nan=True)
    check_ranking_follows(got)
    check_invest(got["invest"], c, ref)
    if c["B"] >= 14:                                                # the special rows took part
        assert got["rank"][0] == got["rank"][1] == NONE and (got["n_adm"][[2, 3, 8]] == 0).all()
        assert got["n_adm"][9] == 3 and got["n_adm"][10] == 5 and (got["top5_pos"][9, 3:] == -1).all()


# ---- 3: kernel against kernel

@pytest.mark.parametrize("mode", [0, 1])
def test_against_the_serving_kernels(exact, mode):
    """One interaction at a time as a one-user query: mode 0 is pfo_recommend_mv_topk(k = 5), mode 1 pfo_recommend_basket_topk(k = 5)
    in positions and fused values.  The embeddings are small integers: both scoring paths are exact, so they agree."""
    c, s, refs = exact
    B, n_neg = c["B"], c["n_neg"]
    got = run_mv(c, 0.5, mode)
    emb = _dev(c["emb"], np.float32)
    ret_mv = _dev(c["ret_mv"], np.float64)
    serve = P.recommend_basket_topk if mode else P.recommend_mv_topk
    for b in (range(B) if B <= 20 else (0, B - 1)):
        items = torch.cat([emb[B + b:B + b + 1], emb[2 * B + b * n_neg:2 * B + (b + 1) * n_neg]])
        stock = _dev(c["cand"][b] - c["upper_u"] - 1, np.int32)
        pos, score, fused, n_valid = serve(emb[b:b + 1], items, 5, stock, ret_mv, _dev(c["mv_day_idx"][b:b + 1], np.int32),
                                           _dev(c["port_idx"][b:b + 1], np.int32), _dev(c["port_len"][b:b + 1], np.int32), c["gamma"], 0.5)
        assert np.array_equal(pos.cpu().numpy()[0], got["top5_pos"][b]), b
        assert np.array_equal(fused.cpu().numpy()[0], got["top5_fused"][b]), b
        assert int(n_valid[0]) == (got["top5_pos"][b] >= 0).sum(), b


# ---- 4: random normal embeddings

@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("spec", V.EXACT_CASES, ids=lambda s: "seed%d" % s[0])
def test_normal_embeddings_with_the_kernels_own_scores(spec, mode):
    """lambda = 0.5 on random normal embeddings: every score within the fp32 dot-product bound of the fp64 product (the eps of
    ``recommend_ref``), and the reference fed the kernel's scores reproduces every integer output and top5_fused."""
    c = V.case(spec)
    c["emb"] = np.random.RandomState(spec[0]).randn(*c["emb"].shape).astype(np.float32)
    got = run_mv(c, 0.5, mode)
    s64, eps = V.scores64(c["emb"], c["B"], c["n_neg"]), V.dot_error_bound(c["emb"], c["B"], c["n_neg"])
    assert np.all(np.abs(got["score"].astype(np.float64) - s64) <= eps)
    ref = V.reference(c, 0.5, mode, got["score"])
    for name in ("rank", "top5_pos", "top5_item", "top5_fused", "n_adm"):
        assert np.array_equal(got[name], ref[name]), name
    assert np.array_equal(got["fused"], ref["fused"], equal_nan=True)
    check_ranking_follows(got)


# ---- 5: end to end

@pytest.fixture(scope="module")
def loop():
    g = load_golden("g9b_eval_loop_L1")
    tgn = _g9b_model(g)
    data, full, tables, mid = _g9b_data(g)
    B, K, U = int(g["batch"]), int(g["K"]), int(g["upper_u"])

    def run(order, mv=None):
        _g9b_reset(tgn, g)
        rows = E.eval_recommendation_rows(tgn, data, full, B, K, U, 30, False, tables=tables, negatives=list(g["negatives"]),
                                          order=order, mv=mv)
        m = tgn.memory
        return rows, (m.memory.clone(), m.last_update.clone(), m.msg_table.clone(), m.has_msg.clone())

    def sampler(lam):
        return P.MVSampler(g["prices_past"], U, DEV, gamma=2.0, lambda_mv=lam, day_of=tables.day_indices)
    return g, run, sampler, run("score"), (tgn, data, full, tables, B, K, U)


SHARED = ("rank", "recall", "ndcg", "top5_pos", "top5_item", "invest")


@pytest.mark.parametrize("order", ["mv", "basket"])
def test_eval_recommendation_in_a_served_order(loop, order):
    g, run, sampler, (score_rows, score_state), (tgn, data, full, tables, B, K, U) = loop
    n = score_rows["rank"].shape[0]
    cand = np.concatenate([data.destinations[:n, None], g["negatives"].reshape(n, -1)], 1)
    # lambda_mv = 0: the rows of the score order (every stock of the fixture moves, so every candidate is admissible) - the
    # basket's rank censored at 5, which no recall or NDCG value sees
    rows, state = run(order, sampler(0.0))
    assert sorted(rows) == sorted(SHARED + ("top5_fused", "n_adm")) and (rows["n_adm"] == cand.shape[1]).all()
    for name in SHARED:
        want = score_rows[name]
        if name == "rank" and order == "basket":
            want = np.where(want < 5, want, NONE)
        assert np.array_equal(rows[name], want, equal_nan=name == "invest"), name
    for a, b in zip(state, score_state):
        assert torch.equal(a, b)                                    # memory and last_update: bitwise the score pass's
    # lambda_mv = 0.5
    mv = sampler(0.5)
    rows, state = run(order, mv)
    for a, b in zip(state, score_state):
        assert torch.equal(a, b)
    for r in range(n):
        rank, pos = int(rows["rank"][r]), rows["top5_pos"][r]
        assert (rank < 5) == (0 in pos.tolist()) and (rank >= 5 or pos[rank] == 0), r
        assert rank < cand.shape[1] or rank == NONE
        live = pos >= 0
        assert np.array_equal(rows["top5_item"][r][live], cand[r][pos[live]]) and (rows["top5_item"][r][~live] == -1).all(), r
    assert not np.array_equal(rows["top5_pos"], score_rows["top5_pos"])     # the order did change something
    # the public entry: the reference's 30 keys
    _g9b_reset(tgn, g)
    d = P.eval_recommendation(tgn, data, full, B, K, U, 30, False, "val", tables=tables, negatives=list(g["negatives"]), order=order, mv=mv)
    assert list(d) == [str(k) for k in g["result_keys"]] and len(d) == 30
    assert d == E.eval_result_dict("val", rows["rank"], rows["invest"])
    # a price ledger seeded from the sampler's prices gives the sampler's rows
    ledger = P.PriceLedger.from_prices([int(k) for k in g["days"]], g["prices_past"], U, DEV, gamma=2.0, lambda_mv=0.5, key_divisor=1.0)
    ledger.reserve(n_days=ledger.n_days + 3, n_stocks=ledger.n_stocks + 2)      # capacity beyond the live table
    rows_l, _ = run(order, ledger)
    for name in rows:
        assert np.array_equal(rows_l[name], rows[name], equal_nan=True), name
