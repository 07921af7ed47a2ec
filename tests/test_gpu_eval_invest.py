"""GPU parity of the fused evaluation kernel (pfo_eval_metrics) and of the native eval_recommendation: against the reference's
own values (fixtures g9a / g9b, tools/make_golden.py) and, at sizes the fixtures cannot cover, against tests/finance_ref.py."""
import numpy as np
import pytest
import torch

from conftest import load_golden, has_gpu
import finance_ref as F

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

import pfotgnrec_amd as P
from pfotgnrec_amd import evaluation as E
from pfotgnrec_amd.synthetic import CONFIGS, make_graph

DEV = "cuda:0"
RTOL_EMB = 1e-4      # BASELINE.json north_star: embeddings / memory within 1e-4 (max norm)


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-12)


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)


def _portfolios(g, rows=None):
    pc, pn = g["port_codes"], g["port_n"]
    rows = range(len(pn)) if rows is None else rows
    return [[str(c) for c in pc[r, :pn[r]]] for r in rows]


def _check_invest(got, g, what):
    """|got - extended-precision value| within finance_ref.invest_bar: 16x the reference's own largest fp64 error in the fixture,
    floored at 8 ulp of |new| + |old|.  Signs (the '>0' shares) compare exactly."""
    hi, lo, scale, ref = g["invest_exact_hi"], g["invest_exact_lo"], g["invest_scale"], g["invest"]
    e_ref = np.abs((ref - hi) - lo).max()
    err = np.abs((got - hi) - lo)
    bar = F.invest_bar(e_ref, scale)
    w = np.unravel_index((err - bar).argmax(), err.shape)
    msg = "%s: max error %.3g (the reference's own %.3g); worst value: error %.3g against its bar %.3g" % (what, err.max(), e_ref, err[w], bar[w])
    print(msg)
    assert np.all(err <= bar), msg
    assert np.array_equal(got > 0, ref > 0), what
    return err.max(), e_ref


def _g9a_inputs(g, D=8):
    s = g["scores"]
    B, N = s.shape[0], s.shape[1] - 1
    emb = np.zeros((B * (2 + N), D), np.float32)
    # the score k / 64 as a sum over all D components (every lane group's partial sums take part): source = 1/8 everywhere,
    # the other side 8 * score / D per component - all dyadic, exact in any order
    emb[:B, :] = 0.125
    emb[B:2 * B, :] = (s[:, 0] * 8 / D)[:, None]
    emb[2 * B:, :] = (s[:, 1:].reshape(-1) * 8 / D)[:, None]
    codes = [str(c) for c in g["codes"]]
    mid = {c: i for i, c in enumerate(codes)}
    tables = P.InvestTables.from_prices([str(d) for d in g["days"]], g["prices_past"], g["prices_future"], mid)
    pidx, _, plen = E.eval_portfolios(_portfolios(g), mid)
    return emb, B, N, tables, mid, pidx, plen


def test_eval_metrics_against_reference_fixture():
    """pfo_eval_metrics vs g9a: top-5 positions and ids bit-exact against the canonical ranking on ALL rows (ties across the
    top-1/3/5 boundaries, all-equal rows, the destination among its negatives, one stock drawn twice); rank / recall / NDCG as
    the g6 test states them; the twelve investment values of every row against the reference's return_sharpe_at_k."""
    g = load_golden("g9a_invest_metrics")
    emb, B, N, tables, mid, pidx, plen = _g9a_inputs(g)
    rp, rf = tables.device_tables(DEV)
    assert tables.day_indices(g["ts"]).tolist() == g["day_idx"].tolist()
    U = int(g["upper_u"])
    rank, hits, ndcg, tpos, titem, inv = P.eval_metrics(torch.from_numpy(emb).to(DEV), B, N, _dev(g["cand"], np.int32),
                                                        _dev(g["day_idx"], np.int32), _dev(pidx, np.int32), _dev(plen, np.int32), rp, rf, U)
    r = rank.cpu().numpy()
    canon = g["canonical"]
    assert np.array_equal(tpos.cpu().numpy(), canon[:, :5])
    assert np.array_equal(titem.cpu().numpy(), np.take_along_axis(g["cand"], canon[:, :5], 1))
    assert np.array_equal(r, g["n_greater"] + g["n_equal"])       # canonical tie policy: behind every negative that scores >= it
    assert np.array_equal(r, np.argmax(canon == 0, axis=1))
    hits, ndcg = hits.cpu().numpy(), ndcg.cpu().numpy()
    for i, k in enumerate((1, 3, 5)):
        assert np.array_equal(hits[:, i], (r < k).astype(np.float32))
        assert np.allclose(ndcg[:, i], np.where(r < k, 1.0 / np.log2(r + 2.0), 0.0), rtol=0, atol=1e-6)
    # the same through pfo_rank_metrics (unchanged)
    r0, h0, n0 = P.rank_metrics(torch.from_numpy(emb).to(DEV), B, N)
    assert torch.equal(r0, rank) and torch.equal(h0.cpu(), torch.from_numpy(hits)) and np.allclose(n0.cpu().numpy(), ndcg, rtol=0, atol=1e-6)
    got = inv.cpu().numpy()
    _check_invest(got, g, "pfo_eval_metrics vs g9a")
    one = np.arange(B) % 9 == 1                                   # the portfolio is the recommended stock: exactly zero at k = 1
    assert np.all(got[one][:, [0, 3, 6, 9]] == 0)


@pytest.mark.parametrize("D", [4, 64, 68, 172, 256])
def test_eval_metrics_row_widths(D):
    """Every float4-per-lane variant of the score loop (D = 172: three 16-byte loads per lane, the last partly masked)."""
    g = load_golden("g9a_invest_metrics")
    emb, B, N, tables, mid, pidx, plen = _g9a_inputs(g, D=4)
    wide = np.zeros((emb.shape[0], D), np.float32)
    rs = np.random.RandomState(D)
    # the score spread over the row: components that sum to 8 * score exactly (multiples of 1/8, all partial sums exact)
    parts = rs.randint(-16, 17, size=(emb.shape[0], D)).astype(np.float32) / 8
    parts[:, 0] += emb[:, :4].sum(1) - parts.sum(1)
    wide[:] = parts
    wide[:B] = 0.125
    rp, rf = tables.device_tables(DEV)
    out = P.eval_metrics(torch.from_numpy(wide).to(DEV), B, N, _dev(g["cand"], np.int32), _dev(g["day_idx"], np.int32),
                         _dev(pidx, np.int32), _dev(plen, np.int32), rp, rf, int(g["upper_u"]))
    assert np.array_equal(out[3].cpu().numpy(), g["canonical"][:, :5])
    assert np.array_equal(out[0].cpu().numpy(), g["n_greater"] + g["n_equal"])
    _check_invest(out[5].cpu().numpy(), g, "D=%d" % D)


def test_eval_metrics_rejects_bad_shapes():
    g = load_golden("g9a_invest_metrics")
    emb, B, N, tables, mid, pidx, plen = _g9a_inputs(g)
    rp, rf = tables.device_tables(DEV)
    args = (_dev(g["cand"], np.int32), _dev(g["day_idx"], np.int32), _dev(pidx, np.int32), _dev(plen, np.int32), rp, rf, int(g["upper_u"]))
    e = torch.from_numpy(emb).to(DEV)
    with pytest.raises(P._lib.PfoError, match="exceed the output buffers"):
        P.eval_metrics(e, B, N, *args, out=P.eval_buffers(B, DEV), out_row0=1)
    with pytest.raises(P._lib.PfoError, match="multiple of 4"):
        P.eval_metrics(torch.zeros(B * (2 + N), 6, device=DEV), B, N, *args)


def test_out_row0_accumulates_batches_in_one_buffer():
    """Two batches written into one set of buffers equal two separate calls."""
    g = load_golden("g9a_invest_metrics")
    emb, B, N, tables, mid, pidx, plen = _g9a_inputs(g)
    rp, rf = tables.device_tables(DEV)
    U, h = int(g["upper_u"]), 50

    def part(lo, hi):
        n = hi - lo
        e = np.concatenate([emb[lo:hi], emb[B + lo:B + hi], emb[2 * B + lo * N:2 * B + hi * N]])
        return (torch.from_numpy(e).to(DEV), n, N, _dev(g["cand"][lo:hi], np.int32), _dev(g["day_idx"][lo:hi], np.int32),
                _dev(pidx[lo:hi], np.int32), _dev(plen[lo:hi], np.int32), rp, rf, U)
    out = P.eval_buffers(B, DEV)
    for o in out:
        o.fill_(-7)
    P.eval_metrics(*part(0, h), out=out, out_row0=0)
    assert all(bool((o[h:] == -7).all()) for o in out)            # rows past the batch are untouched
    P.eval_metrics(*part(h, B), out=out, out_row0=h)
    a, b = P.eval_metrics(*part(0, h)), P.eval_metrics(*part(h, B))
    whole = P.eval_metrics(torch.from_numpy(emb).to(DEV), B, N, _dev(g["cand"], np.int32), _dev(g["day_idx"], np.int32),
                           _dev(pidx, np.int32), _dev(plen, np.int32), rp, rf, U)
    for o, x, y, w in zip(out, a, b, whole):
        assert torch.equal(o, torch.cat([x, y])) and torch.equal(o, w)


def _g9b_model(g):
    L, H, K = int(g["L"]), int(g["H"]), int(g["K"])
    nf = P.NeighborFinder.from_arrays(g["src_all"], g["dst_all"], g["eidx_all"], g["ts_all"], uniform=False)
    D = g["node_features"].shape[1]
    tgn = P.TGN(nf, g["node_features"], g["edge_features"], DEV, n_layers=L, n_heads=H, dropout=0.1, use_memory=True,
                memory_dimension=D, message_function="identity", n_neighbors=K)
    sd = tgn.state_dict()
    with torch.no_grad():
        for k in g.files:
            if k.startswith("sd_") and k[3:] in sd:
                sd[k[3:]].copy_(torch.from_numpy(g[k]))
    _g9b_reset(tgn, g)
    return tgn


def _g9b_reset(tgn, g):
    m = tgn.memory
    with torch.no_grad():
        m.memory.copy_(torch.from_numpy(g["memory0"]))
        m.last_update.copy_(torch.from_numpy(g["last_update0"]))
        m.msg_table.copy_(torch.from_numpy(g["msg_tab"]))
        m.msg_time.copy_(torch.from_numpy(g["msg_t"]))
        m.has_msg.copy_(torch.from_numpy((g["msg_cnt"] > 0).astype(np.uint8)))
    m._any_msg = bool((g["msg_cnt"] > 0).any())


def _g9b_data(g):
    first, n = int(g["eval_first"]), int(g["eval_n"])
    pf = np.empty(len(g["port_n"]), dtype=object)
    for e, p in enumerate(_portfolios(g)):
        pf[e] = p
    full = P.Data(g["src_all"], g["dst_all"], g["ts_all"], g["eidx_all"], portfolios=pf)
    sl = slice(first, first + n)
    data = P.Data(g["src_all"][sl], g["dst_all"][sl], g["ts_all"][sl], g["eidx_all"][sl], portfolios=pf[sl])
    codes = [str(c) for c in g["codes"]]
    mid = {c: i for i, c in enumerate(codes)}
    tables = P.InvestTables.from_prices([str(d) for d in g["days"]], g["prices_past"], g["prices_future"], mid)
    return data, full, tables, mid


@pytest.mark.parametrize("L", [1, 2])
def test_eval_recommendation_against_reference_loop(L):
    """The reference's eval_recommendation (evaluation.py:39-264, reference TGN on the CPU) with its candidate draws injected:
    per-interaction ranks and top-5 stocks exact, the twelve investment values per interaction and the 30-key dict within the
    bars, the memory after the pass within 1e-4."""
    g = load_golden("g9b_eval_loop_L%d" % L)
    tgn = _g9b_model(g)
    data, full, tables, mid = _g9b_data(g)
    B, K, U = int(g["batch"]), int(g["K"]), int(g["upper_u"])
    kw = dict(tables=tables, negatives=list(g["negatives"]))
    rows = E.eval_recommendation_rows(tgn, data, full, B, K, U, 30, False, **kw)
    n = g["rank"].shape[0]
    assert rows["rank"].shape[0] == n == 5 * B                    # the short last batch is skipped
    assert np.array_equal(rows["rank"], g["rank"])
    assert np.array_equal(rows["top5_item"], g["top5_item"])
    assert np.array_equal(rows["recall"].astype(np.float64), g["recall"])
    assert np.allclose(rows["ndcg"], g["ndcg"], rtol=0, atol=1e-6)
    err, e_ref = _check_invest(rows["invest"], g, "eval_recommendation rows vs g9b L%d" % L)
    m = tgn.memory
    assert relerr(m.memory.cpu().numpy(), g["after_memory"]) < RTOL_EMB
    assert np.array_equal(m.last_update.cpu().numpy(), g["after_last_update"])
    has = g["after_msg_cnt"] > 0
    assert np.array_equal(m.has_msg.cpu().numpy() > 0, has)
    assert relerr(m.msg_table.cpu().numpy()[has], g["after_msg_tab"][has]) < RTOL_EMB
    # the public entry, from the same state: the reference's dict
    _g9b_reset(tgn, g)
    tgn.train()
    d = P.eval_recommendation(tgn, data, full, B, K, U, 30, False, "val", tables=tables,
                              negatives=lambda k, sources, portfolios: g["negatives"][k])
    assert not tgn.training
    assert list(d) == [str(k) for k in g["result_keys"]] and len(d) == 30
    bar_avg = F.invest_bar(e_ref, g["invest_scale"]).max(0)       # a mean cannot be further off than its worst row
    for k, ref, canon in zip(d, g["result_values"], g["canonical_values"]):
        if "recall" in k:
            # the canonical order (the positive last among exact ties with its own duplicate among the negatives, where the
            # reference's unstable argsort places it anywhere among them): exact against the reference's functions under it
            assert d[k] == canon and d[k] <= ref, k
        elif "ndcg" in k:
            assert abs(d[k] - canon) <= 1e-6 and d[k] <= ref + 1e-6, k
        elif "percent" in k:
            assert d[k] == ref, k
        else:
            t, m_, i = k.endswith("_"), "sharpe" in k, (1, 3, 5).index(int(k.rstrip("_")[-1]))
            assert abs(d[k] - ref) <= bar_avg[t * 6 + m_ * 3 + i], (k, d[k], ref)
    # is_test_run stops at batch 2
    _g9b_reset(tgn, g)
    rows2 = E.eval_recommendation_rows(tgn, data, full, B, K, U, 30, True, **kw)
    assert rows2["rank"].shape[0] == 2 * B and np.array_equal(rows2["top5_item"], g["top5_item"][:2 * B])


def test_eval_recommendation_with_device_draws():
    """negatives=None: the candidates come from pfo_neg_draw with the reference's set semantics (never a stock of the user's
    portfolio, only stocks seen among full_data.destinations); 30 finite values; two runs bit-identical."""
    g = load_golden("g9b_eval_loop_L2")
    tgn = _g9b_model(g)
    data, full, tables, mid = _g9b_data(g)
    B, K, U = int(g["batch"]), int(g["K"]), int(g["upper_u"])
    runs = []
    for _ in range(2):
        _g9b_reset(tgn, g)
        runs.append(E.eval_recommendation_rows(tgn, data, full, B, K, U, 30, False, tables=tables))
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k
    rows = runs[0]
    seen = set(np.unique(full.destinations).tolist())
    for r in range(rows["rank"].shape[0]):
        held = {mid[c] + U + 1 for c in data.portfolios[r] if c}
        items = set(rows["top5_item"][r].tolist())
        assert items <= seen | {int(data.destinations[r])} and not (items - {int(data.destinations[r])}) & held
    _g9b_reset(tgn, g)
    d = P.eval_recommendation(tgn, data, full, B, K, U, 30, False, "test", tables=tables)
    assert len(d) == 30 and all(np.isfinite(v) for v in d.values())
    assert d == E.eval_result_dict("test", rows["rank"], rows["invest"])


def test_full_size_evaluation_batch_slice_invest_metrics():
    """One C2 evaluation batch slice: 64 interactions x all 500 items (32 128 roots, D = 172) with make_graph's synthetic
    prices and portfolios.  Investment metrics against tests/finance_ref.py fed the device's own top-5; the device's rank and
    top-5 against the scores recomputed in fp64 from the same embeddings, within the +-margin interval the oracle test
    (test_full_size_evaluation_batch_slice_against_oracle) uses."""
    cfg = CONFIGS["C2"]
    g = make_graph(cfg)
    d = g.data
    nf = P.get_neighbor_finder(d, uniform=False)
    torch.manual_seed(14)
    tgn = P.TGN(nf, g.node_features, g.edge_features, DEV, n_layers=cfg.n_layers, n_heads=cfg.n_heads, dropout=0.0,
                use_memory=True, memory_dimension=cfg.dim, message_function="identity", n_neighbors=cfg.n_neighbors)
    with torch.no_grad():
        tgn.memory.msg_table.normal_(0, 0.1); tgn.memory.memory.normal_(0, 0.1); tgn.memory.has_msg.fill_(1)
    tgn.eval()
    rs = np.random.RandomState(5)
    B, K, N, U = 64, cfg.n_neighbors, cfg.n_items, cfg.n_users
    s = 900000
    sb, db, tb, eb = d.sources[s:s + B], d.destinations[s:s + B], d.timestamps[s:s + B], d.edge_idxs[s:s + B]
    neg = np.tile(np.arange(U + 1, U + 1 + N), B).reshape(B, N)
    neg[:, :40] = rs.randint(U + 1, U + 1 + N, size=(B, 40))         # draws with replacement (utils.py:99-101)
    with torch.no_grad():
        se, de, ne = tgn.compute_temporal_embeddings(sb, db, neg.reshape(-1), tb, eb, K)
    emb = torch.cat([se, de, ne])
    future = g.prices * np.exp(np.cumsum(np.random.RandomState(6).randn(*g.prices.shape) * 0.01, axis=2))
    tables = P.InvestTables.from_prices(list(range(cfg.n_days)), g.prices, future, g.map_item_id)
    rp, rf = tables.device_tables(DEV)
    day = g.day_of(tb).astype(np.int32)
    pidx, plen = g.portfolio_idx[s:s + B], g.portfolio_len[s:s + B]
    assert plen.min() == 0 and plen.max() == 7
    cand = np.concatenate([db[:, None], neg], 1)
    rank, hits, ndcg, tpos, titem, inv = P.eval_metrics(emb, B, N, _dev(cand, np.int32), _dev(day, np.int32), _dev(pidx, np.int32),
                                                        _dev(plen, np.int32), rp, rf, U)
    r0, h0, n0 = P.rank_metrics(emb, B, N)
    e = emb.cpu().numpy().astype(np.float64)
    sc = np.concatenate([(e[:B] * e[B:2 * B]).sum(1)[:, None], np.einsum("bd,bkd->bk", e[:B], e[2 * B:].reshape(B, N, -1))], 1)
    eps = 2e-5 * np.abs(sc).max()
    pos, negs = sc[:, 0], sc[:, 1:]
    same = neg == db[:, None]                                         # the destination among its own negatives: an exact tie
    r_lo = ((negs > pos[:, None] + eps) & ~same).sum(1) + same.sum(1)
    r_hi = ((negs >= pos[:, None] - eps) & ~same).sum(1) + same.sum(1)
    gr, tp, ti = rank.cpu().numpy(), tpos.cpu().numpy(), titem.cpu().numpy()
    assert np.all((gr >= r_lo) & (gr <= r_hi)), (gr, r_lo, r_hi)
    assert (r_lo == r_hi).sum() >= B // 2
    assert np.all(np.abs(gr - r0.cpu().numpy()) <= r_hi - r_lo)       # another f32 summation order than pfo_rank_metrics
    for i, k in enumerate((1, 3, 5)):
        assert np.array_equal(hits.cpu().numpy()[:, i], (gr < k).astype(np.float32))
        assert np.allclose(ndcg.cpu().numpy()[:, i], np.where(gr < k, 1.0 / np.log2(gr + 2.0), 0.0), atol=1e-6)
    exact_rows, want, scale, exact = 0, [], [], []
    for b in range(B):
        assert np.array_equal(ti[b], cand[b][tp[b]]) and len(set(tp[b].tolist())) == 5
        # the j-th pick: no candidate outside the picks so far beats it by more than the margin, and it is within the margin of
        # the j-th best fp64 score; consecutive picks descend (up to the margin)
        order = F.canonical_order(sc[b])
        for j in range(5):
            assert abs(sc[b, tp[b, j]] - sc[b, order[j]]) <= eps, (b, j)
        exact_rows += bool(np.array_equal(tp[b], order[:5]))
        day_b = int(day[b])
        args = (tables.returns_past[day_b], tables.returns_future[day_b], pidx[b, :plen[b]], ti[b] - U - 1)
        w, sc_b = F.invest_metrics(*args, parts=True)
        want.append(w); scale.append(sc_b); exact.append(F.invest_metrics(*args, dtype=np.longdouble))
    want, scale, exact = np.stack(want), np.stack(scale), np.stack(exact)
    e_ref = np.abs(want - exact).astype(np.float64).max()             # the fp64 restatement's own error over the batch
    err = np.abs(inv.cpu().numpy() - exact).astype(np.float64)
    bar = F.invest_bar(e_ref, scale)
    w = np.unravel_index((err - bar).argmax(), err.shape)
    msg = "full size: max error %.3g (the restatement's own %.3g); worst value: error %.3g against its bar %.3g" % (err.max(), e_ref, err[w], bar[w])
    print(msg)
    assert np.all(err <= bar), msg
    assert exact_rows >= B // 2
