"""GPU tests of the backtest: ``pfo_list_metrics`` against the numpy restatement (``list_metrics_ref``), against
the reference's own values at depths its call sites never use (fixture g12), and bit for bit against ``pfo_eval_metrics`` /
``pfo_eval_metrics_mv`` at (1, 3, 5) on the lists those kernels wrote; ``backtest`` on a small served model against
``recommend`` / ``list_metrics`` / ``observe`` called by hand on twin models."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from conftest import load_golden, has_gpu
import finance_ref as F
import list_metrics_ref as LR

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

import pfotgnrec_amd as P
from pfotgnrec_amd import _lib
from pfotgnrec_amd import evaluation as E
from pfotgnrec_amd.mv_sampler import log_returns
from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph

BT = importlib.import_module("pfotgnrec_amd.backtest")
DEV = "cuda:0"
UPPER = 50


def _dev(a, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)


def _i32(a):
    return None if a is None else _dev(a, np.int32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


def _same_bits(a, b):
    """Bitwise, except that any NaN equals any NaN (the payload of an invalid operation is the hardware's)."""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all(nan | (_bits(a) == _bits(b))))


def _e_ref_max():
    return float(load_golden("g12_list_metrics")["e_ref_max"])


def _within_bar(got, args, what):
    """invest against the extended-precision restatement under finance_ref.invest_bar with g12's e_ref_max; NaN where it is NaN."""
    x, scale = LR.list_metrics(*args, dtype=np.longdouble, parts=True)[3:]
    nan = np.isnan(x.astype(np.float64))
    assert np.array_equal(np.isnan(got), nan), what
    err = np.abs((got.astype(np.longdouble) - x)).astype(np.float64)
    bar = F.invest_bar(_e_ref_max(), scale.astype(np.float64))
    ok = nan | (err <= bar)
    print("%s: max error %.3g, smallest bar %.3g" % (what, np.nanmax(np.where(nan, 0, err)), np.nanmin(np.where(nan, np.inf, bar))))
    assert ok.all(), (what, err[~ok], bar[~ok])


def _launch(args, **kw):
    li, nv, truth, cuts, pidx, plen, upper, rp, dp, rf, df = args
    same = rf is rp
    rp_d = _dev(rp)
    rf_d = rp_d if same else _dev(rf)
    out = P.list_metrics(_i32(li), _i32(truth), cuts, _i32(pidx), _i32(plen), upper, rp_d, _i32(dp), rf_d, _i32(df), _i32(nv), **kw)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def _case(seed, U, L, n_ret, W, cuts, dyadic):
    """Random rows with every edge mixed in: n_valid 0 / below a cutoff / L, -1 holes, truth absent / first / last / < 0 / named
    twice, a held stock recommended again, stocks and days outside one table only.  past [3, 9, n_ret], future [2, 7, n_ret]."""
    rs = np.random.RandomState(seed)
    tab = lambda d, s: (rs.randint(-64, 65, size=(d, s, n_ret)) / 1024.0) if dyadic else rs.randn(d, s, n_ret) * 0.02
    past, future = tab(3, 9), tab(2, 7)
    hi = 7 if dyadic else 10                                     # dyadic cases stay inside both tables (NaN rows are checked apart)
    li = rs.randint(UPPER + 1, UPPER + 1 + hi, size=(U, L))
    li[rs.rand(U, L) < 0.1] = -1
    nv = np.array([0, max(cuts[0] - 1, 0), L, L + 3, -2])[rs.randint(0, 5, size=U)] if U > 1 else np.array([L])
    nv[rs.rand(U) < 0.5] = L
    truth = np.where(li[:, 0] >= 0, li[:, 0], UPPER + 1)
    mode = np.arange(U) % 5
    truth = np.where(mode == 1, li[:, L - 1], truth)
    truth = np.where(mode == 2, UPPER + 40, truth)
    truth = np.where(mode == 3, -1, truth)
    for u in np.flatnonzero(mode == 4):                          # named twice: the first slot counts
        if L >= 3:
            li[u, 1] = li[u, L - 1] = truth[u] = UPPER + 1 + rs.randint(0, hi)
    pidx = rs.randint(0, hi, size=(U, W)) if W else None
    plen = rs.randint(-1, W + 2, size=U) if W else None
    if W:
        pidx[::3, 0] = np.maximum(li[::3, 0], UPPER + 1) - UPPER - 1      # a held stock is recommended again
    dp = rs.randint(0, 3, size=U) if dyadic else rs.randint(-1, 4, size=U)
    df = rs.randint(0, 2, size=U) if dyadic else rs.randint(-1, 3, size=U)
    return (li, nv, truth, cuts, pidx, plen, UPPER, past, dp, future, df)


# U, L, n_ret, W, cutoffs, exact.  Exact cases (compared bitwise): returns are multiples of 2^-10 below 1/16, so every sum of at
# most W + L <= 64 rows is exact in any order; (a) W + L <= 8, (b) the row counts W and W + c are powers of two wherever the row is
# whole (1 | 2, 4, .., 64).  Every later operation then has the same operands in the same order on both sides.
CASES = [
    (1, 1, 2, 0, (1,), True),                                    # (a)
    (3, 5, 29, 1, (1, 3, 5), True),                              # (a)
    (5, 63, 65, 1, (1, 3, 7, 15, 31, 63), True),                 # (b): counts 1 | 2, 4, .., 64 (holes and short lists aside)
    (4, 63, 64, 7, tuple(range(1, 9)), False),
    (5, 64, 65, 7, (64,), False),
    (257, 64, 128, 7, tuple(range(1, 9)), False),                # n_c = 8 at n_ret = 128: the largest LDS image
    (257, 5, 29, 0, (1, 3, 5), False),
]


@pytest.mark.parametrize("U, L, n_ret, W, cuts, exact", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_kernel_against_the_restatement(U, L, n_ret, W, cuts, exact):
    args = _case(U * 1000 + L, U, L, n_ret, W, cuts, exact)
    rank, hits, ndcg, invest = _launch(args)
    r_rank, r_hits, r_ndcg, r_inv = LR.list_metrics(*args)
    print("rank", rank[:8], "ndcg", ndcg[:2])
    assert np.array_equal(rank, r_rank)
    assert np.array_equal(hits, r_hits)
    assert np.array_equal(ndcg, r_ndcg)
    if exact:
        assert _same_bits(invest, r_inv)
    else:
        _within_bar(invest, args, "U=%d L=%d n_ret=%d" % (U, L, n_ret))
    assert (rank == LR.RANK_NONE).any() or U == 1


def test_ndcg_of_every_place():
    """Every rank 0 .. 63 once.  The kernel's NDCG is ``1.f / log2f(rank + 2)`` with the DEVICE library's log2f, the expression of
    ``pfo_eval_metrics``.  Two faithful fp32 logarithms need not agree in the last place, so this test holds the value to the
    correctly rounded ``1 / log2(rank + 2)`` (from extended precision) instead of to another libm: log2f is within 1 ulp (the HIP
    math library's stated accuracy), the logarithm's relative error passes to the quotient at up to twice its size in ulps
    (the quotient may lie at the top of its binade, the logarithm at the bottom of its own), and the IEEE division adds half an
    ulp: 2 + 0.5 < 3 ulp.  Exact where rank + 2 is a power of two.  Measured on an MI355X: at most 2 ulp; rank 3 is 1 ulp off
    (0x3edc81a4 against 0x3edc81a3) and rank 4 is 1 ulp off (0x3ec61193 against 0x3ec61192), in both kernels alike."""
    L = 64
    li = np.tile(np.arange(UPPER + 1, UPPER + 1 + L), (L, 1))
    tab = np.random.RandomState(0).randn(1, L, 4) * 0.02
    args = (li, None, li[np.arange(L), np.arange(L)], (64,), None, None, UPPER, tab, np.zeros(L, int), tab, np.zeros(L, int))
    rank, hits, ndcg, _ = _launch(args)
    want = (np.longdouble(1) / np.log2(np.arange(L).astype(np.longdouble) + 2)).astype(np.float32)
    off = np.abs(ndcg[:, 0].view(np.int32).astype(np.int64) - want.view(np.int32))
    print("ndcg ulps off the correctly rounded value:", off.max(), "at ranks", np.flatnonzero(off).tolist())
    assert rank.tolist() == list(range(L)) and (hits == 1).all()
    assert off.max() < 3
    pow2 = np.array([0, 2, 6, 14, 30, 62])
    assert np.array_equal(ndcg[pow2, 0], np.float32(1) / np.arange(1, 7, dtype=np.float32))


def test_edges_by_hand():
    rs = np.random.RandomState(5)
    past, future = rs.randn(2, 6, 29) * 0.02, rs.randn(3, 4, 29) * 0.02
    A = UPPER + 1
    li = np.array([[A, A + 1, A + 2, A + 3],        # 0 plain, truth last
                   [A, -1, A + 2, A + 3],           # 1 a hole: skipped, the slots keep their places
                   [A, A + 1, A + 2, A + 3],        # 2 n_valid 2: below cutoff 4
                   [A, A + 1, A + 2, A + 3],        # 3 n_valid 0
                   [A, A + 5, A + 2, A + 3],        # 4 stock 5 is outside the future table only
                   [A, A + 1, A + 2, A + 3],        # 5 past day outside
                   [A, A + 1, A + 2, A + 3],        # 6 future day outside
                   [A + 2, A + 1, A + 2, A + 3],    # 7 truth named twice; stock 2 is held and recommended twice
                   [A, A + 1, A + 2, A + 3]])       # 8 truth < 0
    nv = np.array([4, 4, 2, 0, 4, 9, 4, 4, 4])
    truth = np.array([A + 3, A + 2, A + 3, A, A + 5, A, A + 1, A + 2, -1])
    pidx = np.array([[0, 1]] * 7 + [[2, 2]] + [[3, 0]])
    plen = np.array([2, 1, 0, 0, 2, 2, 2, 2, 5])
    dp, df = np.array([0, 1, 0, 1, 1, 2, 0, 1, 0]), np.array([2, 0, 1, 2, 0, 1, -1, 2, 1])
    cuts = (1, 2, 4)
    args = (li, nv, truth, cuts, pidx, plen, UPPER, past, dp, future, df)
    rank, hits, ndcg, inv = _launch(args)
    ref = LR.list_metrics(*args)
    assert rank.tolist() == [3, 2, LR.RANK_NONE, LR.RANK_NONE, 1, 0, 1, 0, LR.RANK_NONE] == ref[0].tolist()
    assert np.array_equal(hits, ref[1]) and np.array_equal(ndcg, ref[2])
    _within_bar(inv, args, "edges")
    fin, nan = np.isfinite, np.isnan
    assert fin(inv[[0, 1, 2, 7, 8]]).all()
    assert np.array_equal(inv[1, [1, 4, 7, 10]], inv[1, [0, 3, 6, 9]])           # the hole adds nothing at cutoff 2
    assert np.array_equal(inv[2, [2, 5, 8, 11]], inv[2, [1, 4, 7, 10]])          # a short list adds what there is
    assert nan(inv[3]).all()                                                     # nothing held, nothing listed: 0 / 0, no guard
    assert fin(inv[4, :6]).all() and fin(inv[4, [6, 9]]).all() and nan(inv[4, [7, 8, 10, 11]]).all()
    assert nan(inv[5, :6]).all() and fin(inv[5, 6:]).all()
    assert fin(inv[6, :6]).all() and nan(inv[6, 6:]).all()
    # one storage passed twice (a price ledger), different day indices per side
    both = (li, nv, truth, cuts, pidx, plen, UPPER, past, dp % 2, past, (dp + 1) % 2)
    got = _launch(both)
    want = LR.list_metrics(*both)
    assert np.array_equal(got[0], want[0])
    _within_bar(got[3], both, "one table twice")
    swapped = _launch((li, nv, truth, cuts, pidx, plen, UPPER, past, (dp + 1) % 2, past, dp % 2))
    assert _same_bits(got[3][:, :6], swapped[3][:, 6:]) and _same_bits(got[3][:, 6:], swapped[3][:, :6])


def test_out_row0_canaries_and_null_outputs():
    args = _case(77, 5, 10, 29, 3, (1, 3, 5, 10), False)
    alone = _launch(args)
    rows, r0, n_c = 12, 4, 4
    out = P.list_buffers(rows, n_c, DEV)
    canary = [-7, -7.5, -7.5, -7.5]
    for o, c in zip(out, canary):
        o.fill_(c)
    got = _launch(args, out=out, out_row0=r0)
    for o, c, a, g in zip(out, canary, alone, got):
        h = o.cpu().numpy()
        assert _same_bits(h[r0:r0 + 5], a) and _same_bits(g, a)
        assert (h[:r0] == c).all() and (h[r0 + 5:] == c).all()
    with pytest.raises(ValueError, match="exceed"):
        P.list_metrics(list_item=_i32(args[0]), truth=_i32(args[2]), cutoffs=args[3], port_idx=_i32(args[4]), port_len=_i32(args[5]),
                       upper_u=UPPER, ret_past=_dev(args[7]), day_past=_i32(args[8]), ret_future=_dev(args[9]), day_future=_i32(args[10]),
                       out=out, out_row0=8)
    # every output pointer NULL in turn: the others are written as before, nothing else is touched
    li, nv, truth, cuts, pidx, plen, upper, rp, dp, rf, df = args
    t = [_i32(li), _i32(nv), _i32(truth), _i32(pidx), _i32(plen), _dev(rp), _i32(dp), _dev(rf), _i32(df)]
    for skip in range(4):
        for o, c in zip(out, canary):
            o.fill_(c)
        ptrs = [None if i == skip else o.data_ptr() for i, o in enumerate(out)]
        _lib.call("pfo_list_metrics", t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 5, 10, (C.c_int32 * 4)(*cuts), 4, t[3].data_ptr(),
                  t[4].data_ptr(), 3, upper, t[5].data_ptr(), t[6].data_ptr(), 3, 9, t[7].data_ptr(), t[8].data_ptr(), 2, 7, 29, r0, rows,
                  *ptrs, _lib.stream_ptr())
        torch.cuda.synchronize()
        for i, (o, c, a) in enumerate(zip(out, canary, alone)):
            h = o.cpu().numpy()
            assert (h == c).all() if i == skip else _same_bits(h[r0:r0 + 5], a), (skip, i)
    # no rows: nothing is launched, nothing is written
    empty = P.list_metrics(_i32(li[:0]), _i32(truth[:0]), cuts, None, None, upper, t[5], _i32(dp[:0]), t[7], _i32(df[:0]))
    assert [tuple(o.shape) for o in empty] == [(0,), (0, 4), (0, 4), (0, 16)]
    # the dispatcher form is the same call
    op = torch.ops.pfotgn.list_metrics(t[0], t[2], list(cuts), upper, t[5], t[6], t[7], t[8], t[3], t[4], t[1])
    assert all(_same_bits(o.cpu().numpy(), a) for o, a in zip(op, alone))


# ---------------------------------------------------------------------------------------------- identity with the evaluation kernels

def _g9a():
    g = load_golden("g9a_invest_metrics")
    s = g["scores"]
    B, N, D = s.shape[0], s.shape[1] - 1, 8
    emb = np.zeros((B * (2 + N), D), np.float32)
    emb[:B, :] = 0.125
    emb[B:2 * B, :] = (s[:, 0] * 8 / D)[:, None]
    emb[2 * B:, :] = (s[:, 1:].reshape(-1) * 8 / D)[:, None]
    mid = {str(c): i for i, c in enumerate(g["codes"])}
    tables = P.InvestTables.from_prices([str(d) for d in g["days"]], g["prices_past"], g["prices_future"], mid)
    pfs = [[str(c) for c in g["port_codes"][r, :g["port_n"][r]]] for r in range(B)]
    pidx, _, plen = E.eval_portfolios(pfs, mid)
    return g, torch.from_numpy(emb).to(DEV), B, N, tables, _i32(pidx), _i32(plen)


@pytest.mark.parametrize("order", ["score", "basket"])
def test_invest_is_the_evaluation_kernels_to_the_bit(order):
    """pfo_eval_metrics (and pfo_eval_metrics_mv in mode 1, whose rank is the basket position) on g9a's inputs; its top5_item fed
    to pfo_list_metrics at (1, 3, 5): invest equal bit for bit, hits / NDCG equal wherever its rank is below 5.  Rows whose
    positive's id occurs twice among the five (g9a draws the destination among its own negatives) are left out of the ranking
    comparison only: a list names items, and its rank is the FIRST slot holding the id."""
    g, emb, B, N, tables, pidx, plen = _g9a()
    rp, rf = tables.device_tables(DEV)
    U = int(g["upper_u"])
    cand, day = _i32(g["cand"]), _i32(g["day_idx"])
    if order == "score":
        rank, hits, ndcg, _, titem, inv = P.eval_metrics(emb, B, N, cand, day, pidx, plen, rp, rf, U)
    else:
        rank, hits, ndcg, _, titem, inv = P.eval_metrics_mv(emb, B, N, cand, day, pidx, plen, rp, rf, U, rp, day, 2.0, 0.5, 1)[:6]
    l_rank, l_hits, l_ndcg, l_inv = P.list_metrics(titem, cand[:, 0].contiguous(), (1, 3, 5), pidx, plen, U, rp, day, rf, day)
    torch.cuda.synchronize()
    assert _same_bits(l_inv.cpu().numpy(), inv.cpu().numpy())
    assert np.isfinite(inv.cpu().numpy()).all()
    r, lr = rank.cpu().numpy(), l_rank.cpu().numpy()
    once = ((titem == cand[:, :1]).sum(1) == 1).cpu().numpy()
    sel = (r < 5) & once
    assert sel.sum() >= 8, sel.sum()
    assert np.array_equal(lr[sel], r[sel])
    assert np.array_equal(l_hits.cpu().numpy()[sel], hits.cpu().numpy()[sel])
    assert np.array_equal(l_ndcg.cpu().numpy()[sel], ndcg.cpu().numpy()[sel])


def test_kernel_on_g12_lists():
    g = load_golden("g12_list_metrics")
    rp, rf = log_returns(g["prices_past"]), log_returns(g["prices_future"])
    args = (g["list_item"], None, g["truth"], tuple(int(c) for c in g["cutoffs"]), g["port_idx"], g["port_len"], int(g["upper_u"]),
            rp, g["day_idx"], rf, g["day_idx"])
    rank, hits, ndcg, inv = _launch(args)
    err = np.abs((inv - g["invest_exact_hi"]) - g["invest_exact_lo"])
    bar = F.invest_bar(float(g["e_ref_max"]), g["invest_scale"])
    print("g12: max error %.3g (the reference's own %.3g)" % (err.max(), float(g["e_ref_max"])))
    assert np.all(err <= bar)
    assert np.array_equal(inv > 0, g["invest"] > 0)
    assert np.array_equal(rank, g["rank"]) and np.array_equal(hits.astype(np.float64), g["recall"])
    assert np.allclose(ndcg, g["ndcg"], rtol=0, atol=1e-6)
    one = np.arange(100) % 10 == 1
    assert np.all(inv[one][:, [0, 6, 12, 18]] == 0)


# ---------------------------------------------------------------------------------------------- backtest on a small served model
N_USERS, N_ITEMS, K_NBR, CUT, LOG, BATCH, WIDTH, N_DAYS = 30, 40, 5, 300, 64, 16, 8, 64
ITEMS = np.arange(N_USERS + 1, N_USERS + N_ITEMS + 1)
DIV = float(1 << 18)          # synthetic.day_of is floor(ts * 64 / 2^24): the key rule with this divisor
CUTS = (1, 3, 5, 10)


class _SynTables(P.InvestTables):
    """InvestTables over the synthetic calendar: the day of a timestamp is the graph's ``day_of`` (not ``str(ts)[:8]``)."""

    def day_indices(self, timestamps):
        return ((np.asarray(timestamps).astype(np.int64) * N_DAYS) >> 24).astype(np.int32)


class _World:
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
        self.ledger = P.PriceLedger.from_prices(np.arange(N_DAYS), g.prices, g.upper_u, DEV, key_divisor=DIV)
        self.days = g.day_of(self.log[2])

    def model(self):
        """A served model: memory, two layers, the first CUT interactions observed and their portfolios in the holdings ledger."""
        torch.manual_seed(6)
        g, d = self.g, self.g.data
        nf = P.NeighborFinder.from_arrays(d.sources[:CUT], d.destinations[:CUT], d.edge_idxs[:CUT], d.timestamps[:CUT], uniform=False,
                                          max_node_idx=g.node_features.shape[0] - 1)
        t = P.TGN(nf, g.node_features, g.edge_features, DEV, n_layers=2, n_heads=2, dropout=0.0, use_memory=True,
                  memory_dimension=16, message_function="identity", n_neighbors=K_NBR)
        t.eval()
        t.observe(d.sources[:CUT], d.destinations[:CUT], d.timestamps[:CUT], d.edge_idxs[:CUT], batch_size=50)
        t.track_holdings(WIDTH, g.upper_u)
        t.update_holdings(d.sources[:CUT], (g.portfolio_idx[:CUT], g.portfolio_len[:CUT]), d.timestamps[:CUT])
        return t


@pytest.fixture(scope="module")
def world():
    return _World()


def _state(t):
    m = t.memory
    return [x.detach().clone() for x in (m.memory, m.last_update, m.msg_table, m.msg_time, m.has_msg)]


def _forms(w):
    return {
        "score": dict(tables=w.tables, portfolios=w.ports),
        "mv": dict(tables=w.tables, mv=w.mv, portfolios=w.ports),
        "basket": dict(tables=w.tables, mv=w.mv, portfolios=w.ports, basket=True),
        "held": dict(tables=w.tables, mv=w.mv, portfolios="held", exclude="held", keep_truth=False),
        "ledger": dict(tables=w.ledger, mv=w.ledger, portfolios=w.ports, horizon=3),
    }


@pytest.mark.parametrize("form", ["score", "mv", "basket", "held", "ledger"])
def test_backtest_is_recommend_score_observe_by_hand(world, form):
    w = world
    kw = _forms(w)[form]
    src, dst, ts, eidx = w.log
    a, b, c = w.model(), w.model(), w.model()
    opt = P.FusedAdam(a)
    frozen = [a.flat_parameters.detach().clone(), None if getattr(a, 'flat_grad', None) is None else a.flat_grad.detach().clone(), opt._t, a._step, a.training]
    rows = P.backtest_rows(a, src, dst, ts, eidx, ITEMS, 10, cutoffs=CUTS, batch_size=BATCH, **kw)
    assert rows["rank"].shape == (LOG,) and rows["invest"].shape == (LOG, 16) and rows["list_item"].shape == (LOG, 10)
    # parameters, gradients, the optimizer's step count and the mode are untouched
    assert torch.equal(a.flat_parameters, frozen[0]) and opt._t == frozen[2] and a._step == frozen[3] and a.training == frozen[4]
    assert (getattr(a, 'flat_grad', None) is None) == (frozen[1] is None) and (frozen[1] is None or torch.equal(a.flat_grad, frozen[1]))
    # the state afterwards is observe(log, batch_size=16)'s, bit for bit
    c.observe(src, dst, ts, eidx, batch_size=BATCH)
    assert all(torch.equal(x, y) for x, y in zip(_state(a), _state(c)))
    # batch j: recommend on a twin that observed batches 0 .. j-1, list_metrics by hand on those lists
    ledger = isinstance(kw["tables"], P.PriceLedger)
    if ledger:
        rp = rf = kw["tables"].returns
        dp, df = BT.ledger_days(kw["tables"], ts, kw["horizon"], DEV)
    else:
        rp, rf = kw["tables"].device_tables(DEV)
        dp = df = _i32(w.days)
    moved = 0
    for lo in range(0, LOG, BATCH):
        hi = lo + BATCH
        held = kw.get("portfolios") == "held"
        side = {}
        if "mv" in kw:
            side = dict(mv=kw["mv"], portfolios="held" if held else (w.ports[0][lo:hi], w.ports[1][lo:hi]), basket=kw.get("basket", False))
        res = b.recommend(src[lo:hi], ts[lo:hi], 10, ITEMS, exclude=kw.get("exclude"), **side)
        assert np.array_equal(res[0].cpu().numpy(), rows["list_item"][lo:hi]), (form, lo)
        assert np.array_equal(res[2].cpu().numpy(), rows["n_valid"][lo:hi])
        pidx, plen = b.holdings.rows(src[lo:hi]) if held else (_i32(w.ports[0][lo:hi]), _i32(w.ports[1][lo:hi]))
        hand = P.list_metrics(res[0], _i32(dst[lo:hi]), CUTS, pidx, plen, w.g.upper_u, rp, dp[lo:hi], rf, df[lo:hi], res[2])
        for name, h in zip(("rank", "recall", "ndcg", "invest"), hand):
            assert _same_bits(h.cpu().numpy(), rows[name][lo:hi]), (form, name, lo)
        if lo:
            first = w.model() if lo == BATCH else None
            if first is not None:                                # the state matters: a model that saw nothing of the log answers differently
                stale = first.recommend(src[lo:hi], ts[lo:hi], 10, ITEMS, exclude=kw.get("exclude"), **side)
                moved += int(not torch.equal(stale[0], res[0]))
        b.observe(src[lo:hi], dst[lo:hi], ts[lo:hi], eidx[lo:hi], batch_size=None)
    assert moved == 1, "observing batch 0 must move batch 1's lists, or the walk shows nothing"
    # against the numpy restatement, and the dict
    args = (rows["list_item"], rows["n_valid"], dst, CUTS, *(x.cpu().numpy() for x in (a.holdings.rows(src) if held else map(_i32, w.ports))),
            w.g.upper_u, rp.cpu().numpy(), dp.cpu().numpy(), rf.cpu().numpy(), df.cpu().numpy())
    assert np.array_equal(rows["rank"], LR.list_metrics(*args)[0])
    _within_bar(rows["invest"], args, form)
    out = P.backtest_result_dict("bt", rows["rank"], rows["invest"], CUTS)
    assert out["n"] == LOG and out["n_past"] == LOG and out["n_future"] == LOG
    assert out["bt_recall_avg_10"] == np.mean((rows["rank"] < 10).astype(np.float64))
    assert (rows["n_valid"] == 10).all()
    if form == "basket":
        # ten picks of the basket scored at 1, 3, 5, 10: what eval_recommendation's censored rank cannot state
        plain = P.backtest_rows(w.model(), src, dst, ts, eidx, ITEMS, 10, cutoffs=CUTS, batch_size=BATCH, **_forms(w)["mv"])
        assert not np.array_equal(plain["list_item"], rows["list_item"]) and np.array_equal(plain["list_item"][:, 0], rows["list_item"][:, 0])
        assert ((rows["rank"] >= 5) & (rows["rank"] < 10)).any(), "a truth picked in rounds 6 .. 10"
        assert not np.array_equal(rows["invest"][:, 3], rows["invest"][:, 2])


def test_backtest_dict_and_a_ledger_that_ends_too_early(world):
    w = world
    src, dst, ts, eidx = w.log
    horizon = int(N_DAYS - 1 - np.sort(w.days)[LOG // 2])        # about half the rows reach the ledger's last day
    assert horizon >= 1
    kw = dict(cutoffs=CUTS, batch_size=BATCH, tables=w.ledger, mv=w.ledger, portfolios=w.ports, horizon=horizon)
    rows = P.backtest_rows(w.model(), src, dst, ts, eidx, ITEMS, 10, **kw)
    out = P.backtest(w.model(), src, dst, ts, eidx, ITEMS, 10, name="led", **kw)
    reach = w.days + horizon <= N_DAYS - 1
    assert 0 < reach.sum() < LOG
    assert out["n"] == LOG and out["n_past"] == LOG and out["n_future"] == int(reach.sum())
    assert np.isfinite(rows["invest"][:, :8]).all()
    assert np.isnan(rows["invest"][~reach, 8:]).all() and np.isfinite(rows["invest"][reach, 8:]).all()
    for i, c in enumerate(CUTS):
        assert out["led_return_avg_%d_" % c] == np.mean(np.ascontiguousarray(rows["invest"][reach, 8 + i]))
        assert out["led_sharpe_percent_%d_" % c] == (rows["invest"][reach, 12 + i] > 0).sum() / reach.sum()
        assert out["led_return_avg_%d" % c] == np.mean(np.ascontiguousarray(rows["invest"][:, i]))
    # device inputs take the device lookup and give the same rows
    on_dev = (_i32(src), _i32(dst), _dev(ts, np.float64), _i32(eidx))
    again = P.backtest_rows(w.model(), *on_dev, ITEMS, 10, **kw)
    assert all(_same_bits(again[k], rows[k]) for k in rows)


def test_keep_truth(world):
    """A user whose truth is held gets it offered with keep_truth=True and never with False."""
    w = world
    src, dst, ts, eidx = (x[:BATCH] for x in w.log)
    first = np.array([i for i in range(BATCH) if src[i] not in src[:i]])
    got = {}
    for keep in (True, False):
        t = w.model()
        rows_ = np.full((len(first), 2), -1, np.int32)
        rows_[:, 0] = dst[first] - w.g.upper_u - 1               # the stock about to be bought is already held
        rows_[:, 1] = (rows_[:, 0] + 1) % N_ITEMS
        t.update_holdings(src[first], (rows_, np.full(len(first), 2, np.int32)), ts[first] - 1.0)
        got[keep] = P.backtest_rows(t, src, dst, ts, eidx, ITEMS, N_ITEMS, cutoffs=(1, N_ITEMS), batch_size=BATCH, tables=w.tables,
                                    exclude="held", keep_truth=keep)
    yes, no = got[True], got[False]
    assert (yes["rank"][first] < N_ITEMS).all() and (yes["n_valid"][first] == N_ITEMS - 1).all()
    assert (no["rank"][first] == LR.RANK_NONE).all() and (no["n_valid"][first] == N_ITEMS - 2).all()
    for i in first:
        assert dst[i] in yes["list_item"][i] and dst[i] not in no["list_item"][i]
        assert (dst[i] + 1 - ITEMS[0]) % N_ITEMS + ITEMS[0] not in yes["list_item"][i]          # the other holding stays excluded
    # packed rows, on the host and on the device, are treated alike
    ids = np.full((BATCH, 2), -1, np.int32)
    ids[:, 0], ids[:, 1] = dst, ITEMS[0] + (dst + 1 - ITEMS[0]) % N_ITEMS
    lens = np.full(BATCH, 2, np.int32)
    for pair in ((ids, lens), (_i32(ids), _i32(lens))):
        r = P.backtest_rows(w.model(), src, dst, ts, eidx, ITEMS, N_ITEMS, cutoffs=(1,), batch_size=BATCH, tables=w.tables, exclude=pair,
                            upper_u=w.g.upper_u)
        assert (r["rank"] < N_ITEMS).all() and (r["n_valid"] == N_ITEMS - 1).all()
        r = P.backtest_rows(w.model(), src, dst, ts, eidx, ITEMS, N_ITEMS, cutoffs=(1,), batch_size=BATCH, tables=w.tables, exclude=pair,
                            keep_truth=False)
        assert (r["rank"] == LR.RANK_NONE).all() and (r["n_valid"] == N_ITEMS - 2).all()
