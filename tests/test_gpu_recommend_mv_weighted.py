"""GPU tests of the position-weighted mean-variance order: ``pfo_recommend_mv_topk_weighted``, its wide and its list sibling
against the numpy reference of ``recommend_mv_weighted_ref`` (bit for bit on exact arithmetic), against their unweighted
siblings (all-ones weights, a null weight row), ``pfo_holdings_gather_weights`` against its host model, and
``TGN.recommend(portfolio_weights=...)`` / ``backtest`` end to end on a small served world with a quantity ledger and a price
ledger."""
import functools

import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

import pfotgnrec_amd as P
from pfotgnrec_amd import _lib
from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
import recommend_ref as R
import recommend_mv_ref as M
import recommend_list_ref as L
import recommend_mv_weighted_ref as WR

DEV = "cuda:0"
NAMES = ("top_pos", "top_score", "top_fused", "n_valid", "score", "y", "fused")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _call(form, c, lam, k, n_t, port_w="case"):
    """The functional entry of ``form`` ("bounded", "wide", "list") on a case dict; ``port_w``: the case's rows, other rows, or
    None - the unweighted entry."""
    w = c["port_w"] if isinstance(port_w, str) else port_w
    mv = (_dev(c["cand_stock"]), _dev(c["returns"]), _dev(c["day_idx"]), _dev(c["port_idx"]), _dev(c["port_len"]), c["gamma"], lam)
    if form == "list":
        out = P.recommend_list_mv_topk(_dev(c["user_emb"]), _dev(c["item_emb"]), k, _dev(c["list_pos"]), _dev(c["list_len"]), *mv,
                                       _dev(c["user_block"]), _dev(c.get("item_ok")), n_blocks=n_t, want_all=True, port_w=_dev(w))
    else:
        fn = P.recommend_mv_topk if form == "bounded" else P.recommend_mv_topk_wide
        out = fn(_dev(c["user_emb"]), _dev(c["item_emb"]), k, *mv, _dev(c["user_block"]), _dev(c.get("excl_pos")), _dev(c.get("excl_len")),
                 _dev(c.get("item_ok")), n_blocks=n_t, want_all=True, port_w=_dev(w))
    return {n: t.cpu().numpy() for n, t in zip(NAMES, out)}


def _bits(a):
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _assert_same_outputs(a, b, tag):
    for n in NAMES:
        assert a[n].shape == b[n].shape and np.array_equal(_bits(a[n]), _bits(b[n])), (n, tag)


def _same_f64(a, b):
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def _assert_equals_reference(got, ref, tag):
    assert np.array_equal(got["n_valid"], ref["n_valid"]), tag
    assert np.array_equal(got["top_pos"], ref["top_pos"]), tag
    assert np.array_equal(got["top_score"].view(np.int32), ref["top_score"].view(np.int32)), tag
    assert np.array_equal(got["top_fused"], ref["top_fused"]), tag
    assert _same_f64(got["y"], ref["y"]), tag
    assert _same_f64(got["fused"], ref["fused"]), tag


# ---------------------------------------------------------------------------------------------- the kernels alone
U, W, N_RET = 37, 8, 29           # two full tiles of 16 users and a partial one
SHAPES = [(D, k, n_t) for D in (32, 176) for k in (1, 10) for n_t in (1, 3)]     # the smallest and the 11-fragment instantiation


@functools.lru_cache(maxsize=None)
def _side(I):
    """The weighted mean-variance side of the exact cases with I candidates and its y - computed once and shared; nobody writes to them."""
    side = WR.weighted_side(4000 + I, U, I, N_RET, W)
    return side, WR.y_of(side)


def _exact(I, D, k, n_t):
    c = R.exact_case(100 * I + D + 7 * k + n_t, U, I, D, k, n_t)
    s64 = R.scores64(c["user_emb"], c["item_emb"], c["user_block"], I)
    assert np.array_equal(s64.astype(np.float32).astype(np.float64), s64) and np.abs(s64).max() < 2 ** 24
    side, y = _side(I)
    c.update(side)
    return c, y, s64


@pytest.mark.parametrize("I", [1, 5, 40, 513])
def test_exact_arithmetic_bit_exact_everything(I):
    """Small-integer embeddings (every fp32 score exact: asserted) and exact return tables: positions, scores, top_fused,
    n_valid and the whole y and fused rows are the reference's to the last bit, for every user - random positive weights, exact
    1.0 rows, user 2 with one holding, user 3 with a zero, a negative, a NaN and a +inf weight among the valid ones, user 4 with
    only uncounted weights (main.py:254).  The weights matter: the unweighted y differs."""
    side, y = _side(I)
    plain_y = M.y_matrix(side["returns"], side["day_idx"], side["cand_stock"], side["port_idx"], side["port_len"], side["gamma"])
    assert I < 5 or not _same_f64(y, plain_y), "the case must tell the weighted y from the unweighted"
    for D, k, n_t in SHAPES:
        c, y, s64 = _exact(I, D, k, n_t)
        lam = 0.5 if k == 10 else 1.0
        ref = WR.reference(c, lam, k, y=y)
        got = _call("bounded", c, lam, k, n_t)
        assert np.array_equal(got["score"].astype(np.float64), s64), (I, D, k, n_t)
        _assert_equals_reference(got, ref, (I, D, k, n_t))
        assert got["top_pos"].shape == (U, k)                          # no user is left out: every row was compared


@pytest.mark.parametrize("form", ["bounded", "wide", "list"])
@pytest.mark.parametrize("I", [1, 5, 40, 513])
def test_all_ones_weights_equal_the_unweighted_entry(form, I):
    ones = np.ones((U, W))
    for D, k, n_t in SHAPES:
        c, _, _ = _exact(I, D, k, n_t)
        if form == "list":
            c = L.list_case(c, I + D, 16)
        a = _call(form, c, 0.5, k, n_t, port_w=ones)
        b = _call(form, c, 0.5, k, n_t, port_w=None)
        _assert_same_outputs(a, b, (form, I, D, k, n_t))
        if I >= 40 and k == 10:
            assert (b["n_valid"] > 0).sum() > U // 2


def _raw_args(form, c, k, n_t, lam, port_w, out, ws=None):
    """The argument list of the C entry of ``form`` (its weighted sibling when ``port_w`` is not the string "plain")."""
    I = len(c["cand_stock"])
    t = {n: _dev(c.get(n)) for n in ("user_emb", "item_emb", "user_block", "excl_pos", "excl_len", "item_ok", "cand_stock", "returns", "day_idx",
                                     "port_idx", "port_len", "list_pos", "list_len")}
    p = lambda x: None if x is None else x.data_ptr()
    rows = ("list_pos", "list_len") if form == "list" else ("excl_pos", "excl_len")
    stride = 0 if t[rows[0]] is None else int(t[rows[0]].shape[1])
    nd, ns, nr = c["returns"].shape
    args = [p(t["user_emb"]), p(t["item_emb"]), p(t["user_block"]), c["user_emb"].shape[0], I, n_t, c["user_emb"].shape[1], p(t[rows[0]]),
            p(t[rows[1]]), stride, p(t["item_ok"]), p(t["cand_stock"]), p(t["returns"]), nd, ns, nr, p(t["day_idx"]), p(t["port_idx"]),
            p(t["port_len"])]
    keep = [t]
    if not isinstance(port_w, str):
        wd = _dev(port_w)
        keep.append(wd)
        args.append(p(wd))
    args += [c.get("port_stride", 0 if c["port_idx"] is None else c["port_idx"].shape[1]), c["gamma"], lam, k] + [p(o) for o in out]
    if form == "wide":
        args += [p(ws), ws.numel()]
    return args + [_lib.stream_ptr()], keep


def _raw(form, c, k, n_t, lam, port_w):
    symbol = {"bounded": "pfo_recommend_mv_topk", "wide": "pfo_recommend_mv_topk_wide", "list": "pfo_recommend_list_mv_topk"}[form]
    Uc, I = c["user_emb"].shape[0], len(c["cand_stock"])
    cols = c["list_pos"].shape[1] if form == "list" else I
    out = [torch.empty((Uc, k), dtype=torch.int32, device=DEV), torch.empty((Uc, k), dtype=torch.float32, device=DEV),
           torch.empty((Uc, k), dtype=torch.float64, device=DEV), torch.empty(Uc, dtype=torch.int32, device=DEV),
           torch.empty((Uc, cols), dtype=torch.float32, device=DEV), torch.empty((Uc, cols), dtype=torch.float64, device=DEV),
           torch.empty((Uc, cols), dtype=torch.float64, device=DEV)]
    ws = None
    if form == "wide":
        ws = torch.empty(_lib.byte_count("pfo_recommend_mv_wide_workspace_bytes", Uc, I), dtype=torch.uint8, device=DEV)
    args, keep = _raw_args(form, c, k, n_t, lam, port_w, out, ws)
    _lib.call(symbol + ("" if isinstance(port_w, str) else "_weighted"), *args)
    torch.cuda.synchronize()
    return {n: o.cpu().numpy() for n, o in zip(NAMES, out)}


@pytest.mark.parametrize("form", ["bounded", "wide", "list"])
def test_a_null_weight_row_is_the_sibling(form):
    c, _, _ = _exact(40, 32, 10, 3)
    if form == "list":
        c = L.list_case(c, 3, 16)
    sibling = _raw(form, c, 10, 3, 0.5, "plain")
    _assert_same_outputs(_raw(form, c, 10, 3, 0.5, None), sibling, form)
    _assert_same_outputs(_call(form, c, 0.5, 10, 3, port_w=None), sibling, form)
    weighted = _raw(form, c, 10, 3, 0.5, c["port_w"])
    _assert_same_outputs(weighted, _call(form, c, 0.5, 10, 3), form)
    assert not _same_f64(weighted["y"], sibling["y"])
    # weights without holdings to weigh on: refused where port_idx without port_len is
    with pytest.raises(_lib.PfoError, match="port_w without port_idx"):
        _raw(form, dict(c, port_idx=None, port_len=None, port_stride=W), 10, 3, 0.5, c["port_w"])
    if form == "bounded":
        op = torch.ops.pfotgn.recommend_mv_topk(_dev(c["user_emb"]), _dev(c["item_emb"]), 10, _dev(c["cand_stock"]), _dev(c["returns"]),
                                                _dev(c["day_idx"]), c["gamma"], 0.5, 3, _dev(c["port_idx"]), _dev(c["port_len"]),
                                                _dev(c["user_block"]), _dev(c["excl_pos"]), _dev(c["excl_len"]), _dev(c["item_ok"]),
                                                _dev(c["port_w"]))
        for t, n in zip(op, NAMES):
            assert np.array_equal(_bits(t.cpu().numpy()), _bits(weighted[n])), n


def test_the_wide_form_is_the_bounded_form_and_the_reference():
    # I = 300: both forms apply
    rs_side = WR.weighted_side(77, 17, 300, N_RET, W)
    for D, k, n_t in ((32, 10, 3), (176, 1, 1)):
        c = R.exact_case(300 + D, 17, 300, D, k, n_t)
        c.update(rs_side)
        _assert_same_outputs(_call("wide", c, 0.5, k, n_t), _call("bounded", c, 0.5, k, n_t), (D, k, n_t))
    # I = 2100: beyond the bounded form, against the reference
    c = R.exact_case(2100, 17, 2100, 32, 10, 2)
    c.update(WR.weighted_side(78, 17, 2100, N_RET, W))
    ref = WR.reference(c, 0.5, 10)
    got = _call("wide", c, 0.5, 10, 2)
    assert np.array_equal(got["score"].astype(np.float64), ref["s64"])
    _assert_equals_reference(got, ref, 2100)
    assert not _same_f64(ref["y_raw"], M.y_matrix(c["returns"], c["day_idx"], c["cand_stock"], c["port_idx"], c["port_len"], c["gamma"]))


def test_the_list_form_against_the_reference():
    """Lists of length 0, 1, 64 and 65 (one lane's slots, and one more) among random ones, over I = 2500 candidates."""
    Ul, I, D, k, n_t, LW = 17, 2500, 32, 10, 2, 65
    base = R.exact_case(2500, Ul, I, D, k, n_t)
    base.update(WR.weighted_side(79, Ul, I, N_RET, W))
    c = L.list_case(base, 5, LW)
    rs = np.random.RandomState(9)
    for u, n in enumerate((0, 1, 64, 65)):
        c["list_pos"][u] = -1
        c["list_pos"][u, :n] = rs.choice(I, size=n, replace=False)
        c["list_len"][u] = n
    ref = WR.reference_list(c, 0.5, k)
    got = _call("list", c, 0.5, k, n_t)
    for n in ("top_pos", "n_valid", "top_fused"):
        assert np.array_equal(got[n], ref[n]), n
    assert np.array_equal(got["top_score"].view(np.int32), ref["top_score"].view(np.int32))
    assert _same_f64(got["y"], ref["y_slot"]) and _same_f64(got["fused"], ref["fused_slot"])
    assert ref["n_valid"][0] == 0 and ref["n_valid"][1] <= 1 and (ref["n_valid"][2:4] == k).all()
    plain = L.reference_mv(c, 0.5, k)
    assert not _same_f64(plain["y_slot"], ref["y_slot"])


@pytest.mark.parametrize("lam", [0.5, 0.1])
@pytest.mark.parametrize("seed,Ub,I,D,k", M.BLEND_CASES)
def test_blend_on_random_normal_embeddings_in_two_stages(seed, Ub, I, D, k, lam):
    """The two-stage comparison of the unweighted kernel's test with its bars unchanged: (a) every score within the fp32
    dot-product bound of the fp64 score; (b) the reference's ``fuse`` over the kernel's OWN scores reproduces everything exactly;
    the users whose fp64 scores are separated by more than the bounds - at least one in two, a condition on scores alone that
    the weights do not touch (tests/test_recommend_mv_cpu.py establishes it for these seeds) - get the fp64 reference's lists."""
    c = R.normal_case(seed, Ub, I, D)
    c.update(WR.weighted_side(seed, Ub, I, 29))
    ref = WR.reference(c, lam, k)
    got = _call("bounded", c, lam, k, 1)
    eps = R.dot_error_bound(c["user_emb"], c["item_emb"], None, I)
    err = np.abs(got["score"].astype(np.float64) - ref["s64"])
    print("FIGURES recommend_mv_topk_weighted (%d,%d,%d,%d) lambda %.1f: largest |score error| / eps %.3f" % (Ub, I, D, k, lam, (err / eps).max()))
    assert (err <= eps).all()                                                                        # (a)
    own = WR.reference(c, lam, k, scores=got["score"], y=ref["y_raw"])
    _assert_equals_reference(got, own, (seed, lam))                                                  # (b)
    base = R.admissible(Ub, I, c["excl_pos"], c["excl_len"], c["item_ok"])
    sep = np.array([M.separated_share(ref["s64"][u:u + 1], eps[u:u + 1], base[u:u + 1]) == 1.0 for u in range(Ub)])
    print("FIGURES separated share %.3f" % sep.mean())
    assert sep.mean() >= 0.5
    assert np.array_equal(got["top_pos"][sep], ref["top_pos"][sep]) and np.array_equal(got["top_fused"][sep], ref["top_fused"][sep])


@pytest.mark.parametrize("Wl", [1, 64, 256])
def test_gather_weights_against_the_host_model(Wl):
    n_nodes, n_stocks = 50, 40
    g = WR.gather_case(10 + Wl, n_nodes, Wl, 33, n_stocks)
    idx, ln, qty, close, users = (_dev(g[n]) for n in ("hold_idx", "hold_len", "hold_qty", "last_close", "users"))
    for mode, name in ((WR.SHARES, "shares"), (WR.VALUE, "value")):
        want = WR.gather_weights(g["users"], g["hold_idx"], g["hold_len"], g["hold_qty"], mode, g["last_close"])
        got = P.holdings_gather_weights(users, idx, ln, qty, name, close if mode else None).cpu().numpy()
        assert got.shape == (33, Wl) and np.array_equal(got.view(np.int64), want.view(np.int64)), (Wl, name)
        op = torch.ops.pfotgn.holdings_gather_weights(users, idx, ln, qty, mode, close if mode else None)
        assert np.array_equal(op.cpu().numpy().view(np.int64), want.view(np.int64))
    assert P.holdings_gather_weights(users[:0], idx, ln, qty, 0).shape == (0, Wl)
    for bad, msg in (((users.data_ptr(), 33, idx.data_ptr(), ln.data_ptr(), None, n_nodes, Wl, None, 0, 0), "null hold_qty"),
                     ((users.data_ptr(), 33, idx.data_ptr(), ln.data_ptr(), qty.data_ptr(), n_nodes, Wl, None, n_stocks, 1), "null last_close"),
                     ((None, 33, None, None, None, n_nodes, 257, None, 0, 0), "W must lie"),
                     ((None, 33, None, None, None, n_nodes, Wl, None, 0, 2), "mode must be"),
                     ((None, -1, None, None, None, n_nodes, Wl, None, 0, 0), "U must not"),
                     ((None, 33, None, None, None, 0, Wl, None, 0, 0), "n_nodes must"),
                     ((None, 33, None, None, None, n_nodes, Wl, None, -1, 0), "n_stocks must")):
        with pytest.raises(_lib.PfoError, match=msg):
            _lib.call("pfo_holdings_gather_weights", *bad, users.data_ptr(), _lib.stream_ptr())


# ---------------------------------------------------------------------------------------------- TGN.recommend / backtest
# (a served world in the manner of tests/test_gpu_recommend_list.py: 150 nodes, D = 16, L = 1, K = 5 - here with a quantity
# ledger of width 8 fed by trades and a price ledger)
N_USERS, N_ITEMS, K_NBR, CUT, WIDTH, N_DAYS = 120, 30, 5, 900, 8, 64
ITEMS = np.arange(N_USERS + 1, N_USERS + N_ITEMS + 1)
DIV = float(1 << 18)          # synthetic.day_of is floor(ts * 64 / 2^24): the price ledger's key rule with this divisor


def _graph():
    torch.manual_seed(6)
    return make_graph(SyntheticConfig("t", N_USERS, N_ITEMS, 1500, 16, 1, K_NBR, 2), with_prices=True)


def _model(g):
    torch.manual_seed(6)
    d = g.data
    nf = P.NeighborFinder.from_arrays(d.sources[:CUT], d.destinations[:CUT], d.edge_idxs[:CUT], d.timestamps[:CUT], uniform=False,
                                      max_node_idx=g.node_features.shape[0] - 1)
    tgn = P.TGN(nf, g.node_features, g.edge_features, DEV, n_layers=1, n_heads=2, dropout=0.0, use_memory=True, memory_dimension=16,
                message_function="identity", n_neighbors=K_NBR)
    tgn.eval()
    tgn.track_holdings(WIDTH, g.upper_u, quantities=True)
    rs = np.random.RandomState(3)
    side = np.ones(CUT, np.int32)
    side[rs.rand(CUT) < 0.2] = -1
    qty = rs.choice([0.5, 1.0, 2.0, 7.25, 40.0], CUT)
    assert tgn.trade_holdings(d.sources[:CUT], d.destinations[:CUT] - g.upper_u - 1, side, d.timestamps[:CUT], quantities=qty) == CUT
    return tgn


@pytest.fixture(scope="module")
def world():
    g = _graph()
    tgn = _model(g)
    d = g.data
    users = np.unique(d.sources[:CUT])[:21]
    users = np.concatenate([users, users[:2]])
    ts = d.timestamps[CUT:CUT + 600:200][np.arange(len(users)) % 3]                  # three distinct times, not sorted
    led = P.PriceLedger.from_prices(np.arange(N_DAYS), g.prices, g.upper_u, DEV, key_divisor=DIV)
    return g, tgn, users, ts, led


def _state(t):
    m, h = t.memory, t.holdings
    tens = [t.flat_parameters, m.memory, m.last_update, m.msg_table, m.msg_time, m.has_msg, h.idx, h.len, h.time, h.qty]
    return [x.detach().clone() for x in tens], (t.training, t._step, t._gru_applied_now, m._any_msg, m._state_version, t.n_nodes)


def _unchanged(t, before):
    now = _state(t)
    return now[1] == before[1] and all(torch.equal(a, b) for a, b in zip(now[0], before[0]))


def _host_rows(tgn, led, users):
    """(idx, len, shares rows, value rows) computed on the host from the ledger's tables and the price ledger's last close."""
    idx, ln = (t.cpu().numpy() for t in tgn.holdings.rows(users))
    qty = tgn.holdings.qty.cpu().numpy()[users]
    close = led.last_close.cpu().numpy()
    live = np.arange(WIDTH)[None, :] < ln[:, None]
    shares = np.where(live, qty, 0.0)
    inside = (idx >= 0) & (idx < len(close))
    value = np.where(live & inside, qty * close[np.where(inside, idx, 0)], 0.0)
    return idx, ln, shares, value


def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("only", [None, "held"])
def test_recommend_named_weights_are_the_host_rows(world, only):
    g, tgn, users, ts, led = world
    idx, ln, shares, value = _host_rows(tgn, led, users)
    assert (ln >= 2).sum() > 5 and (shares[ln >= 2] != 1.0).any() and not np.array_equal(shares, value)
    kw = dict(mv=led, only=only)
    before = _state(tgn)
    for name, rows in (("shares", shares), ("value", value)):
        named = tgn.recommend(users, ts, 5, ITEMS, portfolios="held", portfolio_weights=name, **kw)
        for form in (rows, _dev(rows), [rows[u, :ln[u]].tolist() for u in range(len(users))]):
            explicit = tgn.recommend(users, ts, 5, ITEMS, portfolios=(idx, ln), portfolio_weights=form, **kw)
            assert len(named) == 4 and _equal(named, explicit), name
    none = tgn.recommend(users, ts, 5, ITEMS, portfolios="held", **kw)
    ones = tgn.recommend(users, ts, 5, ITEMS, portfolios=(idx, ln), portfolio_weights=np.ones((len(users), WIDTH)), **kw)
    assert _equal(none, ones)
    on_dev = tgn.recommend(users, _dev(ts), 5, ITEMS, portfolios="held", portfolio_weights="value", **kw)
    assert _equal(on_dev, tgn.recommend(users, ts, 5, ITEMS, portfolios="held", portfolio_weights="value", **kw))
    assert _unchanged(tgn, before)
    for t in (True, False):
        tgn.train(t)
        before = _state(tgn)
        tgn.recommend(users, ts, 5, ITEMS, portfolios="held", portfolio_weights="shares", **kw)
        assert _unchanged(tgn, before)
    tgn.eval()


def test_recommend_weights_reach_the_kernel(world):
    """The served lists are the weighted kernel's on the query's own embeddings: the rows follow the users through the block
    sort, and the weights change y."""
    g, tgn, users, ts, led = world
    idx, ln, shares, _ = _host_rows(tgn, led, users)
    out = tgn.recommend(users, ts, 5, ITEMS, mv=led, portfolios="held", portfolio_weights="shares", return_embeddings=True)
    ue, ie, ub = out[-3:]
    assert len(set(ub.cpu().numpy().tolist())) == 3 and (np.diff(ub.cpu().numpy()) < 0).any(), "blocks not sorted"
    day = led.lookup(_dev(ts))
    cand = _dev((ITEMS - g.upper_u - 1).astype(np.int32))
    args = (ue, ie, 5, cand, led.returns, day, _dev(idx), _dev(ln), float(led.gamma), float(led.lambda_mv), ub)
    direct = P.recommend_mv_topk(*args, n_blocks=3, want_all=True, port_w=_dev(shares))
    pos = np.where(out[0].cpu().numpy() >= 0, out[0].cpu().numpy() - N_USERS - 1, -1)
    assert np.array_equal(pos, direct[0].cpu().numpy()) and torch.equal(out[1], direct[1]) and torch.equal(out[3], direct[2])
    plain = P.recommend_mv_topk(*args, n_blocks=3, want_all=True)
    assert not _same_f64(direct[5].cpu().numpy(), plain[5].cpu().numpy())


def test_backtest_with_weights_is_the_loop_of_recommend_calls():
    g = _graph()
    d = g.data
    a, b = _model(g), _model(g)
    led = P.PriceLedger.from_prices(np.arange(N_DAYS), g.prices, g.upper_u, DEV, key_divisor=DIV)
    LOG, BATCH = 48, 16
    sl = slice(CUT, CUT + LOG)
    src, dst, ts, eidx = d.sources[sl], d.destinations[sl], d.timestamps[sl], d.edge_idxs[sl]
    rows = P.backtest_rows(a, src, dst, ts, eidx, ITEMS, 5, cutoffs=(1, 5), batch_size=BATCH, tables=led, mv=led, portfolios="held",
                           portfolio_weights="shares")
    plain = 0
    for lo in range(0, LOG, BATCH):
        hi = lo + BATCH
        res = b.recommend(src[lo:hi], ts[lo:hi], 5, ITEMS, mv=led, portfolios="held", portfolio_weights="shares")
        assert np.array_equal(res[0].cpu().numpy(), rows["list_item"][lo:hi]) and np.array_equal(res[2].cpu().numpy(), rows["n_valid"][lo:hi])
        plain += int(not torch.equal(res[3], b.recommend(src[lo:hi], ts[lo:hi], 5, ITEMS, mv=led, portfolios="held")[3]))
        b.observe(src[lo:hi], dst[lo:hi], ts[lo:hi], eidx[lo:hi], batch_size=None)
    assert plain >= 1, "the weights must change a fused value somewhere, or the test shows nothing"
    assert all(torch.equal(x, y) for x, y in zip(_state(a)[0], _state(b)[0]))
