"""CPU side of holdings from trades: the numpy loop of ``holdings_trades_ref`` against a dict-of-lists model,
the two consequences of the rules (composition, snapshot equivalence), the reload round trip, the new symbols and their argument
checks, every host-side refusal of ``trade_holdings`` / ``ingest(portfolios="buys")`` / ``track_holdings(quantities=)`` /
``backtest(advance_holdings=)`` - a rejected call leaves the ledger and the model bit for bit - the op's fake and the new
keywords' defaults.  No kernel runs here."""
import inspect
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import holdings_ref as HR
import holdings_trades_ref as TR
from conftest import REPO

SYMBOLS = ("pfo_holdings_apply", "pfo_holdings_apply_scratch_bytes")
W, UPPER_U = 4, 50                                             # the host model below: 50 users, 10 items


def _tables(n_nodes, width, quantities):
    return HR.new_tables(n_nodes, width) + ((TR.new_qty(n_nodes, width),) if quantities else (None,))


def _run(tabs, ev, counters=None):
    return TR.apply(tabs[0], tabs[1], tabs[2], ev[0], ev[1], ev[2], ev[3], qty=tabs[3], qty_in=ev[4], counters=counters)


def _same(a, b):
    return all((x is None and y is None) or HR.same_bits(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------- 1. the reference's own rules
def _brute(n_nodes, width, ev, quantities):
    """Per user a list of [stock, shares], oldest first - no tables, no slots."""
    book = {u: [] for u in range(n_nodes)}
    when, over, unm = {}, 0, 0
    for e in range(len(ev[0])):
        u, s, sd = int(ev[0][e]), int(ev[1][e]), int(ev[2][e])
        q = float(ev[4][e]) if quantities and ev[4] is not None else 1.0
        if not 1 <= u < n_nodes or s < 0 or sd not in (1, -1) or not (math.isfinite(q) and q > 0):
            continue
        pos = [p for p in book[u] if p[0] == s]
        if sd == 1:
            if pos:
                pos[0][1] += q
            elif len(book[u]) < width:
                book[u].append([s, q])
            else:
                over += 1
        elif not pos:
            unm += 1
        elif quantities and pos[0][1] - q > 0:
            pos[0][1] -= q
        else:
            book[u].remove(pos[0])
        when[u] = ev[3][e]
    return book, when, over, unm


@pytest.mark.parametrize("quantities", [False, True])
@pytest.mark.parametrize("seed", range(6))
def test_reference_is_the_dict_of_lists_model(seed, quantities):
    n_nodes, width, N = 9, 1 + seed % 4, 400
    ev = TR.make_case(100 + seed, n_nodes, width, N, None, quantities)
    tabs = _tables(n_nodes, width, quantities)
    ctr = np.array([5, 7], np.int64)
    counts = _run(tabs, ev, ctr)
    book, when, over, unm = _brute(n_nodes, width, ev, quantities)
    assert (ctr[0] - 5, ctr[1] - 7) == (over, unm) == (counts["overflow"], counts["unmatched"]) and over > 0 and unm > 0
    assert counts["closes"] > 0 and counts["appended"] > 0
    for u in range(n_nodes):
        L = int(tabs[1][u])
        assert tabs[0][u, :L].tolist() == [p[0] for p in book[u]] and (tabs[0][u, L:] == -1).all(), u
        if quantities:
            assert tabs[3][u, :L].tolist() == [p[1] for p in book[u]] and not tabs[3][u, L:].any(), u
        assert tabs[2][u] == when.get(u, -np.inf)


def test_reference_first_occurrence_and_seeded_rows():
    """Rows the snapshot writer seeded may hold duplicates, negative entries and a length beyond the row."""
    idx, ln, tm = HR.new_tables(6, 5)
    HR.store(idx, ln, tm, [2, 3], [[7, -1, 7, 9, 7], [4, 4, -3, 4, 1]], [5, 9], [1.0, 1.0])
    qty = None
    c = TR.apply(idx, ln, tm, [2, 2, 3, 3, 3], [7, -1, 4, -3, 8], [-1, -1, -1, -1, 1], np.arange(5.0) + 2, qty)
    assert idx[2].tolist() == [-1, 7, 9, 7, -1] and ln[2] == 4, "the FIRST 7 is closed; a negative stock is no event"
    assert idx[3].tolist() == [4, -3, 4, 1, 8] and ln[3] == 5, "the first 4 closes, the stored -3 is not addressable, 8 goes behind"
    assert (c["valid"], c["closes"], c["overflow"], c["unmatched"]) == (3, 2, 0, 0) and tm[2] == 2.0 and tm[3] == 6.0
    idx[3, 4], ln[3] = 1, 99                                     # a stored length beyond the row is clamped, and kept when nothing moves
    c = TR.apply(idx, ln, tm, [3, 3], [8, 1], [1, 1], [7.0, 8.0])
    assert c["overflow"] == 1 and ln[3] == 99 and tm[3] == 8.0
    c = TR.apply(idx, ln, tm, [3], [1], [-1], [9.0])
    assert idx[3].tolist() == [4, -3, 4, 1, -1] and ln[3] == 4, "the first 1 closes, the last slot is cleared"


def test_reference_quantities():
    tabs = _tables(4, 3, True)
    ev = (np.array([1, 1, 1, 1, 1, 1, 1]), np.array([5, 5, 6, 5, 5, 6, 6]), np.array([1, 1, 1, -1, -1, -1, 1]),
          np.arange(7.0), np.array([1.5, 2.0, 1.0, 3.0, 0.5, np.nan, np.inf]))
    c = _run(tabs, ev)
    assert tabs[0][1].tolist() == [6, -1, -1] and tabs[3][1].tolist() == [1.0, 0.0, 0.0] and tabs[1][1] == 1
    assert c["valid"] == 5 and c["qty_added"] == 1 and c["qty_reduced"] == 1 and c["closes"] == 1 and tabs[2][1] == 4.0
    c = TR.apply(*tabs[:3], [1], [6], [-1], [9.0], qty=tabs[3])  # no qty_in: every quantity is 1.0
    assert tabs[1][1] == 0 and tabs[3][1].tolist() == [0.0] * 3 and c["closes"] == 1


def test_composition_at_every_cut():
    for quantities, width in ((False, 2), (True, 3)):
        n_nodes, N = 6, 60
        ev = TR.make_case(11, n_nodes, width, N, None, quantities)
        whole, ctr = _tables(n_nodes, width, quantities), np.zeros(2, np.int64)
        _run(whole, ev, ctr)
        assert ctr.sum() > 0 and whole[1].sum() > 0
        for cut in range(N + 1):
            parts, c2 = _tables(n_nodes, width, quantities), np.zeros(2, np.int64)
            _run(parts, tuple(None if a is None else a[:cut] for a in ev), c2)
            _run(parts, tuple(None if a is None else a[cut:] for a in ev), c2)
            assert _same(parts, whole) and np.array_equal(c2, ctr), cut


def test_snapshot_equivalence():
    """Feeding the snapshot writer each user's row after each event leaves what the trades leave (no quantities)."""
    for seed, n_nodes, width, N in ((21, 7, 3, 300), (22, 12, 1, 200), (23, 5, 6, 400)):
        ev = TR.make_case(seed, n_nodes, width, N)
        trades, snap = HR.new_tables(n_nodes, width), HR.new_tables(n_nodes, width)
        for e in range(N):
            c = TR.apply(*trades, *(a[e:e + 1] for a in ev[:4]))
            if c["valid"]:
                HR.store(*snap, *TR.final_rows(*trades, [ev[0][e]]))
        assert _same(snap, trades)
        once = HR.new_tables(n_nodes, width)                     # ... and so does one store of the final rows and last times
        named = np.flatnonzero(np.isfinite(trades[2]))
        HR.store(*once, *TR.final_rows(*trades, named))
        assert _same(once, trades) and named.size > 2


@pytest.mark.parametrize("quantities", [False, True])
def test_reload_round_trip(quantities):
    """A saved ledger reloads as one buy per stored slot in slot order at the row's time."""
    n_nodes, width = 9, 4
    ev = TR.make_case(31, n_nodes, width, 300, None, quantities)
    saved = _tables(n_nodes, width, quantities)
    _run(saved, ev)
    assert (saved[1] > 0).sum() >= 5
    saved[2][saved[1] == 0] = -np.inf                            # (a row that was emptied has a time; the reload gives it none)
    fresh = _tables(n_nodes, width, quantities)
    src, stock, side, ts, q = TR.reload_events(*saved)
    c = TR.apply(*fresh[:3], src, stock, side, ts, qty=fresh[3], qty_in=q)
    assert c["valid"] == c["appended"] == int(saved[1].sum()) and _same(fresh, saved)


def test_issue_cases_bind():
    """The GPU file's binding condition, on the reference alone: cases 3 - 6 meet every branch."""
    want = {3: (316, 663, 122, 544, 193), 4: (338, 792, 692, 0, 0), 5: (638, 561, 119, 780, 433), 6: (198, 867, 566, 0, 0)}
    for seed, n_nodes, width, N, users, quantities in TR.CASES:
        if seed not in want:
            continue
        tabs = _tables(n_nodes, width, quantities)
        c = _run(tabs, TR.make_case(seed, n_nodes, width, N, users, quantities))
        assert (c["overflow"], c["unmatched"], c["middle_closes"], c["qty_added"], c["qty_reduced"]) == want[seed], seed


# ---------------------------------------------------------------------------------------------- 2. the symbols
def test_symbols_in_header_library_and_prototypes():
    from pfotgnrec_amd import _lib
    import ctypes as C
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "pfotgn.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name) and name in _lib.PROTOTYPES, name
    proto = re.search(r"int\s+pfo_holdings_apply\s*\(([^)]*)\)", text).group(1)
    params = [p.strip() for p in proto.split(",")]
    res, args = _lib.PROTOTYPES["pfo_holdings_apply"]
    assert res is C.c_int and len(args) == len(params) == 16
    for p, a in zip(params, args):
        assert a is (C.c_void_p if "*" in p else C.c_int64 if p.startswith("int64_t") else C.c_int32), p
    assert [p.split()[-1].lstrip("*") for p in params] == ["src", "stock", "side", "qty", "ts", "N", "hold_idx", "hold_len", "hold_time",
                                                          "hold_qty", "n_nodes", "W", "counters", "scratch", "scratch_bytes", "stream"]
    assert _lib.PROTOTYPES["pfo_holdings_apply_scratch_bytes"] == (C.c_int64, [C.c_int64, C.c_int64])
    assert lib.pfo_abi_version() == 6
    import pfotgnrec_amd as P
    for name in ("trade_holdings", "holdings_counters"):
        assert hasattr(P.TGN, name)
    assert hasattr(P, "holdings_apply") and hasattr(P, "holdings_store")


def _apply(N=1, n_nodes=10, W=4, scratch_bytes=1 << 20):
    from pfotgnrec_amd import _lib
    return _lib.call("pfo_holdings_apply", None, None, None, None, None, N, None, None, None, None, n_nodes, W, None, None,
                     scratch_bytes, None)


def test_limits_are_refused_before_anything_is_dereferenced():
    """Every pointer is NULL: a limit that was checked behind a read would crash instead of refusing."""
    from pfotgnrec_amd import _lib
    for w in (0, -1, 257):
        with pytest.raises(_lib.PfoError, match=r"pfo_holdings_apply: W must lie in \[1, 256\]"):
            _apply(W=w)
    for n in (0, -3, 2 ** 31):
        with pytest.raises(_lib.PfoError, match=r"pfo_holdings_apply: n_nodes must lie in \[1, 2\^31\)"):
            _apply(n_nodes=n)
    for N in (-1, 2 ** 31):
        with pytest.raises(_lib.PfoError, match=r"pfo_holdings_apply: N must lie in \[0, 2\^31\)"):
            _apply(N=N)
    with pytest.raises(_lib.PfoError, match="pfo_holdings_apply: null pointer"):
        _apply()
    _apply(N=0)                                                 # nothing is queued, nothing is looked at
    _apply(N=0, W=256, n_nodes=2 ** 31 - 1)
    lib = _lib.load()
    assert lib.pfo_holdings_apply_scratch_bytes(0, 1) == -1 and lib.pfo_holdings_apply_scratch_bytes(5, -1) == -1
    assert lib.pfo_holdings_apply_scratch_bytes(5, 2 ** 31) == -1 and lib.pfo_holdings_apply_scratch_bytes(2 ** 31, 5) == -1
    assert b"pfo_holdings_apply_scratch_bytes" in lib.pfo_last_error()
    small, large = lib.pfo_holdings_apply_scratch_bytes(50000, 512), lib.pfo_holdings_apply_scratch_bytes(50000, 200000)
    assert 2 * 512 * 4 <= small <= 3 * 512 * 4 + 1024, "a tick: the keys and one permutation (it sorts in LDS)"
    assert large >= 3 * 200000 * 4 + 2 * 256 * 196 * 4 and lib.pfo_holdings_apply_scratch_bytes(7, 200000) == large
    assert lib.pfo_holdings_apply_scratch_bytes(1, 0) >= 0


def test_functional_checks_on_the_host():
    import pfotgnrec_amd as P
    from pfotgnrec_amd import _lib
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32)
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64)
    good = dict(src=i32(5), stock=i32(5), side=i32(5), ts=f64(5), hold_idx=i32(9, 3), hold_len=i32(9), hold_time=f64(9))
    for kw, msg in ((dict(hold_len=i32(8)), "the ledger must be"), (dict(hold_time=f64(9).float()), "the ledger must be"),
                    (dict(hold_qty=f64(9, 2)), "quantities must be f64"), (dict(hold_qty=i32(9, 3)), "quantities must be f64"),
                    (dict(hold_idx=i32(9, 6)[:, ::2]), "contiguous"), (dict(counters=i32(2)), "counters must be int64"),
                    (dict(counters=torch.zeros(3, dtype=torch.int64)), "counters must be int64"),
                    (dict(stock=i32(4)), "events must be"), (dict(side=i32(5).long()), "events must be"),
                    (dict(ts=f64(5).float()), "events must be"), (dict(qty=f64(4)), "events must be"), (dict(src=i32(5, 1)), "events must be")):
        with pytest.raises(ValueError, match=msg):
            P.holdings_apply(**dict(good, **kw))
    if not torch.cuda.is_available():
        with pytest.raises(_lib.PfoError):                       # valid: only the device is missing - no fallback
            P.holdings_apply(**good)


def test_op_is_registered_with_a_fake():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from pfotgnrec_amd import ops  # noqa: F401
    assert hasattr(torch.ops.pfotgn, "holdings_apply")
    schema = str(torch.ops.pfotgn.holdings_apply.default._schema)
    for name in ("hold_idx", "hold_len", "hold_time", "hold_qty", "counters"):
        assert re.search(r"Tensor\(\w+!\)\?? %s\b" % name, schema), (name, schema)        # written in place
    with FakeTensorMode():
        i32 = lambda *s: torch.empty(s, dtype=torch.int32)
        f64 = lambda *s: torch.empty(s, dtype=torch.float64)
        out = torch.ops.pfotgn.holdings_apply(i32(5), i32(5), i32(5), f64(5), i32(9, 3), i32(9), f64(9), None, None)
        assert out is None
        out = torch.ops.pfotgn.holdings_apply(i32(5), i32(5), i32(5), f64(5), i32(9, 3), i32(9), f64(9), f64(9, 3),
                                              torch.empty(2, dtype=torch.int64), qty=f64(5))
        assert out is None


# ---------------------------------------------------------------------------------------------- 3. the Python surface on a host model
def _host_model(track=True, quantities=False):
    import pfotgnrec_amd as P
    from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
    g = make_graph(SyntheticConfig("t", 50, 10, 400, 8, 1, 4, 2), with_prices=False)
    nf = P.get_neighbor_finder(g.data, False)
    tgn = P.TGN(nf, g.node_features, g.edge_features, "cpu", n_layers=1, n_heads=2, use_memory=True, memory_dimension=8,
                message_function="identity")
    if track:
        tgn.track_holdings(W, UPPER_U, quantities=quantities)
        rs = np.random.RandomState(4)                           # non-trivial content, so that "kept bit for bit" says something
        h = tgn.holdings
        with torch.no_grad():
            h.idx.copy_(torch.from_numpy(rs.randint(-1, 10, size=tuple(h.idx.shape)).astype(np.int32)))
            h.len.copy_(torch.from_numpy(rs.randint(0, W + 1, size=tgn.n_nodes).astype(np.int32)))
            h.time.copy_(torch.from_numpy(rs.rand(tgn.n_nodes)))
            if quantities:
                h.qty.copy_(torch.from_numpy(rs.rand(*h.qty.shape)))
    return tgn, g


def _snapshot(tgn):
    """The ledger with its counters, the edge table, n_nodes and the memory tables: row counts, addresses and every bit."""
    m, h = tgn.memory, tgn.holdings
    tabs = [tgn.node_raw_features, tgn.edge_raw_features, m.memory.data, m.last_update.data, m.msg_table, m.msg_time, m.has_msg]
    if h is not None:
        tabs += [h.idx, h.len, h.time, h.counters] + ([h.qty] if h.quantities else [])
    return (tgn.n_nodes, tgn._cfg.n_nodes, tgn._cfg.n_edges_p1, tgn.neighbor_finder.n_nodes, tgn.neighbor_finder._version,
            None if h is None else (h.n_nodes, h.capacity, h.width, h.upper_u, h.quantities),
            tuple((tuple(t.shape), t.data_ptr(), t.numpy().tobytes()) for t in tabs))


def test_track_holdings_quantities():
    tgn, _ = _host_model(track=False)
    h = tgn.track_holdings(W, UPPER_U, quantities=True)
    assert h.quantities and h.qty.dtype == torch.float64 and tuple(h.qty.shape) == (tgn.n_nodes, W) and not h.qty.any()
    assert h.counters.dtype == torch.int64 and h.counters.tolist() == [0, 0] and tgn.holdings_counters() == (0, 0)
    assert tgn.track_holdings(W, UPPER_U, quantities=True) is h and tgn.track_holdings(W, UPPER_U, True) is h
    for other in (dict(), dict(quantities=False)):
        with pytest.raises(ValueError, match="already tracks"):
            tgn.track_holdings(W, UPPER_U, **other)
    plain, _ = _host_model()
    assert plain.holdings.qty is None and not plain.holdings.quantities and plain.holdings.counters.tolist() == [0, 0]
    assert len(plain.holdings._store.storage) == 3 and len(h._store.storage) == 4
    with pytest.raises(ValueError, match="already tracks"):
        plain.track_holdings(W, UPPER_U, quantities=True)
    assert not any("holdings" in k for k in tgn.state_dict()), "not part of the checkpoint"
    # qty is capacity storage: reserve / add_nodes keep it bit for bit, new rows are 0.0, a move carries it and the counters
    tgn2, _ = _host_model(quantities=True)
    h, n = tgn2.holdings, tgn2.n_nodes
    before = h.qty.numpy().copy()
    tgn2.reserve(n_nodes=n + 7)
    assert HR.same_bits(h.qty.numpy(), before) and not h._store.storage[3][n:].any() and h.qty.data_ptr() == h._store.storage[3].data_ptr()
    assert tgn2.add_nodes(30) == n and tuple(h.qty.shape) == (n + 30, W) and h.capacity == tgn2.node_capacity
    assert HR.same_bits(h.qty.numpy()[:n], before) and not h.qty[n:].any()
    h.counters += torch.tensor([3, 4])
    tgn2.to("cpu")
    tgn2.float()
    assert h.qty.dtype == torch.float64 and HR.same_bits(h.qty.numpy()[:n], before) and tgn2.holdings_counters() == (3, 4)


def _trade_args(g, n=6):
    d = g.data
    return dict(sources=d.sources[:n].copy(), stocks=(d.destinations[:n] - UPPER_U - 1).copy(), sides=np.array([1, -1, 1, 1, -1, 1]),
                edge_times=d.timestamps[:n].copy())


BAD_TRADES = ["length_sources", "length_stocks", "length_sides", "length_times", "float_sources", "float_stocks", "float_sides",
              "string_times", "stock_beyond_int32", "node_beyond_table", "node_negative", "side_zero", "side_two",
              "device_stocks_with_host_sources", "two_d_sources"]
BAD_QTY = ["qty_length", "qty_zero", "qty_negative", "qty_nan", "qty_inf", "qty_strings", "qty_device_with_host_sources"]


def _spoil(kw, case, n_nodes):
    if case.startswith("length_"):
        name = {"sources": "sources", "stocks": "stocks", "sides": "sides", "times": "edge_times"}[case[7:]]
        kw[name] = kw[name][:5]
    elif case.startswith("float_"):
        kw[case[6:]] = kw[case[6:]].astype(np.float64)
    elif case == "string_times":
        kw["edge_times"] = ["a"] * 6
    elif case == "stock_beyond_int32":
        kw["stocks"] = kw["stocks"].astype(np.int64)
        kw["stocks"][2] = 2 ** 31
    elif case == "node_beyond_table":
        kw["sources"][3] = n_nodes
    elif case == "node_negative":
        kw["sources"][3] = -1
    elif case == "side_zero":
        kw["sides"][1] = 0
    elif case == "side_two":
        kw["sides"][4] = 2
    elif case == "device_stocks_with_host_sources":
        kw["stocks"] = torch.from_numpy(kw["stocks"].astype(np.int32))
    elif case == "two_d_sources":
        kw["sources"] = kw["sources"].reshape(2, 3)
    elif case == "qty_length":
        kw["quantities"] = np.ones(5)
    elif case == "qty_strings":
        kw["quantities"] = ["1"] * 6
    elif case == "qty_device_with_host_sources":
        kw["quantities"] = torch.ones(6, dtype=torch.float64)
    elif case.startswith("qty_"):
        kw["quantities"] = np.where(np.arange(6) == 2, {"zero": 0.0, "negative": -1.0, "nan": np.nan, "inf": np.inf}[case[4:]], 1.0)
    return kw


@pytest.mark.parametrize("case", BAD_TRADES + BAD_QTY + ["qty_on_a_plain_ledger"])
def test_rejected_trade_holdings_leaves_everything(case):
    quantities = case in BAD_QTY
    tgn, g = _host_model(quantities=quantities)
    if case == "qty_on_a_plain_ledger":
        kw = dict(_trade_args(g), quantities=np.ones(6))
    else:
        kw = _spoil(_trade_args(g), case, tgn.n_nodes)
    before = _snapshot(tgn)
    with pytest.raises(ValueError):
        tgn.trade_holdings(**kw)
    assert _snapshot(tgn) == before


def test_device_trades_are_checked_for_shape_and_dtype():
    tgn, _ = _host_model(quantities=True)
    i32, f64 = (lambda n: torch.zeros(n, dtype=torch.int32)), (lambda n: torch.zeros(n, dtype=torch.float64))
    before = _snapshot(tgn)
    for args in ((i32(4), i32(4), i32(4).long(), f64(4)), (i32(4), i32(3), i32(4), f64(4)), (i32(4), i32(4), i32(4), f64(4).float()),
                 (i32(4), i32(4), i32(4), f64(4), f64(4).float()), (i32(4), i32(4), i32(4), f64(4), f64(5)),
                 (i32(4).reshape(2, 2), i32(4), i32(4), f64(4))):
        with pytest.raises(ValueError, match="device inputs must be"):
            tgn.trade_holdings(*args)
    assert _snapshot(tgn) == before


def test_valid_writes_reach_the_device_check_and_change_nothing_on_a_host_model():
    from pfotgnrec_amd import _lib
    for quantities in (False, True):
        tgn, g = _host_model(quantities=quantities)
        kw = _trade_args(g)
        before = _snapshot(tgn)
        with pytest.raises(_lib.PfoError):
            tgn.trade_holdings(**kw)
        with pytest.raises(_lib.PfoError):
            tgn.trade_holdings(kw["sources"].tolist(), kw["stocks"].astype(np.int16), kw["sides"].astype(np.int8), kw["edge_times"].astype(np.int64))
        if quantities:
            with pytest.raises(_lib.PfoError):
                tgn.trade_holdings(**kw, quantities=[1, 2, 3, 4, 5, 6])
        d = g.data
        dst = d.destinations[:6].copy()
        dst[2] = tgn.n_nodes
        with pytest.raises(_lib.PfoError):
            tgn.ingest(kw["sources"], dst, d.timestamps[-1] + 1.0 + np.arange(6), np.zeros((6, 4)), portfolios="buys")
        assert _snapshot(tgn) == before
        assert tgn.trade_holdings([], [], [], []) == 0
        assert tgn.ingest(kw["sources"][:0], dst[:0], kw["edge_times"][:0], np.zeros((0, 4)), portfolios="buys")[0] == 0
        assert _snapshot(tgn) == before


def test_without_a_ledger_and_the_snapshot_writers_on_a_quantity_ledger():
    tgn, g = _host_model(track=False)
    kw, d = _trade_args(g), g.data
    before = _snapshot(tgn)
    with pytest.raises(ValueError, match="track_holdings"):
        tgn.trade_holdings(**kw)
    with pytest.raises(ValueError, match="track_holdings"):
        tgn.holdings_counters()
    tick = (kw["sources"], d.destinations[:6], d.timestamps[-1] + 1.0 + np.arange(6), np.zeros((6, 4)))
    with pytest.raises(ValueError, match="track_holdings"):
        tgn.ingest(*tick, portfolios="buys")
    assert _snapshot(tgn) == before
    tgn, g = _host_model(quantities=True)
    before = _snapshot(tgn)
    ports = (g.portfolio_idx[:6, :W].copy(), np.minimum(g.portfolio_len[:6], W))
    with pytest.raises(ValueError, match="trades only"):
        tgn.update_holdings(kw["sources"], ports, kw["edge_times"])
    with pytest.raises(ValueError, match="trades only"):
        tgn.holdings.store(*(torch.zeros(1, dtype=torch.int32),) * 3, torch.zeros(1, dtype=torch.float64))
    for p in (ports, [[1]] * 6):
        with pytest.raises(ValueError, match="trades only"):
            tgn.ingest(*tick, portfolios=p)
    assert _snapshot(tgn) == before
    # ingest's own checks come before the buys: a rejected tick leaves the ledger too
    for quantities in (False, True):
        tgn, g = _host_model(quantities=quantities)
        before = _snapshot(tgn)
        with pytest.raises(ValueError):
            tgn.ingest(tick[0], tick[1], tick[2][::-1].copy(), tick[3], portfolios="buys")
        with pytest.raises(ValueError):
            tgn.ingest(tick[0], tick[1], tick[2], np.zeros((6, 5)), portfolios="buys")
        with pytest.raises(ValueError):
            tgn.ingest(tick[0], tick[1], tick[2], tick[3], portfolios="sells")
        assert _snapshot(tgn) == before


def test_backtest_checks_advance_holdings_before_any_device_work():
    import pfotgnrec_amd as P
    from pfotgnrec_amd import _lib
    p = 100.0 + np.arange(2 * 4 * 6, dtype=np.float64).reshape(2, 4, 6)
    tables = P.InvestTables.from_prices(["20200101", "20200102"], p, p + 1.0, {"a": 0, "b": 1, "c": 2, "d": 3}, upper_u=20)
    n = 8
    base = dict(sources=np.arange(1, n + 1), destinations=np.arange(21, 21 + n), edge_times=20200101000000.0 + np.arange(n),
                edge_idxs=np.arange(1, n + 1), items=np.arange(21, 25), k=3, cutoffs=(1, 3), batch_size=4, tables=tables)
    none = types.SimpleNamespace(holdings=None, device=torch.device("cuda:0"), n_nodes=40)
    other = types.SimpleNamespace(holdings=types.SimpleNamespace(upper_u=21, width=4), device=torch.device("cuda:0"), n_nodes=40)
    for fn in (P.backtest, P.backtest_rows):
        with pytest.raises(ValueError, match="advance_holdings needs a holdings ledger"):
            fn(none, **base, advance_holdings=True)
        with pytest.raises(ValueError, match="number the stocks differently"):
            fn(other, **base, advance_holdings=True)
        with pytest.raises(ValueError, match="batch_size must be at least 1"):          # (with the others: any of them refuses)
            fn(none, **dict(base, batch_size=0), advance_holdings=True)
    tgn, _ = _host_model()
    tgn.holdings.upper_u = 20
    before = _snapshot(tgn)
    with pytest.raises(_lib.PfoError):                           # valid: only the device is missing
        P.backtest_rows(tgn, **base, advance_holdings=True)
    assert _snapshot(tgn) == before


def test_new_keywords_and_their_defaults():
    import importlib
    import pfotgnrec_amd as P
    BT = importlib.import_module("pfotgnrec_amd.backtest")
    for fn in (P.backtest, P.backtest_rows, BT.check):
        params = inspect.signature(fn).parameters
        last = list(params)[-1]
        assert last == "advance_holdings" and params[last].kind is inspect.Parameter.KEYWORD_ONLY and params[last].default is False
    params = inspect.signature(P.TGN.track_holdings).parameters
    assert list(params) == ["self", "width", "upper_u", "quantities"] and params["quantities"].default is False
    params = inspect.signature(P.TGN.trade_holdings).parameters
    assert list(params) == ["self", "sources", "stocks", "sides", "edge_times", "quantities"] and params["quantities"].default is None
    assert inspect.signature(P.TGN.ingest).parameters["portfolios"].default is None
    params = inspect.signature(P.holdings_apply).parameters
    assert list(params)[:7] == ["src", "stock", "side", "ts", "hold_idx", "hold_len", "hold_time"]
    assert all(params[n].default is None for n in ("qty", "hold_qty", "counters", "scratch"))
