"""GPU tests of holdings from trades: ``pfo_holdings_apply`` on raw tensors against the numpy loop of
``holdings_trades_ref`` - every comparison bitwise, the feature has no tolerance - and the serving surface (``trade_holdings``,
``ingest(portfolios="buys")``, ``backtest_rows(advance_holdings=True)``, ``forget`` / ``reserve`` / ``add_nodes`` over ``qty``) on
the served world of ``test_gpu_holdings``.  The cases are the smallest shapes at which the kernels can go wrong: widths 1 / 3 / 8
and a row of exactly one, one-past-one and four 64-slot pieces, one event past two radix tiles' worth of a small call, a chain
far longer than a wavefront pass, ids of one, two and three radix digits, and the 64-event boundary of the walk."""
import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

import pfotgnrec_amd as P
from pfotgnrec_amd import _lib
import holdings_ref as HR
import holdings_trades_ref as TR
import test_gpu_holdings as GH                                   # the served world: its graph, its model, its constants

DEV = "cuda:0"
GUARD = 3                                                        # canary rows in front of and behind every table


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                  # (a copy: the shared reference arrays are read-only)


def _host(*ts):
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


def _same(got, want, what=""):
    for name, a, b in zip(("idx", "len", "time", "qty"), got, want):
        assert (a is None and b is None) or HR.same_bits(a, b), "%s %s" % (what, name)


# ---------------------------------------------------------------------------------------------- 1. the kernel on raw tensors
_REF = {}


def _reference(case):
    """Computed once per case and left unchanged: the events, the reference's tables and counters, its counts."""
    if case not in _REF:
        seed, n_nodes, W, N, users, quantities = case
        ev = TR.make_case(seed, n_nodes, W, N, users, quantities)
        tabs = HR.new_tables(n_nodes, W) + ((TR.new_qty(n_nodes, W),) if quantities else (None,))
        ctr = np.array([11, 13], np.int64)                       # the call ADDS to what is there
        counts = TR.apply(*tabs[:3], *ev[:4], qty=tabs[3], qty_in=ev[4], counters=ctr)
        for a in ev + tabs + (ctr,):
            if a is not None:
                a.setflags(write=False)
        _REF[case] = (ev, tabs, ctr, counts)
    return _REF[case]


class _Guarded:
    """Fresh ledger tables on the device inside canary rows: the kernel sees the middle views."""

    def __init__(self, n_nodes, W, quantities):
        shapes = [((W,), torch.int32, -1, 777), ((), torch.int32, 0, 888), ((), torch.float64, float("-inf"), 99.5)]
        if quantities:
            shapes.append(((W,), torch.float64, 0.0, -5.25))
        self.full, self.canary = [], []
        for trail, dt, init, canary in shapes:
            t = torch.full((n_nodes + 2 * GUARD,) + trail, canary, dtype=dt, device=DEV)
            t[GUARD:GUARD + n_nodes] = init
            self.full.append(t)
            self.canary.append(canary)
        self.views = [t[GUARD:GUARD + n_nodes] for t in self.full] + ([] if quantities else [None])
        self.counters = torch.tensor([11, 13], dtype=torch.int64, device=DEV)

    def apply(self, ev, lo=0, hi=None, scratch=None):
        cols = [None if a is None else a[lo:hi] for a in ev]
        P.holdings_apply(cols[0], cols[1], cols[2], cols[3], *self.views[:3], cols[4], self.views[3], self.counters, scratch)

    def host(self):
        return _host(*self.views)

    def canaries_intact(self):
        torch.cuda.synchronize()
        return all(bool((t[:GUARD] == c).all()) and bool((t[-GUARD:] == c).all()) for t, c in zip(self.full, self.canary))


@pytest.mark.parametrize("case", TR.CASES, ids=["case%d" % c[0] for c in TR.CASES])
def test_apply_is_the_sequential_loop(case):
    seed, n_nodes, W, N, users, quantities = case
    ev, want, want_ctr, counts = _reference(case)
    # the binding condition, from the reference, before the case is trusted
    if seed in (3, 4, 5, 6):
        assert counts["overflow"] > 0 and counts["unmatched"] > 0 and counts["middle_closes"] > 0, counts
    if seed in (3, 5):
        assert counts["qty_added"] > 0 and counts["qty_reduced"] > 0, counts
    dev_ev = tuple(None if a is None else _dev(a) for a in ev)
    first = _Guarded(n_nodes, W, quantities)
    scratch = torch.full((_lib.byte_count("pfo_holdings_apply_scratch_bytes", n_nodes, N) + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    first.apply(dev_ev, scratch=scratch)                         # (a caller's scratch; its content on entry must not matter)
    got = first.host()
    _same(got, want, "case %d" % seed)
    assert np.array_equal(first.counters.cpu().numpy(), want_ctr), "counters: overflow, unmatched"
    assert first.canaries_intact(), "rows around the tables"
    assert bool((scratch[-64:] == 0xA5).all()), "bytes behind the scratch the library asked for"
    for a, b in zip(_host(*dev_ev), ev):
        assert (a is None and b is None) or HR.same_bits(a, b), "the inputs are never written"
    # a second run on fresh tables, the library's own scratch: the same bits
    second = _Guarded(n_nodes, W, quantities)
    second.apply(dev_ev)
    _same(second.host(), got, "repeat")
    assert torch.equal(second.counters, first.counters)
    # composition on the device: the same events cut into two calls
    parts = _Guarded(n_nodes, W, quantities)
    parts.apply(dev_ev, 0, N // 3, scratch)
    parts.apply(dev_ev, N // 3, None, scratch)
    _same(parts.host(), got, "two calls cut at %d" % (N // 3))
    assert torch.equal(parts.counters, first.counters) and parts.canaries_intact()
    # snapshot equivalence: the snapshot writer fed the final rows and last times leaves the same tables
    if not quantities:
        named = np.flatnonzero(np.isfinite(want[2])).astype(np.int32)
        snap = _Guarded(n_nodes, W, False)
        rows = TR.final_rows(*want[:3], named)
        P.holdings_store(_dev(rows[0]), _dev(rows[1]), _dev(rows[2]), _dev(rows[3]), *snap.views[:3])
        _same(snap.host(), got, "pfo_holdings_store of the final rows")


def test_rows_seeded_by_the_snapshot_writer_follow_the_first_occurrence():
    """A duplicate and a -1 inside ``len``, a full row of two pieces: written by ``pfo_holdings_store``, then traded."""
    n_nodes, W = 40, 70                                          # two pieces: the duplicate's copies sit in different ones
    seed_rows = np.full((3, W), -1, np.int32)
    seed_rows[0, :6] = [7, -1, 7, 9, 7, 3]
    seed_rows[1, :W] = np.arange(W) % 67                          # full: stocks 0, 1, 2 twice, the second copies in slots 67 .. 69
    seed_rows[2, :4] = [5, 5, -1, 5]
    users, lens, t0 = np.array([2, 39, 17], np.int32), np.array([6, W + 9, 4], np.int32), np.array([1.0, 2.0, 3.0])
    ev = (np.array([2, 2, 39, 39, 39, 39, 17, 17, 17, 2], np.int32), np.array([7, -1, 1, 1, 68, 68, 5, 5, 5, 7], np.int32),
          np.array([-1, -1, -1, -1, 1, 1, -1, 1, -1, 1], np.int32), np.arange(10.0) + 5, None)
    want = HR.new_tables(n_nodes, W)
    HR.store(*want, users, seed_rows, lens, t0)
    ctr = np.zeros(2, np.int64)
    TR.apply(*want, *ev[:4], counters=ctr)
    assert want[0][2, :6].tolist() == [-1, 7, 9, 7, 3, -1] and want[1][2] == 5, "the first 7 went; the buy of 7 found the next one"
    assert want[1][39] == W - 1 and want[0][39, :3].tolist() == [0, 2, 3] and want[0][39, 62:].tolist() == [63, 64, 65, 66, 0, 2, 68, -1]
    assert want[0][17, :4].tolist() == [-1, 5, -1, -1] and want[1][17] == 2 and ctr.tolist() == [0, 0]
    tabs = _Guarded(n_nodes, W, False)
    P.holdings_store(_dev(users), _dev(seed_rows), _dev(lens), _dev(t0), *tabs.views[:3])
    tabs.counters.zero_()
    tabs.apply(tuple(None if a is None else _dev(a) for a in ev))
    _same(tabs.host(), want + (None,), "seeded rows")
    assert np.array_equal(tabs.counters.cpu().numpy(), ctr) and tabs.canaries_intact()


@pytest.mark.parametrize("quantities", [False, True])
def test_empty_and_all_invalid_calls_write_nothing(quantities):
    n_nodes, W, N = 70, 8, 300
    ev, want, _, _ = _reference(TR.CASES[2])                     # a ledger with content: case 3's result
    tabs = _Guarded(n_nodes, W, True)
    tabs.apply(tuple(None if a is None else _dev(a) for a in ev))
    before, ctr = tabs.host(), tabs.counters.clone()
    rs = np.random.RandomState(5)
    src, stock, side = rs.randint(1, n_nodes, N).astype(np.int32), rs.randint(0, 16, N).astype(np.int32), rs.choice([1, -1], N).astype(np.int32)
    qty = np.ones(N)
    kind = np.arange(N) % 5                                      # every event is invalid, each for one reason
    src[kind == 0] = rs.choice([0, -1, n_nodes, -2 ** 31, 2 ** 31 - 1], (kind == 0).sum())
    stock[kind == 1] = rs.choice([-1, -2 ** 31], (kind == 1).sum())
    side[kind == 2] = rs.choice([0, 2, -2, 2 ** 31 - 1], (kind == 2).sum())
    if quantities:
        qty[kind == 3] = rs.choice([0.0, -0.0, -1.0, np.nan, np.inf, -np.inf], (kind == 3).sum())
        qty[kind == 4] = np.nan
    else:
        src[kind >= 3] = 0
    bad = tuple(_dev(a) for a in (src, stock, side, np.arange(N, dtype=np.float64))) + ((_dev(qty),) if quantities else (None,))
    tabs.apply(bad)
    tabs.apply(bad, 0, 0)                                        # N == 0
    P.holdings_apply(bad[0][:0], bad[1][:0], bad[2][:0], bad[3][:0], *tabs.views[:3])
    _same(tabs.host(), before, "nothing is written, not even the time")
    assert torch.equal(tabs.counters, ctr) and tabs.canaries_intact()
    # without quantities in the ledger the events' are ignored: the same tables as without them
    a, b = _Guarded(n_nodes, W, False), _Guarded(n_nodes, W, False)
    cols = tuple(_dev(x) for x in ev[:4])
    a.apply(cols + (_dev(ev[4]),))
    b.apply(cols + (None,))
    _same(a.host(), b.host(), "qty without hold_qty")
    assert torch.equal(a.counters, b.counters)


def test_refuses_without_writing():
    tabs = _Guarded(10, 4, True)
    before = tabs.host()
    src, ts = _dev(np.array([3], np.int32)), _dev(np.array([1.0]))
    lib = _lib.load()
    v = tabs.views
    rc = lib.pfo_holdings_apply(src.data_ptr(), src.data_ptr(), src.data_ptr(), None, ts.data_ptr(), 1, v[0].data_ptr(), v[1].data_ptr(),
                                v[2].data_ptr(), v[3].data_ptr(), 10, 4, None, v[1].data_ptr(), 7, _lib.stream_ptr())
    assert rc != 0 and b"pfo_holdings_apply: short scratch" in lib.pfo_last_error()
    with pytest.raises(ValueError):
        P.holdings_apply(src, src, src, ts.float(), *v[:3])
    _same(tabs.host(), before)


# ---------------------------------------------------------------------------------------------- 2. end to end on the served world
WIDTH, ITEMS, CUT, TICK = GH.WIDTH, GH.ITEMS, GH.CUT, GH.TICK


def _trades_of(g, lo, hi, rs=None):
    """The interactions [lo, hi) as a feed: buys of the item taken, and - with ``rs`` - some of them turned into sells."""
    d = g.data
    side = np.ones(hi - lo, np.int32)
    if rs is not None:
        side[rs.rand(hi - lo) < 0.3] = -1
    return d.sources[lo:hi], (d.destinations[lo:hi] - g.upper_u - 1), side, d.timestamps[lo:hi]


def _ledger(tgn):
    h = tgn.holdings
    return _host(h.idx, h.len, h.time, h.qty)


def _seeded(g, quantities):
    """A served model whose ledger took the first CUT interactions as trades, and the reference ledger beside it."""
    tgn = GH._model(g, 1)
    tgn.track_holdings(WIDTH, g.upper_u, quantities=quantities)
    rs = np.random.RandomState(3)
    feed = _trades_of(g, 0, CUT, rs)
    qty = rs.choice([0.5, 1.0, 2.0], CUT) if quantities else None
    assert tgn.trade_holdings(*feed, quantities=qty) == CUT
    ref = HR.new_tables(tgn.n_nodes, WIDTH) + ((TR.new_qty(tgn.n_nodes, WIDTH),) if quantities else (None,))
    ctr = np.zeros(2, np.int64)
    TR.apply(*ref[:3], *feed, qty=ref[3], qty_in=qty, counters=ctr)
    return tgn, ref, ctr


@pytest.mark.parametrize("quantities", [False, True])
def test_trade_holdings_host_and_device_inputs(quantities):
    g = GH._graph(1)
    tgn, ref, ctr = _seeded(g, quantities)
    _same(_ledger(tgn), ref, "host feed")
    assert tgn.holdings_counters() == tuple(ctr.tolist()) and ctr[1] > 0 and (ref[1] > 1).sum() > 30
    rs = np.random.RandomState(9)
    feed = _trades_of(g, CUT, CUT + 200, rs)
    qty = rs.choice([0.5, 1.0, 3.0], 200) if quantities else None
    twin, _, _ = _seeded(g, quantities)
    assert tgn.trade_holdings(*feed, quantities=qty) == 200
    on_dev = [_dev(np.ascontiguousarray(a, dtype=dt)) for a, dt in zip(feed, (np.int32, np.int32, np.int32, np.float64))]
    assert twin.trade_holdings(*on_dev, quantities=None if qty is None else _dev(qty)) == 200
    TR.apply(*ref[:3], *feed, qty=ref[3], qty_in=qty, counters=ctr)
    _same(_ledger(tgn), ref, "host tick")
    _same(_ledger(twin), ref, "device tick")
    assert tgn.holdings_counters() == twin.holdings_counters() == tuple(ctr.tolist())
    # device inputs are not validated on the host: the kernel's skipping rules apply
    src = np.array([0, -3, tgn.n_nodes, 4, 4, 4], np.int32)
    stock, side, ts = np.array([1, 1, 1, -1, 2, 2], np.int32), np.array([1, 1, 1, 1, 0, 1], np.int32), np.arange(6.0)
    twin.trade_holdings(_dev(src), _dev(stock), _dev(side), _dev(ts))
    TR.apply(*ref[:3], src, stock, side, ts, qty=ref[3])
    _same(_ledger(twin), ref, "unchecked device inputs")
    assert ref[2][4] == 5.0
    # a saved ledger reloads through trade_holdings: one buy per stored slot
    fresh = GH._model(g, 1)
    fresh.track_holdings(WIDTH, g.upper_u, quantities=quantities)
    ev = TR.reload_events(*ref)
    fresh.trade_holdings(*ev[:4], quantities=ev[4])
    got = _ledger(fresh)
    live = ref[1] > 0
    assert live.sum() > 60 and all(a is None or HR.same_bits(a[live], b[live]) for a, b in zip(got, ref))
    assert np.isneginf(got[2][~live]).all() and not got[1][~live].any()


def test_ingest_buys_is_ingest_then_trade_holdings():
    g = GH._graph(1)
    d = g.data
    for quantities, batch_size in ((False, 7), (True, None)):
        a, ref, ctr = _seeded(g, quantities)
        b, _, _ = _seeded(g, quantities)
        for s in range(CUT, CUT + 4 * TICK, TICK):
            sb, db, tb, fb, _ = GH._tick(g, s)
            n, _ = a.ingest(sb, db, tb, fb, batch_size=batch_size, portfolios="buys")
            assert n == TICK
            b.ingest(sb, db, tb, fb, batch_size=batch_size)
            b.trade_holdings(sb, db - g.upper_u - 1, np.ones(TICK, np.int64), tb)
            TR.apply(*ref[:3], sb, db - g.upper_u - 1, np.ones(TICK, np.int32), tb, qty=ref[3], counters=ctr)
        _same(_ledger(a), ref, "buys")
        _same(_ledger(b), ref, "ingest, then trades")
        assert a.holdings_counters() == b.holdings_counters() == tuple(ctr.tolist())
    # device inputs; a user as a destination is no item: a negative stock, skipped - and a new node's row starts at the initial values
    a, ref, ctr = _seeded(g, True)
    sb, db, tb, fb, _ = GH._tick(g, CUT)
    db = db.copy()
    db[3] = 7
    to = lambda x, dt: _dev(np.ascontiguousarray(x, dtype=dt))
    a.ingest(to(sb, np.int32), to(db, np.int32), to(tb, np.float64), to(fb, np.float32), portfolios="buys")
    TR.apply(*ref[:3], sb, db - g.upper_u - 1, np.ones(TICK, np.int32), tb, qty=ref[3], counters=ctr)
    _same(_ledger(a), ref, "device tick")
    n0 = a.n_nodes
    a.ingest(np.array([n0, 5]), np.array([130, n0 + 1]), tb[-1] + 1.0 + np.arange(2), np.zeros((2, 4)), portfolios="buys")
    got = _ledger(a)
    assert a.n_nodes == n0 + 2 and got[0][n0].tolist() == [130 - g.upper_u - 1] + [-1] * (WIDTH - 1) and got[3][n0, 0] == 1.0
    assert got[1][n0 + 1] == 0 and np.isneginf(got[2][n0 + 1]) and got[2][5] == tb[-1] + 2.0, "stock n0 + 1 - upper_u - 1 is bought like any"


def test_held_queries_after_trades():
    g = GH._graph(1, prices=True)
    tgn, ref, _ = _seeded(g, True)
    mv = P.MVSampler(g.prices, g.upper_u, DEV, day_of=g.day_of)
    users = np.concatenate([np.flatnonzero(ref[1][:GH.N_USERS + 1] > 1)[:9], np.flatnonzero(ref[1][1:GH.N_USERS + 1] == 0)[:1] + 1])
    now = float(g.data.timestamps[CUT]) + 1.0
    lists = HR.held_node_lists(ref[0], ref[1], users, g.upper_u)
    rows = (ref[0][users], ref[1][users])
    assert sum(len(r) for r in lists) > 20
    a = tgn.recommend(users, now, 5, ITEMS, mv=mv, exclude="held", portfolios="held")
    b = tgn.recommend(users, now, 5, ITEMS, mv=mv, exclude=lists, portfolios=rows)
    assert len(a) == 4 and all(torch.equal(x, y) for x, y in zip(a, b))
    plain = tgn.recommend(users, now, 5, ITEMS, mv=mv, portfolios=rows)
    assert not torch.equal(a[0], plain[0]), "the exclusion must move something, or the test shows nothing"
    a = tgn.recommend(users, now, 5, ITEMS, only="held")
    b = tgn.recommend(users, now, 5, ITEMS, only=lists)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_forget_reserve_and_add_nodes_over_quantities():
    g = GH._graph(1)
    tgn, ref, _ = _seeded(g, True)
    h, n = tgn.holdings, tgn.n_nodes
    before = _ledger(tgn)
    assert (before[3] > 0).sum() > 100
    tgn.reserve(n_nodes=n + 50)
    assert h.capacity == tgn.node_capacity == n + 50
    _same(_ledger(tgn), before, "reserve")
    assert tgn.add_nodes(70) == n and h.n_nodes == n + 70
    got = _ledger(tgn)
    _same(tuple(x[:n] for x in got), before, "add_nodes")
    assert not got[3][n:].any() and (got[0][n:] == -1).all()
    gone = np.flatnonzero(before[1] > 1)[:3]
    tgn.forget(gone)
    got = _ledger(tgn)
    kept = np.setdiff1d(np.arange(n), gone)
    assert not got[3][gone].any() and (got[0][gone] == -1).all() and not got[1][gone].any() and np.isneginf(got[2][gone]).all()
    assert all(HR.same_bits(a[kept], b[kept]) for a, b in zip(got, before)), "every other row keeps every bit"
    # a forgotten id starts like a new node
    u = int(gone[0])
    tgn.trade_holdings([u], [4], [1], [1e9], quantities=[2.5])
    got = _ledger(tgn)
    assert got[0][u].tolist() == [4] + [-1] * (WIDTH - 1) and got[3][u].tolist() == [2.5] + [0.0] * (WIDTH - 1) and got[1][u] == 1


class _SynTables(P.InvestTables):
    """InvestTables over the synthetic calendar: the day of a timestamp is the graph's ``day_of``."""

    def day_indices(self, timestamps):
        return ((np.asarray(timestamps).astype(np.int64) * 64) >> 24).astype(np.int32)


def test_backtest_advances_the_ledger_batch_by_batch():
    g = GH._graph(1, prices=True)
    d = g.data
    LOG, BATCH, CUTS = 48, 16, (1, 3, 5)
    sl = slice(CUT, CUT + LOG)
    src, dst, ts, eidx = d.sources[sl].copy(), d.destinations[sl], d.timestamps[sl], d.edge_idxs[sl]
    src[BATCH:] = np.tile(src[:BATCH], 2)                        # the users of batch 0 come back: they meet rows the walk wrote
    mv = P.MVSampler(g.prices, g.upper_u, DEV, day_of=g.day_of)
    tables = _SynTables.from_prices(list(range(64)), g.prices, g.prices * 1.01, g.map_item_id, upper_u=g.upper_u)
    rp, rf = tables.device_tables(DEV)
    days = _dev(np.asarray(g.day_of(ts)).astype(np.int32))

    def model():
        torch.manual_seed(6)
        nf = P.NeighborFinder.from_arrays(d.sources[:CUT], d.destinations[:CUT], d.edge_idxs[:CUT], d.timestamps[:CUT], uniform=False,
                                          max_node_idx=g.node_features.shape[0] - 1)
        t = P.TGN(nf, g.node_features, g.edge_features, DEV, n_layers=1, n_heads=2, dropout=0.0, use_memory=True, memory_dimension=16,
                  message_function="identity", n_neighbors=GH.K_NBR)
        t.eval()
        t.track_holdings(WIDTH, g.upper_u)
        t.trade_holdings(*_trades_of(g, 0, CUT, np.random.RandomState(3)))
        return t

    kw = dict(cutoffs=CUTS, batch_size=BATCH, tables=tables, mv=mv, portfolios="held", exclude="held", keep_truth=False)
    a, b, c = model(), model(), model()
    start, start_ctr = _ledger(a), a.holdings_counters()
    rows = P.backtest_rows(a, src, dst, ts, eidx, ITEMS, 5, advance_holdings=True, **kw)
    ref = tuple(x if x is None else x.copy() for x in start)
    moved = 0
    for lo in range(0, LOG, BATCH):
        hi = lo + BATCH
        res = b.recommend(src[lo:hi], ts[lo:hi], 5, ITEMS, mv=mv, portfolios="held", exclude="held")
        assert np.array_equal(res[0].cpu().numpy(), rows["list_item"][lo:hi]), lo
        pidx, plen = b.holdings.rows(src[lo:hi])
        want_rows = (ref[0][src[lo:hi]], ref[1][src[lo:hi]])
        assert HR.same_bits(pidx.cpu().numpy(), want_rows[0]) and HR.same_bits(plen.cpu().numpy(), want_rows[1]), "held = before THIS batch"
        moved += int(lo > 0 and not HR.same_bits(want_rows[0], start[0][src[lo:hi]]))
        hand = P.list_metrics(res[0], _dev(dst[lo:hi].astype(np.int32)), CUTS, pidx, plen, g.upper_u, rp, days[lo:hi], rf, days[lo:hi], res[2])
        for name, x in zip(("rank", "recall", "ndcg", "invest"), hand):
            assert HR.same_bits(x.cpu().numpy(), rows[name][lo:hi]), (name, lo)
        b.observe(src[lo:hi], dst[lo:hi], ts[lo:hi], eidx[lo:hi], batch_size=None)
        b.trade_holdings(src[lo:hi], dst[lo:hi] - g.upper_u - 1, np.ones(BATCH, np.int32), ts[lo:hi])
        TR.apply(*ref[:3], src[lo:hi], dst[lo:hi] - g.upper_u - 1, np.ones(BATCH, np.int32), ts[lo:hi])
    assert moved >= 1, "a later batch must meet rows the walk itself wrote, or the test shows nothing"
    _same(_ledger(a), _ledger(b), "the ledger ends where the walk by hand leaves it")
    _same(_ledger(a), ref, "... which is the reference's")
    assert not HR.same_bits(_ledger(a)[0], start[0])
    # the default: the holdings ledger is not written
    plain = P.backtest_rows(c, src, dst, ts, eidx, ITEMS, 5, **kw)
    _same(_ledger(c), start, "advance_holdings=False")
    assert c.holdings_counters() == start_ctr
    assert np.array_equal(plain["list_item"][:BATCH], rows["list_item"][:BATCH]), "batch 0 meets the same ledger"
    assert not np.array_equal(plain["list_item"], rows["list_item"]) or not np.array_equal(plain["invest"], rows["invest"])
