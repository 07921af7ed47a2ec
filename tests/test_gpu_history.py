"""GPU tests of the history gather: ``pfo_history_gather`` on raw tensors against the numpy rule of ``history_ref`` -
every comparison exact: integers, and fp64 timestamps as bit patterns - on the cases ``tests/test_history_cpu.py`` proves
binding, and ``TGN.recommend(exclude="seen" / only="seen" / portfolios="seen")``, ``TGN.history`` and ``backtest_rows`` on small
served models against the same calls fed the reference's rows as explicit lists / packed pairs.  The shapes are the smallest at
which the kernel can go wrong: rows around one and two chunks of 64, one of 5000 (three search steps), widths 1 / 8 / 64 / 256."""
import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

import pfotgnrec_amd as P
from pfotgnrec_amd import _lib
from pfotgnrec_amd.neighbor_finder import build_csr
from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
import history_ref as H

DEV = "cuda:0"
CANARY = 64                     # elements behind every output, checked after every launch
OUTPUTS = (("node", np.int32, -77), ("len", np.int32, -77), ("time", np.float64, 123.25), ("count", np.int32, -77),
           ("pos", np.int32, -77), ("stock", np.int32, -77))


def _dev(a, dt=None):
    return torch.from_numpy(np.array(a, dtype=dt)).to(DEV)         # (a copy: broadcast views are not writable)


def _launch(csr_dev, users, ts, since, W, max_scan, want, items=None, pos_scratch=None, upper_u=0):
    """One call of the C entry over buffers with a canary tail -> dict of host arrays; the canaries and every input are checked."""
    U = len(users)
    ins = dict(users=_dev(users, np.int32), ts=_dev(ts, np.float64), since=None if since is None else _dev(since, np.float64),
               items=None if items is None else _dev(items, np.int32))
    before = {k: v.clone() for k, v in ins.items() if v is not None}
    bufs = {}
    for name, dt, fill in OUTPUTS:
        if name in want:
            n = U if name == "len" else U * W
            bufs[name] = torch.full((n + CANARY,), fill, dtype=getattr(torch, np.dtype(dt).name), device=DEV)
    if "pos" in want and pos_scratch is None:
        pos_scratch = torch.empty(int(csr_dev[0].shape[0]) - 1, dtype=torch.int32, device=DEV)
    _lib.call("pfo_history_gather", csr_dev[0].data_ptr(), csr_dev[1].data_ptr(), csr_dev[2].data_ptr(), int(csr_dev[0].shape[0]) - 1,
              ins["users"].data_ptr(), ins["ts"].data_ptr(), _lib.ptr(ins["since"]), U, W, max_scan, _lib.ptr(ins["items"]),
              1 if items is None else len(items), _lib.ptr(pos_scratch if "pos" in want else None), upper_u,
              bufs["node"].data_ptr(), bufs["len"].data_ptr(), _lib.ptr(bufs.get("time")), _lib.ptr(bufs.get("count")),
              _lib.ptr(bufs.get("pos")), _lib.ptr(bufs.get("stock")), _lib.stream_ptr())
    torch.cuda.synchronize()
    out = {}
    for name, dt, fill in OUTPUTS:
        if name in want:
            h = bufs[name].cpu().numpy()
            n = U if name == "len" else U * W
            assert (h[n:] == fill).all(), "canary behind %s" % name
            out[name] = h[:n] if name == "len" else h[:n].reshape(U, W)
    assert all(torch.equal(ins[k].view(torch.uint8), v.view(torch.uint8)) for k, v in before.items()), "inputs are not written"
    return out


def _check(got, ref, what):
    for name in got:
        assert H.same_bits(got[name], getattr(ref, name)), "%s: %s" % (what, name)


@pytest.fixture(scope="module")
def raw_world():
    csr = H.world()
    return csr, tuple(_dev(a) for a in csr)


# ---------------------------------------------------------------------------------------------- 1. the kernel on raw tensors
@pytest.mark.parametrize("W", H.WIDTHS)
@pytest.mark.parametrize("U", H.USER_COUNTS)
def test_gather_is_the_reference(raw_world, U, W):
    """Every call of the case (``history_ref.calls``): all outputs, then the same call without ``count_out`` - the walk may stop
    when the list is full, and node / len / time must not notice."""
    csr, csr_dev = raw_world
    before = [a.clone() for a in csr_dev]
    items = np.concatenate([np.arange(30, 50), [H.N_NODES + 5, 0], np.arange(100, 130), np.arange(1190, 1210)])     # some past the table
    for seed, max_scan in H.calls(U):
        users, ts, since = H.queries(csr[0], csr[2], U, seed)
        ref = H.gather(*csr, users, ts, W, since, max_scan, items, H.UPPER_U)
        what = "U=%d W=%d seed=%d max_scan=%d" % (U, W, seed, max_scan)
        _check(_launch(csr_dev, users, ts, since, W, max_scan, ("node", "len", "time", "count", "pos", "stock"), items, None, H.UPPER_U), ref, what)
        _check(_launch(csr_dev, users, ts, since, W, max_scan, ("node", "len", "time")), ref, what + " no counts")
        if seed % 4 == 3:
            no_since = H.gather(*csr, users, ts, W, None, max_scan)
            _check(_launch(csr_dev, users, ts, None, W, max_scan, ("node", "len", "count")), no_since, what + " since NULL")
    assert all(torch.equal(a, b) for a, b in zip(csr_dev, before)), "the adjacency is not written"


@pytest.mark.parametrize("row", range(1, 14))
def test_every_row_at_every_cut(raw_world, row):
    """One row, queried at every distinct timestamp of it (strict: ties excluded) and past its end, 67 queries a launch; with
    ``since`` ON entries' timestamps (inclusive).  Rows 1 .. 8 have the lengths 0 / 1 / 63 / 64 / 65 / 129 / 300 / 5000."""
    csr, csr_dev = raw_world
    rs = np.random.RandomState(row)
    row_ts = csr[2][csr[0][row]:csr[0][row + 1]]
    cuts = np.unique(np.concatenate([row_ts, [row_ts[-1] + 1.0 if len(row_ts) else 1.0]]))
    cuts = cuts[np.sort(rs.permutation(len(cuts))[:67])] if len(cuts) > 67 else cuts
    users = np.full(len(cuts), row)
    since = np.where(rs.rand(len(cuts)) < 0.5, cuts[rs.randint(0, len(cuts), size=len(cuts))], np.nan)
    for W, max_scan in ((1, 0), (8, 65), (64, 0), (256, 0), (256, 64), (8, 1)):
        ref = H.gather(*csr, users, cuts, W, since, max_scan)
        _check(_launch(csr_dev, users, cuts, since, W, max_scan, ("node", "len", "time", "count")), ref, "row %d W=%d" % (row, W))


def test_positions_survive_a_stale_scratch(raw_world):
    """``pos_scratch`` left over from another ``items``, and filled with values that look like positions: an entry is trusted
    only if ``items`` names the node there."""
    csr, csr_dev = raw_world
    users, ts, since = H.queries(csr[0], csr[2], 67, 3)
    first = np.arange(1, 1200)                                  # every neighbour id is a candidate: position = id - 1
    second = np.concatenate([np.arange(900, 1000), [3, 41, 42], np.arange(200, 260)])[::-1].copy()
    for fill in (None, 0, 5, -1, H.I32_MAX):
        scratch = torch.empty(H.N_NODES, dtype=torch.int32, device=DEV) if fill is None else torch.full((H.N_NODES,), fill, dtype=torch.int32,
                                                                                                        device=DEV)
        for items in (first, second, np.asarray([41]), second):
            ref = H.gather(*csr, users, ts, 64, since, 0, items, H.UPPER_U)
            if items is second:
                assert (ref.pos >= 0).any() and ((ref.pos == -1) & (ref.node >= 0)).any(), "candidates and non-candidates are seen"
            _check(_launch(csr_dev, users, ts, since, 64, 0, ("node", "len", "pos"), items, scratch), ref, "fill %s, I=%d" % (fill, len(items)))
    # stock indices around upper_u: node upper_u is no stock, node upper_u + 1 is stock 0
    ref = H.gather(*csr, [6, 7, 8], [1e9] * 3, 64, None, 0, None, H.UPPER_U)
    assert {-1, 0} <= set(ref.stock.ravel().tolist()) and (ref.node == H.UPPER_U).any() and (ref.node == H.UPPER_U + 1).any()
    _check(_launch(csr_dev, [6, 7, 8], [1e9] * 3, None, 64, 0, ("node", "len", "stock"), upper_u=H.UPPER_U), ref, "stock")
    big = H.gather(*csr, [6, 7, 8], [1e9] * 3, 64, None, 0, None, H.I32_MAX - 1)
    assert (big.stock == -1).all()
    _check(_launch(csr_dev, [6, 7, 8], [1e9] * 3, None, 64, 0, ("node", "len", "stock"), upper_u=H.I32_MAX - 1), big, "stock, huge upper_u")


def test_functional_and_op_forms(raw_world):
    csr, csr_dev = raw_world
    users, ts, since = H.queries(csr[0], csr[2], 67, 3)
    items = np.arange(1, 700)
    ref = H.gather(*csr, users, ts, 8, since, 65, items, H.UPPER_U)
    args = (*csr_dev, _dev(users, np.int32), _dev(ts), 8, _dev(since), 65)
    got = P.history_gather(*args, _dev(items, np.int32), None, H.UPPER_U, ("stock", "node", "len", "time", "count", "pos"))
    torch.cuda.synchronize()
    _check(dict(zip(("stock", "node", "len", "time", "count", "pos"), (t.cpu().numpy() for t in got))), ref, "functional")
    assert len(P.history_gather(*args)) == 4 and len(P.history_gather(*args, want=("len",))) == 1
    from pfotgnrec_amd import ops  # noqa: F401
    op = torch.ops.pfotgn.history_gather(*args, items=_dev(items, np.int32), upper_u=H.UPPER_U)
    _check(dict(zip(("node", "len", "time", "count", "pos", "stock"), (t.cpu().numpy() for t in op))), ref, "op")
    op = torch.ops.pfotgn.history_gather(*args)
    assert tuple(op[4].shape) == (67, 0) and tuple(op[5].shape) == (67, 0) and H.same_bits(op[0].cpu().numpy(), ref.node)
    empty = P.history_gather(*csr_dev, _dev(np.zeros(0, np.int32)), _dev(np.zeros(0)), 8)
    assert tuple(empty[0].shape) == (0, 8) and tuple(empty[1].shape) == (0,)


# ---------------------------------------------------------------------------------------------- 2. the served model
N_USERS, N_ITEMS, K_NBR, TICK, CUT, WIDTH = 120, 30, 5, 24, 900, 8
ITEMS = np.arange(N_USERS + 1, N_USERS + N_ITEMS + 1)


def _model(g, L, cut=CUT):
    d = g.data
    nf = P.NeighborFinder.from_arrays(d.sources[:cut], d.destinations[:cut], d.edge_idxs[:cut], d.timestamps[:cut], uniform=False,
                                      max_node_idx=g.node_features.shape[0] - 1)
    tgn = P.TGN(nf, g.node_features, g.edge_features[:cut + 1], DEV, n_layers=L, n_heads=2, dropout=0.0, use_memory=True,
                memory_dimension=16, message_function="identity", n_neighbors=K_NBR)
    tgn.eval()
    return tgn


def _ref_csr(g, n, cutoff=None):
    """The adjacency of the first ``n`` interactions, built on the host; ``cutoff``: entries before it expired."""
    d = g.data
    indptr, nbr, _, ts = build_csr(d.sources[:n], d.destinations[:n], d.edge_idxs[:n], d.timestamps[:n], g.node_features.shape[0] - 1)
    if cutoff is not None:
        keep = ts >= cutoff
        owner = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
        indptr = np.concatenate([[0], np.cumsum(np.bincount(owner[keep], minlength=len(indptr) - 1))]).astype(np.int64)
        nbr, ts = nbr[keep], ts[keep]
    return indptr, nbr, ts


def _snapshot(tgn):
    m, h = tgn.memory, tgn.holdings
    state = [m.memory, m.last_update, m.msg_table, m.msg_time, m.has_msg, tgn.flat_parameters]
    state += list(tgn.neighbor_finder.device_arrays(tgn.device))
    if h is not None:
        state += [h.idx, h.len, h.time]
    return [x.detach().clone() for x in state], (tgn._step, tgn.training, tgn.neighbor_finder._version)


def _unchanged(tgn, snap):
    now = _snapshot(tgn)
    return now[1] == snap[1] and all(torch.equal(a, b) for a, b in zip(now[0], snap[0]))


def _eq(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("L", [1, 2])
def test_served_seen_queries(L):
    torch.manual_seed(5 + L)
    g = make_graph(SyntheticConfig("t", N_USERS, N_ITEMS, 1500, 16, L, K_NBR, 2), with_prices=True)
    d = g.data
    tgn = _model(g, L)
    tgn.track_holdings(WIDTH, g.upper_u)
    tgn.update_holdings(d.sources[:CUT], (g.portfolio_idx[:CUT], g.portfolio_len[:CUT]), d.timestamps[:CUT])
    mv = P.MVSampler(g.prices, g.upper_u, DEV, day_of=g.day_of)
    groups = np.arange(N_ITEMS) % 4
    n_seen, cutoff = CUT, None
    for phase in ("start", "ingest", "expire"):
        if phase == "ingest":                                   # new interactions: their neighbours are seen
            s = slice(CUT, CUT + 4 * TICK)
            n, _ = tgn.ingest(d.sources[s], d.destinations[s], d.timestamps[s], g.edge_features[d.edge_idxs[s]], batch_size=TICK)
            assert n == 4 * TICK
            n_seen = CUT + 4 * TICK
        elif phase == "expire":                                 # ... and expired ones are not
            cutoff = float(d.timestamps[600])
            assert tgn.expire(cutoff)[0] > 0
        csr = _ref_csr(g, n_seen, cutoff)
        recent = d.sources[n_seen - 40:n_seen]
        users = np.concatenate([np.unique(recent)[:12], [int(recent[-1])] * 2, [int(ITEMS[0])]])      # an item node too: its row names users
        now = float(d.timestamps[n_seen - 1]) + 1.0
        two = np.where(np.arange(len(users)) % 2 == 0, now, float(d.timestamps[n_seen - 20]))          # ON an entry's time for some
        snap = _snapshot(tgn)
        for ts, seen_kw in ((now, {}), (two, {}), (now, dict(seen_width=3)), (two, dict(seen_since=float(d.timestamps[n_seen - 200]), seen_max_scan=6)),
                            (now, dict(seen_since=np.where(np.arange(len(users)) % 3 == 0, np.nan, float(d.timestamps[n_seen - 300]))))):
            q_ts = np.broadcast_to(np.asarray(ts, np.float64), (len(users),))
            sn = seen_kw.get("seen_since")
            sn = None if sn is None else np.broadcast_to(np.asarray(sn, np.float64), (len(users),))
            ref = H.gather(*csr, users, q_ts, seen_kw.get("seen_width", 256), sn, seen_kw.get("seen_max_scan", 0), ITEMS, g.upper_u)
            lists = H.node_lists(ref)
            ports = (ref.stock, ref.len)
            what = "%s %s" % (phase, sorted(seen_kw))
            assert sum(len(r) for r in lists) > 15 and (ref.pos >= 0).sum() > 15, what
            plain = tgn.recommend(users, ts, 5, ITEMS)
            got = tgn.recommend(users, ts, 5, ITEMS, exclude="seen", **seen_kw)
            assert _eq(got, tgn.recommend(users, ts, 5, ITEMS, exclude=lists)), what
            assert not torch.equal(got[0], plain[0]), "the exclusion must move something, or the test shows nothing"
            ids = got[0].cpu().numpy()
            assert all(not (set(ids[q].tolist()) & set(lists[q])) for q in range(len(users)))
            got = tgn.recommend(users, ts, 5, ITEMS, only="seen", **seen_kw)
            assert _eq(got, tgn.recommend(users, ts, 5, ITEMS, only=lists)), what
            ids = got[0].cpu().numpy()
            assert all(set(ids[q].tolist()) - {-1} <= set(lists[q]) for q in range(len(users))) and (ids >= 0).any()
            for kw_seen, kw_ref in ((dict(portfolios="seen"), dict(portfolios=ports)),
                                    (dict(portfolios="seen", exclude="seen"), dict(portfolios=ports, exclude=lists)),
                                    (dict(portfolios="seen", basket=True), dict(portfolios=ports, basket=True)),
                                    (dict(portfolios="seen", only="seen"), dict(portfolios=ports, only=lists)),
                                    (dict(portfolios="held", exclude="seen"), dict(portfolios="held", exclude=lists)),
                                    (dict(portfolios="seen", exclude="held"), dict(portfolios=ports, exclude="held")),
                                    (dict(portfolios="held", only="seen"), dict(portfolios="held", only=lists)),
                                    (dict(portfolios="seen", groups=groups, group_cap=1, held_groups="portfolios", stock_groups=groups),
                                     dict(portfolios=ports, groups=groups, group_cap=1, held_groups="portfolios", stock_groups=groups))):
                a = tgn.recommend(users, ts, 5, ITEMS, mv=mv, **kw_seen, **seen_kw)
                b = tgn.recommend(users, ts, 5, ITEMS, mv=mv, **kw_ref)
                assert len(a) == 4 and _eq(a, b), "%s %s" % (what, sorted(kw_seen))
            # device inputs take the same route
            dev_kw = dict(seen_kw)
            if sn is not None:
                dev_kw["seen_since"] = _dev(sn)
            a = tgn.recommend(_dev(users, np.int32), _dev(q_ts), 5, ITEMS, exclude="seen", **dev_kw)
            assert _eq(a, tgn.recommend(users, ts, 5, ITEMS, exclude=lists)), what + " device inputs"
            # TGN.history: the rows themselves
            hist = tgn.history(users, ts, seen_kw.get("seen_width", 256), seen_kw.get("seen_since"), seen_kw.get("seen_max_scan", 0), items=ITEMS)
            torch.cuda.synchronize()
            _check(dict(zip(("node", "len", "time", "count", "pos"), (t.cpu().numpy() for t in hist))), ref, what + " history")
        assert len(tgn.history(users, now, 4)) == 4
        assert _unchanged(tgn, snap), "no model state, ledger row or finder array is written (%s)" % phase
        if phase == "ingest":
            fresh = H.gather(*_ref_csr(g, CUT), users, np.full(len(users), now), 256)
            assert (H.gather(*csr, users, np.full(len(users), now), 256).len > fresh.len).any(), "the tick brought new neighbours"
        if phase == "expire":
            older = H.gather(*_ref_csr(g, n_seen), users, np.full(len(users), now), 256)
            assert (H.gather(*csr, users, np.full(len(users), now), 256).len < older.len).any(), "the expiry took neighbours away"


# ---------------------------------------------------------------------------------------------- 3. backtest
B_USERS, B_ITEMS, B_CUT, B_LOG, B_BATCH, N_DAYS = 30, 40, 300, 64, 16, 64
B_ITEM_IDS = np.arange(B_USERS + 1, B_USERS + B_ITEMS + 1)
CUTS = (1, 3, 5, 10)


class _SynTables(P.InvestTables):
    """InvestTables over the synthetic calendar: the day of a timestamp is the graph's ``day_of``."""

    def day_indices(self, timestamps):
        return ((np.asarray(timestamps).astype(np.int64) * N_DAYS) >> 24).astype(np.int32)


@pytest.fixture(scope="module")
def bt_world():
    g = make_graph(SyntheticConfig("t", B_USERS, B_ITEMS, 400, 16, 2, K_NBR, 2), with_prices=True)
    rs = np.random.RandomState(4)
    future = g.prices * np.exp(np.cumsum(rs.randn(*g.prices.shape) * 0.02, axis=2))
    tables = _SynTables.from_prices(list(range(N_DAYS)), g.prices, future, g.map_item_id, upper_u=g.upper_u)
    return g, tables, P.MVSampler(g.prices, g.upper_u, DEV, day_of=g.day_of)


def _bt_model(g):
    """A served model whose finder holds the FULL log: the strict comparison serves the prequential walk without append."""
    torch.manual_seed(6)
    d = g.data
    nf = P.NeighborFinder.from_arrays(d.sources, d.destinations, d.edge_idxs, d.timestamps, uniform=False,
                                      max_node_idx=g.node_features.shape[0] - 1)
    t = P.TGN(nf, g.node_features, g.edge_features, DEV, n_layers=2, n_heads=2, dropout=0.0, use_memory=True, memory_dimension=16,
              message_function="identity", n_neighbors=K_NBR)
    t.eval()
    t.observe(d.sources[:B_CUT], d.destinations[:B_CUT], d.timestamps[:B_CUT], d.edge_idxs[:B_CUT], batch_size=50)
    return t


@pytest.mark.parametrize("form", ["keep_truth", "leave_rows", "mv_portfolios", "mv_held_groups"])
def test_backtest_seen_is_recommend_score_observe_by_hand(bt_world, form):
    g, tables, mv = bt_world
    d = g.data
    sl = slice(B_CUT, B_CUT + B_LOG)
    src, dst, ts, eidx = d.sources[sl], d.destinations[sl], d.timestamps[sl], d.edge_idxs[sl]
    keep = form != "leave_rows"
    kw = dict(exclude="seen", keep_truth=keep, seen_width=16, seen_since=float(d.timestamps[40]))
    with_mv = form in ("mv_portfolios", "mv_held_groups")
    cap = {}
    if form == "mv_held_groups":                                # the seen rows also count against a cap of one pick a group
        groups = np.arange(B_ITEMS) % 5
        cap = dict(groups=groups, group_cap=1, held_groups="portfolios", stock_groups=groups)
    if with_mv:
        kw.update(mv=mv, portfolios="seen", **cap)
    a, b = _bt_model(g), _bt_model(g)
    rows = P.backtest_rows(a, src, dst, ts, eidx, B_ITEM_IDS, 10, cutoffs=CUTS, batch_size=B_BATCH, tables=tables, **kw)
    csr = _ref_csr(g, 400)
    rp, rf = tables.device_tables(DEV)
    days = _dev(tables.day_indices(ts), np.int32)
    rebought = 0
    for lo in range(0, B_LOG, B_BATCH):
        hi = lo + B_BATCH
        ref = H.gather(*csr, src[lo:hi], ts[lo:hi], 16, np.full(hi - lo, float(d.timestamps[40])), 0, None, g.upper_u)
        lists = H.node_lists(ref)
        rebought += sum(int(dst[lo + q]) in lists[q] for q in range(hi - lo))
        if keep:
            lists = [[v for v in r if v != int(dst[lo + q])] for q, r in enumerate(lists)]
        side = dict(mv=mv, portfolios=(ref.stock, ref.len), **cap) if with_mv else {}
        res = b.recommend(src[lo:hi], ts[lo:hi], 10, B_ITEM_IDS, exclude=lists, **side)
        assert np.array_equal(res[0].cpu().numpy(), rows["list_item"][lo:hi]), (form, lo)
        assert np.array_equal(res[2].cpu().numpy(), rows["n_valid"][lo:hi])
        pidx, plen = (_dev(ref.stock), _dev(ref.len)) if with_mv else (None, None)
        hand = P.list_metrics(res[0], _dev(dst[lo:hi], np.int32), CUTS, pidx, plen, g.upper_u, rp, days[lo:hi], rf, days[lo:hi], res[2])
        for name, h in zip(("rank", "recall", "ndcg", "invest"), hand):
            assert H.same_bits(h.cpu().numpy(), rows[name][lo:hi]), (form, name, lo)
        b.observe(src[lo:hi], dst[lo:hi], ts[lo:hi], eidx[lo:hi], batch_size=None)
    assert rebought >= 3, "users who take an item they have seen: keep_truth decides whether it can be offered"
    taken_seen = [i for i in range(B_LOG) if int(dst[i]) in H.node_lists(H.gather(*csr, src[i:i + 1], ts[i:i + 1], 16,
                                                                                  np.full(1, float(d.timestamps[40]))))[0]]
    if not keep:
        assert all(dst[i] not in rows["list_item"][i] for i in taken_seen) and (rows["rank"][taken_seen] == _lib.EVAL_RANK_NONE).all()
    m = a.memory
    assert all(torch.equal(x, y) for x, y in zip((m.memory, m.last_update, m.msg_table), (b.memory.memory, b.memory.last_update, b.memory.msg_table)))
