"""GPU tests of the holdings ledger: ``pfo_holdings_store`` / ``pfo_holdings_gather`` on raw tensors and the ledger
of a served model, all against the numpy rules of ``holdings_ref`` - every comparison bitwise (integer tables; times as bits) -
and ``TGN.recommend(exclude="held", portfolios="held")`` against the same query fed from the reference ledger through the
list / packed routes.  The shapes are the smallest at which the kernels can go wrong: N around the wavefront and past one and
several workgroups of 256 with every user named many times, widths 1 / 8 / 33 against a stride below, at and above them."""
import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

import pfotgnrec_amd as P
from pfotgnrec_amd import _lib
from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
import holdings_ref as HR

DEV = "cuda:0"
I32_MAX = 2 ** 31 - 1


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(*ts):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in ts)


def _same(got, want, what=""):
    for name, a, b in zip(("idx", "len", "time"), got, want):
        assert HR.same_bits(a, b), "%s %s" % (what, name)


# ---------------------------------------------------------------------------------------------- 1. store on raw tensors
N_NODES = 300


def _events(rs, N, W, stride, pool):
    src = pool[rs.randint(0, len(pool), size=N)].astype(np.int32)
    if N >= 8:
        bad = rs.permutation(N)[:4]
        src[bad] = [0, -5, N_NODES, -I32_MAX]                    # skipped, nothing written
        src[rs.permutation(N)[:2]] = N_NODES - 1                # (the pool holds it too: the last row of the table)
    port_idx = rs.randint(-3, 50, size=(N, stride)).astype(np.int32)
    port_idx[rs.rand(N, stride) < 0.05] = I32_MAX                # stored verbatim
    port_len = np.asarray([0, 1, W, W + 3], np.int32)[rs.randint(0, 4, size=N)]
    ts = rs.rand(N) * 1e9
    return src, port_idx, port_len, ts


@pytest.mark.parametrize("N", [1, 63, 64, 65, 1025, 5000])
def test_store_is_the_sequential_loop(N):
    rs = np.random.RandomState(N)
    pool = np.concatenate([rs.permutation(np.arange(1, N_NODES - 1))[:39], [N_NODES - 1]])    # 40 distinct users
    for W, stride in [(1, 0), (1, 1), (1, 4), (8, 5), (8, 8), (8, 11), (33, 32), (33, 33), (33, 40)]:
        want = (np.full((N_NODES, W), -7, np.int32), np.full(N_NODES, 99, np.int32), np.full(N_NODES, 123.5))     # sentinels
        tabs = tuple(_dev(a) for a in want)
        scratch = torch.full((N_NODES,), I32_MAX, dtype=torch.int32, device=DEV)          # (its content on entry must not matter)
        first = _events(rs, N, W, stride, pool)
        HR.store(*want, *first)
        args = tuple(_dev(a) for a in first)
        P.holdings_store(args[0], args[1], args[2], args[3], *tabs, scratch)
        got = _host(*tabs)
        _same(got, want, "N=%d W=%d stride=%d" % (N, W, stride))
        if N >= 1025:
            assert len(set(first[0].tolist()) & set(pool.tolist())) >= 30 and (want[1] == 99).sum() >= N_NODES - 40, "many rows keep the sentinels"
        # the same call again: the same bits
        P.holdings_store(args[0], args[1], args[2], args[3], *tabs, scratch)
        _same(_host(*tabs), got, "repeat")
        # a second call over the same tables and scratch, the first one's events reversed and renewed: a user's winner now has a
        # SMALLER event index than the stamp the first call left - stamps of one call must not decide the next
        src2, idx2, len2, ts2 = _events(rs, N, W, stride, pool)
        second = (first[0][::-1].copy(), idx2, len2, ts2)
        HR.store(*want, *second)
        P.holdings_store(*(_dev(a) for a in second), *tabs, scratch)
        _same(_host(*tabs), want, "second call N=%d W=%d stride=%d" % (N, W, stride))
        # ... and without a scratch of the caller's
        third = _events(rs, N, W, stride, pool)
        HR.store(*want, *third)
        P.holdings_store(*(_dev(a) for a in third), *tabs)
        _same(_host(*tabs), want, "own scratch")


def test_store_refuses_without_writing():
    tabs = (torch.full((10, 4), -7, dtype=torch.int32, device=DEV), torch.full((10,), 99, dtype=torch.int32, device=DEV),
            torch.full((10,), 1.5, dtype=torch.float64, device=DEV))
    before = _host(*tabs)
    src, idx, ln, ts = _dev(np.array([3], np.int32)), _dev(np.zeros((1, 4), np.int32)), _dev(np.array([2], np.int32)), _dev(np.array([1.0]))
    lib = _lib.load()
    rc = lib.pfo_holdings_store(src.data_ptr(), idx.data_ptr(), ln.data_ptr(), 4, ts.data_ptr(), 1, tabs[0].data_ptr(), tabs[1].data_ptr(),
                                tabs[2].data_ptr(), 10, 4, tabs[1].data_ptr(), 39, _lib.stream_ptr())
    assert rc != 0 and b"short scratch" in lib.pfo_last_error()
    _same(_host(*tabs), before)
    with pytest.raises(ValueError):
        P.holdings_store(src, idx, ln, ts.float(), *tabs)
    _same(_host(*tabs), before)


# ---------------------------------------------------------------------------------------------- 2. gather
G_NODES, G_UPPER, G_W = 1200, 600, 8


def _gather_world():
    rs = np.random.RandomState(77)
    tabs = HR.new_tables(G_NODES, G_W)
    written = rs.permutation(np.arange(1, G_UPPER + 1))[:200]
    idx = rs.randint(0, G_NODES - G_UPPER - 1, size=(200, G_W)).astype(np.int32)      # stocks whose item node exists ...
    idx[rs.rand(200, G_W) < 0.1] = -1
    idx[rs.rand(200, G_W) < 0.1] = I32_MAX                                            # ... and some that name nothing
    idx[rs.rand(200, G_W) < 0.1] = G_NODES - G_UPPER - 1                              # the first stock past the node table
    HR.store(*tabs, written, idx, rs.randint(0, G_W + 1, size=200), rs.rand(200))
    unwritten = int(np.setdiff1d(np.arange(1, G_UPPER + 1), written)[0])
    return rs, tabs, written, unwritten


@pytest.mark.parametrize("U", [1, 17, 300])
@pytest.mark.parametrize("I", [1, 65, 513])
def test_gather_rows_and_positions(U, I):
    rs, tabs, written, unwritten = _gather_world()
    d_idx, d_len = _dev(tabs[0]), _dev(tabs[1])
    user_sets = []
    if U == 1:
        user_sets = [[int(written[0])], [unwritten], [G_NODES], [-4]]
    else:
        users = written[rs.randint(0, 40, size=U)]                # 40 distinct users: repeated
        users[rs.permutation(U)[:3]] = [unwritten, G_NODES, -4]
        user_sets = [users.tolist()]
    # the scratch is kept over every query below; its first content claims position 0 for every node
    pos = torch.zeros(G_NODES, dtype=torch.int32, device=DEV)
    stocks = np.arange(G_UPPER + 1, G_NODES)
    for users in user_sets:
        users = np.asarray(users, np.int32)
        for trial in range(2):                                   # two consecutive queries with different candidate lists
            items = rs.permutation(stocks)[:I].astype(np.int32)  # shuffled order; most holdings name stocks outside it
            want = HR.gather(tabs[0], tabs[1], users, items, G_UPPER)
            got = _host(*P.holdings_gather(_dev(users), d_idx, d_len, G_UPPER, _dev(items), pos))
            for name, a, b in zip(("port_idx", "port_len", "excl_pos"), got, want):
                assert HR.same_bits(a, b), "%s U=%d I=%d trial %d" % (name, U, I, trial)
            if U > 1 and I == 513:
                assert (want[2] >= 0).any() and (want[2] < 0).any()
        # excl_pos_out NULL: rows and lengths alone, nothing else is read
        rows = P.holdings_gather(_dev(users), d_idx, d_len, G_UPPER)
        assert rows[2] is None
        got = _host(*rows[:2])
        assert HR.same_bits(got[0], want[0]) and HR.same_bits(got[1], want[1])


def test_gather_full_candidate_list_excludes_every_held_stock():
    """Every stock is a candidate: each valid entry whose node exists has a position, and it is the right one."""
    rs, tabs, written, _ = _gather_world()
    items = rs.permutation(np.arange(G_UPPER + 1, G_NODES)).astype(np.int32)
    users = written[:64].astype(np.int32)
    want = HR.gather(tabs[0], tabs[1], users, items, G_UPPER)
    got = _host(*P.holdings_gather(_dev(users), _dev(tabs[0]), _dev(tabs[1]), G_UPPER, _dev(items)))
    assert all(HR.same_bits(a, b) for a, b in zip(got, want))
    ok = got[2] >= 0
    assert ok.sum() > 100 and np.array_equal(items[got[2][ok]], got[0][ok] + G_UPPER + 1)


# ---------------------------------------------------------------------------------------------- 3. end to end on the small world
N_USERS, N_ITEMS, K_NBR, TICK, CUT, WIDTH = 120, 30, 5, 24, 900, 8
ITEMS = np.arange(N_USERS + 1, N_USERS + N_ITEMS + 1)


def _graph(L, prices=False):
    torch.manual_seed(5 + L)
    return make_graph(SyntheticConfig("t", N_USERS, N_ITEMS, 1500, 16, L, K_NBR, 2), with_prices=prices)


def _model(g, L):
    d = g.data
    nf = P.NeighborFinder.from_arrays(d.sources[:CUT], d.destinations[:CUT], d.edge_idxs[:CUT], d.timestamps[:CUT], uniform=False,
                                      max_node_idx=g.node_features.shape[0] - 1)
    tgn = P.TGN(nf, g.node_features, g.edge_features[:CUT + 1], DEV, n_layers=L, n_heads=2, dropout=0.0, use_memory=True,
                memory_dimension=16, message_function="identity", n_neighbors=K_NBR)
    tgn.eval()
    return tgn


def _seeded(g, L):
    """A served model whose ledger holds the first CUT interactions' portfolios, and the reference ledger beside it."""
    tgn, d = _model(g, L), g.data
    assert tgn.holdings is None
    tgn.track_holdings(WIDTH, g.upper_u)
    ref = HR.new_tables(tgn.n_nodes, WIDTH)
    assert tgn.update_holdings(d.sources[:CUT], (g.portfolio_idx[:CUT], g.portfolio_len[:CUT]), d.timestamps[:CUT]) == CUT
    HR.store(*ref, d.sources[:CUT], g.portfolio_idx[:CUT], g.portfolio_len[:CUT], d.timestamps[:CUT])
    return tgn, ref


def _ledger(tgn):
    h = tgn.holdings
    return _host(h.idx, h.len, h.time)


def _tick(g, s, n=TICK):
    d = g.data
    return (d.sources[s:s + n], d.destinations[s:s + n], d.timestamps[s:s + n], g.edge_features[d.edge_idxs[s:s + n]],
            (g.portfolio_idx[s:s + n], g.portfolio_len[s:s + n]))


@pytest.mark.parametrize("L", [1, 2])
def test_served_ledger_and_held_queries(L):
    g = _graph(L, prices=True)
    d = g.data
    tgn, ref = _seeded(g, L)
    _same(_ledger(tgn), ref, "seed")
    assert (ref[1][1:N_USERS + 1] > 0).sum() > 60 and np.isneginf(ref[2][N_USERS + 1:]).all(), "only sources get a row"
    mv = P.MVSampler(g.prices, g.upper_u, DEV, day_of=g.day_of)
    n_checks = 0
    for t, s in enumerate(range(CUT, 1500, TICK)):
        sb, db, tb, fb, pb = _tick(g, s)
        # (the L = 1 run walks every tick in batches of 7, the L = 2 run as one batch: the ledger is the reference's either way)
        n, _ = tgn.ingest(sb, db, tb, fb, batch_size=7 if L == 1 else None, portfolios=pb)
        assert n == TICK
        HR.store(*ref, sb, *pb, tb)
        if t % 3 != 2:
            continue
        n_checks += 1
        _same(_ledger(tgn), ref, "tick %d" % t)
        users = np.concatenate([np.unique(sb)[:9], [int(sb[-1]), int(sb[-1])], [int(np.flatnonzero(ref[1][1:N_USERS + 1] == 0)[0]) + 1]])
        now = float(tb[-1]) + 1.0
        lists = HR.held_node_lists(ref[0], ref[1], users, g.upper_u)
        assert sum(len(r) for r in lists) > 10 and lists[-1] == []
        held = tgn.recommend(users, now, 5, ITEMS, exclude="held")
        want = tgn.recommend(users, now, 5, ITEMS, exclude=lists)
        plain = tgn.recommend(users, now, 5, ITEMS)
        assert len(held) == 3 and all(torch.equal(a, b) for a, b in zip(held, want)), "exclude='held', tick %d" % t
        assert not torch.equal(held[0], plain[0]), "the exclusion must move something, or the test shows nothing"
        ids = held[0].cpu().numpy()
        assert all(not (set(ids[q].tolist()) & set(lists[q])) for q in range(len(users)))
        rows = (ref[0][users], ref[1][users])
        for kw_held, kw_ref in ((dict(portfolios="held"), dict(portfolios=rows)),
                                (dict(portfolios="held", exclude="held"), dict(portfolios=rows, exclude=lists)),
                                (dict(portfolios="held", exclude=lists), dict(portfolios=rows, exclude=lists))):
            a = tgn.recommend(users, now, 5, ITEMS, mv=mv, **kw_held)
            b = tgn.recommend(users, now, 5, ITEMS, mv=mv, **kw_ref)
            assert len(a) == 4 and all(torch.equal(x, y) for x, y in zip(a, b)), "%s, tick %d" % (sorted(kw_held), t)
        # users at two different times: the ledger's rows follow them through the block sort
        ts = np.where(np.arange(len(users)) % 2 == 0, now, now + 5.0)
        a = tgn.recommend(users, ts, 5, ITEMS, mv=mv, portfolios="held", exclude="held")
        b = tgn.recommend(users, ts, 5, ITEMS, mv=mv, portfolios=rows, exclude=lists)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), "two timestamps, tick %d" % t
        a = tgn.recommend(users, ts, 5, ITEMS, exclude="held")
        b = tgn.recommend(users, ts, 5, ITEMS, exclude=lists)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        r_idx, r_len = _host(*tgn.holdings.rows(users))
        assert HR.same_bits(r_idx, rows[0]) and HR.same_bits(r_len, rows[1])
    assert n_checks == 8
    # an ingest without portfolios, an observe and an expire leave the ledger's bits
    before = _ledger(tgn)
    sb, db, tb, fb, _ = _tick(g, 1400)
    tgn.ingest(sb, db, tb + 1e9, fb)
    dropped, _ = tgn.expire(float(d.timestamps[600]))
    assert dropped > 0
    _same(_ledger(tgn), before, "ingest without portfolios / expire")
    _same(before, ref, "end")


def test_new_users_rows_start_at_the_initial_values():
    g = _graph(1)
    tgn, ref = _seeded(g, 1)
    n0 = tgn.n_nodes                                             # 151: the next ids are nodes nobody has seen
    rs = np.random.RandomState(8)
    t0 = float(g.data.timestamps[-1]) + 1.0
    # node n0 arrives as a destination (no row is written for it), n0 + 1 as a source with a portfolio
    src = np.array([5, n0 + 1, 7, 5], np.int64)
    dst = np.array([130, 131, n0, 132], np.int64)
    ports = [[3, 4], [9, 1, 2], [], [6]]
    n, _ = tgn.ingest(src, dst, t0 + np.arange(4), rs.randn(4, 4), portfolios=ports)
    assert n == 4 and tgn.n_nodes == n0 + 2 == tgn.holdings.n_nodes and tgn.holdings.capacity == tgn.node_capacity
    got = _ledger(tgn)
    grown = HR.new_tables(n0 + 2, WIDTH)
    for a, b in zip(grown, ref):
        a[:n0] = b
    idx = np.full((4, 3), -1, np.int32)
    for e, r in enumerate(ports):
        idx[e, :len(r)] = r
    HR.store(*grown, src, idx, [len(r) for r in ports], t0 + np.arange(4))
    _same(got, grown, "tick with new nodes")
    assert got[1][n0] == 0 and np.isneginf(got[2][n0]) and (got[0][n0] == -1).all(), "a new node is at the initial values until written"
    assert got[0][n0 + 1, :3].tolist() == [9, 1, 2] and got[1][5] == 1 and got[2][5] == t0 + 3
    untouched = np.setdiff1d(np.arange(n0), [5, 7])
    assert all(HR.same_bits(a[untouched], b[untouched]) for a, b in zip(got, ref)), "the old rows keep every bit"
    # the next tick writes it; an explicit add_nodes grows the ledger the same way
    tgn.ingest(np.array([n0], np.int64), np.array([133], np.int64), np.array([t0 + 10]), rs.randn(1, 4), portfolios=[[11]])
    HR.store(*grown, [n0], [[11]], [1], [t0 + 10])
    first = tgn.add_nodes(40)
    assert first == n0 + 2 and tgn.holdings.n_nodes == n0 + 42
    got = _ledger(tgn)
    _same(tuple(a[:n0 + 2] for a in got), grown, "after add_nodes")
    assert (got[0][n0 + 2:] == -1).all() and not got[1][n0 + 2:].any() and np.isneginf(got[2][n0 + 2:]).all()


def test_batch_size_and_device_inputs_leave_the_same_ledger():
    g = _graph(1)
    d = g.data
    sb, db, tb, fb, pb = _tick(g, CUT, 48)
    ledgers = []
    for route in ("batch_7", "one_batch", "device", "lists"):
        tgn, ref = _seeded(g, 1)
        if route == "device":
            to = lambda a, dt: _dev(np.ascontiguousarray(a, dtype=dt))
            n, _ = tgn.ingest(to(sb, np.int32), to(db, np.int32), to(tb, np.float64), to(fb, np.float32),
                              portfolios=(to(pb[0], np.int32), to(pb[1], np.int32)))
        elif route == "lists":
            n, _ = tgn.ingest(sb, db, tb, fb, portfolios=[list(r[:k]) for r, k in zip(*pb)])
        else:
            n, _ = tgn.ingest(sb, db, tb, fb, batch_size=7 if route == "batch_7" else None, portfolios=pb)
        assert n == 48
        ledgers.append(_ledger(tgn))
    HR.store(*ref, sb, *pb, tb)
    for route, got in zip(("batch_7", "one_batch", "device", "lists"), ledgers):
        _same(got, ref, route)
    # a saved ledger loads through the one writer, host or device
    tgn, _ = _seeded(g, 1)
    for on_dev in (False, True):
        fresh = _model(g, 1)
        fresh.track_holdings(WIDTH, g.upper_u)
        nodes = np.arange(fresh.n_nodes)
        if on_dev:
            h = tgn.holdings
            fresh.update_holdings(_dev(nodes.astype(np.int32)), (h.idx, h.len), h.time)
        else:
            idx, ln, tm = _ledger(tgn)
            fresh.update_holdings(nodes, (idx, ln), tm)
        _same(_ledger(fresh), _ledger(tgn), "load, device=%s" % on_dev)
    # device inputs are not validated on the host: the kernel skips and clamps by the reference's rules
    want = _ledger(tgn)
    src = np.array([0, -3, tgn.n_nodes, 4, 4], np.int32)
    idx = np.arange(50, dtype=np.int32).reshape(5, 10)
    ln = np.array([3, 3, 3, 2, 12], np.int32)
    tm = np.arange(5, dtype=np.float64)
    tgn.update_holdings(_dev(src), (_dev(idx), _dev(ln)), _dev(tm))
    HR.store(*want, src, idx, ln, tm)
    _same(_ledger(tgn), want, "unchecked device inputs")
    assert want[0][4].tolist() == list(range(40, 48)) and want[1][4] == 8
    # the ledger moves with the model
    tgn.to("cpu")
    assert tgn.holdings.idx.device.type == "cpu" and all(HR.same_bits(a.numpy(), b) for a, b in zip(
        (tgn.holdings.idx, tgn.holdings.len, tgn.holdings.time), want))
