"""CPU side of the holdings ledger: the numpy reference's own properties, the three new symbols and their argument
checks, every host-side refusal of ``track_holdings`` / ``update_holdings`` / ``ingest(portfolios=)`` / ``recommend("held")`` -
a rejected call leaves the ledger and the model bit for bit - and the capacity scheme on CPU tensors.  No kernel runs here."""
import os
import re

import numpy as np
import pytest
import torch

import holdings_ref as HR
from conftest import REPO

SYMBOLS = ("pfo_holdings_store", "pfo_holdings_store_scratch_bytes", "pfo_holdings_gather")
W, UPPER_U = 4, 50                                             # the host model below: 50 users, 10 items


# ---------------------------------------------------------------------------------------------- 1. the reference's own rules
def test_reference_last_wins_and_empty_overwrites():
    idx, ln, tm = HR.new_tables(6, 3)
    HR.store(idx, ln, tm, [2, 3, 2, 3], [[1, 2, 3], [4, 5, -1], [7, -1, -1], [9, 9, 9]], [3, 2, 1, 0], [1.0, 2.0, 3.0, 4.0])
    assert idx[2].tolist() == [7, -1, -1] and ln[2] == 1 and tm[2] == 3.0, "the LAST event of the call wins"
    assert idx[3].tolist() == [-1, -1, -1] and ln[3] == 0 and tm[3] == 4.0, "an empty portfolio overwrites a non-empty one"
    assert idx[1].tolist() == [-1, -1, -1] and ln[1] == 0 and tm[1] == -np.inf, "a row never written holds the initial values"
    HR.store(idx, ln, tm, [2], [[5, 6, 7]], [2], [0.5])         # no comparison with the stored time
    assert idx[2].tolist() == [5, 6, -1] and tm[2] == 0.5


def test_reference_clamps_lengths_and_skips_ids():
    idx, ln, tm = HR.new_tables(5, 2)
    before = (idx.copy(), ln.copy(), tm.copy())
    HR.store(idx, ln, tm, [0, -5, 5, 2 ** 31 - 1], np.arange(12).reshape(4, 3), [3, 3, 3, 3], [1.0] * 4)
    assert all(HR.same_bits(a, b) for a, b in zip((idx, ln, tm), before)), "ids outside [1, n_nodes) are skipped"
    HR.store(idx, ln, tm, [4, 3, 2], [[7, 8, 9], [-3, 2 ** 31 - 1, 0], [1, 2, 3]], [5, 2, -4], [1.0, 2.0, 3.0])
    assert idx[4].tolist() == [7, 8] and ln[4] == 2, "clamped to the ledger's width"
    assert idx[3].tolist() == [-3, 2 ** 31 - 1] and ln[3] == 2, "entries are stored verbatim"
    assert idx[2].tolist() == [-1, -1] and ln[2] == 0 and tm[2] == 3.0, "a negative length is an empty row"
    idx, ln, tm = HR.new_tables(5, 4)
    HR.store(idx, ln, tm, [1], [[6, 7]], [4], [1.0])
    assert idx[1].tolist() == [6, 7, -1, -1] and ln[1] == 2, "clamped to the input's stride"


def test_reference_gather():
    idx, ln, tm = HR.new_tables(25, 3)
    HR.store(idx, ln, tm, [2, 3], [[0, 4, 9], [1, -1, 2 ** 31 - 1]], [3, 3], [1.0, 2.0])
    ln[2] = 2                                                   # (raw tables: an entry behind len that names a candidate)
    items = [15, 11, 12, 20]                                    # upper_u = 10: stocks 4, 0, 1, 9
    pi, pl, ex = HR.gather(idx, ln, [2, 3, 7, -1, 25, 2], items, 10)
    assert pi[0].tolist() == [0, 4, 9] and pl[0] == 2 and ex[0].tolist() == [1, 0, -1], "entries behind len are not excluded"
    assert pi[1].tolist() == [1, -1, 2 ** 31 - 1] and ex[1].tolist() == [2, -1, -1], "-1 and a stock far outside map to -1"
    assert pi[2].tolist() == [-1] * 3 and pl[2] == 0 and ex[2].tolist() == [-1] * 3, "an unwritten user"
    for q in (3, 4):
        assert pi[q].tolist() == [-1] * 3 and pl[q] == 0 and ex[q].tolist() == [-1] * 3, "an out-of-range user"
    assert HR.same_bits(pi[5], pi[0]) and HR.same_bits(ex[5], ex[0])
    assert HR.gather(idx, ln, [2], None)[2] is None
    assert HR.held_node_lists(idx, ln, [2, 7, 99], 10) == [[11, 15], [], []]


# ---------------------------------------------------------------------------------------------- 2. the symbols
def test_symbols_in_header_library_and_prototypes():
    from pfotgnrec_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "pfotgn.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name) and name in _lib.PROTOTYPES, name
    assert lib.pfo_abi_version() == 6
    import pfotgnrec_amd as P
    for name in ("track_holdings", "update_holdings"):
        assert hasattr(P.TGN, name)
    assert hasattr(P, "holdings_store") and hasattr(P, "holdings_gather")


def _store(N=1, n_nodes=10, W=4, stride=4, scratch_bytes=1 << 20):
    from pfotgnrec_amd import _lib
    return _lib.call("pfo_holdings_store", None, None, None, stride, None, N, None, None, None, n_nodes, W, None, scratch_bytes, None)


def _gather(U=1, n_nodes=10, W=4, I=3):
    from pfotgnrec_amd import _lib
    return _lib.call("pfo_holdings_gather", None, U, None, None, n_nodes, W, None, I, 5, None, None, None, None, None)


def test_limits_are_refused_before_anything_is_dereferenced():
    """Every pointer is NULL: a limit that was checked behind a read would crash instead of refusing."""
    from pfotgnrec_amd import _lib
    for call in (_store, _gather):
        for w in (0, -1, 257):
            with pytest.raises(_lib.PfoError, match=r"W must lie in \[1, 256\]"):
                call(W=w)
        for n in (0, -3, 2 ** 31):
            with pytest.raises(_lib.PfoError, match="n_nodes"):
                call(n_nodes=n)
    for N in (-1, 2 ** 31):
        with pytest.raises(_lib.PfoError, match="N must lie"):
            _store(N=N)
    for I in (0, -1, _lib.RECOMMEND_MAX_ITEMS + 1):
        with pytest.raises(_lib.PfoError, match="I must lie"):
            _gather(I=I)
    with pytest.raises(_lib.PfoError, match="null pointer"):
        _store()
    with pytest.raises(_lib.PfoError, match="null pointer"):
        _gather()
    _store(N=0)                                                 # nothing is queued, nothing is looked at
    _gather(U=0)
    _store(N=0, W=256)
    _gather(U=0, I=_lib.RECOMMEND_MAX_ITEMS)
    lib = _lib.load()
    assert lib.pfo_holdings_store_scratch_bytes(300, 5000) == 1200
    assert lib.pfo_holdings_store_scratch_bytes(0, 1) == -1 and lib.pfo_holdings_store_scratch_bytes(5, -1) == -1
    assert lib.pfo_holdings_store_scratch_bytes(5, 2 ** 31) == -1


# ---------------------------------------------------------------------------------------------- 3. the Python surface on a host model
def _host_model(track=True):
    import pfotgnrec_amd as P
    from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
    g = make_graph(SyntheticConfig("t", 50, 10, 400, 8, 1, 4, 2), with_prices=False)
    nf = P.get_neighbor_finder(g.data, False)
    tgn = P.TGN(nf, g.node_features, g.edge_features, "cpu", n_layers=1, n_heads=2, use_memory=True, memory_dimension=8,
                message_function="identity")
    if track:
        tgn.track_holdings(W, UPPER_U)
        rs = np.random.RandomState(4)                           # non-trivial content, so that "kept bit for bit" says something
        h = tgn.holdings
        with torch.no_grad():
            h.idx.copy_(torch.from_numpy(rs.randint(-1, 10, size=tuple(h.idx.shape)).astype(np.int32)))
            h.len.copy_(torch.from_numpy(rs.randint(0, W + 1, size=tgn.n_nodes).astype(np.int32)))
            h.time.copy_(torch.from_numpy(rs.rand(tgn.n_nodes)))
    return tgn, g


def _snapshot(tgn):
    """The ledger, the edge table, n_nodes and the memory tables: row counts, addresses and every bit."""
    m, h = tgn.memory, tgn.holdings
    tabs = [tgn.node_raw_features, tgn.edge_raw_features, m.memory.data, m.last_update.data, m.msg_table, m.msg_time, m.has_msg]
    if h is not None:
        tabs += [h.idx, h.len, h.time]
    return (tgn.n_nodes, tgn._cfg.n_nodes, tgn._cfg.n_edges_p1, tgn.neighbor_finder.n_nodes, tgn.neighbor_finder._version,
            None if h is None else (h.n_nodes, h.capacity, h.width, h.upper_u),
            tuple((tuple(t.shape), t.data_ptr(), t.numpy().tobytes()) for t in tabs))


def test_track_holdings_once():
    tgn, _ = _host_model(track=False)
    assert tgn.holdings is None
    for bad in ((0, 5), (257, 5), (4, -1), ("x", 5)):
        with pytest.raises(ValueError):
            tgn.track_holdings(*bad)
    assert tgn.holdings is None
    h = tgn.track_holdings(W, UPPER_U)
    assert h is tgn.holdings and (h.width, h.upper_u, h.n_nodes, h.capacity) == (W, UPPER_U, tgn.n_nodes, tgn.node_capacity)
    assert h.idx.dtype == torch.int32 and tuple(h.idx.shape) == (tgn.n_nodes, W) and bool((h.idx == -1).all())
    assert h.len.dtype == torch.int32 and tuple(h.len.shape) == (tgn.n_nodes,) and not h.len.any()
    assert h.time.dtype == torch.float64 and bool(torch.isneginf(h.time).all())
    assert tgn.track_holdings(W, UPPER_U) is h                  # the same arguments again: the ledger that is there
    for other in ((W + 1, UPPER_U), (W, UPPER_U + 1)):
        with pytest.raises(ValueError, match="already tracks"):
            tgn.track_holdings(*other)
    assert not any("holdings" in k for k in tgn.state_dict()), "not part of the checkpoint"


def _event_args(g, n=6):
    d = g.data
    return dict(sources=d.sources[:n].copy(), portfolios=(g.portfolio_idx[:n, :W].copy(), np.minimum(g.portfolio_len[:n], W)),
                edge_times=d.timestamps[:n].copy())


BAD_WRITES = ["length_sources", "length_times", "length_len", "float_idx", "float_len", "float_sources", "idx_beyond_int32",
              "list_beyond_int32", "len_negative", "len_beyond_stride", "row_longer_than_width", "list_longer_than_width",
              "node_beyond_table", "node_negative", "list_of_strings", "list_count", "device_pair_with_host_sources"]


def _spoil(kw, case, n_nodes):
    idx, ln = kw["portfolios"]
    if case == "length_sources":
        kw["sources"] = kw["sources"][:5]
    elif case == "length_times":
        kw["edge_times"] = kw["edge_times"][:5]
    elif case == "length_len":
        kw["portfolios"] = (idx, ln[:5])
    elif case == "float_idx":
        kw["portfolios"] = (idx.astype(np.float32), ln)
    elif case == "float_len":
        kw["portfolios"] = (idx, ln.astype(np.float64))
    elif case == "float_sources":
        kw["sources"] = kw["sources"].astype(np.float64)
    elif case == "idx_beyond_int32":
        big = idx.astype(np.int64)
        big[2, 0] = 2 ** 31
        kw["portfolios"] = (big, ln)
    elif case == "list_beyond_int32":
        kw["portfolios"] = [[1], [2], [-2 ** 31 - 1], [], [], []]
    elif case == "len_negative":
        kw["portfolios"] = (idx, np.where(np.arange(6) == 1, -1, ln))
    elif case == "len_beyond_stride":
        kw["portfolios"] = (idx[:, :2], np.full(6, 3, np.int32))
    elif case == "row_longer_than_width":
        kw["portfolios"] = (np.zeros((6, W + 2), np.int32), np.where(np.arange(6) == 4, W + 1, 1))
    elif case == "list_longer_than_width":
        kw["portfolios"] = [[1]] * 5 + [list(range(W + 1))]
    elif case == "node_beyond_table":
        kw["sources"][3] = n_nodes
    elif case == "node_negative":
        kw["sources"][3] = -1
    elif case == "list_of_strings":
        kw["portfolios"] = [["000001"], [], [], [], [], []]
    elif case == "list_count":
        kw["portfolios"] = [[1]] * 5
    elif case == "device_pair_with_host_sources":
        kw["portfolios"] = (torch.from_numpy(idx), torch.from_numpy(ln.astype(np.int32)))
    return kw


@pytest.mark.parametrize("case", BAD_WRITES)
def test_rejected_update_holdings_leaves_everything(case):
    tgn, g = _host_model()
    kw = _spoil(_event_args(g), case, tgn.n_nodes)
    before = _snapshot(tgn)
    with pytest.raises(ValueError):
        tgn.update_holdings(**kw)
    assert _snapshot(tgn) == before


@pytest.mark.parametrize("case", BAD_WRITES + ["ingest_decreasing_times", "ingest_feature_width"])
def test_rejected_ingest_leaves_everything(case):
    """The ledger's checks join ingest's own, and all of them run before the first write - also when the call would add nodes."""
    tgn, g = _host_model()
    d = g.data
    kw = _event_args(g)
    kw.update(destinations=d.destinations[:6].copy(), edge_times=d.timestamps[-1] + 1.0 + np.arange(6),
              edge_features=np.random.RandomState(1).randn(6, 4))
    kw["destinations"][2] = tgn.n_nodes                          # a new node: validated against the table as it WILL be
    if case == "ingest_decreasing_times":
        kw["edge_times"] = kw["edge_times"][::-1].copy()
    elif case == "ingest_feature_width":
        kw["edge_features"] = np.zeros((6, 5))
    elif case == "node_beyond_table":
        kw["sources"][3] = tgn.n_nodes + 2                       # (n_nodes itself is the node this tick adds; + 1 would be the next)
    else:
        kw = _spoil(kw, case, tgn.n_nodes)
    before = _snapshot(tgn)
    with pytest.raises(ValueError):
        tgn.ingest(**kw)
    assert _snapshot(tgn) == before


def test_valid_writes_reach_the_device_check_and_change_nothing_on_a_host_model():
    """A host model has no kernel to run: valid arguments pass every check and are refused where the device is asked for -
    before the first table grows."""
    from pfotgnrec_amd import _lib
    tgn, g = _host_model()
    kw = _event_args(g)
    before = _snapshot(tgn)
    for ports in (kw["portfolios"], [list(r[:n]) for r, n in zip(*kw["portfolios"])], (kw["portfolios"][0].astype(np.int64), kw["portfolios"][1])):
        with pytest.raises(_lib.PfoError):
            tgn.update_holdings(kw["sources"], ports, kw["edge_times"])
    d = g.data
    dst = d.destinations[:6].copy()
    dst[2] = tgn.n_nodes
    with pytest.raises(_lib.PfoError):
        tgn.ingest(kw["sources"], dst, d.timestamps[-1] + 1.0 + np.arange(6), np.zeros((6, 4)), portfolios=kw["portfolios"])
    assert _snapshot(tgn) == before
    assert tgn.update_holdings(kw["sources"][:0], (kw["portfolios"][0][:0], kw["portfolios"][1][:0]), kw["edge_times"][:0]) == 0
    assert tgn.update_holdings([], [], []) == 0
    assert _snapshot(tgn) == before


def test_without_a_ledger():
    tgn, g = _host_model(track=False)
    kw = _event_args(g)
    before = _snapshot(tgn)
    with pytest.raises(ValueError, match="track_holdings"):
        tgn.update_holdings(**kw)
    d = g.data
    with pytest.raises(ValueError, match="track_holdings"):
        tgn.ingest(kw["sources"], d.destinations[:6], d.timestamps[-1] + 1.0 + np.arange(6), np.zeros((6, 4)), portfolios=kw["portfolios"])
    items = np.arange(51, 61)
    with pytest.raises(ValueError, match="track_holdings"):
        tgn.recommend(np.arange(1, 4), 5.0, 3, items, exclude="held")

    class MV:
        returns, upper_u, gamma, lambda_mv = np.zeros((2, 10, 5)), UPPER_U, 1.0, 0.5
        day_of = staticmethod(lambda ts: np.zeros(len(ts), np.int64))
    with pytest.raises(ValueError, match="track_holdings"):
        tgn.recommend(np.arange(1, 4), 5.0, 3, items, mv=MV, portfolios="held")
    assert _snapshot(tgn) == before
    # with a ledger: "held" portfolios still need mv, and mv must number the stocks like the ledger
    tgn.track_holdings(W, UPPER_U)
    with pytest.raises(ValueError, match="need mv"):
        tgn.recommend(np.arange(1, 4), 5.0, 3, items, portfolios="held")
    MV.upper_u = UPPER_U + 1
    with pytest.raises(ValueError, match="upper_u"):
        tgn.recommend(np.arange(1, 4), 5.0, 3, items, mv=MV, portfolios="held")
    from pfotgnrec_amd import recommend as R
    MV.upper_u = UPPER_U
    q = R.validate(tgn.n_nodes, 4, np.arange(1, 4), 5.0, 3, items, "held", None, None, MV, "held", None, tgn.holdings)
    assert q.held == (True, True) and q.ex_ids is None and q.mv.port_idx is None
    q = R.validate(tgn.n_nodes, 4, np.arange(1, 4), 5.0, 3, items, [[51], [], []], None, None, MV, "held", None, tgn.holdings)
    assert q.held == (False, True) and q.ex_ids is not None
    q = R.validate(tgn.n_nodes, 4, np.arange(1, 4), 5.0, 3, items, None, None, None)
    assert q.held is None, "any other argument value: the query is the one it was"


# ---------------------------------------------------------------------------------------------- 4. growth and moves
def _ledger(tgn):
    h = tgn.holdings
    return [t.numpy().copy() for t in (h.idx, h.len, h.time)]


def _initial(stores, lo):
    return bool((stores[0][lo:] == -1).all()) and not stores[1][lo:].any() and bool(torch.isneginf(stores[2][lo:]).all())


def test_reserve_and_add_nodes_grow_the_ledger():
    tgn, _ = _host_model()
    h, n = tgn.holdings, tgn.n_nodes
    before = _ledger(tgn)
    assert h.capacity == tgn.node_capacity == n
    tgn.reserve(n_nodes=n + 7)
    assert h.capacity == tgn.node_capacity == n + 7 and h.n_nodes == n
    assert all(HR.same_bits(a, b) for a, b in zip(_ledger(tgn), before)), "live rows are copied bit for bit"
    assert _initial(h._store.storage, n), "rows behind the live count hold the initial values"
    for view, store in zip((h.idx, h.len, h.time), h._store.storage):
        assert view.data_ptr() == store.data_ptr() and view.is_contiguous() and view.shape[0] == n
    ptr = h.idx.data_ptr()
    assert tgn.add_nodes(3) == n                                # within capacity: nothing moves
    assert h.n_nodes == tgn.n_nodes == n + 3 and h.idx.data_ptr() == ptr and h.capacity == n + 7
    assert tuple(h.idx.shape) == (n + 3, W) and tuple(h.len.shape) == (n + 3,) and tuple(h.time.shape) == (n + 3,)
    now = _ledger(tgn)
    assert all(HR.same_bits(a[:n], b) for a, b in zip(now, before))
    assert _initial([h.idx, h.len, h.time], n), "new rows are at the initial values"
    assert tgn.add_nodes(20) == n + 3                           # across it: reallocated with the node tables
    assert h.n_nodes == tgn.n_nodes == n + 23 and h.capacity == tgn.node_capacity >= n + 23 and h.idx.data_ptr() != ptr
    assert all(HR.same_bits(a[:n], b) for a, b in zip(_ledger(tgn), before))
    assert _initial(h._store.storage, n)
    assert h._stamp.shape[0] == h._pos.shape[0] == h.capacity, "the scratch tables follow the capacity"
    with pytest.raises(ValueError, match="shrink"):
        h.resize(n)


def test_device_move_and_cast_carry_the_ledger():
    tgn, _ = _host_model()
    tgn.reserve(n_nodes=tgn.n_nodes + 4)
    before, cap = _ledger(tgn), tgn.holdings.capacity
    tgn.to("cpu")
    tgn.float()                                                 # a cast of the model's floating tensors leaves the fp64 times alone
    h = tgn.holdings
    assert h.capacity == cap and h.time.dtype == torch.float64 and h.idx.dtype == torch.int32
    assert all(HR.same_bits(a, b) for a, b in zip(_ledger(tgn), before))
    assert h.idx.data_ptr() == h._store.storage[0].data_ptr()
