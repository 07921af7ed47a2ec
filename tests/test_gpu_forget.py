"""GPU tests of erasure by node: ``NeighborFinder.forget`` / ``TGN.forget`` and the kernels behind them against the
numpy restatement ``tests/forget_ref.py``.  "Bitwise" throughout: a removal moves values and writes constants, it computes
none - integers and copied bits are compared exactly, and the served model after a removal runs the same kernels on the same
bits as an isolated node does."""
import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

import pfotgnrec_amd as P
from pfotgnrec_amd import _lib
from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
import expire_ref as X
import forget_ref as R

DEV = "cuda:0"
N_EDGE_ROWS = 400


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _host(t):
    return t.detach().cpu().numpy()


def _to(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _dev_csr(nf):
    torch.cuda.synchronize()
    return tuple(_host(a) for a in nf.device_arrays(DEV))


def _assert_csr(got, want, tag):
    for a, b, name in zip(got, want, ("indptr", "nbr", "eidx", "ts")):
        assert _bits(a, b), "%s: %s differs" % (tag, name)


# ---------------------------------------------------------------------------------------------- hand-made adjacencies
def _make_csr(n_nodes, n_entries, seed):
    """Rows of a time-sorted CSR with many timestamp ties, made directly (no symmetry: the kernels ask for none).  With three
    nodes or more: row 0 and a third of the others are empty, one hub row holds half of all entries, one leaf row a single entry,
    the last row is populated.  Some neighbour ids lie outside the table (they count as not gone), some edge indices outside the
    edge table (they are ignored by the flags)."""
    rs = np.random.RandomState(seed)
    counts = np.zeros(n_nodes, np.int64)
    if n_nodes < 3:
        counts[:] = [n_entries // 3, n_entries - n_entries // 3][:n_nodes]
    elif n_entries:
        hub, leaf = n_nodes // 2, n_nodes - 1
        counts[hub] = n_entries // 2
        counts[leaf] = 1
        others = np.setdiff1d(np.arange(1, n_nodes - 1), [hub])
        live = others[rs.rand(len(others)) > 1.0 / 3.0]
        live = np.union1d(live if len(live) else others[:1], others[-1:])
        np.add.at(counts, rs.choice(live, size=n_entries - int(counts.sum())), 1)
    indptr = np.zeros(n_nodes + 1, np.int64)
    np.cumsum(counts, out=indptr[1:])
    total = int(indptr[-1])
    owner = X.row_of(indptr)
    ts = rs.randint(0, 40, size=total).astype(np.float64) * 0.5 + 10.0
    ts = ts[np.lexsort((ts, owner))]
    nbr = rs.randint(0, n_nodes, size=total).astype(np.int32)
    nbr[1::23] = 0                                                 # (node 0 is named: it goes only when a flag says so)
    nbr[3::17] = n_nodes + 3
    nbr[5::29] = -1
    eidx = rs.randint(1, N_EDGE_ROWS, size=total).astype(np.int32)
    eidx[7::31] = N_EDGE_ROWS + 2
    eidx[11::37] = -5
    return indptr, nbr, eidx, ts


SHAPES = {"two nodes": (2, 9), "65 nodes": (65, 300), "hub of 3000": (2500, 6000), "no entries": (65, 0),
          "1023 entries": (65, 1023), "1024 entries": (65, 1024), "1025 entries": (65, 1025)}
_CSRS = {}


def _csr(shape):
    if shape not in _CSRS:
        _CSRS[shape] = _make_csr(*SHAPES[shape], seed=list(SHAPES).index(shape) + 1)
    return _CSRS[shape]


def _ids(pattern, csr):
    indptr, nbr = csr[0], csr[1]
    n = len(indptr) - 1
    counts = np.diff(indptr)
    hub = max(1, int(np.argmax(counts[1:])) + 1) if n > 1 else 1
    small = np.flatnonzero((counts > 0) & (np.arange(n) != hub) & (np.arange(n) > 0))
    leaf = int(small[np.argmin(counts[small])]) if len(small) else hub
    rs = np.random.RandomState(n)
    if pattern == "none":
        return []
    if pattern == "all":
        return list(range(1, n))
    if pattern == "hub":
        return [hub]
    if pattern == "leaf":
        return [leaf]
    if pattern == "tenth":
        return sorted(rs.choice(np.arange(1, n), size=max(1, n // 10), replace=False).tolist())
    assert pattern == "dirty"
    return [leaf, leaf, 0, n, n + 7, -4, 2 ** 31 - 1, hub if n < 3 else 1 + (leaf % (n - 1)), 0, leaf]


def _finder(csr):
    return P.NeighborFinder(_csr=tuple(a.copy() for a in csr))


# ---------------------------------------------------------------------------------------------- 1. kernel parity, bitwise
@pytest.mark.parametrize("pattern", ["none", "all", "hub", "leaf", "tenth", "dirty"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_forget_equals_mask_and_cumsum_bit_for_bit(shape, pattern):
    csr = _csr(shape)
    n, total = len(csr[0]) - 1, len(csr[1])
    if shape == "hub of 3000":
        counts = np.diff(csr[0])
        assert n > 2 * 1024 and total > 5 * 1024 and counts.max() >= 3000 and (counts == 0).sum() > 500 and (counts == 1).any()
    ids = _ids(pattern, csr)
    gone = R.gone_of(n, ids)
    want, keep = R.forget_csr(*csr, gone)
    want_flags = R.row_flags(N_EDGE_ROWS, [csr[:3]], gone)
    nf = _finder(csr)
    before = nf.device_arrays(DEV)
    flags = torch.zeros(N_EDGE_ROWS, dtype=torch.int32, device=DEV)
    dropped = nf.forget(ids, DEV, _row_flags=flags)
    got = _dev_csr(nf)
    assert dropped == int((~keep).sum())
    _assert_csr(got, want, "%s / %s" % (shape, pattern))
    assert _bits(_host(flags), want_flags), "pfo_edge_rows_mark_nodes"
    assert nf.n_nodes == n
    if pattern == "none" or total == 0:
        assert dropped == 0
    if dropped == 0:
        assert nf._version == 0 and nf.device_arrays(DEV) is before and nf._max_eidx is not None and nf._host is not None
    else:
        assert nf._version == 1 and nf._max_nbr is None and nf._max_eidx is None
        _assert_csr((nf.indptr, nf.nbr, nf.eidx, nf.ts), want, "host mirrors refetched")
        assert nf.max_edge_idx() == int(want[2].max(initial=0)) and nf.max_neighbor_id() == int(want[1].max(initial=0))
    if pattern in ("hub", "leaf", "tenth") and shape == "hub of 3000":
        assert 0 < dropped < total, "some entries go and some stay, or the case shows nothing"
    print("FIGURES forget %s / %s: %d of %d entries dropped, arrays and flags bitwise equal" % (shape, pattern, dropped, total))
    version = nf._version                                          # a second removal of the same nodes finds nothing to drop
    assert nf.forget(ids, DEV) == 0 and nf._version == version


def test_ids_on_the_device_and_flags_give_the_same_arrays():
    csr = _csr("hub of 3000")
    n = len(csr[0]) - 1
    ids = _ids("dirty", csr) + _ids("tenth", csr)
    gone = R.gone_of(n, ids)
    want, keep = R.forget_csr(*csr, gone)
    for form in (torch.tensor(ids, dtype=torch.int64, device=DEV), torch.tensor(ids, dtype=torch.int32), _to(gone)):
        nf = _finder(csr)
        assert nf.forget(form, DEV) == int((~keep).sum()) > 0
        _assert_csr(_dev_csr(nf), want, str(form.dtype))
    literal = gone.copy()
    literal[0] = 1                                                 # flags are taken as they are: row 0 goes when its flag says so
    want0, keep0 = R.forget_csr(*csr, literal)
    nf = _finder(csr)
    assert nf.forget(_to(literal), DEV) == int((~keep0).sum()) > int((~keep).sum())
    _assert_csr(_dev_csr(nf), want0, "flag of node 0")


@pytest.mark.parametrize("shape", ["hub of 3000", "1025 entries", "no entries"])
def test_plan_copy_and_flag_on_raw_tensors(shape):
    """The entry points themselves, outputs filled with sentinels first: what is not written shows."""
    indptr, nbr, eidx, ts = _csr(shape)
    n, total = len(indptr) - 1, len(nbr)
    ids = np.array(_ids("dirty", (indptr, nbr)) + _ids("tenth", (indptr, nbr)), np.int32)
    want_gone = R.gone_of(n, ids)
    d_gone, d_ids = torch.full((n + 4,), 0xAA, dtype=torch.uint8, device=DEV), _to(ids)
    _lib.call("pfo_nodes_flag", d_ids.data_ptr(), len(ids), n, d_gone.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert _bits(_host(d_gone[:n]), want_gone) and (_host(d_gone[n:]) == 0xAA).all(), "pfo_nodes_flag"
    want, keep = R.forget_csr(indptr, nbr, eidx, ts, want_gone)
    d_ptr, d_nbr, d_eid, d_ts = (_to(a) for a in (indptr, nbr, eidx, ts))
    nbytes = _lib.byte_count("pfo_csr_forget_scratch_bytes", n, total)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    d_keep = torch.full((total + 3,), 7, dtype=torch.uint8, device=DEV)
    d_pos = torch.full((total + 4,), -7, dtype=torch.int64, device=DEV)
    d_new = torch.full((n + 4,), -7, dtype=torch.int64, device=DEV)
    p = lambda t: t.data_ptr() if t.numel() else None
    _lib.call("pfo_csr_forget_plan", d_ptr.data_ptr(), p(d_nbr), n, total, d_gone.data_ptr(), d_keep.data_ptr() if total else None,
              d_pos.data_ptr(), d_new.data_ptr(), scratch.data_ptr(), nbytes, _lib.stream_ptr())
    torch.cuda.synchronize()
    want_pos = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    assert _bits(_host(d_keep[:total]), keep.astype(np.uint8)) and (_host(d_keep[total:]) == 7).all()
    assert _bits(_host(d_pos[:total + 1]), want_pos) and (_host(d_pos[total + 1:]) == -7).all()
    assert _bits(_host(d_new[:n + 1]), want[0]) and (_host(d_new[n + 1:]) == -7).all()
    kept = int(want_pos[-1])
    o_nbr = torch.full((kept + 3,), -7, dtype=torch.int32, device=DEV)
    o_eid = torch.full((kept + 3,), -7, dtype=torch.int32, device=DEV)
    o_ts = torch.full((kept + 3,), -7.0, dtype=torch.float64, device=DEV)
    _lib.call("pfo_csr_forget_copy", p(d_nbr), p(d_eid), p(d_ts), total, p(d_keep[:total]), d_pos.data_ptr(), kept, o_nbr.data_ptr(),
              o_eid.data_ptr(), o_ts.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    for got, ref in ((o_nbr, want[1]), (o_eid, want[2]), (o_ts, want[3])):
        assert _bits(_host(got[:kept]), ref) and (_host(got[kept:]) == -7).all()
    print("FIGURES raw entry points %s: %d of %d entries kept; keep / new_pos / new_indptr / copies bitwise equal" % (shape, kept, total))


@pytest.mark.parametrize("n,D,M,Dn,W", [(131, 6, 19, 5, 3), (1, 1, 1, 1, 1), (700, 10, 31, 7, 9)])
def test_node_rows_reset_touches_flagged_rows_only(n, D, M, Dn, W):
    """Widths that are no multiple of 4 (rows start at any dword), rows around the 64 a wavefront reads at once, storage with rows
    behind the live ones: every table is filled with sentinels, only flagged rows may change."""
    rs = np.random.RandomState(n)
    cap = n + 2
    gone = (rs.rand(n) < 0.2).astype(np.uint8)
    gone[[0, n - 1]] = 1
    if n > 130:
        gone[[62, 63, 64, 65, 127, 128]] = (1, 1, 1, 0, 0, 1)
    host = [rs.randn(cap, D).astype(np.float32) + 3, rs.rand(cap).astype(np.float32) + 1, rs.randn(cap, M).astype(np.float32) + 3,
            rs.rand(cap).astype(np.float32) + 1, np.ones(cap, np.uint8), rs.randn(cap, Dn).astype(np.float32) + 3,
            rs.randint(0, 50, size=(cap, W)).astype(np.int32), rs.randint(1, W + 1, size=cap).astype(np.int32), rs.rand(cap) + 5.0]
    fills = [0, 0, 0, 0, 0, 0, -1, 0, -np.inf]
    want = R.reset_rows(host, fills, gone)
    assert all((w[n:] != f).all() for w, f in zip(want, fills)), "the rows behind the live ones hold sentinels"
    d_gone = _to(gone)

    def run(present):
        dev = [_to(a) for a in host]
        ptr = [t.data_ptr() if on else None for t, on in zip(dev, present)]
        _lib.call("pfo_node_rows_reset", d_gone.data_ptr(), n, ptr[0], D, ptr[1], ptr[2], M, ptr[3], ptr[4], ptr[5], Dn, ptr[6], W,
                  ptr[7], ptr[8], _lib.stream_ptr())
        torch.cuda.synchronize()
        return [_host(t) for t in dev]
    names = ("memory", "last_update", "msg_table", "msg_time", "has_msg", "node features", "holdings idx", "holdings len", "holdings time")
    for present in ([True] * 9, [True, False] * 4 + [True], [False, True] * 4 + [False], [False] * 9):
        for got, ref, before, on, name in zip(run(present), want, host, present, names):
            assert _bits(got, ref if on else before), "%s (tables given: %s)" % (name, present)
    print("FIGURES node rows n=%d D=%d M=%d Dn=%d W=%d: %d rows reset, every other bit kept" % (n, D, M, Dn, W, int(gone.sum())))


def test_refused_calls_queue_nothing():
    indptr, nbr, eidx, ts = _csr("65 nodes")
    n, total = len(indptr) - 1, len(nbr)
    d_ptr, d_nbr, d_eid, d_ts = (_to(a) for a in (indptr, nbr, eidx, ts))
    d_gone = _to(np.ones(n, np.uint8))
    outs = [torch.full((total + 1,), 7, dtype=dt, device=DEV) for dt in (torch.uint8, torch.int64, torch.int64, torch.int32)]
    keep, pos, new, flags = outs
    scratch = torch.full((64,), 7, dtype=torch.uint8, device=DEV)
    S, P_ = _lib.stream_ptr(), lambda t: t.data_ptr()
    refused = [
        ("pfo_nodes_flag", [P_(d_nbr), total, 0, P_(keep), S]),
        ("pfo_nodes_flag", [None, total, n, P_(keep), S]),
        ("pfo_csr_forget_plan", [P_(d_ptr), P_(d_nbr), n, total, P_(d_gone), P_(keep), P_(pos), P_(new), P_(scratch), 7, S]),
        ("pfo_csr_forget_plan", [P_(d_ptr), P_(d_nbr), n, total, None, P_(keep), P_(pos), P_(new), P_(scratch), 64, S]),
        ("pfo_csr_forget_plan", [P_(d_ptr), P_(d_nbr), 0, total, P_(d_gone), P_(keep), P_(pos), P_(new), P_(scratch), 64, S]),
        ("pfo_csr_forget_copy", [P_(d_nbr), P_(d_eid), P_(d_ts), total, P_(keep), P_(pos), total + 1, P_(flags), P_(flags), P_(new), S]),
        ("pfo_csr_forget_copy", [P_(d_nbr), P_(d_eid), None, total, P_(keep), P_(pos), 5, P_(flags), P_(flags), P_(new), S]),
        ("pfo_edge_rows_mark_nodes", [P_(d_ptr), P_(d_nbr), P_(d_eid), total, n, P_(d_gone), 0, P_(flags), S]),
        ("pfo_edge_rows_mark_nodes", [P_(d_ptr), P_(d_nbr), P_(d_eid), total, n, None, total, P_(flags), S]),
        ("pfo_node_rows_reset", [P_(d_gone), 0, P_(new), 2, None, None, 0, None, None, None, 0, None, 0, None, None, S]),
        ("pfo_node_rows_reset", [P_(d_gone), n, P_(new), 0, None, None, 0, None, None, None, 0, None, 0, None, None, S]),
        ("pfo_node_rows_reset", [None, n, P_(new), 2, None, None, 0, None, None, None, 0, None, 0, None, None, S]),
    ]
    for name, args in refused:
        assert getattr(_lib.load(), name)(*args) == -1, name               # PFO_ERR_INVALID
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in outs + [scratch]), "a refused call writes nothing"


# ---------------------------------------------------------------------------------------------- the served model
N_USERS, N_ITEMS, K_NBR, BATCH, N_EDGES, D_NODE = 120, 30, 5, 24, 1500, 16
ITEMS = np.arange(N_USERS + 1, N_USERS + N_ITEMS + 1)
ISO = N_USERS + N_ITEMS + 1                                         # one node more than the log names: no entry, zero features
_GRAPH = []


def _graph():
    if not _GRAPH:
        _GRAPH.append(make_graph(SyntheticConfig("t", N_USERS, N_ITEMS, N_EDGES, D_NODE, 1, K_NBR, 2), with_prices=False))
    return _GRAPH[0]


def _finder_of(g, sel, eidx=None):
    d = g.data
    return P.NeighborFinder.from_arrays(d.sources[sel], d.destinations[sel], d.edge_idxs[sel] if eidx is None else eidx, d.timestamps[sel],
                                        max_node_idx=ISO)


def _served(sel=slice(None), seed=7):
    """A model over the log with one isolated node behind it, a holdings ledger, and the state ``observe`` leaves."""
    g = _graph()
    d = g.data
    torch.manual_seed(seed)
    feats = np.vstack([g.node_features, np.zeros((1, D_NODE))])
    tgn = P.TGN(_finder_of(g, sel), feats, g.edge_features, DEV, n_layers=1, n_heads=2, dropout=0.0, use_memory=True,
                memory_dimension=D_NODE, message_function="identity", n_neighbors=K_NBR)
    tgn.eval()
    tgn.track_holdings(g.portfolio_idx.shape[1], g.upper_u)
    tgn.update_holdings(d.sources, (g.portfolio_idx, g.portfolio_len), d.timestamps)
    tgn.observe(d.sources, d.destinations, d.timestamps, d.edge_idxs, batch_size=BATCH)
    for p in tgn.parameters():                                      # (gradients that a removal must leave alone)
        if p.requires_grad:
            p.grad = torch.randn_like(p)
    return g, tgn


def _pick(g):
    """The user and the item to forget: a user of the last batch (a message is pending) and the item traded most."""
    d = g.data
    user = int(d.sources[-1])
    item = int(np.bincount(d.destinations).argmax())
    return user, item


NODE_FILLS = [0, 0, 0, 0, 0, 0, -1, 0, -np.inf]


def _node_tables(tgn):
    """Whole storage (the rows behind the live ones included) of the nine per-node tables."""
    torch.cuda.synchronize()
    return [_host(t).copy() for t in tgn.memory._store.storage + tgn._nodes.storage + tgn.holdings._store.storage]


def _untouchables(tgn):
    torch.cuda.synchronize()
    grads = np.concatenate([_host(p.grad).reshape(-1) for p in tgn.parameters() if p.requires_grad])
    return _host(tgn.flat_parameters).copy(), grads, tgn._step


def _now(g):
    return float(g.data.timestamps[-1]) + 1.0


def test_forget_a_user_and_an_item_end_to_end():
    g, tgn = _served()
    d = g.data
    user, item = _pick(g)
    nf, n_rows, now = tgn.neighbor_finder, N_EDGES + 1, _now(g)
    tgn.reserve(n_edges=n_rows + 40)                               # capacity beyond the live rows: it must survive, zeroed
    csr = tuple(np.array(a) for a in (nf.indptr, nf.nbr, nf.eidx, nf.ts))
    nodes_before, fixed_before = _node_tables(tgn), _untouchables(tgn)
    table = _host(tgn._edges.storage[0]).copy()
    m0 = tgn.memory
    assert bool(m0.has_msg[user]) and bool(m0.memory[user].abs().sum() > 0) and bool(m0.memory[item].abs().sum() > 0)
    assert int(tgn.holdings.len[user]) > 0 and nodes_before[5][user].any()
    fan = np.unique(d.sources[(d.destinations == item) & (d.sources != user)])[:8]     # users that traded the item
    assert len(fan) == 8
    seen0 = _host(tgn.recommend(fan, now, N_ITEMS, ITEMS, exclude="seen")[0])
    assert not (seen0 == item).any(), "before: the item is in every one of these users' histories and is not offered"
    emb0 = _host(tgn.recommend([user, ISO], now, 3, ITEMS, return_embeddings=True)[3])
    assert not _bits(emb0[0], emb0[1]), "before: the user is no isolated node"
    version, tv, sv = nf._version, tgn._tables_version, tgn.memory._state_version

    gone = R.gone_of(tgn.n_nodes, [user, item])
    (want_csr,), want_remap, want_keep, want_dropped = R.forget_all(n_rows, [csr], gone)
    dropped, remap = tgn.forget([user, item, user])
    torch.cuda.synchronize()
    assert dropped == want_dropped > 0 and remap.device.type == "cuda" and remap.dtype == torch.int32
    assert _bits(_host(remap), want_remap) and int(remap[0]) == 0 and 1 < want_keep < n_rows
    # the finder: the filtered log's, edge indices through remap
    m = ~(np.isin(d.sources, [user, item]) | np.isin(d.destinations, [user, item]))
    assert dropped == 2 * int((~m).sum())
    rebuilt = _finder_of(g, m, eidx=want_remap[d.edge_idxs[m]])
    _assert_csr(_dev_csr(nf), (rebuilt.indptr, rebuilt.nbr, rebuilt.eidx, rebuilt.ts), "rebuild over the filtered log")
    _assert_csr(_dev_csr(nf), want_csr, "reference")
    assert nf._version == version + 2 and nf.max_edge_idx() < want_keep
    # the edge table: kept rows in order, row 0 kept, zero rows behind the live count
    assert tgn.edge_raw_features.shape[0] == want_keep == tgn._cfg.n_edges_p1 and tgn._tables_version == tv + 1
    assert _bits(_host(tgn._edges.storage[0]), X.compact_table(table[:n_rows], want_remap, capacity=tgn.edge_capacity))
    assert _bits(_host(tgn.edge_raw_features[0]), table[0]) and not table[n_rows:].any()
    # the node rows: the two forgotten rows initial, every other row of every table bitwise unchanged
    cap_gone = np.zeros(nodes_before[0].shape[0], np.uint8)
    cap_gone[[user, item]] = 1
    names = ("memory", "last_update", "msg_table", "msg_time", "has_msg", "node features", "holdings idx", "holdings len", "holdings time")
    for got, ref, before, name in zip(_node_tables(tgn), R.reset_rows(nodes_before, NODE_FILLS, cap_gone), nodes_before, names):
        assert _bits(got, ref), name
        assert not _bits(got, before), name + ": the rows held something before, or the test shows nothing"
    assert tgn.memory._state_version == sv + 1 and tgn.memory._any_msg is True
    fixed = _untouchables(tgn)
    assert _bits(fixed[0], fixed_before[0]) and _bits(fixed[1], fixed_before[1]) and fixed[2] == fixed_before[2]
    # history / seen follow the finder
    everyone = np.arange(1, N_USERS + 1)
    nodes, lens = (_host(t) for t in tgn.history(everyone, now, 64)[:2])
    assert lens[user - 1] == 0 and not (nodes == item).any() and lens.sum() > 0
    seen1 = _host(tgn.recommend(fan, now, N_ITEMS, ITEMS, exclude="seen")[0])
    assert (seen1 == item).any(axis=1).all(), "after: the item is offered again"
    # the forgotten user embeds like an isolated node with a zero feature row, in the same call
    emb1 = _host(tgn.recommend([user, ISO], now, 3, ITEMS, return_embeddings=True)[3])
    assert _bits(emb1[0], emb1[1])
    # a forgotten id is reusable: a later ingest naming it leaves a finder equal to a rebuild
    rs = np.random.RandomState(2)
    other = [int(i) for i in ITEMS if i != item][:2]
    src2, dst2, ts2 = np.array([user, 5, user, 9]), np.array([item, other[0], other[1], item]), now + np.arange(4.0)
    n_in, new_idx = tgn.ingest(src2, dst2, ts2, rs.randn(4, g.edge_features.shape[1]))
    assert n_in == 4 and np.array_equal(new_idx, np.arange(want_keep, want_keep + 4))
    again = P.NeighborFinder.from_arrays(np.concatenate([d.sources[m], src2]), np.concatenate([d.destinations[m], dst2]),
                                         np.concatenate([want_remap[d.edge_idxs[m]], new_idx]), np.concatenate([d.timestamps[m], ts2]),
                                         max_node_idx=ISO)
    _assert_csr(_dev_csr(nf), (again.indptr, again.nbr, again.eidx, again.ts), "after the ingest")
    assert bool(tgn.memory.has_msg[user]) and int(_host(tgn.history([user], now + 10, 8)[1])[0]) == 2
    print("FIGURES end to end: %d entries dropped, %d of %d rows kept, finder / table / node rows bitwise equal to the references"
          % (dropped, want_keep, n_rows))


def _final(tgn):
    return _dev_csr(tgn.neighbor_finder), _host(tgn._edges.storage[0]).copy(), _node_tables(tgn)


def test_forget_and_expire_commute():
    g, A = _served()
    _, B = _served()
    user, item = _pick(g)
    cutoff = float(g.data.timestamps[N_EDGES // 2])
    a1, ra1 = A.forget([user, item])
    a2, ra2 = A.expire(cutoff)
    b1, rb1 = B.expire(cutoff)
    junk = torch.tensor([item, 0, 10 ** 6, user, -3, item], dtype=torch.int64, device=DEV)     # device ids: bad ones are skipped
    b2, rb2 = B.forget(junk)
    assert a1 > 0 and a2 > 0 and b1 > 0 and b2 > 0 and a1 + a2 == b1 + b2
    assert all(r is not None for r in (ra1, ra2, rb1, rb2))
    (csr_a, tab_a, nodes_a), (csr_b, tab_b, nodes_b) = _final(A), _final(B)
    _assert_csr(csr_a, csr_b, "forget then expire / expire then forget")
    assert _bits(tab_a, tab_b) and A.edge_raw_features.shape[0] == B.edge_raw_features.shape[0] < N_EDGES + 1
    assert all(_bits(x, y) for x, y in zip(nodes_a, nodes_b))
    ra, rb = _host(ra1), _host(rb1)                                 # the two maps, composed, agree on every row that survives
    via_a = np.where(ra >= 0, _host(ra2)[np.maximum(ra, 0)], -1)
    via_b = np.where(rb >= 0, _host(rb2)[np.maximum(rb, 0)], -1)
    assert np.array_equal(via_a, via_b)


def test_without_compaction_the_table_and_the_ids_stay():
    g, tgn = _served()
    user, item = _pick(g)
    nf = tgn.neighbor_finder
    csr = tuple(np.array(a) for a in (nf.indptr, nf.nbr, nf.eidx, nf.ts))
    table, tv, nodes_before = _host(tgn._edges.storage[0]).copy(), tgn._tables_version, _node_tables(tgn)
    gone = R.gone_of(tgn.n_nodes, [user, item])
    want, keep = R.forget_csr(*csr, gone)
    dropped, remap = tgn.forget(np.array([user, item]), compact_edges=False)
    assert remap is None and dropped == int((~keep).sum()) > 0
    _assert_csr(_dev_csr(nf), want, "ids untouched")
    assert _bits(_host(tgn._edges.storage[0]), table) and tgn._tables_version == tv and tgn._cfg.n_edges_p1 == N_EDGES + 1
    cap_gone = np.zeros(nodes_before[0].shape[0], np.uint8)
    cap_gone[[user, item]] = 1
    assert all(_bits(x, y) for x, y in zip(_node_tables(tgn), R.reset_rows(nodes_before, NODE_FILLS, cap_gone)))
    # a second call finds no entry; compaction afterwards, alone: the orphaned rows are 'named by nobody' now and stay
    assert tgn.forget([user, item]) == (0, None) and nf._version == 1 and tgn._tables_version == tv


def test_a_node_without_entries_is_reset_all_the_same():
    g, tgn = _served()
    with torch.no_grad():
        tgn.memory.memory[ISO] = 2.0
        tgn.memory.last_update[ISO] = 5.0
        tgn.node_raw_features[ISO] = 1.0
    tgn.update_holdings(np.array([ISO]), [[1, 2]], np.array([9.0]))
    nodes_before = _node_tables(tgn)
    nf, version = tgn.neighbor_finder, tgn.neighbor_finder._version
    arrays = nf.device_arrays(DEV)
    assert tgn.forget([ISO]) == (0, None)
    assert nf._version == version and nf.device_arrays(DEV) is arrays, "nothing dropped: the finder is not written"
    cap_gone = np.zeros(nodes_before[0].shape[0], np.uint8)
    cap_gone[ISO] = 1
    got, want = _node_tables(tgn), R.reset_rows(nodes_before, NODE_FILLS, cap_gone)
    assert all(_bits(x, y) for x, y in zip(got, want))
    assert sum(not _bits(x, y) for x, y in zip(got, nodes_before)) == 6, "memory, last update, features and the ledger's three"


def test_a_second_finder_is_swept_and_remapped_alike():
    g = _graph()
    d = g.data
    idx = np.arange(N_EDGES)
    full_sel = idx[idx % 7 != 3]                                    # (every seventh row is named by nobody)
    train_sel = full_sel[full_sel % 3 != 1]
    _, tgn = _served(full_sel)
    nf_full, nf_train = tgn.neighbor_finder, _finder_of(g, train_sel)
    user, item = _pick(g)
    n_rows = N_EDGES + 1
    csrs = [tuple(np.array(a) for a in (nf.indptr, nf.nbr, nf.eidx, nf.ts)) for nf in (nf_full, nf_train)]
    table = _host(tgn._edges.storage[0]).copy()
    gone = R.gone_of(tgn.n_nodes, [user, item])
    want_csr, want_remap, want_keep, want_dropped = R.forget_all(n_rows, csrs, gone)
    unnamed = d.edge_idxs[idx[idx % 7 == 3]]
    assert (want_remap[unnamed] >= 0).all() and len(unnamed) > 100, "rows nobody names stay"
    dropped, remap = tgn.forget([user, item], finders=[nf_train, nf_full])
    torch.cuda.synchronize()
    assert dropped == want_dropped and _bits(_host(remap), want_remap) and tgn.edge_raw_features.shape[0] == want_keep < n_rows
    assert _bits(_host(tgn._edges.storage[0]), X.compact_table(table[:n_rows], want_remap, capacity=tgn.edge_capacity))
    for nf, want, tag in ((nf_full, want_csr[0], "full"), (nf_train, want_csr[1], "train")):
        _assert_csr(_dev_csr(nf), want, tag)
        assert nf._version == 2 and nf.max_edge_idx() < want_keep
