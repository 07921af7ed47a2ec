"""GPU tests of the retention window: ``NeighborFinder.expire`` / ``TGN.expire`` and the kernels behind them
against the numpy restatement ``tests/expire_ref.py``.  "Bitwise" throughout: expiry and compaction move values, they compute
none; the served model after an expiry and the model built from the filtered log run the same kernels on the same bits.  The
one numeric bar is the training step's, the README's for gradients (5e-4 in the max norm; loss 1e-4)."""

import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

import pfotgnrec_amd as P
from pfotgnrec_amd import _lib
from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
from parity import relerr
import observe_ref as O
import expire_ref as R

DEV = "cuda:0"
N_USERS, N_ITEMS, K_NBR, BATCH, N_EDGES = 120, 30, 5, 24, 1500
RTOL_GRAD = 5e-4                                               # README, parity bars: parameter gradients, max norm

# Widths of the two-launch scan (csrc/scan64.hpp): XS_WAVE = 64 lanes (the shuffle scan inside a wavefront), XS_TILE = 1024
# values per workgroup, and XS_TILE * (XS_TILE + 1) = 1,049,600 values = 1025 tiles, the most for which every lane of the
# offset pass adds at most ONE earlier tile total (tile 1025 is the first whose lane 0 adds two).  One below, at and one above
# each; 3100 needs four tiles; 1.
SCAN_COUNTS = [1, 63, 64, 65, 1023, 1024, 1025, 3100, 1024 * 1025 - 1, 1024 * 1025, 1024 * 1025 + 1]


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _host(t):
    return t.detach().cpu().numpy()


def _dev_csr(nf):
    torch.cuda.synchronize()
    return tuple(_host(a) for a in nf.device_arrays(DEV))


def _assert_csr(got, want, tag):
    for a, b, name in zip(got, want, ("indptr", "nbr", "eidx", "ts")):
        assert _bits(a, b), "%s: %s differs" % (tag, name)


# ---------------------------------------------------------------------------------------------- hand-made adjacencies
def _make_csr(n_nodes, n_entries, seed, n_edge_rows=400):
    """Rows of a time-sorted CSR with many timestamp ties (40 distinct values), made directly: with three nodes or more, row 0
    and a third of the others are empty, one row holds a single entry, one holds more than half of all entries; the first and
    the last row of a large table hold entries (the offsets of the last tiles are read)."""
    rs = np.random.RandomState(seed)
    counts = np.zeros(n_nodes, np.int64)
    if n_nodes < 3:
        counts[:] = n_entries // n_nodes
    else:
        hub, single = n_nodes // 2, n_nodes - 1
        counts[hub] = n_entries // 2 + 7
        counts[single] = 1
        rest = n_entries - counts.sum()
        others = np.setdiff1d(np.arange(1, n_nodes - 1), [hub])
        if len(others):
            live = others[rs.rand(len(others)) > 1.0 / 3.0]
            live = live if len(live) else others[:1]
            live = np.union1d(live, others[-1:])                  # (a populated row near the end, behind the hub)
            np.add.at(counts, rs.choice(live, size=rest), 1)
    indptr = np.zeros(n_nodes + 1, np.int64)
    np.cumsum(counts, out=indptr[1:])
    total = int(indptr[-1])
    owner = R.row_of(indptr)
    ts = rs.randint(0, 40, size=total).astype(np.float64) * 0.5 + 10.0
    ts = ts[np.lexsort((ts, owner))]                              # sorted inside every row
    nbr = rs.randint(0, n_nodes, size=total).astype(np.int32)
    eidx = rs.randint(1, n_edge_rows, size=total).astype(np.int32)
    return indptr, nbr, eidx, ts


def _finder(csr):
    return P.NeighborFinder(_csr=tuple(a.copy() for a in csr))


def _cutoffs(csr):
    indptr, _, _, ts = csr
    hub = int(np.argmax(np.diff(indptr)))
    row = ts[indptr[hub]:indptr[hub + 1]]
    vals, cnt = np.unique(row, return_counts=True)
    tie = float(vals[cnt > 1][len(vals[cnt > 1]) // 2]) if (cnt > 1).any() else float(vals[0])
    return {"below_all": float(ts.min()) - 1.0, "above_all": float(ts.max()) + 1.0, "tie": tie, "mid": 20.25}


_CSR_300 = []


def _csr_300():
    if not _CSR_300:
        _CSR_300.append(_make_csr(300, 4000, 1))
    return _CSR_300[0]


# ---------------------------------------------------------------------------------------------- 1. kernel parity, bitwise
@pytest.mark.parametrize("kind", ["below_all", "above_all", "tie", "mid"])
def test_expire_equals_mask_and_cumsum_bit_for_bit(kind):
    csr = _csr_300()
    counts = np.diff(csr[0])
    assert (counts == 0).sum() > 20 and (counts == 1).any() and counts.max() > counts.sum() // 2
    cutoff = _cutoffs(csr)[kind]
    want, keep = R.expire_csr(*csr, cutoff)
    nf = _finder(csr)
    before = nf.device_arrays(DEV)
    assert nf._max_nbr is not None and nf._max_eidx is not None
    dropped = nf.expire(cutoff, DEV)
    got = _dev_csr(nf)
    assert dropped == int((~keep).sum())
    _assert_csr(got, want, kind)
    assert nf.n_nodes == 300
    if kind == "below_all":
        assert dropped == 0 and nf._version == 0 and nf.device_arrays(DEV) is before and nf._max_eidx is not None
    else:
        assert dropped > 0 and nf._version == 1 and nf._max_nbr is None and nf._max_eidx is None
        _assert_csr((nf.indptr, nf.nbr, nf.eidx, nf.ts), want, kind + " (host mirrors refetched)")
        assert nf.max_edge_idx() == int(want[2].max(initial=0)) and nf.max_neighbor_id() == int(want[1].max(initial=0))
    if kind == "above_all":
        assert int(got[0][-1]) == 0 and not got[0].any() and got[1].size == 0
    if kind == "tie":
        hub = int(np.argmax(counts))
        old_row, new_row = csr[3][csr[0][hub]:csr[0][hub + 1]], got[3][got[0][hub]:got[0][hub + 1]]
        assert (old_row == cutoff).sum() > 1 and (new_row == cutoff).sum() == (old_row == cutoff).sum(), "strict <: the tie group stays"
        assert new_row[0] == cutoff and 0 < len(new_row) < len(old_row)
    print("FIGURES expire %s: cutoff %.3f, %d of %d entries dropped, arrays bitwise equal" % (kind, cutoff, dropped, len(keep)))
    # a second expiry at the same cutoff finds nothing to drop
    version = nf._version
    assert nf.expire(cutoff, DEV) == 0 and nf._version == version


# ---------------------------------------------------------------------------------------------- 2. scan boundaries
@pytest.mark.parametrize("n_nodes", SCAN_COUNTS)
def test_node_counts_around_the_scan_widths(n_nodes):
    csr = _make_csr(n_nodes, 3000, 100 + n_nodes % 97)
    nf = _finder(csr)
    for cutoff in (20.25, 29.5):                                   # the second runs on the first's output
        want, keep = R.expire_csr(*csr, cutoff)
        assert 0 < keep.sum() < len(keep)
        assert nf.expire(cutoff, DEV) == int((~keep).sum())
        _assert_csr(_dev_csr(nf), want, "n_nodes=%d cutoff=%g" % (n_nodes, cutoff))
        csr = want


def _plan_and_compact(n_rows, Ef, eidx, ts, cutoff, cap):
    """The four table-side entry points on raw tensors -> (table [cap, Ef], remap, n_keep, rewritten eidx) on the host."""
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    rs = np.random.RandomState(n_rows % 1000)
    table = np.zeros((cap, Ef), np.float32)
    table[:n_rows] = rs.randn(n_rows, Ef).astype(np.float32)
    d_table, d_eidx, d_ts = to(table), to(eidx), to(ts)
    flags = torch.zeros(n_rows, dtype=torch.int32, device=DEV)
    half = len(eidx) // 2                                         # two calls: two finders marking one flag table
    for lo, hi in ((0, half), (half, len(eidx))):
        _lib.call("pfo_edge_rows_mark", d_eidx[lo:hi].data_ptr() if hi > lo else None, d_ts[lo:hi].data_ptr() if hi > lo else None,
                  hi - lo, cutoff, n_rows, flags.data_ptr(), _lib.stream_ptr())
    nbytes = _lib.byte_count("pfo_edge_rows_plan_scratch_bytes", n_rows)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    remap = torch.full((n_rows,), -7, dtype=torch.int32, device=DEV)
    n_keep_dev = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    _lib.call("pfo_edge_rows_plan", flags.data_ptr(), n_rows, remap.data_ptr(), n_keep_dev.data_ptr(), scratch.data_ptr(), nbytes,
              _lib.stream_ptr())
    n_keep = int(n_keep_dev.item())
    assert 1 <= n_keep <= n_rows
    tmp = torch.empty((n_keep, Ef), dtype=torch.float32, device=DEV)
    _lib.call("pfo_edge_rows_compact", d_table.data_ptr(), n_rows, n_keep, Ef, remap.data_ptr(), tmp.data_ptr(), _lib.stream_ptr())
    live = d_ts >= cutoff                                        # the surviving entries are the ones that get rewritten
    d_live = d_eidx[live].contiguous()
    _lib.call("pfo_eidx_remap", d_live.data_ptr() if d_live.numel() else None, d_live.numel(), remap.data_ptr(), n_rows,
              _lib.stream_ptr())
    torch.cuda.synchronize()
    return table, _host(d_table), _host(remap), n_keep, _host(d_live)


@pytest.mark.parametrize("n_rows", SCAN_COUNTS)
def test_edge_row_counts_around_the_scan_widths(n_rows):
    rs = np.random.RandomState(7 + n_rows % 89)
    n_entries = max(40, min(3 * n_rows, 30000))
    eidx = rs.randint(1, n_rows, size=n_entries).astype(np.int32) if n_rows > 1 else np.zeros(n_entries, np.int32)
    if n_rows > 2:
        eidx[:2] = (1, n_rows - 1)                                # the first and the last real row are named
    ts = rs.randint(0, 40, size=n_entries).astype(np.float64) * 0.5 + 10.0
    if n_rows > 2:
        ts[:2] = (10.0, 10.0) if n_rows % 2 else (10.0, 29.5)     # ... and expire (odd counts: both; even: the first only)
    cutoff, Ef, cap = 22.0, 4, n_rows + 3
    want_remap, want_keep = R.release_rule(n_rows, [(eidx, ts)], cutoff)
    before, table, remap, n_keep, live = _plan_and_compact(n_rows, Ef, eidx, ts, cutoff, cap)
    assert n_keep == want_keep and _bits(remap, want_remap) and remap[0] == 0
    assert _bits(table, R.compact_table(before[:n_rows], want_remap, capacity=cap)), "kept rows in order, zero rows behind them"
    assert _bits(live, want_remap[eidx[ts >= cutoff]]) and (live >= 0).all()
    if n_rows > 64:
        assert n_keep < n_rows and (want_remap[1:] >= 0).sum() > 0
    print("FIGURES row scan n_rows=%d: %d rows released of %d, remap / table / ids bitwise equal" % (n_rows, n_rows - n_keep, n_rows))


# ---------------------------------------------------------------------------------------------- the served model
_GRAPHS = {}


def _graph(L):
    if L not in _GRAPHS:
        torch.manual_seed(5 + L)
        _GRAPHS[L] = make_graph(SyntheticConfig("t", N_USERS, N_ITEMS, N_EDGES, 16, L, K_NBR, 2), with_prices=False)
    return _GRAPHS[L]


def _model(g, L, nf, edge_features, dropout=0.0):
    return P.TGN(nf, g.node_features, edge_features, DEV, n_layers=L, n_heads=2, dropout=dropout, use_memory=True,
                 memory_dimension=16, message_function="identity", n_neighbors=K_NBR)


def _finder_of(g, sel, uniform=False, eidx=None, ts=None, seed=3):
    d = g.data
    return P.NeighborFinder.from_arrays(d.sources[sel], d.destinations[sel], d.edge_idxs[sel] if eidx is None else eidx,
                                        d.timestamps[sel] if ts is None else ts, uniform=uniform,
                                        max_node_idx=g.node_features.shape[0] - 1, seed=seed)


def _host_csr(nf):
    return tuple(np.array(a) for a in (nf.indptr, nf.nbr, nf.eidx, nf.ts))


def _state(tgn):
    m = tgn.memory
    torch.cuda.synchronize()
    return tuple(_host(t).copy() for t in (m.memory, m.last_update, m.msg_table, m.msg_time, m.has_msg, tgn.flat_parameters)) + (tgn._step,)


def _same_state(a, b):
    return all(_bits(x, y) for x, y in zip(a[:-1], b[:-1])) and a[-1] == b[-1]


def _warm_up(g, tgn, upto, steps=3):
    d = g.data
    rs = np.random.RandomState(3)
    tgn.eval()
    for s in range(upto - steps * BATCH, upto, BATCH):
        neg = rs.randint(N_USERS + 1, N_USERS + N_ITEMS + 1, size=BATCH)
        with torch.no_grad():
            tgn.compute_temporal_embeddings(d.sources[s:s + BATCH], d.destinations[s:s + BATCH], neg, d.timestamps[s:s + BATCH],
                                            d.edge_idxs[s:s + BATCH], K_NBR)


def _cutoff_of(g, frac=0.8):
    ts = g.data.timestamps
    c = float(ts[int(frac * len(ts))])
    return c if c > ts[0] else float(ts[len(ts) // 2])


# ---------------------------------------------------------------------------------------------- 3. compaction, bitwise
def _two_finder_world():
    """One table, two finders: the FULL finder holds every edge except every seventh (rows named by nobody); the TRAIN finder
    holds the full finder's edges except every third, and names 25 of the earliest edges' rows at LATE times - rows that expire
    in the full finder and survive in the other."""
    g = _graph(1)
    d = g.data
    idx = np.arange(N_EDGES)
    full_sel = idx[idx % 7 != 3]
    train_sel = full_sel[full_sel % 3 != 1]
    late = train_sel[:25]
    train_ts = d.timestamps[train_sel].copy()
    train_ts[:25] = d.timestamps[-1] + 1.0 + np.arange(25)
    nf_full, nf_train = _finder_of(g, full_sel), _finder_of(g, train_sel, ts=train_ts)
    tgn = _model(g, 1, nf_full, g.edge_features)
    return g, tgn, nf_full, nf_train, d.edge_idxs[late], d.edge_idxs[idx[idx % 7 == 3]]


def test_compaction_over_two_finders_bit_for_bit():
    g, tgn, nf_full, nf_train, late_rows, unnamed_rows = _two_finder_world()
    cutoff = _cutoff_of(g, 0.6)
    n_rows = N_EDGES + 1
    assert tgn.edge_raw_features.shape[0] == n_rows
    tgn.reserve(n_edges=n_rows + 50)                              # capacity beyond the live rows: it must survive, zeroed
    csrs = [_host_csr(nf_full), _host_csr(nf_train)]
    table = _host(tgn.edge_raw_features).copy()
    want_csr, want_remap, want_keep, want_dropped = R.expire_all(n_rows, csrs, cutoff)
    alone, _ = R.release_rule(n_rows, [(csrs[0][2], csrs[0][3])], cutoff)
    assert (alone[late_rows] == -1).all() and (want_remap[late_rows] >= 0).all(), "expired in one finder, surviving in the other: stays"
    assert (want_remap[unnamed_rows] >= 0).all() and len(unnamed_rows) > 100, "rows nobody names stay"
    assert 1 < want_keep < n_rows - 100
    store_ptr, cap, tv = tgn._edges.storage[0].data_ptr(), tgn.edge_capacity, tgn._tables_version
    tgn._adj_cache, tgn._last_ws, tgn._last_call = ("x",), ("y",), ("z",)
    dropped, remap = tgn.expire(cutoff, finders=[nf_train])
    torch.cuda.synchronize()
    assert dropped == want_dropped and remap.device.type == "cuda" and remap.dtype == torch.int32
    assert _bits(_host(remap), want_remap) and int(remap[0]) == 0
    assert tgn.edge_raw_features.shape[0] == want_keep == tgn._cfg.n_edges_p1
    assert tgn._edges.storage[0].data_ptr() == store_ptr == tgn.edge_raw_features.data_ptr() and tgn.edge_capacity == cap
    assert _bits(_host(tgn._edges.storage[0]), R.compact_table(table, want_remap, capacity=cap)), "table: kept rows, zero rows behind"
    for nf, want, tag in ((nf_full, want_csr[0], "full"), (nf_train, want_csr[1], "train")):
        _assert_csr(_dev_csr(nf), want, tag)
        assert nf._version == 2 and nf._max_eidx is None and nf.max_edge_idx() < want_keep
    assert tgn._tables_version == tv + 1 and tgn._adj_cache is None and tgn._last_ws is None and tgn._last_call is None
    # the next rows continue from the new count, behind zero rows
    new = tgn.add_edge_features(np.random.RandomState(1).randn(3, g.edge_features.shape[1]))
    assert np.array_equal(new, np.arange(want_keep, want_keep + 3)) and tgn._cfg.n_edges_p1 == want_keep + 3
    print("FIGURES compaction, two finders: %d entries dropped, %d of %d rows released (%d kept only by the other finder, %d named "
          "by nobody), bitwise equal" % (dropped, n_rows - want_keep, n_rows, len(late_rows), len(unnamed_rows)))


def test_without_compaction_the_table_and_the_ids_stay():
    g, tgn, nf_full, nf_train, _, _ = _two_finder_world()
    cutoff = _cutoff_of(g, 0.6)
    csr = _host_csr(nf_full)
    train_before = _host_csr(nf_train)
    table, tv = _host(tgn._edges.storage[0]).copy(), tgn._tables_version
    want, keep = R.expire_csr(*csr, cutoff)
    dropped, remap = tgn.expire(cutoff, compact_edges=False)
    assert remap is None and dropped == int((~keep).sum()) > 0
    _assert_csr(_dev_csr(nf_full), want, "ids untouched")
    assert _bits(_host(tgn._edges.storage[0]), table) and tgn._tables_version == tv and tgn._cfg.n_edges_p1 == N_EDGES + 1
    _assert_csr(_dev_csr(nf_train), train_before, "a finder that does not take part")
    assert nf_train._version == 0 and nf_full._version == 1
    # a cutoff below everything: nothing at all happens, whatever compact_edges says
    assert tgn.expire(float(csr[3].min()) - 5.0) == (0, None) and nf_full._version == 1 and tgn._tables_version == tv
    # compaction afterwards, alone: every row the earlier expiry orphaned is 'named by nobody' now and stays
    dropped2, remap2 = tgn.expire(cutoff)
    assert dropped2 == 0 and remap2 is None


# ---------------------------------------------------------------------------------------------- 4. end to end
def _pair_after_expire(L, uniform, dropout=0.0):
    """A: served over the whole log, warmed up, expired.  B: built from the filtered log with remapped ids, its table the
    reference's gathered rows, parameters / memory / messages / step counter A's.  Returns what the tests compare."""
    g = _graph(L)
    d = g.data
    torch.manual_seed(11 + L)
    A = _model(g, L, _finder_of(g, slice(None), uniform), g.edge_features, dropout)
    _warm_up(g, A, N_EDGES)
    cutoff = _cutoff_of(g)
    csr = _host_csr(A.neighbor_finder)
    table = _host(A.edge_raw_features).copy()
    n_rows = N_EDGES + 1
    (want_csr,), remap, n_keep, want_dropped = R.expire_all(n_rows, [csr], cutoff)
    m = d.timestamps >= cutoff
    nf_b = _finder_of(g, m, uniform, eidx=remap[d.edge_idxs[m]])
    _assert_csr(_host_csr(nf_b), want_csr, "the filtered log's adjacency is the reference's")
    B = _model(g, L, nf_b, g.edge_features[:n_keep], dropout)
    with torch.no_grad():
        B.edge_raw_features.copy_(torch.from_numpy(R.compact_table(table, remap)[:n_keep]))
        sd_a, sd_b = A.state_dict(), B.state_dict()
        for k, v in sd_b.items():
            if not k.startswith("memory."):
                v.copy_(sd_a[k])
    B.parameters_changed()
    assert torch.equal(A.flat_parameters, B.flat_parameters)
    B.memory.restore_memory(A.memory.backup_memory())
    B._step = A._step
    B._set_stats(*A.edge_feature_stats)
    return g, A, B, cutoff, remap, n_keep, want_dropped


def _query(g, tgn):
    d = g.data
    users = np.unique(d.sources[-40:])
    items = np.arange(N_USERS + 1, N_USERS + N_ITEMS + 1)
    out = tgn.recommend(users, float(d.timestamps[-1]) + 1.0, 5, items, return_embeddings=True)
    torch.cuda.synchronize()
    return tuple(_host(x).copy() for x in out)


@pytest.mark.parametrize("uniform", [False, True], ids=["recent", "uniform"])
@pytest.mark.parametrize("L", [1, 2])
def test_served_model_after_expire_is_the_model_of_the_filtered_log(L, uniform):
    g, A, B, cutoff, want_remap, n_keep, want_dropped = _pair_after_expire(L, uniform)
    state = _state(A)
    before, want = _query(g, A), _query(g, B)
    moved = relerr(np.concatenate([before[3], before[4]]), np.concatenate([want[3], want[4]]))
    assert moved > 1e-3, "before the expiry the two models must differ, or the test shows nothing"
    assert _same_state(_state(A), state), "recommend writes nothing"
    dropped, remap = A.expire(cutoff)
    assert dropped == want_dropped > 0 and _bits(_host(remap), want_remap) and A.edge_raw_features.shape[0] == n_keep
    assert _same_state(_state(A), state), "memory, last_update, messages, parameters and the step counter keep every bit"
    assert _bits(_host(A.edge_raw_features), _host(B.edge_raw_features))
    got = _query(g, A)
    names = ("item ids", "scores", "n_valid", "user embeddings", "item embeddings", "user block")
    for x, y, name in zip(got, want, names):
        assert _bits(x, y), "%s differ after the expiry" % name
    print("FIGURES end to end L=%d %s: relerr before the expiry %.3g, after it 0 (embeddings and top-k bitwise equal); %d entries "
          "dropped, %d of %d rows kept" % (L, "uniform" if uniform else "most recent", moved, dropped, n_keep, N_EDGES + 1))


# ---------------------------------------------------------------------------------------------- 5. life goes on
@pytest.mark.parametrize("L", [1, 2])
def test_ingest_and_training_continue_after_an_expiry(L):
    g, A, B, cutoff, _, n_keep, _ = _pair_after_expire(L, False)
    d = g.data
    A.expire(cutoff)
    rs = np.random.RandomState(8)
    sb, db = d.sources[-BATCH:], d.destinations[-BATCH:]
    tb = d.timestamps[-1] + 1.0 + np.arange(BATCH, dtype=np.float64)
    raw = rs.randn(BATCH, g.edge_features.shape[1])
    ids = []
    for t in (A, B):
        n, idxs = t.ingest(sb, db, tb, raw)
        assert n == BATCH
        ids.append(idxs)
    assert np.array_equal(ids[0], np.arange(n_keep, n_keep + BATCH)), "the tick's rows start at the new row count"
    assert np.array_equal(ids[0], ids[1]) and A._cfg.n_edges_p1 == n_keep + BATCH
    assert _bits(_host(A.edge_raw_features), _host(B.edge_raw_features))
    _assert_csr(_dev_csr(A.neighbor_finder), _dev_csr(B.neighbor_finder), "adjacency after the tick")
    O.check_tables(_state(A)[:5], _state(B)[:5], "after the tick")
    print("FIGURES life goes on L=%d: state after the tick bitwise equal: %s" % (L, _same_state(_state(A), _state(B))))
    to = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(DEV)
    neg = rs.randint(N_USERS + 1, N_USERS + N_ITEMS + 1, size=BATCH * 3)
    out = []
    for t in (A, B):
        t.deterministic = True
        t.train()
        emb, b = t.embed_device(to(sb, np.int32), to(db, np.int32), [to(neg, np.int32)], [3], to(tb + 1.0, np.float64),
                                to(ids[0], np.int32), K_NBR)
        loss = P.bpr_step(t, emb, b, 3)
        t.join()
        torch.cuda.synchronize()
        out.append((float(loss), _host(t.flat_grad).copy()))
    (la, ga), (lb, gb) = out
    e = relerr(ga, gb)
    print("FIGURES life goes on L=%d: loss %.7g vs %.7g, gradient relerr %.3g (bitwise equal: %s)" % (L, la, lb, e, _bits(ga, gb)))
    assert abs(la - lb) < O.RTOL * max(1.0, abs(lb))
    assert np.isfinite(ga).all() and np.abs(gb).max() > 0 and e < RTOL_GRAD
    O.check_tables(_state(A)[:5], _state(B)[:5], "after the step")


def test_a_step_captured_before_the_expiry_is_refused():
    from pfotgnrec_amd.rand_edge_sampler import item_availability, DeviceNegativeSampler
    g = _graph(1)
    d = g.data
    torch.manual_seed(4)
    tgn = _model(g, 1, _finder_of(g, slice(None)), g.edge_features)
    opt = P.FusedAdam(tgn, lr=1e-3)
    sampler = DeviceNegativeSampler(item_availability(d.destinations, g.upper_u, N_ITEMS), g.upper_u, DEV, seed=1)
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)
    s = N_EDGES - BATCH
    batch = (to(d.sources[s:], np.int32), to(d.destinations[s:], np.int32), to(d.timestamps[s:], np.float64), to(d.edge_idxs[s:], np.int32),
             to(g.portfolio_idx[s:], np.int32), to(g.portfolio_len[s:], np.int32), None)
    gs = P.GraphedTrainStep(tgn, opt, sampler, BATCH, K_NBR, n_neg=3, port_width=g.portfolio_idx.shape[1])
    gs.capture(*batch, warmup=1)
    assert np.isfinite(float(gs(*batch)))
    assert tgn.expire(float(d.timestamps[0]) - 1.0) == (0, None)
    assert np.isfinite(float(gs(*batch))), "a cutoff below everything changes nothing: the captured step is still good"
    dropped, remap = tgn.expire(_cutoff_of(g))
    assert dropped > 0 and remap is not None
    with pytest.raises(RuntimeError, match="stale"):
        gs(*batch)
    gs.finish()
