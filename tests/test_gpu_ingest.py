"""GPU tests of ``TGN.ingest`` and what it is made of: ``pfo_edge_rows_append`` against numpy bit for bit, a model grown tick
by tick against the model built large, new nodes, the capacity scheme, and what an ingest must leave alone.  Bars are the
project's own: ``O.RTOL`` (1e-4 in the max norm) through ``O.check_tables`` / ``relerr``; "bitwise" where both sides run the
same arithmetic on the same inputs, or where the kernel is required to reproduce numpy's two fp32 operations."""

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

DEV = "cuda:0"
N_USERS, N_ITEMS, K_NBR, BATCH, CUT = 120, 30, 5, 24, 900


def _tables(tgn):
    m = tgn.memory
    torch.cuda.synchronize()
    return tuple(t.detach().cpu().numpy().copy() for t in (m.memory, m.last_update, m.msg_table, m.msg_time, m.has_msg))


def _set_params(tgn, params):
    sd = tgn.state_dict()
    with torch.no_grad():
        for k, v in params.items():
            if k in sd:
                sd[k].copy_(torch.from_numpy(np.asarray(v, np.float32)).reshape(sd[k].shape))
    tgn.parameters_changed()


def _params_of(tgn):
    return {k: v.detach().cpu().numpy() for k, v in tgn.state_dict().items() if not k.startswith("memory.")}


def _frozen(raw, stats):
    """numpy's normalisation of ``raw`` with GIVEN statistics: ``ef -= mean; ef /= std`` in fp32."""
    ef = np.asarray(raw).astype(np.float32)
    with np.errstate(all="ignore"):
        ef -= stats[0]
        ef /= stats[1]
    return ef


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _overwrite_edge_table(tgn, table):
    with torch.no_grad():
        tgn.edge_raw_features.copy_(torch.from_numpy(np.ascontiguousarray(table, dtype=np.float32)))


# ---------------------------------------------------------------------------------------------- 6. the kernel against numpy
@pytest.mark.parametrize("m,Ef,row0", [(1, 1, 1), (3, 5, 7), (300, 5, 3), (17, 172, 1)])
def test_kernel_is_numpy_bit_for_bit(m, Ef, row0):
    rs = np.random.RandomState(100 + m + Ef)
    raw = (rs.randn(m, Ef) * 3.0 + 0.5).astype(np.float32)
    mean = rs.randn(Ef).astype(np.float32)
    std = (0.25 + rs.rand(Ef)).astype(np.float32)
    c0 = Ef // 2
    std[c0] = 0.0                                                # a zero-variance column: +-inf, and NaN where raw == mean
    i1, c1 = m // 2, Ef - 1
    raw[i1, c1] = mean[c1]                                       # one raw value equals the mean (with Ef == 1: in column c0, 0/0)
    want = _frozen(raw, (mean, std))
    assert np.isnan(want).any() or np.isinf(want).any()
    assert Ef == 1 or want[i1, c1] == 0.0
    cap, sentinel = row0 + m + 3, np.float32(-12345.5)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    d_raw, d_mean, d_std = to(raw), to(mean), to(std)
    table = torch.full((cap, Ef), float(sentinel), dtype=torch.float32, device=DEV)

    def launch(n_rows, first, capacity):
        return _lib.load().pfo_edge_rows_append(d_raw.data_ptr(), d_mean.data_ptr(), d_std.data_ptr(), n_rows, Ef, table.data_ptr(),
                                                first, capacity, _lib.stream_ptr())
    # the rows do not fit: the error code, a message, and nothing written
    assert launch(m, row0, row0 + m - 1) != 0
    assert b"do not fit" in _lib.load().pfo_last_error()
    torch.cuda.synchronize()
    assert (table.cpu().numpy() == sentinel).all()
    assert launch(m, row0, cap) == 0
    torch.cuda.synchronize()
    got = table.cpu().numpy()
    assert (got[:row0] == sentinel).all() and (got[row0 + m:] == sentinel).all()
    new = got[row0:row0 + m]
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(new), nan), "NaN exactly where numpy has NaN"
    assert np.array_equal(new.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), "every other element bit for bit (inf included)"
    print("FIGURES edge_rows_append (m=%d, Ef=%d, row0=%d): %d elements bitwise equal, %d NaN, %d inf"
          % (m, Ef, row0, int((~nan).sum()), int(nan.sum()), int(np.isinf(want).sum())))


# ---------------------------------------------------------------------------------------------- the serving pair
def _graph(L):
    torch.manual_seed(5 + L)
    return make_graph(SyntheticConfig("t", N_USERS, N_ITEMS, 1500, 16, L, K_NBR, 2), with_prices=False)


def _model(g, L, n_edges, edge_features, use_memory=True, dropout=0.0):
    d = g.data
    nf = P.NeighborFinder.from_arrays(d.sources[:n_edges], d.destinations[:n_edges], d.edge_idxs[:n_edges], d.timestamps[:n_edges],
                                      uniform=False, max_node_idx=g.node_features.shape[0] - 1)
    return P.TGN(nf, g.node_features, edge_features, DEV, n_layers=L, n_heads=2, dropout=dropout, use_memory=use_memory,
                 memory_dimension=16, message_function="identity", n_neighbors=K_NBR)


def _serving_pair(L):
    """``_serving_pair`` of tests/test_gpu_observe.py, except that the served model has NEVER seen the rows behind the cut:
    it is built over the first CUT + 1 rows of the raw edge table (and normalises with THEIR statistics).  The full model is
    built over all rows; its table is then overwritten with the served model's frozen-statistics normalisation of all rows."""
    g = _graph(L)
    served = _model(g, L, CUT, g.edge_features[:CUT + 1])
    full = _model(g, L, CUT + BATCH, g.edge_features)
    _overwrite_edge_table(full, _frozen(g.edge_features, served.edge_feature_stats))
    _set_params(full, _params_of(served))
    return g, served, full


def _batch(d, s, n=BATCH):
    return d.sources[s:s + n], d.destinations[s:s + n], d.timestamps[s:s + n], d.edge_idxs[s:s + n]


def _warm_up(g, models, rs):
    for t in models:
        t.eval()
    for s in range(CUT - 3 * BATCH, CUT, BATCH):
        sb, db, tb, eb = _batch(g.data, s)
        neg = rs.randint(N_USERS + 1, N_USERS + N_ITEMS + 1, size=BATCH)
        with torch.no_grad():
            for t in models:
                t.compute_temporal_embeddings(sb, db, neg, tb, eb, K_NBR)


def _embeddings(out):
    return np.concatenate([out[3].cpu().numpy(), out[4].cpu().numpy()])


# ---------------------------------------------------------------------------------------------- 7. grown == built large
@pytest.mark.parametrize("L", [1, 2])
def test_grown_model_equals_the_model_built_large(L):
    g, served, full = _serving_pair(L)
    d = g.data
    rs = np.random.RandomState(3)
    assert served.edge_raw_features.shape[0] == CUT + 1 and full.edge_raw_features.shape[0] == 1501
    assert _same_bits(served.edge_raw_features.cpu().numpy(), full.edge_raw_features[:CUT + 1].cpu().numpy())
    _warm_up(g, (served, full), rs)
    sb, db, tb, eb = _batch(d, CUT)
    users = np.unique(np.concatenate([sb[:10], d.sources[CUT - BATCH:CUT][:10]]))
    items = np.arange(N_USERS + 1, N_USERS + N_ITEMS + 1)
    now = float(tb[-1]) + 1.0
    before = served.recommend(users, now, 5, items, return_embeddings=True)
    n, idxs = served.ingest(sb, db, tb, g.edge_features[eb])
    assert n == BATCH and idxs.dtype == np.int64 and np.array_equal(idxs, eb), "the batch's original edge indices"
    after = served.recommend(users, now, 5, items, return_embeddings=True)
    with torch.no_grad():
        full.compute_temporal_embeddings(sb, db, rs.randint(N_USERS + 1, N_USERS + N_ITEMS + 1, size=BATCH), tb, eb, K_NBR)
    want = full.recommend(users, now, 5, items, return_embeddings=True)
    got_emb, want_emb = _embeddings(after), _embeddings(want)
    e, moved = relerr(got_emb, want_emb), relerr(_embeddings(before), want_emb)
    print("FIGURES ingest L=%d: embeddings after ingest vs the model built large relerr %.3g (before it: %.3g), bitwise equal: %s"
          % (L, e, moved, got_emb.tobytes() == want_emb.tobytes()))
    assert e < O.RTOL
    assert moved > 1e-3, "the batch must matter to the query, or the test shows nothing"
    e_mem, e_tab = O.check_tables(_tables(served), _tables(full), "ingest")
    print("FIGURES ingest L=%d: memory relerr %.3g, message relerr %.3g" % (L, e_mem, e_tab))
    # the grown table IS the leading rows of the table built large (which holds the whole log's 1501 rows)
    n_rows = CUT + 1 + BATCH
    assert served.edge_raw_features.shape[0] == n_rows == served._cfg.n_edges_p1
    assert _same_bits(served.edge_raw_features.cpu().numpy(), full.edge_raw_features[:n_rows].cpu().numpy())


# ---------------------------------------------------------------------------------------------- 8. new nodes
N0 = N_USERS + N_ITEMS + 1 - 4                                  # the last 4 item ids are unseen by the served model


def _new_node_world():
    """History = the edges before the cut that touch no node >= N0.  Tick = the first 24 later edges such that the ids >= N0,
    in order of first appearance, are N0, N0 + 1, ... (an edge to a later id whose predecessor has not appeared is passed over)."""
    g = _graph(1)
    d = g.data
    hist = np.flatnonzero((d.sources[:CUT] < N0) & (d.destinations[:CUT] < N0))
    tick, seen = [], 0
    for e in range(CUT, len(d.sources)):
        v = int(d.destinations[e])
        if v >= N0 + seen + 1:
            continue
        if v == N0 + seen:
            seen += 1
        tick.append(e)
        if len(tick) == BATCH:
            break
    return g, hist, np.asarray(tick), seen


def test_new_nodes_arrive_with_the_tick():
    g, hist, tick, n_new = _new_node_world()
    d = g.data
    n_all = N_USERS + N_ITEMS + 1
    ids = np.concatenate([d.sources[tick], d.destinations[tick]])
    assert len(tick) == BATCH and n_new >= 1 and int(d.sources.max()) < N0
    assert np.array_equal(np.unique(ids[ids >= N0]), np.arange(N0, N0 + n_new)), "the new ids are consecutive from N0"
    assert len(hist) > 3 * BATCH and not (ids[ids < N0] >= N0).any()
    # edge rows: the served model holds rows 0..CUT; the tick's rows get CUT + 1 .. CUT + 24 in both models
    tick_raw = g.edge_features[d.edge_idxs[tick]]
    tick_idx = np.arange(CUT + 1, CUT + 1 + BATCH)
    nf_s = P.NeighborFinder.from_arrays(d.sources[hist], d.destinations[hist], d.edge_idxs[hist], d.timestamps[hist], uniform=False,
                                        max_node_idx=N0 - 1)
    h_and_t = np.concatenate([hist, tick])
    nf_f = P.NeighborFinder.from_arrays(d.sources[h_and_t], d.destinations[h_and_t], np.concatenate([d.edge_idxs[hist], tick_idx]),
                                        d.timestamps[h_and_t], uniform=False, max_node_idx=n_all - 1)
    assert nf_s.n_nodes == N0
    kw = dict(n_layers=1, n_heads=2, dropout=0.0, use_memory=True, memory_dimension=16, message_function="identity", n_neighbors=K_NBR)
    torch.manual_seed(6)
    served = P.TGN(nf_s, g.node_features[:N0], g.edge_features[:CUT + 1], DEV, **kw)
    full = P.TGN(nf_f, g.node_features, np.concatenate([g.edge_features[:CUT + 1], tick_raw]), DEV, **kw)
    _overwrite_edge_table(full, _frozen(np.concatenate([g.edge_features[:CUT + 1], tick_raw]), served.edge_feature_stats))
    _set_params(full, _params_of(served))
    rs = np.random.RandomState(3)
    for t in (served, full):
        t.eval()
    for k in range(len(hist) - 3 * BATCH, len(hist), BATCH):      # the same warm-up steps on both
        s = hist[k:k + BATCH]
        neg = rs.randint(N_USERS + 1, N0, size=BATCH)
        with torch.no_grad():
            for t in (served, full):
                t.compute_temporal_embeddings(d.sources[s], d.destinations[s], neg, d.timestamps[s], d.edge_idxs[s], K_NBR)
    sb, db, tb = d.sources[tick], d.destinations[tick], d.timestamps[tick]
    n, idxs = served.ingest(sb, db, tb, tick_raw, node_features=g.node_features[N0:N0 + n_new])
    assert n == BATCH and np.array_equal(idxs, tick_idx)
    assert served.n_nodes == served.memory.n_nodes == served._cfg.n_nodes == N0 + n_new and served.neighbor_finder.n_nodes == N0 + n_new
    if n_new < 4:                                               # the ids the tick did not name: the public way to add them
        assert served.add_nodes(4 - n_new, g.node_features[N0 + n_new:]) == N0 + n_new
    assert served.n_nodes == n_all
    with torch.no_grad():
        full.compute_temporal_embeddings(sb, db, rs.randint(N_USERS + 1, N0, size=BATCH), tb, tick_idx, K_NBR)
    e_mem, e_tab = O.check_tables(_tables(served), _tables(full), "new nodes")
    assert _same_bits(served.node_raw_features.cpu().numpy(), full.node_raw_features.cpu().numpy())
    assert _same_bits(served.edge_raw_features.cpu().numpy(), full.edge_raw_features.cpu().numpy())
    # a query whose candidates include the new items: every item comes back (k = all of them) with the full model's score
    users = np.unique(sb[:10])
    items = np.arange(N_USERS + 1, n_all)
    now = float(tb[-1]) + 1.0
    by_item = []
    for t in (served, full):
        ids_k, sc_k, nv = (x.cpu().numpy() for x in t.recommend(users, now, len(items), items)[:3])
        assert (nv == len(items)).all()
        order = np.argsort(ids_k, axis=1)
        assert np.array_equal(np.take_along_axis(ids_k, order, 1), np.broadcast_to(items, ids_k.shape))
        by_item.append(np.take_along_axis(sc_k, order, 1))
    e_all, e_new = relerr(by_item[0], by_item[1]), relerr(by_item[0][:, N0 - N_USERS - 1:], by_item[1][:, N0 - N_USERS - 1:])
    print("FIGURES new nodes (%d of 4 in the tick): memory / message relerr %.3g / %.3g, scores relerr %.3g (new items' columns %.3g)"
          % (n_new, e_mem, e_tab, e_all, e_new))
    assert e_all < O.RTOL and e_new < O.RTOL
    assert np.abs(by_item[1][:, N0 - N_USERS - 1:N0 - N_USERS - 1 + n_new]).max() > 0
    # a training step afterwards: the workspace pool, the adjacency cache and the gradient views survived the growth
    ppos = rs.randint(N_USERS + 1, n_all, size=BATCH)
    pneg = rs.randint(N_USERS + 1, n_all, size=BATCH * 3)
    out = []
    for t in (served, full):
        t.train()
        se, de, pe, ne = t.compute_temporal_embeddings_p(sb, db, ppos, pneg, tb + 1.0, tick_idx, K_NBR)
        loss = P.bpr_loss_blocks(se, de, ne, p_pos_embedding=pe)
        loss.backward()
        t.join()
        out.append((float(loss.detach()), t.flat_grad.detach().cpu().numpy().copy()))
    (la, ga), (lb, gb) = out
    print("FIGURES new nodes, training step after the growth: loss %.6g vs %.6g, gradient relerr %.3g" % (la, lb, relerr(ga, gb)))
    assert abs(la - lb) < O.RTOL * max(1.0, abs(lb))
    assert np.isfinite(ga).all() and np.abs(ga).max() > 0
    O.check_tables(_tables(served), _tables(full), "new nodes, after the step")


# ---------------------------------------------------------------------------------------------- 9. capacity
def test_capacity_is_kept_until_it_is_crossed():
    g = _graph(1)
    d = g.data
    tgn = _model(g, 1, CUT, g.edge_features[:CUT + 1])
    stats = tgn.edge_feature_stats
    live = CUT + 1
    tgn.reserve(n_edges=live + 10)
    assert tgn.edge_capacity == live + 10 and tgn.edge_raw_features.shape[0] == live
    assert _same_bits(tgn.edge_raw_features.cpu().numpy(), _frozen(g.edge_features[:live], stats))
    ptrs, caps, got = [tgn.edge_raw_features.data_ptr()], [tgn.edge_capacity], []
    for k in range(3):
        s = CUT + 8 * k
        sb, db, tb, eb = _batch(d, s, 8)
        n, idxs = tgn.ingest(sb, db, tb, g.edge_features[eb])
        got.append(idxs)
        ptrs.append(tgn.edge_raw_features.data_ptr())
        caps.append(tgn.edge_capacity)
        rows = live + 8 * (k + 1)
        torch.cuda.synchronize()
        assert n == 8 and tgn.edge_raw_features.shape[0] == rows == tgn._cfg.n_edges_p1 and tgn.edge_raw_features.is_contiguous()
        assert _same_bits(tgn.edge_raw_features.cpu().numpy(), _frozen(g.edge_features[:rows], stats)), "tick %d" % k
    assert np.array_equal(np.concatenate(got), np.arange(live, live + 24)), "consecutive across ticks"
    assert ptrs[1] == ptrs[0] and caps[1] == caps[0], "the first tick stays within the reserved capacity"
    assert caps[2] > caps[1] and caps[2] >= live + 16, "the second tick crosses it: reallocated, geometrically"
    for k in range(3):
        if caps[k + 1] == caps[k]:
            assert ptrs[k + 1] == ptrs[k], "a tick within capacity moves nothing (tick %d)" % k
    assert caps[3] == caps[2] and ptrs[3] == ptrs[2]
    # a device tensor of raw rows takes the same launch
    more = torch.from_numpy(g.edge_features[live + 24:live + 29].astype(np.float32)).to(DEV)
    assert np.array_equal(tgn.add_edge_features(more), np.arange(live + 24, live + 29))
    assert _same_bits(tgn.edge_raw_features.cpu().numpy(), _frozen(g.edge_features[:live + 29], stats))


# ---------------------------------------------------------------------------------------------- 10. leaves the rest alone
def test_ingest_leaves_training_alone():
    g = _graph(2)
    d = g.data
    torch.manual_seed(11)
    a = _model(g, 2, CUT, g.edge_features[:CUT + 1], dropout=0.1)
    b = _model(g, 2, CUT, g.edge_features[:CUT + 1], dropout=0.1)
    _set_params(b, _params_of(a))
    rs = np.random.RandomState(9)
    to = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(DEV)

    def dev_batch(s, neg):
        return (to(d.sources[s:s + BATCH], np.int32), to(d.destinations[s:s + BATCH], np.int32), [to(neg, np.int32)], [3],
                to(d.timestamps[s:s + BATCH], np.float64), to(d.edge_idxs[s:s + BATCH], np.int32), K_NBR)
    negs = [rs.randint(N_USERS + 1, N_USERS + N_ITEMS + 1, size=BATCH * 3) for _ in range(2)]

    def train_step(t, args):
        t.train()
        out, _ = t.embed_device(*args)
        loss = P.bpr_loss(out, BATCH, 3)
        loss.backward()
        t.join()
        return float(loss)
    for t in (a, b):                                           # gradients are attached, the state is populated
        train_step(t, dev_batch(CUT - 2 * BATCH, negs[0]))
    params, grad, step = a.flat_parameters.clone(), a.flat_grad.clone(), a._step
    pkey, pcache = a._pcache_key, a._pcache.data_ptr()
    sb, db, tb, eb = _batch(d, CUT)
    n, idxs = a.ingest(sb, db, tb, g.edge_features[eb], batch_size=7)
    torch.cuda.synchronize()
    assert n == BATCH and np.array_equal(idxs, eb)
    assert torch.equal(params, a.flat_parameters) and torch.equal(grad, a.flat_grad) and a._step == step == b._step
    assert a._pcache_key == pkey and a._pcache.data_ptr() == pcache, "the parameter cache and its key are kept"
    assert all(p.grad is not None and p.grad.data_ptr() == v.data_ptr() for (p, _, _, _), v in zip(a._views, a._grad_views[1])
               if p not in a._gru_params)
    # the next forward takes the place in the Philox streams it would have taken without the ingest
    for t in (a, b):
        train_step(t, dev_batch(CUT - BATCH, negs[1]))
    assert a._last_call == b._last_call and a._last_call[4] == pytest.approx(0.1)
    ma, mb = a.debug_dropout_masks(), b.debug_dropout_masks()
    assert all(np.array_equal(ma[l], mb[l]) for l in ma)


def test_without_memory_only_the_tables_and_the_finder_grow():
    g = _graph(1)
    d = g.data
    n_all = N_USERS + N_ITEMS + 1
    tgn = _model(g, 1, CUT, g.edge_features[:CUT + 1], use_memory=False)
    nf = tgn.neighbor_finder
    entries, version = int(nf.indptr[-1]), nf._version
    params, step = tgn.flat_parameters.clone(), tgn._step
    sb, db, tb, eb = _batch(d, CUT, 8)
    db = db.copy()
    db[5] = n_all                                               # an item nobody has seen
    row = np.random.RandomState(2).rand(1, 16)
    n, idxs = tgn.ingest(sb, db, tb, g.edge_features[eb], node_features=row)
    torch.cuda.synchronize()
    assert n == 8 and np.array_equal(idxs, np.arange(CUT + 1, CUT + 9))
    assert tgn.memory is None and tgn._step == step and torch.equal(params, tgn.flat_parameters)
    assert tgn.n_nodes == tgn._cfg.n_nodes == n_all + 1 and tgn.node_raw_features.shape == (n_all + 1, 16)
    assert np.array_equal(tgn.node_raw_features[n_all].cpu().numpy(), row[0].astype(np.float32))
    assert _same_bits(tgn.node_raw_features[:n_all].cpu().numpy(), g.node_features.astype(np.float32))
    assert _same_bits(tgn.edge_raw_features.cpu().numpy(), _frozen(g.edge_features[:CUT + 9], tgn.edge_feature_stats))
    assert nf._version == version + 1 and nf.n_nodes == n_all + 1 and int(nf.indptr[-1]) == entries + 16
    # the grown model embeds: the new item's row is reachable, and the new edges are its neighbourhood
    tgn.eval()
    with torch.no_grad():
        se, de, ne = tgn.compute_temporal_embeddings(sb, db, db, tb + 1.0, idxs, K_NBR)
    assert torch.isfinite(de).all() and float(de[5].abs().max()) > 0
