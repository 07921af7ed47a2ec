"""GPU tests of ``TGN.observe`` (``pfo_tgn_observe``): the state it leaves against the reference's goldens, against the
model's own step, against the CPU helper of tests/observe_ref.py on the shapes the kernels can get wrong, and what it must
leave alone.  Bars: 1e-4 in the max norm for memory and message rows; has_msg, last_update and message times exact."""
import numpy as np
import pytest
import torch

from conftest import load_golden, has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

import pfotgnrec_amd as P
from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
from parity import relerr
import observe_ref as O

DEV = "cuda:0"


def _tables(tgn):
    m = tgn.memory
    torch.cuda.synchronize()
    return tuple(t.detach().cpu().numpy().copy() for t in (m.memory, m.last_update, m.msg_table, m.msg_time, m.has_msg))


def _set_tables(tgn, tables):
    """memory, last_update and the pending-message tables, in place (parameters - and the parameter cache - untouched)."""
    mem, lu, tab, mt, has = tables
    m = tgn.memory
    with torch.no_grad():
        m.memory.copy_(torch.from_numpy(np.ascontiguousarray(mem, dtype=np.float32)))
        m.last_update.copy_(torch.from_numpy(np.ascontiguousarray(lu, dtype=np.float32)))
        m.msg_table.copy_(torch.from_numpy(np.ascontiguousarray(tab, dtype=np.float32)))
        m.msg_time.copy_(torch.from_numpy(np.ascontiguousarray(mt, dtype=np.float32)))
        m.has_msg.copy_(torch.from_numpy((np.asarray(has) > 0).astype(np.uint8)))
    m._any_msg = False
    m._state_version += 1


def _set_params(tgn, params):
    sd = tgn.state_dict()
    with torch.no_grad():
        for k, v in params.items():
            if k in sd:
                sd[k].copy_(torch.from_numpy(np.asarray(v, np.float32)).reshape(sd[k].shape))
    tgn.parameters_changed()


def _golden_state(g, pre):
    return (g[pre + "sd_memory.memory"], g[pre + "sd_memory.last_update"], g[pre + "msg_tab"], g[pre + "msg_t"], g[pre + "msg_cnt"] > 0)


def _golden_params(g, pre):
    return {k[len(pre + "sd_"):]: g[k] for k in g.files if k.startswith(pre + "sd_") and not k.startswith(pre + "sd_memory.")}


def _golden_model(g, finder_edges=None):
    n = len(g["src_all"]) if finder_edges is None else finder_edges
    nf = P.NeighborFinder.from_arrays(g["src_all"][:n], g["dst_all"][:n], g["eidx_all"][:n], g["ts_all"][:n], uniform=False,
                                      max_node_idx=g["node_features"].shape[0] - 1)
    D = g["node_features"].shape[1]
    return P.TGN(nf, g["node_features"], g["edge_features"], DEV, n_layers=int(g["L"]), n_heads=int(g["H"]), dropout=0.0,
                 use_memory=True, memory_dimension=D, message_function="identity", n_neighbors=int(g["K"]))


def _world_model(w):
    rs = np.random.RandomState(1)
    n, E = w["n_nodes"], w["edge_features"].shape[0] - 1
    nf = P.NeighborFinder.from_arrays(rs.randint(1, n, 8), rs.randint(1, n, 8), rs.randint(1, E + 1, 8), np.arange(8.0),
                                      uniform=False, max_node_idx=n - 1)
    tgn = P.TGN(nf, w["node_features"], w["edge_features"], DEV, n_layers=w["L"], n_heads=w["H"], dropout=0.0, use_memory=True,
                memory_dimension=w["D"], message_function="identity", n_neighbors=4)
    _set_params(tgn, w["params"])
    _set_tables(tgn, w["state"])
    return tgn


def _bitwise(a, b):
    return all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------- 4. golden parity on the device
@pytest.mark.parametrize("fixture", O.MEM_FIXTURES)
def test_golden_parity_on_the_device(fixture):
    g = load_golden(fixture)
    tgn = _golden_model(g)
    for step in O.STEPS:
        pre = "s%d_" % step
        _set_params(tgn, _golden_params(g, pre))
        _set_tables(tgn, _golden_state(g, pre))
        step_before = tgn._step
        assert tgn.observe(g[pre + "src"], g[pre + "dst"], g[pre + "ts"], g[pre + "eidx"]) == len(g[pre + "src"])
        e_mem, e_tab = O.check_tables(_tables(tgn), O.golden_after(g, pre), (fixture, step))
        print("FIGURES observe %s step %d: memory relerr %.3g, message relerr %.3g" % (fixture, step, e_mem, e_tab))
        assert tgn._step == step_before and tgn.memory._any_msg


# ---------------------------------------------------------------------------------------------- 5. the model's own step
@pytest.mark.parametrize("fixture", ["g5_step_L1_mem", "g5_step_L2_mem"])
def test_agrees_with_the_models_own_step(fixture):
    """Twin models, identical injected state: one takes the batch through eval-mode ``compute_temporal_embeddings``, the
    other through ``observe``.  Round one right after the parameters were written (observe builds the GRU's weight images
    itself), round two with a valid parameter cache (it takes them from there)."""
    g = load_golden(fixture)
    a, b = _golden_model(g), _golden_model(g)
    K = int(g["K"])
    for t in (a, b):
        _set_params(t, _golden_params(g, "s2_"))
        t.eval()
    bitwise = []
    for rnd, step in enumerate((2, 4)):
        pre = "s%d_" % step
        sb, db, tb, eb, neg = g[pre + "src"], g[pre + "dst"], g[pre + "ts"], g[pre + "eidx"], g[pre + "neg"]
        if rnd == 1:
            with torch.no_grad():                               # a forward of its own leaves b's parameter cache valid
                b.compute_temporal_embeddings(sb, db, neg.flatten(), tb, eb, K)
            assert b.param_cache and b._pcache_key is not None and b._pcache_key == b._param_key()
        for t in (a, b):
            _set_tables(t, _golden_state(g, pre))
        with torch.no_grad():
            a.compute_temporal_embeddings(sb, db, neg.flatten(), tb, eb, K)
        b.observe(sb, db, tb, eb)
        ta, tb_ = _tables(a), _tables(b)
        O.check_tables(tb_, ta, (fixture, step))
        bitwise.append(_bitwise(ta, tb_))
    print("FIGURES observe vs the step's own state update (%s): bitwise equal per round %s" % (fixture, bitwise))


# ---------------------------------------------------------------------------------------------- 6. the batch walk
def test_batch_walk_is_the_chain_of_single_calls():
    g = load_golden("g5_step_L1_mem")
    k0, n = int(np.flatnonzero(g["eidx_all"] == g["s2_eidx"][0])[0]), 5 * 24 + 7
    log = tuple(g[k][k0:k0 + n] for k in ("src_all", "dst_all", "ts_all", "eidx_all"))
    assert len(log[0]) == n and np.array_equal(log[0][:24], g["s2_src"])
    one, many = _golden_model(g), _golden_model(g)
    for t in (one, many):
        _set_params(t, _golden_params(g, "s2_"))
        _set_tables(t, _golden_state(g, "s2_"))
    assert one.observe(*log, batch_size=24) == n
    for k in range(0, n, 24):
        assert many.observe(*(a[k:k + 24] for a in log)) == min(24, n - k)
    t_one, t_many = _tables(one), _tables(many)
    assert _bitwise(t_one, t_many), "one walk over 6 batches and 6 single calls run the same code on the same inputs"
    o = O.golden_oracle(g)
    O.load_golden_state(o, g, "s2_")
    o.observe_log(*log, batch_size=24)
    print("FIGURES observe batch walk vs helper: memory / message relerr %.3g / %.3g" % O.check_tables(t_one, o.tables(), "walk"))
    # device tensors take the same walk
    dev = _golden_model(g)
    _set_params(dev, _golden_params(g, "s2_"))
    _set_tables(dev, _golden_state(g, "s2_"))
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)
    assert dev.observe(to(log[0], np.int32), to(log[1], np.int32), to(log[2], np.float64), to(log[3], np.int32), batch_size=24) == n
    assert _bitwise(t_one, _tables(dev))
    # batch_size = 1: the serial chain
    _set_tables(one, _golden_state(g, "s2_"))
    O.load_golden_state(o, g, "s2_")
    assert one.observe(*(a[:10] for a in log), batch_size=1) == 10
    o.observe_log(*(a[:10] for a in log), batch_size=1)
    O.check_tables(_tables(one), o.tables(), "serial")


# ---------------------------------------------------------------------------------------------- 7. edges the kernels can get wrong
def _edge_case(name):
    """(world, pre-state override or None, [batches of 8]) - hand-made over <= 40 nodes."""
    D, Ef = (172, 4) if name == "c2_widths" else (16, 4)
    w = O.random_world(11, 40, D, Ef, 60, pending=0.5)
    rs = np.random.RandomState(4)
    ts = 200.0 + 3.0 * np.arange(8)
    eidx = rs.randint(1, 61, 8)
    has = w["state"][4]
    with_msg, without = np.flatnonzero(has), np.flatnonzero(~has)[1:]          # (node 0 is the padding node)
    if name == "after_init":
        # the first batch after __init_memory__: nothing is pending, the GRU runs over zero rows; a second batch finds the first's messages
        M = 3 * D + Ef
        w["state"] = (np.zeros((40, D), np.float32), np.zeros(40, np.float32), np.zeros((40, M), np.float32),
                      np.zeros(40, np.float32), np.zeros(40, bool))
        src, dst = rs.randint(1, 20, 8), rs.randint(20, 40, 8)
        return w, [(src, dst, ts, eidx), (src[::-1].copy(), dst, ts + 100.0, eidx)]
    if name == "mixed_pending":
        src = np.array([with_msg[0], without[0], with_msg[1], without[1], with_msg[2], without[2], with_msg[3], without[3]])
        dst = np.array([without[4], with_msg[4], without[5], with_msg[5], with_msg[6], without[6], without[7], with_msg[7]])
        return w, [(src, dst, ts, eidx)]
    if name == "one_node_every_event":
        v = int(with_msg[0])
        return w, [(np.full(8, v), np.full(8, v), ts, eidx), (np.full(8, v), rs.randint(1, 40, 8), ts + 100.0, eidx)]
    if name == "source_then_destination":
        # node v is the source of event 1 and the destination of event 6: e = 8 + 6 is the larger, the destination-side message wins
        v, u = int(with_msg[1]), int(without[0])
        src = np.array([with_msg[2], v, with_msg[3], without[1], u, without[2], with_msg[4], with_msg[5]])
        dst = np.array([without[3], with_msg[6], u, with_msg[7], without[4], with_msg[8], v, without[5]])
        return w, [(src, dst, ts, eidx)]
    if name == "c2_widths":
        src = np.concatenate([with_msg[:6], without[:2]])                       # 13 distinct rows with a message: no multiple of 64
        dst = np.concatenate([with_msg[6:13], with_msg[:1]])
        return w, [(src, dst, ts, eidx)]
    raise KeyError(name)


@pytest.mark.parametrize("name", ["after_init", "mixed_pending", "one_node_every_event", "source_then_destination", "c2_widths"])
def test_edges_against_the_cpu_helper(name):
    w, batches = _edge_case(name)
    tgn, o = _world_model(w), O.world_oracle(w)
    for i, (src, dst, ts, eidx) in enumerate(batches):
        before = _tables(tgn)
        assert tgn.observe(src, dst, ts, eidx) == 8
        o.observe(src, dst, ts, eidx)
        got = _tables(tgn)
        e_mem, e_tab = O.check_tables(got, o.tables(), (name, i))
        print("FIGURES observe edge %s batch %d: memory relerr %.3g, message relerr %.3g" % (name, i, e_mem, e_tab))
        # what the batch does not name keeps every bit; so do memory and last_update of positives without a pending message
        pos = np.zeros(40, bool); pos[np.concatenate([src, dst])] = True
        for x, y in zip(before, got):
            assert np.array_equal(x[~pos], y[~pos])
        kept = pos & ~(before[4] > 0)
        assert np.array_equal(before[0][kept], got[0][kept]) and np.array_equal(before[1][kept], got[1][kept])
        assert (got[4][pos] == 1).all()
    if name == "source_then_destination":
        src, dst, ts, _ = batches[0]
        v = int(src[1])
        assert got[3][v] == np.float32(ts[6]) and np.array_equal(got[2][v, 16:32], got[0][src[6]])   # [memory[v] | memory[other]]: the other side of event 6


# ---------------------------------------------------------------------------------------------- 8. the large-batch store
def test_large_batch_takes_the_winner_table():
    B = 8200                                                    # 2 B = 16400 events: just over the inline limit of 16384
    w = O.random_world(21, 300, 16, 4, 500, pending=0.6)
    rs = np.random.RandomState(8)
    src, dst = rs.randint(1, 150, B), rs.randint(150, 300, B)
    ts, eidx = 300.0 + np.arange(B) * 0.25, rs.randint(1, 501, B)
    tgn, o = _world_model(w), O.world_oracle(w)
    assert tgn.observe(src, dst, ts, eidx) == B
    o.observe(src, dst, ts, eidx)
    e_mem, e_tab = O.check_tables(_tables(tgn), o.tables(), "B=8200")
    print("FIGURES observe B=8200: memory relerr %.3g, message relerr %.3g" % (e_mem, e_tab))
    # and a walk whose trailing batch is back under the limit
    _set_tables(tgn, w["state"])
    o = O.world_oracle(w)
    n = B + 100
    src2, dst2 = np.concatenate([src, src[:100]]), np.concatenate([dst, dst[:100][::-1]])
    ts2, eidx2 = np.concatenate([ts, ts[-1] + 1.0 + np.arange(100)]), np.concatenate([eidx, eidx[:100]])
    assert tgn.observe(src2, dst2, ts2, eidx2, batch_size=B) == n
    o.observe_log(src2, dst2, ts2, eidx2, batch_size=B)
    O.check_tables(_tables(tgn), o.tables(), "B=8200 + 100")


# ---------------------------------------------------------------------------------------------- 9. the serving loop
N_USERS, N_ITEMS, K_NBR, BATCH = 120, 30, 5, 24


def _serving_pair(L):
    torch.manual_seed(5 + L)
    g = make_graph(SyntheticConfig("t", N_USERS, N_ITEMS, 1500, 16, L, K_NBR, 2), with_prices=False)
    d, cut = g.data, 900
    def model(n_edges):
        nf = P.NeighborFinder.from_arrays(d.sources[:n_edges], d.destinations[:n_edges], d.edge_idxs[:n_edges], d.timestamps[:n_edges],
                                          uniform=False, max_node_idx=g.node_features.shape[0] - 1)
        return P.TGN(nf, g.node_features, g.edge_features, DEV, n_layers=L, n_heads=2, dropout=0.0, use_memory=True,
                     memory_dimension=16, message_function="identity", n_neighbors=K_NBR)
    served, full = model(cut), model(cut + BATCH)             # (the served model's finder will get the next batch appended)
    _set_params(full, {k: v.detach().cpu().numpy() for k, v in served.state_dict().items() if not k.startswith("memory.")})
    return g, cut, served, full


@pytest.mark.parametrize("L", [1, 2])
def test_serving_loop_recommend_observe_recommend(L):
    g, cut, served, full = _serving_pair(L)
    d = g.data
    rs = np.random.RandomState(3)
    batch = lambda s: (d.sources[s:s + BATCH], d.destinations[s:s + BATCH], d.timestamps[s:s + BATCH], d.edge_idxs[s:s + BATCH])
    for t in (served, full):
        t.eval()
    for s in range(cut - 3 * BATCH, cut, BATCH):               # both reach the same state the only way the parent commit offers
        sb, db, tb, eb = batch(s)
        neg = rs.randint(N_USERS + 1, N_USERS + N_ITEMS + 1, size=BATCH)
        with torch.no_grad():
            for t in (served, full):
                t.compute_temporal_embeddings(sb, db, neg, tb, eb, K_NBR)
    sb, db, tb, eb = batch(cut)
    users = np.unique(np.concatenate([sb[:10], d.sources[cut - BATCH:cut][:10]]))
    items = np.arange(N_USERS + 1, N_USERS + N_ITEMS + 1)
    now = float(tb[-1]) + 1.0
    before = served.recommend(users, now, 5, items, return_embeddings=True)
    assert served.observe(sb, db, tb, eb, append=True) == BATCH
    after = served.recommend(users, now, 5, items, return_embeddings=True)
    with torch.no_grad():
        full.compute_temporal_embeddings(sb, db, rs.randint(N_USERS + 1, N_USERS + N_ITEMS + 1, size=BATCH), tb, eb, K_NBR)
    want = full.recommend(users, now, 5, items, return_embeddings=True)
    got_emb = np.concatenate([after[3].cpu().numpy(), after[4].cpu().numpy()])
    want_emb = np.concatenate([want[3].cpu().numpy(), want[4].cpu().numpy()])
    e = relerr(got_emb, want_emb)
    moved = relerr(np.concatenate([before[3].cpu().numpy(), before[4].cpu().numpy()]), want_emb)
    print("FIGURES serving loop L=%d: embeddings after observe vs the full model relerr %.3g (before it: %.3g)" % (L, e, moved))
    assert e < O.RTOL
    assert moved > 1e-3, "the batch must matter to the query, or the test shows nothing"
    O.check_tables(_tables(served), _tables(full), "serving")


# ---------------------------------------------------------------------------------------------- 10. leaves training alone
def test_leaves_training_alone():
    g, cut, a, b = _serving_pair(2)
    d = g.data
    # (both finders over the whole log from here on: the twins differ in how they take ONE batch in)
    a.set_neighbor_finder(b.neighbor_finder)
    rs = np.random.RandomState(9)
    to = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(DEV)
    def dev_batch(s, neg):
        return (to(d.sources[s:s + BATCH], np.int32), to(d.destinations[s:s + BATCH], np.int32), [to(neg, np.int32)], [3],
                to(d.timestamps[s:s + BATCH], np.float64), to(d.edge_idxs[s:s + BATCH], np.int32), K_NBR)
    negs = [rs.randint(N_USERS + 1, N_USERS + N_ITEMS + 1, size=BATCH * 3) for _ in range(3)]

    def train_step(t, args):
        t.train()
        out, _ = t.embed_device(*args)
        loss = P.bpr_loss(out, BATCH, 3)
        loss.backward()
        return out.detach().cpu().numpy(), float(loss)
    for t in (a, b):                                           # one training step each: gradients are attached, state is populated
        train_step(t, dev_batch(cut, negs[0]))
    s1, s2 = cut + BATCH, cut + 2 * BATCH
    # a: a batch prepared ahead of time, then observe - the prepared batch must be dropped, not consumed
    pre_args = dev_batch(s2, negs[2])
    a.train()
    with torch.enable_grad(), a.prefetching():
        assert a.prefetch(*pre_args)
    params, grad, step = a.flat_parameters.clone(), a.flat_grad.clone(), a._step
    assert a.observe(d.sources[s1:s1 + BATCH], d.destinations[s1:s1 + BATCH], d.timestamps[s1:s1 + BATCH], d.edge_idxs[s1:s1 + BATCH]) == BATCH
    assert a._prefetched is None
    assert torch.equal(params, a.flat_parameters) and torch.equal(grad, a.flat_grad) and a._step == step
    # b: the same batch through the eval-mode entry point
    b.eval()
    with torch.no_grad():
        b.compute_temporal_embeddings(d.sources[s1:s1 + BATCH], d.destinations[s1:s1 + BATCH], negs[1][:BATCH], d.timestamps[s1:s1 + BATCH],
                                      d.edge_idxs[s1:s1 + BATCH], K_NBR)
    O.check_tables(_tables(a), _tables(b), "twins before the step")
    for t in (a, b):
        t.request_zero_grad()
    (ea, la), (eb, lb) = train_step(a, pre_args), train_step(b, dev_batch(s2, negs[2]))      # (a: the very tensors it had prepared)
    assert relerr(ea, eb) < O.RTOL and abs(la - lb) < 1e-4 * max(1.0, abs(lb))
    O.check_tables(_tables(a), _tables(b), "twins after the step")
    ga, gb = a.flat_grad.cpu().numpy(), b.flat_grad.cpu().numpy()
    assert np.isfinite(ga).all() and np.abs(ga).max() > 0
    print("FIGURES observe then train: embeddings relerr %.3g, loss %.6g vs %.6g, gradient relerr %.3g" % (relerr(ea, eb), la, lb, relerr(ga, gb)))
