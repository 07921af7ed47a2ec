"""GPU tests of the explanation query: ``TGN.explain`` against the numpy rule of ``explain_ref`` on the raw tables
the same call returns - every output bit for bit, the fp64 weights included -, against the oracle's attention weights within
the project's parity bar for forward quantities, the raw tables against the sampler, and that a query leaves the model exactly
as it found it.  The worlds follow ``tests/test_gpu_recommend.py``: model [and oracle] on the same parameters, advanced by three
training-path calls so that memory and pending messages are live."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

import pfotgnrec_amd as P
from pfotgnrec_amd import _lib
from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
from oracle import tgn_oracle as T
from oracle.neighbor_finder import OracleNeighborFinder, build_adjacency
import explain_ref as E

DEV = "cuda:0"
RTOL = 1e-4          # README "Parity bars": forward quantities within 1e-4 relative (max norm); the weights are at most 1
BATCH, K_NBR = 40, 10
SIZES = {"big": (1000, 100, 10_000), "small": (30, 8, 2_000)}      # users, items, interactions
NAMES = ("node", "weight", "n_valid", "count", "age", "eidx")


class _World:
    def __init__(self, size, L, use_mem, oracle):
        torch.manual_seed(77 + L)
        self.L, self.use_mem = L, use_mem
        self.n_users, self.n_items, n_edges = SIZES[size]
        self.g = g = make_graph(SyntheticConfig("t", self.n_users, self.n_items, n_edges, 32, L, K_NBR, 2), with_prices=False)
        d = g.data
        self.tgn = P.TGN(P.get_neighbor_finder(d, uniform=False), g.node_features, g.edge_features, DEV, n_layers=L, n_heads=2,
                         dropout=0.0, use_memory=use_mem, memory_dimension=32, message_function="identity", n_neighbors=K_NBR)
        with torch.no_grad():
            self.tgn.time_encoder.w.bias.normal_(0, 0.3)
            for att in self.tgn.embedding_module.attention_models:
                att.multi_head_target.in_proj_bias.normal_(0, 0.1)
                att.multi_head_target.out_proj.bias.normal_(0, 0.1)
        self.ref = None
        if oracle:
            onf = OracleNeighborFinder(*build_adjacency(d.sources, d.destinations, d.edge_idxs, d.timestamps), uniform=False)
            names = [k for k in self.tgn.state_dict() if "layer_norm" not in k and not k.startswith("memory.")]
            params = {k: self.tgn.state_dict()[k].detach().cpu().numpy().copy() for k in names}
            self.ref = T.OracleTGN(onf, g.node_features, g.edge_features, params, L, 2, use_mem)
        self.rs = np.random.RandomState(5)
        self.cursor = int(0.6 * n_edges)
        for _ in range(3):
            self.step(grad=False)
        self.items = np.arange(self.n_users + 1, self.n_users + self.n_items + 1)
        users = np.unique(d.sources[self.cursor - 3 * BATCH:self.cursor])[:9]          # users with fresh memory and messages
        self.nodes = np.concatenate([users, [3, 4], self.items[:3]])                   # two arbitrary ones, and the item side
        self.now = float(d.timestamps[self.cursor + 200])

    def step(self, grad):
        d, s = self.g.data, self.cursor
        self.cursor += BATCH
        sb, db, tb, eb = d.sources[s:s + BATCH], d.destinations[s:s + BATCH], d.timestamps[s:s + BATCH], d.edge_idxs[s:s + BATCH]
        neg = self.rs.randint(self.n_users + 1, self.n_users + self.n_items + 1, size=BATCH * 3)
        self.tgn.train()
        with torch.set_grad_enabled(grad):
            got = torch.cat(list(self.tgn.compute_temporal_embeddings(sb, db, neg, tb, eb, K_NBR)))
        if self.ref is not None:
            self.ref.compute_temporal_embeddings(sb, db, neg, tb, eb, K_NBR)
        return got

    def state(self):
        t = self.tgn
        out = [t.flat_parameters.detach().clone()]
        if t._flat_grad is not None:
            out.append(t._flat_grad.clone())
        if self.use_mem:
            m = t.memory
            out += [x.detach().clone() for x in (m.memory, m.last_update, m.msg_table, m.msg_time, m.has_msg)]
        return out

    def host_flags(self):
        t = self.tgn
        return (t.training, t._step, t._gru_applied_now, t.memory._any_msg if self.use_mem else None,
                t.memory._state_version if self.use_mem else None)


_WORLDS = {}


def _world(size, L, use_mem=True, oracle=False):
    key = (size, L, use_mem, oracle)
    if key not in _WORLDS:
        _WORLDS[key] = _World(*key)
    return _WORLDS[key]


def _host(out):
    """The answer of ``TGN.explain`` on the host: (dict of the six outputs, raw dict or None)."""
    raw = {k: v.cpu().numpy() for k, v in out[6].items()} if len(out) > 6 else None
    return {n: t.cpu().numpy() for n, t in zip(NAMES, out[:6])}, raw


def _same(a, b):
    """bit for bit, NaN padding included"""
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _assert_equals_the_host_model(got, raw, m, hops, tag):
    want = dict(zip(NAMES, E.explain(raw, m, hops)))
    for n in NAMES:
        assert _same(np.ascontiguousarray(got[n]), np.ascontiguousarray(want[n])), (tag, n)
    assert np.array_equal(got["weight"], want["weight"]), tag


# ---------------------------------------------------------------------------------------------- exact against the host model

@pytest.mark.parametrize("size", ["big", "small"])
@pytest.mark.parametrize("L,K,hops", [(1, 3, 1), (2, 10, 1), (2, 10, 2), (2, 64, 2)])
def test_every_output_equals_the_host_model_on_the_raw_tables(size, L, K, hops):
    """The merge and the rank are exact arithmetic on the returned raw tables: sequential fp64 sums in slot / path order, so the
    device's bits are the host model's.  K = 3 is one wavefront with 61 idle lanes, 10 / 100 entries are no power of two, 64 x 64
    paths fill the kernel's LDS image (96 KB, 1024 threads); m = 256 exercises the padding, m = 1 and 7 the cut."""
    w = _world(size, L)
    nodes = w.nodes if K < 64 else w.nodes[[0, 1, 9, 11, 12]]
    ts = np.full(len(nodes), w.now)
    ts[1] -= 4096.0
    merged = 0
    for m in (1, 7, 256):
        out = w.tgn.explain(nodes, ts, m, hops=hops, n_neighbors=K, return_raw=True)
        assert not any(t.requires_grad for t in out[:6]) and all(t.device.type == "cuda" for t in out[:6])
        got, raw = _host(out)
        H = 2
        assert raw["nbr"].shape == (len(nodes), K) and raw["w"].shape == (len(nodes), H, K) and raw["w"].dtype == np.float32
        if hops == 2:
            assert raw["nbr2"].shape == (len(nodes), K, K) and raw["w2"].shape == (len(nodes), K, H, K) and raw["dt2"].shape == (len(nodes), K, K)
        else:
            assert "nbr2" not in raw
        _assert_equals_the_host_model(got, raw, m, hops, (size, L, K, hops, m))
        again, _ = _host(w.tgn.explain(nodes, ts, m, hops=hops, n_neighbors=K))
        assert all(_same(got[n], again[n]) for n in NAMES), "the same input gives the same bits"
        if m == 256:
            merged = int((got["count"] > 1).sum())
            sums = got["weight"].sum(1)
            has = (raw["nbr"] != 0).any(1)
            assert has.all() and (got["n_valid"] > 0).all()
            if hops == 1:
                assert np.abs(sums - 1.0).max() < 1e-6           # fp32 softmax rows, K terms
            else:
                assert (sums < 1.0 + 1e-6).all() and (sums > 0).all()
            assert (got["node"][:, -1] == -1).all() or K == 64, "padding is exercised"
    # (the newest three of a big-world node never repeat a partner - 100 items; every other case merges slots or paths)
    assert merged > 0 or (size, K) == ("big", 3), "duplicates within a neighbourhood"
    if size == "small" and K >= 10:                            # 8 items: almost every slot repeats a node
        assert (got["n_valid"] <= w.n_users + w.n_items).all() and merged >= len(nodes)


# ---------------------------------------------------------------------------------------------- parity with the oracle

@pytest.mark.parametrize("L,use_mem", [(1, True), (2, True), (2, False)], ids=["L1_mem", "L2_mem", "L2_nomem"])
def test_weights_match_the_oracles_attention(L, use_mem):
    """Full-width answers scattered into [U, n_nodes] against the host model fed the oracle's own weights: no entry is left
    out; the order is not compared here (near-ties may differ - the exact test owns it)."""
    w = _world("big", L, use_mem, oracle=True)
    ts = np.full(len(w.nodes), w.now)
    ts[::3] -= 4096.0
    mem = w.ref._get_updated_memory()[0] if use_mem else None
    ctx = w.ref._embed(mem, np.asarray(w.nodes, np.int64), ts, L, K_NBR, None)[1]
    n_nodes = w.g.node_features.shape[0]
    for hops in range(1, min(2, L) + 1):
        got, _ = _host(w.tgn.explain(w.nodes, ts, 256, hops=hops, n_neighbors=K_NBR))
        want = E.explain(E.oracle_raw(ctx, hops), 256, hops)
        assert (got["n_valid"] < 256).all() and (want[2] < 256).all()
        a, b = E.dense(got["node"], got["weight"], n_nodes), E.dense(want[0], want[1], n_nodes)
        e = np.abs(a - b).max() / np.abs(b).max()
        print("FIGURES explain vs oracle (L=%d, memory=%s, hops=%d): max|a-b| / max|b| = %.3g" % (L, use_mem, hops, e))
        assert e <= RTOL
        assert np.array_equal(got["n_valid"], want[2])         # the same distinct nodes: the sampler is index-exact


# ---------------------------------------------------------------------------------------------- the raw tables

def test_raw_tables_are_the_samplers():
    w = _world("big", 2)
    ts = np.full(len(w.nodes), w.now)
    ts[::2] -= 30000.0
    _, raw = _host(w.tgn.explain(w.nodes, ts, 5, hops=2, n_neighbors=K_NBR, return_raw=True))
    nf = w.tgn.neighbor_finder
    nbr, eidx, et = nf.get_temporal_neighbor(w.nodes, ts, K_NBR)
    assert np.array_equal(raw["nbr"], nbr) and np.array_equal(raw["eidx"], eidx) and (nbr != 0).any() and (nbr == 0).any()
    assert _same(raw["dt"], (ts[:, None] - et.astype(np.float64)).astype(np.float32))
    # ... and one level down: the neighbours' instances, all at their root's time
    ts2 = np.repeat(ts, K_NBR)
    nbr2, eidx2, et2 = nf.get_temporal_neighbor(nbr.reshape(-1), ts2, K_NBR)
    U = len(w.nodes)
    assert np.array_equal(raw["nbr2"], nbr2.reshape(U, K_NBR, K_NBR)) and np.array_equal(raw["eidx2"], eidx2.reshape(U, K_NBR, K_NBR))
    assert _same(raw["dt2"], (ts2[:, None] - et2.astype(np.float64)).astype(np.float32).reshape(U, K_NBR, K_NBR))
    assert (raw["w"][raw["nbr"][:, None, :].repeat(2, 1) == 0] == 0).all(), "padding slots weigh nothing"


# ---------------------------------------------------------------------------------------------- empty rows

@pytest.mark.parametrize("L,hops", [(1, 1), (2, 1), (2, 2)])
def test_empty_rows(L, hops):
    w = _world("big", L)
    d = w.g.data
    first = {int(u): float(d.timestamps[np.flatnonzero(d.sources == u)[0]]) for u in w.nodes[:4]}
    ts = np.full(len(w.nodes), w.now)
    ts[:4] = [first[int(u)] for u in w.nodes[:4]]              # AT the first interaction: nothing lies strictly before it
    ts[2] -= 1.0

    def padded(got, rows):
        return ((got["n_valid"][rows] == 0).all() and (got["node"][rows] == -1).all() and (got["weight"][rows] == 0.0).all()
                and (got["count"][rows] == 0).all() and np.isnan(got["age"][rows]).all() and (got["eidx"][rows] == -1).all())
    got, raw = _host(w.tgn.explain(w.nodes, ts, 6, hops=hops, return_raw=True))
    assert padded(got, slice(0, 4)) and (raw["nbr"][:4] == 0).all() and (got["n_valid"][4:] > 0).all()
    got, raw = _host(w.tgn.explain(w.nodes, w.now, 6, hops=hops, n_neighbors=0, return_raw=True))
    assert padded(got, slice(None)) and raw["nbr"].shape == (len(w.nodes), 1) and (raw["nbr"] == 0).all()
    got, _ = _host(w.tgn.explain(w.nodes[:0], w.now, 6, hops=hops))
    assert got["node"].shape == (0, 6) and got["n_valid"].shape == (0,)


# ---------------------------------------------------------------------------------------------- the walk and the inputs

@pytest.mark.parametrize("hops", [1, 2])
def test_chunk_walk_and_input_forms(hops):
    w = _world("big", 2)
    nodes = w.nodes[:7]
    ts = np.full(7, w.now)
    ts[::3] -= 4096.0
    whole = w.tgn.explain(nodes, ts, 9, hops=hops, return_raw=True)
    w.tgn.eval_chunk_roots = 3                                 # 7 roots in three passes, the last of one root
    try:
        parts = w.tgn.explain(nodes, ts, 9, hops=hops, return_raw=True)
    finally:
        w.tgn.eval_chunk_roots = 16384
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(whole[:6], parts[:6]))
    assert all(torch.equal(whole[6][k], parts[6][k]) for k in whole[6])
    # a scalar time is the equal per-node vector; device tensors are the host inputs
    a = w.tgn.explain(nodes, w.now, 9, hops=hops)
    b = w.tgn.explain(nodes, np.full(7, w.now), 9, hops=hops)
    c = w.tgn.explain(torch.from_numpy(nodes).to(DEV), torch.full((7,), w.now, dtype=torch.float64, device=DEV), 9, hops=hops)
    e = w.tgn.explain(nodes.tolist(), torch.tensor(w.now, dtype=torch.float64), 9, hops=hops)
    for other in (b, c, e):
        assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, other))
    # one node alone at its time gets what it got in the crowd
    one = w.tgn.explain(nodes[4:5], ts[4], 9, hops=hops)
    assert all(torch.equal(x[0:1].view(torch.uint8), y[4:5].view(torch.uint8)) for x, y in zip(one, whole[:6]))


# ---------------------------------------------------------------------------------------------- read-only

@pytest.mark.parametrize("L,use_mem", [(1, True), (2, True), (2, False)], ids=["L1_mem", "L2_mem", "L2_nomem"])
def test_explain_changes_nothing(L, use_mem):
    w = _world("big", L, use_mem, oracle=True)
    w.tgn.dropout = 0.1                                        # train mode with dropout on: a query must not apply it
    try:
        rec = w.tgn.recommend(w.nodes[:9], w.now, 5, w.items)
        for mode in (True, False):
            w.tgn.train(mode)
            before, flags = w.state(), w.host_flags()
            a = w.tgn.explain(w.nodes, w.now, 7, hops=min(2, L), return_raw=True)
            b = w.tgn.explain(w.nodes, w.now, 7, hops=min(2, L), return_raw=True)
            assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a[:6], b[:6]))
            assert all(torch.equal(a[6][k], b[6][k]) for k in a[6])
            assert all(torch.equal(x, y) for x, y in zip(before, w.state()))
            assert flags == w.host_flags()
        w.tgn.train()
        assert all(torch.equal(x, y) for x, y in zip(rec, w.tgn.recommend(w.nodes[:9], w.now, 5, w.items)))
    finally:
        w.tgn.dropout = 0.0


def test_training_step_after_explain_is_the_twins():
    """Two worlds built alike; one answers queries between its steps.  Their next training step - embeddings under autograd,
    then the state update - must be the same to the bit (the forward and the state update add nothing out of order)."""
    asked, twin = _World("big", 2, True, False), _World("big", 2, True, False)
    for hops in (1, 2):
        asked.tgn.explain(asked.nodes, asked.now, 7, hops=hops, return_raw=True)
    asked.tgn.eval_chunk_roots = 5
    try:
        asked.tgn.explain(asked.nodes, asked.now, 256, hops=2, n_neighbors=64)
    finally:
        asked.tgn.eval_chunk_roots = 16384
    a, b = asked.step(grad=True), twin.step(grad=True)
    assert a.requires_grad and torch.equal(a, b)
    assert asked.host_flags() == twin.host_flags()
    for x, y in zip(asked.state(), twin.state()):
        assert torch.equal(x, y)
    P.bpr_loss(a, BATCH, 3).backward()
    grads = [p.grad for p in asked.tgn.parameters() if p.requires_grad and p.grad is not None]
    assert grads and all(torch.isfinite(g_).all() for g_ in grads) and any(float(g_.abs().max()) > 0 for g_ in grads)


# ---------------------------------------------------------------------------------------------- the C entry

def test_entry_refuses_and_queues_nothing():
    w = _world("big", 2)
    U, K, m = len(w.nodes), K_NBR, 7
    w.tgn.explain(w.nodes, w.now, m, hops=2)                   # leaves a sampled workspace behind
    cfg, ws = w.tgn._last_ws
    i32 = lambda *s: torch.full(s, -77, dtype=torch.int32, device=DEV)
    outs = [i32(U, m), torch.full((U, m), 123.25, dtype=torch.float64, device=DEV), i32(U), i32(U, m),
            torch.full((U, m), 123.25, dtype=torch.float32, device=DEV), i32(U, m)]
    raws = [i32(U, K), torch.full((U, 2, K), 123.25, device=DEV), torch.full((U, K), 123.25, device=DEV), i32(U, K),
            i32(U, K, K), torch.full((U, K, 2, K), 123.25, device=DEV), torch.full((U, K, K), 123.25, device=DEV), i32(U, K, K)]
    before = [t.clone() for t in outs + raws]
    lib = _lib.load()

    def call(R=U, K=K, hops=2, m=m, cfg=cfg, ws=ws.data_ptr(), outs=outs, raws=raws):
        rc = lib.pfo_tgn_explain(ctypes.byref(cfg), ws, R, K, hops, m, *[None if t is None else t.data_ptr() for t in list(outs) + list(raws)],
                                 _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc, lib.pfo_last_error().decode()
    one_layer = _lib.TgnConfig(cfg.n_nodes, cfg.n_edges_p1, cfg.D, cfg.Ef, 1, cfg.n_heads, cfg.use_memory, cfg.max_roots,
                               cfg.max_neighbors, cfg.max_batch, cfg.msg_dim, cfg.msg_hidden)
    bad = [(dict(m=0), "m must lie"), (dict(m=257), "m must lie"), (dict(hops=0), "hops must lie"), (dict(hops=3), "hops must lie"),
           (dict(cfg=one_layer), "hops must lie"), (dict(K=0), "K must lie"), (dict(K=65), "K must lie"),
           (dict(K=cfg.max_neighbors + 1), "K must lie"), (dict(R=-1), "R must lie"), (dict(R=cfg.max_roots + 1), "R must lie"),
           (dict(ws=None), "null pointer"), (dict(raws=raws[:2] + [None] + raws[3:]), "raw group"),
           (dict(raws=raws[:4] + [None] + raws[5:]), "raw group")]
    bad += [(dict(outs=outs[:i] + [None] + outs[i + 1:]), "null pointer") for i in range(6)]
    for kw, word in bad:
        rc, err = call(**kw)
        assert rc == -1 and word in err and err.startswith("pfo_tgn_explain:"), (kw.keys(), rc, err)
        assert all(torch.equal(x, y) for x, y in zip(before, outs + raws)), kw.keys()
    assert call(R=0)[0] == 0 and all(torch.equal(x, y) for x, y in zip(before, outs + raws))
    # ... and the call the query itself makes, through the raw entry: the answer of TGN.explain
    assert call()[0] == 0
    want = w.tgn.explain(w.nodes, w.now, m, hops=2, return_raw=True)
    assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(outs, want[:6]))
    assert all(torch.equal(x, want[6][k]) for x, k in zip(raws, ("nbr", "w", "dt", "eidx", "nbr2", "w2", "dt2", "eidx2")))
