"""GPU tests of the backward beside the host loop (``tgn.overlap_backward``, ``TGN.beside``): which stream an optimizer step
takes, and how long an in-flight backward keeps its workspace.  Structural and bitwise: nothing here tries to lose a race."""
import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

if has_gpu():
    import pfotgnrec_amd as P
    DEV = torch.device("cuda:0")

B, K, Q = 48, 8, 3
_GRAPH = []


def _graph():
    if not _GRAPH:
        from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
        _GRAPH.append(make_graph(SyntheticConfig("o6", 300, 25, 6000, 64, 2, 8, 2), with_prices=False))
    return _GRAPH[0]


def _model(kind, overlap):
    g = _graph()
    torch.manual_seed(21)
    tgn = P.TGN(P.get_neighbor_finder(g.data, False), g.node_features, g.edge_features, DEV, n_layers=2, n_heads=2, dropout=0.0,
                use_memory=True, memory_dimension=64, message_function="identity", n_neighbors=K)
    tgn.deterministic = True
    if kind == "fused":
        return tgn, P.FusedAdam(tgn, lr=1e-3, overlap_backward=overlap)
    opt = torch.optim.Adam(tgn.parameters(), lr=1e-3)
    return tgn, (P.overlap_backward(tgn, opt) if overlap else opt)


def _autograd_loss(tgn, step, neg):
    """The reference loop's forward and BPR expression (main.py:364-381) on numpy batches."""
    d, s = _graph().data, 2500 + step * B
    tgn.train()
    se, de, ne = tgn.compute_temporal_embeddings(d.sources[s:s + B], d.destinations[s:s + B], neg, d.timestamps[s:s + B],
                                                  d.edge_idxs[s:s + B], K)
    se, de, ne = se.view(B, 1, -1), de.view(B, 1, -1), ne.view(B, Q, -1)
    pos = torch.sum(se * de, dim=2)
    ngs = torch.matmul(se, ne.transpose(1, 2)).squeeze()
    return -torch.mean(torch.log(torch.sigmoid(torch.mean(pos - ngs, dim=1))))


def _final(tgn):
    tgn.join()
    torch.cuda.synchronize()
    return tgn.flat_parameters.detach().cpu().numpy().copy(), tgn.memory.memory.detach().cpu().numpy().copy()


@pytest.mark.parametrize("kind", ["fused", "torch"])
def test_a_backward_on_the_callers_stream_sends_the_step_the_serial_way(kind):
    """Six steps under an overlap optimizer: even steps ``loss.backward(); opt.step()`` (backward and step beside the loop),
    odd steps ``bpr_step(tgn, emb, B, n_neg)`` without ``optimizer=`` - a native backward on the CALLER's stream - then
    ``opt.step()``.  That step must not go to the backward stream, where nothing orders it behind the caller's: nothing is in
    flight afterwards and the awaited event has not moved.  Losses, parameters and memory bit-identical to the serial order."""
    d = _graph().data
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)

    def run(overlap):
        tgn, opt = _model(kind, overlap)
        rs = np.random.RandomState(3)
        losses = []
        for step in range(6):
            s = 2500 + step * B
            opt.zero_grad()
            neg = rs.randint(301, 326, size=B * Q)
            if step % 2 == 0:
                loss = _autograd_loss(tgn, step, neg)
                loss.backward()
                assert tgn.beside.in_flight == tgn.beside.takes_step() == overlap
                opt.step()
                assert tgn.beside.in_flight == overlap and not tgn.beside.takes_step()
            else:
                tgn.train()
                emb, b = tgn.embed_device(t(d.sources[s:s + B], np.int32), t(d.destinations[s:s + B], np.int32), [t(neg, np.int32)], [Q],
                                          t(d.timestamps[s:s + B], np.float64), t(d.edge_idxs[s:s + B], np.int32), K)
                loss = P.bpr_step(tgn, emb, b, Q)
                awaited = tgn.beside.event
                assert (awaited is not None) == overlap and not tgn.beside.takes_step()
                opt.step()
                assert not tgn.beside.in_flight and tgn.beside.event is awaited        # (it ran on the caller's stream)
            losses.append(loss.item())
            tgn.memory.detach_memory()
        return (losses,) + _final(tgn)

    l0, p0, m0 = run(False)
    l1, p1, m1 = run(True)
    assert l0 == l1 and np.array_equal(p0, p1) and np.array_equal(m0, m1)
    assert np.isfinite(p1).all() and np.isfinite(l1).all()


def test_a_backward_in_flight_keeps_its_workspace_until_its_home_stream_has_waited():
    """One overlapped training step, then - before anything joins - an evaluation forward large enough to miss the workspace
    pool (48 interactions x 60 negatives: 2 976 roots against the step's 240).  The pool drops the step's workspace when it
    allocates the larger one; the backward still in flight must hold it until the caller's stream waits (inside that forward)."""
    d = _graph().data
    neg_eval = np.random.RandomState(5).randint(301, 326, size=B * 60)

    def run(overlap):
        tgn, opt = _model("fused", overlap)
        opt.zero_grad()
        loss = _autograd_loss(tgn, 0, np.random.RandomState(3).randint(301, 326, size=B * Q))
        ws = tgn._last_ws[1]
        held = lambda: any(x is ws for h in tgn.beside.hold for x in h)
        loss.backward()
        assert held() == overlap and any(w is ws for _, w in tgn._ws_pool)
        opt.step()
        assert held() == overlap and tgn.beside.in_flight == overlap
        with torch.no_grad():
            tgn.eval()
            ev = torch.cat(tgn.compute_temporal_embeddings(d.sources[2500:2500 + B], d.destinations[2500:2500 + B], neg_eval,
                                                           d.timestamps[2500:2500 + B], d.edge_idxs[2500:2500 + B], K))
        assert tgn._last_ws[1] is not ws and all(w is not ws for _, w in tgn._ws_pool)      # the pool let it go ...
        assert tgn.beside.hold == [] and not tgn.beside.in_flight                          # ... and so has the joined backward
        ev = ev.cpu().numpy()
        return (ev,) + _final(tgn)

    e0, p0, m0 = run(False)
    e1, p1, m1 = run(True)
    assert np.array_equal(e0, e1) and np.array_equal(p0, p1) and np.array_equal(m0, m1)
    assert e1.shape == (B * 62, 64) and np.isfinite(e1).all() and np.abs(e1).max() > 0


@pytest.mark.parametrize("kind", ["fused", "torch"])
def test_accumulated_backwards_beside_take_one_step_there_and_the_next_one_serially(kind):
    """Gradient accumulation: two forwards outstanding, two backwards beside the loop, one ``opt.step()`` - on the backward
    stream (the awaited event moves behind it); a second ``opt.step()`` right after finds nothing new there and runs on the
    caller's stream.  Parameters bit-identical to the serial order."""
    def run(overlap):
        tgn, opt = _model(kind, overlap)
        rs = np.random.RandomState(3)
        opt.zero_grad()
        losses = [_autograd_loss(tgn, step, rs.randint(301, 326, size=B * Q)) for step in range(2)]
        for loss in losses:
            loss.backward()
        behind_backward = tgn.beside.event
        assert tgn.beside.takes_step() == overlap and len(tgn.beside.hold) == (2 if overlap else 0)
        opt.step()
        behind_step = tgn.beside.event
        assert tgn.beside.in_flight == overlap and (behind_step is not behind_backward) == overlap
        opt.step()
        assert tgn.beside.event is behind_step and not tgn.beside.in_flight and not tgn.beside.takes_step()
        return ([x.item() for x in losses],) + _final(tgn)

    l0, p0, m0 = run(False)
    l1, p1, m1 = run(True)
    assert l0 == l1 and np.array_equal(p0, p1) and np.array_equal(m0, m1)
    assert np.isfinite(p1).all()
