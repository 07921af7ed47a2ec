"""Round-6 GPU tests: the two forms of the attention forward (register form, LDS key ring) against each
other and the oracle at ragged shapes, the optimizer step that clears the gradients it read, the shader-clock stamps."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

if has_gpu():
    import pfotgnrec_amd as P
    from pfotgnrec_amd import _lib
    DEV = torch.device("cuda:0")

RTOL_EMB = 1e-4            # north_star: embeddings within 1e-4 relative (max-norm: max|a - b| / max|b|)


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


_FWD_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[2])
import pfotgnrec_amd as P
from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
D, H, K, L, B, Ef = [int(x) for x in sys.argv[3:9]]
seed = int(sys.argv[9]) if len(sys.argv) > 9 else 11
with_oracle = len(sys.argv) > 10 and sys.argv[10] == "oracle"    # also save the oracle's smallest and largest |fc1 pre-activation| per step
cfg = SyntheticConfig("f6", 400, 30, 8000, D, L, K, H, edge_dim=Ef) if Ef != 4 else SyntheticConfig("f6", 400, 30, 8000, D, L, K, H)
g = make_graph(cfg, with_prices=False)
d = g.data
torch.manual_seed(seed)
tgn = P.TGN(P.get_neighbor_finder(d, False), g.node_features, g.edge_features, torch.device("cuda:0"), n_layers=L, n_heads=H,
            dropout=0.0, use_memory=True, memory_dimension=D, message_function="identity", n_neighbors=K)
tgn.deterministic = True
rs = np.random.RandomState(2)
out = {}
ref = None
if with_oracle:
    from oracle import tgn_oracle as T
    from oracle.neighbor_finder import OracleNeighborFinder, build_adjacency
    sd = {k: v.detach().cpu().numpy() for k, v in tgn.state_dict().items() if "layer_norm" not in k and not k.startswith("memory.")}
    ref = T.OracleTGN(OracleNeighborFinder(*build_adjacency(d.sources, d.destinations, d.edge_idxs, d.timestamps)), g.node_features,
                      g.edge_features, sd, L, H, True)
    def z1_range(c, acc):
        if c[0] != "leaf":
            acc.append((np.abs(c[4]["z1"]).min(), np.abs(c[4]["z1"]).max()))
            z1_range(c[2], acc); z1_range(c[3], acc)
        return acc
for step in range(2):
    s = 300 + step * 3000                     # early in the timeline: many instances with fewer than K (or no) neighbours
    neg = rs.randint(cfg.n_users + 1, cfg.n_users + cfg.n_items + 1, size=B * 3)
    tgn.train()
    emb = torch.cat(tgn.compute_temporal_embeddings(d.sources[s:s + B], d.destinations[s:s + B], neg, d.timestamps[s:s + B],
                                                    d.edge_idxs[s:s + B], K))
    P.bpr_loss(emb, B, 3).backward()
    if ref is not None:
        ref.compute_temporal_embeddings(d.sources[s:s + B], d.destinations[s:s + B], neg, d.timestamps[s:s + B], d.edge_idxs[s:s + B], K)
        acc = z1_range(ref._ctx, [])
        out["z1_%d" % step] = np.array([min(a for a, _ in acc), max(b for _, b in acc)])
    out["emb%d" % step] = emb.detach().cpu().numpy()
    out["grad%d" % step] = tgn.flat_grad.detach().cpu().numpy().copy()
    for p in tgn.parameters():
        p.grad = None
np.savez(sys.argv[1], **out)
"""


_FORMS_EF4 = [(172, 2, 20, 2, 96), (64, 4, 7, 2, 40), (32, 1, 10, 1, 64), (172, 4, 20, 2, 24), (256, 2, 5, 1, 16)]     # (ids as before Ef was a parameter)
# shapes only another Ef sends to the ring (attn_fwd_ring_ok: D + Ef <= 64 ceil(D / 64)), with the parameter seed of each
_FORMS_EF = [(256, 2, 5, 2, 16, 0, 13), (124, 4, 7, 2, 40, 4, 11), (172, 4, 8, 2, 24, 12, 13), (64, 2, 8, 2, 40, 0, 11)]


@pytest.mark.parametrize("D,H,K,L,B,Ef,seed", [pytest.param(*r, 4, None, id="-".join(map(str, r))) for r in _FORMS_EF4]
                         + [pytest.param(*r, id="-".join(map(str, r[:6]))) for r in _FORMS_EF])
def test_attention_forward_forms_agree(tmp_path, D, H, K, L, B, Ef, seed):
    """The LDS key-ring forward (default; one LDS-DMA per key, [node | edge] columns as one vector, scores in log2 units with
    the scale folded into the query) and the round-5 register form (PFO_ATTN_FWD_RING=0) on the same two steps: embeddings
    within 1e-6 of each other (the
    forms differ only in rounding: pre-scaled query, exp2), gradients within 1e-5 (the backward reads ctx' / weights the
    forward wrote).  Shapes: C2's, four heads (NR H = 12: four wavefronts per SIMD), one column group, D = 256 (four groups),
    K < and > the ring; batches early in the timeline hold instances with 0 .. K neighbours (odd counts: the pair tail).
    With Ef = 4, D = 64 and D = 256 take the register form on both sides (D + Ef passes the ring's row): the rows with another Ef
    are the ones where the two runs differ in kernel at NR = 4 (256, 0), NR = 2 with four heads (124, 4), NR H = 12 with a wide
    edge block (172, 12) and a ring row that is all node columns (64, 0).
    Those rows carry a parameter seed chosen on the oracle alone: the two forwards are held to 1e-6 of each other, so a
    merger unit whose pre-activation lies within 1e-6 of zero may take the other ReLU branch in one of the two runs, and one
    flipped unit moves every gradient below it by ~1e-3 (seed 11 at (172, 4, 8, 2, 24, 12): |z1| = 1.5e-7 in layer 1, the ring
    run within 4e-6 of the oracle in every tensor, the register run 1e-3 - 2e-3 off in layer 1's and the time encoder's only).
    The oracle, run beside the ring child, must hold no such unit; the gradient bound is as it was."""
    res = {}
    for name, env in (("ring", {}), ("reg", {"PFO_ATTN_FWD_RING": "0"})):
        path = str(tmp_path / (name + ".npz"))
        extra = [] if seed is None else [str(seed)] + (["oracle"] if name == "ring" else [])
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", _FWD_CHILD, path, REPO, str(D), str(H), str(K), str(L), str(B), str(Ef)] + extra,
                           env=dict(os.environ, **env), capture_output=True)
        assert r.returncode == 0, (name, r.stderr.decode()[-2000:])
        res[name] = np.load(path)
    for k in [k for k in res["ring"].files if k.startswith("z1_")]:
        lo, hi = res["ring"][k]
        print("FIGURES forms %s %s: min |z1| %.3g, max |z1| %.3g" % ((D, H, K, L, B, Ef, seed), k, lo, hi))
        assert lo > 1e-6, (k, lo, hi)             # (pre-activations and embeddings are both O(1): hi is 1.7 - 2.9)
    for k in res["reg"].files:
        tol = 1e-6 if k.startswith("emb") else 2e-5
        assert relerr(res["ring"][k], res["reg"][k]) < tol, ("ring", k, relerr(res["ring"][k], res["reg"][k]))
    assert np.abs(res["ring"]["emb0"]).max() > 0 and np.isfinite(res["ring"]["grad1"]).all()


def test_optimizer_step_that_clears_the_gradients_equals_the_plain_one():
    """FusedAdam(zero_grads_in_step=True): the side-stream optimizer kernel of bpr_step(..., optimizer=) writes zeros behind the
    gradients it read, and the next native backward runs without clearing the flat buffer first.  Four steps bit-identical
    to the plain order (deterministic backward), .grad reads zero after such a step, and a step whose ranges do not cover the
    buffer (the GRU tensors without a gradient: first batch, no pending message) falls back to the plain kernel."""
    from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
    cfg = SyntheticConfig("z6", 300, 25, 6000, 64, 2, 8, 2)
    g = make_graph(cfg, with_prices=False)
    d = g.data
    B, K = 48, 8
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)

    def run(zero_in_step):
        torch.manual_seed(9)
        tgn = P.TGN(P.get_neighbor_finder(d, False), g.node_features, g.edge_features, DEV, n_layers=2, n_heads=2, dropout=0.0,
                    use_memory=True, memory_dimension=64, message_function="identity", n_neighbors=K)
        tgn.deterministic = True
        opt = P.FusedAdam(tgn, lr=1e-3, zero_grads_in_step=zero_in_step)
        rs = np.random.RandomState(1)
        tgn.train()
        zero_seen = []
        for step in range(4):
            s = 2500 + step * B
            neg = t(rs.randint(301, 326, size=B * 3), np.int32)
            emb, b = tgn.embed_device(t(d.sources[s:s + B], np.int32), t(d.destinations[s:s + B], np.int32), [neg], [3],
                                      t(d.timestamps[s:s + B], np.float64), t(d.edge_idxs[s:s + B], np.int32), K)
            P.bpr_step(tgn, emb, b, 3, optimizer=opt)
            tgn.join()
            zero_seen.append(bool((tgn.flat_grad == 0).all()))
            opt.zero_grad(set_to_none=True)
        tgn.join()
        torch.cuda.synchronize()
        return tgn.flat_parameters.detach().cpu().numpy().copy(), tgn.memory.memory.detach().cpu().numpy().copy(), zero_seen

    p0, m0, z0 = run(False)
    p1, m1, z1 = run(True)
    assert np.array_equal(p0, p1) and np.array_equal(m0, m1)
    assert not any(z0)                       # the plain step leaves the gradients in place
    assert all(z1[1:])                       # (step 0: no pending messages -> the GRU tensors have no gradient -> plain kernel)
    assert np.isfinite(p1).all()


def test_shader_clock_stamps_read_a_plausible_clock():
    """pfo_shader_clock: the first wavefront of the attention forward / run-merged backward / grouped weight-gradient kernel stamps
    s_memtime against the 100 MHz counter on every launch.  After two C2-shaped steps every ratio lies in (0.5, 3.0) GHz and a
    reset clears the sums."""
    from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
    cfg = SyntheticConfig("c6", 3000, 60, 60000, 172, 2, 20, 2)
    g = make_graph(cfg, with_prices=False)
    d = g.data
    B = 256
    tgn = P.TGN(P.get_neighbor_finder(d, False), g.node_features, g.edge_features, DEV, n_layers=2, n_heads=2, dropout=0.0,
                use_memory=True, memory_dimension=172, message_function="identity", n_neighbors=20)
    rs = np.random.RandomState(0)
    _lib.shader_clock(reset=True)
    tgn.train()
    for step in range(2):
        s = 40000 + step * B
        neg = rs.randint(cfg.n_users + 1, cfg.n_users + cfg.n_items + 1, size=B * 3)
        emb = torch.cat(tgn.compute_temporal_embeddings(d.sources[s:s + B], d.destinations[s:s + B], neg, d.timestamps[s:s + B],
                                                        d.edge_idxs[s:s + B], 20))
        P.bpr_loss(emb, B, 3).backward()
        for p in tgn.parameters():
            p.grad = None
    torch.cuda.synchronize()
    clk = _lib.shader_clock(reset=True)
    assert set(clk) == {"attn_fwd", "attn_bwd_runs", "gemm_tn_bx"}
    for k, v in clk.items():
        assert 0.5 < v < 3.0, (k, v)
    torch.cuda.synchronize()
    assert all(v == 0.0 for v in _lib.shader_clock().values())


def test_entry_point_blocks_are_outputs_of_one_node_and_the_native_bpr_expression_matches_torch():
    """compute_temporal_embeddings hands out (source, destination, negative) as three OUTPUTS of the native node: the gradient the
    TGN backward receives is one concatenation of the three incoming blocks, bit-identical to what autograd assembled from
    three slices of one output (zero matrices + adds); pfotgnrec_amd.bpr_loss_blocks (one native launch) against the reference's
    torch expression (main.py:364-381) on the same blocks: loss within 1e-6, parameter gradients within 1e-5 - and its gradient
    blocks reach the backward as ONE matrix without a copy."""
    from pfotgnrec_amd.functional import adjacent_rows
    from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
    cfg = SyntheticConfig("b6", 300, 25, 6000, 64, 2, 8, 2)
    g = make_graph(cfg, with_prices=False)
    d = g.data
    B, K, q = 40, 8, 3
    s = 2500
    rs = np.random.RandomState(4)
    neg = rs.randint(301, 326, size=B * q)

    def torch_expression(se, de, ne):
        se, de, ne = se.view(B, 1, -1), de.view(B, 1, -1), ne.view(B, q, -1)
        pos = torch.sum(se * de, dim=2)
        ngs = torch.matmul(se, ne.transpose(1, 2)).squeeze()
        return -torch.mean(torch.log(torch.sigmoid(torch.mean(pos - ngs, dim=1))))

    def run(kind):
        torch.manual_seed(5)
        tgn = P.TGN(P.get_neighbor_finder(d, False), g.node_features, g.edge_features, DEV, n_layers=2, n_heads=2, dropout=0.0,
                    use_memory=True, memory_dimension=64, message_function="identity", n_neighbors=K)
        tgn.deterministic = True
        tgn.train()
        out = None
        for step in range(2):                                       # (second step: pending messages, the GRU has a gradient)
            a = s + step * B
            args = (d.sources[a:a + B], d.destinations[a:a + B], neg, d.timestamps[a:a + B], d.edge_idxs[a:a + B], K)
            if kind == "slices":
                t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(DEV)
                emb, b = tgn.embed_device(t(args[0], np.int32), t(args[1], np.int32), [t(neg, np.int32)], [q], t(args[3], np.float64),
                                          t(args[4], np.int32), K)
                blocks = (emb[:b], emb[b:2 * b], emb[2 * b:])
            else:
                blocks = tgn.compute_temporal_embeddings(*args)
                assert adjacent_rows(blocks) is not None and blocks[0].grad_fn is blocks[2].grad_fn
            loss = P.bpr_loss_blocks(*blocks) if kind == "native" else torch_expression(*blocks)
            loss.backward()
            out = (float(loss), tgn.flat_grad.detach().cpu().numpy().copy(), torch.cat(blocks).detach().cpu().numpy())
            for p in tgn.parameters():
                p.grad = None
        return out

    l_blocks, g_blocks, e_blocks = run("blocks")
    l_slices, g_slices, e_slices = run("slices")
    l_native, g_native, e_native = run("native")
    assert np.array_equal(e_blocks, e_slices) and np.array_equal(e_blocks, e_native)
    assert l_blocks == l_slices and np.array_equal(g_blocks, g_slices)
    assert abs(l_native - l_blocks) < 1e-6 * max(1.0, abs(l_blocks))
    assert relerr(g_native, g_blocks) < 1e-5 and np.abs(g_blocks).max() > 0


@pytest.mark.parametrize("kind", ["fused", "torch"])
def test_backward_beside_the_host_loop_equals_the_serial_order(kind):
    """FusedAdam(tgn, overlap_backward=True) - and pfotgnrec_amd.overlap_backward(tgn, torch.optim.Adam(...)), whose step() is
    wrapped to run behind the backward on its stream - on the reference's loop (main.py:160-394 in shape: numpy batches, torch BPR
    expression, loss.backward(), optimizer.step(), loss.item(), optimizer.zero_grad()): the native backward and the optimizer's
    kernel run on a stream of their own and the next forward waits for them.  Five steps bit-identical (losses, parameters,
    memory) to the serial order with the deterministic backward; ``tgn.join()`` makes gradients readable; a validation forward
    and ``state_dict()`` in between see the stepped parameters."""
    from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
    cfg = SyntheticConfig("o6", 300, 25, 6000, 64, 2, 8, 2)
    g = make_graph(cfg, with_prices=False)
    d = g.data
    B, K, q = 48, 8, 3

    def run(overlap):
        torch.manual_seed(21)
        tgn = P.TGN(P.get_neighbor_finder(d, False), g.node_features, g.edge_features, DEV, n_layers=2, n_heads=2, dropout=0.0,
                    use_memory=True, memory_dimension=64, message_function="identity", n_neighbors=K)
        tgn.deterministic = True
        if kind == "fused":
            opt = P.FusedAdam(tgn, lr=1e-3, overlap_backward=overlap)
        else:
            opt = torch.optim.Adam(tgn.parameters(), lr=1e-3)
            if overlap:
                assert P.overlap_backward(tgn, opt) is opt and P.overlap_backward(tgn, opt) is opt      # (idempotent)
        rs = np.random.RandomState(3)
        losses, extra = [], []
        for step in range(5):
            s = 2500 + step * B
            opt.zero_grad()
            neg = rs.randint(301, 326, size=B * q)
            tgn = tgn.train()
            se, de, ne = tgn.compute_temporal_embeddings(d.sources[s:s + B], d.destinations[s:s + B], neg, d.timestamps[s:s + B],
                                                          d.edge_idxs[s:s + B], K)
            se, de, ne = se.view(B, 1, -1), de.view(B, 1, -1), ne.view(B, q, -1)
            pos = torch.sum(se * de, dim=2)
            ngs = torch.matmul(se, ne.transpose(1, 2)).squeeze()
            loss = -torch.mean(torch.log(torch.sigmoid(torch.mean(pos - ngs, dim=1))))
            loss.backward()
            if overlap and step == 1:
                assert tgn.beside.in_flight                          # in flight: nothing on this stream waits for it yet
            opt.step()
            losses.append(loss.item())
            tgn.memory.detach_memory()
            if step == 2:                                            # a checkpoint and a validation forward between two steps
                sd = tgn.state_dict()
                extra.append(sd[sorted(k for k in sd if k.endswith("weight"))[0]].detach().cpu().numpy().copy())
                with torch.no_grad():
                    tgn.eval()
                    bak = tgn.memory.backup_memory()
                    ev = torch.cat(tgn.compute_temporal_embeddings(d.sources[100:120], d.destinations[100:120], neg[:60],
                                                                   d.timestamps[100:120], d.edge_idxs[100:120], K))
                    tgn.memory.restore_memory(bak)
                    extra.append(ev.cpu().numpy())
            if step == 3:
                tgn.join()
                extra.append(tgn.flat_grad.detach().cpu().numpy().copy())
        tgn.join()
        torch.cuda.synchronize()
        return losses, tgn.flat_parameters.detach().cpu().numpy().copy(), tgn.memory.memory.detach().cpu().numpy().copy(), extra

    l0, p0, m0, e0 = run(False)
    l1, p1, m1, e1 = run(True)
    assert l0 == l1
    assert np.array_equal(p0, p1) and np.array_equal(m0, m1)
    for a, b in zip(e0, e1):
        assert np.array_equal(a, b)
    assert np.isfinite(p1).all() and np.abs(e1[2]).max() > 0


def test_ours_branch_with_native_bpr_blocks_and_backward_overlap():
    """The ``ours`` branch of the loop (main.py:190-337 in shape): compute_temporal_embeddings_p with one p_pos and three p_neg per
    interaction, the BPR expression over (source, p_pos, p_neg) - once as the reference's torch expression in the serial order,
    once as pfotgnrec_amd.bpr_loss_blocks(..., p_pos_embedding=) under FusedAdam(overlap_backward=True).  Four free-running
    steps: step 0's loss and gradient are compared (identical state: 1e-6 / 1e-5), the parameters after four steps stay
    within the optimizer's reach of each other, every workspace is handed back and state_dict() joins the last step."""
    from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
    cfg = SyntheticConfig("p6", 300, 25, 6000, 64, 2, 8, 2)
    g = make_graph(cfg, with_prices=False)
    d = g.data
    B, K = 32, 8
    rs = np.random.RandomState(8)
    ppos = rs.randint(301, 326, size=(4, B * 1))
    pneg = rs.randint(301, 326, size=(4, B * 3))

    def run(native):
        torch.manual_seed(31)
        tgn = P.TGN(P.get_neighbor_finder(d, False), g.node_features, g.edge_features, DEV, n_layers=2, n_heads=2, dropout=0.0,
                    use_memory=True, memory_dimension=64, message_function="identity", n_neighbors=K)
        tgn.deterministic = True
        opt = P.FusedAdam(tgn, lr=1e-3, overlap_backward=native)
        first = None
        for step in range(4):
            s = 2500 + step * B
            opt.zero_grad()
            tgn = tgn.train()
            se, de, pe, ne = tgn.compute_temporal_embeddings_p(d.sources[s:s + B], d.destinations[s:s + B], ppos[step], pneg[step],
                                                                d.timestamps[s:s + B], d.edge_idxs[s:s + B], K)
            if native:
                loss = P.bpr_loss_blocks(se, de, ne, p_pos_embedding=pe)
            else:
                sv, pv, nv = se.view(B, 1, -1), pe.view(B, 1, -1), ne.view(B, 3, -1)
                pos = torch.sum(sv * pv, dim=2)
                ngs = torch.matmul(sv, nv.transpose(1, 2)).squeeze()
                loss = -torch.mean(torch.log(torch.sigmoid(torch.mean(pos - ngs, dim=1))))
            loss.backward()
            if step == 0:
                tgn.join()
                first = (float(loss), tgn.flat_grad.detach().cpu().numpy().copy())
            opt.step()
            loss.item()
            tgn.memory.detach_memory()
        sd = tgn.state_dict()
        torch.cuda.synchronize()
        assert len(tgn._ws_pool) >= 1 and all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
        return first, tgn.flat_parameters.detach().cpu().numpy().copy()

    (l0, g0), p0 = run(False)
    (l1, g1), p1 = run(True)
    assert abs(l0 - l1) < 1e-6 * max(1.0, abs(l0))
    assert relerr(g1, g0) < 1e-5 and np.abs(g0).max() > 0
    # four Adam steps of lr 1e-3 from rounding-level different gradients: a parameter whose gradient is noise moves +-lr per
    # step either way (SURVEY 7 hard part 5) - the bound is the optimizer's reach, not a parity bar
    assert np.abs(p1 - p0).max() <= 4 * 2 * 1e-3 * 1.01 and np.isfinite(p1).all()


# ------------------------------------------------------------------ eval dedup on yyyymmddHHMMSS timestamps
def _real_timestamps(n, rs, n_days=60, n_dup=0):
    """Sorted f64 ``yyyymmddHHMMSS`` timestamps (the recipe of the g10 fixtures, restated): 2023-12-01 onwards, 09:00:00 to
    15:30:00, ``n_dup`` exact duplicates.  Near 2.02e13 one f32 step is 2**21 - about two calendar days."""
    import datetime
    d0 = datetime.date(2023, 12, 1)
    days = np.array([int((d0 + datetime.timedelta(int(k))).strftime("%Y%m%d")) for k in range(n_days)], np.int64)
    sec = rs.randint(9 * 3600, 15 * 3600 + 30 * 60 + 1, n)
    hms = (sec // 3600) * 10000 + (sec // 60 % 60) * 100 + sec % 60
    ts = (days[rs.randint(0, n_days, n)] * 1_000_000 + hms).astype(np.float64)
    dup = rs.choice(n, n_dup, replace=False)
    ts[dup] = ts[rs.randint(0, n, n_dup)]
    return np.sort(ts)


def test_eval_dedup_keeps_roots_apart_that_differ_in_f64_and_collapse_in_f32():
    """The forward-only dedup (R >= 4096) embeds each distinct (node, time) root once.  With real timestamps most roots of
    one item fall into one f32 step while their f64 times - and the histories in front of them - differ: the grid must be
    built from the f64 times.  One evaluation batch of 180 interactions x all 25 items against the oracle, every row."""
    from oracle import tgn_oracle as T
    from oracle.neighbor_finder import OracleNeighborFinder, build_adjacency
    from parity import row_relerr, ROW_RTOL
    torch.manual_seed(5)
    rs = np.random.RandomState(21)
    U, I, E, D, K, L, H, B = 300, 25, 5000, 32, 6, 2, 2, 180
    src, dst = rs.randint(1, U + 1, E), rs.randint(U + 1, U + I + 1, E)
    ts = _real_timestamps(E, rs, n_dup=E // 3)
    eidx = np.arange(1, E + 1)
    node_feat, edge_feat = rs.rand(U + I + 1, D), rs.randn(E + 1, 4)
    edge_feat[0] = 0
    nf = P.NeighborFinder.from_arrays(src, dst, eidx, ts, max_node_idx=U + I)
    tgn = P.TGN(nf, node_feat, edge_feat, DEV, n_layers=L, n_heads=H, dropout=0.2, use_memory=True, memory_dimension=D,
                message_function="identity", n_neighbors=K)
    with torch.no_grad():
        tgn.time_encoder.w.bias.normal_(0, 0.3)
    onf = OracleNeighborFinder(*build_adjacency(src, dst, eidx, ts, max_node_idx=U + I))
    names = [k for k in tgn.state_dict() if "layer_norm" not in k and not k.startswith("memory.")]
    ref = T.OracleTGN(onf, node_feat, edge_feat, {k: tgn.state_dict()[k].cpu().numpy() for k in names}, L, H, True)
    sl = slice(3000, 3000 + B)
    items = np.arange(U + 1, U + I + 1)
    neg = np.tile(items, B)                                                 # R = 180 * 27 = 4860 roots
    taken = []
    dedup = tgn._dedup_roots

    def spy(*a, **k):
        r = dedup(*a, **k)
        taken.append((r[2] is not None, int(r[0].shape[0])))
        return r
    tgn._dedup_roots = spy
    tgn.eval()
    res = []
    for flag in (True, False):
        tgn.eval_dedup = flag
        tgn.memory.__init_memory__()
        with torch.no_grad():
            for warm in (2800, 2900):
                w = slice(warm, warm + 100)
                tgn.compute_temporal_embeddings(src[w], dst[w], dst[w].repeat(3), ts[w], eidx[w], K)
            res.append(torch.cat(tgn.compute_temporal_embeddings(src[sl], dst[sl], neg, ts[sl], eidx[sl], K)).cpu().numpy())
    assert taken == [(True, taken[0][1])] and taken[0][1] < B * (2 + I)    # the dedup ran once, on the big batch, and saved roots
    assert res[0].shape[0] == B * (2 + I) >= 4096 and np.array_equal(res[0], res[1])
    for warm in (2800, 2900):
        w = slice(warm, warm + 100)
        ref.compute_temporal_embeddings(src[w], dst[w], dst[w].repeat(3), ts[w], eidx[w], K)
    remb = np.concatenate(ref.compute_temporal_embeddings(src[sl], dst[sl], neg, ts[sl], eidx[sl], K))
    # pairs of roots on ONE item whose times differ in f64 and are equal in f32 - and whose embeddings differ by far more than
    # the bar (an edge of the item lies between the two times): a grid keyed on f32 times would hand both the same row
    tb = ts[sl]
    t32 = tb.astype(np.float32)
    n_pairs = n_apart = 0
    for a in range(B - 1):
        b = a + 1
        if tb[a] != tb[b] and t32[a] == t32[b]:
            ra, rb = remb[2 * B + a * I:2 * B + (a + 1) * I], remb[2 * B + b * I:2 * B + (b + 1) * I]
            n_pairs += I
            n_apart += int((np.abs(ra - rb).max(1) > 100 * RTOL_EMB * np.abs(remb).max()).sum())
    assert n_pairs >= 25 * 50 and n_apart >= 50, (n_pairs, n_apart)
    e, er = relerr(res[0], remb), row_relerr(res[0], remb)
    print("FIGURES eval dedup on real timestamps: relerr %.3g row_relerr %.3g, %d f32-collapsing pairs, %d apart" % (e, er, n_pairs, n_apart))
    assert e < RTOL_EMB, e
    assert er < ROW_RTOL, er
    assert relerr(tgn.memory.memory.cpu().numpy(), ref.memory) < RTOL_EMB
    assert row_relerr(tgn.memory.memory.cpu().numpy(), ref.memory) < ROW_RTOL
    assert np.array_equal(tgn.memory.last_update.cpu().numpy(), ref.last_update)
