"""The training step, observe, the serving paths, deterministic mode, graph capture and data parallelism with
message_function="mlp": against the reference's own steps (g11) and against the host model of tests/message_ref.py."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import REPO, load_golden, has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

import pfotgnrec_amd as P
from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
from oracle import tgn_oracle as T
from oracle.neighbor_finder import OracleNeighborFinder, build_adjacency
from parity import (relerr, row_relerr, ROW_RTOL, RTOL_EMB, RTOL_GRAD_TIME, RTOL_GRAD_ORACLE_L2, KINK_THR, _near_kink_roots,
                    _relu_sign_disagreements, grad_blocks, block_errors, grad_block_bar, fmt_worst_block)
import message_ref as MR
import observe_ref as O

DEV = "cuda:0"
RTOL_GRAD = 5e-4     # parameter gradients against the reference's (test_gpu_tgn_step.py)


def _params_of(tgn):
    return {k: v.detach().cpu().numpy().copy() for k, v in tgn.state_dict().items()
            if "layer_norm" not in k and not k.startswith("memory.") and not k.startswith(MR.ALIAS)}


def _tables(tgn):
    m = tgn.memory
    torch.cuda.synchronize()
    return tuple(t.detach().cpu().numpy().copy() for t in (m.memory, m.last_update, m.msg_table, m.msg_time, m.has_msg))


def _set_tables(tgn, tables):
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


def _inject(tgn, g, pre):
    sd = tgn.state_dict()
    with torch.no_grad():
        for k in g.files:
            if k.startswith(pre + "sd_") and k[len(pre + "sd_"):] in sd:
                sd[k[len(pre + "sd_"):]].copy_(torch.from_numpy(g[k]))
    _set_tables(tgn, (g[pre + "sd_memory.memory"], g[pre + "sd_memory.last_update"], g[pre + "msg_tab"], g[pre + "msg_t"], g[pre + "msg_cnt"] > 0))


def _golden_model(g):
    nf = P.NeighborFinder.from_arrays(g["src_all"], g["dst_all"], g["eidx_all"], g["ts_all"], uniform=False)
    D = g["node_features"].shape[1]
    return P.TGN(nf, g["node_features"], g["edge_features"], DEV, n_layers=int(g["L"]), n_heads=int(g["H"]), dropout=0.0,
                 use_memory=True, memory_dimension=D, message_function="mlp", message_dimension=100, n_neighbors=int(g["K"]))


def _mlp_views(tgn):
    """(touched node ids, hidden activations, MLP output) of the newest forward, read through the step's debug views."""
    ids, hid, out = tgn.debug_message_mlp()
    return ids.cpu().numpy().astype(np.int64), hid.cpu().numpy(), out.cpu().numpy()


# ---------------------------------------------------------------------------------------------- the reference's own steps
@pytest.mark.parametrize("fixture", ["g11_step_L1_mem_mlp", "g11_step_L2_mem_mlp"])
def test_step_against_reference_golden(fixture):
    g = load_golden(fixture)
    K = int(g["K"])
    tgn = _golden_model(g)
    opt = P.FusedAdam(tgn, lr=float(g["lr"]))
    worst = {}

    def note(key, e):
        worst[key] = max(worst.get(key, 0.0), float(e))
        return e
    for step in g["recorded_steps"]:
        pre = "s%d_" % step
        _inject(tgn, g, pre)
        sb, db, tb, eb, neg = g[pre + "src"], g[pre + "dst"], g[pre + "ts"], g[pre + "eidx"], g[pre + "neg"]
        B = len(sb)
        tgn.train()
        opt.zero_grad()
        se, de, ne = tgn.compute_temporal_embeddings(sb, db, neg.flatten(), tb, eb, K)
        emb = torch.cat([se, de, ne])
        for got, key in ((se, "emb_src"), (de, "emb_dst"), (ne, "emb_neg")):
            assert note("emb relerr", relerr(got.detach().cpu().numpy(), g[pre + key])) < RTOL_EMB, (step, key)
            assert note("emb row_relerr", row_relerr(got.detach().cpu().numpy(), g[pre + key])) < ROW_RTOL, (step, key)
        loss = P.bpr_loss(emb, B, 3)
        assert abs(float(loss) - float(g[pre + "loss"])) < 1e-5 * max(1.0, abs(float(g[pre + "loss"])))
        loss.backward()
        names = dict(tgn.named_parameters())
        for k in g.files:
            if not k.startswith(pre + "grad_"):
                continue
            name = k[len(pre + "grad_"):]
            if "layer_norm" in name or name.startswith("memory."):
                continue
            ref = g[k]
            got = names[name].grad.cpu().numpy()
            if np.abs(ref).max() < 1e-7:
                assert np.abs(got).max() < 1e-6, name
                continue
            e = note("time grad relerr" if name.startswith("time_encoder") else ("mlp grad relerr" if name.startswith("message_function") else "grad relerr"),
                     relerr(got, ref))
            assert e < (RTOL_GRAD_TIME if name.startswith("time_encoder") else RTOL_GRAD), (step, name, e)
        mem = tgn.memory.memory.cpu().numpy()
        assert note("memory relerr", relerr(mem, g[pre + "after_memory"])) < RTOL_EMB
        assert note("memory row_relerr", row_relerr(mem, g[pre + "after_memory"])) < ROW_RTOL
        assert np.array_equal(tgn.memory.last_update.cpu().numpy(), g[pre + "after_last_update"])
        has = g[pre + "after_msg_cnt"] > 0
        assert np.array_equal(tgn.memory.has_msg.cpu().numpy() > 0, has)
        tab = tgn.memory.msg_table.cpu().numpy()[has]
        assert note("msg relerr", relerr(tab, g[pre + "after_msg_tab"][has])) < RTOL_EMB
        assert np.array_equal(tgn.memory.msg_time.cpu().numpy()[has], g[pre + "after_msg_t"][has])
        # Adam with the reference optimizer's moments injected (the bound of test_gpu_tgn_step.py, derived per element)
        opt._m = torch.zeros_like(tgn.flat_parameters)
        opt._v = torch.zeros_like(tgn.flat_parameters)
        views = {p_: (off, n) for p_, off, n, _ in tgn._views}
        grads_now = {}
        for name, p_ in names.items():
            if p_ not in views or (pre + "adam_m_" + name) not in g.files:
                continue
            off, n = views[p_]
            opt._m[off:off + n] = torch.from_numpy(g[pre + "adam_m_" + name].ravel()).to(DEV)
            opt._v[off:off + n] = torch.from_numpy(g[pre + "adam_v_" + name].ravel()).to(DEV)
            grads_now[name] = p_.grad.detach().cpu().numpy().astype(np.float64)
            opt.set_steps({name: int(g[pre + "adam_t_" + name])})
        assert set(MR.MLP_NAMES) <= set(grads_now) and len(grads_now) >= 14
        # the MLP's tensors lag one step like the GRU's: neither module ran in step 0 (no pending message)
        assert int(g[pre + "adam_t_" + MR.MLP + "0.weight"]) == int(g[pre + "adam_t_time_encoder.w.weight"]) - 1
        opt.step()
        lr, b1, b2, eps = float(g["lr"]), 0.9, 0.999, 1e-8
        for name, gn in grads_now.items():
            t = int(g[pre + "adam_t_" + name]) + 1
            bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
            ref_after = g[pre + "after_" + name].astype(np.float64)
            got_after = names[name].detach().cpu().numpy().astype(np.float64)
            g_ref = g[pre + "grad_" + name].astype(np.float64)
            v_new = b2 * g[pre + "adam_v_" + name].astype(np.float64) + (1 - b2) * g_ref * g_ref
            bound = lr * (1 - b1) / bc1 * np.abs(gn - g_ref) / (np.sqrt(v_new / bc2) + eps)
            slack = 4e-7 * np.maximum(1.0, np.abs(ref_after)) + 2e-3 * lr
            assert np.all(np.abs(got_after - ref_after) <= 1.5 * bound + slack), (step, name, float(np.abs(got_after - ref_after).max()))
            m_new = b1 * g[pre + "adam_m_" + name].astype(np.float64) + (1 - b1) * gn
            v_mine = b2 * g[pre + "adam_v_" + name].astype(np.float64) + (1 - b2) * gn * gn
            want = g[pre + "sd_" + name].astype(np.float64) - lr / bc1 * m_new / (np.sqrt(v_mine / bc2) + eps)
            assert np.abs(got_after - want).max() <= 4e-7 * max(1.0, np.abs(want).max()) + 1e-3 * lr, (step, name)
    print("FIGURES %s: %s" % (fixture, ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))


# ---------------------------------------------------------------------------------------------- the host model, random parameters
def _blocks_of(name, shape, D, Ef, H):
    """parity.grad_blocks, except that weight_ih is [3D, message_dimension] here: gate rows, all columns (the MLP's output has
    no column structure); the MLP's own tensors are one block each."""
    if name.endswith("weight_ih"):
        return [(g_, (slice(i * D, (i + 1) * D), slice(None))) for i, g_ in enumerate("rzn")]
    return grad_blocks(name, shape, D, Ef, H)


def _check_blocks(got, g32, g64, D, Ef, H):
    """parity.check_grad_blocks's rule with the blocks above: per tensor, bar = GRAD_MARGIN x max(e32, 2^-23), e32 = the fp32 host
    model's largest block error against its float64 twin."""
    worst, over = (0.0, None, None, 0.0, 0.0), []
    for name in sorted(got):
        blocks = _blocks_of(name, np.shape(g64[name]), D, Ef, H)
        e32, bar = grad_block_bar(g32[name], g64[name], blocks)
        assert np.isfinite(e32), (name, e32)
        for b, e in block_errors(got[name], g64[name], blocks).items():
            if not e <= bar:
                over.append((name, b, e, e32, bar))
            if not e / bar <= worst[0]:
                worst = (e / bar, name, b, e, e32)
    return worst, over


def _bpr_seed(se, de, ne, B, dtype):
    _, cache = T.bpr_loss(se, de.reshape(B, 1, -1), ne.reshape(B, 3, -1), dtype=dtype)
    ds, dp, dn = T.bpr_loss_backward(cache)
    return np.concatenate([ds, dp.reshape(B, -1), dn.reshape(3 * B, -1)])


@pytest.mark.parametrize("D,H,L,K", [(32, 2, 1, 10), (8, 2, 2, 4), (172, 2, 2, 8)])
def test_step_against_host_model(D, H, L, K):
    torch.manual_seed(100 + D)
    cfg = SyntheticConfig("t", 300, 25, 5000, D, L, K, H)
    g = make_graph(cfg, with_prices=False)
    d = g.data
    Ef = g.edge_features.shape[1]
    tgn = P.TGN(P.get_neighbor_finder(d, False), g.node_features, g.edge_features, DEV, n_layers=L, n_heads=H, dropout=0.0,
                use_memory=True, memory_dimension=D, message_function="mlp", message_dimension=100, n_neighbors=K)
    with torch.no_grad():
        tgn.time_encoder.w.bias.normal_(0, 0.3)
        for att in tgn.embedding_module.attention_models:
            att.multi_head_target.in_proj_bias.normal_(0, 0.1)
            att.multi_head_target.out_proj.bias.normal_(0, 0.1)
    opt = P.FusedAdam(tgn, lr=1e-3)
    onf = OracleNeighborFinder(*build_adjacency(d.sources, d.destinations, d.edge_idxs, d.timestamps))
    ref = MR.MlpOracleTGN(onf, g.node_features, g.edge_features, _params_of(tgn), L, H)
    ref64 = MR.f64_twin(ref)
    worst_block = (0.0, None, None, 0.0, 0.0)
    rs = np.random.RandomState(5)
    B = 40
    n_flipped = 0
    for step in range(3):
        s = 2500 + step * B
        sb, db, tb, eb = d.sources[s:s + B], d.destinations[s:s + B], d.timestamps[s:s + B], d.edge_idxs[s:s + B]
        neg = rs.randint(cfg.n_users + 1, cfg.n_users + cfg.n_items + 1, size=B * 3)
        ref.P = _params_of(tgn)
        tgn.train(); opt.zero_grad()
        se, de, ne = tgn.compute_temporal_embeddings(sb, db, neg, tb, eb, K)
        ids_p, hid_p, out_p = _mlp_views(tgn)                            # (before the backward hands the workspace back)
        ref64.load_state(ref)
        e64 = ref64.compute_temporal_embeddings(sb, db, neg, tb, eb, K)
        rse, rde, rne = ref.compute_temporal_embeddings(sb, db, neg, tb, eb, K)
        emb = torch.cat([se, de, ne])
        remb = np.concatenate([rse, rde, rne])
        assert relerr(emb.detach().cpu().numpy(), remb) < RTOL_EMB, (step, relerr(emb.detach().cpu().numpy(), remb))
        ids, pre_act, hid = ref.mlp_rows()
        # ---- the hidden layer's ReLU decisions: the product's mask, row for row of the host model's pending nodes
        mask = None
        if len(ids) > 0:
            pos = {int(v): i for i, v in enumerate(ids_p)}
            touched = np.array([int(v) in pos for v in ids])
            assert touched.sum() > 0
            rows = np.array([pos[int(v)] for v in ids[touched]])
            mask = pre_act > 0                                            # pending nodes the step did not touch: the host's own
            mask_p = hid_p[rows] > 0
            differ = mask_p != mask[touched]
            assert (np.abs(pre_act[touched][differ]) < KINK_THR).all(), "a ReLU decision differs away from the kink"
            n_flipped += int(differ.sum())
            assert relerr(hid_p[rows], hid[touched]) < RTOL_EMB
            x64 = ref64._gru_ctx[1][0]
            assert relerr(out_p[rows], x64[touched]) < RTOL_EMB
            mask[touched] = mask_p
        # ---- backward on all sides from each side's own loss gradient, near-kink roots of the attention layers left out
        loss = P.bpr_loss(emb, B, 3)
        (d_emb,) = torch.autograd.grad(loss, emb, retain_graph=True)
        W = _bpr_seed(rse, rde, rne, B, np.float32).astype(np.float32)
        assert np.abs(d_emb.cpu().numpy() - W).max() <= 2e-5 * np.abs(W).max() + 1e-9
        R = W.shape[0]
        bad = _near_kink_roots(ref._ctx, R, K)
        assert bad.sum() < R // 2
        keep = torch.from_numpy((~bad).astype(np.float32)).to(emb.device)[:, None]
        emb.backward(d_emb * keep)
        W[bad] = 0
        rgrads = ref.backward(W, relu_mask=mask)
        W64 = _bpr_seed(*e64, B, np.float64)
        differ64 = _relu_sign_disagreements(ref._ctx, ref64._ctx, R, K)
        assert not (differ64 & ~bad).any()
        W64[bad] = 0
        g64 = ref64.backward(W64, relu_mask=mask)
        mine = {}
        for name, p in tgn.named_parameters():
            if name not in rgrads:
                continue
            r = rgrads[name].reshape(p.shape)
            if step == 0 and (name.startswith("message_function") or name.startswith(MR.GRU)):
                # no pending message anywhere: neither module ran, their gradients are None (as autograd leaves them) or exactly zero
                assert np.abs(r).max() == 0 and (p.grad is None or p.grad.abs().max().item() == 0.0), name
                continue
            if np.abs(r).max() < 1e-7:
                assert p.grad is None or p.grad.abs().max().item() < 1e-6, name
                continue
            got = p.grad.cpu().numpy().astype(np.float64)
            e = np.linalg.norm(got - r) / (np.linalg.norm(r) + 1e-30)
            assert e < (RTOL_GRAD_TIME if name.startswith("time_encoder") else RTOL_GRAD_ORACLE_L2), (step, name, e)
            mine[name] = got
        if step == 0:
            assert tgn.flat_grad[tgn._layout.mlp_w1:tgn._layout.layer[0].wq].abs().max().item() == 0.0
        else:
            assert set(MR.MLP_NAMES) <= set(mine)
        wb, over = _check_blocks(mine, rgrads, g64, D, Ef, H)
        worst_block = max(worst_block, wb, key=lambda w: w[0])
        if over:
            print("BLOCKS OVER THE BAR step %d: %s" % (step, "; ".join("%s[%s] %.3g e32 %.3g bar %.3g" % o for o in over)))
        assert not over, (step, over)
        assert relerr(tgn.memory.memory.cpu().numpy(), ref.memory) < RTOL_EMB
        assert np.array_equal(tgn.memory.last_update.cpu().numpy(), ref.last_update)
        tab, mt, has = ref.pending_table()
        assert np.array_equal(tgn.memory.has_msg.cpu().numpy() > 0, has)
        assert relerr(tgn.memory.msg_table.cpu().numpy()[has], tab[has]) < RTOL_EMB
        assert np.array_equal(tgn.memory.msg_time.cpu().numpy()[has], mt[has])
        opt.step()
    print("FIGURES mlp step_against_host_model (D %d H %d L %d K %d): %s, hidden units on the other side of the kink: %d" % (
        D, H, L, K, fmt_worst_block(worst_block), n_flipped))


# ---------------------------------------------------------------------------------------------- duplicates and B = 1
def test_duplicate_nodes_and_a_batch_of_one():
    """One node several times in a batch, as source and as destination, then a batch of one interaction."""
    torch.manual_seed(9)
    D, L, K, H = 16, 2, 4, 2
    cfg = SyntheticConfig("t", 60, 12, 1200, D, L, K, H)
    g = make_graph(cfg, with_prices=False)
    d = g.data
    tgn = P.TGN(P.get_neighbor_finder(d, False), g.node_features, g.edge_features, DEV, n_layers=L, n_heads=H, dropout=0.0,
                use_memory=True, memory_dimension=D, message_function="mlp", message_dimension=20, n_neighbors=K)
    onf = OracleNeighborFinder(*build_adjacency(d.sources, d.destinations, d.edge_idxs, d.timestamps))
    ref = MR.MlpOracleTGN(onf, g.node_features, g.edge_features, _params_of(tgn), L, H)
    rs = np.random.RandomState(2)
    s = 600
    warm = (d.sources[s:s + 30], d.destinations[s:s + 30], d.timestamps[s:s + 30], d.edge_idxs[s:s + 30])
    u, v = int(d.sources[s + 30]), int(d.destinations[s + 31])
    dup = (np.array([u, u, v, u, int(d.sources[s + 32])]), np.array([v, int(d.destinations[s + 30]), u, v, v]),
           d.timestamps[s + 30:s + 35].copy(), d.edge_idxs[s + 30:s + 35].copy())
    one = (d.sources[s + 40:s + 41], d.destinations[s + 40:s + 41], d.timestamps[s + 40:s + 41], d.edge_idxs[s + 40:s + 41])
    tgn.train()
    for sb, db, tb, eb in (warm, dup, one):
        B = len(sb)
        neg = rs.randint(cfg.n_users + 1, cfg.n_users + cfg.n_items + 1, size=B * 3)
        tgn.zero_grad(set_to_none=True)
        emb = torch.cat(tgn.compute_temporal_embeddings(sb, db, neg, tb, eb, K))
        rse, rde, rne = ref.compute_temporal_embeddings(sb, db, neg, tb, eb, K)
        assert relerr(emb.detach().cpu().numpy(), np.concatenate([rse, rde, rne])) < RTOL_EMB, B
        W = _bpr_seed(rse, rde, rne, B, np.float32).astype(np.float32)
        emb.backward(torch.from_numpy(W).to(DEV))
        rg = ref.backward(W)
        for name in MR.MLP_NAMES + [MR.GRU + "weight_ih"]:
            got = dict(tgn.named_parameters())[name].grad
            if np.abs(rg[name]).max() == 0:
                assert got is None or got.abs().max().item() == 0.0
                continue
            r = rg[name]
            e = np.linalg.norm(got.cpu().numpy().reshape(r.shape) - r) / np.linalg.norm(r)
            assert e < RTOL_GRAD_ORACLE_L2, (B, name, e)
        assert relerr(tgn.memory.memory.cpu().numpy(), ref.memory) < RTOL_EMB
        tab, mt, has = ref.pending_table()
        assert np.array_equal(tgn.memory.has_msg.cpu().numpy() > 0, has)
        assert relerr(tgn.memory.msg_table.cpu().numpy()[has], tab[has]) < RTOL_EMB
        assert np.array_equal(tgn.memory.msg_time.cpu().numpy()[has], mt[has])


# ---------------------------------------------------------------------------------------------- observe
@pytest.mark.parametrize("fixture", ["g11_step_L1_mem_mlp", "g11_step_L2_mem_mlp"])
def test_observe_leaves_the_state_the_training_step_leaves(fixture):
    """The same log through ``observe`` and through training-mode steps: memory, last_update and the message tables agree
    (tests/observe_ref.py's bars); once right after the parameters were written, once with a valid parameter cache."""
    g = load_golden(fixture)
    K = int(g["K"])
    a, b = _golden_model(g), _golden_model(g)
    pre = "s%d_" % g["recorded_steps"][0]
    for t in (a, b):
        _inject(t, g, pre)
        t.parameters_changed()
    a.train()
    for rnd, step in enumerate(g["recorded_steps"]):
        p = "s%d_" % step
        sb, db, tb, eb, neg = g[p + "src"], g[p + "dst"], g[p + "ts"], g[p + "eidx"], g[p + "neg"]
        if rnd == 1:
            b.eval()
            with torch.no_grad():
                keep = _tables(b)
                b.compute_temporal_embeddings(sb, db, neg.flatten(), tb, eb, K)         # leaves b's parameter cache valid
                _set_tables(b, keep)
        a.compute_temporal_embeddings(sb, db, neg.flatten(), tb, eb, K)
        assert b.observe(sb, db, tb, eb) == len(sb)
        e_mem, e_tab = O.check_tables(_tables(b), _tables(a), (fixture, step))
        if rnd == 0:
            O.check_tables(_tables(b), O.golden_after(g, p), (fixture, step, "golden"))
        print("FIGURES mlp observe %s step %d: memory relerr %.3g, message relerr %.3g" % (fixture, step, e_mem, e_tab))


# ---------------------------------------------------------------------------------------------- serving: ingest, then recommend
def test_ingest_of_unseen_nodes_then_recommend_ranks_like_the_host_model():
    torch.manual_seed(4)
    n_users, n_items, D, L, K = 28, 11, 16, 1, 4                          # 40 nodes with the padding node
    cfg = SyntheticConfig("t", n_users, n_items, 700, D, L, K, 2)
    g = make_graph(cfg, with_prices=False)
    d = g.data
    n_all = n_users + n_items + 1
    assert n_all == 40
    N0, CUT, BATCH = n_all - 2, 400, 24                                   # the last two items are unseen by the served model
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
    tick = np.asarray(tick)
    assert len(tick) == BATCH and seen >= 1
    tick_raw = g.edge_features[d.edge_idxs[tick]]
    tick_idx = np.arange(CUT + 1, CUT + 1 + BATCH)
    nf = P.NeighborFinder.from_arrays(d.sources[hist], d.destinations[hist], d.edge_idxs[hist], d.timestamps[hist], uniform=False,
                                      max_node_idx=N0 - 1)
    served = P.TGN(nf, g.node_features[:N0], g.edge_features[:CUT + 1], DEV, n_layers=L, n_heads=2, dropout=0.0, use_memory=True,
                   memory_dimension=D, message_function="mlp", message_dimension=100, n_neighbors=K)
    served.eval()
    rs = np.random.RandomState(3)
    warm = [hist[k:k + BATCH] for k in range(len(hist) - 3 * BATCH, len(hist), BATCH)]
    for s in warm:
        with torch.no_grad():
            served.compute_temporal_embeddings(d.sources[s], d.destinations[s], rs.randint(n_users + 1, N0, size=BATCH), d.timestamps[s], d.edge_idxs[s], K)
    sb, db, tb = d.sources[tick], d.destinations[tick], d.timestamps[tick]
    n, idxs = served.ingest(sb, db, tb, tick_raw, node_features=g.node_features[N0:N0 + seen])
    assert n == BATCH and np.array_equal(idxs, tick_idx)
    if seen < 2:
        served.add_nodes(2 - seen, g.node_features[N0 + seen:])
    assert served.n_nodes == n_all
    # the host model over the whole graph, on the served model's own (frozen-statistics) edge table
    h_and_t = np.concatenate([hist, tick])
    onf = OracleNeighborFinder(*build_adjacency(d.sources[h_and_t], d.destinations[h_and_t], np.concatenate([d.edge_idxs[hist], tick_idx]),
                                                d.timestamps[h_and_t]))
    ref = MR.MlpOracleTGN(onf, g.node_features, np.zeros((CUT + 1 + BATCH, g.edge_features.shape[1])), _params_of(served), L, 2)
    ref.edge_features = served.edge_raw_features.cpu().numpy().astype(np.float32)
    assert ref.edge_features.shape[0] == CUT + 1 + BATCH
    rs = np.random.RandomState(3)
    for s in warm:
        ref.compute_temporal_embeddings(d.sources[s], d.destinations[s], rs.randint(n_users + 1, N0, size=BATCH), d.timestamps[s], d.edge_idxs[s], K)
    ref.compute_temporal_embeddings(sb, db, np.repeat(db, 1), tb, tick_idx, K)
    O.check_tables(_tables(served), (ref.memory, ref.last_update) + ref.pending_table(), "ingest")
    users = np.unique(sb[:12])
    items = np.arange(n_users + 1, n_all)
    now = float(tb[-1]) + 1.0
    ids_k, sc_k, nv = (x.cpu().numpy() for x in served.recommend(users, now, len(items), items)[:3])
    assert (nv == len(items)).all()
    mem, _, _ = ref._get_updated_memory()
    nodes = np.concatenate([users, items])
    emb, _ = ref._embed(mem, nodes, np.full(len(nodes), now), L, K, None)
    s64 = emb[:len(users)].astype(np.float64) @ emb[len(users):].astype(np.float64).T
    order = np.argsort(ids_k, axis=1)
    by_item = np.take_along_axis(sc_k, order, 1)
    assert np.array_equal(np.take_along_axis(ids_k, order, 1), np.broadcast_to(items, ids_k.shape))
    e = relerr(by_item, s64)
    assert e < O.RTOL, e
    assert np.abs(s64[:, N0 - n_users - 1:N0 - n_users - 1 + seen]).max() > 0         # the new items are scored
    tol = 2 * O.RTOL * np.abs(s64).max()
    decided = 0
    for u in range(len(users)):
        want = np.argsort(s64[u], kind="stable")[::-1]
        if np.min(-np.diff(s64[u][want])) > tol:                           # no two host scores close enough to change places
            decided += 1
            assert np.array_equal(ids_k[u], items[want]), u
    assert decided >= len(users) // 2, decided
    print("FIGURES mlp ingest + recommend: score relerr %.3g, %d of %d users with a decided order" % (e, decided, len(users)))


# ---------------------------------------------------------------------------------------------- retention and growth
def test_expire_and_reserve_need_nothing_new():
    """The raw message table keeps its width: growing the tables (``reserve`` / ``add_nodes``) and dropping old edges with edge
    compaction (``expire``) work as with the identity function - a step afterwards agrees with a model that never grew, and with a
    model built over the surviving edges alone."""
    torch.manual_seed(8)
    D, L, K = 16, 1, 4
    cfg = SyntheticConfig("t", 50, 10, 900, D, L, K, 2)
    g = make_graph(cfg, with_prices=False)
    d = g.data

    def model():
        torch.manual_seed(8)
        return P.TGN(P.get_neighbor_finder(d, False), g.node_features, g.edge_features, DEV, n_layers=L, n_heads=2, dropout=0.0,
                     use_memory=True, memory_dimension=D, message_function="mlp", message_dimension=100, n_neighbors=K)
    a, b = model(), model()
    rs = np.random.RandomState(1)
    for t in (a, b):
        t.eval()
    batches = [(slice(s, s + 20), rs.randint(cfg.n_users + 1, cfg.n_users + cfg.n_items + 1, size=20)) for s in (500, 520, 540)]
    for i, (sl, neg) in enumerate(batches):
        if i == 2:
            b.reserve(n_nodes=b.n_nodes + 16, n_edges=int(b.edge_raw_features.shape[0]) + 64)
            assert b.add_nodes(3, np.zeros((3, D), np.float32)) == a.n_nodes
        outs = []
        for t in (a, b):
            with torch.no_grad():
                outs.append(torch.cat(t.compute_temporal_embeddings(d.sources[sl], d.destinations[sl], neg, d.timestamps[sl], d.edge_idxs[sl], K)).cpu().numpy())
        assert relerr(outs[1], outs[0]) < 1e-6, i
    ta, tb_ = _tables(a), _tables(b)
    n = a.n_nodes
    O.check_tables(tuple(x[:n] for x in tb_), ta, "reserve")
    assert tb_[2].shape[1] == 3 * D + g.edge_features.shape[1]
    # ---- expire, with edge compaction: ``a`` drops every adjacency entry older than the cutoff and renumbers its edge rows; ``c``
    # is a model built over the surviving edges alone (original edge indices, the whole table), given a's parameters and state
    cutoff = float(d.timestamps[300])
    live = d.timestamps >= cutoff
    assert 0 < (~live).sum() and d.timestamps[560] >= cutoff
    torch.manual_seed(8)
    nf_c = P.NeighborFinder.from_arrays(d.sources[live], d.destinations[live], d.edge_idxs[live], d.timestamps[live], uniform=False,
                                        max_node_idx=g.node_features.shape[0] - 1)
    c = P.TGN(nf_c, g.node_features, g.edge_features, DEV, n_layers=L, n_heads=2, dropout=0.0, use_memory=True, memory_dimension=D,
              message_function="mlp", message_dimension=100, n_neighbors=K)
    c.eval()
    assert torch.equal(c.flat_parameters, a.flat_parameters)
    _set_tables(c, ta)
    dropped, remap = a.expire(cutoff)
    assert dropped > 0 and remap is not None and int(a.edge_raw_features.shape[0]) < int(c.edge_raw_features.shape[0])
    remap = remap.cpu().numpy()
    sl, neg = slice(560, 580), rs.randint(cfg.n_users + 1, cfg.n_users + cfg.n_items + 1, size=20)
    eb_a = remap[d.edge_idxs[sl]]
    assert (eb_a >= 1).all() and (eb_a != d.edge_idxs[sl]).any()                 # the batch's rows survive, renumbered
    outs = []
    for t, eb in ((c, d.edge_idxs[sl]), (a, eb_a)):
        with torch.no_grad():
            outs.append(torch.cat(t.compute_temporal_embeddings(d.sources[sl], d.destinations[sl], neg, d.timestamps[sl], eb, K)).cpu().numpy())
    assert relerr(outs[1], outs[0]) < 1e-6
    O.check_tables(_tables(a), _tables(c), "expire")


# ---------------------------------------------------------------------------------------------- prefetch, torch Adam
def test_prefetched_batches_give_the_same_steps():
    """``TGN.prefetch`` hands the step PACKED raw rows (the MLP then reads them without a gather, the GRU takes its packed form);
    without it the rows are gathered from the tables.  Deterministic mode, torch.optim.Adam over ``tgn.parameters()``: embeddings,
    gradients, parameters and the memory tables of a four-step run are bitwise the same both ways."""
    cfg = SyntheticConfig("pre", 300, 25, 6000, 32, 2, 6, 2)
    g = make_graph(cfg, with_prices=False)
    d = g.data
    B, q, K = 48, 3, 6
    rs = np.random.RandomState(5)
    starts = [3000 + B * i for i in range(4)]
    negs = [rs.randint(cfg.n_users + 1, cfg.n_users + cfg.n_items + 1, size=B * q) for _ in starts]

    def run(prefetch):
        torch.manual_seed(11)
        tgn = P.TGN(P.get_neighbor_finder(d, False), g.node_features, g.edge_features, DEV, n_layers=2, n_heads=2, dropout=0.1,
                    use_memory=True, memory_dimension=32, message_function="mlp", message_dimension=100, n_neighbors=K)
        tgn.deterministic = True
        tgn.train()
        opt = torch.optim.Adam(tgn.parameters(), lr=1e-3)
        held = [p for g_ in opt.param_groups for p in g_["params"]]
        assert sum(any(p is q_ for q_ in tgn.message_function.parameters()) for p in held) == 4       # each MLP tensor once
        dev = lambda a, t: tgn._to_dev(a, t)
        batches = [(dev(d.sources[s:s + B], np.int32), dev(d.destinations[s:s + B], np.int32), dev(n, np.int32),
                    dev(d.timestamps[s:s + B], np.float64), dev(d.edge_idxs[s:s + B], np.int32)) for s, n in zip(starts, negs)]
        out = []
        for i, (s_, d_, n_, t_, e_) in enumerate(batches):
            emb, b = tgn.embed_device(s_, d_, [n_], [q], t_, e_, K)
            if prefetch and i + 1 < len(batches):
                s2, d2, n2, t2, e2 = batches[i + 1]
                with tgn.prefetching():
                    assert tgn.prefetch(s2, d2, [n2], [q], t2, e2, K)
            P.bpr_step(tgn, emb, b, q)
            grad = tgn.flat_grad.clone()
            opt.step()
            opt.zero_grad(set_to_none=True)
            out.append((emb.detach().clone(), grad, tgn._flat.detach().clone()))
        mem = [t.clone() for t in (tgn.memory.memory.data, tgn.memory.msg_table, tgn.memory.msg_time)]
        torch.cuda.synchronize()
        return out, mem, tgn._layout
    a, mem_a, lay = run(False)
    b_, mem_b, _ = run(True)
    for (e0, g0, p0), (e1, g1, p1) in zip(a, b_):
        assert torch.equal(e0, e1) and torch.equal(g0, g1) and torch.equal(p0, p1)
    for x, y in zip(mem_a, mem_b):
        assert torch.equal(x, y)
    assert a[0][1][lay.mlp_w1:lay.layer[0].wq].abs().max().item() == 0 and a[1][1][lay.mlp_w1:lay.layer[0].wq].abs().max().item() > 0
    # torch Adam skipped the MLP's and the GRU's tensors in the first step (their gradients are None): they moved in the second
    assert not torch.equal(a[1][2][lay.mlp_w1:lay.layer[0].wq], a[0][2][lay.mlp_w1:lay.layer[0].wq])


# ---------------------------------------------------------------------------------------------- the evaluation pass
def test_evaluation_pass_leaves_the_state_observe_leaves():
    """``eval_recommendation`` (forward-only passes over B (2 + n_items) roots per batch, chunked) runs the same lazy MLP + GRU:
    after the pass the memory and message tables are what ``observe`` leaves over the same interactions, and the ranks are those
    of the model's own embeddings."""
    import test_gpu_eval_invest as EI
    from pfotgnrec_amd import evaluation as E
    g = load_golden("g9b_eval_loop_L2")
    L, H, K = int(g["L"]), int(g["H"]), int(g["K"])
    D = g["node_features"].shape[1]
    data, full, tables, mid = EI._g9b_data(g)
    B, U = int(g["batch"]), int(g["upper_u"])

    def model():
        torch.manual_seed(2)
        nf = P.NeighborFinder.from_arrays(g["src_all"], g["dst_all"], g["eidx_all"], g["ts_all"], uniform=False)
        t = P.TGN(nf, g["node_features"], g["edge_features"], DEV, n_layers=L, n_heads=H, dropout=0.1, use_memory=True,
                  memory_dimension=D, message_function="mlp", message_dimension=100, n_neighbors=K)
        EI._g9b_reset(t, g)
        return t
    a, b = model(), model()
    rows = E.eval_recommendation_rows(a, data, full, B, K, U, 30, False, tables=tables, negatives=list(g["negatives"]))
    n = rows["rank"].shape[0]
    assert n == 5 * B and np.isfinite(rows["invest"]).all()
    assert b.observe(data.sources[:n], data.destinations[:n], data.timestamps[:n], data.edge_idxs[:n], batch_size=B) == n
    e_mem, e_tab = O.check_tables(_tables(a), _tables(b), "eval vs observe")
    print("FIGURES mlp eval pass vs observe: memory relerr %.3g, message relerr %.3g" % (e_mem, e_tab))
    assert len(np.unique(rows["rank"])) > 3                             # the scores tell the candidates apart


# ---------------------------------------------------------------------------------------------- deterministic mode
def test_deterministic_backward_is_bitwise_reproducible():
    torch.manual_seed(3)
    D, K, B = 32, 6, 64
    cfg = SyntheticConfig("det", 300, 25, 5000, D, 2, K, 2)
    g = make_graph(cfg, with_prices=False)
    d = g.data
    tgn = P.TGN(P.get_neighbor_finder(d, False), g.node_features, g.edge_features, DEV, n_layers=2, n_heads=2, dropout=0.1,
                use_memory=True, memory_dimension=D, message_function="mlp", message_dimension=100, n_neighbors=K)
    rs = np.random.RandomState(1)
    tgn.train()
    for s in (2500, 2564):
        neg = rs.randint(cfg.n_users + 1, cfg.n_users + cfg.n_items + 1, size=B * 3)
        with torch.no_grad():
            tgn.compute_temporal_embeddings(d.sources[s:s + B], d.destinations[s:s + B], neg, d.timestamps[s:s + B], d.edge_idxs[s:s + B], K)
    m = tgn.memory
    snap = [t.clone() for t in (m.memory.data, m.last_update.data, m.msg_table, m.msg_time, m.has_msg)]
    s = 2628
    batch = (d.sources[s:s + B], d.destinations[s:s + B], rs.randint(cfg.n_users + 1, cfg.n_users + cfg.n_items + 1, size=B * 3),
             d.timestamps[s:s + B], d.edge_idxs[s:s + B])

    def grad(det):
        with torch.no_grad():
            for dst_t, src_t in zip((m.memory.data, m.last_update.data, m.msg_table, m.msg_time, m.has_msg), snap):
                dst_t.copy_(src_t)
        tgn.deterministic = det
        tgn._step = 1000
        tgn.zero_grad(set_to_none=True)
        emb = torch.cat(tgn.compute_temporal_embeddings(*batch, K))
        P.bpr_loss(emb, B, 3).backward()
        return tgn.flat_grad.clone()
    g1, g2, g3 = grad(True), grad(True), grad(True)
    assert torch.equal(g1, g2) and torch.equal(g2, g3)
    lay = tgn._layout
    assert g1[lay.mlp_w1:lay.layer[0].wq].abs().max().item() > 0
    g0 = grad(False)
    den = g0[2 * D:].abs().max().item()
    assert (g1[2 * D:] - g0[2 * D:]).abs().max().item() <= 2e-5 * den
    tgn.deterministic = False


# ---------------------------------------------------------------------------------------------- graph capture
def test_graphed_step_equals_the_eager_step():
    from pfotgnrec_amd.rand_edge_sampler import item_availability, DeviceNegativeSampler
    D, K, B, q = 32, 6, 32, 3
    cfg = SyntheticConfig("gr", 200, 30, 3000, D, 1, K, 2)
    g = make_graph(cfg, with_prices=False)
    d = g.data
    start = 1500

    def run(graphed):
        torch.manual_seed(5)
        tgn = P.TGN(P.get_neighbor_finder(d, False), g.node_features, g.edge_features, DEV, n_layers=1, n_heads=2, dropout=0.0,
                    use_memory=True, memory_dimension=D, message_function="mlp", message_dimension=100, n_neighbors=K)
        opt = P.FusedAdam(tgn, lr=1e-3)
        tgn.deterministic = True
        sampler = DeviceNegativeSampler(item_availability(d.destinations, g.upper_u, cfg.n_items), g.upper_u, DEV, seed=1)
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)
        src, dst, ts, eidx = t(d.sources, np.int32), t(d.destinations, np.int32), t(d.timestamps, np.float64), t(d.edge_idxs, np.int32)
        pidx, plen = t(g.portfolio_idx, np.int32), t(g.portfolio_len, np.int32)
        tgn.train()
        gs = P.GraphedTrainStep(tgn, opt, sampler, B, K, n_neg=q, port_width=pidx.shape[1])
        batch = lambda i: tuple(x[start + i * B:start + (i + 1) * B] for x in (src, dst, ts, eidx, pidx, plen)) + (None,)
        if graphed:
            gs.capture(*batch(0), warmup=3)
        else:
            for _ in range(3):
                gs.eager(*batch(0))
            gs._fold_steps()
        losses = [float((gs if graphed else gs.eager)(*batch(i))) for i in range(3)]
        tgn.join()
        torch.cuda.synchronize()
        return losses, tgn.flat_parameters.detach().clone(), tgn.memory.memory.detach().clone(), tgn._layout
    le, pe, me, lay = run(False)
    lg, pg, mg, _ = run(True)
    assert le == lg, (le, lg)
    assert torch.equal(pg, pe) and torch.equal(mg, me)
    assert torch.isfinite(pe).all() and torch.isfinite(me).all()


# ---------------------------------------------------------------------------------------------- data parallel
def _run_dp(rank, world, port, out_dir, n_steps, B):
    sys.path.insert(0, REPO)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch.distributed as dist
    import pfotgnrec_amd as P
    from pfotgnrec_amd.distributed import init_from_env, allreduce_flat_grad, broadcast_parameters
    from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
    init_from_env(backend="gloo")
    dev = torch.device("cuda:0")
    torch.manual_seed(5)
    cfg = SyntheticConfig("dp", 300, 25, 5000, 32, 2, 6, 2)
    g = make_graph(cfg, with_prices=False)
    d = g.data
    tgn = P.TGN(P.get_neighbor_finder(d, False), g.node_features, g.edge_features, dev, n_layers=2, n_heads=2, dropout=0.0,
                use_memory=True, memory_dimension=32, message_function="mlp", message_dimension=100)
    tgn.set_data_parallel(rank, world)
    broadcast_parameters(tgn.flat_parameters, world)
    opt = P.FusedAdam(tgn, lr=1e-3)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    rs = np.random.RandomState(0)
    tgn.train()
    grads = []
    for step in range(n_steps):
        s = 2500 + step * B
        neg = t(rs.randint(301, 326, size=B * 3), np.int32)
        emb, b = tgn.embed_device(t(d.sources[s:s + B], np.int32), t(d.destinations[s:s + B], np.int32), [neg], [3],
                                  t(d.timestamps[s:s + B], np.float64), t(d.edge_idxs[s:s + B], np.int32), 6)
        loss = P.bpr_loss(emb, b, 3, grad_scale=tgn.dp_grad_scale)
        loss.backward()
        allreduce_flat_grad(tgn.flat_grad, world)
        if step <= 1:
            grads.append(tgn.flat_grad.cpu().numpy().copy())
            mem1 = tgn.memory.memory.cpu().numpy().copy()
        opt.step()
        opt.zero_grad(set_to_none=True)
    tgn.join()
    torch.cuda.synchronize()
    lay = tgn._layout
    np.savez(os.path.join(out_dir, "mlp_w%d_r%d.npz" % (world, rank)), params=tgn.flat_parameters.cpu().numpy(), grad0=grads[0], grad1=grads[1],
             mem1=mem1, last_update=tgn.memory.last_update.cpu().numpy(), has=tgn.memory.has_msg.cpu().numpy(),
             msg_t=tgn.memory.msg_time.cpu().numpy(), mlp=np.array([lay.mlp_w1, lay.layer[0].wq]))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def test_two_ranks_equal_one_rank(tmp_path):
    """tests/test_gpu_data_parallel.py's criterion with the MLP: two ranks on one GPU (gloo) equal one rank at the same global
    batch.  Gradients are compared on the first TWO steps - in the first no node holds a pending message and the MLP's block
    of the flat gradient is exactly zero on every side."""
    port = 29400 + (os.getpid() % 150)
    ctx = mp.get_context("spawn")
    for world in (1, 2):
        procs = [ctx.Process(target=_run_dp, args=(r, world, port + world, str(tmp_path), 3, 48)) for r in range(world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(600)
            assert p.exitcode == 0
    one = np.load(tmp_path / "mlp_w1_r0.npz")
    r0, r1 = np.load(tmp_path / "mlp_w2_r0.npz"), np.load(tmp_path / "mlp_w2_r1.npz")
    for k in one.files:
        assert np.array_equal(r0[k], r1[k]), "replicas diverged: " + k
    rel = lambda a, b: np.abs(a.astype(np.float64) - b).max() / (np.abs(b).max() + 1e-12)
    D = 32
    lo, hi = (int(v) for v in one["mlp"])
    assert np.abs(one["grad0"][lo:hi]).max() == 0 and np.abs(r0["grad0"][lo:hi]).max() == 0
    assert rel(r0["grad0"][2 * D:], one["grad0"][2 * D:]) < 1e-4
    assert rel(r0["grad0"][:2 * D], one["grad0"][:2 * D]) < 3e-3
    # the second step starts from parameters one Adam step apart by +-lr noise on both sides: the MLP's block, nonzero now, to 1e-2
    assert np.abs(one["grad1"][lo:hi]).max() > 0
    assert rel(r0["grad1"][lo:hi], one["grad1"][lo:hi]) < 1e-2
    assert np.array_equal(r0["last_update"], one["last_update"]) and np.array_equal(r0["has"], one["has"])
    assert np.array_equal(r0["msg_t"], one["msg_t"])
    assert rel(r0["params"], one["params"]) < 1e-2
