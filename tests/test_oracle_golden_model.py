"""Pin oracle/tgn_oracle.py (fp32 numpy, hand-derived backward) against the reference's torch modules + autograd."""
from collections import defaultdict

import numpy as np
import pytest

from conftest import load_golden
from oracle import tgn_oracle as T
from oracle.neighbor_finder import OracleNeighborFinder, build_adjacency

from parity import relerr, row_relerr, ROW_RTOL

RTOL = 1e-4     # north_star bar; observed restatement error is 1e-7..1e-6
FIGURES = {}    # (fixture, quantity) -> worst error seen (printed by the g10 tests: run with -s to read them)


def test_g4_time_encode_bit_exact_argument():
    g = load_golden("g4_modules")
    y = T.time_encode(g["te_t"], g["te_w"], g["te_b"])
    # the fp32 FMA argument is exact; cos implementations may differ by an ulp
    assert np.abs(y - g["te_y"]).max() < 5e-7
    gw, gb = T.time_encode_backward(g["te_t"], g["te_w"], g["te_b"], g["te_gy"])
    assert relerr(gw, g["te_gw"].reshape(-1)) < 1e-5 and relerr(gb, g["te_gb"]) < 1e-5


def test_fmaf_single_rounding():
    rs = np.random.RandomState(0)
    a = rs.randint(0, 1 << 24, 100000).astype(np.float32)
    b = (10 ** -rs.uniform(0, 9, 100000)).astype(np.float32)
    c = rs.randn(100000).astype(np.float32)
    from fractions import Fraction
    got = T.fmaf(a, b, c)
    for i in range(0, 100000, 997):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))        # python float() of a Fraction is correctly rounded to f64; then one more rounding
        # brute-force the correctly rounded f32: nearest of the two f32 neighbours of the exact value
        cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        best = min(cands, key=lambda v: abs(Fraction(float(v)) - exact))
        assert got[i] == best


def test_g4_gru():
    g = load_golden("g4_modules")
    hn, cache = T.gru_cell(g["gru_x"], g["gru_h"], g["gru_weight_ih"], g["gru_weight_hh"], g["gru_bias_ih"], g["gru_bias_hh"])
    assert relerr(hn, g["gru_hn"]) < 1e-5
    gr = T.gru_cell_backward(cache, g["gru_ghn"], g["gru_weight_ih"], g["gru_weight_hh"])
    for k, v in gr.items():
        assert relerr(v, g["gru_g_" + k]) < 1e-5, k


def _att_params(g):
    p = "att_p_"
    return dict(Wq=g[p + "multi_head_target.q_proj_weight"], Wk=g[p + "multi_head_target.k_proj_weight"],
                Wv=g[p + "multi_head_target.v_proj_weight"], b_in=g[p + "multi_head_target.in_proj_bias"],
                Wo=g[p + "multi_head_target.out_proj.weight"], bo=g[p + "multi_head_target.out_proj.bias"],
                W1=g[p + "merger.fc1.weight"], b1=g[p + "merger.fc1.bias"], W2=g[p + "merger.fc2.weight"], b2=g[p + "merger.fc2.bias"])


def test_g4_attention_forward_backward():
    g = load_golden("g4_modules")
    p = _att_params(g)
    H, D = int(g["H"]), int(g["D"])
    out, c = T.attention_forward(p, g["att_x"], g["att_tq"], g["att_nb"], g["att_ef"], g["att_tn"], g["att_mask"], H)
    assert relerr(out, g["att_out"]) < 1e-5
    # rows with no valid neighbour: zero attention output -> MergeLayer([0 | x])
    inv = g["att_mask"].all(1)
    assert inv.sum() == 8
    grads, dx, dtq, dnb, dte = T.attention_backward(p, c, g["att_go"], H, D)
    assert relerr(dx, g["att_gx"]) < 1e-5 and relerr(dnb, g["att_gnb"]) < 1e-5
    assert relerr(dte, g["att_gtn"]) < 1e-5 and relerr(dtq, g["att_gtq"]) < 1e-5
    for k, name in T._LAYER_KEYS.items():
        assert relerr(grads[k], g["att_g_" + name]) < 1e-5, name


def _load_state(g, pre, tgn, use_mem):
    P = {}
    for k in g.files:
        if k.startswith(pre + "sd_"):
            name = k[len(pre + "sd_"):]
            if name in ("memory.memory", "memory.last_update") or "layer_norm" in name:
                continue
            P[name] = g[k]
    tgn.P = {k: v.astype(np.float32) for k, v in P.items()}
    if use_mem:
        tgn.memory = g[pre + "sd_memory.memory"].copy()
        tgn.last_update = g[pre + "sd_memory.last_update"].copy()
        tgn.messages = defaultdict(list)
        tab, mt, cnt = g[pre + "msg_tab"], g[pre + "msg_t"], g[pre + "msg_cnt"]
        for nid in np.nonzero(cnt)[0]:
            tgn.messages[int(nid)] = [(tab[nid], mt[nid])]


def _note(fixture, key, value):
    FIGURES[(fixture, key)] = max(FIGURES.get((fixture, key), 0.0), float(value))
    return value


@pytest.mark.parametrize("tag", ["L1_mem", "L2_mem", "L2_nomem_uniform", "L1_mem_p"])
def test_g5_full_step(tag):
    _full_step("g5_step_" + tag, "draws")


@pytest.mark.parametrize("tag", ["L1_mem", "L2_mem", "L2_nomem_uniform", "L1_mem_p"])
def test_g10_full_step_real_timestamps(tag):
    """The g5 step on yyyymmddHHMMSS timestamps (f32 step 2**21): f32 message times and last_update bit-exact, deltas up to
    ~1e10 through the time encoder, and - uniform, two layers - sampled rows where ties between different edges are the rule:
    the draws of the call on the neighbours are injected re-addressed to the canonical (stable) slot order."""
    _full_step("g10_realts_step_" + tag, "cdraws")
    print({k[1]: "%.3g" % v for k, v in FIGURES.items() if k[0] == "g10_realts_step_" + tag})


def test_g10_uniform_raw_draws_are_misaddressed():
    """The reference logs the neighbour call's draws in ITS slot order (default argsort on f32 times, utils.py:201); injected
    as they are, rows land on other nodes than they were drawn for: the oracle refuses them or the embeddings miss the bar."""
    g = load_golden("g10_realts_step_L2_nomem_uniform")
    assert sum(int(g["s%d_n_readdressed_roots" % s]) for s in g["recorded_steps"]) > 0
    assert any(not np.array_equal(g["s%d_draws2" % s], g["s%d_cdraws2" % s]) for s in g["recorded_steps"])
    for s in g["recorded_steps"]:                                  # the calls on the roots need no re-addressing
        assert np.array_equal(g["s%d_draws0" % s], g["s%d_cdraws0" % s]) and np.array_equal(g["s%d_draws1" % s], g["s%d_cdraws1" % s])
    with pytest.raises((ValueError, AssertionError)):
        _full_step("g10_realts_step_L2_nomem_uniform", "draws")


def _full_step(fixture, draws_key):
    g = load_golden(fixture)
    tag = fixture
    L, H, K = int(g["L"]), int(g["H"]), int(g["K"])
    use_mem, uniform, path = bool(g["use_memory"]), bool(g["uniform"]), str(g["path"])
    nf = OracleNeighborFinder(*build_adjacency(g["src_all"], g["dst_all"], g["eidx_all"], g["ts_all"]), uniform=uniform)
    tgn = T.OracleTGN(nf, g["node_features"], g["edge_features"], {}, L, H, use_memory=use_mem)
    for step in g["recorded_steps"]:
        pre = "s%d_" % step
        _load_state(g, pre, tgn, use_mem)                           # re-inject reference state at every step
        draws = None
        if uniform:
            draws = [g[pre + draws_key + "%d" % j] for j in range(3 if L == 2 else 1)]
        sb, db, tb, eb, neg = g[pre + "src"], g[pre + "dst"], g[pre + "ts"], g[pre + "eidx"], g[pre + "neg"]
        B = len(sb)
        if path == "p":
            se, de, pe, ne = tgn.compute_temporal_embeddings_p(sb, db, g[pre + "ppos"], neg.flatten(), tb, eb, K, draws=draws)
        else:
            se, de, ne = tgn.compute_temporal_embeddings(sb, db, neg.flatten(), tb, eb, K, draws=draws)
            pe = de
        for got, key in ((se, "emb_src"), (de, "emb_dst"), (pe, "emb_pos"), (ne, "emb_neg")):
            assert _note(fixture, "emb relerr", relerr(got, g[pre + key])) < RTOL, (tag, step, key, relerr(got, g[pre + key]))
            assert _note(fixture, "emb row_relerr", row_relerr(got, g[pre + key])) < ROW_RTOL, (tag, step, key, row_relerr(got, g[pre + key]))
        loss, cache = T.bpr_loss(se, pe.reshape(B, 1, -1), ne.reshape(B, 3, -1))
        assert abs(loss - g[pre + "loss"]) < 1e-5 * max(1.0, abs(g[pre + "loss"]))
        d_src, d_pos, d_neg = T.bpr_loss_backward(cache)
        assert relerr(d_src, g[pre + "gemb_src"]) < RTOL and relerr(d_neg.reshape(-1, d_src.shape[1]), g[pre + "gemb_neg"]) < RTOL
        d_dst = np.zeros_like(d_src)
        if path == "p":
            d_emb = np.concatenate([d_src, d_dst, d_pos.reshape(B, -1), d_neg.reshape(3 * B, -1)])
        else:
            d_emb = np.concatenate([d_src, d_pos.reshape(B, -1), d_neg.reshape(3 * B, -1)])
        grads = tgn.backward(d_emb)
        worst = 0.0
        for k in g.files:
            if k.startswith(pre + "grad_"):
                name = k[len(pre + "grad_"):]
                if "layer_norm" in name or name.startswith("memory."):
                    continue
                ref = g[k]
                got = grads[name].reshape(ref.shape)
                if np.abs(ref).max() == 0:
                    assert np.abs(got).max() < 1e-7, name
                    continue
                e = relerr(got, ref)
                worst = max(worst, e)
                _note(fixture, "time grad relerr" if name.startswith("time_encoder") else "grad relerr", e)
                assert e < 5e-4, (tag, step, name, e)
        if use_mem:
            assert _note(fixture, "memory relerr", relerr(tgn.memory, g[pre + "after_memory"])) < RTOL
            assert _note(fixture, "memory row_relerr", row_relerr(tgn.memory, g[pre + "after_memory"])) < ROW_RTOL
            assert np.array_equal(tgn.last_update, g[pre + "after_last_update"])
            tab, mt, has = tgn.pending_table()
            assert np.array_equal(has, g[pre + "after_msg_cnt"] > 0)
            assert _note(fixture, "msg relerr", relerr(tab, g[pre + "after_msg_tab"])) < RTOL
            assert _note(fixture, "msg row_relerr", row_relerr(tab, g[pre + "after_msg_tab"])) < ROW_RTOL
            assert np.array_equal(mt, g[pre + "after_msg_t"])
            # per-node list lengths (all messages of a node come from one batch)
            cnt = np.array([len(tgn.messages.get(i, [])) for i in range(tgn.n_nodes)])
            touched = np.zeros(tgn.n_nodes, bool); touched[np.concatenate([sb, db])] = True
            assert np.array_equal(cnt[touched], g[pre + "after_msg_cnt"][touched])


# ------------------------------------------------------------------ g8: train-mode attention dropout (the benched setting, round 4)
def _att_params_pre(g, pre):
    p = pre + "p_"
    return dict(Wq=g[p + "multi_head_target.q_proj_weight"], Wk=g[p + "multi_head_target.k_proj_weight"],
                Wv=g[p + "multi_head_target.v_proj_weight"], b_in=g[p + "multi_head_target.in_proj_bias"],
                Wo=g[p + "multi_head_target.out_proj.weight"], bo=g[p + "multi_head_target.out_proj.bias"],
                W1=g[p + "merger.fc1.weight"], b1=g[p + "merger.fc1.bias"], W2=g[p + "merger.fc2.weight"], b2=g[p + "merger.fc2.bias"])


@pytest.mark.parametrize("tag", ["p10", "p50"])
def test_g8_attention_layer_with_dropout(tag):
    """TemporalAttentionLayer in train mode (nn.MultiheadAttention dropout on the softmax weights, temporal_attention.py:28,70)
    with the reference's own dropout multipliers injected: forward, input gradients and every parameter gradient."""
    g = load_golden("g8_dropout")
    pre = "att_%s_" % tag
    p = _att_params_pre(g, pre)
    H, D = int(g["H"]), int(g["D"])
    drop = g[pre + "drop"]
    pd = float(g[pre + "p"])
    assert all(min(abs(float(v)), abs(float(v) - 1 / (1 - pd))) < 1e-5 for v in np.unique(drop)) and (drop == 0).any()
    out, c = T.attention_forward(p, g[pre + "x"], g[pre + "tq"], g[pre + "nb"], g[pre + "ef"], g[pre + "tn"], g[pre + "mask"], H, drop)
    assert relerr(out, g[pre + "out"]) < 1e-5
    out0, _ = T.attention_forward(p, g[pre + "x"], g[pre + "tq"], g[pre + "nb"], g[pre + "ef"], g[pre + "tn"], g[pre + "mask"], H)
    assert relerr(out0, g[pre + "out"]) > 1e-3                 # the mask matters: without it the outputs differ
    grads, dx, dtq, dnb, dte = T.attention_backward(p, c, g[pre + "go"], H, D)
    assert relerr(dx, g[pre + "gx"]) < 1e-5 and relerr(dnb, g[pre + "gnb"]) < 1e-5
    assert relerr(dte, g[pre + "gtn"]) < 1e-5 and relerr(dtq, g[pre + "gtq"]) < 1e-5
    for k, name in T._LAYER_KEYS.items():
        assert relerr(grads[k], g[pre + "g_" + name]) < 1e-5, name


def test_g8_full_step_with_dropout():
    """One training step of the 2-layer TGN with memory at dropout 0.1 (main.py --drop_out default), the reference's three
    dropout masks injected in level order: embeddings, loss, every parameter gradient, memory state machine."""
    g = load_golden("g8_dropout")
    L, H, K = int(g["step_L"]), int(g["step_H"]), int(g["step_K"])
    nf = OracleNeighborFinder(*build_adjacency(g["src_all"], g["dst_all"], g["eidx_all"], g["ts_all"]), uniform=False)
    tgn = T.OracleTGN(nf, g["node_features"], g["edge_features"], {}, L, H, use_memory=True)
    _load_state(g, "s_", tgn, True)
    tgn.dropout_masks = {1: g["s_drop_l1"], 2: g["s_drop_l2"]}
    sb, db, tb, eb, neg = g["s_src"], g["s_dst"], g["s_ts"], g["s_eidx"], g["s_neg"]
    B = len(sb)
    se, de, ne = tgn.compute_temporal_embeddings(sb, db, neg.flatten(), tb, eb, K)
    for got, key in ((se, "emb_src"), (de, "emb_dst"), (ne, "emb_neg")):
        assert relerr(got, g["s_" + key]) < RTOL, (key, relerr(got, g["s_" + key]))
        assert _note("g8_dropout", "emb row_relerr", row_relerr(got, g["s_" + key])) < ROW_RTOL, (key, row_relerr(got, g["s_" + key]))
    loss, cache = T.bpr_loss(se, de.reshape(B, 1, -1), ne.reshape(B, 3, -1))
    assert abs(loss - g["s_loss"]) < 1e-5 * max(1.0, abs(g["s_loss"]))
    d_src, d_pos, d_neg = T.bpr_loss_backward(cache)
    grads = tgn.backward(np.concatenate([d_src, d_pos.reshape(B, -1), d_neg.reshape(3 * B, -1)]))
    n_checked = 0
    for k in g.files:
        if k.startswith("s_grad_"):
            name = k[len("s_grad_"):]
            if "layer_norm" in name or name.startswith("memory."):
                continue
            ref = g[k]
            if np.abs(ref).max() == 0:
                continue
            assert relerr(grads[name].reshape(ref.shape), ref) < 5e-4, (name, relerr(grads[name].reshape(ref.shape), ref))
            n_checked += 1
    assert n_checked >= 20
    assert relerr(tgn.memory, g["s_after_memory"]) < RTOL
    assert _note("g8_dropout", "memory row_relerr", row_relerr(tgn.memory, g["s_after_memory"])) < ROW_RTOL
    assert np.array_equal(tgn.last_update, g["s_after_last_update"])
    tab, mt, has = tgn.pending_table()
    assert np.array_equal(has, g["s_after_msg_cnt"] > 0) and relerr(tab, g["s_after_msg_tab"]) < RTOL
    assert _note("g8_dropout", "msg row_relerr", row_relerr(tab, g["s_after_msg_tab"])) < ROW_RTOL
    # without the masks the embeddings are off by far more than the bar: the fixture does pin the dropout algebra
    _load_state(g, "s_", tgn, True)
    tgn.dropout_masks = None
    se0, _, _ = tgn.compute_temporal_embeddings(sb, db, neg.flatten(), tb, eb, K)
    assert relerr(se0, g["s_emb_src"]) > 1e-3


# ------------------------------------------------------------------ the attention layer at widths no fixture has
@pytest.mark.parametrize("D,Ef,H,K", [(8, 0, 1, 3), (12, 8, 2, 4), (32, 4, 2, 64), (16, 64, 2, 5)])
def test_attention_layer_against_torch_at_other_widths(D, Ef, H, K):
    """The fixtures pin the oracle to the reference at ONE edge-feature width.  Here the layer is restated from its public parts -
    torch.nn.MultiheadAttention(embed_dim=2D, kdim=vdim=2D+Ef) + the two-layer merger (temporal_attention.py:22-32,
    utils.py:5-20), float64, same weights - at no edge columns, Ef close to D, Ef far wider than D and a full 64 keys, with the
    rule for rows that are all padding (first slot unmasked, output zeroed, :60-84).  Forward and every gradient (torch.autograd)
    at the bars of test_g4_attention_forward_backward."""
    import torch
    rs = np.random.RandomState(100 * D + Ef)
    N, E, C = 37, 2 * D, 2 * D + Ef
    P = T.init_params(D, Ef, 1, seed=D + K, use_memory=False)
    p = T.layer_params(P, 0)
    x, tq = rs.randn(N, D).astype(np.float32), rs.randn(N, D).astype(np.float32)
    nb, te = rs.randn(N, K, D).astype(np.float32), rs.randn(N, K, D).astype(np.float32)
    ef = rs.randn(N, K, Ef).astype(np.float32)
    n_valid = rs.randint(0, K + 1, N)                                  # most-recent layout: padding in front
    n_valid[:4] = (0, 0, K, 1)
    mask = np.arange(K)[None, :] < (K - n_valid)[:, None]
    assert mask.all(1).sum() >= 2 and (~mask).all(1).any()
    go = rs.randn(N, D).astype(np.float32)
    out, c = T.attention_forward(p, x, tq, nb, ef, te, mask, H)
    grads, dx, dtq, dnb, dte = T.attention_backward(p, c, go, H, D)

    t = lambda a, grad=False: torch.tensor(np.asarray(a, np.float64), requires_grad=grad)
    mha = torch.nn.MultiheadAttention(embed_dim=E, kdim=C, vdim=C, num_heads=H).double()
    fc1, fc2 = torch.nn.Linear(E + D, D).double(), torch.nn.Linear(D, D).double()
    packed = mha.q_proj_weight is None          # Ef = 0: kdim == embed_dim and torch keeps ONE in_proj_weight = [Wq ; Wk ; Wv]
    assert packed == (Ef == 0)
    with torch.no_grad():
        if packed:
            mha.in_proj_weight.copy_(t(np.concatenate([p["Wq"], p["Wk"], p["Wv"]])))
        else:
            for dst, src in ((mha.q_proj_weight, "Wq"), (mha.k_proj_weight, "Wk"), (mha.v_proj_weight, "Wv")):
                dst.copy_(t(p[src]))
        for dst, src in ((mha.in_proj_bias, "b_in"), (mha.out_proj.weight, "Wo"), (mha.out_proj.bias, "bo"), (fc1.weight, "W1"),
                         (fc1.bias, "b1"), (fc2.weight, "W2"), (fc2.bias, "b2")):
            dst.copy_(t(p[src]))
    tx, ttq, tnb, tte = t(x, True), t(tq, True), t(nb, True), t(te, True)
    query = torch.cat([tx, ttq], 1).unsqueeze(0)                                    # [1, N, E]
    key = torch.cat([tnb, t(ef), tte], 2).permute(1, 0, 2)                          # [K, N, C]
    inv = torch.from_numpy(mask.all(1))
    pad = torch.from_numpy(mask.copy())
    pad[inv, 0] = False
    attn, _ = mha(query=query, key=key, value=key, key_padding_mask=pad)
    attn = attn.squeeze(0).masked_fill(inv[:, None], 0.0)
    want = fc2(torch.relu(fc1(torch.cat([attn, tx], 1))))
    want.backward(t(go))
    assert relerr(out, want.detach().numpy()) < 1e-5
    assert row_relerr(out, want.detach().numpy()) < ROW_RTOL
    assert relerr(dx, tx.grad.numpy()) < 1e-5 and relerr(dnb, tnb.grad.numpy()) < 1e-5
    assert relerr(dte, tte.grad.numpy()) < 1e-5 and relerr(dtq, ttq.grad.numpy()) < 1e-5
    if packed:
        tg = dict(zip(("Wq", "Wk", "Wv"), mha.in_proj_weight.grad.numpy().reshape(3, E, E)))
    else:
        tg = dict(Wq=mha.q_proj_weight.grad.numpy(), Wk=mha.k_proj_weight.grad.numpy(), Wv=mha.v_proj_weight.grad.numpy())
    tg.update({k: w.grad.numpy() for k, w in dict(b_in=mha.in_proj_bias, Wo=mha.out_proj.weight, bo=mha.out_proj.bias, W1=fc1.weight,
                                                  b1=fc1.bias, W2=fc2.weight, b2=fc2.bias).items()})
    assert set(tg) == set(T._LAYER_KEYS)
    E3 = slice(E, 2 * E)                                               # the key bias: its gradient cancels in the softmax
    for k, ref in tg.items():
        if k == "b_in":
            assert np.abs(grads[k][E3]).max() < 1e-5 * np.abs(ref).max() and np.abs(ref[E3]).max() < 1e-12
        assert relerr(grads[k], ref) < 1e-5, k
