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


# ------------------------------------------------------------------ the float64 mode of the oracle, on its own
# tests/parity.py takes the bar for the product's gradients from the fp32 oracle's distance to the float64 oracle, so the
# float64 mode is validated here without leaning on the fp32 one: against float64 torch autograd on the same inputs, at 1e-11.
F64_RTOL = 1e-11


def _t64(a, grad=False):
    import torch
    return torch.tensor(np.asarray(a, np.float64), requires_grad=grad)


def _torch_attention_layer(p, x, tq, nb, ef, te, mask, H, drop):
    """TemporalAttentionLayer from plain float64 torch ops (temporal_attention.py:34-90 with nn.MultiheadAttention written
    out, so that a dropout multiplier can be put on the softmax weights); returns (out, leaves, parameters)."""
    import torch
    N, K = mask.shape
    E = 2 * x.shape[1]
    dh = E // H
    w = {k: _t64(v, True) for k, v in p.items()}
    tx, ttq, tnb, tte = _t64(x, True), _t64(tq, True), _t64(nb, True), _t64(te, True)
    q_in = torch.cat([tx, ttq], 1)
    key = torch.cat([tnb, _t64(ef), tte], 2)
    inv = torch.from_numpy(mask.all(1))
    pad = torch.from_numpy(mask.copy())
    pad[inv, 0] = False
    bq, bk, bv = w["b_in"][:E], w["b_in"][E:2 * E], w["b_in"][2 * E:]
    Q = (q_in @ w["Wq"].T + bq).reshape(N, H, dh) / np.sqrt(dh)
    Kp = (key @ w["Wk"].T + bk).reshape(N, K, H, dh)
    Vp = (key @ w["Wv"].T + bv).reshape(N, K, H, dh)
    s = torch.einsum("nhd,nkhd->nhk", Q, Kp).masked_fill(pad[:, None, :], float("-inf"))
    a = torch.softmax(s, -1)
    if drop is not None:
        a = a * _t64(drop)
    o = torch.einsum("nhk,nkhd->nhd", a, Vp).reshape(N, E)
    attn = (o @ w["Wo"].T + w["bo"]).masked_fill(inv[:, None], 0.0)
    h1 = torch.relu(torch.cat([attn, tx], 1) @ w["W1"].T + w["b1"])
    return h1 @ w["W2"].T + w["b2"], (tx, ttq, tnb, tte), w


def _l2rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64).reshape(np.shape(a))
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.mark.parametrize("D,Ef,H,K,pdrop", [(4, 0, 1, 3, 0.0), (4, 4, 4, 5, 0.5), (32, 4, 2, 64, 0.1), (32, 64, 1, 5, 0.0),
                                            (172, 64, 2, 8, 0.0), (172, 4, 4, 7, 0.3), (256, 0, 4, 6, 0.1), (256, 4, 2, 6, 0.0)])
def test_float64_attention_layer_against_torch_autograd(D, Ef, H, K, pdrop):
    """oracle attention_forward / attention_backward with dtype=float64 against float64 torch autograd: forward, the four input
    gradients and every parameter gradient within 1e-11, with rows that are all padding, partially masked rows, full rows, and
    (pdrop > 0) a dropout multiplier on the softmax weights.  Without dropout the torch side is nn.MultiheadAttention itself."""
    import torch
    rs = np.random.RandomState(7 * D + Ef + H)
    N, E, C = 29, 2 * D, 2 * D + Ef
    p = {k: v.astype(np.float64) for k, v in T.layer_params(T.init_params(D, Ef, 1, seed=D + K, use_memory=False), 0).items()}
    x, tq, go = rs.randn(N, D), rs.randn(N, D), rs.randn(N, D)
    nb, te, ef = rs.randn(N, K, D), rs.randn(N, K, D), rs.randn(N, K, Ef)
    n_valid = rs.randint(0, K + 1, N)
    n_valid[:4] = (0, 0, K, 1)
    mask = np.arange(K)[None, :] < (K - n_valid)[:, None]
    assert mask.all(1).sum() >= 2 and (~mask).all(1).any() and (mask.any(1) & ~mask.all(1)).any()
    drop = None
    if pdrop > 0:
        drop = ((rs.rand(N, H, K) >= pdrop) / (1 - pdrop)).astype(np.float32)
        assert (drop == 0).any() and (drop > 0).any()
    out, c = T.attention_forward(p, x, tq, nb, ef, te, mask, H, drop, dtype=np.float64)
    assert out.dtype == np.float64 and c["z1"].dtype == np.float64
    grads, dx, dtq, dnb, dte = T.attention_backward(p, c, go, H, D)
    assert all(v.dtype == np.float64 for v in grads.values()) and dx.dtype == np.float64
    want, (tx, ttq, tnb, tte), w = _torch_attention_layer(p, x, tq, nb, ef, te, mask, H, drop)
    want.backward(_t64(go))
    assert relerr(out, want.detach().numpy()) < F64_RTOL and row_relerr(out, want.detach().numpy()) < F64_RTOL
    for mine, theirs, what in ((dx, tx, "dx"), (dtq, ttq, "dtq"), (dnb, tnb, "dnb"), (dte, tte, "dte")):
        assert relerr(mine, theirs.grad.numpy()) < F64_RTOL and _l2rel(mine, theirs.grad.numpy()) < F64_RTOL, what
    E3 = slice(E, 2 * E)                                               # the key bias: its gradient cancels in the softmax
    for k in T._LAYER_KEYS:
        ref = w[k].grad.numpy()
        if k == "b_in":
            assert np.abs(grads[k][E3]).max() < F64_RTOL * np.abs(ref).max()
            ref = ref.copy(); ref[E3] = grads[k][E3]
        assert relerr(grads[k], ref) < F64_RTOL and _l2rel(grads[k], ref) < F64_RTOL, k
    if drop is None:                                                   # and the written-out torch layer is nn.MultiheadAttention's
        mha = torch.nn.MultiheadAttention(embed_dim=E, kdim=C, vdim=C, num_heads=H).double()
        with torch.no_grad():
            if mha.q_proj_weight is None:
                mha.in_proj_weight.copy_(_t64(np.concatenate([p["Wq"], p["Wk"], p["Wv"]])))
            else:
                for dst, src in ((mha.q_proj_weight, "Wq"), (mha.k_proj_weight, "Wk"), (mha.v_proj_weight, "Wv")):
                    dst.copy_(_t64(p[src]))
            for dst, src in ((mha.in_proj_bias, "b_in"), (mha.out_proj.weight, "Wo"), (mha.out_proj.bias, "bo")):
                dst.copy_(_t64(p[src]))
        inv = torch.from_numpy(mask.all(1))
        pad = torch.from_numpy(mask.copy())
        pad[inv, 0] = False
        attn, _ = mha(query=torch.cat([_t64(x), _t64(tq)], 1).unsqueeze(0), key=torch.cat([_t64(nb), _t64(ef), _t64(te)], 2).permute(1, 0, 2),
                      value=torch.cat([_t64(nb), _t64(ef), _t64(te)], 2).permute(1, 0, 2), key_padding_mask=pad)
        attn = attn.squeeze(0).masked_fill(inv[:, None], 0.0)
        h1 = torch.relu(torch.cat([attn, _t64(x)], 1) @ _t64(p["W1"]).T + _t64(p["b1"]))
        assert relerr(out, (h1 @ _t64(p["W2"]).T + _t64(p["b2"])).detach().numpy()) < F64_RTOL


@pytest.mark.parametrize("D,Ef", [(4, 0), (32, 4), (172, 64), (256, 4), (256, 0)])
def test_float64_gru_cell_against_torch_autograd(D, Ef):
    """oracle gru_cell / gru_cell_backward with dtype=float64 against torch.nn.GRUCell in float64: new memory and the four
    parameter gradients within 1e-11 (message row 3 D + Ef wide)."""
    import torch
    rs = np.random.RandomState(D + Ef)
    n, M = 23, 3 * D + Ef
    P = T.init_params(D, Ef, 1, seed=D, use_memory=True)
    pre = "memory_updater.memory_updater."
    W = [P[pre + k].astype(np.float64) for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    x, h, ghn = rs.randn(n, M), rs.randn(n, D), rs.randn(n, D)
    hn, cache = T.gru_cell(x, h, *W, dtype=np.float64)
    assert hn.dtype == np.float64
    g = T.gru_cell_backward(cache, ghn, W[0], W[1], dtype=np.float64)
    cell = torch.nn.GRUCell(M, D).double()
    with torch.no_grad():
        for dst, src in zip((cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh), W):
            dst.copy_(_t64(src))
    want = cell(_t64(x), _t64(h))
    want.backward(_t64(ghn))
    assert relerr(hn, want.detach().numpy()) < F64_RTOL and row_relerr(hn, want.detach().numpy()) < F64_RTOL
    for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
        ref = getattr(cell, k).grad.numpy()
        assert g[k].dtype == np.float64 and relerr(g[k], ref) < F64_RTOL and _l2rel(g[k], ref) < F64_RTOL, k


@pytest.mark.parametrize("D,q", [(4, 1), (32, 3), (172, 3), (256, 5)])
def test_float64_bpr_against_torch_autograd(D, q):
    """oracle bpr_loss / bpr_loss_backward with dtype=float64 against float64 torch autograd of main.py:321-337 (sigma of the
    MEAN score difference): loss and the three embedding gradients within 1e-11."""
    import torch
    rs = np.random.RandomState(D + q)
    B = 17
    src, pos, neg = rs.randn(B, D) * 0.3, rs.randn(B, 1, D) * 0.3, rs.randn(B, q, D) * 0.3
    loss, cache = T.bpr_loss(src, pos, neg, dtype=np.float64)
    ds, dp, dn = T.bpr_loss_backward(cache)
    assert type(loss) is np.float64 and ds.dtype == np.float64
    ts, tp, tn = _t64(src, True), _t64(pos, True), _t64(neg, True)
    diff = torch.einsum("bd,bpd->bp", ts, tp) - torch.einsum("bd,bqd->bq", ts, tn)
    want = -torch.log(torch.sigmoid(diff.mean(1))).mean()
    want.backward()
    assert abs(loss - want.item()) < F64_RTOL * abs(want.item())
    for mine, theirs, what in ((ds, ts, "src"), (dp, tp, "pos"), (dn, tn, "neg")):
        assert relerr(mine, theirs.grad.numpy()) < F64_RTOL and _l2rel(mine, theirs.grad.numpy()) < F64_RTOL, what


def test_float64_time_encoder_keeps_the_fp32_argument():
    """The time-encoder argument is one fp32 FMA in both modes (a contract rounding, not evaluation noise): the float64 mode is
    the float64 cosine / sine of exactly that fp32 argument, and its gradients are float64 sums of float64 terms."""
    rs = np.random.RandomState(3)
    D = 32
    t = (rs.rand(200) * 1e7).astype(np.float32)
    w = (1 / 10 ** np.linspace(0, 9, D)).astype(np.float32)
    b = (rs.randn(D) * 0.3).astype(np.float32)
    arg = T.fmaf(t[:, None], w, b)
    assert arg.dtype == np.float32
    y = T.time_encode(t, w, b, dtype=np.float64)
    assert y.dtype == np.float64 and np.array_equal(y, np.cos(arg.astype(np.float64)))
    assert np.abs(y - T.time_encode(t, w, b)).max() < 5e-7            # the fp32 mode: cosf of the same argument
    g = rs.randn(200, D)
    gw, gb = T.time_encode_backward(t, w, b, g, dtype=np.float64)
    s = -np.sin(arg.astype(np.float64)) * g
    assert gw.dtype == np.float64 and np.allclose(gw, (s * t[:, None].astype(np.float64)).sum(0), rtol=1e-13, atol=0)
    assert np.allclose(gb, s.sum(0), rtol=1e-13, atol=1e-300)


# ------------------------------------------------------------------ what the per-tensor bar lets through and the block bar does not
_SENS = {}


def _sensitivity_grads(which):
    """(fp32 oracle gradients, float64 oracle gradients, D, Ef, H) of one training step with the near-kink roots left out on
    both sides, computed once per session.  "f": the last step of case f of test_gpu_config_edges (D 172, Ef 64, H 2).
    "scaled": the shape and graph of the "scaled" row of test_step_against_oracle (D 172, H 2, L 2, K 8, memory) on the oracle's
    own initialiser, with the weight blocks moved 2^9-2^10 apart by that row's factors; third step, so the GRU has messages."""
    if which in _SENS:
        return _SENS[which]
    from parity import _near_kink_roots, f64_twin, _f64_backward
    if which == "f":
        import test_gpu_config_edges as CE
        c = CE._Inputs("f")
        ref, D, Ef, H, K, B, n_neg = c.oracle(), c.D, c.Ef, c.H, c.K, c.B, CE.N_NEG
        steps = [(sb, db, tb, eb, neg) for sb, db, tb, eb, neg, _ in c.steps]
    else:
        from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
        D, Ef, H, L, K, B, n_neg = 172, 4, 2, 2, 8, 40, 3
        cfg = SyntheticConfig("t", 300, 25, 5000, D, L, K, H)
        g = make_graph(cfg, with_prices=False)
        d = g.data
        P = T.init_params(D, Ef, L, seed=3)
        P["memory_updater.memory_updater.weight_ih"] *= np.float32(2.0 ** 3)
        P["memory_updater.memory_updater.weight_hh"] *= np.float32(2.0 ** -6)
        for l in range(L):
            pre = "embedding_module.attention_models.%d." % l
            P[pre + "merger.fc1.weight"][:, :2 * D] *= np.float32(2.0 ** 2)
            P[pre + "merger.fc1.weight"][:, 2 * D:] *= np.float32(2.0 ** -8)
            P[pre + "merger.fc2.weight"] *= np.float32(2.0 ** -4)
            P[pre + "multi_head_target.q_proj_weight"] *= np.float32(2.0 ** 2)
        onf = OracleNeighborFinder(*build_adjacency(d.sources, d.destinations, d.edge_idxs, d.timestamps))
        ref = T.OracleTGN(onf, g.node_features, g.edge_features, P, L, H, True)
        rs = np.random.RandomState(5)
        steps = []
        for s in (2500, 2540, 2580):
            steps.append((d.sources[s:s + B], d.destinations[s:s + B], d.timestamps[s:s + B], d.edge_idxs[s:s + B],
                          rs.randint(cfg.n_users + 1, cfg.n_users + cfg.n_items + 1, size=B * n_neg)))
    ref64 = f64_twin(ref)
    for i, (sb, db, tb, eb, neg) in enumerate(steps):
        if i == len(steps) - 1:
            ref64.load_state(ref)
            e64 = ref64.compute_temporal_embeddings(sb, db, neg, tb, eb, K)
        rse, rde, rne = ref.compute_temporal_embeddings(sb, db, neg, tb, eb, K)
    _, cache = T.bpr_loss(rse, rde.reshape(B, 1, -1), rne.reshape(B, n_neg, -1))
    W = np.concatenate([a.reshape(-1, D) for a in T.bpr_loss_backward(cache)])
    bad = _near_kink_roots(ref._ctx, len(W), K)
    assert bad.mean() <= 0.10
    W[bad] = 0
    g32 = ref.backward(W)
    g64 = _f64_backward(ref64, ref, e64, B, K, n_neg=n_neg)
    _SENS[which] = (g32, g64, D, Ef, H)
    return _SENS[which]


# which step, tensor, and what is done to that tensor's fp32-oracle gradient.  Each stands for one way a block goes wrong: a
# block a fraction of a per cent off, a small block entirely wrong, a gate block off by a quarter.  (Zeroing fc1's node half
# and swapping b_hh's r and z rows were tried first: they move the whole tensor by 0.19 and 0.64 and the per-tensor bar
# catches them, so they show nothing about it.  The blocks below are the small ones of their tensors: W_ih's r-gate edge
# columns hold 0.0017 of its gradient norm in the "scaled" step and b_hh's r third 0.0115.)
CORRUPTIONS = {
    # (half a per cent: at Ef = 64 the edge columns hold 0.72 of Wk's gradient norm, and a whole per cent on them is 7.2e-3 of the tensor)
    "Wk Ef columns x 1.005": ("f", "embedding_module.attention_models.1.multi_head_target.k_proj_weight",
                              lambda g, D, Ef: g.__setitem__((slice(None), slice(D, D + Ef)), g[:, D:D + Ef] * np.float32(1.005))),
    "W_ih r-gate Ef block zeroed (scaled)": ("scaled", "memory_updater.memory_updater.weight_ih",
                                             lambda g, D, Ef: g.__setitem__((slice(0, D), slice(2 * D, 2 * D + Ef)), 0)),
    "b_hh r third x 1.25 (scaled)": ("scaled", "memory_updater.memory_updater.bias_hh",
                                     lambda g, D, Ef: g.__setitem__(slice(0, D), g[:D] * np.float32(1.25))),
}


@pytest.mark.parametrize("what", sorted(CORRUPTIONS))
def test_block_bar_catches_what_the_tensor_bar_lets_through(what):
    """One block of the fp32 oracle's own gradient is corrupted; every other element keeps the oracle's value.  The per-tensor
    relative L2 against the float64 oracle stays under 5e-3 (the old measure passes the corrupted tensor), the block measure
    puts that block over GRAD_MARGIN x e32 - and the uncorrupted tensor passes both."""
    from parity import RTOL_GRAD_ORACLE_L2, check_grad_blocks
    which, name, corrupt = CORRUPTIONS[what]
    g32, g64, D, Ef, H = _sensitivity_grads(which)
    clean = {name: g32[name].astype(np.float64)}
    _, over = check_grad_blocks(clean, g32, g64, D, Ef, H)
    assert not over, over
    g = g32[name].copy()
    corrupt(g, D, Ef)
    assert not np.array_equal(g, g32[name])
    tensor_err = np.linalg.norm(g.astype(np.float64) - g64[name]) / np.linalg.norm(g64[name])
    assert tensor_err < RTOL_GRAD_ORACLE_L2, (what, tensor_err)           # the old per-tensor bar lets it through
    worst, over = check_grad_blocks({name: g.astype(np.float64)}, g32, g64, D, Ef, H)
    assert over and worst[0] > 1, (what, worst)                            # the block bar does not
    print("%s: tensor L2 %.3g (bar %.3g); %d block(s) over, worst %s[%s] %.3g = %.3g x its bar" % (
        what, tensor_err, RTOL_GRAD_ORACLE_L2, len(over), worst[1], worst[2], worst[3], worst[0]))
