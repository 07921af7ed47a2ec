"""The MLP message function without a GPU: the host model (tests/message_ref.py) against the reference's own steps (g11), the
constructor and the state dict with the reference's two names per tensor, the flat-buffer layout, and the refusals."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden

import pfotgnrec_amd as P
from pfotgnrec_amd import _lib
from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
from oracle import tgn_oracle as T
from oracle.neighbor_finder import OracleNeighborFinder, build_adjacency
from parity import relerr, row_relerr, ROW_RTOL, KINK_THR
import message_ref as MR

RTOL = 1e-4          # the bars test_oracle_golden_model.py holds the oracle to on g5
RTOL_GRAD = 5e-4
FIXTURES = ["g11_step_L1_mem_mlp", "g11_step_L2_mem_mlp"]


@pytest.mark.parametrize("fixture", FIXTURES)
def test_host_model_against_reference_golden(fixture):
    g = load_golden(fixture)
    L, H, K = int(g["L"]), int(g["H"]), int(g["K"])
    assert bool(g["use_memory"]) and not bool(g["uniform"]) and str(g["path"]) == "base"
    assert float(g["mlp_min_abs_preact"]) >= KINK_THR                 # no hidden unit of the reference's run sits at its kink
    assert len(g["recorded_steps"]) >= 2 and np.all(np.diff(g["recorded_steps"]) == 1)
    nf = OracleNeighborFinder(*build_adjacency(g["src_all"], g["dst_all"], g["eidx_all"], g["ts_all"]), uniform=False)
    pre0 = "s%d_" % g["recorded_steps"][0]
    params = {k[len(pre0 + "sd_"):]: g[k] for k in g.files if k.startswith(pre0 + "sd_")}
    ref = MR.MlpOracleTGN(nf, g["node_features"], g["edge_features"], params, L, H)
    worst = {}

    def note(key, e):
        worst[key] = max(worst.get(key, 0.0), float(e))
        return e
    for step in g["recorded_steps"]:
        pre = "s%d_" % step
        MR.load_golden_state(g, pre, ref)
        sb, db, tb, eb, neg = g[pre + "src"], g[pre + "dst"], g[pre + "ts"], g[pre + "eidx"], g[pre + "neg"]
        B = len(sb)
        se, de, ne = ref.compute_temporal_embeddings(sb, db, neg.flatten(), tb, eb, K)
        ids, pre_act, _ = ref.mlp_rows()
        assert len(ids) > 0 and np.abs(pre_act).min() >= 0.5 * float(g["mlp_min_abs_preact"])
        for got, key in ((se, "emb_src"), (de, "emb_dst"), (ne, "emb_neg")):
            assert note("emb relerr", relerr(got, g[pre + key])) < RTOL, (step, key)
            assert note("emb row_relerr", row_relerr(got, g[pre + key])) < ROW_RTOL, (step, key)
        loss, cache = T.bpr_loss(se, de.reshape(B, 1, -1), ne.reshape(B, 3, -1))
        assert abs(loss - g[pre + "loss"]) < 1e-5 * max(1.0, abs(g[pre + "loss"]))
        d_src, d_pos, d_neg = T.bpr_loss_backward(cache)
        grads = ref.backward(np.concatenate([d_src, d_pos.reshape(B, -1), d_neg.reshape(3 * B, -1)]))
        seen = set()
        for k in g.files:
            if not k.startswith(pre + "grad_"):
                continue
            name = k[len(pre + "grad_"):]
            if "layer_norm" in name or name.startswith("memory."):
                continue
            want = g[k]
            got = grads[name].reshape(want.shape)
            seen.add(name)
            if np.abs(want).max() == 0:
                assert np.abs(got).max() < 1e-7, name
                continue
            assert note("grad relerr", relerr(got, want)) < RTOL_GRAD, (step, name, relerr(got, want))
        assert set(MR.MLP_NAMES) <= seen                              # parameters() yields each MLP tensor once, under .mlp
        assert not any(n.startswith(MR.ALIAS) for n in seen)
        assert all(np.abs(g[pre + "grad_" + n]).max() > 0 for n in MR.MLP_NAMES)
        assert note("memory relerr", relerr(ref.memory, g[pre + "after_memory"])) < RTOL
        assert note("memory row_relerr", row_relerr(ref.memory, g[pre + "after_memory"])) < ROW_RTOL
        assert np.array_equal(ref.last_update, g[pre + "after_last_update"])
        tab, mt, has = ref.pending_table()
        assert np.array_equal(has, g[pre + "after_msg_cnt"] > 0)
        assert note("msg relerr", relerr(tab, g[pre + "after_msg_tab"])) < RTOL
        assert np.array_equal(mt, g[pre + "after_msg_t"])
    print("FIGURES %s: %s" % (fixture, ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))


def test_host_model_float64_twin_and_injected_relu_mask():
    """The float64 twin evaluates the same function; a ReLU mask handed to backward replaces the forward's own decisions."""
    cfg = SyntheticConfig("t", 40, 10, 500, 8, 1, 4, 2)
    gr = make_graph(cfg, with_prices=False)
    d = gr.data
    nf = OracleNeighborFinder(*build_adjacency(d.sources, d.destinations, d.edge_idxs, d.timestamps))
    ref = MR.MlpOracleTGN(nf, gr.node_features, gr.edge_features, MR.init_params(8, gr.edge_features.shape[1], 1, 12), 1, 2)
    ref64 = MR.f64_twin(ref)
    assert isinstance(ref64, MR.MlpOracleTGN) and ref64.dtype is np.float64
    rs = np.random.RandomState(0)
    for step in range(3):
        s = 200 + 16 * step
        args = (d.sources[s:s + 16], d.destinations[s:s + 16], rs.randint(cfg.n_users + 1, cfg.n_users + cfg.n_items + 1, 48),
                d.timestamps[s:s + 16], d.edge_idxs[s:s + 16], 4)
        ref64.load_state(ref)
        e64 = np.concatenate(ref64.compute_temporal_embeddings(*args))
        e32 = np.concatenate(ref.compute_temporal_embeddings(*args))
        assert e64.dtype == np.float64 and relerr(e32, e64) < 1e-5
        w = rs.randn(*e32.shape)
        g32, g64 = ref.backward(w.astype(np.float32)), ref64.backward(w)
        ids, pre_act, hid = ref.mlp_rows()
        if step == 0:
            assert len(ids) == 0 and all(np.abs(g32[n]).max() == 0 for n in MR.MLP_NAMES)     # no pending message anywhere
            continue
        for n in MR.MLP_NAMES + [MR.GRU + "weight_ih"]:
            assert np.abs(g64[n]).max() > 0 and relerr(g32[n], g64[n]) < 1e-4, n
        same = ref.backward(w.astype(np.float32), relu_mask=pre_act > 0)
        assert all(np.array_equal(same[n], g32[n]) for n in g32)
        flipped = ref.backward(w.astype(np.float32), relu_mask=np.ones_like(pre_act, bool))
        assert not np.array_equal(flipped[MR.MLP + "0.weight"], g32[MR.MLP + "0.weight"])
        assert np.array_equal(flipped[MR.MLP + "2.weight"], g32[MR.MLP + "2.weight"])         # d W2 does not pass the ReLU


@pytest.mark.parametrize("fixture", FIXTURES)
def test_constructor_accepts_mlp_and_matches_the_reference_state_dict(fixture):
    g = load_golden(fixture)
    L, D = int(g["L"]), g["node_features"].shape[1]
    nf = P.NeighborFinder.from_arrays(g["src_all"], g["dst_all"], g["eidx_all"], g["ts_all"], uniform=False)
    tgn = P.TGN(nf, g["node_features"], g["edge_features"], "cpu", n_layers=L, n_heads=int(g["H"]), use_memory=True,
                memory_dimension=D, message_function="mlp", message_dimension=100)
    sd = tgn.state_dict()
    pre = "s%d_sd_" % g["recorded_steps"][0]
    ref_shapes = {k[len(pre):]: g[k].shape for k in g.files if k.startswith(pre)}
    mine = {k: tuple(v.shape) for k, v in sd.items()}
    assert set(ref_shapes) <= set(mine), sorted(set(ref_shapes) - set(mine))      # every name the fixture recorded exists here
    for name, shape in ref_shapes.items():
        if name.startswith(("message_function.", "memory_updater.memory_updater.", "embedding_module.attention_models.", "time_encoder.")):
            assert mine.get(name) == tuple(shape), (name, mine.get(name), shape)
    assert {k for k in ref_shapes if k.startswith("message_function.")} == {k for k in mine if k.startswith("message_function.")}
    assert len([k for k in mine if k.startswith("message_function.")]) == 8
    M = 3 * D + tgn.n_edge_features
    assert mine["message_function.mlp.0.weight"] == (M // 2, M) and mine["memory_updater.memory_updater.weight_ih"] == (3 * D, 100)
    for t in ("0.weight", "0.bias", "2.weight", "2.bias"):
        assert sd[MR.MLP + t].data_ptr() == sd[MR.ALIAS + t].data_ptr()                     # one tensor, two names
    names = [n for n, _ in tgn.named_parameters()]
    assert len(names) == len(set(id(p) for p in tgn.parameters()))
    assert sum(n.startswith("message_function.") for n in names) == 4                       # parameters() yields each once
    flat = tgn.flat_parameters
    lo, hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * 4
    for n, p in tgn.named_parameters():
        if "layer_norm" in n or n.startswith("memory."):
            continue
        assert lo <= p.data_ptr() and p.data_ptr() + p.numel() * 4 <= hi, n
    # a reference checkpoint loads strictly, and lands in the flat buffer
    ck = {k: torch.from_numpy(np.array(g[pre + k])) for k in ref_shapes if k in sd}
    for k in sd:
        ck.setdefault(k, sd[k].clone())
    tgn.load_state_dict(ck, strict=True)
    lay = tgn._layout
    w1 = g[pre + MR.MLP + "0.weight"]
    assert np.array_equal(flat[lay.mlp_w1:lay.mlp_w1 + w1.size].numpy().reshape(w1.shape), w1)
    w2 = g[pre + MR.ALIAS + "2.weight"]
    assert np.array_equal(flat[lay.mlp_w2:lay.mlp_w2 + w2.size].numpy().reshape(w2.shape), w2)


def test_constructor_honours_message_dimension_only_for_mlp_and_refuses_the_rest():
    gr = make_graph(SyntheticConfig("t", 30, 8, 300, 8, 1, 4, 2), with_prices=False)
    nf = P.get_neighbor_finder(gr.data, False)
    kw = dict(n_layers=1, n_heads=2, use_memory=True, memory_dimension=8)
    ident = P.TGN(nf, gr.node_features, gr.edge_features, "cpu", message_function="identity", message_dimension=100, **kw)
    M = 3 * 8 + ident.n_edge_features
    assert tuple(ident.memory_updater.memory_updater.weight_ih.shape) == (24, M) and ident.message_dimension == M    # tgn.py:66
    assert not any(k.startswith("message_function.") for k in ident.state_dict())
    assert (ident._cfg.msg_dim, ident._cfg.msg_hidden) == (0, 0)
    mlp = P.TGN(nf, gr.node_features, gr.edge_features, "cpu", message_function="mlp", message_dimension=12, **kw)
    assert tuple(mlp.memory_updater.memory_updater.weight_ih.shape) == (24, 12) and mlp.memory.message_dimension == 12
    assert (mlp._cfg.msg_dim, mlp._cfg.msg_hidden) == (12, M // 2)
    assert tuple(mlp.memory.msg_table.shape) == (gr.n_nodes, M)            # the raw message table keeps its width
    default = P.TGN(nf, gr.node_features, gr.edge_features, "cpu", **kw)   # the reference's own defaults: mlp, 100
    assert tuple(default.memory_updater.memory_updater.weight_ih.shape) == (24, 100)
    with pytest.raises(ValueError, match="multiple of 4"):
        P.TGN(nf, gr.node_features, gr.edge_features, "cpu", message_function="mlp", message_dimension=10, **kw)
    with pytest.raises(ValueError, match="not implemented"):
        P.TGN(nf, gr.node_features, gr.edge_features, "cpu", message_function="attention", **kw)
    # nn.Linear's initialiser: uniform within 1 / sqrt(fan_in)
    lin0 = getattr(default.message_function.mlp, "0")
    assert lin0.weight.abs().max().item() <= 1 / np.sqrt(M) + 1e-6 and lin0.weight.abs().max().item() > 0.5 / np.sqrt(M)
    assert lin0.bias.abs().max().item() <= 1 / np.sqrt(M) + 1e-6 and lin0.bias.abs().sum().item() > 0


def _layout(*cfg_args):
    cfg = _lib.TgnConfig(*cfg_args)
    lay = _lib.TgnLayout()
    rc = _lib.load().pfo_tgn_param_layout(ctypes.byref(cfg), ctypes.byref(lay))
    return rc, cfg, lay


def test_layout_places_the_block_between_the_gru_and_layer_one():
    D, Ef, md = 32, 4, 100
    M, Hm = 3 * D + Ef, (3 * D + Ef) // 2
    rc, cfg, lay = _layout(200, 50, D, Ef, 2, 2, 1, 8, 4, 4, md, Hm)
    assert rc == 0
    assert lay.gru_w_hh - lay.gru_w_ih == 3 * D * md                        # weight_ih is [3D, msg_dim]
    assert lay.gru_b_hh + 3 * D == lay.mlp_w1
    assert (lay.mlp_b1 - lay.mlp_w1, lay.mlp_w2 - lay.mlp_b1, lay.mlp_b2 - lay.mlp_w2) == (Hm * M, 52, md * Hm)   # (b1: 50 floats, padded to 52)
    assert all(o % 4 == 0 for o in (lay.mlp_w1, lay.mlp_b1, lay.mlp_w2, lay.mlp_b2, lay.layer[0].wq))
    assert lay.mlp_b2 + md <= lay.layer[0].wq <= lay.mlp_b2 + md + 3
    split = ctypes.c_int64(0)
    assert _lib.load().pfo_tgn_grad_split(ctypes.byref(cfg), ctypes.byref(split)) == 0
    assert split.value == lay.layer[1].wq and lay.mlp_b2 < split.value      # the MLP's gradients finish last, with the GRU's
    rc1, cfg1, lay1 = _layout(200, 50, D, Ef, 1, 2, 1, 8, 4, 4, md, Hm)
    assert _lib.load().pfo_tgn_grad_split(ctypes.byref(cfg1), ctypes.byref(split)) == 0 and split.value == lay1.total
    # C2: every tensor is a multiple of 4 floats long, nothing is padded
    rc, cfg, lay = _layout(50501, 1000001, 172, 4, 2, 2, 1, 2560, 20, 512, 100, 260)
    per_layer = 596152
    assert rc == 0 and lay.total == 344 + (516 * 100 + 516 * 172 + 2 * 516) + (260 * 520 + 260 + 100 * 260 + 100) + 2 * per_layer
    lib = _lib.load()
    assert lib.pfo_tgn_workspace_bytes(ctypes.byref(cfg)) > 0 and lib.pfo_tgn_pcache_bytes(ctypes.byref(cfg)) > 0


def test_identity_configs_keep_their_layout_and_sizes():
    lib = _lib.load()
    ten = (50501, 1000001, 172, 4, 2, 2, 1, 2560, 20, 512)
    rc, cfg, lay = _layout(*ten)                                            # ten positional values: the rest is zero
    assert rc == 0 and (cfg.msg_dim, cfg.msg_hidden) == (0, 0)
    assert (lay.mlp_w1, lay.mlp_b1, lay.mlp_w2, lay.mlp_b2) == (-1, -1, -1, -1)
    assert lay.total == 344 + 358104 + 2 * 596152                           # test_abi's pinned figure
    ws, pc = lib.pfo_tgn_workspace_bytes(ctypes.byref(cfg)), lib.pfo_tgn_pcache_bytes(ctypes.byref(cfg))
    rc, cfg_h, lay_h = _layout(*ten, 0, 260)                                # msg_hidden is ignored without msg_dim
    assert rc == 0 and lay_h.total == lay.total and lay_h.mlp_w1 == -1
    rc, cfg_m, lay_m = _layout(*ten, 100, 260)
    assert rc == 0 and lay_m.total > lay.total - 516 * 420
    assert lib.pfo_tgn_workspace_bytes(ctypes.byref(cfg_h)) == ws and lib.pfo_tgn_pcache_bytes(ctypes.byref(cfg_h)) == pc
    assert lib.pfo_tgn_workspace_bytes(ctypes.byref(cfg_m)) > ws and lib.pfo_tgn_pcache_bytes(ctypes.byref(cfg_m)) > pc
    zeroed = _lib.TgnConfig()                                               # zeroed memory with the old fields filled in
    for name, v in zip(("n_nodes", "n_edges_p1", "D", "Ef", "n_layers", "n_heads", "use_memory", "max_roots", "max_neighbors", "max_batch"), ten):
        setattr(zeroed, name, v)
    lay_z = _lib.TgnLayout()
    assert lib.pfo_tgn_param_layout(ctypes.byref(zeroed), ctypes.byref(lay_z)) == 0 and lay_z.total == lay.total
    rc, _, lay_nomem = _layout(200, 50, 16, 4, 1, 2, 0, 8, 4, 4)
    assert rc == 0 and lay_nomem.mlp_w1 == -1 and lay_nomem.gru_w_ih == -1


@pytest.mark.parametrize("extra,word", [((10, 50), "msg_dim must be a multiple of 4"), ((-4, 50), "msg_dim must be a multiple of 4"),
                                        ((100, 0), "msg_hidden"), ((100, -3), "msg_hidden")])
def test_bad_message_sizes_are_refused_with_a_message(extra, word):
    lib = _lib.load()
    cfg = _lib.TgnConfig(200, 50, 32, 4, 1, 2, 1, 8, 4, 4, *extra)
    lay = _lib.TgnLayout()
    assert lib.pfo_tgn_param_layout(ctypes.byref(cfg), ctypes.byref(lay)) == -1 and word.encode() in lib.pfo_last_error()
    assert lib.pfo_tgn_workspace_bytes(ctypes.byref(cfg)) == -1
    with pytest.raises(_lib.PfoError, match=word):
        _lib.call("pfo_tgn_param_layout", ctypes.byref(cfg), ctypes.byref(lay))


def test_mlp_without_memory_is_refused_at_the_abi():
    lib = _lib.load()
    cfg = _lib.TgnConfig(200, 50, 32, 4, 1, 2, 0, 8, 4, 4, 100, 50)
    lay = _lib.TgnLayout()
    assert lib.pfo_tgn_param_layout(ctypes.byref(cfg), ctypes.byref(lay)) == -1 and b"use_memory" in lib.pfo_last_error()


def test_gru_probe_refuses_an_unknown_gather_form_before_any_launch():
    lib = _lib.load()
    Pn = 1 << 12                                                            # a 16-byte aligned address that is never followed
    f = _lib.GruDesc(K_msg=12, D=8, cap_rows=5, gather=3)
    for name in ("msg_rows", "h_rows", "img_ih", "img_hh", "b_ih", "b_hh", "hm", "touched", "node_feat", "upd_mem", "h0_tab", "gates", "n_rows"):
        setattr(f, name, Pn)
    assert lib.pfo_debug_gru_fused(ctypes.byref(f), None) == -1 and b"gather must be 0, 1 or 2" in lib.pfo_last_error()


def _mlp_probe_refusals():
    Pn = 1 << 12                                                            # a 16-byte aligned address that is never followed
    fwd = dict(raw=Pn, ld_raw=28, hm=Pn, img_w1=Pn, img_w2=Pn, b1=Pn, b2=Pn, msg_out=Pn, Mr=28, Hm=14, Md=4, cap_rows=5, n_rows=Pn)
    bwd = dict(dgi=Pn, hid=Pn, img_wihT=Pn, img_w2T=Pn, d_m=Pn, d_hid=Pn, D3=24, Hm=14, Md=4, cap_rows=5, n_rows=Pn)
    return [("fwd-null-out", "fwd", dict(fwd, msg_out=None), "null argument"), ("fwd-null-image", "fwd", dict(fwd, img_w2=None), "null argument"),
            ("fwd-null-hm", "fwd", dict(fwd, hm=None), "null argument"), ("fwd-message-width", "fwd", dict(fwd, Md=6), "bad sizes"),
            ("fwd-raw-width", "fwd", dict(fwd, Mr=30, ld_raw=30), "bad sizes"), ("fwd-short-rows", "fwd", dict(fwd, ld_raw=24), "bad sizes"),
            ("fwd-no-rows", "fwd", dict(fwd, cap_rows=0), "bad sizes"), ("fwd-misaligned-raw", "fwd", dict(fwd, raw=Pn + 4), "16-byte aligned"),
            ("fwd-misaligned-out", "fwd", dict(fwd, msg_out=Pn + 8), "16-byte aligned"),
            ("bwd-null-out", "bwd", dict(bwd, d_hid=None), "null argument"), ("bwd-null-hid", "bwd", dict(bwd, hid=None), "null argument"),
            ("bwd-message-width", "bwd", dict(bwd, Md=6), "bad sizes"), ("bwd-gate-width", "bwd", dict(bwd, D3=26), "bad sizes"),
            ("bwd-no-rows", "bwd", dict(bwd, cap_rows=0), "bad sizes"), ("bwd-wide-message", "bwd", dict(bwd, Md=132), "beyond 128"),
            ("bwd-misaligned-dm", "bwd", dict(bwd, d_m=Pn + 4), "16-byte aligned"), ("bwd-misaligned-dgi", "bwd", dict(bwd, dgi=Pn + 4), "16-byte aligned")]


@pytest.mark.parametrize("cid,which,fields,word", _mlp_probe_refusals(), ids=[c[0] for c in _mlp_probe_refusals()])
def test_fused_mlp_launchers_refuse_bad_arguments_before_any_launch(cid, which, fields, word):
    lib = _lib.load()
    desc = (_lib.MsgMlpDesc if which == "fwd" else _lib.MsgMlpBwdDesc)(**fields)
    probe = "pfo_debug_msg_mlp_fwd" if which == "fwd" else "pfo_debug_msg_mlp_bwd"
    assert getattr(lib, probe)(ctypes.byref(desc), None) == -1 and word.encode() in lib.pfo_last_error(), lib.pfo_last_error()
    assert getattr(lib, probe)(None, None) == -1
