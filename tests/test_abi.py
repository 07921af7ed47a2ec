"""CPU-side checks of the boundary: the library loads and exports every symbol include/pfotgn.h declares."""
import os
import re

import numpy as np
import pytest

from conftest import REPO


def _declared_symbols():
    text = open(os.path.join(REPO, "include", "pfotgn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pfo_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from pfotgnrec_amd import _lib
    lib = _lib.load()
    declared = _declared_symbols()
    assert len(declared) >= 14
    for name in declared:
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES, "no ctypes prototype for %s" % name
    assert lib.pfo_abi_version() == 6


def test_attention_form_query_follows_the_shape_table():
    """pfo_debug_attn_form is pure host code over the descriptor (pointers are only tested for null and alignment, never
    followed): every shape of tests/attn_ref.py reports the kernel DESIGN.md's table names for it, a descriptor the common
    checks refuse reports -1 with the message, and the size queries answer."""
    import ctypes
    from pfotgnrec_amd import _lib
    import attn_ref as R
    lib = _lib.load()
    P = 1 << 12                                                           # any 16-byte aligned non-null address

    def desc(D, Ef, H, K=7, N=13, table=False, d_nbr=False, det=0, members=False, qk=P, nbr_ld=None):
        d = _lib.AttnDesc(N=N, K=K, D=D, Ef=Ef, H=H, Cp=R.cp_of(D, Ef), nbr_ld=nbr_ld or D, nbr_rows=N * K + 8, edge_rows=18, det=det)
        for f in ("nbr_tab", "nbr_ids", "eidx", "dt", "tw", "tb", "ctx", "attw", "inv", "edge_feat", "dctx", "dQK"):
            setattr(d, f, P)
        d.QK = qk
        if table:
            d.nbr_row = P
        if d_nbr:
            d.d_nbr = P
        if members:
            for f in ("members", "seg_ptr", "n_rows", "run_cnt", "dqk_live", "qk_row"):
                setattr(d, f, P)
        return d

    def form(d, backward):
        return _lib.ATTN_FORMS[lib.pfo_debug_attn_form(ctypes.byref(d), backward)]
    for ring, shapes in ((True, R.RING_SHAPES), (False, R.REG_SHAPES + [R.ODD_SHAPE])):
        for D, Ef, H in shapes:
            assert form(desc(D, Ef, H), 0) == ("fwd_ring" if ring else "fwd_reg"), (D, Ef, H)
            assert form(desc(D, Ef, H), 1) == ("bwd_ring_none" if ring else "bwd_none")
            assert form(desc(D, Ef, H, d_nbr=True), 1) == ("bwd_ring_direct" if ring else "bwd_direct")
            assert form(desc(D, Ef, H, table=True, d_nbr=True), 1) == "bwd_atomic"
            assert form(desc(D, Ef, H, table=True, d_nbr=True, det=1), 1) == "bwd_det"
            runs = not (D > 192 and H == 4)
            assert form(desc(D, Ef, H, table=True, d_nbr=True, members=True), 1) == ("bwd_runs" if runs else "bwd_atomic")
            assert form(desc(D, Ef, H, table=True, d_nbr=True, det=1, members=True), 1) == ("bwd_runs" if runs else "bwd_det")
    assert form(desc(32, 4, 2, qk=P + 4), 0) == "fwd_reg" and form(desc(32, 4, 2, nbr_ld=33), 0) == "fwd_reg"
    assert form(desc(32, 4, 2, qk=P + 4), 1) == "bwd_ring_none" and form(desc(32, 4, 2, nbr_ld=33, d_nbr=True), 1) == "bwd_direct"
    assert form(desc(32, 4, 2, table=True, d_nbr=True, members=True, qk=P + 4), 1) == "bwd_atomic"     # (staging moves 16 bytes)
    assert lib.pfo_debug_attn_form(ctypes.byref(desc(32, 4, 3)), 1) == -1 and b"n_heads" in lib.pfo_last_error()
    assert lib.pfo_debug_attn_form(None, 0) == -1
    assert lib.pfo_debug_attn_det_parts(13) == 4 and lib.pfo_debug_attn_det_parts(0) == -1
    assert lib.pfo_debug_seg_scratch_ints(20) > 0 and lib.pfo_debug_seg_of_ints(33) >= 33 and lib.pfo_debug_seg_scratch_ints(0) == -1


def test_memory_path_queries_answer_from_the_host():
    """The path queries of the memory-side probes are pure host code: the thresholds the device tests assert before they
    launch, and -1 with a message on a size that makes no sense."""
    from pfotgnrec_amd import _lib
    import memory_ref as R
    lib = _lib.load()
    P = 1 << 12
    assert lib.pfo_debug_msg_store_needs_winner(8192) == 0 and lib.pfo_debug_msg_store_needs_winner(8193) == 1
    for B in (1, 300, 8192, 8200):
        assert lib.pfo_debug_msg_store_needs_winner(B) == int(R.msg_store_needs_winner(B))
    assert lib.pfo_debug_msg_store_needs_winner(0) == -1 and b"bad size" in lib.pfo_last_error()
    assert [lib.pfo_debug_scan_sweeps(n) for n in R.ISCAN_SIZES] == [1, 1, 1, 1, 1, 2, 2]
    assert lib.pfo_debug_scan_sweeps(0) == -1 and lib.pfo_debug_scan_sweeps(1 << 31) == -1
    assert [lib.pfo_debug_fold_parts_rows_in_flight(n) for n in R.FOLD_PARTS] == [1, 1, 1, 1, 8, 8, 8, 8]
    assert lib.pfo_debug_fold_parts_rows_in_flight(R.FOLD_DEEP_FROM - 1) == 1 and lib.pfo_debug_fold_parts_rows_in_flight(R.FOLD_DEEP_FROM) == 8
    assert lib.pfo_debug_fold_parts_rows_in_flight(0) == -1
    assert lib.pfo_debug_fold_parts_scratch_doubles(65) == 32 * 65 and lib.pfo_debug_fold_parts_scratch_doubles(0) == -1
    assert lib.pfo_debug_compact_scratch_ints((1 << 20) + 3) == 2 * 1025 + 8 and lib.pfo_debug_compact_scratch_ints(0) == -1
    vec = lambda D=8, stride=64, off=0, extra=P: lib.pfo_debug_gru_gates_bwd_vec(P + off, P, P, P, D, P, stride, extra)
    assert vec() == 1 and vec(extra=None) == 1 and vec(off=4) == 0 and vec(stride=66) == 0 and vec(D=6) == 0 and vec(extra=P + 4) == 0


def _memory_refusals():
    """(id, probe, arguments, a word of the message): every argument refusal of the memory-side probes.  P stands for a
    device pointer that is never followed: each call is refused on the host, before anything is launched."""
    import ctypes as C
    P, S = 1 << 12, None
    four = lambda v: (C.c_void_p * 4)(v, v, v, v)
    hole = (C.c_void_p * 4)(P, None, P, P)
    compact = lambda **k: [k.get("nodes0", P), 5, k.get("extra", P), k.get("n_extra", 3), k.get("n_nodes", 100), P, P, P, P, P, k.get("scratch", 10),
                           k.get("zero", 1), k.get("marked", 0), S]
    pack = lambda **k: [k.get("tab", P), k.get("M", 28), k.get("mem", P), 8, P, P, P, k.get("cap", 5), k.get("rows", P), P, P, P, 7, P, P, S]
    gates = lambda **k: [P, P, P, P, k.get("hm", P), P, 5, 8, P, k.get("n_rep", 1), 64, P, 0, S]
    persist = lambda **k: [P, P, k.get("B", 3), P, P, P, P, k.get("mem", P), P, 8, None, S]
    store = lambda **k: [P, P, P, P, k.get("B", 3), P, P, k.get("ef", P), P, P, 8, 4, k.get("tab", P), P, P, None, S]
    cq = lambda **k: [k.get("gq", four(P)), four(P), k.get("L", 2), k.get("tb", P), k.get("D", 8), four(P), four(P), k.get("d_tb", P), k.get("part", None), None, k.get("dtime", None),
                      k.get("n_bins", 0), k.get("d_tw", None), S]
    fold = lambda **k: [P, 5, k.get("n", 65), k.get("out", P), 0, P, k.get("scratch", 32 * 65), k.get("tickets", P), None, S]
    return [
        ("compact-short-scratch", "pfo_debug_touch_compact", compact(scratch=9), "short scratch"),
        ("compact-no-nodes", "pfo_debug_touch_compact", compact(n_nodes=0), "bad arguments"),
        ("compact-null-extra", "pfo_debug_touch_compact", compact(extra=None), "bad arguments"),
        ("compact-no-list", "pfo_debug_touch_compact", compact(nodes0=None), "no node list"),
        ("compact-marked-uncleared", "pfo_debug_touch_compact", compact(marked=1, zero=0), "cleared table"),
        ("pack-row-length", "pfo_debug_pack_remap", pack(M=30), "multiples of 4"),
        ("pack-null-memory", "pfo_debug_pack_remap", pack(mem=None), "bad arguments"),
        ("pack-null-message-rows", "pfo_debug_pack_remap", pack(rows=None), "null message buffers"),
        ("pack-no-rows", "pfo_debug_pack_remap", pack(cap=0), "bad sizes"),
        ("gates-null", "pfo_debug_gru_gates_bwd", gates(hm=None), "null argument"),
        ("gates-no-replica", "pfo_debug_gru_gates_bwd", gates(n_rep=0), "bad sizes"),
        ("zero-rows-null", "pfo_debug_zero_rows", [None, P, 5, 8, 1, 64, S], "null argument"),
        ("zero-rows-row-length", "pfo_debug_zero_rows", [P, P, 5, 6, 1, 64, S], "multiple of 4"),
        ("zero-rows-stride", "pfo_debug_zero_rows", [P, P, 5, 8, 2, 66, S], "multiple of 4"),
        ("zero-rows-no-replica", "pfo_debug_zero_rows", [P, P, 5, 8, 0, 64, S], "bad sizes"),
        ("persist-null", "pfo_debug_persist", persist(mem=None), "null argument"),
        ("persist-empty", "pfo_debug_persist", persist(B=0), "bad sizes"),
        ("store-null", "pfo_debug_msg_store", store(tab=None), "null argument"),
        ("store-no-edge-rows", "pfo_debug_msg_store", store(ef=None), "bad sizes"),
        ("store-no-winner-table", "pfo_debug_msg_store", store(B=8193), "winner table"),
        ("select-null", "pfo_debug_observe_select", [P, P, 3, None, P, 0, P, P, P, S], "null argument"),
        ("select-empty", "pfo_debug_observe_select", [P, P, 0, P, P, 0, P, P, P, S], "bad batch size"),
        ("select-stamp-overflow", "pfo_debug_observe_select", [P, P, 3, P, P, 2 ** 31 - 4, P, P, P, S], "stamp base"),
        ("iscan-short-scratch", "pfo_debug_iscan", [P, 5000, P, P, 19, S], "short scratch"),
        ("iscan-no-scratch", "pfo_debug_iscan", [P, 5, P, None, 16, S], "short scratch"),
        ("iscan-empty", "pfo_debug_iscan", [P, 0, P, P, 16, S], "bad size"),
        ("iscan-null", "pfo_debug_iscan", [None, 5, P, P, 16, S], "bad arguments"),
        ("mean-empty", "pfo_debug_mean", [P, 0, P, S], "bad arguments"),
        ("cq-null", "pfo_debug_cq_backward", cq(tb=None), "null argument"),
        ("cq-no-columns", "pfo_debug_cq_backward", cq(D=0), "bad size"),
        ("cq-layer-count", "pfo_debug_cq_backward", cq(L=5), "bad layer count"),
        ("cq-null-layer", "pfo_debug_cq_backward", cq(gq=hole), "null layer pointer"),
        ("cq-nowhere", "pfo_debug_cq_backward", cq(d_tb=None), "no place"),
        ("cq-bins-with-partial", "pfo_debug_cq_backward", cq(dtime=P, n_bins=3, d_tw=P, part=P), "final launch"),
        ("cq-bins-without-d_tw", "pfo_debug_cq_backward", cq(dtime=P, n_bins=3), "final launch"),
        ("cq-no-bins", "pfo_debug_cq_backward", cq(dtime=P, n_bins=0, d_tw=P), "bad bin count"),
        ("fold-too-wide", "pfo_debug_fold_parts", fold(n=4097, scratch=32 * 4097), "too many columns"),
        ("fold-short-scratch", "pfo_debug_fold_parts", fold(scratch=32 * 65 - 1), "short scratch"),
        ("fold-null-tickets", "pfo_debug_fold_parts", fold(tickets=None), "null argument"),
        ("fold-no-output", "pfo_debug_fold_parts", fold(out=None), "null argument"),
        # ... and of the graph side's plan query (host only: its array is a HOST array, there is no stream argument)
        ("csr-plan-negative-edges", "pfo_debug_csr_build_plan", [-1, 5, (C.c_int32 * 3)()], "bad sizes"),
        ("csr-plan-no-nodes", "pfo_debug_csr_build_plan", [5, 0, (C.c_int32 * 3)()], "bad sizes"),
        ("csr-plan-too-many-entries", "pfo_debug_csr_build_plan", [1 << 30, 5, (C.c_int32 * 3)()], "must fit in int32"),
        ("csr-plan-null-output", "pfo_debug_csr_build_plan", [5, 5, None], "null output"),
    ]


@pytest.mark.parametrize("cid,probe,args,word", _memory_refusals(), ids=[c[0] for c in _memory_refusals()])
def test_memory_probe_refuses_bad_arguments(cid, probe, args, word):
    from pfotgnrec_amd import _lib
    lib = _lib.load()
    assert getattr(lib, probe)(*args) == -1                                # PFO_ERR_INVALID: refused before any launch
    assert word.encode() in lib.pfo_last_error(), lib.pfo_last_error()
    with pytest.raises(_lib.PfoError, match=word):
        _lib.call(probe, *args)


def test_param_layout_matches_reference_inventory():
    """1.551 M trainable fp32 at C2 (D=172, Ef=4, L=2), 34 304 at C1 incl. the dead layer_norm."""
    import ctypes
    from pfotgnrec_amd import _lib
    cfg = _lib.TgnConfig(50501, 1000001, 172, 4, 2, 2, 1, 2560, 20, 512)
    lay = _lib.TgnLayout()
    _lib.call("pfo_tgn_param_layout", ctypes.byref(cfg), ctypes.byref(lay))
    per_layer = 344 * 344 + 2 * 344 * 348 + 1032 + 344 * 344 + 344 + 172 * 516 + 172 + 172 * 172 + 172
    assert per_layer == 596152
    assert lay.total == 344 + 358104 + 2 * per_layer
    assert lay.time_b == lay.time_w + 172
    assert _lib.load().pfo_tgn_workspace_bytes(ctypes.byref(cfg)) > 0


def test_invalid_config_is_rejected_with_message():
    import ctypes
    from pfotgnrec_amd import _lib
    cfg = _lib.TgnConfig(100, 10, 30, 4, 1, 2, 1, 8, 4, 4)       # D not a multiple of 4
    lay = _lib.TgnLayout()
    with pytest.raises(_lib.PfoError, match="multiple of 4"):
        _lib.call("pfo_tgn_param_layout", ctypes.byref(cfg), ctypes.byref(lay))


def test_compute_without_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import pfotgnrec_amd as P
    from pfotgnrec_amd import _lib
    from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
    g = make_graph(SyntheticConfig("t", 50, 10, 400, 8, 1, 4, 2), with_prices=False)
    nf = P.get_neighbor_finder(g.data, False)
    with pytest.raises(_lib.PfoError):
        nf.get_temporal_neighbor(g.data.sources[:3], g.data.timestamps[:3], 4)
    tgn = P.TGN(nf, g.node_features, g.edge_features, "cpu", n_layers=1, n_heads=2, use_memory=True, memory_dimension=8,
                message_function="identity")
    with pytest.raises(_lib.PfoError):
        tgn.compute_temporal_embeddings(g.data.sources[:2], g.data.destinations[:2], g.data.destinations[:6],
                                        g.data.timestamps[:2], g.data.edge_idxs[:2], 4)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(REPO, "pfotgnrec_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp")):
                src = open(os.path.join(root, f)).read()
                assert "import oracle" not in src and "from oracle" not in src, f
