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
