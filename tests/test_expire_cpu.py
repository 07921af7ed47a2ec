"""CPU side of ``TGN.expire``: the numpy reference against a rebuild over the filtered log, the release rule on a
table one can check by eye, the new symbols, and the argument checks that run in front of every launch - none needs a kernel."""
import numpy as np
import pytest

import expire_ref as R


def _random_log(seed, n_nodes=40, n_edges=600, n_times=37):
    """A chronological log with many ties: ``n_times`` distinct timestamps over ``n_edges`` edges, node 0 unused."""
    rs = np.random.RandomState(seed)
    src = rs.randint(1, n_nodes // 2, size=n_edges)
    dst = rs.randint(n_nodes // 2, n_nodes - 3, size=n_edges)          # the last three nodes have empty rows
    ts = np.sort(rs.randint(0, n_times, size=n_edges)).astype(np.float64) * 0.5 + 100.0
    return src, dst, np.arange(1, n_edges + 1), ts


@pytest.mark.parametrize("seed", [0, 1])
def test_reference_equals_a_rebuild_over_the_filtered_log(seed):
    from pfotgnrec_amd.neighbor_finder import build_csr
    src, dst, eid, ts = _random_log(seed)
    n_nodes = 40
    full = build_csr(src, dst, eid, ts, max_node_idx=n_nodes - 1)
    tie = float(np.unique(ts)[len(np.unique(ts)) // 2])
    assert (ts == tie).sum() > 1, "the cutoff sits on a tie group"
    for cutoff in (ts.min() - 1.0, ts.min(), tie, np.nextafter(tie, np.inf), 0.5 * (ts.min() + ts.max()) + 0.125, ts.max(),
                   ts.max() + 1.0):
        m = ts >= cutoff
        want = build_csr(src[m], dst[m], eid[m], ts[m], max_node_idx=n_nodes - 1)
        got, keep = R.expire_csr(*full, cutoff)
        for a, b, name in zip(got, want, ("indptr", "nbr", "eidx", "ts")):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (name, cutoff)
        assert int(keep.sum()) == 2 * int(m.sum())
    got, keep = R.expire_csr(*full, tie)
    assert (got[3] == tie).sum() == (full[3] == tie).sum() > 0, "strict <: the tie group at the cutoff stays whole"


def test_release_rule_by_hand():
    # rows 0..7; finder A names 1 (expired), 2 (expired), 3 (alive), 5 (expired and alive); finder B names 2 (alive), 6 (expired);
    # rows 4 and 7 are named by nobody
    a = (np.array([1, 2, 3, 5, 5], np.int32), np.array([1.0, 2.0, 9.0, 3.0, 9.0]))
    b = (np.array([2, 6], np.int32), np.array([8.0, 4.0]))
    remap, n_keep = R.release_rule(8, [a, b], 5.0)
    assert remap.tolist() == [0, -1, 1, 2, 3, 4, -1, 5] and n_keep == 6
    remap_a, n_a = R.release_rule(8, [a], 5.0)                          # alone, A releases row 2 as well
    assert remap_a.tolist() == [0, -1, -1, 1, 2, 3, 4, 5] and n_a == 6
    assert R.release_rule(8, [a, b], 0.0)[0].tolist() == list(range(8)), "nothing expired: the identity"
    table = np.arange(16, dtype=np.float32).reshape(8, 2)
    out = R.compact_table(table, remap, capacity=9)
    assert out.shape == (9, 2) and np.array_equal(out[:6], table[[0, 2, 3, 4, 5, 7]]) and not out[6:].any()


def test_library_and_classes_export_the_retention_surface():
    import pfotgnrec_amd as P
    from pfotgnrec_amd import _lib
    lib = _lib.load()
    for name in ("pfo_csr_expire_scratch_bytes", "pfo_csr_expire_plan", "pfo_csr_expire_copy", "pfo_edge_rows_mark",
                 "pfo_edge_rows_plan_scratch_bytes", "pfo_edge_rows_plan", "pfo_edge_rows_compact", "pfo_eidx_remap"):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES, name
    assert lib.pfo_abi_version() == 6
    assert hasattr(P.TGN, "expire") and hasattr(P.NeighborFinder, "expire") and hasattr(P.NeighborFinder, "remap_edge_idxs")


def test_entry_points_reject_bad_arguments_without_a_device():
    """The argument checks run in front of the launches: no device is needed to see them refuse."""
    from pfotgnrec_amd import _lib
    lib = _lib.load()
    assert lib.pfo_csr_expire_scratch_bytes(0) == -1 and lib.pfo_csr_expire_scratch_bytes(1) == 8
    assert lib.pfo_csr_expire_scratch_bytes(1025) == 16
    assert lib.pfo_edge_rows_plan_scratch_bytes(0) == -1 and lib.pfo_edge_rows_plan_scratch_bytes(1024) == 1025 * 8
    for bad in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(_lib.PfoError, match="finite"):
            _lib.call("pfo_csr_expire_plan", 8, 8, 4, bad, 8, 8, 8, 64, None)
        with pytest.raises(_lib.PfoError, match="finite"):
            _lib.call("pfo_edge_rows_mark", 8, 8, 4, bad, 4, 8, None)
    with pytest.raises(_lib.PfoError, match="node count"):
        _lib.call("pfo_csr_expire_plan", 8, 8, 0, 1.0, 8, 8, 8, 64, None)
    with pytest.raises(_lib.PfoError, match="null pointer"):
        _lib.call("pfo_csr_expire_plan", None, 8, 4, 1.0, 8, 8, 8, 64, None)
    with pytest.raises(_lib.PfoError, match="short scratch"):
        _lib.call("pfo_csr_expire_plan", 8, 8, 1025, 1.0, 8, 8, 8, 8, None)
    with pytest.raises(_lib.PfoError, match="null pointer"):
        _lib.call("pfo_csr_expire_copy", None, None, None, None, 4, None, None, 3, None, None, None, None)
    _lib.call("pfo_csr_expire_copy", None, None, None, None, 4, None, None, 0, None, None, None, None)     # total == 0: nothing queued
    with pytest.raises(_lib.PfoError, match="short scratch"):
        _lib.call("pfo_edge_rows_plan", 8, 1024, 8, 8, 8, 1024 * 8, None)
    with pytest.raises(_lib.PfoError, match="n_keep"):
        _lib.call("pfo_edge_rows_compact", 8, 10, 11, 4, 8, 8, None)
    with pytest.raises(_lib.PfoError, match="n_keep"):
        _lib.call("pfo_edge_rows_compact", 8, 10, 0, 4, 8, 8, None)
    _lib.call("pfo_edge_rows_compact", None, 10, 10, 4, None, None, None)                                   # nothing released
    _lib.call("pfo_edge_rows_mark", None, None, 0, 1.0, 4, None, None)
    _lib.call("pfo_eidx_remap", None, 0, None, 4, None)
    with pytest.raises(_lib.PfoError, match="null pointer"):
        _lib.call("pfo_eidx_remap", None, 3, None, 4, None)


def _host_model():
    import pfotgnrec_amd as P
    from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
    g = make_graph(SyntheticConfig("t", 50, 10, 400, 8, 1, 4, 2), with_prices=False)
    nf = P.get_neighbor_finder(g.data, False)
    tgn = P.TGN(nf, g.node_features, g.edge_features, "cpu", n_layers=1, n_heads=2, use_memory=True, memory_dimension=8,
                message_function="identity")
    return tgn, nf


def _snapshot(tgn, nf):
    return (nf._version, nf.n_nodes, nf._max_nbr, nf._max_eidx, tuple(a.tobytes() for a in nf._host), tuple(nf._dev),
            tgn._cfg.n_edges_p1, tgn._tables_version, tgn.edge_raw_features.data_ptr(), tgn.edge_raw_features.numpy().tobytes(),
            tgn._step)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_cutoffs_are_rejected_before_any_device_call(bad, monkeypatch):
    from pfotgnrec_amd import _lib
    tgn, nf = _host_model()
    before = _snapshot(tgn, nf)

    def no_device_call(*a, **k):
        raise AssertionError("the cutoff must be refused before the library or the device is asked for anything")
    for name in ("require_gpu", "call", "byte_count"):
        monkeypatch.setattr(_lib, name, no_device_call)
    with pytest.raises(ValueError, match="finite"):
        nf.expire(bad)
    with pytest.raises(ValueError, match="finite"):
        tgn.expire(bad)
    with pytest.raises(ValueError, match="finite"):
        tgn.expire(bad, compact_edges=False, finders=[nf])
    assert _snapshot(tgn, nf) == before


def test_a_model_on_the_host_refuses_like_every_compute_method():
    from pfotgnrec_amd import _lib
    tgn, nf = _host_model()                                     # (its tensors live on the host: refused with or without a device)
    before = _snapshot(tgn, nf)
    with pytest.raises(_lib.PfoError):
        tgn.expire(float(nf.ts.max()))
    assert _snapshot(tgn, nf) == before
