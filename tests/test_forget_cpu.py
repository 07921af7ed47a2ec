"""CPU side of ``TGN.forget``: the numpy reference against a rebuild over the log without the interactions that
touch a forgotten node, the flag rule against "a row is released iff its interaction touched a forgotten node", the new symbols,
and the argument checks that run in front of every launch - none needs a kernel."""
import numpy as np
import pytest

import forget_ref as R


def _random_log(seed, n_nodes=40, n_edges=600, n_times=37):
    """A chronological log with many ties: ``n_times`` distinct timestamps over ``n_edges`` edges; node 0 unused, the last three
    nodes have empty rows, user 1 -> item 20 is traded again and again (equal entries next to each other inside a row)."""
    rs = np.random.RandomState(seed)
    src = rs.randint(1, n_nodes // 2, size=n_edges)
    dst = rs.randint(n_nodes // 2, n_nodes - 3, size=n_edges)
    src[::9], dst[::9] = 1, 20
    ts = np.sort(rs.randint(0, n_times, size=n_edges)).astype(np.float64) * 0.5 + 100.0
    return src, dst, np.arange(1, n_edges + 1), ts


def _same(got, want, tag):
    for a, b, name in zip(got, want, ("indptr", "nbr", "eidx", "ts")):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (name, tag)


@pytest.mark.parametrize("seed", [0, 1])
def test_reference_equals_a_rebuild_over_the_filtered_log(seed):
    from pfotgnrec_amd.neighbor_finder import build_csr
    src, dst, eid, ts = _random_log(seed)
    n_nodes = 40
    full = build_csr(src, dst, eid, ts, max_node_idx=n_nodes - 1)
    assert (np.diff(ts) == 0).sum() > 400, "ties: the order inside a row is pinned by the edge order"
    for ids in ([], [1], [20], [1, 20], [5, 25, 25, 5], list(range(1, 20)), list(range(1, n_nodes)), [38], [0, 40, 99, -3, 7]):
        gone = R.gone_of(n_nodes, ids)
        m = ~(gone[src].astype(bool) | gone[dst].astype(bool))
        want = build_csr(src[m], dst[m], eid[m], ts[m], max_node_idx=n_nodes - 1)
        got, keep = R.forget_csr(*full, gone)
        _same(got, want, ids)
        assert int(keep.sum()) == 2 * int(m.sum())
        for v in np.flatnonzero(gone):
            assert got[0][v] == got[0][v + 1] and not (got[1] == v).any(), "a forgotten node has no row and nobody names it"
    assert R.gone_of(n_nodes, [0, 40, 99, -3, 7]).tolist() == R.gone_of(n_nodes, [7]).tolist() and R.gone_of(n_nodes, [7]).sum() == 1
    # a neighbour id outside the table counts as not gone
    ptr, nbr = np.array([0, 0, 3], np.int64), np.array([1, 7, -2], np.int32)
    assert R.dropped_mask(ptr, nbr, np.array([0, 0], np.uint8)).tolist() == [False, False, False]
    assert R.dropped_mask(ptr, nbr, np.array([1, 0], np.uint8)).tolist() == [False, False, False]
    assert R.dropped_mask(np.array([0, 1, 3], np.int64), nbr, np.array([1, 0], np.uint8)).tolist() == [True, False, False]


@pytest.mark.parametrize("two_finders", [False, True], ids=["one finder", "train and full"])
def test_flag_rule_releases_exactly_the_rows_of_touched_interactions(two_finders):
    from pfotgnrec_amd.neighbor_finder import build_csr
    src, dst, eid, ts = _random_log(3)
    n_nodes, n_rows = 40, len(eid) + 6                                   # (rows behind the log's: named by nobody)
    sel = np.arange(len(eid)) % 7 != 3                                    # the full finder leaves every seventh row unnamed
    train = sel & (np.arange(len(eid)) % 3 != 1)
    finders = [build_csr(src[sel], dst[sel], eid[sel], ts[sel], max_node_idx=n_nodes - 1)]
    if two_finders:
        finders.append(build_csr(src[train], dst[train], eid[train], ts[train], max_node_idx=n_nodes - 1))
    for ids in ([], [1], [20], [2, 27, 33], list(range(1, n_nodes))):
        gone = R.gone_of(n_nodes, ids)
        touched = gone[src].astype(bool) | gone[dst].astype(bool)
        want_released = np.zeros(n_rows, bool)
        want_released[eid[sel & touched]] = True                         # named by somebody and touching a forgotten node
        flags = R.row_flags(n_rows, [c[:3] for c in finders], gone)
        assert not (flags == 3).any(), "both entries of an interaction go or stay together, in every finder"
        remap, n_keep = R.release_rule(n_rows, [c[:3] for c in finders], gone)
        assert np.array_equal(remap < 0, want_released) and remap[0] == 0 and n_keep == n_rows - int(want_released.sum())
        assert np.array_equal(remap[remap >= 0], np.arange(n_keep)), "kept rows are renumbered densely, in order"
        swept, remap2, n_keep2, dropped = R.forget_all(n_rows, finders, gone)
        assert np.array_equal(remap, remap2) and n_keep2 == n_keep
        assert dropped == 2 * int((sel & touched).sum()) + (2 * int((train & touched).sum()) if two_finders else 0)
        for c, mask in zip(swept, (sel, train)):
            m = mask & ~touched
            _same(c, build_csr(src[m], dst[m], remap[eid[m]], ts[m], max_node_idx=n_nodes - 1), ids)
    # by hand: rows 0..5; entries of row 1 name nodes 2 (rows 1, 2) and 3 (row 3); node 2 goes
    ptr = np.array([0, 0, 3, 5, 6], np.int64)
    nbr = np.array([2, 2, 3, 1, 1, 1], np.int32)
    eidx = np.array([1, 2, 3, 1, 2, 3], np.int32)
    assert R.row_flags(6, [(ptr, nbr, eidx)], R.gone_of(4, [2])).tolist() == [0, 1, 1, 2, 0, 0]
    assert R.release_rule(6, [(ptr, nbr, eidx)], R.gone_of(4, [2]))[0].tolist() == [0, -1, -1, 1, 2, 3]


def test_reset_rows_puts_only_flagged_rows_back():
    mem = np.arange(12, dtype=np.float32).reshape(4, 3)
    idx = np.arange(8, dtype=np.int32).reshape(4, 2)
    t = np.array([1.0, 2.0, 3.0, 4.0])
    out = R.reset_rows([mem, idx, t], [0, -1, -np.inf], np.array([0, 1, 0, 1], np.uint8))
    assert out[0].tolist() == [[0, 1, 2], [0, 0, 0], [6, 7, 8], [0, 0, 0]] and out[1].tolist() == [[0, 1], [-1, -1], [4, 5], [-1, -1]]
    assert out[2].tolist() == [1.0, -np.inf, 3.0, -np.inf] and mem[1, 0] == 3.0, "the inputs are left alone"


def test_library_and_classes_export_the_forget_surface():
    import pfotgnrec_amd as P
    from pfotgnrec_amd import _lib
    lib = _lib.load()
    for name in ("pfo_nodes_flag", "pfo_csr_forget_scratch_bytes", "pfo_csr_forget_plan", "pfo_csr_forget_copy",
                 "pfo_edge_rows_mark_nodes", "pfo_node_rows_reset"):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES, name
    assert lib.pfo_abi_version() == 6
    assert hasattr(P.TGN, "forget") and hasattr(P.NeighborFinder, "forget")


def test_entry_points_reject_bad_arguments_without_a_device():
    """Every check is made on the host, in front of the launches: no device is needed to see them refuse (PFO_ERR_INVALID)."""
    from pfotgnrec_amd import _lib
    lib = _lib.load()
    P, S = 1 << 12, None                                                  # a device pointer that is never followed; the stream
    assert lib.pfo_csr_forget_scratch_bytes(0, 5) == -1 and lib.pfo_csr_forget_scratch_bytes(5, -1) == -1
    assert lib.pfo_csr_forget_scratch_bytes(5, 1 << 31) == -1 and lib.pfo_csr_forget_scratch_bytes(1 << 31, 5) == -1
    assert lib.pfo_csr_forget_scratch_bytes(5, 0) == 8 and lib.pfo_csr_forget_scratch_bytes(5, 1024) == 8
    assert lib.pfo_csr_forget_scratch_bytes(5, 1025) == 16
    plan = lambda **k: [k.get("indptr", P), k.get("nbr", P), k.get("n", 4), k.get("total", 1025), k.get("gone", P), k.get("keep", P),
                        k.get("pos", P), k.get("new", P), k.get("scratch", P), k.get("nbytes", 16), S]
    copy = lambda **k: [k.get("nbr", P), P, P, k.get("old", 10), k.get("keep", P), P, k.get("total", 4), P, P, k.get("out", P), S]
    mark = lambda **k: [k.get("indptr", P), P, P, k.get("n", 10), k.get("nodes", 4), k.get("gone", P), k.get("rows", 7), k.get("flags", P), S]
    reset = lambda **k: [k.get("gone", P), k.get("n", 4), P, k.get("D", 6), P, P, k.get("M", 19), P, P, P, k.get("Dn", 5), P, k.get("W", 3), P, P, S]
    refused = [
        ("pfo_nodes_flag", [P, -1, 4, P, S], "bad sizes"), ("pfo_nodes_flag", [P, 3, 0, P, S], "bad sizes"),
        ("pfo_nodes_flag", [P, 3, 4, None, S], "null pointer"), ("pfo_nodes_flag", [None, 3, 4, P, S], "null pointer"),
        ("pfo_csr_forget_plan", plan(n=0), "bad sizes"), ("pfo_csr_forget_plan", plan(total=-1), "bad sizes"),
        ("pfo_csr_forget_plan", plan(total=1 << 31), "bad sizes"), ("pfo_csr_forget_plan", plan(nbytes=8), "short scratch"),
        ("pfo_csr_forget_plan", plan(scratch=None), "null pointer"), ("pfo_csr_forget_plan", plan(indptr=None), "null pointer"),
        ("pfo_csr_forget_plan", plan(nbr=None), "null pointer"), ("pfo_csr_forget_plan", plan(keep=None), "null pointer"),
        ("pfo_csr_forget_plan", plan(gone=None), "null pointer"), ("pfo_csr_forget_plan", plan(pos=None), "null pointer"),
        ("pfo_csr_forget_plan", plan(new=None, total=0), "null pointer"),
        ("pfo_csr_forget_copy", copy(old=-1), "bad sizes"), ("pfo_csr_forget_copy", copy(total=11), "bad sizes"),
        ("pfo_csr_forget_copy", copy(total=-1), "bad sizes"), ("pfo_csr_forget_copy", copy(nbr=None), "null pointer"),
        ("pfo_csr_forget_copy", copy(keep=None), "null pointer"), ("pfo_csr_forget_copy", copy(out=None), "null pointer"),
        ("pfo_edge_rows_mark_nodes", mark(rows=0), "bad sizes"), ("pfo_edge_rows_mark_nodes", mark(nodes=0), "bad sizes"),
        ("pfo_edge_rows_mark_nodes", mark(n=-1), "bad sizes"), ("pfo_edge_rows_mark_nodes", mark(indptr=None), "null pointer"),
        ("pfo_edge_rows_mark_nodes", mark(gone=None), "null pointer"), ("pfo_edge_rows_mark_nodes", mark(flags=None), "null pointer"),
        ("pfo_node_rows_reset", reset(n=0), "bad sizes"), ("pfo_node_rows_reset", reset(gone=None), "null pointer"),
        ("pfo_node_rows_reset", reset(D=0), "without columns"), ("pfo_node_rows_reset", reset(M=0), "without columns"),
        ("pfo_node_rows_reset", reset(Dn=-1), "without columns"), ("pfo_node_rows_reset", reset(W=0), "without columns"),
    ]
    for name, args, word in refused:
        assert getattr(lib, name)(*args) == -1, (name, args)              # PFO_ERR_INVALID
        assert word.encode() in lib.pfo_last_error(), (name, args, lib.pfo_last_error())
        with pytest.raises(_lib.PfoError, match=word):
            _lib.call(name, *args)
    _lib.call("pfo_csr_forget_copy", None, None, None, 10, None, None, 0, None, None, None, None)     # total == 0: nothing queued
    _lib.call("pfo_edge_rows_mark_nodes", None, None, None, 0, 4, None, 7, None, None)                # no entries: nothing queued


def _host_model():
    import pfotgnrec_amd as P
    from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
    g = make_graph(SyntheticConfig("t", 50, 10, 400, 8, 1, 4, 2), with_prices=False)
    nf = P.get_neighbor_finder(g.data, False)
    tgn = P.TGN(nf, g.node_features, g.edge_features, "cpu", n_layers=1, n_heads=2, use_memory=True, memory_dimension=8,
                message_function="identity")
    return tgn, nf


def _snapshot(tgn, nf):
    m = tgn.memory
    return (nf._version, nf.n_nodes, nf._max_nbr, nf._max_eidx, tuple(a.tobytes() for a in nf._host), tuple(nf._dev),
            tgn._cfg.n_edges_p1, tgn._tables_version, tgn.edge_raw_features.data_ptr(), tgn.edge_raw_features.numpy().tobytes(),
            tgn.node_raw_features.numpy().tobytes(), m.memory.numpy().tobytes(), m.has_msg.numpy().tobytes(), m._state_version,
            m._any_msg, tgn._step)


def test_bad_ids_are_rejected_before_any_device_call(monkeypatch):
    import torch
    from pfotgnrec_amd import _lib
    tgn, nf = _host_model()
    n = tgn.n_nodes
    before = _snapshot(tgn, nf)

    def no_device_call(*a, **k):
        raise AssertionError("the ids must be refused before the library or the device is asked for anything")
    for name in ("require_gpu", "call", "byte_count"):
        monkeypatch.setattr(_lib, name, no_device_call)
    for bad, word in (([1.0, 2.0], "integers"), (np.array([1.5]), "integers"), ([True, False], "integers"), (["7"], "integers"),
                      ([0], "padding node"), ([3, 0, 5], "padding node"), ([-1], "must lie in"), ([n], "must lie in"),
                      ([3, n + 40], "must lie in"), (np.array([[1, 2]]), "flat list"),
                      (torch.tensor([1.0, 2.0]), "integer tensor"), (torch.zeros((2, 2), dtype=torch.int32), "integer tensor")):
        for kw in ({}, {"compact_edges": False}, {"finders": [nf]}):
            with pytest.raises(ValueError, match=word):
                tgn.forget(bad, **kw)
    with pytest.raises(ValueError, match="integers"):
        nf.forget([1.5])
    with pytest.raises(ValueError, match="int32"):
        nf.forget([2 ** 31])
    with pytest.raises(ValueError, match="flags"):
        nf.forget(torch.zeros(nf.n_nodes + 1, dtype=torch.uint8))
    # nothing to forget: nothing is asked of the device either
    for empty in ([], (), np.zeros(0, np.int64), np.zeros(0), torch.zeros(0, dtype=torch.int64)):
        assert tgn.forget(empty) == (0, None) and tgn.forget(empty, compact_edges=False, finders=[nf]) == (0, None)
    assert _snapshot(tgn, nf) == before


def test_a_model_on_the_host_refuses_like_every_compute_method():
    from pfotgnrec_amd import _lib
    tgn, nf = _host_model()                                     # (its tensors live on the host: refused with or without a device)
    before = _snapshot(tgn, nf)
    with pytest.raises(_lib.PfoError):
        tgn.forget([3, 55])
    with pytest.raises(_lib.PfoError):
        tgn.forget([3], compact_edges=False)
    assert _snapshot(tgn, nf) == before


def test_the_docstring_states_the_limit():
    import pfotgnrec_amd as P
    doc = " ".join(P.TGN.forget.__doc__.split())
    for phrase in ("derived values, not ids", "holdings rows that name a forgotten stock stay", "item_ok", "update_holdings",
                   "EVERY rank calls it with the same ids", "BETWEEN steps"):
        assert phrase in doc, phrase
