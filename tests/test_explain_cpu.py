"""Host side of the explanation query: the numpy rule of ``explain_ref`` on hand-made tables, the same rule fed the
oracle's attention weights (rows are distributions), the refusals of ``TGN.explain`` before a GPU is asked for, and the C
entry's bounds, which are checked on the host."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pfotgnrec_amd as P
from pfotgnrec_amd import _lib, build
from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
from oracle import tgn_oracle as T
from oracle.neighbor_finder import OracleNeighborFinder, build_adjacency
from conftest import REPO
import explain_ref as E

f32 = np.float32


def _raw1(nbr, w, dt, eidx):
    return dict(nbr=np.array([nbr], np.int32), w=np.array([w], f32), dt=np.array([dt], f32), eidx=np.array([eidx], np.int32))


def test_host_model_on_hand_made_tables():
    # ---- hops 1, H = 2, K = 6: node 7 in slots 0, 2, 5 (merged: count 3, the smallest age 2.0 is slot 2's, edge 22); slot 3 is
    # padding - its weight, were it not 0, must not count; nodes 9 and 4 tie on the weight and on the age: the smaller id first
    w = [[0.25, 0.125, 0.125, 0.5, 0.125, 0.25], [0.25, 0.375, 0.125, 0.5, 0.375, 0.0]]
    raw = _raw1([7, 9, 7, 0, 4, 7], w, [5.0, 3.0, 2.0, 1.0, 3.0, 2.0], [20, 21, 22, 23, 24, 25])
    node, weight, n_valid, count, age, eidx = E.explain(raw, 4)
    assert node.tolist() == [[7, 4, 9, -1]] and n_valid.tolist() == [3] and count.tolist() == [[3, 1, 1, 0]]
    assert weight.tolist() == [[0.5, 0.25, 0.25, 0.0]] and eidx.tolist() == [[22, 24, 21, -1]]
    assert age[0, :3].tolist() == [2.0, 3.0, 3.0] and np.isnan(age[0, 3]) and age.dtype == f32 and weight.dtype == np.float64
    # the equal-age rule: slots 2 and 5 both have age 2.0 - the lower slot's edge wins whichever comes first in memory
    raw["eidx"][0, 2], raw["eidx"][0, 5] = 25, 22
    assert E.explain(raw, 4)[5].tolist() == [[25, 24, 21, -1]]
    # ties on the weight order by age before id: make node 9 the younger
    raw["dt"][0, 1] = 2.5
    assert E.explain(raw, 4)[0].tolist() == [[7, 9, 4, -1]]
    # m cuts the list, n_valid = min(m, distinct)
    node, weight, n_valid, *_ = E.explain(raw, 2)
    assert node.tolist() == [[7, 9]] and n_valid.tolist() == [2] and weight.tolist() == [[0.5, 0.25]]
    # an all-padding row is empty, whatever its weights say
    node, weight, n_valid, count, age, eidx = E.explain(_raw1([0] * 6, w, [0.0] * 6, [0] * 6), 3)
    assert node.tolist() == [[-1] * 3] and weight.tolist() == [[0.0] * 3] and n_valid.tolist() == [0]
    assert count.tolist() == [[0] * 3] and np.isnan(age).all() and eidx.tolist() == [[-1] * 3]
    # the head mean is the sequential sum over the heads, divided by H - not a product with 1 / H
    third = _raw1([5], [[0.1], [0.2], [0.3]], [1.0], [1])
    assert E.explain(third, 1)[1][0, 0] == ((np.float64(f32(0.1)) + np.float64(f32(0.2))) + np.float64(f32(0.3))) / 3.0

    # ---- hops 2, H = 1, K = 2: first-hop slots (3, 0): slot 1 is padding, so its level-below row (which names node 8 with
    # weight 1) takes no part; slot 0's row names (8, 8): paths q = 0 and q = 1 merge in path order
    raw = dict(nbr=np.array([[3, 0]], np.int32), w=np.array([[[1.0, 0.0]]], f32), dt=np.array([[4.0, 0.0]], f32),
               eidx=np.array([[40, 0]], np.int32),
               nbr2=np.array([[[8, 8], [8, 8]]], np.int32), w2=np.array([[[[0.75, 0.25]], [[0.5, 0.5]]]], f32),
               dt2=np.array([[[9.0, 6.0], [1.0, 1.0]]], f32), eidx2=np.array([[[90, 91], [92, 93]]], np.int32))
    node, weight, n_valid, count, age, eidx = E.explain(raw, 2, hops=2)
    assert node.tolist() == [[8, -1]] and weight.tolist() == [[1.0, 0.0]] and count.tolist() == [[2, 0]] and n_valid.tolist() == [1]
    assert age[0, 0] == 6.0 and eidx.tolist() == [[91, -1]]            # the LAST edge of the path
    # the sum runs in path order q = j K + i: three paths to one node whose weights do not add associatively
    a, b, c = f32(0.7), f32(0.2), f32(0.1)
    raw = dict(nbr=np.array([[3, 4]], np.int32), w=np.array([[[0.5, 0.5]]], f32), dt=np.zeros((1, 2), f32), eidx=np.zeros((1, 2), np.int32),
               nbr2=np.array([[[8, 8], [8, 6]]], np.int32), w2=np.array([[[[a, b]], [[c, 0.5]]]], f32),
               dt2=np.array([[[3.0, 2.0], [2.0, 1.0]]], f32), eidx2=np.array([[[1, 2], [3, 4]]], np.int32))
    node, weight, n_valid, count, age, eidx = E.explain(raw, 4, hops=2)
    h = np.float64(0.5)
    assert weight[0, 0] == ((np.float64(0.0) + h * np.float64(a)) + h * np.float64(b)) + h * np.float64(c)
    assert node.tolist() == [[8, 6, -1, -1]] and count.tolist() == [[3, 1, 0, 0]] and eidx.tolist() == [[2, 4, -1, -1]]
    assert weight[0, 1] == 0.25 and E.dense(node, weight, 10)[0, 8] == weight[0, 0] and E.dense(node, weight, 10).sum() == weight.sum()


def test_host_model_on_the_oracles_weights_gives_distributions():
    """An fp64 oracle's softmax rows sum to 1 within a few ulp, so the merged rows must: to 1 (or 0 when the root has no
    neighbour) at hops = 1, to at most 1 at hops = 2 (the paths through padded second-hop slots and the self row are left out)."""
    cfg = SyntheticConfig("t", 30, 8, 300, 32, 2, 5, 2)
    g = make_graph(cfg, with_prices=False)
    d = g.data
    tgn = P.TGN(P.get_neighbor_finder(d, uniform=False), g.node_features, g.edge_features, "cpu", n_layers=2, n_heads=2, dropout=0.0,
                use_memory=False, n_neighbors=5)
    params = {k: v.detach().cpu().numpy().copy() for k, v in tgn.state_dict().items() if "layer_norm" not in k and not k.startswith("memory.")}
    onf = OracleNeighborFinder(*build_adjacency(d.sources, d.destinations, d.edge_idxs, d.timestamps), uniform=False)
    ref = T.OracleTGN(onf, g.node_features, g.edge_features, params, 2, 2, False, dtype=np.float64)
    nodes = np.arange(1, 39, dtype=np.int64)
    ts = np.full(len(nodes), float(d.timestamps[150]))
    ts[::4] = float(d.timestamps[0])                          # nothing lies before the first interaction: empty rows
    ctx = ref._embed(None, nodes, ts, 2, 5, None)[1]
    n_nodes = g.node_features.shape[0]
    empty = 0
    for hops in (1, 2):
        raw = E.oracle_raw(ctx, hops)
        assert raw["nbr"].shape == (38, 5) and raw["w"].shape == (38, 2, 5)
        node, weight, n_valid, count, age, eidx = E.explain(raw, 256, hops)
        sums = weight.sum(1)
        has = (raw["nbr"] != 0).any(1)
        empty += int((~has).sum())
        assert (n_valid[~has] == 0).all() and (sums[~has] == 0.0).all() and (n_valid[has] > 0).all()
        if hops == 1:
            assert np.abs(sums[has] - 1.0).max() <= 1e-12
            assert (count.sum(1) == (raw["nbr"] != 0).sum(1)).all()
        else:
            assert (sums <= 1.0 + 1e-12).all() and (sums[has] > 0).any()
            full = has & (raw["nbr2"] != 0).any(2).all(1) & (raw["nbr"] != 0).all(1)      # every path's row has a neighbour
            assert full.any() and np.abs(sums[full] - 1.0).max() <= 1e-12
        assert np.abs(E.dense(node, weight, n_nodes).sum(1) - sums).max() <= 1e-12
    assert empty >= 10


@pytest.fixture(scope="module")
def cpu_model():
    g = make_graph(SyntheticConfig("t", 50, 10, 400, 8, 1, 4, 2), with_prices=False)
    nf = P.get_neighbor_finder(g.data, False)
    one = P.TGN(nf, g.node_features, g.edge_features, "cpu", n_layers=1, n_heads=2, use_memory=True, memory_dimension=8,
                message_function="identity")
    two = P.TGN(nf, g.node_features, g.edge_features, "cpu", n_layers=2, n_heads=2, use_memory=False)
    return one, two


@pytest.mark.parametrize("bad", [
    dict(m=0), dict(m=257), dict(m=2.5), dict(hops=0), dict(hops=3), dict(hops=2), dict(hops="a"),
    dict(nodes=[1, 61, 2]), dict(nodes=[-1, 2, 3]), dict(nodes=[[1, 2, 3]]), dict(nodes=[1.5, 2.0, 3.0]),
    dict(timestamps=[1.0, 2.0]), dict(timestamps=np.zeros((3, 1))), dict(timestamps=torch.zeros(2, dtype=torch.float64)),
    dict(n_neighbors=65), dict(n_neighbors=2.5),
], ids=lambda d: "%s=%s" % (next(iter(d)), str(next(iter(d.values()))).replace("\n", "")[:24]))
def test_explain_rejects_bad_arguments_before_asking_for_a_gpu(cpu_model, bad):
    one, two = cpu_model
    args = dict(nodes=[1, 2, 3], timestamps=5.0, m=3)
    args.update(bad)
    with pytest.raises(ValueError):
        one.explain(**args)                                   # (hops=2 on a one-layer model: hops > n_layers)
    if bad.get("hops") != 2:
        with pytest.raises(ValueError):
            two.explain(**args)
    if not torch.cuda.is_available():                         # ... and a valid query without a device is an error, not a fallback
        for tgn, hops in ((one, 1), (two, 2)):
            was = tgn.training
            with pytest.raises(_lib.PfoError):
                tgn.explain([1, 2, 3], 5.0, 3, hops=hops)
            with pytest.raises(_lib.PfoError):
                tgn.explain(torch.tensor([1, 2, 3]), np.array([5.0, 6.0, 7.0]), 256, hops=hops, n_neighbors=0, return_raw=True)
            assert tgn.training == was


def test_entry_is_declared_and_refuses_bad_sizes_before_any_pointer():
    text = open(os.path.join(REPO, "include", "pfotgn.h")).read()
    assert re.search(r"#define PFO_EXPLAIN_MAX_WIDTH\s+256\b", text) and _lib.EXPLAIN_MAX_WIDTH == 256
    assert re.search(r"\bint pfo_tgn_explain\(const pfo_tgn_config\* cfg, const void\* workspace, int32_t R, int32_t K, int32_t hops", text)
    assert len(_lib.PROTOTYPES["pfo_tgn_explain"][1]) == 21 and "explain.hip" in build.SOURCES and hasattr(P.TGN, "explain")
    lib = _lib.load()
    assert hasattr(lib, "pfo_tgn_explain") and lib.pfo_abi_version() == 6
    P8 = 1 << 12                                              # a non-null address that is never followed

    def call(R=4, K=5, hops=1, m=8, L=2, ws=None, outs=(None,) * 6, raw=(None,) * 8, max_roots=16, max_neighbors=10):
        cfg = _lib.TgnConfig(100, 10, 32, 4, L, 2, 1, max_roots, max_neighbors, 4)
        rc = lib.pfo_tgn_explain(ctypes.byref(cfg), ws, R, K, hops, m, *outs, *raw, None)
        return rc, lib.pfo_last_error().decode()
    for kw, word in ((dict(m=0), "m must lie"), (dict(m=257), "m must lie"), (dict(hops=0), "hops must lie"), (dict(hops=3), "hops must lie"),
                     (dict(hops=2, L=1), "hops must lie"), (dict(K=0), "K must lie"), (dict(K=65, max_neighbors=64), "K must lie"),
                     (dict(K=11), "K must lie"), (dict(R=-1), "R must lie"), (dict(R=17), "R must lie")):
        rc, err = call(**kw)
        assert rc == -1 and word in err and err.startswith("pfo_tgn_explain:"), (kw, rc, err)
        if "R" not in kw:
            rc, err = call(R=0, **kw)
            assert rc == -1 and word in err, "the bounds come first, even with nothing to do"
    assert call(R=0)[0] == 0 and call(R=0, hops=2, m=256, K=10)[0] == 0
    rc, err = call()
    assert rc == -1 and "null pointer" in err
    for missing in range(7):                                  # the workspace and each of the six outputs
        ptrs = [P8] * 7
        ptrs[missing] = None
        rc, err = call(ws=ptrs[0], outs=tuple(ptrs[1:]))
        assert rc == -1 and "null pointer" in err, missing
    for group in (0, 4):                                      # a raw group given in part
        raw = [None] * 8
        raw[group], raw[group + 2] = P8, P8
        rc, err = call(hops=2, ws=P8, outs=(P8,) * 6, raw=tuple(raw))
        assert rc == -1 and "raw group" in err, group
    assert lib.pfo_tgn_explain(None, P8, 4, 5, 1, 8, *([P8] * 6), *([None] * 8), None) == -1
    with pytest.raises(_lib.PfoError, match="pfo_tgn_explain: m must lie"):
        cfg = _lib.TgnConfig(100, 10, 32, 4, 2, 2, 1, 16, 10, 4)
        _lib.call("pfo_tgn_explain", ctypes.byref(cfg), None, 4, 5, 1, 0, *([None] * 14), None)
