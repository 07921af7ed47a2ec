"""Host side of the history gather: the numpy reference (``history_ref``) against a plain loop over row entries,
the cases of the GPU test proved binding from the reference alone, the C entry's refusals with NULL pointers, every new
``ValueError`` of ``recommend`` / ``TGN.history`` / ``backtest`` checked without a device, the op's fake, and the signatures."""
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

import pfotgnrec_amd as P
from pfotgnrec_amd import _lib, build
from pfotgnrec_amd import recommend as RC
from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
import history_ref as H
from conftest import REPO

HEADER = os.path.join(REPO, "include", "pfotgn.h")


# ---- the reference

def _small_graph(rs, n_nodes, n_entries):
    """A random CSR with few distinct neighbours (repeats) and timestamps on a coarse grid (ties)."""
    owner = np.sort(rs.randint(0, n_nodes, size=n_entries))
    nbr = [rs.randint(0, 6, size=int((owner == u).sum())).tolist() for u in range(n_nodes)]
    ts = [np.sort(rs.randint(0, 8, size=len(r)).astype(np.float64)).tolist() for r in nbr]
    return H.csr(nbr, ts)


@pytest.mark.parametrize("seed", range(6))
def test_reference_is_the_loop_over_row_entries(seed):
    rs = np.random.RandomState(seed)
    indptr, nbr, ts = _small_graph(rs, 9, 120)
    U = 40
    users = rs.randint(-1, 10, size=U)                          # -1 and 9 are outside the table
    q_ts = rs.randint(0, 9, size=U).astype(np.float64)          # on the grid: query times EQUAL to entries' times
    q_ts[rs.rand(U) < 0.1] = np.nan
    q_ts[rs.rand(U) < 0.05] = np.inf
    since = rs.randint(0, 9, size=U).astype(np.float64)         # on the grid too: an entry AT since is inside
    since[rs.rand(U) < 0.3] = np.nan
    met = dict(strict=0, inclusive=0)
    for W in (1, 2, 4, 256):
        for max_scan in (0, 1, 3):
            for sn in (None, since):
                got = H.gather(indptr, nbr, ts, users, q_ts, W, sn, max_scan)
                loop = H.gather_loop(indptr, nbr, ts, users, q_ts, W, sn, max_scan)
                for q in range(U):
                    k = got.len[q]
                    assert got.node[q, :k].tolist() == loop[q][0] and got.count[q, :k].tolist() == loop[q][2], (W, max_scan, q)
                    assert got.time[q, :k].tolist() == loop[q][1]
                    assert (got.node[q, k:] == -1).all() and np.isnan(got.time[q, k:]).all() and not got.count[q, k:].any()
                    assert len(set(loop[q][0])) == k <= W
    for q in range(U):
        u = users[q]
        if 0 <= u < 9 and np.isfinite(q_ts[q]):
            row = ts[indptr[u]:indptr[u + 1]]
            met["strict"] += int((row == q_ts[q]).any())
            met["inclusive"] += int(not np.isnan(since[q]) and (row == since[q]).any() and since[q] < q_ts[q])
    assert met["strict"] >= 3 and met["inclusive"] >= 3, met    # entries exactly at ts and at since occur


def test_reference_on_a_hand_built_row():
    #            entry:  0    1    2    3    4    5    6
    indptr, nbr, ts = H.csr([[], [5, 6, 5, 7, 6, 8, 5]], [[], [1.0, 2.0, 2.0, 3.0, 3.0, 3.0, 4.0]])
    g = lambda t, W=4, since=None, ms=0: H.gather(indptr, nbr, ts, [1], [t], W, None if since is None else [since], ms)
    r = g(4.0)                                                   # strict: entry 6 (ts 4.0) is not seen
    assert r.node[0].tolist() == [8, 6, 7, 5] and r.count[0].tolist() == [1, 2, 1, 2] and r.time[0].tolist() == [3.0, 3.0, 3.0, 2.0]
    assert g(4.5).node[0].tolist() == [5, 8, 6, 7] and g(4.5).count[0].tolist() == [3, 1, 2, 1]
    assert g(4.5, W=2).node[0].tolist() == [5, 8] and g(4.5, W=2).count[0].tolist() == [3, 1] and g(4.5, W=2).len[0] == 2
    assert g(4.5, since=3.0).node[0].tolist() == [5, 8, 6, 7] and g(4.5, since=3.0).count[0].tolist() == [1, 1, 1, 1]   # inclusive
    assert g(4.5, ms=2).node[0].tolist() == [5, 8, -1, -1] and g(4.5, since=1.0, ms=3).count[0].tolist() == [1, 1, 1, 0]
    assert g(1.0).len[0] == 0 and g(float("nan")).len[0] == 0 and g(float("inf")).len[0] == 0 and g(4.5, since=9.0).len[0] == 0
    assert g(4.5, since=float("nan")).len[0] == 4
    r = H.gather(indptr, nbr, ts, [1, 0, 2, -1], [9.0] * 4, 4, items=[7, 99, 5], upper_u=5)
    assert r.pos[0].tolist() == [2, -1, -1, 0] and r.stock[0].tolist() == [-1, 2, 0, 1] and r.len.tolist() == [4, 0, 0, 0]
    assert (r.pos[1:] == -1).all() and (r.stock[1:] == -1).all()


def test_gpu_cases_are_binding():
    """What tests/test_gpu_history.py rests on, shown from the reference alone: a case is one (U, W) pair, made of the calls
    ``history_ref.calls(U)`` lists (every ``max_scan`` and none).  In EVERY case at least one user is cut by W, one has
    repeats, one has an empty window, one is cut by ``since`` and one by ``max_scan`` - and the world's rows are what they say."""
    indptr, nbr, ts = H.world()
    assert (np.diff(indptr)[1:9] == H.ROW_LENGTHS).all() and indptr[-1] == len(nbr) == len(ts)
    assert all((np.diff(ts[indptr[u]:indptr[u + 1]]) >= 0).all() for u in range(H.N_NODES)), "rows are time-sorted"
    assert nbr.min() >= 1 and nbr.max() < H.N_NODES
    tied = ts[indptr[H.TIED_ROW]:indptr[H.TIED_ROW + 1]]
    assert len(tied) == 100 and (tied == tied[0]).all()
    chunk = nbr[indptr[H.CHUNK_ROW]:indptr[H.CHUNK_ROW + 1]]
    assert len(chunk) == 40 and (chunk[0::2] == chunk[1::2]).all()                        # repeats inside one chunk
    cross = nbr[indptr[H.CROSS_ROW]:indptr[H.CROSS_ROW + 1]]
    assert (cross[:-70] == cross[70:]).all() and len(set(cross.tolist())) == 70           # repeats 70 entries apart: across chunks
    full = H.gather(indptr, nbr, ts, [H.FULL_ROW], [1e9], 256)
    assert full.len[0] == 256 and (full.count[0, :20] == 5).all() and (full.count[0, 20:] == 1).all()   # counted after the list is full
    assert len(set(nbr[indptr[H.WIDE_ROW]:indptr[H.WIDE_ROW + 1]].tolist())) == 400
    n5000 = H.ROW_LENGTHS[-1]
    steps, n = 0, n5000
    while n > 64:                                                                          # the 64-ary search of the kernel
        n, steps = (n + 63) // 64 - 1, steps + 1
    assert steps + 1 == 3, "a row of 5000 entries takes three search steps"
    for U in H.USER_COUNTS:
        for W in H.WIDTHS:
            total = dict(cut_by_W=0, repeats=0, empty=0, cut_by_since=0, cut_by_max_scan=0)
            per_seed = {}
            for seed, max_scan in H.calls(U):
                users, q_ts, since = H.queries(indptr, ts, U, seed)
                b = {name: int(v) for name, v in H.binding(indptr, nbr, ts, users, q_ts, W, since, max_scan).items()}
                for name, v in b.items():
                    total[name] += v
                    per_seed.setdefault(seed, dict.fromkeys(b, 0))[name] += v
                if U == 67:
                    # no aggregate here: EVERY launch of 67 users meets every rule it can meet (one entry cannot repeat, a
                    # window of max_scan entries is not cut by a W of that many - at 65 it takes 65 distinct ids to be cut by
                    # 64 -, no max_scan cuts nothing)
                    print("U=67 W=%d max_scan=%d: %s" % (W, max_scan, b))
                    assert b["empty"] >= 5 and b["cut_by_since"] >= 5, (W, max_scan, b)
                    assert b["cut_by_max_scan"] >= 5 or max_scan == 0, (W, max_scan, b)
                    assert b["repeats"] >= 5 or max_scan == 1, (W, max_scan, b)
                    assert b["cut_by_W"] >= 5 or (max_scan > 0 and W >= min(max_scan, 64)), (W, max_scan, b)
            print("U=%d W=%d: %s" % (U, W, total))
            assert all(v >= 3 for v in total.values()), (U, W, total)
            if U == 5:
                # ... and for 5 users no few seeds carry the case: every seed's four calls together meet every rule but the cut
                # by a W of 64 or more, which takes one of the three long rows
                for seed, b in per_seed.items():
                    assert b["repeats"] >= 2 and b["empty"] >= 2 and b["cut_by_since"] >= 1 and b["cut_by_max_scan"] >= 2, (W, seed, b)
                    assert b["cut_by_W"] >= 2 or W >= 64, (W, seed, b)
            if U == 1:
                hit = {name: sum(b[name] > 0 for b in per_seed.values()) for name in total}
                print("U=1 W=%d, seeds that meet each rule: %s" % (W, hit))
                assert all(v >= 3 for v in hit.values()), (W, hit)
    users, q_ts, since = H.queries(indptr, ts, 67, 3)
    assert np.isnan(q_ts).any() and np.isposinf(q_ts).any() and np.isneginf(q_ts).any() and np.isnan(since).any()
    assert np.isposinf(since).any() and np.isneginf(since).any() and (users == -1).any() and (users == H.N_NODES).any()
    on_entry = sum(bool((ts[indptr[u]:indptr[u + 1]] == t).any()) for u, t in zip(users, q_ts) if 0 <= u < H.N_NODES)
    on_since = sum(bool((ts[indptr[u]:indptr[u + 1]] == s).any()) for u, s in zip(users, since) if 0 <= u < H.N_NODES)
    assert on_entry >= 10 and on_since >= 5, "query times and since values that sit ON an entry's timestamp"


# ---- the C entry

def test_header_prototype_and_symbol():
    text = open(HEADER).read()
    assert re.search(r"#define PFO_HISTORY_MAX_WIDTH\s+256\b", text) and _lib.HISTORY_MAX_WIDTH == 256
    assert re.search(r"\bint pfo_history_gather\(const int64_t\* indptr, const int32_t\* adj_nbr, const double\* adj_ts", text)
    assert "pfo_history_gather" in _lib.PROTOTYPES and len(_lib.PROTOTYPES["pfo_history_gather"][1]) == 21
    lib = _lib.load()
    assert hasattr(lib, "pfo_history_gather") and lib.pfo_abi_version() == 6 and "history.hip" in build.SOURCES
    assert hasattr(P, "history_gather") and hasattr(P.TGN, "history")


def _null_call(U=4, W=8, n_nodes=10, max_scan=0, I=1, pos_out=None, **ptrs):
    P8 = 1 << 12                                                # a non-null address that is never followed
    p = dict(indptr=None, adj_nbr=None, adj_ts=None, users=None, ts=None, since=None, items=None, pos_scratch=None, node_out=None,
             len_out=None)
    p.update({k: P8 for k, v in ptrs.items() if v})
    lib = _lib.load()
    rc = lib.pfo_history_gather(p["indptr"], p["adj_nbr"], p["adj_ts"], n_nodes, p["users"], p["ts"], p["since"], U, W, max_scan,
                                p["items"], I, p["pos_scratch"], 0, p["node_out"], p["len_out"], None, None, P8 if pos_out else None,
                                None, None)
    return rc, lib.pfo_last_error().decode()


def test_entry_refuses_bad_sizes_before_any_pointer():
    for kw, word in ((dict(W=0), "W must lie"), (dict(W=257), "W must lie"), (dict(W=-1), "W must lie"), (dict(U=-1), "U must lie"), (dict(U=2 ** 62), "U must lie"),
                     (dict(n_nodes=0), "n_nodes"), (dict(n_nodes=2 ** 31), "n_nodes"), (dict(max_scan=-1), "max_scan"),
                     (dict(pos_out=True, I=0), "I must lie"), (dict(pos_out=True, I=65537), "I must lie")):
        rc, err = _null_call(**kw)
        assert rc == -1 and word in err and err.startswith("pfo_history_gather:"), (kw, rc, err)
        rc, err = _null_call(U=0, **{k: v for k, v in kw.items() if k != "U"}) if "U" not in kw else (rc, err)
        assert rc == -1 and word in err, "the bounds come first, even with nothing to do"
    rc, err = _null_call()
    assert rc == -1 and "null pointer" in err and err.startswith("pfo_history_gather:")
    everything = dict(indptr=1, adj_nbr=1, adj_ts=1, users=1, ts=1, node_out=1, len_out=1)
    for missing in everything:
        rc, err = _null_call(**dict(everything, **{missing: 0}))
        assert rc == -1 and "null pointer" in err, missing
    for missing in ("items", "pos_scratch"):                     # needed only with pos_out
        rc, err = _null_call(pos_out=True, **dict(dict(everything, items=1, pos_scratch=1), **{missing: 0}))
        assert rc == -1 and "positions need items and pos_scratch" in err, missing
    assert _null_call(U=0)[0] == 0 and _null_call(U=0, W=256, n_nodes=2 ** 31 - 1, max_scan=2 ** 40)[0] == 0
    assert _null_call(U=0, pos_out=True, I=65536)[0] == 0
    with pytest.raises(_lib.PfoError, match="pfo_history_gather: W must lie"):
        _lib.call("pfo_history_gather", *([None] * 3), 10, None, None, None, 4, 0, 0, None, 1, None, 0, *([None] * 7))


def test_functional_refuses_on_the_host():
    i32, f64 = (lambda *s: torch.zeros(s, dtype=torch.int32)), (lambda *s: torch.zeros(s, dtype=torch.float64))
    good = dict(indptr=torch.zeros(11, dtype=torch.int64), adj_nbr=i32(0), adj_ts=f64(0), users=i32(3), ts=f64(3), width=8)
    for kw, msg in ((dict(width=0), r"width must lie in \[1, 256\]"), (dict(width=257), "width must lie"), (dict(width="a"), "integers"),
                    (dict(max_scan=-1), "max_scan must not be negative"), (dict(indptr=i32(11)), "indptr must be int64"),
                    (dict(indptr=torch.zeros(1, dtype=torch.int64)), "indptr must be int64"), (dict(adj_nbr=i32(2)), "adjacency must be"),
                    (dict(adj_ts=torch.zeros(0)), "adjacency must be"), (dict(users=i32(3).long()), "users must be int32"),
                    (dict(ts=f64(4)), "ts must be float64"), (dict(ts=torch.zeros(3)), "ts must be float64"),
                    (dict(since=f64(2)), "since must be float64"), (dict(want=("node", "nodes")), "want must name"),
                    (dict(want=("pos",)), "positions need items"), (dict(want=("pos",), items=i32(0)), "between 1 and 65536"),
                    (dict(want=("pos",), items=i32(3).long()), "positions need items"), (dict(want=("stock",)), "stock indices need upper_u"),
                    (dict(want=("stock",), upper_u=-1), "upper_u"),
                    # a scratch of the caller's that cannot serve is refused, never quietly replaced
                    (dict(want=("pos",), items=i32(3), pos_scratch=i32(9)), "pos_scratch must be a contiguous int32 tensor of at least n_nodes = 10"),
                    (dict(want=("pos",), items=i32(3), pos_scratch=i32(10).long()), "pos_scratch must be"),
                    (dict(want=("pos",), items=i32(3), pos_scratch=i32(10, 2)[:, 0]), "pos_scratch must be")):
        with pytest.raises(ValueError, match=msg):
            P.history_gather(**dict(good, **kw))
    if not torch.cuda.is_available():
        with pytest.raises(_lib.PfoError):                       # valid: only the device is missing - no fallback
            P.history_gather(**good)


def test_op_is_registered_with_a_fake():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from pfotgnrec_amd import ops  # noqa: F401
    assert hasattr(torch.ops.pfotgn, "history_gather")
    with FakeTensorMode():
        ind, nbr, ts = torch.empty(11, dtype=torch.int64), torch.empty(50, dtype=torch.int32), torch.empty(50, dtype=torch.float64)
        users, q_ts = torch.empty(7, dtype=torch.int32), torch.empty(7, dtype=torch.float64)
        out = torch.ops.pfotgn.history_gather(ind, nbr, ts, users, q_ts, 16)
        assert [tuple(t.shape) for t in out] == [(7, 16), (7,), (7, 16), (7, 16), (7, 0), (7, 0)]
        assert [t.dtype for t in out] == [torch.int32, torch.int32, torch.float64, torch.int32, torch.int32, torch.int32]
        out = torch.ops.pfotgn.history_gather(ind, nbr, ts, users, q_ts, 3, since=q_ts, max_scan=5, items=torch.empty(9, dtype=torch.int32),
                                              upper_u=4)
        assert [tuple(t.shape) for t in out] == [(7, 3), (7,), (7, 3), (7, 3), (7, 3), (7, 3)]


# ---- recommend / history / backtest: checked on the host, before any device is asked for

@pytest.fixture(scope="module")
def cpu_model():
    g = make_graph(SyntheticConfig("t", 50, 10, 400, 8, 1, 4, 2), with_prices=False)
    nf = P.get_neighbor_finder(g.data, False)
    tgn = P.TGN(nf, g.node_features, g.edge_features, "cpu", n_layers=1, n_heads=2, use_memory=True, memory_dimension=8,
                message_function="identity")
    mv = types.SimpleNamespace(returns=torch.zeros(4, 10, 29, dtype=torch.float64), upper_u=50, gamma=2.0, lambda_mv=0.5,
                               day_of=lambda ts: np.asarray(ts, np.int64) % 4)
    return tgn, np.arange(51, 61), mv


def test_signatures_keep_their_tails():
    names = list(inspect.signature(P.TGN.recommend).parameters)
    assert names[-3:] == ["only", "groups", "group_cap"]
    assert names[names.index("stock_groups") + 1:-3] == ["seen_since", "seen_width", "seen_max_scan"]
    params = inspect.signature(P.TGN.recommend).parameters
    assert all(params[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("seen_since", "seen_width", "seen_max_scan"))
    assert (params["seen_since"].default, params["seen_width"].default, params["seen_max_scan"].default) == (None, None, 0)
    v = inspect.signature(RC.validate).parameters
    assert list(v)[-3:] == ["seen_since", "seen_width", "seen_max_scan"] and all(
        v[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(v)[-3:])
    assert RC.Query._fields[-5:] == ("seen", "seen_since", "seen_width", "seen_max_scan", "basket")
    assert list(inspect.signature(P.TGN.history).parameters) == ["self", "users", "timestamps", "width", "since", "max_scan", "items"]
    for fn in (P.backtest, P.backtest_rows):
        assert {"seen_since", "seen_width", "seen_max_scan"} <= set(inspect.signature(fn).parameters)


def test_seen_is_validated_on_the_host(cpu_model):
    tgn, items, mv = cpu_model
    good = dict(users=[1, 2, 3], timestamps=5.0, k=3, items=items)
    for kw, msg in ((dict(seen_since=1.0), "go with exclude=\"seen\""), (dict(seen_width=8), "go with exclude=\"seen\""),
                    (dict(seen_max_scan=5), "go with exclude=\"seen\""), (dict(exclude=[[51], [], []], seen_width=8), "go with exclude=\"seen\""),
                    (dict(exclude="seen", seen_width=0), r"seen_width must lie in \[1, 256\]"),
                    (dict(exclude="seen", seen_width=257), "seen_width must lie"), (dict(only="seen", seen_width=2.5), "must be integers"),
                    (dict(exclude="seen", seen_max_scan=-1), "seen_max_scan must not be negative"),
                    (dict(exclude="seen", seen_since=[1.0, 2.0]), "seen_since must be a scalar or hold one value"),
                    (dict(exclude="seen", seen_since=torch.zeros(4, dtype=torch.float64)), "seen_since must be a scalar or hold one value"),
                    (dict(exclude="seen", seen_since="x"), "seen_since must be a number"),
                    (dict(portfolios="seen"), 'portfolios="seen" needs mv'),
                    (dict(portfolios="seen", held_groups="portfolios", stock_groups=[0] * 10, groups=[0] * 10, group_cap=1),
                     'portfolios="seen" needs mv'),
                    # what is refused for explicit rows stays refused
                    (dict(only="seen", exclude=[[51], [], []]), "only and exclude cannot be combined"),
                    (dict(only="seen", exclude="seen"), "only and exclude cannot be combined"),
                    (dict(only="seen", exclude="held"), "only and exclude cannot be combined"),
                    (dict(only="seen", mv=mv, portfolios="seen", basket=True), "only and basket=True cannot be combined"),
                    (dict(only="seen", groups=[0] * 10, group_cap=1), "groups and only cannot be combined"),
                    (dict(exclude="sen"), "exclude must be None"), (dict(only="SEEN"), "only must be None"),
                    (dict(exclude="held"), "holdings ledger")):
        with pytest.raises(ValueError, match=msg):
            tgn.recommend(**dict(good, **kw))
    args = (tgn.n_nodes, tgn.n_neighbors, [1, 2, 3], 5.0, 3, items)
    q = RC.validate(*args, "seen", None, None)
    assert q.seen == (True, False, False) and (q.seen_since, q.seen_width, q.seen_max_scan) == (None, 256, 0) and q.held is None
    assert q.ex_ids is None and RC.validate(*args, None, None, None).seen is None
    q = RC.validate(*args, None, None, None, mv, "seen", None, None, False, "seen", seen_since=np.float32(2.5), seen_width=7, seen_max_scan=9)
    assert q.seen == (False, True, True) and (q.seen_since, q.seen_width, q.seen_max_scan) == (2.5, 7, 9)
    assert q.held is None and q.mv.port_idx is None and q.only_ids is None and not q.only_held
    q = RC.validate(*args, "seen", None, None, seen_since=[1.0, np.nan, 3.0])
    assert isinstance(q.seen_since, np.ndarray) and q.seen_since.dtype == np.float64 and q.seen_since.shape == (3,)
    dev_since = torch.zeros(3, dtype=torch.float64)
    assert RC.validate(*args, "seen", None, None, seen_since=dev_since).seen_since is dev_since
    if not torch.cuda.is_available():
        for kw in (dict(exclude="seen"), dict(only="seen", seen_width=4), dict(mv=mv, portfolios="seen", exclude="seen")):
            with pytest.raises(_lib.PfoError):                   # valid: only the device is missing - no fallback
                tgn.recommend(**dict(good, **kw))


def test_history_is_validated_on_the_host(cpu_model):
    tgn, items, _ = cpu_model
    for args, kw, msg in ((([1, 2], 5.0, 0), {}, r"^width must lie in \[1, 256\]"), (([1, 2], 5.0, 257), {}, "^width must lie"),
                          (([1, 2], 5.0, 2.5), {}, "^width and max_scan must be integers"),
                          (([1, 2], 5.0, 8), dict(max_scan=-2), "^max_scan must not be negative"),
                          (([1, 2], 5.0, 8), dict(since="x"), "^since must be a number"), (([1, 2], [5.0], 8), {}, "timestamps must be a scalar"),
                          (([1, 2], 5.0, 8), dict(since=[1.0, 2.0, 3.0]), "^since must be a scalar or hold one value"),
                          (([1, tgn.n_nodes], 5.0, 8), {}, "users holds node ids outside"), (([[1, 2]], 5.0, 8), {}, "users must be a 1-D"),
                          (([1, 2], "x", 8), {}, "timestamps must be numbers"),
                          (([1, 2], 5.0, 8), dict(items=[51, 51]), "items holds duplicates"),
                          (([1, 2], 5.0, 8), dict(items=[]), "between 1 and 65536"),
                          (([1, 2], 5.0, 8), dict(items=[51, tgn.n_nodes]), "items holds node ids outside")):
        with pytest.raises(ValueError, match=msg):
            tgn.history(*args, **kw)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.PfoError):
            tgn.history([1, 2], 5.0, 8, items=items)


def test_backtest_refuses_seen_arguments_before_any_device_work():
    tgn = types.SimpleNamespace(holdings=None, device=torch.device("cuda:0"), n_nodes=40)
    p = 100.0 + np.arange(2 * 4 * 6, dtype=np.float64).reshape(2, 4, 6)
    tables = P.InvestTables.from_prices(["20200101", "20200102"], p, p + 1.0, {"a": 0, "b": 1, "c": 2, "d": 3}, upper_u=20)
    n = 8
    base = dict(sources=np.arange(1, n + 1), destinations=np.arange(21, 21 + n), edge_times=20200101000000.0 + np.arange(n),
                edge_idxs=np.arange(1, n + 1), items=np.arange(21, 25), k=3, cutoffs=(1, 3), batch_size=4, tables=tables)
    for kw, msg in ((dict(seen_width=8), "go with exclude=\"seen\""), (dict(exclude="held", seen_since=1.0), "go with exclude=\"seen\""),
                    (dict(exclude="seen", seen_width=300), "seen_width must lie"), (dict(exclude="seen", seen_max_scan=-1), "must not be negative"),
                    (dict(exclude="seen", seen_since=np.zeros(7)), "the log holds 8"), (dict(portfolios="seen"), 'portfolios="seen" needs mv')):
        for fn in (P.backtest, P.backtest_rows):
            with pytest.raises(ValueError, match=msg):
                fn(tgn, **dict(base, **kw))
    # portfolios="seen" under held_groups="portfolios" passes every check: a seen row fits the held-group row like a ledger row
    import importlib
    BT = importlib.import_module("pfotgnrec_amd.backtest")               # (the package exports the function under the same name)
    mv = types.SimpleNamespace(returns=np.zeros((2, 4, 5)), upper_u=20, gamma=2.0, lambda_mv=0.5, day_of=lambda t: np.zeros(len(t), int))
    log = [base[name] for name in ("sources", "destinations", "edge_times", "edge_idxs")]
    out = BT.check(tgn, *log, base["items"], 3, (1, 3), 4, tables, None, mv, False, "seen", "seen", None, [0, 1, 0, 1], 1, 5.0, None, 9)
    assert out[0] == n and out[6] == "seen" and out[7] == "seen" and out[8] == (5.0, 256, 9)
    for pf_log in ("seen", "held"):
        assert BT.check_held_groups(tgn, n, "portfolios", [0, 1, 0, 1], [0, 1, 0, 1], pf_log)[0] == "portfolios"
    wide = (np.zeros((n, 257), np.int32), np.zeros(n, np.int32))
    with pytest.raises(ValueError, match="at most 256"):
        BT.check_held_groups(tgn, n, "portfolios", [0, 1, 0, 1], [0, 1, 0, 1], wide)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.PfoError):                       # valid: only the device is missing
            P.backtest_rows(tgn, **dict(base, mv=mv, exclude="seen", portfolios="seen", held_groups="portfolios", stock_groups=[0, 1, 0, 1],
                                        groups=[0, 1, 0, 1], group_cap=1, seen_since=5.0))
