"""GPU tests of the portfolio-aware top-k: ``pfo_recommend_mv_topk`` against the numpy reference of ``recommend_mv_ref`` (bit for
bit on exact arithmetic; on random embeddings the score within the fp32 dot-product bound and everything behind the score
exact), against ``pfo_recommend_topk`` at lambda = 0, and ``TGN.recommend(mv=...)`` end to end on the small world."""
import types

import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

import pfotgnrec_amd as P
from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
from oracle import tgn_oracle as T
from oracle.neighbor_finder import OracleNeighborFinder, build_adjacency
from parity import relerr
import recommend_ref as R
import recommend_mv_ref as M

DEV = "cuda:0"
RTOL_EMB = 1e-4      # BASELINE.json north_star: embeddings within 1e-4 relative (max norm)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _kernel(c, lam, k, n_t, want_all=True):
    out = P.recommend_mv_topk(_dev(c["user_emb"]), _dev(c["item_emb"]), k, _dev(c["cand_stock"]), _dev(c["returns"]),
                              _dev(c["day_idx"]), _dev(c["port_idx"]), _dev(c["port_len"]), c["gamma"], lam, _dev(c["user_block"]),
                              _dev(c.get("excl_pos")), _dev(c.get("excl_len")), _dev(c.get("item_ok")), n_blocks=n_t, want_all=want_all)
    names = ("top_pos", "top_score", "top_fused", "n_valid", "score", "y", "fused")
    return {n: t.cpu().numpy() for n, t in zip(names, out)}


def _same_f64(a, b):
    """Equal as fp64 values, NaN in the same places."""
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def _assert_equals_reference(got, ref, tag):
    assert np.array_equal(got["n_valid"], ref["n_valid"]), tag
    assert np.array_equal(got["top_pos"], ref["top_pos"]), tag
    assert np.array_equal(got["top_score"].view(np.int32), ref["top_score"].view(np.int32)), tag
    assert np.array_equal(got["top_fused"], ref["top_fused"]), tag
    assert _same_f64(got["y"], ref["y"]), tag
    assert _same_f64(got["fused"], ref["fused"]), tag


# ---------------------------------------------------------------------------------------------- the kernel alone

@pytest.mark.parametrize("I", [1, 63, 65, 513, 2048])
def test_exact_arithmetic_bit_exact_everything(I):
    """Embeddings are integers in [-3, 3] (every fp32 score exact in any order: asserted here from the fp64 scores) and the
    return tables integers / 64 with rows summing to a multiple of n_ret (every mean, deviation and sum of products exact in any
    order: ``recommend_mv_ref``), so positions, counts, scores, fused values and the whole y and fused rows must be the
    reference's to the last bit - ties in y (shared and duplicated stocks) and in the score, +-inf y (n_ret = 2), the NaN y of
    the constant stock, cand_stock outside the table, portfolios of 0, 1 and W entries with duplicates and out-of-range
    entries, days outside the table, user 0 short of candidates, users of mixed blocks.  63 / 65 / 513 are no multiples of the
    16-wide tile or of the 256 threads that share a user's candidates; 2048 is the bound (144 KB of LDS)."""
    U, n_t, full, seed = 17, 2, 0, 0
    for n_ret in (2, 29):
        for D in (4, 172):
            for k in (1, 64):
                seed += 1
                c = M.exact_case(100 * I + seed, U, I, D, k, n_t, n_ret)
                s64 = R.scores64(c["user_emb"], c["item_emb"], c["user_block"], I)
                assert np.array_equal(s64.astype(np.float32).astype(np.float64), s64) and np.abs(s64).max() < 2 ** 24
                y = None
                for lam in (0.0, 0.5, 1.0, 0.1):
                    ref = M.reference(c, lam, k, y=y)
                    y = ref["y_raw"]
                    got = _kernel(c, lam, k, n_t)
                    tag = (I, n_ret, D, k, lam)
                    assert np.array_equal(got["score"].astype(np.float64), s64), tag
                    _assert_equals_reference(got, ref, tag)
                    if I >= 3:
                        assert ref["n_valid"][0] < k, "user 0 must be short of candidates"
                        assert np.isnan(ref["y"][:, [0, I - 1]]).all() and (ref["n_valid"][[5, U - 1]] == 0).all()
                    full += int((ref["n_valid"] == k).sum())
    assert I < 63 or full > 100, "full rows must be the rule"


@pytest.mark.parametrize("D", [48, 64, 112, 128])
def test_exact_arithmetic_at_the_middle_row_widths(D):
    """The row widths the test above does not reach (the kernel is built for rows of up to 32, 64, 128, 176 and 256 floats): the
    instantiations for 64 and 128, at both ends of each.  Exact arithmetic, everything equal to the reference to the bit."""
    U, I, k, n_t, lam = 17, 65, 5, 2, 0.5
    c = M.exact_case(9000 + D, U, I, D, k, n_t, 29)
    s64 = R.scores64(c["user_emb"], c["item_emb"], c["user_block"], I)
    ref, got = M.reference(c, lam, k), _kernel(c, lam, k, n_t)
    assert (ref["n_valid"] == 0).any() and (ref["n_valid"] == k).any()
    assert np.array_equal(got["score"].astype(np.float64), s64), D
    _assert_equals_reference(got, ref, D)


@pytest.mark.parametrize("seed,U,I,D,k,n_t", [(11, 37, 500, 172, 10, 1), (12, 5, 130, 32, 5, 1), (13, 21, 70, 32, 5, 3)])
def test_lambda_zero_is_the_plain_kernel(seed, U, I, D, k, n_t):
    """With lambda = 0 fused is the average-tie rank of the score, whose canonical order is the canonical order of the score:
    on inputs without a NaN y the new kernel must return ``pfo_recommend_topk``'s positions, scores and counts bit for bit
    (the same matrix-core path and accumulation order: one device function)."""
    c = R.normal_case(seed, U, I, D, n_t)
    c.update(M.mv_side(seed, U, I, 29, clean=True))
    got = _kernel(c, 0.0, k, n_t)
    assert not np.isnan(M.y_matrix(c["returns"], c["day_idx"], c["cand_stock"], c["port_idx"], c["port_len"])).any()
    pos, score, n = (t.cpu().numpy() for t in P.recommend_topk(_dev(c["user_emb"]), _dev(c["item_emb"]), k, _dev(c["user_block"]),
                                                               _dev(c["excl_pos"]), _dev(c["excl_len"]), _dev(c["item_ok"]), n_blocks=n_t))
    assert np.array_equal(got["top_pos"], pos) and np.array_equal(got["n_valid"], n)
    assert np.array_equal(got["top_score"].view(np.int32), score.view(np.int32))
    assert np.array_equal(np.take_along_axis(got["score"], np.clip(pos, 0, None).astype(np.int64), 1)[pos >= 0], score[pos >= 0])


@pytest.mark.parametrize("seed,U,I,D,k", [(11, 37, 500, 172, 10), (12, 5, 130, 32, 5)])
def test_lambda_one_on_random_normal_embeddings(seed, U, I, D, k):
    """fused = rank of y: the rounding of the scores cannot touch the order, so positions, fused values, counts and the y /
    fused rows are the reference's for EVERY user; the returned scores are within the fp32 dot-product bound."""
    c = R.normal_case(seed, U, I, D)
    c.update(M.mv_side(seed, U, I, 29))
    ref = M.reference(c, 1.0, k)
    got = _kernel(c, 1.0, k, 1)
    eps = R.dot_error_bound(c["user_emb"], c["item_emb"], None, I)
    assert (np.abs(got["score"].astype(np.float64) - ref["s64"]) <= eps).all()
    for name in ("top_pos", "n_valid", "top_fused"):
        assert np.array_equal(got[name], ref[name]), name
    assert _same_f64(got["y"], ref["y"]) and _same_f64(got["fused"], ref["fused"])
    valid = got["top_pos"] >= 0
    assert np.array_equal(got["top_score"][valid], np.take_along_axis(got["score"], np.clip(got["top_pos"], 0, None).astype(np.int64), 1)[valid])
    assert (ref["n_valid"] == k).sum() >= U - 3 and np.isneginf(got["top_score"][~valid]).all()


@pytest.mark.parametrize("lam", [0.5, 0.1])
@pytest.mark.parametrize("seed,U,I,D,k", M.BLEND_CASES)
def test_blend_on_random_normal_embeddings_in_two_stages(seed, U, I, D, k, lam):
    """(a) every score is within eps(u, i) = gamma_D sum |u_d v_d| of the fp64 score (``recommend_ref.dot_error_bound``: the
    bound of an fp32 dot product in any order); (b) the reference's ``fuse`` applied to the kernel's OWN scores reproduces
    positions, fused values and counts exactly - everything behind the score is exact.  A user none of whose admissible
    candidates have fp64 scores closer than the sum of their eps has the fp64 order of scores whatever the rounding, so for
    those users the positions are the reference's from the fp64 scores; the seeds (``recommend_mv_ref.BLEND_CASES``, I = 40,
    D = 32) leave that share at 1.0 for both cases - every user - computed from the inputs alone in
    tests/test_recommend_mv_cpu.py; the condition here is one user in two."""
    c = R.normal_case(seed, U, I, D)
    c.update(M.mv_side(seed, U, I, 29))
    ref = M.reference(c, lam, k)
    got = _kernel(c, lam, k, 1)
    eps = R.dot_error_bound(c["user_emb"], c["item_emb"], None, I)
    err = np.abs(got["score"].astype(np.float64) - ref["s64"])
    print("FIGURES recommend_mv_topk (%d,%d,%d,%d) lambda %.1f: largest |score error| / eps %.3f" % (U, I, D, k, lam, (err / eps).max()))
    assert (err <= eps).all()                                                                        # (a)
    own = M.reference(c, lam, k, scores=got["score"])
    _assert_equals_reference(got, own, (seed, lam))                                                  # (b)
    base = R.admissible(U, I, c["excl_pos"], c["excl_len"], c["item_ok"])
    sep = np.array([M.separated_share(ref["s64"][u:u + 1], eps[u:u + 1], base[u:u + 1]) == 1.0 for u in range(U)])
    print("FIGURES separated share %.3f" % sep.mean())
    assert sep.mean() >= 0.5
    assert np.array_equal(got["top_pos"][sep], ref["top_pos"][sep]) and np.array_equal(got["top_fused"][sep], ref["top_fused"][sep])


def test_optional_arguments_errors_and_the_dispatcher_op():
    c = M.exact_case(5, 19, 70, 32, 5, 1, 29)
    plain = dict(c, excl_pos=None, excl_len=None, item_ok=None, port_idx=None, port_len=None)
    ref = M.reference(plain, 0.5, 5)
    got = _kernel(plain, 0.5, 5, 1)                                    # nothing skipped, nobody holds anything
    _assert_equals_reference(got, ref, "plain")
    short = _kernel(plain, 0.5, 5, 1, want_all=False)
    assert len(short) == 4 and all(np.array_equal(short[n], got[n]) for n in short)
    op = torch.ops.pfotgn.recommend_mv_topk(_dev(c["user_emb"]), _dev(c["item_emb"]), 5, _dev(c["cand_stock"]), _dev(c["returns"]),
                                            _dev(c["day_idx"]), 2.0, 0.5, 1, _dev(c["port_idx"]), None, None, _dev(c["excl_pos"]))
    ref = M.reference(dict(c, port_len=None, excl_len=None, item_ok=None), 0.5, 5)      # no lengths: whole rows
    for t, name in zip(op, ("top_pos", "top_score", "top_fused", "n_valid")):
        assert np.array_equal(t.cpu().numpy(), ref[name]), name
    from pfotgnrec_amd import _lib
    ue, ie = _dev(c["user_emb"]), _dev(c["item_emb"])
    out = torch.empty(19 * 5 * 8, dtype=torch.int32, device=DEV)
    args = lambda I, k, n_ret: ("pfo_recommend_mv_topk", ue.data_ptr(), ie.data_ptr(), None, 19, I, 1, 32, None, None, 0, None,
                                _dev(c["cand_stock"]).data_ptr(), _dev(c["returns"]).data_ptr(), 3, 72, n_ret, _dev(c["day_idx"]).data_ptr(),
                                None, None, 0, 2.0, 0.5, k, out.data_ptr(), out.data_ptr(), out.data_ptr(), None, None, None, None,
                                _lib.stream_ptr())
    for bad, msg in ((args(2049, 5, 29), "I must be"), (args(70, 65, 29), "k must be"), (args(70, 5, 1), "n_ret must be")):
        with pytest.raises(_lib.PfoError, match=msg):
            _lib.call(*bad)


# ---------------------------------------------------------------------------------------------- TGN.recommend end to end
# (the world of test_gpu_recommend.py)

N_USERS, N_ITEMS, K_NBR, BATCH = 1000, 100, 10, 40


class _World:
    """A C1-size synthetic graph, the model and the oracle on the same parameters, both advanced by a few training-path calls
    so that memory and pending messages are populated; return tables of N_ITEMS stocks over four days next to it."""

    def __init__(self, L, use_mem):
        torch.manual_seed(77 + L)
        self.L, self.use_mem = L, use_mem
        self.cfg = SyntheticConfig("t", N_USERS, N_ITEMS, 10_000, 32, L, K_NBR, 2)
        self.g = g = make_graph(self.cfg, with_prices=False)
        d = g.data
        self.tgn = P.TGN(P.get_neighbor_finder(d, uniform=False), g.node_features, g.edge_features, DEV, n_layers=L, n_heads=2,
                         dropout=0.0, use_memory=use_mem, memory_dimension=32, message_function="identity", n_neighbors=K_NBR)
        with torch.no_grad():
            self.tgn.time_encoder.w.bias.normal_(0, 0.3)
            for att in self.tgn.embedding_module.attention_models:
                att.multi_head_target.in_proj_bias.normal_(0, 0.1)
                att.multi_head_target.out_proj.bias.normal_(0, 0.1)
        onf = OracleNeighborFinder(*build_adjacency(d.sources, d.destinations, d.edge_idxs, d.timestamps), uniform=False)
        self.names = [k for k in self.tgn.state_dict() if "layer_norm" not in k and not k.startswith("memory.")]
        self.ref = T.OracleTGN(onf, g.node_features, g.edge_features, self._params(), L, 2, use_mem)
        self.rs = np.random.RandomState(5)
        self.cursor = 6000
        for _ in range(3):
            self.step(grad=False)
        self.items = np.arange(N_USERS + 1, N_USERS + N_ITEMS + 1)
        self.users = np.unique(d.sources[self.cursor - 3 * BATCH:self.cursor])[:29]     # users with fresh memory and messages
        self.users = np.concatenate([self.users, [3, 4]])                               # ... and two arbitrary ones
        self.now = float(d.timestamps[self.cursor + 200])
        U = len(self.users)
        side = M.mv_side(9, U, N_ITEMS, 29, n_days=4, n_stocks=N_ITEMS)
        self.returns, self.port_idx, self.port_len = side["returns"], side["port_idx"], side["port_len"]
        self.day_idx = np.random.RandomState(3).randint(0, 4, size=U).astype(np.int32)
        self.mv = types.SimpleNamespace(returns=torch.from_numpy(self.returns).to(DEV), upper_u=N_USERS, gamma=2.0, lambda_mv=0.5,
                                        day_of=lambda ts: (np.asarray(ts, np.float64) // 4096.0).astype(np.int64) % 4)

    def _params(self):
        return {k: self.tgn.state_dict()[k].detach().cpu().numpy().copy() for k in self.names}

    def step(self, grad):
        """One ``compute_temporal_embeddings`` on both sides; returns (model's, oracle's) embeddings."""
        d, s = self.g.data, self.cursor
        self.cursor += BATCH
        sb, db, tb, eb = d.sources[s:s + BATCH], d.destinations[s:s + BATCH], d.timestamps[s:s + BATCH], d.edge_idxs[s:s + BATCH]
        neg = self.rs.randint(N_USERS + 1, N_USERS + N_ITEMS + 1, size=BATCH * 3)
        self.tgn.train()
        with torch.set_grad_enabled(grad):
            got = self.tgn.compute_temporal_embeddings(sb, db, neg, tb, eb, K_NBR)
        want = self.ref.compute_temporal_embeddings(sb, db, neg, tb, eb, K_NBR)
        return torch.cat(list(got)), np.concatenate(want)

    def state(self):
        t = self.tgn
        out = [t.flat_parameters.detach().clone()]
        if t._flat_grad is not None:
            out.append(t._flat_grad.clone())
        if self.use_mem:
            m = t.memory
            out += [x.detach().clone() for x in (m.memory, m.last_update, m.msg_table, m.msg_time, m.has_msg)]
        return out

    def host_flags(self):
        t = self.tgn
        return (t.training, t._step, t._gru_applied_now, t.memory._any_msg if self.use_mem else None,
                t.memory._state_version if self.use_mem else None)

    def check(self, out, k, day_idx, exclude_pos=None, item_ok=None):
        """A result of ``TGN.recommend(mv=..., return_embeddings=True)`` against the reference's ``fuse`` of the fp32 scores the
        kernel itself returns for the embeddings of that call, users in the caller's order and unsorted blocks."""
        ids, scores, n_valid, fused, ue, ie, ub = out
        I = N_ITEMS
        pos_of = {int(v): i for i, v in enumerate(self.items)}
        pos = np.array([[pos_of.get(int(v), -1) for v in row] for row in ids.cpu().numpy()], np.int32)
        c = dict(user_emb=ue.cpu().numpy(), item_emb=ie.cpu().numpy(), user_block=ub.cpu().numpy(), returns=self.returns,
                 cand_stock=(self.items - N_USERS - 1).astype(np.int32), day_idx=np.asarray(day_idx, np.int32), port_idx=self.port_idx,
                 port_len=self.port_len, gamma=2.0, excl_pos=exclude_pos, excl_len=None, item_ok=item_ok)
        n_t = ie.shape[0] // I
        direct = _kernel(c, 0.5, k, n_t)
        ref = M.reference(c, 0.5, k, scores=direct["score"])
        eps = R.dot_error_bound(c["user_emb"], c["item_emb"], c["user_block"], I)
        assert (np.abs(direct["score"].astype(np.float64) - ref["s64"]) <= eps).all()
        assert np.array_equal(pos, ref["top_pos"]) and np.array_equal(n_valid.cpu().numpy(), ref["n_valid"])
        assert np.array_equal(fused.cpu().numpy(), ref["top_fused"])
        assert np.array_equal(scores.cpu().numpy().view(np.int32), ref["top_score"].view(np.int32))
        return ref


_WORLDS = {}


@pytest.fixture(params=[(1, True), (2, False)], ids=["L1_mem", "L2_nomem"])
def world(request):
    if request.param not in _WORLDS:
        _WORLDS[request.param] = _World(*request.param)
    return _WORLDS[request.param]


def test_recommend_with_mv_changes_nothing_and_follows_the_portfolio(world):
    w = world
    ports = (w.port_idx, w.port_len)
    for mode in (True, False):
        w.tgn.train(mode)
        before, flags = w.state(), w.host_flags()
        a = w.tgn.recommend(w.users, w.now, 7, w.items, mv=w.mv, portfolios=ports, day_idx=w.day_idx, return_embeddings=True)
        b = w.tgn.recommend(w.users, w.now, 7, w.items, mv=w.mv, portfolios=ports, day_idx=w.day_idx, return_embeddings=True)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        assert all(torch.equal(x, y) for x, y in zip(before, w.state()))
        assert flags == w.host_flags()
        assert not any(t.requires_grad for t in a)
    ref = w.check(a, 7, w.day_idx)
    assert (ref["n_valid"] == 7).all() and a[3].dtype == torch.float64
    # mv=None is the call it was: three outputs, the plain kernel's on the same embeddings
    plain = w.tgn.recommend(w.users, w.now, 7, w.items, return_embeddings=True)
    assert len(plain) == 6 and len(w.tgn.recommend(w.users, w.now, 7, w.items)) == 3
    assert torch.equal(plain[3], a[4]) and torch.equal(plain[4], a[5])
    pos, score, n = P.recommend_topk(plain[3], plain[4], 7)
    assert torch.equal(plain[1], score) and torch.equal(plain[2], n) and torch.equal(plain[0], torch.from_numpy(w.items).to(DEV)[pos.long()].int())
    assert not torch.equal(plain[0], a[0]), "the portfolios must move something"
    # lists of stock indices, device tensors and a day taken from the timestamps are the same query
    lists = [[int(v) for v in w.port_idx[u, :min(w.port_len[u], 8)]] for u in range(len(w.users))]
    again = w.tgn.recommend(w.users, w.now, 7, w.items, mv=w.mv, portfolios=lists, day_idx=w.day_idx)
    again_t = w.tgn.recommend(w.users, w.now, 7, w.items, mv=w.mv, portfolios=(_dev(w.port_idx), _dev(w.port_len)), day_idx=_dev(w.day_idx))
    assert all(torch.equal(x, y) for x, y in zip(a[:4], again)) and all(torch.equal(x, y) for x, y in zip(a[:4], again_t))
    day = int(w.mv.day_of(np.array([w.now]))[0])
    one_day = w.tgn.recommend(w.users, w.now, 7, w.items, mv=w.mv, portfolios=ports)
    same = w.tgn.recommend(w.users, w.now, 7, w.items, mv=w.mv, portfolios=ports, day_idx=day)
    assert all(torch.equal(x, y) for x, y in zip(one_day, same))


def test_per_user_timestamps_keep_the_callers_order(world):
    w = world
    U = len(w.users)
    grid = np.array([w.now, w.now - 30000.0, w.now + 512.0])
    ts = grid[np.random.RandomState(2).randint(0, 3, size=U)]
    ports = (w.port_idx, w.port_len)
    excl = [[int(w.items[i % 5])] for i in range(U)]
    ok = np.arange(N_ITEMS) % 7 != 0
    before, flags = w.state(), w.host_flags()
    out = w.tgn.recommend(w.users, ts, 5, w.items, exclude=excl, item_ok=ok, mv=w.mv, portfolios=ports, day_idx=w.day_idx,
                          return_embeddings=True)
    assert all(torch.equal(x, y) for x, y in zip(before, w.state())) and flags == w.host_flags()
    ub = out[6].cpu().numpy()
    assert np.array_equal(np.unique(ts)[ub], ts) and len(set(ub.tolist())) == 3 and (np.diff(ub) < 0).any()   # blocks not sorted
    ref = w.check(out, 5, w.day_idx, exclude_pos=np.array([[i % 5] for i in range(U)], np.int32), item_ok=ok.astype(np.uint8))
    ids = out[0].cpu().numpy()
    for u in range(U):
        assert excl[u][0] not in ids[u] and not (set(ids[u].tolist()) & set(w.items[~ok].tolist()))
    # the day from the timestamps: mv.day_of on each user's own time
    by_ts = w.tgn.recommend(w.users, ts, 5, w.items, mv=w.mv, portfolios=ports, return_embeddings=True)
    w.check(by_ts, 5, w.mv.day_of(ts))
    # and one user alone at its time gets what it got in the crowd
    one = w.tgn.recommend(w.users[4:5], ts[4], 5, w.items, exclude=excl[4:5], item_ok=ok, mv=w.mv,
                          portfolios=(w.port_idx[4:5], w.port_len[4:5]), day_idx=int(w.day_idx[4]))
    assert all(torch.equal(one[i][0], out[i][4]) for i in range(4))
    assert ref["n_valid"][4] == 5


def test_training_still_works_after_an_mv_query(world):
    w = world
    w.tgn.train()
    w.tgn.recommend(w.users, w.now, 5, w.items, mv=w.mv, portfolios=(w.port_idx, w.port_len), day_idx=w.day_idx)
    w.ref.P = w._params()
    got, want = w.step(grad=True)
    assert got.requires_grad
    e = relerr(got.detach().cpu().numpy(), want)
    assert e < RTOL_EMB, e
    P.bpr_loss(got, BATCH, 3).backward()
    grads = [p.grad for p in w.tgn.parameters() if p.requires_grad and p.grad is not None]
    assert grads and all(torch.isfinite(g_).all() for g_ in grads) and any(float(g_.abs().max()) > 0 for g_ in grads)
    if w.use_mem:
        assert relerr(w.tgn.memory.memory.cpu().numpy(), w.ref.memory) < RTOL_EMB
        assert np.array_equal(w.tgn.memory.last_update.cpu().numpy(), w.ref.last_update)
    out = w.tgn.recommend(w.users, w.now, 5, w.items, mv=w.mv, portfolios=(w.port_idx, w.port_len), day_idx=w.day_idx,
                          return_embeddings=True)
    w.check(out, 5, w.day_idx)
