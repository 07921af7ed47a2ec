"""GPU tests of the wide form of the portfolio-aware top-k (``pfo_recommend_mv_topk_wide``): bit for bit the bounded kernel
where both apply, the numpy reference of ``recommend_mv_ref`` beyond 2048 candidates (exact arithmetic: everything to the bit;
random embeddings: the score within the fp32 dot-product bound and everything behind the score exact), ``pfo_recommend_topk`` at
lambda = 0, the slabs of a short workspace, the errors, and ``TGN.recommend(mv=...)`` over more than 2048 items end to end."""
import types

import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

import pfotgnrec_amd as P
from pfotgnrec_amd import _lib
from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
import holdings_ref as HR
import recommend_ref as R
import recommend_mv_ref as M

DEV = "cuda:0"
NAMES = ("top_pos", "top_score", "top_fused", "n_valid", "score", "y", "fused")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _args(c, lam, k, n_t):
    return ((_dev(c["user_emb"]), _dev(c["item_emb"]), k, _dev(c["cand_stock"]), _dev(c["returns"]), _dev(c["day_idx"]), _dev(c["port_idx"]),
             _dev(c["port_len"]), c["gamma"], lam, _dev(c["user_block"]), _dev(c.get("excl_pos")), _dev(c.get("excl_len")),
             _dev(c.get("item_ok"))), dict(n_blocks=n_t))


def _wide(c, lam, k, n_t, want_all=True, workspace=None):
    a, kw = _args(c, lam, k, n_t)
    out = P.recommend_mv_topk_wide(*a, workspace=workspace, want_all=want_all, **kw)
    return {n: t.cpu().numpy() for n, t in zip(NAMES, out)}


def _bounded(c, lam, k, n_t):
    a, kw = _args(c, lam, k, n_t)
    return {n: t.cpu().numpy() for n, t in zip(NAMES, P.recommend_mv_topk(*a, want_all=True, **kw))}


def _same_bits(a, b):
    """The same bits but for the payload of a NaN: NaN in the same places, everything else equal as integers."""
    if a.dtype.kind != "f":
        return a.shape == b.shape and np.array_equal(a, b)
    ints = np.int32 if a.dtype == np.float32 else np.int64
    nan = np.isnan(a)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(ints)[~nan], b.view(ints)[~nan])


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


def _assert_same_outputs(a, b, tag):
    for n in NAMES:
        assert _same_bits(a[n], b[n]), (tag, n)


# ---------------------------------------------------------------------------------------------- 1. the bounded kernel, to the bit

@pytest.mark.parametrize("I", [1, 63, 65, 513, 2048])
def test_equals_the_bounded_kernel_bit_for_bit(I):
    """All seven outputs of ``recommend_mv_topk`` and ``recommend_mv_topk_wide`` on the inputs of the bounded kernel's own exact
    test: positions, scores, fused values, counts and the three diagnostic matrices, NaN in the same places."""
    U, n_t, seed = 17, 2, 0
    for n_ret in (2, 29):
        for D in (4, 172):
            for k in (1, 64):
                seed += 1
                c = M.exact_case(100 * I + seed, U, I, D, k, n_t, n_ret)
                for lam in (0.0, 0.5, 1.0, 0.1):
                    _assert_same_outputs(_wide(c, lam, k, n_t), _bounded(c, lam, k, n_t), (I, n_ret, D, k, lam))


def test_equals_the_bounded_kernel_where_nothing_is_exact():
    """Random normal embeddings: no score is exact and few are tied, and the two kernels must still agree to the bit - one
    device function for the score, one for y, exact integer counts behind them."""
    c = R.normal_case(11, 37, 500, 172)
    c.update(M.mv_side(11, 37, 500, 29))
    _assert_same_outputs(_wide(c, 0.5, 10, 1), _bounded(c, 0.5, 10, 1), "normal")


@pytest.mark.parametrize("D", [48, 64, 112, 128])
def test_equals_the_bounded_kernel_at_the_middle_row_widths(D):
    c = M.exact_case(9000 + D, 17, 65, D, 5, 2, 29)
    _assert_same_outputs(_wide(c, 0.5, 5, 2), _bounded(c, 0.5, 5, 2), D)


# ---------------------------------------------------------------------------------------------- 2. beyond the LDS bound

@pytest.mark.parametrize("I", [2049, 2303, 2304, 2305, 4095, 4096, 4097, 8200])
def test_beyond_the_bound_exact_arithmetic_equals_the_reference(I):
    """The exact cases of the bounded kernel's test (integer embeddings: every fp32 score exact, asserted from the fp64 scores;
    return tables of integers / 64) at list lengths LDS cannot hold: everything equal to ``recommend_mv_ref.reference`` to the
    bit, the score matrix equal to ``scores64``.  2049, 4097 and 8200 are the issue's; the kernels cut a list at multiples of 512
    (the chunk of candidates a workgroup scores) and of 256 (the step of the compaction over the candidates, and of the radix
    sort's scatter over the admissible ones): 4095 / 4096 / 4097 lie on both sides of a boundary of both kinds, 2303 / 2304 / 2305
    of one that is a step's alone.  (The sort's steps count ADMISSIBLE candidates, whose number differs from user to user: each
    case meets a dozen different remainders.)  User 0 is short of candidates, users 5 and 16 have none, and at k = 64 at least 12
    of the 17 users get a full row."""
    U, n_t, seed = 17, 2, 0
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
                    got = _wide(c, lam, k, n_t)
                    tag = (I, n_ret, D, k, lam)
                    assert np.array_equal(got["score"].astype(np.float64), s64), tag
                    _assert_equals_reference(got, ref, tag)
                    assert ref["n_valid"][0] < k, "user 0 must be short of candidates"
                    assert (ref["n_valid"][[5, U - 1]] == 0).all() and np.isnan(ref["y"][:, [0, I - 1]]).all()
                    assert k == 1 or (ref["n_valid"] == k).sum() >= 12, "full rows must be the rule"


# ---------------------------------------------------------------------------------------------- 3. mostly distinct y

@pytest.mark.parametrize("lam", [0.5, 1.0])
def test_mostly_distinct_y(lam):
    """The helpers' default of at most 300 stocks makes every rank of y a long tie; with a stock table larger than the list most
    y of a user are distinct, so the y sort and its searches meet runs of length one."""
    c = R.exact_case(77, 5, 4097, 32, 64, 1)
    c.update(M.mv_side(84, 5, 4097, 29, 8, n_stocks=4099))
    ref = M.reference(c, lam, 64)
    for u in (2, 3):
        row = ref["y"][u]
        assert len(np.unique(row[~np.isnan(row)])) > 1500, "most y of users 2 and 3 must be distinct"
    got = _wide(c, lam, 64, 1)
    assert np.array_equal(got["score"].astype(np.float64), ref["s64"])
    _assert_equals_reference(got, ref, lam)


# ---------------------------------------------------------------------------------------------- 4. random normal embeddings

@pytest.mark.parametrize("lam", [0.5, 0.1])
def test_blend_on_random_normal_embeddings_in_two_stages(lam):
    """(a) every score within ``recommend_ref.dot_error_bound`` of the fp64 score; (b) the reference's ``fuse`` applied to the
    kernel's OWN scores reproduces positions, scores, fused values, counts and the y / fused rows exactly.  The score keys are
    distinct and of both signs here."""
    U, I, k = 9, 3000, 10
    c = R.normal_case(41, U, I, 172)
    c.update(M.mv_side(41, U, I, 29))
    got = _wide(c, lam, k, 1)
    ref = M.reference(c, lam, k)
    eps = R.dot_error_bound(c["user_emb"], c["item_emb"], None, I)
    assert (np.abs(got["score"].astype(np.float64) - ref["s64"]) <= eps).all()                      # (a)
    assert (got["score"] < 0).any() and (got["score"] > 0).any()
    assert all(len(np.unique(row)) > 0.99 * I for row in got["score"]), "the score keys must be distinct but for a chance pair"
    _assert_equals_reference(got, M.reference(c, lam, k, scores=got["score"], y=ref["y_raw"]), lam)  # (b)


# ---------------------------------------------------------------------------------------------- 5. lambda = 0

def test_lambda_zero_is_the_plain_kernel():
    c = R.normal_case(31, 21, 5000, 32, 3)
    c.update(M.mv_side(31, 21, 5000, 29, clean=True))
    assert not np.isnan(M.y_matrix(c["returns"], c["day_idx"], c["cand_stock"], c["port_idx"], c["port_len"])).any()
    got = _wide(c, 0.0, 10, 3)
    pos, score, n = (t.cpu().numpy() for t in P.recommend_topk(_dev(c["user_emb"]), _dev(c["item_emb"]), 10, _dev(c["user_block"]),
                                                               _dev(c["excl_pos"]), _dev(c["excl_len"]), _dev(c["item_ok"]), n_blocks=3))
    assert np.array_equal(got["top_pos"], pos) and np.array_equal(got["n_valid"], n)
    assert np.array_equal(got["top_score"].view(np.int32), score.view(np.int32))


# ---------------------------------------------------------------------------------------------- 6. the bound

def test_the_bound_of_65536_candidates():
    I, k = 65536, 64
    c = M.exact_case(6553601, 3, I, 32, k, 1, 29)
    ref = M.reference(c, 0.5, k)
    assert ref["n_valid"].tolist() == [53, 64, 64]
    got = _wide(c, 0.5, k, 1)
    assert np.array_equal(got["score"].astype(np.float64), ref["s64"])
    _assert_equals_reference(got, ref, I)


# ---------------------------------------------------------------------------------------------- 7. slabs

def test_the_result_does_not_depend_on_the_slab_size():
    """40 users are three tiles: the minimum workspace serves them in three slabs of one tile, two tiles' worth in two slabs of
    which the second is short, three tiles' worth in one.  Each workspace is the head of a larger tensor whose last 4 KB must
    keep their pattern."""
    U, I, k = 40, 2100, 10
    c = M.exact_case(4021, U, I, 32, k, 2, 29)
    ref = M.reference(c, 0.5, k)
    size = lambda users: _lib.byte_count("pfo_recommend_mv_wide_workspace_bytes", users, I)
    assert size(1) == size(16) < size(32) < size(40) == size(48)
    outs = []
    for users in (16, 32, 40):
        whole = torch.empty(size(users) + 4096, dtype=torch.uint8, device=DEV)
        pattern = (torch.arange(4096, device=DEV) % 251).to(torch.uint8)
        whole[size(users):] = pattern
        outs.append(_wide(c, 0.5, k, 2, workspace=whole[:size(users)]))
        assert torch.equal(whole[size(users):], pattern), "%d users' worth: written beyond the workspace" % users
        _assert_equals_reference(outs[-1], ref, users)
        _assert_same_outputs(outs[-1], outs[0], users)
    assert np.array_equal(outs[0]["score"].astype(np.float64), ref["s64"])


# ---------------------------------------------------------------------------------------------- 8. errors

def test_errors_of_the_entry():
    c = M.exact_case(5, 19, 70, 32, 5, 1, 29)
    ue, ie = _dev(c["user_emb"]), _dev(c["item_emb"])
    cand, ret, day = _dev(c["cand_stock"]), _dev(c["returns"]), _dev(c["day_idx"])
    out = torch.empty(19 * 5 * 8, dtype=torch.int32, device=DEV)
    need = _lib.byte_count("pfo_recommend_mv_wide_workspace_bytes", 16, 70)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def args(I=70, k=5, n_ret=29, wsp=ws.data_ptr(), wsb=need, U=19):
        return ("pfo_recommend_mv_topk_wide", ue.data_ptr(), ie.data_ptr(), None, U, I, 1, 32, None, None, 0, None, cand.data_ptr(),
                ret.data_ptr(), 3, 72, n_ret, day.data_ptr(), None, None, 0, 2.0, 0.5, k, out.data_ptr(), out.data_ptr(), out.data_ptr(),
                None, None, None, None, wsp, wsb, _lib.stream_ptr())
    for bad, msg in ((args(I=65537), "I must be"), (args(k=65), "k must be"), (args(n_ret=1), "n_ret must be"),
                     (args(wsp=None), "workspace"), (args(wsb=need - 1), "workspace")):
        with pytest.raises(_lib.PfoError, match=msg):
            _lib.call(*bad)
    _lib.call(*args())                                                # (the arguments above are good ones)
    _lib.call("pfo_recommend_mv_topk_wide", None, None, None, 0, 70, 1, 32, None, None, 0, None, None, None, 3, 72, 29, None, None, None, 0,
              2.0, 0.5, 5, None, None, None, None, None, None, None, None, 0, _lib.stream_ptr())
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 9. want_all and the dispatcher op

def test_want_all_false_and_the_dispatcher_op():
    I, k = 2100, 5
    c = M.exact_case(77, 19, I, 32, k, 1, 29)
    got = _wide(c, 0.5, k, 1)
    _assert_equals_reference(got, M.reference(c, 0.5, k), "want_all")
    short = _wide(c, 0.5, k, 1, want_all=False)
    assert len(short) == 4 and all(_same_bits(short[n], got[n]) for n in short)
    op = torch.ops.pfotgn.recommend_mv_topk_wide(_dev(c["user_emb"]), _dev(c["item_emb"]), k, _dev(c["cand_stock"]), _dev(c["returns"]),
                                                 _dev(c["day_idx"]), 2.0, 0.5, 1, _dev(c["port_idx"]), _dev(c["port_len"]),
                                                 _dev(c["user_block"]), _dev(c["excl_pos"]), _dev(c["excl_len"]), _dev(c["item_ok"]))
    assert len(op) == 4
    for t, name in zip(op, NAMES):
        assert _same_bits(t.cpu().numpy(), got[name]), name


# ---------------------------------------------------------------------------------------------- 10. TGN.recommend end to end

N_USERS, N_ITEMS, K_NBR, BATCH, WIDTH = 200, 2100, 10, 40, 8
DIV = float(1 << 18)          # synthetic.day_of is floor(ts * 64 / 2^24): the key rule with this divisor


class _World:
    """A synthetic graph with more items than the bounded kernel takes, and the model advanced by a few training-path calls so
    that memory and pending messages are populated; return tables of N_ITEMS stocks over four days next to it."""

    def __init__(self, L, use_mem):
        torch.manual_seed(77 + L)
        self.L, self.use_mem = L, use_mem
        self.g = g = make_graph(SyntheticConfig("t", N_USERS, N_ITEMS, 10_000, 32, L, K_NBR, 2), with_prices=True)
        d = g.data
        self.tgn = P.TGN(P.get_neighbor_finder(d, uniform=False), g.node_features, g.edge_features, DEV, n_layers=L, n_heads=2,
                         dropout=0.0, use_memory=use_mem, memory_dimension=32, message_function="identity", n_neighbors=K_NBR)
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

    def step(self, grad):
        d, s = self.g.data, self.cursor
        self.cursor += BATCH
        sb, db, tb, eb = d.sources[s:s + BATCH], d.destinations[s:s + BATCH], d.timestamps[s:s + BATCH], d.edge_idxs[s:s + BATCH]
        neg = self.rs.randint(N_USERS + 1, N_USERS + N_ITEMS + 1, size=BATCH * 3)
        self.tgn.train()
        with torch.set_grad_enabled(grad):
            return torch.cat(list(self.tgn.compute_temporal_embeddings(sb, db, neg, tb, eb, K_NBR)))

    def state(self):
        t = self.tgn
        out = [t.flat_parameters.detach().clone()]
        if t._flat_grad is not None:
            out.append(t._flat_grad.clone())
        if self.use_mem:
            m = t.memory
            out += [x.detach().clone() for x in (m.memory, m.last_update, m.msg_table, m.msg_time, m.has_msg)]
        nf = t.neighbor_finder
        out += [x.clone() for x in vars(nf).values() if isinstance(x, torch.Tensor)]
        return out

    def host_flags(self):
        t = self.tgn
        return (t.training, t._step, t._gru_applied_now, t.memory._any_msg if self.use_mem else None,
                t.memory._state_version if self.use_mem else None)

    def check(self, out, k, day_idx, items=None, port=None, exclude_pos=None, item_ok=None):
        """A result of ``TGN.recommend(mv=..., return_embeddings=True)`` against the reference's ``fuse`` of the fp32 scores the
        wide kernel itself returns (``want_all``) for the embeddings of that call."""
        ids, scores, n_valid, fused, ue, ie, ub = out
        items = self.items if items is None else items
        port_idx, port_len = (self.port_idx, self.port_len) if port is None else port
        I = len(items)
        pos_of = {int(v): i for i, v in enumerate(items)}
        pos = np.array([[pos_of.get(int(v), -1) for v in row] for row in ids.cpu().numpy()], np.int32)
        c = dict(user_emb=ue.cpu().numpy(), item_emb=ie.cpu().numpy(), user_block=ub.cpu().numpy(), returns=self.returns,
                 cand_stock=(items - N_USERS - 1).astype(np.int32), day_idx=np.asarray(day_idx, np.int32), port_idx=port_idx,
                 port_len=port_len, gamma=2.0, excl_pos=exclude_pos, excl_len=None, item_ok=item_ok)
        n_t = ie.shape[0] // I
        direct = _wide(c, 0.5, k, n_t)
        ref = M.reference(c, 0.5, k, scores=direct["score"])
        eps = R.dot_error_bound(c["user_emb"], c["item_emb"], c["user_block"], I)
        assert (np.abs(direct["score"].astype(np.float64) - ref["s64"]) <= eps).all()
        assert np.array_equal(pos, ref["top_pos"]) and np.array_equal(n_valid.cpu().numpy(), ref["n_valid"])
        assert np.array_equal(fused.cpu().numpy(), ref["top_fused"])
        assert np.array_equal(scores.cpu().numpy().view(np.int32), ref["top_score"].view(np.int32))
        return c, ref


def test_tgn_recommend_over_65536_items():
    """The longest list ``TGN.recommend`` takes, with ``mv``: the list is what ``scipy.stats.rankdata`` and the canonical order
    (``recommend_mv_ref.fuse``) make of the scores and y of the returned embeddings.  The y matrix of the reference costs a
    ``np.cov`` per (user, stock): it is checked to the bit on 400 stocks per user, and the kernel's own y row, once held to
    that, feeds the ranks of all 65536."""
    n_users, I, k = 20, 65536, 10
    torch.manual_seed(3)
    g = make_graph(SyntheticConfig("t", n_users, I, 4000, 16, 1, 5, 2), with_prices=False)
    tgn = P.TGN(P.get_neighbor_finder(g.data, uniform=False), g.node_features, g.edge_features, DEV, n_layers=1, n_heads=2, dropout=0.0,
                use_memory=True, memory_dimension=16, message_function="identity", n_neighbors=5)
    tgn.eval()
    users, items = np.array([1, 2, 7]), np.arange(n_users + 1, n_users + I + 1)
    side = M.mv_side(9, 3, I, 29, n_days=2, n_stocks=I, clean=True)
    mv = types.SimpleNamespace(returns=torch.from_numpy(side["returns"]).to(DEV), upper_u=n_users, gamma=2.0, lambda_mv=0.5, day_of=None)
    now = float(g.data.timestamps[-1]) + 1.0
    excl = [[int(items[5]), int(items[I - 1])], [], [int(items[0])]]
    out = tgn.recommend(users, now, k, items, exclude=excl, mv=mv, portfolios=(side["port_idx"], side["port_len"]), day_idx=side["day_idx"],
                        return_embeddings=True)
    ids, scores, n_valid, fused, ue, ie, ub = out
    c = dict(user_emb=ue.cpu().numpy(), item_emb=ie.cpu().numpy(), user_block=ub.cpu().numpy(), returns=side["returns"],
             cand_stock=np.arange(I, dtype=np.int32), day_idx=side["day_idx"], port_idx=side["port_idx"], port_len=side["port_len"],
             gamma=2.0, excl_pos=np.array([[5, I - 1], [-1, -1], [0, -1]], np.int32), excl_len=np.array([2, 0, 1], np.int32), item_ok=None)
    direct = _wide(c, 0.5, k, 1)
    rs = np.random.RandomState(1)
    for u in range(3):
        some = np.sort(rs.choice(np.arange(6, I - 1), size=400, replace=False))
        want = M.y_mv(side["returns"], int(side["day_idx"][u]), some, M.portfolio(side["port_idx"], side["port_len"], u, I))
        assert np.array_equal(direct["y"][u, some], want) and not np.isnan(want).any(), u
    # outside A(u): the excluded positions, and candidate 0 for everybody - stock 0 never moves, its y is 0 / 0
    assert np.isnan(direct["y"][0, [5, I - 1]]).all() and np.isnan(direct["y"][:, 0]).all() and np.isnan(direct["y"]).sum() == 5
    ref = M.reference(c, 0.5, k, scores=direct["score"], y=direct["y"])      # (NaN where excluded: the reference excludes those itself)
    eps = R.dot_error_bound(c["user_emb"], c["item_emb"], c["user_block"], I)
    assert (np.abs(direct["score"].astype(np.float64) - ref["s64"]) <= eps).all()
    _assert_equals_reference(direct, ref, "direct")
    assert np.array_equal(ids.cpu().numpy(), items[ref["top_pos"]]) and (ref["n_valid"] == k).all()
    assert np.array_equal(n_valid.cpu().numpy(), ref["n_valid"]) and np.array_equal(fused.cpu().numpy(), ref["top_fused"])
    assert np.array_equal(scores.cpu().numpy().view(np.int32), ref["top_score"].view(np.int32))


@pytest.mark.parametrize("L,use_mem", [(1, True), (2, True)], ids=["L1_mem", "L2_mem"])
def test_tgn_recommend_over_more_than_2048_items(L, use_mem):
    w = _World(L, use_mem)
    U, k = len(w.users), 10
    ports = (w.port_idx, w.port_len)
    # ---- the query changes nothing and equals the reference on its own embeddings
    w.tgn.eval()
    before, flags = w.state(), w.host_flags()
    a = w.tgn.recommend(w.users, w.now, k, w.items, mv=w.mv, portfolios=ports, day_idx=w.day_idx, return_embeddings=True)
    assert all(torch.equal(x, y) for x, y in zip(before, w.state())) and flags == w.host_flags()
    assert not any(t.requires_grad for t in a) and a[3].dtype == torch.float64
    _, ref = w.check(a, k, w.day_idx)
    assert (ref["n_valid"] == k).all()
    plain = w.tgn.recommend(w.users, w.now, k, w.items)
    assert not torch.equal(plain[0], a[0]), "the portfolios must move something"
    # ---- per-user timestamps (device tensors need a ledger for the day: host ones here), exclusions and item_ok: the caller's order
    grid = np.array([w.now, w.now - 30000.0, w.now + 512.0])
    ts = grid[np.random.RandomState(2).randint(0, 3, size=U)]
    excl = [[int(w.items[i % 5])] for i in range(U)]
    ok = np.arange(N_ITEMS) % 7 != 0
    out = w.tgn.recommend(w.users, ts, 5, w.items, exclude=excl, item_ok=ok, mv=w.mv, portfolios=ports, day_idx=w.day_idx,
                          return_embeddings=True)
    ub = out[6].cpu().numpy()
    assert np.array_equal(np.unique(ts)[ub], ts) and len(set(ub.tolist())) == 3 and (np.diff(ub) < 0).any()   # blocks not sorted
    w.check(out, 5, w.day_idx, exclude_pos=np.array([[i % 5] for i in range(U)], np.int32), item_ok=ok.astype(np.uint8))
    ids = out[0].cpu().numpy()
    for u in range(U):
        assert excl[u][0] not in ids[u] and not (set(ids[u].tolist()) & set(w.items[~ok].tolist()))
    dev_ts = w.tgn.recommend(w.users, _dev(ts), 5, w.items, exclude=excl, item_ok=ok, mv=w.mv, portfolios=ports, day_idx=w.day_idx)
    assert all(torch.equal(x, y) for x, y in zip(dev_ts, out[:4])), "per-user device timestamps keep the caller's order"
    # ---- the ledger's rows in place of the packed form
    w.tgn.track_holdings(WIDTH, N_USERS)
    kept = [M.portfolio(w.port_idx, w.port_len, u, N_ITEMS) for u in range(U)]      # (a ledger row holds stocks of the table only)
    led_idx, led_len = np.full((U, WIDTH), -1, np.int32), np.array([len(r) for r in kept], np.int32)
    for u, r in enumerate(kept):
        led_idx[u, :len(r)] = r
    w.tgn.update_holdings(w.users, (led_idx, led_len), np.full(U, w.now - 1.0))
    h_idx, h_len = (t.cpu().numpy() for t in (w.tgn.holdings.idx, w.tgn.holdings.len))
    rows = (h_idx[w.users], h_len[w.users])
    lists = HR.held_node_lists(h_idx, h_len, w.users, N_USERS)
    assert sum(len(r) for r in lists) > 10
    held = w.tgn.recommend(w.users, ts, k, w.items, mv=w.mv, day_idx=w.day_idx, exclude="held", portfolios="held")
    packed = w.tgn.recommend(w.users, ts, k, w.items, mv=w.mv, day_idx=w.day_idx, exclude=lists, portfolios=rows)
    assert len(held) == 4 and all(torch.equal(x, y) for x, y in zip(held, packed))
    ids = held[0].cpu().numpy()
    assert all(not (set(ids[q].tolist()) & set(lists[q])) for q in range(U))
    # ---- the first 2048 items take the old route: what the bounded kernel returns on the returned embeddings
    head = w.items[:2048]
    old = w.tgn.recommend(w.users, w.now, k, head, mv=w.mv, portfolios=ports, day_idx=w.day_idx, return_embeddings=True)
    pos, score, fused, n = P.recommend_mv_topk(old[4], old[5], k, _dev((head - N_USERS - 1).astype(np.int32)), w.mv.returns, _dev(w.day_idx),
                                               _dev(w.port_idx), _dev(w.port_len), 2.0, 0.5)
    assert torch.equal(old[0], _dev(head.astype(np.int32))[pos.long()]) and torch.equal(old[1], score)
    assert torch.equal(old[2], n) and torch.equal(old[3], fused) and bool((n == k).all())
    # ---- a price ledger as mv: the day looked up on the device, the same answer as the sampler's from host timestamps
    g = w.g
    led = P.PriceLedger.from_prices(np.arange(g.prices.shape[0]), g.prices, g.upper_u, DEV, key_divisor=DIV)
    sampler = P.MVSampler(g.prices, g.upper_u, DEV, day_of=g.day_of)
    want = w.tgn.recommend(w.users, ts, k, w.items, mv=sampler, portfolios=ports)
    got = w.tgn.recommend(w.users, _dev(ts), k, w.items, mv=led, portfolios=ports)
    assert len(got) == 4 and all(torch.equal(x, y) for x, y in zip(got, want)) and bool((got[2] == k).all())
    # ---- and a training step still runs
    emb = w.step(grad=True)
    assert emb.requires_grad
    P.bpr_loss(emb, BATCH, 3).backward()
    grads = [p.grad for p in w.tgn.parameters() if p.requires_grad and p.grad is not None]
    assert grads and all(torch.isfinite(g_).all() for g_ in grads) and any(float(g_.abs().max()) > 0 for g_ in grads)
