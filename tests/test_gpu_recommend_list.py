"""GPU tests of the list forms of the top-k recommendation: ``pfo_recommend_list_topk`` / ``pfo_recommend_list_mv_topk`` against
the numpy reference of ``recommend_list_ref`` and against the shared-list kernels fed the complement of each list (bit for bit
on exact arithmetic), on random normal embeddings within the any-order fp32 dot-product bound with everything behind the score
exact, the two forms against each other at lambda = 0, and ``TGN.recommend(only=...)`` end to end on the small served world of
tests/test_gpu_holdings.py."""
import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

import pfotgnrec_amd as P
from pfotgnrec_amd import _lib
from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
import recommend_ref as R
import recommend_mv_ref as M
import recommend_list_ref as L
from recommend_list_ref import NORMAL_CASES, normal_list_case

DEV = "cuda:0"
CANARY = 64          # elements of 0x5a bytes before and behind every output


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _Out:
    """An output array between two canaries."""

    def __init__(self, shape, dtype):
        n = int(np.prod(shape))
        self.buf = torch.empty(n + 2 * CANARY, dtype=dtype, device=DEV)
        self.buf.view(torch.uint8).fill_(0x5a)
        self.fresh = self.buf.clone()
        self.t = self.buf[CANARY:CANARY + n].view(shape)

    def ptr(self):
        return self.t.data_ptr()

    def take(self):
        assert torch.equal(self.buf[:CANARY].view(torch.uint8), self.fresh[:CANARY].view(torch.uint8)), "canary in front"
        assert torch.equal(self.buf[-CANARY:].view(torch.uint8), self.fresh[-CANARY:].view(torch.uint8)), "canary behind"
        return self.t.cpu().numpy()


def _call(c, k, n_t, lam=None):
    """One call of the C entry (``lam`` None: the score form) with every output between canaries and every diagnostic array
    asked for; the inputs must hold their bits afterwards.  Returns the outputs by name."""
    U, D = c["user_emb"].shape
    I, W = c["I"], c["list_pos"].shape[1]
    names = ["user_emb", "item_emb", "user_block", "list_pos", "list_len", "item_ok"]
    if lam is not None:
        names += ["cand_stock", "returns", "day_idx", "port_idx", "port_len"]
    d = {n: _dev(c.get(n)) for n in names}
    before = {n: t.clone() for n, t in d.items() if t is not None}
    p = lambda n: _lib.ptr(d[n])
    out = dict(top_pos=_Out((U, k), torch.int32), top_score=_Out((U, k), torch.float32), n_valid=_Out((U,), torch.int32),
               score=_Out((U, W), torch.float32))
    if lam is None:
        _lib.call("pfo_recommend_list_topk", p("user_emb"), p("item_emb"), p("user_block"), U, I, n_t, D, p("list_pos"), p("list_len"), W,
                  p("item_ok"), k, out["top_pos"].ptr(), out["top_score"].ptr(), out["n_valid"].ptr(), out["score"].ptr(), _lib.stream_ptr())
    else:
        out.update(top_fused=_Out((U, k), torch.float64), y=_Out((U, W), torch.float64), fused=_Out((U, W), torch.float64))
        n_days, n_stocks, n_ret = c["returns"].shape
        Wp = c["port_idx"].shape[1] if c["port_idx"] is not None else 0
        _lib.call("pfo_recommend_list_mv_topk", p("user_emb"), p("item_emb"), p("user_block"), U, I, n_t, D, p("list_pos"), p("list_len"), W,
                  p("item_ok"), p("cand_stock"), p("returns"), n_days, n_stocks, n_ret, p("day_idx"), p("port_idx"), p("port_len"), Wp,
                  float(c["gamma"]), float(lam), k, out["top_pos"].ptr(), out["top_score"].ptr(), out["top_fused"].ptr(), out["n_valid"].ptr(),
                  out["score"].ptr(), out["y"].ptr(), out["fused"].ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert all(torch.equal(d[n], t) for n, t in before.items()), "an input changed"
    return {n: o.take() for n, o in out.items()}


def _same(a, b):
    """The same bits but for which NaN it is: NaN in the same places, every other value bit for bit."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind != "f":
        return a.dtype == b.dtype and np.array_equal(a, b)
    nan = np.isnan(a)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes()


def _edge_rows(c, k):
    """The rows the issue names, written over the first users of a list case (in place): an empty list, a negative length, a
    length beyond the stride, a row of -1 only, a row naming masked items only; the all-zero user gets a list with ties."""
    U, W = c["list_pos"].shape
    I, lp, ll = c["I"], c["list_pos"], c["list_len"]
    if U == 1:
        lp[0, 0], ll[0], c["item_ok"][0] = 0, 1, 1                   # (one user, one entry: something to rank)
    if U <= 10:
        return
    ll[0] = 0
    ll[1] = -3
    lp[2], ll[2] = np.arange(W) % I, W + 5
    lp[3], ll[3] = -1, W
    if I >= 2:
        c["item_ok"][0], c["item_ok"][1:3] = 0, 1                     # (position 2 stays listed for user 2: it has no stock row)
        lp[4], ll[4] = 0, W
    z = U // 2                                                       # (exact_case: the all-zero user row - every score ties)
    assert not c["user_emb"][z].any()
    lp[z], ll[z] = (np.arange(W) * 7 + 1) % I, W


# ---------------------------------------------------------------------------------------------- exact arithmetic
# (U, I, D, k, W, n_t): a covering subset of U {1, 5, 67} x I {1, 17, 300} x D {4, 32, 172, 256} x k {1, 10, 64} x
# list_stride {1, 8, 64, 65, 256} x n_t {1, 3}
EXACT = [(1, 1, 4, 1, 1, 1), (5, 17, 32, 10, 8, 3), (67, 300, 172, 64, 256, 1), (67, 17, 256, 10, 65, 3), (5, 300, 172, 1, 64, 1),
         (67, 17, 4, 64, 256, 3), (5, 1, 32, 10, 64, 1), (67, 300, 32, 10, 8, 3)]


def _exact_case(U, I, D, k, W, n_t):
    c = L.list_case(M.exact_case(1000 * W + I + D, U, I, D, k, n_t, 5), 1000 * W + I, W)
    _edge_rows(c, k)
    s64 = R.scores64(c["user_emb"], c["item_emb"], c["user_block"], I)
    assert np.array_equal(s64.astype(np.float32).astype(np.float64), s64) and np.abs(s64).max() < 2 ** 24, "every score is exact"
    return c


@pytest.mark.parametrize("U,I,D,k,W,n_t", EXACT)
def test_exact_arithmetic_score_form(U, I, D, k, W, n_t):
    """Integer embeddings: every output is the reference's bit for bit, and ``pfo_recommend_topk``'s with the complement of each
    list as the exclusion list; canaries and inputs keep their bits (``_call``); the scores by slot, NaN included."""
    c = _exact_case(U, I, D, k, W, n_t)
    ref, got = L.reference(c, k), _call(c, k, n_t)
    for name in ("top_pos", "top_score", "n_valid", "score"):
        assert _same(got[name], ref[name]), name
    excl_pos, excl_len = L.complement(U, I, c["list_pos"], c["list_len"])
    old = P.recommend_topk(_dev(c["user_emb"]), _dev(c["item_emb"]), k, _dev(c["user_block"]), _dev(excl_pos), _dev(excl_len), _dev(c["item_ok"]),
                           n_blocks=n_t)
    for name, t in zip(("top_pos", "top_score", "n_valid"), old):
        assert _same(got[name], t.cpu().numpy()), "pfo_recommend_topk's " + name
    if U > 10:
        assert (ref["n_valid"][[0, 1, 3]] == 0).all() and (ref["n_valid"][4] == 0 or I < 2) and ref["n_valid"][2] == min(k, ref["adm"][2].sum())
        assert (ref["n_valid"] < k).any() or k == 1
        z = U // 2
        tied = ref["top_pos"][z, :ref["n_valid"][z]]
        assert len(tied) >= 2 and (np.diff(tied) < 0).all() and not ref["top_score"][z, :len(tied)].any(), "ties: larger position first"
    else:
        assert ref["n_valid"].any(), "somebody must be offered something"


@pytest.mark.parametrize("U,I,D,k,W,n_t", EXACT)
def test_exact_arithmetic_mean_variance_form(U, I, D, k, W, n_t):
    """The same with exact return tables (``recommend_mv_ref``): positions, scores, fused, counts and the three diagnostic
    arrays by slot are the reference's and ``pfo_recommend_mv_topk``'s (complement as the exclusion list) to the bit."""
    c = _exact_case(U, I, D, k, W, n_t)
    excl_pos, excl_len = L.complement(U, I, c["list_pos"], c["list_len"])
    y = None
    for lam in (0.5, 1.0, 0.0):
        ref = L.reference_mv(c, lam, k, y=y)
        y = ref["y_raw"]
        got = _call(c, k, n_t, lam)
        for name, want in (("top_pos", "top_pos"), ("top_score", "top_score"), ("top_fused", "top_fused"), ("n_valid", "n_valid"),
                           ("score", "score_slot"), ("y", "y_slot"), ("fused", "fused_slot")):
            assert _same(got[name], ref[want]), (name, lam)
        old = P.recommend_mv_topk(_dev(c["user_emb"]), _dev(c["item_emb"]), k, _dev(c["cand_stock"]), _dev(c["returns"]), _dev(c["day_idx"]),
                                  _dev(c["port_idx"]), _dev(c["port_len"]), c["gamma"], lam, _dev(c["user_block"]), _dev(excl_pos),
                                  _dev(excl_len), _dev(c["item_ok"]), n_blocks=n_t, want_all=True)
        old = [t.cpu().numpy() for t in old]
        for name, t in zip(("top_pos", "top_score", "top_fused", "n_valid"), old):
            assert _same(got[name], t), ("pfo_recommend_mv_topk's " + name, lam)
        for name, t in zip(("score", "y", "fused"), old[4:]):
            assert _same(got[name], L.by_slot(c, ref["adm"], t, t.dtype.type)), ("pfo_recommend_mv_topk's " + name + " by slot", lam)
    if I >= 17 and U > 10:
        assert (ref["adm"].sum(1) < L.admissible_list(U, I, c["list_pos"], c["list_len"], c["item_ok"]).sum(1)).any(), "a listed candidate without a y"


# ---------------------------------------------------------------------------------------------- random normal embeddings

@pytest.mark.parametrize("seed,U,I,D,W,k,n_t", NORMAL_CASES)
def test_normal_embeddings_score_form(seed, U, I, D, W, k, n_t):
    """``recommend_ref.check_topk`` with the list's admissible set: every score within the any-order fp32 bound, rows in the
    canonical order, nothing left out that is clearly better; users whose cut is clear (at least nine in ten:
    tests/test_recommend_list_cpu.py has the shares from the inputs alone) hold the reference's ids."""
    c = normal_list_case(seed, U, I, D, W, n_t)
    got = _call(c, k, n_t)
    s64 = R.scores64(c["user_emb"], c["item_emb"], c["user_block"], I)
    eps = R.dot_error_bound(c["user_emb"], c["item_emb"], c["user_block"], I)
    adm = L.admissible_list(U, I, c["list_pos"], c["list_len"], c["item_ok"])
    share = R.check_topk(got["top_pos"], got["top_score"], got["n_valid"], s64, eps, adm, k)
    first = L.first_slots(c, adm)
    err = np.abs(got["score"].astype(np.float64) - L.by_slot(c, adm, s64, np.float64))[first]
    print("FIGURES recommend_list_topk %s: decided share %.3f, largest |score error| / eps %.3f"
          % ((seed, U, I, D, W, k, n_t), share, (err / L.by_slot(c, adm, eps, np.float64)[first]).max() if first.any() else 0.0))
    assert share >= 0.9
    assert np.array_equal(np.isnan(got["score"]), ~first) and (err <= L.by_slot(c, adm, eps, np.float64)[first]).all()


def _score_matrix(c, got, name="score"):
    """The kernel's own scores (or another diagnostic array) by position, [U, I]: NaN where the list names nothing admissible."""
    s = np.full((c["user_emb"].shape[0], c["I"]), np.nan, got[name].dtype)
    u, slot = np.nonzero(~np.isnan(got[name]))
    s[u, c["list_pos"][u, slot]] = got[name][u, slot]
    return s


@pytest.mark.parametrize("seed,U,I,D,W,k,n_t", NORMAL_CASES)
def test_normal_embeddings_mean_variance_form(seed, U, I, D, W, k, n_t):
    """The checks of tests/test_gpu_recommend_mv.py over the list's set: (a) every score within the fp32 bound and y the
    reference's to the bit; (b) the reference's ``fuse`` over the kernel's OWN scores gives positions, fused values, counts and
    the fused row exactly - everything behind the score is exact; (c) users none of whose admissible scores are closer than
    the sum of their bounds (``separated_share``) are in the reference's order from the fp64 scores, with its fused values."""
    lam = 0.5
    c = normal_list_case(seed, U, I, D, W, n_t)
    c.update(M.mv_side(seed, U, I, 5))
    ref = L.reference_mv(c, lam, k)
    got = _call(c, k, n_t, lam)
    eps = R.dot_error_bound(c["user_emb"], c["item_emb"], c["user_block"], I)
    first = L.first_slots(c, ref["adm"])
    assert np.array_equal(np.isnan(got["score"]), ~first)
    err = np.abs(got["score"].astype(np.float64) - L.by_slot(c, ref["adm"], ref["s64"], np.float64))[first]
    assert (err <= L.by_slot(c, ref["adm"], eps, np.float64)[first]).all()                            # (a)
    assert _same(got["y"], ref["y_slot"])
    own = L.reference_mv(c, lam, k, scores=_score_matrix(c, got), y=ref["y_raw"])                     # (b)
    for name, want in (("top_pos", "top_pos"), ("top_score", "top_score"), ("top_fused", "top_fused"), ("n_valid", "n_valid"),
                       ("fused", "fused_slot")):
        assert _same(got[name], own[want]), name
    sep = np.array([M.separated_share(ref["s64"][u:u + 1], eps[u:u + 1], ref["adm"][u:u + 1]) == 1.0 for u in range(U)])   # (c)
    print("FIGURES recommend_list_mv_topk %s: separated share %.3f, admissible per user %.1f" % ((seed, U, I, D, W, k, n_t), sep.mean(),
                                                                                                  ref["adm"].sum(1).mean()))
    assert np.array_equal(got["top_pos"][sep], ref["top_pos"][sep]) and np.array_equal(got["top_fused"][sep], ref["top_fused"][sep])
    assert sep.any()


@pytest.mark.parametrize("seed,U,I,D,W,k,n_t", NORMAL_CASES[:2])
def test_lambda_zero_is_the_score_form(seed, U, I, D, W, k, n_t):
    """fused = the average-tie rank of the score, whose canonical order is the score's: with a y for every listed candidate the
    mean-variance form returns the score form's positions, scores and counts to the bit (one scoring sequence for both)."""
    c = normal_list_case(seed, U, I, D, W, n_t)
    c.update(M.mv_side(seed, U, I, 5, clean=True))
    assert not np.isnan(M.y_matrix(c["returns"], c["day_idx"], c["cand_stock"], c["port_idx"], c["port_len"])).any()
    plain, mv = _call(c, k, n_t), _call(c, k, n_t, 0.0)
    for name in ("top_pos", "top_score", "n_valid", "score"):
        assert _same(plain[name], mv[name]), name
    assert (plain["n_valid"] > 0).any()


def test_functional_forms_defaults_and_the_dispatcher_ops():
    U, I, D, k, W, n_t = 19, 70, 32, 5, 8, 1
    c = L.list_case(M.exact_case(5, U, I, D, k, n_t, 5), 5, W)
    whole = dict(c, list_len=None, item_ok=None, port_len=None)             # no lengths: whole rows; nothing masked
    ref, ref_mv = L.reference(whole, k), L.reference_mv(whole, 0.5, k)
    ue, ie, lp = _dev(c["user_emb"]), _dev(c["item_emb"]), _dev(c["list_pos"])
    mv_args = (_dev(c["cand_stock"]), _dev(c["returns"]), _dev(c["day_idx"]))
    got = P.recommend_list_topk(ue, ie, k, lp, None)
    assert len(got) == 3 and all(_same(t.cpu().numpy(), ref[n]) for t, n in zip(got, ("top_pos", "top_score", "n_valid")))
    got = P.recommend_list_topk(ue, ie, k, lp, None, want_all=True)
    assert len(got) == 4 and _same(got[3].cpu().numpy(), ref["score"])
    got = torch.ops.pfotgn.recommend_list_topk(ue, ie, k, lp)
    assert all(_same(t.cpu().numpy(), ref[n]) for t, n in zip(got, ("top_pos", "top_score", "n_valid")))
    got = P.recommend_list_mv_topk(ue, ie, k, lp, None, *mv_args, _dev(c["port_idx"]), None, 2.0, 0.5, want_all=True)
    names = ("top_pos", "top_score", "top_fused", "n_valid", "score_slot", "y_slot", "fused_slot")
    assert len(got) == 7 and all(_same(t.cpu().numpy(), ref_mv[n]) for t, n in zip(got, names))
    got = torch.ops.pfotgn.recommend_list_mv_topk(ue, ie, k, lp, *mv_args, 2.0, 0.5, None, 1, _dev(c["port_idx"]))
    assert len(got) == 4 and all(_same(t.cpu().numpy(), ref_mv[n]) for t, n in zip(got, names))
    with pytest.raises(ValueError):
        P.recommend_list_topk(ue, ie, k, torch.zeros((U, 257), dtype=torch.int32, device=DEV), None)
    with pytest.raises(ValueError):
        P.recommend_list_topk(ue, ie, k, lp.cpu(), None)


def test_a_universe_of_2500_in_the_mean_variance_order_without_a_workspace():
    """Beyond the 2048 of ``pfo_recommend_mv_topk``: shortlists out of I = 2500 (synthetic embeddings), no workspace anywhere."""
    seed, U, I, D, W, k, n_t = 7, 21, 2500, 32, 64, 10, 2
    c = normal_list_case(seed, U, I, D, W, n_t)
    c.update(M.mv_side(seed, U, I, 5))
    c["list_pos"][0, :4], c["list_len"][0] = (I - 1, 2048, 2047, I), 4       # the far end of the universe by name
    got = P.recommend_list_mv_topk(*(_dev(c[n]) for n in ("user_emb", "item_emb")), k, _dev(c["list_pos"]), _dev(c["list_len"]),
                                   _dev(c["cand_stock"]), _dev(c["returns"]), _dev(c["day_idx"]), _dev(c["port_idx"]), _dev(c["port_len"]),
                                   c["gamma"], 0.5, _dev(c["user_block"]), _dev(c["item_ok"]), n_blocks=n_t, want_all=True)
    got = dict(zip(("top_pos", "top_score", "top_fused", "n_valid", "score", "y", "fused"), (t.cpu().numpy() for t in got)))
    own = L.reference_mv(c, 0.5, k, scores=_score_matrix(c, got))
    eps = R.dot_error_bound(c["user_emb"], c["item_emb"], c["user_block"], I)
    first = L.first_slots(c, own["adm"])
    assert (np.abs(got["score"].astype(np.float64) - L.by_slot(c, own["adm"], own["s64"], np.float64))[first]
            <= L.by_slot(c, own["adm"], eps, np.float64)[first]).all()
    for name, want in (("top_pos", "top_pos"), ("top_score", "top_score"), ("top_fused", "top_fused"), ("n_valid", "n_valid"),
                       ("y", "y_slot"), ("fused", "fused_slot")):
        assert _same(got[name], own[want]), name
    assert (got["top_pos"] >= 2048).any() and (own["n_valid"] == k).sum() > U // 3


# ---------------------------------------------------------------------------------------------- TGN.recommend(only=...)
# (the served world of tests/test_gpu_holdings.py: 150 nodes, D = 16, L = 1, K = 5, a ledger of width 8)
N_USERS, N_ITEMS, K_NBR, CUT, WIDTH, N_DAYS = 120, 30, 5, 900, 8, 64
ITEMS = np.arange(N_USERS + 1, N_USERS + N_ITEMS + 1)
DIV = float(1 << 18)          # synthetic.day_of is floor(ts * 64 / 2^24): the price ledger's key rule with this divisor


@pytest.fixture(scope="module")
def world():
    torch.manual_seed(6)
    g = make_graph(SyntheticConfig("t", N_USERS, N_ITEMS, 1500, 16, 1, K_NBR, 2), with_prices=True)
    d = g.data
    nf = P.NeighborFinder.from_arrays(d.sources[:CUT], d.destinations[:CUT], d.edge_idxs[:CUT], d.timestamps[:CUT], uniform=False,
                                      max_node_idx=g.node_features.shape[0] - 1)
    tgn = P.TGN(nf, g.node_features, g.edge_features[:CUT + 1], DEV, n_layers=1, n_heads=2, dropout=0.0, use_memory=True,
                memory_dimension=16, message_function="identity", n_neighbors=K_NBR)
    tgn.eval()
    tgn.track_holdings(WIDTH, g.upper_u)
    tgn.update_holdings(d.sources[:CUT], (g.portfolio_idx[:CUT], g.portfolio_len[:CUT]), d.timestamps[:CUT])
    users = np.unique(d.sources[:CUT])[:21]
    users = np.concatenate([users, users[:2]])
    ts = d.timestamps[CUT:CUT + 600:200][np.arange(len(users)) % 3]                  # three distinct times, not sorted
    rs = np.random.RandomState(4)
    lists = [[int(v) for v in rs.choice(ITEMS, size=rs.randint(0, 12))] for _ in users]
    lists[1] = []
    lists[2] = [int(ITEMS[3]), int(ITEMS[3]), 5, 10 ** 6, int(ITEMS[29])]              # a repeat, a user node, an id beyond the table
    return g, tgn, users, ts, lists


def _state(t):
    m = t.memory
    tens = [t.flat_parameters, m.memory, m.last_update, m.msg_table, m.msg_time, m.has_msg, t.holdings.idx, t.holdings.len, t.holdings.time]
    return [x.detach().clone() for x in tens], (t.training, t._step, t._gru_applied_now, m._any_msg, m._state_version, t.n_nodes)


def _unchanged(t, before):
    now = _state(t)
    return now[1] == before[1] and all(torch.equal(a, b) for a, b in zip(now[0], before[0]))


def _host_case(out, lists, item_ok=None):
    """The case dict of a ``recommend(only=lists, return_embeddings=True)`` result: its embeddings, the lists as positions."""
    ue, ie, ub = (t.cpu().numpy() for t in out[-3:])
    pos_of = {int(v): i for i, v in enumerate(ITEMS)}
    W = max(1, max(len(r) for r in lists))
    lp = np.full((len(lists), W), -1, np.int32)
    for u, r in enumerate(lists):
        lp[u, :len(r)] = [pos_of.get(v, -1) for v in r]
    return dict(user_emb=ue, item_emb=ie, user_block=ub, list_pos=lp, list_len=np.array([len(r) for r in lists], np.int32), item_ok=item_ok,
                I=N_ITEMS)


def _ids_to_pos(ids):
    ids = ids.cpu().numpy()
    return np.where(ids >= 0, ids - N_USERS - 1, -1).astype(np.int32)


def test_recommend_only_lists_against_the_reference(world):
    g, tgn, users, ts, lists = world
    ok = (np.arange(N_ITEMS) % 7 != 0)
    for mode in (True, False):
        tgn.train(mode)
        before = _state(tgn)
        out = tgn.recommend(users, ts, 5, ITEMS, only=lists, item_ok=ok, return_embeddings=True)
        assert _unchanged(tgn, before) and not any(t.requires_grad for t in out)
    tgn.eval()
    assert len(out) == 6 and len(tgn.recommend(users, ts, 5, ITEMS, only=lists)) == 3
    c = _host_case(out, lists, ok.astype(np.uint8))
    assert len(set(c["user_block"].tolist())) == 3 and (np.diff(c["user_block"]) < 0).any(), "blocks not sorted"
    s64 = R.scores64(c["user_emb"], c["item_emb"], c["user_block"], N_ITEMS)
    eps = R.dot_error_bound(c["user_emb"], c["item_emb"], c["user_block"], N_ITEMS)
    adm = L.admissible_list(len(users), N_ITEMS, c["list_pos"], c["list_len"], c["item_ok"])
    R.check_topk(_ids_to_pos(out[0]), out[1].cpu().numpy(), out[2].cpu().numpy(), s64, eps, adm, 5)
    # the kernel on those embeddings, called directly: the same bits
    direct = P.recommend_list_topk(out[3], out[4], 5, _dev(c["list_pos"]), _dev(c["list_len"]), out[5], _dev(c["item_ok"]), n_blocks=3)
    assert np.array_equal(_ids_to_pos(out[0]), direct[0].cpu().numpy()) and torch.equal(out[1], direct[1]) and torch.equal(out[2], direct[2])
    nv = out[2].cpu().numpy()
    assert nv[1] == 0 and nv[2] == 2 and (nv > 0).sum() > 10
    ids = out[0].cpu().numpy()
    assert all(set(ids[u, :nv[u]].tolist()) <= set(lists[u]) for u in range(len(users)))
    # packed on the host, packed on the device: the same query
    W = c["list_pos"].shape[1]
    packed = np.full((len(users), W), -1, np.int32)
    for u, r in enumerate(lists):
        packed[u, :len(r)] = np.minimum(r, 2 ** 31 - 1)
    for form in ((packed, c["list_len"]), (_dev(packed), _dev(c["list_len"]))):
        again = tgn.recommend(users, ts, 5, ITEMS, only=form, item_ok=ok)
        assert all(torch.equal(a, b) for a, b in zip(again, out[:3]))
    # one user alone gets what it got in the crowd; lists without a column offer nothing
    one = tgn.recommend(users[4:5], float(ts[4]), 5, ITEMS, only=lists[4:5], item_ok=ok)
    assert all(torch.equal(one[i][0], out[i][4]) for i in range(3))
    none = tgn.recommend(users, ts, 5, ITEMS, only=[[] for _ in users])
    assert not none[2].any() and (none[0] == -1).all()
    with pytest.raises(ValueError):
        tgn.recommend(users, ts, 5, ITEMS, only=lists, exclude=lists)


def test_recommend_only_held_is_the_ledgers_rows_as_lists(world):
    g, tgn, users, ts, _ = world
    idx, ln = (t.cpu().numpy() for t in tgn.holdings.rows(users))
    lists = [[int(s) + g.upper_u + 1 for s in idx[u, :ln[u]]] for u in range(len(users))]
    assert sum(len(r) for r in lists) > 20
    before = _state(tgn)
    held = tgn.recommend(users, ts, 5, ITEMS, only="held")
    want = tgn.recommend(users, ts, 5, ITEMS, only=lists)
    assert len(held) == 3 and all(torch.equal(a, b) for a, b in zip(held, want))
    assert held[2].cpu().numpy().tolist() == [min(5, len(set(r) & set(ITEMS.tolist()))) for r in lists]
    mv = P.MVSampler(g.prices, g.upper_u, DEV, day_of=g.day_of)
    held = tgn.recommend(users, ts, 5, ITEMS, only="held", mv=mv, portfolios="held")
    want = tgn.recommend(users, ts, 5, ITEMS, only=lists, mv=mv, portfolios=(idx, ln))
    assert len(held) == 4 and all(torch.equal(a, b) for a, b in zip(held, want))
    assert _unchanged(tgn, before)


def test_recommend_only_with_mv_sampler_and_price_ledger(world):
    g, tgn, users, ts, lists = world
    idx, ln = (t.cpu().numpy() for t in tgn.holdings.rows(users))
    mv = P.MVSampler(g.prices, g.upper_u, DEV, day_of=g.day_of)
    led = P.PriceLedger.from_prices(np.arange(N_DAYS), g.prices, g.upper_u, DEV, key_divisor=DIV)
    before = _state(tgn)
    out = tgn.recommend(users, ts, 5, ITEMS, only=lists, mv=mv, portfolios=(idx, ln), return_embeddings=True)
    assert len(out) == 7 and out[3].dtype == torch.float64
    for t_arg in (ts, _dev(ts)):
        again = tgn.recommend(users, t_arg, 5, ITEMS, only=lists, mv=led, portfolios=(idx, ln))
        assert len(again) == 4 and all(torch.equal(a, b) for a, b in zip(again, out[:4]))
    assert _unchanged(tgn, before)
    # against the reference's fuse over the scores the kernel itself returns for those embeddings
    c = _host_case(out, lists)
    c.update(cand_stock=(ITEMS - g.upper_u - 1).astype(np.int32), returns=mv.returns.cpu().numpy(), day_idx=g.day_of(ts).astype(np.int32),
             port_idx=idx, port_len=ln, gamma=float(mv.gamma))
    direct = _call(c, 5, 3, float(mv.lambda_mv))
    # (and over its own y: real prices are not exact arithmetic, numpy's summation order need not be the kernel's)
    own = L.reference_mv(c, float(mv.lambda_mv), 5, scores=_score_matrix(c, direct), y=_score_matrix(c, direct, "y"))
    eps = R.dot_error_bound(c["user_emb"], c["item_emb"], c["user_block"], N_ITEMS)
    first = L.first_slots(c, own["adm"])
    assert (np.abs(direct["score"].astype(np.float64) - L.by_slot(c, own["adm"], own["s64"], np.float64))[first]
            <= L.by_slot(c, own["adm"], eps, np.float64)[first]).all()
    assert np.array_equal(_ids_to_pos(out[0]), own["top_pos"]) and np.array_equal(out[2].cpu().numpy(), own["n_valid"])
    assert _same(out[1].cpu().numpy(), own["top_score"]) and _same(out[3].cpu().numpy(), own["top_fused"])
    plain = tgn.recommend(users, ts, 5, ITEMS, only=lists)
    assert not torch.equal(plain[0], out[0]), "the mean-variance side must move something"
