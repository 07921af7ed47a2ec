"""GPU tests of the group caps that count holdings: ``pfo_recommend_topk_capped_held`` / ``pfo_recommend_mv_topk_capped_held`` /
``pfo_recommend_basket_topk_capped_held`` against the numpy reference of ``recommend_capped_held_ref`` - exact arithmetic, so every
comparison is equality: positions, counts, score bits, fused values - against their ``_capped`` siblings where nothing is held, and
``TGN.recommend(held_groups=)`` and ``backtest`` end to end."""
import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

import pfotgnrec_amd as P
from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
import recommend_ref as R
import recommend_mv_ref as M
import recommend_basket_ref as B
import recommend_capped_ref as C
import recommend_capped_held_ref as H

DEV = "cuda:0"
NAMES = ("top_pos", "top_score", "top_fused", "n_valid")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _cap(groups, cap, held=None):
    kw = dict(cand_group=_dev(np.asarray(groups, np.int32)), group_cap=cap)
    if held is not None:
        kw.update(held_group=_dev(np.asarray(held[0], np.int32)), held_len=_dev(held[1]))
    return kw


def _plain(c, k, n_t, groups, cap, held=None):
    out = P.recommend_topk(_dev(c["user_emb"]), _dev(c["item_emb"]), k, _dev(c.get("user_block")), _dev(c.get("excl_pos")),
                           _dev(c.get("excl_len")), _dev(c.get("item_ok")), n_blocks=n_t, **_cap(groups, cap, held))
    return {n: t.cpu().numpy() for n, t in zip(("top_pos", "top_score", "n_valid"), out)}


def _mv_args(c, lam, k):
    return (_dev(c["user_emb"]), _dev(c["item_emb"]), k, _dev(c["cand_stock"]), _dev(c["returns"]), _dev(c["day_idx"]),
            _dev(c.get("port_idx")), _dev(c.get("port_len")), c["gamma"], lam, _dev(c.get("user_block")), _dev(c.get("excl_pos")),
            _dev(c.get("excl_len")), _dev(c.get("item_ok")))


def _mv(c, lam, k, n_t, groups, cap, held=None, want_all=False):
    out = P.recommend_mv_topk(*_mv_args(c, lam, k), n_blocks=n_t, want_all=want_all, **_cap(groups, cap, held))
    return {n: t.cpu().numpy() for n, t in zip(NAMES + ("score", "y", "fused"), out)}


def _basket(c, lam, k, n_t, groups, cap, held=None):
    return {n: t.cpu().numpy() for n, t in zip(NAMES, P.recommend_basket_topk(*_mv_args(c, lam, k), n_blocks=n_t, **_cap(groups, cap, held)))}


def _same_plain(a, b):
    return (np.array_equal(a["top_pos"], b["top_pos"]) and np.array_equal(a["n_valid"], b["n_valid"])
            and np.array_equal(np.asarray(a["top_score"]).view(np.int32), np.asarray(b["top_score"]).view(np.int32)))


def _same_mv(a, b):
    """``recommend_basket_ref.same`` to the bit: positions, counts, score bits, fused bits."""
    return (_same_plain(a, b) and np.array_equal(np.asarray(a["top_fused"]).view(np.int64), np.asarray(b["top_fused"]).view(np.int64)))


def _obeys(top_pos, n_valid, groups, cap, held):
    """Distinct picks, -1 behind them, no pick of a closed group, and picks + holdings within the cap."""
    groups = np.asarray(groups)
    for u in range(top_pos.shape[0]):
        p, h = top_pos[u, :n_valid[u]], H.held_counts(held[0], held[1], u)
        g = groups[p]
        if len(set(p.tolist())) != len(p) or (top_pos[u, n_valid[u]:] != -1).any():
            return False
        if any(int((g == v).sum()) + h.get(int(v), 0) > cap for v in np.unique(g[g >= 0])):
            return False
    return True


def _widen(held, width, n_groups, seed):
    """The held rows in ``width`` columns: the same entries, then more drawn from the same ids, the lengths redrawn over the
    whole width (every fourth row left as it is, the first emptied)."""
    ids, lens = held
    U = ids.shape[0]
    rs = np.random.RandomState(seed)
    wide = rs.randint(-1, n_groups, (U, width)).astype(np.int32)
    wide[:, :ids.shape[1]] = np.where(np.arange(ids.shape[1])[None, :] < lens[:, None], ids, wide[:, :ids.shape[1]])
    new = rs.randint(0, width + 1, U).astype(np.int32)
    new[::4] = lens[::4]
    new[0] = 0
    wide[np.arange(width)[None, :] >= new[:, None]] = -1
    return wide, new


# ---------------------------------------------------------------------------------------------- exact arithmetic

@pytest.mark.parametrize("name", sorted(C.PLAIN_CASES))
def test_plain_kernel_equals_the_reference(name):
    """One, two and three chunks (I = 513, 600, 1100 across the 512-candidate boundary), a partial 16-user tile and U = 33 past
    one, mixed blocks, D = 172, k = 64.  Before the device is looked at, by the reference alone: the holdings change a list,
    close a group from the start, leave a quota partly used where the cap is 2, and one row is empty."""
    c, groups, cap, k, n_t, ids, lens = H.plain_case(name)
    cond = H.conditions(c, groups, cap, k, ids, lens)
    assert cond["differ"] >= 1 and cond["closed"] >= 1 and cond["empty"] >= 1 and (cap != 2 or cond["partial"] >= 1), (name, cond)
    ref, got = H.reference_topk(c, groups, cap, k, ids, lens), _plain(c, k, n_t, groups, cap, (ids, lens))
    for n in ("top_pos", "top_score", "n_valid"):
        print("FIGURES held plain %s %s: %d of %d entries differ" % (name, n, int((got[n] != ref[n]).sum()), ref[n].size))
    assert _same_plain(got, ref), name
    assert _obeys(got["top_pos"], got["n_valid"], groups, cap, (ids, lens))


@pytest.mark.parametrize("spec", B.CASES, ids=lambda s: "seed%d" % s[0])
def test_mv_and_basket_kernels_equal_the_reference(spec):
    """The cases of the basket test at 3 groups with cap 1 and at 8 groups with cap 2, lambda 0, 0.5 and 1, held rows 4 wide: all
    four outputs of both forms, and the diagnostics of the mean-variance form - the UNCAPPED y and fused of every admissible
    candidate."""
    c, (seed, U, I, D, k, n_t, n_ret, W) = B.case(spec), spec
    y = None
    moved = False
    for n_groups, cap in C.MV_CAPS:
        groups = C.groups_of(seed, I, n_groups)
        held = H.held_rows_of(seed, U, n_groups, H.MV_HELD_WIDTH)
        h = [H.held_counts(held[0], held[1], u) for u in range(U)]
        assert any(any(v >= cap for v in d.values()) for d in h) and (held[1] == 0).any(), "a closed group and an empty row"
        assert cap != 2 or any(any(0 < v < cap for v in d.values()) for d in h), "a partly used quota"
        for lam in B.LAMBDAS:
            ref = H.reference_mv(c, lam, groups, cap, k, *held, y=y)
            y = ref["y_raw"]
            got = _mv(c, lam, k, n_t, groups, cap, held, want_all=True)
            assert B.same(got, ref) and _same_mv(got, ref), (spec, n_groups, cap, lam)
            assert np.array_equal(got["y"], ref["y"], equal_nan=True) and np.array_equal(got["fused"], ref["fused"], equal_nan=True)
            assert _obeys(got["top_pos"], got["n_valid"], groups, cap, held)
            moved |= bool((ref["top_pos"] != C.reference_mv(c, lam, groups, cap, k, y=y)["top_pos"]).any())
            bk, want = _basket(c, lam, k, n_t, groups, cap, held), H.reference_basket(c, lam, groups, cap, k, *held)
            assert B.same(bk, want) and _same_mv(bk, want), (spec, n_groups, cap, lam)
            assert _obeys(bk["top_pos"], bk["n_valid"], groups, cap, held)
    assert moved, "the holdings must move a list"


@pytest.mark.parametrize("D", [64, 128, 256])
def test_kernels_equal_the_reference_at_the_other_row_widths(D):
    """The cases above reach the instantiations for rows of up to 32 and 176 floats (the plain ones 64 too); these reach the ones
    for 64, 128 and 256."""
    c = M.exact_case(9000 + D, 17, 65, D, 5, 2, 29)
    groups = C.groups_of(D, 65, 3)
    held = H.held_rows_of(D, 17, 3, 5)
    assert _same_plain(_plain(c, 5, 2, groups, 2, held), H.reference_topk(c, groups, 2, 5, *held))
    assert B.same(_mv(c, 0.5, 5, 2, groups, 2, held), H.reference_mv(c, 0.5, groups, 2, 5, *held))
    assert B.same(_basket(c, 0.5, 5, 2, groups, 2, held), H.reference_basket(c, 0.5, groups, 2, 5, *held))


def test_rows_of_256_columns():
    """``held_stride`` 256, the ledger's widest row - four ballots per round in the plain kernel, the whole 1 KB of LDS in the
    other two - with cap 9 over 40 (plain: case B's inputs, three chunks of users and two of candidates) and over 8 groups, so
    that long rows leave quotas partly used and close groups."""
    c, groups, _, k, n_t, ids, lens = H.plain_case("B")
    groups = C.groups_of(77, len(groups), 40)
    held = _widen((ids, lens), 256, 40, 5)
    h = [H.held_counts(held[0], held[1], u) for u in range(len(lens))]
    assert held[1].max() > 192 and any(any(v >= 9 for v in d.values()) for d in h) and any(any(0 < v < 9 for v in d.values()) for d in h)
    ref = H.reference_topk(c, groups, 9, k, *held)
    assert (ref["top_pos"] != C.reference_topk(c, groups, 9, k)["top_pos"]).any()
    assert _same_plain(_plain(c, k, n_t, groups, 9, held), ref)
    spec = B.CASES[1]
    c, (seed, U, I, D, k, n_t, n_ret, W) = B.case(spec), spec
    groups = C.groups_of(seed, I, 8)
    held = _widen(H.held_rows_of(seed, U, 8, 4), 256, 8, 6)
    cap = 30
    h = [H.held_counts(held[0], held[1], u) for u in range(U)]
    assert any(any(v >= cap for v in d.values()) for d in h) and any(any(0 < v < cap for v in d.values()) for d in h)
    got, ref = _mv(c, 0.5, k, n_t, groups, cap, held), H.reference_mv(c, 0.5, groups, cap, k, *held)
    assert B.same(got, ref) and (ref["top_pos"] != C.reference_mv(c, 0.5, groups, cap, k)["top_pos"]).any()
    assert B.same(_basket(c, 0.5, k, n_t, groups, cap, held), H.reference_basket(c, 0.5, groups, cap, k, *held))
    with pytest.raises(ValueError, match="at most 256 columns"):
        _plain(c, k, n_t, groups, cap, (np.zeros((U, 257), np.int32), np.zeros(U, np.int32)))


# ---------------------------------------------------------------------------------------------- the sibling

def _normal(seed, U, I, D, n_t, n_ret=33, W=8):
    """Random normal embeddings, exclusion lists and an item_ok mask with the untidy mean-variance side of ``mv_side``."""
    c = R.normal_case(seed, U, I, D, n_t)
    c.update(M.mv_side(seed + 1, U, I, n_ret, W))
    return c


@pytest.mark.parametrize("U,I,D,k,n_t,kb", [(37, 600, 32, 16, 3, 4), (33, 513, 172, 10, 2, 3), (3, 2048, 172, 5, 1, 3)])
def test_nothing_held_is_the_capped_sibling_to_the_bit(U, I, D, k, n_t, kb):
    """``held_len`` 0 over rows that name every group, rows of -1, and ``held_stride`` 0 with null pointers: every output of the
    ``_capped`` entry run on the device, bit for bit, in the three forms.  The last case is the LDS bound: I = 2048, the basket at
    k = 3, D = 172 (155 904 bytes and the row)."""
    c = _normal(11 * U + I, U, I, D, n_t)
    groups, cap = C.groups_of(U, I, 6), 2
    plain, mv, bk = _plain(c, k, n_t, groups, cap), _mv(c, 0.5, k, n_t, groups, cap, want_all=True), _basket(c, 0.5, kb, n_t, groups, cap)
    full = np.tile(np.arange(8, dtype=np.int32) % 6, (U, 1))
    for held in ((full, np.zeros(U, np.int32)), (np.full((U, 8), -1, np.int32), np.full(U, 8, np.int32)),
                 (full, np.full(U, -5, np.int32)), (np.zeros((U, 0), np.int32), np.zeros(U, np.int32))):
        assert _same_plain(_plain(c, k, n_t, groups, cap, held), plain)
        got = _mv(c, 0.5, k, n_t, groups, cap, held, want_all=True)
        assert _same_mv(got, mv) and all(np.array_equal(got[n], mv[n], equal_nan=True) for n in ("score", "y", "fused"))
        assert _same_mv(_basket(c, 0.5, kb, n_t, groups, cap, held), bk)
    # and held rows that bind, over the device's own scores: the reference needs no rounding tolerance
    held = H.held_rows_of(U, U, 6, 8)
    scores = mv["score"]
    base = R.admissible(U, I, c["excl_pos"], c["excl_len"], c["item_ok"])
    pos, sc, n = H.topk_capped_held(scores, base, groups, cap, k, *held)
    got = _plain(c, k, n_t, groups, cap, held)
    assert _same_plain(got, dict(top_pos=pos, top_score=sc, n_valid=n)) and not _same_plain(got, plain)
    assert B.same(_mv(c, 0.5, k, n_t, groups, cap, held), H.reference_mv(c, 0.5, groups, cap, k, *held, scores=scores))
    assert B.same(_basket(c, 0.5, kb, n_t, groups, cap, held), H.reference_basket(c, 0.5, groups, cap, kb, *held, scores=scores))


def test_basket_under_holdings_equals_the_loop_of_single_picks():
    """What the one launch replaces: k launches of the UNCAPPED ``pfo_recommend_mv_topk`` at k = 1, the closed groups - from the
    start, or by the picks - appended to the exclusion row."""
    U, I, D, k, n_t = 33, 257, 32, 8, 3
    c = _normal(7 * U + I, U, I, D, n_t, 29)
    groups = C.groups_of(I, I, 4)
    held = H.held_rows_of(I, U, 4, 3)
    got = _basket(c, 0.5, k, n_t, groups, 2, held)
    plain_mv = lambda cc: {n: t.cpu().numpy() for n, t in zip(NAMES, P.recommend_mv_topk(*_mv_args(cc, 0.5, 1), n_blocks=n_t))}
    want = H.loop_of_single_picks_capped_held(c, groups, 2, k, plain_mv, *held)
    assert B.same(got, want) and _obeys(got["top_pos"], got["n_valid"], groups, 2, held)
    assert not B.same(got, _basket(c, 0.5, k, n_t, groups, 2)), "the holdings must move a list"


# ---------------------------------------------------------------------------------------------- TGN.recommend and backtest end to end
# (the small served world of tests/test_gpu_recommend_capped.py, with a holdings ledger)
N_USERS, N_ITEMS, K_NBR, CUT, LOG, BATCH, N_DAYS = 30, 40, 5, 300, 32, 16, 64
ITEMS = np.arange(N_USERS + 1, N_USERS + N_ITEMS + 1)
GROUPS = np.arange(N_ITEMS) % 5 - 1                                     # eight items in no group, four groups of eight
CAP = 2


class _SynTables(P.InvestTables):
    """InvestTables over the synthetic calendar: the day of a timestamp is the graph's ``day_of``."""

    def day_indices(self, timestamps):
        return ((np.asarray(timestamps).astype(np.int64) * N_DAYS) >> 24).astype(np.int32)


class _World:
    def __init__(self):
        self.g = g = make_graph(SyntheticConfig("t", N_USERS, N_ITEMS, 400, 16, 2, K_NBR, 2), with_prices=True)
        d = g.data
        assert g.upper_u == N_USERS                                    # stock index = position in ITEMS: GROUPS serves as stock_groups
        sl = slice(CUT, CUT + LOG)
        self.log = (d.sources[sl], d.destinations[sl], d.timestamps[sl], d.edge_idxs[sl])
        self.ports = (g.portfolio_idx[sl].astype(np.int32), g.portfolio_len[sl].astype(np.int32))
        self.mv = P.MVSampler(g.prices, g.upper_u, DEV, day_of=g.day_of)
        rs = np.random.RandomState(4)
        future = g.prices * np.exp(np.cumsum(rs.randn(*g.prices.shape) * 0.02, axis=2))
        self.tables = _SynTables.from_prices(list(range(N_DAYS)), g.prices, future, g.map_item_id, upper_u=g.upper_u)

    def model(self):
        torch.manual_seed(6)
        g, d = self.g, self.g.data
        nf = P.NeighborFinder.from_arrays(d.sources[:CUT], d.destinations[:CUT], d.edge_idxs[:CUT], d.timestamps[:CUT], uniform=False,
                                          max_node_idx=g.node_features.shape[0] - 1)
        t = P.TGN(nf, g.node_features, g.edge_features, DEV, n_layers=2, n_heads=2, dropout=0.0, use_memory=True,
                  memory_dimension=16, message_function="identity", n_neighbors=K_NBR)
        t.eval()
        t.observe(d.sources[:CUT], d.destinations[:CUT], d.timestamps[:CUT], d.edge_idxs[:CUT], batch_size=50)
        t.track_holdings(max(1, g.portfolio_idx.shape[1]), g.upper_u)
        t.update_holdings(d.sources[:CUT], (g.portfolio_idx[:CUT], g.portfolio_len[:CUT]), d.timestamps[:CUT])
        return t


@pytest.fixture(scope="module")
def world():
    return _World()


def _state(t):
    m = t.memory
    out = [x.detach().clone() for x in (t.flat_parameters, m.memory, m.last_update, m.msg_table, m.msg_time, m.has_msg, t.holdings.idx,
                                        t.holdings.len, t.holdings.time)]
    if t._flat_grad is not None:
        out.append(t._flat_grad.clone())
    return out, (t.training, t._step, t._gru_applied_now, t.memory._any_msg, t.memory._state_version)


def _group_lists(idx, ln):
    return [[int(GROUPS[s]) if 0 <= s < N_ITEMS else -1 for s in idx[u, :ln[u]]] for u in range(len(ln))]


def test_recommend_counts_holdings_in_the_three_orders_and_writes_nothing(world):
    w = world
    t = w.model()
    src, _, log_ts, _ = w.log
    users, ts, k = src[:BATCH], np.full(BATCH, float(log_ts[0])), 8
    ts[::3] += 64.0                                                     # two blocks, mixed: the held rows follow the block sort
    ok = np.arange(N_ITEMS) % 7 != 0
    idx, ln = (x.cpu().numpy() for x in t.holdings.rows(users))
    lists = _group_lists(idx, ln)
    packed = (np.array([r + [-1] * (idx.shape[1] - len(r)) for r in lists], np.int32).reshape(BATCH, -1), ln.astype(np.int32))
    h = [H.held_counts(*packed, u) for u in range(BATCH)]
    assert any(any(v >= CAP for v in d.values()) for d in h) and any(any(0 < v < CAP for v in d.values()) for d in h)
    cap = dict(groups=GROUPS, group_cap=CAP)
    sg64 = torch.from_numpy(GROUPS.astype(np.int64)).to(DEV)
    for order in (dict(), dict(mv=w.mv), dict(mv=w.mv, basket=True)):
        ports = dict(portfolios=(idx, ln)) if order else {}
        before = _state(t)
        out = t.recommend(users, ts, k, ITEMS, item_ok=ok, held_groups=lists, **cap, **order, **ports)
        now = _state(t)
        assert all(torch.equal(x, y) for x, y in zip(before[0], now[0])) and before[1] == now[1]
        assert not any(x.requires_grad for x in out)
        ids, n_valid = out[0].cpu().numpy(), out[2].cpu().numpy()
        pos = np.where(ids >= 0, ids - N_USERS - 1, -1)
        assert _obeys(pos, n_valid, GROUPS, CAP, packed) and ok[pos[pos >= 0]].all()
        for u in range(BATCH):                                          # a closed sector offers nothing
            assert not any(h[u].get(int(GROUPS[p]), 0) >= CAP for p in pos[u, :n_valid[u]] if GROUPS[p] >= 0)
        capped = t.recommend(users, ts, k, ITEMS, item_ok=ok, **cap, **order, **ports)
        assert not torch.equal(capped[0], out[0]), "a held name in a capped sector must move a list"
        # the packed pair on host and device, the ledger by name, the portfolio rows by name: the same query
        forms = [dict(held_groups=packed), dict(held_groups=(_dev(packed[0]).long(), _dev(packed[1]))),
                 dict(held_groups="held", stock_groups=GROUPS), dict(held_groups="held", stock_groups=sg64),
                 dict(held_groups="portfolios", stock_groups=GROUPS.tolist(), portfolios=(idx, ln))]
        if order:
            forms.append(dict(held_groups="portfolios", stock_groups=GROUPS, portfolios="held"))
        for form in forms:
            again = t.recommend(users, ts, k, ITEMS, item_ok=ok, **cap, **order, **dict(ports, **form))
            assert len(again) == len(out) and all(torch.equal(x, y) for x, y in zip(again, out)), (sorted(order), sorted(form))
        # nobody holds anything: the query with the cap alone
        none = t.recommend(users, ts, k, ITEMS, item_ok=ok, held_groups=[[] for _ in users], **cap, **order, **ports)
        assert all(torch.equal(x, y) for x, y in zip(none, capped))
        # stocks outside stock_groups are holdings in no group
        short = t.recommend(users, ts, k, ITEMS, item_ok=ok, held_groups="held", stock_groups=GROUPS[:0], **cap, **order, **ports)
        assert all(torch.equal(x, y) for x, y in zip(short, capped))
        assert all(torch.equal(x, y) for x, y in zip(before[0], _state(t)[0]))
    with pytest.raises(ValueError, match="held_groups needs groups"):
        t.recommend(users, ts, k, ITEMS, held_groups=lists)


def test_backtest_with_held_groups_is_recommend_score_observe_by_hand(world):
    """``backtest_rows(held_groups="held", stock_groups=)`` on one short log against a twin model walked by hand: the lists of
    ``recommend``, ``list_metrics`` on them, ``observe``; and rows over the log against ``"portfolios"``."""
    w = world
    src, dst, ts, eidx = w.log
    cuts = (1, 3, 6)
    kw = dict(cutoffs=cuts, batch_size=BATCH, tables=w.tables, mv=w.mv, portfolios=w.ports, groups=GROUPS, group_cap=1)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)
    rows = P.backtest_rows(w.model(), src, dst, ts, eidx, ITEMS, 6, held_groups="held", stock_groups=GROUPS, **kw)
    out = P.backtest(w.model(), src, dst, ts, eidx, ITEMS, 6, name="held", held_groups="held", stock_groups=GROUPS, **kw)
    assert out["held_recall_avg_6"] == np.mean((rows["rank"] < 6).astype(np.float64)) and out["n"] == LOG
    assert not np.array_equal(rows["list_item"], P.backtest_rows(w.model(), src, dst, ts, eidx, ITEMS, 6, **kw)["list_item"])
    b = w.model()
    rp, rf = w.tables.device_tables(DEV)
    day = i32(w.g.day_of(ts))
    for lo in range(0, LOG, BATCH):
        hi = lo + BATCH
        ports = (w.ports[0][lo:hi], w.ports[1][lo:hi])
        res = b.recommend(src[lo:hi], ts[lo:hi], 6, ITEMS, mv=w.mv, portfolios=ports, groups=GROUPS, group_cap=1, held_groups="held",
                          stock_groups=GROUPS)
        assert np.array_equal(res[0].cpu().numpy(), rows["list_item"][lo:hi]) and np.array_equal(res[2].cpu().numpy(), rows["n_valid"][lo:hi])
        hand = P.list_metrics(res[0], i32(dst[lo:hi]), cuts, i32(ports[0]), i32(ports[1]), w.g.upper_u, rp, day[lo:hi], rf, day[lo:hi], res[2])
        for name, hv in zip(("rank", "recall", "ndcg", "invest"), hand):
            hv = hv.cpu().numpy()
            assert np.array_equal(hv.view(np.uint8), rows[name][lo:hi].view(np.uint8)), (name, lo)
        b.observe(src[lo:hi], dst[lo:hi], ts[lo:hi], eidx[lo:hi], batch_size=None)
    # the portfolios of the log by name, and as explicit rows of group ids cut per batch: one walk
    by_name = P.backtest_rows(w.model(), src, dst, ts, eidx, ITEMS, 6, held_groups="portfolios", stock_groups=GROUPS, **kw)
    explicit = P.backtest_rows(w.model(), src, dst, ts, eidx, ITEMS, 6, held_groups=_group_lists(*w.ports), **kw)
    assert all(np.array_equal(by_name[n].view(np.uint8), explicit[n].view(np.uint8)) for n in by_name)
    assert not np.array_equal(by_name["list_item"], P.backtest_rows(w.model(), src, dst, ts, eidx, ITEMS, 6, **kw)["list_item"])
