"""Host side of the group caps that count holdings (``pfo_recommend_*_topk_capped_held`` / ``TGN.recommend(held_groups=)``): the
numpy reference (``recommend_capped_held_ref``) against a brute-force greedy, its count form and its chunk form, the ``n_valid``
formula, empty rows against the capped reference, the basket against the loop of single picks; the header and the ctypes table
against the ``_capped`` siblings, every new bound refused without a device, every ValueError of ``recommend.validate`` and of
``backtest``; and the conditions the GPU test's plain cases rest on, from their inputs alone."""
import importlib
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

import pfotgnrec_amd as P
from pfotgnrec_amd import _lib
from pfotgnrec_amd import recommend as RC
import recommend_ref as R
import recommend_mv_ref as M
import recommend_basket_ref as B
import recommend_capped_ref as C
import recommend_capped_held_ref as H

BT = importlib.import_module("pfotgnrec_amd.backtest")    # (the package's ``backtest`` is the function)

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pfotgn.h")


# ---------------------------------------------------------------------------------------------- the reference

def _small(rs):
    """A small random row: scores with ties (and both zeros), a mask, groups with groupless candidates, a cap, a depth and a
    held row with negative and repeated ids (as a dict of counts)."""
    I = int(rs.randint(1, 41))
    scores = rs.randint(-3, 4, I).astype(np.float64)
    scores[rs.rand(I) < 0.1] = -0.0
    adm = rs.rand(I) > 0.2
    n_groups = int(rs.randint(1, 6))
    groups = rs.randint(-1, n_groups, I).astype(np.int32)
    row = rs.randint(-1, n_groups, (1, int(rs.randint(0, 7)))).astype(np.int32)
    ln = np.array([rs.randint(0, row.shape[1] + 1)], np.int32)
    return I, scores, adm, groups, int(rs.randint(1, 4)), int(rs.randint(1, 12)), row, ln


def _greedy(scores, adm, groups, cap, k, h):
    """The greedy list by definition: again and again the best candidate left that may still be taken, the holdings counted
    with the picks."""
    left = [c for c in range(len(scores)) if adm[c]]
    taken = []
    while len(taken) < k:
        may = [c for c in left if groups[c] < 0 or sum(groups[t] == groups[c] for t in taken) + h.get(int(groups[c]), 0) < cap]
        if not may:
            break
        best = max(may, key=lambda c: (scores[c], c))
        taken.append(best)
        left.remove(best)
    return taken


def test_held_counts_ignore_negatives_and_the_tail_and_count_repeats():
    ids = np.array([[2, -1, 2, 0, 5], [1, 1, 1, 1, 1]], np.int32)
    assert H.held_counts(ids, np.array([4, 0], np.int32), 0) == {2: 2, 0: 1} and H.held_counts(ids, np.array([4, 0], np.int32), 1) == {}
    assert H.held_counts(ids, np.array([9, -3], np.int32), 0) == {2: 2, 0: 1, 5: 1}, "the length is clamped to the width"
    assert H.held_counts(ids, np.array([9, -3], np.int32), 1) == {} and H.held_counts(None, None, 0) == {}


def test_walk_count_form_chunk_form_and_greedy_agree():
    rs = np.random.RandomState(10)
    closed = partial = 0
    for _ in range(500):
        I, scores, adm, groups, cap, k, row, ln = _small(rs)
        h = H.held_counts(row, ln, 0)
        closed += any(v >= cap for v in h.values())
        partial += any(0 < v < cap for v in h.values())
        order = R.canonical_order(scores)
        order = order[adm[order]]
        walk = H.capped_walk(order, groups, cap, k, h)
        assert walk.tolist() == _greedy(scores, adm, groups, cap, k, h) == H.brute_force(order, groups, cap, k, h).tolist()
        assert np.array_equal(H.survivors(order, groups, cap, h)[:k], walk)
        place = np.empty(I, np.int64)
        place[R.canonical_order(scores)] = np.arange(I)
        for chunk in range(1, 21):
            assert np.array_equal(H.chunked(place, np.flatnonzero(adm), groups, cap, k, chunk, h), walk), chunk
        pos, sc, n = H.topk_capped_held(scores[None], adm[None], groups, cap, k, row, ln)
        assert pos[0, :n[0]].tolist() == walk.tolist() and (pos[0, n[0]:] == -1).all() and np.isneginf(sc[0, n[0]:]).all()
        assert n[0] == H.n_valid_formula(adm, groups, cap, k, h)
    assert closed >= 50 and partial >= 25, "the random rows must reach both a closed group and a partly used quota"


def test_empty_rows_give_the_capped_reference():
    rs = np.random.RandomState(11)
    for _ in range(200):
        I, scores, adm, groups, cap, k, row, ln = _small(rs)
        want = C.topk_capped(scores[None], adm[None], groups, cap, k)
        for hg, hl in ((row, np.zeros(1, np.int32)), (np.zeros((1, 0), np.int32), np.zeros(1, np.int32)), (None, None),
                       (np.full((1, 3), -1, np.int32), np.full(1, 3, np.int32))):
            got = H.topk_capped_held(scores[None], adm[None], groups, cap, k, hg, hl)
            assert all(np.array_equal(a, b) for a, b in zip(got, want))
    spec = B.CASES[1]
    c, (seed, U, I, D, k, n_t, n_ret, W) = B.case(spec), spec
    groups = C.groups_of(seed, I, 3)
    none = (np.zeros((U, 4), np.int32), np.zeros(U, np.int32))
    assert B.same(H.reference_mv(c, 0.5, groups, 1, k, *none), C.reference_mv(c, 0.5, groups, 1, k))
    assert B.same(H.reference_basket(c, 0.5, groups, 1, k, *none), C.reference_basket(c, 0.5, groups, 1, k))


# the figures of the issue: (users whose list differs from the capped list without holdings, users, users with a closed group)
CONDITIONS = {"A": (15, 20, 16), "B": (29, 37, 18), "C": (19, 20, 19), "E": (7, 9, 2), "F": (29, 33, 30)}


@pytest.mark.parametrize("name", sorted(C.PLAIN_CASES))
def test_the_holdings_bind_in_the_plain_cases(name):
    """What the GPU test asserts before it trusts a case, here with the issue's counts, and the ``n_valid`` formula on them."""
    c, groups, cap, k, n_t, ids, lens = H.plain_case(name)
    cond = H.conditions(c, groups, cap, k, ids, lens)
    U = c["user_emb"].shape[0]
    print("FIGURES case %s: holdings change %d of %d lists, %d users with a closed group, %d with a partly used quota, %d empty rows"
          % (name, cond["differ"], U, cond["closed"], cond["partial"], cond["empty"]))
    assert (cond["differ"], U, cond["closed"]) == CONDITIONS[name]
    assert cond["differ"] >= 1 and cond["closed"] >= 1 and cond["empty"] >= 1 and (cap != 2 or cond["partial"] >= 1)
    assert (ids[np.arange(ids.shape[1])[None, :] >= lens[:, None]] == -1).all()
    ref = H.reference_topk(c, groups, cap, k, ids, lens)
    assert ref["n_valid"].tolist() == [H.n_valid_formula(ref["adm"][u], groups, cap, k, H.held_counts(ids, lens, u)) for u in range(U)]


@pytest.mark.parametrize("spec", B.CASES[:3] + B.CASES[4:], ids=lambda s: "seed%d" % s[0])
def test_the_basket_under_holdings_is_the_loop_of_single_picks(spec):
    """k single picks of the UNCAPPED mean-variance reference, the closed groups - from the start, or by the picks - appended to
    the exclusion row.  And the mean-variance list keeps the uncapped values and is the count form of its order."""
    c, (seed, U, I, D, k, n_t, n_ret, W) = B.case(spec), spec
    for n_groups, cap in C.MV_CAPS:
        groups = C.groups_of(seed, I, n_groups)
        ids, lens = H.held_rows_of(seed, U, n_groups, H.MV_HELD_WIDTH)
        for lam in B.LAMBDAS:
            got = H.reference_basket(c, lam, groups, cap, k, ids, lens)
            want = H.loop_of_single_picks_capped_held(c, groups, cap, k, lambda cc: M.reference(cc, lam, 1), ids, lens)
            assert B.same(got, want), (n_groups, cap, lam)
            for u in range(U):                                          # the quota holds, picks are distinct
                p, h = got["top_pos"][u, :got["n_valid"][u]], H.held_counts(ids, lens, u)
                g = groups[p]
                assert len(set(p.tolist())) == len(p) and all(int((g == v).sum()) + h.get(int(v), 0) <= max(cap, h.get(int(v), 0))
                                                              for v in np.unique(g[g >= 0]))
                assert not any(h.get(int(v), 0) >= cap for v in g[g >= 0]), "a closed group gives no pick"
        mv = H.reference_mv(c, 0.5, groups, cap, k, ids, lens)
        plain = M.reference(c, 0.5, k)
        assert np.array_equal(mv["fused"], plain["fused"], equal_nan=True)
        s64 = R.scores64(c["user_emb"], c["item_emb"], c["user_block"], I)
        for u in range(U):
            n, h = mv["n_valid"][u], H.held_counts(ids, lens, u)
            p = mv["top_pos"][u, :n]
            assert n == H.n_valid_formula(mv["adm"][u], groups, cap, k, h)
            assert np.array_equal(mv["top_fused"][u, :n], plain["fused"][u, p])
            order = M.fuse(s64[u][None], mv["y_raw"][u][None], mv["adm"][u][None], 0.5, I)[0][0, :int(mv["adm"][u].sum())]
            assert np.array_equal(H.survivors(order, groups, cap, h)[:k], p)


# ---------------------------------------------------------------------------------------------- the C ABI

def _declaration(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^(\w+) %s\(([^;]*)\);" % name, text, re.M)
    assert m, "%s is not declared in include/pfotgn.h" % name
    return m.group(1), [a.strip() for a in m.group(2).replace("\n", " ").split(",")]


SIBLINGS = ("pfo_recommend_topk_capped", "pfo_recommend_mv_topk_capped", "pfo_recommend_basket_topk_capped")


@pytest.mark.parametrize("sibling", SIBLINGS)
def test_header_and_ctypes_table(sibling):
    """The ``_capped`` sibling's parameter list with (held_group, held_len, held_stride) directly behind group_cap and nothing
    else changed - in the header and in the ctypes table; the abi keeps its number."""
    ret, old = _declaration(sibling)
    ret_h, new = _declaration(sibling + "_held")
    at = old.index("int32_t group_cap") + 1
    assert at == 13 and ret == ret_h == "int"
    assert new == old[:at] + ["const int32_t* held_group", "const int32_t* held_len", "int32_t held_stride"] + old[at:]
    (res, args), (res_h, args_h) = _lib.PROTOTYPES[sibling], _lib.PROTOTYPES[sibling + "_held"]
    assert res is res_h and args_h == args[:at] + [_lib._VP, _lib._VP, _lib.C.c_int32] + args[at:] and len(args_h) == len(new)
    lib = _lib.load()
    assert hasattr(lib, sibling + "_held") and lib.pfo_abi_version() == 6
    assert re.search(r"#define PFO_RECOMMEND_HELD_MAX_WIDTH\s+256\b", open(HEADER).read()) and _lib.RECOMMEND_HELD_MAX_WIDTH == 256
    assert _lib.RECOMMEND_HELD_MAX_WIDTH == importlib.import_module("pfotgnrec_amd.holdings").MAX_WIDTH


def _plain_args(U=3, I=10, n_t=1, D=8, excl_stride=0, k=3, group_cap=1, held_stride=0, held=(None, None), others=None, group=None):
    o = others
    return ("pfo_recommend_topk_capped_held", o, o, None, U, I, n_t, D, None, None, excl_stride, None, group, group_cap, held[0], held[1],
            held_stride, k, o, o, None, None)


def _mv_args(symbol, tail):
    def args(U=3, I=10, n_t=1, D=8, excl_stride=0, k=3, group_cap=1, held_stride=0, held=(None, None), others=None, group=None, n_ret=29,
             port_stride=0, n_days=2, n_stocks=5):
        o = others
        return (symbol, o, o, None, U, I, n_t, D, None, None, excl_stride, None, group, group_cap, held[0], held[1], held_stride, o, o,
                n_days, n_stocks, n_ret, o, None, None, port_stride, 2.0, 0.5, k, o, o, o) + (None,) * (tail - 3)
    return args


ENTRIES = {"plain": (_plain_args, 65536), "mv": (_mv_args("pfo_recommend_mv_topk_capped_held", 8), 2048),
           "basket": (_mv_args("pfo_recommend_basket_topk_capped_held", 5), 2048)}
BOUNDS = [(dict(D=6), "D must be a positive multiple of 4"), (dict(D=260), "D must be at most 256"), (dict(k=0), "k must be in"),
          (dict(k=65), "k must be in"), (dict(I=0), "I must be in"), (dict(n_t=0), "n_t must be at least 1"),
          (dict(excl_stride=-1), "must not be negative"), (dict(group_cap=0), "group_cap must be at least 1"),
          (dict(held_stride=-1), "held_stride must be in"), (dict(held_stride=257), "held_stride must be in"),
          (dict(held_stride=2 ** 31 - 1), "held_stride must be in")]
MV_BOUNDS = [(dict(n_ret=1), "n_ret must be in"), (dict(n_ret=129), "n_ret must be in"), (dict(port_stride=-1), "must not be negative"),
             (dict(n_days=0), "must be positive"), (dict(n_stocks=0), "must be positive")]


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_every_bound_is_refused_before_a_pointer_is_looked_at(entry):
    """All pointers are NULL: a refusal that names the entry and the bound shows the bound was checked first, with and without
    users.  Nothing is queued (no device is needed for any of this)."""
    args, max_items = ENTRIES[entry]
    name = args()[0]
    for kw, msg in BOUNDS + [(dict(I=max_items + 1), "I must be in")] + (MV_BOUNDS if entry != "plain" else []):
        for U in (3, 0):
            with pytest.raises(_lib.PfoError, match=name + ": .*" + msg):
                _lib.call(*args(U=U, **kw))
    with pytest.raises(_lib.PfoError, match="null"):                    # every bound kept: the NULL pointers are what is left
        _lib.call(*args(held_stride=256))
    _lib.call(*args(U=0))                                               # U == 0: accepted, no pointer is looked at
    _lib.call(*args(U=0, I=max_items, D=256, k=64, group_cap=64, held_stride=256))


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_null_held_rows_are_refused_by_name(entry):
    """Every other pointer given (host memory: nothing is launched before the refusal): with a stride, held_group and held_len
    are both needed; cand_group is still asked for first."""
    buf = (_lib.C.c_char * 4096)()
    p = _lib.C.addressof(buf)
    p += -p % 16
    args, _ = ENTRIES[entry]
    name = args()[0]
    with pytest.raises(_lib.PfoError, match=name + ": null cand_group"):
        _lib.call(*args(others=p, held_stride=4, held=(p, p)))
    for held in ((None, None), (p, None), (None, p)):
        with pytest.raises(_lib.PfoError, match=name + ": null held_group or held_len"):
            _lib.call(*args(others=p, group=p, held_stride=4, held=held))


# ---------------------------------------------------------------------------------------------- the functional forms

def test_the_functional_forms_validate_then_require_a_gpu():
    ue, ie = torch.zeros(3, 8), torch.zeros(10, 8)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    mv = dict(cand_stock=i32(10), returns=torch.zeros(2, 5, 29, dtype=torch.float64), day_idx=i32(3), port_idx=None, port_len=None,
              gamma=2.0, lambda_mv=0.5)
    forms = ((P.recommend_topk, dict(user_emb=ue, item_emb=ie, k=3)), (P.recommend_mv_topk, dict(user_emb=ue, item_emb=ie, k=3, **mv)),
             (P.recommend_basket_topk, dict(user_emb=ue, item_emb=ie, k=3, **mv)))
    cap = dict(cand_group=i32(10), group_cap=2)
    for fn, good in forms:
        for kw in (dict(held_group=i32(3, 4)), dict(held_group=i32(3, 4), held_len=i32(3), group_cap=2),
                   dict(held_len=i32(3), **cap), dict(held_group=i32(2, 4), **cap), dict(held_group=i32(3, 4), held_len=i32(2), **cap),
                   dict(held_group=i32(3, 257), **cap), dict(held_group=i32(12), **cap), dict(held_group=torch.zeros(3, 4, dtype=torch.int64), **cap),
                   dict(held_group=i32(3, 4), held_len=torch.zeros(3, dtype=torch.int64), **cap), dict(held_group=[[0]] * 3, **cap)):
            with pytest.raises(ValueError):
                fn(**dict(good, **kw))
        if not torch.cuda.is_available():
            with pytest.raises(_lib.PfoError):                          # valid: only the device is missing - no fallback
                fn(held_group=i32(3, 256), held_len=i32(3), **cap, **good)
    for fn in (P.recommend_mv_topk_wide, P.recommend_list_topk, P.recommend_list_mv_topk):
        with pytest.raises(TypeError):                                  # the wide and the list forms take no held rows
            fn(ue, ie, 3, held_group=i32(3, 4))


# ---------------------------------------------------------------------------------------------- validate and backtest

def _mv_object():
    return types.SimpleNamespace(returns=np.zeros((2, 30, 3)), upper_u=4, gamma=2.0, lambda_mv=0.5, day_of=None)


G = np.arange(20) % 3 - 1
LEDGER = types.SimpleNamespace(upper_u=4)


def _validate(I=20, **kw):
    return RC.validate(I + 10, None, [1, 2, 3], 5.0, 3, np.arange(5, I + 5), kw.pop("exclude", None), None, None, **kw)


def test_validate_takes_held_groups_in_every_form():
    q = _validate(groups=G, group_cap=2)
    assert q.held_mode is None and q.hg_ids is None and q.hg_len is None and q.stock_groups is None
    q = _validate(groups=G, group_cap=2, held_groups=[[0, 0, -1], [], [1]])
    assert q.held_mode == "rows" and q.hg_ids.dtype == np.int32 and q.hg_ids.tolist() == [[0, 0, -1], [-1, -1, -1], [1, -1, -1]]
    assert q.hg_len.tolist() == [3, 0, 1]
    ids, lens = torch.zeros(3, 256, dtype=torch.int64), torch.zeros(3, dtype=torch.int32)
    q = _validate(groups=G, group_cap=2, held_groups=(ids, lens))
    assert q.held_mode == "rows" and q.hg_ids is ids and q.hg_len is lens, "a packed device pair is not read back"
    q = _validate(groups=G, group_cap=2, held_groups=(np.zeros((3, 0), np.int32), np.zeros(3, np.int32)))
    assert q.held_mode == "rows" and q.hg_ids.shape == (3, 0)
    sg = np.arange(7, dtype=np.int64) - 1
    q = _validate(groups=G, group_cap=2, held_groups="held", stock_groups=sg, holdings=LEDGER)
    assert q.held_mode == "held" and q.stock_groups.dtype == np.int32 and q.stock_groups.tolist() == sg.tolist() and q.held is None
    t = torch.from_numpy(sg)
    mv = _mv_object()
    for basket in (False, True):
        q = _validate(groups=G, group_cap=2, held_groups="portfolios", stock_groups=t, mv=mv, portfolios=[[1], [], [2, 3]], day_idx=0,
                      basket=basket)
        assert q.held_mode == "portfolios" and q.stock_groups is t and q.mv.port_idx.shape == (3, 2)
    q = _validate(groups=G, group_cap=2, held_groups="portfolios", stock_groups=sg, mv=mv, portfolios="held", day_idx=0, holdings=LEDGER)
    assert q.held_mode == "portfolios" and q.mv.port_idx is None


def _refusals(call, rows=3):
    """Every ValueError the issue lists, through ``call(**keywords)``; ``rows``: how many rows ``held_groups`` must list."""
    cap = dict(groups=G, group_cap=2)
    some = [[0]] * rows
    sg = np.zeros(5, np.int32)
    mv = dict(mv=_mv_object(), portfolios=[[1]] * rows, day_idx=0)
    for kw, msg in ((dict(held_groups=some), "held_groups needs groups"), (dict(held_groups="held", stock_groups=sg), "held_groups needs groups"),
                    (dict(held_groups="held", stock_groups=sg, **cap), "needs a holdings ledger"),
                    (dict(held_groups="held", holdings=LEDGER, **cap), "needs stock_groups"),
                    (dict(held_groups="portfolios", **cap, **mv), "needs stock_groups"),
                    (dict(held_groups="portfolios", stock_groups=sg, **cap), "needs portfolios"),
                    (dict(held_groups="mine", stock_groups=sg, **cap), "held_groups must be"),
                    (dict(stock_groups=sg, **cap), "stock_groups without held_groups"),
                    (dict(held_groups=some, stock_groups=sg, **cap), "explicit rows hold group ids already"),
                    (dict(held_groups=[list(range(257))] + some[1:], **cap), "at most 256"),
                    (dict(held_groups=(np.zeros((rows, 257), np.int32), np.zeros(rows, np.int32)), **cap), "at most 256"),
                    (dict(held_groups=(torch.zeros(rows, 257, dtype=torch.int32), torch.zeros(rows, dtype=torch.int32)), **cap), "at most 256"),
                    (dict(held_groups="portfolios", stock_groups=sg, **cap, **dict(mv, portfolios=[list(range(257))] + [[1]] * (rows - 1))),
                     "at most 256"),
                    (dict(held_groups=some[:-1], **cap), "held_groups lists %d" % (rows - 1)),
                    (dict(held_groups=(np.zeros((rows + 1, 2), np.int32), np.zeros(rows + 1, np.int32)), **cap), "packed held_groups must be"),
                    (dict(held_groups=[[0.5]] * rows, **cap), "held_groups must be"), (dict(held_groups=[["a"]] * rows, **cap), "held_groups must be"),
                    (dict(held_groups=(np.zeros((rows, 2)), np.zeros(rows, np.int32)), **cap), "must be integers"),
                    (dict(held_groups=(np.zeros((rows, 2), np.int32), np.zeros(rows)), **cap), "must be integers"),
                    (dict(held_groups=(torch.zeros(rows, 2), torch.zeros(rows, dtype=torch.int32)), **cap), "must be integers"),
                    (dict(held_groups=[[2 ** 31]] * rows, **cap), "do not fit 32 bits"),
                    (dict(held_groups=(np.full((rows, 1), -2 ** 31 - 1, np.int64), np.ones(rows, np.int32)), **cap), "do not fit 32 bits"),
                    (dict(held_groups="held", stock_groups=np.zeros(5), holdings=LEDGER, **cap), "one integer per stock index"),
                    (dict(held_groups="held", stock_groups=torch.zeros(5), holdings=LEDGER, **cap), "one integer per stock index"),
                    (dict(held_groups="held", stock_groups=np.zeros((5, 1), np.int32), holdings=LEDGER, **cap), "one integer per stock index"),
                    (dict(held_groups="held", stock_groups=["a"], holdings=LEDGER, **cap), "one integer per stock index"),
                    (dict(held_groups="held", stock_groups=np.full(5, 2 ** 31, np.int64), holdings=LEDGER, **cap), "do not fit 32 bits")):
        with pytest.raises(ValueError, match=msg):
            call(**kw)


def test_validate_refuses_what_held_groups_cannot_be():
    _refusals(_validate)
    # what groups refuses stays refused with holdings beside it
    with pytest.raises(ValueError, match="the list forms have no capped order"):
        _validate(groups=G, group_cap=1, held_groups=[[0]] * 3, only=[[5], [6], [7]])
    with pytest.raises(ValueError, match="the capped order has no wide form"):
        _validate(I=2049, groups=np.zeros(2049, np.int32), group_cap=1, held_groups=[[0]] * 3, mv=_mv_object(), portfolios=[[], [], []],
                  day_idx=0)


def test_backtest_makes_the_same_checks_before_any_device_work():
    """``backtest`` / ``backtest_rows`` on a model without a device: each refusal comes back as a ValueError, so it was raised
    before the device was asked for (which would be a PfoError here)."""
    tables = P.InvestTables.__new__(P.InvestTables)
    tables.upper_u = 4
    log = (np.array([1, 2, 3]), np.array([6, 7, 8]), np.array([1.0, 2.0, 3.0]), np.array([1, 2, 3]))

    def call(mv=None, portfolios=None, day_idx=None, holdings=None, **kw):
        tgn = types.SimpleNamespace(holdings=holdings, device="cpu")
        for fn in (BT.backtest_rows, BT.backtest):
            try:
                fn(tgn, *log, np.arange(5, 25), 3, cutoffs=(1, 3), batch_size=2, tables=tables, mv=mv, portfolios=portfolios, **kw)
            except ValueError as e:
                err = e
            else:
                raise AssertionError("not refused")
        raise err
    _refusals(call)
    if not torch.cuda.is_available():
        tgn = types.SimpleNamespace(holdings=None, device="cpu")
        with pytest.raises(_lib.PfoError):                              # valid: the walk gets as far as asking for the device
            BT.backtest(tgn, *log, np.arange(5, 25), 3, cutoffs=(1, 3), batch_size=2, tables=tables, groups=G, group_cap=2,
                        held_groups=[[0], [], [1, 1]])


def test_the_keywords_go_by_name_only_and_sit_where_they_were():
    for fn in (P.TGN.recommend, BT.backtest, BT.backtest_rows, RC.validate):
        p = inspect.signature(fn).parameters
        assert p["held_groups"].kind is p["stock_groups"].kind is inspect.Parameter.KEYWORD_ONLY
        assert p["held_groups"].default is None and p["stock_groups"].default is None
    for fn in (P.recommend_topk, P.recommend_mv_topk, P.recommend_basket_topk):
        names = list(inspect.signature(fn).parameters)
        assert names[-4:] == ["cand_group", "group_cap", "held_group", "held_len"]


def test_stock_rows_to_groups_on_the_host():
    """The mapping of ``held_groups="held"`` / ``"portfolios"`` (torch operations; here on the CPU): an index outside
    ``stock_groups`` - the padding too - gives -1."""
    idx = torch.tensor([[0, 3, -1, 7], [2, 2, 9, -5]], dtype=torch.int32)
    sg = torch.tensor([5, -1, 6, 7], dtype=torch.int32)
    assert RC.stock_rows_to_groups(idx, sg).tolist() == [[5, 7, -1, -1], [6, 6, -1, -1]]
    assert RC.stock_rows_to_groups(idx, sg[:0]).tolist() == [[-1] * 4] * 2
    assert RC.stock_rows_to_groups(idx[:, :0], sg).shape == (2, 0)
