"""Host side of the group caps (``pfo_recommend_*_topk_capped`` / ``TGN.recommend(groups=, group_cap=)``): the numpy reference
(``recommend_capped_ref``) against a brute-force greedy and against its two reformulations the kernels rest on, the header and
the ctypes table against the uncapped siblings, every bound of the three entries refused without a device, every ValueError of
``recommend.validate`` and of ``backtest``'s check, and the condition the GPU test's plain cases rest on, from their inputs alone."""
import importlib
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

BT = importlib.import_module("pfotgnrec_amd.backtest")    # (the package's ``backtest`` is the function)

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pfotgn.h")


# ---------------------------------------------------------------------------------------------- the reference

def _small(rs):
    """A small random row: scores with ties (and both zeros), a mask, groups with groupless candidates, a cap and a depth."""
    I = int(rs.randint(1, 41))
    scores = rs.randint(-3, 4, I).astype(np.float64)
    scores[rs.rand(I) < 0.1] = -0.0
    adm = rs.rand(I) > 0.2
    groups = rs.randint(-1, int(rs.randint(1, 6)), I).astype(np.int32)
    return I, scores, adm, groups, int(rs.randint(1, 4)), int(rs.randint(1, 12))


def _brute_force(scores, adm, groups, cap, k):
    """The greedy list by definition: again and again the best candidate left that may still be taken (score descending, the
    larger position first among equal scores), until k are taken or none may be."""
    left = [c for c in range(len(scores)) if adm[c]]
    taken = []
    while len(taken) < k:
        may = [c for c in left if groups[c] < 0 or sum(groups[t] == groups[c] for t in taken) < cap]
        if not may:
            break
        best = max(may, key=lambda c: (scores[c], c))
        taken.append(best)
        left.remove(best)
    return taken


def test_the_walk_is_the_brute_force_greedy():
    rs = np.random.RandomState(0)
    for _ in range(600):
        I, scores, adm, groups, cap, k = _small(rs)
        pos, sc, n = C.topk_capped(scores[None], adm[None], groups, cap, k)
        want = _brute_force(scores, adm, groups, cap, k)
        assert pos[0, :n[0]].tolist() == want and n[0] == len(want) and (pos[0, n[0]:] == -1).all() and np.isneginf(sc[0, n[0]:]).all()
        assert not np.signbit(sc[0, :n[0]][sc[0, :n[0]] == 0]).any(), "a zero score is +0"


def test_count_form_and_chunk_form_are_the_walk():
    """The two reformulations of the module docstring of ``recommend_capped_ref``, over random small cases with ties, masks and
    groupless candidates; the chunk form at every chunk size from 1 to 20 and with the positions in their natural order - the
    order the kernel meets them in."""
    rs = np.random.RandomState(1)
    for _ in range(400):
        I, scores, adm, groups, cap, k = _small(rs)
        order = R.canonical_order(scores)
        order = order[adm[order]]
        walk = C.capped_walk(order, groups, cap, k)
        assert np.array_equal(C.survivors(order, groups, cap)[:k], walk)
        place = np.empty(I, np.int64)
        place[R.canonical_order(scores)] = np.arange(I)
        for chunk in range(1, 21):
            assert np.array_equal(C.chunked(place, np.flatnonzero(adm), groups, cap, k, chunk), walk), chunk


def test_n_valid_formula():
    rs = np.random.RandomState(2)
    for _ in range(400):
        I, scores, adm, groups, cap, k = _small(rs)
        _, _, n = C.topk_capped(scores[None], adm[None], groups, cap, k)
        assert n[0] == C.n_valid_formula(adm, groups, cap, k)
    for name in C.PLAIN_CASES:
        c, groups, cap, k, _ = C.plain_case(name)
        ref = C.reference_topk(c, groups, cap, k)
        assert ref["n_valid"].tolist() == [C.n_valid_formula(ref["adm"][u], groups, cap, k) for u in range(len(ref["n_valid"]))]


@pytest.mark.parametrize("spec", B.CASES[:3] + B.CASES[4:], ids=lambda s: "seed%d" % s[0])
def test_a_cap_that_cannot_bind_gives_the_uncapped_reference(spec):
    """cap >= k, no candidate in a group, and every candidate in a group of its own: the three orders' uncapped references."""
    c, (seed, U, I, D, k, n_t, n_ret, W) = B.case(spec), spec
    s64 = R.scores64(c["user_emb"], c["item_emb"], c["user_block"], I)
    plain = R.topk(s64, R.admissible(U, I, c["excl_pos"], c["excl_len"], c["item_ok"]), k)
    mv, bk = M.reference(c, 0.5, k), B.reference(c, 0.5, k)
    for groups, cap in ((C.groups_of(seed, I, 3), k), (np.full(I, -1, np.int32), 1), (np.arange(I, dtype=np.int32)[::-1] * 7, 1)):
        got = C.reference_topk(c, groups, cap, k)
        assert all(np.array_equal(got[n], w) for n, w in zip(("top_pos", "top_score", "n_valid"), plain))
        assert B.same(C.reference_mv(c, 0.5, groups, cap, k, y=mv["y_raw"]), mv)
        assert B.same(C.reference_basket(c, 0.5, groups, cap, k), bk)


@pytest.mark.parametrize("spec", B.CASES[:3] + B.CASES[4:], ids=lambda s: "seed%d" % s[0])
def test_the_capped_basket_is_the_loop_of_single_picks(spec):
    """The composition the one launch replaces, run over the reference itself: k uncapped single picks, the exclusion row
    growing by the pick and, when its group fills, by the rest of the group.  And the cap shows: lists change."""
    c, (seed, U, I, D, k, n_t, n_ret, W) = B.case(spec), spec
    for n_groups, cap in C.MV_CAPS:
        groups = C.groups_of(seed, I, n_groups)
        for lam in B.LAMBDAS:
            got = C.reference_basket(c, lam, groups, cap, k)
            assert B.same(got, C.loop_of_single_picks_capped(c, groups, cap, k, lambda cc: M.reference(cc, lam, 1))), (n_groups, cap, lam)
            for u in range(U):                                          # the cap holds, picks are distinct
                p = got["top_pos"][u, :got["n_valid"][u]]
                g = groups[p]
                assert len(set(p.tolist())) == len(p) and all(int((g == v).sum()) <= cap for v in np.unique(g[g >= 0]))
            if (n_groups, cap) == (3, 1):                               # (k >= 4 picks, at most three of them in a group)
                assert (got["top_pos"] != B.reference(c, lam, k)["top_pos"]).any(), "the cap must move a list"


def test_the_capped_mean_variance_list_keeps_the_uncapped_values():
    spec = B.CASES[2]
    c, (seed, U, I, D, k, n_t, n_ret, W) = B.case(spec), spec
    groups = C.groups_of(seed, I, 3)
    plain, got = M.reference(c, 0.5, k), C.reference_mv(c, 0.5, groups, 1, k)
    assert np.array_equal(got["fused"], plain["fused"], equal_nan=True)
    changed = 0
    for u in range(U):
        n = got["n_valid"][u]
        p = got["top_pos"][u, :n]
        assert n == C.n_valid_formula(got["adm"][u], groups, 1, k)
        assert np.array_equal(got["top_fused"][u, :n], plain["fused"][u, p])
        assert np.array_equal(C.survivors(M.fuse(R.scores64(c["user_emb"], c["item_emb"], c["user_block"], I)[u][None], got["y_raw"][u][None],
                                                 got["adm"][u][None], 0.5, I)[0][0, :int(got["adm"][u].sum())], groups, 1)[:k], p)
        changed += int(not np.array_equal(got["top_pos"][u], plain["top_pos"][u]))
    assert changed >= U // 2


# ---------------------------------------------------------------------------------------------- the C ABI

def _declaration(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^(\w+) %s\(([^;]*)\);" % name, text, re.M)
    assert m, "%s is not declared in include/pfotgn.h" % name
    return m.group(1), [a.strip() for a in m.group(2).replace("\n", " ").split(",")]


SIBLINGS = ("pfo_recommend_topk", "pfo_recommend_mv_topk", "pfo_recommend_basket_topk")


@pytest.mark.parametrize("sibling", SIBLINGS)
def test_header_and_ctypes_table(sibling):
    """The sibling's parameter list with (cand_group, group_cap) directly behind item_ok and nothing else changed - in the
    header and in the ctypes table; the siblings themselves keep their signatures and the abi its number."""
    ret, old = _declaration(sibling)
    ret_c, new = _declaration(sibling + "_capped")
    at = old.index("const uint8_t* item_ok") + 1
    assert at == 11 and ret == ret_c == "int"
    assert new == old[:at] + ["const int32_t* cand_group", "int32_t group_cap"] + old[at:]
    (res, args), (res_c, args_c) = _lib.PROTOTYPES[sibling], _lib.PROTOTYPES[sibling + "_capped"]
    assert res is res_c and args_c == args[:at] + [_lib._VP, _lib.C.c_int32] + args[at:] and len(args_c) == len(new)
    assert len(old) == {"pfo_recommend_topk": 16, "pfo_recommend_mv_topk": 31, "pfo_recommend_basket_topk": 28}[sibling]
    lib = _lib.load()
    assert hasattr(lib, sibling + "_capped") and lib.pfo_abi_version() == 6


def _plain_args(U=3, I=10, n_t=1, D=8, excl_stride=0, k=3, group_cap=1):
    return ("pfo_recommend_topk_capped", None, None, None, U, I, n_t, D, None, None, excl_stride, None, None, group_cap, k, None, None, None,
            None)


def _mv_args(symbol, tail):
    def args(U=3, I=10, n_t=1, D=8, excl_stride=0, k=3, group_cap=1, n_ret=29, port_stride=0, n_days=2, n_stocks=5):
        return (symbol, None, None, None, U, I, n_t, D, None, None, excl_stride, None, None, group_cap, None, None, n_days, n_stocks, n_ret,
                None, None, None, port_stride, 2.0, 0.5, k) + (None,) * tail
    return args


ENTRIES = {"plain": (_plain_args, 65536), "mv": (_mv_args("pfo_recommend_mv_topk_capped", 8), 2048),
           "basket": (_mv_args("pfo_recommend_basket_topk_capped", 5), 2048)}
BOUNDS = [(dict(D=6), "D must be a positive multiple of 4"), (dict(D=0), "D must be a positive multiple of 4"),
          (dict(D=260), "D must be at most 256"), (dict(k=0), "k must be in"), (dict(k=65), "k must be in"), (dict(I=0), "I must be in"),
          (dict(n_t=0), "n_t must be at least 1"), (dict(excl_stride=-1), "must not be negative"),
          (dict(group_cap=0), "group_cap must be at least 1"), (dict(group_cap=-3), "group_cap must be at least 1")]
MV_BOUNDS = [(dict(n_ret=1), "n_ret must be in"), (dict(n_ret=129), "n_ret must be in"), (dict(port_stride=-1), "must not be negative"),
             (dict(n_days=0), "must be positive"), (dict(n_stocks=0), "must be positive")]


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_every_bound_is_refused_before_a_pointer_is_looked_at(entry):
    """All pointers are NULL: a refusal that names the bound shows the bound was checked first, with and without users.
    Nothing is queued (no device is needed for any of this)."""
    args, max_items = ENTRIES[entry]
    for kw, msg in BOUNDS + [(dict(I=max_items + 1), "I must be in")] + (MV_BOUNDS if entry != "plain" else []):
        for U in (3, 0):
            with pytest.raises(_lib.PfoError, match=msg):
                _lib.call(*args(U=U, **kw))
    # every bound kept: the NULL pointers are what is left to refuse
    with pytest.raises(_lib.PfoError, match="null"):
        _lib.call(*args())
    with pytest.raises(_lib.PfoError, match="null"):
        _lib.call(*args(I=max_items, D=256, k=64, group_cap=2 ** 31 - 1))
    # U == 0: accepted, no pointer is looked at
    _lib.call(*args(U=0))
    _lib.call(*args(U=0, I=max_items, D=256, k=64, group_cap=64))


def test_a_null_cand_group_is_refused_by_name():
    """Every other pointer given (host memory: nothing is launched before the refusal), cand_group NULL."""
    buf = (_lib.C.c_char * 4096)()
    p = _lib.C.addressof(buf)
    p += -p % 16
    with pytest.raises(_lib.PfoError, match="pfo_recommend_topk_capped: null cand_group"):
        _lib.call("pfo_recommend_topk_capped", p, p, None, 3, 10, 1, 8, None, None, 0, None, None, 1, 3, p, p, None, None)
    for symbol, tail in (("pfo_recommend_mv_topk_capped", (p, p, p, None, None, None, None, None)),
                         ("pfo_recommend_basket_topk_capped", (p, p, p, None, None))):
        with pytest.raises(_lib.PfoError, match=symbol + ": null cand_group"):
            _lib.call(symbol, p, p, None, 3, 10, 1, 8, None, None, 0, None, None, 1, p, p, 2, 5, 29, p, None, None, 0, 2.0, 0.5, 3, *tail)


# ---------------------------------------------------------------------------------------------- the functional forms

def test_the_functional_forms_validate_then_require_a_gpu():
    ue, ie = torch.zeros(3, 8), torch.zeros(10, 8)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    mv = dict(cand_stock=i32(10), returns=torch.zeros(2, 5, 29, dtype=torch.float64), day_idx=i32(3), port_idx=None, port_len=None,
              gamma=2.0, lambda_mv=0.5)
    forms = ((P.recommend_topk, dict(user_emb=ue, item_emb=ie, k=3)), (P.recommend_mv_topk, dict(user_emb=ue, item_emb=ie, k=3, **mv)),
             (P.recommend_basket_topk, dict(user_emb=ue, item_emb=ie, k=3, **mv)))
    for fn, good in forms:
        for kw in (dict(cand_group=i32(10)), dict(group_cap=2), dict(cand_group=i32(9), group_cap=2), dict(cand_group=i32(10), group_cap=0),
                   dict(cand_group=i32(10), group_cap=1.5), dict(cand_group=torch.zeros(10, dtype=torch.int64), group_cap=1),
                   dict(cand_group=i32(2, 5), group_cap=1), dict(cand_group=[0] * 10, group_cap=1)):
            with pytest.raises(ValueError):
                fn(**dict(good, **kw))
        if not torch.cuda.is_available():
            with pytest.raises(_lib.PfoError):                          # valid: only the device is missing - no fallback
                fn(cand_group=i32(10), group_cap=2, **good)
    for fn in (P.recommend_mv_topk_wide, P.recommend_list_topk, P.recommend_list_mv_topk):
        with pytest.raises(TypeError):                                  # the wide and the list forms take no cap
            fn(ue, ie, 3, cand_group=i32(10), group_cap=1)


# ---------------------------------------------------------------------------------------------- validate and backtest

def _mv_object():
    return types.SimpleNamespace(returns=np.zeros((2, 30, 3)), upper_u=4, gamma=2.0, lambda_mv=0.5, day_of=None)


def _validate(I=20, **kw):
    return RC.validate(I + 10, None, [1, 2, 3], 5.0, 3, np.arange(5, I + 5), kw.pop("exclude", None), None, None, **kw)


def test_validate_takes_groups_in_every_form():
    q = _validate()
    assert q.groups is None and q.group_cap is None and q._fields[-1] == "basket", "without the keywords the query is the one it was"
    g = np.arange(20) % 3 - 1
    q = _validate(groups=g.tolist(), group_cap=2)
    assert q.groups.dtype == np.int32 and q.groups.tolist() == g.tolist() and q.group_cap == 2
    q = _validate(groups=g.astype(np.int64) * (2 ** 31 - 1), group_cap=np.int64(64))
    assert q.groups.dtype == np.int32 and q.groups.max() == 2 ** 31 - 1 and q.group_cap == 64 and type(q.group_cap) is int
    t = torch.from_numpy(g)
    q = _validate(groups=t, group_cap=1)
    assert q.groups is t
    mv = _mv_object()
    for kw in (dict(), dict(basket=True)):
        q = _validate(I=2048, groups=np.zeros(2048, np.int16), group_cap=1, mv=mv, portfolios=[[], [], []], day_idx=0, **kw)
        assert q.groups.shape == (2048,) and q.mv is not None
    assert _validate(I=5000, groups=np.zeros(5000, np.int32), group_cap=1).I == 5000      # the score order has no 2048


def _refusals(call, I=20):
    """Every ValueError the issue lists, through ``call(I=..., **keywords)``."""
    g = np.zeros(I, np.int32)
    for kw, msg in ((dict(groups=g), "go together"), (dict(group_cap=2), "go together"),
                    (dict(groups=g[:-1], group_cap=2), "groups holds %d entries" % (I - 1)), (dict(groups=np.zeros((I, 1), np.int32), group_cap=2), "one integer per candidate"),
                    (dict(groups=g.astype(np.float64), group_cap=2), "one integer per candidate"),
                    (dict(groups=[0.5] * I, group_cap=2), "one integer per candidate"), (dict(groups=g != 0, group_cap=2), "one integer per candidate"),
                    (dict(groups=torch.zeros(I), group_cap=2), "one integer per candidate"),
                    (dict(groups=["a"] * I, group_cap=2), "one integer per candidate"),
                    (dict(groups=np.full(I, 2 ** 31, np.int64), group_cap=2), "do not fit 32 bits"),
                    (dict(groups=np.full(I, -2 ** 31 - 1, np.int64), group_cap=2), "do not fit 32 bits"),
                    (dict(groups=g, group_cap=0), "group_cap must be at least 1"), (dict(groups=g, group_cap=-1), "group_cap must be at least 1"),
                    (dict(groups=g, group_cap=1.0), "group_cap must be an integer"), (dict(groups=g, group_cap="2"), "group_cap must be an integer")):
        with pytest.raises(ValueError, match=msg):
            call(I=I, **kw)
    mv = _mv_object()
    with pytest.raises(ValueError, match="the capped order has no wide form"):
        call(I=2049, groups=np.zeros(2049, np.int32), group_cap=1, mv=mv, portfolios=[[], [], []], day_idx=0)


def test_validate_refuses_what_groups_cannot_be():
    _refusals(_validate)
    g = np.zeros(20, np.int32)
    with pytest.raises(ValueError, match="the list forms have no capped order"):
        _validate(groups=g, group_cap=1, only=[[5], [6], [7]])
    with pytest.raises(ValueError, match="the list forms have no capped order"):
        _validate(groups=g, group_cap=1, only="held", holdings=types.SimpleNamespace(upper_u=4))


def test_backtest_makes_the_same_checks_before_any_device_work():
    """``backtest`` / ``backtest_rows`` on a model without a device: each refusal of ``validate`` comes back as a ValueError,
    so it was raised before the device was asked for (which would be a PfoError here)."""
    tgn = types.SimpleNamespace(holdings=None, device="cpu")
    tables = P.InvestTables.__new__(P.InvestTables)
    tables.upper_u = 4
    log = (np.array([1, 2, 3]), np.array([6, 7, 8]), np.array([1.0, 2.0, 3.0]), np.array([1, 2, 3]))

    def call(I, mv=None, portfolios=None, day_idx=None, **kw):
        for fn in (BT.backtest_rows, BT.backtest):
            try:
                fn(tgn, *log, np.arange(5, I + 5), 3, cutoffs=(1, 3), batch_size=2, tables=tables, mv=mv, portfolios=portfolios, **kw)
            except ValueError as e:
                err = e
            else:
                raise AssertionError("not refused")
        raise err
    _refusals(call)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.PfoError):                              # valid: the walk gets as far as asking for the device
            BT.backtest(tgn, *log, np.arange(5, 25), 3, cutoffs=(1, 3), batch_size=2, tables=tables, groups=np.zeros(20, np.int32), group_cap=2)


def test_recommend_and_backtest_take_the_keywords_by_name_only():
    import inspect
    for fn in (P.TGN.recommend, BT.backtest, BT.backtest_rows, RC.validate):
        p = inspect.signature(fn).parameters
        assert p["groups"].kind is p["group_cap"].kind is inspect.Parameter.KEYWORD_ONLY and p["groups"].default is None
    names = list(inspect.signature(P.TGN.recommend).parameters)
    assert names[-3:] == ["only", "groups", "group_cap"]


# ---------------------------------------------------------------------------------------------- what the GPU test rests on

BINDING = {"A": (13, 20, 0), "B": (37, 37, None), "C": (20, 20, None), "E": (9, 9, 9), "F": (33, 33, None)}


@pytest.mark.parametrize("name", sorted(C.PLAIN_CASES))
def test_the_cap_binds_in_the_plain_cases(name):
    """In each plain exact case of the GPU test the cap changes the list of at least half of the users, by the reference alone -
    the counts of the issue; in E every list ends short of min(k, #admissible)."""
    c, groups, cap, k, n_t = C.plain_case(name)
    changed, short = C.binding(c, groups, cap, k)
    U = c["user_emb"].shape[0]
    print("FIGURES case %s: the cap changes %d of %d lists, %d end short" % (name, changed, U, short))
    want_changed, want_U, want_short = BINDING[name]
    assert U == want_U and changed == want_changed and 2 * changed >= U
    assert want_short is None or short == want_short
    assert (groups < 0).any() and (groups >= 0).any()


def test_the_case_the_issue_rules_out_does_not_bind():
    c = R.exact_case(6, 17, 300, 32, 8, 3)
    assert C.binding(c, C.groups_of(6, 300, 8), 3, 8)[0] == 2
