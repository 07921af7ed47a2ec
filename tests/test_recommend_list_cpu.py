"""Host side of the list forms of the top-k recommendation (``pfo_recommend_list_topk`` / ``pfo_recommend_list_mv_topk`` /
``TGN.recommend(only=...)``): the numpy reference against the shared-list one, header and ctypes table, every bound of the two
entries refused without a device, ``validate(only=...)``, the dispatcher ops' fakes, and the condition the GPU test's normal
cases rest on, computed from their inputs alone."""
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
import recommend_list_ref as L

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pfotgn.h")


# ---------------------------------------------------------------------------------------------- the reference

@pytest.mark.parametrize("seed,U,I,W", [(1, 9, 17, 8), (2, 30, 300, 64), (3, 5, 1, 1), (4, 12, 40, 65)])
def test_the_list_and_its_complement_say_the_same(seed, U, I, W):
    """``admissible_list`` is ``recommend_ref.admissible`` with every position the list does not name as the exclusion list -
    so the shared-list kernels with that exclusion list are a second statement of what the list kernels must return."""
    c = L.list_case(R.exact_case(seed, U, I, 8, 5, 1), seed, W)
    adm = L.admissible_list(U, I, c["list_pos"], c["list_len"], c["item_ok"])
    excl_pos, excl_len = L.complement(U, I, c["list_pos"], c["list_len"])
    assert np.array_equal(adm, R.admissible(U, I, excl_pos, excl_len, c["item_ok"]))
    assert np.array_equal(L.admissible_list(U, I, c["list_pos"], c["list_len"]), R.admissible(U, I, excl_pos, excl_len))


def test_the_generator_keeps_its_promises():
    """Padding inside the counted length, positions beyond I, a repeat, a length past the row, an empty list."""
    U, I, W = 300, 17, 8
    c = L.list_case(R.exact_case(7, U, I, 4, 5, 1), 7, W)
    lp, ll = c["list_pos"], c["list_len"]
    counted = np.arange(W)[None, :] < ll[:, None]
    assert (lp[counted] == -1).any() and (lp >= I).any() and (ll > W).any() and (ll == 0).any()
    assert any(ll[u] >= 2 and lp[u, 0] == lp[u, 1] >= 0 for u in range(U))
    assert c["excl_pos"] is None and c["excl_len"] is None and c["I"] == I


def test_a_duplicate_changes_neither_the_set_nor_a_rank():
    U, I, W, k = 9, 40, 16, 6
    c = L.list_case(M.exact_case(3, U, I, 8, k, 1, 5), 3, W)
    once = dict(c, list_pos=np.full((U, W), -1, np.int32), list_len=np.zeros(U, np.int32))
    for u in range(U):
        row = L.list_rows(c["list_pos"], c["list_len"], u)
        _, first = np.unique(row, return_index=True)
        row = row[np.sort(first)]
        once["list_pos"][u, :len(row)] = row
        once["list_len"][u] = len(row)
    assert (once["list_len"] < np.minimum(c["list_len"], W)).any(), "the case must hold duplicates"
    a, b = L.reference_mv(c, 0.5, k), L.reference_mv(once, 0.5, k)
    for name in ("top_pos", "top_score", "top_fused", "n_valid", "adm"):
        assert np.array_equal(a[name], b[name]), name
    assert np.array_equal(np.isnan(a["fused"]), np.isnan(b["fused"])) and np.array_equal(a["fused"][a["adm"]], b["fused"][b["adm"]])
    # by slot: a value in the first occurrence only
    first = L.first_slots(c, a["adm"])
    assert np.array_equal(~np.isnan(a["fused_slot"]), first) and first.sum() == a["adm"].sum()
    s, t = L.reference(c, k), L.reference(once, k)
    assert all(np.array_equal(s[n], t[n]) for n in ("top_pos", "top_score", "n_valid"))


def test_reference_on_a_hand_made_case():
    ue = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]], np.float32)
    ie = np.array([[3.0, 0.0], [2.0, 5.0], [3.0, 1.0], [0.0, 0.0]], np.float32)             # scores: u0 3 2 3 0, u1 0 5 1 0, u2 3 7 4 0
    c = dict(user_emb=ue, item_emb=ie, user_block=None, item_ok=np.array([1, 1, 1, 0], np.uint8), I=4,
             list_pos=np.array([[0, 2, 2, 3, -1], [1, 7, 0, -1, -1], [3, 3, -1, -1, -1]], np.int32), list_len=np.array([9, 2, 2], np.int32))
    ref = L.reference(c, 3)
    assert ref["top_pos"].tolist() == [[2, 0, -1], [1, -1, -1], [-1, -1, -1]]                # equal scores: the larger position first
    assert ref["top_score"].tolist() == [[3.0, 3.0, -np.inf], [5.0, -np.inf, -np.inf], [-np.inf] * 3]
    assert ref["n_valid"].tolist() == [2, 1, 0]
    assert np.array_equal(np.isnan(ref["score"]), ~np.array([[1, 1, 0, 0, 0], [1, 0, 0, 0, 0], [0, 0, 0, 0, 0]], bool))


# ---------------------------------------------------------------------------------------------- the C ABI

def _declaration(name):
    text = open(HEADER).read()
    m = re.search(r"^(\w+) %s\(([^;]*)\);" % name, text, re.M)
    assert m, "%s is not declared" % name
    return m.group(1), [a.strip() for a in m.group(2).replace("\n", " ").split(",")]


def test_header_and_ctypes_table():
    ret, plain = _declaration("pfo_recommend_list_topk")
    _, old = _declaration("pfo_recommend_topk")
    assert ret == "int" and len(plain) == 17
    assert plain[:7] == old[:7] and plain[10:15] == old[10:15]
    assert plain[7:10] == ["const int32_t* list_pos", "const int32_t* list_len", "int32_t list_stride"]
    assert plain[15:] == ["float* score_out", "void* stream"]
    _, mv = _declaration("pfo_recommend_list_mv_topk")
    _, old_mv = _declaration("pfo_recommend_mv_topk")
    assert len(mv) == len(old_mv) == 31 and mv[:7] == old_mv[:7] and mv[10:] == old_mv[10:] and mv[7:10] == plain[7:10]
    assert re.search(r"#define PFO_RECOMMEND_LIST_MAX_WIDTH\s+256\b", open(HEADER).read())
    assert _lib.RECOMMEND_LIST_MAX_WIDTH == 256
    assert len(_lib.PROTOTYPES["pfo_recommend_list_topk"][1]) == 17
    assert _lib.PROTOTYPES["pfo_recommend_list_mv_topk"] == _lib.PROTOTYPES["pfo_recommend_mv_topk"]
    lib = _lib.load()
    assert hasattr(lib, "pfo_recommend_list_topk") and hasattr(lib, "pfo_recommend_list_mv_topk")
    assert lib.pfo_abi_version() == 6
    assert P.recommend_list_topk is P.functional.recommend_list_topk and P.recommend_list_mv_topk is P.functional.recommend_list_mv_topk


def _plain_args(U=3, I=10, n_t=1, D=8, list_stride=4, k=3):
    return ("pfo_recommend_list_topk", None, None, None, U, I, n_t, D, None, None, list_stride, None, k, None, None, None, None, None)


def _mv_args(U=3, I=10, n_t=1, D=8, list_stride=4, k=3, n_ret=29, port_stride=0):
    return ("pfo_recommend_list_mv_topk", None, None, None, U, I, n_t, D, None, None, list_stride, None, None, None, 2, 5, n_ret, None, None,
            None, port_stride, 2.0, 0.5, k, None, None, None, None, None, None, None, None)


BOUNDS = [(dict(D=6), "D must be a positive multiple of 4"), (dict(D=0), "D must be a positive multiple of 4"),
          (dict(D=260), "D must be at most 256"), (dict(k=0), "k must be in"), (dict(k=65), "k must be in"), (dict(I=0), "I must be in"),
          (dict(I=65537), "I must be in"), (dict(n_t=0), "n_t must be at least 1"), (dict(list_stride=0), "list_stride must be in"),
          (dict(list_stride=257), "list_stride must be in")]


@pytest.mark.parametrize("args", [_plain_args, _mv_args], ids=["plain", "mv"])
def test_every_bound_is_refused_before_a_pointer_is_looked_at(args):
    """All pointers are NULL: a refusal that names the bound shows the bound was checked first.  Nothing is queued (no device
    is needed for any of this)."""
    bounds = list(BOUNDS)
    if args is _mv_args:
        bounds += [(dict(n_ret=1), "n_ret must be in"), (dict(n_ret=129), "n_ret must be in"), (dict(port_stride=-1), "must not be negative")]
    for kw, msg in bounds:
        for U in (3, 0):
            with pytest.raises(_lib.PfoError, match=msg):
                _lib.call(*args(U=U, **kw))
    # every bound kept: the NULL pointers are what is left to refuse
    with pytest.raises(_lib.PfoError, match="null"):
        _lib.call(*args())
    # the largest of everything passes the bounds too, and I has no 2048 here
    with pytest.raises(_lib.PfoError, match="null"):
        _lib.call(*args(I=65536, D=256, k=64, list_stride=256))
    # U == 0: accepted, no pointer is looked at
    _lib.call(*args(U=0))
    _lib.call(*args(U=0, I=65536, D=256, k=64, list_stride=256))


# ---------------------------------------------------------------------------------------------- validate(only=...)

def _validate(only, U=3, I=20, **kw):
    return RC.validate(I + 10, None, list(range(1, U + 1)), 5.0, 3, np.arange(5, I + 5), kw.pop("exclude", None), None, None, only=only, **kw)


def test_validate_takes_every_form_of_only():
    q = _validate(None)
    assert q.only_ids is None and q.only_len is None and not q.only_held, "without only the query is the one it was"
    q = _validate([[5, 6, 6], [], [999999, 7]])
    assert q.only_ids.tolist() == [[5, 6, 6], [-1, -1, -1], [999999, 7, -1]] and q.only_len.tolist() == [3, 0, 2] and not q.only_held
    assert q.ex_ids is None and q.held is None
    q = _validate([[], [], []])
    assert q.only_ids.shape == (3, 0)
    ids, lens = np.array([[5, -1], [6, 7], [-1, -1]], np.int32), np.array([1, 2, 0], np.int32)
    q = _validate((ids, lens))
    assert q.only_ids is ids and q.only_len is lens
    q = _validate((torch.from_numpy(ids), torch.from_numpy(lens)))
    assert isinstance(q.only_ids, torch.Tensor) and isinstance(q.only_len, torch.Tensor)
    q = _validate((np.zeros((3, 256), np.int32), np.zeros(3, np.int32)))
    assert q.only_ids.shape == (3, 256)
    ledger = types.SimpleNamespace(upper_u=4)
    q = _validate("held", holdings=ledger)
    assert q.only_held and q.only_ids is None and q.held is None
    mv = types.SimpleNamespace(returns=np.zeros((2, 30, 3)), upper_u=4, gamma=2.0, lambda_mv=0.5, day_of=None)
    q = _validate("held", holdings=ledger, mv=mv, portfolios="held", day_idx=0)
    assert q.only_held and q.held == (False, True) and q.mv.port_idx is None
    # with mv the list form takes any I the plain kernel takes
    q = _validate([[5], [6], [7]], I=5000, mv=mv, portfolios=[[], [], []], day_idx=0)
    assert q.I == 5000 and q.mv is not None and q.only_ids.shape == (3, 1)


def test_validate_refuses_what_only_cannot_be():
    ledger = types.SimpleNamespace(upper_u=4)
    mv = types.SimpleNamespace(returns=np.zeros((2, 30, 3)), upper_u=4, gamma=2.0, lambda_mv=0.5, day_of=None)
    with pytest.raises(ValueError, match="only and exclude"):
        _validate([[5], [6], [7]], exclude=[[5], [], []])
    with pytest.raises(ValueError, match="only and exclude"):
        _validate("held", exclude="held", holdings=ledger)
    with pytest.raises(ValueError, match="only and basket"):
        _validate([[5], [6], [7]], basket=True, mv=mv, portfolios=[[], [], []], day_idx=0)
    with pytest.raises(ValueError, match="at most 256"):
        _validate([list(range(5, 25)) * 13, [], []])                                    # 260 entries: 257 and beyond
    with pytest.raises(ValueError, match="at most 256"):
        _validate([[5] * 257, [], []])
    with pytest.raises(ValueError, match="at most 256"):
        _validate((np.zeros((3, 257), np.int32), np.zeros(3, np.int32)))
    with pytest.raises(ValueError, match="track_holdings"):
        _validate("held")
    with pytest.raises(ValueError, match="only lists 2 users"):
        _validate([[5], [6]])
    with pytest.raises(ValueError, match="U = 3"):
        _validate((np.zeros((2, 4), np.int32), np.zeros(2, np.int32)))
    with pytest.raises(ValueError, match="U = 3"):
        _validate((np.zeros((3, 4), np.int32), np.zeros(2, np.int32)))
    with pytest.raises(ValueError, match="integers"):
        _validate((np.zeros((3, 4), np.float32), np.zeros(3, np.int32)))
    with pytest.raises(ValueError):
        _validate("mine")
    with pytest.raises(ValueError):
        _validate(7)


def test_the_functional_forms_validate_then_require_a_gpu():
    ue, ie = torch.zeros(3, 8), torch.zeros(10, 8)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    good = dict(user_emb=ue, item_emb=ie, k=3, list_pos=i32(3, 4), list_len=i32(3))
    good_mv = dict(good, cand_stock=i32(10), returns=torch.zeros(2, 5, 29, dtype=torch.float64), day_idx=i32(3), port_idx=i32(3, 4),
                   port_len=i32(3), gamma=2.0, lambda_mv=0.5)
    bad = (dict(k=0), dict(k=65), dict(list_pos=i32(2, 4)), dict(list_pos=i32(3, 0)), dict(list_pos=i32(3, 257)), dict(list_pos=None),
           dict(list_pos=torch.zeros(3, 4, dtype=torch.int64)), dict(list_len=i32(2)), dict(list_len=torch.zeros(3, dtype=torch.int64)),
           dict(user_block=i32(2)), dict(item_ok=torch.ones(4, dtype=torch.uint8)), dict(user_emb=torch.zeros(3, 6)), dict(user_emb=ue.double()))
    for kw in bad:
        with pytest.raises(ValueError):
            P.recommend_list_topk(**dict(good, **kw))
        with pytest.raises(ValueError):
            P.recommend_list_mv_topk(**dict(good_mv, **kw))
    for kw in (dict(cand_stock=i32(9)), dict(returns=torch.zeros(2, 5, 1, dtype=torch.float64)), dict(day_idx=i32(2)), dict(port_idx=i32(2, 4)),
               dict(port_len=i32(2)), dict(port_idx=None), dict(n_blocks=3)):
        with pytest.raises(ValueError):
            P.recommend_list_mv_topk(**dict(good_mv, **kw))
    if not torch.cuda.is_available():
        with pytest.raises(_lib.PfoError):
            P.recommend_list_topk(**good)
        with pytest.raises(_lib.PfoError):
            P.recommend_list_mv_topk(**good_mv)
        with pytest.raises(_lib.PfoError):                                              # beyond 2048 candidates: no ValueError
            P.recommend_list_mv_topk(ue, torch.zeros(2500, 8), 3, i32(3, 4), None, i32(2500), torch.zeros(2, 5, 3, dtype=torch.float64), i32(3),
                                     None, None, 2.0, 0.5)


def test_dispatcher_op_fakes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        ue, ie, lp = torch.empty(7, 8), torch.empty(6000, 8), torch.empty(7, 33, dtype=torch.int32)
        plain = torch.ops.pfotgn.recommend_list_topk(ue, ie, 5, lp, None, 2)
        mv = torch.ops.pfotgn.recommend_list_mv_topk(ue, ie, 5, lp, torch.empty(3000, dtype=torch.int32), torch.empty(2, 5, 29, dtype=torch.float64),
                                                     torch.empty(7, dtype=torch.int32), 2.0, 0.5, torch.empty(7, dtype=torch.int32), 2)
    shapes = lambda ts: [(tuple(t.shape), t.dtype) for t in ts]
    assert shapes(plain) == [((7, 5), torch.int32), ((7, 5), torch.float32), ((7,), torch.int32)]
    assert shapes(mv) == [((7, 5), torch.int32), ((7, 5), torch.float32), ((7, 5), torch.float64), ((7,), torch.int32)]


# ---------------------------------------------------------------------------------------------- what the GPU test rests on

def test_the_normal_cases_are_the_five_of_the_issue():
    assert L.NORMAL_CASES == [(1, 67, 300, 32, 8, 10, 1), (2, 67, 300, 172, 64, 10, 3), (3, 130, 1000, 172, 256, 64, 1),
                              (4, 33, 17, 256, 65, 1, 2), (5, 67, 300, 4, 64, 10, 1)]


@pytest.mark.parametrize("seed,U,I,D,W,k,n_t", L.NORMAL_CASES)
def test_decided_share_of_the_normal_cases(seed, U, I, D, W, k, n_t):
    """``recommend_ref.check_topk`` pins the id set of a user only where the fp64 gap at rank k exceeds four times the row's
    largest fp32 error bound; the GPU test asks that share to be at least 0.9 - here it is computed from the inputs alone
    (1.000, 1.000, 0.985, 1.000, 1.000 for the five cases)."""
    c = L.normal_list_case(seed, U, I, D, W, n_t)
    s64 = R.scores64(c["user_emb"], c["item_emb"], c["user_block"], I)
    eps = R.dot_error_bound(c["user_emb"], c["item_emb"], c["user_block"], I)
    adm = L.admissible_list(U, I, c["list_pos"], c["list_len"], c["item_ok"])
    share = R.decided_share(s64, eps, adm, k)
    print("FIGURES decided share (%d,%d,%d,%d,%d,%d,%d): %.3f, admissible per user %.1f" % (seed, U, I, D, W, k, n_t, share, adm.sum(1).mean()))
    assert share >= 0.9
