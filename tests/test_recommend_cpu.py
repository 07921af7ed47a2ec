"""Host side of the read-only top-k recommendation: argument validation of ``TGN.recommend`` / ``recommend_topk`` (ValueError
before the GPU is asked for, PfoError for a valid call without one) and the numpy reference's own checks on hand-made cases."""
import numpy as np
import pytest
import torch

import pfotgnrec_amd as P
from pfotgnrec_amd import _lib
from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
import recommend_ref as R


@pytest.fixture(scope="module")
def cpu_model():
    g = make_graph(SyntheticConfig("t", 50, 10, 400, 8, 1, 4, 2), with_prices=False)
    nf = P.get_neighbor_finder(g.data, False)
    tgn = P.TGN(nf, g.node_features, g.edge_features, "cpu", n_layers=1, n_heads=2, use_memory=True, memory_dimension=8,
                message_function="identity")
    return tgn, np.arange(51, 61)


GOOD = dict(users=[1, 2, 3], timestamps=5.0, k=3)


@pytest.mark.parametrize("bad", [
    dict(k=0), dict(k=65), dict(k=2.5),
    dict(items=[51, 52, 51]), dict(items=[0, 51]), dict(items=[]), dict(items=[[51, 52]]), dict(items=[51, 61]),
    dict(items=[51.0, 52.0]),
    dict(timestamps=[1.0, 2.0]), dict(timestamps=np.zeros((3, 1))),
    dict(users=[1, 61, 2]), dict(users=[-1, 2, 3]), dict(users=[[1, 2, 3]]), dict(users=[1.5, 2.0, 3.0]),
    dict(exclude=[[51]]), dict(exclude=(np.zeros((2, 4), np.int32), np.zeros(2, np.int32))),
    dict(exclude=(np.zeros((3, 4), np.float32), np.zeros(3, np.int32))), dict(exclude=5),
    dict(item_ok=[1, 0]),
], ids=lambda d: "%s=%s" % (next(iter(d)), str(next(iter(d.values()))).replace("\n", "")[:24]))
def test_recommend_rejects_bad_arguments_before_asking_for_a_gpu(cpu_model, bad):
    tgn, items = cpu_model
    args = dict(GOOD, items=items)
    args.update(bad)
    with pytest.raises(ValueError):
        tgn.recommend(**args)


@pytest.mark.parametrize("extra", [
    dict(), dict(timestamps=np.array([5.0, 6.0, 5.0])), dict(exclude=[[51], [], [52, 999999]]),
    dict(exclude=(np.full((3, 2), -1, np.int32), np.zeros(3, np.int32))), dict(item_ok=np.ones(10, bool)),
    dict(users=torch.tensor([1, 2, 3]), items=torch.arange(51, 61)), dict(return_embeddings=True, n_neighbors=3),
], ids=["plain", "per_user_ts", "lists", "packed", "item_ok", "tensors", "embeddings"])
def test_recommend_on_a_cpu_model_is_an_error_not_a_fallback(cpu_model, extra):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    tgn, items = cpu_model
    args = dict(GOOD, items=items)
    args.update(extra)
    was = tgn.training
    with pytest.raises(_lib.PfoError):
        tgn.recommend(**args)
    assert tgn.training == was


def test_recommend_topk_validates_then_requires_a_gpu():
    ue, ie = torch.zeros(3, 8), torch.zeros(10, 8)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    for kw in (dict(k=0), dict(k=65), dict(user_block=i32(3)), dict(user_block=i32(2), n_blocks=2),
               dict(n_blocks=3), dict(item_ok=torch.ones(4, dtype=torch.uint8)), dict(excl_pos=i32(2, 4)),
               dict(excl_len=i32(3)), dict(excl_pos=torch.zeros(3, 4, dtype=torch.int64))):
        args = dict(k=3)
        args.update(kw)
        with pytest.raises(ValueError):
            P.recommend_topk(ue, ie, **args)
    for a, b in ((torch.zeros(3, 6), torch.zeros(10, 6)), (ue, torch.zeros(10, 4)), (ue.double(), ie.double()),
                 (torch.zeros(3, 260), torch.zeros(10, 260))):
        with pytest.raises(ValueError):
            P.recommend_topk(a, b, 3)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.PfoError):
            P.recommend_topk(ue, ie, 3)
        with pytest.raises(_lib.PfoError):
            P.recommend_topk(ue, ie, 3, user_block=i32(3), item_ok=torch.ones(5, dtype=torch.bool))   # two blocks of five


def test_recommend_topk_is_a_dispatcher_op_with_a_fake():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        ue, ie = torch.empty(7, 8), torch.empty(20, 8)
        pos, score, n = torch.ops.pfotgn.recommend_topk(ue, ie, 5, 2, torch.empty(7, dtype=torch.int32))
    assert (tuple(pos.shape), pos.dtype) == ((7, 5), torch.int32)
    assert (tuple(score.shape), score.dtype) == ((7, 5), torch.float32)
    assert (tuple(n.shape), n.dtype) == ((7,), torch.int32)


# ---- the reference's own behaviour on cases small enough to do by hand

def test_reference_ties_take_the_larger_position_first():
    s = np.array([[1.0, 3.0, 3.0, -0.0, 0.0, 3.0]])
    pos, sc, n = R.topk(s, R.admissible(1, 6), 5)
    assert pos.tolist() == [[5, 2, 1, 0, 4]] and n.tolist() == [5]         # +0 and -0 tie: position 4 before 3
    assert sc.tolist() == [[3.0, 3.0, 3.0, 1.0, 0.0]]
    pos, sc, n = R.topk(s, R.admissible(1, 6, np.array([[4]], np.int32)), 5)
    assert pos.tolist() == [[5, 2, 1, 0, 3]] and sc[0, 4] == 0.0 and not np.signbit(sc[0, 4])    # -0 is handed out as +0
    assert R.canonical_order(s[0]).tolist() == [5, 2, 1, 0, 4, 3]


def test_reference_skip_rules():
    excl = np.array([[5, 5, -1, 7, 2, 1], [0, 1, 2, 3, 4, 5]], np.int32)
    adm = R.admissible(2, 6, excl, np.array([4, 9], np.int32), np.array([1, 1, 1, 0, 1, 1], np.uint8))
    # user 0: 5 (twice), -1 and 7 (ignored) within its length, 2 and 1 beyond it; item 3 off for everybody; user 1: a length
    # beyond the row is clamped to it
    assert adm.tolist() == [[True, True, True, False, True, False], [False] * 6]
    assert R.admissible(1, 3, np.array([[1, 2]], np.int32)).tolist() == [[True, False, False]]     # no lengths: whole rows


def test_reference_fewer_than_k_admissible():
    s = np.array([[0.5, 2.0, 1.0], [1.0, 1.0, 1.0]])
    adm = np.array([[True, False, True], [False, False, False]])
    pos, sc, n = R.topk(s, adm, 3)
    assert pos.tolist() == [[2, 0, -1], [-1, -1, -1]] and n.tolist() == [2, 0]
    assert sc[0, :2].tolist() == [1.0, 0.5] and np.isneginf(sc[0, 2]) and np.isneginf(sc[1]).all()


def test_reference_scores_blocks_and_error_bound():
    ue = np.array([[1.0, 2.0, 0.0, -1.0], [0.5, 0.0, 0.0, 0.0]], np.float32)
    ie = np.arange(16, dtype=np.float32).reshape(4, 4)                        # two blocks of two candidates
    s = R.scores64(ue, ie, np.array([1, 0]), 2)
    assert s.tolist() == [[8 + 18 - 11, 12 + 26 - 15], [0.0, 2.0]]
    eps = R.dot_error_bound(ue, ie, np.array([1, 0]), 2)
    g = 4 * 2.0 ** -24 / (1 - 4 * 2.0 ** -24)
    assert np.allclose(eps, g * np.array([[8 + 18 + 11, 12 + 26 + 15], [0.0, 2.0]]), rtol=1e-15)


def test_checker_accepts_the_reference_and_rejects_what_it_must():
    c = R.normal_case(3, 9, 40, 16)
    s, eps = R.scores64(c["user_emb"], c["item_emb"], None, 40), R.dot_error_bound(c["user_emb"], c["item_emb"], None, 40)
    adm = R.admissible(9, 40, c["excl_pos"], c["excl_len"], c["item_ok"])
    pos, sc, n = R.topk(s.astype(np.float32), adm, 5)
    assert R.check_topk(pos, sc, n, s, eps, adm, 5) == R.decided_share(s, eps, adm, 5)
    swapped = pos.copy()
    swapped[0, [0, 1]] = swapped[0, [1, 0]]
    with pytest.raises(AssertionError):
        R.check_topk(swapped, sc, n, s, eps, adm, 5)
    banned = pos.copy()
    banned[1, 4] = np.flatnonzero(~adm[1])[0] if (~adm[1]).any() else pos[1, 0]
    with pytest.raises(AssertionError):
        R.check_topk(banned, sc, n, s, eps, adm, 5)
    off = sc.copy()
    off[2, 0] += 1e-3
    with pytest.raises(AssertionError):
        R.check_topk(pos, off, n, s, eps, adm, 5)


@pytest.mark.parametrize("seed,U,I,D,k", [(11, 37, 500, 172, 10), (12, 5, 130, 32, 5)])
def test_seeds_of_the_gpu_test_leave_nine_users_in_ten_decided(seed, U, I, D, k):
    """The GPU test asserts this share on the kernel's result; here it is taken from the inputs alone."""
    c = R.normal_case(seed, U, I, D)
    s, eps = R.scores64(c["user_emb"], c["item_emb"], None, I), R.dot_error_bound(c["user_emb"], c["item_emb"], None, I)
    share = R.decided_share(s, eps, R.admissible(U, I, c["excl_pos"], c["excl_len"], c["item_ok"]), k)
    print("decided share", share)
    assert share >= 0.9
