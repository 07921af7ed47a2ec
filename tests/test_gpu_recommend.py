"""GPU tests of the read-only top-k recommendation: ``pfo_recommend_topk`` against the numpy reference (bit for bit on exact
arithmetic, within the fp32 dot-product error bound on random embeddings) and ``TGN.recommend`` end to end against the
oracle - embeddings, top-k, and that a query leaves the model exactly as it found it."""
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

DEV = "cuda:0"
RTOL_EMB = 1e-4      # BASELINE.json north_star: embeddings within 1e-4 relative (max norm)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _kernel(c, k, n_t):
    out = P.recommend_topk(_dev(c["user_emb"]), _dev(c["item_emb"]), k, _dev(c["user_block"]), _dev(c["excl_pos"]),
                           _dev(c["excl_len"]), _dev(c["item_ok"]), n_blocks=n_t)
    return tuple(t.cpu().numpy() for t in out)


# ---------------------------------------------------------------------------------------------- the kernel alone

@pytest.mark.parametrize("D", [4, 32, 172, 256])
def test_exact_arithmetic_bit_exact_order(D):
    """Embeddings are integers in [-3, 3]: |score| <= 9 * 256 and every partial sum is an integer below 2^24, so the fp32 dot
    product is exact in any order and positions, scores and counts must be the reference's to the last bit - ties (duplicated
    item rows, an all-zero user), exclusions with duplicates / padding / out-of-range entries, item_ok, a user with fewer than
    k admissible candidates, users of mixed blocks in shuffled order.  The kernel's LDS walk (512 candidates a pass) is not
    reached here, the next test does that; 65 and 130 are not multiples of the 16-wide tile, 37 users make 3 tiles."""
    seed, full = 0, 0
    for U in (1, 5, 37):
        for I in (1, 3, 64, 65, 130, 500):
            for k in (1, 5, 64):
                for n_t in (1, 3):
                    seed += 1
                    c = R.exact_case(1000 * D + seed, U, I, D, k, n_t)
                    s = R.scores64(c["user_emb"], c["item_emb"], c["user_block"], I)
                    adm = R.admissible(U, I, c["excl_pos"], c["excl_len"], c["item_ok"])
                    want_pos, want_score, want_n = R.topk(s, adm, k)
                    assert want_n[0] < k, "user 0 must be short of candidates"
                    full += int((want_n == k).sum())
                    pos, score, n = _kernel(c, k, n_t)
                    tag = (U, I, D, k, n_t)
                    assert np.array_equal(n, want_n), tag
                    assert np.array_equal(pos, want_pos), tag
                    assert np.array_equal(score.view(np.int32), want_score.view(np.int32)), tag
    assert full > 500, "full rows must be the rule"


@pytest.mark.parametrize("D", [48, 64, 112, 128])
def test_exact_arithmetic_at_the_middle_row_widths(D):
    """The kernel is built for rows of up to 32, 64, 128, 176 and 256 floats; the D of the test above reach the first and the
    last two.  These reach the other two, at both ends of each: 17 users (two tiles), 65 candidates, three blocks in shuffled
    order, exact arithmetic, everything equal to the reference to the bit."""
    U, I, k, n_t = 17, 65, 5, 3
    c = R.exact_case(9000 + D, U, I, D, k, n_t)
    s = R.scores64(c["user_emb"], c["item_emb"], c["user_block"], I)
    want_pos, want_score, want_n = R.topk(s, R.admissible(U, I, c["excl_pos"], c["excl_len"], c["item_ok"]), k)
    assert (want_n < k).any() and (want_n == k).any()
    pos, score, n = _kernel(c, k, n_t)
    assert np.array_equal(n, want_n), D
    assert np.array_equal(pos, want_pos), D
    assert np.array_equal(score.view(np.int32), want_score.view(np.int32)), D


def test_exact_arithmetic_across_the_chunk_walk():
    """More candidates than one pass of the kernel's LDS walk holds (512), not a multiple of it, with ties across the chunk
    boundary (duplicated rows) and k = 64: the list carried from chunk to chunk must come out in the canonical order."""
    for (U, I, D, k, n_t) in ((5, 1300, 32, 64, 1), (21, 1025, 172, 10, 3), (3, 4096, 4, 5, 1)):
        c = R.exact_case(77 + I, U, I, D, k, n_t)
        s = R.scores64(c["user_emb"], c["item_emb"], c["user_block"], I)
        want_pos, want_score, want_n = R.topk(s, R.admissible(U, I, c["excl_pos"], c["excl_len"], c["item_ok"]), k)
        pos, score, n = _kernel(c, k, n_t)
        assert np.array_equal(n, want_n) and np.array_equal(pos, want_pos), (U, I, D, k, n_t)
        assert np.array_equal(score.view(np.int32), want_score.view(np.int32)), (U, I, D, k, n_t)


def test_optional_arguments_and_the_dispatcher_op():
    c = R.exact_case(5, 19, 70, 32, 5, 1)
    ue, ie = _dev(c["user_emb"]), _dev(c["item_emb"])
    s = R.scores64(c["user_emb"], c["item_emb"], None, 70)
    pos, score, n = (t.cpu().numpy() for t in P.recommend_topk(ue, ie, 5))               # nothing skipped
    want = R.topk(s, R.admissible(19, 70), 5)
    assert all(np.array_equal(a, b) for a, b in zip((pos, score, n), want))
    pos, score, n = (t.cpu().numpy() for t in torch.ops.pfotgn.recommend_topk(ue, ie, 5, 1, None, _dev(c["excl_pos"])))
    want = R.topk(s, R.admissible(19, 70, c["excl_pos"]), 5)                               # no lengths: whole rows
    assert all(np.array_equal(a, b) for a, b in zip((pos, score, n), want))
    pos, score, n = (t.cpu().numpy() for t in P.recommend_topk(ue, ie, 5, item_ok=_dev(c["item_ok"] != 0)))   # bool mask
    want = R.topk(s, R.admissible(19, 70, item_ok=c["item_ok"]), 5)
    assert all(np.array_equal(a, b) for a, b in zip((pos, score, n), want))
    from pfotgnrec_amd import _lib
    out = torch.empty(19 * 5 * 2 + 19, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.PfoError, match="16-byte aligned"):
        _lib.call("pfo_recommend_topk", ue.data_ptr() + 4, ie.data_ptr(), None, 19, 70, 1, 32, None, None, 0, None, 5,
                  out.data_ptr(), out.data_ptr(), None, _lib.stream_ptr())
    with pytest.raises(_lib.PfoError, match="k must be"):
        _lib.call("pfo_recommend_topk", ue.data_ptr(), ie.data_ptr(), None, 19, 70, 1, 32, None, None, 0, None, 65,
                  out.data_ptr(), out.data_ptr(), None, _lib.stream_ptr())


@pytest.mark.parametrize("seed,U,I,D,k", [(11, 37, 500, 172, 10), (12, 5, 130, 32, 5)])
def test_random_normal_embeddings_within_the_fp32_dot_product_bound(seed, U, I, D, k):
    """eps(u, i) = gamma_D * sum_d |u_d v_d| (``recommend_ref.dot_error_bound``) is the bound of an fp32 dot product in any
    order - derived, not measured.  ``check_topk`` holds the result to (a)-(d) and to the reference's ids for every user whose
    rank k / k + 1 gap exceeds 4 x its largest eps; the seeds leave at least nine users in ten of that kind (computed from the
    inputs alone in tests/test_recommend_cpu.py: all of them)."""
    c = R.normal_case(seed, U, I, D)
    s = R.scores64(c["user_emb"], c["item_emb"], None, I)
    eps = R.dot_error_bound(c["user_emb"], c["item_emb"], None, I)
    adm = R.admissible(U, I, c["excl_pos"], c["excl_len"], c["item_ok"])
    pos, score, n = _kernel(c, k, 1)
    share = R.check_topk(pos, score, n, s, eps, adm, k)
    err = np.abs(score.astype(np.float64) - np.take_along_axis(s, pos.astype(np.int64), 1)) / np.take_along_axis(eps, pos.astype(np.int64), 1)
    print("FIGURES recommend_topk (%d,%d,%d,%d): decided share %.3f, largest |score error| / eps %.3f" % (U, I, D, k, share, err.max()))
    assert share >= 0.9


# ---------------------------------------------------------------------------------------------- TGN.recommend end to end

N_USERS, N_ITEMS, K_NBR, BATCH = 1000, 100, 10, 40


class _World:
    """A C1-size synthetic graph, the model and the oracle on the same parameters, both advanced by a few training-path calls
    so that memory and pending messages are populated."""

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

    def oracle_embed(self, nodes, ts):
        mem = self.ref._get_updated_memory()[0] if self.use_mem else None
        return self.ref._embed(mem, np.asarray(nodes, np.int64), np.asarray(ts, np.float64), self.L, K_NBR, None)[0]

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


_WORLDS = {}


@pytest.fixture(params=[(1, True), (2, True), (2, False)], ids=["L1_mem", "L2_mem", "L2_nomem"])
def world(request):
    if request.param not in _WORLDS:
        _WORLDS[request.param] = _World(*request.param)
    return _WORLDS[request.param]


def _check_against_own_embeddings(w, out, k, exclude_pos=None, item_ok=None):
    """(a)-(d) of the returned top-k against the fp64 scores of the embeddings the same call returned."""
    ids, scores, n_valid, ue, ie, ub = (t.cpu().numpy() for t in out)
    U, I = ue.shape[0], len(w.items)
    s = R.scores64(ue, ie, ub, I)
    eps = R.dot_error_bound(ue, ie, ub, I)
    adm = R.admissible(U, I, exclude_pos, None, item_ok)
    pos_of = {int(v): i for i, v in enumerate(w.items)}
    pos = np.array([[pos_of.get(int(v), -1) for v in row] for row in ids], np.int32)
    assert ((pos >= 0) == (ids >= 0)).all()
    R.check_topk(pos, scores, n_valid, s, eps, adm, k)
    return ids, ue, ie, ub


def test_recommend_changes_nothing(world):
    w = world
    w.tgn.dropout = 0.1                                   # train mode with dropout on: a query must not apply it
    try:
        for mode in (True, False):
            w.tgn.train(mode)
            before, flags = w.state(), w.host_flags()
            a = w.tgn.recommend(w.users, w.now, 7, w.items, return_embeddings=True)
            b = w.tgn.recommend(w.users, w.now, 7, w.items, return_embeddings=True)
            assert all(torch.equal(x, y) for x, y in zip(a, b))
            assert all(torch.equal(x, y) for x, y in zip(before, w.state()))
            assert flags == w.host_flags()
            assert not any(t.requires_grad for t in a)
        ts = np.full(len(w.users), w.now)
        ts[::3] -= 4096.0
        before, flags = w.state(), w.host_flags()
        w.tgn.eval_chunk_roots = 50                       # the chunk walk: 31 users + 2 x 100 grid roots in five passes
        try:
            c = w.tgn.recommend(w.users, ts, 7, w.items, exclude=[[int(w.items[i % 5])] for i in range(len(w.users))],
                                item_ok=np.arange(N_ITEMS) % 7 != 0, return_embeddings=True)
        finally:
            w.tgn.eval_chunk_roots = 16384
        d = w.tgn.recommend(w.users, ts, 7, w.items, exclude=[[int(w.items[i % 5])] for i in range(len(w.users))],
                            item_ok=np.arange(N_ITEMS) % 7 != 0, return_embeddings=True)
        assert all(torch.equal(x, y) for x, y in zip(c, d))                    # chunked and unchunked walks agree to the bit
        assert all(torch.equal(x, y) for x, y in zip(before, w.state()))
        assert flags == w.host_flags()
    finally:
        w.tgn.dropout = 0.0


def test_embeddings_match_the_oracle(world):
    w = world
    w.tgn.train()
    out = w.tgn.recommend(w.users, w.now, 10, w.items, return_embeddings=True)
    ids, ue, ie, ub = _check_against_own_embeddings(w, out, 10)
    assert (ub == 0).all() and ie.shape == (N_ITEMS, 32) and ids.shape == (len(w.users), 10) and (ids > N_USERS).all()
    nodes = np.concatenate([w.users, w.items])
    want = w.oracle_embed(nodes, np.full(len(nodes), w.now))
    e = relerr(np.concatenate([ue, ie]), want)
    print("FIGURES recommend embeddings vs oracle (L=%d, memory=%s): relerr %.3g" % (w.L, w.use_mem, e))
    assert e < RTOL_EMB
    if w.use_mem:                                          # the fixture is worth something: messages are pending for these users
        assert w.tgn.memory.has_msg[torch.from_numpy(w.users).to(DEV)].any()


def test_per_user_timestamps(world):
    w = world
    U = len(w.users)
    grid = np.array([w.now, w.now - 30000.0, w.now + 512.0])
    ts = grid[np.random.RandomState(2).randint(0, 3, size=U)]
    out = w.tgn.recommend(w.users, ts, 5, w.items, return_embeddings=True)
    ids, ue, ie, ub = _check_against_own_embeddings(w, out, 5)      # each user against the block of its own time
    uniq = np.unique(ts)
    assert ie.shape[0] == len(uniq) * N_ITEMS and np.array_equal(uniq[ub], ts)
    nodes = np.concatenate([w.users, np.tile(w.items, len(uniq))])
    want = w.oracle_embed(nodes, np.concatenate([ts, np.repeat(uniq, N_ITEMS)]))
    assert relerr(np.concatenate([ue, ie]), want) < RTOL_EMB
    # a device tensor of timestamps takes the device route to the grid: the same answer
    out_t = w.tgn.recommend(torch.from_numpy(w.users).to(DEV), torch.from_numpy(ts).to(DEV), 5, torch.from_numpy(w.items).to(DEV),
                            return_embeddings=True)
    assert all(torch.equal(x, y) for x, y in zip(out, out_t))
    # and one user alone at its time gets what it got in the crowd
    one = w.tgn.recommend(w.users[4:5], ts[4], 5, w.items)
    assert torch.equal(one[0][0], out[0][4]) and torch.equal(one[1][0], out[1][4])


def test_exclusion_with_real_portfolios(world):
    w = world
    g, U = w.g, len(w.users)
    rows = [np.flatnonzero(g.data.sources == u)[-1] for u in w.users[:-2]] + [0, 1]         # each user's latest interaction
    held = [[int(N_USERS + 1 + j) for j in g.portfolio_idx[r, :g.portfolio_len[r]]] for r in rows]
    held[1] = held[1] + [5, 10 ** 6, -3] + held[1]        # a user id, ids beyond the node table, duplicates: ignored
    held[2] = [int(i) for i in w.items[:-3]]              # holds all but three candidates -> n_valid = 3
    k = 6
    plain = w.tgn.recommend(w.users, w.now, k, w.items)
    out = w.tgn.recommend(w.users, w.now, k, w.items, exclude=held, return_embeddings=True)
    excl_pos = np.full((U, max(len(h) for h in held)), -1, np.int32)
    for u, h in enumerate(held):
        excl_pos[u, :len(h)] = [v - N_USERS - 1 if N_USERS < v <= N_USERS + N_ITEMS else -1 for v in h]
    ids, _, _, _ = _check_against_own_embeddings(w, out, k, exclude_pos=excl_pos)
    for u in range(U):
        assert not set(ids[u].tolist()) & set(held[u]), u
    n_valid = out[2].cpu().numpy()
    assert n_valid[2] == 3 and (ids[2, 3:] == -1).all() and (n_valid[np.arange(U) != 2] == k).all()
    assert any(set(plain[0][u].cpu().tolist()) & set(held[u]) for u in range(U)), "the portfolios must exclude something"
    # the packed form is the same query
    W = max(len(h) for h in held)
    packed = np.full((U, W), -1, np.int32)
    for u, h in enumerate(held):
        packed[u, :len(h)] = np.clip(h, -1, 2 ** 31 - 1)
    lens = np.array([len(h) for h in held], np.int32)
    again = w.tgn.recommend(w.users, w.now, k, w.items, exclude=(packed, lens))
    again_t = w.tgn.recommend(w.users, w.now, k, w.items, exclude=(torch.from_numpy(packed).to(DEV), torch.from_numpy(lens).to(DEV)))
    assert all(torch.equal(x, y) for x, y in zip(out[:3], again)) and all(torch.equal(x, y) for x, y in zip(out[:3], again_t))


def test_training_still_works_afterwards(world):
    """Workspace pool and prefetch hygiene: a batch prepared ahead of time, then a query, then that batch under autograd -
    forward, backward and the state update are the oracle's."""
    w = world
    d, s = w.g.data, w.cursor
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)
    w.tgn.train()
    if w.use_mem:
        args = (dev(d.sources[s:s + BATCH], np.int32), dev(d.destinations[s:s + BATCH], np.int32),
                [dev(np.zeros(BATCH * 3) + N_USERS + 1, np.int32)], [3], dev(d.timestamps[s:s + BATCH], np.float64),
                dev(d.edge_idxs[s:s + BATCH], np.int32), K_NBR)
        with torch.enable_grad(), w.tgn.prefetching():
            assert w.tgn.prefetch(*args)                  # (a batch that will not come: the query drops it, the step prepares its own)
    w.tgn.recommend(w.users, w.now, 5, w.items)
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
        tab, mt, has = w.ref.pending_table()
        assert np.array_equal(w.tgn.memory.has_msg.cpu().numpy() > 0, has)
        assert relerr(w.tgn.memory.msg_table.cpu().numpy()[has], tab[has]) < RTOL_EMB
    # and a query behind the training step still answers for the state as it is now
    out = w.tgn.recommend(w.users, w.now, 5, w.items, return_embeddings=True)
    _, ue, ie, _ = _check_against_own_embeddings(w, out, 5)
    nodes = np.concatenate([w.users, w.items])
    assert relerr(np.concatenate([ue, ie]), w.oracle_embed(nodes, np.full(len(nodes), w.now))) < RTOL_EMB
