"""The training step against the oracle at the edges of the documented configuration domain (include/pfotgn.h: D a multiple of 4 in
[4, 256], Ef a multiple of 4 in [0, 64], 1/2/4 heads, up to 4 layers, K <= 64).  ``Ef`` and ``D`` together choose the attention
kernel ("Which attention form a shape reaches"); K = 64 is the full wavefront of the per-instance kernels and the
point where the run-merged layer-1 backward flushes a group on every change of a node's history count.

Everything a case feeds the two sides - graph, parameters, batches, negatives, raw draws - comes from numpy on the host, so
the coverage and kink conditions below depend on the oracle alone and are checked without a device by
``test_case_batches_cover_what_the_case_is_for``."""
import numpy as np
import pytest
import torch

from conftest import has_gpu

from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
from oracle import tgn_oracle as T
from oracle.neighbor_finder import OracleNeighborFinder, build_adjacency
from parity import (relerr, row_relerr, ROW_RTOL, RTOL_EMB, RTOL_GRAD_TIME, RTOL_GRAD_ORACLE_L2, _near_kink_roots,
                    _masked_bpr_backward, _legal_draws, GRAD_MARGIN, grad_blocks, grad_block_bar, check_grad_blocks,
                    fmt_worst_block, f64_twin, _f64_backward)

DEV = "cuda:0"
N_NEG = 3
MAX_KINK_FRACTION = 0.10      # roots the oracle leaves out per step (a pre-activation within KINK_THR of zero), at most
WIDE = (300, 25, 5000)        # users, items, edges: ~16 entries per user, ~200 per item
DEEP = (40, 8, 6000)          # ~150 entries per user, ~750 per item: histories pass 64

# id: D, Ef, H, L, K, use_mem, uniform, graph, B, first edge of each of the three steps, seed, the layer-1 backward is run-merged
# (memory and most-recent sampling: tgn.hip hands the instance groups over; pfo_attn_bwd_runs_possible refuses D > 192 with H = 4)
CASES = {
    # forward ring NR = 4 (D + Ef = 256); ring backward NR = 4 at layer 2; run-merged layer 1
    "a": (256, 0, 2, 2, 6, True, False, WIDE, 40, (2500, 2540, 2580), 1, True),
    # ring NR = 4 with edge columns (D + Ef = 256); attn_bwd_ring_kernel_none at layer 1 (no memory: level-0 rows are constants)
    "b": (252, 4, 1, 2, 6, False, False, WIDE, 40, (2500, 2540, 2580), 1, False),
    # ring NR = 2 with four heads (D + Ef = 128)
    "c": (124, 4, 4, 2, 7, True, False, WIDE, 40, (2500, 2540, 2580), 1, True),
    # ring at the NR H = 12 boundary with D + Ef = 184 <= 192
    "d": (172, 12, 4, 2, 8, True, False, WIDE, 40, (2500, 2540, 2580), 1, True),
    # register form NR = 3 (D + Ef = 196 > 192)
    "e": (192, 4, 2, 2, 8, True, False, WIDE, 40, (2500, 2540, 2580), 1, True),
    # register form, widest key row C = 2 D + 64 and the largest Cp
    "f": (172, 64, 2, 2, 8, True, False, WIDE, 40, (2500, 2540, 2580), 1, True),
    # D = 64 on the ring (D + Ef = 64); null edge_feat; message row 3 D wide
    "g": (64, 0, 2, 2, 8, True, False, WIDE, 40, (2500, 2540, 2580), 1, True),
    # Ef = 0 through the per-instance backward (uniform sampling, injected draws), no memory
    "h": (32, 0, 2, 1, 10, False, True, WIDE, 40, (2500, 2540, 2580), 1, False),
    # K = 64: a full wavefront of slots, the run-merged flush on every change of count
    "i": (32, 4, 2, 2, 64, True, False, DEEP, 16, (20, 4200, 4216), 1, True),
    # K = 63: one lane short of it
    "j": (32, 4, 2, 2, 63, True, False, DEEP, 16, (20, 4200, 4216), 1, True),
    # K = 33: just past half a wavefront, two instances no longer share one
    "k": (64, 4, 1, 2, 33, True, False, DEEP, 16, (20, 4200, 4216), 1, True),
    # per-instance kernel at the full wavefront (uniform sampling, injected draws)
    "l": (32, 4, 4, 1, 64, True, True, DEEP, 16, (20, 4200, 4216), 1, False),
    # head dim 2, rows of one 16-byte vector
    "m": (4, 4, 4, 2, 5, True, False, WIDE, 40, (2500, 2540, 2580), 1, True),
    # small D, no edge features
    "n": (8, 0, 1, 1, 3, True, False, WIDE, 40, (2500, 2540, 2580), 1, True),
    # small D with Ef close to D
    "o": (12, 8, 2, 2, 4, True, False, WIDE, 40, (2500, 2540, 2580), 1, True),
    # PFO_MAX_LAYERS; B = 8 keeps the 3^3 level growth small
    "p": (16, 4, 2, 4, 2, True, False, WIDE, 8, (2500, 2508, 2516), 1, True),
}
DEEP_CASES = ("i", "j", "k", "l")
F64_LAST_STEP_ONLY = ("i", "j")   # float64 walk of 5 200 instances x 63 / 64 keys: ~2.5 s per step on the host, so the last step only


class _Inputs:
    """What both sides of a case are fed, built on the host."""

    def __init__(self, cid):
        (self.D, self.Ef, self.H, self.L, self.K, self.use_mem, self.uniform, graph, self.B, self.starts, seed,
         self.run_merged) = CASES[cid]
        self.cid = cid
        D, Ef, L, K, B = self.D, self.Ef, self.L, self.K, self.B
        self.cfg = SyntheticConfig("edge_" + cid, graph[0], graph[1], graph[2], D, L, K, self.H, edge_dim=Ef)
        self.g = make_graph(self.cfg, with_prices=False)
        d = self.d = self.g.data
        self.onf = OracleNeighborFinder(*build_adjacency(d.sources, d.destinations, d.edge_idxs, d.timestamps), uniform=self.uniform)
        rs = np.random.RandomState(1000 * seed + D + Ef)
        # the oracle's initialiser (random in/out projection biases) with the time-encoder bias spread as test_step_against_oracle does
        self.params = T.init_params(D, Ef, L, seed=seed, use_memory=self.use_mem)
        self.params["time_encoder.w.bias"] = (rs.randn(D) * 0.3).astype(np.float32)
        self.steps = []
        for s in self.starts:
            sl = slice(s, s + B)
            neg = rs.randint(self.cfg.n_users + 1, self.cfg.n_users + self.cfg.n_items + 1, size=B * N_NEG)
            raw = None
            if self.uniform:
                R = (2 + N_NEG) * B
                raw = [rs.randint(0, 1 << 30, size=(R * (1 + K) ** i, K)).astype(np.int64) for i in range(L)]
            self.steps.append((d.sources[sl], d.destinations[sl], d.timestamps[sl], d.edge_idxs[sl], neg, raw))

    def roots(self, step):
        sb, db, tb, _, neg, _ = self.steps[step]
        return np.concatenate([sb, db, neg]), np.concatenate([tb, tb, np.repeat(tb, N_NEG)])

    def draws(self, step):
        """(product order, oracle order) of the step's legal draw positions, or (None, None)."""
        raw = self.steps[step][5]
        if raw is None:
            return None, None
        nodes, ts = self.roots(step)
        return _legal_draws(self.onf, nodes, ts, self.K, self.L, raw)

    def oracle(self):
        return T.OracleTGN(self.onf, self.g.node_features, self.g.edge_features, self.params, self.L, self.H, self.use_mem)

    def assert_history_coverage(self):
        """The deep-history cases: roots without history, with a partial one, with all K slots full - and, under most-recent
        sampling, two roots on one node whose counts differ (their neighbour lists are shifts of each other by d > 0)."""
        cnt, node = [], []
        for step in range(len(self.steps)):
            nodes, ts = self.roots(step)
            node.append(nodes)
            cnt.append(np.array([len(self.onf.find_before(int(a), b)[0]) for a, b in zip(nodes, ts)]))
        allc = np.concatenate(cnt)
        assert (cnt[0] == 0).any() and ((cnt[0] > 0) & (cnt[0] < self.K)).any(), np.bincount(np.minimum(allc, self.K))
        assert (np.concatenate(cnt[1:]) >= self.K).all()              # the later steps: every slot of every root is full
        if not self.uniform:
            shifted = 0
            for nodes, c in zip(node[1:], cnt[1:]):
                for n_ in np.unique(nodes):
                    shifted += len(np.unique(c[nodes == n_])) > 1
            assert shifted > 0


def _f64_on_step(cid, step, n_steps):
    """Whether the float64 oracle walks this step.  Every step of every case, unless a case's float64 walk is too slow for the
    suite (then its last step only; see F64_LAST_STEP_ONLY)."""
    return cid not in F64_LAST_STEP_ONLY or step == n_steps - 1


def _kink_fraction(ref, R, K):
    return float(_near_kink_roots(ref._ctx, R, K).mean())


def _numpy_adam(P_, grads, m, v, t, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):
    for k, g_ in grads.items():
        g_ = g_.reshape(P_[k].shape).astype(np.float64)
        m[k] = b1 * m.get(k, 0.0) + (1 - b1) * g_
        v[k] = b2 * v.get(k, 0.0) + (1 - b2) * g_ * g_
        P_[k] = (P_[k] - lr * (m[k] / (1 - b1 ** t)) / (np.sqrt(v[k] / (1 - b2 ** t)) + eps)).astype(np.float32)


@pytest.mark.parametrize("cid", sorted(CASES))
def test_case_batches_cover_what_the_case_is_for(cid):
    """Without a device: the oracle alone walks the case's three steps (its own gradients through Adam in numpy stand in for the
    product's optimizer) - at every step it leaves out at most 10 % of the roots as near a ReLU kink, and the deep-history cases
    hold the empty, partial, full and shifted histories they exist for.  Beside it the float64 oracle evaluates every step from
    the fp32 state: its ReLU decisions on the roots the mask keeps are the fp32 run's, and the block bar of the GPU test
    (GRAD_MARGIN x e32 per tensor, parity.py) is finite, positive and below the per-tensor bar it stands beside."""
    c = _Inputs(cid)
    if cid in DEEP_CASES:
        c.assert_history_coverage()
    ref = c.oracle()
    ref64 = f64_twin(ref)
    m, v = {}, {}
    B, R = c.B, (2 + N_NEG) * c.B
    for step, (sb, db, tb, eb, neg, _) in enumerate(c.steps):
        _, odraws = c.draws(step)
        f64_here = _f64_on_step(cid, step, len(c.steps))
        if f64_here:
            ref64.load_state(ref)
            e64 = ref64.compute_temporal_embeddings(sb, db, neg, tb, eb, c.K, draws=None if odraws is None else list(odraws))
        rse, rde, rne = ref.compute_temporal_embeddings(sb, db, neg, tb, eb, c.K, draws=odraws)
        frac = _kink_fraction(ref, R, c.K)
        assert frac <= MAX_KINK_FRACTION, (cid, step, frac)
        assert np.isfinite(np.concatenate([rse, rde, rne])).all()
        _, cache = T.bpr_loss(rse, rde.reshape(B, 1, -1), rne.reshape(B, N_NEG, -1))
        ds, dp, dn = T.bpr_loss_backward(cache)
        W = np.concatenate([ds, dp.reshape(B, -1), dn.reshape(N_NEG * B, -1)])
        grads = ref.backward(W)
        if f64_here:
            assert relerr(np.concatenate(e64), np.concatenate([rse, rde, rne])) < 1e-5     # the same function at the same point
            g64 = _f64_backward(ref64, ref, e64, B, c.K, n_neg=N_NEG)                       # asserts the ReLU decisions agree
            W[_near_kink_roots(ref._ctx, R, c.K)] = 0
            g32 = ref.backward(W)
            n_checked = 0
            for name in sorted(g32):
                if np.abs(g32[name]).max() < 1e-7:                                           # (what _run_case leaves out)
                    continue
                e32, bar = grad_block_bar(g32[name], g64[name], grad_blocks(name, g64[name].shape, c.D, c.Ef, c.H))
                assert np.isfinite(e32) and e32 > 0, (cid, step, name, e32)
                old = RTOL_GRAD_TIME if name.startswith("time_encoder") else RTOL_GRAD_ORACLE_L2
                assert GRAD_MARGIN * e32 < old and bar < old, (cid, step, name, e32)
                n_checked += 1
            assert n_checked >= 2 + 8 * c.L, (cid, step, n_checked)
        _numpy_adam(ref.P, grads, m, v, step + 1)


def _run_case(cid, deterministic=False):
    import pfotgnrec_amd as P
    from pfotgnrec_amd import _lib
    c = _Inputs(cid)
    D, K, L, B = c.D, c.K, c.L, c.B
    if cid in DEEP_CASES:
        c.assert_history_coverage()
    nf = P.get_neighbor_finder(c.d, uniform=c.uniform)
    tgn = P.TGN(nf, c.g.node_features, c.g.edge_features, DEV, n_layers=L, n_heads=c.H, dropout=0.0, use_memory=c.use_mem,
                memory_dimension=D, message_function="identity", n_neighbors=K)
    tgn.deterministic = deterministic
    names = sorted(c.params)
    sd = tgn.state_dict()
    assert sorted(k for k in sd if "layer_norm" not in k and not k.startswith("memory.")) == names
    with torch.no_grad():
        for k in names:
            sd[k].copy_(torch.from_numpy(c.params[k]))
    opt = P.FusedAdam(tgn, lr=1e-3)
    ref = c.oracle()
    ref64 = f64_twin(ref)
    worst, worst_block = {}, (0.0, None, None, 0.0, 0.0)

    def note(key, e):
        worst[key] = max(worst.get(key, 0.0), float(e))
        return e
    R = (2 + N_NEG) * B
    launches = None
    for step, (sb, db, tb, eb, neg, _) in enumerate(c.steps):
        ref.P = {k: tgn.state_dict()[k].detach().cpu().numpy().copy() for k in names}
        draws, odraws = c.draws(step)
        tgn.train(); opt.zero_grad()
        se, de, ne = tgn.compute_temporal_embeddings(sb, db, neg, tb, eb, K, draws=draws)
        f64_here = _f64_on_step(cid, step, len(c.steps))
        if f64_here:                                # float64 from the fp32 state BEFORE the fp32 step moves it on
            ref64.load_state(ref)
            e64 = ref64.compute_temporal_embeddings(sb, db, neg, tb, eb, K, draws=None if odraws is None else list(odraws))
        rse, rde, rne = ref.compute_temporal_embeddings(sb, db, neg, tb, eb, K, draws=odraws)
        emb = torch.cat([se, de, ne])
        got, remb = emb.detach().cpu().numpy(), np.concatenate([rse, rde, rne])
        assert np.isfinite(got).all(), (cid, step)
        e, er = note("emb relerr", relerr(got, remb)), note("emb row_relerr", row_relerr(got, remb))
        assert e < RTOL_EMB, (cid, step, e)
        assert er < ROW_RTOL, (cid, step, er)
        frac = note("kink fraction", _kink_fraction(ref, R, K))
        assert frac <= MAX_KINK_FRACTION, (cid, step, frac)
        last = step == len(c.steps) - 1
        if last:                                   # which layer-1 backward runs: counted on the last step's backward
            _lib.prof_collect()
            _lib.prof_enable(True)
        try:
            rgrads = _masked_bpr_backward(tgn, ref, emb, rse, rde, rne, B, K, n_neg=N_NEG)
            torch.cuda.synchronize()
        finally:
            if last:
                _lib.prof_enable(False)
        if last:
            launches = {k: v["count"] for k, v in _lib.prof_collect().items()}
        n_checked = 0
        mine = {}
        for name, p in tgn.named_parameters():
            if name not in rgrads:
                continue
            r = rgrads[name].reshape(p.shape)
            if np.abs(r).max() < 1e-7:
                assert p.grad is None or p.grad.abs().max().item() < 1e-6, name
                continue
            g_ = p.grad.cpu().numpy().astype(np.float64)
            assert np.isfinite(g_).all(), (cid, step, name)
            mine[name] = g_
            time = name.startswith("time_encoder")
            e = note("time grad L2" if time else "grad L2", np.linalg.norm(g_ - r) / (np.linalg.norm(r) + 1e-30))
            assert e < (RTOL_GRAD_TIME if time else RTOL_GRAD_ORACLE_L2), (cid, step, name, e)
            n_checked += 1
        assert n_checked >= 2 + 8 * L, (cid, step, n_checked)
        if f64_here:                               # beside the per-tensor bars: every block against float64, at the fp32 oracle's bar
            g64 = _f64_backward(ref64, ref, e64, B, K, n_neg=N_NEG)
            wb, over = check_grad_blocks(mine, rgrads, g64, D, c.Ef, c.H)
            worst_block = max(worst_block, wb, key=lambda w: w[0])
            if over:
                print("BLOCKS OVER THE BAR edge %s step %d: %s" % (cid, step, "; ".join("%s[%s] %.3g e32 %.3g bar %.3g" % o for o in over)))
            assert not over, (cid, step, over)
        if c.use_mem:
            mem = tgn.memory.memory.cpu().numpy()
            assert np.isfinite(mem).all()
            assert note("memory relerr", relerr(mem, ref.memory)) < RTOL_EMB, (cid, step)
            assert note("memory row_relerr", row_relerr(mem, ref.memory)) < ROW_RTOL, (cid, step)
            assert np.array_equal(tgn.memory.last_update.cpu().numpy(), ref.last_update)
            tab, mt, has = ref.pending_table()
            assert has.any() and np.array_equal(tgn.memory.has_msg.cpu().numpy() > 0, has)
            mine = tgn.memory.msg_table.cpu().numpy()[has]
            assert mine.shape[1] == 3 * D + c.Ef and np.isfinite(mine).all()
            assert note("msg relerr", relerr(mine, tab[has])) < RTOL_EMB, (cid, step)
            assert note("msg row_relerr", row_relerr(mine, tab[has])) < ROW_RTOL, (cid, step)
            assert np.array_equal(tgn.memory.msg_time.cpu().numpy()[has], mt[has])
        opt.step()
    tag = cid + ("-det" if deterministic else "")
    print("FIGURES edge %s (D %d Ef %d H %d L %d K %d): %s, %s, attn_bwd_runs %d attn_bwd %d" % (
        tag, D, c.Ef, c.H, L, K, ", ".join("%s %.3g" % kv for kv in sorted(worst.items())), fmt_worst_block(worst_block),
        launches["attn_bwd_runs"], launches["attn_bwd"]))
    if c.run_merged:
        assert launches["attn_bwd_runs"] == 1 and launches["attn_bwd"] == L - 1, launches      # layer 1 run-merged, one launch per layer above
    else:
        assert launches["attn_bwd_runs"] == 0 and launches["attn_bwd"] == L, launches


@pytest.mark.gpu
@pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")
@pytest.mark.parametrize("cid", sorted(CASES))
def test_step_against_oracle_at_config_edges(cid):
    """Three training steps (forward, BPR backward with near-kink roots left out on both sides, state, FusedAdam) against the
    oracle from one state dict, at the bars of test_step_against_oracle and the golden comparisons.  The kernels each case reaches
    are named beside it in CASES; the launch counts of the last backward prove which layer-1 backward ran."""
    _run_case(cid)


@pytest.mark.gpu
@pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")
def test_full_wavefront_per_instance_backward_deterministic():
    """Case l (K = 64, four heads, uniform sampling) with the bitwise-reproducible backward: the same bars."""
    _run_case("l", deterministic=True)
