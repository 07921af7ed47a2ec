#!/usr/bin/env python3
"""Generate tests/golden/*.npz by running the REFERENCE itself (build container only).

Imports youngandbin/PfoTGNRec from /root/reference (read-only; Python, CPU) on
the synthetic graphs of ``pfotgnrec_amd.synthetic`` and stores inputs plus the
reference's outputs.  The fixtures are data only - no reference source text is
stored.  The inline MV block of main.py (not importable: wandb/CUDA/data files)
is executed in place from the reference tree, as SURVEY.md App. E describes.

Usage:  python tools/make_golden.py [g1 g2 g3 g4 g5 g6 g7 g8 g9a g9b g10 g11 g12]  (default: all)
g10 = the g1 / g5 recipes on ``yyyymmddHHMMSS`` timestamps (~2.02e13: one f32 step is 2**21, about two calendar days).
Library versions used are recorded in each fixture (``versions``).
"""
import os
import sys
import copy
import types
import textwrap
from collections import defaultdict

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, REPO)
sys.path.insert(0, REF)

import numpy as np
import scipy
import scipy.stats
import torch

from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph, split_train  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
VERSIONS = "torch %s numpy %s scipy %s" % (torch.__version__, np.__version__, scipy.__version__)


def ref_modules():
    from utils.utils import get_neighbor_finder, NeighborFinder, RandEdgeSampler, MergeLayer
    from utils.data import Data
    from model.tgn import TGN
    from model.time_encoding import TimeEncode
    from model.temporal_attention import TemporalAttentionLayer
    return types.SimpleNamespace(**locals())


def save(name, **arrays):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, versions=np.array(VERSIONS), **arrays)
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))


def adversarial_graph():
    """Duplicate timestamps, zero-degree nodes, K > degree, node 0 queried."""
    rs = np.random.RandomState(7)
    U, I, E = 12, 6, 80
    src = rs.randint(1, U - 2, size=E)            # users U-2..U never interact (zero degree)
    dst = rs.randint(U + 1, U + I + 1, size=E)
    ts = np.sort(rs.randint(0, 25, size=E)).astype(np.float64)    # heavy timestamp ties
    eidx = np.arange(1, E + 1)
    return src, dst, ts, eidx, U + I


# ------------------------------------------------------------------ G1: neighbour sampler
def g1():
    R = ref_modules()
    out = {}
    # (a) C1-like graph, most-recent mode
    cfg = SyntheticConfig("g1", 300, 40, 4000, 8, 1, 10, 2)
    g = make_graph(cfg, with_prices=False, with_portfolios=False)
    d = g.data
    nf = R.get_neighbor_finder(R.Data(d.sources, d.destinations, d.timestamps, d.edge_idxs, d.labels, None), uniform=False)
    rs = np.random.RandomState(3)
    q_nodes = np.concatenate([d.sources[2000:2256], d.destinations[2000:2256], rs.randint(0, g.n_nodes, 256)])
    q_ts = np.concatenate([d.timestamps[2000:2256], d.timestamps[2000:2256], rs.randint(0, 1 << 24, 256).astype(np.float64)])
    for K in (10, 3, 0):
        nb, ei, et = nf.get_temporal_neighbor(q_nodes, q_ts, K)
        out["a_K%d_nbr" % K], out["a_K%d_eidx" % K], out["a_K%d_et" % K] = nb, ei, et
    out.update(a_src=d.sources, a_dst=d.destinations, a_ts=d.timestamps, a_eidx=d.edge_idxs, a_q_nodes=q_nodes, a_q_ts=q_ts)

    # (b) adversarial graph, most-recent + uniform (draws logged)
    src, dst, ts, eidx, max_node = adversarial_graph()
    D = R.Data(src, dst, ts, eidx, np.zeros(len(src)), None)
    nf = R.get_neighbor_finder(D, uniform=False)
    q_nodes = np.concatenate([np.arange(0, max_node + 1), src[40:], dst[40:]])
    q_ts = np.concatenate([np.full(max_node + 1, 13.0), ts[40:], ts[40:]])
    for K in (4, 20):
        nb, ei, et = nf.get_temporal_neighbor(q_nodes, q_ts, K)
        out["b_K%d_nbr" % K], out["b_K%d_eidx" % K], out["b_K%d_et" % K] = nb, ei, et
    nfu = R.get_neighbor_finder(D, uniform=True)
    log = []
    orig = np.random.randint

    def rec(lo, hi, n):
        r = orig(lo, hi, n); log.append((hi, r.copy())); return r
    np.random.seed(11)
    np.random.randint = rec
    try:
        nb, ei, et = nfu.get_temporal_neighbor(q_nodes, q_ts, 5)
    finally:
        np.random.randint = orig
    # dense draws: rows without history get -1
    draws = np.full((len(q_nodes), 5), -1, np.int64)
    it = iter(log)
    for i, (n_, t_) in enumerate(zip(q_nodes, q_ts)):
        if len(nf.find_before(n_, t_)[0]) > 0:
            hi, r = next(it); draws[i] = r
    out.update(b_src=src, b_dst=dst, b_ts=ts, b_eidx=eidx, b_q_nodes=q_nodes, b_q_ts=q_ts,
               b_uni_nbr=nb, b_uni_eidx=ei, b_uni_et=et, b_uni_draws=draws, b_uni_seed=np.array(11))
    save("g1_sampler", **out)


# ------------------------------------------------------------------ G2: candidate draw
def g2():
    R = ref_modules()
    cfg = SyntheticConfig("g2", 200, 30, 3000, 8, 1, 10, 2)
    g = make_graph(cfg, with_prices=False)
    d = g.data
    sl = slice(1000, 1064)
    out = dict(src=d.sources[sl], dst_all=d.destinations[:2400], port_idx=g.portfolio_idx[sl], port_len=g.portfolio_len[sl],
               upper_u=np.array(g.upper_u), n_items=np.array(cfg.n_items))
    for size, seed in ((3, None), (20, None), (30, 2024)):      # 30 > available when a portfolio is non-empty -> replace=True
        np.random.seed(5)
        s = R.RandEdgeSampler(d.sources[sl], d.destinations[:2400], d.portfolios[sl], g.upper_u, g.map_item_id, seed=seed)
        out["neg_size%d" % size] = s.sample(size)
        out["seed_size%d" % size] = np.array(-1 if seed is None else seed)
    save("g2_candidates", **out)


# ------------------------------------------------------------------ G3: MV selection (main.py:192-304 executed in place)
class _Rec:
    def __init__(self, mod, hooks):
        self._m, self._h = mod, hooks

    def __getattr__(self, k):
        return self._h.get(k, getattr(self._m, k))


def run_mv_block(g, train_dst, sl, lam, gamma=2.0, num_neg=20, p_pos=1, p_neg=3, seed=9):
    R = ref_modules()
    d = g.data
    src_lines = open(os.path.join(REF, "main.py")).read().split("\n")[191:304]
    code = textwrap.dedent("\n".join(src_lines))
    rank_log, argsort_log, neg_log = [], [], []

    def rankdata(x):
        r = scipy.stats.rankdata(x); rank_log.append((np.array(x, np.float64), r)); return r

    def argsort(x, *a, **k):
        r = np.argsort(x, *a, **k); argsort_log.append((np.array(x, np.float64), r)); return r

    class RecSampler(R.RandEdgeSampler):
        def sample(self, size):
            r = super().sample(size); neg_log.append(r.copy()); return r

    ts_b = d.timestamps[sl]
    time_feature, day_idx = {}, np.zeros(len(ts_b), np.int64)
    for i, ts in enumerate(ts_b):
        key = str(ts)[:8]
        if key not in time_feature:
            day = int(g.day_of(ts))
            time_feature[key] = {"_day": day, **{c: g.prices[day, j] for j, c in enumerate(g.codes)}}
        day_idx[i] = time_feature[key]["_day"]
    ns = dict(np=_Rec(np, {"argsort": argsort}), stats=_Rec(scipy.stats, {"rankdata": rankdata}), RandEdgeSampler=RecSampler,
              args=types.SimpleNamespace(num_negatives=num_neg, p_pos_num=p_pos, p_neg_num=p_neg, gamma=gamma, lambda_mv=lam),
              train_data=types.SimpleNamespace(destinations=train_dst), upper_u=g.upper_u, map_item_id=g.map_item_id,
              time_feature=time_feature, sources_batch=d.sources[sl], destinations_batch=d.destinations[sl].copy(),
              portfolios_batch=d.portfolios[sl], timestamps_batch=ts_b)
    np.random.seed(seed)
    exec(compile(code, "<reference main.py:192-304>", "exec"), ns)
    B = len(ts_b)
    # per interaction: rankdata(y_mv), rankdata(tgn), argsort(y_mv), argsort(new_rank)
    y_mv = np.stack([rank_log[2 * b][0] for b in range(B)])
    invest_rank = np.stack([rank_log[2 * b][1] for b in range(B)])
    new_rank = np.stack([argsort_log[2 * b + 1][0] for b in range(B)])
    order = np.stack([argsort_log[2 * b + 1][1][::-1] for b in range(B)])
    return dict(neg=neg_log[0], y_mv=y_mv, invest_rank=invest_rank, new_rank=new_rank, order=order,
                p_pos=np.asarray(ns["p_pos_batch"]), p_neg=np.asarray(ns["p_neg_batch"]), day_idx=day_idx,
                dst_after=np.asarray(ns["destinations_batch"]))


def g3():
    cfg = SyntheticConfig("g3", 200, 40, 3000, 8, 1, 10, 2, n_days=8)
    g = make_graph(cfg)
    d = g.data
    sl = slice(1500, 1564)
    out = dict(src=d.sources[sl], dst=d.destinations[sl], ts=d.timestamps[sl], dst_all=d.destinations[:2400],
               port_idx=g.portfolio_idx[sl], port_len=g.portfolio_len[sl], prices=g.prices, upper_u=np.array(g.upper_u),
               gamma=np.array(2.0))
    for lam in (0.5, 0.1):
        r = run_mv_block(g, d.destinations[:2400], sl, lam)
        for k, v in r.items():
            out["lam%02d_%s" % (int(lam * 10), k)] = v
    out.update(_g3_layout_arrays(g, sl))
    save("g3_mv", **out)


def _g3_layout_arrays(g, sl):
    """The file-format side of the g3 inputs, as data: the ``time_feature`` day key of every interaction
    (``str(ts)[:8]``, main.py:212 - the keys run_mv_block builds its dict with), the stock codes in item order (the pickle's
    inner keys / ``map_item_id``) and the batch's portfolios as the code lists ``ml_transaction.json`` holds ('' = empty)."""
    d = g.data
    keys = np.array([str(ts)[:8] for ts in d.timestamps[sl]])
    W = max(len(p) for p in d.portfolios[sl])
    ports = np.array([list(p) + [""] * (W - len(p)) for p in d.portfolios[sl]])
    return dict(day_keys=keys, codes=np.array(g.codes), port_codes=ports)


def g3_layout():
    """Adds the layout arrays above to the committed g3 fixture WITHOUT re-running the reference (every other array is kept
    byte for byte): they are inputs derived from the synthetic graph, not reference outputs."""
    cfg = SyntheticConfig("g3", 200, 40, 3000, 8, 1, 10, 2, n_days=8)
    g = make_graph(cfg)
    path = os.path.join(OUT, "g3_mv.npz")
    old = dict(np.load(path, allow_pickle=False))
    assert np.array_equal(old["ts"], g.data.timestamps[1500:1564]) and np.array_equal(old["prices"], g.prices)
    old.update(_g3_layout_arrays(g, slice(1500, 1564)))
    np.savez_compressed(path, **old)
    print("augmented %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))


# ------------------------------------------------------------------ G4: modules (fwd + autograd grads)
def g4():
    R = ref_modules()
    torch.manual_seed(0)
    rs = np.random.RandomState(0)
    D, Ef, K, N, H = 12, 4, 6, 40, 2
    out = dict(D=np.array(D), Ef=np.array(Ef), K=np.array(K), H=np.array(H))
    # time encoder with a non-zero bias, |t*w| up to 1e7 (fp32 FMA sensitivity, SURVEY §7 hard part 1)
    te = R.TimeEncode(D)
    with torch.no_grad():
        te.w.bias.copy_(torch.randn(D) * 0.5)
    t = torch.from_numpy(np.concatenate([rs.randint(0, 1 << 24, 90), [0, 1, 16777215]]).astype(np.float32)).reshape(31, 3)
    y = te(t)
    gy = torch.from_numpy(rs.randn(*y.shape).astype(np.float32))
    y.backward(gy)
    out.update(te_t=t.numpy(), te_w=te.w.weight.detach().numpy(), te_b=te.w.bias.detach().numpy(), te_y=y.detach().numpy(),
               te_gy=gy.numpy(), te_gw=te.w.weight.grad.numpy(), te_gb=te.w.bias.grad.numpy())
    # GRU cell
    M = 3 * D + Ef
    gru = torch.nn.GRUCell(M, D)
    x = torch.randn(N, M); h = torch.randn(N, D)
    hn = gru(x, h)
    ghn = torch.randn(N, D)
    hn.backward(ghn)
    out.update(gru_x=x.numpy(), gru_h=h.numpy(), gru_hn=hn.detach().numpy(), gru_ghn=ghn.numpy(),
               **{"gru_" + k: v.detach().numpy() for k, v in gru.named_parameters()},
               **{"gru_g_" + k: v.grad.numpy() for k, v in gru.named_parameters()})
    # temporal attention layer: all-padding rows, partial masks
    att = R.TemporalAttentionLayer(D, D, Ef, D, output_dimension=D, n_head=H, dropout=0.0)
    xs = torch.randn(N, D, requires_grad=True); tq = torch.randn(N, 1, D, requires_grad=True)
    nb = torch.randn(N, K, D, requires_grad=True); tn = torch.randn(N, K, D, requires_grad=True); ef = torch.randn(N, K, Ef)
    mask = torch.zeros(N, K, dtype=torch.bool)
    mask[:8] = True                         # no valid neighbour at all
    for i in range(8, 24):
        mask[i, :rs.randint(1, K)] = True   # left padding
    o, wts = att(xs, tq, nb, tn, ef, mask.clone())
    go = torch.randn(N, D)
    o.backward(go)
    out.update(att_x=xs.detach().numpy(), att_tq=tq.detach().numpy()[:, 0], att_nb=nb.detach().numpy(), att_tn=tn.detach().numpy(),
               att_ef=ef.numpy(), att_mask=mask.numpy(), att_out=o.detach().numpy(), att_go=go.numpy(), att_w=wts.detach().numpy(),
               att_gx=xs.grad.numpy(), att_gtq=tq.grad.numpy()[:, 0], att_gnb=nb.grad.numpy(), att_gtn=tn.grad.numpy(),
               **{"att_p_" + k: v.detach().numpy() for k, v in att.named_parameters()},
               **{"att_g_" + k: v.grad.numpy() for k, v in att.named_parameters()})
    save("g4_modules", **out)


# ------------------------------------------------------------------ G5: full training steps with injected state
def dense_messages(tgn, n_nodes, M):
    tab = np.zeros((n_nodes, M), np.float32); t = np.zeros(n_nodes, np.float32); cnt = np.zeros(n_nodes, np.int32)
    for nid, lst in tgn.memory.messages.items():
        cnt[nid] = len(lst)
        if lst:
            tab[nid] = lst[-1][0].detach().numpy(); t[nid] = float(lst[-1][1])
    return tab, t, cnt


def g5():
    step_fixtures("g5_step_", 16)


G5_CASES = (("L1_mem", 1, True, False, 2, "base"), ("L2_mem", 2, True, False, 2, "base"),
            ("L2_nomem_uniform", 2, False, True, 4, "base"), ("L1_mem_p", 1, True, False, 2, "p"))


def step_fixtures(prefix, dim, timestamps=None, cases=G5_CASES, message_function="identity", seed=1, recorded=(2, 3, 4), write=True):
    # Note: every recorded step stores its own inputs (state_dict, memory, pending messages, batch, draws) next to its
    # outputs, so a fixture is self-contained.  The 5-step trajectory itself is not bit-reproducible across runs of this
    # script for the 2-layer memory case (multi-threaded CPU reductions in the reference's torch ops); regenerating
    # replaces that fixture with an equally valid one.
    # ``timestamps`` (g10): f64[E] sorted, replace the synthetic graph's; the uniform case then also records every sampler
    # call's output in the reference's own slot order and the draws re-addressed to the canonical order (readdress_draws).
    # ``cases`` / ``message_function`` / ``seed`` / ``recorded`` (g11): the same recipe on other configurations; with the MLP
    # message function the smallest |hidden pre-activation| the reference computed over the recorded steps is stored as
    # ``mlp_min_abs_preact``.  ``write`` = False returns the arrays of the (single) case instead of saving them.
    R = ref_modules()
    for tag, L, use_mem, uniform, H, path in cases:
        torch.manual_seed(seed); np.random.seed(seed)
        cfg = SyntheticConfig("g5", 120, 20, 1500, dim, L, 5, H)
        g = make_graph(cfg, with_prices=False)
        d = g.data
        if timestamps is not None:
            assert len(timestamps) == cfg.n_edges and np.all(np.diff(timestamps) >= 0)
            d.timestamps = np.asarray(timestamps, np.float64).copy()
        D, Ef, K, B, n = cfg.dim, cfg.edge_dim, cfg.n_neighbors, 24, g.n_nodes
        M = 3 * D + Ef
        rdata = R.Data(d.sources, d.destinations, d.timestamps, d.edge_idxs, d.labels, d.portfolios)
        nf = R.get_neighbor_finder(rdata, uniform=uniform)
        tgn = R.TGN(neighbor_finder=nf, node_features=g.node_features, edge_features=g.edge_features.copy(), device=torch.device("cpu"),
                    n_layers=L, n_heads=H, dropout=0.0, use_memory=use_mem, message_dimension=100, memory_dimension=D,
                    memory_update_at_start=True, embedding_module_type="graph_attention", message_function=message_function,
                    aggregator_type="last", memory_updater_type="gru", n_neighbors=K)
        with torch.no_grad():
            tgn.time_encoder.w.bias.copy_(torch.randn(D) * 0.3)
        preact = []                                  # (step, min |Linear 0 output|) of every MLP call
        cur_step = [0]
        if message_function == "mlp":
            tgn.message_function.mlp[0].register_forward_hook(
                lambda mod, inp, res: preact.append((cur_step[0], float(res.detach().abs().min()) if res.numel() else np.inf)))
        opt = torch.optim.Adam(tgn.parameters(), lr=1e-3)
        rs = np.random.RandomState(2)
        out = dict(L=np.array(L), H=np.array(H), K=np.array(K), use_memory=np.array(use_mem), uniform=np.array(uniform),
                   path=np.array(path), src_all=d.sources, dst_all=d.destinations, ts_all=d.timestamps, eidx_all=d.edge_idxs,
                   node_features=g.node_features, edge_features=g.edge_features, lr=np.array(1e-3))
        n_steps, first = max(recorded) + 1, 700
        for step in range(n_steps):
            cur_step[0] = step
            s = first + step * B
            sb, db, tb, eb = d.sources[s:s + B], d.destinations[s:s + B], d.timestamps[s:s + B], d.edge_idxs[s:s + B]
            n_neg = 3
            neg = rs.randint(cfg.n_users + 1, cfg.n_users + cfg.n_items + 1, size=(B, n_neg))
            ppos = rs.randint(cfg.n_users + 1, cfg.n_users + cfg.n_items + 1, size=B)
            record = step in recorded
            pre = "s%d_" % step
            if record:
                sd = {k: v.detach().numpy().copy() for k, v in tgn.state_dict().items()
                      if not (k.startswith("memory_updater.memory.") or k.startswith("embedding_module.memory.")
                              or k.startswith("embedding_module.time_encoder."))}
                for k, v in sd.items():
                    out[pre + "sd_" + k] = v
                if use_mem:
                    tab, mt, cnt = dense_messages(tgn, n, M)
                    out.update({pre + "msg_tab": tab, pre + "msg_t": mt, pre + "msg_cnt": cnt})
                # Adam moments BEFORE this step (main.py:123 optimizer): with them injected, the post-step parameters
                # ("after_*") are a function of this step's gradients alone
                names = {id(v): k for k, v in tgn.named_parameters()}
                for pp_, st_ in opt.state.items():
                    k = names[id(pp_)]
                    out[pre + "adam_m_" + k] = st_["exp_avg"].detach().numpy().copy()
                    out[pre + "adam_v_" + k] = st_["exp_avg_sq"].detach().numpy().copy()
                    out[pre + "adam_t_" + k] = np.array(int(st_["step"]))      # per tensor: the GRU's lag one step (None grad in step 0)
            # uniform mode: log the draws in call order
            draws, orig = [], np.random.randint
            calls = []                                   # uniform: (nodes, ts, nbr, eidx, et) of every sampler call, in call order
            if uniform:
                cur = []

                def rec(lo, hi, n_):
                    r = orig(lo, hi, n_); cur.append(r.copy()); return r
                orig_gtn = nf.get_temporal_neighbor

                def gtn(nodes, ts, n_neighbors=20):
                    cur.clear()
                    np.random.randint = rec
                    try:
                        res = orig_gtn(nodes, ts, n_neighbors)
                    finally:
                        np.random.randint = orig
                    dense = np.full((len(nodes), n_neighbors), -1, np.int64)
                    it = iter(cur)
                    for i, (a, b) in enumerate(zip(nodes, ts)):
                        if len(nf.find_before(a, b)[0]) > 0:
                            dense[i] = next(it)
                    draws.append(dense)
                    calls.append((np.asarray(nodes).copy(), np.asarray(ts, np.float64).copy()) + tuple(np.array(a) for a in res))
                    return res
                nf.get_temporal_neighbor = gtn
            tgn.train(); opt.zero_grad()
            if path == "p":
                se, de, pe, ne = tgn.compute_temporal_embeddings_p(sb, db, ppos, neg.flatten(), tb, eb, K)
            else:
                se, de, ne = tgn.compute_temporal_embeddings(sb, db, neg.flatten(), tb, eb, K)
                pe = de
            if uniform:
                nf.get_temporal_neighbor = orig_gtn
            bs = se.shape[0]
            pos_scores = torch.sum(se.view(bs, 1, -1) * pe.view(bs, 1, -1), dim=2)
            neg_scores = torch.matmul(se.view(bs, 1, -1), ne.view(bs, n_neg, -1).transpose(1, 2)).squeeze()
            loss = -torch.mean(torch.log(torch.sigmoid(torch.mean(pos_scores - neg_scores, dim=1))))
            for e_ in (se, de, pe, ne):
                e_.retain_grad()
            loss.backward()
            if record:
                out.update({pre + "src": sb, pre + "dst": db, pre + "ts": tb, pre + "eidx": eb, pre + "neg": neg, pre + "ppos": ppos,
                            pre + "emb_src": se.detach().numpy(), pre + "emb_dst": de.detach().numpy(),
                            pre + "emb_pos": pe.detach().numpy(), pre + "emb_neg": ne.detach().numpy(),
                            pre + "loss": np.array(loss.item(), np.float32),
                            pre + "gemb_src": se.grad.numpy(), pre + "gemb_neg": ne.grad.numpy(),
                            pre + "gemb_pos": (pe.grad.numpy() if pe.grad is not None else np.zeros_like(pe.detach().numpy()))})
                for k, v in tgn.named_parameters():
                    if v.requires_grad:
                        out[pre + "grad_" + k] = (v.grad.numpy().copy() if v.grad is not None else np.zeros(v.shape, np.float32))
                for j, dr in enumerate(draws):
                    out[pre + "draws%d" % j] = dr
                if uniform and timestamps is not None:
                    out.update({pre + k: v for k, v in readdress_draws(nf, calls, draws, K, L).items()})
            opt.step()
            if use_mem:
                tgn.memory.detach_memory()
            if record:
                for k, v in tgn.named_parameters():
                    if v.requires_grad:
                        out[pre + "after_" + k] = v.detach().numpy().copy()
                if use_mem:
                    tab, mt, cnt = dense_messages(tgn, n, M)
                    out.update({pre + "after_memory": tgn.memory.memory.detach().numpy().copy(),
                                pre + "after_last_update": tgn.memory.last_update.detach().numpy().copy(),
                                pre + "after_msg_tab": tab, pre + "after_msg_t": mt, pre + "after_msg_cnt": cnt})
        out["recorded_steps"] = np.array(list(recorded))
        if message_function == "mlp":
            out["mlp_min_abs_preact"] = np.array(min(v for st_, v in preact if st_ in recorded), np.float64)
        if not write:
            assert len(cases) == 1
            return out
        if uniform and timestamps is not None:
            n_moved = sum(int(out["s%d_n_readdressed_roots" % s_]) for s_ in (2, 3, 4))
            assert n_moved > 0, "no root whose reference slot order differs from the stable one: the fixture would not pin the tie policy"
            print("%s%s: %d roots re-addressed over the recorded steps" % (prefix, tag, n_moved))
        save(prefix + tag, **out)


# ------------------------------------------------------------------ G11: the same steps with the MLP message function
def g11():
    """g5's recipe with message_function="mlp", message_dimension=100 (the reference's and main.py's defaults): memory, most-recent
    sampling.  L = 1 (main.py's own layer count): D 16 / Ef 4 -> raw message 52, hidden 26 (not a multiple of 4); L = 2: D 12 ->
    raw message 40, hidden 20 (at D 16 its two steps do not fit a committed file).  Two consecutive recorded steps each; the state dict carries every MLP tensor under both of the reference's names
    (message_function.mlp.* and message_function.layers.*).
    A hidden unit whose pre-activation sits within rounding distance of zero could take the other ReLU branch on another
    implementation whose forward agrees to ~1e-6; the seed is moved until the smallest |pre-activation| the reference computed
    over the recorded steps is at least parity.KINK_THR, and that minimum is stored in the fixture."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from parity import KINK_THR
    for dim, case in ((16, ("L1_mem_mlp", 1, True, False, 2, "base")), (12, ("L2_mem_mlp", 2, True, False, 2, "base"))):
        for seed in range(1, 40):
            out = step_fixtures("g11_step_", dim, cases=(case,), message_function="mlp", seed=seed, recorded=(2, 3), write=False)
            lo = float(out["mlp_min_abs_preact"])
            print("g11 %s seed %d: min |hidden pre-activation| %.3g" % (case[0], seed, lo))
            if lo >= KINK_THR:
                break
        else:
            raise AssertionError("no seed keeps the hidden pre-activations away from the kink")
        out["seed"] = np.array(seed)
        save("g11_step_" + case[0], **out)


def g6():
    """Ranking metrics of evaluation.py:114-145 through the reference's own recall_at_k / ndcg_at_k (evaluation.py:11-21):
    score rows [positive | N negatives], ranking = np.argsort(scores)[::-1], positive = index 0.  Rows cover clear
    winners / losers, exact ties between the positive and negatives (the destination itself can be among the negatives:
    utils.py:96 only removes the portfolio), ties among negatives only, and all-equal rows."""
    import evaluation as ev                                   # the reference module (imports cleanly: sklearn, tqdm present)
    rs = np.random.RandomState(11)
    B, N = 96, 25
    scores = rs.randn(B, 1 + N).astype(np.float32)
    kind = np.zeros(B, np.int64)
    for b in range(B):
        k = b % 6
        kind[b] = k
        if k == 1:                                            # the destination appears among the negatives: an exact tie
            scores[b, 1 + rs.randint(N)] = scores[b, 0]
        elif k == 2:                                          # several negatives tie with the positive
            scores[b, 1 + rs.choice(N, 3, replace=False)] = scores[b, 0]
        elif k == 3:                                          # ties among negatives only
            scores[b, 1 + rs.choice(N, 4, replace=False)] = scores[b, 1]
        elif k == 4:                                          # positive on top / at the bottom
            scores[b, 0] = scores[b].max() + 1.0 if b % 12 == 4 else scores[b].min() - 1.0
        elif k == 5 and b % 12 == 5:                          # everything equal
            scores[b, :] = 0.25
    topk = [1, 3, 5]
    pos_rank = np.zeros(B, np.int64)                          # position of the positive in the reference's ranking
    recall = np.zeros((B, 3)); ndcg = np.zeros((B, 3))
    n_greater = (scores[:, 1:] > scores[:, :1]).sum(1)        # the positive's rank lies in [n_greater, n_greater + n_equal]
    n_equal = (scores[:, 1:] == scores[:, :1]).sum(1)
    for b in range(B):
        ranking = np.argsort(scores[b])[::-1]                 # evaluation.py:122
        pos_rank[b] = int(np.where(ranking == 0)[0][0])
        recall[b] = [ev.recall_at_k(ranking, [0], k) for k in topk]   # evaluation.py:127
        ndcg[b] = [ev.ndcg_at_k(ranking, [0], k) for k in topk]       # evaluation.py:128
        assert n_greater[b] <= pos_rank[b] <= n_greater[b] + n_equal[b]
    save("g6_eval_metrics", scores=scores, kind=kind, pos_rank=pos_rank, recall=recall, ndcg=ndcg, n_greater=n_greater,
         n_equal=n_equal, topk=np.array(topk))


def g7():
    """Price ingest the way main.py consumes it: ``time_feature[str(ts)[:8]][code]`` -> 30 prices (main.py:88-89, 212-227),
    log-returns np.log(p[1:] / p[:-1]); the fixture holds a small pickled-dict equivalent as arrays (day keys, codes,
    prices) plus the per-interaction features the reference's expressions produce for them."""
    rs = np.random.RandomState(13)
    days = ["20240102", "20240103", "20240105"]
    codes = ["005930", "000660", "035420", "051910"]
    prices = 100.0 * np.exp(np.cumsum(rs.randn(len(days), len(codes), 30) * 0.02, axis=2))
    time_feature = {dkey: {c: prices[i, j] for j, c in enumerate(codes)} for i, dkey in enumerate(days)}
    map_item_id = {c: j for j, c in enumerate(codes)}
    ts_batch = np.array([202401021530, 202401030915, 202401051200, 202401021000], np.int64)
    cand = [["005930", "035420"], ["000660"], ["051910", "005930", "000660"], ["035420"]]
    feats, mus, shapes = [], [], []
    for ts, stocks in zip(ts_batch, cand):
        ts_ = str(ts)[:8]                                                        # main.py:212
        feature_ = np.array([time_feature[ts_][c] for c in stocks])              # main.py:217
        feature = np.log(feature_[:, 1:] / feature_[:, :-1])                     # main.py:218
        feats.append(feature); mus.append(np.mean(feature, axis=1)); shapes.append(len(stocks))
    save("g7_price_ingest", days=np.array(days), codes=np.array(codes), prices=prices, ts_batch=ts_batch,
         cand_idx=np.array([[map_item_id[c] for c in st] + [-1] * (3 - len(st)) for st in cand]),
         cand_len=np.array(shapes), features=np.concatenate(feats), mus=np.concatenate(mus))


# ------------------------------------------------------------------ G8: train-mode attention dropout (the benched setting)
class DropoutLog:
    """Runs the reference with torch.nn.functional.dropout wrapped: the REAL dropout is called and the multiplier it applied
    is read off its result (1/(1-p) where the weight survived, 0 where it was dropped; entries whose input is 0 - masked
    keys - are recorded as kept: they contribute nothing either way).  nn.MultiheadAttention's explicit path
    (need_weights=True, temporal_attention.py:70) calls it on the softmax weights [N*H, 1, K], row n*H + h."""

    def __init__(self):
        import torch.nn.functional as F
        self.F, self.real, self.masks = F, F.dropout, []

    def __enter__(self):
        def rec(input, p=0.5, training=True, inplace=False):
            out = self.real(input, p, training, False)
            if training and p > 0:
                kept = (out != 0) | (input == 0)
                self.masks.append((kept.float() / (1.0 - p)).numpy().copy())
            return out
        self.F.dropout = rec
        return self

    def __exit__(self, *a):
        self.F.dropout = self.real


def g8():
    R = ref_modules()
    out = {}
    # (a) the layer alone, two rates, all-padding rows and partial masks as in g4
    for tag, pdrop in (("p10", 0.1), ("p50", 0.5)):
        torch.manual_seed(3); rs = np.random.RandomState(3)
        D, Ef, K, N, H = 12, 4, 6, 40, 2
        att = R.TemporalAttentionLayer(D, D, Ef, D, output_dimension=D, n_head=H, dropout=pdrop)
        att.train()
        with torch.no_grad():
            att.multi_head_target.in_proj_bias.normal_(0, 0.2); att.multi_head_target.out_proj.bias.normal_(0, 0.2)
        xs = torch.randn(N, D, requires_grad=True); tq = torch.randn(N, 1, D, requires_grad=True)
        nb = torch.randn(N, K, D, requires_grad=True); tn = torch.randn(N, K, D, requires_grad=True); ef = torch.randn(N, K, Ef)
        mask = torch.zeros(N, K, dtype=torch.bool)
        mask[:8] = True
        for i in range(8, 24):
            mask[i, :rs.randint(1, K)] = True
        with DropoutLog() as log:
            o, wts = att(xs, tq, nb, tn, ef, mask.clone())
        assert len(log.masks) == 1 and log.masks[0].shape == (N * H, 1, K)
        go = torch.randn(N, D)
        o.backward(go)
        pre = "att_%s_" % tag
        out.update({pre + "p": np.array(pdrop), pre + "drop": log.masks[0].reshape(N, H, K),
                    pre + "x": xs.detach().numpy(), pre + "tq": tq.detach().numpy()[:, 0], pre + "nb": nb.detach().numpy(),
                    pre + "tn": tn.detach().numpy(), pre + "ef": ef.numpy(), pre + "mask": mask.numpy(),
                    pre + "out": o.detach().numpy(), pre + "go": go.numpy(),
                    pre + "gx": xs.grad.numpy(), pre + "gtq": tq.grad.numpy()[:, 0], pre + "gnb": nb.grad.numpy(), pre + "gtn": tn.grad.numpy(),
                    **{pre + "p_" + k: v.detach().numpy() for k, v in att.named_parameters()},
                    **{pre + "g_" + k: v.grad.numpy() for k, v in att.named_parameters()}})
    out.update(D=np.array(12), Ef=np.array(4), K=np.array(6), H=np.array(2))
    # (b) one full training step of a 2-layer TGN with memory at dropout 0.1 (main.py:33 default --drop_out 0.1), state
    # injected like g5; the masks of the three attention calls in call order (layer 1 on the roots, layer 1 on their
    # neighbours, layer 2 on the roots: embedding_module.py:115,141,159)
    torch.manual_seed(2); np.random.seed(2)
    cfg = SyntheticConfig("g8", 120, 20, 1500, 16, 2, 5, 2)
    g = make_graph(cfg, with_prices=False)
    d = g.data
    D, Ef, K, B, n, L, H = cfg.dim, cfg.edge_dim, cfg.n_neighbors, 24, g.n_nodes, 2, 2
    M = 3 * D + Ef
    rdata = R.Data(d.sources, d.destinations, d.timestamps, d.edge_idxs, d.labels, d.portfolios)
    nf = R.get_neighbor_finder(rdata, uniform=False)
    tgn = R.TGN(neighbor_finder=nf, node_features=g.node_features, edge_features=g.edge_features.copy(), device=torch.device("cpu"),
                n_layers=L, n_heads=H, dropout=0.1, use_memory=True, message_dimension=100, memory_dimension=D,
                memory_update_at_start=True, embedding_module_type="graph_attention", message_function="identity",
                aggregator_type="last", memory_updater_type="gru", n_neighbors=K)
    with torch.no_grad():
        tgn.time_encoder.w.bias.copy_(torch.randn(D) * 0.3)
    opt = torch.optim.Adam(tgn.parameters(), lr=1e-3)
    rs = np.random.RandomState(4)
    out.update(step_L=np.array(L), step_H=np.array(H), step_K=np.array(K), step_p=np.array(0.1),
               src_all=d.sources, dst_all=d.destinations, ts_all=d.timestamps, eidx_all=d.edge_idxs,
               node_features=g.node_features, edge_features=g.edge_features)
    for step in range(3):
        s = 700 + step * B
        sb, db, tb, eb = d.sources[s:s + B], d.destinations[s:s + B], d.timestamps[s:s + B], d.edge_idxs[s:s + B]
        neg = rs.randint(cfg.n_users + 1, cfg.n_users + cfg.n_items + 1, size=(B, 3))
        record = step == 2
        if record:
            for k, v in tgn.state_dict().items():
                if not (k.startswith("memory_updater.memory.") or k.startswith("embedding_module.memory.")
                        or k.startswith("embedding_module.time_encoder.")):
                    out["s_sd_" + k] = v.detach().numpy().copy()
            tab, mt, cnt = dense_messages(tgn, n, M)
            out.update(s_msg_tab=tab, s_msg_t=mt, s_msg_cnt=cnt)
        tgn.train(); opt.zero_grad()
        with DropoutLog() as log:
            se, de, ne = tgn.compute_temporal_embeddings(sb, db, neg.flatten(), tb, eb, K)
        bs = se.shape[0]
        pos_scores = torch.sum(se.view(bs, 1, -1) * de.view(bs, 1, -1), dim=2)
        neg_scores = torch.matmul(se.view(bs, 1, -1), ne.view(bs, 3, -1).transpose(1, 2)).squeeze()
        loss = -torch.mean(torch.log(torch.sigmoid(torch.mean(pos_scores - neg_scores, dim=1))))
        loss.backward()
        if record:
            Rr = 5 * B
            assert [m.shape[0] for m in log.masks] == [Rr * H, Rr * K * H, Rr * H], [m.shape for m in log.masks]
            out.update(s_src=sb, s_dst=db, s_ts=tb, s_eidx=eb, s_neg=neg,
                       s_drop_l1=np.concatenate([log.masks[0].reshape(Rr, H, K), log.masks[1].reshape(Rr * K, H, K)]),
                       s_drop_l2=log.masks[2].reshape(Rr, H, K),
                       s_emb_src=se.detach().numpy(), s_emb_dst=de.detach().numpy(), s_emb_neg=ne.detach().numpy(),
                       s_loss=np.array(loss.item(), np.float32))
            for k, v in tgn.named_parameters():
                if v.requires_grad:
                    out["s_grad_" + k] = (v.grad.numpy().copy() if v.grad is not None else np.zeros(v.shape, np.float32))
        opt.step()
        tgn.memory.detach_memory()
        if record:
            tab, mt, cnt = dense_messages(tgn, n, M)
            out.update(s_after_memory=tgn.memory.memory.detach().numpy().copy(),
                       s_after_last_update=tgn.memory.last_update.detach().numpy().copy(),
                       s_after_msg_tab=tab, s_after_msg_t=mt, s_after_msg_cnt=cnt)
    save("g8_dropout", **out)


# ------------------------------------------------------------------ G9: evaluation loop with the investment metrics
def _finance_ref():
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import finance_ref
    return finance_ref


def _baseline_block():
    """evaluation.py's lines from ``if '' in portfolio:`` to the out-of-sample baseline (:153-172), compiled in place."""
    lines = open(os.path.join(REF, "evaluation.py")).read().split("\n")
    a = next(i for i, l in enumerate(lines) if l.strip().startswith("if '' in portfolio"))
    b = next(i for i, l in enumerate(lines) if "Sort the pos and neg items" in l)
    return compile(textwrap.dedent("\n".join(lines[a:b])), "<reference evaluation.py:153-172>", "exec")


def _ref_invest(ev, block, ts_key, portfolio, items, tf_past, tf_future, period=30):
    """One interaction of evaluation.py:146-190 through the reference's own code; ``items`` = stock codes in ranked order."""
    ns = dict(np=np, portfolio=portfolio, ts=ts_key, time_feature_past=tf_past, time_feature_future=tf_future, period=period)
    exec(block, ns)
    out = np.zeros(12)
    for t, (pf, r, s, tf) in enumerate(((ns["port_feature"], ns["return_"], ns["sharpe"], tf_past),
                                        (ns["port_feature_"], ns["return__"], ns["sharpe_"], tf_future))):
        for i, k in enumerate((1, 3, 5)):
            dr, ds = ev.return_sharpe_at_k(ts_key, pf, r, s, tf, items, k)
            out[t * 6 + i], out[t * 6 + 3 + i] = dr, ds
    return out


def _exact_invest(F, ret_past_day, ret_future_day, portfolio, map_item_id, top_idx):
    port = [] if "" in portfolio else [map_item_id[c] for c in portfolio]
    x, scale = F.invest_metrics(ret_past_day, ret_future_day, port, top_idx, dtype=np.longdouble, parts=True)
    hi = x.astype(np.float64)
    return hi, (x - hi).astype(np.float64), scale.astype(np.float64)


def _check_signs(F, ref, hi, lo, scale):
    """No golden value within the test's bar of zero except exact zeros: the '>0' shares then compare exactly."""
    e_ref = np.abs((ref - hi) - lo)
    bar = F.invest_bar(e_ref.max(), scale)
    near = (np.abs(ref) <= bar) & (ref != 0)
    assert not near.any(), (ref[near], bar[near])
    return e_ref


def g9a():
    """pfo_eval_metrics, kernel level: score rows [positive | 25 negatives] as g6's, scores multiples of 1/64 (any f32
    summation order reproduces them from the embeddings the test builds), candidate ids, portfolios, past / future prices;
    expected values from the reference's return_sharpe_at_k and baseline lines fed the canonical ranking."""
    import evaluation as ev
    from pfotgnrec_amd.mv_sampler import log_returns
    F = _finance_ref()
    block = _baseline_block()
    rs = np.random.RandomState(29)
    B, N, U, I, n_days, W = 120, 25, 50, 40, 4, 7
    codes = ["%06d" % (i + 1) for i in range(I)]
    map_item_id = {c: i for i, c in enumerate(codes)}
    days = ["2020010%d" % (d + 1) for d in range(n_days)]
    past = 100.0 * np.exp(np.cumsum(rs.randn(n_days, I, 30) * 0.02, axis=2))
    future = 100.0 * np.exp(np.cumsum(rs.randn(n_days, I, 30) * 0.02 + 0.001, axis=2))
    tf_past = {d: {c: past[k, j] for j, c in enumerate(codes)} for k, d in enumerate(days)}
    tf_future = {d: {c: future[k, j] for j, c in enumerate(codes)} for k, d in enumerate(days)}
    ret_past, ret_future = log_returns(past), log_returns(future)
    day_idx = rs.randint(0, n_days, B)
    ts = np.array([float(days[d]) * 1e6 + rs.randint(0, 235959) for d in day_idx])          # YYYYMMDDhhmmss
    assert all(str(t)[:8] == days[d] for t, d in zip(ts, day_idx))
    scores = np.zeros((B, 1 + N), np.float32)
    cand = np.zeros((B, 1 + N), np.int64)
    kind = np.zeros(B, np.int64)
    for b in range(B):
        k = kind[b] = b % 10
        scores[b] = rs.choice(np.arange(-400, 400), 1 + N, replace=False) / 64.0            # distinct, |s| < 8
        cand[b] = U + 1 + rs.choice(I, 1 + N, replace=False)
        order = np.argsort(scores[b, 1:])[::-1] + 1                                          # negatives, best first
        if k == 4:                                           # the destination among its own negatives (utils.py:96): an exact tie
            j = 1 + rs.randint(N); cand[b, j] = cand[b, 0]; scores[b, j] = scores[b, 0]
        elif k == 5:                                         # several negatives tie with the positive
            scores[b, 1 + rs.choice(N, 3, replace=False)] = scores[b, 0]
        elif k == 6:                                         # ties among negatives that straddle the top-1 / 3 / 5 boundary
            kk = (1, 3, 5)[(b // 10) % 3]
            scores[b, 0] = scores[b].min() - 1.0
            scores[b, order[kk]] = scores[b, order[kk - 1]]
            if (b // 10) % 2:                                # ... a group of three across it
                scores[b, order[kk + 1]] = scores[b, order[kk - 1]]
        elif k == 7:                                         # everything equal
            scores[b, :] = 0.25
        elif k == 8:                                         # one stock drawn twice (with replacement) inside the top 5
            i0, i1 = order[(b // 10) % 3], order[3]
            cand[b, i1] = cand[b, i0]; scores[b, i1] = scores[b, i0]
        elif k == 9:                                         # the positive on top / at the bottom
            scores[b, 0] = scores[b].max() + 1.0 if (b // 10) % 2 else scores[b].min() - 1.0
    assert np.all(np.abs(scores) < 8) and np.array_equal(scores * 64, np.round(scores * 64))
    canon = np.stack([F.canonical_order(scores[b]) for b in range(B)])
    refrank = np.stack([np.argsort(scores[b])[::-1] for b in range(B)])                      # evaluation.py:122
    tie_free = np.array([[F.tie_free(scores[b], k) for k in (1, 3, 5)] for b in range(B)])
    portfolios = []
    for b in range(B):
        k = b % 9
        top1 = codes[cand[b, canon[b, 0]] - U - 1]
        if k == 0:
            pf = [""]
        elif k == 1:
            pf = [top1]                                      # the recommended stock is the whole portfolio: delta = 0 exactly
        elif k == 2:
            pf = ["", codes[rs.randint(I)], codes[rs.randint(I)]]   # '' mixed in: the whole list counts as empty (:153)
        elif k == 3:
            pf = [codes[j] for j in rs.choice(I, W, replace=False)]  # the packed width
        else:
            pf = [codes[j] for j in rs.choice(I, rs.randint(1, W), replace=False)]
        portfolios.append(pf)
    width = max(len(p) for p in portfolios)
    port_codes = np.full((B, width), "", dtype="U6")
    port_n = np.array([len(p) for p in portfolios])
    for b, p in enumerate(portfolios):
        port_codes[b, :len(p)] = p
    invest = np.zeros((B, 12)); invest_refrank = np.zeros((B, 12))
    hi = np.zeros((B, 12)); lo = np.zeros((B, 12)); scale = np.zeros((B, 12))
    inv_code = {v: k for k, v in map_item_id.items()}
    for b in range(B):
        key = str(ts[b])[:8]
        items = np.array([inv_code[i] for i in cand[b] - (U + 1)])                           # evaluation.py:131-134
        invest[b] = _ref_invest(ev, block, key, portfolios[b], items[canon[b]], tf_past, tf_future)
        invest_refrank[b] = _ref_invest(ev, block, key, portfolios[b], items[refrank[b]], tf_past, tf_future)
        hi[b], lo[b], scale[b] = _exact_invest(F, ret_past[day_idx[b]], ret_future[day_idx[b]], portfolios[b], map_item_id,
                                               (cand[b] - U - 1)[canon[b]][:5])
    free_all = tie_free.all(1)
    assert free_all.sum() * 2 >= B, free_all.sum()
    assert np.array_equal(invest[free_all], invest_refrank[free_all])        # the reference's own ranking: identical metrics there
    e_ref = _check_signs(F, invest, hi, lo, scale)
    assert np.all(invest[np.arange(B) % 9 == 1][:, [0, 3, 6, 9]] == 0)       # portfolio == [top-1]: delta@1 is exactly 0
    n_greater = (scores[:, 1:] > scores[:, :1]).sum(1); n_equal = (scores[:, 1:] == scores[:, :1]).sum(1)
    print("g9a: %d / %d rows tie-free for all k; max e_ref %.3g" % (free_all.sum(), B, e_ref.max()))
    save("g9a_invest_metrics", scores=scores, cand=cand, kind=kind, ts=ts, day_idx=day_idx, days=np.array(days), codes=np.array(codes),
         upper_u=np.array(U), prices_past=past, prices_future=future, port_codes=port_codes, port_n=port_n,
         canonical=canon, ref_ranking=refrank, tie_free=tie_free, n_greater=n_greater, n_equal=n_equal,
         invest=invest, invest_ref_ranking=invest_refrank, invest_exact_hi=hi, invest_exact_lo=lo, invest_scale=scale)


def g12():
    """pfo_list_metrics at depths the reference's call sites never use: return_sharpe_at_k takes any k, only its callers say
    1, 3, 5.  Lists of 20 ranked stocks, cutoffs (1, 2, 3, 5, 10, 20), portfolios of 0..7 stocks (some with a stock twice, some
    lists naming a held stock), n_ret = 29, 4 days; expected values from the reference's return_sharpe_at_k and baseline lines
    (g9a's pattern) and its recall_at_k / ndcg_at_k, plus the restatement of tests/list_metrics_ref.py in extended precision."""
    import evaluation as ev
    from pfotgnrec_amd.mv_sampler import log_returns
    F = _finance_ref()
    import list_metrics_ref as LR
    block = _baseline_block()
    rs = np.random.RandomState(1212)
    B, L, U, I, n_days, W = 100, 20, 50, 40, 4, 7
    cuts = (1, 2, 3, 5, 10, 20)
    n_c = len(cuts)
    codes = ["%06d" % (i + 1) for i in range(I)]
    map_item_id = {c: i for i, c in enumerate(codes)}
    days = ["2020010%d" % (d + 1) for d in range(n_days)]
    past = 100.0 * np.exp(np.cumsum(rs.randn(n_days, I, 30) * 0.02, axis=2))
    future = 100.0 * np.exp(np.cumsum(rs.randn(n_days, I, 30) * 0.02 + 0.001, axis=2))
    tf_past = {d: {c: past[k, j] for j, c in enumerate(codes)} for k, d in enumerate(days)}
    tf_future = {d: {c: future[k, j] for j, c in enumerate(codes)} for k, d in enumerate(days)}
    ret_past, ret_future = log_returns(past), log_returns(future)
    day_idx = rs.randint(0, n_days, B)
    ts = np.array([float(days[d]) * 1e6 + rs.randint(0, 235959) for d in day_idx])
    assert all(str(t)[:8] == days[d] for t, d in zip(ts, day_idx))
    stocks = np.stack([rs.choice(I, L, replace=False) for _ in range(B)])              # the ranked lists, best first
    list_item = (U + 1 + stocks).astype(np.int64)
    portfolios, truth = [], np.zeros(B, np.int64)
    for b in range(B):
        k = b % 10
        rest = np.setdiff1d(np.arange(I), stocks[b])
        if k == 0:
            pf = [""]
        elif k == 1:
            pf = [codes[stocks[b, 0]]]                       # the first pick is the whole portfolio: delta@1 = 0 exactly
        elif k == 2:
            j = rs.choice(rest, 2, replace=False)
            pf = [codes[j[0]], codes[j[1]], codes[j[0]]]     # one stock held twice
        elif k == 3:
            pf = [codes[j] for j in rs.choice(I, W, replace=False)]                    # the packed width
        elif k == 4:
            pf = [codes[j] for j in rs.choice(rest, 3, replace=False)] + [codes[stocks[b, rs.randint(1, L)]]]   # a held stock in the list
        elif k == 5:
            j = stocks[b, rs.randint(0, 5)]
            pf = [codes[j], codes[j], codes[rs.choice(rest)]]                          # ... held twice and recommended again
        else:
            pf = [codes[j] for j in rs.choice(I, rs.randint(1, W), replace=False)]
        portfolios.append(pf)
        m = (b // 10) % 5                                    # the item taken: first, inside, last, not in the list, none
        truth[b] = (list_item[b, 0], list_item[b, rs.randint(1, L - 1)], list_item[b, L - 1], U + 1 + rs.choice(rest), -1)[m]
    width = max(len(p) for p in portfolios)
    port_codes = np.full((B, width), "", dtype="U6")
    port_n = np.array([len(p) for p in portfolios])
    port_idx = np.full((B, width), -1, np.int32)
    port_len = np.zeros(B, np.int32)
    for b, p in enumerate(portfolios):
        port_codes[b, :len(p)] = p
        if "" not in p:
            port_idx[b, :len(p)] = [map_item_id[c] for c in p]
            port_len[b] = len(p)
    invest = np.zeros((B, 4 * n_c))
    recall, ndcg = np.zeros((B, n_c)), np.zeros((B, n_c))
    for b in range(B):
        key = str(ts[b])[:8]
        items = np.array([codes[i] for i in stocks[b]])
        ns = dict(np=np, portfolio=portfolios[b], ts=key, time_feature_past=tf_past, time_feature_future=tf_future, period=30)
        exec(block, ns)
        for t, (pf, r, s, tf) in enumerate(((ns["port_feature"], ns["return_"], ns["sharpe"], tf_past),
                                            (ns["port_feature_"], ns["return__"], ns["sharpe_"], tf_future))):
            for i, c in enumerate(cuts):
                dr, ds = ev.return_sharpe_at_k(key, pf, r, s, tf, items, c)
                invest[b, t * 2 * n_c + i], invest[b, t * 2 * n_c + n_c + i] = dr, ds
        if truth[b] >= 0:
            for i, c in enumerate(cuts):
                recall[b, i] = ev.recall_at_k(list(list_item[b]), [truth[b]], c)
                ndcg[b, i] = ev.ndcg_at_k(list(list_item[b]), [truth[b]], c)
    args = (list_item, None, truth, cuts, port_idx, port_len, U, ret_past, day_idx, ret_future, day_idx)
    rank, hits, nd, x, scale = LR.list_metrics(*args, dtype=np.longdouble, parts=True)
    hi = x.astype(np.float64)
    lo = (x - hi).astype(np.float64)
    scale = scale.astype(np.float64)
    e_ref = _check_signs(F, invest, hi, lo, scale)
    assert np.array_equal(hits.astype(np.float64), recall) and np.allclose(nd, ndcg, rtol=0, atol=1e-6)
    assert np.all(invest[np.arange(B) % 10 == 1][:, [0, n_c, 2 * n_c, 3 * n_c]] == 0)
    print("g12: max e_ref %.3g over %d values" % (e_ref.max(), invest.size))
    save("g12_list_metrics", list_item=list_item, truth=truth, cutoffs=np.array(cuts), ts=ts, day_idx=day_idx, days=np.array(days),
         codes=np.array(codes), upper_u=np.array(U), prices_past=past,
         prices_future=future, port_codes=port_codes, port_n=port_n, port_idx=port_idx, port_len=port_len, rank=rank, recall=recall,
         ndcg=ndcg, invest=invest, invest_exact_hi=hi, invest_exact_lo=lo, invest_scale=scale, e_ref_max=np.array(e_ref.max()))


def _g9b_try(seed, L):
    import contextlib, io, pickle, tempfile
    import evaluation as ev
    from pfotgnrec_amd.mv_sampler import log_returns
    F = _finance_ref()
    R = ref_modules()
    torch.manual_seed(seed); np.random.seed(seed)
    rs = np.random.RandomState(seed)
    U, I, E, D, Ef, K, H, B = 30, 12, 400, 8, 4, 5, 2, 12
    M = 3 * D + Ef
    n = U + I + 1
    src = rs.randint(1, U + 1, E); dst = rs.randint(U + 1, U + I + 1, E)
    day_vals = np.sort(rs.choice(np.arange(10_000_000, 16_000_000), 40, replace=False))      # 8 digits: str(ts)[:8] is the value
    ts = np.sort(day_vals[rs.randint(0, 40, E)]).astype(np.float64)
    eidx = np.arange(1, E + 1)
    node_feat = rs.randn(n, D); edge_feat = rs.randn(E + 1, Ef); edge_feat[0] = 0
    codes = ["%06d" % (i + 1) for i in range(I)]
    map_item_id = {c: i for i, c in enumerate(codes)}
    portfolios = np.empty(E, dtype=object)
    for e in range(E):
        k = rs.randint(0, 6)
        pf = [codes[j] for j in rs.choice(I, k, replace=False)] if k else [""]
        if k and rs.rand() < 0.1:
            pf = pf + [""]                                                                    # '' mixed into a non-empty list
        portfolios[e] = pf
    days = [str(float(v))[:8] for v in day_vals]
    past = 100.0 * np.exp(np.cumsum(rs.randn(40, I, 30) * 0.02, axis=2))
    future = 100.0 * np.exp(np.cumsum(rs.randn(40, I, 30) * 0.02 + 0.001, axis=2))
    tf_past = {d: {c: past[k, j] for j, c in enumerate(codes)} for k, d in enumerate(days)}
    tf_future = {d: {c: future[k, j] for j, c in enumerate(codes)} for k, d in enumerate(days)}
    full = R.Data(src, dst, ts, eidx, np.zeros(E, np.int64), portfolios)
    nf = R.get_neighbor_finder(full, uniform=False)
    tgn = R.TGN(neighbor_finder=nf, node_features=node_feat, edge_features=edge_feat.copy(), device=torch.device("cpu"),
                n_layers=L, n_heads=H, dropout=0.1, use_memory=True, message_dimension=100, memory_dimension=D,
                memory_update_at_start=True, embedding_module_type="graph_attention", message_function="identity",
                aggregator_type="last", memory_updater_type="gru", n_neighbors=K)
    with torch.no_grad():
        tgn.time_encoder.w.bias.copy_(torch.randn(D) * 0.3)
        tgn.eval()
        for w in (200, 212, 224, 236):                                                                 # memory and pending messages to start from
            sl = slice(w, w + B)
            tgn.compute_temporal_embeddings(src[sl], dst[sl], dst[sl].repeat(2), ts[sl], eidx[sl], K)
    n_run = 5
    first, n_eval = 248, n_run * B + 7                                                       # 6 batches: 5 run, the short last one is skipped
    sl = slice(first, first + n_eval)
    data = R.Data(src[sl], dst[sl], ts[sl], eidx[sl], np.zeros(n_eval, np.int64), portfolios[sl])
    sd = {k: v.detach().numpy().copy() for k, v in tgn.state_dict().items()
          if not (k.startswith("memory_updater.memory.") or k.startswith("embedding_module.memory.")
                  or k.startswith("embedding_module.time_encoder."))}
    tab, mt, cnt = dense_messages(tgn, n, M)
    out = dict(L=np.array(L), H=np.array(H), K=np.array(K), batch=np.array(B), upper_u=np.array(U), seed=np.array(seed),
               src_all=src, dst_all=dst, ts_all=ts, eidx_all=eidx, node_features=node_feat, edge_features=edge_feat,
               eval_first=np.array(first), eval_n=np.array(n_eval), codes=np.array(codes), days=np.array(days),
               prices_past=past, prices_future=future, msg_tab=tab, msg_t=mt, msg_cnt=cnt,
               memory0=tgn.memory.memory.detach().numpy().copy(), last_update0=tgn.memory.last_update.detach().numpy().copy())
    width = max(len(p) for p in portfolios)
    pc = np.full((E, width), "", dtype="U6")
    for e, p in enumerate(portfolios):
        pc[e, :len(p)] = p
    out.update(port_codes=pc, port_n=np.array([len(p) for p in portfolios]))
    for k, v in sd.items():
        out["sd_" + k] = v
    neg_log, emb_log = [], []

    class RecSampler(R.RandEdgeSampler):                     # records the draw, changes nothing
        def sample(self, size):
            r = super().sample(size); neg_log.append(r.copy()); return r
    orig_cte = tgn.compute_temporal_embeddings

    def rec_cte(*a, **k):
        r = orig_cte(*a, **k); emb_log.append([t.detach().numpy().copy() for t in r]); return r
    tgn.compute_temporal_embeddings = rec_cte
    cwd, keep = os.getcwd(), ev.RandEdgeSampler
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "data", "period_30"))
        for name, obj in (("time_feature_past_30.pkl", tf_past), ("time_feature_future_30.pkl", tf_future), ("map_item_id.pkl", map_item_id)):
            with open(os.path.join(tmp, "data", "period_30", name), "wb") as f:
                pickle.dump(obj, f)
        os.chdir(tmp)
        ev.RandEdgeSampler = RecSampler
        try:
            with contextlib.redirect_stderr(io.StringIO()):
                result = ev.eval_recommendation(tgn, data, full, B, K, U, 30, False, "val")
        finally:
            os.chdir(cwd); ev.RandEdgeSampler = keep
            del tgn.compute_temporal_embeddings
    assert len(neg_log) == n_run and len(emb_log) == n_run
    # per-interaction lists recomputed from the recorded scores with the reference's functions, under the canonical ranking
    block = _baseline_block()
    inv_code = {v: k for k, v in map_item_id.items()}
    ret_past, ret_future = log_returns(past), log_returns(future)
    day_of = {d: i for i, d in enumerate(days)}
    n_rows = n_run * B
    scores = np.zeros((n_rows, 1 + I), np.float32); canon = np.zeros((n_rows, 1 + I), np.int64); rank = np.zeros(n_rows, np.int64)
    recall_ref = np.zeros((n_rows, 3)); ndcg_ref = np.zeros((n_rows, 3)); self_tie = np.zeros(n_rows, bool)
    recall = np.zeros((n_rows, 3)); ndcg = np.zeros((n_rows, 3)); invest = np.zeros((n_rows, 12))
    hi = np.zeros((n_rows, 12)); lo = np.zeros((n_rows, 12)); scale = np.zeros((n_rows, 12))
    top5_item = np.zeros((n_rows, 5), np.int64)
    worst_gap = np.inf
    for bi in range(n_run):
        se, de, ne = (torch.from_numpy(x) for x in emb_log[bi])
        pos = torch.sum(se.view(B, 1, -1) * de.view(B, 1, -1), dim=2).numpy()               # evaluation.py:114-115
        negs = torch.sum(se.view(B, 1, -1) * ne.view(B, I, -1), dim=2).numpy()
        for i in range(B):
            r = bi * B + i
            e = first + r
            s = scores[r] = np.concatenate((pos[i], negs[i]))
            ids = np.concatenate(([dst[e]], neg_log[bi][i]))
            order = canon[r] = F.canonical_order(s)
            refo = np.argsort(s)[::-1]
            rank[r] = int(np.where(order == 0)[0][0])
            # the gap condition: adjacent scores among the six best and around the positive differ by > 1e-3 of max |score|,
            # except exact ties between two draws of ONE stock (either order selects the same stock)
            sorted_s, sorted_id = s[order], ids[order]
            for j in sorted(set(range(0, 6)) | {rank[r] - 1, rank[r]}):
                if j < 0 or j + 1 > I:
                    continue
                gap = float(sorted_s[j]) - float(sorted_s[j + 1])
                if gap == 0 and sorted_id[j] == sorted_id[j + 1]:
                    continue
                worst_gap = min(worst_gap, gap / float(np.abs(s).max()))
            assert np.array_equal(ids[order][:5], ids[refo][:5])                              # the reference's own order: same stocks
            recall[r] = [ev.recall_at_k(order, [0], k) for k in (1, 3, 5)]
            ndcg[r] = [ev.ndcg_at_k(order, [0], k) for k in (1, 3, 5)]
            # the reference's own np.argsort is not stable (evaluation.py:122): where the destination is among its own negatives
            # (utils.py:96; every empty-portfolio row) it places the positive anywhere among those exact ties, the canonical order
            # last.  Nowhere else may the two differ.
            recall_ref[r] = [ev.recall_at_k(refo, [0], k) for k in (1, 3, 5)]
            ndcg_ref[r] = [ev.ndcg_at_k(refo, [0], k) for k in (1, 3, 5)]
            self_tie[r] = bool(np.any((ids[1:] == ids[0]) & (s[1:] == s[0])))
            rank_ref = int(np.where(refo == 0)[0][0])
            assert rank_ref == rank[r] or (self_tie[r] and rank[r] - int(((ids[1:] == ids[0]) & (s[1:] == s[0])).sum()) <= rank_ref < rank[r])
            items = np.array([inv_code[x] for x in ids - (U + 1)])
            invest[r] = _ref_invest(ev, block, str(ts[e])[:8], portfolios[e], items[order], tf_past, tf_future)
            d = day_of[str(ts[e])[:8]]
            top5_item[r] = ids[order][:5]
            hi[r], lo[r], scale[r] = _exact_invest(F, ret_past[d], ret_future[d], portfolios[e], map_item_id, (ids - U - 1)[order][:5])
    if not worst_gap > 1e-3:
        return None, worst_gap
    # the reference's dict is what these lists average to: its own ranking picked the same stocks, and the same rank of the
    # positive except among exact ties with its own duplicate (recall / NDCG under its ranking: *_ref; under the canonical: the
    # six 'canonical' values the native path has to give)
    mine, canonical = {}, {}
    for name, a, c in (("recall", recall_ref, recall), ("ndcg", ndcg_ref, ndcg)):
        for j, k in enumerate((1, 3, 5)):
            mine["val_%s_avg_%d" % (name, k)] = np.mean([a[i][j] for i in range(n_rows)])
            canonical["val_%s_avg_%d" % (name, k)] = np.mean([c[i][j] for i in range(n_rows)])
    for t, suf in ((0, ""), (1, "_")):
        for m, name in ((0, "return"), (1, "sharpe")):
            for j, k in enumerate((1, 3, 5)):
                col = [invest[i][t * 6 + m * 3 + j] for i in range(n_rows)]
                mine["val_%s_avg_%d%s" % (name, k, suf)] = np.mean(col)
                mine["val_%s_percent_%d%s" % (name, k, suf)] = len([x for x in col if x > 0]) / n_rows
    assert set(mine) == set(result) and len(result) == 30
    for k in result:
        assert mine[k] == result[k], (k, mine[k], result[k])
    e_ref = _check_signs(F, invest, hi, lo, scale)
    tab, mt, cnt = dense_messages(tgn, n, M)
    out.update(negatives=np.stack(neg_log), scores=scores, canonical=canon, rank=rank, recall=recall, ndcg=ndcg, invest=invest,
               top5_item=top5_item, invest_exact_hi=hi, invest_exact_lo=lo, invest_scale=scale,
               result_keys=np.array(list(result)), result_values=np.array([result[k] for k in result], np.float64),
               canonical_values=np.array([canonical.get(k, result[k]) for k in result], np.float64), self_tie=self_tie,
               recall_ref_ranking=recall_ref, ndcg_ref_ranking=ndcg_ref,
               after_memory=tgn.memory.memory.detach().numpy().copy(), after_last_update=tgn.memory.last_update.detach().numpy().copy(),
               after_msg_tab=tab, after_msg_t=mt, after_msg_cnt=cnt, worst_gap=np.array(worst_gap))
    print("g9b L%d seed %d: worst relative gap %.3g, max e_ref %.3g" % (L, seed, worst_gap, e_ref.max()))
    return out, worst_gap


def g9b():
    """eval_recommendation end to end: the reference's own loop (evaluation.py:39-264) on a tiny bipartite graph with the
    reference TGN on the CPU (memory, GRU, L in {1, 2}), synthetic data/period_30/*.pkl in a temporary directory; its
    RandEdgeSampler and compute_temporal_embeddings are wrapped only to RECORD.  The seed is the first for which every
    interaction meets the score-gap condition (see _g9b_try): a native embedding within the project's 1e-4 bar cannot reorder
    the candidates that matter."""
    for L in (1, 2):
        for seed in range(100, 400):
            out, gap = _g9b_try(seed, L)
            if out is not None:
                save("g9b_eval_loop_L%d" % L, **out)
                break
            print("g9b L%d seed %d: worst relative gap %.3g - next seed" % (L, seed, gap))
        else:
            raise SystemExit("g9b: no seed met the gap condition")


# ------------------------------------------------------------------ G10: yyyymmddHHMMSS timestamps (f32 step = 2**21 ~ two days)
def real_timestamps(n, rs, first_day=(2023, 12, 1), n_days=60, n_dup=None, n_edge_of_day=8):
    """Sorted f64[n] ``yyyymmddHHMMSS`` timestamps, the format of the reference's data (main.py:212 takes ``str(ts)[:8]``):
    ``n_days`` calendar days from ``first_day`` (the default spans the 2023-12-31 -> 2024-01-01 boundary, a gap of ~8.87e9),
    several edges per day at 09:00:00-15:30:00, ``n_edge_of_day`` of them moved to 00:00:00 / 23:59:59 and ``n_dup``
    (default n // 12) exact f64 duplicates of other entries.  Near 2.02e13 one f32 step is 2**21: about two days."""
    import datetime
    d0 = datetime.date(*first_day)
    days = np.array([int((d0 + datetime.timedelta(int(k))).strftime("%Y%m%d")) for k in range(n_days)], np.int64)
    day = rs.randint(0, n_days, n)
    sec = rs.randint(9 * 3600, 15 * 3600 + 30 * 60 + 1, n)
    edge = rs.choice(n, n_edge_of_day, replace=False)
    sec[edge[:n_edge_of_day // 2]] = 0
    sec[edge[n_edge_of_day // 2:]] = 86399
    hms = (sec // 3600) * 10000 + (sec // 60 % 60) * 100 + sec % 60
    ts = (days[day] * 1_000_000 + hms).astype(np.float64)            # < 2**53: exact
    dup = rs.choice(n, n // 12 if n_dup is None else n_dup, replace=False)
    ts[dup] = ts[rs.randint(0, n, len(dup))]
    return np.sort(ts)


def _stable_rows(nf, nodes, ts, draws, K):
    """The canonical output of one uniform sampler call (App. A-9): the drawn entries stable-sorted by their f32 time."""
    N = len(nodes)
    nbr = np.zeros((N, K), np.int32); eidx = np.zeros((N, K), np.int32); et = np.zeros((N, K), np.float32)
    for i, (a, b) in enumerate(zip(nodes, ts)):
        h_n, h_e, h_t = nf.find_before(a, b)
        if len(h_n) > 0:
            sel = draws[i]
            t32 = h_t[sel].astype(np.float32)
            pos = np.argsort(t32, kind="stable")
            nbr[i], eidx[i], et[i] = h_n[sel][pos], h_e[sel][pos], t32[pos]
    return nbr, eidx, et


def readdress_draws(nf, calls, draws, K, L):
    """The reference logs the draws of the call on the NEIGHBOURS in the slot order its own (non-stable) argsort gave the call
    above; the canonical order is the stable one.  Per root of that call: a bijection reference slot -> canonical slot that
    preserves the edge (duplicate draws of one edge are interchangeable: the layer above sums over the slots), and the rows of
    the neighbour call's draws moved along it.  Returns the reference's rows per call (ref_nbr/eidx/et<j>), the canonical
    draws (cdraws<j>) and how many roots were moved."""
    assert len(calls) == len(draws) == (3 if L == 2 else 1)
    out = {}
    for j, (_, _, nb, ei, et) in enumerate(calls):
        out["ref_nbr%d" % j], out["ref_eidx%d" % j], out["ref_et%d" % j] = nb, ei, et
    cdraws = [dr.copy() for dr in draws]
    moved = 0
    if L == 2:
        # call order (embedding_module.py:115,125,141): layer 1 on the roots, layer 2 on the roots, layer 1 on call 1's neighbours
        nodes, ts, r_nb, r_ei, r_et = calls[1]
        c_nb, c_ei, c_et = _stable_rows(nf, nodes, ts, draws[1], K)
        assert np.array_equal(c_et, r_et)                         # the times are sorted either way
        N = len(nodes)
        assert np.array_equal(calls[2][0], r_nb.flatten()) and np.array_equal(calls[2][1], np.repeat(ts, K))
        for i in range(N):
            free = list(range(K))
            perm = np.zeros(K, np.int64)
            for s in range(K):
                c = next(c for c in free if c_ei[i, c] == r_ei[i, s] and c_et[i, c] == r_et[i, s])
                free.remove(c)
                perm[s] = c
                assert c_nb[i, c] == r_nb[i, s]
            moved += int(not np.array_equal(perm, np.arange(K)))
            cdraws[2][i * K + perm] = draws[2][i * K:(i + 1) * K]
        # every re-addressed draw is a position in ITS node's history
        for r, (a, b) in enumerate(zip(c_nb.flatten(), np.repeat(ts, K))):
            cnt = len(nf.find_before(a, b)[0])
            row = cdraws[2][r]
            assert (cnt == 0 and np.all(row == -1)) or (cnt > 0 and np.all((row >= 0) & (row < cnt))), (r, a, b, cnt, row)
    for j, dr in enumerate(cdraws):
        out["cdraws%d" % j] = dr
    out["n_readdressed_roots"] = np.array(moved)
    return out


def g10():
    """(a) g10_realts_sampler: the g1 recipe on a small bipartite graph with real timestamps: most-recent K in {10, 3},
    uniform K = 5 with the draws logged, ``dt`` by the reference's expression (embedding_module.py:133-135: f64 query time
    minus f32 edge time, then .float()), the counts the sensitivity tests rely on, and the day key of every interaction.
    (b) g10_realts_step_*: the g5 recipe (narrower features: the files stay below the size of g5's) on the same timestamps."""
    R = ref_modules()
    rs = np.random.RandomState(10)
    U, I, E = 60, 12, 1200
    src = rs.randint(1, U - 2, size=E)                            # users U-2..U never interact
    dst = rs.randint(U + 1, U + I + 1, size=E)
    ts = real_timestamps(E, rs)
    eidx = np.arange(1, E + 1)
    t32 = ts.astype(np.float32)
    print("g10: %d distinct f64 timestamps, %d distinct f32" % (len(np.unique(ts)), len(np.unique(t32))))
    assert len(np.unique(ts)) < E and len(np.unique(t32)) * 10 < len(np.unique(ts))
    keys = np.array([str(t)[:8] for t in ts])                     # main.py:212, per interaction
    assert len(set(k[:4] for k in keys)) == 2 and any(str(t)[8:14] == "000000" for t in ts) and any(str(t)[8:14] == "235959" for t in ts)
    D = R.Data(src, dst, ts, eidx, np.zeros(E), None)
    nf = R.get_neighbor_finder(D, uniform=False)
    sl = slice(500, 756)
    extra = real_timestamps(192, rs, n_dup=0)                     # cut times that are (mostly) no edge's time
    q_nodes = np.concatenate([src[sl], dst[sl], rs.randint(0, U + I + 1, len(extra)), np.arange(0, U + I + 1)])
    q_ts = np.concatenate([ts[sl], ts[sl], extra, np.full(U + I + 1, ts[E // 2] + 1.0)])
    out = dict(src=src, dst=dst, ts=ts, eidx=eidx, q_nodes=q_nodes, q_ts=q_ts, day_keys=keys)

    def deltas(et):                                               # embedding_module.py:133-135
        return torch.from_numpy(q_ts[:, np.newaxis] - et).float().numpy()
    for K in (10, 3):
        nb, ei, et = nf.get_temporal_neighbor(q_nodes, q_ts, K)
        out["K%d_nbr" % K], out["K%d_eidx" % K], out["K%d_et" % K], out["K%d_dt" % K] = nb, ei, et, deltas(et)
    n_neg = int((out["K10_dt"] < 0).sum())
    newest = out["K10_et"][:, -1]
    has = out["K10_nbr"][:, -1] != 0
    n_same_step = int((has & (q_ts.astype(np.float32) == newest)).sum())
    n_rounded_past = int((has & (newest.astype(np.float64) > q_ts)).sum())
    # a query time cast to f32 in front of find_before selects another history on these rows
    n_f32_query = sum(int(len(nf.find_before(a, b)[0]) != len(nf.find_before(a, np.float32(b))[0])) for a, b in zip(q_nodes, q_ts))
    assert n_neg > 0 and n_same_step > 0 and n_rounded_past > 0 and n_f32_query > 0
    nfu = R.get_neighbor_finder(D, uniform=True)
    log, orig = [], np.random.randint

    def rec(lo, hi, n):
        r = orig(lo, hi, n); log.append(r.copy()); return r
    np.random.seed(12)
    np.random.randint = rec
    try:
        nb, ei, et = nfu.get_temporal_neighbor(q_nodes, q_ts, 5)
    finally:
        np.random.randint = orig
    draws = np.full((len(q_nodes), 5), -1, np.int64)
    it = iter(log)
    for i, (a, b) in enumerate(zip(q_nodes, q_ts)):
        if len(nf.find_before(a, b)[0]) > 0:
            draws[i] = next(it)
    n_tie = sum(int(any(et[i, a] == et[i, b] and ei[i, a] != ei[i, b] for a in range(5) for b in range(a))) for i in range(len(et))
                if nb[i].any())
    c_nb, c_ei, c_et = _stable_rows(nf, q_nodes, q_ts, draws, 5)
    n_unstable = int(((c_ei != ei).any(1)).sum())
    assert n_tie > 0 and np.array_equal(c_et, et)
    print("g10 sampler: %d negative dt, %d rows in the newest edge's f32 step, %d with f32(t_e) > t, %d rows move under an f32 "
          "query; uniform: %d rows tie between different edges, %d not in stable order" %
          (n_neg, n_same_step, n_rounded_past, n_f32_query, n_tie, n_unstable))
    out.update(uni_nbr=nb, uni_eidx=ei, uni_et=et, uni_dt=deltas(et), uni_draws=draws, uni_seed=np.array(12),
               n_negative_dt=np.array(n_neg), n_same_step_rows=np.array(n_same_step), n_rounded_past_rows=np.array(n_rounded_past),
               n_f32_query_rows=np.array(n_f32_query), uni_n_tie_rows=np.array(n_tie), uni_n_unstable_rows=np.array(n_unstable))
    save("g10_realts_sampler", **out)
    step_fixtures("g10_realts_step_", 12, real_timestamps(1500, np.random.RandomState(10)))


if __name__ == "__main__":
    import warnings
    warnings.filterwarnings("ignore")
    which = sys.argv[1:] or ["g1", "g2", "g3", "g4", "g5", "g6", "g7", "g8", "g9a", "g9b", "g10", "g11", "g12"]
    for w in which:
        globals()[w]()
