#!/usr/bin/env python3
"""The C2 evaluation batch of tools/bench_eval.py (512 interactions x all 500 items, forward only) under the three orders of
``eval_recommendation(order=)``: "score" (``pfo_eval_metrics``), "mv" and "basket" (``pfo_eval_metrics_mv``, mode 0 / 1).
One process, the orders alternating (rotated every round) from the same model state on the same batch: whole-call medians
(embeddings + the evaluation kernel) with [min, max], and the kernels alone by device events on one batch's embeddings."""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pfotgnrec_amd as P
from pfotgnrec_amd.synthetic import CONFIGS, make_graph

REPS = 9
cfg = CONFIGS["C2"]; g = make_graph(cfg, with_prices=True); d = g.data
dev = torch.device("cuda:0")
tgn = P.TGN(P.get_neighbor_finder(d, False), g.node_features, g.edge_features, dev, n_layers=2, n_heads=2, dropout=0.1,
            use_memory=True, memory_dimension=172, message_function="identity")
with torch.no_grad():
    tgn.memory.msg_table.normal_(0, 0.1); tgn.memory.memory.normal_(0, 0.1); tgn.memory.has_msg.fill_(1)
tgn.eval()
B, n_items, U = 512, cfg.n_items, cfg.n_users
t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
items = torch.arange(U + 1, U + 1 + n_items, dtype=torch.int32, device=dev).repeat(B)
future = g.prices * np.exp(np.cumsum(np.random.RandomState(3).randn(*g.prices.shape) * 0.01, axis=2))
tables = P.InvestTables.from_prices(list(range(cfg.n_days)), g.prices, future, g.map_item_id)
rp, rf = tables.device_tables(dev)
mv = P.MVSampler(g.prices, U, dev, gamma=2.0, lambda_mv=0.5, day_of=g.day_of)
MODES = {"score": None, "mv": 0, "basket": 1}


def batch(it):
    s = 900000 + it * B
    dst = t(d.destinations[s:s + B], np.int32)
    day = t(g.day_of(d.timestamps[s:s + B]), np.int32)
    return (t(d.sources[s:s + B], np.int32), dst, t(d.timestamps[s:s + B], np.float64), t(d.edge_idxs[s:s + B], np.int32),
            torch.cat([dst.view(B, 1), items.view(B, n_items)], 1), day, t(g.portfolio_idx[s:s + B], np.int32),
            t(g.portfolio_len[s:s + B], np.int32))


def metrics(order, emb, cand, day, pidx, plen):
    if MODES[order] is None:
        return P.eval_metrics(emb, B, n_items, cand, day, pidx, plen, rp, rf, U)
    return P.eval_metrics_mv(emb, B, n_items, cand, day, pidx, plen, rp, rf, U, mv.returns, day, mv.gamma, mv.lambda_mv, MODES[order])


def run(order, it):
    src, dst, ts, ei, cand, day, pidx, plen = batch(it)
    emb, _ = tgn.embed_device(src, dst, [items], [n_items], ts, ei, 20)
    return emb, metrics(order, emb, cand, day, pidx, plen)


state = (tgn.memory.memory.data, tgn.memory.last_update.data, tgn.memory.msg_table, tgn.memory.msg_time, tgn.memory.has_msg)
snap = [x.clone() for x in state]


def restore():
    for dst_t, src_t in zip(state, snap):
        dst_t.copy_(src_t)


ms = {o: [] for o in MODES}
names = list(MODES)
for rep in range(REPS + 1):                             # round 0 warms up
    for o in names[rep % 3:] + names[:rep % 3]:
        restore()                                       # every order sees the same state and the same batch
        torch.cuda.synchronize(); t0 = time.perf_counter()
        with torch.no_grad():
            run(o, 4 + rep)
        torch.cuda.synchronize()
        if rep:
            ms[o].append(1e3 * (time.perf_counter() - t0))
# the kernels alone, on one batch's embeddings (device events, 20 launches each after 3 warm-up launches, the orders in turn)
restore()
kern, out = {o: [] for o in MODES}, {}
with torch.no_grad():
    src, dst, ts, ei, cand, day, pidx, plen = batch(4)
    emb, _ = tgn.embed_device(src, dst, [items], [n_items], ts, ei, 20)
    for o in names:
        for _ in range(3):
            out[o] = metrics(o, emb, cand, day, pidx, plen)
    for _ in range(20):
        for o in names:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); metrics(o, emb, cand, day, pidx, plen); b.record()
            torch.cuda.synchronize()
            kern[o].append(1e3 * a.elapsed_time(b))
stat = lambda v, nd: {"median": round(float(np.median(v)), nd), "min": round(min(v), nd), "max": round(max(v), nd)}
rank = {o: out[o][0].cpu().numpy() for o in names}
res = {"what": "evaluation batch under the three orders (evaluation.py:63-207), C2, %d interactions x %d items" % (B, n_items), "reps": REPS,
       "lambda_mv": mv.lambda_mv}
for o in names:
    res["ms_whole_call_" + o] = stat(ms[o], 2)
    res["kernel_us_" + o] = stat(kern[o], 1)
    res["recall_at_5_" + o] = round(float((rank[o] < 5).mean()), 4)
    res["top1_return_in_sample_" + o] = float(out[o][5][:, 0].mean())
res["rows_whose_top5_differs_from_score"] = {o: int((out[o][3] != out["score"][3]).any(1).sum()) for o in ("mv", "basket")}
print(json.dumps(res))
