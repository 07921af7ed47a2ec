#!/usr/bin/env python3
"""Forward-only evaluation batch at C2 scale (evaluation.py:88-145: every interaction scores all items)."""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pfotgnrec_amd as P
from pfotgnrec_amd.synthetic import CONFIGS, make_graph
cfg = CONFIGS["C2"]; g = make_graph(cfg, with_prices="--invest" in sys.argv); d = g.data
dev = torch.device("cuda:0")
tgn = P.TGN(P.get_neighbor_finder(d, False), g.node_features, g.edge_features, dev, n_layers=2, n_heads=2, dropout=0.1,
            use_memory=True, memory_dimension=172, message_function="identity")
with torch.no_grad():
    tgn.memory.msg_table.normal_(0, 0.1); tgn.memory.memory.normal_(0, 0.1); tgn.memory.has_msg.fill_(1)
tgn.eval()
INVEST = "--invest" in sys.argv                     # the fused evaluation kernel against today's paths, see the end of the file
argv = [a for a in sys.argv[1:] if a != "--invest"]
if argv:
    tgn.eval_chunk_roots = int(argv[0])              # roots per forward-only pass (default 16384)
B, n_items = 512, cfg.n_items
t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
items = torch.arange(cfg.n_users + 1, cfg.n_users + 1 + n_items, dtype=torch.int32, device=dev).repeat(B)
times = []
for it in range(4):
    s = 900000 + it * B
    src, dst = t(d.sources[s:s + B], np.int32), t(d.destinations[s:s + B], np.int32)
    ts, ei = t(d.timestamps[s:s + B], np.float64), t(d.edge_idxs[s:s + B], np.int32)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    with torch.no_grad():
        emb, b = tgn.embed_device(src, dst, [items], [n_items], ts, ei, 20)
        rank, hits, ndcg = P.rank_metrics(emb, B, n_items)
    torch.cuda.synchronize(); times.append(time.perf_counter() - t0)
import json
print(json.dumps({"what": "evaluation batch (evaluation.py:63-145): forward only, every interaction scores all items, ranking on device",
                  "config": "C2 graph, L2 K20 D172 H2 memory+GRU", "interactions": B, "roots": B * (2 + n_items), "chunk_roots": tgn.eval_chunk_roots,
                  "ms_per_batch": round(1e3 * min(times), 2), "ms_all": [round(1e3 * x, 2) for x in times],
                  "interactions_per_s": round(B / min(times), 1), "root_embeddings_per_s": round(B * (2 + n_items) / min(times), 0),
                  "recall_at_5": round(hits[:, 2].mean().item(), 4)}))

if INVEST:
    # --invest: the same batch (a) as above: embeddings + rank_metrics; (b) = (a) + the per-interaction finance loop of
    # evaluation.py:146-207 on the host, fed the device scores (what a user of the four-import swap runs today; the numpy
    # restatement of tests/finance_ref.py in a Python loop per interaction, including the read-back of all scores);
    # (c) embeddings + pfo_eval_metrics.  Interleaved, REPS rounds after a warm-up round; medians and the spread.
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import finance_ref as F
    REPS = 9
    rs = np.random.RandomState(3)
    future = g.prices * np.exp(np.cumsum(rs.randn(*g.prices.shape) * 0.01, axis=2))
    tables = P.InvestTables.from_prices(list(range(cfg.n_days)), g.prices, future, g.map_item_id)
    rp, rf = tables.device_tables(dev)
    U = cfg.n_users

    def batch(it):
        s = 900000 + it * B
        return (s, t(d.sources[s:s + B], np.int32), t(d.destinations[s:s + B], np.int32), t(d.timestamps[s:s + B], np.float64),
                t(d.edge_idxs[s:s + B], np.int32))

    def side(s, dst):
        return (torch.cat([dst.view(B, 1), items.view(B, n_items)], 1), t(g.day_of(d.timestamps[s:s + B]), np.int32),
                t(g.portfolio_idx[s:s + B], np.int32), t(g.portfolio_len[s:s + B], np.int32))

    def run_a(it):
        s, src, dst, ts, ei = batch(it)
        emb, _ = tgn.embed_device(src, dst, [items], [n_items], ts, ei, 20)
        return emb, P.rank_metrics(emb, B, n_items)

    def run_b(it):
        s, src, dst, ts, ei = batch(it)
        emb, (rank, hits, ndcg) = run_a(it)
        e = emb.view(-1, emb.shape[1])
        sc = torch.cat([(e[:B] * e[B:2 * B]).sum(1, keepdim=True), torch.bmm(e[2 * B:].view(B, n_items, -1), e[:B].unsqueeze(2)).squeeze(2)], 1).cpu().numpy()
        day = g.day_of(d.timestamps[s:s + B])
        ids = np.concatenate([[0], np.arange(n_items)])
        out, top = np.empty((B, 12)), np.empty((B, 5), np.int64)
        for i in range(B):
            ids[0] = d.destinations[s + i] - U - 1
            order = F.canonical_order(sc[i])
            out[i] = F.invest_metrics(tables.returns_past[day[i]], tables.returns_future[day[i]],
                                      g.portfolio_idx[s + i, :g.portfolio_len[s + i]], ids[order[:5]])
            top[i] = ids[order[:5]] + U + 1
        return out, top

    def run_c(it):
        s, src, dst, ts, ei = batch(it)
        cand, day, pidx, plen = side(s, dst)
        emb, _ = tgn.embed_device(src, dst, [items], [n_items], ts, ei, 20)
        return emb, P.eval_metrics(emb, B, n_items, cand, day, pidx, plen, rp, rf, U)

    def timed(fn, it):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        with torch.no_grad():
            r = fn(it)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), r

    snap = [x.clone() for x in (tgn.memory.memory.data, tgn.memory.last_update.data, tgn.memory.msg_table, tgn.memory.msg_time, tgn.memory.has_msg)]

    def restore():
        for dst_t, src_t in zip((tgn.memory.memory.data, tgn.memory.last_update.data, tgn.memory.msg_table, tgn.memory.msg_time, tgn.memory.has_msg), snap):
            dst_t.copy_(src_t)
    ms = {"a": [], "b": [], "c": []}
    for rep in range(REPS + 1):
        order = [("a", run_a), ("c", run_c), ("b", run_b)]
        for name, fn in order[rep % 3:] + order[:rep % 3]:      # rotated: nobody is always the one behind the host loop's idle gap
            restore()                                   # every variant sees the same state and the same batch
            dt, r = timed(fn, 4 + rep)
            if rep > 0:
                ms[name].append(dt)
    # the kernels alone, on one batch's embeddings (device events, 20 launches each after 3 warm-up launches)
    restore()
    with torch.no_grad():
        emb, ev_out = run_c(4)
        s, src, dst, ts, ei = batch(4)
        cand, day, pidx, plen = side(s, dst)
        kern = {}
        for name, fn in (("rank_metrics", lambda: P.rank_metrics(emb, B, n_items)),
                         ("eval_metrics", lambda: P.eval_metrics(emb, B, n_items, cand, day, pidx, plen, rp, rf, U))):
            for _ in range(3):
                fn()
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
            for a_, b_ in evs:
                a_.record(); fn(); b_.record()
            torch.cuda.synchronize()
            kern[name] = sorted(a_.elapsed_time(b_) for a_, b_ in evs)
        r0 = P.rank_metrics(emb, B, n_items)[0]
        restore()                                       # (run_c moved the memory on: the host loop has to see the same batch)
        host, host_top = run_b(4)
    same_rank = int((r0 == ev_out[0]).sum())
    # the host loop ranks torch's scores (another f32 summation order): compared where both picked the same five stocks
    same_top = np.all(ev_out[4].cpu().numpy() == host_top, axis=1)
    agree = float(np.abs(ev_out[5].cpu().numpy() - host)[same_top].max())
    emb_bytes = B * (2 + n_items) * emb.shape[1] * 4
    med = lambda v: float(np.median(v))
    print(json.dumps({"what": "evaluation batch with investment metrics (evaluation.py:63-207), C2, %d interactions x %d items" % (B, n_items),
                      "reps": REPS, "ms_a_embed_plus_rank_metrics": {"median": round(med(ms["a"]), 2), "min": round(min(ms["a"]), 2), "max": round(max(ms["a"]), 2)},
                      "ms_b_a_plus_host_finance_loop": {"median": round(med(ms["b"]), 2), "min": round(min(ms["b"]), 2), "max": round(max(ms["b"]), 2)},
                      "ms_c_embed_plus_eval_metrics": {"median": round(med(ms["c"]), 2), "min": round(min(ms["c"]), 2), "max": round(max(ms["c"]), 2)},
                      "kernel_us_rank_metrics": {"median": round(1e3 * med(kern["rank_metrics"]), 1), "min": round(1e3 * kern["rank_metrics"][0], 1), "max": round(1e3 * kern["rank_metrics"][-1], 1)},
                      "kernel_us_eval_metrics": {"median": round(1e3 * med(kern["eval_metrics"]), 1), "min": round(1e3 * kern["eval_metrics"][0], 1), "max": round(1e3 * kern["eval_metrics"][-1], 1)},
                      "emb_bytes": emb_bytes, "eval_metrics_GBps_of_emb": round(emb_bytes / (1e-3 * med(kern["eval_metrics"])) / 1e9, 1),
                      "rank_metrics_GBps_of_emb": round(emb_bytes / (1e-3 * med(kern["rank_metrics"])) / 1e9, 1),
                      "rows_with_equal_rank_in_both_kernels": same_rank, "rows_with_equal_top5_in_kernel_and_host_loop": int(same_top.sum()), "max_abs_diff_invest_on_those_rows": agree}))
