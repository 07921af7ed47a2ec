#!/usr/bin/env python3
"""Advancing the model state over a log: ``TGN.observe`` against the only way there was before it.

On the C2 synthetic graph (L2 K20 D172 H2, memory + GRU) the same 100 batches of 512 interactions are taken in twice, from
the same saved state (memory, last_update, pending messages restored in front of every repetition):
  observe : ONE ``TGN.observe(..., batch_size=512)`` call over the 51 200 interactions (device tensors);
  forward : 100 eval-mode ``embed_device`` calls under ``no_grad`` with one negative per interaction (device tensors, the
            negatives drawn ahead of the timed window) - sampling, lazy GRU over the touched frontier, two attention layers
            for 3 x 512 roots, the embeddings thrown away.
Host clock (``time.perf_counter``) around a run that starts and ends in a device synchronise; WARM warm-up runs of each,
then REPS timed runs, the two alternating and the order swapped every repetition; median, min and max are printed.
Kernel launches per run are counted once, outside the timed runs, with torch's profiler (null when it is not available).
The last line is one JSON object."""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pfotgnrec_amd as P
from pfotgnrec_amd.synthetic import CONFIGS, make_graph

WARM, REPS = 2, 9
N_BATCHES, B, START = 100, 512, 600_000
dev = torch.device("cuda:0")
P._lib.require_gpu(dev)


def stats(v):
    v = sorted(v)
    return {"median": round(1e3 * float(np.median(v)), 3), "min": round(1e3 * v[0], 3), "max": round(1e3 * v[-1], 3)}


def count_kernels(fn):
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower())
    except Exception:
        return None


def main():
    cfg = CONFIGS["C2"]
    g = make_graph(cfg, with_prices=False, with_portfolios=False)
    d = g.data
    tgn = P.TGN(P.get_neighbor_finder(d, False), g.node_features, g.edge_features, dev, n_layers=2, n_heads=2, dropout=0.1,
                use_memory=True, memory_dimension=cfg.dim, message_function="identity", n_neighbors=cfg.n_neighbors)
    tgn.eval()
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    n = N_BATCHES * B
    src, dst = to(d.sources[START:START + n], np.int32), to(d.destinations[START:START + n], np.int32)
    ts, eidx = to(d.timestamps[START:START + n], np.float64), to(d.edge_idxs[START:START + n], np.int32)
    neg = to(np.random.RandomState(0).randint(cfg.n_users + 1, cfg.n_users + cfg.n_items + 1, size=n), np.int32)
    K = cfg.n_neighbors

    def forward_path():
        with torch.no_grad():
            for k in range(0, n, B):
                tgn.embed_device(src[k:k + B], dst[k:k + B], [neg[k:k + B]], [1], ts[k:k + B], eidx[k:k + B], K)

    def observe_path():
        tgn.observe(src, dst, ts, eidx, batch_size=B)

    # a populated state to start from: the 20 batches in front of the window, then saved
    with torch.no_grad():
        for k in range(START - 20 * B, START, B):
            s = slice(k, k + B)
            tgn.embed_device(to(d.sources[s], np.int32), to(d.destinations[s], np.int32), [neg[:B]], [1], to(d.timestamps[s], np.float64),
                             to(d.edge_idxs[s], np.int32), K)
    saved = tgn.memory.backup_memory()
    paths = (("observe", observe_path), ("forward", forward_path))
    end_state = {}
    for name, fn in paths:
        for _ in range(WARM):
            tgn.memory.restore_memory(saved)
            fn()
        torch.cuda.synchronize()
        end_state[name] = tgn.memory.memory.detach().clone()
    t = {"observe": [], "forward": []}
    for rep in range(REPS):
        for name, fn in (paths if rep % 2 == 0 else paths[::-1]):
            tgn.memory.restore_memory(saved)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); t[name].append(time.perf_counter() - t0)
    launches = {}
    for name, fn in paths:
        tgn.memory.restore_memory(saved)
        launches[name] = count_kernels(fn)
    diff = float((end_state["observe"] - end_state["forward"]).abs().max() / end_state["forward"].abs().max())
    mo, mf = float(np.median(t["observe"])), float(np.median(t["forward"]))
    print(json.dumps({"what": "100 batches of 512 on the C2 graph (L2 K20 D172 H2): TGN.observe vs eval-mode embed_device, 1 negative",
                      "clock": "host perf_counter around synchronised runs", "warmup": WARM, "reps": REPS,
                      "observe_ms": stats(t["observe"]), "forward_ms": stats(t["forward"]),
                      "observe_us_per_batch": round(1e6 * mo / N_BATCHES, 2), "forward_us_per_batch": round(1e6 * mf / N_BATCHES, 2),
                      "forward_over_observe": round(mf / mo, 2),
                      "kernel_launches_per_run": launches, "observe_launches_per_batch_by_design": 4,
                      "end_memory_max_relative_difference": diff}), flush=True)


if __name__ == "__main__":
    main()
