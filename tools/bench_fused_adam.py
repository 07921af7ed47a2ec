#!/usr/bin/env python3
"""What FusedAdam's weight decay and global-norm clipping cost the training step.

On the C2 synthetic graph (L2 K20 D172 H2 Ef4, memory + GRU, batch 512, 3 negatives; 1.55 M parameters) ONE model runs the
``bpr_step(..., optimizer=)`` loop of bench.py - the end of the backward, the pre-step's two launches (csrc/optim.hip) and the
Adam kernel on the library's side stream, gradients cleared by the Adam kernel - under four settings of the optimizer's
``param_groups[0]``: options off, clip only, decay only, both.  The settings alternate in one process, the order swapped every
round; the clip bound is half the gradient norm measured in the warm-up, so that it binds.  Host clock (``time.perf_counter``)
around windows of STEPS steps that start and end in a device synchronise; WARM untimed windows of each, then REPS timed rounds;
median (min - max) ms per step.  One JSON line.
Then ``kernels()`` (alone with ``--kernels-only``): the two launches by themselves on a buffer of the model's size, one range,
device events around LOOP back-to-back calls; us per call.  A second JSON line."""
import ctypes as C
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pfotgnrec_amd as P
from pfotgnrec_amd import _lib
from pfotgnrec_amd.synthetic import CONFIGS, make_graph

WARM, REPS = 1, 7
STEPS, B, START, NEG = 40, 512, 600_000, 3
LOOP = 100
dev = torch.device("cuda:0")
_lib.require_gpu(dev)


def stats(v, scale):
    v = sorted(x * scale for x in v)
    return {"median": round(float(np.median(v)), 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def main():
    cfg = CONFIGS["C2"]
    g = make_graph(cfg, with_prices=False, with_portfolios=False)
    d = g.data
    K = cfg.n_neighbors
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    span = 400 * B
    src, dst = to(d.sources[START:START + span], np.int32), to(d.destinations[START:START + span], np.int32)
    ts, eidx = to(d.timestamps[START:START + span], np.float64), to(d.edge_idxs[START:START + span], np.int32)
    neg = to(np.random.RandomState(0).randint(cfg.n_users + 1, cfg.n_users + cfg.n_items + 1, size=span * NEG), np.int32)
    torch.manual_seed(1)
    tgn = P.TGN(P.NeighborFinder.from_arrays(d.sources, d.destinations, d.edge_idxs, d.timestamps, device=dev), g.node_features,
                g.edge_features, dev, n_layers=cfg.n_layers, n_heads=cfg.n_heads, dropout=0.1, use_memory=True, memory_dimension=cfg.dim,
                message_function="identity", n_neighbors=K)
    tgn.train()
    opt = P.FusedAdam(tgn, lr=1e-4, zero_grads_in_step=True)
    at = [0]

    def window():
        for _ in range(STEPS):
            k = (at[0] % 400) * B
            at[0] += 1
            emb, b = tgn.embed_device(src[k:k + B], dst[k:k + B], [neg[k * NEG:(k + B) * NEG]], [NEG], ts[k:k + B], eidx[k:k + B], K)
            P.bpr_step(tgn, emb, b, NEG, optimizer=opt)
            opt.zero_grad(set_to_none=True)
        tgn.join()

    group = opt.param_groups[0]
    group["max_grad_norm"] = 1e30                                   # (measures, never binds)
    window()
    torch.cuda.synchronize()
    norm = float(opt.last_grad_norm.item())
    settings = {"off": (0.0, None), "clip": (0.0, 0.5 * norm), "decay": (0.01, None), "both": (0.01, 0.5 * norm)}

    def use(name):
        group["weight_decay"], group["max_grad_norm"] = settings[name]
    for name in settings:
        use(name)
        for _ in range(WARM):
            window()
    t = {name: [] for name in settings}
    norms = {}
    order = list(settings)
    for rep in range(REPS):
        for name in (order if rep % 2 == 0 else order[::-1]):
            use(name)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            window()
            torch.cuda.synchronize(); t[name].append(time.perf_counter() - t0)
            if settings[name][1] is not None:
                norms[name] = round(float(opt.last_grad_norm.item()), 4)
    ms = {name: stats(v, 1e3 / STEPS) for name, v in t.items()}
    off = float(np.median(t["off"]))
    print(json.dumps({"what": "C2 graph (L2 K20 D172 H2), batch 512, 3 negatives, bpr_step(..., optimizer=FusedAdam(zero_grads_in_step=True)): "
                              "ms per step with weight decay / global-norm clipping off and on",
                      "clock": "host perf_counter around synchronised windows of %d steps" % STEPS, "warmup_windows": WARM, "rounds": REPS,
                      "parameters": int(tgn.flat_parameters.numel()), "clip_bound": round(0.5 * norm, 4), "last_grad_norm": norms,
                      "ms_per_step": ms, "over_off": {name: round(float(np.median(v)) / off, 4) for name, v in t.items()}}), flush=True)
    return int(tgn.flat_parameters.numel())


def kernels(n=1_551_352):
    """The two launches alone on a buffer of the C2 model's size (one range over all of it), us per call."""
    rs = np.random.RandomState(0)
    p = torch.from_numpy(rs.randn(n).astype(np.float32)).to(dev)
    g = torch.from_numpy(rs.randn(n).astype(np.float32)).to(dev)
    partial = torch.zeros(_lib.GRAD_NORM_PARTS, dtype=torch.float64, device=dev)
    norm = torch.zeros(1, dtype=torch.float32, device=dev)
    rng = (1, (C.c_int64 * 1)(0), (C.c_int64 * 1)(n))
    sp = _lib.stream_ptr()
    pre = lambda max_norm, decay: _lib.call("pfo_grad_prestep_ranges", p.data_ptr(), g.data_ptr(), *rng, partial.data_ptr(), max_norm, decay,
                                            norm.data_ptr(), sp)
    forms = {"sumsq": lambda: _lib.call("pfo_grad_sumsq_ranges", g.data_ptr(), *rng, partial.data_ptr(), 0, sp),
             "prestep_clip": lambda: pre(1e30, 1.0),                # (coef = 1: the buffer keeps its values over the calls)
             "prestep_decay": lambda: pre(0.0, 1.0 - 6e-8),         # (the largest float below 1)
             "prestep_both": lambda: pre(1e30, 1.0 - 6e-8)}
    for f in forms.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in forms}
    order = list(forms)
    for rep in range(REPS):
        for k in (order if rep % 2 == 0 else order[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(LOOP):
                forms[k]()
            e1.record(); e1.synchronize()
            t[k].append(e0.elapsed_time(e1) / LOOP)
    print(json.dumps({"what": "pfo_grad_sumsq_ranges / pfo_grad_prestep_ranges alone, one range of %d elements: us per call" % n,
                      "clock": "device events around %d back-to-back calls" % LOOP, "rounds": REPS,
                      "bytes_moved": {"sumsq": 4 * n, "prestep_clip": 8 * n, "prestep_decay": 8 * n, "prestep_both": 16 * n},
                      "us_per_call": {k: stats(v, 1e3) for k, v in t.items()}}), flush=True)


if __name__ == "__main__":
    if "--kernels-only" in sys.argv:
        kernels()
    else:
        kernels(main())
