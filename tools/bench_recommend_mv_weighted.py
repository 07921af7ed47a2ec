#!/usr/bin/env python3
"""Position-weighted mean-variance top-k against its unweighted sibling at the same shapes in one run: U = 512, I in {500, 2048}
candidates, portfolios of W in {8, 64} slots (every slot held), n_ret = 30, D = 172, k = 10, one block - the bounded entry
(``pfo_recommend_mv_topk[_weighted]``), and at I = 2048 also the wide and the list entry (lists of 64).  The two alternate, the
order swapping every repetition; device events around every call; median and the spread (min, max) of REPS calls after WARM
warm-up calls, and the ratio of the medians.  One JSON line per shape.

Work the weights add per holding and candidate: one fp64 multiply and the "counts" compare, next to the n_ret
multiply-adds of the covariance."""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pfotgnrec_amd as P

WARM, REPS = 5, 30
U, D, K_TOP, N_RET, N_DAYS, LIST_W = 512, 172, 10, 30, 16, 64
dev = torch.device("cuda:0")
P._lib.require_gpu(dev)


def stats(v, scale=1e3, nd=1):
    v = sorted(v)
    return {"median": round(scale * float(np.median(v)), nd), "min": round(scale * v[0], nd), "max": round(scale * v[-1], nd)}


def run(form, I, W):
    rs = np.random.RandomState(I + W)
    to = lambda a: torch.from_numpy(a).to(dev)
    ue, ie = to(rs.randn(U, D).astype(np.float32)), to(rs.randn(I, D).astype(np.float32))
    port_idx = to(rs.randint(0, I, size=(U, W)).astype(np.int32))
    port_len = torch.full((U,), W, dtype=torch.int32, device=dev)
    port_w = to(rs.uniform(0.5, 500.0, size=(U, W)))
    returns = to(rs.randn(N_DAYS, I, N_RET) * 0.02)
    cand_stock = torch.arange(I, dtype=torch.int32, device=dev)
    day = to(rs.randint(0, N_DAYS, size=U).astype(np.int32))
    mv = (cand_stock, returns, day, port_idx, port_len, 2.0, 0.5)
    if form == "list":
        lists = to(rs.randint(0, I, size=(U, LIST_W)).astype(np.int32))
        call = lambda w: P.recommend_list_mv_topk(ue, ie, K_TOP, lists, None, *mv, port_w=w)
    else:
        fn = P.recommend_mv_topk if form == "bounded" else P.recommend_mv_topk_wide
        kw = dict(workspace=torch.empty(P._lib.byte_count("pfo_recommend_mv_wide_workspace_bytes", U, I), dtype=torch.uint8, device=dev)) \
            if form == "wide" else {}
        call = lambda w: fn(ue, ie, K_TOP, *mv, port_w=w, **kw)
    fns = (("weighted", lambda: call(port_w)), ("unweighted", lambda: call(None)))
    for _ in range(WARM):
        for _, fn_ in fns:
            fn_()
    ev = {name: [] for name, _ in fns}
    for rep in range(REPS):
        for name, fn_ in (fns if rep % 2 == 0 else fns[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn_(); b.record()
            ev[name].append((a, b))
    torch.cuda.synchronize()
    ms = {name: [a.elapsed_time(b) for a, b in v] for name, v in ev.items()}
    ones = call(torch.ones_like(port_w))
    plain = call(None)
    print(json.dumps({"what": "weighted vs unweighted mean-variance top-k, same inputs", "form": form, "U": U, "I": I, "D": D, "k": K_TOP,
                      "W": W, "n_ret": N_RET, "warmup": WARM, "reps": REPS, "weighted_us": stats(ms["weighted"]),
                      "unweighted_us": stats(ms["unweighted"]),
                      "ratio_of_medians": round(float(np.median(ms["weighted"]) / np.median(ms["unweighted"])), 3),
                      "all_ones_equal_unweighted": bool(all(torch.equal(a, b) for a, b in zip(ones, plain)))}), flush=True)


def main():
    for I in (500, 2048):
        for W in (8, 64):
            run("bounded", I, W)
    for form in ("wide", "list"):
        for W in (8, 64):
            run(form, 2048, W)


if __name__ == "__main__":
    main()
