#!/usr/bin/env python3
"""Portfolio-aware top-k at the serving shape: ``pfo_recommend_mv_topk`` at U = 512, I = 500 candidates, D = 172, k = 10,
portfolios of W = 8 slots (0..7 held stocks), n_ret = 29 returns per stock and day, one block - and ``pfo_recommend_topk`` on the
same embeddings and exclusion lists in the same process, the two alternating.  Device events around every call; median and the
spread (min, max) of REPS calls after WARM warm-up calls, and the ratio of the medians.

Work the mean-variance side adds per user: I (1 + held) n_ret fp64 multiply-adds for y (2 passes over each row) and
about 3 I^2 comparisons over LDS for the two ranks and the order."""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pfotgnrec_amd as P

WARM, REPS = 5, 30
U, I, D, K_TOP, W, N_RET, N_DAYS = 512, 500, 172, 10, 8, 29, 16
dev = torch.device("cuda:0")
P._lib.require_gpu(dev)


def stats(v, scale=1e3, nd=1):
    v = sorted(v)
    return {"median": round(scale * float(np.median(v)), nd), "min": round(scale * v[0], nd), "max": round(scale * v[-1], nd)}


def main():
    rs = np.random.RandomState(U)
    to = lambda a: torch.from_numpy(a).to(dev)
    ue, ie = to(rs.randn(U, D).astype(np.float32)), to(rs.randn(I, D).astype(np.float32))
    plen = rs.randint(0, 8, size=U).astype(np.int32)
    held = rs.randint(0, I, size=(U, W)).astype(np.int32)
    held[np.arange(W)[None, :] >= plen[:, None]] = -1
    port_idx, port_len = to(held), to(plen)                       # a held stock is also excluded: stock row = candidate position
    returns = to(rs.randn(N_DAYS, I, N_RET) * 0.02)
    cand_stock = torch.arange(I, dtype=torch.int32, device=dev)
    day = to(rs.randint(0, N_DAYS, size=U).astype(np.int32))

    def mv():
        return P.recommend_mv_topk(ue, ie, K_TOP, cand_stock, returns, day, port_idx, port_len, 2.0, 0.5, None, port_idx, port_len)

    def plain():
        return P.recommend_topk(ue, ie, K_TOP, None, port_idx, port_len)

    for _ in range(WARM):
        mv(); plain()
    ev = {"mv": [], "plain": []}
    for rep in range(REPS):
        order = (("mv", mv), ("plain", plain))
        for name, fn in (order if rep % 2 == 0 else order[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            ev[name].append((a, b))
    torch.cuda.synchronize()
    ms = {name: [a.elapsed_time(b) for a, b in v] for name, v in ev.items()}
    lam0 = P.recommend_mv_topk(ue, ie, K_TOP, cand_stock, returns, day, port_idx, port_len, 2.0, 0.0, None, port_idx, port_len)
    ref = plain()
    print(json.dumps({"what": "pfo_recommend_mv_topk vs pfo_recommend_topk, same embeddings", "U": U, "I": I, "D": D, "k": K_TOP,
                      "W": W, "n_ret": N_RET, "warmup": WARM, "reps": REPS, "mv_us": stats(ms["mv"]), "plain_us": stats(ms["plain"]),
                      "ratio_of_medians": round(float(np.median(ms["mv"]) / np.median(ms["plain"])), 2),
                      "lambda_0_equals_plain": bool(torch.equal(lam0[0], ref[0]) and torch.equal(lam0[1], ref[1]))}), flush=True)


if __name__ == "__main__":
    main()
