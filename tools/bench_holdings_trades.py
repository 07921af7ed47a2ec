#!/usr/bin/env python3
"""Holdings from trades on raw ledger tables of 50 000 node rows, widths 8 and 64: a serving tick (N = 512 events)
and a replay (N = 200 000), users drawn uniformly, 70 % buys over 2 W stocks - and the adversarial replay in which ONE user owns
every event.  Variants, alternating in one process:

  apply  ``pfo_holdings_apply`` (tables put back to the seeded state before every call, outside the timed span)
  store  ``pfo_holdings_store`` of the same N and W - the only other writer there is; NOT equal work (last event per user wins)
  host   the route a caller has without it: ``Holdings.rows`` of the tick's users read back, the loop on the host, the rows
         uploaded and stored (``pfo_holdings_store``)

apply / store: device events around the one native call, 30 calls after 5.  host: host clock around the synchronised route (it
IS host work), 30 calls after 5 at N = 512, 2 after 1 at N = 200 000 (a Python loop).  Median [min, max] in microseconds; the
last line is one JSON object.  No pass / fail threshold."""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pfotgnrec_amd as P
from pfotgnrec_amd import _lib
from pfotgnrec_amd.holdings import Holdings

N_NODES, WARM, REPS = 50_000, 5, 30
dev = torch.device("cuda:0")
_lib.require_gpu(dev)


def stats(v):
    v = sorted(v)
    return {"median": round(float(np.median(v)), 1), "min": round(v[0], 1), "max": round(v[-1], 1)}


def dev_timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b)


def host_loop(idx, ln, pos, stock, side, W):
    """The sequential rule on the rows read back (no quantities): ``pos[e]`` is the event's row among them."""
    for e in range(len(pos)):
        r, s, L = int(pos[e]), int(stock[e]), int(ln[pos[e]])
        hit = np.flatnonzero(idx[r, :L] == s)
        if side[e] == 1:
            if not hit.size and L < W:
                idx[r, L] = s
                ln[r] = L + 1
        elif hit.size:
            j = int(hit[0])
            idx[r, j:L - 1] = idx[r, j + 1:L]
            idx[r, L - 1] = -1
            ln[r] = L - 1


def shape(W, N, one_user):
    rs = np.random.RandomState(W + N + int(one_user))
    src = np.full(N, 777, np.int32) if one_user else rs.randint(1, N_NODES, N).astype(np.int32)
    stock = rs.randint(0, 2 * W, N).astype(np.int32)
    side = rs.choice([1, 1, 1, 1, 1, 1, 1, -1, -1, -1], N).astype(np.int32)
    ts = np.arange(N, dtype=np.float64)
    h = Holdings(N_NODES, N_NODES, W, 0, dev)
    d = [torch.from_numpy(a).to(dev) for a in (src, stock, side, ts)]
    # the seeded state: every row half full
    seed_idx = torch.from_numpy(np.where(np.arange(W) < W // 2, rs.randint(0, 2 * W, (N_NODES, W)), -1).astype(np.int32)).to(dev)
    seed = (seed_idx, torch.full((N_NODES,), W // 2, dtype=torch.int32, device=dev), torch.zeros(N_NODES, dtype=torch.float64, device=dev))

    def reset():
        for t, s in zip((h.idx, h.len, h.time), seed):
            t.copy_(s)
    port_idx = torch.from_numpy(rs.randint(0, 2 * W, (N, W)).astype(np.int32)).to(dev)
    port_len = torch.from_numpy(rs.randint(0, W + 1, N).astype(np.int32)).to(dev)
    scratch = torch.empty(_lib.byte_count("pfo_holdings_apply_scratch_bytes", N_NODES, N), dtype=torch.uint8, device=dev)

    def apply():
        P.holdings_apply(d[0], d[1], d[2], d[3], h.idx, h.len, h.time, None, None, h.counters, scratch)

    def store():
        h.store(d[0], port_idx, port_len, d[3])

    def host():
        users, pos = np.unique(src, return_inverse=True)
        idx, ln = (t.cpu().numpy() for t in h.rows(users))
        host_loop(idx, ln, pos, stock, side, W)
        last = np.zeros(users.shape[0], np.float64)
        last[pos] = ts                                           # (chronological: the last assignment per user stays)
        h.store(*(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (users.astype(np.int32), idx, ln, last)))
        torch.cuda.synchronize()

    out = {"W": W, "N": N, "one_user": one_user}
    times = {"apply": [], "store": []}
    for rep in range(WARM + REPS):
        for name, fn in ((("apply", apply), ("store", store)) if rep % 2 == 0 else (("store", store), ("apply", apply))):
            reset()
            t = dev_timed(fn)
            if rep >= WARM:
                times[name].append(t)
    out["apply_us"], out["store_us"] = stats(times["apply"]), stats(times["store"])
    warm, reps = (WARM, REPS) if N <= 512 else (1, 2)
    th = []
    for rep in range(warm + reps):
        reset()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        host()
        if rep >= warm:
            th.append(1e6 * (time.perf_counter() - t0))
    out["host_us"], out["host_reps"] = stats(th), reps
    print("W=%-3d N=%-7d %s apply %s  store %s  host %s" % (W, N, "one user " if one_user else "all users",
                                                          out["apply_us"], out["store_us"], out["host_us"]), flush=True)
    return out


def main():
    rows = [shape(W, N, False) for W in (8, 64) for N in (512, 200_000)]
    rows += [shape(W, 200_000, True) for W in (8, 64)]
    print(json.dumps({"what": "pfo_holdings_apply vs pfo_holdings_store vs the host route, n_nodes = 50 000; microseconds",
                      "clock": "device events around one native call (apply, store); host perf_counter around the synchronised route (host)",
                      "warmup": WARM, "reps": REPS, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
