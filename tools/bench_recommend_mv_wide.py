#!/usr/bin/env python3
"""The wide form of the portfolio-aware top-k at the serving shape of ``bench_recommend_mv.py`` - U = 512, D = 172, k = 10,
portfolios of W = 8 slots (0..7 held stocks, excluded as well), n_ret = 29, one block - over candidate lists of growing length.

  I = 500, 2048          ``pfo_recommend_mv_topk_wide`` and ``pfo_recommend_mv_topk`` on the same inputs, alternating; every
                         output of the two must be equal (``torch.equal``), or the tool fails.
  I = 4096, 16384, 65536 the wide form with ``pfo_recommend_topk`` beside it on the same embeddings and exclusion lists, for scale.

Device events around every call; median and the spread (min, max) of REPS calls after WARM warm-up calls.  The workspace is
allocated once per list length, by the rule of ``recommend_mv_topk_wide`` (all users at once, 256 MiB at the most).  One JSON line:
per length the times, wide / bounded or wide / plain, and at the end the growth t(65536) / t(2048) of the wide form (a stage that
counts pairs would show about 1024, a radix sort about 32) and the workspace bytes per user at I = 65536."""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pfotgnrec_amd as P

U, D, K_TOP, W, N_RET, N_DAYS = 512, 172, 10, 8, 29, 16
BOTH, WIDE_ONLY = (500, 2048), (4096, 16384, 65536)
dev = torch.device("cuda:0")
P._lib.require_gpu(dev)


def stats(v, scale=1e3, nd=1):
    v = sorted(v)
    return {"median": round(scale * float(np.median(v)), nd), "min": round(scale * v[0], nd), "max": round(scale * v[-1], nd)}


def timed(fns, warm, reps):
    """ms per call of each of ``fns`` (name -> callable), the calls alternating and the order swapped every repetition."""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    ev = {name: [] for name in fns}
    order = list(fns.items())
    for rep in range(reps):
        for name, fn in (order if rep % 2 == 0 else order[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            ev[name].append((a, b))
    torch.cuda.synchronize()
    return {name: [a.elapsed_time(b) for a, b in v] for name, v in ev.items()}


def case(I):
    rs = np.random.RandomState(I)
    to = lambda a: torch.from_numpy(a).to(dev)
    ue, ie = to(rs.randn(U, D).astype(np.float32)), to(rs.randn(I, D).astype(np.float32))
    plen = rs.randint(0, 8, size=U).astype(np.int32)
    held = rs.randint(0, I, size=(U, W)).astype(np.int32)
    held[np.arange(W)[None, :] >= plen[:, None]] = -1
    port_idx, port_len = to(held), to(plen)                       # a held stock is also excluded: stock row = candidate position
    returns = to(rs.randn(N_DAYS, I, N_RET) * 0.02)
    cand_stock = torch.arange(I, dtype=torch.int32, device=dev)
    day = to(rs.randint(0, N_DAYS, size=U).astype(np.int32))
    size = lambda users: P._lib.byte_count("pfo_recommend_mv_wide_workspace_bytes", users, I)
    ws = torch.empty(max(min(size(U), 256 << 20), size(16)), dtype=torch.uint8, device=dev)
    mv_args = (ue, ie, K_TOP, cand_stock, returns, day, port_idx, port_len, 2.0, 0.5, None, port_idx, port_len)
    wide = lambda **kw: P.recommend_mv_topk_wide(*mv_args, workspace=ws, **kw)
    bounded = lambda **kw: P.recommend_mv_topk(*mv_args, **kw)
    plain = lambda: P.recommend_topk(ue, ie, K_TOP, None, port_idx, port_len)
    return wide, bounded, plain, {"workspace_bytes": int(ws.numel()), "slabs": -(-size(U) // int(ws.numel()))}


def main():
    rows, t_wide = [], {}
    for I in BOTH + WIDE_ONLY:
        wide, bounded, plain, row = case(I)
        warm, reps = (5, 30) if I <= 4096 else (2, 10)
        row.update({"I": I, "warmup": warm, "reps": reps})
        if I in BOTH:
            ms = timed({"wide": wide, "bounded": bounded, "plain": plain}, warm, reps)
            same = all(torch.equal(a, b) or (a.dtype.is_floating_point and torch.equal(a.isnan(), b.isnan())
                                             and torch.equal(a.nan_to_num(0.0), b.nan_to_num(0.0)))
                       for a, b in zip(wide(want_all=True), bounded(want_all=True)))
            assert same, "I = %d: the wide form and the bounded kernel differ" % I
            row.update({"bounded_us": stats(ms["bounded"]), "equals_bounded": same,
                        "wide_over_bounded": round(float(np.median(ms["wide"]) / np.median(ms["bounded"])), 2)})
        else:
            ms = timed({"wide": wide, "plain": plain}, warm, reps)
        t_wide[I] = float(np.median(ms["wide"]))
        row.update({"wide_us": stats(ms["wide"]), "plain_us": stats(ms["plain"]),
                    "wide_over_plain": round(t_wide[I] / float(np.median(ms["plain"])), 2)})
        rows.append(row)
        torch.cuda.empty_cache()
    print(json.dumps({"what": "pfo_recommend_mv_topk_wide vs pfo_recommend_mv_topk / pfo_recommend_topk, same inputs", "U": U, "D": D,
                      "k": K_TOP, "W": W, "n_ret": N_RET, "by_I": rows, "growth_65536_over_2048": round(t_wide[65536] / t_wide[2048], 1),
                      "workspace_bytes_per_user_at_65536": P._lib.byte_count("pfo_recommend_mv_wide_workspace_bytes", 16, 65536) // 16}),
          flush=True)


if __name__ == "__main__":
    main()
