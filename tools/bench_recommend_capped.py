#!/usr/bin/env python3
"""Group caps at the serving shapes of the other recommend benches: each capped entry against its uncapped sibling, in the same
process on the same tensors, with a cap that binds (10 groups of ~45 candidates and 50 groupless ones, cap 1: a list of k = 10
holds at most ten grouped picks, the walk skips most of the order's head) and one that never does (cap = k, the same groups).

* ``pfo_recommend_topk_capped`` vs ``pfo_recommend_topk``: U = 50 000 and 512, I = 500, D = 172, k = 10 (bench_recommend.py);
* ``pfo_recommend_mv_topk_capped`` vs ``pfo_recommend_mv_topk``: U = 512, W = 8, n_ret = 29 (bench_recommend_mv.py);
* ``pfo_recommend_basket_topk_capped`` vs ``pfo_recommend_basket_topk`` at the same shape, and against the route a caller has
  without it: k launches of ``pfo_recommend_mv_topk`` at k = 1, the pick appended to the portfolio row and the exclusion row on
  the device in between, and the rest of a group that is full appended to the exclusion row too - outputs asserted equal.

Device events around every call, the variants of a family alternating; median [min, max] of REPS calls after WARM warm-up calls
and the ratios of the medians.  Work the cap adds per user: a few wave-wide operations per round (plain), I^2
comparisons (mean-variance), at most k LDS reads per pick (basket)."""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pfotgnrec_amd as P

WARM, REPS = 5, 30
I, D, K_TOP, W, N_RET, N_DAYS, N_GROUPS = 500, 172, 10, 8, 29, 16, 10
dev = torch.device("cuda:0")
P._lib.require_gpu(dev)


def stats(v, scale=1e3, nd=1):
    v = sorted(v)
    return {"median": round(scale * float(np.median(v)), nd), "min": round(scale * v[0], nd), "max": round(scale * v[-1], nd)}


def alternate(fns, reps=REPS):
    """{name: [ms]} of ``fns`` ((name, callable), ...) alternating, device events around every call."""
    for _ in range(WARM):
        for _, fn in fns:
            fn()
    ev = {name: [] for name, _ in fns}
    for rep in range(reps):
        for name, fn in (fns if rep % 2 == 0 else fns[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            ev[name].append((a, b))
    torch.cuda.synchronize()
    return {name: [a.elapsed_time(b) for a, b in v] for name, v in ev.items()}


def ratios(ms, base):
    return {"%s_over_%s" % (n, base): round(float(np.median(v) / np.median(ms[base])), 3) for n, v in ms.items() if n != base}


def case(U):
    rs = np.random.RandomState(U)
    to = lambda a: torch.from_numpy(a).to(dev)
    c = dict(ue=to(rs.randn(U, D).astype(np.float32)), ie=to(rs.randn(I, D).astype(np.float32)))
    plen = rs.randint(0, 8, size=U).astype(np.int32)
    held = rs.randint(0, I, size=(U, W)).astype(np.int32)
    held[np.arange(W)[None, :] >= plen[:, None]] = -1
    c["port_idx"], c["port_len"] = to(held), to(plen)                 # a held stock is also excluded: stock row = candidate position
    c["returns"] = to(rs.randn(N_DAYS, I, N_RET) * 0.02)
    c["cand_stock"] = torch.arange(I, dtype=torch.int32, device=dev)
    c["day"] = to(rs.randint(0, N_DAYS, size=U).astype(np.int32))
    c["groups_h"] = rs.randint(-1, N_GROUPS, size=I).astype(np.int32)
    c["groups"] = to(c["groups_h"])
    return c


def plain(U):
    c = case(U)
    call = lambda **cap: P.recommend_topk(c["ue"], c["ie"], K_TOP, None, c["port_idx"], c["port_len"], **cap)
    fns = (("uncapped", call), ("cap_binds", lambda: call(cand_group=c["groups"], group_cap=1)),
           ("cap_never_binds", lambda: call(cand_group=c["groups"], group_cap=K_TOP)))
    ms = alternate(fns)
    a, b, n = call(), call(cand_group=c["groups"], group_cap=1), call(cand_group=c["groups"], group_cap=K_TOP)
    assert all(torch.equal(x, y) for x, y in zip(a, n)), "a cap of k must give the uncapped list"
    return {"what": "pfo_recommend_topk_capped vs pfo_recommend_topk, same tensors", "U": U, "I": I, "D": D, "k": K_TOP, "groups": N_GROUPS,
            "warmup": WARM, "reps": REPS, **{n_ + "_us": stats(v) for n_, v in ms.items()}, **ratios(ms, "uncapped"),
            "users_whose_list_the_cap_changes": int((a[0] != b[0]).any(1).sum())}


def mv_forms(U=512):
    c = case(U)
    args = lambda k, port, plen, ex, exlen: (c["ue"], c["ie"], k, c["cand_stock"], c["returns"], c["day"], port, plen, 2.0, 0.5, None, ex, exlen)
    out = []
    for name, fn in (("mv", P.recommend_mv_topk), ("basket", P.recommend_basket_topk)):
        call = lambda fn=fn, **cap: fn(*args(K_TOP, c["port_idx"], c["port_len"], c["port_idx"], c["port_len"]), **cap)
        fns = (("uncapped", call), ("cap_binds", lambda call=call: call(cand_group=c["groups"], group_cap=1)),
               ("cap_never_binds", lambda call=call: call(cand_group=c["groups"], group_cap=K_TOP)))
        ms = alternate(fns)
        a, b, n = call(), call(cand_group=c["groups"], group_cap=1), call(cand_group=c["groups"], group_cap=K_TOP)
        assert all(torch.equal(x, y) for x, y in zip(a, n)), "a cap of k must give the uncapped list"
        out.append({"what": "pfo_recommend_%s_topk_capped vs pfo_recommend_%s_topk, same tensors" % (name, name), "U": U, "I": I, "D": D,
                    "k": K_TOP, "W": W, "n_ret": N_RET, "groups": N_GROUPS, "warmup": WARM, "reps": REPS,
                    **{n_ + "_us": stats(v) for n_, v in ms.items()}, **ratios(ms, "uncapped"),
                    "users_whose_list_the_cap_changes": int((a[0] != b[0]).any(1).sum())})

    # ---- the capped basket against the k = 1 loop it replaces
    cap = 1
    members = [np.flatnonzero(c["groups_h"] == g) for g in range(N_GROUPS)]
    M = max(len(m) for m in members)
    table = np.full((N_GROUPS + 1, M), -1, np.int32)                  # row N_GROUPS: no group, nothing to append
    for g, m in enumerate(members):
        table[g, :len(m)] = m
    table = torch.from_numpy(table).to(dev)
    ar = torch.arange(U, device=dev)

    def basket():
        return P.recommend_basket_topk(*args(K_TOP, c["port_idx"], c["port_len"], c["port_idx"], c["port_len"]), cand_group=c["groups"],
                                       group_cap=cap)

    def loop():
        port = torch.full((U, W + K_TOP), -1, dtype=torch.int32, device=dev)
        port[:, :W] = c["port_idx"]
        ex = torch.full((U, W + K_TOP * (1 + M)), -1, dtype=torch.int32, device=dev)
        ex[:, :W] = c["port_idx"]
        n_port, n_ex = c["port_len"].clone(), c["port_len"].clone()
        held = torch.zeros((U, N_GROUPS + 1), dtype=torch.int32, device=dev)
        pos = torch.full((U, K_TOP), -1, dtype=torch.int32, device=dev)
        score = torch.full((U, K_TOP), float("-inf"), dtype=torch.float32, device=dev)
        fused = torch.full((U, K_TOP), float("-inf"), dtype=torch.float64, device=dev)
        n_valid = torch.zeros(U, dtype=torch.int32, device=dev)
        for r in range(K_TOP):
            one = P.recommend_mv_topk(*args(1, port, n_port, ex, n_ex))
            got = (one[3] == 1) & (n_valid == r)
            p = one[0][:, 0].long().clamp(min=0)
            pos[:, r] = torch.where(got, one[0][:, 0], pos[:, r])
            score[:, r] = torch.where(got, one[1][:, 0], score[:, r])
            fused[:, r] = torch.where(got, one[2][:, 0], fused[:, r])
            n_valid += got.int()
            at = n_port.long()
            port[ar, at] = torch.where(got, c["cand_stock"][p], port[ar, at])
            n_port += got.int()
            g = c["groups"][p].long()
            g = torch.where(got & (g >= 0), g, torch.full_like(g, N_GROUPS))
            held[ar, g] += 1
            full = (held[ar, g] >= cap) & (g < N_GROUPS)
            at = n_ex.long()
            ex[ar, at] = torch.where(got, one[0][:, 0], ex[ar, at])
            rows = table[torch.where(full, g, torch.full_like(g, N_GROUPS))]          # the whole group (the pick again: harmless)
            ex.scatter_(1, (at + 1)[:, None] + torch.arange(M, device=dev)[None, :], rows)
            n_ex += got.int() + full.int() * M
        return pos, score, fused, n_valid

    ms = alternate((("capped_basket", basket), ("loop_of_k_calls", loop)), reps=10)
    assert all(torch.equal(x, y) for x, y in zip(basket(), loop())), "the capped basket and the loop of k calls disagree"
    out.append({"what": "pfo_recommend_basket_topk_capped vs k launches of pfo_recommend_mv_topk(k = 1) with the exclusion row extended "
                        "on the device", "U": U, "I": I, "D": D, "k": K_TOP, "groups": N_GROUPS, "group_cap": cap, "warmup": WARM, "reps": 10,
                **{n_ + "_us": stats(v) for n_, v in ms.items()}, **ratios(ms, "capped_basket"), "capped_basket_equals_loop": True})
    return out


if __name__ == "__main__":
    for U in (50000, 512):
        print(json.dumps(plain(U)), flush=True)
    for line in mv_forms():
        print(json.dumps(line), flush=True)
