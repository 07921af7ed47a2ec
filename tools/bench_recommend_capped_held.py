#!/usr/bin/env python3
"""Group caps that count holdings at the shape of bench_recommend_capped.py: each ``_held`` entry against its ``_capped`` sibling,
in the same process on the same tensors (10 groups of ~45 candidates and 50 groupless ones), held rows 8 wide - the group of
each stock of the portfolio row, 0 to 7 of them a user.  Three variants of a family alternate:

* ``capped``      the sibling, no holdings;
* ``held``        the rows as they are, at cap 2: a user who holds two names of a group finds it closed, one name leaves one slot;
* ``held_empty``  the same rows with every length 0: the work the entry adds when nothing is held.

* ``pfo_recommend_topk_capped_held`` vs ``pfo_recommend_topk_capped``: U = 50 000 and 512, I = 500, D = 172, k = 10;
* ``pfo_recommend_mv_topk_capped_held`` vs ``pfo_recommend_mv_topk_capped``: U = 512, W = 8, n_ret = 29;
* ``pfo_recommend_basket_topk_capped_held`` vs ``pfo_recommend_basket_topk_capped`` at the same shape.

Device events around every call; median [min, max] of REPS calls after WARM warm-up calls and the ratios of the medians.  Work the
rows add per user: one broadcast LDS read per held entry and chunk plus a ballot per 64 entries and round (plain),
one read per held entry and candidate (mean-variance), per candidate once and per pick (basket)."""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pfotgnrec_amd as P

WARM, REPS = 5, 30
I, D, K_TOP, W, N_RET, N_DAYS, N_GROUPS, CAP = 500, 172, 10, 8, 29, 16, 10, 2
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
    groups = rs.randint(-1, N_GROUPS, size=I).astype(np.int32)
    c["groups"] = to(groups)
    c["held_group"] = to(np.where(held >= 0, groups[held.clip(0)], -1).astype(np.int32))   # the group of every held stock
    c["none"] = torch.zeros(U, dtype=torch.int32, device=dev)
    return c


def family(what, U, c, call, extra):
    cap = dict(cand_group=c["groups"], group_cap=CAP)
    fns = (("capped", lambda: call(**cap)), ("held", lambda: call(held_group=c["held_group"], held_len=c["port_len"], **cap)),
           ("held_empty", lambda: call(held_group=c["held_group"], held_len=c["none"], **cap)))
    ms = alternate(fns)
    a, b, n = (fn() for _, fn in fns)
    assert all(torch.equal(x, y) for x, y in zip(a, n)), "empty rows must give the capped list"
    return {"what": what, "U": U, "I": I, "D": D, "k": K_TOP, "groups": N_GROUPS, "group_cap": CAP, "held_stride": W, **extra, "warmup": WARM,
            "reps": REPS, **{n_ + "_us": stats(v) for n_, v in ms.items()}, **ratios(ms, "capped"),
            "users_whose_list_the_holdings_change": int((a[0] != b[0]).any(1).sum())}


def plain(U):
    c = case(U)
    call = lambda **kw: P.recommend_topk(c["ue"], c["ie"], K_TOP, None, c["port_idx"], c["port_len"], **kw)
    return family("pfo_recommend_topk_capped_held vs pfo_recommend_topk_capped, same tensors", U, c, call, {})


def mv_forms(U=512):
    c = case(U)
    args = (c["ue"], c["ie"], K_TOP, c["cand_stock"], c["returns"], c["day"], c["port_idx"], c["port_len"], 2.0, 0.5, None, c["port_idx"],
            c["port_len"])
    out = []
    for name, fn in (("mv", P.recommend_mv_topk), ("basket", P.recommend_basket_topk)):
        out.append(family("pfo_recommend_%s_topk_capped_held vs pfo_recommend_%s_topk_capped, same tensors" % (name, name), U, c,
                          lambda fn=fn, **kw: fn(*args, **kw), {"W": W, "n_ret": N_RET}))
    return out


if __name__ == "__main__":
    for U in (50000, 512):
        print(json.dumps(plain(U)), flush=True)
    for line in mv_forms():
        print(json.dumps(line), flush=True)
