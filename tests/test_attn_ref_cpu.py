"""tests/attn_ref.py on its own, without a GPU: the float64 reference against float64 torch autograd, the run-merged layout
against per-group sums, the generators' invariants, and the discriminating power of the bars the kernels are held to
(tests/test_gpu_attn_forms.py): every wrong-kernel model below misses the true float64 reference by more than the bar in at
least one element, at every case it applies to."""
import numpy as np
import pytest
import torch

import attn_ref as R

F64_RTOL = 1e-11          # the bar of tests/test_oracle_golden_model.py for the oracle's float64 mode
f32, f64 = np.float32, np.float64

PI_CASES = R.per_instance_cases()
RUNS_CASES = R.runs_cases()


def relerr(a, b):
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if b.size else 0.0


def torch_attention(p):
    """The interface written again in float64 torch ops -> loss = sum(ctx * dctx) over the feature and sum-a' columns, and the
    leaves QK, the table (pre-ReLU when nbr_relu), tw, tb."""
    N, K, D, Ef, H, Cp = (p[k] for k in ("N", "K", "D", "Ef", "H", "Cp"))
    C, DE = 2 * D + Ef, D + Ef
    t = lambda a: torch.tensor(np.asarray(a, f64), dtype=torch.float64)
    QK = t(p["QK"]).requires_grad_()
    pre = t(p["nbr_tab"]).requires_grad_()
    tab = torch.relu(pre) if p["nbr_relu"] else pre
    tw, tb = t(p["tw"]).requires_grad_(), t(p["tb"]).requires_grad_()
    rows = torch.tensor(R.rows_of(p))
    valid = torch.tensor(p["nbr_ids"] != 0)
    qr = torch.arange(N) if p["qk_row"] is None else torch.tensor(p["qk_row"].astype(np.int64))
    q = QK[qr][:, :H * Cp].reshape(N, H, Cp)
    qk = torch.cat([q[:, :, :C]], dim=2)
    kn = tab[rows][:, :, :D]
    ke = t(p["edge_feat"]).reshape(-1, max(Ef, 1))[torch.tensor(p["eidx"].astype(np.int64))][:, :, :Ef] if Ef else torch.zeros(N, K, 0, dtype=torch.float64)
    dt = t(p["dt"])[:, :, None]
    lin = dt * tw + tb
    arg32 = t(R.T.fmaf(p["dt"].reshape(N, K, 1), p["tw"], p["tb"]))
    arg = arg32 + (lin - lin.detach())                             # the value of the fp32 FMA, the derivative of dt w + b
    key = torch.cat([kn, ke, torch.cos(arg)], dim=2)               # [N, K, C]
    s = p["scale_f32"] * torch.einsum("nhc,nkc->nhk", qk, key)
    s = s.masked_fill(~valid[:, None, :], float("-inf"))
    some = valid.any(dim=1)
    a = torch.zeros(N, H, K, dtype=torch.float64)
    a[some] = torch.softmax(s[some], dim=2)
    ks = t(np.where(p["keep"], float(R.keep_scale_of(p, f64)), 0.0))
    ap = a * ks
    ctx = torch.einsum("nhk,nkc->nhc", ap, key)
    suma = ap.sum(dim=2)
    g = t(p["dctx"]).reshape(N, H, Cp)
    loss = (ctx * g[:, :, :C]).sum() + (suma * g[:, :, C]).sum()
    return loss, dict(QK=QK, pre=pre, tw=tw, tb=tb), ctx, a, suma


AUTOGRAD_CASES = [("direct_relu", dict(D=32, Ef=4, H=2, K=7, relu=1)), ("table_share_p", dict(D=12, Ef=4, H=4, K=5, p_drop=0.3, table=True, qk_share=True)),
                  ("table_big", dict(D=64, Ef=0, H=1, K=3, table=True, big=True)), ("direct_p", dict(D=30, Ef=6, H=2, K=64, p_drop=0.5)),
                  ("wide", dict(D=172, Ef=64, H=2, K=6, p_drop=0.1, table=True))]


@pytest.mark.parametrize("name,kw", AUTOGRAD_CASES, ids=[c[0] for c in AUTOGRAD_CASES])
def test_float64_reference_against_torch_autograd(name, kw):
    """Forward and the hand-written backward against float64 autograd at 1e-11: the gradients of QK (per-instance rows summed
    over the instances that share a row), of the table rows (plain-stored rows through the ReLU mask, or the per-row sums), of
    tw and of tb - with padding rows, shared table rows, qk_row sharing, a dropout multiplier and nbr_relu."""
    p = R.make_case(**kw)
    p["scale_f32"] = float(f32(p["scale"]))
    N, K, D, H, Cp = p["N"], p["K"], p["D"], p["H"], p["Cp"]
    C = 2 * D + p["Ef"]
    fo, _ = R.forward(p, f64)
    loss, leaves, ctx, a, suma = torch_attention(p)
    got_ctx = fo["ctx"].reshape(N, H, Cp)
    assert relerr(got_ctx[:, :, :C], ctx.detach().numpy()) < F64_RTOL
    assert relerr(got_ctx[:, :, C], suma.detach().numpy()) < F64_RTOL
    assert relerr(fo["attw"], a.detach().numpy()) < F64_RTOL
    some = (p["nbr_ids"] != 0).any(axis=1)
    assert np.array_equal(fo["inv"], (~some).astype(np.uint8)) and np.all(got_ctx[:, 0, C + 1] == some) and not got_ctx[:, :, C + 2:].any()
    assert not got_ctx[:, 1:, C + 1].any() and not got_ctx[~some].any() and not fo["attw"][p["nbr_ids"][:, None, :].repeat(H, 1) == 0].any()
    loss.backward()
    bo, _ = R.backward(p, fo["ctx"], fo["attw"], f64)
    dq = np.zeros_like(p["QK"], dtype=f64)
    qr = np.arange(N) if p["qk_row"] is None else p["qk_row"]
    np.add.at(dq, qr, np.pad(bo["dQK"], ((0, 0), (0, p["qk_ld"] - H * Cp))))
    assert relerr(dq, leaves["QK"].grad.numpy()) < F64_RTOL
    assert not bo["dQK"].reshape(N, H, Cp)[:, :, C:].any() and not bo["dQK"][~some].any()
    gt = leaves["pre"].grad.numpy()[:, :D]
    if p["nbr_row"] is None:
        full = np.zeros((p["nbr_rows"], D))
        full[p["nbr_row_base"]:p["nbr_row_base"] + N * K] = bo["d_slot"]
        assert relerr(full, gt) < F64_RTOL
    else:
        assert relerr(bo["d_tab"], gt) < F64_RTOL
    assert relerr(bo["dw"], leaves["tw"].grad.numpy()) < F64_RTOL
    assert relerr(bo["db"], leaves["tb"].grad.numpy()) < F64_RTOL


@pytest.mark.parametrize("name,kw", RUNS_CASES, ids=[c[0] for c in RUNS_CASES])
def test_run_merged_layout_equals_group_sums(name, kw):
    """For any set of live rows that closes every group - here the kernel's (a run ends at a change of row, at a count step
    beyond 64 - K and at every fourth position) and the coarsest (one row per group) - the live rows summed per group are the
    per-instance dQK summed per group, rows that are not live stay untouched, and empty table rows sum to zero."""
    p = R.make_runs_case(**kw)
    R.check_invariants(p)
    out, _ = R.reference(p)
    seg_ptr, members, seg_of = R.grouping(p["qk_row"], p["nodes"], p["cap_rows"], p["run_cnt"])
    M = len(members)
    assert M == seg_ptr[p["n_rows"]] and (kw.get("groups") is not R.GROUPS_ONE or M == 1) and (kw.get("groups") is not R.GROUPS_SEVEN or M == 7)
    has = (p["nbr_ids"] != 0).any(axis=1)
    for live in (model_live(p, members, seg_of), np.array([q + 1 == M or seg_of[q + 1] != seg_of[q] for q in range(M)])):
        rows = R.runs_rows(out["dQK"], members, seg_of, live)
        assert np.isnan(rows[~live]).all() and np.isfinite(rows[live]).all()
        sums = np.zeros((p["n_rows"], rows.shape[1]))
        for q in np.flatnonzero(live):
            sums[seg_of[q]] += rows[q]
        ref = R.group_sums(out["dQK"], members, seg_ptr, p["n_rows"])
        assert relerr(sums, ref) < 1e-13
        assert not ref[np.diff(seg_ptr[:p["n_rows"] + 1]) == 0].any()
    # instances without a neighbour own zero rows: leaving them out of every run loses nothing
    assert not out["dQK"][~has].any()


def model_live(p, members, seg_of):
    """The live flags the run-merged kernel produces (attn_bwd_runs.hip attn_bwd_runs_kernel), for the layout test only: a sum is stored
    at the last member WITH a neighbour before the row changes, the count steps by more than 64 - K from the run's first, or
    the chunk of four positions ends."""
    M, K = len(members), p["K"]
    has = (p["nbr_ids"] != 0).any(axis=1)
    live = np.zeros(M, bool)
    for m0 in range(0, M, R.RUN_CHUNK):
        slot, cnt0, acc = -1, 0, -1
        for m in range(m0, min(M, m0 + R.RUN_CHUNK)):
            n = members[m]
            d = p["run_cnt"][n] - cnt0
            if p["qk_row"][n] != slot or d < 0 or d > 64 - K:
                if acc >= 0:
                    live[acc] = True
                slot, cnt0, acc = p["qk_row"][n], p["run_cnt"][n], -1
            if has[n]:
                acc = m
        if acc >= 0:
            live[acc] = True
    return live


@pytest.mark.parametrize("cid,form,kw", PI_CASES, ids=[c[0] for c in PI_CASES])
def test_generator_invariants_per_instance(cid, form, kw):
    p = R.make_case(**kw)
    R.check_invariants(p)
    cnt = (p["nbr_ids"] != 0).sum(axis=1)
    assert set(cnt) >= {0, 1, min(2, p["K"]), p["K"]}
    assert np.all(p["dt"][p["nbr_ids"] == 0] == p["dt"][p["nbr_ids"] == 0].round()) and p["Cp"] % 4 == 0 and p["Cp"] >= 2 * p["D"] + p["Ef"] + 2
    if kw.get("big"):
        assert np.abs(R.T.fmaf(p["dt"][..., None], p["tw"], p["tb"])[p["nbr_ids"] != 0]).max() > 2.0e7


def test_generator_covers_the_group_structures():
    p = R.make_runs_case(32, 4, 2, 20)
    R.check_invariants(p)
    seg_ptr, members, seg_of = R.grouping(p["qk_row"], p["nodes"], p["cap_rows"], p["run_cnt"])
    sizes = np.diff(seg_ptr)
    cnts = [list(p["run_cnt"][members[seg_ptr[s]:seg_ptr[s + 1]]]) for s in range(p["cap_rows"]) if sizes[s]]
    assert 1 in sizes and 9 in sizes and [7] * 9 in cnts                                  # one member; nine of equal count
    assert any(np.all(np.diff(c) == 1) and len(c) > 2 for c in cnts) and any(np.all(np.diff(c) == 2) and len(c) > 2 for c in cnts)
    assert any(np.diff(c).max() > 64 - 20 for c in cnts if len(c) > 1)                    # a flush inside a group
    assert any(min(c) < 20 < max(c) for c in cnts)                                        # cnt grows through K
    assert any(c[0] == 0 for c in cnts)                                                   # a member with no valid neighbour
    assert (sizes[1:p["n_rows"]] == 0).any() and p["n_rows"] < p["cap_rows"]              # empty rows; *n_rows below the capacity
    assert (p["nodes"] == 0).sum() == 2 and len(members) == p["N"] - 2                    # padding instances are left out
    # without a key the order inside a group is by instance
    s2, m2, _ = R.grouping(p["qk_row"], p["nodes"], p["cap_rows"], None)
    assert np.array_equal(s2, seg_ptr) and all(list(m2[s2[s]:s2[s + 1]]) == sorted(m2[s2[s]:s2[s + 1]]) for s in range(p["cap_rows"]))
    # lists that are not shifts: the same problem, shuffled slots
    q = R.make_runs_case(32, 4, 2, 20, shifts=False)
    R.check_invariants(q)


def _misses(p, perturb, ref64, bars, n_rep):
    out, _ = R.reference(p, perturb, f64, n_rep)
    worst = 0.0
    for k in R.OUTPUTS:
        if ref64[k] is None:
            continue
        worst = max(worst, R.worst_ratio(out[k], ref64[k], bars[k]))
    return worst


def _discriminate(p, n_rep=2):
    ref64, mag = R.reference(p)
    ref32, _ = R.reference(p, None, f32)
    bars = {k: R.bar(ref32[k], ref64[k], mag[k])[0] for k in R.OUTPUTS if ref64[k] is not None}
    for k in bars:                                                 # the fp32 reference itself sits inside the bar
        assert R.worst_ratio(ref32[k], ref64[k], bars[k]) <= 1.0 / R.ATTN_MARGIN + 1e-12, k
    tried = []
    for perturb in R.PERTURBATIONS:
        if not R.applies(perturb, p, n_rep):
            continue
        w = _misses(p, perturb, ref64, bars, n_rep)
        assert w > 1.0, "%s stays under the bar (worst |wrong - ref64| / bar = %.3g)" % (perturb, w)
        tried.append(perturb)
    return tried


@pytest.mark.parametrize("cid,form,kw", PI_CASES, ids=[c[0] for c in PI_CASES])
def test_discriminating_power_per_instance(cid, form, kw):
    tried = _discriminate(R.make_case(**kw))
    assert "drop_last_key" in tried and ({"time_col_off", "no_scale_key_side"} <= set(tried) or kw["K"] == 1)


@pytest.mark.parametrize("name,kw", RUNS_CASES, ids=[c[0] for c in RUNS_CASES])
def test_discriminating_power_run_merged(name, kw):
    tried = _discriminate(R.make_runs_case(**kw))
    assert {"drop_last_key", "time_col_off"} <= set(tried)
    if kw.get("groups") is None:
        assert {"shift_off", "replica_dropped"} <= set(tried)


def test_every_perturbation_is_exercised():
    seen = set()
    for _, _, kw in PI_CASES:
        p = R.make_case(**kw)
        seen |= {x for x in R.PERTURBATIONS if R.applies(x, p, 2)}
    assert seen == set(R.PERTURBATIONS)
