"""tests/memory_ref.py on its own, without a GPU: the float64 statements against float64 torch autograd and against the
oracle, and the discriminating power of what the kernels are held to (tests/test_gpu_memory_forms.py): every wrong model of
``memory_ref.MUTANTS`` misses the true reference by more than the bar - or differs from the exact arrays - on the shared
case lists."""
import numpy as np
import pytest
import torch

import memory_ref as R
import observe_ref as O
from oracle import tgn_oracle as T

F64_RTOL = 1e-11
f32, f64 = np.float32, np.float64


def relerr(a, b):
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if b.size else 0.0


# ------------------------------------------------------------------------------------------------ the references are right
@pytest.mark.parametrize("D,rows", [(4, 3), (12, 7), (100, 5)])
def test_gate_backward_against_float64_grucell_autograd(D, rows):
    """gates = r | z | n | gh_n from the cell's weights; d gi and d gh are the gradients of the two pre-activation blocks:
    with one row per call they are the gradients of the two bias vectors."""
    torch.manual_seed(D + rows)
    K = 3 * D + 4
    cell = torch.nn.GRUCell(K, D).double()
    x, h, dh = (torch.randn(rows, n, dtype=torch.float64) for n in (K, D, D))
    hm = np.array([(s % 3) != 1 for s in range(rows)], np.uint8)
    with torch.no_grad():
        gi, gh = x @ cell.weight_ih.T + cell.bias_ih, h @ cell.weight_hh.T + cell.bias_hh
        r, z = torch.sigmoid(gi[:, :D] + gh[:, :D]), torch.sigmoid(gi[:, D:2 * D] + gh[:, D:2 * D])
        n = torch.tanh(gi[:, 2 * D:] + r * gh[:, 2 * D:])
        gates = torch.cat([r, z, n, gh[:, 2 * D:]], dim=1).numpy()
        assert relerr(((1 - z) * n + z * h).numpy(), cell(x, h).numpy()) < F64_RTOL        # these ARE the cell's gates
    want_gi, want_gh = np.zeros((rows, 3 * D)), np.zeros((rows, 3 * D))
    for s in range(rows):
        if not hm[s]:
            continue
        cell.zero_grad()
        cell(x[s:s + 1], h[s:s + 1]).backward(dh[s:s + 1])
        want_gi[s], want_gh[s] = cell.bias_ih.grad.numpy(), cell.bias_hh.grad.numpy()
    # d h' arrives as two replicas and the rows' own gradient
    parts = np.random.RandomState(0).randn(2, rows, D)
    c = dict(D=D, rows=rows, det=0, gates=gates, h_rows=h.numpy(), hm=hm, d_h0=parts, d_extra=dh.numpy() - parts.sum(axis=0))
    got, mag = R.gru_gates_bwd(c, f64)
    assert relerr(got["dgi"], want_gi) < F64_RTOL and relerr(got["dgh"], want_gh) < F64_RTOL
    dead = hm == 0
    assert not got["dgi"][dead].any() and not got["dgh"][dead].any() and not mag["dgi"][dead].any() and not mag["dgh"][dead].any()
    assert np.all(mag["dgi"][~dead] >= np.abs(got["dgi"][~dead])) and np.all(mag["dgh"][~dead] >= np.abs(got["dgh"][~dead]))


def test_gate_backward_fixed_point_input():
    """det: dh = table * 2^-40 exactly in float64, rounded once to fp32 in the float32 statement."""
    c = R.make_gates_case(8, 3, 1, 1, True, hm="ones")
    f = dict(c, det=0, d_h0=(c["d_h0"].astype(f64) / R.DET_SCALE)[None])
    a, _ = R.gru_gates_bwd(c, f64)
    b, _ = R.gru_gates_bwd(f, f64)
    assert np.array_equal(a["dgi"], b["dgi"]) and np.array_equal(a["dgh"], b["dgh"])
    a32, _ = R.gru_gates_bwd(c, f32)
    b32, _ = R.gru_gates_bwd(dict(f, d_h0=f["d_h0"].astype(f32)), f32)
    assert np.array_equal(a32["dgi"], b32["dgi"])
    mags = np.abs(c["d_h0"][:3].astype(f64) / R.DET_SCALE)
    assert mags.min() < 1e-8 and mags.max() > 1e2                        # the case spans the magnitudes the issue asks for


@pytest.mark.parametrize("D,L", [(4, 1), (10, 2), (100, 4)])
def test_cq_backward_against_float64_autograd(D, L):
    c = R.make_cq_case(D, L, "final")
    c.update(d_bq=np.zeros_like(c["d_bq"]), d_Wq=np.zeros_like(c["d_Wq"]), d_tb=np.zeros_like(c["d_tb"]), tb_add=None)
    t = lambda a: torch.tensor(np.asarray(a, f64), dtype=torch.float64, requires_grad=True)
    Wq, bq, tb, gq = t(c["Wq"]), t(np.zeros((L, 2 * D))), t(c["tb"]), torch.tensor(c["gq"].astype(f64))
    loss = sum((gq[l] * (Wq[l][:, D:] @ torch.cos(tb) + bq[l])).sum() for l in range(L))
    loss.backward()
    got, _ = R.cq_backward(c, f64)
    assert relerr(got["d_bq"], bq.grad.numpy()) < F64_RTOL and relerr(got["d_Wq"], Wq.grad.numpy()) < F64_RTOL
    assert relerr(got["d_tb"], tb.grad.numpy()) < F64_RTOL
    assert not got["d_Wq"][:, :, :D].any()
    # a stored partial of the top layer handed to the final launch of the others is the same gradient
    if L > 1:
        top = {k: (v[L - 1:] if k in ("gq", "Wq", "d_bq", "d_Wq") else v) for k, v in c.items()}
        rest = {k: (v[:L - 1] if k in ("gq", "Wq", "d_bq", "d_Wq") else v) for k, v in c.items()}
        part, _ = R.cq_backward(dict(top, L=1, form="part"), f64)
        fin, _ = R.cq_backward(dict(rest, L=L - 1, tb_add=part["tb_part"]), f64)
        assert relerr(fin["d_tb"], tb.grad.numpy()) < F64_RTOL
    # the bin fold
    b = R.make_cq_case(D, L, "bins", n_bins=5)
    got, _ = R.cq_backward(b, f64)
    base, _ = R.cq_backward(dict(b, form="final"), f64)
    assert relerr(got["d_tw"], b["d_tw"].astype(f64) + b["dtime"][:, :D].sum(axis=0)) < F64_RTOL
    assert relerr(got["d_tb"], base["d_tb"] + b["dtime"][:, D:].sum(axis=0)) < F64_RTOL


def test_message_time_block_against_the_oracle_time_encode():
    for kind in R.MSG_TS_KINDS:
        c = R.make_msg_case(100, 64, 65, ts_kind=kind)
        tab, mt, has, named = R.msg_store(c)
        X = np.flatnonzero(named)
        delta = mt[X] - c["last_update"][X]
        assert (delta < 0).any() and (delta > 0).any()
        want = T.time_encode(delta, c["tw"], c["tb"], dtype=f64)
        assert np.array_equal(tab[X][:, 2 * c["D"] + c["Ef"]:], want)
        assert np.abs(T.time_encode(delta, c["tw"], c["tb"], dtype=f32) - want).max() < 2.0 ** -22


@pytest.mark.parametrize("seed,B", [(1, 1), (2, 40), (3, 200)])
def test_store_persist_and_select_against_the_observe_oracle(seed, B):
    """One ObserveOracle.observe batch on a random world = observe-select, the GRU on the selected rows, persist, message
    store - state tables equal to the oracle's (copies and times bit for bit, the cosine block within an fp32 rounding)."""
    D, Ef, n_nodes = 8, 4, 30
    w = O.random_world(seed, n_nodes, D, Ef, 3 * B + 5)
    o = O.world_oracle(w)
    mem0, lu0, tab0, mt0, has0 = (np.array(a, copy=True) for a in w["state"])
    rs = np.random.RandomState(seed)
    src, dst = rs.randint(1, n_nodes, B).astype(np.int32), rs.randint(1, n_nodes, B).astype(np.int32)
    ts, eidx = 100.0 + np.sort(rs.randint(0, 50, B)).astype(f64), rs.permutation(3 * B + 5)[:B].astype(np.int32)
    o.observe(src, dst, ts, eidx)
    touched, slot, _ = R.observe_select(src, dst, has0.astype(np.uint8), np.zeros(n_nodes, np.int32), 0, np.full(n_nodes, -1, np.int32))
    ids = np.unique(np.concatenate([src, dst]))
    ids = ids[has0[ids]]
    assert sorted(touched.tolist()) == ids.tolist() and np.array_equal(slot[touched], np.arange(len(touched)))
    upd = np.zeros((len(ids) + 1, D), f32)
    if len(ids):
        upd[slot[ids]] = T.gru_cell(tab0[ids], mem0[ids], *o._gru())[0]
    mem1, lu1, _ = R.persist(src, dst, slot, upd, has0, mt0, mem0, lu0)
    assert np.array_equal(mem1.view(np.int32), o.memory.astype(f32).view(np.int32)) and np.array_equal(lu1.view(np.int32), o.last_update.astype(f32).view(np.int32))
    c = dict(B=B, D=D, Ef=Ef, src=src, dst=dst, ts=ts, eidx=eidx, memory=mem1, last_update=lu1, edge_feat=o.edge_features,
             tw=w["params"]["time_encoder.w.weight"].reshape(-1), tb=w["params"]["time_encoder.w.bias"], msg_table=tab0, msg_time=mt0,
             has_msg=has0.astype(np.uint8))
    tab, mt, has, named = R.msg_store(c)
    _, _, otab, omt, ohas = o.tables()
    # the oracle clears the positives' lists and keeps everybody else's: the store names exactly the positives
    assert np.array_equal(np.flatnonzero(named), np.unique(np.concatenate([src, dst])))
    assert np.array_equal(has > 0, ohas) and np.array_equal(mt[ohas].view(np.int32), omt[ohas].view(np.int32))
    C = 2 * D + Ef
    assert np.array_equal(tab[ohas][:, :C].astype(f32).view(np.int32), otab[ohas][:, :C].astype(f32).view(np.int32))
    assert np.abs(tab[ohas][:, C:] - otab[ohas][:, C:]).max() < 2.0 ** -22
    O.check_tables((mem1, lu1, tab.astype(f32), mt, has), o.tables())


def test_small_statements():
    assert R.iscan([3, 0, 2, 1]).tolist() == [0, 3, 3, 5]
    m, mag = R.mean([1.0, -2.0, 4.0])
    assert m == 1.0 and mag == 7.0 / 3
    d = np.arange(24, dtype=f32) + 1
    z = R.zero_rows(d, 2, 4, 2, 12)
    assert not z[:8].any() and not z[12:20].any() and np.array_equal(z[8:12], d[8:12]) and np.array_equal(z[20:], d[20:])
    slot, touched, cnt = R.compact(6, nodes0=[4, 1, 4, -1, 6], extra=[5, 1, 0, 0, 9])
    assert slot.tolist() == [2, 0, -1, -1, 1, 3] and touched.tolist() == [1, 4, 0, 5] and cnt.tolist() == [4, 2]
    t, s, rep = R.observe_select(np.array([1, 2, 1]), np.array([3, 1, 4]), np.array([0, 1, 0, 1, 1]), np.zeros(5, np.int32), 6, np.full(5, -1))
    assert t.tolist() == [3, 1, 4] and s.tolist() == [-1, 1, -1, 0, 2] and rep.tolist() == [0, 11, 8, 10, 12]
    assert R.msg_store_needs_winner(8193) and not R.msg_store_needs_winner(8192)


# ------------------------------------------------------------------------------------------------ the bars can see
def beyond(case_ref, ref32, ref64, mag):
    """worst |wrong - ref64| / bar over the outputs of one case."""
    worst = 0.0
    for k in ref64:
        b, _ = R.bar(ref32[k], ref64[k], mag[k])
        worst = max(worst, R.worst_ratio(case_ref[k], ref64[k], b))
    return worst


GATE_CASES = R.gates_cases()


def gate_mutant_applies(m, kw):
    if kw["hm"] == "zeros":
        return False
    return {"no_d_extra": kw["extra"], "last_replica_dropped": not kw["det"], "det_scale_39": bool(kw["det"])}.get(m, True)


@pytest.mark.parametrize("mutant", R.MUTANTS["gates"])
def test_gate_backward_mutants_miss_the_bar(mutant):
    seen = 0
    for cid, kw in GATE_CASES:
        if not gate_mutant_applies(mutant, kw):
            continue
        c = R.make_gates_case(**kw)
        assert c["hm"][:c["rows"]].any()
        r64, mag = R.gru_gates_bwd(c, f64)
        r32, _ = R.gru_gates_bwd(c, f32)
        assert beyond(r32, r32, r64, mag) <= 1.0, cid                   # the float32 statement itself passes
        wrong, _ = R.gru_gates_bwd(c, f32, mutant=mutant)
        caught = beyond(wrong, r32, r64, mag) > 1.0
        # (a table value of 1e-9 beside a d_extra of order 1 is below that element's own rounding: the scale shows wherever
        #  a live row holds a value of the gradient's own size, and in every case without d_extra)
        assert caught or (mutant == "det_scale_39" and kw["extra"]), (mutant, cid)
        seen += caught
    assert seen >= 8


CQ_CASES = R.cq_cases()


@pytest.mark.parametrize("mutant", R.MUTANTS["cq"])
def test_cq_backward_mutants_miss_the_bar(mutant):
    seen = 0
    for cid, kw in CQ_CASES:
        if kw["D"] == 172 and kw["L"] == 4:
            continue                                                    # (the largest shape adds nothing here)
        applies = {"no_tb_add": kw["form"] != "part", "last_bin_dropped": kw["form"] == "bins" and kw.get("n_bins", 0) % 4 != 0}.get(mutant, True)
        if not applies:
            continue
        c = R.make_cq_case(**kw)
        r64, mag = R.cq_backward(c, f64)
        r32, _ = R.cq_backward(c, f32)
        assert beyond(r32, r32, r64, mag) <= 1.0, cid
        wrong, _ = R.cq_backward(c, f32, mutant=mutant)
        assert beyond(wrong, r32, r64, mag) > 1.0, (mutant, cid)
        seen += 1
    assert seen >= 8


@pytest.mark.parametrize("mutant", R.MUTANTS["fold"])
def test_fold_parts_mutants_miss_the_bar(mutant):
    seen = 0
    for n in (1, 65):
        for n_parts in R.FOLD_PARTS:
            if mutant == "rows_from_1024_dropped" and n_parts <= 1024:
                continue
            c = R.make_fold_case(n, n_parts)
            s, o, m64, m_out = R.fold_parts(c["parts"], c["out0"], 1)
            b64, b_out = R.fold_bars(n_parts, m64, m_out)
            ws, wo, _, _ = R.fold_parts(c["parts"], c["out0"], 1, mutant=mutant)
            assert R.worst_ratio(c["parts"].sum(axis=0), s, b64) <= 1.0   # a plain fp64 sum passes
            assert max(R.worst_ratio(ws, s, b64), R.worst_ratio(wo.astype(f32), o, b_out)) > 1.0, (mutant, n, n_parts)
            seen += 1
    assert seen >= 4


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


MSG_CASES = R.msg_cases()


@pytest.mark.parametrize("mutant", R.MUTANTS["msg"])
def test_message_store_mutants_differ(mutant):
    seen = []
    for cid, kw, path in MSG_CASES:
        if kw["B"] > 300 and kw["D"] != 4:
            continue
        c = R.make_msg_case(**kw)
        assert R.msg_store_needs_winner(c["B"]) == (path == "winner")
        good, wrong = R.msg_store(c), R.msg_store(c, mutant=mutant)
        tab, mt, has, named = good
        assert named[np.unique(np.concatenate([c["src"], c["dst"]]))].all() and named.sum() == len(np.unique(np.concatenate([c["src"], c["dst"]])))
        assert np.array_equal(tab[~named], c["msg_table"][~named].astype(f64)) and np.array_equal(has[~named], c["has_msg"][~named])
        if not same(good, wrong):
            d = np.abs(good[0] - wrong[0])
            assert mutant == "msg_time_truncated" or d.max() > 2 * R.COS_BAR
            seen.append(cid)
    print(mutant, "seen in", len(seen), "of", len(MSG_CASES))
    assert len(seen) >= 4
    if mutant in ("first_event_wins", "msg_time_truncated"):
        assert any("B8200" in s for s in seen)


def test_message_cases_pin_every_step_of_the_later_event_scan():
    """An event looks for a later event of its node 64 ids per step.  With 7 nodes over hundreds of events some later event
    turns up in nearly every step, so a scan that left steps out would still find one; the 'twice' cases hold nodes named by
    exactly two events, the second of which lies in step 1, 2, 3 and 4 of the first one's scan - the only one it can find -
    within one side and across both."""
    steps = [R.msg_scan_step(a, b) for a, b in R.MSG_TWICE]
    assert sorted(steps) == [1, 2, 3, 4] and any(a < 300 <= b for a, b in R.MSG_TWICE) and any(b < 300 for a, b in R.MSG_TWICE)
    twice = [(cid, kw) for cid, kw, path in MSG_CASES if kw.get("twice")]
    assert sorted((kw["D"], kw["Ef"]) for _, kw in twice) == sorted(R.MSG_SHAPES) and {kw["ts_kind"] for _, kw in twice} == set(R.MSG_TS_KINDS)
    for cid, kw in twice:
        c = R.make_msg_case(**kw)
        ev = np.concatenate([c["src"], c["dst"]])
        for k, pair in enumerate(kw["twice"]):
            assert np.flatnonzero(ev == c["n_nodes"] - len(kw["twice"]) + k).tolist() == list(pair), cid
        # the two events leave different rows, so a first event that also wrote would show: another partner, edge row or time
        tab, mt, _, _ = R.msg_store(c)
        first, _, _, _ = R.msg_store(c, mutant="first_event_wins")
        for k in range(len(kw["twice"])):
            X = c["n_nodes"] - len(kw["twice"]) + k
            assert not np.array_equal(tab[X], first[X]), (cid, X)


COMPACT_CASES = R.compact_cases()


@pytest.mark.parametrize("mutant", R.MUTANTS["compact"])
def test_compaction_mutants_differ(mutant):
    seen = []
    for cid, kw in COMPACT_CASES:
        c = R.make_compact_case(**kw)
        good = R.compact_of_case(c)
        slot, touched, cnt = good
        # the statement's own invariants: slot and touched are inverse, class 1 ascending, class 2 ascending behind it
        assert np.array_equal(slot[touched], np.arange(len(touched))) and (slot >= 0).sum() == len(touched) == cnt[0]
        assert np.all(np.diff(touched[:cnt[1]]) > 0) and np.all(np.diff(touched[cnt[1]:]) > 0)
        if not same(good, R.compact_of_case(c, mutant)):
            seen.append(cid)
    print(mutant, "seen in", len(seen), "of", len(COMPACT_CASES))
    assert len(seen) >= 2
    if mutant != "out_of_range_clipped":
        for n in R.COMPACT_SIZES[-2:]:                                  # one full stride of the look-back, and two
            assert any(s.startswith("n%d-" % n) for s in seen), n
    assert [R.compact_lookback_strides(n) for n in R.COMPACT_SIZES] == [0, 0, 0, 0, 1, 1, 1, 2]


def test_compaction_second_stride_reads_a_count_of_either_class():
    """Workgroup b looks back over b published counts, 1 024 per stride: the last of 1 026 workgroups reads count 1 024 in
    its second stride.  A second stride that was skipped shows only if that count is not zero."""
    n = R.COMPACT_SIZES[-1]
    assert (n + 1023) // 1024 == 1026 and R.compact_lookback_strides(n) == 2 and R.compact_lookback_strides(1025 * 1024) == 1
    for marked in (False, True):
        c = R.make_compact_case(n, True, marked)
        _, touched, cnt = R.compact_of_case(c)
        far = (touched >> 10) == 1024
        # (the last workgroup writes both counts from its look-back, and holds a class-1 node whose slot comes from it too)
        assert far[:cnt[1]].any() and far[cnt[1]:].any() and (touched[:cnt[1]] >> 10).max() == 1025


def test_compaction_cases_cover_what_the_issue_names():
    kinds = set()
    for cid, kw in COMPACT_CASES:
        c = R.make_compact_case(**kw)
        _, _, cnt = R.compact_of_case(c)
        kinds.add((cnt[1] == 0, cnt[0] > cnt[1]))
        if kw["two"]:
            ex = c["extra"].astype(np.int64)
            assert (ex < 0).any() and (ex >= c["n_nodes"]).any() and len(np.unique(ex)) < len(ex)
            if not kw.get("empty1") and c["n_nodes"] > 1:
                assert np.intersect1d(ex, c["nodes0"]).size
    assert (True, True) in kinds and (False, True) in kinds and (False, False) in kinds


@pytest.mark.parametrize("mutant", R.MUTANTS["observe"])
def test_observe_select_mutants_differ(mutant):
    seen = []
    for B in R.OBSERVE_BATCHES:
        c = R.make_observe_case(B)
        n = c["n_nodes"]
        state = [(np.zeros(n, np.int32), np.full(n, -1, np.int32)), (np.zeros(n, np.int32), np.full(n, -1, np.int32))]
        for k, (src, dst, has) in enumerate(c["batches"]):
            out = []
            for j, m in enumerate((None, mutant)):
                rep, slot = state[j]
                t, slot, rep = R.observe_select(src, dst, has, rep, 2 * B * k, slot, mutant=m)
                state[j] = (rep, slot)
                out.append((t, slot))
            if not same(out[0], out[1]):
                seen.append((B, k))
    assert len({b for b, _ in seen}) >= 4, seen
    if mutant == "stamps_without_base":
        assert all(k > 0 for _, k in seen)
