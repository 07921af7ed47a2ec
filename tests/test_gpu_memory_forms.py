"""Every launcher of the memory-side interface (pfotgnrec_amd/csrc/memory.hpp) launched alone through its pfo_debug_* probe and
held to the host model of tests/memory_ref.py.

Each case
  * asserts the path query before it launches (message store: inline / winner; gate backward: float4 / scalar kernel; scan:
    sweeps; part fold: rows in flight), so that a dispatch change cannot quietly turn one case into a copy of another,
  * gives every output a canary (quiet NaNs with the element's index as payload, a sentinel for integers) and a tail, and
    compares bit for bit wherever the contract leaves memory alone: rows at or beyond the device-side count, rows of nodes
    nobody names, the tail,
  * ends every float operand in NaN slack and keeps every index in range over its whole allocation: a wrong case gives a
    wrong number, never a stray access.

Integer and copy launchers are exact.  Bars of the others (DESIGN.md "Memory-side launchers under test"): gate backward and
folded query-bias backward MARGIN * max(e32, 2^-23) * mag with e32 the gap between the reference's own float32 and float64
statements; part fold n_parts 2^-52 sum |parts| (+ 2^-23 mag for the fp32 output); mean 8 * 2^-23 * sum |x| / n; the message
row's cosine block 5e-7 absolute.  Nothing measured on the device enters a bar."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

from pfotgnrec_amd import _lib
import memory_ref as R

DEV = "cuda:0"
f32, f64 = np.float32, np.float64
TAIL = 16
ISENT = -0x5A5A5A5
BSENT = 0xAB
FIGURES = {}               # launcher -> (largest error / bar seen, the case)
PATHS_SEEN = set()


@pytest.fixture(autouse=True)
def stop_after_a_gpu_error():
    """A kernel that faulted leaves the device in an error state: the run ends there instead of launching more on it."""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:                                             # noqa: BLE001 - whatever the runtime raises
        pytest.exit("the GPU reported an error (%s): nothing more is launched" % e, returncode=3)


def canary(n):
    return (np.uint32(0x7FC00000) | (np.arange(n, dtype=np.uint32) % np.uint32(0x3FFFFF) + np.uint32(1))).view(np.float32)


def canary64(n):
    return (np.uint64(0x7FF8000000000000) | (np.arange(n, dtype=np.uint64) + np.uint64(1))).view(np.float64)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.itemsize])


def same_bits(a, b):
    return np.array_equal(bits(a), bits(np.ascontiguousarray(b, a.dtype)))


class Bufs:
    """Device copies of a case's arrays, kept alive for the launch.  ``off``: the pointer starts that many elements into its
    allocation.  Inputs end in slack (NaN behind floats, 0 - an in-range index - behind the rest)."""

    def __init__(self):
        self.keep = []

    def put(self, a, dtype=None, off=0):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype).reshape(-1)
        t = torch.full((a.size + off + 64,), float("nan") if a.dtype.kind == "f" else 0, dtype=getattr(torch, a.dtype.name), device=DEV)
        t[off:off + a.size] = torch.from_numpy(a).to(DEV)
        self.keep.append(t)
        return t.data_ptr() + off * a.itemsize

    def out(self, a, off=0):
        """A buffer holding exactly ``a`` (a canary, a table to update, ...) -> (pointer, its device tensor)."""
        a = np.ascontiguousarray(a).reshape(-1)
        t = torch.empty(a.size + off, dtype=getattr(torch, a.dtype.name), device=DEV)
        t[off:] = torch.from_numpy(a).to(DEV)
        self.keep.append(t)
        return t.data_ptr() + off * a.itemsize, t[off:]


def call(name, *args):
    _lib.call(name, *args, _lib.stream_ptr())
    torch.cuda.synchronize()


def note(launcher, ratio, case):
    if ratio >= FIGURES.get(launcher, (-1.0, ""))[0]:
        FIGURES[launcher] = (ratio, case)


def hold(launcher, case, got, ref32, ref64, mag):
    """Per element |got - ref64| <= MARGIN * max(e32, 2^-23) * mag; where mag is 0 the bits of the reference."""
    got = np.asarray(got).reshape(-1)
    r64, r32, mag = (np.asarray(a, f64).reshape(-1) for a in (ref64, ref32, mag))
    b, e32 = R.bar(r32, r64, mag)
    assert np.isfinite(got).all(), "%s %s: an element the call must write still holds the canary (or is not finite)" % (launcher, case)
    z = mag == 0
    assert same_bits(got[z].astype(f32), r64[z].astype(f32)), "%s %s: an element without rounding differs in its bits" % (launcher, case)
    ratio = R.worst_ratio(got[~z], r64[~z], b[~z])
    note(launcher, ratio, case)
    assert ratio <= 1.0, "%s %s: worst error / bar = %.3g (e32 = %.3g 2^-24)" % (launcher, case, ratio, e32 * 2 ** 24)


# ------------------------------------------------------------------------------------------------ compaction
COMPACT_CASES = R.compact_cases()


def run_compact(c, dirty=False):
    n = c["n_nodes"]
    b = Bufs()
    n_scr = int(_lib.byte_count("pfo_debug_compact_scratch_ints", n))
    assert n_scr >= 2 * ((n + 1023) // 1024)
    mark0 = np.zeros(n + TAIL, np.int32)
    if c["marked"]:
        mark0[:n] = c["marks"]
    scr0 = np.zeros(n_scr + TAIL, np.int32)
    if dirty:                                                           # the launcher clears both itself
        mark0[:n] = 1 + (np.arange(n) % 2)
        scr0[:n_scr] = 7
    mark0[n:], scr0[n_scr:] = ISENT, ISENT
    p_mark, mark = b.out(mark0)
    p_scr, scr = b.out(scr0)
    p_slot, slot = b.out(np.full(n + TAIL, ISENT, np.int32))
    p_touched, touched = b.out(np.full(n + TAIL, ISENT, np.int32))
    p_cnt, cnt = b.out(np.full(2 + TAIL, ISENT, np.int32))
    ex = c["extra"]
    call("pfo_debug_touch_compact", b.put(c["nodes0"], np.int32), len(c["nodes0"]), b.put(ex, np.int32), 0 if ex is None else len(ex), n,
         p_mark, p_slot, p_touched, p_cnt, p_scr, n_scr, 0 if dirty else 1, 1 if c["marked"] else 0)
    return tuple(t.cpu().numpy() for t in (slot, touched, cnt, mark, scr))


@pytest.mark.parametrize("cid,kw", COMPACT_CASES, ids=[c[0] for c in COMPACT_CASES])
def test_touch_compact(cid, kw):
    c = R.make_compact_case(**kw)
    n = c["n_nodes"]
    e_slot, e_touched, e_cnt = R.compact_of_case(c)
    nb = (int(_lib.byte_count("pfo_debug_compact_scratch_ints", n)) - 8) // 2
    assert nb == (n + 1023) // 1024 and R.compact_lookback_strides(n) == (nb + 1022) // 1024
    PATHS_SEEN.add("compact lookback %d strides" % R.compact_lookback_strides(n))
    na, n1 = int(e_cnt[0]), int(e_cnt[1])
    if R.compact_lookback_strides(n) >= 2:                              # the count the second stride reads is not zero, in either class
        in_far = (e_touched >> 10) == 1024
        assert in_far[:n1].any() and (in_far[n1:].any() or not kw["two"]) and (e_touched[:n1] >> 10).max() == nb - 1
    slot, touched, cnt, mark, scr = first = run_compact(c)
    assert cnt[:2].tolist() == [na, n1] and np.all(cnt[2:] == ISENT), (cnt[:2], e_cnt)
    assert np.array_equal(slot[:n], e_slot) and np.all(slot[n:] == ISENT), "slot"
    assert np.array_equal(touched[:na], e_touched) and np.all(touched[na:] == ISENT), "touched ids (or a word behind the last one)"
    e_mark = np.zeros(n, np.int32)
    e_mark[e_touched[:n1]], e_mark[e_touched[n1:]] = 1, 2
    assert np.array_equal(mark[:n], e_mark) and np.all(mark[n:] == ISENT), "flags"
    assert np.all(scr[len(scr) - TAIL:] == ISENT), "scratch tail"
    again = run_compact(c)
    assert all(np.array_equal(x, y) for x, y in zip(first, again)), "two launches on fresh cleared scratch differ"
    if not c["marked"]:
        dirty = run_compact(c, dirty=True)                              # marks_are_zero = false: the launcher's own clear
        assert all(np.array_equal(x, y) for x, y in zip(first[:4], dirty[:4])), "the launcher's own clear gives another result"


# ------------------------------------------------------------------------------------------------ scan
@pytest.mark.parametrize("inplace", [False, True], ids=["out", "inplace"])
@pytest.mark.parametrize("n,zero", [(n, False) for n in R.ISCAN_SIZES] + [(5000, True)], ids=[str(n) for n in R.ISCAN_SIZES] + ["5000-zeros"])
def test_iscan(n, zero, inplace):
    counts = np.zeros(n, np.int32) if zero else np.random.RandomState(n % 1000).randint(0, 4, n).astype(np.int32)
    sweeps = _lib.load().pfo_debug_scan_sweeps(n)
    assert sweeps == (2 if n > 1 << 20 else 1)
    PATHS_SEEN.add("scan sweeps %d" % sweeps)
    b = Bufs()
    n_scr = n // 1024 + 16
    p_scr, scr = b.out(np.full(n_scr + TAIL, ISENT, np.int32))
    p_in, t_in = b.out(np.concatenate([counts, np.full(TAIL, ISENT, np.int32)]))
    p_out, t_out = (p_in, t_in) if inplace else b.out(np.full(n + TAIL, ISENT, np.int32))
    call("pfo_debug_iscan", p_in, n, p_out, p_scr, n_scr)
    out = t_out.cpu().numpy()
    assert np.array_equal(out[:n], R.iscan(counts)) and np.all(out[n:] == ISENT)
    assert np.all(scr.cpu().numpy()[n_scr:] == ISENT)
    if not inplace:
        assert np.array_equal(t_in.cpu().numpy()[:n], counts)


# ------------------------------------------------------------------------------------------------ pack / remap
@pytest.mark.parametrize("cap", [1, 5, 300])
@pytest.mark.parametrize("D,Ef", R.MSG_SHAPES)
def test_pack_remap(D, Ef, cap):
    M = 3 * D + Ef
    rs = np.random.RandomState(D + cap)
    n_nodes = cap + 11
    table, memory = rs.randn(n_nodes, M).astype(f32), rs.randn(n_nodes, D).astype(f32)
    has = (rs.rand(n_nodes) < 0.5).astype(np.uint8)
    ids = rs.permutation(n_nodes)[:cap].astype(np.int32)
    slot = rs.randint(-1, cap, n_nodes).astype(np.int32)
    b = Bufs()
    p_tab, p_mem, p_has, p_ids, p_slot = b.put(table), b.put(memory), b.put(has), b.put(ids), b.put(slot)
    for nt in sorted({0, 1, cap}):
        p_nt = b.put(np.array([nt], np.int32))
        for n0 in (1, 255, 257, 70000):
            nodes0 = rs.randint(0, n_nodes, n0).astype(np.int32)
            p_nodes = b.put(nodes0)
            for with_msg in (True, False):
                rows0, h0, hm0 = canary((cap + 2) * M), canary((cap + 2) * D), np.full(cap + 2, BSENT, np.uint8)
                p_rows, rows = b.out(rows0)
                p_h, h = b.out(h0)
                p_hm, hm = b.out(hm0)
                p_idx, idx = b.out(np.full(n0 + TAIL, ISENT, np.int32))
                if with_msg:
                    call("pfo_debug_pack_remap", p_tab, M, p_mem, D, p_has, p_ids, p_nt, cap, p_rows, p_h, p_hm, p_nodes, n0, p_slot, p_idx)
                else:                                                   # the no-memory form: one table, no flags
                    call("pfo_debug_pack_remap", None, M, p_mem, D, None, p_ids, p_nt, cap, None, p_h, None, p_nodes, n0, p_slot, p_idx)
                e_rows, e_h, e_hm, e_idx = R.pack_remap(table if with_msg else None, memory, has, ids, nt, nodes0, slot)
                rows, h, hm, idx = (t.cpu().numpy() for t in (rows, h, hm, idx))
                tag = (nt, n0, with_msg)
                assert same_bits(h[:nt * D], e_h) and same_bits(h[nt * D:], h0[nt * D:]), tag
                assert np.array_equal(idx[:n0], e_idx) and np.all(idx[n0:] == ISENT), tag
                if with_msg:
                    assert same_bits(rows[:nt * M], e_rows) and same_bits(rows[nt * M:], rows0[nt * M:]), tag
                    assert np.array_equal(hm[:nt], e_hm) and np.all(hm[nt:] == BSENT), tag
                else:
                    assert same_bits(rows, rows0) and np.all(hm == BSENT), tag
                del b.keep[-4:]


# ------------------------------------------------------------------------------------------------ zero rows
@pytest.mark.parametrize("n_rep", [1, 3, 8])
@pytest.mark.parametrize("D", [4, 100])
def test_zero_rows(D, n_rep):
    cap = 5
    stride = cap * D + 8
    for nr in (0, 1, cap):
        b = Bufs()
        d0 = canary(n_rep * stride + TAIL)
        p, t = b.out(d0)
        call("pfo_debug_zero_rows", p, b.put(np.array([nr], np.int32)), cap, D, n_rep, stride)
        assert same_bits(t.cpu().numpy(), R.zero_rows(d0, nr, D, n_rep, stride)), nr


# ------------------------------------------------------------------------------------------------ GRU gate backward
def run_gates(c, scalar):
    """-> dgi, dgh [(cap + 2) * 3 D] as the launch left them, their canaries, and the kernel the launcher reported."""
    D, cap, n_rep, det = c["D"], c["cap"], c["n_rep"], c["det"]
    off = 1 if scalar else 0
    stride = cap * D + (5 if scalar else 8)                             # larger than the table; odd for the scalar kernel
    b = Bufs()
    if det:
        p_dh = b.put(c["d_h0"], np.int64)                               # (int64 words stay 8-byte aligned)
    else:
        tab = np.full(n_rep * stride, np.nan, f32)
        for q in range(n_rep):
            tab[q * stride:q * stride + cap * D] = c["d_h0"][q].reshape(-1)
        p_dh = b.put(tab, f32, off)
    p_gates, p_h = b.put(c["gates"], f32, off), b.put(c["h_rows"], f32, off)
    p_ex = b.put(c["d_extra"], f32, off)
    gi0, gh0 = canary((cap + 2) * 3 * D), canary((cap + 2) * 3 * D)[::-1].copy()
    p_gi, gi = b.out(gi0, off)
    p_gh, gh = b.out(gh0, off)
    vec = _lib.load().pfo_debug_gru_gates_bwd_vec(p_gates, p_gi, p_gh, p_h, D, p_dh, stride, p_ex)
    assert vec == (0 if scalar else 1), "the launcher would not take the kernel this case is about"
    PATHS_SEEN.add("gates %s%s" % ("float4" if vec else "scalar", " det" if det else ""))
    call("pfo_debug_gru_gates_bwd", p_gates, p_gi, p_gh, p_h, b.put(c["hm"], np.uint8), b.put(np.array([c["rows"]], np.int32)), cap, D, p_dh,
         n_rep, stride, p_ex, det)
    return gi.cpu().numpy(), gh.cpu().numpy(), gi0, gh0


@pytest.mark.parametrize("kernel", ["float4", "scalar"])
@pytest.mark.parametrize("rows", R.GATE_ROWS)
@pytest.mark.parametrize("D", R.GATE_DIMS)
def test_gru_gates_bwd(D, rows, kernel):
    for kw in R.gates_grid(D, rows):
        c = R.make_gates_case(**kw)
        case = "D%d rows%d rep%d %s %s hm-%s %s" % (D, rows, c["n_rep"], "det" if c["det"] else "f32", "extra" if kw["extra"] else "noextra", kw["hm"], kernel)
        r64, mag = R.gru_gates_bwd(c, f64)
        r32, _ = R.gru_gates_bwd(c, f32)
        gi, gh, gi0, gh0 = run_gates(c, kernel == "scalar")
        w = rows * 3 * D
        assert same_bits(gi[w:], gi0[w:]) and same_bits(gh[w:], gh0[w:]), case + ": rows >= *n_touched touched"
        hold("gru_gates_bwd", case + " dgi", gi[:w], r32["dgi"], r64["dgi"], mag["dgi"])
        hold("gru_gates_bwd", case + " dgh", gh[:w], r32["dgh"], r64["dgh"], mag["dgh"])
        if kw["hm"] == "zeros":
            assert not bits(gi[:w]).any() and not bits(gh[:w]).any(), case


# ------------------------------------------------------------------------------------------------ persist
@pytest.mark.parametrize("with_winner", [False, True], ids=["plain", "winner"])
@pytest.mark.parametrize("D", [4, 100, 172])
@pytest.mark.parametrize("B", [1, 3, 200])
def test_persist(B, D, with_winner):
    c = R.make_persist_case(B, D)
    n = c["n_nodes"]
    if B >= 3:
        named = np.unique(np.concatenate([c["src"], c["dst"]]))
        assert (c["has_msg"][named] == 0).any() and (c["slot"][named] < 0).any() and (c["src"] == c["dst"]).any()
    b = Bufs()
    mem0 = np.concatenate([c["memory"].reshape(-1), canary(TAIL)])
    lu0 = np.concatenate([c["last_update"], canary(TAIL)])
    win0 = np.concatenate([c["winner"], np.full(TAIL, ISENT, np.int32)])
    p_mem, mem = b.out(mem0)
    p_lu, lu = b.out(lu0)
    p_win, win = b.out(win0)
    call("pfo_debug_persist", b.put(c["src"]), b.put(c["dst"]), B, b.put(c["slot"]), b.put(c["upd_mem"]), b.put(c["has_msg"]), b.put(c["msg_time"]),
         p_mem, p_lu, D, p_win if with_winner else None)
    e_mem, e_lu, e_win = R.persist(c["src"], c["dst"], c["slot"], c["upd_mem"], c["has_msg"], c["msg_time"], c["memory"], c["last_update"],
                                   c["winner"] if with_winner else None)
    mem, lu, win = mem.cpu().numpy(), lu.cpu().numpy(), win.cpu().numpy()
    assert same_bits(mem[:n * D], e_mem) and same_bits(mem[n * D:], mem0[n * D:]), "memory"
    assert same_bits(lu[:n], e_lu) and same_bits(lu[n:], lu0[n:]), "last_update"
    assert np.array_equal(win[:n], e_win if with_winner else c["winner"]) and np.all(win[n:] == ISENT), "winner table"


# ------------------------------------------------------------------------------------------------ message store
MSG_CASES = R.msg_cases()


@pytest.mark.parametrize("cid,kw,path", MSG_CASES, ids=[c[0] for c in MSG_CASES])
def test_msg_store(cid, kw, path):
    c = R.make_msg_case(**kw)
    B, D, Ef, n = c["B"], c["D"], c["Ef"], c["n_nodes"]
    M, C_ = 3 * D + Ef, 2 * D + Ef
    needs = _lib.load().pfo_debug_msg_store_needs_winner(B)
    assert needs == (1 if path == "winner" else 0)
    PATHS_SEEN.add("msg_store " + path)
    if kw["ts_kind"] == "real":
        assert np.any(c["ts"].astype(f32).astype(f64) != c["ts"])       # f32(ts) matters
    e_tab, e_mt, e_has, named = R.msg_store(c)
    ev = np.concatenate([c["src"], c["dst"]])
    for k, (first, last) in enumerate(kw.get("twice", ())):              # named by these two events alone, `step` steps of 64 apart
        assert np.flatnonzero(ev == n - len(kw["twice"]) + k).tolist() == [first, last]
        PATHS_SEEN.add("msg_store later event in step %d" % R.msg_scan_step(first, last))
    delta = e_mt[named] - c["last_update"][named]
    if B >= 65:
        assert (delta < 0).any() and (delta > 0).any()
    b = Bufs()
    tab0 = np.concatenate([c["msg_table"].reshape(-1), canary(TAIL)])
    mt0 = np.concatenate([c["msg_time"], canary(TAIL)])
    has0 = np.concatenate([c["has_msg"], np.full(TAIL, BSENT, np.uint8)])
    p_tab, tab = b.out(tab0)
    p_mt, mt = b.out(mt0)
    p_has, has = b.out(has0)
    p_win = b.put(c["winner"]) if B >= 8192 else None
    call("pfo_debug_msg_store", b.put(c["src"]), b.put(c["dst"]), b.put(c["ts"], f64), b.put(c["eidx"]), B, b.put(c["memory"]), b.put(c["last_update"]),
         b.put(c["edge_feat"]) if Ef else None, b.put(c["tw"]), b.put(c["tb"]), D, Ef, p_tab, p_mt, p_has, p_win)
    tab, mt, has = tab.cpu().numpy(), mt.cpu().numpy(), has.cpu().numpy()
    assert same_bits(tab[n * M:], tab0[n * M:]) and same_bits(mt[n:], mt0[n:]) and np.all(has[n:] == BSENT), "tail"
    tab = tab[:n * M].reshape(n, M)
    assert same_bits(tab[~named], c["msg_table"][~named]) and same_bits(mt[:n][~named], c["msg_time"][~named]), "a node nobody names was written"
    assert np.array_equal(has[:n], e_has), "has_msg"
    assert same_bits(mt[:n][named], e_mt[named]), "msg_time is not f32(ts) of the last event"
    assert same_bits(tab[named][:, :C_], e_tab[named][:, :C_].astype(f32)), "a copied block differs"
    err = float(np.abs(tab[named][:, C_:].astype(f64) - e_tab[named][:, C_:]).max())
    note("msg_store cosine (error / 5e-7)", err / R.COS_BAR, cid)
    assert err < R.COS_BAR, err


# ------------------------------------------------------------------------------------------------ observe-select
@pytest.mark.parametrize("B", R.OBSERVE_BATCHES)
def test_observe_select(B):
    c = R.make_observe_case(B)
    n = c["n_nodes"]
    b = Bufs()
    p_rep, rep = b.out(np.concatenate([np.zeros(n, np.int32), np.full(TAIL, ISENT, np.int32)]))
    p_slot, slot = b.out(np.concatenate([np.full(n, -1, np.int32), np.full(TAIL, ISENT, np.int32)]))
    e_rep, e_slot = np.zeros(n, np.int32), np.full(n, -1, np.int32)
    counts = []
    for k, (src, dst, has) in enumerate(c["batches"]):
        p_t, touched = b.out(np.full(2 * B + TAIL, ISENT, np.int32))
        p_n, n_out = b.out(np.full(1 + TAIL, ISENT, np.int32))
        call("pfo_debug_observe_select", b.put(src), b.put(dst), B, b.put(has), p_rep, 2 * B * k, p_slot, p_t, p_n)
        e_t, e_slot, e_rep = R.observe_select(src, dst, has, e_rep, 2 * B * k, e_slot)
        touched, n_out = touched.cpu().numpy(), n_out.cpu().numpy()
        assert n_out[0] == len(e_t) and np.all(n_out[1:] == ISENT), (k, n_out[0], len(e_t))
        assert np.array_equal(touched[:len(e_t)], e_t) and np.all(touched[len(e_t):] == ISENT), (k, "touched")
        assert np.array_equal(slot.cpu().numpy()[:n], e_slot) and np.all(slot.cpu().numpy()[n:] == ISENT), (k, "slot")
        assert np.array_equal(rep.cpu().numpy()[:n], e_rep) and np.all(rep.cpu().numpy()[n:] == ISENT), (k, "stamps")
        counts.append(len(e_t))
    if B >= 3:
        assert min(counts) > 0 and len({tuple(x[2]) for x in c["batches"]}) >= (3 if B > 3 else 2)


# ------------------------------------------------------------------------------------------------ mean
@pytest.mark.parametrize("kind", ["losses", "signed"])
@pytest.mark.parametrize("n", R.MEAN_SIZES)
def test_mean(n, kind):
    rs = np.random.RandomState(n)
    x = rs.randn(n)
    x = (np.log1p(np.exp(-x)) if kind == "losses" else x * 10.0 ** rs.uniform(-2, 2, n)).astype(f32)
    b = Bufs()
    p, t = b.out(canary(1 + TAIL))
    call("pfo_debug_mean", b.put(x), n, p)
    got = t.cpu().numpy()
    want, mag = R.mean(x)
    assert same_bits(got[1:], canary(1 + TAIL)[1:]) and np.isfinite(got[0])
    ratio = abs(float(got[0]) - want) / (8 * 2.0 ** -23 * mag)
    note("mean", ratio, "n%d %s" % (n, kind))
    assert ratio <= 1.0, ratio


# ------------------------------------------------------------------------------------------------ folded query-bias backward
CQ_CASES = R.cq_cases()


@pytest.mark.parametrize("cid,kw", CQ_CASES, ids=[c[0] for c in CQ_CASES])
def test_cq_backward(cid, kw):
    c = R.make_cq_case(**kw)
    D, L, form = c["D"], c["L"], c["form"]
    E = 2 * D
    r64, mag = R.cq_backward(c, f64)
    r32, _ = R.cq_backward(c, f32)
    b = Bufs()
    arr = lambda ptrs: (C.c_void_p * 4)(*(ptrs + [None] * (4 - len(ptrs))))
    bq = [b.out(np.concatenate([c["d_bq"][l], canary(TAIL)])) for l in range(L)]
    wq = [b.out(np.concatenate([c["d_Wq"][l].reshape(-1), canary(TAIL)])) for l in range(L)]
    tb0, tw0, part0 = np.concatenate([c["d_tb"], canary(TAIL)]), np.concatenate([c["d_tw"], canary(TAIL)]), canary(D + TAIL)
    p_tb, d_tb = b.out(tb0)
    p_tw, d_tw = b.out(tw0)
    p_part, part = b.out(part0)
    nb = c["n_bins"]
    p_bins = b.put(c["dtime"], f64) if form == "bins" else None
    call("pfo_debug_cq_backward", arr([b.put(c["gq"][l]) for l in range(L)]), arr([b.put(c["Wq"][l]) for l in range(L)]), L, b.put(c["tb"]), D,
         arr([p for p, _ in bq]), arr([p for p, _ in wq]), p_tb, p_part if form == "part" else None, b.put(c["tb_add"]), p_bins, nb,
         p_tw if form == "bins" else None)
    for l in range(L):
        g_bq, g_wq = bq[l][1].cpu().numpy(), wq[l][1].cpu().numpy()
        assert same_bits(g_bq[E:], canary(TAIL)) and same_bits(g_wq[E * E:], canary(TAIL)), "tail"
        g_wq = g_wq[:E * E].reshape(E, E)
        assert same_bits(g_wq[:, :D], c["d_Wq"][l][:, :D]), "columns [0, D) of d_Wq were written"
        hold("cq_backward", cid + " d_bq", g_bq[:E], r32["d_bq"][l], r64["d_bq"][l], mag["d_bq"][l])
        hold("cq_backward", cid + " d_Wq", g_wq[:, D:], r32["d_Wq"][l][:, D:], r64["d_Wq"][l][:, D:], mag["d_Wq"][l][:, D:])
    d_tb, d_tw, part = d_tb.cpu().numpy(), d_tw.cpu().numpy(), part.cpu().numpy()
    assert same_bits(d_tb[D:], tb0[D:]) and same_bits(d_tw[D:], tw0[D:]) and same_bits(part[D:], part0[D:]), "tail"
    if form == "part":
        assert same_bits(d_tb, tb0), "a partial launch stores its term: d_tb is not its to touch"
        hold("cq_backward", cid + " tb_part", part[:D], r32["tb_part"], r64["tb_part"], mag["tb_part"])
    else:
        assert same_bits(part, part0)
        hold("cq_backward", cid + " d_tb", d_tb[:D], r32["d_tb"], r64["d_tb"], mag["d_tb"])
    if form == "bins":
        hold("cq_backward", cid + " d_tw", d_tw[:D], r32["d_tw"], r64["d_tw"], mag["d_tw"])
    else:
        assert same_bits(d_tw, tw0)


# ------------------------------------------------------------------------------------------------ part fold
@pytest.mark.parametrize("n_parts", R.FOLD_PARTS)
@pytest.mark.parametrize("n", R.FOLD_COLS)
def test_fold_parts(n, n_parts):
    c = R.make_fold_case(n, n_parts)
    case = "n%d parts%d" % (n, n_parts)
    deep = _lib.load().pfo_debug_fold_parts_rows_in_flight(n_parts)
    assert deep == (8 if n_parts >= R.FOLD_DEEP_FROM else 1)
    PATHS_SEEN.add("fold rows in flight %d" % deep)
    b = Bufs()
    p_parts = b.put(c["parts"], f64)
    n_scr = int(_lib.byte_count("pfo_debug_fold_parts_scratch_doubles", n))
    p_scr, scr = b.out(canary64(n_scr + TAIL))
    p_tick, tick = b.out(np.concatenate([np.zeros(64, np.int32), np.full(TAIL, ISENT, np.int32)]))

    def launch(out32, acc, out64):
        call("pfo_debug_fold_parts", p_parts, n_parts, n, out32, acc, p_scr, n_scr, p_tick, out64)
        t = tick.cpu().numpy()
        assert not t[:64].any() and np.all(t[64:] == ISENT), "the tickets did not reset themselves"

    s, _, m64, _ = R.fold_parts(c["parts"])
    b64, b32 = R.fold_bars(n_parts, m64, m64)
    # 1: the fp64 sums; `out` is not touched
    p64, o64 = b.out(canary64(n + TAIL))
    p32, o32 = b.out(canary(n + TAIL))
    launch(p32, 0, p64)
    g64 = o64.cpu().numpy()
    assert same_bits(g64[n:], canary64(n + TAIL)[n:]) and same_bits(o32.cpu().numpy(), canary(n + TAIL)) and np.isfinite(g64[:n]).all()
    r = R.worst_ratio(g64[:n], s, b64)
    note("fold_parts out64", r, case)
    assert r <= 1.0, r
    # 2: the same ticket array, not cleared: plain fp32 output
    launch(p32, 0, None)
    g32 = o32.cpu().numpy()
    assert same_bits(g32[n:], canary(n + TAIL)[n:]) and np.isfinite(g32[:n]).all()
    r = R.worst_ratio(g32[:n], s, b32)
    note("fold_parts out", r, case)
    assert r <= 1.0, r
    assert same_bits(g32[:n], g64[:n].astype(f32)), "the fp32 output is not the rounded fp64 sum"
    # 3: accumulating onto a non-zero output
    pa, oa = b.out(np.concatenate([c["out0"], canary(TAIL)]))
    launch(pa, 1, None)
    ga = oa.cpu().numpy()
    _, e_acc, _, m_acc = R.fold_parts(c["parts"], c["out0"], 1)
    _, b_acc = R.fold_bars(n_parts, m64, m_acc)
    assert same_bits(ga[n:], canary(TAIL))
    r = R.worst_ratio(ga[:n], e_acc, b_acc)
    note("fold_parts out accumulating", r, case)
    assert r <= 1.0, r
    # 4: the same input again: the same bits
    q64, r64 = b.out(canary64(n + TAIL))
    launch(None, 0, q64)
    assert same_bits(r64.cpu().numpy(), g64), "two folds of the same parts differ"
    assert same_bits(scr.cpu().numpy()[n_scr:], canary64(n_scr + TAIL)[n_scr:]), "scratch tail"


def test_fold_parts_refuses_more_columns_than_tickets():
    n = 4097
    b = Bufs()
    n_scr = 32 * n
    p_scr, scr = b.out(canary64(n_scr))
    p_out, out = b.out(canary(n))
    p_tick, tick = b.out(np.zeros(64 + TAIL, np.int32))
    rc = _lib.load().pfo_debug_fold_parts(b.put(np.ones((2, n)), f64), 2, n, p_out, 0, p_scr, n_scr, p_tick, None, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1 and b"too many columns" in _lib.load().pfo_last_error()
    assert same_bits(out.cpu().numpy(), canary(n)) and same_bits(scr.cpu().numpy(), canary64(n_scr)) and not tick.cpu().numpy().any()


def test_zz_every_path_was_reached_and_figures():
    """Runs last in the file: the paths the cases above reached (when the whole file ran) and the FIGURES line."""
    print("FIGURES " + "; ".join("%s %.3f (%s)" % (k, v[0], v[1]) for k, v in sorted(FIGURES.items())))
    print("PATHS " + "; ".join(sorted(PATHS_SEEN)))
    if len(FIGURES) >= 7:                                                # the whole file ran, not a selection
        want = {"compact lookback 0 strides", "compact lookback 1 strides", "compact lookback 2 strides",
                "msg_store later event in step 1", "msg_store later event in step 2", "msg_store later event in step 3", "msg_store later event in step 4", "scan sweeps 1", "scan sweeps 2", "gates float4", "gates scalar", "gates float4 det", "gates scalar det",
                "msg_store inline", "msg_store winner", "fold rows in flight 1", "fold rows in flight 8"}
        assert want <= PATHS_SEEN, sorted(want - PATHS_SEEN)
