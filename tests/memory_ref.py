"""The memory-side interface (pfotgnrec_amd/csrc/memory.hpp) stated on the host: one function per launcher, the case
generators and the case lists its CPU and GPU tests share (tests/test_memory_ref_cpu.py, tests/test_gpu_memory_forms.py).
Plain numpy, no import of the package.

The integer and copy launchers (compaction, pack / remap, zero rows, persist, observe-select, scan, the copied blocks of the
message store) are stated as the exact arrays they must leave, sequentially over the nodes or events - not as the parallel
algorithm.  The arithmetic ones (GRU gate backward, folded query-bias backward, part fold, mean) are stated in float64 with
the first-order magnitude ``mag`` of their own rounding noise beside every output (the expression with every operand
replaced by its absolute value, sum |terms| for a sum, one absolute unit per sine or cosine), and - where the bar needs
it - once more in float32 in the kernel's order of operations.  A bar is built from these alone (``bar``).

``mutant=``: a deliberately wrong model; tests/test_memory_ref_cpu.py shows each one missed by the bar (or differing exactly)
on the case lists below, i.e. that the cases can see it."""
import math

import numpy as np

from oracle import tgn_oracle as T

f32, f64 = np.float32, np.float64
MARGIN = 8.0
EPS_FLOOR = 2.0 ** -23
DET_SCALE = 2.0 ** 40
COS_BAR = 5e-7            # tests/test_gpu_kernels.py::test_time_encode_large_arguments_vs_float64
MSG_INLINE_MAX = 16384    # events up to which the message store finds its winners inline (memory.hip)

MUTANTS = {
    "gates": ["dz_n_minus_h", "dr_from_n", "dgh_n_without_r", "dgi_n_with_r", "no_d_extra", "last_replica_dropped", "det_scale_39"],
    "cq": ["sin_cos_swapped", "no_tb_add", "last_bin_dropped", "d_bq_every_workgroup"],
    "fold": ["rows_from_1024_dropped", "accumulate_ignored"],
    "msg": ["first_event_wins", "mem_swapped", "delta_from_other", "edge_of_event", "msg_time_truncated"],
    "compact": ["class2_overwrites", "class2_from_zero", "out_of_range_clipped"],
    "observe": ["first_event_representative", "stamps_without_base"],
}


def bar(ref32, ref64, mag):
    """Per element MARGIN * max(e32, 2^-23) * mag with e32 = max |ref32 - ref64| / mag over the output: reference side only."""
    r32, r64, mag = (np.asarray(a, f64).reshape(-1) for a in (ref32, ref64, mag))
    nz = mag > 0
    assert np.all(r32[~nz] == r64[~nz]), "the two references differ where no rounding can occur"
    e32 = float(np.max(np.abs(r32 - r64)[nz] / mag[nz])) if nz.any() else 0.0
    return MARGIN * max(e32, EPS_FLOOR) * mag, e32


def worst_ratio(got, ref64, b):
    """max |got - ref64| / bar (0 where both agree; inf where the bar is 0 and they differ)."""
    d = np.abs(np.asarray(got, f64).reshape(-1) - np.asarray(ref64, f64).reshape(-1))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0.0, d / np.asarray(b, f64).reshape(-1))
    return float(np.max(r)) if r.size else 0.0


# ------------------------------------------------------------------------------------------------ compaction
def compact(n_nodes, nodes0=None, extra=None, marks=None, mutant=None):
    """-> slot i32[n_nodes], touched i32[n_all], n_counts [all, class 1].  Class 1: the ascending distinct in-range ids of
    nodes0 (or the ids whose mark is 1); class 2: those of ``extra`` that are not class 1, slotted behind."""
    def ids_of(a):
        a = np.asarray(a, np.int64).reshape(-1)
        if mutant == "out_of_range_clipped":
            return np.unique(np.clip(a, 0, n_nodes - 1))
        return np.unique(a[(a >= 0) & (a < n_nodes)])
    c1 = np.flatnonzero(np.asarray(marks) == 1) if marks is not None else ids_of(nodes0)
    c2 = ids_of(extra) if extra is not None and len(extra) else np.zeros(0, np.int64)
    if mutant == "class2_overwrites":
        c1 = np.setdiff1d(c1, c2)
    else:
        c2 = np.setdiff1d(c2, c1)
    slot = np.full(n_nodes, -1, np.int32)
    touched = np.full(len(c1) + len(c2), -1, np.int32)
    slot[c1] = np.arange(len(c1))
    touched[:len(c1)] = c1
    base = 0 if mutant == "class2_from_zero" else len(c1)
    slot[c2] = base + np.arange(len(c2))
    touched[base:base + len(c2)] = c2
    n_all = base + len(c2) if extra is not None and len(extra) else len(c1)
    return slot, touched[:n_all], np.array([n_all, len(c1)], np.int32)


# (2^20 + 3: 1 025 workgroups, the last of which looks back over exactly 1 024 published counts - the whole first stride of
#  its loop; a second stride needs 1 026 workgroups, from 1 025 * 1 024 + 1 nodes on: the last size.  There workgroup 1 024,
#  the one the second stride reads, holds a node of either class: make_compact_case names COMPACT_FAR_IDS)
COMPACT_SIZES = [1, 63, 1023, 1024, 1025, 5000, (1 << 20) + 3, 1025 * 1024 + 3]
COMPACT_FAR_IDS = (1024 * 1024 + 1, 1024 * 1024 + 2)      # class 1, class 2 only


def compact_lookback_strides(n_nodes):
    """Strides of 1 024 published counts the LAST workgroup of the one-pass compaction walks (block b reads b counts)."""
    nb = (n_nodes + 1023) // 1024
    return (nb - 1 + 1023) // 1024


def make_compact_case(n_nodes, two, marked, empty1=False, seed=0):
    """nodes0 / extra with duplicates, ids < 0 and ids >= n_nodes; extra overlaps class 1; first and last node named."""
    rs = np.random.RandomState(seed + n_nodes % 9973)
    k = max(4, min(n_nodes, 6000) // 2)
    nodes0 = np.concatenate([rs.randint(-2, n_nodes + 2, k), [0, n_nodes - 1, -1, n_nodes, n_nodes + 7]]).astype(np.int32)
    far = compact_lookback_strides(n_nodes) >= 2
    if far:
        nodes0 = np.concatenate([nodes0[nodes0 != COMPACT_FAR_IDS[1]], [COMPACT_FAR_IDS[0]]]).astype(np.int32)
    if empty1:
        nodes0 = np.array([-1, n_nodes, n_nodes + 3, -5], np.int32)
    c = dict(n_nodes=n_nodes, nodes0=nodes0, extra=None, marks=None, marked=marked)
    if two:
        ex = rs.randint(-3, n_nodes + 3, max(3, k // 2))
        c["extra"] = np.concatenate([ex, ex[:5], nodes0[:7], [n_nodes - 1, 0, -1, n_nodes, 2 ** 31 - 1], [COMPACT_FAR_IDS[1]] if far else []]).astype(np.int32)
    if marked:
        m = np.zeros(n_nodes, np.int32)
        v = nodes0[(nodes0 >= 0) & (nodes0 < n_nodes)]
        m[v] = 1
        c["marks"] = m
    return c


def compact_cases():
    out = []
    for n in COMPACT_SIZES:
        for two in (False, True):
            for marked in (False, True):
                out.append(("n%d-%s-%s" % (n, "two" if two else "one", "marked" if marked else "listed"), dict(n_nodes=n, two=two, marked=marked)))
    for n in (63, 5000):
        for marked in (False, True):
            out.append(("n%d-empty1-two-%s" % (n, "marked" if marked else "listed"), dict(n_nodes=n, two=True, marked=marked, empty1=True)))
    return out


def compact_of_case(c, mutant=None):
    return compact(c["n_nodes"], c["nodes0"], c["extra"], c["marks"] if c["marked"] else None, mutant)


# ------------------------------------------------------------------------------------------------ copies
def iscan(counts):
    c = np.asarray(counts, np.int64)
    return (np.cumsum(c) - c).astype(np.int32)


ISCAN_SIZES = [1, 1023, 1024, 1025, 1 << 20, (1 << 20) + 1, (1 << 20) + 1025]


def pack_remap(msg_table, memory, has_msg, touched, n_touched, nodes0, slot):
    """-> msg_rows [n_touched, M] (None without a message table), h_rows [n_touched, D], hm [n_touched], idx0 [n0]."""
    ids = np.asarray(touched, np.int64)[:n_touched]
    rows = None if msg_table is None else np.asarray(msg_table)[ids]
    hm = None if msg_table is None else np.asarray(has_msg)[ids]
    return rows, np.asarray(memory)[ids], hm, np.asarray(slot)[np.asarray(nodes0, np.int64)]


def zero_rows(dst, n_rows, D, n_rep, rep_stride):
    out = np.array(dst, copy=True).reshape(-1)
    for q in range(n_rep):
        out[q * rep_stride:q * rep_stride + n_rows * D] = 0
    return out


def persist(src, dst, slot, upd_mem, has_msg, msg_time, memory, last_update, winner=None):
    """Acts only where has_msg[id] and slot[id] >= 0; with a winner table every named node's entry is -1 afterwards."""
    memory, last_update = np.array(memory, copy=True), np.array(last_update, copy=True)
    winner = None if winner is None else np.array(winner, copy=True)
    for X in np.concatenate([src, dst]):
        if winner is not None:
            winner[X] = -1
        if has_msg[X] and slot[X] >= 0:
            memory[X] = upd_mem[slot[X]]
            last_update[X] = msg_time[X]
    return memory, last_update, winner


def make_persist_case(B, D, seed=0):
    """Nodes named twice and on both sides, a self-loop, nodes without a message, nodes with slot -1."""
    rs = np.random.RandomState(seed + 31 * B + D)
    n_nodes = max(6, B // 2 + 3)
    src, dst = rs.randint(1, n_nodes, B).astype(np.int32), rs.randint(1, n_nodes, B).astype(np.int32)
    if B >= 3:
        src[0], dst[0] = 2, 2                                           # self-loop
        src[1], dst[2] = 3, 3                                           # both sides
        src[2] = src[1]                                                 # twice on one side
        dst[1] = 4
    has = (rs.rand(n_nodes) < 0.7).astype(np.uint8)
    slot = np.full(n_nodes, -1, np.int32)
    named = np.unique(np.concatenate([src, dst]))
    keep = named[rs.rand(len(named)) < 0.8] if B > 1 else named
    if B >= 3:                                                          # 2: a message and no slot; 3: a slot and no message; 4: both
        has[2], has[3], has[4] = 1, 0, 1
        keep = np.union1d(keep[keep != 2], [3, 4])
    slot[keep] = rs.permutation(len(keep))
    cap = len(keep) + 2
    return dict(B=B, D=D, n_nodes=n_nodes, src=src, dst=dst, slot=slot, has_msg=has, cap=cap,
                upd_mem=rs.randn(cap, D).astype(f32), msg_time=rs.rand(n_nodes).astype(f32) * 100,
                memory=rs.randn(n_nodes, D).astype(f32), last_update=rs.rand(n_nodes).astype(f32) * 50,
                winner=rs.randint(0, 2 * B, n_nodes).astype(np.int32))


# ------------------------------------------------------------------------------------------------ message store
def time_grid(D):
    return (1 / 10 ** np.linspace(0, 9, D)).astype(f32)


def msg_store(c, mutant=None):
    """Event e = side * B + i, the last event naming a node wins:
         row[X] = [ mem[X] | mem[O] | edge_feat[eidx[i]] | cos(fma(f32(ts[i]) - last_update[X], w, b)) ]
       msg_time[X] = f32(ts[i]), has_msg[X] = 1; rows of nodes nobody names are untouched.
    -> table f64 [n_nodes, M] (the copied blocks hold fp32 values exactly, the cosine block cos(float64(arg))), msg_time f32,
    has_msg u8, named bool[n_nodes]."""
    B, D, Ef = c["B"], c["D"], c["Ef"]
    src, dst, ts, eidx = c["src"], c["dst"], c["ts"], c["eidx"]
    mem, lu, ef = c["memory"], c["last_update"], c["edge_feat"]
    tab = np.array(c["msg_table"], f64)
    mt, has = np.array(c["msg_time"], copy=True), np.array(c["has_msg"], copy=True)
    last = {}
    for e in range(2 * B):
        X = int(src[e] if e < B else dst[e - B])
        if mutant == "first_event_wins" and X in last:
            continue
        last[X] = e
    named = np.zeros(len(mt), bool)
    for X, e in last.items():
        i = e % B
        O = int(dst[i] if e < B else src[i])
        t = f32(ts[i])
        if mutant == "msg_time_truncated":
            t = f32(np.nextafter(t, f32(0))) if abs(float(t)) > abs(float(ts[i])) else t
        delta = f32(t - lu[O if mutant == "delta_from_other" else X])
        a, b = (O, X) if mutant == "mem_swapped" else (X, O)
        tab[X, :D], tab[X, D:2 * D] = mem[a], mem[b]
        if Ef:
            tab[X, 2 * D:2 * D + Ef] = ef[e % len(ef)] if mutant == "edge_of_event" else ef[eidx[i]]
        tab[X, 2 * D + Ef:] = np.cos(T.fmaf(delta, c["tw"], c["tb"]).astype(f64))
        mt[X], has[X], named[X] = t, 1, True
    return tab, mt, has, named


MSG_SHAPES = [(4, 0), (8, 4), (100, 64), (172, 4)]
MSG_BATCHES = [1, 2, 65, 300]
MSG_TS_KINDS = ["small", "real"]
# Pairs of events (first, last) of B = 300, each pair naming a node of its own that nothing else names: the first event has
# to find the one later event in step (last - first - 1) // 64 of its scan of 64 ids per step - steps 1, 2, 3 and 4 here,
# within one side and across the two.  (With 7 nodes named hundreds of times some later event turns up in every step.)
MSG_TWICE = [(10, 110), (20, 170), (250, 470), (30, 331)]


def msg_scan_step(first, last):
    return (last - first - 1) // 64


def make_msg_case(D, Ef, B, n_nodes=7, ts_kind="small", seed=0, twice=()):
    """Few nodes, so nearly every node is named many times; a node that is source of one event and destination of a later
    one, and a self-loop; last_update both below and above ts.  twice: pairs of events that name one further node each."""
    rs = np.random.RandomState(seed + 7 * D + B)
    M = 3 * D + Ef
    src, dst = rs.randint(1, n_nodes, B).astype(np.int32), rs.randint(1, n_nodes, B).astype(np.int32)
    for k, pair in enumerate(twice):
        for e in pair:
            (src if e < B else dst)[e % B] = n_nodes + k
    n_nodes += len(twice)
    if B >= 2:
        src[0], dst[B - 1] = 3, 3                                       # source of the first event, destination of the last
        dst[0] = src[0] if B == 2 else dst[0]
    if B >= 3:
        src[1] = dst[1] = 4                                             # self-loop
    n_edges = max(B, 8) + 5
    eidx = rs.permutation(n_edges)[:B].astype(np.int32)
    if ts_kind == "small":
        ts = np.sort(rs.randint(0, 200, B)).astype(f64)
        lu = rs.randint(0, 400, n_nodes).astype(f32)
    else:                                                               # yyyymmddHHMMSS (2^44 .. 2^45): f32(ts) rounds to multiples of 2^21
        ts = np.sort(20240101000000 + rs.randint(0, 1 << 26, B).astype(f64) * 1.0 + rs.randint(0, 1 << 20, B))
        lu = f32(20240101000000 + rs.randint(0, 1 << 27, n_nodes).astype(f64))
    has = (rs.rand(n_nodes) < 0.5).astype(np.uint8)
    return dict(B=B, D=D, Ef=Ef, n_nodes=n_nodes, src=src, dst=dst, ts=ts, eidx=eidx,
                memory=rs.randn(n_nodes, D).astype(f32), last_update=lu.astype(f32),
                edge_feat=rs.randn(n_edges, Ef).astype(f32) if Ef else np.zeros((n_edges, 0), f32),
                tw=time_grid(D), tb=rs.randn(D).astype(f32),
                msg_table=(rs.randn(n_nodes, M) * has[:, None]).astype(f32), msg_time=(rs.rand(n_nodes) * 50 * has).astype(f32),
                has_msg=has, winner=np.full(n_nodes, -1, np.int32))


def msg_cases():
    out = []
    for D, Ef in MSG_SHAPES:
        for B in MSG_BATCHES:
            for kind in MSG_TS_KINDS:
                out.append(("D%d-Ef%d-B%d-%s" % (D, Ef, B, kind), dict(D=D, Ef=Ef, B=B, ts_kind=kind), "inline"))
    for i, (D, Ef) in enumerate(MSG_SHAPES):
        out.append(("D%d-Ef%d-B300-twice" % (D, Ef), dict(D=D, Ef=Ef, B=300, ts_kind=MSG_TS_KINDS[i % 2], twice=MSG_TWICE), "inline"))
    for B, path in ((8200, "winner"), (8192, "inline")):
        for D, Ef in MSG_SHAPES[:2]:
            out.append(("D%d-Ef%d-B%d" % (D, Ef, B), dict(D=D, Ef=Ef, B=B, n_nodes=50, ts_kind="real" if D == 4 else "small"), path))
    return out


def msg_store_needs_winner(B):
    return 2 * B > MSG_INLINE_MAX


# ------------------------------------------------------------------------------------------------ observe-select
def observe_select(src, dst, has_msg, rep, base, slot, mutant=None):
    """touched = the distinct positives of [src | dst] that hold a message, in the order of each node's LAST event; slot[X] its
    position.  rep[X] ends as the largest stamp base + e + 1 of the events that name X (never below what it held).
    -> touched, slot (copy), rep (copy)."""
    B = len(src)
    ev = np.concatenate([src, dst]).astype(np.int64)
    slot, rep = np.array(slot, copy=True), np.array(rep, copy=True)
    if mutant == "stamps_without_base":
        base = 0
    for e, X in enumerate(ev):
        rep[X] = max(rep[X], base + e + 1)
    order = {}
    for e, X in enumerate(ev):
        if mutant == "first_event_representative":
            order.setdefault(int(X), e)
        else:
            order[int(X)] = e
    if mutant == "stamps_without_base":                                 # a stale stamp of an earlier batch hides the node
        order = {X: e for X, e in order.items() if rep[X] == e + 1}
    touched = [X for X, e in sorted(order.items(), key=lambda kv: kv[1]) if has_msg[X]]
    for p, X in enumerate(touched):
        slot[X] = p
    return np.array(touched, np.int32), slot, rep


OBSERVE_BATCHES = [1, 3, 511, 512, 513, 1500]


def make_observe_case(B, seed=0):
    """Three batches over one node set (they share nodes); has_msg changes between them."""
    rs = np.random.RandomState(seed + B)
    n_nodes = max(5, B // 2 + 2)
    batches = []
    for k in range(3):
        src, dst = rs.randint(1, n_nodes, B).astype(np.int32), rs.randint(1, n_nodes, B).astype(np.int32)
        if B >= 3:
            src[0] = dst[0] = 1 + k                                     # self-loop
            dst[B - 1] = src[1]
        has = (rs.rand(n_nodes) < 0.6).astype(np.uint8)
        has[src[0]] = 1
        batches.append((src, dst, has))
    return dict(B=B, n_nodes=n_nodes, batches=batches)


# ------------------------------------------------------------------------------------------------ GRU gate backward
def gru_gates_bwd(c, dtype=f64, mutant=None):
    """torch.nn.GRUCell backward from d h' to the two pre-activation blocks, gates[s] = r | z | n | gh_n, in the kernel's
    order of operations:
        dh = sum_q d_h0[q] (+ d_extra)        det: dh = f32(f64(table) * 2^-40) (+ d_extra)
        dn = dh (1 - z);  dz = dh (h - n);  dn' = dn (1 - n n);  dr = dn' gh_n;  dr' = dr r (1 - r);  dz' = dz z (1 - z)
        d gi = dr' | dz' | dn'          d gh = dr' | dz' | dn' r         zeros where hm = 0
    -> dgi, dgh [rows, 3D] in ``dtype`` and their magnitudes (float64)."""
    rows, D = c["rows"], c["D"]
    g = np.asarray(c["gates"])[:rows].reshape(rows, 4, D)                  # (fp32 on the device; float64 in the autograd check)
    r, z, n, ghn = (g[:, k].astype(dtype) for k in range(4))
    h = np.asarray(c["h_rows"])[:rows].astype(dtype)
    one = dtype(1)
    if c["det"]:
        scale = 2.0 ** -39 if mutant == "det_scale_39" else 2.0 ** -40
        t = np.asarray(c["d_h0"], np.int64)[:rows].astype(f64) * scale
        dh = t.astype(f32).astype(dtype) if dtype == f32 else t
        adh = np.abs(t)
    else:
        reps = np.asarray(c["d_h0"])[:, :rows]
        if mutant == "last_replica_dropped":
            reps = reps[:-1]
        dh = np.zeros((rows, D), dtype)
        for q in range(reps.shape[0]):
            dh = (dh + reps[q].astype(dtype)).astype(dtype)
        adh = np.abs(reps.astype(f64)).sum(axis=0)
    if c["d_extra"] is not None and mutant != "no_d_extra":
        dh = (dh + np.asarray(c["d_extra"])[:rows].astype(dtype)).astype(dtype)
        adh = adh + np.abs(np.asarray(c["d_extra"], f64)[:rows])
    dn = dh * (one - z)
    dz = dh * ((n - h) if mutant == "dz_n_minus_h" else (h - n))
    dpn = dn * (one - n * n)
    dr = dpn * (n if mutant == "dr_from_n" else ghn)
    dpr = dr * r * (one - r)
    dpz = dz * z * (one - z)
    dpnr = dpn * r
    ar, az, an, ag, ah = (np.abs(x.astype(f64)) for x in (r, z, n, ghn, h))
    m_dn = adh * (1 + az)
    m_dz = adh * (ah + an)
    m_dpn = m_dn * (1 + an * an)
    m_dr = m_dpn * ag
    m_dpr = m_dr * ar * (1 + ar)
    m_dpz = m_dz * az * (1 + az)
    m_dpnr = m_dpn * ar
    live = (np.asarray(c["hm"])[:rows] != 0)[:, None]
    gi_n, gh_n = (dpnr if mutant == "dgi_n_with_r" else dpn), (dpn if mutant == "dgh_n_without_r" else dpnr)
    dgi = np.where(live, np.concatenate([dpr, dpz, gi_n], axis=1), 0).astype(dtype)
    dgh = np.where(live, np.concatenate([dpr, dpz, gh_n], axis=1), 0).astype(dtype)
    m_gi = np.where(live, np.concatenate([m_dpr, m_dpz, m_dpn], axis=1), 0.0)
    m_gh = np.where(live, np.concatenate([m_dpr, m_dpz, m_dpnr], axis=1), 0.0)
    return dict(dgi=dgi, dgh=dgh), dict(dgi=m_gi, dgh=m_gh)


GATE_DIMS = [4, 8, 100, 172]
GATE_ROWS = [1, 3, 70]
GATE_REPS = [1, 2, 8]


def make_gates_case(D, rows, n_rep, det, extra, hm="mixed", seed=0):
    """Gates as sigmoid / tanh of N(0, 3): r and z come near 0 and 1, n near +-1.  det: the int64 table holds float64 values
    rounded to 2^-40, magnitudes from 1e-9 to 1e3."""
    rs = np.random.RandomState(seed + 13 * D + rows + 5 * n_rep + det)
    cap = rows + 3
    x = rs.randn(cap, 4, D) * 3
    gates = np.concatenate([1 / (1 + np.exp(-x[:, :2])), np.tanh(x[:, 2:3]), x[:, 3:4] / 3], axis=1).astype(f32).reshape(cap, 4 * D)
    if det:
        v = rs.randn(cap, D) * 10.0 ** rs.uniform(-9, 3, (cap, D))
        d_h0 = np.rint(v * DET_SCALE).astype(np.int64)
        n_rep = 1
    else:
        d_h0 = rs.randn(n_rep, cap, D).astype(f32)
    m = {"mixed": (rs.rand(cap) < 0.6), "zeros": np.zeros(cap, bool), "ones": np.ones(cap, bool)}[hm].astype(np.uint8)
    if hm == "mixed":
        m[0] = 1
        if rows >= 3:
            m[1] = 0
    return dict(D=D, rows=rows, cap=cap, n_rep=n_rep, det=det, gates=gates, h_rows=rs.randn(cap, D).astype(f32), hm=m, d_h0=d_h0,
                d_extra=rs.randn(cap, D).astype(f32) if extra else None)


def gates_cases():
    """(id, make_gates_case arguments): every D x rows, replicas / d_extra / hm / det spread over them, each combination of
    (det, d_extra) and every n_rep and hm kind at every D."""
    out = []
    i = 0
    for D in GATE_DIMS:
        for rows in GATE_ROWS:
            for det in (0, 1):
                for extra in (True, False):
                    n_rep = 1 if det else GATE_REPS[i % 3]
                    hm = ("mixed", "ones", "mixed", "zeros")[i % 4] if rows != 70 else "mixed"
                    out.append(("D%d-r%d-rep%d-%s-%s-%s" % (D, rows, n_rep, "det" if det else "f32", "extra" if extra else "noextra", hm),
                                dict(D=D, rows=rows, n_rep=n_rep, det=det, extra=extra, hm=hm)))
                    i += 1
        for n_rep in GATE_REPS:
            out.append(("D%d-r3-rep%d-f32-extra-mixed-b" % (D, n_rep), dict(D=D, rows=3, n_rep=n_rep, det=0, extra=True, hm="mixed", seed=1)))
        for hm in ("zeros", "ones"):
            out.append(("D%d-r3-rep2-f32-extra-%s" % (D, hm), dict(D=D, rows=3, n_rep=2, det=0, extra=True, hm=hm, seed=2)))
    return out


def gates_grid(D, rows):
    """Every combination of replicas, d_extra, hm and det at one (D, rows): what the device test walks."""
    for det in (0, 1):
        for n_rep in ([1] if det else GATE_REPS):
            for extra in (True, False):
                for hm in ("mixed", "zeros", "ones"):
                    yield dict(D=D, rows=rows, n_rep=n_rep, det=det, extra=extra, hm=hm)


# ------------------------------------------------------------------------------------------------ folded query-bias backward
def cq_backward(c, dtype=f64, mutant=None):
    """cq = Wq[:, D:] cos(tb) + bq, with gq = d cq per layer (E = 2 D):
        d bq += gq;  d Wq[:, D + d] += gq cos(tb_d);  term_d = -sin(tb_d) sum_l sum_e Wq_l[e, D + d] gq_l[e]
    form 'part': tb_part = term (stored), d_tb untouched; 'final': d_tb += term + tb_add; 'bins': additionally
    d_tw = f32(f64(d_tw) + sum_bins dtime[:, :D]), d_tb = f32(f64(d_tb) + sum_bins dtime[:, D:]) first (the device sums the
    bins in fp64: math.fsum here).
    -> outputs dict(d_bq [L, E], d_Wq [L, E, E], d_tb [D] or tb_part [D], d_tw [D]) and magnitudes."""
    D, L, form = c["D"], c["L"], c["form"]
    E = 2 * D
    tb = np.asarray(c["tb"], f32).astype(dtype)
    sb, cb = np.sin(tb), np.cos(tb)
    if mutant == "sin_cos_swapped":
        sb, cb = cb, sb
    gq, Wq = np.asarray(c["gq"], f32).astype(dtype), np.asarray(c["Wq"], f32).astype(dtype)
    d_bq = (np.asarray(c["d_bq"], f32).astype(dtype) + gq * (D if mutant == "d_bq_every_workgroup" else 1)).astype(dtype)
    m_bq = np.abs(np.asarray(c["d_bq"], f64)) + np.abs(gq.astype(f64))
    d_Wq = np.asarray(c["d_Wq"], f32).astype(dtype).copy()
    m_Wq = np.zeros((L, E, E))
    d_Wq[:, :, D:] = (d_Wq[:, :, D:] + gq[:, :, None] * cb[None, None, :]).astype(dtype)
    m_Wq[:, :, D:] = np.abs(np.asarray(c["d_Wq"], f64))[:, :, D:] + np.abs(gq.astype(f64))[:, :, None] * (np.abs(cb.astype(f64)) + 1)[None, None, :]
    total = np.zeros(D, dtype)
    m_total = np.zeros(D)
    for l in range(L):
        total = (total + np.sum(Wq[l][:, D:] * gq[l][:, None], axis=0, dtype=dtype)).astype(dtype)
        m_total += np.abs(Wq[l][:, D:].astype(f64) * gq[l][:, None].astype(f64)).sum(axis=0)
    mine = (-sb * total).astype(dtype)
    m_mine = (np.abs(sb.astype(f64)) + 1) * m_total
    out, mag = dict(d_bq=d_bq, d_Wq=d_Wq), dict(d_bq=m_bq, d_Wq=m_Wq)
    if form == "part":
        out["tb_part"], mag["tb_part"] = mine, m_mine
        return out, mag
    d_tb = np.asarray(c["d_tb"], f32).astype(dtype)
    m_tb = np.abs(np.asarray(c["d_tb"], f64))
    if form == "bins":
        bins = np.asarray(c["dtime"], f64)[:c["n_bins"]]
        if mutant == "last_bin_dropped" and c["n_bins"] % 4:
            bins = bins[:-1]
        fold = np.array([math.fsum(bins[:, k].tolist()) for k in range(2 * D)])
        m_fold = np.abs(bins).sum(axis=0)
        d_tw = np.asarray(c["d_tw"], f64) + fold[:D]
        d_tb = d_tb.astype(f64) + fold[D:]
        if dtype == f32:
            d_tw, d_tb = d_tw.astype(f32), d_tb.astype(f32)
        out["d_tw"], mag["d_tw"] = d_tw, np.abs(np.asarray(c["d_tw"], f64)) + m_fold[:D]
        m_tb = m_tb + m_fold[D:]
    add = np.zeros(D, dtype) if (c["tb_add"] is None or mutant == "no_tb_add") else np.asarray(c["tb_add"]).astype(dtype)
    out["d_tb"] = (d_tb + (mine + add).astype(dtype)).astype(dtype)
    mag["d_tb"] = m_tb + m_mine + (0 if c["tb_add"] is None else np.abs(np.asarray(c["tb_add"], f64)))
    return out, mag


CQ_DIMS = [4, 100, 172]
CQ_LAYERS = [1, 2, 4]
CQ_BINS = [1, 2, 3, 4, 5, 37]


def make_cq_case(D, L, form, n_bins=0, seed=0):
    rs = np.random.RandomState(seed + D + 7 * L + n_bins)
    E = 2 * D
    c = dict(D=D, L=L, form=form, n_bins=n_bins, tb=rs.randn(D).astype(f32) * 2, gq=rs.randn(L, E).astype(f32),
             Wq=rs.randn(L, E, E).astype(f32), d_bq=rs.randn(L, E).astype(f32), d_Wq=rs.randn(L, E, E).astype(f32),
             d_tb=rs.randn(D).astype(f32), d_tw=rs.randn(D).astype(f32), tb_add=None, dtime=None)
    if form != "part":
        c["tb_add"] = rs.randn(D).astype(f32) * 3
    if form == "bins":
        c["dtime"] = rs.randn(n_bins, 2 * D) * 10.0 ** rs.uniform(-3, 2, (n_bins, 1))
    return c


def cq_cases():
    out = []
    for i, D in enumerate(CQ_DIMS):
        for j, L in enumerate(CQ_LAYERS):
            out.append(("D%d-L%d-part" % (D, L), dict(D=D, L=L, form="part")))
            out.append(("D%d-L%d-final" % (D, L), dict(D=D, L=L, form="final")))
            for nb in CQ_BINS:
                out.append(("D%d-L%d-bins%d" % (D, L, nb), dict(D=D, L=L, form="bins", n_bins=nb)))
    return out


# ------------------------------------------------------------------------------------------------ part fold, mean
def fold_parts(parts, out0=None, accumulate=0, mutant=None):
    """out64[c] = sum_p parts[p][c] (the device sums in fp64: math.fsum here, magnitude sum |parts|);
    out[c] = f32(out0[c] + out64[c]) when accumulating, else f32(out64[c]).  -> out64, out (float64 values), m64, m_out."""
    P = np.asarray(parts, f64)
    if mutant == "rows_from_1024_dropped":
        P = P[:1024]
    s = np.array([math.fsum(col) for col in P.T.tolist()])
    m64 = np.abs(P).sum(axis=0)
    acc = accumulate and mutant != "accumulate_ignored" and out0 is not None
    o = s + (np.asarray(out0, f64) if acc else 0.0)
    return s, o, m64, m64 + (np.abs(np.asarray(out0, f64)) if acc else 0.0)


def fold_bars(n_parts, m64, m_out):
    """out64 within n_parts 2^-52 sum |parts|; out within 2^-23 mag on top of that."""
    b64 = n_parts * 2.0 ** -52 * m64
    return b64, b64 + 2.0 ** -23 * m_out


FOLD_COLS = [1, 64, 65, 344, 4096]
FOLD_PARTS = [1, 127, 128, 129, 1023, 1024, 1025, 2500]
FOLD_DEEP_FROM = 897      # part rows from which some thread of the fold keeps eight rows in flight (7 * 128 + 1)


def make_fold_case(n, n_parts, seed=0):
    rs = np.random.RandomState(seed + n + 3 * n_parts)
    parts = rs.randn(n_parts, n) * 10.0 ** rs.uniform(-2, 2, (n_parts, 1))
    return dict(n=n, n_parts=n_parts, parts=parts, out0=rs.randn(n).astype(f32) * 5)


def mean(x):
    x = np.asarray(x, f32).astype(f64)
    n = len(x)
    return math.fsum(x.tolist()) / n, float(np.abs(x).sum()) / n


MEAN_SIZES = [1, 63, 64, 65, 1000, 100000]
