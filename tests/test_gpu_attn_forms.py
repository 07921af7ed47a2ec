"""Every form of the internal attention interface (pfotgnrec_amd/csrc/attn.hpp), launched through the pfo_debug_attn_* probes
and held per element to the float64 statement of tests/attn_ref.py.

Each case
  * asserts ``pfo_debug_attn_form`` before it launches, so that a dispatch change cannot quietly turn one case into a copy
    of another,
  * gives every output a canary (quiet NaNs with the element's index as payload) and compares bit for bit wherever the
    kernel must not write: rows >= N, rows that are not live, plain-stored rows nobody owns, table rows nobody names,
  * ends every float operand in NaN slack, and keeps every index array in range over its whole allocation: a wrong case gives
    a wrong number, never a stray access.

Bars (DESIGN.md "Attention forms under test"): per case and output e32 = max |ref32 - ref64| / mag, an element passes at
|got - ref64| <= ATTN_MARGIN * max(e32, 2^-23) * mag; nothing measured on the product enters.  The backward is fed the
reference's own fp32-rounded ctx and attw (a forward error does not hide in it); one case per form is chained forward to
backward on the device and held to the reference evaluated at what the kernel was fed."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

from pfotgnrec_amd import _lib
import attn_ref as R
import philox_ref as PH

DEV = "cuda:0"
f32, f64 = np.float32, np.float64
TIME_BINS = 64
FIGURES = {}               # output family -> largest |got - ref64| / (max(e32, 2^-23) * mag) seen (the bound is ATTN_MARGIN)
FORMS_SEEN = set()


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


def bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


class Bufs:
    """Device copies of a problem's arrays (kept alive for the launch).  ``off``: the pointer starts that many elements into
    its allocation; every allocation ends in slack - NaNs around a float operand, zeros (an in-range index) around the rest."""

    def __init__(self):
        self.keep = []

    def put(self, a, dtype, off=0):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype).reshape(-1)
        if a.dtype == np.uint64:
            a = a.view(np.int64)
        t = torch.full((a.size + off + 64,), float("nan") if a.dtype.kind == "f" else 0, dtype=getattr(torch, a.dtype.name), device=DEV)
        t[off:off + a.size] = torch.from_numpy(a).to(DEV)
        self.keep.append(t)
        return t.data_ptr() + off * a.itemsize

    def out(self, a):
        """An output buffer holding exactly ``a`` (a canary, zeros, ...) -> (pointer, tensor)."""
        t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        self.keep.append(t)
        return t.data_ptr(), t


def keep_bytes(keep):
    N, H, K = keep.shape
    return sum((keep[:, h, :].astype(np.uint8) << h) for h in range(H)).astype(np.uint8)


def base_desc(b, p, qk_off=0, philox=None):
    d = _lib.AttnDesc()
    N, K, D, Ef, H, Cp = (p[k] for k in ("N", "K", "D", "Ef", "H", "Cp"))
    d.N, d.K, d.D, d.Ef, d.H, d.Cp = N, K, D, Ef, H, Cp
    d.QK = b.put(p["QK"], f32, qk_off)
    d.qk_row = b.put(p["qk_row"], np.int32)
    d.qk_ld = 0 if p["qk_ld"] == H * Cp else p["qk_ld"]
    d.nbr_tab, d.nbr_ld = b.put(p["nbr_tab"], f32), p["nbr_ld"]
    d.nbr_row, d.nbr_row_base = b.put(p["nbr_row"], np.int32), p["nbr_row_base"]
    d.nbr_rows, d.edge_rows, d.nbr_relu = p["nbr_rows"], p["edge_rows"], p["nbr_relu"]
    d.nbr_ids, d.eidx, d.dt = b.put(p["nbr_ids"], np.int32), b.put(p["eidx"], np.int32), b.put(p["dt"], f32)
    d.edge_feat = b.put(p["edge_feat"], f32) if Ef else None
    d.tw, d.tb = b.put(p["tw"], f32), b.put(p["tb"], f32)
    d.scale, d.dropout_p = p["scale"], p["dropout_p"]
    if philox is not None:
        d.seed, d.offset = philox["seed"], philox["offset"]
        d.offset_dev = b.put(np.array([philox["word"]], np.uint64), np.uint64)
    elif p["dropout_p"] > 0:
        d.keep_inject = b.put(keep_bytes(p["keep"]), np.uint8)
    d.d_nbr_nrep = 1
    return d


def form_of(d, backward):
    f = _lib.load().pfo_debug_attn_form(C.byref(d), 1 if backward else 0)
    assert f >= 0, _lib.load().pfo_last_error().decode()
    FORMS_SEEN.add(_lib.ATTN_FORMS[f])
    return _lib.ATTN_FORMS[f]


def hold(name, got, ref32, ref64, mag, where=None, extra=0.0):
    """Per element |got - ref64| <= bar (+ extra: an absolute, derived term); where mag is 0 the bits of the reference."""
    got, r64, mag = np.asarray(got).reshape(-1), np.asarray(ref64, f64).reshape(-1), np.asarray(mag, f64).reshape(-1)
    r32 = np.asarray(ref32, f64).reshape(-1)
    if where is not None:
        w = np.asarray(where).reshape(-1)
        got, r64, r32, mag = got[w], r64[w], r32[w], mag[w]
    bar, e32 = R.bar(r32, r64, mag)
    assert np.isfinite(got).all(), "%s: an element the call must write still holds the canary (or is not finite)" % name
    d = np.abs(got.astype(f64) - r64)
    unit = max(e32, R.EPS_FLOOR) * mag
    nz = mag > 0
    ratio = float((d[nz] / unit[nz]).max()) if nz.any() else 0.0
    FIGURES[name] = max(FIGURES.get(name, 0.0), ratio)
    print("%s: worst |got - ref64| / (max(e32, 2^-23) mag) = %.3g (e32 = %.3g 2^-24, bound %g)" % (name, ratio, e32 * 2 ** 24, R.ATTN_MARGIN))
    if extra == 0.0 and got.dtype == np.float32:
        z = ~nz
        assert np.array_equal(bits(got[z]), bits(r64[z].astype(f32))), "%s: an element without rounding differs in its bits" % name
    bad = d > bar + extra
    assert not bad.any(), "%s: %d elements beyond the bar, worst ratio %.3g (bound %g)" % (name, int(bad.sum()), ratio, R.ATTN_MARGIN)


# ------------------------------------------------------------------------------------------------ forward
class Fwd:
    def __init__(self, p, qk_off=0, philox=None):
        self.p, self.b = p, Bufs()
        N, K, H, Cp = p["N"], p["K"], p["H"], p["Cp"]
        self.d = d = base_desc(self.b, p, qk_off, philox)
        self.ctx0, self.attw0, self.inv0 = canary((N + 2) * H * Cp), canary((N + 2) * H * K), np.full(N + 2, 0xAB, np.uint8)
        d.ctx, self.ctx = self.b.out(self.ctx0)
        d.attw, self.attw = self.b.out(self.attw0)
        d.inv, self.inv = self.b.out(self.inv0)

    def launch(self):
        _lib.call("pfo_debug_attn_fwd", C.byref(self.d), _lib.stream_ptr())
        torch.cuda.synchronize()
        return self.ctx.cpu().numpy(), self.attw.cpu().numpy(), self.inv.cpu().numpy()


def check_forward(p, form, qk_off=0, philox=None, tag="fwd"):
    if philox is not None:
        p["keep"] = PH.dropout_keep(philox["seed"], philox["offset"] + philox["word"], p["N"], p["K"], p["H"], p["dropout_p"])
    N, K, H, Cp = p["N"], p["K"], p["H"], p["Cp"]
    ref64, mag = R.forward(p, f64)
    ref32, _ = R.forward(p, f32)
    f = Fwd(p, qk_off, philox)
    assert form_of(f.d, False) == form
    ctx, attw, inv = f.launch()
    g = Fwd(p, qk_off, philox)
    ctx2, attw2, inv2 = g.launch()
    assert np.array_equal(bits(ctx), bits(ctx2)) and np.array_equal(bits(attw), bits(attw2)) and np.array_equal(inv, inv2), "two launches differ"
    assert np.array_equal(inv[:N], ref64["inv"]) and np.all(inv[N:] == 0xAB), "inv"
    assert np.array_equal(bits(ctx[N * H * Cp:]), bits(f.ctx0[N * H * Cp:])), "ctx rows >= N touched"
    assert np.array_equal(bits(attw[N * H * K:]), bits(f.attw0[N * H * K:])), "attw rows >= N touched"
    hold(tag + " ctx", ctx[:N * H * Cp], ref32["ctx"], ref64["ctx"], mag["ctx"])
    hold(tag + " attw", attw[:N * H * K], ref32["attw"], ref64["attw"], mag["attw"])
    return f, ctx[:N * H * Cp].reshape(N, H * Cp), attw[:N * H * K].reshape(N, H, K)


PI_CASES = R.per_instance_cases()
FWD_FORM = {"ring": "fwd_ring", "reg": "fwd_reg"}
PHILOX = dict(seed=0x1234567890ABCDEF, offset=0x51ED0001, word=0x100000007)


@pytest.mark.parametrize("cid,form,kw", [c for c in PI_CASES if c[1] == "reg"], ids=[c[0] for c in PI_CASES if c[1] == "reg"])
def test_forward_register(cid, form, kw):
    check_forward(R.make_case(**kw), "fwd_reg", tag="fwd_reg")


@pytest.mark.parametrize("cid,form,kw", [c for c in PI_CASES if c[1] == "ring"], ids=[c[0] for c in PI_CASES if c[1] == "ring"])
def test_forward_ring(cid, form, kw):
    check_forward(R.make_case(**kw), "fwd_ring", tag="fwd_ring")


ALL_SHAPES = [("ring", s) for s in R.RING_SHAPES] + [("reg", s) for s in R.REG_SHAPES + [R.ODD_SHAPE]]


@pytest.mark.parametrize("form,shape", ALL_SHAPES, ids=["%s-%d-%d-%d" % ((f,) + s) for f, s in ALL_SHAPES])
def test_forward_philox_draws_and_device_offset(form, shape):
    """p = 0.1 with the kernel's own Philox draws (tests/philox_ref.py) and the offset split between the host word and a
    device word above 2^32."""
    D, Ef, H = shape
    p = R.make_case(D, Ef, H, R.K_DEFAULT, p_drop=0.1, table=True, qk_share=True, seed=5)
    check_forward(p, FWD_FORM[form], philox=PHILOX, tag=FWD_FORM[form])


@pytest.mark.parametrize("how", ["qk_off", "nbr_ld"])
def test_forward_misaligned_operands_take_the_register_form(how):
    """(32, 4, 2) is a ring shape; QK one float into its allocation, or rows of D + 1 floats, cannot move 16 bytes at a time."""
    p = R.make_case(32, 4, 2, R.K_DEFAULT, p_drop=0.1, nbr_ld=33 if how == "nbr_ld" else None, seed=7)
    check_forward(p, "fwd_reg", qk_off=1 if how == "qk_off" else 0, tag="fwd_reg")


# ------------------------------------------------------------------------------------------------ per-instance backward
class Bwd:
    """mode: 'none' | 'direct' | 'atomic' | 'det'.  ctx / attw: numpy arrays (uploaded) or the device tensors of a forward."""

    def __init__(self, p, mode, ctx, attw, n_rep=1, philox=None, runs=None):
        self.p, self.b, self.mode, self.n_rep = p, Bufs(), mode, n_rep
        N, K, D, H, Cp = p["N"], p["K"], p["D"], p["H"], p["Cp"]
        b = self.b
        self.d = d = base_desc(b, p, 0, philox)
        # the forward's outputs are inputs here; inv is not read but must be given
        d.ctx = ctx.data_ptr() if torch.is_tensor(ctx) else b.put(ctx, f32)
        d.attw = attw.data_ptr() if torch.is_tensor(attw) else b.put(attw, f32)
        b.keep += [ctx, attw]
        d.inv, _ = b.out(np.zeros(N + 2, np.uint8))
        d.dctx = b.put(p["dctx"], f32)
        self.dqk0 = canary((N + 2) * H * Cp)
        d.dQK, self.dqk = b.out(self.dqk0)
        self.ld = D + 4
        rows = p["nbr_rows"]
        if mode == "direct":
            assert p["nbr_row"] is None
            self.dn0 = canary(rows * self.ld)
            d.d_nbr, self.dn = b.out(self.dn0)
            d.d_nbr_ld = self.ld
        elif mode == "atomic":
            d.d_nbr, self.dn = b.out(np.zeros(n_rep * rows * self.ld, f32))
            d.d_nbr_ld, d.d_nbr_rep, d.d_nbr_nrep = self.ld, (rows * self.ld if n_rep > 1 else 0), n_rep
        elif mode == "det":
            d.d_nbr, self.dn = b.out(np.zeros(rows * self.ld, np.int64))
            d.d_nbr_ld = self.ld
        self.det = mode == "det"
        d.det = 1 if self.det else 0
        rng = np.random.default_rng(3)
        self.bins0 = rng.standard_normal((TIME_BINS, 2 * D))                   # the kernel ADDS to the bins: they start non-zero
        d.dtime_part, self.bins = b.out(self.bins0)
        self.n_slab = int(_lib.byte_count("pfo_debug_attn_det_parts", N))
        d.dtime_slab, self.slab = b.out(np.full((self.n_slab + 1) * 2 * D, np.nan))
        if runs is not None:
            d.members, d.seg_ptr, d.n_rows, d.run_cnt = runs["members"], runs["seg_ptr"], runs["n_rows"], runs["run_cnt"]
            self.live0 = np.full(N + 2, 0xAB, np.uint8)
            d.dqk_live, self.live = b.out(self.live0)

    def launch(self):
        parts = C.c_int32(-1)
        _lib.call("pfo_debug_attn_bwd", C.byref(self.d), C.byref(parts), _lib.stream_ptr())
        torch.cuda.synchronize()
        self.parts = parts.value
        return self

    def time_sums(self):
        D = self.p["D"]
        if self.det:
            assert self.parts == self.n_slab
            slab = self.slab.cpu().numpy()
            assert np.isfinite(slab[:self.parts * 2 * D]).all(), "a slab row was not written"
            assert np.isnan(slab[self.parts * 2 * D:]).all(), "the slab was written behind its last row"
            assert np.array_equal(self.bins.cpu().numpy(), self.bins0), "deterministic mode must leave the bins alone"
            s = np.zeros(2 * D)
            for r in slab[:self.parts * 2 * D].reshape(self.parts, 2 * D):      # row order
                s = s + r
        else:
            assert self.parts == TIME_BINS
            s = (self.bins.cpu().numpy() - self.bins0).sum(axis=0)
        return s[:D], s[D:]


def check_backward(p, mode, form, ctx=None, attw=None, n_rep=1, tag=None, twice=False):
    """ctx / attw None: the reference's own fp32-rounded forward."""
    N, K, D, H, Cp = p["N"], p["K"], p["D"], p["H"], p["Cp"]
    tag = tag or form
    if ctx is None:
        fo, _ = R.forward(p, f64)
        ctx_np, attw_np = fo["ctx"].astype(f32), fo["attw"].astype(f32)
        ctx, attw = ctx_np, attw_np
    else:
        ctx_np, attw_np = ctx.cpu().numpy()[:N * H * Cp].reshape(N, H * Cp), attw.cpu().numpy()[:N * H * K].reshape(N, H, K)
    ref64, mag = R.backward(p, ctx_np, attw_np, f64)
    ref32, _ = R.backward(p, ctx_np, attw_np, f32)
    w = Bwd(p, mode, ctx, attw, n_rep)
    assert form_of(w.d, True) == form
    w.launch()
    dqk = w.dqk.cpu().numpy()
    assert np.array_equal(bits(dqk[N * H * Cp:]), bits(w.dqk0[N * H * Cp:])), "dQK rows >= N touched"
    hold(tag + " dQK", dqk[:N * H * Cp], ref32["dQK"], ref64["dQK"], mag["dQK"])
    rows, ld = p["nbr_rows"], w.ld
    if mode == "direct":
        dn = w.dn.cpu().numpy().reshape(rows, ld)
        own = np.zeros((rows, ld), bool)
        own[p["nbr_row_base"]:p["nbr_row_base"] + N * K, :D] = True
        assert np.array_equal(bits(dn[~own]), bits(w.dn0.reshape(rows, ld)[~own])), "a plain-stored row nobody owns, or a padding column, was touched"
        hold(tag + " d_slot", dn[own], ref32["d_slot"], ref64["d_slot"], mag["d_slot"])
    elif mode == "atomic":
        dn = w.dn.cpu().numpy().reshape(n_rep, rows, ld)
        named = np.zeros((rows, ld), bool)
        named[np.unique(R.rows_of(p)[p["nbr_ids"] != 0]), :D] = True
        assert not bits(dn[:, ~named]).any(), "a table row nobody names (or a padding column) is no longer +0"
        total = dn[0].astype(f64)
        for r in range(1, n_rep):
            total = total + dn[r]
        hold(tag + " d_tab", total[:, :D], ref32["d_tab"], ref64["d_tab"], mag["d_tab"])
    elif mode == "det":
        dn = w.dn.cpu().numpy().reshape(rows, ld)
        named = np.zeros((rows, ld), bool)
        named[np.unique(R.rows_of(p)[p["nbr_ids"] != 0]), :D] = True
        assert not dn[~named].any(), "a table row nobody names (or a padding column) was added to"
        # every addend is rounded to the table's resolution 2^-40: half a unit per (instance, slot) that can land on an element
        hold(tag + " d_tab", dn[:, :D].astype(f64) / R.DET_SCALE, ref32["d_tab"], ref64["d_tab"], mag["d_tab"], extra=N * K * 0.5 / R.DET_SCALE)
    dw, db = w.time_sums()
    hold(tag + " dw", dw, ref32["dw"], ref64["dw"], mag["dw"])
    hold(tag + " db", db, ref32["db"], ref64["db"], mag["db"])
    if twice:
        v = Bwd(p, mode, ctx, attw, n_rep).launch()
        assert np.array_equal(bits(v.dqk.cpu().numpy()), bits(dqk)), "two launches differ in dQK"
        assert np.array_equal(v.dn.cpu().numpy(), w.dn.cpu().numpy()), "two launches differ in the table"
        assert np.array_equal(v.slab.cpu().numpy()[:v.parts * 2 * D], w.slab.cpu().numpy()[:w.parts * 2 * D]), "two launches differ in the slab"
    return w


def bwd_cases():
    """(id, make_case arguments, mode, expected form, replicas)"""
    out = []
    drops = [0.0, 0.1, 0.5]
    for i, (form, (D, Ef, H)) in enumerate(ALL_SHAPES):
        ring = form == "ring"
        kw = dict(D=D, Ef=Ef, H=H, K=R.K_DEFAULT, p_drop=drops[i % 3], qk_share=bool(i % 2), big=(i % 4 == 1))
        sid = "%d-%d-%d" % (D, Ef, H)
        out.append(("none-" + sid, dict(kw, table=bool((i + 1) % 2)), "none", "bwd_ring_none" if ring else "bwd_none", 1))
        for relu in (0, 1):
            out.append(("direct-relu%d-%s" % (relu, sid), dict(kw, relu=relu), "direct", "bwd_ring_direct" if ring else "bwd_direct", 1))
        reps = [1, 2, 4] if (D, Ef, H) in ((32, 4, 2), (64, 4, 2)) else [(1, 2, 4)[i % 3]]
        for n_rep in reps:
            out.append(("atomic%d-%s" % (n_rep, sid), dict(kw, table=True), "atomic", "bwd_atomic", n_rep))
        out.append(("det-" + sid, dict(kw, table=True), "det", "bwd_det", 1))
    modes = [("none", "bwd_ring_none", "bwd_none"), ("direct", "bwd_ring_direct", "bwd_direct"), ("atomic", "bwd_atomic", "bwd_atomic"),
             ("det", "bwd_det", "bwd_det")]
    for form, (D, Ef, H) in (("ring", (32, 4, 2)), ("reg", (64, 4, 2))):
        for i, K in enumerate(R.K_LIST):
            mode, f_ring, f_reg = modes[i % 4]
            out.append(("%s-%d-%d-%d-K%d" % (mode, D, Ef, H, K), dict(D=D, Ef=Ef, H=H, K=K, p_drop=0.1, table=mode in ("atomic", "det"), relu=1),
                        mode, f_ring if form == "ring" else f_reg, 2 if mode == "atomic" else 1))
    return out


BWD_CASES = bwd_cases()


@pytest.mark.parametrize("cid,kw,mode,form,n_rep", BWD_CASES, ids=[c[0] for c in BWD_CASES])
def test_backward_per_instance(cid, kw, mode, form, n_rep):
    check_backward(R.make_case(**kw), mode, form, n_rep=n_rep, twice=(mode == "det"))


@pytest.mark.parametrize("mode,form", [("none", "bwd_none"), ("direct", "bwd_direct")])
def test_backward_misaligned_rows_take_the_register_form(mode, form):
    check_backward(R.make_case(32, 4, 2, R.K_DEFAULT, p_drop=0.1, nbr_ld=33, relu=1, seed=7), mode, form)


CHAINED = [("bwd_ring_none", (32, 4, 2), "none"), ("bwd_ring_direct", (124, 4, 4), "direct"), ("bwd_none", (64, 4, 2), "none"),
           ("bwd_direct", (192, 4, 2), "direct"), ("bwd_atomic", (172, 12, 4), "atomic"), ("bwd_det", (128, 4, 4), "det")]


@pytest.mark.parametrize("form,shape,mode", CHAINED, ids=[c[0] for c in CHAINED])
def test_forward_chained_to_backward(form, shape, mode):
    """As the product does: the backward reads the ctx and attw the forward left on the device; the reference is evaluated
    at exactly those."""
    D, Ef, H = shape
    p = R.make_case(D, Ef, H, R.K_DEFAULT, p_drop=0.1, table=mode in ("atomic", "det"), relu=1, seed=11)
    f, _, _ = check_forward(p, FWD_FORM["ring" if shape in R.RING_SHAPES else "reg"], tag="chained fwd")
    check_backward(p, mode, form, ctx=f.ctx, attw=f.attw, n_rep=2 if mode == "atomic" else 1, tag="chained " + form)


# ------------------------------------------------------------------------------------------------ run-merged backward
def build_grouping(b, p, with_key):
    """pfo_debug_seg_build over the problem's instances -> device pointers, and the numpy arrays it must equal."""
    N, cap = p["N"], p["cap_rows"]
    scan = int(_lib.byte_count("pfo_debug_seg_scratch_ints", cap))
    n_scr = scan + 2 * (cap + 1) + N
    n_of = int(_lib.byte_count("pfo_debug_seg_of_ints", N))
    idx, nodes, cnt = b.put(p["qk_row"], np.int32), b.put(p["nodes"], np.int32), b.put(p["run_cnt"], np.int32)
    seg_ptr, t_ptr = b.out(np.full(cap + 1, -7, np.int32))
    members, t_mem = b.out(np.zeros(N, np.int32))                        # behind M: in-range values
    seg_of, t_of = b.out(np.zeros(n_of, np.int32))
    scratch, _ = b.out(np.zeros(n_scr, np.int32))
    _lib.call("pfo_debug_seg_build", idx, nodes, N, cap, cnt if with_key else None, seg_ptr, members, seg_of, scratch, n_scr, _lib.stream_ptr())
    torch.cuda.synchronize()
    e_ptr, e_mem, e_of = R.grouping(p["qk_row"], p["nodes"], cap, p["run_cnt"] if with_key else None)
    M = len(e_mem)
    assert np.array_equal(t_ptr.cpu().numpy(), e_ptr), "seg_ptr"
    assert np.array_equal(t_mem.cpu().numpy()[:M], e_mem) and not t_mem.cpu().numpy()[M:].any(), "members"
    assert np.array_equal(t_of.cpu().numpy()[:M], e_of) and not t_of.cpu().numpy()[M:].any(), "seg_of"
    n_rows = b.put(np.array([p["n_rows"]], np.int32), np.int32)
    return dict(members=members, seg_ptr=seg_ptr, seg_of=seg_of, n_rows=n_rows, run_cnt=cnt), e_ptr, e_mem, e_of


RUNS_CASES = R.runs_cases()


@pytest.mark.parametrize("det", [0, 1], ids=["plain", "det"])
@pytest.mark.parametrize("name,kw", RUNS_CASES, ids=[c[0] for c in RUNS_CASES])
def test_backward_run_merged(name, kw, det):
    p = R.make_runs_case(**kw)
    N, K, D, H, Cp = p["N"], p["K"], p["D"], p["H"], p["Cp"]
    W = H * Cp
    b = Bufs()
    build_grouping(b, p, with_key=False)                                 # (uniform sampling's order: by instance)
    g, seg_ptr, members, seg_of = build_grouping(b, p, with_key=True)
    M = len(members)
    fo, _ = R.forward(p, f64)
    ctx, attw = fo["ctx"].astype(f32), fo["attw"].astype(f32)
    ref64, mag = R.backward(p, ctx, attw, f64)
    ref32, _ = R.backward(p, ctx, attw, f32)
    n_rep = 1 if det else 4
    w = Bwd(p, "det" if det else "atomic", ctx, attw, n_rep, runs=g)
    w.b.keep.append(b)
    assert form_of(w.d, True) == "bwd_runs"
    w.launch()
    tag = "bwd_runs det" if det else "bwd_runs"
    # the live-row rule
    live = w.live.cpu().numpy()
    assert np.all(live[M:] == 0xAB) and set(np.unique(live[:M])) <= {0, 1}, "live flags"
    live = live[:M].astype(bool)
    dqk = w.dqk.cpu().numpy().reshape(N + 2, W)
    dead = np.ones(N + 2, bool)
    dead[np.flatnonzero(live)] = False
    assert np.array_equal(bits(dqk[dead]), bits(w.dqk0.reshape(N + 2, W)[dead])), "a dQK row that is not live (or behind M) was touched"
    r64, r32, rmag = (R.runs_rows(x["dQK"], members, seg_of, live) for x in (ref64, ref32, mag))
    for q in range(M):                                                   # every run lies inside one group: a group's last live row closes it
        assert live[q] or q + 1 < M and seg_of[q + 1] == seg_of[q] or not (p["nbr_ids"][members[q]] != 0).any()
    hold(tag + " dQK rows", dqk[:M][live], r32[live], r64[live], rmag[live])
    # the per-row sums through the public pfo_segment_sum, by position with the live flags
    side = np.random.default_rng(9).standard_normal((N, 4)).astype(f32)
    out0 = canary(p["cap_rows"] * (W + 4))
    o_ptr, o_t = b.out(out0)
    _lib.call("pfo_segment_sum", w.d.dQK, W, b.put(side, f32), 4, g["seg_ptr"], g["members"], g["seg_of"], N, g["n_rows"], p["cap_rows"], 1,
              w.d.dqk_live, o_ptr, _lib.stream_ptr())
    torch.cuda.synchronize()
    sums = o_t.cpu().numpy().reshape(p["cap_rows"], W + 4)
    nr = p["n_rows"]
    assert np.array_equal(bits(sums[nr:]), bits(out0.reshape(-1, W + 4)[nr:])), "rows >= *n_rows touched"
    s64, s32, smag = (R.group_sums(x["dQK"], members, seg_ptr, nr) for x in (ref64, ref32, mag))
    hold(tag + " row sums", sums[:nr, :W], s32, s64, smag)
    assert np.allclose(sums[:nr, W:], R.group_sums(side.astype(f64), members, seg_ptr, nr), rtol=1e-6, atol=1e-6)
    # the key-side table
    rows, ld = p["nbr_rows"], w.ld
    named = np.zeros((rows, ld), bool)
    named[np.unique(p["nbr_row"][p["nbr_ids"] != 0]), :D] = True
    if det:
        dn = w.dn.cpu().numpy().reshape(rows, ld)
        assert not dn[~named].any(), "a table row nobody names was added to"
        hold(tag + " d_tab", dn[:, :D].astype(f64) / R.DET_SCALE, ref32["d_tab"], ref64["d_tab"], mag["d_tab"], extra=N * K * 0.5 / R.DET_SCALE)
    else:
        dn = w.dn.cpu().numpy().reshape(n_rep, rows, ld)
        assert not bits(dn[:, ~named]).any(), "a table row nobody names is no longer +0"
        hold(tag + " d_tab", dn.astype(f64).sum(axis=0)[:, :D], ref32["d_tab"], ref64["d_tab"], mag["d_tab"])
    dw, db = w.time_sums()
    hold(tag + " dw", dw, ref32["dw"], ref64["dw"], mag["dw"])
    hold(tag + " db", db, ref32["db"], ref64["db"], mag["db"])
    if det:
        v = Bwd(p, "det", ctx, attw, 1, runs=g).launch()
        assert np.array_equal(v.dn.cpu().numpy(), w.dn.cpu().numpy()) and np.array_equal(v.slab.cpu().numpy()[:v.parts * 2 * D], w.slab.cpu().numpy()[:w.parts * 2 * D])
        assert np.array_equal(bits(v.dqk.cpu().numpy()), bits(w.dqk.cpu().numpy())) and np.array_equal(v.live.cpu().numpy(), w.live.cpu().numpy())


def test_four_heads_beyond_192_columns_stay_per_instance():
    """(256, 0, 4): the run-merged kernel would spill there (pfo_attn_bwd_runs_possible); members given, the launcher must
    take - and report - the per-instance kernel, whose dQK rows belong to instances."""
    p = R.make_runs_case(256, 0, 4, 5, groups=R.GROUPS_SEVEN, p_drop=0.1)
    b = Bufs()
    g, _, _, _ = build_grouping(b, p, with_key=True)
    fo, _ = R.forward(p, f64)
    w = Bwd(p, "atomic", fo["ctx"].astype(f32), fo["attw"].astype(f32), 2, runs=g)
    w.b.keep.append(b)
    assert form_of(w.d, True) == "bwd_atomic"
    check_backward(p, "atomic", "bwd_atomic", n_rep=2)


@pytest.mark.parametrize("D,Ef,H,K", R.RUNS_SHAPES, ids=["%d-%d-%d-K%d" % s for s in R.RUNS_SHAPES])
def test_lists_that_are_not_shifts_go_without_members(D, Ef, H, K):
    """Uniform sampling: the same shapes, slots shuffled per instance, no members -> the per-instance atomic kernel."""
    p = R.make_runs_case(D, Ef, H, K, groups=R.GROUPS_SEVEN, shifts=False, p_drop=0.1)
    check_backward(p, "atomic", "bwd_atomic", n_rep=4, tag="bwd_atomic uniform")


def test_odd_shape_run_merged_matches_or_refuses():
    """(30, 6, 2) passes check_common and no config produces it: the run-merged launcher must match the reference or refuse."""
    p = R.make_runs_case(30, 6, 2, 5, groups=R.GROUPS_SEVEN, p_drop=0.1)
    b = Bufs()
    g, seg_ptr, members, seg_of = build_grouping(b, p, with_key=True)
    fo, _ = R.forward(p, f64)
    ctx, attw = fo["ctx"].astype(f32), fo["attw"].astype(f32)
    w = Bwd(p, "atomic", ctx, attw, 2, runs=g)
    w.b.keep.append(b)
    form = form_of(w.d, True)
    assert form in ("bwd_runs", "bwd_atomic")
    try:
        w.launch()
    except _lib.PfoError:
        return                                                          # a refusal with a message
    ref64, mag = R.backward(p, ctx, attw, f64)
    ref32, _ = R.backward(p, ctx, attw, f32)
    dn = w.dn.cpu().numpy().reshape(2, p["nbr_rows"], w.ld)
    hold("odd shape d_tab", dn.astype(f64).sum(axis=0)[:, :p["D"]], ref32["d_tab"], ref64["d_tab"], mag["d_tab"])
    dw, db = w.time_sums()
    hold("odd shape dw", dw, ref32["dw"], ref64["dw"], mag["dw"])
    if form == "bwd_runs":
        live = w.live.cpu().numpy()[:len(members)].astype(bool)
        r64, r32, rmag = (R.runs_rows(x["dQK"], members, seg_of, live) for x in (ref64, ref32, mag))
        hold("odd shape dQK rows", w.dqk.cpu().numpy().reshape(-1, p["H"] * p["Cp"])[:len(members)][live], r32[live], r64[live], rmag[live])


def test_zz_every_form_was_reached_and_figures():
    """Runs last in the file: the forms reached by the cases above (when the whole file ran) and the FIGURES line."""
    print("FIGURES " + "; ".join("%s %.2f" % (k, v) for k, v in sorted(FIGURES.items())))
    if len(FIGURES) > 20:                                                # the whole file ran, not a selection
        assert FORMS_SEEN == set(_lib.ATTN_FORMS), sorted(set(_lib.ATTN_FORMS) - FORMS_SEEN)
