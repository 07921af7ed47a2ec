"""Every form of the internal contraction interface (pfotgnrec_amd/csrc/gemm.hpp), launched through the pfo_debug_* probes
and held per element to the float64 models of tests/gemm_ref.py.

Each case
  * takes its operands from the wide-dynamic-range generator (randn * exp(2 randn)),
  * fills every output buffer with a canary (quiet NaNs with the element's index as payload), allocated with ldc > N and
    rows beyond M, and asserts bit for bit that padding columns, rows >= m_dev and rows >= M are untouched,
  * runs with the profiler on and asserts the kernel family that ran, so that a dispatch change cannot quietly turn one
    case into a copy of another.

Tolerances (DESIGN.md "Contraction forms under test"): |got - ref| < 4e-6 * mag per element for the image and weight-gradient
forms, mag = sum |a||b| + |every addend| (floored per tile for the weight-gradient forms that keep one scale per tile); the
exact-fp32 kernel to its bound of tests/test_gpu_kernels.py plus a per-element one from its rounding count."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

from pfotgnrec_amd import _lib
import gemm_ref as G

DEV = "cuda:0"
TOL = 4e-6
f64 = np.float64

CONTRACTION_KINDS = ["gemm_nt", "gemm_nn", "gemm_tn", "gemm_devm", "gemm_bx", "gemm_tn_bx", "gemm_bx_skinny", "gru_fused", "gemm_multi",
                     "tn_reduce", "gemm_tn_bx8"]


@pytest.fixture(autouse=True)
def stop_after_a_gpu_error():
    """A kernel that faulted leaves the device in an error state: the run ends there instead of launching more on it."""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:                                             # noqa: BLE001 - whatever the runtime raises
        pytest.exit("the GPU reported an error (%s): nothing more is launched" % e, returncode=3)


def cdiv(a, b):
    return -(-a // b)


def canary(n):
    return (np.uint32(0x7FC00000) | (np.arange(n, dtype=np.uint32) % np.uint32(0x3FFFFF) + np.uint32(1))).view(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


class Bufs:
    """Device copies of a problem's arrays (kept alive for the launch).  ``off``: the pointer starts that many elements
    into its allocation (a misaligned operand); every allocation ends in a little slack.  Around a float operand the slack
    holds NaNs: a kernel that reads past an operand's end (a K tail on the last row) and uses the value shows it."""

    def __init__(self):
        self.keep = []

    def put(self, a, dtype, off=0):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype).reshape(-1)
        t = torch.full((a.size + off + 64,), float("nan") if a.dtype == np.float32 else 0, dtype=getattr(torch, np.dtype(dtype).name),
                       device=DEV)
        t[off:off + a.size] = torch.from_numpy(a).to(DEV)
        self.keep.append(t)
        return t.data_ptr() + off * a.itemsize

    def raw(self, nbytes):
        t = torch.zeros(nbytes + 256, dtype=torch.uint8, device=DEV)
        self.keep.append(t)
        return t.data_ptr()


class profiled:
    """``with profiled() as k:`` - afterwards k.kinds maps every contraction family that ran to its launch count."""

    def __enter__(self):
        _lib.prof_collect()
        _lib.prof_enable(True)
        self.kinds = None
        return self

    def __exit__(self, *exc):
        _lib.prof_enable(False)
        c = _lib.prof_collect()
        self.kinds = {k: c[k]["count"] for k in CONTRACTION_KINDS if c[k]["count"]}
        return False


def image(b, ptr, ld, N, K, trans):
    nbytes = _lib.byte_count("pfo_debug_bimg_bytes", N, K)
    d = _lib.BimgDesc(src=ptr, ld=ld, N=N, K=K, trans=trans, dst=b.raw(nbytes))
    _lib.call("pfo_debug_bimg", C.byref(d), 1, _lib.stream_ptr())
    return d.dst


def fill_gemm_desc(b, d, img=False, bx_force=0, mis=()):
    """The ctypes descriptor of problem ``d`` (tests/gemm_ref.py layout) over device copies; returns (desc, C tensor)."""
    d = G.gemm_desc(**d)
    g = _lib.GemmDesc()
    for s in range(2):
        if d["A"][s] is None:
            continue
        g.A[s] = b.put(d["A"][s], np.float32, 1 if "A%d" % s in mis else 0)
        g.B[s] = b.put(d["B"][s], np.float32, 1 if "B%d" % s in mis else 0)
        g.lda[s], g.ldb[s], g.K[s], g.a_bs[s], g.b_bs[s] = d["lda"][s], d["ldb"][s], d["K"][s], d["a_bs"][s], d["b_bs"][s]
        g.a_idx[s] = b.put(d["a_idx"][s], np.int32)
        if img and d["K"][s] > 0:
            im = image(b, g.B[s], d["ldb"][s], d["N"], d["K"][s], d["b_kmajor"])
            if s == 0:
                g.b_img = im
            else:
                g.b_img2 = im
    g.b_idx = b.put(d["b_idx"], np.int32)
    g.C = b.put(d["C"], np.float32, 1 if "C" in mis else 0)
    c_t, c_off = b.keep[-1], (1 if "C" in mis else 0)
    g.ldc, g.M, g.N = d["ldc"], d["M"], d["N"]
    g.bias = b.put(d["bias"], np.float32, 1 if "bias" in mis else 0)
    g.row_scale, g.rs_ld = b.put(d["row_scale"], np.float32), d["rs_ld"]
    g.row_zero = b.put(d["row_zero"], np.uint8)
    g.relu_src, g.relu_ld = b.put(d["relu_src"], np.float32), d["relu_ld"]
    g.add_src, g.add_ld, g.add_idx = b.put(d["add_src"], np.float32), d["add_ld"], b.put(d["add_idx"], np.int32)
    g.m_dev = b.put(d["m_dev"], np.int32)
    g.relu, g.accumulate, g.a_kmajor, g.b_kmajor, g.batch = d["relu"], d["accumulate"], d["a_kmajor"], d["b_kmajor"], d["batch"]
    g.c_bs, g.bias_bs, g.rs_bs = d["c_bs"], d["bias_bs"], d["rs_bs"]
    g.bx_force = bx_force
    n = np.asarray(d["C"]).size
    return g, (lambda: c_t[c_off:c_off + n].cpu().numpy())


def gemm_plan(g, form=None):
    """What the launcher will do with descriptor ``g`` (pfo_debug_gemm_plan: the function pfo_gemm_launch itself switches on),
    held to the model of tests/gemm_ref.py on this very descriptor; ``form``: the kernel the case was written for."""
    plan = _lib.gemm_plan("pfo_debug_gemm_plan", C.byref(g))
    ref = G.gemm_plan_ref(g)
    assert plan == {k: ref[k] for k in plan}, (plan, ref)
    assert form is None or plan["form"] == form, (plan["form"], form)
    return plan


def launch_gemm(d, img=False, bx_force=0, mis=(), form=None):
    """-> (the C buffer after the launch, the profiler families that ran, the launcher's plan); the plan is asked, and ``form``
    asserted, before anything is launched."""
    b = Bufs()
    g, read = fill_gemm_desc(b, d, img, bx_force, mis)
    plan = gemm_plan(g, form)
    with profiled() as p:
        _lib.call("pfo_debug_gemm", C.byref(g), _lib.stream_ptr())
        torch.cuda.synchronize()
    return read(), p.kinds, plan


def within(got, ref, mag, tol):
    """|got - ref| < tol * mag for every element (exact agreement where mag is 0); returns the worst ratio for the message."""
    diff = np.abs(got.astype(f64) - ref)
    ok = (diff < tol * mag) | (diff == 0)
    worst = float((diff / np.maximum(mag, 1e-300)).max()) if diff.size else 0.0
    return bool(ok.all()), worst


BIG_CHUNK = 4096


def check_gemm(d, got, tol=TOL, big=False):
    """Per-element parity on EVERY written element, every written element finite, every other element of the buffer bit for
    bit what it was.  ``big``: the reference of a large problem is evaluated BIG_CHUNK rows at a time (the same comparison,
    less memory)."""
    d = G.gemm_desc(**d)
    C0 = np.asarray(d["C"], np.float32).reshape(-1)
    if not big:
        ref, mag, wr = G.gemm_ref(d)
        ok, worst = within(got[wr], ref[wr], mag[wr], tol)
        norm = (float(np.abs(got[wr] - ref[wr]).max()), float(np.abs(ref[wr]).max())) if wr.any() else (0.0, 0.0)
    else:
        ok, worst, wr, seen, norm = True, 0.0, None, 0, (0.0, 0.0)
        for m0 in range(0, d["M"], BIG_CHUNK):
            ref, mag, w, rr = G.gemm_ref(d, np.arange(m0, min(d["M"], m0 + BIG_CHUNK)), want_written=wr is None)
            wr = w if wr is None else wr
            ci = rr[:, None] * d["ldc"] + np.arange(d["N"])[None, :]
            o, w_ = within(got[ci], ref, mag, tol)
            ok, worst, seen = ok and o, max(worst, w_), seen + ci.size
            if ci.size:
                norm = (max(norm[0], float(np.abs(got[ci] - ref).max())), max(norm[1], float(np.abs(ref).max())))
        assert seen == int(wr.sum())                                   # every written element went through the comparison
    assert np.isfinite(got[wr]).all(), "an element the call must write still holds the canary (or is not finite)"
    same = bits(got) == bits(C0)
    if d["batch"] == 1 and C0.size % d["ldc"] == 0:
        s2 = same.reshape(-1, d["ldc"])
        M, N = d["M"], d["N"]
        mlim = M if (d["m_dev"] is None or d["a_kmajor"]) else min(M, int(np.asarray(d["m_dev"]).reshape(-1)[0]))
        assert s2[:M, N:].all(), "padding columns touched"
        assert s2[mlim:M, :N].all(), "rows >= m_dev touched"
        assert s2[M:].all(), "rows >= M touched"
    assert same[~wr].all(), "an element outside the output was touched"
    assert ok, "worst |got - ref| / mag = %.3g (bound %.3g)" % (worst, tol)
    return norm                                                        # (max |got - ref|, max |ref|) over the written elements


# ------------------------------------------------------------------------------------------------ row-major image kernels
IMG_FEATURES = ["a_idx0", "a_idx1", "bias", "row_scale", "add_src", "add_idx", "row_zero", "relu", "relu_src", "accumulate"]
IMG_SETS = [(), ("a_idx0",), ("a_idx1",), ("a_idx0", "a_idx1"), ("bias",), ("bias", "row_scale"), ("add_src",), ("add_src", "add_idx"),
            ("row_zero",), ("relu",), ("relu_src",), ("accumulate",), ("b_kmajor",), ("scalar_epilogue",), tuple(IMG_FEATURES),
            tuple(IMG_FEATURES) + ("b_kmajor",), tuple(IMG_FEATURES) + ("scalar_epilogue",)]


def img_problem(rs, M, N, K0, K1, on, m_dev=None):
    """A row-major-A problem the image kernels admit (16-byte aligned rows, K a multiple of 4) with the features of ``on``;
    "scalar_epilogue": leading dimensions of C and of the epilogue operands that rule the float4 epilogue out."""
    on = set(on)
    R = M + 13                                                     # rows of a gathered table
    quad = "scalar_epilogue" not in on
    bkm = int("b_kmajor" in on)
    d = dict(M=M, N=N, K=(K0, K1), b_kmajor=bkm)
    A, B, lda, ldb, a_idx = [None, None], [None, None], [0, 0], [0, 0], [None, None]
    for s, K in enumerate((K0, K1)):
        if K == 0:
            continue
        gathered = ("a_idx%d" % s) in on
        lda[s] = K + 4
        A[s] = G.wide(rs, R if gathered else M, lda[s])
        if gathered:
            a_idx[s] = rs.randint(0, R, size=M).astype(np.int32)   # out of order, and ...
            a_idx[s][M // 2] = a_idx[s][0]                         # ... repeated
        ldb[s] = (N if bkm else K) + 4
        B[s] = G.wide(rs, K if bkm else N, ldb[s])
    d.update(A=A, B=B, lda=lda, ldb=ldb, a_idx=a_idx)
    ldc = N + (4 if quad else 3)
    C0 = canary((M + 3) * ldc).reshape(M + 3, ldc).copy()
    if "accumulate" in on:
        C0[:M, :N] = G.wide(rs, M, N)
    d.update(C=C0, ldc=ldc, accumulate=int("accumulate" in on), relu=int("relu" in on))
    if "bias" in on or "row_scale" in on:
        d["bias"] = G.wide(rs, N)
    if "row_scale" in on:
        d.update(row_scale=G.wide(rs, 3 * M), rs_ld=3)
    if "add_src" in on or "add_idx" in on:
        add_ld = N + (4 if quad else 1)
        d.update(add_src=G.wide(rs, R, add_ld), add_ld=add_ld)
    if "add_idx" in on:
        d["add_idx"] = rs.randint(0, R, size=M).astype(np.int32)
    if "row_zero" in on:
        z = (rs.rand(M) < 0.3).astype(np.uint8)
        z[M - 1] = 1
        d["row_zero"] = z
    if "relu_src" in on:
        relu_ld = N + (4 if quad else 2)
        m = G.wide(rs, M, relu_ld)
        m.reshape(-1)[::3] = 0.0
        m.reshape(-1)[1::5] = -0.0
        d.update(relu_src=m, relu_ld=relu_ld)
    if m_dev is not None:
        d["m_dev"] = np.array([m_dev], np.int32)
    return d


def two_sources_ok(on, K1):
    return K1 > 0 or "a_idx1" not in on


# (M, N, K0, K1): M in {1, 33, 77}, N in {64, 172, 344} and 177 (no multiple of 4: the launcher admits it, the epilogue goes
# element by element), K0 in {36, 148, 172}, K1 in {0, 172}: a K that is no multiple of the 32-deep tile on either source
SKINNY4_SHAPES = [(1, 64, 36, 0), (33, 172, 148, 172), (77, 344, 172, 0), (77, 177, 36, 172), (33, 64, 172, 172), (1, 344, 148, 0),
                  (77, 172, 36, 172)]
AREG_SHAPES = [(128, 64, 36, 0), (300, 172, 148, 172), (300, 344, 172, 0), (128, 177, 36, 172), (300, 64, 172, 172), (128, 344, 148, 172)]


@pytest.mark.parametrize("on", IMG_SETS, ids=lambda o: "+".join(o) or "plain")
@pytest.mark.parametrize("kernel", ["skinny4", "areg"])
def test_image_kernels_every_feature_alone_and_together(kernel, on):
    """gemm_bx_skinny_kernel<4,1> (bx_force = 2, fewer than 512 row x column blocks) and gemm_bx_areg_kernel<1> (bx_force = 1)."""
    rs = np.random.RandomState(len(on) + 100 * (kernel == "areg"))
    for M, N, K0, K1 in (SKINNY4_SHAPES if kernel == "skinny4" else AREG_SHAPES):
        if not two_sources_ok(on, K1):
            continue
        d = img_problem(rs, M, N, K0, K1, on)
        got, kinds, _ = launch_gemm(d, img=True, bx_force=2 if kernel == "skinny4" else 1, form=kernel)
        assert kinds == ({"gemm_bx_skinny": 1} if kernel == "skinny4" else {"gemm_bx": 1}), kinds
        check_gemm(d, got)


@pytest.mark.parametrize("on", [(), tuple(IMG_FEATURES)], ids=["plain", "all"])
@pytest.mark.parametrize("kernel", ["skinny4", "areg"])
def test_image_kernels_device_side_row_count(kernel, on):
    rs = np.random.RandomState(7)
    M, N, K0, K1 = (77, 172, 148, 172) if kernel == "skinny4" else (300, 344, 36, 172)
    for m_dev in (0, 1, M - 1, M, M + 5):
        d = img_problem(rs, M, N, K0, K1, on, m_dev=m_dev)
        got, kinds, _ = launch_gemm(d, img=True, bx_force=2 if kernel == "skinny4" else 1, form=kernel)
        assert kinds == ({"gemm_bx_skinny": 1} if kernel == "skinny4" else {"gemm_bx": 1}), kinds
        check_gemm(d, got)


@pytest.mark.parametrize("on,K1,m_dev", [((), 0, None), (tuple(IMG_FEATURES), 36, None), (("scalar_epilogue",), 0, None),
                                         (tuple(IMG_FEATURES), 0, 32 * 256 + 1)], ids=["plain", "all+two", "scalar", "all+m_dev"])
def test_image_kernel_skinny_176_column_form(on, K1, m_dev):
    """gemm_bx_skinny_kernel<11,1>: 512 or more (32-row x 176-column) blocks."""
    rs = np.random.RandomState(11)
    M, N, K0 = 32 * 256 + 5, 352, 44
    d = img_problem(rs, M, N, K0, K1, on, m_dev=m_dev)
    got, kinds, _ = launch_gemm(d, img=True, bx_force=2, form="skinny11")
    assert kinds == {"gemm_bx_skinny": 1}, kinds
    check_gemm(d, got, big=True)


@pytest.mark.parametrize("on,K1,m_dev", [(("scalar_epilogue",), 0, None), ((), 36, None), (tuple(IMG_FEATURES), 36, None),
                                         (tuple(IMG_FEATURES), 0, 128 * 256 + 1)], ids=["scalar", "plain+two", "all+two", "all+m_dev"])
def test_image_kernel_eight_wavefront_form(on, K1, m_dev):
    """gemm_bx_areg8_kernel<1>: at least 512 tiles of 128 x 176, two column tiles (the XCD tile order is on), a last row tile
    of 77 rows."""
    rs = np.random.RandomState(13)
    M, N, K0 = 128 * 256 + 77, 352, 44
    d = img_problem(rs, M, N, K0, K1, on, m_dev=m_dev)
    got, kinds, plan = launch_gemm(d, img=True, form="areg8")
    assert plan["grid_y"] == 1 and plan["grid_x"] == 2 * 8 * cdiv(cdiv(M, 128), 8)   # two column tiles: the 1-D grid of the XCD tile order
    assert kinds == {"gemm_bx": 1}, kinds
    check_gemm(d, got, big=True)


@pytest.mark.parametrize("N,K0,on", [(352, 44, ()), (1024, 172, ())] + [(352, 44, (f,)) for f in
                                    ("bias", "relu", "relu_src", "add_src", "accumulate", "row_zero")] + [(352, 44, ("bias", "row_scale"))],
                         ids=lambda v: "+".join(v) if isinstance(v, tuple) else str(v))
def test_image_kernel_a_stationary_form_and_its_boundary(N, K0, on):
    """gemm_bx_astat_kernel at the two ends of its column range with ldc != N and a last workgroup of 5 rows; the same shape
    with any single epilogue flag must take another form and still be right."""
    rs = np.random.RandomState(17)
    M = 128 * 256 + 5
    d = img_problem(rs, M, N, K0, 0, on)
    assert d["ldc"] != N
    got, kinds, _ = launch_gemm(d, img=True, form="astat" if not on else "areg8")
    assert kinds == {"gemm_bx": 1}, kinds
    check_gemm(d, got, big=True)


def test_image_kernels_stacked_image():
    """One image whose rows come from two operands stacked along n (row0 / rows_total / last): the product against it is the
    product against the stacked matrix, and the rows up to the padded end hold zeros (columns past N are never written)."""
    rs = np.random.RandomState(19)
    M, K, N1, N2 = 77, 148, 100, 72
    N = N1 + N2
    W1, W2 = G.wide(rs, N1, K + 4), G.wide(rs, K, N2 + 4)               # the second operand k-major
    b = Bufs()
    nbytes = _lib.byte_count("pfo_debug_bimg_bytes", N, K)
    dst = b.raw(nbytes)
    lst = (_lib.BimgDesc * 2)(_lib.BimgDesc(src=b.put(W1, np.float32), ld=K + 4, N=N1, K=K, trans=0, dst=dst, row0=0, rows_total=N),
                              _lib.BimgDesc(src=b.put(W2, np.float32), ld=N2 + 4, N=N2, K=K, trans=1, dst=dst, row0=N1, rows_total=N, last=1))
    _lib.call("pfo_debug_bimg", lst, 2, _lib.stream_ptr())
    W = np.concatenate([W1[:, :K], W2[:, :N2].T], 0)
    d = img_problem(rs, M, N, K, 0, ("bias",))
    d["B"] = [np.ascontiguousarray(W), None]
    d["ldb"] = [K, 0]
    g, read = fill_gemm_desc(b, d)
    g.b_img = dst
    for force, kind, form in ((2, "gemm_bx_skinny", "skinny4"), (1, "gemm_bx", "areg")):
        g.bx_force = force
        gemm_plan(g, form)
        with profiled() as p:
            _lib.call("pfo_debug_gemm", C.byref(g), _lib.stream_ptr())
            torch.cuda.synchronize()
        assert p.kinds == {kind: 1}
        check_gemm(d, read())


# ------------------------------------------------------------------------------------------------ the fp32 MFMA kernel
def f32_tol(d):
    """Exact-fp32 products, fp32 accumulation: each of the K multiply-adds and of the (at most four) epilogue operations
    rounds once, by at most one ulp (2^-23) of a running magnitude that never exceeds mag."""
    return (d["K"][0] + d["K"][1] + 4) * 2.0 ** -23


def check_f32(d, got, big=False):
    d = G.gemm_desc(**d)
    err, top = check_gemm(d, got, tol=f32_tol(d), big=big)
    assert err < 2e-5 * top + 1e-5                                     # the norm-wise bound of tests/test_gpu_kernels.py


def f32_problem(rs, M, N, K, akm, bkm, on=(), pad=4, K1=0, m_dev=None):
    """A problem for the kernel without an image; ``pad``: what every leading dimension adds to its extent (odd: no float4)."""
    on = set(on)
    R = M + 9
    d = dict(M=M, N=N, K=(K, K1), a_kmajor=akm, b_kmajor=bkm)
    A, B, lda, ldb, a_idx = [None, None], [None, None], [0, 0], [0, 0], [None, None]
    for s, Ks in enumerate((K, K1)):
        if Ks == 0:
            continue
        gathered = ("a_idx%d" % s) in on and not akm
        lda[s] = (M if akm else Ks) + pad
        A[s] = G.wide(rs, Ks if akm else (R if gathered else M), lda[s])
        if gathered:
            a_idx[s] = rs.randint(0, R, size=M).astype(np.int32)
            a_idx[s][M // 2] = a_idx[s][0]
        gb = "b_idx" in on and bkm and s == 0
        ldb[s] = (N if bkm else Ks) + pad
        B[s] = G.wide(rs, (Ks + (5 if gb else 0)) if bkm else N, ldb[s])
        if gb:
            d["b_idx"] = rs.permutation(Ks + 5)[:Ks].astype(np.int32)
    d.update(A=A, B=B, lda=lda, ldb=ldb, a_idx=a_idx)
    ldc = N + 3
    C0 = canary((M + 3) * ldc).reshape(M + 3, ldc).copy()
    if "accumulate" in on:
        C0[:M, :N] = G.wide(rs, M, N)
    d.update(C=C0, ldc=ldc, accumulate=int("accumulate" in on), relu=int("relu" in on))
    if "bias" in on or "row_scale" in on:
        d["bias"] = G.wide(rs, N)
    if "row_scale" in on:
        d.update(row_scale=G.wide(rs, 3 * M), rs_ld=3)
    if "row_zero" in on:
        z = (rs.rand(M) < 0.3).astype(np.uint8)
        z[M - 1] = 1
        d["row_zero"] = z
    if "relu_src" in on:
        m = G.wide(rs, M, N + 1)
        m.reshape(-1)[::3] = 0.0
        m.reshape(-1)[1::5] = -0.0
        d.update(relu_src=m, relu_ld=N + 1)
    if m_dev is not None:
        d["m_dev"] = np.array([m_dev], np.int32)
    return d


F32_FEATURES = ["a_idx0", "a_idx1", "b_idx", "bias", "row_scale", "row_zero", "relu", "relu_src", "accumulate"]


@pytest.mark.parametrize("vec", ["float4", "pointer+1", "odd_ld"])
@pytest.mark.parametrize("akm,bkm", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_f32_kernel_layouts_and_vector_loads(akm, bkm, vec):
    """gemm_f32_kernel in all four operand layouts, with float4 loads and without (an operand pointer one float off, or an
    odd leading dimension); k-major A without a split-K workspace.  32-row tiles (fewer than 400 tiles of 128 x 176) for the
    row-major A, 128-row tiles for the k-major one."""
    rs = np.random.RandomState(4 * akm + 2 * bkm + len(vec))
    for M, N, K in ((76, 200, 68), (1, 4, 4), (132, 180, 36)):
        for on in ((), tuple(F32_FEATURES)):
            d = f32_problem(rs, M, N, K, akm, bkm, on, pad=3 if vec == "odd_ld" else 4, K1=(40 if on and not akm else 0))
            got, kinds, plan = launch_gemm(d, mis=("A0", "B0") if vec == "pointer+1" else (), form="f32_128" if akm else "f32_32")
            assert kinds == {plan["kind"]: 1} and plan["kind"] == ("gemm_tn" if akm else ("gemm_nn" if bkm else "gemm_nt")), kinds
            assert plan["vec"] == (vec == "float4" and K % 4 == 0 and (not akm or M % 4 == 0) and (not bkm or N % 4 == 0))
            check_f32(d, got)


@pytest.mark.parametrize("bkm", [0, 1])
def test_f32_kernel_128_row_tiles(bkm):
    """400 or more tiles of 128 x 176 select the 128-row tile for a row-major A; the last row tile holds 5 rows."""
    rs = np.random.RandomState(23 + bkm)
    M, N, K = 128 * 200 + 5, 352, 36
    d = f32_problem(rs, M, N, K, 0, bkm, ("bias", "relu", "accumulate"))
    got, kinds, _ = launch_gemm(d, form="f32_128")
    assert kinds == {"gemm_nn" if bkm else "gemm_nt": 1}, kinds
    check_f32(d, got, big=True)


@pytest.mark.parametrize("akm", [0, 1])
def test_f32_kernel_device_side_extent(akm):
    """m_dev bounds the rows of a row-major A and the contraction extent of a k-major one."""
    rs = np.random.RandomState(29 + akm)
    M, N, K = 76, 180, 68
    for m_dev in ((0, 1, M - 1, M, M + 3) if not akm else (0, 1, 31, 33, K - 1, K, K + 3)):
        d = f32_problem(rs, M, N, K, akm, 1, ("bias", "accumulate") if not akm else ("accumulate",), m_dev=m_dev)
        got, kinds, _ = launch_gemm(d, form="f32_128" if akm else "f32_32")
        assert kinds == {"gemm_devm": 1}, kinds
        check_f32(d, got)


def test_f32_kernel_batched_with_the_strides_of_the_step():
    """batch = 3 with the element-stride patterns tgn.hip uses for its per-head products (H = 3 heads of dh columns, C context
    columns padded to Cp per head), and bias_bs / rs_bs."""
    rs = np.random.RandomState(31)
    H, dh, Cc, D = 3, 12, 52, 44
    E, Cp = H * dh, 56
    wk, wq, cq = G.wide(rs, E, Cc), G.wide(rs, E, E), G.wide(rs, E)
    cases = []
    # cqk_h = Wk_h^T cq_h: one row, A strided by dh inside one vector, B by dh rows, C by Cp inside one row
    cases.append(dict(A=(cq, None), lda=(E, 0), B=(wk, None), ldb=(Cc, 0), K=(dh, 0), M=1, N=Cc, b_kmajor=1, batch=H, a_bs=(dh, 0),
                      b_bs=(dh * Cc, 0), C=canary(H * Cp + 8), ldc=H * Cp, c_bs=Cp))
    # Wqk_h = Wk_h^T Wq_h[:, :D]: both operands k-major, every head its own Cp x D block
    cases.append(dict(A=(wk, None), lda=(Cc, 0), B=(wq, None), ldb=(E, 0), K=(dh, 0), M=Cc, N=D - 8, a_kmajor=1, b_kmajor=1, batch=H,
                      a_bs=(dh * Cc, 0), b_bs=(dh * E, 0), C=canary(H * Cp * D + 8), ldc=D, c_bs=Cp * D))
    # c_f = A^T t: one B shared by the heads (b_bs = 0), accumulate over a previous content
    tq, Aw = G.wide(rs, H * Cp), G.wide(rs, Cp, D)
    prev = canary(H * Cp + 8)
    prev[:H * Cp].reshape(H, Cp)[:, :D] = G.wide(rs, H, D)
    cases.append(dict(A=(tq, None), lda=(Cp, 0), B=(Aw, None), ldb=(D, 0), K=(Cp, 0), M=1, N=D, b_kmajor=1, batch=H, a_bs=(Cp, 0),
                      C=prev, ldc=D, c_bs=Cp, accumulate=1))
    # a batched nn.Linear with per-batch bias and row scale
    M, N, K = 37, 50, 20
    cases.append(dict(A=(G.wide(rs, H, M, K + 4), None), lda=(K + 4, 0), B=(G.wide(rs, H, N, K), None), ldb=(K, 0), K=(K, 0), M=M, N=N,
                      batch=H, a_bs=(M * (K + 4), 0), b_bs=(N * K, 0), C=canary(H * (M + 1) * (N + 3)), ldc=N + 3, c_bs=(M + 1) * (N + 3),
                      bias=G.wide(rs, H, N + 2), bias_bs=N + 2, row_scale=G.wide(rs, H, 3 * M + 1), rs_ld=3, rs_bs=3 * M + 1, relu=1))
    for d, (form, kind) in zip(cases, (("f32_32", "gemm_nn"), ("f32_128", "gemm_tn"), ("f32_32", "gemm_nn"), ("f32_32", "gemm_nt"))):
        got, kinds, _ = launch_gemm(d, form=form)
        assert kinds == {kind: 1}, kinds
        check_f32(d, got)


def test_addend_without_an_image_is_refused():
    """add_src lives in the image kernels' epilogue only: the launcher refuses the launches that would drop it."""
    rs = np.random.RandomState(37)
    d = img_problem(rs, 33, 64, 36, 0, ("add_src",))
    for kw in (dict(img=False), dict(img=True, mis=("A0",))):
        b = Bufs()
        g, read = fill_gemm_desc(b, d, **kw)
        with pytest.raises(_lib.PfoError, match="add_src"):
            _lib.call("pfo_debug_gemm", C.byref(g), _lib.stream_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(bits(read()), bits(d["C"]))
    b = Bufs()
    lst = (_lib.GemmDesc * 1)(fill_gemm_desc(b, d)[0])
    with pytest.raises(_lib.PfoError, match="plain problems"):
        _lib.call("pfo_debug_gemm_multi", lst, 1, _lib.stream_ptr())


def test_gathers_the_layout_does_not_read_are_refused():
    """b_idx gathers the k rows of a k-major B (and a weight image is built from the ungathered operand); a_idx gathers the
    rows of a row-major A.  Anywhere else the launchers refuse them."""
    rs = np.random.RandomState(39)
    idx = np.arange(68, dtype=np.int32)
    cases = [(dict(f32_problem(rs, 76, 64, 68, 0, 0), b_idx=idx), {}, "b_idx"),
             (dict(img_problem(rs, 33, 64, 68, 0, ("b_kmajor",)), b_idx=idx), dict(img=True, bx_force=2), "b_idx"),
             (dict(f32_problem(rs, 76, 64, 68, 1, 1), a_idx=[np.arange(76, dtype=np.int32), None]), {}, "a_idx")]
    for d, kw, word in cases:
        b = Bufs()
        g, read = fill_gemm_desc(b, d, **kw)
        with pytest.raises(_lib.PfoError, match=word):
            _lib.call("pfo_debug_gemm", C.byref(g), _lib.stream_ptr())
        if not kw:
            with pytest.raises(_lib.PfoError, match="gather"):
                _lib.call("pfo_debug_gemm_multi", (_lib.GemmDesc * 1)(g), 1, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(bits(read()), bits(d["C"]))


# ------------------------------------------------------------------------------------------------ several problems in one launch
def multi_case(rs, n, all_vec):
    """n problems whose outputs lie back to back in ONE buffer (ldc = N, no gap between neighbours)."""
    sizes = [(1, 1, 5), (31, 63, 32), (33, 65, 70), (32, 64, 36), (36, 68, 8), (4, 8, 100)]
    probs, off = [], 0
    for i in range(n):
        layout = i % 4
        akm, bkm = layout >> 1, layout & 1
        M, N, K = sizes[i % len(sizes)]
        if all_vec:                                                    # every problem eligible for float4 loads
            K = cdiv(K, 4) * 4
            if akm:
                M = cdiv(M, 4) * 4
            if bkm:
                N = cdiv(N, 4) * 4
        batch = 2 if i == 2 else 1
        pad = 4 if (all_vec or i != 1) else 3                          # problem 1: an odd leading dimension
        d = f32_problem(rs, M, N, K, akm, bkm, ("bias", "relu") if i % 3 == 0 else (("accumulate",) if i % 3 == 1 else ()), pad=pad)
        if batch > 1:
            for key in ("A", "B"):
                d[key] = [np.stack([d[key][0], G.wide(rs, *d[key][0].shape)]), None]
            d.update(batch=2, a_bs=(d["A"][0][0].size, 0), b_bs=(d["B"][0][0].size, 0), c_bs=M * N)
        keep = d["C"][:M, :N].copy()
        d["C"] = np.concatenate([keep.reshape(-1)] * batch) if d["accumulate"] else canary(M * N * batch)
        d["ldc"] = N
        d["off"] = off
        off += M * N * batch
        probs.append(d)
    return probs, off


@pytest.mark.parametrize("n,all_vec", [(1, True), (10, True), (10, False), (11, False)])
def test_multi_launch(n, all_vec):
    """pfo_gemm_multi_launch: 1, 10 and 11 problems (the eleventh spills into a second launch), the four layouts mixed, one
    problem that rules float4 loads out for the whole launch, one with batch 2, sizes around the 32 x 64 tile, outputs adjacent
    in one buffer."""
    rs = np.random.RandomState(41 + n)
    probs, total = multi_case(rs, n, all_vec)
    b = Bufs()
    whole = np.concatenate([np.asarray(d["C"], np.float32).reshape(-1) for d in probs] + [canary(64)])
    base = b.put(whole, np.float32)
    c_t = b.keep[-1]
    lst = (_lib.GemmDesc * n)()
    for i, d in enumerate(probs):
        off = d.pop("off")
        g, _ = fill_gemm_desc(b, d)
        g.C = base + 4 * off
        lst[i] = g
        d["off"] = off
    with profiled() as p:
        _lib.call("pfo_debug_gemm_multi", lst, n, _lib.stream_ptr())
        torch.cuda.synchronize()
    assert p.kinds == {"gemm_multi": cdiv(n, 10)}, p.kinds
    got = c_t[:whole.size].cpu().numpy()
    assert np.array_equal(bits(got[total:]), bits(whole[total:])), "the buffer behind the last output was touched"
    for d in probs:
        off = d.pop("off")
        check_f32(d, got[off:off + np.asarray(d["C"]).size])           # a spill into a neighbour shows as that neighbour's error


# ------------------------------------------------------------------------------------------------ grouped weight gradients
def tn_problem(rs, K, M, N, bias, gather, c_acc, b_acc):
    lda, ldb, ldc = M + 4, N + 4, N + 3
    Kb = K + (7 if gather else 0)
    C0 = canary((M + 2) * ldc).reshape(M + 2, ldc).copy()
    if c_acc:
        C0[:M, :N] = G.wide(rs, M, N)
    b0 = None
    if bias:
        b0 = canary(M + 5)
        if b_acc:
            b0[:M] = G.wide(rs, M)
    return dict(A=G.wide(rs, K, lda), lda=lda, B=G.wide(rs, Kb, ldb), ldb=ldb, b_idx=rs.permutation(Kb)[:K].astype(np.int32) if gather else None,
                M=M, N=N, C=C0, ldc=ldc, c_accumulate=c_acc, bias_out=b0, bias_accumulate=b_acc)


def launch_tn(probs, K, k_dev=None, mis=False, slab_floats=None, form=None):
    """-> (outputs, the profiler families that ran, the launcher's plan); the plan (pfo_debug_gemm_tn_group_plan: the function
    pfo_gemm_tn_group_launch itself switches on) is asked before the launch, held to the model of tests/gemm_ref.py on these
    very descriptors, ``form`` asserted, and the slabs sized from its nsplit."""
    b = Bufs()
    n = len(probs)
    lst = (_lib.TnDesc * n)()
    outs = []
    for i, q in enumerate(probs):
        lst[i] = _lib.TnDesc(A=b.put(q["A"], np.float32, 1 if (mis and i == 0) else 0), lda=q["lda"], B=b.put(q["B"], np.float32), ldb=q["ldb"],
                             b_idx=b.put(q["b_idx"], np.int32), M=q["M"], N=q["N"], c_accumulate=q["c_accumulate"],
                             bias_accumulate=q["bias_accumulate"], ldc=q["ldc"])
        lst[i].C = b.put(q["C"], np.float32)
        ct = b.keep[-1]
        bt = None
        if q["bias_out"] is not None:
            lst[i].bias_out = b.put(q["bias_out"], np.float32)
            bt = b.keep[-1]
        outs.append((ct, bt))
    per_split = sum(q["M"] * (q["N"] + (q["bias_out"] is not None)) for q in probs)
    plan = _lib.gemm_plan("pfo_debug_gemm_tn_group_plan", lst, n, K, 1 << 40)
    ref = G.tn_plan_ref(list(lst), K)
    assert plan == {k: ref[k] for k in plan}, (plan, ref)
    assert form is None or plan["form"] == form, (plan["form"], form)
    need = per_split * plan["nsplit"]
    assert need == ref["need"]
    slabs = b.put(np.zeros(need, np.float32), np.float32)
    kd = b.put(None if k_dev is None else np.array([k_dev], np.int32), np.int32)
    with profiled() as p:
        _lib.call("pfo_debug_gemm_tn_group", lst, n, K, kd, slabs, need if slab_floats is None else slab_floats, _lib.stream_ptr())
        torch.cuda.synchronize()
    res = []
    for q, (ct, bt) in zip(probs, outs):
        res.append((ct[:q["C"].size].cpu().numpy(), None if bt is None else bt[:q["bias_out"].size].cpu().numpy()))
    return res, p.kinds, plan


# form -> (its profiler family, the columns of A one workgroup tile takes and keeps one scale for; None: exact fp32, no scale)
TN_FORMS = {"tn_bx8": ("gemm_tn_bx8", 256), "tn_bx": ("gemm_tn_bx", 128), "tn_f32": ("gemm_tn", None)}
FORM_OF = {kind: form for form, (kind, _) in TN_FORMS.items()}


def check_tn(probs, K, k_dev, res, kinds, plan):
    kind, a_block = TN_FORMS[plan["form"]]
    assert kind == plan["kind"]
    assert kinds == ({kind: 1, "tn_reduce": 1} if kind != "gemm_tn" else {kind: 1}), kinds
    ref = G.tn_group_ref(probs, K, None if k_dev is None else np.array([k_dev]), a_block=a_block)
    for q, r, (gc, gb) in zip(probs, ref, res):
        wr = r["C_written"]
        assert np.array_equal(bits(gc)[~wr], bits(q["C"])[~wr]), "padding of a gradient touched"
        ok, worst = within(gc[wr], r["C"][wr], r["C_mag"][wr], TOL)
        assert ok, "dW: worst |got - ref| / mag = %.3g" % worst
        if gb is not None:
            M = q["M"]
            assert np.array_equal(bits(gb)[M:], bits(q["bias_out"])[M:]), "the bias gradient's tail touched"
            ok, worst = within(gb[:M], r["bias"][:M], r["bias_mag"][:M], TOL)
            assert ok, "bias gradient: worst |got - ref| / mag = %.3g" % worst


# per form: (M, N) of up to 16 problems.  gemm_tn_bx8: every M >= 500 and all float4-eligible; gemm_tn_bx: one M < 500;
# gemm_tn (plain fp32): one M or N that is no multiple of 4 (N = 175 and 177 live here), or a misaligned pointer
TN_SHAPES = {
    "gemm_tn_bx8": [(500, 176), (504, 36), (512, 180), (500, 4)] + [(500 + 4 * i, 8 + 4 * i) for i in range(12)],
    "gemm_tn_bx": [(172, 176), (500, 36), (8, 348), (128, 172)] + [(4 + 12 * i, 180 - 8 * i) for i in range(12)],
    "gemm_tn": [(173, 177), (30, 175), (64, 176), (1, 1)] + [(3 + 11 * i, 179 - 7 * i) for i in range(12)],
}


def tn_group(rs, form, n, K):
    return [tn_problem(rs, K, M, N, bias=i % 2 == 0, gather=i % 3 == 1, c_acc=int(i % 4 < 2), b_acc=int(i % 4 in (0, 3)))
            for i, (M, N) in enumerate(TN_SHAPES[form][:n])]


@pytest.mark.parametrize("n", [1, 3, 16])
@pytest.mark.parametrize("form", ["gemm_tn_bx8", "gemm_tn_bx", "gemm_tn"])
def test_grouped_weight_gradients(form, n):
    """n problems sharing K = 333 (no multiple of 32) and K = 100 (a single slab): different M and N, N = 176 with the bias
    column crossing the 176-column block, gathered B rows, both accumulate flags over a non-zero content; bit-identical between
    two launches."""
    rs = np.random.RandomState(43 + n)
    for K in (333, 100):
        probs = tn_group(rs, form, n, K)
        res, kinds, plan = launch_tn(probs, K, form=FORM_OF[form])
        assert plan["kind"] == form
        check_tn(probs, K, None, res, kinds, plan)
        again, _, _ = launch_tn(probs, K)
        for (c1, b1), (c2, b2) in zip(res, again):
            assert np.array_equal(bits(c1), bits(c2)) and (b1 is None or np.array_equal(bits(b1), bits(b2)))


@pytest.mark.parametrize("form", ["gemm_tn_bx8", "gemm_tn_bx", "gemm_tn"])
def test_grouped_weight_gradients_device_side_extent(form):
    rs = np.random.RandomState(47)
    K = 333
    probs = tn_group(rs, form, 3, K)
    for k_dev in (0, 1, 31, 33, K - 1, K, K + 9):
        res, kinds, plan = launch_tn(probs, K, k_dev, form=FORM_OF[form])
        check_tn(probs, K, k_dev, res, kinds, plan)


def test_grouped_weight_gradients_both_bias_settings_at_the_block_edge():
    """N in {175, 176, 177} with and without the bias column (N + 1 crosses the 176-column block), no accumulation."""
    rs = np.random.RandomState(53)
    K = 96
    for N in (175, 176, 177):
        for bias in (False, True):
            for M in (172, 504):
                probs = [tn_problem(rs, K, M, N, bias=bias, gather=False, c_acc=0, b_acc=0)]
                res, kinds, plan = launch_tn(probs, K, form="tn_f32" if N != 176 else ("tn_bx8" if M == 504 else "tn_bx"))
                check_tn(probs, K, None, res, kinds, plan)


def test_grouped_weight_gradients_misaligned_pointer_takes_the_fp32_form():
    rs = np.random.RandomState(59)
    probs = tn_group(rs, "gemm_tn_bx", 3, 200)
    res, kinds, plan = launch_tn(probs, 200, mis=True, form="tn_f32")
    check_tn(probs, 200, None, res, kinds, plan)


def test_grouped_weight_gradients_small_workspace_is_refused():
    rs = np.random.RandomState(61)
    K = 333
    probs = tn_group(rs, "gemm_tn_bx", 3, K)
    per_split = sum(q["M"] * (q["N"] + (q["bias_out"] is not None)) for q in probs)
    with pytest.raises(_lib.PfoError, match="workspace too small"):
        launch_tn(probs, K, slab_floats=per_split - 1)
    # (launch_tn's buffers are gone with the exception: the refusal comes before any launch, which a second call that reads
    #  its outputs back shows)
    b = Bufs()
    q = probs[0]
    d = _lib.TnDesc(A=b.put(q["A"], np.float32), lda=q["lda"], B=b.put(q["B"], np.float32), ldb=q["ldb"], b_idx=b.put(q["b_idx"], np.int32),
                    M=q["M"], N=q["N"], c_accumulate=1, bias_accumulate=1, ldc=q["ldc"])
    d.C = b.put(q["C"], np.float32)
    ct = b.keep[-1]
    slabs = b.put(np.zeros(16, np.float32), np.float32)
    with pytest.raises(_lib.PfoError, match="workspace too small"):
        _lib.call("pfo_debug_gemm_tn_group", C.byref(d), 1, K, None, slabs, 16, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(bits(ct[:q["C"].size].cpu().numpy()), bits(q["C"]))


# ------------------------------------------------------------------------------------------------ the fused GRU
# Activation term of the gate outputs: the kernel's sigmoid and tanh go through the device's exp2 and reciprocal.
# MEASURED on an MI355X by test_gru_activation_error - not over the wide-range GRU cases, where the pre-activation bound hides
# it, but over twelve dedicated cases (every D, Ef and gather mode) on operands for which both contractions are exact, so that
# the whole error of r, z and n against float64 is this term: 4.979e-07 at most.  Asserted at four times that, 1.992e-06,
# there and as the per-activation addend of every GRU bound below; the step tests grant the memory 1e-4.
GRU_ACT_OBSERVED = 4.979e-07
GRU_ACT_BOUND = 4 * GRU_ACT_OBSERVED


def gru_weights(D, K_msg, scaled, seed):
    torch.manual_seed(seed)
    cell = torch.nn.GRUCell(K_msg, D)                                  # the project's initialiser for the memory updater
    W_ih, W_hh, b_ih, b_hh = (p.detach().numpy().copy() for p in (cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh))
    if scaled:                                                         # the two blocks 2^9 apart (tests/test_gpu_tgn_step.py)
        W_ih *= 2.0 ** 3
        W_hh *= 2.0 ** -6
    return W_ih, W_hh, b_ih, b_hh


class GruCase:
    def __init__(self, D, Ef, weights):
        self.D, self.K_msg = D, 3 * D + Ef
        self.W = weights
        self.b = Bufs()
        b = self.b
        W_ih, W_hh, b_ih, b_hh = weights
        self.p_bih, self.p_bhh = b.put(b_ih, np.float32), b.put(b_hh, np.float32)
        self.img = []
        for W, K, gate in ((W_ih, self.K_msg, 1), (W_hh, D, 2)):
            dst = b.raw(_lib.byte_count("pfo_debug_gru_img_bytes", D, K))
            d = _lib.BimgDesc(src=b.put(W, np.float32), ld=K, N=3 * D, K=K, trans=0, dst=dst, gate=gate, gate_D=D)
            _lib.call("pfo_debug_bimg", C.byref(d), 1, _lib.stream_ptr())
            self.img.append(dst)

    def run(self, msg, h, hm, touched, node_feat, cap, n_rows):
        """-> (upd_mem, h0_tab, gates) as [cap + 2, .] arrays, canary where not written, and the families that ran"""
        b, D = Bufs(), self.D
        outs = [canary((cap + 2) * w) for w in (D, D, 4 * D)]
        f = _lib.GruDesc(msg_rows=b.put(msg, np.float32), K_msg=self.K_msg, h_rows=b.put(h, np.float32), img_ih=self.img[0],
                         img_hh=self.img[1], b_ih=self.p_bih, b_hh=self.p_bhh, hm=b.put(hm, np.uint8), touched=b.put(touched, np.int32),
                         node_feat=b.put(node_feat, np.float32), D=D, cap_rows=cap, n_rows=b.put(np.array([n_rows], np.int32), np.int32),
                         gather=self.gather)
        ts = []
        for name, o in zip(("upd_mem", "h0_tab", "gates"), outs):
            setattr(f, name, b.put(o, np.float32))
            ts.append(b.keep[-1])
        with profiled() as p:
            _lib.call("pfo_debug_gru_fused", C.byref(f), _lib.stream_ptr())
            torch.cuda.synchronize()
        return [t[:o.size].cpu().numpy().reshape(cap + 2, -1) for t, o in zip(ts, outs)], outs, p.kinds


def gru_operands(rs, D, K_msg, cap, gather, make):
    nodes = cap + 37
    touched = np.sort(rs.permutation(nodes)[:cap]).astype(np.int32)   # a subset of the nodes: gaps ...
    rs.shuffle(touched)                                                # ... in no order
    rows = nodes if gather else cap
    hm = (rs.rand(rows) < 0.7).astype(np.uint8)
    hm[touched[0] if gather else 0] = 0
    return make(rows, K_msg), make(rows, D), hm, touched, make(nodes, D)


def gru_bounds(r, nf_rows):
    """Per-element bounds of the three outputs: every pre-activation within 4e-6 of its magnitude sum (the image kernels'
    bound), carried through the gates with the Lipschitz constants 1/4 (sigmoid) and 1 (tanh), plus the fp32 roundings of the
    gate arithmetic and the measured activation term GRU_ACT_BOUND per activation."""
    D = r["h"].shape[1]
    e, u = TOL, 2.0 ** -23
    mr, mz, mi, mh = (r["pre_mag"][:, i * D:(i + 1) * D] for i in range(4))
    g = r["gates"]
    rr, zz, nn, ghn = (g[:, i * D:(i + 1) * D] for i in range(4))
    gin = r["pre"][:, 2 * D:3 * D]
    d_r, d_z, d_gh = e * mr / 4 + GRU_ACT_BOUND, e * mz / 4 + GRU_ACT_BOUND, e * mh
    d_arg = e * mi + np.abs(rr) * d_gh + np.abs(ghn) * d_r + d_r * d_gh + 2 * u * (np.abs(gin) + np.abs(rr * ghn))
    d_n = d_arg + GRU_ACT_BOUND
    hh = np.abs(r["h"])
    d_h = (1 - zz) * d_n + (np.abs(nn) + hh) * d_z + d_z * d_n + 4 * u * (np.abs(nn) + hh)
    d_h = np.where(r["has"][:, None], d_h, 0.0)                        # no pending message: the row is kept bit for bit
    d_h0 = d_h + u * (np.abs(r["upd_mem"]) + np.abs(nf_rows))
    return d_h, d_h0, np.concatenate([d_r, d_z, d_n, d_gh], 1)


@pytest.mark.parametrize("scaled", [False, True], ids=["init", "blocks_2^9_apart"])
@pytest.mark.parametrize("gather", [0, 1])
@pytest.mark.parametrize("Ef", [4, 8])
@pytest.mark.parametrize("D", [32, 100, 172])
def test_gru_fused(D, Ef, gather, scaled):
    """pfo_gru_fused_launch against the float64 cell: cap_rows in {1, 129, 300}, n_rows in {0, 1, cap - 1, cap}, packed rows
    and per-node tables, rows without a pending message."""
    rs = np.random.RandomState(D + Ef + 2 * gather + scaled)
    case = GruCase(D, Ef, gru_weights(D, 3 * D + Ef, scaled, seed=D + Ef))
    case.gather = gather
    for cap in (1, 129, 300):
        msg, h, hm, touched, nf = gru_operands(rs, D, case.K_msg, cap, gather, lambda *s: 0.05 * G.wide(rs, *s))
        for n_rows in sorted({0, 1, cap - 1, cap}):
            (upd, h0, gates), canaries, kinds = case.run(msg, h, hm, touched, nf, cap, n_rows)
            assert kinds == {"gru_fused": 1}, kinds
            for got, can in zip((upd, h0, gates), canaries):
                assert np.array_equal(bits(got[n_rows:]), bits(can.reshape(got.shape)[n_rows:])), "rows >= n_rows touched"
            r = G.gru_ref(msg, h, *case.W, hm, touched, nf, n_rows, gather)
            b_h, b_h0, b_g = gru_bounds(r, nf.astype(f64)[touched[:n_rows]])
            for name, got, ref, bound in (("gates", gates, r["gates"], b_g), ("upd_mem", upd, r["upd_mem"], b_h), ("h0_tab", h0, r["h0_tab"], b_h0)):
                diff = np.abs(got[:n_rows].astype(f64) - ref)
                assert np.isfinite(got[:n_rows]).all() and (diff <= bound).all(), (name, float((diff - bound).max()))
            keep = ~r["has"]
            sel = (touched[:n_rows] if gather else np.arange(n_rows))[keep]
            assert np.array_equal(bits(upd[:n_rows][keep]), bits(h[sel])), "a row without a message must keep h bit for bit"
            if n_rows > 1:
                assert keep.any() and r["has"].any()


def test_gru_activation_error():
    """The activation term alone: operands on a coarse binary grid, so that every product and every partial sum of the two
    contractions is exact in the split format and in fp32 (asserted on gh_n, which leaves the kernel as it is) - what is left
    of the gates' error against float64 is the device's exp2 / reciprocal and the fp32 gate arithmetic.  Observed maximum on
    an MI355X over every D, Ef and gather mode and the bound the other GRU tests add per activation: GRU_ACT_OBSERVED,
    GRU_ACT_BOUND = 4 x that; the step tests grant the memory 1e-4."""
    worst, hi, lo = 0.0, 0.0, 1e9
    for D, Ef, gather in itertools.product((32, 100, 172), (4, 8), (0, 1)):
        rs = np.random.RandomState(D + Ef + gather)
        K_msg = 3 * D + Ef
        grid = lambda lo, hi, q: (lambda *s: (rs.randint(lo, hi + 1, size=s) / q).astype(np.float32))
        W = (grid(-4, 4, 8.0)(3 * D, K_msg), grid(-4, 4, 8.0)(3 * D, D), grid(-8, 8, 32.0)(3 * D), grid(-8, 8, 32.0)(3 * D))
        case = GruCase(D, Ef, W)
        case.gather = gather
        cap = 300
        msg, h, hm, touched, nf = gru_operands(rs, D, K_msg, cap, gather, grid(-3, 3, 4.0))
        (upd, h0, gates), _, kinds = case.run(msg, h, hm, touched, nf, cap, cap)
        assert kinds == {"gru_fused": 1}
        r = G.gru_ref(msg, h, *W, hm, touched, nf, cap, gather)
        assert np.array_equal(gates[:cap, 3 * D:].astype(f64), r["gates"][:, 3 * D:]), "the contraction is not exact on the grid"
        hi, lo = max(hi, np.abs(r["pre"]).max()), min(lo, np.abs(r["pre"]).min())
        worst = max(worst, float(np.abs(gates[:cap, :3 * D].astype(f64) - r["gates"][:, :3 * D]).max()))
    assert hi > 8 and lo < 0.25                                        # saturated and linear arguments both occur
    print("GRU activation error, observed maximum: %.3e" % worst)
    assert worst < 1e-4                                                # the memory's tolerance in the step tests: else a finding
    assert worst <= GRU_ACT_BOUND, worst                               # observed 4.979e-07; bound 4 x that = 1.992e-06


# ------------------------------------------------------------------------------------------------ rank-1 updates and slab sums
@pytest.mark.parametrize("n", [1, 12])
def test_rank1_multi(n):
    """out += sum_r u_r (x) v_r: up to 12 updates in one launch, strided vectors, reps > 1; to a few fp32 ulp of sum |terms|
    (reps fused multiply-adds and one addition: reps + 1 roundings of half an ulp, bound at (reps + 2) * 2^-24)."""
    rs = np.random.RandomState(67 + n)
    b = Bufs()
    lst = (_lib.Rank1Desc * n)()
    cases = []
    for i in range(n):
        M, N, reps = [(1, 1, 1), (37, 65, 3), (172, 5, 2), (3, 300, 1)][i % 4]
        ldu, ldv, ldo = 1 + i % 3, 1 + (i + 1) % 2, N + 2
        u_rs, v_rs = M * ldu + 3, N * ldv + 1
        u, v = G.wide(rs, reps * u_rs), G.wide(rs, reps * v_rs)
        out = canary((M + 1) * ldo).reshape(M + 1, ldo).copy()
        out[:M, :N] = G.wide(rs, M, N)
        lst[i] = _lib.Rank1Desc(u=b.put(u, np.float32), ldu=ldu, v=b.put(v, np.float32), ldv=ldv, M=M, N=N, ldo=ldo, reps=reps, u_rs=u_rs, v_rs=v_rs)
        lst[i].out = b.put(out, np.float32)
        cases.append((b.keep[-1], (u, ldu, v, ldv, M, N, out, ldo, reps, u_rs, v_rs)))
    _lib.call("pfo_debug_rank1_multi", lst, n, _lib.stream_ptr())
    torch.cuda.synchronize()
    for t, args in cases:
        out, reps = args[6], args[8]
        got = t[:out.size].cpu().numpy()
        ref, mag, wr = G.rank1_ref(*args)
        assert np.array_equal(bits(got)[~wr], bits(out)[~wr])
        ok, worst = within(got[wr], ref[wr], mag[wr], (reps + 2) * 2.0 ** -24)
        assert ok, worst
    with pytest.raises(_lib.PfoError):
        _lib.call("pfo_debug_rank1_multi", (_lib.Rank1Desc * 13)(), 13, _lib.stream_ptr())


@pytest.mark.parametrize("n", [1, 4])
def test_sum_slabs(n):
    """dst (+)= sum of n_slabs slabs, up to 4 destinations in one launch, in a fixed order: n_slabs roundings of half an ulp
    of sum |terms|, bound at (n_slabs + 1) * 2^-24; accumulate 0 and 1."""
    rs = np.random.RandomState(71 + n)
    b = Bufs()
    lst = (_lib.SumSlabsDesc * n)()
    cases = []
    for i in range(n):
        count, ns, acc = [(1, 1, 0), (1000, 7, 1), (257, 3, 0), (70000, 2, 1)][i % 4]
        stride = count + 5
        src = G.wide(rs, ns * stride)
        dst = canary(count + 9)
        if acc:
            dst[:count] = G.wide(rs, count)
        lst[i] = _lib.SumSlabsDesc(src=b.put(src, np.float32), stride=stride, count=count, n_slabs=ns, accumulate=acc)
        lst[i].dst = b.put(dst, np.float32)
        cases.append((b.keep[-1], dst, src, stride, count, ns, acc))
    _lib.call("pfo_debug_sum_slabs", lst, n, _lib.stream_ptr())
    torch.cuda.synchronize()
    for t, dst, src, stride, count, ns, acc in cases:
        got = t[:dst.size].cpu().numpy()
        ref, mag, wr = G.sum_slabs_ref(dst, src, stride, count, ns, acc)
        assert np.array_equal(bits(got)[~wr], bits(dst)[~wr])
        ok, worst = within(got[wr], ref[wr], mag[wr], (ns + 1) * 2.0 ** -24)
        assert ok, worst
    with pytest.raises(_lib.PfoError):
        _lib.call("pfo_debug_sum_slabs", (_lib.SumSlabsDesc * 5)(), 5, _lib.stream_ptr())
