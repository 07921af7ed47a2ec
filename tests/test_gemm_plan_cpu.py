"""The contraction launchers' dispatch, held to its second statement on the CPU.

pfo_debug_gemm_plan / pfo_debug_gemm_tn_group_plan return what pfo_gemm_launch / pfo_gemm_tn_group_launch decide before they
touch the device (gemm.hip gemm_plan / tn_group_plan: the function the launchers switch on) - pure host code, so the library
answers without a GPU.  tests/gemm_ref.py states the same rule independently (gemm_plan_ref / tn_plan_ref); the sweeps below
sit on every threshold of it and assert query == model field by field, refusals with a word of the launcher's message.
Pointers are 1 << 12 (aligned), + 4 (misaligned) or null and are never followed."""
import ctypes as C
import itertools

import pytest

from pfotgnrec_amd import _lib
import gemm_ref as G

P = 1 << 12
FIELDS = _lib.GEMM_PLAN_FIELDS
SINGLE_FORMS = {"f32_128", "f32_32", "skinny4", "skinny11", "areg", "areg8", "astat", "tn_group"}
TN_FORMS = {"tn_f32", "tn_bx", "tn_bx8"}
ARRAYS = ("A", "B", "lda", "ldb", "a_idx", "K", "a_bs", "b_bs")


def up4(x):
    return G.cdiv(x, 4) * 4


def gdesc(M, N, K0, K1=0, img=0, **kw):
    """A GemmDesc whose operands admit float4 loads whenever their extents do (aligned pointers, leading dimensions the extent
    rounded up to 4, plus 4); ``img``: 1 = b_img, 2 = b_img and b_img2; keywords set any field afterwards, "A0" / "lda1" the
    array ones."""
    g = _lib.GemmDesc(M=M, N=N, batch=1, C=P, ldc=N + 4, rs_ld=1)
    akm, bkm = kw.get("a_kmajor", 0), kw.get("b_kmajor", 0)
    for s, K in enumerate((K0, K1)):
        g.K[s] = K
        if K:
            g.A[s], g.B[s] = P, P
            g.lda[s], g.ldb[s] = up4(M if akm else K) + 4, up4(N if bkm else K) + 4
    if img:
        g.b_img = P
    if img == 2:
        g.b_img2 = P
    for k, v in kw.items():
        if k[:-1] in ARRAYS and k[-1] in "01":
            getattr(g, k[:-1])[int(k[-1])] = v
        else:
            setattr(g, k, v)
    return g


def check_gemm(g, seen):
    """query == model for one descriptor; notes the form (or the refusal's word) in ``seen``."""
    lib = _lib.load()
    try:
        ref = G.gemm_plan_ref(g)
    except G.PlanRefused as e:
        out = (C.c_int32 * len(FIELDS))()
        assert lib.pfo_debug_gemm_plan(C.byref(g), out) == -1, "the model refuses (%s), the library does not" % e
        assert str(e).encode() in lib.pfo_last_error(), (str(e), lib.pfo_last_error())
        seen.add("refused: %s" % e)
        return
    got = _lib.gemm_plan("pfo_debug_gemm_plan", C.byref(g))
    assert got == {k: ref[k] for k in FIELDS}, (got, ref)
    seen.add(got["form"])


def single_sweep():
    """The descriptors of the single-launch sweep, one at a time."""
    # tile counts (row tiles x column tiles x batch) 399 / 400 and 511 / 512 with one, two, three and seven column tiles; skinny
    # block counts (32-row x 176-column) 511 / 512; row counts around the A-stationary form's 32 768
    Ms = sorted({1, 33, 128, 129, 128 * 57, 128 * 57 + 1, 128 * 73, 128 * 73 + 1, 128 * 133, 128 * 133 + 1, 32 * 255, 32 * 255 + 1, 32 * 256 + 1,
                 32 * 511, 32 * 511 + 1, 128 * 199 + 1, 128 * 200, 128 * 200 + 1, 32767, 32768, 128 * 256 + 5, 128 * 399, 128 * 399 + 1, 128 * 400 + 1,
                 128 * 511, 128 * 511 + 1})
    Ns = (64, 172, 176, 177, 320, 352, 368, 1024, 1056, 176 * 7)
    modes = ((0, 0), (1, 0), (2, 0), (2, 1), (2, 2))                   # (img, bx_force)
    for M, N, K0, K1, (img, force), bkm in itertools.product(Ms, Ns, (36, 192, 193), (0, 36), modes, (0, 1)):
        yield gdesc(M, N, K0, K1, img=img, bx_force=force, b_kmajor=bkm)
    # batch 3: never an image launch; 3 x 133 = 399 and 3 x 134 = 402 tiles
    for M, N, img, bkm, m_dev in itertools.product((77, 128 * 133, 128 * 133 + 1, 128 * 171), (176, 352), (0, 1), (0, 1), (None, P)):
        yield gdesc(M, N, 36, img=img, b_kmajor=bkm, batch=3, a_bs0=M * 40, b_bs0=N * 40, c_bs=M * (N + 4), m_dev=m_dev)
    # the A-stationary form's window: K[0] 192 / 193, N 320 / 352 / 368 / 1024 / 1056, M 32 767 / 32 768, and everything that
    # rules it out one at a time
    outs = [{}, dict(ldc=355), dict(C=P + 4), dict(K1=36)] + [{f: P} for f in ("bias", "relu_src", "add_src", "row_scale", "row_zero")] + \
           [dict(relu=1), dict(accumulate=1), dict(bias=P, row_scale=P)]
    for M, N, K0, out in itertools.product((32767, 32768, 128 * 256 + 5), (320, 352, 368, 1024, 1056), (44, 192, 193), outs):
        out = dict(out)
        yield gdesc(M, N, K0, out.pop("K1", 0), img=2, **out)
    # an A that rules float4 loads out beside an image: the fp32 kernel - refused with add_src, and with two weight images
    for M, img, K1, bad, add in itertools.product((77, 128 * 400 + 1), (1, 2), (0, 36), (dict(A0=P + 4), dict(lda0=39), dict(K0=34), dict(A1=P + 4)), (None, P)):
        kw = dict(bad)
        yield gdesc(M, 352, kw.pop("K0", 36), K1, img=img, add_src=add, **kw)
    # gathers: b_idx with either B layout, with and without an image launch; a_idx with a row-major A
    for img, bkm, b_idx, a_idx in itertools.product((0, 1), (0, 1), (None, P), (None, P)):
        yield gdesc(300, 172, 36, img=img, b_kmajor=bkm, b_idx=b_idx, a_idx0=a_idx)
    # k-major A: K 128 / 129 / 256 / 257 (where nsplit moves) and long; tm x tn x batch around 512 (512 / tiles: 2, 1, 1); with
    # and without slabs, a k-major B, batch 3, an epilogue, a device-side extent, a second source, a gather
    shapes = ((4, 8), (128, 176), (132, 180), (1000, 700), (128 * 32, 176 * 16), (128 * 73, 176 * 7), (128 * 27, 176 * 19), (128 * 16, 176 * 16), (129, 177))
    extra = [{}, dict(bias=P), dict(relu=1), dict(row_zero=P), dict(relu_src=P), dict(accumulate=1), dict(m_dev=P), dict(K1=36), dict(a_idx0=P),
             dict(a_idx1=P), dict(A0=P + 4), dict(b_idx=P)]
    for (M, N), K0, slabs, bkm, batch, kw in itertools.product(shapes, (100, 128, 129, 256, 257, 1000, 53760), (None, P), (0, 1), (1, 3), extra):
        kw = dict(kw)
        yield gdesc(M, N, K0, kw.pop("K1", 0), a_kmajor=1, b_kmajor=bkm, slabs=slabs, slab_floats=1 << 40, batch=batch, **kw)


def test_single_launch_plan_follows_the_model_on_every_threshold():
    seen, count = set(), 0
    for g in single_sweep():
        check_gemm(g, seen)
        count += 1
    assert SINGLE_FORMS <= seen, SINGLE_FORMS - seen
    words = {"b_idx", "a_idx", "add_src", "one source", "split-K with batch", "no epilogue", "two-source"}
    assert {"refused: " + w for w in words} <= seen, seen
    assert count > 5000


def gemm_refusals():
    """(id, descriptor, a word of the message): every refusal of pfo_gemm_launch."""
    return [
        ("no-rows", gdesc(0, 64, 36), "bad sizes"),
        ("no-columns", gdesc(33, 0, 36), "bad sizes"),
        ("no-extent", gdesc(33, 64, 0, A0=P, B0=P), "bad sizes"),
        ("no-batch", gdesc(33, 64, 36, batch=0), "bad sizes"),
        ("null-A", gdesc(33, 64, 36, A0=None), "null operand"),
        ("null-B", gdesc(33, 64, 36, B0=None), "null operand"),
        ("null-C", gdesc(33, 64, 36, C=None), "null operand"),
        ("null-second-A", gdesc(33, 64, 36, 36, A1=None), "source 2"),
        ("null-second-B", gdesc(33, 64, 36, 36, B1=None), "source 2"),
        ("b_idx-row-major-B", gdesc(33, 64, 36, b_idx=P), "b_idx needs"),
        ("b_idx-image", gdesc(33, 64, 36, img=1, b_kmajor=1, b_idx=P), "b_idx needs"),
        ("a_idx-k-major-A", gdesc(64, 64, 36, a_kmajor=1, a_idx0=P), "a_idx needs"),
        ("add_src-no-image", gdesc(33, 64, 36, add_src=P), "add_src needs"),
        ("add_src-misaligned-A", gdesc(33, 64, 36, img=1, add_src=P, A0=P + 4), "add_src needs"),
        ("add_src-odd-lda", gdesc(33, 64, 36, img=1, add_src=P, lda0=39), "add_src needs"),
        ("add_src-batch", gdesc(33, 64, 36, img=1, add_src=P, batch=2), "add_src needs"),
        ("k-major-two-sources", gdesc(64, 64, 36, 36, a_kmajor=1), "one source"),
        ("split-k-batch", gdesc(64, 64, 1000, a_kmajor=1, b_kmajor=1, slabs=P, batch=2), "split-K with batch"),
        ("split-k-bias", gdesc(64, 64, 1000, a_kmajor=1, b_kmajor=1, slabs=P, bias=P), "no epilogue"),
        ("split-k-relu", gdesc(64, 64, 1000, a_kmajor=1, b_kmajor=1, slabs=P, relu=1), "no epilogue"),
        ("two-images-misaligned-A", gdesc(33, 64, 36, 36, img=2, A1=P + 4), "two-source launch with weight images"),
        ("two-images-batch", gdesc(33, 64, 36, 36, img=2, batch=2), "two-source launch with weight images"),
    ]


@pytest.mark.parametrize("cid,g,word", gemm_refusals(), ids=[c[0] for c in gemm_refusals()])
def test_gemm_launch_refusals(cid, g, word):
    """The query answers -1 with the launcher's message, the model refuses with the same word, and the launcher itself - which
    plans before it touches the device - refuses the same way without a GPU."""
    lib = _lib.load()
    out = (C.c_int32 * len(FIELDS))()
    assert lib.pfo_debug_gemm_plan(C.byref(g), out) == -1
    assert word.encode() in lib.pfo_last_error() and lib.pfo_last_error().startswith(b"pfo_gemm_launch: "), lib.pfo_last_error()
    with pytest.raises(G.PlanRefused) as e:
        G.gemm_plan_ref(g)
    assert str(e.value) in word
    with pytest.raises(_lib.PfoError, match=word):
        _lib.gemm_plan("pfo_debug_gemm_plan", C.byref(g))
    with pytest.raises(_lib.PfoError, match=word):
        _lib.call("pfo_debug_gemm", C.byref(g), None)


def test_plan_queries_refuse_null_arguments():
    lib = _lib.load()
    out = (C.c_int32 * len(FIELDS))()
    assert lib.pfo_debug_gemm_plan(None, out) == -1 and lib.pfo_debug_gemm_plan(C.byref(gdesc(33, 64, 36)), None) == -1
    one = (_lib.TnDesc * 1)(tdesc(8, 8))
    assert lib.pfo_debug_gemm_tn_group_plan(None, 1, 32, 1 << 40, out) == -1 and lib.pfo_debug_gemm_tn_group_plan(one, 1, 32, 1 << 40, None) == -1
    assert lib.pfo_debug_gemm_tn_group_plan((_lib.TnDesc * 17)(), 17, 32, 1 << 40, out) == -1 and b"bad problem list" in lib.pfo_last_error()
    assert lib.pfo_debug_gemm_tn_group_plan(one, 0, 32, 1 << 40, out) == -1
    assert lib.pfo_debug_gemm_tn_group_plan(one, 1, 0, 1 << 40, out) == -1 and b"pfo_gemm_tn_group_launch: bad arguments" in lib.pfo_last_error()
    for bad in (dict(A=None), dict(B=None), dict(C=None), dict(M=0), dict(N=0)):
        lst = (_lib.TnDesc * 2)(tdesc(8, 8), tdesc(8, 8, **bad))
        assert lib.pfo_debug_gemm_tn_group_plan(lst, 2, 32, 1 << 40, out) == -1 and b"bad problem" in lib.pfo_last_error()
        with pytest.raises(G.PlanRefused, match="bad problem"):
            G.tn_plan_ref(list(lst), 32)


# ------------------------------------------------------------------------------------------------ grouped weight gradients
def tdesc(M, N, /, bias=False, **kw):
    q = _lib.TnDesc(A=P, lda=up4(M) + 4, B=P, ldb=up4(N) + 4, M=M, N=N, C=P, ldc=N + 3, c_accumulate=1, bias_out=P if bias else None,
                    bias_accumulate=1)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def grouped_sweep():
    """(problems, K) of the grouped sweep, one launch at a time."""
    odd = (None, dict(M=499), dict(M=496), dict(N=177), dict(lda=503), dict(ldb=181), dict(A=P + 4), dict(B=P + 4), dict(M=2052))
    for n, M, N, bias, spoil, K in itertools.product((1, 3, 16), (500, 2048, 2200, 4096, 4100, 8192), (172, 175, 176, 177), (False, True), odd,
                                                     (100, 128, 129, 333, 53760)):
        probs = [tdesc(M + 4 * (i % 3), N, bias and i % 2 == 0) for i in range(n)]
        if spoil:
            for k, v in spoil.items():
                setattr(probs[n // 2], k, v)
        yield probs, K


def test_grouped_plan_follows_the_model_on_every_threshold():
    """1 / 3 / 16 problems; one M 499 or 496 among taller ones; one N, leading dimension or pointer that rules float4 loads out;
    the bias column at N 175 / 176 / 177; K 100 / 128 / 129 / 333 / 53 760; tile totals on both sides of what halves the split
    count (128 of 256 slots with 256-row tiles, 256 of 512 with 128-row ones) and of the slot counts themselves; the 1-D grid
    exactly when a bf16x3 form splits; a workspace one float short."""
    lib = _lib.load()
    seen, count, mapped = set(), 0, set()
    for probs, K in grouped_sweep():
        n = len(probs)
        lst = (_lib.TnDesc * n)(*probs)
        ref = G.tn_plan_ref(probs, K)
        got = _lib.gemm_plan("pfo_debug_gemm_tn_group_plan", lst, n, K, ref["need"])
        assert got == {k: ref[k] for k in FIELDS}, (got, ref)
        assert (got["grid_y"] == 1 and got["nsplit"] > 1) == (got["form"] != "tn_f32" and got["nsplit"] > 1) == bool(ref["xcd_map"])
        out = (C.c_int32 * len(FIELDS))()
        assert lib.pfo_debug_gemm_tn_group_plan(lst, n, K, ref["need"] - 1, out) == -1 and b"workspace too small" in lib.pfo_last_error()
        with pytest.raises(G.PlanRefused, match="workspace too small"):
            G.tn_plan_ref(probs, K, ref["need"] - 1)
        seen.add(got["form"])
        mapped.add((got["form"], got["nsplit"] > 1))
        count += 1
    assert seen == TN_FORMS and mapped == {(f, s) for f in TN_FORMS for s in (False, True)}
    assert count > 3000
