"""The two launches FusedAdam puts in front of the Adam kernel (csrc/optim.hip), on raw tensors through the C ABI, against the
host model of tests/optim_ref.py: the fp64 sum of squares over element ranges, the clip coefficient, the scaled gradients and the
decayed parameters - bit for bit where the arithmetic is fp32 - and nothing outside the ranges touched."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import has_gpu
import optim_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

from pfotgnrec_amd import _lib

DEV = "cuda:0"
GUARD = 32              # canary elements in front of and behind each buffer (32 floats = 128 bytes: the base stays 16-byte aligned)
MAX_NORM = 0.37         # clips every standard-normal case of more than a few elements; a single small element is left alone
DECAY = float(R.decay_factor(1e-2, 0.3))


def _gapped(n_ranges, seed):
    """Ranges of 0-300 elements with gaps of 1-5 elements; the second and the second to last are empty (lo == hi)."""
    rs = np.random.RandomState(seed)
    lo, hi, at = [], [], 0
    for r in range(n_ranges):
        at += int(rs.randint(1, 6))
        n = 0 if r in (1, n_ranges - 2) else int(rs.randint(1, 301))
        lo.append(at); hi.append(at + n)
        at += n
    return lo, hi, at + 3


def _layouts():
    """name -> (lo, hi, buffer length, element offset of the base pointer): the smallest sizes at which the sweep can go wrong -
    less than one vector, one wavefront -1 / +0 / +1, more than one workgroup, a start at every offset inside a vector, many ranges
    with gaps and empty ones, more ranges than one call takes (two chunks, the second accumulating), more elements than one pass
    of the grid (256 workgroups x 256 lanes x 4), and a base that is not 16-byte aligned (the four-scalar form of every access)."""
    out = {}
    for n in (1, 3, 63, 64, 65, 257, 4101):
        out["one-%d" % n] = ([8], [8 + n], n + 16, 0)
    for off in (1, 2, 3):
        out["start+%d" % off] = ([8 + off], [8 + off + 257], 280, 0)
    lo, hi, total = _gapped(16, 1)
    out["gapped-16"] = (lo, hi, total, 0)
    lo, hi, total = _gapped(19, 2)
    out["chunks-19"] = (lo, hi, total, 0)
    out["one-200003"] = ([5], [5 + 200003], 200003 + 9, 0)
    out["one-300001"] = ([2], [2 + 300001], 300001 + 4, 0)          # (> 262144: lanes take a second group)
    out["unaligned-4101"] = ([8], [8 + 4101], 4101 + 16, 1)
    lo, hi, total = _gapped(16, 1)
    out["unaligned-gapped-16"] = (lo, hi, total, 3)
    return out


LAYOUTS = _layouts()
VALUES = ("normal", "zero", "big", "inf", "nan")


def _values(kind, n_total, lo, hi, seed=5):
    rs = np.random.RandomState(seed)
    g = rs.randn(n_total).astype(np.float32)
    idx = R.elements(lo, hi)
    if kind == "zero":
        g[idx] = 0
    elif kind != "normal":
        g[idx[len(idx) // 2]] = {"big": 1e20, "inf": np.inf, "nan": np.nan}[kind]
    p = rs.randn(n_total).astype(np.float32)
    return p, g


def _chunks(lo, hi):
    arr = lambda v: (C.c_int64 * len(v))(*v)
    return [(len(lo[i:i + R.MAX_RANGES]), arr(lo[i:i + R.MAX_RANGES]), arr(hi[i:i + R.MAX_RANGES])) for i in range(0, len(lo), R.MAX_RANGES)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


class _Run:
    """One pass over (p, g): both entries, everything read back.  The buffers sit between canaries; ``base`` shifts the pointer
    the entries get by that many elements (the canary in front grows by as much)."""

    def __init__(self, p, g, lo, hi, base=0, max_norm=MAX_NORM, decay=DECAY, null_partial=False):
        n = len(p)
        hold = lambda a: torch.from_numpy(np.concatenate([np.full(GUARD + base, 7.25, np.float32), a, np.full(GUARD, -3.5, np.float32)])).to(DEV)
        tp, tg = hold(p), hold(g)
        partial = torch.full((R.GRAD_NORM_PARTS + 2,), 1e300, dtype=torch.float64, device=DEV)     # (stale values: accumulate = 0 overwrites)
        norm = torch.full((3,), -1.0, dtype=torch.float32, device=DEV)
        pp, gp = tp.data_ptr() + 4 * (GUARD + base), tg.data_ptr() + 4 * (GUARD + base)
        assert (pp % 16 == 0) == (base % 4 == 0)
        chunks = _chunks(lo, hi)
        s = _lib.stream_ptr()
        if max_norm > 0 and not null_partial:
            for j, ch in enumerate(chunks):
                _lib.call("pfo_grad_sumsq_ranges", gp, *ch, partial.data_ptr() + 8, 1 if j else 0, s)
        for ch in chunks:
            _lib.call("pfo_grad_prestep_ranges", pp, gp, *ch, None if null_partial else partial.data_ptr() + 8, max_norm, decay,
                      None if null_partial else norm.data_ptr() + 4, s)
        torch.cuda.synchronize()
        hp, hg = tp.cpu().numpy(), tg.cpu().numpy()
        self.p, self.g = hp[GUARD + base:GUARD + base + n], hg[GUARD + base:GUARD + base + n]
        self.canaries_ok = all((a[:GUARD + base] == 7.25).all() and (a[GUARD + base + n:] == -3.5).all() for a in (hp, hg))
        part = partial.cpu().numpy()
        self.partial, self.partial_guard = part[1:-1], (part[0], part[-1])
        nm = norm.cpu().numpy()
        self.total, self.norm_guard = nm[1], (nm[0], nm[2])

    def same_bits(self, other):
        return all(np.array_equal(_bits(a), _bits(b)) for a, b in ((self.p, other.p), (self.g, other.g), (self.partial, other.partial),
                                                                    (np.float32([self.total]), np.float32([other.total]))))


def _within_one_ulp(a, b):
    a, b = np.float32(a), np.float32(b)
    if np.isnan(a) or np.isnan(b):
        return bool(np.isnan(a) and np.isnan(b))
    if np.isinf(a) or np.isinf(b):
        return bool(a == b)
    return abs(int(_bits(np.float32([a]))[0]) - int(_bits(np.float32([b]))[0])) <= 1


@pytest.mark.parametrize("values", VALUES)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_prestep_against_the_host_model(layout, values):
    lo, hi, n_total, base = LAYOUTS[layout]
    p, g = _values(values, n_total, lo, hi)
    run = _Run(p, g, lo, hi, base)
    idx = R.elements(lo, hi)
    outside = np.setdiff1d(np.arange(n_total), idx)
    # the norm: fp64 accumulation, (float) sqrt - within one fp32 ulp of numpy's (the order of the fp64 additions differs)
    want_total = R.total_norm(g, lo, hi)
    assert _within_one_ulp(run.total, want_total), (run.total, want_total)
    if values == "big":
        assert np.isfinite(run.total) and run.total >= np.float32(1e20)
    if values in ("inf", "nan"):
        assert not np.isfinite(run.total)
    with np.errstate(all="ignore"):
        assert _within_one_ulp(np.float32(np.sqrt(np.float64(run.partial.sum()))), want_total) or values in ("inf", "nan")
    # gradients and parameters: fp32 products, bit for bit, with the coefficient recomputed from the DEVICE's total
    coef = R.clip_coef(run.total, MAX_NORM)
    if values == "zero":
        assert coef == 1
    if values == "normal" and len(idx) >= 63:
        assert coef < 1
    want_p, want_g, _ = R.prestep(p, g, lo, hi, MAX_NORM, np.float32(DECAY), total=run.total)
    assert np.array_equal(run.g[idx], want_g[idx], equal_nan=True)
    assert np.array_equal(run.p[idx], want_p[idx]) and np.array_equal(want_p[idx], p[idx] * np.float32(DECAY))
    assert np.array_equal(_bits(run.g[outside]), _bits(g[outside])) and np.array_equal(_bits(run.p[outside]), _bits(p[outside]))
    assert run.canaries_ok and run.partial_guard == (1e300, 1e300) and run.norm_guard == (-1.0, -1.0)
    # no dependence on timing: a second run gives the same bits, partial sums included
    assert run.same_bits(_Run(p, g, lo, hi, base))


@pytest.mark.parametrize("layout", ["one-3", "one-4101", "start+3", "gapped-16", "chunks-19", "unaligned-4101"])
def test_options_that_are_off_write_nothing(layout):
    lo, hi, n_total, base = LAYOUTS[layout]
    p, g = _values("normal", n_total, lo, hi)
    idx = R.elements(lo, hi)
    for max_norm in (0.0, -1.0):                                           # no clipping: NULL partial / norm_out, gradients untouched
        run = _Run(p, g, lo, hi, base, max_norm=max_norm, null_partial=True)
        assert np.array_equal(_bits(run.g), _bits(g)) and run.canaries_ok
        assert np.array_equal(run.p[idx], p[idx] * np.float32(DECAY))
    run = _Run(p, g, lo, hi, base, decay=1.0)                              # no decay: parameters untouched
    assert np.array_equal(_bits(run.p), _bits(p)) and run.canaries_ok
    assert np.array_equal(run.g[idx], g[idx] * R.clip_coef(run.total, MAX_NORM))
    run = _Run(p, g, lo, hi, base, max_norm=0.0, decay=1.0, null_partial=True)
    assert np.array_equal(_bits(run.p), _bits(p)) and np.array_equal(_bits(run.g), _bits(g)) and run.total == -1.0


def test_slots_depend_on_the_ranges_alone():
    """Which element feeds which slot is a function of (lo, hi): the same values at the same element offsets give the same 256
    partial sums from a 16-byte aligned base (one 16-byte access per group of 4) and from a base that is not (four accesses)."""
    for layout in ("gapped-16", "one-4101"):
        lo, hi, n_total, _ = LAYOUTS[layout]
        p, g = _values("normal", n_total, lo, hi)
        runs = [_Run(p, g, lo, hi, base) for base in (0, 1, 2, 4)]
        assert all(runs[0].same_bits(r) for r in runs[1:])
    assert np.count_nonzero(runs[0].partial) == 5                           # (4101 elements: 1025 groups of 4 over workgroups of 256 lanes)


def test_accumulate_adds_in_stream_order():
    """Two chunks give the slots of the first call plus those of the second, slot by slot."""
    lo, hi, n_total, _ = LAYOUTS["chunks-19"]
    p, g = _values("normal", n_total, lo, hi)
    both = _Run(p, g, lo, hi)
    first = _Run(p, g, lo[:16], hi[:16])
    second = _Run(p, g, lo[16:], hi[16:])
    assert np.array_equal(both.partial, first.partial + second.partial)
    assert _within_one_ulp(both.total, R.total_norm(g, lo, hi))
