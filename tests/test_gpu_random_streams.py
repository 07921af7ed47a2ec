"""The three kernels that turn Philox words into decisions - the uniform neighbour sampler (pfo_tnbr_sample mode 2), the
candidate / negative draw (pfo_neg_draw[_dev]) and the attention dropout keep bits (pfo_attn_dropout_mask, the step's own
function) - against the host model tests/philox_ref.py, BIT FOR BIT: every comparison is np.array_equal.  That the model's
draws are uniform and independent is checked on the CPU (tests/test_philox_cpu.py); nothing here is statistical.

Tables of cases, not products: each row names the path it is there for."""
import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

import pfotgnrec_amd as P
from pfotgnrec_amd import _lib
from pfotgnrec_amd import rand_edge_sampler as RS
from oracle.neighbor_finder import OracleNeighborFinder, build_adjacency
from philox_ref import uniform_positions, neg_draw, available_lists, dropout_keep

DEV = "cuda:0"
SEED_HI = 0x1234567890ABCDEF          # the high key word is live


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ================================================================== candidate / negative draw
def _neg_inputs(n_items, B, W, rs):
    """Availability (about four in five) and B portfolios of width W that hold, between them: -1 padding INSIDE port_len,
    entries >= n_items, duplicates, unavailable items, port_len = 0 and port_len > W (the kernel clamps it to W)."""
    avail = (rs.rand(n_items) < 0.8).astype(np.uint8)
    avail[rs.randint(n_items)] = 1
    pi = rs.randint(0, n_items, size=(B, W)).astype(np.int32)
    if W:
        pi[rs.rand(B, W) < 0.15] = -1
        pi[rs.rand(B, W) < 0.10] = n_items + 3
        dup = rs.rand(B) < 0.3
        pi[dup, W - 1] = pi[dup, 0]
    pl = rs.randint(0, W + 1, size=B).astype(np.int32)
    pl[rs.rand(B) < 0.2] = W + 5
    pl[rs.rand(B) < 0.1] = 0
    return avail, pi, pl


def _draw(avail, pi, pl, size, upper_u, seed, offset, offset_dev=None):
    s = RS.DeviceNegativeSampler(avail, upper_u, DEV, seed=seed)
    out = s.sample(t(pi), t(pl), size, offset, offset_dev)
    torch.cuda.synchronize()
    assert out.dtype == torch.int32 and tuple(out.shape) == (len(pl), size)
    return out.cpu().numpy().astype(np.int64)


# (n_items, B, W, size, seed, offset)
NEG_CASES = [
    (1, 1, 0, 1, 0, 3 << 24),                    # one item, no portfolio
    (1, 70, 1, 3, 0x5EED, 5 << 36),              # the item is in some portfolios: empty pools (zeros) beside 1-item pools, replacement
    (63, 70, 8, 4, 2024, 3 << 24),               # ballot tail: one partial chunk; words 0..3 of block 0
    (64, 1, 8, 5, SEED_HI, 5 << 36),             # exactly one chunk; slot 4 is word 0 of block 1; high key word, high counter word
    (64, 70, 1, 64, 0, 3 << 24),                 # size 64 against <= 64 available: mostly replacement, one wavefront exactly
    (65, 70, 8, 65, 0x5EED, 3 << 24),            # second chunk holds one item; replacement loop wraps to lane 0 once
    (65, 1, 0, 20, 2024, 5 << 36),               # Fisher-Yates over five blocks
    (200, 70, 8, 130, SEED_HI, 3 << 24),         # multi-chunk compaction; Fisher-Yates over 33 blocks (n_avail >= 130)
    (200, 70, 0, 20, 0x5EED, 5 << 36),
    (200, 70, 1, 1, 0, 3 << 24),
    (63, 70, 8, 130, 2024, 5 << 36),             # replacement, three passes of the lane-strided loop
    (200, 8, 8, 5, 2024, 2 ** 32 - 3),           # b + offset carries into the second counter word at b = 3
    (200, 8, 8, 65, SEED_HI, 2 ** 64 - 3),       # ... and wraps the 64-bit counter
]


@pytest.mark.parametrize("n_items,B,W,size,seed,offset", NEG_CASES)
def test_neg_draw_equals_model(n_items, B, W, size, seed, offset):
    rs = np.random.RandomState(n_items * 1000 + B * 10 + W + size)
    avail, pi, pl = _neg_inputs(n_items, B, W, rs)
    upper_u = 11 + n_items
    got = _draw(avail, pi, pl, size, upper_u, seed, offset)
    want = neg_draw(avail, pi, pl, size, upper_u, seed, offset)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(1))[:8]


@pytest.mark.parametrize("size", [1, 4, 5, 64])
def test_neg_draw_branch_boundary_in_one_batch(size):
    """Rows with n_avail = 0, size - 1, size, size + 1 side by side: zeros / with replacement / a permutation of the pool /
    without replacement."""
    n_items = 150
    rs = np.random.RandomState(size)
    items = np.sort(rs.choice(n_items, size + 1, replace=False))
    avail = np.zeros(n_items, np.uint8)
    avail[items] = 1
    W = size + 1
    pi = np.tile(rs.permutation(items).astype(np.int32), (4, 1))
    pl = np.array([size + 1, 2, 1, 0], np.int32)
    n_av = [len(l) for l in available_lists(avail, pi, pl)]
    assert n_av == [0, size - 1, size, size + 1]
    got = _draw(avail, pi, pl, size, 500, 0x5EED, 3 << 24)
    want = neg_draw(avail, pi, pl, size, 500, 0x5EED, 3 << 24)
    assert np.array_equal(got, want)
    assert not got[0].any()                                                       # nothing available: node id 0, as the header says


def test_neg_draw_portfolio_edges():
    """-1 inside port_len, entries >= n_items, duplicates, an unavailable item, port_len 0, port_len > W: one row each."""
    n_items = 70
    avail = np.ones(n_items, np.uint8)
    avail[[5, 66]] = 0
    pi = np.array([[3, -1, 4, -1], [70, 1000, 2, 69], [7, 7, 7, 7], [5, 66, 0, 1], [1, 2, 3, 4], [1, 2, 3, 4]], np.int32)
    pl = np.array([4, 4, 4, 4, 0, 9], np.int32)
    n_av = [len(l) for l in available_lists(avail, pi, pl)]
    assert n_av == [66, 66, 67, 66, 68, 64]
    for size in (3, 67):
        got = _draw(avail, pi, pl, size, 99, 2024, 5 << 36)
        assert np.array_equal(got, neg_draw(avail, pi, pl, size, 99, 2024, 5 << 36))


def test_neg_draw_offset_on_the_device():
    """An offset_dev word holding x with offset = 0 is offset = x with no word; the two add."""
    rs = np.random.RandomState(5)
    avail, pi, pl = _neg_inputs(200, 70, 8, rs)
    x = 5 << 36
    word = torch.tensor([x], dtype=torch.int64, device=DEV)
    want = neg_draw(avail, pi, pl, 20, 300, SEED_HI, x)
    assert np.array_equal(_draw(avail, pi, pl, 20, 300, SEED_HI, x), want)
    assert np.array_equal(_draw(avail, pi, pl, 20, 300, SEED_HI, 0, offset_dev=word), want)
    assert not np.array_equal(_draw(avail, pi, pl, 20, 300, SEED_HI, 0), want)
    assert np.array_equal(_draw(avail, pi, pl, 20, 300, SEED_HI, 3 << 24, offset_dev=word), neg_draw(avail, pi, pl, 20, 300, SEED_HI, x + (3 << 24)))
    # the plain entry point
    out = torch.empty((70, 20), dtype=torch.int32, device=DEV)
    d_avail, d_pi, d_pl = t(avail), t(pi), t(pl)
    _lib.call("pfo_neg_draw", _lib.ptr(d_avail), 200, _lib.ptr(d_pi), _lib.ptr(d_pl), 8, 70, 20, 300, SEED_HI, x, _lib.ptr(out),
              _lib.stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)


def test_neg_draw_at_the_documented_maximum():
    """n_items = 16384, the bound of pfo_neg_draw_dev: the available list is exactly 64 KiB of dynamic LDS."""
    n_items = 16384
    rs = np.random.RandomState(16384)
    avail, pi, pl = _neg_inputs(n_items, 3, 8, rs)
    avail[-1] = avail[0] = 1
    for size in (5, 130):
        got = _draw(avail, pi, pl, size, 7, 0x5EED, 3 << 24)
        assert np.array_equal(got, neg_draw(avail, pi, pl, size, 7, 0x5EED, 3 << 24))
    few = np.zeros(n_items, np.uint8)                                             # the last chunk's last lane, with replacement
    few[[0, 8191, 16383]] = 1
    got = _draw(few, pi, pl, 5, 7, 0x5EED, 3 << 24)
    assert np.array_equal(got, neg_draw(few, pi, pl, 5, 7, 0x5EED, 3 << 24)) and (got == 16383 + 8).any()
    with pytest.raises(_lib.PfoError):
        _draw(np.ones(n_items + 1, np.uint8), pi, pl, 5, 7, 0, 0)


@pytest.fixture()
def sampler_data():
    """A dataset in the drop-in's own terms: stock codes, a long-lived object array of portfolios (long enough to be packed
    once and served as slices), the train destinations."""
    n_items, upper_u = 65, 300
    rs = np.random.RandomState(77)
    codes = ["%06d" % (i + 1) for i in range(n_items)]
    m = {c: i for i, c in enumerate(codes)}
    seen = np.sort(rs.choice(n_items, 50, replace=False))
    dst_all = rs.choice(seen, 3000) + upper_u + 1
    N = 4200
    ports = np.empty(N, dtype=object)
    idx = np.full((N, 8), -1, np.int32)
    lens = np.zeros(N, np.int32)
    for r in range(N):
        L = rs.randint(0, 9)
        row = rs.choice(n_items, L, replace=False)
        ports[r] = [codes[j] for j in row] if L else [""]
        idx[r, :L], lens[r] = row, L
    avail = np.zeros(n_items, np.uint8)
    avail[np.unique(dst_all) - upper_u - 1] = 1                                   # np.unique(dst_list), utils.py:73
    saved = [list(c) for c in (RS._PORT_CACHE, RS._PORT_BAD, RS._PORT_DEV, RS._AVAIL_DEV, RS._AVAIL_CACHE)]
    yield dict(n_items=n_items, upper_u=upper_u, m=m, dst_all=dst_all, ports=ports, idx=idx, lens=lens, avail=avail,
               src=np.zeros(8, np.int64))
    RS._PORT_CACHE[:], RS._PORT_BAD[:], RS._PORT_DEV[:], RS._AVAIL_DEV[:], RS._AVAIL_CACHE[:] = saved


@pytest.mark.parametrize("size", [5, 60])
def test_rand_edge_sampler_both_seedings(sampler_data, size):
    """RandEdgeSampler.sample: seeded -> the model at (seed, offset 0); unseeded -> seed 0x5EED at the call counter << 24.  Two
    samplers over slices of ONE portfolio array are held at once and sampled in the other order: each draws against its own
    portfolios (the device rows come from the slice, not from what was packed last)."""
    d = sampler_data
    sl_a, sl_b = slice(100, 170), slice(2000, 2070)
    a = P.RandEdgeSampler(d["src"], d["dst_all"], d["ports"][sl_a], d["upper_u"], d["m"], seed=2024)
    b = P.RandEdgeSampler(d["src"], d["dst_all"], d["ports"][sl_b], d["upper_u"], d["m"])
    assert a.port_idx.base is not None and a.port_idx.base is b.port_idx.base      # slices of the one packed base
    got_a = a.sample(size)
    assert got_a.dtype == np.int64
    assert np.array_equal(got_a, neg_draw(d["avail"], d["idx"][sl_a], d["lens"][sl_a], size, d["upper_u"], 2024, 0))
    for _ in range(2):                                                             # a fresh stream every call
        got_b = b.sample(size)
        off = RS._GLOBAL_CALLS[0] << 24
        assert np.array_equal(got_b, neg_draw(d["avail"], d["idx"][sl_b], d["lens"][sl_b], size, d["upper_u"], 0x5EED, off))
    assert np.array_equal(a.sample(size), got_a)                                   # seeded: the same negatives on every run


# ================================================================== uniform neighbour sampling (mode 2)
DEGREES = {0: 0, 1: 1, 2: 2, 3: 17, 4: 300, 5: 5000}       # hub node -> degree; nodes 10..49 are their neighbours (~130 each)
N_NODES = 56                                                 # 50..55 have no edge either


def _graph():
    """Edges hub -> 10 + (e mod 40).  Times repeat inside every row: hubs 1-4 hold each time three times; hub 5 holds
    2^25 + e // 2 - distinct f64 times two by two, and EIGHT consecutive entries per f32 value (one f32 step is 4 there), so
    the slot sort's tie rule decides most of its rows."""
    src, dst, ts = [], [], []
    for hub, deg in DEGREES.items():
        e = np.arange(deg)
        src.append(np.full(deg, hub)); dst.append(10 + (e * 7 + hub) % 40)
        ts.append((2.0 ** 25 + e // 2) if hub == 5 else (100.0 * hub + e // 3))
    src, dst, ts = np.concatenate(src), np.concatenate(dst), np.concatenate(ts).astype(np.float64)
    order = np.argsort(ts, kind="stable")
    src, dst, ts = src[order], dst[order], ts[order]
    return src.astype(np.int64), dst.astype(np.int64), np.arange(1, len(src) + 1, dtype=np.int64), ts


@pytest.fixture(scope="module")
def finders():
    src, dst, eidx, ts = _graph()
    nf = P.NeighborFinder.from_arrays(src, dst, eidx, ts, uniform=True, max_node_idx=N_NODES - 1)
    onf = OracleNeighborFinder(*build_adjacency(src, dst, eidx, ts, N_NODES - 1), uniform=True)
    assert [int(onf.indptr[v + 1] - onf.indptr[v]) for v in DEGREES] == list(DEGREES.values())
    return nf, onf


def _queries(onf, N, rs):
    """Every hub, neighbour nodes, an edgeless node and an id >= n_nodes; times before the row's first edge, ON a repeated
    time (strictly-before: the tie group is out), between two repeated times, and after the last edge."""
    pool = np.array(list(DEGREES) + [10, 23, 49, 50, N_NODES + 3])
    q = pool[(np.arange(N) + 4) % len(pool)]                                      # (N = 1: the hub of degree 300)
    qt = np.zeros(N, np.float64)
    for i, v in enumerate(q):
        row = onf.ts[onf.indptr[v]:onf.indptr[v + 1]] if v < N_NODES else np.zeros(0)
        if len(row) == 0:
            qt[i] = 1000.0
            continue
        pick = rs.randint(len(row))
        qt[i] = (row[0] - 1.0, row[pick], row[pick] + 0.5, row[-1] + 1.0, row[-1] + 1.0)[rs.randint(5)]
    return q.astype(np.int64), qt


def _expected(onf, q, qt, seed, offset, K):
    """(positions, nbr, eidx, et): cnt from the oracle's find_before, the model's positions, the oracle's gather with its
    canonical stable sort.  A node id outside the table has no history."""
    inside = q < N_NODES
    qo = np.where(inside, q, 0)                                                   # node 0 has no edge: an all-padding row
    cnt = np.array([len(onf.find_before(int(a), b)[0]) for a, b in zip(qo, qt)], np.int64)
    assert not cnt[~inside].any()
    pos = uniform_positions(seed, offset, cnt, K)
    nb, ei, et = onf.gather_uniform(qo, qt, np.maximum(pos, 0), K)
    return cnt, pos, nb, ei, et


def _raw_sample(nf, q, qt, K, mode, seed, offset, draws=None):
    """pfo_tnbr_sample through the C ABI with every output: (nbr, eidx, et, dt, next_nodes, next_ts)."""
    indptr, anbr, aeidx, ats = nf.device_arrays(DEV)
    N = len(q)
    qn, qts = t(np.asarray(q).astype(np.int32)), t(np.asarray(qt, np.float64))
    dd = None if draws is None else t(np.asarray(draws, np.int64))
    nb = torch.empty((N, K), dtype=torch.int32, device=DEV)
    ei = torch.empty((N, K), dtype=torch.int32, device=DEV)
    et = torch.empty((N, K), dtype=torch.float32, device=DEV)
    dt = torch.empty((N, K), dtype=torch.float32, device=DEV)
    nxt = torch.empty(N * (K + 1), dtype=torch.int32, device=DEV)
    nts = torch.empty(N * (K + 1), dtype=torch.float64, device=DEV)
    _lib.call("pfo_tnbr_sample", indptr.data_ptr(), anbr.data_ptr(), aeidx.data_ptr(), ats.data_ptr(), nf.n_nodes,
              qn.data_ptr(), qts.data_ptr(), N, K, mode, _lib.ptr(dd), seed, offset, nb.data_ptr(), ei.data_ptr(), et.data_ptr(),
              dt.data_ptr(), nxt.data_ptr(), nts.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return tuple(a.cpu().numpy() for a in (nb, ei, et, dt, nxt, nts))


ABI_OFFSET = (41 << 36) + (2 << 32)           # the step's layout (step 41, level 2): the FOURTH counter word is live

# (N, K, seed): sixteen queries share a workgroup (N = 15, 16, 17: the last group partial / full / one query in a second
# workgroup); K = 3, 4, 5 around one Philox block, 16, 17 around one pass of the 16 lanes of a query, 63, 64 the last pass
UNIFORM_CASES = [(1, 1, 0), (15, 3, 0x5EED), (16, 4, 2024), (17, 5, SEED_HI), (300, 16, 0x5EED), (300, 17, 0), (17, 63, 2024),
                 (300, 64, SEED_HI), (16, 64, 0), (1, 64, 2024), (15, 17, SEED_HI)]


@pytest.mark.parametrize("N,K,seed", UNIFORM_CASES)
def test_uniform_sampler_equals_model(finders, N, K, seed):
    nf, onf = finders
    rs = np.random.RandomState(N * 100 + K)
    q, qt = _queries(onf, N, rs)
    # ---- through the finder: the stream position is its call counter << 20
    nf.seed = seed
    nb, ei, et = nf.get_temporal_neighbor(q, qt, K)
    off = nf._calls << 20
    cnt, pos, rn, re, rt = _expected(onf, q, qt, seed, off, K)
    assert np.array_equal(nb, rn) and np.array_equal(ei, re) and np.array_equal(et, rt)
    assert et.dtype == np.float32 and nb.dtype == np.int32
    m1 = nf.get_temporal_neighbor(q, qt, K, draws=np.maximum(pos, 0))               # the product's own mode 1, same positions
    assert all(np.array_equal(a, b) for a, b in zip(m1, (nb, ei, et)))
    # ---- through the C ABI at a position of the step's layout, every output
    cnt, pos, rn, re, rt = _expected(onf, q, qt, seed, ABI_OFFSET, K)
    got = _raw_sample(nf, q, qt, K, 2, seed, ABI_OFFSET)
    assert np.array_equal(got[0], rn) and np.array_equal(got[1], re) and np.array_equal(got[2], rt)
    assert np.array_equal(got[3], (qt[:, None] - rt.astype(np.float64)).astype(np.float32))
    assert np.array_equal(got[4], np.concatenate([q.astype(np.int32), rn.flatten()]))
    assert np.array_equal(got[5], np.concatenate([qt, np.repeat(qt, K)]))
    inj = _raw_sample(nf, q, qt, K, 1, 0, 0, draws=np.maximum(pos, 0))
    assert all(np.array_equal(a, b) for a, b in zip(inj, got))
    if N == 300:
        # the cases do what they are there for: a row whose slots tie in f32 time while their entries differ, rows without history
        big = np.flatnonzero(cnt >= 1000)
        assert len(big) and any((np.diff(rt[i]) == 0).any() and len(set(re[i].tolist())) > len(set(rt[i].tolist())) for i in big)
        assert (cnt == 0).any() and (cnt == 1).any()


def test_uniform_sampler_stream_position_matters(finders):
    """The same queries at another level of the step's layout (+ 2^32), another step (+ 2^36) and another key draw differently,
    each as the model says (a dropped high counter or key word would repeat the draw)."""
    nf, onf = finders
    q, qt = _queries(onf, 64, np.random.RandomState(9))
    seen = []
    for seed, off in ((SEED_HI, ABI_OFFSET), (SEED_HI, ABI_OFFSET - (1 << 32)), (SEED_HI, ABI_OFFSET + (1 << 36)),
                      (SEED_HI & 0xFFFFFFFF, ABI_OFFSET), (SEED_HI, 2 ** 64 - 2)):
        _, _, rn, re, rt = _expected(onf, q, qt, seed, off, 20)
        got = _raw_sample(nf, q, qt, 20, 2, seed, off)
        assert np.array_equal(got[0], rn) and np.array_equal(got[1], re) and np.array_equal(got[2], rt)
        assert not any(np.array_equal(re, s) for s in seen)
        seen.append(re)


# ================================================================== attention dropout keep bits
# The low counter word is n * 64 + lane: it cannot cross 2^32 at any size a test can afford (n >= 2^26 instances); that word of
# the shared generator is covered by the negative draw's carry cases above.
# (N, K, H, p, seed, offset)
DROPOUT_CASES = [
    (1, 1, 1, 0.1, 0, 0x51ED0001),
    (37, 10, 2, 0.25, 0x5EED, (7 << 36) + 0x51ED0000 + 2),
    (5, 64, 4, 0.5, 2024, (1 << 36) + 0x51ED0000 + 1),
    (33, 7, 4, 0.999, SEED_HI, (41 << 36) + 0x51ED0000 + 1),
    (16400, 64, 1, 0.1, SEED_HI, (3 << 36) + 0x51ED0000 + 2),   # the smallest N * K beyond the 4096 x 256 launch: the grid-stride loop
    (37, 10, 2, 0.0, 0x5EED, 5),                                  # p = 0: all ones
]


@pytest.mark.parametrize("N,K,H,p,seed,offset", DROPOUT_CASES)
def test_dropout_mask_equals_model(N, K, H, p, seed, offset):
    m = torch.full((N, H, K), -1.0, dtype=torch.float32, device=DEV)
    _lib.call("pfo_attn_dropout_mask", seed, offset, N, K, H, p, m.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    m = m.cpu().numpy()
    if p == 0.0:
        assert np.array_equal(m, np.ones((N, H, K), np.float32))
        return
    keep = dropout_keep(seed, offset, N, K, H, p)
    assert np.array_equal(m != 0, keep)
    # the multiplier: ONE value, within one fp32 ulp of 1 / (1 - p) evaluated in fp32 (bit equality would need the build to
    # promise a correctly rounded fp32 divide; it sets no flag either way)
    vals = np.unique(m[keep])
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    assert len(vals) == (1 if keep.any() else 0)
    if keep.any():
        assert abs(np.float64(vals[0]) - np.float64(scale)) <= np.spacing(scale)
    if N * K > 4096 * 256:
        assert (m[4096 * 256 // K:] != 0).any() and (m[4096 * 256 // K:] == 0).any()


# ================================================================== the streams inside a step
def test_step_draws_and_masks_follow_the_stream_layout():
    """One model, uniform finder, L = 2: the step places its streams at offset = step << 36, sampler level l at + (l << 32),
    dropout of layer l at + 0x51ED0000 + l.  (1) train mode: the exported masks are the model's at those positions; (2) eval
    mode: a forward that draws its neighbours itself equals, bitwise, the same forward GIVEN the model's positions, expanded
    level by level with the oracle's gather - at two consecutive step counters."""
    from pfotgnrec_amd.synthetic import SyntheticConfig, make_graph
    cfg = SyntheticConfig("dm", 200, 20, 3000, 32, 2, 10, 2)
    L, H, K, B = 2, 2, 10, 64
    g = make_graph(cfg, with_prices=False)
    d = g.data
    nf = P.get_neighbor_finder(d, True)
    nf.seed = 2024
    onf = OracleNeighborFinder(*build_adjacency(d.sources, d.destinations, d.edge_idxs, d.timestamps), uniform=True)
    torch.manual_seed(5)
    tgn = P.TGN(nf, g.node_features, g.edge_features, DEV, n_layers=L, n_heads=H, dropout=0.25, use_memory=True,
                memory_dimension=32, message_function="identity", n_neighbors=K)
    neg = np.random.RandomState(0).randint(cfg.n_users + 1, cfg.n_users + cfg.n_items + 1, size=B * 3)

    def batch(s):
        return d.sources[s:s + B], d.destinations[s:s + B], neg, d.timestamps[s:s + B], d.edge_idxs[s:s + B], K
    # ---- (1) the masks of a train-mode forward (which also leaves memory and pending messages for part 2)
    tgn.train()
    tgn._step = 6
    tgn.compute_temporal_embeddings(*batch(1400))
    seed, offset = tgn._last_call[:2]
    assert (seed, offset) == (2024, 7 << 36)
    masks = tgn.debug_dropout_masks()
    n = 5 * B
    for l in (2, 1):
        assert masks[l].shape == (n, H, K)
        assert np.array_equal(masks[l] != 0, dropout_keep(seed, offset + 0x51ED0000 + l, n, K, H, 0.25)), l
        n *= 1 + K
    # ---- (2) the draws of an eval-mode forward
    tgn.eval()
    state = tgn.memory.backup_memory()
    sb, db, _, tb, _, _ = batch(1500)
    roots, rts = np.concatenate([sb, db, neg]), np.concatenate([tb, tb, np.repeat(tb, 3)])
    embs = []
    for step in (40, 41):
        with torch.no_grad():
            tgn.memory.restore_memory(state)
            tgn._step = step
            own = torch.cat(tgn.compute_temporal_embeddings(*batch(1500)))
            seed, offset = tgn._last_call[:2]
            assert (seed, offset) == (2024, (step + 1) << 36)
            # product order: one tensor per level L .. 1, level l drawn at offset + (l << 32) over [S_l]
            draws, (n_, t_) = [], (roots, rts)
            for l in range(L, 0, -1):
                cnt = np.array([len(onf.find_before(int(a), b)[0]) for a, b in zip(n_, t_)], np.int64)
                dr = uniform_positions(seed, offset + (l << 32), cnt, K)
                draws.append(dr)
                nb, _, _ = onf.gather_uniform(n_, t_, np.maximum(dr, 0), K)
                n_, t_ = np.concatenate([n_, nb.flatten()]), np.concatenate([t_, np.repeat(t_, K)])
            assert (draws[0] >= 0).any() and draws[1].shape == (5 * B * (1 + K), K)
            tgn.memory.restore_memory(state)
            tgn._step = step
            given = torch.cat(tgn.compute_temporal_embeddings(*batch(1500), draws=draws))
        assert torch.equal(own, given), step
        embs.append(own)
    assert not torch.equal(embs[0], embs[1])                                       # another step, another draw
