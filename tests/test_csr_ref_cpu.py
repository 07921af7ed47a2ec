"""tests/csr_ref.py held to everything else that states the same adjacency - its own vectorised twin, the package's host build,
the oracle on the reference's g1 graphs - on every generator the GPU file uses, with timestamps compared by bits; the append
and root models held to their plain statements; the generators held to what their names promise; the NaN guard of the device
paths; and the plan query of pfo_csr_build (pure host code) on the sizes the GPU cases are built around."""
import numpy as np
import pytest

from conftest import load_golden
from oracle.neighbor_finder import build_adjacency
from pfotgnrec_amd import _lib, neighbor_finder as NF
import csr_ref as R

f64 = np.float64


def _logs():
    """(id, src, dst, eidx, ts, n_nodes): every timestamp generator over hub-heavy edges, at sizes the list form affords."""
    out = []
    for E in (1, 2, 33, 513, 1025):
        out.append(("chrono-E%d" % E, R.edges(E, 40, E), R.chronological_with_ties(E, E), 40))
        for at in (R.inversion_places(E) if E >= 2 else []):
            out.append(("inv%d-E%d" % (at, E), R.edges(E, 40, E), R.one_inversion(E, at, E), 40))
    for k in range(8):
        out.append(("byte%d" % k, R.edges(3000, 300, k), R.byte_decides(k, 3000), 300))
    out.append(("edge-values", R.edges(3000, 300, 9), R.edge_values(3000), 300))
    for n in R.OWNER_TABLES:
        out.append(("table%d" % n, R.edges(600, n, n % 97), R.edge_values(600, 1), n))
    out = [(cid, e[0], e[1], e[2], ts, n) for cid, e, ts, n in out]
    for chrono in (True, False):
        out.append(("zero-example-%s" % chrono,) + R.signed_zero_example(chrono))
        out.append(("zero-log-%s" % chrono,) + R.signed_zero_log(3000, chrono))
    return out


LOGS = _logs()


@pytest.mark.parametrize("case", LOGS, ids=[c[0] for c in LOGS])
def test_list_model_equals_its_twin_and_the_host_build(case):
    cid, src, dst, eidx, ts, n = case
    assert sorted(eidx.tolist()) == list(range(1, len(eidx) + 1))
    assert len(eidx) < 3 or cid.startswith("zero-example") or not np.array_equal(eidx, np.arange(1, len(eidx) + 1)), "eidx must not be arange"
    ref = R.build(src, dst, eidx, ts, n)
    assert ref[0].dtype == np.int64 and ref[1].dtype == np.int32 and ref[2].dtype == np.int32 and ref[3].dtype == f64
    assert len(ref[0]) == n + 1 and ref[0][-1] == 2 * len(src)
    assert R.csr_equal(ref, R.build_fast(src, dst, eidx, ts, n)), "list form and vectorised twin differ"
    assert R.csr_equal(ref, NF.build_csr(src, dst, eidx, ts, max_node_idx=n - 1)), "model and neighbor_finder.build_csr differ"
    # every row ascends (IEEE order) and the multiset of stored timestamp BITS is the input's, twice
    for v in range(min(n, 400)):
        row = ref[3][ref[0][v]:ref[0][v + 1]]
        assert np.all(row[:-1] <= row[1:])
    assert np.array_equal(np.sort(R.bits64(ref[3])), np.sort(np.repeat(R.bits64(ts), 2)))


def test_model_equals_the_oracle_on_the_reference_graphs():
    g = load_golden("g1_sampler")
    for p in ("a", "b"):
        src, dst, eidx, ts = (g[p + k] for k in ("_src", "_dst", "_eidx", "_ts"))
        n = int(max(src.max(), dst.max())) + 1
        want = build_adjacency(src, dst, eidx, ts)
        assert R.csr_equal(R.build(src, dst, eidx, ts, n), want) and R.csr_equal(R.build_fast(src, dst, eidx, ts, n), want)


def test_signed_zeros_tie_and_keep_their_bits():
    """The example of the rule: +0.0 (edge 1) stays in front of -0.0 (edge 2) whether or not the log is chronological, and the
    stored timestamps keep their sign bits."""
    for chrono in (True, False):
        src, dst, eidx, ts, n = R.signed_zero_example(chrono)
        indptr, nbr, eid, t = R.build(src, dst, eidx, ts, n)
        assert eid[indptr[1]:indptr[2]].tolist() == [1, 2, 3]
        assert eid[indptr[3]:indptr[4]].tolist() == ([1, 2, 3, 4] if chrono else [1, 2, 4, 3])
        assert np.signbit(t[indptr[1]:indptr[2]]).tolist() == [False, True, False]
    k = R.sort_keys(np.array([0.0, -0.0, 5e-324, -5e-324]))
    assert k[0] == k[1] and k[3] < k[0] < k[2]
    for chrono in (True, False):
        src, dst, eidx, ts, n = R.signed_zero_log(3000, chrono)
        assert (np.flatnonzero(ts[:-1] > ts[1:]).size == 0) == chrono
        z = ts == 0
        for v in range(1, 12):                                              # both signs meet inside every hub row
            own = z & ((src == v) | (dst == v))
            assert np.signbit(ts[own]).any() and not np.signbit(ts[own]).all()


def test_generators_keep_their_promises():
    x = np.array([-np.inf, -1e300, -R.STAMP, -1.5, -5e-324, -0.0, 0.0, 5e-324, 1.0, R.STAMP, R.STAMP + 0.25, np.inf])
    k = R.sort_keys(x)
    assert np.all(k[:-1] <= k[1:]) and (k[:-1] == k[1:]).sum() == 1          # ascending doubles == ascending keys; one tie: the zeros
    for E in (2, 33, 1025):
        c = R.chronological_with_ties(E, E)
        assert np.all(c[:-1] <= c[1:]) and (E < 33 or (c[:-1] == c[1:]).sum() > E // 3)
        assert R.inversion_places(E) == sorted({0, (E - 2) // 2, E - 2})
        for at in R.inversion_places(E):
            assert np.flatnonzero(np.diff(R.one_inversion(E, at, E)) < 0).tolist() == [at]
    for kbyte in range(8):
        ts = R.byte_decides(kbyte, 3000)
        key = R.sort_keys(ts)
        assert np.flatnonzero(ts[:-1] > ts[1:]).size > 100
        for neg in (False, True):
            ks = np.unique(key[np.signbit(ts) == neg])
            assert len(ks) == 7, "seven values per sign"
            differing = np.bitwise_or.reduce(ks ^ ks[0])
            assert differing != 0 and (int(differing) & ~(0xFF << (8 * kbyte))) == 0, "a byte other than %d differs" % kbyte
    ev = R.edge_values(3000)
    sub = np.abs(ev) < 2.2250738585072014e-308
    assert np.isposinf(ev).any() and np.isneginf(ev).any() and (sub & (ev != 0)).any() and not np.isnan(ev).any()
    assert ((ev == 0) & np.signbit(ev)).any() and ((ev == 0) & ~np.signbit(ev)).any()
    assert np.any((np.abs(ev) > 1e13) & (np.abs(ev) < 1e15) & (ev != np.floor(ev)))
    for n, passes in zip(R.OWNER_TABLES, R.OWNER_PASSES):
        pool = R.id_pool(n)
        assert pool.min() == 0 and pool.max() == n - 1 and R.owner_passes(n) == passes
        for b in range(passes if n > 1 else 0):                             # a pair that differs in byte b alone, per pass
            x = pool[:, None] ^ pool[None, :]
            assert np.any((x != 0) & ((x & ~(0xFF << (8 * b))) == 0)), (n, b)
        src, dst, _ = R.edges(3000, n)
        assert set(pool.tolist()) <= set(src.tolist()) | set(dst.tolist()) and (n > 2 or (src == dst).any())


# ------------------------------------------------------------------------------------------------ append
def _append_cases():
    return ([("counts-%d-%d" % c, R.append_counts_case(*c)) for c in R.APPEND_COUNTS]
            + [("shapes", R.append_shapes_case()), ("ties", R.append_ties_case())])


@pytest.mark.parametrize("cid,c", _append_cases(), ids=[c[0] for c in _append_cases()])
def test_append_model_equals_a_rebuild(cid, c):
    old = R.build(*c["old"], c["n_old"])
    got = R.append(old, c["n_old"], *c["new"], c["n_nodes"])
    both = [np.concatenate([a, b]) for a, b in zip(c["old"], c["new"])]
    assert R.csr_equal(got, R.build(*both, c["n_nodes"])) and R.csr_equal(got, R.build_fast(*both, c["n_nodes"]))
    assert got[0][c["n_nodes"]] == 2 * len(both[0])


def test_append_cases_hold_the_shapes_they_name():
    c = R.append_shapes_case()
    o, a = R.build(*c["old"], c["n_old"])[0], R.build(*c["new"], c["n_nodes"])[0]
    ol = lambda v: int(o[v + 1] - o[v]) if v < c["n_old"] else 0
    al = lambda v: int(a[v + 1] - a[v])
    assert (ol(0), al(0)) == (0, 0) and ol(1) == 0 and al(1) == 9 and ol(2) == 40 and al(2) == 0
    assert ol(3) == 100 and al(3) == 70 and ol(4) == 5000 and al(4) == 300 and ol(9) > 64 and al(9) == 0
    assert all(ol(v) == 0 and al(v) == 3 for v in (10, 11, 12)) and min(ol(5), al(5)) > 64
    for n_old, n in R.APPEND_COUNTS:
        c = R.append_counts_case(n_old, n)
        o, a = R.build(*c["old"], n_old)[0], R.build(*c["new"], n)[0]
        assert np.any(np.diff(o) == 0) and np.all(np.diff(a)[n_old:] > 0)
        assert np.intersect1d(c["old"][3], c["new"][3]).size >= 4           # old and new tie
    assert sorted({(n + 1) % 4 for _, n in R.APPEND_COUNTS}) == [0, 1] and sorted({n - o for o, n in R.APPEND_COUNTS}) == [0, 1, 5]
    # the tie row, written out: new entries behind the WHOLE old group of their timestamp
    c = R.append_ties_case()
    got = R.append(R.build(*c["old"], 7), 7, *c["new"], 7)
    row = lambda v: (got[3][got[0][v]:got[0][v + 1]], got[2][got[0][v]:got[0][v + 1]])
    t, e = row(1)
    assert t.tolist() == [0, 1, 1, 2, 2, 2, 2, 2, 3, 4, 5, 5, 5, 9]
    new_ids = set(c["new"][2].tolist())
    assert [x in new_ids for x in e.tolist()] == [True, False, False, False, False, False, True, True, False, True, False, False, True, True]
    t, e = row(2)
    assert np.signbit(t).tolist() == [True, False, False, True, True, False] and [x in new_ids for x in e.tolist()] == [False] * 3 + [True] * 2 + [False]
    t, e = row(3)
    assert np.signbit(t).tolist() == [True, True, False, True, False, False] and [x in new_ids for x in e.tolist()] == [False] * 2 + [True] * 3 + [False]


# ------------------------------------------------------------------------------------------------ roots
@pytest.mark.parametrize("cid,B,lo,hi,reps", R.root_cases(), ids=[c[0] for c in R.root_cases()])
def test_roots_model_equals_the_slicing_statement(cid, B, lo, hi, reps):
    """roots = [src[lo:hi] | dst[lo:hi] | groups[g][lo:hi, :] ...], root_ts = the interaction's time per root."""
    src, dst, ts, groups = R.roots_case(B, lo, hi, reps)
    got_r, got_t = R.roots(src, dst, ts, lo, hi, groups, reps)
    want_r = np.concatenate([src[lo:hi], dst[lo:hi]] + [g.reshape(B, r)[lo:hi].reshape(-1) for g, r in zip(groups, reps)])
    want_t = np.concatenate([ts[lo:hi], ts[lo:hi]] + [np.repeat(ts[lo:hi], r) for r in reps])
    assert got_r.dtype == np.int32 and np.array_equal(got_r, want_r) and np.array_equal(R.bits64(got_t), R.bits64(want_t))
    assert len(got_r) == (hi - lo) * (2 + sum(reps)) and got_r.min() > 0 and got_t.min() > 1e13, "a sentinel row was read"
    assert np.any(ts[lo:hi] != np.floor(ts[lo:hi])) or hi - lo < 4


def test_root_cases_cover_the_totals_they_name():
    total = {cid: (hi - lo) * (2 + sum(reps)) for cid, B, lo, hi, reps in R.root_cases()}
    assert (total["total255"], total["total256"], total["total257"]) == (255, 256, 257) and total["grid-stride"] > 1024 * 256
    assert {len(reps) for _, _, _, _, reps in R.root_cases()} == {0, 1, 2, 4}
    assert any(lo > 0 and hi < B for _, B, lo, hi, _ in R.root_cases()) and any(hi - lo == 1 for _, _, lo, hi, _ in R.root_cases())


# ------------------------------------------------------------------------------------------------ the NaN guard
def test_timestamp_guard_refuses_nan_and_nothing_else():
    ok = np.array([-np.inf, -0.0, 0.0, 5e-324, R.STAMP, np.inf])
    NF._check_timestamps(ok)
    NF._check_timestamps(np.zeros(0))
    NF._check_timestamps([1, 2, 3])
    for nan in (np.nan, -np.nan, np.array([0xFFF8000000000001], np.uint64).view(f64)[0], np.array([0x7FF0000000000001], np.uint64).view(f64)[0]):
        bad = ok.copy()
        bad[3] = nan
        with pytest.raises(ValueError, match="NaN.*position 3"):
            NF._check_timestamps(bad)


def test_device_build_and_append_refuse_nan_before_they_touch_the_device():
    """ValueError, not the PfoError of a missing device and not a launch: the helper runs first.  The host build is as it was."""
    src, dst, eidx = np.array([1, 2, 3]), np.array([4, 4, 5]), np.array([2, 3, 1])
    bad = np.array([1.0, np.nan, 2.0])
    with pytest.raises(ValueError, match="NaN"):
        NF.build_csr_device(src, dst, eidx, bad, "cuda:0")
    nf = NF.NeighborFinder.from_arrays(src, dst, eidx, np.array([1.0, 1.5, 2.0]))
    before = nf._version
    with pytest.raises(ValueError, match="NaN"):
        nf.append(src, dst, eidx + 3, bad, device="cuda:0")
    assert nf._version == before and nf.n_nodes == 6
    assert len(NF.build_csr(src, dst, eidx, bad)[3]) == 6


# ------------------------------------------------------------------------------------------------ the plan query
def test_csr_build_plan_states_tiles_owner_passes_and_sweeps():
    lib = _lib.load()
    for E in R.BUILD_EDGE_SIZES + [0, 2, 3000, R.TWO_SWEEP_E]:
        for n, passes in zip(R.OWNER_TABLES, R.OWNER_PASSES):
            tiles = max(1, -(-2 * E // 1024))
            assert _lib.csr_build_plan(E, n) == (tiles, passes, lib.pfo_debug_scan_sweeps(256 * tiles)), (E, n)
    assert [_lib.csr_build_plan(E, 40)[0] for E in (511, 512, 513, 1024, 1025)] == [1, 1, 2, 2, 3]
    assert _lib.csr_build_plan(R.TWO_SWEEP_E, 5000) == (4098, 2, 2) and _lib.csr_build_plan((1 << 21) - 1000, 5000)[2] == 1
    assert _lib.csr_build_plan(5, (1 << 31) - 1)[1] == 4
