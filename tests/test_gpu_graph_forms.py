"""Every graph-side launcher - pfo_csr_build, pfo_csr_append (csrc/csr.hip), pfo_roots_assemble (csrc/misc.hip) - called alone
through the C ABI and held to the host model of tests/csr_ref.py (DESIGN.md "Graph-side launchers under test").

Each case
  * asserts what pfo_debug_csr_build_plan says the build will launch (tiles, owner passes, sweeps of the histogram scan) before it
    launches, so that a dispatch change cannot quietly turn two cases into one,
  * gives every output - and the build's workspace - a canary and a 16-element tail that are compared by bits,
  * ends every input in slack and keeps every index in range over its whole allocation: a wrong case gives a wrong array,
    never a stray access.

Everything here is integers and copies: every comparison is bit for bit (timestamps by their 64 bits: a -0.0 that went in comes
out as -0.0).  There are no tolerances.  The append cases take their add-CSR from the host model, so that an error of the build
can neither hide nor fake an error of the merge."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

import pfotgnrec_amd as P
from pfotgnrec_amd import _lib
import csr_ref as R

DEV = "cuda:0"
f64 = np.float64
TAIL = 16
ISENT = -0x5A5A5A5
LSENT = -0x5A5A5A5A5A5A5A5
BSENT = 0xAB
TIMES = {}                 # case -> seconds of the launch and of the whole test body (printed by the last test)
PLANS_SEEN = set()


@pytest.fixture(autouse=True)
def stop_after_a_gpu_error():
    """A kernel that faulted leaves the device in an error state: the run ends there instead of launching more on it."""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:                                             # noqa: BLE001 - whatever the runtime raises
        pytest.exit("the GPU reported an error (%s): nothing more is launched" % e, returncode=3)


def canary64(n):
    return (np.uint64(0x7FF8000000000000) | (np.arange(n, dtype=np.uint64) + np.uint64(1))).view(np.float64)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.itemsize])


def same_bits(a, b):
    return np.array_equal(bits(a), bits(np.ascontiguousarray(b, a.dtype)))


class Bufs:
    """Device copies of a case's arrays, kept alive for the launch.  Inputs end in 64 elements of slack (NaN behind floats, 0 -
    an in-range index - behind the rest); an output holds exactly the array given (a canary with its tail)."""

    def __init__(self):
        self.keep = []

    def put(self, a, dtype=None):
        a = np.ascontiguousarray(a, dtype).reshape(-1)
        t = torch.full((a.size + 64,), float("nan") if a.dtype.kind == "f" else 0, dtype=getattr(torch, a.dtype.name), device=DEV)
        if a.size:
            t[:a.size] = torch.from_numpy(a).to(DEV)
        self.keep.append(t)
        return t.data_ptr()

    def out(self, a):
        t = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(DEV)
        self.keep.append(t)
        return t.data_ptr(), t


def call(name, *args):
    _lib.call(name, *args, _lib.stream_ptr())
    torch.cuda.synchronize()


def first_diff(got, want):
    d = np.flatnonzero(bits(got) != bits(np.ascontiguousarray(want, got.dtype)))
    return "equal" if not len(d) else "%d of %d differ, the first at %d: got %r, want %r" % (len(d), len(got), d[0], got[d[0]], np.asarray(want)[d[0]])


def hold_csr(tag, got, want, n_nodes, total):
    """got: the four output arrays with their tails as the launch left them; want: the model's CSR."""
    ptr, nbr, eid, ts = got
    assert len(want[0]) == n_nodes + 1 and len(want[1]) == total
    assert np.array_equal(ptr[:n_nodes + 1], want[0]), "%s indptr: %s" % (tag, first_diff(ptr[:n_nodes + 1], want[0]))
    assert int(ptr[n_nodes]) == total, "%s: the sentinel indptr[n_nodes] is not the total" % tag
    assert np.array_equal(nbr[:total], want[1]), "%s nbr: %s" % (tag, first_diff(nbr[:total], want[1]))
    assert np.array_equal(eid[:total], want[2]), "%s eidx: %s" % (tag, first_diff(eid[:total], want[2]))
    assert same_bits(ts[:total], want[3]), "%s ts (by bits): %s" % (tag, first_diff(ts[:total], want[3]))
    assert np.all(ptr[n_nodes + 1:] == LSENT) and np.all(nbr[total:] == ISENT) and np.all(eid[total:] == ISENT - 1), tag + ": a tail was written"
    assert same_bits(ts[total:], canary64(total + TAIL)[total:]), tag + ": the ts tail was written"


def csr_outputs(b, n_nodes, total):
    return [b.out(np.full(n_nodes + 1 + TAIL, LSENT, np.int64)), b.out(np.full(total + TAIL, ISENT, np.int32)),
            b.out(np.full(total + TAIL, ISENT - 1, np.int32)), b.out(canary64(total + TAIL))]


# ------------------------------------------------------------------------------------------------ build
def run_build(tag, src, dst, eidx, ts, n_nodes, plan):
    """Asserts the plan, launches pfo_csr_build alone -> the four outputs with their tails."""
    E = len(src)
    assert _lib.csr_build_plan(E, n_nodes) == plan, "%s: the build would launch %r, the case is about %r" % (tag, _lib.csr_build_plan(E, n_nodes), plan)
    PLANS_SEEN.add("owner passes %d" % plan[1])
    PLANS_SEEN.add("scan sweeps %d" % plan[2])
    if E:
        assert min(src.min(), dst.min()) >= 0 and max(src.max(), dst.max()) < n_nodes and not np.isnan(ts).any()
        PLANS_SEEN.add("timestamp passes " + ("run" if np.any(ts[:-1] > ts[1:]) else "skipped"))
    b = Bufs()
    nbytes = int(_lib.byte_count("pfo_csr_build_workspace_bytes", E, n_nodes))
    p_ws, ws = b.out(np.full(nbytes + TAIL, BSENT, np.uint8))
    outs = csr_outputs(b, n_nodes, 2 * E)
    t0 = time.perf_counter()
    call("pfo_csr_build", b.put(src, np.int32), b.put(dst, np.int32), b.put(eidx, np.int32), b.put(ts, f64), E, n_nodes,
         *[p for p, _ in outs], p_ws, nbytes)
    TIMES[tag + " launch"] = time.perf_counter() - t0
    assert np.all(ws[nbytes:].cpu().numpy() == BSENT), tag + ": the workspace tail was written"
    return [t.cpu().numpy() for _, t in outs]


def check_build(tag, src, dst, eidx, ts, n_nodes, plan, model=R.build):
    t0 = time.perf_counter()
    got = run_build(tag, src, dst, eidx, ts, n_nodes, plan)
    hold_csr(tag, got, model(src, dst, eidx, ts, n_nodes), n_nodes, 2 * len(src))
    TIMES[tag] = time.perf_counter() - t0
    return got


def tiles_of(E):
    return max(1, -(-2 * E // 1024))


@pytest.mark.parametrize("E,inverted", [(E, inv) for E in R.BUILD_EDGE_SIZES for inv in (False, True) if E >= 2 or not inv],
                         ids=lambda v: ("inverted" if v else "chronological") if isinstance(v, bool) else str(v))
def test_build_tile_and_step_edges(E, inverted):
    """2E on and beside the 64-lane step, the 1024-entry tile and two tiles; once with the timestamp passes skipped, once with
    one inversion in the middle of the log (all eight run).  (E = 1 has no pair to invert; the shortest descending log, two
    edges, is test_build_inversion_placement's E = 2.)"""
    src, dst, eidx = R.edges(E, 40, E)
    ts = R.one_inversion(E, (E - 2) // 2, E) if inverted else R.chronological_with_ties(E, E)
    assert bool(np.any(ts[:-1] > ts[1:])) == inverted
    check_build("edges E%d %s" % (E, "inverted" if inverted else "chronological"), src, dst, eidx, ts, 40, (tiles_of(E), 1, 1))


@pytest.mark.parametrize("E,at", [(E, at) for E in (2, 33, 1025, 3000) for at in R.inversion_places(E)])
def test_build_inversion_placement(E, at):
    """The ONLY descending pair is the first, a middle or the last one: a sortedness check that stops one pair short (or starts
    one late) skips the timestamp passes and emits the log's order."""
    src, dst, eidx = R.edges(E, 40, E + at)
    ts = R.one_inversion(E, at, E)
    assert np.flatnonzero(ts[:-1] > ts[1:]).tolist() == [at]
    check_build("inversion E%d at %d" % (E, at), src, dst, eidx, ts, 40, (tiles_of(E), 1, 1))


@pytest.mark.parametrize("n_nodes,passes", list(zip(R.OWNER_TABLES, R.OWNER_PASSES)), ids=[str(n) for n in R.OWNER_TABLES])
def test_build_owner_passes(n_nodes, passes):
    """One owner pass per byte of the largest id: the ids are 0, the largest one and values differing from these and from each
    other in one byte alone, for every byte (csr_ref.id_pool); n_nodes = 1 is all self-loops.  Timestamps tie heavily and are
    not chronological, so an owner pass that is not stable shows as well."""
    E = 3000
    src, dst, eidx = R.edges(E, n_nodes, n_nodes % 97)
    assert max(src.max(), dst.max()) == n_nodes - 1 and (n_nodes > 1 or np.all(src == dst))
    check_build("owner table %d" % n_nodes, src, dst, eidx, R.edge_values(E, 2), n_nodes, (tiles_of(E), passes, 1))


@pytest.mark.parametrize("k", list(range(8)) + ["edge-values"])
def test_build_each_timestamp_byte(k):
    """byte_decides(k): inside a sign the keys differ in byte k alone, so pass k alone orders them - and must keep the edge
    order of the ties the seven values per sign leave.  edge-values: infinities, subnormals, both zeros, yyyymmddHHMMSS."""
    E, n = 3000, 300
    src, dst, eidx = R.edges(E, n, 11 if k == "edge-values" else k)
    ts = R.edge_values(E) if k == "edge-values" else R.byte_decides(k, E)
    check_build("timestamp byte %s" % k, src, dst, eidx, ts, n, (tiles_of(E), 2, 1))


def test_build_two_sweep_scan():
    """256 * tiles > 2^20: the scan over the tile histograms takes a second sweep of block totals, in all ten passes."""
    src, dst, eidx, ts, n = R.two_sweep_case()
    E = len(src)
    assert E == R.TWO_SWEEP_E and _lib.load().pfo_debug_scan_sweeps(256 * tiles_of(E)) == 2 and np.any(ts[:-1] > ts[1:])
    check_build("two-sweep scan", src, dst, eidx, ts, n, (4098, 2, 2), model=R.build_fast)


@pytest.mark.parametrize("n_nodes", [1, 5, 1025])
def test_build_no_edges(n_nodes):
    got = run_build("no edges", np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, f64), n_nodes,
                    (1, R.owner_passes(n_nodes), 1))
    hold_csr("no edges", got, (np.zeros(n_nodes + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, f64)), n_nodes, 0)


@pytest.mark.parametrize("log", ["example", "hubs"])
def test_build_signed_zeros(log):
    """-0.0 and +0.0 are ONE timestamp (IEEE, the host build, the reference's sorted()): a tie, kept in edge order, whether the
    timestamp passes run or are skipped; and the emitted ts keeps the sign bit it was stored with."""
    zero_part = []
    for chrono in (True, False):
        src, dst, eidx, ts, n = R.signed_zero_example(chrono) if log == "example" else R.signed_zero_log(3000, chrono)
        assert bool(np.any(ts[:-1] > ts[1:])) != chrono and np.signbit(ts[ts == 0]).any() and not np.signbit(ts[ts == 0]).all()
        got = check_build("signed zeros %s %s" % (log, "chronological" if chrono else "inverted"), src, dst, eidx, ts, n,
                          (tiles_of(len(src)), 1, 1))
        z = got[3][:2 * len(src)] == 0
        assert np.signbit(got[3][:2 * len(src)][z]).any()
        zero_part.append((got[1][:2 * len(src)][z], got[2][:2 * len(src)][z], bits(got[3][:2 * len(src)][z])))
    assert all(np.array_equal(a, b) for a, b in zip(*zero_part)), "the zeros' order depends on an inversion elsewhere in the log"


# ------------------------------------------------------------------------------------------------ append
def run_append(tag, old, n_old, add, n_nodes):
    b = Bufs()
    total = len(old[1]) + len(add[1])
    assert len(old[0]) == n_old + 1 and len(add[0]) == n_nodes + 1 and old[0][-1] == len(old[1]) and add[0][-1] == len(add[1])
    outs = csr_outputs(b, n_nodes, total)
    ins = [b.put(c[0], np.int64) for c in (old, add)], [[b.put(c[1], np.int32), b.put(c[2], np.int32), b.put(c[3], f64)] for c in (old, add)]
    call("pfo_csr_append", ins[0][0], *ins[1][0], n_old, ins[0][1], *ins[1][1], n_nodes, *[p for p, _ in outs])
    return [t.cpu().numpy() for _, t in outs]


def check_append(tag, c):
    old = R.build(*c["old"], c["n_old"])
    add = R.build(*c["new"], c["n_nodes"])                              # the HOST model's add-CSR: pfo_csr_build is not involved
    want = R.append(old, c["n_old"], *c["new"], c["n_nodes"])
    got = run_append(tag, old, c["n_old"], add, c["n_nodes"])
    hold_csr(tag, got, want, c["n_nodes"], len(old[1]) + len(add[1]))


@pytest.mark.parametrize("n_old,n_nodes", R.APPEND_COUNTS)
def test_append_node_counts(n_old, n_nodes):
    """The table stays, grows by 1 and by 5; n_nodes + 1 rows (the sentinel's included) fill the last workgroup of four exactly
    and spill one into the next; rows without old entries, rows without new ones, new nodes with rows."""
    check_append("append counts %d -> %d" % (n_old, n_nodes), R.append_counts_case(n_old, n_nodes))


def test_append_row_shapes():
    """Old empty / new empty / both empty / both longer than the 64 lanes / a hub of 5000 receiving 300; new nodes get rows."""
    check_append("append shapes", R.append_shapes_case())


def test_append_ties():
    """New entries land behind the WHOLE old group of their timestamp, in front of every later old entry; -0.0 against +0.0
    across old and new is such a tie."""
    check_append("append ties", R.append_ties_case())


@pytest.mark.parametrize("chrono", [True, False], ids=["chronological", "inverted"])
def test_append_composition_through_neighbor_finder(chrono):
    """NeighborFinder.append (pfo_csr_build of the batch, then pfo_csr_append) on the signed-zero log: a third built, grown twice
    - the one-shot model, zeros in edge order with their bits."""
    src, dst, eidx, ts, _ = R.signed_zero_log(3000, chrono)
    E = len(src)
    cuts = [0, E // 3, 2 * E // 3, E]
    nf = P.NeighborFinder.from_arrays(src[:cuts[1]], dst[:cuts[1]], eidx[:cuts[1]], ts[:cuts[1]], device=DEV)
    for a, b in zip(cuts[1:-1], cuts[2:]):
        nf.append(src[a:b], dst[a:b], eidx[a:b], ts[a:b], device=DEV)
    want = R.build(src, dst, eidx, ts, nf.n_nodes)
    assert nf.n_nodes == int(max(src.max(), dst.max())) + 1
    assert R.csr_equal((nf.indptr, nf.nbr, nf.eidx, nf.ts), want), [first_diff(np.asarray(g), w) for g, w in zip((nf.indptr, nf.nbr, nf.eidx, nf.ts), want)]


# ------------------------------------------------------------------------------------------------ roots
@pytest.mark.parametrize("cid,B,lo,hi,reps", R.root_cases(), ids=[c[0] for c in R.root_cases()])
def test_roots_assemble(cid, B, lo, hi, reps):
    """[src | dst | group 0 | ...] of interactions [lo, hi) with the interaction's time per root; the group arrays hold B rows,
    indexed by the absolute interaction, with sentinels in the rows outside the shard."""
    src, dst, ts, groups = R.roots_case(B, lo, hi, reps)
    want_r, want_t = R.roots(src, dst, ts, lo, hi, groups, reps)
    n = len(want_r)
    assert n == (hi - lo) * (2 + sum(reps)) and 0 <= lo < hi <= B and all(len(g) == B * r for g, r in zip(groups, reps))
    b = Bufs()
    ng = len(reps)
    gptr = (C.c_void_p * max(1, ng))(*[b.put(g, np.int32) for g in groups])
    greps = (C.c_int32 * max(1, ng))(*reps)
    p_r, r = b.out(np.full(n + TAIL, ISENT, np.int32))
    p_t, t = b.out(canary64(n + TAIL))
    call("pfo_roots_assemble", b.put(src, np.int32), b.put(dst, np.int32), b.put(ts, f64), lo, hi, gptr, greps, ng, p_r, p_t)
    r, t = r.cpu().numpy(), t.cpu().numpy()
    assert np.array_equal(r[:n], want_r), "roots: " + first_diff(r[:n], want_r)
    assert same_bits(t[:n], want_t), "root_ts: " + first_diff(t[:n], want_t)
    assert np.all(r[n:] == ISENT) and same_bits(t[n:], canary64(n + TAIL)[n:]), "a tail was written"


def test_zz_every_plan_was_reached_and_times():
    """Runs last in the file: the plans the build cases reached (when the whole file ran) and the wall times of the largest."""
    print("TIMES " + "; ".join("%s %.3f s" % (k, v) for k, v in sorted(TIMES.items()) if v >= 0.05 or "two-sweep" in k or "16777217" in k))
    print("PLANS " + "; ".join(sorted(PLANS_SEEN)))
    if len(TIMES) >= 60:                                                 # the whole file ran, not a selection
        want = {"owner passes %d" % p for p in (1, 2, 3, 4)} | {"scan sweeps 1", "scan sweeps 2", "timestamp passes run", "timestamp passes skipped"}
        assert want <= PLANS_SEEN, sorted(want - PLANS_SEEN)
