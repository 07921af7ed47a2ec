"""The graph-side launchers (pfo_csr_build, pfo_csr_append, pfo_roots_assemble) stated on the host, with the timestamp and
edge generators their CPU and GPU tests share (tests/test_csr_ref_cpu.py, tests/test_gpu_graph_forms.py).  numpy and plain
Python, no torch, no import of the package.

``build`` is written the way the reference states the adjacency (utils/utils.py:117-142): per node a list of
``(other, eidx, ts)`` in edge order - the edge's entry for its source first, then the one for its destination - and Python's
stable ``sorted(key=ts)`` over every list.  ``sorted`` compares floats the IEEE way: -0.0 and +0.0 are EQUAL, a tie that keeps
edge order, and every entry keeps the bits it came with.  ``build_fast`` is the vectorised twin for the cases whose size the
list form cannot afford; the CPU file holds the two together on every generator.

Everything here is integers and copies: all comparisons are bit for bit."""
import numpy as np

f64 = np.float64
STAMP = 20240131093000.5      # a yyyymmddHHMMSS timestamp with a fraction, exact in fp64: bits 0x42B26885D2F20880


def bits64(a):
    return np.ascontiguousarray(a, f64).view(np.uint64)


def csr_equal(a, b):
    """Two CSR tuples agree in dtype-independent values for the integers and in BITS for the timestamps."""
    return (len(a) == len(b) == 4 and all(np.asarray(x).shape == np.asarray(y).shape for x, y in zip(a, b))
            and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
            and np.array_equal(bits64(a[3]), bits64(b[3])))


# ------------------------------------------------------------------------------------------------ the models
def _rows_of(src, dst, eidx, ts):
    """{node: [(other, eidx, ts), ...] in edge order} over the nodes that own an entry (a dict: a table of 2^24 nodes costs
    nothing).  ts travels as a Python float, which is the same 64 bits."""
    rows = {}
    for s, d, e, t in zip(np.asarray(src).tolist(), np.asarray(dst).tolist(), np.asarray(eidx).tolist(), np.asarray(ts, f64).tolist()):
        rows.setdefault(s, []).append((d, e, t))
        rows.setdefault(d, []).append((s, e, t))
    return rows


def _flatten(rows, n_nodes):
    counts = np.zeros(n_nodes, np.int64)
    for v, r in rows.items():
        assert 0 <= v < n_nodes, "node id %d outside the table of %d" % (v, n_nodes)
        counts[v] = len(r)
    indptr = np.zeros(n_nodes + 1, np.int64)
    np.cumsum(counts, out=indptr[1:])
    flat = [x for v in sorted(rows) for x in rows[v]]
    return (indptr, np.array([x[0] for x in flat], np.int32), np.array([x[1] for x in flat], np.int32),
            np.array([x[2] for x in flat], f64))


def build(src, dst, eidx, ts, n_nodes):
    """-> (indptr i64[n_nodes + 1], nbr i32[2E], eidx i32[2E], ts f64[2E]): the list form."""
    rows = {v: sorted(r, key=lambda x: x[2]) for v, r in _rows_of(src, dst, eidx, ts).items()}
    return _flatten(rows, n_nodes)


def build_fast(src, dst, eidx, ts, n_nodes):
    """The vectorised twin: the 2E entries in edge order, a stable sort by timestamp, then a stable sort by owner."""
    src, dst, eidx, ts = np.asarray(src, np.int64), np.asarray(dst, np.int64), np.asarray(eidx, np.int64), np.asarray(ts, f64)
    E = len(src)
    owner, other = np.empty(2 * E, np.int64), np.empty(2 * E, np.int64)
    owner[0::2], owner[1::2] = src, dst
    other[0::2], other[1::2] = dst, src
    eid2, ts2 = np.repeat(eidx, 2), np.repeat(ts, 2)
    order = np.argsort(ts2, kind="stable")
    order = order[np.argsort(owner[order], kind="stable")]
    indptr = np.zeros(n_nodes + 1, np.int64)
    np.cumsum(np.bincount(owner, minlength=n_nodes), out=indptr[1:])
    assert len(indptr) == n_nodes + 1, "a node id outside the table"
    return indptr, other[order].astype(np.int32), eid2[order].astype(np.int32), ts2[order]


def rows_of_csr(csr, n_nodes):
    indptr, nbr, eidx, ts = csr
    nbr, eidx, ts = np.asarray(nbr).tolist(), np.asarray(eidx).tolist(), np.asarray(ts, f64).tolist()
    return {v: list(zip(nbr[indptr[v]:indptr[v + 1]], eidx[indptr[v]:indptr[v + 1]], ts[indptr[v]:indptr[v + 1]]))
            for v in range(n_nodes) if indptr[v + 1] > indptr[v]}


def merge_row(old, new):
    """One row of an append: both time-sorted; a new entry goes behind every old entry with ts <= its own (new edges are later
    in edge order) and in front of every old entry with a larger ts."""
    out, p = [], 0
    for x in new:
        while p < len(old) and old[p][2] <= x[2]:
            out.append(old[p])
            p += 1
        out.append(x)
    return out + old[p:]


def append(old_csr, n_old_nodes, src, dst, eidx, ts, n_nodes):
    """``build`` over [old edges ; new edges], stated on the rows of the old adjacency (n_old_nodes <= n_nodes rows)."""
    assert n_nodes >= n_old_nodes and len(old_csr[0]) == n_old_nodes + 1
    old = rows_of_csr(old_csr, n_old_nodes)
    new = rows_of_csr(build(src, dst, eidx, ts, n_nodes), n_nodes)
    return _flatten({v: merge_row(old.get(v, []), new.get(v, [])) for v in set(old) | set(new)}, n_nodes)


def roots(src, dst, ts, lo, hi, groups, reps):
    """-> (roots i32[R], root_ts f64[R]), R = (hi - lo) (2 + sum reps): [src | dst | group 0 | group 1 ...] of interactions
    [lo, hi), group g row-major b x reps[g] read at the ABSOLUTE interaction index, every root with its interaction's time."""
    src, dst, ts = np.asarray(src).tolist(), np.asarray(dst).tolist(), np.asarray(ts, f64).tolist()
    r, t = [], []
    for i in range(lo, hi):
        r.append(src[i]); t.append(ts[i])
    for i in range(lo, hi):
        r.append(dst[i]); t.append(ts[i])
    for g, rep in zip(groups, reps):
        g = np.asarray(g).tolist()
        for i in range(lo, hi):
            for j in range(rep):
                r.append(g[i * rep + j]); t.append(ts[i])
    return np.array(r, np.int32).reshape(-1), np.array(t, f64).reshape(-1)


# ------------------------------------------------------------------------------------------------ timestamp generators
def sort_keys(ts):
    """The radix key of a timestamp, stated on the host: ascending keys == ascending doubles, the two zeros share one."""
    u = bits64(ts).copy()
    u[(u << np.uint64(1)) == 0] = 0
    neg = (u >> np.uint64(63)) == 1
    return np.where(neg, ~u, u | np.uint64(1 << 63))


def chronological_with_ties(E, seed=0):
    """Non-decreasing, about three entries per value, fractions and negative values included."""
    rs = np.random.RandomState(1000 + seed)
    return np.sort(rs.randint(-E // 6 - 1, E // 6 + 2, E)).astype(f64) * 0.25


def inversion_places(E):
    """The pairs (at, at + 1) the cases put their only inversion at: the first, a middle and the last one."""
    return sorted({0, (E - 2) // 2, E - 2})


def one_inversion(E, at, seed=0):
    """``chronological_with_ties`` with exactly ONE descending adjacent pair, (at, at + 1); every other pair ascends or ties."""
    assert E >= 2 and 0 <= at <= E - 2
    ts = chronological_with_ties(E, seed)
    ts[at + 1:] += 1.0                                # the pair differs ...
    ts[at], ts[at + 1] = ts[at + 1], ts[at]           # ... and swapping it leaves its neighbours in order
    d = np.flatnonzero(ts[:-1] > ts[1:])
    assert d.tolist() == [at]
    return ts


def byte_decides(k, E, seed=0):
    """Doubles of both signs whose sort keys differ, inside a sign, in byte ``k`` alone; seven values per sign, so ties are heavy;
    in random order (never chronological).  All finite: STAMP's exponent bits outside byte 7 are not all ones."""
    assert 0 <= k <= 7
    rs = np.random.RandomState(2000 + k + 8 * seed)
    base = int(bits64(np.array([STAMP]))[0])
    vals = rs.permutation(128 if k == 7 else 256)[:7].astype(np.uint64)          # (byte 7 holds the sign: 7 bits are free)
    pool = (np.uint64(base & ~(0xFF << (8 * k)) & (2 ** 64 - 1)) | (vals << np.uint64(8 * k)))
    if k == 7:
        pool = pool & np.uint64(2 ** 63 - 1)
    pool = np.concatenate([pool, pool | np.uint64(1 << 63)])
    ts = pool[rs.randint(0, len(pool), E)].view(f64)
    assert np.isfinite(ts).all()
    return ts


def edge_values(E, seed=0):
    """Negatives, both infinities, subnormals, the two zeros interleaved, yyyymmddHHMMSS magnitudes with fractions: drawn at
    random from a pool of 24, so ties are heavy, the zeros of both signs meet inside rows, and the log is not chronological."""
    rs = np.random.RandomState(3000 + seed)
    pool = np.array([0.0, -0.0, 0.0, -0.0, -np.inf, np.inf, 5e-324, -5e-324, 1.1e-308, -1.1e-308, 2.2250738585072014e-308, -1.5, -1e300, 1e300,
                     -STAMP, STAMP, STAMP + 0.25, STAMP + 0.5, 20240131093001.0, 20231231235959.75, 19991231235959.125, 1.0, -1.0, 0.5], f64)
    ts = pool[rs.randint(0, len(pool), E)]
    if E >= 2:
        ts[0], ts[1] = 1.0, -1.0                      # (not chronological whatever was drawn)
    return ts


def signed_zero_example(chronological):
    """The four-edge example: node 1's row holds +0.0 (edge 1) then -0.0 (edge 2) and must keep that order; the inversion of the
    other form (5.0 before 1.0) sits elsewhere in the log."""
    ts = [0.0, -0.0, 1.0, 5.0] if chronological else [0.0, -0.0, 5.0, 1.0]
    return np.array([1, 1, 1, 2]), np.array([3, 3, 3, 3]), np.array([1, 2, 3, 4]), np.array(ts, f64), 4


def signed_zero_log(E, chronological, seed=0):
    """Hub rows holding a long run of zeros of both signs between negative and positive times.  Chronological in the IEEE sense
    (the zeros tie); the other form swaps the timestamps of ONE pair far behind the zeros."""
    rs = np.random.RandomState(4000 + seed)
    n_neg, n_zero = E // 4, E // 2
    ts = np.concatenate([np.sort(rs.randint(-40, 0, n_neg)).astype(f64), np.where(rs.rand(n_zero) < 0.5, 0.0, -0.0),
                         np.sort(rs.randint(1, 40, E - n_neg - n_zero)).astype(f64)])
    if not chronological:
        at = E - 5
        ts[at + 1:] += 1.0
        ts[at], ts[at + 1] = ts[at + 1], ts[at]
    src, dst = rs.randint(1, 6, E), rs.randint(6, 12, E)                          # eleven hub rows
    return src, dst, rs.permutation(E) + 1, ts, 13


# ------------------------------------------------------------------------------------------------ edge generators
def id_pool(n_nodes):
    """Node ids that exercise every owner pass: 0, the largest id, and for every byte of the largest id values that differ in
    that byte alone (from 0, from each other and from the largest id)."""
    top = n_nodes - 1
    pool = {0, top}
    k = 0
    while (1 << (8 * k)) <= top:
        for m in (1, 2, 0x80, 0xFF):
            if (m << (8 * k)) <= top:
                pool.add(m << (8 * k))
            if 0 <= (top ^ (m << (8 * k))) <= top:
                pool.add(top ^ (m << (8 * k)))
        k += 1
    return np.array(sorted(pool), np.int64)


def edges(E, n_nodes, seed=0, pool=None):
    """-> src, dst, eidx: endpoints drawn from ``pool`` (default ``id_pool``: few ids, so rows are long and ties meet), every
    pool id named, some self-loops; eidx a permutation of 1..E - never arange, so an unstable sort shows."""
    rs = np.random.RandomState(5000 + seed)
    pool = id_pool(n_nodes) if pool is None else np.asarray(pool, np.int64)
    src, dst = pool[rs.randint(0, len(pool), E)], pool[rs.randint(0, len(pool), E)]
    m = min(E, len(pool))
    src[:m] = pool[:m]                                 # every id owns an entry when E allows
    return src, dst, rs.permutation(E) + 1


def owner_passes(n_nodes):
    """One pass per byte of the largest node id (at least one)."""
    return max(1, ((n_nodes - 1).bit_length() + 7) // 8)


BUILD_EDGE_SIZES = [1, 31, 32, 33, 511, 512, 513, 1024, 1025]                    # 2E on and beside 64, 1024 and 2048
OWNER_TABLES = [1, 2, 255, 256, 257, 65536, 65537, 1 << 24, (1 << 24) + 1]
OWNER_PASSES = [1, 1, 1, 1, 2, 2, 3, 3, 4]                                       # written down, not computed: the plan must say this
TWO_SWEEP_E = (1 << 21) + 1000                                                    # 256 * ceil(2E / 1024) = 1 049 088 > 2^20


def two_sweep_case():
    rs = np.random.RandomState(77)
    E, n_nodes = TWO_SWEEP_E, 5000
    src, dst = rs.randint(0, 4000, E), rs.randint(3000, n_nodes, E)
    ts = rs.randint(-12000, 50000, E).astype(f64) * 0.25                          # unsorted, ties, negatives, fractions
    return src, dst, rs.permutation(E) + 1, ts, n_nodes


# ------------------------------------------------------------------------------------------------ append cases
def _case(old, n_old, new, n_nodes):
    old, new = [tuple(np.asarray(a) for a in x) for x in (old, new)]
    return dict(old=old, n_old=n_old, new=new, n_nodes=n_nodes)


def append_counts_case(n_old, n_nodes, seed=0):
    """Random small tables: timestamps from a handful of values (old and new tie all the time), some nodes without old entries,
    some without new ones, every new node named."""
    rs = np.random.RandomState(6000 + 31 * n_old + n_nodes + seed)
    Eo, En = 5 * n_old, 4 * n_nodes
    quiet = rs.permutation(n_old)[:max(1, n_old // 4)]                              # nodes without old entries
    ids = np.setdiff1d(np.arange(n_old), quiet) if n_old > len(quiet) + 1 else np.arange(n_old)
    o_src, o_dst = ids[rs.randint(0, len(ids), Eo)], ids[rs.randint(0, len(ids), Eo)]
    o_ts = np.sort(rs.randint(0, 6, Eo)).astype(f64)
    perm = rs.permutation(Eo + En) + 1
    n_src, n_dst = rs.randint(0, n_nodes, En), rs.randint(n_old // 2, n_nodes, En)
    n_src[:n_nodes - n_old] = np.arange(n_old, n_nodes)
    n_ts = rs.randint(-1, 8, En).astype(f64)
    return _case((o_src, o_dst, perm[:Eo], o_ts), n_old, (n_src, n_dst, perm[Eo:], n_ts), n_nodes)


APPEND_COUNTS = [(7, 7), (8, 8), (7, 8), (6, 11), (7, 12), (203, 203), (202, 207)]    # same; +1; +5; n_nodes + 1 = 0 and 1 mod 4


def append_shapes_case():
    """Rows by shape.  0: no entry at all.  1: old empty, new not (its new edges name the NEW nodes 10, 11, 12).  2: old only.
    3: 100 old and 70 new entries.  4: a hub of 5000 old entries receiving 300.  5..9: the other endpoints."""
    rs = np.random.RandomState(61)
    o_src = np.concatenate([np.full(40, 2), np.full(100, 3), np.full(5000, 4)])
    o_dst = rs.randint(5, 10, len(o_src))
    o_ts = np.sort(rs.randint(0, 400, len(o_src))).astype(f64)
    n_src = np.concatenate([np.full(9, 1), np.full(70, 3), np.full(300, 4)])
    n_dst = np.concatenate([np.tile([10, 11, 12], 3), rs.randint(5, 9, 370)])       # (9 gets no new entry)
    n_ts = rs.randint(-5, 420, len(n_src)).astype(f64)
    perm = rs.permutation(len(o_src) + len(n_src)) + 1
    return _case((o_src, o_dst, perm[:len(o_src)], o_ts), 10, (n_src, n_dst, perm[len(o_src):], n_ts), 13)


def append_ties_case():
    """Row 1: new entries equal to an old tie group (behind the WHOLE group), older than every old entry, between old entries,
    equal to the last group, later than all.  Row 2: a new -0.0 against old +0.0s (an IEEE tie: behind them) and row 3 the
    other way round, with both zeros among the new ones.  Rows 4..6: the other endpoints, one per row."""
    o_ts = {1: [1, 1, 2, 2, 2, 3, 5, 5], 2: [-1, 0.0, 0.0, 1], 3: [-0.0, -0.0, 0.5]}
    n_ts = {1: [2, 0, 4, 5, 2, 9], 2: [-0.0, -0.0], 3: [0.0, -0.0, 0.0]}
    flat = lambda d: (np.concatenate([np.full(len(v), k) for k, v in d.items()]), np.concatenate([np.asarray(v, f64) for v in d.values()]))
    (o_src, o_t), (n_src, n_t) = flat(o_ts), flat(n_ts)
    perm = np.random.RandomState(62).permutation(len(o_src) + len(n_src)) + 1
    return _case((o_src, o_src + 3, perm[:len(o_src)], o_t), 7, (n_src, n_src + 3, perm[len(o_src):], n_t), 7)


# ------------------------------------------------------------------------------------------------ root cases
ROOT_REPS_UNEQUAL = (1, 7, 3, 20)
ROOT_SENTINEL = -77


def roots_case(B, lo, hi, reps, seed=0):
    """src, dst, ts and the group arrays over B interactions, with sentinels in every row outside [lo, hi) (a launcher that reads
    them shows it) and yyyymmddHHMMSS times with fractions."""
    rs = np.random.RandomState(7000 + seed + B + 13 * lo)
    inside = np.zeros(B, bool)
    inside[lo:hi] = True
    src, dst = rs.randint(1, 1 << 20, B), rs.randint(1 << 20, 1 << 30, B)
    ts = STAMP + np.sort(rs.randint(0, 4 * 86400, B)) * 0.25
    src[~inside], dst[~inside], ts[~inside] = ROOT_SENTINEL, ROOT_SENTINEL, -1.0
    groups = []
    for g, r in enumerate(reps):
        a = rs.randint(1, 1 << 30, (B, r))
        a[~inside] = ROOT_SENTINEL - 1 - g
        groups.append(a.reshape(-1).astype(np.int32))
    return src.astype(np.int32), dst.astype(np.int32), ts, groups


def root_cases():
    """(id, B, lo, hi, reps)."""
    out = []
    for ng in (0, 1, 2, 4):
        for kind, reps in (("equal", (3,) * ng), ("unequal", ROOT_REPS_UNEQUAL[:ng])):
            if ng == 0 and kind == "unequal":
                continue
            out.append(("g%d-%s-whole" % (ng, kind), 37, 0, 37, reps))
            out.append(("g%d-%s-shard" % (ng, kind), 37, 11, 30, reps))
    out.append(("b1-first", 5, 0, 1, ROOT_REPS_UNEQUAL))
    out.append(("b1-inner", 5, 3, 4, ROOT_REPS_UNEQUAL))
    out.append(("total255", 60, 4, 55, (3,)))                                      # 51 * 5
    out.append(("total256", 40, 5, 37, (3, 3)))                                    # 32 * 8
    out.append(("total257", 3, 1, 2, (1, 7, 3, 244)))                              # 1 * 257
    out.append(("grid-stride", 3010, 6, 3006, (1, 7, 3, 89)))                      # 3000 * 102 = 306 000 > 1024 * 256
    return out
