"""numpy restatement of erasure by node: the reference of tests/test_forget_cpu.py and tests/test_gpu_forget.py.
Nothing here knows how the device does it: a boolean mask, a cumsum, ``np.unique``."""
import numpy as np

from expire_ref import compact_table, row_of       # noqa: F401  (the table side is the retention window's)


def gone_of(n_nodes, ids):
    """u8[n_nodes], 1 = forgotten: ids outside [1, n_nodes) are skipped, duplicates are fine."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    gone = np.zeros(n_nodes, np.uint8)
    gone[ids[(ids >= 1) & (ids < n_nodes)]] = 1
    return gone


def dropped_mask(indptr, nbr, gone):
    """Entry i of row v is dropped iff gone[v] or gone[nbr[i]]; a neighbour id outside [0, n_nodes) counts as not gone."""
    gone = np.asarray(gone).astype(bool)
    n = len(gone)
    nbr = np.asarray(nbr, np.int64)
    inside = (nbr >= 0) & (nbr < n)
    by_nbr = np.zeros(len(nbr), bool)
    by_nbr[inside] = gone[nbr[inside]]
    return gone[row_of(indptr)] | by_nbr


def forget_csr(indptr, nbr, eidx, ts, gone):
    """Mask the flat arrays with the keep decision, re-accumulate indptr.  Returns (indptr i64[n + 1], nbr i32, eidx i32, ts f64)
    and the keep mask."""
    indptr = np.asarray(indptr, np.int64)
    keep = ~dropped_mask(indptr, nbr, gone)
    counts = np.bincount(row_of(indptr)[keep], minlength=len(indptr) - 1)
    new_ptr = np.zeros(len(indptr), np.int64)
    np.cumsum(counts, out=new_ptr[1:])
    return (new_ptr, np.asarray(nbr, np.int32)[keep], np.asarray(eidx, np.int32)[keep], np.asarray(ts, np.float64)[keep]), keep


def row_flags(n_rows, finders, gone):
    """``finders``: (indptr, nbr, eidx) of every adjacency taking part, BEFORE the removal.  flags[r] |= 1 when a dropped entry
    names row r, |= 2 when a surviving one does; entries outside [0, n_rows) are ignored."""
    flags = np.zeros(n_rows, np.int32)
    for indptr, nbr, eidx in finders:
        eidx = np.asarray(eidx, np.int64)
        drop = dropped_mask(indptr, nbr, gone)
        ok = (eidx >= 0) & (eidx < n_rows)
        flags[np.unique(eidx[ok & drop])] |= 1
        flags[np.unique(eidx[ok & ~drop])] |= 2
    return flags


def release_rule(n_rows, finders, gone):
    """Row r >= 1 is released iff some dropped entry names it and no surviving one does; rows nobody names stay; row 0 stays.
    Returns (remap i32[n_rows], n_keep): kept rows renumbered densely in order, released rows -1."""
    keep = row_flags(n_rows, finders, gone) != 1
    keep[0] = True
    remap = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    return remap, int(keep.sum())


def forget_all(n_rows, finders_csr, gone):
    """The graph and table side of ``TGN.forget`` on host arrays: ``finders_csr`` is a list of (indptr, nbr, eidx, ts).  Returns
    the swept and remapped CSRs, remap, n_keep and the number of entries dropped."""
    remap, n_keep = release_rule(n_rows, [c[:3] for c in finders_csr], gone)
    out, dropped = [], 0
    for c in finders_csr:
        (p, n, e, t), keep = forget_csr(*c, gone)
        dropped += int((~keep).sum())
        out.append((p, n, remap[e].astype(np.int32), t))
    return out, remap, n_keep, dropped


def reset_rows(tables, fills, gone):
    """Every row v with gone[v] of every table back to its fill; the other rows as they are."""
    sel = np.flatnonzero(np.asarray(gone))
    out = []
    for t, fill in zip(tables, fills):
        t = np.array(t)
        t[sel] = fill
        out.append(t)
    return out
