"""numpy restatement of the retention window: the reference of tests/test_expire_cpu.py and
tests/test_gpu_expire.py.  Nothing here knows how the device does it: a boolean mask, a cumsum, ``np.unique``."""
import numpy as np


def row_of(indptr):
    """The owning row of every flat adjacency position."""
    indptr = np.asarray(indptr, np.int64)
    return np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr))


def expire_csr(indptr, nbr, eidx, ts, cutoff):
    """Entries with ``ts < cutoff`` (strict, fp64) leave: mask the flat arrays with ``ts >= cutoff``, re-accumulate indptr.
    Returns (indptr i64[n + 1], nbr i32, eidx i32, ts f64) and the mask."""
    indptr, ts = np.asarray(indptr, np.int64), np.asarray(ts, np.float64)
    keep = ts >= np.float64(cutoff)
    counts = np.bincount(row_of(indptr)[keep], minlength=len(indptr) - 1)
    new_ptr = np.zeros(len(indptr), np.int64)
    np.cumsum(counts, out=new_ptr[1:])
    return (new_ptr, np.asarray(nbr, np.int32)[keep], np.asarray(eidx, np.int32)[keep], ts[keep]), keep


def release_rule(n_rows, finders, cutoff):
    """``finders``: (eidx, ts) of every adjacency taking part, BEFORE the expiry.  Row r >= 1 is released iff some expired
    entry names it and no surviving entry does; rows nobody names stay; row 0 stays.  Returns (remap i32[n_rows], n_keep):
    kept rows renumbered densely in order, released rows -1."""
    expired = np.unique(np.concatenate([np.asarray(e)[np.asarray(t, np.float64) < cutoff] for e, t in finders] + [np.zeros(0, np.int32)]))
    alive = np.unique(np.concatenate([np.asarray(e)[np.asarray(t, np.float64) >= cutoff] for e, t in finders] + [np.zeros(0, np.int32)]))
    released = np.setdiff1d(expired, alive)
    released = released[released >= 1]
    keep = np.ones(n_rows, bool)
    keep[released] = False
    remap = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    return remap, int(keep.sum())


def compact_table(table, remap, capacity=None):
    """The kept rows in order, zero rows behind them up to ``capacity`` (default: the old row count)."""
    table = np.asarray(table, np.float32)
    kept = table[remap >= 0]
    out = np.zeros((table.shape[0] if capacity is None else capacity, table.shape[1]), np.float32)
    out[:kept.shape[0]] = kept
    return out


def expire_all(n_rows, finders_csr, cutoff):
    """The whole of ``TGN.expire`` on host arrays: ``finders_csr`` is a list of (indptr, nbr, eidx, ts).  Returns the expired
    and remapped CSRs, remap, n_keep and the number of entries dropped."""
    remap, n_keep = release_rule(n_rows, [(c[2], c[3]) for c in finders_csr], cutoff)
    out, dropped = [], 0
    for c in finders_csr:
        (p, n, e, t), keep = expire_csr(*c, cutoff)
        dropped += int((~keep).sum())
        out.append((p, n, remap[e].astype(np.int32), t))
    return out, remap, n_keep, dropped
