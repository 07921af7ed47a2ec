"""Error measures shared by the parity tests."""
import numpy as np


def relerr(a, b):
    """max |a - b| / max |b|: the project's bar for embeddings (BASELINE.json north_star) is stated in this norm."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-12)


def row_relerr(a, b):
    """max_i ||a_i - b_i||_2 / max(||b_i||_2, floor) over the rows of [n, D] arrays.  ``relerr`` divides by the largest entry
    of the whole array: a whole row of small values could be wrong and pass it.  floor = 1e-3 x the median row norm of the
    reference keeps exact-zero rows finite; where more than half of the reference's rows are exactly zero (the memory table a
    few batches after a reset) that median is 0 and the median of the non-zero rows is taken instead."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    a, b = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    if len(b) == 0:
        return 0.0
    norms = np.linalg.norm(b, axis=1)
    med = np.median(norms)
    if med == 0 and (norms > 0).any():
        med = np.median(norms[norms > 0])
    floor = 1e-3 * med
    return float((np.linalg.norm(a - b, axis=1) / np.maximum(np.maximum(norms, floor), 1e-300)).max())


# Per-row bar, beside every embedding / memory ``relerr`` < 1e-4 of the golden comparisons.  Measured first, oracle against the
# reference's fixtures on the CPU (fp32 numpy restatement against torch): the largest per-row error over every g5, g8 and g10
# fixture is 5.3e-7 (g5_step_L2_mem embeddings; memory rows <= 2.6e-7, pending-message rows <= 1e-7, g10 embeddings <= 4.0e-7).
# That is far below the project's 1e-4, so the bar is the project's own figure and not a measured one.
ROW_RTOL = 1e-4
