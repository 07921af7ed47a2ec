"""Error measures, bars and step helpers shared by the parity tests.  Importable without a GPU: the helpers that need the
package or the oracle import them when called."""
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


# ---------------------------------------------------------------------------- the step against the oracle (test_gpu_tgn_step.py)
RTOL_EMB = 1e-4      # BASELINE.json north_star: embeddings within 1e-4 relative
# time-encoder gradients are sums of terms scaled by dt ~ 1e7 that cancel to a small remainder: relative to
# max|grad| both the reference's fp32 autograd sum and any re-association of it carry ~1e-3 evaluation noise
RTOL_GRAD_TIME = 3e-3
# oracle comparisons on random parameters: a fc1 pre-activation within rounding distance of 0 flips relu' between
# the two implementations and perturbs every upstream gradient by ~1e-3 (observed once in the D=64 case; all other
# tensors / cases agree to ~1e-5, tools/grad_error_survey.py).  Relative L2 is the metric, with room for one kink.
RTOL_GRAD_ORACLE_L2 = 5e-3   # relative L2 vs the oracle: float-rounding-level differences in the forward flip individual ReLU
                             # units (kinks); two builds of this library that agree with each other to 6e-7 sit at 2.0e-3 and 3.6e-3
                             # against the oracle on the H=4 / uniform configuration.  The reference goldens pin 5e-4 (max norm).
KINK_THR = 2e-5              # |fc1 pre-activation| below this on the oracle side: the ReLU decision could differ between the two
                             # implementations (their forwards agree to ~1e-6) - tests/test_gpu_full_size.py uses the same bound


def _near_kink_roots(ctx, R, K, thr=KINK_THR):
    """Roots whose computation tree (embedding_module.py:110-175 recursion, as cached by the oracle) holds a MergeLayer
    fc1 pre-activation within ``thr`` of zero.  Returns bool[R]."""
    bad = np.zeros(R, bool)

    def walk(c, owners):               # owners[i] = root that instance i of this context belongs to
        if c[0] == "leaf":
            return
        _, l, c_x, c_nb, cache, _, _ = c
        near = (np.abs(cache["z1"]) < thr).any(1)
        np.logical_or.at(bad, owners[near], True)
        walk(c_x, owners)
        walk(c_nb, np.repeat(owners, K))
    walk(ctx, np.arange(R))
    return bad


def _masked_bpr_backward(tgn, ref, emb, rse, rde, rne, B, K, n_neg=3):
    """BPR loss on both sides, its embedding gradient compared (2e-5 of its largest entry), then the backward of BOTH sides
    from its own gradient with the rows of near-kink roots zeroed: a ReLU unit whose pre-activation sits within fp32 noise of
    zero may take the other branch here than in the oracle, and one flipped unit moves every gradient below it by ~1/R
    (measured 1-2.5 % at R = 200, tools/probes/time_grad_error.py).  Such a root is left out ON BOTH SIDES instead of
    loosening the bound for the whole step; a step without one (most) is the plain ``loss.backward()``.
    Returns the oracle's parameter gradients; the product's are in ``p.grad``."""
    import torch
    import pfotgnrec_amd as P
    from oracle import tgn_oracle as T
    loss = P.bpr_loss(emb, B, n_neg)
    (d_emb,) = torch.autograd.grad(loss, emb, retain_graph=True)
    rl, cache = T.bpr_loss(rse, rde.reshape(B, 1, -1), rne.reshape(B, n_neg, -1))
    assert abs(float(loss) - float(rl)) < 1e-5
    ds, dp, dn = T.bpr_loss_backward(cache)
    W = np.concatenate([ds, dp.reshape(B, -1), dn.reshape(n_neg * B, -1)]).astype(np.float32)
    # main.py:321-337 backward; both sides start from their OWN embeddings (which agree to ~1e-6 relative)
    assert np.abs(d_emb.cpu().numpy() - W).max() <= 2e-5 * np.abs(W).max() + 1e-9
    R = W.shape[0]
    bad = _near_kink_roots(ref._ctx, R, K)
    assert bad.sum() < R // 2, bad.sum()
    keep = torch.from_numpy((~bad).astype(np.float32)).to(emb.device)[:, None]
    emb.backward(d_emb * keep)
    W[bad] = 0
    return ref.backward(W)


def _legal_draws(onf, roots, ts, K, L, raw):
    """Turns raw random integers into legal per-query positions, level by level, for both call conventions.

    Product order: one tensor per level (L, L-1, ..., 1), level l covering S_l.  Oracle order: the recursion's call
    order.  Levels are expanded with the oracle's own gather so both agree on the frontier.
    """
    nodes, tss = np.asarray(roots, np.int64), np.asarray(ts, np.float64)
    prod = []
    level_nodes = [(nodes, tss)]
    for i in range(L):
        n_, t_ = level_nodes[-1]
        cnt = np.array([len(onf.find_before(int(a), b)[0]) for a, b in zip(n_, t_)])
        dr = np.where(cnt[:, None] > 0, raw[i] % np.maximum(cnt, 1)[:, None], -1)
        prod.append(dr)
        nb, _, _ = onf.gather_uniform(n_, t_, np.maximum(dr, 0), K)
        level_nodes.append((np.concatenate([n_, nb.flatten()]), np.concatenate([t_, np.repeat(t_, K)])))
    # oracle recursion order for L layers: embed(l, S) = embed(l-1, S) ; sample(S) ; embed(l-1, nbrs(S))
    R = len(nodes)

    def rec(l, lo, hi, level):   # rows [lo, hi) of the product's level tensor `level` (0 = roots level)
        out = []
        if l == 0:
            return out
        out += rec(l - 1, lo, hi, level + 1) if level + 1 < L else []
        out.append(prod[level][lo:hi])
        if level + 1 < L:
            n_level = len(level_nodes[level][0])
            out += rec(l - 1, n_level + lo * K, n_level + hi * K, level + 1)
        return out
    return prod, rec(L, 0, R, 0)
